"""The two routes of the five batched after-solve calls (tqgpu_kkt_residual_batch, tqgpu_mpc_adjoint_batch, tqgpu_mpc_sensitivity_batch,
tqgpu_mpc_adjoint_matrices_batch, tqgpu_mpc_predict_batch) side by side on the smallest members that still have both sweeps and a second
level: one set of launches on the lead's stream against TREEQP_AMD_{KKT,ADJ,SENS}_BATCH=members (read by every call) on twin mirrors
stepped the same way.  Results bit for bit (np.uint64 views, no tolerance: each route is the other's reference), launches, copies and
waits of both routes against the figures of the library before the calls got one driver (COUNTS: measured with that commit's library on
these very sequences, which it passes).

Members: `chains`, two chains of three nodes with an input and a leaf (Nh = 3 levels of parents, nx = 2, nu = 1, different data);
`chain_tree`, such a chain and a tree of two levels of parents with two leaves (nk = 2, 1, 1, 0, 0), so that depth and the widths per
level differ between the members of one grid.  Roots are eliminated (nx0 = 2).

Left to the files that pin it in the same form already: each member against its single call and against the numpy references, the
steady-state counts behind tqgpu_mpc_step_batch, refusals leaving every member untouched (test_gpu_mpc_adjoint_batch.py,
test_gpu_mpc_sens_batch.py, test_gpu_mpc_adjoint_matrices.py, test_gpu_kkt_batch.py).  New here: the exact text of the refusal of a
mirror named twice and where `member i: ` stands in a member's refusal, on all four MPC calls; the KKT call taking a mirror named twice
member by member; a stored factor beside a missing one on members of different depth."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import mpc_cases as MC

pytestmark = pytest.mark.gpu

EINVAL = -2
NX0 = 2
SHAPES = {"chain": [1, 1, 1, 0], "tree": [2, 1, 1, 0, 0]}
PAIRS = {"chains": (("chain", 41), ("chain", 42)), "chain_tree": (("chain", 41), ("tree", 43))}

# (launches, copies, waits) of tqgpu_mpc_stats, for the KKT call (launches, copies, waits, batched members) of tqgpu_kkt_batch_stats
COUNTS = {
    ("adjoint", "chains", "batched"): (12, 3, 1),          # packing + (1 + 3) factor + (1 + 3 + 2 + 1) adjoint
    ("adjoint", "chains", "members"): (24, 4, 2),
    ("adjoint", "chain_tree", "batched"): (12, 3, 1),          # the grids of the deeper member
    ("adjoint", "chain_tree", "members"): (21, 4, 2),
    ("sensitivity", "chains", "batched"): (8, 2, 1),
    ("sensitivity", "chains", "members"): (16, 2, 2),
    ("sensitivity", "chain_tree", "batched"): (8, 2, 1),
    ("sensitivity", "chain_tree", "members"): (14, 2, 2),
    ("predictor", "chains", "batched"): (1, 1, 1, 1, 1, 1),          # without duals, then with
    ("predictor", "chains", "members"): (2, 0, 2, 2, 0, 2),
    ("predictor", "chain_tree", "batched"): (1, 1, 1, 1, 1, 1),
    ("predictor", "chain_tree", "members"): (2, 0, 2, 2, 0, 2),
    ("matrices", "chains", "batched"): (1, 2, 1),
    ("matrices", "chains", "members"): (2, 2, 2),
    ("matrices", "chain_tree", "batched"): (1, 2, 1),
    ("matrices", "chain_tree", "members"): (2, 2, 2),
    ("matrices_reduced", "chains", "batched"): (2, 2, 1),          # the sum over the members on the device
    ("matrices_reduced", "chains", "members"): (2, 2, 2),          # on the host, in member order
    ("kkt", "chains", "batched"): (3, 2, 1, 2),
    ("kkt", "chains", "members"): (6, 2, 3, 0),
    ("kkt", "chain_tree", "batched"): (3, 2, 1, 2),
    ("kkt", "chain_tree", "members"): (6, 2, 3, 0),
    ("kkt_named_twice", "chains", "batched"): (9, 3, 4, 0),          # three members, none batched, under either switch
    ("kkt_named_twice", "chains", "members"): (9, 3, 4, 0),
    ("kkt_named_twice", "chain_tree", "batched"): (9, 3, 4, 0),
    ("kkt_named_twice", "chain_tree", "members"): (9, 3, 4, 0),
    ("mixed_need", 1): (12, 3, 1),          # the chain's factor: packing + 1 + 3, and the adjoint's 7
    ("mixed_need", 0): (11, 3, 1),          # the tree's: packing + 1 + 2
}


def _case(shape, seed):
    nk = SHAPES[shape]
    return MC._case(f"{shape}{seed}", H.shaped_qp(nk, [0] + [2] * (len(nk) - 1), 1, seed).as_dict(), NX0, seed)


def _x0(seed):
    return MC.exact_x0s(NX0, seed)[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    """nested lists / dicts of arrays and numbers, bit for bit"""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b)), what


class _Members:
    """fresh mirrors of a pair, stepped once in one batch; `members`: the environment switch that sends every call member by member"""

    def __init__(self, capi, monkeypatch, pair, members=False, step=True):
        self.capi, self.gs = capi, []
        for var in ("TREEQP_AMD_KKT_BATCH", "TREEQP_AMD_ADJ_BATCH", "TREEQP_AMD_SENS_BATCH"):
            if members:
                monkeypatch.setenv(var, "members")
            else:
                monkeypatch.delenv(var, raising=False)
        self.cases = [_case(shape, seed) for shape, seed in PAIRS[pair]]
        self.x0s = [_x0(seed) for _, seed in PAIRS[pair]]

    def __enter__(self):
        for c in self.cases:
            self.gs.append(MC.make(self.capi, c))
        res, _ = self.capi.mpc_step_batch(self.gs, self.x0s)
        assert all(r["status"] == 0 for r in res)
        return self

    def __exit__(self, *exc):
        for g in self.gs:
            g.close()

    def ws(self, nw=2):
        rng = np.random.Generator(np.random.PCG64(7))
        return ([MC.quantised(rng, (int(g.sum_nx), nw), 1.0) for g in self.gs], [MC.quantised(rng, (int(g.sum_nu), nw), 1.0) for g in self.gs])

    def mpc(self):
        st = self.capi.mpc_stats()
        return st["launches"], st["copies"], st["waits"]

    def kkt(self):
        st = self.capi.kkt_batch_stats()
        return st["launches"], st["copies"], st["waits"], st["batched_members"]


def _adjoint(m):
    outs = m.capi.mpc_adjoint_batch(m.gs, *m.ws())
    return dict(out=outs, stored=[g.mpc_adjoint_grads() for g in m.gs]), m.mpc()


def _sensitivity(m):
    n_regs = m.capi.mpc_sensitivity_batch(m.gs)
    return dict(n_reg=n_regs, gain=[g.mpc_gain() for g in m.gs], all=[g.mpc_sensitivities() for g in m.gs]), m.mpc()


def _predictor(m):
    m.capi.mpc_sensitivity_batch(m.gs)
    x1s = [x0 + 2.0 ** -6 for x0 in m.x0s]
    plain = m.capi.mpc_predict_batch(m.gs, x1s)
    first = m.mpc()
    duals = m.capi.mpc_predict_batch(m.gs, x1s, duals=True)
    return dict(plain=plain, duals=duals), first + m.mpc()


def _matrices(m):
    m.capi.mpc_adjoint_batch(m.gs, *m.ws())
    for g in m.gs:
        g.mpc_set_param_groups()
    each = m.capi.mpc_adjoint_matrices_batch(m.gs)
    return dict(each=each), m.mpc()


def _matrices_reduced(m):
    m.capi.mpc_adjoint_batch(m.gs, *m.ws())
    for g in m.gs:
        g.mpc_set_param_groups()
    return dict(sum=m.capi.mpc_adjoint_matrices_batch(m.gs, reduce=True)), m.mpc()


def _kkt(m):
    return dict(res=m.capi.kkt_residual_batch(m.gs)), m.kkt()


def _kkt_named_twice(m):
    """not refused: the group goes member by member (no member of it through the batched kernels), with the results of the batched route"""
    twice = m.capi.kkt_residual_batch(m.gs + [m.gs[0]])
    _same(twice[2], twice[0], "the mirror named twice, both places")
    return dict(res=twice[:2]), m.kkt()


CALLS = {"adjoint": _adjoint, "sensitivity": _sensitivity, "predictor": _predictor, "matrices": _matrices, "matrices_reduced": _matrices_reduced,
         "kkt": _kkt, "kkt_named_twice": _kkt_named_twice}
ROWS = [(call, pair) for call in CALLS for pair in PAIRS if not (call == "matrices_reduced" and pair == "chain_tree")]          # reduce = 1 sums equal shapes


@pytest.mark.parametrize("call,pair", ROWS)
def test_both_routes_give_the_same_bits_at_the_counts_of_before(capi, monkeypatch, call, pair):
    got = {}
    for route in ("batched", "members"):
        with _Members(capi, monkeypatch, pair, members=route == "members") as m:
            got[route] = CALLS[call](m)
        print(f'    ("{call}", "{pair}", "{route}"): {got[route][1]},')
    _same(got["batched"][0], got["members"][0], f"{call}, {pair}: batched against members")
    if call == "kkt_named_twice":
        _same(got["batched"][0], _in_one(capi, monkeypatch, pair, _kkt)[0], f"{call}, {pair}: against the call without the second naming")
        assert got["batched"][1][3] == 0
    for route in got:
        assert got[route][1] == COUNTS[(call, pair, route)], (call, pair, route)


def _in_one(capi, monkeypatch, pair, fn):
    with _Members(capi, monkeypatch, pair) as m:
        return fn(m)


def test_a_stored_factor_beside_a_missing_one(capi, monkeypatch):
    """chain_tree, the tree's factor stored by a sensitivity of its own: the packing, k_sens_hess_batch and the factor levels go out for the
    chain alone (its three levels), the adjoint's sweeps over both; then with the chain's stored and the tree's missing (two levels)"""
    pair = "chain_tree"
    ref = _in_one(capi, monkeypatch, pair, _adjoint)[0]
    for stored in (1, 0):
        with _Members(capi, monkeypatch, pair) as m:
            m.gs[stored].mpc_sensitivity()
            gain = m.gs[stored].mpc_gain()
            got, counts = _adjoint(m)
            print(f'    ("mixed_need", {stored}): {counts},')
            _same(got, ref, f"member {stored}'s factor stored: against the batch that builds both")
            _same(m.gs[stored].mpc_gain(), gain, "the stored sensitivity behind the batch")
            assert counts == COUNTS[("mixed_need", stored)], stored
    assert COUNTS[("mixed_need", 1)][0] - COUNTS[("mixed_need", 0)][0] == 1          # the factor levels of the chain (3) against the tree's (2)


def test_refusal_texts(capi, monkeypatch):
    L = capi.lib()
    o = capi._gpu_opts(0)
    with _Members(capi, monkeypatch, "chains") as m:
        fresh = MC.make(capi, m.cases[1])          # has not solved
        try:
            m.capi.mpc_adjoint_batch(m.gs, *m.ws())
            m.capi.mpc_sensitivity_batch(m.gs)
            for g in m.gs:
                g.mpc_set_param_groups()

            def calls(mirrors):
                arr = (C.c_void_p * len(mirrors))(*[g.h for g in mirrors])
                n = len(mirrors)
                x = np.zeros(NX0 * n)
                return {"tqgpu_mpc_adjoint_batch": lambda: L.tqgpu_mpc_adjoint_batch(arr, n, C.byref(o), None, None, 1, None, None),
                        "tqgpu_mpc_sensitivity_batch": lambda: L.tqgpu_mpc_sensitivity_batch(arr, n, C.byref(o), None),
                        "tqgpu_mpc_adjoint_matrices_batch": lambda: L.tqgpu_mpc_adjoint_matrices_batch(arr, n, 0, *([None] * 7)),
                        "tqgpu_mpc_predict_batch": lambda: L.tqgpu_mpc_predict_batch(arr, n, x.ctypes.data_as(C.POINTER(C.c_double)), None, 0, None)}

            for who, call in calls(m.gs + [m.gs[0]]).items():
                assert call() == EINVAL and L.tqgpu_last_error().decode() == f"{who}: member 2: a mirror is named twice", who
            for who, call in calls([m.gs[0], fresh]).items():
                assert call() == EINVAL and L.tqgpu_last_error().decode().startswith(f"member 1: {who}: "), (who, L.tqgpu_last_error())
            arr = (C.c_void_p * 2)(m.gs[0].h, fresh.h)
            res = np.zeros(12)
            assert L.tqgpu_kkt_residual_batch(arr, 2, res.ctypes.data_as(C.POINTER(C.c_double)), None) == EINVAL
            assert L.tqgpu_last_error().decode() == "tqgpu_kkt_residual_batch: member 1 has not solved yet"
        finally:
            fresh.close()

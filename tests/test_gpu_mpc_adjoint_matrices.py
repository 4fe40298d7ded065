"""The adjoint of an MPC step in H, A, B on the device (tqgpu_mpc_set_param_groups, tqgpu_mpc_adjoint_matrices, tqgpu_mpc_adjoint_matrices_batch)
against adjmat_ref.outer evaluated at the device's own exported point, and against itself.

Cases: adjmat_cases.py.  Tolerances: 10 times the spread of the two numpy evaluations on the CPU (adjmat_cases.SPREAD), floor 1e-12.
Everything the call must leave alone, and everything the header promises bit for bit, is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import adj_ref as AR
import adjmat_cases as XC
import adjmat_ref as AM
import sens_cases as SN

pytestmark = pytest.mark.gpu

EINVAL = -2
NONE7 = (None,) * 7


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _same_dicts(a, b, what):
    for key in AM.KEYS:
        assert len(a[key]) == len(b[key]), (what, key)
        for g, (x, y) in enumerate(zip(a[key], b[key])):
            _same_bits(x, y, f"{what}: {key}[{g}]")


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


def _pad(capi, g):
    """the phantom root states the device counts (embedded x0-eliminated trees)"""
    g.mpc_set_param_groups(None, None)
    hd = np.zeros(5 * len(g.nk), dtype=np.int32)
    assert capi.lib().tqgpu_mpc_get_param_groups(g.h, None, None, hd.ctypes.data_as(C.POINTER(C.c_int)), None, None) == 0
    return int(hd[2])


def _ready(capi, cid, adjoint=True):
    """a mirror of the case, stepped, with its adjoint stored and its groups set -> (g, c, hgroup, cgroup (filled in), pad)"""
    k = XC.case(cid)
    c = k["c"]
    g = SN.make(capi, c)
    r, _ = g.mpc_step(c["x0"], **c["base"]["opts"])
    assert r["status"] == 0
    pad = _pad(capi, g)
    hg, cg = XC.maps(c, k["maps"], pad)
    g.mpc_set_param_groups(hg, cg)
    if adjoint:
        g.mpc_adjoint(*k["w"], **c["base"]["opts"])
    return g, c, XC.filled(c, hg, cg), pad


def _reference(g, c, w, maps, pad):
    sol = g.solution()
    b = AR.dual_form(c["d"], sol["x"], sol["u"], c["param"], w, c["kinds"])
    assert b["n_reg"] == 0
    return AM.outer(c["d"], sol["x"], sol["u"], sol["lam"], c["param"], b, c["kinds"], maps[0], maps[1], c["x0"], pad), sol


@pytest.mark.parametrize("cid", XC.CASE_IDS)
def test_against_the_outer_product_reference(capi, cid):
    g, c, maps, pad = _ready(capi, cid)
    try:
        got = g.mpc_adjoint_matrices()
        multi = any(len(m) > AM.CHUNK for grp in maps for m in AM.members(grp, AM.n_groups(grp)))
        assert _counts(capi) == (2 if multi else 1, 1, 1)
        ref, sol = _reference(g, c, XC.case(cid)["w"], maps, pad)
        for key in AM.KEYS:
            assert len(got[key]) == len(ref[key]), key
            for i, (x, y) in enumerate(zip(got[key], ref[key])):
                assert x.shape == y.shape, (key, i, x.shape, y.shape)
                err = float(np.max(np.abs(x - y))) if y.size else 0.0
                print(f"{cid} {key}[{i}]: |device - (b)| = {err:.3e}, tolerance {XC.tol(cid, key):.3e}")
                assert err <= XC.tol(cid, key), (key, i, err)
        # symmetric bit for bit; exactly 0.0 on the bounds of kind-0 nodes and on phantom states (per-node groups show single entries)
        for x in got["gH"]:
            if x.ndim == 3:
                _same_bits(x, np.transpose(x, (1, 0, 2)), f"{cid}: gH against its transpose")
        if XC.case(cid)["maps"] == "node":
            import sens_ref as SR
            on = SR.pinned(c["d"], sol["x"], sol["u"], c["kinds"])
            t = SR._assemble(c["d"], c["kinds"])
            hit = 0
            for k in range(t["Nn"]):
                front = pad if k == 0 else 0
                x = got["gH"][k]
                if x.ndim == 2:
                    assert np.all(x[:front] == 0.0) and np.all(x[front:][on[t["idx"][k]]] == 0.0), k
                    hit += int(on[t["idx"][k]].sum())
            assert hit > 0 or c["kinds"] is not None
    finally:
        g.close()


@pytest.mark.parametrize("tree", ["elim-three_children", "states-persist_c1", "elim-persist_c1", "elim-dense_kind1_root", "chain66"])
def test_shared_groups_are_the_sums_of_the_per_node_blocks(capi, tree):
    g, c, maps, pad = _ready(capi, tree + "|node")
    try:
        per = g.mpc_adjoint_matrices()
        name = "c65" if tree == "chain66" else "shared"
        hg, cg = XC.maps(c, name, pad)
        g.mpc_set_param_groups(hg, cg)
        sh = g.mpc_adjoint_matrices()
        for keys, grp, first in ((("gH", "gh"), hg, 0), (("gA", "gB", "gb"), cg, 1)):
            for gi, mem in enumerate(AM.members(grp, AM.n_groups(grp))):
                for key in keys:
                    want = sum(per[key][k - first] for k in mem)
                    assert float(np.max(np.abs(sh[key][gi] - want), initial=0.0)) <= XC.tol(tree, key), (key, gi)
        _same_dicts(dict(sh, gH=[], gh=[], gA=[], gB=[], gb=[]), dict(per, gH=[], gh=[], gA=[], gB=[], gb=[]), f"{tree}: the root terms")
    finally:
        g.close()


@pytest.mark.parametrize("cid", ["elim-persist_c1|shared", "states-generic|shared|w3", "chain66|c65", "elim-dense_kind1_root|node"])
def test_twice_the_same_bits_and_nothing_else_moves(capi, cid):
    g, c, _, _ = _ready(capi, cid)
    try:
        g.mpc_sensitivity(**c["base"]["opts"])
        g.mpc_adjoint(*XC.case(cid)["w"], **c["base"]["opts"])
        before = (g.solution(), g.kkt_residual(), g.mpc_adjoint_grads(), g.mpc_gain())
        one, two = g.mpc_adjoint_matrices(), g.mpc_adjoint_matrices()
        _same_dicts(one, two, cid)
        after = (g.solution(), g.kkt_residual(), g.mpc_adjoint_grads(), g.mpc_gain())
        for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
            _same_bits(after[0][k], before[0][k], f"{cid}: {k}")
        _same_bits(after[1]["res"], before[1]["res"], f"{cid}: the KKT residual")
        for k in ("gq", "gr", "gb"):
            _same_bits(after[2][k], before[2][k], f"{cid}: {k}")
        for i in range(3):
            _same_bits(after[3][i], before[3][i], f"{cid}: mpc_gain[{i}]")
        r1, u1 = g.mpc_step(c["x0"], **c["base"]["opts"])
    finally:
        g.close()
    g2, _, _, _ = _ready(capi, cid, adjoint=False)
    try:
        r2, u2 = g2.mpc_step(c["x0"], **c["base"]["opts"])
        assert r1["iter"] == r2["iter"]
        _same_bits(u1, u2, f"{cid}: u[0] of the next step")
    finally:
        g2.close()


def _batch(capi, cids):
    made = [_ready(capi, cid, adjoint=False) for cid in cids]
    gs = [m[0] for m in made]
    ws = [XC.case(cid)["w"] for cid in cids]
    capi.mpc_adjoint_batch(gs, [w[0] for w in ws], [w[1] for w in ws], **made[0][1]["base"]["opts"])
    return gs


@pytest.mark.parametrize("mode", ["batched", "members"])
def test_batch_without_reduction_is_the_single_calls(capi, monkeypatch, mode):
    if mode == "members":
        monkeypatch.setenv("TREEQP_AMD_ADJ_BATCH", "members")
    cids = ["elim-three_children|shared", "elim-single_wg|node", "chain66|c65", "elim-one_child|shared", "states-one_child|node"]          # depths 2, 2, 65, 2, 2
    for n in (2, 5):
        gs = _batch(capi, cids[:n])
        try:
            got = capi.mpc_adjoint_matrices_batch(gs, reduce=False)
            if mode == "batched":
                two = n == 5          # chain66 has groups of two chunks
                assert _counts(capi) == (2 if two else 1, 2, 1)
            for g, one in zip(gs, got):
                _same_dicts(one, g.mpc_adjoint_matrices(), f"{mode} n = {n}")
        finally:
            for g in gs:
                g.close()


@pytest.mark.parametrize("cid,single_chunk", [("elim-three_children|shared", True), ("elim-dense_kind1_root|shared", True), ("chain66|c65", False)])
def test_batch_with_reduction_is_the_host_sum_in_member_order(capi, monkeypatch, cid, single_chunk):
    for n in (2, 5):
        gs = _batch(capi, [cid] * n)
        try:
            # members differ: another loss gradient each
            for i, g in enumerate(gs):
                w = XC.case(cid)["w"]
                g.mpc_adjoint(w[0] * (1.0 + i), w[1] * (1.0 - 0.25 * i), **XC.case(cid)["c"]["base"]["opts"])
            each = capi.mpc_adjoint_matrices_batch(gs, reduce=False)
            red = capi.mpc_adjoint_matrices_batch(gs, reduce=True)
            assert _counts(capi) == (2, 2, 1)
            monkeypatch.setenv("TREEQP_AMD_ADJ_BATCH", "members")
            fall = capi.mpc_adjoint_matrices_batch(gs, reduce=True)
            monkeypatch.delenv("TREEQP_AMD_ADJ_BATCH")
            for key in AM.KEYS:
                for gi in range(len(red[key])):
                    want = each[0][key][gi].copy()
                    for m in range(1, n):
                        want = want + each[m][key][gi]
                    _same_bits(fall[key][gi], want, f"{cid}: {key}[{gi}], the fall-back")
                    if single_chunk:
                        _same_bits(red[key][gi], want, f"{cid}: {key}[{gi}]")
                    else:
                        assert float(np.max(np.abs(red[key][gi] - want), initial=0.0)) <= XC.tol(cid, key), (key, gi)
        finally:
            for g in gs:
                g.close()


def test_refusals_leave_outputs_and_state_alone(capi):
    L = capi.lib()
    cid = "elim-one_child|shared"
    c = XC.case(cid)["c"]
    g = SN.make(capi, c)
    other, _, _, _ = _ready(capi, "elim-three_children|shared")
    Nn = len(c["d"]["nk"])
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    buf = np.full(4096, 7.0)
    bp = buf.ctypes.data_as(C.POINTER(C.c_double))
    call = lambda h: L.tqgpu_mpc_adjoint_matrices(h, bp, bp, bp, bp, bp, bp, bp)
    try:
        assert call(g.h) == EINVAL and call(None) == EINVAL          # no adjoint, no solver
        g.mpc_step(c["x0"], **c["base"]["opts"])
        g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        assert call(g.h) == EINVAL and b"tqgpu_mpc_set_param_groups" in L.tqgpu_last_error()
        bad = np.zeros(Nn, dtype=np.int32)
        assert L.tqgpu_mpc_set_param_groups(g.h, ip(bad), None, 1, 0) == EINVAL and b"node 1" in L.tqgpu_last_error()          # nx differs from node 0's
        bad = np.full(Nn, -1, dtype=np.int32); bad[2] = 3
        assert L.tqgpu_mpc_set_param_groups(g.h, ip(bad), None, 2, 0) == EINVAL and b"node 2" in L.tqgpu_last_error()
        cgb = np.full(Nn, -1, dtype=np.int32); cgb[0] = 0
        assert L.tqgpu_mpc_set_param_groups(g.h, None, ip(cgb), 0, 1) == EINVAL and b"node 0" in L.tqgpu_last_error()
        gap = np.full(Nn, -1, dtype=np.int32); gap[1] = 1
        assert L.tqgpu_mpc_set_param_groups(g.h, ip(gap), None, 2, 0) == EINVAL and b"no member" in L.tqgpu_last_error()
        assert call(g.h) == EINVAL          # still no groups
        hg, cg = XC.maps(c, "shared", _pad(capi, g))
        g.mpc_set_param_groups(hg, cg)
        grads = g.mpc_adjoint_grads()
        arr = lambda hs: (C.c_void_p * len(hs))(*hs)
        bcall = lambda hs, n, red=0: L.tqgpu_mpc_adjoint_matrices_batch(arr(hs) if hs else None, n, red, bp, bp, bp, bp, bp, bp, bp)
        assert bcall([], 1) == EINVAL and bcall([g.h], 0) == EINVAL and bcall([g.h], 1, 2) == EINVAL
        assert bcall([g.h, g.h], 2) == EINVAL and b"member 1" in L.tqgpu_last_error() and b"twice" in L.tqgpu_last_error()
        assert bcall([g.h, other.h], 2, 1) == EINVAL and b"member 1" in L.tqgpu_last_error()          # unequal tables under reduce = 1
        fresh = SN.make(capi, c)
        assert bcall([g.h, fresh.h], 2) == EINVAL and b"member 1" in L.tqgpu_last_error()
        fresh.close()
        assert np.all(buf == 7.0)
        for k, v in g.mpc_adjoint_grads().items():
            _same_bits(v, grads[k], k)
        assert call(g.h) == 0 and not np.all(buf == 7.0)
        # whatever invalidates the stored adjoint
        for event in (lambda: g.mpc_step(c["x0"], **c["base"]["opts"]), lambda: g.set_linear_terms(c["d"]["q"], None), lambda: g.mpc_set_x0(c["x0"])):
            g.mpc_step(c["x0"], **c["base"]["opts"])
            g.mpc_adjoint(*c["w"], **c["base"]["opts"])
            assert call(g.h) == 0
            event()
            assert call(g.h) == EINVAL
    finally:
        g.close()
        other.close()


def test_a_group_that_has_come_to_mix_kinds_is_refused_at_the_call(capi):
    cid = "elim-dense_kind1_root|shared"
    g, c, _, _ = _ready(capi, cid)
    L = capi.lib()
    try:
        g.mpc_adjoint_matrices()
        mixed = XC.tree("mixed")
        g.upload_mixed(c["d"], mixed["kinds"], None)          # the leaves share an h-group and stay together: the maps survive
        g.mpc_step(c["x0"], **c["base"]["opts"])
        g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        out = g.mpc_adjoint_matrices()
        assert any(x.ndim == 2 for x in out["gH"]) and any(x.ndim == 3 for x in out["gH"])
        kinds = np.array(mixed["kinds"], copy=True)
        kinds[-1] = 1          # one leaf of the leaves' group back to kind 1
        g.upload_mixed(c["d"], kinds, None)
        g.mpc_step(c["x0"], **c["base"]["opts"])
        g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        assert L.tqgpu_mpc_adjoint_matrices(g.h, *NONE7) == EINVAL and b"mix kinds" in L.tqgpu_last_error()
        assert L.tqgpu_mpc_adjoint_matrices(g.h, *NONE7) == EINVAL
    finally:
        g.close()

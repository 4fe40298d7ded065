"""tqgpu_kkt_residual_batch on its batched route: the members of one device checked in one set of launches on the first member's
stream (k_export_*_batch, k_kkt_batch, k_kkt_max_batch; one descriptor per member, uploaded with every call).

The contract is equality with the single call: every comparison "batch against tqgpu_kkt_residual" is bit for bit on res and node
(NaN equals NaN), and every comparison against the numpy reference kkt_ref.residuals uses its derived bounds, as test_gpu_kkt.py
does.  Shapes are the smallest at which each part can go wrong: members of different Nn in one grid (4 .. 106 nodes), a node with
nu = 0, entries beyond one wave, kinds 0 / 1 / 2 / 3 with rows, phantom root states, one tree per solver route; 70 members cross
one wave of members; exits with status 1 and 2 and a member that exported ahead ride next to healthy members.

Members on two devices need a second GPU: the grouping by device is not covered here."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gen_cases as GC
import kkt_ref as K
import limit_shapes as LS
from helpers import product_qp_from_lti, with_dense_blocks
from limit_shapes import leaf
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
FULL = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)
CLIP4 = (3, 2, [(2, 1, [leaf(1)]), leaf(4)])          # root (3, 2); kids (2, 1) and (4, 0); a grandchild (1, 0) under the first kid
WAVE5 = (50, 30, [(70, 1, [leaf(2)]), (3, 2, [leaf(2)])])      # entries beyond one wave of 64 on a dense and on a clipping node
# per device group, whatever n: the packing (up to three launches), k_kkt_batch, k_kkt_max_batch; descriptors up, heads down; one wait
MAX_LAUNCHES, MAX_COPIES, MAX_WAITS = 5, 2, 1


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _clip_mirror(gpu, d, lam0=None):
    return gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d, lam0)


def _dense_mirror(gpu, d, kinds, lam0=None):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if "nc" in d:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    return g.upload_mixed(d, kinds, lam0)


def _agree(got, want, bound):
    got, want, bound = np.broadcast_arrays(np.asarray(got, float), np.asarray(want, float), np.asarray(bound, float))
    special = ~np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ok = np.where(special, (np.isnan(got) & np.isnan(want)) | (got == want), np.abs(got - want) <= np.where(special, 0.0, bound))
    return bool(np.all(ok))


def _check(got, ref, what):
    """device dict (with per_node) against the reference of the same point"""
    print(f"{what}: res {got['res']} node {got['node']}\n  ref {ref['res']} node {ref['node']}\n  bound {ref['bound']}")
    assert _agree(got["res"], ref["res"], ref["bound"]), what
    assert _agree(got["per_node"], ref["per_node"], ref["node_bound"]), what
    clear = K.node_is_clear(ref)
    assert np.array_equal(got["node"][clear], ref["node"][clear]), what
    assert np.array_equal(got["node"] < 0, ref["node"] < 0), what


def _same(a, b, what):
    """bit for bit on res and node; NaN equals NaN"""
    assert np.array_equal(a["res"], b["res"], equal_nan=True), f"{what}: res {a['res']} against {b['res']}"
    assert np.array_equal(a["node"], b["node"]), f"{what}: node {a['node']} against {b['node']}"


def _same_sol(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _batch_equals_singles(gpu, mirrors, what):
    """the batch call FIRST (the members' d_out is not packed yet), then each member's single call -> the batch's dicts"""
    batch = gpu.kkt_residual_batch(mirrors)
    for i, (m, b) in enumerate(zip(mirrors, batch)):
        _same(b, m.kkt_residual(), f"{what}: member {i}")
    return batch


def _agrees_with_reference(m, d, kinds, what):
    sol = m.solution()
    _check(m.kkt_residual(per_node=True), K.residuals(d, sol, kinds), what)


def _within_the_bound(st, n_batched):
    assert st["launches"] <= MAX_LAUNCHES and st["copies"] <= MAX_COPIES and st["waits"] <= MAX_WAITS, st
    assert st["batched_members"] == n_batched, st


# ---- 1. uneven members, every packing form ----

def _uneven_members(gpu):
    """[(name, mirror, d in kkt_ref's form, kinds, solve options)], one tree per solver route among them"""
    out = []
    d = K.random_problem(CLIP4, [0] * 4, 11)
    out.append(("clip4", _clip_mirror(gpu, d), d, [0] * 4, {}))
    kinds = [1, 0, 0, 0, 0]
    d = K.random_problem(WAVE5, kinds, 12)
    out.append(("wave5", _dense_mirror(gpu, d, kinds), d, kinds, {}))
    c = GC.case("mixed")
    g = _dense_mirror(gpu, c["d"], c["kinds"], GC.full_start("mixed")[0])
    assert g.plan["gen"] and g.plan["box"]
    out.append(("mixed", g, c["d"], c["kinds"], FULL))
    p = P.linear_chain(2, 5, 5)
    flat = product_qp_from_lti(gpu, p, eliminate_x0=True).flat()
    g = _clip_mirror(gpu, flat, p.lambda0)
    assert flat["nx"][0] == 0 and g.path == 2, (flat["nx"][0], g.path)          # embedded in the uniform tree: phantom root states
    out.append(("x0_elim", g, with_dense_blocks(flat), np.zeros(p.Nn, int), {}))
    d = LS.problem(LS.C, LS.case("g_persist_node_sizes-nz16")[1])
    g = _clip_mirror(gpu, d)
    assert g.path == 3
    out.append(("single_wg", g, with_dense_blocks(d), np.zeros(len(d["nk"]), int), {}))
    d = LS.problem(LS.C, LS.case("widest_level-w97")[1])
    g = _clip_mirror(gpu, d)
    assert g.path == 0 and g.plan["w3"] and len(d["nk"]) == 106
    out.append(("three_launch", g, with_dense_blocks(d), np.zeros(len(d["nk"]), int), {}))
    return out


def test_uneven_members_and_every_packing_form(gpu):
    mem = _uneven_members(gpu)
    try:
        for name, g, _, _, opts in mem:
            r = g.solve(**opts)
            print(f"{name}: {len(g.nk)} nodes, path {g.path}, status {r['status']}, {r['iter']} iterations")
        ms = [m[1] for m in mem]
        _batch_equals_singles(gpu, ms, "first composition")
        for name, g, d, kinds, _ in mem:
            _agrees_with_reference(g, d, kinds, name)
        # another composition (the descriptors must follow it), then the same again
        _batch_equals_singles(gpu, ms[::-1], "reverse order")
        _batch_equals_singles(gpu, ms[::-1], "reverse order again")
        st = gpu.kkt_batch_stats()
        print("stats, every stream drained:", st)
        _within_the_bound(st, len(ms))
        # a second solve of every member from other duals: the same descriptors, the current dual buffer may have changed
        for name, g, _, _, opts in mem:
            g.set_lambda(0.9 * g.solution()["lam"])
            r = g.solve(**opts)
            print(f"{name}, second solve: status {r['status']}, {r['iter']} iterations")
        _batch_equals_singles(gpu, ms[::-1], "after second solves")
        for name, g, d, kinds, _ in mem:
            _agrees_with_reference(g, d, kinds, name + ", second solve")
    finally:
        for m in mem:
            m[1].close()


# ---- 2. cost does not grow with n ----

def _clip4_mirrors(gpu, n):
    d = K.random_problem(CLIP4, [0] * 4, 11)
    return [_clip_mirror(gpu, d) for _ in range(n)]


def test_cost_does_not_grow_with_n(gpu, monkeypatch):
    stats, forced, values = {}, {}, {}
    for n in (1, 2, 5, 70):
        ms = _clip4_mirrors(gpu, n)
        try:
            assert all(r["status"] == 0 for r in gpu.solve_batch(ms))
            values[n] = gpu.kkt_residual_batch(ms)
            stats[n] = gpu.kkt_batch_stats()
            monkeypatch.setenv("TREEQP_AMD_KKT_BATCH", "members")
            by_member = gpu.kkt_residual_batch(ms)
            forced[n] = gpu.kkt_batch_stats()
            monkeypatch.delenv("TREEQP_AMD_KKT_BATCH")
            for i, (a, b) in enumerate(zip(values[n], by_member)):
                _same(a, b, f"n = {n}, member {i}: batched route against the per-member route")
                _same(a, values[n][0], f"n = {n}: member {i} against member 0 (mirrors of one problem)")
        finally:
            for m in ms:
                m.close()
        print(f"n = {n}: batched {stats[n]}, per member {forced[n]}")
    assert stats[1]["batched_members"] == 0
    for n in (2, 5, 70):
        _within_the_bound(stats[n], n)
        assert forced[n]["batched_members"] == 0
    assert {k: v for k, v in stats[70].items() if k != "batched_members"} == {k: v for k, v in stats[2].items() if k != "batched_members"}
    assert forced[2]["launches"] < forced[5]["launches"] < forced[70]["launches"]
    assert forced[70]["launches"] >= 3 * 70 and forced[70]["waits"] >= 70 and forced[70]["copies"] >= 70


# ---- 3. exits and flags per member ----

def test_exits_and_flags_per_member(gpu):
    d = K.random_problem(CLIP4, [0] * 4, 11)
    dn = {k: np.array(v, copy=True) for k, v in d.items()}
    dn["q"][1] = np.nan
    c = GC.case("mixed")
    lam0 = GC.full_start("mixed")[0]
    #      healthy            one iteration (status 1)                   healthy, dense       exported ahead         NaN in q             healthy
    ms = [_clip_mirror(gpu, d), _dense_mirror(gpu, c["d"], c["kinds"], lam0), _dense_mirror(gpu, c["d"], c["kinds"], lam0), _clip_mirror(gpu, d),
          _clip_mirror(gpu, dn), _clip_mirror(gpu, d)]
    try:
        ms[3].export_ahead(True)
        rs = [ms[0].solve(), ms[1].solve(**dict(FULL, maxIter=1)), ms[2].solve(**FULL), ms[3].solve(), ms[4].solve(), ms[5].solve()]
        print("status:", [r["status"] for r in rs])
        assert [r["status"] for r in rs] == [0, 1, 0, 0, 2, 0]
        batch = _batch_equals_singles(gpu, ms, "exits")
        assert np.isnan(batch[4]["res"]).any() and np.isnan(batch[4]["max"])
        for i in (0, 1, 2, 3, 5):
            assert np.isfinite(batch[i]["res"]).all(), f"member {i}: {batch[i]['res']}"
        _same(batch[0], batch[3], "the member that exported ahead against its healthy twin")
        _same(batch[0], batch[5], "the healthy members on either side of the NaN")
        _agrees_with_reference(ms[1], c["d"], c["kinds"], "status 1")
    finally:
        for m in ms:
            m.close()


# ---- 4. straight behind a batch launch ----

def _behind_a_batch_launch(gpu, make, **opts):
    ms, twins = [make(True) for _ in range(4)], [make(False) for _ in range(4)]
    try:
        rs = gpu.solve_batch(ms, **opts)
        batch = gpu.kkt_residual_batch(ms)
        st = gpu.kkt_batch_stats()
        print("behind the batch launch:", st, [(r["status"], r["iter"], r["n_launches"]) for r in rs])
        _within_the_bound(st, 4)
        assert all(m.plan["last_single_wg"] for m in ms), "the members did not share a launch"
        for i, t in enumerate(twins):
            rt = t.solve(**opts)
            assert (rt["status"], rt["iter"], rt["ls_total"], rt["n_launches"]) == (rs[i]["status"], rs[i]["iter"], rs[i]["ls_total"], rs[i]["n_launches"])
            _same(batch[i], t.kkt_residual(), f"member {i} against its twin solved and checked alone")
            _same_sol(ms[i].solution(), t.solution(), f"member {i}")
    finally:
        for m in ms + twins:
            m.close()
    return rs


def test_behind_a_single_workgroup_batch_launch(gpu):
    d = LS.problem(LS.C, LS.case("g_persist_node_sizes-nz16")[1])
    rs = _behind_a_batch_launch(gpu, lambda member: _clip_mirror(gpu, d))
    assert all(r["status"] == 0 for r in rs), rs


def test_behind_a_dense_batch_launch(gpu):
    c = GC.case("mixed")
    lam0 = GC.full_start("mixed")[0]

    def make(member):
        g = _dense_mirror(gpu, c["d"], c["kinds"], lam0)
        if member:
            g.set_dense_batch_launch(True)
            assert g.dense_batch_launch() == (1, 1)
        else:
            g.set_dense_single_launch(True)          # the launch a member of the dense batch launch is, on its own
        return g

    rs = _behind_a_batch_launch(gpu, make, **FULL)
    assert all(r["status"] == 0 for r in rs), rs


# ---- 5. rows redefined between checks ----

def test_rows_redefined_between_checks(gpu):
    c = GC.case("one_row")                      # three nodes, kinds 3, 1, 1; one row on the root (nx = 2, nu = 1)
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    assert list(d["nc"]) == [1, 0, 0] and (d["nx"][0], d["nu"][0]) == (2, 1)
    dc = K.random_problem(CLIP4, [0] * 4, 11)
    g, other = _dense_mirror(gpu, d, c["kinds"], GC.full_start("one_row")[0]), _clip_mirror(gpu, dc)
    try:
        assert g.solve(**FULL)["status"] == 0 and other.solve()["status"] == 0
        _batch_equals_singles(gpu, [other, g], "one row")
        _agrees_with_reference(g, d, c["kinds"], "one row")
        # two more rows, loose, under the old one: the row tables are allocated anew
        rng = np.random.Generator(np.random.PCG64(5))
        d["C"] = np.vstack([d["C"].reshape(1, 2), rng.standard_normal((2, 2))]).flatten(order="F")
        d["D"] = np.vstack([d["D"].reshape(1, 1), rng.standard_normal((2, 1))]).flatten(order="F")
        d["dmin"], d["dmax"] = np.concatenate([d["dmin"], [-50.0, -50.0]]), np.concatenate([d["dmax"], [50.0, 50.0]])
        d["nc"] = np.array([3, 0, 0], np.int32)
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        assert g.sum_nc == 3
        r = g.solve(**FULL)
        print("three rows:", r)
        batch = _batch_equals_singles(gpu, [other, g], "three rows")
        assert batch[1]["node"][K.GFEAS] == 0
        _agrees_with_reference(g, d, c["kinds"], "three rows")
    finally:
        g.close(); other.close()


# ---- 6. the check leaves the solver alone ----

def test_the_check_leaves_the_solver_alone(gpu):
    c = GC.case("mixed")
    lam0 = GC.full_start("mixed")[0]
    dc = K.random_problem(CLIP4, [0] * 4, 11)
    dw = LS.problem(LS.C, LS.case("g_persist_node_sizes-nz16")[1])

    def make():
        return [_dense_mirror(gpu, c["d"], c["kinds"], lam0), _clip_mirror(gpu, dc), _clip_mirror(gpu, dw), _clip_mirror(gpu, dw)]

    a, b = make(), make()
    key = lambda r: (r["status"], r["iter"], r["ls_total"])
    try:
        ra, rb = gpu.solve_batch(a, **FULL), gpu.solve_batch(b, **FULL)
        assert [key(r) for r in ra] == [key(r) for r in rb]
        gpu.kkt_residual_batch(b)
        assert gpu.kkt_batch_stats()["batched_members"] == 4
        for i, (ma, mb) in enumerate(zip(a, b)):
            _same_sol(ma.solution(), mb.solution(), f"member {i} after the check")          # (with mu_d where the mirror has rows)
        gpu.kkt_residual_batch(b)
        ra2, rb2 = gpu.solve_batch(a, **FULL), gpu.solve_batch(b, **FULL)
        assert [key(r) for r in ra2] == [key(r) for r in rb2]
        for i, (ma, mb) in enumerate(zip(a, b)):
            _same_sol(ma.solution(), mb.solution(), f"member {i}, next solve")
        sta, stb = a[0].stage_steps(), b[0].stage_steps()
        assert np.array_equal(sta["last"], stb["last"]) and np.array_equal(sta["total"], stb["total"])
    finally:
        for m in a + b:
            m.close()


# ---- 7. refusals unchanged ----

def test_refusals_unchanged(gpu):
    L = gpu.lib()
    d = K.random_problem(CLIP4, [0] * 4, 17)
    ms = [_clip_mirror(gpu, d) for _ in range(3)]
    p = P.linear_chain(2, 6, 6)
    rank = _clip_mirror(gpu, product_qp_from_lti(gpu, p).flat(), p.lambda0).pshard_init(0, 2)
    res, node = (C.c_double * 18)(), (C.c_int * 18)()
    try:
        ms[0].solve(); ms[2].solve()
        before = [ms[0].kkt_residual(), ms[2].kkt_residual()]
        arr = (C.c_void_p * 3)(*[m.h for m in ms])
        assert L.tqgpu_kkt_residual_batch(arr, 3, res, node) == EINVAL
        assert b"tqgpu_kkt_residual_batch: member 1 has not solved yet" in L.tqgpu_last_error()
        arr = (C.c_void_p * 3)(ms[0].h, rank.h, ms[2].h)
        assert L.tqgpu_kkt_residual_batch(arr, 3, res, node) == EUNSUPPORTED
        assert b"tqgpu_kkt_residual_batch: this mirror is rank 0 of a sharded solve" in L.tqgpu_last_error()
        arr = (C.c_void_p * 3)(ms[0].h, None, ms[2].h)
        assert L.tqgpu_kkt_residual_batch(arr, 3, res, node) == EINVAL and b"null solver" in L.tqgpu_last_error()
        arr = (C.c_void_p * 2)(ms[0].h, ms[2].h)
        assert L.tqgpu_kkt_residual_batch(None, 2, res, node) == EINVAL and b"bad arguments" in L.tqgpu_last_error()
        assert L.tqgpu_kkt_residual_batch(arr, 2, None, node) == EINVAL and b"bad arguments" in L.tqgpu_last_error()
        assert L.tqgpu_kkt_residual_batch(arr, -1, res, node) == EINVAL
        assert L.tqgpu_kkt_residual_batch(arr, 0, None, None) == 0
        after = [ms[0].kkt_residual(), ms[2].kkt_residual()]
        for i in range(2):
            _same(before[i], after[i], f"member {i} after the refused calls")
        assert L.tqgpu_kkt_residual_batch(arr, 2, res, None) == 0          # node may be NULL
        assert list(res[:6]) == list(before[0]["res"]) and list(res[6:12]) == list(before[1]["res"])
        assert gpu.kkt_batch_stats()["batched_members"] == 2
        assert L.tqgpu_kkt_batch_stats(None, None, None, None) == 0
    finally:
        for m in ms:
            m.close()
        rank.close()

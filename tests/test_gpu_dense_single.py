"""The opt-in single-launch route of trees with dense stage QPs (tqgpu_set_dense_single_launch: g_persist_dense, the whole solve
as one launch of one workgroup with the dense-unconstrained branch, stage_box and stage_gen compiled in), on the rows of
box_cases.py and gen_cases.py.

1.  without the opt-in nothing moves: setting 0, plan bit clear, route 0, the launches of a fresh mirror;
2.  with it an eligible tree takes route 3, sets both plan bits and launches what a clipping tree of the same shape launches;
3.  one iteration is the numpy reference's step (the assertions of test_gpu_box_step.py / test_gpu_gen_step.py), for a tree of
    each kind and for the mixed trees;
4.  whole solves agree with the default route of a second mirror: same verdict, iterations and trials, solution to 1e-10;
5.  both sides of the window limit: stage_waves from the getter is the LDS arithmetic of the header comment (16 on small nodes,
    fewer on the nz = 64 and nc = 64 rows), and a tree too wide for one workgroup stays on the default route;
6.  status 4 ends the solve inside the launch and leaves the mirror usable;
7.  hot equals cold bit for bit, repeated solves are bit-identical, the hot start saves active-set steps;
8.  a MAXIMUM_ITERATIONS exit exports what the default route exports;
9.  the option can be switched between the solves of one mirror;
10. a member of a batch stays on the launch-per-phase route.

Tolerances.  Against the numpy references: 1e-10, under the guards of the case tables (cond <= 1e6, strict complementarity 1e-6),
as in the step tests of the default route.  Between the two routes: 1e-10, the project's parity tolerance for routes that share
their bodies and differ in the order of the workgroup's sums; every whole solve compared starts from a clear_start, from which
every Armijo and termination decision keeps its distance from rounding."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import box_cases as BC
import gen_cases as GC
import gen_ref as G
import newton_ref as N
from helpers import rel_err
from limit_shapes import leaf

pytestmark = pytest.mark.gpu

TOL = 1e-10
STEP = dict(maxIter=1, regType=0)
FULL = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)
BETA = GC.BETA
STAGE_QP_SOLVE_FAILED = 4
BIT_DENSE_SINGLE, BIT_LAST_SINGLE = 1 << 19, 1 << 17
BUDGET = 150 * 1024


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _mirror(gpu, d, kinds, lam0=None, single=False, hot=None):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if "nc" in d:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    g.upload_mixed(d, kinds, lam0)
    if hot is not None:
        g.set_gen_hot_start(hot)
    if single:
        g.set_dense_single_launch(True)
    return g


def _flags(gpu, g):
    import ctypes as C
    f = C.c_uint()
    g._chk(gpu.lib().tqgpu_debug_plan(g.h, C.byref(f), None))
    return f.value


def _key(r):
    return r["status"], r["iter"], r["ls_total"]


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}{k}: differs by {np.max(np.abs(a[k] - b[k])):.3e}"


def _close(a, b, what, keys=("x", "u", "lam", "mu_x", "mu_u", "mu_d")):
    errs = {k: rel_err(a[k], b[k]) for k in keys if k in a}
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL, what


def _box(rid):
    c = BC.case(rid)
    return c["d"], c["kinds"]


def _gen(rid):
    c = GC.case(rid)
    return c["d"], c["kinds"]


def _loose(rid, as_box):
    """gen_cases.loose_case(rid): (d, kinds, clear start); as_box: the same tree with its kind-3 nodes as kind 2 (the box row)"""
    d, kinds, _, start = GC.loose_case(rid)
    if as_box:
        d = {k: v for k, v in d.items() if k not in ("nc", "C", "D", "dmin", "dmax")}
        kinds = G._kinds2(kinds)
    return d, kinds, start


@functools.lru_cache(maxsize=None)
def _kind1_case():
    """a three-node tree of dense unconstrained nodes (kind 1) with its reference step at seeded duals"""
    shape, kinds = (3, 2, [leaf(2), leaf(3)]), np.array([1, 1, 1], np.int32)
    d = BC.base_problem(shape, kinds, 5)
    lam0 = N.seeded_duals(5, 0)
    BC.draw_bounds(d, kinds, lam0, BC.frac(0.0), 5)
    ref = N.newton_step(d, lam0, kinds=kinds)
    trials, slack = N.armijo_trials(d, lam0, ref["dlam"], ref["res"], BC.LsOpts, kinds)
    lam1 = lam0 + BETA ** (trials - 1) * ref["dlam"]
    assert ref["cond"] <= BC.COND_MAX and slack >= BC.SLACK_MIN
    return dict(d=d, kinds=kinds, lam0=lam0, ref=ref, trials=trials, slack=slack, st1=N.stage_solutions(d, lam1, kinds=kinds), xu_pin=True)


def expected_stage_waves(d, kinds):
    """the LDS arithmetic of include/treeqp_amd.h: a stage window of the tree's largest need (head, + 2 nz^2 on a kind-2 node,
    + nc + 2 nz^2 + nz nc + nc^2 on a kind-3 node with rows; head = children's nx + nx + 2 nz + 2; rounded up to an even number of
    doubles), the largest count <= 16 whose windows stay within 150 KiB next to the index tables ((13 (Nn + 3)) / 2 + 16 doubles
    and 8 spare)"""
    nk, nx, nu = (np.asarray(d[k], int) for k in ("nk", "nx", "nu"))
    nc = np.asarray(d["nc"], int) if "nc" in d else np.zeros(len(nk), int)
    kid0 = np.concatenate([[1], 1 + np.cumsum(nk)[:-1]])
    win = 0
    for k in range(len(nk)):
        nz = nx[k] + nu[k]
        need = int(nx[kid0[k]:kid0[k] + nk[k]].sum()) + nx[k] + 2 * nz + 2
        if kinds[k] == 3 and nc[k] > 0 and nz > 0:
            need += nc[k] + 2 * nz * nz + nz * nc[k] + nc[k] * nc[k]
        elif kinds[k] >= 2:
            need += 2 * nz * nz
        win = max(win, need)
    win += win & 1
    tables = (13 * (len(nk) + 3)) // 2 + 16
    fits = [w for w in range(1, 17) if (win * w + tables + 8) * 8 <= BUDGET]
    return max(fits) if fits else 0


# ------------------------------------------------------------------------------------------------------------------------------
# 1, 2. the default is untouched; the route with the opt-in
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,rid", [("box", "mixed"), ("gen", "mixed")])
def test_default_is_untouched(gpu, src, rid):
    d, kinds = _box(rid) if src == "box" else _gen(rid)
    a, b = _mirror(gpu, d, kinds), _mirror(gpu, d, kinds)
    try:
        on, eligible, waves = a.dense_single_launch
        assert on == 0 and eligible == 1 and waves >= 1
        assert not _flags(gpu, a) & BIT_DENSE_SINGLE and a.path == 0 and not a.plan["dense_single_wg"]
        ra, rb = a.solve(**FULL), b.solve(**FULL)
        assert not _flags(gpu, a) & (BIT_DENSE_SINGLE | BIT_LAST_SINGLE)
    finally:
        a.close(); b.close()
    assert _key(ra) == _key(rb) and ra["n_launches"] == rb["n_launches"] and ra["n_launches"] > 2


@pytest.mark.parametrize("src,rid", [("box", "nz2"), ("box", "mixed"), ("gen", "one_row"), ("gen", "mixed"), ("gen", "nc64")])
def test_route_with_the_opt_in(gpu, src, rid):
    d, kinds = _box(rid) if src == "box" else _gen(rid)
    g = _mirror(gpu, d, kinds, single=True)
    clip = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    try:
        assert g.dense_single_launch[:2] == (1, 1)
        assert g.path == 3
        if rid == "mixed":
            assert clip.path == 3, "the clipping tree of this shape does not run g_persist"
        assert _flags(gpu, g) & BIT_DENSE_SINGLE and not _flags(gpu, g) & BIT_LAST_SINGLE
        g.solve(**FULL)                      # (the first solve of a dense mirror also launches k_dense_init)
        r = g.solve(**FULL)
        rc = clip.solve()
        f = _flags(gpu, g)
        assert f & BIT_DENSE_SINGLE and f & BIT_LAST_SINGLE and g.plan["dense_single_wg"] and g.plan["last_single_wg"]
    finally:
        g.close(); clip.close()
    assert r["n_launches"] == 1
    if rid == "mixed":
        assert rc["n_launches"] == r["n_launches"]


# ------------------------------------------------------------------------------------------------------------------------------
# 3. one iteration against the numpy references
# ------------------------------------------------------------------------------------------------------------------------------

STEP_ROWS = [("kind1", "kind1"), ("box", "nz2"), ("box", "nz64"), ("box", "mixed"), ("box", "x0_eliminated"), ("box", "equal_bounds"),
             ("gen", "one_row"), ("gen", "swap"), ("gen", "nz64"), ("gen", "nc64"), ("gen", "mixed"), ("gen", "x0_elim")]


def _check_step(gpu, src, rid):
    c = _kind1_case() if src == "kind1" else (BC.case(rid) if src == "box" else GC.case(rid))
    ref, d, kinds = c["ref"], c["d"], c["kinds"]
    g = _mirror(gpu, d, kinds, c["lam0"], single=True)
    try:
        assert g.dense_single_launch[:2] == (1, 1), "the row is not eligible for the single launch"
        r = g.solve(**STEP)
        sol = g.solution()
        assert _flags(gpu, g) & BIT_LAST_SINGLE
    finally:
        g.close()
    tau = BETA ** (r["ls_total"] - 1)
    e_d, e_l = rel_err(sol["dlam"], ref["dlam"]), rel_err(sol["lam"], c["lam0"] + tau * ref["dlam"])
    print(f"{src}/{rid}: {_key(r)} reference trials {c['trials']} slack {c['slack']:.2e} dlam {e_d:.2e} lam {e_l:.2e}")
    assert (r["status"], r["iter"]) == (1, 1) and r["n_launches"] == 2          # k_dense_init + the solve
    assert e_d <= TOL and e_l <= TOL
    if src == "gen" or c["slack"] >= BC.SLACK_MIN:
        assert c["slack"] >= BC.SLACK_MIN and r["ls_total"] == c["trials"]
    if src == "gen":
        assert c["xu_pin"]
    if c["xu_pin"]:
        st1 = c["st1"]
        x, u, sx, su = N.flat_xu(st1)
        errs = dict(x=rel_err(sol["x"], x), u=rel_err(sol["u"], u))
        if src == "gen":
            mx, mu, md = G.flat_multipliers(d, st1, h_stage=ref["stages"]["h"])
            errs.update(mu_x=rel_err(sol["mu_x"], mx), mu_u=rel_err(sol["mu_u"], mu), mu_d=rel_err(sol["mu_d"], md))
            assert np.array_equal(sol["mu_d"] != 0, np.concatenate(st1["rside"]) != 0), "the device's working set of rows is not the reference's"
        print(f"{src}/{rid}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= TOL
        assert np.array_equal(sol["x"][sx != 0], x[sx != 0]) and np.array_equal(sol["u"][su != 0], u[su != 0])
    return sol


@pytest.mark.parametrize("src,rid", STEP_ROWS)
def test_one_iteration_is_the_reference_step(gpu, src, rid):
    _check_step(gpu, src, rid)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. whole solves against the default route
# ------------------------------------------------------------------------------------------------------------------------------

def _check_whole(gpu, d, kinds, start, what, opts=FULL, want_status=0):
    a, b = _mirror(gpu, d, kinds, start, single=True), _mirror(gpu, d, kinds, start)
    try:
        ra = a.solve(**opts); sa = a.solution()
        rb = b.solve(**opts); sb = b.solution()
        assert _flags(gpu, a) & BIT_LAST_SINGLE and not _flags(gpu, b) & BIT_LAST_SINGLE
    finally:
        a.close(); b.close()
    print(f"{what}: single launch {_key(ra)} in {ra['n_launches']} launches, default route {_key(rb)} in {rb['n_launches']}")
    assert _key(ra) == _key(rb) and ra["status"] == want_status
    _close(sa, sb, what)
    return ra, rb


@pytest.mark.parametrize("as_box", [False, True], ids=["gen", "box"])
@pytest.mark.parametrize("rid", ["one_row", "nc64", "nz64", "mixed"])
def test_whole_solve_is_the_default_routes(gpu, rid, as_box):
    d, kinds, start = _loose(rid, as_box)
    _check_whole(gpu, d, kinds, start, f"{rid}/{'box' if as_box else 'gen'}")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. both sides of the window limit
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,rid,full", [("gen", "one_row", True), ("box", "nz2", True), ("box", "nz64", False), ("gen", "nz64", False), ("gen", "nc64", False)])
def test_stage_waves_is_the_lds_arithmetic(gpu, src, rid, full):
    d, kinds = _box(rid) if src == "box" else _gen(rid)
    want = expected_stage_waves(d, kinds)
    g = _mirror(gpu, d, kinds, single=True)
    try:
        on, eligible, waves = g.dense_single_launch
    finally:
        g.close()
    print(f"{src}/{rid}: stage_waves {waves}, arithmetic {want}")
    assert (on, eligible) == (1, 1) and waves == want
    assert waves == 16 if full else 1 <= waves < 16
    # (the step and the whole solve of these rows on this route: STEP_ROWS and test_whole_solve_is_the_default_routes above)
    assert (src, rid) in STEP_ROWS


def test_a_tree_too_wide_for_one_workgroup_keeps_the_default_route(gpu):
    shape = (2, 1, [(2, 1, [leaf(2)] * 10)] * 10)          # a level of 100 nodes: more than the 6 x 16 one workgroup takes
    kinds = np.array([2] * 11 + [1] * 100, np.int32)
    d = BC.base_problem(shape, kinds, 5)
    BC.draw_bounds(d, kinds, np.zeros(2 * 110), BC.frac(0.25), 5)
    a, b = _mirror(gpu, d, kinds, single=True), _mirror(gpu, d, kinds)
    try:
        assert a.dense_single_launch == (1, 0, 0) and a.path == 0 and not _flags(gpu, a) & BIT_DENSE_SINGLE
        ra = a.solve(**FULL); sa = a.solution()
        rb = b.solve(**FULL); sb = b.solution()
        assert not _flags(gpu, a) & BIT_LAST_SINGLE
    finally:
        a.close(); b.close()
    assert _key(ra) == _key(rb) and ra["n_launches"] == rb["n_launches"]
    _same(sa, sb, "wide tree: ")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. status 4
# ------------------------------------------------------------------------------------------------------------------------------

def test_infeasible_stage_qp_ends_with_status_4(gpu):
    bad, good, kinds = GC.infeasible_pair()
    opts = dict(stationarityTolerance=GC.FULL_TOL)
    g = _mirror(gpu, bad, kinds, single=True)
    f = None
    try:
        r = g.solve(**opts)
        assert r["status"] == STAGE_QP_SOLVE_FAILED and _flags(gpu, g) & BIT_LAST_SINGLE
        g.set_constraints(None, None, None, good["dmin"], good["dmax"])
        r2 = g.solve(**opts); s2 = g.solution()
        f = _mirror(gpu, good, kinds, single=True)
        rf = f.solve(**opts); sf = f.solution()
    finally:
        g.close()
        if f is not None:
            f.close()
    assert _key(r2) == _key(rf) and rf["status"] == 0
    _same(s2, sf)
    assert s2["x"][0] + s2["u"][0] >= 1.5 - 1e-12 and s2["mu_d"][0] < 0


def test_indefinite_stage_hessian_ends_with_status_4(gpu):
    bad, good, kinds = BC.indefinite_pair()
    opts = dict(stationarityTolerance=1e-10)
    g, p = _mirror(gpu, bad, kinds, single=True), _mirror(gpu, bad, kinds)
    f = None
    try:
        r = g.solve(**opts); rp = p.solve(**opts)
        assert r["status"] == STAGE_QP_SOLVE_FAILED and _flags(gpu, g) & BIT_LAST_SINGLE
        assert _key(r) == _key(rp), "the verdict of the failed solve is not the launch-per-phase route's"
        g.upload_mixed(good, kinds)
        r2 = g.solve(**opts); s2 = g.solution()
        f = _mirror(gpu, good, kinds, single=True)
        rf = f.solve(**opts); sf = f.solution()
    finally:
        g.close(); p.close()
        if f is not None:
            f.close()
    assert _key(r2) == _key(rf) and rf["status"] == 0
    _same(s2, sf)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. hot start
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rid", ["one_row", "swap", "nc64", "mixed"])
def test_hot_equals_cold_and_repeats(gpu, rid):
    c = GC.case(rid)
    start = GC.clear_start(c["d"], c["kinds"])[0]
    hot, cold = _mirror(gpu, c["d"], c["kinds"], start, single=True), _mirror(gpu, c["d"], c["kinds"], start, single=True, hot=False)
    try:
        rh = hot.solve(**FULL); sh = hot.solution(); nh = hot.stage_steps()["total"].sum()
        rc = cold.solve(**FULL); sc = cold.solution(); nc = cold.stage_steps()["total"].sum()
        rh2 = hot.solve(**FULL); sh2 = hot.solution(); nh2 = hot.stage_steps()["total"].sum()
        assert _flags(gpu, hot) & BIT_LAST_SINGLE and _flags(gpu, cold) & BIT_LAST_SINGLE
    finally:
        hot.close(); cold.close()
    print(f"{rid}: {_key(rh)}, steps of the hot solve {nh}, repeated {nh2}, of the cold solve {nc}")
    assert _key(rh) == _key(rc) == _key(rh2) and rh["status"] == 0
    _same(sh, sc, "hot against cold: ")
    _same(sh, sh2, "repeated: ")
    assert 0 < nh2 <= nh <= nc


# ------------------------------------------------------------------------------------------------------------------------------
# 8. MAXIMUM_ITERATIONS
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,rid", [("box", "mixed"), ("gen", "mixed"), ("gen", "one_row")])
def test_maximum_iterations_exit(gpu, src, rid):
    if src == "box":
        d, kinds, start = _loose(rid, True)
    else:
        d, kinds = _gen(rid)
        start = GC.clear_start(d, kinds)[0]
    ra, _ = _check_whole(gpu, d, kinds, start, f"{src}/{rid} capped", opts=dict(FULL, maxIter=1), want_status=1)
    assert ra["iter"] == 1


# ------------------------------------------------------------------------------------------------------------------------------
# 9, 10. switching the option; batches
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rid", ["one_row", "mixed"])
def test_switching_between_solves(gpu, rid):
    c = GC.case(rid)
    start = GC.clear_start(c["d"], c["kinds"])[0]
    g = _mirror(gpu, c["d"], c["kinds"], start)
    try:
        g.solve(**FULL)                       # (k_dense_init, and the launch-per-phase route learns its chunk)
        r0 = g.solve(**FULL); s0 = g.solution(); f0 = _flags(gpu, g)
        g.set_dense_single_launch(True)
        r1 = g.solve(**FULL); s1 = g.solution(); f1 = _flags(gpu, g)
        g.set_dense_single_launch(False)
        r2 = g.solve(**FULL); s2 = g.solution(); f2 = _flags(gpu, g)
    finally:
        g.close()
    assert _key(r0) == _key(r1) == _key(r2) and r0["status"] == 0
    assert not f0 & BIT_LAST_SINGLE and f1 & BIT_LAST_SINGLE and not f2 & BIT_LAST_SINGLE and f0 == f2
    assert r1["n_launches"] == 1 and r2["n_launches"] == r0["n_launches"] > 1
    _close(s1, s0, f"{rid}: on against off")
    _close(s2, s0, f"{rid}: off again")


def test_batch_member_stays_on_the_launch_per_phase_route(gpu):
    c = GC.case("mixed")
    d, kinds = c["d"], c["kinds"]
    start = GC.clear_start(d, kinds)[0]
    b0, b1 = _mirror(gpu, d, kinds, start, single=True), _mirror(gpu, d, kinds, c["lam0"], single=True)
    a0, a1 = _mirror(gpu, d, kinds, start), _mirror(gpu, d, kinds, c["lam0"])
    try:
        rb = gpu.solve_batch([b0, b1], **FULL)
        sb = [b0.solution(), b1.solution()]
        fb = [_flags(gpu, b0), _flags(gpu, b1)]
        ra = [a0.solve(**FULL), a1.solve(**FULL)]
        sa = [a0.solution(), a1.solution()]
    finally:
        for m in (b0, b1, a0, a1):
            m.close()
    for i in range(2):
        assert fb[i] & BIT_DENSE_SINGLE and not fb[i] & BIT_LAST_SINGLE
        assert _key(rb[i]) == _key(ra[i])
        _same(sb[i], sa[i], f"member {i}: ")

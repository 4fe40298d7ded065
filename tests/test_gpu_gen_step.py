"""The stage solver for general constraints of the device (kind 3 of tqgpu_set_objective_mixed with the rows of
tqgpu_set_constraints: k_stage_gen / stage_gen, k_dense_init, k_export_gen) pinned per operation to the numpy reference of
gen_ref.py, on the rows of gen_cases.py.  The pattern is test_gpu_box_step.py's.

a. one iteration from the row's lambda0 without regularisation: dlam is the reference's Newton step (which rests on every node's
   elimination matrix of its final working set), lambda is lambda0 + tau dlam, x, u are the reference's stage solutions at the new
   lambda with the entries on a bound bit for bit, the trial count is the reference's line search; mu_d is the reference's on the
   reference's working set (zero elsewhere, exactly), mu_x / mu_u are h - H z - G'mu_d with the h of phase S and the z, mu_d of
   the accepted trial on every entry (the pairing of a MAXIMUM_ITERATIONS exit, as k_export_box);
b. a repeated solve, a solve on a fresh mirror and a member of a batch are bit-identical;
c. rows that are loose by construction give what the same tree gives with those nodes as kind 2;
d. an infeasible stage QP ends the solve with status 4 and leaves the mirror usable;
e. refusals and the plan bits.

Tolerances: 1e-10 on the step, lambda, x, u and the multipliers (every row has cond(M) <= 1e6, cond(S) <= 1e6 and strict
complementarity 1e-6: the tolerance and the guards of test_gpu_box_step.py); 1e-12 between a tree with loose rows and the same tree
without (two factorisations of the same H_FF in another order of operations, on nodes of cond(H) ~ 1e2)."""
from __future__ import annotations

import numpy as np
import pytest

import box_cases as BC
import gen_cases as GC
import gen_ref as G
import newton_ref as N
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
STEP = dict(maxIter=1, regType=0)
BETA = GC.BETA
KEYS = ("x", "u", "lam", "mu_x", "mu_u", "mu_d", "dlam")
EINVAL, EUNSUPPORTED = -2, -4
STAGE_QP_SOLVE_FAILED = 4
# tqgpu_debug_plan of row_and_bound's tree (two nodes, nx 3 and 2: no uniform-tree kernel) with its root as a kind-2 node, before a
# solve: fuse | gpersist | gp_state_lds | gp_const_lds | gp_small16 | gp_small8 (all decided at create) | dense | box
PLAN_BOX_TREE = (1 << 6) | (1 << 9) | (1 << 10) | (1 << 11) | (1 << 13) | (1 << 14) | (1 << 15) | (1 << 16)


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _mirror(gpu, d, kinds, lam0=None):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    return g.upload_mixed(d, kinds, lam0)


def _same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}{k}: differs by {np.max(np.abs(a[k] - b[k])):.3e}"


def _flags(gpu, g):
    import ctypes as C
    f = C.c_uint()
    g._chk(gpu.lib().tqgpu_debug_plan(g.h, C.byref(f), None))
    return f.value


@pytest.mark.parametrize("rid", GC.ROW_IDS)
def test_one_iteration_is_the_reference_step(gpu, rid):
    c = GC.case(rid)
    ref = c["ref"]
    g = _mirror(gpu, c["d"], c["kinds"], c["lam0"])
    try:
        assert g.plan["gen"]
        r = g.solve(**STEP)
        sol = g.solution()
    finally:
        g.close()
    tau = BETA ** (r["ls_total"] - 1)
    e_d, e_l = rel_err(sol["dlam"], ref["dlam"]), rel_err(sol["lam"], c["lam0"] + tau * ref["dlam"])
    print(f"{rid}: status {r['status']} iter {r['iter']} trials {r['ls_total']} (reference {c['trials']}, slack {c['slack']:.2e}) "
          f"dlam {e_d:.2e} lam {e_l:.2e} cond {ref['cond']:.2e} condS {ref['condS']:.2e} margin {ref['margin']:.2e}")
    assert (r["status"], r["iter"]) == (1, 1)
    assert e_d <= TOL
    assert e_l <= TOL
    assert c["slack"] >= GC.SLACK_MIN and r["ls_total"] == c["trials"]
    assert c["xu_pin"]
    st1 = c["st1"]
    x, u, sx, su = N.flat_xu(st1)
    mx, mu, md = G.flat_multipliers(c["d"], st1, h_stage=ref["stages"]["h"])
    errs = dict(x=rel_err(sol["x"], x), u=rel_err(sol["u"], u), mu_x=rel_err(sol["mu_x"], mx), mu_u=rel_err(sol["mu_u"], mu), mu_d=rel_err(sol["mu_d"], md))
    print(f"{rid}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" at the accepted point (margin there {st1['margin']:.2e})")
    assert max(errs.values()) <= TOL
    assert np.array_equal(sol["x"][sx != 0], x[sx != 0]) and np.array_equal(sol["u"][su != 0], u[su != 0])
    assert np.array_equal(sol["mu_d"] != 0, np.concatenate(st1["rside"]) != 0), "the device's working set of rows is not the reference's"


@pytest.mark.parametrize("rid", ["one_row", "swap", "mixed"])
def test_repeated_fresh_and_batched_solves_are_bit_identical(gpu, rid):
    c = GC.case(rid)
    opts = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)
    start = GC.clear_start(c["d"], c["kinds"])[0]          # (a whole solve whose decisions are clear of rounding: it ends optimal)
    g = _mirror(gpu, c["d"], c["kinds"], start)
    f = _mirror(gpu, c["d"], c["kinds"], start)
    b0, b1 = _mirror(gpu, c["d"], c["kinds"], start), _mirror(gpu, c["d"], c["kinds"], c["lam0"])
    try:
        r1 = g.solve(**opts); s1 = g.solution()
        r2 = g.solve(**opts); s2 = g.solution()
        rf = f.solve(**opts); sf = f.solution()
        f.set_lambda(c["lam0"])
        rl = f.solve(**opts); sl = f.solution()
        rb = gpu.solve_batch([b0, b1], **opts)
        sb0, sb1 = b0.solution(), b1.solution()
    finally:
        for m in (g, f, b0, b1):
            m.close()
    key = lambda r: (r["status"], r["iter"], r["ls_total"])
    assert key(r1) == key(r2) == key(rf) == key(rb[0]) and r1["status"] == 0
    assert key(rl) == key(rb[1])
    _same(s1, s2, "repeated: "); _same(s1, sf, "fresh: "); _same(s1, sb0, "batch member 0: "); _same(sl, sb1, "batch member 1: ")


@pytest.mark.parametrize("rid", ["one_row", "nc64", "mixed"])
def test_loose_rows_are_the_box_solver(gpu, rid):
    d, kinds, _, lam0 = GC.loose_case(rid)          # a start from which every decision of the whole solve is clear of rounding
    opts = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)
    g = _mirror(gpu, d, kinds, lam0)
    b = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, G._kinds2(kinds), lam0)
    try:
        assert g.plan["gen"] and not b.plan["gen"]
        rg = g.solve(**opts); sg = g.solution()
        rb = b.solve(**opts); sb = b.solution()
    finally:
        g.close(); b.close()
    assert (rg["status"], rg["iter"], rg["ls_total"]) == (rb["status"], rb["iter"], rb["ls_total"]) and rg["status"] == 0
    assert rg["n_launches"] == rb["n_launches"], "the tree with kind-3 nodes did not take the launch-per-phase route of a box tree"
    for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
        e = rel_err(sg[k], sb[k])
        print(f"{rid}: {k} {e:.2e}")
        assert e <= 1e-12
    assert not np.any(sg["mu_d"])


def test_infeasible_stage_qp_ends_with_status_4(gpu):
    bad, good, kinds = GC.infeasible_pair()
    opts = dict(stationarityTolerance=GC.FULL_TOL)
    g = _mirror(gpu, bad, kinds)
    f = None
    try:
        r = g.solve(**opts)
        assert r["status"] == STAGE_QP_SOLVE_FAILED
        g.set_constraints(None, None, None, good["dmin"], good["dmax"])
        r2 = g.solve(**opts); s2 = g.solution()
        print(f"after the feasible row: {r2}")
        f = _mirror(gpu, good, kinds)
        rf = f.solve(**opts); sf = f.solution()
    finally:
        g.close()
        if f is not None:
            f.close()
    assert (r2["status"], r2["iter"], r2["ls_total"]) == (rf["status"], rf["iter"], rf["ls_total"]) and rf["status"] == 0
    _same(s2, sf)
    assert s2["x"][0] + s2["u"][0] >= 1.5 - 1e-12 and s2["mu_d"][0] < 0


def test_refusals(gpu):
    import ctypes as C
    L = gpu.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    c = GC.case("one_row")
    d = c["d"]
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    try:
        nc = np.ascontiguousarray(d["nc"], np.int32)
        lo, hi = np.array([1.0]), np.array([0.5])
        assert L.tqgpu_set_constraints(g.h, ip(nc), dp(d["C"]), dp(d["D"]), dp(lo), dp(hi)) == EINVAL
        nc65 = np.array([65, 0, 0], np.int32)
        assert L.tqgpu_set_constraints(g.h, ip(nc65), None, None, None, None) == EUNSUPPORTED
    finally:
        g.close()
    # nz = 65 on a kind-3 node
    nk, nx, nu = np.array([1, 0], np.int32), np.array([40, 2], np.int32), np.array([25, 0], np.int32)
    g = gpu.TqGpu(nk, nx, nu)
    try:
        g.set_constraints(np.array([1, 0], np.int32), np.zeros(40), np.zeros(25), np.array([-1.0]), np.array([1.0]))
        Q = np.concatenate([np.eye(40).ravel(), np.eye(2).ravel()]); R = np.eye(25).ravel(); S = np.zeros(25 * 40)
        kind = np.array([3, 1], np.int32)
        assert L.tqgpu_set_objective_mixed(g.h, ip(kind), dp(Q), dp(R), dp(S), dp(np.zeros(42)), dp(np.zeros(25))) == EUNSUPPORTED
    finally:
        g.close()


def test_plan_bits(gpu):
    c = GC.case("row_and_bound")
    d, kinds = c["d"], c["kinds"]
    g = _mirror(gpu, d, kinds)
    b = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, G._kinds2(kinds))
    try:
        fg, fb = _flags(gpu, g), _flags(gpu, b)
        rg, rb = g.solve(), b.solve()
    finally:
        g.close(); b.close()
    print(f"plan of the kind-3 tree {fg:#x}, of the kind-2 tree {fb:#x}")
    assert fg & (1 << 18) and not fb & (1 << 18)
    assert fb == PLAN_BOX_TREE
    # no fused tails on either tree: the same launches for the same iterations and trials
    assert rg["status"] == 0 and rb["status"] == 0
    if (rg["iter"], rg["ls_total"]) == (rb["iter"], rb["ls_total"]):
        assert rg["n_launches"] == rb["n_launches"]

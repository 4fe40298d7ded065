"""The box-constrained dense stage solver of the device (kind 2 of tqgpu_set_objective_mixed: k_stage_box / stage_box,
k_dense_init, k_export_box) pinned per operation to the numpy reference of newton_ref.py, on the rows of box_cases.py.

What is compared with what:
a. one iteration from the row's lambda0 without regularisation: the exported dlam is the reference's Newton step (which rests on
   every node's elimination matrix P_k = Z (Z'H_k Z)^-1 Z' and stage solution), lambda is lambda0 + tau dlam, and x, u are the
   reference's stage solutions at the new lambda, with the entries the reference has on a bound on it bit for bit;
b. the trial count of that iteration is the reference's line search (which rests on every node's dual-function term);
c. a whole solve from lambda = 0 ends optimal, passes the oracle's KKT check and the numpy certificate, and exports the
   multipliers of that certificate's KKT solve (negated: mu = h - Hz), exactly zero on free entries;
d. a hot start (the previous z projected onto the box, the stored working set restricted to it) gives bit for bit what a fresh
   mirror gives, across a release, an addition and a swap of sides, after re-uploading the same bounds, and after uploading
   another H;
e. an indefinite H_k ends the solve with status 4 (TREEQP_DN_STAGE_QP_SOLVE_FAILED), and the mirror then solves a well-posed
   problem as a fresh one does.

Tolerances: 1e-10 on the step, on lambda and on x, u is the project's tolerance for this pin (test_gpu_limits.py), meaningful
because every row has cond(M) <= 1e6 (1e6 * 2^-53 ~ 1e-10) and margin >= 1e-6 (no entry is within 1e-6 of changing sides, so
the device and the reference work with the same active sets); a trial count is compared where every Armijo decision of the
reference keeps a slack of 1e-9 (box_cases.SLACK_MIN).  The multipliers are compared to 1e-7: certify holds x, u to 1e-9 of its
KKT solve, and mu = h - Hz moves with x, u by at most the largest absolute row sum of H_k, 61 on the rows of the table (the
share of the duals, converged to 1e-10 in the dynamics residual, is smaller); multipliers on these rows are of order 0.1 to 1."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import box_cases as BC
import newton_ref as N
from helpers import assert_solution_close, bounds_vec, certify, global_kkt, offsets, rel_err
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

TOL = 1e-10
MU_TOL = 1e-7
STEP = dict(maxIter=1, regType=0)
BETA = BC.OPTS["lineSearchBeta"]
KEYS = ("x", "u", "lam", "mu_x", "mu_u", "dlam")
# whole solves of the rows with dozens of active bounds on one node: Levenberg-Marquardt always on (see DENSE_OPTS in
# test_gpu_box_dense.py: with whole dual blocks pinned by the bounds the on-the-fly regularisation stalls the line search)
MANY_ACTIVE = ("nz63", "nz63_last_free", "nz64", "nz64_last_free")
QPOASES = 1
STAGE_QP_SOLVE_FAILED = 4


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _mirror(gpu, d, kinds, lam0=None):
    return gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds, lam0)


def _same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}{k}: differs by {np.max(np.abs(a[k] - b[k])):.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# a, b. one iteration: step, lambda, stage solutions, trial count
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rid", BC.ROW_IDS)
def test_one_iteration_is_the_reference_step(gpu, rid):
    c = BC.case(rid)
    ref = c["ref"]
    g = _mirror(gpu, c["d"], c["kinds"], c["lam0"])
    try:
        assert g.plan["box"]
        r = g.solve(**STEP)
        sol = g.solution()
    finally:
        g.close()
    tau = BETA ** (r["ls_total"] - 1)
    e_d, e_l = rel_err(sol["dlam"], ref["dlam"]), rel_err(sol["lam"], c["lam0"] + tau * ref["dlam"])
    print(f"{rid}: status {r['status']} iter {r['iter']} trials {r['ls_total']} (reference {c['trials']}, slack {c['slack']:.2e}) "
          f"dlam {e_d:.2e} lam {e_l:.2e} cond {ref['cond']:.2e} margin {ref['margin']:.2e}")
    assert (r["status"], r["iter"]) == (1, 1)
    assert e_d <= TOL
    assert e_l <= TOL
    if c["slack"] >= BC.SLACK_MIN:
        assert r["ls_total"] == c["trials"]
    if c["xu_pin"]:
        x, u, sx, su = N.flat_xu(c["st1"])
        e_x, e_u = rel_err(sol["x"], x), rel_err(sol["u"], u)
        print(f"{rid}: x {e_x:.2e} u {e_u:.2e} at the accepted point (margin there {c['st1']['margin']:.2e}), "
              f"{int(np.sum(sx != 0) + np.sum(su != 0))} entries on a bound")
        assert e_x <= TOL and e_u <= TOL
        assert np.array_equal(sol["x"][sx != 0], x[sx != 0]) and np.array_equal(sol["u"][su != 0], u[su != 0])


def test_lands_on_bound_is_clipping(gpu, orc):
    """A diagonal problem in dyadic numbers uploaded as kind 2: stage values that land exactly on a bound are fixed there (the
    inclusive rule), so the step is the clipping step of the reference, and a whole solve is the oracle's (clipping): verdict,
    iterations, trials, solution."""
    c = BC.lands_on_bound()
    d, ref = c["d"], c["ref"]
    full = orc.solve(d, orc.default_opts(), c["lam0"])
    one = orc.solve(d, orc.default_opts(**STEP), c["lam0"])
    g = _mirror(gpu, d, c["kinds"], c["lam0"])
    try:
        r1 = g.solve(**STEP)
        s1 = g.solution()
        g.set_lambda(c["lam0"])
        r = g.solve()
        sol = g.solution()
    finally:
        g.close()
    assert (r1["status"], r1["iter"], r1["ls_total"]) == (1, 1, int(one["trace_ls"][0]))
    assert rel_err(s1["dlam"], ref["dlam"]) <= TOL
    assert rel_err(s1["lam"], c["lam0"] + BETA ** (r1["ls_total"] - 1) * ref["dlam"]) <= TOL
    assert_solution_close(s1, one, TOL)
    assert (r["status"], r["iter"], r["ls_total"]) == (full["status"], full["iter"], full["ls_total"]) and r["status"] == 0
    assert_solution_close(sol, full, TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# c. whole solves: certificate and exported multipliers
# ---------------------------------------------------------------------------------------------------------------------------

def _finite_far_bounds(d):
    """IEEE infinities -> -+1e12, which the oracle's KKT check reads as `no bound` (0 * inf is not a number there)"""
    return dict(d, **{k: np.clip(d[k], -P.INF, P.INF) for k in ("xmin", "xmax", "umin", "umax")})


def _check_whole_solve(orc, d, kinds, r, sol, what):
    assert r["status"] == 0, what
    kkt = orc.max_kkt(_finite_far_bounds(d), sol, dense=True)
    n_active = certify(d, sol)
    z = np.concatenate([sol["x"], sol["u"]])
    mu = np.concatenate([sol["mu_x"], sol["mu_u"]])
    lo, hi = bounds_vec(d)
    on = (z == lo) | (z == hi)
    fixed = {int(i): float(z[i]) for i in np.flatnonzero(on)}
    _, mk = global_kkt(d, fixed)
    want = np.zeros(len(z))
    for i, m in mk.items():
        want[i] = -m
    # (dense unconstrained nodes have bounds of -+1e12 in the table: never met, no multipliers)
    e_mu = rel_err(mu, want)
    print(f"{what}: iter {r['iter']} trials {r['ls_total']} KKT {kkt:.2e} active {n_active} mu {e_mu:.2e}")
    assert kkt < 1e-9
    assert e_mu <= MU_TOL
    assert not np.any(mu[~on]), "a free entry has a multiplier"
    for i in np.flatnonzero(on & (lo < hi)):
        assert (mu[i] <= 0.0) if z[i] == lo[i] else (mu[i] >= 0.0), f"entry {i}: multiplier {mu[i]:.3e} of the wrong sign"
    return n_active


@pytest.mark.parametrize("rid", BC.ROW_IDS + ["lands_on_bound"])
def test_whole_solve_certificate_and_multipliers(gpu, orc, rid):
    c = BC.lands_on_bound() if rid == "lands_on_bound" else BC.case(rid)
    opts = dict(stationarityTolerance=1e-10)
    if rid in MANY_ACTIVE:
        opts.update(regType=1, regValue=1e-8, maxIter=200)
    g = _mirror(gpu, c["d"], c["kinds"])
    try:
        r = g.solve(**opts)
        sol = g.solution()
    finally:
        g.close()
    n_active = _check_whole_solve(orc, c["d"], c["kinds"], r, sol, rid)
    if rid != "none_active":
        assert n_active >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# d. hot starts: bit for bit the fresh mirror's result
# ---------------------------------------------------------------------------------------------------------------------------

def _set_bounds(gpu, g, d):
    keep = [np.ascontiguousarray(d[k], dtype=np.float64) for k in ("xmin", "xmax", "umin", "umax")]
    g._chk(gpu.lib().tqgpu_set_bounds(g.h, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in keep]))


@pytest.mark.parametrize("variant", ["set_lambda", "set_bounds", "other_H"])
@pytest.mark.parametrize("rid", BC.PATH_ROWS)
def test_hot_start_is_path_independent(gpu, rid, variant):
    """Mirror G takes one iteration at lamA, then one at lamB; mirror F starts fresh at lamB.  Relative to G's last trial at lamA
    the working sets at lamB release bounds, add bounds and move entries from their lower to their upper bound
    (box_cases.path_duals).  set_bounds: the same bounds are uploaded again in between (the kept P_k stay valid); other_H: another
    H is uploaded in between with the same bounds (every P_k is rebuilt)."""
    c = BC.case(rid)
    d, kinds = c["d"], c["kinds"]
    lamA, lamB, counts = BC.path_duals(rid)
    d2 = BC.other_hessians(d, kinds) if variant == "other_H" else d
    G = _mirror(gpu, d, kinds, lamA)
    F = None
    try:
        rA = G.solve(**STEP)
        assert rA["status"] == 1
        if variant == "set_bounds":
            _set_bounds(gpu, G, d)
        if variant == "other_H":
            G.upload_mixed(d2, kinds, lamB)
        else:
            G.set_lambda(lamB)
        rG = G.solve(**STEP)
        sG = G.solution()
        F = _mirror(gpu, d2, kinds, lamB)
        rF = F.solve(**STEP)
        sF = F.solution()
    finally:
        G.close()
        if F is not None:
            F.close()
    print(f"{rid}/{variant}: {counts}, trials {rG['ls_total']} / {rF['ls_total']}")
    assert (rG["status"], rG["iter"], rG["ls_total"]) == (rF["status"], rF["iter"], rF["ls_total"])
    _same(sG, sF, f"{rid}/{variant} ")
    if variant != "other_H":
        ref = N.newton_step(d, lamB, kinds=kinds)
        assert rel_err(sG["dlam"], ref["dlam"]) <= TOL


# ---------------------------------------------------------------------------------------------------------------------------
# e. status 4
# ---------------------------------------------------------------------------------------------------------------------------

def test_indefinite_stage_hessian_ends_with_status_4(gpu):
    bad, good, kinds = BC.indefinite_pair()
    opts = dict(stationarityTolerance=1e-10)
    g = _mirror(gpu, bad, kinds)
    f = None
    try:
        r = g.solve(**opts)
        assert r["status"] == STAGE_QP_SOLVE_FAILED
        g.upload_mixed(good, kinds)
        r2 = g.solve(**opts)
        s2 = g.solution()
        f = _mirror(gpu, good, kinds)
        rf = f.solve(**opts)
        sf = f.solution()
    finally:
        g.close()
        if f is not None:
            f.close()
    assert (r2["status"], r2["iter"], r2["ls_total"]) == (rf["status"], rf["iter"], rf["ls_total"]) and rf["status"] == 0
    _same(s2, sf)


def test_indefinite_stage_hessian_through_the_dropin_api(gpu):
    bad, good, kinds = BC.indefinite_pair()
    nk, nx, nu = bad["nk"], bad["nx"], bad["nu"]
    qp = gpu.TreeQp(nx, nu, nk)
    xo, uo = offsets(bad)
    H = BC._node_blocks(bad)
    dad = P.parents_of(nk)
    ao = bo = lo = 0
    for k in range(len(nk)):
        a = int(nx[k])
        Hk = H[k]
        qp.set_node_objective(k, Hk[:a, :a], Hk[a:, a:], Hk[a:, :a], bad["q"][xo[k]:xo[k + 1]], bad["r"][uo[k]:uo[k + 1]])
        qp.set_node_bounds(k, bad["xmin"][xo[k]:xo[k + 1]], bad["xmax"][xo[k]:xo[k + 1]], bad["umin"][uo[k]:uo[k + 1]], bad["umax"][uo[k]:uo[k + 1]])
        if k > 0:
            p = dad[k]
            na, nb = nx[k] * nx[p], nx[k] * nu[p]
            qp.set_edge_dynamics(k - 1, bad["A"][ao:ao + na], bad["B"][bo:bo + nb], bad["b"][lo:lo + nx[k]])
            ao += na; bo += nb; lo += nx[k]
    s = gpu.TdunesSolver(qp)
    for k in range(qp.N):
        s.opts.qp_solver[k] = QPOASES
    try:
        assert s.solve() == STAGE_QP_SOLVE_FAILED
    finally:
        s.destroy()

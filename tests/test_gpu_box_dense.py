"""Dense stage QPs with box bounds (device kind 2): the reference's TREEQP_QPOASES_SOLVER (qpOASES QProblemB, dual_Newton_tree_qpoases.c)
on nodes with finite bounds, through the C-ABI (tqgpu_set_objective_mixed kind 2), the drop-in front end and the JSON tool."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import assert_solution_close, bounds_vec, certify, global_kkt, offsets, product_qp_from_lti, with_dense_blocks
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-10
# Genuinely dense trees with dozens of active bounds: with whole dual blocks pinned by the bounds the dual Hessian is close to
# singular, and the default on-the-fly regularisation lets the line search run out of trials for hundreds of iterations (the
# method's behaviour, not the stage solver's: the same runs converge in 41 - 56 iterations with Levenberg-Marquardt always on).
DENSE_OPTS = dict(stationarityTolerance=1e-10, regType=1, regValue=1e-8, maxIter=200)
QPOASES = 1          # stage_qp_t TREEQP_QPOASES_SOLVER


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


# ---------------------------------------------------------------------------------------------------------------------------
# problem construction and an independent certificate
# ---------------------------------------------------------------------------------------------------------------------------

def stage_of(nk):
    dad = P.parents_of(nk)
    st = np.zeros(len(nk), dtype=int)
    for k in range(1, len(nk)):
        st[k] = st[dad[k]] + 1
    return st


def boxes_around(d, z_f, z_unc, margin=0.05):
    """bounds that hold the feasible point z_f and cut z_unc: entry i in [min(z_f, m) - margin, max(z_f, m) + margin], m the midpoint"""
    mid = 0.5 * (z_f + z_unc)
    return np.minimum(z_f, mid) - margin, np.maximum(z_f, mid) + margin


def set_boxes(d, lo, hi, kinds=None):
    SX = len(d["xmin"])
    xo, uo = offsets(d)
    for k in range(len(d["nk"])):
        ix, iu = slice(xo[k], xo[k + 1]), slice(uo[k], uo[k + 1])
        if kinds is not None and kinds[k] == 1:
            d["xmin"][ix], d["xmax"][ix], d["umin"][iu], d["umax"][iu] = -1e12, 1e12, -1e12, 1e12
        else:
            d["xmin"][ix], d["xmax"][ix] = lo[ix], hi[ix]
            d["umin"][iu], d["umax"][iu] = lo[SX + uo[k]:SX + uo[k + 1]], hi[SX + uo[k]:SX + uo[k + 1]]


def dense_boxed_problem(seed, depth=3, nx_range=(2, 20), nu_range=(1, 10), kinds=None):
    """full Q, R, S (H = diag + M M') on every node and bounds that cut the unconstrained optimum but hold a point that satisfies
    the dynamics (the optimum for another linear term): the QP is feasible and several bounds are active at its solution"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = P.random_shape_qp(seed, depth=depth, max_kids=3, nx_range=nx_range, nu_range=nu_range, ubound=1.0)
    d = with_dense_blocks(f.as_dict())
    nk, nx, nu = d["nk"], d["nx"], d["nu"]
    Nn = len(nk)
    kinds = np.full(Nn, 2, dtype=np.int32) if kinds is None else np.asarray(kinds, dtype=np.int32)
    xo, uo = offsets(d)
    Q, R, S = [], [], []
    for k in range(Nn):
        a, m = int(nx[k]), int(nu[k])
        H = np.diag(np.concatenate([d["Qd"][xo[k]:xo[k + 1]], d["Rd"][uo[k]:uo[k + 1]]]))
        if kinds[k] != 0:
            M = 0.3 * rng.standard_normal((a + m, a + m))
            H = H + M @ M.T
        Q.append(H[:a, :a].ravel(order="F")); R.append(H[a:, a:].ravel(order="F")); S.append(H[a:, :a].ravel(order="F"))
    d["Q"], d["R"], d["S"] = np.concatenate(Q), np.concatenate(R), np.concatenate(S)
    d["q"] = rng.standard_normal(len(d["q"]))
    d["r"] = rng.standard_normal(len(d["r"]))
    z_unc, _ = global_kkt(d)
    z_f, _ = global_kkt(dict(d, q=rng.standard_normal(len(d["q"])), r=rng.standard_normal(len(d["r"]))))
    set_boxes(d, *boxes_around(d, z_f, z_unc), kinds)
    return d, kinds


def active_nodes(d, sol, kinds):
    xo, uo = offsets(d)
    n = 0
    for k in np.flatnonzero(kinds == 2):
        ix, iu = slice(xo[k], xo[k + 1]), slice(uo[k], uo[k + 1])
        n += int(np.any(sol["x"][ix] == d["xmin"][ix]) or np.any(sol["x"][ix] == d["xmax"][ix]) or
                  np.any(sol["u"][iu] == d["umin"][iu]) or np.any(sol["u"][iu] == d["umax"][iu]))
    return n


def c1_eliminated(gpu):
    p = P.spring_mass(xmax1=0.2)
    return p, product_qp_from_lti(gpu, p, eliminate_x0=True).flat()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. diagonal problems: a diagonal box QP is solved by clipping, so kind 2 must reproduce the oracle (clipping)
# ---------------------------------------------------------------------------------------------------------------------------

def _diag_cases(gpu):
    th = P.thesis_example()
    lc = P.linear_chain(2, 5, 5, ubound=0.2)
    out = [("thesis", th.as_dict(), None),
           ("linear_chain", product_qp_from_lti(gpu, lc).flat(), lc.lambda0)]
    for seed in (3, 11):
        f = P.random_shape_qp(seed, depth=3, max_kids=3, nx_range=(1, 5), nu_range=(1, 3), ubound=0.2)
        out.append((f"random_shape_{seed}", f.as_dict(), f.lambda0))
    return out


@pytest.mark.parametrize("case", range(4))
def test_diagonal_box_nodes_match_the_oracle_through_the_c_abi(gpu, orc, case):
    name, d, lam0 = _diag_cases(gpu)[case]
    kind = np.full(len(d["nk"]), 2, dtype=np.int32)
    ref = orc.solve(d, lambda0=lam0)
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(with_dense_blocks(d), kind, lam0)
    assert g.path == 0
    r = g.solve()
    sol = g.solution()
    g.close()
    assert r["status"] == ref["status"] == 0, name
    assert r["iter"] == ref["iter"], name
    assert_solution_close(sol, ref, TOL)
    lo, hi = bounds_vec(d)
    z = np.concatenate([sol["x"], sol["u"]])
    assert np.any((z == lo) | (z == hi)), f"{name}: no bound active"


def test_diagonal_spring_mass_x0_eliminated_through_the_c_abi(gpu, orc):
    """examples/spring_mass.c tdunes branch (58 iterations, 1329 trials on the oracle) with every node on the box solver.  Kind 2
    solves through a Cholesky factor, clipping multiplies by 1 / Q_jj: an Armijo decision near the optimum may fall the other way."""
    p, d = c1_eliminated(gpu)
    assert d["nx"][0] == 0
    ref = orc.solve(d, lambda0=p.lambda0)
    assert ref["iter"] == 58
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(with_dense_blocks(d), np.full(len(d["nk"]), 2), p.lambda0)
    r = g.solve(stationarityTolerance=1e-8)
    sol = g.solution()
    g.close()
    assert r["status"] == 0 and abs(r["iter"] - ref["iter"]) <= 2
    assert orc.max_kkt(d, sol) < 1e-10
    assert_solution_close(sol, ref, TOL if r["iter"] == ref["iter"] else 1e-7)


@pytest.mark.parametrize("x0_eliminated", [False, True])
def test_diagonal_box_nodes_through_the_dropin_api(gpu, orc, x0_eliminated):
    """tree_qp_in + opts.qp_solver[k] = TREEQP_QPOASES_SOLVER with finite bounds (today a fatal error of the front end)"""
    p = P.spring_mass(xmax1=0.2) if x0_eliminated else P.linear_chain(2, 5, 5, ubound=0.2)
    qp = product_qp_from_lti(gpu, p, eliminate_x0=x0_eliminated)
    d = qp.flat()
    ref = orc.solve(d, lambda0=p.lambda0)
    s = gpu.TdunesSolver(qp)
    for k in range(qp.N):
        s.opts.qp_solver[k] = QPOASES
    s.set_dual_initialization(p.lambda0)
    status = s.solve()
    assert status == ref["status"] == 0
    if x0_eliminated:
        assert abs(qp.info["iter"] - ref["iter"]) <= 2 and qp.max_kkt_res() < 1e-10
    else:
        assert qp.info["iter"] == ref["iter"]
    assert_solution_close(qp.solution(), ref, TOL if qp.info["iter"] == ref["iter"] else 1e-7)
    s.destroy()


@pytest.mark.parametrize("opt", [dict(regType=0), dict(regType=1, regValue=1e-8), dict(regType=2),
                                 dict(termCondition=0, stationarityTolerance=1e-12), dict(termCondition=1), dict(termCondition=2),
                                 dict(maxIter=1), dict(maxIter=2)])
def test_options_and_early_exits(gpu, orc, opt):
    """all regularisations and termination norms; maxIter = 1, 2 exits pair mu with x, u as the oracle does (the xUncS restore)"""
    lc = P.linear_chain(2, 5, 5, ubound=0.2)
    d = product_qp_from_lti(gpu, lc).flat()
    ref = orc.solve(d, orc.default_opts(**opt), lc.lambda0)
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(with_dense_blocks(d), np.full(len(d["nk"]), 2), lc.lambda0)
    r = g.solve(**opt)
    sol = g.solution()
    g.close()
    assert (r["status"], r["iter"]) == (ref["status"], ref["iter"])
    assert_solution_close(sol, ref, TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# 2, 3. genuinely dense stage QPs with active bounds; a tree of all three kinds
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [4, 9])
def test_dense_nodes_with_active_bounds(gpu, orc, seed):
    d, kinds = dense_boxed_problem(seed)
    nz = np.asarray(d["nx"]) + np.asarray(d["nu"])
    assert nz.max() > 16
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    r = g.solve(**DENSE_OPTS)
    sol = g.solution()
    g.close()
    assert r["status"] == 0
    assert orc.max_kkt(d, sol, dense=True) < 1e-9
    assert certify(d, sol) >= 20
    assert active_nodes(d, sol, kinds) >= 0.6 * len(kinds)


def test_tree_of_all_three_kinds(gpu, orc):
    f = P.random_shape_qp(6, depth=3, max_kids=3, nx_range=(2, 12), nu_range=(1, 6), ubound=1.0)
    kinds = np.asarray([(2, 0, 1, 2)[s % 4] for s in stage_of(f.nk)], dtype=np.int32)
    d, kinds = dense_boxed_problem(6, nx_range=(2, 12), nu_range=(1, 6), kinds=kinds)
    assert set(kinds.tolist()) == {0, 1, 2}
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    r = g.solve(stationarityTolerance=1e-10)
    sol = g.solution()
    g.close()
    assert r["status"] == 0
    assert orc.max_kkt(d, sol, dense=True) < 1e-9
    certify(d, sol)
    assert active_nodes(d, sol, kinds) >= 1


# ---------------------------------------------------------------------------------------------------------------------------
# 4. MPC loop: hot-started working sets and duals give the fresh solve's answer
# ---------------------------------------------------------------------------------------------------------------------------

def _mpc_qp(gpu, p, x0):
    qp = product_qp_from_lti(gpu, p, eliminate_x0=True)
    qp.set_x0(x0)
    s = gpu.TdunesSolver(qp)
    for k in range(qp.N):
        s.opts.qp_solver[k] = QPOASES
    return qp, s


def test_mpc_loop_with_hot_starts(gpu):
    p = P.spring_mass(md=2, Nr=2, Nh=5, xmax1=0.2)
    rng = np.random.Generator(np.random.PCG64(1))
    qp, s = _mpc_qp(gpu, p, p.x0)
    s.set_dual_initialization(p.lambda0)
    lam = np.array(p.lambda0, dtype=float)
    for step in range(10):
        x0 = np.asarray(p.x0, dtype=float) * (1.0 - 0.08 * step) + 0.01 * rng.standard_normal(len(p.x0))
        qp.set_x0(x0)
        assert s.solve() == 0                       # warm: duals and working sets of the previous solve
        warm, it = qp.solution(), qp.info["iter"]
        qf, sf = _mpc_qp(gpu, p, x0)
        sf.set_dual_initialization(lam)
        assert sf.solve() == 0
        assert qf.info["iter"] == it, step
        assert_solution_close(warm, qf.solution(), TOL)
        sf.destroy()
        lam = warm["lam"]
    # two solves from the same duals are bit-identical (the second starts from the first one's working sets)
    s.set_dual_initialization(p.lambda0)
    assert s.solve() == 0
    a = qp.solution()
    s.set_dual_initialization(p.lambda0)
    assert s.solve() == 0
    b = qp.solution()
    for k in ("x", "u", "lam", "mu_x", "mu_u"):
        assert np.array_equal(a[k], b[k]), k
    s.destroy()


def test_reuploads_need_no_reset(gpu):
    """re-uploading bounds and objective between solves (the drop-in front end does it every solve) leaves the result alone"""
    d, kinds = dense_boxed_problem(4)
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    g.solve(**DENSE_OPTS)
    a = g.solution()
    loose = dict(d, xmin=d["xmin"] - 0.1, xmax=d["xmax"] + 0.1, umin=d["umin"] - 0.1, umax=d["umax"] + 0.1)
    g.upload_mixed(loose, kinds)
    g.solve(**DENSE_OPTS)
    g.upload_mixed(d, kinds)
    r = g.solve(**DENSE_OPTS)
    b = g.solution()
    g.close()
    h = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    rf = h.solve(**DENSE_OPTS)
    c = h.solution()
    h.close()
    assert r["status"] == rf["status"] == 0 and r["iter"] == rf["iter"]
    assert_solution_close(b, c, TOL)
    assert_solution_close(a, c, TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. JSON front end: a bounded dense problem without "clipping" solves
# ---------------------------------------------------------------------------------------------------------------------------

def test_json_front_end_bounded_dense_problem(gpu, orc, tmp_path):
    src = json.loads((ROOT / "tests" / "golden" / "random_qp_data00.json").read_text())
    f = P.random_qp_fixture(0)
    xo, uo = offsets(f)
    SX = int(xo[-1])
    rng = np.random.Generator(np.random.PCG64(3))
    z_unc = np.concatenate([f["xopt"], f["uopt"]])
    z_f, _ = global_kkt(dict(f, q=rng.standard_normal(len(f["q"])), r=rng.standard_normal(len(f["r"]))))
    lo, hi = boxes_around(f, z_f, z_unc)
    for k, n in enumerate(src["nodes"]):
        n["lx"], n["ux"] = lo[xo[k]:xo[k + 1]].tolist(), hi[xo[k]:xo[k + 1]].tolist()
        if f["nu"][k]:
            n["lu"], n["uu"] = lo[SX + uo[k]:SX + uo[k + 1]].tolist(), hi[SX + uo[k]:SX + uo[k + 1]].tolist()
    (tmp_path / "qp_in.json").write_text(json.dumps(src))
    exe = ROOT / "treeqp_amd" / "lib" / "treeqp_solve_json"
    out = subprocess.run([str(exe), str(tmp_path / "qp_in.json")], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout)
    assert res["info"]["status"] == 0 and res["info"]["kkt_tol"] < 1e-8
    nodes = res["solution"]["nodes"]
    cat = lambda key: np.concatenate([np.atleast_1d(np.asarray(n[key], dtype=float)) for n in nodes])
    sol = dict(x=cat("x"), u=cat("u"), mu_x=cat("mu_x"), mu_u=cat("mu_u"),
               lam=np.concatenate([np.atleast_1d(np.asarray(e["lam"], dtype=float)) for e in res["solution"]["edges"]]))
    d = dict(f)
    d["xmin"] = np.concatenate([np.asarray(n["lx"], dtype=float) for n in src["nodes"]])
    d["xmax"] = np.concatenate([np.asarray(n["ux"], dtype=float) for n in src["nodes"]])
    d["umin"] = np.concatenate([np.asarray(n.get("lu", []), dtype=float) for n in src["nodes"]])
    d["umax"] = np.concatenate([np.asarray(n.get("uu", []), dtype=float) for n in src["nodes"]])
    assert np.all(sol["x"] >= d["xmin"] - 1e-12) and np.all(sol["x"] <= d["xmax"] + 1e-12)
    assert np.all(sol["u"] >= d["umin"] - 1e-12) and np.all(sol["u"] <= d["umax"] + 1e-12)
    assert np.any(sol["x"] == d["xmax"]) or np.any(sol["x"] == d["xmin"]) or np.any(sol["u"] == d["umin"]) or np.any(sol["u"] == d["umax"])
    assert orc.max_kkt(d, sol, dense=True) < 1e-8


# ---------------------------------------------------------------------------------------------------------------------------
# 6. batches; 7. limits
# ---------------------------------------------------------------------------------------------------------------------------

def test_batch_member_with_box_nodes_matches_its_single_solve(gpu):
    d, kinds = dense_boxed_problem(9)
    single = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    rs = single.solve(**DENSE_OPTS)
    a = single.solution()
    single.close()
    lc = P.linear_chain(2, 5, 5, ubound=0.2)
    other = product_qp_from_lti(gpu, lc).flat()
    m0 = gpu.TqGpu(other["nk"], other["nx"], other["nu"]).upload(other, lc.lambda0)
    m1 = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    res = gpu.solve_batch([m0, m1], **DENSE_OPTS)
    b = m1.solution()
    m0.close(); m1.close()
    assert res[1]["status"] == rs["status"] == 0 and res[1]["iter"] == rs["iter"]
    for k in ("x", "u", "lam", "mu_x", "mu_u"):
        assert np.array_equal(a[k], b[k]), k


def _two_node(gpu, nx, nu, seed=2):
    rng = np.random.Generator(np.random.PCG64(seed))
    nk, nxs, nus = np.array([1, 0], np.int32), np.array([nx, nx], np.int32), np.array([nu, 0], np.int32)
    Q, R, S = [], [], []
    for a, m in ((nx, nu), (nx, 0)):
        M = 0.2 * rng.standard_normal((a + m, a + m))
        H = np.eye(a + m) * 2.0 + M @ M.T
        Q.append(H[:a, :a].ravel(order="F")); R.append(H[a:, a:].ravel(order="F")); S.append(H[a:, :a].ravel(order="F"))
    d = dict(nk=nk, nx=nxs, nu=nus, A=0.3 * rng.standard_normal(nx * nx), B=0.3 * rng.standard_normal(nx * nu), b=rng.standard_normal(nx),
             Q=np.concatenate(Q), R=np.concatenate(R), S=np.concatenate(S), q=rng.standard_normal(2 * nx), r=rng.standard_normal(nu),
             xmin=np.zeros(2 * nx), xmax=np.zeros(2 * nx), umin=np.zeros(nu), umax=np.zeros(nu))
    z_unc, _ = global_kkt(d)
    z_f, _ = global_kkt(dict(d, q=rng.standard_normal(2 * nx), r=rng.standard_normal(nu)))
    set_boxes(d, *boxes_around(d, z_f, z_unc))
    return d


def test_limits_of_the_box_solver(gpu, orc):
    d = _two_node(gpu, 40, 24)                                      # nz = 64 on the root: the largest box node
    kinds = np.array([2, 2], np.int32)
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, kinds)
    r = g.solve(stationarityTolerance=1e-10)
    sol = g.solution()
    assert r["status"] == 0
    assert orc.max_kkt(d, sol, dense=True) < 1e-9
    assert certify(d, sol) > 0
    # lb > ub on a box node: refused, the mirror and the process stay usable
    bad = dict(d, xmin=d["xmin"].copy())
    bad["xmin"][3] = 1.0
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        g.upload_mixed(bad, kinds)
    g.upload_mixed(d, kinds)
    r2 = g.solve(stationarityTolerance=1e-10)
    assert r2["status"] == 0 and r2["iter"] == r["iter"]
    g.close()
    d = _two_node(gpu, 40, 25)                                      # nz = 65: not one entry per lane
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        g.upload_mixed(d, np.array([2, 2], np.int32))
    g.upload_mixed(d, np.array([1, 2], np.int32))                   # the same node as a dense unconstrained one is fine
    g.close()

"""Parity of the HIP device path against the CPU oracle (run on the MI355X box: pytest -m gpu).

Every solve below goes through the C-ABI of libtreeqp_amd.so -- either the reference-compatible
front end (treeqp_tdunes_*) or the thin device ABI (tqgpu_*).  Tolerance: 1e-10 relative on
x, u, lambda, mu (north_star: "within 1e-10 relative on KKT residuals"), identical Newton
iteration counts; integer tables are bit-exact.
"""
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import (assert_solution_close, lti_dims, oracle_flat_from_lti, product_qp_from_flat,
                     product_qp_from_lti, rel_err)
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-10


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def solve_lti_both(gpu, orc, p, eliminate_x0=False, **opts):
    qp = product_qp_from_lti(gpu, p, eliminate_x0=eliminate_x0)
    flat = qp.flat()
    ref = orc.solve(flat, orc.default_opts(**opts), p.lambda0)
    s = gpu.TdunesSolver(qp, **opts)
    s.set_dual_initialization(p.lambda0)
    status = s.solve()
    return qp, s, status, ref, flat


LTI_CASES = [
    ("c1_default", lambda: P.spring_mass(), False, 3),
    ("c1_depth4", lambda: P.spring_mass(Nh=4), False, None),
    ("chain_small", lambda: P.linear_chain(2, 4, 6), False, None),
    ("c2_chain_1023", lambda: P.linear_chain(2, 9, 9), False, 3),
]


@pytest.mark.parametrize("name,make,elim,expect_iter", LTI_CASES, ids=[c[0] for c in LTI_CASES])
def test_lti_cases_match_oracle(gpu, orc, name, make, elim, expect_iter):
    p = make()
    qp, s, status, ref, flat = solve_lti_both(gpu, orc, p, elim)
    assert status == ref["status"] == 0
    assert qp.info["iter"] == ref["iter"]
    if expect_iter is not None:
        assert qp.info["iter"] == expect_iter
    assert s.ls_total == ref["ls_total"]
    assert_solution_close(qp.solution(), ref, TOL)
    assert qp.max_kkt_res() < 1e-8                      # the reference driver's own assert
    assert abs(qp.max_kkt_res() - orc.max_kkt(flat, ref)) < 1e-9
    # integer tables of the workspace are bit-exact (dual_Newton_tree.c:166-194)
    t = orc.tree_arrays(p.nk(), flat["nx"])
    assert np.array_equal(s.idxpos(), t["idxpos"]) and np.array_equal(s.npar(), t["npar"])
    s.destroy()


def test_x0_eliminated_spring_mass(gpu, orc):
    """examples/spring_mass.c tdunes branch: x0 eliminated (nx[0]=0), xmax[1]=0.2, 58 iterations."""
    p = P.spring_mass(xmax1=0.2)
    qp, s, status, ref, flat = solve_lti_both(gpu, orc, p, eliminate_x0=True)
    assert status == ref["status"] == 0
    assert ref["iter"] == 58
    assert qp.max_kkt_res() < 1e-10                     # examples/spring_mass.c:331
    # a long, line-search heavy run (1329 trials): every Armijo decision of the device falls as the reference's
    assert qp.info["iter"] == ref["iter"] and s.ls_total == ref["ls_total"]
    assert_solution_close(qp.solution(), ref, TOL)
    s.destroy()


@pytest.mark.parametrize("make", [lambda: P.spring_mass(xmax1=0.2), lambda: P.linear_chain(2, 5, 5), lambda: P.linear_chain(2, 2, 6)],
                         ids=["c1_multistage", "chain_uniform", "chain_multistage"])
def test_x0_eliminated_trees_take_the_persistent_path(gpu, orc, make):
    """nx[0] = 0 (tree_qp_in_eliminate_x0) on an otherwise uniform / multistage tree: embedded with phantom root
    states, solved by one persistent launch; dimensions and solution at the ABI are those of the eliminated QP."""
    p = make()
    qp = product_qp_from_lti(gpu, p, eliminate_x0=True)
    flat = qp.flat()
    assert flat["nx"][0] == 0
    ref = orc.solve(flat, lambda0=p.lambda0)
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    assert g.path == 2 and g.sum_nx == int(np.sum(flat["nx"]))
    r = g.solve()
    sol = g.solution()
    g.close()
    os.environ["TREEQP_AMD_PATH"] = "generic"
    try:
        gg = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    finally:
        os.environ.pop("TREEQP_AMD_PATH", None)
    assert gg.path == 0
    rg = gg.solve()
    sg = gg.solution()
    gg.close()
    assert r["status"] == rg["status"] == ref["status"] == 0
    assert r["iter"] == rg["iter"] == ref["iter"]
    for sl in (sol, sg):
        assert_solution_close(sl, ref, TOL)
        assert orc.max_kkt(flat, sl) < 1e-8


FLAT_CASES = [
    ("thesis", lambda: P.thesis_example()),
    ("irregular_dims", lambda: P.irregular_clipping_qp()),
    ("irregular_dims_seed9", lambda: P.irregular_clipping_qp(9)),
    ("pruned_c5", lambda: P.pruned_chain_qp()),
    ("random_c4_small", lambda: P.random_clipping_qp(nx=6, nu=3, md=3, levels=4, seed=5)),
    ("random_c4_mid", lambda: P.random_clipping_qp(nx=20, nu=10, md=3, levels=5, seed=11)),
]


@pytest.mark.parametrize("name,make", FLAT_CASES, ids=[c[0] for c in FLAT_CASES])
def test_flat_cases_match_oracle(gpu, orc, name, make):
    f = make()
    ref = orc.solve(f.as_dict(), orc.default_opts(**f.opts), f.lambda0)
    qp = product_qp_from_flat(gpu, f)
    s = gpu.TdunesSolver(qp, **f.opts)
    status = s.solve()
    assert status == ref["status"] == 0
    assert qp.info["iter"] == ref["iter"]
    assert_solution_close(qp.solution(), ref, TOL)
    assert qp.max_kkt_res() < 1e-8
    s.destroy()


def test_thin_abi_direct(gpu, orc):
    """tqgpu_* with flat arrays, without the treeqp container in between."""
    f = P.irregular_clipping_qp()
    ref = orc.solve(f.as_dict())
    g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f)
    r = g.solve()
    assert r["status"] == 0 and r["iter"] == ref["iter"] and r["ls_total"] == ref["ls_total"]
    assert_solution_close(g.solution(), ref, TOL)
    ls, _ = g.iteration_log()
    assert ls[:r["iter"]].tolist() == ref["trace_ls"][:ref["iter"]].tolist()
    # repeated solves from the same resident lambda0 are reproducible bit for bit
    a = g.solution()
    r2 = g.solve()
    b = g.solution()
    assert r2["iter"] == r["iter"] and all(np.array_equal(a[k], b[k]) for k in a)
    bytes_, flops = g.iteration_cost(1)
    assert bytes_ > 0 and flops > 0
    g.close()


def test_iteration_cost_matches_survey_closed_form(gpu):
    """C2 = 11.41 MB and 5.24 MFLOP per Newton iteration (one LS trial)."""
    p = P.linear_chain(2, 9, 9)
    nx, nu, nk = lti_dims(p)
    g = gpu.TqGpu(nk, nx, nu)
    b, f = g.iteration_cost(1)
    assert abs(b / 1e6 - 11.41) < 0.06 and abs(f / 1e6 - 5.24) < 0.06
    g.close()


def test_options_termination_and_regularisation(gpu, orc):
    p = P.spring_mass(Nh=4)
    for opts in (dict(termCondition=0), dict(termCondition=1), dict(regType=0), dict(regType=1, regValue=1e-8),
                 dict(maxIter=1)):
        qp, s, status, ref, flat = solve_lti_both(gpu, orc, p, **opts)
        assert status == ref["status"], opts
        assert qp.info["iter"] == ref["iter"], opts
        assert_solution_close(qp.solution(), ref, TOL)
        s.destroy()


def test_warm_start_and_workspace_mirrors(gpu, orc):
    p = P.spring_mass()
    qp = product_qp_from_lti(gpu, p)
    s = gpu.TdunesSolver(qp)
    s.set_dual_initialization(p.lambda0)
    assert s.solve() == 0
    first = qp.info["iter"]
    sol = qp.solution()
    # host mirrors used by write_solution_to_txt
    sx = np.concatenate([np.ctypeslib.as_array(s.work.sx[k].pa, shape=(s.work.sx[k].m,)) for k in range(qp.N)])
    lam = np.concatenate([np.ctypeslib.as_array(s.work.slambda[k].pa, shape=(s.work.slambda[k].m,)) for k in range(s.work.Np)])
    assert np.array_equal(sx, sol["x"]) and np.array_equal(lam, sol["lam"])
    # a second solve without re-initialisation starts from the optimal multipliers: 0 iterations
    assert s.solve() == 0 and qp.info["iter"] == 0 and first > 0
    assert_solution_close(qp.solution(), sol, 1e-12)
    s.destroy()


def test_mpc_loop_updates_x0_after_elimination(gpu, orc):
    """§8(f)-1: repeated solves that only change x0 (fault_tolerance.c:625-632 usage pattern)."""
    p = P.spring_mass(xmax1=0.6)
    qp = product_qp_from_lti(gpu, p, eliminate_x0=True)
    s = gpu.TdunesSolver(qp)
    s.set_dual_initialization(p.lambda0)
    for scale in (1.0, 1.5, 0.5):
        qp.set_x0(scale * p.x0)
        assert s.solve() == 0
        flat = qp.flat()
        ref = orc.solve(flat, lambda0=None if scale == 1.0 else prev)      # noqa: F821
        assert ref["status"] == 0
        assert qp.max_kkt_res() < 1e-9
        assert_solution_close(qp.solution(), ref, TOL)
        prev = qp.solution()["lam"]
    s.destroy()


def test_resolve_after_changing_each_input_array(gpu, orc):
    """treeqp_tdunes_solve re-reads qp_in at every call (dual_Newton_tree.c:1142-1160); the device mirror uploads
    only what changed -- every class of change (b, q/r, Q/R, bounds, A/B) must reach the device."""
    p = P.linear_chain(2, 5, 5)
    qp = product_qp_from_lti(gpu, p)
    s = gpu.TdunesSolver(qp)
    rng = np.random.default_rng(3)

    def check():
        s.set_dual_initialization(np.zeros_like(p.lambda0))
        assert s.solve() == 0
        flat = qp.flat()
        ref = orc.solve(flat, lambda0=None)
        assert ref["status"] == 0 and qp.info["iter"] == ref["iter"]
        assert_solution_close(qp.solution(), ref, TOL)

    check()
    check()                                                          # nothing changed
    n, m = p.nx, p.nu
    A0, B0 = p.A[: n * n], p.B[: n * m]
    qp.set_edge_dynamics(3, A0, B0, 0.1 * rng.standard_normal(n)); check()                      # b only
    qp.set_node_objective_diag(5, p.Qd, p.Rd, 0.2 * rng.standard_normal(n), 0.2 * rng.standard_normal(m)); check()   # q, r
    qp.set_node_objective_diag(2, 3.0 * p.Qd, 0.5 * p.Rd, np.zeros(n), np.zeros(m)); check()    # Q, R (new stage inverses)
    qp.set_node_bounds(1, -2.5 * np.ones(n), 2.5 * np.ones(n), -0.1 * np.ones(m), 0.1 * np.ones(m)); check()
    qp.set_edge_dynamics(7, 0.9 * A0, 1.1 * B0, np.zeros(n)); check()                            # A, B
    s.destroy()


# --- larger dual Hessian blocks: the workgroup-per-block MFMA kernels (tdunes_wide.hpp) ---------

@pytest.mark.parametrize("nx,nu,md,levels", [(10, 4, 3, 3), (16, 4, 3, 3), (20, 10, 2, 4), (20, 10, 3, 4), (21, 5, 3, 3), (9, 3, 2, 5)],
                         ids=["d30", "d48_two_wave_panel", "d40", "d60_c4_blocks", "d63", "d18"])
def test_wide_block_kernels_match_oracle(gpu, orc, nx, nu, md, levels):
    """16 < d <= 64: padded 16 x 16 tiles, register panels (one or two waves of rows), MFMA trailing updates."""
    f = P.random_clipping_qp(nx=nx, nu=nu, md=md, levels=levels)
    ref = orc.solve(f.as_dict(), orc.default_opts(**f.opts))
    g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
    assert g.path == 0
    r = g.solve(**f.opts)
    assert r["status"] == ref["status"] == 0 and r["iter"] == ref["iter"] == 1
    assert_solution_close(g.solution(), ref, TOL)
    g.close()


@pytest.mark.parametrize("reg", [1, 2], ids=["always", "on_the_fly"])
def test_wide_block_kernels_regularisation(gpu, orc, reg):
    """Bounded problem with d = 24 blocks (C5 class) under ALWAYS / ON_THE_FLY Levenberg-Marquardt on the wide kernels."""
    f = P.pruned_chain_qp()
    opts = dict(f.opts); opts.update(regType=reg, regValue=1e-6, regTol=1e-6)
    ref = orc.solve(f.as_dict(), orc.default_opts(**opts), lambda0=f.lambda0)
    g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
    r = g.solve(**opts)
    assert r["status"] == ref["status"] == 0 and r["iter"] == ref["iter"] and r["ls_total"] == ref["ls_total"]
    assert_solution_close(g.solution(), ref, TOL)
    g.close()


# --- the wide-block class in three launches per Newton iteration (tdunes_wide3.hpp) -------------

@pytest.mark.parametrize("reg", [0, 1, 2], ids=["no_reg", "always", "on_the_fly"])
def test_three_launch_family_matches_oracle_and_launch_per_phase(gpu, orc, reg):
    """k_sgp / k_hf_w / k_fwd3 (stage + gradient + tails; H + backward sweep + forward preparation; forward sweep + tail) against the
    oracle and against the launch-per-phase kernels they stand in for (TREEQP_AMD_NO_WIDE3=1), on bounded problems with d = 24
    blocks, variable numbers of children, several Newton iterations and line-search trials, under every regularisation mode.
    (On these two problems on-the-fly regularisation shifts no block, at regTol = 1e-3 as little as at 1e-6: the oracle reports
    n_regularized = 0.  The shift-and-refactorise branch of k_hf_w and of the launch-per-phase kernels is pinned by the wide3-* and
    wide-* rows of test_gpu_reg_step.py.)  Same verdict, iteration and trial counts; 3 launches per
    iteration + 1 instead of 11."""
    extra_trials = 0
    for f in (P.pruned_chain_qp(), P.pruned_chain_qp(Nh=6, seed=5)):
        opts = dict(f.opts)
        # (the 83-node tree under a constant shift of 1e-6 is an ill-conditioned case -- the oracle needs 13 iterations and 410
        # trials -- in which no two implementations take the same path: it keeps the 1e-10 of fault_tolerance.c:449-469)
        opts.update(regType=reg, regValue=1e-6 if (reg != 1 or len(f.nk) > 100) else 1e-10, regTol=1e-3 if reg == 2 else 1e-6)
        ref = orc.solve(f.as_dict(), orc.default_opts(**opts), lambda0=f.lambda0)
        r3, s3, _ = _solve_flat_tq(gpu, f.as_dict(), f.lambda0, "generic", **opts)
        os.environ["TREEQP_AMD_NO_WIDE3"] = "1"
        try:
            r1, s1, _ = _solve_flat_tq(gpu, f.as_dict(), f.lambda0, "generic", **opts)
        finally:
            os.environ.pop("TREEQP_AMD_NO_WIDE3", None)
        for r in (r3, r1):
            assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
        assert ref["iter"] >= 3
        extra_trials += ref["ls_total"] - ref["iter"]
        assert_solution_close(s3, ref, TOL)
        assert_solution_close(s1, ref, TOL)
        assert r3["n_launches"] < r1["n_launches"]                                # 3 launches per iteration against 5 (small trees: reductions as sweep tails) or 11
    assert extra_trials > 0                                                        # the cases have what they are meant to exercise


@pytest.mark.parametrize("term", [0, 1], ids=["sum_of_squares", "two_norm"])
def test_three_launch_family_termination_norms(gpu, orc, term):
    """The termination partials of k_sgp are per workgroup (sum of squares) instead of per node: same verdicts as the oracle for the
    norms that are sums (termCondition 0 / 1; the default, the maximum norm, is order-independent)."""
    f = P.pruned_chain_qp()
    opts = dict(f.opts)
    opts.update(termCondition=term, stationarityTolerance=1e-7 if term == 0 else 1e-8)
    ref = orc.solve(f.as_dict(), orc.default_opts(**opts), lambda0=f.lambda0)
    r3, s3, _ = _solve_flat_tq(gpu, f.as_dict(), f.lambda0, "generic", **opts)
    assert (r3["status"], r3["iter"], r3["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]) and ref["status"] == 0
    assert_solution_close(s3, ref, TOL)


def test_three_launch_family_c4_launch_count(gpu, orc):
    """BASELINE config C4 (3280 nodes, 60 x 60 blocks, one Newton iteration): k_sgp, k_hf_w, k_fwd3, k_sgp."""
    f = P.random_clipping_qp()
    g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
    assert g.path == 0
    g.solve(**f.opts)
    r = g.solve(**f.opts)                                                        # (the first solve also runs k_init and enqueues a chunk of iterations ahead)
    assert (r["status"], r["iter"], r["n_launches"]) == (0, 1, 4)
    g.close()


def test_three_launch_family_forward_sweep_without_handovers(gpu, orc, monkeypatch):
    """k_fwd3c (trees of small nodes: every wave recomputes its ancestors' slices of the step instead of waiting for them level by
    level) against k_fwd3 (TREEQP_AMD_NO_FWD_CHAIN=1), and the same computation inside the launch of the first line-search trial
    (k_sgp mode 2; TREEQP_AMD_NO_FWD_MERGE=1 keeps it a launch of its own): the same sums in the same order everywhere -- also the
    reduction of res' dlam -- so verdicts, counts and solutions are identical bit for bit.  Paths of up to 10 blocks (two rounds of path entries), blocks of 8 / 16 / 24 rows, nodes of 1 .. 8
    states; a tree whose paths are longer than 16 blocks keeps k_fwd3 and still agrees with the oracle."""
    cases = [P.pruned_chain_qp(), P.pruned_chain_qp(Nh=6, seed=5), P.random_shape_qp(11, depth=5, max_kids=3, nx_range=(1, 8), nu_range=(1, 3)),
             P.random_shape_qp(12, depth=4, max_kids=2, nx_range=(3, 8), nu_range=(2, 4), ubound=0.2)]
    for f in cases:
        ref = orc.solve(f.as_dict(), orc.default_opts(**f.opts), lambda0=f.lambda0)
        out = []
        # the forward sweep inside the first trial's launch (k_sgp mode 2: two launches per iteration), as a launch of its own without
        # hand-overs (k_fwd3c), with hand-overs (k_fwd3)
        for env in (None, "TREEQP_AMD_NO_FWD_MERGE", "TREEQP_AMD_NO_FWD_CHAIN"):
            monkeypatch.delenv("TREEQP_AMD_NO_FWD_MERGE", raising=False)
            monkeypatch.delenv("TREEQP_AMD_NO_FWD_CHAIN", raising=False)
            if env:
                monkeypatch.setenv(env, "1")
            r, sol, _ = _solve_flat_tq(gpu, f.as_dict(), f.lambda0, "generic", **f.opts)
            assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), (f.name, env, r)
            assert_solution_close(sol, ref, TOL)
            out.append((r, sol))
        monkeypatch.delenv("TREEQP_AMD_NO_FWD_CHAIN", raising=False)
        for o in out[1:]:
            for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
                assert np.array_equal(out[0][1][k], o[1][k]), (f.name, k)
        if out[1][0]["n_launches"] == out[2][0]["n_launches"] and len(f.nk) > 100:      # (the pruned trees: on the three-launch family)
            assert out[0][0]["n_launches"] < out[1][0]["n_launches"]
    deep = P.pruned_chain_qp(Nh=19, seed=3)                                        # 19 stages: paths of 18 blocks
    ref = orc.solve(deep.as_dict(), orc.default_opts(**deep.opts), lambda0=deep.lambda0)
    r, sol, _ = _solve_flat_tq(gpu, deep.as_dict(), deep.lambda0, "generic", **deep.opts)
    assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
    assert_solution_close(sol, ref, TOL)


def test_three_launch_family_verdict_through_the_result_block(gpu, orc, monkeypatch):
    """The last launch of what the host enqueues before it looks posts the control block to pinned host memory (w3_mirror) and the
    host polls for that launch's tag -- no device-to-host copy, no stream synchronisation per read, no HIP event pair per solve.
    Same verdicts, counts and solutions (bit for bit) as with the copy (TREEQP_AMD_NO_W3_MIRROR=1): several iterations with predicted
    and unpredicted further trials (pruned trees, solved repeatedly so that the trial counts of the previous solve are used), a
    solve that is over after its first sweep (started from its own solution: the sweep is not a launch that posts, a one-thread
    launch does), the kernel's own clock as device time, and the event pair when it is asked for."""
    for f in (P.pruned_chain_qp(), P.pruned_chain_qp(Nh=6, seed=5), P.random_shape_qp(5, 2, 6, (3, 9), (2, 5))):
        ref = orc.solve(f.as_dict(), orc.default_opts(**f.opts), lambda0=f.lambda0)
        out = {}
        for mirror in (True, False):
            if mirror:
                monkeypatch.delenv("TREEQP_AMD_NO_W3_MIRROR", raising=False)
            else:
                monkeypatch.setenv("TREEQP_AMD_NO_W3_MIRROR", "1")
            monkeypatch.setenv("TREEQP_AMD_PATH", "generic")
            g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
            monkeypatch.delenv("TREEQP_AMD_PATH")
            assert g.path == 0
            g.event_timing(False)
            rs = [g.solve(**f.opts) for _ in range(3)]                             # the second and third with the first one's trial counts
            for r in rs:
                assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), (mirror, r)
                assert 0.0 < r["device_time"] < 0.05
            sol = g.solution()
            assert_solution_close(sol, ref, TOL)
            g.event_timing(True)
            r = g.solve(**f.opts)
            assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
            assert np.isfinite(g.device_times(1)[0])
            # from its own solution: optimal at the first test, no iteration
            g.event_timing(False)
            g.upload(f.as_dict(), sol["lam"])
            r0 = g.solve(**f.opts)
            assert (r0["status"], r0["iter"]) == (0, 0), r0
            sol0 = g.solution()
            # one iteration allowed, after a solve that took several: the first chunk is the termination test alone, which was the tail
            # of the first sweep -- nothing is launched before the host looks (the one-thread post)
            g.upload(f.as_dict(), f.lambda0)
            g.solve(**f.opts)
            o1 = dict(f.opts); o1["maxIter"] = 1
            r1 = g.solve(**o1)
            assert (r1["status"], r1["iter"]) == (1, 1), r1                       # TREEQP_MAXIMUM_ITERATIONS_REACHED
            out[mirror] = (sol, sol0, g.solution())
            g.close()
        for k in ("x", "u", "lam", "mu_x", "mu_u"):
            assert all(np.array_equal(out[True][i][k], out[False][i][k]) for i in range(3))


# --- full BASELINE sizes: size-independent properties ------------------------------------------

@pytest.mark.parametrize("make", [lambda: P.linear_chain(2, 11, 11)], ids=["c3_chain_4095"])
def test_full_size_lti_properties(gpu, orc, make):
    p = make()
    qp, s, status, ref, flat = solve_lti_both(gpu, orc, p)
    assert status == 0 and qp.info["iter"] == ref["iter"]
    sol = qp.solution()
    assert qp.max_kkt_res() < 1e-8
    # primal feasibility of the dynamics and bounds hold to rounding; multipliers have the right sign
    assert np.all(sol["u"] <= flat["umax"] + 1e-12) and np.all(sol["u"] >= flat["umin"] - 1e-12)
    at_ub = sol["u"] >= flat["umax"]
    assert np.all(sol["mu_u"][at_ub] >= -1e-12) and np.all(np.abs(sol["mu_u"][(~at_ub) & (sol["u"] > flat["umin"])]) < 1e-9)
    assert_solution_close(sol, ref, TOL)
    s.destroy()


def test_full_size_random_c4(gpu, orc):
    f = P.random_clipping_qp()          # nx=20, nu=10, md=3, 8 levels -> 3280 nodes, d = 60
    assert len(f.nk) == 3280
    ref = orc.solve(f.as_dict(), orc.default_opts(**f.opts))
    qp = product_qp_from_flat(gpu, f)
    s = gpu.TdunesSolver(qp, **f.opts)
    status = s.solve()
    assert status == ref["status"] == 0
    assert qp.info["iter"] == ref["iter"] == 1          # unconstrained: one Newton step (random_qp.c:251-253)
    assert qp.max_kkt_res() < 1e-8
    assert_solution_close(qp.solution(), ref, TOL)
    s.destroy()


# --- the reference's own drivers, unchanged, linked against our library --------------------------

def _run_dropin(name, tmp_path):
    exe = ROOT / "oracle" / "_ref" / name
    if not exe.exists():
        pytest.skip(f"{exe} was not built (needs /root/reference at build time)")
    data = tmp_path / "examples" / "spring_mass_utils"
    data.mkdir(parents=True)
    for f in ("x0.txt", "lambda0_tree.txt"):
        shutil.copy(ROOT / "tests" / "golden" / f, data / f)
    env = dict(os.environ, LD_LIBRARY_PATH=str(ROOT / "treeqp_amd" / "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([str(exe)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300), data


def test_dropin_spring_mass_driver(gpu, tmp_path):
    out, data = _run_dropin("spring_mass_tdunes", tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if "Maximum error in KKT residuals" in l][0]
    assert float(line.split()[-1]) < 1e-8               # the driver's own assert (:157)
    assert int((data / "iter.txt").read_text().split()[0]) == 3
    x = np.loadtxt(data / "x_opt.txt")
    assert abs(x[4] - 0.018047417833111958) < 1e-11     # survey probe x[1][0]


def test_dropin_thesis_driver(gpu, tmp_path):
    out, _ = _run_dropin("thesis_example", tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Solver status: 0" in out.stdout and "Number of iterations: 3" in out.stdout


@pytest.mark.parametrize("i", range(6))
def test_dropin_random_qp_driver_goldens(gpu, tmp_path, i):
    """examples/random_qp.c, unchanged, -DDATA=<i>: the reference's own unit test with golden vectors
    (dense Q, S != 0, unconstrained, TREEQP_QPOASES_SOLVER selector).  Its asserts (:249-254): KKT < 1e-12,
    |x - xopt|, |u - uopt| < 1e-12, at most one iteration, status 0 -- they abort the process when violated."""
    out, _ = _run_dropin(f"random_qp_data0{i}", tmp_path)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "SOLVER:\ttdunes" in out.stdout
    its = [l for l in out.stdout.splitlines() if l.startswith("ITERS:")][0]
    assert int(its.split()[-1]) in (0, 1)
    err = [l for l in out.stdout.splitlines() if l.startswith("ERROR:")][0]
    assert float(err.split()[-1]) < 1e-12


# --- fused uniform-tree path (tdunes_fast.hpp) ---------------------------------------------------

FUSED_CASES = [
    ("chain_8_3_2_h4", lambda: P.linear_chain(2, 4, 4)),
    ("chain_8_3_2_h6", lambda: P.linear_chain(2, 6, 6)),
    ("chain_8_3_2_h7_tight", lambda: P.linear_chain(2, 7, 7, ubound=0.2)),
    ("chain_6_2_2_h5", lambda: P.linear_chain(2, 5, 5, nm=3)),
    ("spring_4_1_2_h5", lambda: P.spring_mass(md=2, Nr=5, Nh=5)),
    ("spring_4_1_3_h3", lambda: P.spring_mass(md=3, Nr=3, Nh=3)),
    ("chain_8_3_2_h6_tighter", lambda: P.linear_chain(2, 6, 6, ubound=0.05)),
    # every instantiated (nx, nu, md), single-tier trees, tiers of one level, four tiers
    ("chain_2_1_2_h8", lambda: P.linear_chain(2, 8, 8, nm=1, nu=1)),
    ("chain_8_2_2_h5", lambda: P.linear_chain(2, 5, 5, nm=4, nu=2)),
    ("chain_4_1_3_h5", lambda: P.linear_chain(3, 5, 5, nm=2)),
    ("chain_8_3_2_h2", lambda: P.linear_chain(2, 2, 2)),
    ("chain_4_1_4_h3", lambda: P.linear_chain(4, 3, 3, nm=2)),
    ("chain_8_1_2_h4", lambda: P.linear_chain(2, 4, 4, nm=4, nu=1)),
    ("chain_8_4_2_h4", lambda: P.linear_chain(2, 4, 4, nm=4, nu=4)),
    ("chain_4_2_2_h5", lambda: P.linear_chain(2, 5, 5, nm=2, nu=2)),
    ("chain_4_2_3_h3", lambda: P.linear_chain(3, 3, 3, nm=2, nu=2)),
    ("chain_4_2_4_h3", lambda: P.linear_chain(4, 3, 3, nm=2, nu=2)),
    ("chain_6_1_2_h4", lambda: P.linear_chain(2, 4, 4, nm=3, nu=1)),
    ("chain_6_3_2_h4", lambda: P.linear_chain(2, 4, 4, nm=3, nu=3)),
    ("chain_2_1_4_h3", lambda: P.linear_chain(4, 3, 3, nm=1, nu=1)),                              # four children: d = 16 from nx = 4
    ("chain_8_3_2_h3", lambda: P.linear_chain(2, 3, 3)),
    ("chain_8_3_2_h10", lambda: P.linear_chain(2, 10, 10)),
    ("chain_4_1_4_h5", lambda: P.linear_chain(4, 5, 5, nm=2)),                                    # three tiers of two levels (md = 4): the bottom tier walks down its path through tier 1 (round 4)
    ("chain_4_2_3_h6_tight", lambda: P.linear_chain(3, 6, 6, nm=2, nu=2, ubound=0.1)),            # the same with md = 3 and passes dropped by rejected trials
]


# multistage trees (branching for Nr stages, then one child per node): the reference's setup_multistage_tree(md, Nr, Nh)
MSTAGE_CASES = [
    ("c1_spring_4_1_3_r2_h10", lambda: P.spring_mass()),                              # BASELINE C1
    ("spring_4_1_3_r1_h4", lambda: P.spring_mass(md=3, Nr=1, Nh=4)),
    ("spring_4_1_2_r3_h13", lambda: P.spring_mass(md=2, Nr=3, Nh=13)),                # chains of 10 levels: two stacked chain tiers
    ("chain_8_3_2_r2_h6", lambda: P.linear_chain(2, 2, 6)),
    ("chain_8_3_2_r4_h5", lambda: P.linear_chain(2, 4, 5)),                           # one chain level only
    ("chain_8_2_2_r3_h8_tight", lambda: P.linear_chain(2, 3, 8, nm=4, nu=2, ubound=0.1)),
    ("chain_4_1_4_r2_h6", lambda: P.linear_chain(4, 2, 6, nm=2)),
    ("chain_8_4_2_r2_h6", lambda: P.linear_chain(2, 2, 6, nm=4, nu=4)),
    ("chain_4_2_3_r2_h5", lambda: P.linear_chain(3, 2, 5, nm=2, nu=2)),
]


@pytest.mark.parametrize("name,make", MSTAGE_CASES, ids=[c[0] for c in MSTAGE_CASES])
def test_multistage_tree_persistent_path(gpu, orc, name, make):
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, lambda0=p.lambda0)
    rf, sf, _ = _solve_flat_tq(gpu, flat, p.lambda0, "auto")
    rg, sg, _ = _solve_flat_tq(gpu, flat, p.lambda0, "generic")
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"])
    assert g.path == 2, "multistage trees take the persistent single-launch path"
    g.close()
    assert rf["status"] == rg["status"] == ref["status"] == 0
    assert rf["iter"] == rg["iter"] == ref["iter"] and rf["ls_total"] == rg["ls_total"] == ref["ls_total"]
    assert rf["n_launches"] <= 3 < rg["n_launches"]                             # first solve: reciprocal weights + packed constants + THE launch
    for sol in (sf, sg):
        assert_solution_close(sol, ref, TOL)
        assert orc.max_kkt(flat, sol) < 1e-8
    assert_solution_close(sf, sg, TOL)


def test_multistage_tree_backtracking_and_options(gpu, orc):
    """Far start: Armijo backtracking ends the launch, the host runs the extra trials and relaunches; then ALWAYS regularisation."""
    p = P.spring_mass(md=3, Nr=2, Nh=7)
    flat = oracle_flat_from_lti(orc, p)
    rng = np.random.Generator(np.random.PCG64(11))
    lam0 = 5.0 * rng.standard_normal(len(p.lambda0))
    ref = orc.solve(flat, lambda0=lam0)
    assert ref["status"] == 0 and ref["ls_total"] > ref["iter"], "fixture should need backtracking"
    rf, sf, _ = _solve_flat_tq(gpu, flat, lam0, "auto")
    assert rf["status"] == 0 and rf["iter"] == ref["iter"] and rf["ls_total"] == ref["ls_total"]
    assert_solution_close(sf, ref, TOL)
    for opts in (dict(regType=1, regValue=1e-8), dict(termCondition=1), dict(maxIter=2)):
        ref = orc.solve(flat, orc.default_opts(**opts), p.lambda0)
        rf, sf, _ = _solve_flat_tq(gpu, flat, p.lambda0, "auto", **opts)
        assert rf["status"] == ref["status"] and rf["iter"] == ref["iter"]
        assert_solution_close(sf, ref, TOL)


def _solve_flat_tq(gpu, flat, lambda0, path, **opts):
    os.environ["TREEQP_AMD_PATH"] = path
    try:
        g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, lambda0)
    finally:
        os.environ.pop("TREEQP_AMD_PATH", None)
    r = g.solve(**opts)
    sol = g.solution()
    fused = g.fused
    g.close()
    return r, sol, fused


@pytest.mark.parametrize("name,make", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_path_matches_oracle_and_generic(gpu, orc, name, make):
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, lambda0=p.lambda0)
    rf, sf, fused = _solve_flat_tq(gpu, flat, p.lambda0, "auto")          # persistent single launch
    rt, stt, fused_t = _solve_flat_tq(gpu, flat, p.lambda0, "tiered")     # one launch per tier
    rg, sg, fused_g = _solve_flat_tq(gpu, flat, p.lambda0, "generic")     # one launch per level
    assert fused and fused_t and not fused_g
    assert rf["status"] == rt["status"] == rg["status"] == ref["status"] == 0
    assert rf["iter"] == rt["iter"] == rg["iter"] == ref["iter"]
    assert rf["ls_total"] == rt["ls_total"] == rg["ls_total"] == ref["ls_total"]
    for sol in (sf, stt, sg):
        assert_solution_close(sol, ref, TOL)
        assert orc.max_kkt(flat, sol) < 1e-8
    assert_solution_close(sf, sg, TOL)
    assert_solution_close(stt, sg, TOL)
    # persistent: one launch per solve; the launch-per-tier and launch-per-phase paths need many (the latter fuses the levels of a
    # sweep into one launch since round 2, so it is no longer necessarily above the tiered count)
    assert rf["n_launches"] <= rt["n_launches"] and rf["n_launches"] < rg["n_launches"]


@pytest.mark.parametrize("opts", [dict(regType=0), dict(regType=1, regValue=1e-8), dict(termCondition=0),
                                  dict(termCondition=1), dict(maxIter=2), dict(stationarityTolerance=1e-5)])
def test_fused_path_options(gpu, orc, opts):
    p = P.linear_chain(2, 5, 5)
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, orc.default_opts(**opts), p.lambda0)
    rf, sf, fused = _solve_flat_tq(gpu, flat, p.lambda0, "auto", **opts)
    assert fused
    assert rf["status"] == ref["status"] and rf["iter"] == ref["iter"]
    assert_solution_close(sf, ref, TOL)


def test_fused_path_multi_trial_line_search(gpu, orc):
    """A start far from the solution forces Armijo backtracking: the extra trials run through the
    generic trial kernels while the iteration itself is fused."""
    p = P.linear_chain(2, 6, 6, ubound=0.1)
    flat = oracle_flat_from_lti(orc, p)
    rng = np.random.Generator(np.random.PCG64(2))
    lam0 = 10.0 * rng.standard_normal(len(p.lambda0))
    ref = orc.solve(flat, lambda0=lam0)
    assert ref["status"] == 0 and ref["ls_total"] > ref["iter"], "fixture should need backtracking"
    rf, sf, fused = _solve_flat_tq(gpu, flat, lam0, "auto")
    assert fused and rf["status"] == 0
    assert rf["iter"] == ref["iter"] and rf["ls_total"] == ref["ls_total"]
    assert_solution_close(sf, ref, TOL)


# --- one tree sharded over several (virtual) ranks -----------------------------------------------

SHARD_CASES = [
    ("c3_4095_n2", lambda: P.linear_chain(2, 11, 11), 2),       # BASELINE C3: the configuration north_star shards over 8 GPUs
    ("c3_4095_n4", lambda: P.linear_chain(2, 11, 11), 4),
    ("c3_4095_n8", lambda: P.linear_chain(2, 11, 11), 8),
    ("c2_1023_n2", lambda: P.linear_chain(2, 9, 9), 2),
    ("c2_1023_n4", lambda: P.linear_chain(2, 9, 9), 4),
    ("c2_1023_n8", lambda: P.linear_chain(2, 9, 9), 8),
    ("chain_h7_n2_tight", lambda: P.linear_chain(2, 7, 7, ubound=0.2), 2),
    ("chain_h6_n8", lambda: P.linear_chain(2, 6, 6), 8),
    ("spring_4_1_2_h7_n4", lambda: P.spring_mass(md=2, Nr=7, Nh=7), 4),
]


@pytest.mark.parametrize("name,make,n", SHARD_CASES, ids=[c[0] for c in SHARD_CASES])
def test_sharded_virtual_ranks_match_single_device(gpu, orc, name, make, n):
    """subtrees partitioned over n ranks, replicated top, two small exchanges per Newton
    iteration.  The ranks are mirrors in one process on one GPU (device copies instead of RCCL), which
    exercises the partition lists, workgroup offsets, exchange ranges and the rank-ordered decisions."""
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, lambda0=p.lambda0)
    single, ssol, _ = _solve_flat_tq(gpu, flat, p.lambda0, "auto")
    mirrors = [gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0).shard_init(r, n) for r in range(n)]
    res = gpu.solve_virtual_ranks(mirrors)
    assert res["status"] == ref["status"] == 0
    assert res["iter"] == ref["iter"] == single["iter"]
    assert res["ls_total"] == ref["ls_total"]
    for m in mirrors:                       # every rank ends with the full, identical solution
        sol = m.solution()
        assert_solution_close(sol, ref, TOL)
        assert_solution_close(sol, ssol, 1e-11)
        assert orc.max_kkt(flat, sol) < 1e-8
    for m in mirrors:
        m.close()


@pytest.mark.parametrize("make", [lambda: P.linear_chain(2, 9, 9), lambda: P.linear_chain(2, 11, 11)], ids=["c2", "c3"])
def test_sharded_path_through_rccl_with_one_rank(gpu, orc, make):
    """The RCCL transport of the sharded mode on the one GPU this box has: a ONE-rank communicator (ncclGetUniqueId,
    ncclCommInitRank, grouped in-place ncclAllGather on the solver's stream) carries both exchanges of every Newton iteration
    and the final gather -- the same calls, enqueue order and buffers as with N ranks, with N = 1."""
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, lambda0=p.lambda0)
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    g.shard_init(0, 1, gpu.shard_unique_id())
    assert g.path == 1                                   # sharded: launch-per-tier kernels
    r = g.solve()
    g.shard_gather_solution()
    assert r["status"] == 0 and r["iter"] == ref["iter"] and r["ls_total"] == ref["ls_total"]
    assert_solution_close(g.solution(), ref, TOL)
    g.shard_init(0, 1, gpu.shard_unique_id())           # a second communicator replaces the first (no leak, still correct)
    r = g.solve()
    g.shard_gather_solution()
    assert r["status"] == 0 and r["iter"] == ref["iter"]
    assert_solution_close(g.solution(), ref, TOL)
    g.shard_init(0, 1)                                   # back to the unsharded mirror
    assert g.path == 2 and g.solve()["iter"] == ref["iter"]
    g.close()


def test_sharded_virtual_ranks_backtracking(gpu, orc):
    p = P.linear_chain(2, 6, 6, ubound=0.1)
    flat = oracle_flat_from_lti(orc, p)
    rng = np.random.Generator(np.random.PCG64(2))
    lam0 = 10.0 * rng.standard_normal(len(p.lambda0))
    ref = orc.solve(flat, lambda0=lam0)
    mirrors = [gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, lam0).shard_init(r, 4) for r in range(4)]
    res = gpu.solve_virtual_ranks(mirrors)
    assert res["status"] == 0 and res["iter"] == ref["iter"] and res["ls_total"] == ref["ls_total"]
    assert_solution_close(mirrors[3].solution(), ref, TOL)
    for m in mirrors:
        m.close()


def test_shard_init_rejects_bad_configs(gpu):
    f = P.irregular_clipping_qp()
    g = gpu.TqGpu(f.nk, f.nx, f.nu)
    with pytest.raises(RuntimeError, match="fused"):
        g.shard_init(0, 2)
    g.close()
    p = P.linear_chain(2, 3, 3)
    nx, nu, nk = lti_dims(p)
    g = gpu.TqGpu(nk, nx, nu)
    with pytest.raises(RuntimeError, match="too small"):
        g.shard_init(0, 64)
    g.close()


# ---- dense unconstrained stage solver on the device: the reference's own golden vectors ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("i", range(6))
def test_random_qp_goldens_dense_on_device(gpu, orc, i):
    """examples/random_qp.c + random_qp_utils/data0<i>: dense Q, S != 0, unconstrained, per-node dimensions.
    Same bar as the reference's own asserts (random_qp.c:249-254): |x - xopt|, |u - uopt| < 1e-12, KKT < 1e-12,
    at most one Newton iteration; options of random_qp.c:131-133."""
    f = P.random_qp_fixture(i)
    g = gpu.TqGpu(f["nk"], f["nx"], f["nu"]).upload_dense(f)
    assert g.path == 0                                                          # per-node dense blocks: generic kernels
    r = g.solve(maxIter=10, stationarityTolerance=1e-10, regType=0)
    sol = g.solution()
    g.close()
    assert r["status"] == 0 and r["iter"] in (0, 1)
    assert np.max(np.abs(sol["x"] - f["xopt"])) < 1e-12
    assert np.max(np.abs(sol["u"] - f["uopt"])) < 1e-12
    assert orc.max_kkt(f, sol, dense=True) < 1e-12
    ref = orc.solve_dense(f, orc.default_opts(maxIter=10, stationarityTolerance=1e-10, regType=0))
    assert r["iter"] == ref["iter"]
    assert np.max(np.abs(sol["lam"] - ref["lam"])) < 1e-11


# ---- JSON front end: qp_in.json [init.json] -> qp_out.json -------------------------------

def _run_json_tool(args, tmp_path):
    exe = ROOT / "treeqp_amd" / "lib" / "treeqp_solve_json"
    assert exe.exists(), "treeqp_solve_json was not built"
    out = subprocess.run([str(exe), *map(str, args)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout)


@pytest.mark.parametrize("i", range(6))
def test_json_front_end_replays_reference_fixtures(gpu, tmp_path, i):
    """The reference's unit-test fixtures straight from their JSON files (dense, unconstrained): x, u = goldens to 1e-12."""
    f = P.random_qp_fixture(i)
    d = _run_json_tool([ROOT / "tests" / "golden" / f"random_qp_data0{i}.json"], tmp_path)
    x = np.concatenate([np.atleast_1d(np.asarray(n["x"], dtype=float)) for n in d["solution"]["nodes"]])
    u = np.concatenate([np.atleast_1d(np.asarray(n["u"], dtype=float)) for n in d["solution"]["nodes"]])
    assert d["info"]["solver"] == "tdunes" and d["info"]["status"] == 0 and d["info"]["num_iter"] in (0, 1)
    assert np.max(np.abs(x - f["xopt"])) < 1e-12 and np.max(np.abs(u - f["uopt"])) < 1e-12
    assert d["info"]["kkt_tol"] < 1e-12
    assert len(d["init"]["lam0_tree"]) == int(np.sum(f["nx"][1:]))


def test_json_front_end_clipping_with_init_file(gpu, orc, tmp_path):
    """Clipping stage solver through the wire format: bounds, options, x0 + lam0_tree from the init file, x0 eliminated.
    The tool prints %.17g (round-trip exact) and the oracle solves the SAME x0-eliminated QP from the same duals, so the bar is
    the 1e-10 of every other parity test and the iteration counts agree exactly.  (Earlier rounds compared with the oracle's
    solution of the form that keeps x0 as a node pinned by equal bounds -- an equivalent QP whose iterates differ, so the two
    agreed only to what the stationarity tolerance left: 1e-9 / 1e-8.)"""
    from helpers import flat_to_json
    p = P.spring_mass(md=2, Nr=2, Nh=4)
    flat = oracle_flat_from_lti(orc, p)                                         # x0 pinned by equal bounds on node 0
    flat_e = product_qp_from_lti(gpu, p, eliminate_x0=True).flat()              # what the tool solves after tree_qp_in_eliminate_x0
    assert flat_e["nx"][0] == 0
    rng = np.random.Generator(np.random.PCG64(5))
    lam0 = 0.1 * rng.standard_normal(len(p.lambda0))
    opts = dict(solver="tdunes", maxit=50, stationarityTolerance=1e-9, lineSearchMaxIter=40, lineSearchBeta=0.7, lineSearchGamma=0.1,
                checkLastActiveSet=1, clipping=True, regType="TREEQP_ALWAYS_LEVENBERG_MARQUARDT", regTol=1e-6, regValue=1e-8)
    (tmp_path / "qp_in.json").write_text(json.dumps(flat_to_json(flat, opts)))
    x0 = flat["xmin"][: flat["nx"][0]]
    (tmp_path / "init.json").write_text(json.dumps(dict(x0=list(map(float, x0)), lam0_tree=list(map(float, lam0)))))
    d = _run_json_tool([tmp_path / "qp_in.json", tmp_path / "init.json"], tmp_path)
    ref = orc.solve(flat_e, orc.default_opts(maxIter=50, stationarityTolerance=1e-9, lineSearchMaxIter=40, lineSearchBeta=0.7,
                                             lineSearchGamma=0.1, regType=1, regTol=1e-6, regValue=1e-8), lam0)
    x = np.concatenate([np.atleast_1d(np.asarray(n["x"], dtype=float)) for n in d["solution"]["nodes"]])
    u = np.concatenate([np.atleast_1d(np.asarray(n["u"], dtype=float)) for n in d["solution"]["nodes"]])
    lam = np.concatenate([np.atleast_1d(np.asarray(e["lam"], dtype=float)) for e in d["solution"]["edges"]])
    assert d["info"]["status"] == ref["status"] == 0 and d["info"]["num_iter"] == ref["iter"]
    nx0 = int(flat["nx"][0])
    assert np.array_equal(x[:nx0], x0)                                          # node 0 of the output: the x0 that was eliminated
    assert np.max(np.abs(x[nx0:] - ref["x"])) < 1e-10 and np.max(np.abs(u - ref["u"])) < 1e-10 and np.max(np.abs(lam - ref["lam"])) < 1e-10
    assert np.allclose(d["init"]["lam0_tree"], lam, rtol=0, atol=0)              # tdunes_update_multipliers: the next warm start
    assert d["info"]["kkt_tol"] < 1e-8


# ---- batched multi-tree solve ----------------------------------------------------------

def test_batched_multi_tree_solve_matches_single_solves(gpu, orc):
    """Independent trees (different bounds, sizes, paths) in one batch call == each solved on its own."""
    cases = [P.linear_chain(2, 6, 6), P.linear_chain(2, 6, 6, ubound=0.2), P.linear_chain(2, 7, 7, ubound=0.3),
             P.spring_mass(), P.linear_chain(2, 5, 5, nm=3), P.linear_chain(2, 6, 6, ubound=0.05)]
    flats = [oracle_flat_from_lti(orc, p) for p in cases]
    singles = []
    for p, f in zip(cases, flats):
        g = gpu.TqGpu(f["nk"], f["nx"], f["nu"]).upload(f, p.lambda0)
        singles.append((g.solve(), g.solution()))
        g.close()
    mirrors = [gpu.TqGpu(f["nk"], f["nx"], f["nu"]).upload(f, p.lambda0) for p, f in zip(cases, flats)]
    assert sorted(m.path for m in mirrors) == [2, 2, 2, 2, 2, 2]                # uniform and multistage trees: one persistent launch each
    for _ in range(2):                                                          # twice: hand-over tags must not collide across launches
        res = gpu.solve_batch(mirrors)
    for m, r, (r1, s1), f in zip(mirrors, res, singles, flats):
        sol = m.solution()
        assert r["status"] == r1["status"] == 0 and r["iter"] == r1["iter"] and r["ls_total"] == r1["ls_total"]
        for k in ("x", "u", "lam"):
            assert np.array_equal(sol[k], s1[k])                                # same kernels, same data: bit-identical
        assert orc.max_kkt(f, sol) < 1e-8
        m.close()


def test_batch_of_pruned_trees_is_one_launch(gpu, orc):
    """C5 class (fault_tolerance.c:486-530 keeps one QP per configuration): a batch of independent pruned scenario trees goes
    out as ONE launch, one workgroup per tree; every member must match its own single solve and the oracle."""
    fs = [P.pruned_chain_qp(seed=7 + i) for i in range(6)]
    ms = [gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0) for f in fs]
    opts = fs[0].opts
    single = [m.solve(**opts) for m in ms]
    sols = [m.solution() for m in ms]
    res = gpu.solve_batch(ms, **opts)
    for f, m, r1, s1, rb in zip(fs, ms, single, sols, res):
        ref = orc.solve(f.as_dict(), orc.default_opts(**opts), lambda0=f.lambda0)
        assert rb["status"] == ref["status"] == 0 and rb["iter"] == ref["iter"] == r1["iter"] and rb["ls_total"] == ref["ls_total"]
        assert rb["n_launches"] == 1
        sb = m.solution()
        assert_solution_close(sb, ref, TOL)
        assert_solution_close(sb, s1, TOL)
    for m in ms:
        m.close()


LS_OPTS = [dict(), dict(lineSearchMaxIter=3), dict(lineSearchMaxIter=5, lineSearchRestartTrigger=2), dict(lineSearchBeta=0.3),
           dict(lineSearchBeta=0.9, lineSearchMaxIter=40), dict(lineSearchGamma=0.4), dict(lineSearchMaxIter=1), dict(termCondition=1),
           dict(regType=1, regValue=1e-7)]


@pytest.mark.parametrize("make", [lambda: P.linear_chain(2, 6, 6, ubound=0.1), lambda: P.spring_mass(md=3, Nr=2, Nh=7)], ids=["chain_2_6_6", "multistage_3_2_7"])
def test_persistent_path_line_search_corners(gpu, orc, make):
    """The in-kernel line search (batches of dry trial sweeps) against the oracle: far starts that need backtracking, trial limit
    exhausted, restart trigger, other beta / gamma.  Only runs the oracle itself converges on are compared: a start that defeats
    the method (singular dual Hessian, regularisation-dominated steps of 1e12) has no parity to check."""
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    assert g.path == 2
    compared = backtracked = 0
    for seed in range(3):
        for scale in (3.0, 10.0):
            lam0 = scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(len(p.lambda0))
            for o in LS_OPTS:
                ref = orc.solve(flat, orc.default_opts(**o), lam0)
                if ref["status"] != 0:
                    continue
                g.set_lambda(lam0)
                r = g.solve(**o)
                assert (r["status"], r["iter"], r["ls_total"]) == (0, ref["iter"], ref["ls_total"]), (seed, scale, o)
                assert r["n_launches"] <= 3          # one solve kernel (+ the pack / init kernels of a first solve): no host-run trials
                assert_solution_close(g.solution(), ref, TOL)
                compared += 1
                backtracked += ref["ls_total"] > ref["iter"]
    assert compared >= 30 and backtracked >= 10
    g.close()


def test_mixed_batch_of_all_device_paths(gpu, orc):
    """One batch call over members of every kind -- persistent (uniform, multistage), single-workgroup (small irregular, in LDS or
    not), launch-per-level with the wide-block kernels -- in an order that interleaves them; default options."""
    members = [("uniform", oracle_flat_from_lti(orc, P.linear_chain(2, 6, 6)), None),
               ("pruned_a", P.pruned_chain_qp(seed=11).as_dict(), None),
               ("irregular", P.irregular_clipping_qp().as_dict(), None),
               ("multistage", oracle_flat_from_lti(orc, P.spring_mass()), P.spring_mass().lambda0),
               ("wide", P.random_clipping_qp(nx=10, nu=4, md=3, levels=4).as_dict(), None),
               ("pruned_b", P.pruned_chain_qp(seed=12).as_dict(), None),
               ("thesis", P.thesis_example().as_dict(), None)]
    ms = [gpu.TqGpu(f["nk"], f["nx"], f["nu"]).upload(f, l0) for _, f, l0 in members]
    assert [m.path for m in ms] == [2, 0, 3, 2, 0, 0, 3]
    for _ in range(2):
        res = gpu.solve_batch(ms)
    for (name, f, l0), m, r in zip(members, ms, res):
        ref = orc.solve(f, lambda0=l0)
        assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), name
        assert_solution_close(m.solution(), ref, TOL)
        m.close()


def test_baseline_configs_take_their_intended_device_path(gpu):
    """C1 (multistage), C2, C3 (two workgroups per CU must fit: 293 workgroups) -> one persistent launch; guards against a
    register / LDS regression silently sending C3 back to one launch per tier."""
    for p in (P.spring_mass(), P.linear_chain(2, 9, 9), P.linear_chain(2, 11, 11)):
        nk = p.nk()
        nx = np.full(p.Nn, p.nx, dtype=np.int32)
        nu = np.where(nk > 0, p.nu, 0).astype(np.int32)
        g = gpu.TqGpu(nk, nx, nu)
        assert g.path == 2, p.name
        g.close()


RANDOM_SHAPES = [  # (seed, depth, max_kids, nx range, nu range)
    (1, 3, 3, (1, 4), (1, 3)), (2, 4, 2, (2, 6), (1, 2)), (3, 3, 5, (1, 3), (1, 2)),          # small blocks; parents with five children
    (4, 3, 3, (4, 12), (1, 4)), (5, 2, 6, (3, 9), (2, 5)), (6, 3, 4, (6, 14), (1, 6)),        # blocks of 17..56 rows: the wide kernels, mixed sizes
    (7, 4, 3, (2, 9), (1, 3)), (8, 5, 2, (5, 11), (2, 4)),
]


@pytest.mark.parametrize("seed,depth,kids,nxr,nur", RANDOM_SHAPES, ids=[f"seed{c[0]}_d{c[1]}_k{c[2]}_nx{c[3][1]}" for c in RANDOM_SHAPES])
def test_random_tree_shapes_with_per_node_dimensions(gpu, orc, seed, depth, kids, nxr, nur):
    """Trees of random shape with per-node nx / nu (the class of the irregular probe, scaled up): wave-per-block or workgroup-per-
    block kernels by block size, single-workgroup kernel when small; iteration counts and solution against the oracle."""
    f = P.random_shape_qp(seed, depth, kids, nxr, nur)
    ref = orc.solve(f.as_dict())
    assert ref["status"] == 0
    for path in ("auto", "generic"):
        r, sol, _ = _solve_flat_tq(gpu, f.as_dict(), None, path)
        assert (r["status"], r["iter"], r["ls_total"]) == (0, ref["iter"], ref["ls_total"]), path
        assert_solution_close(sol, ref, TOL)
        assert orc.max_kkt(f.as_dict(), sol) < 1e-8


def test_batch_of_random_tree_shapes(gpu, orc):
    """All the random shapes above as ONE batched call (single-workgroup members share a launch, the others follow)."""
    fs = [P.random_shape_qp(*c) for c in RANDOM_SHAPES]
    ms = [gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), None) for f in fs]
    res = gpu.solve_batch(ms)
    for f, m, r in zip(fs, ms, res):
        ref = orc.solve(f.as_dict())
        assert (r["status"], r["iter"], r["ls_total"]) == (0, ref["iter"], ref["ls_total"]), f.name
        assert_solution_close(m.solution(), ref, TOL)
        m.close()


RANDOM_UNIFORM = [(1, 8, 3, 2, 5, 5), (2, 8, 3, 2, 3, 7), (3, 4, 1, 3, 3, 3), (4, 4, 1, 3, 2, 6), (5, 4, 2, 4, 2, 4), (6, 6, 2, 2, 4, 4),
                  (7, 2, 1, 2, 6, 6), (8, 8, 4, 2, 4, 4), (9, 4, 3, 2, 3, 9), (10, 8, 1, 2, 6, 6), (11, 2, 2, 2, 5, 5), (12, 2, 1, 4, 3, 3)]


@pytest.mark.parametrize("seed,nx,nu,md,Nr,Nh", RANDOM_UNIFORM, ids=[f"seed{c[0]}_{c[1]}_{c[2]}_{c[3]}_r{c[4]}_h{c[5]}" for c in RANDOM_UNIFORM])
def test_persistent_path_on_random_time_varying_data(gpu, orc, seed, nx, nu, md, Nr, Nh):
    """Uniform / multistage shapes with per-edge / per-node random data (no LTI structure): every one needs 4 .. 14 Newton
    iterations with backtracking in most of them -- the whole solve, batched line search included, in one launch."""
    f = P.random_uniform_tree_qp(seed, nx, nu, md, Nr, Nh)
    ref = orc.solve(f.as_dict())
    assert ref["status"] == 0 and ref["ls_total"] > ref["iter"]
    g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), None)
    assert g.path == 2
    for _ in range(2):                                                   # the second solve relaunches on warm hand-over buffers
        r = g.solve()
        assert (r["status"], r["iter"], r["ls_total"]) == (0, ref["iter"], ref["ls_total"])
    sol = g.solution()
    assert_solution_close(sol, ref, TOL)
    assert orc.max_kkt(f.as_dict(), sol) < 1e-8
    g.close()


EDGE_SHAPES = [("one_block_2", lambda: P.linear_chain(2, 1, 1)), ("one_level_then_chain", lambda: P.linear_chain(2, 1, 2)), ("chains_only_9", lambda: P.linear_chain(2, 1, 9)),
               ("two_levels", lambda: P.linear_chain(2, 2, 2)), ("one_block_3", lambda: P.spring_mass(md=3, Nr=1, Nh=1)), ("md3_then_chain", lambda: P.spring_mass(md=3, Nr=1, Nh=2)),
               ("one_block_4", lambda: P.linear_chain(4, 1, 1, nm=2)), ("chains_of_17", lambda: P.linear_chain(2, 3, 20)), ("chains_of_28", lambda: P.spring_mass(md=3, Nr=2, Nh=30))]


@pytest.mark.parametrize("name,make", EDGE_SHAPES, ids=[c[0] for c in EDGE_SHAPES])
def test_smallest_and_longest_shapes(gpu, orc, name, make):
    """One block, one level, chains only, chains of several stacked chain tiers: whatever path the shape takes."""
    p = make()
    flat = oracle_flat_from_lti(orc, p)
    ref = orc.solve(flat, lambda0=p.lambda0)
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    r = g.solve()
    assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
    assert_solution_close(g.solution(), ref, TOL)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 4])
def test_small_block_wide_trees_take_the_three_launch_family(gpu, orc, monkeypatch, seed):
    """Trees of SMALL dual blocks (d <= 16) that are too wide for the single-workgroup kernel (here: a level of more than 96 nodes) run
    on the workgroup-per-block kernels -- three launches per Newton iteration -- since round 4, not on the launch-per-phase kernels
    (TREEQP_AMD_SMALL_WIDE=0): same verdict, iteration and trial counts as the oracle on both, a quarter of the launches."""
    f = P.random_shape_qp(seed, depth=5, max_kids=4, nx_range=(2, 4), nu_range=(1, 2), ubound=0.3)
    ref = orc.solve(f.as_dict(), lambda0=f.lambda0)
    res = {}
    for label in ("three launches", "launch per phase"):
        if label == "launch per phase":
            monkeypatch.setenv("TREEQP_AMD_SMALL_WIDE", "0")
        g = gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
        assert g.path == 0
        g.solve()
        r = g.solve()                          # (the second solve enqueues the first one's trial counts ahead)
        res[label] = (r, g.solution())
        g.close()
        assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), label
        assert_solution_close(res[label][1], ref, TOL)
    assert 2 * res["three launches"][0]["n_launches"] < res["launch per phase"][0]["n_launches"]

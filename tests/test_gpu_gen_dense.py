"""Whole solves of trees with general constraints (device kind 3) through the C-ABI and through the drop-in API (TdunesSolver with
TREEQP_QPOASES_SOLVER on nodes with nc > 0), against the dual Newton method run on the numpy reference (gen_cases.reference_solve):
verdict, iteration count, x, u, lambda and the multipliers to 1e-10, the container's own KKT residual below 1e-8; and an MPC-style
sequence that moves dmin / dmax between solves through the container's setters.  The solves start from the duals of
gen_cases.full_start and stop at gen_cases.FULL_TOL, so that every Armijo and termination decision is clear of rounding (see
gen_cases.reference_solve): only then is the iteration count a property of the method."""
from __future__ import annotations

import numpy as np
import pytest

import gen_cases as GC
import gen_ref as G
import newton_ref as N
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
OPTS = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)
QPOASES = 1


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


@pytest.fixture(scope="module")
def solved():
    cache = {}

    def get(rid):
        if rid not in cache:
            c = GC.case(rid)
            lam0, sol = GC.full_start(rid)
            cache[rid] = dict(_reference(c["d"], c["kinds"], sol), lam0=lam0)
        return cache[rid]
    return get


def _reference(d, kinds, sol):
    assert GC.qualifies(sol)
    it, trials, err, lam, _ = sol
    st = G.stage_solutions(d, lam, kinds)
    x, u, _, _ = N.flat_xu(st)
    mx, mu, md = G.flat_multipliers(d, st)
    return dict(iter=it, trials=trials, x=x, u=u, lam=lam, mu_x=mx, mu_u=mu, mu_d=md)


def _compare(what, sol, ref):
    errs = {k: rel_err(sol[k], ref[k]) for k in ("x", "u", "lam", "mu_x", "mu_u", "mu_d")}
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL


@pytest.mark.parametrize("rid", GC.FULL_IDS)
def test_whole_solve_through_the_c_abi(gpu, solved, rid):
    c, ref = GC.case(rid), solved(rid)
    d = c["d"]
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"]).upload_mixed(d, c["kinds"], ref["lam0"])
    try:
        r = g.solve(**OPTS)
        sol = g.solution()
    finally:
        g.close()
    print(f"{rid}: status {r['status']} iter {r['iter']} (reference {ref['iter']}) trials {r['ls_total']} (reference {ref['trials']})")
    assert r["status"] == 0 and r["iter"] == ref["iter"]
    _compare(rid, sol, ref)
    qp = GC.container_of(gpu, d)
    qp.set_solution(sol)
    assert qp.max_kkt_res() < 1e-8


def _dropin(gpu, d, kinds):
    qp = GC.container_of(gpu, d)
    s = gpu.TdunesSolver(qp, **OPTS)
    for k in range(qp.N):
        s.opts.qp_solver[k] = QPOASES if kinds[k] else 0
    return qp, s


@pytest.mark.parametrize("rid", GC.FULL_IDS)
def test_whole_solve_through_the_dropin_api(gpu, solved, rid):
    c, ref = GC.case(rid), solved(rid)
    qp, s = _dropin(gpu, c["d"], c["kinds"])
    try:
        s.set_dual_initialization(ref["lam0"])
        status = s.solve()
        sol = qp.solution()
        kkt = qp.max_kkt_res()
        it = qp.info["iter"]
    finally:
        s.destroy()
    print(f"{rid}: status {status} iter {it} (reference {ref['iter']}) KKT {kkt:.2e}")
    assert status == 0 and it == ref["iter"]
    _compare(rid, sol, ref)
    assert kkt < 1e-8


def test_mpc_sequence_moving_the_ranges(gpu):
    """five solves of one_row; between them the range of the root's row moves (tree_qp_in_set_node_general_constraints) and the duals
    stay warm (the drop-in solver starts from the previous solve's); each solve against the reference from the same starting duals,
    which must qualify (clear decisions) at every step"""
    c = GC.case("one_row")
    d, kinds = {k: np.array(v, copy=True) for k, v in c["d"].items()}, c["kinds"]
    qp, s = _dropin(gpu, d, kinds)
    Gk, _, _ = G.cons_of(d)[0]
    a = int(d["nx"][0])
    lam = GC.full_start("one_row")[0]
    try:
        s.set_dual_initialization(lam)
        for step in range(5):
            shift = 0.02 * step * (-1) ** step
            d["dmin"], d["dmax"] = c["d"]["dmin"] + shift, c["d"]["dmax"] + shift
            qp.set_node_general_constraints(0, Gk[:, :a], Gk[:, a:], d["dmin"], d["dmax"])
            ref = _reference(d, kinds, GC.reference_solve(d, kinds, lam0=lam))
            status = s.solve()
            sol = qp.solution()
            print(f"step {step}: status {status} iter {qp.info['iter']} (reference {ref['iter']})")
            assert status == 0 and qp.info["iter"] == ref["iter"]
            _compare(f"step {step}", sol, ref)
            assert qp.max_kkt_res() < 1e-8
            lam = sol["lam"]
    finally:
        s.destroy()

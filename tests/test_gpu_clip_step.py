"""The inclusive bound rule of the clipping stage (phase S: x = ub when xUnc >= ub, x = lb when xUnc <= lb, P = 0 exactly on
the entries that are not free) on every device body that has a copy of the comparison, pinned to the numpy reference on the
rows of clip_cases.py, whose unconstrained stage values sit exactly on bounds.  `>` for `>=` exports the same x and u and another
Newton step: test_clip_reference.py shows, without a device, that on every row the step then moves by at least 1e-6 -- for every
single tied entry alone -- while the pin below holds it to 1e-10.  The row id names the route; clip_cases.py and reg_cases.py say
which device body a route runs.

Per row: the plan is the route's; one iteration from the row's lambda0 gives the oracle's verdict and counts, the reference's
step and lambda0 + tau dlam to 1e-10 (reg_cases.TOL; every row has cond <= 1e6 and its untied entries a margin > 1e-6), the
reference's trial count where its Armijo decisions keep a slack of 1e-9.  A whole solve
from the tied start is the oracle's (verdict, iterations, trials, solution to 1e-10).  The mixed row (kinds 0 and 1, which the
oracle does not have) is held to the reference in its one iteration only.  A batch of a tied member and its twin with the tied
bounds moved out by 1e-6 equals the single solves bit for bit.  Two more tests follow: a tie at an accepted trial point (second
step of a two-iteration solve) and a tie at a solution (MPC sensitivities)."""
from __future__ import annotations

import numpy as np
import pytest

import clip_cases as CC
from box_cases import SLACK_MIN
from helpers import assert_solution_close, rel_err
from test_gpu_reg_step import KEYS

pytestmark = pytest.mark.gpu

BETA = CC.RC.BETA


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _set_route(monkeypatch, route):
    for k in CC.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in CC.ROUTES[route][0].items():
        monkeypatch.setenv(k, v)


def _mirror(gpu, c, d=None):
    d = c["d"] if d is None else d
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if c["kinds"] is not None:
        return g.upload_mixed(CC.with_dense_blocks(d), c["kinds"], c["lam0"])
    return g.upload(d, c["lam0"])


def _check_route(g, route):
    _, path, flags = CC.ROUTES[route]
    plan = g.plan
    wrong = {k: (plan[k], v) for k, v in flags.items() if plan[k] != v}
    assert g.path == path and not wrong, f"route {route}: path {g.path} (expected {path}), plan (got, expected) {wrong}"


def _check_step(rid, c, r, sol):
    ref = c["ref"]
    tau = BETA ** (r["ls_total"] - 1)
    e_d, e_l = rel_err(sol["dlam"], ref["dlam"]), rel_err(sol["lam"], c["lam0"] + tau * ref["dlam"])
    print(f"{rid}: status {r['status']} iter {r['iter']} trials {r['ls_total']} (reference {c['trials']}, slack {c['slack']:.2e}) dlam {e_d:.2e} "
          f"lam {e_l:.2e} cond {ref['cond']:.2e}; the exclusive rule would move dlam by {min(c['moved'].values()):.1e} .. {max(c['moved'].values()):.1e}")
    assert e_d <= CC.TOL
    assert e_l <= CC.TOL
    if c["slack"] >= SLACK_MIN:
        assert r["ls_total"] == c["trials"]


def _one_iteration(gpu, orc, monkeypatch, rid, route, c):
    _set_route(monkeypatch, route)
    g = _mirror(gpu, c)
    try:
        _check_route(g, route)
        r = g.solve(maxIter=1, **CC.OPTS)
        sol = g.solution()
    finally:
        g.close()
    if c["kinds"] is None:
        one = orc.solve(c["d"], orc.default_opts(maxIter=1, **CC.OPTS), c["lam0"])
        assert (r["status"], r["iter"], r["ls_total"]) == (one["status"], one["iter"], one["ls_total"])
    else:
        assert (r["status"], r["iter"]) == (1, 1)
    _check_step(rid, c, r, sol)
    return r, sol


@pytest.mark.parametrize("rid", CC.ROW_IDS)
def test_one_iteration_is_the_inclusive_reference_step(gpu, orc, monkeypatch, rid):
    row = CC.row(rid)
    _one_iteration(gpu, orc, monkeypatch, rid, row.route, CC.case(rid))


@pytest.mark.parametrize("rid", CC.COLD_IDS)
def test_cold_start_one_iteration_and_whole_solve(gpu, orc, monkeypatch, rid):
    """umin = 0, r = 0, lambda0 = 0: every input ties in the first iteration; the whole solve has the oracle's counts"""
    route, tree = CC.COLD[rid]
    c = CC.cold_case(orc, tree)
    _one_iteration(gpu, orc, monkeypatch, rid, route, c)
    _whole_solve(gpu, orc, monkeypatch, rid, route, c)


def _whole_solve(gpu, orc, monkeypatch, rid, route, c):
    full = orc.solve(c["d"], orc.default_opts(**CC.OPTS), c["lam0"])
    _set_route(monkeypatch, route)
    g = _mirror(gpu, c)
    try:
        _check_route(g, route)
        r = g.solve(**CC.OPTS)
        sol = g.solution()
    finally:
        g.close()
    print(f"{rid}: whole solve status {r['status']} iter {r['iter']} trials {r['ls_total']} (oracle {full['status']} {full['iter']} {full['ls_total']})")
    assert full["status"] == 0
    assert (r["status"], r["iter"], r["ls_total"]) == (full["status"], full["iter"], full["ls_total"])
    assert_solution_close(sol, full)


@pytest.mark.parametrize("rid", [r.id for r in CC.ROWS if r.kinds is None])
def test_whole_solve_from_the_tied_start_is_the_oracles(gpu, orc, monkeypatch, rid):
    _whole_solve(gpu, orc, monkeypatch, rid, CC.row(rid).route, CC.case(rid))


@pytest.mark.parametrize("rid", CC.BATCH_IDS)
def test_batch_of_a_tied_member_and_its_untied_twin_equals_the_single_solves(gpu, monkeypatch, rid):
    row = CC.row(rid)
    c = CC.case(rid)
    _set_route(monkeypatch, row.route)
    ms = [_mirror(gpu, c, d) for d in (c["d"], c["twin"], c["d"])]
    try:
        singles = []
        for m in ms:
            _check_route(m, row.route)
            r = m.solve(maxIter=1, **CC.OPTS)
            singles.append((r, m.solution()))
            m.set_lambda(c["lam0"])
        res = gpu.solve_batch(ms, maxIter=1, **CC.OPTS)
        sols = [m.solution() for m in ms]
    finally:
        for m in ms:
            m.close()
    _check_step(rid, c, singles[0][0], singles[0][1])
    assert rel_err(singles[1][1]["dlam"], c["ref"]["dlam"]) >= CC.DISCRIMINATION          # the twin's ties are free: another step
    for i, (r, sol, (r1, s1)) in enumerate(zip(res, sols, singles)):
        assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"]), i
        for k in KEYS:
            assert np.array_equal(sol[k], s1[k]), (i, k, float(np.max(np.abs(sol[k] - s1[k]))))


@pytest.mark.parametrize("rid", CC.TRIAL_IDS)
def test_tie_at_the_accepted_trial_point_fixes_the_entry_in_the_next_iteration(gpu, orc, monkeypatch, rid):
    """The trial sweep of the tiered and persistent kernels doubles as phase S of the next iteration.  On the rows of
    clip_cases.trial_case lambda1 = lambda0 + dlam is exact (the dual Hessian at lambda0 is the identity) and some entries tie at
    lambda1: the device's lambda after one iteration IS lambda1, bit for bit, and its second step is the inclusive reference step
    at lambda1, which the exclusive rule would move by at least 1e-6 (test_clip_reference.py)."""
    route, name, _ = rid.split("-")
    c = CC.trial_case(name)
    two = orc.solve(c["d"], orc.default_opts(maxIter=2, **CC.OPTS), c["lam0"])
    _set_route(monkeypatch, route)
    g = _mirror(gpu, c)
    try:
        _check_route(g, route)
        r1 = g.solve(maxIter=1, **CC.OPTS)
        s1 = g.solution()
        g.set_lambda(c["lam0"])
        r2 = g.solve(maxIter=2, **CC.OPTS)
        s2 = g.solution()
    finally:
        g.close()
    ref2 = c["ref2"]
    t2 = r2["ls_total"] - r1["ls_total"]
    e_d, e_l = rel_err(s2["dlam"], ref2["dlam"]), rel_err(s2["lam"], c["lam1"] + BETA ** (t2 - 1) * ref2["dlam"])
    print(f"{rid}: lambda after one iteration differs from the exact lambda1 in {int(np.sum(s1['lam'] != c['lam1']))} entries; second step: trials {t2} "
          f"(reference {c['trials2']}, slack {c['slack2']:.2e}) dlam {e_d:.2e} lam {e_l:.2e}; the exclusive rule would move dlam by "
          f"{min(c['moved'].values()):.1e} .. {max(c['moved'].values()):.1e}")
    assert (r1["status"], r1["iter"], r1["ls_total"]) == (1, 1, 1)
    assert np.array_equal(s1["dlam"], c["ref1"]["dlam"]) and np.array_equal(s1["lam"], c["lam1"])
    assert (r2["status"], r2["iter"], r2["ls_total"]) == (two["status"], two["iter"], two["ls_total"])
    assert e_d <= CC.TOL
    assert e_l <= CC.TOL
    if c["slack2"] >= SLACK_MIN:
        assert t2 == c["trials2"]


def test_sensitivities_treat_a_tied_root_input_as_fixed(gpu):
    """clip_cases.sens_case on the single-workgroup kernel, root with states: lambda0 is the solution exactly, the step takes no iteration
    and its point has input 0 of the root (and three more entries) exactly on a bound.  tqgpu_mpc_sensitivity takes them as fixed: their
    rows of dz/dx0 are 0.0, and K, dx, du are sens_ref.dense_kkt's with that active set, to 10 times the spread of the two numpy
    evaluations (floor 1e-12: the rule of sens_cases.tol); with the ties free K is another matrix (test_clip_reference.py)."""
    import sens_ref as SR
    c = CC.sens_case()
    d = c["d"]
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d, c["lam0"])
    try:
        _check_route(g, "gpersist")
        g.mpc_set_root_states()
        r, u0 = g.mpc_step(c["x0"], **CC.OPTS)
        sol = g.solution()
        n_reg = g.mpc_sensitivity(**CC.OPTS)
        K = g.mpc_gain()[0]
        s = g.mpc_sensitivities()
    finally:
        g.close()
    assert (r["status"], r["iter"]) == (0, 0) and n_reg == 0
    assert np.array_equal(sol["x"], c["x"]) and np.array_equal(sol["u"], c["u"]) and np.array_equal(u0, c["u"][:len(u0)])
    a, b = SR.dense_kkt(d, sol["x"], sol["u"], dict(form="states")), SR.dual_form(d, sol["x"], sol["u"], dict(form="states"), **CC.OPTS)
    spread = max(float(np.max(np.abs(a[w] - b[w]))) for w in ("K", "dx", "du"))
    tol = max(10.0 * spread, 1e-12)
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    for k, e, mode, far in c["ties"]:
        isx, i, _ = CC._slot(d, k, e)
        assert np.all((s["dx"] if isx else s["du"])[i] == 0.0), (k, e)
    assert np.all(K[0] == 0.0) and np.array_equal(K, s["du"][:len(u0)])
    free = SR.dense_kkt(c["twin"], sol["x"], sol["u"], dict(form="states"))
    for what, got in (("K", K), ("dx", s["dx"]), ("du", s["du"])):
        err = float(np.max(np.abs(got - a[what])))
        print(f"sens {what}: |device - dense_kkt| = {err:.2e}, tolerance {tol:.2e}; with the ties free the reference differs by {np.max(np.abs(free[what] - a[what])):.2e}")
        assert err <= tol

"""The regularised block factorisation of every kernel family (phase F: the device bodies of treeqp_dpotrf_l_with_reg_opts)
pinned to the numpy reference of reg_ref.py on the rows of reg_cases.py, in which blocks really are singular.  The row id names
the route, and reg_cases.py says which device body a route runs.

Per row: the plan is the route's; one iteration from the row's lambda0 with the row's options gives the oracle's verdict and
counts, the reference's step to 1e-10 and lambda0 + tau dlam, and the reference's trial
count where its Armijo decisions keep a slack of 1e-9.  Then, per route: a second solve on the same mirror with the pins lifted
gives the unshifted step (no shifted copy, no flag survives a solve), and a batch of a flagged and an unflagged member equals
the two single solves bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import reg_cases as RC
import reg_ref
from box_cases import SLACK_MIN
from helpers import rel_err, with_dense_blocks

pytestmark = pytest.mark.gpu

KEYS = ("x", "u", "lam", "mu_x", "mu_u", "dlam")


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _set_route(monkeypatch, route):
    for k in ("TREEQP_AMD_PATH", "TREEQP_AMD_NO_PERSIST_ONE", "TREEQP_AMD_NO_WIDE3"):
        monkeypatch.delenv(k, raising=False)
    for k, v in RC.ROUTES[route][0].items():
        monkeypatch.setenv(k, v)


def _upload(g, route, d, lam0):
    if route == "dense_single":          # every node of kind 2 (box solver) on the diagonal H
        return g.upload_mixed(with_dense_blocks(d), np.full(len(d["nk"]), 2, np.int32), lam0)
    return g.upload(d, lam0)


def _mirror(gpu, route, d, lam0):
    g = _upload(gpu.TqGpu(d["nk"], d["nx"], d["nu"]), route, d, lam0)
    if route == "dense_single":
        g.set_dense_single_launch(True)
    return g


def _check_route(g, route):
    _, path, flags = RC.ROUTES[route]
    plan = g.plan
    wrong = {k: (plan[k], v) for k, v in flags.items() if plan[k] != v}
    assert g.path == path and not wrong, f"route {route}: path {g.path} (expected {path}), plan (got, expected) {wrong}"


def _check_step(rid, r, sol, lam0, ref, trials, slack, tol):
    tau = RC.BETA ** (r["ls_total"] - 1)
    e_d, e_l = rel_err(sol["dlam"], ref["dlam"]), rel_err(sol["lam"], lam0 + tau * ref["dlam"])
    print(f"{rid}: status {r['status']} iter {r['iter']} trials {r['ls_total']} (reference {trials}, slack {slack:.2e}) dlam {e_d:.2e} "
          f"lam {e_l:.2e} cond {ref['cond']:.2e} flagged {sorted(ref['flagged'])[:8]}")
    assert e_d <= tol
    assert e_l <= RC.TOL
    if slack >= SLACK_MIN:
        assert r["ls_total"] == trials


@pytest.mark.parametrize("rid", RC.ROW_IDS)
def test_one_iteration_is_the_regularised_reference_step(gpu, orc, monkeypatch, rid):
    row = RC.row(rid)
    c = RC.case(rid)
    one = orc.solve(c["d"], orc.default_opts(maxIter=1, **row.opts), c["lam0"])
    _set_route(monkeypatch, row.route)
    g = _mirror(gpu, row.route, c["d"], c["lam0"])
    try:
        _check_route(g, row.route)
        r = g.solve(maxIter=1, **row.opts)
        sol = g.solution()
        if row.route in ("gpersist", "dense_single"):
            assert g.plan["last_single_wg"]
    finally:
        g.close()
    assert (r["status"], r["iter"], r["ls_total"]) == (one["status"], one["iter"], one["ls_total"])
    _check_step(rid, r, sol, c["lam0"], c["ref"], c["trials"], c["slack"], RC.TOL)
    if row.kind == "zero_column":
        assert np.all(sol["dlam"][c["ref"]["zero"]] == 0.0)


LIFT = [r.id for r in RC.ROWS if r.lift]


@pytest.mark.parametrize("rid", LIFT)
def test_no_shift_and_no_flag_survive_a_solve(gpu, monkeypatch, rid):
    """first the flagged row, then the same mirror with the pins lifted (the problem uploaded again, same lambda0, ON_THE_FLY): the
    second step is the reference step of the problem without pins, in which no block is flagged"""
    row = RC.row(rid)
    c = RC.case(rid)
    _set_route(monkeypatch, row.route)
    g = _mirror(gpu, row.route, c["d"], c["lam0"])
    try:
        _check_route(g, row.route)
        r1 = g.solve(maxIter=1, **row.opts)
        s1 = g.solution()
        _upload(g, row.route, c["base"], c["lam0"])
        r2 = g.solve(maxIter=1, **row.opts)
        s2 = g.solution()
    finally:
        g.close()
    _check_step(rid, r1, s1, c["lam0"], c["ref"], c["trials"], c["slack"], RC.TOL)
    free = c["free"]
    trials, slack = reg_ref.armijo(c["base"], c["lam0"], free, RC.LsOpts)
    _check_step(rid + " (pins lifted)", r2, s2, c["lam0"], free, trials, slack, RC.TOL)


@pytest.mark.parametrize("rid", ["persist_one-flag_mid_level-u6", "persist_one-flag_upper_tier-u6", "persist_two-flag_mid_level-u6", "wide3-flag_mid_level", "wide3-flag_root"])
def test_batch_of_a_flagged_and_an_unflagged_member_equals_the_single_solves(gpu, monkeypatch, rid):
    """the property the batch tests assert, on the branch they never reach: tqgpu_solve_batch of the row's problem (a block flagged)
    and of the same problem without pins (none flagged) equals the two single solves bit for bit"""
    row = RC.row(rid)
    c = RC.case(rid)
    _set_route(monkeypatch, row.route)
    ms = [_mirror(gpu, row.route, d, c["lam0"]) for d in (c["d"], c["base"], c["d"])]
    try:
        singles = []
        for m in ms:
            _check_route(m, row.route)
            r = m.solve(maxIter=1, **row.opts)
            singles.append((r, m.solution()))
            m.set_lambda(c["lam0"])
        res = gpu.solve_batch(ms, maxIter=1, **row.opts)
        sols = [m.solution() for m in ms]
    finally:
        for m in ms:
            m.close()
    _check_step(rid, singles[0][0], singles[0][1], c["lam0"], c["ref"], c["trials"], c["slack"], RC.TOL)
    for i, (r, sol, (r1, s1)) in enumerate(zip(res, sols, singles)):
        assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"]), i
        for k in KEYS:
            assert np.array_equal(sol[k], s1[k]), (i, k, float(np.max(np.abs(sol[k] - s1[k]))))

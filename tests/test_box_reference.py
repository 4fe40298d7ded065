"""The reference side of the box-constrained stage solver's pins, without a device: newton_ref.py with per-node kinds (box nodes
included) and the case table box_cases.py, before any device run compares with them.

What is compared with what:
- every row of box_cases.ROWS meets its conditions at its lambda0: cond(M) <= 1e6 (then a float64 solve of the Newton system keeps
  1e6 * 2^-53 ~ 1e-10, the tolerance of the step pins; the bound test_limits_reference.py uses), margin >= 1e-6 (the gap of
  newton_ref.starting_duals: the active set is unambiguous for any implementation good to 1e-6 and the step is smooth), at least
  one active bound on every box node unless the row says otherwise, found within the 20 seeds of starting_duals;
- the reference's box solutions carry their own certificate in longdouble (feasible, g = Hz - h zero on free entries and of the
  right sign on fixed ones, to 1e-13 of |H||z| + |h|), and agree with a search over all working sets on small nodes;
- on problems whose H_k are all diagonal, the step with kinds all 2 is the step with kinds all 0 (a diagonal box QP is solved by
  clipping, inclusive rule included);
- the sign and the constants of the dual function and of the line search come from the CPU oracle, not from the device:
  dual_value with kinds all 0 is the oracle's trace_fval, and armijo_trials is the oracle's trial count on every row of
  limit_shapes.py (kinds 0 and 1).  A trial count is pinned on the device only where every accept/reject decision keeps a slack
  of 1e-9 relative to the sum of the absolute node terms (a float64 sum of those is uncertain by some 1e-14 of it)."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import box_cases as BC
import limit_shapes as S
import newton_ref as N
from helpers import rel_err, with_dense_blocks

LIMIT_CASES = list(S.cases())


@pytest.mark.parametrize("rid", BC.ROW_IDS)
def test_row_meets_its_conditions(rid):
    c = BC.case(rid)
    r, ref = c["row"], c["ref"]
    assert c["seed"] < BC.TRIES
    assert ref["cond"] <= BC.COND_MAX, f"cond(M) = {ref['cond']:.2e}"
    assert ref["margin"] >= BC.GAP, f"margin = {ref['margin']:.2e}"
    assert ref["cert"] <= N.CERT_TOL and c["st1"]["cert"] <= N.CERT_TOL
    for k in np.flatnonzero(c["kinds"] == 2):
        active = int(np.sum(ref["stages"]["side"][k] != 0))
        assert (active == 0) if k in r.inactive_nodes else (active >= 1), f"node {k}: {active} active bounds"
    if r.accept is not None:
        assert r.accept(ref), r.note
    # a box node's P is inv(H_FF) on its free set and zero elsewhere
    for k in np.flatnonzero(c["kinds"] == 2):
        F = ref["stages"]["side"][k] == 0
        Pk = ref["stages"]["P"][k]
        assert not np.any(Pk[~F, :]) and not np.any(Pk[:, ~F])
        if np.any(F):
            Hff = ref["stages"]["H"][k][np.ix_(F, F)]
            assert np.max(np.abs(Pk[np.ix_(F, F)].astype(float) @ Hff - np.eye(int(F.sum())))) < 1e-10


def test_rows_say_what_they_are_about():
    side = lambda rid, k=0: BC.case(rid)["ref"]["stages"]["side"][k]
    nz = lambda rid: int(np.sum(BC.flatten(BC.row(rid).shape)[1:3], axis=0)[0])
    assert [nz(r) for r in ("nz1", "nz2", "nz63", "nz63_last_free", "nz64", "nz64_last_free")] == [1, 2, 63, 63, 64, 64]
    assert side("nz63")[62] != 0 and side("nz64")[63] != 0
    assert side("nz63_last_free")[62] == 0 and side("nz63_last_free")[61] != 0
    assert side("nz64_last_free")[63] == 0 and side("nz64_last_free")[62] != 0
    assert not np.any(side("none_active")) and not np.any(side("none_active", 1))
    assert np.all(side("all_inputs_fixed")[8:] != 0) and not np.any(side("all_inputs_fixed")[:8])
    d = BC.case("equal_bounds")["d"]
    lo, hi = np.concatenate([d["xmin"][4:12], d["umin"][2:6]]), np.concatenate([d["xmax"][4:12], d["umax"][2:6]])
    assert sorted(np.flatnonzero(lo == hi).tolist()) == [1, 5, 10] and np.all(side("equal_bounds", 1)[[1, 5, 10]] != 0)
    Hk = BC.case("equal_bounds")["ref"]["stages"]["H"][1]
    assert np.all(np.abs(Hk[[1, 5, 10], :]).sum(axis=1) - np.abs(np.diag(Hk)[[1, 5, 10]]) > 0.1)          # coupled off the diagonal
    for rid, far in (("one_sided", "min"), ("one_sided_mirror", "max")):
        d = BC.case(rid)["d"]
        v = np.abs(np.concatenate([d["x" + far][:8], d["u" + far]]))
        assert np.all(np.isinf(v[0::2])) and np.all(v[1::2] == 1e12)
        assert int(np.sum(side(rid) != 0)) >= 3
    # tie: the root's data are invariant under swapping entries 2i and 2i + 1
    c = BC.case("tie")
    d, Hk = c["d"], c["ref"]["stages"]["H"][0]
    sw = np.arange(8) ^ 1
    assert np.array_equal(Hk, Hk[np.ix_(sw, sw)]) and np.array_equal(c["ref"]["stages"]["h"][0], c["ref"]["stages"]["h"][0][sw])
    lo, hi = np.concatenate([d["xmin"][:4], d["umin"][:4]]), np.concatenate([d["xmax"][:4], d["umax"][:4]])
    assert np.array_equal(lo, lo[sw]) and np.array_equal(hi, hi[sw]) and np.array_equal(side("tie"), side("tie")[sw])
    assert int(np.sum(side("tie") != 0)) >= 2
    assert set(BC.case("mixed")["kinds"].tolist()) == {0, 1, 2} and 12 <= len(BC.case("mixed")["kinds"]) <= 20
    assert int(np.max(np.sum(BC.flatten(BC.row("mixed").shape)[1:3], axis=0))) <= 18
    assert BC.case("x0_eliminated")["d"]["nx"][0] == 0


def test_pins_the_issue_asks_for_are_in_the_table():
    """x, u are pinned at the accepted point at least on nz64, mixed and equal_bounds; at least two rows pin a trial count of
    two or more."""
    for rid in BC.XU_PIN_REQUIRED:
        assert BC.case(rid)["xu_pin"], rid
    multi = [rid for rid in BC.ROW_IDS if BC.case(rid)["trials"] >= 2 and BC.case(rid)["slack"] >= BC.SLACK_MIN]
    assert len(multi) >= 2, multi


@pytest.mark.parametrize("rid", BC.ROW_IDS)
def test_row_is_a_feasible_qp(rid):
    """the dual Newton method of the reference itself ends on every row from lambda = 0"""
    c = BC.case(rid)
    it, trials, err, _ = BC.reference_solve(c["d"], c["kinds"])
    assert err <= 1e-10, f"residual {err:.2e} after {it} iterations"


@pytest.mark.parametrize("rid", BC.PATH_ROWS)
def test_path_rows_have_their_two_duals(rid):
    lamA, lamB, counts = BC.path_duals(rid)
    assert min(counts["released"], counts["added"], counts["swapped"]) >= 1, counts
    nbox = sum(len(s) for s, k in zip(BC.case(rid)["st1"]["side"], BC.case(rid)["kinds"]) if k == 2)
    assert counts["active_A"] >= 0.15 * nbox, counts


# ---------------------------------------------------------------------------------------------------------------------------
# the box solver of the reference against a search over all working sets
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_box_solution_is_the_best_vertex_of_all_working_sets(seed):
    """nz = 5: each of the 3^5 assignments (lower, free, upper) gives one candidate; the solution is the feasible candidate of
    least objective"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 5
    Mx = rng.standard_normal((n, n))
    Hk = np.diag(0.5 + rng.random(n)) + 0.3 * Mx @ Mx.T
    h = 2.0 * rng.standard_normal(n)
    lo, hi = -0.2 - rng.random(n), 0.2 + rng.random(n)
    if seed % 2:
        lo[0], hi[1] = -np.inf, np.inf
    z, side = N.solve_box(Hk, h, lo, hi)
    v, _ = N.certify_box(Hk, h, lo, hi, z, side)
    assert v <= N.CERT_TOL
    best, zbest = np.inf, None
    for assign in itertools.product((-1, 0, 1), repeat=n):
        a = np.asarray(assign)
        zc = np.where(a < 0, lo, np.where(a > 0, hi, 0.0))
        if not np.all(np.isfinite(zc)):
            continue
        F = a == 0
        if np.any(F):
            zc[F] = np.linalg.solve(Hk[np.ix_(F, F)], h[F] - Hk[np.ix_(F, ~F)] @ zc[~F])
        if np.all(zc >= lo - 1e-13) and np.all(zc <= hi + 1e-13):
            f = 0.5 * zc @ Hk @ zc - h @ zc
            if f < best:
                best, zbest = f, zc
    assert np.max(np.abs(zbest - z.astype(float))) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# diagonal problems: kind 2 is clipping
# ---------------------------------------------------------------------------------------------------------------------------

def test_lands_on_bound_row():
    c = BC.lands_on_bound()
    d, ref = c["d"], c["ref"]
    assert ref["cond"] <= BC.COND_MAX and ref["margin"] == 0.0
    zu = BC.unconstrained_values(d, np.zeros(3, int), c["lam0"])
    st = ref["stages"]
    for k, i in c["landed"]:
        lo = np.concatenate([d["xmin"][2 * k:2 * k + 2], d["umin"] if k == 0 else []])
        hi = np.concatenate([d["xmax"][2 * k:2 * k + 2], d["umax"] if k == 0 else []])
        assert zu[k][i] == lo[i] or zu[k][i] == hi[i]
        assert st["side"][k][i] != 0                       # inclusive: a stage value ON its bound is fixed
    assert set(np.concatenate([d["Qd"], d["Rd"]]).tolist()) <= {1.0, 4.0, 16.0}
    box = N.newton_step(d, c["lam0"], kinds=c["kinds"])
    assert all(np.array_equal(a, b) for a, b in zip(box["stages"]["side"], st["side"]))
    assert np.array_equal(box["dlam"], ref["dlam"]) and np.array_equal(box["res"], ref["res"])


@pytest.mark.parametrize("cid", ["wide_class-d17", "k_sgp_children-kids5", "g_persist_node_sizes-nz17"])
def test_diagonal_box_step_is_the_clipping_step(cid):
    kind, shape, _ = S.case(cid)
    d = with_dense_blocks(S.problem(kind, shape))
    lam0, clip = N.starting_duals(d)
    Nn = len(d["nk"])
    box = N.newton_step(d, lam0, kinds=np.full(Nn, 2))
    viak = N.newton_step(d, lam0, kinds=np.zeros(Nn, int))
    assert np.array_equal(viak["dlam"], clip["dlam"])
    assert all(np.array_equal(a, b) for a, b in zip(box["stages"]["side"], clip["stages"]["side"]))
    assert rel_err(box["dlam"], clip["dlam"]) <= 1e-13 and rel_err(box["res"], clip["res"]) <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# sign and constants of the dual function and the line search: from the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid,kind,shape,flags", LIMIT_CASES, ids=[c[0] for c in LIMIT_CASES])
def test_dual_value_and_trials_are_the_oracles(orc, cid, kind, shape, flags):
    """one iteration of the oracle from lambda0: its trial count is armijo_trials, and (clipping rows, where it keeps a trace) the
    dual value it ends on is dual_value at its new lambda"""
    d = S.problem(kind, shape)
    dense = kind == S.D
    lam0, ref = N.starting_duals(d, dense)
    opts = orc.default_opts(maxIter=1, regType=0)
    got = orc.solve_dense(d, opts, lam0) if dense else orc.solve(d, opts, lam0)
    trials, slack = N.armijo_trials(d, lam0, ref["dlam"], ref["res"], opts, dense=dense)
    assert slack >= BC.SLACK_MIN, f"slack {slack:.2e}: the count is decided by rounding"
    assert trials == (got["ls_total"] if dense else int(got["trace_ls"][0]))
    if not dense:
        terms = N.dual_terms(d, got["lam"])
        assert abs(float(terms.sum()) - got["trace_fval"][0]) <= 1e-12 * float(np.abs(terms).sum())


def test_armijo_trials_backtracks_as_the_oracle_does(orc):
    """a row where the oracle needs more than one trial (lambda0 far from the optimum)"""
    kind, shape, _ = S.case("wide_class-d17")
    d = S.problem(kind, shape)
    found = 0
    for s in range(20):
        lam0 = N.seeded_duals(int(d["nx"][1:].sum()), s, 3.0)
        ref = N.newton_step(d, lam0)
        if ref["margin"] < BC.GAP or ref["cond"] > BC.COND_MAX:
            continue
        opts = orc.default_opts(maxIter=1, regType=0)
        got = orc.solve(d, opts, lam0)
        trials, slack = N.armijo_trials(d, lam0, ref["dlam"], ref["res"], opts)
        if slack >= BC.SLACK_MIN and got["status"] == 1:
            assert trials == int(got["trace_ls"][0])
            found += trials >= 2
    assert found >= 1

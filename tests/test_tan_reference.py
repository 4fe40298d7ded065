"""The two numpy evaluations of tan_ref.py against each other, against adj_ref.py and sens_ref.py, and against the oracle's finite changes,
on the CPU.

Per case (tan_cases.py), at the oracle's solve with stationarityTolerance 1e-12: (a) and (b) agree within the spreads kept in
tan_cases.SPREAD (dlam where the block form regularises nothing); with db = dx0 = None the tangent is the adjoint of adj_ref for w = dh
(symmetry of the KKT system); sum w . dZ = gq . dq + gr . dr + gb . db + gx0 . dx0 (duality); dx0 = e_j alone gives column j of
sens_ref; three columns are three calls; and z(theta + dtheta, x0 + dx0) - z(theta, x0) from two oracle solves matches dZ on the cases
where the sets of bound-sitting entries are equal at both points (the test verifies that itself; at most a third of the cases may drop
out).  The predictor's cases (tan_cases.TRACK_IDS) get the same two checks for the direction of a window move and an x0 change.

Bounds of the comparisons between modules: the sum of what each side is known to within (its own spread table), doubled as everywhere
("another BLAS may sum in another order"), weighted with the 1-norm of the vector it is multiplied with, plus 1e-15."""
import functools

import numpy as np
import pytest

import adj_cases as AC
import adj_ref as AR
import sens_ref as SR
import tan_cases as TN
import tan_ref as TR


def _case_modules():
    """imported where a test runs: mpc_cases loads the native library on import (adj_cases says more)"""
    import mpc_limit_cases as ML
    import sens_cases as SN
    return ML, SN


@functools.lru_cache(maxsize=None)
def _solved(cid):
    ML, SN = _case_modules()
    import oracle_py as orc
    return SN.oracle_solve(orc, TN.case(cid))


@functools.lru_cache(maxsize=None)
def _both(cid):
    c, s = TN.case(cid), _solved(cid)
    return tuple(fn(c["d"], s["x"], s["u"], c["param"], c["dirs"], c["kinds"]) for fn in (TR.dense_kkt, TR.dual_form))


def _spread(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def _check_spreads(cid, a, b, recorded):
    assert b["in_range"] < 1e-10 and b["n_reg"] == 0
    assert a["residual"] < 1e-9 * a["scale"], a["residual"]
    for i, what in enumerate(("dx", "du", "dlam", "du0")):
        assert a[what].shape == b[what].shape
        spread = _spread(a[what], b[what])
        print(f"{cid} {what}: spread {spread:.3e} (recorded {recorded[i]:.1e})")
        assert spread <= 2.0 * recorded[i] + 1e-16, (what, spread)          # (2 x: another BLAS may sum in another order)


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_the_two_evaluations_agree(orc, cid):
    c = TN.case(cid)
    for v in c["dirs"]:
        assert np.array_equal(v * 2.0 ** 22, np.round(v * 2.0 ** 22)) and v.any() and np.max(np.abs(v)) <= TN.FD_H
    _check_spreads(cid, *_both(cid), TN.SPREAD[cid])


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_symmetry_with_the_adjoint(orc, cid):
    """tangent(dq, dr, None, None) is (gq, gr, gb) of the adjoint for w = (dq, dr): one matrix, one right-hand side"""
    c, s = TN.case(cid), _solved(cid)
    dq, dr = c["dirs"][:2]
    t = TR.dual_form(c["d"], s["x"], s["u"], c["param"], (dq, dr, None, None), c["kinds"])
    g = AR.dual_form(c["d"], s["x"], s["u"], c["param"], (dq, dr), c["kinds"])
    for mine, theirs in (("dx", "gq"), ("du", "gr"), ("dlam", "gb")):
        assert np.array_equal(t[mine], g[theirs]), mine          # the same numpy expressions in the same order


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_duality(orc, cid):
    c, s = TN.case(cid), _solved(cid)
    a = _both(cid)[0]
    g = AR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"])
    wx, wu = c["w"]
    dq, dr, db, dx0 = c["dirs"]
    got = float(wx[:, 0] @ a["dx"][:, 0] + wu[:, 0] @ a["du"][:, 0])
    want = float(g["gq"][:, 0] @ dq[:, 0] + g["gr"][:, 0] @ dr[:, 0] + g["gb"][:, 0] @ db[:, 0] + g["gx0"][:, 0] @ dx0[:, 0])
    n1 = lambda *v: float(sum(np.sum(np.abs(x)) for x in v))
    sp, sa = TN.SPREAD[cid], AC.SPREAD[cid]
    bound = 2.0 * max(sp[0], sp[1]) * n1(wx, wu) + 2.0 * max(sa[:4]) * n1(dq, dr, db, dx0) + 1e-15
    print(f"{cid}: |w . dZ - g . dtheta| = {abs(got - want):.3e}, bound {bound:.3e}")
    assert abs(got - want) <= bound


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_unit_dx0_gives_the_columns_of_the_sensitivity(orc, cid):
    ML, SN = _case_modules()
    c, s = TN.case(cid), _solved(cid)
    fwd = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    t = TR.dense_kkt(c["d"], s["x"], s["u"], c["param"], (None, None, None, np.eye(int(c["nx0"]))), c["kinds"])
    sens = SN.SPREAD[cid][:4] if cid in SN.SPREAD else ML.SPREAD[cid]
    bound = 2.0 * max(TN.SPREAD[cid][0], TN.SPREAD[cid][1]) / TN.FD_H + 2.0 * max(sens[1], sens[2]) + 1e-15          # (the table's spreads are of directions of size FD_H)
    for what in ("dx", "du"):
        err = _spread(t[what], fwd[what])
        print(f"{cid} {what}: |tangent(e_j) - dZ/dx0| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("cid", TN.ND3)
def test_three_columns_are_three_calls(orc, cid):
    c, s = TN.case(cid), _solved(cid)
    all3 = TR.dual_form(c["d"], s["x"], s["u"], c["param"], c["dirs3"], c["kinds"])
    assert all3["dx"].shape[1] == 3
    for j in range(3):
        one = TR.dual_form(c["d"], s["x"], s["u"], c["param"], tuple(v[:, j] for v in c["dirs3"]), c["kinds"])
        for what in ("dx", "du", "dlam"):
            assert np.allclose(one[what][:, 0], all3[what][:, j], rtol=0, atol=1e-18 + 4 * np.finfo(float).eps * np.max(np.abs(all3[what])))


@functools.lru_cache(maxsize=None)
def _finite_change(cid):
    """(the set of bound-sitting entries is the same at both points, max |z1 - z0 - dZ|)"""
    ML, SN = _case_modules()
    import oracle_py as orc
    c, s = TN.case(cid), _solved(cid)
    _, x1 = TN.problem_plus(c)
    d1 = SN.problem_at(c, x1)
    for k, dv in zip(("q", "r", "b"), c["dtheta"]):
        d1[k] = d1[k] + dv
    s1 = SN.oracle_solve(orc, c, d1)
    assert s1["status"] == 0
    same = np.array_equal(SR.pinned(c["d"], s["x"], s["u"], c["kinds"]), SR.pinned(d1, s1["x"], s1["u"], c["kinds"]))
    a = _both(cid)[0]
    err = max(_spread(s1["x"] - s["x"], a["dx"][:, 0]), _spread(s1["u"] - s["u"], a["du"][:, 0]))
    return same, err


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_against_the_oracle_finite_change(orc, cid):
    same, err = _finite_change(cid)
    rec = TN.SPREAD[cid][4]
    print(f"{cid}: set unchanged {same}, |z1 - z0 - dZ| = {err:.3e} (recorded {rec})")
    assert (rec is not None) == same, "the table's drop-outs no longer match"
    if same:
        assert err <= 2.0 * rec + 1e-16


def test_at_most_a_third_of_the_cases_drop_out(orc):
    dropped = [cid for cid in TN.CASE_IDS if not _finite_change(cid)[0]]
    print("dropped:", dropped)
    assert 3 * len(dropped) <= len(TN.CASE_IDS)
    dropped_t = [cid for cid in TN.TRACK_IDS if not _track(cid)[2]]
    assert 3 * len(dropped_t) <= len(TN.TRACK_IDS)


@functools.lru_cache(maxsize=None)
def _track(cid):
    """the predictor's direction on a tracking case: ((a), (b), set unchanged, max |z1 - z0 - dZ|)"""
    ML, SN = _case_modules()
    import adjbnd_cases as BC
    import oracle_py as orc
    c = TN.track_case(cid)
    t0, t1 = c["move"]
    d0, d1 = BC.folded(c, t0), BC.folded(dict(c, x0=c["x0_new"]), t1)
    s0, s1 = SN.oracle_solve(orc, c, d0), SN.oracle_solve(orc, c, d1)
    assert s0["status"] == 0 == s1["status"]
    dq, dr = TR.window_direction(c, t0, t1)
    dirs = (dq, dr, None, c["x0_new"] - c["x0"])
    a, b = (fn(d0, s0["x"], s0["u"], c["param"], dirs, c["kinds"]) for fn in (TR.dense_kkt, TR.dual_form))
    same = np.array_equal(SR.pinned(d0, s0["x"], s0["u"], c["kinds"]), SR.pinned(d1, s1["x"], s1["u"], c["kinds"]))
    err = max(_spread(s1["x"] - s0["x"], a["dx"][:, 0]), _spread(s1["u"] - s0["u"], a["du"][:, 0]))
    return a, b, same, err


@pytest.mark.parametrize("cid", TN.TRACK_IDS)
def test_the_predictor_direction(orc, cid):
    import adjbnd_cases as BC
    c = TN.track_case(cid)
    a, b, same, err = _track(cid)
    rec = TN.TRACK_SPREAD[cid]
    _check_spreads(cid, a, b, rec)
    # the direction is the difference of the two folds, to the rounding of the folds themselves
    t0, t1 = c["move"]
    dq, dr = TR.window_direction(c, t0, t1)
    import tracking_cases as TC
    (q0, r0, bq, br), (q1, r1, _, _) = TC.fold(c, t0, c["x0"] if c["form"] == "elim" else None, bound=True), TC.fold(c, t1, c["x0"] if c["form"] == "elim" else None, bound=True)
    assert np.all(np.abs((q1 - q0) - dq) <= 4.0 * bq + 1e-300) and np.all(np.abs((r1 - r0) - dr) <= 4.0 * br + 1e-300)
    assert np.any(dq != 0.0) or np.any(dr != 0.0)
    print(f"{cid}: set unchanged {same}, |z1 - z0 - dZ| = {err:.3e} (recorded {rec[4]})")
    assert (rec[4] is not None) == same, "the table's drop-outs no longer match"
    if same:
        assert err <= 2.0 * rec[4] + 1e-16


def test_the_cases_are_those_of_the_tables():
    ML, SN = _case_modules()
    import adjbnd_cases as BC
    assert set(TN.CASE_IDS) <= set(AC.CASE_IDS) and set(TN.CASE_IDS) == set(TN.SPREAD) and set(TN.ND3) <= set(TN.CASE_IDS)
    assert set(TN.TRACK_IDS) <= set(BC.TRACK_IDS) and set(TN.TRACK_IDS) == set(TN.TRACK_SPREAD)
    assert {TN.case(cid)["form"] for cid in TN.ND3} == {"eliminated", "states"} and all(v.shape[1] == 3 for cid in TN.ND3 for v in TN.case(cid)["dirs3"])
    assert {TN.track_case(cid)["form"] for cid in TN.TRACK_IDS} == {"elim", "states"}
    assert TN.track_case("kind1_S0")["root"]["S0"] is not None and (TN.WINDOW_ID, TN.WINDOW_ND) == (AC.WINDOW_ID, AC.WINDOW_NW)

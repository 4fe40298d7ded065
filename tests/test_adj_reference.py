"""The two numpy evaluations of adj_ref.py against each other, against the forward sensitivities of sens_ref.py and against the oracle's
finite differences, on the CPU.

Per case (adj_cases.py), at the oracle's solve with stationarityTolerance 1e-12: the conditions test_sens_reference.py asserts (status 0;
on clipping trees at least one bound active and one entry free below the root, strict complementarity; the lstsq residual at rounding
level); (a) and (b) agree within the spreads kept in adj_cases.SPREAD (gb where the block form regularises nothing); gx0 = dZ' w with dZ
of sens_ref.dense_kkt; wu = e_i on the root's inputs gives row i of K; and w' (z(theta + dtheta) - z(theta)) from two oracle solves
matches g' dtheta for a direction in q, r, b of size 2^-16.

The two comparisons with sens_ref are between (a) of either module, two lstsq solves of one matrix and its transpose.  Their bound is
the sum of what each side is known to within: the adjoint's own spread of gx0, and the spread of dx, du (of K) of the sensitivity tables
weighted with the 1-norm of w (1 for e_i), both doubled as everywhere ("another BLAS may sum in another order"), plus 1e-15."""
import functools

import numpy as np
import pytest

import adj_cases as AC
import adj_ref as AR
import sens_ref as SR


def _case_modules():
    """(mpc_limit_cases, sens_cases), imported where a test runs: mpc_cases loads the native library on import, and this module is
    collected ahead of the ones that decide which HIP runtime the process gets (adj_cases says more)"""
    import mpc_limit_cases as ML
    import sens_cases as SN
    return ML, SN


@functools.lru_cache(maxsize=None)
def _solved(cid):
    ML, SN = _case_modules()
    import oracle_py as orc
    return SN.oracle_solve(orc, AC.case(cid))


def _sens_spread(cid):
    ML, SN = _case_modules()
    return SN.SPREAD[cid][:4] if cid in SN.SPREAD else ML.SPREAD[cid]


@functools.lru_cache(maxsize=None)
def _both(cid):
    c, s = AC.case(cid), _solved(cid)
    return (AR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"]), AR.dual_form(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"]))


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_case_is_valid(orc, cid):
    c, s = AC.case(cid), _solved(cid)
    assert s["status"] == 0
    on = SR.pinned(c["d"], s["x"], s["u"], c["kinds"])
    below = on[c["nx0"] if c["form"] == "states" else 0:]
    if c["kinds"] is None:
        assert below.any() and not below.all()
        mu = np.concatenate([s["mu_x"], s["mu_u"]])[c["nx0"] if c["form"] == "states" else 0:]
        assert np.all(np.abs(mu[below]) > 1e-6)
    a = _both(cid)[0]
    assert a["residual"] < 1e-9 * a["scale"], a["residual"]
    for v in c["w"] + ((c["w3"]) if "w3" in c else ()):
        assert np.array_equal(v * 64.0, np.round(v * 64.0)) and v.any()


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_the_two_evaluations_agree(orc, cid):
    a, b = _both(cid)
    assert b["in_range"] < 1e-10
    for i, what in enumerate(("gq", "gr", "gb", "gx0")):
        if what == "gb" and b["n_reg"] != 0:
            continue
        assert a[what].shape == b[what].shape
        spread = float(np.max(np.abs(a[what] - b[what]))) if a[what].size else 0.0
        print(f"{cid} {what}: spread {spread:.3e} (recorded {AC.SPREAD[cid][i]:.1e})")
        assert spread <= 2.0 * AC.SPREAD[cid][i] + 1e-16, (what, spread)          # (2 x: another BLAS may sum in another order)
    assert b["n_reg"] == 0


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_gx0_is_the_forward_sensitivity_applied_to_w(orc, cid):
    c, s = AC.case(cid), _solved(cid)
    fwd = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    W = np.vstack(c["w"])
    want = np.vstack([fwd["dx"], fwd["du"]]).T @ W
    sp = _sens_spread(cid)
    bound = 2.0 * AC.SPREAD[cid][3] + 2.0 * max(sp[1], sp[2]) * float(np.sum(np.abs(W))) + 1e-15
    err = float(np.max(np.abs(_both(cid)[0]["gx0"] - want)))
    print(f"{cid}: |gx0 - dZ' w| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_unit_vectors_on_the_root_inputs_give_the_rows_of_K(orc, cid):
    c, s = AC.case(cid), _solved(cid)
    nu0 = int(c["d"]["nu"][0])
    K = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])["K"]
    wu = np.zeros((int(np.sum(c["d"]["nu"])), nu0))
    wu[np.arange(nu0), np.arange(nu0)] = 1.0
    bound = 2.0 * AC.SPREAD[cid][3] + 2.0 * _sens_spread(cid)[0] + 1e-15
    for name, fn in (("(a)", AR.dense_kkt), ("(b)", AR.dual_form)):
        g = fn(c["d"], s["x"], s["u"], c["param"], (None, wu), c["kinds"])["gx0"]
        err = float(np.max(np.abs(g.T - K)))
        print(f"{cid} {name}: |gx0(e_i) - K[i]| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_gradients_against_the_oracle_finite_difference(orc, cid):
    ML, SN = _case_modules()
    c, s = AC.case(cid), _solved(cid)
    d1 = AC.problem_plus(c)
    s1 = SN.oracle_solve(orc, c, d1)
    assert s1["status"] == 0
    assert np.array_equal(SR.pinned(c["d"], s["x"], s["u"], c["kinds"]), SR.pinned(d1, s1["x"], s1["u"], c["kinds"])), "the active set changed: dtheta is too large"
    a = _both(cid)[0]
    wx, wu = c["w"]
    dq, dr, db = c["dtheta"]
    got = float(wx[:, 0] @ (s1["x"] - s["x"]) + wu[:, 0] @ (s1["u"] - s["u"]))
    want = float(a["gq"][:, 0] @ dq + a["gr"][:, 0] @ dr + a["gb"][:, 0] @ db)
    err = abs(got - want)
    print(f"{cid}: |w' dz - g' dtheta| = {err:.3e} (recorded {AC.SPREAD[cid][4]:.1e})")
    assert err <= 2.0 * AC.SPREAD[cid][4] + 1e-16


def test_the_cases_cover_the_limits():
    ML, SN = _case_modules()
    assert tuple(SN.CASE_IDS) == AC.SENS_IDS and set(AC.LIMIT_IDS) <= set(ML.ACCEPTED_IDS)          # (the ids adj_cases writes out)
    assert AC.FD_H == SN.FD_H and AC.WINDOW_NW == (ML.LDS // 8 - 2) // 40 + 1 and set(AC.CASE_IDS) == set(AC.SPREAD)
    forms = {AC.case(cid)["form"] for cid in AC.NW3}
    assert forms == {"eliminated", "states"} and all(AC.case(cid)["w3"][0].shape[1] == 3 for cid in AC.NW3)
    c = ML.case(AC.WINDOW_ID)
    nz = int(np.max(np.asarray(c["d"]["nx"]) + np.asarray(c["d"]["nu"])))
    assert nz == 40 and (nz * (AC.WINDOW_NW - 1) + 2) * 8 <= ML.LDS < (nz * AC.WINDOW_NW + 2) * 8

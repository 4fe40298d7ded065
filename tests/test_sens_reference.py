"""The two numpy evaluations of sens_ref.py against each other and against the oracle's finite differences, on the CPU.

Per case (sens_cases.py), at the oracle's solve with stationarityTolerance 1e-12: status 0; at least one bound active and one entry free
below the root; strict complementarity (|mu| > 1e-6 on every bound); the lstsq residual of (a) at rounding level.  The tree with a kind-1
root has no bounds (kind 1 ignores them): the bound conditions do not apply to it.  Measured spreads max |(a) - (b)| and discrepancies
max |K dx - (u0(x0 + dx) - u0(x0))| are kept in sens_cases.SPREAD (largest: K 3.7e-11, dx 3.8e-11, du 4.2e-11, dlam 1.2e-8 on the 31-node
chain of the tiered route, dx 9.8e-12, du 4.8e-12, K 1.2e-13, dlam 1.5e-9 on the 85-node spring-mass trees, K, dx, du 1.6e-14 and dlam
4e-14 and below on the small ones; finite differences 5.0e-15 and below); this module checks that they still hold."""
import functools

import numpy as np
import pytest

import sens_cases as SN
import sens_ref as SR


@functools.lru_cache(maxsize=None)
def _solved(cid):
    import oracle_py as orc
    c = SN.case(cid)
    return SN.oracle_solve(orc, c)


@pytest.mark.parametrize("cid", SN.CASE_IDS)
def test_case_is_valid(orc, cid):
    c, s = SN.case(cid), _solved(cid)
    assert s["status"] == 0
    on = SR.pinned(c["d"], s["x"], s["u"], c["kinds"])
    below = on[c["nx0"] if c["form"] == "states" else 0:]
    if c["kinds"] is None:
        assert below.any() and not below.all()
        mu = np.concatenate([s["mu_x"], s["mu_u"]])[c["nx0"] if c["form"] == "states" else 0:]
        assert np.all(np.abs(mu[below]) > 1e-6)
    a = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    assert a["residual"] < 1e-9 * a["scale"], a["residual"]


@pytest.mark.parametrize("cid", SN.CASE_IDS)
def test_the_two_evaluations_agree(orc, cid):
    c, s = SN.case(cid), _solved(cid)
    a = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    b = SR.dual_form(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    assert b["n_reg"] == 0 and b["in_range"] < 1e-10
    for i, what in enumerate(("K", "dx", "du", "dlam")):
        spread = float(np.max(np.abs(a[what] - b[what]))) if a[what].size else 0.0
        print(f"{cid} {what}: spread {spread:.3e} (recorded {SN.SPREAD[cid][i]:.1e})")
        assert spread <= 2.0 * SN.SPREAD[cid][i] + 1e-16, (what, spread)          # (2 x: another BLAS may sum in another order)
    if c["form"] == "states":
        assert np.array_equal(b["dx"][:c["nx0"]], np.eye(c["nx0"]))


@pytest.mark.parametrize("cid", SN.CASE_IDS)
def test_gain_against_the_oracle_finite_difference(orc, cid):
    c, s = SN.case(cid), _solved(cid)
    d1 = SN.problem_at(c, c["x0"] + c["dx"])
    s1 = SN.oracle_solve(orc, c, d1)
    assert s1["status"] == 0
    assert np.array_equal(SR.pinned(c["d"], s["x"], s["u"], c["kinds"]), SR.pinned(d1, s1["x"], s1["u"], c["kinds"])), "the active set changed: dx is too large"
    K = SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])["K"]
    nu0 = K.shape[0]
    err = float(np.max(np.abs(K @ c["dx"] - (s1["u"][:nu0] - s["u"][:nu0]))))
    print(f"{cid}: |K dx - du0| = {err:.3e} (recorded {SN.SPREAD[cid][4]:.1e})")
    assert err <= 2.0 * SN.SPREAD[cid][4] + 1e-16


def test_every_route_has_a_case():
    paths = {c["base"]["path"] for c in SN.cases()}
    assert {2, 3, 1, 0} <= paths and "elim-three_launch" in SN.CASE_IDS

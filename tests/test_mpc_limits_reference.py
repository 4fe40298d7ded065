"""The cases of mpc_limit_cases.py meet, on the CPU, the conditions the device tests (test_gpu_mpc_limits.py) rely on.

Per sensitivity case, at the oracle's solve with stationarityTolerance 1e-12: status 0; the lstsq residual of sens_ref.dense_kkt at
rounding level; at least one bound active and, unless the row is about a refusal only, at least one entry of u[0] free (the kind-1 trees
have no bounds: the two conditions do not apply to them, as in test_sens_reference.py); the two numpy evaluations agree within the spreads
kept in mpc_limit_cases.SPREAD and the block form regularises nothing (n_reg == 0: the device must report 0 too, so dlam is compared on
every case).  The nu[0] = 70 case has free entries of u[0] on both sides of index 64, and the prediction at dx * 2^20 clips on both sides;
so do the other predict cases on the sides they have.  The LDS rows sit where setup_sens' formulas put the limit."""
import functools

import numpy as np
import pytest

import mpc_limit_cases as ML
import sens_cases as SN
import sens_ref as SR


@functools.lru_cache(maxsize=None)
def _solved(cid):
    import oracle_py as orc
    return SN.oracle_solve(orc, ML.case(cid))


@functools.lru_cache(maxsize=None)
def _kkt(cid):
    c, s = ML.case(cid), _solved(cid)
    return SR.dense_kkt(c["d"], s["x"], s["u"], c["param"], c["kinds"])


def _on(cid):
    c, s = ML.case(cid), _solved(cid)
    return SR.pinned(c["d"], s["x"], s["u"], c["kinds"])


@pytest.mark.parametrize("cid", ML.SENS_IDS)
def test_case_is_valid(orc, cid):
    c, s = ML.case(cid), _solved(cid)
    assert s["status"] == 0
    a = _kkt(cid)
    assert a["residual"] < 1e-9 * a["scale"], a["residual"]
    if c["kinds"] is not None:
        return
    on = _on(cid)
    sx, nu0 = len(s["x"]), int(c["d"]["nu"][0])
    below = on[c["nx0"] if c["form"] == "states" else 0:]
    assert below.any(), "no bound is active"
    if not ML.flags(cid).get("refused"):
        free = ~on[sx:sx + nu0]
        assert free.any(), "every entry of u[0] sits on a bound"
        if ML.flags(cid).get("both_sides"):
            assert free[:64].any() and free[64:].any()
    mu = np.concatenate([s["mu_x"], s["mu_u"]])[c["nx0"] if c["form"] == "states" else 0:]
    assert np.all(np.abs(mu[below]) > 1e-6)


@pytest.mark.parametrize("cid", ML.ACCEPTED_IDS)
def test_the_two_evaluations_agree(orc, cid):
    c, s = ML.case(cid), _solved(cid)
    a = _kkt(cid)
    b = SR.dual_form(c["d"], s["x"], s["u"], c["param"], c["kinds"])
    assert b["n_reg"] == 0 and b["in_range"] < 1e-10
    for i, what in enumerate(("K", "dx", "du", "dlam")):
        spread = float(np.max(np.abs(a[what] - b[what]))) if a[what].size else 0.0
        print(f"{cid} {what}: spread {spread:.3e} (recorded {ML.SPREAD[cid][i]:.1e})")
        assert spread <= 2.0 * ML.SPREAD[cid][i] + 1e-16, (what, spread)          # (2 x: another BLAS may sum in another order)
    if c["form"] == "states":
        assert np.array_equal(b["dx"][:c["nx0"]], np.eye(c["nx0"]))


@pytest.mark.parametrize("cid", ML.PREDICT_IDS)
def test_the_prediction_clips_on_every_side_of_64(orc, cid):
    """with the reference's K at the oracle's point: the chain of tqgpu_mpc_predict at dx * 2^20 leaves the box below index 64 and, where
    there are such entries, at 64 and above"""
    c, s = ML.case(cid), _solved(cid)
    K = _kkt(cid)["K"]
    nu0 = K.shape[0]
    dx = c["dx"] * 2.0 ** 20
    want = s["u"][:nu0].copy()
    for j in range(len(dx)):
        want = np.array([ML.fma(K[i, j], dx[j], want[i]) for i in range(nu0)])
    out = (want < c["d"]["umin"][:nu0]) | (want > c["d"]["umax"][:nu0])
    assert out[:64].any()
    assert nu0 <= 64 or out[64:].any()


def test_the_lds_rows_sit_at_the_limit():
    lf = {cid: ML.lds_bytes(ML.case(cid)) for cid in ML.ROWS["setup_sens tall"] + ML.ROWS["setup_sens window"]}
    print(lf)
    assert lf["lds_tall-d140_nx0_5"][0] == 163536 and lf["lds_tall-d141_two_states"][0] == 162448 and lf["lds_tall-d141_nx0_5"][0] == 166960
    assert lf["lds_window-accepted"][1] == 163536 and lf["lds_window-refused"][1] == 163856
    for cid, (f, p) in lf.items():
        assert (f > ML.LDS or p > ML.LDS) == bool(ML.flags(cid).get("refused")), cid
    # the smallest refused and the largest accepted: one more row of the root block, one more column of the window
    assert ML.lds_bytes(ML.case("lds_tall-d140_nx0_5"))[0] <= ML.LDS < ML.lds_bytes(ML.case("lds_tall-d141_nx0_5"))[0]
    assert ML.case("lds_window-refused")["nx0"] == ML.case("lds_window-accepted")["nx0"] + 1
    for cid in ML.ACCEPTED_IDS:
        f, p = ML.lds_bytes(ML.case(cid))
        assert f <= ML.LDS and p <= ML.LDS, cid


def test_every_row_has_its_sides():
    ids = [c for row in ML.ROWS.values() for c in row]
    assert sorted(ids) == sorted(ML.SENS_IDS)
    assert ML.parent_levels(ML.case("Nh1-one_leaf")["d"]["nk"]) == 1 == ML.parent_levels(ML.case("Nh1-three_leaves")["d"]["nk"])
    for cid, want in (("root_d-elim_d64", 64), ("root_d-elim_d65", 65), ("root_d-states_d64", 64), ("root_d-states_d65", 65)):
        d = ML.case(cid)["d"]
        assert int(d["nk"][0]) == 8 and int(d["nx"][1:9].sum()) == want
    a, b = ML.batch_cases()
    assert (int(a["d"]["nu"][0]), int(b["d"]["nu"][0])) == (16, 17) and int(a["d"]["nk"][0]) != int(b["d"]["nk"][0])


@pytest.mark.parametrize("cid", ML.TRACKING_IDS)
def test_the_tracking_data_are_exact(cid):
    """every term of the window fold is a multiple of 2^-12 and the absolute sum of an entry's terms stays below 2^40: every partial sum is
    exact in double precision, in any order, so the device's fma chain and the numpy fold must agree bit for bit"""
    import tracking_cases as K
    c = ML.tracking_case(cid)
    x0 = c["x0s"][0]
    eps = np.finfo(np.float64).eps
    for name in ("xtraj", "utraj", "q0", "r0"):
        assert np.array_equal(c[name] * 64.0, np.round(c[name] * 64.0)), name
    for t0 in ML.TRACK_WINDOWS:
        q, r, bq, br = K.fold(c, t0, x0, bound=True)
        for v, b in ((q, bq), (r, br)):
            assert np.array_equal(v * 2.0 ** 12, np.round(v * 2.0 ** 12))
            assert np.max(b) / (4.0 * eps) < 2.0 ** 40          # (the bound is 2 (n + 1) eps times the absolute sum, n >= 1)
    assert max(ML.TRACK_WINDOWS) + K.stages(c["d"]["nk"]).max() > c["T"] - 1 > min(ML.TRACK_WINDOWS)

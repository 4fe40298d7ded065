"""The two numpy evaluations of adjmat_ref.py against each other and against a central finite difference through the oracle, on the CPU.

Per tree of adjmat_cases.py, at the oracle's solve with stationarityTolerance 1e-12: (a) and (b) agree within the spreads kept in
adjmat_cases.SPREAD for every pair of maps the tree has; the dual of the forward KKT solve of (a) is the oracle's lam, not its negative
(this settles the sign the header states); and w' (z(theta + dtheta) - z(theta - dtheta)) / 2 matches <G, dtheta> for a direction in H
(symmetric; the diagonal on kind-0 nodes), A, B, A0 and S0.  Central, because the solution is not linear in a matrix.  Where the active set
moves under +-dtheta the step is halved; the step that held is part of the table."""
import functools

import numpy as np
import pytest

import adj_ref as AR
import adjmat_cases as XC
import adjmat_ref as AM
import sens_ref as SR

TREES = sorted({cid.split("|")[0] for cid in XC.CASE_IDS}, key=[cid.split("|")[0] for cid in XC.CASE_IDS].index)


def _modules():
    import mpc_cases as MC
    import sens_cases as SN
    return MC, SN


@functools.lru_cache(maxsize=None)
def _solved(name):
    _, SN = _modules()
    import oracle_py as orc
    return SN.oracle_solve(orc, XC.tree(name))


def _direction(c, seed):
    """dtheta of size 1 (multiples of 2^-6): per node dH (the diagonal, or symmetric), per edge dA, dB, and dA0 per child, dS0"""
    MC, _ = _modules()
    t = SR._assemble(c["d"], c["kinds"])
    rng = np.random.Generator(np.random.PCG64(seed + 31337))
    dH = []
    for k in range(t["Nn"]):
        nz = len(t["idx"][k])
        M = MC.quantised(rng, (nz, nz), 1.0)
        dH.append(np.diag(M).copy() if t["kinds"][k] == 0 else 0.5 * (M + M.T))
    dA = [MC.quantised(rng, (int(t["nx"][k]), int(t["nx"][t["dad"][k]])), 1.0) for k in range(1, t["Nn"])]
    dB = [MC.quantised(rng, (int(t["nx"][k]), int(t["nu"][t["dad"][k]])), 1.0) for k in range(1, t["Nn"])]
    out = dict(gH=dH, gA=dA, gB=dB)
    if c["form"] == "eliminated":
        out["gA0"] = [MC.quantised(rng, np.asarray(M).shape, 1.0) for M in c["param"]["A0"]]
        if c["param"].get("S0") is not None:
            out["gS0"] = [MC.quantised(rng, np.asarray(c["param"]["S0"]).shape, 1.0)]
    return out


def _moved(c, dth, h):
    """the flat problem with every matrix moved by h * dtheta (A0, S0 through the fold of x0 into b and r[0])"""
    t = SR._assemble(c["d"], c["kinds"])
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    d["A"] = d["A"] + h * np.concatenate([M.ravel(order="F") for M in dth["gA"]])
    d["B"] = d["B"] + h * np.concatenate([M.ravel(order="F") for M in dth["gB"]])
    if "Q" in d and c["kinds"] is not None:
        Q, R, S = [], [], []
        for k in range(t["Nn"]):
            a = int(t["nx"][k])
            Hk = dth["gH"][k] if dth["gH"][k].ndim == 2 else np.diag(dth["gH"][k])
            Q.append(Hk[:a, :a].ravel(order="F")); R.append(Hk[a:, a:].ravel(order="F")); S.append(Hk[a:, :a].ravel(order="F"))
        for key, v in (("Q", Q), ("R", R), ("S", S)):
            d[key] = d[key] + h * np.concatenate(v)
    else:
        d["Qd"] = d["Qd"] + h * np.concatenate([dth["gH"][k][:int(t["nx"][k])] for k in range(t["Nn"])])
        d["Rd"] = d["Rd"] + h * np.concatenate([dth["gH"][k][int(t["nx"][k]):] for k in range(t["Nn"])])
    if "gA0" in dth:
        nb = sum(M.shape[0] for M in dth["gA0"])
        d["b"][:nb] = d["b"][:nb] + h * np.concatenate([M @ c["x0"] for M in dth["gA0"]])
    if "gS0" in dth:
        nu0 = int(t["nu"][0])
        d["r"][:nu0] = d["r"][:nu0] + h * (dth["gS0"][0] @ c["x0"])
    return d


@functools.lru_cache(maxsize=None)
def _measured(name):
    _, SN = _modules()
    import oracle_py as orc
    c, s = XC.tree(name), _solved(name)
    assert s["status"] == 0
    Nn = len(c["d"]["nk"])
    b = AR.dual_form(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"])
    assert b["n_reg"] == 0
    spread = np.zeros(6)
    lam_err = 0.0
    names = sorted({cid.split("|")[1] for cid in XC.CASE_IDS if cid.split("|")[0] == name} | {"node"})
    for mp in names:
        hg, cg = XC.filled(c, *XC.maps(c, mp))
        A, lamf, resid = AM.dense(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"], hg, cg, c["x0"])
        B = AM.outer(c["d"], s["x"], s["u"], s["lam"], c["param"], b, c["kinds"], hg, cg, c["x0"])
        assert max(resid) < 1e-9 * max(1.0, float(np.max(np.abs(lamf), initial=0.0)))
        lam_err = max(lam_err, float(np.max(np.abs(lamf - s["lam"]), initial=0.0)))
        for i, key in enumerate(AM.KEYS):
            for x, y in zip(A[key], B[key]):
                assert x.shape == y.shape
                spread[min(i, 5)] = max(spread[min(i, 5)], float(np.max(np.abs(x - y), initial=0.0)))
        if mp == "node":
            G = A
    dth = _direction(c, SN._seed(name))
    h = XC.FD_H
    on = SR.pinned(c["d"], s["x"], s["u"], c["kinds"])
    while True:
        sp, sm = [SN.oracle_solve(orc, c, _moved(c, dth, sign * h)) for sign in (1.0, -1.0)]
        assert sp["status"] == 0 and sm["status"] == 0
        if all(np.array_equal(on, SR.pinned(c["d"], q["x"], q["u"], c["kinds"])) for q in (sp, sm)):
            break
        h *= 0.5
        assert h > 2.0 ** -30, "no step keeps the active set"
    wx, wu = c["w"]
    got = float(wx[:, 0] @ (sp["x"] - sm["x"]) + wu[:, 0] @ (sp["u"] - sm["u"])) / 2.0
    want = h * AM.inner(G, dth)
    return spread, abs(got - want), h, lam_err, abs(want)


@pytest.mark.parametrize("name", TREES)
def test_the_two_evaluations_agree_and_lam_is_the_solvers(orc, name):
    spread, _, _, lam_err, _ = _measured(name)
    rec = XC.SPREAD[name]
    print(f"{name}: spreads " + " ".join(f"{v:.1e}" for v in spread) + f" (recorded {rec[:6]}), |lam(a) - lam| = {lam_err:.1e}")
    for v, r in zip(spread, rec[:6]):
        assert v <= 2.0 * r + 1e-16          # (2 x: another BLAS may sum in another order)
    assert lam_err <= 1e-8 * max(1.0, float(np.max(np.abs(_solved(name)["lam"]), initial=0.0)))


@pytest.mark.parametrize("name", TREES)
def test_gradients_against_the_central_finite_difference(orc, name):
    _, err, h, _, size = _measured(name)
    rec = XC.SPREAD[name]
    print(f"{name}: |w' (z+ - z-) / 2 - <G, dtheta>| = {err:.3e} of {size:.3e} at step {h:.3e} (recorded {rec[6]:.1e} at {rec[7]:.3e})")
    assert h == rec[7] and err <= 2.0 * rec[6] + 1e-16


def test_the_cases_cover_what_they_name():
    import adj_cases as AC
    assert set(XC.TREES) == set(AC.SENS_IDS) and set(XC.SMALL) <= set(AC.LIMIT_IDS) and set(TREES) == set(XC.SPREAD)
    c = XC.tree("chain66")
    assert len(c["d"]["nk"]) == 66 and int(np.sum(XC.maps(c, "c64")[1] == 0)) == 64 and int(np.sum(XC.maps(c, "c65")[1] == 0)) == 65
    assert 8 * (8 + 3) + 8 > 64 and 8 * (4 + 3) + 8 == 64
    m = XC.tree("mixed")
    assert set(int(k) for k in m["kinds"]) == {0, 1}

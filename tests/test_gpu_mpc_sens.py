"""Parametric sensitivities of an MPC step on the device (tqgpu_mpc_sensitivity, tqgpu_mpc_get_gain, tqgpu_mpc_get_sensitivities,
tqgpu_mpc_predict) against sens_ref.dense_kkt evaluated at the device's own exported point.

Cases: sens_cases.py (its header says which trees were dropped and why; every route keeps a case: 2, 3, three-launch, 1 -- the tiered
chain with a tighter input bound --, 0).
Tolerances: 10 times the spread of the two numpy evaluations on the CPU (sens_cases.SPREAD, measured by test_sens_reference.py), floor
1e-12; dlam is compared where the device reports n_reg == 0.
tqgpu_mpc_predict is not checked on data whose partial sums are exact: the test emulates the chain v = fma(K[i, j], dx_j, v), one rounding
per step, in rational arithmetic on the CPU and asks for the same bits, for any K and dx, the clipped entries included."""
import ctypes as C

import numpy as np
import pytest

import mpc_cases as MC
import sens_cases as SN
import sens_ref as SR
import solve_sequence_cases as SC

pytestmark = pytest.mark.gpu


def _step(g, c, x0=None, **kw):
    return g.mpc_step(c["x0"] if x0 is None else x0, **{**c["base"]["opts"], **kw})


def _blocks_levels(nk):
    """levels of the tree that hold parents"""
    nk = np.asarray(nk)
    lvl, first, n = 0, 0, 1
    while first < len(nk) and np.any(nk[first:first + n] > 0):
        kids = int(nk[first:first + n].sum())
        first, n, lvl = first + n, kids, lvl + 1
    return lvl


@pytest.mark.parametrize("cid", SN.CASE_IDS)
def test_against_the_dense_kkt_reference(capi, cid):
    c = SN.case(cid)
    g = SN.make(capi, c)
    r, u0 = _step(g, c)
    assert r["status"] == 0
    sol_before = g.solution()
    kkt_before = g.kkt_residual()
    n_reg = g.mpc_sensitivity(**c["base"]["opts"])
    st = capi.mpc_stats()
    Nh = _blocks_levels(c["d"]["nk"])
    assert (st["copies"], st["waits"]) == (1, 1), st
    assert st["launches"] == 1 + Nh + (Nh - 1) + 1 + 1, st          # (+ the packing kernel: the point was not packed ahead or by a certified step)
    K, u0s, x0r = g.mpc_gain()
    s = g.mpc_sensitivities()
    sol = g.solution()
    for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
        assert np.array_equal(sol[k], sol_before[k]), k
    kkt_after = g.kkt_residual()
    assert np.array_equal(kkt_after["res"], kkt_before["res"])
    assert np.array_equal(u0s, sol["u"][:len(u0s)]) and np.array_equal(x0r, c["x0"])
    ref = SR.dense_kkt(c["d"], sol["x"], sol["u"], c["param"], c["kinds"])
    assert ref["residual"] < 1e-9 * ref["scale"]
    got = dict(K=K, dx=s["dx"], du=s["du"], dlam=s["dlam"])
    for what in ("K", "dx", "du") + (("dlam",) if n_reg == 0 else ()):
        err = float(np.max(np.abs(got[what] - ref[what]))) if ref[what].size else 0.0
        print(f"{cid} {what}: |device - (a)| = {err:.3e}, tolerance {SN.tol(cid, what):.3e}, n_reg {n_reg}")
        assert err <= SN.tol(cid, what), (what, err)
    # exact structure
    on = SR.pinned(c["d"], sol["x"], sol["u"], c["kinds"])
    nu0, sx = len(u0s), len(sol["x"])
    for i in range(nu0):
        if on[sx + i]:
            assert np.all(K[i] == 0.0), f"row {i} of K: u[0][{i}] sits on a bound"
    if c["form"] == "states":
        assert np.array_equal(s["dx"][:c["nx0"]], np.eye(c["nx0"]))
    assert np.array_equal(K, s["du"][:nu0])


def test_unconstrained_gain(capi):
    c = SN.case("elim-one_child")
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    for k, v in (("xmin", -1e30), ("xmax", 1e30), ("umin", -1e30), ("umax", 1e30)):
        d[k][:] = v
    g = MC.make(capi, c["base"], d=d)
    g.mpc_set_certify(True)
    r, _ = _step(g, c)
    assert r["status"] == 0
    g.mpc_sensitivity()
    st, Nh = capi.mpc_stats(), _blocks_levels(d["nk"])
    assert (st["launches"], st["copies"], st["waits"]) == (1 + Nh + (Nh - 1) + 1, 1, 1), st          # the certified step packed the point
    sol = g.solution()
    ref = SR.dense_kkt(d, sol["x"], sol["u"], c["param"])
    assert ref["n_pinned"] == 0
    K = g.mpc_gain()[0]
    assert np.max(np.abs(K - ref["K"])) <= SN.tol(c["id"], "K")


@pytest.mark.parametrize("cid,scale", [("elim-single_wg", 2.0 ** 10), ("elim-three_children", 2.0 ** 10), ("elim-generic", 2.0 ** 10),
                                       ("elim-three_children", 2.0 ** 20), ("elim-generic", 2.0 ** 20)],
                         ids=["single_wg-small", "three_children-small", "generic-small", "three_children-clipping", "generic-clipping"])
def test_predict_is_the_fma_chain(capi, cid, scale):
    """scale 2^10: dx of about 2^-6, nothing leaves its box; 2^20: dx of about 16, the free entries of u[0] are pushed past their bounds
    (on the trees that have a free entry of u[0]: every entry of single_wg's sits on a bound, its K is zero and nothing can move)"""
    c = SN.case(cid)
    g = SN.make(capi, c)
    _step(g, c)
    g.mpc_sensitivity()
    K, u0s, x0r = g.mpc_gain()
    dx = c["dx"] * scale
    x1 = x0r + dx
    assert np.array_equal(x1 - x0r, dx)
    want = u0s.copy()
    for j in range(len(dx)):
        want = np.array([_fma(K[i, j], dx[j], want[i]) for i in range(len(want))])
    lo, hi = c["d"]["umin"][:len(want)], c["d"]["umax"][:len(want)]
    clipped = np.clip(want, lo, hi)
    got, n = g.mpc_predict(x1)
    assert np.array_equal(got, clipped)
    assert n == int(np.count_nonzero(clipped != want))
    if scale > 2.0 ** 10:
        assert n > 0 and np.any((clipped == lo) | (clipped == hi)), "the clipping branch was not reached"
    st = capi.mpc_stats()
    assert (st["launches"], st["copies"], st["waits"]) == (1, 0, 1), st


def _fma(a, b, c):
    """a * b + c rounded once, through exact rational arithmetic"""
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


@pytest.mark.parametrize("mode", [0, 1])
def test_predicted_duals_start_one_solve(capi, mode):
    c = SN.case("elim-three_children")
    g = SN.make(capi, c)
    lam_user = 0.125 * np.ones(g.sum_lam)
    g.set_lambda(lam_user)
    g.set_warm_start(mode)
    _step(g, c, **SN.TOL12)
    lam_star = g.solution()["lam"]
    g.mpc_sensitivity()
    dlam = g.mpc_sensitivities()["dlam"]
    x1 = c["x0"] + c["dx"] * 2.0 ** 10
    g.mpc_predict(x1, duals=True)
    r1, _ = _step(g, c, x0=x1, maxIter=1)
    # the witness: the error norm of the first iteration is that of the predicted duals
    twin = SN.make(capi, c)
    twin.set_lambda(lam_star + dlam @ (x1 - c["x0"]))
    rt, _ = _step(twin, c, x0=x1, maxIter=1)
    assert abs(r1["last_error_norm"] - rt["last_error_norm"]) <= 1e-13 * max(1.0, abs(rt["last_error_norm"]))
    # the solve after that starts as its mode says
    lam_after = g.solution()["lam"]
    r2, _ = _step(g, c, x0=x1, maxIter=1)
    twin2 = SN.make(capi, c)
    twin2.set_lambda(lam_user if mode == 0 else lam_after)
    rt2, _ = _step(twin2, c, x0=x1, maxIter=1)
    assert r2["last_error_norm"] == rt2["last_error_norm"]


@pytest.mark.parametrize("cid", ["elim-three_launch", "elim-generic", "elim-dense_kind1_root", "states-three_children", "states-generic", "states-tiered_ub"])
def test_finite_differences_on_the_device(capi, cid):
    c = SN.case(cid)
    g = SN.make(capi, c)
    _, u0 = _step(g, c, **SN.TOL12)
    g.mpc_sensitivity()
    K = g.mpc_gain()[0]
    _, u1 = _step(g, c, x0=c["x0"] + c["dx"], **SN.TOL12)
    err = float(np.max(np.abs(K @ c["dx"] - (u1 - u0))))
    print(f"{cid}: |K dx - (u0' - u0)| = {err:.3e}, bound {SN.tol(cid, 'fd'):.3e}")
    assert err <= SN.tol(cid, "fd")


@pytest.mark.parametrize("cid", ["elim-persist_c1", "elim-single_wg", "elim-generic", "states-tiered_ub"])
def test_the_next_step_is_not_disturbed(capi, cid):
    c = SN.case(cid)
    outs = []
    for with_call in (False, True):
        g = SN.make(capi, c)
        g.set_warm_start(1)
        _step(g, c)
        if with_call:
            g.mpc_sensitivity()
        r, u = _step(g, c, x0=c["x0"] + c["dx"] * 2.0 ** 12)
        outs.append((r["iter"], r["ls_total"], u.copy(), g.solution()))
    assert outs[0][:2] == outs[1][:2] and np.array_equal(outs[0][2], outs[1][2])
    for k in ("x", "u", "lam"):
        assert np.array_equal(outs[0][3][k], outs[1][3][k])


def test_refusals_and_invalidation(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    c = SN.case("elim-one_child")
    g = MC.make(capi, c["base"], root=False)
    assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), None) == -2          # no root form yet
    g = SN.make(capi, c)
    assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), None) == -2          # no solve yet
    _step(g, c)
    assert L.tqgpu_mpc_sensitivity(g.h, None, None) == -2
    assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == -2              # nothing computed yet
    g.mpc_sensitivity()
    assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == 0
    g.set_linear_terms(c["d"]["q"], None)
    assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == -2
    _step(g, c)
    g.mpc_sensitivity()
    g.mpc_set_x0(c["x0"])
    assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == -2
    assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), None) == -2          # the fold came after the last solve: point and data do not belong together
    assert b"since the last solve" in L.tqgpu_last_error()
    u = np.zeros(4)
    assert L.tqgpu_mpc_predict(g.h, u.ctypes.data_as(C.POINTER(C.c_double)), u.ctypes.data_as(C.POINTER(C.c_double)), 0, None) == -2
    for kid in ("dense_kind2_root", "dense_kind3_root"):
        b = MC.case(kid)
        gb = MC.make(capi, b)
        gb.mpc_step(MC.exact_x0s(b["nx0"], 0)[0], **b["opts"])
        assert L.tqgpu_mpc_sensitivity(gb.h, C.byref(o), None) == -4
        assert b"kind 2 or 3" in L.tqgpu_last_error()


def test_a_rank_of_a_sharded_solve_is_refused(capi):
    from treeqp_amd import problems as P
    g = SC._lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05))(capi)
    g.pshard_init(0, 2)
    L = capi.lib()
    o = capi._gpu_opts(0)
    assert L.tqgpu_mpc_sensitivity(g.h, C.byref(o), None) == -4
    assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == -4

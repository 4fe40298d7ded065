"""The adjoint of an MPC step on the device (tqgpu_mpc_adjoint, tqgpu_mpc_get_adjoint_x0, tqgpu_mpc_get_adjoint) against adj_ref.dual_form
evaluated at the device's own exported point, against the device's forward sensitivities, and against itself (stored factor or not, one
column or three).

Cases: adj_cases.py (sens_cases' and the limit shapes of mpc_limit_cases on both sides of 64).
Tolerances: 10 times the spread of the two numpy evaluations on the CPU (adj_cases.SPREAD, measured by test_adj_reference.py), floor
1e-12; gb is compared where the device reports n_reg == 0.  Everything the call must leave alone is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import adj_cases as AC
import adj_ref as AR
import mpc_cases as MC
import mpc_limit_cases as ML
import sens_cases as SN

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
GRADS = ("gq", "gr", "gb")


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _step(g, c, x0=None, **kw):
    return g.mpc_step(c["x0"] if x0 is None else x0, **{**c["base"]["opts"], **kw})


def _adjoint(g, c, w):
    out = g.mpc_adjoint(w[0], w[1], **c["base"]["opts"])
    out.update(g.mpc_adjoint_grads())
    return out


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_against_the_block_reference(capi, cid):
    c = AC.case(cid)
    g = SN.make(capi, c)
    try:
        r, _ = _step(g, c)
        assert r["status"] == 0
        sol_before, kkt_before = g.solution(), g.kkt_residual()
        got = g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        Nh = ML.parent_levels(c["d"]["nk"])
        assert _counts(capi) == (3 * Nh + 2 + 1, 2, 1)          # (+ the packing kernel: the point was not packed ahead or by a certified step)
        got.update(g.mpc_adjoint_grads())
        sol = g.solution()
        for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
            _same_bits(sol[k], sol_before[k], f"{cid}: {k} after tqgpu_mpc_adjoint")
        _same_bits(g.kkt_residual()["res"], kkt_before["res"], f"{cid}: the KKT residual after tqgpu_mpc_adjoint")
        ref = AR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["w"], c["kinds"])
        assert ref["n_reg"] == 0 and ref["in_range"] < 1e-10
        for what in ("gq", "gr", "gx0") + (("gb",) if got["n_reg"] == 0 else ()):
            assert got[what].shape == ref[what].shape, what
            err = float(np.max(np.abs(got[what] - ref[what]))) if ref[what].size else 0.0
            print(f"{cid} {what}: |device - (b)| = {err:.3e}, tolerance {AC.tol(cid, what):.3e}, n_reg {got['n_reg']}")
            assert err <= AC.tol(cid, what), (what, err)
    finally:
        g.close()


@pytest.mark.parametrize("cid", AC.CASE_IDS)
def test_forward_sensitivities_and_the_stored_factor(capi, cid):
    """one mirror: the adjoint that builds the factor itself, then tqgpu_mpc_sensitivity, then the adjoint that finds the factor stored"""
    c = AC.case(cid)
    g = SN.make(capi, c)
    try:
        r, _ = _step(g, c)
        assert r["status"] == 0
        Nh = ML.parent_levels(c["d"]["nk"])
        built = _adjoint(g, c, c["w"])
        again = g.mpc_adjoint(*c["w"], **c["base"]["opts"])          # its own factor is stored now
        assert _counts(capi) == (2 * Nh + 1, 2, 1)
        _same_bits(again["gx0"], built["gx0"], f"{cid}: gx0, the call's own factor stored")
        g.mpc_sensitivity(**c["base"]["opts"])
        K, _, _ = g.mpc_gain()
        s = g.mpc_sensitivities()
        stored = g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        assert _counts(capi) == (2 * Nh + 1, 2, 1)
        stored.update(g.mpc_adjoint_grads())
        assert stored["n_reg"] == built["n_reg"]
        for what in GRADS + ("gx0",):
            _same_bits(stored[what], built[what], f"{cid}: {what}, factor stored against factor built")
        want = np.vstack([s["dx"], s["du"]]).T @ np.vstack(c["w"])
        err = float(np.max(np.abs(stored["gx0"] - want)))
        print(f"{cid}: |gx0 - dZ' w| = {err:.3e}, tolerance {AC.tol(cid, 'gx0'):.3e}")
        assert err <= AC.tol(cid, "gx0")
        nu0 = K.shape[0]
        wu = np.zeros((int(g.sum_nu), nu0))
        wu[np.arange(nu0), np.arange(nu0)] = 1.0
        rows = g.mpc_adjoint(None, wu, **c["base"]["opts"])["gx0"]
        err = float(np.max(np.abs(rows.T - K)))
        print(f"{cid}: |gx0(e_i) - K[i]| = {err:.3e}, tolerance {AC.tol(cid, 'gx0'):.3e}")
        assert err <= AC.tol(cid, "gx0")
    finally:
        g.close()


@pytest.mark.parametrize("cid", AC.NW3)
def test_three_columns_are_three_calls(capi, cid):
    c = AC.case(cid)
    g = SN.make(capi, c)
    try:
        _step(g, c)
        wx, wu = c["w3"]
        all3 = _adjoint(g, c, (wx, wu))
        assert all3["gx0"].shape == (c["nx0"], 3)
        for j in range(3):
            one = _adjoint(g, c, (wx[:, j], wu[:, j]))
            for what in GRADS + ("gx0",):
                _same_bits(one[what][:, 0], all3[what][:, j], f"{cid}: column {j} of {what}")
        # a missing part means zero
        only_u = _adjoint(g, c, (None, wu))
        zero_x = _adjoint(g, c, (np.zeros_like(wx), wu))
        for what in GRADS + ("gx0",):
            _same_bits(only_u[what], zero_x[what], f"{cid}: {what} with wx = NULL")
    finally:
        g.close()


@pytest.mark.parametrize("cid", ["elim-three_children", "states-generic", "elim-dense_kind1_root"])
def test_a_stored_sensitivity_is_left_alone(capi, cid):
    c = AC.case(cid)
    g = SN.make(capi, c)
    try:
        _step(g, c)
        g.mpc_sensitivity(**c["base"]["opts"])
        x1 = c["x0"] + c["dx"] * 2.0 ** 10
        before = (g.mpc_gain(), g.mpc_sensitivities(), g.mpc_predict(x1))
        _adjoint(g, c, c["w"])
        after = (g.mpc_gain(), g.mpc_sensitivities(), g.mpc_predict(x1))
        for i in range(3):
            _same_bits(after[0][i], before[0][i], f"{cid}: mpc_gain[{i}]")
        for k in ("dx", "du", "dlam"):
            _same_bits(after[1][k], before[1][k], f"{cid}: {k}")
        _same_bits(after[2][0], before[2][0], f"{cid}: u0_pred")
        assert after[2][1] == before[2][1]
    finally:
        g.close()


@pytest.mark.parametrize("cid", ["elim-persist_c1", "elim-single_wg", "elim-generic", "states-tiered_ub"])
def test_the_next_step_is_not_disturbed(capi, cid):
    c = AC.case(cid)
    outs = []
    for with_call in (False, True):
        g = SN.make(capi, c)
        try:
            g.set_warm_start(1)
            _step(g, c)
            if with_call:
                _adjoint(g, c, c["w"])
            r, u = _step(g, c, x0=c["x0"] + c["dx"] * 2.0 ** 12)
            outs.append((r["iter"], r["ls_total"], u.copy()))
        finally:
            g.close()
    assert outs[0][:2] == outs[1][:2]
    _same_bits(outs[0][2], outs[1][2], f"{cid}: u[0] of the next step")


def test_refusals_and_invalidation(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    c = AC.case("elim-one_child")
    wx, wu = [np.ascontiguousarray(v[:, 0]) for v in c["w"]]
    px, pu = [v.ctypes.data_as(C.POINTER(C.c_double)) for v in (wx, wu)]
    call = lambda g, nw=1: L.tqgpu_mpc_adjoint(g.h, C.byref(o), px, pu, nw, None)
    getters = lambda g: (L.tqgpu_mpc_get_adjoint_x0(g.h, None), L.tqgpu_mpc_get_adjoint(g.h, None, None, None))
    g = MC.make(capi, c["base"], root=False)
    assert call(g) == EINVAL          # no root form yet
    g.close()
    g = SN.make(capi, c)
    try:
        assert call(g) == EINVAL          # no solve yet
        _step(g, c)
        assert L.tqgpu_mpc_adjoint(g.h, None, px, pu, 1, None) == EINVAL
        assert getters(g) == (EINVAL, EINVAL)          # nothing computed yet
        assert call(g, 0) == EINVAL and b"nw" in L.tqgpu_last_error()
        assert call(g) == 0 and getters(g) == (0, 0)
        g.set_linear_terms(c["d"]["q"], None)          # an upload
        assert getters(g) == (EINVAL, EINVAL)
        assert call(g) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
        _step(g, c)
        assert getters(g) == (EINVAL, EINVAL)          # a new solve: the stored adjoint belonged to the point before it
        assert call(g) == 0 and getters(g) == (0, 0)
        g.mpc_set_x0(c["x0"])          # a fold without a solve
        assert getters(g) == (EINVAL, EINVAL)
        assert call(g) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
    finally:
        g.close()


@pytest.mark.parametrize("kid", ["dense_kind2_root", "dense_kind3_root"])
def test_kinds_2_and_3_are_refused(capi, kid):
    L = capi.lib()
    o = capi._gpu_opts(0)
    b = MC.case(kid)
    gb = MC.make(capi, b)
    try:
        gb.mpc_step(MC.exact_x0s(b["nx0"], 0)[0], **b["opts"])
        assert L.tqgpu_mpc_adjoint(gb.h, C.byref(o), None, None, 1, None) == EUNSUPPORTED
        assert b"kind 2 or 3" in L.tqgpu_last_error()
    finally:
        gb.close()


def test_a_window_that_does_not_fit_is_refused_before_any_launch(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    c = ML.case(AC.WINDOW_ID)
    g = SN.make(capi, c)
    try:
        _step(g, c)
        assert capi.mpc_stats()["launches"] > 0
        assert L.tqgpu_mpc_adjoint(g.h, C.byref(o), None, None, AC.WINDOW_NW, None) == EUNSUPPORTED
        assert b"160 KiB" in L.tqgpu_last_error()
        assert _counts(capi) == (0, 0, 0)
        wu = np.zeros((int(g.sum_nu), AC.WINDOW_NW - 1))
        wu[0, :] = 1.0
        out = g.mpc_adjoint(None, wu)          # the largest nw that fits
        assert out["gx0"].shape == (c["nx0"], AC.WINDOW_NW - 1)
        _same_bits(out["gx0"][:, -1], out["gx0"][:, 0], "the last column against the first")
    finally:
        g.close()

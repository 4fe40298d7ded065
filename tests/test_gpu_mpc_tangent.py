"""The tangent of an MPC step on the device (tqgpu_mpc_tangent, tqgpu_mpc_get_tangent_u0, tqgpu_mpc_get_tangent) and the predictor built on it
(tqgpu_mpc_predict_at): against tan_ref.dual_form evaluated at the device's own exported point, against the device's adjoint (bit for bit
where the header says so, by duality elsewhere), against the device's sensitivities, and against itself (stored factor or not, one column or
three, direction staged or built on the device).

Cases: tan_cases.py.  Tolerances: 10 times the spread of the two numpy evaluations on the CPU (tan_cases.SPREAD, measured by
test_tan_reference.py), floor 1e-12; dlam is compared where the device reports n_reg == 0.  Everything the calls must leave alone is compared
bit for bit.

The library has no getter of the start buffer.  The duals tqgpu_mpc_predict_at writes there are read through the witness test_gpu_mpc_sens.py
uses for tqgpu_mpc_predict: the error norm of a first iteration started from them is that of a twin started, through tqgpu_set_lambda, from
lam* + dLam added in numpy -- here bit for bit."""
import ctypes as C

import numpy as np
import pytest

import adj_cases as AC
import mpc_cases as MC
import mpc_limit_cases as ML
import sens_cases as SN
import solve_sequence_cases as SC
import tan_cases as TN
import tan_ref as TR
import tracking_cases as TC

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
VALUES = ("dx", "du", "dlam")
DP = C.POINTER(C.c_double)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _step(g, c, x0=None, **kw):
    return g.mpc_step(c["x0"] if x0 is None else x0, **{**c["base"]["opts"], **kw})


def _tangent(g, c, dirs):
    out = g.mpc_tangent(*dirs, **c["base"]["opts"])
    out.update(g.mpc_tangent_values())
    return out


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


def _err(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_against_the_block_reference(capi, cid):
    """items 1, 8 (solution, KKT residual) and 9 (the factor built)"""
    c = TN.case(cid)
    g = SN.make(capi, c)
    try:
        r, _ = _step(g, c)
        assert r["status"] == 0
        sol_before, kkt_before = g.solution(), g.kkt_residual()
        got = g.mpc_tangent(*c["dirs"], **c["base"]["opts"])
        Nh = ML.parent_levels(c["d"]["nk"])
        assert _counts(capi) == (3 * Nh + 2 + 1, 2, 1)          # (+ the packing kernel: the point was not packed ahead or by a certified step)
        got.update(g.mpc_tangent_values())
        sol = g.solution()
        for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
            _same_bits(sol[k], sol_before[k], f"{cid}: {k} after tqgpu_mpc_tangent")
        _same_bits(g.kkt_residual()["res"], kkt_before["res"], f"{cid}: the KKT residual after tqgpu_mpc_tangent")
        ref = TR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["dirs"], c["kinds"])
        assert ref["n_reg"] == 0 and ref["in_range"] < 1e-10
        for what in ("dx", "du", "du0") + (("dlam",) if got["n_reg"] == 0 else ()):
            assert got[what].shape == ref[what].shape, what
            err = _err(got[what], ref[what])
            print(f"{cid} {what}: |device - (b)| = {err:.3e}, tolerance {TN.tol(cid, what):.3e}, n_reg {got['n_reg']}")
            assert err <= TN.tol(cid, what), (what, err)
        assert np.any(got["dx"] != 0.0)
        _same_bits(got["du0"], got["du"][:got["du0"].shape[0]], f"{cid}: du0 against the u rows of the root")
    finally:
        g.close()


@pytest.mark.parametrize("cid", TN.CASE_IDS)
def test_symmetry_duality_sensitivity_and_the_stored_factor(capi, cid):
    """items 2, 3, 4, 8 (stored sensitivity, stored adjoint) and 9 (the factor stored) on one mirror"""
    c = TN.case(cid)
    g = SN.make(capi, c)
    o = c["base"]["opts"]
    try:
        r, _ = _step(g, c)
        assert r["status"] == 0
        Nh = ML.parent_levels(c["d"]["nk"])
        dq, dr, db, dx0 = c["dirs"]
        # 2: the factor built by the tangent itself, then the adjoint behind it, then the tangent behind the stored factor
        built = _tangent(g, c, (dq, dr, None, None))
        adj = g.mpc_adjoint(dq, dr, **o)
        assert _counts(capi) == (2 * Nh + 1, 2, 1)          # the tangent left the factor counted as stored
        adj.update(g.mpc_adjoint_grads())
        stored = _tangent(g, c, (dq, dr, None, None))
        for mine, theirs in (("dx", "gq"), ("du", "gr"), ("dlam", "gb")):
            _same_bits(built[mine], adj[theirs], f"{cid}: {mine} against {theirs}, factor built")
            _same_bits(stored[mine], adj[theirs], f"{cid}: {mine} against {theirs}, factor stored")
        assert built["n_reg"] == adj["n_reg"] == stored["n_reg"]
        # 8: a stored sensitivity and a stored adjoint keep their bits over a full tangent
        g.mpc_sensitivity(**o)
        gain, sens = g.mpc_gain(), g.mpc_sensitivities()
        wadj = g.mpc_adjoint(*c["w"], **o)
        wadj.update(g.mpc_adjoint_grads())
        x0_ref = gain[2].copy()
        with_gb = wadj["n_reg"] == 0          # gb (and with it the db term) takes part only where nothing was regularised
        full = g.mpc_tangent(dq, dr, db if with_gb else None, dx0, **o)
        assert _counts(capi) == (2 * Nh + 1, 2, 1)
        full.update(g.mpc_tangent_values())
        for i in range(3):
            _same_bits(g.mpc_gain()[i], gain[i], f"{cid}: mpc_gain[{i}]")
        for k in VALUES:
            _same_bits(g.mpc_sensitivities()[k], sens[k], f"{cid}: {k} of the stored sensitivity")
        for k, v in g.mpc_adjoint_grads().items():
            _same_bits(v, wadj[k], f"{cid}: {k} of the stored adjoint")
        _same_bits(g.mpc_gain()[2], x0_ref, f"{cid}: x0_ref")
        # 3: duality with the device's adjoint of the same point
        wx, wu = c["w"]
        got = float(wx[:, 0] @ full["dx"][:, 0] + wu[:, 0] @ full["du"][:, 0])
        assert full["n_reg"] == wadj["n_reg"]
        want = float(wadj["gq"][:, 0] @ dq[:, 0] + wadj["gr"][:, 0] @ dr[:, 0] + (wadj["gb"][:, 0] @ db[:, 0] if with_gb else 0.0) + wadj["gx0"][:, 0] @ dx0[:, 0])
        n1 = lambda *v: float(sum(np.sum(np.abs(x)) for x in v))
        bound = max(TN.tol(cid, "dx"), TN.tol(cid, "du")) * n1(wx, wu) + max(AC.tol(cid, k) for k in ("gq", "gr", "gb", "gx0")) * n1(dq, dr, db, dx0)
        print(f"{cid}: |w . dZ - g . dtheta| = {abs(got - want):.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound
        # 4: dx0 = e_j alone against column j of the sensitivity
        sens_spread = SN.SPREAD[cid][:4] if cid in SN.SPREAD else ML.SPREAD[cid]
        for j in sorted({0, int(c["nx0"]) - 1}):
            e = np.zeros(int(c["nx0"]))
            e[j] = 1.0
            one = _tangent(g, c, (None, None, None, e))
            for i, k in ((1, "dx"), (2, "du")):
                bound = TN.tol(cid, k) + max(10.0 * sens_spread[i], SN.FLOOR)          # the sum of what each side is held to
                err = _err(one[k][:, 0], sens[k][:, j])
                print(f"{cid} {k}: |tangent(e_{j}) - column {j}| = {err:.3e}, bound {bound:.3e}")
                assert err <= bound
    finally:
        g.close()


@pytest.mark.parametrize("cid", TN.ND3)
def test_three_columns_are_three_calls(capi, cid):
    """item 5"""
    c = TN.case(cid)
    g = SN.make(capi, c)
    try:
        _step(g, c)
        all3 = _tangent(g, c, c["dirs3"])
        assert all3["du0"].shape == (int(c["d"]["nu"][0]), 3)
        for j in range(3):
            one = _tangent(g, c, tuple(v[:, j] for v in c["dirs3"]))
            for what in VALUES + ("du0",):
                _same_bits(one[what][:, 0], all3[what][:, j], f"{cid}: column {j} of {what}")
        # a missing part of dh means zero; a missing db or dx0 is skipped, which moves no value either
        dq, dr, db, dx0 = c["dirs3"]
        only = _tangent(g, c, (None, dr, db, None))
        zeros = _tangent(g, c, (np.zeros_like(dq), dr, db, np.zeros_like(dx0)))
        for what in VALUES + ("du0",):
            assert np.array_equal(only[what], zeros[what]), what
    finally:
        g.close()


def _track_stepped(capi, c, **kw):
    g = TC.make(capi, c)
    r, _ = g.mpc_step(c["x0"], t0=c["move"][0], **{**c["opts"], **kw})
    assert r["status"] == 0
    return g


@pytest.mark.parametrize("cid", TN.TRACK_IDS)
def test_the_predictor_is_the_tangent_along_its_direction(capi, cid):
    """items 6 (values), 8 (window, x0_ref) and 9 for tqgpu_mpc_predict_at"""
    c = TN.track_case(cid)
    t0, t1 = c["move"]
    g = _track_stepped(capi, c, **SN.TOL12)
    try:
        Nh = ML.parent_levels(c["d"]["nk"])
        sol = g.solution()
        dq, dr = TR.window_direction(c, t0, t1)
        dx0 = c["x0_new"] - c["x0"]
        want = g.mpc_tangent(dq, dr, None, dx0, **c["opts"])
        want.update(g.mpc_tangent_values())
        ref = TR.dual_form(BC_folded(c, t0), sol["x"], sol["u"], c["param"], (dq, dr, None, dx0), c["kinds"])
        for what in ("dx", "du", "du0"):
            err = _err(want[what], ref[what])
            print(f"{cid} {what}: |device - (b)| = {err:.3e}, tolerance {TN.tol(cid, what):.3e}")
            assert err <= TN.tol(cid, what)
        got = g.mpc_predict_at(c["x0_new"], t1, duals=False, **c["opts"])
        assert _counts(capi) == (2 * Nh + 2, 1, 1)
        assert g.mpc_window == t0
        mine = g.mpc_tangent_values()
        for what in VALUES:
            assert np.array_equal(mine[what], want[what]), f"{cid}: {what}, direction built on the device against the staged one: {_err(mine[what], want[what]):.3e}"
        assert np.array_equal(g.mpc_tangent_u0(), want["du0"])
        nu0 = int(c["d"]["nu"][0])
        u0p = sol["u"][:nu0] + want["du0"][:, 0]
        if c["kinds"] is None:
            lo, hi = c["d"]["umin"][:nu0], c["d"]["umax"][:nu0]
            clipped = np.clip(u0p, lo, hi)
            assert got["n_clipped"] == int(np.count_nonzero(clipped != u0p))
            u0p = clipped
        else:
            assert got["n_clipped"] == 0
        _same_bits(got["u0"], u0p, f"{cid}: u0_pred")
        assert got["n_reg"] == want["n_reg"]
        # the window alone, x0 alone
        only_w = g.mpc_predict_at(None, t1, **c["opts"])
        vw = g.mpc_tangent_values()
        ww = _values(g, c, (dq, dr, None, None))
        only_x = g.mpc_predict_at(c["x0_new"], -1, **c["opts"])
        vx = g.mpc_tangent_values()
        wx = _values(g, c, (None, None, None, dx0))
        for what in VALUES:
            assert np.array_equal(vw[what], ww[what]) and np.array_equal(vx[what], wx[what]), what
        assert only_w["n_reg"] == only_x["n_reg"] == want["n_reg"]
    finally:
        g.close()


def BC_folded(c, t0):
    import adjbnd_cases as BC
    return BC.folded(c, t0)


def _values(g, c, dirs):
    g.mpc_tangent(*dirs, **c["opts"])
    return g.mpc_tangent_values()


def test_n_clipped_counts_a_prediction_that_leaves_the_bounds(capi):
    """item 6, second half: x0_new far enough away that the free entries of u[0] are pushed past their bounds"""
    c = TN.case("elim-three_children")
    g = SN.make(capi, c)
    try:
        _step(g, c)
        x1 = c["x0"] + c["dx"] * 2.0 ** 20
        got = g.mpc_predict_at(x1, -1, **c["base"]["opts"])
        nu0 = int(c["d"]["nu"][0])
        want = g.solution()["u"][:nu0] + g.mpc_tangent_u0()[:, 0]
        lo, hi = c["d"]["umin"][:nu0], c["d"]["umax"][:nu0]
        clipped = np.clip(want, lo, hi)
        _same_bits(got["u0"], clipped, "u0_pred")
        assert got["n_clipped"] == int(np.count_nonzero(clipped != want)) and got["n_clipped"] > 0
    finally:
        g.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cid", TN.TRACK_IDS)
def test_the_predicted_duals_start_one_solve(capi, cid, mode):
    """items 6 (the start buffer) and 7"""
    c = TN.track_case(cid)
    t0, t1 = c["move"]
    outs = {}
    for predict in (False, True):
        g = TC.make(capi, c)
        try:
            g.set_lambda(0.125 * np.ones(g.sum_lam))
            g.set_warm_start(mode)
            r, _ = g.mpc_step(c["x0"], t0=t0, **{**c["opts"], **SN.TOL12})
            assert r["status"] == 0
            if predict:
                lam_star = g.solution()["lam"]
                pred = g.mpc_predict_at(c["x0_new"], t1, duals=True, **c["opts"])
                dlam = g.mpc_tangent_values()["dlam"][:, 0]
                # the witness of the start buffer: one iteration from it against one iteration of a twin started from lam* + dLam
                twin = TC.make(capi, c)
                try:
                    twin.mpc_step(c["x0"], t0=t0, **{**c["opts"], **SN.TOL12})
                    twin.set_warm_start(0)
                    twin.set_lambda(lam_star + dlam)
                    rt, _ = twin.mpc_step(c["x0_new"], t0=t1, **{**c["opts"], "maxIter": 1})
                finally:
                    twin.close()
                probe = TC.make(capi, c)
                try:
                    probe.set_lambda(0.125 * np.ones(probe.sum_lam))
                    probe.set_warm_start(mode)
                    probe.mpc_step(c["x0"], t0=t0, **{**c["opts"], **SN.TOL12})
                    probe.mpc_predict_at(c["x0_new"], t1, duals=True, **c["opts"])
                    rp, _ = probe.mpc_step(c["x0_new"], t0=t1, **{**c["opts"], "maxIter": 1})
                finally:
                    probe.close()
                assert rp["last_error_norm"] == rt["last_error_norm"], (rp["last_error_norm"], rt["last_error_norm"])
            r, u = g.mpc_step(c["x0_new"], t0=t1, **{**c["opts"], **SN.TOL12})
            assert r["status"] == 0
            outs[predict] = (r["iter"], u.copy(), pred["u0"] if predict else None)
        finally:
            g.close()
    print(f"{cid} mode {mode}: iterations {outs[False][0]} without the predictor, {outs[True][0]} with it")
    assert outs[True][0] <= outs[False][0]
    if TN.TRACK_SPREAD[cid][4] is not None:          # test_tan_reference.py found the set of bound-sitting entries unchanged
        err = _err(outs[True][1], outs[True][2])
        print(f"{cid} mode {mode}: |u[0] of the step - u0_pred| = {err:.3e}, tolerance {TN.tol(cid, 'fd'):.3e}")
        assert err <= TN.tol(cid, "fd")


@pytest.mark.parametrize("cid", ["elim-single_wg", "states-generic", "elim-dense_kind1_root"])
def test_the_next_step_is_not_disturbed(capi, cid):
    """item 8, last sentence: without duals the next step is that of a run without the calls"""
    c = TN.case(cid)
    outs = []
    for with_call in (False, True):
        g = SN.make(capi, c)
        try:
            g.set_warm_start(1)
            _step(g, c)
            if with_call:
                _tangent(g, c, c["dirs"])
                g.mpc_predict_at(c["x0"] + c["dx0"], -1, duals=False, **c["base"]["opts"])
            r, u = _step(g, c, x0=c["x0"] + c["dx"] * 2.0 ** 12)
            outs.append((r["iter"], r["ls_total"], u.copy()))
        finally:
            g.close()
    assert outs[0][:2] == outs[1][:2]
    _same_bits(outs[0][2], outs[1][2], f"{cid}: u[0] of the next step")


def test_refusals_and_invalidation(capi):
    """item 10: nothing is launched, the stats do not move, the stored results stay"""
    L = capi.lib()
    o = capi._gpu_opts(0)
    c = TN.case("elim-one_child")
    dirs = [np.ascontiguousarray(v[:, 0]) for v in c["dirs"]]
    p = [v.ctypes.data_as(DP) for v in dirs]
    call = lambda g, nd=1: L.tqgpu_mpc_tangent(g.h, C.byref(o), p[0], p[1], p[2], p[3], nd, None)
    pred = lambda g, t0=-1: L.tqgpu_mpc_predict_at(g.h, C.byref(o), p[3], t0, None, 0, None, None)
    getters = lambda g: (L.tqgpu_mpc_get_tangent_u0(g.h, None), L.tqgpu_mpc_get_tangent(g.h, None, None, None))
    g = MC.make(capi, c["base"], root=False)
    assert call(g) == EINVAL and pred(g) == EINVAL          # no root form yet
    g.close()
    g = SN.make(capi, c)
    try:
        assert call(g) == EINVAL and pred(g) == EINVAL          # no solve yet
        _step(g, c)
        stats = _counts(capi)
        assert L.tqgpu_mpc_tangent(g.h, None, p[0], p[1], p[2], p[3], 1, None) == EINVAL
        assert getters(g) == (EINVAL, EINVAL)          # nothing computed yet
        assert call(g, 0) == EINVAL and b"nd" in L.tqgpu_last_error()
        assert L.tqgpu_mpc_tangent(g.h, C.byref(o), None, None, None, None, 1, None) == EINVAL and b"NULL" in L.tqgpu_last_error()
        assert pred(g, 0) == EINVAL and b"tqgpu_mpc_set_tracking" in L.tqgpu_last_error()          # t0_new >= 0 without tracking
        assert _counts(capi) == stats
        assert call(g) == 0 and getters(g) == (0, 0)
        kept = g.mpc_tangent_values()
        assert call(g, 0) == EINVAL and pred(g, 0) == EINVAL
        for k in VALUES:
            _same_bits(g.mpc_tangent_values()[k], kept[k], f"{k} after a refusal")
        g.set_linear_terms(c["d"]["q"], None)          # an upload
        assert getters(g) == (EINVAL, EINVAL)
        stats = _counts(capi)
        assert call(g) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
        assert pred(g) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
        assert _counts(capi) == stats
        _step(g, c)
        assert getters(g) == (EINVAL, EINVAL)          # a new solve: the stored tangent belonged to the point before it
        assert pred(g) == 0 and getters(g) == (0, 0)
        g.mpc_set_x0(c["x0"])          # a fold without a solve
        assert getters(g) == (EINVAL, EINVAL)
        assert call(g) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
    finally:
        g.close()
    t = TN.track_case("single_wg")
    g = TC.make(capi, t)
    try:
        g.mpc_step(t["x0"], **t["opts"])
        x = np.ascontiguousarray(t["x0_new"])
        assert L.tqgpu_mpc_predict_at(g.h, C.byref(o), x.ctypes.data_as(DP), 1, None, 0, None, None) == EINVAL and b"window" in L.tqgpu_last_error()          # no window in force
        g.mpc_step(t["x0"], t0=1, **t["opts"])
        assert L.tqgpu_mpc_predict_at(g.h, C.byref(o), x.ctypes.data_as(DP), 2, None, 0, None, None) == 0
        g.mpc_set_window(2)          # a window move without a solve
        assert getters(g) == (EINVAL, EINVAL)
        assert L.tqgpu_mpc_predict_at(g.h, C.byref(o), x.ctypes.data_as(DP), 3, None, 0, None, None) == EINVAL and b"since the last solve" in L.tqgpu_last_error()
    finally:
        g.close()


@pytest.mark.parametrize("kid", ["dense_kind2_root", "dense_kind3_root"])
def test_kinds_2_and_3_are_refused(capi, kid):
    L = capi.lib()
    o = capi._gpu_opts(0)
    b = MC.case(kid)
    gb = MC.make(capi, b)
    try:
        x0 = MC.exact_x0s(b["nx0"], 0)[0]
        gb.mpc_step(x0, **b["opts"])
        stats = _counts(capi)
        e = np.ones(int(b["nx0"]))
        assert L.tqgpu_mpc_tangent(gb.h, C.byref(o), None, None, None, e.ctypes.data_as(DP), 1, None) == EUNSUPPORTED
        assert b"kind 2 or 3" in L.tqgpu_last_error()
        assert L.tqgpu_mpc_predict_at(gb.h, C.byref(o), e.ctypes.data_as(DP), -1, None, 0, None, None) == EUNSUPPORTED
        assert b"kind 2 or 3" in L.tqgpu_last_error()
        assert _counts(capi) == stats
    finally:
        gb.close()


def test_a_rank_of_a_sharded_solve_is_refused(capi):
    from treeqp_amd import problems as P
    g = SC._lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05))(capi)
    try:
        g.pshard_init(0, 2)
        L = capi.lib()
        o = capi._gpu_opts(0)
        e = np.ones(64)
        assert L.tqgpu_mpc_tangent(g.h, C.byref(o), None, None, None, e.ctypes.data_as(DP), 1, None) == EUNSUPPORTED
        assert L.tqgpu_mpc_predict_at(g.h, C.byref(o), e.ctypes.data_as(DP), -1, None, 0, None, None) == EUNSUPPORTED
        assert L.tqgpu_mpc_get_tangent_u0(g.h, None) == EUNSUPPORTED and L.tqgpu_mpc_get_tangent(g.h, None, None, None) == EUNSUPPORTED
    finally:
        g.close()


def test_a_window_that_does_not_fit_is_refused_before_any_launch(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    c = TN.window_case()
    g = SN.make(capi, c)
    try:
        _step(g, c)
        stats = _counts(capi)
        assert stats[0] > 0
        dr = np.zeros((int(g.sum_nu), TN.WINDOW_ND))
        dr[0, :] = 1.0
        assert L.tqgpu_mpc_tangent(g.h, C.byref(o), None, dr.ctypes.data_as(DP), None, None, TN.WINDOW_ND, None) == EUNSUPPORTED
        assert b"160 KiB" in L.tqgpu_last_error()
        assert _counts(capi) == stats
        out = g.mpc_tangent(None, np.asfortranarray(dr[:, :-1]))          # the largest nd that fits
        assert out["du0"].shape == (int(c["d"]["nu"][0]), TN.WINDOW_ND - 1)
        _same_bits(out["du0"][:, -1], out["du0"][:, 0], "the last column against the first")
    finally:
        g.close()

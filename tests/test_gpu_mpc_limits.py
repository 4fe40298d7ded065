"""The MPC and sensitivity kernels on both sides of their size limits (mpc_limit_cases.py: one row per limit, its docstring says which
sides exist): k_sens_hess / _factor / _forward / _primal and k_mpc_predict against sens_ref.dense_kkt at the device's own exported point,
the refusals of setup_sens, the fold and the window fold of k_mpc_pre against the numpy chains, k_mpc_post and k_mpc_post_batch against
tqgpu_get_solution.

Tolerances: the sensitivities 10 times the spread of the two numpy evaluations on the CPU (mpc_limit_cases.SPREAD, measured by
test_mpc_limits_reference.py), floor 1e-12; every reference regularises nothing there, so the device must report n_reg == 0 and dlam is
compared on every case.  Everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import mpc_cases as MC
import mpc_limit_cases as ML
import mpc_root_cases as MR
import sens_cases as SN
import sens_ref as SR
import tracking_cases as TK

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")
COUNTS = ("status", "iter", "ls_total")
EUNSUPPORTED = -4


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _step(g, c, x0=None, **kw):
    return g.mpc_step(c["x0"] if x0 is None else x0, **{**c["base"]["opts"], **kw})


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the sensitivities
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_sensitivities(capi, cid):
    c = ML.case(cid)
    g = SN.make(capi, c)
    try:
        r, u0 = _step(g, c)
        assert r["status"] == 0
        sol_before = g.solution()
        kkt_before = g.kkt_residual()
        n_reg = g.mpc_sensitivity(**c["base"]["opts"])
        st = capi.mpc_stats()
        Nh = ML.parent_levels(c["d"]["nk"])
        assert (st["copies"], st["waits"]) == (1, 1), st
        assert st["launches"] == 1 + Nh + (Nh - 1) + 1 + 1, st          # (+ the packing kernel: the point was not packed ahead)
        assert n_reg == 0, f"{cid}: the reference regularises no block, the device {n_reg}"
        K, u0s, x0r = g.mpc_gain()
        s = g.mpc_sensitivities()
        sol = g.solution()
        for k in SOL_KEYS + ("dlam",):
            _same_bits(sol[k], sol_before[k], f"{cid}: {k} after tqgpu_mpc_sensitivity")
        _same_bits(g.kkt_residual()["res"], kkt_before["res"], f"{cid}: the KKT residual after tqgpu_mpc_sensitivity")
        assert np.array_equal(u0s, sol["u"][:len(u0s)]) and np.array_equal(u0s, u0) and np.array_equal(x0r, c["x0"])
        ref = SR.dense_kkt(c["d"], sol["x"], sol["u"], c["param"], c["kinds"])
        assert ref["residual"] < 1e-9 * ref["scale"]
        got = dict(K=K, dx=s["dx"], du=s["du"], dlam=s["dlam"])
        for what in ("K", "dx", "du", "dlam"):
            assert got[what].shape == ref[what].shape, what
            err = float(np.max(np.abs(got[what] - ref[what]))) if ref[what].size else 0.0
            print(f"{cid} {what}: |device - (a)| = {err:.3e}, tolerance {ML.tol(cid, what):.3e}")
            assert err <= ML.tol(cid, what), (what, err)
        on = SR.pinned(c["d"], sol["x"], sol["u"], c["kinds"])
        nu0, sx = len(u0s), len(sol["x"])
        for i in range(nu0):
            if on[sx + i]:
                assert np.all(K[i] == 0.0), f"row {i} of K: u[0][{i}] sits on a bound"
        if c["kinds"] is None:
            assert not on[sx:sx + nu0].all() and on[c["nx0"] if c["form"] == "states" else 0:].any()
        if c["form"] == "states":
            assert np.array_equal(s["dx"][:c["nx0"]], np.eye(c["nx0"]))
        assert np.array_equal(K, s["du"][:nu0])
    finally:
        g.close()


@pytest.mark.parametrize("cid", ML.ACCEPTED_IDS)
def test_sensitivities_against_the_dense_kkt_reference(capi, cid):
    _check_sensitivities(capi, cid)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the prediction
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ML.PREDICT_IDS)
def test_predict_is_the_fma_chain(capi, cid):
    """at dx * 2^10 nothing leaves its box; at dx * 2^20 entries clip below index 64 and, where nu[0] > 64, at 64 and above"""
    c = ML.case(cid)
    g = SN.make(capi, c)
    try:
        _step(g, c)
        g.mpc_sensitivity()
        K, u0s, x0r = g.mpc_gain()
        nu0 = len(u0s)
        lo, hi = c["d"]["umin"][:nu0], c["d"]["umax"][:nu0]
        for scale in (2.0 ** 10, 2.0 ** 20):
            dx = c["dx"] * scale
            x1 = x0r + dx
            assert np.array_equal(x1 - x0r, dx)
            want = u0s.copy()
            for j in range(len(dx)):
                want = np.array([ML.fma(K[i, j], dx[j], want[i]) for i in range(nu0)])
            clipped = np.clip(want, lo, hi)
            got, n = g.mpc_predict(x1)
            _same_bits(got, clipped, f"{cid} scale {scale}: u0_pred")
            moved = clipped != want
            print(f"{cid} scale {scale}: {int(moved.sum())} clipped, {int(moved[64:].sum())} of them at index 64 or above")
            assert n == int(np.count_nonzero(moved))
            if scale > 2.0 ** 10:
                assert moved[:64].any() and (nu0 <= 64 or moved[64:].any()), "the clipping branch was not reached on every side of 64"
            st = capi.mpc_stats()
            assert (st["launches"], st["copies"], st["waits"]) == (1, 0, 1), st
    finally:
        g.close()


def test_predicted_duals_start_one_solve(capi):
    """as test_gpu_mpc_sens.test_predicted_duals_start_one_solve (mode 0), on the tree whose root block has 65 rows: blocks 1 + k of
    k_mpc_predict stride a node's duals by the wave"""
    c = ML.case(ML.DUALS_ID)
    g, twin = SN.make(capi, c), SN.make(capi, c)
    try:
        _step(g, c, **SN.TOL12)
        lam_star = g.solution()["lam"]
        g.mpc_sensitivity()
        dlam = g.mpc_sensitivities()["dlam"]
        x1 = c["x0"] + c["dx"] * 2.0 ** 10
        g.mpc_predict(x1, duals=True)
        r1, _ = _step(g, c, x0=x1, maxIter=1)
        twin.set_lambda(lam_star + dlam @ (x1 - c["x0"]))
        rt, _ = _step(twin, c, x0=x1, maxIter=1)
        assert abs(r1["last_error_norm"] - rt["last_error_norm"]) <= 1e-13 * max(1.0, abs(rt["last_error_norm"]))
    finally:
        g.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the refusals of setup_sens (their accepted neighbours are cases of 1.)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refused,accepted", ML.REFUSAL_PAIRS)
def test_a_window_past_160_kib_is_refused_and_nothing_is_launched(capi, refused, accepted):
    assert accepted in ML.ACCEPTED_IDS
    c = ML.case(refused)
    L, o = capi.lib(), capi._gpu_opts(0)
    g, twin = SN.make(capi, c), SN.make(capi, c)
    try:
        for m in (g, twin):
            m.set_warm_start(1)
            r, _ = _step(m, c)
            assert r["status"] == 0
        assert capi.mpc_stats()["launches"] > 0
        rc = L.tqgpu_mpc_sensitivity(g.h, C.byref(o), None)
        assert rc == EUNSUPPORTED, f"{rc}: {L.tqgpu_last_error().decode()}"
        assert b"160 KiB" in L.tqgpu_last_error()
        assert capi.mpc_stats() == dict(launches=0, copies=0, waits=0)          # the call's own record: nothing went out
        assert L.tqgpu_mpc_get_gain(g.h, None, None, None) == -2
        x1 = c["x0"] + c["dx"] * 2.0 ** 12
        (ra, ua), (rb, ub) = _step(g, c, x0=x1), _step(twin, c, x0=x1)
        for k in COUNTS:
            assert ra[k] == rb[k], k
        _same_bits(ua, ub, f"{refused}: u0 of the next step")
        sa, sb = g.solution(), twin.solution()
        for k in SOL_KEYS:
            _same_bits(sa[k], sb[k], f"{refused}: {k} of the next step")
    finally:
        g.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the fold and the warm start
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(ML.FOLD_ELIM))
def test_exact_fold_and_loop_bit_for_bit(capi, cid):
    c = ML.fold_elim_case(cid)
    dev, host = MC.make(capi, c), MC.make(capi, c, root=False)
    dev.set_warm_start(1)
    lam = None
    try:
        for step, x0 in enumerate(MC.exact_x0s(c["nx0"], 0)[:3]):
            terms = MC.fold(c["root"], x0)
            back = MC.fold(c["root"], x0, order=np.arange(c["nx0"])[::-1])
            dev.mpc_set_x0(x0)
            got = dev.root_terms()
            for k, v in terms.items():
                assert np.array_equal(v, back[k]), f"{cid}: the data are not exact"
                _same_bits(got[k], v, f"{cid} step {step}: root term {k}")
            rd, u0 = dev.mpc_step(x0, **c["opts"])
            sd = dev.solution()
            MC.host_upload(host, c, terms)
            host.set_lambda(lam)
            rh = host.solve(**c["opts"])
            sh = host.solution()
            lam = sh["lam"]
            for k in COUNTS:
                assert rd[k] == rh[k], f"{cid} step {step}: {k} {rd[k]} != {rh[k]}"
            _same_bits(u0, sh["u"][:len(u0)], f"{cid} step {step}: u0")
            for k in SOL_KEYS:
                _same_bits(sd[k], sh[k], f"{cid} step {step}: {k}")
    finally:
        dev.close(); host.close()


def _states_loop(capi, c, xs, before=None):
    dev, host = MR.make(capi, c, root_states=True), MR.make(capi, c)
    dev.set_warm_start(1); host.set_warm_start(1)
    d2 = None
    try:
        if before == "solve":          # the persistent route's constants are packed and current when the first fold comes
            dev.solve(**c["opts"]); host.solve(**c["opts"])
        for step, x0 in enumerate(xs):
            if before == "bounds" and step in (0, 2):          # a re-pack is pending when the fold comes: it reads the folded Data
                d2 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
                nu0 = int(d2["nu"][0])
                d2["umax"][nu0:2 * nu0] *= 0.5 + 0.1 * step
                MR.set_bounds(capi, dev, MR.with_x0(c, xs[max(step - 1, 0)], d2))
            dev.mpc_set_x0(x0)
            lo, hi = dev.root_bounds()
            _same_bits(lo, x0, f"{c['id']} step {step}: xmin[0]"); _same_bits(hi, x0, f"{c['id']} step {step}: xmax[0]")
            rd, u0 = dev.mpc_step(x0, **c["opts"])
            sd = dev.solution()
            rh, sh = MR.host_step(capi, host, c, x0, d2)
            for k in COUNTS:
                assert rd[k] == rh[k], f"{c['id']} step {step}: {k} {rd[k]} != {rh[k]}"
            _same_bits(u0, sh["u"][:len(u0)], f"{c['id']} step {step}: u0")
            for k in SOL_KEYS:
                _same_bits(sd[k], sh[k], f"{c['id']} step {step}: {k}")
    finally:
        dev.close(); host.close()


@pytest.mark.parametrize("cid", list(ML.FOLD_STATES))
def test_root_states_fold_and_loop_bit_for_bit(capi, cid):
    c = ML.fold_states_case(cid)
    xs = MR.x0_sequence(c, steps=3)
    xs[0][63] = -0.0
    xs[1][c["nx0"] - 1] = 5e-324
    _states_loop(capi, c, xs)


@pytest.mark.parametrize("before", ["solve", "bounds"])
def test_persistent_route_fold_with_constants_current_and_pack_pending(capi, before):
    """the (8, 4, 2) tree, the largest nx and nx + nu of the persistent route: the `i < 16` gate on the root's packed constants lets
    every state through"""
    c = ML.persist_case()
    _states_loop(capi, c, MR.x0_sequence(c, steps=3), before)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the window fold
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ML.TRACKING_IDS)
def test_window_fold_bit_for_bit(capi, cid):
    c = ML.tracking_case(cid)
    g = TK.make(capi, c)
    try:
        assert g.mpc_window == -1
        x0 = c["x0s"][0] if c["form"] == "elim" else None
        if x0 is not None:
            g.mpc_set_x0(x0)
        for t0 in ML.TRACK_WINDOWS:
            g.mpc_set_window(t0)
            assert g.mpc_window == t0
            q, r = g.linear_terms()
            qn, rn = TK.fold(c, t0, x0)
            _same_bits(q, qn, f"{cid} window {t0}: q"); _same_bits(r, rn, f"{cid} window {t0}: r")
        if x0 is not None:          # x0 moves after the window: r[0] is one chain from the tracked base
            x1 = c["x0s"][1]
            g.mpc_set_x0(x1)
            q, r = g.linear_terms()
            qn, rn = TK.fold(c, ML.TRACK_WINDOWS[-1], x1)
            _same_bits(q, qn, f"{cid}: q after an x0 fold"); _same_bits(r, rn, f"{cid}: r after an x0 fold")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the post of u[0]
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu0", [256, 257])
def test_single_post_past_256_threads(capi, nu0):
    c = ML.post_case(nu0)
    g = MC.make(capi, c)
    try:
        for x0 in MC.exact_x0s(c["nx0"], 0)[:2]:
            r, u0 = g.mpc_step(x0, **c["opts"])
            assert r["status"] == 0 and len(u0) == nu0
            u = g.solution()["u"][:nu0]
            _same_bits(u0, u, f"nu[0] = {nu0}: u0")
            assert np.count_nonzero(u0) > nu0 // 2 and u0[nu0 - 1] != 0.0
    finally:
        g.close()


def _batch(capi, cs, steps=3):
    rng = np.random.Generator(np.random.PCG64(77))
    x0s = [[MC.quantised(rng, c["nx0"], 1.0) for c in cs] for _ in range(steps)]
    members, alone = [MC.make(capi, c) for c in cs], [MC.make(capi, c) for c in cs]
    try:
        for g in members + alone:
            g.set_warm_start(1)
        for step in range(steps):
            res, u0s = capi.mpc_step_batch(members, x0s[step], **cs[0]["opts"])
            for i, c in enumerate(cs):
                ra, ua = alone[i].mpc_step(x0s[step][i], **c["opts"])
                for k in COUNTS:
                    assert res[i][k] == ra[k], f"step {step} member {i}: {k}"
                assert res[i]["status"] == 0
                _same_bits(u0s[i], ua, f"step {step} member {i}: u0")
                sm, sa = members[i].solution(), alone[i].solution()
                _same_bits(u0s[i], sm["u"][:int(c["d"]["nu"][0])], f"step {step} member {i}: u0 against the solution")
                for k in SOL_KEYS:
                    _same_bits(sm[k], sa[k], f"step {step} member {i}: {k}")
                assert np.count_nonzero(u0s[i]) > 0 and u0s[i][-1] != 0.0
    finally:
        for g in members + alone:
            g.close()


def test_batch_post_of_16_members_of_16_inputs(capi):
    a, _ = ML.batch_cases()
    _batch(capi, [a] * 16)


def test_batch_post_of_17_members_of_two_trees(capi):
    """17 members: the walk `m += 16` takes a second turn; members of nu[0] = 17 take a second turn of their 16 lanes; the two trees' launches
    ahead have 3 and 4 blocks (nk0 + 1 + one warm span), the batch's launch the larger"""
    a, b = ML.batch_cases()
    _batch(capi, [a, b] * 8 + [b])

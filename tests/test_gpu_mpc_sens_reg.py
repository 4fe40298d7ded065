"""The regularised and zero-pivot branches of the MPC derivative kernels on the device (sens_factor_body and the substitutions behind it:
tqgpu_mpc_sensitivity, tqgpu_mpc_adjoint, their batch forms, tqgpu_mpc_predict) against sens_ref.dual_form and adj_ref.dual_form evaluated
at the device's own exported point with the same regType, regTol, regValue.

Rows: sens_reg_cases.py (threshold: a regTol between the first-pass pivots, one block or all blocks shifted, regType 1; pinned: an exact
zero pivot under the default shift, a shift of 2^-6, regType 0 and regTol = 0.0; two batches).  test_sens_reg_reference.py asserts on the
CPU that every row reaches the branch it is meant for with a guard of at least 1 % between regTol and the nearest pivot.
Tolerances: 10 times the spread of dual_form against dense_shifted on the CPU (sens_reg_cases.SPREAD), floor 1e-12; dlam and gb are
compared on every row, both sides solve the same shifted system.  The regType 0 rows are also held to sens_ref.dense_kkt, the exact
derivative (SPREAD_KKT).  The shifted rows are not: a shift moves dZ by O(regValue), see test_the_default_shift_moves_dz_by_its_size.
Everything a call must leave alone, every twin and every batch member against its single call is compared bit for bit."""
import numpy as np
import pytest

import adj_ref as AR
import sens_cases as SN
import sens_ref as SR
import sens_reg_cases as RC
from test_gpu_mpc_sens import _fma

pytestmark = pytest.mark.gpu

SENS = ("K", "dx", "du", "dlam")
GRADS = ("gq", "gr", "gb", "gx0")
SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u", "dlam")


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _close(gs):
    for g in gs:
        g.close()


def _stepped(capi, c):
    g = SN.make(capi, c)
    try:
        r, _ = g.mpc_step(c["x0"], **c["base"]["opts"])
        assert r["status"] == 0
    except Exception:
        g.close()
        raise
    return g


def _sens(g, opts):
    out = dict(n_reg=g.mpc_sensitivity(**opts))
    out["K"] = g.mpc_gain()[0]
    out.update(g.mpc_sensitivities())
    return out


def _adj(g, w, opts):
    out = g.mpc_adjoint(w[0], w[1], **opts)
    out.update(g.mpc_adjoint_grads())
    return out


def _within(rid, got, ref, keys, tol, against):
    for what in keys:
        assert got[what].shape == ref[what].shape, what
        err = float(np.max(np.abs(got[what] - ref[what]), initial=0.0))
        print(f"{rid} {what}: |device - {against}| = {err:.3e}, tolerance {tol(rid, what):.3e}")
        assert err <= tol(rid, what), (rid, what, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the sensitivities
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RC.ROW_IDS)
def test_sensitivity_against_the_block_reference(capi, rid):
    r = RC.row(rid)
    c = r["case"]
    g = _stepped(capi, c)
    try:
        sol_before, kkt_before = g.solution(), g.kkt_residual()
        got = _sens(g, r["opts"])
        sol = g.solution()
        for k in SOL_KEYS:
            _same_bits(sol[k], sol_before[k], f"{rid}: {k} after tqgpu_mpc_sensitivity")
        _same_bits(g.kkt_residual()["res"], kkt_before["res"], f"{rid}: the KKT residual after tqgpu_mpc_sensitivity")
        ref = SR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["kinds"], **r["opts"])
        assert ref["flagged"] == r["flagged"] and ref["guard"] >= 1.01, "the device's point is not the row's"
        assert got["n_reg"] == ref["n_reg"] == r["n_reg"], f"{rid}: the reference regularises {ref['n_reg']} blocks, the device {got['n_reg']}"
        _within(rid, got, ref, SENS, RC.tol, "(b)")
        nu0, sx = got["K"].shape[0], len(sol["x"])
        _same_bits(got["K"], got["du"][:nu0], f"{rid}: K against the first rows of du")
        on = SR.pinned(c["d"], sol["x"], sol["u"], c["kinds"])
        for i in range(nu0):
            if on[sx + i]:
                assert np.all(got["K"][i] == 0.0), f"row {i} of K: u[0][{i}] sits on a bound"
        if c["form"] == "states":
            assert np.array_equal(got["dx"][:c["nx0"]], np.eye(c["nx0"]))
        if r["opts"]["regType"] == 0 and r["zero"]:
            assert list(np.flatnonzero(ref["zero"])) == r["zero"]
            assert np.all(got["dlam"][r["zero"]] == 0.0), "the zero column's entries of dlam"
            exact = SR.dense_kkt(c["d"], sol["x"], sol["u"], c["param"], c["kinds"])
            assert exact["residual"] < 1e-9 * exact["scale"]
            _within(rid, got, exact, ("K", "dx", "du"), RC.tol_kkt, "(a)")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the adjoint
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,nw", [(rid, 1) for rid in RC.ROW_IDS] + [(RC.NW3_ID, 3)])
def test_adjoint_against_the_block_reference(capi, rid, nw):
    """the adjoint that builds the factor itself against the reference, then against the adjoint behind a sensitivity called with the same
    options (bit for bit) and against that sensitivity's dZ' w"""
    r = RC.row(rid)
    c = r["case"]
    w = c["w"] if nw == 1 else c["w3"]
    g = _stepped(capi, c)
    try:
        built = _adj(g, w, r["opts"])
        sol = g.solution()
        ref = AR.dual_form(c["d"], sol["x"], sol["u"], c["param"], w, c["kinds"], **r["opts"])
        assert ref["flagged"] == r["flagged"]
        assert built["n_reg"] == ref["n_reg"] == r["n_reg"], f"{rid}: the reference regularises {ref['n_reg']} blocks, the device {built['n_reg']}"
        _within(rid, built, ref, GRADS, RC.tol, "(b)")
        if r["opts"]["regType"] == 0 and r["zero"]:
            assert np.all(built["gb"][r["zero"]] == 0.0), "the zero column's entries of gb"
        s = _sens(g, r["opts"])
        stored = _adj(g, w, r["opts"])
        assert stored["n_reg"] == built["n_reg"] == s["n_reg"]
        for what in GRADS:
            _same_bits(stored[what], built[what], f"{rid}: {what}, factor stored against factor built")
        want = np.vstack([s["dx"], s["du"]]).T @ np.vstack(w)
        err = float(np.max(np.abs(stored["gx0"] - want)))
        print(f"{rid}: |gx0 - dZ' w| = {err:.3e}, tolerance {RC.tol(rid, 'gx0'):.3e}")
        assert err <= RC.tol(rid, "gx0")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a stored factor is the earlier call's; nothing of it survives the next factorisation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [rid for rid in RC.ROW_IDS if not rid.endswith("-default")])          # every row whose options are not the default
def test_the_factor_is_the_earlier_call_s(capi, rid):
    r = RC.row(rid)
    c = r["case"]
    g, twin = _stepped(capi, c), _stepped(capi, c)
    try:
        assert _sens(g, r["opts"])["n_reg"] == r["n_reg"]
        lazy = _adj(g, c["w"], RC.DEFAULT)          # the header: a stored factor is used as it is, built with the opts of that call
        _sens(twin, r["opts"])
        same = _adj(twin, c["w"], r["opts"])
        assert lazy["n_reg"] == same["n_reg"] == r["n_reg"], "the stored count"
        for what in GRADS:
            _same_bits(lazy[what], same[what], f"{rid}: {what}, default options behind the row's sensitivity")
        again = _sens(g, RC.DEFAULT)          # a new factorisation: no shift and no count of the one before
        fresh = _stepped(capi, c)
        try:
            want = _sens(fresh, RC.DEFAULT)
        finally:
            fresh.close()
        sol = g.solution()
        ref = SR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["kinds"], **RC.DEFAULT)
        assert again["n_reg"] == want["n_reg"] == ref["n_reg"]
        if r["group"] == "threshold":
            assert again["n_reg"] == 0
        for what in SENS:
            _same_bits(again[what], want[what], f"{rid}: {what} of the default call behind the row's")
        moved = max(float(np.max(np.abs(again[k] - SR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["kinds"], **r["opts"])[k]))) for k in ("dx", "du"))
        assert moved > 1e-9, "the row's options and the default give the same numbers: the check above proves nothing"
    finally:
        _close([g, twin])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the predictor over a regularised gain
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", RC.PREDICT_IDS)
def test_predict_is_the_fma_chain(capi, rid):
    r = RC.row(rid)
    c = r["case"]
    g = _stepped(capi, c)
    try:
        assert g.mpc_sensitivity(**r["opts"]) == r["n_reg"] > 0
        K, u0s, x0r = g.mpc_gain()
        assert np.any(K != 0.0)
        lo, hi = c["d"]["umin"][:len(u0s)], c["d"]["umax"][:len(u0s)]
        for scale in (2.0 ** 10, 2.0 ** 20):
            dx = c["dx"] * scale
            x1 = x0r + dx
            assert np.array_equal(x1 - x0r, dx)
            want = u0s.copy()
            for j in range(len(dx)):
                want = np.array([_fma(K[i, j], dx[j], want[i]) for i in range(len(want))])
            clipped = np.clip(want, lo, hi)
            got, n = g.mpc_predict(x1)
            _same_bits(got, clipped, f"{rid} scale {scale}: u0_pred")
            assert n == int(np.count_nonzero(clipped != want))
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the batches
# ---------------------------------------------------------------------------------------------------------------------------------
def _member_tol(bid, m):
    rid = RC.BATCHES[bid][m][0]
    if rid == "regular":
        import adj_cases as AC
        return lambda _, what: SN.tol(RC.REGULAR, what) if what in SENS else AC.tol(RC.REGULAR, what)
    return lambda _, what: RC.tol(rid, what)


def _batch_mirrors(capi, bid):
    """(members, twins): two sets of fresh mirrors of the batch, stepped the same way; the step is made twice, as test_gpu_mpc_sens_batch.py
    does: the second is the steady state of a loop"""
    mem = RC.members(bid)
    gs = []
    try:
        for _ in range(2):
            for c, _, _ in mem:
                gs.append(SN.make(capi, c))
        n = len(mem)
        for part in (gs[:n], gs[n:]):
            for _ in range(2):
                res, _ = capi.mpc_step_batch(part, [x0 for _, x0, _ in mem])
                assert all(r["status"] == 0 for r in res)
    except Exception:
        _close(gs)
        raise
    return mem, gs[:n], gs[n:]


@pytest.mark.parametrize("mode", ["batched", "members"])
@pytest.mark.parametrize("bid", RC.BATCH_IDS)
def test_sensitivity_batch(capi, monkeypatch, bid, mode):
    if mode == "members":
        monkeypatch.setenv("TREEQP_AMD_SENS_BATCH", "members")          # read by every call
    mem, gs, twins = _batch_mirrors(capi, bid)
    try:
        want_n = [n for _, _, n in mem]
        n_regs = capi.mpc_sensitivity_batch(gs, **RC.DEFAULT)
        assert n_regs == want_n, f"{bid}: n_reg per member"
        for m, ((c, x0, _), g, t) in enumerate(zip(mem, gs, twins)):
            one = _sens(t, RC.DEFAULT)
            assert one["n_reg"] == n_regs[m]
            got = dict(K=g.mpc_gain()[0], **g.mpc_sensitivities())
            for what in SENS:
                _same_bits(got[what], one[what], f"{bid}[{m}]: {what}, batch against the single call")
            sol = g.solution()
            d = SN.problem_at(c, x0)
            ref = SR.dual_form(d, sol["x"], sol["u"], c["param"], c["kinds"], **RC.DEFAULT)
            assert ref["n_reg"] == n_regs[m]
            _within(f"{bid}[{m}]", got, ref, SENS, _member_tol(bid, m), "(b)")
        assert capi.mpc_sensitivity_batch(gs, **RC.DEFAULT) == want_n, "the second call on the same mirrors"
    finally:
        _close(gs + twins)


@pytest.mark.parametrize("mode", ["batched", "members"])
@pytest.mark.parametrize("bid", RC.BATCH_IDS)
def test_adjoint_batch(capi, monkeypatch, bid, mode):
    if mode == "members":
        monkeypatch.setenv("TREEQP_AMD_ADJ_BATCH", "members")
    mem, gs, twins = _batch_mirrors(capi, bid)
    try:
        want_n = [n for _, _, n in mem]
        wxs, wus = [c["w"][0] for c, _, _ in mem], [c["w"][1] for c, _, _ in mem]
        outs = capi.mpc_adjoint_batch(gs, wxs, wus, **RC.DEFAULT)          # no factor is stored: the call builds every member's
        assert [o["n_reg"] for o in outs] == want_n, f"{bid}: n_reg per member"
        for m, ((c, x0, _), g, t) in enumerate(zip(mem, gs, twins)):
            one = _adj(t, c["w"], RC.DEFAULT)
            got = dict(outs[m], **g.mpc_adjoint_grads())
            assert got["n_reg"] == one["n_reg"]
            for what in GRADS:
                _same_bits(got[what], one[what], f"{bid}[{m}]: {what}, batch against the single call")
            sol = g.solution()
            ref = AR.dual_form(SN.problem_at(c, x0), sol["x"], sol["u"], c["param"], c["w"], c["kinds"], **RC.DEFAULT)
            assert ref["n_reg"] == got["n_reg"]
            _within(f"{bid}[{m}]", got, ref, GRADS, _member_tol(bid, m), "(b)")
        again = capi.mpc_adjoint_batch(gs, wxs, wus, **RC.DEFAULT)          # the factors are stored now: the counts are theirs
        assert [o["n_reg"] for o in again] == want_n, "the second call on the same mirrors"
        for m in range(len(mem)):
            _same_bits(again[m]["gx0"], outs[m]["gx0"], f"{bid}[{m}]: gx0 of the second call")
    finally:
        _close(gs + twins)

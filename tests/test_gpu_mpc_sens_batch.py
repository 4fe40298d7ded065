"""The sensitivities and the predictor of a batch of MPC steps in one set of launches (tqgpu_mpc_sensitivity_batch, tqgpu_mpc_predict_batch)
against tqgpu_mpc_sensitivity and tqgpu_mpc_predict on twin mirrors stepped the same way, bit for bit (np.uint64 views, no tolerance: the
reference is the existing single kernels), and for `mixed` also against sens_ref.dense_kkt at the device's own point within the tolerance
the single-call tests apply to the case (sens_cases.tol, mpc_limit_cases.tol), so that the test does not rest on the device alone.

Batches: adj_batch_cases.py.  The twins' results are computed once per batch and shared.  Launches, copies and waits are tqgpu_mpc_stats',
compared with the formula of include/treeqp_amd.h."""
import ctypes as C

import numpy as np
import pytest

import adj_batch_cases as AB
import adj_cases as AC
import mpc_cases as MC
import mpc_limit_cases as ML
import sens_cases as SN
import sens_ref as SR

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
SCALES = (2.0 ** 10, 2.0 ** 20)          # of a case's dx: inside the box, and the one of the limit cases that clips
SENS = ("K", "u0", "x0_ref", "dx", "du", "dlam")
SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u", "dlam")
_TWINS = {}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


def _close(gs):
    for g in gs:
        g.close()


def _make(capi, bid, upto=None):
    gs = []
    try:
        for c in AB.members(bid)[:upto]:
            gs.append(SN.make(capi, c))
    except Exception:
        _close(gs)
        raise
    return gs


def _step(capi, gs, x0s, first=False, **kw):
    """first: the mirrors have not solved yet, and the step is made twice.  A mirror's first solve leaves its one-time set-up (the kernels
    behind an upload) marked pending on the streams of members that solve on streams of their own, and the first batched call behind it
    waits for those streams once each, as tqgpu_mpc_adjoint_batch does; the second step is the steady state of a loop, which the counts
    of include/treeqp_amd.h describe.  Twins are stepped through the same helper."""
    for _ in range(2 if first else 1):
        res, u0s = capi.mpc_step_batch(gs, x0s, **kw)
        assert all(r["status"] == 0 for r in res)
    return res, u0s


def _x1s(bid, scale, upto=None):
    """the members' next x0: the one they were stepped from plus the case's dx, scaled"""
    return [x0 + c["dx"] * scale for x0, c in zip(AB.x0s(bid)[:upto], AB.members(bid)[:upto])]


def _stored(g):
    """what the getters of a member return"""
    K, u0, x0r = g.mpc_gain()
    return dict(K=K, u0=u0, x0_ref=x0r, **g.mpc_sensitivities())


def _nh(bid, upto=None):
    return [ML.parent_levels(c["d"]["nk"]) for c in AB.members(bid)[:upto]]


def _sens_launches(nh, packed=False):
    """the header's formula: [the packing] + (1 + Nh_max) + (Nh_max - 1) + 1"""
    return (0 if packed else 1) + (1 + nh) + (nh - 1) + 1


def _twins(capi, bid):
    """per member n_reg, K, u0, x0_ref, dx, du, dlam of tqgpu_mpc_sensitivity and (u0_pred, n_clipped) of tqgpu_mpc_predict at both scales, on a
    twin mirror stepped the same way; computed once"""
    if bid not in _TWINS:
        gs = _make(capi, bid)
        try:
            _step(capi, gs, AB.x0s(bid), first=True)
            out = []
            for m, g in enumerate(gs):
                one = dict(n_reg=g.mpc_sensitivity())
                one.update(_stored(g))
                one["pred"] = {scale: g.mpc_predict(_x1s(bid, scale)[m]) for scale in SCALES}
                out.append(one)
            _TWINS[bid] = out
        finally:
            _close(gs)
    return _TWINS[bid]


def _check_members(capi, bid, gs, n_regs, why):
    ref = _twins(capi, bid)
    for m, g in enumerate(gs):
        cid = AB.BATCHES[bid][m]
        assert n_regs[m] == ref[m]["n_reg"], (cid, why)
        got = _stored(g)
        for what in SENS:
            _same_bits(got[what], ref[m][what], f"{bid}[{m}] {cid}: {what}, {why}")


def _tol(cid, what):
    return SN.tol(cid, what) if cid in AC.SENS_IDS else ML.tol(cid, what)


# 1., 2.
@pytest.mark.parametrize("bid", AB.BATCH_IDS)
def test_each_member_is_its_single_call(capi, bid):
    gs = _make(capi, bid)
    try:
        _step(capi, gs, AB.x0s(bid), first=True)
        n_regs = capi.mpc_sensitivity_batch(gs)
        got = _counts(capi)
        print(f"{bid}: (launches, copies, waits) = {got}")
        assert got == (_sens_launches(max(_nh(bid))), 2, 1)
        _check_members(capi, bid, gs, n_regs, "batch against twins")
        if bid == "mixed":
            for m, g in enumerate(gs):
                c, cid = AB.members(bid)[m], AB.BATCHES[bid][m]
                sol = g.solution()
                ref = SR.dense_kkt(c["d"], sol["x"], sol["u"], c["param"], c["kinds"])
                assert ref["residual"] < 1e-9 * ref["scale"]
                mine = _stored(g)
                for what in ("K", "dx", "du") + (("dlam",) if n_regs[m] == 0 else ()):
                    assert mine[what].shape == ref[what].shape, what
                    err = float(np.max(np.abs(mine[what] - ref[what]))) if ref[what].size else 0.0
                    print(f"{cid} {what}: |device - (a)| = {err:.3e}, tolerance {_tol(cid, what):.3e}, n_reg {n_regs[m]}")
                    assert err <= _tol(cid, what), (cid, what, err)
    finally:
        _close(gs)


# 3.
def test_counts_do_not_grow_with_n(capi):
    bid = "same4"
    seen = {}
    for n in (2, 3, 4):
        gs = _make(capi, bid, n)
        try:
            _step(capi, gs, AB.x0s(bid)[:n], first=True)
            n_regs = capi.mpc_sensitivity_batch(gs)
            sens = _counts(capi)
            capi.mpc_predict_batch(gs, _x1s(bid, SCALES[0], n))
            seen[n] = (sens, _counts(capi))
            print(f"{bid}, {n} members: sensitivity (launches, copies, waits) {sens}, predictor {seen[n][1]}")
            _check_members(capi, bid, gs, n_regs, f"the first {n} members")
        finally:
            _close(gs)
    nh = max(_nh(bid))
    for n, (sens, pred) in seen.items():
        assert sens == (_sens_launches(nh), 2, 1) and pred == (1, 1, 1), n


# 4.
def test_member_by_member_on_request(capi, monkeypatch):
    bid = "same4"
    gs = _make(capi, bid)
    monkeypatch.setenv("TREEQP_AMD_SENS_BATCH", "members")          # read by every call
    try:
        _step(capi, gs, AB.x0s(bid), first=True)
        n_regs = capi.mpc_sensitivity_batch(gs)
        assert _counts(capi) == (sum(_sens_launches(h) for h in _nh(bid)), len(gs), len(gs)), "the sum of the single calls"
        _check_members(capi, bid, gs, n_regs, "TREEQP_AMD_SENS_BATCH=members")
        ref = _twins(capi, bid)
        for scale in SCALES:
            us, ncs = capi.mpc_predict_batch(gs, _x1s(bid, scale))
            assert _counts(capi) == (len(gs), 0, len(gs)), "the sum of the single calls"
            for m in range(len(gs)):
                _same_bits(us[m], ref[m]["pred"][scale][0], f"{bid}[{m}] scale {scale}: u0_pred, member by member")
                assert ncs[m] == ref[m]["pred"][scale][1]
    finally:
        _close(gs)


def test_a_batch_of_one_takes_the_single_route(capi):
    bid = "pair"
    gs = _make(capi, bid)
    try:
        _step(capi, gs, AB.x0s(bid), first=True)
        ref = _twins(capi, bid)
        for m, g in enumerate(gs):
            n_regs = capi.mpc_sensitivity_batch([g])
            assert _counts(capi) == (_sens_launches(_nh(bid)[m]), 1, 1), "tqgpu_mpc_sensitivity's counts: one copy"
            assert n_regs == [ref[m]["n_reg"]]
            got = _stored(g)
            for what in SENS:
                _same_bits(got[what], ref[m][what], f"{bid}[{m}]: {what}, a batch of one")
            us, ncs = capi.mpc_predict_batch([g], [_x1s(bid, SCALES[1])[m]])
            assert _counts(capi) == (1, 0, 1), "tqgpu_mpc_predict's counts: no copy"
            _same_bits(us[0], ref[m]["pred"][SCALES[1]][0], f"{bid}[{m}]: u0_pred, a batch of one")
            assert ncs[0] == ref[m]["pred"][SCALES[1]][1]
    finally:
        _close(gs)


# 5.
@pytest.mark.parametrize("bid", AB.BATCH_IDS)
def test_the_state_is_the_single_call_s(capi, bid):
    nw = 1
    gs, twins = _make(capi, bid), _make(capi, bid)
    try:
        wxs, wus = AB.ws(bid, nw)
        _step(capi, gs, AB.x0s(bid), first=True)
        _step(capi, twins, AB.x0s(bid), first=True)
        capi.mpc_sensitivity_batch(gs)
        # the head hand-off: a single tqgpu_mpc_predict of a member reads the member's own device head
        for m, (g, t) in enumerate(zip(gs, twins)):
            t.mpc_sensitivity()
            for scale in SCALES:
                x1 = _x1s(bid, scale)[m]
                got, want = g.mpc_predict(x1), t.mpc_predict(x1)
                _same_bits(got[0], want[0], f"{bid}[{m}] scale {scale}: a single predict behind the batched sensitivity")
                assert got[1] == want[1]
        # the factor counts as stored
        nh = max(_nh(bid))
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)
        assert _counts(capi)[0] == 2 * nh + 1, "no packing and no factor launches"
        for m, (g, t) in enumerate(zip(gs, twins)):
            want = t.mpc_adjoint(wxs[m], wus[m])
            want.update(t.mpc_adjoint_grads())
            got = dict(outs[m], **g.mpc_adjoint_grads())
            assert got["n_reg"] == want["n_reg"]
            for what in ("gx0", "gq", "gr", "gb"):
                _same_bits(got[what], want[what], f"{bid}[{m}]: {what} of the adjoint behind the batched sensitivity")
    finally:
        _close(gs + twins)


def test_solution_and_kkt_are_left_alone(capi):
    bid = "mixed"
    gs = _make(capi, bid)
    try:
        _step(capi, gs, AB.x0s(bid), first=True)
        before = [(g.solution(), g.kkt_residual()) for g in gs]
        capi.mpc_sensitivity_batch(gs)
        capi.mpc_predict_batch(gs, _x1s(bid, SCALES[1]), duals=False)
        for m, (g, (sol0, kkt0)) in enumerate(zip(gs, before)):
            sol = g.solution()
            for k in SOL_KEYS:
                _same_bits(sol[k], sol0[k], f"{bid}[{m}]: {k} behind the two batch calls")
            _same_bits(g.kkt_residual()["res"], kkt0["res"], f"{bid}[{m}]: the KKT residual behind the two batch calls")
    finally:
        _close(gs)


# 6.
@pytest.mark.parametrize("bid", AB.BATCH_IDS)
def test_the_predictor_is_the_single_call_s(capi, bid):
    gs = _make(capi, bid)
    try:
        _step(capi, gs, AB.x0s(bid), first=True)
        capi.mpc_sensitivity_batch(gs)
        ref = _twins(capi, bid)
        clipped = 0
        for scale in SCALES:
            us, ncs = capi.mpc_predict_batch(gs, _x1s(bid, scale))
            got = _counts(capi)
            print(f"{bid} scale {scale}: (launches, copies, waits) = {got}, n_clipped {ncs}")
            assert got[0] == 1 and got[1] <= 1 and got[2] == 1
            for m in range(len(gs)):
                _same_bits(us[m], ref[m]["pred"][scale][0], f"{bid}[{m}] scale {scale}: u0_pred")
                assert ncs[m] == ref[m]["pred"][scale][1], (bid, m, scale)
            clipped = sum(ncs)
        if bid == "mixed":
            assert clipped > 0, "the clipping branch was not reached"
    finally:
        _close(gs)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bid", AB.BATCH_IDS)
def test_predicted_duals_start_one_solve(capi, bid, mode):
    x0s, x1s = AB.x0s(bid), _x1s(bid, SCALES[0])
    legs = {}
    for leg in ("batch", "single"):
        gs = _make(capi, bid)
        try:
            for g in gs:
                g.set_lambda(0.125 * np.ones(g.sum_lam))
                g.set_warm_start(mode)
            _step(capi, gs, x0s, first=True)
            if leg == "batch":
                capi.mpc_sensitivity_batch(gs)
                capi.mpc_predict_batch(gs, x1s, duals=True)
                got = _counts(capi)
                assert got[0] == 1 and got[1] <= 1 and got[2] == 1, got
            else:
                for g, x1 in zip(gs, x1s):
                    g.mpc_sensitivity()
                    g.mpc_predict(x1, duals=True)
            nxt = _step(capi, gs, x1s)                                    # starts from the predicted duals
            after = capi.mpc_step_batch(gs, x1s, maxIter=1)               # starts as the mode says
            legs[leg] = (nxt, after)
        finally:
            _close(gs)
    for which, name in ((0, "the next step"), (1, "the step after it")):
        (rb, ub), (rs, us) = legs["batch"][which], legs["single"][which]
        for m in range(len(ub)):
            assert (rb[m]["iter"], rb[m]["ls_total"]) == (rs[m]["iter"], rs[m]["ls_total"]), (bid, m, name)
            assert rb[m]["last_error_norm"] == rs[m]["last_error_norm"], (bid, m, name)
            _same_bits(ub[m], us[m], f"{bid}[{m}] mode {mode}: u0 of {name}")
    if mode == 0:
        # the caller's buffer is back: the step after next starts as a fresh mirror does from that buffer
        fresh = _make(capi, bid)
        try:
            for g in fresh:
                g.set_lambda(0.125 * np.ones(g.sum_lam))
            rf, _ = capi.mpc_step_batch(fresh, x1s, maxIter=1)
            for m in range(len(fresh)):
                assert legs["batch"][1][0][m]["last_error_norm"] == rf[m]["last_error_norm"], (bid, m)
        finally:
            _close(fresh)


# 7.
def test_refusals_touch_no_member(capi):
    bid, nw = "pair", 1
    L = capi.lib()
    o = capi._gpu_opts(0)
    gs, twins = _make(capi, bid), _make(capi, bid)
    extra = []
    dp = C.POINTER(C.c_double)
    try:
        for v in (gs, twins):
            _step(capi, v, AB.x0s(bid), first=True)
            capi.mpc_sensitivity_batch(v)
        capi.mpc_adjoint_batch(gs, *AB.ws(bid, nw))

        def stored(g):
            out = _stored(g)
            out.update(g.mpc_adjoint_grads())
            gx0 = np.zeros(max(int(g.nx0) * nw, 1))
            assert L.tqgpu_mpc_get_adjoint_x0(g.h, gx0.ctypes.data_as(dp)) == 0
            out["gx0"] = gx0
            return out

        before = [stored(g) for g in gs]

        def call(mirrors, n=None, opts=o):
            arr = (C.c_void_p * max(len(mirrors), 1))(*[g.h for g in mirrors])
            return L.tqgpu_mpc_sensitivity_batch(arr, len(mirrors) if n is None else n, None if opts is None else C.byref(opts), None)

        def untouched(why):
            for m, g in enumerate(gs):
                now = stored(g)
                for what in before[m]:
                    _same_bits(now[what], before[m][what], f"{bid}[{m}]: {what} after a refusal ({why})")

        b2 = MC.case("dense_kind2_root")
        k2 = MC.make(capi, b2)
        extra.append(k2)
        k2.mpc_step(MC.exact_x0s(b2["nx0"], 0)[0], **b2["opts"])
        assert call([k2] + gs) == EUNSUPPORTED and b"member 0" in L.tqgpu_last_error() and b"kind 2 or 3" in L.tqgpu_last_error()
        untouched("a kind-2 member")
        c = AC.case("elim-one_child")
        fresh = SN.make(capi, c)
        extra.append(fresh)
        assert call(gs + [fresh]) == EINVAL and b"member 2" in L.tqgpu_last_error() and b"has not solved yet" in L.tqgpu_last_error()
        untouched("a member that has not solved")
        fresh.mpc_step(c["x0"])
        fresh.mpc_set_x0(c["x0"])          # a fold behind the last solve
        assert call(gs + [fresh]) == EINVAL and b"member 2" in L.tqgpu_last_error() and b"since the last solve" in L.tqgpu_last_error()
        untouched("a member folded after its last solve")
        assert call(gs + [gs[0]]) == EINVAL and b"named twice" in L.tqgpu_last_error()
        untouched("a mirror named twice")
        assert call(gs, n=0) == EINVAL
        assert call(gs, opts=None) == EINVAL
        untouched("n = 0, opts = NULL")

        # the predictor: a member without a sensitivity; no start buffer is changed, so the next step is that of twins that were not asked
        x1s = _x1s(bid, SCALES[0])
        arr = (C.c_void_p * 3)(*[g.h for g in gs + [fresh]])
        x = np.concatenate(x1s + [np.asarray(c["x0"], dtype=np.float64)])
        u = np.full(sum(int(g.nu[0]) for g in gs + [fresh]), 7.0)
        assert L.tqgpu_mpc_predict_batch(arr, 3, x.ctypes.data_as(dp), u.ctypes.data_as(dp), 1, None) == EINVAL
        assert b"member 2" in L.tqgpu_last_error() and b"no sensitivity" in L.tqgpu_last_error()
        assert np.all(u == 7.0)
        untouched("a predictor with a member that lacks its sensitivity")
        (rb, ub), (rt, ut) = capi.mpc_step_batch(gs, x1s), capi.mpc_step_batch(twins, x1s)
        for m in range(len(gs)):
            assert (rb[m]["iter"], rb[m]["ls_total"], rb[m]["last_error_norm"]) == (rt[m]["iter"], rt[m]["ls_total"], rt[m]["last_error_norm"]), m
            _same_bits(ub[m], ut[m], f"{bid}[{m}]: u0 of the step behind the refused predictor")
    finally:
        _close(gs + twins + extra)

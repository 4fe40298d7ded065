"""The adjoint of a batch of MPC steps in one set of launches (tqgpu_mpc_adjoint_batch) against tqgpu_mpc_adjoint on twin mirrors stepped
the same way, bit for bit (np.uint64 views, no tolerance: the reference is the existing single kernels), and for `mixed` at nw = 1 also
against adj_ref.dual_form at the device's own point within adj_cases.tol, so that the test does not rest on the device alone.

Batches: adj_batch_cases.py.  The twins' results are computed once per (batch, nw) and shared.  Launches, copies and waits are
tqgpu_mpc_stats', compared with the formula of include/treeqp_amd.h."""
import ctypes as C
import os

import numpy as np
import pytest

import adj_batch_cases as AB
import adj_cases as AC
import adj_ref as AR
import mpc_cases as MC
import mpc_limit_cases as ML
import sens_cases as SN

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
GRADS = ("gq", "gr", "gb")
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


def _step(capi, gs, bid):
    res, _ = capi.mpc_step_batch(gs, AB.x0s(bid)[:len(gs)])
    assert all(r["status"] == 0 for r in res)


def _stored(capi, g, nw):
    """what the getters of a member return: gq, gr, gb and gx0"""
    out = g.mpc_adjoint_grads()
    gx0 = np.zeros(max(int(g.nx0) * nw, 1))
    assert capi.lib().tqgpu_mpc_get_adjoint_x0(g.h, gx0.ctypes.data_as(C.POINTER(C.c_double))) == 0
    out["gx0"] = gx0[:int(g.nx0) * nw].reshape((int(g.nx0), nw), order="F")
    return out


def _twins(capi, bid, nw):
    """per member gq, gr, gb, gx0, n_reg of tqgpu_mpc_adjoint on a twin mirror stepped the same way; computed once"""
    if (bid, nw) not in _TWINS:
        gs = _make(capi, bid)
        try:
            _step(capi, gs, bid)
            wxs, wus = AB.ws(bid, nw)
            out = []
            for g, wx, wu in zip(gs, wxs, wus):
                one = g.mpc_adjoint(wx, wu)
                one.update(g.mpc_adjoint_grads())
                out.append(one)
            _TWINS[(bid, nw)] = out
        finally:
            _close(gs)
    return _TWINS[(bid, nw)]


def _check_members(capi, bid, nw, gs, outs, why):
    ref = _twins(capi, bid, nw)
    for m, (g, got) in enumerate(zip(gs, outs)):
        cid = AB.BATCHES[bid][m]
        stored = _stored(capi, g, nw)
        assert got["n_reg"] == ref[m]["n_reg"], (cid, why)
        _same_bits(got["gx0"], ref[m]["gx0"], f"{bid}[{m}] {cid}: gx0 returned, {why}")
        for what in GRADS + ("gx0",):
            _same_bits(stored[what], ref[m][what], f"{bid}[{m}] {cid}: {what}, {why}")


def _nh(bid, upto=None):
    return [ML.parent_levels(c["d"]["nk"]) for c in AB.members(bid)[:upto]]


@pytest.mark.parametrize("nw", AB.NWS)
@pytest.mark.parametrize("bid", AB.BATCH_IDS)
def test_each_member_is_its_single_call(capi, bid, nw):
    gs = _make(capi, bid)
    try:
        _step(capi, gs, bid)
        wxs, wus = AB.ws(bid, nw)
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)
        nh = max(_nh(bid))
        assert _counts(capi)[0] == 1 + (1 + nh) + (2 * nh + 1)          # the packing, the factor, the adjoint
        _check_members(capi, bid, nw, gs, outs, "batch against twins")
        if bid == "mixed" and nw == 1:
            for m, (g, got) in enumerate(zip(gs, outs)):
                c = AB.members(bid)[m]
                cid = AB.BATCHES[bid][m]
                sol = g.solution()
                ref = AR.dual_form(c["d"], sol["x"], sol["u"], c["param"], (wxs[m], wus[m]), c["kinds"])
                assert ref["n_reg"] == 0 and ref["in_range"] < 1e-10
                got = dict(got, **g.mpc_adjoint_grads())
                for what in ("gq", "gr", "gx0") + (("gb",) if got["n_reg"] == 0 else ()):
                    assert got[what].shape == ref[what].shape, what
                    err = float(np.max(np.abs(got[what] - ref[what]))) if ref[what].size else 0.0
                    print(f"{cid} {what}: |device - (b)| = {err:.3e}, tolerance {AC.tol(cid, what):.3e}, n_reg {got['n_reg']}")
                    assert err <= AC.tol(cid, what), (cid, what, err)
    finally:
        _close(gs)


def test_mixed_factor_states(capi):
    bid, nw = "mixed", 1
    gs = _make(capi, bid)
    try:
        _step(capi, gs, bid)
        for g in gs[::2]:
            g.mpc_sensitivity()
        gains = [g.mpc_gain() for g in gs[::2]]
        wxs, wus = AB.ws(bid, nw)
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)
        nh = _nh(bid)
        # the members that lack the factor pack and build theirs; waits: members of a mixed batch may hold work on streams of their own
        assert _counts(capi)[:2] == (1 + (1 + max(nh[1::2])) + (2 * max(nh) + 1), 3)
        _check_members(capi, bid, nw, gs, outs, "every second factor stored")
        for g, before in zip(gs[::2], gains):
            after = g.mpc_gain()
            for i in range(3):
                _same_bits(after[i], before[i], f"mpc_gain[{i}] behind the batch call")
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)          # every factor is stored now
        assert _counts(capi) == (2 * max(nh) + 1, 3, 1)          # (the first call has drained every member's own stream)
        _check_members(capi, bid, nw, gs, outs, "all factors stored")
    finally:
        _close(gs)


@pytest.mark.parametrize("n", [4, 2])
def test_counts_do_not_grow_with_n(capi, n):
    bid, nw = "same4", 1
    gs = _make(capi, bid, n)
    try:
        wxs, wus = [v[:n] for v in AB.ws(bid, nw)]
        nh = max(_nh(bid, n))
        for it in range(3):
            _step(capi, gs, bid)
            outs = capi.mpc_adjoint_batch(gs, wxs, wus)
            built = _counts(capi)
        assert built == (1 + (1 + nh) + (2 * nh + 1), 3, 1), "the steady state behind mpc_step_batch, factors built"
        _check_members(capi, bid, nw, gs, outs, f"the first {n} members, third iteration")
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)
        assert _counts(capi) == (2 * nh + 1, 3, 1), "factors stored"
        _check_members(capi, bid, nw, gs, outs, f"the first {n} members, factors stored")
    finally:
        _close(gs)


# (launches, copies, waits, batched members) of the KKT batch and the waits of the adjoint batch, in both iterations: the figures of the commit
# before the stream rule became one function (order_behind_lead), measured with that commit's library on the sequence of the test below
WAITS_BEHIND_STEP_AND_KKT = {
    "same4": ((3, 2, 1, 2), 1),          # one batch launch on the lead's stream: both calls wait for their results alone
    "pair": ((3, 2, 2, 2), 1),
}


@pytest.mark.parametrize("bid", sorted(WAITS_BEHIND_STEP_AND_KKT))
def test_waits_behind_a_batch_step_and_a_kkt_batch(capi, bid):
    """Two members of one device (two C1 trees; the smallest pair of adj_batch_cases, whose members solve on streams of their own):
    tqgpu_mpc_step_batch, then tqgpu_kkt_residual_batch, then tqgpu_mpc_adjoint_batch.  Both batched calls order their members behind the
    lead's stream by one rule whose switches differ: only the adjoint takes a batch step to have drained every stream."""
    nw = 1
    gs = _make(capi, bid, 2)
    try:
        wxs, wus = [v[:2] for v in AB.ws(bid, nw)]
        nh = max(_nh(bid, 2))
        seen = []
        for it in range(2):
            _step(capi, gs, bid)
            capi.kkt_residual_batch(gs)
            kkt = capi.kkt_batch_stats()
            outs = capi.mpc_adjoint_batch(gs, wxs, wus)
            seen.append(((kkt["launches"], kkt["copies"], kkt["waits"], kkt["batched_members"]), _counts(capi)))
            print(f"{bid}, iteration {it}: kkt batch (launches, copies, waits, batched members) {seen[-1][0]}, adjoint batch (launches, copies, waits) {seen[-1][1]}")
        kkt_ref, adj_waits = WAITS_BEHIND_STEP_AND_KKT[bid]
        for it, (kkt, adj) in enumerate(seen):
            assert kkt == kkt_ref, (bid, it)
            assert adj == (1 + (1 + nh) + (2 * nh + 1), 3, adj_waits), (bid, it)          # the KKT batch packs the points, Export::valid stays: packed again
        _check_members(capi, bid, nw, gs, outs, "behind a batch step and a KKT batch")
    finally:
        _close(gs)


def test_member_by_member_on_request(capi):
    bid, nw = "same4", 1
    gs = _make(capi, bid)
    old = os.environ.get("TREEQP_AMD_ADJ_BATCH")
    os.environ["TREEQP_AMD_ADJ_BATCH"] = "members"          # read by every call
    try:
        _step(capi, gs, bid)
        wxs, wus = AB.ws(bid, nw)
        outs = capi.mpc_adjoint_batch(gs, wxs, wus)
        nh = _nh(bid)
        assert _counts(capi) == (sum(3 * h + 2 + 1 for h in nh), 2 * len(gs), len(gs)), "the sum of the single calls"
        _check_members(capi, bid, nw, gs, outs, "TREEQP_AMD_ADJ_BATCH=members")
    finally:
        if old is None:
            del os.environ["TREEQP_AMD_ADJ_BATCH"]
        else:
            os.environ["TREEQP_AMD_ADJ_BATCH"] = old
        _close(gs)


def test_solution_and_kkt_are_left_alone(capi):
    bid, nw = "mixed", 3
    gs = _make(capi, bid)
    try:
        _step(capi, gs, bid)
        before = [(g.solution(), g.kkt_residual()) for g in gs]
        capi.mpc_adjoint_batch(gs, *AB.ws(bid, nw))
        for m, (g, (sol0, kkt0)) in enumerate(zip(gs, before)):
            sol = g.solution()
            for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
                _same_bits(sol[k], sol0[k], f"{bid}[{m}]: {k} behind the batch call")
            _same_bits(g.kkt_residual()["res"], kkt0["res"], f"{bid}[{m}]: the KKT residual behind the batch call")
    finally:
        _close(gs)


def test_a_new_step_invalidates_every_member(capi):
    bid = "pair"
    gs = _make(capi, bid)
    L = capi.lib()
    try:
        _step(capi, gs, bid)
        capi.mpc_adjoint_batch(gs, *AB.ws(bid, 1))
        for g in gs:
            assert (L.tqgpu_mpc_get_adjoint_x0(g.h, None), L.tqgpu_mpc_get_adjoint(g.h, None, None, None)) == (0, 0)
        _step(capi, gs, bid)
        for g in gs:
            assert (L.tqgpu_mpc_get_adjoint_x0(g.h, None), L.tqgpu_mpc_get_adjoint(g.h, None, None, None)) == (EINVAL, EINVAL)
    finally:
        _close(gs)


def test_refusals_touch_no_member(capi):
    bid, nw = "pair", 1
    L = capi.lib()
    o = capi._gpu_opts(0)
    gs = _make(capi, bid)
    extra = []
    try:
        _step(capi, gs, bid)
        capi.mpc_adjoint_batch(gs, *AB.ws(bid, nw))
        before = [_stored(capi, g, nw) for g in gs]

        def call(mirrors, n=None, nw_=1, opts=o):
            arr = (C.c_void_p * max(len(mirrors), 1))(*[g.h for g in mirrors])
            return L.tqgpu_mpc_adjoint_batch(arr, len(mirrors) if n is None else n, None if opts is None else C.byref(opts), None, None, nw_, None, None)

        def untouched(why):
            for m, g in enumerate(gs):
                now = _stored(capi, g, nw)
                for what in GRADS + ("gx0",):
                    _same_bits(now[what], before[m][what], f"{bid}[{m}]: {what} after a refusal ({why})")

        c = AC.case("elim-one_child")
        fresh = SN.make(capi, c)
        extra.append(fresh)
        assert call(gs + [fresh]) == EINVAL and b"member 2" in L.tqgpu_last_error() and b"has not solved yet" in L.tqgpu_last_error()
        untouched("a member that has not solved")
        fresh.mpc_step(c["x0"])
        fresh.set_linear_terms(c["d"]["q"], None)          # an upload
        assert call(gs + [fresh]) == EINVAL and b"member 2" in L.tqgpu_last_error() and b"since the last solve" in L.tqgpu_last_error()
        untouched("a member whose problem changed")
        b2 = MC.case("dense_kind2_root")
        k2 = MC.make(capi, b2)
        extra.append(k2)
        k2.mpc_step(MC.exact_x0s(b2["nx0"], 0)[0], **b2["opts"])
        assert call([k2] + gs) == EUNSUPPORTED and b"member 0" in L.tqgpu_last_error() and b"kind 2 or 3" in L.tqgpu_last_error()
        untouched("a kind-2 member")
        assert call(gs + [gs[0]]) == EINVAL and b"named twice" in L.tqgpu_last_error()
        untouched("a mirror named twice")
        assert call(gs, n=0) == EINVAL
        untouched("n = 0")
        assert call(gs, nw_=0) == EINVAL and b"nw" in L.tqgpu_last_error()
        untouched("nw = 0")
        assert call(gs, opts=None) == EINVAL
        untouched("opts = NULL")
        cw = ML.case(AC.WINDOW_ID)
        win = SN.make(capi, cw)
        extra.append(win)
        win.mpc_step(cw["x0"])
        assert call(gs + [win], nw_=AC.WINDOW_NW) == EUNSUPPORTED and b"member 2" in L.tqgpu_last_error() and b"160 KiB" in L.tqgpu_last_error()
        untouched("a window that does not fit")
    finally:
        _close(gs + extra)

"""MPC steps on trees whose root keeps its states (tqgpu_mpc_set_root_states) and the certified step (tqgpu_mpc_set_certify), against the
host loop the parent commit offers: tqgpu_set_warm_start(1) once, then per step tqgpu_set_problem (the setter of the bounds on a dense tree)
with the root's xmin / xmax replaced by x0, tqgpu_solve, tqgpu_get_solution, on a twin mirror.  The fold has no arithmetic: every
comparison is exact, on general, unquantised data.  One tree per route (mpc_root_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import mpc_cases as M
import mpc_root_cases as R
import solve_sequence_cases as SC

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")
COUNTS = ("status", "iter", "ls_total")
STEADY = dict(launches=3, copies=0, waits=1)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _sol_keys(c):
    return SOL_KEYS + (("mu_d",) if "nc" in c["d"] else ())


def _same_step(c, what, rd, u0, sd, rh, sh):
    for k in COUNTS:
        assert rd[k] == rh[k], f"{what}: {k} {rd[k]} != {rh[k]}"
    if u0 is not None:
        _same_bits(u0, sh["u"][:int(c["d"]["nu"][0])], f"{what}: u0")
    for k in _sol_keys(c):
        _same_bits(sd[k], sh[k], f"{what}: {k}")


def _pair(capi, c):
    dev, host = R.make(capi, c, root_states=True), R.make(capi, c)
    dev.set_warm_start(1); host.set_warm_start(1)
    return dev, host


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the fold
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_fold_copies_x0_bit_for_bit(capi, cid):
    c = R.case(cid)
    dev, host = _pair(capi, c)
    try:
        lo, hi = dev.root_bounds()
        _same_bits(lo, c["x0"], f"{cid}: xmin[0] as uploaded"); _same_bits(hi, c["x0"], f"{cid}: xmax[0] as uploaded")
        for rep, x0 in enumerate(R.x0_sequence(c, 5)[:2]):          # before the first solve, and with the persistent route's constants packed
            x0[rep] = -0.0
            x0[2] = 5e-324          # the smallest subnormal (every root here has three states or more)
            dev.mpc_set_x0(x0)
            lo, hi = dev.root_bounds()
            _same_bits(lo, x0, f"{cid}: xmin[0]"); _same_bits(hi, x0, f"{cid}: xmax[0]")
            assert np.signbit(lo[rep]) and lo[rep] == 0.0 and lo[2] == 5e-324
            # the other nodes' bounds are untouched: the solve is the twin's
            rd, u0 = dev.mpc_step(None, **c["opts"])
            rh, sh = R.host_step(capi, host, c, x0)
            _same_step(c, f"{cid} solve {rep}", rd, u0, dev.solution(), rh, sh)
    finally:
        dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_loop_bit_for_bit_the_host_loop(capi, cid):
    c = R.case(cid)
    xs = R.x0_sequence(c)
    xs = xs + [xs[0], xs[1], xs[0]]          # a, b, a again: a route that kept a copy of the root's bounds starts the last step from b's
    dev, host = _pair(capi, c)
    try:
        for step, x0 in enumerate(xs):
            rd, u0 = dev.mpc_step(x0, **c["opts"])
            st = capi.mpc_stats()
            sd = dev.solution()
            rh, sh = R.host_step(capi, host, c, x0)
            print(f"{cid} step {step}: device {[rd[k] for k in COUNTS]} host {[rh[k] for k in COUNTS]} launches {rd['n_launches']} stats {st}")
            _same_step(c, f"{cid} step {step}", rd, u0, sd, rh, sh)
            if cid == "persist_c1" and step >= 2:
                # the fold wrote the packed constants itself: no re-pack, nothing copied, one wait
                assert st == STEADY, f"{cid} step {step}: {st}"
    finally:
        dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a re-pack that is pending for another reason
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["persist_c1", "single_wg", "dense_kind2_root"])
def test_bounds_of_another_node_between_two_steps(capi, cid):
    c = R.case(cid)
    xs = R.x0_sequence(c, 1)
    dev, host = _pair(capi, c)
    try:
        for step in range(2):
            rd, u0 = dev.mpc_step(xs[step], **c["opts"])
            rh, sh = R.host_step(capi, host, c, xs[step])
            _same_step(c, f"{cid} step {step}", rd, u0, dev.solution(), rh, sh)
        d2 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
        nu0 = int(d2["nu"][0])
        d2["umax"][nu0:2 * nu0] *= 0.5          # node 1
        d2["umin"][nu0:2 * nu0] *= 0.25
        R.set_bounds(capi, dev, R.with_x0(c, xs[1], d2))          # (asks for a re-pack on the persistent route)
        for step in range(2, 5):
            rd, u0 = dev.mpc_step(xs[step], **c["opts"])
            st = capi.mpc_stats()
            rh, sh = R.host_step(capi, host, c, xs[step], d2)
            print(f"{cid} step {step}: device {[rd[k] for k in COUNTS]} stats {st}")
            _same_step(c, f"{cid} step {step}", rd, u0, dev.solution(), rh, sh)
        if cid == "persist_c1":
            assert st == STEADY, st
    finally:
        dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. leaving the loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["persist_c1", "single_wg"])
def test_set_problem_after_the_loop_uploads_again(capi, cid):
    c = R.case(cid)
    dev, fresh = R.make(capi, c, root_states=True), R.make(capi, c)
    try:
        # the mirror of tqgpu_set_problem holds the original problem ...
        R.host_upload(capi, dev, c, c["d"])
        dev.set_warm_start(1)
        for x0 in R.x0_sequence(c, 2)[:3]:
            dev.mpc_step(x0, **c["opts"])
        assert not np.array_equal(dev.root_bounds()[0], c["x0"])
        # ... and must not claim that the device still does
        R.host_upload(capi, dev, c, c["d"])
        _same_bits(dev.root_bounds()[0], c["x0"], "xmin[0] after tqgpu_set_problem")
        dev.set_warm_start(0)
        dev.set_lambda(None); fresh.set_lambda(None)
        rd, rf = dev.solve(**c["opts"]), fresh.solve(**c["opts"])
        _same_step(c, f"{cid}: after the loop", rd, None, dev.solution(), rf, fresh.solution())
    finally:
        dev.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the batch step
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch_run(capi, cs, makes, steps=4, between=None):
    """cs: the members' cases, makes: how a mirror of each is made; members in one batch step against twins that step alone;
    between(step, seqs, members, alone): called after every step"""
    n = len(cs)
    seqs = [R.x0_sequence(c, 10 + i, steps) if "x0" in c else M.exact_x0s(c["nx0"], i)[:steps] for i, c in enumerate(cs)]
    members, alone = [mk() for mk in makes], [mk() for mk in makes]
    stats = []
    try:
        for g in members + alone:
            g.set_warm_start(1)
        for step in range(steps):
            res, u0s = capi.mpc_step_batch(members, [seqs[i][step] for i in range(n)], **cs[0]["opts"])
            stats.append(capi.mpc_stats())
            for i in range(n):
                ra, ua = alone[i].mpc_step(seqs[i][step], **cs[0]["opts"])
                for k in COUNTS:
                    assert res[i][k] == ra[k], f"step {step} member {i}: {k}"
                _same_bits(u0s[i], ua, f"step {step} member {i}: u0")
                sm, sa = members[i].solution(), alone[i].solution()
                for k in SOL_KEYS:
                    _same_bits(sm[k], sa[k], f"step {step} member {i}: {k}")
            if between is not None:
                between(step, seqs, members, alone)
    finally:
        for g in members + alone:
            g.close()
    return stats


def test_batch_step_of_persistent_members(capi):
    c = R.case("persist_c1")
    stats = _batch_run(capi, [c] * 3, [lambda: R.make(capi, c, root_states=True)] * 3)
    print(f"batch step, 3 x C1: {stats}")
    # one launch ahead (the folds wrote the packed constants), the members' shared launch, the post; the descriptors; the wait for the tag
    assert stats[-1] == dict(launches=3, copies=1, waits=1), stats


def test_batch_step_with_a_repack_pending_on_members_that_do_not_lead(capi):
    """tqgpu_set_bounds on another node of the second and third member between two batch steps: their constants are packed again on their
    own streams, the folds run on the first member's -- the pack must find the folded root bounds (the same holds for every member's
    first step, where nothing is packed yet)"""
    c = R.case("persist_c1")
    nu0 = int(c["d"]["nu"][0])

    def between(step, seqs, members, alone):
        if step != 1:
            return
        for i in (1, 2):
            d2 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
            d2["umax"][nu0:2 * nu0] *= 0.5 / i          # node 1
            d2["umin"][nu0:2 * nu0] *= 0.25
            for g in (members[i], alone[i]):
                R.set_bounds(capi, g, R.with_x0(c, seqs[i][step], d2))

    stats = _batch_run(capi, [c] * 3, [lambda: R.make(capi, c, root_states=True)] * 3, steps=5, between=between)
    print(f"batch step, 3 x C1, bounds of two members changed after step 1: {stats}")
    # the step with the two packs: two launches more, and the wait for the first member's stream that orders the packs behind the folds
    assert stats[2]["launches"] == stats[1]["launches"] + 2 and stats[2]["waits"] >= 2, stats
    assert stats[-1] == dict(launches=3, copies=1, waits=1), stats


def test_batch_step_of_single_workgroup_members(capi):
    c = R.case("single_wg")
    stats = _batch_run(capi, [c] * 2, [lambda: R.make(capi, c, root_states=True)] * 2)
    print(f"batch step, 2 single-workgroup trees: {stats}")


def test_batch_step_mixes_both_forms_of_root(capi):
    ce, cr = M.case("single_wg"), R.case("single_wg")
    assert ce["nx0"] != cr["nx0"]          # the flat x0s array takes nx0 doubles per member, whichever form it has
    _batch_run(capi, [ce, cr], [lambda: M.make(capi, ce), lambda: R.make(capi, cr, root_states=True)])
    _batch_run(capi, [cr, ce], [lambda: R.make(capi, cr, root_states=True), lambda: M.make(capi, ce)])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the certified step
# ---------------------------------------------------------------------------------------------------------------------------------
def _same_kkt(a, b, what):
    _same_bits(a["res"], b["res"], f"{what}: values")
    assert np.array_equal(a["node"], b["node"]), f"{what}: nodes {a['node']} != {b['node']}"


def _certified_step(capi, c, cert, plain, x0, what, **extra):
    """one step on the certifying mirror and on its twin that does not certify; the certificate against tqgpu_kkt_residual of both"""
    opts = {**c["opts"], **extra}
    rp, up = plain.mpc_step(x0, **opts)
    kp, sp = plain.kkt_residual(), plain.solution()
    rc, uc = cert.mpc_step(x0, **opts)
    st = capi.mpc_stats()
    got = cert.mpc_certificate()
    print(f"{what}: {[rc[k] for k in COUNTS]} launches {rc['n_launches']} stats {st} certificate " +
          " ".join(f"{n} {v:.2e}" for n, v in zip(capi.KKT_CLASSES, got["res"])))
    _same_kkt(got, kp, f"{what}: certificate against the uncertified twin's tqgpu_kkt_residual")
    # the check afterwards packs nothing: its two kernels only
    kb = capi.kkt_residual_batch([cert])[0]
    assert capi.kkt_batch_stats()["launches"] == 2, capi.kkt_batch_stats()
    _same_kkt(got, kb, f"{what}: certificate against tqgpu_kkt_residual_batch afterwards")
    _same_kkt(got, cert.kkt_residual(), f"{what}: certificate against tqgpu_kkt_residual afterwards")
    _same_kkt(got, cert.mpc_certificate(), f"{what}: the certificate is host state")
    # the setting changes nothing of the step
    sc = cert.solution()
    _same_step(c, what, rc, uc, sc, rp, sp)
    _same_bits(uc, up, f"{what}: u0")
    _same_bits(sc["u"], cert.solution()["u"], f"{what}: a second download")
    return rc, st


@pytest.mark.parametrize("cid", ["persist_c1", "single_wg", "generic", "dense_kind3_root"])
def test_certified_step(capi, cid):
    c = R.case(cid)
    xs = R.x0_sequence(c, 3)
    cert, plain = R.make(capi, c, root_states=True), R.make(capi, c, root_states=True)
    try:
        cert.mpc_set_certify(True)
        # every solve from the same (zero) duals, stopped after 1, 2, 1 iterations in between: the dual buffer that is current flips
        # between consecutive solves, so a pack that trusted the host's copy of the last solve's control block would read the other one
        parity = []
        for step, extra in enumerate([{}, dict(maxIter=1), dict(maxIter=2), dict(maxIter=1), {}]):
            r, st = _certified_step(capi, c, cert, plain, xs[step], f"{cid} step {step}", **extra)
            parity.append(r["iter"] % 2)
            if c["path"] in (2, 3):
                # a single-launch route: one launch per solve once the mirror's first solve has initialised and packed ahead of its own,
                # and the header's formula: fold (+ warm start), the solve, the packing, the two KKT kernels, the post; the head's download; the tag
                assert step == 0 or r["n_launches"] == 1, f"{cid} step {step}: {r['n_launches']} launches"
                assert st == dict(launches=1 + r["n_launches"] + 1 + 2 + 1, copies=1, waits=1), st
        if c["path"] in (2, 3):          # (the routes on which the certificate goes out while the solve runs)
            assert parity[1:4] == [1, 0, 1], f"{cid}: the stopped solves did not take 1, 2, 1 iterations: {parity}"
        # in a warm-started loop
        cert.set_warm_start(1); plain.set_warm_start(1)
        for step in range(2):
            r, st = _certified_step(capi, c, cert, plain, xs[step], f"{cid} warm step {step}")
            if c["path"] in (2, 3):
                assert r["n_launches"] == 1 and st == dict(launches=1 + 1 + 1 + 2 + 1, copies=1, waits=1), (r, st)
        # switched off again: no certificate of that step
        cert.mpc_set_certify(False)
        cert.mpc_step(xs[2], **c["opts"])
        assert capi.lib().tqgpu_mpc_get_certificate(cert.h, None, None) == -2
    finally:
        cert.close(); plain.close()


def test_certified_step_with_a_long_line_search_inside_the_launch(capi):
    """the far start of solve_sequence_cases' multistage tree: 14 iterations and some 290 trials inside the one persistent launch, while
    the certificate's kernels and the post wait behind it.  (A launch that is NOT the whole solve cannot be had in a quick test: a
    persistent launch leaves its solve only when its 16-bit tag space is used up, after 60 000 sweeps, or on a timeout; what then
    happens -- everything behind the launch enqueued again behind the rest -- is the order of calls every launch-per-phase route takes
    at every step, which test_certified_step covers on the generic route and the dense tree.)"""
    c = R.case("mpersist")
    far = 5.0 * np.random.Generator(np.random.PCG64(11)).standard_normal(len(c["d"]["b"]))
    cert, plain = R.make(capi, c, root_states=True), R.make(capi, c, root_states=True)
    try:
        cert.mpc_set_certify(True)
        for step in range(2):          # the first solve of a mirror initialises and packs ahead of its launch
            cert.set_lambda(far); plain.set_lambda(far)
            r, st = _certified_step(capi, c, cert, plain, c["x0"], f"mpersist, far start, step {step}")
            assert r["status"] == 0 and r["ls_total"] > r["iter"], f"the far start no longer backtracks: {r}"
        assert r["n_launches"] == 1 and st == dict(launches=1 + 1 + 1 + 2 + 1, copies=1, waits=1), (r, st)
    finally:
        cert.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(capi, rc, code, text):
    assert rc == code, f"{rc} != {code}: {capi.lib().tqgpu_last_error().decode()}"
    assert text in capi.lib().tqgpu_last_error().decode(), capi.lib().tqgpu_last_error().decode()


def test_refusals(capi):
    L = capi.lib()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    o, res, u = capi._gpu_opts(), capi.GpuResult(), np.zeros(16)
    # an eliminated tree
    ce = M.case("one_child")
    g = M.make(capi, ce, root=False)
    try:
        launches0 = g.solve(**ce["opts"])["n_launches"]
        _refused(capi, L.tqgpu_mpc_set_root_states(g.h), -2, "tqgpu_mpc_set_root")
        assert g.solve(**ce["opts"])["n_launches"] == launches0
    finally:
        g.close()
    # a root of kind 1, at the call and, where the kinds changed afterwards, at the fold
    c = R.case("dense_kind2_root")
    g = R.make(capi, c)
    try:
        x = np.zeros(c["nx0"])
        steady = lambda: [g.solve(**c["opts"])["n_launches"] for _ in range(2)][1]          # (a first solve after an upload initialises)
        launches0 = steady()
        # before tqgpu_mpc_set_root_states: as before this entry point existed
        _refused(capi, L.tqgpu_mpc_set_x0(g.h, dp(x)), -2, "tqgpu_mpc_set_root")
        _refused(capi, L.tqgpu_mpc_step(g.h, dp(x), C.byref(o), C.byref(res), dp(u)), -2, "tqgpu_mpc_set_root")
        _refused(capi, L.tqgpu_mpc_get_certificate(g.h, dp(u), None), -2, "certified")
        assert g.solve(**c["opts"])["n_launches"] == launches0          # nothing was launched, nothing changed
        kinds1 = c["kinds"].copy()
        kinds1[0] = 1
        g.upload_mixed(c["d"], kinds1, None)
        _refused(capi, L.tqgpu_mpc_set_root_states(g.h), -2, "kind 1")
        g.upload_mixed(c["d"], c["kinds"], None)
        g.mpc_set_root_states()
        g.mpc_set_certify(True)
        _refused(capi, L.tqgpu_mpc_get_certificate(g.h, dp(u), None), -2, "certified")          # no step has run
        g.upload_mixed(c["d"], kinds1, None)
        launches1 = steady()
        _refused(capi, L.tqgpu_mpc_set_x0(g.h, dp(x)), -2, "kind 1")
        _refused(capi, L.tqgpu_mpc_step(g.h, dp(x), C.byref(o), C.byref(res), dp(u)), -2, "kind 1")
        assert g.solve(**c["opts"])["n_launches"] == launches1
        _same_bits(g.root_bounds()[0], c["x0"], "xmin[0] after the refusals")
    finally:
        g.close()
    # a rank of a sharded solve
    from treeqp_amd import problems as P
    mk = SC._lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05))
    ranks = [mk(capi) for _ in range(2)]
    try:
        for i, m in enumerate(ranks):
            m.pshard_init(i, 2)
        # (n_launches of a following tqgpu_solve cannot be had on a rank: the sharded solve of both ranks, before and after, instead)
        keys = COUNTS + ("n_launches",)
        before = [[{k: r[k] for k in keys} for r in capi.pshard_solve_local(ranks)] for _ in range(2)][1]          # (the first one connects)
        m = ranks[1]
        for rc in (L.tqgpu_mpc_set_root_states(m.h), L.tqgpu_get_root_bounds(m.h, None, None), L.tqgpu_mpc_set_certify(m.h, 1),
                   L.tqgpu_mpc_get_certificate(m.h, None, None)):
            _refused(capi, rc, -4, "sharded")
        after = [{k: r[k] for k in keys} for r in capi.pshard_solve_local(ranks)]
        assert after == before, f"the refusals on a rank left something behind: {before} -> {after}"
    finally:
        for m in ranks:
            m.close()

"""MPC steps on the device (tqgpu_mpc_*, tqgpu_set_warm_start): the x0 fold, the warm start and u[0] against the host loop the
parent commit offers -- numpy fold, upload, tqgpu_set_lambda with the last duals, tqgpu_solve, tqgpu_get_solution.  One tree per
route (mpc_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import mpc_cases as M
import solve_sequence_cases as SC

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")
COUNTS = ("status", "iter", "ls_total")


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _host_step(capi, g, c, terms, lam):
    """one step of the host loop on the mirror g: upload the folded terms, start from lam (None: the zeros of the first step), solve, download"""
    M.host_upload(g, c, terms)
    g.set_lambda(lam)
    r = g.solve(**c["opts"])
    return r, g.solution()


def _u0(sol, c):
    return sol["u"][:int(c["d"]["nu"][0])]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact data: the fold bit for bit, the device loop bit for bit the host loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", M.CASE_IDS)
def test_exact_fold_and_loop_bit_for_bit(capi, cid):
    c = M.case(cid)
    dev, host = M.make(capi, c), M.make(capi, c, root=False)
    if c["path"] is not None:
        assert dev.path == c["path"], f"{cid}: route {dev.path}, expected {c['path']}"
    dev.set_warm_start(1)
    assert dev.warm_start == 1
    lam = None
    try:
        for step, x0 in enumerate(M.exact_x0s(c["nx0"], 0)):
            terms = M.fold(c["root"], x0)
            dev.mpc_set_x0(x0)
            got = dev.root_terms()
            for k, v in terms.items():
                _same_bits(got[k], v, f"{cid} step {step}: root term {k}")
            rd, u0 = dev.mpc_step(x0, **c["opts"])
            sd = dev.solution()
            rh, sh = _host_step(capi, host, c, terms, lam)
            lam = sh["lam"]
            print(f"{cid} step {step}: device {[rd[k] for k in COUNTS]} host {[rh[k] for k in COUNTS]} launches {rd['n_launches']} stats {capi.mpc_stats()}")
            for k in COUNTS:
                assert rd[k] == rh[k], f"{cid} step {step}: {k} {rd[k]} != {rh[k]}"
            _same_bits(u0, _u0(sh, c), f"{cid} step {step}: u0")
            for k in SOL_KEYS:
                _same_bits(sd[k], sh[k], f"{cid} step {step}: {k}")
    finally:
        dev.close(); host.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. general data, closed loop
# ---------------------------------------------------------------------------------------------------------------------------------
GENERAL_STEPS = 10


def _general_root(c, seed):
    """random originals (not quantised) with nx0 = nx of the root's first child, so that the loop can be closed through that child:
    x0+ = A0 x0 + B0 u0, A0 a contraction"""
    d = c["d"]
    rng = np.random.Generator(np.random.PCG64(seed))
    nk0, nx0 = int(d["nk"][0]), int(d["nx"][1])
    A0 = [0.6 / np.sqrt(nx0) * rng.standard_normal((int(d["nx"][k]), nx0)) for k in range(1, 1 + nk0)]
    root = dict(A0=A0, b0=0.1 * rng.standard_normal(int(d["nx"][1:1 + nk0].sum())), S0=None, r0=None, C0=None, dmin0=None, dmax0=None)
    B0 = d["B"][:nx0 * int(d["nu"][0])].reshape((nx0, int(d["nu"][0])), order="F")
    return root, B0, rng.standard_normal(nx0)


def _host_loop(capi, c, root, B0, x0, bump=None):
    """the closed loop through the host: per step (counts, solution); bump: a one-ulp perturbation of b at that step's entry"""
    g = M.make(capi, c, root=False)
    out, lam = [], None
    try:
        for step in range(GENERAL_STEPS):
            terms = M.fold(root, x0)
            if bump is not None:
                terms["b"][bump % len(terms["b"])] = np.nextafter(terms["b"][bump % len(terms["b"])], np.inf)
            r, s = _host_step(capi, g, c, terms, lam)
            lam = s["lam"]
            out.append((r, s))
            x0 = root["A0"][0] @ x0 + B0 @ _u0(s, c)
    finally:
        g.close()
    return out


@pytest.mark.parametrize("cid", M.CLIPPING_IDS)
def test_general_data_closed_loop(capi, cid):
    c = M.case(cid)
    root, B0, x0 = _general_root(c, 40 + M.CASE_IDS.index(cid))
    ref = _host_loop(capi, c, root, B0, x0)
    bumped = _host_loop(capi, c, root, B0, x0, bump=3)
    cap = GENERAL_STEPS // 10
    n_ulp = sum(any(a[0][k] != b[0][k] for k in ("iter", "ls_total")) for a, b in zip(ref, bumped))
    print(f"{cid}: host loop against itself with b moved by one ulp: {n_ulp} steps with other counts")
    assert n_ulp <= cap, f"{cid}: the seed does not give a sequence that is stable under a one-ulp perturbation ({n_ulp} steps)"
    dev = M.make(capi, c, root=False)
    dev.mpc_set_root(root["A0"], root["b0"])
    dev.set_warm_start(1)
    other = 0
    try:
        for step in range(GENERAL_STEPS):
            terms = M.fold(root, x0)
            dev.mpc_set_x0(x0)
            err = np.abs(dev.root_terms()["b"] - terms["b"])
            bound = M.fold_bound(root, x0)
            print(f"{cid} step {step}: fold error / bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound), f"{cid} step {step}: fold off by {np.max(err / bound):.2f} of its bound"
            rd, u0 = dev.mpc_step(None, **c["opts"])
            sd = dev.solution()
            rh, sh = ref[step]
            kkt = dev.kkt_residual()["max"]
            print(f"{cid} step {step}: device {[rd[k] for k in COUNTS]} host {[rh[k] for k in COUNTS]} KKT {kkt:.2e}")
            assert rd["status"] == 0 == rh["status"]
            assert kkt < 1e-8
            assert np.array_equal(u0, _u0(sd, c))
            if rd["iter"] == rh["iter"] and rd["ls_total"] == rh["ls_total"]:
                H.assert_solution_close(sd, sh, tol=1e-10)
            else:
                other += 1
                H.assert_solution_close(sd, sh, tol=1e-6, keys=("x", "u"))          # at the optimum only: both are within the solver's tolerance of it
            x0 = root["A0"][0] @ x0 + B0 @ _u0(sh, c)
        assert other <= cap, f"{cid}: {other} of {GENERAL_STEPS} steps took other counts than the host loop"
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the warm start alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["single_wg", "persist_c1", "generic", "dense_kind3_root"])
def test_warm_start_equals_explicit_set_lambda(capi, cid):
    c = M.case(cid)
    x0 = M.exact_x0s(c["nx0"], 0)[0]
    d = M.folded(c, M.fold(c["root"], x0))
    a, b = M.make(capi, c, d=d, root=False), M.make(capi, c, d=d, root=False)
    try:
        assert a.warm_start == 0
        a.set_warm_start(1)
        # three solves, then a maxIter = 1 exit (status 1) and one more solve from where it stopped
        for step, extra in enumerate([{}, {}, {}, dict(maxIter=1), {}]):
            if step == 3:          # away from the optimum, so that one iteration is not enough
                far = 0.5 * np.random.Generator(np.random.PCG64(5)).standard_normal(a.sum_lam)
                a.set_lambda(far); b.set_lambda(far)
            opts = {**c["opts"], **extra}
            ra, rb = a.solve(**opts), b.solve(**opts)
            sa, sb = a.solution(), b.solution()
            if step == 3:
                assert ra["status"] == 1 == rb["status"]
            for k in COUNTS:
                assert ra[k] == rb[k], f"{cid} solve {step}: {k}"
            for k in SOL_KEYS:
                _same_bits(sa[k], sb[k], f"{cid} solve {step}: {k}")
            b.set_lambda(sb["lam"])          # the explicit warm start of the next solve
        # mode 0 is unchanged: every solve from the buffer of set_lambda
        a.set_warm_start(0)
        lam0 = 0.1 * np.random.Generator(np.random.PCG64(6)).standard_normal(a.sum_lam)
        a.set_lambda(lam0); b.set_lambda(lam0)
        first = None
        for _ in range(2):
            ra, rb = a.solve(**c["opts"]), b.solve(**c["opts"])
            sa = a.solution()
            _same_bits(sa["lam"], b.solution()["lam"], f"{cid}: mode 0")
            first = first or (ra, sa)
            assert [ra[k] for k in COUNTS] == [first[0][k] for k in COUNTS]
            _same_bits(sa["lam"], first[1]["lam"], f"{cid}: mode 0 repeats its solve")
        # mode 1 after a set_lambda: that buffer, for one solve
        a.set_warm_start(1)
        a.set_lambda(lam0)
        ra = a.solve(**c["opts"])
        assert [ra[k] for k in COUNTS] == [first[0][k] for k in COUNTS]
        _same_bits(a.solution()["lam"], first[1]["lam"], f"{cid}: mode 1 after set_lambda")
    finally:
        a.close(); b.close()


def test_warm_start_across_a_route_switch(capi):
    c = M.case("dense_kind3_root")
    d = M.folded(c, M.fold(c["root"], M.exact_x0s(c["nx0"], 0)[0]))
    a, b = M.make(capi, c, d=d, root=False), M.make(capi, c, d=d, root=False)
    try:
        a.set_warm_start(1)
        far = 0.3 * np.random.Generator(np.random.PCG64(9)).standard_normal(a.sum_lam)
        a.set_lambda(far); b.set_lambda(far)
        for step, single in enumerate([False, True, False]):
            a.set_dense_single_launch(single); b.set_dense_single_launch(single)
            if single:
                assert a.dense_single_launch[1] == 1 and a.path == 3
            opts = {**c["opts"], **(dict(maxIter=2) if step == 0 else {})}
            ra, rb = a.solve(**opts), b.solve(**opts)
            sa, sb = a.solution(), b.solution()
            for k in COUNTS:
                assert ra[k] == rb[k], f"solve {step}: {k}"
            for k in SOL_KEYS:
                _same_bits(sa[k], sb[k], f"solve {step}: {k}")
            b.set_lambda(sb["lam"])
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the stale mirror of tqgpu_set_problem
# ---------------------------------------------------------------------------------------------------------------------------------
def test_set_problem_after_a_fold_uploads_again(capi):
    c = M.case("persist_c1")
    xs = M.exact_x0s(c["nx0"], 0)
    t0 = M.fold(c["root"], xs[0])
    g = M.make(capi, c)
    try:
        M.host_upload(g, c, t0)
        g.set_lambda(None)
        r0 = g.solve(**c["opts"]); s0 = g.solution()
        g.mpc_set_x0(xs[1])
        assert not np.array_equal(g.root_terms()["b"], t0["b"])
        M.host_upload(g, c, t0)          # the same arrays as before: the mirror must not claim that the device still holds them
        _same_bits(g.root_terms()["b"], t0["b"], "b after tqgpu_set_problem")
        g.set_lambda(None)
        r1 = g.solve(**c["opts"]); s1 = g.solution()
        assert [r0[k] for k in COUNTS] == [r1[k] for k in COUNTS]
        for k in SOL_KEYS:
            _same_bits(s1[k], s0[k], k)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the hot start of the kind-3 stage solver survives a fold
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fold_keeps_the_stored_working_sets(capi):
    c = M.case("dense_kind3_root")
    # rows that are active at the root: a narrow range, so that a cold stage solve has steps to make
    root = dict(c["root"])
    root["dmin0"], root["dmax0"] = np.full(2, -1.0 / 64), np.full(2, 1.0 / 64)
    cc = dict(c, root=root)
    xs = M.exact_x0s(c["nx0"], 0)
    x1 = xs[0] + 1.0 / 64
    hot, cold = M.make(capi, cc), M.make(capi, cc)
    try:
        for g in (hot, cold):
            g.set_warm_start(1)
            g.mpc_step(xs[0], **c["opts"])
        cold.set_gen_hot_start(True)          # empties the stored sets
        rh, _ = hot.mpc_step(x1, **c["opts"])
        rc, _ = cold.mpc_step(x1, **c["opts"])
        th, tc = hot.stage_steps()["total"], cold.stage_steps()["total"]
        print(f"kind-3 root: steps with the kept sets {th[0]}, after emptying them {tc[0]}; iterations {rh['iter']} / {rc['iter']}")
        assert rh["status"] == 0 == rc["status"]
        assert tc[0] > 0 and th[0] < tc[0], "the step after a fold started cold"
    finally:
        hot.close(); cold.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the batch step
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch_run(capi, c, n, steps=3):
    rng = np.random.Generator(np.random.PCG64(77))
    x0s = [[M.quantised(rng, c["nx0"], 1.0) for _ in range(n)] for _ in range(steps)]
    members, alone = [M.make(capi, c) for _ in range(n)], [M.make(capi, c) for _ in range(n)]
    stats = []
    try:
        for g in members + alone:
            g.set_warm_start(1)
        for step in range(steps):
            res, u0s = capi.mpc_step_batch(members, x0s[step], **c["opts"])
            stats.append(capi.mpc_stats())
            for i in range(n):
                ra, ua = alone[i].mpc_step(x0s[step][i], **c["opts"])
                for k in COUNTS:
                    assert res[i][k] == ra[k], f"step {step} member {i}: {k}"
                _same_bits(u0s[i], ua, f"step {step} member {i}: u0")
                sm, sa = members[i].solution(), alone[i].solution()
                for k in SOL_KEYS:
                    _same_bits(sm[k], sa[k], f"step {step} member {i}: {k}")
    finally:
        for g in members + alone:
            g.close()
    return stats


def test_batch_step_members_bit_for_bit_and_flat_cost(capi):
    c = M.case("persist_c1")
    s8, s2 = _batch_run(capi, c, 8), _batch_run(capi, c, 2)
    print(f"batch step: 8 members {s8}, 2 members {s2}")
    # the steady state (the first call uploads, packs and waits for the members' own streams): one launch ahead, the members' shared
    # launch, the post; the descriptors; the wait for the post's tag
    assert s8[-1] == s2[-1] == dict(launches=3, copies=1, waits=1)
    assert s8[1] == s2[1]


def test_single_step_cost_on_the_persistent_route(capi):
    c = M.case("persist_c1")
    g = M.make(capi, c)
    try:
        g.set_warm_start(1)
        for x0 in M.exact_x0s(c["nx0"], 0)[:3]:
            r, _ = g.mpc_step(x0, **c["opts"])
            st = capi.mpc_stats()
        assert r["n_launches"] == 1 and g.path == 2
        # fold + warm start, the solve, the post of u0; nothing is copied in either direction; the host waits once, for the post's tag
        assert st == dict(launches=3, copies=0, waits=1), st
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the routes into k_mpc_pre, two by two: a step that does it all in its one launch, and the same state reached through the call
#    that does one part alone
# ---------------------------------------------------------------------------------------------------------------------------------
# what the commit before the shared launcher counted on this tree (one launch of one workgroup per solve): of a step, k_mpc_pre + the
# solve + the post of u0 and no copy -- whatever k_mpc_pre has to do, and nothing for a tqgpu_mpc_set_x0, _set_window or _shift ahead
# of it, which are no steps; of a tqgpu_solve in warm start mode 1, the solve and its own warm-start copy
PRE_STEP = dict(launches=3, copies=0)
PRE_STEP_N_LAUNCHES = 1
PRE_SOLVE_N_LAUNCHES = 2


def _pre_pair(what, ra, ua, rb, ub, stats_a, stats_b, launches_b):
    print(f"{what}: step {[ra[k] for k in COUNTS]} launches {ra['n_launches']} stats {stats_a}; other route {[rb[k] for k in COUNTS]} "
          f"launches {rb['n_launches']} stats {stats_b}")
    for k in COUNTS:
        assert ra[k] == rb[k], f"{what}: {k} {ra[k]} != {rb[k]}"
    assert ra["status"] == 0
    _same_bits(ua, ub, f"{what}: u0")
    for st in (stats_a, stats_b):
        assert {k: st[k] for k in PRE_STEP} == PRE_STEP, f"{what}: {st}"
    assert ra["n_launches"] == PRE_STEP_N_LAUNCHES and rb["n_launches"] == launches_b


def test_routes_into_the_pre_kernel_agree(capi):
    import tracking_cases as T
    c = M.case("one_child")
    xs = M.exact_x0s(c["nx0"], 3)
    made = []

    def pair(make, mode_a, mode_b):
        a, b = make(), make()
        made.extend([a, b])
        assert a.path == 3
        a.set_warm_start(mode_a); b.set_warm_start(mode_b)
        return a, b
    try:
        # fold + warm start in a step's launch | tqgpu_mpc_set_x0, then the warm-start copy of tqgpu_solve's solve_begin
        a, b = pair(lambda: M.make(capi, c), 1, 1)
        for g in (a, b):
            g.mpc_step(xs[0], **c["opts"])
        ra, ua = a.mpc_step(xs[1], **c["opts"])
        st = capi.mpc_stats()
        b.mpc_set_x0(xs[1])
        rb = b.solve(**c["opts"])
        _pre_pair("warm start", ra, ua, rb, _u0(b.solution(), c), st, capi.mpc_stats(), PRE_SOLVE_N_LAUNCHES)          # (the record stays the step's: b counted nothing)

        # the shifted warm start of mode 2 in a step's launch | tqgpu_mpc_shift of a mirror in mode 0, then a step that only folds
        a, b = pair(lambda: M.make(capi, c).mpc_set_shift(), 2, 0)
        for g in (a, b):
            g.mpc_step(xs[0], **c["opts"])
        ra, ua = a.mpc_step(xs[1], **c["opts"])
        st = capi.mpc_stats()
        b.mpc_shift()
        rb, ub = b.mpc_step(xs[1], **c["opts"])
        _pre_pair("shift", ra, ua, rb, ub, st, capi.mpc_stats(), PRE_STEP_N_LAUNCHES)

        # the window fold in a step's launch (tqgpu_mpc_step_at) | tqgpu_mpc_set_window, then a step that keeps the window.  A reference
        # trajectory needs one nx below the root: the same tree with nx = 3 on every node
        ct = T._elim("one_child_nx3", H.shaped_qp([1, 2, 0, 0], [0, 3, 3, 3], 2, 21).as_dict(), M.NX0, 5, True)
        a, b = pair(lambda: T.make(capi, ct), 1, 1)
        for g in (a, b):
            g.mpc_step(xs[0], t0=0, **ct["opts"])
        ra, ua = a.mpc_step(xs[1], t0=2, **ct["opts"])
        st = capi.mpc_stats()
        b.mpc_set_window(2)
        rb, ub = b.mpc_step(xs[1], **ct["opts"])
        assert a.mpc_window == 2 == b.mpc_window
        _pre_pair("window", ra, ua, rb, ub, st, capi.mpc_stats(), PRE_STEP_N_LAUNCHES)
    finally:
        for g in made:
            g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(capi, rc, code, text):
    assert rc == code, f"{rc} != {code}: {capi.lib().tqgpu_last_error().decode()}"
    assert text in capi.lib().tqgpu_last_error().decode()


def test_refusals(capi):
    L = capi.lib()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    c = M.case("one_child")
    r = c["root"]
    A0 = np.concatenate([A.ravel(order="F") for A in r["A0"]])
    g = M.make(capi, c, root=False)
    x = np.zeros(c["nx0"])
    launches0 = g.solve(**c["opts"])["n_launches"]
    try:
        _refused(capi, L.tqgpu_mpc_set_x0(g.h, dp(x)), -2, "tqgpu_mpc_set_root")                      # before the root terms
        o, res, u = capi._gpu_opts(), capi.GpuResult(), np.zeros(4)
        _refused(capi, L.tqgpu_mpc_step(g.h, dp(x), C.byref(o), C.byref(res), dp(u)), -2, "tqgpu_mpc_set_root")
        _refused(capi, L.tqgpu_mpc_set_root(g.h, 0, dp(A0), dp(r["b0"]), None, None, None, None, None), -2, "nx0")
        S0 = np.ones(int(c["d"]["nu"][0]) * c["nx0"])
        _refused(capi, L.tqgpu_mpc_set_root(g.h, c["nx0"], dp(A0), dp(r["b0"]), dp(S0), dp(np.zeros(8)), None, None, None), -2, "kind 0")
        _refused(capi, L.tqgpu_mpc_set_root(g.h, c["nx0"], dp(A0), dp(r["b0"]), None, None, dp(S0), dp(S0), dp(S0)), -2, "rows")
        _refused(capi, L.tqgpu_set_warm_start(g.h, 2), -2, "mode")
        assert g.solve(**c["opts"])["n_launches"] == launches0          # nothing was launched, nothing changed
    finally:
        g.close()
    # a root that still has states
    kind, shape, _ = __import__("limit_shapes").case("g_persist_node_sizes-nz16")
    d = __import__("limit_shapes").problem(kind, shape)
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)
    try:
        _refused(capi, L.tqgpu_mpc_set_root(g.h, 3, dp(np.zeros(64)), dp(np.zeros(64)), None, None, None, None, None), -2, "eliminate x0 first")
    finally:
        g.close()
    # a rank of a sharded solve
    from treeqp_amd import problems as P
    mk = SC._lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05))
    ranks = [mk(capi) for _ in range(2)]
    try:
        for i, m in enumerate(ranks):
            m.pshard_init(i, 2)
        m = ranks[1]
        o, res, u = capi._gpu_opts(), capi.GpuResult(), np.zeros(4)
        for rc in (L.tqgpu_mpc_set_root(m.h, 3, dp(np.zeros(64)), dp(np.zeros(64)), None, None, None, None, None), L.tqgpu_mpc_set_x0(m.h, dp(x)),
                   L.tqgpu_set_warm_start(m.h, 1), L.tqgpu_get_root_terms(m.h, None, None, None, None),
                   L.tqgpu_mpc_step(m.h, None, C.byref(o), C.byref(res), dp(u))):
            _refused(capi, rc, -4, "sharded")
        arr = (C.c_void_p * 2)(*[q.h for q in ranks])
        res2 = (capi.GpuResult * 2)()
        _refused(capi, L.tqgpu_mpc_step_batch(arr, 2, None, C.byref(o), res2, dp(u)), -4, "sharded")
    finally:
        for m in ranks:
            m.close()

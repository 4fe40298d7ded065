"""The shifted warm start on the device (tqgpu_mpc_set_shift, tqgpu_mpc_set_realised, tqgpu_set_warm_start(2), tqgpu_mpc_shift,
tqgpu_get_working_sets, tqgpu_set_working_sets) against the host loop the parent commit's API allows on a twin mirror: tqgpu_get_solution,
the numpy gather of shift_cases.py, tqgpu_set_lambda, step.  Both mirrors take the same steps (x0 and the window fold on the device), so
every difference is the shift's."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import mpc_cases as M
import mpc_root_cases as R
import shift_cases as SH
import solve_sequence_cases as SC
import tracking_cases as K
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")
COUNTS = ("status", "iter", "ls_total")
STEADY = dict(launches=3, copies=0, waits=1)
STEPS = 8


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _same_step(c, what, rd, u0, sd, rh, sh):
    for k in COUNTS:
        assert rd[k] == rh[k], f"{what}: {k} {rd[k]} != {rh[k]}"
    if u0 is not None:
        _same_bits(u0, sh["u"][:int(c["d"]["nu"][0])], f"{what}: u0")
    for k in SOL_KEYS + (("mu_d",) if "nc" in c["d"] else ()):
        _same_bits(sd[k], sh[k], f"{what}: {k}")


def _uniform_255():
    """the uniform (nx, nu, md) = (4, 1, 2) tree of depth 7: 255 nodes, sum_nx = 1020 = 15 * 64 + 60: two warm blocks, the last one ragged"""
    d = P.random_uniform_tree_qp(5, 4, 1, 2, 7, 7).as_dict()
    assert len(d["nk"]) == 255 and 513 <= int(d["nx"].sum()) <= 1536 and int(d["nx"].sum()) % 64 != 0
    return K._states("uniform_255", d, 7, False, path=2)


def _case(cid):
    if cid == "uniform_255":
        return _uniform_255()
    if cid == "irregular_single_wg":          # nx = 4; 8, 6; 3, 3: no inner node's image fits, zeros are written
        return dict(R.case("single_wg"), x0s=R.x0_sequence(R.case("single_wg"), steps=STEPS))
    return K.case(cid)


def _make(capi, c):
    return K.make(capi, c) if "xtraj" in c else R.make(capi, c, root_states=True)


def _step(g, c, x0, step):
    return g.mpc_step(x0, **(dict(t0=step) if "xtraj" in c else {}), **c["opts"])


def _shift_loop(capi, c, leaf, before=None, steps=STEPS):
    nk, nx = c["d"]["nk"], c["d"]["nx"]
    nk0 = int(nk[0])
    maps = [SH.ref_map(nk, nx, j, leaf)[0] for j in range(nk0)]
    dev, host = _make(capi, c), _make(capi, c)
    differs, stats = 0, []
    try:
        dev.mpc_set_shift(leaf, capi.SHIFT_DUALS)
        dev.set_warm_start(2)
        assert dev.warm_start == 2 and dev.mpc_shift_state == dict(leaf=leaf, what=capi.SHIFT_DUALS, realised=0)
        if before == "solve":          # the persistent route's constants are packed and current when the first step comes
            dev.solve(**c["opts"]); host.solve(**c["opts"])
        for step in range(steps):
            x0, j = c["x0s"][step % len(c["x0s"])], step % nk0
            if before == "bounds" and step in (1, 3):          # a re-pack is pending when the step comes
                d2 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
                nu0 = int(d2["nu"][0])
                d2["umax"][nu0:2 * nu0] *= 0.5 + 0.1 * step
                if c["form"] == "states":
                    d2 = R.with_x0(c, c["x0s"][step - 1], d2)
                for g in (dev, host):
                    R.set_bounds(capi, g, d2)
            if step > 0 or before == "solve":
                dev.mpc_set_realised(j)
                lam = host.solution()["lam"]
                start = SH.gather_lam(nx, maps[j], lam)
                differs += int(not np.array_equal(start, lam))
                host.set_lambda(start)
            rd, u0 = _step(dev, c, x0, step)
            stats.append(capi.mpc_stats())
            rh, _ = _step(host, c, x0, step)
            print(f"{c['id']} leaf {leaf} step {step} realised {j}: device {[rd[k] for k in COUNTS]} host {[rh[k] for k in COUNTS]} stats {stats[-1]}")
            if step == 1:
                assert differs, f"{c['id']}: the gathered duals are the ungathered ones: the test would pass with a plain copy"
            _same_step(c, f"{c['id']} step {step}", rd, u0, dev.solution(), rh, host.solution())
    finally:
        dev.close(); host.close()
    return stats


LOOP_CASES = [(cid, SH.REPEAT, None) for cid in K.CASE_IDS] + [("c1_root_states", SH.REPEAT, "solve"), ("c1_eliminated", SH.REPEAT, "bounds"),
                                                             ("c1_root_states", SH.ZERO, None), ("uniform_255", SH.REPEAT, None),
                                                             ("irregular_single_wg", SH.REPEAT, None), ("irregular_single_wg", SH.ZERO, None)]


@pytest.mark.parametrize("cid,leaf,before", LOOP_CASES, ids=[f"{a}-leaf{b}-{c}" for a, b, c in LOOP_CASES])
def test_loop_bit_for_bit_the_host_loop(capi, cid, leaf, before):
    c = _case(cid)
    stats = _shift_loop(capi, c, leaf, before)
    if cid in ("c1_root_states", "uniform_255") and before is None:
        assert stats[-1] == STEADY, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the shift alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["single_wg", "c1_eliminated"])
def test_shift_alone_then_solve(capi, cid):
    """tqgpu_mpc_shift + tqgpu_solve is set_lambda(gathered) + tqgpu_solve; the solve after it starts from the buffer of tqgpu_set_lambda
    again on a mirror in mode 0 (the twin sets that buffer again and must get the same bits)"""
    c = K.case(cid)
    nk, nx = c["d"]["nk"], c["d"]["nx"]
    j = int(nk[0]) - 1
    img = SH.ref_map(nk, nx, j, SH.REPEAT)[0]
    a, b = K.make(capi, c, tracking=False), K.make(capi, c, tracking=False)
    try:
        for g in (a, b):
            g.mpc_set_x0(c["x0s"][0])
        assert capi.lib().tqgpu_mpc_shift(a.h) == -2 and b"tqgpu_mpc_set_shift" in capi.lib().tqgpu_last_error()
        a.mpc_set_shift(SH.REPEAT).mpc_set_realised(j)
        assert capi.lib().tqgpu_mpc_shift(a.h) == -2 and b"not solved yet" in capi.lib().tqgpu_last_error()
        rng = np.random.Generator(np.random.PCG64(3))
        L0 = 0.01 * rng.standard_normal(a.sum_lam)
        a.set_lambda(L0); b.set_lambda(L0)
        r1a, r1b = a.solve(**c["opts"]), b.solve(**c["opts"])
        _same_step(c, f"{cid}: first solve", r1a, None, a.solution(), r1b, b.solution())
        lam = b.solution()["lam"]
        start = SH.gather_lam(nx, img, lam)
        assert not np.array_equal(start, lam)
        a.mpc_shift()
        b.set_lambda(start)
        assert a.warm_start == 0
        r2a, r2b = a.solve(**c["opts"]), b.solve(**c["opts"])
        print(f"{cid}: after the shift {[r2a[k] for k in COUNTS]}, after set_lambda(gathered) {[r2b[k] for k in COUNTS]}")
        _same_step(c, f"{cid}: the solve behind the shift", r2a, None, a.solution(), r2b, b.solution())
        b.set_lambda(L0)
        r3a, r3b = a.solve(**c["opts"]), b.solve(**c["opts"])
        _same_step(c, f"{cid}: mode 0 after the shifted solve", r3a, None, a.solution(), r3b, b.solution())
        # in mode 1 the shift stands in for the copy of one solve
        a.set_warm_start(1)
        lam = b.solution()["lam"]
        a.mpc_shift(); b.set_lambda(SH.gather_lam(nx, img, lam))
        r4a, r4b = a.solve(**c["opts"]), b.solve(**c["opts"])
        _same_step(c, f"{cid}: mode 1, the solve behind the shift", r4a, None, a.solution(), r4b, b.solution())
        b.set_lambda(b.solution()["lam"])
        r5a, r5b = a.solve(**c["opts"]), b.solve(**c["opts"])
        _same_step(c, f"{cid}: mode 1 after the shifted solve", r5a, None, a.solution(), r5b, b.solution())
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the working sets
# ---------------------------------------------------------------------------------------------------------------------------------
WS_KEYS = ("bounds", "rows", "bound_sides", "row_sides")


def ws_case(seed=41, span=0.0625):
    """7 nodes, nk = [2, 1, 1, 1, 1, 0, 0], nx = 3 everywhere, nu = 2 and two rows on every inner node: the inner nodes of kind 3 with rows
    within +- span (tight at the solution, as tracking_cases.active_rows_case), the leaves of kind 2"""
    nk = [2, 1, 1, 1, 1, 0, 0]
    d = H.dense_shaped_qp(nk, [3] * 7, 2, seed)
    kinds = np.array([3, 3, 3, 3, 3, 2, 2], dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    d["nc"] = np.array([2, 2, 2, 2, 2, 0, 0], dtype=np.int32)
    d["C"] = np.concatenate([np.zeros(2 * 3)] + [M.quantised(rng, 2 * 3, 0.25) for _ in range(4)])
    d["D"] = M.quantised(rng, 5 * 2 * 2, 1.0)
    d["dmin"], d["dmax"] = -span * np.ones(10), span * np.ones(10)
    return K._states(f"ws_tree-{seed}", d, seed, True, kinds=kinds, opts=SC.FULL)


def _gathered(c, ws, j, leaf=SH.REPEAT):
    d = c["d"]
    img, rep = SH.ref_map(d["nk"], d["nx"], j, leaf)
    return SH.gather_sets(d["nx"], d["nu"], d["nc"], c["kinds"], img, rep, ws)


def _same_sets(a, b, what):
    for k in WS_KEYS:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} {a[k]} != {b[k]}"


def test_working_sets_move_with_the_shift(capi):
    """after a converged solve tqgpu_mpc_shift leaves the numpy gather of working_sets(); the halves that say what P_k was built for have no
    getter: that they stay is what the loop below shows, whose device mirror would otherwise solve with another P than its twin"""
    c = ws_case()
    g = K.make(capi, c)
    try:
        g.mpc_set_x0(c["x0s"][0]); g.mpc_set_window(0)
        assert g.solve(**c["opts"])["status"] == 0
        mu = g.solution()["mu_d"]
        ws0 = g.working_sets()
        print(f"ws tree: sets after the solve { {k: [hex(int(v)) for v in ws0[k]] for k in WS_KEYS} }, row multipliers {mu}")
        assert np.count_nonzero(ws0["rows"]) >= 2, "fewer than two nodes have rows in their sets"
        assert not ws0["rows"][5:].any() and not ws0["row_sides"][5:].any()
        moving = [j for j in (0, 1) if any(not np.array_equal(_gathered(c, ws0, j)[k], ws0[k]) for k in WS_KEYS)]
        assert moving, "no realisation moves a set: the test would pass without the gather"
        j = moving[0]
        g.mpc_set_shift(SH.REPEAT, capi.SHIFT_DUALS | capi.SHIFT_WORKING_SETS).mpc_set_realised(j)
        g.mpc_shift()
        ws1, want = g.working_sets(), _gathered(c, ws0, j)
        _same_sets(ws1, want, f"realisation {j}")
        assert any(ws1[k][n] != ws0[k][n] for k in WS_KEYS for n in range(7)), "no node's set changed"
        for n in (3, 4, 5, 6):          # nodes 3, 4 have other nu than their images (leaves), the leaves repeat themselves
            assert all(ws1[k][n] == ws0[k][n] for k in WS_KEYS), n
        # without the flag the sets stay
        g.set_working_sets(**ws0)
        _same_sets(g.working_sets(), ws0, "set / get round trip")
        g.mpc_set_shift(SH.REPEAT, capi.SHIFT_DUALS).mpc_set_realised(j)
        g.mpc_shift()
        _same_sets(g.working_sets(), ws0, "TQGPU_SHIFT_DUALS alone")
        # a partial set: only the rows
        g.set_working_sets(rows=ws1["rows"])
        _same_sets(g.working_sets(), dict(ws0, rows=ws1["rows"]), "rows alone")
    finally:
        g.close()
    # a clipping tree reads as zeros and ignores what is set
    cc = K.case("single_wg")
    g = K.make(capi, cc, tracking=False)
    try:
        ones = np.full(len(cc["d"]["nk"]), 3, dtype=np.uint64)
        g.set_working_sets(ones, ones, ones, ones)
        assert not any(v.any() for v in g.working_sets().values())
    finally:
        g.close()


def _ws_loop(capi, c, what, steps=6):
    d = c["d"]
    dev, host = K.make(capi, c), K.make(capi, c)
    total = 0
    try:
        dev.mpc_set_shift(SH.REPEAT, what)
        dev.set_warm_start(2)
        for step in range(steps):
            x0, j = c["x0s"][step], step % 2
            if step > 0:
                dev.mpc_set_realised(j)
                img = SH.ref_map(d["nk"], d["nx"], j, SH.REPEAT)[0]
                host.set_lambda(SH.gather_lam(d["nx"], img, host.solution()["lam"]))
                if what & capi.SHIFT_WORKING_SETS:
                    host.set_working_sets(**_gathered(c, host.working_sets(), j))
            rd, u0 = dev.mpc_step(x0, t0=step, **c["opts"])
            st = capi.mpc_stats()
            rh, _ = host.mpc_step(x0, t0=step, **c["opts"])
            _same_step(c, f"{c['id']} what {what} step {step}", rd, u0, dev.solution(), rh, host.solution())
            _same_sets(dev.working_sets(), host.working_sets(), f"{c['id']} what {what} step {step}")
            sd, sh = dev.stage_steps()["total"], host.stage_steps()["total"]
            assert np.array_equal(sd, sh), (sd, sh)
            if step > 0:
                total += int(sd.sum())
    finally:
        dev.close(); host.close()
    return total, st


def test_working_set_loop_bit_for_bit_and_costs(capi):
    c = ws_case()
    with_sets, st_with = _ws_loop(capi, c, capi.SHIFT_DUALS | capi.SHIFT_WORKING_SETS)
    without, st_without = _ws_loop(capi, c, capi.SHIFT_DUALS)
    print(f"ws tree: active-set steps of the kind-3 nodes over 5 shifted steps: {with_sets} with TQGPU_SHIFT_WORKING_SETS, {without} without; "
          f"stats {st_with} / {st_without}")
    assert st_with["launches"] <= st_without["launches"], (st_with, st_without)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. what a shifted step costs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_costs(capi):
    c = K.case("c1_root_states", exact=False)
    g = K.make(capi, c)
    try:
        g.mpc_set_shift(SH.REPEAT, capi.SHIFT_DUALS).set_warm_start(2)
        for step in range(4):
            g.mpc_set_realised(step % 2)
            r, _ = g.mpc_step(c["x0s"][step], t0=step, **c["opts"])
            st = capi.mpc_stats()
            print(f"shifted tracking step {step}: {[r[k] for k in COUNTS]} launches {r['n_launches']} stats {st}")
        assert r["n_launches"] == 1 and st == STEADY, (r, st)
    finally:
        g.close()
    members = [K.make(capi, c) for _ in range(4)]
    try:
        for i, m in enumerate(members):
            m.mpc_set_shift(SH.REPEAT, capi.SHIFT_DUALS).set_warm_start(2)
        for step in range(3):
            for i, m in enumerate(members):
                m.mpc_set_realised((step + i) % 2)
            capi.mpc_step_batch(members, [c["x0s"][step + i] for i in range(4)], t0s=[step] * 4, **c["opts"])
            st = capi.mpc_stats()
            print(f"shifted batch step {step}: stats {st}")
        assert st == dict(launches=3, copies=1, waits=1), st
    finally:
        for m in members:
            m.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the batch step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_mixes_modes_and_realisations(capi):
    c = K.case("c1_root_states", exact=False)
    modes = [0, 1, 2, 2, 2]
    track = [True, True, True, False, True]
    mk = [(lambda t=t: K.make(capi, c, tracking=t)) for t in track]
    members, alone = [m() for m in mk], [m() for m in mk]
    try:
        for i in range(5):
            for g in (members[i], alone[i]):
                if modes[i] == 2:
                    g.mpc_set_shift(SH.ZERO if i == 4 else SH.REPEAT, capi.SHIFT_DUALS)
                g.set_warm_start(modes[i])
        for step in range(4):
            xs = [c["x0s"][step + i] for i in range(5)]
            t0s = [step if t else -1 for t in track]
            real = [0, 0, step % 2, (step + 1) % 2, 1]
            for i in range(5):
                if modes[i] == 2:
                    members[i].mpc_set_realised(real[i]); alone[i].mpc_set_realised(real[i])
            res, u0s = capi.mpc_step_batch(members, xs, t0s=t0s, **c["opts"])
            for i in range(5):
                ra, ua = alone[i].mpc_step(xs[i], **(dict(t0=t0s[i]) if track[i] else {}), **c["opts"])
                for k in COUNTS:
                    assert res[i][k] == ra[k], f"step {step} member {i}: {k}"
                _same_bits(u0s[i], ua, f"step {step} member {i}: u0")
                sm, sa = members[i].solution(), alone[i].solution()
                for k in SOL_KEYS:
                    _same_bits(sm[k], sa[k], f"step {step} member {i}: {k}")
        # the members took different starts: mode 1 and mode 2 differ, and so do the two realisations
        lams = [m.solution()["lam"] for m in members]
        print("batch: members' last duals differ pairwise by", [f"{np.max(np.abs(lams[i] - lams[2])):.2e}" for i in range(5)])
    finally:
        for g in members + alone:
            g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals, and what survives an upload
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(capi, rc, code, text):
    assert rc == code, f"{rc} != {code}: {capi.lib().tqgpu_last_error().decode()}"
    assert text in capi.lib().tqgpu_last_error().decode(), capi.lib().tqgpu_last_error().decode()


def test_refusals_and_survival(capi):
    L = capi.lib()
    c = R.case("single_wg")
    g = R.make(capi, c, root_states=True)
    try:
        _refused(capi, L.tqgpu_set_warm_start(g.h, 2), -2, "tqgpu_mpc_set_shift")
        _refused(capi, L.tqgpu_mpc_set_shift(g.h, 2, C.c_uint(1)), -2, "leaf")
        _refused(capi, L.tqgpu_mpc_set_shift(g.h, 0, C.c_uint(4)), -2, "what")
        _refused(capi, L.tqgpu_mpc_set_shift(g.h, 0, C.c_uint(2)), -2, "TQGPU_SHIFT_DUALS")
        g.mpc_set_shift(SH.ZERO, capi.SHIFT_DUALS | capi.SHIFT_WORKING_SETS)
        _refused(capi, L.tqgpu_mpc_set_realised(g.h, int(c["d"]["nk"][0])), -2, "children")
        _refused(capi, L.tqgpu_mpc_set_realised(g.h, -1), -2, "children")
        g.mpc_set_realised(1).set_warm_start(2)
        assert g.mpc_shift_state == dict(leaf=SH.ZERO, what=3, realised=1) and g.warm_start == 2
        # the mode and the maps survive tqgpu_set_problem
        d = R.with_x0(c, c["x0"] * 1.01)
        R.host_upload(capi, g, c, d)
        assert g.mpc_shift_state == dict(leaf=SH.ZERO, what=3, realised=1) and g.warm_start == 2
        r, _ = g.mpc_step(c["x0"], **c["opts"]); r, _ = g.mpc_step(c["x0"], **c["opts"])
        assert r["status"] == 0
        g.mpc_set_shift(0, 0)
        assert g.warm_start == 1 and g.mpc_shift_state["what"] == 0
        _refused(capi, L.tqgpu_mpc_shift(g.h), -2, "tqgpu_mpc_set_shift")
    finally:
        g.close()
    # ... and tqgpu_set_constraints with unchanged nc: the loop goes on as the twin's, which never saw the call
    cw = ws_case()
    a, b = K.make(capi, cw), K.make(capi, cw)
    try:
        d = cw["d"]
        for g in (a, b):
            g.mpc_set_shift(SH.REPEAT, capi.SHIFT_DUALS | capi.SHIFT_WORKING_SETS).set_warm_start(2)
        for step in range(4):
            if step == 2:
                a.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
                assert a.warm_start == 2 and a.mpc_shift_state["what"] == 3
            for g in (a, b):
                g.mpc_set_realised(step % 2)
            ra, ua = a.mpc_step(cw["x0s"][step], t0=step, **cw["opts"])
            rb, ub = b.mpc_step(cw["x0s"][step], t0=step, **cw["opts"])
            assert ra["status"] == 0 == rb["status"]
            H.assert_solution_close(a.solution(), b.solution(), tol=1e-6, keys=("x", "u"))          # (the same QP, both converged; the call may have emptied a's sets)
    finally:
        a.close(); b.close()
    # a rank of a sharded solve
    mk = SC._lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05))
    ranks = [mk(capi) for _ in range(2)]
    try:
        for i, m in enumerate(ranks):
            m.pshard_init(i, 2)
        m = ranks[1]
        w = np.zeros(len(m.nk), dtype=np.uint64)
        p = w.ctypes.data_as(C.POINTER(C.c_uint64))
        v = C.c_int(7)
        for rc in (L.tqgpu_mpc_set_shift(m.h, 0, C.c_uint(1)), L.tqgpu_mpc_set_realised(m.h, 0), L.tqgpu_mpc_get_shift(m.h, C.byref(v), None, None),
                   L.tqgpu_mpc_shift(m.h), L.tqgpu_get_working_sets(m.h, p, p, p, p), L.tqgpu_set_working_sets(m.h, p, p, p, p)):
            _refused(capi, rc, -4, "sharded")
        assert v.value == 7
    finally:
        for m in ranks:
            m.close()

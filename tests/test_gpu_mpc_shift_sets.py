"""The in-place shift of the stored working sets on the device (mpc_shift_sets, block nk0 of k_mpc_pre / k_mpc_pre_batch) on the trees of
shift_set_cases.py: more than one chunk of 64 nodes, two realisations, both leaf policies, every refusal rule of the gather, a tree without
rows.  The words that move are injected through tqgpu_set_working_sets, so a node and its image never hold the same words and a wrong
source shows; the reference is shift_cases.gather_sets, out of place.  Every comparison is bit for bit.

1. the gather alone, on every row, realisation and leaf policy; TQGPU_SHIFT_DUALS alone moves no set;
2. two shifts ahead of one solve: the sets compose, the duals do not (their source is the last solve's duals, which a shift does not touch);
3. the same launch moves the duals of a tree whose sum_nx lies beyond one warm span, and the solve behind it is the twin's;
4. members of a batch step with sets, each against its own single-step twin, and the counts of a batch with and without sets;
5. the rules on what the device holds after tqgpu_set_objective_mixed changed kinds and tqgpu_set_constraints changed nc.
6. a foreign set is only a worse guess: the stage solvers of kinds 3 and 2 are handed twelve in-range sets that are none of their node's
   (shift_set_cases.foreign_set) ahead of a whole solve, and the solve is the cold mirror's bit for bit.

What tqgpu_get_working_sets cannot show: the words of nodes of kinds 0 and 1 (read as 0 whatever the device holds) and the row words of
nodes of kind 2.  A kernel that wrote them would pass here; nothing reads them either."""
from __future__ import annotations

import numpy as np
import pytest

import shift_cases as SH
import shift_set_cases as SS

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")
COUNTS = ("status", "iter", "ls_total")


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _same_sets(a, b, what):
    for key in SS.WS_KEYS:
        bad = np.flatnonzero(a[key] != b[key])
        assert not len(bad), f"{what}: {key} differs at nodes {bad[:8]} ({len(bad)} in all): {[hex(int(v)) for v in a[key][bad[:4]]]} != {[hex(int(v)) for v in b[key][bad[:4]]]}"


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _same_solve(c, what, ra, a, rb, b):
    for k in COUNTS:
        assert ra[k] == rb[k], f"{what}: {k} {ra[k]} != {rb[k]}"
    sa, sb = a.solution(), b.solution()
    for k in SOL_KEYS + (("mu_d",) if "nc" in c["d"] else ()):
        _same_bits(sa[k], sb[k], f"{what}: {k}")
    _same_sets(a.working_sets(), b.working_sets(), what)
    na, nb = a.stage_steps()["total"], b.stage_steps()["total"]
    assert np.array_equal(na, nb), f"{what}: stage steps {na.sum()} != {nb.sum()}"


def _first_solve(g, c, **opts):
    g.mpc_set_x0(c["x0s"][0])
    return g.solve(**{**c["opts"], **opts})


def _both(gpu):
    return gpu.SHIFT_DUALS | gpu.SHIFT_WORKING_SETS


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the gather alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SS.ROW_IDS)
def test_gather_alone(gpu, cid):
    c = SS.case(cid)
    t = c["tree"]
    g = SS.make(gpu, c)
    try:
        _first_solve(g, c, maxIter=1)          # (tqgpu_mpc_shift refuses before the first solve; the first solve also empties the sets of the kind-3 nodes)
        for j in SS.realisations(t):
            for leaf in SS.POLICIES:
                ws = SS.inject(t, j)
                what = f"{cid} realisation {j} leaf {leaf}"
                g.set_working_sets(**ws)
                _same_sets(g.working_sets(), ws, what + ": set / get round trip")
                g.mpc_set_shift(leaf, _both(gpu)).mpc_set_realised(j)
                g.mpc_shift()
                got, want = g.working_sets(), SS.gathered(t, ws, j, leaf)
                _same_sets(got, want, what)
                moved = sum(int(np.count_nonzero(want[k] != ws[k])) for k in SS.WS_KEYS)
                assert moved, what + ": no word moves"
                if cid == "box_only":
                    assert not got["bound_sides"].any() and not got["row_sides"].any() and not got["rows"].any()
                g.set_working_sets(**ws)
                g.mpc_set_shift(leaf, gpu.SHIFT_DUALS).mpc_set_realised(j)
                g.mpc_shift()
                _same_sets(g.working_sets(), ws, what + ": TQGPU_SHIFT_DUALS alone")
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. two shifts ahead of one solve
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,j", [("chain65", 0), ("bin127", 1)])
def test_two_shifts_ahead_of_one_solve(gpu, cid, j):
    """the sets are shifted twice (the gather of the gather: the kernel reads what the first shift stored); the duals once: every shift
    gathers from the duals of the last SOLVE into the start buffer, so the second shift writes what the first wrote.  The twin gets
    gather_lam once and the sets gathered twice, and solves to the same bits."""
    c = SS.case(cid)
    t, d = c["tree"], c["d"]
    a, b = SS.make(gpu, c), SS.make(gpu, c)
    try:
        ra, rb = _first_solve(a, c), _first_solve(b, c)
        _same_solve(c, f"{cid}: first solve", ra, a, rb, b)
        ws = SS.inject(t, 3)
        once = SS.gathered(t, ws, j, SH.REPEAT)
        twice = SS.gathered(t, once, j, SH.REPEAT)
        assert any(np.any(once[k] != twice[k]) for k in SS.WS_KEYS), "the second gather moves nothing"
        a.set_working_sets(**ws)
        a.mpc_set_shift(SH.REPEAT, _both(gpu)).mpc_set_realised(j)
        a.mpc_shift(); a.mpc_shift()
        _same_sets(a.working_sets(), twice, f"{cid}: two shifts")
        lam = b.solution()["lam"]
        img = SH.ref_map(d["nk"], d["nx"], j, SH.REPEAT)[0]
        start = SH.gather_lam(d["nx"], img, lam)
        assert not np.array_equal(SH.gather_lam(d["nx"], img, start), start), "the duals gathered twice are the duals gathered once"
        b.set_lambda(start)
        b.set_working_sets(**twice)
        ra, rb = a.solve(**c["opts"]), b.solve(**c["opts"])
        print(f"{cid}: the solve behind two shifts {[ra[k] for k in COUNTS]}, behind set_lambda(gathered once) {[rb[k] for k in COUNTS]}")
        _same_solve(c, f"{cid}: the solve behind two shifts", ra, a, rb, b)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the same launch also moves the duals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,j,leaf", [("chain129_nx4", 0, SH.REPEAT), ("bin255", 1, SH.ZERO)])
def test_shift_moves_duals_and_sets_in_one_launch(gpu, cid, j, leaf):
    c = SS.case(cid)
    t, d = c["tree"], c["d"]
    assert int(np.sum(d["nx"])) > 512, "sum_nx within one warm span"
    a, b = SS.make(gpu, c), SS.make(gpu, c)
    try:
        ra, rb = _first_solve(a, c), _first_solve(b, c)
        _same_solve(c, f"{cid}: first solve", ra, a, rb, b)
        ws = SS.inject(t, 5)
        a.set_working_sets(**ws)
        a.mpc_set_shift(leaf, _both(gpu)).mpc_set_realised(j)
        a.mpc_shift()
        lam = b.solution()["lam"]
        start = SH.gather_lam(d["nx"], SH.ref_map(d["nk"], d["nx"], j, leaf)[0], lam)
        assert not np.array_equal(start, lam)
        b.set_lambda(start)
        b.set_working_sets(**SS.gathered(t, ws, j, leaf))
        ra, rb = a.solve(**c["opts"]), b.solve(**c["opts"])
        print(f"{cid}: the solve behind the shift {[ra[k] for k in COUNTS]} stage steps {a.stage_steps()['total'].sum()}, the twin's {[rb[k] for k in COUNTS]} {b.stage_steps()['total'].sum()}")
        _same_solve(c, f"{cid}: the solve behind the shift", ra, a, rb, b)
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the batch step
# ---------------------------------------------------------------------------------------------------------------------------------
def _clipping_case():
    import mpc_root_cases as R
    c = dict(R.case("single_wg"))
    c["x0s"] = R.x0_sequence(c, steps=8)
    return c


def test_batch_members_with_sets_equal_their_twins(gpu):
    """five members in one tqgpu_mpc_step_batch: two chains and a binary tree whose sets move (different realisations, both leaf policies),
    `rules` with TQGPU_SHIFT_DUALS alone, and a clipping tree in mode 2, whose node table is null.  Ahead of every step behind the first the
    stored sets of a member and of its twin are replaced by injected ones: what the step's solve starts from is then the gather of words
    that differ from node to node, and a member that gathered through another member's node table starts its stage solves elsewhere
    than its twin (the step counts and the sets it ends with are compared)."""
    both = _both(gpu)
    plan = [("chain65", SH.REPEAT, both), ("chain129", SH.REPEAT, both), ("bin127", SH.ZERO, both), ("rules", SH.REPEAT, gpu.SHIFT_DUALS), (None, SH.REPEAT, gpu.SHIFT_DUALS)]
    cs = [SS.case(cid) if cid else _clipping_case() for cid, _, _ in plan]
    mk = [(lambda c=c: SS.make(gpu, c)) for c in cs]
    members, alone = [m() for m in mk], [m() for m in mk]
    try:
        for i, (_, leaf, what) in enumerate(plan):
            for g in (members[i], alone[i]):
                g.mpc_set_shift(leaf, what).set_warm_start(2)
        for step in range(5):
            xs = [c["x0s"][step] for c in cs]
            for i, (cid, leaf, what) in enumerate(plan):
                real = (step + i) % max(int(cs[i]["d"]["nk"][0]), 1)
                for g in (members[i], alone[i]):
                    g.mpc_set_realised(real)
                    if step > 0 and cid:
                        g.set_working_sets(**SS.inject(cs[i]["tree"], 10 + step))
            res, u0s = gpu.mpc_step_batch(members, xs, **cs[0]["opts"])
            st = gpu.mpc_stats()
            for i, c in enumerate(cs):
                ra, ua = alone[i].mpc_step(xs[i], **cs[0]["opts"])
                what = f"step {step} member {i} ({plan[i][0]})"
                _same_bits(u0s[i], ua, what + ": u0")
                _same_solve(c, what, res[i], members[i], ra, alone[i])
            print(f"batch step {step}: {[[r[k] for k in COUNTS] for r in res]} stats {st}")
    finally:
        for g in members + alone:
            g.close()


def test_batch_costs_with_and_without_sets(gpu):
    """the sets ride in block nk0 of the launch that is there anyway.  Around the solves a batch step has one launch ahead (k_mpc_pre_batch) and
    one behind (the post of u[0]), with sets and without: the launches of tqgpu_mpc_stats less those the members' results count for their
    own solves are 2 either way.  (A dense tree is solved launch by launch, so the totals of a step hold the solves' launches and copies,
    which follow the iteration counts; they are compared only where both variants took the same iterations.)"""
    c = SS.case("chain65")
    seen = {}
    for what in (gpu.SHIFT_DUALS, _both(gpu)):
        members = [SS.make(gpu, c) for _ in range(3)]
        try:
            for m in members:
                m.mpc_set_shift(SH.REPEAT, what).set_warm_start(2)
            for step in range(3):
                res, _ = gpu.mpc_step_batch(members, [c["x0s"][step + i] for i in range(3)], **c["opts"])
                st = gpu.mpc_stats()
            seen[what] = (st, [[r[k] for k in COUNTS] for r in res], st["launches"] - sum(r["n_launches"] for r in res))
        finally:
            for m in members:
                m.close()
    print(f"batch of three chains, steady step: {seen}")
    (st_a, counts_a, around_a), (st_b, counts_b, around_b) = seen[gpu.SHIFT_DUALS], seen[_both(gpu)]
    assert around_a == 2 and around_b == 2, seen
    if counts_a == counts_b:
        assert st_a == st_b, seen


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the rules are applied to what the device holds
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rules_follow_new_kinds_and_new_nc(gpu):
    c = SS.case("rules")
    t, d = c["tree"], c["d"]
    img = SS.maps(t, 0, SH.REPEAT)[0]
    tb, tr = SS.takes(t, 0, SH.REPEAT)
    # a kind-3 node that takes rows becomes kind 1; a kind-2 node that is the image of a kind-3 node with the same nc becomes kind 3
    to1 = int(next(k for k in np.flatnonzero(tr) if k > 0))
    to3 = int(next(img[k] for k in range(1, len(img)) if img[k] >= 0 and t["kinds"][k] == 3 and t["kinds"][img[k]] == 2 and t["nc"][k] == t["nc"][img[k]] and tb[k] and img[k] != to1))
    kinds2 = t["kinds"].copy()
    kinds2[to1], kinds2[to3] = 1, 3
    t2 = SS.with_tree(t, kinds=kinds2)
    # then the rows of one kind-3 node that takes rows under the new kinds go from two to one
    tr2 = SS.takes(t2, 0, SH.REPEAT)[1]
    fewer = int(next(k for k in np.flatnonzero(tr2) if k > 0 and t2["nc"][k] == 2))
    nc3 = t2["nc"].copy()
    nc3[fewer] = 1
    t3 = SS.with_tree(t2, nc=nc3)
    g = SS.make(gpu, c)
    try:
        _first_solve(g, c, maxIter=1)
        g.mpc_set_shift(SH.REPEAT, _both(gpu)).mpc_set_realised(0)
        state = g.mpc_shift_state
        for tree, name in ((t, "as created"), (t2, f"node {to1} of kind 1, node {to3} of kind 3"), (t3, f"nc[{fewer}] = 1")):
            if tree is t2:
                g.upload_mixed(d, kinds2, None)
            if tree is t3:
                d3 = SS.rows_data({}, t3)
                g.set_constraints(d3["nc"], d3["C"], d3["D"], d3["dmin"], d3["dmax"])
            assert g.mpc_shift_state == state, name
            ws = SS.inject(tree, 7)
            g.set_working_sets(**ws)
            _same_sets(g.working_sets(), ws, f"rules, {name}: set / get round trip")
            g.mpc_shift()
            want = SS.gathered(tree, ws, 0, SH.REPEAT)
            _same_sets(g.working_sets(), want, f"rules, {name}")
            if tree is not t:
                old = SS.gathered(t if tree is t2 else t2, ws, 0, SH.REPEAT)
                assert any(np.any(old[k] != want[k]) for k in SS.WS_KEYS), f"rules, {name}: the rule before the change gives the same words"
            assert g.mpc_shift_state == state, name
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. a foreign set is only a worse guess
# ---------------------------------------------------------------------------------------------------------------------------------
def _foreign_mirror(gpu, fc, hot):
    d = fc["d"]
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if "nc" in d:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    g.upload_mixed(d, fc["kinds"], fc["start"])
    if not hot and "nc" in d:
        g.set_gen_hot_start(False)
    return g


@pytest.mark.parametrize("fid", SS.FOREIGN_IDS)
def test_a_foreign_set_is_only_a_worse_guess(gpu, fid):
    """A hot mirror and a cold one (tqgpu_set_gen_hot_start off) solve the row from its clear start; ahead of each solve the hot mirror is
    given one of the twelve sets of shift_set_cases.FOREIGN_KINDS through tqgpu_set_working_sets.  Counts, x, u, lam, every multiplier and
    the final working sets must be the cold mirror's bit for bit (DESIGN, Determinism, under the guards of gen_cases), and no stage solve
    may exceed the step cap (the pass from the given set and one cold redo).  test_shift_set_reference.py has run every pair through the
    numpy model first.

    Kind 2 (stage_box) does consult its stored set, but only as a filter: an entry starts fixed where its bit is set AND its last value
    still sits on that bound; it has no cold switch.  So on the box rows, and on the kind-2 nodes of gen-mixed, the claim is that an injected
    set changes nothing against a mirror that keeps its own sets; both mirrors make the same solves, so their last values agree.  The sides
    of a kind-2 node are no input of stage_box at all; it stores those of its final set (where the tree has rows) for the kind-3 node that a
    shift may hand them to, and this test is what holds it to that: before, the injected sides came back unchanged."""
    fc = SS.foreign_case(fid)
    d = fc["d"]
    keys = SOL_KEYS + (("mu_d",) if "nc" in d else ())
    cap = SS.step_cap(fc)
    hot, cold = _foreign_mirror(gpu, fc, True), _foreign_mirror(gpu, fc, False)
    try:
        # the first solve runs k_dense_init, which empties the sets of the kind-3 nodes: sets are given behind it
        r0h, r0c = hot.solve(**SS.FOREIGN_OPTS), cold.solve(**SS.FOREIGN_OPTS)
        assert r0c["status"] == 0 and [r0h[k] for k in COUNTS] == [r0c[k] for k in COUNTS]
        cold_ws = cold.working_sets()
        _same_sets(hot.working_sets(), cold_ws, f"{fid}: first solve")
        for kind in SS.FOREIGN_KINDS:
            ws = SS.foreign_set(fc, kind, cold_ws)
            for g in (hot, cold):
                g.set_lambda(fc["start"])
            hot.set_working_sets(**ws)
            _same_sets(hot.working_sets(), ws, f"{fid} {kind}: set / get round trip")
            rh, rc = hot.solve(**SS.FOREIGN_OPTS), cold.solve(**SS.FOREIGN_OPTS)
            nh, ncold = hot.stage_steps(), cold.stage_steps()
            print(f"{fid} {kind}: {[rh[k] for k in COUNTS]} (cold {[rc[k] for k in COUNTS]}) stage steps hot {int(nh['total'].sum())} cold {int(ncold['total'].sum())}")
            what = f"{fid} {kind}"
            for k in COUNTS:
                assert rh[k] == rc[k], f"{what}: {k} {rh[k]} != {rc[k]}"
            assert rc["status"] == 0, what
            sh, sc = hot.solution(), cold.solution()
            for k in keys:
                _same_bits(sh[k], sc[k], f"{what}: {k}")
            _same_sets(hot.working_sets(), cold.working_sets(), what)
            _same_sets(cold.working_sets(), cold_ws, what + ": the cold mirror's own sets")
            sweeps = 2 + rh["iter"] + rh["ls_total"]          # one at the start, one per trial, at most one more behind the last
            assert np.all(nh["last"] <= cap) and np.all(nh["total"] <= sweeps * cap), f"{what}: steps {nh} beyond the cap {cap}"
    finally:
        hot.close(); cold.close()

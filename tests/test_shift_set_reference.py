"""The rows of shift_set_cases.py meet their own descriptions, checked without a device: where the images lie relative to the chunks of 64
nodes that mpc_shift_sets walks, which refusal rule of the gather each node of `rules` meets alone, the host map against the walk of
paths, img(k) > k wherever a set is taken, and the numpy simulations of the kernel's in-place walk: the ascending walk with a chunk's loads
ahead of its stores is the out-of-place gather on every row, the descending walk and the walk that stores lane by lane are not, wherever
the tree lets them differ -- so the injected words make the three clauses of the kernel's comment observable on the device
(test_gpu_mpc_shift_sets.py).

Where the walks can differ is a property of the tree, worked out here and asserted as an equivalence:
  descending    differs iff some node that takes a set has its image in a LATER chunk and that image takes a set itself (the image is stored
                first and read afterwards).  The chains of more than 64 inner nodes and `rules` have such nodes.  The binary trees do not: the
                images of a level are the next level, the deepest inner level takes nothing (its images are leaves, whose nu differs), and
                that level alone fills the chunks behind the first.  A descending walk is invisible on them, on any device.
  lane by lane  (lanes descending) differs iff some node that takes a set has its image in the SAME chunk and that image takes a set itself:
                every row."""
from __future__ import annotations

import numpy as np
import pytest

import shift_cases as SH
import shift_set_cases as SS

ALL_IDS = SS.ROW_IDS + SS.EXTRA_IDS


def _combos(t):
    return [(j, leaf) for j in SS.realisations(t) for leaf in SS.POLICIES]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in SS.WS_KEYS)


def _chunks_ahead(t, j, leaf):
    """(among the nodes that take a set, among all entries of the node table): nodes whose image lies 0, 1, >= 2 chunks ahead"""
    tb, _ = SS.takes(t, j, leaf)
    tab = SS.node_table(t, j, leaf)
    out = []
    for ks in (np.flatnonzero(tb), np.flatnonzero(tab >= 0)):
        d = tab[ks] // SS.WAVE - ks // SS.WAVE
        out.append((int(np.sum(d == 0)), int(np.sum(d == 1)), int(np.sum(d >= 2))))
    return out


def _alone(t, j, leaf):
    """reason -> (nodes below 64, nodes from 64 on) refused for that reason alone"""
    cnt = {}
    for k, why in enumerate(SS.refusals(t, j, leaf)):
        if len(why) == 1:
            c = cnt.setdefault(next(iter(why)), [0, 0])
            c[int(k >= SS.WAVE)] += 1
    return cnt


@pytest.mark.parametrize("cid", SS.ROW_IDS)
def test_row_meets_its_description(cid):
    t = SS.tree(cid)
    n = len(t["nk"])
    sizes = dict(chain64=64, chain65=65, chain128=128, chain129=129, bin127=127, bin255=255, bin_pad128=128, box_only=66)
    assert n == sizes.get(cid, n) and (cid != "rules" or n >= 70)
    total, far = {}, 0
    for j, leaf in _combos(t):
        takers, table = _chunks_ahead(t, j, leaf)
        alone = _alone(t, j, leaf)
        print(f"{cid} Nn {n} realisation {j} leaf {leaf}: images same / next / >= 2 chunks ahead: takers {takers}, node table {table}; refused alone (k < 64, k >= 64) {alone}")
        for why, c in alone.items():
            a = total.setdefault(why, [0, 0])
            a[0] += c[0]; a[1] += c[1]
        if cid in SS.CHAIN_IDS:
            assert takers[0] >= 1 and takers[1] == (1 if n > 65 else 0) and alone.get("nu") is not None          # (the last inner node: its image is the leaf)
            if n == 65:
                assert table[1] == 1 and takers[1] == 0          # node 63 reads node 64 (nu differs: nothing moves) -- the ragged chunk of one node
        if cid in SS.BIN_IDS:
            assert takers[0] >= 1 and len(SS.realisations(t)) == 2
            if cid == "bin255":
                assert takers[1] >= 1 and table[1] >= 1
                far += table[2]
            else:
                assert table[1] >= 1
        if cid == "box_only":
            assert takers[0] >= 60 and not np.any(t["nc"]) and np.all(t["kinds"] == 2) and len(SS.realisations(t)) == 2
    assert n % SS.WAVE == dict(chain64=0, chain65=1, chain128=0, chain129=1, bin127=63, bin255=63, bin_pad128=0, box_only=2).get(cid, n % SS.WAVE)
    if cid == "bin255":
        assert far >= 1, "no entry of a node table lies two chunks ahead"          # (realisation 1: node 63 reads node 191)
    if cid == "rules":
        assert set(t["kinds"].tolist()) == {0, 1, 2, 3} and len(set(t["nx"].tolist())) == 2
        dep = SH.depths(t["nk"])
        assert len(set(dep[t["nk"] == 0].tolist())) >= 2, "leaves at one depth only"
        for why in ("kind", "nu", "nc", "rows_kind", "none"):
            assert total.get(why, [0, 0])[0] >= 1 and total[why][1] >= 1, f"rules: no node on either side of lane 63 is refused for `{why}` alone: {total}"
        # a repeated leaf: the nodes it is the image of are leaves, and tqgpu_create wants every parent numbered ahead of every leaf: in a tree
        # whose parents reach beyond node 63 (the other rules need that) no leaf lies below node 64
        assert total["rep"] == [0, total["rep"][1]] and total["rep"][1] >= 1
        # the three rules that the mutations of the kernel's comparisons need, under one realisation and the policy REPEAT
        a = _alone(t, 0, SH.REPEAT)
        for why in ("kind", "nu", "nc", "rows_kind"):
            assert a[why][0] >= 1 and a[why][1] >= 1, (why, a)
        # kinds 3 <- 2 with equal nc: only the kind keeps the rows where they are
        img, _ = SS.maps(t, 0, SH.REPEAT)
        assert any(t["kinds"][k] == 3 and t["kinds"][img[k]] == 2 and t["nc"][k] == t["nc"][img[k]] > 0 and "rows_kind" in w
                   for k, w in enumerate(SS.refusals(t, 0, SH.REPEAT)) if img[k] >= 0)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_host_map_is_the_walk_of_paths_and_images_lie_beyond(capi, cid):
    t = SS.tree(cid)
    for j, leaf in _combos(t):
        want, rep = SS.maps(t, j, leaf)
        assert np.array_equal(capi.shift_map(t["nk"], t["nx"], j, leaf), want), f"{cid} realisation {j} leaf {leaf}"
        tb, tr = SS.takes(t, j, leaf)
        assert np.all(want[tb] > np.flatnonzero(tb)) and not np.any(tr & ~tb)
        assert np.array_equal(SS.node_table(t, j, leaf)[tb], want[tb])
        # the rule written out in takes() is the rule of shift_cases.gather_sets: the two gathers move the same words
        ws = SS.inject(t, 1)
        ref = SS.gathered(t, ws, j, leaf)
        moved = np.zeros(len(want), bool)
        for key in SS.WS_KEYS:
            moved |= ref[key] != ws[key]
        assert np.array_equal(moved, tb), f"{cid} realisation {j} leaf {leaf}: the injected words do not show every node that takes a set"


@pytest.mark.parametrize("cid", ALL_IDS)
def test_injected_words_are_in_range_and_tell_a_node_from_its_image(cid):
    t = SS.tree(cid)
    for seed in (0, 1):
        ws = SS.inject(t, seed)
        nz, nc = (t["nx"] + t["nu"]).astype(np.uint64), t["nc"].astype(np.uint64)
        assert np.all(ws["bounds"] >> nz == 0) and np.all(ws["rows"] >> nc == 0)
        assert not np.any(ws["bound_sides"] & ~ws["bounds"]) and not np.any(ws["row_sides"] & ~ws["rows"])
        assert not np.any(ws["bounds"][t["kinds"] < 2]) and not np.any(ws["rows"][t["kinds"] != 3])
        for j, leaf in _combos(t):
            img, _ = SS.maps(t, j, leaf)
            tb, tr = SS.takes(t, j, leaf)
            for k in np.flatnonzero(tb):
                assert (ws["bounds"][k], ws["bound_sides"][k]) != (ws["bounds"][img[k]], ws["bound_sides"][img[k]])
            for k in np.flatnonzero(tr):
                assert (ws["rows"][k], ws["row_sides"][k]) != (ws["rows"][img[k]], ws["row_sides"][img[k]])
    assert not _same(SS.inject(t, 0), SS.inject(t, 1))
    if cid == "box_only":
        assert not ws["bound_sides"].any() and not ws["rows"].any() and not ws["row_sides"].any()


def _visible(t, j, leaf):
    """(descending, lane by lane): can the walk differ from the gather on this tree?  (module docstring)"""
    tb, _ = SS.takes(t, j, leaf)
    tab = SS.node_table(t, j, leaf)
    ks = np.flatnonzero(tb)
    later = [k for k in ks if tab[k] // SS.WAVE > k // SS.WAVE and tb[tab[k]]]
    same = [k for k in ks if tab[k] // SS.WAVE == k // SS.WAVE and tb[tab[k]]]
    return bool(later), bool(same)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_in_place_walks(cid):
    t = SS.tree(cid)
    seen = [False, False]
    for j, leaf in _combos(t):
        ws = SS.inject(t, 0)
        tab = SS.node_table(t, j, leaf)
        ref = SS.gathered(t, ws, j, leaf)
        assert _same(SS.walk_in_place(t, ws, tab, "ascending"), ref), f"{cid} realisation {j} leaf {leaf}: the kernel's walk is not the gather"
        assert _same(SS.walk_in_place_lanes(t, ws, tab, loads_first=True), ref)
        desc = not _same(SS.walk_in_place(t, ws, tab, "descending"), ref)
        lanes = not _same(SS.walk_in_place_lanes(t, ws, tab, loads_first=False), ref)
        can_desc, can_lanes = _visible(t, j, leaf)
        print(f"{cid} realisation {j} leaf {leaf}: a descending walk differs: {desc} (can: {can_desc}), stores ahead of loads differ: {lanes} (can: {can_lanes})")
        assert desc == can_desc and lanes == can_lanes
        seen[0] |= desc; seen[1] |= lanes
    assert seen[1], f"{cid}: a store ahead of the chunk's loads is invisible"
    if cid in ("chain128", "chain129", "chain129_nx4", "rules"):
        assert seen[0], f"{cid}: a descending walk is invisible"
    if cid in ("chain64", "chain65") + SS.BIN_IDS + ("box_only",):
        assert not seen[0]          # one chunk, a second chunk of one leaf, or chunks behind the first that take nothing (module docstring)


def test_the_wrong_realisation_is_visible_beyond_node_63():
    """a gather through the node table of realisation 0 where realisation 1 is in force differs beyond node 63 on the trees whose nodes beyond 63 take
    sets (rules; on the binary trees the nodes from 63 on are the deepest inner level, whose images are leaves of another nu, and the
    leaves), and below node 64 on every tree with two realisations"""
    for cid in SS.BIN_IDS:
        t = SS.tree(cid)
        ws = SS.inject(t, 0)
        a, b = SS.gathered(t, ws, 0, SH.REPEAT), SS.gathered(t, ws, 1, SH.REPEAT)
        assert any(np.any(a[k] != b[k]) for k in SS.WS_KEYS), cid
    for cid in ("rules",):
        t = SS.tree(cid)
        ws = SS.inject(t, 0)
        a, b = SS.gathered(t, ws, 0, SH.REPEAT), SS.gathered(t, ws, 1, SH.REPEAT)
        assert any(np.any(a[k][SS.WAVE:] != b[k][SS.WAVE:]) for k in SS.WS_KEYS), cid


# ---------------------------------------------------------------------------------------------------------------------------------
# foreign sets for the stage solvers, on the numpy model (gen_hot_ref.solve_gen_from) ahead of the device
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_list_of_rows_with_a_qualifying_whole_solve():
    import gen_cases as GC
    ok = []
    for rid in GC.FULL_IDS + [r for r in ("one_row", "row_and_bound", "more_rows_than_vars", "equality_row", "swap", "nz64", "nc64") if r not in GC.FULL_IDS]:
        c = GC.case(rid)
        try:
            GC.clear_start(c["d"], c["kinds"])
            ok.append(rid)
        except AssertionError:
            pass
    assert tuple(ok) == SS.FOREIGN_GEN_IDS, ok
    assert len(SS.FOREIGN_BOX_IDS) == 2 and len(SS.FOREIGN_KINDS) == 12


@pytest.mark.parametrize("fid", SS.FOREIGN_IDS)
def test_every_foreign_set_ends_on_the_cold_set_in_the_model(fid):
    """every (row, set) pair that the device gets: from the stage QPs of the first sweep the numpy model ends on the cold solve's sets and
    sides whatever in-range set it starts from, within the step cap.  A pair that did not (a degenerate draw) would get another seed in
    shift_set_cases.FOREIGN_SEEDS; no pair is left out."""
    fc = SS.foreign_case(fid)
    cold, cold_steps = SS.model_first_sweep(fc)
    cap = SS.step_cap(fc)
    assert any(fc["kinds"] >= 2) and cold_steps
    seen = set()
    for kind in SS.FOREIGN_KINDS:
        ws = SS.foreign_set(fc, kind, cold)
        nz, nc = fc["nz"].astype(np.uint64), np.where(fc["kinds"] == 3, fc["nc"], 0).astype(np.uint64)
        in_range = lambda w, n: np.all(np.where(n >= 64, 0, w >> np.minimum(n, 63)) == 0)
        assert in_range(ws["bounds"], nz) and in_range(ws["rows"], nc), f"{fid} {kind}: bits out of range"
        assert not np.any(ws["bound_sides"] & ~ws["bounds"]) and not np.any(ws["row_sides"] & ~ws["rows"])
        assert not np.any(ws["bounds"][fc["kinds"] < 2]) and not np.any(ws["rows"][fc["kinds"] != 3])
        got, steps = SS.model_first_sweep(fc, ws)
        print(f"{fid} {kind}: model steps {sum(steps.values())} (cold {sum(cold_steps.values())})")
        assert _same(got, cold), f"{fid} {kind}: the model does not end on the cold set: replace the seed (shift_set_cases.FOREIGN_SEEDS)"
        assert all(steps[k] <= cap[k] for k in steps)
        seen.add(tuple(int(v) for key in SS.WS_KEYS for v in ws[key]))
    assert len(seen) >= 11, f"{fid}: the sets are not different sets"          # (sides_flipped of an empty cold set is the empty set)
    ws = SS.foreign_set(fc, "all_bits", cold)
    assert all(int(ws["bounds"][k]) == (1 << int(fc["nz"][k])) - 1 for k in np.flatnonzero(fc["kinds"] >= 2))
    comp = SS.foreign_set(fc, "complement", cold)
    assert not np.any(comp["bounds"] & cold["bounds"]) and not np.any(comp["rows"] & cold["rows"])
    flip = SS.foreign_set(fc, "sides_flipped", cold)
    assert np.array_equal(flip["bounds"], cold["bounds"]) and not np.any(flip["bound_sides"] & cold["bound_sides"]) and not np.any(flip["row_sides"] & cold["row_sides"])

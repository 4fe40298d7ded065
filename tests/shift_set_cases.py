"""Trees, injected working sets and numpy walks for the in-place shift of the stored working sets (mpc_shift_sets, block nk0 of k_mpc_pre /
k_mpc_pre_batch), shared by test_shift_set_reference.py (what every row is about, without a device) and test_gpu_mpc_shift_sets.py.

The kernel has no scratch copy and no atomics.  It is right because (1) every node that takes a set has img(k) > k, (2) ONE wave walks the
nodes in ascending chunks of 64 and (3) all loads of a chunk complete before any of its stores.  The rows below are the trees on which each
clause can be seen to fail: more than one chunk, images in the same chunk, in the next and further ahead, a full and a ragged last chunk,
two realisations, every refusal rule of the gather on both sides of lane 63, and a tree without rows (rmask == sides == nullptr).

    chain64 .. chain129   a chain, nx = 3, nu = 2, two rows on every inner node (kind 3), the leaf of kind 2: img(k) = k + 1
    chain129_nx4          chain129 with nx = 4, nu = 1: sum_nx = 516 lies beyond one warm span of 512 doubles (the duals' blocks)
    bin127, bin255        shift_cases.uniform(2, 6) / (2, 7), the children alternate between kind 3 (two rows) and kind 2
    bin_pad128            bin127 with a third leaf below its last inner node: the last chunk is exactly full
    rules                 two chains A, B of 46 and 45 levels below the root; kinds 0 .. 3, nu 1 | 2 and nc 1 | 2 vary with the level, two
                          nodes of B have nx = 4 (_rules_tree)
    box_only              66 nodes of kind 2 in two chains of 33 and 32 levels, no rows anywhere: the tree has no row words at all

`tree(cid)` is topology only (nk, nx, nu, nc, kinds); `case(cid)` adds the problem data (helpers.dense_shaped_qp, as ws_case of
test_gpu_mpc_shift.py).  Importing this module must not load the native library (the rule of adj_cases.py): the case modules are imported
where a case is built."""
from __future__ import annotations

import functools

import numpy as np

import shift_cases as SH

WAVE = 64
WS_KEYS = ("bounds", "rows", "bound_sides", "row_sides")
CHAIN_IDS = ("chain64", "chain65", "chain128", "chain129")
BIN_IDS = ("bin127", "bin255", "bin_pad128")
ROW_IDS = CHAIN_IDS + BIN_IDS + ("rules", "box_only")
EXTRA_IDS = ("chain129_nx4",)          # not a row of its own: chain129 for the test of the duals' blocks
POLICIES = (SH.REPEAT, SH.ZERO)
SPAN = 0.5          # every row within +- SPAN: wide enough for every stage QP to stay feasible, tight enough for rows to be active


def _i32(v):
    return np.asarray(v, dtype=np.int32)


def _chain(n, nx=3, nu=2):
    nk = _i32([1] * (n - 1) + [0])
    kinds = _i32([3] * (n - 1) + [2])
    return dict(nk=nk, nx=np.full(n, nx, np.int32), nu=np.where(nk > 0, nu, 0).astype(np.int32), nc=np.where(nk > 0, 2, 0).astype(np.int32), kinds=kinds)


def _bin(depth, pad=False):
    nk = SH.uniform(2, depth).copy()
    if pad:
        nk[np.flatnonzero(nk > 0)[-1]] = 3
        nk = np.append(nk, np.int32(0))          # the third leaf of the last inner node is the last node of its level
    n, k0 = int(nk.sum()) + 1, SH.kid0(nk)
    kinds = np.full(n, 3, np.int32)
    for p in range(len(nk)):
        for c in range(nk[p]):
            kinds[k0[p] + c] = 3 if c % 2 == 0 else 2
    return dict(nk=nk, nx=np.full(n, 3, np.int32), nu=np.where(nk > 0, 2, 0).astype(np.int32), nc=np.where(kinds == 3, 2, 0).astype(np.int32), kinds=kinds)


RULES_LEVELS = (46, 45)          # the last levels of chains A and B: leaves at two depths, and every parent numbered ahead of every leaf (tqgpu_create asks for that)
_A = dict(kind=(3, 3, 2, 3, 0, 3, 1, 2), nu1=(3,), nc1=(0,))          # by level % 8: the kind; the levels with nu = 1; with nc = 1
_B = dict(kind=(2, 3, 3, 1, 3, 2, 3, 0), nu1=(6,), nc1=(2,))
RULES_NX4 = (10, 40)             # the levels at which B has nx = 4: one on either side of lane 63


def _rules_tree():
    """node 0, then level l = (A_l, B_l) = nodes 2 l - 1, 2 l while both chains run.  Under realisation 0 every node of level l has the
    image A_(l + 1), under realisation 1 B_(l + 1).  The kinds, nu and nc follow the tables _A, _B with period 8 in the level, so every pair of (kind, nu, nc) of a
    node and its image that the tables allow is met below and beyond node 63 (level 32).  A node of kind 2 keeps the nc of the table: rows
    that its kind ignores, so that kinds 3 <- 2 meet with equal nc and only the kind refuses the rows."""
    la, lb = RULES_LEVELS
    nk, who = [2], [("R", 0)]
    for l in range(1, max(la, lb) + 1):
        for ch, last in (("A", la), ("B", lb)):
            if l <= last:
                nk.append(0 if l == last else 1)
                who.append((ch, l))
    n = len(nk)
    nk = _i32(nk)
    kinds, nx, nu, nc = np.zeros(n, np.int32), np.full(n, 3, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k, (ch, l) in enumerate(who):
        if ch == "R":
            kinds[k], nu[k], nc[k] = 3, 2, 2
        else:
            t = _A if ch == "A" else _B
            kinds[k] = t["kind"][l % 8]
            nu[k] = 0 if nk[k] == 0 else 1 if l % 8 in t["nu1"] else 2
            nc[k] = 0 if kinds[k] < 2 else 1 if l % 8 in t["nc1"] else 2
            if ch == "B" and l in RULES_NX4:
                nx[k] = 4
    # (a kind-3 node without rows would become a kind-2 node on the device, apply_kinds)
    assert np.all(nc[kinds == 3] > 0) and np.all((nk > 0) == (np.arange(n) < np.count_nonzero(nk)))
    return dict(nk=nk, nx=nx, nu=nu, nc=nc, kinds=kinds)


def _box_only():
    nk = [2] + [1, 1] * 31 + [1, 0] + [0]
    n = len(nk)
    assert n == 66
    nk = _i32(nk)
    return dict(nk=nk, nx=np.full(n, 3, np.int32), nu=np.where(nk > 0, 2, 0).astype(np.int32), nc=np.zeros(n, np.int32), kinds=np.full(n, 2, np.int32))


@functools.lru_cache(maxsize=None)
def tree(cid):
    """dict(nk, nx, nu, nc, kinds): the kinds are those the device ends up with (kind 3 only where nc > 0)"""
    if cid.startswith("chain"):
        t = _chain(129, 4, 1) if cid == "chain129_nx4" else _chain(int(cid[5:]))
    elif cid.startswith("bin"):
        t = _bin(dict(bin127=6, bin255=7, bin_pad128=6)[cid], pad=cid == "bin_pad128")
    elif cid == "rules":
        t = _rules_tree()
    elif cid == "box_only":
        t = _box_only()
    else:
        raise KeyError(cid)
    assert int(t["nk"].sum()) + 1 == len(t["nk"]) and np.all(t["nx"] + t["nu"] <= 6)
    t["id"] = cid
    return t


def realisations(t):
    return range(max(int(t["nk"][0]), 1))


def maps(t, j, leaf):
    return SH.ref_map(t["nk"], t["nx"], j, leaf)


def takes(t, j, leaf):
    """(tb, tr): the nodes that take the bound words of their image, and those that take the row words as well -- the rule of the comment
    above mpc_shift_sets, written out once more and independently of shift_cases.gather_sets (test_shift_set_reference.py compares them)"""
    img, rep = maps(t, j, leaf)
    n = len(t["nk"])
    tb, tr = np.zeros(n, bool), np.zeros(n, bool)
    for k in range(n):
        m = img[k]
        if m < 0 or rep[k]:
            continue
        tb[k] = t["kinds"][k] >= 2 and t["kinds"][m] >= 2 and t["nu"][k] == t["nu"][m]
        tr[k] = tb[k] and t["kinds"][k] == 3 and t["kinds"][m] == 3 and t["nc"][k] == t["nc"][m]
    return tb, tr


def refusals(t, j, leaf):
    """per node the set of reasons why it takes no bound words ("none": img = -1, "rep", "kind", "nu") and, where it takes them and is of
    kind 3, why it takes no row words ("rows_kind": the image is of kind 2, "nc")"""
    img, rep = maps(t, j, leaf)
    out = []
    for k in range(len(t["nk"])):
        m, why = img[k], set()
        if m < 0:
            why.add("none")
        else:
            if rep[k]:
                why.add("rep")
            if t["kinds"][k] < 2 or t["kinds"][m] < 2:
                why.add("kind")
            if t["nu"][k] != t["nu"][m]:
                why.add("nu")
            if not why and t["kinds"][k] == 3:
                if t["kinds"][m] != 3:
                    why.add("rows_kind")
                elif t["nc"][k] != t["nc"][m]:
                    why.add("nc")
        out.append(why)
    return out


# ---- the injected sets ----
def _draw(rng, t, k):
    """(bounds, rows, bound_sides, row_sides) of node k: bits below nz_k (nc_k), a sides bit only under a set bit; what the device
    ignores (the sets of kinds 0 and 1, the row words off kind 3) is 0, as tqgpu_get_working_sets reads it"""
    nz, nc, kind = int(t["nx"][k] + t["nu"][k]), int(t["nc"][k]), int(t["kinds"][k])
    if kind < 2:
        return (0, 0, 0, 0)
    b = int(rng.integers(0, 1 << nz))
    r = int(rng.integers(0, 1 << nc)) if kind == 3 else 0
    return (b, r, b & int(rng.integers(0, 1 << nz)), r & int(rng.integers(0, 1 << max(nc, 1))))


@functools.lru_cache(maxsize=None)
def _inject(cid, seed):
    return inject_tree(tree(cid), seed)


def inject_tree(t, seed):
    """inject() for a tree that is no row of the table (a row whose kinds or nc were changed): the four arrays"""
    cid = t["id"]
    n = len(t["nk"])
    rows_there = bool(np.any(t["kinds"] == 3))
    w = [None] * n
    rngs = [np.random.Generator(np.random.PCG64([seed, k, 9091])) for k in range(n)]
    need = [(tb, tr) for j in realisations(t) for leaf in POLICIES for tb, tr in [takes(t, j, leaf)]]
    imgs = [maps(t, j, leaf)[0] for j in realisations(t) for leaf in POLICIES]
    # descending: the image of a node that takes a set lies beyond it, so its words are final when the node is drawn
    for k in range(n - 1, -1, -1):
        for _ in range(1000):
            w[k] = _draw(rngs[k], t, k)
            if not rows_there:
                w[k] = (w[k][0], 0, 0, 0)          # no row words on the device: Gen::sides is not there either, bound_sides reads 0
            ok = True
            for (tb, tr), img in zip(need, imgs):
                if tb[k] and w[k][0] == w[img[k]][0] and w[k][2] == w[img[k]][2]:
                    ok = False
                if tr[k] and w[k][1] == w[img[k]][1] and w[k][3] == w[img[k]][3]:
                    ok = False
            if ok:
                break
        else:
            raise AssertionError(f"{cid}: node {k} cannot be told from its images")
    a = np.asarray(w, dtype=np.uint64)
    return tuple(np.ascontiguousarray(a[:, i]) for i in range(4))


def inject(c, seed=0):
    """seeded working sets for the tree (or case) c: dict(bounds, rows, bound_sides, row_sides), uint64 per node.  The bound words (or
    their sides) of node k and of img(k) differ wherever k takes them, the row words (or their sides) wherever k takes those, under every
    realisation and both leaf policies: a node is drawn again until they do."""
    words = _inject(c["id"], seed) if c is tree(c["id"]) or "tree" in c else inject_tree(c, seed)
    return {key: v.copy() for key, v in zip(WS_KEYS, words)}


def gathered(t, ws, j, leaf):
    """the reference: shift_cases.gather_sets, out of place"""
    img, rep = maps(t, j, leaf)
    return SH.gather_sets(t["nx"], t["nu"], t["nc"], t["kinds"], img, rep, ws)


# ---- the kernel's walk, in numpy and in place ----
def _lane(t, img, ws, k):
    """what lane k loads (None: nothing): the kernel's `if (m > k && m < Nn)` and its two flags"""
    n = len(t["nk"])
    m = img[k]
    if not (k < m < n):
        return None
    kk, km = t["kinds"][k], t["kinds"][m]
    tb = kk >= 2 and km >= 2 and t["nu"][k] == t["nu"][m]
    tr = tb and kk == 3 and km == 3 and t["nc"][k] == t["nc"][m]
    return (tb, tr, ws["bounds"][m], ws["bound_sides"][m], ws["rows"][m], ws["row_sides"][m])


def _store(ws, k, got):
    tb, tr, vb, vsb, vr, vsr = got
    if tb:
        ws["bounds"][k], ws["bound_sides"][k] = vb, vsb
    if tr:
        ws["rows"][k], ws["row_sides"][k] = vr, vsr


def node_table(t, j, leaf):
    """shift_node of tqgpu_mpc_set_shift for a root that keeps its states: img(k) where it lies beyond k and is no repeated leaf, else -1"""
    img, rep = maps(t, j, leaf)
    return np.where((img > np.arange(len(img))) & ~rep, img, -1)


def walk_in_place(t, ws, table, order="ascending"):
    """chunks of 64 in the given order, all loads of a chunk ahead of its stores"""
    ws = {k: np.array(v, copy=True) for k, v in ws.items()}
    n = len(t["nk"])
    bases = list(range(0, n, WAVE))
    for base in (bases if order == "ascending" else bases[::-1]):
        got = [(k, _lane(t, table, ws, k)) for k in range(base, min(base + WAVE, n))]
        for k, g in got:
            if g is not None:
                _store(ws, k, g)
    return ws


def walk_in_place_lanes(t, ws, table, loads_first=True):
    """ascending chunks; loads_first=False: every lane stores as soon as it has loaded, lanes descending within the chunk -- the order in which
    a store ahead of the wave's loads does harm (an image in the same chunk lies at a higher lane)"""
    if loads_first:
        return walk_in_place(t, ws, table)
    ws = {k: np.array(v, copy=True) for k, v in ws.items()}
    n = len(t["nk"])
    for base in range(0, n, WAVE):
        for k in range(min(base + WAVE, n) - 1, base - 1, -1):
            g = _lane(t, table, ws, k)
            if g is not None:
                _store(ws, k, g)
    return ws


# ---- the problems ----
def with_tree(t, **changed):
    """the tree with some of kinds, nc replaced (copies)"""
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    for k, v in changed.items():
        out[k] = _i32(v)
    return out


def rows_data(d, t, seed=41):
    """nc, C, D, dmin, dmax of the tree t (its nc), drawn as case() draws them -> the dict d, extended"""
    _rows_data(d, t, seed)
    return d


def _rows_data(d, t, seed):
    import mpc_cases as M
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    nx, nu, nc = t["nx"], t["nu"], t["nc"]
    d["nc"] = nc.copy()
    # (the root's states are fixed to x0: its C is zero, as ws_case's)
    d["C"] = np.concatenate([np.zeros(nc[k] * nx[k]) if k == 0 else M.quantised(rng, int(nc[k] * nx[k]), 0.25) for k in range(len(nc))])
    d["D"] = np.concatenate([M.quantised(rng, int(nc[k] * nu[k]), 1.0) for k in range(len(nc))])
    d["dmin"], d["dmax"] = -SPAN * np.ones(int(nc.sum())), SPAN * np.ones(int(nc.sum()))


@functools.lru_cache(maxsize=None)
def case(cid, seed=41):
    """the tree with its problem, a case of mpc_root_cases (the root keeps its states) with x0s for 12 steps.  Trees of one nx and one nu go
    through tracking_cases._states, as ws_case; `rules`, which has two of each, through mpc_root_cases._case with the same x0s"""
    import box_cases as BC
    import helpers as H
    import mpc_root_cases as R
    import solve_sequence_cases as SC
    import tracking_cases as K
    t = tree(cid)
    d = H.dense_shaped_qp(t["nk"], t["nx"], t["nu"], seed)
    if np.any(t["kinds"] == 0):          # clipping nodes: H_k diagonal
        Hs = BC._node_blocks(d)
        BC._set_blocks(d, [np.diag(np.diag(Hk)) if t["kinds"][k] == 0 else Hk for k, Hk in enumerate(Hs)])
    if np.any(t["nc"] > 0):
        _rows_data(d, t, seed)
    uniform = len(set(t["nx"].tolist())) == 1 and len(set(t["nu"][t["nk"] > 0].tolist())) == 1
    if uniform:
        c = K._states(cid, d, seed, True, kinds=t["kinds"], opts=SC.FULL)
    else:
        c = R._case(cid, d, kinds=t["kinds"], opts=SC.FULL)
        c["x0s"] = [c["x0"] * (1.0 + 0.02 * np.sin(0.7 * s + np.arange(c["nx0"]))) for s in range(12)]
    c["tree"] = t
    return c


def make(capi, c):
    import mpc_root_cases as R
    return R.make(capi, c, root_states=True)


# ---- foreign sets for the stage solvers: "a stale set is only ever a worse guess" ----
# The rows of gen_cases whose whole solve qualifies (gen_cases.clear_start succeeds; test_shift_set_reference.py checks the list) and two
# rows of box_cases for kind 2 (their start is the row's lambda0, as test_gpu_box_dense.py solves them).
FOREIGN_GEN_IDS = ("one_row", "mixed", "x0_elim", "row_and_bound", "more_rows_than_vars", "equality_row", "swap", "nz64", "nc64")
FOREIGN_BOX_IDS = ("nz64", "mixed")
FOREIGN_IDS = tuple(f"gen-{r}" for r in FOREIGN_GEN_IDS) + tuple(f"box-{r}" for r in FOREIGN_BOX_IDS)
FOREIGN_KINDS = ("empty", "all_bits", "complement", "sides_flipped") + tuple(f"random{i}" for i in range(8))
# the seeds of the drawn sets (all_bits, complement and random0 .. 7) per row: 0 unless the numpy model of the first sweep does not end on the
# cold set from that draw (a degenerate draw); such a seed is replaced here, never a pair skipped
FOREIGN_SEEDS: dict = {}
FOREIGN_OPTS = dict(stationarityTolerance=1e-8, regType=1, regValue=1e-8)          # gen_cases.FULL_TOL and the regularisation of the whole solves


@functools.lru_cache(maxsize=None)
def foreign_case(fid):
    """dict(id, d, kinds (those the device ends up with), start): the row's problem and the duals its whole solve starts from"""
    import box_cases as BC
    import gen_cases as GC
    fam, rid = fid.split("-", 1)
    if fam == "gen":
        c = GC.case(rid)
        d, kinds, start = c["d"], np.asarray(c["kinds"], np.int32).copy(), GC.clear_start(c["d"], c["kinds"])[0]
        kinds[(kinds == 3) & (np.asarray(d["nc"]) == 0)] = 2
    else:
        c = BC.case(rid)
        d, kinds, start = c["d"], np.asarray(c["kinds"], np.int32).copy(), c["lam0"]
    nc = np.asarray(d["nc"], np.int64) if "nc" in d else np.zeros(len(kinds), np.int64)
    return dict(id=fid, d=d, kinds=kinds, start=np.asarray(start, np.float64), nz=(np.asarray(d["nx"]) + np.asarray(d["nu"])).astype(np.int64), nc=nc)


def _mask(n):
    return (1 << int(n)) - 1


def _word(rng, n):
    return int.from_bytes(rng.bytes(8), "little") & _mask(n)


def foreign_set(fc, kind, cold):
    """one in-range set for every node of kinds 2 / 3 of the row: dict(bounds, rows, bound_sides, row_sides), uint64 per node.  cold: the
    final working sets of the cold solve (the same dict), which `complement` and `sides_flipped` start from."""
    seed = FOREIGN_SEEDS.get((fc["id"], kind), 0)
    out = {k: np.zeros(len(fc["kinds"]), np.uint64) for k in WS_KEYS}
    for k, kd in enumerate(fc["kinds"]):
        if kd < 2:
            continue
        rng = np.random.Generator(np.random.PCG64([seed, k, FOREIGN_KINDS.index(kind), 7717]))
        mb, mr = _mask(fc["nz"][k]), _mask(fc["nc"][k]) if kd == 3 else 0
        cb, cr = int(cold["bounds"][k]), int(cold["rows"][k])
        if kind == "empty":
            b = r = sb = sr = 0
        elif kind == "all_bits":
            b, r, sb, sr = mb, mr, _word(rng, 64), _word(rng, 64)
        elif kind == "complement":
            b, r, sb, sr = ~cb & mb, ~cr & mr, _word(rng, 64), _word(rng, 64)
        elif kind == "sides_flipped":
            b, r, sb, sr = cb, cr, ~int(cold["bound_sides"][k]), ~int(cold["row_sides"][k])
        else:
            b, r, sb, sr = _word(rng, 64) & mb, _word(rng, 64) & mr, _word(rng, 64), _word(rng, 64)
        if "nc" not in fc["d"]:
            r = sb = sr = 0          # a tree without rows has no words for rows and sides: they read 0 (as inject() on box_only)
        out["bounds"][k], out["rows"][k], out["bound_sides"][k], out["row_sides"][k] = b, r, sb & b, sr & r
    return out


def _sides_vector(b, sb, n):
    return np.asarray([(1 if (sb >> i) & 1 else -1) if (b >> i) & 1 else 0 for i in range(int(n))], int)


def _words_of(side):
    b = sum(1 << i for i, s in enumerate(side) if s != 0)
    return b, sum(1 << i for i, s in enumerate(side) if s > 0)


def first_sweep_qps(fc):
    """per node of kinds 2 / 3: (H, h, lo, hi, G, dlo, dhi) of the stage QP at the start duals (a box node has no rows)"""
    import gen_ref as G
    import newton_ref as N
    d, kinds = fc["d"], fc["kinds"]
    cons = G.cons_of(d) if "nc" in d else [None] * len(kinds)
    _, H, hs, los, his = N.stage_data(d, fc["start"], kinds=G._kinds2(kinds))
    out = {}
    for k, kd in enumerate(kinds):
        if kd < 2:
            continue
        n = len(hs[k])
        if kd == 3 and cons[k] is not None:
            out[k] = (H[k], hs[k], los[k], his[k], cons[k][0], cons[k][1], cons[k][2])
        else:
            out[k] = (H[k], hs[k], los[k], his[k], np.zeros((0, n)), np.zeros(0), np.zeros(0))
    return out


def model_first_sweep(fc, ws=None):
    """gen_hot_ref.solve_gen_from on every stage QP of the first sweep, started from the words ws (None: cold) -> (the final sets as
    words, steps per node)"""
    import gen_hot_ref as GH
    out = {k: np.zeros(len(fc["kinds"]), np.uint64) for k in WS_KEYS}
    steps = {}
    for k, qp in first_sweep_qps(fc).items():
        n, m = len(qp[1]), len(qp[5])
        side0 = None
        if ws is not None:
            side0 = np.concatenate([_sides_vector(int(ws["bounds"][k]), int(ws["bound_sides"][k]), n), _sides_vector(int(ws["rows"][k]), int(ws["row_sides"][k]), m)])
        r = GH.solve_gen_from(*qp, side0=side0)
        (out["bounds"][k], out["bound_sides"][k]), (out["rows"][k], out["row_sides"][k]) = _words_of(r["sb"]), _words_of(r["sr"])
        steps[k] = r["steps"]
    return out, steps


def step_cap(fc):
    """per node the steps one stage solve may take: the solver's cap 4 (nz + nc) + 8 for the pass from the given set and once more for the cold
    redo that follows a pass without a solution"""
    return 2 * (4 * (fc["nz"] + np.where(fc["kinds"] == 3, fc["nc"], 0)) + 8)

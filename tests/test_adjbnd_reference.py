"""The two numpy evaluations of adjbnd_ref.py against each other and against finite differences of the oracle's solve, on the CPU.

Bounds (adjbnd_cases.BOUND_TREES), at the oracle's solve with stationarityTolerance 1e-12 (`mixed`, which neither of the oracle's solvers
takes: adjbnd_ref.solve_active_set): every case with a kind-0 node has a kind-0 entry on a bound, every clipping case an input on a bound,
every `shared` h-group of kind 0 a free entry, but for the root groups listed in SATURATED (every stage of more than one entry of a tracking case likewise); over the list a state of a non-root node sits on a bound and a pinned entry (xmin == xmax)
exists; (a) and (b) agree within
the spreads kept in adjbnd_cases.SPREAD; gq / gr vanish exactly where a bound gradient may be non-zero; the lower gradient of the states
of a root with states is gx0.  Reference (TRACK_IDS): (a) and (b) agree within SPREAD for both windows and for T == 1.

Finite differences settle the signs and the side convention: active bound entries (those with the largest gradients of either side), a
pinned root state with both its bounds moved together, and entries of reference rows (the largest of gxref, of its last row and of guref),
moved by 2^-16, the oracle solving again; the active set of every perturbed solve is asserted unchanged.  The QP's solution is piecewise linear in its
data, so with the active set unchanged the difference quotient has no truncation error: what remains is the two solves' own error, each
converged to a dual gradient of 1e-12, times |w|_1 and the conditioning of the dual Hessian.  The bound used is 1e-9 absolute; every
product g h it is held against is asserted to be at least 100 times that (they range from 3e-7 to 8e-5), so that neither a wrong sign nor
a wrong side survives."""
import functools

import numpy as np
import pytest

import adjbnd_cases as BC
import adjbnd_ref as BR
import sens_ref as SR

FD_TOL = 1e-9
FD_MIN = 100 * FD_TOL          # the smallest |g h| a finite difference is held against
# The `shared` h-groups without a free entry, in trees the issue names: the root alone, whose inputs all sit on their bounds (and whose states,
# where it keeps them, are pinned).  Every other kind-0 group of every case has a free entry; the test asserts both directions.
SATURATED = {("states-single_wg", 0), ("elim-persist_c1", 0)}


def _oracle(orc, c, d):
    import sens_cases as SN
    if c["kinds"] is not None and np.any(np.asarray(c["kinds"]) == 0):
        return BR.solve_active_set(d, c["kinds"])          # a mixed tree
    return SN.oracle_solve(orc, dict(d=d, kinds=c["kinds"]))


@functools.lru_cache(maxsize=None)
def _bound(tree):
    import oracle_py as orc
    c = BC.bound_case(tree)
    s = _oracle(orc, c, c["d"])
    return c, s, BR.dense(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"]), BR.dual(c["d"], s["x"], s["u"], c["param"], c["w"], c["kinds"])


def _hgroup(c):
    import adjmat_ref as AM
    return AM.shared(c["d"], c["kinds"], 0)[0]


@pytest.mark.parametrize("tree", BC.BOUND_TREES)
def test_bound_case_is_valid_and_the_two_evaluations_agree(orc, tree):
    c, s, a, b = _bound(tree)
    assert s["status"] == 0 and b["n_reg"] == 0 and a["residual"] < 1e-9 * a["scale"]
    lo, hi = BR.sides(c["d"], s["x"], s["u"], c["kinds"])
    SX = len(s["x"])
    t = SR._assemble(c["d"], c["kinds"])
    if c["kinds"] is None:
        assert (lo | hi)[SX:].any(), "no input on a bound"
    if np.any(t["kinds"] == 0):
        assert (lo | hi).any(), "no kind-0 entry on a bound"
        hg = _hgroup(c)
        for grp in range(int(hg.max()) + 1):
            mem = np.flatnonzero(hg == grp)
            ii = np.concatenate([t["idx"][k] for k in mem])
            if t["kinds"][mem[0]] == 0:
                assert (lo | hi)[ii].all() == ((tree, grp) in SATURATED), f"h-group {grp}: free entries and SATURATED disagree"
    spread = max(float(np.max(np.abs(a[k] - b[k]))) for k in ("lo", "hi"))
    ga = [np.vstack(p) for p in zip(BR.group_sums(c["d"], a["lo"], _hgroup(c), c["kinds"], False), BR.group_sums(c["d"], a["hi"], _hgroup(c), c["kinds"], False))]
    gb = [np.vstack(p) for p in zip(BR.group_sums(c["d"], b["lo"], _hgroup(c), c["kinds"]), BR.group_sums(c["d"], b["hi"], _hgroup(c), c["kinds"]))]
    grouped = max(float(np.max(np.abs(x - y))) for x, y in zip(ga, gb))
    print(f"{tree}: spread bounds {spread:.1e} grouped {grouped:.1e} (recorded {BC.SPREAD[tree]})")
    assert spread <= 2.0 * BC.SPREAD[tree][0] + 1e-16 and grouped <= 2.0 * BC.SPREAD[tree][1] + 1e-16          # (2 x: another BLAS may sum in another order)
    # complementary to gq, gr, exactly
    gz = np.vstack([b["gq"], b["gr"]])
    assert np.all(gz[lo | hi] == 0.0) and np.all(b["lo"][~lo] == 0.0) and np.all(b["hi"][~hi] == 0.0)
    if c["form"] == "states":
        assert np.array_equal(b["lo"][:c["nx0"]], b["gx0"]) and np.all(lo[:c["nx0"]])


def test_the_bound_cases_cover_what_the_issue_asks():
    state_below_root = pinned = False
    for tree in BC.BOUND_TREES:
        c, s, _, _ = _bound(tree)
        lo, hi = BR.sides(c["d"], s["x"], s["u"], c["kinds"])
        nx0 = int(c["d"]["nx"][0])
        state_below_root |= bool((lo | hi)[nx0:len(s["x"])].any())
        pinned |= bool(np.any((c["d"]["xmin"] == c["d"]["xmax"]) & lo[:len(s["x"])]))
    assert state_below_root and pinned
    assert set(BC.SPREAD) == set(BC.BOUND_TREES) | set(BC.TRACK_IDS)


@pytest.mark.parametrize("tree", [t for t in BC.BOUND_TREES if t != "elim-dense_kind1_root"])
def test_bound_gradient_against_the_oracle_finite_difference(orc, tree):
    c, s, a, _ = _bound(tree)
    lo, hi = BR.sides(c["d"], s["x"], s["u"], c["kinds"])
    SX = len(s["x"])
    wx, wu = c["w"]
    checked = 0
    for side, names, sign in ((lo, ("xmin", "umin"), 1.0), (hi, ("xmax", "umax"), -1.0)):
        free_of_pins = side & ~np.concatenate([c["d"]["xmin"] == c["d"]["xmax"], c["d"]["umin"] == c["d"]["umax"]])
        g_side = a["lo" if sign > 0 else "hi"][:, 0]
        for e in sorted(np.flatnonzero(free_of_pins), key=lambda i: -abs(g_side[i]))[:2]:
            d1 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
            name, at = (names[0], e) if e < SX else (names[1], e - SX)
            d1[name][at] += sign * BC.FD_H          # towards the inside: the entry stays on this bound
            s1 = _oracle(orc, c, d1)
            assert s1["status"] == 0
            lo1, hi1 = BR.sides(d1, s1["x"], s1["u"], c["kinds"])
            assert np.array_equal(lo, lo1) and np.array_equal(hi, hi1), f"{tree}: entry {e}: the active set changed"
            got = float(wx[:, 0] @ (s1["x"] - s["x"]) + wu[:, 0] @ (s1["u"] - s["u"]))
            want = float(a["lo" if sign > 0 else "hi"][e, 0]) * sign * BC.FD_H
            print(f"{tree} entry {e} ({name}): w' dz = {got:.6e}, g h = {want:.6e}")
            assert abs(want) >= FD_MIN and abs(got - want) <= FD_TOL
            checked += 1
    assert checked > 0
    if c["form"] == "states":
        # a pinned entry: both bounds moved together, held against the lower gradient
        e = int(np.argmax(np.abs(a["lo"][:c["nx0"], 0])))
        d1 = {k: np.array(v, copy=True) for k, v in c["d"].items()}
        d1["xmin"][e] += BC.FD_H
        d1["xmax"][e] += BC.FD_H
        s1 = _oracle(orc, c, d1)
        lo1, hi1 = BR.sides(d1, s1["x"], s1["u"], c["kinds"])
        assert s1["status"] == 0 and np.array_equal(lo, lo1) and np.array_equal(hi, hi1), f"{tree}: pinned entry {e}: the active set changed"
        got = float(wx[:, 0] @ (s1["x"] - s["x"]) + wu[:, 0] @ (s1["u"] - s["u"]))
        want = float(a["lo"][e, 0]) * BC.FD_H
        print(f"{tree} pinned entry {e}: w' dz = {got:.6e}, g h = {want:.6e}")
        assert np.all(a["hi"][:c["nx0"]] == 0.0) and abs(want) >= FD_MIN and abs(got - want) <= FD_TOL


@functools.lru_cache(maxsize=None)
def _track(cid, t0, T=None):
    import oracle_py as orc
    c = BC.track_case(cid, T)
    d = BC.folded(c, t0)
    s = _oracle(orc, c, d)
    return c, d, s, BR.dense(d, s["x"], s["u"], c["param"], c["w"], c["kinds"]), BR.dual(d, s["x"], s["u"], c["param"], c["w"], c["kinds"])


def _S0(c):
    return c["root"]["S0"] if c["form"] == "elim" else None


@pytest.mark.parametrize("cid", BC.TRACK_IDS)
def test_reference_the_two_evaluations_agree(orc, cid):
    sx = su = 0.0
    for t0, T in [(t, None) for t in BC.windows(BC.track_case(cid))] + [(0, 1)]:
        c, d, s, a, b = _track(cid, t0, T)
        assert s["status"] == 0 and b["n_reg"] == 0
        ra = BR.reference(d, a["gq"], a["gr"], t0, c["T"], c["NXT"], c["NUT"], c["kinds"], _S0(c), chunked=False)
        rb = BR.reference(d, b["gq"], b["gr"], t0, c["T"], c["NXT"], c["NUT"], c["kinds"], _S0(c))
        assert ra[:2] == rb[:2] == BR.rows_of(d["nk"], t0, c["T"])
        sx, su = max(sx, float(np.max(np.abs(ra[2] - rb[2])))), max(su, float(np.max(np.abs(ra[3] - rb[3]))))
        assert np.any(rb[2] != 0.0) and np.any(rb[3] != 0.0)
        on = SR.pinned(d, s["x"], s["u"], c["kinds"])
        t, st = SR._assemble(d, c["kinds"]), BR.stages(d["nk"])
        for stage in range(int(st.max()) + 1):
            ii = np.concatenate([t["idx"][k] for k in np.flatnonzero(st == stage)])
            assert len(ii) == 1 or not on[ii].all(), f"stage {stage}: no free entry"          # (one entry: the one input of C1's eliminated root)
    print(f"{cid}: spread gxref {sx:.1e} guref {su:.1e} (recorded {BC.SPREAD[cid]})")
    assert sx <= 2.0 * BC.SPREAD[cid][0] + 1e-16 and su <= 2.0 * BC.SPREAD[cid][1] + 1e-16


@pytest.mark.parametrize("cid", ["single_wg", "kind1_S0", "fan65"])
def test_reference_gradient_against_the_oracle_finite_difference(orc, cid):
    import tracking_cases as TC
    t0 = BC.windows(BC.track_case(cid))[1]
    c, d, s, a, _ = _track(cid, t0)
    row0, rows, gx, gu = BR.reference(d, a["gq"], a["gr"], t0, c["T"], c["NXT"], c["NUT"], c["kinds"], _S0(c), chunked=False)
    lo, hi = BR.sides(d, s["x"], s["u"], c["kinds"])
    wx, wu = c["w"]
    big = lambda G: tuple(int(v) for v in np.unravel_index(np.argmax(np.abs(G[:, :, 0])), G[:, :, 0].shape))
    for name, G, (r, j) in (("xtraj", gx, big(gx)), ("xtraj", gx, (rows - 1, big(gx[rows - 1:])[1])), ("utraj", gu, big(gu))):
        c1 = dict(c)
        c1[name] = np.array(c[name], copy=True)
        c1[name][row0 + r, j] += BC.FD_H
        d1 = BC.folded(c1, t0)
        s1 = _oracle(orc, c, d1)
        assert s1["status"] == 0
        lo1, hi1 = BR.sides(d1, s1["x"], s1["u"], c["kinds"])
        assert np.array_equal(lo, lo1) and np.array_equal(hi, hi1), f"{cid}: {name}[{row0 + r}, {j}]: the active set changed"
        got = float(wx[:, 0] @ (s1["x"] - s["x"]) + wu[:, 0] @ (s1["u"] - s["u"]))
        want = float(G[r, j, 0]) * BC.FD_H
        print(f"{cid} {name}[{row0 + r}, {j}]: w' dz = {got:.6e}, g h = {want:.6e}")
        assert abs(want) >= FD_MIN and abs(got - want) <= FD_TOL

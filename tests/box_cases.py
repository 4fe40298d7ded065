"""The case table of the box-constrained dense stage solver (device kind 2, stage_box): small trees at the sizes and bound
patterns where one wave with one entry per lane can go wrong, built on the CPU and shared by test_box_reference.py (the
conditions every row must meet, checked without a device) and test_gpu_box_step.py (the device pins).

A row is (id, tree, kinds, bound recipe).  The tree is a nested node (nx, nu, [children]) as in limit_shapes.py; H_k comes from
helpers.dense_shaped_qp (diag + M M'), reduced to its diagonal on clipping nodes.  The bounds are drawn around the unconstrained
stage values z_unc at the row's own lambda0: every entry gets the wide bounds -+(5 + |z_unc|), the entries the row cuts get
z_unc -+ amt with amt in [0.05, 0.5] on one side (that bound is then active or nearly so at lambda0), and the entries it pinches
get z_unc -+ 0.01 on both sides (free at lambda0, on either bound a step away: the path-independence test needs entries that move
from one bound to the other).  Only nodes that have children are cut unless the row says otherwise: the rank of the Newton
matrix M = G P G' is bounded by the free entries of a parent plus the free states of its children.

lambda0 is the first of the 20 seeds of newton_ref.starting_duals at which the row meets its conditions (COND_MAX, GAP, its own
`accept`).  COND_MAX = 1e6 is the bound test_limits_reference.py uses for its 1e-10 tolerance on the step (a float64 solve of a
system of that condition keeps 1e6 * 2^-53 ~ 1e-10), GAP = 1e-6 the gap of starting_duals (the active set is then the same for
every implementation whose stage values are good to 1e-6, and the step a smooth function of the data), SLACK_MIN = 1e-9 the
distance an Armijo decision must keep from equality, relative to the sum of the absolute node terms, before a trial count is
pinned (a float64 sum of some hundred terms is uncertain by about 1e-14 of that)."""
from __future__ import annotations

import functools

import numpy as np

import newton_ref as N
from helpers import dense_shaped_qp, offsets
from limit_shapes import flatten, leaf
from treeqp_amd import problems as P

COND_MAX = 1e6
GAP = 1e-6
SLACK_MIN = 1e-9
TRIES = 20
OPTS = dict(lineSearchGamma=0.1, lineSearchBeta=0.6, lineSearchMaxIter=50)      # the defaults of the solver


class LsOpts:
    lineSearchGamma, lineSearchBeta, lineSearchMaxIter = OPTS["lineSearchGamma"], OPTS["lineSearchBeta"], OPTS["lineSearchMaxIter"]


# ---------------------------------------------------------------------------------------------------------------------------
# problem construction
# ---------------------------------------------------------------------------------------------------------------------------

def _node_blocks(d):
    """per node H_k (dense, from Q, R, S)"""
    return N._blocks(d, True)[-1]


def _set_blocks(d, H):
    Q, R, S = [], [], []
    for k, Hk in enumerate(H):
        a = int(d["nx"][k])
        Q.append(Hk[:a, :a].ravel(order="F")); R.append(Hk[a:, a:].ravel(order="F")); S.append(Hk[a:, :a].ravel(order="F"))
    d["Q"], d["R"], d["S"] = np.concatenate(Q), np.concatenate(R), np.concatenate(S)
    xo, uo = offsets(d)
    for k, Hk in enumerate(H):
        a = int(d["nx"][k])
        d["Qd"][xo[k]:xo[k + 1]] = np.diag(Hk)[:a]
        d["Rd"][uo[k]:uo[k + 1]] = np.diag(Hk)[a:]


def base_problem(shape, kinds, seed, pair_root=False, indefinite_root=False):
    nk, nx, nu = flatten(shape)
    d = dense_shaped_qp(nk, nx, nu, seed)
    H = _node_blocks(d)
    for k in range(len(nk)):
        if kinds[k] == 0:
            H[k] = np.diag(np.diag(H[k]))
    if pair_root:
        # H, q, r of the root and the columns of its children's [A | B] invariant under swapping entries 2i and 2i + 1
        a, m = int(nx[0]), int(nu[0])
        assert a % 2 == 0 and m % 2 == 0
        rng = np.random.Generator(np.random.PCG64(seed + 1))
        Mx = 0.3 * np.repeat(rng.standard_normal(((a + m) // 2, a + m)), 2, axis=0)
        H[0] = np.diag(np.repeat(1.0 + rng.random((a + m) // 2), 2)) + Mx @ Mx.T
        d["q"][:a] = np.repeat(d["q"][:a:2], 2)
        d["r"][:m] = np.repeat(d["r"][:m:2], 2)
        ao = bo = 0
        dad = P.parents_of(nk)
        for k in range(1, len(nk)):
            na, nb = nx[k] * nx[dad[k]], nx[k] * nu[dad[k]]
            if dad[k] == 0:
                A = d["A"][ao:ao + na].reshape((nx[k], a), order="F"); A[:, 1::2] = A[:, ::2]
                B = d["B"][bo:bo + nb].reshape((nx[k], m), order="F"); B[:, 1::2] = B[:, ::2]
                d["A"][ao:ao + na] = A.ravel(order="F"); d["B"][bo:bo + nb] = B.ravel(order="F")
            ao += na; bo += nb
    if indefinite_root:
        H[0] = np.diag([1.0, -1.0, 1.0]) + 0.05 * (np.ones((3, 3)) - np.eye(3))
    _set_blocks(d, H)
    return d


def unconstrained_values(d, kinds, lam):
    """z_unc per node at lam: H_k^-1 h_k"""
    tree, H, hs, _, _ = N.stage_data(d, lam, kinds=np.where(np.asarray(kinds) == 0, 0, 1))
    return [np.asarray(h / Hk if Hk.ndim == 1 else np.linalg.solve(Hk, h.astype(np.float64)), dtype=np.float64) for Hk, h in zip(H, hs)]


def draw_bounds(d, kinds, lam, recipe, seed):
    """the bound recipe of the module docstring; recipe(k, nx_k, nu_k, has_kids, rng) -> dict(cut=[...], pinch=[...], equal=[...],
    side=+1 / -1 / None (drawn), far, pair) with entry indices into [x_k | u_k]"""
    rng = np.random.Generator(np.random.PCG64(seed + 31))
    xo, uo = offsets(d)
    zu = unconstrained_values(d, kinds, lam)
    for k, z in enumerate(zu):
        a, m = int(d["nx"][k]), int(d["nu"][k])
        lo, hi = -(5.0 + np.abs(z)), 5.0 + np.abs(z)
        r = recipe(k, a, m, bool(d["nk"][k]), rng) if kinds[k] != 1 else {}
        for i in r.get("cut", []):
            up = rng.random() < 0.5 if r.get("side") is None else r["side"] > 0
            amt = 0.05 + 0.45 * rng.random()
            if up:
                hi[i] = z[i] - amt
            else:
                lo[i] = z[i] + amt
        for i in r.get("pinch", []):
            lo[i], hi[i] = z[i] - 0.01, z[i] + 0.01
        for i in r.get("equal", []):
            lo[i] = hi[i] = z[i] + 0.1
        if r.get("far"):                                # one-sided rows: the far side is infinite, IEEE on even entries, P.INF on odd ones
            tgt, sgn = (lo, -1.0) if r["side"] > 0 else (hi, 1.0)
            tgt[0::2], tgt[1::2] = sgn * np.inf, sgn * P.INF
        if r.get("pair"):
            lo[1::2], hi[1::2] = lo[::2], hi[::2]
        if kinds[k] == 1:
            lo[:], hi[:] = -P.INF, P.INF
        d["xmin"][xo[k]:xo[k + 1]], d["xmax"][xo[k]:xo[k + 1]] = lo[:a], hi[:a]
        d["umin"][uo[k]:uo[k + 1]], d["umax"][uo[k]:uo[k + 1]] = lo[a:], hi[a:]


# ---------------------------------------------------------------------------------------------------------------------------
# recipes and acceptance conditions of the rows
# ---------------------------------------------------------------------------------------------------------------------------

def frac(f, only_parents=True, only_u=(), pinch=0.0, must=(), never=()):
    """cut a fraction f of the entries (all of `must`, none of `never`; negative indices count from the end), pinch a fraction
    `pinch` of the others; nodes listed in only_u are cut in their inputs only"""
    def recipe(k, a, m, has_kids, rng):
        if only_parents and not has_kids:
            return {}
        n = a + m
        pool = [i for i in (range(a, n) if k in only_u else range(n))]
        mu = [i % n for i in must]
        nv = [i % n for i in never]
        pick = set(int(i) for i in rng.permutation(pool)[:int(round(f * len(pool)))]) | set(mu)
        pick -= set(nv)
        rest = [i for i in range(n) if i not in pick and i not in nv]
        pin = [int(i) for i in rng.permutation(rest)[:int(round(pinch * n))]]
        return dict(cut=sorted(pick), pinch=pin)
    return recipe


def per_node(table, default=None):
    def recipe(k, a, m, has_kids, rng):
        r = table.get(k, default)
        return r(k, a, m, has_kids, rng) if callable(r) else (r or {})
    return recipe


def root_side(ref, i):
    return int(ref["stages"]["side"][0][i])


def box_nodes_active(ref, kinds, except_nodes=()):
    return all(np.any(ref["stages"]["side"][k] != 0) for k in np.flatnonzero(np.asarray(kinds) == 2) if k not in except_nodes)


class Row:
    def __init__(self, rid, shape, kinds, recipe, seed=5, scale=0.1, accept=None, inactive_nodes=(), note="", **base):
        self.id, self.shape, self.kinds, self.recipe, self.seed, self.scale = rid, shape, np.asarray(kinds, np.int32), recipe, seed, scale
        self.accept, self.inactive_nodes, self.note, self.base = accept, inactive_nodes, note, base


def _mixed_shape():
    lv3 = lambda *n: [leaf(v) for v in n]
    return (10, 6, [(8, 4, [(6, 3, lv3(3, 4)), (9, 4, lv3(5, 3))]),
                    (12, 6, [(7, 5, lv3(4, 6)), (4, 2, lv3(2))])])


def _mixed_kinds():
    nk = flatten(_mixed_shape())[0]
    dad = P.parents_of(nk)
    st = np.zeros(len(nk), int)
    for k in range(1, len(nk)):
        st[k] = st[dad[k]] + 1
    return np.asarray([(2, 0, 1, 2)[s % 4] for s in st], np.int32)


ROWS = [
    Row("nz1", (1, 0, [leaf(1)]), [2, 1], frac(1.0), note="root nx = 1, nu = 0: its one entry is fixed, P_0 = 0"),
    Row("nz2", (1, 1, [leaf(1)]), [2, 1], per_node({0: dict(cut=[1])})),
    Row("nz63", (40, 23, [leaf(4)]), [2, 1], frac(0.35, must=(-1,)), accept=lambda ref: root_side(ref, 62) != 0,
        note="entry 62, the last one, in the working set"),
    Row("nz63_last_free", (40, 23, [leaf(4)]), [2, 1], frac(0.35, must=(-2,), never=(-1,)),
        accept=lambda ref: root_side(ref, 62) == 0 and root_side(ref, 61) != 0,
        note="entry 62 free next to a fixed entry 61 (the last lane has one neighbour)"),
    Row("nz64", (40, 24, [leaf(40)]), [2, 2], frac(0.35, only_parents=False, must=(-1,), pinch=0.15),
        accept=lambda ref: root_side(ref, 63) != 0, note="bit 63 of the working set; the leaf (nx = 40) is a box node as well and is cut"),
    Row("nz64_last_free", (40, 24, [leaf(40)]), [2, 2], frac(0.35, only_parents=False, must=(-2,), never=(-1,)),
        accept=lambda ref: root_side(ref, 63) == 0 and root_side(ref, 62) != 0, note="entry 63 free next to a fixed entry 62"),
    Row("none_active", (10, 6, [leaf(5)]), [2, 2], frac(0.0), inactive_nodes=(0, 1), note="every bound wide: mask 0, P = H^-1 of k_dense_init"),
    Row("all_inputs_fixed", (8, 5, [leaf(4)]), [2, 1], per_node({0: dict(cut=list(range(8, 13)))}),
        accept=lambda ref: np.all(ref["stages"]["side"][0][8:] != 0) and np.all(ref["stages"]["side"][0][:8] == 0)),
    Row("equal_bounds", (4, 2, [(8, 4, [leaf(3)])]), [2, 2, 1], per_node({0: dict(cut=[4]), 1: dict(cut=[9, 11], equal=[1, 5, 10])}),
        note="entries 1, 5, 10 of the interior node have lo == hi"),
    Row("one_sided", (8, 6, [leaf(4)]), [2, 1], per_node({0: dict(cut=[1, 4, 9, 12, 13], side=1, far=True)}),
        note="lower bounds -inf (even entries) and -1e12 (odd entries), upper bounds cut"),
    Row("one_sided_mirror", (8, 6, [leaf(4)]), [2, 1], per_node({0: dict(cut=[1, 4, 9, 12, 13], side=-1, far=True)}),
        note="upper bounds +inf / +1e12, lower bounds cut"),
    Row("tie", (4, 4, [leaf(3)]), [2, 1], per_node({0: dict(cut=[0, 1, 4, 5], side=1, pair=True)}), pair_root=True,
        note="root invariant under swapping entries 2i and 2i + 1: two entries block at the same step length"),
    Row("mixed", _mixed_shape(), _mixed_kinds(),
        per_node({0: frac(0.35, pinch=0.15), 1: frac(0.5, only_u=(1,)), 2: frac(0.5, only_u=(2,))},
                 default=lambda k, a, m, kids, rng: {} if kids else dict(cut=[0])),
        note="stage kinds 2, 0, 1, 2; the clipping nodes are cut in their inputs, every leaf (box node) in its first state"),
    Row("x0_eliminated", (0, 4, [(5, 3, [leaf(3)])]), [2, 2, 1], per_node({0: dict(cut=[0, 2]), 1: dict(cut=[5, 7])}),
        note="nx[0] = 0: the root is a dense R with two cut inputs"),
    # farther from the optimum: the full step overshoots and the line search backtracks
    Row("far_nz18", (10, 8, [leaf(6)]), [2, 2], frac(0.4, only_parents=False), scale=2.0, accept=lambda ref: True),
    Row("far_mixed", _mixed_shape(), _mixed_kinds(),
        per_node({0: frac(0.35), 1: frac(0.5, only_u=(1,)), 2: frac(0.5, only_u=(2,))},
                 default=lambda k, a, m, kids, rng: {} if kids else dict(cut=[0])), scale=2.0),
]
ROW_IDS = [r.id for r in ROWS]
PATH_ROWS = ("nz64", "mixed")
XU_PIN_REQUIRED = ("nz64", "mixed", "equal_bounds")


def row(rid):
    return ROWS[ROW_IDS.index(rid)]


@functools.lru_cache(maxsize=None)
def case(rid):
    """The problem of row `rid`: dict(row, d, kinds, lam0, seed, ref, trials, slack, lam1, st1, xu_pin).  ref is the Newton step
    at lam0, (trials, slack) the reference line search from there, lam1 = lam0 + beta^(trials - 1) dlam the point it accepts, st1
    the stage solutions there; xu_pin says whether x, u of the device are compared at lam1 (margin there >= GAP and the trial
    count itself pinned)."""
    r = row(rid)
    nlam = int(flatten(r.shape)[1][1:].sum())
    for s in range(TRIES):
        lam0 = N.seeded_duals(nlam, s, r.scale)
        d = base_problem(r.shape, r.kinds, r.seed, **r.base)
        draw_bounds(d, r.kinds, lam0, r.recipe, r.seed)
        ref = N.newton_step(d, lam0, kinds=r.kinds)
        if not (ref["margin"] >= GAP and ref["cond"] <= COND_MAX and box_nodes_active(ref, r.kinds, r.inactive_nodes)):
            continue
        if r.accept is not None and not r.accept(ref):
            continue
        trials, slack = N.armijo_trials(d, lam0, ref["dlam"], ref["res"], LsOpts, r.kinds)
        lam1 = lam0 + OPTS["lineSearchBeta"] ** (trials - 1) * ref["dlam"]
        st1 = N.stage_solutions(d, lam1, kinds=r.kinds)
        return dict(row=r, d=d, kinds=r.kinds, lam0=lam0, seed=s, ref=ref, trials=trials, slack=slack, lam1=lam1, st1=st1,
                    xu_pin=bool(st1["margin"] >= GAP and slack >= SLACK_MIN))
    raise AssertionError(f"row {rid}: none of the {TRIES} seeds of starting_duals meets the row's conditions")


# ---------------------------------------------------------------------------------------------------------------------------
# lands_on_bound: a diagonal problem in dyadic numbers whose unconstrained stage values meet bounds exactly
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lands_on_bound():
    """root (2, 2) with two leaves of nx = 2.  Weights in {1, 4, 16}, every other number a multiple of 1/8 of small size: h, h / w,
    the Cholesky factor of diag(w) and its solves are exact in float64.  At lam0 entry 1 of the root sits exactly on its upper
    bound, entry 2 exactly on its lower bound, entry 0 of leaf 2 exactly on its upper bound; entry 3 of the root is cut."""
    nk, nx, nu = np.array([2, 0, 0], np.int32), np.array([2, 2, 2], np.int32), np.array([2, 0, 0], np.int32)
    A1, A2 = np.array([[0.5, -1.0], [1.0, 0.5]]), np.array([[-0.5, 0.0], [1.0, 1.0]])
    B1, B2 = np.array([[1.0, 0.5], [-0.5, 1.0]]), np.array([[0.5, -1.0], [0.0, 0.5]])
    d = dict(nk=nk, nx=nx, nu=nu, A=np.concatenate([A1.ravel(order="F"), A2.ravel(order="F")]),
             B=np.concatenate([B1.ravel(order="F"), B2.ravel(order="F")]), b=np.array([0.25, -0.5, 0.125, 0.75]),
             Qd=np.array([4.0, 1.0, 16.0, 4.0, 1.0, 4.0]), Rd=np.array([1.0, 16.0]),
             q=np.array([0.5, -0.25, 1.0, -0.75, 0.25, 0.5]), r=np.array([-0.5, 1.25]))
    lam0 = np.array([0.25, -0.375, 0.5, 0.125])
    H = [np.diag(np.concatenate([d["Qd"][0:2], d["Rd"]])), np.diag(d["Qd"][2:4]), np.diag(d["Qd"][4:6])]
    d["xmin"], d["xmax"], d["umin"], d["umax"] = np.zeros(6), np.zeros(6), np.zeros(2), np.zeros(2)
    _set_blocks(d, H)
    kinds = np.array([2, 2, 2], np.int32)
    zu = unconstrained_values(d, np.zeros(3, int), lam0)
    lo = [-(5.0 + np.abs(z)) for z in zu]
    hi = [5.0 + np.abs(z) for z in zu]
    hi[0][1] = zu[0][1]; lo[0][2] = zu[0][2]; hi[2][0] = zu[2][0]
    hi[0][3] = zu[0][3] - 0.25
    d["xmin"] = np.concatenate([lo[0][:2], lo[1], lo[2]]); d["xmax"] = np.concatenate([hi[0][:2], hi[1], hi[2]])
    d["umin"], d["umax"] = lo[0][2:], hi[0][2:]
    ref = N.newton_step(d, lam0, kinds=np.zeros(3, int))
    return dict(d=d, kinds=kinds, lam0=lam0, ref=ref, landed=[(0, 1), (0, 2), (2, 0)])


# ---------------------------------------------------------------------------------------------------------------------------
# path independence: two duals whose working sets differ by a release, an addition and a swap of sides
# ---------------------------------------------------------------------------------------------------------------------------

def _sides(st):
    return np.concatenate(st["side"])


@functools.lru_cache(maxsize=None)
def path_duals(rid):
    """(lamA, lamB, counts): lamA is the row's lam0; relative to the working sets of lamA's last trial (lam1), those at lamB
    release at least one bound, add at least one and hold at least one entry on its upper bound that was on its lower one.
    lamB is the first of 40 seeded draws (scale 1 around -2 lam1) that does, with margin >= GAP and cond(M) <= COND_MAX."""
    c = case(rid)
    sA = _sides(c["st1"])
    n = len(c["lam0"])
    for s in range(40):
        lamB = -2.0 * c["lam1"] + np.random.Generator(np.random.PCG64(7000 + s)).standard_normal(n)
        ref = N.newton_step(c["d"], lamB, kinds=c["kinds"])
        sB = _sides(ref["stages"])
        counts = dict(released=int(np.sum((sA != 0) & (sB == 0))), added=int(np.sum((sA == 0) & (sB != 0))),
                      swapped=int(np.sum((sA == -1) & (sB == 1))), active_A=int(np.sum(sA != 0)))
        if ref["margin"] >= GAP and ref["cond"] <= COND_MAX and min(counts["released"], counts["added"], counts["swapped"]) >= 1:
            return c["lam0"], lamB, counts
    raise AssertionError(f"row {rid}: no second dual with a release, an addition and a swap")


def other_hessians(d, kinds, seed=77):
    """the same problem with other H_k on the dense nodes (same bounds, same dynamics)"""
    d2 = {k: np.array(v, copy=True) for k, v in d.items()}
    rng = np.random.Generator(np.random.PCG64(seed))
    H = _node_blocks(d2)
    for k, Hk in enumerate(H):
        if kinds[k] != 0:
            Mx = 0.2 * rng.standard_normal(Hk.shape)
            H[k] = Hk + Mx @ Mx.T
    _set_blocks(d2, H)
    return d2


# ---------------------------------------------------------------------------------------------------------------------------
# status 4: an indefinite stage Hessian
# ---------------------------------------------------------------------------------------------------------------------------

def indefinite_pair():
    """(bad, good, kinds): a two-node tree with nz = 3 on the root; `bad` has H_0 = diag(1, -1, 1) + 0.05 off the diagonal and
    wide bounds (entry 1 is free: H_FF is not positive definite), `good` is the well-posed problem on the same tree."""
    shape, kinds = (2, 1, [leaf(2)]), np.array([2, 1], np.int32)
    good = base_problem(shape, kinds, 9)
    draw_bounds(good, kinds, np.zeros(2), per_node({0: dict(cut=[2])}), 9)
    bad = base_problem(shape, kinds, 9, indefinite_root=True)
    for k in ("xmin", "xmax", "umin", "umax"):
        bad[k] = good[k].copy()
    return bad, good, kinds


# ---------------------------------------------------------------------------------------------------------------------------
# the whole dual Newton method on the reference (is the row's QP feasible at all?)
# ---------------------------------------------------------------------------------------------------------------------------

def reference_solve(d, kinds, lam0=None, tol=1e-10, max_iter=50, reg=1e-8):
    """newton_step + armijo_trials until the dynamics residual is below tol (max norm).  Returns (iterations, trials, residual,
    lam).  The bounds of a row are drawn around stage values, not around a point that satisfies the dynamics: a row whose QP is
    infeasible would have an unbounded dual and never end here."""
    lam = np.zeros(int(np.asarray(d["nx"])[1:].sum())) if lam0 is None else np.array(lam0, dtype=float)
    trials = 0
    for it in range(max_iter + 1):
        ref = N.newton_step(d, lam, kinds=kinds, reg=reg)
        err = float(np.max(np.abs(ref["res"]))) if len(ref["res"]) else 0.0
        if err <= tol or it == max_iter:
            return it, trials, err, lam
        t, _ = N.armijo_trials(d, lam, ref["dlam"], ref["res"], LsOpts, kinds)
        trials += t
        lam = lam + OPTS["lineSearchBeta"] ** (t - 1) * ref["dlam"]

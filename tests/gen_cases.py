"""The case table of the stage solver for general constraints (device kind 3, stage_gen): small trees at the shapes where one wave
with one entry and one row per lane can go wrong, built on box_cases.base_problem and shared by test_gen_reference.py (the
conditions every row must meet, without a device) and the device pins test_gpu_gen_step.py / test_gpu_gen_dense.py.

A row is (id, tree, kinds, bound recipe, row recipe).  Bounds are drawn as in box_cases (around the unconstrained stage values
at the row's lambda0).  The rows of G = [C | D] are standard normal; their ranges are drawn around G z_box, z_box the solution of
the node's box QP at lambda0: a `cut` row gets dmax = G z_box - amt (or dmin = G z_box + amt) with amt in [0.05, 0.3] and the
other side far away (active at lambda0), a `loose` row gets -+(5 + |G z_box|) around it, an `eq` row dmin = dmax = G z_box + 0.1.

Guards, asserted at generation (a seed that breaks one is passed over, never a test skipped): cond(M) <= COND_MAX, strict
complementarity and strict inactivity GAP at lambda0 (and at the accepted trial point for the x, u pin), cond(S) <= COND_MAX on
every working set, the row's own `accept`."""
from __future__ import annotations

import functools

import numpy as np

import box_cases as BC
import gen_ref as G
import newton_ref as N
from helpers import offsets
from limit_shapes import flatten, leaf
from treeqp_amd import problems as P

COND_MAX = BC.COND_MAX
GAP = BC.GAP
SLACK_MIN = BC.SLACK_MIN
TRIES = 20
BETA = BC.OPTS["lineSearchBeta"]


class Row:
    def __init__(self, rid, shape, kinds, rows, bounds=None, accept=None, full=False, note=""):
        self.id, self.shape, self.kinds, self.rows = rid, shape, np.asarray(kinds, np.int32), rows
        self.bounds = bounds if bounds is not None else BC.frac(0.25, only_parents=False)
        self.accept, self.full, self.note = accept, full, note


def rside(ref, k):
    return ref["stages"]["rside"][k]


def n_active(ref, k):
    return int(np.sum(rside(ref, k) != 0))


_MIXED = (4, 2, [(3, 2, [leaf(2), leaf(2)]), (3, 2, [leaf(2), leaf(3)])])

ROWS = [
    Row("one_row", (2, 1, [leaf(2), leaf(2)]), [3, 1, 1], {0: ["cut"]}, accept=lambda r: n_active(r, 0) == 1, full=True),
    Row("row_and_bound", (3, 2, [leaf(2)]), [3, 1], {0: ["cut"]}, bounds=BC.per_node({0: dict(cut=[4])}),
        accept=lambda r: n_active(r, 0) == 1 and r["stages"]["side"][0][4] != 0, note="a row and the bound of entry 4 both active"),
    Row("more_rows_than_vars", (2, 1, [leaf(2), leaf(2)]), [3, 1, 1], {0: ["cut", "loose", "cut", "loose", "loose"]}, bounds=BC.frac(0.0),
        accept=lambda r: n_active(r, 0) == 2, note="nz = 3, nc = 5, two rows active"),
    Row("equality_row", (3, 2, [leaf(2)]), [3, 1], {0: ["eq", "cut"]}, accept=lambda r: n_active(r, 0) == 2),
    Row("leaf_rows", (3, 2, [leaf(3)]), [1, 3], {1: ["cut", "loose"]}, accept=lambda r: n_active(r, 1) == 1, note="nu = 0: D is empty"),
    Row("swap", (3, 2, [leaf(2), leaf(2)]), [3, 1, 1], {0: ["cut", "cut", "cut"]}, bounds=BC.frac(0.4),
        accept=lambda r: r["drops"] >= 1, note="the reference's active-set run on the root drops a member (a partial step)"),
    Row("nz64", (40, 24, [leaf(4)]), [3, 1], {0: ["cut"]}, accept=lambda r: n_active(r, 0) == 1),
    Row("nc64", (5, 3, [leaf(3)]), [3, 1], {0: ["cut", "cut", "cut"] + ["loose"] * 61}, bounds=BC.frac(0.0),
        accept=lambda r: 1 <= n_active(r, 0) <= 8),
    Row("mixed", _MIXED, [3, 0, 2, 1, 3, 2, 1], {0: ["cut", "loose"], 4: ["cut"]},
        bounds=BC.per_node({0: BC.frac(0.3), 1: BC.frac(0.5, only_u=(1,)), 2: BC.frac(0.4)}),
        accept=lambda r: n_active(r, 0) >= 1 and n_active(r, 4) == 1, full=True, note="kinds 3, 0, 2, 1 in one 7-node tree"),
    Row("x0_elim", (0, 4, [(5, 3, [leaf(3)])]), [3, 2, 1], {0: ["cut", "loose"]}, bounds=BC.per_node({0: dict(cut=[1]), 1: dict(cut=[6])}),
        accept=lambda r: n_active(r, 0) == 1, full=True, note="root nx = 0: the rows are D's alone"),
]
ROW_IDS = [r.id for r in ROWS]
FULL_IDS = [r.id for r in ROWS if r.full]


def row(rid):
    return ROWS[ROW_IDS.index(rid)]


def draw_rows(d, kinds, lam, recipe, seed, loose_only=False):
    """the row recipe of the module docstring -> d["nc"], C, D, dmin, dmax"""
    rng = np.random.Generator(np.random.PCG64(seed + 57))
    st = N.stage_solutions(d, lam, kinds=G._kinds2(kinds))
    cons = []
    for k in range(len(kinds)):
        spec = recipe.get(k)
        if not spec:
            cons.append(None)
            continue
        z = st["z"][k].astype(np.float64)
        Gk = rng.standard_normal((len(spec), len(z)))
        act = Gk @ z
        dlo, dhi = act - 5.0 - np.abs(act), act + 5.0 + np.abs(act)
        for r, what in enumerate(spec):
            up, amt = rng.random() < 0.5, 0.05 + 0.25 * rng.random()
            if loose_only or what == "loose":
                continue
            if what == "eq":
                dlo[r] = dhi[r] = act[r] + 0.1
            elif up:
                dhi[r] = act[r] - amt
            else:
                dlo[r] = act[r] + amt
        cons.append((Gk, dlo, dhi))
    return G.set_cons(d, cons)


def build(r, s, loose_only=False):
    nlam = int(flatten(r.shape)[1][1:].sum())
    lam0 = N.seeded_duals(nlam, s)
    d = BC.base_problem(r.shape, G._kinds2(r.kinds), 5)
    BC.draw_bounds(d, G._kinds2(r.kinds), lam0, r.bounds, 5)
    draw_rows(d, r.kinds, lam0, r.rows, 5 + s, loose_only)
    return d, lam0


FULL_TOL = 1e-8       # stationarity tolerance of the whole solves (see reference_solve)


def reference_solve(d, kinds, lam0=None, tol=FULL_TOL, max_iter=50, reg=1e-8):
    """box_cases.reference_solve on gen_ref's step: (iterations, trials, residual, lam, guard).  guard = dict(slack, margin, clear):
    the smallest Armijo slack of the decisions made, the smallest margin of the iterates, and whether every termination decision
    kept a factor 4 from tol.

    Why the whole solves use tol = 1e-8 and not 1e-10: the dual of these small problems is piecewise quadratic, so one Newton
    step inside the final region takes the residual from e to about 1e-7 e (what the regularisation 1e-8 leaves).  A further
    iteration from a residual below 1e-5 has an Armijo slack of 1e-16 .. 1e-19 of the dual value: the float64 sums of the device
    (and of the reference C code) then decide it by rounding, may reject all 50 trials and repeat the iteration -- the count is not
    a property of the method any more.  An iteration count is therefore pinned only on solves whose every decision is clear
    (`qualifies`), as box_cases pins a trial count only above SLACK_MIN."""
    lam = np.zeros(int(np.asarray(d["nx"])[1:].sum())) if lam0 is None else np.array(lam0, dtype=float)
    trials = 0
    guard = dict(slack=np.inf, margin=np.inf, clear=True)
    for it in range(max_iter + 1):
        ref = G.newton_step(d, lam, kinds, reg=reg)
        err = float(np.max(np.abs(ref["res"]))) if len(ref["res"]) else 0.0
        guard["margin"] = min(guard["margin"], ref["margin"])
        guard["clear"] = guard["clear"] and (err <= tol / 4 or err >= 4 * tol) and ref["condS"] <= COND_MAX
        if err <= tol or it == max_iter:
            return it, trials, err, lam, guard
        t, slack = G.armijo_trials(d, lam, ref["dlam"], ref["res"], BC.LsOpts, kinds)
        guard["slack"] = min(guard["slack"], slack)
        trials += t
        lam = lam + BETA ** (t - 1) * ref["dlam"]


def qualifies(sol):
    """a reference solve whose iteration count the device must reproduce: it converged after at least one iteration, every Armijo
    decision kept SLACK_MIN, every iterate GAP, every termination decision a factor 4"""
    it, _, err, _, g = sol
    return it >= 1 and err <= FULL_TOL / 4 and g["slack"] >= SLACK_MIN and g["margin"] >= GAP and g["clear"]


def clear_start(d, kinds):
    """(lam_start, reference solve from there): the first of the seeded starting duals, from far to near the solution (scale 1,
    0.3, 0.1, 0.03 around it, 4 seeds each), whose reference solve qualifies"""
    lam_opt = reference_solve(d, kinds, tol=1e-10)[3]
    for scale in (1.0, 0.3, 0.1, 0.03):
        for s in range(4):
            lam = lam_opt + N.seeded_duals(len(lam_opt), 50 + s, scale)
            try:
                sol = reference_solve(d, kinds, lam0=lam)
            except ValueError:
                continue
            if qualifies(sol):
                return lam, sol
    raise AssertionError("no starting duals whose reference solve qualifies")


@functools.lru_cache(maxsize=None)
def full_start(rid):
    """clear_start of row rid's problem"""
    c = case(rid)
    return clear_start(c["d"], c["kinds"])


@functools.lru_cache(maxsize=None)
def case(rid):
    """dict(row, d, kinds, lam0, seed, ref, trials, slack, lam1, st1, xu_pin) as box_cases.case, on gen_ref's step"""
    r = row(rid)
    for s in range(TRIES):
        d, lam0 = build(r, s)
        G.STATS["drops"] = 0
        try:
            ref = G.newton_step(d, lam0, r.kinds)
        except ValueError:                                   # a stage QP of this draw is infeasible
            continue
        ref["drops"] = G.STATS["drops"]
        if not (ref["margin"] >= GAP and ref["cond"] <= COND_MAX and ref["condS"] <= COND_MAX):
            continue
        if r.accept is not None and not r.accept(ref):
            continue
        try:
            trials, slack = G.armijo_trials(d, lam0, ref["dlam"], ref["res"], BC.LsOpts, r.kinds)
            lam1 = lam0 + BETA ** (trials - 1) * ref["dlam"]
            st1 = G.stage_solutions(d, lam1, r.kinds)
            if r.full and reference_solve(d, r.kinds, tol=1e-10)[2] > 1e-10:          # (the whole QP is feasible)
                continue
        except ValueError:
            continue
        assert ref["margin"] >= GAP and ref["cond"] <= COND_MAX and ref["condS"] <= COND_MAX
        return dict(row=r, d=d, kinds=r.kinds, lam0=lam0, seed=s, ref=ref, trials=trials, slack=slack, lam1=lam1, st1=st1,
                    xu_pin=bool(st1["margin"] >= GAP and st1["condS"] <= COND_MAX and slack >= SLACK_MIN))
    raise AssertionError(f"row {rid}: none of the {TRIES} seeds meets the row's conditions")


@functools.lru_cache(maxsize=None)
def loose_case(rid):
    """the problem of case(rid) with every range wide (no row can be active): (d, kinds, lam0, lam_start), lam_start the
    clear_start of a whole solve"""
    c = case(rid)
    d, lam0 = build(c["row"], c["seed"], loose_only=True)
    return d, c["kinds"], lam0, clear_start(d, c["kinds"])[0]


def container_of(capi, d):
    """capi.TreeQp with the problem d (dense objective, bounds, rows)"""
    nk, nx, nu = d["nk"], d["nx"], d["nu"]
    qp = capi.TreeQp(nx, nu, nk, d["nc"])
    xo, uo = offsets(d)
    H = BC._node_blocks(d)
    cons = G.cons_of(d)
    dad = P.parents_of(nk)
    ao = bo = lo = 0
    for k in range(len(nk)):
        a = int(nx[k])
        qp.set_node_objective(k, H[k][:a, :a], H[k][a:, a:], H[k][a:, :a], d["q"][xo[k]:xo[k + 1]], d["r"][uo[k]:uo[k + 1]])
        qp.set_node_bounds(k, d["xmin"][xo[k]:xo[k + 1]], d["xmax"][xo[k]:xo[k + 1]], d["umin"][uo[k]:uo[k + 1]], d["umax"][uo[k]:uo[k + 1]])
        if cons[k] is not None:
            Gk, dlo, dhi = cons[k]
            qp.set_node_general_constraints(k, Gk[:, :a], Gk[:, a:], np.asarray(dlo, float), np.asarray(dhi, float))
        if k > 0:
            p = dad[k]
            na, nb = nx[k] * nx[p], nx[k] * nu[p]
            qp.set_edge_dynamics(k - 1, d["A"][ao:ao + na], d["B"][bo:bo + nb], d["b"][lo:lo + nx[k]])
            ao += na; bo += nb; lo += nx[k]
    return qp


def infeasible_pair():
    """(bad, good, kinds): root nz = 2 with box [0, 1]^2 and the row z0 + z1 >= 3 (no point meets it); `good` asks for z0 + z1 >= 1.5"""
    shape, kinds = (1, 1, [leaf(1)]), np.array([3, 1], np.int32)
    good = BC.base_problem(shape, G._kinds2(kinds), 9)
    good["xmin"][:], good["xmax"][:] = [0.0, -1e12], [1.0, 1e12]
    good["umin"][:], good["umax"][:] = 0.0, 1.0
    row1 = np.array([[1.0, 1.0]])
    G.set_cons(good, [(row1, np.array([1.5]), np.array([1e12])), None])
    bad = {k: np.array(v, copy=True) for k, v in good.items()}
    G.set_cons(bad, [(row1, np.array([3.0]), np.array([1e12])), None])
    return bad, good, kinds


def scaled_one_row(n_nodes=85):
    """one_row's node data repeated on a tree of n_nodes nodes (root, then 4 children per node: 1 + 4 + 16 + 64 = 85): every node
    with children is a kind-3 node with one row, the leaves dense unconstrained.  For timing only."""
    shape = (2, 1, [(2, 1, [(2, 1, [leaf(2)] * 4)] * 4)] * 4)
    nk = flatten(shape)[0]
    assert len(nk) == n_nodes
    kinds = np.where(np.asarray(nk) > 0, 3, 1).astype(np.int32)
    lam0 = np.zeros(int(flatten(shape)[1][1:].sum()))
    d = BC.base_problem(shape, G._kinds2(kinds), 5)
    BC.draw_bounds(d, G._kinds2(kinds), lam0, BC.frac(0.25), 5)
    draw_rows(d, kinds, lam0, {k: ["cut"] for k in np.flatnonzero(kinds == 3)}, 5)
    return d, kinds

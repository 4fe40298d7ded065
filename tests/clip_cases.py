"""The case table of the clipping stage's bound rule (phase S of the dual Newton method: x = ub when xUnc >= ub, x = lb when
xUnc <= lb, otherwise free; the entry's elimination weight P is 0 exactly when it is not free -- dveccl_mask,
dual_Newton_tree_clipping.c:212-224): problems whose unconstrained stage values sit EXACTLY on a bound, built on the CPU and
shared by test_clip_reference.py (every row is what it claims, checked without a device) and test_gpu_clip_step.py (the device
pins).  An implementation that says `>` where the rule says `>=` exports the same x and u; only P moves, and with it the dual
Hessian and the Newton step.

How a tie is made exact.  The data are dyadic: Qd in {1, 2, 4}, Rd in {1/2, 1, 2}, every entry of A, B, q, r and lambda0 an
integer times 2^-3.  Every term of h_p = [lambda_p - q_p - sum A_k'lambda_k | -r_p - sum B_k'lambda_k] is then an integer times
2^-6 of size below 2^4, every partial sum of them in any order (fused or not) is exact in float64, and so is unc = h / w.
The bounds are data: a tied entry gets its bound from the exact unc.  The kinds of tie (`mode`):
    ub, lb      the upper (lower) bound IS unc: fixed
    eq          lb = ub = unc: fixed (the reference takes the upper branch first)
    ub0, lb0    as ub, lb with q_j (r_j) moved so that unc is 0.0 (a bound of 0 met from a cold start)
    ub_in       ub = nextafter(unc, +inf): one unit in the last place inside, FREE;  lb_in its mirror
    ub_out      ub = nextafter(unc, -inf): one unit outside, fixed;                 lb_out its mirror
The other side of a tied entry (`far`) is 5 + |unc| away ("wide"), an IEEE infinity ("inf") or the project's P.INF ("INF").
A root state has xmin = xmax = x0; the only tie there is eq (x0_j = unc_j).  Every entry without a tie keeps margin > GAP, the
rule of reg_cases.py: states unbounded (-+P.INF), inputs within -+UBOUND.

A row is (route, problem, ties, what it is for).  The routes are reg_cases.ROUTES and three more: gpersist_sweep1, g_persist
with TREEQP_AMD_NO_STAGE16 (one node per wave: the stage body of the launch-per-phase kernels inside g_persist; plain gpersist
takes the packed sweep, four nodes per wave, on every tree of the table), mixed (a dense mirror with kind 0 and kind 1 nodes
alternating by depth, ties on the kind-0 nodes: their clipped weights enter the blocks of kind-1 parents), and the cold-start
rows: the spring-mass tree with umin = 0, r = 0, lambda0 = 0 and a dyadic x0, where EVERY input ties in the first iteration.
Two more tables follow the rows: trial_case, ties at an accepted trial point (the trial sweep of the tiered and persistent kernels
is phase S of the next iteration), and sens_case, ties at a solution (the MPC sensitivities freeze the active set there).

Importing this module does not load the native library; cold_case takes the oracle module for the reference's own LTI fill."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import newton_ref as N
import reg_cases as RC
import reg_ref as R
from helpers import oracle_flat_from_lti, rel_err, with_dense_blocks
from limit_shapes import flatten
from treeqp_amd import problems as P

GAP, COND_MAX, TOL = RC.GAP, RC.COND_MAX, RC.TOL
UBOUND = 5.0
K = 6                       # every term of every h_p is an integer times 2^-K
DISCRIMINATION = 1e4 * TOL  # the exclusive rule must move the step by this much (helpers.rel_err), per group of ties
OPTS = RC.DEFAULTS          # the solver's defaults: ON_THE_FLY, 1e-6 / 1e-6; no block of a row is flagged

ROUTES = dict(RC.ROUTES)
ROUTES["gpersist"] = ({}, 3, dict(gpersist=True, gp_state_lds=True, gp_small16=True, wide=False))
ROUTES["gpersist_sweep1"] = (dict(TREEQP_AMD_NO_STAGE16="1"), 3, dict(gpersist=True, gp_state_lds=True, gp_small16=False, wide=False))
ROUTES["mixed"] = (dict(TREEQP_AMD_PATH="generic"), 0, dict(dense=True, box=False, wide=False))
ENV_KEYS = ("TREEQP_AMD_PATH", "TREEQP_AMD_NO_PERSIST_ONE", "TREEQP_AMD_NO_WIDE3", "TREEQP_AMD_NO_STAGE16")

FIXED = ("ub", "lb", "eq", "ub0", "lb0", "ub_out", "lb_out")
EXACT = ("ub", "lb", "eq", "ub0", "lb0")           # the ties proper: the modes on which `>=` and `>` differ
UPPER, LOWER = ("ub", "ub0"), ("lb", "lb0")


# ---------------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------------

def dims(name):
    if name in RC.SHAPES:
        return flatten(RC.SHAPES[name])
    nk = P.multistage_nk(2, RC.UNIFORM[name], RC.UNIFORM[name])
    return nk, np.full(len(nk), 4, np.int32), np.where(nk > 0, 3, 0).astype(np.int32)


@functools.lru_cache(maxsize=None)
def base_problem(name, seed=17):
    """the dyadic clipping QP on the tree `name` (a shape of reg_cases) and its dyadic lambda0, before any tie"""
    nk, nx, nu = dims(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    dad = P.parents_of(nk)
    Nn = len(nk)
    eighths = lambda lo, hi, n: rng.integers(lo, hi + 1, n).astype(np.float64) / 8.0
    A, B = [], []
    for k in range(1, Nn):
        p = dad[k]
        Ak = eighths(-2, 2, (nx[k], nx[p]))
        Ak[np.arange(min(nx[k], nx[p])), np.arange(min(nx[k], nx[p]))] += 0.5
        Bk = eighths(-6, 6, (nx[k], nu[p]))
        A.append(Ak.ravel(order="F")); B.append(Bk.ravel(order="F"))
    sx, su, sl = int(nx.sum()), int(nu.sum()), int(nx[1:].sum())
    xmin, xmax = -P.INF * np.ones(sx), P.INF * np.ones(sx)
    x0 = eighths(-4, 4, nx[0])
    xmin[:nx[0]] = x0
    xmax[:nx[0]] = x0
    d = dict(nk=nk, nx=nx, nu=nu, A=np.concatenate(A), B=np.concatenate(B), b=eighths(-2, 2, sl),
             Qd=2.0 ** rng.integers(0, 3, sx), Rd=2.0 ** rng.integers(-1, 2, su), q=eighths(-4, 4, sx), r=eighths(-4, 4, su),
             xmin=xmin, xmax=xmax, umin=-UBOUND * np.ones(su), umax=UBOUND * np.ones(su))
    return d, eighths(-3, 3, sl)


def _copy(d):
    return {k: np.array(v, copy=True) for k, v in d.items()}


def _slot(d, k, e):
    """entry e of [x_k | u_k] (negative: from the end) -> (is_x, flat index, e >= 0)"""
    nx, nu = int(d["nx"][k]), int(d["nu"][k])
    e = e % (nx + nu)
    if e < nx:
        return True, int(np.sum(d["nx"][:k])) + e, e
    return False, int(np.sum(d["nu"][:k])) + e - nx, e


def unconstrained(d, lam0):
    """per node unc = h / w in float64 on the diagonal weights (what a clipping node takes; a kind-1 node of a mixed row has no
    use for it), term after term in the order of newton_ref.stage_data: test_clip_reference.py shows that no order of the sums
    gives anything else"""
    _, H, hs, _, _ = N.stage_data(d, lam0)
    return [np.asarray(h, dtype=np.float64) / np.asarray(Hk, dtype=np.float64) for Hk, h in zip(H, hs)]


def tied(base, lam0, ties):
    """a copy of `base` with the bounds of `ties` (node, entry, mode, far) set from the exact unconstrained values at lam0"""
    d = _copy(base)
    zu = unconstrained(d, lam0)
    for k, e, mode, far in ties:                      # unc = 0.0 first: the linear term takes what h holds
        if mode.endswith("0"):
            isx, i, e = _slot(d, k, e)
            w = (d["Qd"] if isx else d["Rd"])[i]
            (d["q"] if isx else d["r"])[i] += zu[k][e] * w
    zu = unconstrained(d, lam0)
    for k, e, mode, far in ties:
        isx, i, e = _slot(d, k, e)
        lo, hi = (d["xmin"], d["xmax"]) if isx else (d["umin"], d["umax"])
        v = zu[k][e]
        if mode.endswith("0"):
            assert v == 0.0
            v = 0.0                                   # (+0.0, whatever sign the sum left)
        assert k > 0 or not isx or mode == "eq", "a root state is fixed by x0: eq is its only tie"
        off = {"wide": 5.0 + abs(v), "inf": np.inf, "INF": P.INF}[far]
        if mode == "eq":
            lo[i] = hi[i] = v
            continue
        up = mode.startswith("ub")
        bound = {"": v, "0": v, "_in": np.nextafter(v, np.inf if up else -np.inf), "_out": np.nextafter(v, -np.inf if up else np.inf)}[mode[2:]]
        if up:
            hi[i], lo[i] = bound, -off
        else:
            lo[i], hi[i] = bound, off
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------

class Row:
    def __init__(self, route, problem, ties, note, detail="", kinds=None):
        self.id = f"{route}-{problem}" + (f"-{detail}" if detail else "")
        self.route, self.problem, self.ties, self.note, self.kinds = route, problem, tuple(ties), note, kinds
        self.cold = False

    @property
    def key(self):
        """rows of different routes on the same problem, ties and kinds share one reference"""
        return (self.problem, self.ties, None if self.kinds is None else tuple(int(v) for v in self.kinds))

    def groups(self):
        """name -> the exact ties (node, entry) of the group: the upper ones, the lower ones, the equal ones, each alone"""
        ex = [(k, e, m) for k, e, m, _ in self.ties if m in EXACT]
        out = {"upper": [(k, e) for k, e, m in ex if m in UPPER], "lower": [(k, e) for k, e, m in ex if m in LOWER],
               "equal": [(k, e) for k, e, m in ex if m == "eq"]}
        out.update({f"{m}@{k}[{e}]": [(k, e)] for k, e, m in ex})
        return {n: g for n, g in out.items() if g}


def T(k, e, mode, far="wide"):
    return (k, e, mode, far)


def _ulps(k, nx):
    """neighbours one unit in the last place inside (free) and outside (fixed) of either bound, on states 1, 2 and inputs 0, 1 of node k"""
    return [T(k, 1, "ub_in"), T(k, 2, "lb_out"), T(k, nx, "lb_in"), T(k, nx + 1, "ub_out")]


# The ties of a row are spread thinly.  A fixed state is an equality on the inputs of its ancestors: where the fixed states of a
# subtree outnumber the free inputs above them the constraints are dependent and the dual Hessian singular (the rows of
# reg_cases.py are built that way on purpose; here no block may be flagged and the QP must stay feasible for the whole solves).
# Over a row the first and the last entry of a node's [x | u] and both sides of the x / u boundary are each tied somewhere, and
# there are ties from above and from below, on the root, on interior nodes and on leaves (nu = 0).
def _rows():
    rows = []
    # "tree": 0 (3, 2) | 1 2 (4, 2) | 3..6 (3, 2) | 7..14 (3, 1) | 15..30 (leaves of nx 2)
    t_tree = [T(0, 2, "eq"), T(0, 3, "ub"), T(1, 5, "ub", "inf"), T(4, 0, "lb"), T(4, 3, "lb", "inf"), T(6, 2, "ub", "INF"), T(9, 3, "lb0"),
              T(12, 0, "ub0", "inf"), T(15, 0, "ub"), T(30, 1, "lb", "INF"), T(8, 1, "eq")] + _ulps(2, 4)
    # the packed sweep takes nodes 4 w .. 4 w + 3 on the four quarters of wave w: one tie in every quarter, on wave 0 (nodes 0..3),
    # on later waves (12, 9, 10, 7) and in the last, partly filled group (28, 29, 30 on wave 7)
    t_quarters = [T(0, 4, "lb"), T(1, 4, "ub"), T(2, 3, "lb"), T(3, 0, "ub"), T(12, 0, "lb"), T(9, 2, "ub"), T(10, 3, "lb"), T(7, 3, "ub"),
                  T(28, 0, "ub"), T(29, 1, "lb"), T(30, 0, "lb")]
    for route in ("generic", "gpersist", "gpersist_sweep1"):
        rows.append(Row(route, "tree", t_tree, "root, interior nodes, leaves; ulp neighbours, zeros, equal bounds"))
    rows.append(Row("gpersist", "tree", t_quarters, "a tie in every quarter of the packed sweep's waves", detail="quarters"))
    # "gtree": 94 nodes: 0 (3, 2) | 1..3 (4, 2) | 4..9 (3, 2) | 10..21 (3, 2) | 22..45 (3, 1) | 46..93 (leaves of nx 2)
    t_g = [T(0, 2, "eq"), T(0, 4, "ub"), T(2, 0, "lb", "inf"), T(2, 5, "ub"), T(9, 2, "ub", "INF"), T(9, 3, "lb"), T(21, 0, "ub0"),
           T(45, 3, "lb0", "inf"), T(46, 0, "lb"), T(93, 1, "ub", "INF"), T(64, 0, "ub"), T(70, 1, "lb")] + _ulps(5, 3)
    rows.append(Row("generic", "gtree", t_g, "more than 64 nodes"))
    rows.append(Row("gpersist", "gtree", t_g, "more than 64 nodes: the sweep's rounds past the first, grouped levels"))
    # uniform binary trees of nx = 4, nu = 3; children of i: 2 i + 1, 2 i + 2.  "u3": 0 | 1 2 | 3..6 | 7..14 (leaves)
    t_u3 = [T(0, 3, "eq"), T(0, 4, "ub"), T(1, 0, "lb", "inf"), T(1, 6, "ub", "INF"), T(4, 3, "ub"), T(4, 4, "lb"), T(5, 5, "lb0"), T(6, 0, "ub0"),
            T(7, 0, "ub"), T(14, 3, "lb", "inf")] + _ulps(2, 4)
    rows.append(Row("tiered", "u3", t_u3, "one tier"))
    rows.append(Row("persist_one", "u3", t_u3, "one tier"))
    # "u6": tiers of block levels 3..5 | 0..2: nodes 3..6 (depth 2) are the last level of the top tier, 7..14 the first of the
    # bottom tier (their x goes to the parent workgroup together with its clipped weight), 63..126 the leaves
    t_u6 = [T(0, 3, "eq"), T(0, 6, "lb"), T(3, 0, "ub"), T(3, 4, "lb", "inf"), T(6, 3, "lb", "INF"), T(6, 6, "ub"), T(7, 0, "lb"), T(7, 6, "ub", "inf"),
            T(14, 3, "ub"), T(14, 4, "lb"), T(31, 0, "ub0"), T(31, 5, "lb0"), T(63, 0, "ub"), T(126, 3, "lb", "INF"), T(33, 2, "eq")] + _ulps(8, 4)
    for route in ("tiered", "persist_one", "persist_two"):
        rows.append(Row(route, "u6", t_u6, "both sides of the tier boundary, root, leaves"))
    # "wtree": 0 (4, 2) | 1..3 (6, 2) | 4..9 (3, 2) | 10..21 (3, 1) | 22..45 (leaves of nx 2): the wide class
    t_w = [T(0, 3, "eq"), T(0, 4, "lb"), T(1, 0, "ub"), T(1, 7, "lb", "inf"), T(3, 6, "ub"), T(3, 7, "lb", "INF"), T(4, 0, "lb0"), T(6, 4, "ub0", "inf"),
           T(10, 2, "lb", "INF"), T(10, 3, "ub"), T(11, 1, "eq"), T(26, 0, "lb"), T(45, 1, "ub", "INF")] + _ulps(7, 3)
    for route in ("wide", "wide3"):
        rows.append(Row(route, "wtree", t_w, "a parent's own stage QP and its leaf children's (k_sgp stages both)"))
    # the dense mirror: kinds 0, 1, 0, 1, 0 by depth on "tree"; the ties on kind-0 nodes at depths 0, 2 and 4
    nk = dims("tree")[0]
    dad = P.parents_of(nk)
    depth = np.zeros(len(nk), int)
    for k in range(1, len(nk)):
        depth[k] = depth[dad[k]] + 1
    kinds = (depth % 2).astype(np.int32)
    t_m = [T(0, 2, "eq"), T(0, 3, "ub"), T(3, 0, "lb"), T(3, 4, "ub", "inf"), T(6, 2, "ub", "INF"), T(6, 3, "lb"), T(5, 0, "ub0"), T(5, 4, "lb0"),
           T(15, 0, "ub"), T(30, 1, "lb", "inf"), T(18, 1, "eq")] + _ulps(4, 3)
    rows.append(Row("mixed", "tree", t_m, "kind-0 nodes between kind-1 neighbours: clipped weights in the blocks of dense parents", kinds=kinds))
    return rows


ROWS = _rows()
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)
# cold-start rows: id -> (route, tree).  A uniform spring-mass tree takes the persistent launch by default; the single-workgroup
# kernel gets a multistage tree (md = 2, Nr = 2, Nh = 3: 11 nodes) under the switch that takes the persistent launch away.
ROUTES["gpersist_cold"] = (dict(TREEQP_AMD_PATH="tiered"), 3, ROUTES["gpersist"][2])
ROUTES["gpersist_sweep1_cold"] = (dict(TREEQP_AMD_PATH="tiered", TREEQP_AMD_NO_STAGE16="1"), 3, ROUTES["gpersist_sweep1"][2])
COLD = {"generic-cold_start": ("generic", (2, 3, 3)), "gpersist-cold_start": ("gpersist_cold", (2, 2, 3)),
        "gpersist_sweep1-cold_start": ("gpersist_sweep1_cold", (2, 2, 3)), "tiered-cold_start": ("tiered", (2, 3, 3)),
        "persist_one-cold_start": ("persist_one", (2, 3, 3)), "persist_two-cold_start": ("persist_two", (2, 3, 3))}
COLD_IDS = list(COLD)
BATCH_IDS = ["persist_one-u6", "gpersist-tree", "wide3-wtree"]


def row(rid):
    return ROWS[ROW_IDS.index(rid)]


def exact_mask(d, pairs, value=False):
    """per node a boolean array over [x | u]: `value` on the entries `pairs`, the opposite elsewhere (newton_ref's `inclusive`)"""
    m = [np.full(int(a) + int(b), not value) for a, b in zip(d["nx"], d["nu"])]
    for k, e in pairs:
        m[k][e % len(m[k])] = value
    return m


def untied_margin(d, lam0, pairs, kinds=None):
    """the smallest distance of an unconstrained value to a bound over the entries of clipping nodes that are not in `pairs`
    and whose bounds differ"""
    zu = unconstrained(d, lam0)
    skip = exact_mask(d, pairs, True)
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    best = np.inf
    for k, z in enumerate(zu):
        if kinds is not None and kinds[k] != 0:
            continue
        lo = np.concatenate([d["xmin"][xo[k]:xo[k + 1]], d["umin"][uo[k]:uo[k + 1]]])
        hi = np.concatenate([d["xmax"][xo[k]:xo[k + 1]], d["umax"][uo[k]:uo[k + 1]]])
        use = (lo < hi) & ~skip[k]
        if np.any(use):
            best = min(best, float(np.min(np.minimum(np.abs(z - lo), np.abs(z - hi))[use])))
    return best


def _step(d, lam0, kinds, inclusive=True):
    dd = with_dense_blocks(d) if kinds is not None else d
    return R.block_newton_step(dd, lam0, **OPTS, kinds=kinds, inclusive=inclusive, check=False)          # (xcheck of the reference step: asserted by test_clip_reference.py)


def _wrong_step(d, lam0, kinds, inclusive):
    """the step with the exclusive rule on some entries: the longdouble system of newton_ref.assemble, solved in float64 (good to
    cond * 2^-53, some 1e-10; it is compared with a step that must differ by 1e-6)"""
    dd = with_dense_blocks(d) if kinds is not None else d
    M, res, _ = N.assemble(dd, lam0, kinds=kinds, inclusive=inclusive)
    return np.linalg.solve(M.astype(np.float64), res.astype(np.float64))


def _finish(d, lam0, kinds, ties, groups):
    ref = _step(d, lam0, kinds)
    dd = with_dense_blocks(d) if kinds is not None else d
    trials, slack = R.armijo(dd, lam0, ref, RC.LsOpts, kinds=kinds)
    moved = {"all": rel_err(_wrong_step(d, lam0, kinds, False), ref["dlam"])}
    for name, pairs in groups.items():
        moved[name] = rel_err(_wrong_step(d, lam0, kinds, exact_mask(d, pairs)), ref["dlam"])
    margin = untied_margin(d, lam0, [(k, e) for k, e, _, _ in ties], kinds)
    return dict(d=d, dd=dd, lam0=lam0, kinds=kinds, ref=ref, trials=trials, slack=slack, moved=moved, margin=margin, ties=ties)


@functools.lru_cache(maxsize=None)
def _case(key):
    r = next(r for r in ROWS if r.key == key)
    base, lam0 = base_problem(r.problem)
    d = tied(base, lam0, r.ties)
    c = _finish(d, lam0, r.kinds, r.ties, r.groups())
    # the untied twin of the batch test: every bound of a tied entry moved out by GAP
    twin = _copy(d)
    for k, e, mode, far in r.ties:
        isx, i, _ = _slot(d, k, e)
        lo, hi = (twin["xmin"], twin["xmax"]) if isx else (twin["umin"], twin["umax"])
        lo[i] -= GAP; hi[i] += GAP
    c.update(base=base, twin=twin)
    return c


def case(rid):
    """dict(d, dd, lam0, kinds, ref, trials, slack, moved, margin, ties, base, twin): the tied problem (dd: with dense blocks where
    the row has kinds), the row's lambda0, the reference step there under the inclusive rule (reg_ref.block_newton_step with the
    solver's default options), the reference's line search, how far the step moves under the exclusive rule (all entries, and per
    group of Row.groups), the margin of the untied entries, the dyadic problem before the ties, the untied twin"""
    return _case(row(rid).key)


_COLD = {}


def cold_case(orc, tree=(2, 3, 3)):
    """the cold-start problem: spring-mass tree (md, Nr, Nh) = tree (default: 15 nodes; the reference's own LTI fill through the oracle),
    umin = 0, r = 0, lambda0 = 0, x0 dyadic: h_u = -r - sum B'lambda is 0.0 at every parent, a tie with umin = 0 everywhere"""
    if tree not in _COLD:
        p = P.spring_mass(md=tree[0], Nr=tree[1], Nh=tree[2])
        p.x0 = np.resize(np.array([0.5, -0.25, 0.75, -0.5]), p.nx)
        p.r = np.zeros_like(p.r)
        p.umin = np.zeros_like(p.umin)
        d = {k: np.array(v, copy=True) for k, v in oracle_flat_from_lti(orc, p).items()}
        lam0 = np.zeros(int(d["nx"][1:].sum()))
        ties = tuple((k, int(d["nx"][k]) + j, "lb0", "wide") for k in range(len(d["nk"])) for j in range(int(d["nu"][k])))
        _COLD[tree] = _finish(d, lam0, None, ties, {"lower": [(k, e) for k, e, _, _ in ties]})
    return _COLD[tree]


# ---------------------------------------------------------------------------------------------------------------------------
# a tie at an ACCEPTED TRIAL POINT (the trial sweep of the tiered and persistent kernels doubles as phase S of the next iteration)
# ---------------------------------------------------------------------------------------------------------------------------
# lambda1 = lambda0 + dlam must be exact.  With A = 0 and B rows that pick disjoint input columns with entries 1 the dual Hessian
# M = C P C' + P_x is diagonal, and the weights make every diagonal entry exactly 1 while nothing is clipped: per parent p with
# children k1, k2 row (k1, 0) picks inputs 0 and 1 (1/4 + 1/4 + 1/2), row (k2, 1) picks input 2 (1/2 + 1/2), every other row has
# its own state alone (1/1).  Then L = 1, dlam = res, and res, lambda1 and unc(lambda1) are dyadic and exact in any order.  The
# dual problem splits into one scalar problem per row.  On the parents TRIAL_PARENTS row (k1, 0) gets two bounds between lambda0
# and lambda1: one entry of the row is clipped WITH margin half way (so the residual at lambda1 is not zero and a second step is
# taken; the curvature only falls along the step, so the full step passes the Armijo test), another gets its bound from the exact
# unc(lambda1): the tie.  Kind "u": the tie is on input 0, input 1 is clipped; kind "x": the tie is on the child's state 0, input 0
# is clipped.  The second step of that row is res / M with M = 1/2 resp. 1/4 under the inclusive rule and 3/4 under the wrong one.
TRIAL_PARENTS = {"u3": ((0, "u"), (1, "x"), (3, "u"), (6, "x")), "u6": ((0, "u"), (3, "x"), (7, "u"), (8, "x"), (31, "u"), (62, "x"))}
TRIAL_ROUTES = ("tiered", "persist_one", "persist_two")
TRIAL_IDS = [f"{route}-{name}-trial" for route in TRIAL_ROUTES for name in ("u3", "u6") if not (route == "persist_two" and name == "u3")]
TRIAL_K = 8                 # the terms of h at lambda1 are integers times 2^-5; 2^-8 leaves room


@functools.lru_cache(maxsize=None)
def trial_case(name):
    """dict(d, lam0, lam1, ref1, ref2, ties, moved, margin, trials2, slack2): the problem, the exact lambda1 = lambda0 + res, the
    reference steps at lambda0 and at lambda1 (inclusive), the tied entries (node, entry, side) at lambda1, how far the second step
    moves under the exclusive rule (all ties, and each alone), the margin of every other entry at lambda0 and at lambda1"""
    nk, nx, nu = dims(name)
    rng = np.random.Generator(np.random.PCG64(29))
    eighths = lambda lo, hi, n: rng.integers(lo, hi + 1, n).astype(np.float64) / 8.0
    Nn = len(nk)
    dad = P.parents_of(nk)
    kid0 = np.concatenate([[1], 1 + np.cumsum(nk)[:-1]])
    xo, uo = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nu)])
    sx, su, sl = int(nx.sum()), int(nu.sum()), int(nx[1:].sum())
    Qd, Rd, B = np.ones(sx), np.ones(su), []
    for k in range(1, Nn):
        p = dad[k]
        Bk = np.zeros((nx[k], nu[p]))
        if k == kid0[p]:
            Bk[0, 0] = Bk[0, 1] = 1.0
            Qd[xo[k]] = 2.0
        else:
            Bk[1, 2] = 1.0
            Qd[xo[k] + 1] = 2.0
        Rd[uo[p]:uo[p] + 3] = (4.0, 4.0, 2.0)
        B.append(Bk.ravel(order="F"))
    xmin, xmax = -P.INF * np.ones(sx), P.INF * np.ones(sx)
    x0 = eighths(-4, 4, nx[0])
    xmin[:nx[0]] = x0
    xmax[:nx[0]] = x0
    d = dict(nk=nk, nx=nx, nu=nu, A=np.zeros(int(sum(nx[k] * nx[dad[k]] for k in range(1, Nn)))), B=np.concatenate(B), b=eighths(-8, 8, sl),
             Qd=Qd, Rd=Rd, q=eighths(-4, 4, sx), r=eighths(-4, 4, su), xmin=xmin, xmax=xmax, umin=-8.0 * np.ones(su), umax=8.0 * np.ones(su))
    lam0 = eighths(-3, 3, sl)
    M, res, _ = N.assemble(d, lam0)
    assert np.array_equal(M.astype(np.float64), np.eye(sl)), "the dual Hessian at lambda0 is not the identity"
    lam1 = lam0 + res.astype(np.float64)
    assert np.array_equal(N.LD(lam0) + res, N.LD(lam1))
    z0, z1 = unconstrained(d, lam0), unconstrained(d, lam1)
    ties = []
    for p, kind in TRIAL_PARENTS[name]:
        k = int(kid0[p])
        tie, cut = ((p, nx[p]), (p, nx[p] + 1)) if kind == "u" else ((k, 0), (p, nx[p]))
        for (node, e), exact in ((tie, True), (cut, False)):
            a, b_ = z0[node][e], z1[node][e]
            assert abs(b_ - a) > 1e-2, f"{name}: the row of parent {p} does not move"
            isx, i, _ = _slot(d, node, e)
            lo, hi = (d["xmin"], d["xmax"]) if isx else (d["umin"], d["umax"])
            bound = b_ if exact else 0.5 * (a + b_)
            if b_ > a:
                hi[i] = bound
            else:
                lo[i] = bound
            if exact:
                ties.append((int(node), int(e), 1 if b_ > a else -1))
    pairs = [(k, e) for k, e, _ in ties]
    ref1 = _step(d, lam0, None)
    assert np.array_equal(ref1["dlam"], res.astype(np.float64)), "the bounds moved the first step"
    ref2 = _step(d, lam1, None)
    trials2, slack2 = R.armijo(d, lam1, ref2, RC.LsOpts)
    moved = {"all": rel_err(_wrong_step(d, lam1, None, False), ref2["dlam"])}
    for k, e in pairs:
        moved[f"{k}[{e}]"] = rel_err(_wrong_step(d, lam1, None, exact_mask(d, [(k, e)])), ref2["dlam"])
    margin = min(untied_margin(d, lam0, []), untied_margin(d, lam1, pairs))
    return dict(d=d, lam0=lam0, lam1=lam1, kinds=None, ref1=ref1, ref2=ref2, ties=ties, moved=moved, margin=margin, trials2=trials2, slack2=slack2)


# ---------------------------------------------------------------------------------------------------------------------------
# a tie at a SOLUTION: the MPC sensitivity case
# ---------------------------------------------------------------------------------------------------------------------------

SENS_TIES = (T(0, 3, "ub"), T(4, 0, "lb"), T(9, 3, "lb0"), T(15, 0, "ub"))          # (0, 3): input 0 of the root; "tree", the single-workgroup kernel


@functools.lru_cache(maxsize=None)
def sens_case():
    """dict(d, twin, lam0, x0, ties): the dyadic problem on "tree" with the ties SENS_TIES at lambda0 and b chosen so that the
    dynamics residual at lambda0 is exactly zero: lambda0 IS the solution, a solve from it ends after phase S of iteration 0, and
    the point the sensitivities are taken at has its ties exactly.  twin: the tied bounds moved out by GAP (the entries are free)."""
    base, lam0 = base_problem("tree")
    d = tied(base, lam0, SENS_TIES)
    M, res, st = N.assemble(d, lam0)
    d["b"] = d["b"] - res.astype(np.float64)
    assert np.array_equal(N.LD(d["b"]), N.LD(base["b"]) - res)
    M, res, st = N.assemble(d, lam0)
    assert not np.any(res), "the residual at lambda0 is not exactly zero"
    twin = _copy(d)
    for k, e, mode, far in SENS_TIES:
        isx, i, _ = _slot(d, k, e)
        lo, hi = (twin["xmin"], twin["xmax"]) if isx else (twin["umin"], twin["umax"])
        lo[i] -= GAP; hi[i] += GAP
    x, u, sx, su = N.flat_xu(st)
    return dict(d=d, twin=twin, lam0=lam0, x0=d["xmin"][:int(d["nx"][0])].copy(), ties=SENS_TIES, x=x, u=u, cond=float(np.linalg.cond(M.astype(np.float64))))


# ---------------------------------------------------------------------------------------------------------------------------
# exactness, in rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------

def h_terms(d, lam0):
    """per node and entry of [x | u] the list of the terms of h (floats: own dual, -q or -r, the products -A_ij lambda_i)"""
    nk, nx, nu, xo, uo, dad, A, B, b, _ = N._blocks(d, False)
    lo_ = xo - nx[0]
    out = []
    for p in range(len(nk)):
        rows = []
        for e in range(nx[p] + nu[p]):
            isx = e < nx[p]
            t = [-float(d["q"][xo[p] + e])] if isx else [-float(d["r"][uo[p] + e - nx[p]])]
            if isx and p > 0:
                t.append(float(lam0[lo_[p] + e]))
            rows.append(t)
        out.append(rows)
    for k in range(1, len(nk)):
        p = dad[k]
        for i in range(nx[k]):
            l = float(lam0[lo_[k] + i])
            for e in range(nx[p] + nu[p]):
                c = float(A[k][i, e]) if e < nx[p] else float(B[k][i, e - nx[p]])
                out[p][e].append(-c * l)
    return out


def exactness(d, lam0, K=K):
    """(worst, unc_fraction, unc_forward, unc_reversed): worst is the largest absolute sum of the terms of an h entry, after
    asserting every term an integer times 2^-K; the unconstrained values from Fractions and from float64 sums in both orders"""
    terms = h_terms(d, lam0)
    w = [np.concatenate([d["Qd"][a:b], d["Rd"][c:e]]) for a, b, c, e in zip(np.cumsum(d["nx"]) - d["nx"], np.cumsum(d["nx"]), np.cumsum(d["nu"]) - d["nu"], np.cumsum(d["nu"]))]
    worst, fr, fw, rv = 0.0, [], [], []
    for p, rows in enumerate(terms):
        a, f, r_ = [], [], []
        for e, t in enumerate(rows):
            assert all(Fraction(v) * 2 ** K == int(Fraction(v) * 2 ** K) for v in t), (p, e)
            worst = max(worst, float(sum(abs(Fraction(v)) for v in t)))
            a.append(sum((Fraction(v) for v in t), Fraction(0)) / Fraction(float(w[p][e])))
            s1 = 0.0
            for v in t:
                s1 += v
            s2 = 0.0
            for v in reversed(t):
                s2 += v
            f.append(s1 / w[p][e]); r_.append(s2 / w[p][e])
        fr.append(a); fw.append(np.array(f)); rv.append(np.array(r_))
    return worst, fr, fw, rv

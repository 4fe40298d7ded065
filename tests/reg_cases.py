"""The case table of the regularised block factorisation (treeqp_dpotrf_l_with_reg_opts, phase F of the dual Newton method):
problems in which dual blocks really are singular, built on the CPU and shared by test_reg_reference.py (every row is what it
claims, checked without a device) and test_gpu_reg_step.py (the device pins).

How a block is made exactly singular with bounds alone (kernel selection does not move): a node is PINNED by xmin = xmax on its
states and umin = umax on its inputs; its elimination matrix P is then exactly 0.  With a child k and its parent p pinned, row
and column block k of block p (the duals of the children of p) are exactly zero: E P_k E', the couplings C_k P_p C_j' and the
Schur record from below (Ut = -(C P_k)_x) all vanish in exact arithmetic.  The first pass of the factorisation meets an exact 0
there, which is <= regTol and <= 0 in every implementation.  The rows of the pinned p in the block of ITS parent are
C_p P_dad C_p': p sits at depth >= 2 (its parent has free states), or p is the root.  A pinned p also fixes nx_p
combinations of its ancestors' entries, nu fewer with every level up; where they outnumber the root's inputs the root block is
singular up to rounding, and below that the system is ill-conditioned.  On uniform trees of nx = 8, nu = 3 a pinned interior
node leaves cond between 1.7e7 and 1.4e8 at every seed, past COND_MAX; the uniform rows are on nx = 4, nu = 3 (cond <= 8e5).

A row is (id = route-kind[-detail], route, problem, pins, options, the blocks the reference must flag, what it is for).  The
route says which device body the row runs:
    generic       wave-per-block factorisation of the launch-per-phase kernels (k_factor, tdunes_device.hip)
    gpersist      g_persist (tdunes_gpersist.hpp): factor_body on levels of up to 16 blocks, the "block by block" group variant
                  factor_body_g on wider levels of equal small blocks (the rows with the detail "grouped")
    dense_single  factor_body inside g_persist_dense
    tiered        potrf_rows (tdunes_fast.hpp)
    persist_one   p_factor_rows, p_factor_rows_first, p_refactor_rows, p_potrf_fast (tdunes_persist.hpp), one workgroup per CU
    persist_two   the same bodies in f_persist, two workgroups per CU
    wide          the small_flag path of tdunes_wide.hpp
    wide3         the small_flag path of k_hf_w (tdunes_wide3.hpp)

Options: OTF is ON_THE_FLY with regTol = 1e-3, regValue = 1e-2 (a shift of that size moves every entry of a flagged block
visibly and keeps cond small), DEFAULTS the solver's 1e-6 / 1e-6, ALWAYS regType 1 with 1e-2, NOREG regType 0 (the zero-column
convention).  lambda0 is the first of the 20 seeds of newton_ref.seeded_duals at which the row meets its conditions:
margin > GAP, guard >= GUARD_MIN, cond <= COND_MAX (DEFAULTS rows apart, see below), exactly the named blocks flagged.  MAPPING says,
per route, which blocks one wave or workgroup factorises one after the other.

DEFAULTS rows shift an exactly singular block by 1e-6: cond is then about 1e6 times the largest eigenvalue (5e6 to 1.5e7 here), past
the rule for a 1e-10 pin.  test_reg_reference.py measures instead how far the reference's own float64 step moves (helpers.rel_err)
over four copies of the data with every non-zero moved by one unit in the last place, and asserts that ten times that is within
1e-10: measured 1.6e-16 to 2.7e-16 (the large entries of the step, 1e5, are the well-determined ones), so these rows keep the
1e-10 pin of all the others.  Nothing in this comes from the device."""
from __future__ import annotations

import functools

import numpy as np

import newton_ref as N
import reg_ref as R
from helpers import rel_err, shaped_qp
from limit_shapes import fan, flatten, leaf
from treeqp_amd import problems as P

COND_MAX = 1e6
GAP = 1e-6
GUARD_MIN = 1.9
TRIES = 20
TOL = 1e-10
UBOUND = 5.0         # inputs wide open: a clipped input of an ancestor is one entry fewer to absorb what a pinned node fixes

OTF = dict(regType=2, regTol=1e-3, regValue=1e-2)
DEFAULTS = dict(regType=2, regTol=1e-6, regValue=1e-6)
ALWAYS = dict(regType=1, regTol=1e-6, regValue=1e-2)
NOREG = dict(regType=0, regTol=1e-6, regValue=1e-6)

ROUTES = {
    # route: (environment at tqgpu_create, tqgpu_uses_fused_path, plan flags that must hold)
    "generic": (dict(TREEQP_AMD_PATH="generic"), 0, dict(wide=False)),
    "gpersist": ({}, 3, dict(gpersist=True, gp_state_lds=True, wide=False)),
    "dense_single": ({}, 3, dict(dense=True, box=True, dense_single_wg=True)),
    "tiered": (dict(TREEQP_AMD_PATH="tiered"), 1, {}),
    "persist_one": ({}, 2, dict(persist=True, persist_one=True)),
    "persist_two": (dict(TREEQP_AMD_NO_PERSIST_ONE="1"), 2, dict(persist=True, persist_one=False)),
    # (a wide-class tree this small would take g_persist by default: TREEQP_AMD_PATH=generic keeps it on its own kernels)
    "wide": (dict(TREEQP_AMD_PATH="generic", TREEQP_AMD_NO_WIDE3="1"), 0, dict(wide=True, w3=False)),
    "wide3": (dict(TREEQP_AMD_PATH="generic"), 0, dict(wide=True, w3=True)),
}


# ---------------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------------

def _tree(root, top, last=None):
    """root -> `top` children (nx, nu) -> 2 x (3, 2) each -> 2 x (3, 1) each -> 2 leaves of nx 2 each.  Breadth first: with two
    top nodes 0 | 1 2 | 3..6 | 7..14 | 15..30, with three 0 | 1 2 3 | 4..9 | 10..21 | 22..45."""
    l3 = (3, 1, [leaf(2), leaf(2)])
    l2 = (3, 2, [l3, l3])
    return (root[0], root[1], [(n, m, [l2, l2]) for n, m in top])


def _small(first_l2):
    """root -> 2 x (nx1, 2) -> 2 x (3, 2) each -> leaves; the first (3, 2) node (node 3) has the children `first_l2`"""
    def shape(nx1):
        l2 = (3, 2, [leaf(2)])
        return (3, 2, [(nx1, 2, [(3, 2, first_l2), l2]), (nx1, 2, [l2, l2])])
    return shape


SHAPES = {
    "tree": _tree((3, 2), [(4, 2)] * 2),                       # d <= 8: launch-per-phase kernels and g_persist
    "wtree": _tree((4, 2), [(6, 2)] * 3),                      # root block d = 18: the wide class, every block on its kernels
    "one": _small([leaf(1)])(4), "wone": _small([leaf(1)])(9),          # node 3 has ONE child of nx = 1: block 3 is 1 x 1
    "twin": _small([leaf(1), leaf(1)])(4), "wtwin": _small([leaf(1), leaf(1)])(9),      # node 3 has two children of nx = 1
    "fan88": fan(8, 8), "d17": (3, 2, [(8, 2, [leaf(2)]), (9, 2, [leaf(2)])]), "fan_last1": fan(8, [8] * 7 + [1]),
}
# g_persist's grouped levels: 24 equal blocks of d = 4 on the last parent level (0 | 1..3 | 4..9 | 10..21 | 22..45 | 46..93)
_G4 = (3, 1, [leaf(2), leaf(2)])
_G3 = (3, 2, [_G4, _G4])
_G2 = (3, 2, [_G3, _G3])
SHAPES["gtree"] = (3, 2, [(4, 2, [_G2, _G2])] * 3)
# uniform binary trees of nx = 4, nu = 3 (a shape of the persistent and tiered kernels' table) with 1, 2 and 3 tiers of the
# persistent launch (3 block levels to a tier): name -> depth
UNIFORM = {"u3": 3, "u6": 6, "u7": 7}
# per problem: input bound (clipped root inputs keep the largest eigenvalue down) and a factor on every weight
UBOUND_OF = {"one": 0.3}
WEIGHTS_OF = {"wone": 4.0}           # largest eigenvalue 11 -> below 4: cond of threshold_above is lambda_max / (2 regTol)^2


@functools.lru_cache(maxsize=None)
def base_problem(name):
    """the flat clipping QP `name`, before any pin"""
    if name in SHAPES:
        nk, nx, nu = flatten(SHAPES[name])
    else:
        nk, nx, nu = P.multistage_nk(2, UNIFORM[name], UNIFORM[name]), 4, 3
    d = shaped_qp(nk, nx, nu, 11, ubound=UBOUND_OF.get(name, UBOUND)).as_dict()
    d["Qd"], d["Rd"] = d["Qd"] * WEIGHTS_OF.get(name, 1.0), d["Rd"] * WEIGHTS_OF.get(name, 1.0)
    return d


def pinned(d, pins, tweak=None):
    """a copy of d with the nodes of `pins` pinned: node -> "all", "x" (states only), "u" (inputs only) or ("u_free", j) (everything but input j,
    which gets the bounds -+5 and the weight 1).  tweak = ("L", child, j, L): entry (0, j) of the child's B (nx = 1) becomes L, so
    that with Rd_j = 1 the child's first-pass pivot is L_jj = L; ("twin", k1, k2): the rows [A B] of k2 become those of k1."""
    d = {k: np.array(v, copy=True) for k, v in d.items()}
    xo = np.concatenate([[0], np.cumsum(d["nx"])])
    uo = np.concatenate([[0], np.cumsum(d["nu"])])
    for k, how in pins.items():
        if k > 0 and how != "u":                                     # (the root's states are x0 already)
            d["xmin"][xo[k]:xo[k + 1]] = 0.0
            d["xmax"][xo[k]:xo[k + 1]] = 0.0
        if how != "x":
            d["umin"][uo[k]:uo[k + 1]] = 0.0
            d["umax"][uo[k]:uo[k + 1]] = 0.0
        if isinstance(how, tuple):
            j = uo[k] + how[1]
            d["umin"][j], d["umax"][j], d["Rd"][j] = -5.0, 5.0, 1.0
    if tweak is not None:
        dad = P.parents_of(d["nk"])
        aoff = lambda k: sum(int(d["nx"][c] * d["nx"][dad[c]]) for c in range(1, k))
        boff = lambda k: sum(int(d["nx"][c] * d["nu"][dad[c]]) for c in range(1, k))
        if tweak[0] == "L":
            _, k, j, L = tweak
            assert d["nx"][k] == 1
            d["B"][boff(k) + j] = L                                  # B_k is 1 x nu: column j
        else:
            _, k1, k2 = tweak
            p = dad[k1]
            assert dad[k2] == p and d["nx"][k1] == d["nx"][k2] == 1
            d["A"][aoff(k2):aoff(k2) + d["nx"][p]] = d["A"][aoff(k1):aoff(k1) + d["nx"][p]]
            d["B"][boff(k2):boff(k2) + d["nu"][p]] = d["B"][boff(k1):boff(k1) + d["nu"][p]]
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------

class Row:
    def __init__(self, route, kind, problem, pins, opts, flagged, note, tweak=None, detail=""):
        self.id = f"{route}-{kind}" + (f"-{detail}" if detail else "")
        self.route, self.kind, self.problem = route, kind, problem
        self.pins, self.tweak, self.opts = pins, tweak, opts
        self.flagged = sorted(flagged)
        self.note = note
        self.lift = kind == "flag_mid_level"          # the second solve with the pins lifted runs on these rows

    @property
    def key(self):
        """rows of different routes on the same problem, pins and options share one reference"""
        return (self.problem, tuple(sorted((k, str(v)) for k, v in self.pins.items())), tuple(sorted(self.opts.items())), self.tweak)


# Which blocks one wave (or workgroup) factorises one after the other, read from the kernels; the neighbours rows rely on it.
MAPPING = {
    "generic": "k_factor: a wave per block, one launch per sweep (factor_body once per wave): nothing is carried from block to block; "
               "the row has flagged and unflagged blocks in one launch",
    "wide": "k_factor_w: a workgroup per block (factor_w_body once per workgroup): as generic",
    "wide3": "k_hf_w: a workgroup per block, small_flag in its own LDS: as generic",
    "gpersist": "g_persist, levels of up to 16 blocks: wave w runs factor_body on block w of the level, level after level upwards; on "
                "'tree' wave 0 takes 7, 3, 1, 0 and wave 1 takes 8, 4, 2.  Levels of more than 16 equal small blocks: wave w runs "
                "factor_body_g on blocks 3 w .. 3 w + 2 side by side, the flagged ones redone block by block",
    "dense_single": "g_persist_dense: factor_body, block w of a level on wave w (dense trees never form groups)",
    "tiered": "f_back / f_top: the tiers of detect_fast, a workgroup per tier subtree, wave w on block first(t) + w of level t from the "
              "tier's last level up, the rows in registers (potrf_rows)",
    "persist_one": "p_run: a workgroup per tier subtree; wave w takes block first(t) + w on level t = th - 1 .. 0 with the same registers "
                   "Tc.  On 'u6' (tiers: levels 3..5 | 0..2) wave 0 of the workgroup of node 7 takes 31, 15, 7, that of node 8 takes "
                   "35, 17, 8; wave 0 of the top tier takes 3 (records reloaded by tag in p_refactor_rows), 1, 0",
    "persist_two": "as persist_one (f_persist instead of f_persist_one)",
}


def _irregular(route, t, w):
    """rows of a route that takes trees of any shape; t: "tree" or "wtree" (w = True).  Node numbers: see _tree."""
    top = 3 if w else 2
    thr = {3: ("u_free", 0), 7: "all"}
    l2 = 1 + top                            # first node of depth 2; its children start at l3, theirs at lf
    l3 = l2 + 2 * top
    lf = l3 + 4 * top
    pre = "w" if w else ""
    nb = {l3 + 1: "all", lf + 2: "all", l3 + 4: "all", lf + 8: "all", l3 + 7: "all", lf + 14: "all"}
    return [
        Row(route, "flag_leaf_level", t, {l3: "all", lf: "all"}, OTF, [l3], "a block of the last parent level, first child pinned"),
        Row(route, "flag_mid_level", t, {l2: "all", l3: "all"}, OTF, [l2],
            "block of a depth-2 node: its second child's block sends a non-zero Schur record, the pinned child's a zero one"
            + ("; wave 0 takes an unflagged block, this one, then unflagged ones" if route in ("gpersist", "dense_single") else "")),
        Row(route, "flag_root", t, {0: "all", 1: "all"}, OTF, [0], "the root block, its first row block zero"),
        Row(route, "neighbours", t, nb, OTF, [l3 + 1, l3 + 4, l3 + 7],
            "blocks 2, 5 and 8 of the last parent level flagged, the others not.  " + MAPPING[route]
            + ("; waves 1, 4 and 7 go from a flagged block to unflagged ones (flag_mid_level has the other order)" if route == "gpersist" else "")),
        Row(route, "always", t, {l2: "all", l3: "all"}, ALWAYS, range(l3 + 4 * top), "regType 1: every block shifted"),
        Row(route, "zero_column", t, {l2: "all", l3: "all"}, NOREG, [], "regType 0: the pinned child's entries of the step are 0"),
        Row(route, "defaults", t, {l2: "all", l3: "all"}, DEFAULTS, [l2], "the solver's default 1e-6 / 1e-6"),
        # node 3 of "one" / "wone": one child of nx = 1 (node 7), block 3 is 1 x 1 = B_j^2 / Rd_j
        Row(route, "threshold_below", pre + "one", thr, OTF, [3],
            "first-pass L_jj = regTol / 2 in block 3: flagged", tweak=("L", 7, 0, 0.5e-3)),
        Row(route, "threshold_above", pre + "one", thr, OTF, [],
            "first-pass L_jj = 2 regTol in block 3: not flagged", tweak=("L", 7, 0, 2e-3)),
        Row(route, "rounding_pivot", pre + "twin", {3: "u", 7: "all", 8: "all"}, OTF, [3],
            "block 3 = a P_x a' [1 1; 1 1] (node 3 pinned in its inputs only): its second pivot is zero up to rounding, either sign flags",
            tweak=("twin", 7, 8)),
    ]


def _grouped_rows():
    """g_persist on "gtree": the last parent level has 24 blocks (nodes 22..45, d = 4, R = 8), which factor_body_g takes three to a
    wave: wave 0 has 22, 23, 24, wave 1 has 25, 26, 27"""
    return [Row("gpersist", "flag_leaf_level", "gtree", {22: "all", 46: "all"}, OTF, [22], "the first block of a group of three", detail="grouped"),
            Row("gpersist", "neighbours", "gtree", {23: "all", 48: "all", 25: "all", 52: "all"}, OTF, [23, 25],
                "wave 0's group is unflagged, flagged, unflagged; wave 1's is flagged, unflagged, unflagged.  " + MAPPING["gpersist"], detail="grouped"),
            Row("gpersist", "defaults", "gtree", {23: "all", 48: "all"}, DEFAULTS, [23], "the middle block of a group at 1e-6 / 1e-6", detail="grouped")]


def _position_rows(route):
    out = [Row(route, "flag_position", "fan88", {0: "all", 1 + c: "all"}, OTF, [0], f"columns {8 * c}..{8 * c + 7} of d = 64 zero", detail=f"child{c}")
           for c in (0, 3, 7)]
    out.append(Row(route, "flag_position", "d17", {0: "all", 2: "all"}, OTF, [0], "columns 8..16 of d = 17 zero: across the edge of the first panel", detail="d17"))
    out.append(Row(route, "flag_position", "fan_last1", {0: "all", 8: "all"}, OTF, [0], "column d - 1 = 56 zero (last child, nx = 1)", detail="last1"))
    return out


def _uniform(route):
    """rows on "u6", the uniform binary tree of depth 6 with two tiers (block levels 3..5 | 0..2); children of i: 2 i + 1, 2 i + 2"""
    mid = {15: "all", 31: "all"}
    Np = int((base_problem("u6")["nk"] > 0).sum())
    return [Row(route, "flag_leaf_level", "u6", {31: "all", 63: "all"}, OTF, [31], "level 5, the last level of the bottom tier", detail="u6"),
            Row(route, "flag_mid_level", "u6", mid, OTF, [15], "level 4: records from its own workgroup, subtracted in place", detail="u6"),
            Row(route, "flag_upper_tier", "u6", {3: "all", 7: "all"}, OTF, [3],
                "level 2, the last level of the top tier: its records come from the workgroups of the bottom tier, and the reload before "
                "the second factorisation (p_sub_children_tagged) must carry them", detail="u6"),
            Row(route, "flag_root", "u6", {0: "all", 1: "all"}, OTF, [0], "the root block", detail="u6"),
            Row(route, "neighbours", "u6", {31: "all", 63: "all", 17: "all", 35: "all"}, OTF, [17, 31],
                "wave 0 of the workgroup of node 7: 31 flagged, then 15 and 7 not; of node 8: 35 not, 17 flagged, 8 not.  " + MAPPING[route], detail="u6"),
            Row(route, "always", "u6", mid, ALWAYS, range(Np), "regType 1: every block shifted", detail="u6"),
            Row(route, "zero_column", "u6", mid, NOREG, [], "regType 0: zero column", detail="u6"),
            Row(route, "defaults", "u6", mid, DEFAULTS, [15], "the solver's default 1e-6 / 1e-6", detail="u6")]


def _rows():
    rows = []
    rows += _irregular("generic", "tree", False)
    rows += _irregular("gpersist", "tree", False) + _grouped_rows()
    rows += [Row("dense_single", "flag_mid_level", "tree", {3: "all", 7: "all"}, OTF, [3],
                 "every node of kind 2 (box solver) on diagonal H: the pins are equal bounds of the stage QP")]
    for route in ("tiered", "persist_one", "persist_two"):
        rows += _uniform(route)
    # one tier (depth 3) and three tiers (depth 7: block levels 4..6 | 1..3 | 0)
    rows += [Row("persist_one", "flag_root", "u3", {0: "all", 1: "all"}, OTF, [0], "one tier", detail="u3"),
             Row("persist_one", "flag_leaf_level", "u3", {3: "all", 7: "all"}, OTF, [3], "one tier", detail="u3")]
    for route in ("tiered", "persist_one"):
        rows += [Row(route, "flag_root", "u7", {0: "all", 1: "all"}, OTF, [0], "three tiers: the top tier is the root block alone", detail="u7"),
                 Row(route, "flag_upper_tier", "u7", {7: "all", 15: "all"}, OTF, [7],
                     "three tiers: level 3 is the last level of the middle tier, its records come from the bottom tier by tag", detail="u7")]
    for route in ("wide", "wide3"):
        rows += _irregular(route, "wtree", True) + _position_rows(route)
    return rows


ROWS = _rows()
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)


def row(rid):
    return ROWS[ROW_IDS.index(rid)]


def ulp_copies(d, copies=4):
    """`copies` of d with every non-zero of the data moved by one unit in the last place (the pattern of helpers.ulp_solution_spread)"""
    rng = np.random.default_rng(54321)
    for _ in range(copies):
        d2 = dict(d)
        for k in ("A", "B", "b", "Qd", "Rd", "q", "r"):
            a = np.array(d2[k], dtype=np.float64, copy=True)
            a *= 1.0 + (rng.integers(0, 2, a.shape) * 2 - 1) * 2.0 ** -52
            d2[k] = a
        yield d2


def float64_spread(d, lam0, opts):
    base = R.block_newton_step(d, lam0, **opts, dtype=np.float64)["dlam"]
    return max(rel_err(R.block_newton_step(d2, lam0, **opts, dtype=np.float64)["dlam"], base) for d2 in ulp_copies(d))


class LsOpts:
    lineSearchGamma, lineSearchBeta, lineSearchMaxIter = 0.1, 0.6, 50       # the defaults of the solver


BETA = LsOpts.lineSearchBeta


@functools.lru_cache(maxsize=None)
def _case(key):
    r = next(r for r in ROWS if r.key == key)
    rid = r.id
    base = base_problem(r.problem)
    d = pinned(base, r.pins, r.tweak)
    n = int(np.asarray(d["nx"])[1:].sum())
    why = []
    for s in range(TRIES):
        lam0 = N.seeded_duals(n, s)
        ref = R.block_newton_step(d, lam0, **r.opts, check=False)
        ok = dict(xcheck=ref["xcheck"] <= R.XCHECK_TOL, margin=ref["margin"] > GAP, guard=ref["guard"] >= GUARD_MIN, flagged=sorted(ref["flagged"]) == r.flagged,
                  cond=ref["cond"] <= COND_MAX or r.opts is DEFAULTS)
        free = None
        if r.lift:
            # the same problem with the pins lifted, for the second solve on the same mirror: no block flagged
            free = R.block_newton_step(base, lam0, **r.opts, check=False)
            ok.update(free=free["xcheck"] <= R.XCHECK_TOL and free["margin"] > GAP and free["guard"] >= GUARD_MIN and free["cond"] <= COND_MAX and not free["flagged"])
        if not all(ok.values()):
            why.append((s, [k for k, v in ok.items() if not v], sorted(ref["flagged"]), f"{ref['guard']:.2e}", f"{ref['cond']:.2e}"))
            continue
        trials, slack = R.armijo(d, lam0, ref, LsOpts)
        return dict(d=d, base=base, lam0=lam0, seed=s, ref=ref, free=free, trials=trials, slack=slack)
    raise AssertionError(f"row {rid}: none of the {TRIES} seeds meets the row's conditions: {why[:4]}")


def case(rid):
    """dict(d, base, lam0, seed, ref, free, trials, slack): the pinned problem, the problem without pins, the row's lambda0, the
    reference step there (reg_ref.block_newton_step), the reference step of `base` (flag_mid_level rows), the reference's line
    search; rows of several routes on one problem, pins and options share it"""
    return _case(row(rid).key)

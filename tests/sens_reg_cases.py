"""Rows of the regularisation tests of the MPC derivative kernels (test_sens_reg_reference.py on the CPU, test_gpu_mpc_sens_reg.py on the
device): the points at which sens_factor_body (tdunes_sens.hpp) shifts a block's diagonal or leaves a zero column, and what the
substitutions behind it (sens_forward_body, the root's back substitution, k_adj_backward, k_adj_forward, k_adj_grad) make of that.

A row is a dict: id, group, case (a case of adj_cases: the keys of sens_cases plus w), opts (regType, regTol, regValue of the derivative
call; the step before it is solved with the case's own options), flagged (the blocks -- parent ids, in the order they are factorised,
last parent first -- whose diagonal the reference must shift), n_reg (what the call must report), zero (pinned rows: the dual entries
whose pivot is exactly 0.0 on the first pass).

threshold   existing cases, regType 2 with regValue 2^-6 and a regTol between the first-pass pivots of the reference at the oracle's point
            (`one`: the widest gap between consecutive sorted pivots that separates the block with the smallest pivot from every other
            block; `all`: twice the largest pivot), written out in THRESHOLD; two trees also with regType 1.  The dual Hessian depends on the
            active set alone, so the device's own point gives the same pivots up to rounding, and guard >= 1.01 keeps every pivot a hundred
            times further from regTol than any rounding moves it.
pinned      a state that cannot move: state s of node k gets zero rows in A_k and B_k (and in A0_k under an eliminated root), b = xmin =
            xmax = 0.25.  Its row and column of the dual Hessian are exactly zero at every point, its first-pass pivot is exactly 0.0.
            Options: the default on-the-fly shift of 1e-6, a shift of 2^-6, regType 0 (the zero column; n_reg 0), and on two trees
            regTol = 0.0, where only `<=` in the trigger sees the pivot.
batches     mixed_reg: a regular tree and three pinned ones under the default options (n_reg 0, 1, 2, 1); twice: one pinned tree from two x0.

Importing this module must not load the native library (see adj_cases.py): the case modules are imported where a row is built."""
from __future__ import annotations

import functools

import numpy as np

REG_VALUE = 2.0 ** -6
PIN = 0.25
DEFAULT = dict(regType=2, regTol=1e-6, regValue=1e-6)

# tree -> (regTol of `one`, the block it flags, regTol of `all`), four digits of the value chosen from the reference's first-pass pivots;
# test_sens_reg_reference.py recomputes the pivots and asserts the flagged blocks and the guard (printed with -s: 1.02 to 1.25 for `one`, 2 for `all`)
THRESHOLD = {
    "elim-three_children":   (0.415, 0, 2.166),
    "states-generic":        (0.5071, 0, 2.268),
    "elim-dense_kind1_root": (0.5125, 0, 2.271),
    "elim-persist_c1":       (0.09764, 0, 2.484),
    "states-tiered_ub":      (0.07759, 0, 0.7967),
    "node_d-d65":            (0.3444, 1, 2.55),
    "root_d-states_d65":     (0.4674, 0, 2.93),
    "nx0_elim-65":           (0.4228, 0, 2.084),
}
ALWAYS = ("states-generic", "nx0_elim-65")          # the trees that also run with regType 1

# id -> (tree, ((node, state), ...)); state -1: the node's last
PINNED = {
    "states-generic-child":      ("states-generic", ((1, 0),)),
    "states-generic-deep":       ("states-generic", ((5, 0),)),
    "states-generic-both":       ("states-generic", ((1, 0), (5, 0))),
    "node_d-d65-col64":          ("node_d-d65", ((3, -1),)),          # column 64 of the 65-row block of node 1
    "elim-three_children-child": ("elim-three_children", ((1, 0),)),
    "elim-three_children-deep":  ("elim-three_children", ((4, 0),)),
    "elim-three_children-both":  ("elim-three_children", ((1, 0), (4, 0))),
    "root_d-elim_d65-col64":     ("root_d-elim_d65", ((8, -1),)),     # column 64 of the 65-row root block: the G' rows behind it
}
PINNED_OPTS = {
    "default": dict(DEFAULT),
    "shift6": dict(regType=2, regTol=1e-6, regValue=REG_VALUE),
    "zerocol": dict(regType=0, regTol=1e-6, regValue=1e-6),
}
TOL0 = dict(regType=2, regTol=0.0, regValue=REG_VALUE)
TOL0_TREES = ("node_d-d65-col64", "root_d-elim_d65-col64")

THRESHOLD_IDS = [f"thr-{t}-{side}" for t in THRESHOLD for side in ("one", "all")] + [f"thr-{t}-always" for t in ALWAYS]
PINNED_IDS = [f"pin-{p}-{o}" for p in PINNED for o in PINNED_OPTS] + [f"pin-{p}-tol0" for p in TOL0_TREES]
ROW_IDS = THRESHOLD_IDS + PINNED_IDS
ZEROCOL_IDS = [r for r in PINNED_IDS if r.endswith("-zerocol")]
NW3_ID = "pin-states-generic-both-default"
PREDICT_IDS = ("thr-elim-three_children-all", "pin-elim-three_children-both-shift6")

# batch -> ((row id, multiple of the case's dx * 2^10 added to its x0), ...); every member runs with the default options
BATCHES = {
    "mixed_reg": (("regular", 0), ("pin-elim-three_children-child-default", 0), ("pin-states-generic-both-default", 0), ("pin-node_d-d65-col64-default", 0)),
    "twice": (("pin-states-generic-both-default", 0), ("pin-states-generic-both-default", 1)),
}
BATCH_IDS = tuple(BATCHES)
REGULAR = "elim-three_children"


def _offsets(d):
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    dad = np.zeros(len(nk), dtype=int)
    c = 1
    for k in range(len(nk)):
        dad[c:c + nk[k]] = k
        c += nk[k]
    xo = np.concatenate([[0], np.cumsum(nx)])
    ao = np.concatenate([[0, 0], np.cumsum([nx[k] * nx[dad[k]] for k in range(1, len(nk))])])
    bo = np.concatenate([[0, 0], np.cumsum([nx[k] * nu[dad[k]] for k in range(1, len(nk))])])
    return nk, nx, nu, dad, xo, ao, bo


def pin_state(d, root, k, s):
    """state s of node k cannot move: zero rows in A_k, B_k (and A0_k), b = xmin = xmax = PIN; d and root are changed in place"""
    nk, nx, nu, dad, xo, ao, bo = _offsets(d)
    p = dad[k]
    d["A"][ao[k] + s:ao[k] + nx[k] * nx[p]:nx[k]] = 0.0
    d["B"][bo[k] + s:bo[k] + nx[k] * nu[p]:nx[k]] = 0.0
    d["b"][xo[k] - nx[0] + s] = PIN
    d["xmin"][xo[k] + s] = d["xmax"][xo[k] + s] = PIN
    if root is not None and p == 0:
        root["A0"][k - 1][s, :] = 0.0
        root["b0"][xo[k] + s] = PIN


def _pinned_case(pid):
    import adj_cases as AC
    import mpc_cases as MC
    import mpc_root_cases as MR
    import sens_cases as SN
    tree, pins = PINNED[pid]
    src = AC.case(tree)
    sb = src["base"]
    d = {k: np.array(v, copy=True) for k, v in sb["d"].items()}
    root = None
    if src["form"] == "eliminated":
        root = dict(sb["root"], A0=[np.array(M, copy=True) for M in sb["root"]["A0"]], b0=np.array(sb["root"]["b0"], copy=True))
    nx = np.asarray(d["nx"], dtype=int)
    where = []
    for k, s in pins:
        s = int(nx[k]) - 1 if s < 0 else s
        pin_state(d, root, k, s)
        where.append((k, s))
    cid = "pin-" + pid
    if src["form"] == "states":
        base = MR._case(cid, d, sb["kinds"], sb["env"], sb["opts"], sb["path"])
        c = dict(id=cid, form="states", base=base, d=base["d"], kinds=None, param=dict(form="states"), x0=base["x0"], nx0=base["nx0"])
    else:
        base = dict(sb, id=cid, d=d, root=root)
        c = dict(id=cid, form="eliminated", base=base, d=MC.folded(base, MC.fold(root, src["x0"])), kinds=sb["kinds"],
                 param=dict(form="eliminated", A0=root["A0"], S0=root["S0"]), x0=src["x0"], nx0=src["nx0"])
    seed = SN._seed(cid)
    c.update(dx=SN._dx(c["nx0"], seed), w=AC._w(c, 1, seed), w3=AC._w(c, 3, seed + 1), pins=tuple(where))
    return c


@functools.lru_cache(maxsize=None)
def tree(name):
    """the case behind a row: an adj_cases case (threshold rows), or "pin-" + a key of PINNED"""
    import adj_cases as AC
    return _pinned_case(name[4:]) if name.startswith("pin-") else AC.case(name)


def parents(d):
    """the blocks in factorisation order: last parent first"""
    return [p for p in range(len(d["nk"]) - 1, -1, -1) if d["nk"][p] > 0]


def block_rows(d, p):
    """the dual entries of block p: the states of the children of p"""
    nk, nx, nu, dad, xo, ao, bo = _offsets(d)
    kids = np.flatnonzero(dad == p)
    kids = kids[kids > 0]
    return np.arange(xo[kids[0]], xo[kids[-1] + 1]) - nx[0]


def block_of(d, row):
    """(block, index within it) of a dual entry"""
    for p in parents(d):
        rows = block_rows(d, p)
        if rows[0] <= row <= rows[-1]:
            return p, int(row - rows[0])
    raise KeyError(row)


def pinned_entries(c):
    """(the dual entries of the pinned states, the blocks that hold them in factorisation order)"""
    nk, nx, nu, dad, xo, ao, bo = _offsets(c["d"])
    rows = sorted(int(xo[k] - nx[0] + s) for k, s in c["pins"])
    return rows, sorted({int(dad[k]) for k, _ in c["pins"]}, reverse=True)


@functools.lru_cache(maxsize=None)
def row(rid):
    if rid.startswith("thr-"):
        name, side = rid[4:].rsplit("-", 1)
        c = tree(name)
        one, block, every = THRESHOLD[name]
        if side == "always":
            opts, flagged = dict(regType=1, regTol=1e-6, regValue=REG_VALUE), parents(c["d"])
            n_reg = 0          # regType 1 shifts every block and counts none
        else:
            opts = dict(regType=2, regTol=one if side == "one" else every, regValue=REG_VALUE)
            flagged = [block] if side == "one" else parents(c["d"])
            n_reg = len(flagged)
        return dict(id=rid, group="threshold", case=c, opts=opts, flagged=flagged, n_reg=n_reg, zero=[])
    name, o = rid.rsplit("-", 1)
    c = tree(name)
    opts = dict(TOL0) if o == "tol0" else dict(PINNED_OPTS[o])
    zero, blocks = pinned_entries(c)
    flagged = [] if o == "zerocol" else blocks
    return dict(id=rid, group="pinned", case=c, opts=opts, flagged=flagged, n_reg=len(flagged), zero=zero)


def members(bid):
    """(case, x0, n_reg under the default options) of every member of a batch"""
    out = []
    for rid, mult in BATCHES[bid]:
        if rid == "regular":
            c, n_reg = tree(REGULAR), 0
        else:
            r = row(rid)
            c, n_reg = r["case"], r["n_reg"]
        out.append((c, c["x0"] + c["dx"] * 2.0 ** 10 * mult, n_reg))          # multiples of 2^-12: exactly representable
    return out


# Measured by test_sens_reg_reference.py (it prints them with -s and asserts that they still hold): per row the spread max |(b) - (c)| of
# K, dx, du, dlam between sens_ref.dual_form and sens_ref.dense_shifted, and of gq, gr, gb, gx0 between adj_ref.dual_form and
# adj_ref.dense_shifted, at the oracle's point with the row's options.  The device tests allow 10 times these, with a floor of 1e-12.
SPREAD = {
    #                                              K        dx       du       dlam     gq       gr       gb       gx0
    "thr-elim-three_children-one":                   (2.8e-16, 3.9e-16, 2.8e-16, 2.7e-15, 1.9e-16, 2.2e-16, 1.2e-15, 8.9e-16),
    "thr-elim-three_children-all":                   (5.8e-16, 5.0e-16, 5.8e-16, 4.4e-15, 1.4e-16, 2.8e-16, 1.2e-15, 5.6e-16),
    "thr-states-generic-one":                        (3.3e-16, 4.8e-16, 3.3e-16, 2.2e-15, 1.6e-16, 1.6e-16, 1.1e-15, 3.3e-16),
    "thr-states-generic-all":                        (4.4e-16, 4.7e-16, 4.4e-16, 3.1e-15, 2.2e-16, 9.5e-16, 1.1e-15, 3.3e-16),
    "thr-elim-dense_kind1_root-one":                 (3.3e-16, 2.8e-16, 3.3e-16, 2.0e-15, 8.3e-17, 1.1e-16, 2.2e-16, 2.2e-16),
    "thr-elim-dense_kind1_root-all":                 (4.4e-16, 1.7e-16, 4.4e-16, 1.3e-15, 5.6e-17, 1.7e-16, 3.9e-16, 2.2e-16),
    "thr-elim-persist_c1-one":                       (0.0e+00, 9.1e-15, 7.9e-15, 4.4e-13, 2.6e-15, 2.4e-15, 7.5e-14, 2.6e-14),
    "thr-elim-persist_c1-all":                       (0.0e+00, 1.8e-15, 4.7e-16, 3.0e-14, 6.7e-16, 2.8e-16, 7.7e-15, 4.8e-15),
    "thr-states-tiered_ub-one":                      (1.4e-17, 2.2e-16, 1.4e-16, 4.3e-14, 5.6e-17, 2.8e-17, 2.2e-15, 5.0e-16),
    "thr-states-tiered_ub-all":                      (5.6e-17, 1.7e-16, 6.9e-17, 1.4e-14, 2.8e-17, 2.8e-17, 4.4e-16, 4.4e-16),
    "thr-node_d-d65-one":                            (5.6e-17, 2.5e-16, 1.1e-16, 1.3e-15, 1.0e-15, 8.1e-16, 6.8e-15, 4.4e-16),
    "thr-node_d-d65-all":                            (1.1e-16, 3.9e-16, 1.7e-16, 1.2e-15, 1.0e-15, 2.0e-16, 6.9e-15, 5.0e-16),
    "thr-root_d-states_d65-one":                     (3.9e-16, 6.2e-16, 3.9e-16, 3.6e-15, 4.9e-16, 2.2e-16, 2.8e-15, 1.1e-15),
    "thr-root_d-states_d65-all":                     (3.9e-16, 5.3e-16, 3.9e-16, 3.3e-15, 4.3e-16, 6.2e-16, 2.8e-15, 1.0e-15),
    "thr-nx0_elim-65-one":                           (1.6e-16, 1.1e-16, 1.6e-16, 1.0e-15, 1.1e-16, 8.3e-17, 6.9e-16, 1.6e-16),
    "thr-nx0_elim-65-all":                           (2.9e-16, 2.2e-16, 2.9e-16, 1.6e-15, 5.6e-17, 1.1e-16, 5.6e-16, 2.8e-17),
    "thr-states-generic-always":                     (4.4e-16, 4.7e-16, 4.4e-16, 3.1e-15, 2.2e-16, 9.5e-16, 1.1e-15, 3.3e-16),
    "thr-nx0_elim-65-always":                        (2.9e-16, 2.2e-16, 2.9e-16, 1.6e-15, 5.6e-17, 1.1e-16, 5.6e-16, 2.8e-17),
    "pin-states-generic-child-default":              (6.7e-16, 5.8e-16, 6.7e-16, 2.7e-15, 5.2e-16, 9.7e-17, 3.2e-15, 6.7e-16),
    "pin-states-generic-child-shift6":               (4.4e-16, 4.9e-16, 4.4e-16, 3.8e-15, 3.4e-16, 5.9e-16, 2.4e-15, 5.6e-16),
    "pin-states-generic-child-zerocol":              (8.9e-16, 9.1e-16, 8.9e-16, 4.2e-15, 4.3e-16, 6.9e-16, 2.6e-15, 9.4e-16),
    "pin-states-generic-deep-default":               (6.7e-16, 5.2e-16, 6.7e-16, 2.7e-15, 5.8e-16, 5.9e-16, 4.9e-15, 1.3e-15),
    "pin-states-generic-deep-shift6":                (4.4e-16, 5.2e-16, 4.4e-16, 2.8e-15, 6.1e-16, 1.1e-16, 4.0e-15, 6.1e-16),
    "pin-states-generic-deep-zerocol":               (6.7e-16, 5.3e-16, 6.7e-16, 2.5e-15, 6.8e-16, 5.9e-16, 6.0e-15, 1.4e-15),
    "pin-states-generic-both-default":               (1.0e-15, 5.9e-16, 1.0e-15, 2.8e-15, 2.9e-16, 9.7e-17, 2.0e-15, 4.4e-16),
    "pin-states-generic-both-shift6":                (4.4e-16, 5.3e-16, 4.4e-16, 4.7e-15, 7.0e-16, 2.0e-16, 1.7e-15, 4.4e-16),
    "pin-states-generic-both-zerocol":               (4.4e-16, 8.0e-16, 4.4e-16, 3.7e-15, 2.7e-16, 1.4e-16, 1.4e-15, 3.6e-16),
    "pin-node_d-d65-col64-default":                  (5.6e-17, 3.3e-16, 3.1e-16, 2.3e-15, 1.2e-15, 1.4e-15, 9.5e-15, 1.2e-15),
    "pin-node_d-d65-col64-shift6":                   (5.6e-17, 2.5e-16, 2.2e-16, 1.3e-15, 1.4e-15, 1.8e-15, 1.1e-14, 3.3e-16),
    "pin-node_d-d65-col64-zerocol":                  (5.6e-17, 3.1e-16, 3.1e-16, 2.8e-15, 1.5e-15, 2.0e-15, 1.4e-14, 1.4e-15),
    "pin-elim-three_children-child-default":         (4.4e-16, 7.8e-16, 4.4e-16, 3.1e-15, 2.2e-16, 2.2e-16, 8.9e-16, 8.9e-16),
    "pin-elim-three_children-child-shift6":          (4.4e-16, 1.0e-15, 4.4e-16, 5.8e-15, 2.3e-16, 1.4e-16, 1.4e-15, 1.0e-15),
    "pin-elim-three_children-child-zerocol":         (5.8e-16, 1.0e-15, 5.8e-16, 5.8e-15, 2.2e-16, 1.9e-16, 1.4e-15, 7.8e-16),
    "pin-elim-three_children-deep-default":          (3.9e-16, 4.4e-16, 3.9e-16, 2.7e-15, 4.0e-16, 2.2e-16, 1.4e-15, 7.5e-16),
    "pin-elim-three_children-deep-shift6":           (5.0e-16, 5.6e-16, 5.0e-16, 4.9e-15, 2.2e-16, 2.2e-16, 1.3e-15, 6.7e-16),
    "pin-elim-three_children-deep-zerocol":          (4.4e-16, 6.1e-16, 4.4e-16, 3.3e-15, 3.0e-16, 1.9e-16, 2.9e-15, 1.3e-15),
    "pin-elim-three_children-both-default":          (6.7e-16, 5.3e-16, 6.7e-16, 2.9e-15, 1.3e-16, 3.3e-16, 1.1e-15, 6.1e-16),
    "pin-elim-three_children-both-shift6":           (6.7e-16, 7.2e-16, 6.7e-16, 4.7e-15, 1.5e-16, 4.4e-16, 1.3e-15, 4.4e-16),
    "pin-elim-three_children-both-zerocol":          (5.3e-16, 9.4e-16, 5.3e-16, 6.7e-15, 2.0e-16, 4.4e-16, 1.6e-15, 1.2e-15),
    "pin-root_d-elim_d65-col64-default":             (8.5e-15, 3.6e-15, 8.5e-15, 2.2e-14, 8.3e-16, 2.9e-16, 5.3e-15, 5.1e-15),
    "pin-root_d-elim_d65-col64-shift6":              (6.7e-15, 3.5e-15, 6.7e-15, 2.2e-14, 8.5e-16, 1.2e-15, 6.3e-15, 5.7e-15),
    "pin-root_d-elim_d65-col64-zerocol":             (6.8e-15, 3.9e-15, 6.8e-15, 2.1e-14, 7.8e-16, 2.9e-16, 6.9e-15, 7.5e-15),
    "pin-node_d-d65-col64-tol0":                     (5.6e-17, 2.5e-16, 2.2e-16, 1.3e-15, 1.4e-15, 1.8e-15, 1.1e-14, 3.3e-16),
    "pin-root_d-elim_d65-col64-tol0":                (6.7e-15, 3.5e-15, 6.7e-15, 2.2e-14, 8.5e-16, 1.2e-15, 6.3e-15, 5.7e-15),
}
# the regType 0 pinned rows: max |(b) - (a)| of K, dx, du against sens_ref.dense_kkt, the lstsq route, which knows of no zero column
SPREAD_KKT = {
    #                                              K        dx       du
    "pin-states-generic-child-zerocol":              (9.2e-16, 3.6e-15, 1.2e-15),   # lstsq residual 2.5e-14
    "pin-states-generic-deep-zerocol":               (1.6e-15, 4.1e-15, 1.6e-15),   # lstsq residual 1.6e-14
    "pin-states-generic-both-zerocol":               (2.7e-15, 3.7e-15, 2.7e-15),   # lstsq residual 1.9e-14
    "pin-node_d-d65-col64-zerocol":                  (2.6e-15, 3.0e-15, 2.6e-15),   # lstsq residual 1.3e-14
    "pin-elim-three_children-child-zerocol":         (1.1e-15, 1.6e-15, 2.1e-15),   # lstsq residual 2.3e-15
    "pin-elim-three_children-deep-zerocol":          (7.2e-16, 1.5e-15, 1.1e-15),   # lstsq residual 4.3e-15
    "pin-elim-three_children-both-zerocol":          (1.0e-15, 1.8e-15, 1.5e-15),   # lstsq residual 5.3e-15
    "pin-root_d-elim_d65-col64-zerocol":             (4.1e-15, 5.9e-15, 4.1e-15),   # lstsq residual 1.1e-14
}
FLOOR = 1e-12
WHAT = ("K", "dx", "du", "dlam", "gq", "gr", "gb", "gx0")


def tol(rid, what):
    """10 times the CPU spread of the quantity, with a floor of 1e-12 (the device's order of sums is a third one)"""
    return max(10.0 * SPREAD[rid][WHAT.index(what)], FLOOR)


def tol_kkt(rid, what):
    return max(10.0 * SPREAD_KKT[rid][WHAT.index(what)], FLOOR)

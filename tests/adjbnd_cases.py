"""Cases of the bound-gradient and reference-gradient tests (test_adjbnd_reference.py on the CPU, test_gpu_mpc_adjoint_bounds.py and
test_gpu_mpc_adjoint_reference.py on the device).

Bounds: trees of adjmat_cases.tree (BOUND_TREES): both root forms on the single-workgroup and the generic route, the kind-1 tree (every
entry 0.0), `mixed` (kind-0 leaves under kind-1 parents, a state of each leaf on a bound), the two smallest trees, the embedded x0-eliminated C1 (phantom root states) and
chain66 (groups of 64 and 65 members), and states-xbound, where a state of a non-root node sits on its bound.
Reference: tracking mirrors (TRACK_IDS), general data:
  single_wg       tracking_cases' 5-node tree of kind 0 whose root keeps its states
  c1_eliminated   tracking_cases' x0-eliminated C1: kind 0, no S0, phantom root states
  kind1_S0        4 nodes of kind 1, nx = 3 below an eliminated root whose S0 enters r[0]
  fan65, fan64    a root with states and 65 (64) leaves, nx = 2, nu = 1: a stage of two chunks (of one)
Each with w = (wx, wu) (w3: three columns) and windows(c) = (one stage per row, the last two stages clamped into row T - 1).
Importing this module must not load the native library (see adj_cases)."""
from __future__ import annotations

import functools

import numpy as np

BOUND_TREES = ("elim-single_wg", "states-single_wg", "states-generic", "elim-dense_kind1_root", "mixed", "Nh1-one_leaf", "smallest-nx0_1_nu0_1",
               "elim-persist_c1", "chain66", "states-xbound")
TRACK_IDS = ("single_wg", "c1_eliminated", "kind1_S0", "fan65", "fan64")
FD_H = 2.0 ** -16


XBOUND = 0.05          # states-xbound: mpc_limit_cases' ONE_CHILD tree, root with states, the first state of node 1 within +- XBOUND: it sits on that bound


MIXED_XMIN, MIXED_XMAX = -0.5, 0.125          # mixed: free of bounds these two states solve to -0.746 and 0.253


@functools.lru_cache(maxsize=None)
def bound_case(tree):
    import adjmat_cases as XC
    if tree == "states-xbound":
        import adj_cases as AC
        import mpc_limit_cases as ML
        c = dict(ML.states(tree, ML.ONE_CHILD, xbound=XBOUND, xfirst=True))
        c["w"] = AC._w(c, 1, 77)
        return c
    if tree == "mixed":
        # adjmat_cases' mixed tree with a state of either kind-0 leaf held on a bound (its own leaves' bounds are never active): the only tree with
        # kind-0 nodes under kind-1 parents.  The oracle's solvers do not take it: adjbnd_ref.solve_active_set gives its point on the CPU
        c = dict(XC.tree(tree))

        def tight(d):
            d = {k: np.array(v, copy=True) for k, v in d.items()}
            first = int(np.sum(d["nx"][:2])), int(np.sum(d["nx"][:3]))          # the first state of node 2 and of node 3
            d["xmin"][first[0]], d["xmax"][first[1]] = MIXED_XMIN, MIXED_XMAX
            return d
        c["d"], c["base"] = tight(c["d"]), dict(c["base"], d=tight(c["base"]["d"]))
        return c
    return XC.tree(tree)


@functools.lru_cache(maxsize=None)
def track_case(cid, T=None):
    import adj_cases as AC
    import helpers as H
    import mpc_cases as M
    import solve_sequence_cases as SC
    import tracking_cases as TC
    if cid in ("single_wg", "c1_eliminated"):
        c = dict(TC.case(cid, exact=False))
    elif cid == "kind1_S0":
        d = H.dense_shaped_qp([2, 1, 0, 0], [0, 3, 3, 3], 2, 41)
        c = TC._elim(cid, d, 3, 41, False, kinds=np.ones(4, dtype=np.int32))          # (default options: the regularisation rule of the reference)
    else:
        n = int(cid[3:])
        c = TC._states(cid, H.shaped_qp([n] + [0] * n, 2, 1, 40 + n, ubound=1.0).as_dict(), 40 + n, False)
    import adjbnd_ref as BR
    deep = int(BR.stages(c["d"]["nk"]).max())
    if T is None and deep + 2 > c["T"]:
        T = deep + 3          # (C1 is 10 stages deep: a trajectory long enough for a window with one stage per row)
    if T is not None:
        c = TC._reference(dict(c), c["seed"], False, T=T)
    c["param"] = dict(form="states") if c["form"] == "states" else dict(form="eliminated", A0=c["root"]["A0"], S0=c["root"]["S0"])
    c["x0"] = c["x0s"][0]
    seed = sum(ord(ch) for ch in cid)
    c["w"], c["w3"] = AC._w(c, 1, seed), AC._w(c, 3, seed + 1)
    return c


def windows(c):
    """(t0 with one stage per row, t0 with the last two stages in row T - 1)"""
    import adjbnd_ref as BR
    deep = int(BR.stages(c["d"]["nk"]).max())
    assert deep <= c["T"] - 1
    return max(c["T"] - 1 - deep - 1, 0), c["T"] - deep


def folded(c, t0):
    """the flat problem the device holds after the step: x0 folded (eliminated root) or imposed (root with states), window t0 folded into q, r"""
    import mpc_cases as M
    import mpc_root_cases as R
    import tracking_cases as TC
    d = M.folded(c, M.fold(c["root"], c["x0"])) if c["form"] == "elim" else R.with_x0(c, c["x0"])
    d["q"], d["r"] = TC.fold(c, t0, c["x0"] if c["form"] == "elim" else None)
    return d


# Measured by test_adjbnd_reference.py (it prints them with -s and asserts that they still hold): the spread max |(a) - (b)| of the bound
# gradients (lower and upper together), of their sums over the `shared` groups, and per tracking case over its windows of gxref and guref,
# between the two numpy evaluations of adjbnd_ref at the oracle's point.  The device tests allow 10 times these, with a floor of 1e-12.
SPREAD = {
    #                          bounds   grouped
    "elim-single_wg":         (2.0e-15, 2.0e-15),
    "states-single_wg":       (2.9e-14, 2.9e-14),
    "states-generic":         (3.0e-14, 3.0e-14),
    "elim-dense_kind1_root":  (0.0e+00, 0.0e+00),
    "mixed":                  (8.3e-15, 8.3e-15),
    "Nh1-one_leaf":           (1.4e-16, 1.4e-16),
    "smallest-nx0_1_nu0_1":   (2.0e-15, 2.0e-15),
    "elim-persist_c1":        (1.2e-13, 1.2e-13),
    "chain66":                (6.3e-14, 1.2e-13),
    "states-xbound":          (5.8e-15, 1.1e-14),
    #                          gxref    guref
    "single_wg":              (5.7e-15, 1.0e-15),
    "c1_eliminated":          (1.1e-11, 6.3e-13),
    "kind1_S0":               (1.1e-14, 2.2e-15),
    "fan65":                  (4.4e-14, 1.4e-15),
    "fan64":                  (2.4e-14, 1.6e-15),
}
FLOOR = 1e-12


def tol(cid, which):
    """10 times the CPU spread of the quantity (which: 0 or 1, the column of SPREAD), with a floor of 1e-12 (the device's order of sums is a third one)"""
    return max(10.0 * SPREAD[cid][which], FLOOR)

"""Cases of the matrix-gradient tests (test_adjmat_reference.py on the CPU, test_gpu_mpc_adjoint_matrices.py on the device).

A case id is "<tree>|<maps>": the tree is an id of adj_cases (SENS_IDS, the Nh == 1 trees and nx0 = nu[0] = 1 of its limit shapes) or one of
the trees made here; the maps are "node" (every node its own group), "shared" (one group for all nodes of equal sizes and kind) or a name
of MADE; a third part "w3" takes the three-column loss gradient.  case(cid) -> dict(c (the adj_cases dict), maps (the name; maps() builds
hgroup, cgroup from it, None: NULL), w (the loss gradient)).
  chain66           a chain of 66 nodes, nx = 2, nu = 1, root with states: "c64" puts nodes 1 .. 64 into one c-group (one chunk, node 65 left
                    out with -1), "c65" nodes 1 .. 65 (two chunks); both with the h-group of the 65 inner nodes (two chunks) and the leaf left out
  wide_edge         a chain with nx = 8 everywhere, nu = 3 / nu = 0: a c-block [gA | gB | gb] of 8 x 11 + 8 = 96 > 64 entries; "one" is a group of one node
  edge64            nx = 4, 8, 8 along a chain, nu = 3: node 1's c-block [gA | gB | gb] has exactly 8 x (4 + 3) + 8 = 64 entries
  nz1               nx = 1 on the nodes, nu = 0 below the root: h-groups with nz = 1
  mixed             the kind-1 tree of sens_cases with its leaves turned to kind 0 and their Q made diagonal: one kind-0 and one kind-1 h-group.
                    The leaves have no inputs and their state bounds are never active, so the oracle's dense solve of that problem is the mixed tree's
Importing this module must not load the native library (see adj_cases)."""
from __future__ import annotations

import functools

import numpy as np

TREES = ("elim-single_wg", "elim-persist_c1", "elim-three_launch", "elim-generic", "elim-one_child", "elim-three_children", "elim-dense_kind1_root",
         "states-persist_c1", "states-mpersist", "states-single_wg", "states-generic", "states-tiered_ub", "states-one_child", "states-three_children")
SMALL = ("Nh1-one_leaf", "Nh1-three_leaves", "smallest-nx0_1_nu0_1")
MADE = {"chain66": ("c64", "c65"), "wide_edge": ("shared", "one"), "edge64": ("shared",), "nz1": ("node", "shared"), "mixed": ("node", "shared")}
NW3 = ("elim-three_children|shared|w3", "states-generic|shared|w3")
CASE_IDS = [f"{t}|{m}" for t in TREES for m in ("node", "shared")] + [f"{t}|shared" for t in SMALL] + list(NW3) + [f"{t}|{m}" for t, ms in MADE.items() for m in ms]
FD_H = 2.0 ** -16


def _made(tree):
    import adj_cases as AC
    import helpers as H
    import mpc_root_cases as MR
    shapes = {"chain66": ([1] * 65 + [0], 2, 1, 66), "wide_edge": ([1, 1, 0], 8, 3, 67), "edge64": ([1, 1, 0], [4, 8, 8], 3, 68), "nz1": ([2, 0, 0], 1, 1, 69)}
    nk, nx, nu, seed = shapes[tree]
    base = MR._case(tree, H.shaped_qp(nk, nx, nu, seed, ubound=0.05 if tree == "chain66" else 0.3).as_dict())
    c = dict(id="states-" + tree, form="states", base=base, d=base["d"], kinds=None, param=dict(form="states"), x0=base["x0"], nx0=base["nx0"])
    c["w"] = AC._w(c, 1, seed)
    return c


@functools.lru_cache(maxsize=None)
def tree(name):
    import adj_cases as AC
    if name == "mixed":
        c = dict(AC.case("elim-dense_kind1_root"))
        leaf = np.asarray(c["d"]["nk"]) == 0
        kinds = np.array(c["kinds"], copy=True)
        kinds[leaf] = 0

        def diagonal_leaves(d):
            """the leaves' Q made diagonal (they have no inputs, and bounds on their states that are never active): the oracle's bound-free dense solve of
            this problem is the solve of the mixed tree"""
            d = {k: np.array(v, copy=True) for k, v in d.items()}
            at = 0
            for k, a in enumerate(int(v) for v in d["nx"]):
                if leaf[k]:
                    Q = d["Q"][at:at + a * a].reshape((a, a), order="F")
                    d["Q"][at:at + a * a] = np.diag(np.diag(Q)).ravel(order="F")
                    assert int(d["nu"][k]) == 0
                at += a * a
            return d
        c["kinds"], c["d"] = kinds, diagonal_leaves(c["d"])
        c["base"] = dict(c["base"], kinds=kinds, d=diagonal_leaves(c["base"]["d"]))
        return c
    if name in MADE:
        return _made(name)
    return AC.case(name)


def maps(c, name, pad=0):
    import adjmat_ref as AM
    Nn = len(c["d"]["nk"])
    if name == "node":
        return None, None
    if name == "shared":
        return AM.shared(c["d"], c["kinds"], pad)
    hg, cg = np.full(Nn, -1), np.full(Nn, -1)
    if name in ("c64", "c65"):
        hg[:65] = 0
        cg[1:65 if name == "c64" else 66] = 0
    elif name == "one":
        hg[1], cg[2] = 0, 0
    return hg, cg


@functools.lru_cache(maxsize=None)
def case(cid):
    parts = cid.split("|")
    c = tree(parts[0])
    return dict(c=c, maps=parts[1], w=c["w3"] if len(parts) > 2 else c["w"])


def filled(c, hg, cg):
    """the maps with NULL filled in as the device does"""
    import adjmat_ref as AM
    Nn = len(c["d"]["nk"])
    return (AM.per_node(Nn)[0] if hg is None else hg), (AM.per_node(Nn)[1] if cg is None else cg)


# Measured by test_adjmat_reference.py (it prints them with -s and asserts that they still hold): per tree the spread max |(a) - (b)| over
# the maps of the tree, of gH, gh, gA, gB, gb and of gA0, gS0 together, the discrepancy |w' (z(theta + dtheta) - z(theta - dtheta)) / 2 - <G, dtheta>|
# of the central difference through the oracle at stationarityTolerance 1e-12, and the step it was taken with (halved until the active set
# stays on both sides).  The device tests allow 10 times the spreads, with a floor of 1e-12.
SPREAD = {
    #                             gH       gh       gA       gB       gb       gA0|gS0  fd       step
    "elim-single_wg":            (1.2e-15, 1.3e-15, 2.8e-15, 5.2e-15, 1.2e-14, 1.1e-14, 1.5e-14, 2.0 ** -16),
    "elim-persist_c1":           (1.0e-12, 6.7e-13, 5.8e-11, 1.7e-10, 1.2e-11, 2.9e-12, 1.0e-11, 2.0 ** -16),
    "elim-three_launch":         (9.7e-16, 2.3e-15, 0.0e+00, 1.3e-14, 1.2e-14, 1.1e-14, 3.5e-14, 2.0 ** -16),
    "elim-generic":              (2.0e-15, 1.9e-15, 5.8e-15, 5.7e-15, 7.7e-15, 6.9e-15, 6.6e-14, 2.0 ** -16),
    "elim-one_child":            (2.4e-16, 1.5e-15, 2.3e-16, 1.0e-15, 1.4e-15, 1.0e-15, 4.1e-15, 2.0 ** -16),
    "elim-three_children":       (1.3e-15, 2.1e-15, 2.3e-15, 6.2e-15, 3.7e-15, 3.3e-15, 7.0e-15, 2.0 ** -16),
    "elim-dense_kind1_root":     (6.1e-16, 6.1e-16, 6.5e-16, 4.0e-15, 1.4e-15, 1.0e-15, 3.5e-14, 2.0 ** -16),
    "states-persist_c1":         (2.5e-12, 4.4e-13, 2.8e-10, 8.2e-10, 4.3e-11, 0.0e+00, 4.3e-10, 2.0 ** -16),
    "states-mpersist":           (6.6e-12, 9.7e-13, 1.6e-10, 5.1e-10, 6.4e-11, 0.0e+00, 1.0e-10, 2.0 ** -16),
    "states-single_wg":          (3.4e-15, 3.6e-15, 1.0e-14, 9.1e-15, 9.8e-15, 0.0e+00, 4.8e-15, 2.0 ** -16),
    "states-generic":            (5.8e-16, 2.3e-15, 1.5e-14, 4.1e-15, 1.3e-14, 0.0e+00, 5.0e-15, 2.0 ** -16),
    "states-tiered_ub":          (5.5e-13, 1.6e-12, 3.1e-10, 3.2e-10, 1.6e-10, 0.0e+00, 1.2e-12, 2.0 ** -16),
    "states-one_child":          (2.8e-16, 1.3e-15, 3.4e-15, 2.3e-15, 1.5e-15, 0.0e+00, 4.9e-16, 2.0 ** -16),
    "states-three_children":     (2.0e-15, 1.8e-15, 3.6e-15, 2.2e-15, 3.8e-15, 0.0e+00, 5.5e-15, 2.0 ** -16),
    "Nh1-one_leaf":              (5.5e-17, 3.8e-16, 0.0e+00, 6.9e-16, 3.9e-16, 2.8e-16, 5.7e-16, 2.0 ** -16),
    "Nh1-three_leaves":          (7.1e-16, 1.4e-15, 5.2e-15, 6.7e-15, 5.4e-15, 0.0e+00, 3.1e-15, 2.0 ** -16),
    "smallest-nx0_1_nu0_1":      (7.0e-17, 5.6e-16, 2.8e-16, 3.4e-16, 9.4e-16, 3.9e-16, 1.4e-15, 2.0 ** -16),
    "chain66":                   (1.3e-15, 2.3e-14, 5.4e-14, 2.3e-14, 2.9e-13, 0.0e+00, 2.9e-15, 2.0 ** -16),
    "wide_edge":                 (7.4e-16, 1.9e-15, 4.8e-15, 3.1e-15, 6.7e-15, 0.0e+00, 1.0e-14, 2.0 ** -16),
    "edge64":                    (1.1e-15, 2.9e-15, 6.3e-15, 2.3e-15, 7.8e-15, 0.0e+00, 1.5e-14, 2.0 ** -16),
    "nz1":                       (9.6e-17, 5.7e-16, 4.4e-16, 7.8e-16, 8.9e-16, 0.0e+00, 5.1e-18, 2.0 ** -16),
    "mixed":                     (4.0e-16, 6.4e-16, 8.0e-16, 1.8e-15, 1.3e-15, 1.2e-15, 1.5e-15, 2.0 ** -16),
}
FLOOR = 1e-12
WHAT = ("gH", "gh", "gA", "gB", "gb", "gA0", "gS0")


def tol(cid, what):
    """10 times the CPU spread of the quantity on the case's tree, with a floor of 1e-12 (the device's order of sums is a third one)"""
    return max(10.0 * SPREAD[cid.split("|")[0]][min(WHAT.index(what), 5)], FLOOR)

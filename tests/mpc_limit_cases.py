"""The shapes on both sides of every size limit of the MPC and sensitivity kernels (tdunes_mpc.hpp: mpc_pre_block, mpc_track_node,
k_mpc_post, k_mpc_post_batch; tdunes_adjoint.hpp: setup_sens; tdunes_sens.hpp), shared by the CPU checks (test_mpc_limits_reference.py) and the device
tests (test_gpu_mpc_limits.py).  The limits are the 64 lanes of a wave (the `i = lane; i < n; i += WAVE` loops), the 256 threads and the
16 lanes / 16 members of the post kernels, the `i < 16` gates on the packed constants, and the 160 KiB of LDS setup_sens checks.

A shape is a nested node (nx, nu, [children]) as in limit_shapes.  A sensitivity case is a dict with the keys of sens_cases (id, form,
base, d, kinds, param, x0, nx0, dx), so sens_cases.make, sens_cases.oracle_solve and sens_ref take it as they take their own.  The root of
an eliminated case has made-up originals (mpc_cases.root_terms) of nx0 columns, multiples of 2^-6: its fold is exact in any order.

One row per limit, the smallest shape on each side (ROWS: limit -> the ids of its sides):

  root block d against WAVE          fan of 8 children of nx 8 (d = 64) | the last child nx 9 (d = 65), limit_shapes d64 / d65, both
                                     root forms; nk0 = 8 fold blocks
  non-root block d                   node 1 with leaves of 32 + 32 | 33 + 32
  a kind-0 node's nz                 root (40, 24) | (40, 25), the root keeps its states
  a kind-1 root's nz, with S0        eliminated root of nu[0] = 64 | 65 over (8, 2) -> leaf(4) (dense_pair without the root's states: nz
                                     of an eliminated root is nu[0])
  nu[0]                              64 | 65 and 70, eliminated clipping root
  nx0, eliminated root               64 | 65 on the four-node tree of mpc_cases.one_child
  nx0, root with states              (64, 2, [(4, 2, [leaf(3)])]) | 65 states
  a root child's nx (fold rows)      64 | 65
  Nh == 1                            [1, 0] and a root with three leaf children
  nx0 = 1, nu[0] = 1                 the smallest sizes the API accepts
  setup_sens, tall root block        (((d + nx0) | 1) d + d + 2) * 8 <= 160 KiB: accepted d = 140 with nx0 = 5 (163536 bytes) and
                                     limit_shapes.FACTOR_ACCEPTED (d = 141) with its two-state root kept (162448); refused: the same tree
                                     eliminated with nx0 = 5 (166960)
  setup_sens, nz x nx0 window        (nz nx0 + 2) * 8 <= 160 KiB with the largest nz 40: nx0 = 511 (163536) | 512 (163856)
  k_mpc_post, 256 threads            nu[0] = 256 | 257
  batch post, 16 lanes, 16 members   16 members of nu[0] = 16 | 17 members of two trees, one with nu[0] = 17 and two root children, so
                                     that the members' k_mpc_pre grids differ (nk0 + 1 + the warm spans: 3 and 4 blocks)
  packed constants, i < 16           one side: the persistent route takes the (nx, nu, md) of FAST_TABLE / MSTAGE_TABLE only, whose largest
                                     nx is 8 and largest nx + nu is 12 ((8, 4, 2)): no node of a tree on that route has a 17th entry, the
                                     gates never cut anything off.  The (8, 4, 2) tree is the case.
  nc0 > 64                           unreachable: tqgpu_set_constraints refuses more than 64 rows on a node (the row masks are 64 bits
                                     wide); rows are kind 3, which tqgpu_mpc_sensitivity refuses anyway; no case

The dense kind-1 trees have no bounds (kind 1 ignores them), as sens_cases' own: the conditions on active bounds do not apply to them."""
from __future__ import annotations

import functools

import numpy as np

import helpers as H
import limit_shapes as S
import mpc_cases as MC
import mpc_root_cases as MR
import sens_cases as SN
from treeqp_amd import problems as P

leaf = S.leaf
NX0 = MC.NX0
LDS = 160 * 1024


def fma(a, b, c):
    """a * b + c rounded once, through exact rational arithmetic"""
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _finish(cid, form, base, d, kinds, param, x0, nx0):
    return dict(id=cid, form=form, base=base, d=d, kinds=kinds, param=param, x0=x0, nx0=nx0, dx=SN._dx(nx0, SN._seed(cid)))


def _elim_base(cid, d, nx0, seed, kinds=None, scale=0.5, env=None):
    return dict(id=cid, d=d, kinds=kinds, root=MC.root_terms(d, nx0, seed + 50, kinds, scale), nx0=nx0, env=env or {}, opts={}, single=False, path=None)


def _elim_case(cid, base, seed):
    x0 = MC.exact_x0s(base["nx0"], seed)[0]
    d = MC.folded(base, MC.fold(base["root"], x0))
    param = dict(form="eliminated", A0=base["root"]["A0"], S0=base["root"]["S0"])
    return _finish(cid, "eliminated", base, d, base["kinds"], param, x0, base["nx0"])


def _clipping(shape, seed, ubound, xbound, xfirst=False):
    """helpers.shaped_qp on the tree `shape`; xbound: the states below the root are kept within +- xbound (shaped_qp leaves them free),
    with xfirst the first state of node 1 alone (a tree with one input cannot hold more than one state on a bound)"""
    nk, nx, nu = S.flatten(shape)
    d = H.shaped_qp(nk, nx, nu, seed, ubound=ubound).as_dict()
    if xbound is not None:
        sl = slice(int(nx[0]), int(nx[0]) + 1 if xfirst else None)
        d["xmin"][sl] = -xbound
        d["xmax"][sl] = xbound
    return d


def elim(cid, shape, nx0=NX0, seed=11, ubound=0.3, xbound=None, xfirst=False, scale=0.5):
    """the clipping tree `shape` (its root's states are dropped) with an eliminated root of nx0 made-up columns"""
    d, _ = MC.eliminate(_clipping(shape, seed, ubound, xbound, xfirst))
    return _elim_case(cid, _elim_base(cid, d, nx0, seed, scale=scale), seed)


def states(cid, shape, seed=11, ubound=0.3, xbound=None, xfirst=False):
    """the clipping tree `shape`, its root keeps its states"""
    base = MR._case(cid, _clipping(shape, seed, ubound, xbound, xfirst))
    return _finish(cid, "states", base, base["d"], None, dict(form="states"), base["x0"], base["nx0"])


def elim_dense1(cid, shape, nx0=NX0, seed=31):
    """a tree of kind-1 nodes under an eliminated root (nx[0] == 0) with S0 != 0"""
    nk, nx, nu = S.flatten(shape)
    assert nx[0] == 0
    d = H.dense_shaped_qp(nk, nx, nu, seed)
    kinds = np.ones(len(nk), dtype=np.int32)
    return _elim_case(cid, _elim_base(cid, d, nx0, seed, kinds=kinds, scale=0.25), seed)


def _root_nu(n, kid=(4, 2, [leaf(3)])):
    return (3, n, [kid])


ONE_CHILD = (3, 2, [(3, 2, [leaf(2), leaf(2)])])
# the largest nz is 40, on node 2: as a child of the root its 38 states would make the tall root block [W; G'] the larger window
WINDOW_TREE = (3, 2, [(3, 2, [(38, 2, [leaf(3)])])])
FACTOR_140 = (2, 1, [leaf(47), leaf(47), leaf(46)])
# (nz nx0 + 2) * 8 <= 160 KiB at nz = 40
WINDOW_NX0 = (LDS // 8 - 2) // 40

# id -> (builder, shape, the builder's other arguments -- the seeds and bounds chosen so that test_mpc_limits_reference.py's conditions
# hold --, what the row is about).  "refused": tqgpu_mpc_sensitivity must refuse the shape (no reference is asked for);
# "predict": the case also runs tqgpu_mpc_predict's exact check
_SENS = {
    "root_d-elim_d64":     (elim, S.case("wide_class-d64")[1], {}, {}),
    "root_d-elim_d65":     (elim, S.case("wide_class-d65")[1], {}, dict(duals=True)),
    "root_d-states_d64":   (states, S.case("wide_class-d64")[1], dict(seed=12), {}),
    "root_d-states_d65":   (states, S.case("wide_class-d65")[1], {}, {}),
    "node_d-d64":          (states, (3, 2, [(4, 2, [leaf(32), leaf(32)])]), dict(seed=12), {}),
    "node_d-d65":          (states, (3, 2, [(4, 2, [leaf(33), leaf(32)])]), {}, {}),
    "kind0_nz-nz64":       (states, (40, 24, [(20, 2, [leaf(2)])]), dict(seed=12), {}),
    "kind0_nz-nz65":       (states, (40, 25, [(20, 2, [leaf(2)])]), dict(seed=12), {}),
    "kind1_nz-nz64":       (elim_dense1, (0, 64, [(8, 2, [leaf(4)])]), {}, {}),
    "kind1_nz-nz65":       (elim_dense1, (0, 65, [(8, 2, [leaf(4)])]), {}, {}),
    "nu0-64":              (elim, _root_nu(64), {}, dict(predict=True)),
    "nu0-65":              (elim, _root_nu(65), {}, dict(predict=True)),
    "nu0-70":              (elim, _root_nu(70), {}, dict(predict=True, both_sides=True)),
    "nx0_elim-64":         (elim, ONE_CHILD, dict(nx0=64, scale=0.125, seed=12), {}),
    "nx0_elim-65":         (elim, ONE_CHILD, dict(nx0=65, scale=0.125, seed=12), dict(predict=True)),
    "nx0_states-64":       (states, (64, 2, [(4, 2, [leaf(3)])]), {}, {}),
    "nx0_states-65":       (states, (65, 2, [(4, 2, [leaf(3)])]), dict(seed=12), {}),
    "child_nx-64":         (elim, (3, 2, [(64, 2, [leaf(3)])]), dict(seed=24), {}),
    "child_nx-65":         (elim, (3, 2, [(65, 2, [leaf(3)])]), {}, {}),
    "Nh1-one_leaf":        (elim, (3, 2, [leaf(3)]), {}, {}),
    "Nh1-three_leaves":    (states, (3, 2, [leaf(3), leaf(2), leaf(4)]), dict(seed=14), {}),
    "smallest-nx0_1_nu0_1": (elim, (1, 1, [(2, 1, [leaf(2)])]), dict(nx0=1, seed=20, ubound=0.1), {}),
    "lds_tall-d140_nx0_5": (elim, FACTOR_140, dict(ubound=1.0, xbound=0.6, xfirst=True), {}),
    "lds_tall-d141_two_states": (states, S.FACTOR_ACCEPTED, dict(ubound=1.0, xbound=0.1, xfirst=True), {}),
    "lds_tall-d141_nx0_5": (elim, S.FACTOR_ACCEPTED, dict(ubound=1.0, xbound=0.1, xfirst=True), dict(refused=True)),
    "lds_window-accepted": (elim, WINDOW_TREE, dict(nx0=WINDOW_NX0, scale=1.0 / 32, seed=12), {}),
    "lds_window-refused":  (elim, WINDOW_TREE, dict(nx0=WINDOW_NX0 + 1, scale=1.0 / 32, seed=11), dict(refused=True)),
}
SENS_IDS = list(_SENS)
ACCEPTED_IDS = [c for c in SENS_IDS if not _SENS[c][3].get("refused")]
REFUSED_IDS = [c for c in SENS_IDS if _SENS[c][3].get("refused")]
PREDICT_IDS = [c for c in SENS_IDS if _SENS[c][3].get("predict")]
DUALS_ID = "root_d-elim_d65"
# (refused, its accepted neighbour: the same tree on the other side of the limit)
REFUSAL_PAIRS = [("lds_tall-d141_nx0_5", "lds_tall-d141_two_states"), ("lds_window-refused", "lds_window-accepted")]

ROWS = {
    "root block d": ["root_d-elim_d64", "root_d-elim_d65", "root_d-states_d64", "root_d-states_d65"],
    "non-root block d": ["node_d-d64", "node_d-d65"],
    "kind-0 nz": ["kind0_nz-nz64", "kind0_nz-nz65"],
    "kind-1 nz with S0": ["kind1_nz-nz64", "kind1_nz-nz65"],
    "nu[0]": ["nu0-64", "nu0-65", "nu0-70"],
    "nx0, eliminated": ["nx0_elim-64", "nx0_elim-65"],
    "nx0, states": ["nx0_states-64", "nx0_states-65"],
    "child nx": ["child_nx-64", "child_nx-65"],
    "Nh == 1": ["Nh1-one_leaf", "Nh1-three_leaves"],
    "smallest": ["smallest-nx0_1_nu0_1"],
    "setup_sens tall": ["lds_tall-d140_nx0_5", "lds_tall-d141_two_states", "lds_tall-d141_nx0_5"],
    "setup_sens window": ["lds_window-accepted", "lds_window-refused"],
}


@functools.lru_cache(maxsize=None)
def case(cid):
    build, shape, kw, _ = _SENS[cid]
    return build(cid, shape, **kw)


def flags(cid):
    return _SENS[cid][3]


def lds_bytes(c):
    """(the tall block of k_sens_factor, the window of k_sens_primal) in bytes, by setup_sens' formulas"""
    d, nx0 = c["base"]["d"], c["nx0"]
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    lp = max((int(nx[k] + nu[k]) * nx0 + 2) * 8 for k in range(len(nk)))
    kid, lf = 1, 0
    for k in range(len(nk)):
        if nk[k] == 0:
            continue
        dim = int(nx[kid:kid + nk[k]].sum())
        kid += nk[k]
        R = dim + (int(nx[k]) if k > 0 else nx0)
        lf = max(lf, ((R | 1) * dim + dim + 2) * 8)
    return lf, lp


def parent_levels(nk):
    """the levels of the tree that hold parents (Tree::Nh)"""
    nk = np.asarray(nk)
    lvl, first, n = 0, 0, 1
    while first < len(nk) and np.any(nk[first:first + n] > 0):
        kids = int(nk[first:first + n].sum())
        first, n, lvl = first + n, kids, lvl + 1
    return lvl


# ---- fold rows: exact data (multiples of 2^-6), mpc_cases.fold is the reference ----
def _fold_elim(cid, shape, nx0=NX0, seed=11, scale=0.5):
    nk, nx, nu = S.flatten(shape)
    d, _ = MC.eliminate(H.shaped_qp(nk, nx, nu, seed, ubound=0.3).as_dict())
    return _elim_base(cid, d, nx0, seed, scale=scale)


def _fold_dense1(cid, shape, seed=31):
    nk, nx, nu = S.flatten(shape)
    d = H.dense_shaped_qp(nk, nx, nu, seed)
    return _elim_base(cid, d, NX0, seed, kinds=np.ones(len(nk), dtype=np.int32), scale=0.25)


FOLD_ELIM = {
    "child_nx-64": lambda c: _fold_elim(c, (3, 2, [(64, 2, [leaf(3)])])),
    "child_nx-65": lambda c: _fold_elim(c, (3, 2, [(65, 2, [leaf(3)])])),
    "nk0_8-d64": lambda c: _fold_elim(c, S.case("wide_class-d64")[1]),
    "nk0_8-d65": lambda c: _fold_elim(c, S.case("wide_class-d65")[1]),
    "S0_nu0-64": lambda c: _fold_dense1(c, (0, 64, [(8, 2, [leaf(4)])])),
    "S0_nu0-65": lambda c: _fold_dense1(c, (0, 65, [(8, 2, [leaf(4)])])),
    "nx0-64": lambda c: _fold_elim(c, ONE_CHILD, nx0=64, scale=0.125),
    "nx0-65": lambda c: _fold_elim(c, ONE_CHILD, nx0=65, scale=0.125),
}
FOLD_STATES = {
    "nx0_states-64": (64, 2, [(4, 2, [leaf(3)])]),
    "nx0_states-65": (65, 2, [(4, 2, [leaf(3)])]),
}


@functools.lru_cache(maxsize=None)
def fold_elim_case(cid):
    return FOLD_ELIM[cid](cid)


@functools.lru_cache(maxsize=None)
def fold_states_case(cid):
    nk, nx, nu = S.flatten(FOLD_STATES[cid])
    return MR._case(cid, H.shaped_qp(nk, nx, nu, 11, ubound=0.3).as_dict())


@functools.lru_cache(maxsize=None)
def persist_case():
    """the largest nx and nx + nu the persistent route admits: the uniform tree (8, 4, md = 2); 15 nodes"""
    return MR._case("persist_8_4_2", P.random_uniform_tree_qp(5, nx=8, nu=4, md=2, Nr=2, Nh=3).as_dict(), path=2)


# ---- tracking rows: one nx and one nu on every node, nz = 64 | 65, kind 0 (root with states) and kind 1 (eliminated root with S0) ----
@functools.lru_cache(maxsize=None)
def tracking_case(cid):
    """as tracking_cases._states / _elim with exact data, without their nx + nu <= 64: every term of a chain is a multiple of 2^-12 of
    size at most 4, a chain has at most nu + 2 nx = 105 of them and a base of size 1: every partial sum is a multiple of 2^-12 below
    2^9, exact in any order"""
    import tracking_cases as K
    nu = {"kind0-nz64": 24, "kind0-nz65": 25, "kind1-nz64": 24, "kind1-nz65": 25}[cid]
    if cid.startswith("kind0"):
        seed = 12
        nk, nx, nuv = S.flatten((40, nu, [(40, nu, [leaf(40)])]))
        c = MR._case(cid, K._quantised_problem(H.shaped_qp(nk, nx, nuv, seed, ubound=0.3).as_dict()))
        c.update(form="states", single=False, root=None, seed=seed)
        c["x0s"] = [MC.quantised(np.random.Generator(np.random.PCG64(seed + s)), 40, 1.0) for s in range(3)]
    else:
        seed = 33
        nk, nx, nuv = S.flatten((0, nu, [(40, nu, [leaf(40)])]))
        kinds = np.ones(len(nk), dtype=np.int32)
        c = MC._case(cid, K._quantised_problem(H.dense_shaped_qp(nk, nx, nuv, seed)), 40, seed, kinds=kinds)
        c.update(form="elim", seed=seed)
        c["x0s"] = MC.exact_x0s(40, seed)[:3]
    rng = np.random.Generator(np.random.PCG64(seed + 700))
    c["NXT"], c["NUT"], c["T"] = 40, nu, TRACK_T
    c["xtraj"], c["utraj"] = MC.quantised(rng, (TRACK_T, 40), 1.0), MC.quantised(rng, (TRACK_T, nu), 1.0)
    c["q0"], c["r0"] = MC.quantised(rng, len(c["d"]["q"]), 1.0), MC.quantised(rng, len(c["d"]["r"]), 1.0)
    return c


TRACKING_IDS = ["kind0-nz64", "kind0-nz65", "kind1-nz64", "kind1-nz65"]
TRACK_T = 6
TRACK_WINDOWS = (1, 5)          # stages reach 2: the second window is clamped at T - 1 on every node below the root


# ---- post rows ----
@functools.lru_cache(maxsize=None)
def post_case(nu0):
    return _fold_elim(f"post-nu0_{nu0}", _root_nu(nu0))


@functools.lru_cache(maxsize=None)
def batch_cases():
    """(tree A: nu[0] = 16, one root child; tree B: nu[0] = 17, two root children)"""
    a = _fold_elim("batch-nu0_16", _root_nu(16))
    b = _fold_elim("batch-nu0_17", (3, 17, [(4, 2, [leaf(3)]), (5, 2, [leaf(3)])]), seed=12)
    return a, b


# Measured by test_mpc_limits_reference.py (it prints them with -s and asserts that they still hold): per case the spread max |(a) - (b)|
# of K, dx, du, dlam between the two numpy evaluations of sens_ref at the oracle's point.  The device tests allow 10 times these, floor 1e-12.
SPREAD = {
    #                              K        dx       du       dlam
    "root_d-elim_d64":             (3.6e-15, 3.9e-15, 3.7e-15, 1.9e-14),
    "root_d-elim_d65":             (6.4e-15, 5.6e-15, 6.4e-15, 3.2e-14),
    "root_d-states_d64":           (3.4e-15, 8.6e-15, 4.9e-15, 7.0e-14),
    "root_d-states_d65":           (2.2e-15, 6.0e-15, 4.2e-15, 4.7e-14),
    "node_d-d64":                  (2.8e-15, 3.6e-15, 2.8e-15, 2.4e-14),
    "node_d-d65":                  (2.3e-15, 2.6e-15, 2.3e-15, 1.7e-14),
    "kind0_nz-nz64":               (2.6e-15, 6.2e-15, 2.6e-15, 4.8e-15),
    "kind0_nz-nz65":               (1.7e-15, 2.2e-15, 2.0e-15, 3.5e-15),
    "kind1_nz-nz64":               (1.1e-15, 1.2e-15, 1.1e-15, 9.1e-15),
    "kind1_nz-nz65":               (6.9e-16, 4.4e-16, 6.9e-16, 2.4e-15),
    "nu0-64":                      (2.9e-16, 1.6e-16, 2.9e-16, 3.5e-16),
    "nu0-65":                      (3.2e-16, 1.1e-16, 3.2e-16, 3.0e-16),
    "nu0-70":                      (2.4e-16, 1.3e-16, 2.4e-16, 2.7e-16),
    "nx0_elim-64":                 (3.1e-16, 3.4e-16, 3.1e-16, 2.7e-15),
    "nx0_elim-65":                 (3.7e-16, 3.5e-16, 3.7e-16, 2.3e-15),
    "nx0_states-64":               (1.1e-15, 4.0e-15, 2.7e-15, 1.1e-14),
    "nx0_states-65":               (6.2e-15, 5.0e-15, 6.2e-15, 1.1e-14),
    "child_nx-64":                 (2.2e-15, 4.9e-15, 3.2e-15, 4.0e-14),
    "child_nx-65":                 (4.5e-15, 6.7e-15, 4.5e-15, 3.6e-14),
    "Nh1-one_leaf":                (3.9e-16, 3.3e-16, 3.9e-16, 1.3e-15),
    "Nh1-three_leaves":            (3.4e-15, 1.9e-15, 3.4e-15, 1.1e-14),
    "smallest-nx0_1_nu0_1":        (9.0e-17, 2.6e-16, 9.0e-17, 6.7e-16),
    "lds_tall-d140_nx0_5":         (7.6e-12, 8.1e-12, 7.6e-12, 1.1e-08),
    "lds_tall-d141_two_states":    (2.4e-14, 1.2e-13, 2.4e-14, 2.0e-11),
    "lds_window-accepted":         (2.6e-16, 3.6e-16, 2.6e-16, 2.7e-15),
}
FLOOR = 1e-12


def tol(cid, what):
    return max(10.0 * SPREAD[cid][("K", "dx", "du", "dlam").index(what)], FLOOR)

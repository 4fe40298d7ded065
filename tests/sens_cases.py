"""Cases of the sensitivity tests (test_sens_reference.py on the CPU, test_gpu_mpc_sens.py on the device): the small trees of mpc_cases
(eliminated root) and mpc_root_cases (root with states), one tree with a kind-1 eliminated root and S0 != 0, each with the problem at
its x0, the parameter form of sens_ref and a direction dx for the finite-difference check.

A case is a dict: id, form, base (the mpc_cases / mpc_root_cases case), d (the flat problem at x0), kinds, param, x0, nx0, dx."""
from __future__ import annotations

import functools

import numpy as np

import helpers as H
import mpc_cases as MC
import mpc_root_cases as MR

ELIMINATED = ("single_wg", "persist_c1", "three_launch", "generic", "one_child", "three_children")
# dropped, as trees without a seed that fail a CPU condition: states three_launch and states tiered have no active bound at their x0
# (condition "at least one bound active"); the three-launch route stays through the eliminated case, and route 1 (tiered) through
# tiered_ub: the same tree, linear_chain(2, 4, 4), with the input bound at TIERED_UBOUND instead of the default, where bounds are active
STATES = ("persist_c1", "mpersist", "single_wg", "generic", "tiered_ub", "one_child", "three_children")
TIERED_UBOUND = 0.05
TOL12 = dict(stationarityTolerance=1e-12)
FD_H = 2.0 ** -16           # size of the finite-difference direction: entries are multiples of 2^-22


def _dx(nx0, seed):
    rng = np.random.Generator(np.random.PCG64(seed + 909))
    return FD_H * MC.quantised(rng, nx0, 1.0)


def _seed(cid):
    return sum(ord(ch) for ch in cid)


def _dense_kind1():
    d = H.dense_shaped_qp([2, 1, 0, 0], [0, 3, 2, 2], 2, 31)
    kinds = np.ones(len(d["nk"]), dtype=np.int32)
    return dict(id="dense_kind1_root", d=d, kinds=kinds, root=MC.root_terms(d, MC.NX0, 9, kinds), nx0=MC.NX0, env={}, opts={}, single=False, path=None)


def _tiered_ub():
    """the tiered tree of mpc_root_cases with a tighter input bound, so that some inputs sit on it: the case of route 1"""
    from treeqp_amd import problems as P
    return MR._case("tiered_ub", MR._lti_flat(P.linear_chain(2, 4, 4, ubound=TIERED_UBOUND)), env=MR.TIERED, path=1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for cid in ELIMINATED + ("dense_kind1_root",):
        c = _dense_kind1() if cid == "dense_kind1_root" else MC.case(cid)
        x0 = MC.exact_x0s(c["nx0"], 0)[0]
        d = MC.folded(c, MC.fold(c["root"], x0))
        param = dict(form="eliminated", A0=c["root"]["A0"], S0=c["root"]["S0"])
        out.append(dict(id="elim-" + cid, form="eliminated", base=c, d=d, kinds=c["kinds"], param=param, x0=x0, nx0=c["nx0"], dx=_dx(c["nx0"], _seed("elim-" + cid))))
    for cid in STATES:
        c = _tiered_ub() if cid == "tiered_ub" else MR.case(cid)
        out.append(dict(id="states-" + cid, form="states", base=c, d=c["d"], kinds=None, param=dict(form="states"), x0=c["x0"], nx0=c["nx0"], dx=_dx(c["nx0"], _seed("states-" + cid))))
    return tuple(out)


CASE_IDS = [c["id"] for c in cases()]


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def problem_at(c, x0):
    """the case's flat problem with another x0 folded in"""
    if c["form"] == "states":
        return MR.with_x0(c["base"], x0)
    return MC.folded(c["base"], MC.fold(c["base"]["root"], x0))


def oracle_solve(orc, c, d=None, **opts):
    """the oracle's solve of the case's problem (kind 1: the dense unconstrained variant)"""
    d = c["d"] if d is None else d
    o = H.oracle_opts(orc, {**TOL12, **opts})
    if c["kinds"] is not None:
        s = orc.solve_dense(d, o)
        s["mu_x"], s["mu_u"] = np.zeros(len(s["x"])), np.zeros(len(s["u"]))
        return s
    return orc.solve(d, o, traces=False)


def make(capi, c):
    """a fresh mirror with the root form declared"""
    if c["form"] == "states":
        return MR.make(capi, c["base"], root_states=True)
    return MC.make(capi, c["base"])


# Measured by test_sens_reference.py (it prints them with -s and asserts that they still hold): per case the spread max |(a) - (b)| of K,
# dx, du between the two numpy evaluations at the oracle's point, and the discrepancy max |K dx - (u0(x0 + dx) - u0(x0))| against the
# oracle's solves at stationarityTolerance 1e-12.  The device tests allow 10 times these, with a floor of 1e-12 on the spreads.
SPREAD = {
    #                            K        dx       du       dlam     fd
    "elim-single_wg":          (3.5e-15, 4.0e-15, 4.2e-15, 3.7e-14, 2.3e-17),
    "elim-persist_c1":         (1.2e-14, 6.9e-13, 7.3e-13, 6.5e-11, 2.4e-19),
    "elim-three_launch":       (5.9e-15, 9.5e-15, 5.9e-15, 4.0e-14, 5.0e-15),
    "elim-generic":            (2.8e-15, 3.4e-15, 2.8e-15, 2.9e-14, 2.8e-15),
    "elim-one_child":          (5.1e-16, 8.9e-16, 8.1e-16, 4.5e-15, 4.0e-16),
    "elim-three_children":     (1.0e-15, 2.1e-15, 4.3e-15, 1.7e-14, 1.2e-15),
    "elim-dense_kind1_root":   (6.1e-16, 7.3e-16, 6.4e-16, 5.4e-15, 5.8e-16),
    "states-persist_c1":       (1.2e-13, 8.4e-12, 4.5e-12, 1.5e-09, 1.2e-18),
    "states-mpersist":         (8.3e-14, 9.8e-12, 4.8e-12, 1.3e-09, 2.7e-19),
    "states-single_wg":        (2.6e-15, 6.5e-15, 1.6e-14, 3.8e-14, 1.8e-20),
    "states-generic":          (2.9e-15, 5.2e-15, 2.9e-15, 2.3e-14, 5.0e-16),
    "states-tiered_ub":        (3.7e-11, 3.8e-11, 4.2e-11, 1.2e-08, 3.0e-16),
    "states-one_child":        (2.7e-15, 2.7e-15, 2.7e-15, 1.8e-14, 4.0e-20),
    "states-three_children":   (7.8e-16, 2.4e-15, 1.7e-15, 6.0e-15, 9.7e-17),
}
FLOOR = 1e-12


def tol(cid, what):
    """10 times the CPU spread of the quantity, with a floor of 1e-12 (the device's order of sums is a third one)"""
    return max(10.0 * SPREAD[cid][("K", "dx", "du", "dlam", "fd").index(what)], FLOOR if what != "fd" else 0.0)

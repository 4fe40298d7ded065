"""Cases of the adjoint tests (test_adj_reference.py on the CPU, test_gpu_mpc_adjoint.py on the device): every case of sens_cases, and from
mpc_limit_cases the sensitivity cases on both sides of the root block's d 64 | 65 (both root forms), a non-root block 32 + 32 | 33 + 32, a
kind-0 node's nz 64 | 65, a kind-1 eliminated root with S0 at nu[0] 64 | 65, nx0 64 | 65 for both root forms, the two Nh == 1 trees and
nx0 = nu[0] = 1.  A case is the dict of sens_cases with two more keys: w = (wx, wu), the loss gradient, nw columns of multiples of 2^-6 from
a seeded generator, and dtheta = (dq, dr, db), the direction of the finite-difference check, multiples of 2^-22 of size 2^-16.

nw = 1 everywhere; NW3 names the two cases, one per root form, that also run with three columns (w3).

Importing this module must not load the native library: test_adj_reference.py is collected ahead of the modules that decide which HIP
runtime the process gets, and mpc_cases loads the library when it is imported.  So the ids are written out here (test_adj_reference.py
checks them against sens_cases and mpc_limit_cases) and the case modules are imported where a case is built."""
from __future__ import annotations

import functools

import numpy as np

SENS_IDS = ("elim-single_wg", "elim-persist_c1", "elim-three_launch", "elim-generic", "elim-one_child", "elim-three_children", "elim-dense_kind1_root",
            "states-persist_c1", "states-mpersist", "states-single_wg", "states-generic", "states-tiered_ub", "states-one_child", "states-three_children")
LIMIT_IDS = ("root_d-elim_d64", "root_d-elim_d65", "root_d-states_d64", "root_d-states_d65", "node_d-d64", "node_d-d65",
             "kind0_nz-nz64", "kind0_nz-nz65", "kind1_nz-nz64", "kind1_nz-nz65", "nx0_elim-64", "nx0_elim-65", "nx0_states-64", "nx0_states-65",
             "Nh1-one_leaf", "Nh1-three_leaves", "smallest-nx0_1_nu0_1")
CASE_IDS = list(SENS_IDS) + list(LIMIT_IDS)
NW3 = ("elim-three_children", "states-generic")
FD_H = 2.0 ** -16           # as sens_cases.FD_H: entries are multiples of 2^-22
# the tree whose largest nz is 40 (mpc_limit_cases.WINDOW_TREE) and the first nw whose nz x nw window exceeds 160 KiB there
WINDOW_ID = "lds_window-accepted"
WINDOW_NW = (160 * 1024 // 8 - 2) // 40 + 1


def _w(c, nw, seed):
    import mpc_cases as MC
    rng = np.random.Generator(np.random.PCG64(seed + 4242))
    sx, su = int(np.sum(c["d"]["nx"])), int(np.sum(c["d"]["nu"]))
    return MC.quantised(rng, (sx, nw), 1.0), MC.quantised(rng, (su, nw), 1.0)


@functools.lru_cache(maxsize=None)
def case(cid):
    import mpc_cases as MC
    import mpc_limit_cases as ML
    import sens_cases as SN
    c = dict(SN.case(cid) if cid in SENS_IDS else ML.case(cid))
    seed = SN._seed(cid)
    c["w"] = _w(c, 1, seed)
    if cid in NW3:
        c["w3"] = _w(c, 3, seed + 1)
    rng = np.random.Generator(np.random.PCG64(seed + 777))
    c["dtheta"] = tuple(FD_H * MC.quantised(rng, len(c["d"][k]), 1.0) for k in ("q", "r", "b"))
    return c


def problem_plus(c, scale=1.0):
    """the case's flat problem with q, r, b moved along dtheta"""
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    for k, dv in zip(("q", "r", "b"), c["dtheta"]):
        d[k] = d[k] + scale * dv
    return d


# Measured by test_adj_reference.py (it prints them with -s and asserts that they still hold): per case the spread max |(a) - (b)| of gq,
# gr, gb, gx0 between the two numpy evaluations of adj_ref at the oracle's point (gb where the block form regularises nothing), and the
# discrepancy |w' (z(theta + dtheta) - z(theta)) - g' dtheta| against the oracle's solves at stationarityTolerance 1e-12.  The device tests
# allow 10 times the spreads, with a floor of 1e-12.
SPREAD = {
    #                              gq       gr       gb       gx0      fd
    "elim-single_wg":           (1.4e-15, 1.2e-15, 1.3e-14, 8.9e-15, 1.3e-16),
    "elim-persist_c1":          (6.5e-14, 8.1e-14, 3.3e-12, 2.8e-12, 8.8e-14),
    "elim-three_launch":        (2.3e-15, 1.7e-15, 1.3e-14, 1.5e-14, 4.0e-15),
    "elim-generic":             (2.0e-15, 1.3e-15, 7.7e-15, 6.0e-15, 3.0e-15),
    "elim-one_child":           (9.0e-16, 1.5e-15, 1.5e-15, 4.6e-16, 2.1e-16),
    "elim-three_children":      (1.3e-15, 2.2e-15, 3.7e-15, 3.6e-15, 9.8e-16),
    "elim-dense_kind1_root":    (6.4e-16, 6.1e-16, 1.5e-15, 6.7e-16, 1.7e-16),
    "states-persist_c1":        (6.1e-14, 4.4e-14, 5.8e-12, 5.1e-12, 3.6e-14),
    "states-mpersist":          (6.1e-14, 2.8e-14, 6.0e-12, 1.7e-11, 2.9e-14),
    "states-single_wg":         (1.1e-15, 3.6e-15, 9.8e-15, 1.1e-14, 8.5e-17),
    "states-generic":           (1.6e-15, 1.2e-15, 1.3e-14, 1.1e-14, 2.4e-17),
    "states-tiered_ub":         (2.3e-13, 1.4e-13, 4.7e-11, 1.2e-10, 1.5e-15),
    "states-one_child":         (5.7e-16, 7.1e-16, 1.5e-15, 1.7e-15, 7.6e-17),
    "states-three_children":    (7.8e-16, 1.8e-15, 3.0e-15, 2.9e-15, 8.1e-17),
    "root_d-elim_d64":          (2.4e-15, 2.4e-15, 9.7e-15, 1.3e-14, 1.4e-15),
    "root_d-elim_d65":          (1.6e-15, 2.6e-15, 1.3e-14, 8.9e-15, 3.0e-15),
    "root_d-states_d64":        (2.7e-15, 1.9e-15, 2.2e-14, 1.4e-14, 5.9e-16),
    "root_d-states_d65":        (1.9e-15, 2.8e-15, 8.9e-15, 8.1e-15, 4.1e-16),
    "node_d-d64":               (2.7e-15, 9.4e-16, 1.2e-14, 7.7e-15, 5.6e-17),
    "node_d-d65":               (1.0e-14, 3.3e-15, 7.2e-14, 1.4e-14, 4.0e-16),
    "kind0_nz-nz64":            (2.4e-15, 2.7e-15, 7.2e-15, 3.8e-15, 3.5e-16),
    "kind0_nz-nz65":            (2.8e-15, 2.9e-15, 6.2e-15, 9.0e-15, 4.9e-16),
    "kind1_nz-nz64":            (1.7e-15, 1.6e-15, 7.1e-15, 1.4e-15, 3.8e-16),
    "kind1_nz-nz65":            (7.0e-16, 1.2e-15, 3.0e-15, 2.0e-15, 1.1e-15),
    "nx0_elim-64":              (6.0e-16, 7.3e-16, 2.2e-15, 3.9e-16, 7.3e-17),
    "nx0_elim-65":              (4.2e-16, 5.5e-16, 1.3e-15, 1.3e-16, 4.1e-17),
    "nx0_states-64":            (1.7e-15, 1.7e-15, 6.4e-15, 4.7e-15, 3.5e-17),
    "nx0_states-65":            (3.5e-15, 4.3e-15, 4.9e-15, 1.3e-14, 3.2e-17),
    "Nh1-one_leaf":             (2.0e-16, 4.0e-16, 3.9e-16, 2.1e-16, 7.8e-17),
    "Nh1-three_leaves":         (9.5e-16, 1.4e-15, 5.7e-15, 4.5e-15, 8.9e-17),
    "smallest-nx0_1_nu0_1":     (3.5e-16, 5.9e-16, 9.9e-16, 2.1e-16, 7.5e-17),
}
FLOOR = 1e-12
WHAT = ("gq", "gr", "gb", "gx0", "fd")


def tol(cid, what):
    """10 times the CPU spread of the quantity, with a floor of 1e-12 (the device's order of sums is a third one)"""
    return max(10.0 * SPREAD[cid][WHAT.index(what)], FLOOR if what != "fd" else 0.0)

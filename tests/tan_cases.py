"""Cases of the tangent tests (test_tan_reference.py on the CPU, test_gpu_mpc_tangent.py on the device).

Tangent: adj_cases.case(cid) for the ids below -- the smallest shapes on which k_tan_rhs / k_tan_primal can go wrong: nx0 = nu[0] = 1, the two
Nh == 1 trees (no forward launch), one and three children under both root forms, the kind-1 root with S0, the generic and the single-workgroup
trees, and both sides of every 64-lane boundary the bodies loop over (the root block's d, a non-root block's d, a kind-0 node's nz, nx0 under both
root forms).  A case carries adj_cases' dtheta = (dq, dr, db) of size 2^-16 and w; this module adds dx0, a seeded direction of the same
quantisation (multiples of 2^-22 of size 2^-16), and for ND3 three columns of all four (dirs3).

Predictor: adjbnd_cases.track_case for one tracking case per root form and the kind-1 eliminated root with S0, with a trajectory whose rows differ
by 2^-8 of the table's (so that a window move is a small finite change), a window move MOVE[cid] = (t0, t0_new) and x0_new = x0 + dx0 of size 2^-10.

Importing this module must not load the native library (see adj_cases)."""
from __future__ import annotations

import functools

import numpy as np

import adj_cases as AC

CASE_IDS = ["smallest-nx0_1_nu0_1", "Nh1-one_leaf", "Nh1-three_leaves", "elim-one_child", "elim-three_children", "states-three_children",
            "elim-dense_kind1_root", "states-generic", "elim-single_wg", "root_d-elim_d64", "root_d-elim_d65", "node_d-d64", "node_d-d65",
            "kind0_nz-nz64", "kind0_nz-nz65", "nx0_elim-64", "nx0_elim-65", "nx0_states-64", "nx0_states-65"]
ND3 = ("elim-three_children", "states-generic")
TRACK_IDS = ("single_wg", "c1_eliminated", "kind1_S0")
FD_H = AC.FD_H
TRACK_SHRINK = 2.0 ** -8          # the rows of a predictor case's trajectory: row 0 + TRACK_SHRINK (row - row 0)
TRACK_DX0 = 2.0 ** -10
WINDOW_ID, WINDOW_ND = AC.WINDOW_ID, AC.WINDOW_NW


def _dirs(c, nd, seed):
    import mpc_cases as MC
    rng = np.random.Generator(np.random.PCG64(seed + 999))
    rows = (len(c["d"]["q"]), len(c["d"]["r"]), len(c["d"]["b"]), int(c["nx0"]))
    return tuple(FD_H * MC.quantised(rng, (n, nd), 1.0) for n in rows)


@functools.lru_cache(maxsize=None)
def case(cid):
    import sens_cases as SN
    c = dict(AC.case(cid))
    seed = SN._seed(cid)
    rng = np.random.Generator(np.random.PCG64(seed + 888))
    import mpc_cases as MC
    c["dx0"] = FD_H * MC.quantised(rng, int(c["nx0"]), 1.0)
    c["dirs"] = tuple(np.asarray(v, dtype=np.float64).reshape(-1, 1) for v in (*c["dtheta"], c["dx0"]))
    if cid in ND3:
        c["dirs3"] = _dirs(c, 3, seed)
    return c


def problem_plus(c):
    """(the case's flat problem with q, r, b moved along dtheta, x0 + dx0)"""
    return AC.problem_plus(c), c["x0"] + c["dx0"]


def window_case():
    import mpc_limit_cases as ML
    return ML.case(WINDOW_ID)


@functools.lru_cache(maxsize=None)
def track_case(cid):
    import adjbnd_cases as BC
    c = dict(BC.track_case(cid))
    for key in ("xtraj", "utraj"):
        c[key] = c[key][0] + TRACK_SHRINK * (c[key] - c[key][0])
    t0 = BC.windows(c)[0]
    c["move"] = (t0, t0 + 1)
    rng = np.random.Generator(np.random.PCG64(sum(ord(ch) for ch in cid) + 5))
    c["x0_new"] = c["x0"] + TRACK_DX0 * np.round(64.0 * rng.uniform(-1.0, 1.0, int(c["nx0"]))) / 64.0
    return c


# Measured by test_tan_reference.py (it prints them with -s and asserts that they still hold): per case the spread max |(a) - (b)| of dx, du,
# dlam, du0 between the two numpy evaluations of tan_ref at the oracle's point for the case's direction (dq, dr, db, dx0) (dlam where the
# block form regularises nothing), and fd, the discrepancy max |z(theta + dtheta, x0 + dx0) - z(theta, x0) - dZ| against the oracle's solves
# at stationarityTolerance 1e-12 (None: the set of bound-sitting entries differs at the two points, the case drops out of that check).
# The directions are of size 2^-16, so dZ is of size 1e-5 and most spreads lie below 1e-17: those are recorded as 1.0e-17.
# The device tests allow 10 times the spreads, with a floor of 1e-12.
SPREAD = {
    #                              dx       du       dlam     du0      fd
    "smallest-nx0_1_nu0_1":     (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 4.9e-17),
    "Nh1-one_leaf":             (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 9.0e-17),
    "Nh1-three_leaves":         (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.2e-16),
    "elim-one_child":           (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 3.3e-16),
    "elim-three_children":      (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.0e-15),
    "states-three_children":    (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.5e-16),
    "elim-dense_kind1_root":    (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 4.4e-16),
    "states-generic":           (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 5.4e-16),
    "elim-single_wg":           (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.4e-16),
    "root_d-elim_d64":          (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 3.8e-15),
    "root_d-elim_d65":          (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 4.7e-15),
    "node_d-d64":               (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.7e-16),
    "node_d-d65":               (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.8e-15),
    "kind0_nz-nz64":            (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 3.4e-16),
    "kind0_nz-nz65":            (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 3.5e-16),
    "nx0_elim-64":              (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 3.2e-16),
    "nx0_elim-65":              (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.9e-17),
    "nx0_states-64":            (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 1.4e-16),
    "nx0_states-65":            (1.0e-17, 1.0e-17, 1.0e-17, 1.0e-17, 2.4e-16),
}
TRACK_SPREAD = {
    #                              dx       du       dlam     du0      fd
    "single_wg":                (1.0e-17, 1.0e-17, 1.7e-17, 1.0e-17, 7.9e-17),
    "c1_eliminated":            (1.9e-15, 1.3e-15, 1.9e-13, 1.2e-16, 5.5e-14),
    "kind1_S0":                 (1.0e-17, 1.0e-17, 1.9e-17, 1.0e-17, 6.4e-16),
}
FLOOR = AC.FLOOR
WHAT = ("dx", "du", "dlam", "du0", "fd")


def tol(cid, what):
    """10 times the CPU spread of the quantity, with the floor of adj_cases (the device's order of sums is a third one)"""
    table = SPREAD if cid in SPREAD else TRACK_SPREAD
    return max(10.0 * table[cid][WHAT.index(what)], FLOOR)

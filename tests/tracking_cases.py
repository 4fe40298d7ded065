"""Problems of the tracking-MPC tests (test_gpu_mpc_tracking.py): trees with one nx and one nu on every node (roots and leaves apart), one
per route, a reference trajectory per case, and the numpy fold of a reference window into q, r that the device is compared with.

A case is a dict with the keys of mpc_cases (form "elim": the root is eliminated, `root` holds its originals) or of mpc_root_cases (form
"states": the root keeps its states and x0 enters through its bounds), and: NXT, NUT, T, xtraj (T, NXT), utraj (T, NUT), q0, r0 (the
base linear terms, flat), x0s (the x0 of the steps).  `exact` cases hold multiples of 2^-6 of size <= 4 everywhere the fold reads, so that
every sum of the fold is exact in any order (nx + nu <= 64).  Every tree comes from code the suite already has."""
from __future__ import annotations

import functools

import numpy as np

import helpers as H
import limit_shapes as S
import mpc_cases as M
import mpc_root_cases as R
import solve_sequence_cases as SC

T_LEN = 6
WINDOWS = (0, 1, 3, 5, 9)          # with stages up to Nh: rows beyond T - 1 = 5 (the clamp) from the second window on


def stages(nk):
    nk = np.asarray(nk, dtype=int)
    st, nxt = np.zeros(len(nk), dtype=int), 1
    for k, n in enumerate(nk):
        st[nxt:nxt + n] = st[k] + 1
        nxt += n
    return st


def quantise(v, lo=None):
    """the nearest multiples of 2^-6, at most 4 in size (lo: at least that, for weights)"""
    v = np.clip(np.round(np.asarray(v, dtype=np.float64) * M.Q6) / M.Q6, -4.0, 4.0)
    return v if lo is None else np.maximum(v, lo)


def blocks(d, k):
    """(Q_k, R_k, S_k) of node k of the flat problem d, dense; a clipping problem gives diagonal Q, R and S = 0"""
    nx, nu = [np.asarray(d[n], dtype=int) for n in ("nx", "nu")]
    xo, uo = H.offsets(d)
    if "Q" not in d:
        return np.diag(d["Qd"][xo[k]:xo[k + 1]]), np.diag(d["Rd"][uo[k]:uo[k + 1]]), np.zeros((nu[k], nx[k]))
    oq, orr, os = int((nx[:k] ** 2).sum()), int((nu[:k] ** 2).sum()), int((nx[:k] * nu[:k]).sum())
    return (d["Q"][oq:oq + nx[k] ** 2].reshape((nx[k], nx[k]), order="F"), d["R"][orr:orr + nu[k] ** 2].reshape((nu[k], nu[k]), order="F"),
            d["S"][os:os + nx[k] * nu[k]].reshape((nu[k], nx[k]), order="F"))


def fold(c, t0, x0=None, bound=False):
    """the numpy fold of window t0 -> (q, r) flat; x0: of an eliminated root with S0 (r[0] += S0 (x0 - xref)).
    bound=True: (q, r, bq, br) with the general-data bound of every entry, 2 (n + 1) eps (|base_i| + sum_j |H_ij ref_j|), n the terms of
    the entry's chain: nx_k + nu_k of its node.  r[0] of an eliminated root with S0 is the one longer chain, nu_0 + 2 nx0 terms (R_0 uref,
    S0 xref, S0 x0), whose products are in its sum: n is that count there, and only there -- the form of the bound is the same, and it has
    to cover the chain's n roundings of the device and the n + 1 of this reference."""
    d = c["d"]
    nx, nu = [np.asarray(d[n], dtype=int) for n in ("nx", "nu")]
    xo, uo = H.offsets(d)
    st = stages(d["nk"])
    q, r = np.array(c["q0"], copy=True), np.array(c["r0"], copy=True)
    bq, br = np.abs(q), np.abs(r)
    nq, nr = np.repeat(nx + nu, nx).astype(np.float64), np.repeat(nx + nu, nu).astype(np.float64)          # terms of each entry's chain
    for k in range(len(nx)):
        row = min(t0 + st[k], c["T"] - 1)
        xr = c["xtraj"][row] if nx[k] else np.zeros(0)
        ur = c["utraj"][row] if nu[k] else np.zeros(0)
        Q, Rm, Sm = blocks(d, k)
        for j in range(nx[k]):
            q[xo[k]:xo[k + 1]] -= Q[:, j] * xr[j]
            r[uo[k]:uo[k + 1]] -= Sm[:, j] * xr[j]
            bq[xo[k]:xo[k + 1]] += np.abs(Q[:, j] * xr[j])
            br[uo[k]:uo[k + 1]] += np.abs(Sm[:, j] * xr[j])
        for j in range(nu[k]):
            q[xo[k]:xo[k + 1]] -= Sm[j, :] * ur[j]
            r[uo[k]:uo[k + 1]] -= Rm[:, j] * ur[j]
            bq[xo[k]:xo[k + 1]] += np.abs(Sm[j, :] * ur[j])
            br[uo[k]:uo[k + 1]] += np.abs(Rm[:, j] * ur[j])
    S0 = c["root"]["S0"] if c["form"] == "elim" else None
    if S0 is not None:
        xr = c["xtraj"][min(t0, c["T"] - 1)]
        x0 = np.zeros(c["nx0"]) if x0 is None else x0
        for j in range(c["nx0"]):
            r[:nu[0]] -= S0[:, j] * xr[j]
            br[:nu[0]] += np.abs(S0[:, j] * xr[j])
        for j in range(c["nx0"]):
            r[:nu[0]] += S0[:, j] * x0[j]
            br[:nu[0]] += np.abs(S0[:, j] * x0[j])
        nr[:nu[0]] = nu[0] + 2 * c["nx0"]
    eps = np.finfo(np.float64).eps
    return (q, r, 2 * (nq + 1) * eps * bq, 2 * (nr + 1) * eps * br) if bound else (q, r)


def _reference(c, seed, exact, T=T_LEN, scale=0.25):
    rng = np.random.Generator(np.random.PCG64(seed + 700))
    d = c["d"]
    nx, nu = np.asarray(d["nx"], dtype=int), np.asarray(d["nu"], dtype=int)
    c["NXT"], c["NUT"], c["T"] = int(nx.max()), int(nu.max()), T
    assert set(nx.tolist()) <= {0, c["NXT"]} and set(nu.tolist()) <= {0, c["NUT"]}, f"{c['id']}: not uniform"
    assert c["NXT"] + c["NUT"] <= 64
    if exact:
        c["xtraj"], c["utraj"] = M.quantised(rng, (T, c["NXT"]), 1.0), M.quantised(rng, (T, c["NUT"]), 1.0)
        c["q0"], c["r0"] = M.quantised(rng, len(d["q"]), 1.0), M.quantised(rng, len(d["r"]), 1.0)
    else:
        c["xtraj"], c["utraj"] = scale * rng.standard_normal((T, c["NXT"])), scale * rng.standard_normal((T, c["NUT"]))
        c["q0"], c["r0"] = np.array(d["q"], copy=True), np.array(d["r"], copy=True)
    return c


def _quantised_problem(d):
    """the weights (everything the fold multiplies the reference with) as multiples of 2^-6"""
    d = {k: np.array(v, copy=True) for k, v in d.items()}
    for k in ("Qd", "Rd"):
        d[k] = quantise(d[k], 1.0 / M.Q6)
    if "Q" in d:
        # off-diagonal entries are rounded, the diagonals only grow: H stays positive definite by more than the rounding takes
        nx, nu = np.asarray(d["nx"], dtype=int), np.asarray(d["nu"], dtype=int)
        for name, n in (("Q", nx), ("R", nu)):
            at = 0
            for k in range(len(n)):
                B = d[name][at:at + n[k] ** 2].reshape((n[k], n[k]), order="F")
                Bq = quantise(B)
                Bq[np.diag_indices(n[k])] = quantise(np.diag(B) + (n[k] + nu[k] + nx[k]) / (2 * M.Q6))
                d[name][at:at + n[k] ** 2] = Bq.ravel(order="F")
                at += n[k] ** 2
        d["S"] = quantise(d["S"])
    return d


def _states(cid, d, seed, exact, kinds=None, env=None, opts=None, path=None):
    c = R._case(cid, _quantised_problem(d) if exact else d, kinds=kinds, env=env, opts=opts, path=path)
    c.update(form="states", single=False, root=None, seed=seed)
    c["x0s"] = [c["x0"] * (1.0 + 0.02 * np.sin(0.7 * s + np.arange(c["nx0"]))) for s in range(12)]
    return _reference(c, seed, exact)


def _elim(cid, d, nx0, seed, exact, kinds=None, env=None, opts=None, path=None):
    c = M._case(cid, _quantised_problem(d) if exact else d, nx0, seed, kinds=kinds, env=env, opts=opts, path=path)
    c.update(form="elim", seed=seed)
    c["x0s"] = M.exact_x0s(nx0, seed) + M.exact_x0s(nx0, seed + 1) + M.exact_x0s(nx0, seed + 2)
    return _reference(c, seed, exact)


def _dense_elim(seed, exact):
    """4 nodes, nx = 3 below an eliminated root of kind 2 whose S0 enters r[0]"""
    d, kinds = M._dense([2, 1, 0, 0], [0, 3, 3, 3], 2, seed, 2)
    return _elim("dense_kind2_root_S0", d, 3, seed, exact, kinds=kinds, opts=SC.FULL)


def _dense_states(seed, exact):
    """4 nodes, nx = 3 everywhere, every node of kind 2 under a root of kind 3 (two rows) that keeps its states"""
    d = H.dense_shaped_qp([2, 1, 0, 0], [3, 3, 3, 3], 2, seed)
    kinds = np.full(4, 2, dtype=np.int32)
    kinds[0] = 3
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    d["nc"] = np.array([2, 0, 0, 0], dtype=np.int32)
    d["C"] = 0.25 * rng.standard_normal(2 * 3)
    d["D"] = rng.standard_normal(2 * int(d["nu"][0]))
    d["dmin"], d["dmax"] = -2.0 * np.ones(2), 2.0 * np.ones(2)
    return _states("dense_kind3_root", d, seed, exact, kinds=kinds, opts=SC.FULL)


def active_rows_case(seed=32, span=0.0625, exact=True):
    """the tree of dense_kind3_root with both parents of kind 3 and their rows tight: D u within +- span on the root, C x + D u within
    +- span on node 1, so that rows are in the working sets at a solution (test_working_sets_survive_a_window_move asserts that they are)"""
    d = H.dense_shaped_qp([2, 1, 0, 0], [3, 3, 3, 3], 2, seed)
    kinds = np.array([3, 3, 2, 2], dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    nu0 = int(d["nu"][0])
    d["nc"] = np.array([2, 2, 0, 0], dtype=np.int32)
    d["C"] = np.concatenate([np.zeros(2 * 3), M.quantised(rng, 2 * 3, 0.25)])
    d["D"] = M.quantised(rng, 2 * nu0 + 2 * int(d["nu"][1]), 1.0)
    d["dmin"], d["dmax"] = -span * np.ones(4), span * np.ones(4)
    return _states(f"dense_kind3_active_rows-{seed}", d, seed, exact, kinds=kinds, opts=SC.FULL)


UNIFORM_SMALL = (3, 2, [(3, 2, [S.leaf(3)]), (3, 2, [S.leaf(3)])])          # 5 nodes: the single-workgroup kernel
UNIFORM_NZ32 = (20, 12, [(20, 12, [S.leaf(20)])])                           # blocks of d = 20 under parents of nx + nu = 32: three launches
UNIFORM_WIDE = S.fan(3, 6, kid_nu=2, root=(6, 2), grand=6)                  # root block of d = 18: the wide-block class, the smallest with one nx


def _shaped(shape, seed=11):
    nk, nx, nu = S.flatten(shape)
    return H.shaped_qp(nk, nx, nu, seed, ubound=0.3).as_dict()


@functools.lru_cache(maxsize=None)
def cases(exact=True):
    out = [
        _states("c1_root_states", R.case("persist_c1")["d"], 1, exact, path=2),
        _elim("c1_eliminated", M.case("persist_c1")["d"], M.case("persist_c1")["nx0"], 2, exact, path=2),
        _states("single_wg", _shaped(UNIFORM_SMALL), 3, exact, path=3),
        dict(_states("three_launch", _shaped(UNIFORM_NZ32), 4, exact), plan=("w3",)),
        _states("generic", _shaped(UNIFORM_SMALL), 5, exact, env=SC.GENERIC, path=0),
        # (a tree this small fits the single-workgroup kernel, which route_of prefers: the switch leaves the workgroup-per-block kernels)
        dict(_states("wide", _shaped(UNIFORM_WIDE), 6, exact, env=SC.GENERIC, path=0), plan=("wide",)),
        _dense_elim(23, exact),
        _dense_states(24, exact),
    ]
    return tuple(out)


CASE_IDS = [c["id"] for c in cases()]
PERSIST_IDS = ["c1_root_states", "c1_eliminated"]
CLIPPING_IDS = [c["id"] for c in cases() if c["kinds"] is None]
DENSE_IDS = [c["id"] for c in cases() if c["kinds"] is not None]


def case(cid, exact=True):
    return next(c for c in cases(exact) if c["id"] == cid)


def make(capi, c, tracking=True):
    """a fresh mirror of the case with its root declared (both forms) and, unless tracking=False, its reference trajectory on the device"""
    g = M.make(capi, c) if c["form"] == "elim" else R.make(capi, c, root_states=True)
    if tracking:
        g.mpc_set_tracking(c["xtraj"], c["utraj"], c["q0"], c["r0"])
    return g

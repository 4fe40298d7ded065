"""Problems of the MPC-step tests (test_gpu_mpc.py): x0-eliminated trees, one per route, with the originals of everything that
multiplies x0, and the numpy fold the device is compared with.

A case is a dict: d (the flat x0-eliminated problem, nx[0] == 0), kinds (None: clipping), root (A0 a list of (nx[kid], nx0)
matrices, b0, S0, r0, C0, dmin0, dmax0), env (creation-time switches), opts, single (opt in to the dense single launch).
Every tree comes from code the suite already has (solve_sequence_cases, limit_shapes, helpers, treeqp_amd.problems)."""
from __future__ import annotations

import functools

import numpy as np

import helpers as H
import limit_shapes as S
import solve_sequence_cases as SC
from treeqp_amd import problems as P

NX0 = 5                     # states of the eliminated root in the made-up root terms (C1 keeps the number its own root had)
EXACT_STEPS = 5
Q6 = 64.0                   # entries of the exact data are multiples of 2^-6


def quantised(rng, shape, size):
    """multiples of 2^-6 in [-size, size]"""
    return rng.integers(-int(size * Q6), int(size * Q6) + 1, size=shape).astype(np.float64) / Q6


def eliminate(d):
    """full-root flat clipping problem -> (x0-eliminated flat problem, nx0): the root's states, their weights and bounds and the root
    children's A leave; b stays as it is (the tests set it through the fold)"""
    nx0, nk0 = int(d["nx"][0]), int(d["nk"][0])
    nA0 = int(sum(int(d["nx"][k]) * nx0 for k in range(1, 1 + nk0)))
    e = {k: np.array(v, copy=True) for k, v in d.items()}
    e["nx"][0] = 0
    e["A"] = d["A"][nA0:]
    for k in ("Qd", "q", "xmin", "xmax"):
        e[k] = d[k][nx0:]
    return e, nx0


def root_terms(d, nx0, seed, kinds=None, scale=0.5):
    """made-up originals for the root of the x0-eliminated problem d, all entries multiples of 2^-6 and at most 4 in size: A0 per child,
    b0, and S0, r0 on a dense root, C0, dmin0, dmax0 on a root with rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nk0, nu0 = int(d["nk"][0]), int(d["nu"][0])
    root = dict(A0=[quantised(rng, (int(d["nx"][k]), nx0), scale) for k in range(1, 1 + nk0)],
                b0=quantised(rng, int(d["nx"][1:1 + nk0].sum()), 0.25), S0=None, r0=None, C0=None, dmin0=None, dmax0=None)
    if kinds is not None and kinds[0] != 0:
        root["S0"], root["r0"] = quantised(rng, (nu0, nx0), 0.25), quantised(rng, nu0, 0.5)
    if "nc" in d and int(d["nc"][0]) > 0:
        nc0 = int(d["nc"][0])
        root["C0"] = quantised(rng, (nc0, nx0), 0.125)
        root["dmin0"], root["dmax0"] = -2.0 - np.abs(quantised(rng, nc0, 0.5)), 2.0 + np.abs(quantised(rng, nc0, 0.5))
    return root


def fold(root, x0, order=None):
    """the numpy fold: b of the root's children, r[0], dmin[0], dmax[0] for this x0; order: a permutation of the columns (the exact
    data give the same bits in any order)"""
    j = np.arange(len(x0)) if order is None else np.asarray(order)

    def acc(v, M, sign=1.0):
        v = np.array(v, dtype=np.float64, copy=True)
        for c in j:
            v = v + sign * M[:, c] * x0[c]
        return v
    out, at = dict(), 0
    parts = []
    for A in root["A0"]:
        parts.append(acc(root["b0"][at:at + A.shape[0]], A))
        at += A.shape[0]
    out["b"] = np.concatenate(parts)
    if root["S0"] is not None:
        out["r"] = acc(root["r0"], root["S0"])
    if root["C0"] is not None:
        out["dmin"], out["dmax"] = acc(root["dmin0"], root["C0"], -1.0), acc(root["dmax0"], root["C0"], -1.0)
    return out


def fold_bound(root, x0):
    """entry by entry 2 nx0 eps (|b0| + sum_j |A0_ij x0_j|), the bound of the general-data test"""
    n = len(x0)
    parts, at = [], 0
    for A in root["A0"]:
        parts.append(np.abs(root["b0"][at:at + A.shape[0]]) + np.abs(A) @ np.abs(x0))
        at += A.shape[0]
    return 2 * n * np.finfo(np.float64).eps * np.concatenate(parts)


def folded(c, terms):
    """the case's flat problem with the folded terms in place"""
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    nb = len(terms["b"])
    d["b"][:nb] = terms["b"]
    if "r" in terms:
        d["r"][:len(terms["r"])] = terms["r"]
    if "dmin" in terms:
        d["dmin"][:len(terms["dmin"])] = terms["dmin"]
        d["dmax"][:len(terms["dmax"])] = terms["dmax"]
    return d


def exact_x0s(nx0, seed):
    rng = np.random.Generator(np.random.PCG64(seed + 101))
    return [quantised(rng, nx0, 1.0) for _ in range(EXACT_STEPS)]


def _case(cid, d, nx0, seed, kinds=None, env=None, opts=None, single=False, path=None):
    return dict(id=cid, d=d, kinds=kinds, root=root_terms(d, nx0, seed, kinds), nx0=nx0, env=env or {}, opts=opts or {}, single=single, path=path)


def _from_shape(cid):
    kind, shape, _ = S.case(cid)
    assert kind == S.C
    return eliminate(S.problem(kind, shape))


def _c1():
    """C1, the reference's spring-mass example (85 nodes), x0 eliminated: uniform again with a phantom root, so the persistent route"""
    p = P.spring_mass()
    nk = p.nk()
    from treeqp_amd import capi
    flat = capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()
    return eliminate(flat)


def _dense(nk, nx, nu, seed, root_kind):
    """a small dense tree with an eliminated root of kind 2 (S0 != 0 enters r[0]) or kind 3 (two rows on the root: D u within a range)"""
    d = H.dense_shaped_qp(nk, nx, nu, seed)
    kinds = np.full(len(d["nk"]), 2, dtype=np.int32)
    kinds[0] = root_kind
    if root_kind == 3:
        rng = np.random.Generator(np.random.PCG64(seed + 5))
        nc = np.zeros(len(d["nk"]), dtype=np.int32)
        nc[0] = 2
        d["nc"] = nc
        d["C"] = np.zeros(0)                                          # nc[0] x nx[0] = 2 x 0
        d["D"] = quantised(rng, 2 * int(d["nu"][0]), 1.0)
        d["dmin"], d["dmax"] = -2.0 * np.ones(2), 2.0 * np.ones(2)
    return d, kinds


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    d, _ = _from_shape("g_persist_node_sizes-nz16")
    out.append(_case("single_wg", d, NX0, 1, path=3))
    d, nx0 = _c1()
    out.append(_case("persist_c1", d, nx0, 2, path=2))
    d, _ = _from_shape("k_sgp-nz32_everywhere")
    out.append(_case("three_launch", d, NX0, 3))
    d, _ = _from_shape("forward_chain-nx9")
    out.append(_case("generic", d, NX0, 4, env=SC.GENERIC, path=0))
    out.append(_case("one_child", H.shaped_qp([1, 2, 0, 0], [0, 3, 2, 2], 2, 21).as_dict(), NX0, 5))
    out.append(_case("three_children", H.shaped_qp([3, 1, 1, 1, 0, 0, 0], [0, 2, 3, 4, 2, 2, 2], 2, 22).as_dict(), NX0, 6))
    d, kinds = _dense([2, 1, 0, 0], [0, 3, 2, 2], 2, 23, 2)
    out.append(_case("dense_kind2_root", d, NX0, 7, kinds=kinds, opts=SC.FULL))
    d, kinds = _dense([2, 1, 0, 0], [0, 3, 2, 2], 2, 24, 3)
    out.append(_case("dense_kind3_root", d, NX0, 8, kinds=kinds, opts=SC.FULL))
    return tuple(out)


CASE_IDS = [c["id"] for c in cases()]
CLIPPING_IDS = [c["id"] for c in cases() if c["kinds"] is None]


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def make(capi, c, d=None, root=True):
    """a fresh mirror of the case under its creation-time switches, the problem d (default: the case's own) uploaded, the root terms set"""
    d = c["d"] if d is None else d
    with SC.switches(c["env"]):
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    if c["kinds"] is None:
        g.upload(d)
    else:
        if "nc" in d:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, c["kinds"], None)
        if c["single"]:
            g.set_dense_single_launch(True)
    if root:
        r = c["root"]
        g.mpc_set_root(r["A0"], r["b0"], r["S0"], r["r0"], r["C0"], r["dmin0"], r["dmax0"])
    return g


def host_upload(g, c, terms):
    """the host loop's upload of a folded problem: tqgpu_set_problem on a clipping tree, the dense setters otherwise (dynamics for b, the
    objective for r -- there is no call for the linear terms alone --, the ranges of the rows alone)"""
    import ctypes as C
    d = folded(c, terms)
    L = __import__("treeqp_amd.capi", fromlist=["lib"]).lib()
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    if c["kinds"] is None:
        keep = [np.ascontiguousarray(d[k], dtype=np.float64) for k in ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax")]
        rc = L.tqgpu_set_problem(g.h, *[dp(a) for a in keep], None)
        assert rc == 0, L.tqgpu_last_error()
        return
    keep = [np.ascontiguousarray(d[k], dtype=np.float64) for k in ("A", "B", "b")]
    assert L.tqgpu_set_dynamics(g.h, *[dp(a) for a in keep]) == 0
    if "r" in terms:
        g.upload_mixed(d, c["kinds"], None)
    if "dmin" in terms:
        g.set_constraints(None, None, None, d["dmin"], d["dmax"])

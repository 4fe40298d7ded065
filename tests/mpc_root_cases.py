"""Problems of the root-states MPC-step tests (test_gpu_mpc_root.py): trees whose root keeps its states, one per route, where x0 enters
as xmin[0] = xmax[0] = x0, and the host loop the device loop is compared with.

A case is a dict: d (the flat problem, nx[0] > 0), kinds (None: clipping), env (creation-time switches), opts, path (the route that
tqgpu_uses_fused_path must report, None: not asserted), x0 (the problem's own x0, read from the root's bounds).
Every tree comes from code the suite already has (solve_sequence_cases, limit_shapes, helpers, treeqp_amd.problems)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import helpers as H
import limit_shapes as S
import solve_sequence_cases as SC
from treeqp_amd import problems as P

STEPS = 6
TIERED = {"TREEQP_AMD_PATH": "tiered"}
BOUNDS = ("xmin", "xmax", "umin", "umax")


def _lti_flat(p):
    from treeqp_amd import capi
    nk = p.nk()
    return capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()


def _shape(cid):
    kind, shape, _ = S.case(cid)
    assert kind == S.C
    return S.problem(kind, shape)


def _dense(seed, root_kind):
    """the dense tree of the issue: every node of kind 2, the root of kind `root_kind`; a root of kind 3 has two rows whose C is
    non-zero on the root's states"""
    d = H.dense_shaped_qp([2, 1, 0, 0], [3, 3, 2, 2], 2, seed)
    kinds = np.full(len(d["nk"]), 2, dtype=np.int32)
    kinds[0] = root_kind
    if root_kind == 3:
        rng = np.random.Generator(np.random.PCG64(seed + 5))
        nc = np.zeros(len(d["nk"]), dtype=np.int32)
        nc[0] = 2
        d["nc"] = nc
        d["C"] = 0.25 * rng.standard_normal(2 * int(d["nx"][0]))
        d["D"] = rng.standard_normal(2 * int(d["nu"][0]))
        d["dmin"], d["dmax"] = -2.0 * np.ones(2), 2.0 * np.ones(2)
        assert np.all(d["C"] != 0.0)
    return d, kinds


def _case(cid, d, kinds=None, env=None, opts=None, path=None):
    d = {k: np.array(v, copy=True) for k, v in d.items()}
    nx0 = int(d["nx"][0])
    x0 = d["xmin"][:nx0].copy()
    assert nx0 > 0 and np.all(np.isfinite(x0)) and np.array_equal(x0, d["xmax"][:nx0]), f"{cid}: the root's bounds do not hold an x0"
    return dict(id=cid, d=d, kinds=kinds, env=env or {}, opts=opts or {}, path=path, nx0=nx0, x0=x0)


@functools.lru_cache(maxsize=None)
def cases():
    c1 = _lti_flat(P.spring_mass())
    out = [
        _case("persist_c1", c1, path=2),
        _case("mpersist", _lti_flat(P.spring_mass(md=3, Nr=2, Nh=7)), path=2),          # (limit_shapes has no multistage tree: the one of solve_sequence_cases)
        _case("single_wg", _shape("g_persist_node_sizes-nz16"), path=3),
        _case("three_launch", _shape("k_sgp-nz32_everywhere")),
        _case("generic", _shape("forward_chain-nx9"), env=SC.GENERIC, path=0),
        # C1 created under the tiered switch: that switch only takes the persistent launch away, and a tree of 85 nodes then fits the
        # single-workgroup kernel, which route_of prefers (path 3); the tiered kernels are reached by the tiered tree of solve_sequence_cases
        _case("tiered_c1", c1, env=TIERED, path=3),
        _case("tiered", _lti_flat(P.linear_chain(2, 4, 4)), env=TIERED, path=1),
        _case("one_child", H.shaped_qp([1, 2, 0, 0], [3, 3, 2, 2], 2, 21).as_dict()),
        _case("three_children", H.shaped_qp([3, 1, 1, 1, 0, 0, 0], [4, 2, 3, 4, 2, 2, 2], 2, 22).as_dict()),
    ]
    d, kinds = _dense(23, 2)
    out.append(_case("dense_kind2_root", d, kinds=kinds, opts=SC.FULL))
    d, kinds = _dense(24, 3)
    out.append(_case("dense_kind3_root", d, kinds=kinds, opts=SC.FULL))
    return tuple(out)


CASE_IDS = [c["id"] for c in cases()]
CLIPPING_IDS = [c["id"] for c in cases() if c["kinds"] is None]


def case(cid):
    return next(c for c in cases() if c["id"] == cid)


def x0_sequence(c, seed=0, steps=STEPS):
    """x0 moving by 0.05 * standard_normal around the problem's own x0"""
    rng = np.random.Generator(np.random.PCG64(seed + 303))
    return [c["x0"] + 0.05 * rng.standard_normal(c["nx0"]) for _ in range(steps)]


def make(capi, c, d=None, root_states=False):
    """a fresh mirror of the case under its creation-time switches with the problem d (default: the case's own) uploaded"""
    d = c["d"] if d is None else d
    with SC.switches(c["env"]):
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    if c["kinds"] is None:
        g.upload(d)
    else:
        if "nc" in d:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, c["kinds"], None)
    if c["path"] is not None:
        assert g.path == c["path"], f"{c['id']}: route {g.path}, expected {c['path']}"
    if root_states:
        g.mpc_set_root_states()
    return g


def with_x0(c, x0, d=None):
    """the flat problem with the root's xmin, xmax replaced by x0"""
    d = {k: np.array(v, copy=True) for k, v in (c["d"] if d is None else d).items()}
    d["xmin"][:c["nx0"]] = x0
    d["xmax"][:c["nx0"]] = x0
    return d


def _dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))


def set_bounds(capi, g, d):
    keep = [np.ascontiguousarray(d[k], dtype=np.float64) for k in BOUNDS]
    rc = capi.lib().tqgpu_set_bounds(g.h, *[_dp(a) for a in keep])
    assert rc == 0, capi.lib().tqgpu_last_error()


def host_upload(capi, g, c, d):
    """the host loop's upload of the problem d (the root's bounds hold x0): tqgpu_set_problem on a clipping tree, the setter of the bounds
    on a dense one (as mpc_cases.host_upload: the dense setters)"""
    if c["kinds"] is None:
        keep = [np.ascontiguousarray(d[k], dtype=np.float64) for k in ("A", "B", "b", "Qd", "Rd", "q", "r") + BOUNDS]
        rc = capi.lib().tqgpu_set_problem(g.h, *[_dp(a) for a in keep], None)
        assert rc == 0, capi.lib().tqgpu_last_error()
    else:
        set_bounds(capi, g, d)


def host_step(capi, g, c, x0, d=None, **extra):
    """one step of the host loop on the twin g (tqgpu_set_warm_start was called once, by the caller): upload with the root's bounds
    replaced by x0, solve, download -> (result, solution)"""
    host_upload(capi, g, c, with_x0(c, x0, d))
    r = g.solve(**{**c["opts"], **extra})
    return r, g.solution()

"""KKT residuals evaluated on the device (tqgpu_kkt_residual, _at, _batch: k_kkt, one wave per node, and k_kkt_max) against the
numpy reference kkt_ref.py, which test_kkt_reference.py holds to the host's tree_qp_out_calculate_KKT_res.

Tolerance (derived in kkt_ref.py, not chosen): a class maximum within the largest 2 (m + 2) eps T among the class's entries, a
node's maximum within the largest among the node's; node[c] equal to the reference's wherever the two largest node maxima of the
reference lie further apart than twice that bound -- asserted to hold for every class at the random points, so that no
comparison is passed over there.  Infinities and NaNs must match exactly.

Shapes are the smallest that take each path of the kernel: nu = 0 and uneven children (a), nodes beyond one wave of 64 entries
on a dense and on a clipping node (b), kinds 0 / 1 / 2 / 3 with a kind-3 node without rows, an equality row and a row with an
infinite side (c), the phantom root states of an embedded x0-eliminated tree (d).  Clipping trees have no rows (rows apply on
nodes of kind 3): there the two row classes are empty in the reference too, node -1, and the other four are non-zero."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gen_cases as GC
import kkt_ref as K
import limit_shapes as LS
import mpc_root_cases as R
from helpers import product_qp_from_lti, with_dense_blocks
from limit_shapes import leaf
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -2, -4
FULL = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _clip_mirror(gpu, d, lam0=None):
    return gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d, lam0)


def _dense_mirror(gpu, d, kinds, lam0=None):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if "nc" in d:
        g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    return g.upload_mixed(d, kinds, lam0)


def _agree(got, want, bound):
    got, want, bound = np.broadcast_arrays(np.asarray(got, float), np.asarray(want, float), np.asarray(bound, float))
    special = ~np.isfinite(want)
    with np.errstate(invalid="ignore"):
        ok = np.where(special, (np.isnan(got) & np.isnan(want)) | (got == want), np.abs(got - want) <= np.where(special, 0.0, bound))
    return bool(np.all(ok))


def _check(got, ref, what):
    """device dict (with per_node) against the reference of the same point"""
    print(f"{what}: res {got['res']} node {got['node']}\n  ref {ref['res']} node {ref['node']}\n  bound {ref['bound']}")
    assert _agree(got["res"], ref["res"], ref["bound"]), what
    assert _agree(got["per_node"], ref["per_node"], ref["node_bound"]), what
    clear = K.node_is_clear(ref)
    assert np.array_equal(got["node"][clear], ref["node"][clear]), what
    assert np.array_equal(got["node"] < 0, ref["node"] < 0), what
    assert (np.isnan(got["max"]) and np.isnan(ref["max"])) or _agree(got["max"], ref["max"], np.nanmax(ref["bound"])), what


def _same(a, b, what):
    for k in ("res", "node", "per_node"):
        if k in a or k in b:
            assert np.array_equal(a[k], b[k], equal_nan=k != "node"), f"{what}: {k} differs"


def _random_point_check(g, d, kinds, seed, classes, sol=None):
    sol = K.random_point(d, seed) if sol is None else sol
    ref = K.residuals(d, sol, kinds)
    assert np.all(ref["res"][classes] > 1e-3), ref["res"]
    assert K.node_is_clear(ref).all()
    got = g.kkt_residual_at(sol, per_node=True)
    _check(got, ref, "random point")
    return sol, ref, got


ALL6, FIRST4 = np.arange(6), np.arange(4)
CLIP4 = (3, 2, [(2, 1, [leaf(1)]), leaf(4)])          # root (3, 2); kids (2, 1) and (4, 0); a grandchild (1, 0) under the first kid


# ---- random points through _at ----

def test_a_irregular_clipping_tree(gpu):
    d = K.random_problem(CLIP4, [0] * 4, 11)
    g = _clip_mirror(gpu, d)
    _, ref, got = _random_point_check(g, d, [0] * 4, 11, FIRST4)
    assert list(got["node"][4:]) == [-1, -1] and list(got["res"][4:]) == [0.0, 0.0]
    g.close()


def test_b_nodes_beyond_one_wave(gpu):
    shape, kinds = (50, 30, [(70, 1, [leaf(2)]), (3, 2, [leaf(2)])]), [1, 0, 0, 0, 0]
    d = K.random_problem(shape, kinds, 12)
    g = _dense_mirror(gpu, d, kinds)
    _, ref, got = _random_point_check(g, d, kinds, 12, FIRST4)
    assert got["per_node"][0, K.BFEAS] == 0.0 and got["per_node"][0, K.BCOMPL] == 0.0          # kind 1: bounds ignored
    g.close()


def _mixed_problem():
    """gen_cases' `mixed` row (kinds 3, 0, 2, 1, 3, 2, 1; rows on nodes 0 and 4) with node 2 asked for as kind 3 without rows, the
    second row of node 0 open above and the row of node 4 an equality"""
    d, _ = GC.build(GC.row("mixed"), 0)
    d = {k: np.array(v, copy=True) for k, v in d.items()}
    assert list(d["nc"]) == [2, 0, 0, 0, 1, 0, 0]
    d["dmax"][1] = np.inf
    d["dmin"][2] = d["dmax"][2] = 0.25
    return d, np.array([3, 0, 3, 1, 3, 2, 1], np.int32)


def test_c_kinds_two_and_three(gpu):
    d, kinds = _mixed_problem()
    g = _dense_mirror(gpu, d, kinds)
    assert g.plan["gen"] and g.plan["box"]
    sol = K.random_point(d, 13)
    sol["mu_d"][1] = -abs(sol["mu_d"][1])            # against the finite side of the half-open row
    _random_point_check(g, d, kinds, 13, ALL6, sol)
    # NULL multipliers are zero arrays, bit for bit
    bare = dict(x=sol["x"], u=sol["u"], lam=sol["lam"])
    zeros = dict(bare, mu_x=np.zeros_like(sol["x"]), mu_u=np.zeros_like(sol["u"]), mu_d=np.zeros_like(sol["mu_d"]))
    _same(g.kkt_residual_at(bare, per_node=True), g.kkt_residual_at(zeros, per_node=True), "NULL multipliers")
    g.close()


@pytest.mark.parametrize("generic", [False, True], ids=["embedded", "generic"])
def test_d_x0_eliminated_tree(gpu, monkeypatch, generic):
    p = P.linear_chain(2, 2, 2, nm=1, nu=1)                  # md = 2, three levels, nx = 2, nu = 1: 7 nodes
    flat = product_qp_from_lti(gpu, p, eliminate_x0=True).flat()
    assert list(flat["nx"]) == [0, 2, 2, 2, 2, 2, 2]
    rng = np.random.Generator(np.random.PCG64(14))
    flat["xmin"], flat["xmax"] = -0.2 - rng.random(12), 0.2 + rng.random(12)
    flat["umin"], flat["umax"] = -0.2 - rng.random(3), 0.2 + rng.random(3)
    if generic:
        monkeypatch.setenv("TREEQP_AMD_PATH", "generic")
    g = _clip_mirror(gpu, flat)
    assert (g.path == 0) if generic else (g.path in (1, 2)), g.path          # (1, 2: the uniform-tree kernels, i.e. embedded with phantom root states)
    assert g.sum_nx == 12
    _random_point_check(g, with_dense_blocks(flat), [0] * 7, 14, FIRST4)
    g.close()


# ---- corner semantics ----

def test_infinite_bounds_and_nan(gpu):
    d = K.random_problem(CLIP4, [0] * 4, 15)
    d["xmax"][:] = np.inf
    d["umin"][:] = -np.inf
    g = _clip_mirror(gpu, d)
    sol = K.random_point(d, 15)
    sol["mu_x"][:] = 0.0
    sol["mu_u"][:] = 0.0
    got = g.kkt_residual_at(sol, per_node=True)
    assert got["res"][K.BCOMPL] == 0.0 and np.isfinite(got["res"]).all() and np.isfinite(got["per_node"]).all()
    _check(got, K.residuals(d, sol, [0] * 4), "zero multipliers on infinite bounds")
    sol["mu_x"][4] = 0.5                           # node 1, entry 1, against xmax = inf
    got = g.kkt_residual_at(sol, per_node=True)
    assert np.isinf(got["res"][K.BCOMPL]) and got["node"][K.BCOMPL] == 1 and np.isinf(got["max"])
    _check(got, K.residuals(d, sol, [0] * 4), "a multiplier on an infinite bound")
    sol["mu_x"][4] = 0.0
    sol["x"][3] = np.nan                           # node 1, entry 0
    ref = K.residuals(d, sol, [0] * 4)
    assert np.isnan(ref["res"][[K.STAT, K.DYN, K.BFEAS]]).all() and list(ref["node"][:3]) == [1, 1, 1]
    got = g.kkt_residual_at(sol, per_node=True)
    assert np.array_equal(np.isnan(got["res"]), np.isnan(ref["res"])) and np.isnan(got["max"])
    assert np.array_equal(got["node"][np.isnan(ref["res"])], ref["node"][np.isnan(ref["res"])])
    _check(got, ref, "a NaN in x")
    g.close()


# ---- after real solves, one small tree per route ----

def _route(gpu, name):
    """(mirror, d in kkt_ref's form, kinds, solve options)"""
    if name == "persistent":
        p = P.linear_chain(2, 5, 5)
        flat = product_qp_from_lti(gpu, p).flat()
        g = _clip_mirror(gpu, flat, p.lambda0)
        assert g.path == 2
        return g, with_dense_blocks(flat), np.zeros(p.Nn, int), {}
    if name == "single_wg":
        d = LS.problem(LS.C, LS.case("g_persist_node_sizes-nz16")[1])
        g = _clip_mirror(gpu, d)
        assert g.path == 3
        return g, with_dense_blocks(d), np.zeros(len(d["nk"]), int), {}
    if name == "three_launch":
        d = LS.problem(LS.C, LS.case("widest_level-w97")[1])          # 106 nodes: too wide for one workgroup
        g = _clip_mirror(gpu, d)
        assert g.path == 0 and g.plan["w3"] and not g.plan["gpersist"]
        return g, with_dense_blocks(d), np.zeros(len(d["nk"]), int), {}
    c = GC.case("mixed")
    g = _dense_mirror(gpu, c["d"], c["kinds"], GC.full_start("mixed")[0])
    if name == "dense_single":
        g.set_dense_single_launch(True)
        assert g.path == 3
    else:
        assert name == "per_phase" and g.path == 0
    return g, c["d"], c["kinds"], FULL


ROUTES = ["persistent", "single_wg", "three_launch", "per_phase", "dense_single"]


def _solve_and_compare(g, d, kinds, what, **opts):
    r = g.solve(**opts)
    got = g.kkt_residual(per_node=True)
    sol = g.solution()
    _same(got, g.kkt_residual_at(sol, per_node=True), what + ": tqgpu_kkt_residual against _at on the exported arrays")
    _check(got, K.residuals(d, sol, kinds), what)
    _same(g.kkt_residual(per_node=True), got, what + ": a second call")
    return r, got


@pytest.mark.parametrize("name", ROUTES)
def test_after_a_solve_on_every_route(gpu, name):
    g, d, kinds, opts = _route(gpu, name)
    r, got = _solve_and_compare(g, d, kinds, name, **opts)
    assert r["status"] == 0 and got["max"] < 1e-6, (r, got)
    g.export_ahead(True)
    r2, got2 = _solve_and_compare(g, d, kinds, name + ", export ahead", **opts)
    assert r2["status"] == 0
    g.export_ahead(False)
    r3, got3 = _solve_and_compare(g, d, kinds, name + ", maxIter = 1", **dict(opts, maxIter=1))
    assert r3["status"] == 1
    g.close()


# ---- non-interference ----

def test_the_check_leaves_the_solver_alone(gpu):
    c = GC.case("mixed")
    d, kinds, lam0 = c["d"], c["kinds"], GC.full_start("mixed")[0]
    a, b = _dense_mirror(gpu, d, kinds, lam0), _dense_mirror(gpu, d, kinds, lam0)
    ra, sa = a.solve(**FULL), a.solution()
    rb = b.solve(**FULL)
    b.kkt_residual(per_node=True)
    sb = b.solution()
    key = lambda r: (r["status"], r["iter"], r["ls_total"])
    assert key(ra) == key(rb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    far = K.random_point(d, 16, scale=50.0)
    b.kkt_residual_at(far, per_node=True)
    b.kkt_residual()
    sb1 = b.solution()
    for k in sa:
        assert np.array_equal(sa[k], sb1[k]), f"{k} after tqgpu_kkt_residual_at"
    ra2, sa2, sta = a.solve(**FULL), a.solution(), a.stage_steps()
    rb2, sb2, stb = b.solve(**FULL), b.solution(), b.stage_steps()
    assert key(ra2) == key(rb2)
    for k in sa2:
        assert np.array_equal(sa2[k], sb2[k]), f"second solve: {k}"
    assert np.array_equal(sta["last"], stb["last"]) and np.array_equal(sta["total"], stb["total"])
    a.close(); b.close()


# ---- the export state: every route to tqgpu_get_solution gives the same bits ----

def _thesis(gpu):
    return _clip_mirror(gpu, P.thesis_example().as_dict()), {}


def _kinds_two_and_three(gpu):
    d, kinds = _mixed_problem()
    g = _dense_mirror(gpu, d, kinds)
    assert g.plan["gen"] and g.plan["box"]
    return g, FULL


def _x0_eliminated(gpu):
    p = P.linear_chain(2, 2, 2, nm=1, nu=1)
    g = _clip_mirror(gpu, product_qp_from_lti(gpu, p, eliminate_x0=True).flat())
    assert g.path == 2 and g.sum_nx == 12          # embedded with phantom root states, the single persistent launch
    return g, {}


@pytest.mark.parametrize("make", [_thesis, _kinds_two_and_three, _x0_eliminated], ids=lambda f: f.__name__.strip("_"))
def test_every_route_of_the_export_state_gives_the_same_solution(gpu, monkeypatch, make):
    """One solve with the same options on fresh mirrors, then tqgpu_get_solution behind: nothing, tqgpu_set_export_ahead (a no-op off
    the single persistent launch), tqgpu_kkt_residual, tqgpu_kkt_residual_batch of the mirror and a twin on the batched route and
    member by member, and a second tqgpu_get_solution.  No arithmetic differs between them: every comparison is exact."""
    def solved(ahead=False):
        g, opts = make(gpu)
        if ahead:
            g.export_ahead(True)
        r = g.solve(**opts)
        return g, (r["status"], r["iter"], r["ls_total"])

    sols, kkts, keys = {}, {}, {}
    g, keys["plain"] = solved()
    sols["plain"] = g.solution()
    sols["a second tqgpu_get_solution"] = g.solution()
    g.close()
    g, keys["export ahead"] = solved(ahead=True)
    sols["export ahead"] = g.solution()
    g.close()
    g, keys["kkt_residual first"] = solved()
    kkts["single"] = g.kkt_residual()
    sols["kkt_residual first"] = g.solution()
    g.close()
    for route, batched in (("batched", 2), ("members", 0)):
        if route == "members":
            monkeypatch.setenv("TREEQP_AMD_KKT_BATCH", "members")
        (g, keys[route]), (twin, keys[route + " twin"]) = solved(), solved()
        kkts[route], kkts[route + " twin"] = gpu.kkt_residual_batch([g, twin])
        assert gpu.kkt_batch_stats()["batched_members"] == batched, gpu.kkt_batch_stats()
        sols["kkt_residual_batch first, " + route] = g.solution()
        g.close(); twin.close()
    print(keys["plain"], kkts["single"])
    assert len(set(keys.values())) == 1, keys
    for what, s in sols.items():
        for k in ("x", "u", "lam", "mu_x", "mu_u", "dlam"):
            assert np.all(np.isfinite(s[k])), f"{what}: {k} is not finite"
            assert np.array_equal(s[k], sols["plain"][k]), f"{what}: {k} differs from a plain tqgpu_get_solution"
    for what, k in kkts.items():
        assert np.array_equal(k["res"], kkts["single"]["res"]) and np.array_equal(k["node"], kkts["single"]["node"]), (what, k, kkts["single"])


def test_a_certified_step_exports_the_same_solution(gpu):
    """the same behind a certified tqgpu_mpc_step, whose pack stays on the device until somebody asks: on the smallest tree of
    mpc_root_cases, against a twin that does not certify"""
    c = R.case("one_child")
    x0 = R.x0_sequence(c, 5, steps=1)[0]
    sols, kkts = {}, {}
    for what in ("plain", "certified", "certified, kkt_residual first", "certified, twice"):
        g = R.make(gpu, c, root_states=True)
        g.mpc_set_certify(what != "plain")
        g.mpc_step(x0, **c["opts"])
        if what != "plain":
            kkts[what] = g.mpc_certificate()
        if "kkt_residual" in what:
            kkts["tqgpu_kkt_residual"] = g.kkt_residual()
        if "twice" in what:
            g.solution()
        sols[what] = g.solution()
        g.close()
    for what, s in sols.items():
        for k in s:
            assert np.all(np.isfinite(s[k])) and np.array_equal(s[k], sols["plain"][k]), f"{what}: {k}"
    for what, k in kkts.items():
        assert np.array_equal(k["res"], kkts["certified"]["res"]) and np.array_equal(k["node"], kkts["certified"]["node"]), what


# ---- batch and refusals ----

def test_batch_equals_the_single_calls(gpu):
    ms = []
    for name in ("persistent", "single_wg", "per_phase"):
        g, _, _, opts = _route(gpu, name)
        assert g.solve(**opts)["status"] == 0
        ms.append(g)
    singles = [m.kkt_residual() for m in ms]
    batch = gpu.kkt_residual_batch(ms)
    for s, b in zip(singles, batch):
        _same(s, b, "batch member")
        assert s["max"] == b["max"]
    for m in ms:
        m.close()


def test_refusals(gpu):
    L = gpu.lib()
    res, node = (C.c_double * 6)(), (C.c_int * 6)()
    assert L.tqgpu_kkt_residual(None, res, node, None) == EINVAL
    assert L.tqgpu_kkt_residual_at(None, res, res, res, None, None, None, res, node, None) == EINVAL
    assert L.tqgpu_kkt_residual_batch(None, 1, res, node) == EINVAL
    d = K.random_problem(CLIP4, [0] * 4, 17)
    g = _clip_mirror(gpu, d)
    assert L.tqgpu_kkt_residual(g.h, res, node, None) == EINVAL and b"not solved" in L.tqgpu_last_error()
    arr = (C.c_void_p * 1)(g.h)
    assert L.tqgpu_kkt_residual_batch(arr, 1, res, node) == EINVAL
    assert g.kkt_residual_at(K.random_point(d, 17))["max"] > 0            # a point needs no solve
    assert L.tqgpu_kkt_residual_at(g.h, None, res, res, None, None, None, res, node, None) == EINVAL
    g.close()
    p = P.linear_chain(2, 6, 6)
    flat = product_qp_from_lti(gpu, p).flat()
    s = _clip_mirror(gpu, flat, p.lambda0).pshard_init(0, 2)
    assert L.tqgpu_kkt_residual(s.h, res, node, None) == EUNSUPPORTED
    s.close()

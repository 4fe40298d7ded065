"""The hot start of the stage solver for general constraints (stage_gen: tqgpu_set_gen_hot_start, tqgpu_get_stage_steps), on the
rows of gen_cases.py.

1. a mirror with the hot start (the default) and one without give the same whole solve bit for bit, from a clear start and again
   from the row's lambda0, for which the stored sets are stale;
2. after a solve that ended optimal the last sweep of the hot mirror cost one step per kind-3 node; the cold mirror's cost
   1 + (active members that are no equalities), exactly where the reference's run drops nothing; the hot mirror's total is smaller;
3. an MPC sequence that moves dmin / dmax between solves: hot and cold agree bit for bit after every solve, and an upload of
   ranges keeps the stored set (one step per node in the next sweep);
4. a start that is stale or useless falls back: a dependent stored set is redone cold, an infeasible stage QP still ends with
   status 4 and leaves the mirror usable, tqgpu_set_gen_hot_start and uploads of H or of C, D empty the stored sets;
5. the two entries of the C-ABI.

Every comparison between two mirrors is np.array_equal.  The expected step counts are those of gen_hot_ref.py / gen_ref.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gen_cases as GC
import gen_hot_ref as GH
import gen_ref as G

pytestmark = pytest.mark.gpu

OPTS = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)     # of test_repeated_fresh_and_batched_solves_are_bit_identical
ROWS = ["one_row", "row_and_bound", "more_rows_than_vars", "equality_row", "swap", "nc64", "nz64", "mixed", "x0_elim"]
KEYS = ("x", "u", "lam", "mu_x", "mu_u", "mu_d", "dlam")
EINVAL = -2
STAGE_QP_SOLVE_FAILED = 4


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _mirror(gpu, d, kinds, lam0=None, hot=None):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
    g.upload_mixed(d, kinds, lam0)
    if hot is not None:
        g.set_gen_hot_start(hot)
    return g


def _same(a, b, what="", keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), f"{what}{k}: differs by {np.max(np.abs(a[k] - b[k])):.3e}"


def _key(r):
    return r["status"], r["iter"], r["ls_total"]


@functools.lru_cache(maxsize=None)
def _start(rid):
    c = GC.case(rid)
    return GC.clear_start(c["d"], c["kinds"])


@functools.lru_cache(maxsize=None)
def _pair(gpu, rid):
    """the whole solve of row rid from its clear start on a hot and on a cold mirror, then from the row's lambda0 (computed once and
    shared by tests 1 and 2): per mirror the results, solutions and step counts after either solve"""
    c = GC.case(rid)
    out = {}
    for name, hot in (("hot", None), ("cold", False)):
        g = _mirror(gpu, c["d"], c["kinds"], _start(rid)[0], hot)
        try:
            r1 = g.solve(**OPTS); s1 = g.solution(); n1 = g.stage_steps()
            g.set_lambda(c["lam0"])
            r2 = g.solve(**OPTS); s2 = g.solution(); n2 = g.stage_steps()
        finally:
            g.close()
        out[name] = dict(r1=r1, s1=s1, n1=n1, r2=r2, s2=s2, n2=n2)
    return out


@pytest.mark.parametrize("rid", ROWS)
def test_hot_equals_cold_bit_for_bit(gpu, rid):
    p = _pair(gpu, rid)
    h, c = p["hot"], p["cold"]
    print(f"{rid}: first solve {_key(h['r1'])} steps hot {h['n1']['total'].sum()} cold {c['n1']['total'].sum()}; "
          f"from lambda0 {_key(h['r2'])} steps hot {h['n2']['total'].sum()} cold {c['n2']['total'].sum()}")
    assert _key(h["r1"]) == _key(c["r1"]) and h["r1"]["status"] == 0
    _same(h["s1"], c["s1"], "first solve: ")
    assert _key(h["r2"]) == _key(c["r2"])
    _same(h["s2"], c["s2"], "from lambda0 (stale stored sets): ")


def _active_members(d, kinds, sol):
    """per kind-3 node: the members of the solution's working set that are no equalities, from mu_d != 0 and from the entries of
    x, u on a bound with lb < ub"""
    nx, nu, nc = np.asarray(d["nx"], int), np.asarray(d["nu"], int), np.asarray(d["nc"], int)
    xo, uo, ro = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nu)]), np.concatenate([[0], np.cumsum(nc)])
    out = {}
    for k in np.flatnonzero((np.asarray(kinds) == 3) & (nc > 0)):
        n = 0
        for v, lo, hi in ((sol["x"][xo[k]:xo[k + 1]], d["xmin"][xo[k]:xo[k + 1]], d["xmax"][xo[k]:xo[k + 1]]),
                          (sol["u"][uo[k]:uo[k + 1]], d["umin"][uo[k]:uo[k + 1]], d["umax"][uo[k]:uo[k + 1]])):
            n += int(np.sum((lo < hi) & ((v == lo) | (v == hi))))
        rows = slice(ro[k], ro[k + 1])
        n += int(np.sum((sol["mu_d"][rows] != 0) & (d["dmin"][rows] < d["dmax"][rows])))
        out[int(k)] = n
    return out


@pytest.mark.parametrize("rid", ROWS)
def test_a_stored_optimal_set_costs_one_step(gpu, rid):
    c = GC.case(rid)
    p = _pair(gpu, rid)
    h, cold = p["hot"], p["cold"]
    assert h["r1"]["status"] == 0 and cold["r1"]["status"] == 0
    active = _active_members(c["d"], c["kinds"], h["s1"])
    ref = GH.cold_steps(c["d"], h["s1"]["lam"], c["kinds"])
    print(f"{rid}: last hot {h['n1']['last']} cold {cold['n1']['last']} total hot {h['n1']['total']} cold {cold['n1']['total']} "
          f"active {active} reference {ref}")
    assert set(active) == set(ref)
    for k, m in active.items():
        assert m == ref[k]["active"]
        assert h["n1"]["last"][k] == 1
        assert cold["n1"]["last"][k] >= 1 + m
        if ref[k]["drops"] == 0:
            assert cold["n1"]["last"][k] == 1 + m == ref[k]["steps"]
    others = [k for k in range(len(c["kinds"])) if k not in active]
    assert not np.any(h["n1"]["last"][others]) and not np.any(h["n1"]["total"][others])
    if sum(active.values()) >= 1:
        assert h["n1"]["total"].sum() < cold["n1"]["total"].sum()


@pytest.mark.parametrize("rid", ["one_row", "mixed"])
def test_mpc_sequence_moving_the_ranges(gpu, rid):
    """five solves with warm duals; between them only dmin / dmax are uploaded: the range of the root's cut row (row 0) alternates
    between its drawn value and the `loose` recipe.  The reference run of every solve keeps GAP and cond(S)."""
    c = GC.case(rid)
    kinds = c["kinds"]
    loose = GC.loose_case(rid)[0]
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    lam = GC.full_start(rid)[0]
    hot, cold = _mirror(gpu, d, kinds, lam), _mirror(gpu, d, kinds, lam, hot=False)
    try:
        for step in range(5):
            src = loose if step % 2 else c["d"]
            d["dmin"][0], d["dmax"][0] = src["dmin"][0], src["dmax"][0]
            it, _, err, lam_ref, guard = GC.reference_solve(d, kinds, lam0=lam)
            at_end = G.newton_step(d, lam_ref, kinds, reg=1e-8)
            assert err <= GC.FULL_TOL and guard["margin"] >= GC.GAP and at_end["condS"] <= GC.COND_MAX
            res = []
            for g in (hot, cold):
                g.set_constraints(None, None, None, d["dmin"], d["dmax"])
                g.set_lambda(lam)
                res.append((g.solve(**OPTS), g.solution(), g.stage_steps()))
            (rh, sh, nh), (rc, sc, ncold) = res
            print(f"{rid} step {step}: {_key(rh)} (reference iter {it}) mu_d {sh['mu_d']} steps hot {nh['total'].sum()} cold {ncold['total'].sum()}")
            assert _key(rh) == _key(rc) and rh["status"] == 0
            _same(sh, sc, f"step {step}: ")
            assert (sh["mu_d"][0] != 0) == (step % 2 == 0), "the root's cut row does not follow its range"
            lam = sh["lam"]
            # an upload of ranges keeps the stored set: after one (of the same ranges) a sweep at the solution costs the hot mirror one
            # step per kind-3 node, the cold mirror its cold count
            expect = GH.cold_steps(d, lam, kinds)
            for g in (hot, cold):
                g.set_constraints(None, None, None, d["dmin"], d["dmax"])
            (_, s1, n1), (_, s2, n2) = _one_sweep(hot, lam), _one_sweep(cold, lam)
            _same(s1, s2, f"step {step}, one sweep: ")
            for k, v in expect.items():
                assert n1["last"][k] == 1, "the upload of dmin / dmax emptied the stored set"
                assert n2["last"][k] >= 1 + v["active"] and (v["drops"] or n2["last"][k] == v["steps"])
    finally:
        hot.close(); cold.close()


def _one_sweep(g, lam):
    """a solve from duals that are already optimal: one stage sweep, no iteration"""
    g.set_lambda(lam)
    r = g.solve(**OPTS)
    assert (r["status"], r["iter"]) == (0, 0)
    return r, g.solution(), g.stage_steps()


def test_a_dependent_stored_set_is_redone_cold(gpu):
    """more_rows_than_vars with its loose row 1 a duplicate of the active row 0.  After a solve the hot mirror has stored row 0; then
    row 1 becomes an equality a little inside row 0's range: the start, stored set and equalities, holds two parallel rows with
    different ranges.  (Only ranges are uploaded: an upload of C, D would empty the stored set.)"""
    c = GC.case("more_rows_than_vars")
    kinds = c["kinds"]
    d = {k: np.array(v, copy=True) for k, v in c["d"].items()}
    cons = G.cons_of(d)
    Gk = np.array(cons[0][0], copy=True)
    Gk[1] = Gk[0]
    G.set_cons(d, [(Gk, np.asarray(cons[0][1], float), np.asarray(cons[0][2], float))] + cons[1:])
    lam = GC.clear_start(d, kinds)[0]
    hot, cold = _mirror(gpu, d, kinds, lam), _mirror(gpu, d, kinds, lam, hot=False)
    try:
        rh, sh = hot.solve(**OPTS), hot.solution()
        rc, sc = cold.solve(**OPTS), cold.solution()
        assert _key(rh) == _key(rc) and rh["status"] == 0
        _same(sh, sc, "before: ")
        assert sh["mu_d"][0] != 0 and sh["mu_d"][1] == 0
        upper = sh["mu_d"][0] > 0
        at = d["dmax"][0] if upper else d["dmin"][0]
        d["dmin"][1] = d["dmax"][1] = at - 0.05 if upper else at + 0.05
        for g in (hot, cold):
            g.set_constraints(None, None, None, d["dmin"], d["dmax"])
        assert cold.solve(**OPTS)["status"] == 0
        lam_new = cold.solution()["lam"]
        (r1, s1, n1), (r2, s2, n2) = _one_sweep(hot, lam_new), _one_sweep(cold, lam_new)
    finally:
        hot.close(); cold.close()
    print(f"one sweep on the dependent stored set: steps hot {n1['last']} cold {n2['last']} mu_d {s1['mu_d']}")
    assert _key(r1) == _key(r2)
    _same(s1, s2, "after: ", keys=KEYS[:-1])          # (dlam is the last iteration's: the cold mirror has made one solve more)
    assert s1["mu_d"][0] == 0 and s1["mu_d"][1] != 0
    assert n1["last"][0] == n2["last"][0] + 1, "the failed step of the stored set and the cold redo"


def test_infeasible_stage_qp_ends_with_status_4_with_the_hot_start(gpu):
    bad, good, kinds = GC.infeasible_pair()
    opts = dict(stationarityTolerance=GC.FULL_TOL)
    g = _mirror(gpu, good, kinds, hot=True)
    f = None
    try:
        r0 = g.solve(**opts)                       # (leaves a stored set behind)
        g.set_constraints(None, None, None, bad["dmin"], bad["dmax"])
        r = g.solve(**opts)
        assert r0["status"] == 0 and r["status"] == STAGE_QP_SOLVE_FAILED
        g.set_constraints(None, None, None, good["dmin"], good["dmax"])
        r2 = g.solve(**opts); s2 = g.solution()
        f = _mirror(gpu, good, kinds)
        rf = f.solve(**opts); sf = f.solution()
    finally:
        g.close()
        if f is not None:
            f.close()
    assert _key(r2) == _key(rf) and rf["status"] == 0
    _same(s2, sf)
    assert s2["x"][0] + s2["u"][0] >= 1.5 - 1e-12 and s2["mu_d"][0] < 0


@pytest.mark.parametrize("how", ["set_gen_hot_start", "upload of H", "upload of C, D"])
def test_resets_of_the_stored_set(gpu, how):
    c = GC.case("one_row")
    d, kinds = c["d"], c["kinds"]
    g = _mirror(gpu, d, kinds, _start("one_row")[0])
    try:
        assert g.solve(**OPTS)["status"] == 0
        lam = g.solution()["lam"]
        cold = GH.cold_steps(d, lam, kinds)
        _, s_hot, n_hot = _one_sweep(g, lam)
        if how == "set_gen_hot_start":
            g.set_gen_hot_start(True)
        elif how == "upload of H":
            g.upload_mixed(d, kinds, lam)
        else:
            g.set_constraints(None, d["C"], d["D"], None, None)
        _, s_reset, n_reset = _one_sweep(g, lam)
        _, _, n_again = _one_sweep(g, lam)
    finally:
        g.close()
    print(f"{how}: last {n_hot['last']} -> {n_reset['last']} -> {n_again['last']} (cold count {cold})")
    for k, v in cold.items():
        assert v["drops"] == 0
        assert n_hot["last"][k] == 1 and n_reset["last"][k] == v["steps"] == 1 + v["active"] and n_again["last"][k] == 1
    _same(s_hot, s_reset, keys=KEYS[:-1])


def test_abi(gpu):
    import ctypes as C
    L = gpu.lib()
    for name in ("tqgpu_set_gen_hot_start", "tqgpu_get_stage_steps"):
        assert hasattr(L, name), f"{name} is not exported"
    assert L.tqgpu_set_gen_hot_start(None, 1) == EINVAL
    assert L.tqgpu_get_stage_steps(None, None, None) == EINVAL
    # a tree without kind-3 nodes: the switch is a no-op, the counters are zero
    c = GC.case("one_row")
    d = c["d"]
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload_mixed(d, G._kinds2(c["kinds"]))
    try:
        assert L.tqgpu_set_gen_hot_start(g.h, 0) == 0 and L.tqgpu_set_gen_hot_start(g.h, 1) == 0
        last, total = np.full(len(d["nk"]), 7, np.int32), np.full(len(d["nk"]), 7, np.int64)
        assert L.tqgpu_get_stage_steps(g.h, last.ctypes.data_as(C.POINTER(C.c_int)), total.ctypes.data_as(C.POINTER(C.c_long))) == 0
        assert not last.any() and not total.any()
        assert g.solve()["status"] == 0
        n = g.stage_steps()
        assert not n["last"].any() and not n["total"].any()
        assert L.tqgpu_get_stage_steps(g.h, None, None) == 0
    finally:
        g.close()

"""The opt-in batch launch of trees with dense stage QPs (tqgpu_set_dense_batch_launch: g_persist_dense_batch, one launch for the
dense members of a tqgpu_solve_batch, one workgroup per tree), on the smallest trees of box_cases.py / gen_cases.py.

1.  without the option nothing moves: members on the launch-per-phase route, bit for bit their solo solves;
2.  with it a member IS its solo single launch (tqgpu_set_dense_single_launch on a fresh mirror): verdict, counts, launches and
    solution bit for bit -- the workgroup runs the same body on the same parameters -- and agrees with the default route to 1e-10;
3.  members with different LDS plans, stage waves and kinds in one launch, in two orders (the lead and the member that fixes the
    launch's LDS size change);
4.  one eligible member alone in its batch (next to a tree the plan refuses) is no group: both run the default route;
5.  a clipping group (g_persist_batch) and a dense group in one wave, their members interleaved;
6.  status 4 ends one member's workgroup only, and the mirrors stay usable;
7.  repeated batches are bit-identical, the hot start saves active-set steps, hot equals cold bit for bit;
8.  the option can be switched between the batch calls of the same mirrors;
9.  profiled solves and maxIter = 0 keep the members on the launch-per-phase route;
10. tqgpu_solve_batch_n: three steps are three times one call.

Tolerances.  Bit for bit wherever the two sides run the same body on the same data (a member against its solo single launch; a
member on the launch-per-phase route against its solo solve; hot against cold under the strict-complementarity guard of
gen_cases, where the stage result is a function of the final working set alone).  Between the single-workgroup body and the
default route: 1e-10, as test_gpu_dense_single.py (same bodies, another order of the workgroup's sums).  Every whole solve starts
from a clear_start (gen_cases), from which every Armijo and termination decision keeps its distance from rounding, so verdicts and
counts are compared exactly.  The solo solves a member is compared with are computed once per problem (`_solo`)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import box_cases as BC
import gen_cases as GC
import newton_ref as N
import test_gpu_dense_single as DS
from limit_shapes import leaf

pytestmark = pytest.mark.gpu

FULL = DS.FULL
BIT_LAST_SINGLE = DS.BIT_LAST_SINGLE
STAGE_QP_SOLVE_FAILED = 4
_mirror, _flags, _key, _same, _close = DS._mirror, DS._flags, DS._key, DS._same, DS._close


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


@functools.lru_cache(maxsize=None)
def _two_starts(rid):
    """the first two starting duals of gen_cases.clear_start's sequence whose reference solves of row rid qualify"""
    c = GC.case(rid)
    lam_opt = GC.reference_solve(c["d"], c["kinds"], tol=1e-10)[3]
    out = []
    for scale in (1.0, 0.3, 0.1, 0.03):
        for s in range(4):
            lam = lam_opt + N.seeded_duals(len(lam_opt), 50 + s, scale)
            try:
                ok = GC.qualifies(GC.reference_solve(c["d"], c["kinds"], lam0=lam))
            except ValueError:
                continue
            if ok:
                out.append(lam)
            if len(out) == 2:
                return out
    raise AssertionError(f"row {rid}: no two starting duals whose reference solves qualify")


@functools.lru_cache(maxsize=None)
def _spec(name):
    """(d, kinds, clear start) of the problems of this file"""
    if name in ("mixed_a", "mixed_b"):
        c = GC.case("mixed")
        return c["d"], c["kinds"], _two_starts("mixed")[name == "mixed_b"]
    if name == "kind1":                      # three dense unconstrained nodes
        c = DS._kind1_case()
        return c["d"], c["kinds"], GC.clear_start(c["d"], c["kinds"])[0]
    if name == "box_mixed":                  # kinds 2, 0, 2, 1 in the 7-node tree
        return DS._loose("mixed", True)
    if name == "nz64_box":                   # nz = 64 on the root: two stage waves, the largest window
        return DS._loose("nz64", True)
    c = GC.case(name)                        # one_row, swap, nc64: kind-3 roots
    return c["d"], c["kinds"], GC.full_start(name)[0]


_SOLO = {}


def _solo(gpu, name):
    """the solo solves a member is compared with, each on a fresh mirror, computed once: `single` (tqgpu_set_dense_single_launch)
    and `default` (the launch-per-phase route) -> (result, solution)"""
    if name not in _SOLO:
        d, kinds, start = _spec(name)
        out = {}
        for route in ("single", "default"):
            g = _mirror(gpu, d, kinds, start, single=route == "single")
            try:
                r = g.solve(**FULL)
                out[route] = (r, g.solution())
                assert bool(_flags(gpu, g) & BIT_LAST_SINGLE) == (route == "single")
            finally:
                g.close()
        _SOLO[name] = out
    return _SOLO[name]


def _member(gpu, name, batch=True, hot=None):
    d, kinds, start = _spec(name)
    g = _mirror(gpu, d, kinds, start, hot=hot)
    if batch:
        g.set_dense_batch_launch(True)
        assert g.dense_batch_launch() == (1, 1), f"{name} is not eligible for the batch launch"
    return g


def _is_the_solo_single_launch(gpu, name, r, sol, flags, fresh=True):
    """the assertions of case 2 for one member: r, sol, flags of the member after the batch"""
    (rs, ss), (rd, sd) = _solo(gpu, name)["single"], _solo(gpu, name)["default"]
    print(f"{name}: member {_key(r)} in {r['n_launches']} launches, solo single launch {_key(rs)} in {rs['n_launches']}, default route {_key(rd)} in {rd['n_launches']}")
    assert flags & BIT_LAST_SINGLE, f"{name}: the member did not go out in the launch"
    assert _key(r) == _key(rs)
    _same(sol, ss, f"{name} against its solo single launch: ")
    if fresh:
        assert r["n_launches"] == rs["n_launches"]
    assert _key(r) == _key(rd) and rd["status"] == 0
    _close(sol, sd, f"{name} against the default route")


def _run_batch(gpu, mirrors, **opts):
    res = gpu.solve_batch(mirrors, **(opts or FULL))
    return res, [m.solution() for m in mirrors], [_flags(gpu, m) for m in mirrors]


def _close_all(mirrors):
    for m in mirrors:
        m.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. default off
# ------------------------------------------------------------------------------------------------------------------------------

def test_default_off_members_stay_on_the_launch_per_phase_route(gpu):
    names = ["mixed_a", "mixed_b"]
    mem = [_member(gpu, n, batch=False) for n in names]
    try:
        assert all(m.dense_batch_launch() == (0, 1) for m in mem)
        res, sol, fl = _run_batch(gpu, mem)
    finally:
        _close_all(mem)
    for i, n in enumerate(names):
        rd, sd = _solo(gpu, n)["default"]
        assert not fl[i] & BIT_LAST_SINGLE
        assert _key(res[i]) == _key(rd) and res[i]["n_launches"] == rd["n_launches"]
        _same(sol[i], sd, f"{n}: ")


def test_the_option_alone_leaves_a_solo_solve_alone(gpu):
    g = _member(gpu, "mixed_a")
    try:
        r = g.solve(**FULL); s = g.solution(); f = _flags(gpu, g)
        assert g.dense_single_launch[:2] == (0, 1)
    finally:
        g.close()
    rd, sd = _solo(gpu, "mixed_a")["default"]
    assert not f & (BIT_LAST_SINGLE | DS.BIT_DENSE_SINGLE) and _key(r) == _key(rd) and r["n_launches"] == rd["n_launches"]
    _same(s, sd)


# ------------------------------------------------------------------------------------------------------------------------------
# 2, 3. a member is its solo single launch
# ------------------------------------------------------------------------------------------------------------------------------

def _check_batch(gpu, names):
    mem = [_member(gpu, n) for n in names]
    try:
        res, sol, fl = _run_batch(gpu, mem)
    finally:
        _close_all(mem)
    for i, n in enumerate(names):
        _is_the_solo_single_launch(gpu, n, res[i], sol[i], fl[i])


def test_the_batch_is_the_solo_single_launch(gpu):
    _check_batch(gpu, ["mixed_a", "mixed_b"])


HETEROGENEOUS = ["kind1", "box_mixed", "one_row", "nz64_box"]


@pytest.mark.parametrize("order", [HETEROGENEOUS, HETEROGENEOUS[::-1]], ids=["kind1_leads", "nz64_leads"])
def test_heterogeneous_members_in_one_launch(gpu, order):
    _check_batch(gpu, order)


def test_the_heterogeneous_members_differ_in_their_plans(gpu):
    mem = [_member(gpu, n) for n in HETEROGENEOUS]
    try:
        waves = [m.dense_single_launch[2] for m in mem]
    finally:
        _close_all(mem)
    print("stage waves:", dict(zip(HETEROGENEOUS, waves)))
    assert waves[:3] == [16, 16, 16] and 1 <= waves[3] < 16


# ------------------------------------------------------------------------------------------------------------------------------
# 4. a group of one is no group
# ------------------------------------------------------------------------------------------------------------------------------

def test_one_eligible_member_runs_alone(gpu):
    shape = (2, 1, [(2, 1, [leaf(2)] * 10)] * 10)          # a level of 100 nodes: plan_dense_single refuses it (test_gpu_dense_single.py, point 5)
    kinds = np.array([2] * 11 + [1] * 100, np.int32)
    d = BC.base_problem(shape, kinds, 5)
    BC.draw_bounds(d, kinds, np.zeros(2 * 110), BC.frac(0.25), 5)
    wide, wide_solo = _mirror(gpu, d, kinds), _mirror(gpu, d, kinds)
    m = _member(gpu, "mixed_a")
    try:
        wide.set_dense_batch_launch(True)
        assert wide.dense_batch_launch() == (1, 0)
        res, sol, fl = _run_batch(gpu, [m, wide])
        rw = wide_solo.solve(**FULL); sw = wide_solo.solution()
    finally:
        _close_all([wide, wide_solo, m])
    rd, sd = _solo(gpu, "mixed_a")["default"]
    assert not fl[0] & BIT_LAST_SINGLE and not fl[1] & BIT_LAST_SINGLE
    assert _key(res[0]) == _key(rd) and res[0]["n_launches"] == rd["n_launches"]
    _same(sol[0], sd, "the eligible member: ")
    assert _key(res[1]) == _key(rw) and res[1]["n_launches"] == rw["n_launches"]
    _same(sol[1], sw, "the wide tree: ")


# ------------------------------------------------------------------------------------------------------------------------------
# 5. two groups in one wave
# ------------------------------------------------------------------------------------------------------------------------------

def test_a_clipping_group_and_a_dense_group_in_one_wave(gpu):
    d = _spec("mixed_a")[0]
    starts = _two_starts("mixed")

    def clip(i):
        return gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d, starts[i])

    c = [clip(0), clip(1)]
    c_solo = [clip(0), clip(1)]
    dn = [_member(gpu, "mixed_a"), _member(gpu, "mixed_b")]
    mem = [c[0], dn[0], c[1], dn[1]]
    try:
        assert c[0].path == 3, "the clipping tree of this shape does not run the single-workgroup kernel"
        res, sol, fl = _run_batch(gpu, mem)
        rc = [g.solve(**FULL) for g in c_solo]
        sc = [g.solution() for g in c_solo]
    finally:
        _close_all(mem + c_solo)
    assert all(f & BIT_LAST_SINGLE for f in fl)
    for i, k in enumerate((0, 2)):
        assert _key(res[k]) == _key(rc[i]) and res[k]["n_launches"] == rc[i]["n_launches"] == 1
        _same(sol[k], sc[i], f"clipping member {i}: ")
    for n, k in (("mixed_a", 1), ("mixed_b", 3)):
        _is_the_solo_single_launch(gpu, n, res[k], sol[k], fl[k])


# ------------------------------------------------------------------------------------------------------------------------------
# 6. status 4 in one member
# ------------------------------------------------------------------------------------------------------------------------------

def test_status_4_ends_one_workgroup_only(gpu):
    bad, good, kinds = GC.infeasible_pair()
    b = _mirror(gpu, bad, kinds)
    b_phase = _mirror(gpu, bad, kinds)
    h = _member(gpu, "mixed_a")
    h_phase = _member(gpu, "mixed_a", batch=False)
    f = None
    try:
        b.set_dense_batch_launch(True)
        assert b.dense_batch_launch() == (1, 1)
        res, sol, fl = _run_batch(gpu, [b, h])
        res_p, _, fl_p = _run_batch(gpu, [b_phase, h_phase])          # what the launch-per-phase route reports for such a member
        assert res[0]["status"] == STAGE_QP_SOLVE_FAILED and fl[0] & BIT_LAST_SINGLE
        assert _key(res[0]) == _key(res_p[0]) and not fl_p[0] & BIT_LAST_SINGLE
        _is_the_solo_single_launch(gpu, "mixed_a", res[1], sol[1], fl[1])
        b.set_constraints(None, None, None, good["dmin"], good["dmax"])
        res2, sol2, fl2 = _run_batch(gpu, [b, h])
        f = _mirror(gpu, good, kinds, single=True)
        rf = f.solve(**FULL); sf = f.solution()
    finally:
        _close_all([b, b_phase, h, h_phase] + ([f] if f is not None else []))
    assert fl2[0] & BIT_LAST_SINGLE and fl2[1] & BIT_LAST_SINGLE
    assert _key(res2[0]) == _key(rf) and rf["status"] == 0
    _same(sol2[0], sf, "the repaired member: ")
    assert sol2[0]["x"][0] + sol2[0]["u"][0] >= 1.5 - 1e-12 and sol2[0]["mu_d"][0] < 0
    _is_the_solo_single_launch(gpu, "mixed_a", res2[1], sol2[1], fl2[1], fresh=False)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. hot start and repetition
# ------------------------------------------------------------------------------------------------------------------------------

HOT_ROWS = ["one_row", "swap", "nc64", "mixed_a"]


def test_hot_start_and_repetition(gpu):
    hot = [_member(gpu, n) for n in HOT_ROWS]
    cold = [_member(gpu, n, hot=False) for n in HOT_ROWS]
    try:
        r1, s1, f1 = _run_batch(gpu, hot)
        n1 = [int(m.stage_steps()["total"].sum()) for m in hot]
        r2, s2, f2 = _run_batch(gpu, hot)
        n2 = [int(m.stage_steps()["total"].sum()) for m in hot]
        rc, sc, fc = _run_batch(gpu, cold)
        nc = [int(m.stage_steps()["total"].sum()) for m in cold]
    finally:
        _close_all(hot + cold)
    print("active-set steps, first call / repeated / cold:", dict(zip(HOT_ROWS, zip(n1, n2, nc))))
    for i, n in enumerate(HOT_ROWS):
        assert f1[i] & BIT_LAST_SINGLE and f2[i] & BIT_LAST_SINGLE and fc[i] & BIT_LAST_SINGLE
        assert _key(r1[i]) == _key(r2[i]) == _key(rc[i]) and r1[i]["status"] == 0
        assert r1[i]["n_launches"] == 2 and r2[i]["n_launches"] == 1          # k_dense_init goes out with the first solve of a mirror only
        _same(s1[i], s2[i], f"{n} repeated: ")
        _same(s1[i], sc[i], f"{n} hot against cold: ")
        assert 0 < n2[i] <= n1[i] <= nc[i]


# ------------------------------------------------------------------------------------------------------------------------------
# 8. switching
# ------------------------------------------------------------------------------------------------------------------------------

def test_switching_between_batch_calls(gpu):
    names = ["mixed_a", "one_row"]
    mem = [_member(gpu, n) for n in names]
    try:
        r1, s1, f1 = _run_batch(gpu, mem)
        for m in mem:
            m.set_dense_batch_launch(False)
        r2, s2, f2 = _run_batch(gpu, mem)
        for m in mem:
            m.set_dense_batch_launch(True)
        r3, s3, f3 = _run_batch(gpu, mem)
    finally:
        _close_all(mem)
    for i, n in enumerate(names):
        rd, sd = _solo(gpu, n)["default"]
        assert f1[i] & BIT_LAST_SINGLE and not f2[i] & BIT_LAST_SINGLE and f3[i] & BIT_LAST_SINGLE
        assert _key(r1[i]) == _key(r2[i]) == _key(r3[i]) == _key(rd)
        _same(s2[i], sd, f"{n}, option off, against the default route: ")
        _same(s3[i], s1[i], f"{n}, on again: ")
        assert r3[i]["n_launches"] == 1 and r2[i]["n_launches"] > 1


# ------------------------------------------------------------------------------------------------------------------------------
# 9. what keeps a member off the launch
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [dict(FULL, profile=1), dict(FULL, maxIter=0)], ids=["profile", "maxIter0"])
def test_profiled_and_empty_solves_keep_the_launch_per_phase_route(gpu, opts):
    names = ["mixed_a", "mixed_b"]
    mem = [_member(gpu, n) for n in names]
    solo = [_member(gpu, n) for n in names]
    try:
        res, sol, fl = _run_batch(gpu, mem, **opts)
        rs = [g.solve(**opts) for g in solo]
        ss = [g.solution() for g in solo]
    finally:
        _close_all(mem + solo)
    for i, n in enumerate(names):
        assert not fl[i] & BIT_LAST_SINGLE
        assert _key(res[i]) == _key(rs[i]) and res[i]["n_launches"] == rs[i]["n_launches"]
        _same(sol[i], ss[i], f"{n}: ")


# ------------------------------------------------------------------------------------------------------------------------------
# 10. tqgpu_solve_batch_n
# ------------------------------------------------------------------------------------------------------------------------------

def test_three_steps_are_three_calls(gpu):
    names = ["mixed_a", "mixed_b", "one_row"]
    mem = [_member(gpu, n) for n in names]
    try:
        r1, s1, _ = _run_batch(gpu, mem)
        res, it, ls, la = gpu.solve_batch_n(mem, 3, **FULL)
        s3 = [m.solution() for m in mem]
        fl = [_flags(gpu, m) for m in mem]
    finally:
        _close_all(mem)
    assert all(f & BIT_LAST_SINGLE for f in fl)
    assert it == 3 * sum(r["iter"] for r in r1) and ls == 3 * sum(r["ls_total"] for r in r1)
    assert la == 3 * len(mem)          # one launch per member and step is counted: its workgroup of the batch launch
    for i, n in enumerate(names):
        assert _key(res[i]) == _key(r1[i])
        _same(s3[i], s1[i], f"{n}: ")

"""The cases of the solve-sequence pin (tests/golden/solve_sequence_pins.json), shared by the recorder (tools/make_solve_pins.py)
and the test (test_gpu_solve_sequence.py).

A case makes fresh mirrors under its creation-time switches and runs three consecutive solves on them -- cold, warm, warm -- under its
solve-time switches.  Per solve and mirror it records what the host side of a solve decides: verdict and counts (status, iter, ls_total,
ls_last), the launches it made (n_launches), the tqgpu_debug_plan flags, the route these flags and the options imply (`route_seen`, the
order of route_of in tdunes_device.hip), and the stage solver's step counts where the tree has general constraints.  Solutions are not part
of the record: the default reductions are not order-fixed, and the parity tests bound them.

The sharded cases (one tree over several ranks: virtual ranks, a one-rank RCCL communicator, the sharded persistent launch) record the
verdict, the counts and n_launches per mirror, and sha256 digests of the raw bytes of x, u and lam after the gather: these paths are
launches on ordered streams, and the sharded persistent solution is bit-identical to the single-device one.

Every problem comes from code the suite already has (limit_shapes, box_cases, gen_cases, treeqp_amd.problems)."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import hashlib
import os

import numpy as np

import box_cases as BC
import gen_cases as GC
import limit_shapes as S
from treeqp_amd import problems as P

SOLVES = 3
FULL = dict(stationarityTolerance=GC.FULL_TOL, regType=1, regValue=1e-8)          # the whole solves of the dense single-launch tests
REUSE = dict(checkLastActiveSet=2)
SWITCHES = ("TREEQP_AMD_PATH", "TREEQP_AMD_NO_W3_MIRROR", "TREEQP_AMD_NO_WIDE3", "TREEQP_AMD_NO_FUSE", "TREEQP_AMD_NO_FWD_MERGE", "TREEQP_AMD_FWD", "TREEQP_AMD_BWD")


@contextlib.contextmanager
def switches(env):
    """the environment with exactly the case's switches set (every other switch of SWITCHES unset), restored afterwards"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- problems: name -> function of capi that returns an uploaded mirror ----

def _shape(cid):
    def make(capi):
        kind, shape, _ = S.case(cid)
        d = S.problem(kind, shape)
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        return g.upload(d) if kind == S.C else g.upload_dense(d)
    return make


def _lti(build, far=None):
    """an LTI problem of treeqp_amd.problems; far = (seed, scale): random starting duals of that scale instead of the problem's own"""
    def make(capi):
        p = build()
        nk = p.nk()
        flat = capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()
        lam0 = p.lambda0
        if far:
            lam0 = far[1] * np.random.Generator(np.random.PCG64(far[0])).standard_normal(len(p.lambda0))
        return capi.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, lam0)
    return make


def _flat(build):
    def make(capi):
        f = build()
        return capi.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), f.lambda0)
    return make


def _dense(src, rid, single=False, batch=False):
    def make(capi):
        c = (BC if src == "box" else GC).case(rid)
        d = c["d"]
        g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
        if "nc" in d:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, c["kinds"], None)
        if single:
            g.set_dense_single_launch(True)
        if batch:
            g.set_dense_batch_launch(True)
        return g
    return make


@functools.lru_cache(maxsize=None)
def _backtracking():
    """the smallest problem of the three-launch mirror test of test_gpu_parity.py: 24 nodes, 11 iterations, 50 trials"""
    return P.random_shape_qp(5, 2, 6, (3, 9), (2, 5))


CHAIN7 = _lti(lambda: P.linear_chain(2, 2, 2, ubound=0.05))         # (nx, nu, md) = (8, 3, 2), the first line of FAST_TABLE and of BATCH_TABLE: 7 nodes, two iterations
CLIP_WG = _shape("g_persist_node_sizes-nz16")
DENSE_WG = _dense("box", "nz2", single=True)                        # the smallest tree of test_gpu_dense_single.py
BACKTRACK = _flat(_backtracking)
GENERIC = {"TREEQP_AMD_PATH": "generic"}
NO_MIRROR = {"TREEQP_AMD_NO_W3_MIRROR": "1"}
LEVELS = {"TREEQP_AMD_FWD": "levels", "TREEQP_AMD_BWD": "levels"}
PER_PHASE_ONLY = {**GENERIC, "TREEQP_AMD_NO_WIDE3": "1", "TREEQP_AMD_NO_FUSE": "1"}


def _case(cid, route, *makes, env=None, opts=None, batch=False, profile=0, logs=False, export_ahead=False, backtracks=False, shard=None):
    return dict(id=cid, route=route, makes=makes, env=env or {}, opts=opts or {}, batch=batch, profile=profile, logs=logs,
                export_ahead=export_ahead, backtracks=backtracks, shard=shard)


def _cases():
    out = [
        _case("persist", "PERSIST", CHAIN7),
        _case("persist-reuse", "PERSIST", CHAIN7, opts=REUSE),
        # the far start of test_multistage_tree_backtracking_and_options: the line search runs inside the launch (one launch per warm solve)
        _case("persist-multistage_far_start", "PERSIST", _lti(lambda: P.spring_mass(md=3, Nr=2, Nh=7), far=(11, 5.0))),
        _case("single_wg-clip", "SINGLE_WG", CLIP_WG),
        _case("single_wg-dense", "SINGLE_WG", DENSE_WG, opts=FULL),
        _case("batch-single_wg-clip", "SINGLE_WG", CLIP_WG, CLIP_WG, batch=True),
        _case("batch-single_wg-dense", "SINGLE_WG", _dense("box", "nz2", batch=True), _dense("box", "nz2", batch=True), opts=FULL, batch=True),
        _case("batch-persist", "PERSIST", CHAIN7, CHAIN7, batch=True),
        _case("tiered", "TIERED", _lti(lambda: P.linear_chain(2, 4, 4)), env={"TREEQP_AMD_PATH": "tiered"}),
    ]
    for name, cid in (("merged", "forward_chain-nx8"), ("fwd3", "forward_chain-nx9"), ("fwd3c", "forward_chain-bdim3"), ("one_parent", "k_sgp-nz32_everywhere")):
        # (the forward_chain shapes are small enough for the single-workgroup kernel; bdim3 would merge its forward sweep into the first trial)
        env = {} if name == "one_parent" else {**GENERIC, "TREEQP_AMD_NO_FWD_MERGE": "1"} if name == "fwd3c" else GENERIC
        out.append(_case(f"three_launch-{name}", "THREE_LAUNCH", _shape(cid), env=env))
        out.append(_case(f"three_launch-{name}-no_mirror", "THREE_LAUNCH", _shape(cid), env={**env, **NO_MIRROR}))
    out += [
        _case("three_launch-backtracking", "THREE_LAUNCH", BACKTRACK, env=GENERIC, backtracks=True),
        _case("three_launch-backtracking-no_mirror", "THREE_LAUNCH", BACKTRACK, env={**GENERIC, **NO_MIRROR}, backtracks=True),
        _case("fused_tails", "FUSED_TAILS", _shape("wide_class-d16"), env=GENERIC),
        _case("fused_tails-backtracking", "FUSED_TAILS", BACKTRACK, env={**GENERIC, "TREEQP_AMD_NO_WIDE3": "1"}, backtracks=True),
        _case("per_phase-n513", "PER_PHASE", _shape("FUSE_MAX-n513")),
        # (a small tree of dense unconstrained nodes keeps the fused tails; NO_FUSE takes it to k_stage and the reductions as launches)
        _case("fused_tails-dense", "FUSED_TAILS", _shape("dense_kind_1-nz64")),
        _case("per_phase-dense", "PER_PHASE", _shape("dense_kind_1-nz64"), env={"TREEQP_AMD_NO_FUSE": "1"}),
        _case("per_phase-box", "PER_PHASE", _dense("box", "nz1")),
        _case("per_phase-gen", "PER_PHASE", _dense("gen", "row_and_bound")),
        # one launch per tree level in both sweeps, with the fused tails and without them
        _case("fused_tails-levels", "FUSED_TAILS", _shape("wide_class-d16"), env={**GENERIC, **LEVELS}),
        _case("per_phase-levels", "PER_PHASE", _shape("wide_class-d16"), env={**GENERIC, **LEVELS, "TREEQP_AMD_NO_FUSE": "1"}),
        # (generic alone leaves this tree on the three-launch family: NO_WIDE3 and NO_FUSE take it to the launch-per-phase kernels)
        _case("per_phase-backtracking", "PER_PHASE", BACKTRACK, env=PER_PHASE_ONLY, backtracks=True),
    ]
    # option edges.  maxIter = 0 and profiling take a single-workgroup tree off its route (route_of): the record says where to
    for name, make, env, route in (("per_phase", BACKTRACK, PER_PHASE_ONLY, "PER_PHASE"), ("single_wg", CLIP_WG, {}, "SINGLE_WG")):
        logs = name == "per_phase"
        out += [
            _case(f"{name}-maxiter0", None, make, env=env, opts=dict(maxIter=0), logs=logs),
            _case(f"{name}-maxiter1", route, make, env=env, opts=dict(maxIter=1), logs=logs),
            _case(f"{name}-profile1", None, make, env=env, profile=1, logs=logs),
            _case(f"{name}-profile3", None, make, env=env, profile=3, logs=logs),
        ]
    out.append(_case("single_wg-export_ahead", "SINGLE_WG", CLIP_WG, export_ahead=True))
    # one tree over several ranks (shard = (transport, ranks)): the smallest trees test_gpu_parity.py and test_gpu_pshard.py shard
    chain127 = _lti(lambda: P.linear_chain(2, 6, 6))
    out += [
        _case("shard-virtual-n2", None, chain127, shard=("virtual", 2)),
        _case("shard-virtual-n8", None, chain127, shard=("virtual", 8)),
        # the random start of test_sharded_virtual_ranks_backtracking: further trials, so launch_trial_phase and exchange 2 in the trial loop
        _case("shard-virtual-n4-backtracking", None, _lti(lambda: P.linear_chain(2, 6, 6, ubound=0.1), far=(2, 10.0)), shard=("virtual", 4), backtracks=True),
        # solve and gather after a shard_init with a fresh id, the same after a second shard_init with another id, then once more warm
        _case("shard-rccl-one_rank", None, chain127, shard=("rccl", 1)),
        _case("pshard-local-n2", None, _lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05)), shard=("pshard", 2)),
    ]
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


# ---- running a case ----

def route_seen(g, plan, profile, max_iter):
    """the route of the last solve as the plan flags show it, in the order of route_of (g.path: the mirror's route under default options)"""
    path = g.path
    if plan["last_single_wg"]:
        return "SINGLE_WG"
    if path == 2 and profile == 0 and max_iter > 0:
        return "PERSIST"
    if path in (1, 2) and profile < 3:
        return "TIERED"          # (a multistage tree has no tiered kernels: no case takes one off the persistent route)
    if plan["w3"] and not plan["dense"] and profile < 3:
        return "THREE_LAUNCH"
    if plan["fuse"] and profile < 3 and not plan["box"] and not plan["gen"]:
        return "FUSED_TAILS"
    return "PER_PHASE"


def _flags(capi, g):
    f, a = C.c_uint(), C.c_int()
    g._chk(capi.lib().tqgpu_debug_plan(g.h, C.byref(f), C.byref(a)))
    return int(f.value), int(a.value)


def _phase_log(capi, g, cap=4096):
    cols = [np.full(cap, np.nan) for _ in range(4)]
    dp = C.POINTER(C.c_double)
    n = capi.lib().tqgpu_get_phase_log(g.h, *[c.ctypes.data_as(dp) for c in cols], cap)
    assert n >= 0, "tqgpu_get_phase_log failed"
    return [int(np.isfinite(c).sum()) for c in cols]


def _record(capi, c, g, r):
    flags, accs = _flags(capi, g)
    rec = {k: int(r[k]) for k in ("status", "iter", "ls_total", "ls_last", "n_launches")}
    rec.update(flags=flags, sgp_accs=accs, route=route_seen(g, g.plan, c["profile"], c["opts"].get("maxIter", 100)))
    if g.plan["gen"]:
        st = g.stage_steps()
        rec.update(stage_steps_last=[int(v) for v in st["last"]], stage_steps_total=[int(v) for v in st["total"]])
    if c["logs"]:
        rec.update(iteration_log_finite=int(np.isfinite(g.iteration_log()[1]).sum()), phase_log_finite=_phase_log(capi, g))
    if c["export_ahead"]:
        sol = g.solution()
        rec.update(solution_fetched=bool(all(np.all(np.isfinite(v)) for v in sol.values())))
    return rec


def _shard_record(g, r):
    sol = g.solution()
    rec = {k: int(r[k]) for k in ("status", "iter", "ls_total", "ls_last", "n_launches")}
    rec.update({f"sha256_{k}": hashlib.sha256(np.ascontiguousarray(sol[k]).tobytes()).hexdigest() for k in ("x", "u", "lam")})
    return rec


def _run_sharded(capi, c):
    kind, n = c["shard"]
    ms = [c["makes"][0](capi) for _ in range(n)]
    try:
        for r, g in enumerate(ms):
            if kind == "virtual":
                g.shard_init(r, n)
            elif kind == "pshard":
                g.pshard_init(r, n)
        out = []
        for i in range(SOLVES):
            if kind == "virtual":
                res = [capi.solve_virtual_ranks(ms, **c["opts"])] * n          # one verdict for all ranks; every rank ends with the solution
            elif kind == "pshard":
                res = capi.pshard_solve_local(ms, **c["opts"])
            else:
                if i < 2:
                    ms[0].shard_init(0, 1, capi.shard_unique_id())             # (the second communicator replaces the first)
                    assert ms[0].path == 1, (c["id"], "a sharded mirror runs the launch-per-tier kernels")
                res = [ms[0].solve(**c["opts"])]
                ms[0].shard_gather_solution()
            out.append([_shard_record(g, r) for g, r in zip(ms, res)])
    finally:
        for g in ms:
            g.close()
    return out


def run_case(capi, c):
    """-> [solve 0, solve 1, solve 2], each a list of one record per mirror"""
    if c["shard"]:
        with switches(c["env"]):
            return _run_sharded(capi, c)
    with switches(c["env"]):
        ms = [make(capi) for make in c["makes"]]
        try:
            for g in ms:
                if c["export_ahead"]:
                    g.export_ahead(True)
            out = []
            for _ in range(SOLVES):
                if c["batch"]:
                    res = capi.solve_batch(ms, profile=c["profile"], **c["opts"])
                else:
                    res = [ms[0].solve(profile=c["profile"], **c["opts"])]
                out.append([_record(capi, c, g, r) for g, r in zip(ms, res)])
        finally:
            for g in ms:
                g.close()
    return out


def check_case(c, rec):
    """what a record must show whatever the build: the case reaches the branch it is there for"""
    for solve in rec:
        for r in solve:
            if c["route"]:
                assert r["route"] == c["route"], (c["id"], r["route"])
            if c["backtracks"]:
                assert r["ls_total"] > r["iter"], (c["id"], "the problem no longer backtracks")
    if c["id"] == "single_wg-dense":
        assert [s[0]["n_launches"] for s in rec] == [2, 1, 1], c["id"]          # k_dense_init + the launch, then the launch
    if c["opts"].get("maxIter") == 0:
        assert all((r["status"], r["iter"]) == (1, 0) for s in rec for r in s), c["id"]

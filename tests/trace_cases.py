"""The rows of the result-field pin (test_trace_reference.py on the CPU, test_gpu_result_fields.py on the device): one row is one route
on its smallest problem.  Problems, creation-time switches and expected routes are those of solve_sequence_cases.py (its makers
upload without keeping the data; a row here keeps the data and the starting duals, which the reference needs, and uploads the
same way).

A row: id, family (the kernel family its termination norm and dual value come from), problem(capi) -> dict(d, lam0, kinds, dense,
gen), env (switches at creation), route, opts (beside termCondition and the tolerance), and how it is run: alone, as a batch of two
members with different starting duals, or sharded.  `clip`: every node clips, so the oracle models the row and the verdict is
compared with it."""
from __future__ import annotations

import functools

import numpy as np

import box_cases as BC
import gen_cases as GC
import limit_shapes as S
import solve_sequence_cases as SC
from treeqp_amd import problems as P

NORMS = (0, 1, 2)
TOL_OF = {0: 1e-12, 1: 1e-8, 2: 1e-8}          # sum of squares: the tolerance the parity campaign gives it (helpers.fuzz_case); the others: the default
K_CAP = 6
STRICT = {"TREEQP_AMD_STRICT_SUM": "1"}


def _far(n, far):
    return far[1] * np.random.Generator(np.random.PCG64(far[0])).standard_normal(n)


def _lti(build, far=None, elim=False):
    def problem(capi):
        p = build()
        nk = p.nk()
        qp = capi.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p)
        if elim:
            qp.eliminate_x0()
        d = qp.flat()
        lam0 = np.array(p.lambda0, dtype=float) if far is None else _far(len(p.lambda0), far)
        return dict(d=d, lam0=lam0, kinds=None, dense=False)
    return problem


def _shape(cid, far=None):
    def problem(capi):
        kind, shape, _ = S.case(cid)
        d = S.problem(kind, shape)
        n = int(np.asarray(d["nx"])[1:].sum())
        return dict(d=d, lam0=np.zeros(n) if far is None else _far(n, far), kinds=None, dense=kind != S.C)
    return problem


def _flat(build):
    def problem(capi):
        f = build()
        lam0 = np.zeros(int(np.asarray(f.nx)[1:].sum())) if f.lambda0 is None else np.array(f.lambda0, dtype=float)
        return dict(d=f.as_dict(), lam0=lam0, kinds=None, dense=False)
    return problem


def _mixed(src, rid, far):
    def problem(capi):
        c = (BC if src == "box" else GC).case(rid)
        n = len(c["lam0"])
        return dict(d=c["d"], lam0=_far(n, far), kinds=np.asarray(c["kinds"], np.int32), dense=True, gen=src == "gen")
    return problem


def upload(capi, pr, lam0=None, single=False, batch=False):
    """a mirror of the row's problem, made under the switches the caller has set"""
    d = pr["d"]
    lam0 = pr["lam0"] if lam0 is None else lam0
    g = capi.TqGpu(d["nk"], d["nx"], d["nu"])
    if pr["kinds"] is not None:
        if "nc" in d:
            g.set_constraints(d["nc"], d["C"], d["D"], d["dmin"], d["dmax"])
        g.upload_mixed(d, pr["kinds"], lam0)
        if single:
            g.set_dense_single_launch(True)
        if batch:
            g.set_dense_batch_launch(True)
    elif pr["dense"]:
        g.upload_dense(d, lam0)
    else:
        g.upload(d, lam0)
    return g


CHAIN7 = _lti(lambda: P.linear_chain(2, 2, 2, ubound=0.05))
BACKTRACK = _flat(SC._backtracking)
CHAIN127 = _lti(lambda: P.linear_chain(2, 6, 6))


def _row(rid, family, problem, route=None, env=None, opts=None, clip=True, backtracks=False, shard=None, batch=False, single=False, plan=None,
         quadratic=False):
    """quadratic: every node is dense and unconstrained, so the dual is one quadratic and Newton's method ends after ONE iteration from
    any start; such a row starts far away and is compared at the point that iteration reaches.  Every other row takes two or more."""
    return dict(id=rid, family=family, problem=problem, route=route, env=env or {}, opts=opts or {}, clip=clip, backtracks=backtracks,
                shard=shard, batch=batch, single=single, plan=plan or {}, quadratic=quadratic)


def _rows():
    G, NM = SC.GENERIC, SC.NO_MIRROR
    out = [
        _row("persist-chain7", "persist", CHAIN7, "PERSIST"),
        _row("persist-multistage_far_start", "persist", _lti(lambda: P.spring_mass(md=3, Nr=2, Nh=7), far=(11, 5.0)), "PERSIST", backtracks=True),
        # the smallest tree of test_x0_eliminated_trees_take_the_persistent_path (23 nodes)
        _row("persist-x0_eliminated", "persist", _lti(lambda: P.linear_chain(2, 2, 6), elim=True), "PERSIST"),
        _row("persist-reuse", "persist", CHAIN7, "PERSIST", opts=SC.REUSE),
        # (bounded inputs and a far start: 7 iterations, 102 trials; without bounds the dual is one quadratic and one iteration ends the solve)
        _row("tiered", "tiered", _lti(lambda: P.linear_chain(2, 4, 4, ubound=0.1), far=(2, 10.0)), "TIERED", env={"TREEQP_AMD_PATH": "tiered"}, backtracks=True),
        _row("single_wg-clip-small8", "single_wg", _shape("g_persist_node_sizes-nx8"), "SINGLE_WG", plan=dict(gp_small8=True)),
        _row("single_wg-clip", "single_wg", _shape("g_persist_node_sizes-nx9"), "SINGLE_WG", plan=dict(gp_small8=False)),
        _row("single_wg-dense", "single_wg", _mixed("box", "nz2", (3, 1.0)), "SINGLE_WG", opts=SC.FULL, clip=False, single=True),
    ]
    for name, cid in (("merged", "forward_chain-nx8"), ("fwd3", "forward_chain-nx9"), ("fwd3c", "forward_chain-bdim3"), ("one_parent", "k_sgp-nz32_everywhere")):
        env = {} if name == "one_parent" else {**G, "TREEQP_AMD_NO_FWD_MERGE": "1"} if name == "fwd3c" else G
        out.append(_row(f"three_launch-{name}", "three_launch", _shape(cid), "THREE_LAUNCH", env=env))
        out.append(_row(f"three_launch-{name}-no_mirror", "three_launch", _shape(cid), "THREE_LAUNCH", env={**env, **NM}))
    out += [
        _row("three_launch-backtracking", "three_launch", BACKTRACK, "THREE_LAUNCH", env=G, backtracks=True),
        _row("fused_tails-backtracking", "fused_tails", BACKTRACK, "FUSED_TAILS", env={**G, "TREEQP_AMD_NO_WIDE3": "1"}, backtracks=True),
        _row("per_phase-backtracking", "per_phase", BACKTRACK, "PER_PHASE", env=SC.PER_PHASE_ONLY, backtracks=True),
        _row("per_phase-n513", "per_phase", _shape("FUSE_MAX-n513"), "PER_PHASE"),
        _row("fused_tails-dense", "fused_tails", _shape("dense_kind_1-nz64", far=(7, 1.0)), "FUSED_TAILS", clip=False, quadratic=True),
        _row("per_phase-dense", "per_phase", _shape("dense_kind_1-nz64", far=(7, 1.0)), "PER_PHASE", env={"TREEQP_AMD_NO_FUSE": "1"}, clip=False, quadratic=True),
        _row("per_phase-box", "per_phase", _mixed("box", "nz1", (3, 1.0)), "PER_PHASE", opts=SC.FULL, clip=False),
        _row("per_phase-gen", "per_phase", _mixed("gen", "row_and_bound", (1, 0.3)), "PER_PHASE", opts=SC.FULL, clip=False),
        _row("per_phase-strict_sum", "per_phase", BACKTRACK, "PER_PHASE", env={**SC.PER_PHASE_ONLY, **STRICT}, backtracks=True),
        _row("single_wg-strict_sum", "single_wg", _shape("g_persist_node_sizes-nz16"), "SINGLE_WG", env=STRICT, backtracks=True),
        _row("shard-virtual-n2", "sharded", CHAIN127, shard=("virtual", 2)),
        _row("shard-virtual-n4-backtracking", "sharded", _lti(lambda: P.linear_chain(2, 6, 6, ubound=0.1), far=(2, 10.0)), shard=("virtual", 4), backtracks=True),
        _row("shard-rccl-one_rank", "sharded", CHAIN127, shard=("rccl", 1)),
        _row("pshard-local-n2", "pshard", _lti(lambda: P.linear_chain(2, 6, 6, ubound=0.05)), shard=("pshard", 2)),
        _row("pshard-local-n2-backtracking", "pshard", _lti(lambda: P.linear_chain(2, 6, 6, ubound=0.1), far=(2, 10.0)), shard=("pshard", 2), backtracks=True),
        _row("batch-persist", "persist", CHAIN7, "PERSIST", batch=True),
        _row("batch-single_wg-clip", "single_wg", _shape("g_persist_node_sizes-nz16"), "SINGLE_WG", batch=True),
        _row("batch-single_wg-dense", "single_wg", _mixed("box", "nz2", (3, 1.0)), "SINGLE_WG", opts=SC.FULL, clip=False, batch=True),
    ]
    return out


ROWS = _rows()
ROW_IDS = [r["id"] for r in ROWS]
CLIP_IDS = [r["id"] for r in ROWS if r["clip"]]
# one row per family for the exits that need no reference (NaN data; clipping rows only: the oracle confirms the verdict)
NAN_IDS = ["persist-chain7", "tiered", "single_wg-clip-small8", "three_launch-merged", "three_launch-one_parent", "fused_tails-backtracking",
           "per_phase-backtracking", "shard-virtual-n2", "pshard-local-n2"]


def row(rid):
    return ROWS[ROW_IDS.index(rid)]


@functools.lru_cache(maxsize=None)
def _problem(rid, capi):
    return row(rid)["problem"](capi)


def problem(rid, capi):
    """the row's data (built once per process)"""
    return _problem(rid, capi)


def member_duals(pr, i):
    """starting duals of member i of a batch row: member 0 the row's own, the others moved by a seeded offset of a tenth of their scale"""
    lam0 = pr["lam0"]
    if i == 0:
        return lam0
    scale = 0.1 * max(float(np.max(np.abs(lam0))) if len(lam0) else 0.0, 0.1)
    return lam0 + _far(len(lam0), (100 + i, scale))


def solve_opts(r, term, **more):
    return dict(r["opts"], termCondition=term, stationarityTolerance=TOL_OF[term], **more)


def ks_of(iter_full):
    """maxIter = 1 .. iter_full, capped at K_CAP values, the last always among them"""
    ks = list(range(1, iter_full + 1))
    return ks if len(ks) <= K_CAP else ks[:K_CAP - 1] + [iter_full]

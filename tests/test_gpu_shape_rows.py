"""Every line of the four instantiation tables (FAST_TABLE, MSTAGE_TABLE, BATCH_TABLE, SHARD_TABLE of tdunes_parts.hpp) on every kernel
variant the host can pick for it.  The host keeps the kernels of a line as a row of pointers (tdunes_rows.hpp), so a wrong entry is a
data error that only the affected shape shows on the affected variant: test_gpu_parity.py runs most lines on most variants, this file
runs all of them on all, on the smallest trees that take the route.  The variants are reached through the switches a user has:
TREEQP_AMD_PATH, TREEQP_AMD_NO_PERSIST_ONE, the option checkLastActiveSet, solve_batch, pshard_init / pshard_solve_local with
TREEQP_AMD_PSHARD_AGENT.  A line that is missing from the library fails its case: the shape would not take the route, which every case
asserts before it looks at numbers.  Every solve is held to the CPU oracle by the rule of test_gpu_parity.py: equal status, iterations
and trials, the solution within TOL, KKT residual below 1e-8; a batch member and a sharded solve to the single solve bit by bit.

The lists below restate the tables; a line added to a table gets its case by a line here.  The seeds were chosen on the CPU so that the
oracle ends every case with status 0."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from helpers import assert_solution_close
from test_gpu_parity import TOL
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

FAST_ROWS = [(8, 3, 2), (4, 1, 2), (4, 1, 3), (2, 1, 2), (8, 2, 2), (6, 2, 2), (4, 1, 4), (8, 1, 2), (8, 4, 2), (4, 2, 2), (4, 3, 2),
             (4, 2, 3), (4, 2, 4), (6, 1, 2), (6, 3, 2), (2, 1, 4), (2, 2, 2)]
MSTAGE_ROWS = [(8, 3, 2), (4, 1, 2), (4, 1, 3), (8, 2, 2), (4, 1, 4), (8, 1, 2), (8, 4, 2), (4, 2, 2), (4, 3, 2), (4, 2, 3), (4, 2, 4)]
BATCH_ROWS = [(8, 3, 2, False), (4, 1, 3, True), (8, 3, 2, True), (4, 1, 2, False), (4, 1, 2, True), (8, 2, 2, False)]
SHARD_ROWS = [(8, 3, 2), (4, 1, 2), (8, 2, 2), (6, 2, 2)]
NO_BATCH_ROW = (6, 3, 2, False)          # a FAST_TABLE line without a BATCH_TABLE line: its members are launched one by one

SEED = 29                                # random_uniform_tree_qp(SEED + i, ...) for member i of a case
TIER_HEIGHT = {2: 3, 3: 2, 4: 2}         # Uni<>::TH by md: a tree of more levels has two tiers or more


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mirror(gpu, f, **env):
    with _env(**env):                    # the creation-time switches are read by tqgpu_create
        return gpu.TqGpu(f.nk, f.nx, f.nu).upload(f.as_dict(), None)


def _hold_to_oracle(orc, f, ref, r, sol, what):
    assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), what
    assert_solution_close(sol, ref, TOL)
    assert orc.max_kkt(f.as_dict(), sol) < 1e-8, what


def _reference(orc, f):
    ref = orc.solve(f.as_dict())
    assert ref["status"] == 0, "the fixture's seed must give a problem the oracle solves"
    return ref


def _persistent_variants(gpu, orc, f, ref):
    """the three single-device builds of the persistent kernel: the one the mirror picks (one workgroup per CU where the launch fits),
    the plain one, the one that can keep factors"""
    g = _mirror(gpu, f)
    assert g.path == 2 and g.plan["persist"], "no row for this shape: it does not take the persistent route"
    _hold_to_oracle(orc, f, ref, g.solve(), g.solution(), "auto")
    for rep in range(2):                                   # the second solve finds the first one's factors and signatures
        _hold_to_oracle(orc, f, ref, g.solve(checkLastActiveSet=2), g.solution(), f"checkLastActiveSet=2, solve {rep}")
    g.close()
    g = _mirror(gpu, f, TREEQP_AMD_NO_PERSIST_ONE="1")
    assert g.path == 2 and g.plan["persist"] and not g.plan["persist_one"]
    _hold_to_oracle(orc, f, ref, g.solve(), g.solution(), "auto, two workgroups per CU")
    g.close()


def _tiered(gpu, orc, f, ref, tiers):
    g = _mirror(gpu, f, TREEQP_AMD_PATH="tiered")
    assert g.path == 1, "no row for this shape: it does not take the launch-per-tier route"
    assert g.geometry()["tiers"] == tiers
    _hold_to_oracle(orc, f, ref, g.solve(), g.solution(), f"tiered, {tiers} tier(s)")
    g.close()


@pytest.mark.parametrize("nx,nu,md", FAST_ROWS, ids=[f"{r[0]}_{r[1]}_{r[2]}" for r in FAST_ROWS])
def test_uniform_row_on_every_variant(gpu, orc, nx, nu, md):
    """1 + md + md^2 nodes, the smallest tree detect_fast accepts: f_top and f_stage (one tier), f_persist_one or f_persist<.., false>,
    f_persist<.., false>, f_persist<.., true>.  A tree of one tier launches neither f_back nor f_fwd, so the launch-per-tier route also
    runs the smallest tree of two tiers (TH + 1 levels)."""
    f = P.random_uniform_tree_qp(SEED, nx, nu, md, 2, 2)
    ref = _reference(orc, f)
    _persistent_variants(gpu, orc, f, ref)
    _tiered(gpu, orc, f, ref, 1)
    Nh = TIER_HEIGHT[md] + 1
    f2 = P.random_uniform_tree_qp(SEED, nx, nu, md, Nh, Nh)
    _tiered(gpu, orc, f2, _reference(orc, f2), 2)


@pytest.mark.parametrize("nx,nu,md", MSTAGE_ROWS, ids=[f"{r[0]}_{r[1]}_{r[2]}" for r in MSTAGE_ROWS])
def test_multistage_row_on_every_variant(gpu, orc, nx, nu, md):
    """one branching stage, then one chain level: f_mpersist_one or f_mpersist<.., false>, f_mpersist<.., false>, f_mpersist<.., true>"""
    f = P.random_uniform_tree_qp(SEED, nx, nu, md, 1, 2)
    _persistent_variants(gpu, orc, f, _reference(orc, f))


BATCH_CASES = BATCH_ROWS + [NO_BATCH_ROW]


@pytest.mark.parametrize("nx,nu,md,mstage", BATCH_CASES, ids=[f"{r[0]}_{r[1]}_{r[2]}_{'mstage' if r[3] else 'uniform'}" for r in BATCH_CASES])
def test_batch_row(gpu, orc, nx, nu, md, mstage):
    """Two trees of the row's shape in one solve_batch: f_persist_batch<nx, nu, md, mstage>, each member bit-identical to its own single
    solve.  Whether the two went out as ONE launch shows in their event pairs: a member of a batch launch records none (the launch is on
    the lead's stream), a member launched on its own does.  The shape without a row must still solve, member by member."""
    fs = [P.random_uniform_tree_qp(SEED + i, nx, nu, md, 1 if mstage else 2, 2) for i in range(2)]
    refs = [_reference(orc, f) for f in fs]
    singles = []
    for f, ref in zip(fs, refs):
        g = _mirror(gpu, f)
        assert g.path == 2
        r = g.solve()
        singles.append((r, g.solution()))
        _hold_to_oracle(orc, f, ref, r, singles[-1][1], "single solve")
        g.close()
    ms = [_mirror(gpu, f) for f in fs]
    assert [m.path for m in ms] == [2, 2]
    for _ in range(2):                                     # twice: the launch numbers advance together
        res = gpu.solve_batch(ms)
    one_launch = (nx, nu, md, mstage) != NO_BATCH_ROW
    for m, r, (r1, s1), f, ref in zip(ms, res, singles, fs, refs):
        sol = m.solution()
        assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"])
        for k in ("x", "u", "lam", "mu_x", "mu_u"):
            assert np.array_equal(sol[k], s1[k]), k
        _hold_to_oracle(orc, f, ref, r, sol, "batch member")
        assert bool(np.isnan(m.device_times(1)[0])) == one_launch, "a shape with a batch row goes out in the batch launch, any other on its own"
        m.close()


@pytest.mark.parametrize("nx,nu,md", SHARD_ROWS, ids=[f"{r[0]}_{r[1]}_{r[2]}" for r in SHARD_ROWS])
def test_shard_row_on_both_scopes(gpu, orc, nx, nu, md):
    """Two ranks of one process on one device, as test_gpu_pshard.py drives them, at the smallest tree the rank plan deals over two
    ranks (md = 2: four levels, a bottom tier of two subtrees): f_persist_sh<.., 1>, and f_persist_sh<.., 0> in the single-device
    combination (agent-scope polls of a plain slab)."""
    f = P.random_uniform_tree_qp(SEED, nx, nu, md, 4, 4)
    ref = _reference(orc, f)
    g = _mirror(gpu, f)
    assert g.path == 2
    r1, s1 = g.solve(), g.solution()
    _hold_to_oracle(orc, f, ref, r1, s1, "single device")
    g.close()
    for env in ({}, dict(TREEQP_AMD_PSHARD_AGENT="1", TREEQP_AMD_PSHARD_COARSE="1")):
        ms = [_mirror(gpu, f) for _ in range(2)]
        with _env(**env):                                  # read by tqgpu_pshard_init
            for r, m in enumerate(ms):
                m.pshard_init(r, 2)
        for rep in range(2):
            rs = gpu.pshard_solve_local(ms)
            for m, r in zip(ms, rs):
                sol = m.solution()
                assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"]), (env, rep)
                for k in ("x", "u", "lam", "mu_x", "mu_u"):
                    assert np.array_equal(sol[k], s1[k]), (env, k)
                _hold_to_oracle(orc, f, ref, r, sol, "sharded")
        for m in ms:
            m.close()

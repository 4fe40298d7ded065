"""The device path on both sides of every kernel-selection limit of tqgpu_create's steps (detect_shape, setup_per_phase, setup_wide3,
setup_persist, setup_single_wg in tdunes_device.hip): dual block size, node
sizes, children per parent, path length, level width, node count and LDS bytes.  Each shape of limit_shapes.ROWS is solved on the
default route and with TREEQP_AMD_PATH=generic; tqgpu_debug_plan shows that it took the variant on its side of the limit, and
verdict, iterations, line-search trials and solution equal the CPU oracle's."""
from __future__ import annotations

import numpy as np
import pytest

import limit_shapes as S
from helpers import assert_solution_close, rel_err
from newton_ref import starting_duals
from treeqp_amd import problems as P

pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = list(S.cases())
_STEPS = {}


def _step(cid, kind, d):
    """lambda0 and the dense Newton step there (newton_ref.py), once per case"""
    if cid not in _STEPS:
        _STEPS[cid] = starting_duals(d, kind == S.D)
    return _STEPS[cid]


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _mirror(gpu, kind, d):
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if kind == S.C:
        return g.upload(d)
    return g.upload_dense(d)


def _oracle(orc, kind, d):
    return orc.solve(d, orc.default_opts()) if kind == S.C else orc.solve_dense(d, orc.default_opts())


def _check_plan(plan, flags):
    wrong = {k: (plan[k], v) for k, v in flags.items() if plan[k] != v}
    assert not wrong, f"plan (got, expected): {wrong}"


@pytest.mark.parametrize("path", ["auto", "generic"])
@pytest.mark.parametrize("cid,kind,shape,flags", CASES, ids=[c[0] for c in CASES])
def test_both_sides_of_the_limit_match_the_oracle(gpu, orc, monkeypatch, cid, kind, shape, flags, path):
    """(a) the plan is on the intended side of the limit; (b) verdict, iterations and line-search trials equal the oracle's;
    (c) the solution is the oracle's to 1e-10; (d) with maxIter = 1 and no regularisation, the exported dlam (D.dlam: the step
    of the last iteration run, here the one at lambda0) is the step of newton_ref.py and the new lambda is lambda0 + tau dlam.

    The row "k_sgp, nx+nu" has one side only.  The gate `nx + nu <= 64 on every node` of k_sgp is decided only when the
    three-launch family is on, which needs the wide class (parents' nx + nu <= 32) and nx <= 32 on every node; leaves have no
    inputs, so every node has nx + nu <= 32 there and the gate always holds.  Its row solves the nearest reachable shape:
    nx + nu = 32 on the root and on the leaf."""
    if path == "generic":
        monkeypatch.setenv("TREEQP_AMD_PATH", "generic")
    else:
        monkeypatch.delenv("TREEQP_AMD_PATH", raising=False)
    d = S.problem(kind, shape)
    ref = _oracle(orc, kind, d)
    lam0, step = _step(cid, kind, d)
    opts1 = orc.default_opts(maxIter=1, regType=0)
    ref1 = orc.solve_dense(d, opts1, lam0) if kind == S.D else orc.solve(d, opts1, lam0)
    g = _mirror(gpu, kind, d)
    try:
        _check_plan(g.plan, flags)
        r = g.solve()
        sol = g.solution()
        g.set_lambda(lam0)
        r1 = g.solve(maxIter=1, regType=0)
        sol1 = g.solution()
    finally:
        g.close()
    assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
    assert_solution_close(sol, ref, TOL, keys=("x", "u", "lam") if kind == S.D else ("x", "u", "lam", "mu_x", "mu_u"))
    assert (r1["status"], r1["iter"], r1["ls_total"]) == (ref1["status"], ref1["iter"], ref1["ls_total"]) == (1, 1, r1["ls_total"])
    assert rel_err(sol1["dlam"], step["dlam"]) <= TOL
    tau = opts1.lineSearchBeta ** (r1["ls_total"] - 1)
    assert rel_err(sol1["lam"], lam0 + tau * step["dlam"]) <= TOL


def test_generic_factor_lds_limit(gpu, orc):
    """d = 141 is the largest root block the launch-per-phase kernels hold in 160 KiB of LDS: it solves.  d = 142 is refused
    at create with TQGPU_EUNSUPPORTED (k_forward's window, (d | 1) d + 2 d + nx + 2 doubles, is the first to overflow), and the
    next mirror still solves."""
    ok = S.problem(S.C, S.FACTOR_ACCEPTED)
    ref = _oracle(orc, S.C, ok)
    nk, nx, nu = S.flatten(S.FACTOR_REFUSED)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        gpu.TqGpu(nk, nx, nu)
    for _ in range(2):
        g = gpu.TqGpu(ok["nk"], ok["nx"], ok["nu"]).upload(ok)
        assert not g.plan["wide"]
        r = g.solve()
        sol = g.solution()
        g.close()
        assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
        assert_solution_close(sol, ref, TOL)


def test_dense_node_too_large_for_the_lds_factorization(gpu, orc):
    """A dense unconstrained node of nx + nu = 143 is refused by the upload with TQGPU_EUNSUPPORTED (k_dense_init holds H and
    its pivots in LDS); the mirror then takes a problem of nx + nu = 142 and solves it."""
    big = S.problem(S.D, S.DENSE_REFUSED)
    g = gpu.TqGpu(big["nk"], big["nx"], big["nu"])
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        g.upload_dense(big)
    g.close()
    ok = S.problem(S.D, S.case("dense_kind_1-nz142")[1])
    assert int(ok["nx"][0] + ok["nu"][0]) == 142
    ref = _oracle(orc, S.D, ok)
    g = _mirror(gpu, S.D, ok)
    r = g.solve()
    sol = g.solution()
    g.close()
    assert (r["status"], r["iter"]) == (ref["status"], ref["iter"])
    assert_solution_close(sol, ref, TOL, keys=("x", "u", "lam"))


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_f_persist_two_workgroups_per_cu(gpu, orc, monkeypatch, name):
    """TREEQP_AMD_NO_PERSIST_ONE=1 (what a 128-CU partition gets as well): the persistent launch takes f_persist, two
    workgroups to a CU, instead of f_persist_one."""
    monkeypatch.setenv("TREEQP_AMD_NO_PERSIST_ONE", "1")
    p = P.spring_mass() if name == "C1" else P.linear_chain(2, 9, 9)
    nk = p.nk()
    qp = gpu.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p)
    flat = qp.flat()
    ref = orc.solve(flat, lambda0=p.lambda0)
    g = gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)
    plan = g.plan
    assert g.path == 2 and plan["persist"] and not plan["persist_one"]
    r = g.solve()
    sol = g.solution()
    g.close()
    assert (r["status"], r["iter"], r["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"])
    assert_solution_close(sol, ref, TOL)


def test_batch_of_one_member_per_row_equals_single_solves(gpu):
    """One clipping shape of every row in one tqgpu_solve_batch: each member's verdict and counts equal those of its own single
    solve, and its solution is bit-identical where the batch runs the same kernels as the single solve (to 1e-12 where not).  A member that qualifies for g_persist runs it in the batch (g_persist_batch) whatever its LDS placement,
    alone only when its state is in LDS: the shapes with only the index tables in LDS, or nothing in LDS, run g_persist only here."""
    picked, seen = [], set()
    for cid, kind, shape, flags in CASES:
        row = cid.split("-")[0]
        if kind == S.C and row not in seen:
            seen.add(row)
            picked.append(cid)
    picked += ["g_persist_LDS-tables_in_lds", "g_persist_LDS-tables_in_lds_last", "g_persist_LDS-nothing_in_lds"]
    probs = [S.problem(S.C, S.case(c)[1]) for c in picked]
    ms = [gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d) for d in probs]
    singles, alone = [], []
    for c, m in zip(picked, ms):
        r = m.solve()
        plan = m.plan
        assert plan["last_single_wg"] == (plan["gpersist"] and plan["gp_state_lds"]), c
        singles.append((r, m.solution()))
        alone.append(plan["last_single_wg"])
    res = gpu.solve_batch(ms)
    for c, m, r, (r1, s1), a in zip(picked, ms, res, singles, alone):
        assert m.plan["last_single_wg"] == m.plan["gpersist"], c
        assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"]), c
        sol = m.solution()
        if m.plan["last_single_wg"] == a:
            for k in ("x", "u", "lam", "mu_x", "mu_u"):
                assert np.array_equal(sol[k], s1[k]), (c, k)
        else:
            # another kernel family than alone (g_persist instead of the launch-per-phase kernels): the same decisions, the
            # sums of blocks of d = 31 in another order
            assert_solution_close(sol, s1, 1e-12)
    for c in picked[-3:]:
        assert ms[picked.index(c)].plan["last_single_wg"], c
    for m in ms:
        m.close()


def test_single_workgroup_member_alone_in_its_wave_runs_its_own_route(gpu):
    """The route a batch member runs: a tree that takes g_persist only as a member of a batch launch (its state does not fit LDS) runs
    it when its wave holds at least two single-workgroup trees, and the route of its own single solve when it is the only one --
    here among members of other classes (persistent with a batch kernel, three-launch, fused tails), none of which takes
    g_persist.  Verdict and counts of every member equal its own single solve; the solution of the LDS-too-large trees to 1e-12
    (the bound of test_batch_of_one_member_per_row_equals_single_solves for members that may run another kernel family)."""
    def shaped(cid):
        d = S.problem(S.C, S.case(cid)[1])
        return gpu.TqGpu(d["nk"], d["nx"], d["nu"]).upload(d)

    def persistent():
        p = P.spring_mass()
        nk = p.nk()
        flat = gpu.TreeQp(np.full(p.Nn, p.nx), np.where(nk > 0, p.nu, 0), nk).fill_lti(p).flat()
        return gpu.TqGpu(flat["nk"], flat["nx"], flat["nu"]).upload(flat, p.lambda0)

    for n_big in (1, 2):
        # (widest_level-w97: three-launch and past g_persist's widest level; the small wide trees qualify for g_persist)
        ms = [persistent(), shaped("widest_level-w97"), shaped("g_persist_LDS-tables_in_lds"), shaped("g_persist_LDS-nothing_in_lds"),
              shaped("FUSE_MAX-n512"), persistent()]
        if n_big == 1:
            ms.pop(3).close()
        big = range(2, 2 + n_big)
        singles = []
        for i, m in enumerate(ms):
            r = m.solve()
            plan = m.plan
            assert not plan["last_single_wg"] and (i not in big or (plan["gpersist"] and not plan["gp_state_lds"])), (i, plan)
            singles.append((r, m.solution()))
        res = gpu.solve_batch(ms)
        for i, (m, r, (r1, s1)) in enumerate(zip(ms, res, singles)):
            assert (r["status"], r["iter"], r["ls_total"]) == (r1["status"], r1["iter"], r1["ls_total"]), (n_big, i)
            assert m.plan["last_single_wg"] == (i in big and n_big == 2), (n_big, i)          # (no other member takes g_persist)
            if i in big:
                assert_solution_close(m.solution(), s1, 1e-12)
        for m in ms:
            m.close()

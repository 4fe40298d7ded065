"""tqgpu_result.last_error_norm, last_fval and the trial log of every route, pinned to trace_ref.py (numpy, longdouble) on the rows of
trace_cases.py, under the three termination norms.

Per row and norm, on fresh mirrors made under the row's switches:
a. clipping rows: status, iter, ls_total, ls_last and the trial log equal the oracle's; every row: ls_last and ls_total are what the
   log says;
b. on every exit with status 0 or 1 and iter >= 1, last_fval is the dual function at the RETURNED lam (the last trial's point, on
   both exits) within trace_ref.bound_fval;
c. on an OPTIMAL exit last_error_norm is the norm of the residual of the RETURNED x, u within trace_ref.bound_err, finite and below
   the tolerance; on a MAXIMUM_ITERATIONS exit with maxIter = k it is the norm at lam_prev = lam - beta^(ls_last - 1) dlam, the point
   the last iteration started from, within bound_err alone: that point is known exactly, as the lam the mirror returns with
   maxIter = k - 1 (lambda0 for k = 1), and the returned lam, dlam and ls_last must rebuild it to the rounding of the line search.  k runs
   over 1 .. iter of the full solve (trace_cases.ks_of), every solve from the same starting duals: the device's whole trace;
d. maxIter = 0 directly afterwards: status 1, iter 0 and every other field 0; then a second solve from other starting duals:
   the fields are that solve's (b and c again).
NaN in q (one row per family): status 2, last_error_norm NaN under every norm.

No tolerance here is a constant: every one is a bound of trace_ref.py, the same the oracle is held to in test_trace_reference.py."""
from __future__ import annotations

import numpy as np
import pytest

import gen_ref as G
import solve_sequence_cases as SC
import trace_cases as TC
import trace_ref as R

pytestmark = pytest.mark.gpu
RATIOS = {}         # (family, what, norm) -> largest |device - reference| / bound


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


class Mirrors:
    """the mirrors of a row, made under its switches: one, the two members of a batch, or the ranks of a sharded solve"""

    def __init__(self, gpu, monkeypatch, r, pr):
        self.gpu, self.r, self.pr = gpu, r, pr
        self.kind = r["shard"][0] if r["shard"] else "batch" if r["batch"] else "alone"
        n = r["shard"][1] if r["shard"] else 2 if r["batch"] else 1
        self.starts = [TC.member_duals(pr, i) for i in range(n)] if r["batch"] else [pr["lam0"]]
        for k, v in r["env"].items():
            if k not in SC.SWITCHES:
                monkeypatch.setenv(k, v)
        with SC.switches({k: v for k, v in r["env"].items() if k in SC.SWITCHES}):
            self.ms = [TC.upload(gpu, pr, self.starts[i] if r["batch"] else None, single=r["single"], batch=r["batch"]) for i in range(n)]
        for k in r["env"]:
            if k not in SC.SWITCHES:
                monkeypatch.delenv(k)
        for i, g in enumerate(self.ms):
            if self.kind == "virtual":
                g.shard_init(i, n)
            elif self.kind == "pshard":
                g.pshard_init(i, n)
            elif self.kind == "rccl":
                g.shard_init(0, 1, gpu.shard_unique_id())

    def set_starts(self, starts):
        self.starts = starts
        for i, g in enumerate(self.ms):
            g.set_lambda(starts[i if self.kind == "batch" else 0])

    def solve(self, **opts):
        """-> [(result, mirror, starting duals)] per member (a sharded solve: rank 0 with the gathered solution)"""
        if self.kind == "alone":
            res = [self.ms[0].solve(**opts)]
        elif self.kind == "batch":
            res = self.gpu.solve_batch(self.ms, **opts)
        elif self.kind == "virtual":
            res = [self.gpu.solve_virtual_ranks(self.ms, **opts)]
        elif self.kind == "pshard":
            all_ = self.gpu.pshard_solve_local(self.ms, **opts)
            for q in all_[1:]:          # every rank reports the one verdict
                assert all(q[k] == all_[0][k] or (np.isnan(q[k]) and np.isnan(all_[0][k])) for k in ("status", "iter", "ls_total", "ls_last", "last_error_norm", "last_fval")), (all_[0], q)
            res = all_[:1]
        else:
            res = [self.ms[0].solve(**opts)]
            self.ms[0].shard_gather_solution()
        return [(q, g, lam0) for q, g, lam0 in zip(res, self.ms, self.starts)]

    def close(self):
        for g in self.ms:
            g.close()


def _note(r, what, term, err, bound):
    key = (r["family"], what, term)
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bound)
    print(f"    {r['id']} norm {term} {what}: |device - reference| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")


def _stages(pr, lam):
    return G.stage_solutions(pr["d"], lam, pr["kinds"]) if pr.get("gen") else None


def _check_log(q, g):
    log = g.iteration_log()[0]
    n = q["iter"]
    if n >= 1:
        assert q["ls_last"] == log[n - 1], (q, log[:n])
    assert q["ls_total"] == int(np.sum(log[:n])), (q, log[:n])
    return log[:n].tolist()


def _check_fval(r, pr, term, q, sol):
    fv, Tf = R.dual_value_with_scale(pr["d"], sol["lam"], pr["kinds"], pr["dense"], _stages(pr, sol["lam"]))
    bnd = R.bound_fval(pr["d"], Tf)
    err = abs(q["last_fval"] - float(fv))
    _note(r, "fval", term, err, bnd)
    assert err <= bnd, (r["id"], term, q, float(fv), bnd)


def _check_optimal(r, pr, term, q, sol):
    val, T = R.error_norm(pr["d"], sol["x"], sol["u"], term)
    bnd = R.bound_err(pr["d"], term, T)
    err = abs(q["last_error_norm"] - float(val))
    _note(r, "err_optimal", term, err, bnd)
    assert np.isfinite(q["last_error_norm"]) and q["last_error_norm"] < TC.TOL_OF[term], (r["id"], term, q)
    assert err <= bnd, (r["id"], term, q, float(val), bnd)


def _check_maxiter(gpu, r, pr, term, q, sol, k, lam_prev):
    """lam_prev: the point iteration k - 1 started from, exactly: lambda0, or the lam the same mirror returned with maxIter = k - 1
    (solves from the same starting duals repeat bit for bit).  Known exactly, it needs no Lipschitz term: the bound is bound_err
    alone.  The returned lam, dlam and ls_last must rebuild that point: the line search adds (tau - tau_prev) dlam per trial
    (dual_Newton_tree.c:958-966), each trial rounding the difference, the product and the sum once, u (|lam_prev| + 3 |dlam|)
    per entry at the most (tau <= 1), so || lam - tau dlam - lam_prev || <= trials eps (||lam_prev|| + 2 ||dlam||); tau is
    beta^(trials - 1) of the trials made, min(ls_last, lineSearchMaxIter): ls_last is lineSearchMaxIter + 1 when none was accepted."""
    d = pr["d"]
    o = gpu._default_opts(**r["opts"])
    trials = min(q["ls_last"], o.lineSearchMaxIter)
    tau = 1.0
    for _ in range(trials - 1):
        tau *= o.lineSearchBeta
    rebuilt = np.asarray(sol["lam"], R.LD) - R.LD(tau) * np.asarray(sol["dlam"], R.LD)
    off = float(np.linalg.norm((rebuilt - np.asarray(lam_prev, R.LD)).astype(np.float64)))
    room = trials * R.EPS * (float(np.linalg.norm(lam_prev)) + 2.0 * float(np.linalg.norm(sol["dlam"])))
    assert off <= room, (r["id"], term, k, "lam, dlam and ls_last do not rebuild the point the iteration started from", off, room)
    val, T, _ = R.error_norm_at(d, lam_prev, term, pr["kinds"], pr["dense"], _stages(pr, lam_prev))
    bnd = R.bound_err(d, term, T, at=True, kinds=pr["kinds"], dense=pr["dense"])
    err = abs(q["last_error_norm"] - float(val))
    _note(r, "err_maxiter", term, err, bnd)
    assert err <= bnd, (r["id"], term, k, q, float(val), bnd)


def _check_exit(gpu, r, pr, term, q, g, k=None, lam_prev=None):
    sol = g.solution()
    log = _check_log(q, g)
    if k is None:
        assert q["status"] == 0 and q["iter"] >= 1, (r["id"], term, q)
        _check_optimal(r, pr, term, q, sol)
    else:
        assert (q["status"], q["iter"]) == (1, k), (r["id"], term, k, q)
        _check_maxiter(gpu, r, pr, term, q, sol, k, lam_prev)
    _check_fval(r, pr, term, q, sol)
    return log


@pytest.mark.parametrize("term", TC.NORMS)
@pytest.mark.parametrize("rid", TC.ROW_IDS)
def test_result_fields_are_the_reference(gpu, orc, monkeypatch, rid, term):
    r = TC.row(rid)
    pr = TC.problem(rid, gpu)
    opts = TC.solve_opts(r, term)
    M = Mirrors(gpu, monkeypatch, r, pr)
    try:
        for name, want in r["plan"].items():
            assert M.ms[0].plan[name] == want, (rid, name)
        full = M.solve(**opts)
        n_full = []
        for q, g, lam0 in full:
            if r["route"]:
                assert SC.route_seen(g, g.plan, 0, 100) == r["route"], rid
            log = _check_exit(gpu, r, pr, term, q, g)
            if r["backtracks"]:
                assert q["ls_total"] > q["iter"], (rid, "the problem no longer backtracks")
            if r["quadratic"]:          # one iteration from any start: the comparisons above were made at the point it reached
                assert q["iter"] == 1 and not np.array_equal(g.solution()["lam"], lam0), (rid, q)
            elif lam0 is pr["lam0"]:
                assert q["iter"] >= 2, (rid, "the row must reach a point that is not lambda0 before it converges", q)
            if r["clip"]:
                oo = {k: v for k, v in opts.items() if k != "checkLastActiveSet" or v != 2}
                ref = orc.solve(pr["d"], orc.default_opts(**oo), lambda0=lam0)
                assert (q["status"], q["iter"], q["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), (rid, term, q, ref["iter"], ref["ls_total"])
                assert log == ref["trace_ls"][:ref["iter"]].tolist() and q["ls_last"] == ref["trace_ls"][ref["iter"] - 1], (rid, term, log)
            n_full.append(q["iter"])
        # the device's trace: one solve per iteration count, each from the same starting duals; the point an iteration starts from is
        # the lam of the solve with one iteration fewer (fetched by a solve of its own where the cap left that count out)
        ks = TC.ks_of(max(n_full))
        prev = {0: [lam0 for _, _, lam0 in full]}
        for k in ks:
            if k - 1 not in prev:
                prev[k - 1] = [g.solution()["lam"] for _, g, _ in M.solve(**dict(opts, maxIter=k - 1))]
            res = M.solve(**dict(opts, maxIter=k))
            prev[k] = [g.solution()["lam"] for _, g, _ in res]
            for i, ((q, g, lam0), n) in enumerate(zip(res, n_full)):
                if k <= n:
                    _check_exit(gpu, r, pr, term, q, g, k, prev[k - 1][i])
        # nothing to iterate, directly after a solve that left other values behind
        if M.kind == "pshard":
            with pytest.raises(RuntimeError):          # tqgpu_pshard_begin refuses maxIter <= 0 before anything is launched
                M.solve(**dict(opts, maxIter=0))
        else:
            for q, g, _ in M.solve(**dict(opts, maxIter=0)):
                assert (q["status"], q["iter"], q["ls_total"], q["ls_last"]) == (1, 0, 0, 0), (rid, q)
                assert q["last_error_norm"] == 0.0 and q["last_fval"] == 0.0, (rid, q)
        # a second solve on the same mirrors from other starting duals: its own fields
        M.set_starts([TC.member_duals(pr, 7 + i) for i in range(len(M.starts))])
        for q, g, lam0 in M.solve(**opts):
            if q["status"] == 0 and q["iter"] >= 1:
                _check_exit(gpu, r, pr, term, q, g)
            else:
                assert q["status"] == 0 and q["iter"] == 0, (rid, q)
                _check_optimal(r, pr, term, q, g.solution())
    finally:
        M.close()


@pytest.mark.parametrize("term", TC.NORMS)
@pytest.mark.parametrize("rid", TC.NAN_IDS)
def test_not_descent_exit_reports_a_nan_norm(gpu, orc, monkeypatch, rid, term):
    """the NaN-in-q case of test_nan_data_ends_with_not_descent_direction: the residual norm is NaN under every norm (the maximum keeps
    a NaN, as the reference's MAX(error, NaN) does), `error < tol` is false and the line search ends the solve with status 2"""
    r = TC.row(rid)
    pr = dict(TC.problem(rid, gpu))
    pr["d"] = {k: np.array(v, copy=True) for k, v in pr["d"].items()}
    pr["d"]["q"][len(pr["d"]["q"]) // 2] = np.nan
    opts = TC.solve_opts(r, term)
    assert orc.solve(pr["d"], orc.default_opts(**opts), lambda0=pr["lam0"])["status"] == 2
    M = Mirrors(gpu, monkeypatch, r, pr)
    try:
        for q, g, _ in M.solve(**opts):
            assert q["status"] == 2 and q["iter"] == 0, (rid, term, q)
            assert np.isnan(q["last_error_norm"]), (rid, term, q)
    finally:
        M.close()


def test_largest_ratios_are_printed():
    """(runs last in the module: the figures of a whole run, per kernel family, field and norm)"""
    for (family, what, term), v in sorted(RATIOS.items()):
        print(f"{family:13s} {what:12s} norm {term}: largest |device - reference| / bound = {v:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())

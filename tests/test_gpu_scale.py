"""Every device route held to power-of-two scale equivariance (scale_cases.py has the transform, test_scale_reference.py shows that the
transform is right and that the CPU oracle is equivariant BIT FOR BIT on the clipping cases used here).

A tree QP rescaled by alpha = 2^a in the objective, 2^sx[i] per state entry and 2^su[j] per input entry is the same problem in other
units, and every add, multiply, fma, divide and square root of a dual Newton iteration gives exactly the scaled result.  A kernel
with a hidden unit -- an absolute constant, a comparison against an unscaled quantity, an intermediate with too little exponent
range, a reciprocal (square root) refinement tuned on pivots of order 1 -- does not.  So the mapped arrays are compared with
np.array_equal: no tolerance is involved.

Rows: one per route and node kind, the smallest problems the suite has (scale_cases.ROUTE_ROWS, rows of trace_cases.py).
- fixed iteration counts (maxIter 1, 2, 3, stationarityTolerance 0, regType 0) under PER-ENTRY scalings with exponents in [-20, 20] and
  a = +-30; the members of a batched launch carry different scalings in one launch.  The unscaled run is also held to the oracle
  (clipping rows), so that equivariance cannot hide an error the two runs share;
- whole solves under UNIFORM scalings (s = 12, t = -9, a = 20; s = t = 0, a = +-400) with scale_cases.scaled_opts, under the three
  termination norms, and on rows of reg_cases.py whose blocks are regularised (a pivot at or below regTol^2, an exact zero, ALWAYS);
- the stage solvers of kinds 2 and 3: the same working sets and step counts, cold (first solve) and hot-started (the following ones),
  under per-entry scalings that include the rows;
- tqgpu_kkt_residual_at under uniform scalings: the six classes mapped exactly, the same arg-max nodes;
- MPC steps on both root forms, the tracking fold, the shifted warm start, and sensitivities, predictions, adjoints and adjoint
  matrices (single and reduced batch), the derivatives also within the existing bounds of the block references on the scaled problem."""
from __future__ import annotations

import numpy as np
import pytest

import adj_cases as AC
import adj_ref as AR
import adjmat_cases as XC
import adjmat_ref as AM
import kkt_ref as K
import sens_cases as SN
import sens_ref as SR
import tracking_cases as KC
import mpc_cases as MC
import reg_cases as RC
import scale_cases as SCL
import solve_sequence_cases as SC
import trace_cases as TC
from helpers import assert_solution_close, with_dense_blocks

pytestmark = pytest.mark.gpu

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u", "dlam", "mu_d")
COUNTS = ("status", "iter", "ls_total", "ls_last", "n_launches")
TOL = 1e-10          # of test_gpu_parity.py


@pytest.fixture(scope="module")
def gpu(capi):
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: the -m gpu tests must run on the MI355X box")
    return capi


def _same_arrays(base, got, what):
    """got, already mapped back into the units of base, equals it bit for bit"""
    for k in base:
        if isinstance(base[k], np.ndarray):
            a, b = np.asarray(got[k]), base[k]
            assert a.shape == b.shape, (what, k)
            if not np.array_equal(a, b):
                bad = np.flatnonzero(a.ravel() != b.ravel())
                i = bad[0]
                raise AssertionError(f"{what}: {k} differs in {len(bad)} of {a.size} entries; first [{i}] {a.ravel()[i]!r} != {b.ravel()[i]!r}")


class Group:
    """the mirrors of one run of a row (one, or the members of a batch), made under the row's switches from given problems"""

    def __init__(self, gpu, monkeypatch, r, problems):
        self.gpu, self.r = gpu, r
        for k, v in r["env"].items():
            if k not in SC.SWITCHES:
                monkeypatch.setenv(k, v)
        with SC.switches({k: v for k, v in r["env"].items() if k in SC.SWITCHES}):
            self.ms = [TC.upload(gpu, pr, single=r["single"], batch=r["batch"]) for pr in problems]
        for k in r["env"]:
            if k not in SC.SWITCHES:
                monkeypatch.delenv(k)

    def solve(self, **opts):
        res = self.gpu.solve_batch(self.ms, **opts) if self.r["batch"] else [self.ms[0].solve(**opts)]
        out = []
        for q, g in zip(res, self.ms):
            plan = g.plan
            rec = dict(q=q, sol=g.solution(), log=g.iteration_log()[0][:q["iter"]].copy(), plan=plan,
                       route=SC.route_seen(g, plan, 0, opts.get("maxIter", 100)))
            if plan["box"] or plan["gen"]:
                rec["sets"] = g.working_sets()
            if plan["gen"]:
                rec["steps"] = g.stage_steps()
            out.append(rec)
        return out

    def close(self):
        for g in self.ms:
            g.close()


def _members(r, pr):
    """the problems of a row's run: two members with their own starting duals for a batch row"""
    if not r["batch"]:
        return [pr]
    return [dict(pr, lam0=TC.member_duals(pr, i)) for i in range(2)]


def _scaled_member(pr, s):
    return dict(pr, d=SCL.scaled(pr["d"], s), lam0=SCL.map_lam(pr["lam0"], s))


def _compare(base, got, s, what, term=None):
    """one member's record of the scaled run against that of the unscaled run"""
    for k in COUNTS:
        assert got["q"][k] == base["q"][k], (what, k, got["q"], base["q"])
    assert got["route"] == base["route"] and got["plan"] == base["plan"], (what, got["route"], base["route"])
    assert np.array_equal(got["log"], base["log"]), (what, got["log"], base["log"])
    fv = float(SCL.map_fval(got["q"]["last_fval"], s, -1))
    assert fv == base["q"]["last_fval"] or (np.isnan(fv) and np.isnan(base["q"]["last_fval"])), (what, "last_fval", fv, base["q"]["last_fval"])
    if term is not None:
        en = float(SCL.map_error_norm(got["q"]["last_error_norm"], s, term, -1))
        assert en == base["q"]["last_error_norm"], (what, "last_error_norm", en, base["q"]["last_error_norm"])
    _same_arrays(base["sol"], SCL.map_solution(got["sol"], s, -1), what)
    for k in ("sets", "steps"):
        if k in base:
            _same_arrays(base[k], got[k], (what, k))


@pytest.mark.parametrize("rid", SCL.ROUTE_ROWS)
def test_fixed_iteration_counts_under_per_entry_scaling(gpu, orc, monkeypatch, rid):
    r, pr = SCL.row(rid), SCL.problem(rid, gpu)
    members = _members(r, pr)
    scal = [SCL.entry_scaling(pr["d"], i) for i in range(len(members))]
    G0 = Group(gpu, monkeypatch, r, members)
    G1 = Group(gpu, monkeypatch, r, [_scaled_member(m, s) for m, s in zip(members, scal)])
    # the oracle comparison stops where the oracle's own solve ends: an iteration from a converged point is decided by rounding (its
    # Armijo test compares dual values that differ by less than their last place), in the oracle as on the device
    n_orc = [orc.solve(pr["d"], orc.default_opts(), lambda0=m["lam0"])["iter"] if r["clip"] else 0 for m in members]
    try:
        for k in SCL.FIXED_ITERS:
            opts = dict(r["opts"], maxIter=k, stationarityTolerance=0.0, regType=0)
            base, got = G0.solve(**opts), G1.solve(**opts)
            for i, (b, g, s, m) in enumerate(zip(base, got, scal, members)):
                if r["route"]:
                    assert b["route"] == r["route"], (rid, b["route"])
                assert b["q"]["iter"] >= 1, (rid, k, b["q"])
                _compare(b, g, s, (rid, f"maxIter={k}", f"member {i}"))
                if r["clip"] and k <= n_orc[i] and rid not in SCL.NO_ORACLE:
                    oo = {a: v for a, v in opts.items() if a != "checkLastActiveSet" or v != 2}
                    ref = orc.solve(pr["d"], orc.default_opts(**oo), lambda0=m["lam0"])
                    assert (b["q"]["status"], b["q"]["iter"], b["q"]["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), (rid, k, b["q"])
                    assert b["log"].tolist() == ref["trace_ls"][:ref["iter"]].tolist(), (rid, k)
                    assert_solution_close(b["sol"], ref, TOL)
    finally:
        G0.close(); G1.close()


@pytest.mark.parametrize("rid", SCL.ROUTE_ROWS)
def test_whole_solves_under_uniform_scaling(gpu, orc, monkeypatch, rid):
    r, pr = SCL.row(rid), SCL.problem(rid, gpu)
    members = _members(r, pr)
    scalings = SCL.uniform_scalings(pr["d"])
    G0 = Group(gpu, monkeypatch, r, members)
    Gs = [Group(gpu, monkeypatch, r, [_scaled_member(m, s) for m in members]) for _, s in scalings]
    try:
        for term in TC.NORMS:
            opts = TC.solve_opts(r, term)
            base = G0.solve(**opts)
            for b in base:
                assert b["q"]["status"] == 0 and b["q"]["iter"] >= 1, (rid, term, b["q"])
            if r["clip"]:
                oo = {a: v for a, v in opts.items() if a != "checkLastActiveSet" or v != 2}
                for b, m in zip(base, members):
                    ref = orc.solve(pr["d"], orc.default_opts(**oo), lambda0=m["lam0"])
                    assert (b["q"]["status"], b["q"]["iter"], b["q"]["ls_total"]) == (ref["status"], ref["iter"], ref["ls_total"]), (rid, term, b["q"])
            for (name, s), G in zip(scalings, Gs):
                got = G.solve(**SCL.scaled_opts(opts, s))
                for i, (b, g) in enumerate(zip(base, got)):
                    _compare(b, g, s, (rid, f"norm {term}", name, f"member {i}"), term)
    finally:
        G0.close()
        for G in Gs:
            G.close()


# ---- regularised blocks: rows of reg_cases.py under uniform scalings, the options scaled with them ----

def _reg_mirror(gpu, monkeypatch, route, d, lam0):
    for k in ("TREEQP_AMD_PATH", "TREEQP_AMD_NO_PERSIST_ONE", "TREEQP_AMD_NO_WIDE3"):
        monkeypatch.delenv(k, raising=False)
    for k, v in RC.ROUTES[route][0].items():
        monkeypatch.setenv(k, v)
    g = gpu.TqGpu(d["nk"], d["nx"], d["nu"])
    if route == "dense_single":
        g.upload_mixed(with_dense_blocks(d), np.full(len(d["nk"]), 2, np.int32), lam0)
        g.set_dense_single_launch(True)
    else:
        g.upload(d, lam0)
    for k in RC.ROUTES[route][0]:
        monkeypatch.delenv(k)
    return g


@pytest.mark.parametrize("rid", SCL.REG_ROWS)
def test_regularised_steps_and_solves_under_uniform_scaling(gpu, monkeypatch, rid):
    """the on-the-fly trigger (first-pass pivot <= regTol^2: threshold_below rows sit at regTol / 2, flag_* rows at an exact zero) and
    the ALWAYS shift: one iteration (the step itself, dlam) and the whole solve"""
    row, c = RC.row(rid), RC.case(rid)
    d, lam0 = c["d"], c["lam0"]
    _, path, flags = RC.ROUTES[row.route]
    for name, s in SCL.uniform_scalings(d):
        g0 = _reg_mirror(gpu, monkeypatch, row.route, d, lam0)          # (fresh mirrors on both sides: the first solve of a mirror launches more)
        g1 = _reg_mirror(gpu, monkeypatch, row.route, SCL.scaled(d, s), SCL.map_lam(lam0, s))
        try:
            assert g0.path == path and all(g0.plan[k] == v for k, v in flags.items()), (rid, g0.path, g0.plan)
            for iters in (1, 100):
                opts = dict(row.opts, maxIter=iters)
                q0 = g0.solve(**opts)
                q1 = g1.solve(**SCL.scaled_opts(opts, s))
                base = dict(q=q0, sol=g0.solution(), log=g0.iteration_log()[0][:q0["iter"]].copy(), plan=g0.plan, route=None)
                got = dict(q=q1, sol=g1.solution(), log=g1.iteration_log()[0][:q1["iter"]].copy(), plan=g1.plan, route=None)
                assert q0["iter"] >= 1
                _compare(base, got, s, (rid, name, f"maxIter={iters}"), 2)
        finally:
            g0.close(); g1.close()


# ---- the KKT check ----

@pytest.mark.parametrize("rid", ["single_wg-clip-small8", "fused_tails-dense", "per_phase-box", "per_phase-gen"])
def test_kkt_residuals_under_uniform_scaling(gpu, monkeypatch, rid):
    """tqgpu_kkt_residual_at at a random point (every class non-zero) and tqgpu_kkt_residual after a solve: under a uniform scaling
    with s = t (a class maximum is taken over state and input rows) the six classes are mapped exactly and name the same nodes"""
    r, pr = SCL.row(rid), SCL.problem(rid, gpu)
    d = pr["d"]
    point = K.random_point(d, 5)
    G0 = Group(gpu, monkeypatch, r, [pr])
    try:
        g0 = G0.ms[0]
        at0 = g0.kkt_residual_at(point, per_node=True)
        opts = TC.solve_opts(r, 2)
        q0 = g0.solve(**opts)
        assert q0["status"] == 0
        k0 = g0.kkt_residual(per_node=True)
        for s in (SCL.scaling(d, 12, 12, 20, 12), SCL.scaling(d, -7, -7, -30, 3), SCL.scaling(d, 0, 0, 400), SCL.scaling(d, 0, 0, -400)):
            G1 = Group(gpu, monkeypatch, r, [_scaled_member(pr, s)])
            try:
                g1 = G1.ms[0]
                at1 = g1.kkt_residual_at(SCL.map_solution(point, s), per_node=True)
                q1 = g1.solve(**SCL.scaled_opts(opts, s))
                k1 = g1.kkt_residual(per_node=True)
            finally:
                G1.close()
            assert (q1["status"], q1["iter"], q1["ls_total"]) == (q0["status"], q0["iter"], q0["ls_total"]), (rid, s["a"])
            for what, b, g in (("at a point", at0, at1), ("after a solve", k0, k1)):
                assert np.array_equal(g["node"], b["node"]), (rid, what, s["a"], g["node"], b["node"])
                assert np.array_equal(SCL.map_kkt(g["res"], s, -1), b["res"], equal_nan=True), (rid, what, s["a"], g["res"], b["res"])
                assert np.array_equal(SCL.map_kkt(g["per_node"], s, -1), b["per_node"], equal_nan=True), (rid, what, s["a"])
    finally:
        G0.close()


# ---- MPC steps on an eliminated root, their sensitivities and adjoints ----

def _mpc_make(gpu, c, s=None):
    if s is None:
        return MC.make(gpu, c)
    g = MC.make(gpu, c, SCL.scaled(c["d"], s), root=False)
    r = SCL.map_root_terms(c["root"], c["d"], s)
    return g.mpc_set_root(r["A0"], r["b0"], r["S0"], r["r0"], r["C0"], r["dmin0"], r["dmax0"])


@pytest.mark.parametrize("cid", SCL.MPC_IDS)
def test_mpc_steps_under_uniform_scaling(gpu, cid):
    """tqgpu_mpc_step with a warm start from the last solve's duals: per step the folded root terms, u[0], the verdict, the counts and
    the whole solution are mapped exactly, and the counters of tqgpu_mpc_stats are the same"""
    c = MC.case(cid)
    x0s = MC.exact_x0s(c["nx0"], 3)[:3]
    g0 = _mpc_make(gpu, c).set_warm_start(1)
    try:
        base = []
        for x0 in x0s:
            q, u0 = g0.mpc_step(x0, **c["opts"])
            base.append((q, u0, g0.root_terms(), g0.solution(), gpu.mpc_stats()))
            assert q["status"] == 0, (cid, q)
        for name, s in SCL.mpc_scalings(c):
            g1 = _mpc_make(gpu, c, s).set_warm_start(1)
            try:
                for i, (x0, (q0, u00, rt0, sol0, st0)) in enumerate(zip(x0s, base)):
                    q1, u01 = g1.mpc_step(SCL.map_x0(x0, s), **SCL.scaled_opts(c["opts"], s))
                    what = (cid, name, f"step {i}")
                    assert all(q1[k] == q0[k] for k in COUNTS), (what, q1, q0)
                    assert gpu.mpc_stats() == st0, (what, gpu.mpc_stats(), st0)
                    _same_arrays(rt0, SCL.map_root_terms(g1.root_terms(), c["d"], s, -1), (what, "root terms"))
                    assert np.array_equal(SCL.shift(u01, -s["su"][:len(u01)]), u00), (what, "u0")
                    _same_arrays(sol0, SCL.map_solution(g1.solution(), s, -1), what)
            finally:
                g1.close()
    finally:
        g0.close()


# ---- both root forms, the tracking fold and the shifted warm start: the cases of tracking_cases.py ----

@pytest.mark.parametrize("cid", KC.CASE_IDS)
def test_mpc_loop_with_tracking_and_shift_under_uniform_scaling(gpu, cid):
    """tracking_cases.py has a root that keeps its states (x0 in its bounds) and an eliminated root on every route.  tqgpu_mpc_set_window,
    then tqgpu_get_linear_terms: the folded q, r mapped exactly.  Then three steps of tqgpu_mpc_step_at with the shifted warm start
    (tqgpu_mpc_set_shift, mode 2, the realised child changing): per step the verdict, the counts, tqgpu_mpc_stats, u[0], the folded root
    data (b, r, dmin, dmax of an eliminated root; the root's bounds of one with states), q, r and the whole solution."""
    c = KC.case(cid)
    nk0 = int(c["d"]["nk"][0])

    def run(g, cc):
        out = []
        for t0 in (0, 3):
            g.mpc_set_window(t0)
            out.append(dict(zip(("q", "r"), g.linear_terms())))
        g.mpc_set_shift(gpu.SHIFT_LEAF_REPEAT, gpu.SHIFT_DUALS)
        g.set_warm_start(2)
        for step in range(3):
            if step > 0:
                g.mpc_set_realised(step % nk0)
            q, u0 = g.mpc_step(cc["x0s"][step], t0=step, **cc["opts"])
            rec = dict(counts=[q[k] for k in COUNTS], fval=q["last_fval"], err=q["last_error_norm"], stats=gpu.mpc_stats(), u0=u0, sol=g.solution())
            rec["q"], rec["r"] = g.linear_terms()
            if cc["form"] == "elim":
                rec["root"] = g.root_terms()
            else:
                rec["lo"], rec["hi"] = g.root_bounds()
            out.append(rec)
        return out

    g0 = KC.make(gpu, c)
    try:
        base = run(g0, c)
    finally:
        g0.close()
    assert all(b["counts"][0] == 0 for b in base[2:]), (cid, [b["counts"] for b in base[2:]])
    for name, s in SCL.case_scalings(c):
        cs = dict(SCL.scaled_tracking_case(c, s), opts=SCL.scaled_opts(c["opts"], s))
        g1 = KC.make(gpu, cs)
        try:
            got = run(g1, cs)
        finally:
            g1.close()
        nu0 = int(c["d"]["nu"][0])
        for i, (b, g) in enumerate(zip(base, got)):
            what = (cid, name, i)
            lin = dict(zip(("q", "r"), SCL.map_linear_terms(g["q"], g["r"], s, -1)))
            _same_arrays(dict(q=b["q"], r=b["r"]), lin, what)
            if "counts" not in b:
                continue
            assert g["counts"] == b["counts"] and g["stats"] == b["stats"], (what, g["counts"], b["counts"], g["stats"], b["stats"])
            assert float(SCL.map_fval(g["fval"], s, -1)) == b["fval"] and float(SCL.map_error_norm(g["err"], s, 2, -1)) == b["err"], what
            assert np.array_equal(SCL.shift(g["u0"], -s["su"][:nu0]), b["u0"]), (what, "u0")
            _same_arrays(b["sol"], SCL.map_solution(g["sol"], s, -1), what)
            if "root" in b:
                _same_arrays(b["root"], SCL.map_root_terms(g["root"], c["d"], s, -1), (what, "root terms"))
            else:
                _same_arrays(dict(lo=b["lo"], hi=b["hi"]), dict(lo=SCL.map_x0(g["lo"], s, -1), hi=SCL.map_x0(g["hi"], s, -1)), (what, "root bounds"))


# ---- derivatives: the cases of sens_cases.py / adj_cases.py / adjmat_cases.py, both root forms ----

DERIV_IDS = ("elim-single_wg", "elim-persist_c1", "elim-three_launch", "elim-generic", "elim-dense_kind1_root", "states-persist_c1", "states-generic",
             "states-tiered_ub", "states-three_children")


def _derivatives(gpu, c, opts, ropts, maps, pad_of, x0_new):
    """one step at the case's x0, then every derivative call -> dict"""
    g = SN.make(gpu, c)
    try:
        q, _ = g.mpc_step(c["x0"], **opts)
        sol = g.solution()
        n_reg = g.mpc_sensitivity(**ropts)
        K_, u0, x0r = g.mpc_gain()
        sens = g.mpc_sensitivities()
        pred, nclip = g.mpc_predict(x0_new)
        pad = pad_of(g)
        hg, cg = XC.maps(c, maps, pad)
        g.mpc_set_param_groups(hg, cg)
        adj = g.mpc_adjoint(*c["w"], **ropts)
        grads = g.mpc_adjoint_grads()
        mats = g.mpc_adjoint_matrices()
        return dict(q=q, sol=sol, n_reg=n_reg, K=K_, u0=u0, x0r=x0r, sens=sens, pred=pred, nclip=nclip, gx0=adj["gx0"], n_reg_adj=adj["n_reg"],
                    grads=grads, mats=mats, pad=pad, groups=XC.filled(c, hg, cg))
    finally:
        g.close()


def _pad_of(gpu):
    import ctypes as C

    def pad(g):
        g.mpc_set_param_groups(None, None)
        hd = np.zeros(5 * len(g.nk), dtype=np.int32)
        assert gpu.lib().tqgpu_mpc_get_param_groups(g.h, None, None, hd.ctypes.data_as(C.POINTER(C.c_int)), None, None) == 0
        return int(hd[2])
    return pad


@pytest.mark.parametrize("reg", [0, 2], ids=["no_reg", "scaled_reg_options"])
@pytest.mark.parametrize("cid", DERIV_IDS)
def test_mpc_derivatives_under_uniform_scaling(gpu, cid, reg):
    """tqgpu_mpc_sensitivity (K, dz/dx0, dlam/dx0, n_reg), tqgpu_mpc_predict, tqgpu_mpc_adjoint (gx0, gq, gr, gb) and
    tqgpu_mpc_adjoint_matrices (shared groups) of one step, on both root forms: mapped exactly, with regType 0 and with the
    regularisation options scaled along.  On the SCALED problem each also stays within the existing bound (sens_cases.tol,
    adj_cases.tol, adjmat_cases.tol, taken in the original units) of the block references evaluated on the scaled problem at the
    device's own scaled point, so that an error the scaled and the unscaled run share cannot pass."""
    c = AC.case(cid)
    opts = dict(c["base"]["opts"], regType=reg)
    ropts = SCL.reg_of(opts)
    x0_new = c["x0"] + 2.0 ** -6
    b = _derivatives(gpu, c, opts, ropts, "shared", _pad_of(gpu), x0_new)
    assert b["q"]["status"] == 0
    nu0 = len(b["u0"])
    for name, s in SCL.case_scalings(c):
        cs = SCL.scaled_sens_case(c, s)
        rs = SCL.reg_of(opts, s)
        g = _derivatives(gpu, cs, SCL.scaled_opts(opts, s), rs, "shared", _pad_of(gpu), SCL.map_x0(x0_new, s))
        what = (cid, name)
        assert all(g["q"][k] == b["q"][k] for k in COUNTS), (what, g["q"], b["q"])
        assert (g["n_reg"], g["n_reg_adj"], g["nclip"], g["pad"]) == (b["n_reg"], b["n_reg_adj"], b["nclip"], b["pad"]), what
        dims = SCL.group_dims(c["d"], b["groups"][0], b["pad"])
        back = dict(K=SCL.map_gain(g["K"], s, c["d"], -1), u0=SCL.shift(g["u0"], -s["su"][:nu0]), x0r=SCL.map_x0(g["x0r"], s, -1),
                    pred=SCL.shift(g["pred"], -s["su"][:nu0]))
        back.update(SCL.map_sensitivities(g["sens"], s, -1))
        back.update(SCL.map_adjoint(dict(g["grads"], gx0=g["gx0"]), s, -1))
        ref = dict(K=b["K"], u0=b["u0"], x0r=b["x0r"], pred=b["pred"], gx0=b["gx0"], **b["sens"], **b["grads"])
        _same_arrays(ref, back, what)
        _same_arrays(b["sol"], SCL.map_solution(g["sol"], s, -1), what)
        mb = SCL.map_adjoint_matrices(g["mats"], s, c["d"], dims, -1)
        for key in AM.KEYS:
            assert len(mb[key]) == len(b["mats"][key]), (what, key)
            _same_arrays({f"{key}[{i}]": x for i, x in enumerate(b["mats"][key])}, {f"{key}[{i}]": x for i, x in enumerate(mb[key])}, what)
        # the references on the scaled problem, at the scaled device point
        sol = g["sol"]
        rb = SR.dual_form(cs["d"], sol["x"], sol["u"], cs["param"], cs["kinds"], **rs)
        rsens = dict(SCL.map_sensitivities({k: rb[k] for k in ("dx", "du", "dlam")}, s, -1), K=SCL.map_gain(rb["K"], s, c["d"], -1))
        for k in ("K", "dx", "du") + (("dlam",) if g["n_reg"] == 0 else ()):
            err = float(np.max(np.abs(back[k] - rsens[k]), initial=0.0))
            assert err <= SN.tol(cid, k), (what, k, err)
        ra = AR.dual_form(cs["d"], sol["x"], sol["u"], cs["param"], cs["w"], cs["kinds"], **rs)
        radj = SCL.map_adjoint({k: ra[k] for k in ("gq", "gr", "gb", "gx0")}, s, -1)
        for k in ("gq", "gr", "gx0") + (("gb",) if g["n_reg_adj"] == 0 else ()):
            err = float(np.max(np.abs(back[k] - radj[k]), initial=0.0))
            assert err <= AC.tol(cid, k), (what, k, err)
        if ra["n_reg"] == 0:
            rm = AM.outer(cs["d"], sol["x"], sol["u"], sol["lam"], cs["param"], ra, cs["kinds"], g["groups"][0], g["groups"][1], cs["x0"], g["pad"])
            rmb = SCL.map_adjoint_matrices(rm, s, c["d"], dims, -1)
            for key in AM.KEYS:
                for i, (x, y) in enumerate(zip(mb[key], rmb[key])):
                    err = float(np.max(np.abs(x - y), initial=0.0))
                    assert err <= XC.tol(cid, key), (what, key, i, err)


@pytest.mark.parametrize("cid", ["elim-three_children", "states-generic"])
def test_adjoint_matrices_batch_with_reduction_under_uniform_scaling(gpu, cid):
    """tqgpu_mpc_adjoint_matrices_batch with reduce = 1 over two members with different loss gradients: the sums mapped exactly"""
    c = AC.case(cid)
    opts = c["base"]["opts"]

    def run(cc, o):
        gs = []
        try:
            for i in range(2):
                g = SN.make(gpu, cc)
                gs.append(g)
                q, _ = g.mpc_step(cc["x0"], **o)
                assert q["status"] == 0
                pad = _pad_of(gpu)(g)
                hg, cg = XC.maps(cc, "shared", pad)
                g.mpc_set_param_groups(hg, cg)
                g.mpc_adjoint(cc["w"][0] * (1.0 + i), cc["w"][1] * (1.0 - 0.25 * i), **SCL.reg_of(o))
            return gpu.mpc_adjoint_matrices_batch(gs, reduce=True), XC.filled(cc, hg, cg), pad
        finally:
            for g in gs:
                g.close()

    base, groups, pad = run(c, opts)
    dims = SCL.group_dims(c["d"], groups[0], pad)
    for name, s in SCL.case_scalings(c):
        got, _, _ = run(SCL.scaled_sens_case(c, s), SCL.scaled_opts(opts, s))
        mb = SCL.map_adjoint_matrices(got, s, c["d"], dims, -1)
        for key in AM.KEYS:
            assert len(mb[key]) == len(base[key]), (cid, name, key)
            _same_arrays({f"{key}[{i}]": x for i, x in enumerate(base[key])}, {f"{key}[{i}]": x for i, x in enumerate(mb[key])}, (cid, name))


@pytest.mark.parametrize("route", ["wide", "wide3"])
def test_identity_padding_takes_no_part_in_the_on_the_fly_trigger(gpu, monkeypatch, route):
    """The wide-block factorisations pad a block to 16-column panels with identity.  With regTol = 1 on a problem whose first-pass
    pivots all lie above 2.8 (reg_cases' "wtree" with the objective divided by 64: reg_ref flags no block, guard >= GUARD_MIN) the
    step is the unregularised reference step to reg_cases.TOL; a padding pivot of 1.0 that met regTol^2 would shift every block
    whose dimension is no multiple of 16 by regValue = 1e-2."""
    import newton_ref as N
    import reg_ref
    d = SCL.scaled(RC.base_problem("wtree"), SCL.scaling(RC.base_problem("wtree"), 0, 0, -6))
    lam0 = N.seeded_duals(int(np.asarray(d["nx"])[1:].sum()), 0)
    opts = dict(regType=2, regTol=1.0, regValue=1e-2)
    ref = reg_ref.block_newton_step(d, lam0, **opts)
    assert not ref["flagged"] and ref["guard"] >= RC.GUARD_MIN and ref["margin"] > RC.GAP and ref["cond"] <= RC.COND_MAX
    g = _reg_mirror(gpu, monkeypatch, route, d, lam0)
    try:
        _, path, flags = RC.ROUTES[route]
        assert g.path == path and all(g.plan[k] == v for k, v in flags.items())
        r = g.solve(maxIter=1, **opts)
        sol = g.solution()
    finally:
        g.close()
    scale = max(1.0, float(np.max(np.abs(ref["dlam"]))))
    err = float(np.max(np.abs(sol["dlam"] - ref["dlam"]))) / scale
    print(f"{route}: dlam {err:.2e}")
    assert r["iter"] == 1 and err <= RC.TOL

"""Power-of-two scale equivariance without a device (scale_cases.py has the transform):

1. the transform is right: the kkt_ref residuals of a mapped point of the scaled problem are the mapped residuals of
   the original entry by entry, and the references newton_ref.newton_step and reg_ref.block_newton_step on the scaled problem agree with
   their mapped unscaled result (reg_ref's own cross-check bound, XCHECK_TOL of the largest entry, in the original units);
2. the oracle is EXACTLY equivariant on every clipping case test_gpu_scale.py uses: x, u, lam, multipliers, dual-value trace, trial
   log, n_active and n_regularized bit for bit.  That is what lets the device test demand equality.  No case is tolerated, skipped or
   xfailed: one on which the oracle were not equivariant (its absolute dotp > 1e-10 falling the other way once scaled) would have to be
   replaced by another seed or exponent set.

Run with -s for the measured spreads."""
from __future__ import annotations

import numpy as np
import pytest

import gen_cases as GC
import kkt_ref as K
import mpc_cases as MC
import newton_ref as N
import reg_cases as RC
import reg_ref as R
import scale_cases as SCL
import trace_cases as TC
from limit_shapes import flatten

SOL_KEYS = ("x", "u", "lam", "mu_x", "mu_u")


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0


# ---- 1. the transform ----

def test_scaling_and_unscaling_are_inverse_and_exact():
    d = GC.case("row_and_bound")["d"]
    s = SCL.entry_scaling(d, 0)
    back = SCL.scaled(SCL.scaled(d, s), {k: (-v if k in ("sx", "su", "sc", "x0") else v) for k, v in dict(s, a=-s["a"]).items()})
    for k, v in d.items():
        assert np.array_equal(np.asarray(v), back[k]), k


@pytest.mark.parametrize("seed", [1, 2])
def test_kkt_residuals_of_a_mapped_point_are_the_mapped_residuals(seed):
    shape = (3, 2, [(4, 2, [(2, 0, []), (3, 0, [])]), (2, 1, [(2, 0, [])])])
    nk, nx, nu = flatten(shape)
    kinds = np.array([3, 2, 0, 1, 1, 1])[:len(nk)]
    d = K.random_problem(shape, kinds, seed, nc=np.where(kinds == 3, 2, 0))
    sol = K.random_point(d, seed)
    s = SCL.entry_scaling(d, seed)
    ref = K.residuals(d, sol, kinds)
    got = K.residuals(SCL.scaled(d, s), SCL.map_solution(sol, s), kinds)
    xo, uo, ro = (np.concatenate([[0], np.cumsum(np.asarray(v, int))]) for v in (nx, nu, d["nc"]))
    a = s["a"]
    for k in range(len(nk)):
        ez = np.concatenate([s["sx"][xo[k]:xo[k + 1]], s["su"][uo[k]:uo[k + 1]]])
        er = s["sc"][ro[k]:ro[k + 1]]
        exps = {K.STAT: a - ez, K.DYN: s["sx"][xo[k]:xo[k + 1]], K.BFEAS: ez, K.BCOMPL: np.full(len(ez), a), K.GFEAS: er, K.GCOMPL: np.full(len(er), a)}
        for c in range(6):
            v0, T0, m0 = ref["entries"][c][k]
            v1, T1, m1 = got["entries"][c][k]
            assert len(v0) == len(v1) and np.array_equal(m0, m1)
            if len(v0):
                assert np.array_equal(SCL.shift(v0, exps[c]), v1, equal_nan=True), (k, c)
                assert np.array_equal(SCL.shift(T0, exps[c]), T1, equal_nan=True), (k, c)


REF_ROWS = ("single_wg-clip-small8", "persist-chain7", "fused_tails-dense", "per_phase-box")


@pytest.mark.parametrize("rid", REF_ROWS)
def test_newton_reference_on_the_scaled_problem_is_the_mapped_step(capi, rid):
    pr = TC.problem(rid, capi)
    d, lam0, kinds, dense = pr["d"], pr["lam0"], pr["kinds"], pr["dense"]
    base = N.newton_step(d, lam0, dense, kinds)
    for name, s in [("entry", SCL.entry_scaling(d, 0))] + SCL.uniform_scalings(d):
        got = N.newton_step(SCL.scaled(d, s), SCL.map_lam(lam0, s), dense, kinds)
        e_res = _rel(SCL.shift(got["res"], -s["sx"][len(s["sx"]) - s["nlam"]:]), base["res"])
        e_dl = _rel(SCL.map_lam(got["dlam"], s, -1), base["dlam"])          # (res has the units of x)
        print(f"{rid} {name}: res {e_res:.2e} dlam {e_dl:.2e} (cond {base['cond']:.2e})")
        assert e_res <= R.XCHECK_TOL and e_dl <= R.XCHECK_TOL * max(1.0, base["cond"] * 1e-3)


@pytest.mark.parametrize("rid", ["generic-flag_mid_level", "generic-threshold_below", "generic-always", "persist_one-flag_mid_level-u6"])
def test_regularised_reference_on_the_scaled_problem_is_the_mapped_step(rid):
    """uniform scalings with scaled_opts: the same blocks flagged, the same zero columns, the mapped step"""
    row, c = RC.row(rid), RC.case(rid)
    base = c["ref"]
    for name, s in SCL.uniform_scalings(c["d"]):
        o = SCL.scaled_opts(row.opts, s)
        got = R.block_newton_step(SCL.scaled(c["d"], s), SCL.map_lam(c["lam0"], s), o["regType"], o["regTol"], o["regValue"])
        e = _rel(SCL.map_lam(got["dlam"], s, -1), base["dlam"])
        print(f"{rid} {name}: dlam {e:.2e} flagged {sorted(got['flagged'])[:6]}")
        assert sorted(got["flagged"]) == sorted(base["flagged"]) and np.array_equal(got["zero"], base["zero"])
        assert e <= R.XCHECK_TOL


# ---- 2. the oracle ----

CLIP_ROWS = [rid for rid in SCL.ROUTE_ROWS if SCL.row(rid)["clip"]]


def _same_run(ref, got, s, what):
    back = SCL.map_solution({k: got[k] for k in SOL_KEYS}, s, -1)
    for k in SOL_KEYS:
        assert np.array_equal(back[k], ref[k]), (what, k, _rel(back[k], ref[k]))
    n = ref["iter"]
    assert (got["status"], got["iter"], got["ls_total"], got["n_active"], got["n_regularized"]) == \
        (ref["status"], ref["iter"], ref["ls_total"], ref["n_active"], ref["n_regularized"]), what
    assert np.array_equal(got["trace_ls"][:n], ref["trace_ls"][:n]), what
    assert np.array_equal(SCL.map_fval(got["trace_fval"][:n + 1], s, -1), ref["trace_fval"][:n + 1], equal_nan=True), what


@pytest.mark.parametrize("rid", CLIP_ROWS)
def test_oracle_is_exactly_equivariant_at_fixed_iteration_counts(orc, capi, rid):
    r, pr = SCL.row(rid), SCL.problem(rid, capi)
    d = pr["d"]
    for i in range(2):
        s = SCL.entry_scaling(d, i)
        lam0 = TC.member_duals(pr, i) if r["batch"] else pr["lam0"]
        ds, ls = SCL.scaled(d, s), SCL.map_lam(lam0, s)
        for k in SCL.FIXED_ITERS:
            o = dict(maxIter=k, stationarityTolerance=0.0, regType=0)
            _same_run(orc.solve(d, orc.default_opts(**o), lam0), orc.solve(ds, orc.default_opts(**o), ls), s, (rid, i, k))


@pytest.mark.parametrize("term", TC.NORMS)
@pytest.mark.parametrize("rid", CLIP_ROWS)
def test_oracle_is_exactly_equivariant_on_whole_solves(orc, capi, rid, term):
    r, pr = SCL.row(rid), SCL.problem(rid, capi)
    d, lam0 = pr["d"], pr["lam0"]
    opts = {k: v for k, v in TC.solve_opts(r, term).items() if k != "checkLastActiveSet" or v != 2}
    ref = orc.solve(d, orc.default_opts(**opts), lam0)
    assert ref["status"] == 0
    for name, s in SCL.uniform_scalings(d):
        got = orc.solve(SCL.scaled(d, s), orc.default_opts(**SCL.scaled_opts(opts, s)), SCL.map_lam(lam0, s))
        _same_run(ref, got, s, (rid, term, name))
        n = ref["iter"]
        assert np.array_equal(SCL.map_error_norm(got["trace_err"][:n + 1], s, term, -1), ref["trace_err"][:n + 1], equal_nan=True), (rid, term, name)


@pytest.mark.parametrize("rid", SCL.REG_ROWS)
def test_oracle_is_exactly_equivariant_where_blocks_are_regularised(orc, rid):
    """rows of reg_cases.py: a pivot at or below regTol^2 (threshold_below), an exact zero (flag_*), ALWAYS"""
    row, c = RC.row(rid), RC.case(rid)
    d, lam0 = c["d"], c["lam0"]
    for iters in (1, 100):
        opts = dict(row.opts, maxIter=iters)
        ref = orc.solve(d, orc.default_opts(**opts), lam0)
        if iters == 1:
            assert ref["n_regularized"] >= (1 if row.opts["regType"] else 0)
        for name, s in SCL.uniform_scalings(d):
            got = orc.solve(SCL.scaled(d, s), orc.default_opts(**SCL.scaled_opts(opts, s)), SCL.map_lam(lam0, s))
            _same_run(ref, got, s, (rid, iters, name))


@pytest.mark.parametrize("cid", [c for c in SCL.MPC_IDS if c in MC.CLIPPING_IDS])
def test_oracle_is_exactly_equivariant_on_the_folded_mpc_problems(orc, cid):
    """the problem of the first MPC step of test_gpu_scale.py (x0 folded into b of the root's children in numpy), solved cold"""
    c = MC.case(cid)
    x0 = MC.exact_x0s(c["nx0"], 3)[0]
    d = MC.folded(c, MC.fold(c["root"], x0))
    ref = orc.solve(d, orc.default_opts(**c["opts"]))
    assert ref["status"] == 0
    for name, s in SCL.mpc_scalings(c):
        terms = MC.fold(SCL.map_root_terms(c["root"], c["d"], s), SCL.map_x0(x0, s))
        ds = MC.folded(dict(c, d=SCL.scaled(c["d"], s)), terms)
        for k in ("A", "B", "b", "Qd", "Rd", "q", "r", "xmin", "xmax", "umin", "umax"):
            assert np.array_equal(ds[k], SCL.scaled(d, s)[k]), (cid, name, k)          # folding and scaling commute exactly
        got = orc.solve(ds, orc.default_opts(**SCL.scaled_opts(c["opts"], s)))
        _same_run(ref, got, s, (cid, name))


# ---- the references of the stage solver with rows, of the sensitivities and of the adjoints ----

@pytest.mark.parametrize("rid", ["per_phase-gen", "per_phase-box", "single_wg-dense", "fused_tails-dense"])
def test_dense_rows_have_an_equivariant_reference_step(capi, rid):
    """The oracle does not solve trees with box or general stage constraints: for the dense rows of test_gpu_scale.py gen_ref / newton_ref
    stand in.  One Newton step at the row's starting duals under the per-entry scaling the device test uses (row scales included):
    the mapped step within XCHECK_TOL of the largest entry, the same active bounds and rows on every node."""
    import gen_ref as G
    pr = SCL.problem(rid, capi)
    d, lam0, kinds = pr["d"], pr["lam0"], pr["kinds"]
    step = (lambda dd, ll: G.newton_step(dd, ll, kinds)) if pr.get("gen") else (lambda dd, ll: N.newton_step(dd, ll, pr["dense"], kinds))
    base = step(d, lam0)
    for i in range(2):
        s = SCL.entry_scaling(d, i)
        got = step(SCL.scaled(d, s), SCL.map_lam(lam0, s))
        e = _rel(SCL.map_lam(got["dlam"], s, -1), base["dlam"])
        print(f"{rid} scaling {i}: dlam {e:.2e}")
        assert e <= R.XCHECK_TOL * max(1.0, base.get("cond", 1.0) * 1e-3)
        if pr.get("gen"):
            st0, st1 = G.stage_solutions(d, lam0, kinds), G.stage_solutions(SCL.scaled(d, s), SCL.map_lam(lam0, s), kinds)
            names = ("mu_x", "mu_u", "mu_d")
            m0, m1 = dict(zip(names, G.flat_multipliers(d, st0))), dict(zip(names, G.flat_multipliers(SCL.scaled(d, s), st1)))
            back = SCL.map_solution(m1, s, -1)
            for k in names:
                if True:
                    assert np.array_equal(np.asarray(m0[k]) != 0, np.asarray(back[k]) != 0), (rid, k)
                    assert _rel(back[k], m0[k]) <= R.XCHECK_TOL, (rid, k)


SENS_REF_IDS = ("elim-single_wg", "elim-persist_c1", "elim-three_children", "elim-dense_kind1_root", "states-generic", "states-persist_c1", "states-tiered_ub")


@pytest.mark.parametrize("cid", SENS_REF_IDS)
def test_sensitivity_and_adjoint_references_on_scaled_problems(orc, cid):
    """sens_ref.dual_form, adj_ref.dual_form and adjmat_ref.outer (the block forms the device tests are held to) at the oracle's point of
    the scaled problem against their mapped unscaled results, within sens_cases.tol / adj_cases.tol / adjmat_cases.tol.
    (The dense forms, dense_kkt, solve one KKT matrix by lstsq, which drops singular values below eps times the largest: on a matrix
    whose blocks carry other units that removes real directions -- measured here on these cases under s = 12, t = -9, a = 20:
    differences of 0.1 to 1e3 in dx, du, dlam, gq, gr, gb, gx0.  They hold the block forms on unscaled problems in test_sens_reference.py
    and test_adj_reference.py; on scaled problems the block forms stand alone.)"""
    import adj_cases as AC
    import adj_ref as AR
    import adjmat_cases as XC
    import adjmat_ref as AM
    import sens_cases as SN
    import sens_ref as SR
    c = AC.case(cid)
    sol = SN.oracle_solve(orc, c)
    reg = SCL.reg_of(c["base"]["opts"])
    b = SR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["kinds"], **reg)
    g = AR.dual_form(c["d"], sol["x"], sol["u"], c["param"], c["w"], c["kinds"], **reg)
    hg, cg = XC.maps(c, "shared")
    maps = XC.filled(c, hg, cg)
    m = AM.outer(c["d"], sol["x"], sol["u"], sol["lam"], c["param"], g, c["kinds"], maps[0], maps[1], c["x0"], 0)
    for name, s in SCL.case_scalings(c):
        cs = SCL.scaled_sens_case(c, s)
        ss = SCL.map_solution({k: sol[k] for k in ("x", "u", "lam")}, s)
        regs = SCL.reg_of(c["base"]["opts"], s)
        b2 = SR.dual_form(cs["d"], ss["x"], ss["u"], cs["param"], cs["kinds"], **regs)
        back = dict(SCL.map_sensitivities({k: b2[k] for k in ("dx", "du", "dlam")}, s, -1), K=SCL.map_gain(b2["K"], s, c["d"], -1))
        for k in ("K", "dx", "du", "dlam"):
            e = float(np.max(np.abs(back[k] - b[k]), initial=0.0))
            print(f"{cid} {name} {k}: {e:.2e}")
            assert e <= SN.tol(cid, k), (cid, name, k, e)
        g2 = AR.dual_form(cs["d"], ss["x"], ss["u"], cs["param"], cs["w"], cs["kinds"], **regs)
        assert g2["n_reg"] == g["n_reg"]
        gb = SCL.map_adjoint({k: g2[k] for k in ("gq", "gr", "gb", "gx0")}, s, -1)
        for k in gb:
            e = float(np.max(np.abs(gb[k] - g[k]), initial=0.0))
            print(f"{cid} {name} {k}: {e:.2e}")
            assert e <= AC.tol(cid, k), (cid, name, k, e)
        m2 = AM.outer(cs["d"], ss["x"], ss["u"], ss["lam"], cs["param"], g2, cs["kinds"], maps[0], maps[1], cs["x0"], 0)
        mb = SCL.map_adjoint_matrices(m2, s, c["d"], SCL.group_dims(c["d"], maps[0], 0), -1)
        for k in AM.KEYS:
            assert len(mb[k]) == len(m[k]), k
            for i, (x, y) in enumerate(zip(mb[k], m[k])):
                e = float(np.max(np.abs(x - y), initial=0.0))
                assert e <= XC.tol(cid, k), (cid, name, k, i, e)

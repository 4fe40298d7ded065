"""The oracle's trace of the termination norm and of the dual value held to trace_ref.py, iteration by iteration, on every clipping
row of trace_cases.py (the oracle models no other stage solver) and under the three norms -- with exactly the bounds the device is
held to in test_gpu_result_fields.py.  It shows that the reference alone stays inside the bounds, and that the bounds are small
next to what they guard: below 1e-6 of every value compared before convergence.

trace_err[i] belongs to the dual point at the start of iteration i: the lam the oracle returns with maxIter = i (lambda0 for
i = 0).  trace_fval[i] belongs to the point after iteration i."""
from __future__ import annotations

import numpy as np
import pytest

import trace_cases as TC
import trace_ref as R

RATIO = {t: 0.0 for t in TC.NORMS}
RATIO_F = [0.0]
SMALL = 1e-6


@pytest.fixture(scope="module")
def entries():
    cache = {}

    def get(rid, pr, lam):
        key = (rid, np.asarray(lam, float).tobytes())
        if key not in cache:
            cache[key] = (R.residual_at(pr["d"], lam), R.dual_value_with_scale(pr["d"], lam))
        return cache[key]
    return get


def _starts(r, pr):
    return [TC.member_duals(pr, i) for i in range(2 if r["batch"] else 1)]


@pytest.mark.parametrize("term", TC.NORMS)
@pytest.mark.parametrize("rid", TC.CLIP_IDS)
def test_oracle_trace_is_the_reference(orc, capi, entries, rid, term):
    r = TC.row(rid)
    pr = TC.problem(rid, capi)
    d = pr["d"]
    opts = {k: v for k, v in TC.solve_opts(r, term).items() if k != "checkLastActiveSet" or v != 2}      # (2 is a device variant: the oracle has 0 / 1)
    tol = TC.TOL_OF[term]
    for lam0 in _starts(r, pr):
        full = orc.solve(d, orc.default_opts(**opts), lambda0=lam0)
        n = full["iter"]
        assert full["status"] == 0 and n >= (2 if lam0 is pr["lam0"] else 1), (rid, full["status"], n)
        if r["backtracks"]:
            assert full["ls_total"] > n
        lams = [lam0] + [orc.solve(d, orc.default_opts(**dict(opts, maxIter=i)), lambda0=lam0)["lam"] for i in range(1, n + 1)]
        assert np.array_equal(lams[n], full["lam"])
        for i in range(n + 1):
            ent, (fv, Tf) = entries(rid, pr, lams[i])
            val, T, _ = R.norm_of(ent, term)
            bnd = R.bound_err(d, term, T, at=True)
            e = abs(float(full["trace_err"][i]) - float(val))
            RATIO[term] = max(RATIO[term], e / bnd)
            assert e <= bnd, (rid, term, i, float(full["trace_err"][i]), float(val), bnd)
            if full["trace_err"][i] >= tol:
                assert bnd < SMALL * float(val), (rid, term, i, "the bound is no longer small next to the norm", bnd, float(val))
            else:
                assert i == n
            if i >= 1:
                bf = R.bound_fval(d, Tf)
                e = abs(float(full["trace_fval"][i - 1]) - float(fv))
                RATIO_F[0] = max(RATIO_F[0], e / bf)
                assert e <= bf, (rid, term, i, float(full["trace_fval"][i - 1]), float(fv), bf)
                assert bf < SMALL * abs(float(fv)), (rid, term, i, "the bound is no longer small next to the dual value", bf, float(fv))
    print(f"{rid} norm {term}: iter {n}, largest error / bound so far: err {RATIO[term]:.3f}, fval {RATIO_F[0]:.3f}")


@pytest.mark.parametrize("rid", [i for i in TC.ROW_IDS if i not in TC.CLIP_IDS])
def test_bounds_of_the_dense_rows_are_small(capi, rid):
    """The rows the oracle does not model (dense, box-constrained and general-constraint nodes): the iterates of the numpy Newton
    method itself (newton_ref / gen_ref: step, Armijo trials) from the row's starting duals, under the row's options.  At every
    iterate before convergence the bounds are below 1e-6 of the norm and of the dual value, as on the clipping rows; a row that is
    not `quadratic` takes at least two iterations."""
    import box_cases as BC
    import gen_ref as G
    import newton_ref as N
    r, pr = TC.row(rid), TC.problem(rid, capi)
    d, kinds, dense, gen = pr["d"], pr["kinds"], pr["dense"], pr.get("gen")
    reg = r["opts"].get("regValue", 0.0) if r["opts"].get("regType") == 1 else 0.0
    lam = np.array(pr["lam0"], dtype=float)
    done = {t: None for t in TC.NORMS}
    for it in range(12):
        step = G.newton_step(d, lam, kinds, reg=reg) if gen else N.newton_step(d, lam, dense, kinds, reg=reg)
        st = step["stages"]
        ent = R.residual_at(d, lam, kinds, dense, st if gen else None)
        for t in TC.NORMS:
            val, T, _ = R.norm_of(ent, t)
            if done[t] is None and float(val) < TC.TOL_OF[t]:
                done[t] = it
            if done[t] is None:
                bnd = R.bound_err(d, t, T, at=True, kinds=kinds, dense=dense)
                assert bnd < SMALL * float(val), (rid, t, it, bnd, float(val))
        if all(v is not None for v in done.values()):
            break
        trials, _ = (G.armijo_trials(d, lam, step["dlam"], step["res"], BC.LsOpts, kinds) if gen
                     else N.armijo_trials(d, lam, step["dlam"], step["res"], BC.LsOpts, kinds, dense))
        lam = lam + BC.OPTS["lineSearchBeta"] ** (trials - 1) * step["dlam"]
        fv, Tf = R.dual_value_with_scale(d, lam, kinds, dense, G.stage_solutions(d, lam, kinds) if gen else None)
        bf = R.bound_fval(d, Tf)
        assert bf < SMALL * abs(float(fv)), (rid, it, bf, float(fv))
    print(f"{rid}: iterations until each norm is below its tolerance {done}")
    assert all(v is not None for v in done.values()), (rid, done)
    assert all(v == 1 for v in done.values()) if r["quadratic"] else all(v >= 2 for v in done.values()), (rid, done)


def test_largest_ratios_are_printed():
    """(runs last in the module: the figures of a whole run)"""
    for t in TC.NORMS:
        print(f"norm {t}: largest |oracle - reference| / bound of trace_err = {RATIO[t]:.3f}")
    print(f"largest |oracle - reference| / bound of trace_fval = {RATIO_F[0]:.3f}")
    assert all(v <= 1.0 for v in RATIO.values()) and RATIO_F[0] <= 1.0

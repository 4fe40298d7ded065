"""The rows of clip_cases.py are what they claim, checked on the CPU before any device run compares with them: the tied stage
values are ties exactly (rational arithmetic, and float64 sums in both orders), their neighbours one unit in the last place away
fall on the stated sides, every other entry keeps the margin of reg_cases.py, the Newton system is well conditioned and no block
is flagged, the CPU oracle takes the reference's step and active set, and -- the point of the table -- the step under the
exclusive rule (`>` for `>=`) differs from the reference step by at least 1e4 times the tolerance of the device pin, for the
whole row, for its upper ties alone, its lower ties alone, its equal bounds alone and every single placement alone."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import clip_cases as CC
import newton_ref as N
import reg_cases as RC
import reg_ref as R
from box_cases import SLACK_MIN
from helpers import rel_err

KEYS = {}
for _r in CC.ROWS:
    KEYS.setdefault(_r.key, _r)
UNIQUE = [r.id for r in KEYS.values()]           # rows of several routes share one problem: checked once


def _bounds(d, k):
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    return (np.concatenate([d["xmin"][xo[k]:xo[k + 1]], d["umin"][uo[k]:uo[k + 1]]]), np.concatenate([d["xmax"][xo[k]:xo[k + 1]], d["umax"][uo[k]:uo[k + 1]]]))


def _check_conditions(rid, c):
    ref = c["ref"]
    print(f"{rid}: cond {ref['cond']:.3g} guard {ref['guard']:.3g} margin of the untied entries {c['margin']:.3g} xcheck {ref['xcheck']:.1e} "
          f"trials {c['trials']} slack {c['slack']:.1e}" + (" (trial count pinned)" if c["slack"] >= SLACK_MIN else " (trial count not pinned)"))
    assert ref["cond"] <= CC.COND_MAX
    assert ref["flagged"] == [] and ref["guard"] >= RC.GUARD_MIN
    assert c["margin"] > CC.GAP
    assert ref["xcheck"] <= R.XCHECK_TOL


def _check_discrimination(rid, c, groups):
    print(f"{rid}: step under the exclusive rule moves by " + ", ".join(f"{k} {v:.1e}" for k, v in c["moved"].items()))
    assert set(c["moved"]) == {"all"} | set(groups)
    for name, v in c["moved"].items():
        assert v >= CC.DISCRIMINATION, name


def _check_oracle(orc, c):
    ref = c["ref"]
    opts = orc.default_opts(maxIter=1, **CC.OPTS)
    got = orc.solve(c["d"], opts, c["lam0"])
    assert (got["status"], got["iter"], got["n_regularized"]) == (1, 1, 0)
    trials = int(got["trace_ls"][0])
    if c["slack"] >= SLACK_MIN:
        assert trials == c["trials"]
    assert rel_err(got["lam"], c["lam0"] + opts.lineSearchBeta ** (trials - 1) * ref["dlam"]) <= CC.TOL
    # its active set at lambda0, as a COUNT (the entries with a zero weight after phase S of the one iteration; the oracle exports x and
    # u at the accepted trial point, not at lambda0, so the entries cannot be compared one by one): the reference's number.  That the
    # sets are equal entry for entry follows only indirectly, from the step above and the discrimination of every single placement.
    assert got["n_active"] == sum(int(np.sum(s != 0)) for s in ref["stages"]["side"])
    full = orc.solve(c["d"], orc.default_opts(**CC.OPTS), c["lam0"])
    assert full["status"] == 0, "the tied QP must stay feasible: the device tests solve it to the end"
    return full


@pytest.mark.parametrize("rid", UNIQUE)
def test_row_is_what_it_claims(orc, rid):
    r = CC.row(rid)
    c = CC.case(rid)
    d, lam0, ref = c["d"], c["lam0"], c["ref"]
    # (a) exactness
    worst, fr, fw, rv = CC.exactness(d, lam0)
    assert worst < 2.0 ** (53 - CC.K)
    zu = CC.unconstrained(d, lam0)
    for p in range(len(fr)):
        assert all(Fraction(float(a)) == b for a, b in zip(fw[p], fr[p])), p
        assert np.array_equal(fw[p], rv[p]) and np.array_equal(fw[p], zu[p]), p
    sides = ref["stages"]["side"]
    for k, e, mode, far in r.ties:
        e = e % len(zu[k])
        lo, hi = _bounds(d, k)
        v = Fraction(float(zu[k][e]))
        assert fr[k][e] == v
        if mode in ("ub", "ub0", "eq"):
            assert Fraction(float(hi[e])) == v
        if mode in ("lb", "lb0", "eq"):
            assert Fraction(float(lo[e])) == v
        if mode.endswith("0"):
            assert v == 0
        if mode == "ub_in":
            assert hi[e] > zu[k][e] and np.nextafter(hi[e], -np.inf) == zu[k][e]
        if mode == "ub_out":
            assert hi[e] < zu[k][e] and np.nextafter(hi[e], np.inf) == zu[k][e]
        if mode == "lb_in":
            assert lo[e] < zu[k][e] and np.nextafter(lo[e], np.inf) == zu[k][e]
        if mode == "lb_out":
            assert lo[e] > zu[k][e] and np.nextafter(lo[e], -np.inf) == zu[k][e]
        if r.kinds is None or r.kinds[k] == 0:
            assert (sides[k][e] != 0) == (mode in CC.FIXED), (k, e, mode)
            assert float(ref["stages"]["P"][k][e, e]) == (0.0 if mode in CC.FIXED else 1.0 / N._blocks(d, False)[-1][k][e])
        other = lo[e] if mode.startswith("ub") else hi[e]
        if mode != "eq":
            assert abs(other) == {"wide": 5.0 + abs(zu[k][e]), "inf": np.inf, "INF": N.P.INF}[far]
    if r.kinds is not None:
        assert all(r.kinds[k] == 0 for k, _, _, _ in r.ties) and set(r.kinds) == {0, 1}
    # (b) conditions, (d) discrimination, (e) the slack of the line search
    _check_conditions(rid, c)
    _check_discrimination(rid, c, r.groups())
    # (c) the oracle (clipping trees; it has no mixed kinds)
    if r.kinds is None:
        _check_oracle(orc, c)


@pytest.mark.parametrize("tree", sorted({t for _, t in CC.COLD.values()}))
def test_cold_start_row(orc, tree):
    """umin = 0, r = 0, lambda0 = 0: every input of the spring-mass tree ties on its lower bound in the first iteration"""
    c = CC.cold_case(orc, tree)
    d, ref = c["d"], c["ref"]
    assert not np.any(c["lam0"]) and not np.any(d["r"]) and not np.any(d["umin"]) and int(d["nu"].sum()) == len(c["ties"]) > 0
    for k, e, mode, far in c["ties"]:
        terms = CC.h_terms(d, c["lam0"])[k][e]
        assert sum((Fraction(v) for v in terms), Fraction(0)) == 0 and all(v == 0 for v in terms)
        assert ref["stages"]["side"][k][e] == -1 and float(ref["stages"]["P"][k][e, e]) == 0.0
    x0 = d["xmin"][:d["nx"][0]]
    assert np.array_equal(x0 * 4, np.round(x0 * 4)) and np.array_equal(x0, d["xmax"][:d["nx"][0]])
    _check_conditions("cold_start", c)
    _check_discrimination("cold_start", c, {"lower": None})
    full = _check_oracle(orc, c)
    assert full["iter"] >= 2


def test_every_route_and_placement_has_its_rows():
    by_route = {}
    for r in CC.ROWS:
        by_route.setdefault(r.route, []).append(r)
    has = lambda route, problem: any(r.problem == problem for r in by_route[route])
    assert set(by_route) == set(CC.ROUTES) - {"dense_single"} - {r for r, _ in CC.COLD.values() if r.endswith("_cold")}
    assert {r for r, _ in CC.COLD.values()} == {"generic", "gpersist_cold", "gpersist_sweep1_cold", "tiered", "persist_one", "persist_two"}
    assert has("generic", "tree") and has("generic", "gtree") and len(CC.dims("gtree")[0]) > 64
    assert has("gpersist", "tree") and has("gpersist", "gtree") and has("gpersist_sweep1", "tree")
    assert has("tiered", "u3") and has("tiered", "u6") and has("persist_one", "u6") and has("persist_two", "u6")
    assert has("wide", "wtree") and has("wide3", "wtree") and has("mixed", "tree")
    assert all(len(CC.dims(r.problem)[0]) <= len(CC.dims("u6")[0]) for r in CC.ROWS)
    for r in CC.ROWS:
        nk, nx, nu = CC.dims(r.problem)
        dad = N.P.parents_of(nk)
        ex = [(k, e % (nx[k] + nu[k]), m) for k, e, m, _ in r.ties if m in CC.EXACT]
        if r.id == "gpersist-tree-quarters":
            # one tie in each quarter of a wave of the packed sweep (node k on quarter k % 4), first and last group
            assert {k % 4 for k, _, _ in ex if k < 4} == {0, 1, 2, 3} and {k % 4 for k, _, _ in ex if 4 <= k < 28} == {0, 1, 2, 3}
            assert {k for k, _, _ in ex if k >= 28} == {28, 29, 30}
            continue
        # first and last entry of a node's [x | u] and both sides of the x / u boundary are tied somewhere in the row, and the row
        # has ties from above and from below (test_row_is_what_it_claims holds each of them to the discrimination bound alone)
        for what, test in (("first entry", lambda k, e: e == 0), ("last entry", lambda k, e: e == nx[k] + nu[k] - 1),
                           ("last state", lambda k, e: e == nx[k] - 1 and nu[k] > 0), ("first input", lambda k, e: e == nx[k] and nu[k] > 0)):
            assert any(test(k, e) for k, e, m in ex), (r.id, what)
        assert any(m in CC.UPPER for _, _, m in ex) and any(m in CC.LOWER for _, _, m in ex), r.id
        nodes = {k for k, _, _ in ex}
        assert 0 in nodes and any(nk[k] == 0 for k in nodes) and any(k > 0 and nk[k] > 0 for k in nodes), r.id
        assert {m for _, _, m, _ in r.ties} >= {"ub", "lb", "eq", "ub0", "lb0", "ub_in", "ub_out", "lb_in", "lb_out"}, r.id
        assert {f for _, _, _, f in r.ties} == {"wide", "inf", "INF"}, r.id
        if r.problem == "u6":
            depth = lambda k: int(np.floor(np.log2(k + 1)))
            assert {2, 3} <= {depth(k) for k in nodes}          # last level of the top tier, first level of the bottom tier
    assert CC.BATCH_IDS == ["persist_one-u6", "gpersist-tree", "wide3-wtree"] and all(b in CC.ROW_IDS for b in CC.BATCH_IDS)


@pytest.mark.parametrize("name", ["u3", "u6"])
def test_trial_point_row_is_what_it_claims(orc, name):
    """the rows with a tie at the accepted trial point lambda1 = lambda0 + dlam (clip_cases.trial_case): lambda1 and unc(lambda1) are
    exact, the ties are ties there and not at lambda0, the oracle accepts the full step and its second iteration takes the reference's
    step at lambda1, and that step moves under the exclusive rule, for every tie alone"""
    c = CC.trial_case(name)
    d, lam0, lam1, ref2 = c["d"], c["lam0"], c["lam1"], c["ref2"]
    for lam in (lam0, lam1):
        worst, fr, fw, rv = CC.exactness(d, lam, CC.TRIAL_K)
        assert worst < 2.0 ** (53 - CC.TRIAL_K)
        for p in range(len(fr)):
            assert all(Fraction(float(a)) == b for a, b in zip(fw[p], fr[p])) and np.array_equal(fw[p], rv[p]), p
    z0, z1 = CC.unconstrained(d, lam0), CC.unconstrained(d, lam1)
    s1, s2 = c["ref1"]["stages"]["side"], ref2["stages"]["side"]
    assert len(c["ties"]) == len(CC.TRIAL_PARENTS[name]) and {s for _, _, s in c["ties"]} == {-1, 1}
    for k, e, side in c["ties"]:
        lo, hi = _bounds(d, k)
        assert Fraction(float((hi if side > 0 else lo)[e])) == Fraction(float(z1[k][e])) and s1[k][e] == 0 and s2[k][e] != 0
        assert abs(z0[k][e] - z1[k][e]) > 1e-2
    assert not np.any(s1[0][d["nx"][0]:]) and all(not np.any(s) for s in s1[1:])          # but for x0 nothing is fixed at lambda0: M = I, dlam = res
    print(f"{name}: cond at lambda1 {ref2['cond']:.3g} margin {c['margin']:.3g} trials of the second step {c['trials2']} slack {c['slack2']:.1e}; "
          "the second step under the exclusive rule moves by " + ", ".join(f"{k} {v:.1e}" for k, v in c["moved"].items()))
    assert ref2["cond"] <= CC.COND_MAX and ref2["flagged"] == [] and c["ref1"]["flagged"] == [] and ref2["xcheck"] <= R.XCHECK_TOL
    assert c["margin"] > CC.GAP
    assert all(v >= CC.DISCRIMINATION for v in c["moved"].values())
    one = orc.solve(d, orc.default_opts(maxIter=1, **CC.OPTS), lam0)
    assert int(one["trace_ls"][0]) == 1 and np.array_equal(one["lam"], lam1)
    two = orc.solve(d, orc.default_opts(maxIter=2, **CC.OPTS), lam0)
    t2 = int(two["trace_ls"][1])
    assert (two["status"], two["iter"], two["n_regularized"]) == (1, 2, 0)
    if c["slack2"] >= SLACK_MIN:
        assert t2 == c["trials2"]
    assert rel_err(two["lam"], lam1 + RC.BETA ** (t2 - 1) * ref2["dlam"]) <= CC.TOL
    assert two["n_active"] == sum(int(np.sum(s != 0)) for s in s2)          # (a count: see _check_oracle)


def test_sensitivity_case_is_what_it_claims(orc):
    """clip_cases.sens_case: lambda0 is the solution exactly (a solve from it takes no iteration), the tied entries sit on their bounds
    there, the two numpy evaluations of the sensitivities agree, the tied root input has a zero row of du0/dx0, and with the tied
    entries free (the twin) du0/dx0 is another matrix"""
    import sens_ref as SR
    c = CC.sens_case()
    d = c["d"]
    got = orc.solve(d, orc.default_opts(**CC.OPTS), c["lam0"])
    assert (got["status"], got["iter"]) == (0, 0) and np.array_equal(got["x"], c["x"]) and np.array_equal(got["u"], c["u"])
    on = SR.pinned(d, c["x"], c["u"])
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    for k, e, mode, far in c["ties"]:
        isx, i, _ = CC._slot(d, k, e)
        assert on[i if isx else len(c["x"]) + i]
    a, b = SR.dense_kkt(d, c["x"], c["u"], dict(form="states")), SR.dual_form(d, c["x"], c["u"], dict(form="states"), **CC.OPTS)
    assert a["residual"] < 1e-9 * a["scale"] and b["n_reg"] == 0 and c["cond"] <= CC.COND_MAX
    spread = max(float(np.max(np.abs(a[w] - b[w]))) for w in ("K", "dx", "du"))
    free = SR.dense_kkt(c["twin"], c["x"], c["u"], dict(form="states"))
    print(f"sens: spread of the two numpy evaluations {spread:.2e}; K with the ties free differs by {np.max(np.abs(free['K'] - a['K'])):.2e}")
    assert spread <= 1e-12
    assert np.all(b["K"][0] == 0.0) and np.max(np.abs(a["K"][0])) <= 1e-12 and np.any(a["K"][1] != 0.0)          # (a) is a lstsq: zero to rounding
    assert np.max(np.abs(free["K"] - a["K"])) >= CC.DISCRIMINATION and np.max(np.abs(free["K"][0])) >= CC.DISCRIMINATION

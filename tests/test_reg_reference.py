"""The rows of reg_cases.py are what they claim, checked on the CPU before any device run compares with them, and the CPU oracle's
regularised factorisation (its potrf_with_reg, which no golden file reaches) is the one of reg_ref.py: the reference flags
exactly the blocks a row names, every first-pass pivot is a factor 1.9 away from regTol or exactly 0, the stage values are 1e-6
away from their clipping thresholds, cond(M + shifts) <= 1e6 (the rule of test_box_reference.py for a 1e-10 pin; DEFAULTS rows
are measured instead, see reg_cases.py), the block substitution agrees with a dense solve to 1e-13, and the
oracle's count of regularised blocks, its trial count and its first iterate are the reference's."""
from __future__ import annotations

import numpy as np
import pytest

import reg_cases as RC
import reg_ref as R
from helpers import rel_err

KEYS = {}
for _r in RC.ROWS:
    KEYS.setdefault(_r.key, _r)
UNIQUE = list(KEYS.values())          # rows of several routes share one problem, pins and options: checked once


@pytest.mark.parametrize("rid", [r.id for r in UNIQUE])
def test_row_is_what_it_claims(orc, rid):
    r = RC.row(rid)
    c = RC.case(rid)
    ref = c["ref"]
    print(f"{rid}: seed {c['seed']} flagged {sorted(ref['flagged'])[:8]} guard {ref['guard']:.3g} cond {ref['cond']:.3g} "
          f"margin {ref['margin']:.3g} xcheck {ref['xcheck']:.1e} trials {c['trials']} slack {c['slack']:.1e}")
    assert sorted(ref["flagged"]) == r.flagged
    assert ref["guard"] >= RC.GUARD_MIN
    assert ref["margin"] > RC.GAP
    assert ref["xcheck"] <= R.XCHECK_TOL
    if r.opts is RC.DEFAULTS and ref["cond"] > RC.COND_MAX:
        spread = RC.float64_spread(c["d"], c["lam0"], r.opts)
        print(f"{rid}: spread of the float64 reference step under 1-ulp perturbations of the data {spread:.2e}")
        assert 10.0 * spread <= RC.TOL
    else:
        assert ref["cond"] <= RC.COND_MAX
    if r.kind.startswith("threshold"):
        first = ref["pivots"][3]["first"]
        want = 0.5e-3 if r.kind == "threshold_below" else 2e-3
        assert len(first) == 1 and abs(first[0] / want - 1) < 1e-12
    if r.kind == "rounding_pivot":
        first = ref["pivots"][3]["first"]
        assert len(first) == 2 and first[0] > 1e-2 and abs(first[1]) < 1e-6
    if r.kind == "zero_column":
        assert np.any(ref["zero"]) and np.all(ref["dlam"][ref["zero"]] == 0)
    if r.lift:
        assert c["free"]["flagged"] == [] and rel_err(c["free"]["dlam"], ref["dlam"]) > 1e-3
    # the oracle: as many regularised blocks, the reference's first iterate
    opts = orc.default_opts(maxIter=1, **r.opts)
    got = orc.solve(c["d"], opts, c["lam0"])
    assert got["status"] == 1 and got["iter"] == 1
    assert got["n_regularized"] == len(ref["flagged"])
    trials = int(got["trace_ls"][0])
    if c["slack"] >= 1e-9:
        assert trials == c["trials"]
    assert rel_err(got["lam"], c["lam0"] + opts.lineSearchBeta ** (trials - 1) * ref["dlam"]) <= 1e-12


def test_every_route_has_its_rows():
    kinds = {}
    for r in RC.ROWS:
        kinds.setdefault(r.route, set()).add((r.kind, r.problem))
    has = lambda route, kind, problem=None: any(k == kind and problem in (None, q) for k, q in kinds[route])
    assert set(kinds) == set(RC.ROUTES) == set(RC.MAPPING)
    common = ("flag_leaf_level", "flag_mid_level", "flag_root", "neighbours", "always", "zero_column", "defaults")
    for route in ("generic", "gpersist", "wide", "wide3"):
        for kind in common + ("threshold_below", "threshold_above", "rounding_pivot"):
            assert has(route, kind), (route, kind)
    for route in ("wide", "wide3"):
        assert sum(k == "flag_position" for k, _ in kinds[route]) == 3      # fan88 (three children), d17, fan_last1
        assert {q for k, q in kinds[route] if k == "flag_position"} == {"fan88", "d17", "fan_last1"}
    for route in ("tiered", "persist_one", "persist_two"):
        for kind in common + ("flag_upper_tier",):
            assert has(route, kind, "u6"), (route, kind)
    assert has("persist_one", "flag_root", "u3") and has("persist_one", "flag_upper_tier", "u7") and has("tiered", "flag_upper_tier", "u7")
    assert has("gpersist", "neighbours", "gtree") and has("dense_single", "flag_mid_level")
    assert all(r.lift == (r.kind == "flag_mid_level") for r in RC.ROWS)


def test_tiers_and_groups_are_where_the_rows_say():
    """the structure the uniform and grouped rows rely on, counted on the trees: three block levels to a tier of a binary tree
    (Uni::TH), groups on a level of more than 16 equal blocks with d + 1 + nx <= 21"""
    depth = lambda k: int(np.floor(np.log2(k + 1)))
    assert {n: -(-h // 3) for n, h in RC.UNIFORM.items()} == {"u3": 1, "u6": 2, "u7": 3}
    assert (depth(31), depth(15), depth(3)) == (5, 4, 2) and 6 - 3 == 3          # u6: bottom tier from level 3, level 2 tops the upper tier
    assert depth(7) == 3 and 7 - 3 == 4                                          # u7: tiers 4..6 | 1..3 | 0
    d = RC.base_problem("gtree")
    nk, nx = d["nk"], d["nx"]
    assert list(nk[22:46]) == [2] * 24 and list(nx[22:46]) == [3] * 24 and list(nx[46:]) == [2] * 48 and 4 + 1 + 3 <= 21


def test_shifting_one_column_only_would_show():
    """what the device pin can see: on a flagged row, the step with only the zero pivot's own diagonal entries shifted differs
    from the reference step by far more than the pin's tolerance"""
    c = RC.case("generic-flag_mid_level")
    ref = c["ref"]
    M, res, _ = R.N.assemble(c["d"], c["lam0"])
    zero_rows = np.flatnonzero((np.abs(M).sum(axis=1) == 0))
    assert len(zero_rows) == 3
    sh = np.zeros(len(res))
    sh[zero_rows] = RC.OTF["regValue"]
    wrong = np.linalg.solve((M + np.diag(sh)).astype(np.float64), res.astype(np.float64))
    assert rel_err(wrong, ref["dlam"]) > 1e-4

"""The reference of the stage solver for general constraints (gen_ref.py) and its case table (gen_cases.py), checked without a
device: every row certifies and meets its guards, small stage QPs agree with the enumeration of all working sets, a problem whose
rows are loose gives newton_ref's kind-2 step, and the container's own KKT residual vanishes on a converged reference solve (which
fixes the sign of mu_d against tree_qp_out_max_KKT_res)."""
from __future__ import annotations

import numpy as np
import pytest

import gen_cases as GC
import gen_ref as G
import newton_ref as N


@pytest.mark.parametrize("rid", GC.ROW_IDS)
def test_row_certifies_and_meets_its_guards(rid):
    c = GC.case(rid)
    ref = c["ref"]
    print(f"{rid}: seed {c['seed']} cond {ref['cond']:.2e} condS {ref['condS']:.2e} margin {ref['margin']:.2e} cert {ref['cert']:.2e} "
          f"trials {c['trials']} slack {c['slack']:.2e} xu_pin {c['xu_pin']}")
    assert ref["cert"] <= N.CERT_TOL
    assert ref["margin"] >= GC.GAP and ref["cond"] <= GC.COND_MAX and ref["condS"] <= GC.COND_MAX
    assert any(np.any(s != 0) for s in ref["stages"]["rside"]), "no row is active at lambda0"


@pytest.mark.parametrize("rid", GC.ROW_IDS)
def test_enumeration_agrees_on_small_nodes(rid):
    c = GC.case(rid)
    st = c["ref"]["stages"]
    cons = G.cons_of(c["d"])
    _, H, hs, los, his = N.stage_data(c["d"], c["lam0"], kinds=G._kinds2(c["kinds"]))
    n = 0
    for k in np.flatnonzero(c["kinds"] == 3):
        if cons[k] is None or len(hs[k]) + len(cons[k][1]) > 8:
            continue
        found = G.enumerate_gen(H[k], hs[k], los[k], his[k], *cons[k])
        assert len(found) >= 1
        for z, sb, sr, mu in found:          # one KKT point: every working set that passes describes it
            assert np.max(np.abs((z - st["z"][k]).astype(float))) <= 1e-9
        assert any(np.array_equal(sb, st["side"][k]) and np.array_equal(sr, st["rside"][k]) for _, sb, sr, _ in found)
        n += 1
    if rid in ("one_row", "row_and_bound", "more_rows_than_vars", "equality_row", "leaf_rows", "mixed", "x0_elim"):
        assert n >= 1


@pytest.mark.parametrize("rid", ["one_row", "nc64", "mixed"])
def test_loose_rows_give_the_box_step(rid):
    d, kinds, lam0, _ = GC.loose_case(rid)
    a = G.newton_step(d, lam0, kinds)
    b = N.newton_step(d, lam0, kinds=G._kinds2(kinds))
    assert not any(np.any(s != 0) for s in a["stages"]["rside"])
    assert np.max(np.abs(a["dlam"] - b["dlam"])) <= 1e-13 * max(1.0, np.max(np.abs(b["dlam"])))
    for za, zb in zip(a["stages"]["z"], b["stages"]["z"]):
        assert np.max(np.abs((za - zb).astype(float)), initial=0.0) <= 1e-13


@pytest.mark.parametrize("rid", GC.FULL_IDS)
def test_container_kkt_residual_of_the_reference_solution(capi, rid):
    c = GC.case(rid)
    d, kinds = c["d"], c["kinds"]
    it, trials, err, lam, _ = GC.reference_solve(d, kinds, tol=1e-10)
    assert err <= 1e-10
    st = G.stage_solutions(d, lam, kinds)
    x, u, _, _ = N.flat_xu(st)
    mx, mu, md = G.flat_multipliers(d, st)
    qp = GC.container_of(capi, d)
    qp.set_solution(dict(x=x, u=u, lam=lam, mu_x=mx, mu_u=mu, mu_d=md))
    kkt = qp.max_kkt_res()
    print(f"{rid}: {it} iterations, {trials} trials, residual {err:.2e}, container KKT {kkt:.2e}")
    assert kkt < 1e-9


@pytest.mark.parametrize("rid", GC.FULL_IDS)
def test_whole_solves_have_clear_decisions(rid):
    lam, sol = GC.full_start(rid)
    print(f"{rid}: {sol[0]} iterations, {sol[1]} trials, residual {sol[2]:.2e}, guard {sol[4]}")
    assert GC.qualifies(sol)

"""The hot start of the stage solver for general constraints, checked without a device: gen_hot_ref.solve_gen_from (sanitise, dual-
feasibility rounds, then the dual active-set loop, one cold redo) against gen_ref's cold solve and its longdouble certificate on
every row of gen_cases, from three starts -- the empty set, the optimal set, and the optimal set of a neighbouring lambda (the
accepted trial point of the row's first iteration).  Same final working set and sides, z to the 1e-10 of the existing pins; the
step counts are what test_gpu_gen_hot.py expects of the device: one step from the optimal set, 1 + (active members) from the
equalities where no member is dropped on the way."""
from __future__ import annotations

import numpy as np
import pytest

import gen_cases as GC
import gen_hot_ref as GH
import gen_ref as G
import newton_ref as N
from helpers import rel_err

TOL = 1e-10


def _starts(c, k):
    st0, st1 = c["ref"]["stages"], c["st1"]
    side = lambda st: np.concatenate([st["side"][k], st["rside"][k]])
    return dict(empty=np.zeros(len(side(st0)), int), optimal=side(st0), neighbour=side(st1))


@pytest.mark.parametrize("rid", GC.ROW_IDS)
def test_every_start_ends_at_the_cold_solution(rid):
    c = GC.case(rid)
    qps = GH.node_qps(c["d"], c["lam0"], c["kinds"])
    assert qps
    for k, qp in qps.items():
        G.STATS["drops"] = 0
        z, sb, sr, mu, _, _ = G.solve_gen(*qp)
        drops = G.STATS["drops"]
        lo, hi, dlo, dhi = qp[2], qp[3], qp[5], qp[6]
        active = int(np.sum((sb != 0) & (lo < hi))) + int(np.sum((sr != 0) & (dlo < dhi)))
        for name, s0 in _starts(c, k).items():
            r = GH.solve_gen_from(*qp, side0=s0)
            viol, margin = G.certify_gen(*qp, r["z"], r["sb"], r["sr"], r["mu_d"])
            e = rel_err(r["z"].astype(np.float64), z.astype(np.float64))
            print(f"{rid} node {k} from {name}: steps {r['steps']} redo {r['redo']} z {e:.2e} certificate {viol:.2e} margin {margin:.2e} (active {active}, drops {drops})")
            assert np.array_equal(r["sb"], sb) and np.array_equal(r["sr"], sr)
            assert e <= TOL and rel_err(r["mu_d"].astype(np.float64), mu.astype(np.float64)) <= TOL
            assert viol <= N.CERT_TOL and margin >= GC.GAP
            assert not r["redo"]
            if name == "optimal":
                assert r["steps"] == 1
            if name == "empty":
                assert r["steps"] == GH.solve_gen_from(*qp)["steps"] >= 1 + active
                if drops == 0:
                    assert r["steps"] == 1 + active


def test_a_stale_set_is_only_a_worse_guess():
    """a stored set of other sizes, with members on infinite sides and every multiplier of the wrong sign, and a dependent one"""
    c = GC.case("more_rows_than_vars")
    (k, qp), = GH.node_qps(c["d"], c["lam0"], c["kinds"]).items()
    cold = GH.solve_gen_from(*qp)
    n, m = len(qp[1]), len(qp[5])
    opt = np.concatenate([cold["sb"], cold["sr"]])
    flipped = np.concatenate([-opt, np.ones(7, int)])                   # the other (far or infinite) sides, and rows that do not exist
    for name, s0 in (("flipped", flipped), ("all lower", -np.ones(n + m, int)), ("all upper", np.ones(n + m, int))):
        r = GH.solve_gen_from(*qp, side0=s0)
        print(f"{name}: steps {r['steps']} redo {r['redo']}")
        assert np.array_equal(r["sb"], cold["sb"]) and np.array_equal(r["sr"], cold["sr"])
        assert rel_err(r["z"].astype(np.float64), cold["z"].astype(np.float64)) <= TOL
    # two stored rows made parallel with different ranges: the set is dependent, the solve is redone cold
    H, h, lo, hi, Gm, dlo, dhi = qp
    rows = np.flatnonzero(cold["sr"])
    G2 = np.array(Gm, copy=True)
    G2[rows[1]] = G2[rows[0]]
    act = G2[rows[0]] @ cold["z"].astype(np.float64)
    dlo2, dhi2 = np.array(dlo, copy=True), np.array(dhi, copy=True)
    dlo2[rows[1]], dhi2[rows[1]] = act - 7.0, act + 7.0
    qp2 = (H, h, lo, hi, G2, dlo2, dhi2)
    s0 = opt.copy()
    s0[n + rows[1]] = 1
    r, c2 = GH.solve_gen_from(*qp2, side0=s0), GH.solve_gen_from(*qp2)
    assert r["redo"] and r["steps"] > c2["steps"]
    assert np.array_equal(r["sb"], c2["sb"]) and np.array_equal(r["sr"], c2["sr"])


def test_an_infeasible_stage_qp_is_still_infeasible():
    bad, good, kinds = GC.infeasible_pair()
    lam = np.zeros(int(np.asarray(bad["nx"])[1:].sum()))
    (k, qg), = GH.node_qps(good, lam, kinds).items()
    (_, qb), = GH.node_qps(bad, lam, kinds).items()
    rg = GH.solve_gen_from(*qg)
    with pytest.raises(ValueError):
        GH.solve_gen_from(*qb, side0=np.concatenate([rg["sb"], rg["sr"]]))

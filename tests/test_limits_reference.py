"""The CPU oracle on the shapes of limit_shapes.py (both sides of every kernel-selection limit of the device path), before any
device run compares with it: its first iterate is lambda0 + tau dlam with dlam the step of newton_ref.py (a dense numpy
construction that shares no code with the oracle), its optimum satisfies the KKT conditions of the QP, and on the dense trees the
numpy certificate (one global equality-constrained KKT solve) agrees with it."""
from __future__ import annotations

import numpy as np
import pytest

import limit_shapes as S
from helpers import certify, rel_err
from newton_ref import starting_duals

CASES = list(S.cases())


@pytest.mark.parametrize("cid,kind,shape,flags", CASES, ids=[c[0] for c in CASES])
def test_oracle_optimum_on_limit_shapes(orc, cid, kind, shape, flags):
    d = S.problem(kind, shape)
    if kind == S.C:
        ref = orc.solve(d, orc.default_opts())
        assert ref["status"] == 0
        assert orc.max_kkt(d, ref) < 1e-8
        return
    ref = orc.solve_dense(d, orc.default_opts())
    assert ref["status"] == 0
    # dense unconstrained nodes ignore the bounds: the KKT conditions are those of the QP without them, and the certificate is
    # the global KKT solve itself (no bound active)
    free = dict(d, xmin=np.full(len(d["q"]), -1e12), xmax=np.full(len(d["q"]), 1e12),
                umin=np.full(len(d["r"]), -1e12), umax=np.full(len(d["r"]), 1e12))
    assert orc.max_kkt(free, ref, dense=True) < 1e-8
    assert certify(free, ref) == 0


@pytest.mark.parametrize("cid,kind,shape,flags", CASES, ids=[c[0] for c in CASES])
def test_oracle_first_iterate_is_the_newton_step(orc, cid, kind, shape, flags):
    """maxIter = 1, no regularisation: the oracle's lambda after one iteration is lambda0 + tau dlam_ref, tau = beta^(trials - 1)
    from its line-search trace, at a lambda0 that keeps every stage value 1e-6 away from its clipping thresholds."""
    d = S.problem(kind, shape)
    dense = kind == S.D
    lam0, ref = starting_duals(d, dense)
    assert ref["cond"] <= 1e6, f"cond(M) = {ref['cond']:.2e}: the tolerance below would mean nothing"
    opts = orc.default_opts(maxIter=1, regType=0)
    got = orc.solve_dense(d, opts, lam0) if dense else orc.solve(d, opts, lam0)
    assert got["status"] == 1 and got["iter"] == 1
    trials = got["ls_total"] if dense else int(got["trace_ls"][0])
    tau = opts.lineSearchBeta ** (trials - 1)
    assert rel_err(got["lam"], lam0 + tau * ref["dlam"]) <= 1e-10


def test_shapes_sit_where_the_rows_say():
    """The structural quantities each row is about, counted on the flattened tree (not on the device's own tables)."""
    from treeqp_amd import problems as P
    got = {}
    for cid, kind, shape, flags in CASES:
        nk, nx, nu = S.flatten(shape)
        dad = P.parents_of(nk)
        kid0 = np.concatenate([[1], 1 + np.cumsum(nk)[:-1]])
        d = np.array([nx[kid0[k]:kid0[k] + nk[k]].sum() for k in range(len(nk))])
        lvl = np.zeros(len(nk), int)
        for k in range(1, len(nk)):
            lvl[k] = lvl[dad[k]] + 1
        got[cid] = dict(Nn=len(nk), dmax=int(d.max()), widest=int(np.bincount(lvl).max()), depth=int(lvl.max()),
                        nzmax=int((nx + nu)[nk > 0].max()), kids=int(nk.max()))
    assert (got["wide_class-d16"]["dmax"], got["wide_class-d17"]["dmax"]) == (16, 17)
    assert (got["wide_class-d64"]["dmax"], got["wide_class-d65"]["dmax"]) == (64, 65)
    assert (got["wide_class-nz32"]["nzmax"], got["wide_class-nz33"]["nzmax"]) == (32, 33)
    assert [got[f"k_sgp_children-kids{m}"]["kids"] for m in (4, 5, 8, 9)] == [4, 5, 8, 9]
    assert got["k_sgp_children-kids16_d64"]["dmax"] == 64
    assert (got["forward_chain-path16"]["depth"], got["forward_chain-path17"]["depth"]) == (17, 18)      # deepest parent 16 / 17
    assert (got["widest_level-w96"]["widest"], got["widest_level-w97"]["widest"]) == (96, 97)
    assert (got["FUSE_MAX-n512"]["Nn"], got["FUSE_MAX-n513"]["Nn"]) == (512, 513)
    assert (got["root_fan-out-fan64"]["kids"], got["root_fan-out-fan100"]["kids"]) == (64, 100)
    assert [got[f"dense_kind_1-nz{n}"]["nzmax"] for n in (64, 65, 90, 91, 120, 142)] == [64, 65, 90, 91, 120, 142]

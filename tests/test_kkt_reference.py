"""kkt_ref.py against the host's tree_qp_out_calculate_KKT_res (qp_container.c, the port of tree_qp_common.c:540-788), entry by
entry, without a device: an irregular tree with dense objectives, finite bounds and rows, at a random point (not a solution, so
that every class is non-zero).  Tolerance: the bound of kkt_ref's docstring, 2 (m + 2) eps T per entry -- the host sums the same
m terms in another order."""
import ctypes as C

import numpy as np
import pytest

import gen_cases as GC
import kkt_ref as K
from limit_shapes import leaf

SHAPE = (3, 2, [(2, 1, [leaf(1), leaf(3)]), (4, 2, [leaf(2)]), (1, 1, [leaf(2)])])      # 8 nodes, 1 - 3 children, nx 1 .. 4
NC = [2, 1, 0, 3, 0, 1, 0, 2]


@pytest.fixture(scope="module")
def case():
    d = K.random_problem(SHAPE, [3] * 8, 3, nc=NC)
    sol = K.random_point(d, 3)
    return d, sol, K.residuals(d, sol)


def test_every_class_is_non_zero_and_every_node_clear(case):
    _, _, ref = case
    assert np.all(ref["res"] > 1e-3), ref["res"]
    assert np.all(ref["node"] >= 0)
    assert K.node_is_clear(ref).all()
    assert np.all(ref["bound"] < 1e-12) and np.all(ref["bound"] > 0)


def test_entries_match_the_host_function(capi, case):
    d, sol, ref = case
    qp = GC.container_of(capi, d)
    qp.set_solution(sol)
    want, bound = K.host_order(ref)
    n = 3 * int(np.sum(d["nx"]) + np.sum(d["nu"])) + int(np.sum(d["nx"][1:])) + 2 * int(np.sum(d["nc"]))
    assert len(want) == n
    got = np.zeros(n)
    capi.lib().tree_qp_out_calculate_KKT_res(C.byref(qp.qp_in), C.byref(qp.qp_out), got.ctypes.data_as(C.POINTER(C.c_double)))
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    print(f"largest |host - ref| = {err.max():.3e}, entry {worst}: {err[worst]:.3e} against its bound {bound[worst]:.3e}")
    assert np.all(err <= bound), (worst, got[worst], want[worst], bound[worst])
    assert abs(qp.max_kkt_res() - ref["max"]) <= ref["bound"].max()


def test_corner_semantics_of_the_reference():
    """zero multipliers on infinite bounds give 0, non-zero ones inf; a NaN in x reaches the classes that read it, at the right node"""
    d = K.random_problem((3, 2, [(2, 1, [leaf(1)]), leaf(4)]), [0, 0, 0, 0], 4)
    sol = K.random_point(d, 4)
    d["xmax"][:] = np.inf; d["umin"][:] = -np.inf
    sol["mu_x"][:] = 0.0; sol["mu_u"][:] = 0.0
    ref = K.residuals(d, sol)
    assert ref["res"][K.BCOMPL] == 0.0 and np.isfinite(ref["res"]).all()
    sol["mu_x"][4] = 0.5                      # node 1, entry 1: against xmax = inf
    ref = K.residuals(d, sol)
    assert np.isinf(ref["res"][K.BCOMPL]) and ref["node"][K.BCOMPL] == 1
    sol["mu_x"][4] = 0.0
    sol["x"][3] = np.nan                      # node 1, entry 0
    ref = K.residuals(d, sol)
    assert np.isnan(ref["res"][[K.STAT, K.DYN, K.BFEAS]]).all() and not np.isnan(ref["res"][K.BCOMPL])
    assert list(ref["node"][[K.STAT, K.DYN, K.BFEAS]]) == [1, 1, 1] and np.isnan(ref["max"])
    assert ref["node"][K.GFEAS] == -1 and ref["res"][K.GFEAS] == 0.0

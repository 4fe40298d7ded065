"""The gradient of an MPC step in the tracking reference on the device (tqgpu_mpc_adjoint_reference) against adjbnd_ref.reference evaluated with
adj_ref.dual_form at the device's own exported point, and against itself.

Cases: adjbnd_cases.TRACK_IDS (kind 0 and kind 1, an eliminated root with and without S0, a root with states, a stage of 65 and of 64
nodes), each with a window that gives one stage per row, one that clamps the last two stages into row T - 1, and T == 1.
Tolerances: 10 times the spread of the two numpy evaluations on the CPU (adjbnd_cases.SPREAD), floor 1e-12."""
import numpy as np
import pytest

import adj_ref as AR
import adjbnd_cases as BC
import adjbnd_ref as BR
import adjmat_ref as AM
import tracking_cases as TC

pytestmark = pytest.mark.gpu

EINVAL = -2


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


def _stepped(capi, c, t0, w=None):
    g = TC.make(capi, c)
    r, _ = g.mpc_step(c["x0"], t0=t0, **c["opts"])
    assert r["status"] == 0
    g.mpc_adjoint(*(c["w"] if w is None else w), **c["opts"])
    return g


def _partials(c, t0):
    """per row the number of chunks of its stages"""
    st = BR.stages(c["d"]["nk"])
    row0, rows = BR.rows_of(c["d"]["nk"], t0, c["T"])
    n = np.zeros(rows, dtype=int)
    for s in range(int(st.max()) + 1):
        n[min(t0 + s, c["T"] - 1) - row0] += -(-int(np.sum(st == s)) // 64)
    return n


@pytest.mark.parametrize("which", ["stage_per_row", "clamped", "T1"])
@pytest.mark.parametrize("cid", BC.TRACK_IDS)
def test_against_the_reference(capi, cid, which):
    c = BC.track_case(cid, 1 if which == "T1" else None)
    t0 = 0 if which == "T1" else BC.windows(c)[which == "clamped"]
    g = _stepped(capi, c, t0)
    try:
        sol = g.solution()
        got = g.mpc_adjoint_reference()
        multi = bool(np.any(_partials(c, t0) > 1))
        assert _counts(capi) == (2 if multi else 1, 1, 1)
        assert multi == (which != "stage_per_row" or cid == "fan65")
        d = BC.folded(c, t0)
        b = AR.dual_form(d, sol["x"], sol["u"], c["param"], c["w"], c["kinds"])
        assert b["n_reg"] == 0
        S0 = c["root"]["S0"] if c["form"] == "elim" else None
        row0, rows, gx, gu = BR.reference(d, b["gq"], b["gr"], t0, c["T"], c["NXT"], c["NUT"], c["kinds"], S0)
        assert (got["row0"], got["rows"]) == (row0, rows) == (min(t0, c["T"] - 1), min(t0 + int(BR.stages(d["nk"]).max()), c["T"] - 1) - min(t0, c["T"] - 1) + 1)
        for i, (name, x, y) in enumerate((("gxref", got["gxref"], gx), ("guref", got["guref"], gu))):
            err = float(np.max(np.abs(x - y)))
            print(f"{cid} {which} {name}: |device - (b)| = {err:.3e}, tolerance {BC.tol(cid, i):.3e}")
            assert x.shape == y.shape and err <= BC.tol(cid, i)
        assert np.any(got["gxref"] != 0.0) and np.any(got["guref"] != 0.0)
        # a row whose nodes are all leaves has no part in uref
        st, nk = BR.stages(d["nk"]), np.asarray(d["nk"])
        for r in range(rows):
            mine = np.array([min(t0 + s, c["T"] - 1) - row0 == r for s in st])
            if np.all(nk[mine] == 0):
                assert np.all(got["guref"][r] == 0.0)
        if which == "stage_per_row" and cid != "c1_eliminated":
            assert np.all(got["guref"][rows - 1] == 0.0)
    finally:
        g.close()


@pytest.mark.parametrize("cid", ["single_wg", "kind1_S0", "fan65"])
def test_columns_and_what_is_left_alone(capi, cid):
    c = BC.track_case(cid)
    t0 = BC.windows(c)[1]
    wx, wu = c["w3"]
    g = _stepped(capi, c, t0, (wx, wu))
    try:
        g.mpc_set_param_groups(None, None)
        grads, mat, kkt, sol = g.mpc_adjoint_grads(), g.mpc_adjoint_matrices(), g.kkt_residual(), g.solution()
        g.mpc_sensitivity(**c["opts"])
        gain = g.mpc_gain()
        g.mpc_adjoint(wx, wu, **c["opts"])
        all3 = g.mpc_adjoint_reference()
        assert all3["gxref"].shape == (all3["rows"], c["NXT"], 3) and all3["guref"].shape == (all3["rows"], c["NUT"], 3)
        for key in ("gq", "gr", "gb"):
            _same_bits(g.mpc_adjoint_grads()[key], grads[key], f"{key} after tqgpu_mpc_adjoint_reference")
        _same_bits(g.kkt_residual()["res"], kkt["res"], "the KKT residual")
        for i in range(3):
            _same_bits(g.mpc_gain()[i], gain[i], f"mpc_gain[{i}]")
        again = g.mpc_adjoint_matrices()
        for key in AM.KEYS:
            for x, y in zip(again[key], mat[key]):
                _same_bits(x, y, f"{key} of tqgpu_mpc_adjoint_matrices")
        for j in range(3):
            g.mpc_adjoint(wx[:, j], wu[:, j], **c["opts"])
            one = g.mpc_adjoint_reference()
            for key in ("gxref", "guref"):
                _same_bits(one[key][:, :, 0], all3[key][:, :, j], f"column {j} of {key}")
        r, _ = g.mpc_step(c["x0"], **c["opts"])
        h = TC.make(capi, c)
        try:
            h.mpc_step(c["x0"], t0=t0, **c["opts"])
            h.mpc_step(c["x0"], **c["opts"])
            for k in ("x", "u", "lam"):
                _same_bits(g.solution()[k], h.solution()[k], f"{k} of the next solve")
        finally:
            h.close()
    finally:
        g.close()


def test_refusals(capi):
    import ctypes as C
    c = BC.track_case("single_wg")
    L = capi.lib()
    row0, rows = C.c_int(-7), C.c_int(-7)
    g = TC.make(capi, c, tracking=False)
    try:
        g.mpc_step(c["x0"], **c["opts"])
        g.mpc_adjoint(*c["w"], **c["opts"])
        assert L.tqgpu_mpc_adjoint_reference(g.h, None, None, C.byref(row0), C.byref(rows)) == EINVAL          # before tqgpu_mpc_set_tracking
        g.mpc_set_tracking(c["xtraj"], c["utraj"], c["q0"], c["r0"])
        assert g.mpc_window == -1
        g.mpc_step(c["x0"], **c["opts"])
        g.mpc_adjoint(*c["w"], **c["opts"])
        assert L.tqgpu_mpc_adjoint_reference(g.h, None, None, C.byref(row0), C.byref(rows)) == EINVAL          # no window in force
        g.mpc_step(c["x0"], t0=1, **c["opts"])
        assert L.tqgpu_mpc_adjoint_reference(g.h, None, None, C.byref(row0), C.byref(rows)) == EINVAL          # no stored adjoint
        assert (row0.value, rows.value) == (-7, -7)
        g.mpc_adjoint(*c["w"], **c["opts"])
        assert L.tqgpu_mpc_adjoint_reference(g.h, None, None, C.byref(row0), C.byref(rows)) == 0 and (row0.value, rows.value) == (1, 3)
        g.mpc_set_window(2)
        assert L.tqgpu_mpc_adjoint_reference(g.h, None, None, C.byref(row0), C.byref(rows)) == EINVAL          # the window moved: the adjoint went
    finally:
        g.close()

"""The entry points of tracking MPC (include/treeqp_amd.h: tqgpu_set_linear_terms, tqgpu_get_linear_terms, tqgpu_mpc_set_tracking,
tqgpu_mpc_set_window, tqgpu_mpc_get_window, tqgpu_mpc_step_at, tqgpu_mpc_step_batch_at): declared, exported, wrapped, and the numpy fold
of tracking_cases.py against a plain dense evaluation.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
DECLARED = {
    "tqgpu_set_linear_terms": S + r"\s*,\s*const\s+double\s*\*\s*q\s*,\s*const\s+double\s*\*\s*r",
    "tqgpu_get_linear_terms": S + r"\s*,\s*double\s*\*\s*q\s*,\s*double\s*\*\s*r",
    "tqgpu_mpc_set_tracking": S + r"\s*,\s*int\s+NXT\s*,\s*int\s+NUT\s*,\s*int\s+T\s*,\s*const\s+double\s*\*\s*xtraj\s*,\s*const\s+double\s*\*\s*utraj\s*,"
                                  r"\s*const\s+double\s*\*\s*q0\s*,\s*const\s+double\s*\*\s*r0",
    "tqgpu_mpc_set_window": S + r"\s*,\s*int\s+t0",
    "tqgpu_mpc_get_window": r"const\s+" + S + r"\s*,\s*int\s*\*\s*t0",
    "tqgpu_mpc_step_at": S + r"\s*,\s*const\s+double\s*\*\s*x0\s*,\s*int\s+t0\s*,\s*const\s+tqgpu_opts\s*\*\s*opts\s*,\s*tqgpu_result\s*\*\s*res\s*,\s*double\s*\*\s*u0",
    "tqgpu_mpc_step_batch_at": r"tqgpu_solver\s*\*\*\s*solvers\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*x0s\s*,\s*const\s+int\s*\*\s*t0s\s*,"
                               r"\s*const\s+tqgpu_opts\s*\*\s*opts\s*,\s*tqgpu_result\s*\*\s*results\s*,\s*double\s*\*\s*u0s",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers_have_the_documented_signatures(capi):
    want = {
        "set_linear_terms": ["self", "q", "r"],
        "linear_terms": ["self"],
        "mpc_set_tracking": ["self", "xtraj", "utraj", "q0", "r0"],
        "mpc_set_window": ["self", "t0"],
        # unchanged: t0 / t0s travel with the keywords
        "mpc_step": ["self", "x0", "profile", "kw"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    assert isinstance(capi.TqGpu.mpc_window, property)
    assert list(inspect.signature(capi.mpc_step_batch).parameters) == ["mirrors", "x0s", "profile", "kw"]
    assert "t0" in capi.TqGpu.mpc_step.__doc__ and "t0s" in capi.mpc_step_batch.__doc__


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    x = np.zeros(6)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    w = C.c_int(7)
    o, res = capi._gpu_opts(), capi.GpuResult()
    for rc in (L.tqgpu_set_linear_terms(None, p, p), L.tqgpu_get_linear_terms(None, p, p), L.tqgpu_mpc_set_tracking(None, 1, 1, 1, p, p, None, None),
               L.tqgpu_mpc_set_window(None, 0), L.tqgpu_mpc_get_window(None, C.byref(w)), L.tqgpu_mpc_step_at(None, p, 0, C.byref(o), C.byref(res), p)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert L.tqgpu_mpc_step_batch_at(None, 1, p, None, C.byref(o), C.byref(res), p) == -2
    assert not x.any() and w.value == 7


def test_the_header_documents_the_fold():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("tqgpu_mpc_set_tracking", "min(t0 + stage[k], T - 1)", "fma(-Qd[i], xref[i], q0[i])", "- S0 xref_rho, + S0 x0", "Phantom root states keep their q"):
        assert word in text, word


def test_numpy_fold_is_the_tracking_objective():
    """q, r of tracking_cases.fold are the linear terms of sum_k 1/2 (z_k - ref_k)' H_k (z_k - ref_k) + base' z_k, and the exact cases make
    every order of the sums give the same bits"""
    import tracking_cases as K
    for c in K.cases():
        d = c["d"]
        nx, nu = np.asarray(d["nx"], dtype=int), np.asarray(d["nu"], dtype=int)
        st = K.stages(d["nk"])
        assert st[0] == 0 and st.max() >= 2
        for t0 in (0, 9):
            x0 = c["x0s"][0]
            q, r = K.fold(c, t0, x0)
            at_x, at_u = 0, 0
            for k in range(len(nx)):
                row = min(t0 + st[k], c["T"] - 1)
                Q, Rm, Sm = K.blocks(d, k)
                Hk = np.block([[Q, Sm.T], [Sm, Rm]])
                ref = np.concatenate([c["xtraj"][row][:nx[k]], c["utraj"][row][:nu[k]]])
                base = np.concatenate([c["q0"][at_x:at_x + nx[k]], c["r0"][at_u:at_u + nu[k]]])
                want = base - (Hk[:, ::-1] @ ref[::-1])          # the columns in the other order
                if k == 0 and c["form"] == "elim" and c["root"]["S0"] is not None:
                    want[nx[k]:] += c["root"]["S0"] @ (x0 - c["xtraj"][row])
                got = np.concatenate([q[at_x:at_x + nx[k]], r[at_u:at_u + nu[k]]])
                assert np.array_equal(got, want), f"{c['id']} node {k} window {t0}"
                at_x += nx[k]; at_u += nu[k]
        # exact data: multiples of 2^-6, at most 4 in size, wherever the fold reads
        for name in ("Qd", "Rd") + (("Q", "R", "S") if "Q" in d else ()):
            v = np.asarray(d[name])
            assert np.all(v * 64 == np.round(v * 64)) and np.all(np.abs(v) <= 4), f"{c['id']}: {name}"

"""The entry points of the tangent of an MPC step (include/treeqp_amd.h: tqgpu_mpc_tangent, tqgpu_mpc_get_tangent_u0, tqgpu_mpc_get_tangent,
tqgpu_mpc_predict_at): declared, exported, wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
O = r"\s*,\s*const\s+tqgpu_opts\s*\*\s*opts"
D = r"double\s*\*\s*"
CD = r"\s*,\s*const\s+" + D
DECLARED = {
    "tqgpu_mpc_tangent": S + O + CD + "dq" + CD + "dr" + CD + "db" + CD + r"dx0\s*,\s*int\s+nd\s*,\s*int\s*\*\s*n_reg",
    "tqgpu_mpc_get_tangent_u0": S + r"\s*,\s*" + D + "du0",
    "tqgpu_mpc_get_tangent": S + r"\s*,\s*" + D + r"dx\s*,\s*" + D + r"du\s*,\s*" + D + "dlam",
    "tqgpu_mpc_predict_at": S + O + CD + r"x0_new\s*,\s*int\s+t0_new\s*,\s*" + D + r"u0_pred\s*,\s*int\s+duals\s*,\s*int\s*\*\s*n_clipped\s*,\s*int\s*\*\s*n_reg",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    want = {"mpc_tangent": ["self", "dq", "dr", "db", "dx0", "profile", "kw"], "mpc_tangent_u0": ["self"], "mpc_tangent_values": ["self"],
            "mpc_predict_at": ["self", "x0_new", "t0", "duals", "profile", "kw"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    sig = inspect.signature(capi.TqGpu.mpc_tangent)
    assert all(sig.parameters[k].default is None for k in ("dq", "dr", "db", "dx0")) and sig.parameters["profile"].default == 0
    sig = inspect.signature(capi.TqGpu.mpc_predict_at)
    assert sig.parameters["x0_new"].default is None and sig.parameters["t0"].default == -1 and sig.parameters["duals"].default is False


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    w = np.full(4, 7.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    a, b = C.c_int(7), C.c_int(7)
    o = capi._gpu_opts(0)
    for rc in (L.tqgpu_mpc_tangent(None, C.byref(o), p, p, p, p, 1, C.byref(a)), L.tqgpu_mpc_get_tangent_u0(None, p), L.tqgpu_mpc_get_tangent(None, p, p, p),
               L.tqgpu_mpc_predict_at(None, C.byref(o), p, 0, p, 1, C.byref(a), C.byref(b))):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert np.all(w == 7.0) and a.value == 7 and b.value == 7


def test_the_header_documents_the_formulas():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("R_c = (P_c dh_c)^x - C_c P_p dh_p + db_c + G_c dx0", "dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) - P_k dh_k + direct_k dx0",
                 "dLam is unique only when n_reg == 0", "2 Nh + 2", "dq[i] = fma(-Qd[i], dxref[i], 0.0)", "is not added twice"):
        assert word in text, word

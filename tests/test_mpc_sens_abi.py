"""The entry points of the parametric sensitivities (include/treeqp_amd.h: tqgpu_mpc_sensitivity, tqgpu_mpc_get_gain,
tqgpu_mpc_get_sensitivities, tqgpu_mpc_predict, counted by tqgpu_mpc_stats): declared, exported, wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
D = r"double\s*\*\s*"
DECLARED = {
    "tqgpu_mpc_sensitivity": S + r"\s*,\s*const\s+tqgpu_opts\s*\*\s*opts\s*,\s*int\s*\*\s*n_reg",
    "tqgpu_mpc_get_gain": S + r"\s*,\s*" + D + r"K\s*,\s*" + D + r"u0\s*,\s*" + D + "x0_ref",
    "tqgpu_mpc_get_sensitivities": S + r"\s*,\s*" + D + r"dx\s*,\s*" + D + r"du\s*,\s*" + D + "dlam",
    "tqgpu_mpc_predict": S + r"\s*,\s*const\s+" + D + r"x0_new\s*,\s*" + D + r"u0_pred\s*,\s*int\s+duals\s*,\s*int\s*\*\s*n_clipped",
    "tqgpu_mpc_stats": r"int\s*\*\s*launches\s*,\s*int\s*\*\s*copies\s*,\s*int\s*\*\s*waits",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    want = {"mpc_sensitivity": ["self", "profile", "kw"], "mpc_gain": ["self"], "mpc_sensitivities": ["self"], "mpc_predict": ["self", "x0_new", "duals"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    w = np.full(4, 7.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    a = C.c_int(7)
    o = capi._gpu_opts(0)
    for rc in (L.tqgpu_mpc_sensitivity(None, C.byref(o), C.byref(a)), L.tqgpu_mpc_get_gain(None, p, p, p), L.tqgpu_mpc_get_sensitivities(None, p, p, p),
               L.tqgpu_mpc_predict(None, p, p, 1, C.byref(a))):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert np.all(w == 7.0) and a.value == 7


def test_the_header_documents_the_formulas():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("G_c = A0_c - B_c P_0 S0", "G_c = A_c", "dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) + direct_k", "direct_0 = -P_0 [0; S0]",
                 "v = fma(K[i, j], dx_j, v)", "v = fma(dLam[e, j], dx_j, v)", "dLam is unique only when n_reg == 0", "W_p = C P_p C' + blockdiag(P_c^{xx})"):
        assert word in text, word

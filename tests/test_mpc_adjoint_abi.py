"""The entry points of the adjoint of an MPC step (include/treeqp_amd.h: tqgpu_mpc_adjoint, tqgpu_mpc_get_adjoint_x0,
tqgpu_mpc_get_adjoint): declared, exported, wrapped.  No device needed."""
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
    "tqgpu_mpc_adjoint": S + r"\s*,\s*const\s+tqgpu_opts\s*\*\s*opts\s*,\s*const\s+" + D + r"wx\s*,\s*const\s+" + D + r"wu\s*,\s*int\s+nw\s*,\s*int\s*\*\s*n_reg",
    "tqgpu_mpc_get_adjoint_x0": S + r"\s*,\s*" + D + "gx0",
    "tqgpu_mpc_get_adjoint": S + r"\s*,\s*" + D + r"gq\s*,\s*" + D + r"gr\s*,\s*" + D + "gb",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    want = {"mpc_adjoint": ["self", "wx", "wu", "profile", "kw"], "mpc_adjoint_grads": ["self"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    sig = inspect.signature(capi.TqGpu.mpc_adjoint)
    assert sig.parameters["wx"].default is None and sig.parameters["wu"].default is None and sig.parameters["profile"].default == 0


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    w = np.full(4, 7.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    a = C.c_int(7)
    o = capi._gpu_opts(0)
    for rc in (L.tqgpu_mpc_adjoint(None, C.byref(o), p, p, 1, C.byref(a)), L.tqgpu_mpc_get_adjoint_x0(None, p), L.tqgpu_mpc_get_adjoint(None, p, p, p)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert np.all(w == 7.0) and a.value == 7


def test_the_header_documents_the_formulas():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("R_c = (P_c w_c)^x - C_c P_p w_p", "gb_c = Y_c", "[gq_k; gr_k] = -P_k ( w_k - [Y_k; 0] + sum_c C_c' Y_c )",
                 "gx0 = sum_c A0_c' Y_c + S0' gr_0", "gx0 = wx_0 + sum_c A_c' Y_c", "gb is unique only when n_reg == 0"):
        assert word in text, word

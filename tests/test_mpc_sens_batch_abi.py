"""The entry points of the batched sensitivity and predictor (include/treeqp_amd.h: tqgpu_mpc_sensitivity_batch, tqgpu_mpc_predict_batch):
declared, exported, wrapped, and their refusals of bad arguments, which need no device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
D = r"double\s*\*\s*"
HEAD = r"tqgpu_solver\s*\*\*\s*solvers\s*,\s*int\s+n\s*,\s*"
DECLS = {
    "tqgpu_mpc_sensitivity_batch": HEAD + r"const\s+tqgpu_opts\s*\*\s*opts\s*,\s*int\s*\*\s*n_reg",
    "tqgpu_mpc_predict_batch": HEAD + r"const\s+" + D + r"x0_new\s*,\s*" + D + r"u0_pred\s*,\s*int\s+duals\s*,\s*int\s*\*\s*n_clipped",
}


def test_symbols_declared_and_exported(capi):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    for name, args in DECLS.items():
        assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
        assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    assert hasattr(capi, "mpc_sensitivity_batch"), "capi.mpc_sensitivity_batch is missing"
    sig = inspect.signature(capi.mpc_sensitivity_batch)
    assert list(sig.parameters) == ["mirrors", "profile", "kw"] and sig.parameters["profile"].default == 0
    assert sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert hasattr(capi, "mpc_predict_batch"), "capi.mpc_predict_batch is missing"
    sig = inspect.signature(capi.mpc_predict_batch)
    assert list(sig.parameters) == ["mirrors", "x0s", "duals"] and sig.parameters["duals"].default is False


def test_bad_arguments_are_refused_with_a_message(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    g = np.full(4, 7.0)
    p = g.ctypes.data_as(C.POINTER(C.c_double))
    a = (C.c_int * 1)(7)
    one = (C.c_void_p * 1)(None)
    for rc in (L.tqgpu_mpc_sensitivity_batch(None, 1, C.byref(o), a),          # no array of mirrors
               L.tqgpu_mpc_sensitivity_batch(one, 0, C.byref(o), a),           # n = 0
               L.tqgpu_mpc_sensitivity_batch(one, 1, None, a)):                # no options
        assert rc == -2 and b"tqgpu_mpc_sensitivity_batch" in L.tqgpu_last_error()
    for rc in (L.tqgpu_mpc_predict_batch(None, 1, p, p, 0, a),                 # no array of mirrors
               L.tqgpu_mpc_predict_batch(one, 0, p, p, 0, a),                  # n = 0
               L.tqgpu_mpc_predict_batch(one, 1, None, p, 0, a)):              # no x0_new
        assert rc == -2 and b"tqgpu_mpc_predict_batch" in L.tqgpu_last_error()
    assert np.all(g == 7.0) and a[0] == 7


def test_a_null_member_is_refused_and_the_buffers_are_untouched(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    g = np.full(4, 7.0)
    p = g.ctypes.data_as(C.POINTER(C.c_double))
    a = (C.c_int * 1)(7)
    one = (C.c_void_p * 1)(None)
    assert L.tqgpu_mpc_sensitivity_batch(one, 1, C.byref(o), a) == -2
    assert b"member 0" in L.tqgpu_last_error() and b"null solver" in L.tqgpu_last_error()
    assert L.tqgpu_mpc_predict_batch(one, 1, p, p, 1, a) == -2
    assert b"member 0" in L.tqgpu_last_error() and b"null solver" in L.tqgpu_last_error()
    assert np.all(g == 7.0) and a[0] == 7

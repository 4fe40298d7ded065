"""The entry points of the root-states MPC step and of the certified step (include/treeqp_amd.h: tqgpu_mpc_set_root_states,
tqgpu_get_root_bounds, tqgpu_mpc_set_certify, tqgpu_mpc_get_certificate): declared, exported, wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
DECLARED = {
    "tqgpu_mpc_set_root_states": r"tqgpu_solver\s*\*\s*s",
    "tqgpu_get_root_bounds": r"tqgpu_solver\s*\*\s*s\s*,\s*double\s*\*\s*xmin0\s*,\s*double\s*\*\s*xmax0",
    "tqgpu_mpc_set_certify": r"tqgpu_solver\s*\*\s*s\s*,\s*int\s+on",
    "tqgpu_mpc_get_certificate": r"tqgpu_solver\s*\*\s*s\s*,\s*double\s+res\s*\[\s*6\s*\]\s*,\s*int\s+node\s*\[\s*6\s*\]",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers_have_the_documented_signatures(capi):
    want = {
        "mpc_set_root_states": ["self"],
        "root_bounds": ["self"],
        "mpc_set_certify": ["self", "on"],
        "mpc_certificate": ["self"],
        # unchanged
        "mpc_set_x0": ["self", "x0"],
        "mpc_step": ["self", "x0", "profile", "kw"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    assert list(inspect.signature(capi.mpc_step_batch).parameters) == ["mirrors", "x0s", "profile", "kw"]


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    x = np.zeros(6)
    n = np.zeros(6, dtype=np.int32)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    for rc in (L.tqgpu_mpc_set_root_states(None), L.tqgpu_get_root_bounds(None, p, p), L.tqgpu_mpc_set_certify(None, 1),
               L.tqgpu_mpc_get_certificate(None, p, n.ctypes.data_as(C.POINTER(C.c_int)))):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert not x.any() and not n.any()


def test_the_header_documents_both_forms_and_the_launch_formula():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("tqgpu_mpc_set_root_states", "tqgpu_mpc_set_certify", "tqgpu_mpc_step_batch ignores the setting", "xmin[0] = xmax[0] = x0"):
        assert word in text, word

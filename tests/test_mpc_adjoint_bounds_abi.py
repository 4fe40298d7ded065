"""The entry points of the bound and reference gradients of an MPC step (include/treeqp_amd.h: tqgpu_mpc_get_adjoint_bounds,
tqgpu_mpc_adjoint_bounds, tqgpu_mpc_adjoint_reference): declared, exported, wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
DECLARED = {
    "tqgpu_mpc_get_adjoint_bounds": S + "".join(r"\s*,\s*double\s*\*\s*" + n for n in ("gxmin", "gxmax", "gumin", "gumax")),
    "tqgpu_mpc_adjoint_bounds": S + r"\s*,\s*double\s*\*\s*glb\s*,\s*double\s*\*\s*gub",
    "tqgpu_mpc_adjoint_reference": S + r"\s*,\s*double\s*\*\s*gxref\s*,\s*double\s*\*\s*guref\s*,\s*int\s*\*\s*row0\s*,\s*int\s*\*\s*rows",
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    for name in ("mpc_get_adjoint_bounds", "mpc_adjoint_bounds", "mpc_adjoint_reference"):
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == ["self"], name


def test_null_solver_is_refused_with_a_message_and_nothing_is_written(capi):
    L = capi.lib()
    w = np.full(8, 7.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    i = np.full(2, 7, dtype=np.int32)
    ip = i.ctypes.data_as(C.POINTER(C.c_int))
    for rc in (L.tqgpu_mpc_get_adjoint_bounds(None, p, p, p, p), L.tqgpu_mpc_get_adjoint_bounds(None, None, None, None, None),
               L.tqgpu_mpc_adjoint_bounds(None, p, p), L.tqgpu_mpc_adjoint_bounds(None, None, None),
               L.tqgpu_mpc_adjoint_reference(None, p, p, ip, ip), L.tqgpu_mpc_adjoint_reference(None, None, None, None, None)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert np.all(w == 7.0) and np.all(i == 7)


def test_the_header_documents_the_formulas_and_the_orders():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("dL/dbound_k[i] = v_k[i]", "it equals gx0 bit for", "acc[j] = fma(-Qd[j], gq[j], acc[j])", "acc[j] = fma(-H[i + j nz], gz[i], acc[j])",
                 "acc[j] = fma(-S0[m + j nu0], gr_0[m], acc[j])", "ascending (stage, chunk) order", "row0 = min(t0, T - 1)", "k_nodesum_part"):
        assert word in text, word
    assert "fold; that chain rule stays with the caller" not in text
    assert "for H that chain rule stays with the caller" in text

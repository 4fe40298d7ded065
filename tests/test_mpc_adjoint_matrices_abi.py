"""The entry points of the matrix gradients of an MPC step (include/treeqp_amd.h: tqgpu_mpc_set_param_groups, tqgpu_mpc_adjoint_matrices,
tqgpu_mpc_adjoint_matrices_batch, and the read-out tqgpu_mpc_get_param_groups): declared, exported, wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
OUTS = r"\s*,\s*".join(r"double\s*\*\s*" + n for n in ("gH", "gh", "gA", "gB", "gb", "gA0", "gS0"))
DECLARED = {
    "tqgpu_mpc_set_param_groups": S + r"\s*,\s*const\s+int\s*\*\s*hgroup\s*,\s*const\s+int\s*\*\s*cgroup\s*,\s*int\s+n_hgroups\s*,\s*int\s+n_cgroups",
    "tqgpu_mpc_get_param_groups": S + r"\s*,\s*int\s*\*\s*n_hgroups\s*,\s*int\s*\*\s*n_cgroups\s*,\s*int\s*\*\s*hdims\s*,\s*int\s*\*\s*cdims\s*,\s*int\s*\*\s*root",
    "tqgpu_mpc_adjoint_matrices": S + r"\s*,\s*" + OUTS,
    "tqgpu_mpc_adjoint_matrices_batch": r"tqgpu_solver\s*\*\*\s*solvers\s*,\s*int\s+n\s*,\s*int\s+reduce\s*,\s*" + OUTS,
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers(capi):
    want = {"mpc_set_param_groups": ["self", "hgroup", "cgroup"], "mpc_adjoint_matrices": ["self"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    sig = inspect.signature(capi.TqGpu.mpc_set_param_groups)
    assert sig.parameters["hgroup"].default is None and sig.parameters["cgroup"].default is None
    assert list(inspect.signature(capi.mpc_adjoint_matrices_batch).parameters) == ["mirrors", "reduce"]
    assert inspect.signature(capi.mpc_adjoint_matrices_batch).parameters["reduce"].default is False


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    w = np.full(8, 7.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    i = np.full(8, 7, dtype=np.int32)
    ip = i.ctypes.data_as(C.POINTER(C.c_int))
    none = (C.c_void_p * 1)(None)
    for rc in (L.tqgpu_mpc_set_param_groups(None, None, None, 0, 0), L.tqgpu_mpc_get_param_groups(None, ip, ip, ip, ip, ip),
               L.tqgpu_mpc_adjoint_matrices(None, p, p, p, p, p, p, p), L.tqgpu_mpc_adjoint_matrices_batch(none, 1, 0, p, p, p, p, p, p, p)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert L.tqgpu_mpc_adjoint_matrices_batch(None, 1, 0, p, p, p, p, p, p, p) == -2
    assert L.tqgpu_mpc_adjoint_matrices_batch(none, 0, 0, p, p, p, p, p, p, p) == -2
    assert np.all(w == 7.0) and np.all(i == 7)


def test_the_header_documents_the_formulas_and_the_order_of_the_sum():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("dL = gz' dg + gb' db + gz' dH z + lam' (dE gz) + gb' (dE z)", "gHd_k[i] = gz_k[i] * z_k[i]", "gH_k = 1/2 (gz_k z_k' + z_k gz_k')",
                 "gA_c = lam_c gq_p' + gb_c x_p'", "gB_c = lam_c gr_p' + gb_c u_p'", "gA0_c = gb_c x0'", "gS0 = gr_0 x0'",
                 "acc = fma(lam_c[i], gz_p[j], acc);  acc = fma(gb_c[i], z_p[j], acc);", "ADJMAT_CHUNK = 64",
                 "The group's value is the plain sum of the partials in ascending chunk order", "ascending (member, chunk)", "No atomics are used anywhere"):
        assert word in text, word
    assert "are left to the caller" not in text

"""The MPC-step entry points (include/treeqp_amd.h: tqgpu_mpc_*, tqgpu_set_warm_start, tqgpu_get_root_terms): declared, exported,
wrapped.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("tqgpu_mpc_set_root", "tqgpu_mpc_set_x0", "tqgpu_set_warm_start", "tqgpu_get_warm_start", "tqgpu_get_root_terms",
           "tqgpu_mpc_step", "tqgpu_mpc_step_batch", "tqgpu_mpc_stats")


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), f"{name} is not declared in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_wrappers_have_the_documented_signatures(capi):
    want = {
        "mpc_set_root": ["self", "A0", "b0", "S0", "r0", "C0", "dmin0", "dmax0"],
        "mpc_set_x0": ["self", "x0"],
        "set_warm_start": ["self", "mode"],
        "root_terms": ["self", "nc0"],
        "mpc_step": ["self", "x0", "profile", "kw"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    assert isinstance(capi.TqGpu.warm_start, property)
    assert list(inspect.signature(capi.mpc_step_batch).parameters) == ["mirrors", "x0s", "profile", "kw"]
    assert list(inspect.signature(capi.mpc_stats).parameters) == []
    # TreeQp.set_x0, the host fold of the drop-in layer, stays as it is
    assert list(inspect.signature(capi.TreeQp.set_x0).parameters) == ["self", "x0"]


def test_stats_with_null_pointers(capi):
    L = capi.lib()
    assert L.tqgpu_mpc_stats(None, None, None) == 0
    v = [C.c_int(-1) for _ in range(3)]
    assert L.tqgpu_mpc_stats(*[C.byref(x) for x in v]) == 0
    assert all(x.value >= 0 for x in v)
    assert set(capi.mpc_stats()) == {"launches", "copies", "waits"}


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    x = np.zeros(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    for rc in (L.tqgpu_mpc_set_root(None, 4, p, p, None, None, None, None, None), L.tqgpu_mpc_set_x0(None, p),
               L.tqgpu_set_warm_start(None, 1), L.tqgpu_get_root_terms(None, p, None, None, None)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()


def test_numpy_fold_is_order_independent_on_the_exact_data():
    """the premise of the bit-for-bit fold test: with entries that are multiples of 2^-6 every product and partial sum is exact"""
    import mpc_cases as M
    for c in M.cases():
        rng = np.random.Generator(np.random.PCG64(7))
        for x0 in M.exact_x0s(c["nx0"], 0):
            ref = M.fold(c["root"], x0)
            for _ in range(3):
                got = M.fold(c["root"], x0, order=rng.permutation(c["nx0"]))
                for k in ref:
                    assert np.array_equal(got[k], ref[k]), (c["id"], k)
            for k in ("b0", "S0", "r0", "C0"):
                v = c["root"][k]
                if v is not None:
                    assert np.array_equal(v * 64, np.round(v * 64)) and np.max(np.abs(v), initial=0.0) <= 4
            assert all(np.array_equal(A * 64, np.round(A * 64)) and np.max(np.abs(A)) <= 4 for A in c["root"]["A0"])

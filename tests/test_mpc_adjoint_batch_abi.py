"""The entry point of the batched adjoint (include/treeqp_amd.h: tqgpu_mpc_adjoint_batch): declared, exported, wrapped, and the batches of
adj_batch_cases.py name cases that exist.  No device needed."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
D = r"double\s*\*\s*"
ARGS = (r"tqgpu_solver\s*\*\*\s*solvers\s*,\s*int\s+n\s*,\s*const\s+tqgpu_opts\s*\*\s*opts\s*,\s*const\s+" + D + r"wx\s*,\s*const\s+" + D +
        r"wu\s*,\s*int\s+nw\s*,\s*" + D + r"gx0\s*,\s*int\s*\*\s*n_reg")


def test_symbol_declared_and_exported(capi):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+tqgpu_mpc_adjoint_batch\s*\(\s*%s\s*\)\s*;" % ARGS, text, flags=re.M), "tqgpu_mpc_adjoint_batch is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), "tqgpu_mpc_adjoint_batch"), "tqgpu_mpc_adjoint_batch is not exported by the library"


def test_wrapper(capi):
    assert hasattr(capi, "mpc_adjoint_batch"), "capi.mpc_adjoint_batch is missing"
    sig = inspect.signature(capi.mpc_adjoint_batch)
    assert list(sig.parameters) == ["mirrors", "wxs", "wus", "profile", "kw"]
    assert sig.parameters["wxs"].default is None and sig.parameters["wus"].default is None and sig.parameters["profile"].default == 0


def test_bad_arguments_are_refused_with_a_message(capi):
    L = capi.lib()
    o = capi._gpu_opts(0)
    g = np.full(4, 7.0)
    p = g.ctypes.data_as(C.POINTER(C.c_double))
    a = (C.c_int * 1)(7)
    one = (C.c_void_p * 1)(None)
    for rc in (L.tqgpu_mpc_adjoint_batch(None, 1, C.byref(o), p, p, 1, p, a),          # no array of mirrors
               L.tqgpu_mpc_adjoint_batch(one, 0, C.byref(o), p, p, 1, p, a),           # n = 0
               L.tqgpu_mpc_adjoint_batch(one, 1, None, p, p, 1, p, a)):                # no options
        assert rc == -2 and b"tqgpu_mpc_adjoint_batch" in L.tqgpu_last_error()
    assert L.tqgpu_mpc_adjoint_batch(one, 1, C.byref(o), p, p, 0, p, a) == -2 and b"nw" in L.tqgpu_last_error()
    assert L.tqgpu_mpc_adjoint_batch(one, 1, C.byref(o), p, p, 1, p, a) == -2          # a null member
    assert b"member 0" in L.tqgpu_last_error() and b"null solver" in L.tqgpu_last_error()
    assert np.all(g == 7.0) and a[0] == 7


def test_the_batches_name_cases_that_exist():
    loaded = {m for m in sys.modules if m.startswith("treeqp_amd")}
    import adj_batch_cases as AB
    import adj_cases as AC
    assert {m for m in sys.modules if m.startswith("treeqp_amd")} == loaded, "adj_batch_cases loads the package on import"
    assert set(AB.BATCH_IDS) == {"mixed", "same4", "pair"}
    for bid, ids in AB.BATCHES.items():
        assert ids and all(cid in AC.CASE_IDS for cid in ids), bid
    assert len(AB.BATCHES["mixed"]) == 8 and len(set(AB.BATCHES["mixed"])) == 8
    assert AB.BATCHES["same4"] == ("elim-persist_c1",) * 4
    assert AB.BATCHES["pair"] == ("Nh1-three_leaves", "states-tiered_ub")

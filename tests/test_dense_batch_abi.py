"""The opt-in batch launch of dense trees at the C-ABI: include/treeqp_amd.h declares the setter and the getter, the built library
exports both, the Python binding has them, and no plan bit was added for it (no compute calls, no device)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "treeqp_amd.h"
FUNCTIONS = ("tqgpu_set_dense_batch_launch", "tqgpu_get_dense_batch_launch")


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_functions():
    code = _code(HEADER.read_text())
    assert re.search(r"\bint\s+tqgpu_set_dense_batch_launch\s*\(\s*tqgpu_solver\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+tqgpu_get_dense_batch_launch\s*\(\s*const\s+tqgpu_solver\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)\s*;", code)


def test_no_plan_bit_was_added():
    code = _code(HEADER.read_text())
    bits = sorted(int(b) for b in re.findall(r"#define\s+TQGPU_PLAN_\w+\s+\(1u\s*<<\s*(\d+)\)", code))
    assert bits == list(range(20))


def test_library_exports_both_symbols(capi):
    L = capi.lib()
    for n in FUNCTIONS:
        assert hasattr(L, n), n


def test_python_binding_has_the_option(capi):
    assert callable(getattr(capi.TqGpu, "set_dense_batch_launch", None)) and callable(getattr(capi.TqGpu, "dense_batch_launch", None))
    assert len(capi.TqGpu.PLAN_FLAGS) == 20 and capi.TqGpu.PLAN_FLAGS[17] == "last_single_wg"

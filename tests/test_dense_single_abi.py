"""The opt-in single-launch route of dense trees at the C-ABI: include/treeqp_amd.h declares the setter, the getter and the plan
bit, and the built library exports both functions (no compute calls, no device)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "treeqp_amd.h"
FUNCTIONS = ("tqgpu_set_dense_single_launch", "tqgpu_get_dense_single_launch")


def _code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_functions_and_the_plan_bit():
    code = _code(HEADER.read_text())
    assert re.search(r"\bint\s+tqgpu_set_dense_single_launch\s*\(\s*tqgpu_solver\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+tqgpu_get_dense_single_launch\s*\(\s*const\s+tqgpu_solver\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*,"
                     r"\s*int\s*\*\s*\w+\s*\)\s*;", code)
    m = re.search(r"#define\s+TQGPU_PLAN_DENSE_SINGLE_WG\s+\(1u\s*<<\s*(\d+)\)", code)
    assert m and int(m.group(1)) == 19
    # bits 0 .. 18 keep their values: the new bit is the only one above them
    bits = sorted(int(b) for b in re.findall(r"#define\s+TQGPU_PLAN_\w+\s+\(1u\s*<<\s*(\d+)\)", code))
    assert bits == list(range(20))


def test_library_exports_both_symbols(capi):
    L = capi.lib()
    for n in FUNCTIONS:
        assert hasattr(L, n), n


def test_python_binding_knows_the_plan_bit(capi):
    assert capi.TqGpu.PLAN_FLAGS[19] == "dense_single_wg" and capi.TqGpu.PLAN_FLAGS[17] == "last_single_wg"
    assert hasattr(capi.TqGpu, "set_dense_single_launch") and hasattr(capi.TqGpu, "dense_single_launch")

"""The entry points of the shifted warm start (include/treeqp_amd.h: tqgpu_shift_map, tqgpu_mpc_set_shift, tqgpu_mpc_set_realised,
tqgpu_mpc_get_shift, tqgpu_mpc_shift, tqgpu_get_working_sets, tqgpu_set_working_sets): declared, exported, wrapped, and the map against
the independent walk of paths of shift_cases.py.  No device needed."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import shift_cases as SH

ROOT = Path(__file__).resolve().parent.parent
S = r"tqgpu_solver\s*\*\s*s"
U = r"unsigned\s+long\s+long\s*\*\s*"
DECLARED = {
    "tqgpu_shift_map": r"int\s+Nn\s*,\s*const\s+int\s*\*\s*nk\s*,\s*const\s+int\s*\*\s*nx\s*,\s*int\s+realised\s*,\s*int\s+leaf\s*,\s*int\s*\*\s*img",
    "tqgpu_mpc_set_shift": S + r"\s*,\s*int\s+leaf\s*,\s*unsigned\s+what",
    "tqgpu_mpc_set_realised": S + r"\s*,\s*int\s+child",
    "tqgpu_mpc_get_shift": r"const\s+" + S + r"\s*,\s*int\s*\*\s*leaf\s*,\s*unsigned\s*\*\s*what\s*,\s*int\s*\*\s*realised",
    "tqgpu_mpc_shift": S,
    "tqgpu_get_working_sets": S + r"\s*,\s*" + U + r"bounds\s*,\s*" + U + r"rows\s*,\s*" + U + r"bound_sides\s*,\s*" + U + "row_sides",
    "tqgpu_set_working_sets": S + r"\s*,\s*const\s+" + U + r"bounds\s*,\s*const\s+" + U + r"rows\s*,\s*const\s+" + U + r"bound_sides\s*,\s*const\s+" + U + "row_sides",
}
MAP_CASES = SH.map_cases()
MAP_IDS = [c[0] for c in MAP_CASES]


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_declared_and_exported(capi, name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "treeqp_amd.h").read_text(), flags=re.S)
    assert re.search(r"^int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLARED[name]), text, flags=re.M), f"{name} is not declared as documented in treeqp_amd.h"
    assert hasattr(capi.lib(), name), f"{name} is not exported by the library"


def test_constants_and_wrappers(capi):
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for name, value in (("TQGPU_SHIFT_LEAF_REPEAT", capi.SHIFT_LEAF_REPEAT), ("TQGPU_SHIFT_LEAF_ZERO", capi.SHIFT_LEAF_ZERO),
                        ("TQGPU_SHIFT_DUALS", capi.SHIFT_DUALS), ("TQGPU_SHIFT_WORKING_SETS", capi.SHIFT_WORKING_SETS)):
        m = re.search(r"^#define\s+%s\s+(\d+)u?\s*$" % name, text, flags=re.M)
        assert m and int(m.group(1)) == value, name
    assert (capi.SHIFT_LEAF_REPEAT, capi.SHIFT_LEAF_ZERO) == (SH.REPEAT, SH.ZERO)
    want = {
        "mpc_set_shift": ["self", "leaf", "what"],
        "mpc_set_realised": ["self", "child"],
        "mpc_shift": ["self"],
        "working_sets": ["self"],
        "set_working_sets": ["self", "bounds", "rows", "bound_sides", "row_sides"],
        "set_warm_start": ["self", "mode"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(capi.TqGpu, name)).parameters) == params, name
    assert isinstance(capi.TqGpu.mpc_shift_state, property)
    assert list(inspect.signature(capi.shift_map).parameters) == ["nk", "nx", "realised", "leaf"]
    assert "2" in capi.TqGpu.set_warm_start.__doc__


def test_null_solver_is_refused_with_a_message(capi):
    L = capi.lib()
    w = np.full(4, 7, dtype=np.uint64)
    p = w.ctypes.data_as(C.POINTER(C.c_uint64))
    a, b, c = C.c_int(7), C.c_uint(7), C.c_int(7)
    for rc in (L.tqgpu_mpc_set_shift(None, 0, C.c_uint(1)), L.tqgpu_mpc_set_realised(None, 0), L.tqgpu_mpc_get_shift(None, C.byref(a), C.byref(b), C.byref(c)),
               L.tqgpu_mpc_shift(None), L.tqgpu_get_working_sets(None, p, p, p, p), L.tqgpu_set_working_sets(None, p, p, p, p)):
        assert rc == -2
        assert b"null solver" in L.tqgpu_last_error()
    assert np.all(w == 7) and (a.value, b.value, c.value) == (7, 7, 7)


def test_the_header_documents_the_map():
    text = (ROOT / "include" / "treeqp_amd.h").read_text()
    for word in ("img(0) = kid0[0] + j", "img(k) = kid0[img(p)] + min(c, nk[img(p)] - 1)", "TQGPU_SHIFT_LEAF_REPEAT", "a repeated leaf",
                 "nx[img(k)] != nx[k]", "dad(img(k)) == img(dad(k))", "img(k) > k for every node that takes a set", "tqgpu_set_warm_start(s, 2)",
                 "what P_k was last built for are not touched"):
        assert word in text, word


@pytest.mark.parametrize("leaf", [SH.REPEAT, SH.ZERO])
@pytest.mark.parametrize("cid", MAP_IDS)
def test_map_is_the_walk_of_paths(capi, cid, leaf):
    _, nk, nx = MAP_CASES[MAP_IDS.index(cid)]
    some = 0
    for j in range(max(int(nk[0]), 1)):
        img = capi.shift_map(nk, nx, j, leaf)
        want, rep = SH.ref_map(nk, nx, j, leaf)
        assert np.array_equal(img, want), f"{cid} realisation {j} leaf {leaf}: {img} != {want}"
        some += int(np.count_nonzero(img >= 0))
        if len(nk) == 1:
            continue
        # the properties: off the repeated leaves an image is one level deeper, lies beyond its node, and is the child of its parent's image
        dep, dad = SH.depths(nk), SH.dads(nk)
        for k in range(len(nk)):
            m = img[k]
            if m < 0:
                continue
            if rep[k]:
                assert leaf == SH.REPEAT and nk[m] == 0 and dep[m] == dep[k]
                continue
            assert dep[m] == dep[k] + 1 and m > k
            if k > 0 and img[dad[k]] >= 0:
                assert dad[m] == img[dad[k]], f"{cid}: dad(img({k})) != img(dad({k}))"
    if cid == "one_node" or (cid == "irregular_nx_by_level" and leaf == SH.ZERO):          # (every level has another nx: only a repeated leaf fits)
        assert some == 0
    else:
        assert some > 0


def test_what_the_cases_cover(capi):
    by = {c[0]: c for c in MAP_CASES}
    _, nk, nx = by["persist_c1_multistage"]
    img = capi.shift_map(nk, nx, 1, SH.REPEAT)
    k0 = SH.kid0(nk)
    clamped = [k for k in range(1, len(nk)) if img[k] >= 0 and nk[SH.dads(nk)[k]] > 1 and nk[img[SH.dads(nk)[k]]] == 1]
    assert clamped, "the multistage tree does not reach the clamp"
    assert any(img[k] == img[k + 1] for k in clamped if k + 1 < len(nk) and SH.dads(nk)[k] == SH.dads(nk)[k + 1])
    _, nk, nx = by["irregular_nx_by_level"]
    a, z = capi.shift_map(nk, nx, 0, SH.REPEAT), capi.shift_map(nk, nx, 0, SH.ZERO)
    assert np.all(a[nk > 0] == -1) and np.all(a[nk == 0] >= 0) and np.all(z == -1), (a, z)          # levels differ in nx; a leaf repeats itself
    _, nk, nx = by["chain"]
    assert np.array_equal(capi.shift_map(nk, nx, 0, SH.REPEAT), [1, 2, 3, 4, 4]) and np.array_equal(capi.shift_map(nk, nx, 0, SH.ZERO), [1, 2, 3, 4, -1])
    _, nk, nx = by["uniform_md2_depth3"]
    assert np.array_equal(capi.shift_map(nk, nx, 1, SH.ZERO)[:7], [2, 5, 6, 11, 12, 13, 14])
    assert len(capi.shift_map([0], [3], 0, SH.REPEAT)) == 0
    assert k0[0] == 1


def test_map_refusals(capi):
    L = capi.lib()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    nk, nx = np.asarray([2, 1, 1, 0, 0], dtype=np.int32), np.full(5, 3, dtype=np.int32)
    img = np.full(5, 9, dtype=np.int32)
    bad_nk = [np.asarray([2, 1, 1, 1, 0], dtype=np.int32), np.asarray([2, 0, 0, 0, 0], dtype=np.int32), np.asarray([2, -1, 2, 1, 0], dtype=np.int32),
              np.asarray([0, 2, 1, 1, 0], dtype=np.int32)]
    for rc in [L.tqgpu_shift_map(5, ip(nk), ip(nx), 2, 0, ip(img)), L.tqgpu_shift_map(5, ip(nk), ip(nx), -1, 0, ip(img)),
               L.tqgpu_shift_map(0, ip(nk), ip(nx), 0, 0, ip(img)), L.tqgpu_shift_map(5, ip(nk), ip(nx), 0, 2, ip(img)),
               L.tqgpu_shift_map(5, ip(nk), ip(nx), 0, 0, None)] + [L.tqgpu_shift_map(5, ip(b), ip(nx), 0, 0, ip(img)) for b in bad_nk]:
        assert rc == -2, L.tqgpu_last_error()
        assert b"tqgpu_shift_map" in L.tqgpu_last_error()
    assert np.all(img == 9)
    assert L.tqgpu_shift_map(5, ip(nk), ip(nx), 1, 1, ip(img)) == 0 and np.array_equal(img, [2, 4, 4, -1, -1])

"""The bound gradients of an MPC step on the device (tqgpu_mpc_get_adjoint_bounds, tqgpu_mpc_adjoint_bounds) against adjbnd_ref.dual evaluated
at the device's own exported point, and against itself.

Cases: adjbnd_cases.BOUND_TREES.  Tolerances: 10 times the spread of the two numpy evaluations on the CPU (adjbnd_cases.SPREAD, measured by
test_adjbnd_reference.py), floor 1e-12.  Everything the header promises bit for bit is compared bit for bit."""
import numpy as np
import pytest

import adj_cases as AC
import adjbnd_cases as BC
import adjbnd_ref as BR
import adjmat_cases as XC
import adjmat_ref as AM
import sens_cases as SN

pytestmark = pytest.mark.gpu

EINVAL = -2
SIDES = ("gxmin", "gxmax", "gumin", "gumax")


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}: differs by {np.max(np.abs(a - b), initial=0.0):.3e}"


def _counts(capi):
    st = capi.mpc_stats()
    return st["launches"], st["copies"], st["waits"]


def _ready(capi, c, w=None):
    g = SN.make(capi, c)
    r, _ = g.mpc_step(c["x0"], **c["base"]["opts"])
    assert r["status"] == 0
    out = g.mpc_adjoint(*(c["w"] if w is None else w), **c["base"]["opts"])
    return g, out


def _stacked(got):
    """(lower, upper) over [x | u]"""
    return np.vstack([got["gxmin"], got["gumin"]]), np.vstack([got["gxmax"], got["gumax"]])


@pytest.mark.parametrize("tree", BC.BOUND_TREES)
def test_against_the_reference_and_the_grouped_sums(capi, tree):
    c = BC.bound_case(tree)
    g, adj = _ready(capi, c)
    try:
        sol = g.solution()
        got = g.mpc_get_adjoint_bounds()
        grads = g.mpc_adjoint_grads()
        ref = BR.dual(c["d"], sol["x"], sol["u"], c["param"], c["w"], c["kinds"])
        assert ref["n_reg"] == 0
        lo, hi = _stacked(got)
        for name, x, y in (("lower", lo, ref["lo"]), ("upper", hi, ref["hi"])):
            err = float(np.max(np.abs(x - y)))
            print(f"{tree} {name}: |device - (b)| = {err:.3e}, tolerance {BC.tol(tree, 0):.3e}")
            assert x.shape == y.shape and err <= BC.tol(tree, 0)
        # bit for bit: zero off the bounds and on kind-1 nodes, complementary to gq / gr, glb of a root with states is gx0
        on_lo, on_hi = BR.sides(c["d"], sol["x"], sol["u"], c["kinds"])
        assert np.all(lo[~on_lo] == 0.0) and np.all(hi[~on_hi] == 0.0)
        gz = np.vstack([grads["gq"], grads["gr"]])
        assert np.all(gz[(lo != 0.0)[:, 0] | (hi != 0.0)[:, 0]] == 0.0) and np.all(gz[on_lo | on_hi] == 0.0)
        if c["kinds"] is None or np.any(np.asarray(c["kinds"]) == 0):          # every tree with a kind-0 node: `mixed` too
            assert np.any(lo != 0.0) or np.any(hi != 0.0)
        if tree == "mixed":
            assert np.any(lo != 0.0) and np.any(hi != 0.0)
        if c["form"] == "states":
            _same_bits(got["gxmin"][:c["nx0"]], adj["gx0"], f"{tree}: glb of the root's states against gx0")
        # every node its own group: the getter, bit for bit
        g.mpc_set_param_groups(None, None)
        per = g.mpc_adjoint_bounds()
        assert _counts(capi) == (1, 1, 1)
        hd = np.zeros(5 * len(g.nk), dtype=np.int32)
        import ctypes as C
        assert capi.lib().tqgpu_mpc_get_param_groups(g.h, None, None, hd.ctypes.data_as(C.POINTER(C.c_int)), None, None) == 0
        pad = int(hd[2])
        for key, full in (("glb", lo), ("gub", hi)):
            blocks = BR.node_blocks(c["d"], full, c["kinds"])
            for k, (x, y) in enumerate(zip(per[key], blocks)):
                front = pad if k == 0 else 0
                assert np.all(x[:front] == 0.0), (key, k)
                _same_bits(x[front:], y, f"{tree}: {key} of node {k}")
        # shared groups against the chunked sums of the reference
        hg, cg = AM.shared(c["d"], c["kinds"], pad)
        g.mpc_set_param_groups(hg, cg)
        sh = g.mpc_adjoint_bounds()
        multi = any(len(m) > AM.CHUNK for m in AM.members(hg, AM.n_groups(hg)))
        assert _counts(capi) == (2 if multi else 1, 1, 1)
        for key, full in (("glb", ref["lo"]), ("gub", ref["hi"])):
            want = BR.group_sums(c["d"], full, hg, c["kinds"])
            for gi, (x, y) in enumerate(zip(sh[key], want)):
                front = pad if 0 in np.flatnonzero(hg == gi) else 0
                err = float(np.max(np.abs(x[front:] - y), initial=0.0))
                assert err <= BC.tol(tree, 1), (key, gi, err)
                if c["kinds"] is not None and c["kinds"][np.flatnonzero(hg == gi)[0]] == 1:
                    assert np.all(x == 0.0)
    finally:
        g.close()


def test_a_group_of_64_members_and_of_65(capi):
    c = BC.bound_case("chain66")
    g, _ = _ready(capi, c)
    try:
        got = g.mpc_get_adjoint_bounds()
        blocks = [BR.node_blocks(c["d"], v, None) for v in _stacked(got)]
        for members, launches in ((64, 1), (65, 2)):
            hg, cg = np.full(66, -1), np.full(66, -1)
            hg[:members] = 0
            g.mpc_set_param_groups(hg, cg)
            out = g.mpc_adjoint_bounds()
            assert _counts(capi) == (launches, 1, 1)
            for key, blk in zip(("glb", "gub"), blocks):
                first = np.zeros_like(blk[0])
                for k in range(min(members, 64)):
                    first = first + blk[k]
                want = first if members == 64 else first + (np.zeros_like(blk[0]) + blk[64])
                _same_bits(out[key][0], want, f"{members} members: {key}")
    finally:
        g.close()


def test_columns_the_stored_factor_and_what_is_left_alone(capi):
    c = AC.case("states-generic")
    wx, wu = c["w3"]
    g, _ = _ready(capi, c, (wx, wu))
    try:
        g.mpc_set_param_groups(None, None)
        g.mpc_sensitivity(**c["base"]["opts"])
        gain, sens = g.mpc_gain(), g.mpc_sensitivities()
        stored = g.mpc_adjoint(wx, wu, **c["base"]["opts"])          # gx0, n_reg of the stored adjoint
        all3, mat = g.mpc_get_adjoint_bounds(), g.mpc_adjoint_matrices()
        grads, kkt, sol = g.mpc_adjoint_grads(), g.kkt_residual(), g.solution()
        gx0 = np.zeros(c["nx0"] * 3)
        import ctypes as C
        x0p = gx0.ctypes.data_as(C.POINTER(C.c_double))
        sums = g.mpc_adjoint_bounds()
        g.mpc_get_adjoint_bounds()
        assert capi.lib().tqgpu_mpc_get_adjoint_x0(g.h, x0p) == 0
        _same_bits(gx0.reshape((c["nx0"], 3), order="F"), stored["gx0"], "gx0 after tqgpu_mpc_adjoint_bounds")
        for i in range(3):
            _same_bits(g.mpc_gain()[i], gain[i], f"mpc_gain[{i}] after tqgpu_mpc_adjoint_bounds")
        for key in ("dx", "du", "dlam"):
            _same_bits(g.mpc_sensitivities()[key], sens[key], f"{key} after tqgpu_mpc_adjoint_bounds")
        for key in ("gq", "gr", "gb"):
            _same_bits(g.mpc_adjoint_grads()[key], grads[key], f"{key} after tqgpu_mpc_adjoint_bounds")
        _same_bits(g.kkt_residual()["res"], kkt["res"], "the KKT residual after tqgpu_mpc_adjoint_bounds")
        again = g.mpc_adjoint_matrices()
        for key in AM.KEYS:
            for x, y in zip(again[key], mat[key]):
                _same_bits(x, y, f"{key} of tqgpu_mpc_adjoint_matrices after tqgpu_mpc_adjoint_bounds")
        for j in range(3):
            g.mpc_adjoint(wx[:, j], wu[:, j], **c["base"]["opts"])          # (the factor is stored by now)
            one, one_sum = g.mpc_get_adjoint_bounds(), g.mpc_adjoint_bounds()
            for key in SIDES:
                _same_bits(one[key][:, 0], all3[key][:, j], f"column {j} of {key}")
            for key in ("glb", "gub"):
                for x, y in zip(one_sum[key], sums[key]):
                    _same_bits(x[:, 0], y[:, j], f"column {j} of {key}")
        # factor stored against factor built
        h, _ = _ready(capi, c, (wx, wu))
        try:
            built = h.mpc_get_adjoint_bounds()
            h.mpc_adjoint(wx, wu, **c["base"]["opts"])
            stored = h.mpc_get_adjoint_bounds()
            for key in SIDES:
                _same_bits(stored[key], built[key], f"{key}: factor stored against factor built")
                _same_bits(built[key], all3[key], f"{key}: a second mirror")
            r, _ = h.mpc_step(c["x0"], **c["base"]["opts"])
            r2, _ = g.mpc_step(c["x0"], **c["base"]["opts"])
            for k in ("x", "u", "lam"):
                _same_bits(h.solution()[k], g.solution()[k], f"{k} of the next solve")
                _same_bits(g.solution()[k], sol[k], f"{k} of the next solve against the last")
        finally:
            h.close()
    finally:
        g.close()


@pytest.mark.parametrize("trees", [("states-single_wg", "states-xbound"), ("elim-single_wg", "Nh1-one_leaf", "states-generic")])
def test_a_batch_leaves_every_member_its_own_call(capi, trees):
    cs = [BC.bound_case(t) for t in trees]
    gs = [_ready(capi, c)[0] for c in cs]
    try:
        single = [g.mpc_get_adjoint_bounds() for g in gs]
        for g, c in zip(gs, cs):
            g.mpc_step(c["x0"], **c["base"]["opts"])
        capi.mpc_adjoint_batch(gs, [c["w"][0] for c in cs], [c["w"][1] for c in cs], **cs[0]["base"]["opts"])
        for t, g, want in zip(trees, gs, single):
            got = g.mpc_get_adjoint_bounds()
            for key in SIDES:
                _same_bits(got[key], want[key], f"{t}: {key} after the batch")
    finally:
        for g in gs:
            g.close()


def test_refusals(capi):
    c = BC.bound_case("states-single_wg")
    g = SN.make(capi, c)
    try:
        L = capi.lib()
        g.mpc_step(c["x0"], **c["base"]["opts"])
        assert L.tqgpu_mpc_get_adjoint_bounds(g.h, None, None, None, None) == EINVAL          # no adjoint
        g.mpc_set_param_groups(None, None)
        assert L.tqgpu_mpc_adjoint_bounds(g.h, None, None) == EINVAL
        g.mpc_adjoint(*c["w"], **c["base"]["opts"])
        assert L.tqgpu_mpc_get_adjoint_bounds(g.h, None, None, None, None) == 0 and L.tqgpu_mpc_adjoint_bounds(g.h, None, None) == 0
        g.upload(c["base"]["d"])                                                              # after an upload
        assert L.tqgpu_mpc_get_adjoint_bounds(g.h, None, None, None, None) == EINVAL and L.tqgpu_mpc_adjoint_bounds(g.h, None, None) == EINVAL
    finally:
        g.close()
    h = SN.make(capi, c)
    try:
        h.mpc_step(c["x0"], **c["base"]["opts"])
        h.mpc_adjoint(*c["w"], **c["base"]["opts"])
        assert capi.lib().tqgpu_mpc_adjoint_bounds(h.h, None, None) == EINVAL                 # no groups
    finally:
        h.close()

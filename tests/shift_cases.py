"""The shift of the warm start (tqgpu_shift_map, tqgpu_mpc_set_shift, tqgpu_mpc_shift): trees for the map, an independent Python walk of
paths it is compared with, and the numpy gathers of duals and working sets that the device is compared with (test_mpc_shift_abi.py,
test_gpu_mpc_shift.py).

The walk: the path of node k is the list of sibling indices from the root down to k.  After child j of the root became the root, node k of
the new problem stands where the node with path (j, path(k)) stood in the old one; an index beyond the children of a node is clamped, and a
path that runs on below a leaf stays on that leaf (REPEAT) or has no image (ZERO)."""
from __future__ import annotations

import numpy as np

REPEAT, ZERO = 0, 1


def kid0(nk):
    nk = np.asarray(nk, dtype=int)
    return 1 + np.concatenate([[0], np.cumsum(nk)[:-1]])


def dads(nk):
    nk = np.asarray(nk, dtype=int)
    dad, k0 = np.full(len(nk), -1, dtype=int), kid0(nk)
    for p, n in enumerate(nk):
        dad[k0[p]:k0[p] + n] = p
    return dad


def depths(nk):
    dad = dads(nk)
    dep = np.zeros(len(dad), dtype=int)
    for k in range(1, len(dad)):
        dep[k] = dep[dad[k]] + 1
    return dep


def path(nk, k):
    dad, k0 = dads(nk), kid0(nk)
    out = []
    while k > 0:
        out.append(k - k0[dad[k]])
        k = dad[k]
    return out[::-1]


def ref_map(nk, nx, j, leaf):
    """(img, rep) by the walk of paths; rep[k]: the image is a repeated leaf"""
    nk, nx = np.asarray(nk, dtype=int), np.asarray(nx, dtype=int)
    k0 = kid0(nk)
    img, rep = np.full(len(nk), -1, dtype=int), np.zeros(len(nk), dtype=bool)
    if len(nk) == 1:
        return img[:0], rep[:0]
    for k in range(len(nk)):
        node, repeated = 0, False
        for c in [j] + path(nk, k):
            if nk[node] > 0:
                node = k0[node] + min(c, nk[node] - 1)
            elif leaf == REPEAT:
                repeated = True
            else:
                node = -1
                break
        if node >= 0 and nx[node] == nx[k]:
            img[k], rep[k] = node, repeated
    return img, rep


def uniform(md, depth):
    nk = []
    for lvl in range(depth + 1):
        nk += [md if lvl < depth else 0] * md ** lvl
    return np.asarray(nk, dtype=np.int32)


def multistage(md, Nr, Nh):
    """branching by md for Nr stages, then chains down to stage Nh (the shape of the spring-mass trees)"""
    nk = []
    for lvl in range(Nh + 1):
        nk += [0 if lvl == Nh else md if lvl < Nr else 1] * md ** min(lvl, Nr)
    return np.asarray(nk, dtype=np.int32)


def map_cases():
    """(id, nk, nx)"""
    from treeqp_amd import problems as P
    c1 = P.spring_mass()
    out = [("uniform_md2_depth3", uniform(2, 3), np.full(15, 4)),
           ("persist_c1_multistage", np.asarray(c1.nk(), dtype=np.int32), np.full(c1.Nn, c1.nx)),
           ("chain", np.asarray([1, 1, 1, 1, 0], dtype=np.int32), np.full(5, 3)),
           ("one_node", np.asarray([0], dtype=np.int32), np.asarray([3])),
           ("irregular_nx_by_level", np.asarray([2, 1, 2, 1, 1, 1, 0, 0, 0], dtype=np.int32), np.asarray([2, 3, 3, 4, 4, 4, 5, 5, 5])),
           ("eliminated_root", np.asarray([3, 1, 1, 1, 0, 0, 0], dtype=np.int32), np.asarray([0, 2, 3, 2, 2, 2, 2]))]
    return out


# ---- the numpy gathers ----
def gather_lam(nx, img, lam):
    """the start duals in the layout of tqgpu_set_lambda (nodes 1 .. Nn - 1): those of img(k), 0.0 where there is none"""
    nx = np.asarray(nx, dtype=int)
    off = np.concatenate([[0], np.cumsum(nx[1:])])          # node k >= 1 at off[k - 1]
    out = np.zeros_like(lam)
    for k in range(1, len(nx)):
        m = img[k]
        if m >= 1:
            out[off[k - 1]:off[k - 1] + nx[k]] = lam[off[m - 1]:off[m - 1] + nx[m]]
        # (m == 0 cannot be: an image is at least one level deep)
    return out


def gather_sets(nx, nu, nc, kinds, img, rep, ws):
    """the working sets after the shift: node k takes bounds and bound_sides of img(k) where both are of kind 2 or 3, nx and nu agree, the
    image exists and is no repeated leaf; rows and row_sides where moreover both are of kind 3 and nc agrees; every other node keeps its own"""
    out = {k: np.array(v, copy=True) for k, v in ws.items()}
    for k in range(len(nx)):
        m = img[k]
        if m < 0 or rep[k] or kinds[k] < 2 or kinds[m] < 2 or nx[k] != nx[m] or nu[k] != nu[m]:
            continue
        assert m > k
        out["bounds"][k], out["bound_sides"][k] = ws["bounds"][m], ws["bound_sides"][m]
        if kinds[k] == 3 and kinds[m] == 3 and nc[k] == nc[m]:
            out["rows"][k], out["row_sides"][k] = ws["rows"][m], ws["row_sides"][m]
    return out

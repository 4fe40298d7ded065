"""The tree shapes on both sides of every kernel-selection limit of tqgpu_create's steps (detect_shape, setup_per_phase, setup_wide3,
setup_persist, setup_single_wg in tdunes_device.hip), shared by the CPU reference
checks (test_limits_reference.py) and the device tests (test_gpu_limits.py).

A shape is written as a nested node (nx, nu, [children]); `flatten` lays it out breadth first.  Each row of ROWS is
(limit, [(side id, problem kind, shape, flags the plan must show)]); a flag missing from the dict is not asserted."""
from __future__ import annotations

import numpy as np


def leaf(nx):
    return (nx, 0, [])


def flatten(root):
    nk, nx, nu, level = [], [], [], [root]
    while level:
        nxt = []
        for n, m, kids in level:
            nk.append(len(kids)); nx.append(n); nu.append(m if kids else 0)
            nxt += kids
        level = nxt
    return np.asarray(nk, np.int32), np.asarray(nx, np.int32), np.asarray(nu, np.int32)


def fan(m, kid_nx, kid_nu=2, root=(3, 2), grand=2):
    """root with m children of nx kid_nx[i] (an int: all the same), each with one leaf of nx `grand`"""
    kid_nx = [kid_nx] * m if np.isscalar(kid_nx) else list(kid_nx)
    return (root[0], root[1], [(n, kid_nu, [leaf(grand)]) for n in kid_nx])


def path_tree(depth):
    """root with three children of nx 6 (d = 18: the wide class), each heading a chain whose deepest PARENT is at `depth`
    (nx 3 below the children: every other block is 3 x 3)"""
    def chain():
        node = leaf(3)
        for _ in range(depth - 1):
            node = (3, 1, [node])
        return node
    return (4, 2, [(6, 2, [chain()]) for _ in range(3)])


def chains(m, L, nx, nu, nx1):
    """root (nx, nu) with m chains of L nodes below it; node 1 has nx1 states (not a uniform tree)"""
    def chain(n0):
        node = leaf(nx)
        for i in range(L - 1):
            node = (n0 if i == L - 2 else nx, nu, [node])
        return node
    return (nx, nu, [chain(nx1)] + [chain(nx) for _ in range(m - 1)])


def levels(widths):
    """a tree whose level l has widths[l] nodes (non-decreasing), all of nx = nu = 1: the first nodes of each level take the
    surplus children"""
    cur = [leaf(1) for _ in range(widths[-1])]
    for w in reversed(widths[:-1]):
        per = [len(cur) // w + (1 if i < len(cur) % w else 0) for i in range(w)]
        nxt, c = [], 0
        for p in per:
            nxt.append((1, 1, cur[c:c + p])); c += p
        cur = nxt
    assert len(cur) == 1
    return cur[0]


def dense_pair(nx, nu):
    """root (nx, nu) -> (8, 2) -> leaf (4): a dense root of nz = nx + nu with a 4 x 4 block below"""
    return (nx, nu, [(8, 2, [leaf(4)])])


C = "clip"
D = "dense"
ROWS = [
    ("wide class, d", [
        ("d16", C, (3, 2, [(8, 2, [leaf(2)]), (8, 2, [leaf(2)])]), dict(wide=False)),
        ("d17", C, (3, 2, [(8, 2, [leaf(2)]), (9, 2, [leaf(2)])]), dict(wide=True, wide_small=False, w3=True)),
        ("d64", C, fan(8, 8), dict(wide=True, w3=True)),
        ("d65", C, fan(8, [8] * 7 + [9]), dict(wide=False, w3=False)),
    ]),
    ("wide class, parent nx+nu", [
        ("nz32", C, (20, 12, [(20, 2, [leaf(2)])]), dict(wide=True, w3=True)),
        ("nz33", C, (20, 13, [(20, 2, [leaf(2)])]), dict(wide=False, w3=False)),
    ]),
    ("three-launch, any nx", [
        ("leaf_nx32", C, (4, 2, [(8, 4, [leaf(32)])]), dict(wide=True, w3=True, w3_sgp=True)),
        ("leaf_nx33", C, (4, 2, [(8, 4, [leaf(33)])]), dict(wide=True, w3=False)),
    ]),
    ("k_sgp children", [
        ("kids4", C, fan(4, 5, root=(4, 2)), dict(w3_sgp=True, sgp_accs=4 * 6)),
        ("kids5", C, fan(5, 4, root=(4, 2)), dict(w3_sgp=True, sgp_accs=5 * 6)),
        ("kids8", C, fan(8, 3, kid_nu=1, root=(4, 2)), dict(w3_sgp=True, sgp_accs=8 * 6)),
        ("kids9", C, fan(9, 3, kid_nu=1, root=(4, 2)), dict(w3_sgp=True, sgp_accs=8 * 6)),
        ("kids16_d64", C, fan(16, 4, kid_nu=1, root=(4, 2)), dict(w3_sgp=True, sgp_accs=8 * 6)),
    ]),
    ("k_sgp, nx+nu", [
        # one side only: the gate is unreachable (see test_gpu_limits.test_both_sides_of_the_limit_match_the_oracle)
        ("nz32_everywhere", C, (20, 12, [leaf(32)]), dict(w3=True, w3_sgp=True)),
    ]),
    ("forward chain", [
        ("nx8", C, (4, 2, [(8, 2, [leaf(3)]), (8, 2, [leaf(3)]), (8, 2, [leaf(3)])]), dict(w3=True, fwd_chain=True, w3_merge=True)),
        ("nx9", C, (4, 2, [(8, 2, [leaf(3)]), (8, 2, [leaf(3)]), (9, 2, [leaf(3)])]), dict(w3=True, fwd_chain=False, w3_merge=False)),
        ("path16", C, path_tree(16), dict(w3=True, fwd_chain=True)),
        ("path17", C, path_tree(17), dict(w3=True, fwd_chain=False)),
        ("bdim3", C, (4, 2, [(6, 2, [leaf(3)]), (6, 2, [leaf(3)]), (6, 2, [leaf(3)])]), dict(w3=True, fwd_chain=True)),
        ("bdim2", C, (4, 2, [(6, 2, [leaf(3)]), (6, 2, [leaf(3)]), (6, 2, [leaf(2)])]), dict(w3=True, fwd_chain=False)),
    ]),
    ("g_persist node sizes", [
        ("nz16", C, (4, 2, [(8, 8, [leaf(3)]), (6, 2, [leaf(3)])]), dict(wide=False, gpersist=True, gp_small16=True)),
        ("nz17", C, (4, 2, [(8, 9, [leaf(3)]), (6, 2, [leaf(3)])]), dict(wide=False, gpersist=True, gp_small16=False)),
        ("nx8", C, (4, 2, [(8, 2, [leaf(3)]), (7, 2, [leaf(3)])]), dict(wide=False, gpersist=True, gp_small16=True, gp_small8=True)),
        ("nx9", C, (4, 2, [(9, 2, [leaf(3)]), (6, 2, [leaf(3)])]), dict(wide=False, gpersist=True, gp_small16=True, gp_small8=False)),
    ]),
    ("widest level", [
        ("w96", C, levels([1, 8, 96]), dict(gpersist=True, wide=False)),
        ("w97", C, levels([1, 8, 97]), dict(gpersist=False, wide=True, wide_small=True, w3=True)),
    ]),
    ("g_persist LDS", [
        ("const_in_lds", C, chains(2, 48, 4, 2, 3), dict(gpersist=True, gp_state_lds=True, gp_const_lds=True)),
        ("state_in_lds", C, chains(2, 49, 4, 2, 3), dict(gpersist=True, gp_state_lds=True, gp_const_lds=False)),
        ("state_in_lds_last", C, chains(2, 67, 4, 2, 3), dict(gpersist=True, gp_state_lds=True)),
        ("tables_in_lds", C, chains(2, 68, 4, 2, 3), dict(gpersist=True, gp_state_lds=False, gp_tables_lds=True)),
        ("tables_in_lds_last", C, chains(4, 85, 8, 4, 7), dict(gpersist=True, gp_state_lds=False, gp_tables_lds=True)),
        ("nothing_in_lds", C, chains(4, 86, 8, 4, 7), dict(gpersist=True, gp_state_lds=False, gp_tables_lds=False)),
    ]),
    ("FUSE_MAX", [
        ("n512", C, levels([1, 2, 4, 8, 16, 32, 64, 128, 128, 129]), dict(fuse=True, wide=False, gpersist=False)),
        ("n513", C, levels([1, 2, 4, 8, 16, 32, 64, 128, 128, 130]), dict(fuse=False, wide=False, gpersist=False)),
    ]),
    ("root fan-out", [
        ("fan64", C, fan(64, 1, kid_nu=1, root=(2, 1), grand=1), dict(wide=True, w3=True, w3_sgp=True, sgp_accs=8 * 3)),
        ("fan100", C, fan(100, 1, kid_nu=1, root=(2, 1), grand=1), dict(wide=False, w3=False, gpersist=False)),
    ]),
    ("dense kind 1, nx+nu", [
        ("nz64", D, dense_pair(40, 24), dict(dense=True, box=False)),
        ("nz65", D, dense_pair(40, 25), dict(dense=True, box=False)),
        ("nz90", D, dense_pair(60, 30), dict(dense=True, box=False)),
        ("nz91", D, dense_pair(60, 31), dict(dense=True, box=False)),
        ("nz120", D, dense_pair(80, 40), dict(dense=True, box=False)),
        ("nz142", D, dense_pair(100, 42), dict(dense=True, box=False)),
    ]),
]

# the generic factorization's LDS (160 KiB per workgroup): a root block of d = 141 is the largest that k_forward holds
# ((d | 1) d + 2 d + nx + 2 doubles), d = 142 the smallest refused
FACTOR_ACCEPTED = (2, 1, [leaf(47)] * 3)
FACTOR_REFUSED = (2, 1, [leaf(47), leaf(47), leaf(48)])
# a dense unconstrained node of nx + nu = 143 does not fit k_dense_init's LDS (H and the pivots: (nz (nz + 1) + 2) doubles)
DENSE_REFUSED = dense_pair(100, 43)


def cases():
    for row, sides in ROWS:
        for sid, kind, shape, flags in sides:
            yield f"{row.split(',')[0].replace(' ', '_')}-{sid}", kind, shape, flags


def case(cid):
    """(kind, shape, flags) of the case with id `cid`"""
    for c, kind, shape, flags in cases():
        if c == cid:
            return kind, shape, flags
    raise KeyError(cid)


def problem(kind, shape, seed=11):
    from helpers import dense_shaped_qp, shaped_qp
    nk, nx, nu = flatten(shape)
    if kind == C:
        return shaped_qp(nk, nx, nu, seed, ubound=0.3).as_dict()
    return dense_shaped_qp(nk, nx, nu, seed)

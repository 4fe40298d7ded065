"""The adjoint of a tree QP's solution in the matrices H, A, B (and A0, S0 of an eliminated root), two ways in numpy, for w = dL/dz of a
scalar loss of z = [x | u] at a point with the active set frozen there:
(a) dense: the KKT system K [z; lam; mu] = [-g; -b; fix] of adj_ref.dense_kkt solved forward (lstsq) and transposed (K' a = [w; 0; 0]);
    dL/dtheta = -a' (dK/dtheta) [z; lam; mu] + a' d rhs / dtheta, with dK applied entry by entry: an entry of H_k, of A_c or B_c (it sits in E
    and in E'), of A0 (through b) and of S0 (through r[0]);
(b) outer: the formulas of include/treeqp_amd.h from adj_ref.dual_form's gq, gr, gb and the solver's own lam, grouped and summed
    in the stated order: members ascending in chunks of CHUNK, a chunk's partial one chain from 0.0, the partials added in ascending order.
Both return a dict of lists, one array per group with the column of w as the last axis, as treeqp_amd.capi.TqGpu.mpc_adjoint_matrices
does: gH ((nz, nw) for a kind-0 group: the diagonal; (nz, nz, nw) for a kind-1 group), gh, gA, gB, gb, gA0 (one array per child of the root), gS0.  pad: phantom root states
the device counts in front of node 0 (their entries are 0.0)."""
from __future__ import annotations

import numpy as np

import adj_ref as AR
import sens_ref as SR

CHUNK = 64
KEYS = ("gH", "gh", "gA", "gB", "gb", "gA0", "gS0")


def members(group, n):
    group = np.asarray(group, dtype=int)
    return [np.flatnonzero(group == g) for g in range(n)]


def n_groups(group):
    return int(np.max(group, initial=-1)) + 1


def per_node(Nn):
    return np.arange(Nn), np.arange(Nn) - 1


def shared(d, kinds=None, pad=0):
    """one group for all nodes of equal sizes (and kind): the coarsest maps the sizes allow"""
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    from treeqp_amd import problems as P
    dad = P.parents_of(nk)
    kinds = np.zeros(len(nk), dtype=int) if kinds is None else np.asarray(kinds, dtype=int)
    hk, ck, hg, cg = {}, {}, [], [-1]
    for k in range(len(nk)):
        hg.append(hk.setdefault((int(nx[k]), int(nu[k]), int(kinds[k]), pad if k == 0 else 0), len(hk)))
        if k > 0:
            p = dad[k]
            cg.append(ck.setdefault((int(nx[k]), int(nx[p]) + (pad if p == 0 else 0), int(nu[p])), len(ck)))
    return np.asarray(hg), np.asarray(cg)


def _chunked(terms):
    """terms: one list of addends per member (each member adds its addends in order); chunks of CHUNK members, partials added ascending"""
    total = None
    for at in range(0, len(terms), CHUNK):
        acc = np.zeros_like(terms[0][0])
        for member in terms[at:at + CHUNK]:
            for v in member:
                acc = acc + v
        total = acc if total is None else total + acc
    return total


def _node_vectors(t, x, u, g, k, j, pad):
    """z_k and gz_k of column j, phantom entries (0) in front of node 0"""
    xo, uo = t["xo"], t["uo"]
    front = np.zeros(pad if k == 0 else 0)
    z = np.concatenate([front, x[xo[k]:xo[k + 1]], u[uo[k]:uo[k + 1]]])
    gz = np.concatenate([front, g["gq"][xo[k]:xo[k + 1], j], g["gr"][uo[k]:uo[k + 1], j]])
    return z, gz


def _group_sums(t, x, u, lamf, g, hgroup, cgroup, x0, param, pad, node_H, edge_AB):
    """the grouping and the order of the sums, shared by (a) and (b): node_H(k, j) -> (gH_k or gHd_k, gh_k), edge_AB(c, j) -> (gA, gB, gb)"""
    nw = g["gq"].shape[1]
    out = {key: [] for key in KEYS}
    for mem in members(hgroup, n_groups(hgroup)):
        cols = [[node_H(k, j) for k in mem] for j in range(nw)]
        out["gH"].append(np.stack([_chunked([[v[0]] for v in col]) for col in cols], axis=-1))
        out["gh"].append(np.stack([_chunked([[v[1]] for v in col]) for col in cols], axis=-1))
    for mem in members(cgroup, n_groups(cgroup)):
        cols = [[edge_AB(c, j) for c in mem] for j in range(nw)]
        for i, key in enumerate(("gA", "gB", "gb")):
            out[key].append(np.stack([_chunked([v[i] if isinstance(v[i], list) else [v[i]] for v in col]) for col in cols], axis=-1))
    if param["form"] == "eliminated":
        nk0, xo, nx0 = int(t["nk"][0]), t["xo"], len(x0)
        for c in range(1, 1 + nk0):
            rows = np.arange(xo[c], xo[c + 1]) - t["nx"][0]
            out["gA0"].append(np.stack([np.outer(g["gb"][rows, j], x0) for j in range(nw)], axis=-1))
        nu0 = int(t["nu"][0])
        out["gS0"].append(np.stack([np.outer(g["gr"][:nu0, j], x0) if param.get("S0") is not None else np.zeros((nu0, nx0)) for j in range(nw)], axis=-1))
    return out


def outer(d, x, u, lam, param, g, kinds=None, hgroup=None, cgroup=None, x0=None, pad=0):
    """(b): lam is the solver's (tqgpu_get_solution's), in the sign the formulas take it"""
    t = SR._assemble(d, kinds)
    xo, dad = t["xo"], t["dad"]
    lamf = np.asarray(lam, dtype=np.float64)
    nx0r = int(t["nx"][0])

    def node_H(k, j):
        z, gz = _node_vectors(t, x, u, g, k, j, pad)
        if t["kinds"][k] == 0:
            return gz * z, gz
        return 0.5 * (np.outer(gz, z) + np.outer(z, gz)), gz

    def edge_AB(c, j):
        p = dad[c]
        zp, gzp = _node_vectors(t, x, u, g, p, j, pad)
        nxp = int(t["nx"][p]) + (pad if p == 0 else 0)
        rows = np.arange(xo[c], xo[c + 1]) - nx0r
        lc, gbc = lamf[rows], g["gb"][rows, j]
        return [np.outer(lc, gzp[:nxp]), np.outer(gbc, zp[:nxp])], [np.outer(lc, gzp[nxp:]), np.outer(gbc, zp[nxp:])], gbc

    return _group_sums(t, x, u, lamf, g, hgroup, cgroup, x0, param, pad, node_H, edge_AB)


def dense(d, x, u, param, w, kinds=None, hgroup=None, cgroup=None, x0=None, pad=0):
    """(a): returns (the dict, lam of the forward KKT solve in the sign H z + g + E' lam = 0, the residuals of the two lstsq solves)"""
    t = SR._assemble(d, kinds)
    W = AR.stack(t, w)
    n, SL, SX, xo, uo, dad = t["n"], t["SL"], t["SX"], t["xo"], t["uo"], t["dad"]
    on = SR.pinned(d, x, u, kinds)
    fi = np.flatnonzero(on)
    F = np.zeros((len(fi), n))
    F[np.arange(len(fi)), fi] = 1.0
    m = SL + len(fi)
    Cm = np.vstack([t["E"], F])
    K = np.block([[t["H"], Cm.T], [Cm, np.zeros((m, m))]])
    z = np.concatenate([x, u])
    rhs = np.concatenate([-np.concatenate([d["q"], d["r"]]), -np.asarray(d["b"], dtype=np.float64), z[fi]])
    sol = np.linalg.lstsq(K, rhs, rcond=None)[0]
    a = np.linalg.lstsq(K.T, np.vstack([W, np.zeros((m, W.shape[1]))]), rcond=None)[0]
    resid = (float(np.max(np.abs(K @ sol - rhs))), float(np.max(np.abs(sol[:n] - z))))
    g = dict(gq=-a[:SX], gr=-a[SX:n], gb=-a[n:n + SL])
    nx0r = int(t["nx"][0])

    def entry(row, col, j):
        """-a' dK sol for the entry K[row, col] alone"""
        return -a[row, j] * sol[col]

    def node_H(k, j):
        ii = t["idx"][k]
        front = pad if k == 0 else 0
        nz = len(ii) + front
        G = np.zeros((nz, nz))
        for r, i in enumerate(ii):
            for c, jj in enumerate(ii):
                G[front + r, front + c] = entry(i, jj, j)
        gz = np.concatenate([np.zeros(front), g["gq"][xo[k]:xo[k + 1], j], g["gr"][uo[k]:uo[k + 1], j]])
        return (np.diag(G).copy() if t["kinds"][k] == 0 else 0.5 * (G + G.T)), gz

    def edge_AB(c, j):
        p = dad[c]
        front = pad if p == 0 else 0
        cols_x, cols_u = np.arange(xo[p], xo[p + 1]), SX + np.arange(uo[p], uo[p + 1])
        rows = np.arange(xo[c], xo[c + 1]) - nx0r
        gA, gB = np.zeros((len(rows), front + len(cols_x))), np.zeros((len(rows), len(cols_u)))
        for r, i in enumerate(rows):
            for cc, jj in enumerate(cols_x):          # the entry sits at E[i, jj] and at E'[jj, i]
                gA[r, front + cc] = entry(n + i, jj, j) + entry(jj, n + i, j)
            for cc, jj in enumerate(cols_u):
                gB[r, cc] = entry(n + i, jj, j) + entry(jj, n + i, j)
        return gA, gB, g["gb"][rows, j]

    return _group_sums(t, x, u, None, g, hgroup, cgroup, x0, param, pad, node_H, edge_AB), sol[n:n + SL], resid


def inner(G, dth):
    """<G, dtheta> over every output, column 0"""
    return float(sum(np.sum(a[..., 0] * b) for key in KEYS for a, b in zip(G[key], dth.get(key, [])) if b is not None))

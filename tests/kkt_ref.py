"""KKT residuals of a point of a tree QP in numpy, entry by entry: the reference of tqgpu_kkt_residual* (test_kkt_reference.py
holds it to the host's tree_qp_out_calculate_KKT_res, test_gpu_kkt.py holds the device to it).

The six classes and their formulas are those of tree_qp_out_calculate_KKT_res (qp_container.c, after tree_qp_common.c:540-788):

    0 STAT    Qx + q + S'u + mu_x + C'mu_d - lam_k + sum_kids A'lam_kid ; Ru + r + Sx + mu_u + D'mu_d + sum_kids B'lam_kid
    1 DYN     A x_dad + B u_dad + b - x_k
    2 BFEAS   v > max ? v - max : v < min ? min - v : 0                          on the entries of [x | u]
    3 BCOMPL  mu > 0 ? mu (v - max) : mu (min - v)
    4 GFEAS   the violation of dmin <= Cx + Du <= dmax
    5 GCOMPL  the same product with mu_d and Cx + Du

with the corner semantics of include/treeqp_amd.h: a multiplier that is exactly 0 contributes 0 to its complementarity entry
whatever the bound, a non-zero one against an infinite bound gives inf, a NaN value violates its bounds (NaN), a NaN anywhere
in a class makes the class NaN at the lowest such node, ties go to the lowest node, nodes of kind 1 ignore their bounds
(entries 0), rows count on nodes of kind 3 only, a clipping node (kind 0) has the diagonal of its H alone.

Beside every entry: T, the sum of the absolute values of its terms, and m, their count.  Any order of summing m terms, with or
without fma, differs from any other by at most 2 m eps T; the complementarity product adds two roundings: the bound of an entry
is 2 (m + 2) eps T, of a class maximum (and of a node's) the largest bound among its entries."""
from __future__ import annotations

import numpy as np

from treeqp_amd import problems as P

EPS = np.finfo(np.float64).eps
CLASSES = ("stat", "dyn", "bfeas", "bcompl", "gfeas", "gcompl")
STAT, DYN, BFEAS, BCOMPL, GFEAS, GCOMPL = range(6)


def _sum_terms(terms):
    """terms (entries x m) -> value, T, m per entry"""
    terms = np.asarray(terms, dtype=np.float64)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1), np.full(terms.shape[0], terms.shape[1])


def _viol(v, lo, hi, Tv):
    """(value, T): v - hi, lo - v, 0, or NaN for a NaN value; Tv: the sum of the absolute terms of v"""
    out, T = np.zeros_like(v), np.zeros_like(v)
    up, nan = v > hi, np.isnan(v)
    dn = (v < lo) & ~up
    with np.errstate(invalid="ignore"):
        out[up], T[up] = (v - hi)[up], (Tv + np.abs(hi))[up]
        out[dn], T[dn] = (lo - v)[dn], (Tv + np.abs(lo))[dn]
    out[nan], T[nan] = np.nan, np.nan
    return out, T


def _compl(mu, v, lo, hi, Tv):
    """(value, T): mu (v - hi) for mu > 0, mu (lo - v) otherwise, 0 for mu == 0; Tv: the sum of the absolute terms of v"""
    out, T = np.zeros_like(v), np.zeros_like(v)
    with np.errstate(invalid="ignore"):
        pos, neg = mu > 0, ~(mu > 0) & (mu != 0)
        out[pos], T[pos] = (mu * (v - hi))[pos], (np.abs(mu) * (Tv + np.abs(hi)))[pos]
        out[neg], T[neg] = (mu * (lo - v))[neg], (np.abs(mu) * (Tv + np.abs(lo)))[neg]
    return out, T


def node_blocks(d):
    """per node H_k = [Q S'; S R] from the flat column-major Q, R, S"""
    nx, nu = np.asarray(d["nx"], int), np.asarray(d["nu"], int)
    out, oq, orr, os_ = [], 0, 0, 0
    for k in range(len(nx)):
        a, m = int(nx[k]), int(nu[k])
        H = np.zeros((a + m, a + m))
        H[:a, :a] = np.reshape(d["Q"][oq:oq + a * a], (a, a), order="F"); oq += a * a
        H[a:, a:] = np.reshape(d["R"][orr:orr + m * m], (m, m), order="F"); orr += m * m
        S = np.reshape(d["S"][os_:os_ + m * a], (m, a), order="F"); os_ += m * a
        H[a:, :a], H[:a, a:] = S, S.T
        out.append(H)
    return out


def node_rows(d):
    """per node (G = [C | D], dmin, dmax), or None"""
    nx, nu = np.asarray(d["nx"], int), np.asarray(d["nu"], int)
    nc = np.asarray(d.get("nc", np.zeros(len(nx), int)), int)
    out, oc, od, orow = [], 0, 0, 0
    for k in range(len(nx)):
        m = int(nc[k])
        if m == 0:
            out.append(None)
            continue
        Ck = np.reshape(d["C"][oc:oc + m * nx[k]], (m, nx[k]), order="F"); oc += m * nx[k]
        Dk = np.reshape(d["D"][od:od + m * nu[k]], (m, nu[k]), order="F"); od += m * nu[k]
        out.append((np.hstack([Ck, Dk]), np.asarray(d["dmin"][orow:orow + m], float), np.asarray(d["dmax"][orow:orow + m], float)))
        orow += m
    return out


def residuals(d, sol, kinds=None):
    """d: nk, nx, nu, A, B, b, Q, R, S (column major, node after node), q, r, the bounds and optionally nc, C, D, dmin, dmax;
    sol: x, u, lam and optionally mu_x, mu_u, mu_d (missing or None: zeros), flat; kinds: per node 0 / 1 / 2 / 3 (None: 3 where
    the node has rows, 2 elsewhere -- every bound and every row counts, as on the host).

    Returns dict(entries, res, node, max, per_node, bound, node_bound): entries[c][k] = (values, T, m) of class c on node k (arrays,
    in the host's order: x then u, or the rows); res[6], node[6]; per_node (Nn, 6); bound[6] and node_bound (Nn, 6) as in the
    module docstring."""
    nk, nx, nu = (np.asarray(d[k], int) for k in ("nk", "nx", "nu"))
    Nn = len(nk)
    nc = np.asarray(d.get("nc", np.zeros(Nn, int)), int)
    kinds = np.where(nc > 0, 3, 2) if kinds is None else np.asarray(kinds, int)
    dad = P.parents_of(nk)
    kids = [[c for c in range(1, Nn) if dad[c] == k] for k in range(Nn)]
    xo, uo, ro = (np.concatenate([[0], np.cumsum(v)]) for v in (nx, nu, nc))
    lo_ = xo - nx[0]
    H, rows = node_blocks(d), node_rows(d)
    get = lambda name, n: np.zeros(n) if sol.get(name) is None else np.asarray(sol[name], float)
    x, u, lam = (np.asarray(sol[k], float) for k in ("x", "u", "lam"))
    mu_x, mu_u, mu_d = get("mu_x", xo[-1]), get("mu_u", uo[-1]), get("mu_d", ro[-1])
    A, B, ao, bo = {}, {}, 0, 0
    for k in range(1, Nn):
        p = dad[k]
        A[k] = np.reshape(d["A"][ao:ao + nx[k] * nx[p]], (nx[k], nx[p]), order="F"); ao += nx[k] * nx[p]
        B[k] = np.reshape(d["B"][bo:bo + nx[k] * nu[p]], (nx[k], nu[p]), order="F"); bo += nx[k] * nu[p]
    zof = lambda k: np.concatenate([x[xo[k]:xo[k + 1]], u[uo[k]:uo[k + 1]]])
    none = (np.zeros(0), np.zeros(0), np.zeros(0, int))
    entries = [[none] * Nn for _ in CLASSES]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(Nn):
            a, nz = int(nx[k]), int(nx[k] + nu[k])
            z = zof(k)
            mu = np.concatenate([mu_x[xo[k]:xo[k + 1]], mu_u[uo[k]:uo[k + 1]]])
            lamk = lambda c: lam[lo_[c]:lo_[c] + nx[c]]
            # stationarity
            cols = [H[k] * z[None, :] if kinds[k] else (np.diag(H[k]) * z)[:, None]]
            cols.append(np.concatenate([d["q"][xo[k]:xo[k + 1]], d["r"][uo[k]:uo[k + 1]]])[:, None])
            cols.append(mu[:, None])
            if kinds[k] == 3 and rows[k] is not None:
                cols.append(rows[k][0].T * mu_d[ro[k]:ro[k + 1]][None, :])
            for c in kids[k]:
                cols.append(np.hstack([A[c], B[c]]).T * lamk(c)[None, :])
            val, T, m = _sum_terms(np.hstack(cols)) if nz else none
            if k > 0 and nz:
                own = np.concatenate([lamk(k), np.zeros(nz - a)])
                val, T, m = val - own, T + np.abs(own), m + (np.arange(nz) < a)
            entries[STAT][k] = (val, T, m)
            # dynamics
            if k > 0 and a:
                p = dad[k]
                terms = np.hstack([A[k] * x[xo[p]:xo[p + 1]][None, :], B[k] * u[uo[p]:uo[p + 1]][None, :],
                                   d["b"][lo_[k]:lo_[k] + a][:, None], -x[xo[k]:xo[k + 1]][:, None]])
                entries[DYN][k] = _sum_terms(terms)
            # bounds
            if nz:
                lo = np.concatenate([d["xmin"][xo[k]:xo[k + 1]], d["umin"][uo[k]:uo[k + 1]]]).astype(float)
                hi = np.concatenate([d["xmax"][xo[k]:xo[k + 1]], d["umax"][uo[k]:uo[k + 1]]]).astype(float)
                if kinds[k] == 1:
                    entries[BFEAS][k] = entries[BCOMPL][k] = (np.zeros(nz), np.zeros(nz), np.zeros(nz, int))
                else:
                    v, T = _viol(z, lo, hi, np.abs(z))
                    entries[BFEAS][k] = (v, T, np.full(nz, 2))
                    v, T = _compl(mu, z, lo, hi, np.abs(z))
                    entries[BCOMPL][k] = (v, T, np.full(nz, 2))
            # rows
            if kinds[k] == 3 and rows[k] is not None:
                G, dlo, dhi = rows[k]
                g, Tg, mg = _sum_terms(G * z[None, :])
                v, T = _viol(g, dlo, dhi, Tg)
                entries[GFEAS][k] = (v, T, mg + 1)
                v, T = _compl(mu_d[ro[k]:ro[k + 1]], g, dlo, dhi, Tg)
                entries[GCOMPL][k] = (v, T, mg + 1)
    per_node, node_bound, has = np.zeros((Nn, 6)), np.zeros((Nn, 6)), np.zeros((Nn, 6), bool)
    for c in range(6):
        for k in range(Nn):
            v, T, m = entries[c][k]
            if len(v):
                has[k, c] = True
                av = np.abs(v)
                per_node[k, c] = np.nan if np.isnan(av).any() else av.max()
                with np.errstate(invalid="ignore"):
                    b = 2.0 * (m + 2) * EPS * T
                node_bound[k, c] = np.nan if np.isnan(b).any() else b.max()
    res, node, bound = np.zeros(6), np.full(6, -1, np.int32), np.zeros(6)
    for c in range(6):
        ks = np.flatnonzero(has[:, c])
        if not len(ks):
            continue
        col = per_node[ks, c]
        node[c] = ks[np.flatnonzero(np.isnan(col))[0]] if np.isnan(col).any() else ks[int(np.argmax(col))]      # (argmax: the first of equals)
        res[c] = per_node[node[c], c]
        bound[c] = np.nan if np.isnan(node_bound[ks, c]).any() else node_bound[ks, c].max()
    return dict(entries=entries, res=res, node=node, max=float("nan") if np.isnan(res).any() else float(res.max()),
                per_node=per_node, bound=bound, node_bound=node_bound, has=has)


def node_is_clear(ref):
    """per class: the largest and the second-largest node maximum differ by more than twice the class bound (a class on fewer than
    two nodes is clear), so that the node the device names cannot depend on the order of its sums"""
    out = np.ones(6, bool)
    for c in range(6):
        col = np.sort(ref["per_node"][ref["has"][:, c], c])[::-1]
        if len(col) >= 2:
            out[c] = bool(col[0] - col[1] > 2.0 * ref["bound"][c])
    return out


def host_order(ref):
    """the entries of every class in the order of tree_qp_out_calculate_KKT_res's output: per node stat | dyn | bfeas | bcompl |
    gfeas | gcompl -> (values, bounds)"""
    vals, bnds = [], []
    Nn = len(ref["entries"][0])
    for k in range(Nn):
        for c in range(6):
            v, T, m = ref["entries"][c][k]
            vals.append(v); bnds.append(2.0 * (m + 2) * EPS * T)
    return np.concatenate(vals), np.concatenate(bnds)


# ---------------------------------------------------------------------------------------------------------------------------
# problems and points
# ---------------------------------------------------------------------------------------------------------------------------

def random_problem(shape_or_dims, kinds, seed, nc=None, finite_bounds=True):
    """a tree QP with random data: dense H_k (diagonal on the nodes of kind 0), finite bounds around zero (every entry can be
    violated by a standard normal point), nc[k] standard normal rows with finite ranges; shape_or_dims: a nested shape of
    limit_shapes or (nk, nx, nu)"""
    from helpers import dense_shaped_qp
    from limit_shapes import flatten
    nk, nx, nu = flatten(shape_or_dims) if len(shape_or_dims) == 3 and isinstance(shape_or_dims[2], list) else shape_or_dims
    d = dense_shaped_qp(nk, nx, nu, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 4242))
    kinds = np.asarray(kinds, int)
    H = node_blocks(d)
    Q, R, S = [], [], []
    for k, Hk in enumerate(H):
        a = int(d["nx"][k])
        if kinds[k] == 0:
            Hk = np.diag(np.diag(Hk))
        Q.append(Hk[:a, :a].ravel(order="F")); R.append(Hk[a:, a:].ravel(order="F")); S.append(Hk[a:, :a].ravel(order="F"))
    d["Q"], d["R"], d["S"] = np.concatenate(Q), np.concatenate(R), np.concatenate(S)
    xo, uo = np.concatenate([[0], np.cumsum(d["nx"])]), np.concatenate([[0], np.cumsum(d["nu"])])
    d["Qd"] = np.concatenate([np.diag(Hk)[:int(d["nx"][k])] for k, Hk in enumerate(node_blocks(d))] or [np.zeros(0)])
    d["Rd"] = np.concatenate([np.diag(Hk)[int(d["nx"][k]):] for k, Hk in enumerate(node_blocks(d))] or [np.zeros(0)])
    if finite_bounds:
        sx, su = int(xo[-1]), int(uo[-1])
        d["xmin"], d["xmax"] = -0.2 - rng.random(sx), 0.2 + rng.random(sx)
        d["umin"], d["umax"] = -0.2 - rng.random(su), 0.2 + rng.random(su)
    if nc is not None:
        nc = np.asarray(nc, np.int32)
        d["nc"] = nc
        d["C"] = np.concatenate([rng.standard_normal(int(nc[k] * d["nx"][k])) for k in range(len(nc))] or [np.zeros(0)])
        d["D"] = np.concatenate([rng.standard_normal(int(nc[k] * d["nu"][k])) for k in range(len(nc))] or [np.zeros(0)])
        tot = int(nc.sum())
        d["dmin"], d["dmax"] = -0.3 - rng.random(tot), 0.3 + rng.random(tot)
    return d


def random_point(d, seed, scale=1.0):
    """standard normal x, u, lam and multipliers (none of them zero): not a solution, so that every class is non-zero"""
    rng = np.random.Generator(np.random.PCG64(seed + 99))
    nx, nu = np.asarray(d["nx"], int), np.asarray(d["nu"], int)
    sx, su, sl = int(nx.sum()), int(nu.sum()), int(nx[1:].sum())
    sol = dict(x=scale * rng.standard_normal(sx), u=scale * rng.standard_normal(su), lam=scale * rng.standard_normal(sl),
               mu_x=scale * rng.standard_normal(sx), mu_u=scale * rng.standard_normal(su))
    if "nc" in d:
        sol["mu_d"] = scale * rng.standard_normal(int(np.sum(d["nc"])))
    return sol

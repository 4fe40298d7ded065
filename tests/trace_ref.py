"""What a solve reports beside its solution -- the termination norm (tqgpu_result.last_error_norm, the oracle's trace_err) and the
dual function value (last_fval, trace_fval) -- in numpy, with derived float64 bounds.  No device and no oracle behind it and no
code shared with either: the residual and the node terms come from newton_ref (longdouble).

Norms (termination_t of the reference, dual_Newton_tree.c:412-442): with r the dynamics residual A_k x_p + B_k u_p + b_k - x_k
over all edges,
    0 TREEQP_SUMSQUAREDERRORS   sum r_i^2
    1 TREEQP_TWONORM            sqrt(sum r_i^2)
    2 TREEQP_INFNORM            max |r_i|          (NaN-keeping: one NaN entry makes it NaN)

Bounds.  eps = 2^-52 = 2 u.  A float64 sum of m products, in any order, with or without fma, differs from the exact one by at
most gamma_m T <= m eps T (m u < 1/2), T the sum of the absolute values of the products (kkt_ref.py takes twice that between
two float64 evaluations; here the other side is longdouble, whose own error is 2^-11 of that).  An entry r_i has
m_i = nx_p + nu_p + 2 terms (the products of the row of [A_k B_k], b_k, x_k) with T_i = |A_k||x_p| + |B_k||u_p| + |b_k| + |x_k|:
|dr_i| <= m_i eps T_i.  From there, n the number of entries:
    2  max |r_i|: no further rounding.                       |d| <= m eps T,  T = max T_i
    1  | ||r + dr|| - ||r|| | <= ||dr|| <= m eps sqrt(sum T_i^2); the n squares are summed (n + 1 roundings with the products,
       relative, all terms positive: half of it after the root) and the root is rounded once.
                                                             |d| <= (m + n + 2) eps T,  T = sqrt(sum T_i^2)  (>= ||r||)
    0  d(r_i^2) <= (2 |r_i| + |dr_i|) |dr_i|, and the sum of the squares as above.
                                                             |d| <= (m + n + 2) eps T,  T = sum (2 |r_i| + m_i eps T_i) T_i  (>= sum r_i^2)
The chain of dependent additions is therefore the terms of an entry, then the entries of a block, then the blocks, then the
root: bound_err = c eps T with c = m + 2 (+ n for the two sums), m the largest m_i.  Nothing in c or T is fitted to a device.

At a dual point (error_norm_at) x and u are themselves computed: z = P h on the free entries with h a float64 sum of
m_h = 2 + (the children's nx) terms, T_h its absolute sum, and a solve with H (a division on a clipping node; a Cholesky solve of
order nz on a dense one, backward stable with |dH| <= (3 nz + 1) eps |H|-sized perturbations [Higham, Accuracy and Stability,
Thm 10.4], so |dz| <= (m_h + 3 nz + 1) eps |P| (T_h + |H||z|)).  Entries on a bound are exact.  T_i then has
|z| + |P| (T_h + |H||z|) in the place of |z|, and c grows by the longest such chain, m_h + 3 nz + 1 (nz = 1 for a division).
The active set is that of the longdouble reference: res is continuous and piecewise linear in lambda, so an entry that
float64 puts on the other side of a clipping threshold moves res by no more than its rounding.

A caller that needs the norm at the point an iteration started from takes that point exactly (the lam returned with one iteration
fewer, test_gpu_result_fields.py); error_norm_at also returns ||M||_2, the Lipschitz constant of res in lambda (M = G P G', the
negated dual Hessian, is its Jacobian on every piece), for callers that know a point only to rounding.

The dual value: a node's term -1/2 z'H z + h'z - sum_children b_k'lambda_k is a sum of at most nz + nz + (children's nx) products
behind h's own m_h terms, T_p = 1/2 |z|'|H||z| + T_h'|z| + sum |b_k|'|lambda_k| (newton_ref.terms_of_stages); the node terms are
summed (Nn terms).  The rounding of z itself enters at second order only: the term's gradient in z, h - H z, vanishes on the
free entries, and the fixed ones are exact; on a node with general constraints h - H z = G'mu_d, and the rows of the working
set hold to (nz + 1) eps |G||z|: T_p gains |mu_d|'|G||z| there.  bound_fval = c eps T_f, c = (2 nz + children's nx + m_h + 3)
at its largest node + Nn, T_f = sum T_p."""
from __future__ import annotations

import numpy as np

import newton_ref as N
from treeqp_amd import problems as P

LD = N.LD
EPS = float(np.finfo(np.float64).eps)


def _edges(d):
    nk, nx, nu = (np.asarray(d[k], int) for k in ("nk", "nx", "nu"))
    dad = P.parents_of(nk)
    xo, uo = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nu)])
    ao = bo = lo = 0
    for k in range(1, len(nk)):
        p = dad[k]
        A = np.asarray(d["A"][ao:ao + nx[k] * nx[p]], LD).reshape((nx[k], nx[p]), order="F"); ao += nx[k] * nx[p]
        B = np.asarray(d["B"][bo:bo + nx[k] * nu[p]], LD).reshape((nx[k], nu[p]), order="F"); bo += nx[k] * nu[p]
        b = np.asarray(d["b"][lo:lo + nx[k]], LD); lo += nx[k]
        yield k, p, A, B, b, slice(xo[k], xo[k + 1]), slice(xo[p], xo[p + 1]), slice(uo[p], uo[p + 1])


def _norm(r, T, m, term):
    """(value, T_err) of the norm `term` from the entries r, their absolute sums T and term counts m (all longdouble / int)"""
    if term not in (0, 1, 2):
        raise ValueError(f"termCondition {term}")
    if len(r) == 0:
        return LD(0), LD(0)
    with np.errstate(invalid="ignore", over="ignore"):
        if term == 2:
            return (LD(np.nan) if np.isnan(r).any() else np.abs(r).max()), T.max()
        if term == 1:
            return np.sqrt((r * r).sum()), np.sqrt((T * T).sum())
        return (r * r).sum(), ((2 * np.abs(r) + m * LD(EPS) * T) * T).sum()


def error_norm(d, x, u, term):
    """The norm `term` (0, 1, 2) of the dynamics residual of the given x, u (flat, node after node) -> (value, T_err), longdouble;
    T_err as the module docstring defines it for that norm."""
    x, u = np.asarray(x, LD), np.asarray(u, LD)
    r, T, m = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for k, p, A, B, b, sk, sp, su in _edges(d):
            r.append(A @ x[sp] + B @ u[su] + b - x[sk])
            T.append(np.abs(A) @ np.abs(x[sp]) + np.abs(B) @ np.abs(u[su]) + np.abs(b) + np.abs(x[sk]))
            m.append(np.full(len(b), A.shape[1] + B.shape[1] + 2))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, LD)
    return _norm(cat(r), cat(T), cat(m), term)


def _z_scale(st, lam):
    """per node |z| + |P| (T_h + |H||z|): what an entry of z is uncertain by, in units of its chain's eps"""
    out = []
    for p in range(len(st["z"])):
        Th = N.abs_h(st, lam, p)
        z, Hp, Pp = np.abs(st["z"][p]), np.abs(st["H"][p].astype(LD)), np.abs(st["P"][p])
        Hz = Hp * z if Hp.ndim == 1 else Hp @ z
        out.append(z + Pp @ (Th + Hz))
    return out


def residual_at(d, lam, kinds=None, dense=False, stages=None):
    """The entries behind error_norm_at, whatever the norm: (r, T, m, normM)"""
    st = N.stage_solutions(d, lam, dense, kinds) if stages is None else stages
    M, res = N.assemble_from(st)
    normM = float(np.linalg.norm(M.astype(np.float64), 2)) if len(res) else 0.0
    nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, kd = st["tree"]
    Tz = _z_scale(st, lam)
    r, T, m = [], [], []
    for k in range(1, len(nk)):
        p = dad[k]
        C = np.hstack([A[k], B[k]])
        r.append(C @ st["z"][p] + b[k] - st["z"][k][:nx[k]])
        T.append(np.abs(C) @ Tz[p] + np.abs(b[k]) + Tz[k][:nx[k]])
        m.append(np.full(nx[k], C.shape[1] + 2))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, LD)
    return cat(r), cat(T), cat(m), normM


def norm_of(entries, term):
    """(value, T_err, normM) of norm `term` from residual_at's entries"""
    r, T, m, normM = entries
    return _norm(r, T, m, term) + (normM,)


def error_norm_at(d, lam, term, kinds=None, dense=False, stages=None):
    """The same at the dual point lam, from newton_ref.assemble's res -> (value, T_err, normM): normM the spectral norm of M, the
    Lipschitz constant of res in lam.  stages: stage solutions to use instead of newton_ref's (gen_ref's, for nodes with general
    constraints)."""
    return norm_of(residual_at(d, lam, kinds, dense, stages), term)


def _counts(d):
    nk, nx, nu = (np.asarray(d[k], int) for k in ("nk", "nx", "nu"))
    dad = P.parents_of(nk)
    kid_nx = np.zeros(len(nk), int)
    for k in range(1, len(nk)):
        kid_nx[dad[k]] += nx[k]
    m = max([nx[dad[k]] + nu[dad[k]] + 2 for k in range(1, len(nk))], default=2)
    return nk, nx, nu, kid_nx, int(m), int(nx[1:].sum())


def _stage_chain(d, kinds, dense):
    """the longest chain behind an entry of z: m_h + 3 nz + 1 on a dense node, m_h + 2 on a clipping one"""
    nk, nx, nu, kid_nx, _, _ = _counts(d)
    kd, _ = N._kinds_of(d, dense, None if kinds is None else np.minimum(np.asarray(kinds, int), 2))
    return int(max((2 + kid_nx[p]) + (2 if kd[p] == 0 else 3 * (nx[p] + nu[p]) + 1) for p in range(len(nk))))


def bound_err(d, term, T_err, at=False, kinds=None, dense=False):
    """c eps T_err of the module docstring.  at: the value was taken at a dual point (error_norm_at): c gains the chain of the stage
    solve."""
    _, _, _, _, m, n = _counts(d)
    c = m + 2 + (n if term < 2 else 0) + (_stage_chain(d, kinds, dense) if at else 0)
    return c * EPS * float(T_err)


def dual_value_with_scale(d, lam, kinds=None, dense=False, stages=None):
    """newton_ref.dual_terms(...).sum() and T_f, the sum of the absolute values of every product inside every node term
    (longdouble).  stages: as error_norm_at; the multipliers of the rows (stages["mu_d"]) then enter T_f as the docstring says."""
    st = N.stage_solutions(d, lam, dense, kinds) if stages is None else stages
    t, s = N.terms_of_stages(st, lam)
    Tf = s.sum()
    if stages is not None and "mu_d" in st:
        import gen_ref
        for k, c in enumerate(gen_ref.cons_of(d)):
            if c is not None and len(st["mu_d"][k]):
                Tf = Tf + np.abs(st["mu_d"][k]) @ (np.abs(np.asarray(c[0], LD)) @ np.abs(st["z"][k]))
    return t.sum(), Tf


def bound_fval(d, T_f):
    """c eps T_f of the module docstring"""
    nk, nx, nu, kid_nx, _, _ = _counts(d)
    c = int(max(2 * (nx[p] + nu[p]) + kid_nx[p] + (2 + kid_nx[p]) + 3 for p in range(len(nk)))) + len(nk)
    return c * EPS * float(T_f)

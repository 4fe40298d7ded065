"""One dual Newton step with the solver's block-wise regularisation (treeqp_dpotrf_l_with_reg_opts), in numpy longdouble, on
the dense system of newton_ref.py.  No code is shared with the oracle or the device path.

What the solver does with the Newton system M dlam = res (dual_Newton_tree.c, factorize_Newton_matrix and
calculate_delta_lambda):
- Block p holds the duals of the children of p, in child order.  The blocks are eliminated from the last parent to the root;
  block p has received -U S^-1 U' from each block c of its children that are parents themselves (S the matrix block c
  factorised, regularisation included; U the coupling of the duals of block c with lambda_c) before it is factorised.
- The factorisation is a Cholesky factorisation in which a pivot <= 0 gives a zero column and the reciprocal 0 (so that entry of
  the step is 0, and the entry takes no part in anything after it).
- regType 0 factorises the block as it is; 1 (ALWAYS) adds regValue to the block's diagonal first; 2 (ON_THE_FLY) factorises,
  and if any L_jj <= regTol adds regValue to the WHOLE block's diagonal and factorises again -- once, with no second check.

block_newton_step does just that (the substitution refined once with the same factors) and checks its step against one dense
solve of M + diag(shifts)."""
from __future__ import annotations

import numpy as np

import newton_ref as N

LD = np.longdouble
XCHECK_TOL = 1e-13


def potrf(S):
    """Left-looking Cholesky of S (in its own precision) -> (L, inv): a pivot <= 0 leaves a zero column and inv[j] = 0."""
    n = len(S)
    L = np.zeros((n, n), dtype=S.dtype)
    inv = np.zeros(n, dtype=S.dtype)
    for j in range(n):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if col[0] > 0:
            ljj = np.sqrt(col[0])
            inv[j] = 1 / ljj
            L[j, j] = ljj
            L[j + 1:, j] = col[1:] * inv[j]
    return L, inv


def _right_solve(U, L, inv):
    """Y = U L^-T with the reciprocals `inv` (a zero column of L gives a zero column of Y)"""
    Y = np.zeros_like(U)
    for j in range(L.shape[0]):
        Y[:, j] = (U[:, j] - Y[:, :j] @ L[j, :j]) * inv[j]
    return Y


def _forward(L, inv, r):
    y = np.zeros_like(r)
    for j in range(len(r)):
        y[j] = (r[j] - L[j, :j] @ y[:j]) * inv[j]
    return y


def _backward(L, inv, y):
    x = np.zeros_like(y)
    for j in range(len(y) - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) * inv[j]
    return x


def block_newton_step(d, lam0, regType, regTol, regValue, dense=False, kinds=None, dtype=LD, check=True, inclusive=True):
    """The regularised step at lam0.  Returns dict(dlam, res, flagged, pivots, guard, cond, margin, stages, xcheck, shift, zero):
    - flagged: the blocks (parent ids, in the order they are factorised) whose diagonal was shifted;
    - pivots: per block, dict(first=the L_jj of the first pass up to and including the first one <= regTol (all of them when none
      is), final=those of the factorisation that is used);
    - guard: the smallest, over every L_jj of a first pass, of max(L_jj / regTol, regTol / L_jj); an exact 0 counts as infinity
      (it is <= regTol and <= 0 in every implementation).  regType 0 and 1 do not compare with regTol: there the nonzero L_jj are
      counted one-sidedly, L_jj / regTol (a pivot that rounding could push across 0 is as bad as one next to the threshold);
    - cond: the condition number of the matrix finally solved, M + diag(shift) without the zero-column entries;
    - xcheck: the difference, relative to the largest entry, of the block substitution and the dense solve (asserted <= 1e-13 unless check is False: a caller
      that searches for a usable lambda0 looks at it itself);
    - shift, zero: per dual entry, what was added to its diagonal and whether its column is a zero column.
    dtype = np.float64 runs elimination and substitution in float64 (what a float64 implementation computes, for measuring the
    sensitivity of a row; the cross-check is then not asserted).  inclusive: the clipping rule, see newton_ref.stage_solutions."""
    M, res, st = N.assemble(d, lam0, dense, kinds, inclusive)
    M, res = M.astype(dtype), res.astype(dtype)
    nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, _ = st["tree"]
    n = len(res)
    parents = [p for p in range(len(nk)) if nk[p] > 0]
    idx = {p: np.concatenate([np.arange(lo_[k], lo_[k] + nx[k]) for k in kids[p]]) for p in parents}
    own = {p: np.arange(lo_[p], lo_[p] + nx[p]) for p in parents if p > 0}
    W = M.copy()
    shift = np.zeros(n, dtype=dtype)
    zero = np.zeros(n, dtype=bool)
    fact, flagged, pivots, guard = {}, [], {}, np.inf
    tol, val = dtype(regTol), dtype(regValue)
    for p in reversed(parents):
        I = idx[p]
        S = W[np.ix_(I, I)].copy()
        if regType == 1:
            S[np.diag_indices_from(S)] += val
            shift[I] += val
            flagged.append(p)
        L, inv = potrf(S)
        first = np.diag(L).copy()
        for v in first:
            if v != 0:
                guard = min(guard, float(max(v / tol, tol / v) if regType == 2 else v / tol))
        small = np.flatnonzero(first <= tol)
        if regType == 2 and len(small):
            first = first[:small[0] + 1]
            S[np.diag_indices_from(S)] += val
            shift[I] += val
            flagged.append(p)
            L, inv = potrf(S)
        pivots[p] = dict(first=first.astype(np.float64), final=np.diag(L).astype(np.float64))
        zero[I] = inv == 0
        Y = None
        if p > 0:
            Y = _right_solve(M[np.ix_(own[p], I)], L, inv)
            W[np.ix_(own[p], own[p])] -= Y @ Y.T
        fact[p] = (L, inv, Y)
    def substitute(rhs):
        """forward from the last parent to the root, backward from the root down"""
        r = rhs.copy()
        ys = {}
        for p in reversed(parents):
            L, inv, Y = fact[p]
            ys[p] = _forward(L, inv, r[idx[p]])
            if p > 0:
                r[own[p]] -= Y @ ys[p]
        x = np.zeros(n, dtype=dtype)
        for p in parents:
            L, inv, Y = fact[p]
            x[idx[p]] = _backward(L, inv, ys[p] - Y.T @ x[own[p]] if p > 0 else ys[p])
        return x

    Mfull = M + np.diag(shift)
    dl = substitute(res)
    if dtype is LD:
        # one refinement with the same factors: a longdouble elimination alone keeps cond(M) * 1e-19, 1e-13 on the worst rows
        dl = dl + substitute(np.where(zero, 0, res - Mfull @ dl))
    # the same step from one dense solve: M + diag(shift) without the zero-column entries, float64 refined once in longdouble
    keep = ~zero
    Mf = Mfull[np.ix_(keep, keep)]
    M64 = Mf.astype(np.float64)
    dd = np.zeros(n, dtype=LD)
    if np.any(keep):
        x = np.linalg.solve(M64, res[keep].astype(np.float64)).astype(LD)
        x = x + np.linalg.solve(M64, (res[keep] - Mf @ x).astype(np.float64)).astype(LD)
        dd[keep] = x.astype(LD)
        ev = np.linalg.eigvalsh(M64)
        cond = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    else:
        cond = 1.0
    xcheck = float(np.max(np.abs(dd - dl)) / max(LD(1e-300), np.max(np.abs(dd)))) if n else 0.0
    assert not check or dtype is not LD or xcheck <= XCHECK_TOL, f"block substitution and dense solve differ by {xcheck:.2e} of the largest entry"
    return dict(dlam=dl.astype(np.float64), res=res.astype(np.float64), flagged=flagged, pivots=pivots, guard=guard, cond=cond,
                margin=st["margin"], stages=st, xcheck=xcheck, shift=shift.astype(np.float64), zero=zero)


def armijo(d, lam0, ref, opts, kinds=None, dense=False):
    """(trials, slack) of newton_ref.armijo_trials along the step `ref` of block_newton_step"""
    return N.armijo_trials(d, lam0, ref["dlam"], ref["res"], opts, kinds, dense)

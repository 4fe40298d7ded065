"""The adjoint of a tree QP's solution at a point (x, u) with the active set frozen there, two ways in numpy: for w = dL/dz of a scalar
loss L of z = [x | u], the gradients gq = dL/dq, gr = dL/dr, gb = dL/db and gx0 = dL/dx0.
(a) dense_kkt: the transposed KKT system of sens_ref.dense_kkt (pinned rows included) with the right-hand side [w; 0; 0], by lstsq; the
    gradients are read off its solution, gx0 through the chain rule of the parameter form;
(b) dual_form: R_c = (P_c w_c)^x - C_c P_p w_p, M Y = R, gb = Y, [gq; gr] = -P (w - [Y; 0] + sum_c C_c' Y_c) as include/treeqp_amd.h
    states them, block by block (leaf to root, root, root to leaves) with the regularisation rule of reg_ref.py; it also returns what that
    rule did (sens_ref.RegRecord) and in_range, the residual of the matrix actually solved;
(c) dense_shifted: that same shifted system by one dense solve, given shift and zero.
(a) and (b) take the arguments of sens_ref (the flat problem d, the point, the parameter form, kinds) and w = (wx, wu), each (rows,) or (rows, nw)
in the flat layout of tqgpu_get_solution, and return dict(gq, gr, gb, gx0, ...) with nw columns."""
from __future__ import annotations

import numpy as np

import reg_ref as RR
import sens_ref as SR


def stack(t, w):
    """[wx; wu] as (n, nw)"""
    parts = [None if a is None else np.asarray(a, dtype=np.float64).reshape((rows, -1), order="F") for a, rows in zip(w, (t["SX"], t["SU"]))]
    nw = next((a.shape[1] for a in parts if a is not None), 1)
    return np.vstack([np.zeros((rows, nw)) if a is None else a for a, rows in zip(parts, (t["SX"], t["SU"]))])


def _gx0(t, param, db, dg, nx0, gz, gb, direct):
    """dL/dx0 from dL/d(linear terms), dL/db and the direct part"""
    if param["form"] == "states":
        return direct
    return db.T @ gb + dg.T @ gz


def dense_kkt(d, x, u, param, w, kinds=None):
    """(a): a = lstsq([H E' F'; E 0 0; F 0 0]', [w; 0; 0]); the system's right-hand side is [-g; -b; fix], so dL/dg = -a_z, dL/db = -a_lam,
    dL/dfix = a_mu; x0 enters b and g (eliminated root) or the fixed values of the root's states (root with states)"""
    t = SR._assemble(d, kinds)
    db, dg, nx0 = SR._param_terms(t, param)
    W = stack(t, w)
    on = SR.pinned(d, x, u, kinds)
    fi = np.flatnonzero(on)
    F = np.zeros((len(fi), t["n"]))
    F[np.arange(len(fi)), fi] = 1.0
    m = t["SL"] + len(fi)
    Cm = np.vstack([t["E"], F])
    Kmat = np.block([[t["H"], Cm.T], [Cm, np.zeros((m, m))]])
    rhs = np.vstack([W, np.zeros((m, W.shape[1]))])
    a = np.linalg.lstsq(Kmat.T, rhs, rcond=None)[0]
    resid = float(np.max(np.abs(Kmat.T @ a - rhs))) if rhs.size else 0.0
    n, SL, SX = t["n"], t["SL"], t["SX"]
    gz, gb, gfix = -a[:n], -a[n:n + SL], a[n + SL:]
    direct = None
    if param["form"] == "states":
        assert all(on[:nx0]), "the root's states are not on their bounds"
        direct = np.vstack([gfix[list(fi).index(i)] for i in range(nx0)])
    return dict(gq=gz[:SX], gr=gz[SX:], gb=gb, gx0=_gx0(t, param, db, dg, nx0, gz, gb, direct), residual=resid,
                scale=max(1.0, float(np.max(np.abs(a))) if a.size else 1.0))


def dual_form(d, x, u, param, w, kinds=None, regType=2, regTol=1e-6, regValue=1e-6):
    """(b): the formulas of the header, block by block"""
    t = SR._assemble(d, kinds)
    db, dg, nx0 = SR._param_terms(t, param)
    W = stack(t, w)
    nk, nx, xo, dad, n, SL, E, SX = t["nk"], t["nx"], t["xo"], t["dad"], t["n"], t["SL"], t["E"], t["SX"]
    on = SR.pinned(d, x, u, kinds)
    Pm = np.zeros((n, n))
    for k in range(t["Nn"]):
        ii = t["idx"][k]
        Hk = t["H"][np.ix_(ii, ii)]
        if t["kinds"][k] == 0:
            Pm[ii, ii] = np.where(on[ii], 0.0, 1.0 / np.diag(Hk))
        elif len(ii):
            Pm[np.ix_(ii, ii)] = np.linalg.inv(Hk)
    M = E @ Pm @ E.T
    R = -E @ (Pm @ W)          # rows of child c of p: (P_c w_c)^x - C_c P_p w_p
    Np = int(np.count_nonzero(nk > 0))
    kid0 = np.concatenate([[1], 1 + np.cumsum(nk)[:-1]])
    rng_of = lambda p: np.arange(xo[kid0[p]], xo[kid0[p] + nk[p]]) - nx[0]
    own = lambda p: np.arange(xo[p], xo[p + 1]) - nx[0]
    Wb = {p: M[np.ix_(rng_of(p), rng_of(p))].copy() for p in range(Np)}
    fac, n_reg = {}, 0
    rec = SR.RegRecord(SL)
    for p in range(Np - 1, -1, -1):
        Wp = Wb[p] + (regValue * np.eye(len(Wb[p])) if regType == 1 else 0.0)
        L, inv = RR.potrf(Wp)
        rec.first_pass(p, rng_of(p), np.diag(L), regType, regTol, regValue)
        if regType == 2 and np.any(np.diag(L) <= regTol):
            n_reg += 1
            L, inv = RR.potrf(Wp + regValue * np.eye(len(Wp)))
        rec.final(rng_of(p), inv)
        CUt = None
        if p > 0:
            CUt = RR._right_solve(M[np.ix_(own(p), rng_of(p))], L, inv)
            pos = own(p) - rng_of(dad[p])[0]
            Wb[dad[p]][np.ix_(pos, pos)] -= CUt @ CUt.T
        fac[p] = (L, inv, CUt)
    Y = np.zeros((SL, W.shape[1]))
    for j in range(W.shape[1]):
        r, tt = R[:, j].copy(), {}
        for p in range(Np - 1, 0, -1):          # leaf to root
            L, inv, CUt = fac[p]
            tt[p] = RR._forward(L, inv, r[rng_of(p)])
            r[own(p)] -= CUt @ tt[p]
        L, inv, _ = fac[0]
        Y[rng_of(0), j] = RR._backward(L, inv, RR._forward(L, inv, r[rng_of(0)]))
        for p in range(1, Np):                  # root to leaves
            L, inv, CUt = fac[p]
            Y[rng_of(p), j] = RR._backward(L, inv, tt[p] - CUt.T @ Y[own(p), j])
    gz = -Pm @ (W + E.T @ Y)
    direct = W[:nx0] + E[:, :nx0].T @ Y if param["form"] == "states" else None
    return dict(gq=gz[:SX], gr=gz[SX:], gb=Y, gx0=_gx0(t, param, db, dg, nx0, gz, Y, direct), n_reg=n_reg,
                in_range=rec.in_range(M, Y, R), **rec.fields())


def dense_shifted(d, x, u, param, w, shift, zero, kinds=None):
    """(c): the system dual_form solved, (M + diag(shift)) Y = R without the zero-column entries, by one dense solve (sens_ref.shifted_solve:
    float64 refined once in longdouble), then the gq / gr / gb / gx0 formulas.  Takes only shift and zero from dual_form; shares no
    elimination with it."""
    t, Pm, M = SR.dual_system(d, x, u, kinds)
    db, dg, nx0 = SR._param_terms(t, param)
    W = stack(t, w)
    E, SX = t["E"], t["SX"]
    Y = SR.shifted_solve(M, shift, zero, -E @ (Pm @ W))
    gz = -Pm @ (W + E.T @ Y)
    direct = W[:nx0] + E[:, :nx0].T @ Y if param["form"] == "states" else None
    return dict(gq=gz[:SX], gr=gz[SX:], gb=Y, gx0=_gx0(t, param, db, dg, nx0, gz, Y, direct))

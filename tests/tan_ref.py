"""The tangent of a tree QP's solution at a point (x, u) with the active set frozen there, two ways in numpy: for nd directions
(dq, dr, db, dx0) of the linear terms, dx, du, dlam and du0 (the u rows of the root).
(a) dense_kkt: one dense solve (lstsq) of the full frozen-set KKT system of sens_ref.dense_kkt (pinned rows included) with the right-hand
    side [-(dh + dg/dx0 dx0); -(db + db/dx0 dx0); dfix], dfix = dx0 on the states of a root that keeps them;
(b) dual_form: R_c = (P_c dh_c)^x - C_c P_p dh_p + db_c + G_c dx0, M dLam = R, dZ_k = P_k ([dLam_k; 0] - sum_c C_c' dLam_c) - P_k dh_k +
    direct_k dx0 as include/treeqp_amd.h states them, block by block (leaf to root, root, root to leaves) with the regularisation rule of
    reg_ref.py, as adj_ref.dual_form does for the adjoint; it also returns n_reg and in_range, the residual of the matrix actually solved.
Both take the arguments of sens_ref (the flat problem d, the point, the parameter form, kinds) and dirs = (dq, dr, db, dx0), each None
(zero), (rows,) or (rows, nd) in the flat layouts of q, r, b and x0, and return dict(dx, du, dlam, du0, ...) with nd columns."""
from __future__ import annotations

import numpy as np

import reg_ref as RR
import sens_ref as SR


def stack(t, nx0, dirs):
    """(DH (n, nd), DB (SL, nd), DX0 (nx0, nd)); a missing direction is zero"""
    rows = (t["SX"], t["SU"], t["SL"], nx0)
    parts = [None if a is None else np.asarray(a, dtype=np.float64).reshape((r, -1), order="F") for a, r in zip(dirs, rows)]
    nd = next((a.shape[1] for a in parts if a is not None), 1)
    full = [np.zeros((r, nd)) if a is None else a for a, r in zip(parts, rows)]
    return np.vstack(full[:2]), full[2], full[3]


def _split(t, dz, dlam):
    SX, nu0 = t["SX"], int(t["nu"][0])
    return dict(dx=dz[:SX], du=dz[SX:], du0=dz[SX:SX + nu0], dlam=dlam)


def dense_kkt(d, x, u, param, dirs, kinds=None):
    """(a): [H E' F'; E 0 0; F 0 0] [dz; dlam; dmu] = [-(dh + dg dx0); -(db + db0 dx0); dfix]"""
    t = SR._assemble(d, kinds)
    db0, dg0, nx0 = SR._param_terms(t, param)
    DH, DB, DX0 = stack(t, nx0, dirs)
    on = SR.pinned(d, x, u, kinds)
    fi = np.flatnonzero(on)
    F = np.zeros((len(fi), t["n"]))
    F[np.arange(len(fi)), fi] = 1.0
    dfix = np.zeros((len(fi), DH.shape[1]))
    if param["form"] == "states":
        assert all(on[:nx0]), "the root's states are not on their bounds"
        for r, i in enumerate(fi):
            if i < nx0:
                dfix[r] = DX0[i]
    m = t["SL"] + len(fi)
    Cm = np.vstack([t["E"], F])
    Kmat = np.block([[t["H"], Cm.T], [Cm, np.zeros((m, m))]])
    rhs = np.vstack([-(DH + dg0 @ DX0), -(DB + db0 @ DX0), dfix])
    sol = np.linalg.lstsq(Kmat, rhs, rcond=None)[0]
    out = _split(t, sol[:t["n"]], sol[t["n"]:t["n"] + t["SL"]])
    out.update(residual=float(np.max(np.abs(Kmat @ sol - rhs))) if rhs.size else 0.0, scale=max(1.0, float(np.max(np.abs(sol))) if sol.size else 1.0))
    return out


def dual_form(d, x, u, param, dirs, kinds=None, regType=2, regTol=1e-6, regValue=1e-6):
    """(b): the formulas of the header, block by block"""
    t = SR._assemble(d, kinds)
    db0, dg0, nx0 = SR._param_terms(t, param)
    DH, DB, DX0 = stack(t, nx0, dirs)
    nk, nx, xo, dad, n, SL, E = t["nk"], t["nx"], t["xo"], t["dad"], t["n"], t["SL"], t["E"]
    on = SR.pinned(d, x, u, kinds)
    Pm = np.zeros((n, n))
    for k in range(t["Nn"]):
        ii = t["idx"][k]
        Hk = t["H"][np.ix_(ii, ii)]
        if t["kinds"][k] == 0:
            Pm[ii, ii] = np.where(on[ii], 0.0, 1.0 / np.diag(Hk))
        elif len(ii):
            Pm[np.ix_(ii, ii)] = np.linalg.inv(Hk)
    direct = -Pm @ dg0
    if param["form"] == "states":
        direct[:nx0] = np.eye(nx0)
    M = E @ Pm @ E.T
    G = E @ direct + db0
    R = -E @ (Pm @ DH) + DB + G @ DX0
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
    Y = np.zeros((SL, R.shape[1]))
    for j in range(R.shape[1]):
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
    dz = -Pm @ (DH + E.T @ Y) + direct @ DX0
    out = _split(t, dz, Y)
    out.update(n_reg=n_reg, in_range=rec.in_range(M, Y, R))
    return out


def _fma(a, b, c):
    """fma(a, b, c) of float64 scalars, correctly rounded, through exact rational arithmetic"""
    from fractions import Fraction
    if a == 0.0 or b == 0.0:
        return float(c) + 0.0 if c != 0.0 else 0.0
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def window_direction(c, t0, t1):
    """(dq, dr) flat: the direction tqgpu_mpc_predict_at builds for a window move t0 -> t1 on tracking case c, the chain of the header entry
    by entry: dxref = xtraj[rho(t1)] - xtraj[rho(t0)]; kind 0 fma(-Qd[i], dxref[i], 0.0); kinds 1: row i of H_k, the x columns then the u columns;
    the u rows of an eliminated root with S0 go on with fma(-S0[i, j], dxref[j], .)"""
    import helpers as H
    import tracking_cases as TC
    d = c["d"]
    nx, nu = [np.asarray(d[n], dtype=int) for n in ("nx", "nu")]
    xo, uo = H.offsets(d)
    st = TC.stages(d["nk"])
    dq, dr = np.zeros(int(xo[-1])), np.zeros(int(uo[-1]))
    kinds = np.zeros(len(nx), dtype=int) if c["kinds"] is None else np.asarray(c["kinds"], dtype=int)
    for k in range(len(nx)):
        r1, r0 = min(t1 + st[k], c["T"] - 1), min(t0 + st[k], c["T"] - 1)
        dxr = (c["xtraj"][r1] - c["xtraj"][r0]) if nx[k] else np.zeros(0)
        dur = (c["utraj"][r1] - c["utraj"][r0]) if nu[k] else np.zeros(0)
        Q, Rm, Sm = TC.blocks(d, k)
        Hk = np.block([[Q, Sm.T], [Sm, Rm]])
        ref = np.concatenate([dxr, dur])
        for i in range(nx[k] + nu[k]):
            if kinds[k] == 0:
                v = _fma(-Hk[i, i], ref[i], 0.0)
            else:
                v = 0.0
                for j in range(nx[k] + nu[k]):
                    v = _fma(-Hk[i, j], ref[j], v)
                if k == 0 and i >= nx[k] and c["form"] == "elim" and c["root"]["S0"] is not None:
                    dx0r = c["xtraj"][min(t1, c["T"] - 1)] - c["xtraj"][min(t0, c["T"] - 1)]
                    for j in range(c["nx0"]):
                        v = _fma(-c["root"]["S0"][i - nx[k], j], dx0r[j], v)
            if i < nx[k]:
                dq[xo[k] + i] = v
            else:
                dr[uo[k] + i - nx[k]] = v
    return dq, dr

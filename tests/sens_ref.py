"""Sensitivities of a tree QP's solution with respect to x0 at a point (x, u) with the active set frozen there, two ways in numpy:
(a) dense_kkt: the equality-constrained QP with the entries that sit on a bound pinned, differentiated in x0, solved by lstsq;
(b) dual_form: M dLam = G, dZ = P (..) + direct as include/treeqp_amd.h states them, block by block with the regularisation rule
    of reg_ref.py; it also returns what that rule did (class RegRecord: flagged, pivots, shift, zero, guard), and in_range, the residual
    of the matrix actually solved, M + diag(shift) without the zero-column entries;
(c) dense_shifted: that same shifted system by one dense solve (float64, refined once in longdouble), given shift and zero.
(a) and (b) take the flat problem d (clipping: Qd, Rd; kinds given: Q, R, S column major), the point and the parameter form:
    dict(form="eliminated", A0=[(nx[kid], nx0) ...], S0=None or (nu[0], nx0))      x0 enters b of the root's children and r[0]
    dict(form="states")                                                            x0 enters as xmin[0] = xmax[0] = x0
and return dict(K, dx, du, dlam, ...), column j for parameter x0[j], rows in the flat layout of tqgpu_get_solution."""
from __future__ import annotations

import numpy as np

import reg_ref as RR
from treeqp_amd import problems as P


def _assemble(d, kinds):
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    Nn = len(nk)
    xo, uo = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nu)])
    SX, SU = int(xo[-1]), int(uo[-1])
    n = SX + SU
    dad = P.parents_of(nk)
    kinds = np.zeros(Nn, dtype=int) if kinds is None else np.asarray(kinds, dtype=int)
    H = np.zeros((n, n))
    qo = ro = so = 0
    idx = []
    for k in range(Nn):
        a, m = int(nx[k]), int(nu[k])
        ix, iu = np.arange(xo[k], xo[k + 1]), SX + np.arange(uo[k], uo[k + 1])
        idx.append(np.concatenate([ix, iu]))
        if "Q" in d:
            Q = d["Q"][qo:qo + a * a].reshape((a, a), order="F"); qo += a * a
            R = d["R"][ro:ro + m * m].reshape((m, m), order="F"); ro += m * m
            S = d["S"][so:so + m * a].reshape((m, a), order="F"); so += m * a
            if kinds[k] == 0:
                Q, R, S = np.diag(np.diag(Q)), np.diag(np.diag(R)), np.zeros((m, a))
            H[np.ix_(ix, ix)] = Q; H[np.ix_(iu, iu)] = R; H[np.ix_(iu, ix)] = S; H[np.ix_(ix, iu)] = S.T
        else:
            H[ix, ix] = d["Qd"][xo[k]:xo[k + 1]]; H[iu, iu] = d["Rd"][uo[k]:uo[k + 1]]
    SL = SX - int(nx[0])
    E = np.zeros((SL, n))
    ao = bo = 0
    for k in range(1, Nn):
        p = dad[k]
        A = d["A"][ao:ao + nx[k] * nx[p]].reshape((nx[k], nx[p]), order="F"); ao += nx[k] * nx[p]
        B = d["B"][bo:bo + nx[k] * nu[p]].reshape((nx[k], nu[p]), order="F"); bo += nx[k] * nu[p]
        rows = np.arange(xo[k], xo[k + 1]) - nx[0]
        E[np.ix_(rows, np.arange(xo[k], xo[k + 1]))] = -np.eye(nx[k])
        E[np.ix_(rows, np.arange(xo[p], xo[p + 1]))] = A
        E[np.ix_(rows, SX + np.arange(uo[p], uo[p + 1]))] = B
    return dict(nk=nk, nx=nx, nu=nu, Nn=Nn, xo=xo, uo=uo, SX=SX, SU=SU, n=n, SL=SL, dad=dad, kinds=kinds, H=H, E=E, idx=idx)


def pinned(d, x, u, kinds=None):
    """the entries of z = [x | u] that equal one of their bounds bit for bit (kind-0 nodes; kind 1 ignores its bounds)"""
    t = _assemble(d, kinds)
    z = np.concatenate([x, u])
    lo, hi = np.concatenate([d["xmin"], d["umin"]]), np.concatenate([d["xmax"], d["umax"]])
    on = (z == lo) | (z == hi)
    for k in range(t["Nn"]):
        if t["kinds"][k] != 0:
            on[t["idx"][k]] = False
    return on


def _param_terms(t, param):
    """(d b / d x0 (SL x nx0), d g / d x0 (n x nx0), nx0)"""
    nx, xo, SX = t["nx"], t["xo"], t["SX"]
    if param["form"] == "states":
        nx0 = int(nx[0])
        return np.zeros((t["SL"], nx0)), np.zeros((t["n"], nx0)), nx0
    A0 = [np.asarray(M, dtype=np.float64) for M in param["A0"]]
    nx0 = A0[0].shape[1]
    db, dg = np.zeros((t["SL"], nx0)), np.zeros((t["n"], nx0))
    at = 0
    for M in A0:
        db[at:at + M.shape[0]] = M
        at += M.shape[0]
    if param.get("S0") is not None:
        dg[SX:SX + int(t["nu"][0])] = np.asarray(param["S0"], dtype=np.float64)
    return db, dg, nx0


def _split(t, dz, dlam):
    SX, nu0 = t["SX"], int(t["nu"][0])
    return dict(dx=dz[:SX], du=dz[SX:], K=dz[SX:SX + nu0], dlam=dlam)


def dense_kkt(d, x, u, param, kinds=None):
    """(a): [H E' F'; E 0 0; F 0 0] [dz; dlam; dmu] = [-dg; -db; dfix], F the rows of the pinned entries, by lstsq"""
    t = _assemble(d, kinds)
    db, dg, nx0 = _param_terms(t, param)
    on = pinned(d, x, u, kinds)
    fi = np.flatnonzero(on)
    F = np.zeros((len(fi), t["n"]))
    F[np.arange(len(fi)), fi] = 1.0
    dfix = np.zeros((len(fi), nx0))
    if param["form"] == "states":
        for r, i in enumerate(fi):
            if i < nx0:
                dfix[r, i] = 1.0
        assert all(on[:nx0]), "the root's states are not on their bounds"
    m = t["SL"] + len(fi)
    C = np.vstack([t["E"], F])
    Kmat = np.block([[t["H"], C.T], [C, np.zeros((m, m))]])
    rhs = np.vstack([-dg, -db, dfix])
    sol = np.linalg.lstsq(Kmat, rhs, rcond=None)[0]
    resid = float(np.max(np.abs(Kmat @ sol - rhs))) if rhs.size else 0.0
    out = _split(t, sol[:t["n"]], sol[t["n"]:t["n"] + t["SL"]])
    out.update(residual=resid, n_pinned=len(fi), scale=max(1.0, float(np.max(np.abs(sol))) if sol.size else 1.0))
    return out


def dual_form(d, x, u, param, kinds=None, regType=2, regTol=1e-6, regValue=1e-6):
    """(b): the formulas of the header, block by block"""
    t = _assemble(d, kinds)
    db, dg, nx0 = _param_terms(t, param)
    nk, nx, nu, xo, dad, n, SL, E = t["nk"], t["nx"], t["nu"], t["xo"], t["dad"], t["n"], t["SL"], t["E"]
    on = pinned(d, x, u, kinds)
    Pm = np.zeros((n, n))
    for k in range(t["Nn"]):
        ii = t["idx"][k]
        Hk = t["H"][np.ix_(ii, ii)]
        if t["kinds"][k] == 0:
            Pm[ii, ii] = np.where(on[ii], 0.0, 1.0 / np.diag(Hk))
        elif len(ii):
            Pm[np.ix_(ii, ii)] = np.linalg.inv(Hk)
    direct = -Pm @ dg
    if param["form"] == "states":
        direct[:nx0] = np.eye(nx0)
    M = E @ Pm @ E.T
    G = E @ direct + db
    # block elimination, last parent first; block p = the duals of the children of p
    Np = int(np.count_nonzero(nk > 0))
    kid0 = np.concatenate([[1], 1 + np.cumsum(nk)[:-1]])
    rng_of = lambda p: np.arange(xo[kid0[p]], xo[kid0[p] + nk[p]]) - nx[0]
    own = lambda p: np.arange(xo[p], xo[p + 1]) - nx[0]
    W = {p: M[np.ix_(rng_of(p), rng_of(p))].copy() for p in range(Np)}
    fac, n_reg = {}, 0
    rec = RegRecord(SL)
    for p in range(Np - 1, -1, -1):
        Wp = W[p] + (regValue * np.eye(len(W[p])) if regType == 1 else 0.0)
        L, inv = RR.potrf(Wp)
        rec.first_pass(p, rng_of(p), np.diag(L), regType, regTol, regValue)
        if regType == 2 and np.any(np.diag(L) <= regTol):
            n_reg += 1
            L, inv = RR.potrf(Wp + regValue * np.eye(len(Wp)))
        rec.final(rng_of(p), inv)
        Y = None
        if p > 0:
            Ut = M[np.ix_(own(p), rng_of(p))]
            Y = RR._right_solve(Ut, L, inv)
            pos = own(p) - rng_of(dad[p])[0]
            W[dad[p]][np.ix_(pos, pos)] -= Y @ Y.T
        fac[p] = (L, inv, Y)
    dlam = np.zeros((SL, nx0))
    for j in range(nx0):
        L, inv, _ = fac[0]
        dlam[rng_of(0), j] = RR._backward(L, inv, RR._forward(L, inv, G[rng_of(0), j]))
        for p in range(1, Np):
            L, inv, Y = fac[p]
            dlam[rng_of(p), j] = -RR._backward(L, inv, Y.T @ dlam[own(p), j])
    dz = -Pm @ E.T @ dlam + direct
    out = _split(t, dz, dlam)
    out.update(n_reg=n_reg, in_range=rec.in_range(M, dlam, G), **rec.fields())
    return out


class RegRecord:
    """What the block elimination of dual_form (here and in adj_ref) did to the matrix it solved, kept as reg_ref.block_newton_step keeps it:
    flagged: the blocks (parent ids, in the order they are factorised) whose diagonal was shifted;
    pivots: per block the L_jj of the first pass, all of them;
    shift, zero: per dual entry, what was added to its diagonal and whether its column of the factor in use is a zero column;
    guard: the smallest, over every non-zero L_jj of a first pass, of max(L_jj / regTol, regTol / L_jj) (regType 0 and 1 do not compare
    with regTol: L_jj / regTol there); an exact 0 counts as infinity, and so does every L_jj where regTol is 0."""

    def __init__(self, SL):
        self.flagged, self.pivots, self.guard = [], {}, np.inf
        self.shift, self.zero = np.zeros(SL), np.zeros(SL, dtype=bool)

    def first_pass(self, p, rows, diag, regType, regTol, regValue):
        diag = np.array(diag, dtype=np.float64, copy=True)
        self.pivots[p] = diag
        for v in diag[diag != 0]:
            if regTol > 0:
                self.guard = min(self.guard, float(max(v / regTol, regTol / v) if regType == 2 else v / regTol))
        if regType == 1 or (regType == 2 and np.any(diag <= regTol)):
            self.flagged.append(p)
            self.shift[rows] += regValue

    def final(self, rows, inv):
        self.zero[rows] = np.asarray(inv) == 0

    def in_range(self, M, sol, rhs):
        """max |(M + diag(shift)) sol - rhs| over the entries that are not zero columns: the matrix actually solved"""
        keep = ~self.zero
        if not np.any(keep):
            return 0.0
        Ms = (M + np.diag(self.shift))[np.ix_(keep, keep)]
        return float(np.max(np.abs(Ms @ sol[keep] - rhs[keep]), initial=0.0))

    def fields(self):
        return dict(flagged=list(self.flagged), pivots=self.pivots, shift=self.shift.copy(), zero=self.zero.copy(), guard=self.guard)


def _refined_solve(Ms, rhs):
    """one dense float64 solve refined once in longdouble, as reg_ref.block_newton_step does its cross-check"""
    LD = np.longdouble
    M64 = Ms.astype(np.float64)
    x = np.linalg.solve(M64, rhs.astype(np.float64)).astype(LD)
    x = x + np.linalg.solve(M64, (rhs.astype(LD) - Ms.astype(LD) @ x).astype(np.float64)).astype(LD)
    return x.astype(np.float64)


def dual_system(d, x, u, kinds=None):
    """(t, P, M = E P E') at the point, for dense_shifted here and in adj_ref: no elimination, no regularisation"""
    t = _assemble(d, kinds)
    on = pinned(d, x, u, kinds)
    Pm = np.zeros((t["n"], t["n"]))
    for k in range(t["Nn"]):
        ii = t["idx"][k]
        if t["kinds"][k] == 0:
            free = ii[~on[ii]]
            Pm[free, free] = 1.0 / t["H"][free, free]
        elif len(ii):
            Pm[np.ix_(ii, ii)] = np.linalg.inv(t["H"][np.ix_(ii, ii)])
    return t, Pm, t["E"] @ Pm @ t["E"].T


def shifted_solve(M, shift, zero, rhs):
    """(M + diag(shift)) without the zero-column entries, solved densely for every column of rhs; the zero-column entries get 0.0"""
    keep = ~np.asarray(zero, dtype=bool)
    sol = np.zeros_like(rhs, dtype=np.float64)
    if np.any(keep):
        sol[keep] = _refined_solve((M + np.diag(shift))[np.ix_(keep, keep)], rhs[keep])
    return sol


def dense_shifted(d, x, u, param, shift, zero, kinds=None):
    """(c): the system dual_form solved, (M + diag(shift)) dLam = G without the zero-column entries, by one dense solve, then
    dZ = -P E' dLam + direct.  Takes only shift and zero from dual_form; shares no elimination with it."""
    t, Pm, M = dual_system(d, x, u, kinds)
    db, dg, nx0 = _param_terms(t, param)
    direct = -Pm @ dg
    if param["form"] == "states":
        direct[:nx0] = np.eye(nx0)
    G = t["E"] @ direct + db
    dlam = shifted_solve(M, shift, zero, G)
    return _split(t, -Pm @ t["E"].T @ dlam + direct, dlam)

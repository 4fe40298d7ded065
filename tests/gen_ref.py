"""The numpy reference of the stage solver for general constraints (device kind 3, stage_gen), on top of newton_ref.py (imported,
not edited; no code shared with the device path).

The stage QP of a kind-3 node is  min 1/2 z'Hz - h'z  s.t.  lo <= z <= hi,  dlo <= G z <= dhi,  G = [C | D] (nc x nz).  A problem
dict carries the rows as d["nc"] (per node), d["C"], d["D"] (flat, node after node, column major), d["dmin"], d["dmax"].

`solve_gen` is a dual active-set method on dense KKT systems (bounds and rows alike are rows of [I; G]); its answer does not rest
on that method: the strictly convex QP has one KKT point, and `certify_gen` checks in longdouble that the returned point is it
(stationarity, feasibility, the sign of every multiplier, complementarity).  `enumerate_gen` finds the KKT point of a small QP by
trying every working set.  Multipliers have the sign of the container's KKT check (qp_container.c): H z - h + mu + G'mu_d = 0,
negative on a lower bound / dmin, positive on an upper bound / dmax."""
from __future__ import annotations

import itertools

import numpy as np

import newton_ref as N

LD = N.LD
STATS = dict(drops=0)  # members dropped from a working set (partial steps) by solve_gen since the caller last reset it
FEAS_TOL = 1e-12      # of (|G||z| + |d|)_r: feasibility of a row whose value comes out of a refined KKT solve


def cons_of(d):
    """per node (G, dlo, dhi), G = [C | D] in float64, the ranges in longdouble; None on a node without rows"""
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
        out.append((np.hstack([Ck, Dk]).astype(np.float64), np.asarray(d["dmin"][orow:orow + m], LD), np.asarray(d["dmax"][orow:orow + m], LD)))
        orow += m
    return out


def set_cons(d, cons):
    """write per-node (G, dlo, dhi) (None: no rows) into d as nc, C, D, dmin, dmax"""
    nx = np.asarray(d["nx"], int)
    d["nc"] = np.asarray([0 if c is None else c[0].shape[0] for c in cons], np.int32)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    d["C"] = cat([c[0][:, :nx[k]].ravel(order="F") for k, c in enumerate(cons) if c is not None])
    d["D"] = cat([c[0][:, nx[k]:].ravel(order="F") for k, c in enumerate(cons) if c is not None])
    d["dmin"] = cat([np.asarray(c[1], np.float64) for c in cons if c is not None])
    d["dmax"] = cat([np.asarray(c[2], np.float64) for c in cons if c is not None])
    return d


def eqp(Hk, h, lo, hi, G, dlo, dhi, sb, sr):
    """The minimiser with the entries sb != 0 on their bound (-1 lower, +1 upper) and the rows sr != 0 on dlo / dhi.  Returns (z,
    mu_d, P, cond): fixed entries ARE the bound; mu_d the row multipliers (0 off the working set); P the elimination matrix of the
    working set; cond the condition of G_W H_FF^-1 G_W'."""
    n, m = len(h), len(dlo)
    H64, HL, GL = np.asarray(Hk, np.float64), np.asarray(Hk, LD), np.asarray(G, LD)
    A, W = sb != 0, sr != 0
    F = ~A
    z = np.zeros(n, LD)
    z[A] = np.where(sb[A] < 0, lo[A], hi[A])
    nf, nw = int(F.sum()), int(W.sum())
    K = np.zeros((nf + nw, nf + nw))
    K[:nf, :nf] = H64[np.ix_(F, F)]
    K[:nf, nf:] = np.asarray(G, np.float64)[np.ix_(W, F)].T
    K[nf:, :nf] = K[:nf, nf:].T
    rhs = np.concatenate([h[F] - HL[np.ix_(F, A)] @ z[A], np.where(sr[W] < 0, dlo[W], dhi[W]) - GL[np.ix_(W, A)] @ z[A]])
    mu = np.zeros(m, LD)
    P = np.zeros((n, n), LD)
    cond = 1.0
    if nf + nw:
        sol = N._refined_solve(K, rhs)
        z[F] = sol[:nf]
        mu[W] = sol[nf:]
        P[np.ix_(F, F)] = np.linalg.inv(K)[:nf, :nf].astype(LD)
        if nw:
            GF = K[nf:, :nf]
            cond = float(np.linalg.cond(GF @ np.linalg.solve(K[:nf, :nf], GF.T))) if nf else np.inf
    return z, mu, P, cond


def solve_gen(Hk, h, lo, hi, G, dlo, dhi):
    """argmin 1/2 z'Hz - h'z, lo <= z <= hi, dlo <= G z <= dhi -> (z, sb, sr, mu_d, P, condS).  Dual active-set method (Goldfarb and
    Idnani) from the minimiser over the equalities; raises ValueError on an infeasible QP."""
    n, m = len(h), len(dlo)
    h, lo, hi, dlo, dhi = [np.asarray(v, LD) for v in (h, lo, hi, dlo, dhi)]
    H64, HL = np.asarray(Hk, np.float64), np.asarray(Hk, LD)
    A = np.vstack([np.eye(n), np.asarray(G, np.float64).reshape(m, n)])
    AL = A.astype(LD)
    bl, bu = np.concatenate([lo, dlo]), np.concatenate([hi, dhi])
    eq = bl == bu
    side = np.where(eq, -1, 0)

    def kkt(W, top, bot):
        Nw = (-side[W])[:, None] * A[W]
        K = np.zeros((n + len(W), n + len(W)))
        K[:n, :n] = H64; K[:n, n:] = Nw.T; K[n:, :n] = Nw
        sol = N._refined_solve(K, np.concatenate([top, bot]))
        return sol[:n], sol[n:]

    W = [int(i) for i in np.flatnonzero(eq)]
    z, u = kkt(W, h, np.asarray([-side[i] * bl[i] for i in W], LD))
    u = -u                                                  # H z - h = N u
    for _ in range(8 * (n + m) + 16):
        Az = AL @ z
        scale = np.abs(AL) @ np.abs(z)
        with np.errstate(invalid="ignore"):
            v = np.maximum(np.where(bl - Az > 1e-14 * (scale + np.abs(bl)), bl - Az, 0), np.where(Az - bu > 1e-14 * (scale + np.abs(bu)), Az - bu, 0))
        v[W] = 0
        if not np.any(v > 0):
            break
        p = int(np.argmax(v))
        sp = -1 if bl[p] - Az[p] > 0 else 1
        npv = -sp * AL[p]
        bp = -sp * (bl[p] if sp < 0 else bu[p])
        up = LD(0)
        while True:
            dz, r = kkt(W, npv, np.zeros(len(W), LD))
            q = npv @ dz
            dep = not q > 1e-12 * (npv @ N._refined_solve(H64, npv))
            t1, jb = LD(np.inf), -1
            for j, i in enumerate(W):
                if not eq[i] and r[j] > 0 and max(u[j], LD(0)) / r[j] < t1:
                    t1, jb = max(u[j], LD(0)) / r[j], j
            t2 = LD(np.inf) if dep else (bp - npv @ z) / q
            if not np.isfinite(min(t1, t2)):
                raise ValueError("the stage QP is infeasible")
            t = min(t1, t2)
            if not dep:
                z = z + t * dz
            u = u - t * r
            up = up + t
            if t2 <= t1:
                W.append(p); side[p] = sp; u = np.concatenate([u, [up]])
                break
            STATS["drops"] += 1
            side[W[jb]] = 0
            del W[jb]
            u = np.delete(u, jb)
    else:
        raise AssertionError("the active-set method of the reference did not finish")
    sb, sr = side[:n].copy(), side[n:].copy()
    z, mu, P, cond = eqp(Hk, h, lo, hi, G, dlo, dhi, sb, sr)
    return z, sb, sr, mu, P, cond


def certify_gen(Hk, h, lo, hi, G, dlo, dhi, z, sb, sr, mu_d):
    """The KKT conditions at (z, sb, sr, mu_d) in longdouble.  Returns (violation, margin): violation is the largest of the
    stationarity and sign defects relative to (|H||z| + |h| + |G'||mu_d|)_i (<= newton_ref.CERT_TOL for a certified answer) and
    of the feasibility defects of the rows relative to (|G||z| + |d|)_r / FEAS_TOL * CERT_TOL; margin the smallest, over the
    entries and rows whose bounds differ, of the distance of an inactive one to either side and of the multiplier of an active
    one (strict complementarity and strict inactivity)."""
    HL, GL = np.asarray(Hk, LD), np.asarray(G, LD).reshape(len(dlo), len(h))
    h, lo, hi, dlo, dhi, mu_d = [np.asarray(v, LD) for v in (h, lo, hi, dlo, dhi, mu_d)]
    g = HL @ z - h + GL.T @ mu_d                              # = -mu of the bounds
    scale = np.abs(HL) @ np.abs(z) + np.abs(h) + np.abs(GL.T) @ np.abs(mu_d) + LD(1e-300)
    free, open_ = sb == 0, lo < hi
    assert np.all(z[sb == -1] == lo[sb == -1]) and np.all(z[sb == 1] == hi[sb == 1])
    assert np.all((z >= lo) & (z <= hi)), "a free entry is outside its bounds"
    defect = np.where(free, np.abs(g), np.where(~open_, LD(0), np.where(sb == -1, np.maximum(-g, 0), np.maximum(g, 0))))
    viol = float(np.max(defect / scale)) if len(z) else 0.0
    act = GL @ z
    rs = np.abs(GL) @ np.abs(z) + LD(1e-300)
    inw, ropen = sr != 0, dlo < dhi
    with np.errstate(invalid="ignore"):
        feas = np.where(inw, np.abs(act - np.where(sr < 0, dlo, dhi)), np.maximum(np.maximum(dlo - act, act - dhi), 0))
        feas = feas / (rs + np.where(np.isfinite(dlo), np.abs(dlo), 0) + np.where(np.isfinite(dhi), np.abs(dhi), 0))
    viol = max(viol, float(np.max(feas, initial=0.0)) * N.CERT_TOL / FEAS_TOL)
    assert not np.any(mu_d[~inw]), "a row outside the working set has a multiplier"
    wrong = inw & ropen & (((sr < 0) & (mu_d > 0)) | ((sr > 0) & (mu_d < 0)))
    assert not np.any(wrong), "a row multiplier of the wrong sign"
    with np.errstate(invalid="ignore"):
        dist = np.where(free, np.minimum(z - lo, hi - z), np.abs(g))
        rdist = np.where(inw, np.abs(mu_d), np.minimum(act - dlo, dhi - act))
    margin = min(float(np.min(dist[open_], initial=np.inf)), float(np.min(rdist[ropen], initial=np.inf)))
    return viol, margin


def enumerate_gen(Hk, h, lo, hi, G, dlo, dhi, tol=1e-9):
    """every working set of a small QP (nz + nc <= 8): the list of (z, sb, sr, mu_d) that are KKT points to `tol`"""
    n, m = len(h), len(dlo)
    assert n + m <= 8
    h, lo, hi, dlo, dhi = [np.asarray(v, LD) for v in (h, lo, hi, dlo, dhi)]
    HL, GL = np.asarray(Hk, LD), np.asarray(G, LD).reshape(m, n)
    found = []
    for s in itertools.product((-1, 0, 1), repeat=n + m):
        s = np.asarray(s)
        sb, sr = s[:n], s[n:]
        if np.any((sb == 1) & (lo == hi)) or np.any((sr == 1) & (dlo == dhi)) or np.any((sb == 0) & (lo == hi)) or np.any((sr == 0) & (dlo == dhi)):
            continue
        if np.any(~np.isfinite(np.where(sb < 0, lo, np.where(sb > 0, hi, 0)))) or np.any(~np.isfinite(np.where(sr < 0, dlo, np.where(sr > 0, dhi, 0)))):
            continue
        if np.sum(sr != 0) > np.sum(sb == 0):
            continue
        try:
            z, mu, _, cond = eqp(Hk, h, lo, hi, G, dlo, dhi, sb, sr)
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(z.astype(np.float64))) or cond > 1e12:
            continue
        g = HL @ z - h + GL.T @ mu
        act = GL @ z
        okb = np.all(z >= lo - tol) and np.all(z <= hi + tol) and np.all(act >= dlo - tol) and np.all(act <= dhi + tol)
        oks = np.all(np.where((sb == -1) & (lo < hi), g >= -tol, True)) and np.all(np.where((sb == 1), g <= tol, True))
        okr = np.all(np.where((sr == -1) & (dlo < dhi), mu <= tol, True)) and np.all(np.where(sr == 1, mu >= -tol, True))
        if okb and oks and okr:
            found.append((z, sb, sr, mu))
    return found


# ---------------------------------------------------------------------------------------------------------------------------
# the Newton step of a tree with kind-3 nodes (newton_ref's, with the stage solutions of those nodes from solve_gen)
# ---------------------------------------------------------------------------------------------------------------------------

def _kinds2(kinds):
    kinds = np.asarray(kinds, int)
    return np.where(kinds == 3, 2, kinds)


def stage_solutions(d, lam, kinds):
    """newton_ref.stage_solutions with the kind-3 nodes solved by solve_gen (P from the final working set); adds rside (per node
    the side of every row, empty without rows), mu_d (per node), condS (the largest condition of S on a working set)."""
    kinds = np.asarray(kinds, int)
    cons = cons_of(d)
    gen = [k for k in range(len(kinds)) if kinds[k] == 3 and cons[k] is not None]
    # the other nodes as newton_ref has them (a kind-3 node is solved there as a box node first and replaced below)
    st = N.stage_solutions(d, lam, kinds=_kinds2(kinds))
    tree, H, hs, los, his = N.stage_data(d, lam, kinds=_kinds2(kinds))
    st["rside"] = [np.zeros(0 if c is None else len(c[1]), int) for c in cons]
    st["mu_d"] = [np.zeros(0 if c is None else len(c[1]), LD) for c in cons]
    st["condS"] = 1.0
    if gen:
        # the margin of the nodes that stay: recomputed without the box solutions of the kind-3 nodes
        margin = np.inf
        for k in range(len(kinds)):
            if k in gen or _kinds2(kinds)[k] == 1:
                continue
            if kinds[k] == 0:
                w = H[k].astype(LD)
                zu = hs[k] / w
                op = los[k] < his[k]
                if np.any(op):
                    margin = min(margin, float(np.min(np.minimum(np.abs(zu - los[k]), np.abs(zu - his[k]))[op])))
            else:
                margin = min(margin, N.certify_box(H[k], hs[k], los[k], his[k], st["z"][k], st["side"][k])[1])
        for k in gen:
            G, dlo, dhi = cons[k]
            z, sb, sr, mu, Pk, cs = solve_gen(H[k], hs[k], los[k], his[k], G, dlo, dhi)
            v, mg = certify_gen(H[k], hs[k], los[k], his[k], G, dlo, dhi, z, sb, sr, mu)
            assert v <= N.CERT_TOL, f"node {k}: the reference's own solution misses its certificate ({v:.2e})"
            st["z"][k], st["side"][k], st["P"][k] = z, sb, Pk
            st["rside"][k], st["mu_d"][k] = sr, mu
            st["cert"] = max(st["cert"], v)
            st["condS"] = max(st["condS"], cs)
            margin = min(margin, mg)
        st["margin"] = margin
    return st


def newton_step(d, lam0, kinds, reg=0.0):
    """newton_ref.newton_step on the stage solutions above (same assembly of M = G P G' and of the residual)"""
    st = stage_solutions(d, lam0, kinds)
    nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, _ = st["tree"]
    z, Pm = st["z"], st["P"]
    Nn = len(nk)
    n = int(nx[1:].sum())
    res = np.zeros(n, dtype=LD)
    M = np.zeros((n, n), dtype=LD)
    for k in range(1, Nn):
        p = dad[k]
        ik = slice(lo_[k], lo_[k] + nx[k])
        res[ik] = A[k] @ z[p][:nx[p]] + B[k] @ z[p][nx[p]:] + b[k] - z[k][:nx[k]]
        CP = np.hstack([A[k], B[k]]) @ Pm[p]
        for j in kids[p]:
            M[ik, lo_[j]:lo_[j] + nx[j]] += CP @ np.hstack([A[j], B[j]]).T
        M[ik, ik] += Pm[k][:nx[k], :nx[k]]
        if p > 0:
            ip = slice(lo_[p], lo_[p] + nx[p])
            M[ik, ip] += -CP[:, :nx[p]]
            M[ip, ik] += -CP[:, :nx[p]].T
    if reg:
        M = M + LD(reg) * np.eye(n, dtype=LD)
    M64 = M.astype(np.float64)
    dl = np.linalg.solve(M64, res.astype(np.float64)).astype(LD)
    dl = dl + np.linalg.solve(M64, (res - M @ dl).astype(np.float64)).astype(LD)
    return dict(dlam=dl.astype(np.float64), res=res.astype(np.float64), cond=float(np.linalg.cond(M64)), margin=st["margin"],
                cert=st["cert"], condS=st["condS"], stages=st)


def dual_terms(d, lam, kinds):
    return N.terms_of_stages(stage_solutions(d, lam, kinds), lam)[0]


def armijo_trials(d, lam0, dlam, res, opts, kinds):
    """newton_ref.armijo_trials with the dual terms above"""
    gamma, beta, cap = opts.lineSearchGamma, opts.lineSearchBeta, opts.lineSearchMaxIter
    lam0 = np.asarray(lam0, dtype=LD); dl = np.asarray(dlam, dtype=LD)
    t0 = dual_terms(d, lam0, kinds)
    f0 = t0.sum()
    dot = -(np.asarray(res, dtype=LD) @ dl)
    tau, slack = LD(1), np.inf
    for trial in range(1, cap + 1):
        t = dual_terms(d, lam0 + tau * dl, kinds)
        f, bound = t.sum(), f0 + LD(gamma) * tau * dot
        slack = min(slack, float(abs(f - bound) / (np.abs(t).sum() + np.abs(t0).sum())))
        if f <= bound:
            return trial, slack
        tau = LD(beta) * tau
    return cap + 1, slack


def flat_multipliers(d, st, h_stage=None):
    """mu_x, mu_u, mu_d (float64, flat) of the stage solutions st: mu = h - H z - G'mu_d on the fixed entries of the dense nodes
    with bounds, Q (z_unc - z) on clipping nodes, 0 on free entries.  h_stage: per node the h to pair with z (the device pairs
    phase S's h with the last trial's z on a MAXIMUM_ITERATIONS exit, on every entry); None: st's own, fixed entries only."""
    nx = st["tree"][1]
    kinds = st["tree"][-1]
    cons = cons_of(d)
    mx, mu_, md = [], [], []
    for k, zk in enumerate(st["z"]):
        h = st["h"][k] if h_stage is None else h_stage[k]
        if st["H"][k].ndim == 1:
            m = h - st["H"][k].astype(LD) * zk
        elif kinds[k] == 1:
            m = np.zeros(len(zk), LD)
        else:
            m = h - st["H"][k].astype(LD) @ zk
            if cons[k] is not None and len(st["mu_d"][k]):
                m = m - np.asarray(cons[k][0], LD).T @ st["mu_d"][k]
            if h_stage is None:
                m = np.where(st["side"][k] != 0, m, LD(0))
        mx.append(m[:nx[k]]); mu_.append(m[nx[k]:]); md.append(st["mu_d"][k])
    cat = lambda v: np.concatenate(v).astype(np.float64)
    return cat(mx), cat(mu_), cat(md)

"""The hot start of the stage solver for general constraints (stage_gen) in numpy, beside gen_ref.solve_gen (imported, not edited;
no code shared with the device path): the same dual active-set method started from a given working set.

`solve_gen_from(..., side0)` takes the stored set as one vector of sides over the bounds and the rows (-1 lower / dmin, +1 upper /
dmax, 0 outside), and does what the device does:

1. sanitise: entries beyond nz + nc are cut, a member whose bound on the stored side is infinite leaves, equalities are forced in;
2. dual-feasibility rounds: the minimiser on the set, then every member that is no equality and whose multiplier has the wrong
   sign leaves, all of them in one round, until none is left (the set only shrinks);
3. the Goldfarb-Idnani loop of gen_ref.solve_gen from there;
4. any ending but a solution (a dependent stored set, no step possible, the step cap) is followed by one cold solve.

Steps are counted as the device counts them (tqgpu_get_stage_steps): one per factorisation, i.e. one per dual-feasibility round
that drops members, one per direction computed, and one for the pass that finds nothing violated.  The answer is the solution of
the final working set's system (gen_ref.eqp), as solve_gen's."""
from __future__ import annotations

import numpy as np

import gen_ref as G
import newton_ref as N

LD = N.LD
DEP_COND = 1e12       # cond(N H^-1 N') beyond which a working set counts as dependent
SIGN_TOL = 1e-12      # of (|H||z| + |h| + |N'||u|): a multiplier below minus this has the wrong sign


class _NoSolution(Exception):
    """a pass that ends without a solution; steps: the steps it took, the one that failed included"""
    def __init__(self, what, steps):
        super().__init__(what)
        self.steps = steps


def sanitise(side, lo, hi, dlo, dhi):
    """step 1 of the module docstring on a vector of sides that already has the current sizes"""
    bl, bu = np.concatenate([lo, dlo]), np.concatenate([hi, dhi])
    side = np.asarray(side, int).copy()
    with np.errstate(invalid="ignore"):
        side[(side < 0) & ~np.isfinite(bl.astype(np.float64))] = 0
        side[(side > 0) & ~np.isfinite(bu.astype(np.float64))] = 0
    side[bl == bu] = -1
    return side


def _run(Hk, h, lo, hi, Gm, dlo, dhi, side, rounds):
    """one pass: (side, steps) of the final working set, or _NoSolution"""
    n, m = len(h), len(dlo)
    H64 = np.asarray(Hk, np.float64)
    A = np.vstack([np.eye(n), np.asarray(Gm, np.float64).reshape(m, n)])
    AL = A.astype(LD)
    bl, bu = np.concatenate([lo, dlo]), np.concatenate([hi, dhi])
    eq = bl == bu
    side = side.copy()
    cap = 4 * (n + m) + 8
    steps = 0

    def kkt(W, top, bot, counted=True):
        Nw = (-side[W])[:, None] * A[W]
        if len(W):
            S = Nw @ np.linalg.solve(H64, Nw.T)
            if len(W) > n or not np.linalg.cond(S) <= DEP_COND:
                # the device counts a step when it starts to factorise.  A direction's step is counted before kkt() is called; the
                # minimiser of the start is not (it shares its step with what follows), so its failed factorisation adds the one step
                # that the device has counted by then: a dependent stored set costs 1 + (the steps of the cold redo).
                raise _NoSolution("the working set is dependent", steps + (0 if counted else 1))
        K = np.zeros((n + len(W), n + len(W)))
        K[:n, :n] = H64; K[:n, n:] = Nw.T; K[n:, :n] = Nw
        sol = N._refined_solve(K, np.concatenate([top, bot]))
        return sol[:n], sol[n:]

    def minimiser(W):
        z, u = kkt(W, h, np.asarray([-side[i] * (bl[i] if side[i] < 0 else bu[i]) for i in W], LD), counted=False)
        return z, -u

    W = [int(i) for i in np.flatnonzero(side)]
    while True:
        z, u = minimiser(W)
        if not rounds:
            break
        Nw = (-side[W])[:, None] * AL[W]
        scale = np.abs(np.asarray(Hk, LD)) @ np.abs(z) + np.abs(h) + (np.abs(Nw.T) @ np.abs(u) if len(W) else 0)
        tol = SIGN_TOL * float(np.max(scale, initial=0.0))
        wrong = [j for j, i in enumerate(W) if not eq[i] and u[j] < -tol]
        if not wrong:
            break
        steps += 1
        if steps >= cap:
            raise _NoSolution("the step cap", steps)
        for j in wrong:
            side[W[j]] = 0
        W = [i for j, i in enumerate(W) if j not in wrong]
    while True:
        Az = AL @ z
        scale = np.abs(AL) @ np.abs(z)
        with np.errstate(invalid="ignore"):
            v = np.maximum(np.where(bl - Az > 1e-14 * (scale + np.abs(bl)), bl - Az, 0), np.where(Az - bu > 1e-14 * (scale + np.abs(bu)), Az - bu, 0))
        v[W] = 0
        if not np.any(v > 0):
            steps += 1
            return side, steps
        p = int(np.argmax(v))
        sp = -1 if bl[p] - Az[p] > 0 else 1
        npv = -sp * AL[p]
        bp = -sp * (bl[p] if sp < 0 else bu[p])
        up = LD(0)
        while True:
            steps += 1
            if steps >= cap:
                raise _NoSolution("the step cap", steps)
            dz, r = kkt(W, npv, np.zeros(len(W), LD))
            q = npv @ dz
            dep = not q > 1e-12 * (npv @ N._refined_solve(H64, npv))
            t1, jb = LD(np.inf), -1
            for j, i in enumerate(W):
                if not eq[i] and r[j] > 0 and max(u[j], LD(0)) / r[j] < t1:
                    t1, jb = max(u[j], LD(0)) / r[j], j
            t2 = LD(np.inf) if dep else (bp - npv @ z) / q
            if not np.isfinite(min(t1, t2)):
                raise _NoSolution("no step possible", steps)
            t = min(t1, t2)
            if not dep:
                z = z + t * dz
            u = u - t * r
            up = up + t
            if t2 <= t1:
                W.append(p); side[p] = sp; u = np.concatenate([u, [up]])
                break
            side[W[jb]] = 0
            del W[jb]
            u = np.delete(u, jb)


def solve_gen_from(Hk, h, lo, hi, Gm, dlo, dhi, side0=None):
    """argmin 1/2 z'Hz - h'z, lo <= z <= hi, dlo <= G z <= dhi, started from the working set side0 (None: cold) ->
    dict(z, sb, sr, mu_d, P, condS, steps, redo); raises ValueError on an infeasible QP"""
    n = len(h)
    h, lo, hi, dlo, dhi = [np.asarray(v, LD) for v in (h, lo, hi, dlo, dhi)]
    Gm = np.asarray(Gm, np.float64).reshape(len(dlo), n)
    steps, redo, side = 0, False, None
    if side0 is not None:
        s0 = np.asarray(side0, int)
        # bounds and rows of the stored set, each cut or padded to the current sizes
        sb0, sr0 = s0[:n], s0[n:]
        st = np.zeros(n + len(dlo), int)
        st[:len(sb0)] = sb0
        st[n:n + min(len(sr0), len(dlo))] = sr0[:len(dlo)]
        try:
            side, steps = _run(Hk, h, lo, hi, Gm, dlo, dhi, sanitise(st, lo, hi, dlo, dhi), True)
        except _NoSolution as e:
            redo, steps = True, e.steps
    if side is None:
        cold = sanitise(np.zeros(n + len(dlo), int), lo, hi, dlo, dhi)
        try:
            side, s2 = _run(Hk, h, lo, hi, Gm, dlo, dhi, cold, False)
        except _NoSolution as e:
            raise ValueError(f"the stage QP is infeasible ({e})")
        steps += s2
    sb, sr = side[:n].copy(), side[n:].copy()
    z, mu, P, cond = G.eqp(Hk, h, lo, hi, Gm, dlo, dhi, sb, sr)
    return dict(z=z, sb=sb, sr=sr, mu_d=mu, P=P, condS=cond, steps=steps, redo=redo)


def node_qps(d, lam, kinds):
    """per kind-3 node k with rows: (H, h, lo, hi, G, dlo, dhi) at the duals lam"""
    kinds = np.asarray(kinds, int)
    cons = G.cons_of(d)
    _, H, hs, los, his = N.stage_data(d, lam, kinds=G._kinds2(kinds))
    return {k: (H[k], hs[k], los[k], his[k], cons[k][0], cons[k][1], cons[k][2]) for k in range(len(kinds)) if kinds[k] == 3 and cons[k] is not None}


def cold_steps(d, lam, kinds):
    """per kind-3 node: dict(steps, active, drops) of the cold solve at lam: the steps the device takes from the equalities, the
    members of the final working set that are no equalities, and the members gen_ref.solve_gen dropped on its way"""
    out = {}
    for k, qp in node_qps(d, lam, kinds).items():
        G.STATS["drops"] = 0
        G.solve_gen(*qp)
        drops = G.STATS["drops"]
        r = solve_gen_from(*qp)
        _, _, lo, hi, _, dlo, dhi = qp
        active = int(np.sum((r["sb"] != 0) & (lo < hi))) + int(np.sum((r["sr"] != 0) & (dlo < dhi)))
        out[k] = dict(steps=r["steps"], active=active, drops=drops)
    return out

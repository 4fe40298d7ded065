"""One dual Newton step of the tree QP, built densely in numpy (no code shared with the oracle or the device path).

Conventions, as dual_Newton_tree.c has them:
- The stage QP of node p (solve_stage_problems) minimises 1/2 z'H_p z - h_p'z, with z = [x_p | u_p] and
      h_p = [lambda_p - q_p - sum_k A_k' lambda_k | -r_p - sum_k B_k' lambda_k],
  the sums over the children k of p, and lambda_0 = 0 for the root.  Clipping nodes (kind 0) take z = clip(H_p^-1 h_p) with H_p
  diagonal; dense unconstrained nodes (kind 1) take z = H_p^-1 h_p; box nodes (kind 2) take the solution of the stage QP subject
  to lo <= z <= hi with H_p full.
- The dual gradient is the dynamics residual (build_dual_problem): res_k = A_k x_p + B_k u_p + b_k - x_k.
- The dual Hessian, negated, is M = G P G' (the W and Ut blocks: C_k P_p C_j' for siblings k and j, E P_k E' on the diagonal,
  -C_k P_p E' between an edge and the edge into its parent).  G has the row block [A_k B_k] on the parent's columns and -I on
  the child's x.  P is block diagonal: 1 / diag(H_p) on the free entries of a clipping node and 0 on its clipped ones, H_p^-1 on a
  dense node, inv(H_FF) on the free set F of a box node and 0 elsewhere.
- The step solves M dlam = res (calculate_delta_lambda), and the line search takes lambda + tau dlam with tau = beta^(trials - 1).
- The dual function as the solver minimises it (evaluate_dual_function) is the sum over the nodes of
      -1/2 z'H_p z + h_p'z - sum_k b_k'lambda_k,
  and a trial is accepted when f(lambda + tau dlam) <= f(lambda) + gamma tau dot with dot = -res'dlam (line_search).

Products and residuals are in np.longdouble.  Linear systems are solved in float64 and refined once with a longdouble residual.

The box QP is solved by a textbook primal active-set method on the bounds, written here for itself.  Its answer does not rest on
that method: the strictly convex QP has one solution, and `certify_box` checks in longdouble that the returned z is that solution
(feasible; g = Hz - h zero on the free entries, >= 0 on a lower bound and <= 0 on an upper one)."""
from __future__ import annotations

import numpy as np

from treeqp_amd import problems as P

LD = np.longdouble


def _blocks(d, dense):
    nk, nx, nu = [np.asarray(d[k], dtype=int) for k in ("nk", "nx", "nu")]
    Nn = len(nk)
    xo = np.concatenate([[0], np.cumsum(nx)])
    uo = np.concatenate([[0], np.cumsum(nu)])
    dad = P.parents_of(nk)
    A, B, b = {}, {}, {}
    ao = bo = lo = 0
    for k in range(1, Nn):
        p = dad[k]
        A[k] = np.asarray(d["A"][ao:ao + nx[k] * nx[p]], dtype=LD).reshape((nx[k], nx[p]), order="F"); ao += nx[k] * nx[p]
        B[k] = np.asarray(d["B"][bo:bo + nx[k] * nu[p]], dtype=LD).reshape((nx[k], nu[p]), order="F"); bo += nx[k] * nu[p]
        b[k] = np.asarray(d["b"][lo:lo + nx[k]], dtype=LD); lo += nx[k]
    H = []
    if dense:
        qo = ro = so = 0
        for k in range(Nn):
            a, m = nx[k], nu[k]
            Hk = np.zeros((a + m, a + m))
            Hk[:a, :a] = np.reshape(d["Q"][qo:qo + a * a], (a, a), order="F"); qo += a * a
            Hk[a:, a:] = np.reshape(d["R"][ro:ro + m * m], (m, m), order="F"); ro += m * m
            S = np.reshape(d["S"][so:so + m * a], (m, a), order="F"); so += m * a
            Hk[a:, :a] = S; Hk[:a, a:] = S.T
            H.append(Hk)
    else:
        for k in range(Nn):
            H.append(np.concatenate([d["Qd"][xo[k]:xo[k + 1]], d["Rd"][uo[k]:uo[k + 1]]]).astype(np.float64))
    return nk, nx, nu, xo, uo, dad, A, B, b, H


def _kinds_of(d, dense, kinds):
    Nn = len(d["nk"])
    if kinds is None:
        return np.full(Nn, 1 if dense else 0, dtype=int), dense
    kinds = np.asarray(kinds, dtype=int)
    assert kinds.shape == (Nn,) and np.all((kinds >= 0) & (kinds <= 2))
    return kinds, True               # per-node kinds: H_k from the dense blocks Q, R, S (a clipping node takes their diagonal)


def _refined_solve(Hm, rhs):
    """Hm z = rhs: float64 solve, one refinement against the longdouble residual"""
    z = np.linalg.solve(Hm, np.asarray(rhs, dtype=np.float64)).astype(LD)
    return z + np.linalg.solve(Hm, (rhs - Hm.astype(LD) @ z).astype(np.float64)).astype(LD)


def solve_box(Hk, h, lo, hi):
    """argmin 1/2 z'Hz - h'z, lo <= z <= hi (H positive definite; lo, hi may be IEEE infinities) -> (z, side): side[i] is -1 on
    the lower bound, +1 on the upper bound, 0 for a free entry; entries with lo == hi are fixed (side -1).  Primal active-set
    method on the bounds from the projected unconstrained solution; z of the final working set is refined in longdouble, its
    fixed entries are the bounds themselves."""
    n = len(h)
    h = np.asarray(h, dtype=LD); lo = np.asarray(lo, dtype=LD); hi = np.asarray(hi, dtype=LD)
    if n == 0:
        return np.zeros(0, dtype=LD), np.zeros(0, dtype=int)
    H64 = np.asarray(Hk, dtype=np.float64)
    HL = H64.astype(LD)

    def eqp(z, side):
        """the minimiser with the entries of the working set held where z has them"""
        F = side == 0
        out = z.copy()
        if np.any(F):
            out[F] = _refined_solve(H64[np.ix_(F, F)], h[F] - HL[np.ix_(F, ~F)] @ z[~F])
        return out

    z = np.minimum(np.maximum(_refined_solve(H64, h), lo), hi)
    side = np.where(z <= lo, -1, np.where(z >= hi, 1, 0))
    side[lo == hi] = -1
    for _ in range(20 * n + 20):
        zn = eqp(z, side)
        F = side == 0
        out = F & ((zn < lo) | (zn > hi))
        if np.any(out):
            # step to the first bound the segment z -> zn meets; every entry that meets it there joins the working set
            tgt = np.where(zn < lo, lo, hi)
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.where(out, np.where(zn == z, LD(0), (tgt - z) / (zn - z)), LD(np.inf))
            amin = max(LD(0), min(LD(1), a.min()))
            hit = out & (a <= amin)
            z = np.where(F, z + amin * (zn - z), z)
            z = np.minimum(np.maximum(z, lo), hi)
            z[hit] = tgt[hit]
            side[hit] = np.where(zn[hit] < lo[hit], -1, 1)
            continue
        z = zn
        g = HL @ z - h
        wrong = (lo < hi) & (((side == -1) & (g < 0)) | ((side == 1) & (g > 0)))
        if not np.any(wrong):
            # a free solution exactly on a bound counts as fixed there (the inclusive rule of clipping)
            side = np.where(F & (z <= lo), -1, np.where(F & (z >= hi), 1, side))
            return z, side
        side[int(np.argmax(np.where(wrong, np.abs(g), LD(-1))))] = 0
    raise AssertionError("the active-set method of the reference did not finish")


CERT_TOL = 1e-13      # of (|H||z| + |h|)_i: a float64 solve refined once leaves a longdouble residual some 1e-3 of that


def certify_box(Hk, h, lo, hi, z, side):
    """The optimality conditions of the box QP at (z, side), in longdouble.  Returns (violation, margin): violation is the largest
    of the feasibility, stationarity and sign defects, each relative to (|H||z| + |h|)_i (<= CERT_TOL for a certified answer);
    margin is the smallest, over the entries whose bounds differ, of the distance of a free entry to either bound and |g_i| of a
    fixed entry."""
    if len(z) == 0:
        return 0.0, np.inf
    HL = np.asarray(Hk, dtype=LD)
    h = np.asarray(h, dtype=LD); lo = np.asarray(lo, dtype=LD); hi = np.asarray(hi, dtype=LD)
    g = HL @ z - h
    scale = np.abs(HL) @ np.abs(z) + np.abs(h) + LD(1e-300)
    free = side == 0
    viol = max(float(np.max(np.maximum(lo - z, 0))), float(np.max(np.maximum(z - hi, 0))))        # fixed entries ARE the bound
    assert np.all(z[side == -1] == lo[side == -1]) and np.all(z[side == 1] == hi[side == 1])
    open_ = lo < hi
    defect = np.where(free, np.abs(g), np.where(~open_, LD(0), np.where(side == -1, np.maximum(-g, 0), np.maximum(g, 0))))
    viol = max(viol, float(np.max(defect / scale)))
    with np.errstate(invalid="ignore"):
        dist = np.where(free, np.minimum(z - lo, hi - z), np.abs(g))
    margin = float(np.min(dist[open_])) if np.any(open_) else np.inf
    return viol, margin


def stage_data(d, lam, dense=False, kinds=None):
    """Per node: H_k (float64; a vector of weights on a clipping node), h_k at lam (longdouble), lo, hi (longdouble).
    Returns (tree, H, h, lo, hi) with tree = (nk, nx, nu, xo, uo, dad, A, B, b, kids, lam_off, kinds)."""
    kinds, dense_blocks = _kinds_of(d, dense, kinds)
    nk, nx, nu, xo, uo, dad, A, B, b, H = _blocks(d, dense_blocks)
    Nn = len(nk)
    lo_ = xo - nx[0]                                   # offset of lambda_k in the flat dual vector (k >= 1)
    lam = np.asarray(lam, dtype=LD)
    kids = [[] for _ in range(Nn)]
    for k in range(1, Nn):
        kids[dad[k]].append(k)
    hs, los, his = [], [], []
    for p in range(Nn):
        a = nx[p]
        if dense_blocks and kinds[p] == 0:
            H[p] = np.diag(H[p]).copy()
        hx = -np.asarray(d["q"][xo[p]:xo[p + 1]], dtype=LD)
        if p > 0:
            hx = hx + lam[lo_[p]:lo_[p] + a]
        hu = -np.asarray(d["r"][uo[p]:uo[p + 1]], dtype=LD)
        for k in kids[p]:
            lk = lam[lo_[k]:lo_[k] + nx[k]]
            hx = hx - A[k].T @ lk
            hu = hu - B[k].T @ lk
        hs.append(np.concatenate([hx, hu]))
        if kinds[p] == 1:
            los.append(np.full(a + nu[p], -np.inf, dtype=LD)); his.append(np.full(a + nu[p], np.inf, dtype=LD))
        else:
            los.append(np.concatenate([d["xmin"][xo[p]:xo[p + 1]], d["umin"][uo[p]:uo[p + 1]]]).astype(LD))
            his.append(np.concatenate([d["xmax"][xo[p]:xo[p + 1]], d["umax"][uo[p]:uo[p + 1]]]).astype(LD))
    return (nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, kinds), H, hs, los, his


def stage_solutions(d, lam, dense=False, kinds=None, inclusive=True):
    """The stage QPs at lam.  Returns dict(z, side, P, margin, cert, tree, H, h): per node the solution (longdouble), the bound each
    entry sits on (-1, 0, +1; all 0 on a dense unconstrained node), the elimination matrix; margin as newton_step documents it;
    cert the largest violation certify_box found on a box node.  inclusive: the rule of the clipping nodes.  True is the solver's
    (a value exactly on a bound is fixed there, P_ii = 0); False is the WRONG rule `>` / `<` (such an entry stays free, same
    z), kept for the tests that show a tie moves the step; a list with one boolean array per node over its [x | u] applies the
    wrong rule to the entries that are False there and the solver's to the others."""
    tree, H, hs, los, his = stage_data(d, lam, dense, kinds)
    kinds = tree[-1]
    z, side, Pm = [], [], []
    margin, cert = np.inf, 0.0
    for p in range(len(H)):
        h, lo, hi = hs[p], los[p], his[p]
        n = len(h)
        if kinds[p] == 1:
            Hk = H[p]
            zk = _refined_solve(Hk, h) if n else np.zeros(0, dtype=LD)
            sk = np.zeros(n, dtype=int)
            Pk = np.linalg.inv(Hk).astype(LD) if n else np.zeros((0, 0), dtype=LD)
        elif kinds[p] == 0:
            w = H[p].astype(LD)
            zu = h / w
            free = (zu > lo) & (zu < hi)
            if inclusive is not True:
                wrong = np.ones(n, dtype=bool) if inclusive is False else ~np.asarray(inclusive[p], dtype=bool)
                free = free | (wrong & ((zu == lo) | (zu == hi)))
            zk = np.minimum(np.maximum(zu, lo), hi)
            sk = np.where(free, 0, np.where(zu <= lo, -1, 1))
            open_ = lo < hi
            if np.any(open_):
                margin = min(margin, float(np.min(np.minimum(np.abs(zu - lo), np.abs(zu - hi))[open_])))
            Pk = np.diag(np.where(free, 1 / w, LD(0)))
        else:
            Hk = H[p]
            zk, sk = solve_box(Hk, h, lo, hi)
            v, mg = certify_box(Hk, h, lo, hi, zk, sk)
            assert v <= CERT_TOL, f"node {p}: the reference's own box solution misses its certificate ({v:.2e})"
            cert = max(cert, v)
            margin = min(margin, mg)
            F = sk == 0
            Pk = np.zeros((n, n), dtype=LD)
            if np.any(F):
                Pk[np.ix_(F, F)] = np.linalg.inv(Hk[np.ix_(F, F)]).astype(LD)
        z.append(zk); side.append(sk); Pm.append(Pk)
    return dict(z=z, side=side, P=Pm, margin=margin, cert=cert, tree=tree, H=H, h=hs)


def flat_xu(st):
    """x, u (float64, flat, node after node) of stage_solutions' z, and the flat `side` arrays to go with them"""
    nx = st["tree"][1]
    x = np.concatenate([zk[:nx[k]] for k, zk in enumerate(st["z"])]).astype(np.float64)
    u = np.concatenate([zk[nx[k]:] for k, zk in enumerate(st["z"])]).astype(np.float64)
    sx = np.concatenate([sk[:nx[k]] for k, sk in enumerate(st["side"])])
    su = np.concatenate([sk[nx[k]:] for k, sk in enumerate(st["side"])])
    return x, u, sx, su


def assemble_from(st):
    """(M, res) of assemble from stage solutions st (stage_solutions' here, or gen_ref's)"""
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
        Ck = np.hstack([A[k], B[k]])
        CP = Ck @ Pm[p]
        for j in kids[p]:
            M[ik, lo_[j]:lo_[j] + nx[j]] += CP @ np.hstack([A[j], B[j]]).T
        M[ik, ik] += Pm[k][:nx[k], :nx[k]]
        if p > 0:
            ip = slice(lo_[p], lo_[p] + nx[p])
            blk = -CP[:, :nx[p]]
            M[ik, ip] += blk
            M[ip, ik] += blk.T
    return M, res


def assemble(d, lam0, dense=False, kinds=None, inclusive=True):
    """The Newton system at lam0, in longdouble: (M, res, stages) with M = G P G' the negated dual Hessian, res the dynamics
    residual and stages what stage_solutions returns (its "tree" holds the offsets of the duals)."""
    st = stage_solutions(d, lam0, dense, kinds, inclusive)
    return assemble_from(st) + (st,)


def newton_step(d, lam0, dense=False, kinds=None, reg=0.0, inclusive=True):
    """The step of the dual Newton method at lam0 (concatenation of lambda_1 .. lambda_{Nn-1}).  kinds: per-node stage solver (0
    clipping on the diagonals of Q, R; 1 dense unconstrained; 2 dense with box bounds), H_k then from the blocks Q, R, S; None:
    all clipping on Qd, Rd (dense=False) or all dense unconstrained (dense=True).  Returns dict(dlam, res, cond, margin, cert,
    stages): margin is the smallest, over the entries whose bounds differ, of the distance of an unclipped stage value to a
    clipping threshold (clipping nodes), of the distance of a free entry to either bound and of |g_i| of a fixed entry (box
    nodes); inf on dense unconstrained trees.  stages is what stage_solutions returns.  reg > 0 adds reg I to M (the solver's
    regType = 1); the device pins of the unregularised step use reg = 0 (reg_ref.py has the block-wise regularisation).
    inclusive: see stage_solutions (True everywhere but in the tests of the clipping rule itself)."""
    M, res, st = assemble(d, lam0, dense, kinds, inclusive)
    n = len(res)
    if reg:
        M = M + LD(reg) * np.eye(n, dtype=LD)
    M64 = M.astype(np.float64)
    dl = np.linalg.solve(M64, res.astype(np.float64)).astype(LD)
    dl = dl + np.linalg.solve(M64, (res - M @ dl).astype(np.float64)).astype(LD)
    return dict(dlam=dl.astype(np.float64), res=res.astype(np.float64), cond=float(np.linalg.cond(M64)), margin=st["margin"],
                cert=st["cert"], stages=st)


def seeded_duals(n, s, scale=0.1):
    """the s-th candidate lambda0 of starting_duals"""
    return scale * np.random.Generator(np.random.PCG64(1000 + s)).standard_normal(n)


def starting_duals(d, dense=False, tries=20, gap=1e-6, kinds=None):
    """A seeded lambda0 of scale 0.1 that leaves every stage value at least `gap` away from its clipping thresholds (the step is
    then a smooth function of the data); the first of `tries` seeds that does, with its step."""
    n = int(np.asarray(d["nx"])[1:].sum())
    for s in range(tries):
        lam0 = seeded_duals(n, s)
        ref = newton_step(d, lam0, dense, kinds)
        if ref["margin"] > gap:
            return lam0, ref
    raise AssertionError(f"no lambda0 of {tries} seeds keeps the stage values {gap} away from the clipping thresholds")


def abs_h(st, lam, p):
    """T_h of node p: the sum of the absolute values of the terms of h = [lam_p - q - sum A'lam | -r - sum B'lam]"""
    nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, kd = st["tree"]
    lam = np.asarray(lam, dtype=LD)
    h = st["h"][p]
    Th, own = np.zeros(len(h), dtype=LD), h.copy()
    if p > 0:
        lp = lam[lo_[p]:lo_[p] + nx[p]]
        Th[:nx[p]] += np.abs(lp)
        own[:nx[p]] -= lp
    for k in kids[p]:
        l = lam[lo_[k]:lo_[k] + nx[k]]
        Th += np.concatenate([np.abs(A[k]).T @ np.abs(l), np.abs(B[k]).T @ np.abs(l)])
        own = own + np.concatenate([A[k].T @ l, B[k].T @ l])
    return Th + np.abs(own)                                # (own: -q, -r, what h holds beside the duals)


def terms_of_stages(st, lam):
    """The nodes' terms of the dual function from stage solutions st at lam (what stage_solutions, here or in gen_ref, returns):
    (terms, scales), both per node in longdouble.  terms[p] = -1/2 z'H z + h'z - sum_children b_k'lambda_k; scales[p] is the sum of
    the absolute values of every product inside it, with the sums that make up h taken apart as well:
    1/2 |z|'|H||z| + T_h'|z| + sum_children |b_k|'|lambda_k|, T_h = |lambda_p| + |q| + sum_children |A_k|'|lambda_k| (and |r|,
    |B_k|'|lambda_k| on the inputs)."""
    nk, nx, nu, xo, uo, dad, A, B, b, kids, lo_, kd = st["tree"]
    lam = np.asarray(lam, dtype=LD)
    out, scale = np.zeros(len(nk), dtype=LD), np.zeros(len(nk), dtype=LD)
    for p, (zk, h) in enumerate(zip(st["z"], st["h"])):
        Hp = st["H"][p].astype(LD)
        Hz, aHz = (Hp * zk, np.abs(Hp) * np.abs(zk)) if Hp.ndim == 1 else (Hp @ zk, np.abs(Hp) @ np.abs(zk))
        lk = [lam[lo_[k]:lo_[k] + nx[k]] for k in kids[p]]
        out[p] = -LD(0.5) * (zk @ Hz) + h @ zk - sum((b[k] @ l for k, l in zip(kids[p], lk)), LD(0))
        Th = abs_h(st, lam, p)
        scale[p] = LD(0.5) * (np.abs(zk) @ aHz) + Th @ np.abs(zk) + sum((np.abs(b[k]) @ np.abs(l) for k, l in zip(kids[p], lk)), LD(0))
    return out, scale


def dual_terms(d, lam, kinds=None, dense=False):
    """The nodes' terms of the dual function at lam, as the kernels take them: -1/2 z'H z + h'z - sum_children b_k'lambda_k, in
    longdouble."""
    return terms_of_stages(stage_solutions(d, lam, dense, kinds), lam)[0]


def dual_value(d, lam, kinds=None, dense=False):
    """The dual function at lam as the solver minimises it (the sum of dual_terms), in longdouble."""
    return dual_terms(d, lam, kinds, dense).sum()


def armijo_trials(d, lam0, dlam, res, opts, kinds=None, dense=False):
    """Trials of the backtracking line search from lam0 along dlam: tau = 1, beta, beta^2, ..., the first with
    f(lam0 + tau dlam) <= f(lam0) + gamma tau dot, dot = -res'dlam; lineSearchMaxIter + 1 when none is accepted (the counter the
    loop of line_search leaves behind).  The restart rule (lineSearchRestartTrigger) never fires in a first iteration and is left
    out.  Returns (trials, slack): slack is the smallest |f - (f0 + gamma tau dot)| of the decisions made, relative to the sum
    of the absolute node terms of f and f0 (what a float64 sum of those terms is uncertain by, times 2^-53)."""
    gamma, beta, cap = opts.lineSearchGamma, opts.lineSearchBeta, opts.lineSearchMaxIter
    lam0 = np.asarray(lam0, dtype=LD); dl = np.asarray(dlam, dtype=LD)
    t0 = dual_terms(d, lam0, kinds, dense)
    f0 = t0.sum()
    dot = -(np.asarray(res, dtype=LD) @ dl)
    tau, slack = LD(1), np.inf
    for trial in range(1, cap + 1):
        t = dual_terms(d, lam0 + tau * dl, kinds, dense)
        f, bound = t.sum(), f0 + LD(gamma) * tau * dot
        slack = min(slack, float(abs(f - bound) / (np.abs(t).sum() + np.abs(t0).sum())))
        if f <= bound:
            return trial, slack
        tau = LD(beta) * tau
    return cap + 1, slack

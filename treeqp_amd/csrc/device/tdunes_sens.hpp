/*
 * tdunes_sens.hpp -- parametric sensitivities of an MPC step: d(x, u, lam) / d x0 at the point of the last solve, active set frozen.
 *
 * Included by tdunes_device.hip (host side: tdunes_adjoint.hpp); the kernels are written after hess_body, factor_body and forward_body (same tall Cholesky, same
 * substitutions, same WSYNC discipline), with nx0 right-hand sides instead of one.  One wave per unit on a private LDS window, one
 * launch per phase and block level; no kernel waits for another workgroup: the launch boundaries on the mirror's stream order them.
 *
 *   M dLam = G,   M = the dual Hessian hess_body builds (W_p, Ut_p) with the elimination matrices P_k of the exported point,
 *                 G = d res / d x0 at fixed lam: rows of the root's children only,
 *                     eliminated root:  G_c = A0_c - B_c P_0 S0 (second term where S0 was given);   root with states:  G_c = A_c
 *   dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) + direct_k,   direct_0 = -P_0 [0; S0] (eliminated root), [I; 0] (root with states)
 *   K = the u rows of dZ_0.
 *
 * P_k: kind 0 diagonal, 1 / Qd_i (1 / Rd_i) where the exported value is strictly inside its bounds, 0.0 where it equals a bound bit for
 * bit (clipping assigns the bound itself), phantom root states free; kind 1: Data::Pd.  Everything is written into the feature's own
 * buffers (struct Sens); Data is only read.
 *
 * The adjoint of a step (k_adj_rhs, k_adj_backward, k_adj_forward, k_adj_grad; struct Adj) is the reverse: one more solve with the same
 * factor, one right-hand side per column of w = dL/dz, non-zero in every block; its formulas stand with its kernels below.  The batch
 * forms at the end (struct AItem, k_*_batch) are the same bodies behind a look-up of the member.  The tangent of a step (k_tan_rhs,
 * k_tan_primal, k_tan_apply; struct Tan, last in this file) is the forward-mode twin of the adjoint: its own right-hand side and read-out
 * around the adjoint's two sweeps.
 */
#pragma once

struct Sens {
    const double *x, *u;               /* the export block: x (phantom root states excluded), u */
    double *W, *Ut, *CholW, *CholUt;   /* as Data::W .. of the solver, laid out by Tree::woff / utoff */
    double *invd;                      /* reciprocal pivots, node-indexed as Data::invd */
    double *Px, *Pu;                   /* the diagonal P of kind-0 nodes, node-indexed as Data::x / Data::u */
    double *G;                         /* bdim[0] x nx0, column major */
    double *dlam, *dx, *du;            /* sum_nx x nx0, sum_nx x nx0, sum_nu x nx0, column major, node-indexed (phantom root states included) */
    double *head;                      /* [K (nu0 x nx0, column major) | u0 (nu0) | x0_ref (nx0) | n_reg] */
    int *n_reg;
    const double *A0, *S0;             /* the originals of an eliminated root (S0: nullptr = zero) */
    const double *x0;                  /* pinned: the x0 last folded (eliminated root) */
    int nx0, xpad, root_states, sum_nx, sum_nu, nu0;
};

__device__ __forceinline__ int sens_kind(const Data &D, int k) { return D.dense ? D.kind[k] : 0; }
/* entry i of the diagonal P of kind-0 node k, i over [x | u] */
__device__ __forceinline__ double sens_pdiag(const Tree &T, const Data &D, const Sens &S, int k, int i) {
    const int nx = T.nx[k], pad = k == 0 ? S.xpad : 0;
    if (i < nx) {
        const int g = T.xoff[k] + i;
        if (i < pad) return 1.0 / D.Qd[g];
        const double v = S.x[g - S.xpad];
        return (v == D.xmin[g] || v == D.xmax[g]) ? 0.0 : 1.0 / D.Qd[g];
    }
    const int g = T.uoff[k] + i - nx;
    const double v = S.u[g];
    return (v == D.umin[g] || v == D.umax[g]) ? 0.0 : 1.0 / D.Rd[g];
}

/* ---- k_sens_hess: one wave per parent block p: W_p, Ut_p as hess_body builds them, the diagonal P of p's kind-0 children (and of the
 * root), and from the root's block G ---- */
__device__ void sens_hess_body(const Tree &T, const Data &D, const Sens &S, int p, int lane, double *lds) {
    const int d = T.bdim[p], nxp = T.nx[p], nup = T.nu[p], nz = nxp + nup;
    double *Cs = lds;                 /* d x nz, column major, ld = d */
    double *CP = lds + (size_t)d * nz;
    const int k0 = T.kid0[p];
    const bool pdense = sens_kind(D, p) != 0;
    if (p == 0 && lane == 0) *S.n_reg = 0;
    /* the diagonal P of the kind-0 nodes this block owns: its children, and the root itself */
    for (int cc = (p == 0 ? -1 : 0); cc < T.nk[p]; cc++) {
        const int k = cc < 0 ? 0 : k0 + cc;
        if (sens_kind(D, k)) continue;
        const int nxk = T.nx[k], nzk = nxk + T.nu[k];
        for (int i = lane; i < nzk; i += WAVE) {
            const double pv = sens_pdiag(T, D, S, k, i);
            if (i < nxk) S.Px[T.xoff[k] + i] = pv; else S.Pu[T.uoff[k] + i - nxk] = pv;
        }
    }
    /* stage the children's [A B] rows */
    int rowoff = 0;
    for (int cc = 0; cc < T.nk[p]; cc++) {
        const int kid = k0 + cc, nxc = T.nx[kid];
        const double *A = D.A + T.aoff[kid], *B = D.B + T.boff[kid];
        for (int e = lane; e < nxc * nz; e += WAVE) {
            const int i = e % nxc, col = e / nxc;
            const double a = col < nxp ? A[i + (size_t)col * nxc] : B[i + (size_t)(col - nxp) * nxc];
            Cs[rowoff + i + (size_t)col * d] = a;
            if (!pdense) CP[rowoff + i + (size_t)col * d] = a * sens_pdiag(T, D, S, p, col);
        }
        rowoff += nxc;
    }
    WSYNC();
    if (pdense) {
        const double *P = D.Pd + D.poff[p];
        for (int e = lane; e < d * nz; e += WAVE) {
            const int i = e % d, col = e / d;
            double acc = 0.0;
            for (int cidx = 0; cidx < nz; cidx++) acc = fma(Cs[i + (size_t)cidx * d], P[cidx + (size_t)col * nz], acc);
            CP[i + (size_t)col * d] = acc;
        }
        WSYNC();
    }
    double *W = S.W + T.woff[p];
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i < j) continue;
        double acc = 0.0, acc2 = 0.0;
        for (int cidx = 0; cidx < nxp; cidx++) acc = fma(Cs[i + (size_t)cidx * d], CP[j + (size_t)cidx * d], acc);
        for (int cidx = nxp; cidx < nz; cidx++) acc2 = fma(Cs[i + (size_t)cidx * d], CP[j + (size_t)cidx * d], acc2);
        double w = acc + acc2;
        /* the state block of the child's own elimination matrix on the diagonal block */
        int ro = 0;
        for (int cc = 0; cc < T.nk[p]; cc++) {
            const int kid = k0 + cc, nxc = T.nx[kid];
            if (i >= ro && i < ro + nxc && j >= ro && j < ro + nxc) {
                if (sens_kind(D, kid)) { const int nzk = nxc + T.nu[kid]; w += D.Pd[D.poff[kid] + (i - ro) + (size_t)(j - ro) * nzk]; }
                else if (i == j) w += sens_pdiag(T, D, S, kid, i - ro);
            }
            ro += nxc;
        }
        W[i + (size_t)j * d] = w;
    }
    if (p > 0) {
        double *Ut = S.Ut + T.utoff[p];
        for (int e = lane; e < nxp * d; e += WAVE) {
            const int i = e % nxp, rr = e / nxp;
            Ut[i + (size_t)rr * nxp] = -1.0 * CP[rr + (size_t)i * d];
        }
    } else {
        /* G: A0 - (C P_0)[:, u] S0 for an eliminated root, the state columns of C for a root that keeps its states */
        const int nx0 = S.nx0;
        for (int e = lane; e < d * nx0; e += WAVE) {
            const int i = e % d, j = e / d;
            double g;
            if (S.root_states) g = Cs[i + (size_t)(S.xpad + j) * d];
            else {
                /* A0 lies child after child, each nx[kid] x nx0: find row i's child */
                int ro = 0, ao = 0, kid = k0;
                for (; kid < k0 + T.nk[0]; kid++) { const int n = T.nx[kid]; if (i < ro + n) break; ro += n; ao += n * nx0; }
                const int nxc = T.nx[kid];
                g = S.A0[ao + (i - ro) + (size_t)j * nxc];
                if (S.S0) {
                    double acc = 0.0;
                    for (int m = 0; m < nup; m++) acc = fma(CP[i + (size_t)(nxp + m) * d], S.S0[m + (size_t)j * nup], acc);
                    g -= acc;
                }
            }
            S.G[i + (size_t)j * d] = g;
        }
    }
}

/* ---- k_sens_factor: one wave per block of one level, deepest level first: tall Cholesky of [W; Ut] with factor_body's regularisation,
 * the Schur complement into the parent's W through global memory; the root carries G' as nx0 extra rows: Y = (L^-1 G)', dLam_0 = L^-T Y ---- */
__device__ void sens_factor_body(const Tree &T, const Opts &O, const Sens &S, int ii, int lane, double *lds) {
    const int d = T.bdim[ii], nxi = ii > 0 ? T.nx[ii] : S.nx0;
    const int R = d + nxi, ld = R | 1;
    double *Tm = lds;                         /* ld x d */
    double *invd = lds + (size_t)ld * d;      /* d */
    const double *W = S.W + T.woff[ii];
    const int bo = T.xoff[T.kid0[ii]];
    const double *Ut = S.Ut + T.utoff[ii];

    for (int pass = 0; pass < 2; pass++) {
        for (int e = lane; e < d * d; e += WAVE) {
            const int i = e % d, j = e / d;
            double w = W[i + (size_t)j * d];
            if (i == j && (O.regType == 1 || pass == 1)) w += O.regValue;
            Tm[i + (size_t)j * ld] = w;
        }
        for (int e = lane; e < nxi * d; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            Tm[d + i + (size_t)j * ld] = ii > 0 ? Ut[i + (size_t)j * nxi] : S.G[j + (size_t)i * d];
        }
        WSYNC();
        tall_potrf(Tm, invd, R, d, ld, lane);
        if (O.regType != 2 || pass == 1) break;
        int small = 0;
        for (int j = lane; j < d; j += WAVE) small |= (Tm[j + (size_t)j * ld] <= O.regTol);
        if (!__any(small)) break;
        if (lane == 0) atomicAdd(S.n_reg, 1);
        WSYNC();
    }
    double *L = S.CholW + T.woff[ii];
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * d] = Tm[i + (size_t)j * ld];
    }
    for (int j = lane; j < d; j += WAVE) S.invd[bo + j] = invd[j];
    if (ii > 0) {
        double *CUt = S.CholUt + T.utoff[ii];
        for (int e = lane; e < nxi * d; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            CUt[i + (size_t)j * nxi] = Tm[d + i + (size_t)j * ld];
        }
        const int dd = T.dad[ii], pos = T.pos[ii], ddim = T.bdim[dd];
        double *Wd = S.W + T.woff[dd];
        for (int e = lane; e < nxi * nxi; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            if (i < j) continue;
            double acc = 0.0;
            for (int cidx = 0; cidx < d; cidx++) acc = fma(Tm[d + i + (size_t)cidx * ld], Tm[d + j + (size_t)cidx * ld], acc);
            Wd[(pos + i) + (size_t)(pos + j) * ddim] -= acc;
        }
    } else {
        /* all nx0 right-hand sides at once: column-oriented back substitution, k descending, (row, column) pairs over the lanes */
        for (int k = d - 1; k >= 0; k--) {
            WSYNC();
            const double ivk = invd[k];
            for (int e = lane; e < k * nxi; e += WAVE) {
                const int i = e % k, j = e / k;
                const double zk = Tm[d + j + (size_t)k * ld] * ivk;
                Tm[d + j + (size_t)i * ld] = fma(-Tm[k + (size_t)i * ld], zk, Tm[d + j + (size_t)i * ld]);
            }
            WSYNC();
            for (int j = lane; j < nxi; j += WAVE) Tm[d + j + (size_t)k * ld] *= ivk;
        }
        WSYNC();
        for (int e = lane; e < d * nxi; e += WAVE) {
            const int i = e % d, j = e / d;
            S.dlam[bo + i + (size_t)j * S.sum_nx] = Tm[d + j + (size_t)i * ld];
        }
    }
}

/* ---- k_sens_forward: one wave per (block of one level, column j): dLam_ii = -L^-T CholUt' dLam_dad[pos ..], forward_body's substitution ---- */
__device__ void sens_forward_body(const Tree &T, const Sens &S, int ii, int col, int lane, double *lds) {
    const int d = T.bdim[ii], nxi = T.nx[ii], ld = d | 1;
    double *L = lds;                      /* ld x d */
    double *z = lds + (size_t)ld * d;     /* d */
    double *dl = z + d;                   /* nxi */
    double *iv = dl + nxi;                /* d */
    const int bo = T.xoff[T.kid0[ii]], xo = T.xoff[ii];
    const double *Lg = S.CholW + T.woff[ii];
    double *dlam = S.dlam + (size_t)col * S.sum_nx;
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * ld] = Lg[i + (size_t)j * d];
    }
    for (int j = lane; j < d; j += WAVE) iv[j] = S.invd[bo + j];
    for (int i = lane; i < nxi; i += WAVE) dl[i] = dlam[xo + i];
    WSYNC();
    const double *CUt = S.CholUt + T.utoff[ii];
    for (int j = lane; j < d; j += WAVE) {
        double acc = 0.0;
        for (int i = 0; i < nxi; i++) acc = fma(CUt[i + (size_t)j * nxi], dl[i], acc);
        z[j] = -acc;
    }
    for (int k = d - 1; k >= 0; k--) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = lane; i < k; i += WAVE) z[i] = fma(-L[k + (size_t)i * ld], zk, z[i]);
        WSYNC();
        if (lane == 0) z[k] = zk;
    }
    WSYNC();
    for (int j = lane; j < d; j += WAVE) dlam[bo + j] = z[j];
}

/* ---- k_sens_primal: one wave per node: dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) + direct_k; node 0 also fills the head ---- */
__device__ void sens_primal_body(const Tree &T, const Data &D, const Sens &S, int k, int lane, double *lds) {
    const int nxk = T.nx[k], nuk = T.nu[k], nz = nxk + nuk, nx0 = S.nx0, pad = k == 0 ? S.xpad : 0;
    const int xo = T.xoff[k], uo = T.uoff[k], k0 = T.kid0[k], nkids = k < T.Np ? T.nk[k] : 0;
    double *v = lds;                      /* nz x nx0 */
    for (int e = lane; e < nz * nx0; e += WAVE) {
        const int i = e % nz, j = e / nz;
        const double *dl = S.dlam + (size_t)j * S.sum_nx;
        double acc = 0.0;
        for (int cc = 0; cc < nkids; cc++) {
            const int kid = k0 + cc, nxc = T.nx[kid];
            const double *Cc = i < nxk ? D.A + T.aoff[kid] + (size_t)i * nxc : D.B + T.boff[kid] + (size_t)(i - nxk) * nxc;
            const double *dc = dl + T.xoff[kid];
            for (int r = 0; r < nxc; r++) acc = fma(Cc[r], dc[r], acc);
        }
        double w = (k > 0 && i < nxk ? dl[xo + i] : 0.0) - acc;
        if (k == 0 && !S.root_states && S.S0 && i >= nxk) w -= S.S0[(i - nxk) + (size_t)j * nuk];
        v[e] = w;
    }
    WSYNC();
    const int kind = sens_kind(D, k);
    for (int e = lane; e < nz * nx0; e += WAVE) {
        const int i = e % nz, j = e / nz;
        double r;
        if (kind == 0) r = (i < nxk ? S.Px[xo + i] : S.Pu[uo + i - nxk]) * v[e];
        else {
            const double *P = D.Pd + D.poff[k];
            r = 0.0;
            for (int m = 0; m < nz; m++) r = fma(P[i + (size_t)m * nz], v[m + (size_t)j * nz], r);
        }
        if (k == 0 && S.root_states && i < nxk) r += (i - pad == j) ? 1.0 : 0.0;
        if (i < nxk) S.dx[xo + i + (size_t)j * S.sum_nx] = r;
        else {
            S.du[uo + i - nxk + (size_t)j * S.sum_nu] = r;
            if (k == 0) S.head[(i - nxk) + (size_t)j * nuk] = r;
        }
    }
    if (k == 0) {
        double *h = S.head + (size_t)nuk * nx0;
        for (int i = lane; i < nuk; i += WAVE) h[i] = S.u[i];
        for (int j = lane; j < nx0; j += WAVE) h[nuk + j] = S.root_states ? D.xmin[pad + j] : S.x0[j];
        if (lane == 0) h[nuk + nx0] = (double)*S.n_reg;
    }
}

/* ---- k_mpc_predict: block 0: u0_pred[i] = u0[i], then fma(K[i, j], dx_j, .) over j ascending, dx_j = x0_new[j] - x0_ref[j], clipped into
 * [umin[0], umax[0]] on a root of kind 0; blocks 1 + k (duals != 0): entry e of node k of the start buffer = the current dual, then
 * fma(dLam[e, j], dx_j, .) over j ascending (lam_keep: the entry it replaces is saved first).  out: pinned, [u0_pred (nu0) | n_clipped] ---- */
__device__ void sens_predict_body(const Tree &T, const Data &D, const Sens &S, const double *x0_new, double *lam_init, double *lam_keep, double *out, int blk, int lane) {
    const int nx0 = S.nx0, nu0 = S.nu0;
    const double *h = S.head, *x0r = h + (size_t)nu0 * nx0 + nu0;
    if (blk == 0) {
        const bool clip = sens_kind(D, 0) == 0;
        int moved = 0;
        for (int i0 = 0; i0 < nu0; i0 += WAVE) {
            const int i = i0 + lane;
            bool mv = false;
            if (i < nu0) {
                double w = h[(size_t)nu0 * nx0 + i];
                for (int j = 0; j < nx0; j++) w = fma(h[i + (size_t)j * nu0], x0_new[j] - x0r[j], w);
                if (clip) {
                    const double lo = D.umin[i], hi = D.umax[i];
                    if (w < lo) { w = lo; mv = true; } else if (w > hi) { w = hi; mv = true; }
                }
                out[i] = w;
            }
            moved += __popcll(__builtin_amdgcn_ballot_w64(mv));
        }
        if (lane == 0) out[nu0] = (double)moved;
        return;
    }
    const int k = blk - 1, xo = T.xoff[k];
    const double *src = D.ctrl->cur ? D.lam1 : D.lam0;
    for (int e = lane; e < T.nx[k]; e += WAVE) {
        double w = src[xo + e];
        for (int j = 0; j < nx0; j++) w = fma(S.dlam[xo + e + (size_t)j * S.sum_nx], x0_new[j] - x0r[j], w);
        if (lam_keep) lam_keep[xo + e] = lam_init[xo + e];
        lam_init[xo + e] = w;
    }
}

/* ---- the adjoint of a step (tqgpu_mpc_adjoint): w = dL/dz for a scalar loss of the solution z = (x, u), nw columns at once ----
 *   R_c = (P_c w_c)^x - C_c P_p w_p,   M Y = R with the factor k_sens_factor left (L, CholUt, invd),   gb_c = Y_c,
 *   [gq_k; gr_k] = -P_k ( w_k - [Y_k; 0] + sum_c C_c' Y_c ),
 *   gx0 = sum_c A0_c' Y_c + S0' gr_0 (eliminated root),  wx_0 + sum_c A_c' Y_c (root with states).
 * R is non-zero in every block, so the solve has the leaf-to-root sweep the forward sensitivity skips: t_ii = L_ii^-1 R_ii, the push
 * R_dad[pos ..] -= CholUt_ii t_ii (the rows of node ii, which no other block of the level touches: no atomics), Y_0 = L_0^-T t_0 at the
 * root, then Y_ii = L_ii^-T ( t_ii - CholUt_ii' Y_dad[pos ..] ) level by level.  One wave per (unit, column) on blockIdx.y. */
struct Adj {
    const double *wx, *wu;             /* the staged w: (sum_nx - xpad) x nw and sum_nu x nw, column major, the flat layout of the solution */
    double *Y, *t;                     /* sum_nx x nw each, column major, node-indexed as Sens::dlam: R, then Y in its place; t of the non-root blocks */
    double *gq, *gr, *gb;              /* sum_nx x nw, sum_nu x nw, sum_nx x nw, node-indexed (phantom root states included; gb: the root's rows stay 0) */
    double *head;                      /* [gx0 (nx0 x nw, column major) | n_reg] */
    double *glx, *gux, *glu, *guu;     /* dL/dxmin, dL/dxmax (sum_nx x nw), dL/dumin, dL/dumax (sum_nu x nw), node-indexed as gq, gr: v on the side the exported value sits on, 0.0 elsewhere */
    int nw, nxe;
};
/* entry i of w_k, i over [x | u], column col; phantom root states carry 0 */
__device__ __forceinline__ double adj_w(const Tree &T, const Sens &S, const Adj &A, int k, int i, int col) {
    const int nx = T.nx[k];
    if (i < nx) {
        const int g = T.xoff[k] + i;
        return g < S.xpad ? 0.0 : A.wx[g - S.xpad + (size_t)col * A.nxe];
    }
    return A.wu[T.uoff[k] + i - nx + (size_t)col * S.sum_nu];
}
/* entry i of P_k w_k */
__device__ __forceinline__ double adj_pw(const Tree &T, const Data &D, const Sens &S, const Adj &A, int k, int i, int col) {
    const int nx = T.nx[k], nz = nx + T.nu[k];
    if (sens_kind(D, k) == 0) return (i < nx ? S.Px[T.xoff[k] + i] : S.Pu[T.uoff[k] + i - nx]) * adj_w(T, S, A, k, i, col);
    const double *P = D.Pd + D.poff[k];
    double acc = 0.0;
    for (int m = 0; m < nz; m++) acc = fma(P[i + (size_t)m * nz], adj_w(T, S, A, k, m, col), acc);
    return acc;
}

/* ---- k_adj_rhs: one wave per (parent block p, column): the rows of p's children of R ---- */
__device__ void adj_rhs_body(const Tree &T, const Data &D, const Sens &S, const Adj &A, int p, int col, int lane, double *lds) {
    const int nxp = T.nx[p], nup = T.nu[p], nz = nxp + nup, k0 = T.kid0[p];
    double *pv = lds;                     /* nz: P_p w_p */
    for (int i = lane; i < nz; i += WAVE) pv[i] = adj_pw(T, D, S, A, p, i, col);
    WSYNC();
    double *R = A.Y + (size_t)col * S.sum_nx;
    for (int cc = 0; cc < T.nk[p]; cc++) {
        const int kid = k0 + cc, nxc = T.nx[kid];
        const double *Ac = D.A + T.aoff[kid], *Bc = D.B + T.boff[kid];
        for (int i = lane; i < nxc; i += WAVE) {
            double acc = 0.0;
            for (int m = 0; m < nxp; m++) acc = fma(Ac[i + (size_t)m * nxc], pv[m], acc);
            for (int m = 0; m < nup; m++) acc = fma(Bc[i + (size_t)m * nxc], pv[nxp + m], acc);
            R[T.xoff[kid] + i] = adj_pw(T, D, S, A, kid, i, col) - acc;
        }
    }
}

/* ---- k_adj_backward: one wave per (block of one level, column), deepest level first: t = L^-1 R_ii (column-oriented forward substitution),
 * the push into the parent's rows of R; the root's instance goes on to Y_0 = L^-T t ---- */
__device__ void adj_backward_body(const Tree &T, const Sens &S, const Adj &A, int ii, int col, int lane, double *lds) {
    const int d = T.bdim[ii], ld = d | 1;
    double *L = lds;                      /* ld x d */
    double *z = lds + (size_t)ld * d;     /* d */
    double *iv = z + d;                   /* d */
    const int bo = T.xoff[T.kid0[ii]];
    const double *Lg = S.CholW + T.woff[ii];
    double *R = A.Y + (size_t)col * S.sum_nx;
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * ld] = Lg[i + (size_t)j * d];
    }
    for (int j = lane; j < d; j += WAVE) { iv[j] = S.invd[bo + j]; z[j] = R[bo + j]; }
    for (int k = 0; k < d; k++) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = k + 1 + lane; i < d; i += WAVE) z[i] = fma(-L[i + (size_t)k * ld], zk, z[i]);
        WSYNC();
        if (lane == 0) z[k] = zk;
    }
    WSYNC();
    if (ii > 0) {
        const int nxi = T.nx[ii], xo = T.xoff[ii];
        const double *CUt = S.CholUt + T.utoff[ii];
        double *t = A.t + (size_t)col * S.sum_nx;
        for (int j = lane; j < d; j += WAVE) t[bo + j] = z[j];
        for (int i = lane; i < nxi; i += WAVE) {
            double acc = 0.0;
            for (int j = 0; j < d; j++) acc = fma(CUt[i + (size_t)j * nxi], z[j], acc);
            R[xo + i] -= acc;
        }
        return;
    }
    for (int k = d - 1; k >= 0; k--) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = lane; i < k; i += WAVE) z[i] = fma(-L[k + (size_t)i * ld], zk, z[i]);
        WSYNC();
        if (lane == 0) z[k] = zk;
    }
    WSYNC();
    for (int j = lane; j < d; j += WAVE) R[bo + j] = z[j];
}

/* ---- k_adj_forward: one wave per (block of one level below the root, column): Y_ii = L^-T ( t_ii - CholUt' Y_dad[pos ..] ),
 * sens_forward_body's substitution plus the t term ---- */
__device__ void adj_forward_body(const Tree &T, const Sens &S, const Adj &A, int ii, int col, int lane, double *lds) {
    const int d = T.bdim[ii], nxi = T.nx[ii], ld = d | 1;
    double *L = lds;                      /* ld x d */
    double *z = lds + (size_t)ld * d;     /* d */
    double *dl = z + d;                   /* nxi */
    double *iv = dl + nxi;                /* d */
    const int bo = T.xoff[T.kid0[ii]], xo = T.xoff[ii];
    const double *Lg = S.CholW + T.woff[ii];
    double *Y = A.Y + (size_t)col * S.sum_nx;
    const double *t = A.t + (size_t)col * S.sum_nx;
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * ld] = Lg[i + (size_t)j * d];
    }
    for (int j = lane; j < d; j += WAVE) iv[j] = S.invd[bo + j];
    for (int i = lane; i < nxi; i += WAVE) dl[i] = Y[xo + i];
    WSYNC();
    const double *CUt = S.CholUt + T.utoff[ii];
    for (int j = lane; j < d; j += WAVE) {
        double acc = 0.0;
        for (int i = 0; i < nxi; i++) acc = fma(CUt[i + (size_t)j * nxi], dl[i], acc);
        z[j] = t[bo + j] - acc;
    }
    for (int k = d - 1; k >= 0; k--) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = lane; i < k; i += WAVE) z[i] = fma(-L[k + (size_t)i * ld], zk, z[i]);
        WSYNC();
        if (lane == 0) z[k] = zk;
    }
    WSYNC();
    for (int j = lane; j < d; j += WAVE) Y[bo + j] = z[j];
}

/* ---- k_adj_grad: one wave per (node, column): gq, gr, gb; node 0 also gx0 and, in column 0, n_reg into the head ---- */
__device__ void adj_grad_body(const Tree &T, const Data &D, const Sens &S, const Adj &A, int k, int col, int lane, double *lds) {
    const int nxk = T.nx[k], nuk = T.nu[k], nz = nxk + nuk, nx0 = S.nx0, pad = k == 0 ? S.xpad : 0;
    const int xo = T.xoff[k], uo = T.uoff[k], k0 = T.kid0[k], nkids = k < T.Np ? T.nk[k] : 0;
    double *v = lds;                      /* nz: w_k - [Y_k; 0] + sum_c C_c' Y_c */
    double *g = lds + nz;                 /* nz: -P_k v */
    const double *Y = A.Y + (size_t)col * S.sum_nx;
    for (int i = lane; i < nz; i += WAVE) {
        double acc = 0.0;
        for (int cc = 0; cc < nkids; cc++) {
            const int kid = k0 + cc, nxc = T.nx[kid];
            const double *Cc = i < nxk ? D.A + T.aoff[kid] + (size_t)i * nxc : D.B + T.boff[kid] + (size_t)(i - nxk) * nxc;
            const double *yc = Y + T.xoff[kid];
            for (int r = 0; r < nxc; r++) acc = fma(Cc[r], yc[r], acc);
        }
        v[i] = adj_w(T, S, A, k, i, col) - (k > 0 && i < nxk ? Y[xo + i] : 0.0) + acc;
    }
    WSYNC();
    const int kind = sens_kind(D, k);
    for (int i = lane; i < nz; i += WAVE) {
        double r;
        if (kind == 0) r = (i < nxk ? S.Px[xo + i] : S.Pu[uo + i - nxk]) * v[i];
        else {
            const double *P = D.Pd + D.poff[k];
            r = 0.0;
            for (int m = 0; m < nz; m++) r = fma(P[i + (size_t)m * nz], v[m], r);
        }
        r = -r;
        g[i] = r;
        if (i < nxk) A.gq[xo + i + (size_t)col * S.sum_nx] = r; else A.gr[uo + i - nxk + (size_t)col * S.sum_nu] = r;
        /* the bound gradients: v where P is 0.0 because the exported value equals a bound bit for bit (sens_pdiag's test, read again only behind
         * that 0.0), on the lower side where it equals the lower bound; 0.0 on free entries, kind-1 nodes and phantom root states */
        double lo = 0.0, hi = 0.0;
        if (kind == 0 && i >= pad && (i < nxk ? S.Px[xo + i] : S.Pu[uo + i - nxk]) == 0.0) {
            const int e = i < nxk ? xo + i : uo + i - nxk;
            const double val = i < nxk ? S.x[e - S.xpad] : S.u[e];
            if (val == (i < nxk ? D.xmin[e] : D.umin[e])) lo = v[i];
            else if (val == (i < nxk ? D.xmax[e] : D.umax[e])) hi = v[i];
        }
        if (i < nxk) { A.glx[xo + i + (size_t)col * S.sum_nx] = lo; A.gux[xo + i + (size_t)col * S.sum_nx] = hi; }
        else { A.glu[uo + i - nxk + (size_t)col * S.sum_nu] = lo; A.guu[uo + i - nxk + (size_t)col * S.sum_nu] = hi; }
    }
    if (k > 0) {
        for (int i = lane; i < nxk; i += WAVE) A.gb[xo + i + (size_t)col * S.sum_nx] = Y[xo + i];
        return;
    }
    WSYNC();
    double *gx0 = A.head + (size_t)col * nx0;
    for (int j = lane; j < nx0; j += WAVE) {
        double r;
        if (S.root_states) r = v[pad + j];
        else {
            r = 0.0;
            int ao = 0;
            for (int cc = 0; cc < nkids; cc++) {
                const int kid = k0 + cc, nxc = T.nx[kid];
                const double *A0 = S.A0 + ao + (size_t)j * nxc, *yc = Y + T.xoff[kid];
                for (int i = 0; i < nxc; i++) r = fma(A0[i], yc[i], r);
                ao += nxc * nx0;
            }
            if (S.S0) for (int m = 0; m < nuk; m++) r = fma(S.S0[m + (size_t)j * nuk], g[nxk + m], r);
        }
        gx0[j] = r;
    }
    if (col == 0 && lane == 0) A.head[(size_t)nx0 * A.nw] = (double)*S.n_reg;
}

__global__ void __launch_bounds__(WAVE) k_sens_hess(Tree T, Data D, Sens S)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    sens_hess_body(T, D, S, blockIdx.x, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_sens_factor(Tree T, Opts O, Sens S, int first)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    sens_factor_body(T, O, S, first + (int)blockIdx.x, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_sens_forward(Tree T, Sens S, int first)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    sens_forward_body(T, S, first + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_sens_primal(Tree T, Data D, Sens S)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    sens_primal_body(T, D, S, blockIdx.x, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_mpc_predict(Tree T, Data D, Sens S, const double *x0_new, double *lam_init, double *lam_keep, double *out)
#if !TQ_HAS(TQP_SENS)
;
#else
{ sens_predict_body(T, D, S, x0_new, lam_init, lam_keep, out, blockIdx.x, threadIdx.x); }
#endif
__global__ void __launch_bounds__(WAVE) k_adj_rhs(Tree T, Data D, Sens S, Adj A)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    adj_rhs_body(T, D, S, A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_backward(Tree T, Sens S, Adj A, int first)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    adj_backward_body(T, S, A, first + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_forward(Tree T, Sens S, Adj A, int first)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    adj_forward_body(T, S, A, first + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_grad(Tree T, Data D, Sens S, Adj A)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    adj_grad_body(T, D, S, A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif

/* ---- the adjoint for a batch of mirrors in one set of launches (tqgpu_mpc_adjoint_batch) ----
 * One descriptor per member, uploaded with every call: what the single launches pass as kernel arguments, and the member's level table,
 * which the single launches read on the host (lvl[2 l], lvl[2 l + 1]: first block and block count of block level l < T.Nh; the tables
 * travel in the same block behind the items).  Every kernel below is the single kernel's body behind a look-up of the member:
 * blockIdx.z = member, blockIdx.y = column, blockIdx.x = what it is in the single launch.  The grid is as wide as the largest member
 * needs at that launch; a wave beyond its member's own extent, on a level the member does not have, or in a hess / factor launch of a
 * member whose factor is stored, returns at once and writes nothing.  Launch j of the backward sweeps takes level T.Nh - 1 - j of a
 * member, launch j of the forward sweep level j + 1: members are independent, a shallow one finishes early.  No kernel waits for
 * another workgroup. */
struct AItem {
    Tree T; Data D; Opts O; Sens S; Adj A;
    const int *lvl;                /* [2 T.Nh] first, count of every block level */
    const double *lamc;            /* the packing (k_adj_export_batch, tdunes_adjoint.hpp): the current duals as the host knows them after the solve, */
    double *d_out;                 /* the member's export block, */
    int x_pad, nxe, nue, nl, nx0;  /* phantom root states, the export sizes (x without them, u, lam), the root's states */
    int needs_export, needs_factor;      /* d_out is not packed yet and the factor has to be built from it; the factor is not stored */
    double *head_out;              /* the batched sensitivity: where the member's head lies a second time, in the block of all heads of its group's lead */
};
__global__ void __launch_bounds__(WAVE) k_sens_hess_batch(const AItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    if (!it.needs_factor || (int)blockIdx.x >= it.T.Np) return;
    sens_hess_body(it.T, it.D, it.S, blockIdx.x, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_sens_factor_batch(const AItem *__restrict__ items, int j)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    const int lvl = it.T.Nh - 1 - j;
    if (!it.needs_factor || lvl < 0 || (int)blockIdx.x >= it.lvl[2 * lvl + 1]) return;
    sens_factor_body(it.T, it.O, it.S, it.lvl[2 * lvl] + (int)blockIdx.x, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_rhs_batch(const AItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    if ((int)blockIdx.x >= it.T.Np || (int)blockIdx.y >= it.A.nw) return;
    adj_rhs_body(it.T, it.D, it.S, it.A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_backward_batch(const AItem *__restrict__ items, int j)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    const int lvl = it.T.Nh - 1 - j;
    if (lvl < 0 || (int)blockIdx.x >= it.lvl[2 * lvl + 1] || (int)blockIdx.y >= it.A.nw) return;
    adj_backward_body(it.T, it.S, it.A, it.lvl[2 * lvl] + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_forward_batch(const AItem *__restrict__ items, int j)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    const int lvl = j + 1;
    if (lvl >= it.T.Nh || (int)blockIdx.x >= it.lvl[2 * lvl + 1] || (int)blockIdx.y >= it.A.nw) return;
    adj_forward_body(it.T, it.S, it.A, it.lvl[2 * lvl] + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adj_grad_batch(const AItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    if ((int)blockIdx.x >= it.T.Nn || (int)blockIdx.y >= it.A.nw) return;
    adj_grad_body(it.T, it.D, it.S, it.A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif

/* ---- the sensitivities and the predictor for a batch of mirrors (tqgpu_mpc_sensitivity_batch, tqgpu_mpc_predict_batch) ----
 * The forward half over the same descriptor: k_adj_export_batch, k_sens_hess_batch and k_sens_factor_batch above with needs_factor set for every
 * member, then the two kernels below.  blockIdx.y of the forward sweep is the column of x0: the members' nx0 differ, the grid is as tall as the
 * largest, a wave beyond its member's nx0 returns at once.  The node-0 wave of k_sens_primal_batch fills the member's own head (Sens::head, which
 * k_mpc_predict reads later) as the single kernel does, and then copies it to AItem::head_out, so that the heads of a group come back in one copy. */
__global__ void __launch_bounds__(WAVE) k_sens_forward_batch(const AItem *__restrict__ items, int j)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    const int lvl = j + 1;
    if (lvl >= it.T.Nh || (int)blockIdx.x >= it.lvl[2 * lvl + 1] || (int)blockIdx.y >= it.S.nx0) return;
    sens_forward_body(it.T, it.S, it.lvl[2 * lvl] + (int)blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_sens_primal_batch(const AItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AItem &it = items[blockIdx.z];
    if ((int)blockIdx.x >= it.T.Nn) return;
    sens_primal_body(it.T, it.D, it.S, blockIdx.x, threadIdx.x, lds);
    if (blockIdx.x != 0) return;
    /* the head this wave has just written, read back by other lanes than wrote it: through a device-scope fence */
    __threadfence();
    WSYNC();
    const int n = it.S.nu0 * it.S.nx0 + it.S.nu0 + it.S.nx0 + 1;
    for (int e = threadIdx.x; e < n; e += WAVE) it.head_out[e] = it.S.head[e];
}
#endif
/* one member of a batched predictor: what k_mpc_predict takes as kernel arguments.  x0_new and out lie in a pinned block of the group's lead */
struct PredItem { Tree T; Data D; Sens S; const double *x0_new; double *lam_init, *lam_keep, *out; int duals; };
__global__ void __launch_bounds__(WAVE) k_mpc_predict_batch(const PredItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    const PredItem &it = items[blockIdx.z];
    if (blockIdx.x > 0 && (!it.duals || (int)blockIdx.x - 1 >= it.T.Nn)) return;
    sens_predict_body(it.T, it.D, it.S, it.x0_new, it.lam_init, it.lam_keep, it.out, blockIdx.x, threadIdx.x);
}
#endif

/* ---- the adjoint in H, A, B (tqgpu_mpc_adjoint_matrices): outer products of a stored adjoint with the point, summed over parameter groups ----
 *   z_k = [x_k; u_k] the exported point, gz_k = [gq_k; gr_k] and gb_c = Y_c of struct Adj, lam_c the exported dual (its sign is the one
 *   for which stationarity off the bounds reads H z + g + E' lam = 0 with (E v)_c = C_c v_p - v_c^x); phantom root states carry 0 in z and gz.
 *   kind-0 node k:   gHd_k[i] = gz_k[i] z_k[i]                      kind-1 node k:   gH_k = 1/2 (gz_k z_k' + z_k gz_k'), i >= j computed, mirrored
 *   child c of p:    gA_c = lam_c gq_p' + gb_c x_p',  gB_c = lam_c gr_p' + gb_c u_p'      linear terms: gh_k = gz_k, gb_c
 *   eliminated root: gA0_c = gb_c x0', gS0 = gr_0 x0' (0.0 where S0 was not given)
 * A group's members are taken in ascending node index in chunks of ADJMAT_CHUNK; a chunk's partial is one chain from 0.0 over its members,
 * per member  acc = fma(lam_c[i], gz_p[j], acc); acc = fma(gb_c[i], z_p[j], acc)  (gA, gB),  acc = fma(gz_k[i], z_k[i], acc)  (gHd),
 * acc = fma(gz_k[i], z_k[j], acc); acc = fma(z_k[i], gz_k[j], acc), halved at the end  (gH),  acc = acc + v[i]  (gh, gb); the group's value is
 * the first partial plus the others in ascending chunk order (k_adjmat_sum), in the reducing batch form in ascending (member, chunk) order.
 * No atomics.  One wave per (chunk, column) on a private LDS window [accumulators | the member's vectors]; Data, Sens, Adj are only read. */
#define ADJMAT_CHUNK 64
#define ADJMAT_PF 2                    /* doubles per lane of the next member's vectors kept in flight ahead of the current member's fmas */
struct AdjMat {
    const int *hmem, *cmem;            /* the members (nodes) of the h-groups / c-groups, group after group, ascending within a group */
    const int *hgrp, *cgrp;            /* 8 ints per group: [0] its first member, [1..3] where its result blocks begin (h: gH, gh, -; c: gA, gB, gb), [4] its
                                        * first chunk, [5] its chunks, [6] where its partials begin; offsets in doubles per column of w */
    const int *hchk, *cchk;            /* 4 ints per chunk: group, first member (index into hmem / cmem), members, index of the chunk within its group */
    const int *sums;                   /* the groups of more than one chunk, as units: h-group g = g, c-group g = n_hgrp + g */
    const double *lam;                 /* the duals of the export block (sum_lam) */
    double *res, *part;                /* [gH | gh | gA | gB | gb | gA0 | gS0], every region groups ascending, then columns; the partials */
    int n_hgrp, n_cgrp, n_hchk, n_cchk, n_sums;
    int root;                          /* 1: an eliminated root, the last unit is gA0, gS0 */
    int oA0, oS0, pR;                  /* where gA0, gS0 and the root unit's partial begin, in doubles per column */
};
/* what a unit (h-group, c-group, the root terms) writes: up to three result blocks of s1, s2, s3 doubles per column at o1, o2, o3, one partial of gsz */
struct AdjMatUnit { int s1, s2, s3, o1, o2, o3, gsz, po, nchk, kind, nz, nxc, nzp; };
__device__ __forceinline__ AdjMatUnit adjmat_unit(const Tree &T, const Data &D, const Sens &S, const AdjMat &M, int unit) {
    AdjMatUnit U{};
    if (unit < M.n_hgrp) {
        const int *rec = M.hgrp + 8 * unit;
        const int k = rec[0];
        U.nz = T.nx[k] + T.nu[k]; U.kind = sens_kind(D, k);
        U.s1 = U.kind ? U.nz * U.nz : U.nz; U.s2 = U.nz; U.s3 = 0;
        U.o1 = rec[1]; U.o2 = rec[2]; U.o3 = 0; U.nchk = rec[5]; U.po = rec[6];
    } else if (unit < M.n_hgrp + M.n_cgrp) {
        const int *rec = M.cgrp + 8 * (unit - M.n_hgrp);
        const int c = rec[0], p = T.dad[c];
        U.nxc = T.nx[c]; U.nzp = T.nx[p] + T.nu[p];
        U.s1 = U.nxc * T.nx[p]; U.s2 = U.nxc * T.nu[p]; U.s3 = U.nxc;
        U.o1 = rec[1]; U.o2 = rec[2]; U.o3 = rec[3]; U.nchk = rec[5]; U.po = rec[6];
    } else {
        U.s1 = T.bdim[0] * S.nx0; U.s2 = T.nu[0] * S.nx0; U.s3 = 0;
        U.o1 = M.oA0; U.o2 = M.oS0; U.o3 = 0; U.nchk = 1; U.po = M.pR;
    }
    U.gsz = U.s1 + U.s2 + U.s3;
    return U;
}
/* entry e of a unit's partial, column col: where it lies in res */
__device__ __forceinline__ size_t adjmat_res_at(const AdjMatUnit &U, int e, int col, int nw) {
    if (e < U.s1) return (size_t)U.o1 * nw + (size_t)col * U.s1 + e;
    e -= U.s1;
    if (e < U.s2) return (size_t)U.o2 * nw + (size_t)col * U.s2 + e;
    return (size_t)U.o3 * nw + (size_t)col * U.s3 + (e - U.s2);
}
__device__ __forceinline__ size_t adjmat_part_at(const AdjMatUnit &U, int q, int e, int col, int nw) {
    return ((size_t)U.po + (size_t)q * U.gsz) * nw + (size_t)col * U.gsz + e;
}
/* entry idx of [z_k (nz) | gz_k (nz)] of node k */
__device__ __forceinline__ double adjmat_hvec(const Tree &T, const Sens &S, const Adj &A, int k, int nx, int nz, int idx, int col) {
    const bool g = idx >= nz;
    const int i = g ? idx - nz : idx;
    if (i < nx) {
        const int e = T.xoff[k] + i;
        if (e < S.xpad) return 0.0;
        return g ? A.gq[e + (size_t)col * S.sum_nx] : S.x[e - S.xpad];
    }
    const int e = T.uoff[k] + i - nx;
    return g ? A.gr[e + (size_t)col * S.sum_nu] : S.u[e];
}
/* entry idx of [lam_c (nxc) | gb_c (nxc) | z_p (nzp) | gz_p (nzp)] of child c with parent p */
__device__ __forceinline__ double adjmat_cvec(const Tree &T, const Sens &S, const Adj &A, const AdjMat &M, int c, int p, int nxc, int nxp, int nzp, int idx, int col) {
    if (idx < nxc) return M.lam[T.xoff[c] - T.nx0 + idx];
    if (idx < 2 * nxc) return A.gb[T.xoff[c] + idx - nxc + (size_t)col * S.sum_nx];
    return adjmat_hvec(T, S, A, p, nxp, nzp, idx - 2 * nxc, col);
}

/* ---- k_adjmat_part: one wave per (chunk of a group, column); the unit behind the chunks is the root terms of an eliminated root.  all_partial: every
 * chunk writes its partial (the reducing batch form); otherwise the only chunk of a group writes the group's result itself ---- */
__device__ void adjmat_part_body(const Tree &T, const Data &D, const Sens &S, const Adj &A, const AdjMat &M, int unit, int col, int all_partial, int lane, double *lds) {
    const int nw = A.nw;
    if (unit >= M.n_hchk + M.n_cchk) {
        const AdjMatUnit U = adjmat_unit(T, D, S, M, M.n_hgrp + M.n_cgrp);
        const int nx0 = S.nx0, nu0 = T.nu[0], k0 = T.kid0[0];
        for (int e = lane; e < U.gsz; e += WAVE) {
            double v;
            if (e < U.s1) {
                /* A0 lies child after child, each nx[kid] x nx0: find the entry's child */
                int ao = 0, kid = k0;
                for (; kid < k0 + T.nk[0]; kid++) { const int n = T.nx[kid] * nx0; if (e < ao + n) break; ao += n; }
                const int nxc = T.nx[kid], i = (e - ao) % nxc, j = (e - ao) / nxc;
                v = A.gb[T.xoff[kid] + i + (size_t)col * S.sum_nx] * S.x0[j];
            } else {
                const int i = (e - U.s1) % nu0, j = (e - U.s1) / nu0;
                v = S.S0 ? A.gr[T.uoff[0] + i + (size_t)col * S.sum_nu] * S.x0[j] : 0.0;
            }
            if (all_partial) M.part[adjmat_part_at(U, 0, e, col, nw)] = v; else M.res[adjmat_res_at(U, e, col, nw)] = v;
        }
        return;
    }
    const bool isc = unit >= M.n_hchk;
    const int *ck = isc ? M.cchk + 4 * (unit - M.n_hchk) : M.hchk + 4 * unit;
    const AdjMatUnit U = adjmat_unit(T, D, S, M, isc ? M.n_hgrp + ck[0] : ck[0]);
    const int *mem = (isc ? M.cmem : M.hmem) + ck[1];
    const int cnt = ck[2], q = ck[3];
    const int rep = mem[0], nxc = U.nxc, nzp = isc ? U.nzp : U.nz, nxp = isc ? T.nx[T.dad[rep]] : T.nx[rep];
    const int L = isc ? 2 * nxc + 2 * nzp : 2 * nzp, gsz = U.gsz, hsz = U.s1;
    double *acc = lds;                    /* gsz */
    double *vec = lds + gsz;              /* L: the vectors of the member in hand */
    for (int e = lane; e < gsz; e += WAVE) acc[e] = 0.0;
    auto fetch = [&](int node, int idx) { return isc ? adjmat_cvec(T, S, A, M, node, T.dad[node], nxc, nxp, nzp, idx, col) : adjmat_hvec(T, S, A, node, nxp, nzp, idx, col); };
    int n1 = rep, n2 = cnt > 1 ? mem[1] : rep;
    double pre[ADJMAT_PF];
#pragma unroll
    for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; pre[r] = idx < L ? fetch(n1, idx) : 0.0; }
    for (int m = 0; m < cnt; m++) {
        const int cur = n1;
        n1 = n2;
        if (m + 2 < cnt) n2 = mem[m + 2];
#pragma unroll
        for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; if (idx < L) vec[idx] = pre[r]; }
        for (int idx = lane + ADJMAT_PF * WAVE; idx < L; idx += WAVE) vec[idx] = fetch(cur, idx);
        WSYNC();
        if (m + 1 < cnt) {          /* the next member's loads go out ahead of this member's fmas */
#pragma unroll
            for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; pre[r] = idx < L ? fetch(n1, idx) : 0.0; }
        }
        if (isc) {
            const double *lam = vec, *gb = vec + nxc, *zp = vec + 2 * nxc, *gzp = zp + nzp;
            for (int e = lane; e < gsz; e += WAVE) {
                const int i = e % nxc, j = e / nxc;
                double a = acc[e];
                if (j < nzp) { a = fma(lam[i], gzp[j], a); a = fma(gb[i], zp[j], a); }
                else a = a + gb[i];
                acc[e] = a;
            }
        } else {
            const double *z = vec, *gz = vec + nzp;
            for (int e = lane; e < gsz; e += WAVE) {
                double a = acc[e];
                if (e >= hsz) a = a + gz[e - hsz];
                else if (U.kind) {
                    const int i = e % nzp, j = e / nzp;
                    if (i < j) continue;
                    a = fma(gz[i], z[j], a); a = fma(z[i], gz[j], a);
                } else a = fma(gz[e], z[e], a);
                acc[e] = a;
            }
        }
        WSYNC();
    }
    const bool direct = !all_partial && U.nchk == 1;
    for (int e = lane; e < gsz; e += WAVE) {
        double v = acc[e];
        if (!isc && U.kind && e < hsz) { const int i = e % nzp, j = e / nzp; v = 0.5 * acc[i >= j ? e : j + i * nzp]; }
        if (direct) M.res[adjmat_res_at(U, e, col, nw)] = v; else M.part[adjmat_part_at(U, q, e, col, nw)] = v;
    }
}
/* ---- k_adjmat_sum: one wave per (group of more than one chunk, column): the first partial plus the others, ascending ---- */
__device__ void adjmat_sum_body(const Tree &T, const Data &D, const Sens &S, const AdjMat &M, int nw, int unit, int col, int lane) {
    const AdjMatUnit U = adjmat_unit(T, D, S, M, unit);
    for (int e = lane; e < U.gsz; e += WAVE) {
        double v = M.part[adjmat_part_at(U, 0, e, col, nw)];
        for (int q = 1; q < U.nchk; q++) v = v + M.part[adjmat_part_at(U, q, e, col, nw)];
        M.res[adjmat_res_at(U, e, col, nw)] = v;
    }
}
__global__ void __launch_bounds__(WAVE) k_adjmat_part(Tree T, Data D, Sens S, Adj A, AdjMat M)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    adjmat_part_body(T, D, S, A, M, blockIdx.x, blockIdx.y, 0, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adjmat_sum(Tree T, Data D, Sens S, AdjMat M, int nw)
#if !TQ_HAS(TQP_SENS)
;
#else
{ adjmat_sum_body(T, D, S, M, nw, M.sums[blockIdx.x], blockIdx.y, threadIdx.x); }
#endif

/* the batch forms (tqgpu_mpc_adjoint_matrices_batch): the same bodies behind a look-up of the member, blockIdx.z = member.  In the reducing form every
 * member's res is the one block of the call, every chunk writes its partial into its own member's buffer and k_adjmat_reduce, one wave per (unit, column),
 * adds them in ascending (member, chunk) order; the members' tables have equal shapes then */
struct AMItem { Tree T; Data D; Sens S; Adj A; AdjMat M; };
__global__ void __launch_bounds__(WAVE) k_adjmat_part_batch(const AMItem *__restrict__ items, int all_partial)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const AMItem &it = items[blockIdx.z];
    if ((int)blockIdx.x >= it.M.n_hchk + it.M.n_cchk + it.M.root || (int)blockIdx.y >= it.A.nw) return;
    adjmat_part_body(it.T, it.D, it.S, it.A, it.M, blockIdx.x, blockIdx.y, all_partial, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adjmat_sum_batch(const AMItem *__restrict__ items)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    const AMItem &it = items[blockIdx.z];
    if ((int)blockIdx.x >= it.M.n_sums || (int)blockIdx.y >= it.A.nw) return;
    adjmat_sum_body(it.T, it.D, it.S, it.M, it.A.nw, it.M.sums[blockIdx.x], blockIdx.y, threadIdx.x);
}
#endif
__global__ void __launch_bounds__(WAVE) k_adjmat_reduce(const AMItem *__restrict__ items, int n)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    const int unit = blockIdx.x, col = blockIdx.y, lane = threadIdx.x, nw = items[0].A.nw;
    const AdjMatUnit U0 = adjmat_unit(items[0].T, items[0].D, items[0].S, items[0].M, unit);
    for (int e = lane; e < U0.gsz; e += WAVE) {
        double v = 0.0;
        for (int m = 0; m < n; m++) {
            const AMItem &it = items[m];
            const AdjMatUnit U = adjmat_unit(it.T, it.D, it.S, it.M, unit);
            for (int q = 0; q < U.nchk; q++) {
                const double p = it.M.part[adjmat_part_at(U, q, e, col, nw)];
                v = (m == 0 && q == 0) ? p : v + p;
            }
        }
        items[0].M.res[adjmat_res_at(U0, e, col, nw)] = v;
    }
}
#endif

/* ---- sums of a per-node vector over sets of nodes in a fixed order (tqgpu_mpc_adjoint_bounds, tqgpu_mpc_adjoint_reference) ----
 *   mode 0, the bound gradients over the h-groups: a set is a group, the vector of member k is [glb_k (nz) | gub_k (nz)] of struct Adj, per member
 *           acc = acc + v[i];  the result of a set is its group's block of glb and of gub.
 *   mode 1, the tracking reference: a set is a stage, its members the nodes of that stage, the result the trajectory row the window in force sends
 *           the stage to, rho = min(t0 + stage, T - 1); [q_k; r_k] = base_k - H_k [xref; uref]_rho, so [gxref; guref]_rho = - sum_k H_k' gz_k:
 *           kind 0, per member  acc[j] = fma(-Qd[j], gq[j], acc[j]),  acc[NXT + j] = fma(-Rd[j], gr[j], acc[NXT + j]);
 *           kind 1, per member, for column j of the stored H_k (nz x nz, column major)  acc[j] = fma(-H[i + j nz], gz[i], acc[j]), i ascending
 *           over the rows behind the phantom root states (the fold leaves their q alone; they are no columns either);
 *           an eliminated root with S0, behind its own chain  acc[j] = fma(-S0[m + j nu0], gr_0[m], acc[j]), m ascending.
 *           A member without states (an eliminated root) or inputs (a leaf) leaves those entries alone.
 * The members of a set are taken in ascending node index in chunks of ADJMAT_CHUNK; a chunk's partial is one chain from 0.0 over its members; a
 * result is the first of its partials plus the others in ascending order: the chunks of the group (mode 0), of the row's stages in ascending
 * (stage, chunk) order (mode 1: a clamped last row collects several stages).  Chunks are cut per set, so the tables do not depend on t0.
 * One wave per (chunk, column) on a private LDS window [accumulators | the member's vector], the next member's vector in flight as in
 * k_adjmat_part; a result of one partial is written by its chunk, the others by k_nodesum_sum, one wave per (result, column).  No atomics; Data,
 * Sens, Adj are only read. */
struct NodeSum {
    const int *mem;                    /* the members (nodes), set after set, ascending within a set */
    const int *set;                    /* 4 ints per set: [0] its first chunk, [1] its chunks, [2] mode 0: where its block begins in glb, doubles per column, [3] the accumulators of a chunk */
    const int *chk;                    /* 4 ints per chunk: set, first member (index into mem), members, where its partial begins in doubles per column */
    double *res, *part;                /* mode 0: [glb | gub], each groups ascending, then columns; mode 1: per column, per row [gxref (NXT) | guref (NUT)] */
    int n_set, n_chk, mode;
    int tot;                           /* mode 0: the doubles per column of glb */
    int t0, Tn, nxt, nut, row0, rows;  /* mode 1: the window in force, the rows of the trajectory, its widths, the first row of the result and their number */
};
/* the chunks [c_lo, c_hi) whose partials make up result `target` (mode 0: the set; mode 1: row row0 + target) */
__host__ __device__ inline void nodesum_span(const int *set, int n_set, int mode, int t0, int Tn, int row0, int target, int &c_lo, int &c_hi) {
    int s_lo = target, s_hi = target;
    if (mode) {
        const int rho = row0 + target;
        if (rho >= Tn - 1) { s_lo = Tn - 1 - t0 > 0 ? Tn - 1 - t0 : 0; s_hi = n_set - 1; }
        else s_lo = s_hi = rho - t0;
    }
    c_lo = set[4 * s_lo]; c_hi = set[4 * s_hi] + set[4 * s_hi + 1];
}
__device__ __forceinline__ size_t nodesum_res_at(const NodeSum &N, int target, int W, int e, int col, int nw) {
    if (N.mode) return ((size_t)col * N.rows + target) * W + e;
    const int nz = W / 2, side = e >= nz;
    return (size_t)side * N.tot * nw + (size_t)N.set[4 * target + 2] * nw + (size_t)col * nz + (e - side * nz);
}
__device__ void nodesum_part_body(const Tree &T, const Data &D, const Sens &S, const Adj &A, const NodeSum &N, int unit, int col, int lane, double *lds) {
    const int nw = A.nw;
    const int *ck = N.chk + 4 * unit;
    const int set = ck[0], cnt = ck[2], W = N.set[4 * set + 3], nxt = N.nxt;
    const int *mem = N.mem + ck[1];
    double *acc = lds;                    /* W */
    double *vec = lds + W;                /* W: the vector of the member in hand */
    for (int e = lane; e < W; e += WAVE) acc[e] = 0.0;
    auto fetch = [&](int k, int idx) {
        const int nx = T.nx[k], nu = T.nu[k];
        if (N.mode) {          /* [gq_k behind the phantom states (NXT) | gr_k (NUT)], 0.0 for a part the member does not have */
            const int pad = k == 0 ? S.xpad : 0;
            if (idx < nxt) return nx - pad > 0 ? A.gq[T.xoff[k] + pad + idx + (size_t)col * S.sum_nx] : 0.0;
            return nu > 0 ? A.gr[T.uoff[k] + idx - nxt + (size_t)col * S.sum_nu] : 0.0;
        }
        const int nz = nx + nu, up = idx >= nz, i = up ? idx - nz : idx;
        if (i < nx) return (up ? A.gux : A.glx)[T.xoff[k] + i + (size_t)col * S.sum_nx];
        return (up ? A.guu : A.glu)[T.uoff[k] + i - nx + (size_t)col * S.sum_nu];
    };
    int n1 = mem[0], n2 = cnt > 1 ? mem[1] : n1;
    double pre[ADJMAT_PF];
#pragma unroll
    for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; pre[r] = idx < W ? fetch(n1, idx) : 0.0; }
    for (int m = 0; m < cnt; m++) {
        const int cur = n1;
        n1 = n2;
        if (m + 2 < cnt) n2 = mem[m + 2];
#pragma unroll
        for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; if (idx < W) vec[idx] = pre[r]; }
        for (int idx = lane + ADJMAT_PF * WAVE; idx < W; idx += WAVE) vec[idx] = fetch(cur, idx);
        WSYNC();
        if (m + 1 < cnt) {          /* the next member's loads go out ahead of this member's chain */
#pragma unroll
            for (int r = 0; r < ADJMAT_PF; r++) { const int idx = lane + r * WAVE; pre[r] = idx < W ? fetch(n1, idx) : 0.0; }
        }
        if (!N.mode) for (int e = lane; e < W; e += WAVE) acc[e] = acc[e] + vec[e];
        else {
            const int nx = T.nx[cur], nu = T.nu[cur], pad = cur == 0 ? S.xpad : 0, nz = nx + nu, xo = T.xoff[cur], uo = T.uoff[cur];
            const int kind = sens_kind(D, cur);
            const bool s0 = cur == 0 && !S.root_states && S.S0;
            for (int e = lane; e < W; e += WAVE) {
                const bool isx = e < nxt;
                const int j = isx ? e : e - nxt;
                double a = acc[e];
                if (isx ? nx - pad > 0 : nu > 0) {
                    if (kind == 0) a = fma(-(isx ? D.Qd[xo + pad + j] : D.Rd[uo + j]), vec[e], a);
                    else {
                        const double *H = D.Hd + D.poff[cur] + (size_t)(isx ? pad + j : nx + j) * nz;
                        for (int i = pad; i < nz; i++) a = fma(-H[i], vec[i < nx ? i - pad : nxt + i - nx], a);
                    }
                }
                if (s0 && isx) for (int mm = 0; mm < nu; mm++) a = fma(-S.S0[mm + (size_t)j * nu], vec[nxt + mm], a);
                acc[e] = a;
            }
        }
        WSYNC();
    }
    int c_lo, c_hi;
    const int target = N.mode ? ((N.t0 + set < N.Tn - 1 ? N.t0 + set : N.Tn - 1) - N.row0) : set;
    nodesum_span(N.set, N.n_set, N.mode, N.t0, N.Tn, N.row0, target, c_lo, c_hi);
    const bool direct = c_hi - c_lo == 1;
    for (int e = lane; e < W; e += WAVE) {
        if (direct) N.res[nodesum_res_at(N, target, W, e, col, nw)] = acc[e];
        else N.part[(size_t)ck[3] * nw + (size_t)col * W + e] = acc[e];
    }
}
/* ---- k_nodesum_sum: one wave per (result, column): the first partial plus the others, ascending; a result of one partial has been written already ---- */
__device__ void nodesum_sum_body(const NodeSum &N, int nw, int target, int col, int lane) {
    int c_lo, c_hi;
    nodesum_span(N.set, N.n_set, N.mode, N.t0, N.Tn, N.row0, target, c_lo, c_hi);
    if (c_hi - c_lo < 2) return;
    const int W = N.set[4 * N.chk[4 * c_lo] + 3];
    for (int e = lane; e < W; e += WAVE) {
        double v = N.part[(size_t)N.chk[4 * c_lo + 3] * nw + (size_t)col * W + e];
        for (int c = c_lo + 1; c < c_hi; c++) v = v + N.part[(size_t)N.chk[4 * c + 3] * nw + (size_t)col * W + e];
        N.res[nodesum_res_at(N, target, W, e, col, nw)] = v;
    }
}
__global__ void __launch_bounds__(WAVE) k_nodesum_part(Tree T, Data D, Sens S, Adj A, NodeSum N)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    nodesum_part_body(T, D, S, A, N, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_nodesum_sum(NodeSum N, int nw)
#if !TQ_HAS(TQP_SENS)
;
#else
{ nodesum_sum_body(N, nw, blockIdx.x, blockIdx.y, threadIdx.x); }
#endif

/* ---- the tangent of a step (tqgpu_mpc_tangent, tqgpu_mpc_predict_at): the forward-mode twin of the adjoint, nd directions at once ----
 *   dh_k = [dq_k; dr_k],   R_c = (P_c dh_c)^x - C_c P_p dh_p + db_c + G_c dx0   (G: the rows of the root's children, Sens::G),
 *   M dLam = R with the factor k_sens_factor left, through k_adj_backward / k_adj_forward on Tan::a (Y, t: the tangent's own),
 *   dZ_k = -P_k ( dh_k - [dLam_k; 0] + sum_c C_c' dLam_c ) + direct_k dx0,   direct_0 dx0 = -P_0 [0; S0 dx0] (eliminated root), [dx0; 0] (root with states).
 * The order is fixed: R is adj_rhs_body's expression with w := dh, then + db_c where db was given, then one chain fma(G[., j], dx0[j], .), j
 * ascending, where dx0 was given; dZ is adj_grad_body's chain for [gq; gr], then the direct term (S0 dx0: a chain from 0.0, j ascending; then
 * fma(-P_0[i, nx + m], (S0 dx0)[m], .), m ascending).  A term that was not given is skipped.  With db and dx0 absent (dx, du, dlam) are therefore
 * the (gq, gr, gb) of the adjoint for w = dh bit for bit.
 * The direction is either staged (built == 0: a.wx, a.wu hold dq, dr as adj_stage_w lays them out; db, dx0 where given) or built on the
 * device (built == 1, one column, tqgpu_mpc_predict_at): dx0[j] = x0_new[j] - x0_ref[j] (x0_new == nullptr: no dx0), and, where the window
 * moves (xtraj != nullptr), for node k with row(t) = min(t + stage[k], Tn - 1), dxref = xtraj[row(t1)] - xtraj[row(t0)], duref likewise, dh_k is
 * mpc_track_node's chain started from 0.0: kind 0 fma(-Qd[i], dxref[i], 0.0); kind 1 over row i of H_k, x columns then u columns; the u rows of
 * an x0-eliminated root with S0 go on with fma(-S0[i, j], dxref[j], .) (mpc_track_root_r without its + S0 x0, which is direct_0's). */
struct Tan {
    Adj a;                             /* wx, wu: the staged dq, dr; Y, t: R / dLam in the making and t; gq, gr, gb: dx, du, dlam (node-indexed as the adjoint's); head: [du0 (nu0 x nd) | n_reg]; nw = nd */
    const double *db, *dx0;            /* staged: sum_lam x nd, nx0 x nd, column major (nullptr: not given) */
    const double *x0_new;              /* built: pinned (nullptr: dx0 is zero and skipped) */
    const double *xtraj, *utraj;       /* built: the trajectory (nullptr: the window stays, dh = 0) */
    const int *stage;
    int built, t0, t1, Tn, nxt, nut, sum_lam;
};
__device__ __forceinline__ bool tan_has_dx0(const Tan &X) { return X.built ? X.x0_new != nullptr : X.dx0 != nullptr; }
__device__ __forceinline__ double tan_dx0(const Data &D, const Sens &S, const Tan &X, int j, int col) {
    if (!X.built) return X.dx0[j + (size_t)col * S.nx0];
    return X.x0_new[j] - (S.root_states ? D.xmin[S.xpad + j] : S.x0[j]);
}
__device__ __forceinline__ int tan_row(const Tan &X, int k, int t) {
    const int row = t + X.stage[k];
    return row < X.Tn - 1 ? row : X.Tn - 1;
}
/* entry i of dh_k, i over [x | u]; phantom root states carry 0 */
__device__ __forceinline__ double tan_w(const Tree &T, const Data &D, const Sens &S, const Tan &X, int k, int i, int col) {
    if (!X.built) return adj_w(T, S, X.a, k, i, col);
    const int nx = T.nx[k], nu = T.nu[k], nz = nx + nu, pad = k == 0 ? S.xpad : 0;
    if (!X.xtraj || i < pad) return 0.0;
    const int r1 = tan_row(X, k, X.t1), r0 = tan_row(X, k, X.t0);
    const double *x1 = X.xtraj + (size_t)r1 * X.nxt, *x0 = X.xtraj + (size_t)r0 * X.nxt;
    const double *u1 = X.utraj + (size_t)r1 * X.nut, *u0 = X.utraj + (size_t)r0 * X.nut;
    if (sens_kind(D, k) == 0)
        return i < nx ? fma(-D.Qd[T.xoff[k] + i], x1[i - pad] - x0[i - pad], 0.0) : fma(-D.Rd[T.uoff[k] + i - nx], u1[i - nx] - u0[i - nx], 0.0);
    const double *H = D.Hd + D.poff[k];
    double v = 0.0;
    for (int j = 0; j < nx - pad; j++) v = fma(-H[i + (size_t)(pad + j) * nz], x1[j] - x0[j], v);
    for (int j = 0; j < nu; j++) v = fma(-H[i + (size_t)(nx + j) * nz], u1[j] - u0[j], v);
    if (k == 0 && i >= nx && !S.root_states && S.S0)
        for (int j = 0; j < S.nx0; j++) v = fma(-S.S0[(i - nx) + (size_t)j * nu], x1[j] - x0[j], v);
    return v;
}
/* entry i of P_k w, w the nz staged entries of dh_k: adj_pw's arithmetic */
__device__ __forceinline__ double tan_pw(const Tree &T, const Data &D, const Sens &S, int k, int i, const double *w) {
    const int nx = T.nx[k], nz = nx + T.nu[k];
    if (sens_kind(D, k) == 0) return (i < nx ? S.Px[T.xoff[k] + i] : S.Pu[T.uoff[k] + i - nx]) * w[i];
    const double *P = D.Pd + D.poff[k];
    double acc = 0.0;
    for (int m = 0; m < nz; m++) acc = fma(P[i + (size_t)m * nz], w[m], acc);
    return acc;
}

/* ---- k_tan_rhs: one wave per (parent block p, column): the rows of p's children of R.  LDS: pv (nz of p), w (the largest nz) ---- */
__device__ void tan_rhs_body(const Tree &T, const Data &D, const Sens &S, const Tan &X, int p, int col, int lane, double *lds) {
    const int nxp = T.nx[p], nup = T.nu[p], nz = nxp + nup, k0 = T.kid0[p];
    double *pv = lds;                     /* nz: P_p dh_p */
    double *w = lds + nz;                 /* dh of p, then of each child in turn */
    for (int i = lane; i < nz; i += WAVE) w[i] = tan_w(T, D, S, X, p, i, col);
    WSYNC();
    for (int i = lane; i < nz; i += WAVE) pv[i] = tan_pw(T, D, S, p, i, w);
    WSYNC();
    double *R = X.a.Y + (size_t)col * S.sum_nx;
    const bool with_dx0 = p == 0 && tan_has_dx0(X);
    const int d0 = T.bdim[0], b0 = T.xoff[T.kid0[0]];          /* b0: the root's rows, which the flat layout of b does not have */
    for (int cc = 0; cc < T.nk[p]; cc++) {
        const int kid = k0 + cc, nxc = T.nx[kid], nzc = nxc + T.nu[kid];
        const double *Ac = D.A + T.aoff[kid], *Bc = D.B + T.boff[kid];
        for (int i = lane; i < nzc; i += WAVE) w[i] = tan_w(T, D, S, X, kid, i, col);
        WSYNC();
        for (int i = lane; i < nxc; i += WAVE) {
            double acc = 0.0;
            for (int m = 0; m < nxp; m++) acc = fma(Ac[i + (size_t)m * nxc], pv[m], acc);
            for (int m = 0; m < nup; m++) acc = fma(Bc[i + (size_t)m * nxc], pv[nxp + m], acc);
            double v = tan_pw(T, D, S, kid, i, w) - acc;
            if (X.db) v = v + X.db[T.xoff[kid] - b0 + i + (size_t)col * X.sum_lam];
            if (with_dx0) {
                const int row = T.xoff[kid] - T.xoff[k0] + i;
                for (int j = 0; j < S.nx0; j++) v = fma(S.G[row + (size_t)j * d0], tan_dx0(D, S, X, j, col), v);
            }
            R[T.xoff[kid] + i] = v;
        }
        WSYNC();
    }
}

/* ---- k_tan_primal: one wave per (node, column): dx, du, dlam; node 0 also du0 and, in column 0, n_reg into the head.  LDS: v (nz), w (nz) ---- */
__device__ void tan_primal_body(const Tree &T, const Data &D, const Sens &S, const Tan &X, int k, int col, int lane, double *lds) {
    const int nxk = T.nx[k], nuk = T.nu[k], nz = nxk + nuk, nx0 = S.nx0, pad = k == 0 ? S.xpad : 0;
    const int xo = T.xoff[k], uo = T.uoff[k], k0 = T.kid0[k], nkids = k < T.Np ? T.nk[k] : 0;
    const Adj &A = X.a;
    double *v = lds;                      /* nz: dh_k - [dLam_k; 0] + sum_c C_c' dLam_c */
    double *s0 = lds + nz;                /* nu0: S0 dx0 (node 0 of an eliminated root with S0) */
    const double *Y = A.Y + (size_t)col * S.sum_nx;
    for (int i = lane; i < nz; i += WAVE) {
        double acc = 0.0;
        for (int cc = 0; cc < nkids; cc++) {
            const int kid = k0 + cc, nxc = T.nx[kid];
            const double *Cc = i < nxk ? D.A + T.aoff[kid] + (size_t)i * nxc : D.B + T.boff[kid] + (size_t)(i - nxk) * nxc;
            const double *yc = Y + T.xoff[kid];
            for (int r = 0; r < nxc; r++) acc = fma(Cc[r], yc[r], acc);
        }
        v[i] = tan_w(T, D, S, X, k, i, col) - (k > 0 && i < nxk ? Y[xo + i] : 0.0) + acc;
    }
    const bool with_dx0 = k == 0 && tan_has_dx0(X), with_s0 = with_dx0 && !S.root_states && S.S0;
    if (with_s0) for (int m = lane; m < nuk; m += WAVE) {
        double acc = 0.0;
        for (int j = 0; j < nx0; j++) acc = fma(S.S0[m + (size_t)j * nuk], tan_dx0(D, S, X, j, col), acc);
        s0[m] = acc;
    }
    WSYNC();
    const int kind = sens_kind(D, k);
    for (int i = lane; i < nz; i += WAVE) {
        double r;
        if (kind == 0) r = (i < nxk ? S.Px[xo + i] : S.Pu[uo + i - nxk]) * v[i];
        else {
            const double *P = D.Pd + D.poff[k];
            r = 0.0;
            for (int m = 0; m < nz; m++) r = fma(P[i + (size_t)m * nz], v[m], r);
        }
        r = -r;
        if (with_s0 && kind != 0) {
            const double *P = D.Pd + D.poff[k];
            for (int m = 0; m < nuk; m++) r = fma(-P[i + (size_t)(nxk + m) * nz], s0[m], r);
        }
        if (with_dx0 && S.root_states && i >= pad && i < nxk) r = r + tan_dx0(D, S, X, i - pad, col);
        if (i < nxk) A.gq[xo + i + (size_t)col * S.sum_nx] = r;
        else {
            A.gr[uo + i - nxk + (size_t)col * S.sum_nu] = r;
            if (k == 0) A.head[(i - nxk) + (size_t)col * nuk] = r;
        }
    }
    if (k > 0) {
        for (int i = lane; i < nxk; i += WAVE) A.gb[xo + i + (size_t)col * S.sum_nx] = Y[xo + i];
        return;
    }
    if (col == 0 && lane == 0) A.head[(size_t)nuk * A.nw] = (double)*S.n_reg;
}

/* ---- k_tan_apply (tqgpu_mpc_predict_at): block 0: u0_pred[i] = u0*[i] + du0[i], clipped into [umin[0], umax[0]] on a root of kind 0; blocks 1 + k
 * (duals != 0): entry e of node k of the start buffer = the current dual + dLam[e] (lam_keep: the entry it replaces is saved first).
 * out: pinned, [u0_pred (nu0) | n_clipped | n_reg] ---- */
__device__ void tan_apply_body(const Tree &T, const Data &D, const Sens &S, const Tan &X, double *lam_init, double *lam_keep, double *out, int blk, int lane) {
    const int nu0 = S.nu0;
    if (blk == 0) {
        const bool clip = sens_kind(D, 0) == 0;
        int moved = 0;
        for (int i0 = 0; i0 < nu0; i0 += WAVE) {
            const int i = i0 + lane;
            bool mv = false;
            if (i < nu0) {
                double w = S.u[i] + X.a.gr[i];
                if (clip) {
                    const double lo = D.umin[i], hi = D.umax[i];
                    if (w < lo) { w = lo; mv = true; } else if (w > hi) { w = hi; mv = true; }
                }
                out[i] = w;
            }
            moved += __popcll(__builtin_amdgcn_ballot_w64(mv));
        }
        if (lane == 0) { out[nu0] = (double)moved; out[nu0 + 1] = (double)*S.n_reg; }
        return;
    }
    const int k = blk - 1, xo = T.xoff[k];
    const double *src = D.ctrl->cur ? D.lam1 : D.lam0;
    for (int e = lane; e < T.nx[k]; e += WAVE) {
        const double w = src[xo + e] + X.a.gb[xo + e];
        if (lam_keep) lam_keep[xo + e] = lam_init[xo + e];
        lam_init[xo + e] = w;
    }
}

__global__ void __launch_bounds__(WAVE) k_tan_rhs(Tree T, Data D, Sens S, Tan X)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    tan_rhs_body(T, D, S, X, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_tan_primal(Tree T, Data D, Sens S, Tan X)
#if !TQ_HAS(TQP_SENS)
;
#else
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    tan_primal_body(T, D, S, X, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
#endif
__global__ void __launch_bounds__(WAVE) k_tan_apply(Tree T, Data D, Sens S, Tan X, double *lam_init, double *lam_keep, double *out)
#if !TQ_HAS(TQP_SENS)
;
#else
{ tan_apply_body(T, D, S, X, lam_init, lam_keep, out, blockIdx.x, threadIdx.x); }
#endif

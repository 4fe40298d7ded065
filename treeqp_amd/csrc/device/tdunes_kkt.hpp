/*
 * tdunes_kkt.hpp -- the solution's way out and its check, in the host part: the export kernels (k_export_all, k_export_box, k_export_gen), the KKT
 * kernels (k_kkt, k_kkt_max), their batch forms behind KItem / KHead, and the entry points tqgpu_set_export_ahead, tqgpu_get_solution,
 * tqgpu_kkt_residual, _at, _batch and tqgpu_kkt_batch_stats.  Included once from tdunes_device.hip inside #if TQ_HAS(TQP_HOST), behind the batch
 * solve and ahead of tdunes_mpc.hpp, whose certified step calls mpc_enqueue_certificate.  tdunes_mirror.hpp keeps the mirror's records Export (s->out:
 * the packed solution and the export state, with its three transitions) and Kkt (s->kkt); tdunes_device.hip declares enqueue_export for tqgpu_solve.
 */
#pragma once

namespace {

/* solution export in one piece: out = [x | u | lam | dlam | mu_x | mu_u] (x and mu_x without the phantom root
 * states), mu = Q .* (xUnc - x) (export_mu, clipping.c:386-399) */
__device__ __forceinline__ void export_all_entry(int i, int n_x, int n_u, int n_lam, int x_pad, int nx0, const Data &D, const double *lamc, double *out) {
    double *ox = out, *ou = ox + n_x, *ol = ou + n_u, *od = ol + n_lam, *omx = od + n_lam, *omu = omx + n_x;
    /* MAXIMUM_ITERATIONS_REACHED with at least one iteration done: x, u are the last trial's, the unclipped values phase S's (see Data) */
    const bool maxit = D.ctrl->status == 1 && D.ctrl->iter > 0;
    if (i < n_x) {
        const int j = i + x_pad;
        ox[i] = D.x[j];
        omx[i] = D.Qd[j] * fma(-1.0, D.x[j], (maxit ? D.xUncS : D.xUnc)[j]);      /* dense nodes: Qd = 0 (no bounds, no multipliers) */
    }
    if (i < n_u) { ou[i] = D.u[i]; omu[i] = D.Rd[i] * fma(-1.0, D.u[i], (maxit ? D.uUncS : D.uUnc)[i]); }
    if (i < n_lam) {
        const double *lc = lamc ? lamc : (D.ctrl->cur ? D.lam1 : D.lam0);      /* (enqueued behind a solve that is still running: the device knows) */
        ol[i] = lc[nx0 + i]; od[i] = D.dlam[nx0 + i];
    }
}
__global__ void k_export_all(int n_x, int n_u, int n_lam, int x_pad, int nx0, Data D, const double *lamc, double *out) {
    export_all_entry(blockIdx.x * blockDim.x + threadIdx.x, n_x, n_u, n_lam, x_pad, nx0, D, lamc, out);
}

/* multipliers of the box nodes' bounds (export of the qpOASES stage solver, dual_Newton_tree_qpoases.c:524-560), over what
 * k_export_all wrote for them: mu = hmod - H z with the reference's sign, on the working set; 0 on free entries.  On a
 * MAXIMUM_ITERATIONS exit hmod is phase S's and z the last trial's, on every entry: the pairing of export_mu on clipping nodes
 * (see Data::xUncS), and on a diagonal node the same numbers.  One wave per node, lane = entry. */
__device__ __forceinline__ void export_box_node(const Tree &T, const Data &D, int n_x, int n_u, int n_lam, int x_pad, double *out, int k, int lane) {
    if (!D.dense || D.kind[k] != 2) return;
    const int nxk = T.nx[k], nz = nxk + T.nu[k], xo = T.xoff[k], uo = T.uoff[k];
    if (lane >= nz || (k == 0 && lane < x_pad)) return;           /* (phantom root states are not exported) */
    const bool maxit = D.ctrl->status == 1 && D.ctrl->iter > 0;
    const bool isx = lane < nxk;
    const int j0 = isx ? lane : lane - nxk;
    const double *H = D.Hd + D.poff[k];
    double hz = 0.0;
    for (int j = 0; j < nz; j++) hz = fma(H[lane + (size_t)j * nz], j < nxk ? D.x[xo + j] : D.u[uo + j - nxk], hz);
    const double h = isx ? (maxit ? D.xUncS : D.xUnc)[xo + j0] : (maxit ? D.uUncS : D.uUnc)[uo + j0];
    const double mu = (maxit || ((D.bmask[k] >> lane) & 1ull)) ? h - hz : 0.0;
    double *omx = out + n_x + n_u + 2 * (size_t)n_lam, *omu = omx + n_x;
    if (isx) omx[xo + j0 - x_pad] = mu; else omu[uo + j0] = mu;
}
__global__ void __launch_bounds__(WAVE) k_export_box(Tree T, Data D, int n_x, int n_u, int n_lam, int x_pad, double *out) {
    export_box_node(T, D, n_x, n_u, n_lam, x_pad, out, blockIdx.x, threadIdx.x);
}

/* the same for the nodes with general constraints (kind 3): mu = hmod - H z - G' mu_d on the fixed entries, with the row multipliers
 * stage_gen left in Gen::mu (the sign of tree_qp_out_calculate_KKT_res: Qx + q + ... + mu_x + C' mu_d = 0) */
__device__ __forceinline__ void export_gen_node(const Tree &T, const Data &D, int n_x, int n_u, int n_lam, int x_pad, double *out, int k, int lane) {
    if (!D.dense || D.kind[k] != 3) return;
    const Gen &Gn = *D.gen;
    const int nxk = T.nx[k], nz = nxk + T.nu[k], xo = T.xoff[k], uo = T.uoff[k], nc = Gn.nc[k];
    if (lane >= nz || (k == 0 && lane < x_pad)) return;
    const bool maxit = D.ctrl->status == 1 && D.ctrl->iter > 0;
    const bool isx = lane < nxk;
    const int j0 = isx ? lane : lane - nxk;
    const double *H = D.Hd + D.poff[k], *Gt = Gn.Gt + Gn.goff[k], *mud = Gn.mu + Gn.roff[k];
    double hz = 0.0;
    for (int j = 0; j < nz; j++) hz = fma(H[lane + (size_t)j * nz], j < nxk ? D.x[xo + j] : D.u[uo + j - nxk], hz);
    for (int r = 0; r < nc; r++) hz = fma(Gt[lane + (size_t)r * nz], mud[r], hz);
    const double h = isx ? (maxit ? D.xUncS : D.xUnc)[xo + j0] : (maxit ? D.uUncS : D.uUnc)[uo + j0];
    const double mu = (maxit || ((D.bmask[k] >> lane) & 1ull)) ? h - hz : 0.0;
    double *omx = out + n_x + n_u + 2 * (size_t)n_lam, *omu = omx + n_x;
    if (isx) omx[xo + j0 - x_pad] = mu; else omu[uo + j0] = mu;
}
__global__ void __launch_bounds__(WAVE) k_export_gen(Tree T, Data D, int n_x, int n_u, int n_lam, int x_pad, double *out) {
    export_gen_node(T, D, n_x, n_u, n_lam, x_pad, out, blockIdx.x, threadIdx.x);
}

/* ---- KKT residuals of a point, evaluated where the data is (tqgpu_kkt_residual*; tree_qp_out_calculate_KKT_res, tree_qp_common.c:540-788) ----
 * The point comes as pointers in the flat user layout of tqgpu_get_solution (no phantom root states; a null multiplier array is all
 * zeros), so the same kernels serve Export::d + Gen::mu and the scratch buffer of tqgpu_kkt_residual_at. */
struct KktPoint { const double *x, *u, *lam, *mu_x, *mu_u, *mu_d; };
constexpr int KKT_CLASSES = 6;
constexpr int KKT_HEAD = 10;      /* doubles in front of the per-node table: six maxima, six ints (the nodes), one pad */
static_assert(sizeof(MpcRoot::cert) == sizeof(double) * KKT_HEAD, "the certificate of a step is the head of the KKT result block");

__device__ __forceinline__ double kkt_viol(double v, double lo, double hi) { return v > hi ? v - hi : v < lo ? lo - v : (v != v ? v : 0.0); }
/* a multiplier that is exactly zero contributes zero whatever the bound (the reference's 0 * inf is NaN) */
__device__ __forceinline__ double kkt_compl(double mu, double v, double lo, double hi) { return mu == 0.0 ? 0.0 : mu > 0.0 ? mu * (v - hi) : mu * (lo - v); }
/* entry j of [x | u] of a node; phantom root states are zero and belong to no class */
__device__ __forceinline__ double kkt_z(const KktPoint &P, int j, int nxn, int xo, int uo, int pad, int x_pad) {
    return j < nxn ? (j < pad ? 0.0 : P.x[xo + j - x_pad]) : P.u[uo + j - nxn];
}

/* One wave per node: lane j owns entry j of [x | u], then of the rows, striding by 64 on larger nodes.  Per class the largest absolute
 * entry of the node, NaN kept (nanmax / wmax), goes to table[6 k + class]; -1 where the node has no entry of the class.  Nodes of kind 1
 * ignore their bounds (entries 0); rows count on nodes of kind 3 only. */
__device__ __forceinline__ void kkt_node(const Tree &T, const Data &D, int x_pad, const KktPoint &P, double *table, int k, int lane) {
    const int nxk = T.nx[k], nuk = T.nu[k], nz = nxk + nuk, xo = T.xoff[k], uo = T.uoff[k], nx0 = T.nx0;
    const int pad = k == 0 ? x_pad : 0;
    const int kind = D.dense ? D.kind[k] : 0;
    const int nc = kind == 3 ? D.gen->nc[k] : 0, ro = kind == 3 ? D.gen->roff[k] : 0;
    const double *Gt = kind == 3 ? D.gen->Gt + D.gen->goff[k] : nullptr;
    const double *H = kind ? D.Hd + D.poff[k] : nullptr;
    double m[KKT_CLASSES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    for (int j = lane; j < nz; j += WAVE) {
        if (j < pad) continue;
        const bool isx = j < nxk;
        const int jj = isx ? j : j - nxk;
        const double zj = kkt_z(P, j, nxk, xo, uo, pad, x_pad);
        const double mu = isx ? (P.mu_x ? P.mu_x[xo + j - x_pad] : 0.0) : (P.mu_u ? P.mu_u[uo + jj] : 0.0);
        /* stationarity: H z + h + mu + G' mu_d - lam_k + sum over the children of [A B]' lam_kid (column j of A / B is contiguous) */
        double acc = 0.0;
        if (kind) for (int i = 0; i < nz; i++) acc = fma(H[j + (size_t)i * nz], kkt_z(P, i, nxk, xo, uo, pad, x_pad), acc);
        else acc = (isx ? D.Qd[xo + j] : D.Rd[uo + jj]) * zj;
        acc += isx ? D.q[xo + j] : D.r[uo + jj];
        acc += mu;
        for (int r = 0; r < nc; r++) acc = fma(Gt[(size_t)r * nz + j], P.mu_d ? P.mu_d[ro + r] : 0.0, acc);
        if (k > 0 && isx) acc -= P.lam[xo - nx0 + j];
        for (int c = 0; c < T.nk[k]; c++) {
            const int kid = T.kid0[k] + c, nxc = T.nx[kid];
            const double *col = isx ? D.A + T.aoff[kid] + (size_t)j * nxc : D.B + T.boff[kid] + (size_t)jj * nxc;
            const double *lk = P.lam + T.xoff[kid] - nx0;
            for (int i = 0; i < nxc; i++) acc = fma(col[i], lk[i], acc);
        }
        m[TQGPU_KKT_STAT] = nanmax(m[TQGPU_KKT_STAT], fabs(acc));
        /* bounds: violation and complementarity */
        if (kind != 1) {
            const double lo = isx ? D.xmin[xo + j] : D.umin[uo + jj], hi = isx ? D.xmax[xo + j] : D.umax[uo + jj];
            m[TQGPU_KKT_BFEAS] = nanmax(m[TQGPU_KKT_BFEAS], fabs(kkt_viol(zj, lo, hi)));
            m[TQGPU_KKT_BCOMPL] = nanmax(m[TQGPU_KKT_BCOMPL], fabs(kkt_compl(mu, zj, lo, hi)));
        }
    }
    /* dynamics: A x_dad + B u_dad + b - x_k */
    if (k > 0) {
        const int dad = T.dad[k], nxd = T.nx[dad], nud = T.nu[dad], xod = T.xoff[dad], uod = T.uoff[dad], padd = dad == 0 ? x_pad : 0;
        const double *A = D.A + T.aoff[k], *B = D.B + T.boff[k];
        for (int i = lane; i < nxk; i += WAVE) {
            double acc = 0.0;
            for (int j = padd; j < nxd; j++) acc = fma(A[i + (size_t)j * nxk], P.x[xod + j - x_pad], acc);
            for (int j = 0; j < nud; j++) acc = fma(B[i + (size_t)j * nxk], P.u[uod + j], acc);
            acc += D.b[xo + i];
            acc -= P.x[xo + i - x_pad];
            m[TQGPU_KKT_DYN] = nanmax(m[TQGPU_KKT_DYN], fabs(acc));
        }
    }
    /* rows: G z against [dmin, dmax], row r of G at Gt[r nz ..) */
    for (int r = lane; r < nc; r += WAVE) {
        double g = 0.0;
        for (int j = pad; j < nz; j++) g = fma(Gt[(size_t)r * nz + j], kkt_z(P, j, nxk, xo, uo, pad, x_pad), g);
        const double lo = D.gen->dmin[ro + r], hi = D.gen->dmax[ro + r], mu = P.mu_d ? P.mu_d[ro + r] : 0.0;
        m[TQGPU_KKT_GFEAS] = nanmax(m[TQGPU_KKT_GFEAS], fabs(kkt_viol(g, lo, hi)));
        m[TQGPU_KKT_GCOMPL] = nanmax(m[TQGPU_KKT_GCOMPL], fabs(kkt_compl(mu, g, lo, hi)));
    }
    const bool have_z = nz - pad > 0;
    const bool have[KKT_CLASSES] = {have_z, k > 0 && nxk > 0, have_z, have_z, nc > 0, nc > 0};
#pragma unroll
    for (int c = 0; c < KKT_CLASSES; c++) {
        const double v = wmax(m[c]);
        if (lane == 0) table[(size_t)KKT_CLASSES * k + c] = have[c] ? v : -1.0;
    }
}
__global__ void __launch_bounds__(WAVE) k_kkt(Tree T, Data D, int x_pad, KktPoint P, double *table) {
    kkt_node(T, D, x_pad, P, table, blockIdx.x, threadIdx.x);
}

/* (v, n) before (bv, bn): a NaN first, then the larger value, the lower node among equals; n < 0: nothing yet */
__device__ __forceinline__ bool kkt_before(double v, int n, double bv, int bn) {
    if (n < 0) return false;
    if (bn < 0) return true;
    const bool vn = v != v, bvn = bv != bv;
    if (vn || bvn) return vn && (!bvn || n < bn);
    return v > bv || (v == bv && n < bn);
}

/* One workgroup: the table's six columns to six maxima and the lowest nodes that attain them (head[0..6), ints at head + 6; node -1
 * and value 0 for a class without entries); the table's -1 marks become 0.  A fixed tree of comparisons, no atomics. */
__device__ __forceinline__ void kkt_max_columns(int Nn, double *table, double *head, double *sv, int *sn, int t) {
    int *node = reinterpret_cast<int *>(head + KKT_CLASSES);
    for (int c = 0; c < KKT_CLASSES; c++) {
        double bv = 0.0; int bn = -1;
        for (int k = t; k < Nn; k += 256) {
            const double v = table[(size_t)KKT_CLASSES * k + c];
            if (v < 0.0) { table[(size_t)KKT_CLASSES * k + c] = 0.0; continue; }
            if (kkt_before(v, k, bv, bn)) { bv = v; bn = k; }
        }
        sv[t] = bv; sn[t] = bn;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w && kkt_before(sv[t + w], sn[t + w], sv[t], sn[t])) { sv[t] = sv[t + w]; sn[t] = sn[t + w]; }
            __syncthreads();
        }
        if (t == 0) { head[c] = sn[0] < 0 ? 0.0 : sv[0]; node[c] = sn[0]; }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_kkt_max(int Nn, double *table, double *head) {
    __shared__ double sv[256];
    __shared__ int sn[256];
    kkt_max_columns(Nn, table, head, sv, sn, threadIdx.x);
}

/* ---- the same for a batch of mirrors in one launch each (tqgpu_kkt_residual_batch) ----
 * One descriptor per member, uploaded with every call: what the single launches pass as kernel arguments.  Every kernel below is the
 * single kernel's body (the __device__ functions above, so the arithmetic of a node is the same instruction for instruction) behind
 * a look-up of the member: blockIdx.y = member, blockIdx.x = what blockIdx.x is in the single launch.  The grid is as wide as the
 * largest member needs; a workgroup beyond its member's own extent, or of a member the kernel does not apply to, returns at once
 * and writes nothing. */
struct KItem {
    Tree T; Data D; KktPoint P;
    const double *lamc;            /* the current duals (lam0 or lam1, as the host knows after the solve) */
    double *d_out, *table, *head;  /* the member's export block and per-node table; its KKT_HEAD doubles in the batch's contiguous block of heads */
    int x_pad, nxe, nue, nl, nx0;  /* phantom root states; the export sizes (x without them, u, lam) */
    int needs_export, box, gen;    /* d_out is not packed yet (no export went out ahead); the tree has nodes of kind 2 / of kind 3 */
};
struct KHead { double v[KKT_HEAD]; };      /* six maxima, six ints, one pad: what k_kkt_max writes in front of a mirror's own table */
__global__ void __launch_bounds__(256) k_export_all_batch(const KItem *__restrict__ items) {
    const KItem &it = items[blockIdx.y];
    if (!it.needs_export) return;
    export_all_entry(blockIdx.x * blockDim.x + threadIdx.x, it.nxe, it.nue, it.nl, it.x_pad, it.nx0, it.D, it.lamc, it.d_out);
}
__global__ void __launch_bounds__(WAVE) k_export_box_batch(const KItem *__restrict__ items) {
    const KItem &it = items[blockIdx.y];
    if (!it.needs_export || !it.box || (int)blockIdx.x >= it.T.Nn) return;
    export_box_node(it.T, it.D, it.nxe, it.nue, it.nl, it.x_pad, it.d_out, blockIdx.x, threadIdx.x);
}
__global__ void __launch_bounds__(WAVE) k_export_gen_batch(const KItem *__restrict__ items) {
    const KItem &it = items[blockIdx.y];
    if (!it.needs_export || !it.gen || (int)blockIdx.x >= it.T.Nn) return;
    export_gen_node(it.T, it.D, it.nxe, it.nue, it.nl, it.x_pad, it.d_out, blockIdx.x, threadIdx.x);
}
/* one wave per (member, node) */
__global__ void __launch_bounds__(WAVE) k_kkt_batch(const KItem *__restrict__ items) {
    const KItem &it = items[blockIdx.y];
    if ((int)blockIdx.x >= it.T.Nn) return;
    kkt_node(it.T, it.D, it.x_pad, it.P, it.table, blockIdx.x, threadIdx.x);
}
/* one workgroup per member */
__global__ void __launch_bounds__(256) k_kkt_max_batch(const KItem *__restrict__ items) {
    __shared__ double sv[256];
    __shared__ int sn[256];
    const KItem &it = items[blockIdx.x];
    kkt_max_columns(it.T.Nn, it.table, it.head, sv, sn, threadIdx.x);
}

/* the sizes of the export block [x | u | lam | dlam | mu_x | mu_u]: x and mu_x without the phantom root states, u and mu_u, lam and dlam */
struct ExportSizes { int nxe, nue, nl; };
ExportSizes export_sizes(const tqgpu_solver *s) { return {s->sum_nx - s->x_pad, s->sum_nu, s->sum_lam}; }
/* launches of one export: k_export_all, and the box and row overlays where the tree has such nodes */
int export_launches(const tqgpu_solver *s) { return 1 + (s->sk.box ? 1 : 0) + (s->sk.gen ? 1 : 0); }

/* the buffers of tqgpu_kkt_residual*, on first use (most mirrors never ask): the result block, and with_point the scratch point of
 * tqgpu_kkt_residual_at, which grows when tqgpu_set_constraints has added rows since */
int setup_kkt(tqgpu_solver *s, bool with_point) {
    int rc;
    const size_t res_bytes = sizeof(double) * (KKT_HEAD + (size_t)KKT_CLASSES * s->Nn);
    if (!s->kkt.d && ((rc = s->mem.device(s->kkt.d, res_bytes, TQGPU_ENOMEM, "the KKT residuals")) || (rc = s->mem.host(s->kkt.h, res_bytes, "the host mirror of the KKT residuals"))))
        return rc;
    const ExportSizes z = export_sizes(s);
    const size_t need = 2 * (size_t)z.nxe + 2 * (size_t)z.nue + (size_t)z.nl + (size_t)s->rows.sum_nc;
    if (with_point && (!s->kkt.d_pt || need > s->kkt.pt_cap)) {
        s->mem.release(s->kkt.d_pt); s->mem.release(s->kkt.h_pt);
        s->kkt.pt_cap = 0;
        if ((rc = s->mem.device(s->kkt.d_pt, sizeof(double) * std::max<size_t>(need, 1), TQGPU_ENOMEM, "the point of tqgpu_kkt_residual_at")) ||
            (rc = s->mem.host(s->kkt.h_pt, sizeof(double) * std::max<size_t>(need, 1), "the host mirror of that point")))
            return rc;
        s->kkt.pt_cap = need;
    }
    return TQGPU_OK;
}

}  // namespace

/* export_launches(s) launches into Export::d, and the download into Export::h; download = false: the device block only (tqgpu_kkt_residual reads it there) */
static int enqueue_export(tqgpu_solver *s, const double *lamc, bool download) {
    const Data &D = s->D;
    const ExportSizes z = export_sizes(s);
    const int n = std::max(std::max(z.nxe, z.nue), std::max(z.nl, 1));
    hipLaunchKernelGGL(k_export_all, dim3((n + 255) / 256), dim3(256), 0, s->stream, z.nxe, z.nue, z.nl, s->x_pad, s->nx0, D, lamc, s->out.d);
    if (s->sk.box) hipLaunchKernelGGL(k_export_box, dim3(s->T.Nn), dim3(WAVE), 0, s->stream, s->T, D, z.nxe, z.nue, z.nl, s->x_pad, s->out.d);
    if (s->sk.gen) hipLaunchKernelGGL(k_export_gen, dim3(s->T.Nn), dim3(WAVE), 0, s->stream, s->T, D, z.nxe, z.nue, z.nl, s->x_pad, s->out.d);
    if (download) HIP_TRY(hipMemcpyAsync(s->out.h, s->out.d, sizeof(double) * std::max<size_t>(s->out.doubles, 1), hipMemcpyDeviceToHost, s->stream));
    return TQGPU_OK;
}

extern "C" int tqgpu_set_export_ahead(tqgpu_solver *s, int on) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    s->out.ahead = on != 0;
    s->out.invalidate();
    return TQGPU_OK;
}

extern "C" int tqgpu_get_solution(tqgpu_solver *s, double *x, double *u, double *lam, double *mu_x, double *mu_u, double *dlam) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const Data &D = s->D;
    /* one packing kernel, one download into pinned memory, one synchronisation (ordered behind the solve on the stream) */
    const double *lamc = s->h_ctrl->cur ? D.lam1 : D.lam0;
    const auto [nxe, nue, nl] = export_sizes(s);
    if (!s->out.valid) { int rce = enqueue_export(s, lamc); if (rce != TQGPU_OK) return rce; }      /* (else: went out behind the solve, tqgpu_set_export_ahead) */
    else if (s->out.dev_only) {          /* packed behind a certified tqgpu_mpc_step, not downloaded yet */
        HIP_TRY(hipMemcpyAsync(s->out.h, s->out.d, sizeof(double) * std::max<size_t>(s->out.doubles, 1), hipMemcpyDeviceToHost, st));
        s->out.packed_and_downloading();
    }
    HIP_TRY(hipStreamSynchronize(st));
    const double *ox = s->out.h, *ou = ox + nxe, *ol = ou + nue, *od = ol + nl, *omx = od + nl, *omu = omx + nxe;
    if (x && nxe > 0) memcpy(x, ox, sizeof(double) * (size_t)nxe);
    if (u && nue > 0) memcpy(u, ou, sizeof(double) * (size_t)nue);
    if (lam && nl > 0) memcpy(lam, ol, sizeof(double) * (size_t)nl);
    if (dlam && nl > 0) memcpy(dlam, od, sizeof(double) * (size_t)nl);
    if (mu_x && nxe > 0) memcpy(mu_x, omx, sizeof(double) * (size_t)nxe);
    if (mu_u && nue > 0) memcpy(mu_u, omu, sizeof(double) * (size_t)nue);
    return TQGPU_OK;
}

/* ---- KKT residuals on the device ---- */
namespace {
/* the two kernels and the download of the result block, on the mirror's stream; nothing is waited for */
int kkt_enqueue(tqgpu_solver *s, const KktPoint &P, bool per_node) {
    hipLaunchKernelGGL(k_kkt, dim3(s->T.Nn), dim3(WAVE), 0, s->stream, s->T, s->D, s->x_pad, P, s->kkt.d + KKT_HEAD);
    hipLaunchKernelGGL(k_kkt_max, dim3(1), dim3(256), 0, s->stream, s->T.Nn, s->kkt.d + KKT_HEAD, s->kkt.d);
    HIP_TRY(hipGetLastError());
    const size_t n = KKT_HEAD + (per_node ? (size_t)KKT_CLASSES * s->Nn : 0);
    HIP_TRY(hipMemcpyAsync(s->kkt.h, s->kkt.d, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    return TQGPU_OK;
}
void kkt_collect(const tqgpu_solver *s, double *res, int *node, double *per_node) {
    if (res) memcpy(res, s->kkt.h, sizeof(double) * KKT_CLASSES);
    if (node) memcpy(node, s->kkt.h + KKT_CLASSES, sizeof(int) * KKT_CLASSES);
    if (per_node) memcpy(per_node, s->kkt.h + KKT_HEAD, sizeof(double) * (size_t)KKT_CLASSES * s->Nn);
}
/* the point of a KKT check that reads the export block Export::d (and Gen::mu) */
KktPoint kkt_point_of_export(const tqgpu_solver *s) {
    const ExportSizes z = export_sizes(s);
    KktPoint P;
    P.x = s->out.d; P.u = P.x + z.nxe; P.lam = P.u + z.nue; P.mu_x = P.lam + 2 * (size_t)z.nl; P.mu_u = P.mu_x + z.nxe;
    P.mu_d = s->sk.gen ? s->rows.d_mu : nullptr;
    return P;
}
/* behind the solve of a certified tqgpu_mpc_step (setup_kkt has run): the packing into Export::d with the dual buffer the DEVICE calls current -- the
 * host's h_ctrl->cur is the last solve's while this one runs --, k_kkt, k_kkt_max and the download of the head; nothing is waited for */
int mpc_enqueue_certificate(tqgpu_solver *s) {
    int rc;
    if ((rc = enqueue_export(s, nullptr, false))) return rc;
    MPC_COUNT(launches, export_launches(s));
    if ((rc = kkt_enqueue(s, kkt_point_of_export(s), false))) return rc;
    MPC_COUNT(launches, 2); MPC_COUNT(copies, 1);
    return TQGPU_OK;
}
/* what every entry point refuses: a rank of a sharded solve holds a part of the solution and runs a part of the launches */
int kkt_refuse(const tqgpu_solver *s, const char *who) {
    if (!s) return fail(TQGPU_EINVAL, std::string(who) + ": null solver");
    if ((s->pshard.on || s->shard.on) && s->shard.nranks > 1)
        return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": this mirror is rank " + std::to_string(s->shard.rank) + " of a sharded solve; KKT residuals are evaluated on single-device mirrors");
    return TQGPU_OK;
}
/* the point of the last solve, where tqgpu_get_solution and tqgpu_get_mu_d read it: the export (enqueued here unless it went out ahead) and Gen::mu */
int kkt_enqueue_last(tqgpu_solver *s, bool per_node) {
    int rc;
    if (s->solve_no == 0) return fail(TQGPU_EINVAL, "tqgpu_kkt_residual: this mirror has not solved yet (tqgpu_kkt_residual_at takes any point)");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = setup_kkt(s, false))) return rc;
    if (!s->out.valid && (rc = enqueue_export(s, s->h_ctrl->cur ? s->D.lam1 : s->D.lam0, false))) return rc;
    return kkt_enqueue(s, kkt_point_of_export(s), per_node);
}
}  // namespace

extern "C" int tqgpu_kkt_residual(tqgpu_solver *s, double res[6], int node[6], double *per_node) {
    SETTLE(s);
    int rc;
    if ((rc = kkt_refuse(s, "tqgpu_kkt_residual")) || (rc = kkt_enqueue_last(s, per_node != nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    kkt_collect(s, res, node, per_node);
    return TQGPU_OK;
}

extern "C" int tqgpu_kkt_residual_at(tqgpu_solver *s, const double *x, const double *u, const double *lam, const double *mu_x, const double *mu_u,
                                     const double *mu_d, double res[6], int node[6], double *per_node) {
    SETTLE(s);
    int rc;
    if ((rc = kkt_refuse(s, "tqgpu_kkt_residual_at"))) return rc;
    if (!x || !u || !lam) return fail(TQGPU_EINVAL, "tqgpu_kkt_residual_at: x, u and lam are required");
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = setup_kkt(s, true))) return rc;
    /* the point through pinned memory in one copy; an array that was not given stays a null pointer for the kernel */
    const ExportSizes z = export_sizes(s);
    size_t off = 0;
    auto put = [&](const double *src, size_t n) -> const double * {
        if (!src) return nullptr;
        if (n) memcpy(s->kkt.h_pt + off, src, sizeof(double) * n);
        const double *d = s->kkt.d_pt + off;
        off += n;
        return d;
    };
    KktPoint P;
    P.x = put(x, z.nxe); P.u = put(u, z.nue); P.lam = put(lam, z.nl); P.mu_x = put(mu_x, z.nxe); P.mu_u = put(mu_u, z.nue); P.mu_d = put(mu_d, s->rows.sum_nc);
    if (off) HIP_TRY(hipMemcpyAsync(s->kkt.d_pt, s->kkt.h_pt, sizeof(double) * off, hipMemcpyHostToDevice, s->stream));
    if ((rc = kkt_enqueue(s, P, per_node != nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    kkt_collect(s, res, node, per_node);
    return TQGPU_OK;
}

/* ---- tqgpu_kkt_residual_batch: per device one group; a group of KKT_BATCH_MIN members or more goes out as ONE set of launches on
 * its first member's stream (the lead's), anything else member by member on the members' own streams ---- */
namespace {
struct KktBatchStats { int launches = 0, copies = 0, waits = 0, batched = 0; };
thread_local KktBatchStats g_kkt_stats;          /* of this thread's last tqgpu_kkt_residual_batch (tqgpu_kkt_batch_stats) */
constexpr int KKT_BATCH_MIN = 2;                 /* members of one device from which the batched route is taken: at 2 C1 trees it measured 37 us against 64 us member by member (profiles/r12_kkt_batch_timing.txt) */
constexpr size_t KKT_GRID_Y = 65535;             /* blockIdx.y is the member */

/* one member on its own stream: the route of tqgpu_kkt_residual without the wait */
int kkt_member_enqueue(tqgpu_solver *s, KktBatchStats &st) {
    if (s->links.settle_stream && s->links.settle_stream != s->stream) st.waits++;
    SETTLE(s);
    st.launches += (s->out.valid ? 0 : export_launches(s)) + 2;
    st.copies++;
    return kkt_enqueue_last(s, false);
}

/* A group on its lead's stream: the descriptors in one copy, the packing of the members that have not exported ahead (k_export_all_batch,
 * and the box and row overlays where some member has such nodes), k_kkt_batch, k_kkt_max_batch, the heads in one copy.  Nothing is
 * waited for here in the steady state -- a loop of tqgpu_solve_batch and this call on the same members -- where every member's solve
 * was part of a launch on this very stream (settle_stream), as in join_lead_stream.  A member's own stream is waited for only where it
 * may hold work this stream has not seen: uploads (stream_pending), an export that went out ahead, or a solve of its own that returned
 * on its verdict (a single launch may still write its state back then): order_behind_lead, KKT_ORDER. */
int kkt_group_enqueue(tqgpu_solver **v, const DeviceGroup &g, KktBatchStats &st) {
    tqgpu_solver *lead = v[g.idx[0]];
    const size_t n = g.idx.size();
    int rc;
    HIP_TRY(hipSetDevice(lead->device));
    for (int i : g.idx) if ((rc = setup_kkt(v[i], false))) return rc;
    if ((rc = grow_items(lead, lead->kkt.d_items, lead->kkt.h_items, lead->kkt.items_cap, n)) || (rc = grow_items(lead, lead->kkt.d_heads, lead->kkt.h_heads, lead->kkt.heads_cap, n))) return rc;
    int nn_all = 0, nn_box = 0, nn_gen = 0, cells = 0;          /* widths of the four grids (0: no launch) */
    std::vector<hipStream_t> waited;
    for (size_t m = 0; m < n; m++) {
        tqgpu_solver *s = v[g.idx[m]];
        if ((rc = order_behind_lead(s, lead, s->kkt.drained_at, KKT_ORDER, waited, st.waits))) return rc;
        KItem &it = lead->kkt.h_items[m];
        it.T = s->T; it.D = s->D;
        const ExportSizes z = export_sizes(s);
        it.x_pad = s->x_pad; it.nxe = z.nxe; it.nue = z.nue; it.nl = z.nl; it.nx0 = s->nx0;
        it.lamc = s->h_ctrl->cur ? s->D.lam1 : s->D.lam0;
        it.d_out = s->out.d; it.table = s->kkt.d + KKT_HEAD; it.head = lead->kkt.d_heads[m].v;
        it.P = kkt_point_of_export(s);
        it.needs_export = s->out.valid ? 0 : 1; it.box = s->sk.box ? 1 : 0; it.gen = s->sk.gen ? 1 : 0;
        nn_all = std::max(nn_all, s->T.Nn);
        if (it.needs_export) {
            cells = std::max(cells, std::max(std::max(it.nxe, it.nue), std::max(it.nl, 1)));
            if (it.box) nn_box = std::max(nn_box, s->T.Nn);
            if (it.gen) nn_gen = std::max(nn_gen, s->T.Nn);
        }
    }
    hipStream_t ls = lead->stream;
    const unsigned ny = (unsigned)n;
    HIP_TRY(hipMemcpyAsync(lead->kkt.d_items, lead->kkt.h_items, n * sizeof(KItem), hipMemcpyHostToDevice, ls)); st.copies++;
    if (cells) { hipLaunchKernelGGL(k_export_all_batch, dim3((unsigned)((cells + 255) / 256), ny), dim3(256), 0, ls, lead->kkt.d_items); st.launches++; }
    if (nn_box) { hipLaunchKernelGGL(k_export_box_batch, dim3((unsigned)nn_box, ny), dim3(WAVE), 0, ls, lead->kkt.d_items); st.launches++; }
    if (nn_gen) { hipLaunchKernelGGL(k_export_gen_batch, dim3((unsigned)nn_gen, ny), dim3(WAVE), 0, ls, lead->kkt.d_items); st.launches++; }
    hipLaunchKernelGGL(k_kkt_batch, dim3((unsigned)nn_all, ny), dim3(WAVE), 0, ls, lead->kkt.d_items); st.launches++;
    hipLaunchKernelGGL(k_kkt_max_batch, dim3(ny), dim3(256), 0, ls, lead->kkt.d_items); st.launches++;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lead->kkt.h_heads, lead->kkt.d_heads, n * sizeof(KHead), hipMemcpyDeviceToHost, ls)); st.copies++;
    st.batched += (int)n;
    return TQGPU_OK;
}
}  // namespace

/* Everything goes out before the first wait.  The members' Export::d is packed afterwards, their Export::h is not: Export::valid stays as it
 * was, so tqgpu_get_solution packs and downloads as it does behind tqgpu_kkt_residual. */
extern "C" int tqgpu_kkt_residual_batch(tqgpu_solver **solvers, int n, double *res, int *node) {
    if (!solvers || n < 0 || (n > 0 && !res)) return fail(TQGPU_EINVAL, "tqgpu_kkt_residual_batch: bad arguments");
    int rc;
    for (int i = 0; i < n; i++) {
        if ((rc = kkt_refuse(solvers[i], "tqgpu_kkt_residual_batch"))) return rc;
        if (solvers[i]->solve_no == 0) return fail(TQGPU_EINVAL, "tqgpu_kkt_residual_batch: member " + std::to_string(i) + " has not solved yet");
    }
    KktBatchStats &st = g_kkt_stats;
    st = KktBatchStats();
    /* a mirror named twice is not refused: its group goes member by member (group_fits_one_grid).  The waits are this call's own to count, and a member
     * that goes alone is only enqueued in the first phase and waited for with the others in the second */
    const std::vector<DeviceGroup> groups = plan_device_groups(solvers, n, "TREEQP_AMD_KKT_BATCH", KKT_BATCH_MIN, KKT_GRID_Y);
    return run_device_groups(solvers, groups, GroupRun{true, true, &st.waits},
        [&](const DeviceGroup &g, size_t) { return kkt_group_enqueue(solvers, g, st); },
        [&](int i) { return kkt_member_enqueue(solvers[i], st); },
        [&](const DeviceGroup &g, size_t) {
            for (size_t m = 0; m < g.idx.size(); m++) {
                const int i = g.idx[m];
                if (!g.batched) { HIP_TRY(hipStreamSynchronize(solvers[i]->stream)); st.waits++; kkt_collect(solvers[i], res + (size_t)KKT_CLASSES * i, node ? node + (size_t)KKT_CLASSES * i : nullptr, nullptr); continue; }
                const double *h = solvers[g.idx[0]]->kkt.h_heads[m].v;
                memcpy(res + (size_t)KKT_CLASSES * i, h, sizeof(double) * KKT_CLASSES);
                if (node) memcpy(node + (size_t)KKT_CLASSES * i, h + KKT_CLASSES, sizeof(int) * KKT_CLASSES);
            }
            return TQGPU_OK;
        });
}

extern "C" int tqgpu_kkt_batch_stats(int *launches, int *copies, int *waits, int *batched_members) {
    const KktBatchStats &st = g_kkt_stats;
    if (launches) *launches = st.launches;
    if (copies) *copies = st.copies;
    if (waits) *waits = st.waits;
    if (batched_members) *batched_members = st.batched;
    return TQGPU_OK;
}

/*
 * tdunes_adjoint.hpp -- the host side of the derivatives of an MPC step, in the host part: the entry points tqgpu_mpc_sensitivity, tqgpu_mpc_adjoint,
 * tqgpu_mpc_adjoint_batch, tqgpu_mpc_sensitivity_batch, tqgpu_mpc_set_param_groups / _get_param_groups, tqgpu_mpc_adjoint_matrices, _batch, tqgpu_mpc_adjoint_bounds,
 * tqgpu_mpc_adjoint_reference, tqgpu_mpc_tangent, tqgpu_mpc_predict_at, and the readers tqgpu_mpc_get_gain, _get_sensitivities, _predict, _predict_batch, _get_adjoint*, _get_tangent*. Their kernels are tdunes_sens.hpp's (part TQP_SENS); k_adj_export_batch is the one kernel here.
 * Included once from tdunes_device.hip inside #if TQ_HAS(TQP_HOST), behind tdunes_mpc.hpp (mpc_refuse, mpc_take_x0, MpcLive) and tdunes_kkt.hpp
 * (enqueue_export, export_all_entry).  tdunes_mirror.hpp keeps the mirror's records MpcSens, MpcTan, MpcAdjBatch, MpcAdjMat, tdunes_device.hip the plan and the driver of a
 * batched call (refuse_members, member_spans, plan_device_groups, order_behind_lead, run_device_groups): each of the four batched calls here is its refusals, its offsets and
 * three callbacks (a group out, a member alone, a group back).  What the adjoint's and the sensitivity's groups share is DerivGroup (deriv_group_fill,
 * deriv_group_launch_factor); a further batched derivative fills its own fields of the items between the two and adds its launches behind them.
 */
#pragma once

/* ---- parametric sensitivities of an MPC step (tdunes_sens.hpp): du0/dx0, dz/dx0, dlam/dx0 at the point of the last solve ---- */
namespace {
/* one launch per level of the tree, launch(first node, nodes): to_root walks every level, deepest first; to_leaves walks levels 1 .. Nh - 1 */
enum class Walk { to_root, to_leaves };
template <typename F>
void for_levels(const tqgpu_solver *s, Walk dir, F launch) {
    const bool up = dir == Walk::to_root;
    for (int lvl = up ? s->T.Nh - 1 : 1; up ? lvl >= 0 : lvl < s->T.Nh; lvl += up ? -1 : 1) {
        const int first = s->lvl_first[lvl];
        launch(first, s->lvl_first[lvl + 1] - first);
    }
}
size_t sens_head_doubles(const tqgpu_solver *s) { return (size_t)s->nu[0] * s->sens.nx0 + (size_t)s->nu[0] + (size_t)s->sens.nx0 + 1; }

/* the LDS windows of k_sens_factor (lf) and k_sens_primal (lp), refused where one does not fit; touches nothing */
int sens_window_refuse(const tqgpu_solver *s, size_t &lf, size_t &lp) {
    const size_t nx0 = (size_t)s->mpc.nx0;
    lf = lp = 0;
    for (int k = 0; k < s->Nn; k++) {
        lp = std::max(lp, ((size_t)(s->nx[k] + s->nu[k]) * nx0 + 2) * sizeof(double));
        if (k < s->Np) {
            const size_t d = (size_t)s->bdim[k], R = d + (k > 0 ? (size_t)s->nx[k] : nx0), ld = R | 1;
            lf = std::max(lf, (ld * d + d + 2) * sizeof(double));
        }
    }
    if (lf > 160 * 1024 || lp > 160 * 1024)
        return fail(TQGPU_EUNSUPPORTED, "tqgpu_mpc_sensitivity: the tall root block [W; G'] (or a node's nz x nx0 window) does not fit 160 KiB of LDS");
    return TQGPU_OK;
}
/* the feature's buffers, on first use and again when nx0 changed: one zeroed device block, the pinned block, the LDS windows */
int setup_sens(tqgpu_solver *s) {
    int rc;
    const size_t nx0 = (size_t)s->mpc.nx0, nu0 = (size_t)s->nu[0], snx = (size_t)s->sum_nx, snu = (size_t)s->sum_nu;
    size_t lf = 0, lp = 0;
    if ((rc = sens_window_refuse(s, lf, lp))) return rc;
    if (s->sens.d && s->sens.nx0 == s->mpc.nx0) return TQGPU_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->mem.release(s->sens.d); s->mem.release(s->sens.h);
    s->sens.invalidate(); s->sens.nx0 = 0;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 1) / 2 * 2; return o; };
    const size_t oW = take(s->sum_W), oUt = take(s->sum_Ut), oCW = take(s->sum_W), oCUt = take(s->sum_Ut), oiv = take(snx), oPx = take(snx), oPu = take(snu);
    const size_t oG = take((size_t)s->bdim[0] * nx0), odl = take(snx * nx0), odx = take(snx * nx0), odu = take(snu * nx0);
    const size_t head = nu0 * nx0 + nu0 + nx0 + 1, oh = take(head), onr = take(2);
    if ((rc = s->mem.zeroed(s->sens.d, sizeof(double) * std::max<size_t>(off, 2), TQGPU_ENOMEM, "the sensitivities")) ||
        (rc = s->mem.host(s->sens.h, sizeof(double) * (head + nx0 + nu0 + 2), "the pinned gain")))
        return rc;
    memset(s->sens.h, 0, sizeof(double) * (head + nx0 + nu0 + 2));
    if ((rc = allow_lds(k_sens_hess, s->pp.lds_hess)) || (rc = allow_lds(k_sens_factor, lf)) || (rc = allow_lds(k_sens_forward, s->pp.lds_forward)) || (rc = allow_lds(k_sens_primal, lp)))
        return rc;
    Sens &S = s->sens.v;
    S = Sens{};
    double *p = s->sens.d;
    S.W = p + oW; S.Ut = p + oUt; S.CholW = p + oCW; S.CholUt = p + oCUt; S.invd = p + oiv; S.Px = p + oPx; S.Pu = p + oPu;
    S.G = p + oG; S.dlam = p + odl; S.dx = p + odx; S.du = p + odu; S.head = p + oh; S.n_reg = reinterpret_cast<int *>(p + onr);
    S.nx0 = s->mpc.nx0; S.xpad = s->x_pad; S.sum_nx = s->sum_nx; S.sum_nu = s->sum_nu; S.nu0 = s->nu[0];
    s->sens.nx0 = s->mpc.nx0; s->sens.lds_factor = lf; s->sens.lds_primal = lp;
    return TQGPU_OK;
}
int sens_need(const tqgpu_solver *s, const char *who) {
    if (!s->sens.valid) return fail(TQGPU_EINVAL, std::string(who) + ": no sensitivity has been computed for the point and the data the device holds now (tqgpu_mpc_sensitivity after the last solve, upload and fold)");
    return TQGPU_OK;
}
/* what tqgpu_mpc_sensitivity and tqgpu_mpc_adjoint refuse alike, before anything is touched */
int sens_refuse(tqgpu_solver *s, const tqgpu_opts *o, const char *who) {
    int rc;
    if ((rc = mpc_refuse(s, who))) return rc;
    if (!o) return fail(TQGPU_EINVAL, std::string(who) + ": opts is required (the regularisation rule of the factorisation)");
    if ((rc = mpc_take_x0(s, nullptr, who))) return rc;          /* no root form declared yet, and what a fold would refuse */
    if (s->solve_no == 0) return fail(TQGPU_EINVAL, std::string(who) + ": this mirror has not solved yet: there is no point to differentiate at");
    if (s->sens.dirty)
        return fail(TQGPU_EINVAL, std::string(who) + ": the problem was changed (an upload, an x0 fold or a window move) since the last solve: its point does not belong to the data the device holds now; solve first");
    for (int k = 0; k < s->Nn; k++) if (s->sk.kind(k) >= 2)
        return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": the tree has nodes of kind 2 or 3: Pd need not belong to the final working set after a line search's last trial");
    return TQGPU_OK;
}
/* the view a factorisation takes and leaves behind: the feature's buffers (setup_sens) with the point in the export block, the root form, x0 */
Sens sens_view_of_point(const tqgpu_solver *s) {
    Sens S = s->sens.v;
    S.x = s->out.d; S.u = S.x + export_sizes(s).nxe;
    S.root_states = s->mpc.states ? 1 : 0;
    if (s->mpc.d) { S.A0 = s->mpc.d; S.S0 = s->mpc.S0 ? s->mpc.d + (size_t)s->mpc.nb * s->mpc.nx0 + s->mpc.nb : nullptr; }
    S.x0 = s->mpc.h;
    return S;
}
/* P, W, Ut, G and the factor of the point the device holds, into the feature's buffers: the packing of the point where it has not gone
 * out, k_sens_hess, k_sens_factor per block level, deepest first.  Returns the view the later kernels take (kept in sens.v by the caller) */
int sens_enqueue_factor(tqgpu_solver *s, const Opts &O, Sens &S) {
    int rc;
    if (!s->out.valid) {
        if ((rc = enqueue_export(s, s->h_ctrl->cur ? s->D.lam1 : s->D.lam0, false))) return rc;
        MPC_COUNT(launches, 1);
    }
    S = sens_view_of_point(s);
    const Tree &T = s->T;
    hipLaunchKernelGGL(k_sens_hess, dim3(T.Np), dim3(WAVE), s->pp.lds_hess, s->stream, T, s->D, S);
    for_levels(s, Walk::to_root, [&](int first, int count) { hipLaunchKernelGGL(k_sens_factor, dim3(count), dim3(WAVE), s->sens.lds_factor, s->stream, T, O, S, first); });
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1 + T.Nh);
    return TQGPU_OK;
}

/* the adjoint's buffers, on first use and again when nw grows (or nx0 changed): one zeroed device block, the pinned block, the LDS windows.
 * Refuses, before anything is touched, an nw whose nz x nw window would not fit the 160 KiB setup_sens allows an nz x nx0 window */
int adj_window_refuse(const tqgpu_solver *s, int nw) {
    for (int k = 0; k < s->Nn; k++)
        if (((size_t)(s->nx[k] + s->nu[k]) * (size_t)nw + 2) * sizeof(double) > 160 * 1024)
            return fail(TQGPU_EUNSUPPORTED, "tqgpu_mpc_adjoint: a node's nz x nw window does not fit 160 KiB of LDS");
    return TQGPU_OK;
}
size_t adj_w_doubles(const tqgpu_solver *s, int nw) { return ((size_t)(s->sum_nx - s->x_pad) + (size_t)s->sum_nu) * (size_t)nw; }
int setup_adj(tqgpu_solver *s, int nw) {
    int rc;
    MpcSens &m = s->sens;
    const size_t snx = (size_t)s->sum_nx, snu = (size_t)s->sum_nu, nxe = snx - (size_t)s->x_pad, nx0 = (size_t)s->mpc.nx0;
    if (!m.ad || nw > m.nw_cap || m.adj_nx0 != s->mpc.nx0) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->mem.release(m.ad); s->mem.release(m.ah);
        m.adj_valid = false; m.nw_cap = 0;
        const size_t cap = (size_t)nw;
        size_t off = 0;
        auto take = [&](size_t n) { const size_t o = off; off += (n + 1) / 2 * 2; return o; };
        const size_t ow = take((nxe + snu) * cap), oY = take(snx * cap), ot = take(snx * cap), oq = take(snx * cap), or_ = take(snu * cap), ob = take(snx * cap), oh = take(nx0 * cap + 1),
                     olx = take(snx * cap), oux = take(snx * cap), olu = take(snu * cap), ouu = take(snu * cap);
        if ((rc = s->mem.zeroed(m.ad, sizeof(double) * std::max<size_t>(off, 2), TQGPU_ENOMEM, "the adjoint")) ||
            (rc = s->mem.host(m.ah, sizeof(double) * ((nxe + snu) * cap + nx0 * cap + 2), "the pinned loss gradient and gx0")))
            return rc;
        memset(m.ah, 0, sizeof(double) * ((nxe + snu) * cap + nx0 * cap + 2));
        size_t lr = 0, lg = 0;
        for (int k = 0; k < s->Nn; k++) {
            const size_t nz = (size_t)(s->nx[k] + s->nu[k]);
            lr = std::max(lr, (nz + 2) * sizeof(double)); lg = std::max(lg, (2 * nz + 2) * sizeof(double));
        }
        if ((rc = allow_lds(k_adj_rhs, lr)) || (rc = allow_lds(k_adj_backward, s->pp.lds_forward)) || (rc = allow_lds(k_adj_forward, s->pp.lds_forward)) || (rc = allow_lds(k_adj_grad, lg)))
            return rc;
        Adj &A = m.a;
        A = Adj{};
        double *p = m.ad;
        A.wx = p + ow; A.Y = p + oY; A.t = p + ot; A.gq = p + oq; A.gr = p + or_; A.gb = p + ob; A.head = p + oh;
        A.glx = p + olx; A.gux = p + oux; A.glu = p + olu; A.guu = p + ouu;
        A.nxe = (int)nxe;
        m.nw_cap = nw; m.adj_nx0 = s->mpc.nx0; m.lds_rhs = lr; m.lds_grad = lg;
    }
    /* the columns of this call: wu lies behind the nw columns of wx */
    m.a.nw = nw;
    m.a.wu = m.a.wx + nxe * (size_t)nw;
    return TQGPU_OK;
}
int adj_need(const tqgpu_solver *s, const char *who) {
    if (!s->sens.adj_valid) return fail(TQGPU_EINVAL, std::string(who) + ": no adjoint has been computed for the point and the data the device holds now (tqgpu_mpc_adjoint after the last solve, upload and fold)");
    return TQGPU_OK;
}
/* a diagnostic download (a whole buffer through pageable memory, repacked on the host; not counted into tqgpu_mpc_stats): `cols` columns of sum_nx
 * doubles at d, of each the n entries behind the first `skip`, packed into out */
int download_columns(const tqgpu_solver *s, const double *d, size_t cols, size_t skip, size_t n, double *out) {
    const size_t snx = (size_t)s->sum_nx;
    std::vector<double> tmp(snx * cols + 1);
    HIP_TRY(hipMemcpy(tmp.data(), d, sizeof(double) * snx * cols, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < cols; j++) if (n) memcpy(out + j * n, tmp.data() + j * snx + skip, sizeof(double) * n);
    return TQGPU_OK;
}
/* w of one mirror into a pinned block: [wx | wu], a missing part as zeros */
void adj_stage_w(const tqgpu_solver *s, double *h, const double *wx, const double *wu, int nw) {
    const size_t nx = (size_t)(s->sum_nx - s->x_pad) * nw, nu = (size_t)s->sum_nu * nw;
    if (wx) memcpy(h, wx, sizeof(double) * nx); else memset(h, 0, sizeof(double) * nx);
    if (wu) memcpy(h + nx, wu, sizeof(double) * nu); else memset(h + nx, 0, sizeof(double) * nu);
}
/* a finished adjoint onto its mirror, behind the wait: the head h, [gx0 | n_reg], goes behind w in the pinned block, where tqgpu_mpc_get_adjoint_x0
 * reads it (the single route downloads it there: h is that place), and to the caller's gx0 and n_reg; S is the view the launches took, the factor
 * in it (factored was true already where they did not factorise).  valid stays as it was: a stored sensitivity was not touched, a missing one
 * is still missing (dlam, dZ and the head of this point have not been computed) */
void adj_store(tqgpu_solver *s, const Sens &S, const double *h, int nw, double *gx0, int *n_reg) {
    MpcSens &ms = s->sens;
    const size_t head = (size_t)ms.nx0 * nw + 1;
    double *behind_w = ms.ah + adj_w_doubles(s, nw);
    if (h != behind_w) memcpy(behind_w, h, sizeof(double) * head);
    if (gx0) memcpy(gx0, h, sizeof(double) * (head - 1));
    if (n_reg) *n_reg = (int)h[head - 1];
    ms.v = S; ms.factored = true; ms.nw = nw; ms.adj_valid = true;
}
}  // namespace

/* one mirror on its own stream, behind the refusals that touch nothing; counted into whatever record is live (tqgpu_mpc_sensitivity's own, or that of a
 * tqgpu_mpc_sensitivity_batch that goes member by member) */
static int mpc_sensitivity_one(tqgpu_solver *s, const Opts &O, int *n_reg) {
    int rc;
    if ((rc = setup_sens(s))) return rc;
    s->sens.valid = s->sens.factored = false;
    Sens S;
    if ((rc = sens_enqueue_factor(s, O, S))) return rc;
    const Tree &T = s->T;
    hipStream_t st = s->stream;
    for_levels(s, Walk::to_leaves, [&](int first, int count) { hipLaunchKernelGGL(k_sens_forward, dim3(count, (unsigned)s->sens.nx0), dim3(WAVE), s->pp.lds_forward, st, T, S, first); });
    hipLaunchKernelGGL(k_sens_primal, dim3(T.Nn), dim3(WAVE), s->sens.lds_primal, st, T, s->D, S);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, (T.Nh - 1) + 1);
    const size_t head = sens_head_doubles(s);
    HIP_TRY(hipMemcpyAsync(s->sens.h, S.head, sizeof(double) * head, hipMemcpyDeviceToHost, st)); MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    s->sens.v = S;
    s->sens.valid = s->sens.factored = true;
    if (n_reg) *n_reg = (int)s->sens.h[head - 1];
    return TQGPU_OK;
}
extern "C" int tqgpu_mpc_sensitivity(tqgpu_solver *s, const tqgpu_opts *o, int *n_reg) {
    const char *who = "tqgpu_mpc_sensitivity";
    int rc;
    if ((rc = sens_refuse(s, o, who))) return rc;
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    return mpc_sensitivity_one(s, O, n_reg);
}

/* ---- the adjoint of an MPC step (tdunes_sens.hpp): dL/dq, dL/dr, dL/db, dL/dx0 for w = dL/dz at the point of the last solve ---- */
/* one mirror on its own stream, behind the refusals that touch nothing; counted into whatever record is live (tqgpu_mpc_adjoint's own, or that of a
 * tqgpu_mpc_adjoint_batch that goes member by member) */
static int mpc_adjoint_one(tqgpu_solver *s, const Opts &O, const double *wx, const double *wu, int nw, double *gx0, int *n_reg) {
    int rc;
    if ((rc = adj_window_refuse(s, nw)) || (rc = setup_sens(s)) || (rc = setup_adj(s, nw))) return rc;
    s->sens.adj_valid = false;
    MpcSens &m = s->sens;
    const size_t nwd = adj_w_doubles(s, nw), nx0 = (size_t)m.nx0;
    hipStream_t st = s->stream;
    adj_stage_w(s, m.ah, wx, wu, nw);          /* w through pinned memory in one copy */
    if (nwd) { HIP_TRY(hipMemcpyAsync(const_cast<double *>(m.a.wx), m.ah, sizeof(double) * nwd, hipMemcpyHostToDevice, st)); }
    MPC_COUNT(copies, 1);
    Sens S = m.v;
    if (!m.factored && (rc = sens_enqueue_factor(s, O, S))) return rc;
    const Tree &T = s->T;
    const Adj A = m.a;
    const unsigned cols = (unsigned)nw;
    hipLaunchKernelGGL(k_adj_rhs, dim3(T.Np, cols), dim3(WAVE), m.lds_rhs, st, T, s->D, S, A);
    for_levels(s, Walk::to_root, [&](int first, int count) { hipLaunchKernelGGL(k_adj_backward, dim3(count, cols), dim3(WAVE), s->pp.lds_forward, st, T, S, A, first); });
    for_levels(s, Walk::to_leaves, [&](int first, int count) { hipLaunchKernelGGL(k_adj_forward, dim3(count, cols), dim3(WAVE), s->pp.lds_forward, st, T, S, A, first); });
    hipLaunchKernelGGL(k_adj_grad, dim3(T.Nn, cols), dim3(WAVE), m.lds_grad, st, T, s->D, S, A);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1 + T.Nh + (T.Nh - 1) + 1);
    double *hh = m.ah + nwd;
    HIP_TRY(hipMemcpyAsync(hh, A.head, sizeof(double) * (nx0 * nw + 1), hipMemcpyDeviceToHost, st)); MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    adj_store(s, S, hh, nw, gx0, n_reg);
    return TQGPU_OK;
}
extern "C" int tqgpu_mpc_adjoint(tqgpu_solver *s, const tqgpu_opts *o, const double *wx, const double *wu, int nw, int *n_reg) {
    const char *who = "tqgpu_mpc_adjoint";
    int rc;
    if ((rc = sens_refuse(s, o, who))) return rc;
    if (nw < 1) return fail(TQGPU_EINVAL, std::string(who) + ": nw must be at least 1");
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    return mpc_adjoint_one(s, O, wx, wu, nw, nullptr, n_reg);
}

extern "C" int tqgpu_mpc_get_adjoint_x0(tqgpu_solver *s, double *gx0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_adjoint_x0")) || (rc = adj_need(s, "tqgpu_mpc_get_adjoint_x0"))) return rc;
    const size_t n = (size_t)s->sens.nx0 * (size_t)s->sens.nw;
    if (gx0 && n) memcpy(gx0, s->sens.ah + adj_w_doubles(s, s->sens.nw), sizeof(double) * n);
    return TQGPU_OK;
}

/* a diagnostic download (whole buffers through pageable memory, repacked on the host): not counted into tqgpu_mpc_stats */
extern "C" int tqgpu_mpc_get_adjoint(tqgpu_solver *s, double *gq, double *gr, double *gb) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_adjoint")) || (rc = adj_need(s, "tqgpu_mpc_get_adjoint"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t nw = (size_t)s->sens.nw, snu = (size_t)s->sum_nu;
    if (gq && (rc = download_columns(s, s->sens.a.gq, nw, (size_t)s->x_pad, (size_t)(s->sum_nx - s->x_pad), gq))) return rc;      /* phantom root states are left out */
    if (gb && (rc = download_columns(s, s->sens.a.gb, nw, (size_t)s->nx0, (size_t)s->sum_lam, gb))) return rc;                      /* the root has no dual */
    if (gr && snu * nw) HIP_TRY(hipMemcpy(gr, s->sens.a.gr, sizeof(double) * snu * nw, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* the bound gradients k_adj_grad left beside gq, gr: a diagnostic download like tqgpu_mpc_get_adjoint, not counted into tqgpu_mpc_stats */
extern "C" int tqgpu_mpc_get_adjoint_bounds(tqgpu_solver *s, double *gxmin, double *gxmax, double *gumin, double *gumax) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_adjoint_bounds")) || (rc = adj_need(s, "tqgpu_mpc_get_adjoint_bounds"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t nw = (size_t)s->sens.nw, snu = (size_t)s->sum_nu, pad = (size_t)s->x_pad, nxe = (size_t)s->sum_nx - pad;
    const Adj &A = s->sens.a;
    if (gxmin && (rc = download_columns(s, A.glx, nw, pad, nxe, gxmin))) return rc;      /* phantom root states are left out */
    if (gxmax && (rc = download_columns(s, A.gux, nw, pad, nxe, gxmax))) return rc;
    if (gumin && snu * nw) HIP_TRY(hipMemcpy(gumin, A.glu, sizeof(double) * snu * nw, hipMemcpyDeviceToHost));
    if (gumax && snu * nw) HIP_TRY(hipMemcpy(gumax, A.guu, sizeof(double) * snu * nw, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* ---- tqgpu_mpc_adjoint_batch: per device one group; a group of ADJ_BATCH_MIN members or more goes out as ONE set of launches on its first
 * member's stream (the lead's), anything else member by member through mpc_adjoint_one ---- */
namespace {
constexpr int ADJ_BATCH_MIN = 2;                 /* members of one device from which the batched route is taken: at 2 C1 trees it measured 212 us against 417 us member by member, at 4 212 us against 809 us (profiles/r21_mpc_adjoint_batch.txt) */
constexpr size_t ADJ_GRID_Z = 65535;             /* blockIdx.z is the member */

/* the packing of the members' points: the body of k_export_all_batch over the adjoint's descriptor (kinds 2 and 3 are refused: no overlays) */
__global__ void __launch_bounds__(256) k_adj_export_batch(const AItem *__restrict__ items) {
    const AItem &it = items[blockIdx.y];
    if (!it.needs_export) return;
    export_all_entry(blockIdx.x * blockDim.x + threadIdx.x, it.nxe, it.nue, it.nl, it.x_pad, it.nx0, it.D, it.lamc, it.d_out);
}

/* ---- a batched group of derivatives on its lead's stream: what the adjoint's and the sensitivity's groups share.  deriv_group_fill: the descriptor block
 * (AItem per member, the level tables behind them) with everything in it that the packing, k_sens_hess_batch and k_sens_factor_batch read, every member
 * ordered behind the lead, the widths of the grids; deriv_group_launch_factor: the block up in one copy, then those launches.  A family adds its own fields
 * to the items between the two, and its own launches and the copy of the heads behind them ---- */
struct DerivGroup {
    AItem *items, *d_items;          /* the descriptors in the lead's pinned block and on the device */
    size_t bytes, n;                 /* of the block with the level tables; members */
    /* widths of the grids: per launch the largest member's extent (0: no launch); _fac over the members that factorise only */
    int np_all = 0, nn_all = 0, nh_all = 0, np_fac = 0, nh_fac = 0, cells = 0;
    std::vector<int> wide_bwd, wide_fwd, wide_fac;          /* per level walking to the root, to the leaves, to the root */
    size_t l_hess = 0, l_factor = 0, l_sweep = 0;
};
/* family: the lead's record that owns the block and the members' mark for order_behind_lead (adjb, sensb); needs_factor_of(s): whether member s builds its
 * factor anew, and where the family drops the result it is about to replace; views: per member the view its launches take, kept for the store behind the
 * wait.  The members' buffers are set up by the caller.  Nothing is waited for here in the steady state (order_behind_lead, ADJ_ORDER) */
template <typename Batch, typename NeedsFactor>
int deriv_group_fill(tqgpu_solver **v, const DeviceGroup &g, const Opts &O, Batch tqgpu_solver::*family, const char *what, NeedsFactor needs_factor_of, std::vector<Sens> &views, DerivGroup &G) {
    tqgpu_solver *lead = v[g.idx[0]];
    Batch &B = lead->*family;
    int rc;
    G = DerivGroup{};
    G.n = g.idx.size();
    const size_t items_bytes = G.n * sizeof(AItem);
    G.bytes = items_bytes;
    for (int i : g.idx) G.bytes += 2 * (size_t)v[i]->T.Nh * sizeof(int);
    if ((rc = grow_items(lead, B.d_desc, B.h_desc, B.desc_cap, G.bytes, what))) return rc;
    G.items = reinterpret_cast<AItem *>(B.h_desc); G.d_items = reinterpret_cast<AItem *>(B.d_desc);
    int *h_lvl = reinterpret_cast<int *>(B.h_desc + items_bytes);
    const int *d_lvl = reinterpret_cast<const int *>(B.d_desc + items_bytes);
    std::vector<hipStream_t> waited;
    int waits = 0;
    size_t l_at = 0;
    views.assign(G.n, Sens{});
    for (size_t m = 0; m < G.n; m++) {
        tqgpu_solver *s = v[g.idx[m]];
        if ((rc = order_behind_lead(s, lead, (s->*family).drained_at, ADJ_ORDER, waited, waits))) return rc;
        const ExportSizes z = export_sizes(s);
        AItem &it = G.items[m];
        it = AItem{};
        it.T = s->T; it.D = s->D; it.O = O;
        it.needs_factor = needs_factor_of(s) ? 1 : 0;
        it.needs_export = it.needs_factor && !s->out.valid ? 1 : 0;
        it.S = views[m] = it.needs_factor ? sens_view_of_point(s) : s->sens.v;
        const int Nh = s->T.Nh;
        it.lvl = d_lvl + l_at;
        for (int l = 0; l < Nh; l++) { h_lvl[l_at + 2 * l] = s->lvl_first[l]; h_lvl[l_at + 2 * l + 1] = s->lvl_first[l + 1] - s->lvl_first[l]; }
        l_at += 2 * (size_t)Nh;
        it.lamc = s->h_ctrl->cur ? s->D.lam1 : s->D.lam0;
        it.d_out = s->out.d;
        it.x_pad = s->x_pad; it.nxe = z.nxe; it.nue = z.nue; it.nl = z.nl; it.nx0 = s->nx0;
        G.np_all = std::max(G.np_all, s->T.Np); G.nn_all = std::max(G.nn_all, s->T.Nn); G.nh_all = std::max(G.nh_all, Nh);
        if ((int)G.wide_bwd.size() < Nh) { G.wide_bwd.resize(Nh, 0); G.wide_fwd.resize(Nh, 0); }
        if (it.needs_factor && (int)G.wide_fac.size() < Nh) G.wide_fac.resize(Nh, 0);
        for (int l = 0; l < Nh; l++) {
            const int count = s->lvl_first[l + 1] - s->lvl_first[l];
            G.wide_bwd[Nh - 1 - l] = std::max(G.wide_bwd[Nh - 1 - l], count);
            if (l >= 1) G.wide_fwd[l - 1] = std::max(G.wide_fwd[l - 1], count);
            if (it.needs_factor) G.wide_fac[Nh - 1 - l] = std::max(G.wide_fac[Nh - 1 - l], count);
        }
        G.l_sweep = std::max(G.l_sweep, s->pp.lds_forward);
        if (it.needs_factor) {
            G.np_fac = std::max(G.np_fac, s->T.Np); G.nh_fac = std::max(G.nh_fac, Nh);
            G.l_hess = std::max(G.l_hess, s->pp.lds_hess); G.l_factor = std::max(G.l_factor, s->sens.lds_factor);
            if (it.needs_export) G.cells = std::max(G.cells, std::max(std::max(z.nxe, z.nue), std::max(z.nl, 1)));
        }
    }
    MPC_COUNT(waits, waits);
    return TQGPU_OK;
}
/* the descriptors in one copy; the packing of the points that have not gone out, k_sens_hess_batch, k_sens_factor_batch per level, deepest first, each over
 * the members that factorise: nothing where none does.  The caller looks at hipGetLastError behind its own launches */
int deriv_group_launch_factor(const tqgpu_solver *lead, const DerivGroup &G) {
    int rc;
    if ((rc = allow_lds(k_sens_hess_batch, G.l_hess)) || (rc = allow_lds(k_sens_factor_batch, G.l_factor))) return rc;
    hipStream_t ls = lead->stream;
    const unsigned nz = (unsigned)G.n;
    HIP_TRY(hipMemcpyAsync(G.d_items, G.items, G.bytes, hipMemcpyHostToDevice, ls)); MPC_COUNT(copies, 1);
    if (G.cells) { hipLaunchKernelGGL(k_adj_export_batch, dim3((unsigned)((G.cells + 255) / 256), nz), dim3(256), 0, ls, G.d_items); MPC_COUNT(launches, 1); }
    if (G.np_fac) {
        hipLaunchKernelGGL(k_sens_hess_batch, dim3((unsigned)G.np_fac, 1, nz), dim3(WAVE), G.l_hess, ls, G.d_items);
        for (int j = 0; j < G.nh_fac; j++) hipLaunchKernelGGL(k_sens_factor_batch, dim3((unsigned)G.wide_fac[j], 1, nz), dim3(WAVE), G.l_factor, ls, G.d_items, j);
        MPC_COUNT(launches, 1 + G.nh_fac);
    }
    return TQGPU_OK;
}

struct AdjSpan { size_t wx, wu, gx0; };          /* where a member's blocks begin in the caller's wx, wu and gx0 */

/* The adjoint's group: w of all members in one copy through the lead's pinned block, the factor where a member has none stored, the four adjoint launches, the
 * heads in one copy */
int adj_group_enqueue(tqgpu_solver **v, const DeviceGroup &g, std::vector<Sens> &views, const Opts &O, const double *wx, const double *wu, int nw, const std::vector<AdjSpan> &span) {
    tqgpu_solver *lead = v[g.idx[0]];
    MpcAdjBatch &B = lead->adjb;
    int rc;
    HIP_TRY(hipSetDevice(lead->device));
    size_t w_all = 0, heads_all = 0;
    for (int i : g.idx) {
        tqgpu_solver *s = v[i];
        if ((rc = setup_sens(s)) || (rc = setup_adj(s, nw))) return rc;
        w_all += adj_w_doubles(s, nw); heads_all += (size_t)s->sens.nx0 * nw + 1;
    }
    DerivGroup G;
    if ((rc = deriv_group_fill(v, g, O, &tqgpu_solver::adjb, "the descriptors of a batched adjoint", [](tqgpu_solver *s) { s->sens.adj_valid = false; return !s->sens.factored; }, views, G)) ||
        (rc = grow_items(lead, B.d_w, B.h_w, B.w_cap, w_all, "the loss gradients of a batched adjoint")) ||
        (rc = grow_items(lead, B.d_heads, B.h_heads, B.heads_cap, heads_all, "the heads of a batched adjoint")))
        return rc;
    size_t l_rhs = 0, l_grad = 0, w_at = 0, h_at = 0;
    for (size_t m = 0; m < G.n; m++) {
        tqgpu_solver *s = v[g.idx[m]];
        const MpcSens &ms = s->sens;
        AItem &it = G.items[m];
        it.A = ms.a;
        it.A.wx = B.d_w + w_at; it.A.wu = it.A.wx + (size_t)it.nxe * (size_t)nw; it.A.head = B.d_heads + h_at;
        const AdjSpan &at = span[(size_t)g.idx[m]];
        adj_stage_w(s, B.h_w + w_at, wx ? wx + at.wx : nullptr, wu ? wu + at.wu : nullptr, nw);          /* w through the lead's pinned block */
        w_at += adj_w_doubles(s, nw); h_at += (size_t)ms.nx0 * nw + 1;
        l_rhs = std::max(l_rhs, ms.lds_rhs); l_grad = std::max(l_grad, ms.lds_grad);
    }
    if ((rc = allow_lds(k_adj_rhs_batch, l_rhs)) || (rc = allow_lds(k_adj_backward_batch, G.l_sweep)) || (rc = allow_lds(k_adj_forward_batch, G.l_sweep)) || (rc = allow_lds(k_adj_grad_batch, l_grad)))
        return rc;
    hipStream_t ls = lead->stream;
    const unsigned nz = (unsigned)G.n, cols = (unsigned)nw;
    if (w_all) HIP_TRY(hipMemcpyAsync(B.d_w, B.h_w, sizeof(double) * w_all, hipMemcpyHostToDevice, ls));
    MPC_COUNT(copies, 1);
    if ((rc = deriv_group_launch_factor(lead, G))) return rc;
    hipLaunchKernelGGL(k_adj_rhs_batch, dim3((unsigned)G.np_all, cols, nz), dim3(WAVE), l_rhs, ls, G.d_items);
    for (int j = 0; j < G.nh_all; j++) hipLaunchKernelGGL(k_adj_backward_batch, dim3((unsigned)G.wide_bwd[j], cols, nz), dim3(WAVE), G.l_sweep, ls, G.d_items, j);
    for (int j = 0; j + 1 < G.nh_all; j++) hipLaunchKernelGGL(k_adj_forward_batch, dim3((unsigned)G.wide_fwd[j], cols, nz), dim3(WAVE), G.l_sweep, ls, G.d_items, j);
    hipLaunchKernelGGL(k_adj_grad_batch, dim3((unsigned)G.nn_all, cols, nz), dim3(WAVE), l_grad, ls, G.d_items);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1 + G.nh_all + (G.nh_all - 1) + 1);
    HIP_TRY(hipMemcpyAsync(B.h_heads, B.d_heads, sizeof(double) * heads_all, hipMemcpyDeviceToHost, ls)); MPC_COUNT(copies, 1);
    lead->links.stream_pending = true;
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_mpc_adjoint_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *o, const double *wx, const double *wu, int nw, double *gx0, int *n_reg) {
    const char *who = "tqgpu_mpc_adjoint_batch";
    if (!solvers || n < 1 || !o) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments (solvers and opts are required, n must be at least 1)");
    if (nw < 1) return fail(TQGPU_EINVAL, std::string(who) + ": nw must be at least 1");
    int rc;
    if ((rc = refuse_members(who, solvers, n, [&](tqgpu_solver *s) {
            size_t lf, lp;
            int r;
            if ((r = sens_refuse(s, o, who)) || (r = adj_window_refuse(s, nw))) return r;
            return sens_window_refuse(s, lf, lp);
        })))
        return rc;
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    const std::vector<AdjSpan> span = member_spans<AdjSpan>(n, [&](AdjSpan &at, int i) {
        const tqgpu_solver *s = solvers[i];
        at.wx += (size_t)(s->sum_nx - s->x_pad) * nw; at.wu += (size_t)s->sum_nu * nw; at.gx0 += (size_t)s->mpc.nx0 * nw;
    });
    const std::vector<DeviceGroup> groups = plan_device_groups(solvers, n, "TREEQP_AMD_ADJ_BATCH", ADJ_BATCH_MIN, ADJ_GRID_Z);
    std::vector<std::vector<Sens>> views(groups.size());          /* of a batched group's members, from the enqueue to the collect */
    MpcLive live;
    return run_device_groups(solvers, groups, GroupRun{},
        [&](const DeviceGroup &g, size_t gi) { return adj_group_enqueue(solvers, g, views[gi], O, wx, wu, nw, span); },
        [&](int i) {          /* tqgpu_mpc_adjoint's own route */
            const AdjSpan &at = span[(size_t)i];
            return mpc_adjoint_one(solvers[i], O, wx ? wx + at.wx : nullptr, wu ? wu + at.wu : nullptr, nw, gx0 ? gx0 + at.gx0 : nullptr, n_reg ? n_reg + i : nullptr);
        },
        [&](const DeviceGroup &g, size_t gi) {
            const double *h = solvers[g.idx[0]]->adjb.h_heads;
            for (size_t m = 0; m < g.idx.size(); m++) {
                const int i = g.idx[m];
                adj_store(solvers[i], views[gi][m], h, nw, gx0 ? gx0 + span[(size_t)i].gx0 : nullptr, n_reg ? n_reg + i : nullptr);
                h += (size_t)solvers[i]->sens.nx0 * nw + 1;
            }
            return TQGPU_OK;
        });
}

/* ---- tqgpu_mpc_sensitivity_batch: per device one group; a group of SENS_BATCH_MIN members or more goes out as ONE set of launches on its first
 * member's stream (the lead's), anything else member by member through mpc_sensitivity_one.  Groups on more than one device are built like the
 * adjoint's; only one device could be tested ---- */
namespace {
constexpr int SENS_BATCH_MIN = 2;                /* members of one device from which the batched route is taken: at 2 C1 trees the sensitivity measured 157 us against 290 us member by member, at 4 160 us against 577 us; the predictor with duals 26 us against 42 us, and 28 us against 82 us (profiles/r23_mpc_gain_batch.txt) */
constexpr size_t SENS_GRID_Z = 65535;            /* blockIdx.z is the member */

/* The sensitivity's group: the factor of every member, like the single call always built anew, the forward sweep and the primal launch, the heads of all
 * members in one copy back */
int sens_group_enqueue(tqgpu_solver **v, const DeviceGroup &g, std::vector<Sens> &views, const Opts &O) {
    tqgpu_solver *lead = v[g.idx[0]];
    MpcSensBatch &B = lead->sensb;
    int rc;
    HIP_TRY(hipSetDevice(lead->device));
    size_t heads_all = 0;
    for (int i : g.idx) {
        if ((rc = setup_sens(v[i]))) return rc;
        heads_all += sens_head_doubles(v[i]);
    }
    DerivGroup G;
    if ((rc = deriv_group_fill(v, g, O, &tqgpu_solver::sensb, "the descriptors of a batched sensitivity", [](tqgpu_solver *s) { s->sens.valid = s->sens.factored = false; return true; }, views, G)) ||
        (rc = grow_items(lead, B.d_heads, B.h_heads, B.heads_cap, heads_all, "the heads of a batched sensitivity")))
        return rc;
    int nx0_all = 0;
    size_t l_primal = 0, h_at = 0;
    for (size_t m = 0; m < G.n; m++) {
        const tqgpu_solver *s = v[g.idx[m]];
        G.items[m].head_out = B.d_heads + h_at;
        h_at += sens_head_doubles(s);
        nx0_all = std::max(nx0_all, s->sens.nx0); l_primal = std::max(l_primal, s->sens.lds_primal);
    }
    if ((rc = allow_lds(k_sens_forward_batch, G.l_sweep)) || (rc = allow_lds(k_sens_primal_batch, l_primal)) || (rc = deriv_group_launch_factor(lead, G))) return rc;
    hipStream_t ls = lead->stream;
    const unsigned nz = (unsigned)G.n;
    for (int j = 0; j + 1 < G.nh_all; j++) hipLaunchKernelGGL(k_sens_forward_batch, dim3((unsigned)G.wide_fwd[j], (unsigned)nx0_all, nz), dim3(WAVE), G.l_sweep, ls, G.d_items, j);
    hipLaunchKernelGGL(k_sens_primal_batch, dim3((unsigned)G.nn_all, 1, nz), dim3(WAVE), l_primal, ls, G.d_items);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, (G.nh_all - 1) + 1);
    HIP_TRY(hipMemcpyAsync(B.h_heads, B.d_heads, sizeof(double) * heads_all, hipMemcpyDeviceToHost, ls)); MPC_COUNT(copies, 1);
    lead->links.stream_pending = true;
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_mpc_sensitivity_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *o, int *n_reg) {
    const char *who = "tqgpu_mpc_sensitivity_batch";
    if (!solvers || n < 1 || !o) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments (solvers and opts are required, n must be at least 1)");
    int rc;
    if ((rc = refuse_members(who, solvers, n, [&](tqgpu_solver *s) { size_t lf, lp; const int r = sens_refuse(s, o, who); return r ? r : sens_window_refuse(s, lf, lp); }))) return rc;
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    const std::vector<DeviceGroup> groups = plan_device_groups(solvers, n, "TREEQP_AMD_SENS_BATCH", SENS_BATCH_MIN, SENS_GRID_Z);
    std::vector<std::vector<Sens>> views(groups.size());          /* of a batched group's members, from the enqueue to the store */
    MpcLive live;
    return run_device_groups(solvers, groups, GroupRun{},
        [&](const DeviceGroup &g, size_t gi) { return sens_group_enqueue(solvers, g, views[gi], O); },
        [&](int i) { return mpc_sensitivity_one(solvers[i], O, n_reg ? n_reg + i : nullptr); },          /* tqgpu_mpc_sensitivity's own route */
        [&](const DeviceGroup &g, size_t gi) {
            /* every member's pinned head from the group's copy, then its flags: as its own call leaves it */
            const double *h = solvers[g.idx[0]]->sensb.h_heads;
            for (size_t m = 0; m < g.idx.size(); m++) {
                tqgpu_solver *s = solvers[g.idx[m]];
                const size_t head = sens_head_doubles(s);
                memcpy(s->sens.h, h, sizeof(double) * head);
                s->sens.v = views[gi][m];
                s->sens.valid = s->sens.factored = true;
                if (n_reg) n_reg[g.idx[m]] = (int)h[head - 1];
                h += head;
            }
            return TQGPU_OK;
        });
}

/* ---- the adjoint in H, A, B (tdunes_sens.hpp: k_adjmat_part, k_adjmat_sum): outer products of the stored adjoint with the point, summed over the
 * caller's parameter groups, back through pinned memory in one copy with one wait ---- */
namespace {
constexpr int ADJMAT_REGIONS = 7;          /* gH, gh, gA, gB, gb, gA0, gS0 */
bool adjmat_root(const tqgpu_solver *s) { return s->mpc.d && !s->mpc.states && s->mpc.nx0 > 0; }
/* what the tables depend on beyond the maps: every node's kind, the root form, nx0 */
std::vector<int> adjmat_sig(const tqgpu_solver *s) {
    std::vector<int> sig((size_t)s->Nn + 2);
    for (int k = 0; k < s->Nn; k++) sig[(size_t)k] = s->sk.kind(k);
    sig[(size_t)s->Nn] = adjmat_root(s) ? 1 : 0; sig[(size_t)s->Nn + 1] = s->mpc.nx0;
    return sig;
}
/* member lists, group and chunk records, the list of groups to sum, the region and partial sizes, the LDS window: built from the maps and the kinds the
 * device holds now, uploaded in one block.  Refuses a group that mixes kinds and a group whose window does not fit */
int adjmat_build(tqgpu_solver *s, const char *who) {
    MpcAdjMat &m = s->adjm;
    int rc;
    const int Nn = s->Nn;
    m.sig.clear();
    std::vector<std::vector<int>> hm((size_t)m.n_h), cm((size_t)m.n_c);
    for (int k = 0; k < Nn; k++) {
        if (m.hgroup[(size_t)k] >= 0) hm[(size_t)m.hgroup[(size_t)k]].push_back(k);
        if (m.cgroup[(size_t)k] >= 0) cm[(size_t)m.cgroup[(size_t)k]].push_back(k);
    }
    for (int g = 0; g < m.n_h; g++) for (int k : hm[(size_t)g]) if (s->sk.kind(k) != s->sk.kind(hm[(size_t)g][0]))
        return fail(TQGPU_EINVAL, std::string(who) + ": h-group " + std::to_string(g) + " has come to mix kinds: node " + std::to_string(k) + " is of kind " + std::to_string(s->sk.kind(k)) +
                                  ", node " + std::to_string(hm[(size_t)g][0]) + " of kind " + std::to_string(s->sk.kind(hm[(size_t)g][0])));
    const int root = adjmat_root(s) ? 1 : 0;
    std::vector<int> hmem, cmem, hgrp((size_t)m.n_h * 8, 0), cgrp((size_t)m.n_c * 8, 0), hchk, cchk, sums;
    size_t tot[ADJMAT_REGIONS] = {}, part = 0, lds = 0;
    auto chunks = [](std::vector<int> &chk, int g, int first, int members) {
        int q = 0;
        for (int at = 0; at < members; at += ADJMAT_CHUNK, q++) { chk.push_back(g); chk.push_back(first + at); chk.push_back(std::min(ADJMAT_CHUNK, members - at)); chk.push_back(q); }
        return q;
    };
    for (int g = 0; g < m.n_h; g++) {
        const std::vector<int> &v = hm[(size_t)g];
        const size_t nz = (size_t)(s->nx[(size_t)v[0]] + s->nu[(size_t)v[0]]), hsz = s->sk.kind(v[0]) ? nz * nz : nz;
        int *rec = &hgrp[(size_t)g * 8];
        rec[0] = v[0]; rec[1] = (int)tot[0]; rec[2] = (int)tot[1]; rec[4] = (int)(hchk.size() / 4);
        rec[5] = chunks(hchk, g, (int)hmem.size(), (int)v.size()); rec[6] = (int)part;
        hmem.insert(hmem.end(), v.begin(), v.end());
        tot[0] += hsz; tot[1] += nz; part += (size_t)rec[5] * (hsz + nz);
        lds = std::max(lds, (hsz + nz + 2 * nz + 2) * sizeof(double));
        if (rec[5] > 1) sums.push_back(g);
    }
    for (int g = 0; g < m.n_c; g++) {
        const std::vector<int> &v = cm[(size_t)g];
        const int c = v[0], p = s->dad[(size_t)c];
        const size_t nxc = (size_t)s->nx[(size_t)c], nxp = (size_t)s->nx[(size_t)p], nup = (size_t)s->nu[(size_t)p], gsz = nxc * (nxp + nup + 1);
        int *rec = &cgrp[(size_t)g * 8];
        rec[0] = c; rec[1] = (int)tot[2]; rec[2] = (int)tot[3]; rec[3] = (int)tot[4]; rec[4] = (int)(cchk.size() / 4);
        rec[5] = chunks(cchk, g, (int)cmem.size(), (int)v.size()); rec[6] = (int)part;
        cmem.insert(cmem.end(), v.begin(), v.end());
        tot[2] += nxc * nxp; tot[3] += nxc * nup; tot[4] += nxc; part += (size_t)rec[5] * gsz;
        lds = std::max(lds, (gsz + 2 * nxc + 2 * (nxp + nup) + 2) * sizeof(double));
        if (rec[5] > 1) sums.push_back(m.n_h + g);
    }
    const size_t pR = part;
    if (root) { tot[5] = (size_t)s->mpc.nb * s->mpc.nx0; tot[6] = (size_t)s->nu[0] * s->mpc.nx0; part += tot[5] + tot[6]; }
    if (lds > 160 * 1024) return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": a group's window (its result blocks and a member's vectors) does not fit 160 KiB of LDS");
    /* the region starts: every offset of a record is made absolute */
    m.reg[0] = 0;
    for (int i = 0; i < ADJMAT_REGIONS; i++) m.reg[i + 1] = m.reg[i] + tot[i];
    if (m.reg[ADJMAT_REGIONS] > (size_t)INT_MAX / 2 || part > (size_t)INT_MAX / 2) return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": the result does not fit the tables' 32-bit offsets");
    for (int g = 0; g < m.n_h; g++) { hgrp[(size_t)g * 8 + 1] += (int)m.reg[0]; hgrp[(size_t)g * 8 + 2] += (int)m.reg[1]; }
    for (int g = 0; g < m.n_c; g++) { cgrp[(size_t)g * 8 + 1] += (int)m.reg[2]; cgrp[(size_t)g * 8 + 2] += (int)m.reg[3]; cgrp[(size_t)g * 8 + 3] += (int)m.reg[4]; }
    std::vector<int> tab;
    auto put = [&](const std::vector<int> &v) { const size_t at = tab.size(); tab.insert(tab.end(), v.begin(), v.end()); return at; };
    const size_t o_hmem = put(hmem), o_cmem = put(cmem), o_hgrp = put(hgrp), o_cgrp = put(cgrp), o_hchk = put(hchk), o_cchk = put(cchk), o_sums = put(sums);
    tab.push_back(0);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->mem.release(m.d_tab);
    if ((rc = s->mem.upload(m.d_tab, tab.data(), tab.size() * sizeof(int), TQGPU_ENOMEM, "the tables of the parameter groups"))) return rc;
    AdjMat &M = m.v;
    M = AdjMat{};
    M.hmem = m.d_tab + o_hmem; M.cmem = m.d_tab + o_cmem; M.hgrp = m.d_tab + o_hgrp; M.cgrp = m.d_tab + o_cgrp;
    M.hchk = m.d_tab + o_hchk; M.cchk = m.d_tab + o_cchk; M.sums = m.d_tab + o_sums;
    M.n_hgrp = m.n_h; M.n_cgrp = m.n_c; M.n_hchk = (int)(hchk.size() / 4); M.n_cchk = (int)(cchk.size() / 4); M.n_sums = (int)sums.size();
    M.root = root; M.oA0 = (int)m.reg[5]; M.oS0 = (int)m.reg[6]; M.pR = (int)pR;
    m.n_units = M.n_hchk + M.n_cchk + root;
    m.part1 = part; m.lds = lds;
    /* the same h-groups for tqgpu_mpc_adjoint_bounds: per chunk [glb | gub] of nx + nu entries each */
    std::vector<int> width((size_t)m.n_h);
    for (int g = 0; g < m.n_h; g++) width[(size_t)g] = 2 * (s->nx[(size_t)hm[(size_t)g][0]] + s->nu[(size_t)hm[(size_t)g][0]]);
    if ((rc = nodesum_build(s, s->bsum, hm, width, 0, who))) return rc;
    m.sig = adjmat_sig(s);
    return TQGPU_OK;
}
/* what the two calls refuse for a mirror before anything of its results is touched; brings the tables up to date with the kinds, the root form and nx0 */
int adjmat_refuse(tqgpu_solver *s, const char *who) {
    int rc;
    if ((rc = mpc_refuse(s, who)) || (rc = adj_need(s, who))) return rc;
    if (!s->adjm.set) return fail(TQGPU_EINVAL, std::string(who) + ": no parameter groups have been given (tqgpu_mpc_set_param_groups)");
    if (s->adjm.sig != adjmat_sig(s) && (rc = adjmat_build(s, who))) return rc;
    return TQGPU_OK;
}
/* the result block, its pinned twin and the partials for nw columns */
int adjmat_room(tqgpu_solver *s, int nw) {
    MpcAdjMat &m = s->adjm;
    int rc;
    const size_t need_res = std::max<size_t>(m.reg[ADJMAT_REGIONS] * (size_t)nw, 1), need_part = std::max<size_t>(m.part1 * (size_t)nw, 1);
    if (!m.d_res || m.res_cap < need_res) {
        s->mem.release(m.d_res); s->mem.release(m.h_res); m.res_cap = 0;
        if ((rc = s->mem.device(m.d_res, need_res * sizeof(double), TQGPU_ENOMEM, "the matrix gradients")) || (rc = s->mem.host(m.h_res, need_res * sizeof(double), "the pinned matrix gradients"))) return rc;
        m.res_cap = need_res;
    }
    if (!m.d_part || m.part_cap < need_part) {
        s->mem.release(m.d_part); m.part_cap = 0;
        if ((rc = s->mem.device(m.d_part, need_part * sizeof(double), TQGPU_ENOMEM, "the partial sums of the matrix gradients"))) return rc;
        m.part_cap = need_part;
    }
    return TQGPU_OK;
}
/* the view the kernels take: the tables, the duals of the export block, where to write */
AdjMat adjmat_view(const tqgpu_solver *s, double *res) {
    AdjMat M = s->adjm.v;
    const ExportSizes z = export_sizes(s);
    M.lam = s->out.d + z.nxe + z.nue; M.res = res; M.part = s->adjm.d_part;
    return M;
}
/* the seven regions of a result block of nw columns, each to its pointer at an offset (in doubles) of its own; add: accumulate instead of copying */
void adjmat_scatter(const MpcAdjMat &m, const double *h, int nw, double *const out[ADJMAT_REGIONS], const size_t at[ADJMAT_REGIONS], bool add = false) {
    for (int i = 0; i < ADJMAT_REGIONS; i++) {
        const size_t n = (m.reg[i + 1] - m.reg[i]) * (size_t)nw;
        if (!out[i] || !n) continue;
        const double *src = h + m.reg[i] * (size_t)nw;
        if (!add) memcpy(out[i] + at[i], src, sizeof(double) * n);
        else for (size_t e = 0; e < n; e++) out[i][at[i] + e] = out[i][at[i] + e] + src[e];
    }
}
/* one mirror on its own stream: one or two launches, one copy, one wait */
int adjmat_one(tqgpu_solver *s, double *const out[ADJMAT_REGIONS], const size_t at[ADJMAT_REGIONS], bool add = false) {
    MpcAdjMat &m = s->adjm;
    int rc;
    const int nw = s->sens.nw;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = adjmat_room(s, nw)) || (rc = allow_lds(k_adjmat_part, m.lds))) return rc;
    const AdjMat M = adjmat_view(s, m.d_res);
    hipStream_t st = s->stream;
    if (m.n_units) { hipLaunchKernelGGL(k_adjmat_part, dim3((unsigned)m.n_units, (unsigned)nw), dim3(WAVE), m.lds, st, s->T, s->D, s->sens.v, s->sens.a, M); MPC_COUNT(launches, 1); }
    if (M.n_sums) { hipLaunchKernelGGL(k_adjmat_sum, dim3((unsigned)M.n_sums, (unsigned)nw), dim3(WAVE), 0, st, s->T, s->D, s->sens.v, M, nw); MPC_COUNT(launches, 1); }
    HIP_TRY(hipGetLastError());
    const size_t n = m.reg[ADJMAT_REGIONS] * (size_t)nw;
    if (n) HIP_TRY(hipMemcpyAsync(m.h_res, m.d_res, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    adjmat_scatter(m, m.h_res, nw, out, at, add);
    return TQGPU_OK;
}
/* A group on its lead's stream: the descriptors in one copy, one launch over all members' units, the sums (reduce: over the members into the first
 * member's block, in member order on the device; else per member over its chunks), the lead's result block back in one copy; nothing is waited for
 * here but a member's pending uploads (order_behind_lead, ADJMAT_ORDER).  at: where each member's results begin in that block */
int adjmat_group_enqueue(tqgpu_solver **v, const DeviceGroup &g, int reduce, std::vector<size_t> &at) {
    tqgpu_solver *lead = v[g.idx[0]];
    MpcAdjMat &B = lead->adjm;
    const size_t nm = g.idx.size();
    int rc;
    HIP_TRY(hipSetDevice(lead->device));
    size_t total = 0, lds = 0;
    int units = 0, nsums = 0, cols = 0, waits = 0;
    std::vector<hipStream_t> waited;
    at.assign(nm, 0);
    for (size_t k = 0; k < nm; k++) {
        tqgpu_solver *s = v[g.idx[k]];
        if ((rc = order_behind_lead(s, lead, s->adjb.drained_at, ADJMAT_ORDER, waited, waits)) || (rc = adjmat_room(s, s->sens.nw))) return rc;
        at[k] = total;
        if (!reduce || k == 0) total += s->adjm.reg[ADJMAT_REGIONS] * (size_t)s->sens.nw;
        units = std::max(units, s->adjm.n_units); nsums = std::max(nsums, s->adjm.v.n_sums); cols = std::max(cols, s->sens.nw); lds = std::max(lds, s->adjm.lds);
    }
    MPC_COUNT(waits, waits);
    if ((rc = grow_items(lead, B.d_desc, B.h_desc, B.desc_cap, nm * sizeof(AMItem), "the descriptors of the batched matrix gradients")) ||
        (rc = grow_items(lead, B.d_bres, B.h_bres, B.bres_cap, total, "the matrix gradients of a batch")) ||
        (rc = allow_lds(k_adjmat_part_batch, lds)))
        return rc;
    AMItem *items = reinterpret_cast<AMItem *>(B.h_desc);
    for (size_t k = 0; k < nm; k++) {
        tqgpu_solver *s = v[g.idx[k]];
        AMItem &it = items[k];
        it = AMItem{};
        it.T = s->T; it.D = s->D; it.S = s->sens.v; it.A = s->sens.a;
        it.M = adjmat_view(s, B.d_bres + (reduce ? 0 : at[k]));
    }
    hipStream_t ls = lead->stream;
    const AMItem *d_items = reinterpret_cast<const AMItem *>(B.d_desc);
    HIP_TRY(hipMemcpyAsync(B.d_desc, B.h_desc, nm * sizeof(AMItem), hipMemcpyHostToDevice, ls)); MPC_COUNT(copies, 1);
    if (units) { hipLaunchKernelGGL(k_adjmat_part_batch, dim3((unsigned)units, (unsigned)cols, (unsigned)nm), dim3(WAVE), lds, ls, d_items, reduce); MPC_COUNT(launches, 1); }
    if (reduce) {
        const int gu = B.n_h + B.n_c + B.v.root;
        if (gu) { hipLaunchKernelGGL(k_adjmat_reduce, dim3((unsigned)gu, (unsigned)cols), dim3(WAVE), 0, ls, d_items, (int)nm); MPC_COUNT(launches, 1); }
    } else if (nsums) { hipLaunchKernelGGL(k_adjmat_sum_batch, dim3((unsigned)nsums, (unsigned)cols, (unsigned)nm), dim3(WAVE), 0, ls, d_items); MPC_COUNT(launches, 1); }
    HIP_TRY(hipGetLastError());
    if (total) HIP_TRY(hipMemcpyAsync(B.h_bres, B.d_bres, sizeof(double) * total, hipMemcpyDeviceToHost, ls));
    MPC_COUNT(copies, 1);
    lead->links.stream_pending = true;
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_mpc_set_param_groups(tqgpu_solver *s, const int *hgroup, const int *cgroup, int n_hgroups, int n_cgroups) {
    const char *who = "tqgpu_mpc_set_param_groups";
    int rc;
    if ((rc = mpc_refuse(s, who))) return rc;
    const int Nn = s->Nn;
    std::vector<int> hg((size_t)Nn), cg((size_t)Nn);
    const int n_h = hgroup ? n_hgroups : Nn, n_c = cgroup ? n_cgroups : Nn - 1;
    if (n_h < 0 || n_c < 0) return fail(TQGPU_EINVAL, std::string(who) + ": a negative number of groups");
    for (int k = 0; k < Nn; k++) {
        hg[(size_t)k] = hgroup ? hgroup[k] : k;
        cg[(size_t)k] = cgroup ? cgroup[k] : k - 1;
        if (hg[(size_t)k] < -1 || hg[(size_t)k] >= n_h) return fail(TQGPU_EINVAL, std::string(who) + ": node " + std::to_string(k) + ": hgroup = " + std::to_string(hg[(size_t)k]) + " is outside [-1, " + std::to_string(n_h) + ")");
        if (cg[(size_t)k] < -1 || cg[(size_t)k] >= n_c) return fail(TQGPU_EINVAL, std::string(who) + ": node " + std::to_string(k) + ": cgroup = " + std::to_string(cg[(size_t)k]) + " is outside [-1, " + std::to_string(n_c) + ")");
    }
    if (cg[0] != -1) return fail(TQGPU_EINVAL, std::string(who) + ": node 0: the root has no dynamics, cgroup[0] must be -1");
    std::vector<int> hfirst((size_t)n_h, -1), cfirst((size_t)n_c, -1), hdims((size_t)n_h * 4, 0), cdims((size_t)n_c * 4, 0);
    for (int k = 0; k < Nn; k++) {
        const int g = hg[(size_t)k], pad = k == 0 ? s->x_pad : 0;
        if (g >= 0) {
            int *d = &hdims[(size_t)g * 4];
            if (hfirst[(size_t)g] < 0) { hfirst[(size_t)g] = k; d[0] = s->nx[(size_t)k]; d[1] = s->nu[(size_t)k]; d[2] = pad; }
            else if (d[0] != s->nx[(size_t)k] || d[1] != s->nu[(size_t)k] || d[2] != pad)
                return fail(TQGPU_EINVAL, std::string(who) + ": node " + std::to_string(k) + ": nx, nu or the phantom root states differ from those of node " + std::to_string(hfirst[(size_t)g]) + ", the first member of h-group " + std::to_string(g));
            d[3]++;
        }
        const int gc = cg[(size_t)k];
        if (gc >= 0) {
            const int p = s->dad[(size_t)k];
            int *d = &cdims[(size_t)gc * 4];
            if (cfirst[(size_t)gc] < 0) { cfirst[(size_t)gc] = k; d[0] = s->nx[(size_t)k]; d[1] = s->nx[(size_t)p]; d[2] = s->nu[(size_t)p]; }
            else if (d[0] != s->nx[(size_t)k] || d[1] != s->nx[(size_t)p] || d[2] != s->nu[(size_t)p])
                return fail(TQGPU_EINVAL, std::string(who) + ": node " + std::to_string(k) + ": nx of the node, or nx, nu of its parent differ from those of node " + std::to_string(cfirst[(size_t)gc]) + ", the first member of c-group " + std::to_string(gc));
            d[3]++;
        }
    }
    for (int g = 0; g < n_h; g++) if (hfirst[(size_t)g] < 0) return fail(TQGPU_EINVAL, std::string(who) + ": h-group " + std::to_string(g) + " has no member");
    for (int g = 0; g < n_c; g++) if (cfirst[(size_t)g] < 0) return fail(TQGPU_EINVAL, std::string(who) + ": c-group " + std::to_string(g) + " has no member");
    MpcAdjMat &m = s->adjm;
    m.hgroup = hg; m.cgroup = cg; m.hdims = hdims; m.cdims = cdims; m.n_h = n_h; m.n_c = n_c;
    m.set = false;
    if ((rc = adjmat_build(s, who))) return rc;
    m.set = true;
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_get_param_groups(tqgpu_solver *s, int *n_hgroups, int *n_cgroups, int *hdims, int *cdims, int *root) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_param_groups"))) return rc;
    const MpcAdjMat &m = s->adjm;
    if (!m.set) return fail(TQGPU_EINVAL, "tqgpu_mpc_get_param_groups: no parameter groups have been given (tqgpu_mpc_set_param_groups)");
    if (n_hgroups) *n_hgroups = m.n_h;
    if (n_cgroups) *n_cgroups = m.n_c;
    if (hdims) for (int g = 0; g < m.n_h; g++) {
        memcpy(hdims + 5 * (size_t)g, &m.hdims[4 * (size_t)g], sizeof(int) * 4);
        const int first = (int)(std::find(m.hgroup.begin(), m.hgroup.end(), g) - m.hgroup.begin());
        hdims[5 * (size_t)g + 4] = s->sk.kind(first);
    }
    if (cdims && !m.cdims.empty()) memcpy(cdims, m.cdims.data(), sizeof(int) * m.cdims.size());
    if (root) { root[0] = adjmat_root(s) ? s->mpc.nb : 0; root[1] = s->nu[0]; root[2] = s->mpc.nx0; root[3] = s->sens.adj_valid ? s->sens.nw : 0; }
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_adjoint_matrices(tqgpu_solver *s, double *gH, double *gh, double *gA, double *gB, double *gb, double *gA0, double *gS0) {
    int rc;
    if ((rc = adjmat_refuse(s, "tqgpu_mpc_adjoint_matrices"))) return rc;
    MpcLive live;
    double *const out[ADJMAT_REGIONS] = {gH, gh, gA, gB, gb, gA0, gS0};
    const size_t at[ADJMAT_REGIONS] = {};
    return adjmat_one(s, out, at);
}

/* ---- sums of the stored adjoint over node sets (tdunes_sens.hpp: k_nodesum_part, k_nodesum_sum): the bound gradients over the h-groups, the gradient
 * of the tracking reference over the nodes of a trajectory row ---- */
namespace {
/* one mirror on its own stream: N with the call's own fields set, `targets` results of res_doubles doubles in all: one launch, a second where a
 * result has more than one partial, one copy through pinned memory, one wait; the results are then in m.h_res */
int nodesum_run(tqgpu_solver *s, MpcNodeSum &m, NodeSum N, int targets, size_t res_doubles) {
    int rc;
    const int nw = s->sens.nw;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    const size_t need_res = std::max<size_t>(res_doubles, 1), need_part = std::max<size_t>(m.part1 * (size_t)nw, 1);
    if (!m.d_res || m.res_cap < need_res) {
        s->mem.release(m.d_res); s->mem.release(m.h_res); m.res_cap = 0;
        if ((rc = s->mem.device(m.d_res, need_res * sizeof(double), TQGPU_ENOMEM, "the summed gradients")) || (rc = s->mem.host(m.h_res, need_res * sizeof(double), "the pinned summed gradients"))) return rc;
        m.res_cap = need_res;
    }
    if (!m.d_part || m.part_cap < need_part) {
        s->mem.release(m.d_part); m.part_cap = 0;
        if ((rc = s->mem.device(m.d_part, need_part * sizeof(double), TQGPU_ENOMEM, "the partial sums of the summed gradients"))) return rc;
        m.part_cap = need_part;
    }
    if ((rc = allow_lds(k_nodesum_part, m.lds))) return rc;
    bool many = false;
    for (int t = 0; t < targets && !many; t++) {
        int c_lo, c_hi;
        nodesum_span(m.set.data(), N.n_set, N.mode, N.t0, N.Tn, N.row0, t, c_lo, c_hi);
        many = c_hi - c_lo > 1;
    }
    N.res = m.d_res; N.part = m.d_part;
    hipStream_t st = s->stream;
    if (N.n_chk) { hipLaunchKernelGGL(k_nodesum_part, dim3((unsigned)N.n_chk, (unsigned)nw), dim3(WAVE), m.lds, st, s->T, s->D, s->sens.v, s->sens.a, N); MPC_COUNT(launches, 1); }
    if (many) { hipLaunchKernelGGL(k_nodesum_sum, dim3((unsigned)targets, (unsigned)nw), dim3(WAVE), 0, st, N, nw); MPC_COUNT(launches, 1); }
    HIP_TRY(hipGetLastError());
    if (res_doubles) HIP_TRY(hipMemcpyAsync(m.h_res, m.d_res, sizeof(double) * res_doubles, hipMemcpyDeviceToHost, st));
    MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_mpc_adjoint_bounds(tqgpu_solver *s, double *glb, double *gub) {
    int rc;
    if ((rc = adjmat_refuse(s, "tqgpu_mpc_adjoint_bounds"))) return rc;
    MpcLive live;
    MpcNodeSum &m = s->bsum;
    const size_t n = (size_t)m.v.tot * (size_t)s->sens.nw;
    if ((rc = nodesum_run(s, m, m.v, m.v.n_set, 2 * n))) return rc;
    if (glb && n) memcpy(glb, m.h_res, sizeof(double) * n);
    if (gub && n) memcpy(gub, m.h_res + n, sizeof(double) * n);
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_adjoint_reference(tqgpu_solver *s, double *gxref, double *guref, int *row0, int *rows) {
    const char *who = "tqgpu_mpc_adjoint_reference";
    int rc;
    if ((rc = mpc_refuse(s, who))) return rc;
    for (int k = 0; k < s->Nn; k++) if (s->sk.kind(k) >= 2)
        return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": the tree has nodes of kind 2 or 3, which the adjoint refuses");
    if (!s->trk.d) return fail(TQGPU_EINVAL, std::string(who) + ": the reference trajectory has not been given yet (tqgpu_mpc_set_tracking)");
    if (s->trk.t0 < 0) return fail(TQGPU_EINVAL, std::string(who) + ": no window is in force (tqgpu_mpc_set_window, tqgpu_mpc_step_at): q, r do not depend on the reference yet");
    if ((rc = adj_need(s, who))) return rc;
    MpcNodeSum &m = s->rsum;
    NodeSum N = m.v;
    N.t0 = s->trk.t0; N.Tn = s->trk.T; N.nxt = s->trk.nxt; N.nut = s->trk.nut;
    N.row0 = std::min(N.t0, N.Tn - 1);
    N.rows = std::min(N.t0 + N.n_set - 1, N.Tn - 1) - N.row0 + 1;          /* n_set - 1: the deepest stage */
    if (row0) *row0 = N.row0;
    if (rows) *rows = N.rows;
    if (!gxref && !guref) return TQGPU_OK;          /* the sizes alone: host state only */
    MpcLive live;
    const size_t nw = (size_t)s->sens.nw, W = (size_t)(N.nxt + N.nut), cells = nw * (size_t)N.rows;
    if ((rc = nodesum_run(s, m, N, N.rows, cells * W))) return rc;
    for (size_t c = 0; c < cells; c++) {
        if (gxref && N.nxt) memcpy(gxref + c * N.nxt, m.h_res + c * W, sizeof(double) * (size_t)N.nxt);
        if (guref && N.nut) memcpy(guref + c * N.nut, m.h_res + c * W + N.nxt, sizeof(double) * (size_t)N.nut);
    }
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_adjoint_matrices_batch(tqgpu_solver **solvers, int n, int reduce, double *gH, double *gh, double *gA, double *gB, double *gb, double *gA0, double *gS0) {
    const char *who = "tqgpu_mpc_adjoint_matrices_batch";
    if (!solvers || n < 1) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments (solvers is required, n must be at least 1)");
    if (reduce != 0 && reduce != 1) return fail(TQGPU_EINVAL, std::string(who) + ": reduce must be 0 or 1");
    int rc;
    /* the refusals, all of them before any member's results are touched */
    if ((rc = refuse_members(who, solvers, n, [&](tqgpu_solver *s) { return adjmat_refuse(s, who); }, [&](int i) {
            const MpcAdjMat &a = solvers[0]->adjm, &b = solvers[i]->adjm;
            if (reduce && (a.hdims != b.hdims || a.cdims != b.cdims || !std::equal(a.reg, a.reg + ADJMAT_REGIONS + 1, b.reg) || a.part1 != b.part1 || a.v.n_hchk != b.v.n_hchk || a.v.n_cchk != b.v.n_cchk ||
                           a.v.root != b.v.root || solvers[0]->sens.nw != solvers[i]->sens.nw))
                return fail(TQGPU_EINVAL, std::string(who) + ": member " + std::to_string(i) + ": its group tables (shapes, kinds, root terms) or its columns differ from member 0's; reduce = 1 sums equal shapes");
            return TQGPU_OK;
        })))
        return rc;
    double *const out[ADJMAT_REGIONS] = {gH, gh, gA, gB, gb, gA0, gS0};
    typedef std::array<size_t, ADJMAT_REGIONS> Regions;          /* where a member's regions begin in the caller's seven arrays: under reduce = 1 all at the first member's */
    const std::vector<Regions> span = member_spans<Regions>(n, [&](Regions &at, int i) {
        const MpcAdjMat &m = solvers[i]->adjm;
        if (!reduce) for (int r = 0; r < ADJMAT_REGIONS; r++) at[(size_t)r] += (m.reg[r + 1] - m.reg[r]) * (size_t)solvers[i]->sens.nw;
    });
    const std::vector<DeviceGroup> groups = plan_device_groups(solvers, n, "TREEQP_AMD_ADJ_BATCH", ADJ_BATCH_MIN, ADJ_GRID_Z);
    MpcLive live;
    if (reduce && (groups.size() != 1 || !groups[0].batched)) {
        /* the sum over members on the host, in member order: the first member's blocks, then entry by entry the others' */
        for (int i = 0; i < n; i++) if ((rc = adjmat_one(solvers[i], out, span[0].data(), i > 0))) return rc;
        return TQGPU_OK;
    }
    std::vector<std::vector<size_t>> sent(groups.size());          /* where a batched group's members begin in its lead's result block */
    return run_device_groups(solvers, groups, GroupRun{false},          /* an enqueue error is returned as it is */
        [&](const DeviceGroup &g, size_t gi) { return adjmat_group_enqueue(solvers, g, reduce, sent[gi]); },
        [&](int i) { return adjmat_one(solvers[i], out, span[(size_t)i].data()); },
        [&](const DeviceGroup &g, size_t gi) {
            for (size_t k = 0; k < (reduce ? 1 : g.idx.size()); k++) {
                const tqgpu_solver *s = solvers[g.idx[k]];
                adjmat_scatter(s->adjm, solvers[g.idx[0]]->adjm.h_bres + sent[gi][k], s->sens.nw, out, span[(size_t)g.idx[k]].data());
            }
            return TQGPU_OK;
        });
}

extern "C" int tqgpu_mpc_get_gain(tqgpu_solver *s, double *K, double *u0, double *x0_ref) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_gain")) || (rc = sens_need(s, "tqgpu_mpc_get_gain"))) return rc;
    const size_t nu0 = (size_t)s->nu[0], nx0 = (size_t)s->sens.nx0;
    if (K && nu0 * nx0) memcpy(K, s->sens.h, sizeof(double) * nu0 * nx0);
    if (u0 && nu0) memcpy(u0, s->sens.h + nu0 * nx0, sizeof(double) * nu0);
    if (x0_ref && nx0) memcpy(x0_ref, s->sens.h + nu0 * nx0 + nu0, sizeof(double) * nx0);
    return TQGPU_OK;
}

/* a diagnostic download (whole buffers through pageable memory, repacked on the host): not part of a step, not counted into tqgpu_mpc_stats */
extern "C" int tqgpu_mpc_get_sensitivities(tqgpu_solver *s, double *dx, double *du, double *dlam) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_sensitivities")) || (rc = sens_need(s, "tqgpu_mpc_get_sensitivities"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t nx0 = (size_t)s->sens.nx0, snu = (size_t)s->sum_nu;
    if (dx && (rc = download_columns(s, s->sens.v.dx, nx0, (size_t)s->x_pad, (size_t)(s->sum_nx - s->x_pad), dx))) return rc;      /* phantom root states are left out */
    if (dlam && (rc = download_columns(s, s->sens.v.dlam, nx0, (size_t)s->nx0, (size_t)s->sum_lam, dlam))) return rc;              /* the root has no dual */
    if (du && snu * nx0) HIP_TRY(hipMemcpy(du, s->sens.v.du, sizeof(double) * snu * nx0, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* the predicted duals take the start buffer for ONE solve, as the shifted ones of tqgpu_mpc_shift do: in mode 0 the kernel saves the caller's buffer
 * (once) and the solve after the next puts it back (solve_begin).  predict_keep: where the kernel saves it (allocated on first use; nullptr: nothing
 * to save), before the launch; predict_lent: the host's flags, behind the launch */
static int predict_keep(tqgpu_solver *s, int duals, double *&keep) {
    int rc;
    const bool lend = duals && s->warm.mode == 0;
    if (lend && !s->shift.d_keep && (rc = s->mem.zeroed(s->shift.d_keep, sizeof(double) * (size_t)std::max(s->sum_nx, 1), TQGPU_ENOMEM, "the saved start buffer"))) return rc;
    keep = lend && s->shift.restore == 0 ? s->shift.d_keep : nullptr;
    return TQGPU_OK;
}
static void predict_lent(tqgpu_solver *s, int duals) {
    if (!duals) return;
    if (s->warm.mode == 0) s->shift.restore = 1;
    s->warm.fresh = true;          /* the next solve starts from the start buffer as it is now, in any mode */
    s->lam_valid = false;
}
/* one mirror on its own stream, behind the refusals that touch nothing; counted into whatever record is live */
static int mpc_predict_one(tqgpu_solver *s, const double *x0_new, double *u0_pred, int duals, int *n_clipped) {
    int rc;
    const size_t nu0 = (size_t)s->nu[0], nx0 = (size_t)s->sens.nx0, head = sens_head_doubles(s);
    double *x0n = s->sens.h + head, *out = x0n + nx0;
    memcpy(x0n, x0_new, sizeof(double) * nx0);
    double *keep = nullptr;
    if ((rc = predict_keep(s, duals, keep))) return rc;
    hipLaunchKernelGGL(k_mpc_predict, dim3(duals ? 1 + (unsigned)s->Nn : 1u), dim3(WAVE), 0, s->stream, s->T, s->D, s->sens.v, (const double *)x0n, s->d_lam_init, keep, out);
    HIP_TRY(hipGetLastError()); MPC_COUNT(launches, 1);
    predict_lent(s, duals);
    HIP_TRY(hipStreamSynchronize(s->stream)); MPC_COUNT(waits, 1);
    if (u0_pred && nu0) memcpy(u0_pred, out, sizeof(double) * nu0);
    if (n_clipped) *n_clipped = (int)out[nu0];
    return TQGPU_OK;
}
extern "C" int tqgpu_mpc_predict(tqgpu_solver *s, const double *x0_new, double *u0_pred, int duals, int *n_clipped) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_predict")) || (rc = sens_need(s, "tqgpu_mpc_predict"))) return rc;
    if (!x0_new) return fail(TQGPU_EINVAL, "tqgpu_mpc_predict: x0_new is required");
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    return mpc_predict_one(s, x0_new, u0_pred, duals, n_clipped);
}

/* ---- tqgpu_mpc_predict_batch: per device one group, one launch on the lead's stream over all members; x0_new and the results travel through a pinned
 * block of the lead, which the kernel reads and writes in place, as the single call does through the mirror's ---- */
namespace {
struct PredSpan { size_t x0, u0; };          /* where a member's blocks begin in the caller's x0_new and u0_pred */
int predict_group_enqueue(tqgpu_solver **v, const DeviceGroup &g, const double *x0_new, int duals, const std::vector<PredSpan> &span) {
    tqgpu_solver *lead = v[g.idx[0]];
    MpcSensBatch &B = lead->sensb;
    const size_t n = g.idx.size();
    int rc;
    HIP_TRY(hipSetDevice(lead->device));
    size_t io_all = 0;
    for (int i : g.idx) io_all += (size_t)v[i]->sens.nx0 + (size_t)v[i]->nu[0] + 1;
    if ((rc = grow_items(lead, B.d_pdesc, B.h_pdesc, B.pdesc_cap, n * sizeof(PredItem), "the descriptors of a batched predictor"))) return rc;
    if (!B.h_io || B.io_cap < io_all) {
        lead->mem.release(B.h_io); B.io_cap = 0;
        if ((rc = lead->mem.host(B.h_io, sizeof(double) * 2 * io_all, "the pinned block of a batched predictor"))) return rc;
        B.io_cap = 2 * io_all;
    }
    PredItem *items = reinterpret_cast<PredItem *>(B.h_pdesc);
    std::vector<hipStream_t> waited;
    int waits = 0, nn_all = 0;
    size_t at = 0;
    for (size_t m = 0; m < n; m++) {
        tqgpu_solver *s = v[g.idx[m]];
        /* behind a sensitivity that returned behind its wait, no solve since: only uploads (a start buffer) can be pending on the member's own stream */
        if ((rc = order_behind_lead(s, lead, s->sensb.drained_at, ADJMAT_ORDER, waited, waits))) return rc;
        const size_t nx0 = (size_t)s->sens.nx0;
        PredItem &it = items[m];
        it = PredItem{};
        it.T = s->T; it.D = s->D; it.S = s->sens.v;
        double *x0n = B.h_io + at;
        memcpy(x0n, x0_new + span[(size_t)g.idx[m]].x0, sizeof(double) * nx0);
        it.x0_new = x0n; it.out = x0n + nx0;
        at += nx0 + (size_t)s->nu[0] + 1;
        it.lam_init = s->d_lam_init; it.duals = duals ? 1 : 0;
        if ((rc = predict_keep(s, duals, it.lam_keep))) return rc;
        nn_all = std::max(nn_all, s->Nn);
    }
    MPC_COUNT(waits, waits);
    hipStream_t ls = lead->stream;
    HIP_TRY(hipMemcpyAsync(B.d_pdesc, B.h_pdesc, n * sizeof(PredItem), hipMemcpyHostToDevice, ls)); MPC_COUNT(copies, 1);
    hipLaunchKernelGGL(k_mpc_predict_batch, dim3(duals ? 1 + (unsigned)nn_all : 1u, 1, (unsigned)n), dim3(WAVE), 0, ls, reinterpret_cast<const PredItem *>(B.d_pdesc));
    HIP_TRY(hipGetLastError()); MPC_COUNT(launches, 1);
    for (int i : g.idx) predict_lent(v[i], duals);
    lead->links.stream_pending = true;
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_mpc_predict_batch(tqgpu_solver **solvers, int n, const double *x0_new, double *u0_pred, int duals, int *n_clipped) {
    const char *who = "tqgpu_mpc_predict_batch";
    if (!solvers || n < 1 || !x0_new) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments (solvers and x0_new are required, n must be at least 1)");
    int rc;
    if ((rc = refuse_members(who, solvers, n, [&](tqgpu_solver *s) { const int r = mpc_refuse(s, who); return r ? r : sens_need(s, who); }))) return rc;
    const std::vector<PredSpan> span = member_spans<PredSpan>(n, [&](PredSpan &at, int i) { at.x0 += (size_t)solvers[i]->sens.nx0; at.u0 += (size_t)solvers[i]->nu[0]; });
    const std::vector<DeviceGroup> groups = plan_device_groups(solvers, n, "TREEQP_AMD_SENS_BATCH", SENS_BATCH_MIN, SENS_GRID_Z);
    MpcLive live;
    return run_device_groups(solvers, groups, GroupRun{},
        [&](const DeviceGroup &g, size_t) { return predict_group_enqueue(solvers, g, x0_new, duals, span); },
        [&](int i) {          /* tqgpu_mpc_predict's own route */
            return mpc_predict_one(solvers[i], x0_new + span[(size_t)i].x0, u0_pred ? u0_pred + span[(size_t)i].u0 : nullptr, duals, n_clipped ? n_clipped + i : nullptr);
        },
        [&](const DeviceGroup &g, size_t) {
            const double *io = solvers[g.idx[0]]->sensb.h_io;
            for (int i : g.idx) {
                const size_t nx0 = (size_t)solvers[i]->sens.nx0, nu0 = (size_t)solvers[i]->nu[0];
                const double *out = io + nx0;
                if (u0_pred && nu0) memcpy(u0_pred + span[(size_t)i].u0, out, sizeof(double) * nu0);
                if (n_clipped) n_clipped[i] = (int)out[nu0];
                io += nx0 + nu0 + 1;
            }
            return TQGPU_OK;
        });
}


/* ---- the tangent of an MPC step (tdunes_sens.hpp: k_tan_rhs, k_tan_primal, k_tan_apply around the adjoint's two sweeps): dz, dlam along nd directions
 * (dq, dr, db, dx0) at the point of the last solve, and the predictor that builds its one direction on the device ---- */
namespace {
/* the tangent's buffers, on first use and again when nd grows or nx0 changed: one zeroed device block, the pinned block, the LDS windows */
int setup_tan(tqgpu_solver *s, int nd) {
    int rc;
    MpcTan &m = s->tan;
    const size_t snx = (size_t)s->sum_nx, snu = (size_t)s->sum_nu, nxe = snx - (size_t)s->x_pad, sl = (size_t)s->sum_lam, nx0 = (size_t)s->mpc.nx0, nu0 = (size_t)s->nu[0];
    if (!m.d || nd > m.nd_cap || m.nx0 != s->mpc.nx0) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->mem.release(m.d); s->mem.release(m.h);
        s->sens.tan_valid = false; m.nd_cap = 0;
        const size_t cap = (size_t)nd, staged = (nxe + snu + sl + nx0) * cap, io = nu0 * cap + 1 + nx0 + nu0 + 2;
        size_t off = 0;
        auto take = [&](size_t n) { const size_t o = off; off += (n + 1) / 2 * 2; return o; };
        const size_t os = take(staged), oY = take(snx * cap), ot = take(snx * cap), ox = take(snx * cap), ou = take(snu * cap), ol = take(snx * cap), oh = take(nu0 * cap + 1);
        if ((rc = s->mem.zeroed(m.d, sizeof(double) * std::max<size_t>(off, 2), TQGPU_ENOMEM, "the tangent")) ||
            (rc = s->mem.host(m.h, sizeof(double) * (staged + io + 2), "the pinned directions and du0")))
            return rc;
        memset(m.h, 0, sizeof(double) * (staged + io + 2));
        size_t lds = 0;
        for (int k = 0; k < s->Nn; k++) lds = std::max(lds, (2 * (size_t)(s->nx[k] + s->nu[k]) + 2) * sizeof(double));
        if ((rc = allow_lds(k_tan_rhs, lds)) || (rc = allow_lds(k_adj_backward, s->pp.lds_forward)) || (rc = allow_lds(k_adj_forward, s->pp.lds_forward)) || (rc = allow_lds(k_tan_primal, lds)))
            return rc;
        Tan &X = m.v;
        X = Tan{};
        double *p = m.d;
        m.stage_d = p + os;
        X.a.Y = p + oY; X.a.t = p + ot; X.a.gq = p + ox; X.a.gr = p + ou; X.a.gb = p + ol; X.a.head = p + oh;
        X.a.nxe = (int)nxe; X.sum_lam = s->sum_lam;
        m.io = m.h + staged;
        m.nd_cap = nd; m.nx0 = s->mpc.nx0; m.lds = lds;
    }
    m.v.a.nw = nd;
    return TQGPU_OK;
}
/* where the head, x0_new and the predictor's results lie in the pinned block */
double *tan_io_x0(const tqgpu_solver *s) { return s->tan.io + (size_t)s->nu[0] * (size_t)s->tan.nd_cap + 1; }
double *tan_io_out(const tqgpu_solver *s) { return tan_io_x0(s) + (size_t)s->mpc.nx0; }
int tan_need(const tqgpu_solver *s, const char *who) {
    if (!s->sens.tan_valid) return fail(TQGPU_EINVAL, std::string(who) + ": no tangent has been computed for the point and the data the device holds now (tqgpu_mpc_tangent or tqgpu_mpc_predict_at after the last solve, upload and fold)");
    return TQGPU_OK;
}
/* what the tangent refuses beyond sens_refuse, before anything is touched: the windows of the adjoint (nd for nw) and of the factorisation */
int tan_window_refuse(const tqgpu_solver *s, int nd) {
    int rc;
    size_t lf, lp;
    if ((rc = adj_window_refuse(s, nd)) || (rc = sens_window_refuse(s, lf, lp))) return rc;
    return TQGPU_OK;
}
/* the launches behind the direction: [the factor, where none is stored] k_tan_rhs, the adjoint's two sweeps on the tangent's Y and t, k_tan_primal.
 * S: the view the launches took, kept for tan_store behind the wait */
int tan_enqueue(tqgpu_solver *s, const Opts &O, const Tan &X, Sens &S) {
    int rc;
    MpcSens &m = s->sens;
    S = m.v;
    if (!m.factored && (rc = sens_enqueue_factor(s, O, S))) return rc;
    const Tree &T = s->T;
    hipStream_t st = s->stream;
    const Adj A = X.a;
    const unsigned cols = (unsigned)A.nw;
    hipLaunchKernelGGL(k_tan_rhs, dim3(T.Np, cols), dim3(WAVE), s->tan.lds, st, T, s->D, S, X);
    for_levels(s, Walk::to_root, [&](int first, int count) { hipLaunchKernelGGL(k_adj_backward, dim3(count, cols), dim3(WAVE), s->pp.lds_forward, st, T, S, A, first); });
    for_levels(s, Walk::to_leaves, [&](int first, int count) { hipLaunchKernelGGL(k_adj_forward, dim3(count, cols), dim3(WAVE), s->pp.lds_forward, st, T, S, A, first); });
    hipLaunchKernelGGL(k_tan_primal, dim3(T.Nn, cols), dim3(WAVE), s->tan.lds, st, T, s->D, S, X);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1 + T.Nh + (T.Nh - 1) + 1);
    return TQGPU_OK;
}
/* a finished tangent onto its mirror, behind the wait: the factor counts as stored, a stored sensitivity and a stored adjoint stay as they were */
void tan_store(tqgpu_solver *s, const Sens &S, const Tan &X, int nd, int *n_reg) {
    s->sens.v = S; s->sens.factored = true; s->sens.tan_valid = true;
    s->tan.v = X; s->tan.nd = nd;
    if (n_reg) *n_reg = (int)s->tan.io[(size_t)s->nu[0] * (size_t)nd];
}
}  // namespace

extern "C" int tqgpu_mpc_tangent(tqgpu_solver *s, const tqgpu_opts *o, const double *dq, const double *dr, const double *db, const double *dx0, int nd, int *n_reg) {
    const char *who = "tqgpu_mpc_tangent";
    int rc;
    if ((rc = sens_refuse(s, o, who))) return rc;
    if (nd < 1) return fail(TQGPU_EINVAL, std::string(who) + ": nd must be at least 1");
    if (!dq && !dr && !db && !dx0) return fail(TQGPU_EINVAL, std::string(who) + ": no direction (dq, dr, db and dx0 are all NULL)");
    if ((rc = tan_window_refuse(s, nd))) return rc;
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    if ((rc = setup_sens(s)) || (rc = setup_tan(s, nd))) return rc;
    s->sens.tan_valid = false;
    MpcTan &m = s->tan;
    const size_t nw = adj_w_doubles(s, nd), nb = db ? (size_t)s->sum_lam * nd : 0, n0 = dx0 ? (size_t)s->mpc.nx0 * nd : 0, nu0 = (size_t)s->nu[0];
    hipStream_t st = s->stream;
    /* the directions through pinned memory in one copy: [dq | dr] as the adjoint's w (a missing one as zeros), then db and dx0 where given */
    adj_stage_w(s, m.h, dq, dr, nd);
    if (nb) memcpy(m.h + nw, db, sizeof(double) * nb);
    if (n0) memcpy(m.h + nw + nb, dx0, sizeof(double) * n0);
    if (nw + nb + n0) { HIP_TRY(hipMemcpyAsync(m.stage_d, m.h, sizeof(double) * (nw + nb + n0), hipMemcpyHostToDevice, st)); }
    MPC_COUNT(copies, 1);
    Tan X = m.v;
    X.built = 0; X.x0_new = nullptr; X.xtraj = X.utraj = nullptr; X.stage = nullptr;
    X.a.wx = m.stage_d; X.a.wu = m.stage_d + (size_t)X.a.nxe * (size_t)nd;
    X.db = nb ? m.stage_d + nw : nullptr; X.dx0 = n0 ? m.stage_d + nw + nb : nullptr;
    Sens S;
    if ((rc = tan_enqueue(s, O, X, S))) return rc;
    HIP_TRY(hipMemcpyAsync(m.io, X.a.head, sizeof(double) * (nu0 * nd + 1), hipMemcpyDeviceToHost, st)); MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    tan_store(s, S, X, nd, n_reg);
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_get_tangent_u0(tqgpu_solver *s, double *du0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_tangent_u0")) || (rc = tan_need(s, "tqgpu_mpc_get_tangent_u0"))) return rc;
    const size_t n = (size_t)s->nu[0] * (size_t)s->tan.nd;
    if (du0 && n) memcpy(du0, s->tan.io, sizeof(double) * n);
    return TQGPU_OK;
}

/* a diagnostic download (whole buffers through pageable memory, repacked on the host): not counted into tqgpu_mpc_stats */
extern "C" int tqgpu_mpc_get_tangent(tqgpu_solver *s, double *dx, double *du, double *dlam) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_tangent")) || (rc = tan_need(s, "tqgpu_mpc_get_tangent"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t nd = (size_t)s->tan.nd, snu = (size_t)s->sum_nu;
    const Adj &A = s->tan.v.a;
    if (dx && (rc = download_columns(s, A.gq, nd, (size_t)s->x_pad, (size_t)(s->sum_nx - s->x_pad), dx))) return rc;      /* phantom root states are left out */
    if (dlam && (rc = download_columns(s, A.gb, nd, (size_t)s->nx0, (size_t)s->sum_lam, dlam))) return rc;                  /* the root has no dual */
    if (du && snu * nd) HIP_TRY(hipMemcpy(du, A.gr, sizeof(double) * snu * nd, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* one direction built on the device (Tan::built): x0_new in and [u0_pred | n_clipped | n_reg] back through the pinned block, which k_tan_rhs, k_tan_primal
 * and k_tan_apply read and write in place; the head [du0 | n_reg] in one copy, for tqgpu_mpc_get_tangent_u0 */
extern "C" int tqgpu_mpc_predict_at(tqgpu_solver *s, const tqgpu_opts *o, const double *x0_new, int t0_new, double *u0_pred, int duals, int *n_clipped, int *n_reg) {
    const char *who = "tqgpu_mpc_predict_at";
    int rc;
    if ((rc = sens_refuse(s, o, who)) || (rc = mpc_take_window(s, t0_new, false, who))) return rc;
    if (t0_new >= 0 && s->trk.t0 < 0) return fail(TQGPU_EINVAL, std::string(who) + ": no window is in force yet (tqgpu_mpc_set_window, tqgpu_mpc_step_at): there is no reference row to measure the move from");
    if ((rc = tan_window_refuse(s, 1))) return rc;
    Opts O;
    if ((rc = opts_from(o, O))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    if ((rc = setup_sens(s)) || (rc = setup_tan(s, 1))) return rc;
    s->sens.tan_valid = false;
    MpcTan &m = s->tan;
    const size_t nx0 = (size_t)s->mpc.nx0, nu0 = (size_t)s->nu[0];
    hipStream_t st = s->stream;
    double *x0n = tan_io_x0(s), *out = tan_io_out(s);
    if (x0_new && nx0) memcpy(x0n, x0_new, sizeof(double) * nx0);
    Tan X = m.v;
    X.built = 1; X.db = X.dx0 = nullptr; X.a.wx = X.a.wu = nullptr;
    X.x0_new = x0_new ? x0n : nullptr;
    X.xtraj = X.utraj = nullptr; X.stage = nullptr;
    if (t0_new >= 0) {
        const double *p = s->trk.d;
        X.xtraj = p; p += (size_t)s->trk.T * s->trk.nxt; X.utraj = p; p += (size_t)s->trk.T * s->trk.nut;
        p += (size_t)s->sum_nx + (size_t)s->sum_nu;          /* q0, r0: the bases drop out of the difference */
        X.stage = reinterpret_cast<const int *>(p);
        X.t0 = s->trk.t0; X.t1 = t0_new; X.Tn = s->trk.T; X.nxt = s->trk.nxt; X.nut = s->trk.nut;
    }
    Sens S;
    if ((rc = tan_enqueue(s, O, X, S))) return rc;
    double *keep = nullptr;
    if ((rc = predict_keep(s, duals, keep))) return rc;
    hipLaunchKernelGGL(k_tan_apply, dim3(duals ? 1 + (unsigned)s->Nn : 1u), dim3(WAVE), 0, st, s->T, s->D, S, X, s->d_lam_init, keep, out);
    HIP_TRY(hipGetLastError()); MPC_COUNT(launches, 1);
    predict_lent(s, duals);
    HIP_TRY(hipMemcpyAsync(m.io, X.a.head, sizeof(double) * (nu0 + 1), hipMemcpyDeviceToHost, st)); MPC_COUNT(copies, 1);
    HIP_TRY(hipStreamSynchronize(st)); MPC_COUNT(waits, 1);
    tan_store(s, S, X, 1, nullptr);
    if (u0_pred && nu0) memcpy(u0_pred, out, sizeof(double) * nu0);
    if (n_clipped) *n_clipped = (int)out[nu0];
    if (n_reg) *n_reg = (int)out[nu0 + 1];
    return TQGPU_OK;
}

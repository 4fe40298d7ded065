/*
 * tdunes_problem.hpp -- what problem the mirror holds and which stage solver each node runs, in the host part: the setters of the dynamics, the
 * objective (diagonal, dense, mixed kinds), the bounds, the general constraints, the starting duals and the whole clipping QP (tqgpu_set_problem),
 * the getters of the sizes and of the rows' results, the hot-start switch of stage_gen and the two opt-ins of the single-workgroup dense solve.
 * No kernel here.  Included once from tdunes_device.hip inside #if TQ_HAS(TQP_HOST), ahead of the solve and of tdunes_mpc.hpp (problem_changed).
 * tdunes_mirror.hpp keeps the mirror's records StageKinds, GenRows, DenseSingle; tdunes_device.hip keeps allow_lds.
 */
#pragma once

extern "C" int tqgpu_dims(const tqgpu_solver *s, int *sum_nx, int *sum_nu, int *sum_lam, int *sum_A, int *sum_B) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (sum_nx) *sum_nx = s->sum_nx - s->x_pad;
    if (sum_nu) *sum_nu = s->sum_nu;
    if (sum_lam) *sum_lam = s->sum_lam;
    if (sum_A) *sum_A = s->sum_A - s->A_pad;
    if (sum_B) *sum_B = s->sum_B;
    return TQGPU_OK;
}

/* THE statement of what a change of the problem's data on the device makes stale: the pinned mirror of tqgpu_set_problem's inputs, a stored
 * sensitivity and the pairing of the last solve's point with the data; repack: the packed constants of the persistent route as well */
static void problem_changed(tqgpu_solver *s, bool repack) {
    s->in_valid = false;
    s->sens.invalidate(); s->sens.dirty = true; if (repack) s->persist.need_pack = true;
}
/* THE return to the clipping solver (tqgpu_set_objective_diag, tqgpu_set_problem): the dense kinds are off, the fast paths the tree had at
 * creation are back; the kinds, H and the plan of plan_dense_single stay as they were set.  true: the mirror was dense */
static bool back_to_clipping(tqgpu_solver *s) {
    if (!s->sk.dense) return false;
    s->sk.dense = false; s->sk.box = false; s->sk.gen = false; s->D.dense = 0; s->uni.use_fast = s->uni.use_fast_orig;
    return true;
}

#define H2D(dst, src, count)                                                                                   \
    do {                                                                                                       \
        if ((src) && (count) > 0)                                                                              \
            HIP_TRY(hipMemcpyAsync((dst), (src), sizeof(double) * (size_t)(count), hipMemcpyHostToDevice, s->stream)); \
    } while (0)

extern "C" int tqgpu_set_dynamics(tqgpu_solver *s, const double *A, const double *B, const double *b) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    problem_changed(s, true);
    H2D(s->A + s->A_pad, A, s->sum_A - s->A_pad); H2D(s->B, B, s->sum_B);
    H2D(s->b + s->nx0, b, s->sum_lam);              /* node-indexed on the device: root slot unused */
    HIP_TRY(hipStreamSynchronize(s->stream));       /* the caller may reuse its buffers */
    return TQGPU_OK;
}

extern "C" int tqgpu_set_objective_diag(tqgpu_solver *s, const double *Qd, const double *Rd, const double *q, const double *r) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    problem_changed(s, true);
    H2D(s->Qd + s->x_pad, Qd, s->sum_nx - s->x_pad); H2D(s->Rd, Rd, s->sum_nu); H2D(s->q + s->x_pad, q, s->sum_nx - s->x_pad); H2D(s->r, r, s->sum_nu);
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->need_init = true;
    (void)back_to_clipping(s);
    return TQGPU_OK;
}

/* The linear terms alone, in the layout of tqgpu_set_objective_diag (either may be NULL: left alone): q and r are uploaded and the persistent
 * route packs them again; the kinds, H, the factors of k_init / k_dense_init and the stored working sets of kinds 2 and 3 stay. */
extern "C" int tqgpu_set_linear_terms(tqgpu_solver *s, const double *q, const double *r) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "tqgpu_set_linear_terms: null solver");
    HIP_TRY(hipSetDevice(s->device));
    problem_changed(s, true);
    H2D(s->q + s->x_pad, q, s->sum_nx - s->x_pad); H2D(s->r, r, s->sum_nu);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}
extern "C" int tqgpu_get_linear_terms(tqgpu_solver *s, double *q, double *r) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "tqgpu_get_linear_terms: null solver");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int nxe = s->sum_nx - s->x_pad;
    if (q && nxe > 0) HIP_TRY(hipMemcpy(q, s->q + s->x_pad, sizeof(double) * (size_t)nxe, hipMemcpyDeviceToHost));
    if (r && s->sum_nu > 0) HIP_TRY(hipMemcpy(r, s->r, sizeof(double) * (size_t)s->sum_nu, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* Dense objective for the dense UNCONSTRAINED stage solver (the reference's qpOASES stage backend restricted
 * to nodes without bounds, dual_Newton_tree_qpoases.c:153-217,401-476).  Flat layout of
 * tree_qp_in_set_ltv_objective_colmajor (tree_qp_common.c): per node Q (nx x nx), R (nu x nu), S (nu x nx),
 * all column major, then q, r.  Selects the generic device path; tqgpu_set_objective_diag selects clipping again. */
extern "C" int tqgpu_set_objective_dense(tqgpu_solver *s, const double *Q, const double *R, const double *S, const double *q, const double *r) {
    SETTLE(s);
    return tqgpu_set_objective_mixed(s, nullptr, Q, R, S, q, r);
}

namespace {
/* lb <= ub on every entry of every box node (the phantom root states are not the caller's) */
int check_box_bounds(const tqgpu_solver *s) {
    if (!(s->sk.box || s->sk.gen) || s->sk.h_bounds.empty()) return TQGPU_OK;
    const double *xl = s->sk.h_bounds.data(), *xu = xl + s->sum_nx, *ul = xu + s->sum_nx, *uu = ul + s->sum_nu;
    for (int k = 0; k < s->Nn; k++) {
        if (s->sk.h_kind[(size_t)k] < 2) continue;
        for (int i = (k == 0 ? s->x_pad : 0); i < s->nx[k]; i++)
            if (!(xl[s->xoff[k] + i] <= xu[s->xoff[k] + i])) return fail(TQGPU_EINVAL, "box node " + std::to_string(k) + ": xmin > xmax");
        for (int i = 0; i < s->nu[k]; i++)
            if (!(ul[s->uoff[k] + i] <= uu[s->uoff[k] + i])) return fail(TQGPU_EINVAL, "box node " + std::to_string(k) + ": umin > umax");
    }
    return TQGPU_OK;
}
/* The kinds the caller asked for become the kinds of the device (a kind-3 node that has no rows is a kind-2 node), with the LDS of
 * the sweeps that serve them.  On failure nothing has changed. */
int apply_kinds(tqgpu_solver *s, const std::vector<int> &req) {
    std::vector<int> kd = req;
    size_t lds_box = 0, lds_gen = 0;
    for (int k = 0; k < s->Nn; k++) {
        if (kd[(size_t)k] < 2) continue;
        const size_t nz = (size_t)s->nx[k] + s->nu[k], nc = s->rows.nc.empty() ? 0 : (size_t)s->rows.nc[(size_t)k];
        if (nz > WAVE) return fail(TQGPU_EUNSUPPORTED, "box node " + std::to_string(k) + ": nx + nu = " + std::to_string(nz) + " > 64 (one wave, one entry per lane)");
        if (kd[(size_t)k] == 3 && (nc == 0 || nz == 0)) kd[(size_t)k] = 2;
        const size_t head = (size_t)s->bdim[k] + s->nx[k] + 2 * nz + 2;
        if (kd[(size_t)k] == 2) lds_box = std::max(lds_box, (head + 2 * nz * nz) * sizeof(double));
        else lds_gen = std::max(lds_gen, (head + nc + 2 * nz * nz + nz * nc + nc * nc) * sizeof(double));
    }
    const bool box_was = s->sk.box, gen_was = s->sk.gen;
    const std::vector<int> kind_was = s->sk.h_kind;
    s->sk.box = lds_box > 0; s->sk.gen = lds_gen > 0; s->sk.h_kind = kd;
    int rc = check_box_bounds(s);
    if (rc == TQGPU_OK && s->sk.gen) rc = allow_lds(k_stage_gen, std::max(std::max(s->pp.lds_stage, lds_box), lds_gen));
    else if (rc == TQGPU_OK && s->sk.box) rc = allow_lds(k_stage_box, std::max(s->pp.lds_stage, lds_box));
    if (rc != TQGPU_OK) { s->sk.box = box_was; s->sk.gen = gen_was; s->sk.h_kind = kind_was; return rc; }
    s->sk.lds_box = std::max(s->pp.lds_stage, lds_box);
    s->sk.lds_gen = std::max(s->sk.lds_box, lds_gen);
    s->sk.h_kind_req = req;
    return TQGPU_OK;
}
/* The LDS plan of g_persist_dense for the kinds and rows the mirror has now (they decide the stage windows, so this runs where they are
 * set, not at creation).  The window region holds GPD_WAVES windows of the other phases (gp.lds_wave doubles each; fewer waves take
 * blocks where that many do not fit: the Hessian window of a node with nz = 64 and 40 child states is 40 KiB) or, overlaid,
 * stage_waves windows of the tree's largest stage need (lds_stage / lds_box / lds_gen); behind it the index tables and, while they
 * fit, the state mirror and the constants, as in setup_single_wg.  stage_waves is the largest count <= GPD_WAVES for which the total
 * stays within setup_single_wg's 150 KiB; 0 (or a size the runtime refuses): not eligible. */
void plan_dense_single(tqgpu_solver *s) {
    s->gpd = DenseSingle{s->gpd.single, s->gpd.batch};      /* the caller's two choices stay */
    if (!s->sk.dense) return;
    constexpr size_t budget = 150 * 1024;
    int widest = 0;
    for (int l = 0; l <= s->Nh; l++) widest = std::max(widest, s->lvl_first[l + 1] - s->lvl_first[l]);
    const size_t per_wave = s->gp.lds_wave;
    if (widest > 6 * GP_WAVES) return;      /* the width test of setup_single_wg */
    /* the level table (setup_single_wg uploads it only for trees g_persist takes; the dense kernel reads the first nodes of the levels, never the groups) */
    if (!s->gp.d_lvl_first && s->mem.upload(s->gp.d_lvl_first, s->lvl_first.data(), sizeof(int) * s->lvl_first.size(), TQGPU_ENOMEM, "the level table") != TQGPU_OK) return;
    const size_t win = ((s->sk.gen ? s->sk.lds_gen : s->sk.box ? s->sk.lds_box : s->pp.lds_stage) + 15) / 16 * 2;      /* doubles, even: the windows stay 16-byte aligned */
    auto ev = [](size_t n) { return (n + 1) & ~(size_t)1; };
    const size_t sx = (size_t)s->sum_nx, su = (size_t)s->sum_nu;
    const size_t mirror = 11 * ev(sx) + 5 * ev(su) + 2 * ev((size_t)s->sum_W) + 2 * ev((size_t)s->sum_Ut) + 2 * ev((size_t)s->Nn) + ev(sx + s->Nn + 1);
    const size_t tables = (13 * ((size_t)s->Nn + 3)) / 2 + 16;
    const size_t consts = ev((size_t)s->sum_A) + ev((size_t)s->sum_B) + 5 * ev(sx) + 4 * ev(su);
    int sw = 0, pw = 0;
    for (int w = GPD_WAVES; w >= 1 && !pw; w--) if ((per_wave * w + tables + 8) * 8 <= budget) pw = w;
    for (int w = GPD_WAVES; w >= 1 && !sw; w--) if ((win * w + tables + 8) * 8 <= budget) sw = w;
    if (!sw || !pw) return;
    const size_t region = std::max(per_wave * (size_t)pw, win * (size_t)sw);
    size_t total = (region + tables + 8) * 8;
    s->gpd.tab_in_lds = true;
    if (total + mirror * 8 <= budget) { s->gpd.in_lds = true; total += mirror * 8; }
    if (s->gpd.in_lds && total + consts * 8 <= budget) { s->gpd.const_in_lds = true; total += consts * 8; }
    if (total > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(g_persist_dense), hipFuncAttributeMaxDynamicSharedMemorySize, (int)total) != hipSuccess) {
        (void)hipGetLastError();
        s->gpd.in_lds = s->gpd.const_in_lds = s->gpd.tab_in_lds = false;
        return;
    }
    s->gpd.stage_waves = sw; s->gpd.phase_waves = pw; s->gpd.win_stage = win; s->gpd.win_region = region; s->gpd.lds_total = total;
    s->gpd.ok = true;
}
/* the host side of tqgpu_set_objective_mixed, no HIP call: the kinds asked for (kind == NULL: all 1) with the LDS of k_dense_init, refused where one is
 * no kind or a dense node does not fit; then H of the dense nodes and the diagonal weights Qd, Rd of the clipping nodes (zero elsewhere), in the
 * device's layout, from the caller's Q, R, S */
int mixed_kinds(const tqgpu_solver *s, const int *kind, std::vector<int> &kd, size_t &lds_dense) {
    kd.assign((size_t)s->Nn, 1);
    if (kind) for (int k = 0; k < s->Nn; k++) {
        if (kind[k] < 0 || kind[k] > 3) return fail(TQGPU_EINVAL, "tqgpu_set_objective_mixed: kind must be 0, 1, 2 or 3");
        kd[(size_t)k] = kind[k];
    }
    lds_dense = 0;
    for (int k = 0; k < s->Nn; k++) {
        /* k_dense_init holds a dense node's H (nz x nz) and its pivots in LDS */
        const size_t nzd = (size_t)s->nx[k] + s->nu[k];
        if (kd[(size_t)k]) lds_dense = std::max(lds_dense, (nzd * (nzd + 1) + 2) * sizeof(double));
    }
    if (lds_dense > 160 * 1024) return fail(TQGPU_EUNSUPPORTED, "dense node too large for the LDS-resident factorization of H (160 KiB per workgroup)");
    return TQGPU_OK;
}
void mixed_weights(const tqgpu_solver *s, const std::vector<int> &kd, const double *Q, const double *R, const double *S,
                   std::vector<double> &H, std::vector<double> &Qd, std::vector<double> &Rd) {
    H.assign((size_t)std::max(s->poff[s->Nn], 1), 0.0); Qd.assign((size_t)std::max(s->sum_nx, 1), 0.0); Rd.assign((size_t)std::max(s->sum_nu, 1), 0.0);
    size_t oq = 0, orr = 0, os = 0;
    for (int k = 0; k < s->Nn; k++) {
        const int nu = s->nu[k], nz = s->nx[k] + nu;
        double *Hk = H.data() + s->poff[k];
        if (!kd[(size_t)k]) {
            /* clipping node: diagonal weights (phantom root states of an embedded x0-eliminated tree keep their unit weight) */
            const int nxc = s->nx[k] - ((k == 0) ? s->x_pad : 0);
            for (int i = 0; i < ((k == 0) ? s->x_pad : 0); i++) Qd[(size_t)i] = 1.0;
            for (int i = 0; i < nxc; i++) Qd[(size_t)s->xoff[k] + ((k == 0) ? s->x_pad : 0) + i] = Q[oq + i + (size_t)i * nxc];
            for (int i = 0; i < nu; i++) Rd[(size_t)s->uoff[k] + i] = R ? R[orr + i + (size_t)i * nu] : 0.0;
            oq += (size_t)nxc * nxc; orr += (size_t)nu * nu; os += (size_t)nu * nxc;
            continue;
        }
        if (k == 0 && s->x_pad) {
            /* phantom root states: identity weight, no coupling; the caller's node 0 has no Q and no S */
            for (int i = 0; i < s->x_pad; i++) Hk[i + (size_t)i * nz] = 1.0;
            for (int j = 0; j < nu; j++) for (int i = 0; i < nu; i++) Hk[s->x_pad + i + (size_t)(s->x_pad + j) * nz] = R ? R[orr + i + (size_t)j * nu] : 0.0;
            orr += (size_t)nu * nu;
            continue;
        }
        const int nx = s->nx[k];
        for (int j = 0; j < nx; j++) for (int i = 0; i < nx; i++) Hk[i + (size_t)j * nz] = Q[oq + i + (size_t)j * nx];
        for (int j = 0; j < nu; j++) for (int i = 0; i < nu; i++) Hk[nx + i + (size_t)(nx + j) * nz] = R ? R[orr + i + (size_t)j * nu] : 0.0;
        for (int j = 0; j < nx; j++) for (int i = 0; i < nu; i++) {          /* S is nu x nx */
            const double v = S ? S[os + i + (size_t)j * nu] : 0.0;
            Hk[nx + i + (size_t)j * nz] = v;
            Hk[j + (size_t)(nx + i) * nz] = v;
        }
        oq += (size_t)nx * nx; orr += (size_t)nu * nu; os += (size_t)nu * nx;
    }
}
}  // namespace

/* The same with a per-node choice of the stage solver (opts->qp_solver[] of the reference, dual_Newton_tree.c:124-162):
 * kind[k] = 0: clipping (the diagonals of Q_k, R_k are its weights; their off-diagonals and S_k must be zero), 1: dense
 * unconstrained, 2: dense with the box bounds of tqgpu_set_bounds (stage_box; nx + nu <= 64).  kind == NULL: every node
 * dense unconstrained. */
extern "C" int tqgpu_set_objective_mixed(tqgpu_solver *s, const int *kind, const double *Q, const double *R, const double *S, const double *q, const double *r) {
    SETTLE(s);
    if (!s || !Q || !q) return fail(TQGPU_EINVAL, "tqgpu_set_objective_mixed: bad arguments");
    if (s->shard.on) return fail(TQGPU_EINVAL, "the dense stage solver is not available in sharded mode");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<double> H, Qd, Rd;
    std::vector<int> kd;
    size_t lds_dense = 0;
    int rc;
    if ((rc = mixed_kinds(s, kind, kd, lds_dense)) || (rc = allow_lds(k_dense_init, lds_dense)) || (rc = apply_kinds(s, kd))) return rc;
    mixed_weights(s, kd, Q, R, S, H, Qd, Rd);
    problem_changed(s, false);          /* (dense nodes: no packed constants, uni.use_fast goes to 0 below) */
    H2D(s->sk.d_Hd, H.data(), s->poff[s->Nn]);
    HIP_TRY(hipMemcpyAsync(s->sk.d_kind, s->sk.h_kind.data(), sizeof(int) * (size_t)s->Nn, hipMemcpyHostToDevice, s->stream));      /* ints: not H2D (doubles) */
    H2D(s->q + s->x_pad, q, s->sum_nx - s->x_pad); H2D(s->r, r, s->sum_nu);
    /* weights: zero on dense nodes (k_export_all writes zero multipliers for them; k_export_box those of the box nodes), the diagonals
     * on clipping nodes */
    H2D(s->Qd, Qd.data(), s->sum_nx); H2D(s->Rd, Rd.data(), s->sum_nu);
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->sk.lds_dense = lds_dense;
    s->sk.dense = true; s->sk.need_dense_init = true; s->D.dense = 1; s->need_init = true;
    s->uni.use_fast = 0;                                       /* per-node dense blocks: generic kernels */
    plan_dense_single(s);
    return TQGPU_OK;
}

extern "C" int tqgpu_set_bounds(tqgpu_solver *s, const double *xmin, const double *xmax, const double *umin, const double *umax) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    problem_changed(s, true);
    if (xmin && xmax && umin && umax) {
        /* keep what the box nodes' checks need (lb <= ub); refuse before anything is uploaded */
        std::vector<double> hb((size_t)2 * s->sum_nx + 2 * (size_t)s->sum_nu, 0.0);
        const size_t nxe = (size_t)(s->sum_nx - s->x_pad);
        std::copy(xmin, xmin + nxe, hb.begin() + s->x_pad); std::copy(xmax, xmax + nxe, hb.begin() + s->sum_nx + s->x_pad);
        std::copy(umin, umin + s->sum_nu, hb.begin() + 2 * (size_t)s->sum_nx); std::copy(umax, umax + s->sum_nu, hb.begin() + 2 * (size_t)s->sum_nx + s->sum_nu);
        hb.swap(s->sk.h_bounds);
        const int rc = check_box_bounds(s);
        if (rc != TQGPU_OK) { hb.swap(s->sk.h_bounds); return rc; }
    } else s->sk.h_bounds.clear();
    H2D(s->xmin + s->x_pad, xmin, s->sum_nx - s->x_pad); H2D(s->xmax + s->x_pad, xmax, s->sum_nx - s->x_pad); H2D(s->umin, umin, s->sum_nu); H2D(s->umax, umax, s->sum_nu);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}

namespace {
/* the steps of tqgpu_set_constraints, in its order */
/* the rows per node within a wave, and dmin <= dmax in every row of what the mirror would hold (dr: dmin | dmax, `total` rows each); touches nothing */
int rows_check(const tqgpu_solver *s, const int *nc, const double *dmin, const double *dmax, int &total, std::vector<double> &dr) {
    const GenRows &g = s->rows;
    if (nc) for (int k = 0; k < s->Nn; k++) {
        if (nc[k] < 0) return fail(TQGPU_EINVAL, "tqgpu_set_constraints: negative number of rows");
        if (nc[k] > WAVE) return fail(TQGPU_EUNSUPPORTED, "node " + std::to_string(k) + ": nc = " + std::to_string(nc[k]) + " > 64 (one wave, one row per lane)");
    }
    total = nc ? std::accumulate(nc, nc + s->Nn, 0) : g.sum_nc;
    dr.resize((size_t)2 * total);
    for (int i = 0; i < total; i++) {
        dr[(size_t)i] = dmin ? dmin[i] : (nc ? -__builtin_inf() : g.h_drange[(size_t)i]);
        dr[(size_t)total + i] = dmax ? dmax[i] : (nc ? __builtin_inf() : g.h_drange[(size_t)g.sum_nc + i]);
        if (!(dr[(size_t)i] <= dr[(size_t)total + i])) return fail(TQGPU_EINVAL, "tqgpu_set_constraints: dmin > dmax in row " + std::to_string(i));
    }
    return TQGPU_OK;
}
/* new rows: the kinds planned again for them (refused: the rows stay as they were), the tables, the device blocks (zeroed: no rows of G, no
 * working sets, no multipliers), the record Data.gen points to, the kinds of the device */
int rows_define(tqgpu_solver *s, const int *nc, int total) {
    GenRows &g = s->rows;
    const int Nn = s->Nn;
    const std::vector<int> nc_was = g.nc;
    g.nc.assign(nc, nc + Nn);
    if (s->sk.dense) { const int rck = apply_kinds(s, s->sk.h_kind_req); if (rck != TQGPU_OK) { g.nc = nc_was; return rck; } plan_dense_single(s); }
    g.roff.assign((size_t)Nn + 1, 0); g.goff.assign((size_t)Nn + 1, 0);
    for (int k = 0; k < Nn; k++) {
        g.roff[(size_t)k + 1] = g.roff[(size_t)k] + nc[k];
        g.goff[(size_t)k + 1] = g.goff[(size_t)k] + nc[k] * (s->nx[k] + s->nu[k]);
    }
    g.sum_nc = total;
    s->mem.release(g.d_tab); s->mem.release(g.d_Gt); s->mem.release(g.d_drange); s->mem.release(g.d_mu); s->mem.release(g.d_rmask); s->mem.release(g.d_steps); s->mem.release(g.d_gen);
    std::vector<int> tab(g.nc);
    tab.insert(tab.end(), g.roff.begin(), g.roff.end()); tab.insert(tab.end(), g.goff.begin(), g.goff.end());
    int rc;
    if ((rc = s->mem.upload(g.d_tab, tab.data(), tab.size() * sizeof(int), TQGPU_ENOMEM, "the tables of the general constraints")) ||
        (rc = s->mem.zeroed(g.d_Gt, sizeof(double) * (size_t)std::max(g.goff[(size_t)Nn], 1), TQGPU_ENOMEM, "the rows of the general constraints")) ||
        (rc = s->mem.zeroed(g.d_drange, sizeof(double) * (size_t)std::max(2 * total, 1), TQGPU_ENOMEM, "the ranges of the general constraints")) ||
        (rc = s->mem.zeroed(g.d_mu, sizeof(double) * (size_t)std::max(total, 1), TQGPU_ENOMEM, "the multipliers of the general constraints")) ||
        (rc = s->mem.zeroed(g.d_rmask, sizeof(unsigned long long) * 4 * (size_t)Nn, TQGPU_ENOMEM, "the working sets of the general constraints")) ||
        (rc = s->mem.zeroed(g.d_steps, (sizeof(long) + sizeof(int)) * (size_t)Nn, TQGPU_ENOMEM, "the step counters of the general constraints")))
        return rc;
    Gen v;
    v.nc = g.d_tab; v.roff = g.d_tab + Nn; v.goff = g.d_tab + 2 * Nn + 1;
    v.Gt = g.d_Gt; v.dmin = g.d_drange; v.dmax = g.d_drange + total; v.mu = g.d_mu; v.rmask = g.d_rmask;
    v.sides = g.d_rmask + 2 * (size_t)Nn; v.hot = g.hot ? 1 : 0;
    v.steps_total = g.d_steps; v.steps_last = reinterpret_cast<int *>(g.d_steps + Nn);
    if ((rc = s->mem.upload(g.d_gen, &v, sizeof(Gen), TQGPU_ENOMEM, "the record of the general constraints"))) return rc;
    g.h_gen = v;
    s->D.gen = g.d_gen;
    if (s->sk.dense) HIP_TRY(hipMemcpy(s->sk.d_kind, s->sk.h_kind.data(), sizeof(int) * (size_t)Nn, hipMemcpyHostToDevice));
    s->sk.need_dense_init = true;
    return TQGPU_OK;
}
/* rows of G = [C | D] (the phantom root states keep their zero columns); what is not given stays */
int rows_upload_G(tqgpu_solver *s, const double *C, const double *Dm) {
    const GenRows &g = s->rows;
    const int Nn = s->Nn;
    std::vector<double> Gt((size_t)std::max(g.goff[(size_t)Nn], 1), 0.0);
    if (!(C && Dm)) HIP_TRY(hipMemcpy(Gt.data(), g.d_Gt, sizeof(double) * (size_t)g.goff[(size_t)Nn], hipMemcpyDeviceToHost));
    size_t oc = 0, od = 0;
    for (int k = 0; k < Nn; k++) {
        const int pad = k == 0 ? s->x_pad : 0, nxc = s->nx[k] - pad, nu = s->nu[k], nz = s->nx[k] + nu, m = g.nc[(size_t)k];
        double *Gk = Gt.data() + g.goff[(size_t)k];
        if (C) for (int j = 0; j < nxc; j++) for (int r = 0; r < m; r++) Gk[(size_t)r * nz + pad + j] = C[oc + r + (size_t)j * m];
        if (Dm) for (int j = 0; j < nu; j++) for (int r = 0; r < m; r++) Gk[(size_t)r * nz + s->nx[k] + j] = Dm[od + r + (size_t)j * m];
        oc += (size_t)m * nxc; od += (size_t)m * nu;
    }
    HIP_TRY(hipMemcpy(g.d_Gt, Gt.data(), sizeof(double) * (size_t)g.goff[(size_t)Nn], hipMemcpyHostToDevice));
    s->sk.need_dense_init = true;          /* the kept P_k were built with other rows */
    return TQGPU_OK;
}
/* the ranges checked by rows_check, where the call gave any (given: new rows, dmin or dmax); the host copy always */
int rows_upload_ranges(tqgpu_solver *s, std::vector<double> &dr, int total, bool given) {
    if (total > 0 && given) HIP_TRY(hipMemcpy(s->rows.d_drange, dr.data(), sizeof(double) * 2 * (size_t)total, hipMemcpyHostToDevice));
    s->rows.h_drange.swap(dr); return TQGPU_OK;
}
}  // namespace

/* General constraints dmin <= C x + D u <= dmax of the nodes (the qpOASES QProblem of the reference, dual_Newton_tree_qpoases.c:226-300):
 * nc rows per node, C (nc x nx) and D (nc x nu) column major, node after node.  nc != NULL (re)defines the rows: what is not given with it
 * is zero (C, D) and unbounded (dmin, dmax).  They apply on the nodes of kind 3 (tqgpu_set_objective_mixed, before or after this call). */
extern "C" int tqgpu_set_constraints(tqgpu_solver *s, const int *nc, const double *C, const double *Dm, const double *dmin, const double *dmax) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (s->shard.on || s->pshard.on) return fail(TQGPU_EINVAL, "general constraints are not available in sharded mode");
    if (!nc && s->rows.nc.empty()) return fail(TQGPU_EINVAL, "tqgpu_set_constraints: the rows per node (nc) have not been given yet");
    HIP_TRY(hipSetDevice(s->device));
    int total = 0, rc;
    std::vector<double> dr;
    if ((rc = rows_check(s, nc, dmin, dmax, total, dr))) return rc;          /* before anything changes */
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (nc && (rc = rows_define(s, nc, total))) return rc;
    if ((C || Dm) && (rc = rows_upload_G(s, C, Dm))) return rc;
    if ((rc = rows_upload_ranges(s, dr, total, nc || dmin || dmax))) return rc;
    s->out.invalidate(); s->sens.invalidate(); s->sens.dirty = true;          /* not problem_changed: the rows are no input of tqgpu_set_problem (in_valid stays), the exported point goes */
    return TQGPU_OK;
}

extern "C" int tqgpu_dims2(const tqgpu_solver *s, int *sum_nc) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (sum_nc) *sum_nc = s->rows.sum_nc;
    return TQGPU_OK;
}

/* the row multipliers of the last solve (sum_nc doubles, node after node): those of the final working sets of the kind-3 nodes, 0 elsewhere */
extern "C" int tqgpu_get_mu_d(tqgpu_solver *s, double *mu_d) {
    SETTLE(s);
    if (!s || !mu_d) return fail(TQGPU_EINVAL, "tqgpu_get_mu_d: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->rows.sum_nc > 0) HIP_TRY(hipMemcpy(mu_d, s->rows.d_mu, sizeof(double) * (size_t)s->rows.sum_nc, hipMemcpyDeviceToHost));
    if (!s->sk.gen) std::fill(mu_d, mu_d + s->rows.sum_nc, 0.0);
    return TQGPU_OK;
}

/* stage_gen's hot start on / off (default on).  Off: every stage solve of a kind-3 node starts at the minimiser over the equalities.  Either
 * way the call empties the stored working sets of the kind-3 nodes (the box nodes keep theirs). */
extern "C" int tqgpu_set_gen_hot_start(tqgpu_solver *s, int on) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    s->rows.hot = on != 0;
    if (!s->rows.d_gen) return TQGPU_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t Nn = (size_t)s->Nn;
    s->rows.h_gen.hot = s->rows.hot ? 1 : 0;
    /* everything on the mirror's own stream, so that it is ordered before the next solve's launches by construction */
    std::vector<unsigned long long> bm(Nn);
    HIP_TRY(hipMemcpyAsync(bm.data(), s->D.bmask, sizeof(unsigned long long) * Nn, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t k = 0; k < Nn && k < s->sk.h_kind.size(); k++) if (s->sk.h_kind[k] == 3) bm[k] = 0ull;
    HIP_TRY(hipMemcpyAsync(s->D.bmask, bm.data(), sizeof(unsigned long long) * Nn, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->rows.d_gen, &s->rows.h_gen, sizeof(Gen), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(s->rows.h_gen.rmask, 0, sizeof(unsigned long long) * Nn, s->stream));
    HIP_TRY(hipMemsetAsync(s->rows.h_gen.sides, 0, sizeof(unsigned long long) * 2 * Nn, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}

/* active-set steps of stage_gen per node (Nn entries each, either may be NULL): in the last stage sweep, and summed over the last tqgpu_solve.
 * One step is one factorisation of S: the dual-feasibility rounds of a hot start and a cold redo count.  0 on nodes of other kinds. */
extern "C" int tqgpu_get_stage_steps(tqgpu_solver *s, int *last, long *total) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    const size_t Nn = (size_t)s->Nn;
    if (!s->sk.gen || !s->rows.d_steps) {
        if (last) std::fill(last, last + Nn, 0);
        if (total) std::fill(total, total + Nn, 0L);
        return TQGPU_OK;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (total) HIP_TRY(hipMemcpy(total, s->rows.d_steps, sizeof(long) * Nn, hipMemcpyDeviceToHost));
    if (last) HIP_TRY(hipMemcpy(last, s->rows.d_steps + Nn, sizeof(int) * Nn, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

extern "C" int tqgpu_set_lambda(tqgpu_solver *s, const double *lambda) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    /* kept in a resident buffer: every tqgpu_solve starts from it (device-to-device copy) */
    s->lam_valid = false;
    s->warm.fresh = true;            /* warm start mode 1: the next solve starts from this buffer */
    s->shift.restore = 0;            /* (a buffer saved by tqgpu_mpc_shift is superseded) */
    if (lambda) { H2D(s->d_lam_init + s->nx0, lambda, s->sum_lam); }
    else HIP_TRY(hipMemsetAsync(s->d_lam_init, 0, sizeof(double) * (size_t)s->sum_nx, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}
/* The whole clipping QP (and the starting duals) in one call, for callers that hand over all their data before every
 * solve (treeqp_tdunes_solve re-reads qp_in each time, dual_Newton_tree.c:1142-1160): every array is compared with
 * the pinned host mirror of what the device holds and only what changed is copied and uploaded -- asynchronously,
 * from pinned memory, with no synchronisation (the solve is stream-ordered behind it).  An MPC loop that only
 * moves x0 re-uploads b (and r) and nothing else.  NULL arrays are left alone. */
extern "C" int tqgpu_set_problem(tqgpu_solver *s, const double *A, const double *B, const double *b,
                                 const double *Qd, const double *Rd, const double *q, const double *r,
                                 const double *xmin, const double *xmax, const double *umin, const double *umax, const double *lambda) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    HIP_TRY(hipSetDevice(s->device));
    if (back_to_clipping(s)) { problem_changed(s, true); s->need_init = true; }
    if (xmin || xmax || umin || umax) s->sk.h_bounds.clear();           /* (the checks of the box nodes' bounds see them through tqgpu_set_bounds only) */
    char *slab = static_cast<char *>(s->slab);
    bool any_pack = false, any_init = false;
    auto put = [&](double *dev, const double *src, int count, bool pack, bool init) -> int {
        if (!src || count <= 0) return TQGPU_OK;
        char *mir = s->h_in + ((reinterpret_cast<char *>(dev) - slab) - (ptrdiff_t)s->in_off0);
        const size_t bytes = sizeof(double) * (size_t)count;
        if (s->in_valid && memcmp(mir, src, bytes) == 0) return TQGPU_OK;
        memcpy(mir, src, bytes);
        HIP_TRY(hipMemcpyAsync(dev, mir, bytes, hipMemcpyHostToDevice, s->stream));
        s->links.stream_pending = true;
        s->sens.invalidate(); s->sens.dirty = true;          /* not problem_changed: the pinned mirror has just been brought up to date, in_valid stays */
        any_pack |= pack; any_init |= init;
        return TQGPU_OK;
    };
    int rc;
    const int nxe = s->sum_nx - s->x_pad;
    if ((rc = put(s->A + s->A_pad, A, s->sum_A - s->A_pad, true, false)) || (rc = put(s->B, B, s->sum_B, true, false)) ||
        (rc = put(s->b + s->nx0, b, s->sum_lam, false, false)) ||
        (rc = put(s->Qd + s->x_pad, Qd, nxe, true, true)) || (rc = put(s->Rd, Rd, s->sum_nu, true, true)) ||
        (rc = put(s->q + s->x_pad, q, nxe, true, false)) || (rc = put(s->r, r, s->sum_nu, true, false)) ||
        (rc = put(s->xmin + s->x_pad, xmin, nxe, true, false)) || (rc = put(s->xmax + s->x_pad, xmax, nxe, true, false)) ||
        (rc = put(s->umin, umin, s->sum_nu, true, false)) || (rc = put(s->umax, umax, s->sum_nu, true, false)))
        return rc;
    s->in_valid = A && B && b && Qd && Rd && q && r && xmin && xmax && umin && umax ? true : s->in_valid;
    if (any_init) s->need_init = true;
    if (any_pack) s->persist.need_pack = true;
    if (lambda && s->sum_lam > 0) {
        const size_t bytes = sizeof(double) * (size_t)s->sum_lam;
        s->warm.fresh = true;        /* as tqgpu_set_lambda (a warm-start copy since the last upload has cleared lam_valid) */
        s->shift.restore = 0;
        if (!s->lam_valid || memcmp(s->h_lam, lambda, bytes) != 0) {
            memcpy(s->h_lam, lambda, bytes);
            HIP_TRY(hipMemcpyAsync(s->d_lam_init + s->nx0, s->h_lam, bytes, hipMemcpyHostToDevice, s->stream));
            s->links.stream_pending = true;
            s->lam_valid = true;
        }
    }
    return TQGPU_OK;
}
#undef H2D

/* opt-in: a dense tree (kinds 1 / 2 / 3) that fits runs its whole solve as one launch of one workgroup (g_persist_dense).  The stored working
 * sets are shared between the routes: switching between two solves needs no reset. */
extern "C" int tqgpu_set_dense_single_launch(tqgpu_solver *s, int on) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    s->gpd.single = on != 0;
    return TQGPU_OK;
}
extern "C" int tqgpu_get_dense_single_launch(const tqgpu_solver *s, int *on, int *eligible, int *stage_waves) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    const bool ok = s->sk.dense && s->gpd.ok;
    if (on) *on = s->gpd.single ? 1 : 0;
    if (eligible) *eligible = ok ? 1 : 0;
    if (stage_waves) *stage_waves = ok ? s->gpd.stage_waves : 0;
    return TQGPU_OK;
}

/* opt-in: dense trees that fit go out of tqgpu_solve_batch together, as ONE launch with a workgroup per tree (g_persist_dense_batch), where
 * each would otherwise run the launch-per-phase route on its own, one after the other.  Says nothing about the mirror solved alone, and
 * tqgpu_set_dense_single_launch says nothing about batches.  The stored working sets are shared between the routes, as there. */
extern "C" int tqgpu_set_dense_batch_launch(tqgpu_solver *s, int on) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    s->gpd.batch = on != 0;
    return TQGPU_OK;
}
extern "C" int tqgpu_get_dense_batch_launch(const tqgpu_solver *s, int *on, int *eligible) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (on) *on = s->gpd.batch ? 1 : 0;
    if (eligible) *eligible = s->sk.dense && s->gpd.ok ? 1 : 0;
    return TQGPU_OK;
}

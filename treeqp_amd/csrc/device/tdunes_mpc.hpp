/*
 * tdunes_mpc.hpp -- the MPC family of the host part: kernels (k_mpc_pre, k_mpc_post, their batch forms), the plan and launcher of k_mpc_pre,
 * the entry points tqgpu_mpc_* of the step, its batch, the root forms, tracking, warm start and shift.  Included once from tdunes_device.hip inside
 * #if TQ_HAS(TQP_HOST), behind the batch solve.  That file keeps what the solve path uses: the mirror's records MpcRoot .. MpcTrack (in tdunes_mirror.hpp), MpcStats / MPC_COUNT,
 * MpcPre, mpc_warm_due, problem_changed, and the declarations mpc_before_wave / mpc_behind_launches / mpc_after_wave, the seam to the batch step.
 * The derivatives of a step (sensitivities, adjoints) are tdunes_adjoint.hpp's, included behind this file.
 */
#pragma once

namespace {

/* ---- MPC steps (tqgpu_mpc_*): the x0 fold and the warm-start copy ahead of a solve, the post of u[0] behind it ----
 * One descriptor per mirror: a kernel argument for a mirror on its own, an array (blockIdx.y = member) for a batch, as KItem.
 * k_mpc_pre, waves of 64 lanes, blockIdx.x:
 *   [0, nk0)     the fold of root child blockIdx.x: rows over lanes, b = b0, then fma over the columns j of A0 ascending;
 *   nk0          r[0] = r0 + S0 x0 and the rows dmin[0] = dmin0 - C0 x0, dmax[0] = dmax0 - C0 x0, entries over lanes, same order;
 *                a root that keeps its states (xlo != nullptr) instead: xmin[0] = xmax[0] = x0, copied bit for bit, states over lanes, and
 *                entries 3, 4 (lower, upper) of the root's packed constants, k_pack_persist's layout cst[(0 * 16 + t) * 5 + ..]; blocks [0, nk0) idle;
 *   nk0 + 1 ..   the warm start: MPC_WARM_SPAN doubles of the current duals each (Ctrl::cur says which buffer: read here, so nothing waits for the host)
 *                into the start buffer, node-indexed as they lie (phantom root states included).  A shifted warm start (warm start mode 2,
 *                tqgpu_mpc_shift) gathers instead: entry i of the start buffer is entry shift_src[i] of the current duals, or 0.0 where
 *                shift_src[i] < 0 (the entry-level source table of the current realisation, tqgpu_mpc_set_shift): a copy with an index
 *                load per entry.  Block nk0 then also moves the stored working sets of kinds 2 and 3 a stage (mpc_shift_sets).
 *   behind them, one block per node (mirrors with a reference trajectory, tqgpu_mpc_set_tracking, in a launch that moves the window):
 *                the linear terms of node k for trajectory row min(t0 + stage[k], T - 1), rows of [x | u] over lanes, every entry one chain
 *                of fused multiply-adds from its base, columns ascending (mpc_track_node); where the packed constants of the persistent
 *                route are current, entry 0 of the node's slots as well.  r[0] of an x0-eliminated root with S0 belongs to block nk0,
 *                which then computes base - R_0 uref - S0 xref + S0 x0 as one chain (mpc_track_root_r) instead of r0 + S0 x0.
 * The fold writes b, r, dmin, dmax (or xmin, xmax of the root and their packed copies); the copy reads lam0 / lam1 and writes lam_init; the
 * window fold writes q, r (and their packed copies): the roles touch disjoint data.  No atomics. */
struct MItem {
    Tree T; Data D;
    const double *A0, *b0, *S0, *r0, *C0, *dmin0, *dmax0;      /* the originals in device memory (S0, C0: nullptr = zero, the target is left alone) */
    const double *x0;                  /* pinned, read over the bus */
    double *b, *r, *dmin, *dmax;       /* the targets: Data::b, Data::r, Gen::dmin, Gen::dmax */
    double *xlo, *xhi;                 /* a root that keeps its states (tqgpu_mpc_set_root_states): Data::xmin, Data::xmax of the root, the fold's only targets */
    double *cst;                       /* ... and the root's packed constants of the persistent route where they are current (else nullptr: the coming re-pack reads Data) */
    double *lam_init;                  /* the start buffer */
    double *u0;                        /* pinned: where k_mpc_post puts u[0] */
    int nx0, nc0, nu0, sum_nx;
    int fold, warm;                    /* what k_mpc_pre does for this mirror */
    /* the shift (tqgpu_mpc_set_shift; shift_src == nullptr: the plain copy): the source entry of every entry of the start buffer for the
     * realisation in force (-1: 0.0), and the node table of that realisation, [Nn] the image a node may take its working sets from (-1: it
     * keeps its own), where the sets move too (else nullptr); lam_keep: where tqgpu_mpc_shift saves the start buffer of a mirror in mode 0 */
    const int *shift_src, *shift_node;
    double *lam_keep;
    unsigned long long *ws_rmask, *ws_sides;      /* Gen::rmask, Gen::sides where the tree has rows (else nullptr), with ws_nc = Gen::nc */
    const int *ws_nc;
    int realised;
    /* tracking (xtraj == nullptr: none): the trajectory, the base linear terms and the nodes' stages in device memory; the targets Data::q,
     * Data::r (r above) and entry 0 of the packed constants where they are current (else nullptr); t0: the window now in force (-1: none yet) */
    const double *xtraj, *utraj, *q0, *rb0;
    const int *stage;
    double *q, *pcq;
    int trk, t0, Tn, nxt, nut, xpad;   /* trk: this launch folds the window t0 */
};
constexpr int MPC_WARM_SPAN = 512;
/* the trajectory row of node k for the window in force */
__device__ __forceinline__ int mpc_track_row(const MItem &it, int k) {
    const int row = it.t0 + it.stage[k];
    return row < it.Tn - 1 ? row : it.Tn - 1;
}
/* does block nk0 own r[0]?  (an x0-eliminated root with S0 on a tracking mirror whose window has been set) */
__device__ __forceinline__ bool mpc_track_owns_r0(const MItem &it) { return it.xtraj && it.S0 && it.t0 >= 0; }
/* q, r of node k: kind 0 v = fma(-Qd[i], xref[i], q0[i]) (r: Rd, uref); kinds 1 / 2 / 3, row i of H_k: v = base[i], then
 * v = fma(-H[i, j], xref[j], v) over the x columns, then v = fma(-H[i, nx + j], uref[j], v) over the u columns.  Phantom root states keep
 * their q (and are no columns); a leaf has no u part. */
__device__ __forceinline__ void mpc_track_node(const MItem &it, int k, int lane) {
    const Tree &T = it.T;
    if (!it.trk || !it.xtraj || k >= T.Nn) return;
    const int pad = k == 0 ? it.xpad : 0, nx = T.nx[k], nu = T.nu[k], nxe = nx - pad, nz = nx + nu;
    const int xo = T.xoff[k], uo = T.uoff[k], row = mpc_track_row(it, k);
    const double *xr = it.xtraj + (size_t)row * it.nxt, *ur = it.utraj + (size_t)row * it.nut;
    const int kind = it.D.dense ? it.D.kind[k] : 0;
    const bool r_elsewhere = k == 0 && mpc_track_owns_r0(it);
    for (int i = pad + lane; i < nz; i += WAVE) {
        const bool isx = i < nx;
        if (!isx && r_elsewhere) continue;
        double v = isx ? it.q0[xo + i] : it.rb0[uo + i - nx];
        if (kind == 0) v = isx ? fma(-it.D.Qd[xo + i], xr[i - pad], v) : fma(-it.D.Rd[uo + i - nx], ur[i - nx], v);
        else {
            const double *H = it.D.Hd + it.D.poff[k];
            for (int j = 0; j < nxe; j++) v = fma(-H[i + (size_t)(pad + j) * nz], xr[j], v);
            for (int j = 0; j < nu; j++) v = fma(-H[i + (size_t)(nx + j) * nz], ur[j], v);
        }
        if (isx) it.q[xo + i] = v; else it.r[uo + i - nx] = v;
        if (it.pcq && i < 16) it.pcq[((size_t)k * 16 + i) * 5] = v;          /* k_pack_persist's layout: slot t = i of node k, entry 0 */
    }
}
/* r[0] of an x0-eliminated root with S0, one chain: base, - R_0 uref, - S0 xref, + S0 x0 */
__device__ __forceinline__ void mpc_track_root_r(const MItem &it, int lane) {
    const Tree &T = it.T;
    const int nx = T.nx[0], nu0 = it.nu0, nz = nx + nu0, nx0 = it.nx0, row = mpc_track_row(it, 0);          /* nx: phantom states only */
    const double *xr = it.xtraj + (size_t)row * it.nxt, *ur = it.utraj + (size_t)row * it.nut;
    const double *H = it.D.Hd + it.D.poff[0];          /* (S0 is refused on a root of kind 0) */
    for (int i = lane; i < nu0; i += WAVE) {
        double v = it.rb0[i];
        for (int j = 0; j < nu0; j++) v = fma(-H[nx + i + (size_t)(nx + j) * nz], ur[j], v);
        for (int j = 0; j < nx0; j++) v = fma(-it.S0[i + (size_t)j * nu0], xr[j], v);
        for (int j = 0; j < nx0; j++) v = fma(it.S0[i + (size_t)j * nu0], it.x0[j], v);
        it.r[i] = v;
    }
}
/* The stored working sets move a stage, in place: node k takes the bound set (and its sides) of m = shift_node[k] where both are of kind
 * 2 or 3 and nu agrees (nx does, by the map), the row set (and its sides) where both are of kind 3 and nc agrees; every other node keeps
 * its own; the halves [Nn, 2 Nn) that say what P_k was built for are not touched.  m > k for every node that takes a set (images are one
 * level deeper and nodes are numbered level by level), so ONE wave that walks the nodes in ascending chunks of 64, with all loads of a
 * chunk complete ahead of its stores, reads only words no earlier store has replaced: no scratch copy, no atomics, no dependence on the
 * order of blocks (no other block touches these words).
 * Tested on trees of more than one chunk: tests/shift_set_cases.py holds them (chains of 64 .. 129 nodes, binary trees of 127 .. 255, a tree
 * that meets every refusal rule on both sides of lane 63, a tree without rows), the injected words that tell a node from its image, and
 * numpy walks of this loop, ascending / descending, loads first / lane by lane; tests/test_shift_set_reference.py shows without a device on
 * which of these trees each clause above can be seen to fail, tests/test_gpu_mpc_shift_sets.py holds the kernel to the out-of-place gather bit
 * for bit, alone, twice ahead of one solve, with the duals' blocks, in a batch, and after the kinds or nc have changed. */
__device__ __forceinline__ void mpc_shift_sets(const MItem &it, int lane) {
    const int Nn = it.T.Nn;
    const int *kind = it.D.kind;
    unsigned long long *bm = it.D.bmask, *rm = it.ws_rmask, *sd = it.ws_sides;
    for (int base = 0; base < Nn; base += WAVE) {
        const int k = base + lane;
        const int m = k < Nn ? it.shift_node[k] : -1;
        bool tb = false, tr = false;
        unsigned long long vb = 0ull, vsb = 0ull, vr = 0ull, vsr = 0ull;
        if (m > k && m < Nn) {
            const int kk = kind[k], km = kind[m];
            tb = kk >= 2 && km >= 2 && it.T.nu[k] == it.T.nu[m];
            tr = tb && rm && kk == 3 && km == 3 && it.ws_nc[k] == it.ws_nc[m];
            if (tb) { vb = bm[m]; if (sd) vsb = sd[m]; }
            if (tr) { vr = rm[m]; vsr = sd[Nn + m]; }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          /* every load of the chunk has returned ... */
        __builtin_amdgcn_wave_barrier();                          /* ... before any of its stores is issued */
        if (tb) { bm[k] = vb; if (sd) sd[k] = vsb; }
        if (tr) { rm[k] = vr; sd[Nn + k] = vsr; }
    }
}
__device__ __forceinline__ void mpc_pre_block(const MItem &it, int blk, int lane) {
    const Tree &T = it.T;
    const int nk0 = T.nk[0], nx0 = it.nx0;
    const int track0 = nk0 + 1 + (it.sum_nx + MPC_WARM_SPAN - 1) / MPC_WARM_SPAN;          /* (the host's copy of this layout: mpc_pre_grid) */
    if (blk >= track0) { mpc_track_node(it, blk - track0, lane); return; }
    if (blk < nk0) {
        if (!it.fold || it.xlo) return;
        const int first = T.kid0[0], kid = first + blk, nxk = T.nx[kid];
        int ao = 0, bo = 0;
        for (int c = 0; c < blk; c++) { const int n = T.nx[first + c]; ao += n * nx0; bo += n; }
        const double *A = it.A0 + ao, *b0 = it.b0 + bo;
        double *b = it.b + T.xoff[kid];
        for (int i = lane; i < nxk; i += WAVE) {
            double v = b0[i];
            for (int j = 0; j < nx0; j++) v = fma(A[i + (size_t)j * nxk], it.x0[j], v);
            b[i] = v;
        }
        return;
    }
    if (blk == nk0) {
        if (it.warm && it.shift_node) mpc_shift_sets(it, lane);
        const bool owns_r0 = mpc_track_owns_r0(it);
        if (owns_r0 && (it.fold || it.trk)) mpc_track_root_r(it, lane);
        if (!it.fold) return;
        if (it.xlo) {
            for (int i = lane; i < nx0; i += WAVE) {
                const double v = it.x0[i];
                it.xlo[i] = v; it.xhi[i] = v;
                if (it.cst && i < 16) { it.cst[(size_t)i * 5 + 3] = v; it.cst[(size_t)i * 5 + 4] = v; }
            }
            return;
        }
        const int nu0 = it.nu0, nc0 = it.nc0;
        if (it.S0 && !owns_r0) for (int i = lane; i < nu0; i += WAVE) {
            double v = it.r0[i];
            for (int j = 0; j < nx0; j++) v = fma(it.S0[i + (size_t)j * nu0], it.x0[j], v);
            it.r[i] = v;
        }
        if (it.C0) for (int i = lane; i < nc0; i += WAVE) {
            double lo = it.dmin0[i], hi = it.dmax0[i];
            for (int j = 0; j < nx0; j++) { const double c = -it.C0[i + (size_t)j * nc0]; lo = fma(c, it.x0[j], lo); hi = fma(c, it.x0[j], hi); }
            it.dmin[i] = lo; it.dmax[i] = hi;
        }
        return;
    }
    if (!it.warm) return;
    const double *src = it.D.ctrl->cur ? it.D.lam1 : it.D.lam0;
    const int base = (blk - nk0 - 1) * MPC_WARM_SPAN;
    if (!it.shift_src) {
        for (int t = 0; t < MPC_WARM_SPAN / WAVE; t++) {
            const int i = base + t * WAVE + lane;
            if (i < it.sum_nx) it.lam_init[i] = src[i];
        }
        return;
    }
    /* the shifted start: the indices of the span first, then the gathered duals (independent loads), then the stores; a thread saves the entry
     * it is about to replace where the caller's start buffer has to come back (lam_keep) */
    int from[MPC_WARM_SPAN / WAVE];
    double v[MPC_WARM_SPAN / WAVE];
#pragma unroll
    for (int t = 0; t < MPC_WARM_SPAN / WAVE; t++) {
        const int i = base + t * WAVE + lane;
        from[t] = i < it.sum_nx ? it.shift_src[i] : -1;
    }
#pragma unroll
    for (int t = 0; t < MPC_WARM_SPAN / WAVE; t++) v[t] = from[t] >= 0 && from[t] < it.sum_nx ? src[from[t]] : 0.0;
#pragma unroll
    for (int t = 0; t < MPC_WARM_SPAN / WAVE; t++) {
        const int i = base + t * WAVE + lane;
        if (i >= it.sum_nx) continue;
        if (it.lam_keep) it.lam_keep[i] = it.lam_init[i];
        it.lam_init[i] = v[t];
    }
}
__global__ void __launch_bounds__(WAVE) k_mpc_pre(MItem it) { mpc_pre_block(it, blockIdx.x, threadIdx.x); }
__global__ void __launch_bounds__(WAVE) k_mpc_pre_batch(const MItem *__restrict__ items) { mpc_pre_block(items[blockIdx.y], blockIdx.x, threadIdx.x); }
/* k_mpc_post, one workgroup, enqueued behind the solve: u[0] of every member into pinned memory (sixteen lanes per member), every store
 * acknowledged, then the tag the host polls -- the way the single launches post their verdict (g_persist_body) */
__device__ __forceinline__ void mpc_post_values(const MItem &it, int l, int stride) {
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(it.u0);
    for (int i = l; i < it.nu0; i += stride) __hip_atomic_store(dst + i, (unsigned long long)__double_as_longlong(it.D.u[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void mpc_post_tag(unsigned long long *tag, unsigned long long want) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(tag, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(256) k_mpc_post(MItem it, unsigned long long *tag, unsigned long long want) {
    mpc_post_values(it, threadIdx.x, 256);
    mpc_post_tag(tag, want);
}
__global__ void __launch_bounds__(256) k_mpc_post_batch(const MItem *__restrict__ items, int n, unsigned long long *tag, unsigned long long want) {
    for (int m = threadIdx.x >> 4; m < n; m += 16) mpc_post_values(items[m], threadIdx.x & 15, 16);
    mpc_post_tag(tag, want);
}

/* ---- the host side: x0 fold, warm start and u[0] without the host in the data path (tqgpu_mpc_*) ---- */

int mpc_refuse(const tqgpu_solver *s, const char *who) {
    if (!s) return fail(TQGPU_EINVAL, std::string(who) + ": null solver");
    if ((s->pshard.on || s->shard.on) && s->shard.nranks > 1)
        return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": this mirror is rank " + std::to_string(s->shard.rank) + " of a sharded solve; MPC steps run on single-device mirrors");
    return TQGPU_OK;
}

/* the tables of k_nodesum_part / k_nodesum_sum (tdunes_sens.hpp) for the node sets `sets` (members ascending), width[g] accumulators per chunk of set g:
 * member lists, set records, the chunks of ADJMAT_CHUNK members cut per set, uploaded in one block; mode 0 also lays the sets' blocks of width / 2
 * doubles one behind the other (NodeSum::tot) */
int nodesum_build(tqgpu_solver *s, MpcNodeSum &m, const std::vector<std::vector<int>> &sets, const std::vector<int> &width, int mode, const char *who) {
    int rc;
    std::vector<int> mem, chk;
    m.set.assign(sets.size() * 4, 0);
    size_t part = 0, tot = 0, wmax = 0;
    for (size_t g = 0; g < sets.size(); g++) {
        const int members = (int)sets[g].size(), W = width[g];
        int *rec = &m.set[4 * g];
        rec[0] = (int)(chk.size() / 4); rec[2] = (int)tot; rec[3] = W;
        for (int at = 0; at < members; at += ADJMAT_CHUNK, rec[1]++) {
            chk.push_back((int)g); chk.push_back((int)mem.size() + at); chk.push_back(std::min(ADJMAT_CHUNK, members - at)); chk.push_back((int)part);
            part += (size_t)W;
        }
        mem.insert(mem.end(), sets[g].begin(), sets[g].end());
        tot += (size_t)W / 2; wmax = std::max(wmax, (size_t)W);
    }
    if (part > (size_t)INT_MAX / 2) return fail(TQGPU_EUNSUPPORTED, std::string(who) + ": the partial sums do not fit the tables' 32-bit offsets");
    std::vector<int> tab;
    auto put = [&](const std::vector<int> &v) { const size_t at = tab.size(); tab.insert(tab.end(), v.begin(), v.end()); return at; };
    const size_t o_mem = put(mem), o_set = put(m.set), o_chk = put(chk);
    tab.push_back(0);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* a sum in flight reads the block that is replaced */
    s->mem.release(m.d_tab);
    m.v = NodeSum{};
    if ((rc = s->mem.upload(m.d_tab, tab.data(), tab.size() * sizeof(int), TQGPU_ENOMEM, "the tables of the node sets"))) return rc;
    m.v.mem = m.d_tab + o_mem; m.v.set = m.d_tab + o_set; m.v.chk = m.d_tab + o_chk;
    m.v.n_set = (int)sets.size(); m.v.n_chk = (int)(chk.size() / 4); m.v.mode = mode; m.v.tot = mode ? 0 : (int)tot;
    m.part1 = part; m.lds = (2 * wmax + 2) * sizeof(double);
    return TQGPU_OK;
}

/* the descriptor of a mirror for k_mpc_pre / k_mpc_post: views into mpc.d and mpc.h (null before tqgpu_mpc_set_root / _set_root_states: fold must be false then) */
MItem mpc_item(const tqgpu_solver *s, MpcPre pre) {
    MItem it{};
    it.T = s->T; it.D = s->D;
    const size_t nx0 = (size_t)s->mpc.nx0, nb = (size_t)s->mpc.nb, nu0 = (size_t)s->nu[0], nc0 = (size_t)s->mpc.nc0;
    if (s->mpc.d) {
        const double *p = s->mpc.d;
        it.A0 = p; p += nb * nx0; it.b0 = p; p += nb;
        it.S0 = s->mpc.S0 ? p : nullptr; p += nu0 * nx0; it.r0 = p; p += nu0;
        it.C0 = s->mpc.C0 ? p : nullptr; p += nc0 * nx0; it.dmin0 = p; p += nc0; it.dmax0 = p;
    }
    if (s->mpc.h) { it.x0 = s->mpc.h; it.u0 = s->mpc.h + nx0; }
    if (s->mpc.states) {
        /* the packed constants hold a copy of the bounds (k_pack_persist); no other route keeps one: they read Data::xmin / xmax at every launch */
        it.xlo = s->xmin; it.xhi = s->xmax;
        it.cst = s->persist.ok && s->persist.pcst && !s->persist.need_pack ? s->persist.pcst : nullptr;
    }
    it.b = s->b; it.r = s->r;
    it.dmin = s->mpc.C0 ? s->rows.d_drange : nullptr; it.dmax = s->mpc.C0 ? s->rows.d_drange + s->rows.sum_nc : nullptr;
    it.lam_init = s->d_lam_init;
    it.nx0 = s->mpc.nx0; it.nc0 = s->mpc.nc0; it.nu0 = s->nu[0]; it.sum_nx = s->sum_nx;
    it.fold = pre.fold ? 1 : 0; it.warm = pre.warm ? 1 : 0;
    /* the warm start of mode 2, and tqgpu_mpc_shift in any mode (shift), go through the tables of the realisation in force; the node
     * table only where the sets were asked for and the tree has nodes of kinds 2 / 3 now (Data::kind is read there) */
    if (pre.warm && s->shift.d && (pre.shift || s->warm.mode == 2)) {
        const size_t nreal = (size_t)std::max(s->nk[0], 1), j = (size_t)s->shift.realised;
        it.shift_src = s->shift.d + j * (size_t)s->sum_nx;
        if ((s->shift.what & TQGPU_SHIFT_WORKING_SETS) && s->sk.working_sets((size_t)s->Nn) && s->D.kind && s->D.bmask)
            it.shift_node = s->shift.d + nreal * (size_t)s->sum_nx + j * (size_t)s->Nn;
        if (s->sk.gen && s->rows.d_rmask && s->rows.h_gen.nc) { it.ws_rmask = s->rows.h_gen.rmask; it.ws_sides = s->rows.h_gen.sides; it.ws_nc = s->rows.h_gen.nc; }
        it.realised = s->shift.realised;
        /* tqgpu_mpc_shift: mode 0 promises the caller's start buffer to every solve: the kernel saves it (once: a second shift ahead of the same
         * solve finds the shifted duals there), and the solve after the next puts it back (solve_begin) */
        if (pre.shift && s->warm.mode == 0 && s->shift.restore == 0) it.lam_keep = s->shift.d_keep;
    }
    if (s->trk.d) {
        const double *p = s->trk.d;
        it.xtraj = p; p += (size_t)s->trk.T * s->trk.nxt; it.utraj = p; p += (size_t)s->trk.T * s->trk.nut;
        it.q0 = p; p += s->sum_nx; it.rb0 = p; p += s->sum_nu;
        it.stage = reinterpret_cast<const int *>(p);
        it.q = s->q;
        /* the packed constants hold a copy of q, r (k_pack_persist); every other route reads Data::q / r in place at every launch */
        it.pcq = s->persist.ok && s->persist.pcst && !s->persist.need_pack ? s->persist.pcst : nullptr;
        it.trk = pre.track ? 1 : 0; it.t0 = s->trk.t0; it.Tn = s->trk.T; it.nxt = s->trk.nxt; it.nut = s->trk.nut; it.xpad = s->x_pad;
    }
    return it;
}
/* THE host side of the block layout of k_mpc_pre (mpc_pre_block reads it as blk < nk0, == nk0, < track0, >= track0): the blocks of a launch,
 * up to the fold, the warm-start copy, or the nodes of the window fold */
unsigned mpc_pre_grid(const tqgpu_solver *s, MpcPre p) {
    const unsigned fold_end = (unsigned)(s->nk[0] + 1), track0 = fold_end + (unsigned)((s->sum_nx + MPC_WARM_SPAN - 1) / MPC_WARM_SPAN);
    return p.track ? track0 + (unsigned)s->Nn : p.warm ? track0 : fold_end;
}
/* one launch of k_mpc_pre on the mirror's own stream, nothing waited for.  Counted into the step's record, or, from inside a solve
 * (solve_launches: solve_begin's warm-start copy), with that solve's launches, which a step adds to its record from the result */
int launch_mpc_pre(tqgpu_solver *s, MpcPre p, int *solve_launches = nullptr) {
    hipLaunchKernelGGL(k_mpc_pre, dim3(mpc_pre_grid(s, p)), dim3(WAVE), 0, s->stream, mpc_item(s, p));
    HIP_TRY(hipGetLastError());
    if (solve_launches) ++*solve_launches; else MPC_COUNT(launches, 1);
    if (p.warm) s->lam_valid = false;          /* the pinned mirror of tqgpu_set_problem's duals no longer describes the start buffer */
    s->links.stream_pending = true;
    return TQGPU_OK;
}

/* a new window for a mirror with a reference trajectory, and what its fold makes stale on the host side; nothing is enqueued.  t0 < 0: the
 * window in force stays (no refusal: a mirror without tracking takes such a step as before) */
int mpc_take_window(tqgpu_solver *s, int t0, bool commit, const char *who) {
    if (t0 < 0) return TQGPU_OK;
    if (!s->trk.d) return fail(TQGPU_EINVAL, std::string(who) + ": the reference trajectory has not been given yet (tqgpu_mpc_set_tracking)");
    if (s->mpc.S0 && s->mpc.nx0 != s->trk.nxt)
        return fail(TQGPU_EINVAL, std::string(who) + ": S0 of tqgpu_mpc_set_root has " + std::to_string(s->mpc.nx0) + " columns, the trajectory " + std::to_string(s->trk.nxt) + " states");
    if (s->mpc.S0 && s->sk.kind(0) == 0) return fail(TQGPU_EINVAL, std::string(who) + ": the root became a node of kind 0 after tqgpu_mpc_set_root gave it an S0");
    if (!commit) return TQGPU_OK;
    s->trk.t0 = t0;
    problem_changed(s, false);              /* the pinned mirror of tqgpu_set_problem no longer describes q, r */
    return TQGPU_OK;                        /* persist.need_pack stays as it is: the fold writes the packed copy itself, a pending pack reads Data */
}

/* a new x0 into the mirror's pinned buffer, and what the fold makes stale on the host side; nothing is enqueued */
int mpc_take_x0(tqgpu_solver *s, const double *x0, const char *who) {
    if (!s->mpc.d && !s->mpc.states) return fail(TQGPU_EINVAL, std::string(who) + ": the root terms have not been given yet (tqgpu_mpc_set_root, or tqgpu_mpc_set_root_states on a root that keeps its states)");
    if (s->mpc.states) {
        if (s->sk.kind(0) == 1) return fail(TQGPU_EINVAL, std::string(who) + ": the root became a node of kind 1 after tqgpu_mpc_set_root_states: its bounds are ignored, x0 cannot be imposed");
        if (!x0) return TQGPU_OK;
        const size_t n0 = (size_t)s->mpc.nx0;
        memcpy(s->mpc.h, x0, sizeof(double) * n0);
        problem_changed(s, false);              /* the pinned mirror of tqgpu_set_problem no longer describes xmin, xmax */
        if (!s->sk.h_bounds.empty()) {             /* what the box nodes' checks see (tqgpu_set_bounds) */
            std::copy(x0, x0 + n0, s->sk.h_bounds.begin());
            std::copy(x0, x0 + n0, s->sk.h_bounds.begin() + s->sum_nx);
        }
        return TQGPU_OK;                        /* persist.need_pack stays as it is: the fold writes the packed copy itself */
    }
    if (s->mpc.C0 && (s->rows.nc.empty() || s->rows.nc[0] != s->mpc.nc0 || !s->rows.d_drange))
        return fail(TQGPU_EINVAL, std::string(who) + ": the rows of the root were redefined after tqgpu_mpc_set_root (call it again)");
    /* a tracking mirror whose window is set: r[0] of a root with S0 is the chain of mpc_track_root_r, which reads nx0 entries of a trajectory row */
    if (s->trk.d && s->trk.t0 >= 0 && s->mpc.S0 && s->mpc.nx0 != s->trk.nxt)
        return fail(TQGPU_EINVAL, std::string(who) + ": S0 of tqgpu_mpc_set_root has " + std::to_string(s->mpc.nx0) + " columns, the trajectory of tqgpu_mpc_set_tracking " + std::to_string(s->trk.nxt) + " states");
    if (!x0) return TQGPU_OK;
    memcpy(s->mpc.h, x0, sizeof(double) * (size_t)s->mpc.nx0);
    problem_changed(s, s->mpc.S0);          /* the pinned mirror of tqgpu_set_problem no longer describes b (and r); the persistent route packs r with the bounds (k_pack_persist); b and the rows of kind 3 are read in place */
    return TQGPU_OK;
}

/* the tag of a u0 post: complete at the first look, or waited for -- 2 s of polling, then the stream */
int mpc_wait_tag(const double *block_end, unsigned long long want, hipStream_t st) {
    const volatile unsigned long long *tag = reinterpret_cast<const volatile unsigned long long *>(block_end);
    if (*tag != want) {
        MPC_COUNT(waits, 1);
        const auto t0 = std::chrono::steady_clock::now();
        for (long spins = 0; *tag != want; spins++) {
            __builtin_ia32_pause();
            if ((spins & 0xFFFF) == 0xFFFF && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
        }
        if (*tag != want) {
            HIP_TRY(hipStreamSynchronize(st));
            if (*tag != want) return fail(TQGPU_ENODEVICE, "the post of u[0] did not arrive");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return TQGPU_OK;
}

struct MpcLive {          /* counts into g_mpc_stats while a step runs */
    MpcLive() { g_mpc_stats = MpcStats(); g_mpc_live = &g_mpc_stats; }
    ~MpcLive() { g_mpc_live = nullptr; }
};

int mpc_post_one(tqgpu_solver *s) {
    unsigned long long *tag = reinterpret_cast<unsigned long long *>(s->mpc.h + s->mpc.nx0 + s->nu[0]);
    hipLaunchKernelGGL(k_mpc_post, dim3(1), dim3(256), 0, s->stream, mpc_item(s, MpcPre{}), tag, ++s->mpc.tag);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1);
    return TQGPU_OK;
}

}  // namespace

extern "C" int tqgpu_mpc_set_root(tqgpu_solver *s, int nx0, const double *A0, const double *b0, const double *S0, const double *r0,
                                  const double *C0, const double *dmin0, const double *dmax0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_root"))) return rc;
    SETTLE(s);
    if (s->nx[0] - s->x_pad > 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: the root still has " + std::to_string(s->nx[0] - s->x_pad) + " states: eliminate x0 first");
    if (nx0 <= 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: nx0 must be positive");
    if (s->nk[0] > 0 && (!A0 || !b0)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: A0 and b0 are required");
    if (S0 && !r0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: S0 comes with r0");
    if (C0 && !(dmin0 && dmax0)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: C0 comes with dmin0 and dmax0");
    const size_t n0 = (size_t)nx0, nu0 = (size_t)s->nu[0];
    const bool kind0 = s->sk.kind(0) == 0;
    if (S0 && kind0) {
        for (size_t i = 0; i < nu0 * n0; i++) if (S0[i] != 0.0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: S0 is not zero on a root of kind 0 (clipping: S must be zero)");
        S0 = nullptr;
    }
    const int nc0 = (!s->rows.nc.empty() && s->sk.kind(0) == 3) ? s->rows.nc[0] : 0;
    if (C0 && nc0 <= 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root: C0 without rows on the root (tqgpu_set_constraints, root of kind 3)");
    size_t nb = 0;
    for (int c = 0; c < s->nk[0]; c++) nb += (size_t)s->nx[(size_t)s->kid0[0] + c];
    const size_t nc = C0 ? (size_t)nc0 : 0;
    std::vector<double> blk(nb * n0 + nb + nu0 * n0 + nu0 + nc * n0 + 2 * nc + 1, 0.0);
    double *p = blk.data();
    if (nb) { memcpy(p, A0, sizeof(double) * nb * n0); p += nb * n0; memcpy(p, b0, sizeof(double) * nb); p += nb; }
    if (S0) { memcpy(p, S0, sizeof(double) * nu0 * n0); memcpy(p + nu0 * n0, r0, sizeof(double) * nu0); }
    p += nu0 * n0 + nu0;
    if (C0) { memcpy(p, C0, sizeof(double) * nc * n0); p += nc * n0; memcpy(p, dmin0, sizeof(double) * nc); p += nc; memcpy(p, dmax0, sizeof(double) * nc); }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* a fold in flight reads the block that is replaced */
    s->mem.release(s->mpc.d); s->mem.release(s->mpc.h); s->sens.invalidate();
    s->mpc.nx0 = 0;
    if ((rc = s->mem.upload(s->mpc.d, blk.data(), sizeof(double) * blk.size(), TQGPU_ENOMEM, "the root terms")) ||
        (rc = s->mem.host(s->mpc.h, sizeof(double) * (n0 + nu0 + 2), "the pinned x0 and u0")))
        return rc;
    memset(s->mpc.h, 0, sizeof(double) * (n0 + nu0 + 2));
    s->mpc.nx0 = nx0; s->mpc.nb = (int)nb; s->mpc.nc0 = (int)nc; s->mpc.S0 = S0 != nullptr; s->mpc.C0 = C0 != nullptr;
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_set_root_states(tqgpu_solver *s) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_root_states"))) return rc;
    SETTLE(s);
    const int n0 = s->nx[0] - s->x_pad;
    if (n0 <= 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root_states: the root has no states (x0 is eliminated: tqgpu_mpc_set_root takes the root terms)");
    if (s->sk.kind(0) == 1) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_root_states: the root is of kind 1, whose bounds are ignored: x0 cannot be imposed through them");
    const size_t nu0 = (size_t)s->nu[0];
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* a fold in flight reads the pinned block that is replaced */
    s->mem.release(s->mpc.d); s->mem.release(s->mpc.h); s->sens.invalidate();
    s->mpc.nx0 = 0; s->mpc.states = false;
    if ((rc = s->mem.host(s->mpc.h, sizeof(double) * ((size_t)n0 + nu0 + 2), "the pinned x0 and u0"))) return rc;
    memset(s->mpc.h, 0, sizeof(double) * ((size_t)n0 + nu0 + 2));
    s->mpc.nx0 = n0; s->mpc.nb = 0; s->mpc.nc0 = 0; s->mpc.S0 = false; s->mpc.C0 = false;
    s->mpc.states = true;
    return TQGPU_OK;
}

extern "C" int tqgpu_get_root_bounds(tqgpu_solver *s, double *xmin0, double *xmax0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_get_root_bounds"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int n0 = s->nx[0] - s->x_pad;
    if (xmin0 && n0 > 0) HIP_TRY(hipMemcpy(xmin0, s->xmin + s->x_pad, sizeof(double) * (size_t)n0, hipMemcpyDeviceToHost));
    if (xmax0 && n0 > 0) HIP_TRY(hipMemcpy(xmax0, s->xmax + s->x_pad, sizeof(double) * (size_t)n0, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_set_certify(tqgpu_solver *s, int on) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_certify"))) return rc;
    s->mpc.certify = on != 0;
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_get_certificate(tqgpu_solver *s, double res[6], int node[6]) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_certificate"))) return rc;
    if (!s->mpc.cert_valid) return fail(TQGPU_EINVAL, "tqgpu_mpc_get_certificate: the last tqgpu_mpc_step of this mirror was not certified (tqgpu_mpc_set_certify), or none has run");
    if (res) memcpy(res, s->mpc.cert, sizeof(double) * KKT_CLASSES);
    if (node) memcpy(node, s->mpc.cert + KKT_CLASSES, sizeof(int) * KKT_CLASSES);
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_set_x0(tqgpu_solver *s, const double *x0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_x0"))) return rc;
    if (!x0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_x0: x0 is required");
    if ((rc = mpc_take_x0(s, nullptr, "tqgpu_mpc_set_x0"))) return rc;          /* (the refusals, before anything is touched) */
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = mpc_take_x0(s, x0, "tqgpu_mpc_set_x0"))) return rc;
    return launch_mpc_pre(s, MpcPre{.fold = true});
}

extern "C" int tqgpu_mpc_set_tracking(tqgpu_solver *s, int NXT, int NUT, int T, const double *xtraj, const double *utraj, const double *q0, const double *r0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_tracking"))) return rc;
    SETTLE(s);
    if (T < 1) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_tracking: T must be at least 1");
    if (NXT < 0 || NUT < 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_tracking: NXT and NUT must not be negative");
    if ((NXT > 0 && !xtraj) || (NUT > 0 && !utraj)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_tracking: xtraj and utraj are required where NXT, NUT are positive");
    for (int k = 0; k < s->Nn; k++) {
        const int nxe = s->nx[k] - (k == 0 ? s->x_pad : 0);
        if ((nxe != 0 && nxe != NXT) || (s->nu[k] != 0 && s->nu[k] != NUT))
            return fail(TQGPU_EINVAL, "tqgpu_mpc_set_tracking: node " + std::to_string(k) + " has nx = " + std::to_string(nxe) + ", nu = " + std::to_string(s->nu[k]) +
                        ": every node must have nx in {0, " + std::to_string(NXT) + "} and nu in {0, " + std::to_string(NUT) + "} (one reference per stage)");
    }
    const size_t nxt = (size_t)NXT, nut = (size_t)NUT, nT = (size_t)T, sx = (size_t)s->sum_nx, su = (size_t)s->sum_nu;
    const size_t doubles = nT * nxt + nT * nut + sx + su, ints = (size_t)s->Nn;
    std::vector<double> blk(doubles + (ints + 1) / 2 + 1, 0.0);
    double *p = blk.data();
    if (nxt) memcpy(p, xtraj, sizeof(double) * nT * nxt);
    p += nT * nxt;
    if (nut) memcpy(p, utraj, sizeof(double) * nT * nut);
    p += nT * nut;
    if (q0 && sx > (size_t)s->x_pad) memcpy(p + s->x_pad, q0, sizeof(double) * (sx - (size_t)s->x_pad));          /* (the phantom root states keep their q: their base is never read) */
    p += sx;
    if (r0 && su) memcpy(p, r0, sizeof(double) * su);
    p += su;
    memcpy(p, s->stage.data(), sizeof(int) * ints);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* a fold in flight reads the block that is replaced */
    s->mem.release(s->trk.d);
    s->trk.T = 0; s->trk.t0 = -1;
    if ((rc = s->mem.upload(s->trk.d, blk.data(), sizeof(double) * blk.size(), TQGPU_ENOMEM, "the reference trajectory"))) return rc;
    s->trk.T = T; s->trk.nxt = NXT; s->trk.nut = NUT;
    /* the nodes of every stage and their chunks, for tqgpu_mpc_adjoint_reference: they depend on the tree alone, not on the window */
    std::vector<std::vector<int>> by_stage;
    for (int k = 0; k < s->Nn; k++) {
        if ((size_t)s->stage[k] >= by_stage.size()) by_stage.resize((size_t)s->stage[k] + 1);
        by_stage[(size_t)s->stage[k]].push_back(k);
    }
    return nodesum_build(s, s->rsum, by_stage, std::vector<int>(by_stage.size(), NXT + NUT), 1, "tqgpu_mpc_set_tracking");
}

extern "C" int tqgpu_mpc_set_window(tqgpu_solver *s, int t0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_window"))) return rc;
    if (t0 < 0) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_window: t0 must not be negative");
    if ((rc = mpc_take_window(s, t0, false, "tqgpu_mpc_set_window"))) return rc;          /* (the refusals, before anything is touched) */
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = mpc_take_window(s, t0, true, "tqgpu_mpc_set_window"))) return rc;
    return launch_mpc_pre(s, MpcPre{.track = true});
}

extern "C" int tqgpu_mpc_get_window(const tqgpu_solver *s, int *t0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_window"))) return rc;
    if (t0) *t0 = s->trk.t0;
    return TQGPU_OK;
}

extern "C" int tqgpu_set_warm_start(tqgpu_solver *s, int mode) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_set_warm_start"))) return rc;
    if (mode != 0 && mode != 1 && mode != 2) return fail(TQGPU_EINVAL, "tqgpu_set_warm_start: mode must be 0, 1 or 2");
    if (mode == 2 && !s->shift.d) return fail(TQGPU_EINVAL, "tqgpu_set_warm_start: mode 2 needs the maps of tqgpu_mpc_set_shift first");
    s->warm.mode = mode;
    return TQGPU_OK;
}
extern "C" int tqgpu_get_warm_start(const tqgpu_solver *s, int *mode) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_get_warm_start"))) return rc;
    if (mode) *mode = s->warm.mode;
    return TQGPU_OK;
}

/* ---- the shift: after a step the realised child of the root is the new root, and every node starts from its image's duals and sets ---- */
namespace {
/* img[k], and rep[k] != 0 where the image is a repeated leaf (img[k] == img[dad(k)]).  Nodes are numbered level by level, so kid0 is the
 * running sum of nk and a parent's image is known before its children's.  The fit of nx is applied last and does not propagate: a node
 * below one whose image does not fit still has the image its path gives it. */
int shift_map_core(int Nn, const int *nk, const int *nx, int realised, int leaf, std::vector<int> &img, std::vector<char> &rep, const char *who) {
    if (Nn < 1 || !nk || !nx) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments");
    if (leaf != TQGPU_SHIFT_LEAF_REPEAT && leaf != TQGPU_SHIFT_LEAF_ZERO) return fail(TQGPU_EINVAL, std::string(who) + ": unknown leaf policy " + std::to_string(leaf));
    std::vector<int> kid0((size_t)Nn);
    long at = 1;
    for (int k = 0; k < Nn; k++) {
        if (nk[k] < 0 || (k > 0 && at <= k)) return fail(TQGPU_EINVAL, std::string(who) + ": nk does not describe a tree numbered level by level");
        kid0[(size_t)k] = (int)at;
        at += nk[k];
        if (at > Nn) return fail(TQGPU_EINVAL, std::string(who) + ": nk names more than Nn nodes");
    }
    if (at != Nn) return fail(TQGPU_EINVAL, std::string(who) + ": nk names " + std::to_string(at) + " nodes, Nn is " + std::to_string(Nn));
    img.assign((size_t)Nn, -1); rep.assign((size_t)Nn, 0);
    if (Nn == 1) return TQGPU_OK;          /* (a tree of one node: an empty map, whatever `realised`) */
    if (realised < 0 || realised >= nk[0]) return fail(TQGPU_EINVAL, std::string(who) + ": realised = " + std::to_string(realised) + ", the root has " + std::to_string(nk[0]) + " children");
    img[0] = kid0[0] + realised;
    for (int p = 0; p < Nn; p++) {
        const int ip = img[(size_t)p];
        for (int c = 0; c < nk[p]; c++) {
            const int k = kid0[(size_t)p] + c;
            if (ip < 0) continue;
            if (nk[ip] > 0) img[(size_t)k] = kid0[(size_t)ip] + std::min(c, nk[ip] - 1);
            else if (leaf == TQGPU_SHIFT_LEAF_REPEAT) { img[(size_t)k] = ip; rep[(size_t)k] = 1; }
        }
    }
    for (int k = 0; k < Nn; k++) if (img[(size_t)k] >= 0 && nx[img[(size_t)k]] != nx[k]) { img[(size_t)k] = -1; rep[(size_t)k] = 0; }
    return TQGPU_OK;
}
}  // namespace

extern "C" int tqgpu_shift_map(int Nn, const int *nk, const int *nx, int realised, int leaf, int *img) {
    std::vector<int> m; std::vector<char> rep;
    int rc = shift_map_core(Nn, nk, nx, realised, leaf, m, rep, "tqgpu_shift_map");
    if (rc != TQGPU_OK) return rc;
    if (!img) return fail(TQGPU_EINVAL, "tqgpu_shift_map: img is required");
    if (Nn > 1) std::copy(m.begin(), m.end(), img);
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_set_shift(tqgpu_solver *s, int leaf, unsigned what) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_shift"))) return rc;
    if (what & ~(unsigned)(TQGPU_SHIFT_DUALS | TQGPU_SHIFT_WORKING_SETS)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_shift: unknown bits in `what`");
    if (what != 0 && !(what & TQGPU_SHIFT_DUALS)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_shift: the working sets move with the duals (TQGPU_SHIFT_DUALS | TQGPU_SHIFT_WORKING_SETS)");
    if (what != 0 && leaf != TQGPU_SHIFT_LEAF_REPEAT && leaf != TQGPU_SHIFT_LEAF_ZERO) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_shift: unknown leaf policy " + std::to_string(leaf));
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* (a launch in flight may still read the tables that go) */
    s->mem.release(s->shift.d); s->mem.release(s->shift.d_keep);
    s->shift.what = 0; s->shift.realised = 0; s->shift.restore = 0;
    if (s->warm.mode == 2) s->warm.mode = 1;
    if (what == 0) return TQGPU_OK;
    /* the caller's dimensions: the phantom root states are not theirs (and node 0's entries are copied unshifted whatever its image) */
    const int Nn = s->Nn, nreal = std::max(s->nk[0], 1);
    std::vector<int> nxu(s->nx.begin(), s->nx.begin() + Nn);
    nxu[0] -= s->x_pad;
    std::vector<int> tab((size_t)nreal * ((size_t)s->sum_nx + (size_t)Nn), -1), img;
    std::vector<char> rep;
    for (int j = 0; j < nreal; j++) {
        if ((rc = shift_map_core(Nn, s->nk.data(), nxu.data(), j, leaf, img, rep, "tqgpu_mpc_set_shift"))) return rc;
        int *src = tab.data() + (size_t)j * s->sum_nx, *node = tab.data() + (size_t)nreal * s->sum_nx + (size_t)j * Nn;
        for (int i = 0; i < s->nx[0]; i++) src[s->xoff[0] + i] = s->xoff[0] + i;
        for (int k = 1; k < Nn; k++) {
            const int m = img[(size_t)k];
            if (m < 0) continue;
            for (int i = 0; i < s->nx[k]; i++) src[s->xoff[k] + i] = s->xoff[m] + i;
        }
        /* the sets: never from a repeated leaf, never to the root of a tree with phantom states (its bits are laid out otherwise) */
        for (int k = 0; k < Nn; k++) {
            const int m = img[(size_t)k];
            if (m > k && !rep[(size_t)k] && !(k == 0 && s->x_pad > 0)) node[k] = m;
        }
    }
    if ((rc = s->mem.upload(s->shift.d, tab.data(), sizeof(int) * tab.size(), TQGPU_ENOMEM, "the shift maps")) ||
        (rc = s->mem.zeroed(s->shift.d_keep, sizeof(double) * (size_t)std::max(s->sum_nx, 1), TQGPU_ENOMEM, "the saved start buffer"))) {
        s->mem.release(s->shift.d); s->mem.release(s->shift.d_keep);
        return rc;
    }
    s->shift.leaf = leaf; s->shift.what = what;
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_set_realised(tqgpu_solver *s, int child) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_set_realised"))) return rc;
    if (child < 0 || child >= std::max(s->nk[0], 1)) return fail(TQGPU_EINVAL, "tqgpu_mpc_set_realised: child = " + std::to_string(child) + ", the root has " + std::to_string(s->nk[0]) + " children");
    s->shift.realised = child;
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_get_shift(const tqgpu_solver *s, int *leaf, unsigned *what, int *realised) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_get_shift"))) return rc;
    if (leaf) *leaf = s->shift.leaf;
    if (what) *what = s->shift.what;
    if (realised) *realised = s->shift.realised;
    return TQGPU_OK;
}

/* the shift alone: one launch of k_mpc_pre (block nk0 for the sets, the warm blocks for the duals) on the mirror's stream, nothing waited for */
extern "C" int tqgpu_mpc_shift(tqgpu_solver *s) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_mpc_shift"))) return rc;
    if (!s->shift.d) return fail(TQGPU_EINVAL, "tqgpu_mpc_shift: the maps have not been built yet (tqgpu_mpc_set_shift)");
    if (s->solve_no < 1) return fail(TQGPU_EINVAL, "tqgpu_mpc_shift: this mirror has not solved yet: there are no duals to shift");
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = launch_mpc_pre(s, MpcPre{.warm = true, .shift = true}))) return rc;
    if (s->warm.mode == 0) s->shift.restore = 1;          /* the start buffer is lent for one solve (mpc_item has the kernel save the caller's) */
    s->warm.fresh = true;          /* the next solve starts from the start buffer as it is now, in any mode */
    return TQGPU_OK;
}

/* the hot-start halves of the stored working sets, [0, Nn) of bmask, rmask and of both parts of sides; 0 on nodes of kinds 0 and 1 */
extern "C" int tqgpu_get_working_sets(tqgpu_solver *s, unsigned long long *bounds, unsigned long long *rows, unsigned long long *bound_sides, unsigned long long *row_sides) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_get_working_sets"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t Nn = (size_t)s->Nn, bytes = sizeof(unsigned long long) * Nn;
    const bool sets = s->sk.working_sets(Nn), rows_there = sets && s->sk.gen && s->rows.d_rmask;
    unsigned long long *out[4] = {bounds, rows, bound_sides, row_sides};
    const unsigned long long *from[4] = {sets ? s->D.bmask : nullptr, rows_there ? s->rows.h_gen.rmask : nullptr, rows_there ? s->rows.h_gen.sides : nullptr, rows_there ? s->rows.row_sides(Nn) : nullptr};
    for (int a = 0; a < 4; a++) {
        if (!out[a]) continue;
        if (from[a]) HIP_TRY(hipMemcpy(out[a], from[a], bytes, hipMemcpyDeviceToHost));
        else std::fill(out[a], out[a] + Nn, 0ull);
        for (size_t k = 0; k < Nn; k++) if (!sets || s->sk.h_kind[k] < 2 || ((a == 1 || a == 3) && s->sk.h_kind[k] != 3)) out[a][k] = 0ull;
    }
    return TQGPU_OK;
}

extern "C" int tqgpu_set_working_sets(tqgpu_solver *s, const unsigned long long *bounds, const unsigned long long *rows, const unsigned long long *bound_sides, const unsigned long long *row_sides) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_set_working_sets"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t Nn = (size_t)s->Nn, bytes = sizeof(unsigned long long) * Nn;
    const bool sets = s->sk.working_sets(Nn), rows_there = sets && s->sk.gen && s->rows.d_rmask;
    if (!sets) return TQGPU_OK;          /* no node of kind 2 or 3: nothing reads a set */
    const unsigned long long *in[4] = {bounds, rows, bound_sides, row_sides};
    unsigned long long *to[4] = {s->D.bmask, rows_there ? s->rows.h_gen.rmask : nullptr, rows_there ? s->rows.h_gen.sides : nullptr, rows_there ? s->rows.row_sides(Nn) : nullptr};
    std::vector<unsigned long long> w(Nn);
    for (int a = 0; a < 4; a++) {
        if (!in[a] || !to[a]) continue;
        HIP_TRY(hipMemcpy(w.data(), to[a], bytes, hipMemcpyDeviceToHost));          /* (the words of the other nodes stay) */
        for (size_t k = 0; k < Nn; k++) if (s->sk.h_kind[k] >= 2 && !((a == 1 || a == 3) && s->sk.h_kind[k] != 3)) w[k] = in[a][k];
        HIP_TRY(hipMemcpy(to[a], w.data(), bytes, hipMemcpyHostToDevice));
    }
    return TQGPU_OK;
}

extern "C" int tqgpu_get_root_terms(tqgpu_solver *s, double *b_kids, double *r0, double *dmin0, double *dmax0) {
    int rc;
    if ((rc = mpc_refuse(s, "tqgpu_get_root_terms"))) return rc;
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    size_t nb = 0;
    for (int c = 0; c < s->nk[0]; c++) nb += (size_t)s->nx[(size_t)s->kid0[0] + c];
    if (b_kids && nb) HIP_TRY(hipMemcpy(b_kids, s->b + s->xoff[(size_t)s->kid0[0]], sizeof(double) * nb, hipMemcpyDeviceToHost));          /* the children are nodes 1 .. nk[0]: one piece */
    if (r0 && s->nu[0] > 0) HIP_TRY(hipMemcpy(r0, s->r, sizeof(double) * (size_t)s->nu[0], hipMemcpyDeviceToHost));
    const int nc0 = s->rows.nc.empty() || !s->rows.d_drange ? 0 : s->rows.nc[0];
    if (dmin0 && nc0) HIP_TRY(hipMemcpy(dmin0, s->rows.d_drange, sizeof(double) * (size_t)nc0, hipMemcpyDeviceToHost));
    if (dmax0 && nc0) HIP_TRY(hipMemcpy(dmax0, s->rows.d_drange + s->rows.sum_nc, sizeof(double) * (size_t)nc0, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

/* tqgpu_mpc_step (t0 = -1) and tqgpu_mpc_step_at: the window fold, where there is one, rides in the step's one launch ahead of the solve */
static int mpc_step_impl(tqgpu_solver *s, const double *x0, int t0, const tqgpu_opts *o, tqgpu_result *res, double *u0, const char *who) {
    int rc;
    if ((rc = mpc_refuse(s, who))) return rc;
    if (!o || !res || !u0) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments");
    if ((rc = mpc_take_x0(s, nullptr, who)) || (rc = mpc_take_window(s, t0, false, who))) return rc;          /* (the refusals, before anything is touched) */
    SETTLE(s);
    HIP_TRY(hipSetDevice(s->device));
    MpcLive live;
    if ((rc = mpc_take_x0(s, x0, who)) || (rc = mpc_take_window(s, t0, true, who))) return rc;
    const MpcPre pre{.fold = x0 != nullptr, .warm = mpc_warm_due(s), .track = t0 >= 0};
    if ((pre.fold || pre.warm || pre.track) && (rc = launch_mpc_pre(s, pre))) return rc;
    s->warm.fresh = true;          /* the start buffer is ready: solve_begin copies nothing */
    if (s->persist.backoff > 0 && --s->persist.backoff == 0) s->persist.use = s->persist.use_orig;
    const bool certify = s->mpc.certify;
    s->mpc.cert_valid = false;
    if (certify && (rc = setup_kkt(s, false))) return rc;          /* (allocations, the first time: ahead of the launch) */
    SolveCtx cx(read_solve_env(false), route_of(s, o, false));
    if ((rc = solve_begin(s, o, cx)) != TQGPU_OK) return rc;
    const int launches0 = cx.launches;
    const double *tag = s->mpc.h + s->mpc.nx0 + s->nu[0];
    /* what goes out behind the solve: of a certified step the packing of the point (which dual buffer is current is the device's knowledge, as
     * behind tqgpu_set_export_ahead), the two KKT kernels and the download of their head; then the post, whose tag therefore covers them all */
    auto behind = [&]() -> int {
        int rcb;
        if (certify && (rcb = mpc_enqueue_certificate(s))) return rcb;
        if ((rcb = mpc_post_one(s))) return rcb;
        return mpc_wait_tag(tag, s->mpc.tag, s->stream);
    };
    /* a single launch: all of it goes out behind it now, and the host waits for the tag alone -- the verdict is in the result block by then */
    bool ahead = single_launch(cx.route);
    if (ahead) {
        const MpcStats mark = g_mpc_stats;
        if (behind() != TQGPU_OK) {          /* (solve_end says what became of the launch; all of it is enqueued again behind it, and counted then) */
            ahead = false;
            g_mpc_stats.launches = mark.launches; g_mpc_stats.copies = mark.copies;
        }
    }
    rc = solve_end(s, o, cx, res);
    if (rc == TQGPU_ETIMEOUT) { rc = solve_after_timeout(s, o, cx.env, res); ahead = false; }
    if (rc != TQGPU_OK) return rc;
    MPC_COUNT(launches, res->n_launches);
    if (ahead && res->n_launches != launches0) ahead = false;          /* further trials or a relaunch moved u behind the post */
    if (!ahead && (rc = behind())) return rc;
    memcpy(u0, s->mpc.h + s->mpc.nx0, sizeof(double) * (size_t)s->nu[0]);
    if (certify) {
        memcpy(s->mpc.cert, s->kkt.h, sizeof(s->mpc.cert));
        s->mpc.cert_valid = true;
        s->out.packed_on_device();          /* d_out holds the returned point: tqgpu_kkt_residual reads it there, tqgpu_get_solution downloads it */
    }
    return TQGPU_OK;
}
extern "C" int tqgpu_mpc_step(tqgpu_solver *s, const double *x0, const tqgpu_opts *o, tqgpu_result *res, double *u0) { return mpc_step_impl(s, x0, -1, o, res, u0, "tqgpu_mpc_step"); }
extern "C" int tqgpu_mpc_step_at(tqgpu_solver *s, const double *x0, int t0, const tqgpu_opts *o, tqgpu_result *res, double *u0) { return mpc_step_impl(s, x0, t0, o, res, u0, "tqgpu_mpc_step_at"); }

/* ---- the batch step: per device one launch ahead of the waves of tqgpu_solve_batch, one behind them ---- */
struct MpcDevice {
    int device = 0;
    tqgpu_solver *lead = nullptr;      /* the device's first member: its stream carries both launches, its mirror owns the descriptors and the u0 block */
    std::vector<int> idx;              /* the device's members, indices into the batch */
    bool ordered = false;              /* every launch of a later wave finds the launch ahead complete */
    bool posted = false;               /* u[0] of all members is in the block, behind their last launch */
    std::vector<int> launches0;        /* per member of idx: launches when its solve had begun (an ahead post is valid if none followed) */
    size_t n_u0 = 0;                   /* doubles of u0 in the block; the tag lies behind them */
};
struct MpcBatch { std::vector<MpcDevice> dev; };

static MpcDevice *mpc_device_of(MpcBatch &mb, int device) {
    for (MpcDevice &d : mb.dev) if (d.device == device) return &d;
    return nullptr;
}
/* the stream a member's solve launches on in this wave: its group's lead's, or its own */
static hipStream_t mpc_launch_stream(const BatchMember &m, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg) {
    const BatchGroup *g = group_of(m, wg, dg, pg);
    return g ? g->lead->stream : m.s->stream;
}
static int mpc_post_batch(MpcDevice &d) {
    tqgpu_solver *lead = d.lead;
    unsigned long long *tag = reinterpret_cast<unsigned long long *>(lead->mpcb.h_u0s + d.n_u0);
    hipLaunchKernelGGL(k_mpc_post_batch, dim3(1), dim3(256), 0, lead->stream, lead->mpcb.d_items, (int)d.idx.size(), tag, ++lead->mpc.tag);
    HIP_TRY(hipGetLastError());
    MPC_COUNT(launches, 1);
    return mpc_wait_tag(lead->mpcb.h_u0s + d.n_u0, lead->mpc.tag, lead->stream);
}
/* A wave's launches go out on its group leads' streams and its other members' own; the launch ahead is on the device lead's.  The first wave of
 * a device that launches anywhere else waits for that stream once; a later wave comes after a verdict of the first, which came after the launch.
 * A member of the persistent group launches on the lead's stream, but packs its constants on its OWN stream where a re-pack is pending (launch_persist:
 * k_pack_persist, first solves and changed data only), and the pack reads what the fold writes -- the root's bounds of a root that keeps its
 * states, Data::r: such a member counts as launching elsewhere, so its pack finds the fold complete. */
static int mpc_before_wave(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int j, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg) {
    MpcDevice *d = mpc_device_of(mb, tab[(size_t)i].s->device);
    if (!d || d->ordered) return TQGPU_OK;
    bool elsewhere = false;
    for (int k = i; k < j; k++) {
        const BatchMember &m = tab[(size_t)k];
        elsewhere |= mpc_launch_stream(m, wg, dg, pg) != d->lead->stream;
        elsewhere |= m.in_persist && m.s->persist.need_pack && m.s->stream != d->lead->stream;
    }
    if (elsewhere) { HIP_TRY(hipStreamSynchronize(d->lead->stream)); MPC_COUNT(waits, 1); }
    d->ordered = true;
    return TQGPU_OK;
}
/* behind the launches of a wave that holds all members of its device, every one of them a single launch on the device lead's stream: the post goes
 * out now and the host waits for its tag alone; the verdicts are in by then */
static int mpc_behind_launches(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int j, int ok_to, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg) {
    MpcDevice *d = mpc_device_of(mb, tab[(size_t)i].s->device);
    if (!d || ok_to != j || (size_t)(j - i) != d->idx.size() || d->idx[0] != i) return TQGPU_OK;
    for (int k = i; k < j; k++) {
        const BatchMember &m = tab[(size_t)k];
        if (!single_launch(m.cx.route) || mpc_launch_stream(m, wg, dg, pg) != d->lead->stream) return TQGPU_OK;
    }
    d->launches0.clear();
    for (int k = i; k < j; k++) d->launches0.push_back(tab[(size_t)k].cx.launches);
    if (mpc_post_batch(*d) == TQGPU_OK) d->posted = true;          /* (else: the solves' ends say what became of the launches, and the post is made again) */
    return TQGPU_OK;
}
/* the wave's launches, a shared one once; and whether a post that went out ahead still holds */
static void mpc_after_wave(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int ok_to, const tqgpu_result *results, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg) {
    for (const BatchGroup *g : {&wg, &dg, &pg}) if (g->launched) MPC_COUNT(launches, 1);
    MpcDevice *d = mpc_device_of(mb, tab[(size_t)i].s->device);
    for (int k = i; k < ok_to; k++) {
        const BatchGroup *g = group_of(tab[(size_t)k], wg, dg, pg);
        MPC_COUNT(launches, results[k].n_launches - (g && g->launched ? 1 : 0));
        if (d && d->posted && (size_t)(k - i) < d->launches0.size() && results[k].n_launches != d->launches0[(size_t)(k - i)]) d->posted = false;
    }
}

/* tqgpu_mpc_step_batch (t0s = nullptr) and tqgpu_mpc_step_batch_at: t0s[i] >= 0 moves member i's window in the launch ahead */
static int mpc_step_batch_impl(tqgpu_solver **solvers, int n, const double *x0s, const int *t0s, const tqgpu_opts *o, tqgpu_result *results, double *u0s, const char *who) {
    if (!solvers || n < 1 || !o || !results || !u0s) return fail(TQGPU_EINVAL, std::string(who) + ": bad arguments");
    int rc;
    for (int i = 0; i < n; i++) {
        if ((rc = mpc_refuse(solvers[i], who)) || (rc = mpc_take_x0(solvers[i], nullptr, who)) || (rc = mpc_take_window(solvers[i], t0s ? t0s[i] : -1, false, who))) return rc;
        for (int k = 0; k < i; k++) if (solvers[k] == solvers[i]) return fail(TQGPU_EINVAL, std::string(who) + ": a mirror is named twice");
    }
    MpcLive live;
    MpcBatch mb;
    for (int i = 0; i < n; i++) {
        MpcDevice *d = mpc_device_of(mb, solvers[i]->device);
        if (!d) { mb.dev.push_back(MpcDevice()); d = &mb.dev.back(); d->device = solvers[i]->device; d->lead = solvers[i]; }
        d->idx.push_back(i);
    }
    /* the launch ahead, per device: a member's data is touched on the lead's stream, so whatever its own stream (uploads, a solve of its own) or
     * another batch's lead's stream may still hold for it comes first -- as kkt_group_enqueue; in a loop of batch steps nothing is waited for */
    size_t x_at = 0, out_at = 0;
    std::vector<size_t> x_off((size_t)n), out_off((size_t)n);          /* member i's x0 in x0s, its u[0] in u0s */
    for (int i = 0; i < n; i++) { x_off[(size_t)i] = x_at; x_at += (size_t)solvers[i]->mpc.nx0; out_off[(size_t)i] = out_at; out_at += (size_t)solvers[i]->nu[0]; }
    auto waited_for = [](const std::vector<hipStream_t> &w, hipStream_t t) { return std::find(w.begin(), w.end(), t) != w.end(); };
    for (MpcDevice &d : mb.dev) {
        tqgpu_solver *lead = d.lead;
        const size_t nm = d.idx.size();
        HIP_TRY(hipSetDevice(lead->device));
        if ((rc = grow_items(lead, lead->mpcb.d_items, lead->mpcb.h_items, lead->mpcb.items_cap, nm))) return rc;
        d.n_u0 = 0;
        for (int i : d.idx) d.n_u0 += (size_t)solvers[i]->nu[0];
        if (lead->mpcb.u0s_cap < (int)d.n_u0 + 1) {
            HIP_TRY(hipStreamSynchronize(lead->stream));
            lead->mem.release(lead->mpcb.h_u0s); lead->mpcb.u0s_cap = 0;
            if ((rc = lead->mem.host(lead->mpcb.h_u0s, sizeof(double) * (2 * d.n_u0 + 2), "the pinned u0 block of a batch step"))) return rc;
            memset(lead->mpcb.h_u0s, 0, sizeof(double) * (2 * d.n_u0 + 2));
            lead->mpcb.u0s_cap = (int)(2 * d.n_u0 + 2);
        }
        std::vector<hipStream_t> waited;
        unsigned blocks = 1;
        bool any = false;
        size_t u_at = 0;
        for (size_t m = 0; m < nm; m++) {
            tqgpu_solver *s = solvers[d.idx[m]];
            const bool in_launch = s->links.settle_stream != nullptr;
            if (in_launch && s->links.settle_stream != lead->stream && !waited_for(waited, s->links.settle_stream)) {
                if (s->links.settle_stream != s->stream) { waited.push_back(s->links.settle_stream); MPC_COUNT(waits, 1); }
                SETTLE(s);
            }
            const bool own_solve = !in_launch && s->solve_no != s->mpcb.drained_at;
            if (s->stream != lead->stream && (s->links.stream_pending || own_solve)) {
                HIP_TRY(hipStreamSynchronize(s->stream));
                s->links.stream_pending = false;
                waited.push_back(s->stream);
                MPC_COUNT(waits, 1);
            }
            const int t0 = t0s ? t0s[d.idx[m]] : -1;
            if ((rc = mpc_take_x0(s, x0s ? x0s + x_off[(size_t)d.idx[m]] : nullptr, who)) || (rc = mpc_take_window(s, t0, true, who))) return rc;
            const MpcPre pre{.fold = x0s != nullptr, .warm = mpc_warm_due(s), .track = t0 >= 0};
            MItem &it = lead->mpcb.h_items[m];
            it = mpc_item(s, pre);
            it.u0 = lead->mpcb.h_u0s + u_at;          /* the batch's block, not the member's own */
            u_at += (size_t)s->nu[0];
            if (pre.fold || pre.warm || pre.track) { any = true; blocks = std::max(blocks, mpc_pre_grid(s, pre)); }
            if (pre.warm) s->lam_valid = false;
            s->warm.fresh = true;          /* the start buffer is ready (or stays the caller's): solve_begin copies nothing */
        }
        HIP_TRY(hipMemcpyAsync(lead->mpcb.d_items, lead->mpcb.h_items, nm * sizeof(MItem), hipMemcpyHostToDevice, lead->stream)); MPC_COUNT(copies, 1);
        if (any) {
            hipLaunchKernelGGL(k_mpc_pre_batch, dim3(blocks, (unsigned)nm), dim3(WAVE), 0, lead->stream, lead->mpcb.d_items);
            HIP_TRY(hipGetLastError());
            MPC_COUNT(launches, 1);
        }
        lead->links.stream_pending = true;
    }
    rc = solve_batch_impl(solvers, n, o, results, &mb);
    for (int i = 0; i < n; i++) solvers[i]->mpcb.drained_at = solvers[i]->solve_no;          /* (a member that launched on its own stream is waited for below, where the post is made) */
    if (rc != TQGPU_OK) return rc;
    for (MpcDevice &d : mb.dev) {
        HIP_TRY(hipSetDevice(d.lead->device));
        if (!d.posted) {
            /* the post behind everything: a member whose last launch ran on another stream than the lead's is waited for first */
            std::vector<hipStream_t> waited;
            for (int i : d.idx) {
                tqgpu_solver *s = solvers[i];
                const hipStream_t t = s->links.settle_stream ? s->links.settle_stream : s->stream;
                if (t == d.lead->stream || waited_for(waited, t)) continue;
                HIP_TRY(hipStreamSynchronize(t));
                waited.push_back(t);
                MPC_COUNT(waits, 1);
            }
            if ((rc = mpc_post_batch(d))) return rc;
        }
        size_t u_at = 0;
        for (int i : d.idx) {
            memcpy(u0s + out_off[(size_t)i], d.lead->mpcb.h_u0s + u_at, sizeof(double) * (size_t)solvers[i]->nu[0]);
            u_at += (size_t)solvers[i]->nu[0];
        }
    }
    return TQGPU_OK;
}

extern "C" int tqgpu_mpc_step_batch(tqgpu_solver **solvers, int n, const double *x0s, const tqgpu_opts *o, tqgpu_result *results, double *u0s) { return mpc_step_batch_impl(solvers, n, x0s, nullptr, o, results, u0s, "tqgpu_mpc_step_batch"); }
extern "C" int tqgpu_mpc_step_batch_at(tqgpu_solver **solvers, int n, const double *x0s, const int *t0s, const tqgpu_opts *o, tqgpu_result *results, double *u0s) { return mpc_step_batch_impl(solvers, n, x0s, t0s, o, results, u0s, "tqgpu_mpc_step_batch_at"); }

extern "C" int tqgpu_mpc_stats(int *launches, int *copies, int *waits) {
    const MpcStats &st = g_mpc_stats;
    if (launches) *launches = st.launches;
    if (copies) *copies = st.copies;
    if (waits) *waits = st.waits;
    return TQGPU_OK;
}

/*
 * tdunes_shard.hpp -- the two multi-device modes of the host part: the subtree-sharded mode with RCCL (tqgpu_shard_*, tqgpu_solve_virtual_ranks;
 * RcclApi, the ranges the ranks exchange, the two all-gathers, the partition plan and its lists) and the sharded persistent launch (tqgpu_pshard_*).
 * Included once from tdunes_device.hip inside #if TQ_HAS(TQP_HOST), behind tdunes_mpc.hpp: the entry points need solve_begin's pieces.  That file
 * keeps the mirror's records SubtreeShard (s->shard) and PersistShard (s->pshard) (in tdunes_mirror.hpp), the kernels k_shard_pack1, k_shard_pack2, k_ls_decide_parts,
 * and declares what its launches per tier and tqgpu_destroy call here: shard_desc, shard_exchange, shard_release.
 */
#pragma once

/* ============================================================================================ */
/* sharded mode: one tree over several devices                                  */
/* ============================================================================================ */

namespace {

/* ---- RCCL, loaded lazily so that single-device users do not depend on it ---- */
struct RcclApi {
    void *lib = nullptr;
    struct UniqueId { char internal[128]; };
    int (*GetUniqueId)(UniqueId *) = nullptr;
    int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;

int rccl_load() {
    if (g_rccl.lib) return TQGPU_OK;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *lib = nullptr;
    for (const char *n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!lib) return fail(TQGPU_ECOMM, std::string("cannot load librccl.so: ") + dlerror());
#define SYM(field, name) g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(lib, name)); if (!g_rccl.field) return fail(TQGPU_ECOMM, std::string("librccl.so lacks ") + name)
    SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllGather, "ncclAllGather"); SYM(GroupStart, "ncclGroupStart"); SYM(GroupEnd, "ncclGroupEnd"); SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.lib = lib;
    return TQGPU_OK;
}
constexpr int NCCL_DOUBLE = 8;     /* ncclFloat64 */

#define NCCL_TRY(expr) do { int r_ = (expr); if (r_ != 0) return fail(TQGPU_ECOMM, std::string(#expr) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error")); } while (0)

Shard shard_desc(const tqgpu_solver *s, int tier) {
    Shard sh{};
    if (s->shard.on) {
        if (tier >= 0 && tier <= s->shard.part_top) sh.wg_off = s->shard.rank * (s->uni.tier_grid[tier] / s->shard.nranks);
        sh.gh_list = s->shard.d_gh_list; sh.gh_n = s->shard.gh_n; sh.gh_counted = s->shard.gh_counted;
        sh.err_src = s->shard.d_xerr;
    }
    return sh;
}

/* a rank-partitioned range: rank r's share is base[r * per_rank, (r + 1) * per_rank) */
struct RangeSpec { double *base; size_t per_rank; };

/* what the ranks exchange per Newton iteration.  which = 1 (after the last partitioned backward tier): Schur records of the boundary
 * subtree roots and the termination partials; which = 2 (after a trial sweep): {fval, dot} partials and x / QinvCal of the boundary
 * root nodes */
std::vector<RangeSpec> exchange_ranges(tqgpu_solver *s, int which) {
    const size_t NX = (size_t)s->uni.fNX, SCH = NX * NX + NX;
    const size_t f0 = (size_t)uni_first(s->uni.fMD, s->uni.tier_l0[s->shard.part_top]), w = (size_t)(s->uni.tier_grid[s->shard.part_top] / s->shard.nranks);
    if (which == 1) return {{s->D.Sbuf + f0 * SCH, w * SCH}, {s->shard.d_xerr, 1}};
    return {{s->shard.d_xs, 2}, {s->D.x + NX * f0, w * NX}, {s->D.QinvCal + NX * f0, w * NX}};
}

/* the partitioned part of the solution, one set of ranges per node level >= the boundary level: for the gather after a solve */
std::vector<RangeSpec> solution_ranges(tqgpu_solver *s) {
    std::vector<RangeSpec> out;
    const int MD = s->uni.fMD, NX = s->uni.fNX, NU = s->uni.fNU, N = s->shard.nranks;
    const int lb = s->uni.tier_l0[s->shard.part_top];
    const Data &D = s->D;
    double *lamc = s->h_ctrl->cur ? D.lam1 : D.lam0;
    for (int l = lb; l <= s->Nh; l++) {
        const size_t f0 = (size_t)uni_first(MD, l), w = (size_t)uni_width(MD, l) / N;
        double *xs[] = {D.x, D.xUnc, D.xUncS, lamc, D.dlam};
        for (double *a : xs) out.push_back({a + NX * f0, w * NX});
        if (l < s->Nh) { double *us[] = {D.u, D.uUnc, D.uUncS}; for (double *a : us) out.push_back({a + NU * f0, w * NU}); }
    }
    return out;
}

/* the RCCL transport: one group of in-place all-gathers on the solver's stream, in the order of the list */
int allgather_rccl(tqgpu_solver *s, const std::vector<RangeSpec> &ranges) {
    NCCL_TRY(g_rccl.GroupStart());
    for (const RangeSpec &rg : ranges) NCCL_TRY(g_rccl.AllGather(rg.base + (size_t)s->shard.rank * rg.per_rank, rg.base, rg.per_rank, NCCL_DOUBLE, s->shard.comm, s->stream));
    NCCL_TRY(g_rccl.GroupEnd());
    return TQGPU_OK;
}

/* one exchange point of a Newton iteration on the launch-per-tier path (launch_fast_iteration, launch_trial) */
int shard_exchange(tqgpu_solver *s, int which) { return allgather_rccl(s, exchange_ranges(s, which)); }

/* the same between `n` mirrors living in one process on one device ("virtual ranks", to validate the partition / hand-off logic on a
 * single GPU).  ranges_of is asked per mirror: a mirror's h_ctrl->cur selects its own dual buffer */
template <typename F>
int allgather_virtual(tqgpu_solver **R, int n, F ranges_of) {
    for (int r = 0; r < n; r++) HIP_TRY(hipStreamSynchronize(R[r]->stream));
    /* every source stream is idle now; the copies are ordered on the DESTINATION mirror's stream, in
     * front of its next phase (the solver streams are non-blocking: the null stream would not order) */
    for (int src = 0; src < n; src++) for (int dst = 0; dst < n; dst++) {
        if (src == dst) continue;
        const std::vector<RangeSpec> from = ranges_of(R[src]), to = ranges_of(R[dst]);
        for (size_t i = 0; i < from.size(); i++)
            HIP_TRY(hipMemcpyAsync(to[i].base + (size_t)src * to[i].per_rank, from[i].base + (size_t)src * from[i].per_rank, sizeof(double) * from[i].per_rank, hipMemcpyDeviceToDevice, R[dst]->stream));
    }
    for (int r = 0; r < n; r++) HIP_TRY(hipStreamSynchronize(R[r]->stream));
    return TQGPU_OK;
}

/* The partition of a uniform tree over `N` ranks, host arithmetic only: tiers whose subtree count is a multiple of N
 * are partitioned by contiguous subtree ranges, the tiers above are replicated.  Used by shard_build_lists and exported as
 * tqgpu_shard_plan (the CPU tests compare it with the Python planner the gloo protocol tests use). */
struct ShardPlanHost {
    int part_top = -1, lb = 0, gh_counted = 0;
    int bnd_b0 = 0, bnd_bn = 0, bnd_own0 = 0, bnd_ownn = 0;
    std::vector<int> gh, nodes, nodes_cnt, blks;
};

int shard_plan_host(int MD, int NX, int Nh, const std::vector<int> &tier_l0, const std::vector<int> &tier_grid, int N, int r, ShardPlanHost &P) {
    const int nt = (int)tier_l0.size();
    /* highest partitioned tier: subtree count divisible by the number of ranks */
    P.part_top = -1;
    for (int i = 0; i < nt - 1; i++) if (tier_grid[i] % N == 0 && tier_grid[i] >= N) P.part_top = i;
    if (P.part_top < 0) return fail(TQGPU_EUNSUPPORTED, "tree too small to shard over this many ranks");
    const int lb = tier_l0[P.part_top], l00 = tier_l0[0];
    P.lb = lb;
    {
        const int gb = uni_width(MD, lb), w = gb / N;
        P.bnd_b0 = NX * uni_first(MD, lb); P.bnd_bn = NX * gb; P.bnd_own0 = NX * r * w; P.bnd_ownn = NX * w;
    }
    std::vector<int> &gh = P.gh, &nodes = P.nodes, &nodes_cnt = P.nodes_cnt, &blks = P.blks;
    gh.clear(); nodes.clear(); nodes_cnt.clear(); blks.clear();
    /* owned */
    for (int l = lb; l <= Nh; l++) {
        const int w = uni_width(MD, l) / N, f0 = uni_first(MD, l) + r * w;
        for (int i = 0; i < w; i++) {
            nodes.push_back(f0 + i); nodes_cnt.push_back(f0 + i);
            if (l < Nh) blks.push_back(f0 + i);
            if (l < l00) gh.push_back(f0 + i);
        }
    }
    P.gh_counted = (int)gh.size();
    /* replicated (levels above the boundary): computed by every rank, counted by rank 0 only */
    for (int l = 0; l < lb; l++) {
        const int w = uni_width(MD, l), f0 = uni_first(MD, l);
        for (int i = 0; i < w; i++) {
            nodes.push_back(f0 + i); gh.push_back(f0 + i);
            if (r == 0) { nodes_cnt.push_back(f0 + i); blks.push_back(f0 + i); }
        }
    }
    if (r == 0) P.gh_counted = (int)gh.size();
    return TQGPU_OK;
}

int shard_build_lists(tqgpu_solver *s) {
    const int N = s->shard.nranks;
    ShardPlanHost P;
    int rcp = shard_plan_host(s->uni.fMD, s->uni.fNX, s->Nh, s->uni.tier_l0, s->uni.tier_grid, N, s->shard.rank, P);
    if (rcp) return rcp;
    s->shard.part_top = P.part_top;
    s->shard.bnd_b0 = P.bnd_b0; s->shard.bnd_bn = P.bnd_bn; s->shard.bnd_own0 = P.bnd_own0; s->shard.bnd_ownn = P.bnd_ownn;
    std::vector<int> &gh = P.gh, &nodes = P.nodes, &nodes_cnt = P.nodes_cnt, &blks = P.blks;
    s->shard.gh_counted = P.gh_counted;
    s->shard.gh_n = (int)gh.size(); s->shard.n_nodes = (int)nodes.size(); s->shard.n_nodes_counted = (int)nodes_cnt.size(); s->shard.n_blk_counted = (int)blks.size();
    const size_t ints = gh.size() + nodes.size() + nodes_cnt.size() + blks.size() + 16;
    const size_t bytes = ints * sizeof(int) + (3 * (size_t)N + 8) * sizeof(double) + 1024;
    s->mem.release(s->shard.slab);
    if (int rc = s->mem.zeroed(s->shard.slab, bytes, TQGPU_ENODEVICE, "the shard lists")) return rc;
    char *p = static_cast<char *>(s->shard.slab);
    s->shard.d_xerr = reinterpret_cast<double *>(p); p += sizeof(double) * (size_t)(N + 2);
    s->shard.d_xs = reinterpret_cast<double *>(p); p += sizeof(double) * (size_t)(2 * N + 2);
    auto put = [&](std::vector<int> &v, int *&dst) -> int {
        dst = reinterpret_cast<int *>(p); p += sizeof(int) * (v.size() + 2);
        if (!v.empty() && hipMemcpy(dst, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(TQGPU_ENODEVICE, "shard list upload failed");
        return TQGPU_OK;
    };
    int rc;
    if ((rc = put(gh, s->shard.d_gh_list)) || (rc = put(nodes, s->shard.d_node_list)) || (rc = put(nodes_cnt, s->shard.d_node_cnt_list)) || (rc = put(blks, s->shard.d_blk_list))) return rc;
    return TQGPU_OK;
}

void set_shard(tqgpu_solver *s, int rank, int nranks, bool on) { s->shard.rank = rank; s->shard.nranks = nranks; s->shard.on = on; }

void shard_release(tqgpu_solver *s) {      /* tqgpu_destroy: the peer slabs opened through IPC handles, the communicator */
    for (int r = 0; r < 8; r++) if (s->pshard.ipc[r]) (void)hipIpcCloseMemHandle(s->pshard.ipc[r]);
    if (s->shard.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(s->shard.comm);
}

/* the table of the ranks' slabs (sharded persistent launch), host to device */
int upload_peers(tqgpu_solver *s) {
    HIP_TRY(hipMemcpy(s->pshard.d_peers, s->pshard.h_peers, sizeof(s->pshard.h_peers), hipMemcpyHostToDevice));
    return TQGPU_OK;
}

}  // namespace

extern "C" int tqgpu_shard_unique_id(void *id128) {
    if (!id128) return fail(TQGPU_EINVAL, "null id buffer");
    int rc = rccl_load();
    if (rc) return rc;
    RcclApi::UniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return TQGPU_OK;
}

/* the partition plan without a device (host arithmetic of shard_build_lists): uniform complete md-ary tree with Nh block levels, tiers
 * of the fused path (3 levels for md = 2, 2 for md <= 4, else 1).  Lists may be NULL / caps 0 to query the sizes only. */
extern "C" int tqgpu_shard_plan(int md, int nx, int Nh, int nranks, int rank, int *part_top, int *boundary_level, int *gh_counted,
                                int *gh_list, int gh_cap, int *gh_n, int *owned_nodes, int owned_cap, int *owned_n) {
    if (md < 2 || Nh < 2 || nranks < 1 || rank < 0 || rank >= nranks) return fail(TQGPU_EINVAL, "tqgpu_shard_plan: bad arguments");
    const int TH = md == 2 ? 3 : (md <= 4 ? 2 : 1);
    std::vector<int> l0v, gridv;
    for (const UniTier &t : uni_tiers(Nh, TH, md)) { l0v.push_back(t.l0); gridv.push_back(t.grid); }
    ShardPlanHost P;
    int rc = shard_plan_host(md, nx, Nh, l0v, gridv, nranks, rank, P);
    if (rc) return rc;
    if (part_top) *part_top = P.part_top;
    if (boundary_level) *boundary_level = P.lb;
    if (gh_counted) *gh_counted = P.gh_counted;
    if (gh_n) *gh_n = (int)P.gh.size();
    if (gh_list) for (int i = 0; i < (int)P.gh.size() && i < gh_cap; i++) gh_list[i] = P.gh[(size_t)i];
    /* owned nodes = the partitioned part of the node list (levels >= boundary), in level order */
    int no = 0;
    const int first_repl = uni_first(md, P.lb);
    for (int v : P.nodes) if (v >= first_repl) { if (owned_nodes && no < owned_cap) owned_nodes[no] = v; no++; }
    if (owned_n) *owned_n = no;
    return TQGPU_OK;
}

extern "C" int tqgpu_shard_init(tqgpu_solver *s, int rank, int nranks, const void *id128) {
    SETTLE(s);
    if (!s || nranks < 1 || rank < 0 || rank >= nranks) return fail(TQGPU_EINVAL, "tqgpu_shard_init: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    if (s->shard.comm) { (void)g_rccl.CommDestroy(s->shard.comm); s->shard.comm = nullptr; }      /* a second call replaces the communicator, it does not leak it */
    /* one rank WITHOUT a communicator = back to the unsharded mirror; one rank WITH one = the sharded code path on a single device
     * (every exchange is a one-rank in-place all-gather): exercises rccl_load / ncclCommInitRank / ncclAllGather where only one GPU exists */
    if (nranks == 1 && !id128) { set_shard(s, 0, 1, false); return TQGPU_OK; }
    if (s->uni.fast < 0 || !s->uni.use_fast || s->uni.mstage) return fail(TQGPU_EUNSUPPORTED, "sharding needs the fused uniform-tree path");
    set_shard(s, rank, nranks, true);
    s->out.invalidate();
    int rc = shard_build_lists(s);
    if (rc) { set_shard(s, 0, 1, false); return rc; }
    if (id128) {
        if ((rc = rccl_load())) { set_shard(s, 0, 1, false); return rc; }
        RcclApi::UniqueId id;
        memcpy(&id, id128, sizeof(id));
        NCCL_TRY(g_rccl.CommInitRank(&s->shard.comm, nranks, id, rank));
    }
    return TQGPU_OK;
}

/* after a sharded solve every rank holds valid x,u,lambda,... only for its own and the replicated
 * nodes: gather the partitioned ranges so that tqgpu_get_solution returns the full solution */
extern "C" int tqgpu_shard_gather_solution(tqgpu_solver *s) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (!s->shard.on) return TQGPU_OK;
    if (!s->shard.comm) return fail(TQGPU_ECOMM, "no communicator (virtual ranks gather through tqgpu_solve_virtual_ranks)");
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = allgather_rccl(s, solution_ranges(s))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}

/* ============================================================================================ */
/* ONE tree over several devices INSIDE the persistent launch                                   */
/* ============================================================================================ */
/* The single-device persistent launch is a set of workgroups that talk through tagged words in one slab (tdunes_persist.hpp).
 * Sharded, the SAME set of workgroups is dealt over one launch per device: tiers whose subtree count is a multiple of the number of
 * ranks go to the ranks by contiguous subtree ranges, the tiers above them to rank 0 -- no workgroup exists twice,
 * so there is nothing to keep consistent but the words themselves.  Every rank has a slab of the same layout; a producer writes
 * each word into every slab (system-scope stores into peer-mapped memory), a consumer polls its own.  What crosses devices per
 * Newton iteration: the Schur records and x / QinvCal of the boundary subtree roots and every workgroup's termination and
 * dual-function partials upwards, the step of the boundary blocks, the line-search commands and the halt word downwards; no
 * collective, no host in the loop.  RCCL (or any transport the caller has: tqgpu_pshard_pack / _unpack) is only used to collect
 * the solution afterwards.  Every rank must call tqgpu_pshard_solve the same number of times (the launch number tags the words). */
extern "C" int tqgpu_pshard_init(tqgpu_solver *s, int rank, int nranks) {
    SETTLE(s);
    if (!s || nranks < 1 || nranks > 8 || rank < 0 || rank >= nranks) return fail(TQGPU_EINVAL, "tqgpu_pshard_init: bad arguments (1 .. 8 ranks)");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->persist.ok || s->uni.mstage || s->uni.fast < 0 || !s->uni.use_fast || !s->persist.use) return fail(TQGPU_EUNSUPPORTED, "sharding inside the persistent launch needs the persistent path of a uniform complete tree");
    s->pshard.row = find_row(SHARD_ROWS, s->uni.fNX, s->uni.fNU, s->uni.fMD);
    if (!s->pshard.row) return fail(TQGPU_EUNSUPPORTED, "the sharded persistent kernel is not instantiated for this shape (SHARD_TABLE)");
    { int rca = allow_lds(s->pshard.row->sys, s->persist.lds); if (!rca) rca = allow_lds(s->pshard.row->agent, s->persist.lds); if (rca) return rca; }
    int nwg = 0, top = -1;
    if (tqgpu_pshard_plan(s->uni.fMD, s->Nh, nranks, rank, nullptr, 0, &nwg, &top, nullptr) != 0) return fail(TQGPU_EUNSUPPORTED, "tree too small to shard over this many ranks");
    std::vector<int> map((size_t)std::max(nwg, 1));
    (void)tqgpu_pshard_plan(s->uni.fMD, s->Nh, nranks, rank, map.data(), nwg, &nwg, &top, nullptr);
    map.resize((size_t)nwg);
    if (nranks == 1) top = s->uni.n_tiers - 1;
    if ((int)map.size() > s->persist.co_capacity) return fail(TQGPU_EUNSUPPORTED, "this rank's workgroups cannot all be resident");
    s->mem.release(s->pshard.wg_map);
    if (int rc = s->mem.device(s->pshard.wg_map, sizeof(int) * std::max<size_t>(map.size(), 1), TQGPU_ENODEVICE, "this rank's workgroup table")) return rc;
    HIP_TRY(hipMemcpy(s->pshard.wg_map, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice));
    s->pshard.G = (int)map.size();
    /* First contact with real xGMI is somebody else's run, so the two things a peer's writes depend on are settled by construction:
     * (a) the slab the peers write into is FINE-GRAINED memory (coarse-grained hipMalloc memory is only guaranteed coherent across
     *     devices at kernel boundaries; this kernel polls it while the peers write), and
     * (b) the polls are system-scope loads (ps_sys: f_persist_sh<.., 1>, compiled with TQ_LD_SCOPE = system).
     * TREEQP_AMD_PSHARD_COARSE=1 / TREEQP_AMD_PSHARD_AGENT=1 restore the single-device combination for an A/B on a node. */
    s->pshard.sys = !getenv("TREEQP_AMD_PSHARD_AGENT");
    if (!s->pshard.fine && !getenv("TREEQP_AMD_PSHARD_COARSE")) {
        void *fresh = nullptr;
        if (int rc = s->mem.device(fresh, s->persist.sync_bytes, TQGPU_ENODEVICE, "the fine-grained hand-over slab", Owned::FINE_GRAINED)) return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));
        char *ob = static_cast<char *>(s->persist.sync_slab), *nb = static_cast<char *>(fresh);
        auto mv = [&](auto *&q) { if (q) q = reinterpret_cast<std::remove_reference_t<decltype(q)>>(nb + (reinterpret_cast<char *>(q) - ob)); };
        PSync &Y = s->persist.psync;
        mv(Y.sch); mv(Y.dlt); mv(Y.ndt); mv(Y.parts); mv(Y.errs); mv(Y.cmd); mv(Y.vrd); mv(Y.bparts); mv(Y.sgt); mv(Y.rfl); mv(Y.halt); mv(Y.timeout); mv(Y.base); mv(Y.verdict); mv(Y.anc);
        s->mem.release(s->persist.sync_slab);
        s->persist.sync_slab = fresh;
        s->pshard.fine = true;
        s->persist.pitems_key.clear();                                             /* (a cached batch descriptor would hold the old slab) */
    }
    s->out.invalidate();
    s->pshard.on = true; s->shard.rank = rank; s->shard.nranks = nranks; s->shard.part_top = nranks > 1 ? top : -1;
    s->persist.psync.npeer = nranks;
    s->persist.psync.anc_local = (nranks == 1 || top >= 1) ? 1 : 0;          /* tiers 0 .. top are dealt over the ranks by contiguous subtree ranges: with top >= 1 a tier-1 workgroup sits with the bottom-tier workgroups below it */
    s->persist.psync.relay_wg = (rank > 0 && !map.empty()) ? map[0] : -1;          /* ranks without the top workgroup: their first workgroup passes the verdict on to the host */
    for (int r = 0; r < 8; r++) s->pshard.h_peers[r] = s->persist.psync.base;             /* until connected: own slab */
    if (int rc = upload_peers(s)) return rc;
    s->persist.psync.nap = nap_for_grid(s->pshard.G);
    s->persist.launch_no = 0;
    HIP_TRY(hipMemsetAsync(s->persist.sync_slab, 0, s->persist.sync_bytes, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}

/* peer `r` lives in this process (several mirrors on one device, or on several devices with peer access enabled by the caller) */
extern "C" int tqgpu_pshard_connect_local(tqgpu_solver *s, int r, tqgpu_solver *peer) {
    SETTLE(s);
    if (!s || !peer || !s->pshard.on || r < 0 || r >= s->shard.nranks || !peer->persist.sync_slab || peer->persist.sync_bytes != s->persist.sync_bytes) return fail(TQGPU_EINVAL, "tqgpu_pshard_connect_local: bad arguments");
    if (peer->device != s->device) {
        HIP_TRY(hipSetDevice(s->device));
        hipError_t e = hipDeviceEnablePeerAccess(peer->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(TQGPU_ECOMM, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        (void)hipGetLastError();
    }
    s->pshard.h_peers[r] = static_cast<unsigned long long *>(peer->persist.sync_slab);
    return upload_peers(s);
}
/* peers in other processes: an IPC handle of this rank's slab (64 bytes) out, the peers' handles in */
extern "C" int tqgpu_pshard_ipc_export(tqgpu_solver *s, void *handle64) {
    if (!s || !handle64 || !s->persist.sync_slab) return fail(TQGPU_EINVAL, "tqgpu_pshard_ipc_export: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    hipIpcMemHandle_t h;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    hipError_t e = hipIpcGetMemHandle(&h, s->persist.sync_slab);
    if (e != hipSuccess) return fail(TQGPU_ECOMM, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e));
    memcpy(handle64, &h, 64);
    return TQGPU_OK;
}
extern "C" int tqgpu_pshard_ipc_connect(tqgpu_solver *s, int r, const void *handle64) {
    if (!s || !handle64 || !s->pshard.on || r < 0 || r >= s->shard.nranks || r == s->shard.rank) return fail(TQGPU_EINVAL, "tqgpu_pshard_ipc_connect: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, 64);
    void *ptr = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return fail(TQGPU_ECOMM, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
    if (s->pshard.ipc[r]) (void)hipIpcCloseMemHandle(s->pshard.ipc[r]);
    s->pshard.ipc[r] = ptr;
    s->pshard.h_peers[r] = static_cast<unsigned long long *>(ptr);
    return upload_peers(s);
}

/* one solve in two halves (so that one process can drive several ranks): _begin enqueues this rank's launch, _end waits for the
 * verdict.  All ranks' launches have to be in flight together: they wait for each other (bounded: 0.5 s, then TQGPU_ETIMEOUT). */
extern "C" int tqgpu_pshard_begin(tqgpu_solver *s, const tqgpu_opts *o) {
    SETTLE(s);
    if (!s || !o || !s->pshard.on) return fail(TQGPU_EINVAL, "tqgpu_pshard_begin: not a sharded mirror");
    HIP_TRY(hipSetDevice(s->device));
    if (o->profile || o->maxIter <= 0 || o->checkLastActiveSet == 2) return fail(TQGPU_EUNSUPPORTED, "sharded persistent solve: default solve options only (no profiling, no factor keeping)");
    Opts O;
    if (opts_from(o, O) != TQGPU_OK) return TQGPU_EINVAL;
    if (launch_no_after(s->persist.launch_no) == 0)
        return fail(TQGPU_EUNSUPPORTED, "65535 sharded solves since the launch numbers were last reset: call tqgpu_pshard_rewind on every rank, between two barriers of the caller's "
                                        "(the 16-bit launch number tags the hand-over words; a single device wipes its slab when it wraps, ranks that write into each other's slabs cannot do that on their own)");
    memset(s->h_res, 0, sizeof(HostRes));
    int launches = 0;
    s->solve_no++;
    s->out.invalidate();
    return launch_persist(s, O, launches, 1);
}
/* launch numbers back to zero and the slab wiped; peers stay connected.  EVERY rank, with no sharded solve in flight anywhere (a barrier
 * of the caller's before and after): a peer's launch that is still running, or already running again, writes into the slab being wiped */
extern "C" int tqgpu_pshard_rewind(tqgpu_solver *s) {
    SETTLE(s);
    if (!s || !s->pshard.on) return fail(TQGPU_EINVAL, "tqgpu_pshard_rewind: not a sharded mirror");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    /* (hipMemset of device memory may return before the wipe has happened; it runs on the null stream, which the solver's non-blocking
     * stream does not wait for: the wipe goes on the solver's stream and is waited for -- found by the 100 000-solve soak, where the
     * first C3 solve after a rewind lost words to the wipe) */
    HIP_TRY(hipMemsetAsync(s->persist.sync_slab, 0, s->persist.sync_bytes, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->persist.launch_no = 0;
    return TQGPU_OK;
}
/* tqgpu_pshard_end without a verdict: a time-out of a bounded wait (the sticky word, cleared here), or the error the caller names */
static int pshard_no_verdict(tqgpu_solver *s, const char *timeout_hint, int code, const char *text) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    unsigned tmo = 0;
    if (int rc = read_timeout_word(s, tmo)) return rc;
    if (!tmo) return fail(code, text);
    if (int rc = clear_timeout_word(s)) return rc;
    return fail(TQGPU_ETIMEOUT, std::string("sharded persistent solve: a bounded wait for another rank's workgroups timed out") + timeout_hint);
}
extern "C" int tqgpu_pshard_end(tqgpu_solver *s, tqgpu_result *res) {
    SETTLE(s);
    if (!s || !res || !s->pshard.on) return fail(TQGPU_EINVAL, "tqgpu_pshard_end: not a sharded mirror");
    HIP_TRY(hipSetDevice(s->device));
    /* the verdict reaches every rank's host through its pinned result block: written by the top workgroup (rank 0) or passed on from the
     * rank's slab by its relay workgroup -- no stream synchronisation on the way (the state write-back of the other workgroups is still
     * running; everything the host does next on this mirror is stream-ordered behind the launch).  (rank 0: the top workgroup's tagged
     * words; the other ranks' relay workgroups post the plain block) */
    if (!await_result_block(s->h_res, s->persist.psync.seq, true))
        return pshard_no_verdict(s, " (are all ranks' launches in flight together?)", TQGPU_ECOMM, "sharded persistent solve: no verdict from the top workgroup");
    const Ctrl &c = *s->h_ctrl;
    if (!c.done)
        return pshard_no_verdict(s, "", TQGPU_EUNSUPPORTED, "sharded persistent solve: the launch ended without a verdict (tag space exhausted: more than 60000 passes)");
    fill_result(res, c, 1, s->shard.rank == 0 ? 1e-8 * (double)(s->h_res->t_end - s->h_res->t_start) : 0.0);
    s->last_iter = c.iter;
    return TQGPU_OK;
}

/* what this rank holds of the solution (its chunk of every partitioned range; rank 0: also the levels above the partition), packed
 * into a host buffer, and the inverse: the transport hook for callers that collect the solution themselves (any all-gather of
 * equal-sized buffers: tqgpu_pshard_pack_size is the same on every rank) */
namespace {
struct PsRange { double *base; size_t n; };
std::vector<PsRange> pshard_owned_ranges(tqgpu_solver *s, int rank) {
    std::vector<PsRange> out;
    const int MD = s->uni.fMD, NX = s->uni.fNX, NU = s->uni.fNU, N = s->shard.nranks;
    const Data &D = s->D;
    double *lamc = s->h_ctrl->cur ? D.lam1 : D.lam0;
    const int lb = N > 1 ? s->uni.tier_l0[s->shard.part_top] : s->Nh + 1;
    for (int l = 0; l <= s->Nh; l++) {
        const int wl = uni_width(MD, l);
        const size_t f0 = (size_t)uni_first(MD, l);
        /* node data (x, u, ...) of level l belongs to the workgroup that owns the node; the duals of a node's own edge belong to the
         * BLOCK of its parent, one level up: the duals of the boundary level are the top tiers' (rank 0) */
        for (int what = 0; what < 2; what++) {
            const int lbw = what == 0 ? lb : lb + 1;
            size_t first, cnt;
            if (l >= lbw) { cnt = (size_t)wl / N; first = f0 + (size_t)rank * cnt; }
            else { if (rank != 0) continue; cnt = (size_t)wl; first = f0; }
            if (what == 0) {
                double *xs[] = {D.x, D.xUnc, D.xUncS};
                for (double *a : xs) out.push_back({a + NX * first, cnt * NX});
                if (l < s->Nh) { double *us[] = {D.u, D.uUnc, D.uUncS}; for (double *a : us) out.push_back({a + NU * first, cnt * NU}); }
            } else {
                double *ls[] = {lamc, D.dlam};
                for (double *a : ls) out.push_back({a + NX * first, cnt * NX});
            }
        }
    }
    return out;
}
/* rank `rank`'s ranges to the host buffer (to_host: tqgpu_pshard_pack) or from it (tqgpu_pshard_unpack) */
int copy_owned_ranges(tqgpu_solver *s, int rank, double *buf, long cap, bool to_host) {
    size_t o = 0;
    for (auto &rg : pshard_owned_ranges(s, rank)) {
        if ((long)(o + rg.n) > cap) return fail(TQGPU_EINVAL, to_host ? "tqgpu_pshard_pack: buffer too small" : "tqgpu_pshard_unpack: buffer too small");
        if (to_host) HIP_TRY(hipMemcpy(buf + o, rg.base, sizeof(double) * rg.n, hipMemcpyDeviceToHost));
        else HIP_TRY(hipMemcpy(rg.base, buf + o, sizeof(double) * rg.n, hipMemcpyHostToDevice));
        o += rg.n;
    }
    return TQGPU_OK;
}
}  // namespace
extern "C" long tqgpu_pshard_pack_size(tqgpu_solver *s) {
    if (!s || !s->pshard.on) return -1;
    size_t n = 0;
    for (auto &rg : pshard_owned_ranges(s, 0)) n += rg.n;          /* rank 0 holds the most */
    return (long)n;
}
extern "C" int tqgpu_pshard_pack(tqgpu_solver *s, double *out, long cap) {
    SETTLE(s);
    if (!s || !out || !s->pshard.on) return fail(TQGPU_EINVAL, "tqgpu_pshard_pack: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    /* tqgpu_pshard_end returns on the verdict word while the workgroups still write their state back, and the copies below run on the
     * null stream, which the solver's non-blocking stream does not order: wait for the launch first */
    HIP_TRY(hipStreamSynchronize(s->stream));
    return copy_owned_ranges(s, s->shard.rank, out, cap, true);
}
extern "C" int tqgpu_pshard_unpack(tqgpu_solver *s, int src_rank, const double *in, long n_in) {
    SETTLE(s);
    if (!s || !in || !s->pshard.on || src_rank < 0 || src_rank >= s->shard.nranks) return fail(TQGPU_EINVAL, "tqgpu_pshard_unpack: bad arguments");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));          /* (as tqgpu_pshard_pack: this rank's own write-back must not land on top of the peers' shares) */
    return copy_owned_ranges(s, src_rank, const_cast<double *>(in), n_in, false);
}

/* n mirrors of the SAME problem in this process (one device: a rehearsal with real concurrency -- n launches on n streams that wait
 * for each other inside the kernels -- or n devices with peer access): connect, solve, collect the solution into every mirror */
extern "C" int tqgpu_pshard_solve_local(tqgpu_solver **R, int n, const tqgpu_opts *o, tqgpu_result *res) {
    for (int r_ = 0; R && r_ < n; r_++) SETTLE(R[r_]);
    if (!R || n < 1 || n > 8 || !o || !res) return fail(TQGPU_EINVAL, "tqgpu_pshard_solve_local: bad arguments");
    for (int r = 0; r < n; r++) if (!R[r] || !R[r]->pshard.on || R[r]->shard.nranks != n || R[r]->shard.rank != r) return fail(TQGPU_EINVAL, "tqgpu_pshard_solve_local: mirror r must be tqgpu_pshard_init(r, n)");
    for (int r = 0; r < n; r++) for (int q = 0; q < n; q++) { int rc = tqgpu_pshard_connect_local(R[r], q, R[q]); if (rc) return rc; }
    for (int r = 0; r < n; r++) HIP_TRY(hipStreamSynchronize(R[r]->stream));          /* uploads done: the launches go out back to back */
    if (R[0]->persist.launch_no >= 0x8000u) for (int r = 0; r < n; r++) { int rc = tqgpu_pshard_rewind(R[r]); if (rc) return rc; }      /* (all ranks idle here) */
    for (int r = 0; r < n; r++) { int rc = tqgpu_pshard_begin(R[r], o); if (rc) return rc; }
    int first = TQGPU_OK;
    std::string msg;
    for (int r = 0; r < n; r++) { int rc = tqgpu_pshard_end(R[r], &res[r]); if (rc && !first) { first = rc; msg = g_err; } }
    if (first) return fail(first, msg);
    std::vector<double> buf((size_t)std::max<long>(tqgpu_pshard_pack_size(R[0]), 1));
    for (int src = 0; src < n; src++) {
        int rc = tqgpu_pshard_pack(R[src], buf.data(), (long)buf.size());
        if (rc) return rc;
        for (int dst = 0; dst < n; dst++) if (dst != src && (rc = tqgpu_pshard_unpack(R[dst], src, buf.data(), (long)buf.size()))) return rc;
    }
    return TQGPU_OK;
}

/* Diagnostic / test entry: run `n` mirrors of the SAME problem as ranks 0..n-1 of a sharded solve
 * inside one process on one device, exchanging by device copies.  Validates partition, hand-off and
 * decision logic without a multi-GPU node.  Every mirror must have been shard-initialised with
 * (rank = its index, nranks = n, id128 = NULL).  The full solution is gathered into every mirror. */
extern "C" int tqgpu_solve_virtual_ranks(tqgpu_solver **R, int n, const tqgpu_opts *o, tqgpu_result *res) {
    for (int r_ = 0; R && r_ < n; r_++) SETTLE(R[r_]);
    if (!R || n < 2 || !o || !res) return fail(TQGPU_EINVAL, "tqgpu_solve_virtual_ranks: bad arguments");
    for (int r = 0; r < n; r++) if (!R[r] || R[r]->shard.nranks != n || R[r]->shard.rank != r || R[r]->shard.comm) return fail(TQGPU_EINVAL, "mirror is not virtual rank r of n");
    HIP_TRY(hipSetDevice(R[0]->device));
    Opts O;
    if (opts_from(o, O) != TQGPU_OK) return TQGPU_EINVAL;
    int launches = 0, rc;
    for (int r = 0; r < n; r++) {
        SolveCtx prologue(SolveEnv(), Route::TIERED);          /* its launch count is dropped: n_launches reports the iterations' and trials' launches */
        if ((rc = begin_enqueued(R[r], prologue))) return rc;
    }
    auto exchange = [&](int which) { return allgather_virtual(R, n, [which](tqgpu_solver *m) { return exchange_ranges(m, which); }); };
    bool finished = o->maxIter <= 0;
    int h = 0;
    while (!finished) {
        for (int r = 0; r < n; r++) launch_fast_phase(R[r], O, h, 0, launches);
        if ((rc = exchange(1))) return rc;
        for (int r = 0; r < n; r++) launch_fast_phase(R[r], O, h, 1, launches);
        if ((rc = exchange(2))) return rc;
        for (int r = 0; r < n; r++) launch_fast_phase(R[r], O, h, 2, launches);
        for (int r = 0; r < n; r++) if ((rc = read_ctrl(R[r]))) return rc;
        while (!R[0]->h_ctrl->done && R[0]->h_ctrl->ls_pending) {
            const int it = R[0]->h_ctrl->iter, t = R[0]->h_ctrl->ls_iter;
            for (int r = 0; r < n; r++) launch_trial_phase(R[r], O, Route::TIERED, it, t, 0, launches);
            if ((rc = exchange(2))) return rc;
            for (int r = 0; r < n; r++) launch_trial_phase(R[r], O, Route::TIERED, it, t, 1, launches);
            for (int r = 0; r < n; r++) if ((rc = read_ctrl(R[r]))) return rc;
        }
        for (int r = 1; r < n; r++)
            if (R[r]->h_ctrl->iter != R[0]->h_ctrl->iter || R[r]->h_ctrl->done != R[0]->h_ctrl->done || R[r]->h_ctrl->status != R[0]->h_ctrl->status)
                return fail(TQGPU_ECOMM, "virtual ranks took different decisions");
        h = R[0]->h_ctrl->iter;
        finished = R[0]->h_ctrl->done != 0;
    }
    /* gather the partitioned solution ranges into every mirror (nothing iterated: only the wait for the streams) */
    if (o->maxIter > 0) { if ((rc = allgather_virtual(R, n, solution_ranges))) return rc; }
    else for (int r = 0; r < n; r++) {
        /* as end_enqueued: reported as "maximum iterations" with every count and both values 0, whatever the last solve left in the host copy */
        HIP_TRY(hipStreamSynchronize(R[r]->stream));
        memset(R[r]->h_ctrl, 0, sizeof(Ctrl)); R[r]->h_ctrl->status = 1;
    }
    const Ctrl &c = *R[0]->h_ctrl;
    fill_result(res, c, launches, 0.0);
    for (int r = 0; r < n; r++) R[r]->last_iter = c.iter;
    return TQGPU_OK;
}

/*
 * tdunes_mirror.hpp -- what a mirror (tqgpu_solver) is, in the host part: the last error (g_err, fail), Route, the owner of its memory (Owned),
 * the creation-time switches, one record per route (PerPhase, Wide3, SingleWg, Uniform, Persist), per feature family (Mpc*, Export, Kkt,
 * SubtreeShard, PersistShard, StageKinds, GenRows, DenseSingle) and for timing and batch membership (Timing, BatchLinks), tqgpu_solver itself,
 * and settle with the set of live streams.  No kernel here.  Included first into the host part by tdunes_device.hip, inside #if TQ_HAS(TQP_HOST).
 */
#pragma once

namespace tqd {
thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }
}  // namespace tqd

/* ============================================================================================ */
/* host side of the C-ABI                                                                       */
/* ============================================================================================ */

/* which kernels a solve launches, decided once per solve by route_of: the paths of DESIGN.md §4 (FUSED_TAILS: k_stage_f, k_grad_f) */
enum class Route { PERSIST, SINGLE_WG, TIERED, THREE_LAUNCH, FUSED_TAILS, PER_PHASE };
static bool single_launch(Route r) { return r == Route::PERSIST || r == Route::SINGLE_WG; }      /* verdict through the result block */

/* The device and pinned host memory of a mirror.  What is allocated through it is freed by tqgpu_destroy (free_all) unless it was given
 * back before (release); the named pointers of tqgpu_solver are views.  A failed call has set the error text, with `name` in it. */
struct Owned {
    std::vector<void *> dev, pinned;
    enum Fill { RAW, ZEROED, FINE_GRAINED };      /* FINE_GRAINED: hipExtMallocWithFlags (tqgpu_pshard_init) */
    static int failed(int code, const char *name, hipError_t e) { return fail(code, std::string("allocation of ") + name + " failed: " + hipGetErrorString(e)); }
    template <typename T>
    int device(T *&p, size_t bytes, int code, const char *name, Fill fill = RAW, const void *src = nullptr) {
        void *q = nullptr;
        hipError_t e = fill == FINE_GRAINED ? hipExtMallocWithFlags(&q, bytes, hipDeviceMallocFinegrained) : hipMalloc(&q, bytes);
        if (e != hipSuccess) return failed(code, name, e);
        dev.push_back(q); p = static_cast<T *>(q);
        if (fill == ZEROED) e = hipMemset(q, 0, bytes);
        if (src) e = hipMemcpy(q, src, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? TQGPU_OK : failed(code, name, e);
    }
    template <typename T> int zeroed(T *&p, size_t bytes, int code, const char *name) { return device(p, bytes, code, name, ZEROED); }
    template <typename T> int upload(T *&p, const void *src, size_t bytes, int code, const char *name) { return device(p, bytes, code, name, RAW, src); }
    template <typename T>
    int host(T *&p, size_t bytes, const char *name) {
        void *q = nullptr;
        hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return failed(TQGPU_ENOMEM, name, e);
        pinned.push_back(q); p = static_cast<T *>(q);
        return TQGPU_OK;
    }
    /* a buffer that is replaced during the mirror's life (nullptr: nothing to do) */
    template <typename T>
    void release(T *&p) {
        auto d = std::find(dev.begin(), dev.end(), (void *)p), h = std::find(pinned.begin(), pinned.end(), (void *)p);
        if (d != dev.end()) { (void)hipFree(*d); dev.erase(d); }
        else if (h != pinned.end()) { (void)hipHostFree(*h); pinned.erase(h); }
        p = nullptr;
    }
    void free_all() {
        for (void *q : dev) (void)hipFree(q);
        for (void *q : pinned) (void)hipHostFree(q);
    }
};

/* the creation-time switches: read from the environment once per tqgpu_create (read_switches), tested as fields by its steps */
struct Switches {
    bool generic, tiered, strict_sum, fwd_levels, bwd_levels, small_wide;
    bool no_fuse, no_wide3, no_sgp, no_fwd_chain, no_fwd_merge, no_stage16, gp_no_groups, no_persist_one, verbose, has_lds_pad, has_nap;
    bool dense_single, dense_batch;
    int chunk, lds_pad, capacity_margin, nap;
};

namespace { struct KItem; struct KHead; struct MItem; }      /* the descriptors of the batched KKT check and of the MPC steps, the check's head (defined with their kernels) */
namespace { struct ShapeRow; struct ShardRow; }      /* a shape's sizes and kernels, one record per line of the instantiation tables (tdunes_rows.hpp) */

/* ---- what a mirror keeps for the MPC family (tqgpu_mpc_*, tdunes_mpc.hpp), one record per feature ---- */
/* the root terms (tqgpu_mpc_set_root): d, the originals of what multiplies x0, [A0 | b0 | S0 | r0 | C0 | dmin0 | dmax0] in one device block;
 * h, pinned: x0 (nx0 doubles), u[0] (nu[0] doubles) and the tag of k_mpc_post */
struct MpcRoot {
    double *d = nullptr, *h = nullptr;
    int nx0 = 0, nb = 0, nc0 = 0;       /* nx0, rows of b0 (the children's nx), rows of C0; nx0 == 0: no root terms yet */
    bool S0 = false, C0 = false, states = false;      /* states, tqgpu_mpc_set_root_states: x0 enters as xmin[0] = xmax[0] = x0 over the root's nx[0] states; no originals (d stays null) */
    bool certify = false, cert_valid = false;      /* tqgpu_mpc_set_certify; cert holds the certificate of the last tqgpu_mpc_step */
    double cert[10] = {};               /* the head of the KKT result block (KKT_HEAD doubles) as it arrived with the step's tag */
    unsigned long long tag = 0;         /* the tag of the last u0 post this mirror waited for (its own block, or as the lead of a batch) */
};
/* tqgpu_set_warm_start; fresh: the start buffer holds what the caller (or a batch step's launch) put there for the next solve: no copy ahead of it */
struct MpcWarm { int mode = 0; bool fresh = true; };
/* the shift (tqgpu_mpc_set_shift): d, per realisation j < max(nk[0], 1) the source entry of every entry of the start buffer, [j][sum_nx]
 * ints, and behind them the node tables [j][Nn] (the image a node may take its working sets from, -1: none), in one device block;
 * d_keep: sum_nx doubles, the caller's start buffer while a tqgpu_mpc_shift of a mirror in mode 0 holds its place for one solve */
struct MpcShift {
    int *d = nullptr; double *d_keep = nullptr; int leaf = 0, realised = 0; unsigned what = 0;
    int restore = 0;                    /* 1: tqgpu_mpc_shift saved the start buffer of a mirror in mode 0, the next solve consumes the shifted one; 2: that solve has begun, the one after it puts the saved buffer back first */
};
struct MpcBatchBuf {
    long drained_at = 0;                /* as Kkt::drained_at, for the batch step's launch ahead of the solves */
    MItem *d_items = nullptr, *h_items = nullptr; int items_cap = 0;      /* batch steps: one descriptor per member of this device (the device's first member owns the array) */
    double *h_u0s = nullptr; int u0s_cap = 0;                             /* ... and their u[0] with the tag behind them, pinned */
};
/* tracking (tqgpu_mpc_set_tracking): d, [xtraj T x NXT | utraj T x NUT | q0 (sum_nx, node-indexed as Data::q, phantom root states included) |
 * r0 (sum_nu)] in one device block, the nodes' stages behind it as ints; t0: the window the device's q, r were last folded for (-1: none yet) */
struct MpcTrack { double *d = nullptr; int T = 0, nxt = 0, nut = 0, t0 = -1; };
/* ---- what a mirror keeps for the derivatives of an MPC step (tdunes_adjoint.hpp; kernels in tdunes_sens.hpp): MpcSens, MpcTan, MpcAdjBatch, MpcSensBatch, MpcAdjMat ---- */
/* tqgpu_mpc_sensitivity: buffers of its own (setup_sens, on first use; one device block d, views in v); pinned h:
 * [head: K (nu0 x nx0) | u0 (nu0) | x0_ref (nx0) | n_reg] [x0_new (nx0)] [u0_pred (nu0) | n_clipped]; valid: the stored sensitivity
 * belongs to the point and the data the device holds now (cleared by every upload, fold, window move and solve) */
struct MpcSens {
    double *d = nullptr, *h = nullptr; Sens v{}; int nx0 = 0;
    bool valid = false, dirty = false;  /* dirty: the problem was changed (upload, fold, window move) since the last solve: its point and the data no longer belong together */
    bool factored = false;              /* P, L, CholUt, invd of the point and the data the device holds now are in v (tqgpu_mpc_sensitivity, tqgpu_mpc_adjoint); valid implies it */
    size_t lds_factor = 0, lds_primal = 0;
    /* tqgpu_mpc_adjoint: buffers of its own (setup_adj, on first use and again when nw grows; one device block ad, views in a); pinned ah:
     * [w: wx ((sum_nx - x_pad) x nw) | wu (sum_nu x nw)] [head: gx0 (nx0 x nw) | n_reg]; adj_valid: the stored adjoint (nw columns)
     * belongs to the point and the data the device holds now */
    double *ad = nullptr, *ah = nullptr; Adj a{}; int nw_cap = 0, nw = 0, adj_nx0 = 0;
    bool adj_valid = false;
    size_t lds_rhs = 0, lds_grad = 0;
    bool tan_valid = false;             /* the stored tangent (MpcTan) belongs to the point and the data the device holds now */
    void invalidate() { valid = factored = adj_valid = tan_valid = false; }      /* every upload, fold, window move and solve */
};
/* tqgpu_mpc_tangent / tqgpu_mpc_predict_at: buffers of its own (setup_tan, on first use and again when nd grows or nx0 changed; one device block d,
 * views in v); pinned h: [the staged directions dq | dr | db | dx0, those given, nd columns each] and, at io, [head: du0 (nu0 x nd) | n_reg]
 * [x0_new (nx0)] [u0_pred (nu0) | n_clipped | n_reg]; nd: the columns of the stored tangent (MpcSens::tan_valid says whether it is current) */
struct MpcTan {
    double *d = nullptr, *h = nullptr, *io = nullptr; Tan v{}; int nd_cap = 0, nd = 0, nx0 = 0;
    double *stage_d = nullptr;          /* where the staged directions go on the device: (nxe + sum_nu + sum_lam + nx0) x nd_cap doubles */
    size_t lds = 0;                     /* the window of k_tan_rhs and k_tan_primal */
};
/* tqgpu_mpc_adjoint_batch, batched route (the first member of a device's group owns all three): desc, the descriptors (AItem) with the members'
 * level tables behind them, uploaded with every call in one copy; w, the loss gradients of all members, [wx | wu] member after member, one
 * copy (Adj::wx, Adj::wu of a descriptor point into d_w); heads, [gx0 | n_reg] of all members, one copy back (Adj::head points into d_heads).
 * Each is a device block and its pinned twin; the capacities are bytes of desc, doubles of w and of heads */
struct MpcAdjBatch {
    long drained_at = 0;                /* as Kkt::drained_at, for the launches of the batched adjoint */
    char *d_desc = nullptr, *h_desc = nullptr; size_t desc_cap = 0;
    double *d_w = nullptr, *h_w = nullptr; size_t w_cap = 0;
    double *d_heads = nullptr, *h_heads = nullptr; size_t heads_cap = 0;
};
/* tqgpu_mpc_sensitivity_batch and tqgpu_mpc_predict_batch, batched route (the first member of a device's group owns them): desc, the descriptors
 * (AItem) with the members' level tables behind them, one copy per call; heads, the heads of all members ([K | u0 | x0_ref | n_reg] each, AItem::head_out
 * points into d_heads), one copy back; pdesc, the predictor's descriptors (PredItem), one copy per call; h_io, pinned only, per member
 * [x0_new (nx0) | u0_pred (nu0) | n_clipped], which the predictor's kernel reads and writes in place.  Capacities: bytes of desc and pdesc, doubles of
 * heads and io */
struct MpcSensBatch {
    long drained_at = 0;                /* as Kkt::drained_at, for the launches of the batched sensitivity */
    char *d_desc = nullptr, *h_desc = nullptr; size_t desc_cap = 0;
    double *d_heads = nullptr, *h_heads = nullptr; size_t heads_cap = 0;
    char *d_pdesc = nullptr, *h_pdesc = nullptr; size_t pdesc_cap = 0;
    double *h_io = nullptr; size_t io_cap = 0;
};

/* tqgpu_mpc_set_param_groups / tqgpu_mpc_adjoint_matrices*: the maps as given (a NULL map filled in), the tables built from them and from the kinds, the
 * root form and nx0 the device held then (sig; compared at every call, built and uploaded again where they moved), the sizes of the seven result regions
 * and of the partials in doubles per column of w, the result block on the device and pinned, the partials.  Batched route (the first member of a device's
 * group owns them): the descriptors (AMItem), uploaded with every call, and the result block of all members with its pinned twin */
struct MpcAdjMat {
    bool set = false;
    std::vector<int> hgroup, cgroup, sig, hdims, cdims;      /* hdims: nx, nu, pad, members per h-group; cdims: nx_c, nx_p, nu_p, members per c-group */
    int n_h = 0, n_c = 0, n_units = 0;
    int *d_tab = nullptr;
    AdjMat v{};
    size_t reg[8] = {}, part1 = 0, lds = 0;      /* reg[i]: where region i of [gH | gh | gA | gB | gb | gA0 | gS0] begins, reg[7] the total */
    double *d_res = nullptr, *h_res = nullptr, *d_part = nullptr; size_t res_cap = 0, part_cap = 0;
    char *d_desc = nullptr, *h_desc = nullptr; size_t desc_cap = 0;
    double *d_bres = nullptr, *h_bres = nullptr; size_t bres_cap = 0;
};
/* tqgpu_mpc_adjoint_bounds (bsum; built with the parameter groups) and tqgpu_mpc_adjoint_reference (rsum; built by tqgpu_mpc_set_tracking): the tables of
 * k_nodesum_part / k_nodesum_sum in one device block (members, set and chunk records), the set records once more on the host (which results have
 * more than one partial), the partials per column of w, the LDS window, and the call's own result block, its pinned twin and partials */
struct MpcNodeSum {
    int *d_tab = nullptr; NodeSum v{}; std::vector<int> set;
    size_t part1 = 0, lds = 0;
    double *d_res = nullptr, *h_res = nullptr, *d_part = nullptr; size_t res_cap = 0, part_cap = 0;
};
/* ---- the solution's way out and its check (tdunes_kkt.hpp): the solution in one piece, [x | u | lam | dlam | mu_x | mu_u], packed on the device (d) and
 * downloaded into pinned memory (h).  valid: h holds (or is about to hold, stream-ordered) the solution of the last solve; dev_only, with valid: the pack
 * is in d only (a certified tqgpu_mpc_step), tqgpu_get_solution downloads it.  The three transitions below are the only writers of the two flags. ---- */
struct Export {
    double *d = nullptr, *h = nullptr; size_t doubles = 0;
    bool ahead = false;                 /* tqgpu_set_export_ahead: the packing kernel and the download of the solution are enqueued right behind a single persistent launch */
    bool valid = false, dev_only = false;
    void invalidate() { valid = false; }                                   /* the device holds another point, or is about to: a solve begins, rows or the sharing change */
    void packed_on_device() { valid = true; dev_only = true; }             /* packed behind a certified step; no download yet */
    void packed_and_downloading() { valid = true; dev_only = false; }      /* the pack and its download are on the stream (an export ahead), or the download of a pack that was on the device only */
};
/* tqgpu_kkt_residual*: d, h, [six maxima | six nodes | pad | Nn x 6 table] on the device and pinned (setup_kkt, on first use); d_pt, h_pt, the point of
 * tqgpu_kkt_residual_at, [x | u | lam | mu_x | mu_u | mu_d], on the device and pinned (grows with sum_nc).
 * tqgpu_kkt_residual_batch, batched route (the first member of a device's group owns both): one descriptor per member, uploaded
 * with every call, and the members' heads in one block, downloaded in one copy */
struct Kkt {
    double *d = nullptr, *h = nullptr, *d_pt = nullptr, *h_pt = nullptr; size_t pt_cap = 0;
    KItem *d_items = nullptr, *h_items = nullptr; int items_cap = 0;
    KHead *d_heads = nullptr, *h_heads = nullptr; int heads_cap = 0;
    long drained_at = 0;                /* solve_no at which the batched route last knew this mirror's own stream to hold nothing of its solves */
};
/* ---- the two multi-device modes (tdunes_shard.hpp): the subtree-sharded mode (tqgpu_shard_*); rank, nranks and part_top are the sharded persistent launch's as well ---- */
struct SubtreeShard {
    int nranks = 1, rank = 0, part_top = -1;      /* part_top: highest partitioned tier */
    bool on = false;          /* subtree-sharded mode (nranks > 1, or ONE rank with a communicator: the same code path, used to exercise the RCCL transport on a one-GPU box) */
    int *d_gh_list = nullptr, *d_node_list = nullptr, *d_node_cnt_list = nullptr, *d_blk_list = nullptr;
    int gh_n = 0, gh_counted = 0, n_nodes = 0, n_nodes_counted = 0, n_blk_counted = 0;
    double *d_xerr = nullptr, *d_xs = nullptr;
    int bnd_b0 = 0, bnd_bn = 0, bnd_own0 = 0, bnd_ownn = 0;   /* element ranges of the boundary nodes' duals */
    void *slab = nullptr;
    void *comm = nullptr;     /* RCCL communicator (nullptr: single device or virtual ranks) */
};
/* ONE tree over several devices INSIDE the persistent launch (tqgpu_pshard_*): this rank's share of the workgroups */
struct PersistShard {
    bool on = false;
    bool sys = true;                /* the sharded launch polls its slab with system-scope loads (f_persist_sh<.., 1>); TREEQP_AMD_PSHARD_AGENT=1: agent scope, as on one device */
    bool fine = false;              /* the hand-over slab was re-allocated as fine-grained memory (tqgpu_pshard_init; TREEQP_AMD_PSHARD_COARSE=1 keeps plain hipMalloc memory) */
    int *wg_map = nullptr;          /* blockIdx.x -> workgroup id, this rank's workgroups (bottom tier first) */
    int G = 0;
    const ShardRow *row = nullptr;  /* the sharded kernels of this shape (SHARD_ROWS), looked up by tqgpu_pshard_init */
    void *ipc[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      /* peer slabs opened through IPC handles (closed by tqgpu_destroy) */
    unsigned long long *h_peers[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   /* slabs of all ranks (a mirror that is not sharded: its own, eight times) ... */
    unsigned long long **d_peers = nullptr;                                                               /* ... and the device copy of the table the kernel reads */
};
/* ---- what problem the mirror holds and which stage solver each node runs (tdunes_problem.hpp): StageKinds, GenRows, DenseSingle ---- */
/* the stage solvers selected (tqgpu_set_objective_mixed; tqgpu_set_objective_diag and tqgpu_set_problem return to clipping): dense, some nodes
 * use a dense stage solver (generic path only); box, some of them have box bounds (kind 2): the stage sweep is k_stage_box with lds_box bytes;
 * gen, some have general constraints as well (kind 3): k_stage_gen with lds_gen bytes; lds_dense: k_dense_init's */
struct StageKinds {
    bool dense = false, need_dense_init = false, box = false, gen = false;
    size_t lds_dense = 0, lds_box = 0, lds_gen = 0;
    std::vector<int> h_kind;     /* the kinds last set, as the device has them: a kind-3 node without rows is a kind-2 node */
    std::vector<int> h_kind_req; /* ... as the caller gave them */
    std::vector<double> h_bounds; /* the bounds last set by tqgpu_set_bounds (device layout: xmin | xmax | umin | umax); empty: unknown */
    double *d_Hd = nullptr; int *d_kind = nullptr;      /* writable aliases of Data.Hd, Data.kind */
    int kind(int k) const { return dense && !h_kind.empty() ? h_kind[(size_t)k] : 0; }      /* of node k; 0 (clipping) unless the mirror is dense */
    bool working_sets(size_t Nn) const { return dense && (box || gen) && h_kind.size() == Nn; }      /* the mirror has stored working sets (kinds 2, 3) */
};
/* general constraints (tqgpu_set_constraints): rows per node, their offsets and those of the blocks of Gt, host copies of dmin | dmax, the
 * device blocks and the record Data.gen points to */
struct GenRows {
    std::vector<int> nc, roff, goff;
    std::vector<double> h_drange; int sum_nc = 0;
    int *d_tab = nullptr;        /* Gen::nc, roff, goff */
    double *d_Gt = nullptr, *d_drange = nullptr, *d_mu = nullptr;
    unsigned long long *d_rmask = nullptr;     /* 4 Nn words: Gen::rmask (2 Nn), Gen::sides (2 Nn) */
    long *d_steps = nullptr;     /* Gen::steps_total (Nn longs), then Gen::steps_last (Nn ints) */
    bool hot = true;             /* stage_gen starts from the stored working sets (tqgpu_set_gen_hot_start) */
    Gen h_gen{};                 /* what d_gen holds: the views of the blocks above are taken from it */
    Gen *d_gen = nullptr;
    unsigned long long *row_sides(size_t Nn) const { return d_rmask + 3 * Nn; }      /* the second half of h_gen.sides: the sides of the rows */
};
/* the single-workgroup solve of a dense tree (g_persist_dense, opt-in): the caller's two choices, then the plan of plan_dense_single for the
 * kinds and rows last set */
struct DenseSingle {
    bool single = false;         /* tqgpu_set_dense_single_launch, TREEQP_AMD_DENSE_SINGLE_LAUNCH=1 */
    bool batch = false;          /* ... for the members of a batch: one launch of g_persist_dense_batch, a workgroup per tree (tqgpu_set_dense_batch_launch, TREEQP_AMD_DENSE_BATCH_LAUNCH=1); independent of single */
    bool ok = false;             /* the tree with its current kinds and rows fits */
    int stage_waves = 0, phase_waves = 0;      /* waves of the stage sweep (0: does not fit), of the sweeps over blocks (GPD_WAVES unless that many windows of gp.lds_wave doubles do not fit) */
    size_t win_stage = 0, win_region = 0, lds_total = 0;      /* doubles: a stage window, the window region; bytes of dynamic LDS of g_persist_dense */
    bool in_lds = false, const_in_lds = false, tab_in_lds = false;
};

/* ---- what a mirror keeps per route (Route; set up by the setup_* steps of tqgpu_create, used by the launch_* helpers and the solve), one record per route ---- */
/* The seven records below sit in one unnamed namespace.  The library's dynamic symbols are part of its contract, and a member function of a
 * record with a name of its own linkage joins them as a weak symbol as soon as the compiler emits it out of line (Timing's destructor did).  Whether
 * it does is the inliner's choice, so nothing but a comparison of `nm -D --defined-only` with the release before guards the records outside the
 * bracket (Owned's templates are in that list already and stay there). */
namespace {
/* the launch-per-phase kernels, wave-per-block (tdunes_device.hip) and workgroup-per-block (tdunes_wide.hpp): their LDS windows,
 * the tagged words of the fused sweeps and of the reductions that run as a sweep's tail, and how many iterations go out per read-back */
struct PerPhase {
    size_t lds_stage = 0, lds_hess = 0, lds_factor = 0, lds_forward = 0;
    bool wide = false;              /* larger blocks (16 < d <= 64): workgroup-per-block MFMA kernels (tdunes_wide.hpp) */
    bool wide_small = false;        /* ... taken by a tree of small blocks (d <= 16) too wide for the single-workgroup kernel */
    size_t lds_hess_w = 0, lds_factor_w = 0, lds_forward_w = 0;
    unsigned long long *fw_words = nullptr;   /* launch-per-phase path: the steps of a forward sweep as tagged words (k_forward_all_w), [sum_nx][2] */
    unsigned fw_epoch = 0;              /* tag of the last fused forward launch */
    bool fw_fused = true;               /* TREEQP_AMD_FWD=levels: one launch per level instead */
    unsigned long long *sch_words = nullptr;  /* launch-per-phase path: Schur records of a fused backward sweep as tagged words (k_factor_all_w), [Nn][sch_rs][2] */
    int sch_rs = 0;                     /* doubles per record: (max nx + 1)^2 */
    unsigned bw_epoch = 0;
    bool bw_fused = true;               /* TREEQP_AMD_BWD=levels: one launch per level instead */
    unsigned long long *fuse_red = nullptr;   /* small trees: partials of the reductions that run as the tail of a sweep (Fuse), [Nn][2] tagged words */
    int *fuse_cnt = nullptr;            /* ... and the counter of the workgroups that have posted theirs */
    unsigned fuse_epoch = 0;
    bool fuse_ok = false;
    std::vector<int> ls_pred;           /* trials per iteration of the previous solve: that many trial launches are enqueued behind an iteration's forward sweep (a trial beyond the accepted one is a no-op; a read-back per extra trial is 20 us) */
    int chunk = 4;            /* Newton iterations enqueued per status read-back */
};
/* three launches per Newton iteration for the wide-block class (tdunes_wide3.hpp): k_sg, k_hf_w, k_fwd3 */
struct Wide3 {
    bool ok = false;
    unsigned long long *xu = nullptr, *red = nullptr;
    int *cnt = nullptr;
    unsigned epoch = 0;
    size_t lds_hf_w = 0, lds_sgp = 0;
    int sgp_accs = 0;
    bool sgp = false;                   /* k_sgp (a workgroup per parent) instead of k_sg (a wave per node) */
    unsigned long long *d_pdw = nullptr; /* k_sgp mode 2: the blocks' parts of res' dlam as tagged words */
    bool merge = false;                 /* forward sweep and first trial in one launch (k_sgp mode 2) */
    int *d_anc = nullptr;               /* k_fwd3c: the path to the root of every block (tdunes_wide3.hpp); nullptr: the tree does not qualify */
    bool mirror = false;                /* this solve: the launches of k_sg / k_sgp post the control block to h_res (w3_mirror in tdunes_wide3.hpp) */
    bool tail_sg = false;               /* the last launch enqueued is one of them: its tag (wait) is what the host polls for */
    unsigned wait = 0;
    bool post_next = false;             /* the next launch of k_sg / k_sgp is the last of what the host enqueues before it reads the verdict: it posts */
    bool seen = false;                  /* the last read of the control block came through the result block */
};
/* the whole solve in one launch of one workgroup (tdunes_gpersist.hpp; the dense build's plan is DenseSingle) */
struct SingleWg {
    bool ok = false;                /* small tree of any shape: whole solve in one launch of one workgroup (tdunes_gpersist.hpp) */
    int use = 1;
    int *d_lvl_first = nullptr;
    size_t lds_wave = 0;            /* doubles of LDS per wave of g_persist */
    size_t lds_total = 0;           /* bytes of dynamic LDS of g_persist (windows + state mirror) */
    bool in_lds = false, const_in_lds = false, tab_in_lds = false, small16 = false, small8 = false;
    GItem *d_gitems = nullptr, *h_gitems = nullptr; int gitems_cap = 0;   /* batched single-workgroup launches (first mirror of a batch owns the array) */
};
/* fused path for uniform complete trees and multistage trees (tdunes_fast.hpp, tdunes_persist.hpp): the shape found by detect_fast /
 * detect_multistage and the tiers of the launches per tier */
struct Uniform {
    int fast = -1;            /* index into the instantiation table, -1: generic path only */
    const ShapeRow *row = nullptr;   /* that line's sizes and kernels (FAST_ROWS; MSTAGE_ROWS where mstage): set and cleared with `fast` */
    int fNX = 0, fNU = 0, fMD = 0;
    int n_tiers = 0;          /* tiers of block levels, index 0 = bottom */
    bool mstage = false;      /* multistage tree (branching for Nr stages, then chains): persistent kernel f_mpersist only */
    int ms_Nr = 0, ms_S = 0, ms_nB = 0;
    std::vector<int> tier_chain;
    std::vector<int> tier_l0, tier_l1, tier_grid;
    size_t lds_fast = 0, lds_fstage = 0;
    int use_fast = 1;         /* can be switched off (TREEQP_AMD_PATH=generic) */
    int use_fast_orig = 1;
    int *d_desc = nullptr;
};
/* the persistent single launch (tdunes_persist.hpp; setup_persist, launch_persist, launch_persist_batch): geometry, hand-over and sync slab,
 * packed constants, the launch number and the descriptors of a batch launch */
struct Persist {
    int use = 1;              /* whole Newton loop in one launch when every tier workgroup can be co-resident */
    int use_orig = 1, backoff = 0, n_timeouts = 0;   /* see solve_after_timeout */
    bool ok = false;
    bool one = false;                  /* the persistent launch of this tree takes the one-workgroup-per-CU build */
    PGeom geom{};
    PSync psync{};
    PConst pconst{};
    void *sync_slab = nullptr; size_t sync_bytes = 0;
    size_t sync_words_bytes = 0, lds = 0;
    unsigned launch_no = 0;         /* persistent launches so far (16 bits, never 0): tags of the hand-over words */
    void *pconst_slab = nullptr;    /* packed constants of the persistent path + its PDump */
    int *wg_map = nullptr;          /* blockIdx.x -> workgroup id (XCD-aware placement) */
    int co_capacity = 1;            /* workgroups of persistent launches that can be resident on the device together */
    double *pab = nullptr, *pcst = nullptr;
    bool need_pack = true;          /* QP data changed since the constants were packed */
    PItem *d_pitems = nullptr, *h_pitems = nullptr; int pitems_cap = 0;   /* batched persistent launches: one descriptor per tree (first mirror of a batch owns the array) */
    std::vector<unsigned long> pitems_key;                                /* the mirrors (by uid) the device copy of the array describes */
};
/* ---- device times on request (recorded by the solve, read by the log getters at the end of tdunes_device.hip) ---- */
struct Timing {
    std::vector<hipEvent_t> ring_ev0, ring_ev1;   /* events of the last solves (device times on request) */
    std::vector<char> ring_ok;                    /* the event pair of that ring slot was recorded by the solve that owns it */
    bool ev_timing = true;                        /* record a HIP event pair around every solve (tqgpu_set_event_timing) */
    std::vector<hipEvent_t> iter_ev;
    std::vector<double> iter_times;
    bool times_dirty = true;              /* iter_times / phase_times may hold times of an earlier (profiled) solve */
    /* profile level 3 (profiling.h:38-68): events around the phase groups of every iteration on the launch-per-level path:
     * [iteration][0..4] = start, gradient + termination test + dual Hessian done, factorisation + substitution done, line search done */
    std::vector<hipEvent_t> phase_ev;
    std::vector<double> phase_times;      /* [iteration][3]: build_dual, newton_direction, line_search (seconds) */
    double first_sweep_time = NAN;        /* phase S of iteration 0 (the later ones are the accepted trial sweeps of the line searches) */
    hipEvent_t sweep_ev0 = nullptr, sweep_ev1 = nullptr;
};
/* ---- what ties a mirror's stream to a batch launch on another mirror's (tqgpu_solve_batch; settle below) ---- */
struct BatchLinks {
    bool in_batch = false;             /* inside tqgpu_solve_batch: members launched one by one run side by side, two workgroups to a CU -- not with that build */
    bool stream_pending = false;                                          /* something was enqueued on `stream` without a synchronisation after it (asynchronous uploads, constant packing): a batch launch on ANOTHER stream waits for it first */
    hipStream_t batch_stream = nullptr;                                   /* member of a batch launch in flight: the stream that launch is on (the lead's) */
    hipStream_t settle_stream = nullptr;                                  /* member of a batch launch whose verdict is in but whose last workgroups may still write back:
                                                                           * the lead's stream, to be waited for before this mirror is touched through its own stream (settle) */
};
}  // namespace

struct tqgpu_solver {
    Owned mem;
    Switches sw{};
    int device = 0;
    int Nn = 0, Np = 0, Nh = 0;
    std::vector<int> nk, nx, nu, dad, stage, kid0, xoff, uoff, aoff, boff, pos, bdim, woff, utoff, lvl_first;
    int sum_nx = 0, sum_nu = 0, sum_lam = 0, sum_A = 0, sum_B = 0, sum_W = 0, sum_Ut = 0, nx0 = 0, nxmax = 0;
    Route route = Route::PER_PHASE;     /* of the last solve begun */
    PerPhase pp; Wide3 w3; SingleWg gp; Uniform uni; Persist persist;      /* one record per route (the setup_* steps, the launch_* helpers) */
    StageKinds sk; GenRows rows; DenseSingle gpd;      /* what problem the mirror holds and which stage solver each node runs (tdunes_problem.hpp) */
    std::vector<int> poff;
    void *slab = nullptr;
    size_t slab_bytes = 0;
    Tree T{};
    Data D{};
    double *d_mu_x = nullptr, *d_mu_u = nullptr;
    double *d_lam_init = nullptr;   /* starting point of every solve (tqgpu_set_lambda) */
    int n_cu = 0;
    /* writable aliases of the const inputs */
    double *A = nullptr, *B = nullptr, *b = nullptr, *Qd = nullptr, *Rd = nullptr, *q = nullptr, *r = nullptr;
    double *xmin = nullptr, *xmax = nullptr, *umin = nullptr, *umax = nullptr;
    HostRes *h_res = nullptr;    /* pinned; the persistent kernel writes it directly */
    Ctrl *h_ctrl = nullptr;      /* = &h_res->c */
    long solve_no = 0;
    Timing tm;                   /* event rings and the iteration and phase logs' times (tqgpu_get_iteration_log ..) */
    int *h_ls_log = nullptr;     /* pinned */
    int ls_log_cap = 0;
    hipStream_t stream = nullptr;
    int last_iter = 0;
    int last_ls_extra = 0;          /* the previous solve needed line-search trials beyond the first of an iteration */
    bool need_init = true;
    /* pinned host mirrors: the inputs in slab layout (compare-and-copy uploads of what changed, no synchronisation),
     * the solution in one piece */
    char *h_in = nullptr; size_t in_off0 = 0, in_bytes = 0; bool in_valid = false;
    double *h_lam = nullptr; bool lam_valid = false;
    Export out; Kkt kkt;                /* the packed solution and its export state; the buffers of the KKT check (tdunes_kkt.hpp) */
    MpcRoot mpc; MpcWarm warm; MpcShift shift; MpcBatchBuf mpcb; MpcTrack trk; MpcSens sens; MpcTan tan; MpcAdjBatch adjb; MpcSensBatch sensb; MpcAdjMat adjm; MpcNodeSum bsum, rsum;      /* the MPC family (tdunes_mpc.hpp; sens, adjb, sensb, adjm: tdunes_adjoint.hpp), one record per feature */
    int x_pad = 0, A_pad = 0; /* phantom root states of an x0-eliminated tree embedded in a uniform one (doubles in front of x-sized arrays / of A) */
    unsigned long uid = 0;                                                /* unique per mirror of this process (an address can come back) */
    BatchLinks links;               /* this mirror as a member of a batch launch (tqgpu_solve_batch) */
    bool strict_sum = false;        /* TREEQP_AMD_STRICT_SUM=1 (Data::strict) */
    SubtreeShard shard; PersistShard pshard;      /* the two multi-device modes (tdunes_shard.hpp) */
};

extern "C" const char *tqgpu_last_error(void) { return g_err.c_str(); }
/* A batch launch runs on its lead's stream; the other members' own streams are not ordered behind it.  Its end is waited for lazily:
 * a loop of batch solves on the same lead stays stream-ordered by itself and pays no synchronisation per step (10 - 15 us of a
 * 150 us step), anything else that touches a member comes through here first. */
/* (the lead may have been destroyed in the meantime -- tqgpu_destroy synchronises its stream first, so there is nothing left to wait
 * for, but the handle must not be used: the streams of live mirrors are kept in a set) */
static std::mutex g_streams_mu;
static std::set<hipStream_t> g_live_streams;
static int settle(tqgpu_solver *s) {
    if (s && s->links.settle_stream) {
        hipStream_t t = s->links.settle_stream;
        s->links.settle_stream = nullptr;
        bool live;
        { std::lock_guard<std::mutex> lk(g_streams_mu); live = g_live_streams.count(t) != 0; }
        if (t != s->stream && live) HIP_TRY(hipStreamSynchronize(t));
    }
    return TQGPU_OK;
}
#define SETTLE(s) do { int rc_ = settle(const_cast<tqgpu_solver *>(s)); if (rc_ != TQGPU_OK) return rc_; } while (0)
extern "C" const char *tqgpu_version(void) { return "treeqp_amd tdunes device path r3 (gfx950: persistent single launch, three-launch MFMA family for 16 < d <= 64, single-workgroup and launch-per-phase kernels; sharded persistent mode)"; }

extern "C" int tqgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

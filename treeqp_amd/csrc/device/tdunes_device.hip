/*
 * tdunes_device.hip -- MI355X (gfx950) device path of the tdunes hot path + its C-ABI.
 *
 * Replaces, as hand-written HIP kernels, the reference call sequences:
 *   k_stage   <- solve_stage_problems (dual_Newton_tree.c:218-330) + clipping solve_extended
 *                (dual_Newton_tree_clipping.c:188-227) fused with evaluate_dual_function
 *                (:823-918) + eval_dual_term (clipping.c:359-382) and the multiplier update of
 *                line_search (:964-968)
 *   k_grad    <- dual gradient loop of build_dual_problem (:519-539) + per-node norm partials
 *   k_check   <- calculate_error_in_residuals (:412-442) + termination test (:542-546)
 *   k_hess    <- dual Hessian loop (:551-615) with set_CmPnCmT / add_EPmE / add_CmPnCkT
 *                (clipping.c:264-355) as ONE C*P*C' product per parent block
 *   k_factor  <- backward sweep of calculate_delta_lambda (:668-752) with
 *                treeqp_dpotrf_l_with_reg_opts (dual_Newton_common.c:36-78): potrf, trsv_lnn and
 *                trsm_rltn done as one "tall" Cholesky of [W; resMod'; Ut], then dsyrk/dgemv Schur
 *                updates into the parent block
 *   k_forward <- forward sweep (:756-775) + partial of gradient_trans_times_direction (:808-820)
 *   k_ls_*    <- line_search control flow (:922-1019), decided on the device
 *
 * Design: one 64-lane wavefront owns one tree node (k_stage, k_grad) or one dual-Hessian block
 * (k_hess, k_factor, k_forward); the block lives in LDS while it is worked on; nodes/blocks of
 * one tree level form one grid.  All indices come from flat prefix-sum tables, so per-node
 * dimensions nx[k], nu[k], nk[k] are free (nx[0] = 0 after x0 elimination included).  The active
 * set bookkeeping of the reference (checkLastActiveSet) is not needed: every iteration rebuilds
 * every block, which yields bit-identical factors (DESIGN.md "checkLastActiveSet").
 *
 * Control flow lives in a device control block (struct Ctrl): every kernel first looks at it and
 * returns if its phase is not due, so the host may enqueue ahead without reading back.
 *
 * The kernels above are the launch-per-phase protocol (any tree); they and the host side of a solve (setup, launch helpers, solve, batch, logs)
 * are in this file, with what more than one kernel family uses (Tree .. rdlane).  What is in a header of its own:
 *   tdunes_fast.hpp / tdunes_persist.hpp   uniform and multistage trees: launches per tier; the whole solve as ONE launch, also dealt over several
 *                        devices (tqgpu_pshard_*)
 *   tdunes_wide.hpp / tdunes_wide3.hpp     dual blocks of 16 < d <= 64 rows: MFMA kernels, three launches per Newton iteration
 *   tdunes_gpersist.hpp  small trees of any shape: one workgroup per tree
 *   tdunes_sens.hpp      kernels of the sensitivities and adjoints of an MPC step
 *   tdunes_mirror.hpp    (host part, as all below) tqgpu_solver and its records: one per route (PerPhase, Wide3, SingleWg, Uniform, Persist), one per
 *                        feature family (Mpc*, Export, Kkt, SubtreeShard, PersistShard, StageKinds, GenRows, DenseSingle), Timing, BatchLinks; Owned, fail, settle
 *   tdunes_rows.hpp      the kernels of every instantiated (nx, nu, md) as rows of typed pointers, one array per table of tdunes_parts.hpp, and their lookups:
 *                        how detect_fast .. launch_persist_batch and tqgpu_pshard_init pick a shape's kernels (no switch on a shape in the host code)
 *   tdunes_problem.hpp   what problem a mirror holds and which stage solver each node runs: the setters and getters of the problem's data
 *   tdunes_kkt.hpp       solution export and the KKT check, kernels and entry points
 *   tdunes_mpc.hpp       the MPC family (tqgpu_mpc_*), kernels and entry points; MpcStats, MpcPre stay here with the solve
 *   tdunes_adjoint.hpp   the host side of a step's sensitivities and adjoints, the builder of a batched derivative group (DerivGroup); the plan and the driver the batched
 *                        after-solve calls share (refuse_members, plan_device_groups, order_behind_lead, run_device_groups) stay here
 *   tdunes_shard.hpp     the two multi-device modes (tqgpu_shard_*, tqgpu_pshard_*)
 */
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <set>
#include <string>
#include <vector>

#include "treeqp_amd.h"

#define WAVE 64
#include "tdunes_parts.hpp"

namespace tqd {

int fail(int code, const std::string &msg);      /* defined in the host part */



#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(TQGPU_ENODEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

/* ------------------------------------------------------------------------------------------ */
/* device-side tables                                                                         */
/* ------------------------------------------------------------------------------------------ */

struct Tree {            /* device pointers, passed by value */
    int Nn, Np, Nh, nx0;
    const int *dad, *nk, *kid0, *nx, *nu, *xoff, *uoff, *aoff, *boff, *pos, *bdim, *woff, *utoff;
    /* everything the workgroup-per-block kernels need to know about node k in ONE 128-byte record (a dependent
     * chain of table look-ups costs a global round trip, ~2.4 us, per hop):
     * [0] bdim [1] nx [2] nu [3] nk [4] kid0 [5] xoff [6] uoff [7] xoff[kid0] [8] woff [9] utoff [10] dad [11] pos
     * [12] bdim[dad] [13] woff[dad] [16 + 3u ..] nx, aoff, boff of child u < 4 */
    const int *desc;
};
#define DESC_INTS 32

struct Ctrl {
    int done;            /* all work finished (converged / max iterations / failure)        */
    int status;          /* return_t value                                                   */
    int iter;            /* completed Newton iterations                                      */
    int cur;             /* which lambda buffer holds the current point                      */
    int ls_pending;      /* line search wants another trial                                  */
    int ls_iter;         /* trial counter of the running line search                         */
    int ls_total;
    int ls_last;
    int restart_counter; /* work->lineSearchRestartCounter                                   */
    int n_reg;           /* blocks regularised (diagnostic)                                  */
    int pad0, pad1;
    double tau, tauPrev, fval0, fval, dot, err;
};

struct Data {            /* device pointers, passed by value */
    const double *A, *B, *b, *Qd, *Rd, *q, *r, *xmin, *xmax, *umin, *umax;
    double *Qinv, *Rinv;
    double *qmod, *rmod, *x, *u, *xUnc, *uUnc, *QinvCal, *RinvCal;
    /* unclipped solution of phase S of the iteration in progress: the first trial sweep of a line search saves it before it
     * overwrites xUnc / uUnc.  The reference's trial sweeps (stage_qp_clipping_solve, clipping.c:231-260) do not write xUnc,
     * so on a MAXIMUM_ITERATIONS exit export_mu (:386-399) pairs the x of the last trial with the xUnc of the last phase S. */
    double *xUncS, *uUncS;
    double *lam0, *lam1, *dlam, *res, *resMod;
    double *W, *CholW, *invd, *Ut, *CholUt;
    double *fval, *part_err, *part_dot;
    double *Sbuf, *ybuf;     /* fused path: Schur hand-off records across tiers; backward solution L^-1 resMod */
    unsigned long long *stamps;   /* diagnostic time stamps (written only when Opts.stamps != 0; never read by kernels) */
    Ctrl *ctrl;
    int *ls_log;
    int ls_log_cap;
    /* dense unconstrained stage solver (generic path only; dual_Newton_tree_qpoases.c restricted to no bounds):
     * per node the stage Hessian H = [Q S'; S R] ((nx+nu)^2, column major) and its inverse P = H^-1 */
    int strict;               /* TREEQP_AMD_STRICT_SUM=1: sums that feed decisions are taken in the reference's order (node by node, block by block), see strict_* below */
    int dense;                /* some nodes use the dense unconstrained stage solver */
    const int *kind;          /* [Nn] per node: 0 clipping, 1 dense unconstrained, 2 dense with box bounds (read only when dense != 0) */
    const double *Hd;
    double *Pd;
    const int *poff;          /* [Nn+1] offsets of the (nx+nu)^2 blocks */
    /* dense nodes with box bounds (kind 2, stage_box): [0, Nn) the working set of node k (bit i: entry i of [x | u] sits on a
     * bound), kept across sweeps and solves as the hot start; [Nn, 2 Nn) the working set that P_k was last built for */
    unsigned long long *bmask;
    int xpad;                 /* phantom root states of an x0-eliminated tree embedded in a uniform one: unbounded in stage_box */
    const struct Gen *gen;    /* dense nodes with box bounds and general constraints (kind 3, stage_gen); nullptr until tqgpu_set_constraints */
};

/* general constraints dmin <= G z <= dmax of the kind-3 nodes, G = [C | D] (tqgpu_set_constraints): a record in device memory, so that
 * Data grows by one pointer */
struct Gen {
    const int *nc;            /* [Nn] rows of node k */
    const int *roff;          /* [Nn + 1] offsets of the rows (dmin, dmax, mu) */
    const int *goff;          /* [Nn + 1] offsets of the blocks of Gt */
    const double *Gt;         /* per node: row r of G at Gt[r nz .. r nz + nz) (phantom root states included, zero) */
    const double *dmin, *dmax;
    double *mu;               /* row multipliers of the last stage solve, with the sign of qp_out->mu_d; 0 off the working set */
    unsigned long long *rmask;   /* [0, Nn) rows in the final working set of node k; [Nn, 2 Nn) the rows P_k was last built for */
    /* the hot start of stage_gen: with bmask[k] and rmask[k] the sides of the final working set (bit set = upper side), [0, Nn) of the
     * bounds, [Nn, 2 Nn) of the rows; hot = 0: every stage solve starts cold (tqgpu_set_gen_hot_start) */
    unsigned long long *sides;
    int hot;
    int *steps_last;             /* [Nn] active-set steps of node k in the last stage sweep, [Nn] their sum over the last solve (tqgpu_get_stage_steps) */
    long *steps_total;
};

struct Opts {
    int maxIter, termCondition, regType, lsMaxIter, lsRestartTrigger, stamps;
    int reuse;               /* checkLastActiveSet: keep the factors of workgroups whose active set did not change (persistent path) */
    double tol, regTol, regValue, gamma, beta;
};

/* Tagged words: what crosses workgroups INSIDE a launch.  A double travels as two 64-bit relaxed agent-scope atomic stores,
 * each (tag << 32) | 32-bit half; the consumer polls the payload itself until every word carries the tag it expects (see
 * tdunes_persist.hpp).  Relaxed agent-scope accesses go to the memory side, so nothing depends on one XCD's L2 seeing another's. */
#ifndef TQ_WIDE_NAP
#define TQ_WIDE_NAP 1        /* s_sleep between two looks of a wait inside a fused sweep (x 64 cycles): 1 / 2 / 4 give 0.94 / 0.97 / 0.99 ms for one C5-class tree, no difference on C4; 16 and 32 are slower on both */
#endif
#define RLX __ATOMIC_RELAXED
#define AGENT __HIP_MEMORY_SCOPE_AGENT
typedef unsigned long long u64;
__device__ __forceinline__ void st_tag(u64 *p, double v, unsigned tag) {
    const u64 t = (u64)tag << 32;
    __hip_atomic_store(p, t | (unsigned)__double2loint(v), RLX, AGENT);
    __hip_atomic_store(p + 1, t | (unsigned)__double2hiint(v), RLX, AGENT);
}
/* TQ_LD_SCOPE: the scope of the POLLS of hand-over words.  Agent scope everywhere but in the part that holds the sharded persistent kernel
 * (tdunes_parts.hpp, treeqp_amd/build.py): there the slab is written by peer devices over xGMI and the polls are system-scope loads. */
#ifndef TQ_LD_SCOPE
#define TQ_LD_SCOPE __HIP_MEMORY_SCOPE_AGENT
#endif
__device__ __forceinline__ double ld_tag(const u64 *p, unsigned tag, bool &ok) {
    const u64 a = __hip_atomic_load(p, RLX, TQ_LD_SCOPE), b = __hip_atomic_load(p + 1, RLX, TQ_LD_SCOPE);
    ok = ok && (unsigned)(a >> 32) == tag && (unsigned)(b >> 32) == tag;
    return __hiloint2double((int)(unsigned)b, (int)(unsigned)a);
}
/* one tagged double, polled until it is there; gives up after 0.5 s (dead = true, value 0) */
__device__ __forceinline__ double wait_tag(const u64 *p, unsigned tag, bool &dead) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        bool ok = true;
        const double v = ld_tag(p, tag, ok);
        if (ok) return v;
        if (dead || wall_clock64() - t0 > 50000000ull) { dead = true; return 0.0; }      /* 100 MHz clock */
        __builtin_amdgcn_s_sleep(TQ_WIDE_NAP);
    }
}

/* Phase guards.  The host enqueues kernels ahead of the device's decisions and tags every launch
 * with the Newton iteration `h` (and line-search trial `t`) it belongs to; a kernel whose tag does
 * not match the device state is a no-op.  This keeps the host out of the loop: it only reads the
 * control block once per enqueued chunk. */
__device__ __forceinline__ bool phase_main(const Ctrl *c, int h) { return !c->done && c->iter == h && !c->ls_pending; }
__device__ __forceinline__ bool phase_trial(const Ctrl *c, int h, int t) { return !c->done && c->iter == h && c->ls_pending && c->ls_iter == t; }

/* Cross-lane sums without LDS round trips (all 64 lanes must be active):
 *   dpp_mov<row_ror:n>  rotate inside each row of 16 lanes (one VALU op per 32-bit half),
 *   v_permlane16/32_swap (gfx950) fold the rows.  Every lane ends with the full sum. */
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_mov<0x128>(v); v += dpp_mov<0x124>(v); v += dpp_mov<0x122>(v); v += dpp_mov<0x121>(v);
    return v;
}
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, dpp_mov<0x128>(v)); v = fmax(v, dpp_mov<0x124>(v)); v = fmax(v, dpp_mov<0x122>(v)); v = fmax(v, dpp_mov<0x121>(v));
    return v;
}
/* value of lane l combined with lanes l ^ 16, l ^ 32, l ^ 48 */
template <bool IS_MAX = false>
__device__ __forceinline__ double rows_fold(double v) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double x0 = __hiloint2double((int)b[0], (int)a[0]), x1 = __hiloint2double((int)b[1], (int)a[1]);
    const double x = IS_MAX ? fmax(x0, x1) : x0 + x1;
    const unsigned xl = (unsigned)__double2loint(x), xh = (unsigned)__double2hiint(x);
    auto c = __builtin_amdgcn_permlane32_swap(xl, xl, false, false);
    auto d = __builtin_amdgcn_permlane32_swap(xh, xh, false, false);
    const double y0 = __hiloint2double((int)d[0], (int)c[0]), y1 = __hiloint2double((int)d[1], (int)c[1]);
    return IS_MAX ? fmax(y0, y1) : y0 + y1;
}
__device__ __forceinline__ double wsum(double v) { return rows_fold<false>(row16_sum(v)); }
/* Maxima that feed the termination test must PROPAGATE a NaN (the reference's MAX(error, NaN) is NaN, `error < tol` is then
 * false and the line search ends the solve with NOT_DESCENT_DIRECTION, dual_Newton_tree.c:412-442, :949); fmax / v_max_f64
 * return the other operand.  nanmax: NaN if either operand is.  wmax: the fast v_max tree, then NaN if any lane's input was. */
__device__ __forceinline__ double nanmax(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double wmax(double v) {
    const double r = rows_fold<true>(row16_max(v));
    return __builtin_amdgcn_ballot_w64(v != v) ? __builtin_nan("") : r;
}

/* historical names, used by the generic kernels: same fixed-order reductions (a ds_bpermute butterfly cost
 * ~1.4 k cycles per call, five of them per node in the stage sweep) */
__device__ __forceinline__ double wave_sum(double v) { return wsum(v); }
__device__ __forceinline__ double wave_max(double v) { return wmax(v); }

/* The generic kernels work one wavefront per node / block on a private LDS window.  Their bodies are
 * device functions so that the same code runs (a) as one launch per phase and tree level, one wave per
 * workgroup, and (b) inside the single-workgroup persistent kernel g_persist, many waves side by side.
 * Inside a body the only synchronisation needed is among the lanes of ONE wave (they run in lockstep;
 * LDS operations of a wave complete in order), i.e. a compiler-level fence. */
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

/* ------------------------------------------------------------------------------------------ */
/* k_init: Qinv = 1/Qd, Rinv = 1/Rd  (stage_qp_clipping_init, clipping.c:163-170)             */
/* ------------------------------------------------------------------------------------------ */
#if TQ_HAS(TQP_HOST)
__global__ void k_init(int n_x, int n_u, Data D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_x) D.Qinv[i] = 1.0 / D.Qd[i];
    if (i < n_u) D.Rinv[i] = 1.0 / D.Rd[i];
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* k_dense_init: one wave per node: P = H^-1 through the Cholesky factor of H (stage_qp_qpoases */
/* restricted to unconstrained nodes, dual_Newton_tree_qpoases.c:153-217: the stage solution is */
/* z = H^-1 h and the elimination matrix is P = H^-1).  H in LDS, column by column; then lane j  */
/* solves L L' p_j = e_j.                                                                       */
/* ------------------------------------------------------------------------------------------ */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_dense_init(Tree T, Data D) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int nz = T.nx[k] + T.nu[k];
    if (nz == 0 || !D.kind[k]) return;
    if (D.kind[k] >= 2 && lane == 0) D.bmask[T.Nn + k] = 0ull;      /* box nodes: P below is the one of the empty working set */
    if (D.kind[k] == 3 && lane == 0) {                              /* and stage_gen starts cold after an upload of H or of C, D */
        D.gen->rmask[T.Nn + k] = 0ull;
        D.bmask[k] = 0ull; D.gen->rmask[k] = 0ull; D.gen->sides[k] = 0ull; D.gen->sides[T.Nn + k] = 0ull;
    }
    const double *H = D.Hd + D.poff[k];
    double *P = D.Pd + D.poff[k];
    double *Lm = lds;                      /* nz x nz, ld = nz */
    double *dinv = lds + (size_t)nz * nz;  /* nz */
    for (int e = lane; e < nz * nz; e += WAVE) Lm[e] = H[e];
    __syncthreads();
    for (int j = 0; j < nz; j++) {
        for (int i = j + lane; i < nz; i += WAVE) {
            double sacc = Lm[i + (size_t)j * nz];
            for (int c = 0; c < j; c++) sacc = fma(-Lm[i + (size_t)c * nz], Lm[j + (size_t)c * nz], sacc);
            Lm[i + (size_t)j * nz] = sacc;
        }
        __syncthreads();
        const double cjj = Lm[j + (size_t)j * nz];
        const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;
        for (int i = j + lane; i < nz; i += WAVE) Lm[i + (size_t)j * nz] *= finv;
        if (lane == 0) dinv[j] = finv;
        __syncthreads();
    }
    /* column j of P: forward then backward substitution on e_j (solution kept in global memory) */
    for (int j = lane; j < nz; j += WAVE) {
        double *pj = P + (size_t)j * nz;
        for (int i = 0; i < nz; i++) {
            double v = (i == j) ? 1.0 : 0.0;
            for (int c = 0; c < i; c++) v = fma(-Lm[i + (size_t)c * nz], pj[c], v);
            pj[i] = v * dinv[i];
        }
        for (int i = nz - 1; i >= 0; i--) {
            double v = pj[i];
            for (int c = i + 1; c < nz; c++) v = fma(-Lm[c + (size_t)i * nz], pj[c], v);
            pj[i] = v * dinv[i];
        }
    }
}
#endif

/* acc + sum_{i < n} a[i * sa] * b[i * sb], terms added in ascending order (the reference's order), but the loads go out DOT_BATCH
 * AT A TIME: a runtime-bounded `for (i) acc = fma(a[i], b[i], acc)` makes one memory round trip per trip of the loop (the
 * compiler does not move loads across the back edge), which is what the node sweeps of wider nodes spent their time on
 * (k_stage / k_grad at nx = 20, nu = 10: 15.6 / 13.3 us per launch).  Clamped addresses, masked use: nothing diverges. */
#ifndef DOT_BATCH
#define DOT_BATCH 8       /* loads in flight per lane and batch (16 and 24 measured slower inside the single-workgroup kernel: registers).
                             Also tried, none faster: 24 in flight in the standalone sweeps at nx = 20, the node's dimensions from its one
                             128-byte record instead of the index tables, the children's [A | B] fetched coalesced into LDS and read back
                             with typed LDS pointers, the staging loops of the block bodies batched the same way (slower).  k_stage /
                             k_grad at nx = 20 stream 16 MB in 12 us behind a ~4.5 us launch floor. */
#endif
__device__ __forceinline__ double dot_batched(const double *a, int sa, const double *b, int sb, int n, double acc, bool batch) {
    if (!batch) {                                            /* operands in LDS (g_persist with its state mirrored): the plain loop is the shorter program */
        for (int i = 0; i < n; i++) acc = fma(a[(size_t)i * sa], b[(size_t)i * sb], acc);
        return acc;
    }
    for (int i0 = 0; i0 < n; i0 += DOT_BATCH) {
        double va[DOT_BATCH], vb[DOT_BATCH];
#pragma unroll
        for (int m = 0; m < DOT_BATCH; m++) { const int i = i0 + m < n ? i0 + m : 0; va[m] = a[(size_t)i * sa]; vb[m] = b[(size_t)i * sb]; }
        asm volatile("" ::: "memory");                       /* the batch stays a batch (see LOADS_DONE in tdunes_wide.hpp) */
#pragma unroll
        for (int m = 0; m < DOT_BATCH; m++) { const double t = fma(va[m], vb[m], acc); acc = i0 + m < n ? t : acc; }
    }
    return acc;
}

/* ------------------------------------------------------------------------------------------ */
/* k_stage: one wave per node.  mode 0: evaluate at lam[cur] (first sweep of a solve);         */
/* mode 1: line-search trial, lam_next = lam_cur + (tau - tauPrev) * dlam, evaluate there.     */
/* Produces qmod,rmod,x,u,xUnc,uUnc,QinvCal,RinvCal and the node's dual-function term.         */
/* ------------------------------------------------------------------------------------------ */
/* xu != nullptr (k_sg): x, u of a PARENT node are also posted as tagged words -- entry j of x at xu[2 (xoff + j)], of u at
 * xu[2 (sum_nx + uoff + j)] -- for the children's gradient in the same launch */
/* Cl != nullptr (k_sgp): the children's [A | B], rows stacked child after child, column major with leading dimension ldcl, are in LDS */
/* value of lane l (l uniform across the wave) to every lane */
__device__ __forceinline__ double rdlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

/* ------------------------------------------------------------------------------------------ */
/* stage_box: the stage QP of a dense node with box bounds (kind 2) -- the qpOASES QProblemB   */
/* solve of the reference (dual_Newton_tree_qpoases.c:312-358) and its elimination matrix      */
/* (:153-210), as a primal active-set method on the bounds in one wave:                        */
/*   z = argmin 1/2 z'Hz - hmod'z  s.t.  lb <= z <= ub,   P = Z (Z'HZ)^-1 Z'                     */
/* Lane i owns entry i of z = [x | u] (nz <= 64).  H and the Cholesky factor of the working-set */
/* matrix M (H with the rows and columns of fixed entries replaced by those of the identity:    */
/* its factor is chol(H_FF) in place) live in LDS.  Hot start: the previous z projected onto   */
/* the box, with the stored working set restricted to the bounds that point meets.  Each step  */
/* solves M zn = [hmod_F - H_FA z_A ; z_A]; if zn leaves the box (or lands on a bound) the     */
/* step stops at the first blocking bound (lowest index on ties), which joins the working set; */
/* entries with equal bounds are always in it; otherwise the fixed                             */
/* entry of lowest index whose multiplier has the wrong sign is released, or the solve is done. */
/* Every decision is a wave-uniform ballot.  The returned z is the last zn, i.e. a function of  */
/* the final working set alone (not of the path).  Multipliers: xUnc / uUnc keep hmod, from    */
/* which k_export_box forms mu = hmod - Hz.  P is rebuilt only when the working set differs     */
/* from the one P was built for.                                                                */
/* ------------------------------------------------------------------------------------------ */
#define BOX_MAX_STEPS(nz) (4 * (nz) + 8)
__device__ void stage_box(const Tree &T, const Data &D, int k, int lane, double *lds, const double *hm, const double *lk, int ko, bool save_s) {
    const int nxk = T.nx[k], nuk = T.nu[k], xo = T.xoff[k], uo = T.uoff[k], d = T.bdim[k];
    const int nz = nxk + nuk;
    double *dv = lds;                      /* nz: 1 / L_ii */
    double *Hs = dv + nz;                  /* nz x nz, column major: H_k, later the columns of P */
    double *Ls = Hs + (size_t)nz * nz;     /* nz x nz, column major: Cholesky factor of M */
    const double *Hg = D.Hd + D.poff[k];
    for (int e = lane; e < nz * nz; e += WAVE) Hs[e] = Hg[e];

    const bool own = lane < nz, isx = lane < nxk;
    const int j0 = isx ? lane : lane - nxk;
    const double inf = __builtin_inf();
    double lo = -inf, hi = inf, h = 0.0, z = 0.0;
    if (own) {
        const bool phantom = isx && k == 0 && lane < D.xpad;
        if (!phantom) { lo = isx ? D.xmin[xo + j0] : D.umin[uo + j0]; hi = isx ? D.xmax[xo + j0] : D.umax[uo + j0]; }
        h = hm[lane];
        z = isx ? D.x[xo + j0] : D.u[uo + j0];
        if (z != z) z = 0.0;
        z = fmin(fmax(z, lo), hi);
    }
    const u64 bit = 1ull << lane;
    bool fixed = own && (lo == hi || ((D.bmask[k] & bit) && (z == lo || z == hi)));      /* equal bounds: always in the working set */
    u64 m = __builtin_amdgcn_ballot_w64(fixed);
    WSYNC();

    bool ok = false;
    double hz = 0.0, habs = 0.0;           /* (H z)_i and sum_j |H_ij z_j| at the final z */
    for (int step = 0; step < BOX_MAX_STEPS(nz); step++) {
        WSYNC();
        /* M and the right-hand side of the working set m */
        double r = h;
        for (int j = 0; j < nz; j++) {
            const bool fj = (m >> j) & 1ull;
            if (own) Ls[lane + (size_t)j * nz] = (fixed || fj) ? (lane == j ? 1.0 : 0.0) : Hs[lane + (size_t)j * nz];
            if (fj) { const double zj = rdlane(z, j); r = fma(-Hs[lane < nz ? lane + (size_t)j * nz : 0], zj, r); }
        }
        if (fixed) r = z;
        WSYNC();
        /* Cholesky factor of M, left looking, lane i = row i */
        bool pd = true;
        for (int j = 0; j < nz; j++) {
            if (own && lane >= j) {
                double sacc = Ls[lane + (size_t)j * nz];
                for (int c = 0; c < j; c++) sacc = fma(-Ls[lane + (size_t)c * nz], Ls[j + (size_t)c * nz], sacc);
                Ls[lane + (size_t)j * nz] = sacc;
            }
            WSYNC();
            const double cjj = Ls[j + (size_t)j * nz];
            pd = pd && cjj > 0.0;
            const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;
            if (own && lane >= j) Ls[lane + (size_t)j * nz] *= finv;
            if (lane == 0) dv[j] = finv;
            WSYNC();
        }
        if (!pd) break;                                        /* H_FF not positive definite: the stage QP has no solution here */
        /* L L' zn = r */
        for (int c = 0; c < nz; c++) {
            const double yc = rdlane(r, c) * dv[c];
            if (lane == c) r = yc;
            else if (own && lane > c) r = fma(-Ls[lane + (size_t)c * nz], yc, r);
        }
        for (int c = nz - 1; c >= 0; c--) {
            const double xc = rdlane(r, c) * dv[c];
            if (lane == c) r = xc;
            else if (lane < c) r = fma(-Ls[c + (size_t)lane * nz], xc, r);
        }
        const double zn = fixed ? z : (own ? r : 0.0);
        /* the first bound the segment z -> zn meets; a free solution ON a bound fixes it too (inclusive, as clipping's
         * `unc >= ub` / `unc <= lb`: on a diagonal node the working set is the clipping's active set, and so is P) */
        const bool blk = own && !fixed && (zn <= lo || zn >= hi);
        double a = 1.0;
        if (blk) a = zn == z ? 0.0 : fmin(fmax((zn <= lo ? lo - z : hi - z) / (zn - z), 0.0), 1.0);
        const u64 bm = __builtin_amdgcn_ballot_w64(blk);
        if (bm) {
            const double amin = -wmax(-a);
            const u64 at = __builtin_amdgcn_ballot_w64(blk && a == amin);
            const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(at));
            if (own && !fixed) z = fmin(fmax(fma(amin, zn - z, z), lo), hi);
            if (lane == i) { z = zn <= lo ? lo : hi; fixed = true; }
            m |= 1ull << i;
            continue;
        }
        z = zn;
        /* multipliers of the fixed entries: g = H z - hmod >= 0 on a lower bound, <= 0 on an upper one */
        hz = 0.0; habs = 0.0;
        for (int j = 0; j < nz; j++) {
            const double zj = rdlane(z, j), hij = Hs[lane < nz ? lane + (size_t)j * nz : 0];
            hz = fma(hij, zj, hz);
            habs = fma(fabs(hij), fabs(zj), habs);
        }
        const double g = hz - h, tol = 64.0 * __DBL_EPSILON__ * (habs + fabs(h));
        const bool wrong = fixed && lo < hi && ((z == lo && g < -tol) || (z == hi && g > tol));
        const u64 wm = __builtin_amdgcn_ballot_w64(wrong);
        if (!wm) { ok = true; break; }
        const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(wm));
        if (lane == i) fixed = false;
        m &= ~(1ull << i);
    }
    if (!ok && lane == 0) { D.ctrl->status = 4; D.ctrl->done = 1; }      /* TREEQP_DN_STAGE_QP_SOLVE_FAILED */
    if (lane == 0) D.bmask[k] = m;
    /* the sides of the final set, where the tree has rows: a shift may hand this node's set to a node of kind 3, which reads them (bit
     * set = upper bound; equal bounds count as lower, as stage_gen's).  Without them the word kept whatever was stored there last. */
    const u64 up = __builtin_amdgcn_ballot_w64(fixed && lo < hi && z == hi);
    if (lane == 0 && D.gen) D.gen->sides[k] = up & m;
    if (own) {
        if (isx) { if (save_s) D.xUncS[xo + j0] = D.xUnc[xo + j0]; D.x[xo + j0] = z; D.xUnc[xo + j0] = h; }
        else { if (save_s) D.uUncS[uo + j0] = D.uUnc[uo + j0]; D.u[uo + j0] = z; D.uUnc[uo + j0] = h; }
    }
    /* dual term -1/2 z'Hz + hmod'z - cmod, as the unconstrained dense branch takes it */
    double p_quad = own ? z * hz : 0.0, p_lin = own ? h * z : 0.0, p_cd = 0.0;
    for (int t = lane; t < d; t += WAVE) p_cd = fma(D.b[ko + t], lk[t], p_cd);
    p_quad = wave_sum(p_quad); p_lin = wave_sum(p_lin); p_cd = wave_sum(p_cd);
    if (lane == 0) D.fval[k] = -0.5 * p_quad - p_cd + p_lin;
    if (!ok || m == D.bmask[T.Nn + k]) return;
    /* P = M^-1 with the rows and columns of the working set zeroed: lane j solves L L' p_j = e_j into column j of Hs */
    WSYNC();
    if (own) {
        double *col = Hs + (size_t)lane * nz;
        for (int i = 0; i < nz; i++) {
            double v = (i == lane && !fixed) ? 1.0 : 0.0;
            for (int c = 0; c < i; c++) v = fma(-Ls[i + (size_t)c * nz], col[c], v);
            col[i] = v * dv[i];
        }
        for (int i = nz - 1; i >= 0; i--) {
            double v = col[i];
            for (int c = i + 1; c < nz; c++) v = fma(-Ls[c + (size_t)i * nz], col[c], v);
            col[i] = v * dv[i];
        }
    }
    WSYNC();
    double *P = D.Pd + D.poff[k];
    for (int e = lane; e < nz * nz; e += WAVE) P[e] = Hs[e];
    if (lane == 0) D.bmask[T.Nn + k] = m;
}


/* ------------------------------------------------------------------------------------------ */
/* stage_gen: the stage QP of a dense node with box bounds and general constraints (kind 3) -- */
/* the qpOASES QProblem solve of the reference (dual_Newton_tree_qpoases.c:226-300, 312-358)   */
/* as a dual active-set method (Goldfarb and Idnani) in one wave:                              */
/*   z = argmin 1/2 z'Hz - hmod'z  s.t.  lb <= z <= ub,  dmin <= G z <= dmax,  G = [C | D]      */
/* Lane i owns entry i of z (nz <= 64) and row i of G (nc <= 64).  The working set is a set of */
/* bounds (fixed entries, as in stage_box: M is H with the rows and columns of fixed entries   */
/* replaced by those of the identity, so fixed entries stay exactly on their bound) and a set  */
/* of rows W; Y = L^-1 G_W' on the free entries (L the factor of M) and S = Y'Y, with the rows */
/* and columns of the rows outside W replaced by those of the identity, are rebuilt and        */
/* factorised at every step; M and L only when the set of fixed entries differs from the one L */
/* was built for.  The method needs no feasible point.  Per step: the most violated constraint */
/* p (lowest index on ties, bounds before rows), the primal direction dz = P n_p and the dual   */
/* direction r, the step min(t_dual, t_full); a partial step drops the blocking member and     */
/* keeps p, a full step adds p.  n_p'P n_p <= 64 eps n_p'M^-1 n_p means p depends on the        */
/* working set: only the dual step is taken.  Every decision is a wave-uniform ballot.         */
/* Start.  Cold (Gen::hot == 0): the minimiser over the equalities (entries with lb == ub,     */
/* rows with dmin == dmax).  Hot (the default): the working set and sides the node's last      */
/* stage solve ended with (bmask[k], rmask[k], Gen::sides, kept across sweeps and solves),     */
/* made safe against the current data -- lanes beyond nz / nc and members whose bound on the   */
/* stored side is infinite leave, equalities come in -- then dual-feasibility rounds: the      */
/* minimiser on the set, and every member that is no equality and whose multiplier (sg om for  */
/* a bound, sr nu_r for a row) is negative beyond 64 eps (sum of |terms|) leaves, all of them  */
/* in one round, until none does (the set only shrinks).  What remains -- z minimises on W,    */
/* multipliers >= 0, W independent -- is a state of the loop above, which goes on from there.  */
/* A hot pass that ends in any other way than with a solution (a non-positive pivot of M or S  */
/* on the stored set, i.e. a dependent one; the step cap of 4 (nz + nc) + 8, which the rounds  */
/* count against; no step possible) is followed by one cold pass, exactly the cold solve; only */
/* its failure is status 4 (an infeasible stage QP still ends there).  The returned z and row  */
/* multipliers are the solution of the final working set's system alone, not of the path: hot  */
/* and cold solves that end on the same set and sides (they do where the solution is strictly  */
/* complementary) agree bit for bit, and so do repeated solves.  k_dense_init empties the      */
/* stored set when H or C, D are uploaded.  P = M^-1 - M^-1 G_W' S^-1 G_W M^-1 (fixed rows and */
/* columns zero) is rebuilt only when either mask differs from the one it was built for.       */
/* Gen::steps_last / steps_total count the passes of the loop (one factorisation of S each).   */
/* ------------------------------------------------------------------------------------------ */
#define GEN_MAX_STEPS(nz, nc) (4 * ((nz) + (nc)) + 8)
__device__ void stage_gen(const Tree &T, const Data &D, int k, int lane, double *lds, const double *hm, const double *lk, int ko, bool save_s) {
    const Gen &Gn = *D.gen;
    const int nxk = T.nx[k], nuk = T.nu[k], xo = T.xoff[k], uo = T.uoff[k], d = T.bdim[k];
    const int nz = nxk + nuk, nc = Gn.nc[k], ro = Gn.roff[k];
    double *dv = lds;                      /* nz: 1 / L_ii */
    double *sv = dv + nz;                  /* nc: 1 / (factor of S)_ii */
    double *Hs = sv + nc;                  /* nz x nz, column major: H_k */
    double *Ls = Hs + (size_t)nz * nz;     /* nz x nz: Cholesky factor of M */
    double *Ys = Ls + (size_t)nz * nz;     /* nz x nc: Y, the columns of the rows in W */
    double *Ss = Ys + (size_t)nz * nc;     /* nc x nc: S and its factor */
    const double *Hg = D.Hd + D.poff[k];
    const double *Gt = Gn.Gt + Gn.goff[k];
    for (int e = lane; e < nz * nz; e += WAVE) Hs[e] = Hg[e];

    const bool own = lane < nz, isx = lane < nxk, row = lane < nc;
    const int j0 = isx ? lane : lane - nxk;
    const int zl = own ? lane : 0, rl = row ? lane : 0;      /* clamped indices for masked reads */
    const double inf = __builtin_inf(), eps64 = 64.0 * __DBL_EPSILON__;
    double lo = -inf, hi = inf, h = 0.0, z = 0.0, dlo = -inf, dhi = inf;
    if (own) {
        const bool phantom = isx && k == 0 && lane < D.xpad;
        if (!phantom) { lo = isx ? D.xmin[xo + j0] : D.umin[uo + j0]; hi = isx ? D.xmax[xo + j0] : D.umax[uo + j0]; }
        h = hm[lane];
    }
    if (row) { dlo = Gn.dmin[ro + lane]; dhi = Gn.dmax[ro + lane]; }
    /* the working set: fixed / sg (+1 on the lower bound, -1 on the upper one) per entry, inw / sr per row; nu_r is the multiplier
     * of row r in  H z - hmod = G_W' nu + (multipliers of the fixed entries) */
    bool fixed = false, inw = false;
    double sg = 1.0, sr = 1.0, nur = 0.0;
    u64 mb = 0ull, mr = 0ull;
    WSYNC();

    /* L v = w and L' v = w, entry i of the vectors in lane i; the same with the factor of S (row space) */
    auto fwdL = [&](double v) { for (int c = 0; c < nz; c++) { const double yc = rdlane(v, c) * dv[c]; if (lane == c) v = yc; else if (own && lane > c) v = fma(-Ls[lane + (size_t)c * nz], yc, v); } return v; };
    auto bwdL = [&](double v) { for (int c = nz - 1; c >= 0; c--) { const double xc = rdlane(v, c) * dv[c]; if (lane == c) v = xc; else if (lane < c) v = fma(-Ls[c + (size_t)lane * nz], xc, v); } return v; };
    auto solveS = [&](double v) {
        for (int c = 0; c < nc; c++) { const double yc = rdlane(v, c) * sv[c]; if (lane == c) v = yc; else if (row && lane > c) v = fma(-Ss[lane + (size_t)c * nc], yc, v); }
        for (int c = nc - 1; c >= 0; c--) { const double xc = rdlane(v, c) * sv[c]; if (lane == c) v = xc; else if (lane < c) v = fma(-Ss[c + (size_t)lane * nc], xc, v); }
        return v;
    };
    /* (Y' a)_r in lane r for the rows of W, 0 elsewhere; (Y w)_i in lane i; (G_W' w)_i in lane i */
    auto Yt = [&](double a) { double acc = 0.0; for (int i = 0; i < nz; i++) acc = fma(Ys[i + (size_t)rl * nz], rdlane(a, i), acc); return inw ? acc : 0.0; };
    auto Yw = [&](double w) { double acc = 0.0; for (int r = 0; r < nc; r++) if ((mr >> r) & 1ull) acc = fma(Ys[zl + (size_t)r * nz], rdlane(w, r), acc); return own ? acc : 0.0; };
    auto Gtw = [&](double w) { double acc = 0.0; for (int r = 0; r < nc; r++) if ((mr >> r) & 1ull) acc = fma(Gt[zl + (size_t)r * nz], rdlane(w, r), acc); return own ? acc : 0.0; };
    auto Hv = [&](double v) { double acc = 0.0; for (int j = 0; j < nz; j++) acc = fma(Hs[zl + (size_t)j * nz], rdlane(v, j), acc); return own ? acc : 0.0; };
    /* the minimiser on the working set (fixed entries of z stay): z and nu */
    auto eqp = [&]() {
        double r = h;
        for (int j = 0; j < nz; j++) if ((mb >> j) & 1ull) r = fma(-Hs[zl + (size_t)j * nz], rdlane(z, j), r);
        if (fixed || !own) r = fixed ? z : 0.0;
        const double y0 = fwdL(r);
        double c = 0.0;                                       /* G_W z0 - d_W */
        for (int j = 0; j < nz; j++) if ((mb >> j) & 1ull) c = fma(Gt[j + (size_t)rl * nz], rdlane(z, j), c);
        const double yt = Yt(y0);
        c = inw ? c + yt - (sr > 0.0 ? dlo : dhi) : 0.0;
        const double w = solveS(c);
        const double zn = bwdL(y0 - Yw(w));
        if (own && !fixed) z = zn;
        nur = inw ? -w : 0.0;
    };

    bool ok = false;
    int steps = 0;                         /* active-set steps of this stage solve, every pass (tqgpu_get_stage_steps) */
    u64 lmb = 0ull;                        /* the fixed set the factor in Ls was built for (lhave: there is one) */
    bool lhave = false;
    /* pass 0: from the stored working set (hot start on); pass 1: cold, from the equalities -- the only pass with the hot start off, and the
     * redo of a pass 0 that did not end with ok */
    for (int pass = Gn.hot ? 0 : 1; pass < 2 && !ok; pass++) {
        bool dfr = pass == 0;                  /* dual-feasibility rounds of the stored set still to do */
        {
            /* the stored set against the current data: lanes beyond nz / nc and members whose bound on the stored side is infinite drop out */
            bool kb = false, kr = false, ub = false, ur = false;
            if (dfr) {
                ub = (Gn.sides[k] >> lane) & 1ull; ur = (Gn.sides[T.Nn + k] >> lane) & 1ull;
                kb = own && ((D.bmask[k] >> lane) & 1ull) && (ub ? hi < inf : lo > -inf);
                kr = row && ((Gn.rmask[k] >> lane) & 1ull) && (ur ? dhi < inf : dlo > -inf);
            }
            fixed = own && (lo == hi || kb); inw = row && (dlo == dhi || kr);
            sg = (fixed && lo < hi && ub) ? -1.0 : 1.0; sr = (inw && dlo < dhi && ur) ? -1.0 : 1.0;
            nur = 0.0;
            z = fixed ? (sg > 0.0 ? lo : hi) : 0.0;
            mb = __builtin_amdgcn_ballot_w64(fixed); mr = __builtin_amdgcn_ballot_w64(inw);
        }
        int ptype = 0, pidx = 0;               /* the constraint being added: 0 none, 1 bound, 2 row; its side in psg, its multiplier in up */
        double psg = 1.0, up = 0.0;
        for (int step = 0; step < GEN_MAX_STEPS(nz, nc); step++) {
            steps++;
            WSYNC();
            bool pd = true;
            if (!lhave || mb != lmb) {
                /* M of the fixed set and its Cholesky factor, left looking, lane i = row i (as stage_box); kept while the fixed set stays */
                lhave = false;
                for (int j = 0; j < nz; j++) {
                    const bool fj = (mb >> j) & 1ull;
                    if (own) Ls[lane + (size_t)j * nz] = (fixed || fj) ? (lane == j ? 1.0 : 0.0) : Hs[lane + (size_t)j * nz];
                }
                WSYNC();
                for (int j = 0; j < nz; j++) {
                    if (own && lane >= j) {
                        double sacc = Ls[lane + (size_t)j * nz];
                        for (int c = 0; c < j; c++) sacc = fma(-Ls[lane + (size_t)c * nz], Ls[j + (size_t)c * nz], sacc);
                        Ls[lane + (size_t)j * nz] = sacc;
                    }
                    WSYNC();
                    const double cjj = Ls[j + (size_t)j * nz];
                    pd = pd && cjj > 0.0;
                    const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;
                    if (own && lane >= j) Ls[lane + (size_t)j * nz] *= finv;
                    if (lane == 0) dv[j] = finv;
                    WSYNC();
                }
                lhave = pd; lmb = mb;
            }
            if (!pd) break;                                        /* H_FF not positive definite */
            /* Y and S of the rows in W, and the factor of S */
            for (int r = 0; r < nc; r++) {
                if (!((mr >> r) & 1ull)) continue;
                const double y = fwdL(own && !fixed ? Gt[lane + (size_t)r * nz] : 0.0);
                if (own) Ys[lane + (size_t)r * nz] = y;
            }
            WSYNC();
            for (int j = 0; j < nc; j++) {
                const bool wj = (mr >> j) & 1ull;
                double acc = lane == j ? 1.0 : 0.0;
                if (wj && inw) { acc = 0.0; for (int i = 0; i < nz; i++) acc = fma(Ys[i + (size_t)rl * nz], Ys[i + (size_t)j * nz], acc); }
                else if (wj) acc = 0.0;
                if (row) Ss[lane + (size_t)j * nc] = acc;
            }
            WSYNC();
            for (int j = 0; j < nc; j++) {
                const double sjj = Ss[j + (size_t)j * nc];
                if (row && lane >= j) {
                    double sacc = Ss[lane + (size_t)j * nc];
                    for (int c = 0; c < j; c++) sacc = fma(-Ss[lane + (size_t)c * nc], Ss[j + (size_t)c * nc], sacc);
                    Ss[lane + (size_t)j * nc] = sacc;
                }
                WSYNC();
                const double cjj = Ss[j + (size_t)j * nc];
                pd = pd && cjj > eps64 * sjj;                      /* the rows of the working set depend on each other */
                const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;
                if (row && lane >= j) Ss[lane + (size_t)j * nc] *= finv;
                if (lane == 0) sv[j] = finv;
                WSYNC();
            }
            if (!pd) break;
            if (dfr) {
                /* the minimiser on the stored set and the multipliers of its members that are no equalities, sg om and sr nu_r: every member whose
                 * multiplier is negative beyond 64 eps (sum of |terms|) leaves, all of them in one round; the set only shrinks */
                eqp();
                double om = -h, oa = fabs(h);
                for (int j = 0; j < nz; j++) { const double t = Hs[zl + (size_t)j * nz] * rdlane(z, j); om += t; oa += fabs(t); }
                for (int r = 0; r < nc; r++) if ((mr >> r) & 1ull) { const double t = Gt[zl + (size_t)r * nz] * rdlane(nur, r); om -= t; oa += fabs(t); }
                const double na = wsum(fabs(nur));
                const bool wrongb = fixed && lo < hi && sg * om < -eps64 * oa, wrongr = inw && dlo < dhi && sr * nur < -eps64 * na;
                const u64 wb = __builtin_amdgcn_ballot_w64(wrongb), wr = __builtin_amdgcn_ballot_w64(wrongr);
                if (wb | wr) {
                    if (wrongb) fixed = false;
                    if (wrongr) { inw = false; nur = 0.0; }
                    mb &= ~wb; mr &= ~wr;
                    continue;
                }
                dfr = false;                                       /* z minimises on W, the multipliers are >= 0: the loop below goes on from here */
            } else if (step == 0) eqp();
            if (ptype == 0) {
                /* the most violated constraint outside the working set */
                double vb = 0.0, vr = 0.0, act = 0.0, aabs = 0.0;
                if (own && !fixed) {
                    if (lo - z > eps64 * (fabs(z) + fabs(lo))) vb = lo - z;
                    if (z - hi > eps64 * (fabs(z) + fabs(hi))) vb = z - hi;
                }
                for (int j = 0; j < nz; j++) { const double t = Gt[j + (size_t)rl * nz] * rdlane(z, j); act += t; aabs += fabs(t); }
                if (row && !inw) {
                    if (dlo - act > eps64 * (aabs + fabs(dlo))) vr = dlo - act;
                    if (act - dhi > eps64 * (aabs + fabs(dhi))) vr = act - dhi;
                }
                const double vmax = fmax(wmax(vb), wmax(vr));
                if (!(vmax > 0.0)) { eqp(); ok = true; break; }
                const u64 bb = __builtin_amdgcn_ballot_w64(vb == vmax), br = __builtin_amdgcn_ballot_w64(vr == vmax);
                ptype = bb ? 1 : 2;
                pidx = __builtin_amdgcn_readfirstlane(__builtin_ctzll(bb ? bb : br));
                const double side = ptype == 1 ? (z < lo ? 1.0 : -1.0) : (act < dlo ? 1.0 : -1.0);
                psg = rdlane(side, pidx);
                up = 0.0;
            }
            /* n_p, its violation b_p - n_p'z > 0, the directions */
            const double np = ptype == 1 ? (lane == pidx ? psg : 0.0) : (own ? psg * Gt[lane + (size_t)pidx * nz] : 0.0);
            double viol;
            if (ptype == 1) viol = rdlane(psg > 0.0 ? lo - z : z - hi, pidx);
            else { const double act = wsum(own ? Gt[lane + (size_t)pidx * nz] * z : 0.0); viol = psg > 0.0 ? rdlane(dlo, pidx) - act : act - rdlane(dhi, pidx); }
            const double a = fwdL(own && !fixed ? np : 0.0);
            const double rr = solveS(Yt(a));
            const double e = a - Yw(rr);
            const double q = wsum(e * e), qd = wsum(a * a);
            const bool dep = !(q > eps64 * qd);                    /* p depends on the working set: no primal step */
            double dz = bwdL(e);
            if (!own || fixed) dz = 0.0;
            /* multipliers of the fixed entries and of the rows (u >= 0 with their sides) and the rates at which a step lowers them */
            const double gtr = Gtw(rr), gtn = Gtw(nur);
            const double om = Hv(z) - h - gtn - np * up;           /* fixed entries: sg * om is their multiplier */
            const double rb = np - Hv(dz) - gtr;
            const bool cb = fixed && lo < hi && sg * rb > 0.0, cr = inw && dlo < dhi && sr * rr > 0.0;
            const double tb = cb ? fmax(sg * om, 0.0) / (sg * rb) : inf, tr = cr ? fmax(sr * nur, 0.0) / (sr * rr) : inf;
            const double tbm = -wmax(-tb), trm = -wmax(-tr);
            const double t1 = fmin(tbm, trm), t2 = dep ? inf : fmax(viol, 0.0) / q;
            if (t1 == inf && t2 == inf) break;                     /* no step possible: the stage QP is infeasible */
            const double t = fmin(t1, t2);
            if (!dep && own && !fixed) z = fma(t, dz, z);
            if (inw) nur = fma(-t, rr, nur);
            up += t;
            if (t2 <= t1) {
                /* full step: p joins the working set */
                if (ptype == 1) { if (lane == pidx) { z = psg > 0.0 ? lo : hi; fixed = true; sg = psg; } mb |= 1ull << pidx; }
                else { if (lane == pidx) { inw = true; sr = psg; nur = psg * up; } mr |= 1ull << pidx; }
                ptype = 0;
            } else if (tbm <= trm) {
                const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__builtin_amdgcn_ballot_w64(cb && tb == tbm)));
                if (lane == i) fixed = false;
                mb &= ~(1ull << i);
            } else {
                const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__builtin_amdgcn_ballot_w64(cr && tr == trm)));
                if (lane == i) { inw = false; nur = 0.0; }
                mr &= ~(1ull << i);
            }
        }
    }
    if (!ok && lane == 0) { D.ctrl->status = 4; D.ctrl->done = 1; }      /* TREEQP_DN_STAGE_QP_SOLVE_FAILED */
    const u64 ub = __builtin_amdgcn_ballot_w64(fixed && sg < 0.0), ur = __builtin_amdgcn_ballot_w64(inw && sr < 0.0);
    if (lane == 0) {
        D.bmask[k] = mb; Gn.rmask[k] = mr; Gn.sides[k] = ub; Gn.sides[T.Nn + k] = ur;
        Gn.steps_last[k] = steps; Gn.steps_total[k] += steps;
    }
    if (row) Gn.mu[ro + lane] = inw ? -nur : 0.0;
    if (own) {
        if (isx) { if (save_s) D.xUncS[xo + j0] = D.xUnc[xo + j0]; D.x[xo + j0] = z; D.xUnc[xo + j0] = h; }
        else { if (save_s) D.uUncS[uo + j0] = D.uUnc[uo + j0]; D.u[uo + j0] = z; D.uUnc[uo + j0] = h; }
    }
    /* dual term -1/2 z'Hz + hmod'z - cmod, as stage_box takes it */
    const double hz = Hv(z);
    double p_quad = own ? z * hz : 0.0, p_lin = own ? h * z : 0.0, p_cd = 0.0;
    for (int t = lane; t < d; t += WAVE) p_cd = fma(D.b[ko + t], lk[t], p_cd);
    p_quad = wave_sum(p_quad); p_lin = wave_sum(p_lin); p_cd = wave_sum(p_cd);
    if (lane == 0) D.fval[k] = -0.5 * p_quad - p_cd + p_lin;
    if (!ok || (mb == D.bmask[T.Nn + k] && mr == Gn.rmask[T.Nn + k])) return;
    /* column j of P is the primal direction of n = e_j (the factors of the final working set are in LDS) */
    double *P = D.Pd + D.poff[k];
    for (int j = 0; j < nz; j++) {
        double col = 0.0;
        if (!((mb >> j) & 1ull)) {
            const double a = fwdL(lane == j ? 1.0 : 0.0);
            col = bwdL(a - Yw(solveS(Yt(a))));
            if (!own || fixed) col = 0.0;
        }
        if (own) P[lane + (size_t)j * nz] = col;
    }
    if (lane == 0) { D.bmask[T.Nn + k] = mb; Gn.rmask[T.Nn + k] = mr; }
}

/* BOX: 0 no box nodes, 1 stage_box compiled in, 2 stage_box and stage_gen */
template <int BOX = 0>
__device__ void stage_body(const Tree &T, const Data &D, int mode, int k, int lane, double *lds, bool batch = true, u64 *xu = nullptr, int sum_nx = 0, unsigned xtag = 0u,
                           const double *Cl = nullptr, int ldcl = 0) {
    const Ctrl *c = D.ctrl;
    const int nxk = T.nx[k], nuk = T.nu[k], xo = T.xoff[k], uo = T.uoff[k];
    const int nkid = T.nk[k], d = T.bdim[k];
    const double *lamc = c->cur ? D.lam1 : D.lam0;
    double *lamn = c->cur ? D.lam0 : D.lam1;
    const double step = c->tau - c->tauPrev;
    const bool save_s = mode == 1 && c->ls_iter == 1;     /* first trial of a line search: xUnc / uUnc still hold phase S of this iteration */

    /* lambda of the children = dual block of node k, contiguous at xoff[kid0] */
    double *lk = lds;                   /* d doubles  */
    double *lown = lds + d;             /* nxk doubles */
    const int ko = nkid > 0 ? T.xoff[T.kid0[k]] : 0;
    for (int t = lane; t < d; t += WAVE) {
        double v = lamc[ko + t];
        if (mode == 1) v = fma(step, D.dlam[ko + t], v);
        lk[t] = v;
    }
    for (int t = lane; t < nxk; t += WAVE) {
        double v = 0.0;
        if (k > 0) {
            v = lamc[xo + t];
            if (mode == 1) { v = fma(step, D.dlam[xo + t], v); lamn[xo + t] = v; }
        }
        lown[t] = v;
    }
    WSYNC();

    if (D.dense && D.kind[k]) {
        /* dense unconstrained stage QP: z = P hmod; dual term -1/2 z'Hz + hmod'z - cmod */
        const int nz = nxk + nuk;
        double *hm = lds + d + nxk, *zz = hm + nz;
        for (int t = lane; t < nz; t += WAVE) {
            const bool isx = t < nxk;
            const int j = isx ? t : t - nxk;
            double v = isx ? fma(-1.0, D.q[xo + j], lown[j]) : -1.0 * D.r[uo + j];
            int rowoff = 0;
            for (int cc = 0; cc < nkid; cc++) {
                const int kid = T.kid0[k] + cc, nxc = T.nx[kid];
                const double *col = isx ? D.A + T.aoff[kid] + (size_t)j * nxc : D.B + T.boff[kid] + (size_t)j * nxc;
                double acc = 0.0;
                acc = dot_batched(col, 1, lk + rowoff, 1, nxc, acc, batch);
                v = fma(-1.0, acc, v);
                rowoff += nxc;
            }
            hm[t] = v;
            if (isx) D.qmod[xo + j] = v; else D.rmod[uo + j] = v;
        }
        WSYNC();
        if constexpr (BOX) {
            if (D.kind[k] == 2) { stage_box(T, D, k, lane, hm + nz, hm, lk, ko, save_s); return; }
        }
        if constexpr (BOX == 2) {
            if (D.kind[k] == 3) { stage_gen(T, D, k, lane, hm + nz, hm, lk, ko, save_s); return; }
        }
        const double *P = D.Pd + D.poff[k], *H = D.Hd + D.poff[k];
        for (int t = lane; t < nz; t += WAVE) {
            double acc = 0.0;
            for (int j = 0; j < nz; j++) acc = fma(P[t + (size_t)j * nz], hm[j], acc);
            zz[t] = acc;
            if (xu && nkid > 0) st_tag(xu + 2 * (size_t)(t < nxk ? xo + t : sum_nx + uo + t - nxk), acc, xtag);
            if (t < nxk) { if (save_s) D.xUncS[xo + t] = D.xUnc[xo + t]; D.x[xo + t] = acc; D.xUnc[xo + t] = acc; }
            else { if (save_s) D.uUncS[uo + t - nxk] = D.uUnc[uo + t - nxk]; D.u[uo + t - nxk] = acc; D.uUnc[uo + t - nxk] = acc; }
        }
        WSYNC();
        double p_quad = 0.0, p_lin = 0.0, p_cd = 0.0;
        for (int t = lane; t < nz; t += WAVE) {
            double acc = 0.0;
            for (int j = 0; j < nz; j++) acc = fma(H[t + (size_t)j * nz], zz[j], acc);
            p_quad = fma(zz[t], acc, p_quad);
            p_lin = fma(hm[t], zz[t], p_lin);
        }
        for (int t = lane; t < d; t += WAVE) p_cd = fma(D.b[ko + t], lk[t], p_cd);
        p_quad = wave_sum(p_quad); p_lin = wave_sum(p_lin); p_cd = wave_sum(p_cd);
        if (lane == 0) D.fval[k] = -0.5 * p_quad - p_cd + p_lin;
        return;
    }

    double p_qx = 0.0, p_hx = 0.0, p_ru = 0.0, p_hu = 0.0;   /* partial dots for the dual term */
    for (int t = lane; t < nxk + nuk; t += WAVE) {
        const bool isx = t < nxk;
        const int j = isx ? t : t - nxk;
        double v = isx ? fma(-1.0, D.q[xo + j], lown[j]) : -1.0 * D.r[uo + j];
        int rowoff = 0;
        for (int cc = 0; cc < nkid; cc++) {
            const int kid = T.kid0[k] + cc, nxc = T.nx[kid];
            const double *col = Cl ? Cl + rowoff + (size_t)t * ldcl : (isx ? D.A + T.aoff[kid] + (size_t)j * nxc : D.B + T.boff[kid] + (size_t)j * nxc);
            double acc = 0.0;
            acc = dot_batched(col, 1, lk + rowoff, 1, nxc, acc, batch && !Cl);
            v = fma(-1.0, acc, v);
            rowoff += nxc;
        }
        if (isx) {
            D.qmod[xo + j] = v;
            const double qi = D.Qinv[xo + j];
            const double unc = qi * v, lo = D.xmin[xo + j], hi = D.xmax[xo + j];
            double xv, cal;
            if (unc >= hi) { xv = hi; cal = 0.0; } else if (unc <= lo) { xv = lo; cal = 0.0; } else { xv = unc; cal = qi; }
            if (xu && nkid > 0) st_tag(xu + 2 * (size_t)(xo + j), xv, xtag);
            if (save_s) D.xUncS[xo + j] = D.xUnc[xo + j];
            D.xUnc[xo + j] = unc; D.x[xo + j] = xv; D.QinvCal[xo + j] = cal;
            p_qx = fma(D.Qd[xo + j] * xv, xv, p_qx);
            p_hx = fma(v, xv, p_hx);
        } else {
            D.rmod[uo + j] = v;
            const double ri = D.Rinv[uo + j];
            const double unc = ri * v, lo = D.umin[uo + j], hi = D.umax[uo + j];
            double uv, cal;
            if (unc >= hi) { uv = hi; cal = 0.0; } else if (unc <= lo) { uv = lo; cal = 0.0; } else { uv = unc; cal = ri; }
            if (xu && nkid > 0) st_tag(xu + 2 * (size_t)(sum_nx + uo + j), uv, xtag);
            if (save_s) D.uUncS[uo + j] = D.uUnc[uo + j];
            D.uUnc[uo + j] = unc; D.u[uo + j] = uv; D.RinvCal[uo + j] = cal;
            p_ru = fma(D.Rd[uo + j] * uv, uv, p_ru);
            p_hu = fma(v, uv, p_hu);
        }
    }
    /* cmod = sum_kids b_kid' lambda_kid */
    double p_c = 0.0;
    for (int t = lane; t < d; t += WAVE) p_c = fma(D.b[ko + t], lk[t], p_c);
    p_qx = wave_sum(p_qx); p_hx = wave_sum(p_hx); p_ru = wave_sum(p_ru); p_hu = wave_sum(p_hu); p_c = wave_sum(p_c);
    if (D.strict && nxk + nuk <= WAVE) {
        /* the node's term from sequential dot products, as eval_dual_term takes them (clipping.c:374-381): lane t holds entry t of
         * [x | u] (read back from where this wave has just put it), every lane takes the same sums */
        WSYNC();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        const int t = lane < nxk + nuk ? lane : 0;
        const bool isx = t < nxk;
        const int j = isx ? t : t - nxk;
        const double val = isx ? D.x[xo + j] : D.u[uo + j], hm = isx ? D.qmod[xo + j] : D.rmod[uo + j];
        const double wv = (isx ? D.Qd[xo + j] : D.Rd[uo + j]) * val;
        double a_qx = 0.0, a_hx = 0.0, a_ru = 0.0, a_hu = 0.0, cm = 0.0;
        for (int i = 0; i < nxk; i++) { const double vi = __shfl(val, i), wi = __shfl(wv, i), hi = __shfl(hm, i); a_qx = fma(wi, vi, a_qx); a_hx = fma(hi, vi, a_hx); }
        for (int i = nxk; i < nxk + nuk; i++) { const double vi = __shfl(val, i), wi = __shfl(wv, i), hi = __shfl(hm, i); a_ru = fma(wi, vi, a_ru); a_hu = fma(hi, vi, a_hu); }
        int off = 0;
        for (int cc = 0; cc < nkid; cc++) {                 /* cmod += ddot(b_kid, lambda_kid), child after child (dual_Newton_tree.c:892) */
            const int nxc = T.nx[T.kid0[k] + cc];
            double acc = 0.0;
            for (int i = 0; i < nxc; i++) acc = fma(D.b[ko + off + i], lk[off + i], acc);
            cm += acc;
            off += nxc;
        }
        p_qx = a_qx; p_hx = a_hx; p_ru = a_ru; p_hu = a_hu; p_c = cm;
    }
    if (lane == 0) {
        double f = -0.5 * p_qx - p_c;       /* clipping.c:375 */
        f += p_hx;                          /* :376 */
        f -= 0.5 * p_ru;                    /* :380 */
        f += p_hu;                          /* :381 */
        D.fval[k] = f;
    }
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_stage(Tree T, Data D, int mode, int h, int t) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (mode == 1 && !phase_trial(D.ctrl, h, t)) return;
    stage_body(T, D, mode, blockIdx.x, threadIdx.x, lds);
}
/* k_stage for trees with dense box nodes (kind 2): the same sweep with stage_box compiled in (its LDS, s->sk.lds_box, only here) */
__global__ void __launch_bounds__(WAVE) k_stage_box(Tree T, Data D, int mode, int h, int t) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (mode == 1 && !phase_trial(D.ctrl, h, t)) return;
    stage_body<1>(T, D, mode, blockIdx.x, threadIdx.x, lds);
}
/* k_stage for trees with kind-3 nodes: the same sweep with stage_gen compiled in as well (its LDS, s->sk.lds_gen, only here) */
__global__ void __launch_bounds__(WAVE) k_stage_gen(Tree T, Data D, int mode, int h, int t) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (mode == 1 && !phase_trial(D.ctrl, h, t)) return;
    stage_body<2>(T, D, mode, blockIdx.x, threadIdx.x, lds);
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* block reductions (one workgroup of 256 threads, fixed pairwise order => deterministic)      */
/* ------------------------------------------------------------------------------------------ */
/* Reference-order sums (opt-in: TREEQP_AMD_STRICT_SUM=1, Data::strict).  The reference adds the nodes' dual-function terms one after the other
 * (evaluate_dual_function, dual_Newton_tree.c:915), takes res' dlam and the squared residual norm as one ddot per dual block, blocks in order
 * (gradient_trans_times_direction :808-820, calculate_error_in_residuals :412-442), and a node's own term from sequential dot products
 * (eval_dual_term, dual_Newton_tree_clipping.c:359-382).  The default kernels take all of these as fixed trees (deterministic, but another
 * order): near the optimum two dual values may then differ in their last bit and an Armijo or termination test goes the other way
 * (0.6 % of a random campaign).  With the switch on, one thread takes the sums in the reference's order -- slow, for parity work. */
__device__ double strict_sum(const double *v, int n) {
    double acc = 0.0;
    for (int i = 0; i < n; i++) acc += v[i];
    return acc;
}
__device__ double strict_block_dots(const Tree &T, const double *a, const double *b) {
    double ans = 0.0;
    for (int p = 0; p < T.Np; p++) {
        const int o = T.xoff[T.kid0[p]], d = T.bdim[p];
        double acc = 0.0;
        for (int i = 0; i < d; i++) acc = fma(a[o + i], b[o + i], acc);
        ans += acc;
    }
    return ans;
}
/* a value computed by thread 0 to every thread of the workgroup */
__device__ double bcast0(double v, double *sh) {
    __syncthreads();
    if (threadIdx.x == 0) sh[0] = v;
    __syncthreads();
    const double r = sh[0];
    __syncthreads();
    return r;
}

template <bool IS_MAX>
__device__ double block_reduce(const double *v, int n, double *sh) {
    /* strided per-thread partials, wave shuffle tree, then the (<= 16) wave results in order */
    double acc = 0.0;
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * blockDim.x) {          /* eight loads in flight per thread, same order of the sums */
        double t[8];
#pragma unroll
        for (int m = 0; m < 8; m++) { const int i = i0 + m * (int)blockDim.x; t[m] = v[i < n ? i : 0]; }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int m = 0; m < 8; m++) { const int i = i0 + m * (int)blockDim.x; if (i < n) acc = IS_MAX ? nanmax(acc, t[m]) : acc + t[m]; }
    }
    acc = IS_MAX ? wave_max(acc) : wave_sum(acc);
    __syncthreads();                                   /* sh may still be read from a previous call */
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    double r = 0.0;
    const int nw = (blockDim.x + WAVE - 1) / WAVE;
    for (int w = 0; w < nw; w++) r = IS_MAX ? nanmax(r, sh[w]) : r + sh[w];
    return r;
}

/* first sweep of a solve: fval0 = sum of the node terms */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(256) k_fval_init(Tree T, Data D) {
    __shared__ double sh[256];
    const double f = D.strict ? bcast0(threadIdx.x == 0 ? strict_sum(D.fval, T.Nn) : 0.0, sh) : block_reduce<false>(D.fval, T.Nn, sh);
    if (threadIdx.x == 0) { D.ctrl->fval0 = f; D.ctrl->fval = f; }
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* The small reductions as the TAIL of the sweep that produces their input (trees of <= FUSE_MAX nodes).  A reduction kernel of
 * its own (k_check, k_fval_init, k_ls_begin, k_ls_decide) is a launch of one workgroup: ~5 us for a few hundred additions, and a
 * single tree of a few hundred nodes is bound by its launch count.  Instead every workgroup of the sweep posts its partial as a
 * tagged word and counts itself off; the workgroup that finds it is the last takes the reduction -- in the order block_reduce
 * takes it with 256 threads, so the result is bit-identical to the separate kernel's -- and the decision.  (The partials
 * travel as tagged words and are polled, so nothing depends on the order in which plain stores of other XCDs become visible.) */
#define FUSE_MAX 512
struct Fuse { u64 *red; int *cnt; unsigned tag; int on; };

__device__ __forceinline__ bool fuse_last(const Fuse &F, int total, int lane) {
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(F.cnt, 1, RLX, AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old == total - 1 && lane == 0) __hip_atomic_store(F.cnt, 0, RLX, AGENT);      /* the next launch counts from zero */
    return old == total - 1;
}
/* sum / maximum of entries first .. first + n - 1 (n <= FUSE_MAX) of the tagged partials, by ONE wave, as block_reduce<IS_MAX> with
 * 256 threads: lane l stands in for threads l, l + 64, l + 128, l + 192; `extra0` (with_extra) is entry 0 of the reduced vector,
 * known to this wave already (the root's part_dot), the tagged words then hold entries 1 .. */
template <bool IS_MAX>
__device__ double fuse_reduce(const u64 *red, int first, int n, unsigned tag, int lane, bool with_extra = false, double extra0 = 0.0) {
    double v[4][2];
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int i = w * WAVE + lane + 256 * j;                    /* index into the reduced vector */
                const bool in = i < n;
                bool okk = true;
                double val = 0.0;
                if (with_extra && i == 0) val = extra0;
                else { val = ld_tag(red + (size_t)(first + (in ? i - (with_extra ? 1 : 0) : 0)) * 2, tag, okk); ok = ok && (okk || !in); }
                v[w][j] = in ? val : 0.0;
            }
        if (__all(ok)) break;
        if (wall_clock64() - t0 > 20000000ull) return __builtin_nan("");      /* 0.2 s: cannot happen (every workgroup posted before it counted itself off); a NaN ends the solve */
        __builtin_amdgcn_s_sleep(2);
    }
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 2; j++) { const int i = w * WAVE + lane + 256 * j; if (i < n) acc = IS_MAX ? nanmax(acc, v[w][j]) : acc + v[w][j]; }
        acc = IS_MAX ? wave_max(acc) : wave_sum(acc);
        r = IS_MAX ? nanmax(r, acc) : r + acc;
    }
    return r;
}

/* ------------------------------------------------------------------------------------------ */
/* k_grad: one wave per node k >= 1:  res_k = b_k - x_k + A_k x_dad + B_k u_dad                */
/* ------------------------------------------------------------------------------------------ */
__device__ void grad_body(const Tree &T, const Data &D, int termCondition, int k, int lane, bool batch = true) {
    const int p = T.dad[k], nxk = T.nx[k], nxp = T.nx[p], nup = T.nu[p];
    const int xo = T.xoff[k], xp = T.xoff[p], up = T.uoff[p];
    const double *A = D.A + T.aoff[k], *B = D.B + T.boff[k];
    double part = 0.0;
    for (int i = lane; i < nxk; i += WAVE) {
        double rv = fma(-1.0, D.x[xo + i], D.b[xo + i]);
        double acc = 0.0;
        acc = dot_batched(A + i, nxk, D.x + xp, 1, nxp, acc, batch);
        rv += acc;
        acc = 0.0;
        acc = dot_batched(B + i, nxk, D.u + up, 1, nup, acc, batch);
        rv += acc;
        D.res[xo + i] = rv;
        D.resMod[xo + i] = rv;
        part = (termCondition == 2) ? nanmax(part, fabs(rv)) : fma(rv, rv, part);
    }
    part = (termCondition == 2) ? wave_max(part) : wave_sum(part);
    if (lane == 0) D.part_err[k] = part;
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_grad(Tree T, Data D, int termCondition, int h) {
    if (!phase_main(D.ctrl, h)) return;
    grad_body(T, D, termCondition, blockIdx.x + 1, threadIdx.x);
}
#endif

/* termination test; also the top-of-loop bookkeeping of the Newton iteration */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(256) k_check(Tree T, Data D, Opts O, int h) {
    __shared__ double sh[256];
    Ctrl *c = D.ctrl;
    if (!phase_main(c, h)) return;
    double err = (O.termCondition == 2) ? block_reduce<true>(D.part_err + 1, T.Nn - 1, sh)
                                        : (D.strict ? bcast0(threadIdx.x == 0 ? strict_block_dots(T, D.res, D.res) : 0.0, sh) : block_reduce<false>(D.part_err + 1, T.Nn - 1, sh));
    if (threadIdx.x == 0) {
        if (O.termCondition == 1) err = sqrt(err);
        c->err = err;
        if (err < O.tol) { c->done = 1; c->status = 0; }      /* TREEQP_OPTIMAL_SOLUTION_FOUND */
    }
}
#endif

/* k_grad with k_check as its tail (small trees) */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_grad_f(Tree T, Data D, Opts O, Fuse F, int h) {
    Ctrl *c = D.ctrl;
    if (!phase_main(c, h)) return;
    const int k = blockIdx.x + 1, lane = threadIdx.x;
    grad_body(T, D, O.termCondition, k, lane);
    if (lane == 0) st_tag(F.red + (size_t)(k - 1) * 2, D.part_err[k], F.tag);
    if (!fuse_last(F, T.Nn - 1, lane)) return;
    double err = (O.termCondition == 2) ? fuse_reduce<true>(F.red, 0, T.Nn - 1, F.tag, lane) : fuse_reduce<false>(F.red, 0, T.Nn - 1, F.tag, lane);
    if (lane == 0) {
        if (O.termCondition == 1) err = sqrt(err);
        c->err = err;
        if (err < O.tol) { c->done = 1; c->status = 0; }      /* TREEQP_OPTIMAL_SOLUTION_FOUND */
    }
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* k_hess: one wave per parent block p.                                                        */
/*   W_p = C P C' + blockdiag(QinvCal_kids),  C = [A_c B_c] stacked over the children,         */
/*   P = diag(QinvCal_p, RinvCal_p);   Ut_p = -(C[:, :nx_p] P)'                                */
/* ------------------------------------------------------------------------------------------ */
__device__ void hess_body(const Tree &T, const Data &D, int p, int lane, double *lds) {
    const int d = T.bdim[p], nxp = T.nx[p], nup = T.nu[p], nz = nxp + nup;
    double *Cs = lds;                 /* d x nz, column major, ld = d */
    double *CP = lds + (size_t)d * nz;
    const int k0 = T.kid0[p], ko = T.xoff[k0];
    const double *Qc = D.QinvCal + T.xoff[p], *Rc = D.RinvCal + T.uoff[p];
    const bool pdense = D.dense && D.kind[p];           /* the parent's elimination matrix: dense P_p = H_p^-1, or diag(QinvCal_p, RinvCal_p) */
    /* stage the children's [A B] rows */
    int rowoff = 0;
    for (int cc = 0; cc < T.nk[p]; cc++) {
        const int kid = k0 + cc, nxc = T.nx[kid];
        const double *A = D.A + T.aoff[kid], *B = D.B + T.boff[kid];
        for (int e = lane; e < nxc * nz; e += WAVE) {
            const int i = e % nxc, col = e / nxc;
            const double a = col < nxp ? A[i + (size_t)col * nxc] : B[i + (size_t)(col - nxp) * nxc];
            Cs[rowoff + i + (size_t)col * d] = a;
            if (!pdense) { const double pc = col < nxp ? Qc[col] : Rc[col - nxp]; CP[rowoff + i + (size_t)col * d] = a * pc; }
        }
        rowoff += nxc;
    }
    WSYNC();
    if (pdense) {
        /* CP = C P_p with the dense elimination matrix of the parent (build_M of the qpOASES stage solver) */
        const double *P = D.Pd + D.poff[p];
        for (int e = lane; e < d * nz; e += WAVE) {
            const int i = e % d, col = e / d;
            double acc = 0.0;
            for (int cidx = 0; cidx < nz; cidx++) acc = fma(Cs[i + (size_t)cidx * d], P[cidx + (size_t)col * nz], acc);
            CP[i + (size_t)col * d] = acc;
        }
        WSYNC();
    }
    double *W = D.W + T.woff[p];
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i < j) continue;
        double acc = 0.0, acc2 = 0.0;
        for (int cidx = 0; cidx < nxp; cidx++) acc = fma(Cs[i + (size_t)cidx * d], CP[j + (size_t)cidx * d], acc);
        for (int cidx = nxp; cidx < nz; cidx++) acc2 = fma(Cs[i + (size_t)cidx * d], CP[j + (size_t)cidx * d], acc2);
        double w = acc + acc2;
        if (!D.dense) { if (i == j) w += D.QinvCal[ko + i]; }
        else {
            /* add_EPmE: the state block of the CHILD's own elimination matrix on the diagonal block -- dense P_kid, or the
             * clipped inverse weights of a clipping child (the solver kinds of a node and of its children need not agree:
             * per-node opts->qp_solver[], dual_Newton_tree.c:124-162) */
            int ro = 0;
            for (int cc = 0; cc < T.nk[p]; cc++) {
                const int kid = k0 + cc, nxc = T.nx[kid];
                if (i >= ro && i < ro + nxc && j >= ro && j < ro + nxc) {
                    if (D.kind[kid]) { const int nzk = nxc + T.nu[kid]; w += D.Pd[D.poff[kid] + (i - ro) + (size_t)(j - ro) * nzk]; }
                    else if (i == j) w += D.QinvCal[ko + i];
                }
                ro += nxc;
            }
        }
        W[i + (size_t)j * d] = w;
    }
    if (p > 0) {
        double *Ut = D.Ut + T.utoff[p];
        for (int e = lane; e < nxp * d; e += WAVE) {
            const int i = e % nxp, rr = e / nxp;
            Ut[i + (size_t)rr * nxp] = -1.0 * CP[rr + (size_t)i * d];
        }
    }
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_hess(Tree T, Data D, int h) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (!phase_main(D.ctrl, h)) return;
    hess_body(T, D, blockIdx.x, threadIdx.x, lds);
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* k_factor: one wave per block of one tree level (blocks first .. first+count-1).             */
/* Tall Cholesky of T = [W ; resMod' ; Ut] (R = d + 1 + nx_ii rows, d columns), left-looking,   */
/* one lane per row:  rows 0..d-1 -> L,  row d -> (L^-1 resMod)',  rows d+1.. -> Ut L^-T.       */
/* Root block (ii == 0): no Ut rows; followed by the backward solve L^-T.                       */
/* ------------------------------------------------------------------------------------------ */
/* (Tried in round 2 and dropped: the tall matrix in registers, row per lane with readlane broadcasts as in the persistent kernels,
 * for R <= 64 and d <= 32: the factor phase of the single-workgroup kernel gained 6 %, the rest of that kernel lost more to the
 * code it added -- a block step there is bound by its global round trips, not by this loop; batching the k loop eight LDS reads
 * at a time: slower.) */
__device__ __forceinline__ void tall_potrf(double *Tm, double *invd, int R, int d, int ld, int lane) {
    for (int j = 0; j < d; j++) {
        /* every row i >= j : s_i = T[i,j] - sum_{k<j} T[i,k] T[j,k] */
        for (int i = j + lane; i < R; i += WAVE) {
            double s = Tm[i + (size_t)j * ld];
            for (int k = 0; k < j; k++) s = fma(-Tm[i + (size_t)k * ld], Tm[j + (size_t)k * ld], s);
            Tm[i + (size_t)j * ld] = s;
        }
        WSYNC();
        const double cjj = Tm[j + (size_t)j * ld];
        const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;      /* pivot <= 0 -> zero column */
        for (int i = j + lane; i < R; i += WAVE) Tm[i + (size_t)j * ld] *= finv;
        if (lane == 0) invd[j] = finv;
        WSYNC();
    }
}

/* sch != nullptr: the backward sweep of all levels is ONE launch (k_factor_all): the Schur complement of a block does not go
 * into the parent's W / resMod in global memory but travels as a record of tagged words -- entry (gi, gj), 1 <= gi <= nx,
 * 0 <= gj <= gi, of [v | S] at gi * (nx + 1) + gj of the block's record (rs doubles per node) -- and the parent subtracts the
 * records of its children from its tall matrix in LDS as they arrive (see factor_w_body in tdunes_wide.hpp). */
__device__ void factor_body(const Tree &T, const Data &D, const Opts &O, int ii, int lane, double *lds, u64 *sch = nullptr, int rs = 0, unsigned tag = 0u) {
    Ctrl *c = D.ctrl;
    const int d = T.bdim[ii], nxi = ii > 0 ? T.nx[ii] : 0;
    const int R = d + 1 + nxi, ld = R | 1;
    double *Tm = lds;                         /* ld x d */
    double *invd = lds + (size_t)ld * d;      /* d */
    const double *W = D.W + T.woff[ii];
    const int bo = T.xoff[T.kid0[ii]];        /* offset of the block vector */
    const double *Ut = D.Ut + T.utoff[ii];

    for (int pass = 0; pass < 2; pass++) {
        for (int e = lane; e < d * d; e += WAVE) {
            const int i = e % d, j = e / d;
            double w = W[i + (size_t)j * d];
            if (i == j && (O.regType == 1 || pass == 1)) w += O.regValue;   /* ddiare */
            Tm[i + (size_t)j * ld] = w;
        }
        for (int j = lane; j < d; j += WAVE) Tm[d + (size_t)j * ld] = D.resMod[bo + j];
        for (int e = lane; e < nxi * d; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            Tm[d + 1 + i + (size_t)j * ld] = Ut[i + (size_t)j * nxi];
        }
        if (sch) {
            WSYNC();
            const int k0 = T.kid0[ii];
            bool dead = false;
            for (int cc = 0, posc = 0; cc < T.nk[ii]; cc++) {
                const int kid = k0 + cc, nxc = T.nx[kid];
                if (kid < T.Np) {
                    const int w = nxc + 1;
                    const u64 *rec = sch + (size_t)kid * rs * 2;
                    for (int f = lane; f < w * w; f += WAVE) {
                        const int gi = f / w, gj = f - gi * w;
                        if (gi < 1 || gj > gi) continue;
                        const double val = wait_tag(rec + (size_t)f * 2, tag, dead);
                        double *dst = gj == 0 ? Tm + d + (size_t)(posc + gi - 1) * ld : Tm + (posc + gi - 1) + (size_t)(posc + gj - 1) * ld;
                        *dst -= val;
                    }
                }
                posc += nxc;
            }
            if (dead) { c->status = 3; __hip_atomic_store(&c->done, 1, RLX, AGENT); }      /* cannot happen: the children were started first */
        }
        WSYNC();
        tall_potrf(Tm, invd, R, d, ld, lane);
        if (O.regType != 2 || pass == 1) break;
        /* on-the-fly Levenberg-Marquardt: any diagonal entry <= regTol -> shift and refactorize */
        int small = 0;
        for (int j = lane; j < d; j += WAVE) small |= (Tm[j + (size_t)j * ld] <= O.regTol);
        if (!__any(small)) break;
        if (lane == 0) atomicAdd(&c->n_reg, 1);
        WSYNC();
    }

    /* outputs: factor, reciprocal diagonal */
    double *L = D.CholW + T.woff[ii];
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * d] = Tm[i + (size_t)j * ld];
    }
    for (int j = lane; j < d; j += WAVE) D.invd[bo + j] = invd[j];

    if (ii > 0) {
        for (int j = lane; j < d; j += WAVE) D.dlam[bo + j] = Tm[d + (size_t)j * ld];
        double *CUt = D.CholUt + T.utoff[ii];
        for (int e = lane; e < nxi * d; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            CUt[i + (size_t)j * nxi] = Tm[d + 1 + i + (size_t)j * ld];
        }
        /* Schur complement into the parent's diagonal sub-block and right-hand side */
        const int dd = T.dad[ii], pos = T.pos[ii], ddim = T.bdim[dd];
        double *Wd = D.W + T.woff[dd];
        for (int e = lane; e < nxi * nxi; e += WAVE) {
            const int i = e % nxi, j = e / nxi;
            if (i < j) continue;
            double acc = 0.0;
            for (int cidx = 0; cidx < d; cidx++) acc = fma(Tm[d + 1 + i + (size_t)cidx * ld], Tm[d + 1 + j + (size_t)cidx * ld], acc);
            if (sch) st_tag(sch + ((size_t)ii * rs + (size_t)(i + 1) * (nxi + 1) + (j + 1)) * 2, acc, tag);
            else Wd[(pos + i) + (size_t)(pos + j) * ddim] -= acc;
        }
        const int xo = T.xoff[ii];
        for (int i = lane; i < nxi; i += WAVE) {
            double acc = 0.0;
            for (int cidx = 0; cidx < d; cidx++) acc = fma(Tm[d + 1 + i + (size_t)cidx * ld], Tm[d + (size_t)cidx * ld], acc);
            if (sch) st_tag(sch + ((size_t)ii * rs + (size_t)(i + 1) * (nxi + 1)) * 2, acc, tag);
            else D.resMod[xo + i] -= acc;
        }
    } else {
        /* root: dlam_0 = L^-T (L^-1 resMod_0); column-oriented back substitution, k descending */
        double *z = Tm + d;                 /* row d, stride ld */
        double pd = 0.0;
        for (int k = d - 1; k >= 0; k--) {
            WSYNC();
            const double zk = z[(size_t)k * ld] * invd[k];
            for (int i = lane; i < k; i += WAVE) z[(size_t)i * ld] = fma(-Tm[k + (size_t)i * ld], zk, z[(size_t)i * ld]);
            WSYNC();
            if (lane == 0) z[(size_t)k * ld] = zk;
        }
        WSYNC();
        for (int j = lane; j < d; j += WAVE) {
            const double v = z[(size_t)j * ld];
            D.dlam[bo + j] = v;
            pd = fma(D.res[bo + j], v, pd);
        }
        pd = wave_sum(pd);
        if (lane == 0) D.part_dot[0] = pd;
    }
}

/* factor_body for NG small blocks of one level AT ONCE in one wave (the single-workgroup kernel, trees whose levels are wider than its 16
 * waves: the chains of a pruned scenario tree are 27 - 40 blocks of 8 x 8 on every level): the wave is split into NG groups of 64 / NG
 * lanes, group g works on block ii0 + g in its own LDS window with factor_body's loops (lane -> lane within the group, stride -> the
 * group's width).  A block step is a chain of LDS and memory round trips around a handful of multiply-adds -- ~8 us whatever the
 * block's size -- and three of them side by side take the time of one.  Per block the arithmetic is factor_body's operation for
 * operation (bit-identical results).  All blocks of a call have the same d and nx (the caller checks), d + 1 + nx <= 64 / NG. */
template <int NG, int DC = 0, int NXC = 0>      /* DC, NXC > 0: the blocks' dimensions, known at compile time (index arithmetic without divisions, loops unrolled) */
__device__ void factor_body_g(const Tree &T, const Data &D, const Opts &O, int ii0, int nblk, int lane, double *lds, int win) {
    constexpr int GW = WAVE / NG;
    Ctrl *c = D.ctrl;
    const int g = lane / GW, l = lane - g * GW;
    const bool act = g < NG && g < nblk;
    const int ii = ii0 + (act ? g : 0);
    const int d = DC > 0 ? DC : T.bdim[ii], nxi = NXC > 0 ? NXC : T.nx[ii];
    const int R = d + 1 + nxi, ld = R | 1;
    double *Tm = lds + (size_t)(g < NG ? g : 0) * win;      /* ld x d */
    double *invd = Tm + (size_t)ld * d;                     /* d */
    const double *W = D.W + T.woff[ii];
    const int bo = T.xoff[T.kid0[ii]];
    const double *Ut = D.Ut + T.utoff[ii];
    bool redo = true;                       /* pass 1 (on-the-fly regularisation) only touches the groups whose block needs it */
    for (int pass = 0; pass < 2; pass++) {
        if (redo) {
            for (int e = l; e < d * d; e += GW) {
                const int i = e % d, j = e / d;
                double w = W[i + (size_t)j * d];
                if (i == j && (O.regType == 1 || pass == 1)) w += O.regValue;   /* ddiare */
                Tm[i + (size_t)j * ld] = w;
            }
            for (int j = l; j < d; j += GW) Tm[d + (size_t)j * ld] = D.resMod[bo + j];
            for (int e = l; e < nxi * d; e += GW) {
                const int i = e % nxi, j = e / nxi;
                Tm[d + 1 + i + (size_t)j * ld] = Ut[i + (size_t)j * nxi];
            }
        }
        WSYNC();
        for (int j = 0; j < d; j++) {           /* tall_potrf, per group */
            if (redo) for (int i = j + l; i < R; i += GW) {
                double s = Tm[i + (size_t)j * ld];
                for (int k = 0; k < j; k++) s = fma(-Tm[i + (size_t)k * ld], Tm[j + (size_t)k * ld], s);
                Tm[i + (size_t)j * ld] = s;
            }
            WSYNC();
            const double cjj = Tm[j + (size_t)j * ld];
            const double finv = cjj > 0.0 ? 1.0 / sqrt(cjj) : 0.0;      /* pivot <= 0 -> zero column */
            if (redo) {
                for (int i = j + l; i < R; i += GW) Tm[i + (size_t)j * ld] *= finv;
                if (l == 0) invd[j] = finv;
            }
            WSYNC();
        }
        if (O.regType != 2 || pass == 1) break;
        /* on-the-fly Levenberg-Marquardt, block by block: any diagonal entry <= regTol -> shift and refactorise THAT block */
        int small = 0;
        for (int j = l; j < d; j += GW) small |= (Tm[j + (size_t)j * ld] <= O.regTol);
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(small != 0);
        const unsigned long long gmask = (GW == 64 ? ~0ull : ((1ull << GW) - 1ull)) << (g < NG ? g * GW : 0);
        redo = g < NG && (bal & gmask) != 0ull;
        if (bal == 0ull) break;
        if (redo && act && l == 0) atomicAdd(&c->n_reg, 1);
        WSYNC();
    }
    if (!act) return;
    /* outputs: factor, reciprocal diagonal */
    double *L = D.CholW + T.woff[ii];
    for (int e = l; e < d * d; e += GW) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * d] = Tm[i + (size_t)j * ld];
    }
    for (int j = l; j < d; j += GW) D.invd[bo + j] = invd[j];
    for (int j = l; j < d; j += GW) D.dlam[bo + j] = Tm[d + (size_t)j * ld];
    double *CUt = D.CholUt + T.utoff[ii];
    for (int e = l; e < nxi * d; e += GW) {
        const int i = e % nxi, j = e / nxi;
        CUt[i + (size_t)j * nxi] = Tm[d + 1 + i + (size_t)j * ld];
    }
    /* Schur complement into the parent's diagonal sub-block and right-hand side.  (Fetching a lane's entries in one batch before updating them
     * -- the loop below is a memory round trip per trip -- measured SLOWER: 235 against 180 us per backward sweep of a 308-node tree; the
     * kernel has no registers to hold a batch in.) */
    const int dd = T.dad[ii], pos = T.pos[ii], ddim = T.bdim[dd];
    double *Wd = D.W + T.woff[dd];
    const int xo = T.xoff[ii];
    for (int e = l; e < nxi * nxi; e += GW) {
        const int i = e % nxi, j = e / nxi;
        if (i < j) continue;
        double acc = 0.0;
        for (int cidx = 0; cidx < d; cidx++) acc = fma(Tm[d + 1 + i + (size_t)cidx * ld], Tm[d + 1 + j + (size_t)cidx * ld], acc);
        Wd[(pos + i) + (size_t)(pos + j) * ddim] -= acc;
    }
    for (int i = l; i < nxi; i += GW) {
        double acc = 0.0;
        for (int cidx = 0; cidx < d; cidx++) acc = fma(Tm[d + 1 + i + (size_t)cidx * ld], Tm[d + (size_t)cidx * ld], acc);
        D.resMod[xo + i] -= acc;
    }
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_factor(Tree T, Data D, Opts O, int first, int h) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (!phase_main(D.ctrl, h)) return;
    factor_body(T, D, O, first + blockIdx.x, threadIdx.x, lds);
}
#endif
/* all levels in one launch: workgroup b takes block Np - 1 - b, so that the children a block waits for were started before it */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_factor_all(Tree T, Data D, Opts O, u64 *sch, int rs, unsigned tag, int h) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (!phase_main(D.ctrl, h)) return;
    factor_body(T, D, O, T.Np - 1 - (int)blockIdx.x, threadIdx.x, lds, sch, rs, tag);
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* k_forward: one wave per block of one level:                                                 */
/*   dlam_ii = L^-T ( y_ii - CholUt_ii' * dlam_dad[pos..] )                                    */
/* ------------------------------------------------------------------------------------------ */
/* fw != nullptr: the forward sweep of all levels is ONE launch (k_forward_all): the step of the parent block arrives as tagged
 * words (children of the root read D.dlam, which k_factor wrote in an earlier launch), and the block's own step is posted the
 * same way.  Everything that does not depend on the parent is fetched before the wait. */
__device__ void forward_body(const Tree &T, const Data &D, int ii, int lane, double *lds, u64 *fw = nullptr, unsigned tag = 0u) {
    const int d = T.bdim[ii], nxi = T.nx[ii], ld = d | 1;
    double *L = lds;                      /* ld x d */
    double *z = lds + (size_t)ld * d;     /* d */
    double *dl = z + d;                   /* nxi : dlam of node ii (inside the parent's block) */
    double *iv = dl + nxi;                /* d : reciprocal diagonal (from global memory it was one round trip per step of the chain below) */
    const int bo = T.xoff[T.kid0[ii]], xo = T.xoff[ii];
    const double *Lg = D.CholW + T.woff[ii];
    for (int e = lane; e < d * d; e += WAVE) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * ld] = Lg[i + (size_t)j * d];
    }
    for (int j = lane; j < d; j += WAVE) iv[j] = D.invd[bo + j];
    if (fw && T.dad[ii] != 0) {
        bool dead = false;
        for (int i = lane; i < nxi; i += WAVE) dl[i] = wait_tag(fw + (size_t)(xo + i) * 2, tag, dead);
        if (dead) { D.ctrl->status = 3; __hip_atomic_store(&D.ctrl->done, 1, RLX, AGENT); }      /* cannot happen: the parent was started first */
    } else {
        for (int i = lane; i < nxi; i += WAVE) dl[i] = D.dlam[xo + i];
    }
    WSYNC();
    const double *CUt = D.CholUt + T.utoff[ii];
    for (int j = lane; j < d; j += WAVE) {
        double acc = 0.0;
        for (int i = 0; i < nxi; i++) acc = fma(CUt[i + (size_t)j * nxi], dl[i], acc);
        z[j] = fma(-1.0, acc, D.dlam[bo + j]);
    }
    for (int k = d - 1; k >= 0; k--) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = lane; i < k; i += WAVE) z[i] = fma(-L[k + (size_t)i * ld], zk, z[i]);
        WSYNC();
        if (lane == 0) z[k] = zk;
    }
    WSYNC();
    double pd = 0.0;
    for (int j = lane; j < d; j += WAVE) {
        if (fw) st_tag(fw + (size_t)(bo + j) * 2, z[j], tag);       /* first: my children wait for it */
        D.dlam[bo + j] = z[j];
        pd = fma(D.res[bo + j], z[j], pd);
    }
    pd = wave_sum(pd);
    if (lane == 0) D.part_dot[ii] = pd;
}

/* forward_body for NG blocks of one level side by side in one wave (see factor_body_g); the partial of res' dlam of every block is taken with the
 * lanes arranged as forward_body has them (entry j in lane j), so that it comes out bit-identical */
template <int NG>
__device__ void forward_body_g(const Tree &T, const Data &D, int ii0, int nblk, int lane, double *lds, int win) {
    constexpr int GW = WAVE / NG;
    const int g = lane / GW, l = lane - g * GW;
    const bool act = g < NG && g < nblk;
    const int ii = ii0 + (act ? g : 0);
    const int d = T.bdim[ii], nxi = T.nx[ii], ld = d | 1;
    double *L = lds + (size_t)(g < NG ? g : 0) * win;      /* ld x d */
    double *z = L + (size_t)ld * d;       /* d */
    double *dl = z + d;                   /* nxi */
    double *iv = dl + nxi;                /* d */
    const int bo = T.xoff[T.kid0[ii]], xo = T.xoff[ii];
    const double *Lg = D.CholW + T.woff[ii];
    for (int e = l; e < d * d; e += GW) {
        const int i = e % d, j = e / d;
        if (i >= j) L[i + (size_t)j * ld] = Lg[i + (size_t)j * d];
    }
    for (int j = l; j < d; j += GW) iv[j] = D.invd[bo + j];
    for (int i = l; i < nxi; i += GW) dl[i] = D.dlam[xo + i];
    WSYNC();
    const double *CUt = D.CholUt + T.utoff[ii];
    for (int j = l; j < d; j += GW) {
        double acc = 0.0;
        for (int i = 0; i < nxi; i++) acc = fma(CUt[i + (size_t)j * nxi], dl[i], acc);
        z[j] = fma(-1.0, acc, D.dlam[bo + j]);
    }
    for (int k = d - 1; k >= 0; k--) {
        WSYNC();
        const double zk = z[k] * iv[k];
        for (int i = l; i < k; i += GW) z[i] = fma(-L[k + (size_t)i * ld], zk, z[i]);
        WSYNC();
        if (l == 0) z[k] = zk;
    }
    WSYNC();
    double term = 0.0;
    for (int j = l; j < d; j += GW) {          /* (d <= GW: one trip) */
        if (act) D.dlam[bo + j] = z[j];
        term = fma(D.res[bo + j], z[j], term);
    }
#pragma unroll
    for (int gg = 0; gg < NG; gg++) {
        double v = __shfl(term, gg * GW + (lane < d ? lane : 0));
        v = lane < d ? v : 0.0;
        const double pd = wave_sum(v);
        if (lane == 0 && gg < nblk) D.part_dot[ii0 + gg] = pd;
    }
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_forward(Tree T, Data D, int first, int h) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (!phase_main(D.ctrl, h)) return;
    forward_body(T, D, first + blockIdx.x, threadIdx.x, lds);
}
#endif
/* all levels below the root in one launch, blocks in BFS order: a block's parent was started before it */
/* the tail of a fused forward sweep (small trees): the direction test and the start of the line search (k_ls_begin) */
__device__ __forceinline__ void fuse_ls_begin(const Tree &T, const Data &D, const Fuse &F, int ii, int lane) {
    if (lane == 0) st_tag(F.red + (size_t)(ii - 1) * 2, D.part_dot[ii], F.tag);
    if (!fuse_last(F, T.Np - 1, lane)) return;
    const double s = fuse_reduce<false>(F.red, 0, T.Np, F.tag, lane, true, D.part_dot[0]);      /* entry 0: the root's, from k_factor */
    if (lane == 0) {
        Ctrl *c = D.ctrl;
        const double dotp = -s;                                     /* :819 */
        c->dot = dotp;
        if (dotp > 1e-10 || !((dotp > 1e-10) || (dotp < 1e-10))) { c->done = 1; c->status = 2; }      /* :951, NaN included */
        else { c->tau = 1.0; c->tauPrev = 0.0; c->ls_iter = 1; c->ls_pending = 1; }
    }
}
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_forward_all(Tree T, Data D, u64 *fw, unsigned tag, int h, Fuse F) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (!phase_main(D.ctrl, h)) return;
    forward_body(T, D, 1 + (int)blockIdx.x, threadIdx.x, lds, fw, tag);
    if (F.on) fuse_ls_begin(T, D, F, 1 + (int)blockIdx.x, threadIdx.x);
}
#endif

/* ------------------------------------------------------------------------------------------ */
/* line-search control (line_search, dual_Newton_tree.c:922-1019)                              */
/* ------------------------------------------------------------------------------------------ */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(256) k_ls_begin(Tree T, Data D, int h) {
    __shared__ double sh[256];
    Ctrl *c = D.ctrl;
    if (!phase_main(c, h)) return;
    const double s = D.strict ? bcast0(threadIdx.x == 0 ? strict_block_dots(T, D.res, D.dlam) : 0.0, sh) : block_reduce<false>(D.part_dot, T.Np, sh);
    if (threadIdx.x == 0) {
        const double dotp = -s;                                     /* :819 */
        c->dot = dotp;
        if (dotp > 1e-10 || !((dotp > 1e-10) || (dotp < 1e-10))) {  /* :951, NaN included */
            c->done = 1; c->status = 2;                             /* TREEQP_DN_NOT_DESCENT_DIRECTION */
        } else {
            c->tau = 1.0; c->tauPrev = 0.0; c->ls_iter = 1; c->ls_pending = 1;
        }
    }
}
#endif

/* Armijo test and iteration bookkeeping for the trial whose dual value is f (line_search :973-1000) */
__device__ void ls_decide_tail(Ctrl *c, int *ls_log, int ls_log_cap, const Opts &O, double f) {
    c->cur ^= 1;                       /* the trial point is now the current point */
    c->fval = f;
    int finished = 0, lsIter = c->ls_iter;
    if (c->restart_counter == O.lsRestartTrigger) finished = 1;                        /* :973 */
    else if (f <= c->fval0 + O.gamma * c->tau * c->dot) finished = 1;                  /* :982 */
    else {
        c->tauPrev = c->tau;
        c->tau = O.beta * c->tauPrev;
        if (lsIter + 1 > O.lsMaxIter) { finished = 1; lsIter = lsIter + 1; }           /* loop exhausted */
        else c->ls_iter = lsIter + 1;
    }
    if (finished) {
        if (lsIter >= O.lsMaxIter) c->restart_counter++; else c->restart_counter = 0;  /* :993-1000 */
        c->ls_pending = 0;
        c->ls_last = lsIter;
        c->ls_total += lsIter;
        if (c->iter < ls_log_cap) ls_log[c->iter] = lsIter;
        c->iter += 1;
        c->fval0 = f;                  /* same point, same sweep => identical to a re-evaluation */
        if (c->iter >= O.maxIter) { c->done = 1; c->status = 1; }                      /* MAXIMUM_ITERATIONS */
    }
}

__device__ void ls_decide_tail(Ctrl *c, const Data &D, const Opts &O, double f) { ls_decide_tail(c, D.ls_log, D.ls_log_cap, O, f); }

/* direction test (:944-954); returns true when the solve must stop with NOT_DESCENT_DIRECTION */
__device__ bool ls_not_descent(Ctrl *c, double dotp) {
    c->dot = dotp;
    const bool bad = (dotp > 1e-10 || !((dotp > 1e-10) || (dotp < 1e-10)));
    if (bad) { c->done = 1; c->status = 2; c->ls_pending = 0; }
    return bad;
}

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(256) k_ls_decide(Tree T, Data D, Opts O, int h, int t, int with_descent_check) {
    __shared__ double sh[256];
    __shared__ int bail;
    Ctrl *c = D.ctrl;
    if (!phase_trial(c, h, t)) return;
    if (with_descent_check) {
        /* fused path: the first trial was evaluated speculatively; test the direction now */
        const double s = D.strict ? bcast0(threadIdx.x == 0 ? strict_block_dots(T, D.res, D.dlam) : 0.0, sh) : block_reduce<false>(D.part_dot, T.Np, sh);
        if (threadIdx.x == 0) bail = ls_not_descent(c, -s);
        __syncthreads();
        if (bail) return;
    }
    const double f = D.strict ? bcast0(threadIdx.x == 0 ? strict_sum(D.fval, T.Nn) : 0.0, sh) : block_reduce<false>(D.fval, T.Nn, sh);
    if (threadIdx.x == 0) ls_decide_tail(c, D, O, f);
}
#endif

/* k_stage with k_fval_init (mode 0) or k_ls_decide (mode 1) as its tail (small trees) */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_stage_f(Tree T, Data D, Opts O, Fuse F, int mode, int h, int t) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    Ctrl *c = D.ctrl;
    if (mode == 1 && !phase_trial(c, h, t)) return;
    const int k = blockIdx.x, lane = threadIdx.x;
    stage_body(T, D, mode, k, lane, lds);
    if (lane == 0) st_tag(F.red + (size_t)k * 2, D.fval[k], F.tag);
    if (!fuse_last(F, T.Nn, lane)) return;
    const double f = fuse_reduce<false>(F.red, 0, T.Nn, F.tag, lane);
    if (lane == 0) {
        if (mode == 0) { c->fval0 = f; c->fval = f; }
        else ls_decide_tail(c, D, O, f);
    }
}
#endif

/* ---- sharded mode (one tree over several devices): rank-local partials and the decision from the
 * gathered per-rank records; sums run in rank order so that every rank takes the same decision ---- */
#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(256) k_shard_pack1(Data D, int nlocal, double *xerr, int rank, int termCondition, int h) {
    __shared__ double sh[256];
    if (!phase_main(D.ctrl, h)) return;
    const double e = (termCondition == 2) ? block_reduce<true>(D.part_err, nlocal, sh) : block_reduce<false>(D.part_err, nlocal, sh);
    if (threadIdx.x == 0) xerr[rank] = e;
}
#endif

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_shard_pack2(Data D, const int *nodes, int n_nodes, const int *blocks, int n_blocks,
                                                     double *xs, int rank, int b0, int bn, int own0, int ownn, int h, int t) {
    const Ctrl *c = D.ctrl;
    if (!phase_trial(c, h, t)) return;
    /* The duals of the boundary nodes live in REPLICATED blocks but each boundary node is staged by its
     * owner only: every rank advances the slices of the boundary nodes it does not own itself (same
     * fma on the same replicated lam / dlam, hence identical values on every rank). */
    {
        const double *lamc = c->cur ? D.lam1 : D.lam0;
        double *lamn = c->cur ? D.lam0 : D.lam1;
        const double step = c->tau - c->tauPrev;
        for (int e = threadIdx.x; e < bn; e += WAVE)
            if (e < own0 || e >= own0 + ownn) lamn[b0 + e] = fma(step, D.dlam[b0 + e], lamc[b0 + e]);
    }
    /* fixed order: lane-strided partials then the shuffle tree */
    double f = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < n_nodes; i += WAVE) f += D.fval[nodes[i]];
    for (int i = threadIdx.x; i < n_blocks; i += WAVE) d += D.part_dot[blocks[i]];
    f = wave_sum(f); d = wave_sum(d);
    if (threadIdx.x == 0) { xs[2 * rank] = f; xs[2 * rank + 1] = d; }
}
#endif

#if TQ_HAS(TQP_HOST)
__global__ void __launch_bounds__(WAVE) k_ls_decide_parts(Data D, Opts O, const double *xs, int nranks, int h, int t, int with_descent_check) {
    Ctrl *c = D.ctrl;
    if (!phase_trial(c, h, t)) return;
    if (threadIdx.x != 0) return;
    double f = 0.0, d = 0.0;
    for (int r = 0; r < nranks; r++) { f += xs[2 * r]; d += xs[2 * r + 1]; }
    if (with_descent_check && ls_not_descent(c, -d)) return;
    ls_decide_tail(c, D, O, f);
}
#endif

#include "tdunes_fast.hpp"
#include "tdunes_persist.hpp"
#include "tdunes_wide.hpp"
#include "tdunes_wide3.hpp"
#include "tdunes_gpersist.hpp"
#include "tdunes_sens.hpp"

}  // namespace tqd
using namespace tqd;

#if TQ_HAS(TQP_HOST)
#include "tdunes_mirror.hpp"
#include "tdunes_rows.hpp"

namespace {

constexpr int EV_RING = 512;     /* solves whose device times can still be asked for */

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; }
};

template <typename T>
T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }

int build_tables(tqgpu_solver *s) {
    const int Nn = s->Nn;
    s->dad.assign(Nn, -1); s->stage.assign(Nn, 0); s->kid0.assign(Nn, -1);
    int cursor = 1;
    for (int i = 0; i < Nn; i++) {
        if (s->nk[i] < 0) return fail(TQGPU_EINVAL, "negative number of children");
        if (s->nk[i] > 0) s->kid0[i] = cursor;
        for (int c = 0; c < s->nk[i]; c++) {
            if (cursor + c >= Nn) return fail(TQGPU_EINVAL, "children counts exceed the number of nodes");
            s->dad[cursor + c] = i;
            s->stage[cursor + c] = s->stage[i] + 1;
        }
        cursor += s->nk[i];
    }
    if (cursor != Nn) return fail(TQGPU_EINVAL, "children counts do not add up to Nn - 1");
    s->Np = 0;
    for (int i = 0; i < Nn; i++) s->Np += s->nk[i] > 0;
    for (int i = 0; i < Nn; i++)
        if ((s->nk[i] > 0) != (i < s->Np)) return fail(TQGPU_EINVAL, "tdunes needs all leaves at the same depth");
    s->Nh = s->stage[Nn - 1];
    s->lvl_first.assign(s->Nh + 2, Nn);
    for (int i = Nn - 1; i >= 0; i--) s->lvl_first[s->stage[i]] = i;
    s->lvl_first[s->Nh + 1] = Nn;

    s->xoff.assign(Nn + 1, 0); s->uoff.assign(Nn + 1, 0); s->aoff.assign(Nn + 1, 0); s->boff.assign(Nn + 1, 0);
    s->pos.assign(Nn, 0); s->bdim.assign(Nn, 0); s->woff.assign(Nn + 1, 0); s->utoff.assign(Nn + 1, 0);
    for (int k = 0; k < Nn; k++) {
        if (s->nx[k] < 0 || s->nu[k] < 0) return fail(TQGPU_EINVAL, "negative dimension");
        s->xoff[k + 1] = s->xoff[k] + s->nx[k];
        s->uoff[k + 1] = s->uoff[k] + s->nu[k];
        if (k > 0) {
            s->aoff[k + 1] = s->aoff[k] + s->nx[k] * s->nx[s->dad[k]];
            s->boff[k + 1] = s->boff[k] + s->nx[k] * s->nu[s->dad[k]];
            int first = s->kid0[s->dad[k]];
            for (int j = first; j < k; j++) s->pos[k] += s->nx[j];     /* dual_Newton_tree.c:177-194 */
        }
        int d = 0;
        for (int c = 0; c < s->nk[k]; c++) d += s->nx[s->kid0[k] + c];
        s->bdim[k] = d;
        s->woff[k + 1] = s->woff[k] + d * d;
        s->utoff[k + 1] = s->utoff[k] + (k > 0 ? s->nx[k] * d : 0);
    }
    s->nx0 = s->nx[0];
    s->sum_nx = s->xoff[Nn]; s->sum_nu = s->uoff[Nn]; s->sum_lam = s->sum_nx - s->nx0;
    s->sum_A = s->aoff[Nn]; s->sum_B = s->boff[Nn]; s->sum_W = s->woff[Nn]; s->sum_Ut = s->utoff[Nn];

    /* LDS budgets of the wave-per-block kernels */
    s->pp.lds_stage = s->pp.lds_hess = s->pp.lds_factor = s->pp.lds_forward = 0;
    for (int k = 0; k < Nn; k++) {
        const size_t d = s->bdim[k], nz = s->nx[k] + s->nu[k];
        s->pp.lds_stage = std::max(s->pp.lds_stage, (d + s->nx[k] + 2 * (s->nx[k] + s->nu[k]) + 2) * sizeof(double));
        if (k < s->Np) {
            s->pp.lds_hess = std::max(s->pp.lds_hess, (2 * d * nz + 2) * sizeof(double));
            const size_t R = d + 1 + (k > 0 ? s->nx[k] : 0), ld = R | 1;
            s->pp.lds_factor = std::max(s->pp.lds_factor, (ld * d + d + 2) * sizeof(double));
            s->pp.lds_forward = std::max(s->pp.lds_forward, ((d | 1) * d + 2 * d + s->nx[k] + 2) * sizeof(double));
        }
    }
    {
        int dmax = 0, rmax = 0, nzmax = 0;
        for (int k = 0; k < s->Np; k++) {
            const int d = s->bdim[k], nxi = k > 0 ? s->nx[k] : 0, nz = s->nx[k] + s->nu[k];
            dmax = std::max(dmax, d); rmax = std::max(rmax, wide_rows(d, nxi)); nzmax = std::max(nzmax, nz);
            s->pp.lds_hess_w = std::max(s->pp.lds_hess_w, wide_lds_hess(d, nz));
            s->pp.lds_factor_w = std::max(s->pp.lds_factor_w, wide_lds_factor(d, nxi));
            s->pp.lds_forward_w = std::max(s->pp.lds_forward_w, wide_lds_forward(d));
        }
        s->pp.wide_small = false;
        s->pp.wide = dmax > 16 && dmax <= 64 && rmax <= 128 && nzmax <= 32;      /* k_hess_w keeps a parent's entries of P for 8 k-steps of 4 in registers */
        /* Trees of SMALL blocks (d <= 16) that are too wide for the single-workgroup kernel (a level of more than 6 x 16 blocks) take the
         * workgroup-per-block kernels as well: three launches per Newton iteration instead of the five to eight of the launch-per-phase
         * kernels (TREEQP_AMD_SMALL_WIDE=0: as before) */
        {
            int widest = 0;
            for (int l = 0; l + 1 < (int)s->lvl_first.size(); l++) widest = std::max(widest, s->lvl_first[l + 1] - s->lvl_first[l]);
            if (!s->pp.wide && dmax >= 3 && dmax <= 16 && widest > 6 * 16 && rmax <= 128 && nzmax <= 32 && s->sw.small_wide) s->pp.wide = s->pp.wide_small = true;
        }
    }
    const size_t lim = 160 * 1024;
    if (s->pp.lds_factor > lim || s->pp.lds_hess > lim || s->pp.lds_forward > lim)
        return fail(TQGPU_EUNSUPPORTED, "dual Hessian block too large for the LDS-resident kernels (160 KiB per workgroup)");
    return TQGPU_OK;
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return TQGPU_OK;
}


/* level `level` of a uniform tree with MD children per parent: the index of its first node, and its width */
int uni_first(int MD, int level) { int n = 0, w = 1; for (int l = 0; l < level; l++) { n += w; w *= MD; } return n; }
int uni_width(int MD, int level) { int w = 1; for (int l = 0; l < level; l++) w *= MD; return w; }

/* the branching part of a uniform tree: block levels 0 .. top-1 grouped bottom-up into tiers of TH levels, the top tier takes the rest;
 * the grid of a tier is the width of its first level */
struct UniTier { int l0, l1, grid; };
std::vector<UniTier> uni_tiers(int top, int TH, int MD) {
    std::vector<UniTier> out;
    for (int l1 = top; l1 > 0;) {
        const int l0 = std::max(0, l1 - TH);
        out.push_back({l0, l1, uni_width(MD, l0)});
        l1 = l0;
    }
    return out;
}
void add_tier(tqgpu_solver *s, int l0, int l1, int grid, int chain) {
    s->uni.tier_l0.push_back(l0); s->uni.tier_l1.push_back(l1); s->uni.tier_grid.push_back(grid); s->uni.tier_chain.push_back(chain);
}
/* the table line a mirror's fused routes run with (tdunes_rows.hpp): its index, its shape and its LDS sizes; nullptr: none, generic path only */
void use_row(tqgpu_solver *s, const ShapeRow *row) {
    s->uni.row = row; s->uni.fast = row ? row->idx : -1;
    if (row) { s->uni.fNX = row->nx; s->uni.fNU = row->nu; s->uni.fMD = row->md; s->uni.lds_fast = row->tier_lds; s->uni.lds_fstage = row->stage_lds; }
}

/* multistage tree?  (setup_multistage_tree(md, Nr, Nh) with 1 <= Nr < Nh: every node above stage Nr has md
 * children, every parent from stage Nr on has one; uniform nx, nu) */
void detect_multistage(tqgpu_solver *s) {
    s->uni.mstage = false;
    const int Nn = s->Nn, NX = s->nx[0], NU = s->nu[0], MD = s->nk[0], Nh = s->Nh;
    if (Nh < 2 || MD < 2 || NX % 4 != 0) return;
    int Nr = 0;
    while (Nr < Nh) {
        bool all = true;
        for (int k = s->lvl_first[Nr]; k < s->lvl_first[Nr + 1]; k++) if (s->nk[k] != MD) { all = false; break; }
        if (!all) break;
        Nr++;
    }
    if (Nr < 1 || Nr >= Nh) return;
    for (int k = 0; k < Nn; k++) {
        if (s->nx[k] != NX) return;
        if (k < s->Np) { if (s->nu[k] != NU) return; if (k >= s->lvl_first[Nr] && s->nk[k] != 1) return; }
        else if (s->nu[k] != 0) return;
    }
    const ShapeRow *row = find_row(MSTAGE_ROWS, NX, NU, MD);
    if (!row) return;
    const int S = uni_width(MD, Nr);
    use_row(s, row);
    s->uni.mstage = true; s->uni.ms_Nr = Nr; s->uni.ms_S = S; s->uni.ms_nB = s->lvl_first[Nr];
    const int TH = row->TH;
    s->uni.tier_l0.clear(); s->uni.tier_l1.clear(); s->uni.tier_grid.clear(); s->uni.tier_chain.clear();
    /* chain part bottom-up in tiers of at most 8 levels (Uni<..., 1>::TH), then the branching part in tiers of TH levels */
    for (int l1 = Nh; l1 > Nr;) {
        const int l0 = std::max(Nr, l1 - 8);
        add_tier(s, l0, l1, S, 1);
        l1 = l0;
    }
    for (const UniTier &t : uni_tiers(Nr, TH, MD)) add_tier(s, t.l0, t.l1, t.grid, 0);
    s->uni.n_tiers = (int)s->uni.tier_l0.size();
}

/* uniform complete tree? (every node nx, every parent nu + md children, one leaf depth) */
void detect_fast(tqgpu_solver *s) {
    use_row(s, nullptr);
    const int Nn = s->Nn, NX = s->nx[0], NU = s->nu[0], MD = s->nk[0];
    if (s->Nh < 2 || MD < 2) return;
    for (int k = 0; k < Nn; k++) {
        if (s->nx[k] != NX) return;
        if (k < s->Np) { if (s->nu[k] != NU || s->nk[k] != MD) return; }
        else if (s->nu[k] != 0) return;
    }
    const ShapeRow *row = find_row(FAST_ROWS, NX, NU, MD);
    if (!row) return;
    use_row(s, row);
    s->uni.tier_l0.clear(); s->uni.tier_l1.clear(); s->uni.tier_grid.clear(); s->uni.tier_chain.clear();
    for (const UniTier &t : uni_tiers(s->Nh, row->TH, MD)) add_tier(s, t.l0, t.l1, t.grid, 0);
    s->uni.n_tiers = (int)s->uni.tier_l0.size();
}

/* the sharded modes' part in the launches per tier and in tqgpu_destroy (tdunes_shard.hpp) */
Shard shard_desc(const tqgpu_solver *s, int tier); int shard_exchange(tqgpu_solver *s, int which); void shard_release(tqgpu_solver *s);

/* One fused Newton iteration, split in three phases around the two exchange points of the sharded
 * mode.  Single device: phases run back to back, no exchange. */
void launch_fast_phase(tqgpu_solver *s, const Opts &O, int h, int phase, int &launches) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    const dim3 blk(FW * WAVE);
    const int nt = s->uni.n_tiers, N = s->shard.nranks;
    const bool sharded = s->shard.on;
    const int P = sharded ? s->shard.part_top : -1;
    auto tgrid = [&](int i) { return (sharded && i <= P) ? s->uni.tier_grid[i] / N : s->uni.tier_grid[i]; };
    /* which kernel runs first / performs the termination test */
    const int check_tier = sharded ? P + 1 : 1;          /* index in 0..nt-1 (nt-1 = top) */
    const int nparts = sharded ? N : (nt > 1 ? s->uni.tier_grid[0] : FW);
    const int n_stage = sharded ? s->shard.n_nodes : T.Nn;
    const ShapeRow &K = *s->uni.row;
    if (phase == 0) {
        for (int i = 0; i < nt - 1 && (!sharded || i <= P); i++) {
            hipLaunchKernelGGL(K.back, dim3(tgrid(i)), blk, s->uni.lds_fast, st, T, D, O, shard_desc(s, i),
                               s->uni.tier_l0[i], s->uni.tier_l1[i], i == 0, !sharded && i == check_tier, nparts, i, h); launches++;
        }
        if (sharded) { hipLaunchKernelGGL(k_shard_pack1, dim3(1), dim3(256), 0, st, D, tgrid(0), s->shard.d_xerr, s->shard.rank, O.termCondition, h); launches++; }
    }
    if (phase == 1) {
        for (int i = (sharded ? P + 1 : nt - 1); i < nt - 1; i++) {
            hipLaunchKernelGGL(K.back, dim3(tgrid(i)), blk, s->uni.lds_fast, st, T, D, O, shard_desc(s, i),
                               s->uni.tier_l0[i], s->uni.tier_l1[i], 0, i == check_tier, nparts, i, h); launches++;
        }
        hipLaunchKernelGGL(K.top, dim3(1), blk, s->uni.lds_fast, st, T, D, O, shard_desc(s, nt - 1),
                           s->uni.tier_l1[nt - 1], nt == 1, (nt - 1) == check_tier, nparts, nt - 1, h); launches++;
        for (int i = nt - 2; i >= 0; i--) {
            hipLaunchKernelGGL(K.fwd, dim3(tgrid(i)), blk, s->uni.lds_fast, st, T, D, O, shard_desc(s, i),
                               s->uni.tier_l0[i], s->uni.tier_l1[i], nt + (nt - 2 - i), h); launches++;
        }
        hipLaunchKernelGGL(K.stage, dim3((n_stage + FW - 1) / FW), blk, s->uni.lds_fstage, st, T, D, O,
                           sharded ? s->shard.d_node_list : nullptr, n_stage, 2 * nt - 1, h, 1); launches++;
        if (sharded) { hipLaunchKernelGGL(k_shard_pack2, dim3(1), dim3(WAVE), 0, st, D, s->shard.d_node_cnt_list, s->shard.n_nodes_counted,
                                          s->shard.d_blk_list, s->shard.n_blk_counted, s->shard.d_xs, s->shard.rank, s->shard.bnd_b0, s->shard.bnd_bn, s->shard.bnd_own0, s->shard.bnd_ownn, h, 1); launches++; }
    }
    if (phase == 2) {
        if (sharded) hipLaunchKernelGGL(k_ls_decide_parts, dim3(1), dim3(WAVE), 0, st, D, O, s->shard.d_xs, N, h, 1, 1);
        else hipLaunchKernelGGL(k_ls_decide, dim3(1), dim3(256), 0, st, T, D, O, h, 1, 1);
        launches++;
    }
}

int launch_fast_iteration(tqgpu_solver *s, const Opts &O, int h, int &launches) {
    launch_fast_phase(s, O, h, 0, launches);
    if (s->shard.on) { int rc = shard_exchange(s, 1); if (rc) return rc; }
    launch_fast_phase(s, O, h, 1, launches);
    if (s->shard.on) { int rc = shard_exchange(s, 2); if (rc) return rc; }
    launch_fast_phase(s, O, h, 2, launches);
    return TQGPU_OK;
}

/* one more line-search trial of iteration `it`; phase 0: sweep (+ pack), phase 1: decide */
/* the next tag of a family of tagged words: counts up and skips 0, the value of a word never written */
static unsigned next_tag(unsigned &epoch) { if (++epoch == 0) epoch = 1; return epoch; }
static Fuse next_fuse(tqgpu_solver *s) {
    Fuse F; F.red = s->pp.fuse_red; F.cnt = s->pp.fuse_cnt; F.on = 1;
    F.tag = next_tag(s->pp.fuse_epoch);
    return F;
}
static Fuse no_fuse() { Fuse F; F.red = nullptr; F.cnt = nullptr; F.tag = 0; F.on = 0; return F; }
static W3 next_w3(tqgpu_solver *s) {
    W3 w; w.xu = s->w3.xu; w.red = s->w3.red; w.cnt = s->w3.cnt; w.sum_nx = s->sum_nx; w.lds_wave = (int)((s->pp.lds_stage + 7) / 8);
    w.hm = nullptr;
    s->w3.tail_sg = false;
    w.tag = next_tag(s->w3.epoch);
    return w;
}
/* one stage sweep of the launch-per-phase route, by the stage solver the tree's nodes need (general constraints / box bounds / clipping
 * and dense unconstrained): the one place that picks among the three */
static void launch_stage_sweep(tqgpu_solver *s, int mode, int h, int t) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    if (s->sk.gen) hipLaunchKernelGGL(k_stage_gen, dim3(T.Nn), dim3(WAVE), s->sk.lds_gen, st, T, D, mode, h, t);
    else if (s->sk.box) hipLaunchKernelGGL(k_stage_box, dim3(T.Nn), dim3(WAVE), s->sk.lds_box, st, T, D, mode, h, t);
    else hipLaunchKernelGGL(k_stage, dim3(T.Nn), dim3(WAVE), s->pp.lds_stage, st, T, D, mode, h, t);
}
static void launch_sg(tqgpu_solver *s, const Opts &O, int mode, int h, int t, bool fresh = false) {
    W3 w = next_w3(s);
    /* (a post is ~14 system-scope stores to host memory and the wait for their acknowledgements, on the launch's critical path: only
     * where the host is going to look) */
    if (s->w3.mirror && s->w3.post_next) { w.hm = s->h_res; s->w3.wait = w.tag; s->w3.tail_sg = true; }
    s->w3.post_next = false;
    if (s->w3.sgp) {
        if (mode == 2) { SgpFwdYes fa; fa.anc = s->w3.d_anc; fa.pdw = s->w3.d_pdw; hipLaunchKernelGGL(k_sgp_t<true>, dim3(s->T.Np), dim3(WT), s->w3.lds_sgp, s->stream, s->T, s->D, O, w, mode, h, t, s->w3.sgp_accs, (const double *)nullptr, fa); }
        else hipLaunchKernelGGL(k_sgp_t<false>, dim3(s->T.Np), dim3(WT), s->w3.lds_sgp, s->stream, s->T, s->D, O, w, mode, h, t, s->w3.sgp_accs, fresh ? (const double *)s->d_lam_init : (const double *)nullptr, SgpFwdNo());
        return;
    }
    const int grid = (s->T.Nn + SG_WAVES - 1) / SG_WAVES;
    hipLaunchKernelGGL(k_sg, dim3(grid), dim3(SG_WAVES * WAVE), SG_WAVES * ((s->pp.lds_stage + 7) / 8) * 8, s->stream, s->T, s->D, O, w, mode, h, t);
}

void launch_trial_phase(tqgpu_solver *s, const Opts &O, Route r, int it, int t, int phase, int &launches) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    const bool sharded = s->shard.on;
    if (phase == 0) {
        bool done = false;
        if (r == Route::TIERED) {
            const int n_stage = sharded ? s->shard.n_nodes : T.Nn;
            hipLaunchKernelGGL(s->uni.row->stage, dim3((n_stage + FW - 1) / FW), dim3(FW * WAVE), s->uni.lds_fstage, st, T, D, O, sharded ? s->shard.d_node_list : nullptr, n_stage, 7, it, t);
            done = true;
        }
        if (!done && r == Route::THREE_LAUNCH) { launch_sg(s, O, 1, it, t); done = true; }      /* with the Armijo test and the next termination test as its tail */
        if (!done) {
            if (r == Route::FUSED_TAILS) hipLaunchKernelGGL(k_stage_f, dim3(T.Nn), dim3(WAVE), s->pp.lds_stage, st, T, D, O, next_fuse(s), 1, it, t);      /* with k_ls_decide as its tail */
            else launch_stage_sweep(s, 1, it, t);
        }
        launches++;
        if (sharded) { hipLaunchKernelGGL(k_shard_pack2, dim3(1), dim3(WAVE), 0, st, D, s->shard.d_node_cnt_list, s->shard.n_nodes_counted, s->shard.d_blk_list, s->shard.n_blk_counted, s->shard.d_xs, s->shard.rank, s->shard.bnd_b0, s->shard.bnd_bn, s->shard.bnd_own0, s->shard.bnd_ownn, it, t); launches++; }
    } else {
        if (sharded) { hipLaunchKernelGGL(k_ls_decide_parts, dim3(1), dim3(WAVE), 0, st, D, O, s->shard.d_xs, s->shard.nranks, it, t, 0); launches++; }
        else if (r != Route::FUSED_TAILS && r != Route::THREE_LAUNCH) { hipLaunchKernelGGL(k_ls_decide, dim3(1), dim3(256), 0, st, T, D, O, it, t, 0); launches++; }
    }
}

int launch_trial(tqgpu_solver *s, const Opts &O, Route r, int it, int t, int &launches) {
    launch_trial_phase(s, O, r, it, t, 0, launches);
    if (s->shard.on) { int rc = shard_exchange(s, 2); if (rc) return rc; }
    launch_trial_phase(s, O, r, it, t, 1, launches);
    return TQGPU_OK;
}


/* THE list of process-lifetime switches: read from the environment once, when the first of them is asked for */
struct ProcessSwitches { int nap_t1, nap, ls_chunk, trial_batch; bool has_nap; };
static const ProcessSwitches &process_switches() {
    static const ProcessSwitches w = [] {
        auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        ProcessSwitches p;
        p.nap_t1 = num("TREEQP_AMD_NAP_T1", 128);                             /* workgroups of a launch from which the bottom tier's long poll naps are on (nap_for_grid) */
        p.has_nap = getenv("TREEQP_AMD_NAP") != nullptr; p.nap = num("TREEQP_AMD_NAP", 0);      /* ... of a batch launch off (0) / on (1) instead (launch_persist_batch) */
        p.ls_chunk = std::max(1, num("TREEQP_AMD_LS_CHUNK", 2));              /* iterations enqueued per read-back after a solve that backtracked (solve_end) */
        p.trial_batch = std::max(1, num("TREEQP_AMD_TRIAL_BATCH", 3));        /* line-search trials in the first batch beyond the first trial (solve_end) */
        return p;
    }();
    return w;
}

/* persistent launch: geometry, sync words, co-residency test */
/* poll naps by launch size (PollGuard::go_on) */
static int nap_for_grid(int workgroups) { return workgroups > process_switches().nap_t1 ? 1 : 0; }
/* workgroups per CU of the three builds of a persistent kernel at `lds` bytes of LDS each; the build for one workgroup per CU is allowed that much
 * LDS here, and counts 0 where it cannot have it or cannot be asked */
static int persist_occupancy(const PersistKernels &k, size_t lds, int &per_cu, int &per_cu_r, int &per_cu_one) {
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.plain, FW * WAVE, lds));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_r, k.reuse, FW * WAVE, lds));
    if (allow_lds(k.one, lds) != TQGPU_OK || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_one, k.one, FW * WAVE, lds) != hipSuccess) per_cu_one = 0;
    return TQGPU_OK;
}
int setup_persist(tqgpu_solver *s) {
    s->persist.ok = false;
    if (s->uni.fast < 0 || s->uni.n_tiers > 8) return TQGPU_OK;
    PGeom &G = s->persist.geom;
    G.n_tiers = s->uni.n_tiers;
    int wg = 0;
    for (int i = 0; i < s->uni.n_tiers; i++) { G.l0[i] = s->uni.tier_l0[i]; G.l1[i] = s->uni.tier_l1[i]; G.grid[i] = s->uni.tier_grid[i]; G.chain[i] = s->uni.tier_chain[i]; G.wg0[i] = wg; wg += s->uni.tier_grid[i]; }
    G.G = wg;
    int per_cu = 0, per_cu_r = 1 << 20, per_cu_one = 0;      /* _r: the variant that can keep factors (checkLastActiveSet == 2); _one: the build for one workgroup per CU */
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, s->device));
    const ShapeRow &K = *s->uni.row;
    const PersistKernels &kernels = s->uni.mstage ? K.mpersist : K.persist;
    s->persist.lds = s->uni.mstage ? std::max(K.persist_lds, K.chain_lds) : K.persist_lds;
    if (int rc = persist_occupancy(kernels, s->persist.lds, per_cu, per_cu_r, per_cu_one)) return rc;
    if (s->sw.has_lds_pad) {      /* experiment: force fewer workgroups per CU */
        s->persist.lds += (size_t)s->sw.lds_pad * 1024;
        if (!s->uni.mstage) { allow_lds(K.persist.plain, s->persist.lds); HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K.persist.plain, FW * WAVE, s->persist.lds)); }
    }
    /* every workgroup must be resident at once (they wait for each other); keep one block per CU of
     * margin against the occupancy query over-reporting (MI355X guide, "Residency and cooperative launch") */
    per_cu = std::min(per_cu, per_cu_r);
    /* one workgroup per CU needs no margin (the figure is exact when registers allow a single 4-wave workgroup);
     * with more per CU keep half a CU-load of workgroups in hand */
    /* (rounds 1 - 2 kept half a CU-load in hand; the admission rule of the MI355X guide -- min(API answer, 8, 800 / (sgpr rounded up to
     * 16 + 16)) per CU -- is what per_cu_r holds, the grid is admitted CU by CU, and a launch that is not resident after all ends in the
     * bounded waits' timeout and the launch-per-tier redo, not in a hang: no margin.  C2 batched: 5 trees 99 k it/s -> 7 trees 133 k.) */
    const int margin = s->sw.capacity_margin;      /* experiment */
    const int capacity = per_cu <= 1 ? prop.multiProcessorCount * per_cu : prop.multiProcessorCount * per_cu - margin;
    if (s->sw.verbose) fprintf(stderr, "[treeqp_amd] persistent path: %d workgroups, %d per CU possible, capacity %d\n", G.G, per_cu, capacity);
    s->persist.co_capacity = std::max(1, capacity);
    s->n_cu = prop.multiProcessorCount;
    /* the build for ONE workgroup per CU (f_persist_one: more registers, 2 % faster) when the launch fits the device that way */
    s->persist.one = per_cu_one >= 1 && G.G <= prop.multiProcessorCount * std::min(per_cu_one, 1) && !s->sw.no_persist_one;
    if (per_cu < 1 || G.G > capacity) return TQGPU_OK;
    /* hand-over buffers (tagged 64-bit words, see tdunes_persist.hpp); zeroed once, never reset */
    const int nx0 = s->nx[0];
    const size_t n_sch = (size_t)s->Nn * (nx0 * nx0 + nx0) * 2, n_dlt = (size_t)s->sum_nx * 2, n_ndt = (size_t)s->Nn * 2 * nx0 * 2;
    const size_t n_parts = (size_t)G.G * 4, n_errs = (size_t)G.G * 2;
    const size_t n_bparts = (size_t)G.G * 16;
    const size_t n_sgt = (size_t)s->Nn * 2, n_rfl = (size_t)s->Nn * 2;      /* active-set signature / reuse flag of a tier subtree root (one tagged double each) */
    const size_t n_verdict = 16;
    const size_t n_anc = (size_t)s->Np * (size_t)(nx0 * s->uni.fMD) * (nx0 + 1) * 2;      /* forward records [z0 | M] of the blocks, for the bottom tier's walk down its path (tdunes_persist.hpp, p_forward_tier) */
    const size_t bytes = (n_sch + n_dlt + n_ndt + n_parts + n_errs + 32 + n_bparts + n_sgt + n_rfl + n_verdict + n_anc) * sizeof(unsigned long long);
    if (int rc = s->mem.zeroed(s->persist.sync_slab, bytes, TQGPU_ENODEVICE, "the hand-over slab")) return rc;
    HIP_TRY(hipDeviceSynchronize());          /* (a device memset may return before it has happened, and the solver's non-blocking stream does not wait for the null stream) */
    s->persist.sync_bytes = bytes;
    unsigned long long *w = static_cast<unsigned long long *>(s->persist.sync_slab);
    s->persist.psync.sch = w; s->persist.psync.dlt = w + n_sch; s->persist.psync.ndt = s->persist.psync.dlt + n_dlt; s->persist.psync.parts = s->persist.psync.ndt + n_ndt;
    s->persist.psync.errs = s->persist.psync.parts + n_parts;
    s->persist.psync.halt = reinterpret_cast<unsigned *>(s->persist.psync.errs + n_errs);
    s->persist.psync.timeout = s->persist.psync.halt + 32;
    s->persist.psync.cmd = s->persist.psync.errs + n_errs + 24;          /* same 256-byte block: halt | timeout | cmd | vrd */
    s->persist.psync.vrd = s->persist.psync.errs + n_errs + 28;
    s->persist.psync.bparts = s->persist.psync.errs + n_errs + 32;
    s->persist.psync.sgt = s->persist.psync.bparts + n_bparts; s->persist.psync.rfl = s->persist.psync.sgt + n_sgt;
    s->persist.psync.verdict = s->persist.psync.rfl + n_rfl;
    s->persist.psync.anc = s->persist.psync.verdict + n_verdict;
    s->persist.psync.base = w; s->persist.psync.npeer = 1; s->persist.psync.relay_wg = -1; s->persist.psync.anc_local = 1;
    for (int r = 0; r < 8; r++) s->pshard.h_peers[r] = w;
    if (int rc = s->mem.upload(s->pshard.d_peers, s->pshard.h_peers, sizeof(s->pshard.h_peers), TQGPU_ENODEVICE, "the table of peer slabs")) return rc;
    s->persist.psync.peers = s->pshard.d_peers;
    s->persist.psync.seq = 0; s->persist.psync.trip = 0;
    s->persist.psync.nap = s->sw.has_nap ? s->sw.nap : nap_for_grid(G.G);
    /* XCD-aware placement: the hardware deals workgroups round-robin over the 8 XCDs (workgroup b -> XCD b % 8)
     * and every XCD has its own L2.  A tier subtree talks to its parent and its children only, so whole
     * families go to one XCD: each subtree of the lowest tier with at most 8 subtrees picks an XCD, everything
     * below follows its ancestor there; the tiers above (one workgroup each, typically) take what is left. */
    {
        const int NXCD = 8, Gn = G.G;
        int anchor = s->uni.n_tiers - 1;
        for (int i = 0; i < s->uni.n_tiers; i++) if (G.grid[i] <= NXCD) { anchor = i; break; }
        std::vector<std::vector<int>> want(NXCD);
        std::vector<int> rest;
        for (int i = 0; i < s->uni.n_tiers; i++)
            for (int q = 0; q < G.grid[i]; q++) {
                const int id = G.wg0[i] + q;
                if (i <= anchor) want[(int)((long long)q * G.grid[anchor] / G.grid[i]) % NXCD].push_back(id);   /* subtree q of tier i sits under subtree q*grid[anchor]/grid[i] */
                else rest.push_back(id);
            }
        std::vector<int> map((size_t)Gn, -1);
        std::vector<size_t> next(NXCD, 0);
        for (int b = 0; b < Gn; b++) { auto &w = want[b % NXCD]; if (next[b % NXCD] < w.size()) map[b] = w[next[b % NXCD]++]; }
        for (int x = 0; x < NXCD; x++) for (size_t k = next[x]; k < want[x].size(); k++) rest.push_back(want[x][k]);
        size_t r = 0;
        for (int b = 0; b < Gn; b++) if (map[b] < 0) map[b] = rest[r++];
        /* more workgroups than CUs (two per CU): the workgroups dispatched last share a CU with an earlier one.  Let those be
         * the UPPER tiers -- they work while the bottom tier waits and vice versa -- instead of two bottom-tier subtrees
         * halving each other on the critical path: plain tier order (bottom tier first). */
        if (Gn > prop.multiProcessorCount) for (int b = 0; b < Gn; b++) map[b] = b;
        if (int rc = s->mem.upload(s->persist.wg_map, map.data(), sizeof(int) * (size_t)Gn, TQGPU_ENODEVICE, "the workgroup placement")) return rc;
        G.wg_of_block = s->persist.wg_map;
    }
    /* packed constants + the start/end view of the mirror */
    const int nz = nx0 + s->nu[0];
    const size_t n_ab = (size_t)(s->Nn - 1) * nx0 * nz, n_cst = (size_t)s->Nn * 16 * 5;
    if (int rc = s->mem.device(s->persist.pconst_slab, (n_ab + n_cst) * sizeof(double) + sizeof(PDump) + 256, TQGPU_ENODEVICE, "the packed constants")) return rc;
    double *pc = static_cast<double *>(s->persist.pconst_slab);
    s->persist.pab = pc; s->persist.pcst = pc + n_ab;
    PDump hd;
    const Data &D = s->D;
    hd.x = D.x; hd.u = D.u; hd.xUnc = D.xUnc; hd.uUnc = D.uUnc; hd.xUncS = D.xUncS; hd.uUncS = D.uUncS; hd.qmod = D.qmod; hd.rmod = D.rmod; hd.QinvCal = D.QinvCal; hd.RinvCal = D.RinvCal;
    hd.lam0 = D.lam0; hd.lam1 = D.lam1; hd.dlam = D.dlam; hd.lam_init = s->d_lam_init; hd.stamps = D.stamps; hd.ls_log = D.ls_log; hd.ls_log_cap = D.ls_log_cap;
    hd.hres = s->h_res;
    PDump *dd = reinterpret_cast<PDump *>(pc + n_ab + n_cst);
    HIP_TRY(hipMemcpy(dd, &hd, sizeof(PDump), hipMemcpyHostToDevice));
    s->persist.pconst.AB = s->persist.pab; s->persist.pconst.b = D.b; s->persist.pconst.cst = s->persist.pcst; s->persist.pconst.ctrl = D.ctrl; s->persist.pconst.dump = dd; s->persist.pconst.lam0_src = s->d_lam_init; s->persist.pconst.Np = s->Np;
    s->persist.pconst.S = s->uni.mstage ? s->uni.ms_S : 0; s->persist.pconst.nB = s->uni.mstage ? s->uni.ms_nB : s->Np; s->persist.pconst.Nr = s->uni.mstage ? s->uni.ms_Nr : s->Nh;
    s->persist.need_pack = true;
    s->persist.ok = true;
    return TQGPU_OK;
}

/* one persistent launch (prologue = first sweep of the solve + control block reset): no memset, the
 * hand-over words are told apart by the launch number in their tags */
/* the 16-bit launch number of a mirror's single launches (f_persist*, g_persist*): the tag of the hand-over words and of the result block,
 * never 0.  launch_no_after: 0 when the number wraps; step_launch_no: takes the next number and says whether it wrapped */
static unsigned launch_no_after(unsigned n) { return (n + 1) & 0xFFFFu; }
static bool step_launch_no(tqgpu_solver *s) {
    s->persist.launch_no = launch_no_after(s->persist.launch_no);
    if (s->persist.launch_no != 0) return false;
    s->persist.launch_no = 1;
    return true;
}

int launch_persist(tqgpu_solver *s, const Opts &O, int &launches, int prologue, unsigned batch_seq = 0) {
    const Data &D = s->D; hipStream_t st = s->stream;
    if (batch_seq) s->persist.launch_no = batch_seq >> 16;          /* part of a batch launch: the caller chose the number (and wiped the buffers if it wrapped) */
    else if (step_launch_no(s)) {
        /* the 16-bit launch number wraps: words that are not rewritten by every launch (the line-search command / verdict /
         * batch partials) could still carry a tag of 65535 launches ago -- wipe the hand-over buffers (stream-ordered) */
        HIP_TRY(hipMemsetAsync(s->persist.sync_slab, 0, s->persist.sync_bytes, st));
    }
    s->persist.psync.seq = s->persist.launch_no << 16;
    if (s->persist.need_pack) {
        const int n = std::max(s->Nn * 16, (s->Nn - 1) * s->nx[0] * (s->nx[0] + s->nu[0]));
        hipLaunchKernelGGL(k_pack_persist, dim3((n + 255) / 256), dim3(256), 0, st, s->Nn, s->Np, s->nx[0], s->nu[0], D, s->persist.pab, s->persist.pcst); launches++;
        s->persist.need_pack = false;
        s->links.stream_pending = true;
    }
    if (batch_seq) { launches++; return TQGPU_OK; }          /* the caller launches the batch */
    if (s->pshard.on) {
        /* this rank's share of the workgroups; the geometry (tiers, global workgroup numbers, G) is the whole tree's */
        PGeom Gm = s->persist.geom;
        Gm.wg_of_block = s->pshard.wg_map;
        if (!s->pshard.row) return fail(TQGPU_EUNSUPPORTED, "the sharded persistent kernel is not instantiated for this shape");
        hipLaunchKernelGGL(s->pshard.sys ? s->pshard.row->sys : s->pshard.row->agent, dim3(s->pshard.G), dim3(FW * WAVE), s->persist.lds, st, s->persist.pconst, O, Gm, s->persist.psync, prologue);
        launches++;
        return TQGPU_OK;
    }
    const PersistKernels &kernels = s->uni.mstage ? s->uni.row->mpersist : s->uni.row->persist;
    const PersistFn kernel = O.reuse ? kernels.reuse : (s->persist.one && !s->links.in_batch) ? kernels.one : kernels.plain;
    hipLaunchKernelGGL(kernel, dim3(s->persist.geom.G), dim3(FW * WAVE), s->persist.lds, st, s->persist.pconst, O, s->persist.geom, s->persist.psync, prologue);
    launches++;
    return TQGPU_OK;
}

/* one Newton iteration on the generic path = its termination test (gradient + check) and the rest (Newton system, step,
 * first trial); `parts` bit 0 / bit 1 select them.  The host enqueues the iteration it expects to be the last one
 * (warm: as many as the previous solve needed) without the rest: ~17 launches that would only find `done` set.
 * Two families: launch_w3_iteration (THREE_LAUNCH), launch_phase_iteration (FUSED_TAILS, PER_PHASE); launch_generic_iteration picks. */
/* the three-launch family: k_hf_w, the forward sweep, the first trial and the trials the previous solve's counts predict */
void launch_w3_iteration(tqgpu_solver *s, const Opts &O, int h, int &launches, int parts, bool last) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    /* three launches: the termination test of this iteration was the tail of the previous launch of k_sg */
    if (!(parts & 2)) return;
    const unsigned bw_tag = next_tag(s->pp.bw_epoch);
    s->w3.tail_sg = false;
    hipLaunchKernelGGL(k_hf_w, dim3(T.Np), dim3(WT), s->w3.lds_hf_w, st, T, D, O, s->pp.sch_words, s->pp.sch_rs, bw_tag, h); launches++;
    const bool merged = T.Np > 1 && s->w3.merge;      /* forward sweep + first trial: one launch (k_sgp mode 2) */
    if (!merged && T.Np > 1) {
        const unsigned fw_tag = next_tag(s->pp.fw_epoch);
        if (s->w3.d_anc) hipLaunchKernelGGL(k_fwd3c, dim3((T.Np - 1 + SG_WAVES - 1) / SG_WAVES), dim3(SG_WAVES * WAVE), 0, st, T, D, next_w3(s), s->w3.d_anc, h);
        else hipLaunchKernelGGL(k_fwd3, dim3((T.Np - 1 + SG_WAVES - 1) / SG_WAVES), dim3(SG_WAVES * WAVE), 0, st, T, D, next_w3(s), s->pp.fw_words, fw_tag, h);
        launches++;
    } else if (!merged) { hipLaunchKernelGGL(k_ls_begin, dim3(1), dim3(256), 0, st, T, D, h); launches++; }
    /* the first trial and the predicted trials 2 .. kpred; where this is the last iteration of the chunk that launches anything, the last of them posts */
    const int kpred = h < (int)s->pp.ls_pred.size() ? std::min(s->pp.ls_pred[(size_t)h], O.lsMaxIter) : 1;
    s->w3.post_next = last && kpred < 2;
    launch_sg(s, O, merged ? 2 : 1, h, 1); launches++;
    for (int tt = 2; tt <= kpred; tt++) { s->w3.post_next = last && tt == kpred; launch_sg(s, O, 1, h, tt); launches++; }
}

/* the launch-per-phase kernels, with the reductions as launches of their own (PER_PHASE) or as the tails of their producers (FUSED_TAILS) */
void launch_phase_iteration(tqgpu_solver *s, const Opts &O, int h, int &launches, int parts, bool phases) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    auto mark = [&](int i) { if (phases && (size_t)(4 * h + i) < s->tm.phase_ev.size()) (void)hipEventRecord(s->tm.phase_ev[(size_t)(4 * h + i)], st); };
    const bool fuse = s->route == Route::FUSED_TAILS;
    mark(0);
    if (parts & 1) {
        if (fuse) { hipLaunchKernelGGL(k_grad_f, dim3(T.Nn - 1), dim3(WAVE), 0, st, T, D, O, next_fuse(s), h); launches++; }      /* with k_check as its tail */
        else {
            hipLaunchKernelGGL(k_grad, dim3(T.Nn - 1), dim3(WAVE), 0, st, T, D, O.termCondition, h); launches++;
            hipLaunchKernelGGL(k_check, dim3(1), dim3(256), 0, st, T, D, O, h); launches++;
        }
    }
    if (!(parts & 2)) return;
    const bool wide = s->pp.wide && !s->sk.dense;
    bool ls_begun = false;           /* the forward sweep's last workgroup has done k_ls_begin's work */
    if (wide) hipLaunchKernelGGL(k_hess_w, dim3(T.Np), dim3(WT), s->pp.lds_hess_w, st, T, D, h);
    else hipLaunchKernelGGL(k_hess, dim3(T.Np), dim3(WAVE), s->pp.lds_hess, st, T, D, h);
    launches++;
    mark(1);
    if (s->pp.sch_words && s->pp.bw_fused && !phases) {
        /* all levels in one launch, last block first: a block waits for its children's Schur records inside the kernel */
        const unsigned bw_tag = next_tag(s->pp.bw_epoch);
        if (wide) hipLaunchKernelGGL(k_factor_all_w, dim3(T.Np), dim3(WT), s->pp.lds_factor_w, st, T, D, O, s->pp.sch_words, s->pp.sch_rs, bw_tag, h);
        else hipLaunchKernelGGL(k_factor_all, dim3(T.Np), dim3(WAVE), s->pp.lds_factor, st, T, D, O, s->pp.sch_words, s->pp.sch_rs, bw_tag, h);
        launches++;
    } else
    for (int lvl = T.Nh - 1; lvl >= 0; lvl--) {
        const int first = s->lvl_first[lvl], count = s->lvl_first[lvl + 1] - first;
        if (wide) hipLaunchKernelGGL(k_factor_w, dim3(count), dim3(WT), s->pp.lds_factor_w, st, T, D, O, first, h);
        else hipLaunchKernelGGL(k_factor, dim3(count), dim3(WAVE), s->pp.lds_factor, st, T, D, O, first, h);
        launches++;
    }
    if (s->pp.fw_words && s->pp.fw_fused && !phases) {
        /* all levels below the root in one launch: a block waits for its parent's step inside the kernel */
        if (T.Np > 1) {
            const unsigned fw_tag = next_tag(s->pp.fw_epoch);
            const Fuse F = fuse ? next_fuse(s) : no_fuse();          /* with k_ls_begin as its tail */
            ls_begun = fuse;
            if (wide) hipLaunchKernelGGL(k_forward_all_w, dim3(T.Np - 1), dim3(WT), s->pp.lds_forward_w, st, T, D, s->pp.fw_words, fw_tag, h, F);
            else hipLaunchKernelGGL(k_forward_all, dim3(T.Np - 1), dim3(WAVE), s->pp.lds_forward, st, T, D, s->pp.fw_words, fw_tag, h, F);
            launches++;
        }
    } else
    for (int lvl = 1; lvl < T.Nh; lvl++) {
        const int first = s->lvl_first[lvl], count = s->lvl_first[lvl + 1] - first;
        if (wide) hipLaunchKernelGGL(k_forward_w, dim3(count), dim3(WT), s->pp.lds_forward_w, st, T, D, first, h);
        else hipLaunchKernelGGL(k_forward, dim3(count), dim3(WAVE), s->pp.lds_forward, st, T, D, first, h);
        launches++;
    }
    mark(2);
    if (!ls_begun) { hipLaunchKernelGGL(k_ls_begin, dim3(1), dim3(256), 0, st, T, D, h); launches++; }
    if (fuse) { hipLaunchKernelGGL(k_stage_f, dim3(T.Nn), dim3(WAVE), s->pp.lds_stage, st, T, D, O, next_fuse(s), 1, h, 1); launches++; }      /* with k_ls_decide as its tail */
    else {
        launch_stage_sweep(s, 1, h, 1); launches++;
        hipLaunchKernelGGL(k_ls_decide, dim3(1), dim3(256), 0, st, T, D, O, h, 1, 0); launches++;
    }
    mark(3);
}

void launch_generic_iteration(tqgpu_solver *s, const Opts &O, int h, int &launches, int parts, bool phases, bool last) {
    if (s->route == Route::THREE_LAUNCH) launch_w3_iteration(s, O, h, launches, parts, last);
    else launch_phase_iteration(s, O, h, launches, parts, phases);
}

/* ---- tqgpu_create step by step: each step takes the mirror and returns a TQGPU_* code ---- */
/* THE list of creation-time switches. Read per tqgpu_create call, never cached: tests and A/B runs change them between two mirrors. */
void read_switches(Switches &w) {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto is = [](const char *name, const char *value) { const char *e = getenv(name); return e && strcmp(e, value) == 0; };
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    w.generic = is("TREEQP_AMD_PATH", "generic");                /* launch-per-phase kernels only; no phantom root for x0-eliminated trees */
    w.tiered = is("TREEQP_AMD_PATH", "tiered");                  /* uniform trees: launches per tier instead of the persistent launch */
    w.strict_sum = num("TREEQP_AMD_STRICT_SUM", 0) != 0;         /* reference-order sums (Data::strict) */
    w.chunk = num("TREEQP_AMD_CHUNK", 0);                        /* > 0: Newton iterations enqueued per status read-back */
    w.fwd_levels = is("TREEQP_AMD_FWD", "levels");               /* forward sweep: one launch per tree level (the round-1 protocol) */
    w.bwd_levels = is("TREEQP_AMD_BWD", "levels");               /* backward sweep: one launch per tree level */
    w.no_fuse = set("TREEQP_AMD_NO_FUSE");                       /* small trees: the reductions as launches of their own */
    w.no_wide3 = set("TREEQP_AMD_NO_WIDE3");                     /* wide-block class: launch-per-phase kernels instead of the three-launch family */
    w.no_sgp = set("TREEQP_AMD_NO_SGP");                         /* three-launch family: k_sg (a wave per node) instead of k_sgp */
    w.no_fwd_chain = set("TREEQP_AMD_NO_FWD_CHAIN");             /* ... forward sweep with hand-overs (no k_fwd3c) */
    w.no_fwd_merge = set("TREEQP_AMD_NO_FWD_MERGE");             /* ... forward sweep as a launch of its own */
    w.no_stage16 = set("TREEQP_AMD_NO_STAGE16");                 /* single-workgroup kernel: one node per wave in the node sweeps */
    w.gp_no_groups = set("TREEQP_AMD_GP_NO_GROUPS");             /* single-workgroup kernel: one block per wave on every level */
    w.small_wide = num("TREEQP_AMD_SMALL_WIDE", 1) != 0;         /* =0: wide trees of small blocks stay on the launch-per-phase kernels */
    w.has_lds_pad = set("TREEQP_AMD_LDS_PAD"); w.lds_pad = num("TREEQP_AMD_LDS_PAD", 0);      /* experiment: KiB of LDS added to a persistent workgroup, to force fewer per CU */
    w.capacity_margin = num("TREEQP_AMD_CAPACITY_MARGIN", 0);    /* experiment: workgroups kept free in the co-residency test */
    w.no_persist_one = set("TREEQP_AMD_NO_PERSIST_ONE");         /* persistent path: never the one-workgroup-per-CU build */
    w.has_nap = set("TREEQP_AMD_NAP"); w.nap = num("TREEQP_AMD_NAP", 0);      /* persistent path: poll naps of the bottom tier off (0) / on (1) instead of by launch size */
    w.dense_single = num("TREEQP_AMD_DENSE_SINGLE_LAUNCH", 0) != 0;      /* dense trees that fit: the whole solve as one launch of one workgroup (tqgpu_set_dense_single_launch) */
    w.dense_batch = num("TREEQP_AMD_DENSE_BATCH_LAUNCH", 0) != 0;        /* ... as members of a batch: one launch, a workgroup per tree (tqgpu_set_dense_batch_launch) */
    w.verbose = set("TREEQP_AMD_VERBOSE");                       /* the persistent path's geometry on stderr */
}

/* tree tables, the uniform / multistage / x0-padded form, and what the switches take away from it */
int detect_shape(tqgpu_solver *s) {
    auto detect = [s] { detect_fast(s); if (s->uni.fast < 0) detect_multistage(s); };
    int rc = build_tables(s);
    if (rc != TQGPU_OK) return rc;
    detect();
    if (s->uni.fast < 0 && s->nx[0] == 0 && s->Nn > 1 && s->nx[1] > 0 && !s->sw.generic) {
        /* x0 eliminated (tree_qp_in_eliminate_x0: nx[0] = 0, the form every MPC caller solves).  If the tree would be
         * uniform / multistage with a full root node, give the root nx phantom states pinned to zero (bounds [0, 0],
         * unit weight, no linear term, zero A columns for the root's children): the same QP, and it takes the
         * persistent path.  The phantom entries sit in front of every x-sized array (A: in front of the first edges)
         * and never leave the device: the setters / getters skip them. */
        const int nx1 = s->nx[1];
        s->nx[0] = nx1;
        if (build_tables(s) == TQGPU_OK) detect();
        if (s->uni.fast >= 0) { s->x_pad = nx1; s->A_pad = s->nk[0] * nx1 * nx1; }
        else { s->nx[0] = 0; use_row(s, nullptr); s->uni.mstage = false; if ((rc = build_tables(s)) != TQGPU_OK) return rc; }
    }
    if (s->sw.generic) { s->uni.use_fast = 0; s->gp.use = 0; }
    s->gpd.single = s->sw.dense_single;
    s->gpd.batch = s->sw.dense_batch;
    if (s->sw.tiered) s->persist.use = 0;
    /* reference-order sums (strict_sum / strict_block_dots): the launch-per-phase kernels and the single-workgroup kernel carry them;
     * the fused tails, the three-launch family and the persistent / tiered kernels (their partial sums are per workgroup by
     * construction) stand aside */
    s->strict_sum = s->sw.strict_sum;
    if (s->strict_sum) { s->uni.use_fast = 0; s->pp.wide = s->pp.wide_small = false; }          /* (the MFMA kernels of the wide-block class sum in tile order) */
    s->persist.use_orig = s->persist.use;
    if (s->sw.chunk > 0) s->pp.chunk = s->sw.chunk;
    s->nxmax = *std::max_element(s->nx.begin(), s->nx.end());
    return TQGPU_OK;
}

/* the slab and what points into it: tables, node records, Tree / Data, host mirrors; the stream and the event ring */
int layout_slab(tqgpu_solver *s) {
    /* one slab for everything */
    Carver cv;
    const size_t I = sizeof(int), Dbl = sizeof(double);
    const size_t o_dad = cv.take(s->Nn * I), o_nk = cv.take(s->Nn * I), o_kid0 = cv.take(s->Nn * I), o_nx = cv.take(s->Nn * I), o_nu = cv.take(s->Nn * I);
    const size_t o_xoff = cv.take((s->Nn + 1) * I), o_uoff = cv.take((s->Nn + 1) * I), o_aoff = cv.take((s->Nn + 1) * I), o_boff = cv.take((s->Nn + 1) * I);
    const size_t o_pos = cv.take(s->Nn * I), o_bdim = cv.take(s->Nn * I), o_woff = cv.take((s->Nn + 1) * I), o_utoff = cv.take((s->Nn + 1) * I);
    const size_t SX = s->sum_nx, SU = s->sum_nu;
    const size_t o_A = cv.take(s->sum_A * Dbl), o_B = cv.take(s->sum_B * Dbl), o_b = cv.take(SX * Dbl);
    const size_t o_Qd = cv.take(SX * Dbl), o_q = cv.take(SX * Dbl), o_xmin = cv.take(SX * Dbl), o_xmax = cv.take(SX * Dbl);
    const size_t o_Rd = cv.take(SU * Dbl), o_r = cv.take(SU * Dbl), o_umin = cv.take(SU * Dbl), o_umax = cv.take(SU * Dbl);
    const size_t o_Qinv = cv.take(SX * Dbl), o_Rinv = cv.take(SU * Dbl);
    const size_t o_qmod = cv.take(SX * Dbl), o_x = cv.take(SX * Dbl), o_xUnc = cv.take(SX * Dbl), o_Qcal = cv.take(SX * Dbl);
    const size_t o_rmod = cv.take(SU * Dbl), o_u = cv.take(SU * Dbl), o_uUnc = cv.take(SU * Dbl), o_Rcal = cv.take(SU * Dbl);
    const size_t o_xUncS = cv.take(SX * Dbl), o_uUncS = cv.take(SU * Dbl);
    const size_t o_lam0 = cv.take(SX * Dbl), o_lam1 = cv.take(SX * Dbl), o_dlam = cv.take(SX * Dbl), o_res = cv.take(SX * Dbl), o_resMod = cv.take(SX * Dbl);
    const size_t o_invd = cv.take(SX * Dbl);
    const size_t o_W = cv.take(s->sum_W * Dbl), o_CW = cv.take(s->sum_W * Dbl), o_Ut = cv.take(s->sum_Ut * Dbl), o_CUt = cv.take(s->sum_Ut * Dbl);
    const size_t o_fval = cv.take(s->Nn * Dbl), o_perr = cv.take((SX + s->Nn + 1) * Dbl), o_pdot = cv.take(s->Nn * Dbl);
    const size_t maxnx = (size_t)s->nxmax;
    const size_t o_sbuf = cv.take((s->uni.fast >= 0 ? (size_t)s->Nn * (maxnx * maxnx + maxnx) : 1) * Dbl), o_ybuf = cv.take((SX + 1) * Dbl);
    const size_t o_mux = cv.take(SX * Dbl), o_muu = cv.take(SU * Dbl);
    const size_t o_lami = cv.take(SX * Dbl);
    s->poff.assign(s->Nn + 1, 0);
    for (int k = 0; k < s->Nn; k++) s->poff[k + 1] = s->poff[k] + (s->nx[k] + s->nu[k]) * (s->nx[k] + s->nu[k]);
    const size_t o_kind = cv.take(s->Nn * I), o_bmask = cv.take(2 * (size_t)s->Nn * sizeof(unsigned long long));
    const size_t o_poff = cv.take((s->Nn + 1) * I), o_Hd = cv.take((size_t)std::max(s->poff[s->Nn], 1) * Dbl), o_Pd = cv.take((size_t)std::max(s->poff[s->Nn], 1) * Dbl);
    const size_t o_ctrl = cv.take(sizeof(Ctrl));
    const size_t o_stamps = cv.take((8 * 32 * 2 + 1024) * sizeof(unsigned long long));   /* + 1024: placement census of the persistent launch (diagnostic builds) */
    s->ls_log_cap = 4096;
    const size_t o_log = cv.take(s->ls_log_cap * I);
    s->slab_bytes = cv.off + 256;

    int rc;
    if ((rc = s->mem.device(s->slab, s->slab_bytes, TQGPU_ENOMEM, "the device mirror"))) return rc;
    if (hipMemset(s->slab, 0, s->slab_bytes) != hipSuccess) return fail(TQGPU_ENODEVICE, "hipMemset failed");
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return fail(TQGPU_ENODEVICE, "hipStreamCreate failed");
    { std::lock_guard<std::mutex> lk(g_streams_mu); g_live_streams.insert(s->stream); }
    s->tm.ring_ev0.assign(EV_RING, nullptr); s->tm.ring_ev1.assign(EV_RING, nullptr); s->tm.ring_ok.assign(EV_RING, 0);
    for (int i = 0; i < EV_RING; i++)
        if (hipEventCreate(&s->tm.ring_ev0[i]) != hipSuccess || hipEventCreate(&s->tm.ring_ev1[i]) != hipSuccess) return fail(TQGPU_ENODEVICE, "hipEventCreate failed");
    if ((rc = s->mem.host(s->h_res, sizeof(HostRes), "the result block"))) return rc;
    memset(s->h_res, 0, sizeof(HostRes));
    s->h_ctrl = &s->h_res->c;
    if ((rc = s->mem.host(s->h_ls_log, s->ls_log_cap * I, "the line-search log"))) return rc;

    void *base = s->slab;
#define UP(off, vec) if (hipMemcpy(at<int>(base, off), (vec).data(), (vec).size() * I, hipMemcpyHostToDevice) != hipSuccess) return fail(TQGPU_ENODEVICE, "table upload failed")
    UP(o_dad, s->dad); UP(o_nk, s->nk); UP(o_kid0, s->kid0); UP(o_nx, s->nx); UP(o_nu, s->nu);
    UP(o_xoff, s->xoff); UP(o_uoff, s->uoff); UP(o_aoff, s->aoff); UP(o_boff, s->boff);
    UP(o_pos, s->pos); UP(o_bdim, s->bdim); UP(o_woff, s->woff); UP(o_utoff, s->utoff);
    UP(o_poff, s->poff);
#undef UP
    Tree &T = s->T;
    T.Nn = s->Nn; T.Np = s->Np; T.Nh = s->Nh; T.nx0 = s->nx0;
    T.dad = at<int>(base, o_dad); T.nk = at<int>(base, o_nk); T.kid0 = at<int>(base, o_kid0);
    T.nx = at<int>(base, o_nx); T.nu = at<int>(base, o_nu); T.xoff = at<int>(base, o_xoff); T.uoff = at<int>(base, o_uoff);
    T.aoff = at<int>(base, o_aoff); T.boff = at<int>(base, o_boff); T.pos = at<int>(base, o_pos);
    T.bdim = at<int>(base, o_bdim); T.woff = at<int>(base, o_woff); T.utoff = at<int>(base, o_utoff);
    {
        std::vector<int> desc((size_t)DESC_INTS * s->Nn, 0);
        for (int k = 0; k < s->Nn; k++) {
            int *e = &desc[(size_t)DESC_INTS * k];
            const int k0 = s->nk[k] > 0 ? s->kid0[k] : 0, dd = k > 0 ? s->dad[k] : 0;
            e[0] = s->bdim[k]; e[1] = s->nx[k]; e[2] = s->nu[k]; e[3] = s->nk[k]; e[4] = k0; e[5] = s->xoff[k]; e[6] = s->uoff[k];
            e[7] = s->xoff[k0]; e[8] = s->woff[k]; e[9] = s->utoff[k]; e[10] = dd; e[11] = s->pos[k]; e[12] = s->bdim[dd]; e[13] = s->woff[dd];
            for (int u = 0; u < 4 && u < s->nk[k]; u++) { e[16 + 3 * u] = s->nx[k0 + u]; e[17 + 3 * u] = s->aoff[k0 + u]; e[18 + 3 * u] = s->boff[k0 + u]; }
        }
        if ((rc = s->mem.upload(s->uni.d_desc, desc.data(), desc.size() * I, TQGPU_ENOMEM, "the node records"))) return rc;
        T.desc = s->uni.d_desc;
    }
    Data &D = s->D;
    s->A = at<double>(base, o_A); s->B = at<double>(base, o_B); s->b = at<double>(base, o_b);
    s->Qd = at<double>(base, o_Qd); s->Rd = at<double>(base, o_Rd); s->q = at<double>(base, o_q); s->r = at<double>(base, o_r);
    s->xmin = at<double>(base, o_xmin); s->xmax = at<double>(base, o_xmax); s->umin = at<double>(base, o_umin); s->umax = at<double>(base, o_umax);
    D.A = s->A; D.B = s->B; D.b = s->b; D.Qd = s->Qd; D.Rd = s->Rd; D.q = s->q; D.r = s->r;
    D.xmin = s->xmin; D.xmax = s->xmax; D.umin = s->umin; D.umax = s->umax;
    D.Qinv = at<double>(base, o_Qinv); D.Rinv = at<double>(base, o_Rinv);
    D.qmod = at<double>(base, o_qmod); D.rmod = at<double>(base, o_rmod); D.x = at<double>(base, o_x); D.u = at<double>(base, o_u);
    D.xUnc = at<double>(base, o_xUnc); D.uUnc = at<double>(base, o_uUnc); D.QinvCal = at<double>(base, o_Qcal); D.RinvCal = at<double>(base, o_Rcal);
    D.xUncS = at<double>(base, o_xUncS); D.uUncS = at<double>(base, o_uUncS);
    D.lam0 = at<double>(base, o_lam0); D.lam1 = at<double>(base, o_lam1); D.dlam = at<double>(base, o_dlam);
    D.res = at<double>(base, o_res); D.resMod = at<double>(base, o_resMod); D.invd = at<double>(base, o_invd);
    D.W = at<double>(base, o_W); D.CholW = at<double>(base, o_CW); D.Ut = at<double>(base, o_Ut); D.CholUt = at<double>(base, o_CUt);
    D.fval = at<double>(base, o_fval); D.part_err = at<double>(base, o_perr); D.part_dot = at<double>(base, o_pdot);
    D.Sbuf = at<double>(base, o_sbuf); D.ybuf = at<double>(base, o_ybuf);
    D.stamps = at<unsigned long long>(base, o_stamps);
    D.ctrl = at<Ctrl>(base, o_ctrl); D.ls_log = at<int>(base, o_log); D.ls_log_cap = s->ls_log_cap;
    D.strict = s->strict_sum ? 1 : 0;
    D.dense = 0; s->sk.d_kind = at<int>(base, o_kind); D.kind = s->sk.d_kind; s->sk.d_Hd = at<double>(base, o_Hd); D.Hd = s->sk.d_Hd; D.Pd = at<double>(base, o_Pd); D.poff = at<int>(base, o_poff);
    D.bmask = at<unsigned long long>(base, o_bmask); D.xpad = s->x_pad;
    s->uni.use_fast_orig = s->uni.use_fast;
    s->d_mu_x = at<double>(base, o_mux); s->d_mu_u = at<double>(base, o_muu);
    s->d_lam_init = at<double>(base, o_lami);
    s->in_off0 = o_A; s->in_bytes = o_Qinv - o_A;
    s->out.doubles = 2 * (size_t)(s->sum_nx - s->x_pad) + 2 * (size_t)s->sum_nu + 2 * (size_t)s->sum_lam;
    if ((rc = s->mem.host(s->h_in, std::max<size_t>(s->in_bytes, 8), "the host mirror of the inputs")) ||
        (rc = s->mem.host(s->h_lam, sizeof(double) * (size_t)std::max(s->sum_nx, 1), "the host mirror of the duals")) ||
        (rc = s->mem.host(s->out.h, sizeof(double) * std::max<size_t>(s->out.doubles, 1), "the host mirror of the solution")) ||
        (rc = s->mem.device(s->out.d, sizeof(double) * std::max<size_t>(s->out.doubles, 1), TQGPU_ENOMEM, "the packed solution")))
        return rc;
    if (s->x_pad) {
        /* phantom root states: weight 1, everything else zero (the slab is zeroed) */
        std::vector<double> ones((size_t)s->x_pad, 1.0);
        if (hipMemcpy(s->Qd, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(TQGPU_ENODEVICE, "hipMemcpy failed");
    }
    return TQGPU_OK;
}

/* launch-per-phase kernels (any tree): LDS budgets, one launch per sweep or per level, the reductions as tails of the sweeps */
int setup_per_phase(tqgpu_solver *s) {
    int rc;
    if ((rc = allow_lds(k_stage, s->pp.lds_stage)) || (rc = allow_lds(k_hess, s->pp.lds_hess)) ||
        (rc = allow_lds(k_factor, s->pp.lds_factor)) || (rc = allow_lds(k_forward, s->pp.lds_forward)) ||
        (rc = allow_lds(k_factor_all, s->pp.lds_factor)) || (rc = allow_lds(k_forward_all, s->pp.lds_forward)) || (rc = allow_lds(k_stage_f, s->pp.lds_stage)))
        return rc;
    if (s->pp.wide && ((rc = allow_lds(k_hess_w, s->pp.lds_hess_w)) || (rc = allow_lds(k_factor_w, s->pp.lds_factor_w)) || (rc = allow_lds(k_forward_w, s->pp.lds_forward_w)) || (rc = allow_lds(k_forward_all_w, s->pp.lds_forward_w)) || (rc = allow_lds(k_factor_all_w, s->pp.lds_factor_w))))
        return rc;
    if (s->uni.fast >= 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, s->device) != hipSuccess || prop.maxThreadsPerBlock < FW * WAVE) use_row(s, nullptr);
    }
    s->pp.fw_fused = !s->sw.fwd_levels && !s->strict_sum;      /* (strict: the reference's launch-per-level order of operations) */
    s->pp.bw_fused = !s->sw.bwd_levels && !s->strict_sum;      /* (a fused sweep subtracts a child's Schur record AFTER an ALWAYS shift of the diagonal, the reference before it) */
    s->pp.sch_rs = (s->nxmax + 1) * (s->nxmax + 1);
    s->pp.fuse_ok = s->Nn <= FUSE_MAX && s->Nn >= 2 && !s->sw.no_fuse && !s->strict_sum;
    /* hand-over words of the fused forward / backward sweeps of the launch-per-phase path (zeroed once; every launch brings its own tag) */
    const size_t U = sizeof(unsigned long long);
    if ((rc = s->mem.zeroed(s->pp.fw_words, U * 2 * (size_t)std::max(s->sum_nx, 1), TQGPU_ENOMEM, "the forward hand-over words")) ||
        (rc = s->mem.zeroed(s->pp.sch_words, U * 2 * (size_t)s->pp.sch_rs * (size_t)s->Nn, TQGPU_ENOMEM, "the Schur hand-over words")))
        return rc;
    if (s->pp.fuse_ok && ((rc = s->mem.zeroed(s->pp.fuse_red, U * 2 * (size_t)s->Nn, TQGPU_ENOMEM, "the fused reductions")) ||
                       (rc = s->mem.zeroed(s->pp.fuse_cnt, 4 * sizeof(int), TQGPU_ENOMEM, "the fused reductions' counter"))))
        return rc;
    return TQGPU_OK;
}

/* the three-launch family of the wide-block class (tdunes_wide3.hpp) */
int setup_wide3(tqgpu_solver *s) {
    if (!(s->pp.wide && s->pp.fw_fused && s->pp.bw_fused && !s->sw.no_wide3 && !s->strict_sum)) return TQGPU_OK;      /* (TREEQP_AMD_FWD / BWD = levels ask for the launch-per-level kernels) */
    for (int k = 0; k < s->Np; k++) s->w3.lds_hf_w = std::max(s->w3.lds_hf_w, wide3_lds(s->bdim[k], k > 0 ? s->nx[k] : 0, s->nx[k] + s->nu[k]));
    if (!(s->nxmax <= 32 && s->w3.lds_hf_w <= 160 * 1024 && SG_WAVES * s->pp.lds_stage <= 160 * 1024)) return TQGPU_OK;
    /* k_sgp: one entry of a node's [x | u] per lane, one row of a block per lane */
    bool fits = true;
    for (int k = 0; k < s->Nn; k++) fits = fits && s->nx[k] + s->nu[k] <= 64;
    for (int k = 0; k < s->Np; k++) s->w3.sgp_accs = std::max(s->w3.sgp_accs, std::min(s->nk[k], 8) * (s->nx[k] + s->nu[k]));      /* the children's terms in LDS: up to 8 children (more: taken by wave 0 on its own) */
    for (int k = 0; k < s->Np; k++) s->w3.lds_sgp = std::max(s->w3.lds_sgp, wide3_lds_sgp(s->bdim[k], s->nx[k] + s->nu[k], s->w3.sgp_accs));
    s->w3.sgp = fits && s->w3.lds_sgp <= 64 * 1024 && !s->sw.no_sgp;
    /* forward sweep without hand-overs (k_fwd3c): small nodes, short paths, blocks whose region of CholW has room for the copy of z0
     * beside the diagnostic stamps */
    bool okc = s->Np > 1 && !s->sw.no_fwd_chain;
    for (int k = 0; k < s->Nn && okc; k++) okc = s->nx[k] <= 8;
    for (int k = 0; k < s->Np && okc; k++) okc = s->bdim[k] >= 3 && s->bdim[k] <= 64;
    std::vector<int> anc;
    if (okc) {
        anc.assign((size_t)FWDC_INTS * s->Np, 0);
        for (int ii = 1; ii < s->Np && okc; ii++) {
            std::vector<int> path;                      /* ii, dad(ii), .., the root's child */
            for (int n = ii; n != 0; n = s->dad[n]) path.push_back(n);
            const int L = (int)path.size();
            if (L > 16) { okc = false; break; }
            int *a = &anc[(size_t)FWDC_INTS * ii];
            a[0] = L;
            for (int k = 0; k < L; k++) {
                const int node = path[(size_t)(L - 1 - k)], prev = s->dad[node], dp_ = s->bdim[prev];
                a[1 + 4 * k + 0] = s->woff[prev] + dp_ * dp_ - dp_ + s->pos[node];
                a[1 + 4 * k + 1] = s->utoff[prev] + s->pos[node];
                a[1 + 4 * k + 2] = dp_;
                a[1 + 4 * k + 3] = (prev == 0 ? 0 : s->nx[prev]) | (s->nx[node] << 8);
            }
        }
    }
    s->w3.merge = okc && s->w3.sgp && !s->sw.no_fwd_merge;
    const size_t U = sizeof(unsigned long long);
    const size_t groups = std::max((size_t)(s->Nn + SG_WAVES - 1) / SG_WAVES, (size_t)s->Np);      /* workgroups of k_sg / k_sgp / k_fwd3 */
    int rc;
    if ((rc = s->mem.zeroed(s->w3.xu, U * 2 * (size_t)std::max(s->sum_nx + s->sum_nu, 1), TQGPU_ENOMEM, "the three-launch hand-over words")) ||
        (rc = s->mem.zeroed(s->w3.red, U * 4 * groups, TQGPU_ENOMEM, "the three-launch reductions")) ||
        (rc = s->mem.zeroed(s->w3.cnt, 4 * sizeof(int), TQGPU_ENOMEM, "the three-launch reductions' counter")) ||
        (rc = allow_lds(k_hf_w, s->w3.lds_hf_w)) || (rc = allow_lds(k_sg, SG_WAVES * ((s->pp.lds_stage + 7) / 8) * 8)))
        return rc;
    if (okc && (rc = s->mem.upload(s->w3.d_anc, anc.data(), anc.size() * sizeof(int), TQGPU_ENOMEM, "the path table of the forward sweep"))) return rc;
    if (s->w3.merge && (rc = s->mem.zeroed(s->w3.d_pdw, U * 2 * (size_t)s->Np, TQGPU_ENOMEM, "the forward sweep's partial sums"))) return rc;
    s->w3.ok = true;
    return TQGPU_OK;
}

int setup_single_wg(tqgpu_solver *s) {
    /* single-workgroup persistent kernel for small trees of any shape: every level must be a few rounds
     * of GP_WAVES blocks at most, and the per-wave LDS windows must fit the default 64 KB */
    int widest = 0;
    for (int l = 0; l <= s->Nh; l++) widest = std::max(widest, s->lvl_first[l + 1] - s->lvl_first[l]);
    const size_t per_wave = (std::max(std::max(s->pp.lds_stage, s->pp.lds_hess), std::max(s->pp.lds_factor, s->pp.lds_forward)) + 7) / 8 + 2;
    s->gp.lds_wave = per_wave;
    {
        /* four nodes per wave in the stage sweep: nx + nu <= 16 everywhere, clipping nodes only, and a quarter of the wave's window
         * holds a node's duals (bdim + nx doubles) */
        bool ok16 = !s->sk.dense && !s->sw.no_stage16;
        for (int k = 0; k < s->Nn && ok16; k++) ok16 = s->nx[k] + s->nu[k] <= 16 && (size_t)(s->bdim[k] + s->nx[k]) <= per_wave / 4;
        s->gp.small16 = ok16;
        bool ok8 = !s->sw.no_stage16 && !s->strict_sum;          /* eight nodes per wave in the gradient sweep: nx <= 8 everywhere */
        for (int k = 0; k < s->Nn && ok8; k++) ok8 = s->nx[k] <= 8;
        s->gp.small8 = ok8;
    }
    s->gp.ok = widest <= 6 * GP_WAVES && per_wave * 8 * GP_WAVES <= 150 * 1024;
    /* LDS mirror of the mutable state (tdunes_gpersist.hpp): 16 node-sized vectors (rounded up to even), 4 block arrays */
    {
        auto ev = [](size_t n) { return (n + 1) & ~(size_t)1; };
        const size_t sx = (size_t)s->sum_nx, su = (size_t)s->sum_nu;
        const size_t mirror = 11 * ev(sx) + 5 * ev(su) + 2 * ev((size_t)s->sum_W) + 2 * ev((size_t)s->sum_Ut) + 2 * ev((size_t)s->Nn) + ev(sx + s->Nn + 1) + ev(su) * 0;
        const size_t tables = (13 * ((size_t)s->Nn + 3)) / 2 + 16;            /* int tables, in doubles */
        s->gp.lds_total = (per_wave * GP_WAVES + mirror + tables + 8) * 8;
        s->gp.in_lds = s->gp.ok && s->gp.lds_total <= 150 * 1024;
        const size_t consts = (ev((size_t)s->sum_A) + ev((size_t)s->sum_B) + 5 * ev(sx) + 4 * ev(su)) * 8;
        s->gp.const_in_lds = s->gp.in_lds && s->gp.lds_total + consts <= 150 * 1024;
        if (s->gp.const_in_lds) s->gp.lds_total += consts;
        if (!s->gp.in_lds) {
            /* the state does not fit: the index tables alone, next to the per-wave windows, if THEY fit */
            s->gp.tab_in_lds = s->gp.ok && (per_wave * GP_WAVES + tables + 8) * 8 <= 150 * 1024;
            s->gp.lds_total = (per_wave * GP_WAVES + (s->gp.tab_in_lds ? tables + 8 : 0)) * 8;
        }
        else if (s->gp.lds_total > 64 * 1024 &&
                 hipFuncSetAttribute(reinterpret_cast<const void *>(g_persist), hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->gp.lds_total) != hipSuccess) {
            (void)hipGetLastError();
            s->gp.in_lds = false; s->gp.tab_in_lds = false; s->gp.lds_total = per_wave * GP_WAVES * 8;
        }
        if (s->gp.ok && !s->gp.in_lds && s->gp.lds_total > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void *>(g_persist), hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->gp.lds_total) != hipSuccess) {
            (void)hipGetLastError();
            s->gp.ok = false;
        }
    }
    if (s->gp.ok) {
        /* behind the level table: for every level of parents, how many of its blocks one wave takes side by side in the backward /
         * forward / Hessian sweeps (factor_body_g ...): levels wider than the workgroup's 16 waves whose blocks all have the same
         * small dimensions (the chains of a pruned scenario tree); 1 = one block per wave */
        std::vector<int> tab(s->lvl_first);
        for (int lvl = 0; lvl <= s->Nh; lvl++) {
            int grp = 1;
            const int first = s->lvl_first[lvl], count = s->lvl_first[lvl + 1] - first;
            if (!s->sw.gp_no_groups && lvl >= 1 && lvl < s->Nh && count > GP_WAVES && !s->sk.dense) {
                const int d0 = s->bdim[first], n0 = s->nx[first], u0 = s->nu[first], c0 = s->nk[first];
                bool same = true;
                for (int k = first; k < first + count && same; k++) {
                    same = s->bdim[k] == d0 && s->nx[k] == n0 && s->nu[k] == u0 && s->nk[k] == c0;
                    for (int cc = 0; cc < s->nk[k] && same; cc++) same = s->nx[s->kid0[k] + cc] == s->nx[s->kid0[first] + cc];
                }
                const int R = d0 + 1 + n0;
                /* doubles of a group's window: factor_body's tall matrix, forward_body's factor + vectors, hess_body's C and C P */
                const size_t need = std::max(std::max((size_t)(R | 1) * d0 + d0 + 2, (size_t)(d0 | 1) * d0 + 2 * d0 + n0 + 2), (size_t)2 * d0 * (n0 + u0) + 2);
                if (same && d0 >= 1) {
                    if (R <= WAVE / 3 && 3 * need <= s->gp.lds_wave) grp = 3;
                    else if (R <= WAVE / 2 && 2 * need <= s->gp.lds_wave) grp = 2;
                }
            }
            tab.push_back(grp);
        }
        return s->mem.upload(s->gp.d_lvl_first, tab.data(), sizeof(int) * tab.size(), TQGPU_ENOMEM, "the level table");
    }
    return TQGPU_OK;
}

}  // namespace

extern "C" int tqgpu_create(tqgpu_solver **out, int device, int Nn, const int *nk, const int *nx, const int *nu) {
    if (!out || Nn < 2 || !nk || !nx || !nu) return fail(TQGPU_EINVAL, "tqgpu_create: bad arguments");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(TQGPU_ENODEVICE, std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") + "); the tdunes hot path has no CPU fallback");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(TQGPU_EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    tqgpu_solver *s = new tqgpu_solver();
    { static std::atomic<unsigned long> next_uid{1}; s->uid = next_uid.fetch_add(1); }
    s->device = device; s->Nn = Nn;
    s->nk.assign(nk, nk + Nn); s->nx.assign(nx, nx + Nn); s->nu.assign(nu, nu + Nn);
    read_switches(s->sw);
    int rc;
    if ((rc = detect_shape(s)) || (rc = layout_slab(s)) || (rc = setup_per_phase(s)) || (rc = setup_wide3(s)) || (rc = setup_persist(s)) || (rc = setup_single_wg(s))) {}
    /* the zeroing of the slabs above went out as device memsets, which may return before they have happened, on the null stream, which
     * the solver's non-blocking stream does not wait for: everything is in place before the first solve can be enqueued */
    else if (hipDeviceSynchronize() != hipSuccess) rc = fail(TQGPU_ENODEVICE, "hipDeviceSynchronize failed");
    if (rc != TQGPU_OK) { tqgpu_destroy(s); return rc; }
    *out = s;
    return TQGPU_OK;
}

extern "C" void tqgpu_destroy(tqgpu_solver *s) {
    (void)settle(s);
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (auto &ev : s->tm.iter_ev) (void)hipEventDestroy(ev);
    for (auto &ev : s->tm.phase_ev) (void)hipEventDestroy(ev);
    if (s->tm.sweep_ev0) (void)hipEventDestroy(s->tm.sweep_ev0);
    if (s->tm.sweep_ev1) (void)hipEventDestroy(s->tm.sweep_ev1);
    for (auto &ev : s->tm.ring_ev0) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : s->tm.ring_ev1) if (ev) (void)hipEventDestroy(ev);
    if (s->stream) { { std::lock_guard<std::mutex> lk(g_streams_mu); g_live_streams.erase(s->stream); } (void)hipStreamDestroy(s->stream); }
    shard_release(s);
    s->mem.free_all();
    delete s;
}

/* what a mirror admits: the persistent single launch (uniform or multistage trees), launches per tier (uniform trees only) */
static bool persist_capable(const tqgpu_solver *s) { return s->uni.fast >= 0 && s->uni.use_fast && s->persist.ok && s->persist.use && !s->shard.on; }
static bool tiered_capable(const tqgpu_solver *s) { return s->uni.fast >= 0 && s->uni.use_fast && !s->uni.mstage; }
/* `batch`: as a member of a batched launch (one workgroup per tree) the single-workgroup kernel also takes trees whose
 * state does not fit the LDS mirror; alone, such a tree is faster with one launch per level */
static bool uses_gpersist(const tqgpu_solver *s, bool batch) {
    /* a dense tree: only on request, only where plan_dense_single found room; alone and as a member of a batch are two requests
     * (g_persist_dense, g_persist_dense_batch) */
    if (s->sk.dense) return (batch ? s->gpd.batch : s->gpd.single) && s->gpd.ok && s->gp.use && !s->shard.on;
    return s->gp.ok && (s->gp.in_lds || batch) && s->gp.use && !s->shard.on && !persist_capable(s) && !tiered_capable(s);
}
/* the first route that the mirror and the options admit (batch_member: see uses_gpersist) */
static Route route_of(const tqgpu_solver *s, const tqgpu_opts *o, bool batch_member) {
    const int p = o->profile, m = o->maxIter;
    if (persist_capable(s) && p == 0 && m > 0) return Route::PERSIST;
    if (uses_gpersist(s, batch_member) && p == 0 && m > 0) return Route::SINGLE_WG;
    if (tiered_capable(s) && p < 3) return Route::TIERED;
    if (s->w3.ok && !s->sk.dense && p < 3 && !s->shard.on) return Route::THREE_LAUNCH;
    if (s->pp.fuse_ok && p < 3 && !s->shard.on && !s->sk.box && !s->sk.gen) return Route::FUSED_TAILS;     /* (box nodes: a failed stage solve ends the solve in the control block, which the NEXT launch reads) */
    return Route::PER_PHASE;       /* (profile level 3: one launch per level, whose launches ARE the reference's phases) */
}
/* the kernel variants the steps of tqgpu_create (setup_per_phase, setup_wide3, setup_persist, setup_single_wg) and tqgpu_set_objective_mixed chose, and whether the last solve ran g_persist (TQGPU_PLAN_* bits);
 * reads fields, changes nothing */
extern "C" int tqgpu_debug_plan(const tqgpu_solver *s, unsigned *flags, int *sgp_accs) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    const bool bits[] = {s->pp.wide, s->pp.wide_small, s->w3.ok, s->w3.sgp, s->w3.merge, s->w3.d_anc != nullptr, s->pp.fuse_ok, s->persist.ok,
                         s->persist.one, s->gp.ok, s->gp.in_lds, s->gp.const_in_lds, s->gp.tab_in_lds, s->gp.small16, s->gp.small8,
                         s->sk.dense, s->sk.box, s->solve_no > 0 && s->route == Route::SINGLE_WG, s->sk.gen,
                         s->sk.dense && s->gpd.single && s->gpd.ok};
    unsigned f = 0;
    for (unsigned i = 0; i < sizeof(bits) / sizeof(bits[0]); i++) f |= bits[i] ? 1u << i : 0u;
    if (flags) *flags = f;
    if (sgp_accs) *sgp_accs = s->w3.sgp_accs;
    return TQGPU_OK;
}
extern "C" int tqgpu_uses_fused_path(const tqgpu_solver *s) {
    if (!s) return 0;
    tqgpu_opts o{}; o.maxIter = 1;          /* the route under default options */
    const Route r = route_of(s, &o, false);
    return r == Route::PERSIST ? 2 : r == Route::TIERED ? 1 : r == Route::SINGLE_WG ? 3 : 0;
}

/* the options as the kernels take them; TREEQP_AMD_STAMPS is for the caller to set */
static int opts_from(const tqgpu_opts *o, Opts &O) {
    O.maxIter = o->maxIter; O.termCondition = o->termCondition; O.regType = o->regType;
    O.lsMaxIter = o->lineSearchMaxIter; O.lsRestartTrigger = o->lineSearchRestartTrigger; O.reuse = o->checkLastActiveSet == 2 ? 1 : 0;
    O.tol = o->stationarityTolerance; O.regTol = o->regTol; O.regValue = o->regValue;
    O.gamma = o->lineSearchGamma; O.beta = o->lineSearchBeta; O.stamps = 0;
    if (O.termCondition < 0 || O.termCondition > 2 || O.regType < 0 || O.regType > 2 || O.regValue < 0) return fail(TQGPU_EINVAL, "invalid option value");
    return TQGPU_OK;
}

/* diagnostic: copy the in-kernel time stamps of the last fused iteration (8 kernels x 32 slots x
 * {shader clock, 100 MHz wall clock}); only filled when TREEQP_AMD_STAMPS is set */
/* diagnostic builds (-DTQ_WIDE_STAMPS): per-block time stamps of k_hf_w, four 64-bit words per block kept in the (otherwise unused) CholW array */
extern "C" int tqgpu_debug_block_stamps(tqgpu_solver *s, unsigned long long *out, int cap_blocks) {
    SETTLE(s);
    if (!s || !out) return fail(TQGPU_EINVAL, "bad arguments");
    HIP_TRY(hipStreamSynchronize(s->stream));          /* (the copy below is on the null stream, which the solver's non-blocking stream does not order) */
    std::vector<double> tmp((size_t)std::max(s->sum_W, 1));
    HIP_TRY(hipMemcpy(tmp.data(), getenv("TQ_STAMPS_OF_SGP") ? s->D.W : s->D.CholW, sizeof(double) * (size_t)s->sum_W, hipMemcpyDeviceToHost));
    const int n = std::min(cap_blocks, s->Np);
    for (int k = 0; k < n; k++) memcpy(out + 4 * (size_t)k, tmp.data() + s->woff[k], 4 * sizeof(unsigned long long));
    return n;
}

extern "C" int tqgpu_get_stamps(tqgpu_solver *s, unsigned long long *out, int cap) {
    SETTLE(s);
    if (!s || !out) return fail(TQGPU_EINVAL, "bad arguments");
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int n = std::min(cap, 8 * 32 * 2 + 1024);
    HIP_TRY(hipMemcpy(out, s->D.stamps, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
    return TQGPU_OK;
}

#include "tdunes_problem.hpp"

namespace {

/* tqgpu_mpc_stats: what this thread's last MPC step cost.  `live` points at the record while a step runs, so that the solve's own read-backs
 * and waits are counted where they happen; outside a step nothing is counted. */
struct MpcStats { int launches = 0, copies = 0, waits = 0; };
thread_local MpcStats g_mpc_stats;
thread_local MpcStats *g_mpc_live = nullptr;
#define MPC_COUNT(field, n) do { if (g_mpc_live) g_mpc_live->field += (n); } while (0)

/* What one launch of k_mpc_pre does for a mirror (tdunes_mpc.hpp: mpc_item, mpc_pre_grid, launch_mpc_pre): fold x0 into the root terms; copy the last
 * duals into the start buffer (warm); fold the window in force into q, r (track); shift: the copy is tqgpu_mpc_shift's, through its tables in any mode */
struct MpcPre { bool fold = false, warm = false, track = false, shift = false; };
/* THE warm-start test: the mode asks for the last duals, nobody has put anything else into the start buffer since, and there are last duals */
bool mpc_warm_due(const tqgpu_solver *s) { return s->warm.mode >= 1 && !s->warm.fresh && s->solve_no > 0; }
int launch_mpc_pre(tqgpu_solver *s, MpcPre p, int *solve_launches);

/* the block as tagged words (HostRes::tg, posted by the persistent launches): complete when every word carries `want`; unpacked into the fields */
bool take_tagged_block(HostRes *hr, unsigned want) {
    volatile unsigned long long *tg = hr->tg;
    unsigned long long w[HOSTRES_WORDS];
    for (int i = 0; i < HOSTRES_WORDS; i++) { w[i] = tg[i]; if ((unsigned)(w[i] >> 32) != want) return false; }
    unsigned *dst = reinterpret_cast<unsigned *>(&hr->c);
    for (int i = 0; i < 24; i++) dst[i] = (unsigned)w[i];
    hr->t_start = (w[24] & 0xFFFFFFFFull) | (w[25] << 32);
    hr->t_end = (w[26] & 0xFFFFFFFFull) | (w[27] << 32);
    hr->seq = want;
    return true;
}

/* spin until the pinned result block carries `want`, for 2 s at the most (the clock is read every 65 536 spins); tagged: the block may
 * arrive as tagged words.  -> whether it arrived; what to do when it did not is the caller's */
bool await_result_block(HostRes *hr, unsigned want, bool tagged) {
    volatile unsigned *seq = &hr->seq;
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = true;
    for (long spins = 0; *seq != want; spins++) {
        if (tagged && take_tagged_block(hr, want)) break;
        if (spins == 0) MPC_COUNT(waits, 1);          /* not complete at the first look */
        __builtin_ia32_pause();
        if ((spins & 0xFFFF) == 0xFFFF && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) { seen = false; break; }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return seen;
}

/* the sticky word a bounded wait inside a persistent launch sets when it gives up: read (the stream has been waited for, or the verdict
 * is in), and cleared on the mirror's stream */
int read_timeout_word(tqgpu_solver *s, unsigned &tmo) {
    HIP_TRY(hipMemcpy(&tmo, s->persist.psync.timeout, sizeof(unsigned), hipMemcpyDeviceToHost));
    return TQGPU_OK;
}
int clear_timeout_word(tqgpu_solver *s) {
    HIP_TRY(hipMemsetAsync(s->persist.psync.timeout, 0, sizeof(unsigned), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return TQGPU_OK;
}

void fill_result(tqgpu_result *res, const Ctrl &c, int launches, double device_seconds) {
    res->status = c.status; res->iter = c.iter; res->ls_total = c.ls_total; res->ls_last = c.ls_last;
    res->n_launches = launches; res->device_time = device_seconds; res->last_error_norm = c.err; res->last_fval = c.fval;
}

int read_ctrl(tqgpu_solver *s) {
    if (s->route == Route::THREE_LAUNCH && s->w3.mirror && !s->w3.tail_sg) {
        /* the last launch enqueued does not post (the first sweep of a solve whose chunk launches nothing else): a one-thread launch does */
        W3 w = next_w3(s);
        w.hm = s->h_res; s->w3.wait = w.tag; s->w3.tail_sg = true;
        hipLaunchKernelGGL(k_w3_post, dim3(1), dim3(WAVE), 0, s->stream, s->D, w);
    }
    if (s->route == Route::THREE_LAUNCH && s->w3.mirror && s->w3.tail_sg) {
        /* three-launch family: the last launch enqueued posts the control block to pinned memory itself (w3_mirror) */
        if (await_result_block(s->h_res, s->w3.wait, false)) { s->w3.seen = true; return TQGPU_OK; }      /* h_ctrl IS the block's control block */
    }
    s->w3.seen = false;
    HIP_TRY(hipMemcpyAsync(s->h_ctrl, s->D.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    MPC_COUNT(copies, 1); MPC_COUNT(waits, 1);
    return TQGPU_OK;
}

/* persistent launch: wait for the result block the top workgroup writes into pinned host memory (the
 * kernel may still be writing the state back -- everything else the host does is stream-ordered behind it) */
int wait_result_block(tqgpu_solver *s) {
    if (await_result_block(s->h_res, s->persist.psync.seq, true)) return TQGPU_OK;
    /* no verdict (a wait inside the kernel timed out, or the launch failed): fall back to the stream.  A member of a
     * batch launch first waits for THAT launch (it runs on the lead's stream; the member's own stream is not ordered
     * behind it, and its control block is only final when the launch has ended) */
    if (s->links.batch_stream) HIP_TRY(hipStreamSynchronize(s->links.batch_stream));
    return read_ctrl(s);
}

}  // namespace

#ifdef TQ_HOSTPROF
#include <chrono>
static double hp_acc[4] = {0, 0, 0, 0}; static long hp_n = 0;
#define HP_NOW() std::chrono::steady_clock::now()
#define HP_US(a, b) std::chrono::duration<double, std::micro>((b) - (a)).count()
#endif

namespace {

/* A solve in two halves, so that several mirrors can have their (single) persistent launch in flight at the
 * same time (tqgpu_solve_batch): solve_begin enqueues everything up to and including the first launch,
 * solve_end waits for the verdict, runs whatever is left (extra line-search trials, relaunches, the whole
 * Newton loop on the non-persistent paths) and fills the result. */
/* THE list of solve-time switches: read from the environment once per public call that reaches solve_begin (tqgpu_solve, tqgpu_solve_batch),
 * not once per member or per redo -- a getenv is a scan of the environment: two dozen of them per batch call of seven members were
 * microseconds of a 125 us step */
struct SolveEnv { int stamps = 0; bool no_w3_mirror = false, batch_launches = false, batch_sync = false; };
SolveEnv read_solve_env(bool batch) {
    SolveEnv e;
    const char *st = getenv("TREEQP_AMD_STAMPS");
    e.stamps = st ? std::max(1, atoi(st)) : 0;                                /* Opts::stamps: diagnostic in-kernel time stamps */
    e.no_w3_mirror = getenv("TREEQP_AMD_NO_W3_MIRROR") != nullptr;            /* (A/B and tests) three-launch family: copy + synchronisation per read, HIP events per solve, as before */
    if (!batch) return e;
    e.batch_launches = getenv("TREEQP_AMD_BATCH_LAUNCHES") != nullptr;        /* one launch per tree, the round-1 protocol */
    e.batch_sync = getenv("TREEQP_AMD_BATCH_SYNC") != nullptr;                /* every call waits for the end of its batch launches (hand_over) */
    return e;
}

struct SolveCtx {
    Opts O;
    int launches = 0, ring = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Route route = Route::PER_PHASE;  /* decided by the caller: route_of(s, o, false) for a solve on its own, batch_route for a member of a batch */
    SolveEnv env;
    bool phases = false, events = true;
    unsigned batch_seq = 0;          /* != 0: this solve's persistent launch is part of a batch launch the caller makes with this launch number */
#ifdef TQ_HOSTPROF
    std::chrono::steady_clock::time_point hp0, hp1, hp2;
#endif
    SolveCtx() = default;
    SolveCtx(const SolveEnv &e, Route r) : route(r), env(e) {}
};

int grow_events(std::vector<hipEvent_t> &v, int n) {
    while ((int)v.size() < n) { hipEvent_t ev; HIP_TRY(hipEventCreate(&ev)); v.push_back(ev); }
    return TQGPU_OK;
}

/* solve_begin, every route: the options, the time records, the ring slot of the event pair, how the verdict will travel (w3_mirror),
 * and the first event.  in_batch_launch: the solve's launch is made by the caller, on the lead's stream */
int prepare_solve(tqgpu_solver *s, const tqgpu_opts *o, SolveCtx &cx, bool in_batch_launch) {
    HIP_TRY(hipSetDevice(s->device));
    s->out.invalidate();
    s->sens.invalidate(); s->sens.dirty = false;          /* (not problem_changed: the data stays) a stored sensitivity belongs to the point of the solve before this one; point and data belong together again */
    if (opts_from(o, cx.O) != TQGPU_OK) return TQGPU_EINVAL;
    cx.O.stamps = cx.env.stamps;

    if (s->shard.on && !s->shard.comm) return fail(TQGPU_ECOMM, "sharded mirror without a communicator: use tqgpu_solve_virtual_ranks");

    /* ls_log needs no reset: entry i is written by iteration i */

    int rc;
    if (o->profile && (rc = grow_events(s->tm.iter_ev, o->maxIter + 1)) != TQGPU_OK) return rc;
    /* (the per-iteration / per-phase time records are all-NaN unless a profiled solve has written into them: not refilled per solve) */
    const size_t n_it = (size_t)std::max(o->maxIter, 1);
    if (s->tm.times_dirty || s->tm.iter_times.size() != n_it) s->tm.iter_times.assign(n_it, NAN);

    s->route = cx.route;
    cx.phases = o->profile >= 3;
    if (cx.phases) {
        if ((rc = grow_events(s->tm.phase_ev, 4 * (o->maxIter + 1))) != TQGPU_OK) return rc;
        if (!s->tm.sweep_ev0) { HIP_TRY(hipEventCreate(&s->tm.sweep_ev0)); HIP_TRY(hipEventCreate(&s->tm.sweep_ev1)); }
    }
    if (s->tm.times_dirty || s->tm.phase_times.size() != 3 * n_it) s->tm.phase_times.assign(3 * n_it, NAN);
    s->tm.first_sweep_time = NAN;
    s->tm.times_dirty = o->profile != 0;
    cx.ring = (int)(s->solve_no % EV_RING);
    cx.ev0 = s->tm.ring_ev0[cx.ring]; cx.ev1 = s->tm.ring_ev1[cx.ring];
    s->solve_no++;
    /* the event pair costs two more packets on the queue per solve; a single persistent launch reports its own clock (launch
     * start to verdict) anyway, so there the pair is optional */
    /* the three-launch family reports through the pinned result block as well (launches of k_sg / k_sgp post the control block and
     * their own clock: w3_mirror) */
    s->w3.mirror = cx.route == Route::THREE_LAUNCH && !o->profile && !cx.env.no_w3_mirror;
    s->w3.seen = false;
    if (s->w3.mirror) s->h_res->seq = 0;          /* (no launch of this mirror is in flight) */
    cx.events = (s->tm.ev_timing || (!single_launch(cx.route) && !s->w3.mirror)) && !cx.batch_seq && !in_batch_launch;      /* (a member of a batch launch: the launch is on the lead's stream, an event pair on the member's own would time nothing) */
    s->tm.ring_ok[(size_t)cx.ring] = cx.events ? 1 : 0;
    if (cx.events) HIP_TRY(hipEventRecord(cx.ev0, s->stream));
    return TQGPU_OK;
}

/* solve_begin, every route: what a first solve or changed data ask for, and the stage solver's step counters */
int enqueue_setup(tqgpu_solver *s, SolveCtx &cx, const GItem *defer) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    if (s->need_init && cx.route != Route::SINGLE_WG) {     /* g_persist recomputes the reciprocal weights itself; dense nodes never read theirs */
        const int nxu = std::max(s->sum_nx, s->sum_nu);
        hipLaunchKernelGGL(k_init, dim3((nxu + 255) / 256), dim3(256), 0, st, s->sum_nx, s->sum_nu, D); cx.launches++;
        s->need_init = false;
        s->links.stream_pending = true;
    }
    /* tqgpu_get_stage_steps: per solve.  (A dense member of a batch launch: that launch is on the lead's stream and resets the counters in its own
     * prologue, g_persist_dense_batch -- a memset on this stream would have to be waited for, once per member and call) */
    if (s->sk.gen && s->rows.d_steps && !(defer && s->sk.dense)) HIP_TRY(hipMemsetAsync(s->rows.d_steps, 0, (sizeof(long) + sizeof(int)) * (size_t)T.Nn, st));
    if (s->sk.dense && s->sk.need_dense_init) {
        hipLaunchKernelGGL(k_dense_init, dim3(T.Nn), dim3(WAVE), s->sk.lds_dense, st, T, D); cx.launches++;
        s->sk.need_dense_init = false;
        if (defer) s->links.stream_pending = true;      /* the batch launch on the lead's stream waits for it (join_lead_stream): first solves and changed data only */
    }
    return TQGPU_OK;
}

/* TIERED, THREE_LAUNCH, FUSED_TAILS, PER_PHASE: control block, starting duals and the first sweep; solve_end enqueues the iterations */
int begin_enqueued(tqgpu_solver *s, SolveCtx &cx) {
    const Tree &T = s->T; const Data &D = s->D; hipStream_t st = s->stream;
    const bool w3 = cx.route == Route::THREE_LAUNCH;
    /* the three-launch family with k_sgp: the first launch of the solve takes the starting duals and resets the control block itself */
    const bool fresh = w3 && s->w3.sgp;
    if (!fresh) HIP_TRY(hipMemsetAsync(D.ctrl, 0, sizeof(Ctrl), st));     /* persistent path: reset by the launch's prologue */
    int rc = enqueue_setup(s, cx, nullptr);
    if (rc != TQGPU_OK) return rc;
    /* the current buffer is lam0 at the start of every solve */
    if (!fresh) HIP_TRY(hipMemcpyAsync(D.lam0, s->d_lam_init, sizeof(double) * (size_t)s->sum_nx, hipMemcpyDeviceToDevice, st));
    /* first sweep at lambda0 (phase S of iteration 0 + fval0); the persistent launch does it as its prologue */
    if (cx.phases) HIP_TRY(hipEventRecord(s->tm.sweep_ev0, st));
    if (w3) { launch_sg(s, cx.O, 0, 0, 0, fresh); cx.launches++; }          /* with fval0 and the first termination test as its tail */
    else if (cx.route == Route::FUSED_TAILS) { hipLaunchKernelGGL(k_stage_f, dim3(T.Nn), dim3(WAVE), s->pp.lds_stage, st, T, D, cx.O, next_fuse(s), 0, 0, 0); cx.launches++; }      /* with k_fval_init as its tail */
    else {
        launch_stage_sweep(s, 0, 0, 0); cx.launches++;
        hipLaunchKernelGGL(k_fval_init, dim3(1), dim3(256), 0, st, T, D); cx.launches++;
    }
    if (cx.phases) HIP_TRY(hipEventRecord(s->tm.sweep_ev1, st));
    return TQGPU_OK;
}

/* the parameters of this mirror's single-workgroup launch: g_persist with the plan of setup_single_wg, or, on a dense tree,
 * g_persist_dense with the plan of plan_dense_single (deferred: the same parameters for this member's workgroup of the batch launch) */
GParams gparams_of(const tqgpu_solver *s) {
    GParams gp;
    gp.lvl_first = s->gp.d_lvl_first; gp.lam_init = s->d_lam_init; gp.hres = s->h_res; gp.seq = s->persist.psync.seq; gp.lds_wave = (int)s->gp.lds_wave;
    gp.sum_nx = s->sum_nx; gp.sum_nu = s->sum_nu; gp.sum_W = s->sum_W; gp.sum_Ut = s->sum_Ut; gp.sum_A = s->sum_A; gp.sum_B = s->sum_B;
    gp.small8 = s->gp.small8 ? 1 : 0;
    if (!s->sk.dense) {
        gp.in_lds = s->gp.in_lds ? 1 : 0; gp.tab_in_lds = (!s->gp.in_lds && s->gp.tab_in_lds) ? 1 : 0; gp.const_in_lds = s->gp.const_in_lds ? 1 : 0;
        gp.small16 = s->gp.small16 ? 1 : 0;
        gp.stage_waves = 0; gp.win_stage = 0; gp.win_region = 0; gp.phase_waves = 0;
    } else {
        gp.in_lds = s->gpd.in_lds ? 1 : 0; gp.tab_in_lds = (!s->gpd.in_lds && s->gpd.tab_in_lds) ? 1 : 0; gp.const_in_lds = s->gpd.const_in_lds ? 1 : 0;
        gp.small16 = 0;
        gp.stage_waves = s->gpd.stage_waves; gp.phase_waves = s->gpd.phase_waves; gp.win_stage = (int)s->gpd.win_stage; gp.win_region = (int)s->gpd.win_region;
    }
    return gp;
}

/* SINGLE_WG: the whole solve as one launch of one workgroup, g_persist or g_persist_dense; defer: described there for the caller's batch
 * launch instead.  No wipe when the launch number wraps, unlike launch_persist: one workgroup hands nothing over through sync_slab, and
 * every word of the result block, the only thing the number tags here, is rewritten by every launch */
int begin_single_wg(tqgpu_solver *s, SolveCtx &cx, GItem *defer) {
    (void)step_launch_no(s);
    s->persist.psync.seq = s->persist.launch_no << 16;
    const GParams gp = gparams_of(s);
    if (defer) { defer->T = s->T; defer->D = s->D; defer->G = gp; }           /* launched by the caller, together with the rest of its batch */
    else if (s->sk.dense) hipLaunchKernelGGL(g_persist_dense, dim3(1), dim3(GPD_WAVES * WAVE), s->gpd.lds_total, s->stream, s->T, s->D, cx.O, gp);
    else hipLaunchKernelGGL(g_persist, dim3(1), dim3(GP_WAVES * WAVE), s->gp.lds_total, s->stream, s->T, s->D, cx.O, gp);
    cx.launches++;          /* (also the caller's) */
    return TQGPU_OK;
}

/* PERSIST: the launch with its prologue, or its share of the caller's batch launch (batch_seq) */
int begin_persist(tqgpu_solver *s, SolveCtx &cx) { return launch_persist(s, cx.O, cx.launches, 1, cx.batch_seq); }

/* warm start mode 1 (tqgpu_set_warm_start): the duals of the last solve into the start buffer, on the mirror's own stream ahead of everything the
 * solve enqueues there.  The last solve may have been part of a batch launch on another stream (settle); a launch the caller makes on
 * another stream waits for this one (stream_pending, join_lead_stream).  A batch step does all its members' copies in one launch
 * instead and leaves warm.fresh set. */
int enqueue_warm_start(tqgpu_solver *s, SolveCtx &cx) {
    int rc = settle(s);
    if (rc != TQGPU_OK) return rc;
    return launch_mpc_pre(s, MpcPre{.warm = true}, &cx.launches);
}

/* defer: the solve runs Route::SINGLE_WG as a member of a batch launch -- its launch is described there and made by the caller */
int solve_begin(tqgpu_solver *s, const tqgpu_opts *o, SolveCtx &cx, GItem *defer = nullptr) {
#ifdef TQ_HOSTPROF
    cx.hp0 = HP_NOW();
#endif
    const bool warm = mpc_warm_due(s);          /* (it reads solve_no: before prepare_solve counts this one) */
    s->warm.fresh = false;
    int rc = prepare_solve(s, o, cx, defer != nullptr);
    if (rc != TQGPU_OK) return rc;
    if (warm && (rc = enqueue_warm_start(s, cx)) != TQGPU_OK) return rc;
    /* a tqgpu_mpc_shift of a mirror in mode 0 lent the start buffer to the shifted duals for ONE solve: this one (1 -> 2), or the one before
     * (2: the caller's buffer comes back first, on the mirror's own stream as the warm-start copy; in another mode the buffer is not the caller's) */
    if (s->shift.restore == 1) s->shift.restore = 2;
    else if (s->shift.restore == 2) {
        s->shift.restore = 0;
        if (s->warm.mode == 0 && s->shift.d_keep) {
            if ((rc = settle(s)) != TQGPU_OK) return rc;
            HIP_TRY(hipMemcpyAsync(s->d_lam_init, s->shift.d_keep, sizeof(double) * (size_t)s->sum_nx, hipMemcpyDeviceToDevice, s->stream)); MPC_COUNT(copies, 1);
            s->lam_valid = false;
            s->links.stream_pending = true;
        }
    }
    if (!single_launch(cx.route)) return begin_enqueued(s, cx);
    if ((rc = enqueue_setup(s, cx, defer)) != TQGPU_OK) return rc;
#ifdef TQ_HOSTPROF
    cx.hp1 = HP_NOW();
#endif
    rc = cx.route == Route::SINGLE_WG ? begin_single_wg(s, cx, defer) : begin_persist(s, cx);
    if (rc != TQGPU_OK) return rc;
    /* the launch normally ends the solve: close the timing here */
    if (cx.events) HIP_TRY(hipEventRecord(cx.ev1, s->stream));
#ifdef TQ_HOSTPROF
    cx.hp2 = HP_NOW();
#endif
    return TQGPU_OK;
}

/* the line search of iteration h_ctrl->iter wants more trials than were enqueued: batches of them, a read-back after each, until it
 * is decided.  `any`: at least one trial went out */
int run_extra_trials(tqgpu_solver *s, const Opts &O, Route trials, int &launches, bool &any) {
    /* trials beyond the first go out in batches: 3, then 6, 12, 16, .. per read-back of the control block.  A trial that is
     * accepted turns the rest of its batch into no-ops (~6 us each), so short searches -- the usual case: one or two more
     * trials -- want small batches (one C5-class tree: 1.09 ms with batches of 8, 0.99 ms with 3), long ones few read-backs. */
    const int trial_batch0 = process_switches().trial_batch;
    int trial_batch = trial_batch0, ls_of = -1;
    any = false;
    while (!s->h_ctrl->done && s->h_ctrl->ls_pending) {
        any = true;
        /* the line search of iteration `iter` wants more trials: a batch of them */
        const int it = s->h_ctrl->iter, t0 = s->h_ctrl->ls_iter;
        if (it != ls_of) { ls_of = it; trial_batch = trial_batch0; }
        for (int t = t0; t < t0 + trial_batch && t <= O.lsMaxIter; t++) {
            s->w3.post_next = t + 1 >= t0 + trial_batch || t + 1 > O.lsMaxIter;      /* the last of the batch */
            int rcx = launch_trial(s, O, trials, it, t, launches);
            if (rcx != TQGPU_OK) return rcx;
        }
        trial_batch = std::min(2 * trial_batch, 16);
        int rc = read_ctrl(s);
        if (rc != TQGPU_OK) return rc;
    }
    return TQGPU_OK;
}

/* solve_end of PERSIST and SINGLE_WG: solve_begin made the launch; the verdict comes through the result block in pinned host memory.
 * (route_of gives these routes only with profile == 0 and maxIter > 0: no iteration events, no empty solve.)
 * tail_done: that one launch was the whole solve */
int end_single_launch(tqgpu_solver *s, SolveCtx &cx, bool &tail_done) {
    const Route route = cx.route;
    /* (a persistent launch that ends inside a line search leaves its further trials to the tiered kernels, where the tree has them) */
    const Route trials = route == Route::PERSIST && tiered_capable(s) ? Route::TIERED : route;
    for (bool relaunch = false;; relaunch = true) {
        if (relaunch) {
            if (route == Route::SINGLE_WG) return fail(TQGPU_ENODEVICE, "single-workgroup persistent kernel ended without a verdict");
            int rcx = launch_persist(s, cx.O, cx.launches, 0);          /* no prologue: the state is in global memory */
            if (rcx != TQGPU_OK) return rcx;
            if (cx.events) HIP_TRY(hipEventRecord(cx.ev1, s->stream));
        }
        int rc = wait_result_block(s);
        if (rc != TQGPU_OK) return rc;
#ifdef TQ_HOSTPROF
        { auto hp3 = HP_NOW(); hp_acc[0] += HP_US(cx.hp0, cx.hp1); hp_acc[1] += HP_US(cx.hp1, cx.hp2); hp_acc[2] += HP_US(cx.hp2, hp3); hp_n++;
          if (hp_n % 200 == 0) { fprintf(stderr, "[hostprof] pre %.2f us, launch %.2f us, readback+sync %.2f us (avg of %ld)\n", hp_acc[0] / hp_n, hp_acc[1] / hp_n, hp_acc[2] / hp_n, hp_n); } }
#endif
        bool extra_trials = false;
        if ((rc = run_extra_trials(s, cx.O, trials, cx.launches, extra_trials)) != TQGPU_OK) return rc;
        tail_done = !extra_trials;
        if (s->h_ctrl->done) return TQGPU_OK;
        tail_done = false;
        if (route == Route::PERSIST) {
            unsigned tmo = 0;
            if ((rc = read_timeout_word(s, tmo)) != TQGPU_OK) return rc;
            if (tmo) return fail(TQGPU_ETIMEOUT, "persistent solve kernel: a bounded inter-workgroup wait timed out");
        }
    }
}

/* solve_end of TIERED, THREE_LAUNCH, FUSED_TAILS and PER_PHASE.  host_iter: iterations whose event was recorded */
int end_enqueued(tqgpu_solver *s, const tqgpu_opts *o, SolveCtx &cx, int &host_iter) {
    const Opts &O = cx.O;
    hipStream_t st = s->stream;
    const Route route = cx.route;
    const bool generic = route != Route::TIERED;      /* generic: launch_generic_iteration */
    int &launches = cx.launches;
    /* Newton loop (dual_Newton_tree.c:1166-1228).  The device decides (termination, Armijo);
     * the host enqueues `chunk` tagged iterations ahead and reads the control block once per chunk.
     * Iterations enqueued beyond convergence, or while a line search still needs trials, are
     * no-ops by their phase guards. */
    int h = 0, ev_idx = 0;
    bool finished = o->maxIter <= 0;       /* nothing to iterate: reported as "maximum iterations" */
    if (finished) { HIP_TRY(hipStreamSynchronize(st)); memset(s->h_ctrl, 0, sizeof(Ctrl)); s->h_ctrl->status = 1; }
    if (o->profile) HIP_TRY(hipEventRecord(s->tm.iter_ev[0], st));
    int chunk = s->last_iter > 0 ? std::min(s->last_iter + 1, 16) : s->pp.chunk;
    bool predicted = s->last_iter > 0 && generic;     /* the chunk is a prediction: its last iteration should only find convergence */
    /* a line search that wants a second trial turns everything enqueued behind it into no-ops (~3 us a launch): a problem that
     * backtracked last time is fed two iterations at a time (TREEQP_AMD_LS_CHUNK; one C5-class tree: 1.15 ms with chunks of 8, 1.04 / 1.01 / 1.06 ms with 4 / 2 / 1),
     * a read-back per chunk instead */
    const int ls_chunk = process_switches().ls_chunk;
    if (s->last_ls_extra && generic && chunk > ls_chunk && !(route == Route::THREE_LAUNCH && !s->pp.ls_pred.empty())) { chunk = ls_chunk; predicted = false; }      /* (three-launch family: the further trials are predicted too) */
    if (cx.phases) { chunk = 1; predicted = false; }            /* phase timing: one iteration per read-back, so that every recorded event belongs to work that ran */
    int rest_due = -1;                                          /* iteration whose termination test ran, whose step did not */
    while (!finished) {
        const int n = std::min(chunk, o->maxIter - h);
        int deferred = -1;
        for (int i = 0; i < n; i++) {
            if (route == Route::TIERED) { int rcx = launch_fast_iteration(s, O, h + i, launches); if (rcx != TQGPU_OK) return rcx; }
            else {
                int parts = 3;
                if (rest_due == h + i) parts &= ~1;                                   /* its test already ran */
                if (predicted && i == n - 1) { parts &= ~2; deferred = h + i; }
                /* (three-launch family: the last iteration of the chunk that launches anything posts the verdict to the host) */
                const bool last = i == n - 1 || (predicted && i == n - 2);
                if (parts) launch_generic_iteration(s, O, h + i, launches, parts, cx.phases, last);
            }
            if (o->profile && ev_idx + 1 < (int)s->tm.iter_ev.size()) HIP_TRY(hipEventRecord(s->tm.iter_ev[++ev_idx], st));
        }
        int rc = read_ctrl(s);
        if (rc != TQGPU_OK) return rc;
        bool extra_trials = false;
        if ((rc = run_extra_trials(s, O, route, launches, extra_trials)) != TQGPU_OK) return rc;
        h = s->h_ctrl->iter;
        finished = s->h_ctrl->done != 0;
        chunk = cx.phases ? 1 : s->pp.chunk;
        predicted = false;
        /* the termination test of the deferred iteration was enqueued behind the FIRST trial of the line search before it: when that
         * line search needed further trials (enqueued above, after the read-back), the test found the search pending and did nothing --
         * it is then due again with the rest of its iteration */
        rest_due = (!finished && deferred == h && !extra_trials) ? h : -1;
    }
    host_iter = ev_idx;
    return TQGPU_OK;
}

/* the device time of the solve [ms], by what is known without waiting: the three-launch mirror's clock, the event pair or the last
 * launch's clock (these two wait for the stream), the single launch's clock */
int solve_device_ms(tqgpu_solver *s, const tqgpu_opts *o, const SolveCtx &cx, bool tail_done, float &ms) {
    hipStream_t st = s->stream;
    if (!tail_done && cx.route == Route::THREE_LAUNCH && s->w3.mirror && s->w3.seen && !cx.events && !o->profile && !cx.phases) {
        /* three-launch family: every launch of the solve is accounted for (the last one's tail has posted the verdict; what its other
         * workgroups still write is stream-ordered before anything the host does next): no synchronisation, the device's own clock */
        unsigned long long t_first;
        memcpy(&t_first, &s->h_ctrl->pad0, sizeof(t_first));
        ms = 1e-5f * (float)(s->h_res->t_end - t_first);
    } else if (!tail_done) {
        if (cx.events) HIP_TRY(hipEventRecord(cx.ev1, st));
        HIP_TRY(hipStreamSynchronize(st));
        MPC_COUNT(waits, 1);
        if (cx.events) HIP_TRY(hipEventElapsedTime(&ms, cx.ev0, cx.ev1));
        else ms = 1e-5f * (float)(s->h_res->t_end - s->h_res->t_start);      /* several persistent launches (relaunch): the last one's own clock */
    } else {
        /* single persistent launch: the kernel's own clock, launch start to verdict (the event pair of this
         * solve can be read later through tqgpu_get_device_times, which synchronises) */
        ms = 1e-5f * (float)(s->h_res->t_end - s->h_res->t_start);
    }
    return TQGPU_OK;
}

/* solve_end, every route: device time, the time records of a profiled solve, the result, and what the next solve of this mirror predicts from */
int finish_solve(tqgpu_solver *s, const tqgpu_opts *o, SolveCtx &cx, tqgpu_result *res, bool tail_done, int host_iter) {
    hipStream_t st = s->stream;
    float ms = 0.f;
    int rc = solve_device_ms(s, o, cx, tail_done, ms);
    if (rc != TQGPU_OK) return rc;
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(TQGPU_ENODEVICE, std::string("kernel launch failed: ") + hipGetErrorString(le));

    if (cx.phases) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, s->tm.sweep_ev0, s->tm.sweep_ev1) == hipSuccess) s->tm.first_sweep_time = 1e-3 * t;
        for (int i = 0; i < host_iter && (size_t)(4 * i + 3) < s->tm.phase_ev.size() && (size_t)(3 * i + 2) < s->tm.phase_times.size(); i++)
            for (int ph = 0; ph < 3; ph++)
                if (hipEventElapsedTime(&t, s->tm.phase_ev[(size_t)(4 * i + ph)], s->tm.phase_ev[(size_t)(4 * i + ph + 1)]) == hipSuccess) s->tm.phase_times[(size_t)(3 * i + ph)] = 1e-3 * t;
    }
    if (o->profile) {
        for (int i = 0; i < host_iter && i + 1 < (int)s->tm.iter_ev.size() && i < (int)s->tm.iter_times.size(); i++) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, s->tm.iter_ev[i], s->tm.iter_ev[i + 1]) == hipSuccess) s->tm.iter_times[i] = 1e-3 * t;
        }
    }
    const Ctrl &c = *s->h_ctrl;
    fill_result(res, c, cx.launches, 1e-3 * ms);
    s->last_iter = c.iter;
    s->last_ls_extra = c.ls_total > c.iter ? 1 : 0;
    if (cx.route == Route::THREE_LAUNCH && s->w3.merge && c.status == 2 && s->T.Np > 1) {
        /* NOT_DESCENT_DIRECTION out of the merged launch (k_sgp mode 2: forward sweep + first trial): the trial sweep ran before the
         * direction test and has put x, u, xUnc, QinvCal of the point lambda + dlambda in place.  The reference returns from
         * line_search with the phase-S iterate at lambda (dual_Newton_tree.c:944-954): one stage sweep at the current duals (which the
         * trial did not touch: it wrote the other buffer) restores exactly that -- same arithmetic, operation for operation. */
        hipLaunchKernelGGL(k_stage, dim3(s->T.Nn), dim3(WAVE), s->pp.lds_stage, st, s->T, s->D, 0, 0, 0);
        res->n_launches = ++cx.launches;
        s->links.stream_pending = true;
    }
    if (cx.route == Route::THREE_LAUNCH) {
        s->pp.ls_pred.clear();
        if (c.status == 0 && c.ls_total > c.iter) {
            /* some iteration needed further trials: fetch the trial counts (only then: a copy is a packet on the queue and a synchronisation) */
            const int nlog = std::min(c.iter, std::min(s->ls_log_cap, 256));
            HIP_TRY(hipMemcpyAsync(s->h_ls_log, s->D.ls_log, sizeof(int) * (size_t)nlog, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            MPC_COUNT(copies, 1); MPC_COUNT(waits, 1);
            s->pp.ls_pred.assign(s->h_ls_log, s->h_ls_log + nlog);
        }
    }
    return TQGPU_OK;
}

int solve_end(tqgpu_solver *s, const tqgpu_opts *o, SolveCtx &cx, tqgpu_result *res) {
    HIP_TRY(hipSetDevice(s->device));
    bool tail_done = false;
    int host_iter = 0;
    const int rc = single_launch(cx.route) ? end_single_launch(s, cx, tail_done) : end_enqueued(s, o, cx, host_iter);
    if (rc != TQGPU_OK) return rc;
    return finish_solve(s, o, cx, res, tail_done, host_iter);
}

}  // namespace

/* A persistent launch needs all its workgroups resident at once; that was checked at creation against THIS process's launches.
 * When something else holds compute units (another process, another stream), a bounded wait inside the launch gives up after
 * 0.5 s and the launch ends itself.  That is not an error of the solve: clear the sticky word, and redo the solve from the
 * same starting duals on the path that has no residency requirement (launch per tier, or per level).  The mirror keeps off
 * the persistent path for the next `PERSIST_BACKOFF` solves, then tries it again. */
constexpr int PERSIST_BACKOFF = 1000;

static int solve_after_timeout(tqgpu_solver *s, const tqgpu_opts *o, const SolveEnv &env, tqgpu_result *res) {
    if (int rc = clear_timeout_word(s)) return rc;
    s->persist.use = 0;
    s->persist.backoff = PERSIST_BACKOFF;
    s->persist.n_timeouts++;
    if (getenv("TREEQP_AMD_VERBOSE")) fprintf(stderr, "[treeqp_amd] persistent launch timed out (device shared?): solving on the launch-per-tier path\n");
    s->warm.fresh = true;                              /* from the same starting duals: the start buffer holds them, whatever the warm-start mode */
    if (s->shift.restore == 2) s->shift.restore = 1;   /* (... also where tqgpu_mpc_shift put them there for this solve) */
    SolveCtx cx(env, route_of(s, o, false));          /* a fresh decision: persist.use is off now */
    int rc = solve_begin(s, o, cx);
    if (rc != TQGPU_OK) return rc;
    return solve_end(s, o, cx, res);
}

static int enqueue_export(tqgpu_solver *s, const double *lamc, bool download = true);      /* tdunes_kkt.hpp */

extern "C" int tqgpu_solve(tqgpu_solver *s, const tqgpu_opts *o, tqgpu_result *res) {
    SETTLE(s);
    if (!s || !o || !res) return fail(TQGPU_EINVAL, "tqgpu_solve: bad arguments");
    /* a mirror that is one rank's share of a sharded solve launches only that share: on its own it would time out, and its launch number
     * would fall out of step with its peers' */
    if (s->pshard.on && s->shard.nranks > 1) return fail(TQGPU_EINVAL, "tqgpu_solve: this mirror is rank " + std::to_string(s->shard.rank) + " of a sharded solve (tqgpu_pshard_init): use tqgpu_pshard_begin / _end");
    if (s->persist.backoff > 0 && --s->persist.backoff == 0) s->persist.use = s->persist.use_orig;
    SolveCtx cx(read_solve_env(false), route_of(s, o, false));
    int rc = solve_begin(s, o, cx);
    if (rc != TQGPU_OK) return rc;
    const int launches0 = cx.launches;
    /* a caller that always fetches the solution (the drop-in front end): the packing kernel and the download go out behind the single
     * persistent launch now, while it runs, instead of after its verdict has travelled to the host and back (a launch latency, the
     * launch's write-back tail and a synchronisation off the caller's critical path); which dual buffer is current is the device's
     * knowledge.  Valid if that one launch was the whole solve. */
    const bool ahead = s->out.ahead && single_launch(cx.route) && !s->pshard.on && !s->shard.on;          /* (solve_begin has made the launch) */
    if (ahead && enqueue_export(s, nullptr) != TQGPU_OK) return TQGPU_ENODEVICE;
    rc = solve_end(s, o, cx, res);
    if (rc == TQGPU_ETIMEOUT) rc = solve_after_timeout(s, o, cx.env, res);
    else if (rc == TQGPU_OK && ahead && res->n_launches == launches0) s->out.packed_and_downloading();
    return rc;
}

/* n solves of the same problem from the same starting duals, one after the other (each waits for its verdict), as the reference's
 * drivers time the solver (`for (jj = 0; jj < NREP; jj++) treeqp_tdunes_solve(...)`, examples/spring_mass_dual_newton_tree.c:135-140):
 * the loop is in C, so what is timed is the solver and not the caller's interpreter.  res = the last solve's result; sums over
 * the n solves in iter_sum / ls_sum / launch_sum.  Stops at the first solve that does not end with status 0 or 1. */
extern "C" int tqgpu_solve_n(tqgpu_solver *s, const tqgpu_opts *o, int n, tqgpu_result *res, long *iter_sum, long *ls_sum, long *launch_sum) {
    SETTLE(s);
    if (!s || !o || !res || n < 1) return fail(TQGPU_EINVAL, "tqgpu_solve_n: bad arguments");
    long it = 0, ls = 0, la = 0;
    /* (waiting for the stream to drain, or a few microseconds, before the next launch measured slower than launching at once) */
    for (int i = 0; i < n; i++) {
        const int rc = tqgpu_solve(s, o, res);
        if (rc != TQGPU_OK) return rc;
        it += res->iter; ls += res->ls_total; la += res->n_launches;
        if (res->status != 0 && res->status != 1) break;
    }
    if (iter_sum) *iter_sum = it;
    if (ls_sum) *ls_sum = ls;
    if (launch_sum) *launch_sum = la;
    return TQGPU_OK;
}

/* diagnostic / test support: a foreign kernel that holds compute units.  `blocks` workgroups of 256 threads, each claiming `lds_kb`
 * KiB of LDS (160 = a whole CU each), spin for `ms` milliseconds of wall clock (at most 3000) on a stream of their own; the call
 * returns at once.  tqgpu_debug_occupy_wait() waits for them.  Used by the tests to take co-residency away from a persistent launch. */
namespace {
__global__ void __launch_bounds__(256) k_occupy(unsigned long long ticks, int *sink) {
    extern __shared__ __attribute__((aligned(16))) double lds_occ[];
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) lds_occ[0] = 1.0;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (lds_occ[0] == 2.0 && sink) *sink = 1;
}
hipStream_t g_occ_stream = nullptr;
}
extern "C" int tqgpu_debug_occupy(int device, int blocks, int lds_kb, int ms) {
    if (blocks < 1 || lds_kb < 0 || lds_kb > 160 || ms < 1) return fail(TQGPU_EINVAL, "tqgpu_debug_occupy: bad arguments");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    if (!g_occ_stream) {
        /* a stream of another PRIORITY than the solvers': the runtime deals streams of one priority over a handful of hardware queues, and
         * two streams that share a queue run their kernels one after the other -- the occupying kernel would then hold back the very launch
         * it is meant to run beside (one test run in four, depending on how many mirrors the process had created before) */
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&g_occ_stream, hipStreamNonBlocking, greatest));
    }
    const size_t lds = (size_t)lds_kb * 1024;
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_occupy), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_occupy, dim3((unsigned)blocks), dim3(256), lds, g_occ_stream, (unsigned long long)std::min(ms, 3000) * 100000ull, (int *)nullptr);
    HIP_TRY(hipGetLastError());
    return TQGPU_OK;
}
extern "C" int tqgpu_debug_occupy_wait(void) {
    if (g_occ_stream) HIP_TRY(hipStreamSynchronize(g_occ_stream));
    return TQGPU_OK;
}

/* geometry of the persistent launch of this mirror: block levels of the tree, tiers, workgroups of one launch, workgroups of
 * such launches the device holds at once (co-residency: what tqgpu_solve_batch may have in flight together), compute units */
extern "C" int tqgpu_geometry(const tqgpu_solver *s, int *levels, int *tiers, int *workgroups, int *capacity, int *compute_units) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    if (levels) *levels = s->Nh;
    if (tiers) *tiers = s->uni.fast >= 0 ? s->uni.n_tiers : 0;
    if (workgroups) *workgroups = s->persist.ok ? s->persist.geom.G : 0;
    if (capacity) *capacity = s->persist.ok ? s->persist.co_capacity : 0;
    if (compute_units) *compute_units = s->n_cu;
    return TQGPU_OK;
}

/* diagnostic: how often a persistent launch of this mirror timed out and the solve was redone on another path */
extern "C" int tqgpu_timeouts(const tqgpu_solver *s) { return s ? s->persist.n_timeouts : 0; }

/* a block of a batch launch (device array and its pinned host copy, owned by the batch's first mirror): room for `need` units, twice the
 * need where it has to grow (the lead's stream holds nothing that reads it: every batched call ends with its wait) */
template <typename Item, typename Cap>
static int grow_items(tqgpu_solver *s, Item *&d, Item *&h, Cap &cap, size_t need, const char *what = "the batch descriptors") {
    if ((size_t)cap >= need && d) return TQGPU_OK;
    s->mem.release(d); s->mem.release(h);
    cap = 0;
    int rc;
    const size_t units = 2 * std::max<size_t>(need, 1);
    if ((rc = s->mem.device(d, units * sizeof(Item), TQGPU_ENOMEM, what)) || (rc = s->mem.host(h, units * sizeof(Item), what))) return rc;
    cap = (Cap)units;
    return TQGPU_OK;
}

/* ---- the plan of the batched after-solve calls (tqgpu_kkt_residual_batch, tqgpu_mpc_adjoint_batch, tqgpu_mpc_adjoint_matrices_batch, tqgpu_mpc_sensitivity_batch, tqgpu_mpc_predict_batch): per device
 * one group; a group that fits one grid goes out as ONE set of launches on its first member's stream (the lead's), anything else member by member.  A call is its refusals
 * (refuse_members), its offsets into the caller's flat arrays (member_spans), the groups with their routes decided (plan_device_groups) and three callbacks for
 * run_device_groups: a batched group out on its lead's stream, one member alone, a batched group's results out of the lead's pinned block behind the one wait ---- */
struct DeviceGroup { int device; std::vector<int> idx; bool batched = false; };
/* what every member is refused for, before any is touched: refuse(s)'s own message behind "member i: ", then a mirror named twice, then also(i) with a message
 * of its own, member after member */
template <typename Refuse, typename Also>
static int refuse_members(const char *who, tqgpu_solver **v, int n, Refuse refuse, Also also) {
    std::set<const tqgpu_solver *> seen;
    for (int i = 0; i < n; i++) {
        int rc;
        if ((rc = refuse(v[i]))) return fail(rc, "member " + std::to_string(i) + ": " + g_err);
        if (!seen.insert(v[i]).second) return fail(TQGPU_EINVAL, std::string(who) + ": member " + std::to_string(i) + ": a mirror is named twice");
        if ((rc = also(i))) return rc;
    }
    return TQGPU_OK;
}
template <typename Refuse>
static int refuse_members(const char *who, tqgpu_solver **v, int n, Refuse refuse) { return refuse_members(who, v, n, refuse, [](int) { return TQGPU_OK; }); }
/* where every member's blocks begin in the caller's flat arrays: advance(at, i) moves the offsets past member i */
template <typename Span, typename Advance>
static std::vector<Span> member_spans(int n, Advance advance) {
    std::vector<Span> span((size_t)n);
    Span at{};
    for (int i = 0; i < n; i++) { span[(size_t)i] = at; advance(at, i); }
    return span;
}
/* The batched kernels' grids are as wide as the largest member: a group in which one tree dwarfs the others would launch mostly
 * waves that return at once, and goes member by member instead.  mx, the largest member's nodes, n members, sum, the nodes of all of them. */
static bool batch_grid_lopsided(size_t mx, size_t n, size_t sum) { return mx * n > 8 * sum + 4096; }
/* at least min_members, at most as many as the grid dimension that counts the members takes, no mirror twice, not lopsided */
static bool group_fits_one_grid(tqgpu_solver **v, const DeviceGroup &g, int min_members, size_t grid_limit) {
    if (g.idx.size() < (size_t)min_members || g.idx.size() > grid_limit) return false;
    size_t sum = 0, mx = 0;
    std::set<const tqgpu_solver *> seen;
    for (int i : g.idx) {
        if (!seen.insert(v[i]).second) return false;          /* a mirror named twice: two workgroups would reduce (and rewrite) one table */
        sum += (size_t)v[i]->Nn; mx = std::max(mx, (size_t)v[i]->Nn);
    }
    return !batch_grid_lopsided(mx, g.idx.size(), sum);
}
/* the members by device, in the caller's order, every group's route decided before anything goes out.  members_var (TREEQP_AMD_KKT_BATCH,
 * TREEQP_AMD_ADJ_BATCH, TREEQP_AMD_SENS_BATCH) = members, read by every call: every member on its own stream, as a group of one goes */
static std::vector<DeviceGroup> plan_device_groups(tqgpu_solver **v, int n, const char *members_var, int min_members, size_t grid_limit) {
    std::vector<DeviceGroup> groups;
    for (int i = 0; i < n; i++) {
        auto g = std::find_if(groups.begin(), groups.end(), [&](const DeviceGroup &q) { return q.device == v[i]->device; });
        if (g == groups.end()) { groups.push_back(DeviceGroup{v[i]->device, {}}); g = groups.end() - 1; }
        g->idx.push_back(i);
    }
    const char *sw = getenv(members_var);
    const bool by_member = sw && strcmp(sw, "members") == 0;
    for (DeviceGroup &g : groups) g.batched = !by_member && group_fits_one_grid(v, g, min_members, grid_limit);
    return groups;
}
/* THE stream rule of a batched group: member s is about to be read and written on its lead's stream, so whatever may still run for it elsewhere
 * comes first.  A member whose last solve was part of a launch on the lead's stream is ordered by it (settle_stream); one whose launch ran on a
 * stream this call has waited for already (the members of a later wave of the batch solve, behind their lead) needs nothing more; any other
 * launch is waited for (settle).  The member's own stream is waited for only where it may hold work the lead's stream has not seen: uploads
 * (stream_pending), an export that went out ahead, or a solve of its own since this family last drained the stream (`drained_at`, the family's
 * mark: solve_no at which it last knew the stream to hold nothing of the member's solves; set here).  `waited` holds the streams this call has
 * synchronised (a handful), `waits` counts them.
 * Three switches, because the callers' wait counts are pinned and differ:
 *   step_drains   a member whose last solve was a tqgpu_mpc_step_batch's holds nothing anywhere: that call returned behind the post of u[0], which
 *                 went out behind every member's last launch (MpcBatchBuf::drained_at).  The adjoint takes it; the KKT check does not, and waits
 *                 for such a member's own stream once.
 *   skip_waited   a member's own stream that this call has waited for already (as another member's settle_stream) is not waited for again.
 *                 The adjoint takes it; the KKT check synchronises again where that stream also has uploads pending or an export ahead.
 *   behind_wait   the call follows one of this member's that returned behind its wait, with no solve between (the adjoint in H, A, B: adj_need
 *                 guarantees a stored adjoint, which every solve clears): only uploads can be pending.  A launch not yet settled is settled
 *                 uncounted, an export ahead and the solves are not looked at, and the family's mark stays: a member-by-member adjoint does
 *                 not set MpcAdjBatch::drained_at, so the full rule would wait once more here. */
struct LeadOrder { bool step_drains, skip_waited, behind_wait; };
static int order_behind_lead(tqgpu_solver *s, const tqgpu_solver *lead, long &drained_at, LeadOrder rule, std::vector<hipStream_t> &waited, int &waits) {
    auto was_waited_for = [&](hipStream_t t) { return t && std::find(waited.begin(), waited.end(), t) != waited.end(); };
    const bool drained = rule.step_drains && s->solve_no == s->mpcb.drained_at;
    const bool in_launch = s->links.settle_stream != nullptr;          /* its last solve was part of a batch launch that has not been waited for */
    if (rule.behind_wait) SETTLE(s);
    else if (drained || s->links.settle_stream == lead->stream || was_waited_for(s->links.settle_stream)) s->links.settle_stream = nullptr;
    else if (in_launch) { if (s->links.settle_stream != s->stream) { waited.push_back(s->links.settle_stream); waits++; } SETTLE(s); }
    const bool own_solve = !in_launch && !drained && s->solve_no != drained_at;
    const bool own_work = s->links.stream_pending || (!rule.behind_wait && (s->out.valid || own_solve));
    if (s->stream != lead->stream && !(rule.skip_waited && was_waited_for(s->stream)) && own_work) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->links.stream_pending = false;
        waited.push_back(s->stream);
        waits++;
    }
    if (!rule.behind_wait) drained_at = s->solve_no;
    return TQGPU_OK;
}
constexpr LeadOrder KKT_ORDER{false, false, false}, ADJ_ORDER{true, true, false}, ADJMAT_ORDER{false, false, true};
/* THE two phases of a batched after-solve call.  Out: enqueue_group(g, gi) for a batched group (an error waits for the lead's stream first, where drain_on_error),
 * run_member(i) for every member of any other group, to its end behind settle and hipSetDevice.  Back: per batched group the device, ONE wait for the lead's
 * stream, counted into the live MPC record, stream_pending cleared, collect_group(g, gi).  So everything goes out before the first wait of a batched group; a
 * group that goes member by member waits member by member.  The KKT check differs in two ways and says so: alone_collects_later, its run_member only enqueues
 * (and settles, counting, itself) and collect_group is called for the groups that went member by member too, behind no wait of the driver's; waits, where it
 * counts a batched group's wait instead, stream_pending left as it was */
struct GroupRun { bool drain_on_error = true, alone_collects_later = false; int *waits = nullptr; };
template <typename Enqueue, typename Member, typename Collect>
static int run_device_groups(tqgpu_solver **v, const std::vector<DeviceGroup> &groups, GroupRun how, Enqueue enqueue_group, Member run_member, Collect collect_group) {
    int rc;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const DeviceGroup &g = groups[gi];
        if (g.batched) {
            if ((rc = enqueue_group(g, gi))) { if (how.drain_on_error) (void)hipStreamSynchronize(v[g.idx[0]]->stream); return rc; }
        } else for (int i : g.idx) {
            if (!how.alone_collects_later) { SETTLE(v[i]); HIP_TRY(hipSetDevice(v[i]->device)); }
            if ((rc = run_member(i))) return rc;
        }
    }
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const DeviceGroup &g = groups[gi];
        if (!g.batched && !how.alone_collects_later) continue;
        tqgpu_solver *lead = v[g.idx[0]];
        HIP_TRY(hipSetDevice(lead->device));
        if (g.batched) {
            HIP_TRY(hipStreamSynchronize(lead->stream));
            if (how.waits) ++*how.waits; else { MPC_COUNT(waits, 1); lead->links.stream_pending = false; }
        }
        if ((rc = collect_group(g, gi))) return rc;
    }
    return TQGPU_OK;
}
static int launch_persist_batch(tqgpu_solver *lead, const BatchRow *row, const PItem *items, const Opts &O, int n_trees, unsigned seq) {
    const int G = lead->persist.geom.G;
    const ProcessSwitches &ps = process_switches();
    const int batch_nap = ps.has_nap ? ps.nap : nap_for_grid(G * n_trees);     /* the whole launch polls the same memory system */
    static size_t lds_allowed[sizeof(BATCH_ROWS) / sizeof(BATCH_ROWS[0])] = {};      /* per row: the LDS its kernel has been allowed so far */
    if (!row) return fail(TQGPU_EINVAL, "no batch kernel for this shape");
    size_t &allowed = lds_allowed[row - BATCH_ROWS];
    if (allowed < lead->persist.lds) { int rc = allow_lds(row->batch, lead->persist.lds); if (rc != TQGPU_OK) return rc; allowed = lead->persist.lds; }
    hipLaunchKernelGGL(row->batch, dim3((unsigned)(G * n_trees)), dim3(FW * WAVE), lead->persist.lds, lead->stream, items, O, G, seq, batch_nap);
    return TQGPU_OK;
}

/* ---- tqgpu_solve_batch step by step: member table, wave, groups, begin, group launches, end, hand-over ---- */

/* what a batch call knows of one member; everything but the three group flags is decided once per call (plan_members) */
struct BatchMember {
    tqgpu_solver *s;
    Route plan;                  /* route_of(s, o, true): what the waves and the groups are planned with */
    Route alone;                 /* route_of(s, o, false): differs from `plan` only for a tree that is SINGLE_WG as a group member alone (uses_gpersist) */
    const BatchRow *krow;        /* the batch kernel (BATCH_ROWS) this member can go out in under these options, or nullptr */
    int need;                    /* workgroups that have to be resident while it runs */
    bool in_single_wg = false;   /* member of its wave's single-workgroup group (clipping trees: g_persist_batch) ... */
    bool in_dense_wg = false;    /* ... of its wave's dense single-workgroup group (g_persist_dense_batch) ... */
    bool in_persist = false;     /* ... of its wave's persistent group (form_groups) */
    SolveCtx cx;
};
/* THE rule for the route a member runs: a member planned as SINGLE_WG runs it as a member of its wave's single-workgroup group -- the
 * clipping trees' or the dense trees', two kernels -- and a wave has such a group only with at least two members of that kind; without
 * the group it runs what it would run on its own.  Every other plan is the same on its own. */
static Route batch_route(const BatchMember &m) { return m.plan == Route::SINGLE_WG && !m.in_single_wg && !m.in_dense_wg ? m.alone : m.plan; }
/* the group a member goes out in, or nullptr */
template <typename Group>
static Group *group_of(const BatchMember &m, Group &wg, Group &dg, Group &pg) { return m.in_persist ? &pg : m.in_single_wg ? &wg : m.in_dense_wg ? &dg : nullptr; }

static std::vector<BatchMember> plan_members(tqgpu_solver **solvers, int n, const tqgpu_opts *o) {
    std::vector<BatchMember> tab((size_t)n);
    for (int k = 0; k < n; k++) {
        BatchMember &m = tab[(size_t)k];
        tqgpu_solver *s = m.s = solvers[k];
        m.plan = route_of(s, o, true);
        m.alone = m.plan == Route::SINGLE_WG ? route_of(s, o, false) : m.plan;
        m.krow = m.plan == Route::PERSIST && o->checkLastActiveSet != 2 ? find_batch_row(s->uni.fNX, s->uni.fNU, s->uni.fMD, s->uni.mstage) : nullptr;
        /* single-workgroup mirrors do not wait for each other: any number per launch; launch-per-level mirrors go alone */
        /* (a SINGLE_WG plan counts 0 even where batch_route sends the member to a launch-per-level route in the end) */
        m.need = m.plan == Route::PERSIST ? s->persist.geom.G : (m.plan == Route::SINGLE_WG ? 0 : s->persist.co_capacity + 1);
    }
    return tab;
}

/* j of the wave [i, j): mirrors on one device whose persistent launches fit together */
static int wave_end(const std::vector<BatchMember> &tab, int i, const SolveEnv &env) {
    const int n = (int)tab.size(), dev = tab[(size_t)i].s->device;
    int used = 0, j = i;
    for (; j < n; j++) {
        const BatchMember &m = tab[(size_t)j];
        const tqgpu_solver *s = m.s;
        /* separate launches: two workgroups on one CU run at half speed each, so a batch fills the CUs once, not twice, unless a
         * member needs more.  Members that go out together as ONE launch (batch kernel) fill the device up to what is co-resident:
         * a tree's waves are parked at barriers and waits two thirds of the time, and trees that share CUs fill those gaps
         * (C2: 3 trees 72 k it/s, 5 trees 98 k; C1: 22 trees 656 k, 38 trees 922 k). */
        const bool one_launch = m.krow && !env.batch_launches;
        const int cap = (!one_launch && s->n_cu > 0 && m.need <= s->n_cu) ? std::min(s->persist.co_capacity, s->n_cu) : s->persist.co_capacity;
        if (j > i && (s->device != dev || used + m.need > cap)) break;
        used += m.need;
    }
    return j;
}

/* members of a wave that go out as ONE launch on the lead's stream; the lead's mirror owns the descriptor array */
struct BatchGroup {
    std::vector<int> members;          /* indices into the member table, ascending; members[0] is the lead's */
    tqgpu_solver *lead = nullptr;      /* nullptr: the wave has no such group */
    size_t launched = 0;               /* members[0 .. launched) went out in the launch */
};

/* the three groups of the wave [i, j) */
static int form_groups(std::vector<BatchMember> &tab, int i, int j, const SolveEnv &env, BatchGroup &wg, BatchGroup &dg, BatchGroup &pg) {
    /* single-workgroup mirrors of this wave go out as ONE launch (one workgroup per tree) on the first one's stream; the dense ones among
     * them (uses_gpersist: opted in with tqgpu_set_dense_batch_launch) run another kernel and are a group of their own */
    for (int k = i; k < j; k++) if (tab[(size_t)k].plan == Route::SINGLE_WG) (tab[(size_t)k].s->sk.dense ? dg : wg).members.push_back(k);
    if (wg.members.size() < 2) wg.members.clear();
    if (dg.members.size() < 2) dg.members.clear();
    /* persistent mirrors of this wave that share a shape with a batch kernel go out as ONE launch as well */
    const BatchMember *f = nullptr;          /* the first one that has a batch kernel: the others have to match it */
    for (int k = i; k < j; k++) {
        const BatchMember &m = tab[(size_t)k];
        if (!m.krow) continue;
        if (!f) f = &m;
        if (m.krow == f->krow && m.s->persist.geom.G == f->s->persist.geom.G && m.s->persist.lds == f->s->persist.lds && m.s->Nn == f->s->Nn) pg.members.push_back(k);
    }
    if (pg.members.size() < 2 || env.batch_launches) pg.members.clear();      /* (=1: one launch per tree, the round-1 protocol) */
    for (int k : wg.members) tab[(size_t)k].in_single_wg = true;
    for (int k : dg.members) tab[(size_t)k].in_dense_wg = true;
    for (int k : pg.members) tab[(size_t)k].in_persist = true;
    if (!wg.members.empty()) wg.lead = tab[(size_t)wg.members[0]].s;
    if (!dg.members.empty()) dg.lead = tab[(size_t)dg.members[0]].s;
    if (!pg.members.empty()) pg.lead = tab[(size_t)pg.members[0]].s;
    /* (the single-workgroup members describe their launches into the array as they begin) */
    for (BatchGroup *g : {&wg, &dg})
        if (g->lead) if (int rc = grow_items(g->lead, g->lead->gp.d_gitems, g->lead->gp.h_gitems, g->lead->gp.gitems_cap, g->members.size())) return rc;
    return TQGPU_OK;
}

/* before a wave begins: whatever batch launch its members were part of last has ended (settle) */
static int settle_wave(std::vector<BatchMember> &tab, int i, int j, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg) {
    for (int k = i; k < j; k++) {
        const BatchMember &m = tab[(size_t)k];
        const BatchGroup *g = group_of(m, wg, dg, pg);
        /* a member of the previous batch launch that goes out again on the same lead's stream is ordered behind it by that stream */
        if (g && m.s->links.settle_stream == g->lead->stream) { if (k == g->members[0]) m.s->links.settle_stream = nullptr; }
        else SETTLE(m.s);
    }
    return TQGPU_OK;
}

/* the launch number of the persistent group's launch, << 16 (0: no group): one more than any member's */
static int persist_group_seq(std::vector<BatchMember> &tab, const BatchGroup &pg, unsigned &pseq) {
    pseq = 0;
    if (!pg.lead) return TQGPU_OK;
    unsigned mx = 0;
    for (int k : pg.members) mx = std::max(mx, tab[(size_t)k].s->persist.launch_no);
    unsigned nn = mx + 1;
    if (nn > 0xFFFFu) {          /* the 16-bit launch number wraps: see launch_persist */
        HIP_TRY(hipStreamSynchronize(pg.lead->stream));      /* (the previous batch launch's last workgroups are done with the slabs) */
        for (int k : pg.members) {
            tqgpu_solver *s = tab[(size_t)k].s;
            HIP_TRY(hipMemsetAsync(s->persist.sync_slab, 0, s->persist.sync_bytes, s->stream));
            s->links.stream_pending = true;          /* the batch launch (on the lead's stream) waits for the wipe */
        }
        nn = 1;
    }
    pseq = nn << 16;
    return TQGPU_OK;
}

/* the first n members of a group join the launch on the lead's stream: what the others enqueued on their own streams since their
 * last synchronisation (stream_pending: asynchronous uploads, constant packing -- first solves and changed data only) comes before
 * the launch, and until the wave is over the members wait for THAT stream where they would wait for their own (batch_stream;
 * cleared by BatchGuard).  Their later work (solution export) is ordered behind the launch lazily, see hand_over and settle(). */
/* (round 3: no event traffic in the steady state -- a record and a wait per member before the launch and another wait after it
 * were 1.5 ms of an 11.5 ms step with 256 single-workgroup trees, a pair of calls per member and step most of a step with 22 small
 * persistent ones) */
static int join_lead_stream(std::vector<BatchMember> &tab, const BatchGroup &g, size_t n) {
    for (size_t m = 1; m < n; m++) {
        tqgpu_solver *sm = tab[(size_t)g.members[m]].s;
        if (sm->links.stream_pending) { HIP_TRY(hipStreamSynchronize(sm->stream)); sm->links.stream_pending = false; }
    }
    for (size_t m = 0; m < n; m++) tab[(size_t)g.members[m]].s->links.batch_stream = g.lead->stream;
    return TQGPU_OK;
}

/* g_persist_batch over the first n members of the group (those that have begun: solve_begin described each one's launch in the lead's array) */
static int launch_single_wg_group(std::vector<BatchMember> &tab, BatchGroup &wg, size_t n) {
    tqgpu_solver *lead = wg.lead;
    size_t lds_batch = 0;
    for (size_t m = 0; m < n; m++) lds_batch = std::max(lds_batch, tab[(size_t)wg.members[m]].s->gp.lds_total);
    int rc = join_lead_stream(tab, wg, n);
    if (rc != TQGPU_OK) return rc;
    HIP_TRY(hipMemcpyAsync(lead->gp.d_gitems, lead->gp.h_gitems, n * sizeof(GItem), hipMemcpyHostToDevice, lead->stream));
    if (lds_batch > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(g_persist_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_batch));
    hipLaunchKernelGGL(g_persist_batch, dim3((unsigned)n), dim3(GP_WAVES * WAVE), lds_batch, lead->stream, lead->gp.d_gitems, tab[(size_t)wg.members[0]].cx.O);
    wg.launched = n;
    return TQGPU_OK;
}

/* g_persist_dense_batch over the first n members of the dense group: n workgroups of GPD_WAVES waves, the LDS of the largest plan among them
 * (every member's offsets come from its own GParams).  What a member enqueued on its own stream for this solve (k_dense_init after an upload)
 * is waited for by join_lead_stream; in the steady state nothing is, and the call costs no synchronisation per member. */
static int launch_dense_wg_group(std::vector<BatchMember> &tab, BatchGroup &dg, size_t n) {
    tqgpu_solver *lead = dg.lead;
    size_t lds_batch = 0;
    for (size_t m = 0; m < n; m++) lds_batch = std::max(lds_batch, tab[(size_t)dg.members[m]].s->gpd.lds_total);
    int rc = join_lead_stream(tab, dg, n);
    if (rc != TQGPU_OK) return rc;
    HIP_TRY(hipMemcpyAsync(lead->gp.d_gitems, lead->gp.h_gitems, n * sizeof(GItem), hipMemcpyHostToDevice, lead->stream));
    if ((rc = allow_lds(g_persist_dense_batch, lds_batch)) != TQGPU_OK) return rc;      /* (plan_dense_single asked the same of g_persist_dense for every member) */
    hipLaunchKernelGGL(g_persist_dense_batch, dim3((unsigned)n), dim3(GPD_WAVES * WAVE), lds_batch, lead->stream, lead->gp.d_gitems, tab[(size_t)dg.members[0]].cx.O);
    dg.launched = n;
    return TQGPU_OK;
}

/* f_persist_batch over the whole group, with the launch number of persist_group_seq */
static int launch_persist_group(std::vector<BatchMember> &tab, BatchGroup &pg, unsigned pseq) {
    tqgpu_solver *pl = pg.lead;
    const size_t np = pg.members.size();
    if (pl->persist.pitems_cap < (int)np) pl->persist.pitems_key.clear();
    if (int rc = grow_items(pl, pl->persist.d_pitems, pl->persist.h_pitems, pl->persist.pitems_cap, np)) return rc;
    std::vector<unsigned long> key;
    for (int k : pg.members) key.push_back(tab[(size_t)k].s->uid);
    if (key != pl->persist.pitems_key) {
        /* the descriptors are what the single launches pass as kernel arguments; they do not change from solve to solve, so
         * the device copy is refreshed only when the batch is composed of other mirrors than last time */
        HIP_TRY(hipStreamSynchronize(pl->stream));                 /* a previous batch launch may still read the array */
        for (size_t m = 0; m < np; m++) { const tqgpu_solver *sm = tab[(size_t)pg.members[m]].s; pl->persist.h_pitems[m].C = sm->persist.pconst; pl->persist.h_pitems[m].Gm = sm->persist.geom; pl->persist.h_pitems[m].Sy = sm->persist.psync; }
        HIP_TRY(hipMemcpyAsync(pl->persist.d_pitems, pl->persist.h_pitems, np * sizeof(PItem), hipMemcpyHostToDevice, pl->stream));
        pl->persist.pitems_key = key;
    }
    int rc = join_lead_stream(tab, pg, np);
    if (rc != TQGPU_OK) return rc;
    const BatchMember &lead = tab[(size_t)pg.members[0]];
    if ((rc = launch_persist_batch(pl, lead.krow, pl->persist.d_pitems, lead.cx.O, (int)np, pseq)) != TQGPU_OK) return rc;
    pg.launched = np;
    return TQGPU_OK;
}

/* after a wave: the members' later work (solution export, the next solve) runs on their own streams: it has to find the batch launch
 * complete -- every verdict is in, so this waits for the write-back of the last workgroups only, once per batch (sync: after an
 * error, or TREEQP_AMD_BATCH_SYNC), or leaves the wait to the first such use */
static int hand_over(std::vector<BatchMember> &tab, const BatchGroup &g, bool sync) {
    if (!g.launched) return TQGPU_OK;
    if (sync) HIP_TRY(hipStreamSynchronize(g.lead->stream));
    else for (size_t m = 1; m < g.launched; m++) tab[(size_t)g.members[m]].s->links.settle_stream = g.lead->stream;      /* see settle() */
    return TQGPU_OK;
}

/* the per-call state a batch leaves on its members, taken back on EVERY exit: in_batch (see BatchLinks::in_batch) on all of them,
 * batch_stream on those of the current wave (wait_result_block and the redo after a timeout read it while the wave is in flight) */
struct BatchGuard {
    tqgpu_solver **v; int n, w0 = 0, w1 = 0;
    BatchGuard(tqgpu_solver **v_, int n_) : v(v_), n(n_) { for (int i = 0; i < n; i++) v[i]->links.in_batch = true; }
    void wave(int i, int j) { for (int k = w0; k < w1; k++) v[k]->links.batch_stream = nullptr; w0 = i; w1 = j; }
    ~BatchGuard() { wave(0, 0); for (int i = 0; i < n; i++) v[i]->links.in_batch = false; }
};

/* Batched multi-tree solve (the usage pattern of examples/fault_tolerance.c:486-530, one QP per
 * configuration): n independent mirrors, same options.  Mirrors on the persistent path have their launches in
 * flight together, as many at a time as fit on the device at once (every workgroup of a persistent launch must
 * be resident); the others are solved one after the other.  results[i] belongs to solvers[i]; the first error
 * is returned after every started solve has been waited for. */
/* mb: the batch is a batch step (tqgpu_mpc_step_batch), which orders its launch ahead of each wave, posts u[0] behind the wave's launches where
 * it can, and counts what went out; nullptr for tqgpu_solve_batch itself */
struct MpcBatch;
static int mpc_before_wave(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int j, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg);
static int mpc_behind_launches(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int j, int ok_to, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg);
static void mpc_after_wave(MpcBatch &mb, std::vector<BatchMember> &tab, int i, int ok_to, const tqgpu_result *results, const BatchGroup &wg, const BatchGroup &dg, const BatchGroup &pg);
static int solve_batch_impl(tqgpu_solver **solvers, int n, const tqgpu_opts *o, tqgpu_result *results, MpcBatch *mb) {
    if (!solvers || n < 1 || !o || !results) return fail(TQGPU_EINVAL, "tqgpu_solve_batch: bad arguments");
    for (int i = 0; i < n; i++) if (!solvers[i]) return fail(TQGPU_EINVAL, "tqgpu_solve_batch: null mirror");
    for (int i = 0; i < n; i++) if (solvers[i]->pshard.on && solvers[i]->shard.nranks > 1) return fail(TQGPU_EINVAL, "tqgpu_solve_batch: a member is one rank of a sharded solve (tqgpu_pshard_init)");
    BatchGuard guard(solvers, n);
    const SolveEnv env = read_solve_env(true);
    for (int k = 0; k < n; k++) {          /* as tqgpu_solve: a mirror that backed off the persistent path returns to it after PERSIST_BACKOFF solves */
        tqgpu_solver *sk = solvers[k];
        if (sk->persist.backoff > 0 && --sk->persist.backoff == 0) sk->persist.use = sk->persist.use_orig;
    }
    std::vector<BatchMember> tab = plan_members(solvers, n, o);          /* (after the loop above: route_of reads persist.use) */
    int first_err = TQGPU_OK, rc;
    std::string first_msg;
    for (int i = 0, j; i < n && first_err == TQGPU_OK; i = j) {
        j = wave_end(tab, i, env);
        guard.wave(i, j);
        BatchGroup wg, dg, pg;      /* single-workgroup group, dense single-workgroup group, persistent group */
        unsigned pseq = 0;
        if ((rc = form_groups(tab, i, j, env, wg, dg, pg)) || (rc = settle_wave(tab, i, j, wg, dg, pg)) || (rc = persist_group_seq(tab, pg, pseq))) return rc;
        if (mb && (rc = mpc_before_wave(*mb, tab, i, j, wg, dg, pg))) return rc;
        int ok_to = i;
        size_t gi = 0, di = 0;      /* members of the single-workgroup group / of the dense one that have begun */
        for (int k = i; k < j; k++) {
            BatchMember &m = tab[(size_t)k];
            m.cx = SolveCtx(env, batch_route(m));
            if (m.in_persist) m.cx.batch_seq = pseq;
            rc = solve_begin(m.s, o, m.cx, m.in_single_wg ? &wg.lead->gp.h_gitems[gi] : m.in_dense_wg ? &dg.lead->gp.h_gitems[di] : nullptr);
            if (rc != TQGPU_OK) { first_err = rc; first_msg = g_err; break; }
            if (m.in_single_wg) gi++;
            if (m.in_dense_wg) di++;
            ok_to = k + 1;
        }
        if (gi > 0 && (rc = launch_single_wg_group(tab, wg, gi))) return rc;
        if (di > 0 && (rc = launch_dense_wg_group(tab, dg, di))) return rc;
        if (pg.lead && ok_to == j && (rc = launch_persist_group(tab, pg, pseq))) return rc;
        if (mb && (rc = mpc_behind_launches(*mb, tab, i, j, ok_to, wg, dg, pg))) return rc;
        for (int k = i; k < ok_to; k++) {
            tqgpu_solver *sk = solvers[k];
            rc = solve_end(sk, o, tab[(size_t)k].cx, &results[k]);
            if (rc == TQGPU_ETIMEOUT) {
                /* device shared: redone on its own, see tqgpu_solve.  The redo works on the same device state as the batch launch,
                 * whose later workgroups may not even have started: the launch has to be over before the sticky word is cleared */
                if (sk->links.batch_stream) HIP_TRY(hipStreamSynchronize(sk->links.batch_stream));
                rc = solve_after_timeout(sk, o, env, &results[k]);
            }
            if (rc != TQGPU_OK && first_err == TQGPU_OK) { first_err = rc; first_msg = g_err; }
        }
        if (mb) mpc_after_wave(*mb, tab, i, ok_to, results, wg, dg, pg);
        const bool sync = first_err != TQGPU_OK || env.batch_sync;
        if ((rc = hand_over(tab, pg, sync)) || (rc = hand_over(tab, wg, sync)) || (rc = hand_over(tab, dg, sync))) return rc;
    }
    if (first_err != TQGPU_OK) return fail(first_err, first_msg);
    return TQGPU_OK;
}

extern "C" int tqgpu_solve_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *o, tqgpu_result *results) { return solve_batch_impl(solvers, n, o, results, nullptr); }

extern "C" int tqgpu_solve_batch_n(tqgpu_solver **solvers, int n, const tqgpu_opts *o, int steps, tqgpu_result *results, long *iter_sum, long *ls_sum, long *launch_sum) {
    if (steps < 1) return fail(TQGPU_EINVAL, "tqgpu_solve_batch_n: bad arguments");
    long it = 0, ls = 0, la = 0;
    for (int k = 0; k < steps; k++) {
        const int rc = tqgpu_solve_batch(solvers, n, o, results);
        if (rc != TQGPU_OK) return rc;
        for (int i = 0; i < n; i++) { it += results[i].iter; ls += results[i].ls_total; la += results[i].n_launches; }
    }
    if (iter_sum) *iter_sum = it;
    if (ls_sum) *ls_sum = ls;
    if (launch_sum) *launch_sum = la;
    return TQGPU_OK;
}

#include "tdunes_kkt.hpp"
#include "tdunes_mpc.hpp"
#include "tdunes_adjoint.hpp"
#include "tdunes_shard.hpp"

extern "C" int tqgpu_get_iteration_log(tqgpu_solver *s, int *ls_iters, double *iter_times, int cap) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    const int n = std::min(std::min(cap, s->last_iter), s->ls_log_cap);
    if (n > 0 && ls_iters) {
        /* fetched on request (stream-ordered behind the solve), not on every solve */
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipMemcpyAsync(s->h_ls_log, s->D.ls_log, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    for (int i = 0; i < n; i++) {
        if (ls_iters) ls_iters[i] = s->h_ls_log[i];
        if (iter_times) iter_times[i] = i < (int)s->tm.iter_times.size() ? s->tm.iter_times[i] : NAN;
    }
    return TQGPU_OK;
}

/* profile level 3: per Newton iteration the device time of the reference's phases (profiling.h:58-67) on the launch-per-level path:
 * build_dual = gradient, termination test, dual Hessian; newton_direction = backward factorisation + forward substitution;
 * line_search = direction test + first trial sweep + Armijo decision (further trials of a backtracking search are enqueued after the
 * read-back and are NOT in this figure).  stage_qps[0] = the first sweep of the solve; phase S of every later iteration IS the accepted
 * trial sweep of the line search before it, so stage_qps[i > 0] = 0.  NaN where nothing was recorded (opts.profile < 3). */
extern "C" int tqgpu_get_phase_log(tqgpu_solver *s, double *stage_qps, double *build_dual, double *newton_direction, double *line_search, int cap) {
    SETTLE(s);
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    const int n = std::min(cap, s->last_iter);
    for (int i = 0; i < n; i++) {
        const bool have = (size_t)(3 * i + 2) < s->tm.phase_times.size();
        if (stage_qps) stage_qps[i] = i == 0 ? s->tm.first_sweep_time : (std::isnan(s->tm.first_sweep_time) ? NAN : 0.0);
        if (build_dual) build_dual[i] = have ? s->tm.phase_times[(size_t)(3 * i)] : NAN;
        if (newton_direction) newton_direction[i] = have ? s->tm.phase_times[(size_t)(3 * i + 1)] : NAN;
        if (line_search) line_search[i] = have ? s->tm.phase_times[(size_t)(3 * i + 2)] : NAN;
    }
    return n;
}

/* Device times (HIP events on the solver's stream, first to last enqueued operation of a solve) of the
 * last `n` solves, oldest first; synchronises the stream.  Returns the number written. */
extern "C" int tqgpu_get_device_times(tqgpu_solver *s, double *out, int n) {
    SETTLE(s);
    if (!s || !out || n < 0) return -1;
    if (hipSetDevice(s->device) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return -1;
    const long have = std::min<long>(std::min<long>(n, s->solve_no), EV_RING);
    for (long i = 0; i < have; i++) {
        const int ring = (int)((s->solve_no - have + i) % EV_RING);
        float ms = 0.f;
        out[i] = (s->tm.ring_ok[(size_t)ring] && hipEventElapsedTime(&ms, s->tm.ring_ev0[ring], s->tm.ring_ev1[ring]) == hipSuccess) ? 1e-3 * ms : NAN;
    }
    return (int)have;
}

/* per-solve HIP event pairs on or off (default on).  Off: a single persistent launch is enqueued with nothing around it -- two
 * queue packets fewer per solve -- and tqgpu_get_device_times reports NaN for such solves; tqgpu_result.device_time is the
 * kernel's own clock (launch start to verdict) either way.  The other paths always record (their device time IS the pair). */
extern "C" int tqgpu_set_event_timing(tqgpu_solver *s, int on) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    s->tm.ev_timing = on != 0;
    return TQGPU_OK;
}

/* Algorithmic bytes / flops of one Newton iteration (every input read once, every output written
 * once per phase; SURVEY.md §8(d) generalised to per-node dimensions; n_ls line-search trials,
 * each counted as the reference does: one dual-function sweep, plus the fval0 sweep). */
extern "C" int tqgpu_iteration_cost(const tqgpu_solver *s, int n_ls, double *bytes, double *flops) {
    if (!s) return fail(TQGPU_EINVAL, "null solver");
    double Sb = 0, Gb = 0, Hb = 0, Fb = 0, Lb = 0, Sf = 0, Gf = 0, Hf = 0, Ff = 0, Lf = 0;
    const int Nn = s->Nn;
    for (int k = 0; k < Nn; k++) {
        const double nx = s->nx[k], nu = s->nu[k], d = s->bdim[k];
        Sb += 9 * nx + 9 * nu; Lb += 6 * nx + 1 + 6 * nu;
        if (k > 0) {
            const int p = s->dad[k];
            const double AB = nx * (s->nx[p] + s->nu[p]);
            Sb += AB + 2 * nx; Gb += AB + 4 * nx; Hb += AB + nx; Lb += AB + 3 * nx;
            Sf += 2 * AB; Gf += 2 * AB; Lf += 2 * AB;
            Hf += AB + nx * (nx + 1) * (s->nx[p] + s->nu[p]);
        }
        if (k < s->Np) {
            Gb += nx + nu; Hb += nx + nu + d * (d + 1) / 2; Lb += 1.5 * d;
            Fb += 3 * d * (d + 1) / 2 + 5 * d;
            Ff += d * d * d / 3 + 2 * d * d;
            /* off-diagonal sibling blocks */
            for (int a = 0; a < s->nk[k]; a++) for (int c = 0; c < a; c++) {
                const double na = s->nx[s->kid0[k] + a], nc = s->nx[s->kid0[k] + c];
                Hf += nc * (nx + nu) + 2 * na * nc * (nx + nu);
            }
            if (k > 0) {
                Hb += nx * d; Fb += 3 * nx * d + nx * (nx + 1) + 3 * nx;
                Ff += nx * d * d + nx * (nx + 1) * d + 4 * nx * d;
            }
        }
    }
    const double sweeps = 1 + n_ls;       /* fval0 + trials */
    if (bytes) *bytes = 8.0 * (Sb + Gb + Hb + Fb + sweeps * Lb);
    if (flops) *flops = Sf + Gf + Hf + Ff + sweeps * Lf;
    return TQGPU_OK;
}
#endif  /* TQ_HAS(TQP_HOST) */

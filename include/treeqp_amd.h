/*
 * treeqp_amd.h -- C-ABI of the MI355X (gfx950) device path of the tdunes hot path.
 *
 * This is the drop-in boundary: plain `extern "C"`, pointers and sizes only, no C++/torch types.
 * The reference has no FFI for this path (it is a static C library, Makefile:55-63); the entry
 * points below are what its own solver front end binds, one per reference interface:
 *
 *   tqgpu_create / tqgpu_destroy    <- treeqp_tdunes_calculate_size + treeqp_tdunes_create
 *                                      (dual_Newton_tree.c:1291-1407, 1411-1648): workspace sizing,
 *                                      setup_npar/setup_idxpos (:166-194) become device tables
 *   tqgpu_set_dynamics / _objective_diag / _bounds
 *                                   <- the QP values the solver reads from tree_qp_in every solve
 *                                      (tree_qp_common.h:85-115) + stage_qp_clipping_init
 *                                      (dual_Newton_tree_clipping.c:149-184: Qinv = 1/diag(Q))
 *   tqgpu_set_lambda                <- treeqp_tdunes_set_dual_initialization (dual_Newton_tree.c:1654-1663)
 *   tqgpu_solve                     <- the Newton loop of treeqp_tdunes_solve (dual_Newton_tree.c:1166-1228):
 *                                      solve_stage_problems, build_dual_problem, calculate_delta_lambda,
 *                                      line_search, all as HIP kernels
 *   tqgpu_get_solution              <- the export block of treeqp_tdunes_solve (:1235-1247) + export_mu
 *                                      (dual_Newton_tree_clipping.c:386-399)
 *
 * Flat data layout ("ltv" order of tree_qp_common.c:1952-2090):
 *   per node k: Qd,q,xmin,xmax (nx[k] doubles each, nodes concatenated); Rd,r,umin,umax (nu[k])
 *   per edge e=k-1: A (nx[k] x nx[dad(k)], column major), B (nx[k] x nu[dad(k)]), b (nx[k])
 *   lambda / lam / dlam: concatenation over k=1..Nn-1 of nx[k] doubles
 *
 * All functions return 0 on success, a negative TQGPU_E* code otherwise; tqgpu_last_error()
 * returns a human-readable message for the calling thread.  Nothing here falls back to the CPU.
 */
#ifndef TREEQP_AMD_H_
#define TREEQP_AMD_H_
#ifdef __cplusplus
extern "C" {
#endif

#define TQGPU_OK 0
#define TQGPU_ENODEVICE (-1)     /* no usable HIP device / HIP runtime error */
#define TQGPU_EINVAL (-2)        /* inconsistent tree / dimensions / options */
#define TQGPU_ENOMEM (-3)
#define TQGPU_EUNSUPPORTED (-4)  /* e.g. dual block too large for the LDS-resident kernels */
#define TQGPU_ECOMM (-5)         /* RCCL failure */
#define TQGPU_ETIMEOUT (-6)      /* a bounded wait inside the persistent launch gave up (its workgroups were not all resident: the device is
                                    shared); tqgpu_solve does not return this -- it redoes the solve on the launch-per-tier / per-level path */

typedef struct tqgpu_solver tqgpu_solver;

typedef struct tqgpu_opts {
    int maxIter;
    int termCondition;           /* termination_t value */
    double stationarityTolerance;
    int regType;                 /* regType_t value */
    double regTol, regValue;
    int lineSearchMaxIter;
    double lineSearchGamma, lineSearchBeta;
    int lineSearchRestartTrigger;
    int profile;                 /* 0: total device time only; 1: per-iteration event timing; 3: + per-phase event timing (launch-per-level path) */
    int checkLastActiveSet;      /* treeqp_tdunes_opts_t.checkLastActiveSet (dual_Newton_tree.c:98, default 1 there).  In the reference the option
                                    changes the work, never the result (a kept Cholesky factor is bit-identical to a rebuilt one), so 0 and 1 both
                                    run the default kernel, which rebuilds every pass.  2 selects the kernel variant that keeps the factor data of
                                    a workgroup (tier subtree) whose active set did not change and only substitutes (persistent path only); its
                                    steps agree with rebuilt ones to rounding, not bit for bit -- see DESIGN.md "checkLastActiveSet" */
} tqgpu_opts;

typedef struct tqgpu_result {
    int status;                  /* return_t value: 0 optimal, 1 max iterations, 2 not a descent direction, 4 stage QP solve failed (box nodes, nodes with general constraints) */
    int iter;                    /* Newton iterations */
    int ls_total;                /* total line-search trials */
    int ls_last;                 /* trials of the last iteration */
    int n_launches;              /* kernels launched during the solve */
    double device_time;          /* seconds between the first and last kernel (HIP events) */
    double last_error_norm;      /* termination norm (opts->termCondition: sum of squares, two-norm or largest entry of the dynamics residual), see below */
    double last_fval;            /* dual function value as the solver minimises it, see below */
} tqgpu_result;
/* Which point last_error_norm and last_fval belong to, per exit (the pairing of the reference's loop, dual_Newton_tree.c:1166-1228: the norm
 * is taken when an iteration starts, the value when its line search ends):
 *   status 0 (optimal)         last_error_norm: at the returned point -- the norm of A x_dad + B u_dad + b - x of the returned x, u; below the
 *                              tolerance.  last_fval: at the returned lam, the point the last line search accepted (iter >= 1).  With iter == 0
 *                              (the starting duals were optimal) no line search ran and last_fval belongs to no accepted point.
 *   status 1 (max iterations)  the two belong to DIFFERENT points.  last_error_norm: at the point the last iteration started from,
 *                              lam - beta^(t - 1) dlam of the returned lam and dlam, t = min(ls_last, lineSearchMaxIter) the trials made (ls_last is
 *                              lineSearchMaxIter + 1 when none was accepted); the starting duals for maxIter = 1.  last_fval:
 *                              at the returned lam, the last trial's point (accepted, or the last one tried when the line search ran out).
 *                              maxIter <= 0: nothing is iterated; status 1, iter, ls_total, ls_last, last_error_norm and last_fval are 0 on
 *                              every route, whatever an earlier solve reported (tqgpu_pshard_begin refuses maxIter <= 0).
 *   status 2 (not a descent direction)  last_error_norm: at the point the failed iteration started from, NaN if the data or the duals hold a
 *                              NaN (the largest-entry norm keeps a NaN); last_fval is not that of the returned point.
 *   status 4 (stage QP solve failed)    neither belongs to the returned point.
 * ls_last is the last entry of tqgpu_get_iteration_log and ls_total the sum of its first `iter` entries.  A member of tqgpu_solve_batch and
 * every rank of a sharded solve report their own solve's values. */

int tqgpu_device_count(void);
const char *tqgpu_last_error(void);
const char *tqgpu_version(void);

int tqgpu_create(tqgpu_solver **out, int device, int Nn, const int *nk, const int *nx, const int *nu);
void tqgpu_destroy(tqgpu_solver *s);

int tqgpu_set_dynamics(tqgpu_solver *s, const double *A, const double *B, const double *b);
int tqgpu_set_objective_diag(tqgpu_solver *s, const double *Qd, const double *Rd, const double *q, const double *r);
/* Dense objective + dense UNCONSTRAINED stage solver: replaces the reference's qpOASES stage backend
 * (dual_Newton_tree_qpoases.c:153-217 init/solve, :401-476 elimination matrices) for nodes without
 * bounds: z_k = H_k^-1 h_k, P_k = H_k^-1 with H_k = [Q S'; S R].  Flat layout as
 * tree_qp_in_set_ltv_objective_colmajor (tree_qp_common.c:2010-2050): per node Q (nx x nx), R (nu x nu),
 * S (nu x nx) column major, then q, r.  Bounds are ignored while it is selected. */
/* Routes of the dense kinds (1, 2, 3 below).  By default a tree with dense nodes runs one launch per phase and tree level.  With
 * tqgpu_set_dense_single_launch (further down; opt-in) a small tree runs its whole solve as ONE launch of one workgroup, the dense
 * stage solvers compiled in: same bodies, same results up to the order of the workgroup's sums. */
int tqgpu_set_objective_dense(tqgpu_solver *s, const double *Q, const double *R, const double *S, const double *q, const double *r);
/* the same with a per-node choice (opts->qp_solver[] of the reference, dual_Newton_tree.c:124-162): kind[k] = 0 clipping (the
 * diagonals of Q_k and R_k are the weights; off-diagonals and S_k must be zero), 1 dense unconstrained (bounds ignored),
 * 3 dense with box bounds and the general constraints of tqgpu_set_constraints (below; without rows on the node: kind 2),
 * 2 dense with box bounds: the bounds of tqgpu_set_bounds apply (qpOASES QProblemB of the reference,
 * dual_Newton_tree_qpoases.c:153-210, 312-358, 524-560: a hot-started active-set method on the bounds per node, one wave each,
 * P_k = Z (Z'H_k Z)^-1 Z' of the final working set, multipliers of the bounds in mu_x / mu_u).  NULL = all kind 1.
 * Kinds 1 and 2 need nx[k] + nu[k] <= 142 (H_k is factored in 160 KiB of LDS; TQGPU_EUNSUPPORTED otherwise).
 * Kind 2 needs nx[k] + nu[k] <= 64 (TQGPU_EUNSUPPORTED otherwise) and lb <= ub on its entries (TQGPU_EINVAL from this call or
 * from tqgpu_set_bounds, whichever makes it inconsistent).  A stage solve that does not finish ends tqgpu_solve with
 * tqgpu_result.status = 4 (TREEQP_DN_STAGE_QP_SOLVE_FAILED).  Re-uploads between solves need no reset: the working sets
 * kept for the hot start are only a starting guess. */
int tqgpu_set_objective_mixed(tqgpu_solver *s, const int *kind, const double *Q, const double *R, const double *S, const double *q, const double *r);
int tqgpu_set_bounds(tqgpu_solver *s, const double *xmin, const double *xmax, const double *umin, const double *umax);
/* General constraints dmin <= C x + D u <= dmax on the nodes of kind 3 (qpOASES QProblem of the reference,
 * dual_Newton_tree_qpoases.c:226-300, 312-358, 524-570): nc[k] rows on node k, C (nc x nx) and D (nc x nu) column major, node after
 * node; NULL = leave alone.  nc != NULL (re)defines the rows: C, D not given with it are zero, dmin, dmax unbounded.  The stage QP
 * is solved by a dual active-set method (Goldfarb and Idnani), one wave per node, on the launch-per-phase route or, on request,
 * inside the single-workgroup launch (tqgpu_set_dense_single_launch); it needs
 * nx[k] + nu[k] <= 64 (TQGPU_EUNSUPPORTED from tqgpu_set_objective_mixed) and nc[k] <= 64 (TQGPU_EUNSUPPORTED from this call);
 * dmin > dmax is TQGPU_EINVAL.  An infeasible stage QP ends tqgpu_solve with tqgpu_result.status = 4.  The multipliers of the
 * rows (sign of tree_qp_out.mu_d: + on dmax, - on dmin) come from tqgpu_get_mu_d, sum_nc doubles (tqgpu_dims2). */
int tqgpu_set_constraints(tqgpu_solver *s, const int *nc, const double *C, const double *D, const double *dmin, const double *dmax);
int tqgpu_get_mu_d(tqgpu_solver *s, double *mu_d);
int tqgpu_dims2(const tqgpu_solver *s, int *sum_nc);
/* The hot start of the kind-3 stage solver (default on, per mirror).  On: a stage solve starts from the working set (bounds, rows and
 * their sides) its node ended the last stage solve with, across sweeps and solves: the set is checked against the current data,
 * members with a multiplier of the wrong sign leave, and the dual active-set method goes on from there; a start that does not lead
 * to a solution is followed by one cold solve, so that only a cold solve's failure gives status 4.  Where the solution is strictly
 * complementary the result is that of the cold start bit for bit (it is a function of the final working set alone).  Off: every
 * stage solve starts at the minimiser over the equalities.  The call empties the stored sets of every kind-3 node; so does any
 * tqgpu_set_objective* (H, and with it q, r: there is no call for the linear terms alone) and a tqgpu_set_constraints that passes nc
 * (the rows are redefined), C or D, while bounds, dmin / dmax alone, duals and x0 keep them.  treeqp_tdunes_solve sends all of these
 * at every solve, so through the drop-in layer the hot start acts from sweep to sweep within a solve only.
 * TQGPU_EINVAL on a null solver; without kind-3 nodes the setting is kept for later and nothing else happens. */
int tqgpu_set_gen_hot_start(tqgpu_solver *s, int on);
/* Active-set steps of the kind-3 stage solver per node, last[Nn] and total[Nn] (either may be NULL): one step is one pass of its loop,
 * with one factorisation of S (the dual-feasibility rounds of a hot start and a cold redo count).  last: in the last stage sweep;
 * total: summed over the sweeps of the last tqgpu_solve (zeroed when a solve starts).  0 on nodes of other kinds. */
int tqgpu_get_stage_steps(tqgpu_solver *s, int *last, long *total);
/* Everything above in one call (NULL = leave alone) plus the starting duals: compared with a pinned host mirror of
 * what the device holds, only what changed is uploaded, without synchronisation.  This is what the drop-in
 * treeqp_tdunes_solve uses, which -- like the reference, dual_Newton_tree.c:1142-1160 -- re-reads qp_in at every solve. */
int tqgpu_set_problem(tqgpu_solver *s, const double *A, const double *B, const double *b,
                      const double *Qd, const double *Rd, const double *q, const double *r,
                      const double *xmin, const double *xmax, const double *umin, const double *umax, const double *lambda);
int tqgpu_set_lambda(tqgpu_solver *s, const double *lambda);   /* NULL = zeros */

int tqgpu_solve(tqgpu_solver *s, const tqgpu_opts *opts, tqgpu_result *res);

/* on != 0: tqgpu_solve enqueues the packing kernel and the download of the solution right behind a single persistent launch, while it
 * runs; the tqgpu_get_solution that follows only waits for the copy.  For callers that fetch the solution after every solve (the
 * drop-in front end, treeqp_tdunes_solve -> dual_Newton_tree.c:1235-1247); off by default (a caller that only wants the verdict pays
 * for nothing).  Results are the same either way. */
int tqgpu_set_export_ahead(tqgpu_solver *s, int on);

/* any output pointer may be NULL */
int tqgpu_get_solution(tqgpu_solver *s, double *x, double *u, double *lam, double *mu_x, double *mu_u, double *dlam);

/* KKT residuals of a point, evaluated on the device: what tree_qp_out_calculate_KKT_res (tree_qp_common.c:540-788) and
 * tree_qp_out_max_KKT_res compute on the host after a download, from the device copies of the data (one wave per node, then one
 * workgroup for the maxima; no atomics, so the result does not depend on scheduling).  Six classes, in the reference's order: */
#define TQGPU_KKT_STAT   0   /* Qx + q + S'u + mu_x + C'mu_d - lam_k + sum_kids A'lam_kid ; Ru + r + Sx + mu_u + D'mu_d + sum_kids B'lam_kid */
#define TQGPU_KKT_DYN    1   /* A x_dad + B u_dad + b - x_k */
#define TQGPU_KKT_BFEAS  2   /* violation of xmin/xmax, umin/umax */
#define TQGPU_KKT_BCOMPL 3   /* mu > 0 ? mu (v - max) : mu (min - v) */
#define TQGPU_KKT_GFEAS  4   /* violation of dmin <= Cx + Du <= dmax */
#define TQGPU_KKT_GCOMPL 5   /* the same product with mu_d and Cx + Du */
/* res[c]: the largest absolute entry of class c over the tree; node[c]: the lowest node that attains it, -1 (and res[c] = 0) where the
 * class has no entry (no edges, no rows); per_node (Nn x 6, node-major, or NULL): the six maxima of every node, 0 where the node has no
 * entry of the class.  The figure the reference's drivers assert on (`kkt_err < 1e-8`) is the largest of res[0..6), NaN if any is.
 *   - A multiplier that is exactly 0 contributes 0 to its complementarity entry whatever the bound (the reference computes 0 * inf = NaN);
 *     a non-zero multiplier against an infinite bound gives inf.
 *   - A NaN anywhere in a class makes res[c] NaN and node[c] the lowest such node (tree_qp_out_max_KKT_res treats NaN as worst too);
 *     a NaN value counts as violating its bounds.  Ties between nodes go to the lowest index.
 *   - Nodes of kind 1 ignore their bounds, which may never have been uploaded: they contribute 0 to BFEAS and BCOMPL, while their
 *     mu_x, mu_u enter stationarity as given.  Rows count on the nodes of kind 3, the only ones where they apply.
 *   - The phantom root states of an x0-eliminated tree on the persistent path belong to no class.
 * tqgpu_kkt_residual: the point of the last solve, whatever its route and status -- exactly what tqgpu_get_solution and tqgpu_get_mu_d
 *   return, read where it lies (the packing kernel is enqueued unless it went out ahead, tqgpu_set_export_ahead); 12 (+ Nn x 6) values
 *   come back through pinned memory, one synchronisation.  TQGPU_EINVAL on a null solver and on a mirror that has not solved yet.
 * tqgpu_kkt_residual_at: any point (a warm start, another solver's answer) in the flat layout of tqgpu_get_solution, mu_d as
 *   tqgpu_get_mu_d gives it; x, u, lam are required, a NULL multiplier array is all zeros.  Needs an uploaded problem, no solve, and
 *   changes nothing a later solve or tqgpu_get_solution reads.
 * tqgpu_kkt_residual_batch: res n x 6, node n x 6 or NULL; member i gets bit for bit what tqgpu_kkt_residual(solvers[i]) gives.  The
 *   members of one device are checked together on the stream of the first of them: one upload of a descriptor per member, at most five
 *   launches (the packing of the members that have not exported ahead -- up to three -- , one wave per (member, node), one workgroup per
 *   member for the maxima), one download of all heads and one wait, whatever n.  A member's own stream is waited for only where it may
 *   hold work that stream has not seen: uploads since its last synchronisation, an export that went out ahead, a solve of its own
 *   (tqgpu_solve) since its last check; behind a tqgpu_solve_batch whose launch the members shared nothing is.  A member alone on its
 *   device, a batch that names a mirror twice and one in which a single tree is most of the nodes go member by member: everything is
 *   enqueued on the members' own streams (3 to 5 launches and a copy each), then each is waited for once.
 *   TREEQP_AMD_KKT_BATCH=members in the environment, read at each call, forces that route (A/B runs, escape hatch).
 *   Afterwards the members' solution is packed on the device but not downloaded: tqgpu_get_solution does what it does behind
 *   tqgpu_kkt_residual.
 * tqgpu_kkt_batch_stats: what the calling thread's last tqgpu_kkt_residual_batch cost, summed over devices: kernel launches, copies (either
 *   direction), stream waits, and the members that went through the batched kernels (0 on the per-member route).  Any pointer may be
 *   NULL; reads host state only.
 * A rank of a sharded solve (tqgpu_pshard_init / tqgpu_shard_init with nranks > 1) is refused with TQGPU_EUNSUPPORTED by all three. */
int tqgpu_kkt_residual(tqgpu_solver *s, double res[6], int node[6], double *per_node);
int tqgpu_kkt_residual_at(tqgpu_solver *s, const double *x, const double *u, const double *lam,
                          const double *mu_x, const double *mu_u, const double *mu_d,
                          double res[6], int node[6], double *per_node);
int tqgpu_kkt_residual_batch(tqgpu_solver **solvers, int n, double *res, int *node);
int tqgpu_kkt_batch_stats(int *launches, int *copies, int *waits, int *batched_members);

/* 2: persistent single-launch solve (tdunes_persist.hpp); 1: tiered fused kernels (tdunes_fast.hpp);
 * 0: generic per-level kernels.  TREEQP_AMD_PATH=generic|tiered in the environment at create time
 * forces the lower paths. */
int tqgpu_uses_fused_path(const tqgpu_solver *s);
/* diagnostic: the kernel variants chosen by tqgpu_create and the last tqgpu_set_objective_mixed, and the last solve's route, one bit each (any pointer may be
 * NULL; reads the mirror, changes nothing).  *sgp_accs: children's [x | u] entries that k_sgp keeps in LDS per parent. */
#define TQGPU_PLAN_WIDE            (1u << 0)    /* workgroup-per-block kernels of the wide-block class */
#define TQGPU_PLAN_WIDE_SMALL      (1u << 1)    /* ... taken by the rule for wide trees of small blocks (d <= 16) */
#define TQGPU_PLAN_W3              (1u << 2)    /* three launches per Newton iteration */
#define TQGPU_PLAN_W3_SGP          (1u << 3)    /* ... with k_sgp, a workgroup per parent */
#define TQGPU_PLAN_W3_MERGE        (1u << 4)    /* ... forward sweep and first trial in one launch */
#define TQGPU_PLAN_FWD_CHAIN       (1u << 5)    /* ... forward sweep along each block's path to the root (k_fwd3c) */
#define TQGPU_PLAN_FUSE            (1u << 6)    /* reductions as the tails of the sweeps (<= 512 nodes) */
#define TQGPU_PLAN_PERSIST         (1u << 7)    /* persistent single launch */
#define TQGPU_PLAN_PERSIST_ONE     (1u << 8)    /* ... in the one-workgroup-per-CU build */
#define TQGPU_PLAN_GPERSIST        (1u << 9)    /* single-workgroup persistent kernel */
#define TQGPU_PLAN_GP_STATE_LDS    (1u << 10)   /* ... its mutable state in LDS */
#define TQGPU_PLAN_GP_CONST_LDS    (1u << 11)   /* ... and its constants */
#define TQGPU_PLAN_GP_TABLES_LDS   (1u << 12)   /* ... only its index tables (the state does not fit) */
#define TQGPU_PLAN_GP_SMALL16      (1u << 13)   /* ... four nodes per wave in the stage sweep */
#define TQGPU_PLAN_GP_SMALL8       (1u << 14)   /* ... eight nodes per wave in the gradient sweep */
#define TQGPU_PLAN_DENSE           (1u << 15)   /* dense stage solver selected */
#define TQGPU_PLAN_BOX             (1u << 16)   /* ... with box-constrained nodes */
#define TQGPU_PLAN_LAST_SINGLE_WG  (1u << 17)   /* the last solve begun (alone or in a batch) ran the single-workgroup kernel */
#define TQGPU_PLAN_GEN             (1u << 18)   /* dense stage solver with nodes that have general constraints (kind 3) */
#define TQGPU_PLAN_DENSE_SINGLE_WG (1u << 19)   /* dense tree opted in to the single-workgroup launch AND eligible for it (tqgpu_set_dense_single_launch) */
int tqgpu_debug_plan(const tqgpu_solver *s, unsigned *flags, int *sgp_accs);
/* Single-launch solves of dense trees (kinds 1 / 2 / 3), per mirror, default off; TREEQP_AMD_DENSE_SINGLE_LAUNCH=1 in the environment
 * at create time is the same as calling the setter with 1.  On: a dense tree that fits runs its whole solve as one launch of one
 * workgroup (tqgpu_uses_fused_path gives 3) instead of one launch per phase and level.  It fits when no tree level has more than 96
 * nodes and the stage windows find room: a node's stage solve needs head + 2 nz^2 doubles of LDS (kind 2) or
 * head + nc + 2 nz^2 + nz nc + nc^2 (kind 3), nz = nx + nu, head = children's nx + nx + 2 nz + 2; the stage sweep runs on
 * stage_waves <= 16 waves, each with a window of the tree's largest need, stage_waves being the largest count whose windows, with the
 * index tables, stay within 150 KiB.  Eligibility follows the kinds and rows last set (tqgpu_set_objective_mixed / _dense,
 * tqgpu_set_constraints with nc).  A tree that does not fit, a profiled solve (opts->profile != 0), maxIter <= 0 and the members of a
 * tqgpu_solve_batch keep the launch-per-phase route, unless tqgpu_set_dense_batch_launch.  The stored working sets (the hot start of kinds 2 and 3) are shared by both
 * routes: switching between two solves needs no reset.  Results agree with the default route's up to the order of the sums (1e-10
 * on well-conditioned problems); status 4 (a stage QP without solution) ends the solve inside the launch with the same verdict. */
int tqgpu_set_dense_single_launch(tqgpu_solver *s, int on);
/* any pointer may be NULL: the setting, whether the current kinds / rows fit, waves of the stage sweep (0 if not eligible) */
int tqgpu_get_dense_single_launch(const tqgpu_solver *s, int *on, int *eligible, int *stage_waves);
/* Batches of dense trees in one launch, per mirror, default off; TREEQP_AMD_DENSE_BATCH_LAUNCH=1 in the environment at create time is
 * the same as calling the setter with 1.  On: where tqgpu_solve_batch finds at least two such members that fit (the rule above, the same
 * `eligible`) next to each other on one device, they go out as ONE launch with one workgroup per tree, each workgroup computing exactly what the
 * member's tqgpu_set_dense_single_launch solve computes (bit for bit) -- instead of one member after the other on the launch-per-phase
 * route.  A member alone in its batch, a profiled solve and maxIter <= 0 run what the mirror runs on its own.  Independent of
 * tqgpu_set_dense_single_launch: this option says nothing about tqgpu_solve, that one nothing about batches.  Status 4 in one member ends
 * that member's workgroup only; working sets and step counters are shared with the other routes, switching needs no reset.  After the
 * batch, TQGPU_PLAN_LAST_SINGLE_WG is set on the members that went out in the launch. */
int tqgpu_set_dense_batch_launch(tqgpu_solver *s, int on);
/* any pointer may be NULL: the setting, whether the current kinds / rows fit (as tqgpu_get_dense_single_launch reports it) */
int tqgpu_get_dense_batch_launch(const tqgpu_solver *s, int *on, int *eligible);
/* geometry of the persistent launch: block levels, tiers, workgroups per launch, co-resident workgroup capacity of the device, CUs */
int tqgpu_geometry(const tqgpu_solver *s, int *levels, int *tiers, int *workgroups, int *capacity, int *compute_units);
/* diagnostic: persistent launches of this mirror that timed out (device shared with other work) and were redone on another path */
int tqgpu_timeouts(const tqgpu_solver *s);

/* sizes of the flat arrays, for callers that did not keep them */
int tqgpu_dims(const tqgpu_solver *s, int *sum_nx, int *sum_nu, int *sum_lam, int *sum_A, int *sum_B);

/* per-iteration line-search counts and event times (seconds) of the last solve; arrays of
 * length >= iter; times are NaN unless opts.profile != 0 */
int tqgpu_get_iteration_log(tqgpu_solver *s, int *ls_iters, double *iter_times, int cap);

/* opts.profile >= 3: device time per Newton iteration of the reference's phases (treeqp/utils/profiling.h:58-67): build_dual,
 * newton_direction, line_search; stage_qps[0] = first sweep of the solve, 0 afterwards (phase S of a later iteration IS the accepted
 * trial sweep of the line search before it).  Arrays of length >= cap (any may be NULL); returns the number of iterations written. */
int tqgpu_get_phase_log(tqgpu_solver *s, double *stage_qps, double *build_dual, double *newton_direction, double *line_search, int cap);
/* roofline support: algorithmic bytes and flops of ONE Newton iteration with n_ls line-search
 * trials (closed form of SURVEY.md §8(d) generalised to per-node dimensions) */
int tqgpu_iteration_cost(const tqgpu_solver *s, int n_ls, double *bytes, double *flops);

/* The partition plan of the sharded mode without a device: which tier is the highest partitioned one, the boundary level, the
 * blocks above the bottom tier whose gradient / Hessian this rank computes (the first gh_counted of them enter its termination
 * partial) and the nodes it owns.  Host arithmetic only (the CPU tests compare it with treeqp_amd/sharding.py). */
int tqgpu_shard_plan(int md, int nx, int Nh, int nranks, int rank, int *part_top, int *boundary_level, int *gh_counted,
                     int *gh_list, int gh_cap, int *gh_n, int *owned_nodes, int owned_cap, int *owned_n);
/* ---- one tree sharded over several devices --------------------------------------
 * Every rank creates a mirror of the WHOLE tree and uploads the whole problem; tqgpu_shard_init then
 * restricts the rank's work to a contiguous range of subtrees (tiers above the partition boundary
 * are replicated).  Per Newton iteration two small in-place all-gathers over RCCL exchange the
 * boundary Schur records + termination partials and the {fval, dot} partials + boundary x/QinvCal.
 * id128: 128-byte RCCL unique id created by rank 0 (tqgpu_shard_unique_id) and broadcast by the
 * caller (e.g. through torch.distributed); NULL creates a "virtual rank" without a communicator. */
int tqgpu_shard_unique_id(void *id128);
int tqgpu_shard_init(tqgpu_solver *s, int rank, int nranks, const void *id128);
int tqgpu_shard_gather_solution(tqgpu_solver *s);
/* test / diagnostic: n virtual ranks of one tree in one process on one device, lock-step */
int tqgpu_solve_virtual_ranks(tqgpu_solver **ranks, int n, const tqgpu_opts *opts, tqgpu_result *res);

/* ---- one tree sharded over several devices INSIDE the persistent launch ----------
 * The workgroups of the single persistent launch (one per tier subtree, tdunes_persist.hpp) are dealt over one launch per
 * rank: tiers whose subtree count is a multiple of the number of ranks by contiguous subtree ranges (the independent subtrees
 * of dual_Newton_tree.c:668-775), the tiers above them to rank 0.  What crosses ranks -- the Schur push of
 * dual_Newton_tree.c:726-732, the forward pull of :768-769, the global scalars of :542, :944-945, :970 -- travels as the
 * same tagged words as on one device: every rank has a hand-over slab, a producer writes each word into every rank's slab
 * (system-scope stores into peer-mapped memory), a consumer polls its own.  No collective and no host in the loop; the
 * solution is collected afterwards by any transport (tqgpu_pshard_pack / _unpack: equal-sized buffers for an all-gather).
 *   tqgpu_pshard_init          this mirror (whole tree created, whole problem uploaded) becomes rank `rank` of `nranks` (<= 8)
 *   tqgpu_pshard_connect_local peer r is another mirror of this process (same device: rehearsal; other device: peer access)
 *   tqgpu_pshard_ipc_export / _ipc_connect   peers in other processes: 64-byte IPC handle of the slab out / of peer r in
 *   tqgpu_pshard_begin / _end  one solve: enqueue this rank's launch / wait for the verdict.  All ranks' launches must be in
 *                              flight together (they wait for each other: bounded, TQGPU_ETIMEOUT after 0.5 s) and every rank
 *                              must solve the same number of times (the launch number tags the words)
 *   tqgpu_pshard_solve_local   n mirrors of one process: connect, solve, collect the solution into every mirror */
/* the partition without a device (host arithmetic; tqgpu_pshard_init uses it): this rank's workgroups of the persistent launch */
int tqgpu_pshard_plan(int md, int Nh, int nranks, int rank, int *wgs, int cap, int *n, int *part_top, int *boundary_level);
int tqgpu_pshard_init(tqgpu_solver *s, int rank, int nranks);
int tqgpu_pshard_connect_local(tqgpu_solver *s, int r, tqgpu_solver *peer);
int tqgpu_pshard_ipc_export(tqgpu_solver *s, void *handle64);
int tqgpu_pshard_ipc_connect(tqgpu_solver *s, int r, const void *handle64);
int tqgpu_pshard_begin(tqgpu_solver *s, const tqgpu_opts *opts);
/* after 65535 sharded solves tqgpu_pshard_begin refuses (the 16-bit launch number tags the hand-over words): every rank then calls
 * tqgpu_pshard_rewind -- launch numbers back to zero, slab wiped, peers stay connected -- with no sharded solve in flight anywhere, i.e.
 * between two barriers of the caller's.  tqgpu_pshard_solve_local does it by itself. */
int tqgpu_pshard_rewind(tqgpu_solver *s);
int tqgpu_pshard_end(tqgpu_solver *s, tqgpu_result *res);
long tqgpu_pshard_pack_size(tqgpu_solver *s);
int tqgpu_pshard_pack(tqgpu_solver *s, double *out, long cap);
int tqgpu_pshard_unpack(tqgpu_solver *s, int src_rank, const double *in, long n_in);
int tqgpu_pshard_solve_local(tqgpu_solver **ranks, int n, const tqgpu_opts *opts, tqgpu_result *res);

/* n solves of the same problem from the same starting duals, one after the other, each waiting for its verdict: the timing loop
 * of the reference's drivers (examples/spring_mass_dual_newton_tree.c:135-140, `for (jj = 0; jj < NREP; jj++)
 * treeqp_tdunes_solve(...)`) in C.  res: the last solve; sums over the solves in *iter_sum, *ls_sum, *launch_sum (each may be NULL). */
int tqgpu_solve_n(tqgpu_solver *s, const tqgpu_opts *opts, int n, tqgpu_result *res, long *iter_sum, long *ls_sum, long *launch_sum);
/* the same loop for a batch: `steps` calls of tqgpu_solve_batch(solvers, n, ...) one after the other (the scenario sweep of
 * examples/fault_tolerance.c:486-530 repeated, e.g. once per MPC step); results: the n results of the last call; sums over all
 * calls and members in *iter_sum, *ls_sum, *launch_sum (each may be NULL) */
int tqgpu_solve_batch_n(tqgpu_solver **solvers, int n, const tqgpu_opts *opts, int steps, tqgpu_result *results, long *iter_sum, long *ls_sum, long *launch_sum);

/* Batched multi-tree solve: n independent mirrors with the same options (examples/fault_tolerance.c:486-530
 * holds one tree_qp_in / workspace pair per configuration and solves them one after the other).  Mirrors whose
 * solve is a single persistent launch run concurrently, as many as fit on the device at once. */
int tqgpu_solve_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *opts, tqgpu_result *results);

/* ---- MPC steps without the host in the data path: the x0 fold, the warm start and u[0] on the device ----------------------------
 * An MPC loop on an x0-eliminated tree (nx[0] == 0, tree_qp_in_eliminate_x0 / tree_qp_in_set_x0_*: qp_container.c), or on a tree whose
 * root keeps its states (tqgpu_mpc_set_root_states), moves x0, starts from the last duals, solves and applies u[0].  These calls
 * keep all of it on the device: the originals of what multiplies x0 stay there, a kernel folds a new x0 into b, r[0], dmin[0],
 * dmax[0] in place, another copies the last duals into the start buffer, and a small kernel behind the solve posts u[0] into
 * pinned memory.  Every call below, the getters included, refuses a rank of a sharded solve (tqgpu_shard_init / tqgpu_pshard_init
 * with nranks > 1) with TQGPU_EUNSUPPORTED, before it touches the device.
 *   tqgpu_mpc_set_root   the originals, copied into device memory (the caller's arrays are free afterwards).  nk0 = nk[0] children:
 *                        A0: for each child of the root in order nx[kid] x nx0, column major, concatenated; b0: nx[kid] each;
 *                        S0 (nu[0] x nx0, column major) with r0 (nu[0]); C0 (nc[0] x nx0, column major) with dmin0, dmax0 (nc[0] each).
 *                        S0 == NULL and C0 == NULL mean zero: r[0] resp. dmin[0], dmax[0] are then left alone by the fold.
 *                        TQGPU_EINVAL: the root still has states (eliminate x0 first), nx0 <= 0, A0 or b0 missing, S0 without r0 or C0
 *                        without dmin0 and dmax0, a non-zero S0 on a root of kind 0 (clipping: S must be zero), C0 without rows on the
 *                        root (tqgpu_set_constraints; a root that is not of kind 3 has none).  A call replaces an earlier one.
 *   tqgpu_mpc_set_x0     one kernel on the mirror's stream, no synchronisation (the next solve is ordered behind it):
 *                          b_kid   = b0_kid + A0_kid x0   for the children of the root, one wave per child, rows over lanes;
 *                          r[0]    = r0 + S0 x0           where S0 was given;
 *                          dmin[0] = dmin0 - C0 x0, dmax[0] = dmax0 - C0 x0   where C0 was given.
 *                        Summation order: every entry starts from the original (b0, r0, dmin0, dmax0) and takes one fused
 *                        multiply-add per column j = 0, 1, .., nx0 - 1, ascending: v = fma(A0[i, j], x0[j], v), for the rows
 *                        v = fma(-C0[i, j], x0[j], v).  x0 is copied into a pinned buffer of the mirror, which the kernel reads.
 *                        The stored working sets of kinds 2 and 3 are kept; the pinned host mirror of tqgpu_set_problem is
 *                        invalidated (the next tqgpu_set_problem uploads everything it is given).  No route packs b; the persistent
 *                        route packs r and the bounds (they are repacked when r[0] moved), the rows of kind 3 are read in place.
 *                        A tqgpu_set_constraints that changes nc[0] after tqgpu_mpc_set_root leaves C0 without its rows: TQGPU_EINVAL
 *                        here until tqgpu_mpc_set_root is called again.
 *                        TQGPU_EINVAL before tqgpu_mpc_set_root (or tqgpu_mpc_set_root_states).
 *   tqgpu_mpc_set_root_states   the other form of root: a tree whose root keeps its nx[0] states takes x0 as xmin[0] = xmax[0] = x0 (the
 *                        nx0 > 0 branch of tree_qp_in_set_x0_strvec).  The call declares that, keeps nothing on the device but a pinned
 *                        buffer for x0 and u[0], and afterwards tqgpu_mpc_set_x0, tqgpu_mpc_step, tqgpu_mpc_step_batch,
 *                        tqgpu_set_warm_start and tqgpu_mpc_stats work on the mirror as on an eliminated one, with nx0 = nx[0].
 *                        The fold is one more role of the same kernel and launch: lanes copy x0[i] bit for bit into xmin[0][i] and
 *                        xmax[0][i]; no arithmetic.  The persistent route keeps a copy of the bounds in its packed constants: where
 *                        those are current the fold writes the root's lower and upper entries there as well, so that no re-pack is
 *                        asked for and a steady-state step stays at 3 launches, 0 copies, 1 wait; where a re-pack is pending for
 *                        another reason, it reads the folded bounds.  Every other route (single-workgroup, three-launch, wide,
 *                        tiered, generic, the stage solvers of kinds 2 and 3, the batched launches) reads the bounds in place at
 *                        every launch.  The stored working sets of kinds 2 and 3 are kept; the pinned host mirror of
 *                        tqgpu_set_problem is invalidated.
 *                        TQGPU_EINVAL: the root has no states (tqgpu_mpc_set_root is the call for an eliminated root), or it is of
 *                        kind 1, whose bounds are ignored -- checked here and again at every fold, in case the kinds changed.
 *   tqgpu_get_root_bounds       what the device holds now for the root: xmin[0], xmax[0], nx[0] doubles each (either may be NULL).
 *                        Waits for the mirror's stream.  TQGPU_EUNSUPPORTED on a rank of a sharded solve, as every call here.
 *   tqgpu_set_warm_start mode 0 (default): every solve starts from the buffer of tqgpu_set_lambda.  Mode 1: every solve starts from
 *                        the duals tqgpu_get_solution would return at that moment, whatever the last route and status: a kernel
 *                        ahead of the solve copies them (sum_nx doubles, node-indexed, phantom root states included) into the start
 *                        buffer, and reads on the device which of the two dual buffers is current.  Before the mirror's first solve,
 *                        and after a tqgpu_set_lambda (or a tqgpu_set_problem that passes lambda), the start is what that call filled,
 *                        for one solve.  The mode applies to tqgpu_solve, tqgpu_solve_n, the members of tqgpu_solve_batch(_n) and the
 *                        step calls.  The redo after a timed-out persistent launch starts where the timed-out attempt started.
 *                        Mode 2: as mode 1, through the shift map of the realised child (tqgpu_mpc_set_shift, below).
 *   tqgpu_get_root_terms what the device holds now (any pointer may be NULL): b of the root's children (sum of their nx), r[0] (nu[0]),
 *                        dmin[0], dmax[0] (nc[0] each; untouched where the root has no rows).  Waits for the mirror's stream.
 *   tqgpu_mpc_step       tqgpu_mpc_set_x0 (x0 == NULL: keep the current one), the warm start of the current mode and tqgpu_solve, then
 *                        u[0] (nu[0] doubles) into u0: a one-workgroup kernel behind the solve writes the values into pinned memory,
 *                        then a tag the host polls.  On the single-launch routes (persistent, single-workgroup) that kernel is
 *                        enqueued behind the launch at once and the host waits for its tag only: the verdict is in by then.  If
 *                        the launch was not the whole solve (further line-search trials, a relaunch, a timeout) u[0] is posted again
 *                        behind the rest.  tqgpu_get_solution, tqgpu_get_mu_d, tqgpu_kkt_residual work afterwards as behind tqgpu_solve.
 *   tqgpu_mpc_set_certify       per mirror, default off.  On: tqgpu_mpc_step also evaluates the KKT residuals of the point it returns, in
 *                        the same wait: behind the solve and ahead of the post of u[0] it enqueues the packing of the solution (one
 *                        kernel, one more each where the tree has nodes of kind 2 and of kind 3; the device says which dual buffer
 *                        is current), the two kernels of tqgpu_kkt_residual and the download of their 12-value head, so the tag the
 *                        host waits for covers the certificate.  On the single-launch routes all of it goes out behind the launch
 *                        at once; if the launch was not the whole solve it is enqueued again behind the rest, and the certificate
 *                        belongs to the returned point.  A certified step on a single-launch route that ends inside its launch:
 *                        1 (fold + warm start) + 1 (the solve) + 1 + [kind 2] + [kind 3] (packing) + 2 (KKT) + 1 (post) launches,
 *                        1 copy, 1 wait.  Afterwards the packed point is valid on the device: tqgpu_kkt_residual does not pack
 *                        again, tqgpu_get_solution only downloads.  tqgpu_mpc_step_batch ignores the setting (a batch has
 *                        tqgpu_kkt_residual_batch).
 *   tqgpu_mpc_get_certificate   res[6], node[6] of the last tqgpu_mpc_step of this mirror (either may be NULL; host state only): bit for
 *                        bit what tqgpu_kkt_residual(s, res, node, NULL) returns right after that step.  TQGPU_EINVAL if that step
 *                        was not certified, or none has run.
 *   tqgpu_mpc_step_batch the same for n mirrors, x0s member after member (NULL: all keep theirs), u0s member after member, nu[0] of
 *                        each (x0s: nx0 doubles per member, whichever form its root has; both forms may be mixed).  Per device the
 *                        folds and warm-start copies of all members are ONE launch on the stream of the device's first member (a
 *                        descriptor per member, one upload per device and call), ahead of what tqgpu_solve_batch launches, and their
 *                        u[0] are collected by ONE launch behind it.  A member gets bit for bit what tqgpu_mpc_step gives it alone
 *                        wherever tqgpu_solve_batch gives what tqgpu_solve gives.  A member of a shared persistent launch whose
 *                        constants have to be packed again (its first solve, changed data) packs them on its own stream: that
 *                        stream's work is ordered behind the folds by one wait for the first member's stream in such a step.
 *   tqgpu_mpc_stats      what the calling thread's last tqgpu_mpc_step / _step_batch cost (any pointer may be NULL; host state only):
 *                        launches: kernels enqueued (fold + warm start, the solves' own -- a launch shared by a group of a batch counts
 *                          once --, u0 posts);
 *                        copies: hipMemcpy calls in either direction (descriptor uploads, read-backs of the control block on the
 *                          launch-per-phase routes);
 *                        waits: times the host had to wait for the device: a stream synchronisation, or a poll of a pinned block
 *                          that was not complete at the first look.
 *                        A step on the persistent route that ends inside its launch: 3 launches, 0 copies, 1 wait.  A batch step of
 *                        persistent members that share one launch: 3 launches, 1 copy, 1 wait, whatever n. */
int tqgpu_mpc_set_root(tqgpu_solver *s, int nx0, const double *A0, const double *b0, const double *S0, const double *r0,
                       const double *C0, const double *dmin0, const double *dmax0);
int tqgpu_mpc_set_root_states(tqgpu_solver *s);
int tqgpu_get_root_bounds(tqgpu_solver *s, double *xmin0, double *xmax0);
int tqgpu_mpc_set_x0(tqgpu_solver *s, const double *x0);
int tqgpu_set_warm_start(tqgpu_solver *s, int mode);
int tqgpu_get_warm_start(const tqgpu_solver *s, int *mode);
int tqgpu_get_root_terms(tqgpu_solver *s, double *b_kids, double *r0, double *dmin0, double *dmax0);
int tqgpu_mpc_step(tqgpu_solver *s, const double *x0, const tqgpu_opts *opts, tqgpu_result *res, double *u0);
int tqgpu_mpc_step_batch(tqgpu_solver **solvers, int n, const double *x0s, const tqgpu_opts *opts, tqgpu_result *results, double *u0s);
int tqgpu_mpc_set_certify(tqgpu_solver *s, int on);
int tqgpu_mpc_get_certificate(tqgpu_solver *s, double res[6], int node[6]);
int tqgpu_mpc_stats(int *launches, int *copies, int *waits);

/* ---- Tracking MPC: the linear terms alone, and a reference window folded into q, r on the device ----------------------------------
 * A tracking MPC penalises (x - xref)' Q (x - xref) + (u - uref)' R (u - uref) (+ the S terms) along a setpoint or a trajectory that
 * shifts by one stage per step: only the linear terms q_k = q0_k - Q_k xref - S_k' uref, r_k = r0_k - S_k xref - R_k uref change, on
 * every node.  In a scenario tree all nodes of a stage share the reference, so the whole trajectory lives on the device once and a step
 * moves a window index.
 *   tqgpu_set_linear_terms      q, r in the layout of tqgpu_set_objective_diag; either may be NULL (left alone).  Uploads q and r only, asks
 *                        the persistent route to pack its constants again and invalidates the pinned host mirror of tqgpu_set_problem.
 *                        The kinds, H, the factors (k_init / k_dense_init are not run again) and the stored working sets of kinds 2 and
 *                        3 (the hot start) stay -- tqgpu_set_objective_mixed, the only other way to move r on a dense tree, empties them.
 *                        Works on every mirror (a rank of a sharded solve included).
 *   tqgpu_get_linear_terms      what the device holds now, same layout (phantom root states excluded; either may be NULL).  Waits for the
 *                        mirror's stream.
 *   tqgpu_mpc_set_tracking      xtraj (T x NXT) and utraj (T x NUT), stage-major (row t, then the entries), T >= 1 (T == 1: a setpoint);
 *                        q0, r0: the base linear terms in the flat layout (NULL: zeros).  All of it is copied into one device block with
 *                        the nodes' stages (the caller's arrays are free afterwards); a call replaces an earlier one and forgets the
 *                        window.  The device's q, r are not touched until a window is set.
 *                        TQGPU_EINVAL: a node with nx[k] not in {0, NXT} or nu[k] not in {0, NUT}, T < 1, xtraj / utraj NULL while the
 *                        matching width is positive.
 *   tqgpu_mpc_set_window        one kernel on the mirror's stream, no synchronisation (as tqgpu_mpc_set_x0): node k reads trajectory row
 *                        rho = min(t0 + stage[k], T - 1) and every entry of its q, r becomes one chain of fused multiply-adds from its
 *                        base, columns ascending, one wave per node, rows over lanes:
 *                          kind 0:          q[i] = fma(-Qd[i], xref[i], q0[i]),  r[i] = fma(-Rd[i], uref[i], r0[i]);
 *                          kinds 1 / 2 / 3: row i of H_k = [Q S'; S R]: v = base[i]; v = fma(-H[i, j], xref[j], v), j = 0 .. nx - 1;
 *                                           v = fma(-H[i, nx + j], uref[j], v), j = 0 .. nu - 1.
 *                        Phantom root states keep their q; a leaf has no u part; the root of an x0-eliminated tree has no x part.
 *                        An x0-eliminated root with S0 (tqgpu_mpc_set_root; nx0 must equal NXT): r[0] is one chain, base (r0 of
 *                        tqgpu_mpc_set_tracking; the r0 of tqgpu_mpc_set_root is not read), - R_0 uref, - S0 xref_rho, + S0 x0 with the
 *                        x0 last given (zeros before the first), computed whenever the window or x0 moves once a window is set: the
 *                        x0 fold of such a mirror never starts from a stale original.  A tqgpu_mpc_set_root with another nx0 while a
 *                        window is in force makes every x0 fold and step TQGPU_EINVAL until nx0 and NXT agree again.
 *                        The persistent route keeps q, r in its packed constants: where those are current the fold writes entry 0 of
 *                        every node's slots as well and asks for no re-pack; where a re-pack is pending it reads the folded Data.  Every
 *                        other route (single-workgroup, three-launch, wide, tiered, generic, the stage solvers of kinds 1 / 2 / 3, the
 *                        batched launches) reads q, r in place at every launch.  Kept: the stored working sets, H, the factor of
 *                        k_dense_init.  The pinned host mirror of tqgpu_set_problem is invalidated.  tqgpu_set_linear_terms or an
 *                        upload of the objective afterwards overwrites q, r until the next window fold, which starts from the bases.
 *                        TQGPU_EINVAL: t0 < 0, or before tqgpu_mpc_set_tracking.
 *   tqgpu_mpc_get_window        the window in force, -1 before the first fold (host state only).
 *   tqgpu_mpc_step_at / tqgpu_mpc_step_batch_at   tqgpu_mpc_step / tqgpu_mpc_step_batch with the window fold inside their ONE launch ahead
 *                        of the solve (further blocks of the same kernel): t0 (t0s[i] per member; t0s == NULL: all -1) >= 0 moves the
 *                        window, < 0 keeps it -- then the call is the plain step, on mirrors without tracking too, which a batch may
 *                        mix with tracking ones.  t0 >= 0 before tqgpu_mpc_set_tracking: TQGPU_EINVAL.  Counts are those of the plain
 *                        steps (persistent route, ending inside its launch: 3 launches, 0 copies, 1 wait; a batch of persistent members
 *                        3, 1, 1); certification (tqgpu_mpc_set_certify) works unchanged.
 * The tqgpu_mpc_* calls above refuse a rank of a sharded solve with TQGPU_EUNSUPPORTED, as every tqgpu_mpc_* call. */
int tqgpu_set_linear_terms(tqgpu_solver *s, const double *q, const double *r);
int tqgpu_get_linear_terms(tqgpu_solver *s, double *q, double *r);
int tqgpu_mpc_set_tracking(tqgpu_solver *s, int NXT, int NUT, int T, const double *xtraj, const double *utraj, const double *q0, const double *r0);
int tqgpu_mpc_set_window(tqgpu_solver *s, int t0);
int tqgpu_mpc_get_window(const tqgpu_solver *s, int *t0);
int tqgpu_mpc_step_at(tqgpu_solver *s, const double *x0, int t0, const tqgpu_opts *opts, tqgpu_result *res, double *u0);
int tqgpu_mpc_step_batch_at(tqgpu_solver **solvers, int n, const double *x0s, const int *t0s, const tqgpu_opts *opts, tqgpu_result *results, double *u0s);

/* ---- The shifted warm start: duals and working sets move a stage with the horizon ------------------------------------------------
 * After an MPC step one child j of the root has been realised and becomes the new root: what was stage t + 1 is stage t now (with
 * tracking, tqgpu_mpc_step_at(.., t + 1, ..) moves every node's reference one row).  Warm start mode 1 copies lam_k into lam_k and so
 * starts every node one stage late; mode 2 starts node k from the duals of its image img(k) in the old problem, on the device.
 * Nodes are numbered level by level: the children of k are kid0[k] .. kid0[k] + nk[k] - 1.
 *   the map              img(0) = kid0[0] + j.  For k >= 1 with parent p and sibling index c = k - kid0[p]:
 *                          img(p) has children:  img(k) = kid0[img(p)] + min(c, nk[img(p)] - 1)   (the clamp: a multistage tree, whose
 *                                                image has stopped branching);
 *                          img(p) is a leaf:     img(k) = img(p) under TQGPU_SHIFT_LEAF_REPEAT (a repeated leaf), -1 under TQGPU_SHIFT_LEAF_ZERO;
 *                          img(p) == -1 by the leaf policy:  img(k) = -1.
 *                        Last, where nx[img(k)] != nx[k] the image does not fit and img(k) = -1; this does not propagate: the nodes
 *                        below keep the image their path gives them.  Off the repeated leaves img(k) is one level deeper than k, so
 *                        img(k) > k, and dad(img(k)) == img(dad(k)): the copied dual belongs to an edge between corresponding nodes.
 *                        The start dual of node k >= 1 is the last dual of img(k), copied bit for bit, or 0.0 where img(k) = -1.  The
 *                        entries of node 0 (phantom root states, or the root's own) are copied unshifted, as mode 1 does.
 *   tqgpu_shift_map      the map, img[Nn], for nk, nx as tqgpu_create takes them: host arithmetic only, no device (as tqgpu_shard_plan).
 *                        TQGPU_EINVAL: realised outside [0, nk[0]), Nn < 1, an nk that is negative somewhere or does not name Nn nodes
 *                        level by level, an unknown leaf policy, img == NULL.  A tree of one node gives an empty map (img is not written).
 *   tqgpu_mpc_set_shift  what = TQGPU_SHIFT_DUALS, optionally | TQGPU_SHIFT_WORKING_SETS: builds the maps of all nk[0] realisations once
 *                        and keeps them in device memory: per realisation an entry-level source table (for every entry of the start
 *                        buffer the entry of the last duals it is copied from, -1: 0.0; sum_nx ints), which fits the span-per-block copy
 *                        of the warm start, and a node table (Nn ints).  Waits for the mirror's stream.  what == 0 forgets the maps and
 *                        returns mode 2 to mode 1.  A call replaces an earlier one and resets the realisation to 0.
 *                        TQGPU_EINVAL: an unknown leaf policy, unknown bits, TQGPU_SHIFT_WORKING_SETS without TQGPU_SHIFT_DUALS.
 *   tqgpu_mpc_set_realised   the child of the root that the last step realised: host state only, default 0, TQGPU_EINVAL outside [0, nk[0]).
 *   tqgpu_mpc_get_shift  leaf policy, what and the realisation in force (any pointer may be NULL; host state only).
 *   tqgpu_set_warm_start(s, 2)   every warm start goes through the map of the realisation in force, wherever mode 1 would copy: tqgpu_solve,
 *                        tqgpu_solve_n, the members of tqgpu_solve_batch(_n) and every tqgpu_mpc_step*; the warm blocks of the step's ONE
 *                        launch gather instead of copying (an index load per entry), so the counts of tqgpu_mpc_stats stay (3, 0, 1 on
 *                        a single-launch route, 3, 1, 1 for a batch of persistent members).  TQGPU_EINVAL before tqgpu_mpc_set_shift.
 *                        The rules of mode 1 stay: the mirror's first solve and the solve after a tqgpu_set_lambda start from what
 *                        that call filled; the redo of a timed-out launch starts where the attempt started.  A member of a batch gets
 *                        bit for bit what it gets alone; members in modes 0, 1 and 2 and with different realisations may be mixed.
 *   tqgpu_mpc_shift      the shift alone, as tqgpu_mpc_set_x0 is the fold alone: one kernel on the mirror's stream, no synchronisation.
 *                        The next solve starts from the shifted duals, for one solve, in any mode; a mirror in mode 0 starts from the
 *                        buffer of tqgpu_set_lambda again afterwards (the kernel saves it, the solve after the next puts it back with
 *                        one device-to-device copy).  It also moves the working sets if they were asked for.  TQGPU_EINVAL before
 *                        tqgpu_mpc_set_shift and before the mirror's first solve.  Two calls ahead of one solve: the working sets move
 *                        twice (the second call gathers what the first stored), the duals once -- every call gathers from the duals
 *                        of the last solve, which a shift does not touch, so the second call fills the start buffer as the first did.
 *   the working sets     (TQGPU_SHIFT_WORKING_SETS, trees with nodes of kind 2 or 3) in the same launch as the duals, wherever those
 *                        are gathered: node k takes the bound set and its sides from img(k) where both nodes are of kind 2 or 3, nx
 *                        and nu agree, img(k) != -1 and img(k) is not a repeated leaf; under the same conditions it takes the row set
 *                        and its sides where both are of kind 3 and nc agrees.  Every other node keeps its own sets.  The kinds, nu and
 *                        nc are read on the device at every launch: after tqgpu_set_objective_mixed or a tqgpu_set_constraints that
 *                        changes nc the maps need no rebuild, the rule is applied to what the device holds then.  The stage solvers
 *                        re-validate a set they are given, so a shifted set needs no reset after tqgpu_set_constraints.  The gather is
 *                        in place: img(k) > k for every node that takes a set, and one wave walks the nodes in ascending chunks of 64
 *                        with all loads of a chunk ahead of its stores.  The halves that say what P_k was last built for are not touched.
 *   tqgpu_get_working_sets / tqgpu_set_working_sets   Nn words each, any pointer may be NULL: the hot-start halves of the stored sets,
 *                        bounds (bit i: entry i of [x | u] of node k sits on a bound), rows, and their sides (bit set: upper side).
 *                        Nodes of kinds 0 and 1 read as 0 and ignore what is set; rows and row_sides are those of the kind-3 nodes.
 *                        The getter waits for the stream; the setter uploads and keeps everything else.
 * All of the calls above that take a solver refuse a rank of a sharded solve with TQGPU_EUNSUPPORTED, and a null solver with TQGPU_EINVAL. */
#define TQGPU_SHIFT_LEAF_REPEAT 0
#define TQGPU_SHIFT_LEAF_ZERO   1
#define TQGPU_SHIFT_DUALS        1u
#define TQGPU_SHIFT_WORKING_SETS 2u
int tqgpu_shift_map(int Nn, const int *nk, const int *nx, int realised, int leaf, int *img);
int tqgpu_mpc_set_shift(tqgpu_solver *s, int leaf, unsigned what);
int tqgpu_mpc_set_realised(tqgpu_solver *s, int child);
int tqgpu_mpc_get_shift(const tqgpu_solver *s, int *leaf, unsigned *what, int *realised);
int tqgpu_mpc_shift(tqgpu_solver *s);
int tqgpu_get_working_sets(tqgpu_solver *s, unsigned long long *bounds, unsigned long long *rows, unsigned long long *bound_sides, unsigned long long *row_sides);
int tqgpu_set_working_sets(tqgpu_solver *s, const unsigned long long *bounds, const unsigned long long *rows, const unsigned long long *bound_sides, const unsigned long long *row_sides);

/* ---- Parametric sensitivities of an MPC step: du0/dx0 (the feedback gain K), dz/dx0 and dlam/dx0 on the device ----------------------
 * How the answer of the last solve moves when x0 moves, at the point tqgpu_get_solution would return, with the active set frozen there.
 *   P_k                  the elimination matrix of node k for z_k = [x_k; u_k].  Kind 0: diagonal, 1/Qd_i (1/Rd_i) where the exported value
 *                        is strictly inside its bounds, 0.0 where it equals xmin / xmax (umin / umax) bit for bit (clipping assigns the
 *                        bound itself, so the comparison is exact); the phantom root states of an embedded x0-eliminated tree are free
 *                        (their A columns are zero).  Kind 1: P_k = H_k^-1, what the device keeps since its last factorisation of H_k.
 *   M                    the dual Hessian as the solver builds it: with C = [A_c B_c] stacked over the children c of p,
 *                        W_p = C P_p C' + blockdiag(P_c^{xx}),  Ut_p = -(C P_p)[:, :nx_p]';  with res_c = A_c x_p + B_c u_p + b_c - x_c
 *                        (class TQGPU_KKT_DYN), d res / d lam = -M.
 *   G                    G = d res / d x0 at fixed lam (sum_lam x nx0), non-zero only in the rows of the root's children c:
 *                        eliminated root (tqgpu_mpc_set_root):  G_c = A0_c - B_c P_0 S0  (the second term only where S0 was given);
 *                        root with states (tqgpu_mpc_set_root_states):  G_c = A_c.
 *   M dLam = G           solved block by block with the tall Cholesky of the solver and the regularisation rule of opts (regType, regTol,
 *                        regValue) as the solver's own factorisation applies it; n_reg: the blocks regularised.
 *   dZ                   dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) + direct_k  for every node k, with
 *                        direct_0 = -P_0 [0; S0] for an eliminated root, direct_0 = [I; 0] on the root's states for a root with states,
 *                        direct_k = 0 elsewhere.  K = the u rows of dZ_0.
 *   uniqueness           M = E P E', so a null vector v of M gives P E' v = 0: dZ (and K) is unique even where M is singular, as long as
 *                        G lies in the range of M; dLam is unique only when n_reg == 0.  This holds for an exact solve, and for what the
 *                        call computes under regType 0: a pivot <= 0 gives a zero column, that entry of dLam is 0.0 and the rest is the
 *                        solve without it.  The on-the-fly rule (regType 2, the default) adds regValue to the diagonal of the WHOLE
 *                        flagged block: where M is singular (a pinned state, xmin == xmax) dZ and K then differ from the exact
 *                        derivative by O(regValue), some 1e-6 at the default regValue = 1e-6.  Pinned by tests/test_sens_reg_reference.py
 *                        (test_the_zero_column_is_the_exact_derivative, test_the_default_shift_moves_dz_by_its_size) and
 *                        tests/test_gpu_mpc_sens_reg.py.
 *   tqgpu_mpc_sensitivity   evaluates all of it for the point of the last solve, whatever its route and status.  Like tqgpu_kkt_residual it
 *                        reads the export block (the packing is enqueued unless it went out ahead or a certified step packed the point)
 *                        and the problem data in place.  Launches, one wave per unit, ordered by launch boundaries on the mirror's
 *                        stream (no kernel waits for another workgroup): 1 (W, Ut, P, G) + one per block level, deepest first (tall
 *                        Cholesky of [W; Ut], Schur complement into the parent's W; the root carries G' as nx0 extra rows) + one per
 *                        block level below the root (grid: blocks x nx0) + 1 (dZ, K).  The results stay on the device; K (nu[0] x nx0,
 *                        column major), u0*, x0_ref (the x0 last folded) and n_reg come back through pinned memory in one copy, with
 *                        one wait.  It works in buffers of its own (allocated on first use, freed by tqgpu_destroy) and changes nothing
 *                        a later solve, tqgpu_get_solution or tqgpu_kkt_residual reads.  Counted into tqgpu_mpc_stats.
 *                        TQGPU_EINVAL: before tqgpu_mpc_set_root / _set_root_states, before the first solve, opts == NULL, and where the
 *                        problem was changed (an upload, an x0 fold, a window move) since the last solve: the point and the data must
 *                        belong together.
 *                        TQGPU_EUNSUPPORTED: a tree with nodes of kind 2 or 3 (Pd need not belong to the final working set after a line
 *                        search's last trial), a rank of a sharded solve, a tall root block [W; G'] that does not fit 160 KiB of LDS.
 *   tqgpu_mpc_get_gain   K, u0*, x0_ref of the last tqgpu_mpc_sensitivity (any pointer may be NULL; host state only).
 *   tqgpu_mpc_get_sensitivities   dx, du, dlam: column j of each array is the flat layout of tqgpu_get_solution for parameter x0[j]
 *                        (sum_nx x nx0, sum_nu x nx0, sum_lam x nx0; phantom root states excluded).  Downloads and waits: a stream
 *                        synchronisation and up to three blocking copies, which tqgpu_mpc_stats does not count (a diagnostic read-out).
 *   tqgpu_mpc_predict    one kernel and one wait.  With dx_j = x0_new[j] - x0_ref[j] every entry is one chain, j ascending:
 *                          v = u0*[i];  v = fma(K[i, j], dx_j, v);
 *                        on a root of kind 0 the result is clipped into [umin[0], umax[0]] as the device holds them, n_clipped counts the
 *                        entries moved.  duals != 0: the same launch (a wave per node) writes lam*_e + sum_j dLam[e, j] dx_j into the
 *                        start buffer, v = lam*[e]; v = fma(dLam[e, j], dx_j, v), j ascending.  That start holds for ONE solve in any
 *                        warm-start mode, by the mechanism of tqgpu_mpc_shift: the buffer of tqgpu_set_lambda is saved and restored the
 *                        same way.
 * A stored sensitivity is invalidated by any upload that changes the problem (tqgpu_set_*, an x0 fold, a window move) and by a new solve:
 * the getters and tqgpu_mpc_predict then return TQGPU_EINVAL, as they do before the first tqgpu_mpc_sensitivity. */
int tqgpu_mpc_sensitivity(tqgpu_solver *s, const tqgpu_opts *opts, int *n_reg);
int tqgpu_mpc_get_gain(tqgpu_solver *s, double *K, double *u0, double *x0_ref);
int tqgpu_mpc_get_sensitivities(tqgpu_solver *s, double *dx, double *du, double *dlam);
int tqgpu_mpc_predict(tqgpu_solver *s, const double *x0_new, double *u0_pred, int duals, int *n_clipped);

/* ---- The adjoint of an MPC step: dL/dq, dL/dr, dL/db and dL/dx0 on the device ----------------------------------------------------------
 * The reverse of the sensitivities above.  For a scalar loss L of the step's solution z = (x, u) and w = dL/dz, with the active set frozen
 * at the point tqgpu_get_solution would return, the KKT system is symmetric: the adjoint is one more solve with the same dual Hessian M,
 * with one right-hand side per column of w instead of nx0, and a right-hand side that is non-zero in every block.  P_k, M, C_c = [A_c B_c],
 * W_p, Ut_p as above; w_k = [wx_k; wu_k], the phantom root states of an embedded x0-eliminated tree carry w = 0.
 *   R                    rows of child c of p:  R_c = (P_c w_c)^x - C_c P_p w_p
 *   M Y = R              the same tall Cholesky, the same regularisation rule of opts, the same n_reg.  Block by block with L, CholUt as the
 *                        factorisation leaves them: leaf to root, every non-root block ii, deepest level first, t_ii = L_ii^-1 R_ii and
 *                        R_dad[pos .. pos + nx_ii) -= CholUt_ii t_ii (the rows of different children of one parent are disjoint: no
 *                        atomics); at the root t_0 = L_0^-1 R_0, Y_0 = L_0^-T t_0; root to leaves Y_ii = L_ii^-T ( t_ii - CholUt_ii' Y_dad[pos ..] ).
 *   gb                   gb_c = Y_c  (dL/db_c, sum_lam entries)
 *   gq, gr               [gq_k; gr_k] = -P_k ( w_k - [Y_k; 0] + sum_c C_c' Y_c )  for every node k ([Y_0; 0] = 0 at the root)
 *   gx0                  eliminated root (tqgpu_mpc_set_root):  gx0 = sum_c A0_c' Y_c + S0' gr_0  (the second term where S0 was given);
 *                        root with states (tqgpu_mpc_set_root_states):  gx0 = wx_0 + sum_c A_c' Y_c.
 *   uniqueness           R lies in the range of M = E P E', so gq and gr are unique even where M is singular;
 *                        gb is unique only when n_reg == 0, and on the same condition gx0 of an eliminated root.  As for the
 *                        sensitivities: true of an exact solve and of the zero column of regType 0; under the on-the-fly shift gq, gr and
 *                        gx0 move by O(regValue) with the whole flagged block.
 *   tqgpu_mpc_adjoint    wx ((sum_nx without phantom root states) x nw) and wu (sum_nu x nw): column j is the flat layout of
 *                        tqgpu_get_solution; either may be NULL, meaning zero.  One host-to-device copy of w through pinned memory, the
 *                        launches (one wave per unit and column, the nw columns on grid dimension y, ordered by launch boundaries on the
 *                        mirror's stream): 1 (R) + one per block level, deepest first (t, the push; the root completes Y_0) + one per
 *                        block level below the root (Y) + 1 (gq, gr, gb, gx0), that is 2 Nh + 1; then one device-to-host copy of
 *                        [gx0 | n_reg] and one wait.  The factor: where tqgpu_mpc_sensitivity (or an earlier tqgpu_mpc_adjoint) has left
 *                        the factor of this point on the device, it is used as it is (built with the opts of that call); otherwise the
 *                        call builds it first exactly as tqgpu_mpc_sensitivity does, Nh + 1 more launches (3 Nh + 2 in all), plus the
 *                        packing of the point where that has not gone out.  Results are the same bit for bit either way, and column j of
 *                        a call with nw columns is bit for bit the call with that column alone.  It works in buffers of its own
 *                        (allocated on first use, again when nw grows, freed by tqgpu_destroy) and changes nothing a later solve,
 *                        tqgpu_get_solution or tqgpu_kkt_residual reads, nor a stored sensitivity: tqgpu_mpc_predict and the getters
 *                        above keep their values.  Counted into tqgpu_mpc_stats (2 copies, 1 wait).
 *                        TQGPU_EINVAL, TQGPU_EUNSUPPORTED: wherever tqgpu_mpc_sensitivity returns them; TQGPU_EINVAL also for nw < 1;
 *                        TQGPU_EUNSUPPORTED also, before any launch, for an nw with (nz nw + 2) * 8 > 160 KiB for a node's nz = nx + nu
 *                        (the rule of the sensitivity's nz x nx0 window).
 *   tqgpu_mpc_get_adjoint_x0   gx0 (nx0 x nw, column major) of the last tqgpu_mpc_adjoint (host state only).
 *   tqgpu_mpc_get_adjoint      gq ((sum_nx without phantom root states) x nw), gr (sum_nu x nw), gb (sum_lam x nw), column major; any
 *                        pointer may be NULL.  Downloads and waits; not counted (a diagnostic read-out).
 * A stored adjoint is invalidated by the same events as a stored sensitivity; the getters then return TQGPU_EINVAL.  The gradients with
 * respect to H, A, B are outer products of these vectors with the solution: tqgpu_mpc_adjoint_matrices below. */
int tqgpu_mpc_adjoint(tqgpu_solver *s, const tqgpu_opts *opts, const double *wx, const double *wu, int nw, int *n_reg);
int tqgpu_mpc_get_adjoint_x0(tqgpu_solver *s, double *gx0);
int tqgpu_mpc_get_adjoint(tqgpu_solver *s, double *gq, double *gr, double *gb);
/* The adjoint of a batch of steps in one set of launches per device: what tqgpu_mpc_adjoint does for one mirror, for n of them.
 *   wx, wu               the members' blocks one behind the other, member 0 first: member i's block is what tqgpu_mpc_adjoint takes for it,
 *                        ((sum_nx_i without phantom root states) x nw) and (sum_nu_i x nw), column major; either may be NULL, meaning
 *                        zero; nw is the same for every member.
 *   gx0, n_reg           may be NULL; the members' nx0_i x nw blocks one behind the other, and n ints.
 *   per device           the members of one device form a group led by its first member, whose stream carries everything: three copies
 *                        (the descriptors with the members' level tables, w of all members, the heads [gx0 | n_reg] of all members) and one
 *                        wait, whatever n; launches, with Nh_max the deepest member's block levels: [1, the packing of the points, where a
 *                        member that lacks the factor has not packed its point] + [1 + Nh_max, where a member lacks the factor] +
 *                        1 + Nh_max + (Nh_max - 1) + 1.  Blocks z of the grid are the members, y the columns, x what it is in the single
 *                        launches; the backward launch j takes level Nh_i - 1 - j of member i, the forward launch j level j + 1, a
 *                        shallower member finishes early.  The arithmetic of a member is that of its own tqgpu_mpc_adjoint: every
 *                        result is the same bit for bit.  Counted into tqgpu_mpc_stats.
 *   state                afterwards every member is as a successful tqgpu_mpc_adjoint leaves it (tqgpu_mpc_get_adjoint_x0 and
 *                        tqgpu_mpc_get_adjoint read its own buffers; the factor counts as stored); the flags are set after the wait has
 *                        succeeded.  A stored sensitivity and everything a solve reads are left alone.
 *   member by member     groups of fewer than ADJ_BATCH_MIN members (tdunes_adjoint.hpp), of more than 65 535, or in which one tree dwarfs
 *                        the others (the rule of tqgpu_kkt_residual_batch), and every group under TREEQP_AMD_ADJ_BATCH=members, go through
 *                        tqgpu_mpc_adjoint one member after the other: same results and state, the counts are the sum of the single calls.
 *   refusals             before any member is touched, with the member's index in the message: whatever tqgpu_mpc_adjoint refuses for a
 *                        member; TQGPU_EINVAL for n < 1, solvers == NULL, opts == NULL, nw < 1 and a mirror named twice.  Every member's
 *                        stored adjoint and sensitivity are then as before. */
int tqgpu_mpc_adjoint_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *opts, const double *wx, const double *wu, int nw, double *gx0, int *n_reg);
/* The sensitivities and the predictor of a batch of steps in one set of launches per device: what tqgpu_mpc_sensitivity and tqgpu_mpc_predict
 * do for one mirror, for n of them.
 *   tqgpu_mpc_sensitivity_batch
 *   n_reg                may be NULL; n ints.
 *   per device           the members of one device form a group led by its first member, whose stream carries everything: two copies (the
 *                        descriptors with the members' level tables; the heads [K | u0* | x0_ref | n_reg] of all members) and one wait,
 *                        whatever n; launches, with Nh_max the deepest member's block levels: [1, the packing of the points, where a member
 *                        has not packed its point] + (1 + Nh_max) + (Nh_max - 1) + 1.  Blocks z of the grid are the members, x what it is in
 *                        the single launches, y of the forward sweep the column of x0: the grid is as tall as the largest nx0_i, a wave beyond
 *                        its member's nx0 returns at once; the factor launch j takes level Nh_i - 1 - j of member i, the forward launch j
 *                        level j + 1.  Like the single call it always builds the factor anew.  The arithmetic of a member is that of its
 *                        own tqgpu_mpc_sensitivity: every result is the same bit for bit.  Counted into tqgpu_mpc_stats.  (The one wait
 *                        is that of a loop's steady state behind tqgpu_mpc_step_batch.  A member whose own stream may still hold work
 *                        the lead's stream has not seen -- uploads, a solve of its own, the set-up kernels of its first solve -- is
 *                        waited for first, once per such stream, as in tqgpu_mpc_adjoint_batch.)
 *   state                afterwards every member is as a successful tqgpu_mpc_sensitivity leaves it: tqgpu_mpc_get_gain,
 *                        tqgpu_mpc_get_sensitivities and tqgpu_mpc_predict of the member read the member's own buffers (the kernel that
 *                        fills a member's head on the device writes it a second time into the lead's block; the member's pinned head is
 *                        filled from the group's copy), the factor counts as stored, so that a later tqgpu_mpc_adjoint / _adjoint_batch
 *                        does not build it; the flags are set after the wait has succeeded.  A stored adjoint and everything a solve
 *                        reads are left as the single call leaves them.
 *   member by member     groups of fewer than SENS_BATCH_MIN members (tdunes_adjoint.hpp), of more than 65 535, or in which one tree dwarfs
 *                        the others (the rule of tqgpu_kkt_residual_batch), and every group under TREEQP_AMD_SENS_BATCH=members, go through
 *                        tqgpu_mpc_sensitivity one member after the other: same results and state, the counts are the sum of the single calls.
 *   refusals             before any member is touched, with the member's index in the message ("member i:"): whatever
 *                        tqgpu_mpc_sensitivity refuses for a member (kinds 2 / 3 and the LDS window included); TQGPU_EINVAL for n < 1,
 *                        solvers == NULL, opts == NULL and a mirror named twice.  Every member's stored sensitivity and adjoint are then
 *                        as before.
 *   tqgpu_mpc_predict_batch
 *   x0_new               required: the members' nx0_i vectors one behind the other, member 0 first.
 *   u0_pred, n_clipped   may be NULL; the members' nu[0]_i blocks one behind the other, and n ints.  duals is one flag for all members.
 *   per device           one launch on the lead's stream (blocks z: the members; x: 0 the prediction of u0, 1 + k node k of the start
 *                        buffer, with duals only), one copy (the descriptors) and one wait, whatever n; x0_new and the results travel
 *                        through a pinned block of the lead, which the kernel reads and writes in place.  The arithmetic of a member is
 *                        tqgpu_mpc_predict's chain, entry for entry; with duals every member's start buffer is treated as the single call
 *                        treats it (saved once and restored by the solve after the next in warm-start mode 0; it holds for ONE solve in
 *                        any mode).  Counted into tqgpu_mpc_stats.
 *   member by member     the rule and the switch of tqgpu_mpc_sensitivity_batch; the counts are the sum of the single calls.
 *   refusals             before any member is touched, with the member's index in the message: TQGPU_EINVAL for a member without a valid
 *                        sensitivity, for n < 1, solvers == NULL, x0_new == NULL and a mirror named twice.  No start buffer is changed then.
 * Groups on more than one device are built like tqgpu_mpc_adjoint_batch's; only one device could be tested. */
int tqgpu_mpc_sensitivity_batch(tqgpu_solver **solvers, int n, const tqgpu_opts *opts, int *n_reg);
int tqgpu_mpc_predict_batch(tqgpu_solver **solvers, int n, const double *x0_new, double *u0_pred, int duals, int *n_clipped);

/* ---- The adjoint of an MPC step in H, A, B: outer products on the device, summed over parameter groups and over a batch -----------------
 * Behind tqgpu_mpc_adjoint (or tqgpu_mpc_adjoint_batch), for every column j of w.  z_k = [x_k; u_k] is the point tqgpu_get_solution would
 * return, gz_k = [gq_k; gr_k] and gb_c = Y_c the stored adjoint, C_c = [A_c B_c], (E v)_c = C_c v_p - v_c^x.  With the active set frozen and
 * lam taken in the sign for which stationarity off the bounds reads H z + g + E' lam = 0,
 *     dL = gz' dg + gb' db + gz' dH z + lam' (dE gz) + gb' (dE z).
 * That lam is tqgpu_get_solution's lam as it stands, not its negative (settled by the dense KKT solve and the finite differences of the tests).
 *   kind-0 node k        (diagonal Qd, Rd)  gHd_k[i] = gz_k[i] * z_k[i], nx + nu entries; an entry on a bound has gz = 0, its gradient is 0.0 exactly
 *   kind-1 node k        (dense H_k = [Q S'; S R], (nx + nu)^2, column major)  gH_k = 1/2 (gz_k z_k' + z_k gz_k'); i >= j is computed and mirrored, so
 *                        the result is symmetric bit for bit
 *   child c of p         gA_c = lam_c gq_p' + gb_c x_p' (nx_c x nx_p),  gB_c = lam_c gr_p' + gb_c u_p' (nx_c x nu_p), column major
 *   eliminated root      (tqgpu_mpc_set_root)  gA0_c = gb_c x0' for the root's children, child after child, each nx_c x nx0 (the layout of A0), and
 *                        gS0 = gr_0 x0' (nu[0] x nx0) where S0 was given, 0.0 where it was not; x0 is the x0 last folded.  A root with states
 *                        has neither: gA0 and gS0 are not written
 *   phantom root states  of an x0-eliminated tree embedded in a uniform one (x_pad states in front of node 0, reported by tqgpu_mpc_get_param_groups)
 *                        count in the sizes of node 0's blocks and of its children's gA; their entries are written 0.0
 * These are gradients with respect to H, A, B as the device holds them.  Under tqgpu_mpc_set_tracking q and r depend on Q, R, S through the
 * fold; for H that chain rule stays with the caller, who has gh = [gq; gr] of the same groups for it (for the reference trajectory itself:
 * tqgpu_mpc_adjoint_reference below).
 *   groups               a parameter group is a set of nodes whose matrices are one learnable parameter.  hgroup[k] (int[Nn], -1: in no group) is
 *                        the group of node k's stage Hessian: all members have the same nx, nu, kind and phantom states.  cgroup[c] is the group
 *                        of node c's dynamics (A_c, B_c, b_c): all members have the same nx_c, nx_p, nu_p; cgroup[0] must be -1.  A NULL map
 *                        means every node is its own group (h-group k = node k, Nn groups; c-group c - 1 = node c, Nn - 1 groups; the
 *                        count given with a NULL map is not read).  The result of an h-group is the sum of its members' gH (gHd) and of
 *                        their linear terms gh = [gq; gr]; of a c-group the sum of gA, gB and gb.
 *   the order of the sum  is part of the contract.  The members of a group are taken in ascending node index and cut into chunks of
 *                        ADJMAT_CHUNK = 64 consecutive members.  A chunk's partial is one chain from 0.0 over its members in ascending order, per member
 *                          gA, gB:  acc = fma(lam_c[i], gz_p[j], acc);  acc = fma(gb_c[i], z_p[j], acc);
 *                          gHd:     acc = fma(gz_k[i], z_k[i], acc);
 *                          gH:      acc = fma(gz_k[i], z_k[j], acc);  acc = fma(z_k[i], gz_k[j], acc);   (i >= j; the partial is 0.5 * acc)
 *                          gh, gb:  acc = acc + gz_k[i],  acc = acc + gb_c[i].
 *                        The group's value is the plain sum of the partials in ascending chunk order (the first partial, then + the next); in the
 *                        batch form that sums over members the order is ascending (member, chunk).  No atomics are used anywhere: a value
 *                        depends neither on the grid nor on which call produced it.
 *   tqgpu_mpc_set_param_groups   validates the maps (TQGPU_EINVAL with the offending node in tqgpu_last_error: a value outside [-1, n), members of
 *                        unequal sizes, cgroup[0] != -1, a group without a member, a group that mixes kinds), builds the member lists and chunk
 *                        tables and uploads them once.  Kinds, the root form and nx0 are compared again at every call: the maps survive
 *                        tqgpu_set_objective_mixed and tqgpu_mpc_set_root (the tables are then built and uploaded again, once); a group that has
 *                        come to mix kinds is refused at the call.  TQGPU_EUNSUPPORTED: a group whose result blocks and one member's vectors do
 *                        not fit 160 KiB of LDS.  The tables are cleared only by another tqgpu_mpc_set_param_groups and tqgpu_destroy.
 *   tqgpu_mpc_get_param_groups   the counts, per h-group 5 ints (nx, nu, phantom states, members, the kind it has now), per c-group 4 ints (nx_c,
 *                        nx_p, nu_p, members), sizes as the device counts them, and root[4]: the rows of gA0 (the nx of the root's children; 0: a
 *                        root with states, no gA0 and gS0), nu[0], nx0, and nw, the columns of the stored adjoint (0: none is stored), by
 *                        which every output of tqgpu_mpc_adjoint_matrices is sized; any pointer may be NULL (host state only).  This
 *                        read-out is public so that a caller can size the outputs without repeating the library's bookkeeping.
 *   tqgpu_mpc_adjoint_matrices   needs a stored adjoint (TQGPU_EINVAL otherwise, as the getters: whatever invalidates it makes this call
 *                        TQGPU_EINVAL) and the groups; any output may be NULL.  An output holds its groups' blocks one behind the other,
 *                        ascending group and then column of w: gH (nx + nu entries of a kind-0 group, (nx + nu)^2 of a kind-1 group), gh (nx + nu),
 *                        gA (nx_c nx_p), gB (nx_c nu_p), gb (nx_c); gA0 and gS0 column after column.  One launch (k_adjmat_part: one wave per
 *                        chunk and column; a group of one chunk writes its result itself) and, where a group has more than one chunk, a
 *                        second (k_adjmat_sum); one copy through pinned memory and one wait, counted into tqgpu_mpc_stats.  It writes only
 *                        buffers of its own: a later solve, tqgpu_kkt_residual, a stored sensitivity and the stored adjoint keep their bits.
 *                        Refusals are the adjoint's: kinds 2 and 3 and ranks of a sharded solve have no stored adjoint.
 *   tqgpu_mpc_adjoint_matrices_batch   behind tqgpu_mpc_adjoint_batch.  Per device one copy of the descriptors, one or two launches (grid z: the
 *                        member), one copy of the results and one wait, whatever n.  reduce = 0: every member's blocks one behind the other in
 *                        every output, each member bit for bit its own single call.  reduce = 1: one set of blocks, the sum over the members in
 *                        member order (every chunk writes its partial, k_adjmat_reduce adds them in ascending (member, chunk) order); all
 *                        members must then have group tables of equal shapes, kinds, root terms and columns, otherwise TQGPU_EINVAL with the
 *                        member's index.  All refusals come before any member is touched: a member without a stored adjoint or groups, a mirror
 *                        named twice, n < 1, solvers == NULL, reduce outside {0, 1}.  Groups per device and the fall-back to member by member
 *                        (TREEQP_AMD_ADJ_BATCH=members, fewer than ADJ_BATCH_MIN members, lopsided groups) are tqgpu_mpc_adjoint_batch's; with
 *                        reduce = 1 the fall-back, and members on more than one device, add the members' results on the host in the same
 *                        member order (the same bits for groups of one chunk). */
int tqgpu_mpc_set_param_groups(tqgpu_solver *s, const int *hgroup, const int *cgroup, int n_hgroups, int n_cgroups);
int tqgpu_mpc_get_param_groups(tqgpu_solver *s, int *n_hgroups, int *n_cgroups, int *hdims, int *cdims, int *root);
int tqgpu_mpc_adjoint_matrices(tqgpu_solver *s, double *gH, double *gh, double *gA, double *gB, double *gb, double *gA0, double *gS0);
int tqgpu_mpc_adjoint_matrices_batch(tqgpu_solver **solvers, int n, int reduce, double *gH, double *gh, double *gA, double *gB, double *gb, double *gA0, double *gS0);

/* ---- The adjoint of an MPC step in the bounds and in the tracking reference -----------------------------------------------------------------
 * Behind tqgpu_mpc_adjoint (or tqgpu_mpc_adjoint_batch), for every column j of w.  The frozen-active-set KKT system is H z + g + E' lam + I_A' mu = 0,
 * E z + b = 0, z_A = l_A; its adjoint K a = [w; 0; 0] gives gq = -a_z, gb = -a_lam = Y and dL/dl_A = a_mu = (w - H a_z - E' a_lam)_A.  On a kind-0
 * node H is diagonal and a_z vanishes on A, so with v_k = w_k - [Y_k; 0] + sum_c C_c' Y_c, the vector k_adj_grad multiplies by -P_k,
 *     dL/dbound_k[i] = v_k[i]   where the exported value equals that bound bit for bit (the test that makes P_k[i] = 0.0),
 *                      0.0      elsewhere, on every entry of a kind-1 node (its bounds are not read) and on phantom root states.
 *   side                 the value equals xmin (umin): the lower gradient takes v, the upper is 0.0; otherwise it equals xmax (umax): the upper
 *                        gradient takes v.  Where min == max bit for bit (a pinned entry; every state of a root with states) the lower gradient
 *                        therefore is the derivative for both bounds moved together: on the states of a root with states it equals gx0 bit for
 *                        bit.  Wherever a bound gradient is written from v, gq / gr of that entry is 0.0, and the reverse.
 *   tqgpu_mpc_get_adjoint_bounds   gxmin, gxmax ((sum_nx without phantom root states) x nw), gumin, gumax (sum_nu x nw), column major, the layout
 *                        of tqgpu_mpc_get_adjoint's gq / gr; any pointer may be NULL.  k_adj_grad (and its batch form: after
 *                        tqgpu_mpc_adjoint_batch every member holds those of its own call, bit for bit) stores them beside gq, gr in the
 *                        adjoint's own buffers; this is a diagnostic read-out like tqgpu_mpc_get_adjoint: it downloads, waits and is not
 *                        counted.  TQGPU_EINVAL where tqgpu_mpc_get_adjoint returns it.
 * Two sums over node sets are computed on the device (k_nodesum_part, k_nodesum_sum).  The order of each sum is part of the contract.  The members of
 * a set are taken in ascending node index and cut into chunks of ADJMAT_CHUNK = 64 consecutive members; a chunk's partial is one chain from 0.0 over
 * its members in that order; a result is the first of its partials plus the others in ascending order.  No atomics: a value depends neither on the
 * grid nor on which call produced it.  One launch (one wave per chunk and column; a result of one partial is written by its chunk), a second where
 * a result has more than one partial, one copy through pinned memory and one wait, counted into tqgpu_mpc_stats.  Both calls write only buffers of
 * their own: a later solve, tqgpu_kkt_residual, a stored sensitivity, the stored adjoint and a result of tqgpu_mpc_adjoint_matrices keep their bits.
 *   tqgpu_mpc_adjoint_bounds   the bound gradients summed over the h-groups of tqgpu_mpc_set_param_groups (a NULL map: every node its own group).
 *                        glb, gub: per h-group nx + nu entries [x | u], groups ascending, then columns of w: layout and sizes of gh of
 *                        tqgpu_mpc_adjoint_matrices (tqgpu_mpc_get_param_groups); either may be NULL.  Per member acc = acc + v[i]; the
 *                        partials are those of the group's chunks in ascending chunk order.  A kind-1 group's block and phantom entries are
 *                        written 0.0.  Refusals are those of tqgpu_mpc_adjoint_matrices: no stored adjoint, no groups, a group that has come to
 *                        mix kinds.
 *   tqgpu_mpc_adjoint_reference   under tqgpu_mpc_set_tracking the fold of node k reads row rho_k = min(t0 + stage[k], T - 1) and
 *                        [q_k; r_k] = base_k - H_k [xref; uref]_rho, hence [gxref; guref]_rho = - sum over {k : rho_k = rho} of H_k' [gq_k; gr_k]
 *                        (dL/dq0, dL/dr0 are gq, gr as they stand).  row0 = min(t0, T - 1) and rows, up to row min(t0 + deepest stage, T - 1),
 *                        for the window t0 in force; gxref (rows x NXT) and guref (rows x NUT), stage-major like xtraj / utraj, column of w
 *                        outermost.  Any pointer may be NULL; row0, rows are host state only: with both arrays NULL the call gives the sizes
 *                        and touches nothing else.  A set is a stage (the member lists and chunks are cut per stage and uploaded once by
 *                        tqgpu_mpc_set_tracking; they do not depend on t0).  Per member, one chain per entry j:
 *                          kind 0:  acc[j] = fma(-Qd[j], gq[j], acc[j]),  likewise Rd, gr;
 *                          kind 1:  for column j of the stored H_k (nz x nz, column major)  acc[j] = fma(-H[i + j nz], gz[i], acc[j]), i ascending
 *                                   over the rows behind the phantom root states, which contribute nothing and are no columns;
 *                          an x0-eliminated root with S0, behind its own chain:  acc[j] = fma(-S0[m + j nu0], gr_0[m], acc[j]), m ascending
 *                                   (the mirror image of + S0' gr_0 in gx0); its own chain gives -R_0 gr_0 to guref.
 *                        A leaf contributes to gxref only.  A row's partials are those of its stages in ascending (stage, chunk) order: a clamped
 *                        last row collects several stages, T == 1 all of them.  TQGPU_EINVAL: no stored adjoint, before
 *                        tqgpu_mpc_set_tracking, no window in force (tqgpu_mpc_get_window gives -1; a window moved after the solve has
 *                        invalidated the adjoint).  TQGPU_EUNSUPPORTED: what the adjoint refuses (kinds 2 and 3, ranks of a sharded solve). */
int tqgpu_mpc_get_adjoint_bounds(tqgpu_solver *s, double *gxmin, double *gxmax, double *gumin, double *gumax);
int tqgpu_mpc_adjoint_bounds(tqgpu_solver *s, double *glb, double *gub);
int tqgpu_mpc_adjoint_reference(tqgpu_solver *s, double *gxref, double *guref, int *row0, int *rows);

/* ---- The tangent of an MPC step: dz, dlam along directions in q, r, b, x0, and a predictor that follows the tracking reference -----------------
 * The forward-mode twin of the adjoint above: how the point of the last solve moves along a direction (dq, dr, db, dx0) of the linear terms,
 * with the active set frozen.  There the solution is affine in (q, r, b, x0), so the tangent along a FINITE change is exact until the active set
 * changes.  P_k, M, C_c = [A_c B_c], G, direct_k, the factor and n_reg as in the two sections above; dh_k = [dq_k; dr_k], phantom root states carry 0.
 *   R                    rows of child c of p:  R_c = (P_c dh_c)^x - C_c P_p dh_p + db_c + G_c dx0  (G_c: the rows of the root's children only)
 *   M dLam = R           with the stored factor where there is one (tqgpu_mpc_sensitivity, tqgpu_mpc_adjoint or an earlier call left it), otherwise
 *                        built first exactly as tqgpu_mpc_sensitivity does; the two sweeps are the adjoint's own kernels on the tangent's buffers.
 *   dZ                   dZ_k = P_k ( [dLam_k; 0] - sum_c C_c' dLam_c ) - P_k dh_k + direct_k dx0;  du0 = the u rows of dZ_0.
 *   order                R: the adjoint's expression for w := dh, then + db_c where db was given, then v = fma(G[., j], dx0[j], v), j ascending, where
 *                        dx0 was given.  dZ: the adjoint's chain -P_k ( dh_k - [dLam_k; 0] + sum_c C_c' dLam_c ), then the direct term: a root with
 *                        states + dx0[i]; an eliminated root with S0  s = S0 dx0 (a chain from 0.0, j ascending), v = fma(-P_0[i, nx + m], s[m], v),
 *                        m ascending.  A term that was not given is skipped, not added as 0.0.  So with db == dx0 == NULL (dx, du, dlam) equals
 *                        (gq, gr, gb) of tqgpu_mpc_adjoint(wx = dq, wu = dr) on the same mirror bit for bit, and column j of a call with nd
 *                        columns is bit for bit the call with that column alone.
 *   uniqueness           as for the adjoint: dZ is unique where R lies in the range of M (db moves R out of it only where a state is pinned);
 *                        dLam is unique only when n_reg == 0.
 *   tqgpu_mpc_tangent    nd directions, column major: dq ((sum_nx without phantom root states) x nd), dr (sum_nu x nd), db (sum_lam x nd, the flat
 *                        layout of b), dx0 (nx0 x nd); any may be NULL, meaning zero.  One host-to-device copy of the directions through pinned
 *                        memory; the launches (one wave per unit and column, columns on grid dimension y, ordered by launch boundaries on the
 *                        mirror's stream): [Nh + 1 for the factor where none is stored, plus the packing of the point where that has not gone
 *                        out] + 1 (k_tan_rhs) + Nh (k_adj_backward) + Nh - 1 (k_adj_forward) + 1 (k_tan_primal: dZ, dLam, the head), that is
 *                        2 Nh + 1 behind a stored factor; one device-to-host copy of [du0 | n_reg] and one wait.  Counted into tqgpu_mpc_stats
 *                        (2 copies, 1 wait).  It works in buffers of its own (allocated on first use, again when nd grows, freed by
 *                        tqgpu_destroy): a stored sensitivity, a stored adjoint and everything a solve, tqgpu_get_solution or tqgpu_kkt_residual
 *                        reads keep their bits; the factor counts as stored afterwards.
 *                        TQGPU_EINVAL, TQGPU_EUNSUPPORTED: wherever tqgpu_mpc_adjoint returns them, with nd for nw (kinds 2 and 3, a rank of a
 *                        sharded solve, (nz nd + 2) * 8 > 160 KiB, a problem changed since the last solve, before the first solve);
 *                        TQGPU_EINVAL also for nd < 1 and where all four directions are NULL.  All of them before any launch.
 *   tqgpu_mpc_get_tangent_u0   du0 (nu[0] x nd, column major) of the last tangent (host state only).
 *   tqgpu_mpc_get_tangent      dx ((sum_nx without phantom root states) x nd), du (sum_nu x nd), dlam (sum_lam x nd), column major; any pointer
 *                        may be NULL.  Downloads and waits; not counted (a diagnostic read-out).
 *   tqgpu_mpc_predict_at   one direction, built on the device: the change the next tqgpu_mpc_step_at(s, x0_new, t0_new) will fold in, measured from
 *                        the point of the last solve.  dx0 = x0_new - x0_ref (x0_new == NULL: no dx0 term); db = 0; t0_new < 0 keeps the window
 *                        (dh = 0); t0_new >= 0, under tqgpu_mpc_set_tracking with a window t0 in force: for node k with
 *                        rho(t) = min(t + stage[k], T - 1), dxref = xtraj[rho(t0_new)] - xtraj[rho(t0)], duref likewise, and dh_k is the chain of
 *                        the window fold started from 0.0: kind 0  dq[i] = fma(-Qd[i], dxref[i], 0.0), likewise Rd, duref; kind 1  row i of H_k,
 *                        v = fma(-H[i, j], dxref[j], v) over the x columns, then the u columns with duref; the u rows of an eliminated root
 *                        with S0 go on with v = fma(-S0[i, j], dxref[j], v) (the + S0 dx0 term is direct_0's and is not added twice).
 *                        Then the solve above with nd = 1 and ONE more kernel (k_tan_apply): u0_pred[i] = u0*[i] + du0[i], clipped into
 *                        [umin[0], umax[0]] on a root of kind 0 (n_clipped counts the entries moved); duals != 0: a wave per node writes
 *                        lam*[e] + dLam[e] into the start buffer, which holds for ONE solve in any warm-start mode, by the mechanism of
 *                        tqgpu_mpc_predict.  x0_new goes in and [u0_pred | n_clipped | n_reg] come back through pinned memory, which the kernels
 *                        read and write in place; no q, r, b, trajectory row or direction crosses the bus.  Behind a stored factor: 2 Nh + 2
 *                        launches, 1 copy (the head [du0 | n_reg], for tqgpu_mpc_get_tangent_u0) and 1 wait, counted into tqgpu_mpc_stats; without
 *                        one, the factor's launches in front as above.  The call moves neither the window nor x0 (tqgpu_mpc_get_window and
 *                        x0_ref are unchanged; the step that follows folds both); its tangent stays readable through the two getters.
 *                        Refusals: those of tqgpu_mpc_tangent; TQGPU_EINVAL also for t0_new >= 0 before tqgpu_mpc_set_tracking, before a window
 *                        is in force, and where tqgpu_mpc_step_at refuses the window (nx0 != NXT on an eliminated root with S0).
 * A stored tangent is invalidated by the same events as a stored adjoint; the getters then return TQGPU_EINVAL. */
int tqgpu_mpc_tangent(tqgpu_solver *s, const tqgpu_opts *opts, const double *dq, const double *dr, const double *db, const double *dx0, int nd, int *n_reg);
int tqgpu_mpc_get_tangent_u0(tqgpu_solver *s, double *du0);
int tqgpu_mpc_get_tangent(tqgpu_solver *s, double *dx, double *du, double *dlam);
int tqgpu_mpc_predict_at(tqgpu_solver *s, const tqgpu_opts *opts, const double *x0_new, int t0_new, double *u0_pred, int duals, int *n_clipped, int *n_reg);

/* Device times [s] of the last n solves (oldest first), measured with HIP events on the solver's
 * stream around everything a solve enqueues; synchronises the stream; returns the number written
 * (at most 512 solves back) or -1.  tqgpu_result.device_time of a single-launch (persistent) solve is
 * the kernel's own clock from launch start to verdict instead, so that tqgpu_solve can return as soon
 * as the verdict is in pinned host memory. */
int tqgpu_get_device_times(tqgpu_solver *s, double *out, int n);
/* Per-solve event pairs on (default) or off.  Off: a solve that is ONE persistent launch is enqueued with nothing around it
 * (two queue packets fewer per solve); tqgpu_get_device_times then reports NaN for such solves.  No counterpart in the
 * reference (its timers are host timers, treeqp/utils/timing.c:39-61). */
int tqgpu_set_event_timing(tqgpu_solver *s, int on);

/* diagnostic in-kernel time stamps of the last fused iteration (TREEQP_AMD_STAMPS=1) */
int tqgpu_get_stamps(tqgpu_solver *s, unsigned long long *out, int cap);
/* test support: a foreign kernel holding compute units (blocks x 256 threads, lds_kb KiB of LDS each, spinning for ms milliseconds
 * on its own stream; returns at once), and the wait for it */
int tqgpu_debug_occupy(int device, int blocks, int lds_kb, int ms);
int tqgpu_debug_occupy_wait(void);

/* sizeof() of the public structs (0 dmat, 1 dvec, 2 node, 3 tree_qp_in, 4 tree_qp_out,
 * 5 tdunes opts, 6 tdunes workspace, 7 profiling record, 8 qp_internal_t) for FFI self-checks */
int treeqp_amd_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif  /* TREEQP_AMD_H_ */

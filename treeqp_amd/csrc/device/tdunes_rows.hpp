/*
 * tdunes_rows.hpp -- the kernels of every instantiated (nx, nu, md), as data: each table of tdunes_parts.hpp is expanded ONCE in host code, here,
 * into a constant array with one row per table line.  A row holds the shape, the sizes that depend on it and typed pointers to its kernels.
 * detect_fast / detect_multistage, plan_members and tqgpu_pshard_init look a row up once and keep the pointer; the launch helpers launch through
 * it and never switch on a shape.  The kernels stay external symbols that the part owning the family defines (their declarations are enough for
 * a pointer), so a new line in a table of tdunes_parts.hpp needs no other host edit: its row, its lookup and its launches follow from the line.
 * Host part only, in the unnamed namespace (plain records: no dynamic symbol).  Included by tdunes_device.hip behind tdunes_mirror.hpp.
 */
#pragma once

namespace {

/* one signature per kernel: the tier kernels (tdunes_fast.hpp), the persistent family and its batch form (tdunes_persist.hpp) */
typedef void (*BackFn)(Tree, Data, Opts, Shard, int, int, int, int, int, int, int);
typedef void (*TopFn)(Tree, Data, Opts, Shard, int, int, int, int, int, int);
typedef void (*FwdFn)(Tree, Data, Opts, Shard, int, int, int, int);
typedef void (*StageFn)(Tree, Data, Opts, const int *, int, int, int, int);
typedef void (*PersistFn)(PConst, Opts, PGeom, PSync, int);
typedef void (*BatchFn)(const PItem *, Opts, int, unsigned, int);

/* the three builds of a single-device persistent kernel: plain, the one that can keep factors (checkLastActiveSet == 2), the one for one workgroup per CU */
struct PersistKernels { PersistFn plain, reuse, one; };

/* a line of FAST_TABLE or MSTAGE_TABLE; idx is the table's own (sparse) index, what Uniform::fast holds.  Sizes in bytes.  A multistage line has the
 * index and the shape of a FAST_TABLE line, and its row everything that line's row has; chain_lds and mpersist are set in MSTAGE_ROWS only. */
struct ShapeRow {
    int idx, nx, nu, md;
    int TH;                          /* levels per tier (Uni<>::TH) */
    size_t tier_lds, stage_lds;      /* f_back / f_top / f_fwd; f_stage */
    size_t persist_lds;              /* PLds<nx, nu, md> */
    BackFn back; TopFn top; FwdFn fwd; StageFn stage;
    PersistKernels persist;          /* f_persist<.., false>, f_persist<.., true>, f_persist_one */
    size_t chain_lds;                /* PLds<nx, nu, 1>: the chain tiers of a multistage tree */
    PersistKernels mpersist;         /* f_mpersist<.., false>, f_mpersist<.., true>, f_mpersist_one */
};
struct ShardRow { int idx, nx, nu, md; PersistFn agent, sys; };      /* f_persist_sh<.., 0>, f_persist_sh<.., 1> */
struct BatchRow { int idx, nx, nu, md; bool mstage; BatchFn batch; };

#define TQ_UNI_ROW(idx, nx, nu, md) \
    idx, nx, nu, md, Uni<nx, nu, md>::TH, Uni<nx, nu, md>::TIER_LDS * sizeof(double), FW * (Uni<nx, nu, md>::D + nx + 8) * sizeof(double), \
    PLds<nx, nu, md>::DOUBLES * sizeof(double), f_back<nx, nu, md>, f_top<nx, nu, md>, f_fwd<nx, nu, md>, f_stage<nx, nu, md>, \
    {f_persist<nx, nu, md, false>, f_persist<nx, nu, md, true>, f_persist_one<nx, nu, md>}

#define X(idx, nx, nu, md) {TQ_UNI_ROW(idx, nx, nu, md), 0, {nullptr, nullptr, nullptr}},
const ShapeRow FAST_ROWS[] = {
    FAST_TABLE(X)
};
#undef X
#define X(idx, nx, nu, md) {TQ_UNI_ROW(idx, nx, nu, md), PLds<nx, nu, 1>::DOUBLES * sizeof(double), {f_mpersist<nx, nu, md, false>, f_mpersist<nx, nu, md, true>, f_mpersist_one<nx, nu, md>}},
const ShapeRow MSTAGE_ROWS[] = {
    MSTAGE_TABLE(X)
};
#undef X
#undef TQ_UNI_ROW
#define X(idx, nx, nu, md) {idx, nx, nu, md, f_persist_sh<nx, nu, md, 0>, f_persist_sh<nx, nu, md, 1>},
const ShardRow SHARD_ROWS[] = {
    SHARD_TABLE(X)
};
#undef X
#define X(idx, nx, nu, md, ms) {idx, nx, nu, md, ms, f_persist_batch<nx, nu, md, ms>},
const BatchRow BATCH_ROWS[] = {
    BATCH_TABLE(X)
};
#undef X

/* the row of a shape, nullptr: the table has no line for it */
template <typename Row, size_t N>
const Row *find_row(const Row (&rows)[N], int nx, int nu, int md) {
    for (const Row &r : rows) if (r.nx == nx && r.nu == nu && r.md == md) return &r;
    return nullptr;
}
const BatchRow *find_batch_row(int nx, int nu, int md, bool mstage) {
    for (const BatchRow &r : BATCH_ROWS) if (r.nx == nx && r.nu == nu && r.md == md && r.mstage == mstage) return &r;
    return nullptr;
}

}  // namespace

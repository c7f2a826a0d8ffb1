/* mz_gpu.h — C ABI of the MI355X-native incremental join/reduce engine.
 *
 * This is the drop-in boundary for Materialize's compute hot path
 * (SURVEY.md §8b). Each entry point states the reference interface it
 * replaces (file:line under /root/reference). A Rust host would bind these
 * over plain `extern "C"` FFI; no torch types appear
 * here — plain pointers and sizes only.
 *
 * Ownership: the caller owns all host/device memory passed in via
 * descriptors until the call returns. The library owns arrangements,
 * operators and returned out-batches; out-batches are freed with
 * mz_gpu_out_release. All calls on one context must be serialized by the
 * caller (one driver thread per GPU, mirroring one timely worker per core —
 * src/compute/src/server.rs:327-377).
 *
 * Errors: non-zero int return; mz_gpu_last_error(ctx) gives a message.
 */
#ifndef MZ_GPU_H
#define MZ_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mz_gpu_ctx mz_gpu_ctx;
typedef struct mz_gpu_arr mz_gpu_arr;   /* an arrangement (trace/spine) */
typedef struct mz_gpu_join mz_gpu_join; /* a linear-join operator (mz_join_core state) */
typedef struct mz_gpu_red mz_gpu_red;   /* an accumulable-reduce operator */

/* ---------------------------------------------------------------- schema */

/* Arrangement schema: fixed-width keys (1..2 u64 words) and vals (bytes).
 * Blueprint: RowRowSpine columnar layout, src/row-spine/src/lib.rs:56-135. */
typedef struct {
  uint32_t key_words;  /* 1 or 2; keys compared as i64-tuple ascending */
  uint32_t val_bytes;  /* 0..64 fixed width, or MZ_GPU_VARLEN: vals are
                          variable-length byte strings compared
                          lexicographically (shorter-prefix-first), the
                          reference's byte-arena row layout
                          (row-spine/src/lib.rs:110-135)              */
} mz_gpu_schema;

#define MZ_GPU_VARLEN 0xFFFFFFFFu

/* A set of updates ((key, val), time, diff), SoA columns.
 * `on_device` = 1 when the pointers are HIP device pointers on the ctx's
 * device; 0 for host memory (the library stages them in).
 * This is both the delta-batch input format and the sealed-batch push
 * format; sealed batches must additionally be sorted by (key, val, time)
 * and consolidated (duplicate (key,val,time) diffs summed, zeros dropped) —
 * use mz_gpu_consolidate to produce that form. */
typedef struct {
  const uint64_t *keys;   /* [key_words * n] key words, key-major          */
  const uint8_t  *vals;   /* [val_bytes * n], may be NULL if val_bytes==0  */
  const uint64_t *times;  /* [n] */
  const int64_t  *diffs;  /* [n] */
  uint64_t n;
  uint64_t lower, upper;  /* batch time bounds [lower, upper)              */
  int32_t  on_device;
  /* 1 when rows are already sorted ascending by (key, val, time) in the
   * canonical order (the form mz_gpu_consolidate produces). Purely an
   * optimization hint: sorted delta streams probe large arrangements by
   * merge scan (streaming both sorted sides) instead of per-row hash
   * lookups. 0 is always safe. */
  int32_t  sorted;
  /* VARLEN schemas only: n+1 offsets into `vals` (the byte arena); row
   * i's val is vals[val_offs[i] .. val_offs[i+1]). NULL otherwise. */
  const uint32_t *val_offs;
} mz_gpu_updates;

/* ----------------------------------------------------------- closures
 * JoinClosure (src/compute-types/src/plan/join.rs:60-86) restated as a
 * filter + field-map spec evaluated inside the probe kernel. Fields are
 * copied from the probe inputs into the output (key,val) row. */
enum {
  MZ_SRC_KEY = 0,      /* the (shared) join key words                  */
  MZ_SRC_VAL_STREAM = 1, /* the delta/stream side's val bytes          */
  MZ_SRC_VAL_LOOKUP = 2, /* the arrangement side's val bytes           */
  MZ_SRC_COMPUTE = 3   /* computed field; `off` = compute id           */
};
enum { MZ_CMP_LT = 0, MZ_CMP_LE, MZ_CMP_GT, MZ_CMP_GE, MZ_CMP_EQ, MZ_CMP_NE };
enum {
  /* revenue = extendedprice_cents * (10000 - discount_bp) as i64 1e-4
   * units — Q3/Q5/Q10's `l_extendedprice * (1 - l_discount)` with TPC-H
   * fixed-scale decimals mapped to exact integers. Operand
   * offsets are given by arg0/arg1 on the out field. */
  MZ_COMPUTE_REVENUE = 0,
  /* 8 zero bytes (re-key to a constant, e.g. cross-join stages). */
  MZ_COMPUTE_CONST0 = 1,
  /* Q17's correlated-average filter, exact in integers:
   * quantity < 0.2 * sum/count  <=>  5*q*count < sum  (count > 0).
   * As a FILTER compute: arg0 = i64 quantity offset; arg1 = the offset of
   * a SUM_I64 aggregate slot's i128 value, with the COUNT slot's i64 at
   * arg1+24 (the 24-byte aggregate slot layout). NULL count (count==0 in
   * the reference's CASE, tpch_create_index.slt:1470) fails the filter. */
  MZ_COMPUTE_Q17_QTYLT = 2,
  /* i64 division as an OUT FIELD: arg0 / arg1 (both i64 at the given
   * offsets). arg1 == 0 raises MZ_ERR_DIVISION_BY_ZERO: the row is
   * diverted to the out-batch's error stream — the could_error ok/err
   * split of linear_join.rs:495-541. */
  MZ_COMPUTE_DIV_I64 = 3,
  /* i64 wrapping multiply as an OUT FIELD: arg0 * arg1 (both i64 at the
   * given offsets; Diff-style wrapping per overflowing.rs:24-31). Q6's
   * `l_extendedprice * l_discount` term. */
  MZ_COMPUTE_MUL_I64 = 4,
  /* Field-vs-field compare as a FILTER compute: passes iff
   * cmp(arg0_field, arg1_field) holds, both read at the filter's `width`
   * (4 or 8, signed LE) from (arg0_src, arg0) / (arg1_src, arg1) with
   * the filter's `cmp`. Q12's `l_commit_date < l_receipt_date` /
   * `l_ship_date < l_commit_date` predicates. */
  MZ_COMPUTE_CMP_FIELDS = 5
};

typedef struct {
  uint8_t  src;     /* MZ_SRC_* (KEY/VAL_STREAM/VAL_LOOKUP), or
                       MZ_SRC_COMPUTE with `off` = compute filter id    */
  uint16_t off;     /* byte offset into src (or compute id)            */
  uint8_t  width;   /* 4 or 8 (signed little-endian integer)           */
  uint8_t  cmp;     /* MZ_CMP_*                                        */
  int64_t  imm;     /* literal operand                                 */
  uint16_t arg0, arg1;          /* compute-filter operand offsets      */
  uint8_t  arg0_src, arg1_src;
} mz_gpu_filter;

typedef struct {
  uint8_t  src;     /* MZ_SRC_*                                        */
  uint16_t off;     /* byte offset (or compute id for MZ_SRC_COMPUTE)  */
  uint8_t  width;   /* bytes copied / produced                         */
  uint16_t arg0, arg1; /* compute operand byte offsets (both in VAL_*) */
  uint8_t  arg0_src, arg1_src;
} mz_gpu_field;

#define MZ_GPU_MAX_FILTERS 6
#define MZ_GPU_MAX_FIELDS  8

typedef struct {
  uint32_t n_filters;
  mz_gpu_filter filters[MZ_GPU_MAX_FILTERS];
  uint32_t n_key_fields;             /* output key (next stage / reduce) */
  mz_gpu_field key_fields[MZ_GPU_MAX_FIELDS];
  uint32_t n_val_fields;             /* output val                        */
  mz_gpu_field val_fields[MZ_GPU_MAX_FIELDS];
  mz_gpu_schema out;                 /* shape of the output rows          */
} mz_gpu_closure;

/* ------------------------------------------------------------- reduce
 * AccumulablePlan (src/compute-types/src/plan/reduce.rs:233) restated.
 * Accum semantics follow src/compute/src/render/reduce.rs:1611-2270:
 * SimpleNumber = wrapping i128 + non_nulls; Float = 24-frac-bit fixed-point
 * wrapping i128 + inf/nan/non_null counts; COUNT = non_nulls only. */
enum {
  MZ_AGG_COUNT = 0,
  MZ_AGG_SUM_I64,    /* also exact-decimal sums (i64 cents etc.)       */
  MZ_AGG_SUM_F64,    /* fixed-point accumulation, reduce.rs:1641-1697  */
  /* Hierarchical aggregates — mz_gpu_collation_* only (mz_gpu_reduce_create
   * rejects them). The datum is `width` (4 or 8) bytes at `off`, signed
   * little-endian, sign-extended to i64; `nullable` must be 0. */
  MZ_AGG_MIN_I64,
  MZ_AGG_MAX_I64
};

typedef struct {
  uint8_t  func;     /* MZ_AGG_*                                       */
  uint16_t off;      /* byte offset of the datum in the input val      */
  uint8_t  width;    /* 4 or 8                                         */
  uint8_t  is_float; /* datum is f64 (for SUM_F64)                     */
  uint8_t  nullable; /* datum has a null indicator byte at off+width   */
  uint8_t  distinct; /* COUNT/SUM(DISTINCT x), see below. Occupies the
                        struct's former padding byte: sizeof stays 8 and 0
                        is the plain aggregate                            */
} mz_gpu_aggregate;

/* distinct = 1 — AccumulablePlan::distinct_aggrs (plan/reduce.rs:233,
 * rendered by build_accumulable, render/reduce.rs:1357-1581, which keeps
 * one distinct arrangement of (key, datum) per such aggregate): the
 * aggregate sees each distinct datum of a key once, for as long as the net
 * multiplicity of (key, datum) is nonzero. The operator keeps a resident
 * (key, datum) count table per distinct aggregate and feeds the accumulator
 * only the presence changes (±1) of those pairs.
 *   - MZ_AGG_COUNT / MZ_AGG_SUM_I64 over a 4- or 8-byte signed LE datum at
 *     `off` (inside in.val_bytes), sign-extended to i64; distinctness is
 *     equality of that i64. `nullable` is honoured: a NULL datum
 *     contributes nothing; a key whose datums are all NULL finalizes
 *     SUM(DISTINCT) to the NULL slot and COUNT(DISTINCT) to 0.
 *   - MZ_AGG_MIN_I64 / MZ_AGG_MAX_I64 accept the flag and ignore it.
 *   - MZ_AGG_SUM_F64 or is_float with distinct is rejected at create time
 *     (float Datum equality is not byte equality).
 * The per-key row count that decides key existence and "all NULL -> NULL"
 * stays the net input row count. */

#define MZ_GPU_MAX_AGGS 4

typedef struct {
  uint32_t n_aggs;
  mz_gpu_aggregate aggs[MZ_GPU_MAX_AGGS];
  mz_gpu_schema in;   /* input (key,val) schema                        */
  mz_gpu_schema out;  /* output: key + finalized aggregate row         */
} mz_gpu_reduce_spec;

/* --------------------------------------------------------------- context */

typedef struct {
  uint64_t hbm_pool_bytes;   /* 0 = default                            */
  uint32_t device_index;
} mz_gpu_cfg;

mz_gpu_ctx *mz_gpu_init(const mz_gpu_cfg *cfg);
void        mz_gpu_fini(mz_gpu_ctx *ctx);
const char *mz_gpu_last_error(mz_gpu_ctx *ctx);
/* Synchronize the context's stream (all prior calls complete). */
int         mz_gpu_sync(mz_gpu_ctx *ctx);

/* ----------------------------------------------------------- arrangement
 * Replaces mz_arrange_core + Spine maintenance
 * (src/compute/src/extensions/arrange.rs:69-114,
 *  src/compute/src/arrangement/manager.rs:54). */
mz_gpu_arr *mz_gpu_arr_create(mz_gpu_ctx *ctx, const mz_gpu_schema *schema);
void        mz_gpu_arr_drop(mz_gpu_ctx *ctx, mz_gpu_arr *arr);
/* Push a sealed, sorted, consolidated batch (see mz_gpu_updates docs). */
int  mz_gpu_arr_push_batch(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                           const mz_gpu_updates *batch);
/* Consolidate raw updates and push the sealed batch in one call (the
 * MergeBatcher + arrange step fused — no intermediate out-batch). */
int  mz_gpu_arr_insert(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                       const mz_gpu_updates *raw);

/* Overlapped maintenance: the async form enqueues the insert's
 * consolidation+build on the arrangement's own HIP stream and returns
 * without a device sync; the sealed batch joins the spine at
 * mz_gpu_arr_flush (any probe of the arrangement flushes implicitly, as
 * does mz_gpu_sync). Independent arrangements' inserts overlap this way.
 * mz_gpu_arr_insert == insert_async + flush.
 * Lifetime: host-memory updates are staged inside the call (pageable
 * async copies complete in-call); DEVICE-pointer updates must stay
 * valid until the arrangement is flushed (explicitly or by a probe). */
int  mz_gpu_arr_insert_async(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                             const mz_gpu_updates *updates);
int  mz_gpu_arr_flush(mz_gpu_ctx *ctx, mz_gpu_arr *arr);
/* Advance the logical compaction frontier (times advance to it on merge) —
 * cf. set_logical_compaction, mz_join_core.rs:461. */
int  mz_gpu_arr_set_logical_compaction(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                                       uint64_t frontier);
/* Physical-compaction hint (mz_join_core.rs:465): a floor on batch
 * merging. This spine merges eagerly by level policy,
 * so the hint is recorded but imposes nothing — batches at or beyond
 * the frontier are already merged as the policy reaches them. */
int  mz_gpu_arr_set_physical_compaction(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                                        uint64_t frontier);
/* Perform up to `fuel` rows of spine merge work — cf. manager.rs:54. */
int  mz_gpu_arr_maintain(mz_gpu_ctx *ctx, mz_gpu_arr *arr, uint64_t fuel);
/* Introspection (arrangement-size logging, extensions/arrange.rs:249). */
int  mz_gpu_arr_stats(mz_gpu_ctx *ctx, mz_gpu_arr *arr, uint64_t *n_batches,
                      uint64_t *n_updates, uint64_t *hbm_bytes);

/* ------------------------------------------------------------- out batch */
typedef struct {
  uint64_t *keys;  uint8_t *vals;  uint64_t *times;  int64_t *diffs;
  uint64_t n;
  int32_t on_device;      /* 1: device pointers (default)              */
  mz_gpu_schema schema;
  /* Error-row stream: the ok/err split of the reference's join closure
   * (JoinClosure::could_error, linear_join.rs:495-541). A closure field
   * whose evaluation errors (e.g. MZ_COMPUTE_DIV_I64 by zero) diverts
   * the would-be output row here as (error code, time, diff),
   * consolidated like any update stream. err_* are device arrays owned
   * by the out-batch (NULL/0 when the closure cannot error). */
  uint64_t err_n;
  uint64_t *err_codes;    /* MZ_ERR_* per row */
  uint64_t *err_times;
  int64_t  *err_diffs;
  /* VARLEN schemas only (schema.val_bytes == MZ_GPU_VARLEN): n+1
   * offsets into `vals`; val_arena_bytes = val_offs[n]. */
  uint32_t *val_offs;
  uint64_t val_arena_bytes;
} mz_gpu_out;

enum { MZ_ERR_DIVISION_BY_ZERO = 1 };

/* VARLEN out-batches: copy the [n+1] val offsets to the host; `vals`
 * passed to mz_gpu_out_to_host must then be sized val_arena_bytes. */
int mz_gpu_out_voffs_to_host(mz_gpu_ctx *ctx, const mz_gpu_out *out,
                             uint32_t *offs);

/* Copy an out-batch's error rows to caller host buffers (sized err_n). */
int mz_gpu_out_err_to_host(mz_gpu_ctx *ctx, const mz_gpu_out *out,
                           uint64_t *codes, uint64_t *times,
                           int64_t *diffs);

/* Flush like mz_gpu_arr_flush, and additionally hand back the pending
 * insert's CONSOLIDATED flat rows as a sorted out-batch (*out = NULL when
 * no insert was pending or it was empty). This is the arrangement's
 * update stream: the same sealed rows the reference's mz_arrange_core
 * publishes to downstream operators (extensions/arrange.rs:69-114) —
 * delta-path probes consume it with `sorted = 1`. Caller releases. */
int mz_gpu_arr_flush_take(mz_gpu_ctx *ctx, mz_gpu_arr *arr,
                          mz_gpu_out **out);

void mz_gpu_out_release(mz_gpu_ctx *ctx, mz_gpu_out *out);
/* Copy an out-batch's columns to caller host buffers (sized n). */
int  mz_gpu_out_to_host(mz_gpu_ctx *ctx, const mz_gpu_out *out,
                        uint64_t *keys, uint8_t *vals, uint64_t *times,
                        int64_t *diffs);

/* Sort by (key,val,time), consolidate diffs, drop zeros — DD
 * consolidate_updates as used at mz_join_core.rs:604. */
int  mz_gpu_consolidate(mz_gpu_ctx *ctx, const mz_gpu_schema *schema,
                        const mz_gpu_updates *in, mz_gpu_out **out);

/* ------------------------------------------------------------ linear join
 * Replaces mz_join_core (mz_join_core.rs:57-496). The operator tracks the
 * acknowledged frontier of each side implicitly: a push probes the opposing
 * arrangement AS OF the call. Push concurrent batches side-1-first to
 * reproduce the reference's drain order (exactly-once). */
mz_gpu_join *mz_gpu_join_create(mz_gpu_ctx *ctx, mz_gpu_arr *arr1,
                                mz_gpu_arr *arr2, const mz_gpu_closure *cl);
void mz_gpu_join_drop(mz_gpu_ctx *ctx, mz_gpu_join *op);
/* Join `delta` (side = 1 or 2, already consolidated) against the opposing
 * arrangement; output consolidated. NOTE: push the delta to its own
 * arrangement via mz_gpu_arr_push_batch BEFORE or AFTER this call per the
 * reference discipline: arr_push(arr1,b1); join_push(1,b1);
 * arr_push(arr2,b2); join_push(2,b2). */
int  mz_gpu_join_push(mz_gpu_ctx *ctx, mz_gpu_join *op, int side,
                      const mz_gpu_updates *delta, mz_gpu_out **out);

/* ------------------------------------------------------------- half join
 * Replaces half_join2 (delta_join.rs:500,544): probe `delta`'s updates
 * (whose `times` are the promoted data-times) against `lookup`; a trace
 * update at t' matches a stream update at t iff t' <= t (le=1; source
 * relation precedes lookup relation) or t' < t (le=0) —
 * delta_join.rs:362,372. Output time = t. Output consolidated.
 * `stream_val_bytes` = the delta updates' val stride (the stream row was
 * re-keyed/thinned by the previous stage and need not match `lookup`'s). */
int  mz_gpu_halfjoin(mz_gpu_ctx *ctx, mz_gpu_arr *lookup,
                     const mz_gpu_updates *delta, uint32_t stream_val_bytes,
                     int le, const mz_gpu_closure *cl, mz_gpu_out **out);

/* Fused two-stage delta path (one path's two lookup stages,
 * delta_join.rs:338-472, in a single kernel): delta -> lookup1 (le1,
 * closure1 produces the intermediate key/val in registers) -> lookup2
 * (le2, closure2 produces the output). Equivalent to two halfjoin calls
 * with the intermediate stream never materialized; output is RAW
 * (unconsolidated — the consumer consolidates) with the err stream
 * attached. Constraints: fixed-width lookups; closure1's output key
 * must be lookup2's key schema, its output <= 2 key words / 48 val
 * bytes. */
int  mz_gpu_halfjoin2(mz_gpu_ctx *ctx, mz_gpu_arr *lookup1, int le1,
                      const mz_gpu_closure *cl1, mz_gpu_arr *lookup2,
                      int le2, const mz_gpu_closure *cl2,
                      const mz_gpu_updates *delta,
                      uint32_t stream_val_bytes, mz_gpu_out **out);

/* --------------------------------------------------------------- reduce
 * Replaces build_accumulable + mz_reduce_abelian (reduce.rs:1357-1581,
 * extensions/reduce.rs:131). The operator owns the resident accumulator
 * table AND the output arrangement; each push returns output corrections
 * (new minus old finalized rows, diffs ±1) per changed key. Input updates
 * are (key, input-val) rows; the datum→accumulator move (explode_one,
 * reduce.rs:1409-1431) happens inside. Multi-timestamp batches are
 * processed in time order. */
mz_gpu_red *mz_gpu_reduce_create(mz_gpu_ctx *ctx,
                                 const mz_gpu_reduce_spec *spec);
void mz_gpu_reduce_drop(mz_gpu_ctx *ctx, mz_gpu_red *op);
int  mz_gpu_reduce_push(mz_gpu_ctx *ctx, mz_gpu_red *op,
                        const mz_gpu_updates *delta, mz_gpu_out **out);

/* Diagnostics: when the environment sets MZ_GPU_PROF=1, the engine
 * records per-phase HIP event pairs; this prints and resets the sums
 * ("MZPROF <phase> <ms> <count>" lines on stdout). No-op otherwise. */
void mz_gpu_prof_dump(mz_gpu_ctx *ctx);

/* ----------------------------------------------------------- threshold
 * Replaces build_threshold_basic / threshold_local
 * (src/compute/src/render/threshold.rs:34-51,75-97): a reduce over the
 * row-keyed arrangement that keeps each record whose accumulated count is
 * positive, with that count as the output multiplicity
 * (count.is_positive() filter, threshold.rs:42). The operator owns the
 * resident per-(key,val) net-count table; each push returns corrections
 * with diff = pos(new_count) - pos(old_count) per changed record
 * (reduce_abelian contract, src/compute/src/extensions/reduce.rs:131).
 * Output schema equals the input schema. */
typedef struct mz_gpu_thr mz_gpu_thr;
mz_gpu_thr *mz_gpu_threshold_create(mz_gpu_ctx *ctx,
                                    const mz_gpu_schema *schema);
int  mz_gpu_threshold_push(mz_gpu_ctx *ctx, mz_gpu_thr *op,
                           const mz_gpu_updates *delta, mz_gpu_out **out);
void mz_gpu_threshold_drop(mz_gpu_ctx *ctx, mz_gpu_thr *op);

/* ----------------------------------------------------------------- topk
 * Replaces render_topk's Basic plan path — build_topk /
 * build_topk_negated_stage (src/compute/src/render/top_k.rs:322-418,
 * 614-770): per group-key, order records by the order columns
 * (ColumnOrder asc/desc; compare_columns at :733-739, ties broken in the
 * engine's canonical val order, standing in for the reference's Row-order
 * tie-break :738), then keep the multiplicity window [offset,
 * offset+limit) of the running prefix (:743-766). The operator owns the
 * resident group-contents state; each push returns corrections (new
 * minus old kept rows per changed group, reduce_abelian contract).
 * Restrictions vs the reference: literal limits only (no
 * per-key limit expressions, :659-688); order columns are non-null signed
 * little-endian integers of width 4 or 8; the monotonic plan variants
 * (MonotonicTop1/TopK, :157-288) are streaming-input optimizations whose
 * output equals Basic's and are not separate entry points; the bucketed
 * stage hierarchy (:380-398) is a work-thinning policy that leaves the
 * final modulus-1 stage's output unchanged, so groups are evaluated
 * directly. Negative input multiplicities return an error
 * ("Negative multiplicities in TopK", :494). */
typedef struct {
  uint16_t off;    /* byte offset of the order datum in the val bytes */
  uint8_t  width;  /* 4 or 8 (signed little-endian integer)           */
  uint8_t  desc;   /* 1 = descending                                  */
} mz_gpu_order_col;

#define MZ_GPU_MAX_ORDER 4

typedef struct {
  mz_gpu_schema in;  /* group key words + record val bytes            */
  uint64_t offset;   /* rows to skip per group (TopKPlan::offset)     */
  int64_t  limit;    /* rows to keep after offset; < 0 = no limit     */
  uint32_t n_order;
  mz_gpu_order_col order[MZ_GPU_MAX_ORDER];
} mz_gpu_topk_spec;

typedef struct mz_gpu_topk mz_gpu_topk;
mz_gpu_topk *mz_gpu_topk_create(mz_gpu_ctx *ctx,
                                const mz_gpu_topk_spec *spec);
int  mz_gpu_topk_push(mz_gpu_ctx *ctx, mz_gpu_topk *op,
                      const mz_gpu_updates *delta, mz_gpu_out **out);
void mz_gpu_topk_drop(mz_gpu_ctx *ctx, mz_gpu_topk *op);

/* ------------------------------------------------------------ exchange
 * Replaces the Exchange pact routing (linear_join.rs:390,
 * extensions/arrange.rs:134): shard = splitmix64(key words) % nshards
 * (hash substitution per DESIGN.md §2.2). Writes each update into its
 * shard's contiguous region of the caller-provided output columns (device
 * or host, matching `in->on_device`) and fills counts[nshards]. The
 * collective itself is the caller's (RCCL all-to-all-v over xGMI). */
int  mz_gpu_partition(mz_gpu_ctx *ctx, const mz_gpu_schema *schema,
                      const mz_gpu_updates *in, uint32_t nshards,
                      uint64_t *out_keys, uint8_t *out_vals,
                      uint64_t *out_times, int64_t *out_diffs,
                      uint64_t *counts);

/* -------------------------------------------------------------- flat map
 * FlatMap / key-preparation analog (src/compute/src/render/flat_map.rs;
 * DeltaJoinKeyPreparation, delta_join.rs:444-464): apply a closure to a
 * stream without a lookup (VAL_STREAM = the input val). */
int  mz_gpu_map(mz_gpu_ctx *ctx, const mz_gpu_schema *in,
                const mz_gpu_updates *updates, const mz_gpu_closure *cl,
                mz_gpu_out **out);

/* --------------------------------------------------- hierarchical reduce
 * Replaces build_bucketed/build_monotonic + ReductionMonoid
 * (src/compute/src/render/reduce.rs:850-1224, :2273): MIN/MAX maintained
 * through a val-hash bucket reduction tree (plan/reduce.rs:319-326);
 * retracting the current extremum recomputes only the affected buckets.
 * Input vals are single i64 datums; pushes are single-timestamp.
 * `buckets` e.g. {4096, 256, 16, 1} (last level = per key). */
typedef struct mz_gpu_minmax mz_gpu_minmax;
mz_gpu_minmax *mz_gpu_minmax_create(mz_gpu_ctx *ctx,
                                    const mz_gpu_schema *in, int is_max,
                                    const uint32_t *buckets,
                                    uint32_t n_levels);
int  mz_gpu_minmax_push(mz_gpu_ctx *ctx, mz_gpu_minmax *op,
                        const mz_gpu_updates *delta, mz_gpu_out **out);
void mz_gpu_minmax_drop(mz_gpu_ctx *ctx, mz_gpu_minmax *op);

/* ------------------------------------------------------- collated reduce
 * Replaces ReducePlan::Collation / build_collation
 * (src/compute/src/render/reduce.rs): a GROUP BY that mixes reduction
 * types, e.g. COUNT(*), SUM(a), MIN(b), MAX(c). Each reduction type runs on
 * its own — one accumulable sub-reduce over all COUNT/SUM aggregates, one
 * hierarchical bucket tree per MIN/MAX aggregate — and a final stitch
 * keeps, per key, every part's current value and emits one output row per
 * key in the SQL aggregate order.
 *
 * Output row: one 24-byte slot per aggregate in spec order. COUNT/SUM
 * slots are the mz_gpu_reduce_* slots; a MIN/MAX slot is [0] = 0 (never
 * null), [8..16) = the i64 extremum, remaining bytes zero.
 * Corrections follow the reduce_abelian contract: per changed key -1 of
 * the old stitched row and +1 of the new one, nothing when they are
 * byte-equal, only the retraction when the group becomes empty; the output
 * is consolidated and in canonical order.
 *
 * Restrictions (each an error via mz_gpu_last_error): fixed-width schemas
 * only; single-timestamp pushes (upper <= lower + 1); 1..MZ_GPU_MAX_AGGS
 * aggregates, each reading inside in.val_bytes; MIN/MAX inputs not
 * nullable. A key present in some reduction types but not in others (only
 * possible with negative input multiplicities) fails the push with
 * "collation: key missing a reduction type" — the condition the reference
 * logs as an error in its collation reduce. */
typedef struct {
  uint32_t n_aggs;                         /* 1..MZ_GPU_MAX_AGGS, SQL order  */
  mz_gpu_aggregate aggs[MZ_GPU_MAX_AGGS];  /* any mix of the five funcs      */
  mz_gpu_schema in;                        /* input (key,val), fixed width   */
  mz_gpu_schema out;                       /* key_words = in.key_words,
                                              val_bytes = 24 * n_aggs        */
  uint32_t n_levels;                       /* minmax bucket tree, 1..4       */
  uint32_t buckets[4];                     /* e.g. {256,16,1}; last == 1     */
} mz_gpu_collation_spec;
typedef struct mz_gpu_collation mz_gpu_collation;
mz_gpu_collation *mz_gpu_collation_create(mz_gpu_ctx *ctx,
                                          const mz_gpu_collation_spec *spec);
int  mz_gpu_collation_push(mz_gpu_ctx *ctx, mz_gpu_collation *op,
                           const mz_gpu_updates *delta, mz_gpu_out **out);
void mz_gpu_collation_drop(mz_gpu_ctx *ctx, mz_gpu_collation *op);

/* ------------------------------------------------------------------ peek
 * Replaces the peek path (handle_peek/process_peeks,
 * src/compute/src/compute_state.rs:763,1155): read, for each requested
 * key, the arrangement's (val, summed diff) pairs as of `time` (updates at
 * t' <= time accumulate; zero-sum vals are dropped). `keys` are n_keys
 * host key rows. Out rows: (key, val, time, diff). */
int  mz_gpu_peek(mz_gpu_ctx *ctx, mz_gpu_arr *arr, const uint64_t *keys,
                 uint64_t n_keys, uint64_t time, mz_gpu_out **out);

/* Full-scan peek (IndexPeek with no literal constraints, compute_state.rs):
 * every (key, val) of the arrangement with its diffs at t' <= as_of summed,
 * passed through `mfp` (NULL = identity), consolidated. Out rows:
 * (key, val, as_of, diff) in canonical order, the format mz_gpu_peek
 * returns; rows whose mfp evaluation errors land in the out-batch's error
 * stream as (MZ_ERR_DIVISION_BY_ZERO, as_of, summed diff).
 * `mfp` is a closure over (MZ_SRC_KEY, MZ_SRC_VAL_LOOKUP = the stored val):
 * filters, a projection, computed fields. The reference fails a peek that
 * meets a negative net count ("saw retractions ... for row that does not
 * exist"); so does this call unless `allow_negative` is set, in which case
 * such rows are returned as they are.
 * An as_of at or beyond the arrangement's upper is legal and answers over
 * what is installed: waiting for the frontier is the caller's, as with
 * mz_gpu_peek. A pending mz_gpu_arr_insert_async batch whose lower bound is
 * beyond as_of is not waited for.
 * Errors (non-zero return, nothing allocated is kept): a varlen
 * arrangement; an mfp that reads MZ_SRC_VAL_STREAM, that reads past the
 * arrangement's key words or val bytes, or whose field widths do not add
 * up to its `out` schema (a computed field is 8 bytes); as_of
 * before the logical compaction frontier (times below it may already have
 * been advanced to it — the reference refuses peeks before `since`); a
 * negative net count without `allow_negative`.
 * ORDER BY / LIMIT finishing and key-range bounds are mz_gpu_peek_select's,
 * below. */
int  mz_gpu_peek_scan(mz_gpu_ctx *ctx, mz_gpu_arr *arr, uint64_t as_of,
                      const mz_gpu_closure *mfp, int allow_negative,
                      mz_gpu_out **out);

/* Peek with a key range and a finishing (IndexPeek::collect_finished_data,
 * compute_state.rs: the RowSetFinishing's order and limit + offset applied
 * while the index is walked, so that what leaves is the size of the answer).
 *
 * Range (NULL = all keys): applies to the STORED key, before the mfp,
 * compared as a signed i64 tuple of the arrangement's key_words words. A key
 * passes when it is at or above `lo` and at or below `hi`; an exclusive
 * bound makes that comparison strict, an unbounded side always passes, and
 * lo > hi is the empty answer, not an error. Only in-range keys are visited:
 * each batch's sorted keys are searched for the two ends, and the walk covers
 * the vals between them. stats->scanned_vals is the number of (batch, val)
 * items walked, stats->rows_matched the consolidated ok rows before
 * finishing.
 *
 * Scan, mfp, consolidation, as_of, the compaction frontier, pending async
 * inserts, allow_negative and the error stream are mz_gpu_peek_scan's; with
 * range == NULL and fin == NULL the out-batch is byte-equal to its.
 *
 * Finishing (NULL = none), over the consolidated ok rows (key, val, c),
 * c > 0. Rows are ordered by the order columns in spec order, ties broken
 * in the canonical (key, val) order. One column
 * compares as the reference's compare_columns: NULL equals NULL; a NULL is
 * greater than any datum when nulls_last is set and less otherwise, whatever
 * `desc` says; two datums compare as signed little-endian integers, reversed
 * under `desc`; the datum bytes of a NULL are ignored. An order column
 * addresses the mfp's OUT row (the stored row without an mfp): MZ_SRC_KEY a
 * key word, MZ_SRC_VAL_LOOKUP the val bytes. Row r then occupies positions
 * [lo_r, lo_r + c) of the expanded sequence; the positions [offset,
 * offset + limit) are kept ([offset, inf) when limit < 0; the sum does not
 * wrap), a row's out diff is the number of its copies kept, rows with none
 * are dropped, the out time is as_of. The total multiplicity is computed
 * exactly and a total above INT64_MAX fails the call ("peek_select: total
 * multiplicity exceeds int64") before anything is emitted. n_order == 0,
 * offset == 0, limit < 0 is the identity.
 * The out-batch of a finishing is in FINISHING order, not canonical order:
 * it must not be fed anywhere as `sorted = 1`.
 * Finishing does not touch the error stream. The reference fails a peek on
 * any error row, so the caller checks err_n before it uses the rows. There
 * is no finishing projection: an ORDER BY column must be in the mfp's
 * output, and the caller drops it (the mfp is the projection).
 *
 * Errors (non-zero return, nothing allocated is kept, message prefixed
 * "peek_select:"): everything mz_gpu_peek_scan refuses; a bound kind above
 * 2; a nonzero bound word beyond key_words or on an unbounded side; n_order
 * above MZ_GPU_MAX_ORDER; an order column whose src is neither MZ_SRC_KEY
 * nor MZ_SRC_VAL_LOOKUP, a key column that is not width 8, not at a word
 * boundary inside the out key, or with a null_off, a val column of width
 * other than 4, 8 or 16 or reading past the out val, a null_off past the
 * out val or inside its own datum, desc or nulls_last above 1; a finishing
 * together with allow_negative. */
enum { MZ_KB_UNBOUNDED = 0, MZ_KB_INCLUSIVE = 1, MZ_KB_EXCLUSIVE = 2 };
typedef struct {
  uint8_t lo_kind, hi_kind;      /* MZ_KB_*                                  */
  int64_t lo[2], hi[2];          /* first key_words words; i64-tuple order   */
} mz_gpu_key_range;

#define MZ_GPU_NO_NULL 0xFFFFu
typedef struct {                 /* 8 bytes; ColumnOrder restated            */
  uint8_t  src;        /* MZ_SRC_KEY | MZ_SRC_VAL_LOOKUP, of the OUT row      */
  uint8_t  width;      /* val: 4, 8 or 16 (signed LE); key: 8                 */
  uint8_t  desc;
  uint8_t  nulls_last;
  uint16_t off;        /* byte offset; key: 8 * word                          */
  uint16_t null_off;   /* val byte that is nonzero when the datum is NULL, or
                          MZ_GPU_NO_NULL. A window value slot and an
                          mz_gpu_mfp nullable field put it after the datum, a
                          reduce or collation slot at slot byte 0, before the
                          value at [8..24)                                    */
} mz_gpu_peek_order;

typedef struct {
  uint32_t n_order;              /* 0..MZ_GPU_MAX_ORDER                      */
  mz_gpu_peek_order order[MZ_GPU_MAX_ORDER];
  uint64_t offset;
  int64_t  limit;                /* < 0 = none                               */
} mz_gpu_finishing;

typedef struct {
  uint64_t scanned_vals;   /* (batch, val) items the scan walked             */
  uint64_t rows_matched;   /* consolidated ok rows before finishing          */
} mz_gpu_peek_stats;

int  mz_gpu_peek_select(mz_gpu_ctx *ctx, mz_gpu_arr *arr, uint64_t as_of,
                        const mz_gpu_key_range *range,   /* NULL = all keys  */
                        const mz_gpu_closure *mfp,       /* as mz_gpu_peek_scan */
                        const mz_gpu_finishing *fin,     /* NULL = none      */
                        int allow_negative,
                        mz_gpu_peek_stats *stats,        /* NULL = not wanted */
                        mz_gpu_out **out);

/* ------------------------------------------------------- temporal filter
 * Replaces the temporal half of MapFilterProject — MfpPlan { lower_bounds,
 * upper_bounds } and MfpPlan::evaluate (src/expr/src/linear.rs, mod plan;
 * lowered from `mz_now() <cmp> expr` predicates by MfpPlan::create_from in
 * the same file), as used by render/flat_map.rs, the join closures and
 * persist_source. A predicate on mz_now() gives a row a
 * validity interval, which is how sliding and tumbling windows and TTLs are
 * written (WHERE mz_now() >= ts AND mz_now() < ts + 30000).
 *
 * Row semantics, for an input update (key, val, t, d):
 *  1. The mfp's filters run first; a failing row yields nothing.
 *  2. lo = t, hi = none; the bounds are evaluated in spec order. A NULL
 *     datum: the row yields nothing (the predicate is NULL). v = datum + add
 *     is computed exactly, in 128 bits; v < 0 is not an mz_timestamp and
 *     yields the one error row (MZ_ERR_TIMESTAMP_OUT_OF_RANGE, t, d) and no
 *     ok row. MZ_TB_LOWER: lo = max(lo, v). MZ_TB_UPPER: hi = min(hi, v).
 *  3. hi exists and hi <= lo: the row yields nothing.
 *  4. Otherwise (proj(row), lo, d) unless lo >= until, and, if hi exists and
 *     hi < until, (proj(row), hi, -d); the negation wraps, as Diff does.
 * Unlike the reference, the projection may not contain a field that can
 * error (MZ_COMPUTE_DIV_I64): put the division in a following
 * mz_gpu_mfp program, whose out-batch has the error stream for it (that of
 * mz_gpu_map has none). Bound errors are emitted at the input time and are never held.
 *
 * Frontier and hold-back. The -d update usually lies in the future, beyond
 * the batch's upper. Timely lets such updates travel and the downstream
 * arrange batcher holds them; here the operator owns them. It keeps a
 * frontier f: UINT64_MAX (in stats) before the first push, which sets it to
 * delta.lower. A push must have delta.lower == f, upper >= lower and every
 * input time in [lower, upper); anything else is an error that leaves the
 * state untouched. Its out-batch is every update with time < delta.upper,
 * from this delta and from the held buffer, consolidated and in canonical
 * order; bound errors arrive in its error stream. Everything else stays
 * held, itself consolidated, so an insert's -d at hi cancels against the +d
 * at hi of the row's later deletion. f becomes delta.upper. An empty delta
 * with an advanced upper is a legal frontier tick that releases
 * expirations. All output times lie in [lower, upper): safe to insert into
 * an arrangement or push into a multi-timestamp reduce with those bounds.
 *
 * Refused at create (NULL, message in last_error): a varlen schema; an mfp
 * that reads MZ_SRC_VAL_LOOKUP, reads past the input row, has a
 * MZ_COMPUTE_DIV_I64 field, or whose out schema is wider than 2 key words /
 * 64 val bytes; n_bounds == 0 or > MZ_GPU_MAX_BOUNDS; a bound of unknown
 * kind, of a source other than the input row, of width other than 4 or 8,
 * or reading past the row. */
enum { MZ_TB_LOWER = 0,   /* mz_now() >= v : v is a lower bound (inclusive)  */
       MZ_TB_UPPER = 1 }; /* mz_now() <  v : v is an upper bound (exclusive) */
typedef struct {
  uint8_t  kind;      /* MZ_TB_*                                            */
  uint8_t  src;       /* MZ_SRC_KEY or MZ_SRC_VAL_STREAM (the input row)    */
  uint16_t off;       /* byte offset of the datum                           */
  uint8_t  width;     /* 4 or 8, signed LE, sign-extended                   */
  uint8_t  nullable;  /* null indicator byte at off+width, as aggregates    */
  int64_t  add;       /* v = datum + add, computed exactly (no wrap)        */
} mz_gpu_time_bound;
#define MZ_GPU_MAX_BOUNDS 4
typedef struct {
  mz_gpu_schema in;
  int32_t  has_mfp;  mz_gpu_closure mfp;   /* filters + projection over
                        (MZ_SRC_KEY, MZ_SRC_VAL_STREAM); 0 = identity       */
  uint32_t n_bounds; mz_gpu_time_bound bounds[MZ_GPU_MAX_BOUNDS]; /* >= 1   */
  uint64_t until;          /* outputs at time >= until are dropped;
                              UINT64_MAX = none                             */
  uint64_t initial_rows;   /* held-buffer capacity hint; 0 = default        */
} mz_gpu_temporal_spec;
typedef struct mz_gpu_temporal mz_gpu_temporal;
mz_gpu_temporal *mz_gpu_temporal_create(mz_gpu_ctx *ctx,
                                        const mz_gpu_temporal_spec *spec);
int  mz_gpu_temporal_push(mz_gpu_ctx *ctx, mz_gpu_temporal *op,
                          const mz_gpu_updates *delta, mz_gpu_out **out);
/* Held row count, the smallest held time (UINT64_MAX when nothing is held:
 * the first tick that produces output is the one past it) and f. */
int  mz_gpu_temporal_stats(mz_gpu_ctx *ctx, mz_gpu_temporal *op,
                           uint64_t *held_rows, uint64_t *next_time,
                           uint64_t *frontier);
void mz_gpu_temporal_drop(mz_gpu_ctx *ctx, mz_gpu_temporal *op);
enum { MZ_ERR_TIMESTAMP_OUT_OF_RANGE = 2 };

/* ------------------------------------------- scalar-expression MFP
 * Replaces the non-temporal half of MapFilterProject: SafeMfpPlan::evaluate
 * (src/expr/src/linear.rs) over MirScalarExpr trees — BinaryFunc::eval,
 * UnaryFunc::eval, VariadicFunc::And / Or / Coalesce, MirScalarExpr::If
 * (src/expr/src/scalar.rs, scalar/func.rs) — for the integer and boolean
 * datums this engine carries. A stateless stream operator: it sits before
 * or after any join, reduce or temporal filter. This is where a division
 * that the temporal filter's projection refuses goes (mz_gpu_map has no
 * error stream: do not put a field that can error there).
 *
 * The program is postfix over a value stack of at most MZ_GPU_XSTACK
 * entries. Pushes: COL, LIT, NULL. Unary: NEG ABS NOT IS_NULL. Binary
 * (left operand pushed first): ADD SUB MUL DIV MOD, LT LE GT GE EQ NE,
 * AND OR, COALESCE. Ternary: IF (cond, then, else pushed in that order).
 * Statements pop one value and leave the stack empty: FILTER, OUT.
 *
 * Value model. A value is (i64, tag): tag 0 = datum, 1 = NULL,
 * 1 + MZ_ERR_* = that error. Booleans are 0 / 1. COL sign-extends a 4- or
 * 8-byte little-endian integer; a width-1 COL reads a boolean byte; with
 * `nullable`, a nonzero byte at off + width makes the value NULL. Errors
 * are values: every operator is evaluated eagerly, and an operator the
 * reference evaluates lazily selects among its evaluated operands. As
 * expressions are pure, that is the lazy semantics.
 *
 * Strict operators (arithmetic, comparisons, NEG, ABS, NOT), in this order:
 * a left operand that is an error gives that error; else a right operand
 * that is an error gives that error; else any NULL operand gives NULL; else
 * the operator computes. (An error on the right beats a NULL on the left:
 * both operands are evaluated before the NULL check.)
 *   ADD SUB MUL  checked; overflow gives MZ_ERR_NUMERIC_FIELD_OVERFLOW.
 *   DIV          truncates toward zero; a zero divisor gives
 *                MZ_ERR_DIVISION_BY_ZERO; INT64_MIN / -1 gives
 *                MZ_ERR_INT64_OUT_OF_RANGE.
 *   MOD          a zero divisor gives MZ_ERR_DIVISION_BY_ZERO; the sign
 *                follows the dividend; INT64_MIN % -1 = 0.
 *   NEG ABS      of INT64_MIN give MZ_ERR_INT64_OUT_OF_RANGE.
 * AND: either operand a definite false gives false; else an operand that is
 * an error gives that error (the left one first); else either operand NULL
 * gives NULL; else true. OR is the dual on true. (When both operands error
 * with different codes the reference takes the larger EvalError; this takes
 * the left one — DESIGN.md §2.9.)
 * IS_NULL: an error stays an error; otherwise 0 / 1.
 * IF: an error condition is that error; a true condition gives the
 * then-value; a false or NULL condition the else-value. The value not taken
 * is discarded, errors included.
 * COALESCE(a, b): b when a is NULL, otherwise a (an error a included).
 * N-ary COALESCE / AND / OR are built by right-nesting.
 *
 * Statements run in program order; the first decisive one wins, and later
 * statements of a dropped or errored row have no effect.
 *   FILTER  an error makes the row the error row (code, time, diff) in the
 *           out-batch's error stream; false or NULL drops the row.
 *   OUT     the first matching rule decides: an error value makes the row
 *           an error row; a NULL into a non-nullable field gives
 *           MZ_ERR_UNEXPECTED_NULL; a width-4 store of a value outside i32
 *           gives MZ_ERR_INT32_OUT_OF_RANGE; otherwise the datum is stored.
 *           A NULL into a nullable field stores zero datum bytes and null
 *           byte 1 (canonical: byte-equal consolidation stays exact); a
 *           datum into a nullable field stores null byte 0.
 *
 * Refused (non-zero return, message in mz_gpu_last_error): n_ops >
 * MZ_GPU_MAX_XOPS; an unknown opcode; a stack that goes below 0 or above
 * MZ_GPU_XSTACK, is not empty after a statement or at the end; a COL of a
 * source other than MZ_SRC_KEY / MZ_SRC_VAL_STREAM, of width other than 1,
 * 4, 8, or reading past the input key or val (the null byte included); OUT
 * fields that do not tile the out key and the out val exactly (every byte
 * written once: no gap, no overlap); a key OUT that is not width 8 and
 * non-nullable; a varlen schema; a schema, in or out, outside 1..2 key
 * words and 0..64 val bytes.
 *
 * Out-batch: one row per passing input row, at the input's time and diff.
 * consolidate != 0: consolidated, in canonical order. consolidate == 0: the
 * raw rows in queue order, for a consolidating consumer. The error rows are
 * always consolidated. */
enum {
  MZ_X_COL = 0, MZ_X_LIT, MZ_X_NULL,
  MZ_X_NEG, MZ_X_ABS, MZ_X_NOT, MZ_X_IS_NULL,
  MZ_X_ADD, MZ_X_SUB, MZ_X_MUL, MZ_X_DIV, MZ_X_MOD,
  MZ_X_LT, MZ_X_LE, MZ_X_GT, MZ_X_GE, MZ_X_EQ, MZ_X_NE,
  MZ_X_AND, MZ_X_OR, MZ_X_COALESCE,
  MZ_X_IF,
  MZ_X_FILTER, MZ_X_OUT
};
enum { MZ_ERR_INT64_OUT_OF_RANGE = 3,
       MZ_ERR_NUMERIC_FIELD_OVERFLOW = 4,
       MZ_ERR_INT32_OUT_OF_RANGE = 5,
       MZ_ERR_UNEXPECTED_NULL = 6 };
#define MZ_GPU_MAX_XOPS 64
#define MZ_GPU_XSTACK   8
typedef struct {            /* 16 bytes */
  uint8_t  op;              /* MZ_X_* */
  uint8_t  src;             /* COL: MZ_SRC_KEY | MZ_SRC_VAL_STREAM; OUT: 0 = key, 1 = val */
  uint8_t  width;           /* COL / OUT: 1, 4 or 8 */
  uint8_t  nullable;        /* COL / OUT: null-indicator byte at off + width */
  uint16_t off;             /* COL / OUT: byte offset */
  uint16_t pad;
  int64_t  imm;             /* LIT */
} mz_gpu_xop;
typedef struct {
  uint32_t n_ops;
  mz_gpu_xop ops[MZ_GPU_MAX_XOPS];
  mz_gpu_schema in, out;
} mz_gpu_mfp_spec;
int  mz_gpu_mfp(mz_gpu_ctx *ctx, const mz_gpu_mfp_spec *spec,
                const mz_gpu_updates *updates, int consolidate,
                mz_gpu_out **out);

/* ------------------------------------------------------ window functions
 * Replaces ReducePlan::Basic for the window AggregateFuncs — RowNumber,
 * Rank, DenseRank, LagLead, FirstValue, LastValue and WindowAggregate over
 * SUM / COUNT / MIN / MAX (src/expr/src/relation/func.rs), which
 * build_basic_aggregate (src/compute/src/render/reduce.rs) evaluates by
 * recomputing a whole
 * partition whenever any row of it changes and emitting new minus old. The
 * operator owns an arrangement of the partition contents, as mz_gpu_topk
 * does.
 *
 * Output row: the key unchanged; the val is the input val bytes followed by
 * one slot per function, in spec order. A ROW_NUMBER, RANK, DENSE_RANK or
 * COUNT slot is an i64 (8 bytes). A value slot (LAG, LEAD, FIRST_VALUE,
 * LAST_VALUE, SUM, MIN, MAX) is 9 bytes: the datum sign-extended to i64,
 * then a null byte — what mz_gpu_mfp reads as `COL width 8 nullable`. NULL is eight zero
 * bytes and null byte 1 (canonical, as mz_gpu_mfp's OUT). out.val_bytes =
 * in.val_bytes + the slots, at most 64.
 *
 * Semantics. Take one partition (key) as of the push time: its rows
 * (val, m), net multiplicity m > 0, ordered by the order columns, ties
 * broken in the engine's canonical val order (the deviation TopK records,
 * DESIGN.md §2.5). The reference repeats a row m times, so the partition is
 * the expanded sequence E[0..M), M = sum of m, row r occupying [lo_r, hi_r).
 * A peer group is a maximal run of rows whose order-column values are all
 * equal; with n_order == 0 the whole partition is one peer group. At
 * position p:
 *   ROW_NUMBER   p + 1
 *   RANK         lo of the first row of p's peer group, plus 1
 *   DENSE_RANK   1 + the number of peer groups before p's
 *   LAG(x, k)    the datum of E[p - k] if p - k >= 0, else the default
 *   LEAD(x, k)   the datum of E[p + k] if p + k < M, else the default
 *                (k = 0 is the row's own datum; a NULL datum stays NULL;
 *                the default is `dflt` with has_default, else NULL)
 *   FIRST_VALUE  the datum of E[0], for either frame
 *   LAST_VALUE   MZ_WF_FRAME_TO_CURRENT: the datum of the last row of p's
 *                peer group; MZ_WF_FRAME_PARTITION: the datum of E[M - 1]
 * The partition's output is one row (key, val ++ slots) of diff 1 per
 * position, consolidated. Each push returns corrections (reduce_abelian
 * contract, as mz_gpu_topk): per changed partition -(old output) and
 * +(new output) at the slice's time, consolidated and in canonical order,
 * so unchanged rows cancel; a partition that becomes empty yields only
 * retractions. Multi-timestamp pushes are processed per time slice, in time
 * order.
 *
 * Expansion. The value differs between the copies of one row only for
 * ROW_NUMBER, LAG, LEAD and the ROWS aggregates below. A spec with none of
 * them emits one output row per input row with diff m and never
 * materialises M rows. A spec with one
 * of them expands: a slice whose old or new expanded size exceeds 2^31 - 1
 * fails the push with "window: expanded partition exceeds 2^31 rows" before
 * anything of that size is allocated.
 *
 * Window aggregates: SUM, COUNT, MIN, MAX over a frame of E. For these
 * `off` / `width` / `nullable` describe the datum as for the value
 * functions; COUNT with width == 0 is COUNT(*), COUNT with a datum counts
 * its non-NULLs. The frame of position p:
 *   MZ_WF_FRAME_TO_CURRENT  E[0 .. last position of p's peer group] (RANGE
 *                           UNBOUNDED PRECEDING..CURRENT ROW, the SQL
 *                           default; peers included)
 *   MZ_WF_FRAME_PARTITION   E[0 .. M - 1]
 *   MZ_WF_FRAME_ROWS        E[a .. b], a = 0 | p - k | p | p + k by the start
 *                           bound, b = p - k' | p | p + k' | M - 1 by the end
 *                           bound, clipped to [0, M - 1]; empty if a > b.
 *                           `bounds` = start kind | end kind << 4 (MZ_WB_*),
 *                           `offset` = k, `end_offset` = k'. `bounds` and
 *                           `end_offset` are the bytes other functions leave
 *                           zero as `pad` and `pad2`.
 * Over the frame's non-NULL datums (all of them for COUNT(*)):
 *   SUM    NULL if there are none, else their exact sum
 *   COUNT  their number; 0 for an empty frame
 *   MIN    NULL if there are none, else the least
 *   MAX    NULL if there are none, else the greatest
 * COUNT fills an i64 slot (8 bytes) like the ranks; SUM, MIN and MAX fill
 * the 9-byte value slot, so AVG is SUM / COUNT in a downstream mz_gpu_mfp.
 * SUM accumulates exactly in 128 bits; a frame sum outside int64 fails the
 * push with "window: SUM out of int64 range" (the reference widens
 * sum(int8) to numeric). A spec holding SUM bounds every
 * multiplicity by 2^31 - 1 whether or not it expands: a larger one fails the
 * push with the expansion message below. A ROWS aggregate distinguishes the
 * copies of a row and expands, except with both ends unbounded, which is
 * the whole partition; TO_CURRENT and PARTITION aggregates do not expand.
 *
 * Restrictions vs the reference: rows are emitted
 * directly (no list + FlatMap unnest); literal LAG/LEAD offsets, defaults
 * and frame bounds; RESPECT NULLS only; integer datums and order columns.
 * Not provided: GROUPS frames; RANGE frames with offsets; MIN / MAX over a
 * ROWS frame bounded on both sides (it needs a range-minimum structure);
 * AVG (compose SUM and COUNT with mz_gpu_mfp); string_agg, array_agg.
 *
 * Refused at create (NULL, message in last_error): a varlen schema; a
 * schema outside 1..2 key words; n_funcs outside 1..MZ_GPU_MAX_WFUNCS;
 * n_order > MZ_GPU_MAX_ORDER; an order column or datum of width other than
 * 4 or 8 (COUNT(*)'s 0 excepted), or reading past in.val_bytes (the null
 * byte included); an unknown func or frame; a nonzero frame on anything but
 * LAST_VALUE and the aggregates; MZ_WF_FRAME_ROWS on anything but the
 * aggregates; for an aggregate: an unknown bound kind, a start of UNBOUNDED
 * FOLLOWING, an end of UNBOUNDED PRECEDING, a start of CURRENT ROW with an
 * end of PRECEDING, a start of FOLLOWING with an end of PRECEDING or
 * CURRENT ROW (k PRECEDING .. k' PRECEDING is legal for any k, k' and may
 * be empty), a nonzero offset on an UNBOUNDED or CURRENT ROW bound, nonzero
 * bounds or offsets without MZ_WF_FRAME_ROWS, COUNT(*) with off or
 * nullable set, has_default or dflt set, MIN / MAX with a ROWS frame of which neither end
 * is UNBOUNDED; an `out` that is not the schema derived above. A snapshot
 * with a negative net count fails the push with "negative multiplicities in
 * window" (the reference's "Non-positive accumulation in
 * ReduceInaccumulable"). After a failed push the operator may only be
 * dropped. */
enum { MZ_WF_ROW_NUMBER = 0, MZ_WF_RANK, MZ_WF_DENSE_RANK,
       MZ_WF_LAG, MZ_WF_LEAD, MZ_WF_FIRST_VALUE, MZ_WF_LAST_VALUE,
       /* 7..15 are unknown */
       MZ_WF_SUM = 16, MZ_WF_COUNT = 17, MZ_WF_MIN = 18, MZ_WF_MAX = 19 };
enum { MZ_WF_FRAME_TO_CURRENT = 0,   /* RANGE UNBOUNDED PRECEDING..CURRENT ROW
                                        (SQL default; peers included)       */
       MZ_WF_FRAME_PARTITION  = 1,   /* UNBOUNDED PRECEDING..UNBOUNDED
                                        FOLLOWING                           */
       MZ_WF_FRAME_ROWS       = 2 }; /* ROWS start..end; aggregates only   */
enum { MZ_WB_UNBOUNDED_PRECEDING = 0, MZ_WB_PRECEDING, MZ_WB_CURRENT_ROW,
       MZ_WB_FOLLOWING, MZ_WB_UNBOUNDED_FOLLOWING };
typedef struct {            /* 24 bytes */
  uint8_t  func;            /* MZ_WF_* */
  uint8_t  width;           /* datum width 4 or 8, signed LE; COUNT(*): 0 */
  uint8_t  nullable;        /* null byte at off + width */
  uint8_t  frame;           /* LAST_VALUE and aggregates; others pass 0 */
  uint16_t off;             /* datum offset in the input val */
  uint8_t  has_default;     /* LAG/LEAD: 1 = `dflt` when out of partition,
                               0 = NULL */
  union {
    uint8_t pad;
    uint8_t bounds;         /* ROWS aggregates: start kind | end kind << 4 */
  };
  uint32_t offset;          /* LAG/LEAD: literal row offset >= 0; ROWS
                               aggregates: the start bound's k */
  union {
    uint32_t pad2;
    uint32_t end_offset;    /* ROWS aggregates: the end bound's k' */
  };
  int64_t  dflt;
} mz_gpu_window_func;
#define MZ_GPU_MAX_WFUNCS 4
typedef struct {
  mz_gpu_schema in;         /* partition key words + row val bytes */
  uint32_t n_order;         /* as TopK; 0 is legal */
  mz_gpu_order_col order[MZ_GPU_MAX_ORDER];
  uint32_t n_funcs;         /* 1..MZ_GPU_MAX_WFUNCS */
  mz_gpu_window_func funcs[MZ_GPU_MAX_WFUNCS];
  mz_gpu_schema out;        /* key_words = in.key_words; val = in val ++ slots */
} mz_gpu_window_spec;
typedef struct mz_gpu_window mz_gpu_window;
mz_gpu_window *mz_gpu_window_create(mz_gpu_ctx *ctx,
                                    const mz_gpu_window_spec *spec);
int  mz_gpu_window_push(mz_gpu_ctx *ctx, mz_gpu_window *op,
                        const mz_gpu_updates *delta, mz_gpu_out **out);
void mz_gpu_window_drop(mz_gpu_ctx *ctx, mz_gpu_window *op);

/* The routing hash itself (host helper; device code uses the same). */
uint64_t mz_gpu_route_hash(const uint64_t *key_words, uint32_t n_words);

#ifdef __cplusplus
}
#endif
#endif /* MZ_GPU_H */

/*
 * otbx.h — C-ABI of the MI355X-native OpenTenBase executor offload.
 *
 * This is the drop-in boundary: the entry points a
 * CustomScan provider (include/nodes/extensible.h:117-152, driven by
 * executor/nodeCustom.c:31-125 in the reference) calls from
 * BeginCustomScan / ExecCustomScan / EndCustomScan, callable equally from a
 * standalone C harness. Plain pointers + sizes only; all device work is
 * stream-ordered on the caller's HIP stream (passed as void*); errors are
 * status codes the provider shim converts to ereport(ERROR) (the reference's
 * error convention, utils/error/elog.c).
 *
 * Replaced reference interfaces, per entry point:
 *   otbx_init/_finish      — _PG_init library load + per-GPU arbiter
 *                            (utils/fmgr/dfmgr.c:98 load path; one backend
 *                            process per DN ↔ one HIP device context)
 *   otbx_stage_*           — heap → device-resident columnar staging; stands
 *                            where heapgetpage/heapgettup_pagemode
 *                            (access/heap/heapam.c:388,920) feed the scan
 *   otbx_scan_count        — SeqScan + ExecQual + COUNT (execScan.c:140,
 *                            execExprInterp.c:324, int8inc int8.c:714)
 *   otbx_q1_partial        — the whole DN fragment of TPC-H Q1:
 *                            SeqScan → qual → project → Partial HashAgg
 *                            (nodeAgg.c:2609/856; AGGSPLIT_INITIAL_SERIAL,
 *                            include/nodes/nodes.h:964) as one CustomScan
 *                            covering the fragment subtree
 *   otbx_q3_partial        — DN fragment of TPC-H Q3: two hash joins
 *                            (nodeHash.c:1828/2174, nodeHashjoin.c:186) +
 *                            Partial HashAgg keyed on l_orderkey
 *   otbx_agg_i64 /
 *   otbx_join_i64          — the composable HashAggregate / inner HashJoin
 *                            operators for generic plan shapes (+ NULL
 *                            semantics parity: execGrouping.c:295 NULL==NULL
 *                            grouping; nodeHash.c:2026 NULL keys dropped)
 *   otbx_agg_i64_var       — HashAggregate carrying the full float8_accum
 *                            state [N,Sx,Sxx] (float.c:2823) for var_pop /
 *                            var_samp / stddev_pop / stddev_samp
 *   otbx_sort_perm         — the Sort node for any tuple shape: ExecSort
 *                            (executor/nodeSort.c:49) → tuplesort.c, with
 *                            the bounded top-N of a Limit above it
 *   otbx_window            — the WindowAgg node over that sorted input:
 *                            ExecWindowAgg (executor/nodeWindowAgg.c) with
 *                            row_number / rank / dense_rank and count / sum
 *                            over the default frame (windowfuncs.c:82-118)
 *   otbx_window_frame      — the rest of that node's PG10-era frame model:
 *                            explicit ROWS / RANGE frames (row_is_in_frame,
 *                            nodeWindowAgg.c:1472) with lag / lead / ntile
 *                            (windowfuncs.c:231-378), first / last /
 *                            nth_value (WinGetFuncArgInFrame :3368) and
 *                            count / sum / min / max over the frame
 *   otbx_group_agg         — the Agg node's sorted strategies over that
 *                            sorted input: AGG_SORTED / AGG_PLAIN
 *                            (agg_retrieve_direct, nodeAgg.c:2249) with
 *                            several count / sum / min / max per group
 *   otbx_ordered_agg       — the aggregates that sort their input inside
 *                            each group: agg(DISTINCT x)
 *                            (process_ordered_aggregate_single,
 *                            nodeAgg.c:888) and percentile_disc /
 *                            percentile_cont / mode() WITHIN GROUP
 *                            (utils/adt/orderedsetaggs.c)
 *   otbx_filter_sel       — ExecScan/ExecQual for any qual shape: a CNF of
 *                            typed, nullable comparisons (execScan.c:140,
 *                            EEOP_QUAL execExprInterp.c:919) → the ordered
 *                            selection vector the other operators gather by
 *   otbx_project           — ExecProject for one target-list expression:
 *                            typed arithmetic, casts, comparisons, Kleene
 *                            logic, CASE and COALESCE (execExprInterp.c)
 *                            over selected rows, with the reference's
 *                            first-error behaviour in a device error slot
 *   otbx_text_rank         — text as a sort, group or join key: bttextcmp
 *                            (utils/adt/varlena.c:1998) as the sort support
 *                            of a text ORDER BY, and texteq + hashing for a
 *                            text GROUP BY / join, both replaced by ordered
 *                            dictionary codes the int64 operators take
 *   merge (Coordinator)   — NOT here: the shard merge (execFragment.c:3877)
 *                            is a collective over ranks, done by the host
 *                            layer with RCCL (torch.distributed) on the
 *                            partial-state buffers these calls return.
 *
 * THREADING / STREAM CONTRACT: the library is single-threaded per process,
 * matching the reference's execution model (each DataNode backend is a
 * single-threaded process). Entry points may be called from one
 * thread at a time with one stream in flight; concurrent calls from
 * multiple threads or interleaved streams are NOT supported (several entry
 * points keep per-process cached scratch). Multiple backends on one host
 * each load their own copy (process isolation). otbx_finish releases all
 * cached scratch, so init → work → finish → init(other_device) is clean.
 *
 * Tuning/test environment variables (read at call time; all optional — the
 * GUC analog of the provider shim, guc.c):
 *   OTBX_PART_TILE=0       — select the legacy cursor-scatter partitioner
 *                            in otbx_agg_i64/otbx_join_i64 (default is the
 *                            tile-staged counting sort)
 *   OTBX_JOINP_FORCE=1     — force the partitioned join path below its
 *                            8 M-row build threshold (tests)
 *   OTBX_Q9_BITMAP_BITS=N  — cap the Q9 part-bitmap slice width (bits);
 *                            affects otbx_q9_workspace_bytes AND
 *                            otbx_q9_partial identically (default 2^30 =
 *                            single-pass for any realistic part table)
 *   OTBX_DIRECT_CAP / OTBX_Q3_FORCE_HASH / OTBX_Q3_HASH_BUDGET
 *                          — Q3 dense-direct vs hash+bloom path selection
 *                            overrides (tests force the fallback)
 *   OTBX_Q9_FILTER_WAVE=1  — legacy per-wave appender in the Q9 part filter
 *                            (default is the tile-staged compaction; A/B)
 *   OTBX_Q3_COMPACT_LEGACY=1 — legacy block-chunk Q3 group compaction
 *                            (default is the word-granular bitmap walk)
 *   OTBX_Q3_COMPACT_TILE=1 — quad-granular tile-staged compaction (A/B)
 *   OTBX_NK_FORCE_CAP=N    — force a tiny first-attempt table in the
 *                            generality-tier aggregates (tests the
 *                            estimator-overflow abort + full-cap rerun)
 *   OTBX_JOINX_VIA_INNER=1 — route 1-key left/right/full via the inner
 *                            join + mark-and-fill (measured slower than
 *                            the FSM table at all tested shapes; kept
 *                            parity-tested for future shapes). Affects
 *                            otbx_join_ext_workspace_bytes AND the route
 *                            identically (query sizing under the same env)
 *   OTBX_TEXT_STAGE=0      — otbx_text_pred reads every row straight from
 *                            global memory instead of staging a tile's
 *                            bytes in LDS; =1 stages wherever a tile's
 *                            offsets allow it. Unset: staged only for a
 *                            LIKE with a % before the pattern's last token,
 *                            the shapes where staging measured faster
 *                            (tests run both paths; A/B)
 *   OTBX_WIN_FRAME_DIRECT=N — otbx_window_frame reduces a bounded ROWS frame
 *                            of at most N positions by a per-row loop and a
 *                            wider one by segmented scans; 0 = never the
 *                            loop. Unset: the measured default (tests run
 *                            both paths on one input; A/B)
 */
#ifndef OTBX_H
#define OTBX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    OTBX_OK = 0,
    OTBX_ERR_HIP = 1,       /* HIP runtime failure (provider → ereport)   */
    OTBX_ERR_OOM = 2,
    OTBX_ERR_INVALID = 3,
    OTBX_ERR_OVERFLOW = 4,  /* numeric value out of range                 */
    OTBX_ERR_NO_GPU = 5
} otbx_status;

const char *otbx_version(void);
const char *otbx_status_str(otbx_status s);

/* Device lifecycle. otbx_init selects the HIP device (one DN backend ↔ one
 * GPU; the per-GPU arbiter of SURVEY §8b). */
otbx_status otbx_init(int device);
otbx_status otbx_finish(void);

/* Stream-ordered device allocation for standalone (non-torch) callers. */
otbx_status otbx_device_malloc(void **ptr, size_t bytes);
otbx_status otbx_device_free(void *ptr);
otbx_status otbx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);

/* ---- heap-page → SoA staging shim (host-side; the provider's
 * BeginCustomScan staging step — INTEGRATION.md §4). Walks PostgreSQL-format
 * heap pages (PageHeaderData storage/bufpage.h:157; ItemIdData
 * storage/itemid.h:25; HeapTupleHeaderData access/htup_details.h:118) and
 * deforms each LP_NORMAL tuple (heap_deform_tuple,
 * access/common/heaptuple.c:936) into caller-provided per-column host
 * arrays, ready for otbx_memcpy_h2d. Fixed-width attributes only; MVCC
 * visibility stays server-side (LP_NORMAL = post-heapgetpage state).
 * out_nulls[a] (byte-per-row, may be NULL per column) receives the NULL
 * bitmap; a NULL attribute with no out_nulls[a] is an error. */
typedef struct {
    uint16_t attlen;   /* attribute width: 1, 2, 4 or 8 bytes */
    uint16_t attalign; /* typalign in bytes: 1, 2, 4 or 8 */
} otbx_attdesc;
otbx_status otbx_stage_pages(const void *pages_host, int64_t npages,
                             size_t page_size, const otbx_attdesc *atts,
                             int32_t natts, void **out_cols_host,
                             uint8_t **out_nulls_host, int64_t cap_rows,
                             int64_t *nrows_out);
otbx_status otbx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
otbx_status otbx_stream_sync(void *stream);

/* ---- staged columnar tables (device pointers; SoA — DESIGN.md §2) ---- */

/* Layout of one packed Q1 code word (otbx_lineitem_dev.q1code; DESIGN.md
 * §7b). Five bit fields, lowest first — date_off, gid, qty, disc, tax — each
 * `*_bits` wide starting at bit `*_off`; a width of 0 means the column holds
 * one value and the field reads as 0.
 *   l_shipdate  = date_base + date_off field
 *   group slot  = gid field: ('A'→0, 'N'→1, other→2) * 2 + ('F'→0, other→1)
 *   l_quantity  = dict[code]                      as an f64 BIT PATTERN
 *   l_discount  = dict[OTBX_Q1_DICT_MAX + code]
 *   l_tax       = dict[2 * OTBX_Q1_DICT_MAX + code]
 * Each dictionary is sorted by unsigned bit pattern, so codes are
 * deterministic; +0.0 and -0.0 are two entries and NaN payloads survive.
 * sizeof == 72. */
#define OTBX_Q1_DICT_MAX 256
typedef struct {
    int32_t date_base;             /* minimum of l_shipdate */
    int32_t date_off, date_bits;
    int32_t gid_off, gid_bits;     /* gid_bits is always 3 */
    int32_t qty_off, qty_bits;
    int32_t disc_off, disc_bits;
    int32_t tax_off, tax_bits;
    int32_t nqty, ndisc, ntax;     /* dictionary sizes, 1..OTBX_Q1_DICT_MAX */
    int32_t gid_present;           /* bit g set: some row has group slot g */
    uint64_t *dict;                /* device, uint64[3 * OTBX_Q1_DICT_MAX] */
} otbx_q1code_desc;

/* Layout of one packed Q1 price word (otbx_lineitem_dev.q1pcode; DESIGN.md
 * §7c): a lossless 32-bit code of l_extendedprice for money columns, i.e.
 * f64 values within a few ulp of K * 10^-e for an integer K. Two bit fields,
 * the K field lowest (k_off == 0), each `*_bits` wide starting at bit
 * `*_off`; a width of 0 means a single value and the field reads as 0.
 *   K     = k_base + K field                      (fits a signed 32-bit int)
 *   pred  = fl((double)K * mul)                   (one rounding, no fma)
 *   delta = d_base + delta field                  (a signed ulp correction)
 *   bits(l_extendedprice) = bits(pred) + (int64)delta   (wrapping 64-bit add)
 * mul is the C literal 1.0, 0.1, 0.01, 0.001 or 0.0001 for scale_exp
 * 0..4. k_base + K field and d_base + delta field never leave int32.
 * sizeof == 40. */
typedef struct {
    int32_t scale_exp;             /* e: K = llrint(x * 10^e), 0..4 */
    double mul;                    /* the literal 10^-e */
    int32_t k_base, k_off, k_bits;
    int32_t d_base, d_off, d_bits; /* d_bits <= 8 */
} otbx_q1price_desc;

typedef struct {
    int64_t n;
    int64_t *l_orderkey;      /* may be NULL if not staged (Q1 needs none) */
    double  *l_quantity, *l_extendedprice, *l_discount, *l_tax;
    uint8_t *l_returnflag, *l_linestatus;
    int32_t *l_shipdate;
    int64_t *l_partkey;       /* appended; may be NULL (Q9-mix only) */
    /* optional Q9 probe-side record cache {l_orderkey i64, l_extendedprice
     * f64, l_discount f64, pad} (32 B/row), built ONCE at staging
     * (otbx_build_q9recs — a derived layout like the zone-map metadata):
     * the Q9 probe's per-survivor gather then touches one cache line
     * instead of three column lines. NULL = probe gathers the columns. */
    void *q9rec;
    /* optional compact-key cache (otbx_build_key32, built once at staging):
     * int32 copy of l_orderkey, valid iff every key fits [0, 2^31) — at
     * TPC-H scales orderkeys do (SF100: max 6e8). Halves the probe's key
     * stream. NULL = kernels read the i64 column. */
    int32_t *l_orderkey32;
    int32_t *l_partkey32;     /* same compact-key cache for l_partkey
                               * (halves the Q9 filter's key stream) */
    /* optional packed Q1 code column (otbx_build_q1codes, built once at
     * staging): one 32-bit word per row holding the shipdate offset, the Q1
     * group slot and dictionary codes of l_quantity / l_discount / l_tax,
     * laid out as q1desc says. Q1 then streams this word plus
     * l_extendedprice, 12 B/row instead of 38. NULL = Q1 reads the raw
     * columns. q1desc is meaningful only while q1code is non-NULL. */
    uint32_t *q1code;
    otbx_q1code_desc q1desc;
    /* optional packed Q1 price column (otbx_build_q1pcodes, built once at
     * staging after q1code): one 32-bit word per row from which
     * l_extendedprice is rebuilt bit for bit, laid out as q1pdesc says. Q1
     * then streams q1code + q1pcode, 8 B/row instead of 12. NULL = Q1 reads
     * l_extendedprice. Only used together with q1code; q1pdesc is meaningful
     * only while q1pcode is non-NULL. */
    uint32_t *q1pcode;
    otbx_q1price_desc q1pdesc;
} otbx_lineitem_dev;

typedef struct {
    int64_t n;
    int64_t *o_orderkey, *o_custkey;
    int32_t *o_orderdate, *o_shippriority;
    /* staged-table metadata (zone-map style, computed once at staging —
     * otbx_gen_orders_dev fills it; a provider computes it while walking
     * pages). has_minmax = 0 → executors run their own minmax kernel. */
    int64_t okey_min, okey_max;
    int32_t has_minmax;
    /* optional compact-key caches (otbx_build_key32; see lineitem note) */
    int32_t *o_orderkey32, *o_custkey32;
} otbx_orders_dev;

typedef struct {
    int64_t n;
    int64_t *c_custkey;
    uint8_t *c_mktsegment;
} otbx_customer_dev;

typedef struct {
    int64_t n;
    int64_t *p_partkey;
    uint8_t *p_type;
} otbx_part_dev;

/* On-device synthetic generation (the dbgen analog; same counter-based
 * functions as the CPU oracle — oracle/otbx_gen.h — so tables are
 * bit-identical on both sides). Caller provides the device buffers
 * (column pointers in the struct, each sized for n_global/nranks rows). */
/* build an int32 compact-key cache from an i64 key column: writes
 * saturated casts into dst32_dev and *ok_host = 1 if every value fit
 * [0, 2^31), else 0 (caller must then leave the cache pointer NULL).
 * Synchronous (staging-time only). */
otbx_status otbx_build_key32(const int64_t *src_dev, int64_t n,
                             int32_t *dst32_dev, int32_t *ok_host,
                             void *stream);
/* Plan the packed Q1 code word. Pure host code (no HIP call). Inputs: the
 * three dictionary sizes and date_span = max(l_shipdate) - min(l_shipdate).
 * A field's width is ceil(log2(size)) (size 1 → 0 bits), the date field has
 * as many bits as date_span, gid always 3. *fits_host = 1 and the offsets /
 * widths / sizes of *desc are filled (date_base, gid_present and dict are
 * left alone) when every size is in 1..OTBX_Q1_DICT_MAX, date_span < 2^32
 * and the widths sum to at most 32; otherwise *fits_host = 0 and *desc is
 * untouched.
 * OTBX_ERR_INVALID only for NULL pointers. */
otbx_status otbx_q1code_plan(int32_t nqty, int32_t ndisc, int32_t ntax,
                             uint64_t date_span, otbx_q1code_desc *desc,
                             int32_t *fits_host);
/* Build the packed Q1 code column of a staged lineitem table. Collects the
 * distinct bit patterns of l_quantity / l_discount / l_tax and the shipdate
 * range on the device, plans the word with otbx_q1code_plan, writes the
 * sorted dictionaries to dict_dev (uint64[3 * OTBX_Q1_DICT_MAX]) and one
 * word per row to codes_dev (uint32[t->n]); the encode pass decodes every
 * word it wrote and compares it bit-for-bit with the source row.
 * *ok_host = 1 and *desc_host filled (dict = dict_dev) on success; the
 * caller then sets t->q1code / t->q1desc. *ok_host = 0 (caller leaves
 * q1code NULL, Q1 keeps reading the raw columns) when the data does not
 * fit: more than OTBX_Q1_DICT_MAX distinct patterns in a column, a column
 * holding the all-ones pattern (the set's empty marker), widths above 32
 * bits, a failed round trip, t->n == 0 or any Q1 column not staged.
 * Synchronous (staging-time only), like otbx_build_key32. */
otbx_status otbx_build_q1codes(const otbx_lineitem_dev *t,
                               uint32_t *codes_dev, uint64_t *dict_dev,
                               otbx_q1code_desc *desc_host, int32_t *ok_host,
                               void *stream);
/* Plan the packed Q1 price word. Pure host code (no HIP call). Inputs, one
 * entry per candidate exponent e = 0..4 (scale 10^e): bad[e] != 0 when some
 * x * 10^e was not finite or K = llrint(x * 10^e) left int32; otherwise the
 * column's min/max of K and of delta = bits(x) - bits(fl((double)K * 10^-e)).
 * k_bits = bits(kmax - kmin), d_bits = bits(dmax - dmin), both differences
 * formed in 64 bit. A candidate fits when it is not bad, d_bits <= 8,
 * k_bits + d_bits <= 32 and dmin, dmax lie in int32 (d_base is one). The
 * fitting candidate with the fewest total bits wins, ties go to the smaller
 * e. *fits_host = 1 and *desc filled (K field at offset 0, delta field above
 * it) when one fits; otherwise *fits_host = 0 and *desc is untouched.
 * OTBX_ERR_INVALID only for NULL pointers. */
otbx_status otbx_q1price_plan(const int32_t *bad, const int64_t *kmin,
                              const int64_t *kmax, const int64_t *dmin,
                              const int64_t *dmax, otbx_q1price_desc *desc,
                              int32_t *fits_host);
/* Build the packed Q1 price column of a staged lineitem table. One pass
 * over l_extendedprice collects the five candidates' statistics on the
 * device, otbx_q1price_plan picks the layout, a second pass writes one word
 * per row to pcodes_dev (uint32[t->n]), decodes the word it wrote with the
 * Q1 kernel's own decode and compares it bit for bit with the source double.
 * *ok_host = 1 and *desc_host filled on success; the caller then sets
 * t->q1pcode / t->q1pdesc. *ok_host = 0 (caller leaves q1pcode NULL, Q1
 * keeps streaming l_extendedprice) when t->q1code is NULL, t->n == 0,
 * l_extendedprice is not staged, no candidate fits (NaN, +-Inf, -0.0 among
 * positive values, doubles without decimal structure) or the round trip
 * failed. Synchronous (staging-time only), like otbx_build_q1codes. */
otbx_status otbx_build_q1pcodes(const otbx_lineitem_dev *t,
                                uint32_t *pcodes_dev,
                                otbx_q1price_desc *desc_host,
                                int32_t *ok_host, void *stream);
/* build the q9rec cache from the staged columns (32 B/row into recs_dev) */
otbx_status otbx_build_q9recs(const otbx_lineitem_dev *l, void *recs_dev,
                              void *stream);
otbx_status otbx_gen_lineitem_dev(const otbx_lineitem_dev *t, uint64_t seed,
                                  int64_t n_global, uint32_t rank,
                                  uint32_t nranks, void *stream);
otbx_status otbx_gen_orders_dev(otbx_orders_dev *t, uint64_t seed,
                                int64_t n_global, int64_t ncust_global,
                                uint32_t rank, uint32_t nranks, int skew,
                                void *stream);
otbx_status otbx_gen_customer_dev(const otbx_customer_dev *t, uint64_t seed,
                                  int64_t n_global, uint32_t rank,
                                  uint32_t nranks, void *stream);
/* part is a replicated dimension table: every rank holds all n_global rows */
otbx_status otbx_gen_part_dev(const otbx_part_dev *t, uint64_t seed,
                              int64_t n_global, void *stream);

/* ---- config 2: SeqScan + qual + COUNT(*) (scan-bandwidth kernel) ----
 * count_dev: one int64 device slot (zeroed by the call). */
otbx_status otbx_scan_count(const int32_t *shipdate_dev, int64_t n,
                            int32_t cutoff, int64_t *count_dev, void *stream);

/* ---- TPC-H Q1 DN fragment ----
 * Partial-aggregate state per (l_returnflag,l_linestatus) group, dense over
 * the 6 possible combos, fixed slot order (A,F)(A,O)(N,F)(N,O)(R,F)(R,O):
 *   sums_dev:   double[6][5] = {sum_qty, sum_base_price, sum_disc_price,
 *                               sum_charge, sum_disc}
 *   counts_dev: int64[6]     = count(*)
 * Both zeroed by the call; the Coordinator-side merge all-gathers exactly
 * these buffers. kernel_ms (host, may be NULL): HIP-event time of the fused
 * kernel on `stream` (the bench's roofline numerator — DESIGN.md §4). */
otbx_status otbx_q1_partial(const otbx_lineitem_dev *t, int32_t cutoff_day,
                            double *sums_dev, int64_t *counts_dev,
                            void *stream, float *kernel_ms);
/* A/B harness entry: variant 0 = 2 rows/lane, 1 = 4 rows/lane,
 * 2 = 4 rows/lane + non-temporal loads (all three read the raw columns,
 * 38 B/row); 3 = the packed code column + l_extendedprice, 12 B/row, 4
 * rows/lane; 4 = as 3 with 8 rows/lane; 5 = as 3, accumulating only the
 * group slots in q1desc.gid_present; 6 = as 5 with the price decoded from
 * the packed price column q1pcode instead of l_extendedprice, 8 B/row;
 * 7 = as 6 with 8 rows/lane. Variants 3 to 7 need t->q1code, 6 and 7 also
 * t->q1pcode and a valid q1pdesc; they return OTBX_ERR_INVALID without
 * launching anything otherwise, as does any variant above 7.
 * otbx_q1_partial dispatches variant 7 when t->q1pcode is set, else 5 when
 * t->q1code is set, else 2. */
otbx_status otbx_q1_partial_variant(const otbx_lineitem_dev *t,
                                    int32_t cutoff_day, double *sums_dev,
                                    int64_t *counts_dev, void *stream,
                                    float *kernel_ms, int variant);

/* ---- TPC-H Q3 DN fragment ----
 * customer/orders/lineitem staged on-device; custkeys of the replicated
 * (broadcast) customer build side are read from cust_keys_dev when non-NULL
 * (ncust_keys rows; the post-all-gather buffer), else from c->... filtered
 * by segment locally.
 * Outputs (device, caller-allocated):
 *   groups_dev:  capacity cap_groups entries of otbx_q3_group
 *   ngroups_dev: int64[1] — compacted group count
 * ws_dev: workspace (hash tables), size from otbx_q3_workspace_bytes.
 *
 * Input domain. Every int32 date and priority is an ordinary value: day 0,
 * negative days and any o_shippriority, INT32_MIN and -1 included. Prices
 * and discounts are any finite doubles; a group exists as soon as one
 * lineitem matched, whatever its revenue sums to (zero and negative sums
 * included). Keys (c_custkey, o_custkey, o_orderkey, l_orderkey, the
 * cust_keys_dev entries) are any int64 EXCEPT INT64_MIN, the one reserved
 * key: the hash-path tables keep it as their empty marker, so a build row
 * carrying it is not inserted and a probe row carrying it matches nothing.
 * Key 0 and negative keys are ordinary keys (a column holding a negative
 * key takes the hash path: the key-range kernels compare unsigned).
 * c_custkey may repeat (the customer side is a key SET); o_orderkey must be
 * unique. okey_min/okey_max, when has_minmax is set, must be the exact
 * signed bounds of o_orderkey. */
typedef struct {
    int64_t l_orderkey;
    double revenue;
    int32_t o_orderdate, o_shippriority;
} otbx_q3_group;

otbx_status otbx_q3_workspace_bytes(int64_t ncust, int64_t norders,
                                    int64_t nlineitem, size_t *bytes);
/* kernel_ms (host, may be NULL): float[4] = {customer-keyset build,
 * orders build+probe, lineitem probe+partial-agg, compact} HIP-event times.
 * stats_dev (may be NULL): int64[1] = probe hits (lineitem rows passing the
 * date qual AND matching an order — the N_probe_hits of the §8d roofline
 * formula); zeroed by the call. */
otbx_status otbx_q3_partial(const otbx_customer_dev *c,
                            const otbx_orders_dev *o,
                            const otbx_lineitem_dev *l,
                            const int64_t *cust_keys_dev, int64_t ncust_keys,
                            uint8_t segment, int32_t q3date,
                            void *ws_dev, size_t ws_bytes,
                            otbx_q3_group *groups_dev, int64_t cap_groups,
                            int64_t *ngroups_dev, int64_t *stats_dev,
                            void *stream, float *kernel_ms);

/* top-k selection over compacted Q3 groups (ORDER BY revenue DESC …
 * LIMIT k pre-selection; the final k-way ordering happens host-side on the
 * ≤ cap_cand candidates). hist_dev: uint32[16384] workspace (zeroed by the
 * call). ncand_dev ≥ k unless n < k; candidates are all groups with revenue
 * ≥ the selection threshold (a bin boundary of the order-preserving bit
 * normalisation, so any finite revenue ranks correctly: negative, zero and
 * -0.0 == +0.0 included). *ncand_dev receives the TRUE candidate count even
 * when it exceeds cap_cand; at most cap_cand entries of cand_dev are
 * written, and the caller retries with a larger buffer. */
otbx_status otbx_topk_by_revenue(const otbx_q3_group *groups_dev, int64_t n,
                                 int64_t k, otbx_q3_group *cand_dev,
                                 int64_t cap_cand, int64_t *ncand_dev,
                                 uint32_t *hist_dev, void *stream);
/* helper for the broadcast build side: compact custkeys where
 * c_mktsegment == segment into keys_out_dev, count into nkeys_dev (zeroed). */
otbx_status otbx_filter_customer(const otbx_customer_dev *c, uint8_t segment,
                                 int64_t *keys_out_dev, int64_t *nkeys_dev,
                                 void *stream);

/* ---- Q9-mix DN fragment (BASELINE config 5's second query shape) ----
 * lineitem ⋈ part (p_type % typemod == typeval) ⋈ orders, partial aggregate
 * GROUP BY year(o_orderdate) — two joins under an aggregate on a COMPUTED
 * key. Dense outputs over the 7 order years (0 = 1992):
 *   sums_dev: double[7] revenue, counts_dev: int64[7]; both zeroed by the
 * call; the Coordinator merge all-gathers them like Q1's states.
 * ws: otbx_q9_workspace_bytes(nparts, norders_local, nranks).
 *
 * Input domain. p_partkey is a permutation of 1..p->n (any row order): the
 * part filter is a bitmap indexed by p_partkey - 1, and l_partkey values
 * outside [1, p->n] match nothing. o_orderkey is unique, ≥ 0, and dense
 * enough that max - min + 1 ≤ norders * nranks; a wider range does not fit
 * the workspace and is refused with OTBX_ERR_INVALID before any kernel
 * runs. okey_min/okey_max, when has_minmax is set, must be exact.
 * o_orderdate lies in [0, 2557] (the 7 calendar years of otbx_year_of_day),
 * day 0 included; OTBX_Q9_DATE_ABSENT is the one int32 the date lookup table
 * reserves for "no such order" (dates are stored XOR this value, so that a
 * zeroed entry decodes to it). An empty lineitem (n == 0) may carry NULL
 * columns. */
#define OTBX_Q9_DATE_ABSENT ((int32_t)0x80808080u)
otbx_status otbx_q9_workspace_bytes(int64_t nparts, int64_t norders,
                                    int64_t nlineitem, uint32_t nranks,
                                    size_t *bytes);
otbx_status otbx_q9_partial(const otbx_part_dev *p, const otbx_orders_dev *o,
                            const otbx_lineitem_dev *l, uint8_t typemod,
                            uint8_t typeval, void *ws, size_t ws_bytes,
                            double *sums_dev, int64_t *counts_dev,
                            void *stream, float *kernel_ms);

/* ---- composable operators (generic plan shapes + NULL-semantics parity) --

 * Hash aggregate: group by nullable i64 key, aggregate nullable f64 value;
 * count(*), count(v), sum(v), avg-N/Sx. Output: open-addressing table
 * compacted to groups_dev (cap = n). Null bitmaps are byte-per-row (1 =
 * NULL), may be NULL pointers. */
typedef struct {
    int64_t key;
    int64_t count_star;
    int64_t count_v;
    double sum_v;
    int32_t key_isnull;
    int32_t sum_isnull;
} otbx_agg_group;

otbx_status otbx_agg_i64_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_agg_i64(const int64_t *keys_dev, const uint8_t *key_null_dev,
                         const double *vals_dev, const uint8_t *val_null_dev,
                         int64_t n, void *ws_dev, size_t ws_bytes,
                         otbx_agg_group *groups_dev, int64_t *ngroups_dev,
                         void *stream);

/* Variance/stddev aggregate: the full float8_accum transition state
 * [N, Sx, Sxx] (utils/adt/float.c:2823) per group, feeding var_pop /
 * var_samp / stddev_pop / stddev_samp (float.c:3011-3096; finalizers in the
 * host layer). Grouping contract identical to otbx_agg_i64: NULL keys form
 * one group, the INT64_MIN-valued key is supported, NULL values are skipped
 * by count_v/sum_v/sxx and counted by count_star, n == 0 gives zero groups,
 * emission order is arbitrary, groups_dev capacity = n.
 * Numerics: sxx is NOT sum(x^2) - Sx^2/N (that form cancels
 * catastrophically once |mean| >> stddev). The call runs otbx_agg_i64 for
 * N and Sx, then a second pass accumulates d = x - Sx/N per row and emits
 * sxx = sum(d^2) - sum(d)^2/N, which stays within the float8 parity bar of
 * the reference's Youngs-Cramer recurrence.
 *   count_v == 1            -> sxx == 0
 *   group holds Inf or NaN  -> sxx == NaN
 *   otherwise sxx >= 0 (a negative rounding residue is clamped to 0).
 * Overflow of FINITE inputs is not detected (the reference raises "value
 * out of range: overflow"): like otbx_agg_i64 the call has no device-to-host
 * error channel; an overflowed Sx or Sxx reads back as Inf / NaN. */
typedef struct {
    int64_t key;
    int64_t count_star;
    int64_t count_v;     /* = N of the float8_accum state */
    double  sum_v;       /* = Sx */
    double  sxx;         /* = Sxx = sum((x - mean)^2), >= 0 or NaN */
    int32_t key_isnull;
    int32_t sum_isnull;  /* count_v == 0: the whole state is SQL NULL */
} otbx_var_group;        /* 48 B */

otbx_status otbx_agg_i64_var_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_agg_i64_var(const int64_t *keys_dev, const uint8_t *key_null_dev,
                             const double *vals_dev, const uint8_t *val_null_dev,
                             int64_t n, void *ws_dev, size_t ws_bytes,
                             otbx_var_group *groups_dev, int64_t *ngroups_dev,
                             void *stream);

/* ---- extended join types + two-key variants ----
 * The HJ_* fill-state FSM (executor/nodeHashjoin.c:139-144) on the generic
 * join, and multi-key (2 x i64) variants of join and group-by.
 * join_type: 0 inner, 1 left, 2 semi, 3 anti, 4 right, 5 full.
 * Pair encoding in (out_bidx, out_pidx):
 *   match                          -> (bidx, pidx)
 *   left/full unmatched probe row  -> (-1, pidx)  [HJ_FILL_OUTER_TUPLE,
 *     incl. NULL-key probe rows]      nodeHashjoin.c:142,668]
 *   right/full unmatched build row -> (bidx, -1)  [HJ_FILL_INNER_TUPLES,
 *     incl. NULL-key build rows]      nodeHashjoin.c:143,693;
 *                                     ExecScanHashTableForUnmatched
 *                                     nodeHash.c:2322]
 *   semi: (-1, pidx) once per probe row with >= 1 match (JOIN_SEMI
 *     advances after the first match, nodeHashjoin.c:572)
 *   anti: (-1, pidx) per probe row with no match (nodeHashjoin.c:631)
 * Two-key variants join/group on the ROW (k1,k2): a row with EITHER key
 * NULL never matches (strict equality; multi-key hash combine =
 * rotate-left-1 xor, nodeHash.c:2059, restated at 64 bit — parity is on
 * result sets). Overflow contract identical to otbx_join_i64.
 * nb == 0 and np == 0 are valid: an empty side may pass NULL columns, it
 * matches nothing, and the other side's rows are emitted as fills where the
 * join type fills them. OTBX_ERR_INVALID: join_type out of range, ws_dev or
 * npairs_dev NULL, ws_bytes below otbx_join_ext_workspace_bytes(nb, np),
 * otbx_join_i64x2 with a NULL second key column on a side that has rows. */
otbx_status otbx_join_ext_workspace_bytes(int64_t nb, int64_t np,
                                          size_t *bytes);
otbx_status otbx_join_i64_ext(const int64_t *bkeys_dev,
                              const uint8_t *bnull_dev, int64_t nb,
                              const int64_t *pkeys_dev,
                              const uint8_t *pnull_dev, int64_t np,
                              int32_t join_type, void *ws_dev,
                              size_t ws_bytes, int64_t *out_bidx_dev,
                              int64_t *out_pidx_dev, int64_t cap_pairs,
                              int64_t *npairs_dev, void *stream);
otbx_status otbx_join_i64x2(const int64_t *bk1_dev, const uint8_t *bn1_dev,
                            const int64_t *bk2_dev, const uint8_t *bn2_dev,
                            int64_t nb, const int64_t *pk1_dev,
                            const uint8_t *pn1_dev, const int64_t *pk2_dev,
                            const uint8_t *pn2_dev, int64_t np,
                            int32_t join_type, void *ws_dev, size_t ws_bytes,
                            int64_t *out_bidx_dev, int64_t *out_pidx_dev,
                            int64_t cap_pairs, int64_t *npairs_dev,
                            void *stream);

/* two-key hash aggregate: group by (nullable k1, nullable k2) with
 * NULL==NULL grouping (execGrouping.c:295,:525); aggregates as
 * otbx_agg_i64. groups_dev capacity = n rows; *ngroups_dev receives the
 * group count; emission order is arbitrary (hash-table order, as the
 * reference's simplehash iteration). n == 0 gives zero groups and may pass
 * NULL columns; a NULL key column with n > 0 is OTBX_ERR_INVALID. */
typedef struct {
    int64_t key1;
    int64_t key2;
    int64_t count_star;
    int64_t count_v;
    double sum_v;
    int32_t key1_isnull;
    int32_t key2_isnull;
    int32_t sum_isnull;
    int32_t _pad;
} otbx_agg2_group; /* 56 B */

otbx_status otbx_agg_i64x2_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_agg_i64x2(const int64_t *k1_dev, const uint8_t *k1null_dev,
                           const int64_t *k2_dev, const uint8_t *k2null_dev,
                           const double *vals_dev,
                           const uint8_t *val_null_dev, int64_t n,
                           void *ws_dev, size_t ws_bytes,
                           otbx_agg2_group *groups_dev, int64_t *ngroups_dev,
                           void *stream);

/* ---- N-key (1..8 columns) group-by and join ----
 * Group/join identity is the ROW of key columns: NULL==NULL for grouping
 * (execGrouping.c:295,:525), any-NULL-never-matches for joins
 * (nodeHash.c:2026); hash = iterated rotate-left-1 xor over per-column
 * hashes (nodeHash.c:2059). Groups carry the DEFINING ROW INDEX instead of
 * N key values — the reference's hash table stores the representative
 * tuple the same way (execGrouping.c firstTuple); the caller reads the key
 * values back through the index. Joins emit (bidx, pidx) pairs exactly as
 * otbx_join_i64_ext (same join_type codes, fills and overflow contract).
 * otbx_agg_i64n with n == 0 gives zero groups; otbx_join_i64n with nb == 0
 * or np == 0 treats that side as empty. The columns of an empty input may be
 * NULL; nkeys must still be 1..OTBX_MAX_KEYS and equal on both join sides.
 * A NULL key (or, for the aggregate, value) column with a row count > 0 is
 * OTBX_ERR_INVALID. */
#define OTBX_MAX_KEYS 8
typedef struct {
    int32_t nkeys;                           /* 1..OTBX_MAX_KEYS */
    const int64_t *keys[OTBX_MAX_KEYS];      /* device pointers */
    const uint8_t *nulls[OTBX_MAX_KEYS];     /* per column; may be NULL */
} otbx_keyset;

typedef struct {
    int64_t row_idx;          /* defining row (representative tuple) */
    int64_t count_star;
    int64_t count_v;
    double sum_v;
    int32_t sum_isnull;
    int32_t _pad;
} otbx_aggn_group; /* 40 B */

otbx_status otbx_agg_i64n_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_agg_i64n(const otbx_keyset *ks, const double *vals_dev,
                          const uint8_t *val_null_dev, int64_t n,
                          void *ws_dev, size_t ws_bytes,
                          otbx_aggn_group *groups_dev, int64_t *ngroups_dev,
                          void *stream);

otbx_status otbx_join_i64n_workspace_bytes(int64_t nb, int64_t np,
                                           size_t *bytes);
otbx_status otbx_join_i64n(const otbx_keyset *bks, int64_t nb,
                           const otbx_keyset *pks, int64_t np,
                           int32_t join_type, void *ws_dev, size_t ws_bytes,
                           int64_t *out_bidx_dev, int64_t *out_pidx_dev,
                           int64_t cap_pairs, int64_t *npairs_dev,
                           void *stream);

/* ---- exact decimal (scaled-int64) aggregate with int128 sum ----
 * The reference's HAVE_INT128 numeric aggregation: group state =
 * Int128AggState {N, sumX} (utils/adt/numeric.c:5072; do_int128_accum
 * :4998; transition int8_avg_accum :5365; sum(bigint) promotes to numeric
 * and cannot overflow, int8_sum :6206). Values are scaled-decimal int64
 * (e.g. NUMERIC(15,2) money in cents); the emitted two's-complement
 * 128-bit sum is EXACT, so parity with the reference is bit-exact —
 * no float tolerance. groups_dev capacity = n. n == 0 gives zero groups and
 * may pass NULL columns; NULL keys_dev or vals_dev with n > 0 is
 * OTBX_ERR_INVALID. */
typedef struct {
    int64_t key;
    int64_t count_star;
    int64_t count_v;
    int64_t sum_hi;          /* int128 two's-complement high word */
    uint64_t sum_lo;
    int32_t key_isnull;
    int32_t sum_isnull;
} otbx_dec_group; /* 48 B */

otbx_status otbx_agg_i64_dec_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_agg_i64_dec(const int64_t *keys_dev,
                             const uint8_t *key_null_dev,
                             const int64_t *vals_dev,
                             const uint8_t *val_null_dev, int64_t n,
                             void *ws_dev, size_t ws_bytes,
                             otbx_dec_group *groups_dev,
                             int64_t *ngroups_dev, void *stream);

/* ---- GPU ORDER BY ----
 * Full sort of Q3 group rows by (revenue DESC, o_orderdate ASC) — the
 * tuplesort.c analog for the no-LIMIT ORDER BY case (LIMIT queries use
 * otbx_topk_by_revenue). Stable LSD radix sort; out_dev must not alias
 * groups_dev. Preconditions: 0 ≤ o_orderdate < 2^16 (the date key is sorted
 * in two 8-bit passes); revenue any non-NaN double (-0.0 ties with +0.0). */
otbx_status otbx_order_groups_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_order_groups(const otbx_q3_group *groups_dev, int64_t n,
                              otbx_q3_group *out_dev, void *ws,
                              size_t ws_bytes, void *stream);

/* ---- generic GPU Sort: multi-column ORDER BY [LIMIT k] ----
 * The ExecSort → tuplesort analog (executor/nodeSort.c:49,
 * utils/sort/tuplesort.c; bounded top-N of tuplesort_set_bound :1471) for
 * any tuple shape: up to OTBX_MAX_KEYS key columns of type int64, float64,
 * int32 or uint8, each with its own direction, NULL placement and optional
 * null mask. The result is a PERMUTATION: perm_dev[j] is the input row
 * index of the j-th output row, int64 so it feeds otbx_gather_* unchanged.
 *
 * limit == 0: full sort; capacity of perm_dev and *nout_dev are n.
 * limit  > 0: LIMIT k; capacity and *nout_dev are min(limit, n), and the
 *             result equals the first `limit` entries of the full sort.
 * limit  < 0: invalid.
 *
 * ORDERING CONTRACT (ApplySortComparator, include/utils/sortsupport.h:201):
 *   - key[0] is the primary key; key[i+1] breaks ties of key[0..i].
 *   - Per key, two NULLs compare equal. A NULL sorts before every non-NULL
 *     iff OTBX_SORT_NULLS_FIRST is set — independently of OTBX_SORT_DESC,
 *     which (as ssup_reverse) only negates the comparison of two non-NULLs.
 *   - I64, I32, U8: ordinary signed / signed / unsigned order (btint8cmp,
 *     nbtcompare.c:129).
 *   - F64: float8_cmp_internal (utils/adt/float.c:1172): every NaN equals
 *     every other NaN — whatever its sign bit or payload — and is greater
 *     than every non-NaN, +Inf included; -0.0 == +0.0.
 *   - The value stored under a NULL is ignored entirely.
 *   - The sort is STABLE: rows that compare equal on all keys keep input
 *     order (the reference's qsort promises less; stability makes the
 *     permutation unique, so parity is bit-exact).
 *
 * Stream-ordered, no host synchronisation and no device-to-host channel
 * (like otbx_order_groups). Checked before any HIP call, each returning
 * OTBX_ERR_INVALID: nkeys outside 1..8, a type code outside 0..3, flags
 * outside bits 0-1, n < 0, n > INT32_MAX (row indices are 32-bit
 * internally), limit < 0, a NULL col with n > 0, ws_bytes below
 * otbx_sort_workspace_bytes(n, nkeys, limit). n == 0 is valid and writes
 * *nout_dev = 0. otbx_sort_workspace_bytes is pure host code, monotone in
 * n and in nkeys. */
enum { OTBX_SORT_I64 = 0, OTBX_SORT_F64 = 1, OTBX_SORT_I32 = 2, OTBX_SORT_U8 = 3 };
#define OTBX_SORT_DESC        1
#define OTBX_SORT_NULLS_FIRST 2
typedef struct {
    const void    *col;     /* device column of `type`                      */
    const uint8_t *nulls;   /* byte per row, nonzero = NULL; may be NULL    */
    int32_t        type;    /* OTBX_SORT_*                                  */
    int32_t        flags;   /* OTBX_SORT_DESC | OTBX_SORT_NULLS_FIRST       */
} otbx_sortkey;
typedef struct { int32_t nkeys; otbx_sortkey key[OTBX_MAX_KEYS]; } otbx_sortspec;

otbx_status otbx_sort_workspace_bytes(int64_t n, int32_t nkeys, int64_t limit,
                                      size_t *bytes);
otbx_status otbx_sort_perm(const otbx_sortspec *spec, int64_t n, int64_t limit,
                           void *ws_dev, size_t ws_bytes,
                           int64_t *perm_dev, int64_t *nout_dev, void *stream);

/* ---- GPU WindowAgg: ranking and running aggregates over sorted input ----
 * The ExecWindowAgg analog (executor/nodeWindowAgg.c; window functions in
 * utils/adt/windowfuncs.c) for ONE window specification
 *     OVER (PARTITION BY key[0..npart) ORDER BY key[npart..nkeys))
 * with the reference's default frame. It is the pass over the permutation
 * otbx_sort_perm produced for exactly these keys.
 *
 * INPUTS
 *   - spec lists the key columns the input is sorted by: the first npart
 *     keys are the PARTITION BY columns, the rest the ORDER BY columns.
 *     spec->nkeys may be 0..8 and 0 <= npart <= nkeys. With nkeys == 0 all
 *     rows form one partition of peers.
 *   - perm_dev is what otbx_sort_perm(spec, n, limit = 0) returned: row
 *     perm[j] is the j-th row in sorted order. NULL means identity (the
 *     columns are already in order). The caller guarantees it is a sorted
 *     permutation of [0, n); this is not checked (an entry outside [0, n) is
 *     clamped, so it cannot address outside the columns).
 *   - vals_dev / val_null_dev (byte per row, nonzero = NULL; may be NULL)
 *     are indexed by INPUT row and read through perm.
 *   - every output is indexed by SORTED POSITION j — WindowAgg emits rows in
 *     sorted order. Each out-> pointer is a device array of n entries, or
 *     NULL = not wanted: nothing is loaded or stored for it, and a call that
 *     asks for ranking outputs only never touches vals_dev.
 *
 * EQUALITY (are_peers, nodeWindowAgg.c:2960, over ApplySortComparator)
 *   Two adjacent rows are in the same partition iff they compare EQUAL on
 *   every partition key, and are peers iff they are also equal on every
 *   order key. Equal means what otbx_sort_perm means — NULL equals NULL,
 *   every NaN equals every NaN, -0.0 == +0.0, the value stored under a NULL
 *   is ignored — because the test is made on the sort's own normalised key
 *   (null bit + normalised bits).
 *
 * FRAME: RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW (row_is_in_frame,
 *   nodeWindowAgg.c:1472-1505): from the partition's first row through the
 *   LAST PEER of the current row. All peers therefore receive identical
 *   count_star / count_v / sum_v / sum_isnull, and with npart == nkeys the
 *   whole partition is the frame.
 *
 * OUTPUTS
 *   row_number = j - partition_start + 1          (window_row_number :82)
 *   rank       = peer_group_start - partition_start + 1  (window_rank :98)
 *   dense_rank = peer groups up to and including the current one    (:118)
 *   part_rows  = rows in the partition (WinGetPartitionRowCount)
 *   count_star = rows in the frame; count_v = its non-NULL values
 *   sum_v      = their float8pl sum; NULL (sum_isnull = 1, value 0.0) when
 *                the frame holds no non-NULL value.
 *
 * NUMERICS OF sum_v: the scan is SEGMENTED — a partition's sums are computed
 *   from that partition's values only, so an Inf, NaN or 1e300 in one
 *   partition never reaches another, and nothing is obtained as a
 *   difference of prefix sums. Inside a partition the association order
 *   differs from the reference's left-to-right float8pl (tiled tree); the
 *   result is within the standard recursive-summation bound
 *   m*u*sum|x| / (1 - m*u), u = 2^-53, and exact wherever every order is
 *   (integer-valued doubles). Overflow of finite inputs is not detected
 *   (same clause as otbx_agg_i64_var).
 *
 * Stream-ordered, no host synchronisation and no device-to-host channel.
 * Checked before any HIP call, each returning OTBX_ERR_INVALID: spec or out
 * NULL; nkeys outside 0..8; npart outside 0..nkeys; a type code outside
 * 0..3 or flags outside bits 0-1; n < 0 or n > INT32_MAX; a NULL key column
 * with n > 0; no output requested; sum_v without sum_isnull or the reverse;
 * sum_v or count_v requested with vals_dev == NULL; ws_bytes below
 * otbx_window_workspace_bytes(n), or ws_dev not 16-byte aligned. n == 0 is
 * valid and writes nothing.
 * otbx_window_workspace_bytes is pure host code and monotone in n. Nothing
 * is cached by this entry point (otbx_finish has nothing to release). */
typedef struct {            /* each pointer: device array of n entries, or NULL = not wanted */
    int64_t *row_number;    /* window_row_number, windowfuncs.c:82  */
    int64_t *rank;          /* window_rank        :98               */
    int64_t *dense_rank;    /* window_dense_rank  :118              */
    int64_t *count_star;    /* count(*) over the frame              */
    int64_t *count_v;       /* count(v) over the frame              */
    double  *sum_v;         /* sum(v)  over the frame (float8pl)    */
    uint8_t *sum_isnull;    /* 1 where the frame holds no non-NULL v */
    int64_t *part_rows;     /* rows in the partition (WinGetPartitionRowCount) */
} otbx_window_out;

otbx_status otbx_window_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_window(const otbx_sortspec *spec, int32_t npart,
                        const int64_t *perm_dev, int64_t n,
                        const double *vals_dev, const uint8_t *val_null_dev,
                        void *ws_dev, size_t ws_bytes,
                        const otbx_window_out *out, void *stream);

/* ---- GPU WindowAgg frames: lag / lead, ntile, value functions and
 * aggregates over an explicit ROWS or RANGE frame ----
 * The rest of ExecWindowAgg for the reference's frame model: one call serves
 * ONE window specification and ONE frame and evaluates up to
 * OTBX_MAX_WINCALLS function calls that share them. spec, npart, perm_dev
 * (NULL = identity; entries are clamped) and n mean exactly what they mean
 * for otbx_window, and partition / peer equality is the sort's normalised
 * key. otbx_window is unchanged; this entry point stands beside it.
 *
 * FRAME (row_is_in_frame / update_frameheadpos, nodeWindowAgg.c:1472-1560)
 *   For sorted position j in partition [ps, pe] with peer group [gs, ge] the
 *   frame is [lo, hi], empty when lo > hi.
 *   ROWS:  lo = ps (UNBOUNDED) or max(ps, j + start_off);
 *          hi = pe (UNBOUNDED) or min(pe, j + end_off); CURRENT is offset 0.
 *   RANGE: lo = ps (UNBOUNDED) or gs (CURRENT); hi = pe (UNBOUNDED) or ge
 *          (CURRENT). OTBX_FB_OFFSET under RANGE is OTBX_ERR_INVALID.
 *   Offsets are any int64; j + off saturates, so INT64_MIN / INT64_MAX mean
 *   "before / after everything". The parser's shape restrictions
 *   (gram.y:17275-17316: no "UNBOUNDED FOLLOWING" start, no start after the
 *   end, ...) are NOT enforced: a shape such as "CURRENT ROW .. 1 PRECEDING"
 *   simply gives empty frames.
 *
 * FUNCTIONS — col / nulls are indexed by INPUT row and read through perm;
 * every output is indexed by SORTED POSITION.
 *   NTILE(param)       int32 (window_ntile, windowfuncs.c:231): with T rows
 *                      in the partition, q = T / param, r = T % param and
 *                      0-based row i: i + 1 if q == 0; i/(q+1) + 1 if
 *                      i < r*(q+1); else r + (i - r*(q+1))/q + 1.
 *   LAG / LEAD(param)  leadlag_common (:306) with a constant signed offset
 *                      (a negative lag is a lead); the frame is ignored. The
 *                      source position j -/+ param inside the partition
 *                      gives that row's value and null flag; outside it the
 *                      default: def_i (I64 / I32 / U8) or def_f (F64), or
 *                      NULL when def_isnull is set.
 *   FIRST_VALUE / LAST_VALUE / NTH_VALUE(param >= 1)
 *                      WinGetFuncArgInFrame (nodeWindowAgg.c:3368): the row
 *                      at lo, hi or lo + param - 1; NULL when the frame is
 *                      empty or that position is past hi. A NULL value is
 *                      returned as NULL (no IGNORE NULLS).
 *   COUNT_STAR / COUNT / SUM / MIN / MAX over the frame: the result types,
 *                      strictness, int128 SUM(I64) encoding and float MIN /
 *                      MAX rules (bit pattern of the chosen row, the later
 *                      row of the frame wins a tie) of otbx_group_agg. An
 *                      empty frame, or one without a non-NULL input, gives
 *                      out_null = 1 and value 0 for SUM / MIN / MAX, and 0
 *                      for the counts.
 *   Wherever a result is NULL the value stored is 0. out_null is required
 *   for every function except NTILE and the two counts and must be NULL for
 *   those; out_hi is required for SUM over I64 and must be NULL otherwise.
 *
 * NUMERICS OF SUM(F64): float8 sum has no inverse transition, so the
 *   reference re-aggregates every frame left to right (eval_windowaggregates,
 *   nodeWindowAgg.c:919-933). Here the reduction is SEGMENTED: no differences
 *   of float prefix sums and no float atomics, so an Inf or NaN never leaks
 *   into another frame or partition. With both bounds OFFSET / CURRENT under
 *   ROWS and end_off - start_off + 1 at most the direct cut-over, the frame's
 *   non-NULL values are added left to right: BIT-EQUAL to the reference.
 *   Otherwise (an unbounded side, RANGE, or a wider frame) the sum is a
 *   tree: within m*u*sum|x| / (1 - m*u), m = non-NULL terms - 1, u = 2^-53
 *   (otbx_window's clause), bit-equal wherever every order is exact. Results
 *   are bit-identical from run to run. Overflow of finite inputs is not
 *   detected.
 *
 * DIRECT CUT-OVER: *width of otbx_window_frame_direct_default (128) is the widest
 *   bounded ROWS frame reduced by a per-row loop; wider ones take two
 *   segmented scans whatever their width. OTBX_WIN_FRAME_DIRECT=N overrides
 *   it at call time (0 = never direct).
 *
 * Stream-ordered, no host synchronisation, nothing cached (otbx_finish has
 * nothing to release). Checked before any HIP call, each returning
 * OTBX_ERR_INVALID: spec, frame or calls NULL; ncalls outside 1..8; nkeys,
 * npart, key type / flags, key columns and n as for otbx_window; units or a
 * bound kind out of range, or OFFSET under RANGE; func or type of a call out
 * of range; out NULL; col NULL with n > 0 for anything but NTILE /
 * COUNT_STAR / COUNT; the out_null / out_hi rules above; NTILE param <= 0,
 * NTH_VALUE param < 1, a LAG / LEAD param outside int32; ws_bytes below
 * otbx_window_frame_workspace_bytes(n, ncalls), ws_dev NULL or not 16-byte
 * aligned. n == 0 is valid and writes nothing.
 * otbx_window_frame_workspace_bytes is pure host code and monotone in both
 * arguments. sizeof(otbx_frame) == 32, sizeof(otbx_wincall) == 80. */
enum { OTBX_FRAME_ROWS = 0, OTBX_FRAME_RANGE = 1 };
enum { OTBX_FB_UNBOUNDED = 0,  /* start: UNBOUNDED PRECEDING; end: UNBOUNDED FOLLOWING */
       OTBX_FB_CURRENT   = 1,  /* CURRENT ROW; under RANGE: first / last peer          */
       OTBX_FB_OFFSET    = 2 };/* ROWS only: position + off; off<0 PRECEDING, >0 FOLLOWING */
typedef struct {
    int32_t units, start_kind, end_kind, _pad;
    int64_t start_off, end_off;
} otbx_frame;

enum { OTBX_WF_NTILE = 0, OTBX_WF_LAG, OTBX_WF_LEAD, OTBX_WF_FIRST_VALUE,
       OTBX_WF_LAST_VALUE, OTBX_WF_NTH_VALUE, OTBX_WF_COUNT_STAR,
       OTBX_WF_COUNT, OTBX_WF_SUM, OTBX_WF_MIN, OTBX_WF_MAX };
#define OTBX_MAX_WINCALLS 8
typedef struct {
    const void    *col;        /* input column of `type`, indexed by INPUT row  */
    const uint8_t *nulls;      /* byte per row, nonzero = NULL; may be NULL      */
    void          *out;        /* n entries, indexed by SORTED position          */
    int64_t       *out_hi;     /* SUM over I64 only: high words                  */
    uint8_t       *out_null;   /* see above                                      */
    int64_t        param;      /* NTILE: buckets; LAG/LEAD: offset; NTH_VALUE: n */
    int64_t        def_i;      /* LAG/LEAD default for I64 / I32 / U8            */
    double         def_f;      /* LAG/LEAD default for F64                       */
    int32_t        def_isnull; /* LAG/LEAD: the default is NULL                  */
    int32_t        func;       /* OTBX_WF_*                                      */
    int32_t        type;       /* OTBX_SORT_I64 / F64 / I32 / U8                 */
    int32_t        _pad;
} otbx_wincall;                /* 80 B */

otbx_status otbx_window_frame_direct_default(int64_t *width);
otbx_status otbx_window_frame_workspace_bytes(int64_t n, int32_t ncalls,
                                              size_t *bytes);
otbx_status otbx_window_frame(const otbx_sortspec *spec, int32_t npart,
                              const int64_t *perm_dev, int64_t n,
                              const otbx_frame *frame,
                              const otbx_wincall *calls, int32_t ncalls,
                              void *ws_dev, size_t ws_bytes, void *stream);

/* ---- GPU GroupAggregate: count / sum / min / max per run of equal keys ----
 * The sorted-input aggregation strategy of the Agg node (AGG_SORTED, and
 * AGG_PLAIN with no keys: agg_retrieve_direct, executor/nodeAgg.c:2249,
 * advancing every aggregate of the target list per row, advance_aggregates
 * :856). One call reduces every key run of the sorted input to ONE ROW PER
 * GROUP for up to OTBX_MAX_AGGS aggregates at once; all outputs share the
 * same group index, and groups come out in key order.
 *
 * GROUPING
 *   - spec lists the GROUP BY keys (0..8), typed and flagged as for
 *     otbx_sort_perm. Position j is input row perm_dev[j]; perm_dev == NULL
 *     means identity (the columns are already in order). An entry outside
 *     [0, n) is clamped, so it cannot address outside the columns.
 *   - A new group starts at j = 0 and wherever row j differs from row j-1 on
 *     any key. Equal means what otbx_sort_perm and otbx_window mean: NULL
 *     equals NULL, every NaN equals every NaN, -0.0 == +0.0, the value
 *     stored under a NULL is ignored (the test is made on the sort's own
 *     normalised key).
 *   - The caller guarantees that equal keys are adjacent: a perm from
 *     otbx_sort_perm on these keys, or on a longer key list with these as
 *     prefix, qualifies. This is not checked; non-adjacent equal keys form
 *     separate groups, as the reference's GroupAggregate does on unsorted
 *     input.
 *   - Groups are emitted in position order: output g is the g-th key run.
 *     first_row_dev[g] is the input row index of the group's first position
 *     (the representative tuple, the row_idx convention of otbx_agg_i64n);
 *     it feeds otbx_gather_* to materialise the key columns.
 *   - naggs == 0 is legal: DISTINCT on the keys.
 *   - nkeys == 0 is AGG_PLAIN: one group over all rows. With n == 0 it still
 *     emits one row, as agg_retrieve_direct does for an empty input without
 *     grouping columns: counts 0, SUM / MIN / MAX NULL, first_row = -1.
 *   - nkeys > 0 and n == 0: *ngroups_dev = 0 and nothing else is written.
 *
 * AGGREGATES — all transition functions are strict: NULL inputs are skipped
 * and the first non-NULL input becomes the state.
 *   COUNT_STAR            int64 rows in the group           (int8inc :714)
 *   COUNT      any type   int64 non-NULL rows; only the mask is read, and
 *                         without a mask it equals COUNT_STAR (int8inc_any)
 *   SUM   F64             double (float8pl, float.c:970); see NUMERICS
 *   SUM   I32, U8         int64, exact (int4_sum, numeric.c:6154; cannot
 *                         overflow for n <= INT32_MAX)
 *   SUM   I64             exact int128: out = uint64 low word, out_hi =
 *                         int64 high word (int8_sum / Int128AggState; the
 *                         encoding of otbx_dec_group)
 *   MIN / MAX I64,I32,U8  same type as the input (int8smaller / int8larger,
 *                         int4larger)
 *   MIN / MAX F64         double, the BIT PATTERN OF THE CHOSEN INPUT ROW
 *                         (float8smaller / float8larger, float.c:839/853)
 *   SUM / MIN / MAX of a group without a non-NULL input: out_null = 1 and
 *   the value stored is 0.
 *
 * FLOAT MIN / MAX follow float8_cmp_internal: NaN is greater than
 *   everything, +Inf included. On a tie the reference returns its second
 *   argument, so THE LATER ROW IN POSITION ORDER WINS; this covers -0 / +0
 *   and NaNs of different sign or payload and is reproduced bit for bit:
 *   MAX of [+0.0, -0.0] is -0.0 and of [-0.0, +0.0] is +0.0; MAX of
 *   [NaN(a), 1.0, NaN(b)] is NaN(b); MIN of [1.0, NaN] is 1.0; MIN of an
 *   all-NaN group is its last NaN. ("Keep the left operand if it is strictly
 *   greater — MIN: strictly smaller — else the right" is associative, so the
 *   order-preserving tree reduction is exact.)
 *
 * NUMERICS OF SUM(F64): the clause of otbx_window's sum_v. The reduction is
 *   SEGMENTED — nothing from one group ever reaches another, nothing is a
 *   difference of prefix sums, and there are no float atomics. The identity
 *   is -0.0. The association order is a tree: bit-equal to left-to-right
 *   float8pl wherever every order is exact, and otherwise within
 *   m*u*sum|x| / (1 - m*u), m = group rows - 1, u = 2^-53. Overflow of
 *   finite inputs is not detected. The result is run-to-run deterministic:
 *   the same call twice gives the same bits.
 *
 * Stream-ordered, no host synchronisation, nothing cached (otbx_finish has
 * nothing to release); entries past *ngroups_dev are never written. Checked
 * before any HIP call, each returning OTBX_ERR_INVALID: spec, aggs or
 * ngroups_dev NULL; nkeys outside 0..8; naggs outside 0..8; a key type code
 * outside 0..3 or key flags outside bits 0-1; func or type of an aggregate
 * out of range; SUM / MIN / MAX with col == NULL and n > 0; out == NULL;
 * out_null missing for SUM / MIN / MAX or present for a count; out_hi
 * missing for SUM over I64 or present for anything else; naggs == 0 with
 * first_row_dev == NULL (nothing requested); n < 0 or n > INT32_MAX; a NULL
 * key column with n > 0; ws_bytes below otbx_group_agg_workspace_bytes(n),
 * or ws_dev not 16-byte aligned. otbx_group_agg_workspace_bytes is pure host
 * code and monotone in n. */
enum { OTBX_AGG_COUNT_STAR = 0, OTBX_AGG_COUNT, OTBX_AGG_SUM,
       OTBX_AGG_MIN, OTBX_AGG_MAX };
#define OTBX_MAX_AGGS 8
typedef struct {
    const void    *col;      /* input column of `type`; ignored by COUNT_STAR / COUNT */
    const uint8_t *nulls;    /* byte per row, nonzero = NULL; may be NULL              */
    void          *out;      /* one entry per group, capacity n                        */
    int64_t       *out_hi;   /* SUM over I64 only: high words of the int128 sum        */
    uint8_t       *out_null; /* SUM / MIN / MAX: 1 where the group held no non-NULL
                                input (value stored is 0); must be NULL for counts     */
    int32_t        func;     /* OTBX_AGG_*                                             */
    int32_t        type;     /* OTBX_SORT_I64 / F64 / I32 / U8                         */
} otbx_aggcall;              /* 48 B */
typedef struct { int32_t naggs; int32_t _pad; otbx_aggcall agg[OTBX_MAX_AGGS]; } otbx_aggcalls;

otbx_status otbx_group_agg_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_group_agg(const otbx_sortspec *spec,   /* the GROUP BY keys, 0..8 */
                           const int64_t *perm_dev,     /* NULL = identity         */
                           int64_t n, const otbx_aggcalls *aggs,
                           void *ws_dev, size_t ws_bytes,
                           int64_t *first_row_dev,      /* capacity n; may be NULL */
                           int64_t *ngroups_dev,        /* int64[1], required      */
                           void *stream);

/* ---- GPU DISTINCT and ordered-set aggregates over sorted input ----
 * The aggregates that sort their own input inside each group: agg(DISTINCT x)
 * (process_ordered_aggregate_single, executor/nodeAgg.c:888: sort, then skip
 * every row equal to its predecessor) and the ordered-set aggregates
 * percentile_disc / percentile_cont / mode() WITHIN GROUP (ORDER BY x)
 * (utils/adt/orderedsetaggs.c: sort, then pick or interpolate a row). Here
 * the sort is done ONCE for all groups: the caller sorts on (GROUP BY keys,
 * x) with otbx_sort_perm, and every aggregate is one pass over that
 * permutation.
 *
 * INPUTS AND GROUPING
 *   - spec->nkeys == ngroup + 1, 0 <= ngroup <= 7. key[0..ngroup-1] are the
 *     GROUP BY keys; key[ngroup] is the ONE argument column x that all calls
 *     share. Its type, null mask, DESC and NULLS FIRST flags are the sort
 *     key's: "ORDER BY x DESC NULLS FIRST" is a flag pair, not another call.
 *   - perm_dev is what otbx_sort_perm(spec, n, limit 0) returned; NULL means
 *     identity. An entry outside [0, n) is clamped.
 *   - Group g is the g-th run of equal GROUP BY keys. The numbering,
 *     first_row_dev and *ngroups_dev are exactly what otbx_group_agg gives
 *     for the first ngroup keys of spec and the same perm_dev, so a target
 *     list can take count(DISTINCT x) from here and sum(y) from
 *     otbx_group_agg side by side, from one sort.
 *   - ngroup == 0 is AGG_PLAIN: one group over all rows. With n == 0 it
 *     still emits one row: COUNT_DISTINCT 0, everything else NULL,
 *     first_row = -1. ngroup > 0 and n == 0: *ngroups_dev = 0, nothing else
 *     is written.
 *   - Equality everywhere is that of the sort's normalised key: NULL equals
 *     NULL, every NaN equals every NaN, -0.0 == +0.0, and the value stored
 *     under a NULL is ignored.
 *   - ncalls == 0 is legal and needs first_row_dev: DISTINCT on the GROUP BY
 *     keys.
 *
 * NULL ARGUMENTS take part in no aggregate (the transition functions are
 *   strict; ordered_set_transition drops NULLs). Inside a group they sit
 *   together at the end the key's flags put them. Below, N is the number of
 *   the group's non-NULL rows and lo the position of the first of them, so
 *   they occupy positions lo .. lo+N-1 in the order of perm_dev.
 *
 * AGGREGATES ("the value at position j" is the argument of row perm_dev[j])
 *   COUNT_DISTINCT      int64: the runs of equal non-NULL values; 0 for an
 *                       all-NULL group. Never NULL.
 *   SUM_DISTINCT        the sum over the FIRST POSITION of each such run,
 *                       typed and encoded exactly as OTBX_AGG_SUM: F64 gives
 *                       a double under the NUMERICS clause of otbx_group_agg
 *                       (a segmented tree, deterministic; m = runs - 1);
 *                       I32 / U8 give an exact int64; I64 gives the exact
 *                       int128 in out / out_hi. NULL when N == 0.
 *   PERCENTILE_DISC(p)  the value at lo + max(K, 1) - 1 with
 *                       K = (int64)ceil(p * (double)N): the type of the
 *                       column, the BIT PATTERN of that row
 *                       (orderedsetaggs.c:468). NULL when N == 0.
 *   PERCENTILE_CONT(p)  always a double. t = p * (double)(N - 1),
 *                       f = floor(t), c = ceil(t); if f == c the value at
 *                       lo + f, else v_f + (t - f) * (v_c - v_f), evaluated
 *                       in exactly that order without a fused multiply-add
 *                       (:568-594, float8_lerp :496). Integer columns
 *                       convert as i8tod / i4tod. Bit-exact. NULL when
 *                       N == 0.
 *   MODE                the value at the first position of the longest run
 *                       of equal non-NULL values; among runs of equal
 *                       length the earliest in sort order (mode_final :1090
 *                       takes a new mode only on ">"). Type of the column,
 *                       bit pattern of that row. NULL when N == 0.
 *   A NULL result stores 0 and sets out_null = 1. A NaN that the arithmetic
 *   itself creates (SUM_DISTINCT over +Inf and -Inf, PERCENTILE_CONT between
 *   them) is a NaN with the adder's payload; a NaN that is picked
 *   (PERCENTILE_DISC, MODE, PERCENTILE_CONT with f == c) keeps its bits.
 *   Several percentiles — the reference's percentile_disc(array[...]) too —
 *   are several calls of one invocation. avg(DISTINCT x) is a finalizer over
 *   SUM_DISTINCT and COUNT_DISTINCT. Since otbx_sort_perm is stable and the
 *   reference's sort is not, "the row" among equal values is defined by
 *   perm_dev: the first position of the run. That is what makes -0 / +0 and
 *   NaN payloads reproducible bit for bit.
 *
 * Stream-ordered, no host synchronisation, nothing cached (otbx_finish has
 * nothing to release); entries past *ngroups_dev are never written. Checked
 * before any HIP call, each returning OTBX_ERR_INVALID: spec, calls or
 * ngroups_dev NULL; ngroup outside 0..7 or nkeys != ngroup + 1; a key type
 * code outside 0..3 or key flags outside bits 0-1; ncalls outside 0..8;
 * ncalls == 0 with first_row_dev == NULL; func out of range; fraction below
 * 0, above 1 or NaN on a percentile call (the reference raises "percentile
 * value is not between 0 and 1"); out == NULL; out_null missing where the
 * result can be NULL or present for COUNT_DISTINCT; out_hi missing for
 * SUM_DISTINCT over I64 or present elsewhere; n < 0 or n > INT32_MAX; a NULL
 * key column with n > 0; ws_bytes below
 * otbx_ordered_agg_workspace_bytes(n, ncalls), or ws_dev not 16-byte
 * aligned. The workspace function is pure host code and monotone in n. */
enum { OTBX_OAGG_COUNT_DISTINCT = 0, OTBX_OAGG_SUM_DISTINCT,
       OTBX_OAGG_PERCENTILE_DISC, OTBX_OAGG_PERCENTILE_CONT, OTBX_OAGG_MODE };
typedef struct {
    void    *out;       /* one entry per group, capacity n                      */
    int64_t *out_hi;    /* SUM_DISTINCT over I64 only: high words of the int128 */
    uint8_t *out_null;  /* 1 where the result is NULL; must be NULL for
                           COUNT_DISTINCT                                       */
    double   fraction;  /* the percentiles' p in [0, 1]; ignored elsewhere      */
    int32_t  func;      /* OTBX_OAGG_*                                          */
    int32_t  _pad;
} otbx_oaggcall;        /* 40 B */
typedef struct { int32_t ncalls; int32_t _pad; otbx_oaggcall call[OTBX_MAX_AGGS]; } otbx_oaggcalls;

otbx_status otbx_ordered_agg_workspace_bytes(int64_t n, int32_t ncalls,
                                             size_t *bytes);
otbx_status otbx_ordered_agg(const otbx_sortspec *spec,  /* GROUP BY keys, then x */
                             int32_t ngroup,             /* 0..7                  */
                             const int64_t *perm_dev,    /* NULL = identity       */
                             int64_t n, const otbx_oaggcalls *calls,
                             void *ws_dev, size_t ws_bytes,
                             int64_t *first_row_dev,     /* capacity n; may be NULL */
                             int64_t *ngroups_dev,       /* int64[1], required    */
                             void *stream);

/* ---- generic GPU Filter: WHERE quals → ordered selection vector ----
 * The ExecScan / ExecQual analog (executor/execScan.c:140-363 over the
 * expression steps of executor/execExprInterp.c) for any qual in
 * conjunctive normal form over typed, nullable columns: clauses are AND'ed,
 * the terms of one clause are OR'ed, and a term is
 *     col OP constant | col OP rcol | col IS NULL | col IS NOT NULL
 * with OP one of = <> < <= > >=. Clause ids are non-decreasing along
 * term[], so a clause is a run of adjacent terms. nterms == 0 selects every
 * row (ExecQual with no qual returns true).
 *
 * RESULT: sel_dev[0 .. *nsel_dev) receives the passing row indices in
 * ASCENDING order (order-preserving, deterministic compaction), int64 so
 * it feeds otbx_gather_* unchanged; entries past *nsel_dev are not written.
 * With sel_dev == NULL only the count is produced and the write pass is not
 * launched (SELECT count(*) ... WHERE).
 *
 * SEMANTICS
 *   - A row passes iff the whole qual is TRUE; NULL counts as failure
 *     (EEOP_QUAL, execExprInterp.c:919).
 *   - A comparison with a NULL operand is NULL (strict operator,
 *     EEOP_FUNCEXPR_STRICT :703). AND / OR are Kleene (EEOP_BOOL_AND_STEP*
 *     :783-838, EEOP_BOOL_OR_STEP* :850-904). There is no NOT above a term
 *     and every operator has its complement, so this collapses to: a row
 *     passes iff EVERY clause has AT LEAST ONE term that is TRUE, a term
 *     being TRUE only when its operands are non-NULL and the comparison
 *     holds.
 *   - ISNULL / NOTNULL are never NULL (EEOP_NULLTEST_ISNULL :973); a column
 *     without a mask has no NULLs.
 *   - The value stored under a NULL never influences the result.
 *   - I64 / I32 / U8: ordinary integer order; the column value is widened
 *     to int64 and compared with `ci`, so a constant outside the column's
 *     range is legal and compares mathematically (u8col < 256 is always
 *     true, i32col = 2^40 never).
 *   - F64: float8_cmp_internal (utils/adt/float.c:1172), exactly as
 *     otbx_sort_perm orders — every NaN equals every NaN whatever its sign
 *     or payload and is greater than every non-NaN, +Inf included;
 *     -0.0 == +0.0 — for `cf` as well as for column values.
 *
 * Columns need only the natural alignment of their element type (a torch
 * view such as col[1:] is a valid input); 16-byte-aligned columns take the
 * vector-load path.
 *
 * Stream-ordered, no host synchronisation, nothing cached. Checked before
 * any HIP call, each returning OTBX_ERR_INVALID: q or nsel_dev NULL; nterms
 * outside 0..16; a type outside 0..3; an op outside 0..7; rcol set together
 * with ISNULL / NOTNULL; rnulls set without rcol; decreasing clause ids;
 * n < 0 or n > INT32_MAX; a NULL col with n > 0; ws_bytes below
 * otbx_filter_workspace_bytes(n); ws_dev not 16-byte aligned. n == 0 is
 * valid and writes *nsel_dev = 0. otbx_filter_workspace_bytes is pure host
 * code and monotone in n (n/8 B of bitmask padded to whole tiles + 4 B per
 * tile). sizeof(otbx_qualterm) == 64, sizeof(otbx_qual) == 1032. */
enum { OTBX_CMP_EQ = 0, OTBX_CMP_NE, OTBX_CMP_LT, OTBX_CMP_LE, OTBX_CMP_GT,
       OTBX_CMP_GE, OTBX_CMP_ISNULL, OTBX_CMP_NOTNULL };
#define OTBX_MAX_QUAL_TERMS 16
typedef struct {
    const void    *col;     /* left operand: device column of `type`          */
    const uint8_t *nulls;   /* byte per row, nonzero = NULL; may be NULL      */
    const void    *rcol;    /* non-NULL: right operand is a column of the     */
    const uint8_t *rnulls;  /*   SAME type (col OP rcol); NULL: a constant    */
    int64_t        ci;      /* constant for I64 / I32 / U8 columns            */
    double         cf;      /* constant for F64 columns                       */
    int32_t        type;    /* OTBX_SORT_I64 / F64 / I32 / U8 (same codes)    */
    int32_t        op;      /* OTBX_CMP_*                                     */
    int32_t        clause;  /* terms with equal clause id are OR'ed           */
    int32_t        _pad;
} otbx_qualterm;
typedef struct { int32_t nterms; otbx_qualterm term[OTBX_MAX_QUAL_TERMS]; } otbx_qual;

otbx_status otbx_filter_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_filter_sel(const otbx_qual *q, int64_t n,
                            void *ws_dev, size_t ws_bytes,
                            int64_t *sel_dev,   /* cap n; NULL = count only */
                            int64_t *nsel_dev,  /* int64[1], required       */
                            void *stream);

/* ---- generic GPU Project: one typed scalar expression per row ----
 * The ExecProject analog for one target-list entry (the expression steps of
 * executor/execExprInterp.c): a postfix program over typed, nullable
 * columns is evaluated for every output row into one output column plus
 * null mask. With sel_dev the rows are read through a selection vector
 * (what otbx_filter_sel wrote): output row j is computed from source row
 * sel_dev[j]; rows the selection leaves out are never evaluated. An entry
 * outside [0, n_src) is clamped into it, so a broken selection can never
 * index outside the columns.
 *
 * PROGRAM: instr[0 .. ninstr) in postfix order over a value stack of at
 * most OTBX_MAX_EXPR_DEPTH entries. A value is INT8 (int64), FLOAT8
 * (double) or BOOL and carries a null flag. I32 and U8 columns widen to
 * INT8 on load (the int48 implicit cast); int4-typed arithmetic does not
 * exist here. Every function is strict (a NULL operand gives NULL, the
 * function is not called) unless stated:
 *   COL              push column `col` of `type` OTBX_SORT_*, mask `nulls`
 *   CONST            push `ci` (INT8; BOOL: nonzero = TRUE) or `cf` (FLOAT8)
 *                    of `type` OTBX_EXT_*; isnull != 0: the NULL of that type
 *   ADD SUB MUL DIV  two INT8 (int8pl/mi/mul/div, utils/adt/int8.c:534-640)
 *                    or two FLOAT8 (float8pl/mi/mul/div, float.c:809-1025)
 *   MOD              two INT8 (int8mod :643): x % -1 = 0, sign of dividend
 *   NEG ABS          one INT8 (int8um, int8abs) or FLOAT8 (sign bit only)
 *   CAST             `type` = OTBX_EXT_FLOAT8 on INT8: i8tod (int8.c:1235);
 *                    OTBX_EXT_INT8 on FLOAT8: dtoi8 (:1249), rint (ties to
 *                    even) then the range check
 *   EQ NE LT LE GT GE  two INT8 or two FLOAT8 → BOOL; FLOAT8 compares as
 *                    float8_cmp_internal, exactly as the Filter and the Sort
 *                    do: every NaN equals every NaN and is above +Inf,
 *                    -0 = +0
 *   AND OR           two BOOL, Kleene (EEOP_BOOL_AND_STEP* / OR_STEP*,
 *                    execExprInterp.c:783-904); not strict
 *   NOT              one BOOL
 *   ISNULL NOTNULL   any type → BOOL, never NULL
 *   CASE             pops else, then, cond: `then` iff cond is TRUE, a NULL
 *                    cond takes the else arm (EEOP_JUMP_IF_NOT_TRUE :964);
 *                    arms of one type
 *   COALESCE         two values of one type: the first if non-NULL, else
 *                    the second
 *
 * ERRORS are values. The reference aborts at the first row whose evaluation
 * raises and never evaluates the untaken arm of a CASE, the right side of an
 * AND whose left is FALSE (OR: TRUE) or the second argument of a COALESCE
 * whose first is non-NULL. Evaluation here is eager and every stack value
 * carries an error code:
 *   - strict operator: its first operand's code if nonzero, else the
 *     second's, else — only when every operand is non-NULL — its own. A NULL
 *     operand never hides an error raised in a sibling subtree.
 *   - CASE: cond's code, else the code of the chosen arm only.
 *   - AND / OR: the left code; the right code only if the left value did
 *     not decide the result. COALESCE: the first code; the second only if
 *     the first value is NULL. ISNULL / NOTNULL: the operand's code.
 *   - the value stored under a NULL is never used and never raises.
 * Codes (OTBX_EXERR_*): 1 division by zero (INT8 x / 0, x % 0; FLOAT8
 * x / ±0.0 whatever x, NaN and 0 included); 2 bigint out of range (INT8
 * overflow of + - *, INT64_MIN / -1, -INT64_MIN, abs(INT64_MIN); dtoi8 of
 * NaN or of a rounded value outside [-2^63, 2^63) — the reference's check
 * lets exactly 2^63 through into an undefined C conversion, here 2^63
 * raises); 3 value out of range: overflow (CHECKFLOATVAL, float.c:58:
 * FLOAT8 result ±Inf and no operand was); 4 value out of range: underflow
 * (result 0 and MUL: neither operand 0, DIV: dividend not 0; ADD / SUB
 * never); 5 integer out of range (int84, int8.c:1201, on an I32 output).
 *
 * ERROR SLOT: *err_dev receives -1 when no output row raised, otherwise
 * (j << 8) | code for the SMALLEST output position j that raised and that
 * row's code (deterministic: an unsigned 64-bit minimum). It is written by
 * the call, stream-ordered. When the slot is not -1 the contents of out_dev
 * and out_null_dev are unspecified: the caller MUST read the slot before it
 * uses the output.
 *
 * OUTPUT: out_type OTBX_SORT_I64 takes an INT8 result, F64 a FLOAT8 one,
 * I32 an INT8 one through int84's range check (code 5), U8 a BOOL as 0 / 1.
 * out_null_dev[j] is 1 where the result is NULL, else 0; the value stored
 * under a NULL is 0. out_null_dev may be NULL only when the program cannot
 * produce NULL, decided by the abstract interpretation that type-checks it:
 * a COL with a mask and a NULL CONST are the only sources; arithmetic,
 * casts, comparisons, NOT, AND, OR and CASE are nullable when any value
 * operand is (CASE: either arm), COALESCE when both are, ISNULL / NOTNULL
 * never. FLOAT8 results are bit-exact IEEE (no contraction).
 *
 * Columns, masks and outputs need only the natural alignment of their
 * element type (col[1:] is legal); 16-byte-aligned ones take the
 * vector-access path on whole tiles. No workspace, nothing cached, no host
 * synchronisation. Checked before any HIP call, each returning
 * OTBX_ERR_INVALID: e or err_dev NULL; ninstr outside 1..32; an unknown op
 * or type code; a stack underflow or a depth above 8; operand types that do
 * not fit the operator (INT8 meeting FLOAT8 without a cast, MOD on FLOAT8,
 * AND on a non-BOOL, CASE arms of different types, a CAST to the operand's
 * own type or from / to BOOL, ...); a final stack that does not hold exactly
 * one value; out_type not matching it; n < 0, n > INT32_MAX, n_src < 0,
 * n > n_src without sel_dev, n > 0 with n_src == 0; a NULL col with n > 0;
 * out_dev NULL with n > 0; out_null_dev NULL although the result is
 * nullable. n == 0 is valid and writes *err_dev = -1.
 * sizeof(otbx_exprinstr) == 48, sizeof(otbx_expr) == 1544. */
enum { OTBX_EX_COL = 0, OTBX_EX_CONST, OTBX_EX_ADD, OTBX_EX_SUB, OTBX_EX_MUL,
       OTBX_EX_DIV, OTBX_EX_MOD, OTBX_EX_NEG, OTBX_EX_ABS, OTBX_EX_CAST,
       OTBX_EX_EQ, OTBX_EX_NE, OTBX_EX_LT, OTBX_EX_LE, OTBX_EX_GT, OTBX_EX_GE,
       OTBX_EX_AND, OTBX_EX_OR, OTBX_EX_NOT, OTBX_EX_ISNULL, OTBX_EX_NOTNULL,
       OTBX_EX_CASE, OTBX_EX_COALESCE };
enum { OTBX_EXT_INT8 = 0, OTBX_EXT_FLOAT8 = 1, OTBX_EXT_BOOL = 2 };
enum { OTBX_EXERR_DIV0 = 1, OTBX_EXERR_INT8 = 2, OTBX_EXERR_OVERFLOW = 3,
       OTBX_EXERR_UNDERFLOW = 4, OTBX_EXERR_INT4 = 5 };
#define OTBX_MAX_EXPR_INSTRS 32
#define OTBX_MAX_EXPR_DEPTH  8
typedef struct {
    const void    *col;     /* COL: device column of `type`                   */
    const uint8_t *nulls;   /* COL: byte per row, nonzero = NULL; may be NULL */
    int64_t        ci;      /* CONST INT8 / BOOL payload                      */
    double         cf;      /* CONST FLOAT8 payload                           */
    int32_t        op;      /* OTBX_EX_*                                      */
    int32_t        type;    /* COL: OTBX_SORT_*; CONST / CAST: OTBX_EXT_*     */
    int32_t        isnull;  /* CONST: nonzero = the NULL of `type`            */
    int32_t        _pad;
} otbx_exprinstr;
typedef struct {
    int32_t ninstr; int32_t _pad;
    otbx_exprinstr instr[OTBX_MAX_EXPR_INSTRS];
} otbx_expr;

otbx_status otbx_project(const otbx_expr *e,
                         const int64_t *sel_dev,  /* NULL = identity          */
                         int64_t n,      /* output rows (= len(sel) if given) */
                         int64_t n_src,  /* rows in the columns               */
                         int32_t out_type,        /* OTBX_SORT_*              */
                         void *out_dev, uint8_t *out_null_dev,
                         int64_t *err_dev,        /* int64[1], required       */
                         void *stream);

/* ---- GPU text columns: LIKE / compare predicates and text gather ----
 * A text column is variable-width: row i is bytes[offs[i] .. offs[i+1]).
 * offs[0] need not be 0, so offs[a : b+1] over the same bytes is a valid
 * column (a slice costs nothing). Every offset a kernel reads is clamped
 * into [0, nbytes] and a negative length reads as 0, so broken offsets can
 * never address outside bytes — the policy the other operators apply to
 * perm and sel entries. The bytes under a NULL are never read for their
 * value. sizeof(otbx_textcol) == 32.
 *
 * otbx_text_pred evaluates ONE predicate per call into a uint8 0 / 1
 * column plus null mask — the operand types a U8 otbx_qualterm (b = 1) and
 * Project's COL take, so a text qual flows into otbx_filter_sel without a
 * text term in the pinned otbx_qualterm. Every function is strict: a NULL
 * operand gives NULL, the value stored under a NULL is 0. out_null_dev may
 * be NULL only when no operand carries a mask. With sel_dev, output row j
 * is evaluated on source row sel_dev[j], clamped into [0, n_src); rows the
 * selection leaves out are never read.
 *
 * The right operand is either the column *right (the six comparisons only;
 * `right` is a host pointer, read during the call) or the constant
 * cbytes[0 .. clen), at most OTBX_MAX_TEXT_CONST bytes; it travels in the
 * launch arguments by value.
 *   LIKE / NLIKE     textlike / textnlike (utils/adt/like.c:269,290) over
 *                    MatchText (like_match.c:78): % any sequence, _ one
 *                    character, \ makes the next pattern byte literal, the
 *                    empty pattern matches only the empty text, everything
 *                    else compares bytewise (no case folding; no ILIKE).
 *                    `encoding` decides how _ and the restart after a %
 *                    advance: OTBX_TEXT_SB one byte (SB_MatchText),
 *                    OTBX_TEXT_UTF8 the fast NextChar (like.c:142): one
 *                    byte, then every following byte with
 *                    (b & 0xC0) == 0x80. The UTF-8 is not validated;
 *                    invalid sequences match exactly as that macro makes
 *                    them. The pattern is parsed on the host, before any
 *                    HIP call, into literal / any-character / any-sequence
 *                    tokens, a run of % and _ collapsed to "k characters,
 *                    then any sequence" (like_match.c:128-144); the kernel
 *                    matches iteratively with two cursors and one restart
 *                    point (the position after the last %, advanced by one
 *                    CHARACTER on a mismatch) — the same language as the
 *                    reference's recursion, O(text × pattern), no stack.
 *                    A pattern whose last byte is an unescaped \ is refused
 *                    with OTBX_ERR_INVALID at call time. The reference
 *                    raises "LIKE pattern must not end with escape
 *                    character" only on rows whose match reaches that byte;
 *                    refusing always is stricter and data-independent. The
 *                    ESCAPE clause is host work (do_like_escape,
 *                    like_match.c:247; executor.like_escape).
 *   EQ NE LT LE GT GE  texteq / textne / text_lt … (varlena.c:1874-1998)
 *                    under C collation (varstr_cmp with lc_collate_is_c,
 *                    varlena.c:1624-1629): memcmp over the common prefix,
 *                    bytes as UNSIGNED, then the shorter string is smaller.
 *                    EQ / NE decide on the lengths first, as texteq does.
 *                    Other collations are not supported.
 * Stream-ordered, no workspace, no host synchronisation, nothing cached.
 * Checked before any HIP call, each returning OTBX_ERR_INVALID: p NULL;
 * out_dev NULL with n > 0; op or encoding out of range; a right column with
 * LIKE / NLIKE or with clen != 0; clen outside 0..256; a trailing lone
 * escape; n < 0, n > INT32_MAX, n_src < 0, n > n_src without sel_dev, n > 0
 * with n_src == 0; bytes NULL with nbytes > 0; offs NULL with n_src > 0;
 * nbytes < 0; out_null_dev NULL although an operand has a mask. n == 0 is
 * valid and writes nothing. sizeof(otbx_textpred) == 312.
 *
 * TEXT GATHER applies a selection or permutation: dst row j = src row
 * perm[j], entries clamped into [0, n_src); perm need not be a permutation
 * (join output repeats rows). Two calls, because the caller must size the
 * destination in between:
 *   otbx_text_gather_offsets  dst_offs[0] = 0, dst_offs[j+1] = dst_offs[j]
 *                    + len(perm[j]); dst_offs[n] is the total, the one
 *                    value the caller reads back (the one synchronisation,
 *                    where the Filter's caller reads its count). Tile sums
 *                    → single-workgroup scan → apply; no inter-workgroup
 *                    waiting. ws_dev: 8-byte aligned, at least
 *                    otbx_text_gather_workspace_bytes(n).
 *   otbx_text_gather_bytes    copies the bytes, balanced over OUTPUT BYTES:
 *                    each workgroup owns a fixed slice of dst_bytes and
 *                    finds its rows by binary search in dst_offs, so one
 *                    1 MiB row among short ones is copied by many
 *                    workgroups. dst_nbytes below dst_offs[n] truncates the
 *                    writes and never overruns; dst_offs that were not made
 *                    for this src and perm can give wrong bytes but never
 *                    an access outside src->bytes or dst_bytes.
 * The null mask travels by otbx_gather_u8. OTBX_ERR_INVALID before any HIP
 * call: src, dst_offs_dev or (n > 0) perm_dev NULL; n < 0, n > INT32_MAX,
 * n_src < 0, n > 0 with n_src == 0; the column checks above; a workspace
 * that is short, NULL when bytes are needed or not 8-byte aligned;
 * dst_nbytes < 0; dst_bytes_dev NULL with dst_nbytes > 0. */
enum { OTBX_TXT_LIKE = 0, OTBX_TXT_NLIKE, OTBX_TXT_EQ, OTBX_TXT_NE,
       OTBX_TXT_LT, OTBX_TXT_LE, OTBX_TXT_GT, OTBX_TXT_GE };
enum { OTBX_TEXT_SB = 0, OTBX_TEXT_UTF8 = 1 };
#define OTBX_MAX_TEXT_CONST 256
typedef struct {
    const uint8_t *bytes;   /* device, nbytes bytes, any alignment            */
    const int64_t *offs;    /* device, n+1 non-decreasing byte offsets        */
    const uint8_t *nulls;   /* byte per row, nonzero = NULL; may be NULL      */
    int64_t        nbytes;  /* size of bytes[]                                 */
} otbx_textcol;
typedef struct {
    otbx_textcol        left;
    const otbx_textcol *right;     /* host pointer; NULL = use the constant   */
    int32_t             op;        /* OTBX_TXT_*                              */
    int32_t             encoding;  /* OTBX_TEXT_*                             */
    int32_t             clen;      /* constant length, 0..256; 0 with right   */
    int32_t             _pad;
    uint8_t             cbytes[OTBX_MAX_TEXT_CONST];
} otbx_textpred;

otbx_status otbx_text_pred(const otbx_textpred *p,
                           const int64_t *sel_dev,  /* NULL = identity        */
                           int64_t n,      /* output rows (= len(sel) if given) */
                           int64_t n_src,  /* rows in the columns             */
                           uint8_t *out_dev, uint8_t *out_null_dev,
                           void *stream);

otbx_status otbx_text_gather_workspace_bytes(int64_t n, size_t *bytes);
otbx_status otbx_text_gather_offsets(const otbx_textcol *src, int64_t n_src,
                                     const int64_t *perm_dev, int64_t n,
                                     void *ws_dev, size_t ws_bytes,
                                     int64_t *dst_offs_dev /* n+1 */,
                                     void *stream);
otbx_status otbx_text_gather_bytes(const otbx_textcol *src, int64_t n_src,
                                   const int64_t *perm_dev, int64_t n,
                                   const int64_t *dst_offs_dev,
                                   uint8_t *dst_bytes_dev, int64_t dst_nbytes,
                                   void *stream);

/* ---- GPU text keys: ordered dictionary codes for sort, group, join ----
 * otbx_text_rank gives every row of a text column the dense rank of its
 * string under C collation: an order-preserving dictionary encoding. The
 * codes are an ordinary int64 key column and the column's null mask is the
 * mask the other operators take, so ORDER BY, PARTITION BY, GROUP BY,
 * DISTINCT, MIN / MAX and equi-joins over text run through otbx_sort_perm,
 * otbx_window, otbx_group_agg, otbx_agg_i64* and otbx_join_i64* unchanged;
 * the pinned otbx_sortkey / otbx_qualterm / otbx_aggcall get no text type.
 *
 * ROWS. The 1..OTBX_MAX_TEXT_RANK_COLS columns of the set form one virtual
 * column of n_total = Σ n[c] rows, numbered consecutively, column 0 first.
 * Ranking several columns jointly is what a text join needs: both sides get
 * codes from one dictionary, and no byte is copied.
 *
 * CODES. codes_dev[i] is the number of distinct non-NULL strings of the
 * whole set that are strictly smaller than row i, under varstr_cmp with
 * lc_collate_is_c (utils/adt/varlena.c:1614-1629): memcmp over the common
 * prefix, bytes UNSIGNED, then the shorter string is smaller. So
 * code(a) < code(b) ⇔ a < b, and code(a) == code(b) ⇔ same length and same
 * bytes. A 0x00 byte is an ordinary byte: "a" < "a\0" < "a\0\0" < "a\1". The
 * empty string is the smallest value and is not NULL. A NULL row gets code
 * -1; its bytes are never read.
 *
 * OUTPUTS. *ndistinct_dev = D. dict_row_dev[c], c < D, is the smallest
 * virtual row holding code c (the first occurrence: unique); it feeds
 * otbx_text_gather_* to materialise the dictionary in sorted order. Entries
 * at and past D are not written. *rounds_host is the number of refinement
 * rounds run: round r sorts the rows still undecided by bytes [8r, 8r+8)
 * with otbx_sort_perm, so rounds <= 1 + Lmax / 8 (Lmax the longest non-NULL
 * row), and rounds == 1 whenever no two non-NULL rows that share their
 * first 8 bytes are both longer than 8 bytes.
 *
 * Offsets are clamped as otbx_text_pred clamps them; broken offsets can give
 * wrong codes but never an access outside bytes. Results are bit-identical
 * from run to run.
 *
 * SYNCHRONOUS, unlike otbx_sort_perm and otbx_filter_sel: the call reads
 * back one int64 per round (the rows still undecided) and returns with the
 * stream drained, like otbx_build_q1codes. A dictionary is built once per
 * column, at staging or plan time.
 *
 * Checked before any HIP call, each returning OTBX_ERR_INVALID: ts or
 * ndistinct_dev NULL; ncols outside 1..4; an n[c] < 0; n_total > INT32_MAX;
 * per column bytes NULL with nbytes > 0, offs NULL with n[c] > 0,
 * nbytes < 0; codes_dev NULL with n_total > 0; ws_bytes below
 * otbx_text_rank_workspace_bytes(n_total); ws_dev NULL or not 16-byte
 * aligned. n_total == 0 is valid: *ndistinct_dev = 0, rounds 0.
 * otbx_text_rank_workspace_bytes is pure host code, monotone in n_total. */
#define OTBX_MAX_TEXT_RANK_COLS 4
typedef struct {
    int32_t      ncols;                         /* 1..OTBX_MAX_TEXT_RANK_COLS */
    int32_t      _pad;
    otbx_textcol col[OTBX_MAX_TEXT_RANK_COLS];
    int64_t      n[OTBX_MAX_TEXT_RANK_COLS];    /* rows of each column */
} otbx_textset;

otbx_status otbx_text_rank_workspace_bytes(int64_t n_total, size_t *bytes);
otbx_status otbx_text_rank(const otbx_textset *ts,
                           void *ws_dev, size_t ws_bytes,
                           int64_t *codes_dev,      /* n_total entries            */
                           int64_t *dict_row_dev,   /* cap n_total; may be NULL   */
                           int64_t *ndistinct_dev,  /* int64[1], required         */
                           int32_t *rounds_host,    /* may be NULL                */
                           void *stream);

/* ---- repartition exchange ----
 * The GPU half of the reference's "Distribute results by H: col" exchange
 * (make_remotesubplan, optimizer/plan/createplan.c:8671; locator semantics
 * shardid → node, pgxc/shard/shardmap.c:2231 restated as key % nranks for
 * the dense-key locator of DESIGN.md §2 — owner = (uint64_t)key % nranks,
 * i.e. the UNSIGNED-cast modulo: negative keys map to
 * (2^64 + key) % nranks, NOT the C signed remainder and NOT Python's
 * floored modulo; server-side locator code must use the same cast): groups
 * rows by owning rank into a
 * permutation with contiguous per-rank segments; the host layer then
 * all-to-alls the gathered segments over RCCL (fragment.py). nranks ≤ 64.
 * counts_host: int64[nranks], written synchronously (the call syncs). */
otbx_status otbx_partition_by_key(const int64_t *keys_dev, int64_t n,
                                  uint32_t nranks, int64_t *perm_dev,
                                  int64_t *counts_host, void *stream);

/* permutation gathers (dst[i] = src[perm[i]]) for applying the partition to
 * payload columns without leaving the native path */
otbx_status otbx_gather_i64(const int64_t *src, const int64_t *perm, int64_t n,
                            int64_t *dst, void *stream);
otbx_status otbx_gather_f64(const double *src, const int64_t *perm, int64_t n,
                            double *dst, void *stream);
otbx_status otbx_gather_i32(const int32_t *src, const int64_t *perm, int64_t n,
                            int32_t *dst, void *stream);
otbx_status otbx_gather_u8(const uint8_t *src, const int64_t *perm, int64_t n,
                           uint8_t *dst, void *stream);

/* Inner hash join on i64 keys: emits (build_idx, probe_idx) pairs in
 * arbitrary order (result-set parity; SQL imposes no order).
 * OVERFLOW CONTRACT: *npairs_dev always receives the TRUE match count; if
 * it exceeds cap_pairs the output arrays hold only a cap_pairs-bounded
 * subset and the caller MUST treat the result as overflowed (re-run with
 * cap_pairs >= *npairs_dev). The call itself still returns OTBX_OK — the
 * count lives on the device and is not visible to the host entry point;
 * this mirrors how the reference sizes hash tables from observed counts
 * (ExecHashTableInsert growth, nodeHash.c:1876) rather than failing
 * mid-scan. Pinned by tests/test_gpu_parity.py::test_join_overflow_contract. */
otbx_status otbx_join_i64_workspace_bytes(int64_t nb, int64_t np,
                                           size_t *bytes);
otbx_status otbx_join_i64(const int64_t *bkeys_dev, const uint8_t *bnull_dev,
                          int64_t nb,
                          const int64_t *pkeys_dev, const uint8_t *pnull_dev,
                          int64_t np, void *ws_dev, size_t ws_bytes,
                          int64_t *out_bidx_dev, int64_t *out_pidx_dev,
                          int64_t cap_pairs, int64_t *npairs_dev,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif

/*
 * otbx_groupagg.hip — the GPU GroupAggregate operator (otbx_group_agg):
 * several count / sum / min / max aggregates per run of equal keys over
 * sorted input, one output row per group, in key order. The AGG_SORTED /
 * AGG_PLAIN analog (executor/nodeAgg.c: agg_retrieve_direct :2249,
 * advance_aggregates :856). DESIGN.md §8k.
 *
 * Input is the permutation otbx_sort_perm produced for the GROUP BY keys.
 * Everything is stream-ordered; kernel boundaries are the only ordering
 * between workgroups, and no output value is ever touched by an atomic:
 *   k_ga_flags   — once per call. Per sorted position: gather the normalised
 *                  keys through perm (ss_norm, the sort's own key), compare
 *                  with the left neighbour (through LDS; only the first row
 *                  of a tile gathers perm[tile0-1]) → one start flag per
 *                  position and the tile's start count.
 *   k_ga_scan    — one workgroup: exclusive scan of the tile counts → the
 *                  group id of every tile's first start, and *ngroups.
 *   k_ga_first   — first_row[g] = row of the g-th start (only when wanted).
 *   k_ga_reduce  — once per aggregate, templated on the aggregate's operator.
 *                  GA_ITEMS consecutive positions per thread: gather the
 *                  value once, segmented scan in registers + one block scan.
 *                  A group that starts in the tile and ends before the
 *                  tile's last start is written to out[g] directly; the run
 *                  before the first start (head) and the run from the last
 *                  start on (tail) go to the tile's record.
 *   k_ga_fix     — once per aggregate, one workgroup: segmented scan over
 *                  the tile records, GA_FIX_THREADS per pass with a running
 *                  carry: tail ⊕ whole tiles ⊕ head for every group that
 *                  reaches a tile edge, written to out[g].
 * The reduction is SEGMENTED: a start drops the left operand, so no value of
 * one group ever reaches another. Every operator keeps position order (the
 * left operand is always the earlier rows), which is what the float MIN/MAX
 * tie rule needs. The operators are templated on the column's C type: the
 * kernels hold no run-time switch on the type code. ga_row is this unit's
 * own copy of otbx_window.hip's win_row; the neighbour compare is written for
 * this unit's LDS layout and shares only ss_norm with the window operator.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm: the normalised key */

#define GA_THREADS 256
#define GA_WAVES (GA_THREADS / WAVE)
#define GA_ITEMS 8
#define GA_TILE (GA_THREADS * GA_ITEMS)   /* 2048 positions per tile */
#define GA_FIX_THREADS 1024               /* tile records per pass of k_ga_fix */
#define GA_FIX_WAVES (GA_FIX_THREADS / WAVE)
#define GA_REC_BYTES 48                   /* head + tail of the widest state */

/* row of sorted position p; a perm entry outside [0, n) is clamped so that a
 * broken permutation can never index outside the columns */
__device__ __forceinline__ uint32_t ga_row(const int64_t *perm, uint32_t p,
                                           uint32_t n)
{
    if (!perm)
        return p;
    const int64_t r = perm[p];
    return r < 0 ? 0u : (r >= (int64_t)n ? n - 1 : (uint32_t)r);
}

/* ---- the aggregates' operators ----
 * S: the transition state; identity(): the state of no rows; load(): the
 * state of one row (identity under a NULL: the transition functions are
 * strict); comb(a, b): a = the earlier rows, b = the later ones; store():
 * the final value of group g. */

struct ga_st64 {            /* a 64-bit value + "saw a non-NULL input" */
    unsigned long long v;
    uint32_t has, pad_;
};
struct ga_st128 {
    unsigned long long lo;
    long long hi;
    uint32_t has, pad_;
};
static_assert(sizeof(ga_st64) == 16 && sizeof(ga_st128) == 24, "state layout");
static_assert(2 * sizeof(ga_st128) <= GA_REC_BYTES, "record size");

__device__ __forceinline__ bool ga_isnull(const otbx_aggcall &c, uint32_t row)
{
    return c.nulls && c.nulls[row];
}

/* count(*) (no mask) and count(col): int8inc / int8inc_any */
struct ga_op_count {
    typedef uint32_t S;
    static __device__ __forceinline__ S identity() { return 0u; }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        return (c.func == OTBX_AGG_COUNT && ga_isnull(c, row)) ? 0u : 1u;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        return a + b;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((int64_t *)c.out)[g] = (int64_t)s;
    }
};

/* sum(float8): float8pl; -0.0 is the identity of IEEE addition */
struct ga_op_sumf {
    typedef ga_st64 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.v = 0x8000000000000000ull;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        S s = identity();
        if (!ga_isnull(c, row)) {
            s.v = ((const unsigned long long *)c.col)[row];
            s.has = 1;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        S s;
        s.v = (unsigned long long)__double_as_longlong(
            __longlong_as_double((long long)a.v) +
            __longlong_as_double((long long)b.v));
        s.has = a.has | b.has;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((unsigned long long *)c.out)[g] = s.has ? s.v : 0ull;
        c.out_null[g] = s.has ? 0 : 1;
    }
};

/* sum(int4) and sum over uint8: int4_sum, an int64 that cannot overflow.
 * T is the column's C type: the kernels carry no run-time type switch */
template <typename T> struct ga_op_sumi {
    typedef ga_st64 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.v = 0;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        S s = identity();
        if (!ga_isnull(c, row)) {
            s.v = (unsigned long long)(long long)((const T *)c.col)[row];
            s.has = 1;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        S s;
        s.v = a.v + b.v;
        s.has = a.has | b.has;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((unsigned long long *)c.out)[g] = s.has ? s.v : 0ull;
        c.out_null[g] = s.has ? 0 : 1;
    }
};

/* sum(int8): int8_sum's Int128AggState, exact */
struct ga_op_sum128 {
    typedef ga_st128 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.lo = 0;
        s.hi = 0;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        S s = identity();
        if (!ga_isnull(c, row)) {
            const long long v = ((const int64_t *)c.col)[row];
            s.lo = (unsigned long long)v;
            s.hi = v < 0 ? -1ll : 0ll;
            s.has = 1;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        S s;
        s.lo = a.lo + b.lo;
        s.hi = (long long)((unsigned long long)a.hi + (unsigned long long)b.hi +
                           (s.lo < a.lo ? 1ull : 0ull));
        s.has = a.has | b.has;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((unsigned long long *)c.out)[g] = s.has ? s.lo : 0ull;
        c.out_hi[g] = s.has ? s.hi : 0ll;
        c.out_null[g] = s.has ? 0 : 1;
    }
};

/* min / max over I64, I32, U8 (T: the column's C type): int8smaller /
 * int8larger on the int64 value */
template <typename T, bool MAX> struct ga_op_mmi {
    typedef ga_st64 S;
    static __device__ __forceinline__ S identity()
    {
        return ga_op_sumi<T>::identity();
    }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        return ga_op_sumi<T>::load(c, row);
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        const long long x = (long long)a.v, y = (long long)b.v;
        const bool left = a.has && (!b.has || (MAX ? x > y : x < y));
        S s;
        s.v = left ? a.v : b.v;
        s.has = a.has | b.has;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((T *)c.out)[g] = s.has ? (T)(long long)s.v : (T)0;
        c.out_null[g] = s.has ? 0 : 1;
    }
};

/* min / max over F64: float8smaller / float8larger under float8_cmp_internal
 * (ss_norm_f64). The state is the chosen row's bit pattern; on a tie the
 * reference returns its second argument, so the later rows (b) win. */
template <bool MAX> struct ga_op_mmf {
    typedef ga_st64 S;
    static __device__ __forceinline__ S identity()
    {
        return ga_op_sumi<int32_t>::identity();
    }
    static __device__ __forceinline__ S load(const otbx_aggcall &c,
                                             uint32_t row)
    {
        S s = identity();
        if (!ga_isnull(c, row)) {
            s.v = ((const unsigned long long *)c.col)[row];
            s.has = 1;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        const unsigned long long x =
            ss_norm_f64(__longlong_as_double((long long)a.v));
        const unsigned long long y =
            ss_norm_f64(__longlong_as_double((long long)b.v));
        const bool left = a.has && (!b.has || (MAX ? x > y : x < y));
        S s;
        s.v = left ? a.v : b.v;
        s.has = a.has | b.has;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const otbx_aggcall &c,
                                                 uint32_t g, const S &s)
    {
        ((unsigned long long *)c.out)[g] = s.has ? s.v : 0ull;
        c.out_null[g] = s.has ? 0 : 1;
    }
};

/* ---- the segmented scan ---- */

/* the summary of a run of positions: ns = starts inside it, s = the state of
 * the rows from its last start on (of the whole run if ns == 0) */
template <typename S> struct ga_seg {
    uint32_t ns;
    S s;
};

template <typename Op>
__device__ __forceinline__ ga_seg<typename Op::S>
ga_seg_identity()
{
    ga_seg<typename Op::S> r;
    r.ns = 0;
    r.s = Op::identity();
    return r;
}

/* a is the run to the left of b */
template <typename Op>
__device__ __forceinline__ ga_seg<typename Op::S>
ga_seg_comb(const ga_seg<typename Op::S> &a, const ga_seg<typename Op::S> &b)
{
    ga_seg<typename Op::S> r;
    r.ns = a.ns + b.ns;
    r.s = b.ns ? b.s : Op::comb(a.s, b.s);
    return r;
}

template <typename T>
__device__ __forceinline__ T ga_shfl_up(const T &a, int o)
{
    static_assert(sizeof(T) % 4 == 0, "shuffled as 32-bit words");
    constexpr int W = (int)(sizeof(T) / 4);
    uint32_t w[W];
    __builtin_memcpy(w, &a, sizeof(T));
#pragma unroll
    for (int i = 0; i < W; i++)
        w[i] = (uint32_t)__shfl_up((int)w[i], o);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

/* block-wide exclusive ga_seg_comb scan of one summary per thread (NW
 * waves); *total gets the whole block. wtot: NW LDS entries, reusable after
 * return */
template <typename Op, int NW>
__device__ __forceinline__ ga_seg<typename Op::S>
ga_block_excl_scan(const ga_seg<typename Op::S> &v,
                   ga_seg<typename Op::S> *wtot,
                   ga_seg<typename Op::S> *total)
{
    typedef ga_seg<typename Op::S> E;
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    E incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const E t = ga_shfl_up(incl, o);
        if (lane >= o)
            incl = ga_seg_comb<Op>(t, incl);
    }
    if (lane == WAVE - 1)
        wtot[wid] = incl;
    __syncthreads();
    E pre = ga_seg_identity<Op>(), tot = ga_seg_identity<Op>();
    for (int w = 0; w < NW; w++) {
        const E s = wtot[w];
        if (w < wid)
            pre = ga_seg_comb<Op>(pre, s);
        tot = ga_seg_comb<Op>(tot, s);
    }
    __syncthreads();
    E excl = ga_shfl_up(incl, 1);
    if (lane == 0)
        excl = ga_seg_identity<Op>();
    *total = tot;
    return ga_seg_comb<Op>(pre, excl);
}

/* block-wide exclusive sum of one uint32 per thread; ws: NW LDS words */
template <int NW>
__device__ __forceinline__ uint32_t ga_block_excl_sum(uint32_t v, uint32_t *ws,
                                                      uint32_t *total)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o)
            incl += t;
    }
    if (lane == WAVE - 1)
        ws[wid] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (int w = 0; w < NW; w++) {
        const uint32_t s = ws[w];
        if (w < wid)
            pre += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

/* start bits of the GA_ITEMS positions from p0 on (p0 is a multiple of 8 and
 * the flag array is padded to whole tiles); positions past n read as 0 */
__device__ __forceinline__ uint32_t ga_load_flags(const uint8_t *flags,
                                                  uint32_t p0, uint32_t n)
{
    static_assert(GA_ITEMS == 8, "one 8-byte load");
    const uint2 w = *(const uint2 *)(flags + p0);
    uint32_t fb = 0;
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        const uint32_t b = ((i < 4 ? w.x : w.y) >> (8 * (i % 4))) & 1u;
        fb |= (p0 + i < n ? b : 0u) << i;
    }
    return fb;
}

/* ---- start flags + tile start counts ----
 * item i of thread t is position tile0 + i*GA_THREADS + t: the perm loads
 * and the flag stores are coalesced. The keys of one column go through LDS
 * so that every position finds its left neighbour's. */
__global__ __launch_bounds__(GA_THREADS) void
k_ga_flags(const otbx_sortspec spec, const int64_t *perm, const uint32_t n,
           uint8_t *flags, uint32_t *tilecnt)
{
    __shared__ unsigned long long sk[GA_TILE];
    __shared__ uint8_t snd[GA_TILE];
    __shared__ uint32_t wcnt[GA_WAVES];

    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile0 = blockIdx.x * (uint32_t)GA_TILE;

    uint32_t row[GA_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        const uint32_t p = tile0 + i * GA_THREADS + threadIdx.x;
        const bool v = p < n;
        valid |= (v ? 1u : 0u) << i;
        row[i] = v ? ga_row(perm, p, n) : 0u;
    }
    const bool edge = threadIdx.x == 0 && tile0 > 0;  /* reads perm[tile0-1] */
    const uint32_t lrow = edge ? ga_row(perm, tile0 - 1, n) : 0u;

    uint32_t sbits = 0;   /* item differs from its left neighbour */
#pragma unroll 1
    for (int c = 0; c < spec.nkeys; c++) {
        unsigned long long k[GA_ITEMS];
        uint32_t ndm = 0;
#pragma unroll
        for (int i = 0; i < GA_ITEMS; i++) {
            const uint32_t q = i * GA_THREADS + threadIdx.x;
            uint32_t nd = 0;
            k[i] = ((valid >> i) & 1u) ? ss_norm(spec.key[c], row[i], &nd)
                                       : 0ull;
            ndm |= nd << i;
            sk[q] = k[i];
            snd[q] = (uint8_t)nd;
        }
        unsigned long long k0left = 0;
        uint32_t nd0left = 0;
        if (edge)
            k0left = ss_norm(spec.key[c], lrow, &nd0left);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GA_ITEMS; i++) {
            const uint32_t q = i * GA_THREADS + threadIdx.x;
            unsigned long long lk = k0left;
            uint32_t lnd = nd0left;
            if (q > 0) {
                lk = sk[q - 1];
                lnd = snd[q - 1];
            }
            const bool d = lk != k[i] || lnd != ((ndm >> i) & 1u);
            sbits |= (d ? 1u : 0u) << i;
        }
        __syncthreads();
    }
    if (tile0 == 0 && threadIdx.x == 0)
        sbits |= 1u;                 /* position 0 starts the first group */
    sbits &= valid;

#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        if ((valid >> i) & 1u)
            flags[tile0 + i * GA_THREADS + threadIdx.x] =
                (uint8_t)((sbits >> i) & 1u);
    }
    uint32_t cnt = (uint32_t)__popc(sbits);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1)
        cnt += (uint32_t)__shfl_xor((int)cnt, o);
    if (lane == 0)
        wcnt[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < GA_WAVES; w++)
            t += wcnt[w];
        tilecnt[blockIdx.x] = t;
    }
}

/* ---- exclusive scan of the tile start counts: one workgroup, the running
 * sum in a register between passes ---- */
__global__ __launch_bounds__(GA_FIX_THREADS) void
k_ga_scan(const uint32_t *__restrict__ tilecnt, uint32_t *__restrict__ tilebase,
          const uint32_t ntiles, int64_t *ngroups)
{
    __shared__ uint32_t ws[GA_FIX_WAVES];
    uint32_t run = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += GA_FIX_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const uint32_t v = idx < ntiles ? tilecnt[idx] : 0u;
        uint32_t tot;
        const uint32_t ex = ga_block_excl_sum<GA_FIX_WAVES>(v, ws, &tot);
        if (idx < ntiles)
            tilebase[idx] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0)
        *ngroups = (int64_t)run;
}

/* ---- first_row[g] = the input row of the g-th start ----
 * thread t holds positions tile0 + t*GA_ITEMS .. +GA_ITEMS-1 */
__global__ __launch_bounds__(GA_THREADS) void
k_ga_first(const int64_t *perm, const uint32_t n,
           const uint8_t *__restrict__ flags,
           const uint32_t *__restrict__ tilebase, int64_t *first_row)
{
    __shared__ uint32_t ws[GA_WAVES];
    const uint32_t p0 =
        blockIdx.x * (uint32_t)GA_TILE + threadIdx.x * GA_ITEMS;
    const uint32_t fb = ga_load_flags(flags, p0, n);
    uint32_t tot;
    uint32_t g = tilebase[blockIdx.x] +
                 ga_block_excl_sum<GA_WAVES>((uint32_t)__popc(fb), ws, &tot);
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        if ((fb >> i) & 1u)
            first_row[g++] = (int64_t)ga_row(perm, p0 + i, n);
    }
}

/* ---- one aggregate, reduced per tile ----
 * thread t holds positions tile0 + t*GA_ITEMS .. +GA_ITEMS-1. The perm loads
 * are coalesced (striped) and the clamped rows go through LDS, rows padded
 * by one slot against bank conflicts, into the blocked layout. */
template <typename S> struct ga_rec {
    S head, tail;
};

template <typename Op>
__global__ __launch_bounds__(GA_THREADS) void
k_ga_reduce(const otbx_aggcall call, const int64_t *perm, const uint32_t n,
            const uint8_t *__restrict__ flags,
            const uint32_t *__restrict__ tilebase,
            ga_rec<typename Op::S> *recs)
{
    typedef typename Op::S S;
    typedef ga_seg<S> E;
    __shared__ E wtot[GA_WAVES];
    __shared__ uint32_t srow[GA_TILE + GA_THREADS];

    const uint32_t tile0 = blockIdx.x * (uint32_t)GA_TILE;
    const uint32_t p0 = tile0 + threadIdx.x * GA_ITEMS;

    uint32_t row[GA_ITEMS];
    if (perm) {
#pragma unroll
        for (int i = 0; i < GA_ITEMS; i++) {
            const uint32_t q = i * GA_THREADS + threadIdx.x;
            srow[q + q / GA_ITEMS] = tile0 + q < n ? ga_row(perm, tile0 + q, n)
                                                   : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GA_ITEMS; i++)
            row[i] = srow[threadIdx.x * (GA_ITEMS + 1) + i];
    } else {
#pragma unroll
        for (int i = 0; i < GA_ITEMS; i++)
            row[i] = p0 + i < n ? p0 + i : 0u;
    }
    const uint32_t fb = ga_load_flags(flags, p0, n);
    /* the start bit of the position after this thread's last one, if it is
     * in the same tile: a group that ends at the tile's last position is the
     * tile's tail */
    uint32_t fnext = 0;
    if (threadIdx.x < GA_THREADS - 1 && p0 + GA_ITEMS < n)
        fnext = flags[p0 + GA_ITEMS] & 1u;

    S x[GA_ITEMS];
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++)
        x[i] = p0 + i < n ? Op::load(call, row[i]) : Op::identity();

    /* the thread's own summary, the block scan, then the values */
    E a = ga_seg_identity<Op>();
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        if ((fb >> i) & 1u) {
            a.ns++;
            a.s = x[i];
        } else {
            a.s = Op::comb(a.s, x[i]);
        }
    }
    E tot;
    E r = ga_block_excl_scan<Op, GA_WAVES>(a, wtot, &tot);
    const uint32_t g0 = tilebase[blockIdx.x];
#pragma unroll
    for (int i = 0; i < GA_ITEMS; i++) {
        if ((fb >> i) & 1u) {
            r.ns++;
            r.s = x[i];
        } else {
            r.s = Op::comb(r.s, x[i]);
        }
        const uint32_t nxt = i + 1 < GA_ITEMS ? (fb >> (i + 1)) & 1u : fnext;
        if (nxt) {
            if (r.ns)
                Op::store(call, g0 + r.ns - 1, r.s);
            else
                recs[blockIdx.x].head = r.s;   /* began in an earlier tile */
        }
    }
    if (threadIdx.x == 0) {
        /* no start: the whole tile is head. A start at the tile's first
         * position: the head is empty. Otherwise the position before the
         * first start has written it above. */
        if (tot.ns == 0)
            recs[blockIdx.x].head = tot.s;
        else if (fb & 1u)
            recs[blockIdx.x].head = Op::identity();
        recs[blockIdx.x].tail = tot.s;
    }
}

/* ---- the groups that reach a tile edge ----
 * One workgroup. Per tile the scan element is (has a start, tail if so, else
 * the whole tile): the exclusive scan gives the state of the group open at
 * the tile's left edge, which ends at the tile's first start. The group open
 * at the right edge of the last tile is the last group. */
template <typename Op>
__global__ __launch_bounds__(GA_FIX_THREADS) void
k_ga_fix(const otbx_aggcall call, const uint32_t *__restrict__ tilecnt,
         const uint32_t *__restrict__ tilebase,
         const ga_rec<typename Op::S> *__restrict__ recs,
         const uint32_t ntiles, const int64_t *ngroups)
{
    typedef typename Op::S S;
    typedef ga_seg<S> E;
    __shared__ E wtot[GA_FIX_WAVES];

    E run = ga_seg_identity<Op>();
    for (uint32_t c0 = 0; c0 < ntiles; c0 += GA_FIX_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const bool in = idx < ntiles;
        const bool has = in && tilecnt[idx] > 0;
        const S head = in ? recs[idx].head : Op::identity();
        E v;
        v.ns = has ? 1u : 0u;
        v.s = has ? recs[idx].tail : head;
        E tot;
        const E ex = ga_block_excl_scan<Op, GA_FIX_WAVES>(v, wtot, &tot);
        const E open = ga_seg_comb<Op>(run, ex);
        if (has && idx > 0)
            Op::store(call, tilebase[idx] - 1, Op::comb(open.s, head));
        run = ga_seg_comb<Op>(run, tot);
    }
    if (threadIdx.x == 0) {
        const int64_t ng = *ngroups;
        if (ng > 0)
            Op::store(call, (uint32_t)(ng - 1), run.s);
    }
}

/* ---- n == 0: no group with keys, one empty group without (AGG_PLAIN) ---- */
__global__ void k_ga_empty(const otbx_aggcalls aggs, const int plain,
                           int64_t *first_row, int64_t *ngroups)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    *ngroups = plain ? 1 : 0;
    if (!plain)
        return;
    if (first_row)
        first_row[0] = -1;
    for (int a = 0; a < aggs.naggs; a++) {
        const otbx_aggcall &c = aggs.agg[a];
        if (c.func == OTBX_AGG_COUNT_STAR || c.func == OTBX_AGG_COUNT) {
            ((int64_t *)c.out)[0] = 0;
            continue;
        }
        c.out_null[0] = 1;
        if (c.func == OTBX_AGG_SUM || c.type == OTBX_SORT_I64 ||
            c.type == OTBX_SORT_F64)
            ((int64_t *)c.out)[0] = 0;     /* 0 and +0.0 share the bits */
        else if (c.type == OTBX_SORT_I32)
            ((int32_t *)c.out)[0] = 0;
        else
            ((uint8_t *)c.out)[0] = 0;
        if (c.out_hi)
            c.out_hi[0] = 0;
    }
}

/* ---- host side ---- */

struct ga_layout {
    size_t flags, tilecnt, tilebase, recs, total;
    uint32_t ntiles;
};

static void ga_plan_layout(int64_t n, ga_layout *L)
{
    L->ntiles = (uint32_t)((n + GA_TILE - 1) / GA_TILE);
    size_t o = 0;
    L->flags = o;    o += align256_sz((size_t)L->ntiles * GA_TILE);
    L->tilecnt = o;  o += align256_sz((size_t)L->ntiles * 4);
    L->tilebase = o; o += align256_sz((size_t)L->ntiles * 4);
    L->recs = o;     o += align256_sz((size_t)L->ntiles * GA_REC_BYTES);
    L->total = o;
}

template <typename Op>
static void ga_launch(const otbx_aggcall &call, const int64_t *perm,
                      uint32_t n, const ga_layout &L, char *w,
                      const int64_t *ngroups, hipStream_t s)
{
    static_assert(sizeof(ga_rec<typename Op::S>) <= GA_REC_BYTES, "record");
    const uint8_t *flags = (const uint8_t *)(w + L.flags);
    const uint32_t *tilecnt = (const uint32_t *)(w + L.tilecnt);
    const uint32_t *tilebase = (const uint32_t *)(w + L.tilebase);
    ga_rec<typename Op::S> *recs = (ga_rec<typename Op::S> *)(w + L.recs);
    hipLaunchKernelGGL(k_ga_reduce<Op>, dim3(L.ntiles), dim3(GA_THREADS), 0, s,
                       call, perm, n, flags, tilebase, recs);
    hipLaunchKernelGGL(k_ga_fix<Op>, dim3(1), dim3(GA_FIX_THREADS), 0, s, call,
                       tilecnt, tilebase, recs, L.ntiles, ngroups);
}

extern "C" {

otbx_status otbx_group_agg_workspace_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    ga_layout L;
    ga_plan_layout(n, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_group_agg(const otbx_sortspec *spec, const int64_t *perm_dev,
                           int64_t n, const otbx_aggcalls *aggs, void *ws_dev,
                           size_t ws_bytes, int64_t *first_row_dev,
                           int64_t *ngroups_dev, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!spec || !aggs || !ngroups_dev)
        return OTBX_ERR_INVALID;
    if (spec->nkeys < 0 || spec->nkeys > OTBX_MAX_KEYS)
        return OTBX_ERR_INVALID;
    if (aggs->naggs < 0 || aggs->naggs > OTBX_MAX_AGGS)
        return OTBX_ERR_INVALID;
    if (n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    for (int c = 0; c < spec->nkeys; c++) {
        const otbx_sortkey *k = &spec->key[c];
        if (k->type < OTBX_SORT_I64 || k->type > OTBX_SORT_U8)
            return OTBX_ERR_INVALID;
        if (k->flags & ~(OTBX_SORT_DESC | OTBX_SORT_NULLS_FIRST))
            return OTBX_ERR_INVALID;
        if (n > 0 && !k->col)
            return OTBX_ERR_INVALID;
    }
    for (int a = 0; a < aggs->naggs; a++) {
        const otbx_aggcall *c = &aggs->agg[a];
        if (c->func < OTBX_AGG_COUNT_STAR || c->func > OTBX_AGG_MAX)
            return OTBX_ERR_INVALID;
        if (c->type < OTBX_SORT_I64 || c->type > OTBX_SORT_U8)
            return OTBX_ERR_INVALID;
        const bool count =
            c->func == OTBX_AGG_COUNT_STAR || c->func == OTBX_AGG_COUNT;
        if (!c->out)
            return OTBX_ERR_INVALID;
        if (!count && n > 0 && !c->col)
            return OTBX_ERR_INVALID;
        if (count ? c->out_null != nullptr : c->out_null == nullptr)
            return OTBX_ERR_INVALID;
        const bool wide = c->func == OTBX_AGG_SUM && c->type == OTBX_SORT_I64;
        if (wide ? c->out_hi == nullptr : c->out_hi != nullptr)
            return OTBX_ERR_INVALID;
    }
    if (aggs->naggs == 0 && !first_row_dev)
        return OTBX_ERR_INVALID;
    ga_layout L;
    ga_plan_layout(n, &L);
    /* the kernels read the workspace with 8-byte vectors */
    if (ws_bytes < L.total || (L.total > 0 && !ws_dev) ||
        ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(k_ga_empty, dim3(1), dim3(1), 0, s, *aggs,
                           spec->nkeys == 0 ? 1 : 0, first_row_dev,
                           ngroups_dev);
        HIP_CHECK(hipGetLastError());
        return OTBX_OK;
    }

    char *w = (char *)ws_dev;
    uint8_t *flags = (uint8_t *)(w + L.flags);
    uint32_t *tilecnt = (uint32_t *)(w + L.tilecnt);
    uint32_t *tilebase = (uint32_t *)(w + L.tilebase);
    const uint32_t un = (uint32_t)n;

    hipLaunchKernelGGL(k_ga_flags, dim3(L.ntiles), dim3(GA_THREADS), 0, s,
                       *spec, perm_dev, un, flags, tilecnt);
    hipLaunchKernelGGL(k_ga_scan, dim3(1), dim3(GA_FIX_THREADS), 0, s, tilecnt,
                       tilebase, L.ntiles, ngroups_dev);
    if (first_row_dev)
        hipLaunchKernelGGL(k_ga_first, dim3(L.ntiles), dim3(GA_THREADS), 0, s,
                           perm_dev, un, flags, tilebase, first_row_dev);
#define GA_LAUNCH(...) \
    ga_launch<__VA_ARGS__>(c, perm_dev, un, L, w, ngroups_dev, s)
#define GA_LAUNCH_MM(MAX)                                  \
    do {                                                   \
        if (c.type == OTBX_SORT_F64)                       \
            GA_LAUNCH(ga_op_mmf<MAX>);                     \
        else if (c.type == OTBX_SORT_I64)                  \
            GA_LAUNCH(ga_op_mmi<int64_t, MAX>);            \
        else if (c.type == OTBX_SORT_I32)                  \
            GA_LAUNCH(ga_op_mmi<int32_t, MAX>);            \
        else                                               \
            GA_LAUNCH(ga_op_mmi<uint8_t, MAX>);            \
    } while (0)
    for (int a = 0; a < aggs->naggs; a++) {
        const otbx_aggcall &c = aggs->agg[a];
        switch (c.func) {
        case OTBX_AGG_COUNT_STAR:
        case OTBX_AGG_COUNT:
            GA_LAUNCH(ga_op_count);
            break;
        case OTBX_AGG_SUM:
            if (c.type == OTBX_SORT_F64)
                GA_LAUNCH(ga_op_sumf);
            else if (c.type == OTBX_SORT_I64)
                GA_LAUNCH(ga_op_sum128);
            else if (c.type == OTBX_SORT_I32)
                GA_LAUNCH(ga_op_sumi<int32_t>);
            else
                GA_LAUNCH(ga_op_sumi<uint8_t>);
            break;
        case OTBX_AGG_MIN:
            GA_LAUNCH_MM(false);
            break;
        default:
            GA_LAUNCH_MM(true);
            break;
        }
    }
#undef GA_LAUNCH_MM
#undef GA_LAUNCH
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/*
 * otbx_ordagg.hip — DISTINCT and ordered-set aggregates over sorted input
 * (otbx_ordered_agg): count(DISTINCT x), sum(DISTINCT x), percentile_disc,
 * percentile_cont and mode() per run of equal GROUP BY keys. The analog of
 * process_ordered_aggregate_single (executor/nodeAgg.c:888) and of
 * utils/adt/orderedsetaggs.c. DESIGN.md §8o.
 *
 * Input is the permutation otbx_sort_perm produced for (GROUP BY keys, x):
 * inside a group the argument is sorted, its NULLs sit together at one end,
 * and equal values are adjacent. Every aggregate is then a segmented
 * reduction over one byte of flags per position. Everything is
 * stream-ordered; kernel boundaries are the only ordering between
 * workgroups, and no output value is ever touched by an atomic:
 *   k_oa_flags   — once per call. Per sorted position: gather the normalised
 *                  keys through perm (ss_norm), compare with the left
 *                  neighbour through LDS → OA_F_GROUP (a GROUP BY key
 *                  differs), OA_F_RUN (group start, or the argument
 *                  differs), OA_F_NULL (the argument is NULL); and the
 *                  tile's group-start count.
 *   k_oa_scan    — one workgroup: exclusive scan of the tile counts.
 *   k_oa_first   — first_row[g] (only when wanted).
 *   k_oa_reduce  — once per KIND of aggregate, templated on its operator:
 *                  oa_op_stats  (N, distinct runs, first non-NULL position)
 *                               reads only the flags; its store() finishes
 *                               COUNT_DISTINCT and every percentile of the
 *                               call list with at most two value gathers per
 *                               GROUP;
 *                  oa_op_mode   the associative longest-run state over the
 *                               flags; one gather per group;
 *                  oa_op_sum*   the segmented sum, gathering a value only
 *                               where a run of non-NULL values starts.
 *   k_oa_fix     — once per kind, one workgroup: the groups that reach a
 *                  tile edge, from the tile records.
 * The segmented scan, the records and the fix-up are this unit's own copy of
 * otbx_groupagg.hip's scheme (as that unit copied win_row); the two units
 * share only ss_norm.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm: the normalised key */

#define OA_THREADS 256
#define OA_WAVES (OA_THREADS / WAVE)
#define OA_ITEMS 8
#define OA_TILE (OA_THREADS * OA_ITEMS)   /* 2048 positions per tile */
#define OA_FIX_THREADS 1024               /* tile records per pass of k_oa_fix */
#define OA_FIX_WAVES (OA_FIX_THREADS / WAVE)
#define OA_REC_BYTES 48                   /* head + tail of the widest state */

#define OA_F_GROUP 1u   /* first position of a group */
#define OA_F_RUN 2u     /* first position of a run of equal arguments */
#define OA_F_NULL 4u    /* the argument is NULL */
#define OA_NONE 0xffffffffu

/* what every operator needs: the argument column (the last sort key), the
 * permutation and the call list */
struct oa_ctx {
    otbx_sortkey arg;
    const int64_t *perm;
    uint32_t n, pad_;
    otbx_oaggcalls calls;
};

/* row of sorted position p; a perm entry outside [0, n) is clamped so that a
 * broken permutation can never index outside the columns */
__device__ __forceinline__ uint32_t oa_row(const int64_t *perm, uint32_t p,
                                           uint32_t n)
{
    if (!perm)
        return p;
    const int64_t r = perm[p];
    return r < 0 ? 0u : (r >= (int64_t)n ? n - 1 : (uint32_t)r);
}

/* the argument of position p (clamped into [0, n)): its bits, zero-extended */
__device__ __forceinline__ unsigned long long oa_arg_bits(const oa_ctx &x,
                                                          uint32_t p)
{
    const uint32_t row = oa_row(x.perm, p < x.n ? p : x.n - 1, x.n);
    switch (x.arg.type) {
    case OTBX_SORT_I64:
    case OTBX_SORT_F64:
        return ((const unsigned long long *)x.arg.col)[row];
    case OTBX_SORT_I32:
        return (unsigned long long)((const uint32_t *)x.arg.col)[row];
    default:
        return (unsigned long long)((const uint8_t *)x.arg.col)[row];
    }
}

/* ... as a double: float8 as it is, the integers as i8tod / i4tod convert */
__device__ __forceinline__ double oa_arg_f64(const oa_ctx &x, uint32_t p)
{
    const unsigned long long b = oa_arg_bits(x, p);
    switch (x.arg.type) {
    case OTBX_SORT_F64:
        return __longlong_as_double((long long)b);
    case OTBX_SORT_I64:
        return (double)(long long)b;
    case OTBX_SORT_I32:
        return (double)(int32_t)(uint32_t)b;
    default:
        return (double)(uint32_t)b;
    }
}

/* a result of the argument's own type */
__device__ __forceinline__ void oa_put(const oa_ctx &x, const otbx_oaggcall &c,
                                       uint32_t g, unsigned long long bits,
                                       bool isnull)
{
    if (isnull)
        bits = 0;
    switch (x.arg.type) {
    case OTBX_SORT_I64:
    case OTBX_SORT_F64:
        ((unsigned long long *)c.out)[g] = bits;
        break;
    case OTBX_SORT_I32:
        ((uint32_t *)c.out)[g] = (uint32_t)bits;
        break;
    default:
        ((uint8_t *)c.out)[g] = (uint8_t)bits;
        break;
    }
    c.out_null[g] = isnull ? 1 : 0;
}

/* ---- the operators ----
 * S: the state; identity(): the state of no rows; load(): the state of one
 * position from its flag byte (identity under a NULL: the transition
 * functions are strict); comb(a, b): a = the earlier positions, b = the
 * later ones; store(): every result of group g this operator serves. */

/* N, the number of runs, and the first non-NULL position: COUNT_DISTINCT and
 * the percentiles. Reads nothing but the flags. */
struct oa_st_stats {
    uint32_t n, nd, lo, pad_;
};

struct oa_op_stats {
    typedef oa_st_stats S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.n = 0;
        s.nd = 0;
        s.lo = OA_NONE;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const oa_ctx &, uint32_t p,
                                             uint32_t f)
    {
        S s = identity();
        if (!(f & OA_F_NULL)) {
            s.n = 1;
            s.nd = (f & OA_F_RUN) ? 1u : 0u;
            s.lo = p;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        S s;
        s.n = a.n + b.n;
        s.nd = a.nd + b.nd;
        s.lo = a.lo < b.lo ? a.lo : b.lo;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ void store(const oa_ctx &x, uint32_t g,
                                                 const S &s)
    {
        for (int a = 0; a < x.calls.ncalls; a++) {
            const otbx_oaggcall &c = x.calls.call[a];
            if (c.func == OTBX_OAGG_COUNT_DISTINCT) {
                ((int64_t *)c.out)[g] = (int64_t)s.nd;
            } else if (c.func == OTBX_OAGG_PERCENTILE_DISC) {
                /* the smallest K with K/N >= p (orderedsetaggs.c:468) */
                unsigned long long bits = 0;
                if (s.n) {
                    long long k = (long long)ceil(c.fraction * (double)s.n);
                    k = k < 1 ? 1 : (k > (long long)s.n ? (long long)s.n : k);
                    bits = oa_arg_bits(x, s.lo + (uint32_t)(k - 1));
                }
                oa_put(x, c, g, bits, s.n == 0);
            } else if (c.func == OTBX_OAGG_PERCENTILE_CONT) {
                /* percentile_cont_final_common :568-594, float8_lerp :496;
                 * the intrinsics keep the products and sums unfused */
                double r = 0.0;
                if (s.n) {
                    const double t = __dmul_rn(c.fraction, (double)(s.n - 1));
                    const double fl = floor(t), ce = ceil(t);
                    uint32_t i0 = (uint32_t)(long long)fl;
                    if (i0 > s.n - 1)
                        i0 = s.n - 1;
                    const double v0 = oa_arg_f64(x, s.lo + i0);
                    if (fl == ce || i0 + 1 > s.n - 1) {
                        r = v0;
                    } else {
                        const double v1 = oa_arg_f64(x, s.lo + i0 + 1);
                        const double prop = __dsub_rn(t, fl);
                        r = __dadd_rn(v0, __dmul_rn(prop, __dsub_rn(v1, v0)));
                    }
                }
                ((double *)c.out)[g] = r;
                c.out_null[g] = s.n ? 0 : 1;
            }
        }
    }
};

/* mode(): the longest run of equal non-NULL arguments, the earliest among
 * equals (mode_final :1090 takes a new mode only on ">"). The state of a
 * range of positions: lead = positions before its first run start (they
 * continue a run that began to the left), (tstart, tlen) = its last run,
 * (bstart, blen) = the best run that starts inside it, the last one
 * included. tlen == 0: no run starts in the range. NULL positions are the
 * identity: they sit at one end of the group and never split a run. */
struct oa_st_mode {
    uint32_t lead, tstart, tlen, bstart, blen, pad_;
};

struct oa_op_mode {
    typedef oa_st_mode S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.lead = s.tstart = s.tlen = s.bstart = s.blen = s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const oa_ctx &, uint32_t p,
                                             uint32_t f)
    {
        S s = identity();
        if (f & OA_F_NULL)
            return s;
        if (f & OA_F_RUN) {
            s.tstart = s.bstart = p;
            s.tlen = s.blen = 1;
        } else {
            s.lead = 1;
        }
        return s;
    }
    static __device__ __forceinline__ S comb(const S &a, const S &b)
    {
        S r;
        r.pad_ = 0;
        /* a's last run, grown by the positions of b that continue it */
        const uint32_t mid = a.tlen ? a.tlen + b.lead : 0u;
        r.lead = a.tlen ? a.lead : a.lead + b.lead;
        r.bstart = a.bstart;
        r.blen = a.blen;
        if (mid > r.blen) {
            r.bstart = a.tstart;
            r.blen = mid;
        }
        if (b.blen > r.blen) {
            r.bstart = b.bstart;
            r.blen = b.blen;
        }
        r.tstart = b.tlen ? b.tstart : a.tstart;
        r.tlen = b.tlen ? b.tlen : mid;
        return r;
    }
    static __device__ __forceinline__ void store(const oa_ctx &x, uint32_t g,
                                                 const S &s)
    {
        const unsigned long long bits = s.blen ? oa_arg_bits(x, s.bstart) : 0;
        for (int a = 0; a < x.calls.ncalls; a++) {
            const otbx_oaggcall &c = x.calls.call[a];
            if (c.func == OTBX_OAGG_MODE)
                oa_put(x, c, g, bits, s.blen == 0);
        }
    }
};

/* sum(DISTINCT): otbx_group_agg's SUM operators, fed only by the first
 * position of each run of non-NULL arguments */
struct oa_st64 {
    unsigned long long v;
    uint32_t has, pad_;
};
struct oa_st128 {
    unsigned long long lo;
    long long hi;
    uint32_t has, pad_;
};
static_assert(sizeof(oa_st64) == 16 && sizeof(oa_st128) == 24 &&
                  sizeof(oa_st_stats) == 16 && sizeof(oa_st_mode) == 24,
              "state layout");
static_assert(2 * sizeof(oa_st128) <= OA_REC_BYTES, "record size");

__device__ __forceinline__ bool oa_counts(uint32_t f)
{
    return (f & (OA_F_RUN | OA_F_NULL)) == OA_F_RUN;
}

/* float8pl; -0.0 is the identity of IEEE addition */
struct oa_op_sumf {
    typedef oa_st64 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.v = 0x8000000000000000ull;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const oa_ctx &x, uint32_t p,
                                             uint32_t f)
    {
        S s = identity();
        if (oa_counts(f)) {
            s.v = ((const unsigned long long *)
                       x.arg.col)[oa_row(x.perm, p, x.n)];
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
    static __device__ __forceinline__ void store(const oa_ctx &x, uint32_t g,
                                                 const S &s)
    {
        for (int a = 0; a < x.calls.ncalls; a++) {
            const otbx_oaggcall &c = x.calls.call[a];
            if (c.func != OTBX_OAGG_SUM_DISTINCT)
                continue;
            ((unsigned long long *)c.out)[g] = s.has ? s.v : 0ull;
            c.out_null[g] = s.has ? 0 : 1;
        }
    }
};

/* int4_sum over I32 / U8 (T: the column's C type): an int64 that cannot
 * overflow */
template <typename T> struct oa_op_sumi {
    typedef oa_st64 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.v = 0;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const oa_ctx &x, uint32_t p,
                                             uint32_t f)
    {
        S s = identity();
        if (oa_counts(f)) {
            s.v = (unsigned long long)(long long)((const T *)
                      x.arg.col)[oa_row(x.perm, p, x.n)];
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
    static __device__ __forceinline__ void store(const oa_ctx &x, uint32_t g,
                                                 const S &s)
    {
        oa_op_sumf::store(x, g, s);
    }
};

/* int8_sum's Int128AggState, exact */
struct oa_op_sum128 {
    typedef oa_st128 S;
    static __device__ __forceinline__ S identity()
    {
        S s;
        s.lo = 0;
        s.hi = 0;
        s.has = 0;
        s.pad_ = 0;
        return s;
    }
    static __device__ __forceinline__ S load(const oa_ctx &x, uint32_t p,
                                             uint32_t f)
    {
        S s = identity();
        if (oa_counts(f)) {
            const long long v =
                ((const int64_t *)x.arg.col)[oa_row(x.perm, p, x.n)];
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
    static __device__ __forceinline__ void store(const oa_ctx &x, uint32_t g,
                                                 const S &s)
    {
        for (int a = 0; a < x.calls.ncalls; a++) {
            const otbx_oaggcall &c = x.calls.call[a];
            if (c.func != OTBX_OAGG_SUM_DISTINCT)
                continue;
            ((unsigned long long *)c.out)[g] = s.has ? s.lo : 0ull;
            c.out_hi[g] = s.has ? s.hi : 0ll;
            c.out_null[g] = s.has ? 0 : 1;
        }
    }
};

/* ---- the segmented scan ---- */

/* the summary of a range of positions: ns = group starts inside it, s = the
 * state of the positions from its last start on (of the whole range if
 * ns == 0) */
template <typename S> struct oa_seg {
    uint32_t ns;
    S s;
};

template <typename Op>
__device__ __forceinline__ oa_seg<typename Op::S> oa_seg_identity()
{
    oa_seg<typename Op::S> r;
    r.ns = 0;
    r.s = Op::identity();
    return r;
}

/* a is the range to the left of b */
template <typename Op>
__device__ __forceinline__ oa_seg<typename Op::S>
oa_seg_comb(const oa_seg<typename Op::S> &a, const oa_seg<typename Op::S> &b)
{
    oa_seg<typename Op::S> r;
    r.ns = a.ns + b.ns;
    r.s = b.ns ? b.s : Op::comb(a.s, b.s);
    return r;
}

template <typename T>
__device__ __forceinline__ T oa_shfl_up(const T &a, int o)
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

/* block-wide exclusive oa_seg_comb scan of one summary per thread (NW
 * waves); *total gets the whole block. wtot: NW LDS entries, reusable after
 * return */
template <typename Op, int NW>
__device__ __forceinline__ oa_seg<typename Op::S>
oa_block_excl_scan(const oa_seg<typename Op::S> &v,
                   oa_seg<typename Op::S> *wtot,
                   oa_seg<typename Op::S> *total)
{
    typedef oa_seg<typename Op::S> E;
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    E incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const E t = oa_shfl_up(incl, o);
        if (lane >= o)
            incl = oa_seg_comb<Op>(t, incl);
    }
    if (lane == WAVE - 1)
        wtot[wid] = incl;
    __syncthreads();
    E pre = oa_seg_identity<Op>(), tot = oa_seg_identity<Op>();
    for (int w = 0; w < NW; w++) {
        const E s = wtot[w];
        if (w < wid)
            pre = oa_seg_comb<Op>(pre, s);
        tot = oa_seg_comb<Op>(tot, s);
    }
    __syncthreads();
    E excl = oa_shfl_up(incl, 1);
    if (lane == 0)
        excl = oa_seg_identity<Op>();
    *total = tot;
    return oa_seg_comb<Op>(pre, excl);
}

/* block-wide exclusive sum of one uint32 per thread; ws: NW LDS words */
template <int NW>
__device__ __forceinline__ uint32_t oa_block_excl_sum(uint32_t v, uint32_t *ws,
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

/* the flag bytes of the OA_ITEMS positions from p0 on (p0 is a multiple of 8
 * and the flag array is padded to whole tiles); positions past n read as 0 */
__device__ __forceinline__ void oa_load_flags(const uint8_t *flags,
                                              uint32_t p0, uint32_t n,
                                              uint32_t f[OA_ITEMS])
{
    static_assert(OA_ITEMS == 8, "one 8-byte load");
    const uint2 w = *(const uint2 *)(flags + p0);
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        const uint32_t b = ((i < 4 ? w.x : w.y) >> (8 * (i % 4))) & 0xffu;
        f[i] = p0 + i < n ? b : 0u;
    }
}

/* ---- the flags + tile group-start counts ----
 * item i of thread t is position tile0 + i*OA_THREADS + t: the perm loads
 * and the flag stores are coalesced. The keys of one column go through LDS
 * so that every position finds its left neighbour's. Keys 0..ngroup-1 are
 * the GROUP BY keys, key ngroup is the argument. */
__global__ __launch_bounds__(OA_THREADS) void
k_oa_flags(const otbx_sortspec spec, const int ngroup, const int64_t *perm,
           const uint32_t n, uint8_t *flags, uint32_t *tilecnt)
{
    __shared__ unsigned long long sk[OA_TILE];
    __shared__ uint8_t snd[OA_TILE];
    __shared__ uint32_t wcnt[OA_WAVES];

    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile0 = blockIdx.x * (uint32_t)OA_TILE;

    uint32_t row[OA_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        const uint32_t p = tile0 + i * OA_THREADS + threadIdx.x;
        const bool v = p < n;
        valid |= (v ? 1u : 0u) << i;
        row[i] = v ? oa_row(perm, p, n) : 0u;
    }
    const bool edge = threadIdx.x == 0 && tile0 > 0;  /* reads perm[tile0-1] */
    const uint32_t lrow = edge ? oa_row(perm, tile0 - 1, n) : 0u;

    uint32_t gbits = 0;   /* a GROUP BY key differs from the left neighbour */
    uint32_t abits = 0;   /* the argument differs */
    uint32_t nbits = 0;   /* the argument is NULL */
#pragma unroll 1
    for (int c = 0; c <= ngroup; c++) {
        unsigned long long k[OA_ITEMS];
        uint32_t ndm = 0;
#pragma unroll
        for (int i = 0; i < OA_ITEMS; i++) {
            const uint32_t q = i * OA_THREADS + threadIdx.x;
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
        uint32_t dbits = 0;
#pragma unroll
        for (int i = 0; i < OA_ITEMS; i++) {
            const uint32_t q = i * OA_THREADS + threadIdx.x;
            unsigned long long lk = k0left;
            uint32_t lnd = nd0left;
            if (q > 0) {
                lk = sk[q - 1];
                lnd = snd[q - 1];
            }
            const bool d = lk != k[i] || lnd != ((ndm >> i) & 1u);
            dbits |= (d ? 1u : 0u) << i;
        }
        if (c < ngroup) {
            gbits |= dbits;
        } else {
            abits = dbits;
            /* the null digit of a NULL: 0 under NULLS FIRST, else 1 */
            nbits = (spec.key[c].flags & OTBX_SORT_NULLS_FIRST) ? ~ndm : ndm;
        }
        __syncthreads();
    }
    if (tile0 == 0 && threadIdx.x == 0)
        gbits |= 1u;                 /* position 0 starts the first group */
    gbits &= valid;
    abits = (abits | gbits) & valid;
    nbits &= valid;

#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        if ((valid >> i) & 1u)
            flags[tile0 + i * OA_THREADS + threadIdx.x] =
                (uint8_t)((((gbits >> i) & 1u) ? OA_F_GROUP : 0u) |
                          (((abits >> i) & 1u) ? OA_F_RUN : 0u) |
                          (((nbits >> i) & 1u) ? OA_F_NULL : 0u));
    }
    uint32_t cnt = (uint32_t)__popc(gbits);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1)
        cnt += (uint32_t)__shfl_xor((int)cnt, o);
    if (lane == 0)
        wcnt[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < OA_WAVES; w++)
            t += wcnt[w];
        tilecnt[blockIdx.x] = t;
    }
}

/* ---- exclusive scan of the tile group-start counts: one workgroup, the
 * running sum in a register between passes ---- */
__global__ __launch_bounds__(OA_FIX_THREADS) void
k_oa_scan(const uint32_t *__restrict__ tilecnt, uint32_t *__restrict__ tilebase,
          const uint32_t ntiles, int64_t *ngroups)
{
    __shared__ uint32_t ws[OA_FIX_WAVES];
    uint32_t run = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += OA_FIX_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const uint32_t v = idx < ntiles ? tilecnt[idx] : 0u;
        uint32_t tot;
        const uint32_t ex = oa_block_excl_sum<OA_FIX_WAVES>(v, ws, &tot);
        if (idx < ntiles)
            tilebase[idx] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0)
        *ngroups = (int64_t)run;
}

/* ---- first_row[g] = the input row of the g-th group start ----
 * thread t holds positions tile0 + t*OA_ITEMS .. +OA_ITEMS-1 */
__global__ __launch_bounds__(OA_THREADS) void
k_oa_first(const int64_t *perm, const uint32_t n,
           const uint8_t *__restrict__ flags,
           const uint32_t *__restrict__ tilebase, int64_t *first_row)
{
    __shared__ uint32_t ws[OA_WAVES];
    const uint32_t p0 =
        blockIdx.x * (uint32_t)OA_TILE + threadIdx.x * OA_ITEMS;
    uint32_t f[OA_ITEMS];
    oa_load_flags(flags, p0, n, f);
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++)
        cnt += f[i] & OA_F_GROUP;
    uint32_t tot;
    uint32_t g = tilebase[blockIdx.x] +
                 oa_block_excl_sum<OA_WAVES>(cnt, ws, &tot);
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        if (f[i] & OA_F_GROUP)
            first_row[g++] = (int64_t)oa_row(perm, p0 + i, n);
    }
}

/* ---- one kind of aggregate, reduced per tile ----
 * thread t holds positions tile0 + t*OA_ITEMS .. +OA_ITEMS-1. A group that
 * starts in the tile and ends before the tile's last start is stored
 * directly; the positions before the first start (head) and those from the
 * last start on (tail) go to the tile's record. */
template <typename S> struct oa_rec {
    S head, tail;
};

template <typename Op>
__global__ __launch_bounds__(OA_THREADS) void
k_oa_reduce(const oa_ctx ctx, const uint8_t *__restrict__ flags,
            const uint32_t *__restrict__ tilebase,
            oa_rec<typename Op::S> *recs)
{
    typedef typename Op::S S;
    typedef oa_seg<S> E;
    __shared__ E wtot[OA_WAVES];

    const uint32_t n = ctx.n;
    const uint32_t tile0 = blockIdx.x * (uint32_t)OA_TILE;
    const uint32_t p0 = tile0 + threadIdx.x * OA_ITEMS;

    uint32_t f[OA_ITEMS];
    oa_load_flags(flags, p0, n, f);
    /* the group bit of the position after this thread's last one, if it is
     * in the same tile: a group that ends at the tile's last position is the
     * tile's tail */
    uint32_t fnext = 0;
    if (threadIdx.x < OA_THREADS - 1 && p0 + OA_ITEMS < n)
        fnext = flags[p0 + OA_ITEMS] & OA_F_GROUP;

    S x[OA_ITEMS];
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++)
        x[i] = p0 + i < n ? Op::load(ctx, p0 + i, f[i]) : Op::identity();

    /* the thread's own summary, the block scan, then the values */
    E a = oa_seg_identity<Op>();
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        if (f[i] & OA_F_GROUP) {
            a.ns++;
            a.s = x[i];
        } else {
            a.s = Op::comb(a.s, x[i]);
        }
    }
    E tot;
    E r = oa_block_excl_scan<Op, OA_WAVES>(a, wtot, &tot);
    const uint32_t g0 = tilebase[blockIdx.x];
#pragma unroll
    for (int i = 0; i < OA_ITEMS; i++) {
        if (f[i] & OA_F_GROUP) {
            r.ns++;
            r.s = x[i];
        } else {
            r.s = Op::comb(r.s, x[i]);
        }
        const uint32_t nxt =
            i + 1 < OA_ITEMS ? (f[i + 1] & OA_F_GROUP) : fnext;
        if (nxt) {
            if (r.ns)
                Op::store(ctx, g0 + r.ns - 1, r.s);
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
        else if (f[0] & OA_F_GROUP)
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
__global__ __launch_bounds__(OA_FIX_THREADS) void
k_oa_fix(const oa_ctx ctx, const uint32_t *__restrict__ tilecnt,
         const uint32_t *__restrict__ tilebase,
         const oa_rec<typename Op::S> *__restrict__ recs,
         const uint32_t ntiles, const int64_t *ngroups)
{
    typedef typename Op::S S;
    typedef oa_seg<S> E;
    __shared__ E wtot[OA_FIX_WAVES];

    E run = oa_seg_identity<Op>();
    for (uint32_t c0 = 0; c0 < ntiles; c0 += OA_FIX_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const bool in = idx < ntiles;
        const bool has = in && tilecnt[idx] > 0;
        const S head = in ? recs[idx].head : Op::identity();
        E v;
        v.ns = has ? 1u : 0u;
        v.s = has ? recs[idx].tail : head;
        E tot;
        const E ex = oa_block_excl_scan<Op, OA_FIX_WAVES>(v, wtot, &tot);
        const E open = oa_seg_comb<Op>(run, ex);
        if (has && idx > 0)
            Op::store(ctx, tilebase[idx] - 1, Op::comb(open.s, head));
        run = oa_seg_comb<Op>(run, tot);
    }
    if (threadIdx.x == 0) {
        const int64_t ng = *ngroups;
        if (ng > 0)
            Op::store(ctx, (uint32_t)(ng - 1), run.s);
    }
}

/* ---- n == 0: no group with keys, one empty group without (AGG_PLAIN) ---- */
__global__ void k_oa_empty(const otbx_oaggcalls calls, const int argtype,
                           const int plain, int64_t *first_row,
                           int64_t *ngroups)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    *ngroups = plain ? 1 : 0;
    if (!plain)
        return;
    if (first_row)
        first_row[0] = -1;
    for (int a = 0; a < calls.ncalls; a++) {
        const otbx_oaggcall &c = calls.call[a];
        if (c.func == OTBX_OAGG_COUNT_DISTINCT) {
            ((int64_t *)c.out)[0] = 0;
            continue;
        }
        c.out_null[0] = 1;
        const bool own = c.func == OTBX_OAGG_PERCENTILE_DISC ||
                         c.func == OTBX_OAGG_MODE;
        if (own && argtype == OTBX_SORT_I32)
            ((int32_t *)c.out)[0] = 0;
        else if (own && argtype == OTBX_SORT_U8)
            ((uint8_t *)c.out)[0] = 0;
        else
            ((int64_t *)c.out)[0] = 0;     /* 0 and +0.0 share the bits */
        if (c.out_hi)
            c.out_hi[0] = 0;
    }
}

/* ---- host side ---- */

struct oa_layout {
    size_t flags, tilecnt, tilebase, recs, total;
    uint32_t ntiles;
};

static void oa_plan_layout(int64_t n, int32_t ncalls, oa_layout *L)
{
    L->ntiles = (uint32_t)((n + OA_TILE - 1) / OA_TILE);
    size_t o = 0;
    L->flags = o;    o += align256_sz((size_t)L->ntiles * OA_TILE);
    L->tilecnt = o;  o += align256_sz((size_t)L->ntiles * 4);
    L->tilebase = o; o += align256_sz((size_t)L->ntiles * 4);
    L->recs = o;
    if (ncalls > 0)
        o += align256_sz((size_t)L->ntiles * OA_REC_BYTES);
    L->total = o;
}

template <typename Op>
static void oa_launch(const oa_ctx &ctx, const oa_layout &L, char *w,
                      const int64_t *ngroups, hipStream_t s)
{
    static_assert(sizeof(oa_rec<typename Op::S>) <= OA_REC_BYTES, "record");
    const uint8_t *flags = (const uint8_t *)(w + L.flags);
    const uint32_t *tilecnt = (const uint32_t *)(w + L.tilecnt);
    const uint32_t *tilebase = (const uint32_t *)(w + L.tilebase);
    oa_rec<typename Op::S> *recs = (oa_rec<typename Op::S> *)(w + L.recs);
    hipLaunchKernelGGL(k_oa_reduce<Op>, dim3(L.ntiles), dim3(OA_THREADS), 0, s,
                       ctx, flags, tilebase, recs);
    hipLaunchKernelGGL(k_oa_fix<Op>, dim3(1), dim3(OA_FIX_THREADS), 0, s, ctx,
                       tilecnt, tilebase, recs, L.ntiles, ngroups);
}

extern "C" {

otbx_status otbx_ordered_agg_workspace_bytes(int64_t n, int32_t ncalls,
                                             size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX || ncalls < 0 ||
        ncalls > OTBX_MAX_AGGS)
        return OTBX_ERR_INVALID;
    oa_layout L;
    oa_plan_layout(n, ncalls, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_ordered_agg(const otbx_sortspec *spec, int32_t ngroup,
                             const int64_t *perm_dev, int64_t n,
                             const otbx_oaggcalls *calls, void *ws_dev,
                             size_t ws_bytes, int64_t *first_row_dev,
                             int64_t *ngroups_dev, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!spec || !calls || !ngroups_dev)
        return OTBX_ERR_INVALID;
    if (ngroup < 0 || ngroup > OTBX_MAX_KEYS - 1 || spec->nkeys != ngroup + 1)
        return OTBX_ERR_INVALID;
    if (calls->ncalls < 0 || calls->ncalls > OTBX_MAX_AGGS)
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
    const int argtype = spec->key[ngroup].type;
    bool any_stats = false, any_mode = false, any_sum = false;
    for (int a = 0; a < calls->ncalls; a++) {
        const otbx_oaggcall *c = &calls->call[a];
        if (c->func < OTBX_OAGG_COUNT_DISTINCT || c->func > OTBX_OAGG_MODE)
            return OTBX_ERR_INVALID;
        const bool pct = c->func == OTBX_OAGG_PERCENTILE_DISC ||
                         c->func == OTBX_OAGG_PERCENTILE_CONT;
        /* written so that a NaN fails */
        if (pct && !(c->fraction >= 0.0 && c->fraction <= 1.0))
            return OTBX_ERR_INVALID;
        if (!c->out)
            return OTBX_ERR_INVALID;
        const bool count = c->func == OTBX_OAGG_COUNT_DISTINCT;
        if (count ? c->out_null != nullptr : c->out_null == nullptr)
            return OTBX_ERR_INVALID;
        const bool wide =
            c->func == OTBX_OAGG_SUM_DISTINCT && argtype == OTBX_SORT_I64;
        if (wide ? c->out_hi == nullptr : c->out_hi != nullptr)
            return OTBX_ERR_INVALID;
        if (c->func == OTBX_OAGG_SUM_DISTINCT)
            any_sum = true;
        else if (c->func == OTBX_OAGG_MODE)
            any_mode = true;
        else
            any_stats = true;
    }
    if (calls->ncalls == 0 && !first_row_dev)
        return OTBX_ERR_INVALID;
    oa_layout L;
    oa_plan_layout(n, calls->ncalls, &L);
    /* the kernels read the workspace with 8-byte vectors */
    if (ws_bytes < L.total || (L.total > 0 && !ws_dev) ||
        ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(k_oa_empty, dim3(1), dim3(1), 0, s, *calls, argtype,
                           ngroup == 0 ? 1 : 0, first_row_dev, ngroups_dev);
        HIP_CHECK(hipGetLastError());
        return OTBX_OK;
    }

    char *w = (char *)ws_dev;
    uint8_t *flags = (uint8_t *)(w + L.flags);
    uint32_t *tilecnt = (uint32_t *)(w + L.tilecnt);
    uint32_t *tilebase = (uint32_t *)(w + L.tilebase);
    const uint32_t un = (uint32_t)n;

    hipLaunchKernelGGL(k_oa_flags, dim3(L.ntiles), dim3(OA_THREADS), 0, s,
                       *spec, (int)ngroup, perm_dev, un, flags, tilecnt);
    hipLaunchKernelGGL(k_oa_scan, dim3(1), dim3(OA_FIX_THREADS), 0, s, tilecnt,
                       tilebase, L.ntiles, ngroups_dev);
    if (first_row_dev)
        hipLaunchKernelGGL(k_oa_first, dim3(L.ntiles), dim3(OA_THREADS), 0, s,
                           perm_dev, un, flags, tilebase, first_row_dev);

    oa_ctx ctx;
    ctx.arg = spec->key[ngroup];
    ctx.perm = perm_dev;
    ctx.n = un;
    ctx.pad_ = 0;
    ctx.calls = *calls;
    if (any_stats)
        oa_launch<oa_op_stats>(ctx, L, w, ngroups_dev, s);
    if (any_mode)
        oa_launch<oa_op_mode>(ctx, L, w, ngroups_dev, s);
    if (any_sum) {
        if (argtype == OTBX_SORT_F64)
            oa_launch<oa_op_sumf>(ctx, L, w, ngroups_dev, s);
        else if (argtype == OTBX_SORT_I64)
            oa_launch<oa_op_sum128>(ctx, L, w, ngroups_dev, s);
        else if (argtype == OTBX_SORT_I32)
            oa_launch<oa_op_sumi<int32_t>>(ctx, L, w, ngroups_dev, s);
        else
            oa_launch<oa_op_sumi<uint8_t>>(ctx, L, w, ngroups_dev, s);
    }
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

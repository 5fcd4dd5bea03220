/*
 * otbx_sort.hip — the generic GPU Sort operator (otbx_sort_perm): multi-column
 * ORDER BY with per-key ASC/DESC, NULLS FIRST/LAST and LIMIT, producing the
 * int64 row permutation the otbx_gather_* kernels consume. The ExecSort →
 * tuplesort analog (executor/nodeSort.c:49, utils/sort/tuplesort.c;
 * comparator ApplySortComparator, include/utils/sortsupport.h:201;
 * float8_cmp_internal, utils/adt/float.c:1172). DESIGN.md §8g.
 *
 * Shape of the work (everything stream-ordered, no host round trip):
 *   - every key column is mapped to an order-preserving unsigned radix key
 *     (ss_norm) plus a separate null bit;
 *   - columns are processed last to first; per column a stable LSD radix
 *     sort over (u64 key, u32 row) pairs with 8-bit digits: 1 / 4 / 8 passes
 *     for U8 / I32 / I64,F64, plus a 1-bit null pass for nullable columns;
 *   - the key-build kernel also histograms every digit of the column, so a
 *     pass whose digit is constant over all rows is skipped ON THE DEVICE
 *     (ss_state.pass[] carries skip + ping-pong side per pass);
 *   - one pass = tile histogram (SS_TILE rows per block) → device scan of
 *     the [digit][tile] table → tile scatter. The scatter holds SS_ITEMS
 *     rows per lane in registers, ranks the tile with wave match masks and
 *     per-wave LDS counters, stages the tile digit-sorted in LDS and writes
 *     each digit's rows as one contiguous run;
 *   - LIMIT k < n: a 12-bit-per-level radix select on the leading key finds
 *     a threshold prefix, candidate rows (everything at or before it) are
 *     compacted IN ROW ORDER, and only those are sorted. The row count the
 *     sort kernels see (ss_state.m) lives on the device.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm: the normalised key */

#define SS_THREADS 256
#define SS_WAVES (SS_THREADS / WAVE)
/* rows per lane. Measured at 200 M i64 rows: 8 → 27.3 ms,
 * 12 → 23.3, 16 → 22.1, 24 → 18.6, 32 → 23.4. Longer per-digit runs write
 * fuller cache lines; at 32 the tile no longer fits two blocks per CU. */
#ifndef SS_ITEMS
#define SS_ITEMS 24
#endif
#define SS_TILE (SS_THREADS * SS_ITEMS)      /* 6144 rows per block tile */
#define SS_WSEG (WAVE * SS_ITEMS)            /* rows per wave segment    */
#define SS_BINS 256
#define SS_NULLSLOT 8                        /* pass slot of the null pass */
#define SS_NSLOTS 9
#define SS_SCAN_CHUNK 4096                   /* 256 threads x 16 entries */
#define SS_LBITS 12                          /* LIMIT select: bits per level */
#define SS_LBINS (1 << SS_LBITS)
#define SS_HEADER_BYTES 32768

struct ss_pass {
    uint32_t skip;   /* 1 = digit constant over all rows (or slot unused) */
    uint32_t side;   /* ping-pong side holding this pass's input */
};

struct ss_state {
    uint32_t m;               /* rows being sorted (n, or LIMIT candidates) */
    uint32_t cur;             /* side holding the current (key, idx) arrays */
    unsigned long long prefix; /* LIMIT select: threshold prefix so far */
    unsigned long long below;  /* LIMIT select: rows strictly before it */
    ss_pass pass[SS_NSLOTS];
    uint32_t ghist[SS_NSLOTS][SS_BINS]; /* per-column digit histograms */
    uint32_t lhist[SS_LBINS];           /* LIMIT select level histogram */
};
static_assert(sizeof(ss_state) <= SS_HEADER_BYTES, "state exceeds header");

static inline int ss_wbits(int type)
{
    return type == OTBX_SORT_U8 ? 8 : type == OTBX_SORT_I32 ? 32 : 64;
}

/* 64-bit monotone summary of (null digit, key) for the LIMIT select: the
 * null digit on top, the key left-aligned below it (its lowest bit falls
 * off — the select only needs a non-strict order) */
__device__ __forceinline__ unsigned long long
ss_lead(const otbx_sortkey &k, int wbits, uint32_t row)
{
    uint32_t nd;
    const unsigned long long v = ss_norm(k, row, &nd);
    return ((unsigned long long)nd << 63) | ((v << (64 - wbits)) >> 1);
}

/* block-wide exclusive scan of one u32 per thread (NW waves); *total gets
 * the block sum. wsum: NW LDS words, reusable after return. */
template <int NW>
__device__ __forceinline__ uint32_t ss_block_excl_scan(uint32_t v,
                                                       uint32_t *wsum,
                                                       uint32_t *total)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= o)
            incl += t;
    }
    if (lane == WAVE - 1)
        wsum[wid] = incl;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint32_t s = wsum[w];
        if (w < wid)
            woff += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return woff + incl - v;
}

/* add 1 to lh[d] for every valid lane; a wave whose lanes all carry the same
 * digit (constant or heavily skewed columns) adds once instead of serialising
 * 64 same-address LDS atomics */
__device__ __forceinline__ void ss_lds_count(uint32_t *lh, uint32_t d,
                                             bool valid)
{
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
    if (__all(valid && d == d0)) {
        if (threadIdx.x % WAVE == 0)
            atomicAdd(&lh[d0], (uint32_t)WAVE);
    } else if (valid) {
        atomicAdd(&lh[d], 1u);
    }
}

__global__ void k_ss_init(ss_state *st, uint32_t n, uint32_t *idx0, int iota)
{
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            st->m = n;
            st->cur = 0;
            st->prefix = 0;
            st->below = 0;
        }
        uint32_t *gh = &st->ghist[0][0];
        for (int i = threadIdx.x; i < SS_NSLOTS * SS_BINS; i += blockDim.x)
            gh[i] = 0;
        for (int i = threadIdx.x; i < SS_LBINS; i += blockDim.x)
            st->lhist[i] = 0;
    }
    if (iota) {
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
             i += stride)
            idx0[i] = (uint32_t)i;
    }
}

/* per column: keys[i] = norm(col[idx[i]]) on the current side, and the
 * histogram of every digit (+ the null digit) into st->ghist */
__global__ __launch_bounds__(SS_THREADS) void
k_ss_build(ss_state *st, otbx_sortkey key, int npass, uint32_t rowmax,
           unsigned long long *kA, unsigned long long *kB,
           const uint32_t *iA, const uint32_t *iB)
{
    __shared__ uint32_t lh[SS_NSLOTS][SS_BINS];
    for (int i = threadIdx.x; i < SS_NSLOTS * SS_BINS; i += SS_THREADS)
        (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint32_t m = st->m;
    const uint32_t side = st->cur;
    unsigned long long *keys = side ? kB : kA;
    const uint32_t *idx = side ? iB : iA;
    const int64_t stride = (int64_t)gridDim.x * SS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * SS_THREADS; base < m;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < m;
        unsigned long long v = 0;
        uint32_t nd = 0;
        if (valid) {
            const uint32_t row = idx[i];
            v = ss_norm(key, row < rowmax ? row : rowmax, &nd);
            keys[i] = v;
        }
        for (int p = 0; p < npass; p++)
            ss_lds_count(lh[p], (uint32_t)(v >> (8 * p)) & 0xffu, valid);
        if (key.nulls)
            ss_lds_count(lh[SS_NULLSLOT], nd, valid);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_NSLOTS * SS_BINS; i += SS_THREADS) {
        const uint32_t c = (&lh[0][0])[i];
        if (c)
            atomicAdd(&(&st->ghist[0][0])[i], c);
    }
}

/* per column: decide which passes run (a digit held by all m rows sorts
 * nothing) and which ping-pong side each pass reads; re-zero ghist */
__global__ __launch_bounds__(SS_THREADS) void
k_ss_plan(ss_state *st, int npass, int hasnull)
{
    __shared__ uint32_t sk[SS_NSLOTS];
    const uint32_t m = st->m;
    for (int p = 0; p < SS_NSLOTS; p++) {
        const bool active = p < npass || (p == SS_NULLSLOT && hasnull);
        const uint32_t c = st->ghist[p][threadIdx.x];
        st->ghist[p][threadIdx.x] = 0;
        const int single = __syncthreads_or(c == m);
        if (threadIdx.x == 0)
            sk[p] = (!active || single || m <= 1) ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t side = st->cur;
        for (int p = 0; p < SS_NSLOTS; p++) {
            st->pass[p].skip = sk[p];
            st->pass[p].side = side;
            if (!sk[p])
                side ^= 1u;
        }
        st->cur = side;
    }
}

template <bool NULLPASS>
__device__ __forceinline__ uint32_t
ss_digit(unsigned long long key, uint32_t row, int shift,
         const uint8_t *nulls, uint32_t dnull, uint32_t rowmax)
{
    /* row ids come from the workspace: clamp so that a stale id can never
     * index outside the column */
    if (NULLPASS)
        return nulls[row < rowmax ? row : rowmax] ? dnull : 1u - dnull;
    return (uint32_t)(key >> shift) & 0xffu;
}

/* tile histogram: hist[digit][tile], tiles = ceil(m / SS_TILE) */
template <bool NULLPASS>
__global__ __launch_bounds__(SS_THREADS) void
k_ss_hist(const ss_state *st, int pslot, int shift,
          const unsigned long long *kA, const unsigned long long *kB,
          const uint32_t *iA, const uint32_t *iB, const uint8_t *nulls,
          uint32_t dnull, uint32_t rowmax, uint32_t *hist)
{
    const ss_pass pi = st->pass[pslot];
    if (pi.skip)
        return;
    const uint32_t m = st->m;
    const uint32_t nbe = (m + SS_TILE - 1) / SS_TILE;
    if (blockIdx.x >= nbe)
        return;
    const unsigned long long *keys = pi.side ? kB : kA;
    const uint32_t *idx = pi.side ? iB : iA;
    __shared__ uint32_t lh[SS_BINS];
    lh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * (uint32_t)SS_TILE;
#pragma unroll 4
    for (int j = 0; j < SS_ITEMS; j++) {
        const uint32_t i = tile0 + j * SS_THREADS + threadIdx.x;
        const bool valid = i < m;
        uint32_t d = 0;
        if (valid)
            d = ss_digit<NULLPASS>(NULLPASS ? 0ull : keys[i],
                                   NULLPASS ? idx[i] : 0u, shift, nulls, dnull,
                                   rowmax);
        ss_lds_count(lh, d, valid);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nbe + blockIdx.x] = lh[threadIdx.x];
}

/* ---- device exclusive scan of a u32 array, in place, three kernels ----
 * length: host_len, or (st != NULL) the current pass's 256 x tiles table */
__device__ __forceinline__ uint32_t ss_scan_len(const ss_state *st, int pslot,
                                                uint32_t host_len)
{
    if (!st)
        return host_len;
    if (st->pass[pslot].skip)
        return 0;
    return SS_BINS * ((st->m + SS_TILE - 1) / SS_TILE);
}

__global__ __launch_bounds__(SS_THREADS) void
k_ss_scan_sum(const ss_state *st, int pslot, uint32_t host_len,
              const uint32_t *__restrict__ data, uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wsum[SS_WAVES];
    const uint32_t len = ss_scan_len(st, pslot, host_len);
    const uint64_t c0 = (uint64_t)blockIdx.x * SS_SCAN_CHUNK;
    if (c0 >= len)
        return;
    uint32_t s = 0;
    const uint64_t t0 = c0 + (uint64_t)threadIdx.x * 16;
#pragma unroll
    for (int e = 0; e < 16; e++)
        s += (t0 + e < len) ? data[t0 + e] : 0u;
    uint32_t tot;
    ss_block_excl_scan<SS_WAVES>(s, wsum, &tot);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = tot;
}

#define SS_MID_THREADS 1024
__global__ __launch_bounds__(SS_MID_THREADS) void
k_ss_scan_mid(const ss_state *st, int pslot, uint32_t host_len, uint32_t *sums)
{
    __shared__ uint32_t wsum[SS_MID_THREADS / WAVE];
    const uint32_t len = ss_scan_len(st, pslot, host_len);
    const uint32_t cnt = (len + SS_SCAN_CHUNK - 1) / SS_SCAN_CHUNK;
    const uint32_t per = (cnt + SS_MID_THREADS - 1) / SS_MID_THREADS;
    const uint32_t lo = threadIdx.x * per;
    const uint32_t hi = lo + per < cnt ? lo + per : cnt;
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++)
        s += sums[i];
    uint32_t tot;
    uint32_t acc = ss_block_excl_scan<SS_MID_THREADS / WAVE>(s, wsum, &tot);
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = sums[i];
        sums[i] = acc;
        acc += c;
    }
}

__global__ __launch_bounds__(SS_THREADS) void
k_ss_scan_apply(const ss_state *st, int pslot, uint32_t host_len,
                uint32_t *data, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wsum[SS_WAVES];
    const uint32_t len = ss_scan_len(st, pslot, host_len);
    const uint64_t c0 = (uint64_t)blockIdx.x * SS_SCAN_CHUNK;
    if (c0 >= len)
        return;
    const uint64_t t0 = c0 + (uint64_t)threadIdx.x * 16;
    uint32_t c[16];
    uint32_t s = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        c[e] = (t0 + e < len) ? data[t0 + e] : 0u;
        s += c[e];
    }
    uint32_t tot;
    uint32_t acc = ss_block_excl_scan<SS_WAVES>(s, wsum, &tot) +
                   sums[blockIdx.x];
#pragma unroll
    for (int e = 0; e < 16; e++) {
        if (t0 + e < len)
            data[t0 + e] = acc;
        acc += c[e];
    }
}

/* ---- tile scatter (the hot kernel) ----
 * Tile order: wave w owns rows [w*SS_WSEG, (w+1)*SS_WSEG) of the tile, item
 * j of lane l is row w*SS_WSEG + j*64 + l (coalesced loads; tile order =
 * wave, item, lane). Rank of a row among equal digits of its tile:
 *   rows of earlier waves   — per-wave digit counters, prefixed over waves
 *   earlier items, same wave — the counter value read when the item ranks
 *   same item, lower lanes  — popcount of the match mask below the lane
 * which is exactly tile order, so the pass is stable. The tile is then laid
 * out digit-sorted in LDS and written out: every digit's rows are one
 * contiguous run in LDS and in global memory. base = scanned hist.
 * Budget at SS_ITEMS = 24: 205 VGPRs (2 waves/SIMD) and 61,456 B of LDS
 * (48 KiB staging buffer shared by keys and row ids, 6 KiB digit bytes,
 * 6 KiB counters) — two resident blocks per CU (160 KiB LDS). */
template <bool NULLPASS>
__global__ __launch_bounds__(SS_THREADS) void
k_ss_scatter(const ss_state *st, int pslot, int shift,
             unsigned long long *kA, unsigned long long *kB, uint32_t *iA,
             uint32_t *iB, const uint8_t *nulls, uint32_t dnull,
             uint32_t rowmax, const uint32_t *__restrict__ base)
{
    const ss_pass pi = st->pass[pslot];
    if (pi.skip)
        return;
    const uint32_t m = st->m;
    const uint32_t nbe = (m + SS_TILE - 1) / SS_TILE;
    if (blockIdx.x >= nbe)
        return;
    const unsigned long long *ksrc = pi.side ? kB : kA;
    unsigned long long *kdst = pi.side ? kA : kB;
    const uint32_t *isrc = pi.side ? iB : iA;
    uint32_t *idst = pi.side ? iA : iB;

    __shared__ uint32_t wc[SS_WAVES][SS_BINS];  /* per-wave digit counters */
    __shared__ uint32_t lstart[SS_BINS];        /* digit start in the tile */
    __shared__ uint32_t gbase[SS_BINS];         /* global start - lstart   */
    __shared__ uint32_t wsum[SS_WAVES];
    /* one staging buffer: the tile's keys first, its row ids after them */
    __shared__ unsigned long long sbuf[NULLPASS ? SS_TILE / 2 : SS_TILE];
    __shared__ uint8_t sdig[NULLPASS ? 4 : SS_TILE];
    uint32_t *sidx = (uint32_t *)sbuf;

    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile0 = blockIdx.x * (uint32_t)SS_TILE;
    const uint32_t tcount = m - tile0 < SS_TILE ? m - tile0 : SS_TILE;
    const uint32_t r0 = (uint32_t)wid * SS_WSEG + (uint32_t)lane;

#pragma unroll
    for (int w = 0; w < SS_WAVES; w++)
        wc[w][threadIdx.x] = 0;

    unsigned long long key[SS_ITEMS];
    uint32_t id[SS_ITEMS];
#pragma unroll
    for (int j = 0; j < SS_ITEMS; j++) {
        const uint32_t r = r0 + j * WAVE;
        const bool valid = r < tcount;
        key[j] = (!NULLPASS && valid) ? ksrc[tile0 + r] : 0ull;
        id[j] = valid ? isrc[tile0 + r] : 0u;
    }
    __syncthreads();

    uint32_t dig[SS_ITEMS];
    uint32_t rank[SS_ITEMS];
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < SS_ITEMS; j++) {
        const bool valid = r0 + j * WAVE < tcount;
        const uint32_t d = valid ? ss_digit<NULLPASS>(key[j], id[j], shift,
                                                      nulls, dnull, rowmax)
                                 : 0u;
        unsigned long long match = __ballot(valid);
#pragma unroll
        for (int b = 0; b < (NULLPASS ? 1 : 8); b++) {
            const unsigned long long bb = __ballot((d >> b) & 1u);
            match &= ((d >> b) & 1u) ? bb : ~bb;
        }
        /* lanes of one digit: the lowest takes the wave's running count */
        const int leader = valid ? __ffsll((long long)match) - 1 : lane;
        uint32_t old = 0;
        if (valid && lane == leader)
            old = atomicAdd(&wc[wid][d], (uint32_t)__popcll(match));
        old = __shfl(old, leader);
        dig[j] = d;
        rank[j] = old + (uint32_t)__popcll(match & lt);
    }
    __syncthreads();

    {   /* thread t owns digit t: prefix its count over waves, scan digits */
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < SS_WAVES; w++) {
            const uint32_t c = wc[w][threadIdx.x];
            wc[w][threadIdx.x] = tot;
            tot += c;
        }
        uint32_t all;
        const uint32_t ex = ss_block_excl_scan<SS_WAVES>(tot, wsum, &all);
        lstart[threadIdx.x] = ex;
        gbase[threadIdx.x] = base[(size_t)threadIdx.x * nbe + blockIdx.x] - ex;
    }
    __syncthreads();

    /* rank[j] becomes the row's slot in the digit-sorted tile */
#pragma unroll
    for (int j = 0; j < SS_ITEMS; j++) {
        const bool valid = r0 + j * WAVE < tcount;
        const uint32_t p = lstart[dig[j]] + wc[wid][dig[j]] + rank[j];
        rank[j] = (valid && p < SS_TILE) ? p : SS_TILE;
    }
    if (NULLPASS) {
#pragma unroll
        for (int j = 0; j < SS_ITEMS; j++)
            if (rank[j] < SS_TILE)
                sidx[rank[j]] = id[j] | (dig[j] << 31);
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < tcount; q += SS_THREADS) {
            const uint32_t v = sidx[q];
            const uint32_t pos = gbase[v >> 31] + q;
            if (pos < m)
                idst[pos] = v & 0x7fffffffu;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < SS_ITEMS; j++)
        if (rank[j] < SS_TILE)
            sbuf[rank[j]] = key[j];
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < tcount; q += SS_THREADS) {
        const unsigned long long k = sbuf[q];
        const uint32_t d = (uint32_t)(k >> shift) & 0xffu;
        const uint32_t pos = gbase[d] + q;
        sdig[q] = (uint8_t)d;     /* read back by this same thread below */
        if (pos < m)
            kdst[pos] = k;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SS_ITEMS; j++)
        if (rank[j] < SS_TILE)
            sidx[rank[j]] = id[j];
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < tcount; q += SS_THREADS) {
        const uint32_t pos = gbase[sdig[q]] + q;
        if (pos < m)
            idst[pos] = sidx[q];
    }
}

/* ---- LIMIT: radix select on the leading key ---- */

/* level histogram: rows whose top 12*level lead bits equal the threshold
 * prefix found so far, binned by the next 12 bits */
__global__ __launch_bounds__(SS_THREADS) void
k_ss_lim_hist(ss_state *st, otbx_sortkey key, int wbits, uint32_t n, int level)
{
    __shared__ uint32_t lh[SS_LBINS];
    for (int i = threadIdx.x; i < SS_LBINS; i += SS_THREADS)
        lh[i] = 0;
    __syncthreads();
    const unsigned long long prefix = st->prefix;
    const int sh = 64 - SS_LBITS * (level + 1);
    const int64_t stride = (int64_t)gridDim.x * SS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * SS_THREADS; base < n;
         base += stride) {
        const int64_t i = base + threadIdx.x;
        bool part = i < n;
        uint32_t bin = 0;
        if (part) {
            const unsigned long long lead = ss_lead(key, wbits, (uint32_t)i);
            part = level == 0 || (lead >> (sh + SS_LBITS)) == prefix;
            bin = (uint32_t)(lead >> sh) & (SS_LBINS - 1);
        }
        ss_lds_count(lh, bin, part);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_LBINS; i += SS_THREADS) {
        const uint32_t c = lh[i];
        if (c)
            atomicAdd(&st->lhist[i], c);
    }
}

/* threshold bin of the level: the first bin whose cumulative count reaches
 * limit - below. Extends prefix, advances below, re-zeroes lhist. */
__global__ __launch_bounds__(SS_THREADS) void
k_ss_lim_thresh(ss_state *st, unsigned long long limit)
{
    __shared__ uint32_t wsum[SS_WAVES];
    const unsigned long long below = st->below;
    const unsigned long long prefix = st->prefix;
    const unsigned long long need = limit - below;
    uint32_t c[16];
    uint32_t s = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        c[e] = st->lhist[threadIdx.x * 16 + e];
        st->lhist[threadIdx.x * 16 + e] = 0;
        s += c[e];
    }
    uint32_t tot;
    const uint32_t ex = ss_block_excl_scan<SS_WAVES>(s, wsum, &tot);
    if ((unsigned long long)ex < need && need <= (unsigned long long)ex + s) {
        uint32_t cum = ex;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            if ((unsigned long long)cum + c[e] >= need) {
                st->prefix = (prefix << SS_LBITS) |
                             (unsigned long long)(threadIdx.x * 16 + e);
                st->below = below + cum;
                break;
            }
            cum += c[e];
        }
    }
}

/* candidates = rows whose lead, cut to the selected bits, is <= the
 * threshold prefix. WRITE = false: per-tile candidate counts. WRITE = true:
 * order-preserving compaction of the candidate row ids (offs = scanned
 * counts), and st->m = candidate count. */
template <bool WRITE>
__global__ __launch_bounds__(SS_THREADS) void
k_ss_lim_compact(ss_state *st, otbx_sortkey key, int wbits, uint32_t n, int sh,
                 uint32_t *offs, uint32_t *iA, uint32_t *iB)
{
    __shared__ uint32_t wsum[SS_WAVES];
    const unsigned long long prefix = st->prefix;
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint64_t tile0 = (uint64_t)blockIdx.x * SS_TILE;
    const uint64_t r0 = tile0 + (uint64_t)wid * SS_WSEG + (uint64_t)lane;
    uint32_t predmask = 0, wtot = 0;
#pragma unroll 4
    for (int j = 0; j < SS_ITEMS; j++) {
        const uint64_t row = r0 + (uint64_t)j * WAVE;
        const bool pred = row < n &&
                          (ss_lead(key, wbits, (uint32_t)row) >> sh) <= prefix;
        predmask |= (pred ? 1u : 0u) << j;
        wtot += (uint32_t)__popcll(__ballot(pred));
    }
    if (lane == 0)
        wsum[wid] = wtot;
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < SS_WAVES; w++)
                t += wsum[w];
            offs[blockIdx.x] = t;
        }
        return;
    }
    uint32_t off = offs[blockIdx.x];
    for (int w = 0; w < wid; w++)
        off += wsum[w];
    uint32_t *idx = st->cur ? iB : iA;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int j = 0; j < SS_ITEMS; j++) {
        const bool pred = (predmask >> j) & 1u;
        const unsigned long long bal = __ballot(pred);
        const uint32_t pos = off + (uint32_t)__popcll(bal & lt);
        if (pred && pos < n)
            idx[pos] = (uint32_t)(r0 + (uint64_t)j * WAVE);
        off += (uint32_t)__popcll(bal);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == SS_THREADS - 1)
        st->m = off;
}

__global__ void k_ss_emit(const ss_state *st, const uint32_t *iA,
                          const uint32_t *iB, int64_t nout,
                          int64_t *__restrict__ perm, int64_t *nout_dev)
{
    const uint32_t *idx = st->cur ? iB : iA;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nout;
         i += stride)
        perm[i] = (int64_t)idx[i];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *nout_dev = nout;
}

/* ---- host side ---- */

struct ss_layout {
    size_t keyA, keyB, idxA, idxB, hist, sums, total;
    uint32_t nb;      /* tiles at capacity n */
    uint32_t chunks;  /* scan chunks at capacity */
};

static void ss_plan_layout(int64_t n, ss_layout *L)
{
    const size_t nal = ((size_t)n + 63) & ~(size_t)63;
    L->nb = (uint32_t)((n + SS_TILE - 1) / SS_TILE);
    L->chunks = (uint32_t)(((size_t)SS_BINS * L->nb + SS_SCAN_CHUNK - 1) /
                           SS_SCAN_CHUNK);
    size_t o = SS_HEADER_BYTES;
    L->keyA = o; o += align256_sz(nal * 8);
    L->keyB = o; o += align256_sz(nal * 8);
    L->idxA = o; o += align256_sz(nal * 4);
    L->idxB = o; o += align256_sz(nal * 4);
    L->hist = o; o += align256_sz((size_t)SS_BINS * L->nb * 4);
    L->sums = o; o += align256_sz((size_t)L->chunks * 4);
    L->total = o;
}

extern "C" {

otbx_status otbx_sort_workspace_bytes(int64_t n, int32_t nkeys, int64_t limit,
                                      size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX || nkeys < 1 ||
        nkeys > OTBX_MAX_KEYS || limit < 0)
        return OTBX_ERR_INVALID;
    /* key count and limit do not change the requirement: columns are
     * normalised one at a time into the same ping-pong arrays, and the
     * LIMIT candidate set is sized for n (a heavy threshold bin makes every
     * row a candidate) */
    ss_layout L;
    ss_plan_layout(n, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_sort_perm(const otbx_sortspec *spec, int64_t n, int64_t limit,
                           void *ws_dev, size_t ws_bytes, int64_t *perm_dev,
                           int64_t *nout_dev, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!spec || spec->nkeys < 1 || spec->nkeys > OTBX_MAX_KEYS)
        return OTBX_ERR_INVALID;
    if (n < 0 || n > INT32_MAX || limit < 0)
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
    ss_layout L;
    ss_plan_layout(n, &L);
    if (ws_bytes < L.total || !ws_dev || !nout_dev || (n > 0 && !perm_dev))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(nout_dev, 0, 8, s));
        return OTBX_OK;
    }
    char *w = (char *)ws_dev;
    ss_state *st = (ss_state *)w;
    unsigned long long *kA = (unsigned long long *)(w + L.keyA);
    unsigned long long *kB = (unsigned long long *)(w + L.keyB);
    uint32_t *iA = (uint32_t *)(w + L.idxA);
    uint32_t *iB = (uint32_t *)(w + L.idxB);
    uint32_t *hist = (uint32_t *)(w + L.hist);
    uint32_t *sums = (uint32_t *)(w + L.sums);
    const uint32_t un = (uint32_t)n;
    const bool select = limit > 0 && limit < n;
    const int64_t nout = select ? limit : n;

    hipLaunchKernelGGL(k_ss_init, dim3(select ? 1 : grid_for(n, 256)),
                       dim3(256), 0, s, st, un, iA, select ? 0 : 1);

    if (select) {
        const otbx_sortkey k0 = spec->key[0];
        const int wb = ss_wbits(k0.type);
        /* 1 null bit + wb key bits, 12 bits per level */
        const int levels = (1 + wb + SS_LBITS - 1) / SS_LBITS > 5
                               ? 5 : (1 + wb + SS_LBITS - 1) / SS_LBITS;
        for (int lv = 0; lv < levels; lv++) {
            hipLaunchKernelGGL(k_ss_lim_hist, dim3(grid_for(n, SS_THREADS)),
                               dim3(SS_THREADS), 0, s, st, k0, wb, un, lv);
            hipLaunchKernelGGL(k_ss_lim_thresh, dim3(1), dim3(SS_THREADS), 0,
                               s, st, (unsigned long long)limit);
        }
        const int sh = 64 - SS_LBITS * levels;
        const uint32_t cch = (L.nb + SS_SCAN_CHUNK - 1) / SS_SCAN_CHUNK;
        hipLaunchKernelGGL(k_ss_lim_compact<false>, dim3(L.nb),
                           dim3(SS_THREADS), 0, s, st, k0, wb, un, sh, hist,
                           iA, iB);
        hipLaunchKernelGGL(k_ss_scan_sum, dim3(cch), dim3(SS_THREADS), 0, s,
                           (const ss_state *)nullptr, 0, L.nb, hist, sums);
        hipLaunchKernelGGL(k_ss_scan_mid, dim3(1), dim3(SS_MID_THREADS), 0, s,
                           (const ss_state *)nullptr, 0, L.nb, sums);
        hipLaunchKernelGGL(k_ss_scan_apply, dim3(cch), dim3(SS_THREADS), 0, s,
                           (const ss_state *)nullptr, 0, L.nb, hist, sums);
        hipLaunchKernelGGL(k_ss_lim_compact<true>, dim3(L.nb),
                           dim3(SS_THREADS), 0, s, st, k0, wb, un, sh, hist,
                           iA, iB);
    }

    for (int c = spec->nkeys - 1; c >= 0; c--) {
        const otbx_sortkey k = spec->key[c];
        const int npass = ss_wbits(k.type) / 8;
        const int hasnull = k.nulls != nullptr;
        const uint32_t dnull = (k.flags & OTBX_SORT_NULLS_FIRST) ? 0u : 1u;
        hipLaunchKernelGGL(k_ss_build, dim3(grid_for(n, SS_THREADS)),
                           dim3(SS_THREADS), 0, s, st, k, npass, un - 1, kA, kB,
                           iA, iB);
        hipLaunchKernelGGL(k_ss_plan, dim3(1), dim3(SS_THREADS), 0, s, st,
                           npass, hasnull);
        for (int p = 0; p < npass + hasnull; p++) {
            const bool np = p == npass;
            const int slot = np ? SS_NULLSLOT : p;
            const int shift = 8 * p;
            if (np)
                hipLaunchKernelGGL(k_ss_hist<true>, dim3(L.nb),
                                   dim3(SS_THREADS), 0, s, st, slot, 0, kA,
                                   kB, iA, iB, k.nulls, dnull, un - 1,
                                   hist);
            else
                hipLaunchKernelGGL(k_ss_hist<false>, dim3(L.nb),
                                   dim3(SS_THREADS), 0, s, st, slot, shift,
                                   kA, kB, iA, iB, k.nulls, dnull, un - 1,
                                   hist);
            hipLaunchKernelGGL(k_ss_scan_sum, dim3(L.chunks),
                               dim3(SS_THREADS), 0, s, st, slot, 0u, hist,
                               sums);
            hipLaunchKernelGGL(k_ss_scan_mid, dim3(1), dim3(SS_MID_THREADS),
                               0, s, st, slot, 0u, sums);
            hipLaunchKernelGGL(k_ss_scan_apply, dim3(L.chunks),
                               dim3(SS_THREADS), 0, s, st, slot, 0u, hist,
                               sums);
            if (np)
                hipLaunchKernelGGL(k_ss_scatter<true>, dim3(L.nb),
                                   dim3(SS_THREADS), 0, s, st, slot, 0, kA,
                                   kB, iA, iB, k.nulls, dnull, un - 1,
                                   hist);
            else
                hipLaunchKernelGGL(k_ss_scatter<false>, dim3(L.nb),
                                   dim3(SS_THREADS), 0, s, st, slot, shift,
                                   kA, kB, iA, iB, k.nulls, dnull, un - 1,
                                   hist);
        }
    }
    hipLaunchKernelGGL(k_ss_emit, dim3(grid_for(nout, 256)), dim3(256), 0, s,
                       st, iA, iB, nout, perm_dev, nout_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

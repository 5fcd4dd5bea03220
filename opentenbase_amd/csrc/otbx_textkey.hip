/*
 * otbx_textkey.hip — text as a sort, group or join key: otbx_text_rank gives
 * every row of one to four text columns the dense rank of its string under C
 * collation (varstr_cmp with lc_collate_is_c, varlena.c:1614-1629), an
 * order-preserving dictionary code. The codes are an ordinary int64 key
 * column for otbx_sort_perm, otbx_window, otbx_group_agg, otbx_agg_i64* and
 * otbx_join_i64*. Contract in include/otbx.h, DESIGN.md §8m.
 *
 * The rows of the set are one virtual column, column 0 first. Refinement in
 * rounds of 8 bytes: every row carries a group id, the start position of its
 * group in the order known so far (0 for all rows at the start). Round r
 * looks at bytes [8r, 8r+8) of the rows still undecided:
 *   k_tk_extract  — per undecided row: the group id, the up to 8 bytes as a
 *                   big-endian u64, zero-padded, top bit flipped so it
 *                   orders as I64 (`chunk`), and min(len − 8r, 9) as U8
 *                   (`lencode`). Aligned 8-byte loads plus a shift where
 *                   both words lie inside the column's bytes, byte loads
 *                   otherwise; nothing outside bytes is ever read. A NULL
 *                   row (round 0 only) sets a mask byte, its bytes are not
 *                   read.
 *   otbx_sort_perm — the radix sort itself, by (group id, chunk, lencode);
 *                   NULL rows go last through the primary key's mask.
 *   k_tk_flags    — per sorted position: does a new group start here (any
 *                   key differs from the row before), did an old group
 *                   start here, is lencode 9, is the row NULL.
 *   k_tk_reduce / k_tk_scan_tiles / k_tk_apply — tile aggregates, one
 *                   workgroup scanning them, and the pass that applies them;
 *                   kernel boundaries are the only ordering between
 *                   workgroups. Three scans in one: the last new-group start
 *                   at or before a position (max), the last old-group start
 *                   (max), and the number of rows still undecided before it
 *                   (sum). New group id = old id + (new start − old start).
 *                   A group is finished when it is a singleton or its
 *                   lencode is ≤ 8 (all members ended inside this chunk and
 *                   are equal); rows of unfinished groups are compacted, in
 *                   sorted order, into the next round's input.
 * One int64, the number of rows still undecided, is read back per round:
 * the call is synchronous.
 * After the last round the group ids are the positions of the groups in the
 * final order:
 *   k_tk_fin_init / k_tk_fin_mark — minrow[id] = the smallest row holding
 *                   the id (atomicMin: the result does not depend on the
 *                   order of arrival).
 *   k_tk_reduce<RANK> / k_tk_scan_tiles / k_tk_rank_apply — exclusive count
 *                   of the ids in use = the dense code of every id, D, and
 *                   dict_row[code] = minrow.
 *   k_tk_codes    — codes[row] = rank[id[row]], −1 under a NULL.
 */
#include <string.h>

#include "otbx_common.h"
#include "otbx_textcol.h"   /* txt_clamp, txt_row, txt_col_ok */

#define TK_THREADS 256
#define TK_ITEMS 8
#define TK_TILE (TK_THREADS * TK_ITEMS)   /* positions per workgroup tile */
#define TK_SCAN_THREADS 1024              /* tiles per pass of the tile scan */
#define TK_HEADER_BYTES 256

/* flag bits of a sorted position */
#define TKF_NEW 1u     /* a new group starts here */
#define TKF_OLD 2u     /* a group of the round's input starts here */
#define TKF_LONG 4u    /* lencode 9: the row goes on past this chunk */
#define TKF_NULL 8u
#define TK_NOROW 0xffffffffu   /* minrow of an id no row holds */

static_assert(sizeof(otbx_textset) == 8 + 32 * OTBX_MAX_TEXT_RANK_COLS +
                                          8 * OTBX_MAX_TEXT_RANK_COLS,
              "otbx_textset layout");
static_assert(OTBX_MAX_TEXT_RANK_COLS == 4, "tk_locate: three compares");

/* the set as the kernels get it: start[c] is the virtual row of column c's
 * row 0; start[c] for c >= ncols is n_total, which no row reaches. It lives
 * in the workspace header, not in the launch arguments: the column is
 * picked per row, and an indexed read of a by-value argument goes through
 * scratch (168 bytes per lane in the extraction kernel). */
struct tk_cols {
    otbx_textcol col[OTBX_MAX_TEXT_RANK_COLS];
    int64_t start[OTBX_MAX_TEXT_RANK_COLS];
};
#define TK_COLS_OFFSET 64   /* in the header, after the two counters */
static_assert(TK_COLS_OFFSET + sizeof(tk_cols) <= TK_HEADER_BYTES,
              "set exceeds header");

/* virtual row → (column, local row). An empty column shares its start with
 * the next one and is stepped over. */
__device__ __forceinline__ otbx_textcol
tk_locate(const tk_cols &t, uint32_t row, int64_t *local)
{
    const int64_t r = (int64_t)row;
    const int c = (r >= t.start[1]) + (r >= t.start[2]) + (r >= t.start[3]);
    *local = r - t.start[c];
    return t.col[c];
}

/* bytes [p, p + k) of the column, 0 <= k <= 8, all inside [0, nbytes):
 * packed big-endian, zero-padded */
__device__ __forceinline__ unsigned long long
tk_chunk(const uint8_t *bytes, int64_t nbytes, int64_t p, int k)
{
    if (k <= 0)
        return 0;
    const uintptr_t base = (uintptr_t)bytes, end = base + (uintptr_t)nbytes;
    const uintptr_t a = base + (uintptr_t)p, a0 = a & ~(uintptr_t)7;
    const int sh = (int)(a & 7u);
    unsigned long long v;
    if (a0 >= base && a0 + 8 <= end && (sh + k <= 8 || a0 + 16 <= end)) {
        v = *(const unsigned long long *)a0 >> (8 * sh);
        if (sh + k > 8)   /* sh >= 1 here */
            v |= *(const unsigned long long *)(a0 + 8) << (64 - 8 * sh);
    } else {
        v = 0;
        for (int i = 0; i < k; i++)
            v |= (unsigned long long)bytes[p + i] << (8 * i);
    }
    v = __builtin_bswap64(v);
    return k >= 8 ? v : v & ~(~0ull >> (8 * k));
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_extract(const tk_cols *__restrict__ tp, const uint32_t *__restrict__ act,
             const uint32_t m, const int round,
             const int32_t *__restrict__ gid, int32_t *__restrict__ kg,
             int64_t *__restrict__ chunk, uint8_t *__restrict__ lc,
             uint8_t *__restrict__ nl)
{
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; j < m;
         j += stride) {
        /* round 0 takes every row, in row order, all in group 0 */
        const uint32_t row = act ? act[j] : (uint32_t)j;
        int64_t local;
        const otbx_textcol c = tk_locate(*tp, row, &local);
        const bool isnull = c.nulls && c.nulls[local];
        unsigned long long v = 0;
        int code = 0;
        if (!isnull) {
            int64_t s;
            int len;
            txt_row(c, local, &s, &len);
            const int64_t off = 8 * (int64_t)round;
            const int64_t rem = len > off ? len - off : 0;
            v = tk_chunk(c.bytes, c.nbytes, s + off, rem < 8 ? (int)rem : 8);
            code = rem < 9 ? (int)rem : 9;
        }
        kg[j] = act ? gid[row] : 0;
        chunk[j] = (int64_t)(v ^ (1ull << 63));
        lc[j] = (uint8_t)code;
        if (nl)
            nl[j] = isnull ? 1 : 0;
    }
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_flags(const uint32_t m, const int64_t *__restrict__ perm,
           const int32_t *__restrict__ kg, const int64_t *__restrict__ chunk,
           const uint8_t *__restrict__ lc, const uint8_t *__restrict__ nl,
           uint8_t *__restrict__ flags)
{
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; j < m;
         j += stride) {
        const int64_t a = perm[j];
        const bool isnull = nl && nl[a];
        bool bold = j == 0 || isnull, bnew = bold;
        if (!bold) {
            const int64_t b = perm[j - 1];
            bold = kg[a] != kg[b];
            bnew = bold || chunk[a] != chunk[b] || lc[a] != lc[b];
        }
        flags[j] = (uint8_t)((bnew ? TKF_NEW : 0u) | (bold ? TKF_OLD : 0u) |
                             (lc[a] == 9 ? TKF_LONG : 0u) |
                             (isnull ? TKF_NULL : 0u));
    }
}

/* a row goes on to the next round: it continues past this chunk and shares
 * its new group with a neighbour */
__device__ __forceinline__ uint32_t
tk_undecided(const uint8_t *flags, uint32_t j, uint32_t m)
{
    const uint32_t f = flags[j];
    if ((f & (TKF_LONG | TKF_NULL)) != TKF_LONG)
        return 0;
    if (!(f & TKF_NEW))
        return 1;
    return j + 1 < m && !(flags[j + 1] & TKF_NEW) ? 1 : 0;
}

struct tk_v3 {
    uint32_t mxn, mxo, cnt;   /* max, max, sum */
};

__device__ __forceinline__ tk_v3 tk_join(tk_v3 a, tk_v3 b)
{
    tk_v3 r;
    r.mxn = a.mxn > b.mxn ? a.mxn : b.mxn;
    r.mxo = a.mxo > b.mxo ? a.mxo : b.mxo;
    r.cnt = a.cnt + b.cnt;
    return r;
}

/* inclusive scan over the workgroup; ws: one slot per wave, reusable after
 * return. *total gets the workgroup's aggregate */
template <int THREADS>
__device__ __forceinline__ tk_v3 tk_block_scan(tk_v3 v, tk_v3 *ws,
                                               tk_v3 *total)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        tk_v3 x;
        x.mxn = __shfl_up(v.mxn, o);
        x.mxo = __shfl_up(v.mxo, o);
        x.cnt = __shfl_up(v.cnt, o);
        if (lane >= o)
            v = tk_join(x, v);
    }
    if (lane == WAVE - 1)
        ws[wid] = v;
    __syncthreads();
    tk_v3 pre = {0, 0, 0}, tot = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < THREADS / WAVE; w++) {
        const tk_v3 x = ws[w];
        if (w < wid)
            pre = tk_join(pre, x);
        tot = tk_join(tot, x);
    }
    __syncthreads();
    *total = tot;
    return tk_join(pre, v);
}

/* what position j contributes to the three scans. RANK: flags is the u32
 * minrow array of the final pass (an id is in use where a row was recorded)
 * and only the sum is used */
template <bool RANK>
__device__ __forceinline__ tk_v3 tk_item(const void *flags, uint32_t j,
                                         uint32_t m)
{
    tk_v3 v = {0, 0, 0};
    if (j < m) {
        if (RANK) {
            v.cnt = ((const uint32_t *)flags)[j] != TK_NOROW;
        } else {
            const uint32_t f = ((const uint8_t *)flags)[j];
            v.mxn = (f & TKF_NEW) ? j : 0;
            v.mxo = (f & TKF_OLD) ? j : 0;
            v.cnt = tk_undecided((const uint8_t *)flags, j, m);
        }
    }
    return v;
}

template <bool RANK>
__global__ __launch_bounds__(TK_THREADS) void
k_tk_reduce(const uint32_t m, const void *__restrict__ flags,
            uint32_t *__restrict__ aggN, uint32_t *__restrict__ aggO,
            uint32_t *__restrict__ aggC)
{
    __shared__ tk_v3 ws[TK_THREADS / WAVE];
    const uint32_t tile0 = blockIdx.x * (uint32_t)TK_TILE;
    tk_v3 v = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < TK_ITEMS; k++)
        v = tk_join(v, tk_item<RANK>(flags, tile0 + k * TK_THREADS +
                                                threadIdx.x, m));
    tk_v3 tot;
    tk_block_scan<TK_THREADS>(v, ws, &tot);
    if (threadIdx.x == 0) {
        aggN[blockIdx.x] = tot.mxn;
        aggO[blockIdx.x] = tot.mxo;
        aggC[blockIdx.x] = tot.cnt;
    }
}

/* one workgroup: the tile aggregates become exclusive prefixes in place,
 * TK_SCAN_THREADS tiles per pass with a register carry; *total = the sum */
__global__ __launch_bounds__(TK_SCAN_THREADS) void
k_tk_scan_tiles(const uint32_t ntiles, uint32_t *aggN, uint32_t *aggO,
                uint32_t *aggC, int64_t *total)
{
    __shared__ tk_v3 ws[TK_SCAN_THREADS / WAVE];
    __shared__ tk_v3 inc[TK_SCAN_THREADS];
    tk_v3 run = {0, 0, 0};
    for (uint32_t c0 = 0; c0 < ntiles; c0 += TK_SCAN_THREADS) {
        const uint32_t i = c0 + threadIdx.x;
        tk_v3 v = {0, 0, 0};
        if (i < ntiles) {
            v.mxn = aggN[i];
            v.mxo = aggO[i];
            v.cnt = aggC[i];
        }
        tk_v3 tot;
        inc[threadIdx.x] = tk_block_scan<TK_SCAN_THREADS>(v, ws, &tot);
        __syncthreads();
        /* exclusive: the inclusive value of the tile before this one */
        if (i < ntiles) {
            const tk_v3 zero = {0, 0, 0};
            const tk_v3 ex =
                tk_join(run, threadIdx.x ? inc[threadIdx.x - 1] : zero);
            aggN[i] = ex.mxn;
            aggO[i] = ex.mxo;
            aggC[i] = ex.cnt;
        }
        __syncthreads();   /* inc is rewritten by the next pass */
        run = tk_join(run, tot);
    }
    if (threadIdx.x == 0)
        *total = (int64_t)run.cnt;
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_apply(const uint32_t m, const uint8_t *__restrict__ flags,
           const int64_t *__restrict__ perm, const uint32_t *__restrict__ act,
           const int32_t *__restrict__ kg, const uint32_t *__restrict__ aggN,
           const uint32_t *__restrict__ aggO,
           const uint32_t *__restrict__ aggC, int32_t *__restrict__ gid,
           uint32_t *__restrict__ act_next)
{
    __shared__ tk_v3 ws[TK_THREADS / WAVE];
    const uint32_t tile0 = blockIdx.x * (uint32_t)TK_TILE;
    tk_v3 carry;
    carry.mxn = aggN[blockIdx.x];
    carry.mxo = aggO[blockIdx.x];
    carry.cnt = aggC[blockIdx.x];
    for (int k = 0; k < TK_ITEMS; k++) {
        const uint32_t j = tile0 + k * TK_THREADS + threadIdx.x;
        const tk_v3 v = tk_item<false>(flags, j, m);
        tk_v3 tot;
        const tk_v3 incl =
            tk_join(carry, tk_block_scan<TK_THREADS>(v, ws, &tot));
        if (j < m) {
            const int64_t a = perm[j];
            const uint32_t row = act ? act[a] : (uint32_t)a;
            /* the new groups of an old group keep its place in the order:
             * old id + rows of it that sort before this new group */
            gid[row] = kg[a] + (int32_t)(incl.mxn - incl.mxo);
            if (v.cnt)
                act_next[incl.cnt - 1] = row;   /* cnt: inclusive sum */
        }
        carry = tk_join(carry, tot);
    }
}

/* ---- after the last round ---- */

__global__ __launch_bounds__(TK_THREADS) void
k_tk_fin_init(const uint32_t n, uint32_t *__restrict__ minrow)
{
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < n;
         i += stride)
        minrow[i] = TK_NOROW;
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_fin_mark(const tk_cols *__restrict__ tp, const uint32_t n,
              const int32_t *__restrict__ gid, uint32_t *minrow)
{
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < n;
         i += stride) {
        int64_t local;
        const otbx_textcol c = tk_locate(*tp, (uint32_t)i, &local);
        if (c.nulls && c.nulls[local])
            continue;
        /* an id is a position of the order: below n by construction,
         * checked all the same before it is used as an index. The plain
         * read first: rows arrive roughly in ascending order, so after the
         * first few almost no row can lower the minimum, and a column of 7
         * distinct strings does not send 200 M atomics to 7 addresses
         * (the whole call at 200 M ship modes: 356 ms with an atomic per
         * row, 36 ms with the read). A stale read is only
         * ever too large and costs one atomic more, never a wrong result. */
        const uint32_t g = (uint32_t)gid[i];
        if (g < n && minrow[g] > (uint32_t)i)
            atomicMin(&minrow[g], (uint32_t)i);
    }
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_rank_apply(const uint32_t n, const uint32_t *__restrict__ minrow,
                const uint32_t *__restrict__ aggC, uint32_t *__restrict__ rank,
                int64_t *__restrict__ dict_row)
{
    __shared__ tk_v3 ws[TK_THREADS / WAVE];
    const uint32_t tile0 = blockIdx.x * (uint32_t)TK_TILE;
    uint32_t carry = aggC[blockIdx.x];
    for (int k = 0; k < TK_ITEMS; k++) {
        const uint32_t p = tile0 + k * TK_THREADS + threadIdx.x;
        const tk_v3 v = tk_item<true>(minrow, p, n);
        tk_v3 tot;
        const tk_v3 incl = tk_block_scan<TK_THREADS>(v, ws, &tot);
        if (p < n) {
            const uint32_t r = carry + incl.cnt - v.cnt;
            rank[p] = r;
            if (v.cnt && dict_row)
                dict_row[r] = (int64_t)minrow[p];
        }
        carry += tot.cnt;
    }
}

__global__ __launch_bounds__(TK_THREADS) void
k_tk_codes(const tk_cols *__restrict__ tp, const uint32_t n, const int32_t *__restrict__ gid,
           const uint32_t *__restrict__ rank, int64_t *__restrict__ codes)
{
    const int64_t stride = (int64_t)gridDim.x * TK_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < n;
         i += stride) {
        int64_t local;
        const otbx_textcol c = tk_locate(*tp, (uint32_t)i, &local);
        int64_t code = -1;
        if (!(c.nulls && c.nulls[local])) {
            const uint32_t g = (uint32_t)gid[i];
            code = g < n ? (int64_t)rank[g] : -1;
        }
        codes[i] = code;
    }
}

/* ---- host side ---- */

struct tk_layout {
    size_t sort, perm, chunk, kg, gid, actA, actB, lc, nl, flags, aggN, aggO,
        aggC, total;
    size_t sort_bytes;
    uint32_t ntiles;
};

/* After the last round chunk and perm are dead: minrow (u32) lives in
 * chunk's 8 bytes per row, rank (u32) in perm's. */
static bool tk_plan_layout(int64_t n, tk_layout *L)
{
    size_t sb = 0;
    if (otbx_sort_workspace_bytes(n, 3, 0, &sb) != OTBX_OK)
        return false;
    const size_t un = (size_t)n;
    L->sort_bytes = sb;
    L->ntiles = (uint32_t)((n + TK_TILE - 1) / TK_TILE);
    size_t o = TK_HEADER_BYTES;
    L->sort = o;  o += align256_sz(sb);
    L->perm = o;  o += align256_sz(un * 8);
    L->chunk = o; o += align256_sz(un * 8);
    L->kg = o;    o += align256_sz(un * 4);
    L->gid = o;   o += align256_sz(un * 4);
    L->actA = o;  o += align256_sz(un * 4);
    L->actB = o;  o += align256_sz(un * 4);
    L->lc = o;    o += align256_sz(un);
    L->nl = o;    o += align256_sz(un);
    L->flags = o; o += align256_sz(un);
    L->aggN = o;  o += align256_sz((size_t)L->ntiles * 4);
    L->aggO = o;  o += align256_sz((size_t)L->ntiles * 4);
    L->aggC = o;  o += align256_sz((size_t)L->ntiles * 4);
    L->total = o;
    return true;
}

extern "C" {

otbx_status otbx_text_rank_workspace_bytes(int64_t n_total, size_t *bytes)
{
    if (!bytes || n_total < 0 || n_total > INT32_MAX)
        return OTBX_ERR_INVALID;
    tk_layout L;
    if (!tk_plan_layout(n_total, &L))
        return OTBX_ERR_INVALID;
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_text_rank(const otbx_textset *ts, void *ws_dev,
                           size_t ws_bytes, int64_t *codes_dev,
                           int64_t *dict_row_dev, int64_t *ndistinct_dev,
                           int32_t *rounds_host, void *stream)
{
    /* argument checks first: nothing in this block touches HIP */
    if (!ts || !ndistinct_dev)
        return OTBX_ERR_INVALID;
    if (ts->ncols < 1 || ts->ncols > OTBX_MAX_TEXT_RANK_COLS)
        return OTBX_ERR_INVALID;
    int64_t n = 0;
    bool anynull = false;
    tk_cols t;
    memset(&t, 0, sizeof t);
    for (int c = 0; c < ts->ncols; c++) {
        if (ts->n[c] < 0 || ts->n[c] > INT32_MAX)
            return OTBX_ERR_INVALID;
        if (!txt_col_ok(&ts->col[c], ts->n[c]))
            return OTBX_ERR_INVALID;
        t.col[c] = ts->col[c];
        t.start[c] = n;
        n += ts->n[c];
        anynull = anynull || (ts->n[c] > 0 && ts->col[c].nulls);
    }
    if (n > INT32_MAX)
        return OTBX_ERR_INVALID;
    for (int c = ts->ncols; c < OTBX_MAX_TEXT_RANK_COLS; c++)
        t.start[c] = n;
    if (n > 0 && !codes_dev)
        return OTBX_ERR_INVALID;
    tk_layout L;
    if (!tk_plan_layout(n, &L))
        return OTBX_ERR_INVALID;
    if (ws_bytes < L.total || !ws_dev || ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    if (rounds_host)
        *rounds_host = 0;
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(ndistinct_dev, 0, 8, s));
        HIP_CHECK(hipStreamSynchronize(s));
        return OTBX_OK;
    }

    char *w = (char *)ws_dev;
    int64_t *nact_dev = (int64_t *)w;       /* rows still undecided */
    int64_t *nout_dev = (int64_t *)w + 1;   /* the sort's row count */
    const tk_cols *t_dev = (const tk_cols *)(w + TK_COLS_OFFSET);
    HIP_CHECK(hipMemcpyAsync(w + TK_COLS_OFFSET, &t, sizeof t,
                             hipMemcpyHostToDevice, s));
    void *sortws = w + L.sort;
    int64_t *perm = (int64_t *)(w + L.perm);
    int64_t *chunk = (int64_t *)(w + L.chunk);
    int32_t *kg = (int32_t *)(w + L.kg);
    int32_t *gid = (int32_t *)(w + L.gid);
    uint32_t *act[2] = {(uint32_t *)(w + L.actA), (uint32_t *)(w + L.actB)};
    uint8_t *lc = (uint8_t *)(w + L.lc);
    uint8_t *nl = (uint8_t *)(w + L.nl);
    uint8_t *flags = (uint8_t *)(w + L.flags);
    uint32_t *aggN = (uint32_t *)(w + L.aggN);
    uint32_t *aggO = (uint32_t *)(w + L.aggO);
    uint32_t *aggC = (uint32_t *)(w + L.aggC);

    int64_t m = n;
    int round = 0;
    while (m > 0) {
        const uint32_t um = (uint32_t)m;
        const uint32_t *cur = round ? act[round & 1] : nullptr;
        uint32_t *next = act[(round + 1) & 1];
        uint8_t *rnl = round == 0 && anynull ? nl : nullptr;
        const dim3 g1((uint32_t)grid_for(m, TK_THREADS));
        const uint32_t ntiles = (uint32_t)((m + TK_TILE - 1) / TK_TILE);

        hipLaunchKernelGGL(k_tk_extract, g1, dim3(TK_THREADS), 0, s, t_dev, cur,
                           um, round, (const int32_t *)gid, kg, chunk, lc,
                           rnl);
        HIP_CHECK(hipGetLastError());

        /* (group id, chunk, lencode); round 0 has one group, so the id is
         * a key only where it carries the null mask */
        otbx_sortspec sp;
        memset(&sp, 0, sizeof sp);
        int nk = 0;
        if (round > 0 || rnl) {
            sp.key[nk].col = kg;
            sp.key[nk].nulls = rnl;
            sp.key[nk].type = OTBX_SORT_I32;
            nk++;
        }
        sp.key[nk].col = chunk;
        sp.key[nk].type = OTBX_SORT_I64;
        nk++;
        sp.key[nk].col = lc;
        sp.key[nk].type = OTBX_SORT_U8;
        nk++;
        sp.nkeys = nk;
        const otbx_status st = otbx_sort_perm(&sp, m, 0, sortws, L.sort_bytes,
                                              perm, nout_dev, stream);
        if (st != OTBX_OK)
            return st;

        hipLaunchKernelGGL(k_tk_flags, g1, dim3(TK_THREADS), 0, s, um,
                           (const int64_t *)perm, (const int32_t *)kg,
                           (const int64_t *)chunk, (const uint8_t *)lc,
                           (const uint8_t *)rnl, flags);
        hipLaunchKernelGGL(k_tk_reduce<false>, dim3(ntiles), dim3(TK_THREADS),
                           0, s, um, (const void *)flags, aggN, aggO, aggC);
        hipLaunchKernelGGL(k_tk_scan_tiles, dim3(1), dim3(TK_SCAN_THREADS), 0,
                           s, ntiles, aggN, aggO, aggC, nact_dev);
        hipLaunchKernelGGL(k_tk_apply, dim3(ntiles), dim3(TK_THREADS), 0, s,
                           um, (const uint8_t *)flags, (const int64_t *)perm,
                           cur, (const int32_t *)kg, (const uint32_t *)aggN,
                           (const uint32_t *)aggO, (const uint32_t *)aggC, gid,
                           next);
        HIP_CHECK(hipGetLastError());
        int64_t nact = 0;
        HIP_CHECK(hipMemcpyAsync(&nact, nact_dev, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        /* every round decides at least the rows that end inside its chunk;
         * a count that does not fit the input is not ours */
        if (nact < 0 || nact > m)
            return OTBX_ERR_HIP;
        m = nact;
        round++;
    }
    if (rounds_host)
        *rounds_host = round;

    const uint32_t un = (uint32_t)n;
    uint32_t *minrow = (uint32_t *)chunk;
    uint32_t *rank = (uint32_t *)perm;
    const dim3 gn((uint32_t)grid_for(n, TK_THREADS));
    hipLaunchKernelGGL(k_tk_fin_init, gn, dim3(TK_THREADS), 0, s, un, minrow);
    hipLaunchKernelGGL(k_tk_fin_mark, gn, dim3(TK_THREADS), 0, s, t_dev, un,
                       (const int32_t *)gid, minrow);
    hipLaunchKernelGGL(k_tk_reduce<true>, dim3(L.ntiles), dim3(TK_THREADS), 0,
                       s, un, (const void *)minrow, aggN, aggO, aggC);
    hipLaunchKernelGGL(k_tk_scan_tiles, dim3(1), dim3(TK_SCAN_THREADS), 0, s,
                       L.ntiles, aggN, aggO, aggC, ndistinct_dev);
    hipLaunchKernelGGL(k_tk_rank_apply, dim3(L.ntiles), dim3(TK_THREADS), 0, s,
                       un, (const uint32_t *)minrow, (const uint32_t *)aggC,
                       rank, dict_row_dev);
    hipLaunchKernelGGL(k_tk_codes, gn, dim3(TK_THREADS), 0, s, t_dev, un,
                       (const int32_t *)gid, (const uint32_t *)rank,
                       codes_dev);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    return OTBX_OK;
}

} /* extern "C" */

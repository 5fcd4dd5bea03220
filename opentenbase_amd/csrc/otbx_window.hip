/*
 * otbx_window.hip — the GPU WindowAgg operator (otbx_window): ranking
 * functions and running aggregates over sorted input. The ExecWindowAgg
 * analog (executor/nodeWindowAgg.c; window_row_number / window_rank /
 * window_dense_rank, utils/adt/windowfuncs.c:82/98/118; are_peers
 * nodeWindowAgg.c:2960; the default frame RANGE BETWEEN UNBOUNDED PRECEDING
 * AND CURRENT ROW, row_is_in_frame :1472). DESIGN.md §8h.
 *
 * Input is the permutation otbx_sort_perm produced for (partition keys,
 * order keys). Everything is stream-ordered, four kernels, and kernel
 * boundaries are the only ordering between workgroups:
 *   k_win_flags  — per sorted position: gather the normalised keys through
 *                  perm (ss_norm, the sort's own key), compare with the left
 *                  neighbour (wave shuffle; LDS across waves; only the first
 *                  row of a tile gathers perm[j-1]) → partition-start and
 *                  peer-start bits, plus the value's non-NULL bit and the
 *                  gathered value. Also reduces the tile to a win_tile
 *                  aggregate.
 *   k_win_mid    — one workgroup scans the tile aggregates, WIN_MID_THREADS
 *                  tiles per pass with a running carry: forward with the
 *                  segmented-scan operator (win_comb), backward a min-scan
 *                  of the first partition / peer start of each tile.
 *   k_win_apply  — per tile, WIN_ITEMS consecutive positions per thread:
 *                  max-scan of partition and peer starts, segmented counts
 *                  of peer starts and non-NULL values and the segmented
 *                  double sum in one register pass, seeded with the tile's
 *                  carry; the reverse min-scan gives the frame end and the
 *                  partition end. Writes the position-only outputs, and the
 *                  running count / sum / frame end to the workspace.
 *   k_win_frame  — count(v) / sum(v): every row reads the running values at
 *                  its frame end, so all peers hold identical bits.
 * The sum is SEGMENTED: win_comb drops the left operand at a partition
 * start, so no value of one partition ever reaches another one.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm: the normalised key */

#define WIN_THREADS 256
#define WIN_WAVES (WIN_THREADS / WAVE)
#define WIN_ITEMS 16
#define WIN_TILE (WIN_THREADS * WIN_ITEMS)   /* 4096 positions per tile */
#define WIN_MID_THREADS 1024                 /* tiles per pass of k_win_mid */
#define WIN_MID_WAVES (WIN_MID_THREADS / WAVE)
#define WIN_NONE INT_MAX                     /* "no start" for the min-scans */

/* per-position flag byte */
#define WIN_FP 1u   /* first row of a partition  */
#define WIN_FG 2u   /* first row of a peer group */
#define WIN_FV 4u   /* value is not NULL         */

/* requested outputs */
#define WIN_O_ROWNUM 1u
#define WIN_O_RANK 2u
#define WIN_O_DENSE 4u
#define WIN_O_CSTAR 8u
#define WIN_O_CNTV 16u
#define WIN_O_SUM 32u
#define WIN_O_PROWS 64u

/* the summary of a run of positions: lastP / lastG = last partition / peer
 * start inside it (-1: none); dc / vc / vs = peer starts, non-NULL values and
 * their sum from lastP on (from the run's first position if lastP < 0) */
struct win_agg {
    int32_t lastP, lastG;
    uint32_t dc, vc;
    double vs;
};

/* per tile: its aggregate and its first partition / peer start (WIN_NONE:
 * none). In the carry table the same struct holds what a tile starts from:
 * f = everything to its left, firstP / firstG = the next start to its right */
struct win_tile {
    win_agg f;
    int32_t firstP, firstG;
};
static_assert(sizeof(win_tile) == 32, "win_tile layout");

/* -0.0 is the identity of IEEE addition (-0.0 + x == x for every x, -0.0
 * included), so a frame of -0.0 values still sums to -0.0 as float8pl does */
__device__ __forceinline__ win_agg win_identity()
{
    win_agg r;
    r.lastP = -1;
    r.lastG = -1;
    r.dc = 0;
    r.vc = 0;
    r.vs = -0.0;
    return r;
}

/* the segmented-scan operator: a is the run to the left of b */
__device__ __forceinline__ win_agg win_comb(const win_agg &a, const win_agg &b)
{
    const bool cut = b.lastP >= 0;
    win_agg r;
    r.lastP = cut ? b.lastP : a.lastP;
    r.lastG = b.lastG >= 0 ? b.lastG : a.lastG;
    r.dc = cut ? b.dc : a.dc + b.dc;
    r.vc = cut ? b.vc : a.vc + b.vc;
    r.vs = cut ? b.vs : a.vs + b.vs;
    return r;
}

__device__ __forceinline__ win_agg win_shfl_up(const win_agg &a, int o)
{
    win_agg r;
    r.lastP = __shfl_up(a.lastP, o);
    r.lastG = __shfl_up(a.lastG, o);
    r.dc = __shfl_up(a.dc, o);
    r.vc = __shfl_up(a.vc, o);
    r.vs = __shfl_up(a.vs, o);
    return r;
}

/* block-wide exclusive win_comb scan of one aggregate per thread (NW waves);
 * *total gets the whole block. wtot: NW LDS entries, reusable after return */
template <int NW>
__device__ __forceinline__ win_agg win_block_excl_scan(const win_agg &v,
                                                       win_agg *wtot,
                                                       win_agg *total)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    win_agg incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const win_agg t = win_shfl_up(incl, o);
        if (lane >= o)
            incl = win_comb(t, incl);
    }
    if (lane == WAVE - 1)
        wtot[wid] = incl;
    __syncthreads();
    win_agg pre = win_identity(), tot = win_identity();
    for (int w = 0; w < NW; w++) {
        const win_agg s = wtot[w];
        if (w < wid)
            pre = win_comb(pre, s);
        tot = win_comb(tot, s);
    }
    __syncthreads();
    win_agg excl = win_shfl_up(incl, 1);
    if (lane == 0)
        excl = win_identity();
    *total = tot;
    return win_comb(pre, excl);
}

/* block-wide exclusive min-scan of an int32 pair per thread; REV scans from
 * the last thread down (each thread gets the min over the threads after
 * it). *ta / *tb get the block minima. wa, wb: NW LDS words each */
template <int NW, bool REV>
__device__ __forceinline__ void win_block_excl_min2(int32_t *a, int32_t *b,
                                                    int32_t *wa, int32_t *wb,
                                                    int32_t *ta, int32_t *tb)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    int32_t ia = *a, ib = *b;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int32_t xa = REV ? __shfl_down(ia, o) : __shfl_up(ia, o);
        const int32_t xb = REV ? __shfl_down(ib, o) : __shfl_up(ib, o);
        if (REV ? lane + o < WAVE : lane >= o) {
            ia = min(ia, xa);
            ib = min(ib, xb);
        }
    }
    if (lane == (REV ? 0 : WAVE - 1)) {
        wa[wid] = ia;
        wb[wid] = ib;
    }
    __syncthreads();
    int32_t pa = WIN_NONE, pb = WIN_NONE, alla = WIN_NONE, allb = WIN_NONE;
    for (int w = 0; w < NW; w++) {
        const int32_t xa = wa[w], xb = wb[w];
        if (REV ? w > wid : w < wid) {
            pa = min(pa, xa);
            pb = min(pb, xb);
        }
        alla = min(alla, xa);
        allb = min(allb, xb);
    }
    __syncthreads();
    int32_t ea = REV ? __shfl_down(ia, 1) : __shfl_up(ia, 1);
    int32_t eb = REV ? __shfl_down(ib, 1) : __shfl_up(ib, 1);
    if (lane == (REV ? WAVE - 1 : 0)) {
        ea = WIN_NONE;
        eb = WIN_NONE;
    }
    *a = min(pa, ea);
    *b = min(pb, eb);
    *ta = alla;
    *tb = allb;
}

/* row of sorted position p; a perm entry outside [0, n) is clamped so that a
 * broken permutation can never index outside the columns */
__device__ __forceinline__ uint32_t win_row(const int64_t *perm, uint32_t p,
                                            uint32_t n)
{
    if (!perm)
        return p;
    const int64_t r = perm[p];
    return r < 0 ? 0u : (r >= (int64_t)n ? n - 1 : (uint32_t)r);
}

/* ---- flags + tile aggregate ----
 * item i of thread t is position tile0 + i*WIN_THREADS + t, so the perm loads
 * and the flag / value stores are coalesced and the left neighbour of a
 * position sits one lane down in the same item. want: 0 = ranking only
 * (vals untouched), 1 = non-NULL bits only, 2 = values too. */
__global__ __launch_bounds__(WIN_THREADS) void
k_win_flags(const otbx_sortspec spec, const int npart, const int64_t *perm,
            const uint32_t n, const double *vals, const uint8_t *vnull,
            const int want, uint8_t *flags, double *sval, win_tile *tiles)
{
    __shared__ unsigned long long sk[WIN_ITEMS][WIN_WAVES];
    __shared__ uint32_t snd[WIN_WAVES];
    __shared__ int32_t rlP[WIN_WAVES], rlG[WIN_WAVES], rfP[WIN_WAVES],
        rfG[WIN_WAVES];
    __shared__ uint32_t rdc[WIN_WAVES], rvc[WIN_WAVES];
    __shared__ double rvs[WIN_WAVES];

    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile0 = blockIdx.x * (uint32_t)WIN_TILE;

    uint32_t row[WIN_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        const uint32_t p = tile0 + i * WIN_THREADS + threadIdx.x;
        const bool v = p < n;
        valid |= (v ? 1u : 0u) << i;
        row[i] = v ? win_row(perm, p, n) : 0u;
    }
    const bool edge = threadIdx.x == 0 && tile0 > 0;  /* reads perm[tile0-1] */
    const uint32_t lrow = edge ? win_row(perm, tile0 - 1, n) : 0u;

    uint32_t pbits = 0, gbits = 0;   /* item differs from its left neighbour */
#pragma unroll
    for (int c = 0; c < OTBX_MAX_KEYS; c++) {
        if (c >= spec.nkeys)
            break;
        unsigned long long k[WIN_ITEMS];
        uint32_t ndm = 0;
#pragma unroll
        for (int i = 0; i < WIN_ITEMS; i++) {
            uint32_t nd = 0;
            k[i] = ((valid >> i) & 1u) ? ss_norm(spec.key[c], row[i], &nd)
                                       : 0ull;
            ndm |= nd << i;
        }
        unsigned long long k0left = 0;
        uint32_t nd0left = 0;
        if (edge)
            k0left = ss_norm(spec.key[c], lrow, &nd0left);
        if (lane == WAVE - 1) {
#pragma unroll
            for (int i = 0; i < WIN_ITEMS; i++)
                sk[i][wid] = k[i];
            snd[wid] = ndm;
        }
        __syncthreads();
        const uint32_t lndm = __shfl_up(ndm, 1);
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < WIN_ITEMS; i++) {
            unsigned long long lk = __shfl_up(k[i], 1);
            uint32_t lnd = (lndm >> i) & 1u;
            if (lane == 0) {
                if (wid > 0) {
                    lk = sk[i][wid - 1];
                    lnd = (snd[wid - 1] >> i) & 1u;
                } else if (i > 0) {
                    lk = sk[i - 1][WIN_WAVES - 1];
                    lnd = (snd[WIN_WAVES - 1] >> (i - 1)) & 1u;
                } else {
                    lk = k0left;
                    lnd = nd0left;
                }
            }
            const bool d = lk != k[i] || lnd != ((ndm >> i) & 1u);
            diff |= (d ? 1u : 0u) << i;
        }
        if (c < npart)
            pbits |= diff;
        gbits |= diff;
        __syncthreads();
    }
    if (tile0 == 0 && threadIdx.x == 0)
        pbits |= 1u;                 /* position 0 starts everything */
    pbits &= valid;
    gbits = (gbits | pbits) & valid;

    uint32_t vbits = 0;
    double v[WIN_ITEMS];
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        v[i] = -0.0;
        if (want && ((valid >> i) & 1u)) {
            const bool nonnull = !(vnull && vnull[row[i]]);
            vbits |= (nonnull ? 1u : 0u) << i;
            if (want == 2 && nonnull)
                v[i] = vals[row[i]];
        }
    }
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        if ((valid >> i) & 1u) {
            const uint32_t p = tile0 + i * WIN_THREADS + threadIdx.x;
            flags[p] = (uint8_t)((((pbits >> i) & 1u) ? WIN_FP : 0u) |
                                 (((gbits >> i) & 1u) ? WIN_FG : 0u) |
                                 (((vbits >> i) & 1u) ? WIN_FV : 0u));
            if (want == 2)
                sval[p] = v[i];
        }
    }

    /* tile aggregate, step 1: last / first partition and peer start */
    int32_t lP = -1, lG = -1, fP = WIN_NONE, fG = WIN_NONE;
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        const int32_t p = (int32_t)(tile0 + i * WIN_THREADS + threadIdx.x);
        if ((pbits >> i) & 1u) {
            lP = max(lP, p);
            fP = min(fP, p);
        }
        if ((gbits >> i) & 1u) {
            lG = max(lG, p);
            fG = min(fG, p);
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        lP = max(lP, __shfl_xor(lP, o));
        lG = max(lG, __shfl_xor(lG, o));
        fP = min(fP, __shfl_xor(fP, o));
        fG = min(fG, __shfl_xor(fG, o));
    }
    if (lane == 0) {
        rlP[wid] = lP;
        rlG[wid] = lG;
        rfP[wid] = fP;
        rfG[wid] = fG;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WIN_WAVES; w++) {
        lP = max(lP, rlP[w]);
        lG = max(lG, rlG[w]);
        fP = min(fP, rfP[w]);
        fG = min(fG, rfG[w]);
    }
    /* step 2: counts and sum over the positions from the last partition
     * start on (the whole tile if it holds none) */
    uint32_t dc = 0, vc = 0;
    double vs = -0.0;
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        const int32_t p = (int32_t)(tile0 + i * WIN_THREADS + threadIdx.x);
        if (((valid >> i) & 1u) && p >= lP) {
            dc += (gbits >> i) & 1u;
            vc += (vbits >> i) & 1u;
            vs += v[i];
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        dc += __shfl_xor(dc, o);
        vc += __shfl_xor(vc, o);
        vs += __shfl_xor(vs, o);
    }
    if (lane == 0) {
        rdc[wid] = dc;
        rvc[wid] = vc;
        rvs[wid] = vs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        win_tile t;
        t.f.lastP = lP;
        t.f.lastG = lG;
        t.f.dc = 0;
        t.f.vc = 0;
        t.f.vs = -0.0;
        for (int w = 0; w < WIN_WAVES; w++) {
            t.f.dc += rdc[w];
            t.f.vc += rvc[w];
            t.f.vs += rvs[w];
        }
        t.firstP = fP;
        t.firstG = fG;
        tiles[blockIdx.x] = t;
    }
}

/* ---- scan of the tile aggregates: one workgroup, WIN_MID_THREADS tiles per
 * pass, the running carry in registers between passes ---- */
__global__ __launch_bounds__(WIN_MID_THREADS) void
k_win_mid(const win_tile *__restrict__ tiles, win_tile *__restrict__ carry,
          const uint32_t ntiles, const uint32_t n)
{
    __shared__ win_agg wtot[WIN_MID_WAVES];
    __shared__ int32_t wa[WIN_MID_WAVES], wb[WIN_MID_WAVES];

    win_agg run = win_identity();
    for (uint32_t c0 = 0; c0 < ntiles; c0 += WIN_MID_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const win_agg v = idx < ntiles ? tiles[idx].f : win_identity();
        win_agg tot;
        const win_agg ex = win_block_excl_scan<WIN_MID_WAVES>(v, wtot, &tot);
        if (idx < ntiles)
            carry[idx].f = win_comb(run, ex);
        run = win_comb(run, tot);
    }
    /* next start to the right of each tile: thread order = tiles from the
     * last one down; past the last tile the next start is n */
    int32_t runP = (int32_t)n, runG = (int32_t)n;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += WIN_MID_THREADS) {
        const uint32_t j = c0 + threadIdx.x;
        const bool in = j < ntiles;
        const uint32_t idx = in ? ntiles - 1 - j : 0;
        int32_t a = in ? tiles[idx].firstP : WIN_NONE;
        int32_t b = in ? tiles[idx].firstG : WIN_NONE;
        int32_t ta, tb;
        win_block_excl_min2<WIN_MID_WAVES, false>(&a, &b, wa, wb, &ta, &tb);
        if (in) {
            carry[idx].firstP = min(runP, a);
            carry[idx].firstG = min(runG, b);
        }
        runP = min(runP, ta);
        runG = min(runG, tb);
    }
}

/* coalesced store of one int64 per tile position from the blocked layout
 * (thread t holds positions t*WIN_ITEMS ..): staged through LDS, rows padded
 * by one slot so that neither side has a bank conflict */
#define WIN_STAGE (WIN_TILE + WIN_THREADS)
__device__ __forceinline__ void win_store(int64_t *dst, uint32_t tile0,
                                          uint32_t n,
                                          const int64_t (&x)[WIN_ITEMS],
                                          int64_t *stage)
{
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++)
        stage[threadIdx.x * (WIN_ITEMS + 1) + i] = x[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        const uint32_t q = i * WIN_THREADS + threadIdx.x;
        const uint32_t p = tile0 + q;
        if (p < n)
            dst[p] = stage[q + q / WIN_ITEMS];
    }
    __syncthreads();
}

/* ---- the scans, applied per tile ----
 * thread t holds positions tile0 + t*WIN_ITEMS .. +WIN_ITEMS-1 */
__global__ __launch_bounds__(WIN_THREADS) void
k_win_apply(const uint8_t *__restrict__ flags, double *sval,
            const win_tile *__restrict__ carry, const uint32_t n,
            const uint32_t mask, const otbx_window_out out,
            uint32_t *__restrict__ rcnt, uint32_t *__restrict__ fendw)
{
    __shared__ win_agg wtot[WIN_WAVES];
    __shared__ int32_t wa[WIN_WAVES], wb[WIN_WAVES];
    __shared__ int64_t stage[WIN_STAGE];

    const uint32_t tile0 = blockIdx.x * (uint32_t)WIN_TILE;
    const uint32_t p0 = tile0 + threadIdx.x * WIN_ITEMS;
    const bool frame = (mask & (WIN_O_CNTV | WIN_O_SUM)) != 0;
    const bool sums = (mask & WIN_O_SUM) != 0;

    /* the flag and value arrays are padded to whole tiles: the vector loads
     * stay inside them, and what lies past n is masked here */
    uint32_t f[WIN_ITEMS];
    {
        const uint4 w = *(const uint4 *)(flags + p0);
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < WIN_ITEMS; i++)
            f[i] = p0 + i < n ? (ww[i / 4] >> (8 * (i % 4))) & 0xffu : 0u;
    }
    double v[WIN_ITEMS];
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i += 2) {
        double2 d = make_double2(-0.0, -0.0);
        if (sums)
            d = *(const double2 *)(sval + p0 + i);
        v[i] = p0 + i < n ? d.x : -0.0;
        v[i + 1] = p0 + i + 1 < n ? d.y : -0.0;
    }
    const win_tile cin = carry[blockIdx.x];

    /* reverse: next peer / partition start after each position */
    int32_t nP = WIN_NONE, nG = WIN_NONE;
#pragma unroll
    for (int i = WIN_ITEMS - 1; i >= 0; i--) {
        if (f[i] & WIN_FP)
            nP = (int32_t)(p0 + i);
        if (f[i] & WIN_FG)
            nG = (int32_t)(p0 + i);
    }
    int32_t ta, tb;
    win_block_excl_min2<WIN_WAVES, true>(&nP, &nG, wa, wb, &ta, &tb);
    nP = min(nP, cin.firstP);
    nG = min(nG, cin.firstG);
    int32_t fend[WIN_ITEMS], pend[WIN_ITEMS];
#pragma unroll
    for (int i = WIN_ITEMS - 1; i >= 0; i--) {
        fend[i] = nG - 1;
        pend[i] = nP - 1;
        if (f[i] & WIN_FP)
            nP = (int32_t)(p0 + i);
        if (f[i] & WIN_FG)
            nG = (int32_t)(p0 + i);
    }

    /* forward: the thread's own aggregate, the block scan, then the values */
    win_agg a = win_identity();
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        if (f[i] & WIN_FP) {
            a.lastP = (int32_t)(p0 + i);
            a.dc = 0;
            a.vc = 0;
            a.vs = -0.0;
        }
        if (f[i] & WIN_FG) {
            a.lastG = (int32_t)(p0 + i);
            a.dc++;
        }
        a.vc += (f[i] & WIN_FV) ? 1u : 0u;
        a.vs += v[i];
    }
    win_agg tot;
    const win_agg ex = win_block_excl_scan<WIN_WAVES>(a, wtot, &tot);
    a = win_comb(cin.f, ex);

    int64_t rn[WIN_ITEMS], rk[WIN_ITEMS], dr[WIN_ITEMS], cs[WIN_ITEMS],
        pr[WIN_ITEMS];
    uint32_t rc[WIN_ITEMS];
#pragma unroll
    for (int i = 0; i < WIN_ITEMS; i++) {
        const int32_t p = (int32_t)(p0 + i);
        if (f[i] & WIN_FP) {
            a.lastP = p;
            a.dc = 0;
            a.vc = 0;
            a.vs = -0.0;
        }
        if (f[i] & WIN_FG) {
            a.lastG = p;
            a.dc++;
        }
        a.vc += (f[i] & WIN_FV) ? 1u : 0u;
        a.vs += v[i];
        rn[i] = (int64_t)p - a.lastP + 1;
        rk[i] = (int64_t)a.lastG - a.lastP + 1;
        dr[i] = (int64_t)a.dc;
        cs[i] = (int64_t)fend[i] - a.lastP + 1;
        pr[i] = (int64_t)pend[i] - a.lastP + 1;
        rc[i] = a.vc;
        v[i] = a.vs;
    }
    if (frame) {
        /* workspace arrays are 256-byte aligned and padded to whole tiles */
#pragma unroll
        for (int i = 0; i < WIN_ITEMS; i += 4) {
            *(uint4 *)(rcnt + p0 + i) =
                make_uint4(rc[i], rc[i + 1], rc[i + 2], rc[i + 3]);
            *(uint4 *)(fendw + p0 + i) =
                make_uint4((uint32_t)fend[i], (uint32_t)fend[i + 1],
                           (uint32_t)fend[i + 2], (uint32_t)fend[i + 3]);
        }
        if (sums) {
#pragma unroll
            for (int i = 0; i < WIN_ITEMS; i += 2)
                *(double2 *)(sval + p0 + i) = make_double2(v[i], v[i + 1]);
        }
    }
    if (mask & WIN_O_ROWNUM)
        win_store(out.row_number, tile0, n, rn, stage);
    if (mask & WIN_O_RANK)
        win_store(out.rank, tile0, n, rk, stage);
    if (mask & WIN_O_DENSE)
        win_store(out.dense_rank, tile0, n, dr, stage);
    if (mask & WIN_O_CSTAR)
        win_store(out.count_star, tile0, n, cs, stage);
    if (mask & WIN_O_PROWS)
        win_store(out.part_rows, tile0, n, pr, stage);
}

/* ---- count(v) / sum(v): read the running values at the frame end ---- */
__global__ __launch_bounds__(WIN_THREADS) void
k_win_frame(const uint32_t *__restrict__ fendw,
            const uint32_t *__restrict__ rcnt, const double *__restrict__ rsum,
            const uint32_t n, const uint32_t mask, const otbx_window_out out)
{
    const uint32_t p = blockIdx.x * (uint32_t)WIN_THREADS + threadIdx.x;
    if (p >= n)
        return;
    uint32_t e = fendw[p];
    e = e < n ? e : n - 1;
    const uint32_t c = rcnt[e];
    if (mask & WIN_O_CNTV)
        out.count_v[p] = (int64_t)c;
    if (mask & WIN_O_SUM) {
        out.sum_v[p] = c ? rsum[e] : 0.0;
        out.sum_isnull[p] = c ? 0 : 1;
    }
}

/* ---- host side ---- */

struct win_layout {
    size_t flags, sval, rcnt, fend, tiles, carry, total;
    uint32_t ntiles;
};

static void win_plan_layout(int64_t n, win_layout *L)
{
    L->ntiles = (uint32_t)((n + WIN_TILE - 1) / WIN_TILE);
    const size_t padded = (size_t)L->ntiles * WIN_TILE;
    size_t o = 0;
    L->flags = o; o += align256_sz(padded);
    L->sval = o;  o += align256_sz(padded * 8);
    L->rcnt = o;  o += align256_sz(padded * 4);
    L->fend = o;  o += align256_sz(padded * 4);
    L->tiles = o; o += align256_sz((size_t)L->ntiles * sizeof(win_tile));
    L->carry = o; o += align256_sz((size_t)L->ntiles * sizeof(win_tile));
    L->total = o;
}

extern "C" {

otbx_status otbx_window_workspace_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    win_layout L;
    win_plan_layout(n, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_window(const otbx_sortspec *spec, int32_t npart,
                        const int64_t *perm_dev, int64_t n,
                        const double *vals_dev, const uint8_t *val_null_dev,
                        void *ws_dev, size_t ws_bytes,
                        const otbx_window_out *out, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!spec || !out)
        return OTBX_ERR_INVALID;
    if (spec->nkeys < 0 || spec->nkeys > OTBX_MAX_KEYS)
        return OTBX_ERR_INVALID;
    if (npart < 0 || npart > spec->nkeys)
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
    const uint32_t mask = (out->row_number ? WIN_O_ROWNUM : 0u) |
                          (out->rank ? WIN_O_RANK : 0u) |
                          (out->dense_rank ? WIN_O_DENSE : 0u) |
                          (out->count_star ? WIN_O_CSTAR : 0u) |
                          (out->count_v ? WIN_O_CNTV : 0u) |
                          (out->sum_v ? WIN_O_SUM : 0u) |
                          (out->part_rows ? WIN_O_PROWS : 0u);
    if (!mask && !out->sum_isnull)
        return OTBX_ERR_INVALID;
    if ((out->sum_v != nullptr) != (out->sum_isnull != nullptr))
        return OTBX_ERR_INVALID;
    const bool frame = (mask & (WIN_O_CNTV | WIN_O_SUM)) != 0;
    if (frame && !vals_dev)
        return OTBX_ERR_INVALID;
    win_layout L;
    win_plan_layout(n, &L);
    /* the kernels read and write the workspace with 16-byte vectors */
    if (ws_bytes < L.total || (L.total > 0 && !ws_dev) ||
        ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;
    if (n == 0)
        return OTBX_OK;

    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws_dev;
    uint8_t *flags = (uint8_t *)(w + L.flags);
    double *sval = (double *)(w + L.sval);
    uint32_t *rcnt = (uint32_t *)(w + L.rcnt);
    uint32_t *fend = (uint32_t *)(w + L.fend);
    win_tile *tiles = (win_tile *)(w + L.tiles);
    win_tile *carry = (win_tile *)(w + L.carry);
    const uint32_t un = (uint32_t)n;
    const int want = (mask & WIN_O_SUM) ? 2 : (frame ? 1 : 0);

    hipLaunchKernelGGL(k_win_flags, dim3(L.ntiles), dim3(WIN_THREADS), 0, s,
                       *spec, (int)npart, perm_dev, un, vals_dev, val_null_dev,
                       want, flags, sval, tiles);
    hipLaunchKernelGGL(k_win_mid, dim3(1), dim3(WIN_MID_THREADS), 0, s, tiles,
                       carry, L.ntiles, un);
    hipLaunchKernelGGL(k_win_apply, dim3(L.ntiles), dim3(WIN_THREADS), 0, s,
                       flags, sval, carry, un, mask, *out, rcnt, fend);
    if (frame)
        hipLaunchKernelGGL(k_win_frame,
                           dim3((un + WIN_THREADS - 1) / WIN_THREADS),
                           dim3(WIN_THREADS), 0, s, fend, rcnt, sval, un, mask,
                           *out);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

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
 *
 * The second half of the file is otbx_window_frame: explicit ROWS / RANGE
 * frames with lag / lead, ntile, the value functions and count / sum / min /
 * max, built on the first three kernels above.
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

/* ======================================================================
 * otbx_window_frame — lag / lead, ntile, value functions and aggregates
 * over an explicit ROWS / RANGE frame. DESIGN.md §8n.
 *
 * The partition / peer bounds come from the kernels above, asked for
 * row_number and part_rows (plus rank / count_star for a RANGE CURRENT
 * bound): ps = j - row_number + 1, pe = ps + part_rows - 1,
 * gs = ps + rank - 1, ge = ps + count_star - 1. Then, per function call:
 *   k_wf_pos     — NTILE, LAG / LEAD, FIRST / LAST / NTH_VALUE, COUNT_STAR:
 *                  one pass, the source row gathered through perm.
 *   k_wf_gather  — an aggregate's input in sorted order: 64-bit value (0
 *                  under NULL) and a non-NULL byte.
 *   k_wf_direct  — bounded ROWS frame up to the cut-over: left-to-right loop.
 *   k_wf_scan / k_wf_mid / k_wf_scan (apply) — a segmented inclusive scan
 *                  that restarts at partition (or peer) starts AND every B
 *                  positions; run forward (S) and, on the mirrored index,
 *                  backward (R).
 *   k_wf_final   — the frame from S and R: S[hi] (unbounded start, or a peer
 *                  group), R[lo] (unbounded end), and for a bounded frame of
 *                  width W with B = W: R[lo] (+) S[hi] when lo and hi lie in
 *                  different blocks, S[hi] when lo starts its block or
 *                  partition, else R[lo]. The decomposition keeps position
 *                  order, so the MIN / MAX tie rule survives it.
 * One state type serves every aggregate: c = non-NULL inputs, (lo, hi) = the
 * value (int128 sum, double bits, or the chosen row's bits); c == 0 is the
 * identity and has lo = hi = 0.
 * ====================================================================== */

#define WF_THREADS 256
#define WF_ITEMS 16
#define WF_TILE (WF_THREADS * WF_ITEMS)
#define WF_WAVES (WF_THREADS / WAVE)
#define WF_MID_THREADS 512
#define WF_MID_WAVES (WF_MID_THREADS / WAVE)
/* measured: the loop beats the two scans up to W = 256 on a float sum
 * (profiles/winframe_ops.txt); half of that leaves room for the costlier
 * int128 and MIN / MAX steps */
#define WF_DIRECT_DEFAULT 128

enum { WF_OP_CNT = 0, WF_OP_SUMI, WF_OP_SUMF, WF_OP_MINI, WF_OP_MAXI,
       WF_OP_MINF, WF_OP_MAXF };
enum { WF_MODE_S = 0, WF_MODE_R, WF_MODE_SR };

struct wf_st {
    unsigned long long lo;
    long long hi;
    uint32_t c;
    uint32_t h;   /* scans only: the run holds a segment head */
};
static_assert(sizeof(wf_st) == 24, "wf_st layout");

__device__ __forceinline__ wf_st wf_identity()
{
    wf_st r;
    r.lo = 0;
    r.hi = 0;
    r.c = 0;
    r.h = 0;
    return r;
}

/* float8_cmp_internal: NaN == NaN, NaN above everything, -0.0 == +0.0 */
__device__ __forceinline__ int wf_fcmp(double a, double b)
{
    if (a != a)
        return b != b ? 0 : 1;
    if (b != b)
        return -1;
    return a > b ? 1 : (a < b ? -1 : 0);
}

/* a is the run to the left of b. MIN / MAX keep the left operand only when
 * it is strictly smaller / greater: the later row wins a tie */
template <int OP>
__device__ __forceinline__ wf_st wf_comb(const wf_st &a, const wf_st &b)
{
    wf_st r;
    r.h = 0;
    r.hi = 0;
    r.lo = 0;
    r.c = a.c + b.c;
    if (OP == WF_OP_CNT)
        return r;
    if (OP == WF_OP_SUMI) {
        r.lo = a.lo + b.lo;
        r.hi = a.hi + b.hi + (r.lo < a.lo ? 1 : 0);
        return r;
    }
    unsigned long long x;
    if (OP == WF_OP_SUMF) {
        x = (unsigned long long)__double_as_longlong(
            __longlong_as_double((long long)a.lo) +
            __longlong_as_double((long long)b.lo));
    } else {
        bool keep;
        if (OP == WF_OP_MAXI)
            keep = (long long)a.lo > (long long)b.lo;
        else if (OP == WF_OP_MINI)
            keep = (long long)a.lo < (long long)b.lo;
        else {
            const int c = wf_fcmp(__longlong_as_double((long long)a.lo),
                                  __longlong_as_double((long long)b.lo));
            keep = OP == WF_OP_MAXF ? c > 0 : c < 0;
        }
        x = keep ? a.lo : b.lo;
    }
    r.lo = !a.c ? b.lo : (!b.c ? a.lo : x);
    return r;
}

/* a comes before b in SCAN order; on the mirrored (rev) index that makes b
 * the run to the left in position order */
template <int OP>
__device__ __forceinline__ wf_st wf_seg_comb(const wf_st &a, const wf_st &b,
                                             const int rev)
{
    wf_st r = rev ? wf_comb<OP>(b, a) : wf_comb<OP>(a, b);
    if (b.h) {
        r.lo = b.lo;
        r.hi = b.hi;
        r.c = b.c;
    }
    r.h = a.h | b.h;
    return r;
}

__device__ __forceinline__ wf_st wf_shfl_up(const wf_st &a, int o)
{
    wf_st r;
    r.lo = __shfl_up(a.lo, o);
    r.hi = __shfl_up(a.hi, o);
    r.c = __shfl_up(a.c, o);
    r.h = __shfl_up(a.h, o);
    return r;
}

/* block-wide exclusive wf_seg_comb scan, the shape of win_block_excl_scan */
template <int OP, int NW>
__device__ __forceinline__ wf_st wf_block_excl_scan(const wf_st &v,
                                                    wf_st *wtot, wf_st *total,
                                                    const int rev)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    wf_st incl = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const wf_st t = wf_shfl_up(incl, o);
        if (lane >= o)
            incl = wf_seg_comb<OP>(t, incl, rev);
    }
    if (lane == WAVE - 1)
        wtot[wid] = incl;
    __syncthreads();
    wf_st pre = wf_identity(), tot = wf_identity();
    for (int w = 0; w < NW; w++) {
        const wf_st s = wtot[w];
        if (w < wid)
            pre = wf_seg_comb<OP>(pre, s, rev);
        tot = wf_seg_comb<OP>(tot, s, rev);
    }
    __syncthreads();
    wf_st excl = wf_shfl_up(incl, 1);
    if (lane == 0)
        excl = wf_identity();
    *total = tot;
    return wf_seg_comb<OP>(pre, excl, rev);
}

__device__ __forceinline__ int64_t wf_sat_add(int64_t a, int64_t b)
{
    int64_t r;
    if (__builtin_add_overflow(a, b, &r))
        return b < 0 ? INT64_MIN : INT64_MAX;
    return r;
}

/* a column entry as 64 bits: sign- / zero-extended integer or double bits */
__device__ __forceinline__ unsigned long long wf_load(const void *col,
                                                      uint32_t row, int type)
{
    switch (type) {
    case OTBX_SORT_I64:
    case OTBX_SORT_F64:
        return ((const unsigned long long *)col)[row];
    case OTBX_SORT_I32:
        return (unsigned long long)(long long)((const int32_t *)col)[row];
    default:
        return ((const uint8_t *)col)[row];
    }
}

__device__ __forceinline__ void wf_store_typed(void *out, uint32_t p, int type,
                                               unsigned long long v)
{
    switch (type) {
    case OTBX_SORT_I64:
    case OTBX_SORT_F64:
        ((unsigned long long *)out)[p] = v;
        break;
    case OTBX_SORT_I32:
        ((int32_t *)out)[p] = (int32_t)v;
        break;
    default:
        ((uint8_t *)out)[p] = (uint8_t)v;
        break;
    }
}

/* what every per-position kernel needs to find its partition and frame.
 * f is normalised by the host: under ROWS a CURRENT bound is OFFSET 0 */
struct wf_bnd {
    otbx_frame f;
    const int64_t *rn, *pr, *rk, *cs;
    uint32_t n;
};

__device__ __forceinline__ void wf_frame(const wf_bnd &b, uint32_t p,
                                         int64_t *ps_, int64_t *pe_,
                                         int64_t *lo_, int64_t *hi_)
{
    const int64_t ps = (int64_t)p - (b.rn[p] - 1);
    const int64_t pe = ps + b.pr[p] - 1;
    int64_t lo = ps, hi = pe;
    if (b.f.units == OTBX_FRAME_ROWS) {
        if (b.f.start_kind != OTBX_FB_UNBOUNDED)
            lo = max(ps, wf_sat_add((int64_t)p, b.f.start_off));
        if (b.f.end_kind != OTBX_FB_UNBOUNDED)
            hi = min(pe, wf_sat_add((int64_t)p, b.f.end_off));
    } else {
        if (b.f.start_kind != OTBX_FB_UNBOUNDED)
            lo = ps + b.rk[p] - 1;
        if (b.f.end_kind != OTBX_FB_UNBOUNDED)
            hi = ps + b.cs[p] - 1;
    }
    *ps_ = ps;
    *pe_ = pe;
    *lo_ = lo;
    *hi_ = hi;
}

__device__ __forceinline__ uint32_t wf_clamp(int64_t q, uint32_t n)
{
    return q < 0 ? 0u : (q >= (int64_t)n ? n - 1 : (uint32_t)q);
}

/* ---- NTILE, LAG / LEAD, FIRST / LAST / NTH_VALUE, COUNT_STAR ---- */
struct wf_poscall {
    wf_bnd b;
    const int64_t *perm;
    const void *col;
    const uint8_t *nulls;
    void *out;
    uint8_t *out_null;
    int64_t param, def_i;
    double def_f;
    int32_t def_isnull, func, type;
};

__global__ __launch_bounds__(WF_THREADS) void k_wf_pos(const wf_poscall a)
{
    const uint32_t n = a.b.n;
    const uint32_t p = blockIdx.x * (uint32_t)WF_THREADS + threadIdx.x;
    if (p >= n)
        return;
    int64_t ps, pe, lo, hi;
    wf_frame(a.b, p, &ps, &pe, &lo, &hi);
    if (a.func == OTBX_WF_NTILE) {
        const int64_t T = pe - ps + 1, i = (int64_t)p - ps, nb = a.param;
        const int64_t q = T / nb, r = T % nb;
        int64_t res;
        if (q == 0)
            res = i + 1;
        else if (i < r * (q + 1))
            res = i / (q + 1) + 1;
        else
            res = r + (i - r * (q + 1)) / q + 1;
        ((int32_t *)a.out)[p] = (int32_t)res;
        return;
    }
    if (a.func == OTBX_WF_COUNT_STAR) {
        ((int64_t *)a.out)[p] = lo <= hi ? hi - lo + 1 : 0;
        return;
    }
    int64_t src;
    bool have, usedef = false;
    if (a.func == OTBX_WF_LAG || a.func == OTBX_WF_LEAD) {
        src = (int64_t)p + (a.func == OTBX_WF_LAG ? -a.param : a.param);
        have = src >= ps && src <= pe;
        usedef = !have && !a.def_isnull;
    } else {
        src = a.func == OTBX_WF_FIRST_VALUE
                  ? lo
                  : (a.func == OTBX_WF_LAST_VALUE
                         ? hi
                         : wf_sat_add(lo, a.param - 1));
        have = lo <= hi && src <= hi;
    }
    unsigned long long v = 0;
    uint8_t isnull = 1;
    if (have) {
        const uint32_t row = win_row(a.perm, wf_clamp(src, n), n);
        isnull = a.nulls && a.nulls[row] ? 1 : 0;
        if (!isnull)
            v = wf_load(a.col, row, a.type);
    } else if (usedef) {
        isnull = 0;
        v = a.type == OTBX_SORT_F64
                ? (unsigned long long)__double_as_longlong(a.def_f)
                : (unsigned long long)a.def_i;
    }
    wf_store_typed(a.out, p, a.type, v);
    a.out_null[p] = isnull;
}

/* ---- an aggregate's input in sorted order ---- */
__global__ __launch_bounds__(WF_THREADS) void
k_wf_gather(const int64_t *perm, const void *col, const uint8_t *nulls,
            const int type, const int want_vals, const uint32_t n,
            unsigned long long *sv, uint8_t *nn)
{
    const uint32_t p = blockIdx.x * (uint32_t)WF_THREADS + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t row = win_row(perm, p, n);
    const bool nonnull = !(nulls && nulls[row]);
    nn[p] = nonnull ? 1 : 0;
    if (want_vals)
        sv[p] = nonnull ? wf_load(col, row, type) : 0ull;
}

template <int OP>
__device__ __forceinline__ wf_st wf_elem(const unsigned long long *sv,
                                         const uint8_t *nn, uint32_t p)
{
    wf_st e;
    e.h = 0;
    e.c = nn[p];
    e.lo = (OP != WF_OP_CNT && e.c) ? sv[p] : 0ull;
    e.hi = OP == WF_OP_SUMI ? ((long long)e.lo >> 63) : 0;
    return e;
}

/* ---- the aggregate's result, stored in the aggregate's own type ---- */
struct wf_aggcall {
    wf_bnd b;
    const unsigned long long *sv;
    const uint8_t *nn;
    const unsigned long long *Slo, *Rlo;
    const long long *Shi, *Rhi;
    const uint32_t *Sc, *Rc;
    void *out;
    int64_t *out_hi;
    uint8_t *out_null;
    uint32_t B;
    int32_t mode, type;
};

template <int OP>
__device__ __forceinline__ void wf_store(const wf_aggcall &a, uint32_t p,
                                         const wf_st &s)
{
    if (OP == WF_OP_CNT) {
        ((int64_t *)a.out)[p] = (int64_t)s.c;
        return;
    }
    const bool null = s.c == 0;
    const unsigned long long v = null ? 0ull : s.lo;
    if (OP == WF_OP_MINI || OP == WF_OP_MAXI) {
        wf_store_typed(a.out, p, a.type, v);
    } else {
        ((unsigned long long *)a.out)[p] = v;
        if (OP == WF_OP_SUMI && a.out_hi)
            a.out_hi[p] = null ? 0 : s.hi;
    }
    a.out_null[p] = null ? 1 : 0;
}

/* bounded ROWS frame up to the cut-over: left to right, as the reference */
template <int OP>
__global__ __launch_bounds__(WF_THREADS) void k_wf_direct(const wf_aggcall a)
{
    const uint32_t n = a.b.n;
    const uint32_t p = blockIdx.x * (uint32_t)WF_THREADS + threadIdx.x;
    if (p >= n)
        return;
    int64_t ps, pe, lo, hi;
    wf_frame(a.b, p, &ps, &pe, &lo, &hi);
    wf_st acc = wf_identity();
    if (lo <= hi) {
        const uint32_t l = wf_clamp(lo, n), h = wf_clamp(hi, n);
        for (uint32_t q = l; q <= h; q++)
            acc = wf_comb<OP>(acc, wf_elem<OP>(a.sv, a.nn, q));
    }
    wf_store<OP>(a, p, acc);
}

__device__ __forceinline__ wf_st wf_read(const unsigned long long *lo,
                                         const long long *hi,
                                         const uint32_t *c, uint32_t p)
{
    wf_st s;
    s.h = 0;
    s.lo = lo[p];
    s.hi = hi ? hi[p] : 0;
    s.c = c[p];
    return s;
}

template <int OP>
__global__ __launch_bounds__(WF_THREADS) void k_wf_final(const wf_aggcall a)
{
    const uint32_t n = a.b.n;
    const uint32_t p = blockIdx.x * (uint32_t)WF_THREADS + threadIdx.x;
    if (p >= n)
        return;
    int64_t ps, pe, lo, hi;
    wf_frame(a.b, p, &ps, &pe, &lo, &hi);
    wf_st s = wf_identity();
    if (lo <= hi) {
        const uint32_t l = wf_clamp(lo, n), h = wf_clamp(hi, n);
        if (a.mode == WF_MODE_S) {
            s = wf_read(a.Slo, a.Shi, a.Sc, h);
        } else if (a.mode == WF_MODE_R) {
            s = wf_read(a.Rlo, a.Rhi, a.Rc, l);
        } else if (l / a.B != h / a.B) {
            s = wf_comb<OP>(wf_read(a.Rlo, a.Rhi, a.Rc, l),
                            wf_read(a.Slo, a.Shi, a.Sc, h));
        } else if ((int64_t)l == ps || l % a.B == 0) {
            s = wf_read(a.Slo, a.Shi, a.Sc, h);
        } else {
            s = wf_read(a.Rlo, a.Rhi, a.Rc, l);
        }
    }
    wf_store<OP>(a, p, s);
}

/* ---- segmented inclusive scan over the sorted positions ----
 * A segment starts at every position whose flag byte has hbit (partition or
 * peer start) and at every multiple of B. rev scans the mirrored index
 * q -> n-1-q, where a segment starts at the LAST position of a partition /
 * peer group / block. phase 0 writes the tile's aggregate; phase 1 starts
 * from the tile's carry and writes the running state of every position. */
struct wf_scancall {
    const unsigned long long *sv;
    const uint8_t *nn;
    const uint8_t *flags;
    wf_st *tiles;         /* phase 0 out; phase 1 in: the carries */
    unsigned long long *olo;
    long long *ohi;       /* NULL: not wanted */
    uint32_t *oc;
    uint32_t n, B, hbit;
    int32_t rev, phase;
};

__device__ __forceinline__ bool wf_head(const wf_scancall &a, uint32_t p)
{
    if (!a.rev)
        return (a.flags[p] & a.hbit) || p % a.B == 0;
    return p == a.n - 1 || (a.flags[p + 1] & a.hbit) || p % a.B == a.B - 1;
}

template <int OP>
__global__ __launch_bounds__(WF_THREADS) void k_wf_scan(const wf_scancall a)
{
    __shared__ wf_st wtot[WF_WAVES];
    const uint32_t n = a.n;
    const uint32_t q0 = blockIdx.x * (uint32_t)WF_TILE + threadIdx.x * WF_ITEMS;

    wf_st run = wf_identity();
    for (int i = 0; i < WF_ITEMS; i++) {
        const uint32_t q = q0 + i;
        if (q >= n)
            break;
        const uint32_t p = a.rev ? n - 1 - q : q;
        const wf_st e = wf_elem<OP>(a.sv, a.nn, p);
        if (wf_head(a, p)) {
            run = e;
            run.h = 1;
        } else {
            const uint32_t h = run.h;
            run = a.rev ? wf_comb<OP>(e, run) : wf_comb<OP>(run, e);
            run.h = h;
        }
    }
    wf_st tot;
    const wf_st ex =
        wf_block_excl_scan<OP, WF_WAVES>(run, wtot, &tot, a.rev);
    if (a.phase == 0) {
        if (threadIdx.x == 0)
            a.tiles[blockIdx.x] = tot;
        return;
    }
    run = wf_seg_comb<OP>(a.tiles[blockIdx.x], ex, a.rev);
    for (int i = 0; i < WF_ITEMS; i++) {
        const uint32_t q = q0 + i;
        if (q >= n)
            break;
        const uint32_t p = a.rev ? n - 1 - q : q;
        const wf_st e = wf_elem<OP>(a.sv, a.nn, p);
        run = wf_head(a, p)
                  ? e
                  : (a.rev ? wf_comb<OP>(e, run) : wf_comb<OP>(run, e));
        a.olo[p] = run.lo;
        a.oc[p] = run.c;
        if (a.ohi)
            a.ohi[p] = run.hi;
    }
}

/* exclusive scan of the tile aggregates in place: one workgroup, the running
 * carry in registers between passes */
template <int OP>
__global__ __launch_bounds__(WF_MID_THREADS) void
k_wf_mid(wf_st *tiles, const uint32_t ntiles, const int rev)
{
    __shared__ wf_st wtot[WF_MID_WAVES];
    wf_st run = wf_identity();
    for (uint32_t c0 = 0; c0 < ntiles; c0 += WF_MID_THREADS) {
        const uint32_t idx = c0 + threadIdx.x;
        const wf_st v = idx < ntiles ? tiles[idx] : wf_identity();
        wf_st tot;
        const wf_st ex =
            wf_block_excl_scan<OP, WF_MID_WAVES>(v, wtot, &tot, rev);
        if (idx < ntiles)
            tiles[idx] = wf_seg_comb<OP>(run, ex, rev);
        run = wf_seg_comb<OP>(run, tot, rev);
    }
}

/* ---- host side ---- */

struct wf_layout {
    size_t flags, tiles, carry, rn, pr, rk, cs, sv, nn, slo, shi, sc, rlo, rhi,
        rc, stiles, total;
    uint32_t ntiles;
};

static void wf_plan_layout(int64_t n, wf_layout *L)
{
    L->ntiles = (uint32_t)((n + WIN_TILE - 1) / WIN_TILE);
    const size_t padded = (size_t)L->ntiles * WIN_TILE, un = (size_t)n;
    size_t o = 0;
    L->flags = o;  o += align256_sz(padded);
    L->tiles = o;  o += align256_sz((size_t)L->ntiles * sizeof(win_tile));
    L->carry = o;  o += align256_sz((size_t)L->ntiles * sizeof(win_tile));
    L->rn = o;     o += align256_sz(un * 8);
    L->pr = o;     o += align256_sz(un * 8);
    L->rk = o;     o += align256_sz(un * 8);
    L->cs = o;     o += align256_sz(un * 8);
    L->sv = o;     o += align256_sz(un * 8);
    L->nn = o;     o += align256_sz(un);
    L->slo = o;    o += align256_sz(un * 8);
    L->shi = o;    o += align256_sz(un * 8);
    L->sc = o;     o += align256_sz(un * 4);
    L->rlo = o;    o += align256_sz(un * 8);
    L->rhi = o;    o += align256_sz(un * 8);
    L->rc = o;     o += align256_sz(un * 4);
    L->stiles = o; o += align256_sz((size_t)L->ntiles * sizeof(wf_st));
    L->total = o;
}

static_assert(WF_TILE == WIN_TILE, "one tile count serves both scans");

static bool wf_is_agg(int func)
{
    return func >= OTBX_WF_COUNT && func <= OTBX_WF_MAX;
}

static int wf_op(int func, int type)
{
    const bool f = type == OTBX_SORT_F64;
    switch (func) {
    case OTBX_WF_COUNT: return WF_OP_CNT;
    case OTBX_WF_SUM:   return f ? WF_OP_SUMF : WF_OP_SUMI;
    case OTBX_WF_MIN:   return f ? WF_OP_MINF : WF_OP_MINI;
    default:            return f ? WF_OP_MAXF : WF_OP_MAXI;
    }
}

/* the cut-over in force: OTBX_WIN_FRAME_DIRECT, else the default */
static int64_t wf_direct_limit(void)
{
    const char *e = getenv("OTBX_WIN_FRAME_DIRECT");
    if (e && *e) {
        char *end;
        const long long v = strtoll(e, &end, 10);
        if (*end == '\0' && v >= 0)
            return (int64_t)v;
    }
    return WF_DIRECT_DEFAULT;
}

template <int OP>
static void wf_run_scan(hipStream_t s, const wf_layout &L, char *w,
                        uint32_t n, uint32_t B, uint32_t hbit, int rev,
                        bool want_hi)
{
    wf_scancall c;
    c.sv = (const unsigned long long *)(w + L.sv);
    c.nn = (const uint8_t *)(w + L.nn);
    c.flags = (const uint8_t *)(w + L.flags);
    c.tiles = (wf_st *)(w + L.stiles);
    c.olo = (unsigned long long *)(w + (rev ? L.rlo : L.slo));
    c.ohi = want_hi ? (long long *)(w + (rev ? L.rhi : L.shi)) : nullptr;
    c.oc = (uint32_t *)(w + (rev ? L.rc : L.sc));
    c.n = n;
    c.B = B;
    c.hbit = hbit;
    c.rev = rev;
    c.phase = 0;
    hipLaunchKernelGGL(k_wf_scan<OP>, dim3(L.ntiles), dim3(WF_THREADS), 0, s,
                       c);
    hipLaunchKernelGGL(k_wf_mid<OP>, dim3(1), dim3(WF_MID_THREADS), 0, s,
                       c.tiles, L.ntiles, rev);
    c.phase = 1;
    hipLaunchKernelGGL(k_wf_scan<OP>, dim3(L.ntiles), dim3(WF_THREADS), 0, s,
                       c);
}

template <int OP>
static void wf_run_agg(hipStream_t s, const wf_layout &L, char *w,
                       const wf_bnd &b, const otbx_wincall &c, int64_t direct)
{
    const uint32_t n = b.n;
    const dim3 grid((n + WF_THREADS - 1) / WF_THREADS), block(WF_THREADS);
    wf_aggcall a;
    a.b = b;
    a.sv = (const unsigned long long *)(w + L.sv);
    a.nn = (const uint8_t *)(w + L.nn);
    a.Slo = (const unsigned long long *)(w + L.slo);
    a.Rlo = (const unsigned long long *)(w + L.rlo);
    const bool want_hi = OP == WF_OP_SUMI && c.type == OTBX_SORT_I64;
    a.Shi = want_hi ? (const long long *)(w + L.shi) : nullptr;
    a.Rhi = want_hi ? (const long long *)(w + L.rhi) : nullptr;
    a.Sc = (const uint32_t *)(w + L.sc);
    a.Rc = (const uint32_t *)(w + L.rc);
    a.out = c.out;
    a.out_hi = c.out_hi;
    a.out_null = c.out_null;
    a.type = c.type;
    a.B = n;
    a.mode = WF_MODE_S;

    const otbx_frame &f = b.f;
    const bool rows = f.units == OTBX_FRAME_ROWS;
    const bool sunb = f.start_kind == OTBX_FB_UNBOUNDED;
    const bool eunb = f.end_kind == OTBX_FB_UNBOUNDED;
    const __int128 W = (__int128)f.end_off - (__int128)f.start_off + 1;
    if (rows && !sunb && !eunb && direct > 0 && W <= (__int128)direct) {
        hipLaunchKernelGGL(k_wf_direct<OP>, grid, block, 0, s, a);
        return;
    }
    uint32_t hbit = WIN_FP;
    if (sunb) {
        a.mode = WF_MODE_S;
    } else if (eunb) {
        a.mode = WF_MODE_R;
    } else if (!rows) {
        a.mode = WF_MODE_S;          /* the peer group: restart at peer starts */
        hbit = WIN_FG;
    } else {
        a.mode = WF_MODE_SR;
        a.B = W < 1 ? 1u : (W > (__int128)n ? n : (uint32_t)W);
    }
    if (a.mode != WF_MODE_R)
        wf_run_scan<OP>(s, L, w, n, a.B, hbit, 0, want_hi);
    if (a.mode != WF_MODE_S)
        wf_run_scan<OP>(s, L, w, n, a.B, hbit, 1, want_hi);
    hipLaunchKernelGGL(k_wf_final<OP>, grid, block, 0, s, a);
}

extern "C" {

otbx_status otbx_window_frame_direct_default(int64_t *width)
{
    if (!width)
        return OTBX_ERR_INVALID;
    *width = WF_DIRECT_DEFAULT;
    return OTBX_OK;
}

otbx_status otbx_window_frame_workspace_bytes(int64_t n, int32_t ncalls,
                                              size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX || ncalls < 1 ||
        ncalls > OTBX_MAX_WINCALLS)
        return OTBX_ERR_INVALID;
    /* the calls of one list run one after the other on the stream and share
     * the aggregate scratch, so the size does not grow with ncalls */
    wf_layout L;
    wf_plan_layout(n, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_window_frame(const otbx_sortspec *spec, int32_t npart,
                              const int64_t *perm_dev, int64_t n,
                              const otbx_frame *frame,
                              const otbx_wincall *calls, int32_t ncalls,
                              void *ws_dev, size_t ws_bytes, void *stream)
{
    /* argument checks first: nothing in this block touches HIP */
    if (!spec || !frame || !calls)
        return OTBX_ERR_INVALID;
    if (ncalls < 1 || ncalls > OTBX_MAX_WINCALLS)
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
    if (frame->units != OTBX_FRAME_ROWS && frame->units != OTBX_FRAME_RANGE)
        return OTBX_ERR_INVALID;
    if (frame->start_kind < OTBX_FB_UNBOUNDED ||
        frame->start_kind > OTBX_FB_OFFSET ||
        frame->end_kind < OTBX_FB_UNBOUNDED || frame->end_kind > OTBX_FB_OFFSET)
        return OTBX_ERR_INVALID;
    if (frame->units == OTBX_FRAME_RANGE &&
        (frame->start_kind == OTBX_FB_OFFSET ||
         frame->end_kind == OTBX_FB_OFFSET))
        return OTBX_ERR_INVALID;
    for (int i = 0; i < ncalls; i++) {
        const otbx_wincall *c = &calls[i];
        if (c->func < OTBX_WF_NTILE || c->func > OTBX_WF_MAX)
            return OTBX_ERR_INVALID;
        if (c->type < OTBX_SORT_I64 || c->type > OTBX_SORT_U8)
            return OTBX_ERR_INVALID;
        if (!c->out)
            return OTBX_ERR_INVALID;
        const bool plain = c->func == OTBX_WF_NTILE ||
                           c->func == OTBX_WF_COUNT_STAR ||
                           c->func == OTBX_WF_COUNT;
        if (!plain && n > 0 && !c->col)
            return OTBX_ERR_INVALID;
        if (plain ? c->out_null != nullptr : c->out_null == nullptr)
            return OTBX_ERR_INVALID;
        const bool sum128 = c->func == OTBX_WF_SUM && c->type == OTBX_SORT_I64;
        if (sum128 ? c->out_hi == nullptr : c->out_hi != nullptr)
            return OTBX_ERR_INVALID;
        if (c->func == OTBX_WF_NTILE && c->param <= 0)
            return OTBX_ERR_INVALID;
        if (c->func == OTBX_WF_NTH_VALUE && c->param < 1)
            return OTBX_ERR_INVALID;
        if ((c->func == OTBX_WF_LAG || c->func == OTBX_WF_LEAD) &&
            (c->param < INT32_MIN || c->param > INT32_MAX))
            return OTBX_ERR_INVALID;
    }
    wf_layout L;
    wf_plan_layout(n, &L);
    /* a workspace pointer is required even for n == 0, where it is unused */
    if (ws_bytes < L.total || !ws_dev || ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;
    if (n == 0)
        return OTBX_OK;
    const int64_t direct = wf_direct_limit();

    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws_dev;
    const uint32_t un = (uint32_t)n;
    uint8_t *flags = (uint8_t *)(w + L.flags);
    win_tile *tiles = (win_tile *)(w + L.tiles);
    win_tile *carry = (win_tile *)(w + L.carry);

    wf_bnd b;
    b.f = *frame;
    if (b.f.units == OTBX_FRAME_ROWS) {
        if (b.f.start_kind == OTBX_FB_CURRENT) {
            b.f.start_kind = OTBX_FB_OFFSET;
            b.f.start_off = 0;
        }
        if (b.f.end_kind == OTBX_FB_CURRENT) {
            b.f.end_kind = OTBX_FB_OFFSET;
            b.f.end_off = 0;
        }
    }
    if (b.f.start_kind != OTBX_FB_OFFSET)
        b.f.start_off = 0;
    if (b.f.end_kind != OTBX_FB_OFFSET)
        b.f.end_off = 0;
    const bool range = b.f.units == OTBX_FRAME_RANGE;
    b.rn = (const int64_t *)(w + L.rn);
    b.pr = (const int64_t *)(w + L.pr);
    b.rk = (const int64_t *)(w + L.rk);
    b.cs = (const int64_t *)(w + L.cs);
    b.n = un;

    /* partition and peer bounds: the ranking pass of otbx_window */
    otbx_window_out bo = {};
    bo.row_number = (int64_t *)(w + L.rn);
    bo.part_rows = (int64_t *)(w + L.pr);
    uint32_t mask = WIN_O_ROWNUM | WIN_O_PROWS;
    if (range && b.f.start_kind == OTBX_FB_CURRENT) {
        bo.rank = (int64_t *)(w + L.rk);
        mask |= WIN_O_RANK;
    }
    if (range && b.f.end_kind == OTBX_FB_CURRENT) {
        bo.count_star = (int64_t *)(w + L.cs);
        mask |= WIN_O_CSTAR;
    }
    hipLaunchKernelGGL(k_win_flags, dim3(L.ntiles), dim3(WIN_THREADS), 0, s,
                       *spec, (int)npart, perm_dev, un, (const double *)nullptr,
                       (const uint8_t *)nullptr, 0, flags, (double *)nullptr,
                       tiles);
    hipLaunchKernelGGL(k_win_mid, dim3(1), dim3(WIN_MID_THREADS), 0, s, tiles,
                       carry, L.ntiles, un);
    hipLaunchKernelGGL(k_win_apply, dim3(L.ntiles), dim3(WIN_THREADS), 0, s,
                       flags, (double *)nullptr, carry, un, mask, bo,
                       (uint32_t *)nullptr, (uint32_t *)nullptr);

    const dim3 grid((un + WF_THREADS - 1) / WF_THREADS), block(WF_THREADS);
    for (int i = 0; i < ncalls; i++) {
        const otbx_wincall &c = calls[i];
        if (!wf_is_agg(c.func) || (c.func == OTBX_WF_COUNT && !c.nulls)) {
            wf_poscall a;
            a.b = b;
            a.perm = perm_dev;
            a.col = c.col;
            a.nulls = c.nulls;
            a.out = c.out;
            a.out_null = c.out_null;
            a.param = c.param;
            a.def_i = c.def_i;
            a.def_f = c.def_f;
            a.def_isnull = c.def_isnull;
            /* count(v) without a mask counts the frame's rows */
            a.func = c.func == OTBX_WF_COUNT ? OTBX_WF_COUNT_STAR : c.func;
            a.type = c.type;
            hipLaunchKernelGGL(k_wf_pos, grid, block, 0, s, a);
            continue;
        }
        const int op = wf_op(c.func, c.type);
        hipLaunchKernelGGL(k_wf_gather, grid, block, 0, s, perm_dev, c.col,
                           c.nulls, (int)c.type, op != WF_OP_CNT ? 1 : 0, un,
                           (unsigned long long *)(w + L.sv),
                           (uint8_t *)(w + L.nn));
        switch (op) {
        case WF_OP_CNT:  wf_run_agg<WF_OP_CNT>(s, L, w, b, c, direct); break;
        case WF_OP_SUMI: wf_run_agg<WF_OP_SUMI>(s, L, w, b, c, direct); break;
        case WF_OP_SUMF: wf_run_agg<WF_OP_SUMF>(s, L, w, b, c, direct); break;
        case WF_OP_MINI: wf_run_agg<WF_OP_MINI>(s, L, w, b, c, direct); break;
        case WF_OP_MAXI: wf_run_agg<WF_OP_MAXI>(s, L, w, b, c, direct); break;
        case WF_OP_MINF: wf_run_agg<WF_OP_MINF>(s, L, w, b, c, direct); break;
        default:         wf_run_agg<WF_OP_MAXF>(s, L, w, b, c, direct); break;
        }
    }
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

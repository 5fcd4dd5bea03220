/*
 * otbx_filter.hip — the generic GPU Filter operator (otbx_filter_sel): a
 * WHERE qual in conjunctive normal form over typed, nullable columns → the
 * ascending vector of passing row indices. The ExecScan / ExecQual analog
 * (executor/execScan.c:140-363; EEOP_QUAL execExprInterp.c:919, strict
 * operators :703, Kleene AND / OR :783-904, NullTest :973; float order
 * float8_cmp_internal, utils/adt/float.c:1172). Contract in include/otbx.h,
 * DESIGN.md §8i.
 *
 * A row passes iff every clause has at least one TRUE term (see the header
 * for why the three-valued logic collapses to that), so one "true" bit per
 * row and clause is all the state there is. Everything is stream-ordered,
 * three kernels, and kernel boundaries are the only ordering between
 * workgroups:
 *   k_flt_eval   — one FLT_TILE-row tile per workgroup, FLT_ITEMS consecutive
 *                  rows per thread. Loops over the terms in order; per term
 *                  the thread's rows are loaded (16-byte vectors where the
 *                  column is 16-byte aligned and the tile is whole, checked
 *                  scalar loads otherwise) and reduced to two 16-bit masks,
 *                  "less" and "equal"; the operator is applied to the masks,
 *                  not per row. A term no row of the wave still needs is
 *                  skipped before its loads (wave-uniform branch): rows that
 *                  failed an earlier clause, or already passed this one.
 *                  Writes one count per tile and, unless the call is
 *                  count-only, 1 bit per row.
 *   k_flt_scan   — one workgroup: exclusive scan of the tile counts in place,
 *                  FLT_SCAN_CHUNK tiles per pass with a register carry;
 *                  writes *nsel. The last kernel of a count-only call.
 *   k_flt_write  — one wave per tile: the tile's 4096 rows are 64 64-bit mask
 *                  words; each word is the ballot of 64 consecutive rows, so
 *                  the popcount below a lane's bit is its rank and the stores
 *                  of a wave are contiguous. The columns are not read again.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm_f64: float8_cmp_internal as an order */

#define FLT_THREADS 256
#define FLT_WAVES (FLT_THREADS / WAVE)
#define FLT_ITEMS 16
#define FLT_TILE (FLT_THREADS * FLT_ITEMS)   /* 4096 rows per tile */
#define FLT_TILE_WORDS (FLT_TILE / 64)       /* 64-bit mask words per tile */
#define FLT_SCAN_THREADS 1024
#define FLT_SCAN_ITEMS 4
#define FLT_SCAN_CHUNK (FLT_SCAN_THREADS * FLT_SCAN_ITEMS)   /* tiles per pass */
#define FLT_ALL 0xffffu                      /* all FLT_ITEMS rows of a thread */

static_assert(FLT_ITEMS == 16, "one uint16 of mask per thread");
static_assert(FLT_TILE_WORDS == WAVE, "k_flt_write: one mask word per lane");
static_assert(sizeof(otbx_qualterm) == 64, "otbx_qualterm layout");
static_assert(sizeof(otbx_qual) == 1032, "otbx_qual layout");

/* the thread's FLT_ITEMS rows of one column. fast: the column is 16-byte
 * aligned and the tile lies wholly inside it; otherwise every row is
 * bounds-checked and loaded on its own (rows past n read as 0 and are
 * masked by the caller) */
template <typename T>
__device__ __forceinline__ void flt_load(const void *col, uint32_t p0,
                                         uint32_t n, bool fast,
                                         T (&v)[FLT_ITEMS])
{
    const T *c = (const T *)col + p0;
    if (fast) {
        constexpr int PER = 16 / (int)sizeof(T);
        const uint4 *c4 = (const uint4 *)c;
#pragma unroll
        for (int k = 0; k < FLT_ITEMS / PER; k++) {
            const uint4 w = c4[k];
            __builtin_memcpy(&v[k * PER], &w, 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < FLT_ITEMS; i++)
            v[i] = p0 + i < n ? c[i] : (T)0;
    }
}

__device__ __forceinline__ bool flt_fast(const void *p, bool whole)
{
    return whole && ((uintptr_t)p & 15u) == 0;
}

/* bit i set iff row p0 + i is NULL; no mask = no NULLs */
__device__ __forceinline__ uint32_t flt_nullbits(const uint8_t *nulls,
                                                 uint32_t p0, uint32_t n,
                                                 bool whole)
{
    if (!nulls)
        return 0u;
    uint8_t b[FLT_ITEMS];
    flt_load<uint8_t>(nulls, p0, n, flt_fast(nulls, whole), b);
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < FLT_ITEMS; i++)
        m |= (b[i] ? 1u : 0u) << i;
    return m;
}

/* the comparison key of a value: integers widen to int64, doubles map to
 * the unsigned order of float8_cmp_internal */
__device__ __forceinline__ int64_t flt_key(int64_t v) { return v; }
__device__ __forceinline__ int64_t flt_key(int32_t v) { return v; }
__device__ __forceinline__ int64_t flt_key(uint8_t v) { return v; }
__device__ __forceinline__ unsigned long long flt_key(double v)
{
    return ss_norm_f64(v);
}

/* "less" and "equal" masks of the thread's rows: col against rcol when the
 * term has one, against the constant key c otherwise */
template <typename T, typename K>
__device__ __forceinline__ void flt_cmp(const otbx_qualterm &tm, K c,
                                        uint32_t p0, uint32_t n, bool whole,
                                        uint32_t *lt, uint32_t *eq)
{
    T a[FLT_ITEMS];
    flt_load<T>(tm.col, p0, n, flt_fast(tm.col, whole), a);
    uint32_t l = 0, e = 0;
    if (tm.rcol) {
        T b[FLT_ITEMS];
        flt_load<T>(tm.rcol, p0, n, flt_fast(tm.rcol, whole), b);
#pragma unroll
        for (int i = 0; i < FLT_ITEMS; i++) {
            const K ka = flt_key(a[i]), kb = flt_key(b[i]);
            l |= (ka < kb ? 1u : 0u) << i;
            e |= (ka == kb ? 1u : 0u) << i;
        }
    } else {
#pragma unroll
        for (int i = 0; i < FLT_ITEMS; i++) {
            const K ka = flt_key(a[i]);
            l |= (ka < c ? 1u : 0u) << i;
            e |= (ka == c ? 1u : 0u) << i;
        }
    }
    *lt = l;
    *eq = e;
}

/* ---- qual → 1 bit per row + one count per tile ----
 * thread t holds rows tile0 + t*FLT_ITEMS .. +FLT_ITEMS-1; its uint16 of
 * result bits is word t of the tile, so the mask is a plain little-endian
 * bitmask: row p is bit p % 64 of 64-bit word p / 64 */
__global__ __launch_bounds__(FLT_THREADS) void
k_flt_eval(const otbx_qual q, const uint32_t n, uint16_t *__restrict__ bits,
           uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wcnt[FLT_WAVES];

    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile0 = blockIdx.x * (uint32_t)FLT_TILE;
    const uint32_t p0 = tile0 + threadIdx.x * FLT_ITEMS;
    const bool whole = n - tile0 >= (uint32_t)FLT_TILE;   /* tile0 < n */

    /* alive: rows that passed every finished clause; ctrue: rows with a TRUE
     * term in the current clause */
    uint32_t alive = p0 >= n ? 0u
                     : (n - p0 >= FLT_ITEMS ? FLT_ALL
                                            : (1u << (n - p0)) - 1u);
    uint32_t ctrue = 0;
    for (int t = 0; t < q.nterms; t++) {
        const otbx_qualterm &tm = q.term[t];
        if (t > 0 && tm.clause != q.term[t - 1].clause) {
            alive &= ctrue;
            ctrue = 0;
        }
        /* nothing in this wave still depends on the term: skip its loads */
        if (__ballot((alive & ~ctrue) != 0u) == 0ull)
            continue;
        uint32_t nb = flt_nullbits(tm.nulls, p0, n, whole);
        uint32_t tb;
        if (tm.op >= OTBX_CMP_ISNULL) {
            tb = tm.op == OTBX_CMP_ISNULL ? nb : ~nb;
        } else {
            if (tm.rcol)
                nb |= flt_nullbits(tm.rnulls, p0, n, whole);
            uint32_t lt, eq;
            switch (tm.type) {
            case OTBX_SORT_I64:
                flt_cmp<int64_t, int64_t>(tm, tm.ci, p0, n, whole, &lt, &eq);
                break;
            case OTBX_SORT_F64:
                flt_cmp<double, unsigned long long>(tm, ss_norm_f64(tm.cf),
                                                    p0, n, whole, &lt, &eq);
                break;
            case OTBX_SORT_I32:
                flt_cmp<int32_t, int64_t>(tm, tm.ci, p0, n, whole, &lt, &eq);
                break;
            default:
                flt_cmp<uint8_t, int64_t>(tm, tm.ci, p0, n, whole, &lt, &eq);
                break;
            }
            switch (tm.op) {
            case OTBX_CMP_EQ: tb = eq; break;
            case OTBX_CMP_NE: tb = ~eq; break;
            case OTBX_CMP_LT: tb = lt; break;
            case OTBX_CMP_LE: tb = lt | eq; break;
            case OTBX_CMP_GT: tb = ~(lt | eq); break;
            default:          tb = ~lt; break;
            }
            tb &= ~nb;   /* a NULL operand: the term is not TRUE */
        }
        ctrue |= tb & FLT_ALL;
    }
    if (q.nterms > 0)
        alive &= ctrue;

    if (bits)   /* NULL: count only */
        bits[(size_t)blockIdx.x * FLT_THREADS + threadIdx.x] = (uint16_t)alive;

    uint32_t c = (uint32_t)__popc(alive);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1)
        c += __shfl_xor(c, o);
    if (lane == 0)
        wcnt[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < FLT_WAVES; w++)
            s += wcnt[w];
        counts[blockIdx.x] = s;
    }
}

/* ---- exclusive scan of the tile counts, in place: one workgroup,
 * FLT_SCAN_CHUNK tiles per pass (FLT_SCAN_ITEMS consecutive counts per
 * thread, one 16-byte load), the running total in a register; the next
 * pass's counts are loaded before this pass's scan. The counts array is
 * padded to whole 16-byte groups; what lies past ntiles is masked here ---- */
__device__ __forceinline__ uint4 flt_scan_load(const uint32_t *counts,
                                               uint32_t i0, uint32_t ntiles)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i0 < ntiles) {
        v = *(const uint4 *)(counts + i0);
        v.y = i0 + 1 < ntiles ? v.y : 0u;
        v.z = i0 + 2 < ntiles ? v.z : 0u;
        v.w = i0 + 3 < ntiles ? v.w : 0u;
    }
    return v;
}

__global__ __launch_bounds__(FLT_SCAN_THREADS) void
k_flt_scan(uint32_t *counts, const uint32_t ntiles, int64_t *nsel)
{
    __shared__ uint32_t wsum[FLT_SCAN_THREADS / WAVE];
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);

    uint32_t run = 0;
    uint4 nxt = flt_scan_load(counts, threadIdx.x * FLT_SCAN_ITEMS, ntiles);
    for (uint32_t c0 = 0; c0 < ntiles; c0 += FLT_SCAN_CHUNK) {
        const uint32_t i0 = c0 + threadIdx.x * FLT_SCAN_ITEMS;
        const uint4 v = nxt;
        /* ntiles <= 2^19, so i0 + FLT_SCAN_CHUNK cannot wrap */
        nxt = flt_scan_load(counts, i0 + FLT_SCAN_CHUNK, ntiles);
        const uint32_t mine = v.x + v.y + v.z + v.w;
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t x = __shfl_up(incl, o);
            if (lane >= o)
                incl += x;
        }
        if (lane == WAVE - 1)
            wsum[wid] = incl;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < FLT_SCAN_THREADS / WAVE; w++) {
            const uint32_t s = wsum[w];
            pre += w < wid ? s : 0u;
            tot += s;
        }
        __syncthreads();
        if (i0 < ntiles) {
            const uint32_t e = run + pre + incl - mine;
            *(uint4 *)(counts + i0) =
                make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
        }
        run += tot;
    }
    if (threadIdx.x == 0)
        *nsel = (int64_t)run;
}

/* ---- bitmask + tile offset → row ids ----
 * one wave per tile, FLT_WAVES tiles per workgroup, nothing shared between
 * the waves. Lane j loads mask word j of the tile; word i is the ballot of
 * rows i*64 .. i*64+63, read back wave-uniformly, so the popcount below a
 * lane's bit is its rank and the running base stays in a scalar. */
__global__ __launch_bounds__(FLT_THREADS) void
k_flt_write(const unsigned long long *__restrict__ bits,
            const uint32_t *__restrict__ offs, const uint32_t ntiles,
            const uint32_t n, int64_t *__restrict__ sel)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    const uint32_t tile = blockIdx.x * (uint32_t)FLT_WAVES + wid;
    if (tile >= ntiles)
        return;
    const uint32_t tile0 = tile * (uint32_t)FLT_TILE;
    const unsigned long long word = bits[(size_t)tile * FLT_TILE_WORDS + lane];
    uint32_t base = offs[tile];
    if (__ballot(word != 0ull) == 0ull)
        return;
    const int wlo = (int)(uint32_t)word, whi = (int)(uint32_t)(word >> 32);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < FLT_TILE_WORDS; i++) {
        const unsigned long long m =
            (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(wlo, i) |
            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(whi, i)
             << 32);
        if (m == 0ull)
            continue;   /* wave-uniform */
        if ((m >> lane) & 1ull) {
            const uint32_t pos = base + (uint32_t)__popcll(m & below);
            /* pos < n holds for a mask k_flt_eval wrote; the test keeps a
             * stale workspace from ever addressing outside sel */
            if (pos < n)
                sel[pos] = (int64_t)(tile0 + i * 64 + lane);
        }
        base += (uint32_t)__popcll(m);
    }
}

/* ---- host side ---- */

struct flt_layout {
    size_t bits, counts, total;
    uint32_t ntiles;
};

static void flt_plan_layout(int64_t n, flt_layout *L)
{
    L->ntiles = (uint32_t)((n + FLT_TILE - 1) / FLT_TILE);
    size_t o = 0;
    L->bits = o;   o += align256_sz((size_t)L->ntiles * (FLT_TILE / 8));
    L->counts = o; o += align256_sz((size_t)L->ntiles * sizeof(uint32_t));
    L->total = o;
}

extern "C" {

otbx_status otbx_filter_workspace_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    flt_layout L;
    flt_plan_layout(n, &L);
    *bytes = L.total;
    return OTBX_OK;
}

otbx_status otbx_filter_sel(const otbx_qual *q, int64_t n, void *ws_dev,
                            size_t ws_bytes, int64_t *sel_dev,
                            int64_t *nsel_dev, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!q || !nsel_dev)
        return OTBX_ERR_INVALID;
    if (q->nterms < 0 || q->nterms > OTBX_MAX_QUAL_TERMS)
        return OTBX_ERR_INVALID;
    if (n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    for (int t = 0; t < q->nterms; t++) {
        const otbx_qualterm *tm = &q->term[t];
        if (tm->type < OTBX_SORT_I64 || tm->type > OTBX_SORT_U8)
            return OTBX_ERR_INVALID;
        if (tm->op < OTBX_CMP_EQ || tm->op > OTBX_CMP_NOTNULL)
            return OTBX_ERR_INVALID;
        if (tm->rcol && tm->op >= OTBX_CMP_ISNULL)
            return OTBX_ERR_INVALID;
        if (tm->rnulls && !tm->rcol)
            return OTBX_ERR_INVALID;
        if (t > 0 && tm->clause < q->term[t - 1].clause)
            return OTBX_ERR_INVALID;
        if (n > 0 && !tm->col)
            return OTBX_ERR_INVALID;
    }
    flt_layout L;
    flt_plan_layout(n, &L);
    if (ws_bytes < L.total || (L.total > 0 && !ws_dev) ||
        ((uintptr_t)ws_dev & 15u))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)ws_dev;
    uint32_t *counts = (uint32_t *)(w + L.counts);
    const uint32_t un = (uint32_t)n;

    if (L.ntiles > 0)
        hipLaunchKernelGGL(k_flt_eval, dim3(L.ntiles), dim3(FLT_THREADS), 0, s,
                           *q, un,
                           sel_dev ? (uint16_t *)(w + L.bits) : (uint16_t *)0,
                           counts);
    /* with no tiles this only writes *nsel_dev = 0 */
    hipLaunchKernelGGL(k_flt_scan, dim3(1), dim3(FLT_SCAN_THREADS), 0, s,
                       counts, L.ntiles, nsel_dev);
    if (sel_dev && L.ntiles > 0)
        hipLaunchKernelGGL(k_flt_write,
                           dim3((L.ntiles + FLT_WAVES - 1) / FLT_WAVES),
                           dim3(FLT_THREADS), 0, s,
                           (const unsigned long long *)(w + L.bits), counts,
                           L.ntiles, un, sel_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

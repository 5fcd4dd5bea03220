/*
 * otbx.hip — MI355X (gfx950/CDNA4) kernels + C-ABI runtime for the
 * OpenTenBase executor offload. See include/otbx.h for the boundary contract
 * and DESIGN.md for the kernel/roofline map.
 *
 * Everything here is HBM-bound streaming/random work (no dense contraction →
 * no MFMA): coalesced vectorized columnar loads, per-lane register
 * accumulators, wave64 shuffle reductions, device-scope atomics for the
 * shared open-addressing hash tables (cross-XCD correctness: all shared
 * mutable hash-table words are accessed ONLY through atomics — per-XCD L2s
 * are not coherent for plain loads within a launch; payloads written plainly
 * are read only by later kernels, where the launch boundary orders them).
 *
 * Reference semantics being reproduced (citations, /root/reference):
 *   scan+qual       execScan.c:140, execExprInterp.c:324
 *   hash join       nodeHash.c:1828/2026/2141/2174, nodeHashjoin.c:186
 *   hash aggregate  execGrouping.c:295, simplehash.h (open addressing),
 *                   nodeAgg.c:856/2609
 *   transition fns  int8inc int8.c:714, float8pl float.c:970,
 *                   float8_accum float.c:2823 ([N,Sx] in every aggregate;
 *                   the full [N,Sx,Sxx] state in otbx_agg_i64_var, by a
 *                   corrected two-pass sum of squared deviations — the
 *                   additive sum(x^2) form cancels)
 *   NULL semantics  strict transfns skip NULL (nodeAgg.c:743), NULL group
 *                   keys equal (execGrouping.c:520), NULL join keys never
 *                   match (nodeHash.c:2026)
 */
#include <stdlib.h>  /* getenv, atoll */
#include <string.h>

#include "otbx_common.h"
#include "otbx_sortkey.h"            /* ss_norm_f64: revenue ranking */
#include "../../oracle/otbx_gen.h"   /* shared deterministic datagen */

#define OTBX_VERSION_STR "otbx 0.1 gfx950"

/* Lazily-cached per-process scratch (function-local statics here and in
 * otbx_q1.hip): every allocation registers its slot here so otbx_finish can
 * release it and null the static — re-initializing on a different device
 * must not see stale allocations. The C-ABI is single-threaded per process
 * (each reference backend is a single-threaded process; contract in
 * otbx.h), so no locking. Declared in otbx_common.h. */
#define OTBX_SCRATCH_MAX 64
static void **g_scr_slot[OTBX_SCRATCH_MAX];
static unsigned char g_scr_host[OTBX_SCRATCH_MAX];
static int g_nscr = 0;

hipError_t otbx_scr_alloc(void **slot, size_t bytes, int host)
{
    hipError_t e = host ? hipHostMalloc(slot, bytes) : hipMalloc(slot, bytes);
    if (e != hipSuccess)
        return e;
    if (g_nscr == OTBX_SCRATCH_MAX) {
        /* an unregistered pointer would outlive otbx_finish and be reused on
         * another device: refuse it instead */
        if (host)
            (void)hipHostFree(*slot);
        else
            (void)hipFree(*slot);
        *slot = nullptr;
        return hipErrorOutOfMemory;
    }
    g_scr_slot[g_nscr] = slot;
    g_scr_host[g_nscr] = (unsigned char)host;
    g_nscr++;
    return hipSuccess;
}

extern "C" {

const char *otbx_version(void) { return OTBX_VERSION_STR; }

const char *otbx_status_str(otbx_status s)
{
    switch (s) {
    case OTBX_OK: return "ok";
    case OTBX_ERR_HIP: return "hip runtime error";
    case OTBX_ERR_OOM: return "out of memory";
    case OTBX_ERR_INVALID: return "invalid argument";
    case OTBX_ERR_OVERFLOW: return "value out of range";
    case OTBX_ERR_NO_GPU: return "no gpu";
    }
    return "unknown";
}

otbx_status otbx_init(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return OTBX_ERR_NO_GPU;
    HIP_CHECK(hipSetDevice(device));
    return OTBX_OK;
}

otbx_status otbx_finish(void)
{
    HIP_CHECK(hipDeviceSynchronize());
    /* release the registered lazy scratch and null the owning statics so a
     * later otbx_init on another device starts clean */
    for (int i = 0; i < g_nscr; i++) {
        if (*g_scr_slot[i]) {
            if (g_scr_host[i])
                HIP_CHECK(hipHostFree(*g_scr_slot[i]));
            else
                HIP_CHECK(hipFree(*g_scr_slot[i]));
            *g_scr_slot[i] = nullptr;
        }
    }
    g_nscr = 0;
    return OTBX_OK;
}

otbx_status otbx_device_malloc(void **ptr, size_t bytes)
{
    hipError_t e = hipMalloc(ptr, bytes);
    if (e == hipErrorOutOfMemory) return OTBX_ERR_OOM;
    if (e != hipSuccess) return OTBX_ERR_HIP;
    return OTBX_OK;
}

otbx_status otbx_device_free(void *ptr)
{
    HIP_CHECK(hipFree(ptr));
    return OTBX_OK;
}

otbx_status otbx_memcpy_h2d(void *dst, const void *src, size_t n, void *stream)
{
    HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (hipStream_t)stream));
    return OTBX_OK;
}

otbx_status otbx_memcpy_d2h(void *dst, const void *src, size_t n, void *stream)
{
    HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return OTBX_OK;
}

otbx_status otbx_stream_sync(void *stream)
{
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return OTBX_OK;
}

} /* extern "C" (reopened below for the API functions) */

/* ================= generation kernels ================= */

__global__ void k_gen_lineitem(otbx_lineitem_dev t, uint64_t seed,
                               uint32_t rank, uint32_t nranks,
                               int64_t n_global)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < t.n;
         l += stride) {
        uint64_t i = otbx_li_global_row((uint64_t)l, rank, nranks);
        if (t.l_orderkey) t.l_orderkey[l] = otbx_li_orderkey(i);
        t.l_quantity[l] = otbx_li_quantity(seed, i);
        t.l_extendedprice[l] = otbx_li_extendedprice(seed, i);
        t.l_discount[l] = otbx_li_discount(seed, i);
        t.l_tax[l] = otbx_li_tax(seed, i);
        t.l_returnflag[l] = otbx_li_returnflag(seed, i);
        t.l_linestatus[l] = otbx_li_linestatus(seed, i);
        t.l_shipdate[l] = otbx_li_shipdate(seed, i);
        if (t.l_partkey)
            t.l_partkey[l] = otbx_li_partkey(
                seed, i, n_global / 30 > 0 ? n_global / 30 : 1);
    }
}

__global__ void k_gen_orders(otbx_orders_dev t, uint64_t seed, int64_t ncust,
                             uint32_t rank, uint32_t nranks, int skew)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < t.n;
         l += stride) {
        uint64_t i = otbx_ord_global_row((uint64_t)l, rank, nranks);
        t.o_orderkey[l] = otbx_ord_orderkey(i);
        t.o_custkey[l] = skew ? otbx_ord_custkey_skewed(seed, i, ncust)
                              : otbx_ord_custkey(seed, i, ncust);
        t.o_orderdate[l] = otbx_ord_orderdate(seed, i);
        t.o_shippriority[l] = otbx_ord_shippriority(i);
    }
}

__global__ void k_gen_part(otbx_part_dev t, uint64_t seed)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < t.n;
         l += stride) {
        t.p_partkey[l] = otbx_part_partkey((uint64_t)l);
        t.p_type[l] = otbx_part_type(seed, (uint64_t)l);
    }
}

__global__ void k_gen_customer(otbx_customer_dev t, uint64_t seed,
                               uint32_t rank, uint32_t nranks)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < t.n;
         l += stride) {
        uint64_t i = otbx_cust_global_row((uint64_t)l, rank, nranks);
        t.c_custkey[l] = otbx_cust_custkey(i);
        t.c_mktsegment[l] = otbx_cust_mktsegment(seed, i);
    }
}

extern "C" {

otbx_status otbx_gen_lineitem_dev(const otbx_lineitem_dev *t, uint64_t seed,
                                  int64_t n_global, uint32_t rank,
                                  uint32_t nranks, void *stream)
{
    if (!t || nranks == 0 || n_global % nranks || t->n != n_global / nranks)
        return OTBX_ERR_INVALID;
    hipLaunchKernelGGL(k_gen_lineitem, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, *t, seed, rank, nranks, n_global);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gen_orders_dev(otbx_orders_dev *t, uint64_t seed,
                                int64_t n_global, int64_t ncust_global,
                                uint32_t rank, uint32_t nranks, int skew,
                                void *stream)
{
    if (!t || nranks == 0 || n_global % nranks || t->n != n_global / nranks)
        return OTBX_ERR_INVALID;
    hipLaunchKernelGGL(k_gen_orders, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, *t, seed, ncust_global, rank, nranks,
                       skew);
    /* staged-table zone-map metadata: o_orderkey = global_row + 1 with
     * global_row = l·nranks + res (otbx_gen.h otbx_ord_global_row) */
    if (t->n > 0) {
        int64_t res = ((int64_t)rank + nranks - 1) % nranks;
        t->okey_min = res + 1;
        t->okey_max = (t->n - 1) * (int64_t)nranks + res + 1;
        t->has_minmax = 1;
    }
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gen_customer_dev(const otbx_customer_dev *t, uint64_t seed,
                                  int64_t n_global, uint32_t rank,
                                  uint32_t nranks, void *stream)
{
    if (!t || nranks == 0 || n_global % nranks || t->n != n_global / nranks)
        return OTBX_ERR_INVALID;
    hipLaunchKernelGGL(k_gen_customer, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, *t, seed, rank, nranks);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gen_part_dev(const otbx_part_dev *t, uint64_t seed,
                              int64_t n_global, void *stream)
{
    if (!t || t->n != n_global) return OTBX_ERR_INVALID;
    hipLaunchKernelGGL(k_gen_part, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, *t, seed);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ================= config 2: scan + filter + COUNT(*) ================= */

/* 4 B/row algorithmic. int4 vector loads (4 rows/lane/iter), wave ballot +
 * popcount, one atomic per block. */
__global__ void k_scan_count(const int32_t *__restrict__ sd, int64_t n,
                             int32_t cutoff, int64_t *out)
{
    int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t nvec = n / 4;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t c = 0;
    const int4 *sd4 = (const int4 *)sd;
    for (int64_t i = tid; i < nvec; i += stride) {
        int4 v = sd4[i];
        c += (v.x <= cutoff) + (v.y <= cutoff) + (v.z <= cutoff) + (v.w <= cutoff);
    }
    /* tail rows */
    for (int64_t i = nvec * 4 + tid; i < n; i += stride)
        c += (sd[i] <= cutoff);
    /* wave reduction */
    for (int off = WAVE / 2; off > 0; off >>= 1)
        c += __shfl_down((long long)c, off, WAVE);
    __shared__ int64_t ws_[256 / WAVE];
    int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) ws_[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int w = 0; w < (int)(blockDim.x / WAVE); w++) s += ws_[w];
        atomicAdd((unsigned long long *)out, (unsigned long long)s);
    }
}

extern "C" otbx_status otbx_scan_count(const int32_t *sd, int64_t n,
                                       int32_t cutoff, int64_t *count_dev,
                                       void *stream)
{
    HIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(int64_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_scan_count, dim3(grid_for(n / 4, 256)), dim3(256), 0,
                       (hipStream_t)stream, sd, n, cutoff, count_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

/* ================= open-addressing hash-table helpers =================
 *
 * GPU analog of the reference's two tables:
 *  - join build: chained buckets (nodeHash.c:1828) → here an OA table where
 *    duplicate keys occupy their own slots; probe walks from h(key) to the
 *    first never-claimed slot (same result set, SURVEY §7 item 5: parity is
 *    on results, hashing may differ).
 *  - agg groups: simplehash OA linear probing (simplehash.h) → directly an
 *    OA table; slot claim by atomicCAS on the key word (device-scope →
 *    coherent across XCDs; plain loads are NOT used on mutable words inside
 *    a launch).
 * Hash = splitmix64 finalizer (same as the oracle). */

__device__ __forceinline__ uint64_t d_hash_i64(int64_t k)
{
    return otbx_splitmix64((uint64_t)k);
}

/* wave-aggregated append: one atomicAdd per wave instead of per lane
 * (Guideline 12). Returns this lane's output slot, or -1 if !pred.
 * blockDim must be a multiple of 64. */
__device__ __forceinline__ int64_t wave_append(int64_t *counter, bool pred)
{
    unsigned long long mask = __ballot(pred);
    if (!mask) return -1;
    int lane = (int)(threadIdx.x % WAVE);
    int leader = __ffsll((long long)mask) - 1;
    int rank = __popcll(mask & ((1ull << lane) - 1ull));
    long long base = 0;
    if (lane == leader)
        base = (long long)atomicAdd((unsigned long long *)counter,
                                    (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, WAVE);
    return pred ? base + rank : -1;
}

/* max - min + 1 without signed overflow: key columns may span more than
 * 2^63 (a negative key next to INT64_MAX - 1). A span that does not fit
 * comes back as INT64_MAX, which no direct-table cap admits. */
static int64_t key_range(int64_t mn, int64_t mx)
{
    if (mx < mn) return 0;
    uint64_t span = (uint64_t)mx - (uint64_t)mn;
    return span >= (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)span + 1;
}

static inline int64_t next_pow2_host(int64_t v)
{
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

/* ================= generic hash aggregate (otbx_agg_i64) ================= */

/* slot: {key, count_star, count_v, sum}; key EMPTY sentinel = INT64_MIN
 * (documented reserved value — include/otbx.h). NULL-key group is a
 * dedicated accumulator block appended after the table. */
struct agg_slot {
    long long key;
    unsigned long long count_star;
    unsigned long long count_v;
    double sum_v;
};
#define AGG_EMPTY LLONG_MIN

__global__ void k_agg_init(agg_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride) {
        tab[i].key = AGG_EMPTY;
        tab[i].count_star = 0;
        tab[i].count_v = 0;
        tab[i].sum_v = 0.0;
    }
}

/* two-level hash aggregate (SURVEY §7 hard-part 2): a per-block LDS table
 * absorbs hot keys (a 4-group input otherwise serializes every lane on four
 * global atomics — measured 0.08 Grows/s), spilling to the global table when
 * the LDS probe window is exhausted; block-end flush merges LDS partials
 * into the global table. */
#define AGG_LDS_SLOTS 512
#define AGG_LDS_PROBES 4

struct agg_lds_slot {
    long long key;
    unsigned int cs, cv;
    double sum;
};

#define AGG_GLOBAL_PROBE_BOUND 256

/* merge (cs, cv, sum) into key k's global slot (simplehash linear probe).
 * BOUNDED is the small-table first attempt: it gives up after
 * AGG_GLOBAL_PROBE_BOUND steps (table effectively full → the sample-based
 * sizing was wrong) and returns false instead of spinning. */
template <bool BOUNDED = false>
__device__ __forceinline__ bool
d_agg_global_update(agg_slot *tab, int64_t mask, int64_t k,
                    unsigned long long cs, unsigned long long cv, double sum)
{
    int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
    /* t counts only in the bounded form (t += 0 otherwise: no overflow) */
    for (int t = 0; !BOUNDED || t < AGG_GLOBAL_PROBE_BOUND; t += BOUNDED) {
        long long old = atomicCAS((unsigned long long *)&tab[s].key,
                                  (unsigned long long)AGG_EMPTY,
                                  (unsigned long long)k);
        if (old == AGG_EMPTY || old == k) {
            atomicAdd(&tab[s].count_star, cs);
            if (cv) {
                atomicAdd(&tab[s].count_v, cv);
                atomicAdd(&tab[s].sum_v, sum);
            }
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

/* BOUNDED = the estimator-sized build attempt: bounded global probes + an
 * abort flag. When that table overflows (rare-key tail the sample missed),
 * the whole call is redone against the full-size table (BOUNDED = false,
 * abort unused). */
template <bool BOUNDED>
__global__ void k_agg_build(const int64_t *__restrict__ keys,
                            const uint8_t *__restrict__ knull,
                            const double *__restrict__ vals,
                            const uint8_t *__restrict__ vnull, int64_t n,
                            agg_slot *tab, int64_t cap, agg_slot *nullgrp,
                            unsigned int *abort)
{
    __shared__ agg_lds_slot ltab[AGG_LDS_SLOTS];
    for (int s = threadIdx.x; s < AGG_LDS_SLOTS; s += blockDim.x) {
        ltab[s].key = AGG_EMPTY;
        ltab[s].cs = 0;
        ltab[s].cv = 0;
        ltab[s].sum = 0.0;
    }
    __syncthreads();
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool dead = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n && !dead; i += stride) {
        bool kn = knull && knull[i];
        bool vn = vnull && vnull[i];
        double v = vn ? 0.0 : vals[i];
        if (kn || keys[i] == AGG_EMPTY) {
            /* NULL keys form one group (execGrouping.c:520); the sentinel
             * VALUE gets its own accumulator so any i64 key is supported */
            agg_slot *e = kn ? nullgrp : nullgrp + 1;
            atomicAdd(&e->count_star, 1ull);
            if (!vn) {
                atomicAdd(&e->count_v, 1ull);
                atomicAdd(&e->sum_v, v);
            }
            continue;
        }
        int64_t k = keys[i];
        int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)(AGG_LDS_SLOTS - 1));
        bool placed = false;
        for (int t = 0; t < AGG_LDS_PROBES; t++) {
            long long old = atomicCAS((unsigned long long *)&ltab[s].key,
                                      (unsigned long long)AGG_EMPTY,
                                      (unsigned long long)k);
            if (old == AGG_EMPTY || old == k) {
                atomicAdd(&ltab[s].cs, 1u);
                if (!vn) {
                    atomicAdd(&ltab[s].cv, 1u);
                    atomicAdd(&ltab[s].sum, v);
                }
                placed = true;
                break;
            }
            s = (s + 1) & (AGG_LDS_SLOTS - 1);
        }
        /* LDS window full: spill straight to the global table */
        if (!placed && !d_agg_global_update<BOUNDED>(tab, mask, k, 1ull,
                                                     vn ? 0ull : 1ull, v)) {
            atomicAdd(abort, 1u); /* undersized: caller redoes at full cap */
            dead = true;
        }
    }
    __syncthreads();
    /* flush LDS partials into the global table */
    for (int s = threadIdx.x; s < AGG_LDS_SLOTS; s += blockDim.x) {
        if (ltab[s].key != AGG_EMPTY &&
            !d_agg_global_update<BOUNDED>(tab, mask, ltab[s].key,
                                          (unsigned long long)ltab[s].cs,
                                          (unsigned long long)ltab[s].cv,
                                          ltab[s].sum))
            atomicAdd(abort, 1u);
    }
}

__global__ void k_agg_compact(const agg_slot *tab, int64_t cap,
                              const agg_slot *nullgrp,
                              otbx_agg_group *out, int64_t *ngroups)
{
    d_block_compact(
        cap, ngroups, [=](int64_t i) { return tab[i].key != AGG_EMPTY; },
        [=](int64_t i, int64_t pos) {
            out[pos].key = tab[i].key;
            out[pos].key_isnull = 0;
            out[pos].count_star = (int64_t)tab[i].count_star;
            out[pos].count_v = (int64_t)tab[i].count_v;
            out[pos].sum_v = tab[i].sum_v;
            out[pos].sum_isnull = tab[i].count_v == 0;
        });
    /* specials: the NULL-key and AGG_EMPTY-valued-key groups */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (nullgrp->count_star > 0) {
            int64_t pos = (int64_t)atomicAdd((unsigned long long *)ngroups, 1ull);
            out[pos].key = 0;
            out[pos].key_isnull = 1;
            out[pos].count_star = (int64_t)nullgrp->count_star;
            out[pos].count_v = (int64_t)nullgrp->count_v;
            out[pos].sum_v = nullgrp->sum_v;
            out[pos].sum_isnull = nullgrp->count_v == 0;
        }
        if (nullgrp[1].count_star > 0) { /* the AGG_EMPTY-valued key group */
            int64_t pos = (int64_t)atomicAdd((unsigned long long *)ngroups, 1ull);
            out[pos].key = AGG_EMPTY;
            out[pos].key_isnull = 0;
            out[pos].count_star = (int64_t)nullgrp[1].count_star;
            out[pos].count_v = (int64_t)nullgrp[1].count_v;
            out[pos].sum_v = nullgrp[1].sum_v;
            out[pos].sum_isnull = nullgrp[1].count_v == 0;
        }
    }
}

template <typename T>
__global__ void k_gather(const T *__restrict__ src,
                         const int64_t *__restrict__ perm, int64_t n,
                         T *__restrict__ dst)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        dst[i] = src[perm[i]];
}

/* ---- partitioned aggregation (mid-cardinality; round-2 item 1) ----
 * When the distinct-key estimate exceeds what one block's LDS table can
 * absorb but is far below n, hash-partition the rows into P bucket segments
 * (each LDS-table-resident) and aggregate one bucket per block — turning
 * per-row random global atomics into sequential traffic + per-bucket LDS
 * work. Bucket = high hash bits (decorrelated from the table-slot bits). */
#define AGGP_MAX_BUCKETS 2048

__device__ __forceinline__ uint32_t d_agg_bucket(int64_t k, uint32_t nb)
{
    return (uint32_t)((d_hash_i64(k) >> 40) & (uint64_t)(nb - 1));
}

/* exact distinct count over a strided sample, via a global open-addressing
 * key set (2^21 slots, staged in the — still unused — perm region of the
 * workspace). The earlier one-block linear-counting estimator saturated
 * (65k-bit set vs a 65k sample), and its noisy collision count made the
 * birthday estimate swing 4× at 100 M groups — which undersized nb2 and
 * sent EVERY bucket down the flagged-recompute path (102 ms of a 162 ms
 * call). The birthday estimator needs the sample''s distinct count EXACTLY;
 * only a key-exact set gives it. */
#define AGG_SCAP (1ll << 21)
#define AGG_SAMPLE (1ll << 20)

__global__ void k_fill_i64(int64_t *a, int64_t n, int64_t v)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        a[i] = v;
}

__global__ void k_agg_sample_exact(const int64_t *__restrict__ keys,
                                   const uint8_t *__restrict__ knull,
                                   int64_t n, int64_t *__restrict__ stab,
                                   unsigned long long *out2 /* {d, s_eff} */)
{
    int64_t stride_n = n > AGG_SAMPLE ? n / AGG_SAMPLE : 1;
    unsigned long long mynew = 0, myproc = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         j < AGG_SAMPLE; j += stride) {
        int64_t i = j * stride_n;
        if (i >= n) break;
        if (knull && knull[i]) continue;
        myproc++;
        int64_t k = keys[i];
        int64_t pos = (int64_t)(d_hash_i64(k) & (uint64_t)(AGG_SCAP - 1));
        for (;;) {
            /* plain read first: hot keys resolve with a broadcast load —
             * 1 M CASes on 4 slots measured +3.7 ms on the 4-group case */
            long long cur = __hip_atomic_load(
                (long long *)&stab[pos], __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            if (cur == k) break;
            if (cur == AGG_EMPTY) {
                long long old = atomicCAS((unsigned long long *)&stab[pos],
                                          (unsigned long long)AGG_EMPTY,
                                          (unsigned long long)k);
                if (old == AGG_EMPTY) {
                    mynew++;
                    break;
                }
                if (old == k) break;
                continue; /* someone else claimed it: re-read this slot */
            }
            pos = (pos + 1) & (AGG_SCAP - 1);
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        mynew += __shfl_down(mynew, off, WAVE);
        myproc += __shfl_down(myproc, off, WAVE);
    }
    if ((threadIdx.x % WAVE) == 0 && (mynew | myproc)) {
        atomicAdd(&out2[0], mynew);
        atomicAdd(&out2[1], myproc);
    }
}

__global__ void k_aggp_count(const int64_t *__restrict__ keys,
                             const uint8_t *__restrict__ knull, int64_t n,
                             uint32_t nb, unsigned long long *counts)
{
    __shared__ unsigned int bc[AGGP_MAX_BUCKETS];
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x) bc[i] = 0;
    __syncthreads();
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (knull && knull[i]) continue;
        atomicAdd(&bc[d_agg_bucket(keys[i], nb)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x)
        if (bc[i]) atomicAdd(&counts[i], (unsigned long long)bc[i]);
}

__global__ void k_aggp_scatter(const int64_t *__restrict__ keys,
                               const uint8_t *__restrict__ knull, int64_t n,
                               uint32_t nb, unsigned long long *cursor,
                               int64_t *__restrict__ perm)
{
    __shared__ unsigned int lcur[AGGP_MAX_BUCKETS];
    __shared__ long long base[AGGP_MAX_BUCKETS];
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x) lcur[i] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (knull && knull[i]) continue;
        atomicAdd(&lcur[d_agg_bucket(keys[i], nb)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x) {
        base[i] = lcur[i] ? (long long)atomicAdd(
                                &cursor[i], (unsigned long long)lcur[i])
                          : 0;
        lcur[i] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (knull && knull[i]) continue;
        uint32_t b = d_agg_bucket(keys[i], nb);
        unsigned int off = atomicAdd(&lcur[b], 1u);
        perm[base[b] + off] = i;
    }
}

/* direct (key,val) record scatter — the no-NULL fast path: one pass, no
 * index gathers (an index permutation would make every downstream gather a
 * random 64-B line read — measured 2x slower end to end) */
__global__ void k_aggp_scatter_kv(const int64_t *__restrict__ keys,
                                  const double *__restrict__ vals, int64_t n,
                                  uint32_t nb, unsigned long long *cursor,
                                  ulonglong2 *__restrict__ recs)
{
    __shared__ unsigned int lcur[AGGP_MAX_BUCKETS];
    __shared__ long long base[AGGP_MAX_BUCKETS];
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x) lcur[i] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        atomicAdd(&lcur[d_agg_bucket(keys[i], nb)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x) {
        base[i] = lcur[i] ? (long long)atomicAdd(
                                &cursor[i], (unsigned long long)lcur[i])
                          : 0;
        lcur[i] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        int64_t k = keys[i];
        uint32_t b = d_agg_bucket(k, nb);
        unsigned int off = atomicAdd(&lcur[b], 1u);
        ulonglong2 r;
        r.x = (unsigned long long)k;
        r.y = (unsigned long long)__double_as_longlong(vals[i]);
        recs[base[b] + off] = r;
    }
}

/* level-2 bucket bits: decorrelated from both the level-1 bits (>>40) and
 * the LDS-slot bits (low) */
__device__ __forceinline__ uint32_t d_agg_bucket2(int64_t k, uint32_t nb2)
{
    return (uint32_t)((d_hash_i64(k) >> 28) & (uint64_t)(nb2 - 1));
}

/* second partition level (kv fast path): block b re-partitions level-1
 * bucket b's record segment into nb2 sub-buckets, in place of the random
 * global spills that dominate when est/nb1 overflows the 1024-slot LDS
 * table (measured 1.9 Grows/s at 100 M groups). Segment-local: the block
 * counts, serial-scans, then scatters — 3 streaming passes. */
__global__ void k_aggp_scatter_kv2(const ulonglong2 *__restrict__ recs,
                                   const unsigned long long *__restrict__ offs,
                                   const unsigned long long *__restrict__ cnts,
                                   uint32_t nb2, ulonglong2 *__restrict__ recs2,
                                   unsigned long long *__restrict__ offs2,
                                   unsigned long long *__restrict__ cnts2)
{
    __shared__ unsigned int c2[AGGP_MAX_BUCKETS];
    __shared__ unsigned long long b2[AGGP_MAX_BUCKETS];
    int64_t lo = (int64_t)offs[blockIdx.x];
    int64_t hi = lo + (int64_t)cnts[blockIdx.x];
    for (int j = threadIdx.x; j < (int)nb2; j += blockDim.x) c2[j] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        atomicAdd(&c2[d_agg_bucket2((int64_t)recs[i].x, nb2)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = (unsigned long long)lo;
        for (uint32_t j = 0; j < nb2; j++) {
            b2[j] = acc;
            offs2[(size_t)blockIdx.x * nb2 + j] = acc;
            cnts2[(size_t)blockIdx.x * nb2 + j] = c2[j];
            acc += c2[j];
            c2[j] = 0;
        }
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        ulonglong2 r = recs[i];
        uint32_t j = d_agg_bucket2((int64_t)r.x, nb2);
        unsigned int off = atomicAdd(&c2[j], 1u);
        recs2[b2[j] + off] = r;
    }
}

/* ---- tile-staged counting-sort partitioner (OTBX_PART_TILE) ----------
 * Replaces the cursor scatters above (§8b.0; default ON, =0 restores
 * them). A/B-measured in tools/microbench/scatter_ab.hip
 * (profiles/r01_scatter_ab.txt): at 600 M rows the tile sort at fanout 256
 * runs 7.30 ms vs 14.14 ms for the shipped cursor-scatter shape — the
 * random 16-B record writes become coalesced per-bucket runs (avg 32
 * records = 512 B at nb=256; fanout 2048 keeps runs at 4 records and loses
 * the gain, hence the level-1 fanout drops to 256 and level-2 takes up to
 * 2048). Per tile of 8192 rows: LDS histogram -> serial exclusive scan ->
 * LDS-sorted stage -> one global cursor reservation per (tile, bucket) ->
 * linear coalesced write-out. delta[] folds (segment run base - tile-local
 * base) into one u32 per bucket (mod-2^32 arithmetic — requires n < 2^32,
 * which the workspace sizes already imply). */
#define PT_TILE 8192

/* level 1: keys[] (+ optional knull skip list) -> (key, payload) records;
 * vals == NULL emits the row index as payload (the join shape), else the
 * double bits (the agg kv shape). nb ≤ 256. */
typedef long long otbx_ll2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(1024) void k_tile_scatter1(
    const int64_t *__restrict__ keys, const uint8_t *__restrict__ knull,
    const double *__restrict__ vals, int64_t n, uint32_t nb,
    unsigned long long *__restrict__ cursor, ulonglong2 *__restrict__ recs)
{
    __shared__ ulonglong2 stage[PT_TILE];
    __shared__ unsigned int hist[256], excl[256], delta[256];
    __shared__ unsigned int tot;
    /* 16-B vector path needs 16-B-aligned bases (lo is even, so tile
     * offsets preserve base alignment) and no null bitmap */
    const bool vec = !knull &&
                     (((uintptr_t)keys | (vals ? (uintptr_t)vals : 0)) & 15)
                         == 0;
    int64_t ntiles = (n + PT_TILE - 1) / PT_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t lo = t * (int64_t)PT_TILE;
        int tn = (int)(n - lo < PT_TILE ? n - lo : PT_TILE);
        int tq = tn / 2;
        const otbx_ll2 *k2 = (const otbx_ll2 *)(keys + lo);
        for (int j = threadIdx.x; j < (int)nb; j += blockDim.x) hist[j] = 0;
        __syncthreads();
        if (vec) {
            /* microbenched fast path (scatter_ab v7, profiles/
             * r2_scatter_ab.txt: 5.14 vs 7.34 ms at 600 M): 2 rows/thread,
             * 16-B vector loads in the hist and stage passes */
            for (int q = threadIdx.x; q < tq; q += blockDim.x) {
                otbx_ll2 kk = k2[q];
                atomicAdd(&hist[d_agg_bucket(kk.x, nb)], 1u);
                atomicAdd(&hist[d_agg_bucket(kk.y, nb)], 1u);
            }
            if (threadIdx.x == 0 && (tn & 1))
                atomicAdd(&hist[d_agg_bucket(keys[lo + tn - 1], nb)], 1u);
        } else {
            for (int i = threadIdx.x; i < tn; i += blockDim.x) {
                if (knull && knull[lo + i]) continue;
                atomicAdd(&hist[d_agg_bucket(keys[lo + i], nb)], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int acc = 0;
            for (uint32_t j = 0; j < nb; j++) {
                excl[j] = acc;
                acc += hist[j];
            }
            tot = acc;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < (int)nb; j += blockDim.x) {
            unsigned int rb =
                hist[j] ? (unsigned int)atomicAdd(&cursor[j],
                                                  (unsigned long long)hist[j])
                        : 0u;
            delta[j] = rb - excl[j]; /* mod 2^32 */
            hist[j] = 0;             /* reused as the stage cursor */
        }
        __syncthreads();
        if (vec) {
            for (int q = threadIdx.x; q < tq; q += blockDim.x) {
                otbx_ll2 kk = k2[q];
                uint32_t b0 = d_agg_bucket(kk.x, nb);
                uint32_t b1 = d_agg_bucket(kk.y, nb);
                unsigned int r0 = excl[b0] + atomicAdd(&hist[b0], 1u);
                unsigned int r1 = excl[b1] + atomicAdd(&hist[b1], 1u);
                ulonglong2 ra, rb;
                ra.x = (unsigned long long)kk.x;
                rb.x = (unsigned long long)kk.y;
                if (vals) {
                    double2 vv = ((const double2 *)(vals + lo))[q];
                    ra.y = (unsigned long long)__double_as_longlong(vv.x);
                    rb.y = (unsigned long long)__double_as_longlong(vv.y);
                } else {
                    ra.y = (unsigned long long)(lo + 2 * (int64_t)q);
                    rb.y = (unsigned long long)(lo + 2 * (int64_t)q + 1);
                }
                stage[r0] = ra;
                stage[r1] = rb;
            }
            if (threadIdx.x == 0 && (tn & 1)) {
                int64_t k = keys[lo + tn - 1];
                uint32_t b = d_agg_bucket(k, nb);
                unsigned int r = excl[b] + atomicAdd(&hist[b], 1u);
                ulonglong2 rr;
                rr.x = (unsigned long long)k;
                rr.y = vals ? (unsigned long long)__double_as_longlong(
                                  vals[lo + tn - 1])
                            : (unsigned long long)(lo + tn - 1);
                stage[r] = rr;
            }
        } else {
            for (int i = threadIdx.x; i < tn; i += blockDim.x) {
                if (knull && knull[lo + i]) continue;
                int64_t k = keys[lo + i];
                uint32_t b = d_agg_bucket(k, nb);
                unsigned int r = excl[b] + atomicAdd(&hist[b], 1u);
                ulonglong2 rec;
                rec.x = (unsigned long long)k;
                rec.y = vals ? (unsigned long long)__double_as_longlong(
                                   vals[lo + i])
                             : (unsigned long long)(lo + i);
                stage[r] = rec;
            }
        }
        __syncthreads();
        int wtot = (int)tot;
        for (int p = threadIdx.x; p < wtot; p += blockDim.x) {
            ulonglong2 rec = stage[p];
            uint32_t b = d_agg_bucket((int64_t)rec.x, nb);
            recs[(size_t)(uint32_t)(delta[b] + (unsigned int)p)] = rec;
        }
        __syncthreads();
    }
}

/* level-2 sub-bucket histogram: grid (blocks-per-segment, nb segments);
 * cnts2 must be zeroed first */
__global__ void k_tile_count2(const ulonglong2 *__restrict__ recs,
                              const unsigned long long *__restrict__ offs,
                              const unsigned long long *__restrict__ cnts,
                              uint32_t nb2,
                              unsigned long long *__restrict__ cnts2)
{
    __shared__ unsigned int h[AGGP_MAX_BUCKETS];
    int sg = blockIdx.y;
    int64_t lo = (int64_t)offs[sg];
    int64_t hi = lo + (int64_t)cnts[sg];
    for (int j = threadIdx.x; j < (int)nb2; j += blockDim.x) h[j] = 0;
    __syncthreads();
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = lo + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < hi; i += stride)
        atomicAdd(&h[d_agg_bucket2((int64_t)recs[i].x, nb2)], 1u);
    __syncthreads();
    for (int j = threadIdx.x; j < (int)nb2; j += blockDim.x)
        if (h[j])
            atomicAdd(&cnts2[(size_t)sg * nb2 + j], (unsigned long long)h[j]);
}

/* per-segment serial exclusive scan: offs2[s][j] = offs[s] + Σ cnts2[s][<j]
 * (one block per segment; nb2 ≤ 2048 so a serial loop is cheap) */
__global__ void k_tile_scan2(const unsigned long long *__restrict__ offs,
                             uint32_t nb2,
                             const unsigned long long *__restrict__ cnts2,
                             unsigned long long *__restrict__ offs2)
{
    if (threadIdx.x != 0) return;
    unsigned long long acc = offs[blockIdx.x];
    for (uint32_t j = 0; j < nb2; j++) {
        offs2[(size_t)blockIdx.x * nb2 + j] = acc;
        acc += cnts2[(size_t)blockIdx.x * nb2 + j];
    }
}

/* level 2: tile sort within each level-1 segment (records in, records
 * out). cursor2 is offs2 itself, mutated by the run reservations —
 * k_tile_restore_offs subtracts cnts2 afterwards to recover the segment
 * starts for the bucket kernels. nb2 ≤ 2048. */
__global__ __launch_bounds__(1024) void k_tile_scatter2(
    const ulonglong2 *__restrict__ recs,
    const unsigned long long *__restrict__ offs,
    const unsigned long long *__restrict__ cnts, uint32_t nb2,
    unsigned long long *__restrict__ cursor2, ulonglong2 *__restrict__ recs2)
{
    __shared__ ulonglong2 stage[PT_TILE];
    __shared__ unsigned int hist[AGGP_MAX_BUCKETS];
    __shared__ unsigned int excl[AGGP_MAX_BUCKETS];
    __shared__ unsigned int delta[AGGP_MAX_BUCKETS];
    int sg = blockIdx.y;
    int64_t slo = (int64_t)offs[sg];
    int64_t scnt = (int64_t)cnts[sg];
    int64_t ntiles = (scnt + PT_TILE - 1) / PT_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t lo = slo + t * (int64_t)PT_TILE;
        int tn = (int)(slo + scnt - lo < PT_TILE ? slo + scnt - lo : PT_TILE);
        for (int j = threadIdx.x; j < (int)nb2; j += blockDim.x) hist[j] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < tn; i += blockDim.x)
            atomicAdd(&hist[d_agg_bucket2((int64_t)recs[lo + i].x, nb2)], 1u);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int acc = 0;
            for (uint32_t j = 0; j < nb2; j++) {
                excl[j] = acc;
                acc += hist[j];
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < (int)nb2; j += blockDim.x) {
            unsigned int rb =
                hist[j]
                    ? (unsigned int)atomicAdd(&cursor2[(size_t)sg * nb2 + j],
                                              (unsigned long long)hist[j])
                    : 0u;
            delta[j] = rb - excl[j]; /* mod 2^32 */
            hist[j] = 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < tn; i += blockDim.x) {
            ulonglong2 rec = recs[lo + i];
            uint32_t b = d_agg_bucket2((int64_t)rec.x, nb2);
            unsigned int r = excl[b] + atomicAdd(&hist[b], 1u);
            stage[r] = rec;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < tn; p += blockDim.x) {
            ulonglong2 rec = stage[p];
            uint32_t b = d_agg_bucket2((int64_t)rec.x, nb2);
            recs2[(size_t)(uint32_t)(delta[b] + (unsigned int)p)] = rec;
        }
        __syncthreads();
    }
}

__global__ void k_tile_restore_offs(unsigned long long *__restrict__ offs2,
                                    const unsigned long long *__restrict__
                                        cnts2,
                                    int64_t n)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        offs2[i] -= cnts2[i];
}

/* default ON (measured on MI355X, gpurun_out/tile_ops_bench.txt →
 * profiles/r01_tile_ops.txt: agg-100M 29.4→22.8 ms, join-150M 38.7→34.2,
 * join-15M 28.8→23.2, agg-1M 19.9→18.5, all parity-green);
 * OTBX_PART_TILE=0 selects the legacy cursor scatters (kept as the
 * fallback for NULL-carrying agg inputs and n ≥ 2^32, and pinned by the
 * *_legacy_parity tests) */
static inline bool part_tile_enabled(void)
{
    const char *e = getenv("OTBX_PART_TILE");
    return !e || atoi(e);
}

/* direct-emit per-bucket aggregation: two-level buckets hold DISJOINT key
 * sets, so a bucket that fits its LDS table emits its groups straight to
 * the output — no shared global table, no cap-sized init or compact scan
 * (those dominated the 100 M-group case: 34 GB init + scan + 100 M random
 * CAS flushes). A bucket whose LDS table overflows (est noise/skew) is
 * FLAGGED and recomputed by k_aggp_bucket_agg_kv_flagged through the
 * global table; its LDS result is discarded. */
__global__ void k_aggp_bucket_agg_kv_direct(
    const ulonglong2 *__restrict__ recs,
    const unsigned long long *__restrict__ offs,
    const unsigned long long *__restrict__ cnts, uint8_t *__restrict__ flags,
    unsigned int *nflagged, otbx_agg_group *__restrict__ out,
    int64_t *ngroups)
{
    const int LSLOTS = 1024;
    __shared__ agg_lds_slot ltab[LSLOTS];
    __shared__ int bfail;
    if (threadIdx.x == 0) bfail = 0;
    for (int t = threadIdx.x; t < LSLOTS; t += blockDim.x) {
        ltab[t].key = AGG_EMPTY;
        ltab[t].cs = 0;
        ltab[t].cv = 0;
        ltab[t].sum = 0.0;
    }
    __syncthreads();
    int64_t lo = (int64_t)offs[blockIdx.x];
    int64_t hi = lo + (int64_t)cnts[blockIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        ulonglong2 r = recs[i];
        int64_t k = (int64_t)r.x;
        double v = __longlong_as_double((long long)r.y);
        if (k == AGG_EMPTY)
            continue; /* handled by k_aggp_specials */
        uint64_t h = d_hash_i64(k);
        int64_t t0 = (int64_t)(h & (uint64_t)(LSLOTS - 1));
        /* odd-step double hashing: linear runs at ~0.4 load flagged whole
         * buckets often enough that their recompute dominated */
        int64_t step = (int64_t)(((h >> 52) & (uint64_t)(LSLOTS - 2)) | 1ull);
        bool placed = false;
        for (int t = 0; t < 64; t++) {
            long long old = atomicCAS((unsigned long long *)&ltab[t0].key,
                                      (unsigned long long)AGG_EMPTY,
                                      (unsigned long long)k);
            if (old == AGG_EMPTY || old == k) {
                atomicAdd(&ltab[t0].cs, 1u);
                atomicAdd(&ltab[t0].cv, 1u);
                atomicAdd(&ltab[t0].sum, v);
                placed = true;
                break;
            }
            t0 = (t0 + step) & (LSLOTS - 1);
        }
        if (!placed) bfail = 1; /* plain store: any-lane sets, read after
                                 * barrier */
    }
    __syncthreads();
    if (bfail) {
        if (threadIdx.x == 0) {
            flags[blockIdx.x] = 1;
            atomicAdd(nflagged, 1u);
        }
        return;
    }
    /* block-aggregated flush: ONE global reservation per block (per-wave
     * wave_append over 262k blocks × 16 waves made 4.2 M single-counter
     * reservations = 47 of this kernel''s 50 ms at 100 M groups) */
    __shared__ unsigned long long fbase;
    __shared__ unsigned int fcnt;
    if (threadIdx.x == 0) fcnt = 0;
    __syncthreads();
    int lane = (int)(threadIdx.x % WAVE);
    for (int t = threadIdx.x; t < LSLOTS; t += blockDim.x) {
        unsigned long long m = __ballot(ltab[t].key != AGG_EMPTY);
        if (lane == 0 && m) atomicAdd(&fcnt, (unsigned int)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        fbase = fcnt ? (unsigned long long)atomicAdd(
                           (unsigned long long *)ngroups,
                           (unsigned long long)fcnt)
                     : 0;
        fcnt = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < LSLOTS; t += blockDim.x) {
        bool used = ltab[t].key != AGG_EMPTY;
        unsigned long long m = __ballot(used);
        if (!m) continue;
        unsigned int wbase = 0;
        if (lane == 0) wbase = atomicAdd(&fcnt, (unsigned int)__popcll(m));
        wbase = (unsigned int)__shfl((int)wbase, 0, WAVE);
        if (used) {
            int64_t pos = (int64_t)fbase + wbase +
                          __popcll(m & ((1ull << lane) - 1ull));
            out[pos].key = ltab[t].key;
            out[pos].key_isnull = 0;
            out[pos].count_star = (int64_t)ltab[t].cs;
            out[pos].count_v = (int64_t)ltab[t].cv;
            out[pos].sum_v = ltab[t].sum;
            out[pos].sum_isnull = ltab[t].cv == 0;
        }
    }
}

/* recompute pass for flagged (overflowed) buckets: straight through the
 * shared global table; k_agg_compact then appends those groups. */
__global__ void k_aggp_bucket_agg_kv_flagged(
    const ulonglong2 *__restrict__ recs,
    const unsigned long long *__restrict__ offs,
    const unsigned long long *__restrict__ cnts,
    const uint8_t *__restrict__ flags, agg_slot *tab, int64_t cap)
{
    if (!flags[blockIdx.x]) return;
    int64_t mask = cap - 1;
    int64_t lo = (int64_t)offs[blockIdx.x];
    int64_t hi = lo + (int64_t)cnts[blockIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        ulonglong2 r = recs[i];
        int64_t k = (int64_t)r.x;
        if (k == AGG_EMPTY) continue;
        d_agg_global_update(tab, mask, k, 1ull, 1ull,
                            __longlong_as_double((long long)r.y));
    }
}

/* append the two special groups (NULL key, AGG_EMPTY-sentinel key) when the
 * direct path skipped k_agg_compact */
__global__ void k_agg_emit_specials(const agg_slot *nullgrp,
                                    otbx_agg_group *out, int64_t *ngroups)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (nullgrp->count_star > 0) {
            int64_t pos =
                (int64_t)atomicAdd((unsigned long long *)ngroups, 1ull);
            out[pos].key = 0;
            out[pos].key_isnull = 1;
            out[pos].count_star = (int64_t)nullgrp->count_star;
            out[pos].count_v = (int64_t)nullgrp->count_v;
            out[pos].sum_v = nullgrp->sum_v;
            out[pos].sum_isnull = nullgrp->count_v == 0;
        }
        if (nullgrp[1].count_star > 0) {
            int64_t pos =
                (int64_t)atomicAdd((unsigned long long *)ngroups, 1ull);
            out[pos].key = AGG_EMPTY;
            out[pos].key_isnull = 0;
            out[pos].count_star = (int64_t)nullgrp[1].count_star;
            out[pos].count_v = (int64_t)nullgrp[1].count_v;
            out[pos].sum_v = nullgrp[1].sum_v;
            out[pos].sum_isnull = nullgrp[1].count_v == 0;
        }
    }
}

/* accumulate NULL-key rows (and AGG_EMPTY-valued keys, which the partition
 * passes route normally but the per-bucket table cannot hold) */
__global__ void k_aggp_specials(const int64_t *__restrict__ keys,
                                const uint8_t *__restrict__ knull,
                                const double *__restrict__ vals,
                                const uint8_t *__restrict__ vnull, int64_t n,
                                agg_slot *nullgrp)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long cs0 = 0, cv0 = 0, cs1 = 0, cv1 = 0;
    double s0 = 0, s1 = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        bool kn = knull && knull[i];
        bool sent = !kn && keys[i] == AGG_EMPTY;
        if (!kn && !sent) continue;
        bool vn = vnull && vnull[i];
        double v = vn ? 0.0 : vals[i];
        if (kn) {
            cs0++;
            if (!vn) { cv0++; s0 += v; }
        } else {
            cs1++;
            if (!vn) { cv1++; s1 += v; }
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        cs0 += __shfl_down(cs0, off, WAVE);
        cv0 += __shfl_down(cv0, off, WAVE);
        s0 += __shfl_down(s0, off, WAVE);
        cs1 += __shfl_down(cs1, off, WAVE);
        cv1 += __shfl_down(cv1, off, WAVE);
        s1 += __shfl_down(s1, off, WAVE);
    }
    if ((threadIdx.x % WAVE) == 0) {
        if (cs0) {
            atomicAdd(&nullgrp[0].count_star, cs0);
            if (cv0) {
                atomicAdd(&nullgrp[0].count_v, cv0);
                atomicAdd(&nullgrp[0].sum_v, s0);
            }
        }
        if (cs1) {
            atomicAdd(&nullgrp[1].count_star, cs1);
            if (cv1) {
                atomicAdd(&nullgrp[1].count_v, cv1);
                atomicAdd(&nullgrp[1].sum_v, s1);
            }
        }
    }
}

/* per-bucket aggregation: block b owns the partitioned segment of bucket b
 * (offsets from the scanned counts); rows were gathered into partitioned
 * order so the reads stream. LDS table + global spill (same update fn). */
__global__ void k_aggp_bucket_agg(const int64_t *__restrict__ pkeys,
                                  const double *__restrict__ pvals,
                                  const uint8_t *__restrict__ pvnull,
                                  const unsigned long long *__restrict__ offs,
                                  const unsigned long long *__restrict__ cnts,
                                  agg_slot *tab, int64_t cap)
{
    const int LSLOTS = 1024;
    __shared__ agg_lds_slot ltab[LSLOTS];
    for (int s = threadIdx.x; s < LSLOTS; s += blockDim.x) {
        ltab[s].key = AGG_EMPTY;
        ltab[s].cs = 0;
        ltab[s].cv = 0;
        ltab[s].sum = 0.0;
    }
    __syncthreads();
    int64_t mask = cap - 1;
    int64_t lo = (int64_t)offs[blockIdx.x];
    int64_t hi = lo + (int64_t)cnts[blockIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        int64_t k = pkeys[i];
        bool vn = pvnull && pvnull[i];
        double v = vn ? 0.0 : pvals[i];
        if (k == AGG_EMPTY) /* handled by k_aggp_specials */
            continue;
        int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)(LSLOTS - 1));
        bool placed = false;
        for (int t = 0; t < 8; t++) {
            long long old = atomicCAS((unsigned long long *)&ltab[s].key,
                                      (unsigned long long)AGG_EMPTY,
                                      (unsigned long long)k);
            if (old == AGG_EMPTY || old == k) {
                atomicAdd(&ltab[s].cs, 1u);
                if (!vn) {
                    atomicAdd(&ltab[s].cv, 1u);
                    atomicAdd(&ltab[s].sum, v);
                }
                placed = true;
                break;
            }
            s = (s + 1) & (LSLOTS - 1);
        }
        if (!placed)
            d_agg_global_update(tab, mask, k, 1ull, vn ? 0ull : 1ull, v);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < LSLOTS; s += blockDim.x) {
        if (ltab[s].key != AGG_EMPTY)
            d_agg_global_update(tab, mask, ltab[s].key,
                                (unsigned long long)ltab[s].cs,
                                (unsigned long long)ltab[s].cv, ltab[s].sum);
    }
}

extern "C" {

#define AGGP_THRESHOLD (8ll << 20) /* rows: partitioned path considered */

otbx_status otbx_agg_i64_workspace_bytes(int64_t n, size_t *bytes)
{
    int64_t cap = next_pow2_host(n < 16 ? 16 : (int64_t)(n / 0.7) + 1);
    size_t b = (size_t)(cap + 2) * sizeof(agg_slot); /* + NULL and
                                                      * sentinel-key groups */
    if (n >= AGGP_THRESHOLD) {
        /* partitioned-path buffers: perm + partitioned key/val/vnull copies
         * + bucket counts/cursor/offsets, plus the level-2 record buffer
         * and sub-bucket arrays of the two-level kv path */
        b += (size_t)n * (8 + 8 + 8 + 1 + 16) +
             (size_t)AGGP_MAX_BUCKETS * 8 * 3 +
             (size_t)(1 << 19) * (8 * 2 + 1) + 8192;
    }
    *bytes = b;
    return OTBX_OK;
}

/* what the partitioned direct path leaves behind in the workspace: the
 * (key,val) records grouped into key-disjoint buckets. otbx_agg_i64_var
 * runs its second pass over them; nbuckets == 0 = another path was taken */
struct agg_part_layout {
    const ulonglong2 *recs;
    const unsigned long long *offs, *cnts;
    const uint8_t *flags; /* 1 = bucket overflowed its LDS table */
    uint32_t nbuckets;
};

static otbx_status agg_i64_run(const int64_t *keys, const uint8_t *knull,
                               const double *vals, const uint8_t *vnull,
                               int64_t n, void *ws, size_t ws_bytes,
                               otbx_agg_group *out, int64_t *ngroups_dev,
                               void *stream, agg_part_layout *lay)
{
    int64_t cap = next_pow2_host(n < 16 ? 16 : (int64_t)(n / 0.7) + 1);
    {
        size_t need;
        otbx_agg_i64_workspace_bytes(n, &need);
        if (ws_bytes < need) return OTBX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    agg_slot *tab = (agg_slot *)ws;
    agg_slot *nullgrp = tab + cap;
    HIP_CHECK(hipMemsetAsync(ngroups_dev, 0, sizeof(int64_t), s));
    if (n == 0) {
        HIP_CHECK(hipGetLastError());
        return OTBX_OK;
    }

    /* path decision first: the two-level direct path never touches the
     * cap-sized global table, so its init (34 GB of writes at n=600 M) is
     * skipped unless actually needed */
    int64_t est = 0;
    bool partitioned = false;
    if (n >= AGGP_THRESHOLD) {
        static unsigned long long *d_ds = nullptr;
        static unsigned long long *h_ds = nullptr;
        if (!d_ds) {
            SCR_ALLOC_DEV(d_ds, 16);
            SCR_ALLOC_HOST(h_ds, 16);
        }
        /* sample set lives in the (still unwritten) perm region */
        int64_t *stab = (int64_t *)((char *)(nullgrp + 2));
        HIP_CHECK(hipMemsetAsync(d_ds, 0, 16, s));
        hipLaunchKernelGGL(k_fill_i64, dim3(grid_for(AGG_SCAP, 256)),
                           dim3(256), 0, s, stab, AGG_SCAP, AGG_EMPTY);
        hipLaunchKernelGGL(k_agg_sample_exact,
                           dim3(grid_for(AGG_SAMPLE, 256)), dim3(256), 0, s,
                           keys, knull, n, stab, d_ds);
        HIP_CHECK(hipMemcpyAsync(h_ds, d_ds, 16, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        double d = (double)h_ds[0], se = (double)h_ds[1];
        if (se < 1.0) se = 1.0;
        if (d < se / 2.0) {
            est = (int64_t)d; /* sample saturated the key domain */
        } else {
            double c = se - d;
            if (c < 1.0) c = 1.0;
            est = (int64_t)(se * se / (2.0 * c)); /* birthday */
        }
        if (est > n) est = n;
        /* two-level partitioning (kv fast path only) extends the reach far
         * past the single-level 2048×~768 ≈ 1.5 M-group ceiling */
        int64_t est_cap = (!knull && !vnull) ? (256ll << 20) : (32ll << 20);
        partitioned = est > 1536 && est <= est_cap;
    }

    /* tile-sort partitioner (§8b.0, default ON — see part_tile_enabled):
     * level-1 fanout drops to 256 so the per-bucket write runs coalesce;
     * level-2 fanout grows to compensate (same total nb*nb2). */
    bool tile = part_tile_enabled() && !knull && !vnull &&
                n < (int64_t)UINT32_MAX;
    uint32_t nb = 0, nb2 = 1;
    if (partitioned) {
        nb = (uint32_t)next_pow2_host(est / 256 < 64 ? 64 : est / 256);
        if (nb > AGGP_MAX_BUCKETS) nb = AGGP_MAX_BUCKETS;
        if (tile && nb > 256) nb = 256;
        int64_t per_b = est / nb;
        if (!knull && !vnull && per_b > 768) {
            nb2 = (uint32_t)next_pow2_host(per_b / 384 + 1);
            if (nb2 > AGGP_MAX_BUCKETS) nb2 = AGGP_MAX_BUCKETS;
            while ((size_t)nb * nb2 > (1 << 19)) nb2 >>= 1;
        }
    }
    /* buckets are key-disjoint at either level, so the whole kv fast path
     * emits direct — no global table, no cap-sized init or compact scan */
    bool direct = partitioned && !knull && !vnull;
    bool smalltab = !partitioned && est > 0 && est <= 1536;
    if (direct)
        HIP_CHECK(hipMemsetAsync(nullgrp, 0, 2 * sizeof(agg_slot), s));
    else if (!smalltab) /* the small-table attempt inits its own size */
        hipLaunchKernelGGL(k_agg_init, dim3(grid_for(cap + 2, 256)), dim3(256),
                           0, s, tab, cap + 2);

    bool compact_tab = !direct; /* does the final compact scan the table? */
    if (partitioned) {
        char *p = (char *)(nullgrp + 2);
        int64_t *perm = (int64_t *)p;
        int64_t *pkeys = perm + n;
        double *pvals = (double *)(pkeys + n);
        uint8_t *pvnull = (uint8_t *)(pvals + n);
        unsigned long long *cnts =
            (unsigned long long *)(pvnull + ((n + 63) & ~63ll));
        unsigned long long *cursor = cnts + AGGP_MAX_BUCKETS;
        unsigned long long *offs = cursor + AGGP_MAX_BUCKETS;
        unsigned long long *cnts2 = offs + AGGP_MAX_BUCKETS;
        unsigned long long *offs2 = cnts2 + (1 << 19);
        uint8_t *flags = (uint8_t *)(offs2 + (1 << 19));
        ulonglong2 *recs2 = (ulonglong2 *)(flags + (1 << 19));
        HIP_CHECK(hipMemsetAsync(cnts, 0, (size_t)nb * 8, s));
        hipLaunchKernelGGL(k_aggp_count, dim3(grid_for(n, 256)), dim3(256), 0,
                           s, keys, knull, n, nb, cnts);
        static unsigned long long *h_cnts = nullptr;
        if (!h_cnts)
            SCR_ALLOC_HOST(h_cnts, AGGP_MAX_BUCKETS * 8 * 2);
        HIP_CHECK(hipMemcpyAsync(h_cnts, cnts, (size_t)nb * 8,
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        unsigned long long *h_offs = h_cnts + AGGP_MAX_BUCKETS;
        unsigned long long acc = 0;
        for (uint32_t b = 0; b < nb; b++) {
            h_offs[b] = acc;
            acc += h_cnts[b];
        }
        HIP_CHECK(hipMemcpyAsync(offs, h_offs, (size_t)nb * 8,
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(cursor, h_offs, (size_t)nb * 8,
                                 hipMemcpyHostToDevice, s));
        int64_t nr = (int64_t)acc; /* partitioned (non-NULL-key) rows */
        if (!knull && !vnull) {
            /* fast path: scatter (key,val) records directly — no index
             * gathers */
            ulonglong2 *recs = (ulonglong2 *)perm; /* n×16 ≤ region */
            if (tile)
                hipLaunchKernelGGL(k_tile_scatter1, dim3(2048), dim3(1024), 0,
                                   s, keys, nullptr, vals, n, nb, cursor,
                                   recs);
            else
                hipLaunchKernelGGL(k_aggp_scatter_kv, dim3(grid_for(n, 256)),
                                   dim3(256), 0, s, keys, vals, n, nb, cursor,
                                   recs);
            if (nr > 0) {
                static unsigned int *d_nflag = nullptr;
                static unsigned int *h_nflag = nullptr;
                if (!d_nflag) {
                    SCR_ALLOC_DEV(d_nflag, 4);
                    SCR_ALLOC_HOST(h_nflag, 4);
                }
                const ulonglong2 *frecs = recs;
                const unsigned long long *foffs = offs, *fcnts = cnts;
                uint32_t fgrid = nb;
                if (nb2 > 1) { /* second partition level */
                    if (tile) {
                        HIP_CHECK(hipMemsetAsync(cnts2, 0,
                                                 (size_t)nb * nb2 * 8, s));
                        hipLaunchKernelGGL(k_tile_count2, dim3(16, nb),
                                           dim3(256), 0, s, recs, offs, cnts,
                                           nb2, cnts2);
                        hipLaunchKernelGGL(k_tile_scan2, dim3(nb), dim3(64),
                                           0, s, offs, nb2, cnts2, offs2);
                        hipLaunchKernelGGL(k_tile_scatter2, dim3(8, nb),
                                           dim3(1024), 0, s, recs, offs, cnts,
                                           nb2, offs2, recs2);
                        hipLaunchKernelGGL(
                            k_tile_restore_offs,
                            dim3(grid_for((int64_t)nb * nb2, 256)), dim3(256),
                            0, s, offs2, cnts2, (int64_t)nb * nb2);
                    } else {
                        hipLaunchKernelGGL(k_aggp_scatter_kv2, dim3(nb),
                                           dim3(256), 0, s, recs, offs, cnts,
                                           nb2, recs2, offs2, cnts2);
                    }
                    frecs = recs2;
                    foffs = offs2;
                    fcnts = cnts2;
                    fgrid = (uint32_t)(nb * nb2);
                }
                HIP_CHECK(hipMemsetAsync(d_nflag, 0, 4, s));
                HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)fgrid, s));
                hipLaunchKernelGGL(k_aggp_bucket_agg_kv_direct, dim3(fgrid),
                                   dim3(256), 0, s, frecs, foffs, fcnts,
                                   flags, d_nflag, out, ngroups_dev);
                HIP_CHECK(hipMemcpyAsync(h_nflag, d_nflag, 4,
                                         hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                if (*h_nflag > 0) {
                    /* rare: est noise/skew overflowed some LDS tables —
                     * recompute those buckets through the global table */
                    hipLaunchKernelGGL(k_agg_init, dim3(grid_for(cap, 256)),
                                       dim3(256), 0, s, tab, cap);
                    hipLaunchKernelGGL(k_aggp_bucket_agg_kv_flagged,
                                       dim3(fgrid), dim3(256), 0, s, frecs,
                                       foffs, fcnts, flags, tab, cap);
                    compact_tab = true;
                }
                if (lay) {
                    lay->recs = frecs;
                    lay->offs = foffs;
                    lay->cnts = fcnts;
                    lay->flags = flags;
                    lay->nbuckets = fgrid;
                }
            }
        } else {
            hipLaunchKernelGGL(k_aggp_scatter, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, keys, knull, n, nb, cursor,
                               perm);
            if (nr > 0) {
                hipLaunchKernelGGL(k_gather<int64_t>, dim3(grid_for(nr, 256)),
                                   dim3(256), 0, s, keys, perm, nr, pkeys);
                hipLaunchKernelGGL(k_gather<double>, dim3(grid_for(nr, 256)),
                                   dim3(256), 0, s, vals, perm, nr, pvals);
                if (vnull)
                    hipLaunchKernelGGL(k_gather<uint8_t>,
                                       dim3(grid_for(nr, 256)), dim3(256), 0,
                                       s, vnull, perm, nr, pvnull);
                hipLaunchKernelGGL(k_aggp_bucket_agg, dim3(nb), dim3(256), 0,
                                   s, pkeys, pvals, vnull ? pvnull : nullptr,
                                   offs, cnts, tab, cap);
            }
        }
        hipLaunchKernelGGL(k_aggp_specials, dim3(grid_for(n, 256)), dim3(256),
                           0, s, keys, knull, vals, vnull, n, nullgrp);
    } else if (smalltab) {
        /* low-cardinality (exact-sampled): try an estimator-sized table —
         * the full cap-sized init + compact scan cost ~12 ms of the
         * 4-group case's 17 ms. The rare-key tail the sample missed can
         * overflow it: bounded probes set an abort flag and the call
         * redoes against the full table. */
        static unsigned int *d_ab = nullptr;
        static unsigned int *h_ab = nullptr;
        if (!d_ab) {
            SCR_ALLOC_DEV(d_ab, 4);
            SCR_ALLOC_HOST(h_ab, 4);
        }
        int64_t cap_s = next_pow2_host(est * 64 < 4096 ? 4096 : est * 64);
        if (cap_s > cap) cap_s = cap;
        HIP_CHECK(hipMemsetAsync(d_ab, 0, 4, s));
        hipLaunchKernelGGL(k_agg_init, dim3(grid_for(cap_s, 256)),
                           dim3(256), 0, s, tab, cap_s);
        /* nullgrp sits at tab+cap (FULL cap), outside the small init */
        HIP_CHECK(hipMemsetAsync(nullgrp, 0, 2 * sizeof(agg_slot), s));
        hipLaunchKernelGGL(k_agg_build<true>, dim3(grid_for(n, 256)),
                           dim3(256), 0, s, keys, knull, vals, vnull, n, tab,
                           cap_s, nullgrp, d_ab);
        HIP_CHECK(hipMemcpyAsync(h_ab, d_ab, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (*h_ab == 0) {
            cap = cap_s; /* compact scans only the small table */
        } else {
            hipLaunchKernelGGL(k_agg_init, dim3(grid_for(cap + 2, 256)),
                               dim3(256), 0, s, tab, cap + 2);
            hipLaunchKernelGGL(k_agg_build<false>, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, keys, knull, vals, vnull, n,
                               tab, cap, nullgrp, (unsigned int *)nullptr);
        }
    } else {
        hipLaunchKernelGGL(k_agg_build<false>, dim3(grid_for(n, 256)),
                           dim3(256), 0, s, keys, knull, vals, vnull, n, tab,
                           cap, nullgrp, (unsigned int *)nullptr);
    }
    if (compact_tab)
        hipLaunchKernelGGL(k_agg_compact, dim3(grid_for(cap, 256)), dim3(256),
                           0, s, tab, cap, nullgrp, out, ngroups_dev);
    else
        hipLaunchKernelGGL(k_agg_emit_specials, dim3(1), dim3(64), 0, s,
                           nullgrp, out, ngroups_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_agg_i64(const int64_t *keys, const uint8_t *knull,
                         const double *vals, const uint8_t *vnull, int64_t n,
                         void *ws, size_t ws_bytes, otbx_agg_group *out,
                         int64_t *ngroups_dev, void *stream)
{
    return agg_i64_run(keys, knull, vals, vnull, n, ws, ws_bytes, out,
                       ngroups_dev, stream, nullptr);
}

} /* extern "C" */

/* ============ variance aggregate (otbx_agg_i64_var) ============
 * The full float8_accum state [N, Sx, Sxx] (float.c:2823). Sxx has no
 * accurate additive one-pass form (sum(x^2) - Sx^2/N cancels: 4e-4 relative
 * at mean 1e6 / stddev 1), so this is two passes over the input:
 *   pass 1  otbx_agg_i64, unchanged, into a scratch group array -> N, Sx
 *   index   key -> {mean = Sx/N, acc} open-addressing table over the
 *           COMPACTED groups (sized from ngroups, not n), staged in the
 *           then-dead pass-1 table region; NULL-key and AGG_EMPTY-key
 *           groups get the two dedicated slots after it (as nullgrp[0..1])
 *   pass 2  per row d = x - mean(group); accumulate sum(d^2) and sum(d):
 *           bucket-resident over pass 1's partitioned records when the
 *           direct path ran (k_var_bucket_pass2), else streamed with
 *           pre-aggregation in a per-block LDS table keyed by slot index
 *           (k_var_pass2, the k_agg_build recipe: hot keys never reach
 *           global atomics)
 *   final   Sxx = sum(d^2) - sum(d)^2/N   (corrected two-pass: the second
 *           term removes the rounding error of the mean), clamped at 0.
 * Inf/NaN inputs make mean, d and both sums non-finite, and Inf - Inf = NaN
 * lands Sxx on NaN as float8_accum does. A one-row group has d == 0
 * exactly. */
struct var_slot {
    long long key;
    double mean;
    double sd2; /* sum(d^2) */
    double sd;  /* sum(d)   */
};

#define VAR_LDS_SLOTS 512
#define VAR_LDS_PROBES 4

struct var_lds_slot {
    long long si; /* index slot; -1 = empty */
    double sd2, sd;
};

__global__ __launch_bounds__(256) void k_var_init(var_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride) {
        tab[i].key = AGG_EMPTY;
        tab[i].mean = 0.0;
        tab[i].sd2 = 0.0;
        tab[i].sd = 0.0;
    }
}

/* insert the compacted pass-1 groups (unique keys: one writer per slot) */
__global__ __launch_bounds__(256) void
k_var_index(const otbx_agg_group *__restrict__ g, int64_t ng, var_slot *tab,
            int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ng;
         i += stride) {
        double mean =
            g[i].count_v > 0 ? g[i].sum_v / (double)g[i].count_v : 0.0;
        int64_t k = g[i].key;
        if (g[i].key_isnull) {
            tab[cap].mean = mean;
            continue;
        }
        if (k == AGG_EMPTY) {
            tab[cap + 1].mean = mean;
            continue;
        }
        int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
        for (int64_t t = 0; t <= mask; t++) {
            long long old = atomicCAS((unsigned long long *)&tab[s].key,
                                      (unsigned long long)AGG_EMPTY,
                                      (unsigned long long)k);
            if (old == AGG_EMPTY) {
                tab[s].mean = mean;
                break;
            }
            s = (s + 1) & mask;
        }
    }
}

/* read-only lookup (the index was built by an earlier launch); bounded so a
 * missing key ends the probe instead of spinning */
__device__ __forceinline__ int64_t d_var_find(const var_slot *tab,
                                              int64_t mask, int64_t k)
{
    int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
    for (int64_t t = 0; t <= mask; t++) {
        long long kk = tab[s].key;
        if (kk == k) return s;
        if (kk == AGG_EMPTY) return -1;
        s = (s + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(256) void
k_var_pass2(const int64_t *__restrict__ keys,
            const uint8_t *__restrict__ knull,
            const double *__restrict__ vals,
            const uint8_t *__restrict__ vnull, int64_t n, var_slot *tab,
            int64_t cap, bool specials_only)
{
    __shared__ var_lds_slot ltab[VAR_LDS_SLOTS];
    for (int s = threadIdx.x; s < VAR_LDS_SLOTS; s += blockDim.x) {
        ltab[s].si = -1;
        ltab[s].sd2 = 0.0;
        ltab[s].sd = 0.0;
    }
    __syncthreads();
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (vnull && vnull[i]) continue; /* strict transfn skips NULL */
        int64_t k = keys[i];
        bool kn = knull && knull[i];
        /* the bucket pass covers ordinary keys; this launch then only
         * sweeps up the two dedicated groups */
        if (specials_only && !kn && k != AGG_EMPTY) continue;
        int64_t si = kn                ? cap
                     : k == AGG_EMPTY ? cap + 1
                                      : d_var_find(tab, mask, k);
        if (si < 0) continue; /* unreachable: pass 1 saw every key */
        double d = vals[i] - tab[si].mean;
        double d2 = d * d;
        int s = (int)(d_hash_i64(si) & (uint64_t)(VAR_LDS_SLOTS - 1));
        bool placed = false;
        for (int t = 0; t < VAR_LDS_PROBES; t++) {
            long long old = atomicCAS((unsigned long long *)&ltab[s].si,
                                      (unsigned long long)-1ll,
                                      (unsigned long long)si);
            if (old == -1ll || old == si) {
                atomicAdd(&ltab[s].sd2, d2);
                atomicAdd(&ltab[s].sd, d);
                placed = true;
                break;
            }
            s = (s + 1) & (VAR_LDS_SLOTS - 1);
        }
        if (!placed) { /* LDS window full: spill straight to global */
            atomicAdd(&tab[si].sd2, d2);
            atomicAdd(&tab[si].sd, d);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < VAR_LDS_SLOTS; s += blockDim.x) {
        long long si = ltab[s].si;
        if (si >= 0) {
            atomicAdd(&tab[si].sd2, ltab[s].sd2);
            atomicAdd(&tab[si].sd, ltab[s].sd);
        }
    }
}

/* bucket-resident pass 2 over the records the partitioned direct path of
 * pass 1 left in the workspace. Buckets hold DISJOINT key sets and fit one
 * LDS table (k_aggp_bucket_agg_kv_direct's sizing and probe sequence), so
 * the per-row work never leaves LDS: scattered global f64 atomics run at
 * ~22 G/s chip-wide, which bound the generic pass at 11 Grows/s.
 *   A  insert the bucket's keys into the LDS table
 *   B  one index lookup per DISTINCT key -> mean
 *   C  second sweep of the records: d = v - mean into LDS sum(d^2), sum(d)
 *   D  one global add per distinct key
 * A bucket that pass 1 flagged, or whose table overflows here, takes the
 * generic per-row route for its own rows. */
#define VARB_LSLOTS 1024

struct varb_lds_slot {
    long long key;
    double mean, sd2, sd;
};

__device__ __forceinline__ void d_var_row_global(var_slot *tab, int64_t mask,
                                                 int64_t k, double v)
{
    int64_t si = d_var_find(tab, mask, k);
    if (si < 0) return;
    double d = v - tab[si].mean;
    atomicAdd(&tab[si].sd2, d * d);
    atomicAdd(&tab[si].sd, d);
}

__global__ __launch_bounds__(256) void
k_var_bucket_pass2(const ulonglong2 *__restrict__ recs,
                   const unsigned long long *__restrict__ offs,
                   const unsigned long long *__restrict__ cnts,
                   const uint8_t *__restrict__ flags, var_slot *tab,
                   int64_t cap)
{
    __shared__ varb_lds_slot ltab[VARB_LSLOTS];
    __shared__ int bfail;
    int64_t mask = cap - 1;
    int64_t lo = (int64_t)offs[blockIdx.x];
    int64_t hi = lo + (int64_t)cnts[blockIdx.x];
    if (threadIdx.x == 0) bfail = flags[blockIdx.x] ? 1 : 0;
    for (int t = threadIdx.x; t < VARB_LSLOTS; t += blockDim.x) {
        ltab[t].key = AGG_EMPTY;
        ltab[t].mean = 0.0;
        ltab[t].sd2 = 0.0;
        ltab[t].sd = 0.0;
    }
    __syncthreads();
    if (!bfail) { /* A (block-uniform: bfail was read after the barrier) */
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            int64_t k = (int64_t)recs[i].x;
            if (k == AGG_EMPTY) continue; /* dedicated slot: specials sweep */
            uint64_t h = d_hash_i64(k);
            int t0 = (int)(h & (uint64_t)(VARB_LSLOTS - 1));
            int step = (int)(((h >> 52) & (uint64_t)(VARB_LSLOTS - 2)) | 1ull);
            bool placed = false;
            for (int t = 0; t < 64; t++) {
                long long old = atomicCAS((unsigned long long *)&ltab[t0].key,
                                          (unsigned long long)AGG_EMPTY,
                                          (unsigned long long)k);
                if (old == AGG_EMPTY || old == k) {
                    placed = true;
                    break;
                }
                t0 = (t0 + step) & (VARB_LSLOTS - 1);
            }
            if (!placed) bfail = 1; /* any-lane plain store, read after the
                                     * barrier */
        }
    }
    __syncthreads();
    if (bfail) { /* generic route for this bucket's rows */
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            ulonglong2 r = recs[i];
            if ((int64_t)r.x == AGG_EMPTY) continue;
            d_var_row_global(tab, mask, (int64_t)r.x,
                             __longlong_as_double((long long)r.y));
        }
        return;
    }
    /* B: each thread owns the same LDS slots here and in D (256 threads:
     * the launch and __launch_bounds__ agree), so the index slot stays in
     * a register instead of being looked up twice */
    int64_t sis[VARB_LSLOTS / 256];
#pragma unroll
    for (int j = 0; j < VARB_LSLOTS / 256; j++) {
        int t = (int)threadIdx.x + j * 256;
        long long k = ltab[t].key;
        sis[j] = k == AGG_EMPTY ? -1 : d_var_find(tab, mask, k);
        if (sis[j] >= 0) ltab[t].mean = tab[sis[j]].mean;
    }
    __syncthreads();
    /* C: every key of the bucket is in the table, so the probe ends */
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        ulonglong2 r = recs[i];
        int64_t k = (int64_t)r.x;
        if (k == AGG_EMPTY) continue;
        uint64_t h = d_hash_i64(k);
        int t0 = (int)(h & (uint64_t)(VARB_LSLOTS - 1));
        int step = (int)(((h >> 52) & (uint64_t)(VARB_LSLOTS - 2)) | 1ull);
        for (int t = 0; t < 64 && ltab[t0].key != k; t++)
            t0 = (t0 + step) & (VARB_LSLOTS - 1);
        if (ltab[t0].key != k) continue; /* unreachable */
        double d = __longlong_as_double((long long)r.y) - ltab[t0].mean;
        atomicAdd(&ltab[t0].sd2, d * d);
        atomicAdd(&ltab[t0].sd, d);
    }
    __syncthreads();
    /* D */
#pragma unroll
    for (int j = 0; j < VARB_LSLOTS / 256; j++) {
        int t = (int)threadIdx.x + j * 256;
        if (sis[j] < 0) continue;
        atomicAdd(&tab[sis[j]].sd2, ltab[t].sd2);
        atomicAdd(&tab[sis[j]].sd, ltab[t].sd);
    }
}

__global__ __launch_bounds__(256) void
k_var_finalize(const otbx_agg_group *__restrict__ g, int64_t ng,
               const var_slot *__restrict__ tab, int64_t cap,
               otbx_var_group *__restrict__ out)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ng;
         i += stride) {
        otbx_agg_group gi = g[i];
        double sxx = 0.0;
        if (gi.count_v > 0) {
            int64_t si = gi.key_isnull          ? cap
                         : gi.key == AGG_EMPTY ? cap + 1
                                               : d_var_find(tab, mask, gi.key);
            if (si < 0) {
                sxx = __longlong_as_double(0x7ff8000000000000ll);
            } else {
                double sd2 = tab[si].sd2, sd = tab[si].sd;
                sxx = sd2 - sd * sd / (double)gi.count_v;
                if (sxx < 0.0) sxx = 0.0; /* rounding residue */
                /* float8_accum never leaves Sxx infinite (float.c:2855) */
                if (isinf(sxx)) sxx = __longlong_as_double(0x7ff8000000000000ll);
            }
        }
        out[i].key = gi.key;
        out[i].count_star = gi.count_star;
        out[i].count_v = gi.count_v;
        out[i].sum_v = gi.sum_v;
        out[i].sxx = sxx;
        out[i].key_isnull = gi.key_isnull;
        out[i].sum_isnull = gi.sum_isnull;
    }
}

static_assert(sizeof(otbx_var_group) == 48, "otbx_var_group ABI");
static_assert(sizeof(var_slot) == sizeof(agg_slot),
              "the index reuses the pass-1 table region slot for slot");

extern "C" {

otbx_status otbx_agg_i64_var_workspace_bytes(int64_t n, size_t *bytes)
{
    size_t a;
    otbx_agg_i64_workspace_bytes(n, &a);
    a = (a + 255) & ~(size_t)255;
    /* + the pass-1 scratch groups (capacity n, as groups_dev) */
    *bytes = a + (size_t)(n < 1 ? 1 : n) * sizeof(otbx_agg_group);
    return OTBX_OK;
}

otbx_status otbx_agg_i64_var(const int64_t *keys, const uint8_t *knull,
                             const double *vals, const uint8_t *vnull,
                             int64_t n, void *ws, size_t ws_bytes,
                             otbx_var_group *out, int64_t *ngroups_dev,
                             void *stream)
{
    size_t need, a;
    otbx_agg_i64_var_workspace_bytes(n, &need);
    if (ws_bytes < need) return OTBX_ERR_INVALID;
    otbx_agg_i64_workspace_bytes(n, &a);
    hipStream_t s = (hipStream_t)stream;
    otbx_agg_group *g1 =
        (otbx_agg_group *)((char *)ws + ((a + 255) & ~(size_t)255));
    /* pass 1: every existing path (LDS two-level, small table + redo,
     * partitioned direct, NULL-carrying gather) -> count(*), N, Sx */
    agg_part_layout lay = {};
    otbx_status st = agg_i64_run(keys, knull, vals, vnull, n, ws, a, g1,
                                 ngroups_dev, stream, &lay);
    if (st != OTBX_OK || n == 0) return st;

    static int64_t *h_ng = nullptr;
    if (!h_ng) SCR_ALLOC_HOST(h_ng, 8);
    HIP_CHECK(hipMemcpyAsync(h_ng, ngroups_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t ng = *h_ng;
    if (ng <= 0) return OTBX_OK;
    if (ng > n) return OTBX_ERR_INVALID; /* cannot happen: capacity is n */

    /* the pass-1 table region is dead now; ng <= n keeps the index inside
     * it: (cap + 2) slots of the same 32 B */
    int64_t cap = next_pow2_host(ng < 16 ? 16 : (int64_t)(ng / 0.7) + 1);
    var_slot *tab = (var_slot *)ws;
    hipLaunchKernelGGL(k_var_init, dim3(grid_for(cap + 2, 256)), dim3(256), 0,
                       s, tab, cap + 2);
    hipLaunchKernelGGL(k_var_index, dim3(grid_for(ng, 256)), dim3(256), 0, s,
                       g1, ng, tab, cap);
    /* the partition records sit past the pass-1 table region, which the
     * index (cap <= pass-1 cap) never leaves */
    if (lay.nbuckets)
        hipLaunchKernelGGL(k_var_bucket_pass2, dim3(lay.nbuckets), dim3(256),
                           0, s, lay.recs, lay.offs, lay.cnts, lay.flags, tab,
                           cap);
    hipLaunchKernelGGL(k_var_pass2, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       keys, knull, vals, vnull, n, tab, cap,
                       lay.nbuckets != 0);
    hipLaunchKernelGGL(k_var_finalize, dim3(grid_for(ng, 256)), dim3(256), 0,
                       s, g1, ng, tab, cap, out);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ================= Q9-mix DN fragment (config 5) ================= */

__global__ void k_minmax_i64(const int64_t *__restrict__ keys, int64_t n,
                             unsigned long long *minkey,
                             unsigned long long *maxkey)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long mymin = ~0ull >> 1, mymax = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        unsigned long long k = (unsigned long long)keys[i];
        if (k < mymin) mymin = k;
        if (k > mymax) mymax = k;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        unsigned long long mn = (unsigned long long)__shfl_down(
            (long long)mymin, off, WAVE);
        unsigned long long mx = (unsigned long long)__shfl_down(
            (long long)mymax, off, WAVE);
        if (mn < mymin) mymin = mn;
        if (mx > mymax) mymax = mx;
    }
    if ((threadIdx.x % WAVE) == 0) {
        if (mymin != (~0ull >> 1)) atomicMin(minkey, mymin);
        if (mymax) atomicMax(maxkey, mymax);
    }
}

/* part bitmap for partkey slice [lo, hi): dense p_partkey 1..nparts, bit
 * (idx - lo) set where p_type % typemod == typeval (the p_name LIKE filter
 * restatement). Sliced so the bitmap stays inside a per-XCD L2: at SF300
 * a full 7.5 MB bitmap spilled to HBM and the gather rate collapsed
 * (DESIGN.md §7 SF300 table). */
__global__ void k_q9_part_bitmap(const otbx_part_dev p, uint8_t typemod,
                                 uint8_t typeval, int64_t lo, int64_t hi,
                                 unsigned long long *bitmap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p.n;
         i += stride) {
        if (p.p_type[i] % typemod == typeval) {
            int64_t idx = p.p_partkey[i] - 1;
            if (idx >= lo && idx < hi)
                atomicOr(&bitmap[(idx - lo) >> 6], 1ull << ((idx - lo) & 63));
        }
    }
}

/* orders date lookup: direct-addressed by (o_orderkey - mino); orderkeys are
 * dense per shard so the table is the merge of local rows (the same
 * dense-direct reasoning as Q3 — DESIGN.md §3). Entries hold the date
 * XOR OTBX_Q9_DATE_ABSENT (otbx.h): the memset(0) word that no order wrote
 * then decodes to that one reserved date value, and day 0 is an ordinary
 * date. */
__global__ void k_q9_odate_build(const otbx_orders_dev o, int64_t mino,
                                 int32_t *dtab)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (o.o_orderkey32) { /* compact-key cache: 12 -> 8 B/row stream */
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
             i < o.n; i += stride)
            dtab[(int64_t)o.o_orderkey32[i] - mino] =
                o.o_orderdate[i] ^ OTBX_Q9_DATE_ABSENT;
    } else {
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
             i < o.n; i += stride)
            dtab[o.o_orderkey[i] - mino] =
                o.o_orderdate[i] ^ OTBX_Q9_DATE_ABSENT;
    }
}

/* Q9 probe, split in two phases. The single fused kernel measured as the
 * SUM of its component costs with no overlap (request-bound;
 * profiles/r01_q9mix_microbench.txt), so splitting is free — and phase 1
 * then streams only l_partkey (8 B/row), while phase 2 runs dense over the
 * ~6% survivors.
 *
 * phase 1: part-bitmap semi-join over the l_partkey stream; wave-aggregated
 * append (Guideline 12) of surviving row ids (u32 — otbx_q9_partial guards
 * n < 2^32). */
__global__ void k_q9_filter(const int64_t *__restrict__ pk, int64_t n,
                            const unsigned long long *__restrict__ pbitmap,
                            int64_t lo, int64_t hi,
                            uint32_t *__restrict__ hits, int64_t *nhits)
{
    /* LDS-staged per-wave append, one global reservation per ~BUF rows —
     * a bare wave_append here would make ~n/64 single-counter reservations,
     * which caps at ~88/µs (the measured law behind every append kernel in
     * this file; a first cut of this kernel measured 107 ms at SF100 for
     * exactly that reason). */
    const int BUF = 4096; /* A/B: 1024 → 2048 −0.49 ms/step, → 4096 −0.51;
                           * 64 KB LDS (1 block/CU) measured no occupancy
                           * penalty on this stream+gather kernel */
    __shared__ uint32_t buf[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0;
    int64_t nq = n / 4;
    const v2l *pk2 = (const v2l *)pk;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         q += stride) {
        bool m[4] = {false, false, false, false};
        int64_t r0 = q * 4;
        int mycnt = 0;
        if (q < nq) {
            /* non-temporal: the single-use pk stream must not evict the
             * L2-resident slice bitmap it races against */
            v2l pa = __builtin_nontemporal_load(&pk2[2 * q]);
            v2l pb = __builtin_nontemporal_load(&pk2[2 * q + 1]);
            int64_t pks[4] = {pa.x, pa.y, pb.x, pb.y};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int64_t pidx = pks[j] - 1 - lo;
                m[j] = pidx >= 0 && pidx < hi - lo &&
                       ((pbitmap[pidx >> 6] >> (pidx & 63)) & 1ull);
                mycnt += m[j];
            }
        } else if (q == nq) { /* tail rows (n % 4) */
            for (int64_t i = nq * 4; i < n; i++) {
                int j = (int)(i - nq * 4);
                int64_t pidx = pk[i] - 1 - lo;
                m[j] = pidx >= 0 && pidx < hi - lo &&
                       ((pbitmap[pidx >> 6] >> (pidx & 63)) & 1ull);
                mycnt += m[j];
            }
        }
        int incl = mycnt;
        for (int off = 1; off < WAVE; off <<= 1) {
            int up = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += up;
        }
        int tot = __shfl(incl, WAVE - 1, WAVE);
        if (tot) {
            if (nbuf + tot > BUF) {
                long long bpos = 0;
                if (lane == 0)
                    bpos = (long long)atomicAdd((unsigned long long *)nhits,
                                                (unsigned long long)nbuf);
                bpos = __shfl(bpos, 0, WAVE);
                for (int j = lane; j < nbuf; j += WAVE)
                    hits[bpos + j] = buf[wid][j];
                nbuf = 0;
            }
            int pos = nbuf + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j])
                    buf[wid][pos++] = (uint32_t)(r0 + j);
            nbuf += tot;
        }
        if (__all(q >= nq))
            break;
    }
    if (nbuf) {
        long long bpos = 0;
        if (lane == 0)
            bpos = (long long)atomicAdd((unsigned long long *)nhits,
                                        (unsigned long long)nbuf);
        bpos = __shfl(bpos, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE)
            hits[bpos + j] = buf[wid][j];
    }
}

/* phase 1 (tile variant, default): tile-staged compaction — the append_ab
 * v6 pattern (profiles/r2_append_ab.txt: 0.22 vs 0.94 ms for the per-wave
 * staged appender at 150 M rows). Per 8192-row tile: wave prefix sums →
 * 16 wave totals scanned by thread 0 → stable ranks into an LDS stage →
 * ONE cursor reservation per tile → linear write-out with consecutive
 * lanes on consecutive addresses (the per-wave appender's run-strided
 * writes, not its atomics, were the plateau). Survivor ids stay ascending
 * within a tile; tiles land in arbitrary order (result-set parity only —
 * the probe pass is order-free). */
#define Q9T 8192
template <bool K32>
__global__ __launch_bounds__(1024) void k_q9_filter_tile(
    const int64_t *__restrict__ pk, const int32_t *__restrict__ pk32,
    int64_t n, const unsigned long long *__restrict__ pbitmap, int64_t lo_k,
    int64_t hi_k, uint32_t *__restrict__ hits, int64_t *nhits)
{
    __shared__ uint32_t stage[Q9T];
    __shared__ int wtot[16];
    __shared__ int woff[16];
    __shared__ int sweepbase;
    __shared__ long long gbase;
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    const v2l *pk2 = (const v2l *)pk;
    int64_t ntiles = (n + Q9T - 1) / Q9T;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t tl = t * (int64_t)Q9T;
        int64_t th = tl + Q9T < n ? tl + Q9T : n;
        if (threadIdx.x == 0) sweepbase = 0;
        __syncthreads();
        for (int64_t s0 = tl; s0 < th; s0 += 4096) {
            int64_t r0 = s0 + 4 * (int64_t)threadIdx.x;
            bool m[4] = {false, false, false, false};
            int mycnt = 0;
            if (r0 + 3 < n) {
                int64_t pks[4];
                if (K32) { /* staged compact-key cache: 4 B/row stream */
                    v4i pp = __builtin_nontemporal_load(
                        (const v4i *)&pk32[r0]);
                    pks[0] = pp.x; pks[1] = pp.y;
                    pks[2] = pp.z; pks[3] = pp.w;
                } else {
                    v2l pa = __builtin_nontemporal_load(&pk2[r0 / 2]);
                    v2l pb = __builtin_nontemporal_load(&pk2[r0 / 2 + 1]);
                    pks[0] = pa.x; pks[1] = pa.y;
                    pks[2] = pb.x; pks[3] = pb.y;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int64_t pidx = pks[j] - 1 - lo_k;
                    m[j] = pidx >= 0 && pidx < hi_k - lo_k &&
                           ((pbitmap[pidx >> 6] >> (pidx & 63)) & 1ull);
                    mycnt += m[j];
                }
            } else {
                for (int j = 0; j < 4 && r0 + j < n; j++) {
                    int64_t pidx = pk[r0 + j] - 1 - lo_k;
                    m[j] = pidx >= 0 && pidx < hi_k - lo_k &&
                           ((pbitmap[pidx >> 6] >> (pidx & 63)) & 1ull);
                    mycnt += m[j];
                }
            }
            int incl = mycnt;
            for (int off = 1; off < WAVE; off <<= 1) {
                int up = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl += up;
            }
            if (lane == WAVE - 1) wtot[wid] = incl;
            __syncthreads();
            if (threadIdx.x == 0) {
                int acc = sweepbase;
                for (int w = 0; w < 16; w++) {
                    woff[w] = acc;
                    acc += wtot[w];
                }
                sweepbase = acc;
            }
            __syncthreads();
            int pos = woff[wid] + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j]) stage[pos++] = (uint32_t)(r0 + j);
            __syncthreads();
        }
        int tot = sweepbase;
        if (threadIdx.x == 0)
            gbase = tot ? (long long)atomicAdd((unsigned long long *)nhits,
                                               (unsigned long long)tot)
                        : 0;
        __syncthreads();
        for (int p = threadIdx.x; p < tot; p += blockDim.x)
            hits[gbase + p] = stage[p];
        __syncthreads();
    }
}

/* Q9 probe-side AoS record (otbx.h q9rec): one 32-B record per lineitem
 * row so a survivor's gather touches one cache line instead of three
 * column lines (l_orderkey / l_extendedprice / l_discount). Built once at
 * staging. */
struct q9_rec {
    long long okey;
    double price;
    double disc;
    long long pad;
};

__global__ void k_q9_build_recs(const otbx_lineitem_dev l,
                                q9_rec *__restrict__ r)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < l.n;
         i += stride) {
        q9_rec x;
        x.okey = l.l_orderkey[i];
        x.price = l.l_extendedprice[i];
        x.disc = l.l_discount[i];
        x.pad = 0;
        r[i] = x;
    }
}

/* phase 2: dense pass over the survivors — orders date lookup + year
 * partial aggregate in per-lane registers (the Q1 pattern: 7-year domain,
 * compile-time indexed), wave+block reduce, one atomic per (year, block). */
__global__ void k_q9_probe(const otbx_lineitem_dev l,
                           const uint32_t *__restrict__ hits,
                           const int64_t *__restrict__ nhits_p,
                           const int32_t *__restrict__ dtab, int64_t mino,
                           int64_t orange, double *__restrict__ out_sums,
                           unsigned long long *__restrict__ out_counts)
{
    double acc[7];
    uint32_t cnt[7];
#pragma unroll
    for (int y = 0; y < 7; y++) {
        acc[y] = 0.0;
        cnt[y] = 0;
    }
    int64_t nh = *nhits_p;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t h = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; h < nh;
         h += stride) {
        int64_t i = (int64_t)hits[h];
        const q9_rec *recs = (const q9_rec *)l.q9rec;
        int64_t okey;
        double price, disc;
        if (recs) { /* staged record cache: one line per survivor */
            q9_rec rc = recs[i];
            okey = rc.okey;
            price = rc.price;
            disc = rc.disc;
        } else {
            okey = l.l_orderkey[i];
            price = l.l_extendedprice[i];
            disc = l.l_discount[i];
        }
        int64_t oidx = okey - mino;
        if (oidx < 0 || oidx >= orange)
            continue;
        int32_t date = dtab[oidx] ^ OTBX_Q9_DATE_ABSENT;
        if (date == OTBX_Q9_DATE_ABSENT)
            continue; /* the memset(0) word: no such order */
        int32_t y = otbx_year_of_day(date);
        double rev = price * (1.0 - disc);
#pragma unroll
        for (int yy = 0; yy < 7; yy++) {
            bool hit = yy == y;
            acc[yy] += hit ? rev : 0.0;
            cnt[yy] += hit;
        }
    }
    /* wave + block reduction, one atomic per (year) per block */
#pragma unroll
    for (int y = 0; y < 7; y++) {
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            acc[y] += __shfl_down(acc[y], off, WAVE);
            cnt[y] += __shfl_down(cnt[y], off, WAVE);
        }
    }
    __shared__ double lacc[256 / WAVE][7];
    __shared__ uint32_t lcnt[256 / WAVE][7];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    if (lane == 0) {
#pragma unroll
        for (int y = 0; y < 7; y++) {
            lacc[wid][y] = acc[y];
            lcnt[wid][y] = cnt[y];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nw = (int)(blockDim.x / WAVE);
#pragma unroll
        for (int y = 0; y < 7; y++) {
            double v = 0;
            unsigned long long c = 0;
            for (int w = 0; w < nw; w++) {
                v += lacc[w][y];
                c += lcnt[w][y];
            }
            if (v != 0.0) atomicAdd(&out_sums[y], v);
            if (c) atomicAdd(&out_counts[y], c);
        }
    }
}

extern "C" {

static inline size_t align64_sz(size_t x) { return (x + 63) / 64 * 64; }

/* Part-bitmap slice width in bits. Measured on MI355X: at
 * SF300 a 3 MB L2-resident slice in 3 passes LOST to the single-pass
 * 7.5 MB bitmap (27.95 vs 23.54 ms/step) — re-streaming 14.4 GB of
 * l_partkey per extra pass costs more than the partially-spilled gathers
 * it avoids. So the default cap is 1 Gbit (128 MB bitmap, ~17× SF300's
 * part table): slicing only engages for part tables far beyond benchmark
 * sizes, where the workspace itself would balloon. OTBX_Q9_BITMAP_BITS
 * overrides (tests force multipass with tiny values). */
static inline int64_t q9_slice_bits(void)
{
    int64_t cap_bits = 1ll << 30;
    const char *cb = getenv("OTBX_Q9_BITMAP_BITS");
    if (cb) {
        int64_t e = atoll(cb);
        if (e >= 64) cap_bits = e;
    }
    return cap_bits;
}

otbx_status otbx_q9_workspace_bytes(int64_t nparts, int64_t norders,
                                    int64_t nlineitem, uint32_t nranks,
                                    size_t *bytes)
{
    int64_t orange = norders * (int64_t)(nranks ? nranks : 1);
    int64_t cap = q9_slice_bits();
    int64_t slice = nparts < cap ? nparts : cap;
    *bytes = align64_sz(8 * (size_t)((slice + 63) / 64)) /* part bitmap */ +
             align64_sz((size_t)orange * 4) /* odate direct table */ +
             64 /* hit counter */ +
             (size_t)(nlineitem > 0 ? nlineitem : 1) * 4 /* hit row ids */;
    return OTBX_OK;
}

otbx_status otbx_q9_partial(const otbx_part_dev *p, const otbx_orders_dev *o,
                            const otbx_lineitem_dev *l, uint8_t typemod,
                            uint8_t typeval, void *ws, size_t ws_bytes,
                            double *sums_dev, int64_t *counts_dev,
                            void *stream, float *kernel_ms)
{
    if (!p || !o || !l || typemod == 0)
        return OTBX_ERR_INVALID;
    if (l->n > 0 && (!l->l_partkey || !l->l_orderkey))
        return OTBX_ERR_INVALID; /* an empty table may carry no columns */
    if (l->n >= (int64_t)UINT32_MAX)
        return OTBX_ERR_INVALID;  /* u32 hit row ids; shard larger tables */
    hipStream_t s = (hipStream_t)stream;
    /* orderkey range from a minmax kernel (layout-agnostic; the dense shard
     * layout makes the direct odate table the size of the global orders
     * table). Running the two small build kernels CONCURRENTLY with the
     * filter on a second stream was measured neutral (6.33 → 6.46 ms step):
     * on this request-bound pipeline concurrent kernels just split the same
     * resource — so everything stays on the caller's stream. */
    static int64_t *h_mm = nullptr;
    static unsigned long long *d_mm = nullptr;
    if (!h_mm) {
        SCR_ALLOC_HOST(h_mm, 16);
        SCR_ALLOC_DEV(d_mm, 16);
    }
    int64_t mino, orange;
    if (o->n == 0) {
        mino = 1;
        orange = 1;
    } else if (o->has_minmax) { /* staged zone-map metadata */
        mino = o->okey_min;
        orange = key_range(o->okey_min, o->okey_max);
    } else {
        HIP_CHECK(hipMemsetAsync(d_mm, 0x7f, 8, s));
        HIP_CHECK(hipMemsetAsync(d_mm + 1, 0, 8, s));
        hipLaunchKernelGGL(k_minmax_i64, dim3(grid_for(o->n, 256)), dim3(256),
                           0, s, o->o_orderkey, o->n, d_mm, d_mm + 1);
        HIP_CHECK(hipMemcpyAsync(h_mm, d_mm, 16, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        mino = h_mm[0];
        orange = key_range(h_mm[0], h_mm[1]);
    }
    /* Grace-style partkey slices: each pass rebuilds the bitmap for one
     * key range, re-streams l_partkey, and gathers only rows whose key
     * falls in the slice (each row gathers in exactly one pass). With the
     * default 1 Gbit cap (see q9_slice_bits) this is single-pass for any
     * realistic part table; slicing engages only for huge key domains or
     * under the OTBX_Q9_BITMAP_BITS test hook. */
    int64_t cap_bits = q9_slice_bits();
    int64_t slice = p->n < cap_bits ? p->n : cap_bits;
    if (slice < 1) slice = 1; /* empty part table: one no-match pass */
    int64_t npasses = (p->n + slice - 1) / slice;
    if (npasses < 1) npasses = 1;
    size_t bm_bytes = align64_sz(8 * (size_t)((slice + 63) / 64));
    /* a range the workspace cannot hold (sparse keys, or keys outside the
     * documented domain that the unsigned minmax misreads) is refused here,
     * before any kernel indexes the date table */
    if (orange <= 0 || (uint64_t)orange > ws_bytes / 4)
        return OTBX_ERR_INVALID;
    size_t dt_bytes = align64_sz((size_t)orange * 4);
    size_t need = bm_bytes + dt_bytes + 64 +
                  (size_t)(l->n > 0 ? l->n : 1) * 4;
    if (ws_bytes < need) return OTBX_ERR_INVALID;
    unsigned long long *pbitmap = (unsigned long long *)ws;
    int32_t *dtab = (int32_t *)((char *)ws + bm_bytes);
    int64_t *nhits = (int64_t *)((char *)ws + bm_bytes + dt_bytes);
    uint32_t *hits = (uint32_t *)((char *)ws + bm_bytes + dt_bytes + 64);
    HIP_CHECK(hipMemsetAsync(sums_dev, 0, 7 * 8, s));
    HIP_CHECK(hipMemsetAsync(counts_dev, 0, 7 * 8, s));
    HIP_CHECK(hipMemsetAsync(dtab, 0, (size_t)orange * 4, s));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms) {
        HIP_CHECK(hipEventCreate(&ev0));
        HIP_CHECK(hipEventCreate(&ev1));
    }
    if (o->n > 0)
        hipLaunchKernelGGL(k_q9_odate_build, dim3(grid_for(o->n, 256)),
                           dim3(256), 0, s, *o, mino, dtab);
    bool rec0 = false;
    for (int64_t pass = 0; pass < npasses; pass++) {
        int64_t lo = pass * slice;
        int64_t hi = lo + slice < p->n ? lo + slice : p->n;
        HIP_CHECK(hipMemsetAsync(pbitmap, 0, bm_bytes, s));
        HIP_CHECK(hipMemsetAsync(nhits, 0, 8, s));
        hipLaunchKernelGGL(k_q9_part_bitmap, dim3(grid_for(p->n, 256)),
                           dim3(256), 0, s, *p, typemod, typeval, lo, hi,
                           pbitmap);
        if (kernel_ms && !rec0) {
            HIP_CHECK(hipEventRecord(ev0, s));
            rec0 = true;
        }
        const char *fw = getenv("OTBX_Q9_FILTER_WAVE");
        if (fw && atoi(fw)) /* legacy per-wave appender (A/B) */
            hipLaunchKernelGGL(k_q9_filter, dim3(grid_for(l->n / 4, 256)),
                               dim3(256), 0, s, l->l_partkey, l->n, pbitmap,
                               lo, hi, hits, nhits);
        else if (l->l_partkey32)
            hipLaunchKernelGGL((k_q9_filter_tile<true>), dim3(2048),
                               dim3(1024), 0, s, l->l_partkey,
                               l->l_partkey32, l->n, pbitmap, lo, hi, hits,
                               nhits);
        else
            hipLaunchKernelGGL((k_q9_filter_tile<false>), dim3(2048),
                               dim3(1024), 0, s, l->l_partkey, NULL, l->n,
                               pbitmap, lo, hi, hits, nhits);
        hipLaunchKernelGGL(k_q9_probe, dim3(grid_for(l->n / 8, 256)),
                           dim3(256), 0, s, *l, hits, nhits, dtab, mino,
                           orange, sums_dev, (unsigned long long *)counts_dev);
    }
    HIP_CHECK(hipGetLastError());
    if (kernel_ms) {
        HIP_CHECK(hipEventRecord(ev1, s));
        HIP_CHECK(hipEventSynchronize(ev1));
        HIP_CHECK(hipEventElapsedTime(kernel_ms, ev0, ev1));
        HIP_CHECK(hipEventDestroy(ev0));
        HIP_CHECK(hipEventDestroy(ev1));
    }
    return OTBX_OK;
}

} /* extern "C" */

/* ================= GPU ORDER BY =================
 *
 * Full ordering of Q3 group rows: ORDER BY revenue DESC, o_orderdate ASC
 * (tuplesort.c analog). Stable LSD radix sort over (key u64, idx u32) pairs,
 * 8-bit digits, two stages chained by stability:
 *   stage A: date ASC  (2 passes — precondition in otbx.h: 0 ≤ date < 2^16)
 *   stage B: ~ss_norm_f64(revenue) ASC ≡ revenue DESC (8 passes; the
 *            normalisation is order-preserving for every sign, -0 == +0)
 * Stable scatter: per-wave 8-ballot multi-split rank + per-digit wave/round
 * prefix counters in LDS — lane order preserved, so every pass is stable.
 */

#define RS_BLOCK 256
#define RS_BINS 256

__global__ void k_rs_hist(const unsigned long long *__restrict__ keys,
                          int64_t n, int shift, uint32_t *hist /* [bins][nblocks] */)
{
    __shared__ uint32_t lh[RS_BINS];
    for (int i = threadIdx.x; i < RS_BINS; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        atomicAdd(&lh[(keys[i] >> shift) & 0xff], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < RS_BINS; i += blockDim.x)
        hist[(size_t)i * gridDim.x + blockIdx.x] = lh[i];
}

/* stable scatter: block processes its chunk in rounds of 256 elements;
 * within a round, rank among equal digits = wave multi-split (8 ballots,
 * lane-ordered) + per-digit wave-offset prefix; across rounds, per-digit
 * running counters. base[digit][block] comes from the scanned histogram. */
__global__ void k_rs_scatter(const unsigned long long *__restrict__ keys,
                             const uint32_t *__restrict__ vals, int64_t n,
                             int shift,
                             const uint32_t *__restrict__ base /* [bins][nblocks] */,
                             unsigned long long *__restrict__ okeys,
                             uint32_t *__restrict__ ovals)
{
    __shared__ uint32_t run[RS_BINS];        /* per-digit running count */
    __shared__ uint32_t wcnt[4][RS_BINS];    /* per-wave per-digit counts */
    for (int i = threadIdx.x; i < RS_BINS; i += blockDim.x) run[i] = 0;
    __syncthreads();
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    for (int64_t r0 = lo; r0 < hi; r0 += blockDim.x) {
        int64_t i = r0 + threadIdx.x;
        bool valid = i < hi;
        unsigned long long k = valid ? keys[i] : 0;
        uint32_t v = valid ? vals[i] : 0;
        int digit = (int)((k >> shift) & 0xff);
        /* wave multi-split: match = lanes with my digit (8 ballots) */
        unsigned long long match = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            unsigned long long bb = __ballot((digit >> b) & 1);
            match &= ((digit >> b) & 1) ? bb : ~bb;
        }
        unsigned long long vb = __ballot(valid);
        match &= vb;
        int wrank = __popcll(match & ((1ull << lane) - 1ull));
        int wtotal = __popcll(match);
        /* per-wave digit counts (leader writes) */
        for (int i2 = threadIdx.x; i2 < 4 * RS_BINS; i2 += blockDim.x)
            ((uint32_t *)wcnt)[i2] = 0;
        __syncthreads();
        if (valid && lane == (__ffsll((long long)match) - 1))
            wcnt[wid][digit] = (uint32_t)wtotal;
        __syncthreads();
        if (valid) {
            uint32_t before = 0;
            for (int w = 0; w < wid; w++) before += wcnt[w][digit];
            int64_t pos = (int64_t)base[(size_t)digit * gridDim.x + blockIdx.x] +
                          run[digit] + before + wrank;
            okeys[pos] = k;
            ovals[pos] = v;
        }
        __syncthreads();
        /* advance running counters by this round's totals */
        for (int d = threadIdx.x; d < RS_BINS; d += blockDim.x) {
            uint32_t t = 0;
            for (int w = 0; w < 4; w++) t += wcnt[w][d];
            run[d] += t;
        }
        __syncthreads();
    }
}

/* device-side exclusive scan of the [bins][nblocks] histogram (≤ 524k
 * entries): block partials → single-block scan of partials → add back.
 * Removes the per-pass host round trip. */
#define RS_SCAN_CHUNK 1024

__global__ void k_rs_scan_partials(const uint32_t *__restrict__ in, int64_t n,
                                   uint32_t *__restrict__ sums)
{
    __shared__ uint32_t sh[256];
    int64_t lo = (int64_t)blockIdx.x * RS_SCAN_CHUNK;
    uint32_t my = 0;
    for (int i = threadIdx.x; i < RS_SCAN_CHUNK; i += blockDim.x) {
        int64_t j = lo + i;
        my += j < n ? in[j] : 0;
    }
    sh[threadIdx.x] = my;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < 256; i++) t += sh[i];
        sums[blockIdx.x] = t;
    }
}

__global__ void k_rs_scan_sums(uint32_t *sums, int64_t nb)
{
    /* single block: exclusive scan of ≤512 partials */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int64_t i = 0; i < nb; i++) {
            uint32_t c = sums[i];
            sums[i] = acc;
            acc += c;
        }
    }
}

__global__ void k_rs_scan_apply(const uint32_t *__restrict__ in, int64_t n,
                                const uint32_t *__restrict__ sums,
                                uint32_t *__restrict__ out)
{
    /* per chunk: sequential exclusive scan by thread 0 over LDS-staged
     * values (1024 adds — trivial next to the global traffic) */
    __shared__ uint32_t sh[RS_SCAN_CHUNK];
    int64_t lo = (int64_t)blockIdx.x * RS_SCAN_CHUNK;
    for (int i = threadIdx.x; i < RS_SCAN_CHUNK; i += blockDim.x) {
        int64_t j = lo + i;
        sh[i] = j < n ? in[j] : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = sums[blockIdx.x];
        for (int i = 0; i < RS_SCAN_CHUNK; i++) {
            uint32_t c = sh[i];
            sh[i] = acc;
            acc += c;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RS_SCAN_CHUNK; i += blockDim.x) {
        int64_t j = lo + i;
        if (j < n) out[j] = sh[i];
    }
}

__global__ void k_rs_key_date(const otbx_q3_group *__restrict__ g,
                              const uint32_t *__restrict__ idx, int64_t n,
                              unsigned long long *keys)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        keys[i] = (unsigned long long)(uint32_t)g[idx[i]].o_orderdate;
}

__global__ void k_rs_key_revdesc(const otbx_q3_group *__restrict__ g,
                                 const uint32_t *__restrict__ idx, int64_t n,
                                 unsigned long long *keys)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        keys[i] = ~ss_norm_f64(g[idx[i]].revenue);
}

__global__ void k_rs_iota(uint32_t *idx, int64_t n)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        idx[i] = (uint32_t)i;
}

__global__ void k_rs_apply(const otbx_q3_group *__restrict__ g,
                           const uint32_t *__restrict__ idx, int64_t n,
                           otbx_q3_group *__restrict__ out)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        out[i] = g[idx[i]];
}

extern "C" {

otbx_status otbx_order_groups_workspace_bytes(int64_t n, size_t *bytes)
{
    int64_t nb = grid_for(n, RS_BLOCK);
    *bytes = (size_t)n * (8 + 8 + 4 + 4) /* key ping-pong + idx ping-pong */ +
             (size_t)RS_BINS * nb * 4 * 2 /* hist + scanned base */ +
             4096 /* scan partial sums */ + 4096;
    return OTBX_OK;
}

/* sorts groups by (revenue DESC, o_orderdate ASC) into out_dev (may not
 * alias groups_dev). ORDER BY without LIMIT (§8f.2); ties in both keys keep
 * arbitrary (but stable-by-input) order, as SQL allows. */
otbx_status otbx_order_groups(const otbx_q3_group *groups_dev, int64_t n,
                              otbx_q3_group *out_dev, void *ws,
                              size_t ws_bytes, void *stream)
{
    if (n < 0) return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return OTBX_OK;
    int nb = grid_for(n, RS_BLOCK);
    size_t need;
    otbx_order_groups_workspace_bytes(n, &need);
    if (ws_bytes < need) return OTBX_ERR_INVALID;
    unsigned long long *kA = (unsigned long long *)ws;
    unsigned long long *kB = kA + n;
    uint32_t *iA = (uint32_t *)(kB + n);
    uint32_t *iB = iA + n;
    uint32_t *hist = iB + n;
    uint32_t *basep = hist + (size_t)RS_BINS * nb;
    uint32_t *scansums = basep + (size_t)RS_BINS * nb;
    hipLaunchKernelGGL(k_rs_iota, dim3(grid_for(n, 256)), dim3(256), 0, s, iA, n);

    /* stage A: date ASC (2 passes), stage B: ~rev bits ASC (8 passes) */
    for (int stage = 0; stage < 2; stage++) {
        int passes = stage == 0 ? 2 : 8;
        if (stage == 0)
            hipLaunchKernelGGL(k_rs_key_date, dim3(grid_for(n, 256)), dim3(256),
                               0, s, groups_dev, iA, n, kA);
        else
            hipLaunchKernelGGL(k_rs_key_revdesc, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, groups_dev, iA, n, kA);
        for (int p = 0; p < passes; p++) {
            int shift = p * 8;
            hipLaunchKernelGGL(k_rs_hist, dim3(nb), dim3(RS_BLOCK), 0, s, kA, n,
                               shift, hist);
            /* device-side exclusive scan of the [bins][nblocks] histogram */
            int64_t hn = (int64_t)RS_BINS * nb;
            int64_t snb = (hn + RS_SCAN_CHUNK - 1) / RS_SCAN_CHUNK;
            hipLaunchKernelGGL(k_rs_scan_partials, dim3((uint32_t)snb),
                               dim3(256), 0, s, hist, hn, scansums);
            hipLaunchKernelGGL(k_rs_scan_sums, dim3(1), dim3(64), 0, s,
                               scansums, snb);
            hipLaunchKernelGGL(k_rs_scan_apply, dim3((uint32_t)snb), dim3(256),
                               0, s, hist, hn, scansums, basep);
            hipLaunchKernelGGL(k_rs_scatter, dim3(nb), dim3(RS_BLOCK), 0, s, kA,
                               iA, n, shift, basep, kB, iB);
            unsigned long long *tk = kA; kA = kB; kB = tk;
            uint32_t *ti = iA; iA = iB; iB = ti;
        }
    }
    hipLaunchKernelGGL(k_rs_apply, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       groups_dev, iA, n, out_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ================= repartition exchange ================= */

/* owner = key % nranks (dense-key locator restatement of shardid→node,
 * shardmap.c:2231/1147) */
#define PART_MAX_RANKS 64

__global__ void k_part_count(const int64_t *__restrict__ keys, int64_t n,
                             uint32_t nranks, unsigned long long *counts)
{
    __shared__ unsigned int bc[PART_MAX_RANKS];
    for (int r = threadIdx.x; r < (int)nranks; r += blockDim.x) bc[r] = 0;
    __syncthreads();
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        atomicAdd(&bc[(uint32_t)(((uint64_t)keys[i]) % nranks)], 1u);
    __syncthreads();
    for (int r = threadIdx.x; r < (int)nranks; r += blockDim.x)
        if (bc[r])
            atomicAdd(&counts[r], (unsigned long long)bc[r]);
}

/* scatter: contiguous chunk per block; pass 1 counts the block's rows per
 * rank, one global cursor reservation per (block, rank), pass 2 places rows
 * at LDS-allocated in-block offsets (re-reads the chunk from L2). */
__global__ void k_part_scatter(const int64_t *__restrict__ keys, int64_t n,
                               uint32_t nranks,
                               unsigned long long *__restrict__ cursor,
                               int64_t *__restrict__ perm)
{
    __shared__ unsigned int lcur[PART_MAX_RANKS];
    __shared__ long long base[PART_MAX_RANKS];
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int r = threadIdx.x; r < (int)nranks; r += blockDim.x) lcur[r] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        atomicAdd(&lcur[(uint32_t)(((uint64_t)keys[i]) % nranks)], 1u);
    __syncthreads();
    for (int r = threadIdx.x; r < (int)nranks; r += blockDim.x) {
        base[r] = lcur[r]
                      ? (long long)atomicAdd(&cursor[r],
                                             (unsigned long long)lcur[r])
                      : 0;
        lcur[r] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t owner = (uint32_t)(((uint64_t)keys[i]) % nranks);
        unsigned int off = atomicAdd(&lcur[owner], 1u);
        perm[base[owner] + off] = i;
    }
}

extern "C" {

otbx_status otbx_partition_by_key(const int64_t *keys, int64_t n,
                                  uint32_t nranks, int64_t *perm,
                                  int64_t *counts_host, void *stream)
{
    if (nranks == 0 || nranks > PART_MAX_RANKS || !counts_host)
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    static unsigned long long *scratch = nullptr; /* counts + cursors */
    if (!scratch)
        SCR_ALLOC_DEV(scratch, PART_MAX_RANKS * 2 * 8);
    unsigned long long *counts = scratch, *cursor = scratch + PART_MAX_RANKS;
    HIP_CHECK(hipMemsetAsync(counts, 0, PART_MAX_RANKS * 8, s));
    if (n > 0)
        hipLaunchKernelGGL(k_part_count, dim3(grid_for(n, 256)), dim3(256), 0,
                           s, keys, n, nranks, counts);
    static int64_t *h_counts = nullptr;
    if (!h_counts)
        SCR_ALLOC_HOST(h_counts, PART_MAX_RANKS * 8);
    HIP_CHECK(hipMemcpyAsync(h_counts, counts, nranks * 8,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t off = 0;
    static int64_t *h_cursor = nullptr;
    if (!h_cursor)
        SCR_ALLOC_HOST(h_cursor, PART_MAX_RANKS * 8);
    for (uint32_t r = 0; r < nranks; r++) {
        counts_host[r] = h_counts[r];
        h_cursor[r] = off;
        off += h_counts[r];
    }
    HIP_CHECK(hipMemcpyAsync(cursor, h_cursor, nranks * 8,
                             hipMemcpyHostToDevice, s));
    if (n > 0)
        hipLaunchKernelGGL(k_part_scatter, dim3(grid_for(n, 256)), dim3(256),
                           0, s, keys, n, nranks, cursor, perm);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gather_i64(const int64_t *src, const int64_t *perm, int64_t n,
                            int64_t *dst, void *stream)
{
    if (n > 0)
        hipLaunchKernelGGL(k_gather<int64_t>, dim3(grid_for(n, 256)), dim3(256),
                           0, (hipStream_t)stream, src, perm, n, dst);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gather_f64(const double *src, const int64_t *perm, int64_t n,
                            double *dst, void *stream)
{
    if (n > 0)
        hipLaunchKernelGGL(k_gather<double>, dim3(grid_for(n, 256)), dim3(256),
                           0, (hipStream_t)stream, src, perm, n, dst);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gather_i32(const int32_t *src, const int64_t *perm, int64_t n,
                            int32_t *dst, void *stream)
{
    if (n > 0)
        hipLaunchKernelGGL(k_gather<int32_t>, dim3(grid_for(n, 256)), dim3(256),
                           0, (hipStream_t)stream, src, perm, n, dst);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_gather_u8(const uint8_t *src, const int64_t *perm, int64_t n,
                           uint8_t *dst, void *stream)
{
    if (n > 0)
        hipLaunchKernelGGL(k_gather<uint8_t>, dim3(grid_for(n, 256)), dim3(256),
                           0, (hipStream_t)stream, src, perm, n, dst);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ================= generic inner hash join (otbx_join_i64) ================= */

/* build slot: {idx (claim word, -1 empty), key}; duplicates occupy their own
 * slots; probe walks to the first unclaimed slot. */
struct join_slot {
    long long idx;
    long long key;
};

__global__ void k_join_init(join_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride)
        tab[i].idx = -1;
}

__global__ void k_join_build(const int64_t *__restrict__ keys,
                             const uint8_t *__restrict__ knull, int64_t nb,
                             join_slot *tab, int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nb;
         i += stride) {
        if (knull && knull[i])
            continue; /* NULL join key never matches (nodeHash.c:2026) */
        int64_t k = keys[i];
        int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
        while (atomicCAS((unsigned long long *)&tab[s].idx,
                         (unsigned long long)(-1ll),
                         (unsigned long long)i) != (unsigned long long)(-1ll))
            s = (s + 1) & mask;
        tab[s].key = k; /* plain store: read only by the NEXT launch */
    }
}

__global__ void k_join_probe(const join_slot *__restrict__ tab, int64_t cap,
                             const int64_t *__restrict__ pkeys,
                             const uint8_t *__restrict__ pnull, int64_t np,
                             int64_t *__restrict__ out_b,
                             int64_t *__restrict__ out_p, int64_t cap_pairs,
                             int64_t *npairs)
{
    /* wave-uniform chain walk (all lanes step while any is walking, so the
     * match ballot is wave-converged) + per-wave LDS pair buffer: one
     * global counter reservation per 512 pairs instead of per pair. */
    const int BUF = 512;
    __shared__ int64_t bufb[256 / WAVE][BUF];
    __shared__ int64_t bufp[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0; /* wave-uniform */
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool active = i0 < np && !(pnull && pnull[i0]);
        int64_t k = pkeys[active ? i0 : 0];
        int64_t s = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
        bool walking = active;
        while (__any(walking)) {
            long long bidx = walking ? tab[s].idx : -1;
            bool have = walking && bidx >= 0;
            bool match = have && tab[s].key == k;
            /* buffered pair append (converged point) */
            unsigned long long mmask = __ballot(match);
            int cnt = __popcll(mmask);
            if (cnt) {
                if (nbuf + cnt > BUF) {
                    long long base = 0;
                    if (lane == 0)
                        base = (long long)atomicAdd(
                            (unsigned long long *)npairs,
                            (unsigned long long)nbuf);
                    base = __shfl(base, 0, WAVE);
                    for (int j = lane; j < nbuf; j += WAVE) {
                        int64_t pos = base + j;
                        if (pos < cap_pairs) {
                            out_b[pos] = bufb[wid][j];
                            out_p[pos] = bufp[wid][j];
                        }
                    }
                    nbuf = 0;
                }
                if (match) {
                    int rank = __popcll(mmask & ((1ull << lane) - 1ull));
                    bufb[wid][nbuf + rank] = bidx;
                    bufp[wid][nbuf + rank] = i0;
                }
                nbuf += cnt;
            }
            s = (s + 1) & mask;
            walking = have;
        }
        if (__all(i0 >= np))
            break;
    }
    if (nbuf) {
        long long base = 0;
        if (lane == 0)
            base = (long long)atomicAdd((unsigned long long *)npairs,
                                        (unsigned long long)nbuf);
        base = __shfl(base, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE) {
            int64_t pos = base + j;
            if (pos < cap_pairs) {
                out_b[pos] = bufb[wid][j];
                out_p[pos] = bufp[wid][j];
            }
        }
    }
}

/* ---- partitioned join (build ≥ JOINP_THRESHOLD rows) ----
 * The single shared table runs at 4.8 Gprobes/s at a 150 M-row build
 * (random 64-B line per probe step). Hash-partition BOTH sides with the
 * same bucket bits (reusing the aggregation partitioner: level-1
 * k_joinp_scatter, level-2 k_aggp_scatter_kv2 — records are (key, row)
 * pairs) into key-disjoint buckets whose build side fits an LDS chained
 * table; each block joins one bucket with streaming reads. A bucket whose
 * build side exceeds the LDS capacity (row skew, or an INT64_MIN key — the
 * LDS table's claim sentinel) is FLAGGED and joined by the global-table
 * fallback kernels instead. */
#define JOINP_THRESHOLD (8ll << 20) /* measured: partitioned wins 28.7 vs
                                     * 49.5 ms at a 15 M-row build, 38.7 vs
                                     * 125 ms at 150 M (600 M probes) */
#define JB_CAP 768 /* max build rows per final bucket (LDS arrays) */

__global__ void k_joinp_scatter(const int64_t *__restrict__ keys,
                                const uint8_t *__restrict__ knull, int64_t n,
                                uint32_t nbuk, unsigned long long *cursor,
                                ulonglong2 *__restrict__ recs)
{
    __shared__ unsigned int lcur[AGGP_MAX_BUCKETS];
    __shared__ long long base[AGGP_MAX_BUCKETS];
    int64_t per_block = (n + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < n ? lo + per_block : n;
    for (int i = threadIdx.x; i < (int)nbuk; i += blockDim.x) lcur[i] = 0;
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (knull && knull[i]) continue; /* NULL keys never match */
        atomicAdd(&lcur[d_agg_bucket(keys[i], nbuk)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (int)nbuk; i += blockDim.x) {
        base[i] = lcur[i] ? (long long)atomicAdd(
                                &cursor[i], (unsigned long long)lcur[i])
                          : 0;
        lcur[i] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (knull && knull[i]) continue;
        int64_t k = keys[i];
        uint32_t b = d_agg_bucket(k, nbuk);
        unsigned int off = atomicAdd(&lcur[b], 1u);
        ulonglong2 r;
        r.x = (unsigned long long)k;
        r.y = (unsigned long long)i;
        recs[base[b] + off] = r;
    }
}

/* per-bucket LDS chained join. Build: open-addressing key slots (claim
 * sentinel INT64_MIN → such keys force the fallback) with a chain head per
 * slot; entries chain through lnext. Probe runs TWICE: a counting pass,
 * then ONE global reservation per block, then an emitting pass writing
 * pairs at exact offsets through an LDS cursor — per-wave buffer flushes
 * to the single pair counter measured 2.3 M reservations ≈ 27 ms at 600 M
 * pairs (the ~88/µs single-counter law); this form makes one per block. */
__global__ void k_joinp_bucket(const ulonglong2 *__restrict__ brecs,
                               const unsigned long long *__restrict__ boffs,
                               const unsigned long long *__restrict__ bcnts,
                               const ulonglong2 *__restrict__ precs,
                               const unsigned long long *__restrict__ poffs,
                               const unsigned long long *__restrict__ pcnts,
                               uint8_t *__restrict__ flags,
                               unsigned int *nflagged,
                               int64_t *__restrict__ out_b,
                               int64_t *__restrict__ out_p, int64_t cap_pairs,
                               int64_t *npairs)
{
    const int HSLOTS = 1024;
    __shared__ long long hkey[HSLOTS];
    __shared__ int hhead[HSLOTS];
    __shared__ int lnext[JB_CAP];
    __shared__ int bfail;
    __shared__ unsigned long long bbase;
    __shared__ unsigned int bcur;
    int64_t blo = (int64_t)boffs[blockIdx.x];
    int64_t nbb = (int64_t)bcnts[blockIdx.x];
    if (threadIdx.x == 0) {
        bfail = nbb > JB_CAP;
        bcur = 0;
    }
    for (int t = threadIdx.x; t < HSLOTS; t += blockDim.x) {
        hkey[t] = INT64_MIN;
        hhead[t] = -1;
    }
    __syncthreads();
    if (!bfail) {
        for (int e = threadIdx.x; e < (int)nbb; e += blockDim.x) {
            int64_t k = (int64_t)brecs[blo + e].x;
            if (k == INT64_MIN) {
                bfail = 1;
                break;
            }
            uint64_t h = d_hash_i64(k);
            int t0 = (int)(h & (HSLOTS - 1));
            int step = (int)(((h >> 52) & (HSLOTS - 2)) | 1ull);
            bool placed = false;
            for (int t = 0; t < HSLOTS; t++) {
                long long old = atomicCAS((unsigned long long *)&hkey[t0],
                                          (unsigned long long)INT64_MIN,
                                          (unsigned long long)k);
                if (old == INT64_MIN || old == k) {
                    lnext[e] = atomicExch(&hhead[t0], e);
                    placed = true;
                    break;
                }
                t0 = (t0 + step) & (HSLOTS - 1);
            }
            if (!placed) bfail = 1; /* cannot happen at load ≤ 0.75 */
        }
    }
    __syncthreads();
    if (bfail) {
        if (threadIdx.x == 0) {
            flags[blockIdx.x] = 1;
            atomicAdd(nflagged, 1u);
        }
        return;
    }
    int64_t plo = (int64_t)poffs[blockIdx.x];
    int64_t npb = (int64_t)pcnts[blockIdx.x];
    int lane = (int)(threadIdx.x % WAVE);
    /* pass 1: count matches */
    unsigned int my = 0;
    for (int64_t i0 = threadIdx.x; i0 < npb; i0 += blockDim.x) {
        int64_t k = (int64_t)precs[plo + i0].x;
        if (k == INT64_MIN) continue;
        uint64_t h = d_hash_i64(k);
        int t0 = (int)(h & (HSLOTS - 1));
        int step = (int)(((h >> 52) & (HSLOTS - 2)) | 1ull);
        int e = -1;
        for (;;) {
            long long sk = hkey[t0];
            if (sk == k) {
                e = hhead[t0];
                break;
            }
            if (sk == INT64_MIN) break;
            t0 = (t0 + step) & (HSLOTS - 1);
        }
        while (e >= 0) {
            my++;
            e = lnext[e];
        }
    }
    {
        unsigned int w = my;
        for (int off = WAVE / 2; off > 0; off >>= 1)
            w += (unsigned int)__shfl_down((int)w, off, WAVE);
        if (lane == 0 && w) atomicAdd(&bcur, w);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bbase = bcur ? (unsigned long long)atomicAdd(
                           (unsigned long long *)npairs,
                           (unsigned long long)bcur)
                     : 0;
        bcur = 0;
    }
    __syncthreads();
    /* pass 2: emit at exact offsets (LDS cursor, zero global atomics) */
    for (int64_t i0 = threadIdx.x; i0 < npb; i0 += blockDim.x) {
        ulonglong2 pr = precs[plo + i0];
        int64_t k = (int64_t)pr.x;
        if (k == INT64_MIN) continue;
        uint64_t h = d_hash_i64(k);
        int t0 = (int)(h & (HSLOTS - 1));
        int step = (int)(((h >> 52) & (HSLOTS - 2)) | 1ull);
        int e = -1;
        for (;;) {
            long long sk = hkey[t0];
            if (sk == k) {
                e = hhead[t0];
                break;
            }
            if (sk == INT64_MIN) break;
            t0 = (t0 + step) & (HSLOTS - 1);
        }
        if (e < 0) continue;
        unsigned int cnt = 0;
        for (int e2 = e; e2 >= 0; e2 = lnext[e2]) cnt++;
        int64_t pos = (int64_t)bbase + atomicAdd(&bcur, cnt);
        for (; e >= 0; e = lnext[e]) {
            if (pos < cap_pairs) {
                out_b[pos] = (long long)brecs[blo + e].y;
                out_p[pos] = (long long)pr.y;
            }
            pos++;
        }
    }
}

/* fallback for flagged buckets: build/probe through the global idx-claim
 * table (key-agnostic, handles INT64_MIN and any skew) */
__global__ void k_joinp_build_flagged(const ulonglong2 *__restrict__ brecs,
                                      const unsigned long long *__restrict__ boffs,
                                      const unsigned long long *__restrict__ bcnts,
                                      const uint8_t *__restrict__ flags,
                                      join_slot *tab, int64_t cap)
{
    if (!flags[blockIdx.x]) return;
    int64_t mask = cap - 1;
    int64_t lo = (int64_t)boffs[blockIdx.x];
    int64_t hi = lo + (int64_t)bcnts[blockIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        ulonglong2 r = brecs[i];
        int64_t k = (int64_t)r.x;
        int64_t t = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
        while (atomicCAS((unsigned long long *)&tab[t].idx,
                         (unsigned long long)(-1ll), r.y) !=
               (unsigned long long)(-1ll))
            t = (t + 1) & mask;
        tab[t].key = k;
    }
}

__global__ void k_joinp_probe_flagged(const join_slot *__restrict__ tab,
                                      int64_t cap,
                                      const ulonglong2 *__restrict__ precs,
                                      const unsigned long long *__restrict__ poffs,
                                      const unsigned long long *__restrict__ pcnts,
                                      const uint8_t *__restrict__ flags,
                                      int64_t *__restrict__ out_b,
                                      int64_t *__restrict__ out_p,
                                      int64_t cap_pairs, int64_t *npairs)
{
    if (!flags[blockIdx.x]) return;
    int64_t mask = cap - 1;
    int64_t lo = (int64_t)poffs[blockIdx.x];
    int64_t npb = (int64_t)pcnts[blockIdx.x];
    for (int64_t i0 = threadIdx.x;; i0 += blockDim.x) {
        bool active = i0 < npb;
        ulonglong2 pr;
        pr.x = 0;
        pr.y = 0;
        if (active) pr = precs[lo + i0];
        int64_t k = (int64_t)pr.x;
        int64_t t = (int64_t)(d_hash_i64(k) & (uint64_t)mask);
        bool walking = active;
        while (__any(walking)) {
            long long bidx = walking ? tab[t].idx : -1;
            bool have = walking && bidx >= 0;
            bool match = have && tab[t].key == k;
            int64_t pos = wave_append(npairs, match);
            if (match && pos < cap_pairs) {
                out_b[pos] = bidx;
                out_p[pos] = (int64_t)pr.y;
            }
            t = (t + 1) & mask;
            walking = have;
        }
        if (__all(i0 >= npb)) break;
    }
}

extern "C" {

otbx_status otbx_join_i64_workspace_bytes(int64_t nb, int64_t np,
                                           size_t *bytes)
{
    int64_t cap = next_pow2_host(nb < 16 ? 16 : (int64_t)(nb / 0.7) + 1);
    size_t b = (size_t)cap * sizeof(join_slot);
    const char *fj = getenv("OTBX_JOINP_FORCE");
    if (nb >= JOINP_THRESHOLD || (fj && atoi(fj))) {
        /* two partition levels of (key,row) records for both sides +
         * level-1/level-2 bucket arrays + flags */
        b += (size_t)(nb + np) * 32 + (size_t)AGGP_MAX_BUCKETS * 8 * 6 +
             (size_t)(1 << 19) * (8 * 4 + 1) + 8192;
    }
    *bytes = b;
    return OTBX_OK;
}

otbx_status otbx_join_i64(const int64_t *bkeys, const uint8_t *bnull, int64_t nb,
                          const int64_t *pkeys, const uint8_t *pnull, int64_t np,
                          void *ws, size_t ws_bytes, int64_t *out_b,
                          int64_t *out_p, int64_t cap_pairs, int64_t *npairs_dev,
                          void *stream)
{
    int64_t cap = next_pow2_host(nb < 16 ? 16 : (int64_t)(nb / 0.7) + 1);
    {
        size_t need;
        otbx_join_i64_workspace_bytes(nb, np, &need);
        if (ws_bytes < need) return OTBX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    join_slot *tab = (join_slot *)ws;
    HIP_CHECK(hipMemsetAsync(npairs_dev, 0, sizeof(int64_t), s));

    const char *fj = getenv("OTBX_JOINP_FORCE"); /* test hook: force the
                                                   * partitioned path */
    if ((nb >= JOINP_THRESHOLD || (fj && atoi(fj))) && np > 0 && nb > 0) {
        /* partitioned path: bucket count from build ROWS (duplicates
         * occupy chain entries), aiming ≤ ~384 rows per final bucket */
        bool tile = part_tile_enabled() && nb < (int64_t)UINT32_MAX &&
                    np < (int64_t)UINT32_MAX;
        uint32_t nbuk = tile ? 256 : AGGP_MAX_BUCKETS;
        int64_t per_b = nb / nbuk;
        uint32_t nb2 = 1;
        if (per_b > 384) {
            nb2 = (uint32_t)next_pow2_host(per_b / 384 + 1);
            if (nb2 > AGGP_MAX_BUCKETS) nb2 = AGGP_MAX_BUCKETS;
            while ((size_t)nbuk * nb2 > (1 << 19)) nb2 >>= 1;
        }
        char *p = (char *)(tab + cap);
        ulonglong2 *brecs = (ulonglong2 *)p;
        ulonglong2 *brecs2 = brecs + nb;
        ulonglong2 *precs = brecs2 + nb;
        ulonglong2 *precs2 = precs + np;
        unsigned long long *cnts_b = (unsigned long long *)(precs2 + np);
        unsigned long long *cursor_b = cnts_b + AGGP_MAX_BUCKETS;
        unsigned long long *offs_b = cursor_b + AGGP_MAX_BUCKETS;
        unsigned long long *cnts_p = offs_b + AGGP_MAX_BUCKETS;
        unsigned long long *cursor_p = cnts_p + AGGP_MAX_BUCKETS;
        unsigned long long *offs_p = cursor_p + AGGP_MAX_BUCKETS;
        unsigned long long *bcnts2 = offs_p + AGGP_MAX_BUCKETS;
        unsigned long long *boffs2 = bcnts2 + (1 << 19);
        unsigned long long *pcnts2 = boffs2 + (1 << 19);
        unsigned long long *poffs2 = pcnts2 + (1 << 19);
        uint8_t *flags = (uint8_t *)(poffs2 + (1 << 19));
        HIP_CHECK(hipMemsetAsync(cnts_b, 0, (size_t)nbuk * 8, s));
        HIP_CHECK(hipMemsetAsync(cnts_p, 0, (size_t)nbuk * 8, s));
        hipLaunchKernelGGL(k_aggp_count, dim3(grid_for(nb, 256)), dim3(256),
                           0, s, bkeys, bnull, nb, nbuk, cnts_b);
        hipLaunchKernelGGL(k_aggp_count, dim3(grid_for(np, 256)), dim3(256),
                           0, s, pkeys, pnull, np, nbuk, cnts_p);
        static unsigned long long *h_j = nullptr;
        if (!h_j) SCR_ALLOC_HOST(h_j, AGGP_MAX_BUCKETS * 8 * 4);
        HIP_CHECK(hipMemcpyAsync(h_j, cnts_b, (size_t)nbuk * 8,
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(h_j + AGGP_MAX_BUCKETS, cnts_p,
                                 (size_t)nbuk * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        unsigned long long *h_ob = h_j + 2 * AGGP_MAX_BUCKETS;
        unsigned long long *h_op = h_j + 3 * AGGP_MAX_BUCKETS;
        unsigned long long ab = 0, ap = 0;
        for (uint32_t b = 0; b < nbuk; b++) {
            h_ob[b] = ab;
            ab += h_j[b];
            h_op[b] = ap;
            ap += h_j[AGGP_MAX_BUCKETS + b];
        }
        HIP_CHECK(hipMemcpyAsync(offs_b, h_ob, (size_t)nbuk * 8,
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(cursor_b, h_ob, (size_t)nbuk * 8,
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(offs_p, h_op, (size_t)nbuk * 8,
                                 hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(cursor_p, h_op, (size_t)nbuk * 8,
                                 hipMemcpyHostToDevice, s));
        if (tile) {
            hipLaunchKernelGGL(k_tile_scatter1, dim3(2048), dim3(1024), 0, s,
                               bkeys, bnull, nullptr, nb, nbuk, cursor_b,
                               brecs);
            hipLaunchKernelGGL(k_tile_scatter1, dim3(2048), dim3(1024), 0, s,
                               pkeys, pnull, nullptr, np, nbuk, cursor_p,
                               precs);
        } else {
            hipLaunchKernelGGL(k_joinp_scatter, dim3(grid_for(nb, 256)),
                               dim3(256), 0, s, bkeys, bnull, nb, nbuk,
                               cursor_b, brecs);
            hipLaunchKernelGGL(k_joinp_scatter, dim3(grid_for(np, 256)),
                               dim3(256), 0, s, pkeys, pnull, np, nbuk,
                               cursor_p, precs);
        }
        const ulonglong2 *fb = brecs, *fp = precs;
        const unsigned long long *fbo = offs_b, *fbc = cnts_b;
        const unsigned long long *fpo = offs_p, *fpc = cnts_p;
        uint32_t fgrid = nbuk;
        if (nb2 > 1) {
            if (tile) {
                HIP_CHECK(hipMemsetAsync(bcnts2, 0, (size_t)nbuk * nb2 * 8,
                                         s));
                HIP_CHECK(hipMemsetAsync(pcnts2, 0, (size_t)nbuk * nb2 * 8,
                                         s));
                hipLaunchKernelGGL(k_tile_count2, dim3(16, nbuk), dim3(256),
                                   0, s, brecs, offs_b, cnts_b, nb2, bcnts2);
                hipLaunchKernelGGL(k_tile_scan2, dim3(nbuk), dim3(64), 0, s,
                                   offs_b, nb2, bcnts2, boffs2);
                hipLaunchKernelGGL(k_tile_scatter2, dim3(8, nbuk), dim3(1024),
                                   0, s, brecs, offs_b, cnts_b, nb2, boffs2,
                                   brecs2);
                hipLaunchKernelGGL(k_tile_restore_offs,
                                   dim3(grid_for((int64_t)nbuk * nb2, 256)),
                                   dim3(256), 0, s, boffs2, bcnts2,
                                   (int64_t)nbuk * nb2);
                hipLaunchKernelGGL(k_tile_count2, dim3(16, nbuk), dim3(256),
                                   0, s, precs, offs_p, cnts_p, nb2, pcnts2);
                hipLaunchKernelGGL(k_tile_scan2, dim3(nbuk), dim3(64), 0, s,
                                   offs_p, nb2, pcnts2, poffs2);
                hipLaunchKernelGGL(k_tile_scatter2, dim3(8, nbuk), dim3(1024),
                                   0, s, precs, offs_p, cnts_p, nb2, poffs2,
                                   precs2);
                hipLaunchKernelGGL(k_tile_restore_offs,
                                   dim3(grid_for((int64_t)nbuk * nb2, 256)),
                                   dim3(256), 0, s, poffs2, pcnts2,
                                   (int64_t)nbuk * nb2);
            } else {
                hipLaunchKernelGGL(k_aggp_scatter_kv2, dim3(nbuk), dim3(256),
                                   0, s, brecs, offs_b, cnts_b, nb2, brecs2,
                                   boffs2, bcnts2);
                hipLaunchKernelGGL(k_aggp_scatter_kv2, dim3(nbuk), dim3(256),
                                   0, s, precs, offs_p, cnts_p, nb2, precs2,
                                   poffs2, pcnts2);
            }
            fb = brecs2;
            fbo = boffs2;
            fbc = bcnts2;
            fp = precs2;
            fpo = poffs2;
            fpc = pcnts2;
            fgrid = (uint32_t)(nbuk * nb2);
        }
        static unsigned int *d_nflag = nullptr;
        static unsigned int *h_nflag = nullptr;
        if (!d_nflag) {
            SCR_ALLOC_DEV(d_nflag, 4);
            SCR_ALLOC_HOST(h_nflag, 4);
        }
        HIP_CHECK(hipMemsetAsync(d_nflag, 0, 4, s));
        HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)fgrid, s));
        hipLaunchKernelGGL(k_joinp_bucket, dim3(fgrid), dim3(256), 0, s, fb,
                           fbo, fbc, fp, fpo, fpc, flags, d_nflag, out_b,
                           out_p, cap_pairs, npairs_dev);
        HIP_CHECK(hipMemcpyAsync(h_nflag, d_nflag, 4, hipMemcpyDeviceToHost,
                                 s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (*h_nflag > 0) {
            hipLaunchKernelGGL(k_join_init, dim3(grid_for(cap, 256)),
                               dim3(256), 0, s, tab, cap);
            hipLaunchKernelGGL(k_joinp_build_flagged, dim3(fgrid), dim3(256),
                               0, s, fb, fbo, fbc, flags, tab, cap);
            hipLaunchKernelGGL(k_joinp_probe_flagged, dim3(fgrid), dim3(256),
                               0, s, tab, cap, fp, fpo, fpc, flags, out_b,
                               out_p, cap_pairs, npairs_dev);
        }
        HIP_CHECK(hipGetLastError());
        return OTBX_OK;
    }

    hipLaunchKernelGGL(k_join_init, dim3(grid_for(cap, 256)), dim3(256), 0, s,
                       tab, cap);
    if (nb > 0)
        hipLaunchKernelGGL(k_join_build, dim3(grid_for(nb, 256)), dim3(256), 0, s,
                           bkeys, bnull, nb, tab, cap);
    if (np > 0)
        hipLaunchKernelGGL(k_join_probe, dim3(grid_for(np, 256)), dim3(256), 0, s,
                           tab, cap, pkeys, pnull, np, out_b, out_p, cap_pairs,
                           npairs_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ================= TPC-H Q3 DN fragment ================= */

/* The Q3 hash tables (customer keyset, orders table, group table) are
 * cleared with memset(0) and claim slots by CAS on the key word, so one
 * 64-bit pattern has to mean "empty". Keys are stored with the sign bit
 * flipped (q3_kenc): the empty word 0 then stands for INT64_MIN, the one key
 * value otbx.h reserves, and key 0 and negative keys are ordinary keys.
 * Hashing stays on the raw key. */
__device__ __forceinline__ unsigned long long q3_kenc(int64_t k)
{
    return (unsigned long long)k ^ 0x8000000000000000ull;
}
__device__ __forceinline__ int64_t q3_kdec(unsigned long long v)
{
    return (int64_t)(v ^ 0x8000000000000000ull);
}

/* keyset table (filtered customer): stored word q3_kenc(custkey), EMPTY = 0 */
__global__ void k_keyset_build(const int64_t *__restrict__ keys, int64_t n,
                               unsigned long long *tab, int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        unsigned long long k = q3_kenc(keys[i]);
        int64_t s = (int64_t)(d_hash_i64(keys[i]) & (uint64_t)mask);
        for (;;) {
            unsigned long long old = atomicCAS(&tab[s], 0ull, k);
            if (old == 0ull || old == k) break; /* dedupe: set semantics */
            s = (s + 1) & mask;
        }
    }
}

/* filter+build fused for the local (non-broadcast) path */
__global__ void k_keyset_build_filter(const int64_t *__restrict__ keys,
                                      const uint8_t *__restrict__ seg, uint8_t want,
                                      int64_t n, unsigned long long *tab,
                                      int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (seg[i] != want)
            continue;
        unsigned long long k = q3_kenc(keys[i]);
        int64_t s = (int64_t)(d_hash_i64(keys[i]) & (uint64_t)mask);
        for (;;) {
            unsigned long long old = atomicCAS(&tab[s], 0ull, k);
            if (old == 0ull || old == k) break;
            s = (s + 1) & mask;
        }
    }
}

__device__ __forceinline__ bool d_keyset_probe(const unsigned long long *tab,
                                               int64_t cap, int64_t key)
{
    int64_t mask = cap - 1;
    int64_t s = (int64_t)(d_hash_i64(key) & (uint64_t)mask);
    for (;;) {
        unsigned long long v = tab[s];
        if (v == 0ull) return false; /* empty first: a probe key that
                                      * encodes to 0 can never hit */
        if (v == q3_kenc(key)) return true;
        s = (s + 1) & mask;
    }
}

/* orders hash table: slot {q3_kenc(okey) (EMPTY=0), date, prio};
 * o_orderkey unique */
struct ord_slot {
    unsigned long long okey;
    int32_t date;
    int32_t prio;
};

/* bloom pre-filter over the build keys (the reference's block bloom,
 * utils/misc/bloomfilter.c built in nodeHash.c:208, probed
 * nodeHashjoin.c:1862): ~90% of Q3 probes miss the orders table — testing
 * two bits in an L2/L3-resident bitset rejects them without touching the
 * (HBM-sized) hash table. */
__device__ __forceinline__ void d_bloom_set(unsigned long long *bloom,
                                            int64_t nwords, int64_t key)
{
    uint64_t h = d_hash_i64(key);
    uint64_t w = (h >> 12) & (uint64_t)(nwords - 1);
    unsigned long long bits =
        (1ull << (h & 63)) | (1ull << ((h >> 6) & 63));
    atomicOr(&bloom[w], bits);
}

__device__ __forceinline__ bool d_bloom_test(const unsigned long long *bloom,
                                             int64_t nwords, int64_t key)
{
    uint64_t h = d_hash_i64(key);
    uint64_t w = (h >> 12) & (uint64_t)(nwords - 1);
    unsigned long long bits =
        (1ull << (h & 63)) | (1ull << ((h >> 6) & 63));
    return (bloom[w] & bits) == bits;
}

/* orders side, FUSED single pass (when the customer filter is the dense
 * bitmap, its test is an L2-resident word — no reason to materialize the
 * date-filtered candidate list first): 4 rows/lane via 16-B vector loads,
 * date qual + custkey filter, LDS-staged append of matched row ids +
 * matched-orderkey min/max for the direct-path decision. */
__global__ void k_ord_filter_probe_fused(const otbx_orders_dev o,
                                         int32_t q3date,
                                         const unsigned long long *__restrict__ ckeys,
                                         int64_t ccap,
                                         const unsigned long long *__restrict__ cbitmap,
                                         int64_t cmin, int64_t crange,
                                         int64_t *__restrict__ out,
                                         int64_t *nout,
                                         unsigned long long *minkey,
                                         unsigned long long *maxkey)
{
    const int BUF = 1024;
    __shared__ int64_t buf[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0;
    unsigned long long mymin = ~0ull >> 1, mymax = 0;
    int64_t nq = o.n / 4;
    const int4 *od4 = (const int4 *)o.o_orderdate;
    const longlong2 *ck2 = (const longlong2 *)o.o_custkey;
    const longlong2 *okk2 = (const longlong2 *)o.o_orderkey;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         q += stride) {
        bool m[4] = {false, false, false, false};
        int64_t r0 = q * 4;
        int mycnt = 0;
        if (q < nq) {
            int4 d = od4[q];
            longlong2 ca = ck2[2 * q], cb = ck2[2 * q + 1];
            longlong2 ka = okk2[2 * q], kb = okk2[2 * q + 1];
            int32_t ds[4] = {d.x, d.y, d.z, d.w};
            int64_t ck[4] = {ca.x, ca.y, cb.x, cb.y};
            int64_t ok[4] = {ka.x, ka.y, kb.x, kb.y};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bool pass = ds[j] < q3date;       /* ExecQual on orders */
                if (pass) {
                    if (cbitmap) {
                        int64_t idx = ck[j] - cmin;
                        pass = idx >= 0 && idx < crange &&
                               ((cbitmap[idx >> 6] >> (idx & 63)) & 1ull);
                    } else {
                        pass = d_keyset_probe(ckeys, ccap, ck[j]);
                    }
                }
                m[j] = pass;
                if (pass) {
                    mycnt++;
                    unsigned long long k = (unsigned long long)ok[j];
                    if (k < mymin) mymin = k;
                    if (k > mymax) mymax = k;
                }
            }
        } else if (q == nq) { /* tail rows */
            for (int64_t i = nq * 4; i < o.n; i++) {
                int j = (int)(i - nq * 4);
                bool pass = o.o_orderdate[i] < q3date;
                if (pass) {
                    int64_t ckv = o.o_custkey[i];
                    if (cbitmap) {
                        int64_t idx = ckv - cmin;
                        pass = idx >= 0 && idx < crange &&
                               ((cbitmap[idx >> 6] >> (idx & 63)) & 1ull);
                    } else {
                        pass = d_keyset_probe(ckeys, ccap, ckv);
                    }
                }
                m[j] = pass;
                if (pass) {
                    mycnt++;
                    unsigned long long k = (unsigned long long)o.o_orderkey[i];
                    if (k < mymin) mymin = k;
                    if (k > mymax) mymax = k;
                }
            }
        }
        int incl = mycnt;
        for (int off = 1; off < WAVE; off <<= 1) {
            int up = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += up;
        }
        int tot = __shfl(incl, WAVE - 1, WAVE);
        if (tot) {
            if (nbuf + tot > BUF) {
                long long bpos = 0;
                if (lane == 0)
                    bpos = (long long)atomicAdd((unsigned long long *)nout,
                                                (unsigned long long)nbuf);
                bpos = __shfl(bpos, 0, WAVE);
                for (int j = lane; j < nbuf; j += WAVE)
                    out[bpos + j] = buf[wid][j];
                nbuf = 0;
            }
            int pos = nbuf + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j])
                    buf[wid][pos++] = r0 + j;
            nbuf += tot;
        }
        if (__all(q >= nq))
            break;
    }
    if (nbuf) {
        long long bpos = 0;
        if (lane == 0)
            bpos = (long long)atomicAdd((unsigned long long *)nout,
                                        (unsigned long long)nbuf);
        bpos = __shfl(bpos, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE)
            out[bpos + j] = buf[wid][j];
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        unsigned long long mn = (unsigned long long)__shfl_down(
            (long long)mymin, off, WAVE);
        unsigned long long mx = (unsigned long long)__shfl_down(
            (long long)mymax, off, WAVE);
        if (mn < mymin) mymin = mn;
        if (mx > mymax) mymax = mx;
    }
    if (lane == 0) {
        if (mymin != (~0ull >> 1)) atomicMin(minkey, mymin);
        if (mymax) atomicMax(maxkey, mymax);
    }
}

/* orders side, candidate-list pipeline (same rationale as the lineitem
 * scan): date-filter to a dense row-id list, dense customer-keyset probe to
 * a matched list (count = table size), dense insert into the right-sized
 * table + bloom. Replaces a divergent fused build + a duplicated counting
 * pass. */
/* pass/npasses: grace batching for the hash path — a pass
 * owns the keys with hash % npasses == pass, so per-pass table memory is
 * bounded; the scan's bloom filter is rebuilt per pass and naturally admits
 * only that pass's keys. */
__global__ void k_ord_insert(const otbx_orders_dev o,
                             const int64_t *__restrict__ cand,
                             const int64_t *__restrict__ ncand_p,
                             ord_slot *tab, int64_t cap,
                             unsigned long long *bloom, int64_t bloom_words,
                             uint32_t pass, uint32_t npasses)
{
    int64_t mask = cap - 1;
    int64_t n = *ncand_p;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < n;
         ci += stride) {
        int64_t i = cand[ci];
        int64_t rk = o.o_orderkey[i];
        unsigned long long k = q3_kenc(rk);
        uint64_t h = d_hash_i64(rk);
        if (npasses > 1 && (uint32_t)(h >> 32) % npasses != pass)
            continue;
        if (k == 0ull)
            continue; /* reserved key (otbx.h): never inserted, never hit */
        d_bloom_set(bloom, bloom_words, rk);
        int64_t s = (int64_t)(h & (uint64_t)mask);
        while (atomicCAS(&tab[s].okey, 0ull, k) != 0ull)
            s = (s + 1) & mask;      /* keys unique: claim exactly one slot */
        tab[s].date = o.o_orderdate[i];   /* plain: read by NEXT launch */
        tab[s].prio = o.o_shippriority[i];
    }
}

__global__ void k_ord_count_pass(const otbx_orders_dev o,
                                 const int64_t *__restrict__ cand,
                                 const int64_t *__restrict__ ncand_p,
                                 uint32_t pass, uint32_t npasses,
                                 int64_t *count)
{
    int64_t n = *ncand_p;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long my = 0;
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < n;
         ci += stride) {
        uint64_t h = d_hash_i64(o.o_orderkey[cand[ci]]);
        my += (uint32_t)(h >> 32) % npasses == pass;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
        my += __shfl_down(my, off, WAVE);
    if ((threadIdx.x % WAVE) == 0 && my)
        atomicAdd((unsigned long long *)count, my);
}

/* ---- dense-orderkey DIRECT path ----
 * When the filtered build side's key range (max-min+1) fits
 * OTBX_DIRECT_CAP, hashing is strictly worse than direct addressing: the
 * probe stream arrives in (clustered) key order, so un-hashed bitmap/table
 * indices give consecutive probes the SAME cache lines — the random-line
 * traffic that bounds the hash path collapses to streaming. The reference
 * always hashes (nodeHash.c); on MI355X the locality is worth preserving.
 * Fallback to the bloom+hash path above when the range is too wide
 * (sparse keys). The packed payload date | prio<<32 has no reserved
 * value (day 0 with priority 0 packs to 0): presence lives in the bitmap
 * alone. */
#define OTBX_DIRECT_CAP_DEFAULT (1ll << 29)

/* direct-table entry: revenue accumulator + packed (date|prio<<32) payload
 * INTERLEAVED so the insert's zero+payload store, the probe's payload read
 * + revenue atomicAdd, and the compaction's gather each touch ONE cache
 * line per entry instead of two (the split ptab/rtab layout cost a line
 * each). Every mode is bitmap-authoritative: entries at unset bits are
 * stale and never emitted. */
struct q3_rec {
    double rev;
    unsigned long long pl;
};

/* "Some lineitem matched" is carried by the accumulator's sign bit, not by
 * its value: the build side stores -0.0, and every probe add is a value
 * with its zero normalised to +0.0 (q3_pos0). Under round-to-nearest
 * -0.0 + x is x for x != 0, -0.0 + +0.0 is +0.0, and an exact cancellation
 * x + -x is +0.0, so the bit pattern of -0.0 survives if and only if no add
 * happened. A group whose revenue sums to zero is therefore still a group.
 * Costs no extra table traffic (a second "matched" bitmap would add one
 * atomic per hit). */
#define Q3_REV_UNMATCHED (-0.0)
__device__ __forceinline__ double q3_pos0(double x)
{
    return x == 0.0 ? 0.0 : x;
}
__device__ __forceinline__ bool q3_matched(double rev)
{
    return (unsigned long long)__double_as_longlong(rev) !=
           0x8000000000000000ull;
}

/* single-pass orders side for the common dense case: when the UNFILTERED
 * orderkey range already fits the direct table (known from a cheap minmax
 * overlapped with the customer phase), the date qual + customer filter
 * writes the bitmap/payload table directly — no candidate list and no
 * separate insert pass (measured 0.92 + 0.91 ms as two kernels). */
template <bool K32>
__global__ void k_ord_filter_insert_fused(
    const otbx_orders_dev o, int32_t q3date,
    const unsigned long long *__restrict__ ckeys, int64_t ccap,
    const unsigned long long *__restrict__ cbitmap, int64_t cmin,
    int64_t crange, int64_t mino, int64_t range,
    unsigned long long *__restrict__ bitmap, q3_rec *__restrict__ grec)
{
    int64_t nq = o.n / 4;
    const int4 *od4 = (const int4 *)o.o_orderdate;
    const int4 *op4 = (const int4 *)o.o_shippriority;
    const longlong2 *ck2 = (const longlong2 *)o.o_custkey;
    const longlong2 *okk2 = (const longlong2 *)o.o_orderkey;
    /* K32 (otbx.h o_orderkey32/o_custkey32): 24 -> 16 B/row stream */
    const int4 *ck4 = (const int4 *)o.o_custkey32;
    const int4 *ok4 = (const int4 *)o.o_orderkey32;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq;
         q += stride) {
        int4 d = od4[q];
        int64_t ck[4];
        int64_t ok[4];
        if (K32) {
            int4 cc = ck4[q], kk = ok4[q];
            ck[0] = cc.x; ck[1] = cc.y; ck[2] = cc.z; ck[3] = cc.w;
            ok[0] = kk.x; ok[1] = kk.y; ok[2] = kk.z; ok[3] = kk.w;
        } else {
            longlong2 ca = ck2[2 * q], cb = ck2[2 * q + 1];
            longlong2 ka = okk2[2 * q], kb = okk2[2 * q + 1];
            ck[0] = ca.x; ck[1] = ca.y; ck[2] = cb.x; ck[3] = cb.y;
            ok[0] = ka.x; ok[1] = ka.y; ok[2] = kb.x; ok[3] = kb.y;
        }
        int4 pr = op4[q];
        int32_t ds[4] = {d.x, d.y, d.z, d.w};
        int32_t prio[4] = {pr.x, pr.y, pr.z, pr.w};
        /* branchless filter phase first: the 4 customer-bitmap gathers
         * issue independently (the early-continue form serialized them
         * behind each j's control flow) */
        bool m[4];
        if (cbitmap) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int64_t cidx = ck[j] - cmin;
                bool in = (ds[j] < q3date) /* ExecQual on orders */ &&
                          cidx >= 0 && cidx < crange;
                unsigned long long w = cbitmap[in ? cidx >> 6 : 0];
                m[j] = in && ((w >> (cidx & 63)) & 1ull);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                m[j] = (ds[j] < q3date) &&
                       d_keyset_probe(ckeys, ccap, ck[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!m[j]) continue;
            int64_t idx = ok[j] - mino;
            if (idx < 0 || idx >= range) continue;
            atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
            q3_rec r;
            r.rev = Q3_REV_UNMATCHED; /* see k_ord_insert_direct */
            r.pl = (unsigned long long)(uint32_t)ds[j] |
                   ((unsigned long long)(uint32_t)prio[j] << 32);
            grec[idx] = r; /* one 16-B store on one line */
        }
    }
    /* tail rows */
    if ((o.n & 3) && blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t i = nq * 4; i < o.n; i++) {
            if (!(o.o_orderdate[i] < q3date)) continue;
            bool pass;
            int64_t ckv = o.o_custkey[i];
            if (cbitmap) {
                int64_t cidx = ckv - cmin;
                pass = cidx >= 0 && cidx < crange &&
                       ((cbitmap[cidx >> 6] >> (cidx & 63)) & 1ull);
            } else {
                pass = d_keyset_probe(ckeys, ccap, ckv);
            }
            if (!pass) continue;
            int64_t idx = o.o_orderkey[i] - mino;
            if (idx < 0 || idx >= range) continue;
            atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
            q3_rec r;
            r.rev = Q3_REV_UNMATCHED;
            r.pl = (unsigned long long)(uint32_t)o.o_orderdate[i] |
                   ((unsigned long long)(uint32_t)o.o_shippriority[i] << 32);
            grec[idx] = r;
        }
    }
}

__global__ void k_ord_insert_direct(const otbx_orders_dev o,
                                    const int64_t *__restrict__ cand,
                                    const int64_t *__restrict__ ncand_p,
                                    int64_t mino, int64_t range,
                                    unsigned long long *bitmap,
                                    q3_rec *grec)
{
    int64_t n = *ncand_p;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < n;
         ci += stride) {
        int64_t i = cand[ci];
        int64_t idx = o.o_orderkey[i] - mino;
        if (idx < 0 || idx >= range)
            continue; /* outside this grace pass's key sub-range */
        atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
        q3_rec r;
        r.rev = Q3_REV_UNMATCHED; /* survivor-slot reset: replaces a
                      * whole-range memset (orderkeys unique -> one writer
                      * per idx; unset-bit entries are never read:
                      * compaction is bitmap-authoritative) */
        r.pl = (unsigned long long)(uint32_t)o.o_orderdate[i] |
               ((unsigned long long)(uint32_t)o.o_shippriority[i] << 32);
        grec[idx] = r;
    }
}

/* fully fused direct-path probe: scan + bitmap filter + payload read +
 * revenue accumulation in ONE pass. The candidate-list split exists for the
 * HASH path's divergent chain walk; on the direct path the "probe" is a
 * single clustered table read + one atomic, so materializing candidates
 * (write + re-read + key re-gather) only costs bandwidth. */
template <bool K32>
__global__ void k_q3_scan_probe_agg_direct(const otbx_lineitem_dev l,
                                           int32_t q3date, int64_t mino,
                                           int64_t range,
                                           const unsigned long long *__restrict__ bitmap,
                                           q3_rec *__restrict__ grec,
                                           unsigned long long *__restrict__ nhits)
{
    int64_t nq = l.n / 4;
    const int4 *sd4 = (const int4 *)l.l_shipdate;
    const longlong2 *ok2 = (const longlong2 *)l.l_orderkey;
    /* K32: the staged compact-key cache (otbx.h l_orderkey32) halves the
     * orderkey stream — 12 → 8 B/row on this kernel's dominant traffic */
    const int4 *ok4 = (const int4 *)l.l_orderkey32;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long myhits = 0;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq;
         q += stride) {
        /* plain loads: nt loads here measured neutral-to-worse (r5 vs r4,
         * profiles/r5_q3.json) — the streams already miss L2 and the nt
         * hint bought nothing */
        int4 d = sd4[q];
        int64_t ky[4];
        if (K32) {
            int4 kk = ok4[q];
            ky[0] = kk.x; ky[1] = kk.y; ky[2] = kk.z; ky[3] = kk.w;
        } else {
            longlong2 ka = ok2[2 * q], kb = ok2[2 * q + 1];
            ky[0] = ka.x; ky[1] = ka.y; ky[2] = kb.x; ky[3] = kb.y;
        }
        int32_t ds[4] = {d.x, d.y, d.z, d.w};
        bool m[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int64_t idx = ky[j] - mino;
            bool pass = (ds[j] > q3date) && idx >= 0 && idx < range;
            int64_t bidx = pass ? idx : 0;
            unsigned long long w = bitmap[bidx >> 6];
            m[j] = pass && ((w >> (bidx & 63)) & 1ull);
        }
        /* in-lane run combine: lineitem rows arrive clustered by orderkey
         * (~4 rows/order), so a lane's quad usually hits one or two keys —
         * summing runs locally cuts the f64 atomics (same-address atomics
         * serialize) several-fold */
        int64_t run_key = 0;
        double run_sum = 0.0;
        bool run_valid = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!m[j]) /* the bitmap is the presence authority: any
                        * payload value, 0 included, is a real order */
                continue;
            myhits++;
            int64_t i = q * 4 + j;
            double rev = l.l_extendedprice[i] * (1.0 - l.l_discount[i]);
            if (run_valid && ky[j] == run_key) {
                run_sum += rev;
            } else {
                if (run_valid)
                    atomicAdd(&grec[run_key - mino].rev, q3_pos0(run_sum));
                run_key = ky[j];
                run_sum = rev;
                run_valid = true;
            }
        }
        if (run_valid)
            atomicAdd(&grec[run_key - mino].rev, q3_pos0(run_sum));
    }
    /* tail rows */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t i = nq * 4; i < l.n; i++) {
            int64_t idx = l.l_orderkey[i] - mino;
            if (!(l.l_shipdate[i] > q3date) || idx < 0 || idx >= range)
                continue;
            if (!((bitmap[idx >> 6] >> (idx & 63)) & 1ull))
                continue;
            myhits++;
            double rev = l.l_extendedprice[i] * (1.0 - l.l_discount[i]);
            atomicAdd(&grec[idx].rev, q3_pos0(rev));
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
        myhits += __shfl_down(myhits, off, WAVE);
    if ((threadIdx.x % WAVE) == 0 && myhits)
        atomicAdd(nhits, myhits);
}

/* Word-granular tile compaction (A/B vs k_q3_compact_tile): each thread
 * owns one 64-entry bitmap word per sweep — the bitmap is read ONCE (the
 * quad-granular tile reads each word 16x) and the per-entry sweep
 * machinery collapses to a popcount + a short set-bit loop. Tile = 1024
 * words = 65536 entries; stage cap 32768 survivor ids (64 KB LDS) with a
 * per-thread direct-write fallback for denser-than-50% tiles. */
#define Q3CW (1024 * 64)
#define Q3CW_STAGE 32768
__global__ __launch_bounds__(1024) void k_q3_compact_word(
    const q3_rec *__restrict__ grec,
    const unsigned long long *__restrict__ bitmap, int64_t range,
    int64_t mino, otbx_q3_group *out, int64_t cap_out, int64_t *ngroups)
{
    __shared__ uint16_t stage[Q3CW_STAGE];
    __shared__ int wtot[16];
    __shared__ int woff[16];
    __shared__ int tot_s;
    __shared__ long long gbase;
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int64_t nwords = (range + 63) / 64;
    int64_t ntiles = (nwords + 1023) / 1024;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t w0 = t * 1024 + threadIdx.x;     /* my bitmap word */
        int64_t tl = t * (int64_t)Q3CW;          /* tile base entry */
        unsigned long long w = w0 < nwords ? bitmap[w0] : 0ull;
        /* drop bits past range in the last word */
        if (w0 == nwords - 1 && (range & 63))
            w &= (1ull << (range & 63)) - 1ull;
        /* count survivors in my word (q3_matched drops build rows that no
         * lineitem hit) */
        int64_t base_e = w0 * 64;
        int mycnt = 0;
        unsigned long long wm = w;
        unsigned long long keep = 0;
        while (wm) {
            int b = __builtin_ctzll(wm);
            wm &= wm - 1;
            if (q3_matched(grec[base_e + b].rev)) {
                keep |= 1ull << b;
                mycnt++;
            }
        }
        int incl = mycnt;
        for (int off = 1; off < WAVE; off <<= 1) {
            int up = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += up;
        }
        if (lane == WAVE - 1) wtot[wid] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            int acc = 0;
            for (int ww = 0; ww < 16; ww++) {
                woff[ww] = acc;
                acc += wtot[ww];
            }
            tot_s = acc;
            gbase = acc ? (long long)atomicAdd((unsigned long long *)ngroups,
                                               (unsigned long long)acc)
                        : 0;
        }
        __syncthreads();
        int pos = woff[wid] + incl - mycnt;
        int tot = tot_s;
        if (tot <= Q3CW_STAGE) {
            unsigned long long km = keep;
            while (km) {
                int b = __builtin_ctzll(km);
                km &= km - 1;
                stage[pos++] = (uint16_t)(base_e + b - tl);
            }
            __syncthreads();
            for (int p = threadIdx.x; p < tot; p += blockDim.x) {
                int64_t gp = gbase + p;
                if (gp >= cap_out) continue;
                int64_t i = tl + (int64_t)stage[p];
                q3_rec r = grec[i];
                out[gp].l_orderkey = mino + i;
                out[gp].revenue = r.rev;
                out[gp].o_orderdate = (int32_t)(r.pl & 0xffffffffull);
                out[gp].o_shippriority = (int32_t)(r.pl >> 32);
            }
        } else {
            /* dense tile (>50% survivors): direct per-thread writes */
            unsigned long long km = keep;
            int64_t gp = gbase + pos;
            while (km) {
                int b = __builtin_ctzll(km);
                km &= km - 1;
                if (gp < cap_out) {
                    int64_t i = base_e + b;
                    q3_rec r = grec[i];
                    out[gp].l_orderkey = mino + i;
                    out[gp].revenue = r.rev;
                    out[gp].o_orderdate = (int32_t)(r.pl & 0xffffffffull);
                    out[gp].o_shippriority = (int32_t)(r.pl >> 32);
                }
                gp++;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

static inline bool q3_compact_legacy(void)
{
    const char *e = getenv("OTBX_Q3_COMPACT_LEGACY");
    return e && atoi(e);
}

static inline bool q3_compact_tile_sel(void)
{
    const char *e = getenv("OTBX_Q3_COMPACT_TILE");
    return e && atoi(e);
}

/* Tile-staged variant (default; append_ab v6 pattern, profiles/
 * r2_append_ab.txt): per 8192-entry tile — count/rank via wave prefix sums,
 * ONE group-counter reservation per tile, tile-relative survivor ids staged
 * as u16 in LDS (16 KB, always fits), then a linear write-out with
 * consecutive lanes on consecutive out positions; the rtab slice is L2-hot
 * for the write-out's re-reads. The legacy kernel (below) re-reads its
 * whole 73 k-row block chunk from HBM on the emit pass and writes
 * per-thread runs. */
#define Q3CT 8192
__global__ __launch_bounds__(1024) void k_q3_compact_tile(
    const q3_rec *__restrict__ grec,
    const unsigned long long *__restrict__ bitmap, int64_t range,
    int64_t mino, otbx_q3_group *out, int64_t cap_out, int64_t *ngroups)
{
    __shared__ uint16_t stage[Q3CT];
    __shared__ int wtot[16];
    __shared__ int woff[16];
    __shared__ int sweepbase;
    __shared__ long long gbase;
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int64_t ntiles = (range + Q3CT - 1) / Q3CT;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t tl = t * (int64_t)Q3CT;
        int64_t th = tl + Q3CT < range ? tl + Q3CT : range;
        if (threadIdx.x == 0) sweepbase = 0;
        __syncthreads();
        for (int64_t s0 = tl; s0 < th; s0 += 4096) {
            int64_t r0 = s0 + 4 * (int64_t)threadIdx.x;
            bool m[4] = {false, false, false, false};
            int mycnt = 0;
            /* bitmap is the presence authority (records are NOT memset
             * per step; stale entries live at unset-bit positions);
             * q3_matched then drops build rows with no probe match (the
             * revenue VALUE says nothing: a group may sum to zero). The
             * record loads only run near set bits — most quads fast-skip. */
            if (r0 + 3 < range) {
                unsigned long long w = bitmap[r0 >> 6] >> (r0 & 63);
                if (w & 0xfull) {
                    /* one 16-B load per candidate record (rev+pl share the
                     * line anyway) instead of an 8-B stride-16 pick */
                    const v2d *gr2 = (const v2d *)&grec[r0];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        m[j] = ((w >> j) & 1ull) && q3_matched(gr2[j].x);
                        mycnt += m[j];
                    }
                }
            } else {
                for (int j = 0; j < 4 && r0 + j < range; j++) {
                    int64_t i = r0 + j;
                    m[j] = ((bitmap[i >> 6] >> (i & 63)) & 1ull) &&
                           q3_matched(grec[i].rev);
                    mycnt += m[j];
                }
            }
            int incl = mycnt;
            for (int off = 1; off < WAVE; off <<= 1) {
                int up = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl += up;
            }
            if (lane == WAVE - 1) wtot[wid] = incl;
            __syncthreads();
            if (threadIdx.x == 0) {
                int acc = sweepbase;
                for (int w = 0; w < 16; w++) {
                    woff[w] = acc;
                    acc += wtot[w];
                }
                sweepbase = acc;
            }
            __syncthreads();
            int pos = woff[wid] + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j]) stage[pos++] = (uint16_t)(r0 + j - tl);
            __syncthreads();
        }
        int tot = sweepbase;
        if (threadIdx.x == 0)
            gbase = tot ? (long long)atomicAdd((unsigned long long *)ngroups,
                                               (unsigned long long)tot)
                        : 0;
        __syncthreads();
        for (int p = threadIdx.x; p < tot; p += blockDim.x) {
            int64_t gp = gbase + p;
            if (gp >= cap_out) continue;
            int64_t i = tl + (int64_t)stage[p];
            q3_rec r = grec[i];
            out[gp].l_orderkey = mino + i;
            out[gp].revenue = r.rev;
            out[gp].o_orderdate = (int32_t)(r.pl & 0xffffffffull);
            out[gp].o_shippriority = (int32_t)(r.pl >> 32);
        }
        __syncthreads();
    }
}

__global__ void k_q3_compact_direct(const q3_rec *__restrict__ grec,
                                    const unsigned long long *__restrict__ bitmap,
                                    int64_t range, int64_t mino,
                                    otbx_q3_group *out, int64_t cap_out,
                                    int64_t *ngroups)
{
    /* legacy block-chunk compaction over the interleaved record table:
     * one 16-B load per entry on each pass. Presence comes from the bitmap
     * and "matched" from q3_matched, as in the other two kernels; the
     * whole-range memset only keeps the loads at unset-bit entries
     * defined. */
    int64_t per_block = (range + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < range ? lo + per_block : range;
    __shared__ int64_t tcnt[256];
    __shared__ int64_t tbase[257];
    int64_t my = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        my += ((bitmap[i >> 6] >> (i & 63)) & 1ull) &&
              q3_matched(grec[i].rev);
    tcnt[threadIdx.x] = my;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t tot = 0;
        for (int t = 0; t < (int)blockDim.x; t++) {
            tbase[t] = tot;
            tot += tcnt[t];
        }
        tbase[256] = tot ? (int64_t)atomicAdd((unsigned long long *)ngroups,
                                              (unsigned long long)tot)
                         : 0;
    }
    __syncthreads();
    int64_t pos = tbase[256] + tbase[threadIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        q3_rec r = grec[i];
        if (((bitmap[i >> 6] >> (i & 63)) & 1ull) && q3_matched(r.rev)) {
            if (pos < cap_out) {
                out[pos].l_orderkey = mino + i;
                out[pos].revenue = r.rev;
                out[pos].o_orderdate = (int32_t)(r.pl & 0xffffffffull);
                out[pos].o_shippriority = (int32_t)(r.pl >> 32);
            }
            pos++;
        }
    }
}

/* group table for the partial agg: slot {q3_kenc(okey) (EMPTY=0 claim via
 * CAS), date, prio, revenue (f64 atomic)} */
struct q3g_slot {
    unsigned long long okey;
    int32_t date;
    int32_t prio;
    double revenue;
};

__global__ void k_q3_scan_filter(const otbx_lineitem_dev l, int32_t q3date,
                                 const unsigned long long *__restrict__ bloom,
                                 int64_t bloom_words,
                                 int64_t *__restrict__ cand, int64_t *ncand)
{
    /* hash-fallback scan (sparse/wide key ranges): same 16-B-vector,
     * order-preserving structure as k_q3_scan_filter_direct, with the
     * hashed two-bit bloom test (nodeHashjoin.c:1862 analog) instead of the
     * dense bitmap; date-failing lanes read bloom word 0 (hot in L1). */
    const int BUF = 1024;
    __shared__ int64_t buf[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0; /* wave-uniform */
    int64_t nq = l.n / 4;
    const int4 *sd4 = (const int4 *)l.l_shipdate;
    const longlong2 *ok2 = (const longlong2 *)l.l_orderkey;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         q += stride) {
        bool m[4] = {false, false, false, false};
        int64_t r0 = q * 4;
        int mycnt = 0;
        if (q < nq) {
            int4 d = sd4[q];
            longlong2 ka = ok2[2 * q], kb = ok2[2 * q + 1];
            int32_t ds[4] = {d.x, d.y, d.z, d.w};
            int64_t ky[4] = {ka.x, ka.y, kb.x, kb.y};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bool pass = ds[j] > q3date;
                uint64_t h = otbx_splitmix64((uint64_t)ky[j]);
                uint64_t w =
                    pass ? ((h >> 12) & (uint64_t)(bloom_words - 1)) : 0;
                unsigned long long bits =
                    (1ull << (h & 63)) | (1ull << ((h >> 6) & 63));
                unsigned long long v = bloom[w];
                m[j] = pass && ((v & bits) == bits);
                mycnt += m[j];
            }
        }
        if (q == nq) { /* tail rows (l.n % 4) */
            for (int64_t i = nq * 4; i < l.n; i++) {
                int j = (int)(i - nq * 4);
                bool pass = l.l_shipdate[i] > q3date;
                uint64_t h = otbx_splitmix64((uint64_t)l.l_orderkey[i]);
                uint64_t w =
                    pass ? ((h >> 12) & (uint64_t)(bloom_words - 1)) : 0;
                unsigned long long bits =
                    (1ull << (h & 63)) | (1ull << ((h >> 6) & 63));
                m[j] = pass && ((bloom[w] & bits) == bits);
                mycnt += m[j];
            }
        }
        int incl = mycnt;
        for (int off = 1; off < WAVE; off <<= 1) {
            int up = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += up;
        }
        int tot = __shfl(incl, WAVE - 1, WAVE);
        if (tot) {
            if (nbuf + tot > BUF) {
                long long bpos = 0;
                if (lane == 0)
                    bpos = (long long)atomicAdd((unsigned long long *)ncand,
                                                (unsigned long long)nbuf);
                bpos = __shfl(bpos, 0, WAVE);
                for (int j = lane; j < nbuf; j += WAVE)
                    cand[bpos + j] = buf[wid][j];
                nbuf = 0;
            }
            int pos = nbuf + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j])
                    buf[wid][pos++] = r0 + j;
            nbuf += tot;
        }
        if (__all(q >= nq))
            break;
    }
    if (nbuf) {
        long long bpos = 0;
        if (lane == 0)
            bpos = (long long)atomicAdd((unsigned long long *)ncand,
                                        (unsigned long long)nbuf);
        bpos = __shfl(bpos, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE)
            cand[bpos + j] = buf[wid][j];
    }
}

/* probe phase B: dense over candidates, 4 per lane per batch so the key
 * gathers and first-slot table loads pipeline; the (rare) collision walk and
 * the group-table atomics stay scalar. The 16-B slot is read as one load
 * (okey | date,prio). */
__global__ void k_q3_probe_agg(const otbx_lineitem_dev l,
                               const int64_t *__restrict__ cand,
                               const int64_t *__restrict__ ncand_p,
                               const ord_slot *__restrict__ otab, int64_t ocap,
                               q3g_slot *gtab, int64_t gcap,
                               unsigned long long *__restrict__ nhits)
{
    const int B = 4;
    int64_t omask = ocap - 1, gmask = gcap - 1;
    int64_t n = *ncand_p;
    int64_t chunk = (int64_t)blockDim.x * B;
    int64_t stride = (int64_t)gridDim.x * chunk;
    unsigned long long myhits = 0;
    const ulonglong2 *otab2 = (const ulonglong2 *)otab;
    for (int64_t base = (int64_t)blockIdx.x * chunk; base < n; base += stride) {
        int64_t row[B], key[B], slot[B];
        ulonglong2 sv[B];
        bool valid[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            int64_t ci = base + (int64_t)k * blockDim.x + threadIdx.x;
            valid[k] = ci < n;
            row[k] = valid[k] ? cand[ci] : 0;
        }
#pragma unroll
        for (int k = 0; k < B; k++)
            key[k] = l.l_orderkey[row[k]];
        /* consecutive candidates sit in consecutive lanes (the scan append
         * preserves row order): only run-leading lanes load a table slot,
         * dupes take the leader's line via nearest-leader broadcast */
        int lane = (int)(threadIdx.x % WAVE);
        bool lead[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            int64_t kprev = __shfl_up((long long)key[k], 1, WAVE);
            lead[k] = (lane == 0) || key[k] != kprev;
            slot[k] = (int64_t)(d_hash_i64(key[k]) & (uint64_t)omask);
            sv[k] = otab2[lead[k] ? slot[k] : 0];
        }
        double ep[B], dc[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            ep[k] = l.l_extendedprice[row[k]];
            dc[k] = l.l_discount[row[k]];
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            /* leaders resolve their slot (collision walk); every lane then
             * broadcasts from its nearest leader */
            unsigned long long v = sv[k].x;
            unsigned long long payload = sv[k].y;
            unsigned long long ek = q3_kenc(key[k]);
            if (lead[k]) {
                int64_t s = slot[k];
                while (v != 0ull && v != ek) {
                    s = (s + 1) & omask;      /* rare: collision walk */
                    ulonglong2 sv2 = otab2[s];
                    v = sv2.x;
                    payload = sv2.y;
                }
            }
            /* an empty slot ends the walk and is never a hit, whatever the
             * probe key encodes to */
            int hitv = v != 0ull && v == ek;
            int lidx = lead[k] ? lane : -1;
            for (int st = 1; st < WAVE; st <<= 1) {
                int u = __shfl_up(lidx, st, WAVE);
                if (lane >= st && u > lidx) lidx = u;
            }
            int hit = __shfl(hitv, lidx, WAVE);
            payload = (unsigned long long)__shfl(
                (long long)payload, lidx, WAVE);
            if (!valid[k] || !hit)
                continue;
            myhits++;
            int32_t date = (int32_t)(payload & 0xffffffffull);
            int32_t prio = (int32_t)(payload >> 32);
            double rev = ep[k] * (1.0 - dc[k]);
            int64_t g = (int64_t)(d_hash_i64(key[k]) & (uint64_t)gmask);
            for (;;) {
                unsigned long long old = atomicCAS(&gtab[g].okey, 0ull, ek);
                if (old == 0ull) {
                    gtab[g].date = date;  /* winner writes payload; read by
                                           * the compact kernel (next launch) */
                    gtab[g].prio = prio;
                    break;
                }
                if (old == ek) break;
                g = (g + 1) & gmask;
            }
            atomicAdd(&gtab[g].revenue, rev);
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
        myhits += __shfl_down(myhits, off, WAVE);
    if ((threadIdx.x % WAVE) == 0 && myhits)
        atomicAdd(nhits, myhits);
}

__global__ void k_q3_compact(const q3g_slot *gtab, int64_t gcap,
                             otbx_q3_group *out, int64_t cap_out,
                             int64_t *ngroups)
{
    int64_t per_block = (gcap + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < gcap ? lo + per_block : gcap;
    __shared__ int64_t tcnt[256];
    __shared__ int64_t tbase[257];
    int64_t my = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        my += gtab[i].okey != 0ull;
    tcnt[threadIdx.x] = my;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t tot = 0;
        for (int t = 0; t < (int)blockDim.x; t++) {
            tbase[t] = tot;
            tot += tcnt[t];
        }
        tbase[256] = tot ? (int64_t)atomicAdd((unsigned long long *)ngroups,
                                              (unsigned long long)tot)
                         : 0;
    }
    __syncthreads();
    int64_t pos = tbase[256] + tbase[threadIdx.x];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (gtab[i].okey != 0ull) {
            if (pos < cap_out) {
                out[pos].l_orderkey = q3_kdec(gtab[i].okey);
                out[pos].revenue = gtab[i].revenue;
                out[pos].o_orderdate = gtab[i].date;
                out[pos].o_shippriority = gtab[i].prio;
            }
            pos++;
        }
    }
}

/* compact filtered customer keys for the broadcast build side */
/* tile-staged compaction (the append_ab v6 pattern, as k_q9_filter_tile):
 * the original bare wave_append ran at 48 GB/s — LINEAR in n, i.e. the
 * measured ~88-reservations/us single-counter cap, not a fixed cost
 * (profiles/r29 diagnosis) — which would put ~2.6 ms/step on every rank
 * of the multi-GPU Q3 broadcast path at SF100. */
#define FCT 8192
__global__ __launch_bounds__(1024) void k_filter_customer(
    const otbx_customer_dev c, uint8_t want, int64_t *__restrict__ out_keys,
    int64_t *nkeys)
{
    __shared__ int64_t stage[FCT];
    __shared__ int wtot[16];
    __shared__ int woff[16];
    __shared__ int sweepbase;
    __shared__ long long gbase;
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int64_t n = c.n;
    int64_t ntiles = (n + FCT - 1) / FCT;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t tl = t * (int64_t)FCT;
        int64_t th = tl + FCT < n ? tl + FCT : n;
        if (threadIdx.x == 0) sweepbase = 0;
        __syncthreads();
        for (int64_t s0 = tl; s0 < th; s0 += 4096) {
            int64_t r0 = s0 + 4 * (int64_t)threadIdx.x;
            bool m[4] = {false, false, false, false};
            int64_t ks[4];
            int mycnt = 0;
            if (r0 + 3 < n) {
                uchar4 sv = *(const uchar4 *)&c.c_mktsegment[r0];
                v2l ka = *(const v2l *)&c.c_custkey[r0];
                v2l kb = *(const v2l *)&c.c_custkey[r0 + 2];
                uint8_t ss[4] = {sv.x, sv.y, sv.z, sv.w};
                ks[0] = ka.x; ks[1] = ka.y; ks[2] = kb.x; ks[3] = kb.y;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    m[j] = ss[j] == want;
                    mycnt += m[j];
                }
            } else {
                for (int j = 0; j < 4 && r0 + j < n; j++) {
                    m[j] = c.c_mktsegment[r0 + j] == want;
                    ks[j] = c.c_custkey[r0 + j];
                    mycnt += m[j];
                }
            }
            int incl = mycnt;
            for (int off = 1; off < WAVE; off <<= 1) {
                int up = __shfl_up(incl, off, WAVE);
                if (lane >= off) incl += up;
            }
            if (lane == WAVE - 1) wtot[wid] = incl;
            __syncthreads();
            if (threadIdx.x == 0) {
                int acc = sweepbase;
                for (int w = 0; w < 16; w++) {
                    woff[w] = acc;
                    acc += wtot[w];
                }
                sweepbase = acc;
            }
            __syncthreads();
            int pos = woff[wid] + incl - mycnt;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m[j]) stage[pos++] = ks[j];
            __syncthreads();
        }
        int tot = sweepbase;
        if (threadIdx.x == 0)
            gbase = tot ? (long long)atomicAdd((unsigned long long *)nkeys,
                                               (unsigned long long)tot)
                        : 0;
        __syncthreads();
        for (int p = threadIdx.x; p < tot; p += blockDim.x)
            out_keys[gbase + p] = stage[p];
        __syncthreads();
    }
}

/* count rows passing {segment} / {date + customer-keyset} predicates —
 * sizes the right-fit hash tables before building (count-then-build). */
__global__ void k_count_customer_seg(const otbx_customer_dev c, uint8_t want,
                                     int64_t *count,
                                     unsigned long long *minkey,
                                     unsigned long long *maxkey)
{
    /* 4 rows/lane; custkey loaded UNCONDITIONALLY as 16-B vectors — at the
     * ~20 % segment selectivity the divergent conditional scalar gathers
     * of the first version touched most custkey lines anyway but with poor
     * MLP (measured 308 us for a 15 M-row table, ~8x its stream floor);
     * select-based min/max keeps the lane code branchless */
    int64_t nq = c.n / 4;
    const uchar4 *seg4 = (const uchar4 *)c.c_mktsegment;
    const v2l *ck2 = (const v2l *)c.c_custkey;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long my = 0, mymin = ~0ull >> 1, mymax = 0;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq;
         q += stride) {
        uchar4 sv = seg4[q];
        v2l ka = ck2[2 * q], kb = ck2[2 * q + 1];
        uint8_t ss[4] = {sv.x, sv.y, sv.z, sv.w};
        unsigned long long ks[4] = {
            (unsigned long long)ka.x, (unsigned long long)ka.y,
            (unsigned long long)kb.x, (unsigned long long)kb.y};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bool m = ss[j] == want;
            my += m;
            unsigned long long k = ks[j];
            mymin = (m && k < mymin) ? k : mymin;
            mymax = (m && k > mymax) ? k : mymax;
        }
    }
    /* tail */
    for (int64_t i = nq * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < c.n; i += stride) {
        if (c.c_mktsegment[i] == want) {
            my++;
            unsigned long long k = (unsigned long long)c.c_custkey[i];
            if (k < mymin) mymin = k;
            if (k > mymax) mymax = k;
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        my += __shfl_down(my, off, WAVE);
        unsigned long long mn = (unsigned long long)__shfl_down(
            (long long)mymin, off, WAVE);
        unsigned long long mx = (unsigned long long)__shfl_down(
            (long long)mymax, off, WAVE);
        if (mn < mymin) mymin = mn;
        if (mx > mymax) mymax = mx;
    }
    if ((threadIdx.x % WAVE) == 0) {
        if (my) atomicAdd((unsigned long long *)count, my);
        if (mymin != (~0ull >> 1)) atomicMin(minkey, mymin);
        if (mymax) atomicMax(maxkey, mymax);
    }
}

/* customer-key bitmap build (dense-custkey direct filter; 1-2 MB and
 * L2-resident vs a 64+ MB hashed keyset — same reasoning as the orderkey
 * direct path) */
__global__ void k_cust_bitmap_filter(const otbx_customer_dev c, uint8_t want,
                                     int64_t minc, unsigned long long *bitmap)
{
    /* 4 rows/lane, unconditional vector loads (see k_count_customer_seg) */
    int64_t nq = c.n / 4;
    const uchar4 *seg4 = (const uchar4 *)c.c_mktsegment;
    const v2l *ck2 = (const v2l *)c.c_custkey;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq;
         q += stride) {
        uchar4 sv = seg4[q];
        v2l ka = ck2[2 * q], kb = ck2[2 * q + 1];
        uint8_t ss[4] = {sv.x, sv.y, sv.z, sv.w};
        long long ks[4] = {ka.x, ka.y, kb.x, kb.y};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (ss[j] == want) {
                int64_t idx = ks[j] - minc;
                atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
            }
        }
    }
    for (int64_t i = nq * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < c.n; i += stride) {
        if (c.c_mktsegment[i] == want) {
            int64_t idx = c.c_custkey[i] - minc;
            atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
        }
    }
}

__global__ void k_cust_bitmap_keys(const int64_t *__restrict__ keys, int64_t n,
                                   int64_t minc, unsigned long long *bitmap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t idx = keys[i] - minc;
        atomicOr(&bitmap[idx >> 6], 1ull << (idx & 63));
    }
}

extern "C" {

otbx_status otbx_filter_customer(const otbx_customer_dev *c, uint8_t segment,
                                 int64_t *keys_out_dev, int64_t *nkeys_dev,
                                 void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(nkeys_dev, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(k_filter_customer, dim3(2048), dim3(1024),
                       0, s, *c, segment, keys_out_dev, nkeys_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

static int64_t fit_cap(int64_t n)
{
    return next_pow2_host(n < 16 ? 16 : (int64_t)(n / 0.7) + 1);
}

/* dense-direct path admission: key range the direct tables can cover.
 * Deterministic in the inputs so workspace_bytes and q3_partial agree. */
static int64_t direct_cap_for(int64_t norders)
{
    int64_t cap = next_pow2_host(norders < 16 ? 16 : norders) * 32;
    if (cap > OTBX_DIRECT_CAP_DEFAULT) cap = OTBX_DIRECT_CAP_DEFAULT;
    const char *env = getenv("OTBX_DIRECT_CAP"); /* test hook */
    if (env) {
        int64_t e = atoll(env);
        if (e >= (1 << 14) && e < cap) cap = e;
    }
    return cap;
}

otbx_status otbx_q3_workspace_bytes(int64_t ncust, int64_t norders,
                                    int64_t nlineitem, size_t *bytes)
{
    /* fixed region layout at worst-case caps; tables inside each region are
     * right-sized at run time (count-then-build) so only the live prefix is
     * cleared/touched */
    int64_t ccap_w = fit_cap(ncust), ocap_w = fit_cap(norders);
    int64_t dcap = direct_cap_for(norders);
    int64_t dcap_c = direct_cap_for(ncust);
    *bytes = 64 + (size_t)ccap_w * 8 + ((size_t)1 << 23) * 8 /* bloom */ +
             (size_t)ocap_w * sizeof(ord_slot) + (size_t)ocap_w * sizeof(q3g_slot) +
             (size_t)nlineitem * 8 /* lineitem candidates */ +
             (size_t)norders * 8 /* matched-orders candidate list */ +
             (size_t)(dcap / 8 + 64) /* direct orderkey bitmap */ +
             (size_t)dcap * 8 /* direct payload */ +
             (size_t)dcap * 8 /* direct revenue */ +
             (size_t)(dcap_c / 8 + 64) /* direct custkey bitmap */;
    return OTBX_OK;
}

static int64_t bloom_words_for(int64_t nkeys)
{
    int64_t w = next_pow2_host(nkeys / 2 < 16 ? 16 : nkeys / 2);
    if (w > (1ll << 23)) w = 1ll << 23; /* cap 64 MB (L3-resident) */
    return w;
}

otbx_status otbx_q3_partial(const otbx_customer_dev *c, const otbx_orders_dev *o,
                            const otbx_lineitem_dev *l,
                            const int64_t *cust_keys_dev, int64_t ncust_keys,
                            uint8_t segment, int32_t q3date, void *ws,
                            size_t ws_bytes, otbx_q3_group *groups_dev,
                            int64_t cap_groups, int64_t *ngroups_dev,
                            int64_t *stats_dev, void *stream, float *kernel_ms)
{
    int64_t ncust = cust_keys_dev ? ncust_keys : c->n;
    {
        size_t worst;
        otbx_q3_workspace_bytes(ncust, o->n, l->n, &worst);
        if (ws_bytes < worst) return OTBX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    /* fixed region offsets at worst-case caps */
    int64_t ccap_w = fit_cap(ncust), ocap_w = fit_cap(o->n);
    int64_t *hdr = (int64_t *)ws;  /* [0]=ncust_f [1]=nof [2]=li cand [3]=ord date cand */
    char *p0 = (char *)ws + 64;
    unsigned long long *ctab = (unsigned long long *)p0;
    unsigned long long *bloom = (unsigned long long *)(p0 + (size_t)ccap_w * 8);
    ord_slot *otab = (ord_slot *)((char *)bloom + ((size_t)1 << 23) * 8);
    q3g_slot *gtab = (q3g_slot *)((char *)otab + (size_t)ocap_w * sizeof(ord_slot));
    int64_t *cand_li = (int64_t *)((char *)gtab + (size_t)ocap_w * sizeof(q3g_slot));
    int64_t *cand_o2 = cand_li + l->n;
    int64_t dcap = direct_cap_for(o->n);
    int64_t dcap_c = direct_cap_for(ncust);
    unsigned long long *dbitmap = (unsigned long long *)(cand_o2 + o->n);
    q3_rec *dgrec = (q3_rec *)(dbitmap + dcap / 64 + 8); /* 16 B/entry —
        occupies exactly the former split ptab+rtab regions */
    unsigned long long *cbitmap_buf = (unsigned long long *)(dgrec + dcap);

    static int64_t *h_cnt = nullptr;        /* pinned host readback */
    if (!h_cnt)
        SCR_ALLOC_HOST(h_cnt, 8 * sizeof(int64_t));

    HIP_CHECK(hipMemsetAsync(hdr, 0, 64, s));
    HIP_CHECK(hipMemsetAsync(&hdr[4], 0x7f, 8, s)); /* min orderkey */
    HIP_CHECK(hipMemsetAsync(&hdr[6], 0x7f, 8, s)); /* min custkey  */
    HIP_CHECK(hipMemsetAsync(ngroups_dev, 0, sizeof(int64_t), s));
    unsigned long long *nhits = nullptr;
    if (stats_dev) {
        HIP_CHECK(hipMemsetAsync(stats_dev, 0, sizeof(int64_t), s));
        nhits = (unsigned long long *)stats_dev;
    } else {
        static unsigned long long *scratch = nullptr;
        if (!scratch)
            SCR_ALLOC_DEV(scratch, sizeof(unsigned long long));
        nhits = scratch;
    }

    hipEvent_t ev[5] = {};
    if (kernel_ms)
        for (int i = 0; i < 5; i++) HIP_CHECK(hipEventCreate(&ev[i]));
    if (kernel_ms) HIP_CHECK(hipEventRecord(ev[0], s));

    /* ---- phase 1: customer build side — count + key range, then either a
     * dense custkey BITMAP (direct filter, L2-resident) or the hashed
     * keyset fallback for wide key ranges */
    bool force_hash = getenv("OTBX_Q3_FORCE_HASH") != nullptr;
    int64_t ccap = 16, cmin = 0, crange = 0;
    unsigned long long *cbitmap = nullptr;
    if (cust_keys_dev) {
        if (ncust_keys > 0)
            hipLaunchKernelGGL(k_minmax_i64, dim3(grid_for(ncust_keys, 256)),
                               dim3(256), 0, s, cust_keys_dev, ncust_keys,
                               (unsigned long long *)&hdr[6],
                               (unsigned long long *)&hdr[7]);
    } else {
        /* 256-thread launch (measured: a 1024-thread variant tripled the
         * phase — r32 probe A/B; the ~0.3 ms residual stays a round-3 item) */
        hipLaunchKernelGGL(k_count_customer_seg, dim3(grid_for(c->n, 256)),
                           dim3(256), 0, s, *c, segment, &hdr[0],
                           (unsigned long long *)&hdr[6],
                           (unsigned long long *)&hdr[7]);
    }
    /* UNFILTERED orderkey range (staged zone-map metadata when available,
     * else a minmax kernel read back with the same sync): decides the
     * single-pass orders fast path below */
    if (o->n > 0 && !o->has_minmax)
        hipLaunchKernelGGL(k_minmax_i64, dim3(grid_for(o->n, 256)), dim3(256),
                           0, s, o->o_orderkey, o->n,
                           (unsigned long long *)&hdr[4],
                           (unsigned long long *)&hdr[5]);
    HIP_CHECK(hipMemcpyAsync(h_cnt, hdr, 64, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t ncust_f = cust_keys_dev ? ncust_keys : h_cnt[0];
    cmin = h_cnt[6];
    crange = key_range(h_cnt[6], h_cnt[7]);
    bool cust_direct = ncust_f > 0 && crange > 0 && crange <= dcap_c &&
                       !force_hash;
    if (cust_direct) {
        cbitmap = cbitmap_buf;
        HIP_CHECK(hipMemsetAsync(cbitmap, 0, (size_t)(crange / 64 + 8) * 8, s));
        if (cust_keys_dev)
            hipLaunchKernelGGL(k_cust_bitmap_keys,
                               dim3(grid_for(ncust_keys, 256)), dim3(256), 0, s,
                               cust_keys_dev, ncust_keys, cmin, cbitmap);
        else
            hipLaunchKernelGGL(k_cust_bitmap_filter, dim3(grid_for(c->n, 256)),
                               dim3(256), 0, s, *c, segment, cmin, cbitmap);
    } else {
        ccap = fit_cap(ncust_f); /* ≤ the ccap_w region: ncust_f ≤ ncust
                                  * (an empty set used to get fit_cap(16)
                                  * = 32 slots in a 16-slot region) */
        HIP_CHECK(hipMemsetAsync(ctab, 0, (size_t)ccap * 8, s));
        if (cust_keys_dev) {
            if (ncust_keys > 0)
                hipLaunchKernelGGL(k_keyset_build,
                                   dim3(grid_for(ncust_keys, 256)), dim3(256),
                                   0, s, cust_keys_dev, ncust_keys, ctab, ccap);
        } else {
            hipLaunchKernelGGL(k_keyset_build_filter, dim3(grid_for(c->n, 256)),
                               dim3(256), 0, s, c->c_custkey, c->c_mktsegment,
                               segment, c->n, ctab, ccap);
        }
    }
    if (kernel_ms) HIP_CHECK(hipEventRecord(ev[1], s));

    /* ---- phase 2 FAST PATH: when the unfiltered orderkey range (minmax
     * overlapped with phase 1) already fits one direct table, the date
     * qual + customer filter writes the bitmap/payload table in ONE pass —
     * no candidate list, no separate insert, no second host sync. */
    int64_t mino_all = o->has_minmax ? o->okey_min : h_cnt[4];
    int64_t range_all =
        o->n > 0 ? key_range(mino_all, o->has_minmax ? o->okey_max : h_cnt[5])
                 : 0;
    if (o->n > 0 && range_all > 0 && range_all <= dcap && !force_hash) {
        HIP_CHECK(hipMemsetAsync(dbitmap, 0,
                                 (size_t)(range_all / 64 + 8) * 8, s));
        if (q3_compact_legacy()) {
            /* legacy compaction loads every record of the range, so it
             * keeps the full-range zeroing the default path skips */
            HIP_CHECK(hipMemsetAsync(dgrec, 0, (size_t)range_all * 16, s));
        }
        if (o->o_orderkey32 && o->o_custkey32)
            hipLaunchKernelGGL((k_ord_filter_insert_fused<true>),
                               dim3(grid_for(o->n / 4, 256)), dim3(256), 0, s,
                               *o, q3date, ctab, ccap, cbitmap, cmin, crange,
                               mino_all, range_all, dbitmap, dgrec);
        else
            hipLaunchKernelGGL((k_ord_filter_insert_fused<false>),
                               dim3(grid_for(o->n / 4, 256)), dim3(256), 0, s,
                               *o, q3date, ctab, ccap, cbitmap, cmin, crange,
                               mino_all, range_all, dbitmap, dgrec);
        if (kernel_ms) HIP_CHECK(hipEventRecord(ev[2], s));
        if (l->l_orderkey32)
            hipLaunchKernelGGL((k_q3_scan_probe_agg_direct<true>),
                               dim3(grid_for(l->n / 4, 256)), dim3(256), 0, s,
                               *l, q3date, mino_all, range_all, dbitmap,
                               dgrec, nhits);
        else
            hipLaunchKernelGGL((k_q3_scan_probe_agg_direct<false>),
                               dim3(grid_for(l->n / 4, 256)), dim3(256), 0, s,
                               *l, q3date, mino_all, range_all, dbitmap,
                               dgrec, nhits);
        if (kernel_ms) HIP_CHECK(hipEventRecord(ev[3], s));
        if (q3_compact_legacy())
            hipLaunchKernelGGL(k_q3_compact_direct,
                               dim3(grid_for(range_all, 256)), dim3(256), 0,
                               s, dgrec, dbitmap, range_all, mino_all,
                               groups_dev, cap_groups, ngroups_dev);
        else if (q3_compact_tile_sel())
            hipLaunchKernelGGL(k_q3_compact_tile, dim3(2048), dim3(1024), 0,
                               s, dgrec, dbitmap, range_all, mino_all,
                               groups_dev, cap_groups, ngroups_dev);
        else /* default: word-granular (A/B winner, profiles/r12_*) */
            hipLaunchKernelGGL(k_q3_compact_word, dim3(2048), dim3(1024), 0,
                               s, dgrec, dbitmap, range_all, mino_all,
                               groups_dev, cap_groups, ngroups_dev);
        if (kernel_ms) HIP_CHECK(hipEventRecord(ev[4], s));
        goto emit;
    }

    /* ---- phase 2: orders side, fused date qual + customer filter →
     * matched row-id list (exact count for the right-sized build) */
    HIP_CHECK(hipMemsetAsync(&hdr[4], 0x7f, 8, s)); /* reset matched minmax */
    HIP_CHECK(hipMemsetAsync(&hdr[5], 0, 8, s));
    hipLaunchKernelGGL(k_ord_filter_probe_fused, dim3(grid_for(o->n, 256)),
                       dim3(256), 0, s, *o, q3date, ctab, ccap, cbitmap, cmin,
                       crange, cand_o2, &hdr[1],
                       (unsigned long long *)&hdr[4],
                       (unsigned long long *)&hdr[5]);
    HIP_CHECK(hipMemcpyAsync(h_cnt, hdr, 48, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    {
    int64_t nof = h_cnt[1];
    int64_t mino = h_cnt[4], maxo = h_cnt[5];
    int64_t range = key_range(mino, maxo);
    /* grace-style multi-pass (SURVEY §8f.4 analog): when the build side's
     * key range exceeds the direct tables' capacity, split it into ≤64
     * sub-ranges and run the direct pipeline once per sub-range — bounded
     * memory per pass, P passes over the probe stream (the reference's
     * batch spill tradeoff, nodeHash.c:1086). */
    int64_t npasses = 1;
    if (nof > 0 && range > dcap) {
        npasses = range / dcap + (range % dcap != 0);
        if (npasses > 64) npasses = 1; /* too sparse: hash path */
    }
    bool use_direct = nof > 0 && range > 0 &&
                      (range <= dcap || npasses > 1) && !force_hash;
    if (use_direct) {
        /* dense-orderkey direct path: bitmap filter + direct-addressed
         * payload/revenue tables preserve the probe stream's key locality;
         * npasses > 1 = the grace multi-pass over key sub-ranges */
        bool rec2 = false, rec3 = false;
        for (int64_t pass = 0; pass < npasses; pass++) {
            int64_t pmin = mino + pass * dcap;
            int64_t prange = range - pass * dcap < dcap ? range - pass * dcap
                                                        : dcap;
            HIP_CHECK(hipMemsetAsync(dbitmap, 0,
                                     (size_t)(prange / 64 + 8) * 8, s));
            if (q3_compact_legacy())
                HIP_CHECK(hipMemsetAsync(dgrec, 0, (size_t)prange * 16, s));
            if (pass > 0)
                HIP_CHECK(hipMemsetAsync(&hdr[2], 0, 8, s)); /* reset cands */
            hipLaunchKernelGGL(k_ord_insert_direct, dim3(grid_for(o->n, 256)),
                               dim3(256), 0, s, *o, cand_o2, &hdr[1], pmin,
                               prange, dbitmap, dgrec);
            if (kernel_ms && !rec2) {
                HIP_CHECK(hipEventRecord(ev[2], s));
                rec2 = true;
            }
            if (l->l_orderkey32)
                hipLaunchKernelGGL((k_q3_scan_probe_agg_direct<true>),
                                   dim3(grid_for(l->n / 4, 256)), dim3(256),
                                   0, s, *l, q3date, pmin, prange, dbitmap,
                                   dgrec, nhits);
            else
                hipLaunchKernelGGL((k_q3_scan_probe_agg_direct<false>),
                                   dim3(grid_for(l->n / 4, 256)), dim3(256),
                                   0, s, *l, q3date, pmin, prange, dbitmap,
                                   dgrec, nhits);
            if (kernel_ms && !rec3 && pass == npasses - 1) {
                HIP_CHECK(hipEventRecord(ev[3], s));
                rec3 = true;
            }
            if (q3_compact_legacy())
                hipLaunchKernelGGL(k_q3_compact_direct,
                                   dim3(grid_for(prange, 256)), dim3(256), 0,
                                   s, dgrec, dbitmap, prange, pmin,
                                   groups_dev, cap_groups, ngroups_dev);
            else if (q3_compact_tile_sel())
                hipLaunchKernelGGL(k_q3_compact_tile, dim3(2048), dim3(1024),
                                   0, s, dgrec, dbitmap, prange, pmin,
                                   groups_dev, cap_groups, ngroups_dev);
            else
                hipLaunchKernelGGL(k_q3_compact_word, dim3(2048), dim3(1024),
                                   0, s, dgrec, dbitmap, prange, pmin,
                                   groups_dev, cap_groups, ngroups_dev);
        }
        if (kernel_ms) HIP_CHECK(hipEventRecord(ev[4], s));
    } else {
        /* hash+bloom fallback (wide/sparse key ranges), with grace batching
         * when the build side exceeds the per-pass table budget: keys are
         * hash-partitioned over P passes, each pass builds a bounded table
         * and re-scans the probe stream (nodeHash.c:1086 batch tradeoff). */
        int64_t hash_budget = 1ll << 30;  /* slots per pass (~40 GB tables) */
        const char *hb = getenv("OTBX_Q3_HASH_BUDGET"); /* test hook */
        if (hb) {
            int64_t e = atoll(hb);
            if (e >= 1024) hash_budget = e;
        }
        uint32_t nph = (uint32_t)((nof + hash_budget - 1) / hash_budget);
        if (nph < 1) nph = 1;
        if (nph > 64) nph = 64;
        bool rec2 = false, rec3 = false;
        for (uint32_t pass = 0; pass < nph; pass++) {
            int64_t nof_p = nof;
            if (nph > 1) {
                HIP_CHECK(hipMemsetAsync(&hdr[3], 0, 8, s));
                hipLaunchKernelGGL(k_ord_count_pass, dim3(grid_for(o->n, 256)),
                                   dim3(256), 0, s, *o, cand_o2, &hdr[1], pass,
                                   nph, &hdr[3]);
                HIP_CHECK(hipMemcpyAsync(h_cnt + 3, hdr + 3, 8,
                                         hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                nof_p = h_cnt[3];
                if (nof_p == 0)
                    continue;
                HIP_CHECK(hipMemsetAsync(&hdr[2], 0, 8, s)); /* reset cands */
            }
            int64_t ocap = fit_cap(nof_p), gcap = ocap;
            int64_t bwords = bloom_words_for(nof_p);
            HIP_CHECK(hipMemsetAsync(bloom, 0, (size_t)bwords * 8, s));
            HIP_CHECK(hipMemsetAsync(otab, 0, (size_t)ocap * sizeof(ord_slot), s));
            HIP_CHECK(hipMemsetAsync(gtab, 0, (size_t)gcap * sizeof(q3g_slot), s));
            hipLaunchKernelGGL(k_ord_insert, dim3(grid_for(o->n, 256)),
                               dim3(256), 0, s, *o, cand_o2, &hdr[1], otab,
                               ocap, bloom, bwords, pass, nph);
            if (kernel_ms && !rec2) {
                HIP_CHECK(hipEventRecord(ev[2], s));
                rec2 = true;
            }
            /* lineitem scan+filter (compacted candidates), dense probe +
             * partial agg */
            hipLaunchKernelGGL(k_q3_scan_filter, dim3(grid_for(l->n, 256)),
                               dim3(256), 0, s, *l, q3date, bloom, bwords,
                               cand_li, &hdr[2]);
            hipLaunchKernelGGL(k_q3_probe_agg, dim3(grid_for(l->n, 256)),
                               dim3(256), 0, s, *l, cand_li, &hdr[2], otab,
                               ocap, gtab, gcap, nhits);
            if (kernel_ms && !rec3 && pass == nph - 1) {
                HIP_CHECK(hipEventRecord(ev[3], s));
                rec3 = true;
            }
            /* compact this pass's groups (append) */
            hipLaunchKernelGGL(k_q3_compact, dim3(grid_for(gcap, 256)),
                               dim3(256), 0, s, gtab, gcap, groups_dev,
                               cap_groups, ngroups_dev);
        }
        if (kernel_ms) HIP_CHECK(hipEventRecord(ev[4], s));
    }
    }
emit:
    HIP_CHECK(hipGetLastError());
    if (kernel_ms) {
        HIP_CHECK(hipEventSynchronize(ev[4]));
        for (int i = 0; i < 4; i++)
            HIP_CHECK(hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]));
        for (int i = 0; i < 5; i++) HIP_CHECK(hipEventDestroy(ev[i]));
    }
    return OTBX_OK;
}

/* ---- top-k by revenue: bit-pattern histogram selection ----
 * ss_norm_f64 (otbx_sortkey.h) maps a double to bits that compare as the
 * doubles do, negative revenue and -0.0 included, so its top 14 bits
 * (sign+exp+mantissa head) give 16384 monotonic bins; select the threshold
 * bin from the suffix sum, collect candidates ≥ threshold. */

__device__ __forceinline__ uint32_t rev_bin(double r)
{
    return (uint32_t)(ss_norm_f64(r) >> 50);
}

__global__ void k_topk_hist(const otbx_q3_group *__restrict__ g, int64_t n,
                            uint32_t *hist)
{
    /* per-block LDS histogram: the global bins are few and hot (revenues
     * cluster in a couple of octaves), device-atomic contention would
     * serialize — accumulate in LDS, flush nonzero bins once per block */
    __shared__ uint32_t lh[16384];
    for (int i = threadIdx.x; i < 16384; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        atomicAdd(&lh[rev_bin(g[i].revenue)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < 16384; i += blockDim.x) {
        uint32_t v = lh[i];
        if (v)
            atomicAdd(&hist[i], v);
    }
}

__global__ void k_topk_collect(const otbx_q3_group *__restrict__ g, int64_t n,
                               uint32_t thr_bin, otbx_q3_group *out,
                               int64_t cap, int64_t *ncand)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        bool m = rev_bin(g[i].revenue) >= thr_bin;
        int64_t pos = wave_append(ncand, m);
        if (m && pos < cap)
            out[pos] = g[i];
    }
}

extern "C" otbx_status otbx_topk_by_revenue(const otbx_q3_group *groups,
                                            int64_t n, int64_t k,
                                            otbx_q3_group *cand, int64_t cap,
                                            int64_t *ncand_dev, uint32_t *hist,
                                            void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(hist, 0, 16384 * 4, s));
    HIP_CHECK(hipMemsetAsync(ncand_dev, 0, 8, s));
    if (n <= 0) return OTBX_OK;
    hipLaunchKernelGGL(k_topk_hist, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       groups, n, hist);
    static uint32_t *h_hist = nullptr;
    if (!h_hist)
        SCR_ALLOC_HOST(h_hist, 16384 * 4);
    HIP_CHECK(hipMemcpyAsync(h_hist, hist, 16384 * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int64_t cum = 0;
    uint32_t thr = 0;
    for (int b = 16383; b >= 0; b--) {
        cum += h_hist[b];
        if (cum >= k) { thr = (uint32_t)b; break; }
    }
    hipLaunchKernelGGL(k_topk_collect, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       groups, n, thr, cand, cap, ncand_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

__device__ __forceinline__ bool d_nk_rownull(const otbx_keyset &ks, int64_t i)
{
    for (int c = 0; c < ks.nkeys; c++)
        if (ks.nulls[c] && ks.nulls[c][i])
            return true;
    return false;
}

__device__ __forceinline__ uint64_t d_nk_hash(const otbx_keyset &ks,
                                              int64_t i)
{
    uint64_t h = 0;
    for (int c = 0; c < ks.nkeys; c++) {
        h = (h << 1) | (h >> 63);
        bool isnull = ks.nulls[c] && ks.nulls[c][i];
        h ^= isnull ? (0x9e3779b97f4a7c15ull + (uint64_t)c)
                    : d_hash_i64(ks.keys[c][i]);
    }
    return h;
}

__device__ __forceinline__ bool d_nk_row_eq(const otbx_keyset &ks, int64_t a,
                                            int64_t b)
{
    for (int c = 0; c < ks.nkeys; c++) {
        bool na = ks.nulls[c] && ks.nulls[c][a];
        bool nb = ks.nulls[c] && ks.nulls[c][b];
        if (na != nb) return false;
        if (!na && ks.keys[c][a] != ks.keys[c][b]) return false;
    }
    return true;
}

__device__ __forceinline__ bool d_nk_match(const otbx_keyset &bks, int64_t b,
                                           const otbx_keyset &pks, int64_t p)
{
    for (int c = 0; c < bks.nkeys; c++)
        if (bks.keys[c][b] != pks.keys[c][p])
            return false;
    return true;
}


/* Distinct-group estimator for the generality-tier aggregates: samples
 * AGG_SAMPLE rows' COMBINED group hashes (d_nk_hash over the keyset view
 * of the op's columns — any group-consistent hash estimates group
 * cardinality) into a small exact table, then the 1-key path's birthday
 * formula (see otbx_agg_i64). Right-sizing the open-addressing tables is
 * the same lever that took the 1-key aggregate from 1.9 to 20+ Grows/s:
 * a full-n table is both probe-collision-heavy and init/compact-heavy. */
__global__ void k_nk_sample_hash(const otbx_keyset ks, int64_t n,
                                 int64_t *__restrict__ stab,
                                 unsigned long long *out2)
{
    int64_t stride_n = n > AGG_SAMPLE ? n / AGG_SAMPLE : 1;
    unsigned long long mynew = 0, myproc = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         j < AGG_SAMPLE; j += stride) {
        int64_t i = j * stride_n;
        if (i >= n) break;
        myproc++;
        int64_t k = (int64_t)d_nk_hash(ks, i);
        if (k == AGG_EMPTY) k ^= 1; /* sentinel remap (1-in-2^64 case) */
        int64_t pos = (int64_t)((uint64_t)k & (uint64_t)(AGG_SCAP - 1));
        for (;;) {
            long long cur = __hip_atomic_load(
                (long long *)&stab[pos], __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            if (cur == k) break;
            if (cur == AGG_EMPTY) {
                long long old = atomicCAS((unsigned long long *)&stab[pos],
                                          (unsigned long long)AGG_EMPTY,
                                          (unsigned long long)k);
                if (old == AGG_EMPTY) {
                    mynew++;
                    break;
                }
                if (old == k) break;
                continue;
            }
            pos = (pos + 1) & (AGG_SCAP - 1);
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        mynew += __shfl_down(mynew, off, WAVE);
        myproc += __shfl_down(myproc, off, WAVE);
    }
    if ((threadIdx.x % WAVE) == 0 && (mynew | myproc)) {
        atomicAdd(&out2[0], mynew);
        atomicAdd(&out2[1], myproc);
    }
}

/* returns the estimated distinct-group count (<= n); stab is an
 * AGG_SCAP-entry device scratch region; synchronous (reads the counters
 * back), matching the 1-key aggregate's estimator step */
static int64_t nk_estimate_groups(const otbx_keyset &ks, int64_t n,
                                  int64_t *stab, hipStream_t s)
{
    static unsigned long long *d_ds = nullptr;
    static unsigned long long *h_ds = nullptr;
    if (!d_ds) {
        if (otbx_scr_alloc((void **)&d_ds, 16, 0) != hipSuccess)
            return n;
        if (otbx_scr_alloc((void **)&h_ds, 16, 1) != hipSuccess)
            return n;
    }
    if (hipMemsetAsync(d_ds, 0, 16, s) != hipSuccess)
        return n;
    hipLaunchKernelGGL(k_fill_i64, dim3(grid_for(AGG_SCAP, 256)), dim3(256),
                       0, s, stab, AGG_SCAP, AGG_EMPTY);
    hipLaunchKernelGGL(k_nk_sample_hash, dim3(grid_for(AGG_SAMPLE, 256)),
                       dim3(256), 0, s, ks, n, stab, d_ds);
    if (hipMemcpyAsync(h_ds, d_ds, 16, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return n;
    double d = (double)h_ds[0], se = (double)h_ds[1];
    if (se < 1.0) se = 1.0;
    int64_t est;
    if (d < se / 2.0) {
        est = (int64_t)d;
    } else {
        double c = se - d;
        if (c < 1.0) c = 1.0;
        est = (int64_t)(se * se / (2.0 * c)); /* birthday */
    }
    if (est > n) est = n;
    if (est < 1) est = 1;
    return est;
}

#define NK_PROBE_BOUND 128

/* ---- claim-by-row-index aggregate table (agg2 / aggn; dec_slot below has
 * the same claim word with a 128-bit sum) ---- */
struct claim_slot {
    long long idx; /* claim word: -1 empty, else defining row index */
    unsigned long long count_star;
    unsigned long long count_v;
    double sum;
};

__global__ void k_claim_init(claim_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride) {
        tab[i].idx = -1;
        tab[i].count_star = 0;
        tab[i].count_v = 0;
        tab[i].sum = 0.0;
    }
}

/* the 4-byte abort flag and its pinned host mirror, shared by the three
 * aggregates (calls are serial per process — otbx.h) */
static otbx_status nk_abort_words(unsigned int **d_ab, unsigned int **h_ab)
{
    static unsigned int *d = nullptr;
    static unsigned int *h = nullptr;
    if (!d) {
        SCR_ALLOC_DEV(d, 4);
        SCR_ALLOC_HOST(h, 4);
    }
    *d_ab = d;
    *h_ab = h;
    return OTBX_OK;
}

/* Driver of the claim-slot aggregates. Estimator-sized attempt first (the
 * 1-key recipe: a full-n table is probe- and init/compact-heavy when
 * groups << rows), bounded by the abort flag; if the flag comes back set
 * (rare-tail overflow) everything is redone against the full cap-slot
 * table. init(c) and compact(c) launch over a c-slot table, build(c, abortf)
 * over the n rows; one stream sync per bounded attempt. stab is the
 * estimator's AGG_SCAP-entry sample table. */
template <typename Init, typename Build, typename Compact>
static otbx_status nk_bounded_agg(const otbx_keyset &ks, int64_t n,
                                  int64_t cap, int64_t *stab,
                                  int64_t *ngroups_dev, hipStream_t s,
                                  Init init, Build build, Compact compact)
{
    int64_t cap_use = cap;
    if (n >= AGGP_THRESHOLD) {
        int64_t est = nk_estimate_groups(ks, n, stab, s);
        int64_t cs = next_pow2_host(est * 8 < 4096 ? 4096 : est * 8);
        if (cs < cap) cap_use = cs;
    }
    const char *fcap = getenv("OTBX_NK_FORCE_CAP"); /* test hook: force a
        tiny first-attempt table so the abort+full-rerun path executes */
    if (fcap) {
        int64_t v = atoll(fcap);
        if (v >= 16 && v < cap)
            cap_use = next_pow2_host(v);
    }
    unsigned int *d_ab, *h_ab;
    otbx_status st = nk_abort_words(&d_ab, &h_ab);
    if (st != OTBX_OK)
        return st;
    for (int attempt = 0; attempt < 2; attempt++) {
        bool bounded = cap_use < cap;
        HIP_CHECK(hipMemsetAsync(ngroups_dev, 0, 8, s));
        HIP_CHECK(hipMemsetAsync(d_ab, 0, 4, s));
        init(cap_use);
        if (n > 0)
            build(cap_use, bounded ? d_ab : (unsigned int *)NULL);
        if (!bounded)
            break;
        HIP_CHECK(hipMemcpyAsync(h_ab, d_ab, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!*h_ab)
            break;
        cap_use = cap; /* rare-tail overflow: redo against the full table */
    }
    compact(cap_use);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

/* ================= extended joins (otbx_join_i64_ext / _i64x2) ===========
 * The HJ_* fill-state FSM (nodeHashjoin.c:139-144) on the generic open-
 * addressing join: inner/left/semi/anti/right/full, optionally on a
 * two-column key (multi-key hash combine nodeHash.c:2059 restated at
 * 64 bit — rotate-left-1 then xor; parity is on result sets).
 * Pair encoding (matches oracle/oracle.h ora_join_ext):
 *   match -> (bidx, pidx); left/full unmatched (or NULL-key) probe row and
 *   every semi/anti emission -> (-1, pidx); right/full unmatched (or
 *   NULL-key) build row -> (bidx, -1).
 * Same overflow contract as otbx_join_i64 (npairs = TRUE count).
 * Generality tier: correctness-first kernels, not the Q3 roofline path. */

struct joinx_slot {
    long long idx; /* claim word: -1 empty, else build row index */
    long long k1;
    long long k2;
};

__global__ void k_joinx_init(joinx_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride)
        tab[i].idx = -1;
}

__device__ __forceinline__ uint64_t d_jx_hash(int64_t k1, int64_t k2, int nk)
{
    uint64_t h = d_hash_i64(k1);
    if (nk == 2) {
        h = (h << 1) | (h >> 63); /* pg_rotate_left analog, nodeHash.c:2059 */
        h ^= d_hash_i64(k2);
    }
    return h;
}

__global__ void k_joinx_build(const int64_t *__restrict__ k1,
                              const uint8_t *__restrict__ n1,
                              const int64_t *__restrict__ k2,
                              const uint8_t *__restrict__ n2, int64_t nb,
                              int nk, joinx_slot *tab, int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nb;
         i += stride) {
        if ((n1 && n1[i]) || (nk == 2 && n2 && n2[i]))
            continue; /* NULL join key never enters the table
                       * (ExecHashGetHashValue nodeHash.c:2026) */
        int64_t a = k1[i], b = nk == 2 ? k2[i] : 0;
        int64_t s = (int64_t)(d_jx_hash(a, b, nk) & (uint64_t)mask);
        while (atomicCAS((unsigned long long *)&tab[s].idx,
                         (unsigned long long)(-1ll),
                         (unsigned long long)i) != (unsigned long long)(-1ll))
            s = (s + 1) & mask;
        tab[s].k1 = a; /* plain stores: read only by the NEXT launch */
        tab[s].k2 = b;
    }
}

/* probe: wave-uniform slot walk (as k_join_probe) + per-row match count;
 * the fill decisions are per-probe-row local except right/full, which mark
 * a matched bitmap for the trailing unmatched-build sweep
 * (ExecScanHashTableForUnmatched nodeHash.c:2322 analog). */
__global__ void k_joinx_probe(const joinx_slot *__restrict__ tab, int64_t cap,
                              const int64_t *__restrict__ k1,
                              const uint8_t *__restrict__ n1,
                              const int64_t *__restrict__ k2,
                              const uint8_t *__restrict__ n2, int64_t np,
                              int nk, int jt,
                              unsigned long long *__restrict__ mbitmap,
                              int64_t *__restrict__ out_b,
                              int64_t *__restrict__ out_p, int64_t cap_pairs,
                              int64_t *npairs)
{
    const bool emit_match = (jt == 0 || jt == 1 || jt == 4 || jt == 5);
    const bool fill_probe = (jt == 1 || jt == 3 || jt == 5); /* left/anti/full */
    const bool semi = jt == 2;
    const int BUF = 512;
    __shared__ int64_t bufb[256 / WAVE][BUF];
    __shared__ int64_t bufp[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0; /* wave-uniform */
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool inrange = i0 < np;
        bool rownull =
            inrange && ((n1 && n1[i0]) || (nk == 2 && n2 && n2[i0]));
        bool active = inrange && !rownull;
        int64_t a = k1[active ? i0 : 0];
        int64_t b = nk == 2 ? k2[active ? i0 : 0] : 0;
        int64_t s = (int64_t)(d_jx_hash(a, b, nk) & (uint64_t)mask);
        bool walking = active;
        int nmatch = 0;
        while (__any(walking)) {
            long long bidx = walking ? tab[s].idx : -1;
            bool have = walking && bidx >= 0;
            bool match =
                have && tab[s].k1 == a && (nk != 2 || tab[s].k2 == b);
            if (match) {
                nmatch++;
                if (mbitmap)
                    atomicOr(&mbitmap[bidx >> 6], 1ull << (bidx & 63));
                if (semi && nmatch > 1)
                    match = false; /* JOIN_SEMI: first match suffices
                                    * (nodeHashjoin.c:572); keep walking the
                                    * wave-converged loop but emit nothing */
            }
            bool emit = match && emit_match;
            unsigned long long mmask = __ballot(emit);
            int cnt = __popcll(mmask);
            if (cnt) {
                if (nbuf + cnt > BUF) {
                    long long base = 0;
                    if (lane == 0)
                        base = (long long)atomicAdd(
                            (unsigned long long *)npairs,
                            (unsigned long long)nbuf);
                    base = __shfl(base, 0, WAVE);
                    for (int j = lane; j < nbuf; j += WAVE) {
                        int64_t pos = base + j;
                        if (pos < cap_pairs) {
                            out_b[pos] = bufb[wid][j];
                            out_p[pos] = bufp[wid][j];
                        }
                    }
                    nbuf = 0;
                }
                if (emit) {
                    int rank = __popcll(mmask & ((1ull << lane) - 1ull));
                    bufb[wid][nbuf + rank] = bidx;
                    bufp[wid][nbuf + rank] = i0;
                }
                nbuf += cnt;
            }
            s = (s + 1) & mask;
            walking = have;
        }
        /* post-walk per-row fills (wave-converged point):
         *   left/full: no match or NULL-key row -> (-1, i0)
         *   anti:      same condition (NULL-key rows match nothing)
         *   semi:      >=1 match -> (-1, i0) */
        bool fill = false;
        if (inrange) {
            if (fill_probe)
                fill = rownull || nmatch == 0;
            else if (semi)
                fill = nmatch > 0;
        }
        unsigned long long fmask = __ballot(fill);
        int fcnt = __popcll(fmask);
        if (fcnt) {
            if (nbuf + fcnt > BUF) {
                long long base = 0;
                if (lane == 0)
                    base = (long long)atomicAdd((unsigned long long *)npairs,
                                                (unsigned long long)nbuf);
                base = __shfl(base, 0, WAVE);
                for (int j = lane; j < nbuf; j += WAVE) {
                    int64_t pos = base + j;
                    if (pos < cap_pairs) {
                        out_b[pos] = bufb[wid][j];
                        out_p[pos] = bufp[wid][j];
                    }
                }
                nbuf = 0;
            }
            if (fill) {
                int rank = __popcll(fmask & ((1ull << lane) - 1ull));
                bufb[wid][nbuf + rank] = -1;
                bufp[wid][nbuf + rank] = i0;
            }
            nbuf += fcnt;
        }
        if (__all(i0 >= np))
            break;
    }
    if (nbuf) {
        long long base = 0;
        if (lane == 0)
            base = (long long)atomicAdd((unsigned long long *)npairs,
                                        (unsigned long long)nbuf);
        base = __shfl(base, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE) {
            int64_t pos = base + j;
            if (pos < cap_pairs) {
                out_b[pos] = bufb[wid][j];
                out_p[pos] = bufp[wid][j];
            }
        }
    }
}

/* trailing sweep for right/full: NULL-key build rows never entered the
 * table, so they are unmatched by construction (HJ_FILL_INNER_TUPLES,
 * nodeHashjoin.c:693). */
__global__ void k_joinx_fill_build(const uint8_t *__restrict__ n1,
                                   const uint8_t *__restrict__ n2, int64_t nb,
                                   int nk,
                                   const unsigned long long *__restrict__ mbitmap,
                                   int64_t *__restrict__ out_b,
                                   int64_t *__restrict__ out_p,
                                   int64_t cap_pairs, int64_t *npairs)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool fill = false;
        if (i0 < nb) {
            bool rownull = (n1 && n1[i0]) || (nk == 2 && n2 && n2[i0]);
            fill = rownull || !((mbitmap[i0 >> 6] >> (i0 & 63)) & 1ull);
        }
        int64_t pos = wave_append(npairs, fill);
        if (fill && pos < cap_pairs) {
            out_b[pos] = i0;
            out_p[pos] = -1;
        }
        if (__all(i0 >= nb))
            break;
    }
}

/* ---- outer joins via the FAST inner join + mark-and-fill ----
 * For 1-key left/right/full with a large build side, the FSM table above
 * is dominated by random probes; instead: run otbx_join_i64 (dense-direct
 * or partitioned — 18-28 Gprobes/s), then mark matched probe/build rows
 * from the emitted pairs and sweep the unmatched (+ NULL-key) rows as
 * fills. Exactly the reference's split between the probe loop and
 * HJ_FILL_* states, just batched. Overflow caveat: if the TRUE pair count
 * exceeds cap_pairs the marks are incomplete and the fills with them —
 * the documented contract already requires the caller to re-run on
 * overflow (include/otbx.h). */
__global__ void k_joinx_mark_pairs(const int64_t *__restrict__ out_b,
                                   const int64_t *__restrict__ out_p,
                                   const int64_t *__restrict__ npairs_p,
                                   int64_t cap_pairs,
                                   unsigned long long *__restrict__ bbm,
                                   unsigned long long *__restrict__ pbm)
{
    int64_t n = *npairs_p;
    if (n > cap_pairs) n = cap_pairs;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (bbm) {
            int64_t b = out_b[i];
            atomicOr(&bbm[b >> 6], 1ull << (b & 63));
        }
        if (pbm) {
            int64_t p = out_p[i];
            atomicOr(&pbm[p >> 6], 1ull << (p & 63));
        }
    }
}

__global__ void k_joinx_fill_probe(const uint8_t *__restrict__ n1,
                                   const uint8_t *__restrict__ n2, int64_t np,
                                   int nk,
                                   const unsigned long long *__restrict__ pbm,
                                   int64_t *__restrict__ out_b,
                                   int64_t *__restrict__ out_p,
                                   int64_t cap_pairs, int64_t *npairs)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool fill = false;
        if (i0 < np) {
            bool rownull = (n1 && n1[i0]) || (nk == 2 && n2 && n2[i0]);
            fill = rownull || !((pbm[i0 >> 6] >> (i0 & 63)) & 1ull);
        }
        int64_t pos = wave_append(npairs, fill);
        if (fill && pos < cap_pairs) {
            out_b[pos] = -1;
            out_p[pos] = i0;
        }
        if (__all(i0 >= np))
            break;
    }
}

/* ================= two-key hash aggregate (otbx_agg_i64x2) ===============
 * Group identity (k1_isnull, k1, k2_isnull, k2) with NULL==NULL for
 * grouping (execGrouping.c:295,:525). Open-addressing slots claimed by row
 * index (no reserved key value); the claiming row's key columns define the
 * slot's group. Aggregates as otbx_agg_i64: count(*), count(v), sum(v)
 * (avg = sum/count; the GPU keeps [N, Sx] — include/otbx.h note). */

__global__ void k_agg2_build(const int64_t *__restrict__ k1,
                             const uint8_t *__restrict__ n1,
                             const int64_t *__restrict__ k2,
                             const uint8_t *__restrict__ n2,
                             const double *__restrict__ vals,
                             const uint8_t *__restrict__ vnull, int64_t n,
                             claim_slot *tab, int64_t cap,
                             unsigned int *abortf)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (abortf && __hip_atomic_load(abortf, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT))
            return; /* estimator-sized table overflowed: full-cap rerun */
        bool in1 = n1 && n1[i], in2 = n2 && n2[i];
        int64_t a = in1 ? 0 : k1[i], b = in2 ? 0 : k2[i];
        uint64_t h1 = in1 ? 0x9e3779b97f4a7c15ull : d_hash_i64(a);
        uint64_t h2 = in2 ? 0xc2b2ae3d27d4eb4full : d_hash_i64(b);
        uint64_t h = ((h1 << 1) | (h1 >> 63)) ^ h2;
        int64_t s = (int64_t)(h & (uint64_t)mask);
        int steps = 0;
        for (;;) {
            if (abortf && ++steps > NK_PROBE_BOUND) {
                atomicOr(abortf, 1u);
                break;
            }
            long long owner = tab[s].idx;
            if (owner < 0) {
                long long prev = (long long)atomicCAS(
                    (unsigned long long *)&tab[s].idx,
                    (unsigned long long)(-1ll), (unsigned long long)i);
                owner = prev == -1ll ? i : prev;
            }
            bool on1 = n1 && n1[owner], on2 = n2 && n2[owner];
            if (on1 == in1 && on2 == in2 && (in1 || k1[owner] == a) &&
                (in2 || k2[owner] == b))
                break;
            s = (s + 1) & mask;
        }
        if (abortf && steps > NK_PROBE_BOUND)
            continue; /* row unplaced; results discarded by the rerun */
        atomicAdd(&tab[s].count_star, 1ull);
        if (!(vnull && vnull[i])) {
            atomicAdd(&tab[s].count_v, 1ull);
            atomicAdd(&tab[s].sum, vals[i]);
        }
    }
}

__global__ void k_agg2_compact(const claim_slot *__restrict__ tab, int64_t cap,
                               const int64_t *__restrict__ k1,
                               const uint8_t *__restrict__ n1,
                               const int64_t *__restrict__ k2,
                               const uint8_t *__restrict__ n2,
                               otbx_agg2_group *__restrict__ out,
                               int64_t *ngroups)
{
    d_block_compact(
        cap, ngroups, [=](int64_t i) { return tab[i].idx >= 0; },
        [=](int64_t i, int64_t pos) {
            long long r = tab[i].idx;
            bool in1 = n1 && n1[r], in2 = n2 && n2[r];
            out[pos].key1 = in1 ? 0 : k1[r];
            out[pos].key2 = in2 ? 0 : k2[r];
            out[pos].count_star = (int64_t)tab[i].count_star;
            out[pos].count_v = (int64_t)tab[i].count_v;
            out[pos].sum_v = tab[i].sum;
            out[pos].key1_isnull = in1;
            out[pos].key2_isnull = in2;
            out[pos].sum_isnull = tab[i].count_v == 0;
            out[pos]._pad = 0;
        });
}

extern "C" {

static int64_t jx_cap_for(int64_t nb)
{
    return next_pow2_host(nb < 16 ? 16 : (int64_t)(nb / 0.7) + 1);
}

otbx_status otbx_join_ext_workspace_bytes(int64_t nb, int64_t np,
                                          size_t *bytes)
{
    size_t fsm = (size_t)jx_cap_for(nb) * sizeof(joinx_slot) +
                 (size_t)((nb + 63) / 64 + 1) * 8;
    *bytes = fsm;
    /* OTBX_JOINX_VIA_INNER=1 (env-gated, default off) additionally needs
     * the inner join's workspace plus matched bitmaps; the env affects
     * this sizing AND the route identically (the OTBX_Q9_BITMAP_BITS
     * convention) so default callers never over-allocate the ~30x larger
     * via-route scratch */
    const char *ov = getenv("OTBX_JOINX_VIA_INNER");
    if (ov && atoi(ov)) {
        size_t inner;
        otbx_join_i64_workspace_bytes(nb, np, &inner);
        size_t via = inner + (size_t)((nb + 63) / 64 + 1) * 8 +
                     (size_t)((np + 63) / 64 + 1) * 8;
        if (via > *bytes) *bytes = via;
    }
    return OTBX_OK;
}

static otbx_status joinx_run(const int64_t *bk1, const uint8_t *bn1,
                             const int64_t *bk2, const uint8_t *bn2,
                             int64_t nb, const int64_t *pk1,
                             const uint8_t *pn1, const int64_t *pk2,
                             const uint8_t *pn2, int64_t np, int nk,
                             int32_t jt, void *ws, size_t ws_bytes,
                             int64_t *out_b, int64_t *out_p,
                             int64_t cap_pairs, int64_t *npairs_dev,
                             void *stream)
{
    if (jt < 0 || jt > 5 || !ws || !npairs_dev)
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int64_t cap = jx_cap_for(nb);
    size_t need;
    otbx_join_ext_workspace_bytes(nb, np, &need);
    if (ws_bytes < need)
        return OTBX_ERR_INVALID;
    joinx_slot *tab = (joinx_slot *)ws;
    unsigned long long *mbitmap =
        (unsigned long long *)((char *)ws + (size_t)cap * sizeof(joinx_slot));
    const bool fill_build = (jt == 4 || jt == 5);

    /* 1-key left/right/full with a non-trivial build side: fast inner
     * join + mark-and-fill (see k_joinx_mark_pairs). Threshold overridable
     * for tests (OTBX_JOINX_VIA_INNER: 1 = always, 0 = never). */
    if (nk == 1 && (jt == 1 || jt == 4 || jt == 5)) {
        /* measured OFF by default: at both tested shapes the FSM table
         * beat this route (nb=15M/np=600M: 55.7 vs 143.9 ms; nb=10M/
         * np=100M: 16.8 vs 24.3 — profiles/r23 notes). The pair
         * materialization + mark-pass traffic outweighs the faster inner
         * probe. Kept behind OTBX_JOINX_VIA_INNER=1 (parity-tested) as
         * the starting point if a future shape favors it. */
        bool via = false;
        const char *ov = getenv("OTBX_JOINX_VIA_INNER");
        if (ov) via = atoi(ov) != 0;
        if (via) {
            size_t inner_ws;
            otbx_join_i64_workspace_bytes(nb, np, &inner_ws);
            unsigned long long *bbm =
                (unsigned long long *)((char *)ws + inner_ws);
            unsigned long long *pbm = bbm + ((nb + 63) / 64 + 1);
            size_t need_v = inner_ws + (size_t)((nb + 63) / 64 + 1) * 8 +
                            (size_t)((np + 63) / 64 + 1) * 8;
            if (ws_bytes < need_v)
                return OTBX_ERR_INVALID;
            otbx_status st = otbx_join_i64(bk1, bn1, nb, pk1, pn1, np, ws,
                                           inner_ws, out_b, out_p, cap_pairs,
                                           npairs_dev, stream);
            if (st != OTBX_OK)
                return st;
            const bool mark_b = (jt == 4 || jt == 5);
            const bool mark_p = (jt == 1 || jt == 5);
            if (mark_b)
                HIP_CHECK(hipMemsetAsync(bbm, 0,
                                         (size_t)((nb + 63) / 64 + 1) * 8,
                                         s));
            if (mark_p)
                HIP_CHECK(hipMemsetAsync(pbm, 0,
                                         (size_t)((np + 63) / 64 + 1) * 8,
                                         s));
            hipLaunchKernelGGL(k_joinx_mark_pairs,
                               dim3(grid_for(np, 256)), dim3(256), 0, s,
                               out_b, out_p, npairs_dev, cap_pairs,
                               mark_b ? bbm : NULL, mark_p ? pbm : NULL);
            if (mark_p && np > 0)
                hipLaunchKernelGGL(k_joinx_fill_probe,
                                   dim3(grid_for(np, 256)), dim3(256), 0, s,
                                   pn1, NULL, np, 1, pbm, out_b, out_p,
                                   cap_pairs, npairs_dev);
            if (mark_b && nb > 0)
                hipLaunchKernelGGL(k_joinx_fill_build,
                                   dim3(grid_for(nb, 256)), dim3(256), 0, s,
                                   bn1, NULL, nb, 1, bbm, out_b, out_p,
                                   cap_pairs, npairs_dev);
            HIP_CHECK(hipGetLastError());
            return OTBX_OK;
        }
    }

    HIP_CHECK(hipMemsetAsync(npairs_dev, 0, 8, s));
    hipLaunchKernelGGL(k_joinx_init, dim3(grid_for(cap, 256)), dim3(256), 0,
                       s, tab, cap);
    if (fill_build)
        HIP_CHECK(hipMemsetAsync(mbitmap, 0,
                                 (size_t)((nb + 63) / 64 + 1) * 8, s));
    if (nb > 0)
        hipLaunchKernelGGL(k_joinx_build, dim3(grid_for(nb, 256)), dim3(256),
                           0, s, bk1, bn1, bk2, bn2, nb, nk, tab, cap);
    if (np > 0)
        hipLaunchKernelGGL(k_joinx_probe, dim3(grid_for(np, 256)), dim3(256),
                           0, s, tab, cap, pk1, pn1, pk2, pn2, np, nk, jt,
                           fill_build ? mbitmap : NULL, out_b, out_p,
                           cap_pairs, npairs_dev);
    if (fill_build && nb > 0)
        hipLaunchKernelGGL(k_joinx_fill_build, dim3(grid_for(nb, 256)),
                           dim3(256), 0, s, bn1, bn2, nb, nk, mbitmap, out_b,
                           out_p, cap_pairs, npairs_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_join_i64_ext(const int64_t *bkeys, const uint8_t *bnull,
                              int64_t nb, const int64_t *pkeys,
                              const uint8_t *pnull, int64_t np,
                              int32_t join_type, void *ws, size_t ws_bytes,
                              int64_t *out_b, int64_t *out_p,
                              int64_t cap_pairs, int64_t *npairs_dev,
                              void *stream)
{
    return joinx_run(bkeys, bnull, NULL, NULL, nb, pkeys, pnull, NULL, NULL,
                     np, 1, join_type, ws, ws_bytes, out_b, out_p, cap_pairs,
                     npairs_dev, stream);
}

otbx_status otbx_join_i64x2(const int64_t *bk1, const uint8_t *bn1,
                            const int64_t *bk2, const uint8_t *bn2,
                            int64_t nb, const int64_t *pk1,
                            const uint8_t *pn1, const int64_t *pk2,
                            const uint8_t *pn2, int64_t np,
                            int32_t join_type, void *ws, size_t ws_bytes,
                            int64_t *out_b, int64_t *out_p, int64_t cap_pairs,
                            int64_t *npairs_dev, void *stream)
{
    /* an empty side may carry NULL columns (the otbx_sort_perm rule) */
    if ((nb > 0 && !bk2) || (np > 0 && !pk2))
        return OTBX_ERR_INVALID;
    return joinx_run(bk1, bn1, bk2, bn2, nb, pk1, pn1, pk2, pn2, np, 2,
                     join_type, ws, ws_bytes, out_b, out_p, cap_pairs,
                     npairs_dev, stream);
}

otbx_status otbx_agg_i64x2_workspace_bytes(int64_t n, size_t *bytes)
{
    /* full-cap table (the abort-fallback path) + the estimator's sample
     * table (AGG_SCAP i64 hashes) */
    *bytes = (size_t)jx_cap_for(n) * sizeof(claim_slot) +
             (size_t)AGG_SCAP * 8;
    return OTBX_OK;
}

otbx_status otbx_agg_i64x2(const int64_t *k1, const uint8_t *k1null,
                           const int64_t *k2, const uint8_t *k2null,
                           const double *vals, const uint8_t *val_null,
                           int64_t n, void *ws, size_t ws_bytes,
                           otbx_agg2_group *groups_dev, int64_t *ngroups_dev,
                           void *stream)
{
    if (!ws || !ngroups_dev || (n > 0 && (!k1 || !k2)))
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int64_t cap = jx_cap_for(n);
    size_t need;
    otbx_agg_i64x2_workspace_bytes(n, &need);
    if (ws_bytes < need)
        return OTBX_ERR_INVALID;
    claim_slot *tab = (claim_slot *)ws;
    int64_t *stab = (int64_t *)((char *)ws + (size_t)cap * sizeof(claim_slot));
    otbx_keyset ks;
    ks.nkeys = 2;
    ks.keys[0] = k1; ks.keys[1] = k2;
    ks.nulls[0] = k1null; ks.nulls[1] = k2null;
    return nk_bounded_agg(
        ks, n, cap, stab, ngroups_dev, s,
        [&](int64_t c) {
            hipLaunchKernelGGL(k_claim_init, dim3(grid_for(c, 256)),
                               dim3(256), 0, s, tab, c);
        },
        [&](int64_t c, unsigned int *abortf) {
            hipLaunchKernelGGL(k_agg2_build, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, k1, k1null, k2, k2null, vals,
                               val_null, n, tab, c, abortf);
        },
        [&](int64_t c) {
            hipLaunchKernelGGL(k_agg2_compact, dim3(grid_for(c, 256)),
                               dim3(256), 0, s, tab, c, k1, k1null, k2,
                               k2null, groups_dev, ngroups_dev);
        });
}

otbx_status otbx_build_q9recs(const otbx_lineitem_dev *l, void *recs_dev,
                              void *stream)
{
    if (!l || !recs_dev || !l->l_orderkey || !l->l_extendedprice ||
        !l->l_discount)
        return OTBX_ERR_INVALID;
    hipLaunchKernelGGL(k_q9_build_recs, dim3(grid_for(l->n, 256)), dim3(256),
                       0, (hipStream_t)stream, *l, (q9_rec *)recs_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ============ exact decimal aggregate (otbx_agg_i64_dec) ============
 * Int128AggState {N, sumX} semantics (numeric.c:5072, do_int128_accum
 * :4998, int8_avg_accum :5365): 128-bit two's-complement sum accumulated
 * with a carry-propagating pair of 64-bit atomics — lo += (u64)v returns
 * the old word, carry-out = (old + v) wrapped; hi += sign_extend(v) +
 * carry. Exact for any input (|sum| <= 2^126), bit-exact parity. */

struct dec_slot {
    long long idx; /* claim word: -1 empty, else defining row index */
    unsigned long long count_star;
    unsigned long long count_v;
    unsigned long long sum_lo;
    unsigned long long sum_hi; /* two's complement */
};

__global__ void k_dec_init(dec_slot *tab, int64_t cap)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
         i += stride) {
        tab[i].idx = -1;
        tab[i].count_star = 0;
        tab[i].count_v = 0;
        tab[i].sum_lo = 0;
        tab[i].sum_hi = 0;
    }
}

__global__ void k_dec_build(const int64_t *__restrict__ keys,
                            const uint8_t *__restrict__ knull,
                            const int64_t *__restrict__ vals,
                            const uint8_t *__restrict__ vnull, int64_t n,
                            dec_slot *tab, int64_t cap,
                            unsigned int *abortf)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (abortf && __hip_atomic_load(abortf, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT))
            return; /* estimator-sized table overflowed: full-cap rerun */
        bool kn = knull && knull[i];
        int64_t k = kn ? 0 : keys[i];
        uint64_t h = kn ? 0x9e3779b97f4a7c15ull : d_hash_i64(k);
        int64_t s = (int64_t)(h & (uint64_t)mask);
        int steps = 0;
        for (;;) {
            if (abortf && ++steps > NK_PROBE_BOUND) {
                atomicOr(abortf, 1u);
                break;
            }
            long long owner = tab[s].idx;
            if (owner < 0) {
                long long prev = (long long)atomicCAS(
                    (unsigned long long *)&tab[s].idx,
                    (unsigned long long)(-1ll), (unsigned long long)i);
                owner = prev == -1ll ? i : prev;
            }
            bool on = knull && knull[owner];
            if (on == kn && (kn || keys[owner] == k))
                break;
            s = (s + 1) & mask;
        }
        if (abortf && steps > NK_PROBE_BOUND)
            continue; /* row unplaced; results discarded by the rerun */
        atomicAdd(&tab[s].count_star, 1ull);
        if (!(vnull && vnull[i])) {
            int64_t v = vals[i];
            atomicAdd(&tab[s].count_v, 1ull);
            unsigned long long uv = (unsigned long long)v;
            unsigned long long old = atomicAdd(&tab[s].sum_lo, uv);
            unsigned long long nw = old + uv;
            long long hid = (v < 0 ? -1ll : 0ll) + (nw < old ? 1ll : 0ll);
            if (hid)
                atomicAdd(&tab[s].sum_hi, (unsigned long long)hid);
        }
    }
}

__global__ void k_dec_compact(const dec_slot *__restrict__ tab, int64_t cap,
                              const int64_t *__restrict__ keys,
                              const uint8_t *__restrict__ knull,
                              otbx_dec_group *__restrict__ out,
                              int64_t *ngroups)
{
    d_block_compact(
        cap, ngroups, [=](int64_t i) { return tab[i].idx >= 0; },
        [=](int64_t i, int64_t pos) {
            long long r = tab[i].idx;
            bool kn = knull && knull[r];
            out[pos].key = kn ? 0 : keys[r];
            out[pos].count_star = (int64_t)tab[i].count_star;
            out[pos].count_v = (int64_t)tab[i].count_v;
            out[pos].sum_hi = (int64_t)tab[i].sum_hi;
            out[pos].sum_lo = tab[i].sum_lo;
            out[pos].key_isnull = kn;
            out[pos].sum_isnull = tab[i].count_v == 0;
        });
}

extern "C" {

otbx_status otbx_agg_i64_dec_workspace_bytes(int64_t n, size_t *bytes)
{
    *bytes = (size_t)jx_cap_for(n) * sizeof(dec_slot) +
             (size_t)AGG_SCAP * 8; /* + estimator sample table */
    return OTBX_OK;
}

otbx_status otbx_agg_i64_dec(const int64_t *keys, const uint8_t *knull,
                             const int64_t *vals, const uint8_t *vnull,
                             int64_t n, void *ws, size_t ws_bytes,
                             otbx_dec_group *groups_dev, int64_t *ngroups_dev,
                             void *stream)
{
    if (!ws || !ngroups_dev || (n > 0 && (!keys || !vals)))
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int64_t cap = jx_cap_for(n);
    size_t need;
    otbx_agg_i64_dec_workspace_bytes(n, &need);
    if (ws_bytes < need)
        return OTBX_ERR_INVALID;
    dec_slot *tab = (dec_slot *)ws;
    int64_t *stab = (int64_t *)((char *)ws + (size_t)cap * sizeof(dec_slot));
    otbx_keyset ks;
    ks.nkeys = 1;
    ks.keys[0] = keys;
    ks.nulls[0] = knull;
    return nk_bounded_agg(
        ks, n, cap, stab, ngroups_dev, s,
        [&](int64_t c) {
            hipLaunchKernelGGL(k_dec_init, dim3(grid_for(c, 256)), dim3(256),
                               0, s, tab, c);
        },
        [&](int64_t c, unsigned int *abortf) {
            hipLaunchKernelGGL(k_dec_build, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, keys, knull, vals, vnull, n,
                               tab, c, abortf);
        },
        [&](int64_t c) {
            hipLaunchKernelGGL(k_dec_compact, dim3(grid_for(c, 256)),
                               dim3(256), 0, s, tab, c, keys, knull,
                               groups_dev, ngroups_dev);
        });
}

__global__ void k_build_key32(const int64_t *__restrict__ src, int64_t n,
                              int32_t *__restrict__ dst,
                              unsigned int *bad)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int mybad = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t v = src[i];
        mybad |= (v < 0 || v > 0x7fffffffll);
        dst[i] = (int32_t)v;
    }
    if (__ballot(mybad) && (threadIdx.x % WAVE) == 0)
        atomicOr(bad, 1u);
}

otbx_status otbx_build_key32(const int64_t *src, int64_t n, int32_t *dst,
                             int32_t *ok_host, void *stream)
{
    if (!src || !dst || !ok_host)
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    static unsigned int *d_bad = nullptr;
    static unsigned int *h_bad = nullptr;
    if (!d_bad) {
        SCR_ALLOC_DEV(d_bad, 4);
        SCR_ALLOC_HOST(h_bad, 4);
    }
    HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, s));
    if (n > 0)
        hipLaunchKernelGGL(k_build_key32, dim3(grid_for(n, 256)), dim3(256),
                           0, s, src, n, dst, d_bad);
    HIP_CHECK(hipMemcpyAsync(h_bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *ok_host = *h_bad ? 0 : 1;
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

/* ============ N-key group-by / join (otbx_agg_i64n, otbx_join_i64n) ======
 * See include/otbx.h for semantics + citations. The otbx_keyset is passed
 * to kernels BY VALUE (132 B of kernarg — no device-side pointer array).
 * Slots claim by defining row index (execGrouping.c firstTuple pattern);
 * identity compares run over the keyset columns. Generality tier. */

__global__ void k_aggn_build(const otbx_keyset ks,
                             const double *__restrict__ vals,
                             const uint8_t *__restrict__ vnull, int64_t n,
                             claim_slot *tab, int64_t cap,
                             unsigned int *abortf)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (abortf && __hip_atomic_load(abortf, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT))
            return;
        int64_t s = (int64_t)(d_nk_hash(ks, i) & (uint64_t)mask);
        int steps = 0;
        for (;;) {
            if (abortf && ++steps > NK_PROBE_BOUND) {
                atomicOr(abortf, 1u);
                break;
            }
            long long owner = tab[s].idx;
            if (owner < 0) {
                long long prev = (long long)atomicCAS(
                    (unsigned long long *)&tab[s].idx,
                    (unsigned long long)(-1ll), (unsigned long long)i);
                owner = prev == -1ll ? i : prev;
            }
            if (d_nk_row_eq(ks, owner, i))
                break;
            s = (s + 1) & mask;
        }
        if (abortf && steps > NK_PROBE_BOUND)
            continue;
        atomicAdd(&tab[s].count_star, 1ull);
        if (!(vnull && vnull[i])) {
            atomicAdd(&tab[s].count_v, 1ull);
            atomicAdd(&tab[s].sum, vals[i]);
        }
    }
}

__global__ void k_aggn_compact(const claim_slot *__restrict__ tab, int64_t cap,
                               otbx_aggn_group *__restrict__ out,
                               int64_t *ngroups)
{
    d_block_compact(
        cap, ngroups, [=](int64_t i) { return tab[i].idx >= 0; },
        [=](int64_t i, int64_t pos) {
            out[pos].row_idx = tab[i].idx;
            out[pos].count_star = (int64_t)tab[i].count_star;
            out[pos].count_v = (int64_t)tab[i].count_v;
            out[pos].sum_v = tab[i].sum;
            out[pos].sum_isnull = tab[i].count_v == 0;
            out[pos]._pad = 0;
        });
}

/* N-key join: same structure as k_joinx_* but identity through keysets */
__global__ void k_joinn_build(const otbx_keyset ks, int64_t nb,
                              long long *slot_idx, int64_t cap)
{
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nb;
         i += stride) {
        if (d_nk_rownull(ks, i))
            continue;
        int64_t s = (int64_t)(d_nk_hash(ks, i) & (uint64_t)mask);
        while (atomicCAS((unsigned long long *)&slot_idx[s],
                         (unsigned long long)(-1ll),
                         (unsigned long long)i) != (unsigned long long)(-1ll))
            s = (s + 1) & mask;
    }
}

__global__ void k_joinn_probe(const otbx_keyset bks,
                              const long long *__restrict__ slot_idx,
                              int64_t cap, const otbx_keyset pks, int64_t np,
                              int jt,
                              unsigned long long *__restrict__ mbitmap,
                              int64_t *__restrict__ out_b,
                              int64_t *__restrict__ out_p, int64_t cap_pairs,
                              int64_t *npairs)
{
    /* per-wave LDS pair buffer (the k_joinx_probe form): one global
     * reservation per ~BUF pairs instead of one per walk step — the
     * per-step wave_append serialized on the single pair counter. */
    const bool emit_match = (jt == 0 || jt == 1 || jt == 4 || jt == 5);
    const bool fill_probe = (jt == 1 || jt == 3 || jt == 5);
    const bool semi = jt == 2;
    const int BUF = 512;
    __shared__ int64_t bufb[256 / WAVE][BUF];
    __shared__ int64_t bufp[256 / WAVE][BUF];
    int wid = (int)(threadIdx.x / WAVE), lane = (int)(threadIdx.x % WAVE);
    int nbuf = 0; /* wave-uniform */
    int64_t mask = cap - 1;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool inrange = i0 < np;
        bool rownull = inrange && d_nk_rownull(pks, i0);
        bool active = inrange && !rownull;
        int64_t s = active
                        ? (int64_t)(d_nk_hash(pks, i0) & (uint64_t)mask)
                        : 0;
        bool walking = active;
        int nmatch = 0;
        while (__any(walking)) {
            long long bidx = walking ? slot_idx[s] : -1;
            bool have = walking && bidx >= 0;
            bool match = have && d_nk_match(bks, bidx, pks, i0);
            if (match) {
                nmatch++;
                if (mbitmap)
                    atomicOr(&mbitmap[bidx >> 6], 1ull << (bidx & 63));
                if (semi && nmatch > 1)
                    match = false;
            }
            bool emit = match && emit_match;
            unsigned long long mmask = __ballot(emit);
            int cnt = __popcll(mmask);
            if (cnt) {
                if (nbuf + cnt > BUF) {
                    long long base = 0;
                    if (lane == 0)
                        base = (long long)atomicAdd(
                            (unsigned long long *)npairs,
                            (unsigned long long)nbuf);
                    base = __shfl(base, 0, WAVE);
                    for (int j = lane; j < nbuf; j += WAVE) {
                        int64_t pos = base + j;
                        if (pos < cap_pairs) {
                            out_b[pos] = bufb[wid][j];
                            out_p[pos] = bufp[wid][j];
                        }
                    }
                    nbuf = 0;
                }
                if (emit) {
                    int rank = __popcll(mmask & ((1ull << lane) - 1ull));
                    bufb[wid][nbuf + rank] = bidx;
                    bufp[wid][nbuf + rank] = i0;
                }
                nbuf += cnt;
            }
            s = (s + 1) & mask;
            walking = have;
        }
        bool fill = false;
        if (inrange) {
            if (fill_probe)
                fill = rownull || nmatch == 0;
            else if (semi)
                fill = nmatch > 0;
        }
        unsigned long long fmask = __ballot(fill);
        int fcnt = __popcll(fmask);
        if (fcnt) {
            if (nbuf + fcnt > BUF) {
                long long base = 0;
                if (lane == 0)
                    base = (long long)atomicAdd((unsigned long long *)npairs,
                                                (unsigned long long)nbuf);
                base = __shfl(base, 0, WAVE);
                for (int j = lane; j < nbuf; j += WAVE) {
                    int64_t pos = base + j;
                    if (pos < cap_pairs) {
                        out_b[pos] = bufb[wid][j];
                        out_p[pos] = bufp[wid][j];
                    }
                }
                nbuf = 0;
            }
            if (fill) {
                int rank = __popcll(fmask & ((1ull << lane) - 1ull));
                bufb[wid][nbuf + rank] = -1;
                bufp[wid][nbuf + rank] = i0;
            }
            nbuf += fcnt;
        }
        if (__all(i0 >= np))
            break;
    }
    if (nbuf) {
        long long base = 0;
        if (lane == 0)
            base = (long long)atomicAdd((unsigned long long *)npairs,
                                        (unsigned long long)nbuf);
        base = __shfl(base, 0, WAVE);
        for (int j = lane; j < nbuf; j += WAVE) {
            int64_t pos = base + j;
            if (pos < cap_pairs) {
                out_b[pos] = bufb[wid][j];
                out_p[pos] = bufp[wid][j];
            }
        }
    }
}

__global__ void k_joinn_fill_build(const otbx_keyset ks, int64_t nb,
                                   const unsigned long long *__restrict__ mbitmap,
                                   int64_t *__restrict__ out_b,
                                   int64_t *__restrict__ out_p,
                                   int64_t cap_pairs, int64_t *npairs)
{
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;;
         i0 += stride) {
        bool fill = false;
        if (i0 < nb)
            fill = d_nk_rownull(ks, i0) ||
                   !((mbitmap[i0 >> 6] >> (i0 & 63)) & 1ull);
        int64_t pos = wave_append(npairs, fill);
        if (fill && pos < cap_pairs) {
            out_b[pos] = i0;
            out_p[pos] = -1;
        }
        if (__all(i0 >= nb))
            break;
    }
}

extern "C" {

/* n = the row count the keyset's columns hold: an empty side may carry NULL
 * columns (the otbx_sort_perm rule), nkeys is checked either way */
static bool keyset_ok(const otbx_keyset *ks, int64_t n)
{
    if (!ks || ks->nkeys < 1 || ks->nkeys > OTBX_MAX_KEYS)
        return false;
    for (int c = 0; n > 0 && c < ks->nkeys; c++)
        if (!ks->keys[c])
            return false;
    return true;
}

otbx_status otbx_agg_i64n_workspace_bytes(int64_t n, size_t *bytes)
{
    *bytes = (size_t)jx_cap_for(n) * sizeof(claim_slot) +
             (size_t)AGG_SCAP * 8; /* + estimator sample table */
    return OTBX_OK;
}

otbx_status otbx_agg_i64n(const otbx_keyset *ks, const double *vals,
                          const uint8_t *vnull, int64_t n, void *ws,
                          size_t ws_bytes, otbx_aggn_group *groups_dev,
                          int64_t *ngroups_dev, void *stream)
{
    if (!keyset_ok(ks, n) || !ws || !ngroups_dev || (n > 0 && !vals))
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int64_t cap = jx_cap_for(n);
    size_t need;
    otbx_agg_i64n_workspace_bytes(n, &need);
    if (ws_bytes < need)
        return OTBX_ERR_INVALID;
    claim_slot *tab = (claim_slot *)ws;
    int64_t *stab = (int64_t *)((char *)ws + (size_t)cap * sizeof(claim_slot));
    return nk_bounded_agg(
        *ks, n, cap, stab, ngroups_dev, s,
        [&](int64_t c) {
            hipLaunchKernelGGL(k_claim_init, dim3(grid_for(c, 256)),
                               dim3(256), 0, s, tab, c);
        },
        [&](int64_t c, unsigned int *abortf) {
            hipLaunchKernelGGL(k_aggn_build, dim3(grid_for(n, 256)),
                               dim3(256), 0, s, *ks, vals, vnull, n, tab, c,
                               abortf);
        },
        [&](int64_t c) {
            hipLaunchKernelGGL(k_aggn_compact, dim3(grid_for(c, 256)),
                               dim3(256), 0, s, tab, c, groups_dev,
                               ngroups_dev);
        });
}

otbx_status otbx_join_i64n_workspace_bytes(int64_t nb, int64_t np,
                                           size_t *bytes)
{
    (void)np;
    *bytes = (size_t)jx_cap_for(nb) * 8 + (size_t)((nb + 63) / 64 + 1) * 8;
    return OTBX_OK;
}

otbx_status otbx_join_i64n(const otbx_keyset *bks, int64_t nb,
                           const otbx_keyset *pks, int64_t np,
                           int32_t join_type, void *ws, size_t ws_bytes,
                           int64_t *out_b, int64_t *out_p, int64_t cap_pairs,
                           int64_t *npairs_dev, void *stream)
{
    if (!keyset_ok(bks, nb) || !keyset_ok(pks, np) ||
        bks->nkeys != pks->nkeys ||
        join_type < 0 || join_type > 5 || !ws || !npairs_dev)
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int64_t cap = jx_cap_for(nb);
    size_t need;
    otbx_join_i64n_workspace_bytes(nb, np, &need);
    if (ws_bytes < need)
        return OTBX_ERR_INVALID;
    long long *slot_idx = (long long *)ws;
    unsigned long long *mbitmap =
        (unsigned long long *)((char *)ws + (size_t)cap * 8);
    const bool fill_build = (join_type == 4 || join_type == 5);
    HIP_CHECK(hipMemsetAsync(npairs_dev, 0, 8, s));
    hipLaunchKernelGGL(k_fill_i64, dim3(grid_for(cap, 256)), dim3(256), 0, s,
                       (int64_t *)slot_idx, cap, -1ll);
    if (fill_build)
        HIP_CHECK(hipMemsetAsync(mbitmap, 0,
                                 (size_t)((nb + 63) / 64 + 1) * 8, s));
    if (nb > 0)
        hipLaunchKernelGGL(k_joinn_build, dim3(grid_for(nb, 256)), dim3(256),
                           0, s, *bks, nb, slot_idx, cap);
    if (np > 0)
        hipLaunchKernelGGL(k_joinn_probe, dim3(grid_for(np, 256)), dim3(256),
                           0, s, *bks, slot_idx, cap, *pks, np, join_type,
                           fill_build ? mbitmap : NULL, out_b, out_p,
                           cap_pairs, npairs_dev);
    if (fill_build && nb > 0)
        hipLaunchKernelGGL(k_joinn_fill_build, dim3(grid_for(nb, 256)),
                           dim3(256), 0, s, *bks, nb, mbitmap, out_b, out_p,
                           cap_pairs, npairs_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

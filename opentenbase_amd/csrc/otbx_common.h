/*
 * otbx_common.h — what more than one otbx*.hip unit needs: the error macro,
 * launch/size helpers and the block-aggregated emission primitive. Private
 * to csrc/; the public boundary is include/otbx.h.
 */
#ifndef OTBX_COMMON_H
#define OTBX_COMMON_H

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>

#include "../../include/otbx.h"

/* wave width is 64 on CDNA4 — hard-coded per the HIP guide */
#define WAVE 64

#define HIP_CHECK(x)                                                     \
    do {                                                                 \
        hipError_t err_ = (x);                                           \
        if (err_ != hipSuccess) {                                        \
            fprintf(stderr, "otbx: HIP error %s at %s:%d\n",             \
                    hipGetErrorString(err_), __FILE__, __LINE__);        \
            return OTBX_ERR_HIP;                                         \
        }                                                                \
    } while (0)

static inline int grid_for(int64_t work, int block)
{
    int64_t g = (work + block - 1) / block;
    if (g > 2048) g = 2048;   /* 256 CUs × 8 blocks; grid-stride the rest */
    if (g < 1) g = 1;
    return (int)g;
}

static inline size_t align256_sz(size_t x) { return (x + 255) & ~(size_t)255; }

/* clang vector types: what __builtin_nontemporal_load takes for a 16-B load */
typedef double v2d __attribute__((ext_vector_type(2)));
typedef long long v2l __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));

/* The one registry of lazily allocated per-process scratch (defined in
 * otbx.hip next to otbx_finish, which releases every registered slot and
 * nulls the static that owns it). Not part of the C-ABI. */
__attribute__((visibility("hidden")))
hipError_t otbx_scr_alloc(void **slot, size_t bytes, int host);

#define SCR_ALLOC_DEV(p, bytes) \
    HIP_CHECK(otbx_scr_alloc((void **)&(p), (bytes), 0))
#define SCR_ALLOC_HOST(p, bytes) \
    HIP_CHECK(otbx_scr_alloc((void **)&(p), (bytes), 1))

/* blockDim.x for device functions. The HIP header's form picks between the
 * group size and the last group's remainder; written in a kernel it folds
 * to one scalar load (work-groups are uniform), inside an inlined helper it
 * stays a select + vector load. The builtin is the uniform size itself. */
__device__ __forceinline__ unsigned int d_block_dim_x(void)
{
    return __builtin_amdgcn_workgroup_size_x();
}

/* block-aggregated two-phase emission of the used slots of a cap-slot table:
 * ONE global reservation per block (a per-wave wave_append over a
 * 1-billion-slot table made ~16 M global-counter reservations — measured
 * 201 ms of a 339 ms call at cap 2^30; this form costs one extra pass over
 * the block's range). used(i) tests slot i; emit(i, pos) writes output row
 * pos from slot i. Every thread of the block must call it; blocks whose
 * range is all empty (low-cardinality tables) skip pass 2. */
template <typename Used, typename Emit>
__device__ __forceinline__ void d_block_compact(int64_t cap, int64_t *ngroups,
                                                Used used, Emit emit)
{
    __shared__ unsigned long long lbase;
    __shared__ unsigned int lcnt, ltot;
    if (threadIdx.x == 0) lcnt = 0;
    __syncthreads();
    int64_t per_block = (cap + gridDim.x - 1) / gridDim.x;
    int64_t lo = blockIdx.x * per_block;
    int64_t hi = lo + per_block < cap ? lo + per_block : cap;
    int lane = (int)(threadIdx.x % WAVE);
    for (int64_t i = lo + threadIdx.x; i < hi; i += d_block_dim_x()) {
        unsigned long long mask = __ballot(used(i));
        if (lane == 0 && mask)
            atomicAdd(&lcnt, (unsigned int)__popcll(mask));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ltot = lcnt;
        lbase = lcnt ? (unsigned long long)atomicAdd(
                           (unsigned long long *)ngroups,
                           (unsigned long long)lcnt)
                     : 0;
        lcnt = 0;
    }
    __syncthreads();
    if (ltot == 0) return;
    for (int64_t i = lo + threadIdx.x; i < hi; i += d_block_dim_x()) {
        bool u = used(i);
        unsigned long long mask = __ballot(u);
        if (!mask) continue;
        unsigned int wbase = 0;
        if (lane == 0)
            wbase = atomicAdd(&lcnt, (unsigned int)__popcll(mask));
        wbase = (unsigned int)__shfl((int)wbase, 0, WAVE);
        if (u)
            emit(i, (int64_t)lbase + wbase +
                        __popcll(mask & ((1ull << lane) - 1ull)));
    }
}

#endif /* OTBX_COMMON_H */

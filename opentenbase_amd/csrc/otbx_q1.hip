/*
 * otbx_q1.hip — the TPC-H Q1 fused partial aggregate, the flagship kernel
 * (otbx_q1_partial, otbx_q1_partial_variant), and the staging passes that
 * build the packed columns it prefers (otbx_build_q1codes /
 * otbx_q1code_plan, otbx_build_q1pcodes / otbx_q1price_plan). SeqScan + qual
 * + project + partial HashAgg in one pass: execScan.c:140,
 * execExprInterp.c:324, nodeAgg.c:856 with int8inc / float8pl transitions.
 * DESIGN.md §3 (the kernel), §7b (code column), §7c (price column).
 *
 * Two kernel families share everything but the loads:
 *   k_q1_raw<R, NT>        — variants 0-2. Reads the raw columns, 38 B/row
 *                            algorithmic; the path for tables without a code
 *                            column. R rows per lane per iteration (2 or 4),
 *                            NT: non-temporal loads on the read-once f64
 *                            streams.
 *   k_q1_coded<R, NG, PC>  — variants 3-7. Reads the staged packed code
 *                            column plus l_extendedprice (12 B/row; variants
 *                            3-5, the default when otbx_build_q1codes
 *                            succeeded) or plus the packed price column
 *                            (8 B/row; variants 6-7, the default when
 *                            otbx_build_q1pcodes succeeded too).
 * Each family has one row function (d_q1_raw_row, d_q1c_row) used by its
 * main loop and its tail, and both end in the one epilogue d_q1_reduce.
 * The 6-combo group domain lives in per-lane registers (compile-time-indexed
 * — runtime indexing would go to scratch), selected by compare + multiply;
 * wave64 shuffle reduction, per-block LDS combine, one device atomic per
 * (group, aggregate) per block.
 *
 * Staging: k_q1c_collect / k_q1c_encode build the code column,
 * k_q1p_collect / k_q1p_encode the price column; each encode pass decodes
 * its own word again and compares it with the source row. Their lazily
 * allocated state goes through the scratch registry of otbx.hip
 * (otbx_common.h: otbx_scr_alloc), which otbx_finish releases.
 */
#include <string.h>

#include <algorithm>   /* std::sort (code dictionaries) */

#include "otbx_common.h"

#define Q1_NG 6
#define Q1_NS 5

template <bool NT>
__device__ __forceinline__ double2 ld2(const double2 *p)
{
    if (NT) {
        v2d v = __builtin_nontemporal_load((const v2d *)p);
        return make_double2(v.x, v.y);
    }
    return *p;
}

/* The epilogue of every Q1 kernel: wave64 shuffle reduction, per-block LDS
 * combine (the 4 waves added in index order by thread 0), then one atomic
 * per non-zero value; accumulator g lands in output group slot[g]. Every
 * thread of the 256-thread block must call it, once per kernel. */
template <int NG>
__device__ __forceinline__ void d_q1_reduce(
    double (&acc)[NG][Q1_NS], uint32_t (&cnt)[NG],
    const uint32_t (&slot)[NG], double *__restrict__ out_sums, /* [6][5] */
    unsigned long long *__restrict__ out_counts /* [6] */)
{
#pragma unroll
    for (int g = 0; g < NG; g++) {
#pragma unroll
        for (int s = 0; s < Q1_NS; s++)
            for (int off = WAVE / 2; off > 0; off >>= 1)
                acc[g][s] += __shfl_down(acc[g][s], off, WAVE);
        for (int off = WAVE / 2; off > 0; off >>= 1)
            cnt[g] += __shfl_down(cnt[g], off, WAVE);
    }
    __shared__ double lacc[256 / WAVE][NG][Q1_NS];
    __shared__ uint32_t lcnt[256 / WAVE][NG];
    int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < NG; g++) {
#pragma unroll
            for (int s = 0; s < Q1_NS; s++) lacc[wid][g][s] = acc[g][s];
            lcnt[wid][g] = cnt[g];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nw = d_block_dim_x() / WAVE;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            unsigned long long c = 0;
#pragma unroll
            for (int s = 0; s < Q1_NS; s++) {
                double v = 0;
                for (int w = 0; w < nw; w++) v += lacc[w][g][s];
                if (v != 0.0) atomicAdd(&out_sums[slot[g] * Q1_NS + s], v);
            }
            for (int w = 0; w < nw; w++) c += lcnt[w][g];
            if (c) atomicAdd(&out_counts[slot[g]], c);
        }
    }
}

/* variants 0 - 2: the raw columns. One row: group id from the two flag
 * bytes, the projection, and the masked six-way accumulate — acc += w * x
 * with w in {0.0, 1.0}, a mul and an add under -ffp-contract=off (the
 * instruction count DESIGN.md §7b measured against). Main loop and tail
 * both call it, so a non-finite operand in a row that does not pass turns
 * its sums NaN (0.0 * Inf) wherever the row sits, as in the coded kernels. */
__device__ __forceinline__ void d_q1_raw_row(double (&acc)[Q1_NG][Q1_NS],
                                             uint32_t (&cnt)[Q1_NG],
                                             int32_t dd, uint8_t rr,
                                             uint8_t ll, double qv, double pv,
                                             double dv, double tv,
                                             int32_t cutoff)
{
    bool pass = dd <= cutoff;
    int gid = (rr == 'A' ? 0 : (rr == 'N' ? 1 : 2)) * 2 + (ll == 'F' ? 0 : 1);
    double dp = pv * (1.0 - dv);   /* disc_price (ExecProject) */
    double ch = dp * (1.0 + tv);   /* charge */
#pragma unroll
    for (int g = 0; g < Q1_NG; g++) {
        bool m = pass && (gid == g);
        double w = m ? 1.0 : 0.0;
        acc[g][0] += w * qv;
        acc[g][1] += w * pv;
        acc[g][2] += w * dp;
        acc[g][3] += w * ch;
        acc[g][4] += w * dv;
        cnt[g] += m;
    }
}

/* R consecutive rows of one f64 column, as R/2 16-B loads (coalescing sweet
 * spot per the HIP guide G13) */
template <int R, bool NT>
__device__ __forceinline__ void d_q1_ld(const double *col, int64_t i,
                                        double (&v)[R])
{
    const double2 *col2 = (const double2 *)col;
#pragma unroll
    for (int k = 0; k < R / 2; k++) {
        double2 x = ld2<NT>(&col2[(R / 2) * i + k]);
        v[2 * k] = x.x;
        v[2 * k + 1] = x.y;
    }
}

template <typename T, int N>
using q1_vec = T __attribute__((ext_vector_type(N)));

/* R: rows per lane per iteration — 2 (variant 0: one 8-B date load, one 2-B
 * load per flag column, one 16-B load per f64 column) or 4 (variants 1 and
 * 2: 16-B dates, 4-B flags, two 16-B loads per f64 column). NT: non-temporal
 * loads on the read-once f64 streams (variant 2). */
template <int R, bool NT>
__launch_bounds__(256, 2)
__global__ void k_q1_raw(const int32_t *__restrict__ sd,
                         const uint8_t *__restrict__ rf,
                         const uint8_t *__restrict__ ls,
                         const double *__restrict__ qty,
                         const double *__restrict__ price,
                         const double *__restrict__ disc,
                         const double *__restrict__ tax, int64_t n,
                         int32_t cutoff, double *__restrict__ out_sums,
                         unsigned long long *__restrict__ out_counts)
{
    double acc[Q1_NG][Q1_NS] = {};
    uint32_t cnt[Q1_NG] = {};
    int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t nv = n / R;
    const q1_vec<int32_t, R> *sdv = (const q1_vec<int32_t, R> *)sd;
    const q1_vec<uint8_t, R> *rfv = (const q1_vec<uint8_t, R> *)rf;
    const q1_vec<uint8_t, R> *lsv = (const q1_vec<uint8_t, R> *)ls;
    for (int64_t i = tid; i < nv; i += stride) {
        q1_vec<int32_t, R> d = sdv[i];
        q1_vec<uint8_t, R> r = rfv[i];
        q1_vec<uint8_t, R> l = lsv[i];
        double qv[R], pv[R], dv[R], tv[R];
        d_q1_ld<R, NT>(qty, i, qv);
        d_q1_ld<R, NT>(price, i, pv);
        d_q1_ld<R, NT>(disc, i, dv);
        d_q1_ld<R, NT>(tax, i, tv);
#pragma unroll
        for (int j = 0; j < R; j++)
            d_q1_raw_row(acc, cnt, d[j], r[j], l[j], qv[j], pv[j], dv[j],
                         tv[j], cutoff);
    }
    /* tail rows (n % R) by thread 0 of block 0 */
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * R; i < n; i++)
            d_q1_raw_row(acc, cnt, sd[i], rf[i], ls[i], qty[i], price[i],
                         disc[i], tax[i], cutoff);
    const uint32_t ident[Q1_NG] = {0, 1, 2, 3, 4, 5};
    d_q1_reduce<Q1_NG>(acc, cnt, ident, out_sums, out_counts);
}

/* variants 3 - 5: the staged packed code column (otbx.h q1code; DESIGN.md
 * §7b). One 32-bit word per row carries the shipdate offset, the group slot
 * and dictionary codes of quantity / discount / tax; the kernel streams that
 * word plus l_extendedprice — 12 B/row instead of 38. The dictionaries hold
 * the exact f64 bit patterns, so every per-row operand is bit-identical to
 * what the raw-column kernels load. The masked accumulate is an explicit
 * fma(w, x, acc): with w in {0.0, 1.0} the product is exact, so it rounds
 * exactly as acc + w * x does under -ffp-contract=off, in half the f64
 * instructions. */
struct q1c_fields {   /* bit offset / width of each field, by-value kernarg */
    uint32_t date_off, date_bits, gid_off, qty_off, qty_bits, disc_off,
        disc_bits, tax_off, tax_bits;
    /* the group slots the kernel accumulates: all six, or (variant 5) only
     * those the build found in the table (otbx.h gid_present) */
    uint32_t slot[Q1_NG];
};

template <int NG>
__device__ __forceinline__ void d_q1c_row(double (&acc)[NG][Q1_NS],
                                          uint32_t (&cnt)[NG], uint32_t c,
                                          double pv, const double *sdict,
                                          const q1c_fields &f, int32_t cut_rel)
{
    /* v_bfe_u32: a width of 0 (single-valued column) reads as 0 */
    int32_t off = (int32_t)__builtin_amdgcn_ubfe(c, f.date_off, f.date_bits);
    uint32_t gid = __builtin_amdgcn_ubfe(c, f.gid_off, 3u);
    double qv = sdict[__builtin_amdgcn_ubfe(c, f.qty_off, f.qty_bits)];
    double dv = sdict[OTBX_Q1_DICT_MAX +
                      __builtin_amdgcn_ubfe(c, f.disc_off, f.disc_bits)];
    double tv = sdict[2 * OTBX_Q1_DICT_MAX +
                      __builtin_amdgcn_ubfe(c, f.tax_off, f.tax_bits)];
    /* l_shipdate <= cutoff  <=>  off <= cutoff - date_base (host-clamped) */
    uint32_t sel = off <= cut_rel ? gid : 7u;
    double dp = pv * (1.0 - dv);   /* disc_price (ExecProject) */
    double ch = dp * (1.0 + tv);   /* charge */
#pragma unroll
    for (int g = 0; g < NG; g++) {
        bool m = sel == f.slot[g];   /* uniform (SGPR) operand */
        double w = m ? 1.0 : 0.0;
        acc[g][0] = __builtin_fma(w, qv, acc[g][0]);
        acc[g][1] = __builtin_fma(w, pv, acc[g][1]);
        acc[g][2] = __builtin_fma(w, dp, acc[g][2]);
        acc[g][3] = __builtin_fma(w, ch, acc[g][3]);
        acc[g][4] = __builtin_fma(w, dv, acc[g][4]);
        cnt[g] += m;
    }
}

/* variants 6 / 7: the packed price word (otbx.h q1pcode)
 * replaces l_extendedprice, 8 B/row instead of 12. By-value kernarg; the K
 * field is the lowest of the word, so it is taken with a mask (a 32-bit
 * wide field is outside v_bfe_u32's 5-bit width operand). */
struct q1p_fields {
    uint32_t k_mask;
    int32_t k_base;
    uint32_t d_off, d_bits;
    int32_t d_base;
    double mul;
};

/* the one decode of a price word: the encode pass checks every word with
 * it, the Q1 kernel reads prices through it. (double)K and K * mul are one
 * v_cvt_f64_i32 and one v_mul_f64 (no contraction: -ffp-contract=off), so
 * pred is the same double wherever it is computed. */
__device__ __forceinline__ double d_q1p_decode(uint32_t w, const q1p_fields &p)
{
    int32_t k = (int32_t)((uint32_t)p.k_base + (w & p.k_mask));
    double pred = (double)k * p.mul;
    int32_t d = p.d_base + (int32_t)__builtin_amdgcn_ubfe(w, p.d_off, p.d_bits);
    return __longlong_as_double((long long)(
        (unsigned long long)__double_as_longlong(pred) +
        (unsigned long long)(long long)d));
}

/* R: rows per lane per iteration (4 or 8); NG: group slots accumulated;
 * PC: `price` is the packed price column (uint32 words decoded through pf)
 * instead of l_extendedprice (f64). With PC and R = 4 (variant 6) every lane
 * sees the same rows in the same order as variant 5 and every operand is
 * bit-identical (the decode is lossless), so per-lane, per-wave and
 * per-block partials are bit-identical to variant 5's; only the order of
 * the block atomics differs. */
template <int R, int NG, bool PC>
__launch_bounds__(256, 2)
__global__ void k_q1_coded(const uint32_t *__restrict__ code,
                           const void *__restrict__ price_col,
                           const uint64_t *__restrict__ dict,
                           const q1c_fields f, const q1p_fields pf, int64_t n,
                           int32_t cut_rel, double *__restrict__ out_sums,
                           unsigned long long *__restrict__ out_counts)
{
    const double *price = (const double *)price_col;
    const uint32_t *pcode = (const uint32_t *)price_col;
    __shared__ double sdict[3 * OTBX_Q1_DICT_MAX];   /* 6 KB */
    for (int i = threadIdx.x; i < 3 * OTBX_Q1_DICT_MAX; i += 256)
        sdict[i] = __longlong_as_double((long long)dict[i]);
    __syncthreads();

    /* acc is zeroed by a loop, not by `= {}` like cnt and like k_q1_raw's:
     * that form costs <4, 3, true> one more VGPR (69, not 68) */
    double acc[NG][Q1_NS];
    uint32_t cnt[NG] = {};
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int s = 0; s < Q1_NS; s++) acc[g][s] = 0.0;
    int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t nq = n / R;
    const v4i *code4 = (const v4i *)code;
    const v4i *pcode4 = (const v4i *)pcode;
    for (int64_t i = tid; i < nq; i += stride) {
        uint32_t cw[R];
        double pv[R];
#pragma unroll
        for (int k = 0; k < R / 4; k++) {
            v4i c = __builtin_nontemporal_load(&code4[(R / 4) * i + k]);
            cw[4 * k] = (uint32_t)c.x;
            cw[4 * k + 1] = (uint32_t)c.y;
            cw[4 * k + 2] = (uint32_t)c.z;
            cw[4 * k + 3] = (uint32_t)c.w;
        }
        if (PC) {
            uint32_t pw[R];
#pragma unroll
            for (int k = 0; k < R / 4; k++) {
                v4i c = __builtin_nontemporal_load(&pcode4[(R / 4) * i + k]);
                pw[4 * k] = (uint32_t)c.x;
                pw[4 * k + 1] = (uint32_t)c.y;
                pw[4 * k + 2] = (uint32_t)c.z;
                pw[4 * k + 3] = (uint32_t)c.w;
            }
#pragma unroll
            for (int j = 0; j < R; j++) pv[j] = d_q1p_decode(pw[j], pf);
        } else
            d_q1_ld<R, true>(price, i, pv);
#pragma unroll
        for (int j = 0; j < R; j++)
            d_q1c_row<NG>(acc, cnt, cw[j], pv[j], sdict, f, cut_rel);
    }
    /* tail rows (n % R) by thread 0 of block 0 */
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nq * R; i < n; i++)
            d_q1c_row<NG>(acc, cnt, code[i],
                          PC ? d_q1p_decode(pcode[i], pf) : price[i], sdict,
                          f, cut_rel);
    /* group g lands in output slot f.slot[g]. The map is copied here: given
     * a reference into the kernarg struct, the compiler loads all of f at
     * kernel entry and keeps it live (<8, 4, true>: 140 VGPRs, not 92) */
    uint32_t slot[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) slot[g] = f.slot[g];
    d_q1_reduce<NG>(acc, cnt, slot, out_sums, out_counts);
}

/* a descriptor the coded kernel can run with: every dictionary index stays
 * below OTBX_Q1_DICT_MAX and every field inside the word */
static bool q1c_desc_ok(const otbx_q1code_desc *d)
{
    const int32_t off[5] = {d->date_off, d->gid_off, d->qty_off, d->disc_off,
                            d->tax_off};
    const int32_t bits[5] = {d->date_bits, d->gid_bits, d->qty_bits,
                             d->disc_bits, d->tax_bits};
    for (int k = 0; k < 5; k++)
        if (off[k] < 0 || bits[k] < 0 || off[k] + bits[k] > 32)
            return false;
    return d->dict && d->gid_bits == 3 && d->date_bits <= 29 &&
           d->gid_present > 0 && d->gid_present < (1 << Q1_NG) &&
           d->qty_bits <= 8 && d->disc_bits <= 8 && d->tax_bits <= 8;
}

static const double q1p_mul[5] = {1.0, 0.1, 0.01, 0.001, 0.0001};
static const double q1p_scale[5] = {1.0, 10.0, 100.0, 1000.0, 10000.0};

/* a price descriptor the coded kernel can decode with: the K field lowest,
 * both fields inside the word, the correction at most 8 bits, and mul the
 * literal of its exponent */
static bool q1p_desc_ok(const otbx_q1price_desc *d)
{
    if (d->k_off != 0 || d->k_bits < 0 || d->k_bits > 32 || d->d_off < 0 ||
        d->d_bits < 0 || d->d_bits > 8 || d->d_off + d->d_bits > 32 ||
        d->d_off < d->k_bits)
        return false;
    return d->scale_exp >= 0 && d->scale_exp <= 4 &&
           d->mul == q1p_mul[d->scale_exp];
}

static q1p_fields q1p_fields_of(const otbx_q1price_desc *d)
{
    q1p_fields p = {d->k_bits >= 32 ? 0xffffffffu : (1u << d->k_bits) - 1u,
                    d->k_base, (uint32_t)d->d_off, (uint32_t)d->d_bits,
                    d->d_base, d->mul};
    return p;
}

extern "C" otbx_status otbx_q1_partial_variant(const otbx_lineitem_dev *t,
                                               int32_t cutoff_day,
                                               double *sums_dev,
                                               int64_t *counts_dev,
                                               void *stream, float *kernel_ms,
                                               int variant)
{
    if (!t || !sums_dev || !counts_dev) return OTBX_ERR_INVALID;
    if (variant >= 3 && (variant > 7 || !t->q1code || !q1c_desc_ok(&t->q1desc)))
        return OTBX_ERR_INVALID;
    if (variant >= 6 ? !t->q1pcode || !q1p_desc_ok(&t->q1pdesc)
                     : variant >= 3 && !t->l_extendedprice)
        return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(sums_dev, 0, Q1_NG * Q1_NS * sizeof(double), s));
    HIP_CHECK(hipMemsetAsync(counts_dev, 0, Q1_NG * sizeof(int64_t), s));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms) {
        HIP_CHECK(hipEventCreate(&ev0));
        HIP_CHECK(hipEventCreate(&ev1));
        HIP_CHECK(hipEventRecord(ev0, s));
    }
#define Q1R_LAUNCH(R, NT)                                                   \
    hipLaunchKernelGGL((k_q1_raw<R, NT>), dim3(grid_for(t->n / R, 256)),    \
                       dim3(256), 0, s, t->l_shipdate, t->l_returnflag,     \
                       t->l_linestatus, t->l_quantity, t->l_extendedprice,  \
                       t->l_discount, t->l_tax, t->n, cutoff_day, sums_dev, \
                       (unsigned long long *)counts_dev)
    if (variant == 0)
        Q1R_LAUNCH(2, false);
    else if (variant == 1)
        Q1R_LAUNCH(4, false);
    else if (variant >= 3) {
        const otbx_q1code_desc *d = &t->q1desc;
        q1c_fields f = {(uint32_t)d->date_off, (uint32_t)d->date_bits,
                        (uint32_t)d->gid_off, (uint32_t)d->qty_off,
                        (uint32_t)d->qty_bits, (uint32_t)d->disc_off,
                        (uint32_t)d->disc_bits, (uint32_t)d->tax_off,
                        (uint32_t)d->tax_bits, {0, 1, 2, 3, 4, 5}};
        /* date offsets are below 2^29, so the 64-bit difference clamped to
         * [-1, INT32_MAX] compares right for every int32 cutoff */
        int64_t rel = (int64_t)cutoff_day - (int64_t)d->date_base;
        int32_t cut_rel = rel < 0 ? -1 : rel > INT32_MAX ? INT32_MAX
                                                         : (int32_t)rel;
        const bool pc = variant >= 6;
        q1p_fields pf = {};
        if (pc) pf = q1p_fields_of(&t->q1pdesc);
#define Q1C_LAUNCH(R, NG, PC)                                               \
    hipLaunchKernelGGL((k_q1_coded<R, NG, PC>),                             \
                       dim3(grid_for(t->n / R, 256)), dim3(256), 0, s,      \
                       t->q1code,                                           \
                       PC ? (const void *)t->q1pcode                        \
                          : (const void *)t->l_extendedprice,               \
                       d->dict, f, pf, t->n, cut_rel, sums_dev,             \
                       (unsigned long long *)counts_dev)
#define Q1C_LAUNCH_NG(R, PC)                                                \
    switch (ng) {                                                           \
    case 1: Q1C_LAUNCH(R, 1, PC); break;                                    \
    case 2: Q1C_LAUNCH(R, 2, PC); break;                                    \
    case 3: Q1C_LAUNCH(R, 3, PC); break;                                    \
    case 4: Q1C_LAUNCH(R, 4, PC); break;                                    \
    case 5: Q1C_LAUNCH(R, 5, PC); break;                                    \
    default: Q1C_LAUNCH(R, 6, PC); break;                                   \
    }
        if (variant == 3)
            Q1C_LAUNCH(4, 6, false);
        else if (variant == 4)
            Q1C_LAUNCH(8, 6, false);
        else {
            /* only the slots present in the table (real Q1 data: 4 of 6) */
            int ng = 0;
            for (uint32_t g = 0; g < Q1_NG; g++)
                if (d->gid_present >> g & 1) f.slot[ng++] = g;
            if (variant == 5)
                Q1C_LAUNCH_NG(4, false)
            else if (variant == 6)
                Q1C_LAUNCH_NG(4, true)
            else
                Q1C_LAUNCH_NG(8, true)
        }
#undef Q1C_LAUNCH_NG
#undef Q1C_LAUNCH
    } else
        Q1R_LAUNCH(4, true);
#undef Q1R_LAUNCH
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

extern "C" otbx_status otbx_q1_partial(const otbx_lineitem_dev *t,
                                       int32_t cutoff_day, double *sums_dev,
                                       int64_t *counts_dev, void *stream,
                                       float *kernel_ms)
{
    /* With the packed price column as well (otbx_build_q1pcodes) the scan
     * reads 8 B/row; of the two kernels that decode it variant 7 (8 rows per
     * lane) had the lower time in each of 8 interleaved rounds at SF100:
     * median 1.080 ms vs 1.128 (v6, 4 rows/lane) and 1.285 (v5) in the same
     * process (profiles/q1_price_ab.txt).
     * With the staged code column alone (otbx_build_q1codes) the scan reads 12
     * B/row; of the coded kernels variant 5 (only the group slots present in
     * the table) measured best at SF100: 1.26 ms vs 1.36 (v3) and 1.88 (v4,
     * 8 rows/lane), against 3.78 ms for variant 2 in the same process — 8
     * interleaved rounds, profiles/q1_codes_ab.txt, DESIGN.md §7b. Without
     * the cache, variant 2 (4 rows/lane + non-temporal loads) is the best of the
     * raw-column kernels: 3.85 ms vs 4.25 ms (v0) at SF100 — within-probe
     * interleaved A/B, 8 rounds (profiles/r01_q1_ab.txt) */
    if (!t) return OTBX_ERR_INVALID;
    return otbx_q1_partial_variant(t, cutoff_day, sums_dev, counts_dev, stream,
                                   kernel_ms,
                                   t->q1code ? (t->q1pcode ? 7 : 5) : 2);
}

/* ---- staging: build the packed Q1 code column (otbx.h q1code) ---- */

#define Q1C_EMPTY 0xffffffffffffffffull   /* empty slot of a distinct set */
#define Q1C_LSET 512                      /* per-block LDS set, slots/column */
#define Q1C_GSET 1024                     /* global set, slots/column */
#define Q1C_F_NOFIT 1u                    /* too many values / marker seen */
#define Q1C_F_MISMATCH 2u                 /* encode round trip failed */

struct q1c_state {   /* device scratch + its pinned host mirror */
    unsigned long long set[3][Q1C_GSET];
    unsigned long long dict[3 * OTBX_Q1_DICT_MAX];
    unsigned int count[3];
    unsigned int flags;
    unsigned int present;   /* bit g: some row has group slot g */
    int dmin, dmax;
};

/* insert bit pattern v into an open-addressing set: 1 = inserted by this
 * call, 0 = already present, -1 = no free slot. The slot is read before the
 * CAS, so a value seen before costs loads only. All accesses are atomics
 * (otbx.hip header: no plain loads of mutable shared words in a launch). */
template <int SCOPE>
__device__ __forceinline__ int d_q1c_set_insert(unsigned long long *tab,
                                                uint32_t nslots,
                                                unsigned long long v)
{
    uint32_t s = ((uint32_t)(v >> 32) * 0x9E3779B1u ^
                  (uint32_t)v * 0x85EBCA6Bu) >> 16;
    for (uint32_t step = 0; step < nslots; step++) {
        s &= nslots - 1;
        unsigned long long cur =
            __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, SCOPE);
        if (cur == v) return 0;
        if (cur == Q1C_EMPTY) {
            unsigned long long prev = atomicCAS(&tab[s], Q1C_EMPTY, v);
            if (prev == Q1C_EMPTY) return 1;
            if (prev == v) return 0;
        }
        s++;
    }
    return -1;
}

/* pass 1: distinct bit patterns of the three measure columns (block-local
 * LDS set first; only a block's first sighting goes to the global set) and
 * the shipdate range. Stops early once any block reports "does not fit". */
__global__ void k_q1c_collect(const double *__restrict__ qty,
                              const double *__restrict__ disc,
                              const double *__restrict__ tax,
                              const int32_t *__restrict__ sd, int64_t n,
                              q1c_state *st)
{
    __shared__ unsigned long long lset[3][Q1C_LSET];
    for (uint32_t i = threadIdx.x; i < 3 * Q1C_LSET; i += d_block_dim_x())
        (&lset[0][0])[i] = Q1C_EMPTY;
    __syncthreads();
    const double *col[3] = {qty, disc, tax};
    int dmin = INT_MAX, dmax = INT_MIN;
    unsigned int bad = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (__hip_atomic_load(&st->flags, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
            break;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            unsigned long long v =
                (unsigned long long)__double_as_longlong(col[c][i]);
            if (v == Q1C_EMPTY) {
                bad = 1;
                continue;
            }
            int r = d_q1c_set_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(
                lset[c], Q1C_LSET, v);
            if (r == 1) {
                r = d_q1c_set_insert<__HIP_MEMORY_SCOPE_AGENT>(
                    st->set[c], Q1C_GSET, v);
                if (r == 1 &&
                    atomicAdd(&st->count[c], 1u) >= OTBX_Q1_DICT_MAX)
                    bad = 1;
            }
            if (r < 0) bad = 1;
        }
        int d = sd[i];
        dmin = d < dmin ? d : dmin;
        dmax = d > dmax ? d : dmax;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        int a = __shfl_down(dmin, off, WAVE), b = __shfl_down(dmax, off, WAVE);
        dmin = a < dmin ? a : dmin;
        dmax = b > dmax ? b : dmax;
    }
    if ((threadIdx.x % WAVE) == 0) {
        atomicMin(&st->dmin, dmin);
        atomicMax(&st->dmax, dmax);
    }
    if (bad) atomicOr(&st->flags, Q1C_F_NOFIT);
}

__device__ __forceinline__ uint32_t d_q1c_field(uint32_t w, int32_t off,
                                                int32_t bits)
{
    return bits ? (uint32_t)((uint64_t)w >> off) & ((1u << bits) - 1u) : 0u;
}

/* pass 2: one code word per row, then decode that word again and compare it
 * bit-for-bit with the source row — the round trip is checked by the build
 * itself. gid uses exactly the raw-column kernels' mapping, so unexpected
 * flag bytes land in the same slot as there. */
__global__ void k_q1c_encode(const int32_t *__restrict__ sd,
                             const uint8_t *__restrict__ rf,
                             const uint8_t *__restrict__ ls,
                             const double *__restrict__ qty,
                             const double *__restrict__ disc,
                             const double *__restrict__ tax, int64_t n,
                             const otbx_q1code_desc d,
                             uint32_t *__restrict__ codes, q1c_state *st)
{
    __shared__ unsigned long long sdict[3 * OTBX_Q1_DICT_MAX];
    for (uint32_t i = threadIdx.x; i < 3 * OTBX_Q1_DICT_MAX;
         i += d_block_dim_x())
        sdict[i] = d.dict[i];
    __syncthreads();
    const double *col[3] = {qty, disc, tax};
    const int32_t nd[3] = {d.nqty, d.ndisc, d.ntax};
    const int32_t foff[3] = {d.qty_off, d.disc_off, d.tax_off};
    const int32_t fbits[3] = {d.qty_bits, d.disc_bits, d.tax_bits};
    unsigned int bad = 0, present = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int32_t date = sd[i];
        uint8_t rr = rf[i], ll = ls[i];
        uint32_t gid = (rr == 'A' ? 0 : (rr == 'N' ? 1 : 2)) * 2 +
                       (ll == 'F' ? 0 : 1);
        present |= 1u << gid;
        uint32_t doff = (uint32_t)date - (uint32_t)d.date_base;
        uint64_t w = ((uint64_t)doff << d.date_off) |
                     ((uint64_t)gid << d.gid_off);
        unsigned long long v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[c] = (unsigned long long)__double_as_longlong(col[c][i]);
            const unsigned long long *tab = &sdict[c * OTBX_Q1_DICT_MAX];
            /* largest index whose (sorted) entry is <= v */
            int32_t lo = 0;
#pragma unroll
            for (int32_t step = OTBX_Q1_DICT_MAX / 2; step > 0; step >>= 1)
                if (lo + step < nd[c] && tab[lo + step] <= v[c]) lo += step;
            w |= (uint64_t)lo << foff[c];
        }
        uint32_t word = (uint32_t)w;
        bad |= w >> 32 != 0;
        bad |= (int64_t)d.date_base +
                   (int64_t)d_q1c_field(word, d.date_off, d.date_bits) !=
               (int64_t)date;
        bad |= d_q1c_field(word, d.gid_off, d.gid_bits) != gid;
#pragma unroll
        for (int c = 0; c < 3; c++)
            bad |= sdict[c * OTBX_Q1_DICT_MAX +
                         d_q1c_field(word, foff[c], fbits[c])] != v[c];
        codes[i] = word;
    }
    if (bad) atomicOr(&st->flags, Q1C_F_MISMATCH);
    for (int off = WAVE / 2; off > 0; off >>= 1)
        present |= __shfl_down(present, off, WAVE);
    if ((threadIdx.x % WAVE) == 0 && present) atomicOr(&st->present, present);
}

static int32_t q1c_bits_of(uint64_t v)   /* bits needed to hold v; 0 for 0 */
{
    int32_t b = 0;
    while (v) {
        b++;
        v >>= 1;
    }
    return b;
}

extern "C" otbx_status otbx_q1code_plan(int32_t nqty, int32_t ndisc,
                                        int32_t ntax, uint64_t date_span,
                                        otbx_q1code_desc *desc,
                                        int32_t *fits_host)
{
    if (!desc || !fits_host) return OTBX_ERR_INVALID;
    *fits_host = 0;
    const int32_t nd[3] = {nqty, ndisc, ntax};
    for (int c = 0; c < 3; c++)
        if (nd[c] < 1 || nd[c] > OTBX_Q1_DICT_MAX) return OTBX_OK;
    if (date_span > 0xffffffffull) return OTBX_OK;
    /* a field is ceil(log2(size)) bits wide: the bits of its largest code */
    int32_t bits[5] = {q1c_bits_of(date_span), 3,
                       q1c_bits_of((uint64_t)nqty - 1),
                       q1c_bits_of((uint64_t)ndisc - 1),
                       q1c_bits_of((uint64_t)ntax - 1)};
    int32_t off[5], total = 0;
    for (int k = 0; k < 5; k++) {
        off[k] = total;
        total += bits[k];
    }
    if (total > 32) return OTBX_OK;
    desc->date_off = off[0]; desc->date_bits = bits[0];
    desc->gid_off = off[1];  desc->gid_bits = bits[1];
    desc->qty_off = off[2];  desc->qty_bits = bits[2];
    desc->disc_off = off[3]; desc->disc_bits = bits[3];
    desc->tax_off = off[4];  desc->tax_bits = bits[4];
    desc->nqty = nqty;
    desc->ndisc = ndisc;
    desc->ntax = ntax;
    *fits_host = 1;
    return OTBX_OK;
}

extern "C" otbx_status otbx_build_q1codes(const otbx_lineitem_dev *t,
                                          uint32_t *codes_dev,
                                          uint64_t *dict_dev,
                                          otbx_q1code_desc *desc_host,
                                          int32_t *ok_host, void *stream)
{
    if (!t || !desc_host || !ok_host) return OTBX_ERR_INVALID;
    *ok_host = 0;
    if (t->n <= 0 || !t->l_quantity || !t->l_extendedprice ||
        !t->l_discount || !t->l_tax || !t->l_returnflag ||
        !t->l_linestatus || !t->l_shipdate)
        return OTBX_OK;   /* nothing to build: Q1 keeps the raw columns */
    if (!codes_dev || !dict_dev) return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    static q1c_state *d_st = nullptr;
    static q1c_state *h_st = nullptr;
    if (!d_st) SCR_ALLOC_DEV(d_st, sizeof(q1c_state));
    if (!h_st) SCR_ALLOC_HOST(h_st, sizeof(q1c_state));
    memset(h_st, 0xff, sizeof(h_st->set));
    memset(h_st->dict, 0, sizeof(h_st->dict));
    h_st->count[0] = h_st->count[1] = h_st->count[2] = 0;
    h_st->flags = h_st->present = 0;
    h_st->dmin = INT_MAX;
    h_st->dmax = INT_MIN;
    HIP_CHECK(hipMemcpyAsync(d_st, h_st, sizeof(q1c_state),
                             hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_q1c_collect, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       s, t->l_quantity, t->l_discount, t->l_tax,
                       t->l_shipdate, t->n, d_st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_st, d_st, sizeof(q1c_state),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_st->flags) return OTBX_OK;

    /* sorted dictionaries: a code is an index, so codes are deterministic */
    int32_t nd[3];
    for (int c = 0; c < 3; c++) {
        unsigned long long *dict = &h_st->dict[c * OTBX_Q1_DICT_MAX];
        int32_t k = 0;
        for (int i = 0; i < Q1C_GSET; i++)
            if (h_st->set[c][i] != Q1C_EMPTY) {
                if (k == OTBX_Q1_DICT_MAX) return OTBX_OK;
                dict[k++] = h_st->set[c][i];
            }
        std::sort(dict, dict + k);
        nd[c] = k;
    }
    otbx_q1code_desc d;
    memset(&d, 0, sizeof(d));
    int32_t fits = 0;
    otbx_q1code_plan(nd[0], nd[1], nd[2],
                     (uint64_t)((int64_t)h_st->dmax - (int64_t)h_st->dmin), &d,
                     &fits);
    if (!fits) return OTBX_OK;
    d.date_base = h_st->dmin;
    d.dict = dict_dev;
    HIP_CHECK(hipMemcpyAsync(dict_dev, h_st->dict, sizeof(h_st->dict),
                             hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_q1c_encode, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       s, t->l_shipdate, t->l_returnflag, t->l_linestatus,
                       t->l_quantity, t->l_discount, t->l_tax, t->n, d,
                       codes_dev, d_st);
    HIP_CHECK(hipGetLastError());
    /* flags and present are adjacent: one copy */
    HIP_CHECK(hipMemcpyAsync(&h_st->flags, &d_st->flags,
                             2 * sizeof(unsigned int), hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_st->flags) return OTBX_OK;
    d.gid_present = (int32_t)h_st->present;
    *desc_host = d;
    *ok_host = 1;
    return OTBX_OK;
}

/* ---- staging: build the packed Q1 price column (otbx.h q1pcode) ---- */

#define Q1P_NE 5   /* candidate exponents e = 0..4 */

struct q1p_state {   /* device scratch + its pinned host mirror */
    long long dmin[Q1P_NE], dmax[Q1P_NE];
    int kmin[Q1P_NE], kmax[Q1P_NE];
    unsigned int bad[Q1P_NE];
    unsigned int mismatch;   /* encode round trip failed */
};

/* pass 1: per candidate exponent, whether every K = llrint(x * 10^e) is a
 * signed 32-bit integer, and the ranges of K and of the ulp correction
 * delta = bits(x) - bits(fl((double)K * 10^-e)). Lanes reduce per wave, waves
 * per block in LDS, one set of device atomics per block. */
__global__ void k_q1p_collect(const double *__restrict__ price, int64_t n,
                              q1p_state *st)
{
    const double scale[Q1P_NE] = {1.0, 10.0, 100.0, 1000.0, 10000.0};
    const double mul[Q1P_NE] = {1.0, 0.1, 0.01, 0.001, 0.0001};
    __shared__ q1p_state ls;
    if (threadIdx.x < Q1P_NE) {
        ls.dmin[threadIdx.x] = LLONG_MAX;
        ls.dmax[threadIdx.x] = LLONG_MIN;
        ls.kmin[threadIdx.x] = INT_MAX;
        ls.kmax[threadIdx.x] = INT_MIN;
        ls.bad[threadIdx.x] = 0;
    }
    __syncthreads();
    long long dmin[Q1P_NE], dmax[Q1P_NE];
    int kmin[Q1P_NE], kmax[Q1P_NE];
    unsigned int bad[Q1P_NE];
#pragma unroll
    for (int e = 0; e < Q1P_NE; e++) {
        dmin[e] = LLONG_MAX;
        dmax[e] = LLONG_MIN;
        kmin[e] = INT_MAX;
        kmax[e] = INT_MIN;
        bad[e] = 0;
    }
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        double x = price[i];
        unsigned long long xb = (unsigned long long)__double_as_longlong(x);
#pragma unroll
        for (int e = 0; e < Q1P_NE; e++) {
            double y = x * scale[e];
            /* NaN fails the comparison; llrint may still round up to 2^31 */
            long long k = fabs(y) < 2147483648.0 ? llrint(y) : LLONG_MAX;
            if (k > INT_MAX) {
                bad[e] = 1;
                continue;
            }
            double pred = (double)(int)k * mul[e];
            long long d = (long long)(
                xb - (unsigned long long)__double_as_longlong(pred));
            kmin[e] = (int)k < kmin[e] ? (int)k : kmin[e];
            kmax[e] = (int)k > kmax[e] ? (int)k : kmax[e];
            dmin[e] = d < dmin[e] ? d : dmin[e];
            dmax[e] = d > dmax[e] ? d : dmax[e];
        }
    }
#pragma unroll
    for (int e = 0; e < Q1P_NE; e++) {
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            int a = __shfl_down(kmin[e], off, WAVE);
            int b = __shfl_down(kmax[e], off, WAVE);
            long long c = __shfl_down(dmin[e], off, WAVE);
            long long d = __shfl_down(dmax[e], off, WAVE);
            kmin[e] = a < kmin[e] ? a : kmin[e];
            kmax[e] = b > kmax[e] ? b : kmax[e];
            dmin[e] = c < dmin[e] ? c : dmin[e];
            dmax[e] = d > dmax[e] ? d : dmax[e];
            bad[e] |= __shfl_down(bad[e], off, WAVE);
        }
        if ((threadIdx.x % WAVE) == 0) {
            atomicMin(&ls.kmin[e], kmin[e]);
            atomicMax(&ls.kmax[e], kmax[e]);
            atomicMin(&ls.dmin[e], dmin[e]);
            atomicMax(&ls.dmax[e], dmax[e]);
            if (bad[e]) atomicOr(&ls.bad[e], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < Q1P_NE) {
        int e = threadIdx.x;
        atomicMin(&st->kmin[e], ls.kmin[e]);
        atomicMax(&st->kmax[e], ls.kmax[e]);
        atomicMin(&st->dmin[e], ls.dmin[e]);
        atomicMax(&st->dmax[e], ls.dmax[e]);
        if (ls.bad[e]) atomicOr(&st->bad[e], 1u);
    }
}

/* pass 2: one price word per row, then decode that word with the Q1
 * kernel's own d_q1p_decode and compare it bit-for-bit with the source
 * double (k_q1c_encode's rule: the build checks its own round trip). */
__global__ void k_q1p_encode(const double *__restrict__ price, int64_t n,
                             const otbx_q1price_desc d, const q1p_fields pf,
                             double scale, uint32_t *__restrict__ pcodes,
                             q1p_state *st)
{
    unsigned int bad = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        double x = price[i];
        unsigned long long xb = (unsigned long long)__double_as_longlong(x);
        double y = x * scale;
        long long k = fabs(y) < 2147483648.0 ? llrint(y) : LLONG_MAX;
        bad |= k > INT_MAX;
        double pred = (double)(int)k * d.mul;
        unsigned long long delta =
            xb - (unsigned long long)__double_as_longlong(pred);
        uint64_t kf = (uint64_t)k - (uint64_t)(long long)d.k_base;
        uint64_t df = delta - (unsigned long long)(long long)d.d_base;
        bad |= (kf >> 32) != 0 || (df >> 8) != 0;
        uint64_t w = (kf & 0xffffffffull) << d.k_off | (df & 0xffull) << d.d_off;
        uint32_t word = (uint32_t)w;
        bad |= (w >> 32) != 0;
        bad |= (unsigned long long)__double_as_longlong(
                   d_q1p_decode(word, pf)) != xb;
        pcodes[i] = word;
    }
    if (bad) atomicOr(&st->mismatch, 1u);
}

extern "C" otbx_status otbx_q1price_plan(const int32_t *bad,
                                         const int64_t *kmin,
                                         const int64_t *kmax,
                                         const int64_t *dmin,
                                         const int64_t *dmax,
                                         otbx_q1price_desc *desc,
                                         int32_t *fits_host)
{
    if (!bad || !kmin || !kmax || !dmin || !dmax || !desc || !fits_host)
        return OTBX_ERR_INVALID;
    *fits_host = 0;
    int best = -1, best_k = 0, best_d = 0;
    for (int e = 0; e < Q1P_NE; e++) {
        if (bad[e] || kmin[e] > kmax[e] || dmin[e] > dmax[e] ||
            kmin[e] < INT32_MIN || kmax[e] > INT32_MAX ||
            dmin[e] < INT32_MIN || dmax[e] > INT32_MAX)
            continue;
        int32_t kb = q1c_bits_of((uint64_t)kmax[e] - (uint64_t)kmin[e]);
        int32_t db = q1c_bits_of((uint64_t)dmax[e] - (uint64_t)dmin[e]);
        if (db > 8 || kb + db > 32) continue;
        if (best < 0 || kb + db < best_k + best_d) {
            best = e;
            best_k = kb;
            best_d = db;
        }
    }
    if (best < 0) return OTBX_OK;
    desc->scale_exp = best;
    desc->mul = q1p_mul[best];
    desc->k_base = (int32_t)kmin[best];
    desc->k_off = 0;
    desc->k_bits = best_k;
    desc->d_base = (int32_t)dmin[best];
    desc->d_off = best_k;
    desc->d_bits = best_d;
    *fits_host = 1;
    return OTBX_OK;
}

extern "C" otbx_status otbx_build_q1pcodes(const otbx_lineitem_dev *t,
                                           uint32_t *pcodes_dev,
                                           otbx_q1price_desc *desc_host,
                                           int32_t *ok_host, void *stream)
{
    if (!t || !desc_host || !ok_host) return OTBX_ERR_INVALID;
    *ok_host = 0;
    if (t->n <= 0 || !t->q1code || !t->l_extendedprice)
        return OTBX_OK;   /* nothing to build: Q1 keeps l_extendedprice */
    if (!pcodes_dev) return OTBX_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    static q1p_state *d_st = nullptr;
    static q1p_state *h_st = nullptr;
    if (!d_st) SCR_ALLOC_DEV(d_st, sizeof(q1p_state));
    if (!h_st) SCR_ALLOC_HOST(h_st, sizeof(q1p_state));
    for (int e = 0; e < Q1P_NE; e++) {
        h_st->dmin[e] = LLONG_MAX;
        h_st->dmax[e] = LLONG_MIN;
        h_st->kmin[e] = INT_MAX;
        h_st->kmax[e] = INT_MIN;
        h_st->bad[e] = 0;
    }
    h_st->mismatch = 0;
    HIP_CHECK(hipMemcpyAsync(d_st, h_st, sizeof(q1p_state),
                             hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_q1p_collect, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       s, t->l_extendedprice, t->n, d_st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_st, d_st, sizeof(q1p_state),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));

    int32_t bad[Q1P_NE], fits = 0;
    int64_t kmin[Q1P_NE], kmax[Q1P_NE], dmin[Q1P_NE], dmax[Q1P_NE];
    for (int e = 0; e < Q1P_NE; e++) {
        bad[e] = (int32_t)h_st->bad[e];
        kmin[e] = h_st->kmin[e];
        kmax[e] = h_st->kmax[e];
        dmin[e] = h_st->dmin[e];
        dmax[e] = h_st->dmax[e];
    }
    otbx_q1price_desc d;
    memset(&d, 0, sizeof(d));
    otbx_q1price_plan(bad, kmin, kmax, dmin, dmax, &d, &fits);
    if (!fits || !q1p_desc_ok(&d)) return OTBX_OK;
    hipLaunchKernelGGL(k_q1p_encode, dim3(grid_for(t->n, 256)), dim3(256), 0,
                       s, t->l_extendedprice, t->n, d, q1p_fields_of(&d),
                       q1p_scale[d.scale_exp], pcodes_dev, d_st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(&h_st->mismatch, &d_st->mismatch,
                             sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (h_st->mismatch) return OTBX_OK;
    *desc_host = d;
    *ok_host = 1;
    return OTBX_OK;
}


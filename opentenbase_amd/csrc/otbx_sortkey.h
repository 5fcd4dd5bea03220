/*
 * otbx_sortkey.h — the normalised sort key shared by the Sort operator
 * (otbx_sort.hip) and the WindowAgg operator (otbx_window.hip). Both decide
 * "these two rows compare equal on this key" from the same (null digit,
 * normalised bits) pair, so partition / peer boundaries can never disagree
 * with the order the sort produced. The Filter operator (otbx_filter.hip)
 * compares doubles on the same normalisation (ss_norm_f64). Device code only.
 */
#ifndef OTBX_SORTKEY_H
#define OTBX_SORTKEY_H

#include <hip/hip_runtime.h>

#include "../../include/otbx.h"

/* float8_cmp_internal (utils/adt/float.c:1172) as an unsigned order: the
 * returned bits compare (as uint64) exactly as the doubles do under it —
 * every NaN one value above +Inf, -0 == +0. No direction, no NULLs: ss_norm
 * adds those; the Filter operator (otbx_filter.hip) compares these directly. */
__device__ __forceinline__ unsigned long long ss_norm_f64(double d)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(d);
    if (d != d)
        b = 0x7ff8000000000000ull;  /* every NaN: one value, above +Inf */
    else if (d == 0.0)
        b = 0ull;                   /* -0 == +0 */
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}

/* ---- key normalisation ----
 * returns the radix key (wbits wide, zero-extended) and the null digit:
 * NULLS FIRST → NULL 0 / non-NULL 1, NULLS LAST → NULL 1 / non-NULL 0.
 * The value stored under a NULL is never read. */
__device__ __forceinline__ unsigned long long
ss_norm(const otbx_sortkey &k, uint32_t row, uint32_t *nulldigit)
{
    const bool isnull = k.nulls && k.nulls[row];
    const bool nf = (k.flags & OTBX_SORT_NULLS_FIRST) != 0;
    *nulldigit = isnull ? (nf ? 0u : 1u) : (nf ? 1u : 0u);
    if (isnull)
        return 0ull;
    const bool desc = (k.flags & OTBX_SORT_DESC) != 0;
    unsigned long long v;
    switch (k.type) {
    case OTBX_SORT_I64:
        v = (unsigned long long)((const int64_t *)k.col)[row] ^
            0x8000000000000000ull;
        return desc ? ~v : v;
    case OTBX_SORT_F64:
        v = ss_norm_f64(((const double *)k.col)[row]);
        return desc ? ~v : v;
    case OTBX_SORT_I32:
        v = (unsigned long long)((uint32_t)((const int32_t *)k.col)[row] ^
                                 0x80000000u);
        return desc ? (v ^ 0xffffffffull) : v;
    default:
        v = (unsigned long long)((const uint8_t *)k.col)[row];
        return desc ? (v ^ 0xffull) : v;
    }
}

#endif

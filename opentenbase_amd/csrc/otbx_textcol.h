/*
 * otbx_textcol.h — what every unit that reads an otbx_textcol shares: the
 * clamping policy for offsets (into [0, nbytes], a negative length reads as
 * 0) and the host-side column check. Private to csrc/.
 */
#ifndef OTBX_TEXTCOL_H
#define OTBX_TEXTCOL_H

#include "otbx_common.h"

__device__ __forceinline__ int64_t txt_clamp(int64_t v, int64_t hi)
{
    return v < 0 ? 0 : (v > hi ? hi : v);
}

/* row r of a column as (clamped start, length): offsets outside [0, nbytes]
 * are clamped into it and a negative length reads as 0 */
__device__ __forceinline__ void txt_row(const otbx_textcol &c, int64_t r,
                                        int64_t *s, int *len)
{
    const int64_t a = txt_clamp(c.offs[r], c.nbytes);
    const int64_t b = txt_clamp(c.offs[r + 1], c.nbytes);
    *s = a;
    /* a row longer than INT32_MAX cannot exist: nbytes of one column fits
     * the device, the cursors are ints — cut it there */
    const int64_t l = b > a ? b - a : 0;
    *len = l > (int64_t)INT32_MAX ? INT32_MAX : (int)l;
}

static inline bool txt_col_ok(const otbx_textcol *c, int64_t n_src)
{
    if (c->nbytes < 0)
        return false;
    if (c->nbytes > 0 && !c->bytes)
        return false;
    if (n_src > 0 && !c->offs)
        return false;
    return true;
}

#endif /* OTBX_TEXTCOL_H */

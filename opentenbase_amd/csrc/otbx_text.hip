/*
 * otbx_text.hip — variable-width text columns on the GPU: one text predicate
 * per call (otbx_text_pred: LIKE / NOT LIKE and the six comparisons → a
 * bool column plus null mask) and the gather that moves a text column
 * through a selection or a permutation (otbx_text_gather_offsets /
 * otbx_text_gather_bytes). Semantics: textlike / textnlike
 * (utils/adt/like.c:269,290) over MatchText (like_match.c:78) with the
 * fast NextChar of like.c:142; texteq … text_ge (varlena.c:1874-1998) under
 * C collation (varstr_cmp, varlena.c:1624-1629). Contract in include/otbx.h,
 * DESIGN.md §8l.
 *
 * Everything is stream-ordered; kernel boundaries are the only ordering
 * between workgroups.
 *   k_txt_pred<KIND> — one TXT_TILE-row tile per workgroup, one row per
 *                  thread. KIND: LIKE against the prepared pattern, compare
 *                  with the constant, compare with a second column. The
 *                  pattern tokens / constant bytes arrive by value in the
 *                  launch arguments and are copied to LDS once, because the
 *                  matcher indexes them per lane. Two paths, chosen per
 *                  workgroup from offs alone:
 *                    staged — the tile's byte span is copied to LDS with
 *                             16-byte loads (checked bytewise head and tail)
 *                             and the rows are matched from LDS;
 *                    direct — every row is read from global memory, any
 *                             length. Taken with a selection, with a right
 *                             column, when the span exceeds
 *                             TXT_LDS_BUDGET, when an offset of the tile
 *                             lies outside its span (broken offsets), for
 *                             a predicate that stops early in each row (a
 *                             comparison, a pattern without a % before its
 *                             end) unless OTBX_TEXT_STAGE=1, and always
 *                             with OTBX_TEXT_STAGE=0.
 *   k_tg_sum     — gather, pass 1: bytes per TG_TILE output rows.
 *   k_tg_scan    — one workgroup: exclusive scan of the tile sums in place,
 *                  TG_SCAN_THREADS tiles per pass with a register carry;
 *                  writes dst_offs[n].
 *   k_tg_apply   — per tile: block scan of the row lengths + the tile base
 *                  → dst_offs[j].
 *   k_tg_bytes   — the byte copy, balanced over OUTPUT BYTES: workgroup b
 *                  owns dst bytes [b*TGB_SLICE, +TGB_SLICE), finds the rows
 *                  overlapping them by binary search in dst_offs, stages
 *                  their offsets in LDS TGB_ROWS at a time, and each thread
 *                  writes 16 contiguous bytes per step.
 */
#include <stdlib.h>
#include <string.h>

#include "otbx_common.h"
#include "otbx_textcol.h"   /* txt_clamp, txt_row, txt_col_ok */

#define TXT_THREADS 256
#define TXT_TILE TXT_THREADS          /* rows per workgroup */
#define TXT_LDS_BUDGET 32768          /* largest staged span, bytes */
/* the staged window starts at the 16-byte line of its first byte and ends
 * at the line end of its last: up to 15 bytes more on either side */
#define TXT_LDS_BYTES (TXT_LDS_BUDGET + 32)

#define TXT_KIND_LIKE 0
#define TXT_KIND_CONST 1
#define TXT_KIND_COL 2

#define TOK_LIT 0
#define TOK_ANYCHAR 1
#define TOK_ANYSEQ 2

#define TG_THREADS 256
#define TG_TILE TG_THREADS            /* output rows per tile */
#define TG_SCAN_THREADS 1024          /* tiles per scan pass */
#define TGB_THREADS 256
#define TGB_SLICE 16384               /* dst bytes per workgroup */
#define TGB_ROWS 1024                 /* offsets staged per step */

static_assert(OTBX_MAX_TEXT_CONST == 256, "one token per thread");
static_assert(OTBX_MAX_TEXT_CONST <= TXT_THREADS, "LDS copy of the constant");
static_assert(sizeof(otbx_textcol) == 32, "otbx_textcol layout");
static_assert(sizeof(otbx_textpred) == 312, "otbx_textpred layout");
static_assert(TXT_LDS_BYTES % 16 == 0, "whole 16-byte lines");

/* what the kernel gets: the prepared pattern (or the constant) by value */
struct txt_args {
    otbx_textcol l, r;
    int32_t op, utf8, np, _pad;
    uint8_t byte[OTBX_MAX_TEXT_CONST];   /* LIT: the byte; constant bytes */
    uint8_t kind[OTBX_MAX_TEXT_CONST];   /* TOK_* (LIKE only) */
};

/* NextChar (like.c:142): one byte, then every continuation byte; one byte
 * in a single-byte encoding. Never past len. */
template <typename P>
__device__ __forceinline__ int txt_next(P t, int i, int len, bool utf8)
{
    i++;
    if (utf8)
        while (i < len && (t[i] & 0xC0) == 0x80)
            i++;
    return i;
}

/* MatchText without the recursion: two cursors and one restart point, the
 * position after the last any-sequence token. The tokens are normalised
 * (a run of % and _ is k any-char tokens, then one any-sequence), so the
 * token after an any-sequence is a literal or the end. */
template <typename P>
__device__ __forceinline__ bool
txt_like(P t, int len, const uint8_t *tb, const uint8_t *tk, int np, bool utf8)
{
    int i = 0, p = 0, rp = -1, ri = 0;
    while (i < len) {
        const int k = p < np ? (int)tk[p] : -1;
        if (k == TOK_ANYSEQ) {
            if (++p == np)
                return true;
            rp = p;
            ri = i;
        } else if (k == TOK_ANYCHAR) {
            i = txt_next(t, i, len, utf8);
            p++;
        } else if (k == TOK_LIT && t[i] == tb[p]) {
            i++;
            p++;
        } else if (rp >= 0) {
            ri = txt_next(t, ri, len, utf8);
            i = ri;
            p = rp;
        } else {
            return false;
        }
    }
    while (p < np && tk[p] == TOK_ANYSEQ)
        p++;
    return p == np;
}

/* varstr_cmp under C collation: memcmp over the common prefix (unsigned
 * bytes), then the shorter is smaller. <0, 0, >0 */
template <typename P, typename Q>
__device__ __forceinline__ int txt_cmp(P a, int la, Q b, int lb)
{
    const int m = la < lb ? la : lb;
    for (int i = 0; i < m; i++) {
        const int d = (int)a[i] - (int)b[i];
        if (d != 0)
            return d;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

__device__ __forceinline__ bool txt_cmp_op(int op, int c)
{
    switch (op) {
    case OTBX_TXT_EQ: return c == 0;
    case OTBX_TXT_NE: return c != 0;
    case OTBX_TXT_LT: return c < 0;
    case OTBX_TXT_LE: return c <= 0;
    case OTBX_TXT_GT: return c > 0;
    default:          return c >= 0;
    }
}

template <int KIND, typename P>
__device__ __forceinline__ bool
txt_eval(const txt_args &a, P t, int len, const uint8_t *tb, const uint8_t *tk,
         int64_t row)
{
    if (KIND == TXT_KIND_LIKE) {
        const bool m = txt_like(t, len, tb, tk, a.np, a.utf8 != 0);
        return a.op == OTBX_TXT_LIKE ? m : !m;
    }
    if (KIND == TXT_KIND_CONST) {
        if (a.op <= OTBX_TXT_NE && len != a.np)   /* texteq: length first */
            return a.op == OTBX_TXT_NE;
        return txt_cmp_op(a.op, txt_cmp(t, len, tb, a.np));
    }
    int64_t rs;
    int rl;
    txt_row(a.r, row, &rs, &rl);
    if (a.op <= OTBX_TXT_NE && len != rl)
        return a.op == OTBX_TXT_NE;
    return txt_cmp_op(a.op, txt_cmp(t, len, a.r.bytes + rs, rl));
}

template <int KIND>
__global__ __launch_bounds__(TXT_THREADS) void
k_txt_pred(const txt_args a, const int64_t *__restrict__ sel, const uint32_t n,
           const int64_t n_src, const int stage, uint8_t *__restrict__ out,
           uint8_t *__restrict__ out_null)
{
    __shared__ uint4 buf4[TXT_LDS_BYTES / 16];
    __shared__ uint8_t tb[OTBX_MAX_TEXT_CONST], tk[OTBX_MAX_TEXT_CONST];
    uint8_t *buf = (uint8_t *)buf4;

    const uint32_t tile0 = blockIdx.x * (uint32_t)TXT_TILE;   /* < n */
    const uint32_t j = tile0 + threadIdx.x;
    const uint32_t cnt = n - tile0 < (uint32_t)TXT_TILE ? n - tile0
                                                        : (uint32_t)TXT_TILE;
    if (KIND != TXT_KIND_COL && threadIdx.x < OTBX_MAX_TEXT_CONST) {
        tb[threadIdx.x] = a.byte[threadIdx.x];
        tk[threadIdx.x] = a.kind[threadIdx.x];
    }

    const bool live = j < n;
    int64_t row = 0, s = 0;
    int len = 0;
    bool isnull = false;
    if (live) {
        row = sel ? txt_clamp(sel[j], n_src - 1) : (int64_t)j;
        isnull = a.l.nulls && a.l.nulls[row];
        if (KIND == TXT_KIND_COL)
            isnull = isnull || (a.r.nulls && a.r.nulls[row]);
        txt_row(a.l, row, &s, &len);
    }

    /* staged or direct: the same answer in every thread of the workgroup */
    bool staged = false;
    int64_t w0 = 0;   /* global byte index of buf[0] (may be negative) */
    if (KIND != TXT_KIND_COL && stage && !sel) {
        const int64_t lo = txt_clamp(a.l.offs[tile0], a.l.nbytes);
        const int64_t hi = txt_clamp(a.l.offs[tile0 + cnt], a.l.nbytes);
        const bool in = !live || (s >= lo && s + len <= hi);
        staged = __syncthreads_and(in ? 1 : 0) != 0 && hi > lo &&
                 hi - lo <= (int64_t)TXT_LDS_BUDGET;
        if (staged) {
            /* 16-byte lines of the address space that overlap the span */
            const uintptr_t base = (uintptr_t)a.l.bytes;
            const uintptr_t g0 = (base + (uintptr_t)lo) & ~(uintptr_t)15;
            const uintptr_t g1 = (base + (uintptr_t)hi + 15) & ~(uintptr_t)15;
            const uintptr_t end = base + (uintptr_t)a.l.nbytes;
            w0 = (int64_t)(g0 - base);
            const int nlines = (int)((g1 - g0) / 16);   /* <= LDS_BYTES/16 */
            for (int k = threadIdx.x; k < nlines; k += TXT_THREADS) {
                const uintptr_t g = g0 + (uintptr_t)k * 16;
                if (g >= base && g + 16 <= end) {
                    buf4[k] = *(const uint4 *)g;
                } else {   /* head or tail line: only bytes of the column */
                    for (int b = 0; b < 16; b++) {
                        const uintptr_t q = g + b;
                        buf[k * 16 + b] =
                            q >= base && q < end ? *(const uint8_t *)q : 0;
                    }
                }
            }
        }
    }
    __syncthreads();

    if (!live)
        return;
    bool v = false;
    if (!isnull) {
        if (staged)
            v = txt_eval<KIND>(a, (const uint8_t *)buf + (s - w0), len, tb, tk,
                               row);
        else
            v = txt_eval<KIND>(a, a.l.bytes + s, len, tb, tk, row);
    }
    out[j] = v ? 1 : 0;
    if (out_null)
        out_null[j] = isnull ? 1 : 0;
}

/* ---- gather: offsets ---- */

__device__ __forceinline__ int64_t tg_len(const otbx_textcol &c, int64_t n_src,
                                          const int64_t *perm, int64_t j,
                                          int64_t *start)
{
    const int64_t r = txt_clamp(perm[j], n_src - 1);
    const int64_t a = txt_clamp(c.offs[r], c.nbytes);
    const int64_t b = txt_clamp(c.offs[r + 1], c.nbytes);
    *start = a;
    return b > a ? b - a : 0;
}

/* inclusive scan over the workgroup; wsum: one slot per wave. Returns the
 * inclusive prefix and the workgroup total */
template <int THREADS>
__device__ __forceinline__ int64_t tg_block_scan(int64_t mine, int64_t *wsum,
                                                 int64_t *total)
{
    const int lane = (int)(threadIdx.x % WAVE), wid = (int)(threadIdx.x / WAVE);
    int64_t incl = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t x = __shfl_up(incl, o);
        if (lane >= o)
            incl += x;
    }
    if (lane == WAVE - 1)
        wsum[wid] = incl;
    __syncthreads();
    int64_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / WAVE; w++) {
        const int64_t x = wsum[w];
        pre += w < wid ? x : 0;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return pre + incl;
}

__global__ __launch_bounds__(TG_THREADS) void
k_tg_sum(const otbx_textcol c, const int64_t n_src,
         const int64_t *__restrict__ perm, const uint32_t n,
         int64_t *__restrict__ sums)
{
    __shared__ int64_t wsum[TG_THREADS / WAVE];
    const uint32_t j = blockIdx.x * (uint32_t)TG_TILE + threadIdx.x;
    int64_t s, tot;
    const int64_t mine = j < n ? tg_len(c, n_src, perm, j, &s) : 0;
    tg_block_scan<TG_THREADS>(mine, wsum, &tot);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(TG_SCAN_THREADS) void
k_tg_scan(int64_t *sums, const uint32_t ntiles, int64_t *total)
{
    __shared__ int64_t wsum[TG_SCAN_THREADS / WAVE];
    int64_t run = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += TG_SCAN_THREADS) {
        const uint32_t i = c0 + threadIdx.x;
        const int64_t mine = i < ntiles ? sums[i] : 0;
        int64_t tot;
        const int64_t incl = tg_block_scan<TG_SCAN_THREADS>(mine, wsum, &tot);
        if (i < ntiles)
            sums[i] = run + incl - mine;
        run += tot;
    }
    if (threadIdx.x == 0)
        *total = run;
}

__global__ __launch_bounds__(TG_THREADS) void
k_tg_apply(const otbx_textcol c, const int64_t n_src,
           const int64_t *__restrict__ perm, const uint32_t n,
           const int64_t *__restrict__ sums, int64_t *__restrict__ dst_offs)
{
    __shared__ int64_t wsum[TG_THREADS / WAVE];
    const uint32_t j = blockIdx.x * (uint32_t)TG_TILE + threadIdx.x;
    int64_t s, tot;
    const int64_t mine = j < n ? tg_len(c, n_src, perm, j, &s) : 0;
    const int64_t incl = tg_block_scan<TG_THREADS>(mine, wsum, &tot);
    if (j < n)
        dst_offs[j] = sums[blockIdx.x] + incl - mine;
}

/* ---- gather: bytes ----
 * first index in [lo, hi) with v[index] > key (upper bound) */
__device__ __forceinline__ int64_t tg_upper(const int64_t *v, int64_t lo,
                                            int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (v[mid] <= key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TGB_THREADS) void
k_tg_bytes(const otbx_textcol c, const int64_t n_src,
           const int64_t *__restrict__ perm, const int64_t n,
           const int64_t *__restrict__ dst_offs, uint8_t *__restrict__ dst,
           const int64_t dst_nbytes)
{
    __shared__ int64_t doff[TGB_ROWS + 1];   /* dst offset of each row */
    __shared__ int64_t sbeg[TGB_ROWS];       /* clamped src start */

    int64_t tot = dst_offs[n];
    tot = tot < dst_nbytes ? tot : dst_nbytes;
    const int64_t b0 = (int64_t)blockIdx.x * TGB_SLICE;
    if (b0 >= tot)
        return;   /* uniform */
    const int64_t b1 = b0 + TGB_SLICE < tot ? b0 + TGB_SLICE : tot;

    /* rows [jlo, jhi) cover dst bytes [b0, b1): jlo is the last row that
     * starts at or before b0, jhi the first that starts at or after b1 */
    int64_t jlo = tg_upper(dst_offs, 0, n, b0) - 1;
    if (jlo < 0)
        jlo = 0;
    int64_t jhi = tg_upper(dst_offs, jlo, n, b1 - 1);
    if (jhi <= jlo)
        jhi = jlo + 1;

    /* 16-byte groups are lines of the destination's address space */
    const int64_t shift = (int64_t)((uintptr_t)dst & 15u);

    for (int64_t j0 = jlo; j0 < jhi; j0 += TGB_ROWS) {
        const int cnt = (int)(jhi - j0 < TGB_ROWS ? jhi - j0 : TGB_ROWS);
        __syncthreads();   /* the previous step's readers are done */
        for (int k = threadIdx.x; k <= cnt; k += TGB_THREADS) {
            doff[k] = dst_offs[j0 + k];
            if (k < cnt) {
                int64_t s;
                tg_len(c, n_src, perm, j0 + k, &s);
                sbeg[k] = s;
            }
        }
        __syncthreads();
        int64_t lo = doff[0] > b0 ? doff[0] : b0;
        int64_t hi = doff[cnt] < b1 ? doff[cnt] : b1;
        if (hi <= lo)
            continue;   /* uniform: empty rows only */
        const int64_t g0 = (lo + shift) / 16, g1 = (hi + shift + 15) / 16;
        for (int64_t g = g0 + threadIdx.x; g < g1; g += TGB_THREADS) {
            int64_t p = g * 16 - shift, pe = p + 16;
            const bool whole = p >= lo && pe <= hi;
            p = p > lo ? p : lo;
            pe = pe < hi ? pe : hi;
            /* the row that holds byte p: the last one starting at or
             * before it */
            int r = (int)tg_upper(doff, 0, cnt, p) - 1;
            r = r < 0 ? 0 : r;
            uint8_t v[16];
            const int m = (int)(pe - p);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < m) {
                    const int64_t q = p + k;
                    while (r + 1 < cnt && doff[r + 1] <= q)
                        r++;
                    const int64_t si = sbeg[r] + (q - doff[r]);
                    /* offsets that do not belong to this column and perm
                     * can never read outside bytes */
                    v[k] = si >= 0 && si < c.nbytes ? c.bytes[si] : 0;
                }
            }
            if (whole) {
                uint4 w;
                __builtin_memcpy(&w, v, 16);
                *(uint4 *)(dst + p) = w;
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (k < m)
                        dst[p + k] = v[k];
            }
        }
    }
}

/* ---- host side ---- */

/* pattern → tokens, on the host: literal / any-char / any-sequence, a run
 * of % and _ normalised to "k characters, then any sequence"
 * (like_match.c:128-144). false: the pattern ends in a lone escape */
static bool txt_prepare_like(const uint8_t *pat, int plen, txt_args *a)
{
    int np = 0, i = 0;
    while (i < plen) {
        if (pat[i] == '%' || pat[i] == '_') {
            int nchar = 0;
            bool seq = false;
            for (; i < plen && (pat[i] == '%' || pat[i] == '_'); i++) {
                if (pat[i] == '%')
                    seq = true;
                else
                    nchar++;
            }
            for (int k = 0; k < nchar; k++) {
                a->kind[np] = TOK_ANYCHAR;
                a->byte[np++] = 0;
            }
            if (seq) {
                a->kind[np] = TOK_ANYSEQ;
                a->byte[np++] = 0;
            }
            continue;
        }
        if (pat[i] == '\\') {
            if (++i >= plen)
                return false;
        }
        a->kind[np] = TOK_LIT;
        a->byte[np++] = pat[i++];
    }
    a->np = np;
    return true;
}

static bool txt_gather_args_ok(const otbx_textcol *src, int64_t n_src,
                               const int64_t *perm_dev, int64_t n)
{
    if (!src || n < 0 || n > INT32_MAX || n_src < 0)
        return false;
    if (n > 0 && (!perm_dev || n_src == 0))
        return false;
    return txt_col_ok(src, n_src);
}

static size_t tg_ws_bytes(int64_t n)
{
    return align256_sz((size_t)((n + TG_TILE - 1) / TG_TILE) * sizeof(int64_t));
}

extern "C" {

otbx_status otbx_text_pred(const otbx_textpred *p, const int64_t *sel_dev,
                           int64_t n, int64_t n_src, uint8_t *out_dev,
                           uint8_t *out_null_dev, void *stream)
{
    /* argument checks and the pattern preparation first: nothing in this
     * block touches HIP */
    if (!p)
        return OTBX_ERR_INVALID;
    if (p->op < OTBX_TXT_LIKE || p->op > OTBX_TXT_GE)
        return OTBX_ERR_INVALID;
    if (p->encoding != OTBX_TEXT_SB && p->encoding != OTBX_TEXT_UTF8)
        return OTBX_ERR_INVALID;
    if (p->clen < 0 || p->clen > OTBX_MAX_TEXT_CONST)
        return OTBX_ERR_INVALID;
    if (p->right && (p->op <= OTBX_TXT_NLIKE || p->clen != 0))
        return OTBX_ERR_INVALID;
    if (n < 0 || n > INT32_MAX || n_src < 0)
        return OTBX_ERR_INVALID;
    if (!sel_dev && n > n_src)
        return OTBX_ERR_INVALID;
    if (n > 0 && (n_src == 0 || !out_dev))
        return OTBX_ERR_INVALID;
    if (!txt_col_ok(&p->left, n_src))
        return OTBX_ERR_INVALID;
    if (p->right && !txt_col_ok(p->right, n_src))
        return OTBX_ERR_INVALID;
    if (!out_null_dev && (p->left.nulls || (p->right && p->right->nulls)))
        return OTBX_ERR_INVALID;

    txt_args a;
    memset(&a, 0, sizeof a);
    a.l = p->left;
    a.op = p->op;
    a.utf8 = p->encoding == OTBX_TEXT_UTF8;
    int kind;
    if (p->right) {
        kind = TXT_KIND_COL;
        a.r = *p->right;
    } else if (p->op <= OTBX_TXT_NLIKE) {
        kind = TXT_KIND_LIKE;
        if (!txt_prepare_like(p->cbytes, p->clen, &a))
            return OTBX_ERR_INVALID;
    } else {
        kind = TXT_KIND_CONST;
        memcpy(a.byte, p->cbytes, (size_t)p->clen);
        a.np = p->clen;
    }
    if (n == 0)
        return OTBX_OK;

    /* staging pays when the rows are read to their end: a LIKE with an
     * any-sequence token before its last token (%green%: 0.85 x the direct
     * time, %special%requests%: 0.79 x). A comparison or a pattern like
     * forest% stops after a few bytes of each row and is faster direct
     * (staged 1.04 x and 1.11 x; profiles/text_ops.txt). OTBX_TEXT_STAGE=0
     * / =1 overrides the rule either way */
    int stage = 0;
    if (kind == TXT_KIND_LIKE)
        for (int k = 0; k + 1 < a.np; k++)
            stage |= a.kind[k] == TOK_ANYSEQ;
    const char *e = getenv("OTBX_TEXT_STAGE");
    if (e && (e[0] == '0' || e[0] == '1') && e[1] == '\0')
        stage = e[0] == '1';
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((uint32_t)((n + TXT_TILE - 1) / TXT_TILE));
    const uint32_t un = (uint32_t)n;
    if (kind == TXT_KIND_LIKE)
        hipLaunchKernelGGL(k_txt_pred<TXT_KIND_LIKE>, grid, dim3(TXT_THREADS),
                           0, s, a, sel_dev, un, n_src, stage, out_dev,
                           out_null_dev);
    else if (kind == TXT_KIND_CONST)
        hipLaunchKernelGGL(k_txt_pred<TXT_KIND_CONST>, grid, dim3(TXT_THREADS),
                           0, s, a, sel_dev, un, n_src, stage, out_dev,
                           out_null_dev);
    else
        hipLaunchKernelGGL(k_txt_pred<TXT_KIND_COL>, grid, dim3(TXT_THREADS),
                           0, s, a, sel_dev, un, n_src, stage, out_dev,
                           out_null_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_text_gather_workspace_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > INT32_MAX)
        return OTBX_ERR_INVALID;
    *bytes = tg_ws_bytes(n);
    return OTBX_OK;
}

otbx_status otbx_text_gather_offsets(const otbx_textcol *src, int64_t n_src,
                                     const int64_t *perm_dev, int64_t n,
                                     void *ws_dev, size_t ws_bytes,
                                     int64_t *dst_offs_dev, void *stream)
{
    if (!txt_gather_args_ok(src, n_src, perm_dev, n) || !dst_offs_dev)
        return OTBX_ERR_INVALID;
    const size_t need = tg_ws_bytes(n);
    if (ws_bytes < need || (need > 0 && !ws_dev) || ((uintptr_t)ws_dev & 7u))
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    const uint32_t ntiles = (uint32_t)((n + TG_TILE - 1) / TG_TILE);
    int64_t *sums = (int64_t *)ws_dev;
    if (ntiles > 0)
        hipLaunchKernelGGL(k_tg_sum, dim3(ntiles), dim3(TG_THREADS), 0, s,
                           *src, n_src, perm_dev, (uint32_t)n, sums);
    /* with no tiles this only writes dst_offs[0] = 0 */
    hipLaunchKernelGGL(k_tg_scan, dim3(1), dim3(TG_SCAN_THREADS), 0, s, sums,
                       ntiles, dst_offs_dev + n);
    if (ntiles > 0)
        hipLaunchKernelGGL(k_tg_apply, dim3(ntiles), dim3(TG_THREADS), 0, s,
                           *src, n_src, perm_dev, (uint32_t)n,
                           (const int64_t *)sums, dst_offs_dev);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

otbx_status otbx_text_gather_bytes(const otbx_textcol *src, int64_t n_src,
                                   const int64_t *perm_dev, int64_t n,
                                   const int64_t *dst_offs_dev,
                                   uint8_t *dst_bytes_dev, int64_t dst_nbytes,
                                   void *stream)
{
    if (!txt_gather_args_ok(src, n_src, perm_dev, n) || !dst_offs_dev)
        return OTBX_ERR_INVALID;
    if (dst_nbytes < 0 || (dst_nbytes > 0 && !dst_bytes_dev))
        return OTBX_ERR_INVALID;
    const int64_t nslices = (dst_nbytes + TGB_SLICE - 1) / TGB_SLICE;
    if (nslices > INT32_MAX)
        return OTBX_ERR_INVALID;
    if (n == 0 || dst_nbytes == 0)
        return OTBX_OK;
    hipLaunchKernelGGL(k_tg_bytes, dim3((uint32_t)nslices), dim3(TGB_THREADS),
                       0, (hipStream_t)stream, *src, n_src, perm_dev, n,
                       dst_offs_dev, dst_bytes_dev, dst_nbytes);
    HIP_CHECK(hipGetLastError());
    return OTBX_OK;
}

} /* extern "C" */

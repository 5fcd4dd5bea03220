/*
 * otbx_project.hip — the generic GPU Project operator (otbx_project): one
 * typed scalar expression, given as a postfix program, evaluated per row
 * into an output column plus null mask, optionally through a selection
 * vector. The ExecProject analog over the expression interpreter
 * (executor/execExprInterp.c; operators utils/adt/int8.c:534-685,
 * utils/adt/float.c:809-1025 with CHECKFLOATVAL :58; casts int8.c:1201-1265).
 * Contract in include/otbx.h, DESIGN.md §8j.
 *
 * The host type-checks the program by abstract interpretation and lowers it
 * to typed device instructions, each annotated with the stack slot it
 * writes. One kernel, one pass, nothing shared between workgroups but the
 * error slot:
 *   k_prj_eval — one PRJ_TILE-row tile per workgroup, PRJ_ITEMS consecutive
 *                rows per thread. The instruction loop is wave-uniform (the
 *                program lives in the kernel arguments): per instruction the
 *                operands are copied out of the value stack by a switch on
 *                the annotated slot, the operator runs on fixed registers
 *                and the result is copied back the same way, so every stack
 *                index is a compile-time constant and the stack stays in
 *                VGPRs (8 slots × 4 rows × 8 B + one word of null bits and
 *                one of error codes per slot). A leaf is loaded straight
 *                into its slot, so the loads of neighbouring leaves are in
 *                flight together. Two instances: programs no deeper than 4
 *                run the one without the upper four slots, at twice the
 *                occupancy. Evaluation is eager; an error
 *                is a code carried beside the value (byte i of `err` = row
 *                i) and merged by the rules of the header, so the untaken
 *                arm of a CASE never raises. A wave with a raising row
 *                reduces (row << 8 | code) to its minimum and issues one
 *                64-bit atomicMin on the slot, preset to all-ones = -1.
 */
#include "otbx_common.h"
#include "otbx_sortkey.h"   /* ss_norm_f64: float8_cmp_internal as an order */

#define PRJ_THREADS 256
#define PRJ_ITEMS 4
#define PRJ_TILE (PRJ_THREADS * PRJ_ITEMS)   /* 1024 rows per tile */
#define PRJ_ALL 0xfu                         /* all PRJ_ITEMS rows of a thread */

static_assert(PRJ_ITEMS == 4, "one byte of error code per row in a uint32");
static_assert(sizeof(otbx_exprinstr) == 48, "otbx_exprinstr layout");
static_assert(sizeof(otbx_expr) == 1544, "otbx_expr layout");
static_assert(OTBX_MAX_EXPR_DEPTH == 8, "PRJ_GET / PRJ_PUT switch on 8 slots");

/* device opcodes: the public ones with the operand type resolved */
enum { PJ_LD8 = 0, PJ_LD_I32, PJ_LD_U8, PJ_CONST,
       PJ_I_ADD, PJ_I_SUB, PJ_I_MUL, PJ_I_DIV, PJ_I_MOD, PJ_I_NEG, PJ_I_ABS,
       PJ_F_ADD, PJ_F_SUB, PJ_F_MUL, PJ_F_DIV, PJ_F_NEG, PJ_F_ABS,
       PJ_I2F, PJ_F2I, PJ_I_CMP, PJ_F_CMP, PJ_NOT,
       PJ_AND, PJ_OR, PJ_ISNULL, PJ_NOTNULL, PJ_CASE, PJ_COALESCE };
enum { PJ_OUT_8 = 0, PJ_OUT_I32, PJ_OUT_U8 };

struct prj_instr {
    const void *col;          /* loads */
    const uint8_t *nulls;
    unsigned long long imm;   /* PJ_CONST: the value's bits */
    int32_t op;               /* PJ_* */
    int16_t dst;              /* stack slot of the result = of the first operand */
    int16_t aux;              /* PJ_CONST: is NULL; PJ_*_CMP: OTBX_CMP_EQ..GE */
};
struct prj_prog {
    int32_t ninstr;
    int32_t out_kind;         /* PJ_OUT_* */
    prj_instr instr[OTBX_MAX_EXPR_INSTRS];
};
static_assert(sizeof(prj_instr) == 32, "prj_instr layout");

/* the thread's rows of one stack slot: value bits, null bit i and error
 * byte i for row i */
struct prj_val {
    unsigned long long v[PRJ_ITEMS];
    uint32_t nul, err;
};

/* the value stack is eight local variables of the kernel, s0 .. s7, reached
 * only through these switches on a wave-uniform slot number: every access
 * has a constant address, so the stack is promoted to registers. Macros, not
 * functions: behind a reference parameter the eight copies are merged into
 * one access through a selected pointer before the function is inlined, and
 * the stack then stays in scratch. DEPTH is the kernel's template argument:
 * the instance for programs no deeper than 4 never touches s4 .. s7, which
 * then cost no registers. */
#define PRJ_SLOT_SWITCH(d, X)                                                 \
    if (DEPTH <= 4 || (d) < 4) {                                              \
        switch (d) {                                                          \
        case 0: X(s0); break;                                                 \
        case 1: X(s1); break;                                                 \
        case 2: X(s2); break;                                                 \
        default: X(s3); break;                                                \
        }                                                                     \
    } else {                                                                  \
        switch (d) {                                                          \
        case 4: X(s4); break;                                                 \
        case 5: X(s5); break;                                                 \
        case 6: X(s6); break;                                                 \
        default: X(s7); break;                                                \
        }                                                                     \
    }
#define PRJ_GET(r, d)                                                         \
    prj_val r;                                                                \
    PRJ_SLOT_SWITCH(d, r = )
#define PRJ_PUT_X(slot) slot = r
#define PRJ_PUT(d) PRJ_SLOT_SWITCH(d, PRJ_PUT_X)   /* r → slot d */
#define PRJ_LEAF_X(slot) prj_leaf(in, gather, row, p0, n, whole, slot)

__device__ __forceinline__ uint32_t prj_err(uint32_t e, int i)
{
    return (e >> (8 * i)) & 0xffu;
}

/* error bytes of a strict operator: the first operand's, else the second's,
 * else its own where no operand is NULL */
__device__ __forceinline__ uint32_t prj_strict(uint32_t ea, uint32_t eb,
                                               uint32_t nul, uint32_t own)
{
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < PRJ_ITEMS; i++) {
        const uint32_t a = prj_err(ea, i), b = prj_err(eb, i);
        const uint32_t o = (nul >> i) & 1u ? 0u : prj_err(own, i);
        out |= (a ? a : (b ? b : o)) << (8 * i);
    }
    return out;
}

/* the thread's rows of a column as T. Identity: rows p0 .. p0+3, one or two
 * 16-byte loads (4 bytes for a byte column) where the column is 16-byte
 * aligned and the tile whole, checked scalar loads otherwise. Selection:
 * a gather through the clamped row ids. Rows past n read as 0. */
template <typename T>
__device__ __forceinline__ void prj_load(const void *col, bool gather,
                                         const int64_t (&row)[PRJ_ITEMS],
                                         uint32_t p0, uint32_t n, bool whole,
                                         T (&v)[PRJ_ITEMS])
{
    if (gather) {
        const T *c = (const T *)col;
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            v[i] = p0 + i < n ? c[row[i]] : (T)0;
        return;
    }
    const T *c = (const T *)col + p0;
    if (whole && ((uintptr_t)col & 15u) == 0) {
        if constexpr (sizeof(T) == 8) {
            const uint4 *c4 = (const uint4 *)c;
            const uint4 w0 = c4[0], w1 = c4[1];
            __builtin_memcpy(&v[0], &w0, 16);
            __builtin_memcpy(&v[2], &w1, 16);
        } else if constexpr (sizeof(T) == 4) {
            const uint4 w = *(const uint4 *)c;
            __builtin_memcpy(&v[0], &w, 16);
        } else {
            const uint32_t w = *(const uint32_t *)c;
            __builtin_memcpy(&v[0], &w, 4);
        }
    } else {
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            v[i] = p0 + i < n ? c[i] : (T)0;
    }
}

/* the thread's rows of an output array: the mirror of prj_load's identity
 * side */
template <typename T>
__device__ __forceinline__ void prj_store(void *out, uint32_t p0, uint32_t n,
                                          bool whole,
                                          const T (&v)[PRJ_ITEMS])
{
    T *o = (T *)out + p0;
    if (whole && ((uintptr_t)out & 15u) == 0) {
        if constexpr (sizeof(T) == 8) {
            uint4 w0, w1;
            __builtin_memcpy(&w0, &v[0], 16);
            __builtin_memcpy(&w1, &v[2], 16);
            ((uint4 *)o)[0] = w0;
            ((uint4 *)o)[1] = w1;
        } else if constexpr (sizeof(T) == 4) {
            uint4 w;
            __builtin_memcpy(&w, &v[0], 16);
            *(uint4 *)o = w;
        } else {
            uint32_t w;
            __builtin_memcpy(&w, &v[0], 4);
            *(uint32_t *)o = w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            if (p0 + i < n)
                o[i] = v[i];
    }
}

__device__ __forceinline__ double prj_f(unsigned long long b)
{
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ unsigned long long prj_b(double d)
{
    return (unsigned long long)__double_as_longlong(d);
}
__device__ __forceinline__ bool prj_isinf(double d)
{
    return (prj_b(d) & 0x7fffffffffffffffull) == 0x7ff0000000000000ull;
}

/* CHECKFLOATVAL (float.c:58) as a code */
__device__ __forceinline__ uint32_t prj_checkfloat(double r, bool inf_ok,
                                                   bool zero_ok)
{
    if (prj_isinf(r) && !inf_ok)
        return OTBX_EXERR_OVERFLOW;
    if (r == 0.0 && !zero_ok)
        return OTBX_EXERR_UNDERFLOW;
    return 0u;
}

/* one strict arithmetic / cast / comparison operator on row values: the
 * result bits, *own = the operator's own error code (0 = none). Total for
 * every input: what lies under a NULL reaches it too. */
__device__ __forceinline__ unsigned long long
prj_scalar(int op, int aux, unsigned long long ua, unsigned long long ub,
           uint32_t *own)
{
    const int64_t a = (int64_t)ua, b = (int64_t)ub;
    const double x = prj_f(ua), y = prj_f(ub);
    const int64_t imin = INT64_MIN;
    uint32_t e = 0;
    unsigned long long r = 0;
    switch (op) {
    case PJ_I_ADD: {
        int64_t t;
        e = __builtin_add_overflow(a, b, &t) ? OTBX_EXERR_INT8 : 0u;
        r = (unsigned long long)t;
        break;
    }
    case PJ_I_SUB: {
        int64_t t;
        e = __builtin_sub_overflow(a, b, &t) ? OTBX_EXERR_INT8 : 0u;
        r = (unsigned long long)t;
        break;
    }
    case PJ_I_MUL: {
        int64_t t;
        e = __builtin_mul_overflow(a, b, &t) ? OTBX_EXERR_INT8 : 0u;
        r = (unsigned long long)t;
        break;
    }
    case PJ_I_DIV:
    case PJ_I_MOD: {
        /* the divisions themselves only ever see a divisor that is neither
         * 0 nor -1 */
        const bool special = b == 0 || b == -1;
        const int64_t bs = special ? 1 : b;
        if (op == PJ_I_DIV) {
            e = b == 0 ? OTBX_EXERR_DIV0
                       : (b == -1 && a == imin ? OTBX_EXERR_INT8 : 0u);
            r = special ? 0ull - ua : (unsigned long long)(a / bs);
        } else {
            e = b == 0 ? OTBX_EXERR_DIV0 : 0u;
            r = special ? 0ull : (unsigned long long)(a % bs);
        }
        break;
    }
    case PJ_I_NEG:
        e = a == imin ? OTBX_EXERR_INT8 : 0u;
        r = 0ull - ua;
        break;
    case PJ_I_ABS:
        e = a == imin ? OTBX_EXERR_INT8 : 0u;
        r = a < 0 ? 0ull - ua : ua;
        break;
    case PJ_F_ADD: {
        const double t = x + y;
        e = prj_checkfloat(t, prj_isinf(x) || prj_isinf(y), true);
        r = prj_b(t);
        break;
    }
    case PJ_F_SUB: {
        const double t = x - y;
        e = prj_checkfloat(t, prj_isinf(x) || prj_isinf(y), true);
        r = prj_b(t);
        break;
    }
    case PJ_F_MUL: {
        const double t = x * y;
        e = prj_checkfloat(t, prj_isinf(x) || prj_isinf(y),
                           x == 0.0 || y == 0.0);
        r = prj_b(t);
        break;
    }
    case PJ_F_DIV: {
        const double t = x / y;
        e = y == 0.0 ? OTBX_EXERR_DIV0
                     : prj_checkfloat(t, prj_isinf(x) || prj_isinf(y),
                                      x == 0.0);
        r = prj_b(t);
        break;
    }
    case PJ_F_NEG:
        r = ua ^ 0x8000000000000000ull;
        break;
    case PJ_F_ABS:
        r = ua & 0x7fffffffffffffffull;
        break;
    case PJ_I2F:
        r = prj_b((double)a);
        break;
    case PJ_F2I: {
        /* dtoi8: 2^63 itself is refused (the header says why) */
        const double t = __builtin_rint(x);
        const bool ok = t >= -9223372036854775808.0 &&
                        t < 9223372036854775808.0;   /* false for NaN */
        e = ok ? 0u : OTBX_EXERR_INT8;
        r = ok ? (unsigned long long)(int64_t)t : 0ull;
        break;
    }
    case PJ_I_CMP:
    case PJ_F_CMP: {
        bool lt, eq;
        if (op == PJ_I_CMP) {
            lt = a < b;
            eq = a == b;
        } else {
            const unsigned long long ka = ss_norm_f64(x), kb = ss_norm_f64(y);
            lt = ka < kb;
            eq = ka == kb;
        }
        bool t;
        switch (aux) {
        case OTBX_CMP_EQ: t = eq; break;
        case OTBX_CMP_NE: t = !eq; break;
        case OTBX_CMP_LT: t = lt; break;
        case OTBX_CMP_LE: t = lt || eq; break;
        case OTBX_CMP_GT: t = !(lt || eq); break;
        default:          t = !lt; break;
        }
        r = t ? 1ull : 0ull;
        break;
    }
    default:   /* PJ_NOT */
        r = ua ^ 1ull;
        break;
    }
    *own = e;
    return r;
}

/* a leaf: the thread's rows of a column (widened to 64 bits) with its null
 * bits, or a constant */
__device__ __forceinline__ void
prj_leaf(const prj_instr &in, bool gather, const int64_t (&row)[PRJ_ITEMS],
         uint32_t p0, uint32_t n, bool whole, prj_val &r)
{
    const int op = in.op;
    r.nul = 0u;
    r.err = 0u;
    if (op == PJ_CONST) {
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            r.v[i] = in.imm;
        r.nul = in.aux ? PRJ_ALL : 0u;
        return;
    }
    if (op == PJ_LD8) {
        prj_load<unsigned long long>(in.col, gather, row, p0, n, whole, r.v);
    } else if (op == PJ_LD_I32) {
        int32_t t[PRJ_ITEMS];
        prj_load<int32_t>(in.col, gather, row, p0, n, whole, t);
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            r.v[i] = (unsigned long long)(int64_t)t[i];
    } else {
        uint8_t t[PRJ_ITEMS];
        prj_load<uint8_t>(in.col, gather, row, p0, n, whole, t);
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            r.v[i] = t[i];
    }
    if (in.nulls) {
        uint8_t m[PRJ_ITEMS];
        prj_load<uint8_t>(in.nulls, gather, row, p0, n, whole, m);
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            r.nul |= (m[i] ? 1u : 0u) << i;
    }
}

template <int DEPTH>
__global__ __launch_bounds__(PRJ_THREADS) void
k_prj_eval(const prj_prog prog, const int64_t *__restrict__ sel,
           const uint32_t n, const int64_t n_src, void *__restrict__ out,
           uint8_t *__restrict__ out_null, unsigned long long *err_slot)
{
    const uint32_t tile0 = blockIdx.x * (uint32_t)PRJ_TILE;
    const uint32_t p0 = tile0 + threadIdx.x * PRJ_ITEMS;
    const bool whole = n - tile0 >= (uint32_t)PRJ_TILE;   /* tile0 < n */
    const uint32_t valid = p0 >= n ? 0u
                           : (n - p0 >= PRJ_ITEMS ? PRJ_ALL
                                                  : (1u << (n - p0)) - 1u);
    const bool gather = sel != nullptr;

    /* source rows under a selection, clamped into [0, n_src) (n_src > 0) */
    int64_t row[PRJ_ITEMS];
#pragma unroll
    for (int i = 0; i < PRJ_ITEMS; i++)
        row[i] = 0;
    if (gather) {
        int64_t dummy[PRJ_ITEMS] = {0, 0, 0, 0};
        prj_load<int64_t>(sel, false, dummy, p0, n, whole, row);
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            row[i] = row[i] < 0 ? 0 : (row[i] >= n_src ? n_src - 1 : row[i]);
    }

    prj_val s0 = {}, s1 = {}, s2 = {}, s3 = {}, s4 = {}, s5 = {}, s6 = {},
            s7 = {};

    for (int pc = 0; pc < prog.ninstr; pc++) {
        const prj_instr &in = prog.instr[pc];
        const int op = in.op, dst = in.dst;
        prj_val r;
        r.nul = 0u;
        r.err = 0u;
        if (op <= PJ_CONST) {
            /* a leaf is written straight into its slot, not through r: the
             * wait for a column's loads then sits at the first operator that
             * reads the slot, and the loads of neighbouring leaves overlap */
            PRJ_SLOT_SWITCH(dst, PRJ_LEAF_X)
            continue;
        }
        if (op <= PJ_NOT) {
            /* ---- strict operators on one or two values ---- */
            const bool binary = op <= PJ_I_MOD ||
                                (op >= PJ_F_ADD && op <= PJ_F_DIV) ||
                                op == PJ_I_CMP || op == PJ_F_CMP;
            PRJ_GET(a, dst);
            prj_val b = a;
            uint32_t eb = 0u;
            if (binary) {
                PRJ_GET(b2, dst + 1);
                b = b2;
                eb = b.err;
            }
            uint32_t own = 0u;
            const int aux = in.aux;
#pragma unroll
            for (int i = 0; i < PRJ_ITEMS; i++) {
                uint32_t o;
                r.v[i] = prj_scalar(op, aux, a.v[i], b.v[i], &o);
                own |= o << (8 * i);
            }
            r.nul = a.nul | (binary ? b.nul : 0u);
            r.err = prj_strict(a.err, eb, r.nul, own);
        } else if (op <= PJ_OR) {
            /* ---- Kleene AND / OR: `dec` is the left value that decides ---- */
            PRJ_GET(a, dst);
            PRJ_GET(b, dst + 1);
            const unsigned long long dec = op == PJ_AND ? 0ull : 1ull;
#pragma unroll
            for (int i = 0; i < PRJ_ITEMS; i++) {
                const bool an = (a.nul >> i) & 1u, bn = (b.nul >> i) & 1u;
                const bool adec = !an && a.v[i] == dec;
                const bool bdec = !bn && b.v[i] == dec;
                const bool isnull = !adec && !bdec && (an || bn);
                r.v[i] = (adec || bdec) ? dec : (isnull ? 0ull : dec ^ 1ull);
                r.nul |= (isnull ? 1u : 0u) << i;
                const uint32_t ea = prj_err(a.err, i);
                r.err |= (ea ? ea : (adec ? 0u : prj_err(b.err, i))) << (8 * i);
            }
        } else if (op <= PJ_NOTNULL) {
            PRJ_GET(a, dst);
#pragma unroll
            for (int i = 0; i < PRJ_ITEMS; i++) {
                const unsigned long long isn = (a.nul >> i) & 1u;
                r.v[i] = op == PJ_ISNULL ? isn : isn ^ 1ull;
            }
            r.err = a.err;
        } else if (op == PJ_CASE) {
            PRJ_GET(c, dst);
            PRJ_GET(t, dst + 1);
            PRJ_GET(f, dst + 2);
#pragma unroll
            for (int i = 0; i < PRJ_ITEMS; i++) {
                const bool take = !((c.nul >> i) & 1u) && c.v[i] != 0ull;
                r.v[i] = take ? t.v[i] : f.v[i];
                r.nul |= (((take ? t.nul : f.nul) >> i) & 1u) << i;
                const uint32_t ec = prj_err(c.err, i);
                r.err |= (ec ? ec : prj_err(take ? t.err : f.err, i))
                         << (8 * i);
            }
        } else {   /* PJ_COALESCE */
            PRJ_GET(a, dst);
            PRJ_GET(b, dst + 1);
#pragma unroll
            for (int i = 0; i < PRJ_ITEMS; i++) {
                const bool an = (a.nul >> i) & 1u;
                r.v[i] = an ? b.v[i] : a.v[i];
                r.nul |= (an ? (b.nul >> i) & 1u : 0u) << i;
                const uint32_t ea = prj_err(a.err, i);
                r.err |= (ea ? ea : (an ? prj_err(b.err, i) : 0u)) << (8 * i);
            }
        }
        PRJ_PUT(dst);
    }

    /* ---- result → output column, mask, error slot ---- */
    const prj_val top = s0;
    uint32_t err = top.err;
    if (prog.out_kind == PJ_OUT_8) {
        unsigned long long o[PRJ_ITEMS];
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            o[i] = (top.nul >> i) & 1u ? 0ull : top.v[i];
        prj_store<unsigned long long>(out, p0, n, whole, o);
    } else if (prog.out_kind == PJ_OUT_I32) {
        int32_t o[PRJ_ITEMS];
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++) {
            const bool isn = (top.nul >> i) & 1u;
            const int64_t v = (int64_t)top.v[i];
            /* int84 (int8.c:1201) */
            if (!isn && prj_err(err, i) == 0u && (v < INT32_MIN || v > INT32_MAX))
                err |= (uint32_t)OTBX_EXERR_INT4 << (8 * i);
            o[i] = isn ? 0 : (int32_t)v;
        }
        prj_store<int32_t>(out, p0, n, whole, o);
    } else {
        uint8_t o[PRJ_ITEMS];
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            o[i] = (top.nul >> i) & 1u ? 0 : (uint8_t)(top.v[i] != 0ull);
        prj_store<uint8_t>(out, p0, n, whole, o);
    }
    if (out_null) {
        uint8_t m[PRJ_ITEMS];
#pragma unroll
        for (int i = 0; i < PRJ_ITEMS; i++)
            m[i] = (uint8_t)((top.nul >> i) & 1u);
        prj_store<uint8_t>(out_null, p0, n, whole, m);
    }

    /* rows past n hold zeros and may "raise": they do not count */
    unsigned long long key = ~0ull;
#pragma unroll
    for (int i = PRJ_ITEMS - 1; i >= 0; i--)
        if (((valid >> i) & 1u) && prj_err(err, i))
            key = ((unsigned long long)(p0 + i) << 8) | prj_err(err, i);
    if (__ballot(key != ~0ull) != 0ull) {   /* wave-uniform, rare */
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other < key ? other : key;
        }
        if (threadIdx.x % WAVE == 0)
            atomicMin(err_slot, key);
    }
}

/* ---- host side ---- */

struct prj_type {
    int t;           /* OTBX_EXT_* */
    bool nullable;
};

/* type-check `e` by abstract interpretation and lower it to `p`; false = the
 * program is not well-formed. *res = the type of its one result, *depth the
 * deepest the stack gets. */
static bool prj_compile(const otbx_expr *e, int64_t n, prj_prog *p,
                        prj_type *res, int *depth)
{
    prj_type st[OTBX_MAX_EXPR_DEPTH];
    int d = 0, maxd = 0;
    if (e->ninstr < 1 || e->ninstr > OTBX_MAX_EXPR_INSTRS)
        return false;
    p->ninstr = e->ninstr;
    for (int pc = 0; pc < e->ninstr; pc++) {
        const otbx_exprinstr *in = &e->instr[pc];
        prj_instr *o = &p->instr[pc];
        o->col = nullptr;
        o->nulls = nullptr;
        o->imm = 0;
        o->aux = 0;
        const int op = in->op;
        const int arity = op <= OTBX_EX_CONST ? 0
                          : (op == OTBX_EX_NEG || op == OTBX_EX_ABS ||
                             op == OTBX_EX_CAST || op == OTBX_EX_NOT ||
                             op == OTBX_EX_ISNULL || op == OTBX_EX_NOTNULL) ? 1
                          : op == OTBX_EX_CASE ? 3 : 2;
        if (op < OTBX_EX_COL || op > OTBX_EX_COALESCE)
            return false;
        if (d < arity || d - arity + 1 > OTBX_MAX_EXPR_DEPTH)
            return false;
        prj_type *a = &st[d - arity];   /* first operand = result slot */
        const prj_type *b = a + 1, *c = a + 2;
        o->dst = (int16_t)(d - arity);
        prj_type r;
        switch (op) {
        case OTBX_EX_COL:
            if (in->type < OTBX_SORT_I64 || in->type > OTBX_SORT_U8)
                return false;
            if (n > 0 && !in->col)
                return false;
            o->op = in->type == OTBX_SORT_I32 ? PJ_LD_I32
                    : in->type == OTBX_SORT_U8 ? PJ_LD_U8 : PJ_LD8;
            o->col = in->col;
            o->nulls = in->nulls;
            r.t = in->type == OTBX_SORT_F64 ? OTBX_EXT_FLOAT8 : OTBX_EXT_INT8;
            r.nullable = in->nulls != nullptr;
            break;
        case OTBX_EX_CONST:
            if (in->type < OTBX_EXT_INT8 || in->type > OTBX_EXT_BOOL)
                return false;
            o->op = PJ_CONST;
            o->aux = in->isnull ? 1 : 0;
            if (in->isnull)
                o->imm = 0;
            else if (in->type == OTBX_EXT_FLOAT8)
                __builtin_memcpy(&o->imm, &in->cf, 8);
            else if (in->type == OTBX_EXT_BOOL)
                o->imm = in->ci != 0;
            else
                o->imm = (unsigned long long)in->ci;
            r.t = in->type;
            r.nullable = in->isnull != 0;
            break;
        case OTBX_EX_ADD: case OTBX_EX_SUB: case OTBX_EX_MUL:
        case OTBX_EX_DIV: case OTBX_EX_MOD:
            if (a->t != b->t || a->t == OTBX_EXT_BOOL)
                return false;
            if (op == OTBX_EX_MOD && a->t != OTBX_EXT_INT8)
                return false;
            o->op = (a->t == OTBX_EXT_INT8 ? PJ_I_ADD : PJ_F_ADD) +
                    (op - OTBX_EX_ADD);
            r.t = a->t;
            r.nullable = a->nullable || b->nullable;
            break;
        case OTBX_EX_NEG: case OTBX_EX_ABS:
            if (a->t == OTBX_EXT_BOOL)
                return false;
            o->op = (a->t == OTBX_EXT_INT8 ? PJ_I_NEG : PJ_F_NEG) +
                    (op - OTBX_EX_NEG);
            r = *a;
            break;
        case OTBX_EX_CAST:
            if (in->type == OTBX_EXT_FLOAT8 && a->t == OTBX_EXT_INT8)
                o->op = PJ_I2F;
            else if (in->type == OTBX_EXT_INT8 && a->t == OTBX_EXT_FLOAT8)
                o->op = PJ_F2I;
            else
                return false;
            r.t = in->type;
            r.nullable = a->nullable;
            break;
        case OTBX_EX_EQ: case OTBX_EX_NE: case OTBX_EX_LT:
        case OTBX_EX_LE: case OTBX_EX_GT: case OTBX_EX_GE:
            if (a->t != b->t || a->t == OTBX_EXT_BOOL)
                return false;
            o->op = a->t == OTBX_EXT_INT8 ? PJ_I_CMP : PJ_F_CMP;
            o->aux = (int16_t)(OTBX_CMP_EQ + (op - OTBX_EX_EQ));
            r.t = OTBX_EXT_BOOL;
            r.nullable = a->nullable || b->nullable;
            break;
        case OTBX_EX_AND: case OTBX_EX_OR:
            if (a->t != OTBX_EXT_BOOL || b->t != OTBX_EXT_BOOL)
                return false;
            o->op = op == OTBX_EX_AND ? PJ_AND : PJ_OR;
            r.t = OTBX_EXT_BOOL;
            r.nullable = a->nullable || b->nullable;
            break;
        case OTBX_EX_NOT:
            if (a->t != OTBX_EXT_BOOL)
                return false;
            o->op = PJ_NOT;
            r = *a;
            break;
        case OTBX_EX_ISNULL: case OTBX_EX_NOTNULL:
            o->op = op == OTBX_EX_ISNULL ? PJ_ISNULL : PJ_NOTNULL;
            r.t = OTBX_EXT_BOOL;
            r.nullable = false;
            break;
        case OTBX_EX_CASE:
            if (a->t != OTBX_EXT_BOOL || b->t != c->t)
                return false;
            o->op = PJ_CASE;
            r.t = b->t;
            r.nullable = b->nullable || c->nullable;
            break;
        default:   /* OTBX_EX_COALESCE */
            if (a->t != b->t)
                return false;
            o->op = PJ_COALESCE;
            r.t = a->t;
            r.nullable = a->nullable && b->nullable;
            break;
        }
        *a = r;
        d = d - arity + 1;
        maxd = d > maxd ? d : maxd;
    }
    if (d != 1)
        return false;
    *res = st[0];
    *depth = maxd;
    return true;
}

static_assert(PJ_I_SUB - PJ_I_ADD == OTBX_EX_SUB - OTBX_EX_ADD &&
              PJ_I_MOD - PJ_I_ADD == OTBX_EX_MOD - OTBX_EX_ADD &&
              PJ_F_DIV - PJ_F_ADD == OTBX_EX_DIV - OTBX_EX_ADD &&
              PJ_I_ABS - PJ_I_NEG == OTBX_EX_ABS - OTBX_EX_NEG &&
              PJ_F_ABS - PJ_F_NEG == OTBX_EX_ABS - OTBX_EX_NEG,
              "prj_compile maps operators by offset");

extern "C" {

otbx_status otbx_project(const otbx_expr *e, const int64_t *sel_dev, int64_t n,
                         int64_t n_src, int32_t out_type, void *out_dev,
                         uint8_t *out_null_dev, int64_t *err_dev, void *stream)
{
    /* argument checks first: nothing below this block may run on bad input,
     * and nothing in it touches HIP */
    if (!e || !err_dev)
        return OTBX_ERR_INVALID;
    if (n < 0 || n > INT32_MAX || n_src < 0)
        return OTBX_ERR_INVALID;
    if (!sel_dev && n > n_src)
        return OTBX_ERR_INVALID;
    if (n > 0 && n_src == 0)
        return OTBX_ERR_INVALID;
    prj_prog prog;
    prj_type res;
    int depth;
    if (!prj_compile(e, n, &prog, &res, &depth))
        return OTBX_ERR_INVALID;
    switch (out_type) {
    case OTBX_SORT_I64:
    case OTBX_SORT_I32:
        if (res.t != OTBX_EXT_INT8)
            return OTBX_ERR_INVALID;
        prog.out_kind = out_type == OTBX_SORT_I64 ? PJ_OUT_8 : PJ_OUT_I32;
        break;
    case OTBX_SORT_F64:
        if (res.t != OTBX_EXT_FLOAT8)
            return OTBX_ERR_INVALID;
        prog.out_kind = PJ_OUT_8;
        break;
    case OTBX_SORT_U8:
        if (res.t != OTBX_EXT_BOOL)
            return OTBX_ERR_INVALID;
        prog.out_kind = PJ_OUT_U8;
        break;
    default:
        return OTBX_ERR_INVALID;
    }
    if (n > 0 && !out_dev)
        return OTBX_ERR_INVALID;
    if (res.nullable && !out_null_dev)
        return OTBX_ERR_INVALID;

    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(err_dev, 0xff, sizeof(int64_t), s));   /* -1 */
    if (n > 0) {
        const uint32_t ntiles = (uint32_t)((n + PRJ_TILE - 1) / PRJ_TILE);
        /* the instance without the upper four slots runs at a higher
         * occupancy; most expressions fit it */
        if (depth <= 4)
            hipLaunchKernelGGL(k_prj_eval<4>, dim3(ntiles), dim3(PRJ_THREADS),
                               0, s, prog, sel_dev, (uint32_t)n, n_src,
                               out_dev, out_null_dev,
                               (unsigned long long *)err_dev);
        else
            hipLaunchKernelGGL(k_prj_eval<OTBX_MAX_EXPR_DEPTH>, dim3(ntiles),
                               dim3(PRJ_THREADS), 0, s, prog, sel_dev,
                               (uint32_t)n, n_src, out_dev, out_null_dev,
                               (unsigned long long *)err_dev);
        HIP_CHECK(hipGetLastError());
    }
    return OTBX_OK;
}

} /* extern "C" */

"""Two independent restatements of the Project operator's semantics
(include/otbx.h, otbx_project), plus the seeded expression generator the host
and the GPU tests share. No GPU, no torch.

An expression is a tree of tuples:
    ("col", name) | ("const", vtype, value-or-None) | ("cast", vtype, x) |
    (op, x[, y[, z]])   with op one of + - * / % neg abs = <> < <= > >=
                        and or not isnull notnull case coalesce
vtype is "i64", "f64" or "bool"; a None value is the NULL constant. `cols`
maps a name to (values, mask-or-None): int64 / int32 / uint8 columns are i64
values, float64 ones f64; a mask byte != 0 is NULL.

    ref_eval   vectorised numpy over the whole tree, eager, with an array of
               error codes beside every value merged by the header's rules;
               int64 wraps and overflow is an explicit predicate.
    step_eval  compiles the tree to steps with jumps, the way the reference
               does (execExpr.c → execExprInterp.c), and runs them row by
               row on Python int / float: untaken arms are never executed
               and the first raising row ends the run.

Both return (values, nulls, err): err = -1 or (j << 8) | code for the first
raising output row j; values hold 0 under a NULL. With err != -1 only err is
specified.
"""
import math

import numpy as np

I64_MIN, I64_MAX = -2**63, 2**63 - 1
DIV0, INT8_RANGE, OVERFLOW, UNDERFLOW, INT4_RANGE = 1, 2, 3, 4, 5
ARITH = ("+", "-", "*", "/", "%")
CMP = ("=", "<>", "<", "<=", ">", ">=")
OUT_DTYPE = {"i64": np.int64, "f64": np.float64, "i32": np.int32,
             "u8": np.uint8}


def tree_type(t, cols):
    op = t[0]
    if op == "col":
        return "f64" if cols[t[1]][0].dtype == np.float64 else "i64"
    if op in ("const", "cast"):
        return t[1]
    if op in ARITH or op in ("neg", "abs", "coalesce"):
        return tree_type(t[1], cols)
    if op == "case":
        return tree_type(t[2], cols)
    return "bool"


def tree_ninstr(t):
    return 1 + sum(tree_ninstr(c) for c in _children(t))


def tree_depth(t):
    return max([1] + [i + tree_depth(c) for i, c in enumerate(_children(t))])


def _children(t):
    if t[0] in ("col", "const"):
        return ()
    if t[0] == "cast":
        return (t[2],)
    return t[1:]


def _rows(cols, sel, n):
    """The columns as the evaluation sees them: gathered through sel."""
    out = {}
    for k, (v, m) in cols.items():
        v = np.asarray(v)
        m = None if m is None else np.asarray(m) != 0
        if sel is not None:
            v = v[sel]
            m = None if m is None else m[sel]
        out[k] = (v, m)
    if n is None:
        n = len(sel) if sel is not None else len(next(iter(out.values()))[0])
    return out, n


def _default_out(vtype):
    return {"i64": "i64", "f64": "f64", "bool": "u8"}[vtype]


# --------------------------------------------------------------------------
# ref_eval: vectorised
# --------------------------------------------------------------------------

def _tdiv(a, b):
    """int64 division truncating toward zero; b is neither 0 nor -1."""
    q = a // b
    return np.where((a % b != 0) & ((a < 0) != (b < 0)), q + 1, q)


def _f8key_cmp(x, y):
    """(less, equal) under float8_cmp_internal: NaN = NaN, NaN above all."""
    xn, yn = np.isnan(x), np.isnan(y)
    lt = (~xn & yn) | (~xn & ~yn & (x < y))
    eq = (xn & yn) | (x == y)
    return lt, eq


def _strict(n, operands, own):
    """Error codes of a strict operator."""
    nul = np.zeros(n, bool)
    for _, m, _ in operands:
        nul |= m
    err = np.where(nul, 0, own).astype(np.uint8)
    for _, _, e in reversed(operands):
        err = np.where(e != 0, e, err)
    return nul, err.astype(np.uint8)


def _vec(t, rows, n, cols):
    """(values, null bool array, error uint8 array) of subtree t."""
    op = t[0]
    zero = np.zeros(n, np.uint8)
    if op == "col":
        v, m = rows[t[1]]
        v = v.astype(np.float64) if v.dtype == np.float64 else v.astype(np.int64)
        return v, (np.zeros(n, bool) if m is None else m.copy()), zero
    if op == "const":
        dt = np.float64 if t[1] == "f64" else np.int64
        if t[2] is None:
            return np.zeros(n, dt), np.ones(n, bool), zero
        return np.full(n, t[2], dt), np.zeros(n, bool), zero
    kids = [_vec(c, rows, n, cols) for c in _children(t)]
    ktype = tree_type(_children(t)[0], cols)
    with np.errstate(all="ignore"):
        if op in ARITH:
            (a, _, _), (b, _, _) = kids
            own = np.zeros(n, np.uint8)
            if ktype == "i64":
                if op == "+":
                    r = a + b
                    own[((a ^ r) & (b ^ r)) < 0] = INT8_RANGE
                elif op == "-":
                    r = a - b
                    own[((a ^ b) & (a ^ r)) < 0] = INT8_RANGE
                elif op == "*":
                    r = a * b
                    # wrapped iff dividing the product back does not give b
                    plain = (a != 0) & (a != -1)
                    ovf = plain & (_tdiv(r, np.where(plain, a, 2)) != b)
                    ovf |= (a == -1) & (b == I64_MIN)
                    own[ovf] = INT8_RANGE
                else:
                    special = (b == 0) | (b == -1)
                    sb = np.where(special, 2, b)
                    if op == "/":
                        r = np.where(special, -a, _tdiv(a, sb))
                        own[(b == -1) & (a == I64_MIN)] = INT8_RANGE
                    else:
                        r = np.where(special, 0, a - _tdiv(a, sb) * sb)
                    own[b == 0] = DIV0
            else:
                inf_ok = np.isinf(a) | np.isinf(b)
                if op == "+":
                    r, zero_ok = a + b, np.ones(n, bool)
                elif op == "-":
                    r, zero_ok = a - b, np.ones(n, bool)
                elif op == "*":
                    r, zero_ok = a * b, (a == 0) | (b == 0)
                else:
                    r, zero_ok = a / b, a == 0
                own[(r == 0) & ~zero_ok] = UNDERFLOW
                own[np.isinf(r) & ~inf_ok] = OVERFLOW
                if op == "/":
                    own[b == 0] = DIV0
            nul, err = _strict(n, kids, own)
            return r, nul, err
        if op in ("neg", "abs"):
            (a, _, _), = kids
            own = np.zeros(n, np.uint8)
            if ktype == "i64":
                own[a == I64_MIN] = INT8_RANGE
                r = -a if op == "neg" else np.where(a < 0, -a, a)
            else:
                r = -a if op == "neg" else np.abs(a)
            nul, err = _strict(n, kids, own)
            return r, nul, err
        if op == "cast":
            (a, _, _), = kids
            own = np.zeros(n, np.uint8)
            if t[1] == "f64":
                r = a.astype(np.float64)
            else:
                ri = np.rint(a)
                ok = (ri >= -2.0**63) & (ri < 2.0**63)
                own[~ok] = INT8_RANGE
                r = np.where(ok, ri, 0.0).astype(np.int64)
            nul, err = _strict(n, kids, own)
            return r, nul, err
        if op in CMP:
            (a, _, _), (b, _, _) = kids
            if ktype == "i64":
                lt, eq = a < b, a == b
            else:
                lt, eq = _f8key_cmp(a, b)
            r = {"=": eq, "<>": ~eq, "<": lt, "<=": lt | eq,
                 ">": ~(lt | eq), ">=": ~lt}[op].astype(np.int64)
            nul, err = _strict(n, kids, zero)
            return r, nul, err
        if op == "not":
            (a, _, _), = kids
            nul, err = _strict(n, kids, zero)
            return 1 - a, nul, err
        if op in ("isnull", "notnull"):
            (_, m, e), = kids
            r = (m if op == "isnull" else ~m).astype(np.int64)
            return r, np.zeros(n, bool), e
        if op in ("and", "or"):
            (a, am, ae), (b, bm, be) = kids
            dec = 0 if op == "and" else 1
            adec, bdec = ~am & (a == dec), ~bm & (b == dec)
            nul = ~adec & ~bdec & (am | bm)
            r = np.where(adec | bdec, dec, 1 - dec).astype(np.int64)
            err = np.where(ae != 0, ae, np.where(adec, 0, be)).astype(np.uint8)
            return r, nul, err
        if op == "case":
            (c, cm, ce), (a, am, ae), (b, bm, be) = kids
            take = ~cm & (c != 0)
            err = np.where(ce != 0, ce, np.where(take, ae, be)).astype(np.uint8)
            return np.where(take, a, b), np.where(take, am, bm), err
        if op == "coalesce":
            (a, am, ae), (b, bm, be) = kids
            err = np.where(ae != 0, ae, np.where(am, be, 0)).astype(np.uint8)
            return np.where(am, b, a), am & bm, err
    raise ValueError(f"unknown operator {op!r}")


def _finish(v, nul, err, out):
    v = np.where(nul, 0, v)
    if out == "i32":
        bad = ~nul & (err == 0) & ((v < -2**31) | (v > 2**31 - 1))
        err = np.where(bad, INT4_RANGE, err)
    with np.errstate(all="ignore"):
        vals = v.astype(OUT_DTYPE[out])
    raised = np.flatnonzero(err)
    code = -1 if len(raised) == 0 else (int(raised[0]) << 8) | int(err[raised[0]])
    return vals, nul.astype(np.uint8), code


def ref_eval(tree, cols, sel=None, out=None, n=None):
    rows, n = _rows(cols, sel, n)
    v, nul, err = _vec(tree, rows, n, cols)
    return _finish(v, nul, err, out or _default_out(tree_type(tree, cols)))


# --------------------------------------------------------------------------
# step_eval: the reference's control flow, row by row
# --------------------------------------------------------------------------

class _Raise(Exception):
    def __init__(self, code):
        self.code = code


def _compile(t, cols, steps):
    """Append the steps of subtree t; jump targets are step indices."""
    op = t[0]
    if op == "col":
        steps.append(["col", t[1]])
    elif op == "const":
        steps.append(["const", t[1], t[2]])
    elif op in ("and", "or"):
        _compile(t[1], cols, steps)
        first = ["bool_first", op, None]     # jump when the left decides
        steps.append(first)
        _compile(t[2], cols, steps)
        steps.append(["bool_last", op])
        first[2] = len(steps)
    elif op == "case":
        _compile(t[1], cols, steps)
        jelse = ["jump_if_not_true", None]
        steps.append(jelse)
        _compile(t[2], cols, steps)
        jdone = ["jump", None]
        steps.append(jdone)
        jelse[1] = len(steps)
        _compile(t[3], cols, steps)
        jdone[1] = len(steps)
    elif op == "coalesce":
        _compile(t[1], cols, steps)
        j = ["jump_if_not_null", None]
        steps.append(j)
        _compile(t[2], cols, steps)
        steps.append(["coalesce_second"])
        j[1] = len(steps)
    elif op in ("isnull", "notnull"):
        _compile(t[1], cols, steps)
        steps.append(["nulltest", op])
    else:
        kids = _children(t)
        for c in kids:
            _compile(c, cols, steps)
        name = op if op != "cast" else ("i8tod" if t[1] == "f64" else "dtoi8")
        steps.append(["func_strict", name, len(kids),
                      tree_type(kids[0], cols)])


def _f8cmp(x, y):
    """float8_cmp_internal."""
    if math.isnan(x):
        return 0 if math.isnan(y) else 1
    if math.isnan(y):
        return -1
    return (x > y) - (x < y)


def _checkfloat(r, inf_ok, zero_ok):
    if math.isinf(r) and not inf_ok:
        raise _Raise(OVERFLOW)
    if r == 0.0 and not zero_ok:
        raise _Raise(UNDERFLOW)
    return r


def _int8(r):
    if not I64_MIN <= r <= I64_MAX:
        raise _Raise(INT8_RANGE)
    return r


def _call(name, ktype, a):
    if name in CMP:
        c = _f8cmp(a[0], a[1]) if ktype == "f64" else (a[0] > a[1]) - (a[0] < a[1])
        return {"=": c == 0, "<>": c != 0, "<": c < 0, "<=": c <= 0,
                ">": c > 0, ">=": c >= 0}[name]
    if name == "not":
        return not a[0]
    if name == "i8tod":
        return float(a[0])
    if name == "dtoi8":
        x = a[0]
        if math.isnan(x) or math.isinf(x):
            raise _Raise(INT8_RANGE)
        r = round(x)                      # ties to even, exact int
        if not I64_MIN <= r <= I64_MAX:   # 2^63 itself is refused
            raise _Raise(INT8_RANGE)
        return r
    if ktype == "i64":
        x = a[0]
        if name == "neg":
            return _int8(-x)
        if name == "abs":
            return _int8(abs(x))
        y = a[1]
        if name == "+":
            return _int8(x + y)
        if name == "-":
            return _int8(x - y)
        if name == "*":
            return _int8(x * y)
        if y == 0:
            raise _Raise(DIV0)
        q = abs(x) // abs(y) * (1 if (x < 0) == (y < 0) else -1)
        if name == "/":
            return _int8(q)
        return 0 if y == -1 else x - q * y
    x = a[0]
    if name == "neg":
        return -x
    if name == "abs":
        return math.fabs(x)
    y = a[1]
    inf_ok = math.isinf(x) or math.isinf(y)
    if name == "+":
        return _checkfloat(x + y, inf_ok, True)
    if name == "-":
        return _checkfloat(x - y, inf_ok, True)
    if name == "*":
        return _checkfloat(x * y, inf_ok, x == 0 or y == 0)
    if y == 0.0:
        raise _Raise(DIV0)
    return _checkfloat(x / y, inf_ok, x == 0)


def _run_row(steps, rows, j):
    """One row through the steps: (value, isnull). Raises _Raise."""
    st = []          # (value, isnull)
    anynull = []     # one flag per open AND / OR
    pc = 0
    while pc < len(steps):
        s = steps[pc]
        pc += 1
        k = s[0]
        if k == "col":
            v, m = rows[s[1]]
            isn = bool(m[j]) if m is not None else False
            x = v[j]
            st.append((float(x) if v.dtype == np.float64 else int(x), isn))
        elif k == "const":
            st.append((s[2], s[2] is None))
        elif k == "func_strict":
            args = st[len(st) - s[2]:]
            del st[len(st) - s[2]:]
            if any(isn for _, isn in args):
                st.append((None, True))
            else:
                st.append((_call(s[1], s[3], [v for v, _ in args]), False))
        elif k == "nulltest":
            _, isn = st.pop()
            st.append((isn if s[1] == "isnull" else not isn, False))
        elif k == "bool_first":
            v, isn = st.pop()
            decides = (s[1] == "or")
            if not isn and bool(v) == decides:
                st.append((decides, False))
                pc = s[2]
            else:
                anynull.append(isn)
        elif k == "bool_last":
            v, isn = st.pop()
            decides = (s[1] == "or")
            an = anynull.pop()
            if not isn and bool(v) == decides:
                st.append((decides, False))
            elif isn or an:
                st.append((None, True))
            else:
                st.append((not decides, False))
        elif k == "jump_if_not_true":
            v, isn = st.pop()
            if isn or not v:
                pc = s[1]
        elif k == "jump":
            pc = s[1]
        elif k == "jump_if_not_null":
            if not st[-1][1]:
                pc = s[1]
            else:
                st.pop()
        elif k == "coalesce_second":
            pass
        else:
            raise ValueError(k)
    assert len(st) == 1
    return st[0]


def step_eval(tree, cols, sel=None, out=None, n=None):
    rows, n = _rows(cols, sel, n)
    out = out or _default_out(tree_type(tree, cols))
    steps = []
    _compile(tree, cols, steps)
    vals = np.zeros(n, OUT_DTYPE[out])
    nulls = np.zeros(n, np.uint8)
    for j in range(n):
        try:
            v, isn = _run_row(steps, rows, j)
            if isn:
                nulls[j] = 1
                continue
            if out == "i32" and not -2**31 <= v <= 2**31 - 1:
                raise _Raise(INT4_RANGE)
            vals[j] = v
        except _Raise as r:
            return vals, nulls, (j << 8) | r.code
    return vals, nulls, -1


def assert_same(got, want, what=""):
    """The parity rule: err equal; where it is -1, masks equal and values
    bit-equal (NaN against NaN by isnan) wherever the mask is 0."""
    gv, gn, ge = got
    wv, wn, we = want
    assert ge == we, f"{what}: err {ge} != {we}"
    if we != -1:
        return
    gv, wv = np.asarray(gv), np.asarray(wv)
    assert gv.dtype == wv.dtype, f"{what}: dtype {gv.dtype} != {wv.dtype}"
    assert np.array_equal(np.asarray(gn), np.asarray(wn)), f"{what}: masks differ"
    keep = np.asarray(wn) == 0
    g, w = gv[keep], wv[keep]
    if g.dtype == np.float64:
        gn_, wn_ = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn_, wn_), f"{what}: NaN positions differ"
        g, w = g[~wn_].view(np.int64), w[~wn_].view(np.int64)
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[:5]}"


# --------------------------------------------------------------------------
# the seeded generator of well-typed programs
# --------------------------------------------------------------------------

F64_POOL = [0.0, -0.0, 1.0, -1.0, 0.5, 1.5, 2.5, -0.5, 3.25, 1e10, -1e10,
            1e-10, 123456.789, float("inf"), float("-inf"), float("nan")]
FUZZ_SEEDS = list(range(40))
FUZZ_ROWS = 5000


def fuzz_columns(seed, n=FUZZ_ROWS):
    """One column of each of the four types, each with a 20 % mask, plus a
    small-divisor column with zeros."""
    rng = np.random.default_rng(1000 + seed)
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    edge = rng.random(n) < 0.002
    a[edge] = rng.choice([I64_MIN, I64_MAX, 2**40, -2**40], edge.sum())
    b = rng.integers(-3, 4, n).astype(np.int64)
    x = rng.normal(0, 100, n)
    pool = rng.random(n) < 0.05
    x[pool] = rng.choice(F64_POOL, pool.sum())
    d = rng.integers(-2**20, 2**20, n).astype(np.int32)
    f = rng.integers(0, 6, n).astype(np.uint8)

    def mask():
        return (rng.random(n) < 0.2).astype(np.uint8)
    return {"a": (a, mask()), "b": (b, None), "x": (x, mask()),
            "d": (d, mask()), "f": (f, mask()), "y": (rng.normal(0, 3, n), None)}


def gen_tree(rng, want, budget):
    """A random well-typed tree of type `want` with at most ~budget levels.
    Divisions are guarded most of the time, so that most programs raise on
    no row but some do."""
    icols, fcols = ["a", "b", "d", "f"], ["x", "y"]
    if budget <= 0 or rng.random() < 0.15:
        if want == "i64":
            return ("col", str(rng.choice(icols))) if rng.random() < 0.75 \
                else ("const", "i64", int(rng.integers(-5, 6)))
        if want == "f64":
            return ("col", str(rng.choice(fcols))) if rng.random() < 0.75 \
                else ("const", "f64", float(rng.choice([0.5, 2.0, -1.25, 100.0])))
        return ("const", "bool", bool(rng.integers(0, 2))) if rng.random() < 0.3 \
            else (str(rng.choice(CMP)), gen_tree(rng, "i64", 0),
                  gen_tree(rng, "i64", 0))
    sub = lambda ty: gen_tree(rng, ty, budget - 1)   # noqa: E731
    r = rng.random()
    if want == "bool":
        if r < 0.35:
            ty = "i64" if rng.random() < 0.5 else "f64"
            return (str(rng.choice(CMP)), sub(ty), sub(ty))
        if r < 0.6:
            return (str(rng.choice(["and", "or"])), sub("bool"), sub("bool"))
        if r < 0.7:
            return ("not", sub("bool"))
        if r < 0.85:
            return (str(rng.choice(["isnull", "notnull"])),
                    sub(str(rng.choice(["i64", "f64", "bool"]))))
        if r < 0.93:
            return ("case", sub("bool"), sub("bool"), sub("bool"))
        return ("coalesce", sub("bool"), sub("bool"))
    if r < 0.4:
        return (str(rng.choice(["+", "-", "*"])), sub(want), sub(want))
    if r < 0.55:
        # a division or modulo: guarded three times out of four
        op = "/" if want == "f64" or rng.random() < 0.5 else "%"
        num, den = sub(want), gen_tree(rng, want, 0)
        zero = ("const", want, 0 if want == "i64" else 0.0)
        if rng.random() < 0.75:
            return ("case", ("<>", den, zero), (op, num, den), zero)
        return (op, num, den)
    if r < 0.65:
        return (str(rng.choice(["neg", "abs"])), sub(want))
    if r < 0.75:
        if want == "f64":
            return ("cast", "f64", sub("i64"))
        # keep the float side small enough for dtoi8 most of the time
        return ("cast", "i64", ("col", "y") if rng.random() < 0.7 else sub("f64"))
    if r < 0.88:
        return ("case", sub("bool"), sub(want), sub(want))
    if r < 0.95:
        return ("coalesce", sub(want), sub(want))
    return ("coalesce", sub(want), ("const", want, None))


def fuzz_program(seed):
    """(tree, out) for a seed: a tree within the instruction and depth
    limits; i64 results sometimes go to an I32 output."""
    rng = np.random.default_rng(seed)
    while True:
        want = str(rng.choice(["i64", "f64", "bool"]))
        tree = gen_tree(rng, want, int(rng.integers(2, 5)))
        if 3 <= tree_ninstr(tree) <= 32 and tree_depth(tree) <= 8:
            out = _default_out(want)
            if want == "i64" and rng.random() < 0.25:
                out = "i32"
            return tree, out


def fuzz_selection(seed, n=FUZZ_ROWS):
    rng = np.random.default_rng(5000 + seed)
    return np.sort(rng.choice(n, int(rng.integers(1, n)), replace=False)) \
        .astype(np.int64)

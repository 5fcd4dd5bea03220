"""GPU parity of the generic Project operator (otbx_project / GpuProject)
against ref_eval of tests/project_ref.py. The parity rule has no tolerance:
the error slot is equal; where it is -1 the masks are equal and the values
bit-equal (NaN against NaN by isnan) wherever the mask is 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import project_ref as pr
from project_ref import (ARITH, CMP, DIV0, I64_MAX, I64_MIN, INT4_RANGE,
                         INT8_RANGE, OVERFLOW, UNDERFLOW, assert_same,
                         ref_eval)
from test_gpu_filter import dev
from test_gpu_sort import F64_EDGE
from test_project_host import (A, B, DIV, I64_EDGE, LAZY_CASES, ab, code_at,
                               f64c, i64c, lazy_cols)

pytestmark = pytest.mark.gpu

OUT_TORCH = {"i64": torch.int64, "f64": torch.float64, "i32": torch.int32,
             "u8": torch.uint8}


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def T(ex):
    return ex.PROJECT_TILE    # PRJ_TILE of otbx_project.hip: rows per workgroup


def dev_cols(cols, col_skip=0, mask_skip=0):
    return {k: (dev(v, col_skip), dev(m, mask_skip)) for k, (v, m) in cols.items()}


def to_expr(ex, t, dcols):
    """The builder's Expr of a project_ref tree over device columns."""
    op = t[0]
    if op == "col":
        return ex.col(*dcols[t[1]])
    if op == "const":
        return ex.null(t[1]) if t[2] is None else ex.const(t[2])
    k = [to_expr(ex, c, dcols) for c in pr._children(t)]
    if op == "cast":
        return k[0].cast(t[1])
    if op in ARITH:
        return {"+": k[0].__add__, "-": k[0].__sub__, "*": k[0].__mul__,
                "/": k[0].__truediv__, "%": k[0].__mod__}[op](k[1])
    if op in CMP:
        return {"=": k[0].eq, "<>": k[0].ne, "<": k[0].lt, "<=": k[0].le,
                ">": k[0].gt, ">=": k[0].ge}[op](k[1])
    if op == "neg":
        return -k[0]
    if op == "abs":
        return abs(k[0])
    if op == "and":
        return k[0] & k[1]
    if op == "or":
        return k[0] | k[1]
    if op == "not":
        return ~k[0]
    if op in ("isnull", "notnull"):
        return getattr(k[0], op)()
    if op == "case":
        return ex.case(*k)
    assert op == "coalesce"
    return ex.coalesce(*k)


def gpu_eval(ex, tree, dcols, sel=None, out=None, n=None, out_skip=0):
    """(values, nulls, err) of one GpuProject run, through the lifecycle."""
    e = to_expr(ex, tree, dcols)
    dsel = None if sel is None else dev(np.asarray(sel, dtype=np.int64))
    if n is None:
        n = len(sel) if sel is not None else e.n_src
    otype = out or pr._default_out(e.vtype)
    base = torch.zeros(n + out_skip, dtype=OUT_TORCH[otype], device="cuda")
    node = ex.GpuProject(e, sel=dsel, n=n, out=base[out_skip:])
    node.BeginCustomScan()
    try:
        row = node.ExecCustomScan()
    except ex.OtbxError as err:
        assert err.status == 4
        assert node.err != -1
        assert ex.PROJECT_ERRORS[node.err & 0xff] in str(err)
        assert f"at output row {node.err >> 8}" in str(err)
        node.EndCustomScan()
        return None, None, node.err
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    vals, nulls = row
    assert node.err == -1 and len(vals) == n
    assert (nulls is None) == (not e.nullable)
    nl = np.zeros(n, np.uint8) if nulls is None else nulls.cpu().numpy()
    return vals.cpu().numpy(), nl, -1


def check(ex, tree, cols, sel=None, out=None, n=None, col_skip=0, mask_skip=0,
          out_skip=0):
    want = ref_eval(tree, cols, sel, out, n)
    got = gpu_eval(ex, tree, dev_cols(cols, col_skip, mask_skip), sel, out, n,
                   out_skip)
    assert_same(got, want, repr(tree))
    return want


# ---- sizes and alignment ----

MIXED = ("case", (">", ("col", "f"), ("const", "i64", 2)),
         ("*", ("cast", "f64", ("+", ("col", "a"), ("col", "d"))), ("col", "x")),
         ("col", "x"))


def mixed_cols(n, seed):
    rng = np.random.default_rng(seed)

    def mask():
        return (rng.random(n) < 0.2).astype(np.uint8)
    return {"a": (rng.integers(-10**6, 10**6, n).astype(np.int64), mask()),
            "x": (rng.normal(0, 1e3, n), mask()),
            "d": (rng.integers(-2**31, 2**31, n).astype(np.int32), mask()),
            "f": (rng.integers(0, 6, n).astype(np.uint8), mask())}


def sizes(T):
    return [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17,
            100_003]


@pytest.mark.parametrize("k", range(13))
def test_sizes_nullable_mixed_expression(ex, T, k):
    n = sizes(T)[k]
    w = check(ex, MIXED, mixed_cols(n, n + 1))
    assert w[2] == -1
    if n > 300:
        assert 0 < w[1].sum() < n


@pytest.mark.parametrize("col_skip,mask_skip,out_skip",
                         [(1, 0, 0), (0, 1, 0), (3, 3, 0), (0, 0, 1),
                          (1, 3, 1), (3, 1, 3)])
def test_unaligned_views(ex, T, col_skip, mask_skip, out_skip):
    n = 3 * T + 17
    cols = mixed_cols(n, 77)
    kw = dict(col_skip=col_skip, mask_skip=mask_skip, out_skip=out_skip)
    check(ex, MIXED, cols, **kw)                                   # f64 out
    check(ex, (">", ("col", "f"), ("col", "d")), cols, **kw)       # u8 out
    check(ex, ("+", ("col", "d"), ("col", "f")), cols, out="i32", **kw)
    check(ex, ("+", ("col", "a"), ("col", "f")), cols, **kw)       # i64 out


# ---- every operator x type on the edge values, no row raising ----

def non_raising(tree, cols):
    """The columns restricted to the rows on which `tree` does not raise."""
    n = len(next(iter(cols.values()))[0])
    keep = np.arange(n, dtype=np.int64)
    while True:
        e = ref_eval(tree, cols, keep)[2]
        if e == -1:
            return {k: (v[keep], None if m is None else m[keep])
                    for k, (v, m) in cols.items()}
        keep = np.delete(keep, e >> 8)


def edge_pairs(vals, seed):
    a, b = np.repeat(vals, len(vals)), np.tile(vals, len(vals))
    rng = np.random.default_rng(seed)
    return a, b, (rng.random(len(a)) < 0.2).astype(np.uint8), \
        (rng.random(len(a)) < 0.2).astype(np.uint8)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("op,ty", [
    (op, ty) for op in ARITH + CMP + ("neg", "abs", "coalesce", "case")
    for ty in ("i64", "f64") if (op, ty) != ("%", "f64")])
def test_operators_on_edge_values(ex, op, ty, masked):
    a, b, am, bm = edge_pairs(I64_EDGE if ty == "i64" else F64_EDGE, 5)
    cols = {"a": (a, am if masked else None), "b": (b, bm if masked else None)}
    if op in ("neg", "abs"):
        tree = (op, A)
    elif op == "case":
        tree = ("case", ("<", A, B), A, B)
    else:
        tree = (op, A, B)
    cols = non_raising(tree, cols)
    assert len(cols["a"][0]) > len(a) // 4
    assert check(ex, tree, cols)[2] == -1


@pytest.mark.parametrize("masked", [False, True])
def test_casts_on_edge_values(ex, masked):
    rng = np.random.default_rng(6)
    x = np.concatenate([F64_EDGE, f64c(0.5, 1.5, 2.5, -0.5, -1.5, 1e15 + 0.5,
                                       -2.0**63, 2.0**63 - 1024, 2.0**53 + 2)])
    cols = {"a": (x, (rng.random(len(x)) < 0.2).astype(np.uint8) if masked else None)}
    tree = ("cast", "i64", A)
    assert check(ex, tree, non_raising(tree, cols))[2] == -1
    big = np.concatenate([I64_EDGE, i64c(2**53 + 1, -2**53 - 1, 2**62 + 1)])
    cols = {"a": (big, (rng.random(len(big)) < 0.2).astype(np.uint8) if masked else None)}
    assert check(ex, ("cast", "f64", A), cols)[2] == -1
    d = np.array([-2**31, -1, 0, 1, 2**31 - 1], dtype=np.int32)
    f = np.array([0, 1, 127, 128, 255], dtype=np.uint8)
    cols = {"d": (d, None), "f": (f, np.array([0, 1, 0, 0, 1], np.uint8) if masked else None)}
    check(ex, ("*", ("col", "d"), ("col", "f")), cols)
    check(ex, ("cast", "f64", ("col", "f")), cols)


@pytest.mark.parametrize("masked", [False, True])
def test_boolean_operators(ex, masked):
    p = np.array([1, 1, 1, 0, 0, 0, 1, 0, 1] * 3, dtype=np.int64)
    q = np.array([1, 0, 1, 1, 0, 0, 0, 1, 1] * 3, dtype=np.int64)
    rng = np.random.default_rng(8)
    pm = (rng.random(27) < 0.35).astype(np.uint8) if masked else None
    qm = (rng.random(27) < 0.35).astype(np.uint8) if masked else None
    cols = {"p": (p, pm), "q": (q, qm)}
    P = ("=", ("col", "p"), ("const", "i64", 1))
    Q = ("=", ("col", "q"), ("const", "i64", 1))
    for tree in (("and", P, Q), ("or", P, Q), ("not", P), ("isnull", P),
                 ("notnull", ("col", "q")), ("case", P, Q, ("not", Q)),
                 ("coalesce", P, Q), ("coalesce", P, ("const", "bool", None)),
                 ("and", P, ("const", "bool", None)),
                 ("or", ("const", "bool", None), Q),
                 ("case", ("const", "bool", None), P, Q)):
        check(ex, tree, cols)


# ---- the error slot ----

ERR_CASES = [
    (DIV0, ("/", A, B), "i64", 7, 0, None),
    (INT8_RANGE, ("+", A, B), "i64", I64_MAX, 1, None),
    (OVERFLOW, ("*", A, B), "f64", 1e200, 1e200, None),
    (UNDERFLOW, ("*", A, B), "f64", 1e-200, 1e-200, None),
    (INT4_RANGE, ("+", A, B), "i64", 2**31 - 1, 1, "i32"),
]


def err_cols(ty, n, rows):
    """Harmless columns of n rows with (a, b) planted at the given rows."""
    mk = i64c if ty == "i64" else f64c
    a, b = mk(*[6] * n), mk(*[3] * n)
    for j, (va, vb) in rows.items():
        a[j], b[j] = va, vb
    return ab(a, b)


@pytest.mark.parametrize("code,tree,ty,va,vb,out", ERR_CASES,
                         ids=[str(c[0]) for c in ERR_CASES])
def test_one_case_per_error_code(ex, T, code, tree, ty, va, vb, out):
    n = 2 * T + 100
    j = T + 5
    assert check(ex, tree, err_cols(ty, n, {j: (va, vb)}), out=out)[2] == \
        code_at(j, code)
    assert check(ex, tree, err_cols(ty, n, {}), out=out)[2] == -1


@pytest.mark.parametrize("swap", [False, True])
def test_smallest_raising_row_wins(ex, T, swap):
    """Two raising rows in different workgroups, different codes, in each
    order of the codes."""
    n = 40 * T + 3
    first, second = (I64_MIN, -1), (5, 0)       # code 2, code 1
    if swap:
        first, second = second, first
    j1, j2 = 2 * T + 1, 37 * T + 9
    w = check(ex, DIV, err_cols("i64", n, {j1: first, j2: second}))
    assert w[2] == code_at(j1, DIV0 if swap else INT8_RANGE)
    # and many raising rows: still the first
    cols = err_cols("i64", n, {j: (1, 0) for j in range(j1, n, 97)})
    assert check(ex, DIV, cols)[2] == code_at(j1, DIV0)


def test_raising_row_excluded_by_sel_and_in_the_last_partial_tile(ex, T):
    n = 3 * T + 17
    j = n - 2                                    # the last, partial tile
    cols = err_cols("i64", n, {j: (1, 0)})
    assert check(ex, DIV, cols)[2] == code_at(j, DIV0)
    sel = np.delete(np.arange(n, dtype=np.int64), j)
    assert check(ex, DIV, cols, sel=sel)[2] == -1
    # selected again, it raises at its OUTPUT position
    sel = np.array([5, j, 7], dtype=np.int64)
    assert check(ex, DIV, cols, sel=sel)[2] == code_at(1, DIV0)


# ---- laziness ----

@pytest.mark.parametrize("name,tree,code", LAZY_CASES, ids=[c[0] for c in LAZY_CASES])
def test_laziness(ex, T, name, tree, code):
    cols = lazy_cols(3 * T + 17)
    first_zero = int(np.flatnonzero(cols["b"][0] == 0)[0])
    w = check(ex, tree, cols)
    assert w[2] == (code_at(first_zero, code) if code else -1)


def test_garbage_under_a_null_never_raises(ex, T):
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    m = (rng.random(n) < 0.5).astype(np.uint8)
    a = np.where(m, I64_MIN, rng.integers(-99, 99, n)).astype(np.int64)
    b = np.where(m, rng.choice([0, -1], n), rng.integers(1, 9, n)).astype(np.int64)
    cols = {"a": (a, m), "b": (b, m)}
    for tree in (DIV, ("%", A, B), ("neg", A), ("abs", A), ("*", A, B)):
        assert check(ex, tree, cols)[2] == -1
    # the mask on one side only
    cols = {"a": (rng.integers(-99, 99, n).astype(np.int64), None), "b": (b, m)}
    assert check(ex, DIV, cols)[2] == -1
    x = np.where(m, 0.0, rng.normal(0, 1, n) + 5)
    cols = {"a": (rng.normal(0, 1, n), None), "b": (x, m)}
    assert check(ex, DIV, cols)[2] == -1


def test_division_around_the_int32_range(ex, T):
    """int8div / int8mod on operands at and just outside the int32 corners,
    among ordinary ones."""
    n = 3 * T + 17
    rng = np.random.default_rng(21)
    a = rng.integers(-2**31, 2**31, n).astype(np.int64)
    b = rng.integers(-2**31, 2**31, n).astype(np.int64)
    b[b == 0] = 7
    a[:8] = [-2**31, -2**31, 2**31 - 1, -2**31, 2**31 - 1, 0, -1, 1]
    b[:8] = [-1, 1, -1, 2**31 - 1, -2**31, -2**31, -2**31, 2]
    wide = rng.choice(np.arange(T, n), 6, replace=False)
    a[wide[:3]] = [2**31, -2**31 - 1, 2**40 + 3]
    b[wide[3:]] = [2**31, -2**31 - 1, -2**40]
    for op in ("/", "%"):
        assert check(ex, (op, A, B), ab(a, b))[2] == -1


# ---- selections ----

def test_empty_and_one_row_selection(ex):
    cols = mixed_cols(500, 12)
    w = check(ex, MIXED, cols, sel=np.zeros(0, dtype=np.int64))
    assert len(w[0]) == 0 and w[2] == -1
    w = check(ex, MIXED, cols, sel=np.array([499], dtype=np.int64))
    assert len(w[0]) == 1


def test_unordered_and_repeating_selection(ex, T):
    n = 3 * T + 17
    cols = mixed_cols(n, 13)
    rng = np.random.default_rng(14)
    check(ex, MIXED, cols, sel=rng.integers(0, n, 2 * T + 5).astype(np.int64))
    check(ex, MIXED, cols, sel=rng.integers(0, n, 100).astype(np.int64),
          col_skip=1, mask_skip=3)


def test_selection_from_gpufilter_guards_a_division(ex, T):
    n = 3 * T + 17
    rng = np.random.default_rng(15)
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    b = rng.integers(-3, 4, n).astype(np.int64)
    da, db = dev(a), dev(b)
    flt = ex.GpuFilter([[ex.qual_term(db, "<>", 0)]])
    flt.BeginCustomScan()
    sel = flt.ExecCustomScan()
    flt.EndCustomScan()
    assert 0 < len(sel) < n
    node = ex.GpuProject(ex.col(da) / ex.col(db), sel=sel)
    node.BeginCustomScan()
    vals, nulls = node.ExecCustomScan()
    node.EndCustomScan()
    assert nulls is None
    keep = b != 0
    want = (np.abs(a[keep]) // np.abs(b[keep])) * np.sign(a[keep]) * np.sign(b[keep])
    assert np.array_equal(vals.cpu().numpy(), want)
    # without the selection the same expression raises
    node = ex.GpuProject(ex.col(da) / ex.col(db))
    node.BeginCustomScan()
    with pytest.raises(ex.OtbxError) as ei:
        node.ExecCustomScan()
    assert ei.value.status == 4 and "division by zero" in str(ei.value)
    assert node.err == code_at(int(np.flatnonzero(b == 0)[0]), DIV0)


def test_out_of_range_selection_entries_are_clamped(ex):
    cols = ab(i64c(10, 20, 30), i64c(1, 2, 3))
    dc = dev_cols(cols)
    got = gpu_eval(ex, ("+", A, B), dc, sel=np.array([-5, 1, 99], np.int64))
    assert list(got[0]) == [11, 22, 33] and got[2] == -1


# ---- output types ----

def test_i32_output(ex, T):
    n = 2 * T + 9
    rng = np.random.default_rng(16)
    d = rng.integers(0, 2**31 - 1, n).astype(np.int32)
    m = (rng.random(n) < 0.2).astype(np.uint8)
    cols = {"d": (d, m)}
    w = check(ex, ("/", ("col", "d"), ("const", "i64", 365)), cols, out="i32")
    assert w[0].dtype == np.int32 and w[2] == -1
    # out of range: code 5 — but not under a NULL
    a = np.full(n, 7, dtype=np.int64)
    a[T + 3] = 2**31
    a[5] = -2**31 - 1
    am = np.zeros(n, np.uint8)
    am[5] = 1
    assert check(ex, A, {"a": (a, am)}, out="i32")[2] == code_at(T + 3, INT4_RANGE)
    a[T + 3] = -2**31
    assert check(ex, A, {"a": (a, am)}, out="i32")[2] == -1


def test_bool_goes_to_u8(ex, T):
    n = T + 77
    cols = mixed_cols(n, 17)
    w = check(ex, ("and", (">", ("col", "x"), ("const", "f64", 0.0)),
                   ("<", ("col", "a"), ("col", "d"))), cols)
    assert w[0].dtype == np.uint8 and set(np.unique(w[0])) <= {0, 1}


def test_no_mask_output_for_a_non_nullable_program(ex, T):
    """out_null_dev == NULL: nothing but out[0:n) is written."""
    n, G = T + 100, 64
    SENT = 0x5a5a5a5a5a5a5a5a
    rng = np.random.default_rng(18)
    a = rng.integers(-99, 99, n).astype(np.int64)
    base = torch.full((n + 2 * G,), SENT, dtype=torch.int64, device="cuda")
    e = ex.col(dev(a)) * 3 + 1
    assert not e.nullable
    node = ex.GpuProject(e, out=base[G:G + n])
    node.BeginCustomScan()
    vals, nulls = node.ExecCustomScan()
    node.EndCustomScan()
    assert nulls is None and vals.data_ptr() == base[G:].data_ptr()
    got = base.cpu().numpy()
    assert (got[:G] == SENT).all() and (got[G + n:] == SENT).all()
    assert np.array_equal(got[G:G + n], a * 3 + 1)
    # a nullable program without a mask is refused by the C checks
    from opentenbase_amd import _lib
    m = dev(np.zeros(n, np.uint8))
    d = (ex.col(dev(a), m) + 1).to_dev()
    err = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = _lib.lib().otbx_project(
        C.byref(d), None, C.c_int64(n), C.c_int64(n), C.c_int32(0),
        C.c_void_p(base.data_ptr()), None, C.c_void_p(err.data_ptr()), None)
    assert st == 3


# ---- program limits ----

def test_32_instructions_at_depth_8(ex, T):
    """a0 + (a1 + ... (a6 + a7)) is depth 8 with 15 instructions; negations
    and more left-deep terms bring it to 32."""
    n = T + 5
    rng = np.random.default_rng(19)
    cols = {f"c{i}": (rng.integers(-1000, 1000, n).astype(np.int64),
                      (rng.random(n) < 0.05).astype(np.uint8) if i % 3 == 0 else None)
            for i in range(8)}
    tree = ("col", "c7")
    for i in range(6, -1, -1):
        tree = ("+", ("col", f"c{i}"), tree)            # 15 instrs, depth 8
    for i in range(8):
        tree = ("-", tree, ("col", f"c{i}"))            # + 16
    tree = ("neg", tree)                                # 32
    assert pr.tree_ninstr(tree) == 32 and pr.tree_depth(tree) == 8
    assert check(ex, tree, cols)[2] == -1


# ---- fuzz ----

@pytest.mark.parametrize("seed", pr.FUZZ_SEEDS)
def test_fuzz(ex, seed):
    tree, out = pr.fuzz_program(seed)
    cols = pr.fuzz_columns(seed)
    dc = dev_cols(cols)
    # n by hand: a program of constants alone has no column to take it from
    assert_same(gpu_eval(ex, tree, dc, out=out, n=pr.FUZZ_ROWS),
                ref_eval(tree, cols, out=out), repr(tree))
    sel = pr.fuzz_selection(seed)
    assert_same(gpu_eval(ex, tree, dc, sel=sel, out=out),
                ref_eval(tree, cols, sel, out), repr(tree))


# ---- pipeline and lifecycle ----

def test_filter_project_hashagg_pipeline(ex):
    n = 20_000
    rng = np.random.default_rng(20)
    date = rng.integers(0, 2500, n).astype(np.int32)
    price = rng.uniform(900, 105000, n).round(2)
    disc = rng.integers(0, 11, n) / 100.0
    flag = rng.integers(0, 3, n).astype(np.int64)
    dm = (rng.random(n) < 0.1).astype(np.uint8)          # NULL discounts
    ddate, dprice, ddisc, dflag, ddm = map(dev, (date, price, disc, flag, dm))

    flt = ex.GpuFilter([[ex.qual_term(ddate, "<=", 2000)]])
    flt.BeginCustomScan()
    sel = flt.ExecCustomScan()
    flt.EndCustomScan()
    prj = ex.GpuProject(ex.col(dprice) * (1 - ex.col(ddisc, ddm)), sel=sel)
    prj.BeginCustomScan()
    vals, nulls = prj.ExecCustomScan()
    prj.EndCustomScan()
    agg = ex.GpuHashAgg(ex.gather(dflag, sel), vals, val_null=nulls)
    agg.BeginCustomScan()
    groups = []
    while (g := agg.ExecCustomScan()) is not None:
        groups.append(g)
    agg.EndCustomScan()

    keep = date <= 2000
    want = price[keep] * (1 - disc[keep])
    wnull = dm[keep]
    assert np.array_equal(nulls.cpu().numpy(), wnull)
    got = vals.cpu().numpy()
    assert np.array_equal(got[wnull == 0].view(np.int64),
                          want[wnull == 0].view(np.int64))
    assert (got[wnull == 1] == 0).all()
    assert [int(g["key"]) for g in groups] == [0, 1, 2]
    for g in groups:
        rows = flag[keep] == g["key"]
        assert g["count_star"] == rows.sum()
        assert g["count_v"] == (rows & (wnull == 0)).sum()
        s = want[rows & (wnull == 0)].sum()
        assert abs(g["sum_v"] - s) <= 1e-6 * abs(s)
    # the projected column also feeds a sort and a qual unchanged
    srt = ex.GpuSort([vals], nulls=[nulls])
    srt.BeginCustomScan()
    assert srt.ExecCustomScan() is not None
    srt.EndCustomScan()
    flt2 = ex.GpuFilter([[ex.qual_term(vals, ">", 50000.0, nulls=nulls)]])
    flt2.BeginCustomScan()
    sel2 = flt2.ExecCustomScan()
    flt2.EndCustomScan()
    assert len(sel2) == ((want > 50000.0) & (wnull == 0)).sum()


def test_lifecycle(ex):
    a = dev(np.arange(10, dtype=np.int64))
    node = ex.GpuProject(ex.col(a) * 2)
    with pytest.raises(ex.OtbxError):
        node.ExecCustomScan()
    assert node.explain() is None
    node.BeginCustomScan()
    vals, nulls = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    assert nulls is None and vals.cpu().tolist() == list(range(0, 20, 2))
    assert node.explain()["project"] >= 0.0
    a += 1
    node.ReScanCustomScan()
    vals, _ = node.ExecCustomScan()
    assert vals.cpu().tolist() == list(range(2, 22, 2))
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    with pytest.raises(ex.OtbxError):
        node.ExecCustomScan()

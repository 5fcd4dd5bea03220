"""GPU parity of the generic Filter operator (otbx_filter_sel / GpuFilter):
the selection vector must be equal to ref_sel of tests/filter_ref.py — no
tolerance anywhere (the selection is the ascending list of passing rows, so
it is unique)."""
import ctypes as C

import numpy as np
import pytest
import torch

from filter_ref import OPS, ref_sel, term, truth_cases
from test_gpu_sort import F64_EDGE

pytestmark = pytest.mark.gpu

TILE = 4096          # FLT_TILE of otbx_filter.hip: rows per workgroup
SCAN_CHUNK = 4096    # FLT_SCAN_CHUNK: tile counts per pass of k_flt_scan
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
DTYPES = {"i64": np.int64, "f64": np.float64, "i32": np.int32, "u8": np.uint8}


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


def dev(a, skip=0):
    """a on the device; skip > 0: as the view base[skip:] of a longer tensor,
    so that its address is `skip` elements past an aligned allocation"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not skip:
        return torch.from_numpy(a).cuda()
    base = torch.zeros(len(a) + skip, dtype=torch.from_numpy(a).dtype,
                       device="cuda")
    base[skip:] = torch.from_numpy(a).cuda()
    return base[skip:]


def to_node(ex, clauses, n=None, count_only=False, col_skip=0, mask_skip=0):
    q = [[ex.qual_term(dev(c, col_skip), op,
                       dev(r, col_skip) if isinstance(r, np.ndarray) else r,
                       dev(m, mask_skip), dev(rm, mask_skip))
          for c, op, r, m, rm in clause] for clause in clauses]
    return ex.GpuFilter(q, count_only=count_only, n=n)


def gpu_sel(ex, clauses, n=None, **kw):
    node = to_node(ex, clauses, n, **kw)
    node.BeginCustomScan()
    sel = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    assert sel.dtype == torch.int64 and node.count == len(sel)
    return sel.cpu().numpy()


def check(ex, clauses, n=None, **kw):
    got = gpu_sel(ex, clauses, n, **kw)
    exp = ref_sel(clauses, n)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp)
    return exp


def column(rng, type_, n):
    if type_ == "i64":
        return rng.integers(-2**62, 2**62, n, dtype=np.int64)
    if type_ == "f64":
        return rng.normal(0, 1e6, n)
    if type_ == "i32":
        return rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    return rng.integers(0, 256, n).astype(np.uint8)


def median_const(type_):
    return {"i64": 0, "f64": 0.0, "i32": 0, "u8": 128}[type_]


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1,
         3 * TILE + 17, 4 * TILE, 4 * TILE + 1, 100_003]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_nullable_i64(ex, n):
    rng = np.random.default_rng(n + 1)
    k = rng.integers(-1000, 1000, n).astype(np.int64)
    nl = (rng.random(n) < 0.1).astype(np.uint8)
    exp = check(ex, [[term(k, "<", 0, nl)]])          # ~45 % pass
    assert n < 1000 or 0.35 * n < len(exp) < 0.55 * n


def test_tile_count_scan_takes_more_than_one_chunk(ex):
    n = (SCAN_CHUNK + 3) * TILE + 1234                 # 4100 tiles, 16.8 MB
    rng = np.random.default_rng(3)
    u = rng.integers(0, 256, n, dtype=np.uint8)
    exp = check(ex, [[term(u, "<", 13)]])              # ~5 %: a small result
    assert len(exp) > SCAN_CHUNK


@pytest.mark.parametrize("what", ["none", "all", "one_in_1e4"])
def test_selectivity(ex, what):
    rng = np.random.default_rng(5)
    n = 25 * TILE + 77
    k = rng.integers(0, 10_000, n).astype(np.int32)
    c = {"none": -1, "all": 10_000, "one_in_1e4": 1}[what]
    exp = check(ex, [[term(k, "<", c)]])
    assert len(exp) == {"none": 0, "all": n}.get(what, len(exp))
    assert what != "one_in_1e4" or 0 < len(exp) < 40


def test_whole_tiles_pass_and_neighbours_fail(ex):
    """tiles 0, 1, 4, 5, ... pass the first clause entirely, tiles 2, 3, 6,
    7, ... fail it entirely: their waves skip the second clause's columns
    and their tile offsets repeat"""
    rng = np.random.default_rng(6)
    n = 11 * TILE + 100
    k = ((np.arange(n) // (2 * TILE)) % 2).astype(np.uint8)
    f = rng.normal(0, 1, n)
    fn = (rng.random(n) < 0.1).astype(np.uint8)
    check(ex, [[term(k, "=", 0)]])
    check(ex, [[term(k, "=", 0)], [term(f, "<", 0.5, fn)]])
    # dead and live waves inside one tile: 1024-row stripes
    w = ((np.arange(n) // 1024) % 3 == 0).astype(np.uint8)
    check(ex, [[term(w, "=", 1)], [term(f, ">=", 0.0, fn)]])


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("type_", list(DTYPES))
def test_types_and_ops(ex, type_, mask):
    rng = np.random.default_rng(11)
    n = 2 * TILE + 1811
    col = column(rng, type_, n)
    nl = (rng.random(n) < 0.15).astype(np.uint8) if mask else None
    c = median_const(type_)
    col[::7] = c                                       # "=" hits
    for op in OPS:
        if op in ("isnull", "notnull"):
            check(ex, [[term(col, op, nulls=nl)]])
        else:
            check(ex, [[term(col, op, c, nl)]])


def test_column_against_column_i32(ex):
    rng = np.random.default_rng(12)
    n = 3 * TILE + 5
    a = rng.integers(-50, 50, n).astype(np.int32)
    b = rng.integers(-50, 50, n).astype(np.int32)
    an = (rng.random(n) < 0.2).astype(np.uint8)
    bn = (rng.random(n) < 0.2).astype(np.uint8)
    for nl, rn in [(an, bn), (an, None), (None, bn), (None, None)]:
        check(ex, [[term(a, "<", b, nl, rn)]])
    for op in OPS[:6]:
        check(ex, [[term(a, op, b, an, bn)]])
    for type_ in ("i64", "f64", "u8"):
        x, y = column(rng, type_, n), column(rng, type_, n)
        y[::3] = x[::3]
        check(ex, [[term(x, "<=", y, an, bn)]])
        check(ex, [[term(x, "=", y)]])


def test_float_edges_against_every_edge_constant(ex):
    rng = np.random.default_rng(21)
    n = TILE + 301
    f = F64_EDGE[rng.integers(0, len(F64_EDGE), n)]
    f[:len(F64_EDGE)] = F64_EDGE
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    fd, nd = dev(f), dev(nl)
    from opentenbase_amd import executor
    for c in F64_EDGE:
        for op in OPS[:6]:
            node = executor.GpuFilter(
                [[executor.qual_term(fd, op, float(c), nulls=nd)]])
            node.BeginCustomScan()
            got = node.ExecCustomScan().cpu().numpy()
            node.EndCustomScan()
            assert np.array_equal(got, ref_sel([[term(f, op, float(c), nl)]])), \
                (op, c)
    g = F64_EDGE[rng.integers(0, len(F64_EDGE), n)]
    for op in OPS[:6]:
        check(ex, [[term(f, op, g, nl)]])


def test_int_edges(ex):
    rng = np.random.default_rng(22)
    n = TILE + 9
    k = rng.choice(np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1,
                             I64_MAX], dtype=np.int64), n)
    for c in (I64_MIN, I64_MIN + 1, 0, I64_MAX - 1, I64_MAX):
        for op in OPS[:6]:
            check(ex, [[term(k, op, c)]])
    i = rng.choice(np.array([-2**31, -1, 0, 2**31 - 1], dtype=np.int32), n)
    for c in (2**40, -2**40, 2**31, -2**31 - 1, 2**32, -2**31, 2**31 - 1):
        for op in OPS[:6]:
            check(ex, [[term(i, op, c)]])
    u = rng.choice(np.array([0, 1, 127, 128, 255], dtype=np.uint8), n)
    for c in (-1, 256, 0, 255, -256, 2**32 + 5):
        for op in OPS[:6]:
            check(ex, [[term(u, op, c)]])
    assert len(ref_sel([[term(u, "<", 256)]])) == n
    assert len(ref_sel([[term(i, "=", 2**40)]])) == 0


def test_garbage_under_nulls_is_never_read(ex):
    rng = np.random.default_rng(23)
    n = 2 * TILE + 3
    nl = (rng.random(n) < 0.3).astype(np.uint8)
    f0 = np.where(nl, 0.0, rng.normal(0, 1, n))
    k0 = np.where(nl, 0, rng.integers(-5, 5, n)).astype(np.int64)
    f1, k1 = f0.copy(), k0.copy()
    f1[nl != 0] = np.nan
    k1[nl != 0] = I64_MIN
    for op in OPS:
        rhs = (None, None) if op in ("isnull", "notnull") else (0.0, 0)
        a = gpu_sel(ex, [[term(f0, op, rhs[0], nl)], [term(k0, "<=", 3, nl),
                                                      term(k0, "isnull",
                                                           nulls=nl)]])
        b = gpu_sel(ex, [[term(f1, op, rhs[0], nl)], [term(k1, "<=", 3, nl),
                                                      term(k1, "isnull",
                                                           nulls=nl)]])
        assert np.array_equal(a, b)
        a = check(ex, [[term(k0, op, rhs[1], nl), term(f0, "<", 0.0, nl)]])
        b = gpu_sel(ex, [[term(k1, op, rhs[1], nl), term(f1, "<", 0.0, nl)]])
        assert np.array_equal(a, b)
    # as the right operand too
    x = rng.normal(0, 1, n)
    assert np.array_equal(gpu_sel(ex, [[term(x, "<", f0, None, nl)]]),
                          gpu_sel(ex, [[term(x, "<", f1, None, nl)]]))


def test_truth_tables(ex):
    total = 0
    for name, clauses, exp in truth_cases():
        got = gpu_sel(ex, clauses)
        total += len(clauses[0][0][0])
        assert got.tolist() == exp, name
        assert np.array_equal(got, ref_sel(clauses))
    assert total == 45


def test_sixteen_terms_four_columns_four_types(ex):
    rng = np.random.default_rng(31)
    n = 5 * TILE + 123
    a = rng.integers(-100, 100, n).astype(np.int64)
    f = rng.normal(0, 1, n)
    i = rng.integers(0, 2400, n).astype(np.int32)
    u = rng.integers(0, 25, n).astype(np.uint8)
    an, fn, in_, un = ((rng.random(n) < 0.1).astype(np.uint8)
                       for _ in range(4))
    clauses = [
        [term(i, "<=", 2300, in_), term(i, "isnull", nulls=in_)],
        [term(u, "=", 3, un), term(u, "=", 7, un), term(u, "=", 11, un),
         term(u, ">", 15, un), term(a, "<", -90, an)],
        [term(f, "<", 1.0, fn), term(f, ">", 2.0, fn),
         term(f, "isnull", nulls=fn)],
        [term(a, "<>", 0, an)],
        [term(a, ">=", -50, an), term(i, "<", 100, in_),
         term(f, "notnull", nulls=fn), term(u, "<>", 4, un)],
        [term(a, "notnull", nulls=an)],
    ]
    assert sum(len(c) for c in clauses) == 16
    exp = check(ex, clauses)
    assert 0 < len(exp) < n


def test_no_qual_selects_every_row(ex):
    for n in (0, 1, TILE, 2 * TILE + 5):
        got = gpu_sel(ex, [], n)
        assert np.array_equal(got, np.arange(n, dtype=np.int64))


@pytest.mark.parametrize("type_", list(DTYPES))
def test_unaligned_views(ex, type_):
    """col = base[1:], mask = mask_base[3:]: natural alignment only"""
    rng = np.random.default_rng(41)
    n = 3 * TILE + 40
    col, other = column(rng, type_, n), column(rng, type_, n)
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    c = median_const(type_)
    node = to_node(ex, [[term(col, "<", c, nl)]], col_skip=1, mask_skip=3)
    t = node.clauses[0][0]
    assert t.col.data_ptr() % 16 == t.col.element_size()
    assert t.nulls.data_ptr() % 16 == 3
    check(ex, [[term(col, "<", c, nl)]], col_skip=1, mask_skip=3)
    check(ex, [[term(col, ">=", other, nl, nl)]], col_skip=1, mask_skip=3)
    check(ex, [[term(col, ">=", other, nl, nl)]], col_skip=3, mask_skip=0)
    check(ex, [[term(col, "isnull", nulls=nl)]], col_skip=0, mask_skip=1)


def test_count_only_and_untouched_tail(ex):
    rng = np.random.default_rng(51)
    n = 4 * TILE + 11
    k = rng.integers(0, 100, n).astype(np.int32)
    nl = (rng.random(n) < 0.1).astype(np.uint8)
    clauses = [[term(k, "<", 30, nl)]]
    exp = ref_sel(clauses)
    node = to_node(ex, clauses, count_only=True)
    node.BeginCustomScan()
    assert node.ExecCustomScan() == (len(exp),)
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    assert node.count == len(exp) and node.sel is None

    # a direct call: sel pre-filled with -1 is untouched beyond nsel
    from opentenbase_amd._lib import call, lib
    full = to_node(ex, clauses)
    q = full.qual()
    wsb = C.c_size_t(0)
    assert lib().otbx_filter_workspace_bytes(n, C.byref(wsb)) == 0
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    sel = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    nsel = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call("otbx_filter_sel", C.byref(q), C.c_int64(n),
         C.c_void_p(ws.data_ptr()), C.c_size_t(wsb.value),
         C.c_void_p(sel.data_ptr()), C.c_void_p(nsel.data_ptr()), stream)
    torch.cuda.synchronize()
    got = sel.cpu().numpy()
    assert int(nsel.item()) == len(exp)
    assert np.array_equal(got[:len(exp)], exp)
    assert (got[len(exp):] == -1).all()
    # count-only through the C entry point: sel_dev = NULL
    nsel.fill_(-7)
    call("otbx_filter_sel", C.byref(q), C.c_int64(n),
         C.c_void_p(ws.data_ptr()), C.c_size_t(wsb.value), None,
         C.c_void_p(nsel.data_ptr()), stream)
    torch.cuda.synchronize()
    assert int(nsel.item()) == len(exp)
    # n == 0 writes a zero count
    nsel.fill_(-7)
    call("otbx_filter_sel", C.byref(q), C.c_int64(0), None, C.c_size_t(0),
         None, C.c_void_p(nsel.data_ptr()), stream)
    torch.cuda.synchronize()
    assert int(nsel.item()) == 0


def test_composition_with_gather_and_hashagg(ex):
    rng = np.random.default_rng(61)
    n = 6 * TILE + 321
    key = rng.integers(0, 50, n).astype(np.int64)
    val = rng.integers(-1000, 1000, n).astype(np.float64)   # exact sums
    date = rng.integers(0, 2400, n).astype(np.int32)
    flag = rng.integers(0, 3, n).astype(np.uint8)
    clauses = [[term(date, "<=", 1200)], [term(flag, "=", 0),
                                          term(flag, "=", 2)]]
    ref = ref_sel(clauses)
    node = to_node(ex, clauses)
    for col in (key, val, date, flag):
        assert np.array_equal(node.gather(dev(col)).cpu().numpy(), col[ref])
    assert node.count == len(ref) and node.explain()["filter"] > 0

    def groups(k, v):
        agg = ex.GpuHashAgg(k, v)
        agg.BeginCustomScan()
        rows = []
        while (r := agg.ExecCustomScan()) is not None:
            rows.append(tuple(r))
        agg.EndCustomScan()
        return rows

    got = groups(node.gather(dev(key)), node.gather(dev(val)))
    exp = groups(dev(key[ref]), dev(val[ref]))
    assert got == exp and len(got) == 50
    assert sum(r[1] for r in got) == len(ref)


def test_lifecycle(ex):
    rng = np.random.default_rng(71)
    n = TILE + 7
    k = rng.integers(0, 10, n).astype(np.int32)
    clauses = [[term(k, ">=", 5)]]
    exp = ref_sel(clauses)
    node = to_node(ex, clauses)
    from opentenbase_amd._lib import OtbxError
    with pytest.raises(OtbxError):
        node.ExecCustomScan()
    assert node.explain() is None
    node.BeginCustomScan()
    assert np.array_equal(node.ExecCustomScan().cpu().numpy(), exp)
    assert node.ExecCustomScan() is None
    assert node.explain()["filter"] >= 0
    node.ReScanCustomScan()
    assert np.array_equal(node.ExecCustomScan().cpu().numpy(), exp)
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    with pytest.raises(OtbxError):
        node.ExecCustomScan()

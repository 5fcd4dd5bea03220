"""CPU-side tests of the Filter operator's host layers: the two reference
implementations agree, the three-valued truth tables, the argument checks
and workspace sizing of otbx_filter_sel (pure host code — no HIP call is
reached), the GpuFilter argument checks and the ctypes layout of the qual."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import QualDev, QualTermDev
from filter_ref import OPS, ref_sel, step_sel, term, truth_cases
from test_gpu_sort import F64_EDGE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
DTYPES = (np.int64, np.float64, np.int32, np.uint8)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def small_col(rng, dtype, n):
    """few distinct values, so that =, < and > all hit"""
    if dtype == np.float64:
        return rng.choice(np.array([-1.5, -0.0, 0.0, 2.0, np.nan, np.inf]), n)
    if dtype == np.uint8:
        return rng.integers(0, 5, n).astype(np.uint8)
    return rng.integers(-2, 3, n).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_ref_sel_equals_step_sel_every_op_and_type(op, dtype):
    rng = np.random.default_rng(OPS.index(op) * 4 + DTYPES.index(dtype))
    n = 400
    col = small_col(rng, dtype, n)
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    if op in ("isnull", "notnull"):
        quals = [[[term(col, op, nulls=nl)]], [[term(col, op)]]]
    else:
        other = small_col(rng, dtype, n)
        rn = (rng.random(n) < 0.2).astype(np.uint8)
        c = 0.0 if dtype == np.float64 else 1
        quals = [[[term(col, op, c, nl)]], [[term(col, op, c)]],
                 [[term(col, op, other, nl, rn)]],
                 [[term(col, op, other, None, rn)]],
                 # OR with a second term, AND with a second clause
                 [[term(col, op, c, nl), term(other, "=", c, rn)],
                  [term(other, "notnull", nulls=rn), term(col, "<", c, nl)]]]
    for q in quals:
        a, b = ref_sel(q), step_sel(q)
        assert a.dtype == np.int64 and b.dtype == np.int64
        assert np.array_equal(a, b)
    # 20 % NULLs: a nullable "=" can never select a NULL row
    if op == "=":
        assert not nl[ref_sel(quals[0])].any()


@pytest.mark.parametrize("op", OPS[:6])
def test_ref_sel_equals_step_sel_on_float_edges(op):
    rng = np.random.default_rng(7)
    n = len(F64_EDGE) * 8
    col = F64_EDGE[rng.integers(0, len(F64_EDGE), n)]
    col[:len(F64_EDGE)] = F64_EDGE
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    for c in F64_EDGE:
        q = [[term(col, op, float(c), nl)]]
        assert np.array_equal(ref_sel(q), step_sel(q))
    other = F64_EDGE[rng.integers(0, len(F64_EDGE), n)]
    q = [[term(col, op, other, nl)]]
    assert np.array_equal(ref_sel(q), step_sel(q))


def test_float_order_is_float8_cmp_internal():
    nan2 = np.array([0xfff8000000000001], dtype=np.uint64).view(np.float64)[0]
    col = np.array([np.nan, nan2, np.inf, -0.0, 0.0, -np.inf, 1.0])
    for f in (ref_sel, step_sel):
        assert f([[term(col, "=", float("nan"))]]).tolist() == [0, 1]
        assert f([[term(col, ">", float("inf"))]]).tolist() == [0, 1]
        assert f([[term(col, "<", float("nan"))]]).tolist() == [2, 3, 4, 5, 6]
        assert f([[term(col, "=", 0.0)]]).tolist() == [3, 4]
        assert f([[term(col, "<", 0.0)]]).tolist() == [5]
        assert f([[term(col, ">=", -0.0)]]).tolist() == [0, 1, 2, 3, 4, 6]


def test_int_constants_outside_the_column_range():
    u8 = np.array([0, 255, 7], dtype=np.uint8)
    i32 = np.array([-2**31, 2**31 - 1, 0], dtype=np.int32)
    for f in (ref_sel, step_sel):
        assert f([[term(u8, "<", 256)]]).tolist() == [0, 1, 2]
        assert f([[term(u8, ">", -1)]]).tolist() == [0, 1, 2]
        assert f([[term(u8, "=", 256)]]).tolist() == []
        assert f([[term(i32, "=", 2**40)]]).tolist() == []
        assert f([[term(i32, "<", 2**40)]]).tolist() == [0, 1, 2]
        assert f([[term(i32, ">", -2**40)]]).tolist() == [0, 1, 2]
        assert f([[term(i32, "<=", -2**40)]]).tolist() == []


# ---- three-valued logic: every assignment of {TRUE, FALSE, NULL} ----

def test_truth_tables_exhaustive():
    total = 0
    for name, clauses, exp in truth_cases():
        total += len(clauses[0][0][0])
        assert ref_sel(clauses).tolist() == exp, name
        assert step_sel(clauses).tolist() == exp, name
    assert total == 9 + 9 + 27


def test_no_qual_selects_every_row():
    assert ref_sel([], 5).tolist() == [0, 1, 2, 3, 4]
    assert step_sel([], 5).tolist() == [0, 1, 2, 3, 4]
    assert ref_sel([], 0).tolist() == []


def test_golden_aggtest_a_lt_100():
    with open(os.path.join(REPO, "tests", "golden", "expected.json")) as f:
        agg = json.load(f)["aggtest"]
    a = np.array([r[0] for r in agg["rows"]], dtype=np.int64)
    for f in (ref_sel, step_sel):
        sel = f([[term(a, "<", 100)]])
        assert sel.tolist() == [0, 2, 3]
        assert a[sel].mean() == agg["avg_a_lt100"]


# ---- otbx_filter_sel argument checks: all rejected before any HIP call ----

def _ws(so, n):
    out = C.c_size_t(0)
    st = so.otbx_filter_workspace_bytes(n, C.byref(out))
    return st, out.value


def test_filter_workspace_sizing(so):
    prev = -1
    for n in (0, 1, 1000, 10**6, 10**8, INT32_MAX):
        st, b = _ws(so, n)
        assert st == 0 and b >= prev
        if n > 0:
            assert b >= (n + 7) // 8     # one bit per row at least
        prev = b
    assert _ws(so, 0) == (0, 0)
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert so.otbx_filter_workspace_bytes(10, None) == OTBX_ERR_INVALID
    # n/8 B of bitmask plus 4 B per 4096-row tile, to 256-byte granules
    assert _ws(so, 10**8)[1] < 10**8 // 8 * 1.01 + 4096


def _qual(nterms=2, type_=0, op=2, col=0x1000):
    q = QualDev()
    q.nterms = nterms
    for t in range(min(max(nterms, 0), 16)):
        q.term[t].col = col
        q.term[t].type = type_
        q.term[t].op = op
        q.term[t].clause = t
    return q


def _filter(so, q, n, ws_bytes=None, ws=0x1000, sel=0x1000, nsel=0x1000):
    """otbx_filter_sel with dummy (never dereferenced) device pointers."""
    if ws_bytes is None:
        st, ws_bytes = _ws(so, max(min(n, INT32_MAX), 0))
        assert st == 0
    return so.otbx_filter_sel(
        None if q is None else C.byref(q), C.c_int64(n), C.c_void_p(ws),
        C.c_size_t(ws_bytes), C.c_void_p(sel), C.c_void_p(nsel), None)


@pytest.mark.parametrize("case", [
    "null_qual", "null_nsel", "nterms_neg", "nterms17", "type_neg", "type4",
    "op_neg", "op8", "rcol_isnull", "rcol_notnull", "rnulls_without_rcol",
    "clause_decreasing", "n_neg", "n_big", "null_col", "ws_short",
    "ws_unaligned", "ws_null"])
def test_filter_invalid_arguments(so, case):
    n, kw = 100, {}
    q = _qual()
    if case == "null_qual":
        q = None
    elif case == "null_nsel":
        kw["nsel"] = None
    elif case == "nterms_neg":
        q = _qual(nterms=-1)
    elif case == "nterms17":
        q = _qual(nterms=17)
    elif case == "type_neg":
        q = _qual(type_=-1)
    elif case == "type4":
        q = _qual(type_=4)
    elif case == "op_neg":
        q = _qual(op=-1)
    elif case == "op8":
        q = _qual(op=8)
    elif case == "rcol_isnull":
        q = _qual(op=6)
        q.term[1].rcol = 0x1000
    elif case == "rcol_notnull":
        q = _qual(op=7)
        q.term[0].rcol = 0x1000
    elif case == "rnulls_without_rcol":
        q.term[1].rnulls = 0x1000
    elif case == "clause_decreasing":
        q.term[0].clause, q.term[1].clause = 1, 0
    elif case == "n_neg":
        n = -1
    elif case == "n_big":
        n, kw["ws_bytes"] = INT32_MAX + 1, 1 << 62
    elif case == "null_col":
        q = _qual(col=None)
    elif case == "ws_short":
        kw["ws_bytes"] = _ws(so, n)[1] - 1
    elif case == "ws_unaligned":
        kw["ws"] = 0x1008
    elif case == "ws_null":
        kw["ws"] = None
    assert _filter(so, q, n, **kw) == OTBX_ERR_INVALID


def test_filter_bad_term_in_a_later_slot_is_rejected(so):
    q = _qual(nterms=16)
    q.term[15].type = 9
    assert _filter(so, q, 10) == OTBX_ERR_INVALID
    q = _qual(nterms=16)
    q.term[15].op = 8
    assert _filter(so, q, 10) == OTBX_ERR_INVALID
    q = _qual(nterms=3)
    q.term[2].col = None
    assert _filter(so, q, 10) == OTBX_ERR_INVALID


# ---- the ctypes mirror of otbx_qual ----

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "otbx.h"
int main(void)
{
    printf("%zu %zu", sizeof(otbx_qualterm), sizeof(otbx_qual));
    printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu",
           offsetof(otbx_qualterm, col), offsetof(otbx_qualterm, nulls),
           offsetof(otbx_qualterm, rcol), offsetof(otbx_qualterm, rnulls),
           offsetof(otbx_qualterm, ci), offsetof(otbx_qualterm, cf),
           offsetof(otbx_qualterm, type), offsetof(otbx_qualterm, op),
           offsetof(otbx_qualterm, clause));
    printf(" %zu %zu\n", offsetof(otbx_qual, nterms), offsetof(otbx_qual, term));
    return 0;
}
"""


def test_qualdev_matches_the_documented_layout():
    # the numbers include/otbx.h documents and otbx_filter.hip asserts
    assert C.sizeof(QualTermDev) == 64
    assert C.sizeof(QualDev) == 1032
    assert QualDev.term.offset == 8
    assert len(QualDev().term) == ex.MAX_QUAL_TERMS == 16


def test_qualdev_matches_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run(
        [str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = QualTermDev
    assert got == [C.sizeof(QualTermDev), C.sizeof(QualDev),
                   T.col.offset, T.nulls.offset, T.rcol.offset,
                   T.rnulls.offset, T.ci.offset, T.cf.offset, T.type.offset,
                   T.op.offset, T.clause.offset,
                   QualDev.nterms.offset, QualDev.term.offset]


# ---- GpuFilter / qual_term argument checks (CPU tensors, nothing runs) ----

def test_gpufilter_builds_the_qual():
    import torch
    a = torch.zeros(6, dtype=torch.int32)
    b = torch.zeros(6, dtype=torch.int32)
    f = torch.zeros(6, dtype=torch.float64)
    m = torch.zeros(6, dtype=torch.uint8)
    node = ex.GpuFilter([[ex.qual_term(a, "<=", 7, nulls=m)],
                         [ex.qual_term(f, "<", 2.5),
                          ex.qual_term(a, "<", b, rnulls=m)],
                         [ex.qual_term(f, "isnull", nulls=m)]])
    assert node.n == 6 and node.explain() is None and node.count is None
    q = node.qual()
    assert q.nterms == 4
    assert [q.term[i].clause for i in range(4)] == [0, 1, 1, 2]
    assert [q.term[i].op for i in range(4)] == [3, 2, 2, 6]
    assert [q.term[i].type for i in range(4)] == [2, 1, 2, 1]
    assert q.term[0].ci == 7 and q.term[0].nulls == m.data_ptr()
    assert q.term[0].rcol is None and q.term[0].rnulls is None
    assert q.term[1].cf == 2.5 and q.term[1].nulls is None
    assert q.term[2].rcol == b.data_ptr() and q.term[2].rnulls == m.data_ptr()
    assert q.term[3].col == f.data_ptr()
    # an int constant for a float column is converted
    assert ex.GpuFilter([[ex.qual_term(f, "=", 3)]]).qual().term[0].cf == 3.0
    # no qual: every row, n given by the caller
    node = ex.GpuFilter([], n=10, count_only=True)
    assert node.qual().nterms == 0 and node.n == 10 and node.count_only


def test_gpufilter_argument_checks():
    import torch
    a = torch.zeros(6, dtype=torch.int32)
    f = torch.zeros(6, dtype=torch.float64)
    m = torch.zeros(6, dtype=torch.uint8)
    bad = [
        lambda: ex.qual_term(a, "!=", 1),                       # operator
        lambda: ex.qual_term(a.to(torch.int16), "=", 1),        # dtype
        lambda: ex.qual_term([1, 2], "=", 1),                   # not a tensor
        lambda: ex.qual_term(a, "="),                           # no rhs
        lambda: ex.qual_term(a, "=", "1"),
        lambda: ex.qual_term(a, "=", True),
        lambda: ex.qual_term(a, "<", 1.5),                      # int column
        lambda: ex.qual_term(a, "<", 2**63),                    # beyond int64
        lambda: ex.qual_term(a, "<", f),                        # mixed types
        lambda: ex.qual_term(a, "<", a[:5]),                    # lengths
        lambda: ex.qual_term(a, "isnull", 1),
        lambda: ex.qual_term(a, "notnull", rnulls=m),
        lambda: ex.qual_term(a, "<", 1, rnulls=m),
        lambda: ex.qual_term(a, "<", 1, nulls=m[:5]),
        lambda: ex.qual_term(a, "<", 1, nulls=a),               # mask dtype
        lambda: ex.GpuFilter([]),                               # no n
        lambda: ex.GpuFilter([[]], n=6),                        # empty clause
        lambda: ex.GpuFilter([[(a, "<", 1)]]),                  # raw tuple
        lambda: ex.GpuFilter([[ex.qual_term(a, "<", 1)],
                              [ex.qual_term(a[:5], "<", 1)]]),  # lengths
        lambda: ex.GpuFilter([[ex.qual_term(a, "<", 1)]], n=7),
        lambda: ex.GpuFilter([[ex.qual_term(a, "<", i)] for i in range(17)]),
        lambda: ex.GpuFilter([[ex.qual_term(a, "<", i) for i in range(17)]]),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(_lib.OtbxError) as e:
            make()
        assert e.value.status == 3, i
    # 16 terms are fine
    ex.GpuFilter([[ex.qual_term(a, "<", i) for i in range(8)],
                  [ex.qual_term(a, ">", i) for i in range(8)]])
    node = ex.GpuFilter([[ex.qual_term(a, "<", 1)]], count_only=True)
    with pytest.raises(_lib.OtbxError):
        node.gather(a)
    with pytest.raises(_lib.OtbxError):
        node.ExecCustomScan()           # before BeginCustomScan

"""CPU-side tests of the text rank's host layers: the two references agree
with each other and with the reference's regression output (ORDER BY /
DISTINCT over onek), the workspace sizing, the argument checks of
otbx_text_rank (pure host code — no HIP call is reached), the ctypes layout
of otbx_textset, and fragment.merge_text_dictionaries without and with a
process group."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from opentenbase_amd import _lib
from opentenbase_amd import fragment
from opentenbase_amd._lib import TextColDev, TextSetDev
from textkey_ref import (column_rows, rank_cmp, rank_set, text_sort_perm,
                         varstr_cmp_c)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
GOLDEN = os.path.join(REPO, "tests", "golden", "text_order_cases.json")


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


# ---- the two references ----

def test_varstr_cmp_c_is_bytes_order():
    rng = random.Random(3)
    for _ in range(4000):
        a = bytes(rng.choice(b"\0ab\xff") for _ in range(rng.randint(0, 5)))
        b = bytes(rng.choice(b"\0ab\xff") for _ in range(rng.randint(0, 5)))
        assert varstr_cmp_c(a, b) == (a > b) - (a < b), (a, b)
    # the chain of the contract: a 0x00 byte is an ordinary byte
    chain = [b"", b"a", b"a\0", b"a\0\0", b"a\1", b"a\xff", b"b"]
    for x, y in zip(chain, chain[1:]):
        assert varstr_cmp_c(x, y) < 0 and varstr_cmp_c(y, x) > 0


def test_rank_refs_agree_on_random_columns():
    rng = random.Random(17)
    lens = (0, 1, 6, 7, 8, 9, 10, 15, 16, 17, 18, 24, 25)
    ndup = 0
    for _ in range(3000):
        n = rng.randint(0, 40)
        rows = [None if rng.random() < 0.1 else
                bytes(rng.choice(b"\0ab\xff")
                      for _ in range(rng.choice(lens)))
                for _ in range(n)]
        a, b = rank_cmp(rows), rank_set(rows)
        assert a == b, rows
        codes, d, first = a
        live = [r for r in rows if r is not None]
        assert d == len(set(live)) and len(first) == d
        ndup += d < len(live)
        for i, r in enumerate(rows):
            assert (codes[i] == -1) == (r is None)
        for c, i in enumerate(first):
            assert codes[i] == c and rows.index(rows[i]) == i
    assert ndup > 1000   # duplicates are common, or equality is untested


def test_rank_refs_reproduce_golden_orders(golden):
    rows = golden["rows"]
    u1 = [r["unique1"] for r in rows]
    su1 = [r["stringu1"].encode() for r in rows]
    s4 = [r["string4"].encode() for r in rows]
    assert len(rows) == 19
    for rank in (rank_cmp, rank_set):
        c1, d1, _ = rank(su1)
        c4, d4, first4 = rank(s4)
        assert d1 == 19 and d4 == 4
        assert [s4[i].decode() for i in first4] == golden["distinct_string4"]
        order = sorted(range(19), key=lambda i: c1[i])
        assert [[u1[i], su1[i].decode()] for i in order] == \
            golden["orders"]["stringu1_asc"]
        order = sorted(range(19), key=lambda i: (c4[i], -u1[i]))
        assert [[u1[i], s4[i].decode()] for i in order] == \
            golden["orders"]["string4_asc_unique1_desc"]
        order = sorted(range(19), key=lambda i: (-c4[i], u1[i]))
        assert [[u1[i], s4[i].decode()] for i in order] == \
            golden["orders"]["string4_desc_unique1_asc"]
    # and the comparator sort over the strings themselves
    order = text_sort_perm(s4, desc=True, then=u1)
    assert [[u1[i], s4[i].decode()] for i in order] == \
        golden["orders"]["string4_desc_unique1_asc"]


def test_column_rows_clamps_like_the_kernels():
    raw = b"abcdef"
    assert column_rows(raw, [2, 4, 3, 99, -5, 6], [0, 0, 1, 0, 0]) == \
        [b"cd", b"", None, b"", b"abcdef"]


# ---- sizing and layout ----

def _ws(so, n):
    out = C.c_size_t(0)
    return so.otbx_text_rank_workspace_bytes(n, C.byref(out)), out.value


def test_text_rank_workspace_sizing(so):
    prev = 0
    for n in (0, 1, 63, 64, 2047, 2048, 2049, 6144, 10**6, 10**8, INT32_MAX):
        st, b = _ws(so, n)
        assert st == 0 and b >= prev and b > 0
        prev = b
    sort = C.c_size_t(0)
    assert so.otbx_sort_workspace_bytes(10**6, 3, 0, C.byref(sort)) == 0
    assert _ws(so, 10**6)[1] > sort.value     # the sort's workspace is inside
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert so.otbx_text_rank_workspace_bytes(10, None) == OTBX_ERR_INVALID


def test_textset_layout():
    assert C.sizeof(TextSetDev) == 168
    assert TextSetDev.col.offset == 8 and TextSetDev.n.offset == 136
    assert _lib.MAX_TEXT_RANK_COLS == 4


# ---- argument checks: every refusal comes before any HIP call ----

def _col(bytes_=0x1000, offs=0x2000, nulls=None, nbytes=64):
    c = TextColDev()
    c.bytes, c.offs, c.nulls, c.nbytes = bytes_, offs, nulls, nbytes
    return c


def _set(cols=None, ns=None, ncols=None):
    cols = [_col()] if cols is None else cols
    ns = [10] * len(cols) if ns is None else ns
    ts = TextSetDev()
    ts.ncols = len(cols) if ncols is None else ncols
    for i, (c, n) in enumerate(zip(cols, ns)):
        ts.col[i] = c
        ts.n[i] = n
    return ts


def _rank(so, ts, ws=0x10000, ws_bytes=None, codes=0x3000, dict_row=0x4000,
          ndistinct=0x5000, n_total=None):
    if ws_bytes is None:
        if n_total is None:
            n_total = sum(ts.n[i] for i in range(max(min(ts.ncols, 4), 0))) \
                if ts is not None else 0
        ws_bytes = _ws(so, max(min(n_total, INT32_MAX), 0))[1]
    rounds = C.c_int32(-7)
    return so.otbx_text_rank(
        None if ts is None else C.byref(ts), C.c_void_p(ws),
        C.c_size_t(ws_bytes), C.c_void_p(codes), C.c_void_p(dict_row),
        C.c_void_p(ndistinct), C.byref(rounds), None)


BAD = {
    "null_set": lambda so: _rank(so, None),
    "null_ndistinct": lambda so: _rank(so, _set(), ndistinct=None),
    "ncols_zero": lambda so: _rank(so, _set(ncols=0)),
    "ncols_five": lambda so: _rank(so, _set(ncols=5)),
    "ncols_neg": lambda so: _rank(so, _set(ncols=-1)),
    "n_neg": lambda so: _rank(so, _set(ns=[-1])),
    "n_neg_second": lambda so: _rank(so, _set([_col(), _col()], [5, -1])),
    "n_total_big": lambda so: _rank(
        so, _set([_col(), _col()], [INT32_MAX, 1])),
    "n_one_col_big": lambda so: _rank(so, _set(ns=[INT32_MAX + 1])),
    "null_bytes": lambda so: _rank(so, _set([_col(bytes_=None)])),
    "null_offs": lambda so: _rank(so, _set([_col(offs=None)])),
    "nbytes_neg": lambda so: _rank(so, _set([_col(nbytes=-1)])),
    "null_offs_second": lambda so: _rank(
        so, _set([_col(), _col(offs=None)], [3, 3])),
    "null_codes": lambda so: _rank(so, _set(), codes=None),
    "ws_short": lambda so: _rank(so, _set(), ws_bytes=_ws(so, 10)[1] - 1),
    "ws_null": lambda so: _rank(so, _set(), ws=None),
    "ws_unaligned": lambda so: _rank(so, _set(), ws=0x10008),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_text_rank_invalid_arguments(so, case):
    assert BAD[case](so) == OTBX_ERR_INVALID


def test_text_rank_exported_and_listed(so):
    for name in ("otbx_text_rank", "otbx_text_rank_workspace_bytes"):
        assert getattr(so, name, None) is not None
        assert name in _lib.EXPORTED_SYMBOLS


def test_executor_argument_checks():
    from opentenbase_amd import executor as ex
    with pytest.raises(_lib.OtbxError):
        ex.GpuTextRank([])
    with pytest.raises(_lib.OtbxError):
        ex.GpuTextRank([b"not a column"])
    assert ex.GpuTextRank.__doc__ and "GpuSort" in ex.GpuTextRank.__doc__


# ---- the dictionary merge ----

def test_merge_text_dictionaries_identity_without_process_group():
    d = [b"", b"a", b"a\0", b"b\xff"]
    g, remap = fragment.merge_text_dictionaries(d)
    assert g == d and remap.dtype == np.int64
    assert remap.tolist() == [0, 1, 2, 3]
    g, remap = fragment.merge_text_dictionaries([])
    assert g == [] and remap.tolist() == []
    with pytest.raises(_lib.OtbxError):
        fragment.merge_text_dictionaries([b"a", None])


_SHIP = [b"AIR", b"FOB", b"MAIL", b"RAIL", b"REG AIR", b"SHIP", b"TRUCK",
         b"", b"a\0", b"a"]


def _table():
    rng = np.random.default_rng(23)
    n = 600
    return [_SHIP[i] for i in rng.integers(0, len(_SHIP), n)], \
        rng.integers(-50, 50, n)


def _worker_textdict(rank, world, port, q):
    import torch
    from test_fragment_gloo import _init
    _init(rank, world, port)
    rows, vals = _table()
    # rank 0 never sees TRUCK / "a", rank 1 never sees AIR: overlapping,
    # different dictionaries
    drop = (b"TRUCK", b"a") if rank == 0 else (b"AIR",)
    mine = [i for i in range(len(rows))
            if i % world == rank and rows[i] not in drop]
    codes, d, first = rank_set([rows[i] for i in mine])
    local_dict = [rows[mine[i]] for i in first]
    gdict, remap = fragment.merge_text_dictionaries(local_dict)
    cnt = np.zeros(d, dtype=np.int64)
    tot = np.zeros(d, dtype=np.int64)
    for c, i in zip(codes, mine):
        cnt[c] += 1
        tot[c] += vals[i]
    keys = remap[np.arange(d)]
    k, _, aggs = fragment.merge_group_partials(
        [keys], [("count_star", cnt, None),
                 ("sum", tot, np.zeros(d, dtype=np.uint8))])
    if rank == 0:
        q.put((gdict, np.asarray(k[0]).tolist(),
               np.asarray(aggs[0][0]).tolist(),
               np.asarray(aggs[1][0]).tolist()))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_merge_text_dictionaries_two_ranks():
    """Two ranks with overlapping dictionaries: the remapped partial counts
    and sums, merged by merge_group_partials, equal the single-table GROUP
    BY over the strings."""
    from test_fragment_gloo import _run
    gdict, keys, cnt, tot = _run(_worker_textdict)
    rows, vals = _table()
    kept = [i for i in range(len(rows))
            if rows[i] not in ((b"TRUCK", b"a") if i % 2 == 0 else (b"AIR",))]
    exp = {}
    for i in kept:
        e = exp.setdefault(rows[i], [0, 0])
        e[0] += 1
        e[1] += int(vals[i])
    assert gdict == sorted(exp)
    assert keys == list(range(len(gdict)))
    assert cnt == [exp[s][0] for s in gdict]
    assert tot == [exp[s][1] for s in gdict]

"""CPU-side tests of the WindowAgg operator's host layers: the two reference
implementations agree, hand-written cases of the window semantics, the
percent_rank / cume_dist finalizers, and the argument checks and workspace
sizing of otbx_window (pure host code — no HIP call is reached)."""
import ctypes as C
import os

import numpy as np
import pytest

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import SortSpecDev, WindowOutDev
from window_ref import loop_window, ref_window

OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
INT_KEYS = ("row_number", "rank", "dense_rank", "count_star", "part_rows",
            "count_v", "sum_isnull")


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def _rand_col(rng, t, n):
    if t == 0:
        return rng.integers(-2, 3, n).astype(np.int64) * (2**40 + 1)
    if t == 1:
        return rng.choice(np.array([0.5, -0.0, 0.0, np.nan, -np.nan, np.inf,
                                    -np.inf, 7.0]), n)
    if t == 2:
        return rng.integers(-2, 2, n).astype(np.int32)
    return rng.integers(0, 3, n).astype(np.uint8)


def assert_same(a, b, with_vals=True):
    keys = INT_KEYS if with_vals else INT_KEYS[:5]
    assert np.array_equal(a["perm"], b["perm"])
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    if with_vals:
        assert a["sum_v"].tobytes() == b["sum_v"].tobytes()


@pytest.mark.parametrize("seed", range(24))
def test_ref_window_equals_loop_window(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(0, 301))
    nkeys = seed % 5                       # 0..4 keys, all four types occur
    spec = []
    for c in range(nkeys):
        t = (seed + c) % 4
        col = _rand_col(rng, t, n)
        nl = (rng.random(n) < 0.25).astype(np.uint8) if rng.random() < 0.6 \
            else None
        spec.append((col, nl, bool(rng.integers(0, 2)),
                     bool(rng.integers(0, 2))))
    # integer-valued doubles: the per-partition cumsum and the row loop add
    # in the same order, and every partial sum is exact
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    vn = (rng.random(n) < 0.3).astype(np.uint8) if seed % 3 else None
    for npart in range(nkeys + 1):
        assert_same(ref_window(spec, npart, vals, vn),
                    loop_window(spec, npart, vals, vn))
    a = ref_window(spec, 0, n=n)
    assert "sum_v" not in a
    assert_same(a, loop_window(spec, 0, n=n), with_vals=False)


def test_rank_versus_dense_rank_on_ties():
    part = np.zeros(6, dtype=np.int32)
    order = np.array([10, 10, 20, 30, 30, 30], dtype=np.int64)
    for f in (ref_window, loop_window):
        r = f([(part, None, False, False), (order, None, False, False)], 1)
        assert r["row_number"].tolist() == [1, 2, 3, 4, 5, 6]
        assert r["rank"].tolist() == [1, 1, 3, 4, 4, 4]
        assert r["dense_rank"].tolist() == [1, 1, 2, 3, 3, 3]
        assert r["count_star"].tolist() == [2, 2, 3, 6, 6, 6]
        assert r["part_rows"].tolist() == [6] * 6


def test_null_partition_key_forms_one_partition():
    part = np.array([7, 1, 99, 1, -5], dtype=np.int64)   # garbage under NULL
    pn = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    order = np.array([3, 2, 1, 1, 2], dtype=np.int32)
    for f in (ref_window, loop_window):
        r = f([(part, pn, False, False), (order, None, False, False)], 1)
        # partition key 1 first (rows 3, 1), then the NULLs (rows 2, 4, 0)
        assert r["perm"].tolist() == [3, 1, 2, 4, 0]
        assert r["part_rows"].tolist() == [2, 2, 3, 3, 3]
        assert r["row_number"].tolist() == [1, 2, 1, 2, 3]
        assert r["rank"].tolist() == [1, 2, 1, 2, 3]


def test_nan_and_signed_zero_keys_are_peers():
    nan2 = np.array([0xfff8000000000001], dtype=np.uint64).view(np.float64)[0]
    order = np.array([np.nan, 0.0, -0.0, nan2, 1.0], dtype=np.float64)
    for f in (ref_window, loop_window):
        r = f([(order, None, False, False)], 0)
        assert r["perm"].tolist() == [1, 2, 4, 0, 3]
        assert r["rank"].tolist() == [1, 1, 3, 4, 4]
        assert r["dense_rank"].tolist() == [1, 1, 2, 3, 3]
        assert r["count_star"].tolist() == [2, 2, 3, 5, 5]


def test_frame_of_only_nulls_has_null_sum():
    part = np.array([0, 0, 0, 1, 1], dtype=np.uint8)
    order = np.array([1, 1, 2, 1, 2], dtype=np.int32)
    vals = np.array([5.0, 6.0, 7.0, 8.0, 9.0])
    vn = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    for f in (ref_window, loop_window):
        r = f([(part, None, False, False), (order, None, False, False)], 1,
              vals, vn)
        assert r["sum_isnull"].tolist() == [1, 1, 0, 1, 1]
        assert r["sum_v"].tolist() == [0.0, 0.0, 7.0, 0.0, 0.0]
        assert r["count_v"].tolist() == [0, 0, 1, 0, 0]
        assert r["count_star"].tolist() == [2, 2, 3, 1, 2]


def test_whole_partition_is_the_frame_without_order_keys():
    part = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
    vals = np.array([1.0, 10.0, 2.0, 20.0, 4.0])
    for f in (ref_window, loop_window):
        r = f([(part, None, False, False)], 1, vals)
        assert r["sum_v"].tolist() == [30.0, 30.0, 7.0, 7.0, 7.0]
        assert r["rank"].tolist() == [1] * 5
        assert r["row_number"].tolist() == [1, 2, 1, 2, 3]
    r = ref_window([], 0, vals)
    assert r["sum_v"].tolist() == [37.0] * 5 and r["perm"].tolist() == \
        [0, 1, 2, 3, 4]


def test_percent_rank_and_cume_dist_finalizers():
    assert ex.percent_rank(1, 1) == 0.0          # single-row partition
    assert ex.percent_rank(1, 5) == 0.0
    assert ex.percent_rank(3, 5) == 0.5
    assert ex.percent_rank(5, 5) == 1.0
    assert ex.cume_dist(1, 1) == 1.0
    assert ex.cume_dist(2, 8) == 0.25
    rank = np.array([1, 1, 3, 1], dtype=np.int64)
    rows = np.array([3, 3, 3, 1], dtype=np.int64)
    cstar = np.array([2, 2, 3, 1], dtype=np.int64)
    assert ex.percent_rank(rank, rows).tolist() == [0.0, 0.0, 1.0, 0.0]
    assert ex.cume_dist(cstar, rows).tolist() == [2 / 3, 2 / 3, 1.0, 1.0]
    assert ex.percent_rank(2, 4) == (2 - 1) / (4 - 1)


# ---- otbx_window argument checks: all rejected before any HIP call ----

def _ws(so, n):
    out = C.c_size_t(0)
    st = so.otbx_window_workspace_bytes(n, C.byref(out))
    return st, out.value


def test_window_workspace_sizing(so):
    prev = -1
    for n in (0, 1, 1000, 10**6, 10**8):
        st, b = _ws(so, n)
        assert st == 0 and b >= prev
        if n > 0:
            assert b > 0
        prev = b
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX)[0] == 0
    assert so.otbx_window_workspace_bytes(10, None) == OTBX_ERR_INVALID


def _spec(nkeys=2, type_=0, flags=0, col=0x1000):
    sp = SortSpecDev()
    sp.nkeys = nkeys
    for c in range(min(max(nkeys, 0), 8)):
        sp.key[c].col = col
        sp.key[c].nulls = None
        sp.key[c].type = type_
        sp.key[c].flags = flags
    return sp


def _out(**want):
    o = WindowOutDev()
    for k in want:
        setattr(o, k, 0x1000)
    return o


def _window(so, sp, npart, n, out, vals=0x1000, ws_bytes=None):
    """otbx_window with dummy (never dereferenced) device pointers."""
    if ws_bytes is None:
        st, ws_bytes = _ws(so, max(min(n, INT32_MAX), 0))
        assert st == 0
    return so.otbx_window(
        None if sp is None else C.byref(sp), C.c_int32(npart),
        C.c_void_p(0x1000), C.c_int64(n), C.c_void_p(vals), None,
        C.c_void_p(0x1000), C.c_size_t(ws_bytes),
        None if out is None else C.byref(out), None)


@pytest.mark.parametrize("case", [
    "null_spec", "null_out", "nkeys_neg", "nkeys9", "npart_neg", "npart_big",
    "type_neg", "type4", "flags4", "flags_neg", "n_neg", "n_big", "null_col",
    "no_output", "sum_without_isnull", "isnull_without_sum",
    "sum_without_vals", "count_v_without_vals", "ws_short"])
def test_window_invalid_arguments(so, case):
    n, npart, ws, vals = 100, 1, None, 0x1000
    sp = _spec()
    out = _out(rank=1, sum_v=1, sum_isnull=1)
    if case == "null_spec":
        sp = None
    elif case == "null_out":
        out = None
    elif case == "nkeys_neg":
        sp, npart = _spec(nkeys=-1), 0
    elif case == "nkeys9":
        sp = _spec(nkeys=9)
    elif case == "npart_neg":
        npart = -1
    elif case == "npart_big":
        npart = 3
    elif case == "type_neg":
        sp = _spec(type_=-1)
    elif case == "type4":
        sp = _spec(type_=4)
    elif case == "flags4":
        sp = _spec(flags=4)
    elif case == "flags_neg":
        sp = _spec(flags=-1)
    elif case == "n_neg":
        n = -1
    elif case == "n_big":
        n, ws = INT32_MAX + 1, 1 << 62
    elif case == "null_col":
        sp = _spec(col=None)
    elif case == "no_output":
        out = _out()
    elif case == "sum_without_isnull":
        out = _out(rank=1, sum_v=1)
    elif case == "isnull_without_sum":
        out = _out(rank=1, sum_isnull=1)
    elif case == "sum_without_vals":
        vals = None
    elif case == "count_v_without_vals":
        out, vals = _out(count_v=1), None
    elif case == "ws_short":
        ws = _ws(so, n)[1] - 1
    assert _window(so, sp, npart, n, out, vals, ws) == OTBX_ERR_INVALID


def test_window_bad_key_in_later_column_is_rejected(so):
    sp = _spec(nkeys=3)
    sp.key[2].type = 7
    assert _window(so, sp, 1, 10, _out(rank=1)) == OTBX_ERR_INVALID
    sp = _spec(nkeys=3)
    sp.key[1].col = None
    assert _window(so, sp, 1, 10, _out(rank=1)) == OTBX_ERR_INVALID


def test_window_zero_rows_is_valid_and_reaches_no_kernel(so):
    # n == 0 returns before any HIP call, with keys, with none and with a
    # NULL key column (nothing to read)
    assert _window(so, _spec(), 1, 0, _out(rank=1)) == 0
    assert _window(so, _spec(nkeys=0), 0, 0, _out(row_number=1)) == 0
    assert _window(so, _spec(col=None), 2, 0, _out(part_rows=1)) == 0


def test_gpuwindowagg_builds_the_combined_key_list():
    import torch
    p = torch.zeros(4, dtype=torch.int32)
    o1 = torch.zeros(4, dtype=torch.float64)
    o2 = torch.zeros(4, dtype=torch.int64)
    nm = torch.zeros(4, dtype=torch.uint8)
    node = ex.GpuWindowAgg([p], [o1, o2], descending=[True, False],
                           part_nulls=[nm], order_nulls=[None, nm])
    # partition key: ASC NULLS LAST; order keys: the sort_flags defaults
    assert node.flags == [0, 1 | 2, 0]
    assert node.keys == [p, o1, o2] and node.nulls == [nm, None, nm]
    assert node.n == 4 and node.explain() is None
    assert "sum_v" not in node.funcs and "rank" in node.funcs
    node = ex.GpuWindowAgg([], [], vals=o1)
    assert node.n == 4 and "sum_v" in node.funcs
    with pytest.raises(_lib.OtbxError):
        ex.GpuWindowAgg([p], [o1], funcs=("sum_v",))
    with pytest.raises(_lib.OtbxError):
        ex.GpuWindowAgg([p], [o1], funcs=("lag",))
    with pytest.raises(_lib.OtbxError):
        ex.GpuWindowAgg([], [])
    with pytest.raises(_lib.OtbxError):
        ex.GpuWindowAgg([p] * 5, [o1] * 4)

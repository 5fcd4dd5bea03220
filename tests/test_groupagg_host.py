"""CPU-side tests of the GroupAggregate operator's host layers: the two
reference implementations agree, hand-written cases of the aggregate
semantics, the avg_f64 / int128_sums finalizers, the argument checks and
workspace sizing of otbx_group_agg (pure host code — no HIP call is reached)
and the Coordinator combine merge_group_partials over gloo."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import AggCallDev, AggCallsDev, SortSpecDev
from groupagg_ref import assert_same, loop_groupagg, ref_groupagg
from test_fragment_gloo import _init, _run

OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
INT64_MAX, INT64_MIN = 2**63 - 1, -2**63
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def _rand_col(rng, t, n):
    """the key value sets of test_window_host.py::_rand_col"""
    if t == 0:
        return rng.integers(-2, 3, n).astype(np.int64) * (2**40 + 1)
    if t == 1:
        return rng.choice(np.array([0.5, -0.0, 0.0, np.nan, -np.nan, np.inf,
                                    -np.inf, 7.0]), n)
    if t == 2:
        return rng.integers(-2, 2, n).astype(np.int32)
    return rng.integers(0, 3, n).astype(np.uint8)


def _rand_val(rng, t, n):
    """value columns: integer-valued doubles (every order exact) with ±0 and
    NaN of both signs for the MIN/MAX ties; wide int64 for the int128 sum."""
    if t == 0:
        return rng.integers(-2**62, 2**62, n, dtype=np.int64) * 2 + \
            rng.integers(0, 2, n)
    if t == 1:
        v = rng.integers(-1000, 1001, n).astype(np.float64)
        v[rng.random(n) < 0.1] = -0.0
        v[rng.random(n) < 0.1] = 0.0
        return v
    if t == 2:
        return rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    return rng.integers(0, 256, n).astype(np.uint8)


def _rand_mm_f64(rng, n):
    return rng.choice(np.array([0.5, -0.0, 0.0, np.nan, -np.nan, np.inf,
                                -np.inf, 7.0, -3.0]), n)


def all_aggs(rng, n, with_nulls=True):
    """every func x type once (14 aggregates), in lists of at most 8"""
    def mask():
        return (rng.random(n) < 0.3).astype(np.uint8) if with_nulls and \
            rng.random() < 0.7 else None
    cols = {t: _rand_val(rng, t, n) for t in range(4)}
    aggs = [("count_star", None, None), ("count", cols[2], mask())]
    for t in range(4):
        aggs.append(("sum", cols[t], mask()))
    for f in ("min", "max"):
        for t in range(4):
            col = _rand_mm_f64(rng, n) if t == 1 else cols[t]
            aggs.append((f, col, mask()))
    return aggs


@pytest.mark.parametrize("seed", range(24))
def test_ref_groupagg_equals_loop_groupagg(seed):
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.integers(0, 301)) if seed else 0
    nkeys = seed % 5                       # 0..4 keys, all four types occur
    spec = []
    for c in range(nkeys):
        t = (seed + c) % 4
        col = _rand_col(rng, t, n)
        nl = (rng.random(n) < 0.25).astype(np.uint8) if rng.random() < 0.6 \
            else None
        spec.append((col, nl, bool(rng.integers(0, 2)),
                     bool(rng.integers(0, 2))))
    aggs = all_aggs(rng, n)
    assert len(aggs) == 14
    a, b = ref_groupagg(spec, aggs, n=n), loop_groupagg(spec, aggs, n=n)
    assert_same(a, b)
    # unsorted input (identity order): non-adjacent equal keys stay apart
    ident = np.arange(n, dtype=np.int64)
    assert_same(ref_groupagg(spec, aggs, perm=ident, n=n),
                loop_groupagg(spec, aggs, perm=ident, n=n))
    # DISTINCT
    assert_same(ref_groupagg(spec, [], n=n), loop_groupagg(spec, [], n=n))


def _nan(payload, neg=False):
    bits = 0x7ff8000000000000 | payload | ((1 << 63) if neg else 0)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def _one_group(func, vals, nulls=None):
    vals = np.asarray(vals)
    key = np.zeros(len(vals), dtype=np.int32)
    out = []
    for f in (ref_groupagg, loop_groupagg):
        r = f([(key, None, False, False)], [(func, vals, nulls)])
        assert r["ngroups"] == 1
        out.append(r["aggs"][0])
    assert out[0]["val"].tobytes() == out[1]["val"].tobytes()
    assert np.array_equal(out[0]["null"], out[1]["null"])
    return out[0]


def test_float_minmax_ties_take_the_later_row():
    na, nb = _nan(0xa), _nan(0xb, neg=True)
    assert _bits(_one_group("max", [0.0, -0.0])["val"]) == _bits([-0.0])
    assert _bits(_one_group("max", [-0.0, 0.0])["val"]) == _bits([0.0])
    assert _bits(_one_group("min", [0.0, -0.0])["val"]) == _bits([-0.0])
    assert _bits(_one_group("min", [-0.0, 0.0])["val"]) == _bits([0.0])
    assert _bits(_one_group("max", [na, 1.0, nb])["val"]) == _bits([nb])
    assert _bits(_one_group("max", [nb, 1.0, na])["val"]) == _bits([na])
    assert _bits(_one_group("min", [1.0, na])["val"]) == _bits([1.0])
    assert _bits(_one_group("min", [na, 1.0])["val"]) == _bits([1.0])
    assert _bits(_one_group("min", [na, nb])["val"]) == _bits([nb])
    assert _bits(_one_group("min", [nb, na])["val"]) == _bits([na])
    assert _bits(_one_group("max", [np.inf, na, 5.0])["val"]) == _bits([na])
    # a NULL never wins, whatever is stored under it
    m = np.array([0, 1, 0], dtype=np.uint8)
    assert _bits(_one_group("max", [1.0, na, 2.0], m)["val"]) == _bits([2.0])


def test_group_of_only_nulls():
    key = np.array([0, 0, 1, 1], dtype=np.uint8)
    v = np.array([5.0, 6.0, 7.0, 8.0])
    vi = np.array([5, 6, 7, 8], dtype=np.int64)
    m = np.array([1, 1, 0, 1], dtype=np.uint8)
    aggs = [("sum", v, m), ("min", v, m), ("max", vi, m), ("count", v, m),
            ("count_star",), ("sum", vi, m)]
    for f in (ref_groupagg, loop_groupagg):
        r = f([(key, None, False, False)], aggs)
        a = r["aggs"]
        assert r["ngroups"] == 2 and r["first_row"].tolist() == [0, 2]
        assert a[0]["null"].tolist() == [1, 0] and \
            a[0]["val"].tolist() == [0.0, 7.0]
        assert a[1]["null"].tolist() == [1, 0] and \
            a[1]["val"].tolist() == [0.0, 7.0]
        assert a[2]["null"].tolist() == [1, 0] and \
            a[2]["val"].tolist() == [0, 7]
        assert a[3]["val"].tolist() == [0, 1] and a[3]["null"] is None
        assert a[4]["val"].tolist() == [2, 2]
        assert a[5]["null"].tolist() == [1, 0] and \
            a[5]["val"].tolist() == [0, 7] and a[5]["hi"].tolist() == [0, 0]


def test_plain_aggregate_over_no_rows_emits_one_row():
    e = np.zeros(0)
    ei = np.zeros(0, dtype=np.int64)
    aggs = [("count_star",), ("count", e), ("sum", e), ("min", ei),
            ("sum", ei)]
    for f in (ref_groupagg, loop_groupagg):
        r = f([], aggs, n=0)
        assert r["ngroups"] == 1 and r["first_row"].tolist() == [-1]
        a = r["aggs"]
        assert a[0]["val"].tolist() == [0] and a[1]["val"].tolist() == [0]
        for x in a[2:]:
            assert x["null"].tolist() == [1] and x["val"].tolist() == [0]
        assert a[4]["hi"].tolist() == [0]
        # with keys: no group at all
        r = f([(ei, None, False, False)], aggs)
        assert r["ngroups"] == 0 and len(r["aggs"][2]["val"]) == 0


def test_int64_sum_is_exact_in_hi_lo():
    cases = [([INT64_MAX, INT64_MAX, 1], 2 * INT64_MAX + 1),
             ([INT64_MIN, -1], INT64_MIN - 1),
             ([INT64_MIN, INT64_MIN, INT64_MIN], 3 * INT64_MIN),
             ([-1, 1], 0), ([-1], -1)]
    for vals, total in cases:
        a = _one_group("sum", np.array(vals, dtype=np.int64))
        got = ex.int128_sums(a["val"], a["hi"], a["null"])
        assert got == [total], (vals, got)
        assert int(a["val"][0]) == total & (2**64 - 1)
        assert int(a["hi"][0]) == total >> 64
    # [INT64_MAX, INT64_MAX, 1] carries out of the low word
    a = _one_group("sum", np.array([INT64_MAX, INT64_MAX, 1], dtype=np.int64))
    assert int(a["hi"][0]) == 0 and int(a["val"][0]) == 2**64 - 1
    a = _one_group("sum", np.array([INT64_MAX, INT64_MAX, 2], dtype=np.int64))
    assert int(a["hi"][0]) == 1 and int(a["val"][0]) == 0


def test_non_adjacent_equal_keys_form_separate_groups():
    key = np.array([1, 1, 2, 1, 1, 1], dtype=np.int64)
    v = np.arange(6, dtype=np.float64)
    ident = np.arange(6, dtype=np.int64)
    for f in (ref_groupagg, loop_groupagg):
        r = f([(key, None, False, False)], [("count_star",), ("sum", v)],
              perm=ident)
        assert r["ngroups"] == 3 and r["first_row"].tolist() == [0, 2, 3]
        assert r["aggs"][0]["val"].tolist() == [2, 1, 3]
        assert r["aggs"][1]["val"].tolist() == [1.0, 2.0, 12.0]
        r = f([(key, None, False, False)], [("count_star",)])
        assert r["ngroups"] == 2 and r["aggs"][0]["val"].tolist() == [5, 1]


def test_null_nan_and_signed_zero_keys_group_together():
    k = np.array([np.nan, 0.0, -0.0, -np.nan, 1.0, 9.0, 8.0])
    kn = np.array([0, 0, 0, 0, 0, 1, 1], dtype=np.uint8)
    for f in (ref_groupagg, loop_groupagg):
        r = f([(k, kn, False, False)], [("count_star",)])
        # ±0, 1.0, the NaNs, the NULLs
        assert r["aggs"][0]["val"].tolist() == [2, 1, 2, 2]
        assert r["first_row"].tolist() == [1, 4, 0, 5]


def test_finalizers():
    assert ex.avg_f64(10.0, 4) == 2.5
    assert ex.avg_f64(0.0, 0) is None
    out = ex.avg_f64(np.array([1.0, 0.0, 9.0]), np.array([2, 0, 3]))
    assert out[0] == 0.5 and np.isnan(out[1]) and out[2] == 3.0
    assert ex.int128_sums(np.array([2**64 - 1], dtype=np.uint64),
                          np.array([-1], dtype=np.int64)) == [-1]
    assert ex.int128_sums(torch.tensor([-1]), torch.tensor([0])) == \
        [2**64 - 1]
    assert ex.int128_sums(np.array([5], dtype=np.uint64),
                          np.array([0], dtype=np.int64),
                          np.array([1], dtype=np.uint8)) == [None]
    # dec_avg takes the exact integer sum
    assert ex.dec_avg(ex.int128_sums(np.array([7], dtype=np.uint64),
                                     np.array([0], dtype=np.int64))[0], 2) == 4


def test_gpugroupagg_argument_handling():
    k = torch.zeros(4, dtype=torch.int32)
    v = torch.zeros(4, dtype=torch.float64)
    node = ex.GpuGroupAgg([k], [("count_star",), ("sum", v)],
                          descending=[True])
    assert node.n == 4 and node.flags == [1 | 2] and node.explain() is None
    assert ex.GpuGroupAgg([], [("max", v, None)]).n == 4
    assert ex.GpuGroupAgg([], [("count_star",)], n=7).n == 7
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([], [("count_star",)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([k], [("avg", v)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([k], [("sum",)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([k], [("count_star",)] * 9)
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([k] * 9, [("count_star",)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuGroupAgg([k.to(torch.int16)], [("count_star",)])


# ---- otbx_group_agg argument checks: all rejected before any HIP call ----

def test_struct_sizes_match_the_header():
    hdr = open(os.path.join(REPO, "include", "otbx.h")).read()
    assert re.search(r"\}\s*otbx_aggcall;\s*/\*\s*48 B\s*\*/", hdr)
    assert int(re.search(r"#define OTBX_MAX_AGGS (\d+)", hdr).group(1)) == \
        _lib.MAX_AGGS == 8
    assert C.sizeof(AggCallDev) == 48
    assert C.sizeof(AggCallsDev) == 8 + 8 * 48
    assert AggCallDev.func.offset == 40 and AggCallDev.type.offset == 44
    assert AggCallsDev.agg.offset == 8
    m = re.search(r"enum \{ OTBX_AGG_COUNT_STAR = 0, OTBX_AGG_COUNT, "
                  r"OTBX_AGG_SUM,\s*OTBX_AGG_MIN, OTBX_AGG_MAX \};", hdr)
    assert m and _lib.AGG_FUNCS == {"count_star": 0, "count": 1, "sum": 2,
                                    "min": 3, "max": 4}


def _ws(so, n):
    out = C.c_size_t(0)
    st = so.otbx_group_agg_workspace_bytes(n, C.byref(out))
    return st, out.value


def test_group_agg_workspace_sizing(so):
    prev = -1
    for n in (0, 1, 1000, 2048, 2049, 10**6, 10**8, INT32_MAX):
        st, b = _ws(so, n)
        assert st == 0 and b >= prev
        if n > 0:
            assert b > 0
        prev = b
    assert _ws(so, 0)[1] == 0
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert so.otbx_group_agg_workspace_bytes(10, None) == OTBX_ERR_INVALID


def _spec(nkeys=2, type_=0, flags=0, col=0x1000):
    sp = SortSpecDev()
    sp.nkeys = nkeys
    for c in range(min(max(nkeys, 0), 8)):
        sp.key[c].col = col
        sp.key[c].nulls = None
        sp.key[c].type = type_
        sp.key[c].flags = flags
    return sp


P = 0x1000   # a dummy device pointer: never dereferenced


def _agg(func, type_=1, col=P, out=P, out_hi=None, out_null="auto"):
    if out_null == "auto":
        out_null = None if func in (0, 1) else P
    return dict(func=func, type=type_, col=col, out=out, out_hi=out_hi,
                out_null=out_null)


def _calls(aggs, naggs=None):
    cs = AggCallsDev()
    cs.naggs = len(aggs) if naggs is None else naggs
    for i, a in enumerate(aggs[:8]):
        for k, v in a.items():
            setattr(cs.agg[i], k, v)
    return cs


def _group_agg(so, sp, n, calls, ws_bytes=None, ws=P, first=P, ng=P):
    """otbx_group_agg with dummy (never dereferenced) device pointers."""
    if ws_bytes is None:
        st, ws_bytes = _ws(so, max(min(n, INT32_MAX), 0))
        assert st == 0
    return so.otbx_group_agg(
        None if sp is None else C.byref(sp), C.c_void_p(P), C.c_int64(n),
        None if calls is None else C.byref(calls), C.c_void_p(ws),
        C.c_size_t(ws_bytes), C.c_void_p(first), C.c_void_p(ng), None)


@pytest.mark.parametrize("case", [
    "null_spec", "null_aggs", "null_ngroups", "nkeys_neg", "nkeys9",
    "naggs_neg", "naggs9", "key_type_neg", "key_type4", "key_flags4",
    "key_flags_neg", "func_neg", "func5", "type_neg", "type4",
    "sum_null_col", "min_null_col", "max_null_col", "null_out",
    "count_null_out", "sum_without_out_null", "min_without_out_null",
    "count_with_out_null", "count_star_with_out_null", "sum_i64_without_hi",
    "sum_f64_with_hi", "sum_i32_with_hi", "max_i64_with_hi", "count_with_hi",
    "nothing_requested", "n_neg", "n_big", "null_key_col", "ws_short",
    "ws_null", "ws_misaligned", "bad_agg_in_last_slot"])
def test_group_agg_invalid_arguments(so, case):
    n, ws_bytes, ws, first, ng = 100, None, P, P, P
    sp = _spec()
    good = [_agg(0), _agg(2)]
    calls = _calls(good)
    if case == "null_spec":
        sp = None
    elif case == "null_aggs":
        calls = None
    elif case == "null_ngroups":
        ng = None
    elif case == "nkeys_neg":
        sp = _spec(nkeys=-1)
    elif case == "nkeys9":
        sp = _spec(nkeys=9)
    elif case == "naggs_neg":
        calls = _calls(good, naggs=-1)
    elif case == "naggs9":
        calls = _calls([_agg(0)] * 8, naggs=9)
    elif case == "key_type_neg":
        sp = _spec(type_=-1)
    elif case == "key_type4":
        sp = _spec(type_=4)
    elif case == "key_flags4":
        sp = _spec(flags=4)
    elif case == "key_flags_neg":
        sp = _spec(flags=-1)
    elif case == "func_neg":
        calls = _calls([_agg(-1)])
    elif case == "func5":
        calls = _calls([_agg(5)])
    elif case == "type_neg":
        calls = _calls([_agg(2, type_=-1)])
    elif case == "type4":
        calls = _calls([_agg(0, type_=4)])
    elif case == "sum_null_col":
        calls = _calls([_agg(2, col=None)])
    elif case == "min_null_col":
        calls = _calls([_agg(3, col=None)])
    elif case == "max_null_col":
        calls = _calls([_agg(4, type_=2, col=None)])
    elif case == "null_out":
        calls = _calls([_agg(2, out=None)])
    elif case == "count_null_out":
        calls = _calls([_agg(1, out=None)])
    elif case == "sum_without_out_null":
        calls = _calls([_agg(2, out_null=None)])
    elif case == "min_without_out_null":
        calls = _calls([_agg(3, out_null=None)])
    elif case == "count_with_out_null":
        calls = _calls([_agg(1, out_null=P)])
    elif case == "count_star_with_out_null":
        calls = _calls([_agg(0, out_null=P)])
    elif case == "sum_i64_without_hi":
        calls = _calls([_agg(2, type_=0)])
    elif case == "sum_f64_with_hi":
        calls = _calls([_agg(2, type_=1, out_hi=P)])
    elif case == "sum_i32_with_hi":
        calls = _calls([_agg(2, type_=2, out_hi=P)])
    elif case == "max_i64_with_hi":
        calls = _calls([_agg(4, type_=0, out_hi=P)])
    elif case == "count_with_hi":
        calls = _calls([_agg(1, out_hi=P)])
    elif case == "nothing_requested":
        calls, first = _calls([]), None
    elif case == "n_neg":
        n = -1
    elif case == "n_big":
        n, ws_bytes = INT32_MAX + 1, 1 << 62
    elif case == "null_key_col":
        sp = _spec(col=None)
    elif case == "ws_short":
        ws_bytes = _ws(so, n)[1] - 1
    elif case == "ws_null":
        ws = None
    elif case == "ws_misaligned":
        ws = P + 8
    elif case == "bad_agg_in_last_slot":
        calls = _calls([_agg(0)] * 7 + [_agg(2, type_=0)])
    assert _group_agg(so, sp, n, calls, ws_bytes, ws, first, ng) == \
        OTBX_ERR_INVALID


def test_group_agg_bad_key_in_later_column_is_rejected(so):
    sp = _spec(nkeys=3)
    sp.key[2].type = 7
    assert _group_agg(so, sp, 10, _calls([_agg(0)])) == OTBX_ERR_INVALID
    sp = _spec(nkeys=3)
    sp.key[1].col = None
    assert _group_agg(so, sp, 10, _calls([_agg(0)])) == OTBX_ERR_INVALID


# ---- merge_group_partials over gloo, world size 2 ----

def _rank_partial(rank):
    """rank 0 holds keys [1, 5], rank 1 keys [1, 3, 5]: key 3 is on one rank
    only. Float MAX of key 1 ties -0.0 (rank 0) with +0.0 (rank 1); the
    int128 sum of key 1 carries across the low word."""
    if rank == 0:
        keys = [np.array([1, 5], dtype=np.int64)]
        aggs = [
            ("count_star", np.array([10, 2], dtype=np.int64), None),
            ("sum", np.array([1.5, 0.0]), np.array([0, 1], dtype=np.uint8)),
            ("sum128", np.array([2**64 - 1, 7], dtype=np.uint64),
             np.array([0, 0], dtype=np.int64),
             np.array([0, 0], dtype=np.uint8)),
            ("max", np.array([-0.0, 4.0]), np.array([0, 0], dtype=np.uint8)),
            ("min", np.array([3, 0], dtype=np.int32),
             np.array([0, 1], dtype=np.uint8)),
        ]
    else:
        keys = [np.array([1, 3, 5], dtype=np.int64)]
        aggs = [
            ("count_star", np.array([20, 1, 3], dtype=np.int64), None),
            ("sum", np.array([2.25, 8.0, 0.0]),
             np.array([0, 0, 1], dtype=np.uint8)),
            ("sum128", np.array([2, 5, 2**64 - 9], dtype=np.uint64),
             np.array([0, 0, -1], dtype=np.int64),
             np.array([0, 0, 0], dtype=np.uint8)),
            ("max", np.array([0.0, 1.0, np.nan]),
             np.array([0, 0, 0], dtype=np.uint8)),
            ("min", np.array([-4, 9, 0], dtype=np.int32),
             np.array([0, 0, 1], dtype=np.uint8)),
        ]
    return keys, aggs


def _worker_group(rank, world, port, q):
    from opentenbase_amd import fragment
    _init(rank, world, port)
    keys, aggs = _rank_partial(rank)
    out = fragment.merge_group_partials(keys, aggs)
    if rank == 0:
        q.put(out)
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_merge_group_partials_two_ranks():
    keys, knulls, aggs = _run(_worker_group)
    assert keys[0].tolist() == [1, 3, 5] and knulls == [None]
    assert aggs[0][0].tolist() == [30, 1, 5]
    assert aggs[1][0].tolist() == [3.75, 8.0, 0.0]
    assert aggs[1][1].tolist() == [0, 0, 1]          # key 5: NULL on both
    # int128: (2^64 - 1) + 2 carries; 7 + (-9) = -2
    assert ex.int128_sums(aggs[2][0], aggs[2][1], aggs[2][2]) == \
        [2**64 + 1, 5, -2]
    # float MAX: -0.0 (rank 0) ties +0.0 (rank 1): the later rank wins
    assert _bits(aggs[3][0]) == _bits([0.0, 1.0, np.nan])
    assert aggs[4][0].tolist() == [-4, 9, 0] and \
        aggs[4][1].tolist() == [0, 0, 1]
    assert aggs[4][0].dtype == np.int32


def test_merge_group_partials_single_process_is_identity():
    from opentenbase_amd import fragment
    keys, aggs = _rank_partial(0)
    k2, n2, a2 = fragment.merge_group_partials(keys, aggs)
    assert k2 is keys and a2 is aggs and n2 == [None]


def test_merge_group_partials_combine_rules():
    """the combine itself, on a hand-made 'gathered' stream in rank order"""
    from opentenbase_amd import fragment
    k0, a0 = _rank_partial(0)
    k1, a1 = _rank_partial(1)
    keys = [np.concatenate([k0[0], k1[0]])]
    aggs = []
    for x, y in zip(a0, a1):
        aggs.append((x[0],) + tuple(
            None if p is None else np.concatenate([p, q])
            for p, q in zip(x[1:], y[1:])))
    k, kn, out = fragment.combine_group_partials(keys, [None], [0], aggs)
    assert k[0].tolist() == [1, 3, 5]
    assert _bits(out[3][0]) == _bits([0.0, 1.0, np.nan])
    # reversed rank order: now -0.0 is the later one
    rev = [np.concatenate([k1[0], k0[0]])]
    aggs_r = []
    for x, y in zip(a1, a0):
        aggs_r.append((x[0],) + tuple(
            None if p is None else np.concatenate([p, q])
            for p, q in zip(x[1:], y[1:])))
    k, kn, out = fragment.combine_group_partials(rev, [None], [0], aggs_r)
    assert _bits(out[3][0]) == _bits([-0.0, 1.0, np.nan])
    assert ex.int128_sums(out[2][0], out[2][1], out[2][2]) == \
        [2**64 + 1, 5, -2]

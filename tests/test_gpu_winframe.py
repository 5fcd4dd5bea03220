"""GPU tests of otbx_window_frame / GpuWindowFrame: every function over ROWS
and RANGE frames against winframe_ref. Integer outputs and everything except
tree-path float sums are compared bit for bit."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd._lib import SortSpecDev, WinCallDev
from winframe_ref import (frame_terms, golden_inputs, golden_load,
                          golden_rows, loop_frame, ref_frame)

pytestmark = pytest.mark.gpu

T = 4096                 # otbx_window.hip: positions per block tile
WF_MID_THREADS = 512     # tile aggregates per pass of the tile-aggregate scan
GUARD = 64
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
_SORT_TYPE = {np.dtype(np.int64): 0, np.dtype(np.float64): 1,
              np.dtype(np.int32): 2, np.dtype(np.uint8): 3}
DTYPES = (np.int64, np.float64, np.int32, np.uint8)


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def D(ex):
    return ex.window_frame_direct_default()


def dev(a):
    return None if a is None else \
        torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_frame(ex, frame):
    units, start, end = frame
    return (ex.rows_between if units == "rows" else ex.range_between)(start,
                                                                      end)


def _out_dtypes(call):
    """numpy dtypes of (out, out_hi or None, out_null or None)"""
    func = call[0]
    if func == "ntile":
        return np.int32, None, None
    if func in ("count_star", "count"):
        return np.int64, None, None
    dt = np.asarray(call[1]).dtype
    if func == "sum":
        if dt == np.int64:
            return np.uint64, np.int64, np.uint8
        return (np.float64 if dt == np.float64 else np.int64), None, np.uint8
    return dt, None, np.uint8


def raw_frame(ex, spec, npart, n, frame, calls, perm):
    """otbx_window_frame itself on an explicit permutation. Every output
    buffer is pre-filled with a sentinel and carries GUARD extra entries that
    must come back untouched, and the inputs must come back unchanged.
    Returns the calls' results in winframe_ref's tuple format."""
    keep, inputs = [], []

    def up(a):
        t = dev(a)
        if t is not None:
            keep.append(t)
            inputs.append((t, np.ascontiguousarray(a).copy()))
        return t

    sp = SortSpecDev()
    sp.nkeys = len(spec)
    for c, (col, nulls, desc, nf) in enumerate(spec):
        col = np.ascontiguousarray(col)
        tc, tn = up(col), up(nulls)
        sp.key[c].col = tc.data_ptr()
        sp.key[c].nulls = tn.data_ptr() if tn is not None else None
        sp.key[c].type = _SORT_TYPE[col.dtype]
        sp.key[c].flags = (1 if desc else 0) | (2 if nf else 0)
    arr = (WinCallDev * 8)()
    bufs = []
    for i, call in enumerate(calls):
        func = call[0]
        wc = arr[i]
        wc.func = _lib.WIN_FUNCS[func]
        col = nl = None
        if func == "ntile":
            wc.param = call[1]
        else:
            col = call[1] if len(call) > 1 else None
            nl = call[2] if len(call) > 2 else None
            if func in ("lag", "lead"):
                wc.param = call[3]
                default = call[4]
                wc.def_isnull = 1 if default is None else 0
                if default is not None:
                    if np.asarray(col).dtype == np.float64:
                        wc.def_f = float(default)
                    else:
                        wc.def_i = int(default)
            elif func == "nth_value":
                wc.param = call[3]
        if col is not None:
            col = np.ascontiguousarray(col)
            wc.type = _SORT_TYPE[col.dtype]
            wc.col = up(col).data_ptr() if n else 0x1000
        tn = up(nl)
        wc.nulls = tn.data_ptr() if tn is not None and n else None
        ob = []
        for dt, field in zip(_out_dtypes(call), ("out", "out_hi",
                                                 "out_null")):
            if dt is None:
                ob.append(None)
                continue
            t = dev(np.full(n + GUARD, 0x5a, dtype=dt))
            setattr(wc, field, t.data_ptr())
            ob.append(t)
        bufs.append(ob)
    b = C.c_size_t(0)
    assert _lib.lib().otbx_window_frame_workspace_bytes(
        n, len(calls), C.byref(b)) == 0
    ws = torch.empty(max(b.value, 1) + GUARD, dtype=torch.uint8,
                     device="cuda")
    ws[b.value:] = 0x5a
    tp = up(perm)
    fr = make_frame(ex, frame)
    st = _lib.lib().otbx_window_frame(
        C.byref(sp), C.c_int32(npart),
        C.c_void_p(tp.data_ptr()) if tp is not None and n else None,
        C.c_int64(n), C.byref(fr), arr, C.c_int32(len(calls)),
        C.c_void_p(ws.data_ptr()), C.c_size_t(b.value),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    assert bool((ws[b.value:] == 0x5a).all()), "workspace overrun"
    for t, a in inputs:
        assert t.cpu().numpy().tobytes() == a.tobytes(), "an input changed"
    res = []
    for ob in bufs:
        tup = []
        for t in ob:
            if t is None:
                continue
            a = t.cpu().numpy()
            assert (a[n:] == np.full(1, 0x5a, dtype=a.dtype)).all(), \
                "written past n"
            tup.append(a[:n])
        res.append(tuple(tup) if len(tup) > 1 else (tup[0], None))
    return res


def assert_calls(got, exp, calls, skip=()):
    assert len(got) == len(exp) == len(calls)
    for i, (g, e) in enumerate(zip(got, exp)):
        if i in skip:
            continue
        assert len(g) == len(e), (i, calls[i][0])
        for u, v in zip(g, e):
            if u is None or v is None:
                assert u is None and v is None, (i, calls[i][0])
                continue
            assert u.dtype == v.dtype, (i, calls[i][0], u.dtype, v.dtype)
            if u.tobytes() != v.tobytes():
                bad = np.flatnonzero(u.view(np.uint8).reshape(len(u), -1) !=
                                     v.view(np.uint8).reshape(len(v), -1))
                j = int(bad[0]) // u.dtype.itemsize
                raise AssertionError((i, calls[i][0], "position", j, u[j],
                                      v[j]))


def all_calls(col, nl, default=None, off=1, nb=3, nth=2):
    return [("ntile", nb), ("lag", col, nl, off, default),
            ("lead", col, nl, off, None), ("first_value", col, nl),
            ("last_value", col, nl), ("nth_value", col, nl, nth),
            ("count_star",), ("count", col, nl), ("sum", col, nl),
            ("min", col, nl), ("max", col, nl)]


def check_all(ex, spec, npart, n, frame, calls, skip=()):
    """calls (any number) through the raw entry point, 8 per list, against
    ref_frame; returns (got, exp)"""
    exp = ref_frame(spec, npart, frame, calls, n=n)
    got = []
    for i in range(0, len(calls), 8):
        got += raw_frame(ex, spec, npart, n, frame, calls[i:i + 8],
                         exp["perm"])
    assert_calls(got, exp["calls"], calls, skip)
    return got, exp["calls"]


def keys_for(rng, n, nparts=5, peers=3):
    """(partition key, order key) with random partitions and peer groups"""
    part = np.sort(rng.integers(0, max(nparts, 1), n)).astype(np.int32)
    order = (rng.integers(0, max(n // peers, 1), n)).astype(np.int64)
    return [(part, None, False, False), (order, None, False, False)]


def values(rng, dtype, n, p_null=0.25):
    """a column with NULLs and garbage stored under them"""
    if dtype == np.float64:
        v = rng.normal(1e7, 1e6, n)
    elif dtype == np.int64:
        v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    elif dtype == np.int32:
        v = rng.integers(-2**31, 2**31, n).astype(np.int32)
    else:
        v = rng.integers(0, 256, n).astype(np.uint8)
    nl = (rng.random(n) < p_null).astype(np.uint8)
    v = v.copy()
    v[nl == 1] = np.array(77).astype(dtype) if dtype != np.float64 else np.nan
    return v, nl


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ex, n):
    rng = np.random.default_rng(100 + n)
    spec = keys_for(rng, n, nparts=4)
    fcol, fnl = values(rng, np.float64, n)
    icol, inl = values(rng, np.int64, n)
    calls = all_calls(fcol, fnl, default=-1.5) + \
        all_calls(icol, inl, default=9, off=2, nb=4, nth=3)[1:]
    check_all(ex, spec, 1, n, ("rows", -2, 2), calls)


STARTS = [None, 0, -1, -65, 1]
ENDS = [None, 0, -1, 1, 65]
SHAPES = [("rows", s, e) for s in STARTS for e in ENDS] + \
    [("range", s, e) for s in (None, 0) for e in (None, 0)] + \
    [("rows", 0, -1), ("rows", -2, -1), ("rows", 1, None), ("rows", 1, 3),
     ("rows", -2**62, 2**62), ("rows", 2**62, None), ("rows", None, -2**62),
     ("rows", INT64_MIN, INT64_MAX), ("rows", INT64_MAX, INT64_MAX),
     ("rows", INT64_MIN, INT64_MIN), ("rows", INT64_MIN, 0),
     ("rows", 0, INT64_MAX), ("rows", 2**62, -2**62)]


@pytest.mark.parametrize("frame", SHAPES, ids=lambda f: f"{f[0]}_{f[1]}_{f[2]}")
def test_frame_shapes(ex, frame):
    """Partitions of 1..200 rows (most narrower than the 131-wide frame),
    peer groups of ~3. Integer-valued doubles: every sum order is exact."""
    rng = np.random.default_rng(7)
    sizes = [1, 1, 2, 3, 40, 64, 65, 130, 131, 200, 1, 70]
    n = sum(sizes)
    part = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    order = (np.arange(n) // 3).astype(np.int64)
    spec = [(part, None, False, False), (order, None, False, False)]
    fcol = rng.integers(-1000, 1001, n).astype(np.float64)
    fnl = (rng.random(n) < 0.25).astype(np.uint8)
    fcol[fnl == 1] = np.nan
    icol, inl = values(rng, np.int64, n)
    calls = all_calls(fcol, fnl) + all_calls(icol, inl)[3:]
    check_all(ex, spec, 1, n, frame, calls)


def _edge_spec(n):
    """partitions start at T-1, T, T+1 and 2T+5; peer groups also at 2T-1,
    2T and 2T+1"""
    pos = np.arange(n)
    part = np.searchsorted([T - 1, T, T + 1, 2 * T + 5], pos,
                           side="right").astype(np.uint8)
    order = np.searchsorted([2 * T - 1, 2 * T, 2 * T + 1, 3 * T], pos,
                            side="right").astype(np.int32)
    return [(part, None, False, False), (order, None, False, False)]


@pytest.mark.parametrize("w", [T - 1, T, T + 1, 2 * T + 3, 3 * T + 100])
@pytest.mark.parametrize("place", ["trailing", "centred", "leading"])
def test_tile_edges_bounded(ex, w, place):
    n = 3 * T + 17
    rng = np.random.default_rng(w)
    spec = _edge_spec(n)
    # one long partition too: npart = 0 makes the whole input one partition
    frame = {"trailing": ("rows", -(w - 1), 0),
             "centred": ("rows", -(w // 2), w - w // 2 - 1),
             "leading": ("rows", 0, w - 1)}[place]
    icol, inl = values(rng, np.int64, n)
    fcol = rng.integers(-1000, 1001, n).astype(np.float64)
    calls = [("sum", icol, inl), ("min", fcol, inl), ("max", icol, inl),
             ("count", icol, inl), ("first_value", icol, inl),
             ("last_value", fcol, None), ("nth_value", icol, inl, w),
             ("count_star",)]
    for npart in (1, 0):
        check_all(ex, spec, npart, n, frame, calls)


@pytest.mark.parametrize("frame", [("rows", None, 0), ("rows", 0, None),
                                   ("rows", None, 5), ("rows", -5, None),
                                   ("range", None, 0), ("range", 0, None),
                                   ("range", 0, 0), ("range", None, None)],
                         ids=lambda f: f"{f[0]}_{f[1]}_{f[2]}")
def test_tile_edges_unbounded(ex, frame):
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    spec = _edge_spec(n)
    icol, inl = values(rng, np.int64, n)
    fcol = rng.integers(-1000, 1001, n).astype(np.float64)
    calls = [("sum", icol, inl), ("sum", fcol, inl), ("min", fcol, inl),
             ("max", icol, inl), ("count", icol, inl),
             ("first_value", icol, inl), ("last_value", fcol, None),
             ("count_star",)]
    check_all(ex, spec, 1, n, frame, calls)


def test_both_bounded_paths_on_one_input(ex, D, monkeypatch):
    """The per-row loop and the two scans on the same input: forced by
    OTBX_WIN_FRAME_DIRECT = 4097 / 0, each against the reference and against
    each other; then the widths around the default cut-over with the
    variable unset."""
    n = T + 300
    rng = np.random.default_rng(23)
    spec = keys_for(rng, n, nparts=3)
    icol, inl = values(rng, np.int64, n)
    i32, i32nl = values(rng, np.int32, n)
    fcol = rng.integers(-1000, 1001, n).astype(np.float64)
    calls = [("min", fcol, inl), ("max", fcol, inl), ("min", icol, inl),
             ("max", i32, i32nl), ("count", icol, inl), ("sum", icol, inl),
             ("sum", i32, i32nl), ("sum", fcol, inl)]
    for w in (1, 7, 64, T, T + 1):
        frame = ("rows", -(w // 2), w - w // 2 - 1)
        monkeypatch.setenv("OTBX_WIN_FRAME_DIRECT", "0")
        scans, _ = check_all(ex, spec, 1, n, frame, calls)
        monkeypatch.setenv("OTBX_WIN_FRAME_DIRECT", "4097")
        loop, _ = check_all(ex, spec, 1, n, frame, calls)
        assert_calls(scans, loop, calls)
    monkeypatch.delenv("OTBX_WIN_FRAME_DIRECT")
    for w in (D - 1, D, D + 1):
        check_all(ex, spec, 1, n, ("rows", -(w - 1), 0), calls)
        check_all(ex, spec, 1, n, ("rows", 1, w), calls)


def _float_specials(rng, n):
    bits = np.array([0x7ff8000000000000, 0xfff8000000000000,
                     0x7ff8000000000123, 0xfff80000000abcde,
                     0x0000000000000000, 0x8000000000000000,
                     0x7ff0000000000000, 0xfff0000000000000,
                     0x3ff0000000000000, 0xbff0000000000000,
                     0x4000000000000000], dtype=np.uint64)
    return bits[rng.integers(0, len(bits), n)].view(np.float64)


@pytest.mark.parametrize("dtype,mask", list(itertools.product(
    DTYPES, (False, True))), ids=lambda x: getattr(x, "__name__", str(x)))
@pytest.mark.parametrize("frame", [("rows", -3, 1), ("rows", -100, 100),
                                   ("range", None, 0)],
                         ids=["direct", "scans", "default"])
def test_types_and_masks(ex, dtype, mask, frame):
    n = 1500
    rng = np.random.default_rng(31)
    spec = keys_for(rng, n, nparts=6)
    col, nl = values(rng, dtype, n)
    if dtype == np.float64:
        # NaN payloads, signed zeros and infinities for everything that
        # returns a row's bits; the sum takes finite integer-valued doubles
        spec_col = _float_specials(rng, n)
        sum_col = rng.integers(-1000, 1001, n).astype(np.float64)
        sum_col[nl == 1] = np.inf            # garbage under NULL
    else:
        spec_col = sum_col = col
    if not mask:
        nl = None
        if dtype == np.float64:
            sum_col = rng.integers(-1000, 1001, n).astype(np.float64)
    default = -2.5 if dtype == np.float64 else (200 if dtype == np.uint8
                                                else -3)
    calls = all_calls(spec_col, nl, default=default)
    calls[8] = ("sum", sum_col, nl)
    check_all(ex, spec, 1, n, frame, calls)


@pytest.mark.parametrize("frame", [("rows", -3, 0), ("rows", -200, 0),
                                   ("rows", None, 0), ("rows", 0, None),
                                   ("range", None, None)],
                         ids=lambda f: f"{f[0]}_{f[1]}_{f[2]}")
def test_sum_i64_moves_the_high_word(ex, frame):
    n = T + 50
    rng = np.random.default_rng(37)
    spec = keys_for(rng, n, nparts=3)
    col = rng.choice(np.array([INT64_MAX, INT64_MAX - 1, INT64_MIN,
                               INT64_MIN + 1, -1, 0, 1, 2**62, -2**62],
                              dtype=np.int64), n)
    nl = (rng.random(n) < 0.1).astype(np.uint8)
    got, exp = check_all(ex, spec, 1, n, frame, [("sum", col, nl)])
    assert np.abs(got[0][1]).max() > 1        # the high word really moves


def test_float_sum_direct_path_is_bit_equal_to_the_row_loop(ex, D):
    """general normals at mean 1e7: every addition rounds, so the result
    depends on the order — left to right, as the reference re-aggregates"""
    n = 700
    rng = np.random.default_rng(43)
    spec = keys_for(rng, n, nparts=4)
    col = rng.normal(1e7, 1e6, n)
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    for frame in (("rows", -6, 0), ("rows", -(D - 1), 0), ("rows", 1, D),
                  ("rows", -2, 2), ("rows", 0, 0)):
        calls = [("sum", col, nl), ("sum", col, None)]
        exp = loop_frame(spec, 1, frame, calls, n=n)
        got = raw_frame(ex, spec, 1, n, frame, calls, exp["perm"])
        assert_calls(got, exp["calls"], calls)


@pytest.mark.parametrize("frame", [("rows", None, 0), ("rows", 0, None),
                                   ("rows", -100, 100), ("rows", -T, 0),
                                   ("range", 0, 0), ("range", None, None)],
                         ids=lambda f: f"{f[0]}_{f[1]}_{f[2]}")
@pytest.mark.parametrize("dist", ["n01", "n1e7"])
def test_float_sum_tree_paths_within_summation_bound(ex, frame, dist):
    """|got - fsum(terms)| <= m*u*sum|x| / (1 - m*u), u = 2^-53, with m the
    frame's non-NULL terms - 1 (>= 1 so that the rounding of the exact sum is
    covered): the bound of recursive summation in any order — derived, not
    measured. Small partitions in full, a stride and all tile-edge rows of
    the long ones. The same call twice gives the same bits."""
    rng = np.random.default_rng(47)
    sizes = [40, 7000, 64, 3, 5000, 17]
    n = sum(sizes)
    loc, scale = {"n01": (0, 1), "n1e7": (1e7, 1e6)}[dist]
    col = rng.normal(loc, scale, n)
    nl = (rng.random(n) < 0.1).astype(np.uint8)
    part = np.repeat(np.arange(len(sizes), dtype=np.uint8), sizes)
    order = (np.arange(n, dtype=np.int64) // 3)
    spec = [(part, None, False, False), (order, None, False, False)]
    calls = [("sum", col, nl), ("count", col, nl)]
    exp = ref_frame(spec, 1, frame, [calls[1]], n=n)
    got = raw_frame(ex, spec, 1, n, frame, calls, exp["perm"])
    again = raw_frame(ex, spec, 1, n, frame, calls, exp["perm"])
    assert_calls(got, again, calls)
    assert np.array_equal(got[1][0], exp["calls"][0][0])
    lo, hi, v, nn = frame_terms(spec, 1, frame, col, nl)
    pos = np.arange(n)
    psize = np.repeat(sizes, sizes)
    rows = np.flatnonzero((psize <= 64) | np.isin(pos % T, (0, 1, T - 2,
                                                           T - 1)) |
                          (pos % 53 == 0))
    u = 2.0 ** -53
    worst = 0.0
    for j in rows.tolist():
        terms = v[lo[j]:hi[j] + 1][nn[lo[j]:hi[j] + 1]] if lo[j] <= hi[j] \
            else v[:0]
        assert len(terms) == got[1][0][j]
        if len(terms) == 0:
            assert got[0][1][j] == 1 and got[0][0][j] == 0.0
            continue
        assert got[0][1][j] == 0
        m = max(len(terms) - 1, 1)
        bound = m * u * math.fsum(np.abs(terms)) / (1.0 - m * u)
        err = abs(got[0][0][j] - math.fsum(terms))
        worst = max(worst, err / bound)
        assert err <= bound, (j, m, err, bound)
    print(f"{frame} {dist}: {len(rows)} rows, worst err/bound = {worst:.4f}")


@pytest.mark.parametrize("frame", [("rows", -1, 0), ("rows", -40, 0),
                                   ("rows", -300, 0), ("rows", None, 0),
                                   ("rows", 0, None), ("range", 0, 0)],
                         ids=lambda f: f"{f[0]}_{f[1]}_{f[2]}")
def test_float_sum_inf_nan_do_not_leak(ex, frame):
    """Inf, -Inf and NaN in one partition and in single frames of another:
    every frame without one of them is finite and exact (integer-valued
    doubles), every frame with one is non-finite"""
    rng = np.random.default_rng(53)
    sizes = [300, 5, T + 9, 300]
    n = sum(sizes)
    part = np.repeat(np.arange(len(sizes), dtype=np.uint8), sizes)
    order = (np.arange(n, dtype=np.int64) // 2)
    spec = [(part, None, False, False), (order, None, False, False)]
    col = rng.integers(-1000, 1001, n).astype(np.float64)
    col[300:305] = [np.inf, -np.inf, np.nan, np.inf, 1.0]
    col[305 + 100] = np.inf
    col[305 + T] = np.nan
    calls = [("sum", col, None)]
    exp = ref_frame(spec, 1, frame, calls, n=n)
    got = raw_frame(ex, spec, 1, n, frame, calls, exp["perm"])
    lo, hi, v, nn = frame_terms(spec, 1, frame, col)
    bad = np.concatenate([[0], np.cumsum(~np.isfinite(v))])
    tainted = (bad[np.clip(hi, 0, n - 1) + 1] - bad[np.clip(lo, 0, n - 1)]
               > 0) & (lo <= hi)
    g, e = got[0][0], exp["calls"][0][0]
    assert np.array_equal(got[0][1], exp["calls"][0][1])
    assert np.isfinite(g[~tainted]).all() and not np.isfinite(g[tainted]).any()
    assert g[~tainted].tobytes() == e[~tainted].tobytes()
    assert np.array_equal(np.isnan(g), np.isnan(e))
    assert tainted.any() and (~tainted).sum() > 500


@pytest.mark.parametrize("off", [0, 1, 64, T, 2 * T, -1, -64, -T])
def test_lag_lead_offsets_and_defaults(ex, off):
    n = T + 70
    rng = np.random.default_rng(59)
    sizes = [1, 2, 64, 65, T - 200, 138]
    assert sum(sizes) == n
    part = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    spec = [(part, None, False, False)]
    calls = []
    for dtype, default in ((np.int64, -2**40), (np.float64, -0.0),
                           (np.int32, -7), (np.uint8, 255)):
        col, nl = values(rng, dtype, n)
        calls += [("lag", col, nl, off, default), ("lead", col, nl, off, None)]
    got, exp = check_all(ex, spec, 1, n, ("range", None, 0), calls)
    calls = [("lag", calls[0][1], None, off, None),
             ("lead", calls[2][1], calls[2][2], off, 1.5)]
    got, exp = check_all(ex, spec, 1, n, ("rows", 0, 0), calls)
    if off == 1:
        # a NULL source row and a source row outside the partition are told
        # apart: the first is NULL whatever the default, the second is the
        # default
        col = np.arange(6, dtype=np.int64)
        nl = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)
        p = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
        r = raw_frame(ex, [(p, None, False, False)], 1, 6, ("rows", 0, 0),
                      [("lag", col, nl, 1, 99)], np.arange(6))[0]
        assert r[0].tolist() == [99, 0, 0, 99, 3, 0]
        assert r[1].tolist() == [0, 0, 1, 0, 0, 1]


def test_ntile_buckets(ex):
    sizes = [1, 2, 10, T + 1]
    n = sum(sizes)
    part = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    spec = [(part, None, False, False)]
    buckets = [1, 2, 3, 7, 9, 10, 11, T, T + 1, T + 2, 2**31 - 1]
    calls = [("ntile", b) for b in buckets]
    got, _ = check_all(ex, spec, 1, n, ("rows", 0, 0), calls)
    exp = loop_frame(spec, 1, ("rows", 0, 0), calls, n=n)
    assert_calls(got, exp["calls"], calls)
    assert got[3][0][-1] == 7 and got[0][0].max() == 1


def test_single_call_equals_the_call_in_a_full_list(ex):
    n = 2 * T + 77
    rng = np.random.default_rng(61)
    spec = keys_for(rng, n, nparts=4)
    col, nl = values(rng, np.int64, n)
    fcol = rng.integers(-1000, 1001, n).astype(np.float64)
    calls = [("ntile", 5), ("lag", col, nl, 3, 4), ("nth_value", fcol, nl, 3),
             ("count", col, nl), ("sum", col, nl), ("sum", fcol, nl),
             ("min", fcol, nl), ("max", col, nl)]
    for frame in (("rows", -3, 3), ("rows", -300, 300), ("range", None, 0)):
        exp = ref_frame(spec, 1, frame, calls, n=n)
        full = raw_frame(ex, spec, 1, n, frame, calls, exp["perm"])
        assert_calls(full, exp["calls"], calls)
        for i, c in enumerate(calls):
            one = raw_frame(ex, spec, 1, n, frame, [c], exp["perm"])
            assert_calls(one, [full[i]], [c])


def test_tile_aggregate_scan_spanning_several_chunks(ex):
    """12.6 M rows = 3,078 tiles: more than the tile aggregates one pass of
    the tile-aggregate scan holds, so the running carry crosses passes, for
    the forward and the backward scan. Integer-valued, compared on the
    device."""
    n = 3 * 1024 * T + 5 * T + 13
    assert -(-n // T) > 3 * WF_MID_THREADS
    rng = np.random.default_rng(67)
    k = rng.integers(0, 3, n, dtype=np.uint8)
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    ivals = rng.integers(-2**40, 2**40, n).astype(np.int64)
    perm = np.argsort(k, kind="stable")
    cnt = np.bincount(k, minlength=3).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    ks = k[perm]
    ps = start[ks]
    pe = ps + cnt[ks] - 1

    def run(frame, calls):
        node = ex.GpuWindowFrame([dev(k)], [], frame=frame, calls=calls)
        node.BeginCustomScan()
        got = node.ExecCustomScan()
        node.EndCustomScan()
        assert torch.equal(got["perm"], torch.from_numpy(perm).cuda())
        return got["calls"]

    sv = vals[perm]
    cs = np.concatenate([[0.0], np.cumsum(sv)])          # exact: integers
    got = run(ex.rows_between(None, 0), [("sum", dev(vals))])
    pos = np.arange(n)
    assert torch.equal(got[0][0], torch.from_numpy(cs[pos + 1] - cs[ps])
                       .cuda())
    got = run(ex.rows_between(0, None), [("sum", dev(vals)),
                                         ("count", dev(vals))])
    assert torch.equal(got[0][0], torch.from_numpy(cs[pe + 1] - cs[pos])
                       .cuda())
    assert torch.equal(got[1][0], torch.from_numpy(pe - pos + 1).cuda())
    assert int(got[0][1].sum().item()) == 0
    # bounded and wider than a tile: both scans and the block decomposition
    w = 2 * T + 3
    lo = np.maximum(ps, pos - (w - 1))
    ics = np.concatenate([[0], np.cumsum(ivals[perm])])  # int64, no overflow
    got = run(ex.rows_between(-(w - 1), 0), [("sum", dev(ivals))])
    assert torch.equal(got[0][0], torch.from_numpy(ics[pos + 1] - ics[lo])
                       .cuda())
    assert torch.equal(got[0][1], torch.from_numpy(
        (ics[pos + 1] - ics[lo]) >> 63).cuda())


def node_frame(ex, spec, npart, frame, calls, n=None):
    part, order = spec[:npart], spec[npart:]
    dcalls = []
    for c in calls:
        if c[0] == "ntile":
            dcalls.append(c)
        else:
            dcalls.append((c[0],) + tuple(
                dev(x) if isinstance(x, np.ndarray) else x for x in c[1:]))
    node = ex.GpuWindowFrame(
        [dev(c) for c, _, _, _ in part], [dev(c) for c, _, _, _ in order],
        descending=[d for _, _, d, _ in order],
        nulls_first=[f for _, _, _, f in order],
        part_nulls=[dev(m) for _, m, _, _ in part],
        order_nulls=[dev(m) for _, m, _, _ in order],
        frame=make_frame(ex, frame), calls=dcalls, n=n)
    node.BeginCustomScan()
    row = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    node.ReScanCustomScan()
    again = node.ExecCustomScan()
    node.EndCustomScan()
    for a, b in zip(row["calls"], again["calls"]):
        for u, v in zip(a, b):
            assert (u is None and v is None) or torch.equal(u, v)
    assert set(node.explain()) == {"sort", "window_frame"}
    calls_np = [tuple(None if t is None else t.cpu().numpy() for t in r)
                for r in row["calls"]]
    # an int64 SUM's low word is an int64 tensor holding the unsigned word
    calls_np = [(r[0].view(np.uint64),) + r[1:] if len(r) == 3 else r
                for r in calls_np]
    return row, row["perm"].cpu().numpy(), calls_np


def test_golden_cases_through_the_node(ex):
    gold = golden_load()
    for case in gold["cases"]:
        cols, spec, npart, frame, calls = golden_inputs(gold, case)
        _, perm, res = node_frame(ex, spec, npart, frame, calls, n=10)
        got, want = golden_rows(case, cols, perm, res)
        assert got == want, case["name"]


def test_node_sorts_and_names_its_results(ex):
    n = 3000
    rng = np.random.default_rng(71)
    part = rng.integers(0, 7, n).astype(np.int32)
    pn = (rng.random(n) < 0.1).astype(np.uint8)
    order = rng.normal(0, 1, n).round(1)
    spec = [(part, pn, False, False), (order, None, True, True)]
    col, nl = values(rng, np.int64, n)
    calls = [("lag", col, nl, 1, 5), ("ntile", 4), ("sum", col, nl),
             ("lead", col, nl, 2, None), ("count_star",)]
    for frame in (("rows", -6, 0), ("range", None, 0)):
        row, perm, res = node_frame(ex, spec, 1, frame, calls)
        exp = ref_frame(spec, 1, frame, calls)
        assert np.array_equal(perm, exp["perm"])
        assert_calls(res, exp["calls"], calls)
        assert torch.equal(row["sum"][0], row["calls"][2][0])
        assert len(row["sum"]) == 3 and row["ntile"][1] is None
        assert set(row) == {"calls", "perm", "lag", "ntile", "sum", "lead",
                            "count_star"}
        sums = ex.int128_sums(*row["sum"])
        e = ex.int128_sums(*exp["calls"][2])
        assert sums == e
    # no keys: the sort is skipped and the input order is the window order
    row, perm, res = node_frame(ex, [], 0, ("rows", -1, 1),
                                [("sum", col, nl), ("max", col, nl)])
    assert np.array_equal(perm, np.arange(n))
    assert_calls(res, ref_frame([], 0, ("rows", -1, 1),
                                [("sum", col, nl), ("max", col, nl)])["calls"],
                 calls[:2])


def test_end_to_end_filter_window_gather_moving_average(ex):
    """WHERE qty > 10, then per store the 7-row moving average of price in
    day order — avg = sum / count over ROWS 6 PRECEDING .. CURRENT ROW — and
    the day column gathered into output order"""
    n = 20000
    rng = np.random.default_rng(73)
    store = rng.integers(0, 9, n).astype(np.int32)
    day = rng.permutation(n).astype(np.int64)
    qty = rng.integers(0, 50, n).astype(np.int64)
    price = rng.integers(1, 100000, n).astype(np.float64) / 4.0
    pnl = (rng.random(n) < 0.15).astype(np.uint8)
    flt = ex.GpuFilter([[ex.qual_term(dev(qty), ">", 10)]])
    flt.BeginCustomScan()
    sel = flt.ExecCustomScan()
    flt.EndCustomScan()
    cols = [flt.gather(dev(c)) for c in (store, day, price, pnl)]
    node = ex.GpuWindowFrame([cols[0]], [cols[1]],
                             frame=ex.rows_between(-6, 0),
                             calls=[("sum", cols[2], cols[3]),
                                    ("count", cols[2], cols[3])])
    node.BeginCustomScan()
    row = node.ExecCustomScan()
    node.EndCustomScan()
    days = node.gather(cols[1]).cpu().numpy()
    s, snull = (t.cpu().numpy() for t in row["sum"])
    c = row["count"][0].cpu().numpy()
    avg = ex.avg_f64(s, c)

    keep = np.flatnonzero(qty > 10)
    assert np.array_equal(sel.cpu().numpy(), keep)
    st, dy, pr, nl_ = store[keep], day[keep], price[keep], pnl[keep]
    o = np.lexsort((dy, st))
    assert np.array_equal(days, dy[o])
    st, pr, nl_ = st[o], pr[o], nl_[o]
    m = len(o)
    for j in list(range(0, m, 97)) + [0, m - 1]:
        a = j
        while a > 0 and j - a < 6 and st[a - 1] == st[j]:
            a -= 1
        terms = [pr[q] for q in range(a, j + 1) if not nl_[q]]
        assert c[j] == len(terms)
        if terms:
            acc = terms[0]
            for x in terms[1:]:
                acc += x
            assert s[j] == acc and snull[j] == 0 and avg[j] == acc / len(terms)
        else:
            assert snull[j] == 1 and np.isnan(avg[j])

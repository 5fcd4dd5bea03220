"""GPU parity of the DISTINCT / ordered-set aggregates (otbx_ordered_agg /
GpuOrderedAgg) against tests/ordagg_ref.py. Everything is bit-equal to the
reference except SUM_DISTINCT over F64 on non-integer data, which is held to
the recursive-summation bound m*u*sum|x| / (1 - m*u) (m = summed values - 1)
and to bit equality between two identical calls; where the reference's float
sum is NaN, a NaN is required (the payload of an Inf - Inf is the adder's)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd._lib import OAGG_FUNCS, OAggCallsDev, SortSpecDev
from ordagg_ref import (assert_same, golden_case, golden_check, loop_ordagg,
                        ref_ordagg)
from sort_ref import ref_perm
from test_gpu_groupagg import (dev, keys_from_runs, node_result, random_runs,
                               raw_group_agg, run_node)

pytestmark = pytest.mark.gpu

OA_TILE = 2048          # otbx_ordagg.hip: positions per block tile
OA_FIX_THREADS = 1024   # tile records per pass of the fix-up scan
T, M = OA_TILE, OA_FIX_THREADS
GUARD = 64
U = 2.0 ** -53
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden",
                                     "ordagg_cases.json")))

_SORT_TYPE = {np.dtype(np.int64): 0, np.dtype(np.float64): 1,
              np.dtype(np.int32): 2, np.dtype(np.uint8): 3}
TYPES = {"i64": np.int64, "f64": np.float64, "i32": np.int32, "u8": np.uint8}

# all five functions plus three more percentiles: the eight slots
EIGHT = [("count_distinct",), ("sum_distinct",), ("percentile_disc", 0.5),
         ("percentile_cont", 0.5), ("mode",), ("percentile_disc", 0.0),
         ("percentile_cont", 1.0), ("percentile_cont", 0.37)]


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


def _out_dtype(func, adt):
    if func == "count_distinct":
        return np.int64, False, False
    if func == "sum_distinct":
        if adt == np.float64:
            return np.float64, False, True
        return (np.uint64, True, True) if adt == np.int64 else \
            (np.int64, False, True)
    if func == "percentile_cont":
        return np.float64, False, True
    return adt, False, True


def _sentinel(dt):
    dt = np.dtype(dt)
    if dt == np.uint8:
        return np.uint8(0x5a)
    if dt == np.float64:
        return np.float64(-777.0)
    if dt == np.uint64:
        return np.uint64(0x5a5a5a5a5a5a5a5a)
    return dt.type(-777)


def raw_ordered_agg(spec, ngroup, calls, perm=None, want_first=True):
    """otbx_ordered_agg itself. Every output buffer — requested or not — is
    pre-filled with a sentinel and carries GUARD extra entries: the entries
    past ngroups and the buffers not requested must come back untouched.
    perm: numpy array, device tensor or None (identity). Returns (status,
    result shaped as ordagg_ref's)."""
    n = len(spec[ngroup][0])
    adt = np.asarray(spec[ngroup][0]).dtype
    keep = []
    sp = SortSpecDev()
    sp.nkeys = len(spec)
    for c, (col, nulls, desc, nf) in enumerate(spec):
        col = np.ascontiguousarray(col)
        tc, tn = dev(col), dev(nulls)
        keep += [tc, tn]
        sp.key[c].col = tc.data_ptr() if n else 0x1000
        sp.key[c].nulls = tn.data_ptr() if tn is not None and n else None
        sp.key[c].type = _SORT_TYPE[col.dtype]
        sp.key[c].flags = (1 if desc else 0) | (2 if nf else 0)
    cs = OAggCallsDev()
    cs.ncalls = len(calls)
    bufs = []
    for i, c in enumerate(calls):
        dt, has_hi, has_null = _out_dtype(c[0], adt)
        oc = cs.call[i]
        oc.func = OAGG_FUNCS[c[0]]
        oc.fraction = c[1] if len(c) > 1 else float("nan")   # ignored there
        b = {"val": dev(np.full(n + GUARD, _sentinel(dt), dtype=dt)
                        .view(np.int64 if dt == np.uint64 else dt)),
             "hi": dev(np.full(n + GUARD, -777, dtype=np.int64)),
             "null": dev(np.full(n + GUARD, 0x5a, dtype=np.uint8)),
             "dt": dt, "has_hi": has_hi, "has_null": has_null}
        oc.out = b["val"].data_ptr()
        if has_hi:
            oc.out_hi = b["hi"].data_ptr()
        if has_null:
            oc.out_null = b["null"].data_ptr()
        bufs.append(b)
    first = dev(np.full(n + GUARD, -777, dtype=np.int64))
    ng = dev(np.array([-777], dtype=np.int64))
    wsb = C.c_size_t(0)
    assert _lib.lib().otbx_ordered_agg_workspace_bytes(
        n, len(calls), C.byref(wsb)) == 0
    ws = torch.empty(max(wsb.value, 16), dtype=torch.uint8, device="cuda")
    tp = perm if isinstance(perm, torch.Tensor) else dev(perm)
    st = _lib.lib().otbx_ordered_agg(
        C.byref(sp), C.c_int32(ngroup),
        C.c_void_p(tp.data_ptr()) if tp is not None and n else None,
        C.c_int64(n), C.byref(cs), C.c_void_p(ws.data_ptr()),
        C.c_size_t(wsb.value),
        C.c_void_p(first.data_ptr()) if want_first else None,
        C.c_void_p(ng.data_ptr()),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if st != 0:
        return st, None
    ngroups = int(ng.cpu().item())
    assert 0 <= ngroups <= max(n, 1)

    def cut(t, dt, requested, what):
        a = t.cpu().numpy()
        if dt == np.uint64:
            a = a.view(np.uint64)
        sent = _sentinel(a.dtype)
        if not requested:
            assert (a == sent).all(), f"{what}: not requested but written"
            return None
        assert (a[ngroups:] == sent).all(), f"{what}: written past ngroups"
        return a[:ngroups]

    res = {"ngroups": ngroups, "aggs": [],
           "first_row": cut(first, np.int64, want_first, "first_row")}
    for i, b in enumerate(bufs):
        r = {"val": cut(b["val"], b["dt"], True, f"call {i} out"),
             "null": cut(b["null"], np.uint8, b["has_null"],
                         f"call {i} out_null")}
        hi = cut(b["hi"], np.int64, b["has_hi"], f"call {i} out_hi")
        if hi is not None:
            r["hi"] = hi
        res["aggs"].append(r)
    return 0, res


def check(got, exp, calls, approx=False):
    """bit-equality with the reference. Where arithmetic made a NaN in the
    reference (a float sum, or percentile_cont's interpolation), a NaN is
    required, whatever its payload; with approx the float sums are held to
    the bound instead. Returns the worst observed fraction of the bound."""
    worst = 0.0
    g2 = dict(got, aggs=list(got["aggs"]))
    for i, y in enumerate(exp["aggs"]):
        if "abs" not in y and calls[i][0] != "percentile_cont":
            continue
        x = got["aggs"][i]
        assert np.array_equal(x["null"], y["null"])
        nan = np.isnan(y["val"])
        assert np.array_equal(np.isnan(x["val"]), nan), i
        val = np.where(nan, y["val"], x["val"])
        if approx and "abs" in y:
            m = np.maximum(y["rows"] - 1, 0).astype(np.float64)
            ok = ~nan & np.isfinite(y["abs"])
            bound = m * U * np.where(ok, y["abs"], 0.0) / (1.0 - m * U)
            err = np.where(ok, np.abs(x["val"] - y["val"]), 0.0)
            assert (err <= bound).all(), (i, err.max())
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
            val = np.where(ok, y["val"], val)
        g2["aggs"][i] = dict(x, val=val)
    if g2["first_row"] is None:
        g2 = dict(g2, first_row=exp["first_row"])
    assert_same(g2, exp)
    return worst


def arg_col(rng, t, n, distinct=12):
    """an argument column with heavy duplication; floats integer-valued (every
    summation order exact) with ±0"""
    dt = TYPES[t]
    if t == "i64":
        return rng.integers(-distinct, distinct, n).astype(dt) * (2**59 + 7)
    if t == "f64":
        v = rng.integers(-distinct, distinct, n).astype(dt)
        v[rng.random(n) < 0.1] = -0.0
        return v
    if t == "i32":
        return rng.integers(-distinct, distinct, n).astype(dt) * 100000007
    return (rng.integers(0, distinct, n) * 9).astype(dt)


def masked(rng, v, p=0.2):
    """a null mask, with garbage stored under it"""
    nl = (rng.random(len(v)) < p).astype(np.uint8)
    v = v.copy()
    v[nl.astype(bool)] = 113 if v.dtype == np.uint8 else \
        (1e300 if v.dtype == np.float64 else 2**30 + 5)
    return v, nl


def run_case(spec, ngroup, calls=EIGHT, perm=None, loop=False, **kw):
    if perm is None:
        perm = ref_perm(spec) if len(spec[ngroup][0]) else None
    st, got = raw_ordered_agg(spec, ngroup, calls, perm=perm, **kw)
    assert st == 0
    exp = (loop_ordagg if loop else ref_ordagg)(spec, ngroup, calls,
                                                perm=perm)
    check(got, exp, calls)
    return got, exp


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 3 * T + 17])
def test_sizes_all_eight_slots(n, t):
    rng = np.random.default_rng(n + 5)
    key = keys_from_runs(random_runs(rng, n, 40) if n else [])
    rng.shuffle(key)
    arg, anl = masked(rng, arg_col(rng, t, n))
    spec = [(key, None, False, False), (arg, anl, False, False)]
    got, exp = run_case(spec, 1)
    if 0 < n <= T + 1:
        assert_same(exp, loop_ordagg(spec, 1, EIGHT))
    # AGG_PLAIN on the same rows
    got, exp = run_case(spec[1:], 0)
    assert got["ngroups"] == 1
    assert got["first_row"][0] == (exp["perm"][0] if n else -1)


def test_ncalls_zero_is_distinct_on_the_keys():
    rng = np.random.default_rng(8)
    n = T + 77
    key = keys_from_runs(random_runs(rng, n, 9), np.uint8)
    arg = arg_col(rng, "i32", n)
    spec = [(key, None, False, False), (arg, None, False, False)]
    got, exp = run_case(spec, 1, calls=[])
    assert got["ngroups"] == len(np.unique(key))
    # and one call without first_row_dev
    got, _ = run_case(spec, 1, calls=[("mode",)], want_first=False)
    assert got["first_row"] is None


@pytest.mark.parametrize("ngroup", [0, 1, 3, 7])
def test_ngroup_through_a_real_sort(ex, ngroup):
    rng = np.random.default_rng(20 + ngroup)
    n = 2 * T + 3
    spec = []
    for c in range(ngroup):
        col = rng.integers(0, 2 if ngroup > 3 else 4, n).astype(
            [np.int64, np.int32, np.uint8, np.float64][c % 4])
        nl = (rng.random(n) < 0.1).astype(np.uint8) if c % 2 == 0 else None
        spec.append((col, nl, c % 3 == 1, c % 2 == 1))
    arg, anl = masked(rng, arg_col(rng, "f64", n, 5))
    spec.append((arg, anl, True, True))
    srt = ex.GpuSort([dev(s[0]) for s in spec],
                     descending=[s[2] for s in spec],
                     nulls_first=[s[3] for s in spec],
                     nulls=[dev(s[1]) for s in spec])
    perm = run_node(srt)
    assert np.array_equal(perm.cpu().numpy(), ref_perm(spec))
    st, got = raw_ordered_agg(spec, ngroup, EIGHT, perm=perm)
    assert st == 0
    check(got, ref_ordagg(spec, ngroup, EIGHT, perm=perm.cpu().numpy()),
          EIGHT)
    # the numbering and first_row are otbx_group_agg's on the same perm
    st, ga = raw_group_agg(spec[:ngroup], [("count_star",)], n,
                           perm=perm.cpu().numpy())
    assert st == 0 and ga["ngroups"] == got["ngroups"]
    assert np.array_equal(ga["first_row"], got["first_row"])


@pytest.mark.parametrize("layout", ["one_group", "one_row_per_group",
                                    "edges_on_tile_edges"])
def test_group_layouts(layout):
    rng = np.random.default_rng(33)
    n = 3 * T
    if layout == "one_group":
        key = np.zeros(n, dtype=np.int32)
    elif layout == "one_row_per_group":
        key = np.arange(n, dtype=np.int32)
    else:
        key = np.repeat(np.arange(3, dtype=np.int32), T)
    for t in ("i64", "f64"):
        arg, anl = masked(rng, arg_col(rng, t, n))
        run_case([(key, None, False, False), (arg, anl, False, False)], 1)


def test_mode_run_spans_three_tiles():
    """one value from position T-5 to 2T+9 (in three tiles) is the mode of a
    group that starts in tile 0 and ends in tile 3"""
    n = 4 * T
    arg = np.arange(n, dtype=np.int64)          # every other run: length 1
    arg[T - 5:2 * T + 10] = arg[T - 5]
    arg[100:200] = arg[100]                     # a shorter run before it
    arg[3 * T:3 * T + 300] = arg[3 * T]         # and one after
    key = np.zeros(n, dtype=np.int32)
    key[:7] = -1
    key[4 * T - 11:] = 5
    spec = [(key, None, False, False), (arg, None, False, False)]
    got, exp = run_case(spec, 1)
    assert got["aggs"][4]["val"][1] == arg[T - 5]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("where", ["inside", "straddle"])
def test_mode_tie_goes_to_the_earlier_run(where, desc):
    """two runs of equal length; the first in sort order wins, also when it
    (or the later one) straddles a tile edge"""
    n = 2 * T
    rng = np.random.default_rng(12)
    seq = np.arange(n, dtype=np.int32) + 10     # the values in sort order
    a0 = 50 if where == "inside" else T - 20
    seq[a0:a0 + 40] = seq[a0]
    b0 = a0 + 100
    seq[b0:b0 + 40] = seq[b0]
    if desc:
        seq = -seq
    p = rng.permutation(n)

    def column(s):
        col = np.empty_like(s)
        col[p] = s                              # row p[j] sorts to position j
        return col
    got, exp = run_case([(column(seq), None, desc, False)], 0, loop=True)
    assert got["aggs"][4]["val"][0] == seq[a0]
    # a longer later run does win
    seq[b0 + 40] = seq[b0]
    got, exp = run_case([(column(seq), None, desc, False)], 0, loop=True)
    assert got["aggs"][4]["val"][0] == seq[b0]


def test_fixup_crosses_a_pass_boundary():
    """(M+1)*T + 5 rows: more tile records than one pass of the fix-up scan
    holds, the smallest n that crosses it. Groups of ~1.5 tiles: nearly
    every group crosses a tile edge, and one group spans the pass boundary
    itself; a value run inside it does too."""
    n = (M + 1) * T + 5
    rng = np.random.default_rng(9)
    runs = [T + T // 2 + 7] * ((M - 3) * T // (T + T // 2 + 7))
    runs.append(4 * T)                     # from tile M-4 into tile M
    runs.append(n - sum(runs))
    assert min(runs) > 0
    assert sum(runs[:-2]) < (M - 1) * T < M * T < sum(runs[:-1])
    key = np.repeat(np.arange(len(runs), dtype=np.int32), runs)
    arg = np.sort(rng.integers(0, 40, n)).astype(np.float64)
    # sorted inside each group, with a long run across tile M-1 | M
    starts = np.cumsum([0] + runs[:-1])
    for s, r in zip(starts, runs):
        arg[s:s + r] = np.sort(rng.integers(0, 40, r))
    big = int(starts[-2])
    arg[big + 100:big + 3100] = 39.0        # sorts to the group's far end
    anl = np.zeros(n, dtype=np.uint8)
    anl[rng.random(n) < 0.05] = 1
    # identity order must be a sorted order: NULLs last inside each group
    order = np.lexsort((arg, anl, key))
    arg, anl = arg[order], anl[order]
    spec = [(key, None, False, False), (arg, anl, False, False)]
    ident = np.arange(n, dtype=np.int64)
    st, got = raw_ordered_agg(spec, 1, EIGHT, perm=None)
    assert st == 0
    exp = ref_ordagg(spec, 1, EIGHT, perm=ident)
    check(got, exp, EIGHT)
    run39 = np.flatnonzero((key == len(runs) - 2) & (arg == 39.0) & (anl == 0))
    assert run39[0] < M * T - 1000 and run39[-1] > M * T + 1000
    # and one group over everything (sorted as a whole)
    order = np.lexsort((arg, anl))
    spec = [(arg[order], anl[order], False, False)]
    st, got = raw_ordered_agg(spec, 0, EIGHT, perm=None)
    assert st == 0 and got["ngroups"] == 1
    check(got, ref_ordagg(spec, 0, EIGHT, perm=ident), EIGHT)


@pytest.mark.parametrize("t", list(TYPES))
@pytest.mark.parametrize("desc,nf", [(False, False), (False, True),
                                     (True, False), (True, True)])
def test_null_arguments(t, desc, nf):
    """all-NULL groups, NULLs in front (NULLS FIRST) and at the back, a
    descending argument, garbage under the mask"""
    rng = np.random.default_rng(44)
    n = T + 300
    key = rng.integers(0, 25, n).astype(np.int32)
    arg, anl = masked(rng, arg_col(rng, t, n, 6), 0.35)
    anl[(key == 3) | (key == 4) | (key == 24)] = 1     # all-NULL groups
    spec = [(key, None, False, False), (arg, anl, desc, nf)]
    got, exp = run_case(spec, 1)
    assert_same(exp, loop_ordagg(spec, 1, EIGHT))
    assert got["aggs"][0]["val"][3] == 0
    for a in range(1, 8):
        assert got["aggs"][a]["null"][3] == 1 and not got["aggs"][a]["val"][3]
    # everything NULL, AGG_PLAIN
    anl[:] = 1
    run_case([(arg, anl, desc, nf)], 0)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("zeros", [[0.0, -0.0], [-0.0, 0.0]])
def test_signed_zeros_are_one_value(zeros):
    arg = np.array(zeros + [3.0])
    got, _ = run_case([(arg, None, False, False)], 0, loop=True,
                      calls=[("count_distinct",), ("percentile_disc", 0.0),
                             ("mode",), ("sum_distinct",)])
    assert got["aggs"][0]["val"][0] == 2
    # the first position's bits, for both
    assert _bits(got["aggs"][1]["val"]) == _bits(zeros[:1])
    assert _bits(got["aggs"][2]["val"]) == _bits(zeros[:1])
    assert got["aggs"][3]["val"][0] == 3.0


def test_nans_count_once_and_sort_last():
    nan = np.array([0x7ff8000000000001, 0xfff8000000000123,
                    0x7ff80000000fffff], dtype=np.uint64).view(np.float64)
    arg = np.array([nan[0], 1.0, nan[1], np.inf, nan[2], 1.0])
    got, exp = run_case([(arg, None, False, False)], 0, loop=True,
                        calls=[("count_distinct",), ("percentile_disc", 1.0),
                               ("mode",), ("percentile_disc", 0.5)])
    assert got["aggs"][0]["val"][0] == 3              # 1.0, Inf, NaN
    # the last position is the last NaN in input order (the sort is stable)
    assert _bits(got["aggs"][1]["val"]) == _bits(nan[2:])
    # three NaNs are the longest run; the value is the first of them
    assert _bits(got["aggs"][2]["val"]) == _bits(nan[:1])
    assert got["aggs"][3]["val"][0] == np.inf         # K = 3 of 6


def test_inf_and_nan_stay_in_their_group():
    """groups around a tile edge: an Inf / NaN group between finite ones"""
    rng = np.random.default_rng(55)
    n = 2 * T + 40
    key = np.repeat(np.arange(5, dtype=np.int32),
                    [T - 30, 20, 20, T, n - 2 * T - 10])
    arg = rng.integers(-50, 50, n).astype(np.float64)
    arg[key == 1] = np.where(rng.random(20) < 0.5, np.inf, -np.inf)
    arg[key == 2] = np.nan
    arg[T - 30] = np.inf
    arg[T - 29] = -np.inf                   # group 1 holds both: sum is NaN
    spec = [(key, None, False, False), (arg, None, False, False)]
    got, exp = run_case(spec, 1)
    s, pc = got["aggs"][1]["val"], got["aggs"][3]["val"]
    assert np.isnan(s[1]) and np.isnan(s[2])
    for g in (0, 3, 4):
        assert np.isfinite(s[g]) and np.isfinite(pc[g])
        assert np.isfinite(got["aggs"][7]["val"][g])


@pytest.mark.parametrize("t", ["f64", "i64", "i32", "u8"])
def test_percentile_edges(t):
    """p = 0, 1, 0.5 on even and odd N, N = 1, and p * N an exact integer"""
    rng = np.random.default_rng(66)
    sizes = [1, 2, 3, 4, 5, 8, 10, 11, 64, 100]
    key = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    n = len(key)
    arg = arg_col(rng, t, n, 100)
    if t == "i64":
        arg = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)  # i8tod
    if t == "f64":
        arg = rng.normal(0, 1e3, n)
    spec = [(key, None, False, False), (arg, None, False, False)]
    for ps in ([0.0, 1.0, 0.5, 0.25], [0.1, 0.2, 0.75, 0.3]):
        calls = [("percentile_disc", p) for p in ps] + \
            [("percentile_cont", p) for p in ps]
        got, exp = run_case(spec, 1, calls=calls)
        assert_same(exp, loop_ordagg(spec, 1, calls))


def test_float_sum_distinct_bound_and_determinism():
    rng = np.random.default_rng(77)
    n = 3 * T + 17
    key = keys_from_runs(random_runs(rng, n, 700))
    pool = rng.normal(0, 1e6, 300)
    arg = rng.choice(pool, n)
    arg, anl = masked(rng, arg)
    spec = [(key, None, False, False), (arg, anl, False, False)]
    perm = ref_perm(spec)
    calls = [("sum_distinct",), ("count_distinct",)]
    st, a = raw_ordered_agg(spec, 1, calls, perm=perm)
    st2, b = raw_ordered_agg(spec, 1, calls, perm=perm)
    assert st == 0 and st2 == 0
    assert_same(a, b)
    worst = check(a, ref_ordagg(spec, 1, calls, perm=perm), calls,
                  approx=True)
    print(f"sum_distinct f64: worst error / bound = {worst:.3f}")


def test_q16_shaped_pipeline(ex):
    """count(DISTINCT x) from GpuOrderedAgg next to count(*) from
    GpuGroupAgg(perm=...) on the same sort, against the two-step
    composition: DISTINCT on (key, x), then count per key"""
    rng = np.random.default_rng(88)
    n = 40_000
    key = rng.integers(0, 300, n).astype(np.int64)
    x = rng.integers(0, 50, n).astype(np.int32)
    dk, dx = dev(key), dev(x)
    node = ex.GpuOrderedAgg([dk], dx, [("count_distinct",)])
    row = run_node(node)
    assert set(node.explain()) == {"sort", "ordered_agg"}
    ga = run_node(ex.GpuGroupAgg([dk], [("count_star",)], perm=row["perm"]))
    assert ga["ngroups"] == row["ngroups"]
    assert torch.equal(ga["first_row"], row["first_row"])
    # the parent's route
    pairs = run_node(ex.GpuGroupAgg([dk, dx], []))
    two = run_node(ex.GpuGroupAgg([pairs["keys"][0][0]], [("count_star",)]))
    assert two["ngroups"] == row["ngroups"]
    assert torch.equal(two["keys"][0][0], row["keys"][0][0])
    assert torch.equal(two["aggs"][0][0], row["aggs"][0][0])
    # and numpy
    for g, k in enumerate(row["keys"][0][0].cpu().tolist()):
        assert int(row["aggs"][0][0][g]) == len(np.unique(x[key == k]))
        assert int(ga["aggs"][0][0][g]) == int((key == k).sum())


def test_node_against_ref(ex):
    rng = np.random.default_rng(99)
    for n in (0, 1, T + 9):
        k1 = rng.integers(0, 5, n).astype(np.int32)
        k1n = (rng.random(n) < 0.2).astype(np.uint8)
        arg, anl = masked(rng, arg_col(rng, "i64", n, 4))
        spec = [(k1, k1n, True, True), (arg, anl, True, False)]
        node = ex.GpuOrderedAgg([dev(k1)], dev(arg), EIGHT,
                                arg_nulls=dev(anl), arg_descending=True,
                                descending=[True], nulls_first=[True],
                                key_nulls=[dev(k1n)])
        row = run_node(node)
        exp = ref_ordagg(spec, 1, EIGHT)
        check(node_result(row), exp, EIGHT)
        assert np.array_equal(row["perm"].cpu().numpy(), exp["perm"])
        g1, g1n = row["keys"][0]
        assert np.array_equal(g1n.cpu().numpy(), k1n[exp["first_row"]])
        # AGG_PLAIN, a passed permutation
        plain = ex.GpuOrderedAgg([], dev(arg), EIGHT, arg_nulls=dev(anl),
                                 perm=dev(ref_perm(spec[1:])) if n else None,
                                 arg_descending=True)
        row = run_node(plain)
        assert row["ngroups"] == 1 and row["keys"] == []
        check(node_result(row), ref_ordagg(spec[1:], 0, EIGHT), EIGHT)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_golden_cases_through_the_node(ex, case):
    spec, ngroup, calls = golden_case(GOLDEN, case)
    text = GOLDEN["text"].get(f"{case['table']}.{case['arg']}")
    keys = [dev(s[0]) for s in spec[:ngroup]]
    decode = None
    if text is None:
        arg = dev(spec[ngroup][0])
    else:
        # a text argument: rank the strings, aggregate the codes, decode
        strings = [text[i] for i in spec[ngroup][0].tolist()]
        r = ex.GpuText(strings).rank()
        arg = r.codes[0]

        def decode(code):
            t = torch.tensor([int(code)], dtype=torch.int64, device="cuda")
            return r.decode(t).to_list()[0].decode()
    # at most 8 calls per invocation: a longer percentile array is several
    # invocations on the first one's permutation
    row = run_node(ex.GpuOrderedAgg(keys, arg, calls[:8]))
    res = node_result(row)
    for at in range(8, len(calls), 8):
        more = run_node(ex.GpuOrderedAgg(keys, arg, calls[at:at + 8],
                                         perm=row["perm"]))
        assert more["ngroups"] == row["ngroups"]
        res["aggs"] += node_result(more)["aggs"]
    res["keys"] = [k.cpu().numpy() for k, _ in row["keys"]]
    golden_check(GOLDEN, case, res, decode=decode)
    if text is not None and case["name"] == "percentile_disc_array_names":
        cd = run_node(ex.GpuOrderedAgg([], arg, [("count_distinct",)]))
        assert int(cd["aggs"][0][0][0]) == 5      # count(DISTINCT name)


def test_finish_then_init_stays_clean(ex):
    """nothing is cached by otbx_ordered_agg: the same call gives the same
    result after otbx_finish → otbx_init"""
    from opentenbase_amd._lib import call
    rng = np.random.default_rng(95)
    n = T + 9
    key = keys_from_runs(random_runs(rng, n, 30))
    arg, anl = masked(rng, arg_col(rng, "f64", n))
    spec = [(key, None, False, False), (arg, anl, False, False)]
    perm = ref_perm(spec)
    st, a = raw_ordered_agg(spec, 1, EIGHT, perm=perm)
    call("otbx_finish")
    ex.init_device(0)
    st2, b = raw_ordered_agg(spec, 1, EIGHT, perm=perm)
    assert st == 0 and st2 == 0
    assert_same(a, b)

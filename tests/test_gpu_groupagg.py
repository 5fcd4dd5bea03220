"""GPU parity of the GroupAggregate operator (otbx_group_agg / GpuGroupAgg)
against tests/groupagg_ref.py. Everything is bit-equal to the reference
except SUM(F64) on non-integer data, which is checked against the derived
recursive-summation bound m*u*sum|x| / (1 - m*u)."""
import ctypes as C

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd._lib import AGG_FUNCS, AggCallsDev, SortSpecDev
from groupagg_ref import assert_same, ref_groupagg
from sort_ref import ref_perm

pytestmark = pytest.mark.gpu

GA_TILE = 2048          # otbx_groupagg.hip: positions per block tile
GA_FIX_THREADS = 1024   # tile records per pass of the fix-up scan
T, M = GA_TILE, GA_FIX_THREADS
GUARD = 64
U = 2.0 ** -53

_SORT_TYPE = {np.dtype(np.int64): 0, np.dtype(np.float64): 1,
              np.dtype(np.int32): 2, np.dtype(np.uint8): 3}


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


def dev(a):
    return None if a is None else \
        torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ws_bytes_for(n):
    b = C.c_size_t(0)
    assert _lib.lib().otbx_group_agg_workspace_bytes(n, C.byref(b)) == 0
    return b.value


def _out_dtypes(func, col):
    """(out dtype, has out_hi, has out_null) of one aggregate"""
    if func in ("count_star", "count"):
        return np.int64, False, False
    if func == "sum":
        if col.dtype == np.float64:
            return np.float64, False, True
        return (np.uint64, True, True) if col.dtype == np.int64 else \
            (np.int64, False, True)
    return col.dtype, False, True


def _sentinel(dt):
    dt = np.dtype(dt)
    if dt == np.uint8:
        return np.uint8(0x5a)
    if dt == np.float64:
        return np.float64(-777.0)
    if dt == np.uint64:
        return np.uint64(0x5a5a5a5a5a5a5a5a)
    return dt.type(-777)


def raw_group_agg(spec, aggs, n, perm=None, want_first=True, col_tensors=None):
    """otbx_group_agg itself. Every output buffer — requested or not — is
    pre-filled with a sentinel and carries GUARD extra entries: the entries
    past ngroups (and so past n) and the buffers not requested must come
    back untouched. col_tensors: {agg index: device tensor} to pass a
    prepared (e.g. offset) device column. Returns (status, result shaped as
    groupagg_ref's)."""
    keep = []
    sp = SortSpecDev()
    sp.nkeys = len(spec)
    for c, (col, nulls, desc, nf) in enumerate(spec):
        col = np.ascontiguousarray(col)
        tc, tn = dev(col), dev(nulls)
        keep += [tc, tn]
        sp.key[c].col = tc.data_ptr() if n else None
        sp.key[c].nulls = tn.data_ptr() if tn is not None and n else None
        sp.key[c].type = _SORT_TYPE[col.dtype]
        sp.key[c].flags = (1 if desc else 0) | (2 if nf else 0)
    calls = AggCallsDev()
    calls.naggs = len(aggs)
    bufs = []
    for i, a in enumerate(aggs):
        func = a[0]
        col = a[1] if len(a) > 1 else None
        nl = a[2] if len(a) > 2 else None
        dt, has_hi, has_null = _out_dtypes(func, col)
        ac = calls.agg[i]
        ac.func = AGG_FUNCS[func]
        ac.type = _SORT_TYPE[col.dtype] if col is not None else 0
        if col is not None:
            tc = col_tensors[i] if col_tensors and i in col_tensors \
                else dev(col)
            keep.append(tc)
            ac.col = tc.data_ptr() if n else None
        if nl is not None:
            tn = dev(nl)
            keep.append(tn)
            ac.nulls = tn.data_ptr() if n else None
        b = {"val": dev(np.full(n + GUARD, _sentinel(dt), dtype=dt)
                        .view(np.int64 if dt == np.uint64 else dt)),
             "hi": dev(np.full(n + GUARD, -777, dtype=np.int64)),
             "null": dev(np.full(n + GUARD, 0x5a, dtype=np.uint8)),
             "dt": dt, "has_hi": has_hi, "has_null": has_null}
        ac.out = b["val"].data_ptr()
        if has_hi:
            ac.out_hi = b["hi"].data_ptr()
        if has_null:
            ac.out_null = b["null"].data_ptr()
        bufs.append(b)
    first = dev(np.full(n + GUARD, -777, dtype=np.int64))
    ng = dev(np.array([-777], dtype=np.int64))
    wsb = ws_bytes_for(n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    tp = dev(perm)
    st = _lib.lib().otbx_group_agg(
        C.byref(sp), C.c_void_p(tp.data_ptr()) if tp is not None and n
        else None, C.c_int64(n), C.byref(calls), C.c_void_p(ws.data_ptr()),
        C.c_size_t(wsb), C.c_void_p(first.data_ptr()) if want_first else None,
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
        r = {"val": cut(b["val"], b["dt"], True, f"agg {i} out"),
             "null": cut(b["null"], np.uint8, b["has_null"],
                         f"agg {i} out_null")}
        hi = cut(b["hi"], np.int64, b["has_hi"], f"agg {i} out_hi")
        if hi is not None:
            r["hi"] = hi
        res["aggs"].append(r)
    return 0, res


def check(got, exp, approx=()):
    """bit-equality with the reference; the aggregates listed in approx are
    SUM(F64) over non-integer data and are held to the derived bound.
    Returns the worst observed fraction of the bound."""
    worst = 0.0
    if approx:
        g2 = dict(got, aggs=list(got["aggs"]))
        for i in approx:
            x, y = got["aggs"][i], exp["aggs"][i]
            assert np.array_equal(x["null"], y["null"])
            m = np.maximum(y["rows"] - 1, 0).astype(np.float64)
            bound = m * U * y["abs"] / (1.0 - m * U)
            err = np.abs(x["val"] - y["val"])
            assert (err <= bound).all(), (i, err.max())
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
            g2["aggs"][i] = dict(x, val=y["val"])
        got = g2
    if got["first_row"] is None:
        got = dict(got, first_row=exp["first_row"])
    assert_same(got, exp)
    return worst


def int_vals(rng, n, p_null=0.2):
    """Integer-valued doubles in [-1000, 1000] with NULLs (garbage stored
    under them): every partial sum is exact in every association order."""
    v = rng.integers(-1000, 1001, n).astype(np.float64)
    vn = (rng.random(n) < p_null).astype(np.uint8)
    v[vn.astype(bool)] = rng.normal(0, 1e300, int(vn.sum()))
    return v, vn


def mm_vals(rng, n):
    """doubles with ties of every kind for MIN / MAX: ±0, NaNs of both signs
    and several payloads, ±Inf"""
    pool = np.array([0.5, -0.0, 0.0, np.inf, -np.inf, 7.0, -3.0, 7.0, 1e300])
    v = rng.choice(pool, n)
    k = rng.random(n) < 0.15
    nan = (0x7ff8000000000000 | rng.integers(0, 1 << 20, n).astype(np.uint64)
           | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)))
    v[k] = nan.view(np.float64)[k]
    return v


def keys_from_runs(runs, dtype=np.int32):
    return np.repeat(np.arange(len(runs)) % 120, runs).astype(dtype)


def random_runs(rng, n, mean):
    runs = []
    left = n
    while left > 0:
        r = int(min(left, max(1, rng.geometric(1.0 / mean))))
        runs.append(r)
        left -= r
    return runs


def eight_aggs(rng, n):
    """all eight slots: every func, every type, masks on some"""
    v, vn = int_vals(rng, n)
    i64 = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    u8 = rng.integers(0, 256, n).astype(np.uint8)
    m2 = (rng.random(n) < 0.5).astype(np.uint8)
    return [("count_star",), ("count", i32, m2), ("sum", v, vn),
            ("sum", i32, m2), ("sum", i64, vn), ("min", mm_vals(rng, n), m2),
            ("max", i64, None), ("min", u8, vn)]


SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_all_eight_slots(n):
    rng = np.random.default_rng(n + 3)
    runs = random_runs(rng, n, 40) if n else []
    key = keys_from_runs(runs)
    spec = [(key, None, False, False)]
    aggs = eight_aggs(rng, n)
    st, got = raw_group_agg(spec, aggs, n)
    assert st == 0
    exp = ref_groupagg(spec, aggs, perm=np.arange(n, dtype=np.int64))
    assert exp["ngroups"] == len(runs)
    check(got, exp)


def _layouts():
    n = 6 * T + 100
    big = [7] * 100 + [3 * T + 11] + [5] * 50
    big.append(n - sum(big))
    # starts at 0, T-1 (a tile's last position), 2T (a group ends exactly at
    # the tile edge), 3T, 3T+1, 4T
    edge = [T - 1, T + 1, T, 1, T - 1]
    edge.append(n - sum(edge))
    rng = np.random.default_rng(5)
    return n, {"one": [n], "each": [1] * n, "big": big, "edge": edge,
               "random": random_runs(rng, n, 300),
               "short": random_runs(rng, n, 3)}


@pytest.mark.parametrize("layout", ["one", "each", "big", "edge", "random",
                                    "short"])
def test_group_layouts(layout):
    """Hand-placed groups on already sorted columns (perm = NULL): the cases
    a wrong tile record or fix-up carry breaks."""
    n, layouts = _layouts()
    runs = layouts[layout]
    assert sum(runs) == n and min(runs) > 0
    rng = np.random.default_rng(77)
    key = np.repeat(np.arange(len(runs), dtype=np.int64), runs)
    spec = [(key, None, False, False)]
    aggs = eight_aggs(rng, n)
    st, got = raw_group_agg(spec, aggs, n)
    assert st == 0
    exp = ref_groupagg(spec, aggs, perm=np.arange(n, dtype=np.int64))
    assert exp["ngroups"] == len(runs)
    assert np.array_equal(exp["first_row"],
                          np.cumsum([0] + runs[:-1]).astype(np.int64))
    check(got, exp)


def test_fixup_crosses_a_pass_boundary():
    """(M+1)*T + 5 rows: more tile records than one pass of the fix-up scan
    holds. Groups of ~1.5 tiles: nearly every group crosses a tile edge, and
    one group spans the pass boundary itself."""
    n = (M + 1) * T + 5
    rng = np.random.default_rng(9)
    runs = [T + T // 2 + 7] * ((M - 3) * T // (T + T // 2 + 7))
    runs.append(4 * T)                     # from tile M-4 into tile M
    runs.append(n - sum(runs))
    assert min(runs) > 0
    assert sum(runs[:-2]) < (M - 1) * T < M * T < sum(runs[:-1])
    key = np.repeat(np.arange(len(runs), dtype=np.int32), runs)
    v, vn = int_vals(rng, n)
    i64 = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    aggs = [("count_star",), ("sum", v, vn), ("max", mm_vals(rng, n), vn),
            ("sum", i64, None), ("min", i64, vn)]
    spec = [(key, None, False, False)]
    st, got = raw_group_agg(spec, aggs, n)
    assert st == 0
    check(got, ref_groupagg(spec, aggs, perm=np.arange(n, dtype=np.int64)))
    # and one group over everything
    st, got = raw_group_agg([], aggs, n)
    assert st == 0 and got["ngroups"] == 1
    check(got, ref_groupagg([], aggs, n=n))


def _key_col(rng, t, n):
    if t == 0:
        return rng.integers(-2, 3, n).astype(np.int64) * (2**40 + 1)
    if t == 1:
        return rng.choice(np.array([0.5, -0.0, 0.0, np.nan, -np.nan, np.inf,
                                    -np.inf, 7.0]), n)
    if t == 2:
        return rng.integers(-2, 2, n).astype(np.int32)
    return rng.integers(0, 3, n).astype(np.uint8)


def _key_spec(rng, nkeys, n):
    spec = []
    for c in range(nkeys):
        col = _key_col(rng, (c + nkeys) % 4, n)
        nl = (rng.random(n) < 0.2).astype(np.uint8) if c % 2 == 0 else None
        spec.append((col, nl, bool((c + nkeys) % 3 == 0), bool(c % 2)))
    return spec


@pytest.mark.parametrize("nkeys", [0, 1, 3, 8])
def test_keys_through_a_real_sort_permutation(ex, nkeys):
    """NULL, NaN of both signs, ±0, DESC and NULLS FIRST keys across the four
    types; the permutation is otbx_sort_perm's own."""
    rng = np.random.default_rng(100 + nkeys)
    n = 2 * T + 301
    spec = _key_spec(rng, nkeys, n)
    aggs = eight_aggs(rng, n)[:4] + [("max", mm_vals(rng, n), None)]
    perm = None
    if nkeys:
        node = ex.GpuSort([dev(c) for c, _, _, _ in spec],
                          descending=[d for _, _, d, _ in spec],
                          nulls_first=[f for _, _, _, f in spec],
                          nulls=[dev(m) for _, m, _, _ in spec])
        node.BeginCustomScan()
        perm = node.ExecCustomScan().cpu().numpy()
        node.EndCustomScan()
        assert np.array_equal(perm, ref_perm(spec))
    st, got = raw_group_agg(spec, aggs, n, perm=perm)
    assert st == 0
    exp = ref_groupagg(spec, aggs, perm=perm, n=n)
    if nkeys == 1:
        # -Inf, ±0, 0.5, 7.0, +Inf, the NaNs, the NULLs
        assert exp["ngroups"] == 7
    check(got, exp)


@pytest.mark.parametrize("nkeys", [1, 3, 8])
def test_keys_on_presorted_columns_without_perm(nkeys):
    rng = np.random.default_rng(200 + nkeys)
    n = 2 * T + 301
    spec = _key_spec(rng, nkeys, n)
    p = ref_perm(spec)
    spec = [(c[p], None if m is None else m[p], d, f) for c, m, d, f in spec]
    aggs = eight_aggs(rng, n)[3:]
    st, got = raw_group_agg(spec, aggs, n, perm=None)
    assert st == 0
    exp = ref_groupagg(spec, aggs, perm=np.arange(n, dtype=np.int64))
    assert exp["ngroups"] > 1
    check(got, exp)


def _val_col(rng, t, n):
    if t == "i64":
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    if t == "f64":
        return mm_vals(rng, n)
    if t == "i32":
        return rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    return rng.integers(0, 256, n).astype(np.uint8)


@pytest.mark.parametrize("func,type_", [
    ("count_star", None), ("count", "f64")] + [
    (f, t) for f in ("sum", "min", "max")
    for t in ("i64", "f64", "i32", "u8")])
def test_each_aggregate_alone(func, type_):
    """one aggregate per call, a masked value column read through a shuffled
    permutation, and first_row_dev == NULL"""
    rng = np.random.default_rng(31)
    n = 2 * T + 3
    runs = random_runs(rng, n, 25)
    p = rng.permutation(n).astype(np.int64)
    key = np.empty(n, dtype=np.int64)
    key[p] = np.repeat(np.arange(len(runs)), runs)
    if func == "count_star":
        agg = ("count_star",)
    else:
        col = int_vals(rng, n, 0.0)[0] if (func, type_) == ("sum", "f64") \
            else _val_col(rng, type_, n)
        agg = (func, col, (rng.random(n) < 0.3).astype(np.uint8))
    spec = [(key, None, False, False)]
    st, got = raw_group_agg(spec, [agg], n, perm=p, want_first=False)
    assert st == 0 and got["first_row"] is None
    check(got, ref_groupagg(spec, [agg], perm=p))


def test_distinct_and_offset_column():
    rng = np.random.default_rng(41)
    n = T + 77
    runs = random_runs(rng, n, 9)
    key = keys_from_runs(runs, np.uint8)
    spec = [(key, None, False, False)]
    ident = np.arange(n, dtype=np.int64)
    # naggs == 0: DISTINCT on the keys
    st, got = raw_group_agg(spec, [], n)
    assert st == 0
    check(got, ref_groupagg(spec, [], perm=ident))
    assert got["ngroups"] == len(runs)
    # a column that starts one element into its buffer: natural alignment
    for dt in (np.float64, np.int64, np.int32, np.uint8):
        base = (rng.integers(-100, 100, n + 1)).astype(dt)
        tb = dev(base)
        col = base[1:]
        for func in ("sum", "max"):
            st, got = raw_group_agg(spec, [(func, col, None)], n,
                                    col_tensors={0: tb[1:]})
            assert st == 0
            check(got, ref_groupagg(spec, [(func, col, None)], perm=ident))


def _nan(payload, neg=False):
    bits = 0x7ff8000000000000 | payload | ((1 << 63) if neg else 0)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def test_isolation_between_groups():
    """±Inf, NaN and 1e300 in one group never change a neighbouring group's
    SUM / MIN / MAX — the counterpart of the window operator's
    test_sum_isolation_between_partitions. The wild group crosses a tile
    edge, its neighbours sit on both sides of one."""
    n = 3 * T
    runs = [T - 10, 20, T - 5, 1, n - (2 * T + 6)]
    key = np.repeat(np.arange(len(runs), dtype=np.int32), runs)
    rng = np.random.default_rng(51)
    v = rng.integers(-1000, 1001, n).astype(np.float64)
    clean = v.copy()
    a = runs[0]
    v[a:a + 20] = rng.choice(np.array([np.inf, -np.inf, np.nan, 1e300,
                                       -1e300]), 20)
    v[a], v[a + 19] = np.inf, -np.inf          # Inf - Inf = NaN inside
    v[a + 5] = np.nan
    aggs = [("sum", v, None), ("min", v, None), ("max", v, None)]
    spec = [(key, None, False, False)]
    st, got = raw_group_agg(spec, aggs, n)
    assert st == 0
    base = ref_groupagg(spec, [("sum", clean, None), ("min", clean, None),
                               ("max", clean, None)],
                        perm=np.arange(n, dtype=np.int64))
    for i in range(3):
        for g in (0, 2, 3, 4):
            assert got["aggs"][i]["val"][g:g + 1].tobytes() == \
                base["aggs"][i]["val"][g:g + 1].tobytes(), (i, g)
    assert np.isnan(got["aggs"][0]["val"][1])
    assert got["aggs"][1]["val"][1] == -np.inf
    assert np.isnan(got["aggs"][2]["val"][1])   # NaN is the greatest


def test_float_tie_cases_inside_a_group_that_crosses_a_tile_edge():
    na, nb = _nan(0xa), _nan(0xb, neg=True)
    cases = [("max", [0.0, -0.0], -0.0), ("max", [-0.0, 0.0], 0.0),
             ("min", [0.0, -0.0], -0.0), ("min", [-0.0, 0.0], 0.0),
             ("max", [na, 1.0, nb], nb), ("max", [nb, 1.0, na], na),
             ("min", [1.0, na], 1.0), ("min", [na, nb], nb),
             ("min", [nb, na], na)]
    n = 2 * T
    key = np.zeros(n, dtype=np.int32)
    key[:T - 40] = -1                   # the tested group: [T-40, 2T)
    mask = np.ones(n, dtype=np.uint8)   # NULL everywhere else in the group
    aggs, want = [], []
    for func, vals, res in cases[:8]:
        # the tie partners sit on the two sides of the tile edge
        v = np.full(n, 123.0)
        m = mask.copy()
        pos = [T - 3, T + 5, T + 900][:len(vals)]
        for p, x in zip(pos, vals):
            v[p], m[p] = x, 0
        m[:T - 40] = 0
        aggs.append((func, v, m))
        want.append(res)
    spec = [(key, None, False, False)]
    st, got = raw_group_agg(spec, aggs, n)
    assert st == 0 and got["ngroups"] == 2
    for i, w in enumerate(want):
        assert got["aggs"][i]["val"][1:2].tobytes() == \
            np.array([w]).tobytes(), cases[i]
    check(got, ref_groupagg(spec, aggs, perm=np.arange(n, dtype=np.int64)))
    # the ninth case alone, both rows in one tile
    func, vals, res = cases[8]
    st, got = raw_group_agg([], [(func, np.array(vals), None)], 2)
    assert st == 0 and got["aggs"][0]["val"].tobytes() == \
        np.array([res]).tobytes()


def test_sum_f64_bound_and_determinism(capsys):
    """random non-integer doubles of mixed magnitude: within the derived
    bound of the left-to-right float8pl sum, and the same bytes twice"""
    rng = np.random.default_rng(61)
    n = 5 * T + 123
    runs = [1, 2, 3, 70, T, 2 * T + 9]
    runs += random_runs(rng, n - sum(runs), 200)
    key = np.repeat(np.arange(len(runs), dtype=np.int64), runs)
    v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 7, n)
    vn = (rng.random(n) < 0.1).astype(np.uint8)
    p = np.arange(n, dtype=np.int64)
    aggs = [("sum", v, vn), ("count", v, vn), ("sum", v, None)]
    spec = [(key, None, False, False)]
    st, a = raw_group_agg(spec, aggs, n)
    st2, b = raw_group_agg(spec, aggs, n)
    assert st == 0 and st2 == 0
    for x, y in zip(a["aggs"], b["aggs"]):
        assert x["val"].tobytes() == y["val"].tobytes()
    exp = ref_groupagg(spec, aggs, perm=p)
    worst = check(a, exp, approx=(0, 2))
    with capsys.disabled():
        print(f"\n  SUM(F64): worst observed fraction of the bound "
              f"{worst:.4f}")
    assert worst <= 1.0


def run_node(node):
    node.BeginCustomScan()
    row = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    return row


def node_result(row):
    """a GpuGroupAgg row in groupagg_ref's shape"""
    res = {"ngroups": row["ngroups"],
           "first_row": row["first_row"].cpu().numpy(), "aggs": []}
    for a in row["aggs"]:
        if len(a) == 3:
            res["aggs"].append({"val": a[0].cpu().numpy().view(np.uint64),
                                "hi": a[1].cpu().numpy(),
                                "null": a[2].cpu().numpy()})
        else:
            res["aggs"].append({"val": a[0].cpu().numpy(),
                                "null": None if a[1] is None
                                else a[1].cpu().numpy()})
    return res


@pytest.mark.parametrize("n", [0, 1, 3 * T + 17])
def test_node_against_ref_with_keys_materialised(ex, n):
    rng = np.random.default_rng(71 + n)
    k1 = _key_col(rng, 1, n)
    k2 = _key_col(rng, 2, n)
    k1n = (rng.random(n) < 0.2).astype(np.uint8)
    aggs = eight_aggs(rng, n)
    spec = [(k1, k1n, True, True), (k2, None, False, False)]
    node = ex.GpuGroupAgg(
        [dev(k1), dev(k2)],
        [tuple(dev(x) if isinstance(x, np.ndarray) else x for x in a)
         for a in aggs],
        descending=[True, False], nulls_first=[True, False],
        key_nulls=[dev(k1n), None])
    row = run_node(node)
    exp = ref_groupagg(spec, aggs)
    check(node_result(row), exp)
    assert set(node.explain()) == {"sort", "group_agg"}
    fr = exp["first_row"]
    (g1, g1n), (g2, g2n) = row["keys"]
    assert g2n is None
    assert np.array_equal(g1n.cpu().numpy(), k1n[fr])
    live = k1n[fr] == 0
    assert g1.cpu().numpy()[live].tobytes() == k1[fr][live].tobytes()
    assert np.array_equal(g2.cpu().numpy(), k2[fr])
    # a passed permutation skips the sort; no keys: AGG_PLAIN
    node = ex.GpuGroupAgg([], [("count_star",), ("sum", dev(aggs[2][1]),
                                                 dev(aggs[2][2]))], n=n)
    row = run_node(node)
    assert row["ngroups"] == 1 and row["keys"] == []
    check(node_result(row), ref_groupagg([], [aggs[0], aggs[2]], n=n))
    assert int(row["first_row"][0]) == (0 if n else -1)


def test_node_against_hash_agg(ex):
    rng = np.random.default_rng(81)
    n = 50_000
    keys = rng.integers(-500, 500, n).astype(np.int64)
    kn = (rng.random(n) < 0.05).astype(np.uint8)
    vals = rng.normal(0, 100, n)
    vn = (rng.random(n) < 0.1).astype(np.uint8)
    h = run_all(ex.GpuHashAgg(dev(keys), dev(vals), dev(kn), dev(vn)))
    node = ex.GpuGroupAgg([dev(keys)], [("count_star",),
                                        ("count", dev(vals), dev(vn)),
                                        ("sum", dev(vals), dev(vn))],
                          key_nulls=[dev(kn)])
    row = run_node(node)
    assert row["ngroups"] == len(h)
    gk = row["keys"][0][0].cpu().numpy()
    gkn = row["keys"][0][1].cpu().numpy()
    cs = row["aggs"][0][0].cpu().numpy()
    cv = row["aggs"][1][0].cpu().numpy()
    sv, svn = (t.cpu().numpy() for t in row["aggs"][2])
    # GpuHashAgg rows are sorted by (key_isnull, key): ASC NULLS LAST
    for g, r in enumerate(h):
        assert int(r["key_isnull"]) == int(gkn[g])
        if not gkn[g]:
            assert int(r["key"]) == int(gk[g])
        assert int(r["count_star"]) == int(cs[g])
        assert int(r["count_v"]) == int(cv[g])
        assert int(r["sum_isnull"]) == int(svn[g])
        assert abs(float(r["sum_v"]) - sv[g]) <= 1e-6 * abs(sv[g])


def run_all(node):
    node.BeginCustomScan()
    rows = []
    while True:
        r = node.ExecCustomScan()
        if r is None:
            break
        rows.append(r)
    node.EndCustomScan()
    return rows


def test_q1_shaped_pipeline(ex):
    """GpuFilter → GpuProject price*(1-disc) → GpuGroupAgg on (returnflag,
    linestatus) with sum, min, max and count, against numpy"""
    rng = np.random.default_rng(91)
    n = 100_000
    flag = rng.choice(np.frombuffer(b"ANR", dtype=np.uint8), n)
    status = rng.choice(np.frombuffer(b"FO", dtype=np.uint8), n)
    ship = rng.integers(0, 2600, n).astype(np.int32)
    price = rng.integers(100, 100000, n).astype(np.float64)
    disc = rng.integers(0, 11, n).astype(np.float64) / 100.0
    qty = rng.integers(1, 51, n).astype(np.int32)
    d = {k: dev(v) for k, v in dict(flag=flag, status=status, ship=ship,
                                    price=price, disc=disc, qty=qty).items()}
    flt = ex.GpuFilter([[ex.qual_term(d["ship"], "<=", 2436)]])
    sel = run_node(flt)
    disc_price, dn = run_node(ex.GpuProject(
        ex.col(d["price"]) * (1.0 - ex.col(d["disc"])), sel=sel))
    assert dn is None
    node = ex.GpuGroupAgg(
        [flt.gather(d["flag"]), flt.gather(d["status"])],
        [("sum", disc_price), ("min", disc_price), ("max", disc_price),
         ("count_star",), ("sum", flt.gather(d["qty"]))])
    row = run_node(node)
    keep = ship <= 2436
    dp = (price * (1.0 - disc))[keep]
    f, s, q = flag[keep], status[keep], qty[keep]
    groups = sorted(set(zip(f.tolist(), s.tolist())))
    assert row["ngroups"] == len(groups) == 6
    gf = row["keys"][0][0].cpu().numpy().tolist()
    gs = row["keys"][1][0].cpu().numpy().tolist()
    assert list(zip(gf, gs)) == groups
    a = [[t.cpu().numpy() if t is not None else None for t in x]
         for x in row["aggs"]]
    assert np.array_equal(disc_price.cpu().numpy(), dp)
    for g, (ff, ss) in enumerate(groups):
        x = dp[(f == ff) & (s == ss)]
        m = len(x) - 1
        assert abs(a[0][0][g] - np.cumsum(x)[-1]) <= \
            m * U * np.abs(x).sum() / (1 - m * U)
        assert a[1][0][g] == x.min() and a[2][0][g] == x.max()
        assert a[3][0][g] == len(x)
        assert a[4][0][g] == int(q[(f == ff) & (s == ss)].sum())
        assert a[0][1][g] == 0 and a[4][1][g] == 0


def test_finish_then_init_stays_clean(ex):
    """nothing is cached by otbx_group_agg: the same call gives the same
    result after otbx_finish → otbx_init"""
    from opentenbase_amd._lib import call
    rng = np.random.default_rng(95)
    n = T + 9
    key = keys_from_runs(random_runs(rng, n, 30))
    spec = [(key, None, False, False)]
    aggs = eight_aggs(rng, n)
    st, a = raw_group_agg(spec, aggs, n)
    call("otbx_finish")
    ex.init_device(0)
    st2, b = raw_group_agg(spec, aggs, n)
    assert st == 0 and st2 == 0
    assert_same(a, b)

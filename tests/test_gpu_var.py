"""GPU tests of the variance/stddev aggregate (otbx_agg_i64_var /
GpuHashAggVar): the [N, Sx, Sxx] state against the oracle's Youngs-Cramer
float8_accum (oracle_py.agg_i64(...).acc) on the same inputs.

Sxx tolerance close(got, exp, N, Sx): |got - exp| <= 1e-6*|exp| +
1e-26*Sx^2/N — the float8 parity bar plus an absolute floor
for zero-variance groups that sits far below the double resolution of the
data, (1e-16*mean)^2 * N. Counts and keys are bit-exact, sum_v within 1e-6
relative, as for otbx_agg_i64."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REL = 1e-6
I64_MIN = -(2**63)


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def ora():
    from oracle import oracle_py
    return oracle_py


def close(got, exp, N, Sx):
    floor = 1e-26 * Sx * Sx / N if N > 0 else 0.0
    return abs(got - exp) <= REL * abs(exp) + floor


def drain(node):
    node.BeginCustomScan()
    rows = []
    while True:
        r = node.ExecCustomScan()
        if r is None:
            break
        rows.append(r)
    node.EndCustomScan()
    return rows


def _dev(a, dt):
    return None if a is None else torch.as_tensor(a, dtype=dt, device="cuda")


def _var(ex, keys, vals, kn=None, vn=None):
    return drain(ex.GpuHashAggVar(_dev(keys, torch.int64),
                                  _dev(vals, torch.float64),
                                  _dev(kn, torch.uint8),
                                  _dev(vn, torch.uint8)))


def _var_raw(ex, keys, vals, kn=None, vn=None, ws=None, ws_bytes=None):
    """otbx_agg_i64_var at the C-ABI: returns the group records as one
    structured array (no per-row Python objects), optionally reusing a
    caller's workspace tensor."""
    from opentenbase_amd._lib import call, lib
    n = len(keys)
    k, v = _dev(keys, torch.int64), _dev(vals, torch.float64)
    knd, vnd = _dev(kn, torch.uint8), _dev(vn, torch.uint8)
    if ws_bytes is None:
        wsb = C.c_size_t(0)
        lib().otbx_agg_i64_var_workspace_bytes(C.c_int64(n), C.byref(wsb))
        ws_bytes = wsb.value
    if ws is None:
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device="cuda")
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")

    def vp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    call("otbx_agg_i64_var", vp(k), vp(knd), vp(v), vp(vnd), C.c_int64(n),
         C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes),
         C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    g = int(ng.cpu().item())
    return out[: g * 48].cpu().numpy().view(np.dtype(ex.VAR_GROUP_DTYPE))


def _ident(isnull, key):
    return (bool(isnull), 0 if isnull else int(key))


def check_parity(got, exp, every=1, label=""):
    """Every `every`-th oracle group: the otbx_agg_i64 invariants (keys and
    counts bit-exact, sum_v within 1e-6) plus Sxx within close()."""
    assert len(got) == len(exp)
    gm = {_ident(g["key_isnull"], g["key"]): g for g in got}
    assert len(gm) == len(got)
    worst = 0.0
    for e in exp[::every]:
        g = gm[_ident(e.key_isnull, e.key)]
        assert int(g["count_star"]) == e.count_star
        assert int(g["count_v"]) == e.count_v
        assert int(g["sum_isnull"]) == int(e.count_v == 0)
        N, Sx, Sxx = e.acc[0], e.acc[1], e.acc[2]
        sv, sxx = float(g["sum_v"]), float(g["sxx"])
        if e.count_v == 0:
            assert sxx == 0.0
            continue
        if math.isfinite(e.sum_v):
            assert abs(sv - e.sum_v) <= REL * abs(e.sum_v)
        else:
            assert sv == e.sum_v or (math.isnan(sv) and math.isnan(e.sum_v))
        if math.isnan(Sxx):
            assert math.isnan(sxx)
            continue
        if Sxx > 0:
            worst = max(worst, abs(sxx - Sxx) / Sxx)
        assert sxx >= 0.0
        assert close(sxx, Sxx, N, Sx), (e.key, sxx, Sxx, N, Sx)
    print(f"{label} groups={len(exp)} worst rel Sxx err={worst:.3e}")


# 1. cancellation: the case that tells the algorithms apart -----------------

@pytest.mark.parametrize("off", [0.0, 1e6, 1e7])
def test_var_cancellation(ex, ora, off):
    """At mean 1e6/1e7 and stddev 1 the oracle is within 1e-9 of exact and
    a sum(x^2) - Sx^2/N implementation is off by >= 4e-4: the 1e-6 bar
    separates them."""
    rng = np.random.default_rng(101)
    n = 100_003  # not a multiple of 64 or 256
    keys = rng.integers(0, 250, n)
    vals = off + rng.standard_normal(n)
    check_parity(_var(ex, keys, vals), ora.agg_i64(keys, vals),
                 label=f"cancel off={off:g}")


# 2. hot keys: LDS pre-aggregation + flush ----------------------------------

def test_var_hot_keys(ex, ora):
    rng = np.random.default_rng(102)
    n = 200_000
    keys = rng.integers(0, 4, n)
    vals = 1e6 + rng.standard_normal(n)
    got = _var(ex, keys, vals)
    assert len(got) == 4
    check_parity(got, ora.agg_i64(keys, vals), label="hot4")


# 3. NULL semantics ---------------------------------------------------------

@pytest.fixture(scope="module")
def null_case(ora):
    rng = np.random.default_rng(103)
    n = 100_000
    keys = rng.integers(0, 500, n)
    kn = (rng.random(n) < 0.10).astype(np.uint8)
    vn = (rng.random(n) < 0.20).astype(np.uint8)
    vals = rng.random(n) * 100
    vn[keys == 499] = 1  # a key whose values are all NULL
    return keys, vals, kn, vn, ora.agg_i64(keys, vals, kn, vn)


def test_var_null_semantics(ex, null_case):
    keys, vals, kn, vn, exp = null_case
    got = _var(ex, keys, vals, kn, vn)
    check_parity(got, exp, label="nulls")
    nullg = [g for g in got if g["key_isnull"]]
    assert len(nullg) == 1
    assert int(nullg[0]["count_star"]) == int(kn.sum())
    assert int(nullg[0]["count_v"]) == int(((kn == 1) & (vn == 0)).sum())
    assert float(nullg[0]["sxx"]) > 0.0
    # sorted by (key_isnull, key): the NULL-key group is last
    assert got[-1]["key_isnull"] == 1
    allnull = [g for g in got if not g["key_isnull"] and g["key"] == 499]
    assert len(allnull) == 1
    assert int(allnull[0]["sum_isnull"]) == 1
    assert int(allnull[0]["count_v"]) == 0
    assert int(allnull[0]["count_star"]) == int(((keys == 499) &
                                                 (kn == 0)).sum())
    assert ex.var_pop(allnull[0]["count_v"], allnull[0]["sxx"]) is None


# 4. edges ------------------------------------------------------------------

def test_var_empty_input(ex):
    assert _var(ex, np.zeros(0, np.int64), np.zeros(0, np.float64)) == []


def test_var_singleton_groups(ex, ora):
    rng = np.random.default_rng(104)
    keys = np.arange(1000)
    vals = 1e6 + rng.standard_normal(1000)
    got = _var(ex, keys, vals)
    check_parity(got, ora.agg_i64(keys, vals), label="singletons")
    for g in got:
        assert float(g["sxx"]) == 0.0
        assert ex.var_samp(g["count_v"], g["sxx"]) is None
        assert ex.var_pop(g["count_v"], g["sxx"]) == 0.0


def test_var_constant_group(ex, ora):
    keys = np.zeros(1000, dtype=np.int64)
    vals = np.full(1000, 1000000.1)
    got = _var(ex, keys, vals)
    assert len(got) == 1
    assert float(got[0]["sxx"]) >= 0.0
    check_parity(got, ora.agg_i64(keys, vals), label="constant")


def test_var_int64_min_key(ex, ora):
    rng = np.random.default_rng(105)
    n = 20_000
    keys = rng.integers(0, 30, n)
    keys[::37] = I64_MIN
    vals = 1e6 + rng.standard_normal(n)
    got = _var(ex, keys, vals)
    check_parity(got, ora.agg_i64(keys, vals), label="int64_min")
    g = [g for g in got if int(g["key"]) == I64_MIN and not g["key_isnull"]]
    assert len(g) == 1
    assert int(g[0]["count_v"]) == len(keys[::37])
    assert float(g[0]["sxx"]) > 0.0


def test_var_inf_nan_groups(ex, ora):
    rng = np.random.default_rng(106)
    n = 5000
    keys = np.concatenate([rng.integers(0, 20, n), [100, 100, 100],
                           [200, 200, 200]])
    vals = np.concatenate([1e6 + rng.standard_normal(n),
                           [1.0, np.inf, 2.0], [1.0, np.nan, 2.0]])
    got = _var(ex, keys, vals)
    gm = {int(g["key"]): g for g in got}
    assert math.isnan(float(gm[100]["sxx"]))
    assert math.isnan(float(gm[200]["sxx"]))
    for k in range(20):
        assert math.isfinite(float(gm[k]["sxx"]))
    check_parity(got, ora.agg_i64(keys, vals), label="inf/nan")


# 5. partitioned pass-1 paths (direct emission leaves no global table) ------

def _partitioned_input():
    rng = np.random.default_rng(107)
    n = 8_400_000  # smallest size above the 8 Mi-row partition threshold
    keys = rng.integers(0, 100_000, n)
    keys[1_234_567] = I64_MIN
    keys[7_654_321] = I64_MIN
    vals = 1e5 + 30 * rng.standard_normal(n)
    return rng, n, keys, vals


def test_var_partitioned_direct_path(ex, ora):
    _, n, keys, vals = _partitioned_input()
    got = _var(ex, keys, vals)
    exp = ora.agg_i64(keys, vals)
    assert sum(int(g["count_star"]) for g in got) == n
    check_parity(got, exp, every=29, label="partitioned direct")
    sent = [e for e in exp if e.key == I64_MIN]
    check_parity([g for g in got if int(g["key"]) == I64_MIN], sent,
                 label="partitioned direct sentinel")


def test_var_partitioned_gather_path(ex, ora):
    rng, n, keys, vals = _partitioned_input()
    kn = (rng.random(n) < 0.02).astype(np.uint8)
    vn = (rng.random(n) < 0.05).astype(np.uint8)
    got = _var(ex, keys, vals, kn, vn)
    exp = ora.agg_i64(keys, vals, kn, vn)
    assert sum(int(g["count_star"]) for g in got) == n
    check_parity(got, exp, every=29, label="partitioned gather")
    check_parity([g for g in got if g["key_isnull"]],
                 [e for e in exp if e.key_isnull],
                 label="partitioned gather NULL group")


def test_var_partitioned_two_level_path(ex, ora):
    """300k distinct keys: pass 1 partitions at both levels (nb=256,
    nb2=4); the bucket-resident second pass runs over the level-2
    records."""
    rng = np.random.default_rng(109)
    n = 8_400_000
    keys = rng.integers(0, 300_000, n)
    keys[::2_000_000] = I64_MIN
    vals = 1e6 + rng.standard_normal(n)
    got = _var(ex, keys, vals)
    exp = ora.agg_i64(keys, vals)
    assert sum(int(g["count_star"]) for g in got) == n
    check_parity(got, exp, every=29, label="partitioned two-level")
    check_parity([g for g in got if int(g["key"]) == I64_MIN],
                 [e for e in exp if e.key == I64_MIN],
                 label="partitioned two-level sentinel")


def test_var_partitioned_flagged_buckets(ex, ora):
    """The estimator's strided sample (every 8th row) sees a 3000-key
    domain, the other rows a 400k-key one: pass 1 partitions into 64
    buckets of ~6000 distinct keys, every LDS table overflows and the
    buckets are recomputed through the global table. The second pass must
    take its per-row route for those buckets."""
    rng = np.random.default_rng(110)
    n = 8_400_000
    stride = n // (1 << 20)
    keys = rng.integers(0, 400_000, n)
    keys[::stride] = rng.integers(0, 3000, len(keys[::stride]))
    vals = 1e6 + rng.standard_normal(n)
    got = _var(ex, keys, vals)
    exp = ora.agg_i64(keys, vals)
    assert sum(int(g["count_star"]) for g in got) == n
    check_parity(got, exp, every=29, label="partitioned flagged")


# 6. small-table abort path-------------------------------------------------

def test_var_small_table_abort_path(ex):
    """Input of test_agg_small_table_abort_path: the estimator sees only the
    hot key, the estimator-sized table aborts and pass 1 redoes at full
    capacity; the index is then built over ~7.3 M groups."""
    n = 8_400_000
    stride = n // (1 << 20)
    keys = np.arange(n, dtype=np.int64) + 1_000_000
    keys[::stride] = 7
    vals = 1e6 + (np.arange(n) % 7).astype(np.float64)
    groups = _var_raw(ex, keys, vals)
    assert len(groups) == len(np.unique(keys))
    assert int(groups["count_star"].sum()) == n
    hot = groups[groups["key"] == 7]
    assert len(hot) == 1
    hv = vals[::stride]
    assert int(hot["count_v"][0]) == len(hv)
    two_pass = float(((hv - hv.mean()) ** 2).sum())
    sxx = float(hot["sxx"][0])
    print(f"abort path hot group sxx={sxx!r} two-pass={two_pass!r}")
    assert close(sxx, two_pass, len(hv), float(hot["sum_v"][0]))
    cold = groups[groups["key"] != 7]
    assert (cold["count_v"] == 1).all()
    assert (cold["sxx"] == 0.0).all()


# 7. workspace contract -----------------------------------------------------

def test_var_workspace_contract(ex, ora):
    from opentenbase_amd._lib import OtbxError, lib
    rng = np.random.default_rng(108)
    n = 50_000
    wsb = C.c_size_t(0)
    lib().otbx_agg_i64_var_workspace_bytes(C.c_int64(n), C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    keys1 = rng.integers(0, 3000, n)
    vals1 = 1e6 + rng.standard_normal(n)
    with pytest.raises(OtbxError) as ei:
        _var_raw(ex, keys1, vals1, ws=ws, ws_bytes=wsb.value - 1)
    assert ei.value.status == 3
    # two calls, different inputs, same workspace: no stale index or
    # accumulator survives
    keys2 = rng.integers(2000, 2040, n)
    vals2 = -5e5 + 3 * rng.standard_normal(n)
    for keys, vals, label in ((keys1, vals1, "ws call 1"),
                              (keys2, vals2, "ws call 2")):
        got = _var_raw(ex, keys, vals, ws=ws, ws_bytes=wsb.value)
        check_parity(list(got), ora.agg_i64(keys, vals), label=label)


# 8. consistency with the old operator --------------------------------------

def test_var_consistent_with_hash_agg(ex, null_case):
    keys, vals, kn, vn, _ = null_case
    new = _var(ex, keys, vals, kn, vn)
    old = drain(ex.GpuHashAgg(_dev(keys, torch.int64),
                              _dev(vals, torch.float64),
                              _dev(kn, torch.uint8), _dev(vn, torch.uint8)))
    assert len(new) == len(old)
    for a, b in zip(new, old):  # both sorted by (key_isnull, key)
        for f in ("key", "key_isnull", "count_star", "count_v", "sum_isnull"):
            assert int(a[f]) == int(b[f])
        assert abs(float(a["sum_v"]) - float(b["sum_v"])) <= \
            1e-9 * abs(float(b["sum_v"]))

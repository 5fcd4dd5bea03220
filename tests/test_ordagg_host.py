"""CPU-side tests of the DISTINCT / ordered-set aggregates' host layers: the
row-loop reference against the reference suite's own recorded results and
against a brute-force restatement (numpy unique / Counter per group), the
vectorised reference against the row loop, GpuOrderedAgg's argument handling,
and the argument checks and workspace sizing of otbx_ordered_agg (pure host
code — no HIP call is reached)."""
import ctypes as C
import itertools
import json
import math
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import OAggCallDev, OAggCallsDev, SortSpecDev
from groupagg_ref import ref_groupagg
from ordagg_ref import (assert_same, check_fraction, golden_case,
                        golden_check, loop_ordagg, ref_ordagg)
from sort_ref import norm_key, ref_perm

OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden",
                                     "ordagg_cases.json")))
ALL_CALLS = [("count_distinct",), ("sum_distinct",), ("percentile_disc", 0.5),
             ("percentile_cont", 0.5), ("mode",), ("percentile_disc", 0.0),
             ("percentile_cont", 1.0), ("percentile_cont", 0.37)]


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


# ---- the reference against the reference suite's recorded results ----

@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_ref_reproduces_the_recorded_results(case):
    spec, ngroup, calls = golden_case(GOLDEN, case)
    for fn in (ref_ordagg, loop_ordagg):
        if fn is loop_ordagg and len(spec[0][0]) > 2000:
            continue    # the row loop is for small inputs
        res = fn(spec, ngroup, calls)
        res["keys"] = [spec[c][0][res["first_row"]] for c in range(ngroup)]
        golden_check(GOLDEN, case, res)


def test_the_golden_set_is_the_issues():
    names = {c["name"] for c in GOLDEN["cases"]}
    assert names == {
        "count_distinct_four", "sum_distinct_four_by_ten",
        "percentile_cont_series5", "percentile_cont_aggtest_b",
        "percentile_cont_thousand", "percentile_disc_thousand",
        "percentile_disc_array_thousand", "percentile_cont_array_thousand",
        "percentile_cont_array_series6", "mode_string4_by_ten",
        "percentile_disc_array_names"}
    by = {c["name"]: c for c in GOLDEN["cases"]}
    assert by["count_distinct_four"]["expected"] == [[4]]
    assert by["percentile_cont_aggtest_b"]["expected"] == [[53.4485001564026]]
    assert by["percentile_disc_array_names"]["expected"] == \
        [["fred", "jill", "jim"]]
    # count(four) next to sum(DISTINCT four): the ordinary aggregate of the
    # same target list, on the same permutation
    case = by["sum_distinct_four_by_ten"]
    spec, ngroup, _ = golden_case(GOLDEN, case)
    perm = ref_perm(spec)
    g = ref_groupagg(spec[:1], [("count", spec[1][0], None)], perm=perm)
    assert g["aggs"][0]["val"].tolist() == case["count"]


def test_percentile_cont_of_aggtest_b_bits():
    """b is float4: the float32-rounded values widened, then the formula"""
    case = [c for c in GOLDEN["cases"]
            if c["name"] == "percentile_cont_aggtest_b"][0]
    spec, ngroup, calls = golden_case(GOLDEN, case)
    b = spec[0][0]
    assert (b == b.astype(np.float32).astype(np.float64)).all()
    v = loop_ordagg(spec, ngroup, calls)["aggs"][0]["val"][0]
    assert repr(float(v)) == "53.44850015640259"


# ---- row loop == vectorised == brute force ----

def _rand_arg(rng, t, n):
    if t == 0:
        return rng.integers(-3, 4, n).astype(np.int64) * (2**61 // 3)
    if t == 1:
        v = rng.integers(-4, 5, n).astype(np.float64)
        v[rng.random(n) < 0.1] = -0.0
        v[rng.random(n) < 0.1] = 0.0
        k = rng.random(n) < 0.1
        nan = (0x7ff8000000000000 | rng.integers(0, 1 << 20, n)
               .astype(np.uint64)
               | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)))
        v[k] = nan.view(np.float64)[k]
        v[rng.random(n) < 0.03] = np.inf
        return v
    if t == 2:
        return rng.integers(-5, 5, n).astype(np.int32) * 300000000
    return rng.integers(0, 6, n).astype(np.uint8) * 50


def _rand_spec(rng, n, ngroup, t):
    spec = []
    for c in range(ngroup):
        col = rng.integers(0, 3, n).astype([np.int64, np.int32,
                                            np.uint8][c % 3])
        nl = (rng.random(n) < 0.15).astype(np.uint8) if c == 0 else None
        spec.append((col, nl, bool(rng.integers(0, 2)),
                     bool(rng.integers(0, 2))))
    arg = _rand_arg(rng, t, n)
    anl = (rng.random(n) < 0.3).astype(np.uint8)
    if rng.integers(0, 4) == 0:
        anl[:] = 1                         # every argument NULL
    if t == 1:
        arg[anl.astype(bool)] = 1e300      # garbage under the mask
    spec.append((arg, anl, bool(rng.integers(0, 2)),
                 bool(rng.integers(0, 2))))
    return spec


def brute_ordagg(spec, ngroup, calls, perm):
    """a second restatement: per group, numpy unique and a Counter over the
    normalised argument; returns rows of Python values (None = NULL)"""
    n = len(perm)
    gk = [norm_key(*s) for s in spec[:ngroup]]
    acol, anull, adesc, anf = spec[ngroup]
    _, ak = norm_key(acol, None, False, False)
    rows = perm.tolist()
    ident = [tuple((int(nb[r]), int(k[r])) for nb, k in gk) for r in rows]
    out = []
    j = 0
    for _, grp in itertools.groupby(range(n), key=lambda p: ident[p]):
        grp = [rows[p] for p in grp]
        j += len(grp)
        nn = [r for r in grp if anull is None or not anull[r]]
        N = len(nn)
        res = []
        keys = np.array([ak[r] for r in nn], dtype=np.uint64)
        uniq, idx = np.unique(keys, return_index=True)
        for c in calls:
            f = c[0]
            if f == "count_distinct":
                res.append(len(uniq))
            elif N == 0:
                res.append(None)
            elif f == "sum_distinct":
                # np.unique picks each value's first occurrence
                vals = [acol[nn[i]] for i in sorted(idx.tolist())]
                if acol.dtype == np.float64:
                    s = float(vals[0])
                    for x in vals[1:]:
                        s = s + float(x)
                    res.append(s)
                else:
                    res.append(sum(int(x) for x in vals))
            elif f == "percentile_disc":
                k = max(int(math.ceil(c[1] * N)), 1)
                res.append(acol[nn[k - 1]])
            elif f == "percentile_cont":
                t = c[1] * (N - 1)
                lo, hi = int(math.floor(t)), int(math.ceil(t))
                a, b = float(acol[nn[lo]]), float(acol[nn[hi]])
                res.append(a if lo == hi else a + (t - lo) * (b - a))
            else:
                cnt = Counter(keys.tolist())   # keeps first-seen order
                best = max(cnt.values())
                first = next(k for k, v in cnt.items() if v == best)
                res.append(acol[nn[keys.tolist().index(first)]])
        out.append(res)
    assert j == n
    if n == 0 and ngroup == 0:
        out.append([0 if c[0] == "count_distinct" else None for c in calls])
    return out


def _bits(x):
    return np.asarray(x).tobytes()


def _same_as_brute(res, brute, calls, adt):
    assert res["ngroups"] == len(brute)
    for g, row in enumerate(brute):
        for a, c in enumerate(calls):
            out = res["aggs"][a]
            want = row[a]
            if want is None:
                assert out["null"][g] == 1 and not out["val"][g]
                continue
            assert out["null"] is None or out["null"][g] == 0
            if c[0] == "sum_distinct" and adt == np.int64:
                got = (int(out["hi"][g]) << 64) | int(out["val"][g])
                assert got == want
            elif c[0] in ("count_distinct", "sum_distinct") and \
                    adt != np.float64:
                assert int(out["val"][g]) == want
            else:
                # bit patterns: -0 / +0 and NaN payloads count
                w = np.array(want, dtype=out["val"].dtype)
                assert _bits(out["val"][g]) == _bits(w), (g, a, c)


@pytest.mark.parametrize("t", [0, 1, 2, 3])
@pytest.mark.parametrize("ngroup", [0, 1, 3])
def test_loop_vectorised_and_brute_force_agree(t, ngroup):
    rng = np.random.default_rng(100 * t + ngroup)
    for n in (0, 1, 2, 7, 60, 300):
        spec = _rand_spec(rng, n, ngroup, t)
        perm = ref_perm(spec) if n else np.zeros(0, np.int64)
        a = loop_ordagg(spec, ngroup, ALL_CALLS, perm=perm)
        b = ref_ordagg(spec, ngroup, ALL_CALLS, perm=perm)
        assert_same(a, b)
        _same_as_brute(a, brute_ordagg(spec, ngroup, ALL_CALLS, perm),
                       ALL_CALLS, spec[ngroup][0].dtype)
        # the group numbering is otbx_group_agg's for the GROUP BY keys
        if n:
            g = ref_groupagg(spec[:ngroup], [("count_star",)], perm=perm)
            assert g["ngroups"] == a["ngroups"]
            assert np.array_equal(g["first_row"], a["first_row"])


def test_hand_cases():
    f = np.array([2.0, -0.0, 0.0, 2.0, 2.0, 5.0, 5.0, 5.0])
    perm = ref_perm([(f, None, False, False)])
    r = loop_ordagg([(f, None, False, False)], 0,
                    [("count_distinct",), ("mode",), ("percentile_disc", 0.0),
                     ("sum_distinct",)], perm=perm)
    assert r["aggs"][0]["val"][0] == 3
    assert r["aggs"][1]["val"][0] == 2.0           # 3 x 2.0 before 3 x 5.0
    assert _bits(r["aggs"][2]["val"][0]) == _bits(np.float64(-0.0))
    assert r["aggs"][3]["val"][0] == 7.0
    # descending: 5.0 comes first and wins the tie
    perm = ref_perm([(f, None, True, False)])
    r = loop_ordagg([(f, None, True, False)], 0, [("mode",)], perm=perm)
    assert r["aggs"][0]["val"][0] == 5.0
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            check_fraction(bad)


# ---- GpuOrderedAgg's argument handling ----

def test_gpuorderedagg_argument_handling():
    k = torch.zeros(4, dtype=torch.int32)
    v = torch.zeros(4, dtype=torch.float64)
    node = ex.GpuOrderedAgg([k], v, [("count_distinct",),
                                     ("percentile_cont", 0.5)],
                            descending=[True], arg_descending=True)
    assert node.n == 4 and node.flags == [1 | 2, 1]
    assert node.explain() is None
    assert ex.GpuOrderedAgg([], v, [("mode",)], arg_descending=True,
                            arg_nulls_first=None).flags == [1 | 2]
    for bad in ([("median",)], [("percentile_disc",)], [("mode", 0.5)],
                [("percentile_cont", 1.5)], [("percentile_disc", -0.1)],
                [("percentile_disc", float("nan"))], [("mode",)] * 9):
        with pytest.raises(_lib.OtbxError):
            ex.GpuOrderedAgg([k], v, bad)
    with pytest.raises(_lib.OtbxError):
        ex.GpuOrderedAgg([k] * 8, v, [("mode",)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuOrderedAgg([k], v.to(torch.float32), [("mode",)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuOrderedAgg([k[:3]], v, [("mode",)])


# ---- otbx_ordered_agg argument checks: all rejected before any HIP call ----

def test_struct_sizes_match_the_header():
    hdr = open(os.path.join(REPO, "include", "otbx.h")).read()
    assert re.search(r"\}\s*otbx_oaggcall;\s*/\*\s*40 B\s*\*/", hdr)
    assert C.sizeof(OAggCallDev) == 40
    assert C.sizeof(OAggCallsDev) == 8 + 8 * 40
    assert OAggCallDev.fraction.offset == 24 and OAggCallDev.func.offset == 32
    assert OAggCallsDev.call.offset == 8
    m = re.search(r"enum \{ OTBX_OAGG_COUNT_DISTINCT = 0, "
                  r"OTBX_OAGG_SUM_DISTINCT,\s*OTBX_OAGG_PERCENTILE_DISC, "
                  r"OTBX_OAGG_PERCENTILE_CONT, OTBX_OAGG_MODE \};", hdr)
    assert m and _lib.OAGG_FUNCS == {
        "count_distinct": 0, "sum_distinct": 1, "percentile_disc": 2,
        "percentile_cont": 3, "mode": 4}


def _ws(so, n, ncalls=1):
    out = C.c_size_t(0)
    st = so.otbx_ordered_agg_workspace_bytes(n, ncalls, C.byref(out))
    return st, out.value


def test_ordered_agg_workspace_sizing(so):
    for ncalls in (0, 1, 8):
        prev = -1
        for n in (0, 1, 1000, 2048, 2049, 10**6, 10**8, INT32_MAX):
            st, b = _ws(so, n, ncalls)
            assert st == 0 and b >= prev
            if n > 0:
                assert b > 0
            prev = b
    assert _ws(so, 0)[1] == 0
    assert _ws(so, 10**6, 0)[1] <= _ws(so, 10**6, 1)[1]
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert _ws(so, 10, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, 10, 9)[0] == OTBX_ERR_INVALID
    assert so.otbx_ordered_agg_workspace_bytes(10, 1, None) == \
        OTBX_ERR_INVALID


P = 0x1000   # a dummy device pointer: never dereferenced


def _spec(nkeys=2, type_=1, flags=0, col=P):
    sp = SortSpecDev()
    sp.nkeys = nkeys
    for c in range(min(max(nkeys, 0), 8)):
        sp.key[c].col = col
        sp.key[c].nulls = None
        sp.key[c].type = type_
        sp.key[c].flags = flags
    return sp


def _call(func, fraction=0.5, out=P, out_hi=None, out_null="auto"):
    if out_null == "auto":
        out_null = None if func == 0 else P
    return dict(func=func, fraction=fraction, out=out, out_hi=out_hi,
                out_null=out_null)


def _calls(cs, ncalls=None):
    s = OAggCallsDev()
    s.ncalls = len(cs) if ncalls is None else ncalls
    for i, a in enumerate(cs[:8]):
        for k, v in a.items():
            setattr(s.call[i], k, v)
    return s


def _ordered_agg(so, sp, ngroup, n, calls, ws_bytes=None, ws=P, first=P,
                 ng=P):
    """otbx_ordered_agg with dummy (never dereferenced) device pointers."""
    if ws_bytes is None:
        st, ws_bytes = _ws(so, max(min(n, INT32_MAX), 0), 8)
        assert st == 0
    return so.otbx_ordered_agg(
        None if sp is None else C.byref(sp), C.c_int32(ngroup),
        C.c_void_p(P), C.c_int64(n),
        None if calls is None else C.byref(calls), C.c_void_p(ws),
        C.c_size_t(ws_bytes), C.c_void_p(first), C.c_void_p(ng), None)


@pytest.mark.parametrize("case", [
    "null_spec", "null_calls", "null_ngroups", "ngroup_neg", "ngroup8",
    "nkeys_short", "nkeys_long", "key_type_neg", "key_type4", "key_flags4",
    "key_flags_neg", "ncalls_neg", "ncalls9", "nothing_requested",
    "func_neg", "func5", "disc_fraction_neg", "disc_fraction_big",
    "disc_fraction_nan", "cont_fraction_neg", "cont_fraction_big",
    "cont_fraction_nan", "null_out", "count_null_out",
    "sum_without_out_null", "disc_without_out_null", "cont_without_out_null",
    "mode_without_out_null", "count_with_out_null", "sum_i64_without_hi",
    "sum_f64_with_hi", "sum_i32_with_hi", "count_with_hi", "mode_with_hi",
    "n_neg", "n_big", "null_key_col", "null_arg_col", "ws_short", "ws_null",
    "ws_misaligned", "bad_call_in_last_slot"])
def test_ordered_agg_invalid_arguments(so, case):
    n, ngroup, ws_bytes, ws, first, ng = 100, 1, None, P, P, P
    sp = _spec()
    good = [_call(0), _call(1), _call(2), _call(3), _call(4)]
    calls = _calls(good)
    nan = float("nan")
    if case == "null_spec":
        sp = None
    elif case == "null_calls":
        calls = None
    elif case == "null_ngroups":
        ng = None
    elif case == "ngroup_neg":
        ngroup, sp = -1, _spec(nkeys=0)
    elif case == "ngroup8":
        ngroup, sp = 8, _spec(nkeys=9)
    elif case == "nkeys_short":
        sp = _spec(nkeys=1)
    elif case == "nkeys_long":
        sp = _spec(nkeys=3)
    elif case == "key_type_neg":
        sp = _spec(type_=-1)
    elif case == "key_type4":
        sp = _spec(type_=4)
    elif case == "key_flags4":
        sp = _spec(flags=4)
    elif case == "key_flags_neg":
        sp = _spec(flags=-1)
    elif case == "ncalls_neg":
        calls = _calls(good, ncalls=-1)
    elif case == "ncalls9":
        calls = _calls([_call(0)] * 8, ncalls=9)
    elif case == "nothing_requested":
        calls, first = _calls([]), None
    elif case == "func_neg":
        calls = _calls([_call(-1)])
    elif case == "func5":
        calls = _calls([_call(5)])
    elif case == "disc_fraction_neg":
        calls = _calls([_call(2, fraction=-1e-9)])
    elif case == "disc_fraction_big":
        calls = _calls([_call(2, fraction=1.0000001)])
    elif case == "disc_fraction_nan":
        calls = _calls([_call(2, fraction=nan)])
    elif case == "cont_fraction_neg":
        calls = _calls([_call(3, fraction=-0.5)])
    elif case == "cont_fraction_big":
        calls = _calls([_call(3, fraction=2.0)])
    elif case == "cont_fraction_nan":
        calls = _calls([_call(3, fraction=nan)])
    elif case == "null_out":
        calls = _calls([_call(4, out=None)])
    elif case == "count_null_out":
        calls = _calls([_call(0, out=None)])
    elif case == "sum_without_out_null":
        calls = _calls([_call(1, out_null=None)])
    elif case == "disc_without_out_null":
        calls = _calls([_call(2, out_null=None)])
    elif case == "cont_without_out_null":
        calls = _calls([_call(3, out_null=None)])
    elif case == "mode_without_out_null":
        calls = _calls([_call(4, out_null=None)])
    elif case == "count_with_out_null":
        calls = _calls([_call(0, out_null=P)])
    elif case == "sum_i64_without_hi":
        sp = _spec(type_=0)
        calls = _calls([_call(1)])
    elif case == "sum_f64_with_hi":
        calls = _calls([_call(1, out_hi=P)])
    elif case == "sum_i32_with_hi":
        sp = _spec(type_=2)
        calls = _calls([_call(1, out_hi=P)])
    elif case == "count_with_hi":
        calls = _calls([_call(0, out_hi=P)])
    elif case == "mode_with_hi":
        sp = _spec(type_=0)
        calls = _calls([_call(4, out_hi=P)])
    elif case == "n_neg":
        n = -1
    elif case == "n_big":
        n, ws_bytes = INT32_MAX + 1, 1 << 62
    elif case == "null_key_col":
        sp.key[0].col = None
    elif case == "null_arg_col":
        sp.key[1].col = None
    elif case == "ws_short":
        ws_bytes = _ws(so, n, 5)[1] - 1
    elif case == "ws_null":
        ws = None
    elif case == "ws_misaligned":
        ws = P + 8
    elif case == "bad_call_in_last_slot":
        calls = _calls([_call(0)] * 7 + [_call(3, fraction=nan)])
    assert _ordered_agg(so, sp, ngroup, n, calls, ws_bytes, ws, first, ng) \
        == OTBX_ERR_INVALID

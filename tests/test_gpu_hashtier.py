"""GPU parity of the multi-key hash joins and hash aggregates
(otbx_join_i64_ext / _i64x2 / _i64n, otbx_agg_i64x2 / _i64n / _i64_dec)
against tests/hashtier_ref.py, at the shapes where the kernels change path:
the two flushes of the per-wave pair buffer, the second grid-stride
iteration, the overflow contract, NULL placement by join type, empty inputs,
group identity, the bounded first attempt of the aggregates and the int128
carry. test_hashtier_host.py pins the reference against the C oracle and
proves that each case reaches its branch.

Every comparison is exact: pair multisets as sorted lists, counts and int128
sums as integers, float sums bit for bit (the values are integer-valued with
|sum| < 2^53, so every order of the atomic adds gives the same bits). The one
non-finite case compares the class of the sum (NaN / +Inf) and the counts."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
import hashtier_ref as hr
from hashtier_ref import JOIN_TYPES

pytestmark = pytest.mark.gpu

ALL6 = ["inner", "left", "semi", "anti", "right", "full"]
OPS = ["ext", "x2", "n"]
NK_OF = {"ext": 1, "x2": 2, "n": 3}
SENTINEL = -7           # neither a row index nor the -1 of a fill


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


def dev(a):
    return None if a is None else \
        torch.from_numpy(np.ascontiguousarray(a)).cuda()


def devs(arrs, nk):
    return [None] * nk if arrs is None else [dev(a) for a in arrs]


def raw_join(ex, op, case, jt, cap, tail=0, fill=None):
    """The C entry point itself (otbx_join_i64_ext / _i64x2 / _i64n) with
    cap_pairs = cap. The output arrays are tail entries longer than cap and
    pre-filled with fill. Returns (status, *npairs_dev, out_b, out_p)."""
    L = _lib.lib()
    nk = case.nk
    bk, pk = devs(case.bcols, nk), devs(case.pcols, nk)
    bn, pn = devs(case.bnulls, nk), devs(case.pnulls, nk)

    def vp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    wsb = C.c_size_t(0)
    if op == "n":
        assert L.otbx_join_i64n_workspace_bytes(
            C.c_int64(case.nb), C.c_int64(case.np), C.byref(wsb)) == 0
    else:
        assert L.otbx_join_ext_workspace_bytes(
            C.c_int64(case.nb), C.c_int64(case.np), C.byref(wsb)) == 0
    ws = torch.empty(max(wsb.value, 1), dtype=torch.uint8, device="cuda")
    ob = torch.full((cap + tail,), 0 if fill is None else fill,
                    dtype=torch.int64, device="cuda")
    opp = torch.full((cap + tail,), 0 if fill is None else fill,
                     dtype=torch.int64, device="cuda")
    npairs = torch.zeros(1, dtype=torch.int64, device="cuda")
    common = (C.c_int32(jt), vp(ws), C.c_size_t(wsb.value), vp(ob), vp(opp),
              C.c_int64(cap), vp(npairs), ex._stream())
    if op == "ext":
        assert nk == 1
        st = L.otbx_join_i64_ext(vp(bk[0]), vp(bn[0]), C.c_int64(case.nb),
                                 vp(pk[0]), vp(pn[0]), C.c_int64(case.np),
                                 *common)
    elif op == "x2":
        assert nk == 2
        st = L.otbx_join_i64x2(vp(bk[0]), vp(bn[0]), vp(bk[1]), vp(bn[1]),
                               C.c_int64(case.nb), vp(pk[0]), vp(pn[0]),
                               vp(pk[1]), vp(pn[1]), C.c_int64(case.np),
                               *common)
    else:
        bks = ex._keyset_dev(bk, bn)
        pks = ex._keyset_dev(pk, pn)
        st = L.otbx_join_i64n(C.byref(bks), C.c_int64(case.nb), C.byref(pks),
                              C.c_int64(case.np), *common)
    torch.cuda.synchronize()
    return st, int(npairs.cpu().item()), ob.cpu().numpy(), opp.cpu().numpy()


def run_join(ex, op, case, jt_name):
    """Sorted pair list of one join through the host classes. The 1-key
    inner join of GpuHashJoin is otbx_join_i64, another operator, so the
    inner join of otbx_join_i64_ext is called directly. cap_pairs is the
    reference count plus slack; an overflow raises."""
    jt = JOIN_TYPES[jt_name]
    cap = len(case.ref(jt)) + 64
    nk = case.nk
    if op == "ext" and jt == 0:
        st, n, ob, opp = raw_join(ex, op, case, jt, cap)
        assert st == 0 and n <= cap, (st, n, cap)
        return sorted(zip(ob[:n].tolist(), opp[:n].tolist()))
    bk, pk = devs(case.bcols, nk), devs(case.pcols, nk)
    bn, pn = devs(case.bnulls, nk), devs(case.pnulls, nk)
    if op == "ext":
        assert nk == 1
        node = ex.GpuHashJoin(bk[0], pk[0], bn[0], pn[0], cap_pairs=cap,
                              join_type=jt_name)
    elif op == "x2":
        assert nk == 2
        node = ex.GpuHashJoin(bk[0], pk[0], bn[0], pn[0], cap_pairs=cap,
                              join_type=jt_name, build_keys2=bk[1],
                              probe_keys2=pk[1], build_null2=bn[1],
                              probe_null2=pn[1])
    else:
        node = ex.GpuHashJoinN(bk, pk, join_type=jt_name, bnulls=bn,
                               pnulls=pn, cap_pairs=cap)
    node.BeginCustomScan()
    pairs = node._run()
    node.EndCustomScan()
    return sorted(pairs)


def check_join(ex, op, case, jt_name):
    got = run_join(ex, op, case, jt_name)
    exp = case.ref(JOIN_TYPES[jt_name])
    assert len(got) == len(exp), (case.name, op, jt_name)
    assert got == exp, (case.name, op, jt_name)


def run_agg(ex, op, case):
    """{identity: (count_star, count_v, sum_isnull, sum)} of one aggregate
    through its host class; op is "x2", "n" or "dec"."""
    nk = case.nk
    keys = devs(case.keycols, nk)
    nulls = devs(case.keynulls, nk)
    vals, vn = dev(case.vals), dev(case.valnulls)
    if op == "x2":
        assert nk == 2
        node = ex.GpuHashAgg2(keys[0], keys[1], vals, key1_null=nulls[0],
                              key2_null=nulls[1], val_null=vn)
    elif op == "n":
        node = ex.GpuHashAggN(keys, vals, null_tensors=nulls, val_null=vn)
    else:
        assert nk == 1
        node = ex.GpuHashAggDec(keys[0], vals, key_null=nulls[0],
                                val_null=vn)
    node.BeginCustomScan()
    rows = node._run()
    node.EndCustomScan()
    out = {}
    for r in rows:
        if op == "x2":
            ident = tuple((bool(r[f"key{c}_isnull"]),
                           0 if r[f"key{c}_isnull"] else int(r[f"key{c}"]))
                          for c in (1, 2))
            s = float(r["sum_v"])
        elif op == "n":
            ri = int(r["row_idx"])
            assert 0 <= ri < case.n
            ident = case.identity(ri)          # row_idx is of its own group
            s = float(r["sum_v"])
        else:
            ident = ((bool(r["key_isnull"]),
                      0 if r["key_isnull"] else r["key"]),)
            hi, lo = r["sum_hi"], r["sum_lo"]
            assert -2**63 <= hi < 2**63 and 0 <= lo < 2**64   # hi is signed
            assert r["sum128"] == hi * 2**64 + lo
            s = r["sum128"]
        assert ident not in out, (case.name, op, ident)
        out[ident] = (int(r["count_star"]), int(r["count_v"]),
                      bool(r["sum_isnull"]), s)
    assert len(out) == len(rows)
    return out


def check_agg(ex, op, case):
    got = run_agg(ex, op, case)
    exp = case.ref()
    assert len(got) == len(exp), (case.name, op)
    assert set(got) == set(exp), (case.name, op)
    for ident, e in exp.items():
        cs, cv, isnull, s = got[ident]
        assert (cs, cv) == (e["count_star"], e["count_v"]), (case.name, ident)
        assert isnull == (e["count_v"] == 0), (case.name, ident)
        if e["count_v"]:
            assert hr.same_sum(s, e["sum"]), (case.name, op, ident, s,
                                              e["sum"])
    return got


# ---- 1. the flush inside the slot walk ----

@pytest.mark.parametrize("jt", ["inner", "left", "right", "full"])
@pytest.mark.parametrize("op", OPS)
def test_midwalk_flush(ex, op, jt):
    """1024 pairs per 64-row probe wave against a 512-pair buffer: the wave
    flushes in the middle of its slot walk and goes on buffering."""
    check_join(ex, op, hr.case_midwalk_flush(NK_OF[op]), jt)


# ---- 2. the flush before the post-walk fills ----

@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("jt", ["left", "full", "anti"])
@pytest.mark.parametrize("op", OPS)
def test_fill_flush(ex, op, jt, with_nulls):
    """496 buffered matches plus 33 fills in one wave: the buffer is flushed
    between the walk and the fills (left, full). Anti buffers only the 33
    fills here; its carried buffer is covered by test_join_grid_stride. The
    second variant makes eleven of the fills NULL-key probe rows over a
    stored key that exists on the build side."""
    check_join(ex, op, hr.case_fill_flush(NK_OF[op], with_nulls), jt)


# ---- 3. the second grid-stride iteration ----

@pytest.mark.parametrize("op,jt",
                         [("ext", jt) for jt in ALL6] +
                         [(op, jt) for op in ("x2", "n")
                          for jt in ("inner", "right", "anti")])
def test_join_grid_stride(ex, op, jt):
    """2048 * 256 + 64 + 37 probe rows: grid_for() (otbx_common.h) caps the
    grid at 2048 blocks of 256 threads, so the first two waves run a second
    iteration with the first one's pairs still buffered, the second of them
    ragged, and every other wave leaves through the all-out-of-range exit."""
    check_join(ex, op, hr.case_join_grid_stride(NK_OF[op]), jt)


@pytest.mark.parametrize("op", ["x2", "n", "dec"])
def test_agg_grid_stride(ex, op):
    """2048 * 256 + 101 rows (the same grid_for() cap): the build loops of
    k_agg2_build, k_aggn_build and k_dec_build run a second iteration."""
    check_agg(ex, op, hr.case_agg_grid_stride(op == "dec"))


# ---- 4. the overflow contract ----

@pytest.mark.parametrize("jt", ["inner", "full"])
@pytest.mark.parametrize("op", OPS)
def test_overflow_contract(ex, op, jt, monkeypatch):
    """include/otbx.h: *npairs_dev receives the TRUE count, at most
    cap_pairs entries are written, the call returns OTBX_OK, and the host
    classes raise. The arrays are 4096 entries longer than cap_pairs and
    pre-filled with a sentinel. The OTBX_JOINX_VIA_INNER=1 route of the
    1-key outer joins documents that its fills are incomplete on overflow;
    it is switched off here and not part of this test."""
    monkeypatch.delenv("OTBX_JOINX_VIA_INNER", raising=False)
    case = hr.case_overflow(NK_OF[op])
    exp = case.ref(JOIN_TYPES[jt])
    cap = hr.OVERFLOW_CAP
    assert len(exp) > cap
    st, n, ob, opp = raw_join(ex, op, case, JOIN_TYPES[jt], cap, tail=4096,
                              fill=SENTINEL)
    assert st == 0
    assert n == len(exp)
    assert np.all(ob[cap:] == SENTINEL) and np.all(opp[cap:] == SENTINEL)
    wb, wp = ob[:cap] != SENTINEL, opp[:cap] != SENTINEL
    assert np.array_equal(wb, wp)            # written together or not at all
    assert wb.any()
    written = collections.Counter(zip(ob[:cap][wb].tolist(),
                                      opp[:cap][wb].tolist()))
    assert not written - collections.Counter(exp)    # a sub-multiset
    nk = case.nk
    bk, pk = devs(case.bcols, nk), devs(case.pcols, nk)
    bn, pn = devs(case.bnulls, nk), devs(case.pnulls, nk)
    if op == "n":
        node = ex.GpuHashJoinN(bk, pk, join_type=jt, bnulls=bn, pnulls=pn,
                               cap_pairs=cap)
    elif op == "x2":
        node = ex.GpuHashJoin(bk[0], pk[0], bn[0], pn[0], cap_pairs=cap,
                              join_type=jt, build_keys2=bk[1],
                              probe_keys2=pk[1], build_null2=bn[1],
                              probe_null2=pn[1])
    else:
        node = ex.GpuHashJoin(bk[0], pk[0], bn[0], pn[0], cap_pairs=cap,
                              join_type=jt)
    node.BeginCustomScan()
    with pytest.raises(ex.OtbxError):
        node._run()


# ---- 5. join type by NULL placement ----

@pytest.mark.parametrize("jt", ALL6)
@pytest.mark.parametrize("mask", hr.X2_MASKS)
def test_null_placement_x2(ex, mask, jt):
    """NULL masks in turn on each of the four key columns and on all of
    them; a matching value under every NULL; INT64_MIN / INT64_MAX / -1 / 0
    as keys; (a, b) and (b, a) both present."""
    check_join(ex, "x2", hr.case_null_placement_x2(mask), jt)


@pytest.mark.parametrize("jt", ALL6)
@pytest.mark.parametrize("nk", [1, 2, 8])
def test_null_placement_n(ex, nk, jt):
    """masks on the last build column and on the probe side; with 8 keys,
    rows that differ only in column 7"""
    check_join(ex, "n", hr.case_null_placement_n(nk), jt)


# ---- 6. empty inputs ----

@pytest.mark.parametrize("jt", ALL6)
@pytest.mark.parametrize("which", hr.EMPTY_SIDES)
@pytest.mark.parametrize("op", ["x2", "n"])
def test_empty_join_side(ex, op, which, jt):
    """nb == 0, np == 0 and both (a zero-length tensor passes a NULL
    pointer): left / full / anti fill every probe row of an empty build
    side, right / full every build row of an empty probe side."""
    case = hr.case_empty(NK_OF[op], which)
    got = run_join(ex, op, case, jt)
    assert got == case.ref(JOIN_TYPES[jt])
    n = JOIN_TYPES[jt]
    if which == "build":
        assert len(got) == (case.np if n in (1, 3, 5) else 0)
    elif which == "probe":
        assert len(got) == (case.nb if n in (4, 5) else 0)
    else:
        assert got == []


@pytest.mark.parametrize("op,nk", [("x2", 2), ("n", 2), ("n", 8), ("dec", 1)])
def test_empty_agg_input(ex, op, nk):
    """GROUP BY over zero rows gives zero groups"""
    assert run_agg(ex, op, hr.case_agg_empty(nk, op == "dec")) == {}


# ---- 7. aggregate identity and NULLs ----

@pytest.mark.parametrize("op,nk", [("x2", 2), ("n", 2), ("n", 8)])
def test_agg_identity(ex, op, nk):
    """(NULL, 5), (5, NULL), (NULL, NULL), (0, 0), (NULL, 0) are five
    groups; garbage under a NULL does not split a group; INT64_MIN /
    INT64_MAX / -1 are ordinary keys; rows differing only in column 7 are
    distinct; an all-NULL-value group is sum_isnull with its count_star;
    +Inf and -Inf in one group give NaN, +Inf alone +Inf."""
    case = hr.case_agg_identity(nk)
    got = check_agg(ex, op, case)
    classes = sorted(c for c in (hr.sum_class(s) for _, cv, _, s in
                                 got.values() if cv) if c)
    assert classes == ["+inf", "nan"]
    assert sum(1 for _, _, isnull, _ in got.values() if isnull) == 1


# ---- 8. the bounded first attempt ----

@pytest.mark.parametrize("cap,ngroups", [(16, 5000), (4096, 100)])
@pytest.mark.parametrize("op", ["x2", "n", "dec"])
def test_bounded_attempt(ex, monkeypatch, op, cap, ngroups):
    """OTBX_NK_FORCE_CAP forces the size of the first-attempt table: 16
    slots for 5000 groups must abort and rerun against the full table, 4096
    slots for 100 groups succeed at once. Both against the reference."""
    monkeypatch.setenv("OTBX_NK_FORCE_CAP", str(cap))
    check_agg(ex, op, hr.case_agg_bounded(ngroups, op == "dec"))


# ---- 9. the int128 carry ----

def test_dec_carry(ex):
    """-1 + 1 and 1 - 1 (borrow and carry cancel), 4 x INT64_MIN,
    INT64_MAX + 1, 3 x -1, exactly +-2^64, 1000 alternating extremes: sum_hi
    (signed), sum_lo and the composed sum128 against Python ints."""
    case = hr.case_dec_carry()
    got = check_agg(ex, "dec", case)
    want = [0, 0, -2**65, 2**63, -3, 2**64, -2**64, -500]
    for g, s in enumerate(want):
        cs, cv, isnull, s128 = got[((False, g),)]
        assert (s128, cv, isnull) == (s, len(hr.DEC_CARRY_LISTS[g]), False)
        assert cs == cv + 2

"""CPU-side tests of the multi-key hash join / hash aggregate references.

tests/hashtier_ref.py (plain Python, written from include/otbx.h) and the C
oracle (oracle/oracle.c through oracle_py) are two independent restatements
of the same contract; they must agree on every case before either is held
against the GPU in tests/test_gpu_hashtier.py. The second half proves, from
the reference alone, that each case reaches the kernel branch it is named
for: the conditions are arithmetic on the reference result and the launch
geometry (64-lane waves, a 512-pair buffer per wave, at most 2048 x 256
threads per grid), so they hold without running a kernel."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_py as ora
from opentenbase_amd import _lib
import hashtier_ref as hr
from hashtier_ref import (GRID_THREADS, INT64_MAX, INT64_MIN, JOIN_TYPES,
                          PAIR_BUF, WAVE)

OTBX_ERR_INVALID = 3
ALL6 = ["inner", "left", "semi", "anti", "right", "full"]
STRIDE_SUBSET = ["inner", "right", "anti"]


def _join_cases():
    """(case builder args, join types) of every join case the GPU test runs"""
    out = []
    for nk in (1, 2, 3):
        out.append((hr.case_midwalk_flush, (nk,), ALL6))
        out.append((hr.case_fill_flush, (nk, False), ALL6))
        out.append((hr.case_fill_flush, (nk, True), ALL6))
        out.append((hr.case_join_grid_stride, (nk,),
                    ALL6 if nk == 1 else STRIDE_SUBSET))
        out.append((hr.case_overflow, (nk,), ["inner", "full"]))
    for mask in hr.X2_MASKS:
        out.append((hr.case_null_placement_x2, (mask,), ALL6))
    for nk in (1, 2, 8):
        out.append((hr.case_null_placement_n, (nk,), ALL6))
    for nk in (2, 3):
        for which in hr.EMPTY_SIDES:
            out.append((hr.case_empty, (nk, which), ALL6))
    return out


def _agg_cases():
    return [(hr.case_agg_grid_stride, (False,)),
            (hr.case_agg_grid_stride, (True,)),
            (hr.case_agg_identity, (2,)), (hr.case_agg_identity, (8,)),
            (hr.case_agg_bounded, (5000, False)),
            (hr.case_agg_bounded, (5000, True)),
            (hr.case_agg_bounded, (100, False)),
            (hr.case_agg_bounded, (100, True)),
            (hr.case_dec_carry, ()),
            (hr.case_agg_empty, (2, False)), (hr.case_agg_empty, (8, False)),
            (hr.case_agg_empty, (1, True))]


def _id(v):
    b, args = v[0], v[1]
    return b.__name__[5:] + "-" + "-".join(str(a) for a in args)


# ------------------------------------------------- reference == C oracle

@pytest.mark.parametrize("spec", _join_cases(), ids=_id)
def test_ref_join_equals_oracle(spec):
    builder, args, jts = spec
    case = builder(*args)
    for name in jts:
        jt = JOIN_TYPES[name]
        exp = case.ref(jt)
        obi, opi = ora.join_i64n(case.bcols, case.pcols, jt,
                                 bnull_cols=case.bnulls,
                                 pnull_cols=case.pnulls)
        assert sorted(zip(obi.tolist(), opi.tolist())) == exp, \
            (case.name, name, "join_i64n")
        if case.nk > 2:
            continue
        bn = case.bnulls or [None] * case.nk
        pn = case.pnulls or [None] * case.nk
        two = case.nk == 2
        obi, opi = ora.join_ext(
            case.bcols[0], case.pcols[0], jt, bnull=bn[0], pnull=pn[0],
            bkeys2=case.bcols[1] if two else None,
            pkeys2=case.pcols[1] if two else None,
            bnull2=bn[1] if two else None, pnull2=pn[1] if two else None)
        assert sorted(zip(obi.tolist(), opi.tolist())) == exp, \
            (case.name, name, "join_ext")


@pytest.mark.parametrize("spec", _agg_cases(), ids=_id)
def test_ref_agg_equals_oracle(spec):
    builder, args = spec
    case = builder(*args)
    exp = case.ref()
    nulls = case.keynulls or [None] * case.nk
    if case.vals.dtype == np.int64:
        got = ora.agg_i64_dec(case.keycols[0], case.vals, key_null=nulls[0],
                              val_null=case.valnulls)
        assert len(got) == len(exp)
        for o in got:
            e = exp[((bool(o.key_isnull), 0 if o.key_isnull else o.key),)]
            assert (o.count_star, o.count_v) == (e["count_star"],
                                                 e["count_v"])
            assert bool(o.sum_isnull) == (e["count_v"] == 0)
            if e["count_v"]:
                assert o.sum128 == e["sum"], (case.name, o.key)
        return
    got = ora.agg_i64n(case.keycols, case.vals, null_cols=nulls,
                       val_null=case.valnulls)
    assert len(got) == len(exp)
    assert len({case.identity(o.row_idx) for o in got}) == len(got)
    for o in got:
        e = exp[case.identity(o.row_idx)]
        assert o.row_idx == e["first_row"]      # the oracle scans in order
        assert (o.count_star, o.count_v) == (e["count_star"], e["count_v"])
        assert bool(o.sum_isnull) == (e["count_v"] == 0)
        if e["count_v"]:
            assert hr.same_sum(o.sum_v, e["sum"]), (case.name, o.row_idx)
    if case.nk != 2:
        return
    got = ora.agg_i64x2(case.keycols[0], case.keycols[1], case.vals,
                        k1null=nulls[0], k2null=nulls[1],
                        val_null=case.valnulls)
    assert len(got) == len(exp)
    seen = set()
    for o in got:
        ident = ((bool(o.key1_isnull), 0 if o.key1_isnull else o.key1),
                 (bool(o.key2_isnull), 0 if o.key2_isnull else o.key2))
        seen.add(ident)
        e = exp[ident]
        assert (o.count_star, o.count_v) == (e["count_star"], e["count_v"])
        assert bool(o.sum_isnull) == (e["count_v"] == 0)
        if e["count_v"]:
            assert hr.same_sum(o.sum_v, e["sum"]), (case.name, ident)
    assert len(seen) == len(got)


def test_ref_join_hand_case():
    """the header's pair encoding on six rows, by hand"""
    b = [np.array([1, 2, 2, 9], dtype=np.int64)]
    bn = [np.array([0, 0, 0, 1], dtype=np.uint8)]
    p = [np.array([2, 3, 9, 1], dtype=np.int64)]
    pn = [np.array([0, 0, 0, 1], dtype=np.uint8)]    # NULL over a matching 1
    assert hr.ref_join(b, bn, p, pn, 0) == [(1, 0), (2, 0)]
    assert hr.ref_join(b, bn, p, pn, 1) == [(-1, 1), (-1, 2), (-1, 3),
                                            (1, 0), (2, 0)]
    assert hr.ref_join(b, bn, p, pn, 2) == [(-1, 0)]
    assert hr.ref_join(b, bn, p, pn, 3) == [(-1, 1), (-1, 2), (-1, 3)]
    assert hr.ref_join(b, bn, p, pn, 4) == [(0, -1), (1, 0), (2, 0), (3, -1)]
    assert hr.ref_join(b, bn, p, pn, 5) == [(-1, 1), (-1, 2), (-1, 3),
                                            (0, -1), (1, 0), (2, 0), (3, -1)]


def test_ref_agg_hand_case():
    k = [np.array([5, 7, 5, 7], dtype=np.int64),
         np.array([1, 2, 3, 4], dtype=np.int64)]
    kn = [None, np.array([1, 0, 1, 0], dtype=np.uint8)]
    v = np.array([1.0, 2.0, 4.0, 8.0])
    vn = np.array([0, 1, 0, 0], dtype=np.uint8)
    assert hr.ref_agg(k, kn, v, vn) == {
        ((False, 5), (True, 0)): {"count_star": 2, "count_v": 2, "sum": 5.0,
                                  "first_row": 0},
        ((False, 7), (False, 2)): {"count_star": 1, "count_v": 0, "sum": 0.0,
                                   "first_row": 1},
        ((False, 7), (False, 4)): {"count_star": 1, "count_v": 1, "sum": 8.0,
                                   "first_row": 3}}
    d = hr.ref_agg(k[:1], None, np.array([INT64_MAX, 1, INT64_MAX, 2]), None)
    assert d[((False, 5),)]["sum"] == 2 * INT64_MAX
    assert isinstance(d[((False, 7),)]["sum"], int)


# ------------------------------- each case reaches the branch it is named for

@pytest.mark.parametrize("nk", [1, 2, 3])
@pytest.mark.parametrize("jt", ["inner", "left", "right", "full"])
def test_midwalk_case_overflows_every_wave(nk, jt):
    """A wave serves 64 consecutive probe rows of one loop iteration and
    buffers 512 pairs; a 64-row block with more than 512 match pairs cannot
    finish its slot walk without the mid-walk flush."""
    case = hr.case_midwalk_flush(nk)
    assert case.np % WAVE == 0 and case.np <= GRID_THREADS
    matches, _ = hr.block_counts(case.ref(JOIN_TYPES[jt]), case.np)
    assert len(matches) == case.np // WAVE == 2
    assert all(m > PAIR_BUF for m in matches), matches
    assert matches == [1024, 1024]


@pytest.mark.parametrize("nk", [1, 2, 3])
@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("jt", ["left", "full"])
def test_fill_case_overflows_only_at_the_fills(nk, with_nulls, jt):
    """One wave: its matches fit the buffer (no mid-walk flush, which
    triggers only when a step would exceed 512), matches + fills do not, so
    the flush before the post-walk fills runs with a non-empty buffer."""
    case = hr.case_fill_flush(nk, with_nulls)
    assert case.np == WAVE
    matches, fills = hr.block_counts(case.ref(JOIN_TYPES[jt]), case.np)
    assert matches == [496] and fills == [33]
    assert matches[0] <= PAIR_BUF < matches[0] + fills[0]
    # anti buffers fills only: 33 of them, no flush at this size; its
    # carried-buffer coverage is the grid-stride case
    _, afills = hr.block_counts(case.ref(JOIN_TYPES["anti"]), case.np)
    assert afills == [33]
    if with_nulls:
        nullrows = np.flatnonzero(np.bitwise_or.reduce(
            [m for m in case.pnulls if m is not None]))
        assert len(nullrows) == 11
        _assert_nulls_hide_matches(case)


def _assert_nulls_hide_matches(case):
    """every NULL-key row stores key values that match when the masks are
    dropped, and matches nothing with them"""
    bare = hr.ref_join(case.bcols, None, case.pcols, None, 0)
    with_masks = case.ref(0)
    bare_b = {b for b, _ in bare}
    bare_p = {p for _, p in bare}
    got_b = {b for b, _ in with_masks}
    got_p = {p for _, p in with_masks}
    for side, masks, bare_rows, got_rows in (
            ("build", case.bnulls, bare_b, got_b),
            ("probe", case.pnulls, bare_p, got_p)):
        if masks is None:
            continue
        anynull = np.bitwise_or.reduce([m for m in masks if m is not None])
        rows = np.flatnonzero(anynull).tolist()
        assert rows, (case.name, side)
        assert set(rows) <= bare_rows, (case.name, side)
        assert not (set(rows) & got_rows), (case.name, side)


@pytest.mark.parametrize("nk", [1, 2, 3])
def test_join_stride_case_needs_a_second_iteration(nk):
    case = hr.case_join_grid_stride(nk)
    extra = case.np - GRID_THREADS
    assert extra == WAVE + 37                 # one full wave, one ragged
    assert case.nb <= GRID_THREADS
    for jt, want_match, want_fill in (("inner", True, False),
                                      ("anti", False, True)):
        pairs = case.ref(JOIN_TYPES[jt])
        tail = [(b, p) for b, p in pairs if p >= GRID_THREADS]
        head0 = [(b, p) for b, p in pairs if 0 <= p < WAVE]
        # the wave of rows 0..63 also serves rows GRID_THREADS..+63: it
        # enters the second iteration with pairs of the first in its buffer
        assert head0 and tail
        assert any(b >= 0 for b, _ in tail) == want_match
        assert any(b < 0 for b, _ in tail) == want_fill
        # both second-iteration waves emit, the ragged one included
        assert any(p >= GRID_THREADS + WAVE for _, p in tail)
    absent = 1 - len({p for _, p in case.ref(2)}) / case.np
    assert 0.25 < absent < 0.45               # "about a third"


@pytest.mark.parametrize("dec", [False, True])
def test_agg_stride_case_needs_a_second_iteration(dec):
    case = hr.case_agg_grid_stride(dec)
    assert case.n == GRID_THREADS + 101
    ref = case.ref()
    assert 2000 < len(ref) < 5000
    assert any(any(isn for isn, _ in ident) for ident in ref)
    assert any(g["count_v"] < g["count_star"] for g in ref.values())
    tail = {case.identity(i) for i in range(GRID_THREADS, case.n)}
    assert len(tail) > 50                     # rows of the second iteration
    if not dec:
        mag = np.abs(case.vals).sum()
        assert mag < 2**53 and np.all(case.vals == np.rint(case.vals))


@pytest.mark.parametrize("nk", [1, 2, 3])
@pytest.mark.parametrize("jt", ["inner", "full"])
def test_overflow_case_exceeds_cap(nk, jt):
    """cap_pairs is far below the true count, and the true count is below
    cap_pairs + 4096: a kernel that ignored cap_pairs would write into the
    sentinel tail of the test's arrays, not past them."""
    case = hr.case_overflow(nk)
    n = len(case.ref(JOIN_TYPES[jt]))
    assert n > 6 * hr.OVERFLOW_CAP
    assert n < hr.OVERFLOW_CAP + 4096
    if jt == "full":
        pairs = case.ref(5)
        assert any(b < 0 for b, _ in pairs) and any(p < 0 for _, p in pairs)
        assert n > len(case.ref(0))


@pytest.mark.parametrize("mask", hr.X2_MASKS)
def test_null_x2_case_properties(mask):
    case = hr.case_null_placement_x2(mask)
    assert case.nb == case.np == 200
    for cols in (case.bcols, case.pcols):
        rows = set(zip(cols[0].tolist(), cols[1].tolist()))
        assert {(INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (-1, 0),
                (0, -1), (0, 0), (INT64_MIN, INT64_MIN)} <= rows
    masked = {"b1": (0,), "b2": (1,), "p1": (2,), "p2": (3,),
              "all": (0, 1, 2, 3)}[mask]
    have = [m is not None for m in (case.bnulls or [None, None]) +
            (case.pnulls or [None, None])]
    assert have == [i in masked for i in range(4)]
    _assert_nulls_hide_matches(case)
    assert len(case.ref(0)) > 200             # NULLs leave plenty of matches


@pytest.mark.parametrize("nk", [1, 2, 8])
def test_null_n_case_properties(nk):
    case = hr.case_null_placement_n(nk)
    assert case.nk == nk and case.nb == case.np == 200
    assert case.bnulls[nk - 1] is not None and case.pnulls[nk - 1] is not None
    assert all(m is None for m in case.bnulls[:nk - 1])
    _assert_nulls_hide_matches(case)
    last = set(case.bcols[nk - 1].tolist())
    assert {INT64_MIN, INT64_MAX, -1, 0} <= last
    if nk == 8:
        for cols in (case.bcols, case.pcols):
            head = set(zip(*[c.tolist() for c in cols[:7]]))
            assert len(head) == 2             # differ in column 0 only
            full = set(zip(*[c.tolist() for c in cols]))
            a = [r for r in full if r[:7] == min(head)]
            assert len(a) == 6                # ... or in column 7 only


@pytest.mark.parametrize("nk", [2, 3])
def test_empty_join_fills(nk):
    """an empty build side fills every probe row of left/full/anti; an empty
    probe side fills every build row of right/full; nothing else comes out"""
    eb = hr.case_empty(nk, "build")
    ep = hr.case_empty(nk, "probe")
    for jt in range(6):
        assert eb.ref(jt) == ([(-1, p) for p in range(eb.np)]
                              if jt in (1, 3, 5) else [])
        assert ep.ref(jt) == ([(b, -1) for b in range(ep.nb)]
                              if jt in (4, 5) else [])
        assert hr.case_empty(nk, "both").ref(jt) == []


@pytest.mark.parametrize("nk", [2, 8])
def test_agg_identity_case_properties(nk):
    case = hr.case_agg_identity(nk)
    ref = case.ref()
    mid = tuple((False, int(c[0])) for c in case.keycols[1:-1])

    def ident(a, b):
        f = lambda x: (True, 0) if x is None else (False, x)   # noqa: E731
        return (f(a),) + mid + (f(b),)

    five = [ident(None, 5), ident(5, None), ident(None, None), ident(0, 0),
            ident(None, 0)]
    assert len(set(five)) == 5 and all(i in ref for i in five)
    for a, b in ((INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (-1, -1),
                 (INT64_MIN, INT64_MIN)):
        assert ident(a, b) in ref
    assert len(ref) == 16
    # different garbage under the NULLs of one group
    first = case.keycols[0]
    rows = [i for i in range(case.n) if case.identity(i) == ident(None, 5)]
    assert len({int(first[i]) for i in rows}) > 1
    g = ref[ident(1, 1)]
    assert g["count_v"] == 0 and g["count_star"] > 1
    assert hr.sum_class(ref[ident(2, 2)]["sum"]) == "nan"
    assert hr.sum_class(ref[ident(3, 3)]["sum"]) == "+inf"
    if nk == 8:
        assert all(len(set(c.tolist())) == 1 for c in case.keycols[1:7])


@pytest.mark.parametrize("dec", [False, True])
def test_bounded_cases_abort_or_fit(dec):
    """A 16-slot first table cannot hold more than 16 groups: a row of a
    17th group walks a full table until the 128-step bound aborts the
    attempt. With fewer than 128 groups no walk can be longer than the number
    of occupied slots plus one, so a 4096-slot attempt never aborts."""
    assert len(hr.case_agg_bounded(5000, dec).ref()) > 16 * 100
    assert len(hr.case_agg_bounded(100, dec).ref()) < 128
    assert hr.case_agg_bounded(5000, dec).n == 20000


def test_dec_carry_case_sums():
    case = hr.case_dec_carry()
    ref = case.ref()
    want = [0, 0, -2**65, 2**63, -3, 2**64, -2**64, -500]
    assert [sum(lst) for lst in hr.DEC_CARRY_LISTS] == want
    assert len(hr.DEC_CARRY_LISTS[-1]) == 1000
    for g, s in enumerate(want):
        e = ref[((False, g),)]
        assert e["sum"] == s
        assert e["count_v"] == len(hr.DEC_CARRY_LISTS[g])
        assert e["count_star"] == e["count_v"] + 2


# --------------------------------------------------- entry checks (host code)

@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def test_null_column_with_rows_is_invalid(so):
    """The n == 0 rule of the entry points only relaxes EMPTY inputs: a NULL
    key column with a row count > 0 is still OTBX_ERR_INVALID, decided
    before any HIP call (the zero-row side is tested on the GPU)."""
    fake = C.c_void_p(4096)          # non-NULL, never dereferenced
    i64, i32, sz = C.c_int64, C.c_int32, C.c_size_t
    assert so.otbx_agg_i64x2(None, None, fake, None, fake, None, i64(5),
                             fake, sz(1 << 30), fake, fake, None) \
        == OTBX_ERR_INVALID
    assert so.otbx_agg_i64x2(fake, None, None, None, fake, None, i64(5),
                             fake, sz(1 << 30), fake, fake, None) \
        == OTBX_ERR_INVALID
    assert so.otbx_agg_i64_dec(None, None, fake, None, i64(5), fake,
                               sz(1 << 30), fake, fake, None) \
        == OTBX_ERR_INVALID
    assert so.otbx_agg_i64_dec(fake, None, None, None, i64(5), fake,
                               sz(1 << 30), fake, fake, None) \
        == OTBX_ERR_INVALID
    ks = _lib.KeysetDev()
    ks.nkeys = 2
    ks.keys[0] = 4096                # keys[1] stays NULL
    full = _lib.KeysetDev()
    full.nkeys = 2
    full.keys[0] = full.keys[1] = 4096
    assert so.otbx_agg_i64n(C.byref(ks), fake, None, i64(5), fake,
                            sz(1 << 30), fake, fake, None) == OTBX_ERR_INVALID
    assert so.otbx_agg_i64n(C.byref(full), None, None, i64(5), fake,
                            sz(1 << 30), fake, fake, None) == OTBX_ERR_INVALID
    for nb, npr, bks, pks in ((5, 0, ks, full), (0, 5, full, ks)):
        assert so.otbx_join_i64n(C.byref(bks), i64(nb), C.byref(pks),
                                 i64(npr), i32(0), fake, sz(1 << 30), fake,
                                 fake, i64(64), fake, None) \
            == OTBX_ERR_INVALID
    # nkeys is checked whatever the row counts are
    bad = _lib.KeysetDev()
    bad.nkeys = 9
    assert so.otbx_join_i64n(C.byref(bad), i64(0), C.byref(bad), i64(0),
                             i32(0), fake, sz(1 << 30), fake, fake, i64(64),
                             fake, None) == OTBX_ERR_INVALID
    assert so.otbx_agg_i64n(C.byref(bad), None, None, i64(0), fake,
                            sz(1 << 30), fake, fake, None) == OTBX_ERR_INVALID
    for nb, npr, bk2, pk2 in ((5, 0, None, fake), (0, 5, fake, None)):
        assert so.otbx_join_i64x2(fake, None, bk2, None, i64(nb), fake, None,
                                  pk2, None, i64(npr), i32(0), fake,
                                  sz(1 << 30), fake, fake, i64(64), fake,
                                  None) == OTBX_ERR_INVALID

"""CPU-side tests of the generic Sort operator's host layers: the two
reference orderings agree, workspace sizing and argument checks of
otbx_sort_perm (pure host code — no HIP call is reached), the GpuSort spec
builder, and the Coordinator merge of sorted streams over gloo."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd import fragment
from opentenbase_amd._lib import SortSpecDev
from sort_ref import cmp_perm, ref_perm

OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def special_f64(rng, n):
    bits = np.array([0x7ff8000000000000, 0xfff8000000000000,  # +/- quiet NaN
                     0x7ff0000000000001, 0xfff00000deadbeef,  # signalling
                     0x7fffffffffffffff], dtype=np.uint64).view(np.float64)
    vals = np.concatenate([
        bits, [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308,
               np.finfo(np.float64).max, -np.finfo(np.float64).max,
               1.0, -1.0, 1.5, 3.0]])
    return vals[rng.integers(0, len(vals), n)]


def special_i64(rng, n):
    vals = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1,
                     2**32, -2**32, 2**31 - 1, 255], dtype=np.int64)
    return vals[rng.integers(0, len(vals), n)]


def test_ref_perm_equals_comparator_sort_all_flag_combinations():
    rng = np.random.default_rng(7)
    n = 3000
    u8 = rng.integers(0, 3, n).astype(np.uint8)
    f64 = special_f64(rng, n)
    f64_null = (rng.random(n) < 0.2).astype(np.uint8)
    i64 = special_i64(rng, n)
    i64_null = (rng.random(n) < 0.2).astype(np.uint8)
    i32 = rng.choice(np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max,
                               0, -7, 7], dtype=np.int32), n)
    for bits in range(16):
        # bit 0/1: f64 DESC / NULLS FIRST; bit 2/3: i64 DESC / NULLS FIRST;
        # the two non-nullable keys take the directions as well
        d1, nf1 = bool(bits & 1), bool(bits & 2)
        d2, nf2 = bool(bits & 4), bool(bits & 8)
        spec = [(u8, None, d2, nf1), (f64, f64_null, d1, nf1),
                (i64, i64_null, d2, nf2), (i32, None, d1, nf2)]
        a, b = ref_perm(spec), cmp_perm(spec)
        assert np.array_equal(a, b), bits
        assert np.array_equal(np.sort(a), np.arange(n))


def test_null_placement_is_independent_of_desc():
    col = np.array([3, 1, 2, 9], dtype=np.int64)
    nulls = np.array([0, 0, 0, 1], dtype=np.uint8)
    assert ref_perm([(col, nulls, False, False)]).tolist() == [1, 2, 0, 3]
    assert ref_perm([(col, nulls, True, False)]).tolist() == [0, 2, 1, 3]
    assert ref_perm([(col, nulls, False, True)]).tolist() == [3, 1, 2, 0]
    assert ref_perm([(col, nulls, True, True)]).tolist() == [3, 0, 2, 1]


def _ws(so, n, nkeys=1, limit=0):
    out = C.c_size_t(0)
    st = so.otbx_sort_workspace_bytes(n, nkeys, limit, C.byref(out))
    return st, out.value


def test_sort_workspace_sizing(so):
    prev = 0
    for n in (0, 1, 1000, 10**6, 6 * 10**8):
        st, b = _ws(so, n)
        assert st == 0
        assert b >= prev
        if n > 0:
            assert b > 0
        prev = b
    # 8 B key + 4 B row id, ping-pong: at least 24 B/row
    assert _ws(so, 10**6)[1] >= 24 * 10**6
    prev = 0
    for nk in range(1, 9):
        st, b = _ws(so, 10**6, nk)
        assert st == 0 and b >= prev
        prev = b
    for lim in (0, 10, 10**6, 10**7):
        assert _ws(so, 10**6, 2, lim)[0] == 0
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX)[0] == 0
    assert _ws(so, 10, 0)[0] == OTBX_ERR_INVALID
    assert _ws(so, 10, 9)[0] == OTBX_ERR_INVALID
    assert _ws(so, 10, 1, -1)[0] == OTBX_ERR_INVALID


def _spec(nkeys=1, type_=0, flags=0, col=0x1000):
    sp = SortSpecDev()
    sp.nkeys = nkeys
    for c in range(min(max(nkeys, 0), 8)):
        sp.key[c].col = col
        sp.key[c].nulls = None
        sp.key[c].type = type_
        sp.key[c].flags = flags
    return sp


def _sort(so, sp, n, limit=0, ws_bytes=None):
    """otbx_sort_perm with dummy (never dereferenced) device pointers: every
    case here must be rejected before any HIP call."""
    if ws_bytes is None:
        st, ws_bytes = _ws(so, max(min(n, INT32_MAX), 0))
        assert st == 0
    return so.otbx_sort_perm(C.byref(sp), C.c_int64(n), C.c_int64(limit),
                             C.c_void_p(0x1000), C.c_size_t(ws_bytes),
                             C.c_void_p(0x1000), C.c_void_p(0x1000), None)


@pytest.mark.parametrize("case", [
    "nkeys0", "nkeys9", "type_neg", "type4", "flags4", "flags_neg", "n_neg",
    "n_big", "limit_neg", "null_col", "ws_short", "null_spec"])
def test_sort_invalid_arguments(so, case):
    n, limit, ws = 100, 0, None
    sp = _spec()
    if case == "nkeys0":
        sp = _spec(nkeys=0)
    elif case == "nkeys9":
        sp = _spec(nkeys=9)
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
        n = INT32_MAX + 1
        ws = 1 << 62
    elif case == "limit_neg":
        limit = -1
    elif case == "null_col":
        sp = _spec(col=None)
    elif case == "ws_short":
        ws = _ws(so, n)[1] - 1
    if case == "null_spec":
        st = so.otbx_sort_perm(None, C.c_int64(n), C.c_int64(0),
                               C.c_void_p(0x1000), C.c_size_t(1 << 30),
                               C.c_void_p(0x1000), C.c_void_p(0x1000), None)
    else:
        st = _sort(so, sp, n, limit, ws)
    assert st == OTBX_ERR_INVALID


def test_sort_bad_key_in_later_column_is_rejected(so):
    sp = _spec(nkeys=3)
    sp.key[2].type = 7
    assert _sort(so, sp, 10) == OTBX_ERR_INVALID
    sp = _spec(nkeys=3)
    sp.key[1].col = None
    assert _sort(so, sp, 10) == OTBX_ERR_INVALID


def test_gpusort_default_nulls_first_rule_and_spec():
    a = torch.zeros(5, dtype=torch.float64)
    b = torch.zeros(5, dtype=torch.int32)
    c = torch.zeros(5, dtype=torch.uint8)
    d = torch.zeros(5, dtype=torch.int64)
    nm = torch.zeros(5, dtype=torch.uint8)
    # SQL default: ASC -> NULLS LAST, DESC -> NULLS FIRST
    node = ex.GpuSort([a, b, c, d], descending=[True, False, True, False],
                      nulls=[None, nm, None, None], limit=7)
    sp = node.spec()
    assert sp.nkeys == 4
    assert [sp.key[i].type for i in range(4)] == [1, 2, 3, 0]
    assert [sp.key[i].flags for i in range(4)] == [1 | 2, 0, 1 | 2, 0]
    assert sp.key[0].col == a.data_ptr() and sp.key[3].col == d.data_ptr()
    assert sp.key[0].nulls is None and sp.key[1].nulls == nm.data_ptr()
    assert node.limit == 7 and node.explain() is None
    # explicit placement overrides the default, entry by entry
    node = ex.GpuSort([a, b], descending=[True, False],
                      nulls_first=[False, None])
    assert node.flags == [1, 0]
    node = ex.GpuSort([a, b], descending=[False, True],
                      nulls_first=[True, False])
    assert node.flags == [2, 1]
    assert ex.GpuSort([d]).flags == [0]
    with pytest.raises(_lib.OtbxError):
        ex.GpuSort([])
    with pytest.raises(_lib.OtbxError):
        ex.GpuSort([torch.zeros(3, dtype=torch.float32)])
    with pytest.raises(_lib.OtbxError):
        ex.GpuSort([a, b], descending=[True])


# ---- Coordinator merge over gloo ----

DESC = [True, False, False]
NFIRST = [False, None, True]     # middle key: the SQL default (ASC -> LAST)
NFIRST_RESOLVED = [False, False, True]


def _rank_rows(rank, limit, empty_rank=None):
    """This rank's locally sorted rows: (f64 DESC NULLS LAST, i32 ASC,
    nullable i64 ASC NULLS FIRST) + an int64 payload naming (rank, row).
    Low-cardinality keys, so ranks tie with each other."""
    rng = np.random.default_rng(100 + rank)
    n = 0 if rank == empty_rank else 400 + 37 * rank
    k0 = rng.choice(np.array([1.5, -0.0, 0.0, np.nan, np.inf, 2.0]), n)
    k0n = (rng.random(n) < 0.2).astype(np.uint8)
    k1 = rng.integers(-2, 2, n).astype(np.int32)
    k2 = rng.integers(0, 3, n).astype(np.int64)
    k2n = (rng.random(n) < 0.3).astype(np.uint8)
    pay = rank * 1_000_000 + np.arange(n, dtype=np.int64)
    spec = [(k0, k0n, DESC[0], NFIRST_RESOLVED[0]),
            (k1, None, DESC[1], NFIRST_RESOLVED[1]),
            (k2, k2n, DESC[2], NFIRST_RESOLVED[2])]
    p = ref_perm(spec)
    if limit:
        p = p[:limit]
    return [k0[p], k1[p], k2[p]], [k0n[p], None, k2n[p]], pay[p]


def _expected(world, limit, empty_rank):
    parts = [_rank_rows(r, limit, empty_rank) for r in range(world)]
    keys = [np.concatenate([p[0][c] for p in parts]) for c in range(3)]
    nulls = [np.concatenate([p[1][0] for p in parts]), None,
             np.concatenate([p[1][2] for p in parts])]
    pay = np.concatenate([p[2] for p in parts])
    perm = ref_perm([(keys[c], nulls[c], DESC[c], NFIRST_RESOLVED[c])
                     for c in range(3)])
    if limit:
        perm = perm[:limit]
    return [k[perm] for k in keys], \
        [None if m is None else m[perm] for m in nulls], pay[perm]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _worker_sort(rank, world, port, q, limit, empty_rank):
    from opentenbase_amd import fragment as frag
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    keys, nulls, pay = _rank_rows(rank, limit, empty_rank)
    gk, gp, gn = frag.merge_sorted_partials(
        [_t(k) for k in keys], [_t(pay)], DESC, NFIRST,
        [_t(m) for m in nulls], limit)
    if rank == 0:
        q.put(([k.numpy().tobytes() for k in gk], gp[0].numpy().tobytes(),
               [None if m is None else m.numpy().tobytes() for m in gn]))
    torch.distributed.destroy_process_group()


def _run(worker, args, world=2):
    # fresh port per attempt: a lingering TIME_WAIT on a reused MASTER_PORT
    # can fail the rendezvous
    last = None
    for attempt in range(3):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = 33711 + np.random.randint(0, 2000)
        procs = [ctx.Process(target=worker, args=(r, world, port, q) + args)
                 for r in range(world)]
        for p in procs:
            p.start()
        try:
            res = q.get(timeout=120)
        except Exception as e:
            last = e
            for p in procs:
                p.terminate()
                p.join(timeout=30)
            continue
        ok = True
        for p in procs:
            p.join(timeout=60)
            ok = ok and p.exitcode == 0
        if ok:
            return res
        last = AssertionError([p.exitcode for p in procs])
    raise last


@pytest.mark.timeout(180)
@pytest.mark.parametrize("limit,empty_rank", [(0, None), (50, None), (0, 1),
                                              (50, 0)])
def test_merge_sorted_partials_two_ranks(limit, empty_rank):
    gk, gp, gn = _run(_worker_sort, (limit, empty_rank))
    ek, en, ep = _expected(2, limit, empty_rank)
    # bit-equal (tobytes: NaN payloads and the sign of zero included)
    for c in range(3):
        assert gk[c] == ek[c].tobytes(), c
    assert gp == ep.tobytes()
    assert gn[1] is None
    assert gn[0] == en[0].tobytes() and gn[2] == en[2].tobytes()
    pay = np.frombuffer(gp, dtype=np.int64)
    assert len(pay) == (limit if limit else len(ep))
    if empty_rank is None:
        # cross-rank ties: both ranks contribute, and rows equal on every
        # key keep rank order (rank 0's rows first)
        assert (pay < 1_000_000).any() and (pay >= 1_000_000).any()


def test_merge_sorted_partials_single_rank_is_identity():
    assert not fragment.is_dist()
    keys, nulls, pay = _rank_rows(0, 0)
    tk, tn, tp = [_t(k) for k in keys], [_t(m) for m in nulls], [_t(pay)]
    gk, gp, gn = fragment.merge_sorted_partials(tk, tp, DESC, NFIRST, tn, 0)
    assert all(a is b for a, b in zip(gk, tk))
    assert gp[0] is tp[0]
    assert all(a is b for a, b in zip(gn, tn))


def test_host_normalisation_matches_reference():
    """fragment's numpy key mapping (the gloo merge path) against the
    comparator sort, on the special values."""
    rng = np.random.default_rng(3)
    n = 800
    f = special_f64(rng, n)
    fn = (rng.random(n) < 0.25).astype(np.uint8)
    i = special_i64(rng, n)
    for desc, nf in itertools.product([False, True], repeat=2):
        cols = []
        for col, nl in ((i, None), (f, fn)):     # f64 primary, i64 second
            nd, k = fragment._sort_norm_host(col, (1 if desc else 0) |
                                             (2 if nf else 0), nl)
            cols += [k, nd]
        got = np.lexsort(cols)
        exp = cmp_perm([(f, fn, desc, nf), (i, None, desc, nf)])
        assert np.array_equal(got, exp)

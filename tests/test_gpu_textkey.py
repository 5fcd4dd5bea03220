"""GPU parity of the text rank (otbx_text_rank / GpuTextRank / GpuText.rank)
and of text keys flowing through the unchanged Sort, GroupAggregate, hash
aggregate, hash join and WindowAgg nodes as int64 codes. Everything is exact,
against the row-loop references of tests/textkey_ref.py."""
import json
import os

import numpy as np
import pytest
import torch

from sort_ref import ref_perm
from textkey_ref import column_rows, rank_cmp, rank_set, text_sort_perm
from window_ref import ref_window

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, TXT_TILE, SS_TILE = 64, 256, 6144
SIZES = (0, 1, WAVE - 1, WAVE, WAVE + 1, TXT_TILE - 1, TXT_TILE, TXT_TILE + 1,
         SS_TILE - 1, SS_TILE, SS_TILE + 1, 3 * SS_TILE + 17)
ALPHABET = b"\0ab\xff"


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(REPO, "tests", "golden",
                           "text_order_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def random_rows(rng, n, null_frac=0.01, maxlen=40):
    """4-symbol alphabet, lengths 0..maxlen: every row is a prefix of one of
    eight base strings, a third of them with the last byte changed — heavy
    duplication and deep shared prefixes"""
    a = np.frombuffer(ALPHABET, dtype=np.uint8)
    bases = [a[rng.integers(0, 4, maxlen)].tobytes() for _ in range(8)]
    rows = []
    for _ in range(n):
        if rng.random() < null_frac:
            rows.append(None)
            continue
        r = bytearray(bases[rng.integers(0, 8)][:rng.integers(0, maxlen + 1)])
        if r and rng.random() < 0.33:
            r[-1] = ALPHABET[rng.integers(0, 4)]
        rows.append(bytes(r))
    return rows


def adopt(ex, raw, offs, nulls=None, skip=0):
    """a GpuText over given bytes / offsets; skip > 0: bytes is the view
    buf[skip:] of a longer allocation"""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    buf = torch.full((len(raw) + skip,), 0xEE, dtype=torch.uint8,
                     device="cuda")
    buf[skip:] = torch.from_numpy(raw.copy()).cuda()
    return ex.GpuText(
        bytes=buf[skip:],
        offs=torch.tensor(list(offs), dtype=torch.int64, device="cuda"),
        nulls=None if nulls is None else
        torch.tensor(list(nulls), dtype=torch.uint8, device="cuda"))


def run_rank(ex, texts):
    node = ex.GpuTextRank(texts)
    node.BeginCustomScan()
    r = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    info = node.explain()
    node.EndCustomScan()
    assert info["rounds"] == r.rounds and info["text_rank"] >= 0
    assert len(r.codes) == len(texts)
    for c, t in zip(r.codes, texts):
        assert c.dtype == torch.int64 and len(c) == len(t)
    return r


def check_rank(ex, texts, rows_per_col, refs=(rank_set,)):
    """rank of the columns on the GPU == the references over the
    concatenated host rows; dictionary and decode round-trip"""
    r = run_rank(ex, texts)
    rows = [x for col in rows_per_col for x in col]
    got = [c for t in r.codes for c in t.cpu().tolist()]
    for ref in refs:
        codes, d, first = ref(rows)
        assert got == codes
        assert r.ndistinct == d
        assert r.dict_rows.cpu().tolist() == first
    live = [x for x in rows if x is not None]
    assert r.dictionary().to_list() == sorted(set(live))
    for c, col in zip(r.codes, rows_per_col):
        assert r.decode(c).to_list() == col
    lmax = max((len(x) for x in live), default=0)
    assert r.rounds <= 1 + lmax // 8
    assert (r.rounds == 0) == (len(rows) == 0)
    return r


# ---- sizes ----

@pytest.mark.parametrize("n", SIZES)
def test_rank_sizes(ex, n):
    rows = random_rows(np.random.default_rng(100 + n), n)
    text = ex.GpuText(rows)
    r = check_rank(ex, [text], [rows])
    if n >= WAVE:
        assert r.ndistinct < n and r.rounds > 1


# ---- edge rows ----

EDGE = {
    "nul_bytes": [b"a\1", b"a\0\0", b"a", b"", b"a\0", b"a", b"a\0"],
    "null_next_to_empty": [None, b"", b"", None, b"\0", None],
    "high_bytes": [b"z", b"\x80", b"\xff", b"a\x80", b"a~", b"\x7f", b"\xc3\xa9",
                   b"e", b"\xff\xff", b"\xff\0"],
    "last_byte": [b"x" * (k - 1) + c for k in (7, 8, 9, 16, 17)
                  for c in (b"b", b"a", b"\xff", b"\0")],
    "prefixes": [b"abcdefghijklmnopq"[:k] for k in (17, 9, 8, 7, 16, 0, 1, 17, 8,
                                                    15)],
    "all_null": [None] * 70,
    "all_equal_short": [b"same"] * 300,
    "all_equal_long": [b"the same nineteen b"] * 300,
    "one_row_null": [None],
}


@pytest.mark.parametrize("case", sorted(EDGE))
def test_rank_edge_rows(ex, case):
    rows = EDGE[case]
    r = check_rank(ex, [ex.GpuText(rows)], [rows], refs=(rank_set, rank_cmp))
    if case == "nul_bytes":
        c = dict(zip(rows, r.codes[0].cpu().tolist()))
        assert c[b""] < c[b"a"] < c[b"a\0"] < c[b"a\0\0"] < c[b"a\1"]
    if case == "all_null":
        assert r.ndistinct == 0 and set(r.codes[0].cpu().tolist()) == {-1}
    if case == "all_equal_long":
        assert r.ndistinct == 1 and r.rounds == 3


# ---- rounds ----

def test_rounds_short_strings_take_one_round(ex):
    rng = np.random.default_rng(5)
    rows = random_rows(rng, 3000, maxlen=8)
    assert len(set(rows)) < len(rows)
    r = check_rank(ex, [ex.GpuText(rows)], [rows])
    assert r.rounds == 1


def test_rounds_one_round_unless_two_long_rows_share_8_bytes(ex):
    # long rows, but no two of them share their first 8 bytes; the short
    # rows share theirs with long ones
    rows = [b"%07dX" % i + b"tail" * (i % 5) for i in range(500)] + \
           [b"%07dX" % i for i in range(0, 500, 3)] + [b"0000", None]
    r = check_rank(ex, [ex.GpuText(rows)], [rows])
    assert r.rounds == 1


def test_rounds_shared_200_byte_prefix(ex):
    rng = np.random.default_rng(6)
    pre = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    tails = [bytes(rng.integers(97, 100, rng.integers(0, 12), dtype=np.uint8))
             for _ in range(120)]
    rows = [pre + tails[i] for i in rng.integers(0, 120, 300)]
    assert len(set(rows)) < len(rows)
    lmax = max(len(x) for x in rows)
    r = check_rank(ex, [ex.GpuText(rows)], [rows], refs=(rank_set, rank_cmp))
    assert 1 < r.rounds <= 1 + lmax // 8
    assert r.rounds >= 200 // 8


def test_rounds_one_mib_row_among_short_rows(ex):
    rng = np.random.default_rng(7)
    rows = random_rows(rng, 1000, maxlen=8)
    big = bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    rows[517] = big
    # its first 8 bytes also stand alone as a short row
    rows[3] = big[:8]
    r = check_rank(ex, [ex.GpuText(rows)], [rows])
    assert r.rounds == 1


# ---- slices and broken offsets ----

def test_rank_slice_over_shared_bytes(ex):
    rng = np.random.default_rng(8)
    rows = random_rows(rng, 900)
    text = ex.GpuText(rows)
    for a, b in ((1, 900), (257, 700), (450, 450), (899, 900)):
        check_rank(ex, [text.slice(a, b)], [rows[a:b]])
    # and an unaligned bytes base: every aligned-load decision shifts
    live = [x if x is not None else b"" for x in rows]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in live])])
    for skip in (1, 3, 7):
        t = adopt(ex, b"".join(live), offs, skip=skip)
        check_rank(ex, [t], [live])


def test_rank_broken_offsets(ex):
    rng = np.random.default_rng(9)
    raw = bytes(rng.integers(97, 101, 400, dtype=np.uint8))
    offs = rng.integers(-50, 460, 301).tolist()     # any order, out of range
    offs[10:14] = [30, 20, 10, 0]                   # decreasing
    offs[100] = -(1 << 40)
    offs[101] = 1 << 40
    nulls = (rng.random(300) < 0.05).astype(np.uint8).tolist()
    t = adopt(ex, raw, offs, nulls)
    check_rank(ex, [t], [column_rows(raw, offs, nulls)])


# ---- joint rank and the text equality join ----

def ref_join(brows, prows, left):
    pairs = []
    for p, s in enumerate(prows):
        hit = [b for b, x in enumerate(brows) if s is not None and x == s]
        pairs += [(b, p) for b in hit]
        if left and not hit:
            pairs.append((-1, p))
    return sorted(pairs)


@pytest.mark.parametrize("ncols", [2, 4])
def test_joint_rank_and_text_join(ex, ncols):
    rng = np.random.default_rng(20 + ncols)
    sizes = (300, 0, 77, 411) if ncols == 4 else (257, 500)
    cols = [random_rows(rng, n, null_frac=0.05, maxlen=12) for n in sizes]
    texts = [ex.GpuText(c) for c in cols]
    r = check_rank(ex, texts, cols)
    # one dictionary: equal strings of different columns share a code
    code = {}
    for t, col in zip(r.codes, cols):
        for c, s in zip(t.cpu().tolist(), col):
            assert code.setdefault(s, c) == c
    b, p = 0, ncols - 1
    for jt in ("inner", "left"):
        exp = ref_join(cols[b], cols[p], jt == "left")
        node = ex.GpuHashJoin(r.codes[b], r.codes[p],
                              build_null=texts[b].nulls,
                              probe_null=texts[p].nulls, join_type=jt,
                              cap_pairs=len(exp) + 64)
        node.BeginCustomScan()
        got = sorted(node._run())
        node.EndCustomScan()
        assert got == exp
        assert any(x == -1 for x, _ in got) == (jt == "left")


# ---- compositions with the unchanged nodes ----

def run_sort(ex, **kw):
    node = ex.GpuSort(**kw)
    node.BeginCustomScan()
    perm = node.ExecCustomScan()
    node.EndCustomScan()
    return perm.cpu().tolist()


def test_order_by_text_desc_nulls_first_then_int(ex):
    rng = np.random.default_rng(30)
    rows = random_rows(rng, 700, null_frac=0.04)
    x = rng.integers(-5, 5, 700)
    t = ex.GpuText(rows)
    r = t.rank()
    got = run_sort(ex, keys=[r.codes[0], torch.from_numpy(x).cuda()],
                   descending=[True, False], nulls_first=[True, None],
                   nulls=[t.nulls, None])
    assert got == text_sort_perm(rows, desc=True, nulls_first=True,
                                 then=x.tolist())
    got = run_sort(ex, keys=[r.codes[0]], nulls=[t.nulls])
    assert got == text_sort_perm(rows)


def test_order_by_reproduces_reference_regression_output(ex, golden):
    rows = golden["rows"]
    u1 = np.array([x["unique1"] for x in rows], dtype=np.int64)
    du1 = torch.from_numpy(u1).cuda()
    su1 = ex.GpuText([x["stringu1"] for x in rows])
    s4 = ex.GpuText([x["string4"] for x in rows])
    r1, r4 = su1.rank(), s4.rank()
    assert r1.ndistinct == 19 and r4.ndistinct == 4
    assert [s.decode() for s in r4.dictionary().to_list()] == \
        golden["distinct_string4"]

    def table(perm, col):
        return [[int(u1[i]), rows[i][col]] for i in perm]

    assert table(run_sort(ex, keys=[r1.codes[0]]), "stringu1") == \
        golden["orders"]["stringu1_asc"]
    assert table(run_sort(ex, keys=[r4.codes[0], du1],
                          descending=[False, True]), "string4") == \
        golden["orders"]["string4_asc_unique1_desc"]
    assert table(run_sort(ex, keys=[r4.codes[0], du1],
                          descending=[True, False]), "string4") == \
        golden["orders"]["string4_desc_unique1_asc"]


def test_group_by_text_count_and_sum(ex):
    rng = np.random.default_rng(31)
    n = 5000
    rows = random_rows(rng, n, null_frac=0.03, maxlen=10)
    v = rng.integers(-100, 100, n).astype(np.float64)
    exp = {}
    for s, x in zip(rows, v.tolist()):
        e = exp.setdefault(s, [0, 0.0])
        e[0] += 1
        e[1] += x
    t = ex.GpuText(rows)
    r = t.rank()
    dv = torch.from_numpy(v).cuda()

    node = ex.GpuGroupAgg([r.codes[0]], [("count_star",), ("sum", dv)],
                          key_nulls=[t.nulls])
    node.BeginCustomScan()
    res = node.ExecCustomScan()
    node.EndCustomScan()
    keys, knull = res["keys"][0]
    codes = torch.where(knull.bool(), torch.full_like(keys, -1), keys)
    names = r.decode(codes).to_list()
    assert names == sorted(s for s in exp if s is not None) + [None]
    assert res["aggs"][0][0].cpu().tolist() == [exp[s][0] for s in names]
    assert res["aggs"][1][0].cpu().tolist() == [exp[s][1] for s in names]

    node = ex.GpuHashAgg(r.codes[0], dv, key_null=t.nulls)
    node.BeginCustomScan()
    groups = node._run()
    node.EndCustomScan()
    codes = torch.tensor([-1 if g["key_isnull"] else int(g["key"])
                          for g in groups], dtype=torch.int64, device="cuda")
    names = r.decode(codes).to_list()
    assert sorted(names, key=lambda s: (s is None, s)) == names
    assert set(names) == set(exp) and len(names) == len(exp)
    assert [int(g["count_star"]) for g in groups] == [exp[s][0] for s in names]
    assert [float(g["sum_v"]) for g in groups] == [exp[s][1] for s in names]


def test_min_max_text_per_int_group(ex):
    rng = np.random.default_rng(32)
    n = 3000
    rows = random_rows(rng, n, null_frac=0.2, maxlen=20)
    g = rng.integers(0, 40, n)
    for i in np.flatnonzero(g == 7):      # one group with no string at all
        rows[i] = None
    t = ex.GpuText(rows)
    r = t.rank()
    node = ex.GpuGroupAgg([torch.from_numpy(g).cuda()],
                          [("min", r.codes[0], t.nulls),
                           ("max", r.codes[0], t.nulls)])
    node.BeginCustomScan()
    res = node.ExecCustomScan()
    node.EndCustomScan()
    gk = res["keys"][0][0].cpu().tolist()
    assert gk == sorted(set(g.tolist()))
    for (vals, nulls), pick in zip(res["aggs"], (min, max)):
        codes = torch.where(nulls.bool(), torch.full_like(vals, -1), vals)
        got = r.decode(codes).to_list()
        exp = []
        for k in gk:
            live = [s for s, q in zip(rows, g.tolist())
                    if q == k and s is not None]
            exp.append(pick(live) if live else None)
        assert got == exp
        assert got[gk.index(7)] is None


def test_window_rank_partitioned_by_text(ex):
    rng = np.random.default_rng(33)
    n = 2000
    rows = random_rows(rng, n, null_frac=0.05, maxlen=9)
    x = rng.integers(0, 6, n)
    t = ex.GpuText(rows)
    r = t.rank()
    node = ex.GpuWindowAgg([r.codes[0]], [torch.from_numpy(x).cuda()],
                           part_nulls=[t.nulls],
                           funcs=("rank", "dense_rank", "part_rows"))
    node.BeginCustomScan()
    res = node.ExecCustomScan()
    node.EndCustomScan()
    # the reference partitions by codes computed on the host, independently
    codes = np.array(rank_set(rows)[0], dtype=np.int64)
    nulls = np.array([s is None for s in rows], dtype=np.uint8)
    spec = [(codes, nulls, False, False), (x, None, False, False)]
    exp = ref_window(spec, 1)
    assert res["perm"].cpu().tolist() == ref_perm(spec).tolist()
    for f in ("rank", "dense_rank", "part_rows"):
        assert res[f].cpu().tolist() == exp[f].tolist(), f
    # and against the strings themselves: rank 1 is the smallest x of a string
    perm = res["perm"].cpu().tolist()
    for j, rk in zip(perm, res["rank"].cpu().tolist()):
        if rk == 1:
            assert x[j] == min(q for s, q in zip(rows, x) if s == rows[j])


# ---- the optional outputs of the C entry point ----

def test_rank_without_dict_rows_and_rounds(ex):
    import ctypes as C
    from opentenbase_amd._lib import call, lib
    rows = random_rows(np.random.default_rng(50), 3000)
    text = ex.GpuText(rows)
    node = ex.GpuTextRank([text])
    ts = node.textset()
    wsb = C.c_size_t(0)
    assert lib().otbx_text_rank_workspace_bytes(len(rows), C.byref(wsb)) == 0
    # 16 bytes into an allocation: the least alignment the contract allows
    ws = torch.empty(wsb.value + 16, dtype=torch.uint8, device="cuda")[16:]
    assert ws.data_ptr() % 16 == 0
    codes = torch.empty(len(rows), dtype=torch.int64, device="cuda")
    nd = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    call("otbx_text_rank", C.byref(ts), C.c_void_p(ws.data_ptr()),
         C.c_size_t(wsb.value), C.c_void_p(codes.data_ptr()), None,
         C.c_void_p(nd.data_ptr()), None,
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    exp, d, _ = rank_set(rows)
    assert codes.cpu().tolist() == exp and int(nd.item()) == d


# ---- determinism, rescan ----

def test_rank_is_deterministic_and_rescans(ex):
    rng = np.random.default_rng(40)
    rows = random_rows(rng, 2 * SS_TILE + 5)
    a = ex.GpuText(rows[:5000])
    b = ex.GpuText(rows[5000:])
    node = ex.GpuTextRank([a, b])
    node.BeginCustomScan()
    r1 = node.ExecCustomScan()
    node.ReScanCustomScan()
    r2 = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    r3 = a.rank(b)
    for r in (r2, r3):
        assert r.ndistinct == r1.ndistinct and r.rounds == r1.rounds
        assert torch.equal(r.dict_rows, r1.dict_rows)
        for x, y in zip(r.codes, r1.codes):
            assert torch.equal(x, y)
    assert [c for t in r1.codes for c in t.cpu().tolist()] == \
        rank_set(rows)[0]

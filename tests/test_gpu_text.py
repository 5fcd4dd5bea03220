"""GPU parity of the text operators (otbx_text_pred / GpuTextPred, the text
gather / GpuText.gather): exact equality with the row-loop references of
tests/text_ref.py everywhere. Every predicate test runs three times: with
OTBX_TEXT_STAGE=1, the tile's bytes staged in LDS wherever its offsets
allow, with OTBX_TEXT_STAGE=0, every row read from global memory, and with
the variable unset, the library choosing per predicate."""
import ctypes as C

import numpy as np
import pytest
import torch

from text_ref import (OPS, P_NAME_WORDS, clamped_rows, like_dp, like_rec,
                      ref_gather, ref_pred)

pytestmark = pytest.mark.gpu

T = 256                   # TXT_TILE of otbx_text.hip: rows per workgroup
BUDGET = 32768            # TXT_LDS_BUDGET: largest staged tile span, bytes
GATHER_CHUNK = 256 * 1024  # TG_TILE * TG_SCAN_THREADS: rows per scan pass
GATHER_SLICE = 16384      # TGB_SLICE: dst bytes per workgroup
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    assert executor.TEXT_TILE == T and executor.TEXT_LDS_BUDGET == BUDGET
    assert executor.TEXT_GATHER_CHUNK == GATHER_CHUNK
    return executor


@pytest.fixture(params=["staged", "direct", "default"])
def path(request, monkeypatch):
    """staged: every tile whose offsets allow it goes through LDS; direct:
    none does; default: the library's own rule picks per predicate"""
    if request.param == "default":
        monkeypatch.delenv("OTBX_TEXT_STAGE", raising=False)
    else:
        monkeypatch.setenv("OTBX_TEXT_STAGE",
                           "1" if request.param == "staged" else "0")
    return request.param


def run_node(node):
    node.BeginCustomScan()
    v, m = node.ExecCustomScan()
    assert node.ExecCustomScan() is None
    node.EndCustomScan()
    assert v.dtype == torch.uint8 and len(v) == node.n
    assert (m is None) == (not node.nullable)
    return v.cpu().tolist(), ([0] * node.n if m is None else m.cpu().tolist())


_REF = {}   # references shared by the two paths of a test


def check_pred(ex, text, rows, op, rhs, rhs_rows=None, encoding="utf8",
               sel=None, matcher=like_dp, ref_key=None):
    """text OP rhs on the GPU == ref_pred over `rows` (the host image of
    text); with sel, over the selected rows. ref_key: compute the reference
    once under that key"""
    got = run_node(ex.GpuTextPred(text, op, rhs, sel=sel, encoding=encoding))
    r = rhs_rows if rhs_rows is not None else rhs
    if sel is not None:
        ids = sel.cpu().tolist()
        rows = ref_gather(rows, ids)
        if isinstance(r, list):
            r = ref_gather(r, ids)
    if ref_key is not None and ref_key in _REF:
        exp = _REF[ref_key]
    else:
        exp = ref_pred(rows, op, r, encoding == "utf8", matcher)
        if ref_key is not None:
            _REF[ref_key] = exp
    assert got[0] == exp[0], (op, rhs if not isinstance(rhs, ex.GpuText)
                              else "column", encoding)
    assert got[1] == exp[1]
    return exp


def random_rows(rng, n, lo=0, hi=40, alphabet=b"abcd"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [a[rng.integers(0, len(a), rng.integers(lo, hi + 1))].tobytes()
            for _ in range(n)]


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


# ---- sizes and length shapes ----

@pytest.mark.parametrize("n", SIZES)
def test_pred_sizes(ex, path, n):
    rng = np.random.default_rng(n)
    rows = random_rows(rng, n)
    if n > 2:
        rows[n // 2] = None
    text = ex.GpuText(rows)
    assert len(text) == n and text.to_list() == rows
    for op, rhs in (("like", "%ab%"), ("not like", "a_%b"), ("like", "%"),
                    ("=", rows[0] if n and rows[0] is not None else b"a"),
                    ("<", b"c")):
        check_pred(ex, text, rows, op, rhs)


@pytest.mark.parametrize("shape", ["empty", "one_byte"])
def test_pred_all_rows_empty_or_one_byte(ex, path, shape):
    rng = np.random.default_rng(3)
    n = 2 * T + 5
    rows = [b""] * n if shape == "empty" else random_rows(rng, n, 1, 1)
    text = ex.GpuText(rows)
    for op, rhs in (("like", ""), ("like", "%"), ("like", "_"),
                    ("not like", "a"), ("=", ""), (">=", "b"), ("<>", "a")):
        check_pred(ex, text, rows, op, rhs)


def test_pred_one_huge_row_in_a_tile_of_short_rows(ex, path):
    # 300 KB in one row: the tile's span is far above the LDS budget, so it
    # is read from global memory even with staging on; its neighbours in
    # other tiles are staged
    rng = np.random.default_rng(4)
    rows = random_rows(rng, 2 * T + 9, 0, 20)
    rows[T + 17] = b"q" * 300_000 + b"xyz"
    rows[T + 18] = b"q" * 10 + b"xyz"
    text = ex.GpuText(rows)
    for op, rhs in (("like", "%xyz"), ("not like", "q%z"), ("like", "%ab%"),
                    ("=", rows[T + 18]), (">", b"q" * 100)):
        check_pred(ex, text, rows, op, rhs, matcher=like_rec_or_dp,
                   ref_key=("huge", op, rhs))


def like_rec_or_dp(t, p, utf8):
    # the table is quadratic: the 300 KB row goes through the recursion
    return like_rec(t, p, utf8) if len(t) > 5000 else like_dp(t, p, utf8)


@pytest.mark.parametrize("span", [BUDGET - 1, BUDGET, BUDGET + 1])
def test_pred_tile_span_around_the_lds_budget(ex, path, span):
    rng = np.random.default_rng(span)
    per = BUDGET // T                       # 128 bytes per row fills it
    mid = random_rows(rng, T, per, per)
    mid[7] = mid[7][:per - 1] if span < BUDGET else \
        mid[7] + (b"d" if span > BUDGET else b"")
    mid[T - 1] = mid[T - 1][:-3] + b"abc"   # the tile's very last bytes
    assert sum(len(r) for r in mid) == span
    rows = random_rows(rng, T, 0, 9) + mid + random_rows(rng, T // 2, 0, 9)
    text = ex.GpuText(rows)
    for op, rhs in (("like", "%abc"), ("like", "%abcd%dcba%"),
                    ("not like", "a%"), ("<=", mid[3])):
        check_pred(ex, text, rows, op, rhs)


# ---- layout ----

@pytest.mark.parametrize("skip", [1, 7])
def test_pred_bytes_at_an_odd_address(ex, path, skip):
    rng = np.random.default_rng(skip)
    rows = random_rows(rng, T + 50, 0, 30)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    text = adopt(ex, b"".join(rows), offs, skip=skip)
    assert text.bytes.data_ptr() % 16 == skip
    for op, rhs in (("like", "%ab%c"), ("not like", "_b%"), (">", "bb")):
        check_pred(ex, text, rows, op, rhs)


def test_pred_slice_with_a_nonzero_first_offset(ex, path):
    rng = np.random.default_rng(8)
    rows = random_rows(rng, 2 * T + 40, 0, 25)
    text = ex.GpuText(rows)
    for a, b in ((5, 2 * T + 40), (T - 3, T + 9), (11, 11)):
        part = text.slice(a, b)
        assert part.to_list() == rows[a:b]
        check_pred(ex, part, rows[a:b], "like", "%a%b")
        check_pred(ex, part, rows[a:b], "<>", rows[a] if b > a else b"")


def test_pred_garbage_offsets_under_a_null(ex, path):
    rows = [b"abc", b"", b"", b"bcd", b"ab"] * 20
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    nulls = [0] * len(rows)
    # rows 41 and 42 are NULL; the offset between them is garbage
    for k, junk in ((41, -7), (61, 10**15)):
        nulls[k] = nulls[k + 1] = 1
        offs[k + 1] = junk
    text = adopt(ex, b"".join(rows), offs, nulls)
    exp_rows = [None if nulls[i] else r for i, r in enumerate(rows)]
    assert text.to_list() == exp_rows
    for op, rhs in (("like", "%b%"), ("not like", "%b%"), ("=", "ab")):
        check_pred(ex, text, exp_rows, op, rhs)


def test_pred_broken_offsets_read_nothing_outside(ex, path):
    # one call: decreasing offsets, offsets beyond nbytes, negative ones.
    # The answer is that of the clamped column
    raw = b"abcabcabcabcabcabcab"
    offs = [0, 3, 2, 9, 10**12, 6, -5, 4, 20, 25, 18, 17, 20, -2**62, 2**62,
            12, 15]
    text = adopt(ex, raw, offs)
    rows = clamped_rows(raw, offs)
    assert rows[3] == raw[9:] and rows[1] == b"" and rows[13] == raw
    assert text.to_list() == rows
    check_pred(ex, text, rows, "like", "%ca%")


# ---- the LIKE table ----

LIKE_PATTERNS = ["%", "", "_", "__%", "%_", "a%", "%a", "%a%", "a%b%c",
                 "%a%a%a%b", "\\%", "\\_", "\\\\", "%\\%%", "%\\_", "a\\%b",
                 "_%_", "%b_", "ab", "%é%", "_é", "é_", "__", "___", "____",
                 "%€", "a_c", "%\x80".encode("latin1"),
                 b"_\x82%", b"%\xc3"]


@pytest.fixture(scope="module")
def like_rows():
    rng = np.random.default_rng(12)
    rows = random_rows(rng, T - 20, 0, 9, b"abc")
    rows += random_rows(rng, 40, 0, 6, b"ab%_\\")
    # 1-, 2-, 3- and 4-byte characters, alone and between ASCII
    for ch in ("a", "é", "€", "😀"):
        e = ch.encode()
        rows += [e, e + e, b"a" + e, e + b"c", b"a" + e + b"c", e + e + e]
    rows += [b"\x80", b"a\x80", b"\x80\x80", b"a\x80c",     # stray tail byte
             b"a\xe2\x82", b"\xf0\x9f", b"ab\xc3",          # truncated last
             b"%", b"_", b"\\", b"a%b", b"a_b", b"100%", b""]
    rows += [b"a" * 3000, b"a" * 2999 + b"b", None]
    return rows


@pytest.fixture(scope="module")
def like_text(ex, like_rows):
    return ex.GpuText(like_rows)


@pytest.mark.parametrize("encoding", ["utf8", "sb"])
@pytest.mark.parametrize("pat", LIKE_PATTERNS, ids=repr)
def test_like_table(ex, path, like_text, like_rows, pat, encoding):
    for op in ("like", "not like"):
        check_pred(ex, like_text, like_rows, op, pat, encoding=encoding,
                   matcher=like_rec_or_dp, ref_key=("table", op, pat, encoding))


def test_like_encodings_differ_on_a_two_byte_character(ex, path):
    rows = ["é".encode(), b"e", b"ab"]
    text = ex.GpuText(rows)
    u = run_node(ex.GpuTextPred(text, "like", "_", encoding="utf8"))[0]
    s = run_node(ex.GpuTextPred(text, "like", "_", encoding="sb"))[0]
    assert u == [1, 1, 0] and s == [0, 1, 0]
    s2 = run_node(ex.GpuTextPred(text, "like", "__", encoding="sb"))[0]
    assert s2 == [1, 0, 1]


def test_like_pattern_of_256_bytes(ex, path):
    rows = [b"a" * 255, b"a" * 255 + b"zz", b"a" * 254 + b"b", b"a" * 256]
    text = ex.GpuText(rows)
    check_pred(ex, text, rows, "like", "a" * 255 + "%")
    check_pred(ex, text, rows, "not like", "_" * 255 + "a")
    check_pred(ex, text, rows, ">=", b"a" * 256)
    with pytest.raises(ex.OtbxError) as e:
        ex.GpuTextPred(text, "like", "a" * 256 + "%")
    assert e.value.status == 3


# ---- comparisons ----

CMP_ROWS = [b"", b"a", b"ab", b"abc", b"abd", b"b", b"\x7f", b"\x80",
            b"\xff", b"a\x00", b"a\x00b", b"\x00", b"ab\x80", b"ab\x7f", None]


@pytest.mark.parametrize("op", OPS[2:])
def test_compare_with_constants(ex, path, op):
    rng = np.random.default_rng(OPS.index(op))
    rows = CMP_ROWS * 20 + random_rows(rng, 77, 0, 5, b"ab\x80\x00")
    text = ex.GpuText(rows)
    for c in (b"", b"ab", b"abc", b"\x80", b"a\x00", b"\x7f"):
        check_pred(ex, text, rows, op, c)
    # the same column without a mask: no null output is needed
    plain = [r for r in rows if r is not None]
    node = ex.GpuTextPred(ex.GpuText(plain), op, b"ab")
    assert not node.nullable
    assert run_node(node) == ref_pred(plain, op, b"ab")


@pytest.mark.parametrize("op", OPS[2:])
def test_compare_two_columns(ex, path, op):
    rng = np.random.default_rng(40 + OPS.index(op))
    n = T + 90
    pool = [r for r in CMP_ROWS if r is not None]
    left = [pool[i] for i in rng.integers(0, len(pool), n)]
    right = [pool[i] for i in rng.integers(0, len(pool), n)]
    for i in range(0, n, 5):
        right[i] = left[i]                       # equal pairs
    lnull, rnull = list(left), list(right)
    for i in range(3, n, 11):
        lnull[i] = None
    for i in range(4, n, 13):
        rnull[i] = None
    rnull[3] = None                              # NULL on both sides
    for a, b in ((left, right), (lnull, right), (left, rnull), (lnull, rnull)):
        check_pred(ex, ex.GpuText(a), a, op, ex.GpuText(b), rhs_rows=b)


# ---- selections ----

def test_pred_through_a_selection(ex, path):
    rng = np.random.default_rng(21)
    n = 3 * T + 31
    rows = random_rows(rng, n, 0, 20)
    rows[5] = rows[n - 1] = None
    other = random_rows(rng, n, 0, 3, b"ab")
    text, otext = ex.GpuText(rows), ex.GpuText(other)
    key = torch.from_numpy(rng.integers(0, 100, n)).cuda()
    flt = ex.GpuFilter([[ex.qual_term(key, "<", 30)]])
    flt.BeginCustomScan()
    asc = flt.ExecCustomScan()
    flt.EndCustomScan()
    assert 0 < len(asc) < n
    sels = [asc, torch.flip(asc, [0]).contiguous(),
            torch.tensor([7, 7, 7, 0, n - 1, 5, 5, 7], device="cuda"),
            torch.tensor([-1, -2**62, n, 2**62, 3, n - 1, 10**12],
                         device="cuda"),
            torch.zeros(0, dtype=torch.int64, device="cuda")]
    for sel in sels:
        for op, rhs, rr in (("like", "%ab%", None), ("not like", "a%", None),
                            ("<", b"bb", None), (">=", otext, other)):
            exp = check_pred(ex, text, rows, op, rhs, rhs_rows=rr, sel=sel)
            # the same as the predicate over the gathered column
            if len(sel):
                g = text.gather(sel)
                r2 = otext.gather(sel) if rr is not None else rhs
                assert run_node(ex.GpuTextPred(g, op, r2)) == exp


# ---- gather ----

def check_gather(ex, text, rows, perm):
    got = text.gather(torch.tensor(perm, dtype=torch.int64, device="cuda"))
    exp = ref_gather(rows, perm) if len(perm) else []
    assert len(got) == len(perm)
    lens = [0 if r is None else len(r) for r in exp]
    assert got.offs.cpu().tolist() == \
        [0] + np.cumsum(lens, dtype=np.int64).tolist()
    assert got.to_list() == exp
    return got


def test_gather_small_shapes(ex):
    rng = np.random.default_rng(31)
    n = 2 * T + 3
    rows = random_rows(rng, n, 0, 12)
    rows[4] = rows[n - 2] = None
    text = ex.GpuText(rows)
    check_gather(ex, text, rows, list(range(n)))
    check_gather(ex, text, rows, list(range(n - 1, -1, -1)))
    check_gather(ex, text, rows, [3, 3, 3, 4, 0, n - 1, 3, 4, 4])
    check_gather(ex, text, rows, [-1, n, 2**62, -2**62, 5])
    g = check_gather(ex, text, rows, [])
    assert len(g.bytes) == 0
    empty = ex.GpuText([b""] * 700)
    g = check_gather(ex, empty, [b""] * 700, list(range(699, -1, -1)))
    assert len(g.bytes) == 0
    # a slice gathers like a column of its own
    part = text.slice(10, T + 20)
    check_gather(ex, part, rows[10:T + 20], [0, T + 9, 5, 5])


def test_gather_one_megabyte_row_among_short_rows(ex):
    rng = np.random.default_rng(32)
    n = 10_000
    lens = rng.integers(0, 8, n)
    lens[n // 3] = 1 << 20
    flat = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)])
    text = ex.GpuText(bytes=torch.from_numpy(flat).cuda(),
                      offs=torch.from_numpy(offs).cuda())
    perm = rng.permutation(n)
    perm[17] = perm[n - 5] = n // 3               # the big row three times
    check_gather_np(ex, text, flat, offs, perm)


def check_gather_np(ex, text, flat, offs, perm):
    got = text.gather(torch.from_numpy(perm).cuda())
    lens = (offs[1:] - offs[:-1])[perm]
    doffs = np.concatenate([[0], np.cumsum(lens)])
    assert np.array_equal(got.offs.cpu().numpy(), doffs)
    total = int(doffs[-1])
    src = np.repeat(offs[:-1][perm] - doffs[:-1], lens) + np.arange(total)
    assert len(got.bytes) == total
    assert np.array_equal(got.bytes.cpu().numpy(), flat[src])


def test_gather_crosses_the_scan_chunk(ex):
    # one row more than one pass of the offset scan takes
    rng = np.random.default_rng(33)
    n = GATHER_CHUNK + 1
    lens = rng.integers(0, 4, n)
    flat = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)])
    text = ex.GpuText(bytes=torch.from_numpy(flat).cuda(),
                      offs=torch.from_numpy(offs).cuda())
    check_gather_np(ex, text, flat, offs, rng.permutation(n))


def test_gather_bytes_truncates_at_dst_nbytes(ex):
    from opentenbase_amd._lib import call
    rng = np.random.default_rng(34)
    rows = random_rows(rng, 5000, 0, 15)
    text = ex.GpuText(rows)
    perm = torch.from_numpy(rng.permutation(5000)).cuda()
    full = text.gather(perm)
    total = len(full.bytes)
    assert total > 2 * GATHER_SLICE
    # one byte short: the last byte of the buffer's tail stays as it was
    dst = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    c = text.col()
    call("otbx_text_gather_bytes", C.byref(c), C.c_int64(len(text)),
         C.c_void_p(perm.data_ptr()), C.c_int64(len(perm)),
         C.c_void_p(full.offs.data_ptr()), C.c_void_p(dst.data_ptr()),
         C.c_int64(total - 1),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(dst[:total - 1], full.bytes[:total - 1])
    assert bool((dst[total - 1:] == 0xEE).all())


# ---- composition with the other operators ----

def test_part_names_like_green_filter_join(ex, path):
    rng = np.random.default_rng(50)
    n = 50_000
    assert len(P_NAME_WORDS) == 92
    w = rng.integers(0, 92, (n, 5))
    names = [" ".join(P_NAME_WORDS[j] for j in r).encode() for r in w]
    partkey = np.arange(1, n + 1, dtype=np.int64) * 3
    name = ex.GpuText(names)
    pk = torch.from_numpy(partkey).cuda()
    pred = ex.GpuTextPred(name, "like", "%green%")
    flt = ex.GpuFilter([[pred.term()]])
    keys = flt.gather(pk)
    exp = [int(k) for k, s in zip(partkey, names) if b"green" in s]
    assert 0 < len(exp) < n and keys.cpu().tolist() == exp
    assert pred.explain()["text_pred"] >= 0.0
    # the names travel with the selection
    assert name.gather(flt.sel).to_list() == [s for s in names
                                              if b"green" in s]
    # the surviving keys join unchanged
    probe = rng.integers(1, 3 * n + 1, 20_000).astype(np.int64)
    join = ex.GpuHashJoin(keys, torch.from_numpy(probe).cuda())
    join.BeginCustomScan()
    pairs = []
    while (p := join.ExecCustomScan()) is not None:
        pairs.append(p)
    join.EndCustomScan()
    pos = {k: i for i, k in enumerate(exp)}
    want = sorted((pos[int(k)], j) for j, k in enumerate(probe)
                  if int(k) in pos)
    assert len(want) > 0 and sorted(pairs) == want


def test_sort_permutation_gathers_text(ex):
    rng = np.random.default_rng(51)
    n = 5000
    rows = random_rows(rng, n, 0, 18)
    rows[100] = None
    key = rng.permutation(n).astype(np.int64)
    srt = ex.GpuSort([torch.from_numpy(key).cuda()])
    srt.BeginCustomScan()
    perm = srt.ExecCustomScan()
    srt.EndCustomScan()
    order = np.argsort(key)
    assert ex.GpuText(rows).gather(perm).to_list() == [rows[i] for i in order]


def test_text_pred_lifecycle(ex, path):
    rows = [b"green apple", None, b"red", b"evergreen"] * 70
    node = ex.GpuTextPred(ex.GpuText(rows), "like", "%green%")
    exp = ref_pred(rows, "like", b"%green%")
    assert node.explain() is None
    for _ in range(2):
        node.BeginCustomScan()
        v, m = node.ExecCustomScan()
        assert (v.cpu().tolist(), m.cpu().tolist()) == exp
        assert node.ExecCustomScan() is None
        node.ReScanCustomScan()
        v, m = node.ExecCustomScan()
        assert (v.cpu().tolist(), m.cpu().tolist()) == exp
        node.EndCustomScan()
        assert node.explain()["text_pred"] >= 0.0
    with pytest.raises(ex.OtbxError):
        node.ExecCustomScan()

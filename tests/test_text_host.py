"""CPU-side tests of the text operators' host layers: the two LIKE references
agree with each other and with the reference's regression cases,
like_escape, the argument checks of otbx_text_pred and the text gather (pure
host code — no HIP call is reached), the ctypes layout of the structs and
the GpuText / GpuTextPred argument checks."""
import ctypes as C
import json
import os
import random
import shutil
import subprocess

import pytest

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import TextColDev, TextPredDev
from text_ref import (TrailingEscape, has_trailing_escape, like_dp, like_rec,
                      ref_gather, ref_pred, tokens)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


# ---- the two references ----

def _agree(text, pat, utf8):
    if has_trailing_escape(pat):
        with pytest.raises(TrailingEscape):
            tokens(pat)
        return None
    a, b = like_rec(text, pat, utf8), like_dp(text, pat, utf8)
    assert a == b, (text, pat, utf8, a, b)
    return a


@pytest.mark.parametrize("utf8", [False, True])
def test_like_refs_agree_on_small_alphabet(utf8):
    rng = random.Random(11 + utf8)
    text_syms = b"abcd"
    pat_syms = b"abcd%_\\" + b"%_"     # wildcards twice as likely
    seen = {True: 0, False: 0, None: 0}
    for _ in range(4000):
        text = bytes(rng.choice(text_syms) for _ in range(rng.randint(0, 12)))
        pat = bytes(rng.choice(pat_syms) for _ in range(rng.randint(0, 8)))
        seen[_agree(text, pat, utf8)] += 1
    # the sample decides nothing unless both answers are common
    assert seen[True] > 300 and seen[False] > 300


@pytest.mark.parametrize("utf8", [False, True])
def test_like_refs_agree_on_valid_and_broken_utf8(utf8):
    rng = random.Random(23 + utf8)
    # 1- to 4-byte characters, then pieces that break them: a stray
    # continuation byte, lead bytes without their tail
    chars = ["a", "é", "€", "😀"]
    pieces = [c.encode() for c in chars] + [b"\x80", b"\xc3", b"\xe2\x82",
                                            b"\xf0\x9f"]
    pat_pieces = pieces + [b"%", b"_", b"%", b"_", b"\\"]
    seen = {True: 0, False: 0, None: 0}
    for _ in range(4000):
        text = b"".join(rng.choice(pieces) for _ in range(rng.randint(0, 6)))
        pat = b"".join(rng.choice(pat_pieces)
                       for _ in range(rng.randint(0, 5)))
        seen[_agree(text, pat, utf8)] += 1
    assert seen[True] > 300 and seen[False] > 300


def test_encodings_differ_on_multibyte_any_char():
    e = "é".encode()
    for f in (like_rec, like_dp):
        assert f(e, b"_", True) and not f(e, b"_", False)
        assert f(e, b"__", False) and not f(e, b"__", True)
        # a truncated last character is one character, a stray continuation
        # byte is one too
        assert f(b"a\xe2\x82", b"a_", True)
        assert f(b"\x80", b"_", True) and f(b"\x80\x80", b"_", True)
        assert f(b"", b"", True) and not f(b"a", b"", True)
        assert f(b"%", b"\\%", True) and not f(b"a", b"\\%", True)


def _golden():
    with open(os.path.join(REPO, "tests", "golden", "like_cases.json"),
              encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_golden_like_cases():
    cases = _golden()
    assert len(cases) == 57     # 44 single statements, 13 in the %/_ rows
    assert any(c["escape"] is not None for c in cases)
    assert any(c["negate"] for c in cases)
    for c in cases:
        pat = c["pattern"].encode()
        if c["escape"] is not None:
            pat = ex.like_escape(pat, c["escape"])
        for f in (like_rec, like_dp):
            for utf8 in (False, True):
                got = f(c["text"].encode(), pat, utf8)
                assert (not got if c["negate"] else got) == c["expected"], c


def test_like_escape_edges():
    assert ex.like_escape("a\\b%", "") == b"a\\\\b%"      # doubled
    assert ex.like_escape(b"a\\%b", "\\") == b"a\\%b"      # as it is
    assert ex.like_escape("h#%", "#") == b"h\\%"
    assert ex.like_escape("a##b", "#") == b"a\\#b"         # escape, itself
    assert ex.like_escape("m%a%%a", "%") == b"m\\a\\%a"
    assert ex.like_escape("a\\b", "#") == b"a\\\\b"        # literal backslash
    assert ex.like_escape("a#\\b", "#") == b"a\\\\b"       # escaped backslash
    assert ex.like_escape("aéé_", "é") == "a\\é_".encode()
    assert ex.like_escape("", "#") == b""
    for bad in ("ab", "éé"):
        with pytest.raises(_lib.OtbxError) as e:
            ex.like_escape("x", bad)
        assert e.value.status == 3
    with pytest.raises(_lib.OtbxError):
        ex.like_escape(5, "#")


def test_ref_pred_and_gather():
    rows = [b"ab", None, b"", b"abc", b"\x80", b"a\x00"]
    assert ref_pred(rows, "<", b"abc") == ([1, 0, 1, 0, 0, 1],
                                           [0, 1, 0, 0, 0, 0])
    assert ref_pred(rows, ">", b"\x7f")[0] == [0, 0, 0, 0, 1, 0]   # unsigned
    assert ref_pred(rows, "=", rows)[0] == [1, 0, 1, 1, 1, 1]
    assert ref_pred(rows, "not like", b"a%")[0] == [0, 0, 1, 0, 1, 0]
    assert ref_gather(rows, [5, 5, -3, 99, 2]) == [b"a\x00", b"a\x00", b"ab",
                                                   b"a\x00", b""]


# ---- otbx_text_pred argument checks: all rejected before any HIP call ----

def _col(bytes_=0x1000, offs=0x1000, nulls=None, nbytes=64):
    c = TextColDev()
    c.bytes, c.offs, c.nulls, c.nbytes = bytes_, offs, nulls, nbytes
    return c


def _pred(op=0, encoding=1, const=b"a%", right=None, left=None):
    p = TextPredDev()
    p.left = left if left is not None else _col()
    p.op, p.encoding = op, encoding
    p.clen = len(const)
    C.memmove(p.cbytes, const, min(len(const), 256))
    if right is not None:
        p.right = C.pointer(right)
    return p


def _call_pred(so, p, n=10, n_src=10, sel=None, out=0x1000, out_null=0x1000):
    return so.otbx_text_pred(
        None if p is None else C.byref(p), C.c_void_p(sel), C.c_int64(n),
        C.c_int64(n_src), C.c_void_p(out), C.c_void_p(out_null), None)


@pytest.mark.parametrize("case", [
    "null_pred", "null_out", "op_neg", "op8", "enc_neg", "enc2",
    "right_like", "right_nlike", "right_and_const", "clen_neg", "clen257",
    "trailing_escape", "trailing_escape3", "n_neg", "n_big", "n_src_neg",
    "n_over_src", "n_src_zero", "null_bytes", "null_offs", "nbytes_neg",
    "right_null_offs", "right_nbytes_neg", "mask_without_out_null",
    "right_mask_without_out_null"])
def test_text_pred_invalid_arguments(so, case):
    p, kw = _pred(), {}
    if case == "null_pred":
        p = None
    elif case == "null_out":
        kw["out"] = None
    elif case == "op_neg":
        p = _pred(op=-1)
    elif case == "op8":
        p = _pred(op=8)
    elif case == "enc_neg":
        p = _pred(encoding=-1)
    elif case == "enc2":
        p = _pred(encoding=2)
    elif case == "right_like":
        p = _pred(op=0, const=b"", right=_col())
    elif case == "right_nlike":
        p = _pred(op=1, const=b"", right=_col())
    elif case == "right_and_const":
        p = _pred(op=2, const=b"x", right=_col())
    elif case == "clen_neg":
        p.clen = -1
    elif case == "clen257":
        p.clen = 257
    elif case == "trailing_escape":
        p = _pred(const=b"abc\\")
    elif case == "trailing_escape3":
        p = _pred(op=1, const=b"a\\\\\\")
    elif case == "n_neg":
        kw["n"] = -1
    elif case == "n_big":
        kw["n"], kw["n_src"] = INT32_MAX + 1, INT32_MAX + 1
    elif case == "n_src_neg":
        kw["n"], kw["n_src"] = 0, -1
    elif case == "n_over_src":
        kw["n"], kw["n_src"] = 11, 10
    elif case == "n_src_zero":
        kw["n"], kw["n_src"], kw["sel"] = 5, 0, 0x1000
    elif case == "null_bytes":
        p = _pred(left=_col(bytes_=None))
    elif case == "null_offs":
        p = _pred(left=_col(offs=None))
    elif case == "nbytes_neg":
        p = _pred(left=_col(nbytes=-1))
    elif case == "right_null_offs":
        p = _pred(op=2, const=b"", right=_col(offs=None))
    elif case == "right_nbytes_neg":
        p = _pred(op=4, const=b"", right=_col(nbytes=-5))
    elif case == "mask_without_out_null":
        p = _pred(left=_col(nulls=0x1000))
        kw["out_null"] = None
    elif case == "right_mask_without_out_null":
        p = _pred(op=2, const=b"", right=_col(nulls=0x1000))
        kw["out_null"] = None
    assert _call_pred(so, p, **kw) == OTBX_ERR_INVALID


def test_text_pred_zero_rows_is_valid_and_reaches_no_kernel(so):
    # n == 0 returns before any launch: no GPU is needed here
    assert _call_pred(so, _pred(), n=0, n_src=0) == 0
    assert _call_pred(so, _pred(), n=0, n_src=10, out=None,
                      out_null=None) == 0
    # an escaped backslash at the end is a literal, not a lone escape; 256
    # bytes are accepted
    assert _call_pred(so, _pred(const=b"ab\\\\"), n=0) == 0
    assert _call_pred(so, _pred(const=b"a" * 256), n=0) == 0
    assert _call_pred(so, _pred(op=2, const=b"abc\\"), n=0) == 0   # not LIKE


# ---- the gather entry points ----

def _ws(so, n):
    out = C.c_size_t(0)
    return so.otbx_text_gather_workspace_bytes(n, C.byref(out)), out.value


def test_text_gather_workspace_sizing(so):
    prev = -1
    for n in (0, 1, 255, 256, 257, 10**6, 10**8, INT32_MAX):
        st, b = _ws(so, n)
        assert st == 0 and b >= prev
        prev = b
    assert _ws(so, 0) == (0, 0)
    assert _ws(so, 1)[1] >= 8
    assert _ws(so, -1)[0] == OTBX_ERR_INVALID
    assert _ws(so, INT32_MAX + 1)[0] == OTBX_ERR_INVALID
    assert so.otbx_text_gather_workspace_bytes(10, None) == OTBX_ERR_INVALID


def _offsets(so, c, n_src=10, perm=0x1000, n=10, ws=0x1000, ws_bytes=None,
             dst_offs=0x1000):
    if ws_bytes is None:
        ws_bytes = _ws(so, max(min(n, INT32_MAX), 0))[1]
    return so.otbx_text_gather_offsets(
        None if c is None else C.byref(c), C.c_int64(n_src), C.c_void_p(perm),
        C.c_int64(n), C.c_void_p(ws), C.c_size_t(ws_bytes),
        C.c_void_p(dst_offs), None)


def _bytes(so, c, n_src=10, perm=0x1000, n=10, dst_offs=0x1000, dst=0x1000,
           dst_nbytes=100):
    return so.otbx_text_gather_bytes(
        None if c is None else C.byref(c), C.c_int64(n_src), C.c_void_p(perm),
        C.c_int64(n), C.c_void_p(dst_offs), C.c_void_p(dst),
        C.c_int64(dst_nbytes), None)


COMMON_BAD = {
    "null_src": dict(c=None),
    "n_neg": dict(n=-1),
    "n_big": dict(n=INT32_MAX + 1, n_src=INT32_MAX + 1),
    "n_src_neg": dict(n=0, n_src=-1),
    "n_src_zero": dict(n=3, n_src=0),
    "null_perm": dict(perm=None),
    "null_dst_offs": dict(dst_offs=None),
    "null_bytes": dict(c=_col(bytes_=None)),
    "null_offs": dict(c=_col(offs=None)),
    "nbytes_neg": dict(c=_col(nbytes=-1)),
}


@pytest.mark.parametrize("case", sorted(COMMON_BAD) + [
    "ws_short", "ws_null", "ws_unaligned"])
def test_text_gather_offsets_invalid_arguments(so, case):
    kw = {"c": _col()}
    if case == "ws_short":
        kw["ws_bytes"] = _ws(so, 10)[1] - 1
    elif case == "ws_null":
        kw["ws"] = None
    elif case == "ws_unaligned":
        kw["ws"] = 0x1004
    else:
        kw.update(COMMON_BAD[case])
    assert _offsets(so, **kw) == OTBX_ERR_INVALID


@pytest.mark.parametrize("case", sorted(COMMON_BAD) + [
    "dst_nbytes_neg", "null_dst"])
def test_text_gather_bytes_invalid_arguments(so, case):
    kw = {"c": _col()}
    if case == "dst_nbytes_neg":
        kw["dst_nbytes"] = -1
    elif case == "null_dst":
        kw["dst"] = None
    else:
        kw.update(COMMON_BAD[case])
    assert _bytes(so, **kw) == OTBX_ERR_INVALID


def test_text_gather_bytes_nothing_to_copy_reaches_no_kernel(so):
    assert _bytes(so, _col(), n=0, perm=None) == 0
    assert _bytes(so, _col(), dst=None, dst_nbytes=0) == 0


# ---- the ctypes mirrors ----

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "otbx.h"
int main(void)
{
    printf("%zu %zu", sizeof(otbx_textcol), sizeof(otbx_textpred));
    printf(" %zu %zu %zu %zu", offsetof(otbx_textcol, bytes),
           offsetof(otbx_textcol, offs), offsetof(otbx_textcol, nulls),
           offsetof(otbx_textcol, nbytes));
    printf(" %zu %zu %zu %zu %zu %zu\n", offsetof(otbx_textpred, left),
           offsetof(otbx_textpred, right), offsetof(otbx_textpred, op),
           offsetof(otbx_textpred, encoding), offsetof(otbx_textpred, clen),
           offsetof(otbx_textpred, cbytes));
    printf("%d %d %d %d %d\n", OTBX_TXT_LIKE, OTBX_TXT_GE, OTBX_TEXT_SB,
           OTBX_TEXT_UTF8, OTBX_MAX_TEXT_CONST);
    return 0;
}
"""


def test_text_structs_match_the_c_layout(tmp_path):
    assert C.sizeof(TextColDev) == 32 and C.sizeof(TextPredDev) == 312
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run(
        [str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T, P = TextColDev, TextPredDev
    assert got == [C.sizeof(T), C.sizeof(P), T.bytes.offset, T.offs.offset,
                   T.nulls.offset, T.nbytes.offset, P.left.offset,
                   P.right.offset, P.op.offset, P.encoding.offset,
                   P.clen.offset, P.cbytes.offset,
                   _lib.TXT_OPS["like"], _lib.TXT_OPS[">="],
                   _lib.TEXT_ENCODINGS["sb"], _lib.TEXT_ENCODINGS["utf8"],
                   _lib.MAX_TEXT_CONST]
    assert [_lib.TXT_OPS[o] for o in ("like", "not like", "=", "<>", "<",
                                      "<=", ">", ">=")] == list(range(8))


# ---- GpuText / GpuTextPred argument checks (CPU tensors, nothing runs) ----

def _cpu_text(n=4, nulls=False):
    import torch
    return ex.GpuText(bytes=torch.zeros(8, dtype=torch.uint8),
                      offs=torch.arange(n + 1, dtype=torch.int64),
                      nulls=torch.zeros(n, dtype=torch.uint8) if nulls
                      else None)


def test_gputext_adopts_tensors_and_slices():
    import torch
    t = _cpu_text(4, nulls=True)
    assert len(t) == 4
    c = t.col()
    assert c.bytes == t.bytes.data_ptr() and c.nbytes == 8
    assert c.offs == t.offs.data_ptr() and c.nulls == t.nulls.data_ptr()
    s = t.slice(1, 3)
    assert len(s) == 2 and s.bytes is t.bytes
    assert s.col().offs == t.offs.data_ptr() + 8
    assert s.col().nulls == t.nulls.data_ptr() + 1
    assert len(t.slice(2, 2)) == 0
    assert t.to_list() == [b"\0"] * 4
    # to_list clamps like the kernels do
    broken = ex.GpuText(bytes=torch.tensor([65, 66, 67], dtype=torch.uint8),
                        offs=torch.tensor([2, 1, -4, 9, 2], dtype=torch.int64))
    assert broken.to_list() == [b"", b"", b"ABC", b""]


def test_gputext_and_textpred_argument_checks():
    import torch
    t = _cpu_text()
    u8 = torch.zeros(8, dtype=torch.uint8)
    o = torch.arange(5, dtype=torch.int64)
    bad = [
        lambda: ex.GpuText([b"a"], bytes=u8, offs=o),          # both forms
        lambda: ex.GpuText([b"a", 7]),                         # not text
        lambda: ex.GpuText(bytes=u8),                          # no offs
        lambda: ex.GpuText(bytes=u8.to(torch.int32), offs=o),
        lambda: ex.GpuText(bytes=u8, offs=o.to(torch.int32)),
        lambda: ex.GpuText(bytes=u8, offs=o[:0]),              # n + 1 >= 1
        lambda: ex.GpuText(bytes=u8, offs=o[::2]),             # strided
        lambda: ex.GpuText(bytes=u8, offs=o, nulls=u8[:3]),    # mask length
        lambda: ex.GpuText(bytes=u8, offs=o, nulls=o[:4]),     # mask dtype
        lambda: t.slice(3, 2),
        lambda: t.slice(0, 5),
        lambda: t.gather([0, 1]),                              # not a tensor
        lambda: t.gather(torch.zeros(2, dtype=torch.int32)),
        lambda: ex.GpuTextPred(u8, "like", "a%"),              # not a GpuText
        lambda: ex.GpuTextPred(t, "ilike", "a%"),
        lambda: ex.GpuTextPred(t, "~~", "a%"),
        lambda: ex.GpuTextPred(t, "like", "a%", encoding="latin1"),
        lambda: ex.GpuTextPred(t, "like", _cpu_text()),        # column pattern
        lambda: ex.GpuTextPred(t, "not like", _cpu_text()),
        lambda: ex.GpuTextPred(t, "=", _cpu_text(3)),          # lengths
        lambda: ex.GpuTextPred(t, "=", 5),
        lambda: ex.GpuTextPred(t, "=", None),
        lambda: ex.GpuTextPred(t, "=", b"x" * 257),
        lambda: ex.GpuTextPred(t, "like", "abc\\"),            # lone escape
        lambda: ex.GpuTextPred(t, "not like", "a\\\\\\"),
        lambda: ex.GpuTextPred(t, "=", "a", sel=[0, 1]),
        lambda: ex.GpuTextPred(t, "=", "a",
                               sel=torch.zeros(2, dtype=torch.int32)),
        lambda: ex.GpuTextPred(_cpu_text(0), "=", "a",
                               sel=torch.zeros(2, dtype=torch.int64)),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(_lib.OtbxError) as e:
            make()
        assert e.value.status == 3, i
    # what is fine: 256 bytes, an escaped backslash at the end, a lone
    # backslash in a comparison constant
    ex.GpuTextPred(t, "like", "a" * 256)
    ex.GpuTextPred(t, "like", "a\\\\")
    ex.GpuTextPred(t, "=", "a\\")
    node = ex.GpuTextPred(t, "<=", _cpu_text(nulls=True), encoding="sb")
    assert node.nullable and node.n == 4 and node.explain() is None
    p, right = node.pred()
    assert p.op == 5 and p.encoding == 0 and p.clen == 0
    assert p.right.contents.nulls == right.nulls
    p, right = ex.GpuTextPred(t, "like", "%gr\\%").pred()
    assert right is None and not p.right
    assert p.clen == 5 and bytes(p.cbytes[:5]) == b"%gr\\%"
    with pytest.raises(_lib.OtbxError):
        node.ExecCustomScan()           # before BeginCustomScan

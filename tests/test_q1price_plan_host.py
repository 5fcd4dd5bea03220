"""otbx_q1price_plan is pure host code: the layout of the packed Q1 price word
(include/otbx.h) is checked here without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from opentenbase_amd import _lib
from opentenbase_amd._lib import LineitemDev, Q1CodeDesc, Q1PriceDesc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUL = (1.0, 0.1, 0.01, 0.001, 0.0001)
BAD = (1, 0, 0, 0, 0)   # one candidate: (bad, kmin, kmax, dmin, dmax)
SENTINEL = (-7, 3.5, -11, 13, 17, -19, 23, 29)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def fields(d):
    return (d.scale_exp, d.mul, d.k_base, d.k_off, d.k_bits, d.d_base,
            d.d_off, d.d_bits)


def plan(so, cands):
    """cands: five (bad, kmin, kmax, dmin, dmax), one per exponent 0..4.
    Returns the descriptor, or None when nothing fits (then the descriptor
    must be untouched)."""
    assert len(cands) == 5
    bad = (C.c_int32 * 5)(*[c[0] for c in cands])
    cols = [(C.c_int64 * 5)(*[c[k] for c in cands]) for k in (1, 2, 3, 4)]
    d = Q1PriceDesc(*SENTINEL)
    fits = C.c_int32(-1)
    assert so.otbx_q1price_plan(bad, *cols, C.byref(d), C.byref(fits)) == 0
    assert fits.value in (0, 1)
    if not fits.value:
        assert fields(d) == SENTINEL
        return None
    assert d.mul == MUL[d.scale_exp]
    assert d.k_off == 0 and d.d_off == d.k_bits   # K lowest, delta above it
    assert d.k_bits + d.d_bits <= 32 and d.d_bits <= 8
    return d


def only(e, cand):
    return [cand if k == e else BAD for k in range(5)]


def test_generator_domain_is_27_bits(so):
    d = plan(so, only(2, (0, 90_000, 10_500_000, -2, 2)))
    assert fields(d) == (2, 0.01, 90_000, 0, 24, -2, 24, 3)


def test_fewest_bits_win(so):
    # e=1: 10 + 2 bits, e=2: 14 + 0, e=3: 17 + 0, e=0 and e=4 do not fit
    cands = [(0, 0, 100, 0, 10**6),
             (0, 1000, 2000, 0, 3),
             (0, 10_000, 20_000, 1, 1),
             (0, 100_000, 200_000, 0, 0),
             BAD]
    d = plan(so, cands)
    assert (d.scale_exp, d.k_bits, d.d_bits) == (1, 10, 2)
    assert (d.k_base, d.d_base) == (1000, 0)
    cands[2] = (0, 10_000, 10_500, 1, 1)           # now 9 + 0 bits
    d = plan(so, cands)
    assert (d.scale_exp, d.k_bits, d.d_bits, d.d_base) == (2, 9, 0, 1)


def test_tie_goes_to_smaller_exponent(so):
    c = (0, 0, 1023, 0, 3)                          # 10 + 2 bits
    for first in range(5):
        cands = [c if e >= first else BAD for e in range(5)]
        assert plan(so, cands).scale_exp == first
    # same total from different splits: still the smaller e
    d = plan(so, [BAD, (0, 0, 255, 0, 15), (0, 0, 1023, 0, 3), BAD, BAD])
    assert (d.scale_exp, d.k_bits, d.d_bits) == (1, 8, 4)


def test_single_valued_column(so):
    d = plan(so, only(2, (0, 123_456, 123_456, -1, -1)))
    assert fields(d) == (2, 0.01, 123_456, 0, 0, -1, 0, 0)


def test_32_and_33_bit_boundary(so):
    d = plan(so, only(2, (0, 0, 2**24 - 1, 0, 255)))        # 24 + 8
    assert (d.k_bits, d.d_bits, d.d_off) == (24, 8, 24)
    assert plan(so, only(2, (0, 0, 2**24, 0, 255))) is None  # 25 + 8
    d = plan(so, only(0, (0, -2**31, 2**31 - 1, 5, 5)))     # 32 + 0
    assert (d.k_base, d.k_bits, d.d_bits, d.d_off) == (-2**31, 32, 0, 32)
    assert plan(so, only(0, (0, -2**31, 2**31 - 1, 5, 6))) is None  # 32 + 1
    d = plan(so, only(3, (0, 7, 7 + 2**29 - 1, -3, 3)))     # 29 + 3
    assert (d.k_bits, d.d_bits) == (29, 3)
    assert plan(so, only(3, (0, 7, 7 + 2**29, -3, 3))) is None      # 30 + 3


def test_nine_delta_bits_do_not_fit(so):
    d = plan(so, only(2, (0, 0, 1000, -128, 127)))          # span 255
    assert (d.d_bits, d.d_base) == (8, -128)
    assert plan(so, only(2, (0, 0, 1000, -128, 128))) is None   # span 256
    assert plan(so, only(2, (0, 5, 5, 0, 256))) is None     # 0 + 9 bits


def test_all_bad_leaves_descriptor_untouched(so):
    assert plan(so, [BAD] * 5) is None
    # the statistics of a bad candidate are ignored, whatever they hold
    assert plan(so, [(1, 0, 10, 0, 1)] * 5) is None


def test_negative_base_and_span_crossing_zero(so):
    d = plan(so, only(2, (0, -10_500_000, -90_000, -2, 2)))
    assert (d.k_base, d.k_bits, d.d_base, d.d_bits) == (-10_500_000, 24, -2, 3)
    d = plan(so, only(1, (0, -5, 10, -1, 0)))
    assert (d.k_base, d.k_bits, d.d_base, d.d_bits) == (-5, 4, -1, 1)
    d = plan(so, only(0, (0, -2**31, -2**31 + 1, 0, 0)))
    assert (d.k_base, d.k_bits) == (-2**31, 1)


def test_differences_are_formed_in_64_bit(so):
    # kmax - kmin = 2^32 - 1 needs 32 bits, not a wrapped -1
    d = plan(so, only(0, (0, -2**31, 2**31 - 1, 0, 0)))
    assert d.k_bits == 32
    # a delta range as wide as int64 must not wrap into a small width
    assert plan(so, only(2, (0, 0, 10, -2**63, 2**63 - 1))) is None
    assert plan(so, only(2, (0, 0, 10, -2**63, -2**63 + 1))) is None
    # d_base is an int32: corrections outside it do not fit
    assert plan(so, only(2, (0, 0, 10, 2**31, 2**31))) is None
    assert plan(so, only(2, (0, 0, 10, -2**31 - 1, -2**31 - 1))) is None
    d = plan(so, only(2, (0, 0, 10, 2**31 - 2, 2**31 - 1)))
    assert (d.d_base, d.d_bits) == (2**31 - 2, 1)
    # K outside int32 cannot be a field base either
    assert plan(so, only(2, (0, 2**31, 2**31, 0, 0))) is None
    # an empty range (min above max: no row was seen) does not fit
    assert plan(so, only(2, (0, 2**31 - 1, -2**31, 0, 0))) is None


def test_null_pointers_are_invalid(so):
    bad = (C.c_int32 * 5)()
    a = (C.c_int64 * 5)()
    d, fits = Q1PriceDesc(), C.c_int32(0)
    good = [bad, a, a, a, a, C.byref(d), C.byref(fits)]
    assert so.otbx_q1price_plan(*good) == 0
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert so.otbx_q1price_plan(*args) == 3, k


def test_struct_mirrors_match_header(tmp_path):
    """Q1PriceDesc / LineitemDev (ctypes) against the C header: size and
    member offsets of the new descriptor, the offsets of the appended
    fields, and q1code / q1desc where they were."""
    cc = os.environ.get("CC", "cc")
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "otbx.h"\n'
        "#define O(m) offsetof(otbx_q1price_desc, m)\n"
        "#define L(m) offsetof(otbx_lineitem_dev, m)\n"
        "int main(void) {\n"
        '    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ",\n'
        "           sizeof(otbx_q1price_desc), O(scale_exp), O(mul),\n"
        "           O(k_base), O(k_off), O(k_bits), O(d_base), O(d_off),\n"
        "           O(d_bits), sizeof(otbx_q1code_desc));\n"
        '    printf("%zu %zu %zu %zu %zu",\n'
        "           sizeof(otbx_lineitem_dev), L(q1code), L(q1desc),\n"
        "           L(q1pcode), L(q1pdesc));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run(
        [str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = Q1PriceDesc
    assert got == [C.sizeof(P), P.scale_exp.offset, P.mul.offset,
                   P.k_base.offset, P.k_off.offset, P.k_bits.offset,
                   P.d_base.offset, P.d_off.offset, P.d_bits.offset,
                   C.sizeof(Q1CodeDesc),
                   C.sizeof(LineitemDev), LineitemDev.q1code.offset,
                   LineitemDev.q1desc.offset, LineitemDev.q1pcode.offset,
                   LineitemDev.q1pdesc.offset]
    assert C.sizeof(P) == 40 and C.sizeof(Q1CodeDesc) == 72
    # appended at the end: nothing before them moved
    assert LineitemDev.q1code.offset == 104
    assert LineitemDev.q1desc.offset == 112
    assert LineitemDev.q1pcode.offset == 112 + 72
    assert LineitemDev.q1pdesc.offset == 192
    assert C.sizeof(LineitemDev) == 232

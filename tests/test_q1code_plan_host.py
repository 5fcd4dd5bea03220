"""otbx_q1code_plan is pure host code: the layout of the packed Q1 code word
(include/otbx.h) is checked here without a GPU."""
import ctypes as C
import subprocess
import os

import pytest

from opentenbase_amd import _lib
from opentenbase_amd._lib import LineitemDev, Q1CodeDesc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def plan(so, nq, nd, nt, span):
    d = Q1CodeDesc()
    d.date_base = -77            # the plan must leave these three alone
    d.gid_present = 0x2a
    d.dict = 0x1234
    fits = C.c_int32(-1)
    assert so.otbx_q1code_plan(nq, nd, nt, span, C.byref(d), C.byref(fits)) == 0
    assert (d.date_base, d.gid_present, d.dict) == (-77, 0x2a, 0x1234)
    assert fits.value in (0, 1)
    return d if fits.value else None


def widths(d):
    return (d.date_bits, d.gid_bits, d.qty_bits, d.disc_bits, d.tax_bits)


def offsets(d):
    return (d.date_off, d.gid_off, d.qty_off, d.disc_off, d.tax_off)


def test_benchmark_domain_is_29_bits(so):
    d = plan(so, 50, 11, 9, 2525)
    assert widths(d) == (12, 3, 6, 4, 4)
    assert offsets(d) == (0, 12, 15, 21, 25)
    assert sum(widths(d)) == 29
    assert (d.nqty, d.ndisc, d.ntax) == (50, 11, 9)


def test_fields_are_adjacent_and_disjoint(so):
    for args in ((50, 11, 9, 2525), (256, 256, 256, 31), (1, 1, 1, 0),
                 (2, 3, 5, 1), (129, 128, 17, 500)):
        d = plan(so, *args)
        pos = 0
        for off, bits in zip(offsets(d), widths(d)):
            assert off == pos
            pos += bits
        assert pos <= 32


def test_power_of_two_sizes(so):
    # ceil(log2(size)): 2 -> 1, 3 -> 2, 4 -> 2, 5 -> 3, 128 -> 7, 129 -> 8
    for size, bits in ((1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (128, 7),
                       (129, 8), (256, 8)):
        assert plan(so, size, 1, 1, 0).qty_bits == bits
        assert plan(so, 1, size, 1, 0).disc_bits == bits
        assert plan(so, 1, 1, size, 0).tax_bits == bits
    # the date field holds the span itself: 1 -> 1 bit, 2 -> 2, 4095 -> 12
    for span, bits in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 3), (4095, 12),
                       (4096, 13)):
        assert plan(so, 1, 1, 1, span).date_bits == bits


def test_32_and_33_bit_boundary(so):
    d = plan(so, 256, 256, 256, 31)            # 5 + 3 + 24 = 32
    assert widths(d) == (5, 3, 8, 8, 8) and d.tax_off + d.tax_bits == 32
    assert plan(so, 256, 256, 256, 32) is None  # 6 + 3 + 24 = 33
    d = plan(so, 1, 1, 1, 2**29 - 1)            # 29 + 3 = 32
    assert widths(d) == (29, 3, 0, 0, 0)
    assert plan(so, 1, 1, 1, 2**29) is None     # 30 + 3 = 33
    assert plan(so, 2, 1, 1, 2**29 - 1) is None
    assert plan(so, 1, 1, 1, 2**32 - 1) is None
    assert plan(so, 1, 1, 1, 2**32) is None
    assert plan(so, 1, 1, 1, 2**63) is None


def test_all_single_valued(so):
    d = plan(so, 1, 1, 1, 0)
    assert widths(d) == (0, 3, 0, 0, 0)
    assert offsets(d) == (0, 0, 3, 3, 3)


def test_sizes_out_of_range_rejected(so):
    assert plan(so, 257, 1, 1, 0) is None
    assert plan(so, 1, 257, 1, 0) is None
    assert plan(so, 1, 1, 257, 0) is None
    assert plan(so, 0, 1, 1, 0) is None
    assert plan(so, 1, -1, 1, 0) is None


def test_null_pointers_are_invalid(so):
    fits = C.c_int32(0)
    assert so.otbx_q1code_plan(1, 1, 1, 0, None, C.byref(fits)) == 3
    assert so.otbx_q1code_plan(1, 1, 1, 0, C.byref(Q1CodeDesc()), None) == 3


def test_struct_mirrors_match_header(tmp_path):
    """Q1CodeDesc / LineitemDev (ctypes) against the C header: sizes, and the
    offsets of the appended fields; the fields before them did not move."""
    cc = os.environ.get("CC", "cc")
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "otbx.h"\n'
        "int main(void) {\n"
        '    printf("%zu %zu %zu %zu %zu %zu %zu",\n'
        "           sizeof(otbx_q1code_desc), offsetof(otbx_q1code_desc, dict),\n"
        "           sizeof(otbx_lineitem_dev),\n"
        "           offsetof(otbx_lineitem_dev, l_partkey32),\n"
        "           offsetof(otbx_lineitem_dev, q1code),\n"
        "           offsetof(otbx_lineitem_dev, q1desc),\n"
        "           offsetof(otbx_q1code_desc, nqty));\n"
        "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run(
        [str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(Q1CodeDesc), Q1CodeDesc.dict.offset,
                   C.sizeof(LineitemDev), LineitemDev.l_partkey32.offset,
                   LineitemDev.q1code.offset, LineitemDev.q1desc.offset,
                   Q1CodeDesc.nqty.offset]
    assert C.sizeof(Q1CodeDesc) == 72
    assert LineitemDev.l_partkey32.offset == 96   # as before this cache

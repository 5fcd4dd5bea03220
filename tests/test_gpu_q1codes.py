"""The staged packed Q1 code column (otbx.h q1code): the build
round-trips bit-exactly, the coded kernels (variants 3-5) agree with the
raw-column kernel (variant 2) on the same table, the fit rule and the
fallback behave as the header says."""
import ctypes as C

import numpy as np
import pytest

from q1_ref import gid_of, host_cols, ref_q1_partial

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REL = 1e-6          # the parity bar against the oracle (test_gpu_parity.REL)
REL_VARIANTS = 1e-12  # between kernel variants (test_q1_variants_agree_sf1)
DICT = 256


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def ora():
    from oracle import oracle_py
    return oracle_py


def run_variant(li, cutoff, variant):
    from opentenbase_amd._lib import call
    sums = torch.empty((6, 5), dtype=torch.float64, device="cuda")
    counts = torch.empty(6, dtype=torch.int64, device="cuda")
    ms = C.c_float(0.0)
    call("otbx_q1_partial_variant", C.byref(li.cstruct), C.c_int32(cutoff),
         C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()),
         C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ms),
         C.c_int(variant))
    return sums.cpu().numpy().copy(), counts.cpu().numpy().copy()


def run_default(ex, li, cutoff):
    node = ex.GpuQ1PartialAgg(li, cutoff=cutoff)
    node.BeginCustomScan()
    node._rows = node._run()
    s, c = node.partial_state_tensors()
    return s.cpu().numpy().copy(), c.cpu().numpy().copy()


def assert_same(got, ref, what=""):
    (s, c), (rs, rc) = got, ref
    assert (c == rc).all(), (what, c, rc)
    rel = np.abs(s - rs) / np.maximum(np.abs(rs), 1e-300)
    print(what, "max rel diff of sums", rel.max())
    assert rel.max() < REL_VARIANTS, (what, rel.max())


def built(li):
    return bool(li.cstruct.q1code)


def decode(li):
    """numpy decode of the code column through the descriptor."""
    d = li.cstruct.q1desc
    codes = li._q1code.cpu().numpy().view(np.uint32).astype(np.uint64)
    dic = li._q1dict.cpu().numpy().view(np.uint64)

    def field(off, bits):
        return (codes >> np.uint64(off)) & np.uint64((1 << bits) - 1)

    return {
        "l_shipdate": d.date_base + field(d.date_off, d.date_bits).astype(np.int64),
        "gid": field(d.gid_off, d.gid_bits).astype(np.uint32),
        "l_quantity": dic[field(d.qty_off, d.qty_bits).astype(np.int64)],
        "l_discount": dic[DICT + field(d.disc_off, d.disc_bits).astype(np.int64)],
        "l_tax": dic[2 * DICT + field(d.tax_off, d.tax_bits).astype(np.int64)],
    }


def assert_round_trip(li):
    dec = decode(li)
    for col in ("l_quantity", "l_discount", "l_tax"):
        raw = li.t[col].cpu().numpy().view(np.uint64)
        assert np.array_equal(dec[col], raw), col
    assert np.array_equal(dec["l_shipdate"],
                          li.t["l_shipdate"].cpu().numpy().astype(np.int64))
    assert np.array_equal(dec["gid"],
                          gid_of(li.t["l_returnflag"].cpu().numpy(),
                                 li.t["l_linestatus"].cpu().numpy()))
    d = li.cstruct.q1desc
    assert d.gid_present == int(np.bitwise_or.reduce(1 << dec["gid"]))
    for base, n in ((0, d.nqty), (DICT, d.ndisc), (2 * DICT, d.ntax)):
        dic = li._q1dict.cpu().numpy().view(np.uint64)[base:base + n]
        assert (np.diff(dic.astype(object)) > 0).all()   # sorted, distinct


N_CRAFT = 4099


def test_round_trip(ex):
    li = ex.GpuLineitem.generate(400_003, with_orderkey=False)
    assert built(li)
    d = li.cstruct.q1desc
    assert (d.nqty, d.ndisc, d.ntax) == (50, 11, 9)
    assert d.date_base == int(li.t["l_shipdate"].min().item())
    assert_round_trip(li)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 4099, 400_003, 2_097_157])
def test_coded_vs_raw(ex, n):
    li = ex.GpuLineitem.generate(n, with_orderkey=False)
    assert built(li)
    base = li.cstruct.q1desc.date_base
    dmax = int(li.t["l_shipdate"].max().item())
    for cutoff in (2436, 1200, base - 1, base, dmax, dmax + 1,
                   -2**31, 2**31 - 1):
        ref = run_variant(li, cutoff, 2)
        assert_same(run_variant(li, cutoff, 3), ref, f"v3 n={n} cut={cutoff}")
        assert_same(run_variant(li, cutoff, 4), ref, f"v4 n={n} cut={cutoff}")
        assert_same(run_variant(li, cutoff, 5), ref, f"v5 n={n} cut={cutoff}")
        assert_same(run_default(ex, li, cutoff), ref, f"default n={n}")
    assert run_variant(li, base - 1, 3)[1].sum() == 0
    assert run_variant(li, dmax, 3)[1].sum() == n


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 255, 513, 4099])
def test_raw_variants_small_n(ex, n, variant):
    """The raw-column kernels (the fallback of every table whose code column
    does not build) against an exactly summed host reference: every n % 2
    and n % 4, n below one vector, one row past a block multiple. At most
    4099 non-negative terms per sum, so any summation order is within
    n * 2^-53 ~ 4.6e-13 of the exact sum: inside REL_VARIANTS."""
    cols = host_cols(n)
    li = ex.GpuLineitem.from_host(cols, with_orderkey=False)
    for cutoff in (1200, -2**31, 2**31 - 1):
        got = run_variant(li, cutoff, variant)
        assert_same(got, ref_q1_partial(cols, cutoff),
                    f"v{variant} n={n} cut={cutoff}")
        if cutoff != 1200:
            assert got[1].sum() == (0 if cutoff < 0 else n)


def test_coded_vs_oracle(ex, ora):
    n = 400_003
    li = ex.GpuLineitem.generate(n, with_orderkey=False)
    assert built(li)
    node = ex.GpuQ1PartialAgg(li)
    node.BeginCustomScan()
    rows = []
    while (r := node.ExecCustomScan()) is not None:
        rows.append(r)
    node.EndCustomScan()
    rows = ex.q1_finalize(rows)
    og = ora.q1_finalize(ora.q1_partial(ora.gen_tables(n)))
    assert len(rows) == len(og)
    for g, o in zip(rows, og):
        assert g["l_returnflag"] == chr(o.returnflag)
        assert g["l_linestatus"] == chr(o.linestatus)
        assert g["count_order"] == o.count_order
        for fld, ov in [("sum_qty", o.sum_qty),
                        ("sum_base_price", o.sum_base_price),
                        ("sum_disc_price", o.sum_disc_price),
                        ("sum_charge", o.sum_charge), ("avg_qty", o.avg_qty),
                        ("avg_price", o.avg_price), ("avg_disc", o.avg_disc)]:
            assert abs(g[fld] - ov) <= REL * max(abs(g[fld]), abs(ov), 1e-300), \
                (fld, g[fld], ov)


def test_too_many_distinct_values_not_built(ex):
    cols = host_cols(N_CRAFT,
                     l_discount=(np.arange(N_CRAFT) % 300) / 1000.0)
    li = ex.GpuLineitem.from_host(cols, with_orderkey=False)
    assert not built(li) and li._q1code is None
    assert_same(run_default(ex, li, 2436), run_variant(li, 2436, 2))
    with pytest.raises(ex.OtbxError) as e:
        run_variant(li, 2436, 3)
    assert e.value.status == 3


def wide_cols(date_span):
    """256 distinct values per measure column (3 x 8 bits) + gid 3 bits; the
    date field takes the rest."""
    i = np.arange(N_CRAFT)
    return host_cols(
        N_CRAFT,
        l_quantity=(i % 256 + 1).astype(np.float64),
        l_discount=((i * 7) % 256) / 1024.0,
        l_tax=((i * 13) % 256) / 2048.0,
        l_shipdate=(1000 + (i * 5) % (date_span + 1)).astype(np.int32))


def test_widths_exactly_32_built(ex):
    li = ex.GpuLineitem.from_host(wide_cols(31), with_orderkey=False)
    assert built(li)
    d = li.cstruct.q1desc
    assert (d.date_bits, d.gid_bits, d.qty_bits, d.disc_bits, d.tax_bits) == \
        (5, 3, 8, 8, 8)
    assert d.tax_off + d.tax_bits == 32
    assert_round_trip(li)
    for cutoff in (1015, 999, 1031, 2436):
        assert_same(run_variant(li, cutoff, 3), run_variant(li, cutoff, 2))


def test_widths_33_not_built(ex):
    li = ex.GpuLineitem.from_host(wide_cols(32), with_orderkey=False)
    assert not built(li)
    assert_same(run_default(ex, li, 1015), run_variant(li, 1015, 2))


def test_signed_zero_and_denormal_round_trip(ex):
    disc = np.where(np.arange(N_CRAFT) % 3 == 0, -0.0,
                    np.where(np.arange(N_CRAFT) % 3 == 1, 0.0, 0.05))
    tax = np.where(np.arange(N_CRAFT) % 2 == 0, 5e-324, 0.02)
    li = ex.GpuLineitem.from_host(
        host_cols(N_CRAFT, l_discount=disc, l_tax=tax), with_orderkey=False)
    assert built(li)
    d = li.cstruct.q1desc
    assert (d.ndisc, d.ntax) == (3, 2)   # +0.0 and -0.0 are two entries
    assert_round_trip(li)
    assert_same(run_variant(li, 2436, 3), run_variant(li, 2436, 2))


def test_single_valued_columns_zero_widths(ex):
    one = np.ones(N_CRAFT)
    cols = host_cols(
        N_CRAFT, l_quantity=one * 17.0, l_discount=one * 0.04,
        l_tax=one * 0.02, l_shipdate=np.full(N_CRAFT, 1234, np.int32),
        l_returnflag=np.full(N_CRAFT, ord("N"), np.uint8),
        l_linestatus=np.full(N_CRAFT, ord("O"), np.uint8))
    li = ex.GpuLineitem.from_host(cols, with_orderkey=False)
    assert built(li)
    d = li.cstruct.q1desc
    assert (d.date_bits, d.qty_bits, d.disc_bits, d.tax_bits) == (0, 0, 0, 0)
    assert_round_trip(li)
    assert d.gid_present == 1 << 3   # (N, O) only
    for cutoff in (1233, 1234, 1235, 2436):
        assert_same(run_variant(li, cutoff, 3), run_variant(li, cutoff, 2))
        assert_same(run_variant(li, cutoff, 5), run_variant(li, cutoff, 2))


def test_unexpected_flag_bytes_same_groups(ex):
    rng = np.random.default_rng(11)
    cols = host_cols(
        N_CRAFT,
        l_returnflag=rng.choice(np.frombuffer(b"ANRXa\x00\xff", np.uint8),
                                N_CRAFT),
        l_linestatus=rng.choice(np.frombuffer(b"FOfZ\x00", np.uint8),
                                N_CRAFT))
    li = ex.GpuLineitem.from_host(cols, with_orderkey=False)
    assert built(li)
    assert_round_trip(li)
    got, ref = run_variant(li, 2436, 3), run_variant(li, 2436, 2)
    assert (got[1] == ref[1]).all()
    assert_same(got, ref)
    assert li.cstruct.q1desc.gid_present == 0x3f
    assert_same(run_variant(li, 2436, 5), ref)


def test_variant3_without_cache_is_invalid(ex):
    li = ex.GpuLineitem(1024, with_orderkey=False)
    assert not built(li)
    for v in (3, 4, 5):
        with pytest.raises(ex.OtbxError) as e:
            run_variant(li, 2436, v)
        assert e.value.status == 3

"""The staged packed Q1 price column (otbx.h q1pcode): the
build round-trips l_extendedprice bit-exactly, the kernels that decode it
(variants 6 and 7) agree with variant 5 and the raw-column kernel (variant 2)
on the same table, the fit rule and the fallback behave as the header says."""
import ctypes as C

import numpy as np
import pytest

import q1_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REL = 1e-6            # the parity bar against the oracle
REL_VARIANTS = 1e-12  # between kernel variants
N_CRAFT = 4099
CUTOFF = 2436


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def ora():
    from oracle import oracle_py
    return oracle_py


def variant_status(li, cutoff, variant):
    """(status, sums, counts) of otbx_q1_partial_variant, without raising."""
    from opentenbase_amd._lib import lib
    sums = torch.empty((6, 5), dtype=torch.float64, device="cuda")
    counts = torch.empty(6, dtype=torch.int64, device="cuda")
    ms = C.c_float(0.0)
    st = lib().otbx_q1_partial_variant(
        C.byref(li.cstruct), C.c_int32(cutoff), C.c_void_p(sums.data_ptr()),
        C.c_void_p(counts.data_ptr()),
        C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(ms),
        C.c_int(variant))
    if st != 0:
        return st, None, None
    return st, sums.cpu().numpy().copy(), counts.cpu().numpy().copy()


def run_variant(li, cutoff, variant):
    st, s, c = variant_status(li, cutoff, variant)
    assert st == 0, (variant, st)
    return s, c


def run_default(ex, li, cutoff):
    node = ex.GpuQ1PartialAgg(li, cutoff=cutoff)
    node.BeginCustomScan()
    node._rows = node._run()
    s, c = node.partial_state_tensors()
    return s.cpu().numpy().copy(), c.cpu().numpy().copy()


def assert_same(got, ref, what=""):
    """Counts equal; sums within REL_VARIANTS, where entries that are the
    same non-finite value (NaN, +-Inf) on both sides count as equal."""
    (s, c), (rs, rc) = got, ref
    assert (c == rc).all(), (what, c, rc)
    same = (s == rs) | (np.isnan(s) & np.isnan(rs))
    with np.errstate(invalid="ignore"):
        rel = np.abs(s - rs) / np.maximum(np.abs(rs), 1e-300)
    rel = np.where(same, 0.0, rel)
    print(what, "max rel diff of sums", rel.max())
    assert not np.isnan(rel).any(), (what, s, rs)
    assert rel.max() < REL_VARIANTS, (what, rel.max())


def built(li):
    return bool(li.cstruct.q1pcode)


def mask(bits):
    return np.uint64((1 << bits) - 1)


def decode_price_bits(li):
    """numpy decode of the price column through the descriptor, as uint64
    bit patterns."""
    d = li.cstruct.q1pdesc
    w = li._q1pcode.cpu().numpy().view(np.uint32).astype(np.uint64)
    kf = (w >> np.uint64(d.k_off)) & mask(d.k_bits)
    df = (w >> np.uint64(d.d_off)) & mask(d.d_bits)
    k = (np.int64(d.k_base) + kf.astype(np.int64)).astype(np.int32)
    pred = k.astype(np.float64) * np.float64(d.mul)
    delta = np.int64(d.d_base) + df.astype(np.int64)
    return pred.view(np.uint64) + delta.astype(np.uint64)   # wraps


def assert_round_trip(li):
    assert built(li) and li._q1pcode is not None
    d = li.cstruct.q1pdesc
    assert 0 <= d.scale_exp <= 4
    assert d.mul == (1.0, 0.1, 0.01, 0.001, 0.0001)[d.scale_exp]
    assert d.k_off == 0 and d.d_off == d.k_bits
    assert d.d_bits <= 8 and d.k_bits + d.d_bits <= 32
    raw = li.t["l_extendedprice"].cpu().numpy().view(np.uint64)
    assert np.array_equal(decode_price_bits(li), raw)


def assert_agrees(ex, li, cutoffs=(CUTOFF,)):
    """variants 6, 7 and the default against variants 5 and 2"""
    for cutoff in cutoffs:
        v2 = run_variant(li, cutoff, 2)
        v5 = run_variant(li, cutoff, 5)
        assert_same(v5, v2, f"v5 vs v2 cut={cutoff}")
        for name, got in (("v6", run_variant(li, cutoff, 6)),
                          ("v7", run_variant(li, cutoff, 7)),
                          ("default", run_default(ex, li, cutoff))):
            assert_same(got, v5, f"{name} vs v5 n={li.n} cut={cutoff}")
            assert_same(got, v2, f"{name} vs v2 n={li.n} cut={cutoff}")


def assert_not_built(ex, li):
    """Q1 runs as without the price column; asking for it is invalid."""
    assert not built(li) and li._q1pcode is None
    assert bool(li.cstruct.q1code)
    ref = run_variant(li, CUTOFF, 2)
    assert_same(run_variant(li, CUTOFF, 5), ref, "v5 vs v2")
    assert_same(run_default(ex, li, CUTOFF), run_variant(li, CUTOFF, 5),
                "default vs v5")
    assert_same(run_default(ex, li, CUTOFF), ref, "default vs v2")
    for v in (6, 7):
        assert variant_status(li, CUTOFF, v)[0] == 3


def host_cols(n, **over):
    """q1_ref.host_cols with two-decimal money prices."""
    return q1_ref.host_cols(n, money=True, **over)


def staged(ex, **over):
    return ex.GpuLineitem.from_host(host_cols(N_CRAFT, **over),
                                    with_orderkey=False)


def test_round_trip_generated(ex):
    li = ex.GpuLineitem.generate(400_003, with_orderkey=False)
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert d.scale_exp == 2 and d.k_bits <= 24 and d.d_bits <= 3
    held = sum(v.numel() * v.element_size()
               for v in list(li.t.values()) + [li._q1code, li._q1dict]
               if v is not None)
    assert li.bytes_staged() == held + 4 * li.n


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 255, 4099, 400_003])
def test_price_coded_vs_others(ex, n):
    li = ex.GpuLineitem.generate(n, with_orderkey=False)
    assert_round_trip(li)
    base = li.cstruct.q1desc.date_base
    dmax = int(li.t["l_shipdate"].max().item())
    assert_agrees(ex, li, (2436, 1200, base - 1, base, dmax, dmax + 1,
                           -2**31, 2**31 - 1))
    for v in (6, 7):
        assert run_variant(li, base - 1, v)[1].sum() == 0
        assert run_variant(li, dmax, v)[1].sum() == n
    assert run_default(ex, li, base - 1)[1].sum() == 0
    assert run_default(ex, li, dmax)[1].sum() == n


def test_default_vs_oracle(ex, ora):
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


def test_two_decimal_money_built(ex):
    li = staged(ex)
    assert_round_trip(li)
    assert li.cstruct.q1pdesc.scale_exp == 2
    assert_agrees(ex, li)


def test_integer_prices_scale_zero(ex):
    rng = np.random.default_rng(3)
    price = rng.integers(900, 105_001, N_CRAFT).astype(np.float64)
    li = staged(ex, l_extendedprice=price)
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    # e = 0 predicts every integer exactly; larger e only widen the K field
    assert (d.scale_exp, d.mul, d.d_bits, d.d_base) == (0, 1.0, 0, 0)
    assert d.k_base == int(price.min())
    assert_agrees(ex, li)


def test_single_valued_price_zero_widths(ex):
    # 1234.56 is 1.9e12 ulp from 1235 and 1.7e11 ulp from 1234.6, so e = 0
    # and 1 have no int32 correction; e = 2, 3, 4 all need 0 + 0 bits and
    # the tie goes to e = 2
    li = staged(ex, l_extendedprice=np.full(N_CRAFT, 1234.56))
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert (d.scale_exp, d.k_base, d.k_bits, d.d_bits) == (2, 123456, 0, 0)
    assert (li._q1pcode == 0).all().item()
    assert_agrees(ex, li, (CUTOFF, -1, 2600))


def test_negative_prices_negative_base(ex):
    rng = np.random.default_rng(5)
    price = -(rng.integers(90_000, 10_500_001, N_CRAFT) / 100.0)
    li = staged(ex, l_extendedprice=price)
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert d.scale_exp == 2 and d.k_base < 0
    assert d.k_base == int(np.rint(price * 100.0).min())
    assert_agrees(ex, li)


def test_three_decimals_scale_three(ex):
    rng = np.random.default_rng(6)
    k = rng.integers(900_000, 105_000_001, N_CRAFT)
    k[:4] = (900_001, 900_005, 104_999_999, 1_234_567)   # third decimal set
    li = staged(ex, l_extendedprice=k / 1000.0)
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert (d.scale_exp, d.mul) == (3, 0.001)
    assert_agrees(ex, li)


def ulp_prices(kmax):
    """Integers 1..kmax, each moved up by 0..255 ulp: at e = 0 the K field
    spans kmax - 1 and the correction exactly 0..255 (8 bits); at e >= 1 the
    K field alone is at least 3 bits wider."""
    rng = np.random.default_rng(8)
    k = rng.integers(1, kmax + 1, N_CRAFT)
    j = rng.integers(0, 256, N_CRAFT)
    k[:2], j[:2] = (1, kmax), (0, 255)
    bits = k.astype(np.float64).view(np.uint64) + j.astype(np.uint64)
    return bits.view(np.float64)


def test_widths_exactly_32_built(ex):
    li = staged(ex, l_extendedprice=ulp_prices(2**24))
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert (d.scale_exp, d.k_base, d.k_bits, d.d_base, d.d_bits, d.d_off) == \
        (0, 1, 24, 0, 8, 24)
    assert_agrees(ex, li)


def test_widths_33_not_built(ex):
    li = staged(ex, l_extendedprice=ulp_prices(2**24 + 1))
    assert_not_built(ex, li)


def full_range_integers():
    """Integer prices over all of (-2^31, 2^31): K needs 32 bits at e = 0 and
    leaves int32 at every other e. All but one value are positive, so the
    sums do not cancel."""
    rng = np.random.default_rng(9)
    k = rng.integers(1, 2**31, N_CRAFT)
    k[:2] = (-(2**31 - 1), 2**31 - 1)
    return k.astype(np.float64)


def test_k_field_of_32_bits_built(ex):
    li = staged(ex, l_extendedprice=full_range_integers())
    assert_round_trip(li)
    d = li.cstruct.q1pdesc
    assert (d.scale_exp, d.k_base, d.k_bits, d.d_bits) == \
        (0, -(2**31 - 1), 32, 0)
    assert_agrees(ex, li)


def test_k_field_of_32_bits_plus_one_not_built(ex):
    price = full_range_integers()
    price[7] = np.nextafter(1000.0, np.inf)   # one correction of +1: 32 + 1
    assert_not_built(ex, staged(ex, l_extendedprice=price))


def test_uniform_random_doubles_not_built(ex):
    rng = np.random.default_rng(7)
    li = staged(ex, l_extendedprice=rng.uniform(900.0, 105000.0, N_CRAFT))
    assert_not_built(ex, li)


@pytest.mark.parametrize("odd", [np.nan, np.inf, -0.0])
def test_one_odd_value_not_built(ex, odd):
    price = host_cols(N_CRAFT)["l_extendedprice"]
    price[1234] = odd
    assert_not_built(ex, staged(ex, l_extendedprice=price))


def test_no_price_code_without_code_column(ex):
    li = staged(ex, l_discount=(np.arange(N_CRAFT) % 300) / 1000.0)
    assert not bool(li.cstruct.q1code) and li._q1code is None
    assert not built(li) and li._q1pcode is None
    assert_same(run_default(ex, li, CUTOFF), run_variant(li, CUTOFF, 2))
    for v in (5, 6, 7):
        assert variant_status(li, CUTOFF, v)[0] == 3


def test_invalid_calls(ex):
    li = ex.GpuLineitem(1024, with_orderkey=False)   # constructed, not staged
    assert not built(li)
    for v in (6, 7, 8):
        assert variant_status(li, CUTOFF, v)[0] == 3
    li = ex.GpuLineitem.generate(1024, with_orderkey=False)
    assert built(li)
    for v in (8, 9):
        assert variant_status(li, CUTOFF, v)[0] == 3

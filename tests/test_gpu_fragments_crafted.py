"""The fused Q3 and Q9-mix fragments on hand-built tables (fragment_ref.py),
through every code path the env hooks and the staged caches select, against
the CPU oracle — which test_fragment_ref_host.py pins to a brute-force
reference on the same cases. All comparisons are ==: the builders keep every
revenue sum exact in float64.

At the commit before the input-domain fixes these fail: the day-0 cases on
the Q3 direct paths and on Q9 (an order dated day 0 with priority 0 was read
as an empty table entry) and the zero-revenue case on all three direct-path
compaction kernels (a group summing to 0.0 was read as "no lineitem
matched")."""
import ctypes as C

import numpy as np
import pytest

import fragment_ref as fr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

Q3_DT = np.dtype([("l_orderkey", "i8"), ("revenue", "f8"),
                  ("o_orderdate", "i4"), ("o_shippriority", "i4")])

Q3_ENVS = ["OTBX_Q3_COMPACT_TILE", "OTBX_Q3_COMPACT_LEGACY",
           "OTBX_DIRECT_CAP", "OTBX_Q3_FORCE_HASH", "OTBX_Q3_HASH_BUDGET"]
Q3_CONFIGS = [
    ("default", {}),
    ("compact_tile", {"OTBX_Q3_COMPACT_TILE": "1"}),
    ("compact_legacy", {"OTBX_Q3_COMPACT_LEGACY": "1"}),
    ("direct_cap", {"OTBX_DIRECT_CAP": "16384"}),
    ("force_hash", {"OTBX_Q3_FORCE_HASH": "1"}),
    ("hash_grace", {"OTBX_Q3_FORCE_HASH": "1",
                    "OTBX_Q3_HASH_BUDGET": "1024"}),
]
Q9_ENVS = ["OTBX_Q9_BITMAP_BITS", "OTBX_Q9_FILTER_WAVE"]
Q9_CONFIGS = [
    ("default", {}, ()),
    ("bitmap_slices", {"OTBX_Q9_BITMAP_BITS": "64"}, ()),
    ("filter_wave", {"OTBX_Q9_FILTER_WAVE": "1"}, ()),
    ("no_q9rec", {}, ("q9rec",)),
    ("no_partkey32", {}, ("l_partkey32",)),
]


@pytest.fixture(scope="module")
def ex():
    from opentenbase_amd import executor
    executor.init_device(0)
    return executor


@pytest.fixture(scope="module")
def ora():
    from oracle import oracle_py
    return oracle_py


def set_env(monkeypatch, names, env):
    for n in names:
        monkeypatch.delenv(n, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class nulled:
    """Null staged-cache pointers of a table's cstruct for the duration (the
    way test_q3_key32_vs_i64_selfconsistent does), then put them back."""

    def __init__(self, table, fields):
        self.cs, self.fields = table.cstruct, fields

    def __enter__(self):
        self.saved = {f: getattr(self.cs, f) for f in self.fields}
        for f in self.fields:
            setattr(self.cs, f, C.c_void_p(0))

    def __exit__(self, *exc):
        for f, v in self.saved.items():
            setattr(self.cs, f, C.c_void_p(v))


_q3_expected = {}


def q3_expected(ora, name):
    """Oracle groups, top-10 and reference hit count of a case, computed
    once and shared."""
    if name not in _q3_expected:
        case = fr.q3_case(name)
        rows = ora.q3_partial(fr.q3_oracle_tables(ora, case),
                              segment=case["segment"], date=case["date"])
        top = [tuple(r) for r in ora.q3_topk(rows, 10)]
        _q3_expected[name] = (fr.q3_rows_to_dict(rows), len(rows), top,
                              fr.q3_ref(case)[1])
    return _q3_expected[name]


def check_q3_case(ex, ora, monkeypatch, name):
    case = fr.q3_case(name)
    exp, exp_n, exp_top, exp_hits = q3_expected(ora, name)
    cu = ex.GpuCustomer.from_host(case["customer"])
    li = ex.GpuLineitem.from_host(case["lineitem"])
    ck = None
    if case["cust_keys"] is not None:
        ck = torch.from_numpy(case["cust_keys"].copy()).cuda()
    for minmax in (True, False):
        od = ex.GpuOrders.from_host(case["orders"], minmax=minmax)
        assert od.cstruct.has_minmax == int(minmax and od.n > 0)
        for cfg, env in Q3_CONFIGS:
            set_env(monkeypatch, Q3_ENVS, env)
            for key32 in (True, False):
                what = (name, cfg, "minmax" if minmax else "no-minmax",
                        "key32" if key32 else "i64")
                with nulled(li, () if key32 else ("l_orderkey32",)), \
                        nulled(od, () if key32 else ("o_orderkey32",
                                                     "o_custkey32")):
                    node = ex.GpuQ3Fragment(cu, od, li,
                                            segment=case["segment"],
                                            date=case["date"], cust_keys=ck)
                    node.BeginCustomScan()
                    top = node._run()
                    got = fr.q3_rows_to_dict(node.fetch_groups())
                assert set(got) == set(exp), what
                assert got == exp, what     # revenue, date, priority
                assert node.ngroups == exp_n, what
                assert node.probe_hits == exp_hits, what
                assert top == exp_top, what


Q3_SMALL = [n for n in fr.Q3_CASES if not n.startswith("sizes_")]


@pytest.mark.parametrize("name", Q3_SMALL)
def test_q3_crafted(ex, ora, monkeypatch, name):
    check_q3_case(ex, ora, monkeypatch, name)


@pytest.mark.parametrize("norders", fr.SIZES)
def test_q3_crafted_sizes(ex, ora, monkeypatch, norders):
    for nl in fr.SIZES:
        check_q3_case(ex, ora, monkeypatch, f"sizes_{norders}_{nl}")


def test_q3_crafted_cases_take_the_paths_they_name(ex, monkeypatch):
    """The staged int32 caches exist where a case relies on them and are
    void where its keys leave [0, 2^31)."""
    set_env(monkeypatch, Q3_ENVS, {})
    case = fr.q3_case("shuffled")
    li = ex.GpuLineitem.from_host(case["lineitem"])
    od = ex.GpuOrders.from_host(case["orders"])
    assert li.cstruct.l_orderkey32 and od.cstruct.o_orderkey32 \
        and od.cstruct.o_custkey32
    assert (od.cstruct.okey_min, od.cstruct.okey_max) == (1, 500)
    case = fr.q3_case("key_domain")
    li = ex.GpuLineitem.from_host(case["lineitem"])
    od = ex.GpuOrders.from_host(case["orders"])
    assert not li.cstruct.l_orderkey32 and not od.cstruct.o_orderkey32 \
        and not od.cstruct.o_custkey32
    assert od.cstruct.okey_min == -2**62
    assert od.cstruct.okey_max == fr.I64_MAX - 1


@pytest.mark.parametrize("name", list(fr.Q9_CASES))
def test_q9_crafted(ex, ora, monkeypatch, name):
    case = fr.q9_case_get(name)
    rows = ora.q9_partial(fr.q9_oracle_tables(ora, case),
                          typemod=case["typemod"], typeval=case["typeval"])
    exp_s, exp_c = [0.0] * 7, [0] * 7
    for r in rows:
        exp_s[r.year], exp_c[r.year] = float(r.revenue), int(r.count_rows)
    ref = fr.q9_ref(case)
    assert {y: (exp_s[y], exp_c[y]) for y in range(7) if exp_c[y]} == ref
    pt = ex.GpuPart.from_host(case["part"])
    li = ex.GpuLineitem.from_host(case["lineitem"], with_partkey=True)
    for minmax in (True, False):
        od = ex.GpuOrders.from_host(case["orders"], minmax=minmax)
        for cfg, env, null in Q9_CONFIGS:
            set_env(monkeypatch, Q9_ENVS, env)
            what = (name, cfg, "minmax" if minmax else "no-minmax")
            with nulled(li, null):
                node = ex.GpuQ9Fragment(pt, od, li, typemod=case["typemod"],
                                        typeval=case["typeval"])
                node.BeginCustomScan()
                node._run()
                s, c = node.partial_state_tensors()
                s, c = s.cpu().numpy().tolist(), c.cpu().numpy().tolist()
            assert c == exp_c, what
            assert s == exp_s, what


def test_q9_sparse_order_keys_refused(ex, monkeypatch):
    """An order-key range wider than norders * nranks does not fit the date
    table: refused with OTBX_ERR_INVALID before any kernel indexes it."""
    from opentenbase_amd._lib import OtbxError
    set_env(monkeypatch, Q9_ENVS, {})
    case = fr.q9_case_get("type_all")
    orders = {k: v[:2].copy() for k, v in case["orders"].items()}
    orders["o_orderkey"][:] = [1, 1000]
    pt = ex.GpuPart.from_host(case["part"])
    li = ex.GpuLineitem.from_host(
        {k: v[:64] for k, v in case["lineitem"].items()}, with_partkey=True)
    for minmax in (True, False):
        od = ex.GpuOrders.from_host(orders, minmax=minmax)
        node = ex.GpuQ9Fragment(pt, od, li, typemod=1, typeval=0)
        node.BeginCustomScan()
        with pytest.raises(OtbxError) as e:
            node._run()
        assert e.value.status == 3


# ---- top-k and ORDER BY through the raw C ABI ----

def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _groups(keys, revs, dates):
    g = np.zeros(len(keys), dtype=Q3_DT)
    g["l_orderkey"], g["revenue"], g["o_orderdate"] = keys, revs, dates
    g["o_shippriority"] = np.arange(len(keys)) % 3
    return g


GUARD = 0xA5


def run_topk(groups, k, cap_cand):
    """-> (ncand, candidates written, guard region intact)."""
    from opentenbase_amd._lib import call
    n = len(groups)
    gdev = torch.from_numpy(groups.view(np.uint8).reshape(-1).copy()).cuda()
    nguard = 64 * 24
    cand = torch.full((cap_cand * 24 + nguard,), GUARD, dtype=torch.uint8,
                      device="cuda")
    ncand = torch.zeros(1, dtype=torch.int64, device="cuda")
    hist = torch.empty(16384, dtype=torch.int32, device="cuda")
    call("otbx_topk_by_revenue", C.c_void_p(gdev.data_ptr()), C.c_int64(n),
         C.c_int64(k), C.c_void_p(cand.data_ptr()), C.c_int64(cap_cand),
         C.c_void_p(ncand.data_ptr()), C.c_void_p(hist.data_ptr()), _stream())
    nc = int(ncand.cpu().item())
    host = cand.cpu().numpy()
    got = host[: min(nc, cap_cand) * 24].copy().view(Q3_DT)
    return nc, got, bool(np.all(host[cap_cand * 24:] == GUARD))


def host_topk(ex, cands, k):
    return [tuple(r) for r in ex.q3_topk(cands, k)]


def test_topk_crafted(ex, ora):
    rng = np.random.default_rng(3)
    n = 1000
    keys = rng.permutation(np.arange(1, n + 1))
    dates = rng.integers(0, 2000, n)
    cases = {
        "all_equal": _groups(keys, np.full(n, 64.0), dates),
        # 40 distinct revenues, 25 rows each: the k-th place is always tied
        "ties_at_kth": _groups(keys, 4.0 * (1 + np.arange(n) % 40), dates),
        "ties_same_date": _groups(keys, 4.0 * (1 + np.arange(n) % 40),
                                  np.full(n, 7)),
        "zero_present": _groups(keys, 4.0 * (np.arange(n) % 3), dates),
        "negative_present": _groups(keys, 4.0 * (np.arange(n) % 9 - 4.0),
                                    dates),
        "all_zero_or_negzero": _groups(keys, np.where(keys % 2, 0.0, -0.0),
                                       dates),
    }
    for name, g in cases.items():
        for k in (1, 10, n):
            nc, got, guard_ok = run_topk(g, k, cap_cand=n)
            assert guard_ok, (name, k)
            assert k <= nc <= n, (name, k, nc)
            exp = [tuple(r) for r in ora.q3_topk(g, k)]
            assert host_topk(ex, got, k) == exp, (name, k)


def test_topk_cap_smaller_than_candidates(ex):
    """cap_cand below the candidate count: *ncand is the TRUE count and
    nothing is written past cap_cand entries."""
    n = 5000
    g = _groups(np.arange(1, n + 1), np.full(n, 64.0), np.arange(n) % 100)
    for cap in (1, 7, 64, 4999):
        nc, got, guard_ok = run_topk(g, 10, cap_cand=cap)
        assert nc == n, cap          # all revenues equal: all are candidates
        assert guard_ok, cap
        assert len(got) == cap and np.all(got["revenue"] == 64.0)
        assert len(set(got["l_orderkey"].tolist())) == cap  # real, distinct
        assert np.all((got["l_orderkey"] >= 1) & (got["l_orderkey"] <= n))


def test_order_groups_crafted(ex):
    """ORDER BY revenue DESC, o_orderdate ASC against np.lexsort: revenue
    ties broken by date, revenue 0.0 present, dates inside [0, 2^16)."""
    rng = np.random.default_rng(4)
    n = 3000
    keys = np.arange(1, n + 1)
    revs = 4.0 * rng.integers(0, 12, n)            # many ties, zeros
    revs[::17] = -0.0                              # ties with +0.0
    dates = rng.integers(0, 2**16, n)
    dates[:4] = [0, 2**16 - 1, 255, 256]
    g = _groups(keys, revs, dates)
    gdev = torch.from_numpy(g.view(np.uint8).reshape(-1).copy()).cuda()
    got = ex.order_groups(gdev, n)
    # the sort is stable by input order on full ties: lexsort's last key is
    # the primary one, and lexsort is stable too
    order = np.lexsort((g["o_orderdate"], -g["revenue"]))
    exp = g[order]
    assert np.array_equal(got["revenue"], exp["revenue"])
    assert np.array_equal(got["o_orderdate"], exp["o_orderdate"])
    assert np.array_equal(got["l_orderkey"], exp["l_orderkey"])
    assert np.array_equal(got["o_shippriority"], exp["o_shippriority"])

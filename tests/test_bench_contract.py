"""CPU-side guards on bench.py's contract pieces: the cpu_baseline leg (runs
the oracle CLI) and the committed roofline-traffic file."""
import importlib.util
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cpu_baseline_object():
    b = _bench()
    cb = b.cpu_baseline("q1", 2_000_000)
    assert cb["kind"] == "port" and cb["cores"] == 1
    assert cb["unit"] == "rows/s" and cb["value"] > 0
    assert "scalar" in cb["sample"]


def test_cpu_baseline_q3():
    b = _bench()
    cb = b.cpu_baseline("q3", 1_000_000)
    assert cb["value"] > 0


def test_traffic_file_parses():
    b = _bench()
    t = b.load_traffic("tpch_q1", 100)
    assert t is not None and 20e9 < t < 30e9  # ≈ algorithmic 22.8 GB
    assert b.load_traffic("tpch_q1", 10) is None  # sf mismatch → null
    assert b.load_traffic("nope", 100) is None


def test_committed_bench_snapshots_schema():
    for f in ("r01_bench_q1.json", "r01_bench_q3.json"):
        with open(os.path.join(REPO, "profiles", f)) as fh:
            d = json.load(fh)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling", "dtype",
                  "data", "config", "roofline"):
            assert k in d, k
        assert d["roofline"]["bound"] == "hbm"
        assert 0 < d["roofline"]["frac"] < 1


def test_dump_outputs_group_rows(tmp_path):
    """--dump-outputs: group rows (the Q1/Q9 step result) become one float64
    array per column, row order kept, character keys as code points."""
    import numpy as np
    b = _bench()
    rows = [{"l_returnflag": "A", "l_linestatus": "F", "sum_qty": 1.5,
             "count_order": 600_000_001},
            {"l_returnflag": "N", "l_linestatus": "O", "sum_qty": 2.25,
             "count_order": 7}]
    d = tmp_path / "out"
    b.dump_outputs(str(d), "tpch_q1", rows)
    assert sorted(os.listdir(d)) == ["count_order.npy", "l_linestatus.npy",
                                     "l_returnflag.npy", "sum_qty.npy"]
    for f in os.listdir(d):
        assert np.load(d / f).dtype == np.float64
    assert np.load(d / "count_order.npy").tolist() == [600_000_001, 7]
    assert np.load(d / "l_returnflag.npy").tolist() == [ord("A"), ord("N")]
    assert np.load(d / "sum_qty.npy").tolist() == [1.5, 2.25]


def test_dump_outputs_topk_and_scalar():
    """The Q3 step result (structured top-k rows) dumps field by field; the
    scan_count result is a 1-element array."""
    import numpy as np
    b = _bench()
    dt = np.dtype([("l_orderkey", "i8"), ("revenue", "f8"),
                   ("o_orderdate", "i4"), ("o_shippriority", "i4")])
    top = np.array([(3_000_000_007, 9.5, 2400, 0), (11, 8.25, 2399, 0)],
                   dtype=dt)
    a = b.outputs_as_arrays("tpch_q3", top)
    assert set(a) == set(dt.names)
    assert all(v.dtype == np.float64 and v.shape == (2,) for v in a.values())
    assert a["l_orderkey"].tolist() == [3_000_000_007, 11]
    assert a["revenue"].tolist() == [9.5, 8.25]
    c = b.outputs_as_arrays("scan_count", 123_456_789)
    assert c["count"].dtype == np.float64 and c["count"].tolist() == [123_456_789]


def test_cpu_baseline_sharded():
    """shards>1 = one CLI process per shard (DataNode deployment analog):
    whole-job rows/s over max-shard time, cores = shards, and roughly
    additive throughput vs the 1-core run on an idle host."""
    b = _bench()
    one = b.cpu_baseline("q1", 2_000_000)
    four = b.cpu_baseline("q1", 2_000_000, shards=4)
    assert four["cores"] == 4 and four["kind"] == "port"
    assert "4 shard processes" in four["sample"]
    # parallel shards must beat one core (loose: >=1.5x, CI boxes share)
    assert four["value"] > 1.5 * one["value"]


def test_cpu_baseline_shard_rounding():
    """sample_rows not divisible by shards is rounded down (generator
    requires rows % nranks == 0)."""
    b = _bench()
    cb = b.cpu_baseline("q1", 1_000_001, shards=4)
    assert cb["value"] > 0 and "1000000 " in cb["sample"]

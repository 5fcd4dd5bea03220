"""CPU-side tests of the variance/stddev aggregate's host layers: workspace
sizing (pure host code in libotbx.so), the float8 finalizers, float8_combine
on [N, Sx, Sxx] states and the Coordinator merge over gloo. The oracle
(Youngs-Cramer float8_accum + the C float8_combine) is the yardstick."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd import fragment
from oracle import oracle_py as ora

REL = 1e-6


def close(got, exp, N, Sx):
    """|got - exp| <= 1e-6*|exp| + 1e-26*Sx^2/N: the float8 parity bar plus
    an absolute floor for zero-variance groups, far below the resolution of
    the data ((1e-16*mean)^2 * N)."""
    floor = 1e-26 * Sx * Sx / N if N > 0 else 0.0
    return abs(got - exp) <= REL * abs(exp) + floor


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def _ws(so, fn, n):
    out = C.c_size_t(0)
    assert getattr(so, fn)(C.c_int64(n), C.byref(out)) == 0
    return out.value


def test_var_workspace_sizing(so):
    assert "otbx_agg_i64_var_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert "otbx_agg_i64_var" in _lib.EXPORTED_SYMBOLS
    assert getattr(so, "otbx_agg_i64_var", None) is not None
    prev = 0
    for n in (0, 1, 1000, 10**6, 8 << 20, 10**8):
        b = _ws(so, "otbx_agg_i64_var_workspace_bytes", n)
        assert b >= prev
        assert b >= _ws(so, "otbx_agg_i64_workspace_bytes", n)
        prev = b


def test_finalizers_hand_values():
    # [N=4, Sxx=5.0]: var_pop 5/4, var_samp 5/3
    assert ex.var_pop(4, 5.0) == 1.25
    assert ex.var_samp(4, 5.0) == 5.0 / 3.0
    assert ex.stddev_pop(4, 5.0) == math.sqrt(1.25)
    assert ex.stddev_samp(4, 5.0) == math.sqrt(5.0 / 3.0)


def test_finalizers_null_rules():
    for f in (ex.var_pop, ex.var_samp, ex.stddev_pop, ex.stddev_samp):
        assert f(0, 0.0) is None
    assert ex.var_samp(1, 0.0) is None
    assert ex.stddev_samp(1, 0.0) is None
    assert ex.var_pop(1, 0.0) == 0.0
    assert ex.stddev_pop(1, 0.0) == 0.0
    assert math.isnan(ex.var_pop(3, float("nan")))
    assert math.isnan(ex.stddev_samp(3, float("nan")))


def test_finalizers_against_numpy():
    rng = np.random.default_rng(3)
    x = 50.0 + 7.0 * rng.standard_normal(1000)
    g = ora.agg_i64(np.zeros(1000, dtype=np.int64), x)[0]
    N, Sxx = g.acc[0], g.acc[2]
    assert N == 1000.0
    for ddof, var, std in ((0, ex.var_pop, ex.stddev_pop),
                           (1, ex.var_samp, ex.stddev_samp)):
        v, s = var(N, Sxx), std(N, Sxx)
        assert abs(v - np.var(x, ddof=ddof)) <= 1e-9 * np.var(x, ddof=ddof)
        assert abs(s - np.std(x, ddof=ddof)) <= 1e-9 * np.std(x, ddof=ddof)
        assert s == math.sqrt(v)


def test_combine_bit_identical_to_oracle_float8_combine():
    parts = [ora.q1_partial(ora.gen_tables(40000, rank=r, nranks=2))
             for r in range(2)]
    exp = ora.q1_combine(parts)
    assert len(exp) >= 4
    by_key = [{(g.returnflag, g.linestatus): g for g in p} for p in parts]
    for e in exp:
        k = (e.returnflag, e.linestatus)
        assert k in by_key[0] and k in by_key[1]
        for fld in ("qty_acc", "price_acc", "disc_acc"):
            a = tuple(getattr(by_key[0][k], fld))
            b = tuple(getattr(by_key[1][k], fld))
            got = fragment.combine_var_state(a, b)
            assert got == tuple(getattr(e, fld)), (k, fld)
            # an empty state on either side leaves the other unchanged
            assert fragment.combine_var_state((0.0, 0.0, 0.0), a) == a
            assert fragment.combine_var_state(a, (0.0, 0.0, 0.0)) == a
    z = (0.0, 0.0, 0.0)
    assert fragment.combine_var_state(z, z) == z


def test_split_merge_matches_whole_input():
    rng = np.random.default_rng(11)
    n = 20000
    keys = rng.integers(0, 50, n)
    vals = 1e6 + rng.standard_normal(n)
    bounds = [0, 40, 7000, n]           # 3 uneven shards
    # the first shard must lack some keys
    assert len(np.unique(keys[:40])) < 50
    states = {}
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for g in ora.agg_i64(keys[lo:hi], vals[lo:hi]):
            st = tuple(g.acc)
            states[g.key] = (fragment.combine_var_state(states[g.key], st)
                             if g.key in states else st)
    full = ora.agg_i64(keys, vals)
    assert len(full) == len(states) == 50
    for g in full:
        N, Sx, Sxx = states[g.key]
        assert N == g.acc[0]
        assert abs(Sx - g.acc[1]) <= REL * abs(g.acc[1])
        assert close(Sxx, g.acc[2], N, Sx), (g.key, Sxx, g.acc[2])


# ---- merge_var_partials over gloo, world 2 ----

def _rank_rows(rank):
    """Hand-made otbx_var_group rows: key 1 and 2 overlap, 10/20 are
    disjoint, rank 1 holds a NULL-key row, key 2 has count_v == 0 on rank 0
    and key 3 has count_v == 0 on both."""
    dt = np.dtype(ex.VAR_GROUP_DTYPE)
    if rank == 0:
        rows = [(1, 5, 4, 40.0, 5.0, 0, 0),
                (2, 3, 0, 0.0, 0.0, 0, 1),
                (3, 2, 0, 0.0, 0.0, 0, 1),
                (10, 2, 2, 3.0, 0.5, 0, 0)]
    else:
        rows = [(1, 7, 6, 30.0, 17.5, 0, 0),
                (2, 4, 3, 6.0, 2.0, 0, 0),
                (3, 1, 0, 0.0, 0.0, 0, 1),
                (20, 1, 1, 9.0, 0.0, 0, 0),
                (0, 6, 5, 15.0, 10.0, 1, 0)]
    return list(np.array(rows, dtype=dt))


def _fold_in_process(world=2):
    merged = {}
    for rank in range(world):
        for r in _rank_rows(rank):
            ident = (int(r["key_isnull"]), int(r["key"]))
            st = (float(r["count_v"]), float(r["sum_v"]), float(r["sxx"]))
            if ident in merged:
                merged[ident][0] += int(r["count_star"])
                merged[ident][1] = fragment.combine_var_state(
                    merged[ident][1], st)
            else:
                merged[ident] = [int(r["count_star"]), st]
    return [(ident[1], cs, int(st[0]), st[1], st[2], ident[0],
             int(st[0] == 0)) for ident, (cs, st) in sorted(merged.items())]


def _worker_var(rank, world, port, q):
    from opentenbase_amd import fragment as frag
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    rows = frag.merge_var_partials(_rank_rows(rank))
    if rank == 0:
        q.put([tuple(r.tolist()) for r in rows])
    torch.distributed.destroy_process_group()


def _run(worker, world=2):
    # fresh port per attempt: a lingering TIME_WAIT on a reused MASTER_PORT
    # can fail the rendezvous
    last = None
    for attempt in range(3):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = 31611 + np.random.randint(0, 2000)
        procs = [ctx.Process(target=worker, args=(r, world, port, q))
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
def test_merge_var_partials_two_ranks():
    got = _run(_worker_var)
    exp = _fold_in_process()
    assert got == exp
    # sorted by (key_isnull, key); NULL-key group last
    assert [(g[5], g[0]) for g in got] == [(0, 1), (0, 2), (0, 3), (0, 10),
                                           (0, 20), (1, 0)]
    k1 = got[0]
    assert k1[1] == 12 and k1[2] == 10 and k1[3] == 70.0
    # Sxx1 + Sxx2 + N1*N2*(Sx1/N1 - Sx2/N2)^2/N = 5 + 17.5 + 4*6*25/10
    assert k1[4] == 82.5
    k2, k3 = got[1], got[2]
    assert (k2[1], k2[2], k2[3], k2[4], k2[6]) == (7, 3, 6.0, 2.0, 0)
    assert (k3[1], k3[2], k3[6]) == (3, 0, 1)


def test_merge_var_partials_single_rank_is_identity():
    assert not fragment.is_dist()
    rows = _rank_rows(1)
    assert fragment.merge_var_partials(rows) is rows

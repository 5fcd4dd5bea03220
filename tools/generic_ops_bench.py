#!/usr/bin/env python3
"""Scale benchmark of the generic composable operators (otbx_agg_i64 /
otbx_agg_i64_var / otbx_join_i64) — arbitrary-plan building blocks,
distinct from the fused query pipelines.

  generic_ops_bench.py             agg + join shapes
  generic_ops_bench.py --agg-var   agg and agg_var at the same three shapes
                                   in one process (profiles/agg_var_ops.txt)
  generic_ops_bench.py --sort [--out PATH]
                                   otbx_sort_perm next to otbx_order_groups,
                                   600 M-row sorts and LIMIT (writes
                                   profiles/sort_ops.txt, or PATH)
  generic_ops_bench.py --window [--out PATH]
                                   otbx_window at 600 M rows, timed apart
                                   from its sort, next to a plain-torch
                                   composition of the ranking functions
                                   (writes profiles/window_ops.txt, or PATH)
  generic_ops_bench.py --filter [--out PATH]
                                   otbx_filter_sel at 600 M rows next to
                                   otbx_scan_count and to a plain-torch
                                   composition of the same quals (writes
                                   profiles/filter_ops.txt, or PATH)
  generic_ops_bench.py --project [--out PATH]
                                   otbx_project at 600 M rows next to a
                                   plain-torch composition of the same
                                   expressions (writes
                                   profiles/project_ops.txt, or PATH)
  generic_ops_bench.py --groupagg [--rows N] [--out PATH]
                                   otbx_group_agg at 600 M rows (or N) and
                                   4 / 1 M / 100 M groups, timed apart from
                                   its sort, next to otbx_window, the hash
                                   aggregate and a plain-torch composition
                                   (writes profiles/groupagg_ops.txt, or PATH)
  generic_ops_bench.py --ordagg [--rows N] [--out PATH]
                                   otbx_ordered_agg at 600 M rows (or N) and
                                   4 / 1 M / 100 M groups, timed apart from
                                   its sort, next to the two-call
                                   otbx_group_agg route to count(DISTINCT),
                                   otbx_group_agg set A and plain torch
                                   (writes profiles/ordagg_ops.txt, or PATH)
  generic_ops_bench.py --text [--rows N[,N..]] [--out PATH]
                                   otbx_text_pred (LIKE / compare, staged and
                                   forced-direct) and the text gather on
                                   part-name-, comment- and shipmode-shaped
                                   columns at 20 M and 200 M rows, next to
                                   numpy's np.char.find on one core (writes
                                   profiles/text_ops.txt, or PATH)
  generic_ops_bench.py --textkey [--rows N[,N..]] [--mode-rows N[,N..]]
                       [--out PATH] [--one N | --one-mode N]
                                   otbx_text_rank on part-name-shaped columns
                                   (20 M and 200 M rows, or --rows) and
                                   shipmode-shaped ones (200 M and 600 M, or
                                   --mode-rows), ORDER BY p_name and GROUP BY
                                   l_shipmode end to end, next to numpy's
                                   np.unique on one core (writes
                                   profiles/textkey_ops.txt, or PATH). --one N
                                   / --one-mode N: a single rank of N part
                                   names / ship modes and nothing else, for a
                                   kernel tracer
"""
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opentenbase_amd import executor as ex  # noqa: E402
from opentenbase_amd._lib import (AGG_FUNCS, AggCallsDev,  # noqa: E402
                                  WindowOutDev, call, lib)


def bench_agg(n, ngroups):
    g = torch.Generator(device="cuda").manual_seed(1)
    keys = torch.randint(0, ngroups, (n,), dtype=torch.int64, device="cuda",
                         generator=g)
    vals = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    L = lib()
    ws_bytes = C.c_size_t(0)
    L.otbx_agg_i64_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.time()
        call("otbx_agg_i64", C.c_void_p(keys.data_ptr()), None,
             C.c_void_p(vals.data_ptr()), None, C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream)
        torch.cuda.synchronize()
        best = min(best, time.time() - t0)
    print(f"agg  n={n:>11_} groups={ngroups:>9_}: {best*1e3:8.2f} ms "
          f"({n/best/1e9:6.1f} Grows/s), ngroups={int(ng.cpu().item())}")
    return best


def bench_agg_var(n, ngroups):
    """otbx_agg_i64_var on bench_agg's input (same seed, same keys/values):
    pass 1 is the otbx_agg_i64 call timed above, so time(agg_var) /
    time(agg) prices the index build + second pass + finalize."""
    g = torch.Generator(device="cuda").manual_seed(1)
    keys = torch.randint(0, ngroups, (n,), dtype=torch.int64, device="cuda",
                         generator=g)
    vals = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    L = lib()
    ws_bytes = C.c_size_t(0)
    L.otbx_agg_i64_var_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        call("otbx_agg_i64_var", C.c_void_p(keys.data_ptr()), None,
             C.c_void_p(vals.data_ptr()), None, C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream)
        torch.cuda.synchronize()

    run()  # warm-up (lazy scratch, code-object load)
    best = 1e9
    for _ in range(5):
        t0 = time.time()
        run()
        best = min(best, time.time() - t0)
    print(f"agg_var n={n:>11_} groups={ngroups:>9_}: {best*1e3:8.2f} ms "
          f"({n/best/1e9:6.1f} Grows/s), ngroups={int(ng.cpu().item())}")
    return best


def bench_join(nb, np_):
    g = torch.Generator(device="cuda").manual_seed(2)
    bk = torch.randint(0, nb, (nb,), dtype=torch.int64, device="cuda",
                       generator=g)
    pk = torch.randint(0, nb, (np_,), dtype=torch.int64, device="cuda",
                       generator=g)
    L = lib()
    ws_bytes = C.c_size_t(0)
    L.otbx_join_i64_workspace_bytes(C.c_int64(nb), C.c_int64(np_),
                                    C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    cap = int(np_ * 2.2)
    ob = torch.empty(cap, dtype=torch.int64, device="cuda")
    op = torch.empty(cap, dtype=torch.int64, device="cuda")
    npairs = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.time()
        call("otbx_join_i64", C.c_void_p(bk.data_ptr()), None, C.c_int64(nb),
             C.c_void_p(pk.data_ptr()), None, C.c_int64(np_),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(ob.data_ptr()), C.c_void_p(op.data_ptr()),
             C.c_int64(cap), C.c_void_p(npairs.data_ptr()), stream)
        torch.cuda.synchronize()
        best = min(best, time.time() - t0)
    print(f"join nb={nb:>10_} np={np_:>11_}: {best*1e3:8.2f} ms "
          f"({np_/best/1e9:6.1f} Gprobes/s), pairs={int(npairs.cpu().item())}")


def bench_round2_ops():
    """Generality-tier round-2 operators at scale, timed at the C-ABI
    (device outputs; no host materialization — the executor wrappers
    additionally convert results to Python objects, which dominates at
    100 M-pair scale and is not kernel time). Correctness-first designs;
    numbers are evidence-of-function, not roofline targets."""
    L = lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(3)
    n = 100_000_000
    k1 = torch.randint(0, 100_000, (n,), dtype=torch.int64, device="cuda",
                       generator=g)
    k2 = torch.randint(0, 50, (n,), dtype=torch.int64, device="cuda",
                       generator=g)
    v = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    vi = torch.randint(-10**12, 10**12, (n,), dtype=torch.int64,
                       device="cuda", generator=g)

    def timed(label, fn, units):
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.time() - t0)
        print(f"{label}: {best*1e3:8.2f} ms ({units/best/1e9:6.1f} Grows/s)")

    ws_bytes = C.c_size_t(0)
    L.otbx_agg_i64x2_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    timed("agg2  n=100M groups=5M       ", lambda: call(
        "otbx_agg_i64x2", C.c_void_p(k1.data_ptr()), None,
        C.c_void_p(k2.data_ptr()), None, C.c_void_p(v.data_ptr()), None,
        C.c_int64(n), C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
        C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream), n)

    L.otbx_agg_i64_dec_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    timed("dec   n=100M groups=100k     ", lambda: call(
        "otbx_agg_i64_dec", C.c_void_p(k1.data_ptr()), None,
        C.c_void_p(vi.data_ptr()), None, C.c_int64(n),
        C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
        C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream), n)

    from opentenbase_amd._lib import KeysetDev
    ks = KeysetDev()
    ks.nkeys = 4
    for c, t in enumerate([k1, k2, k2, k2]):
        ks.keys[c] = t.data_ptr()
    L.otbx_agg_i64n_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    timed("aggn4 n=100M groups=5M       ", lambda: call(
        "otbx_agg_i64n", C.byref(ks), C.c_void_p(v.data_ptr()), None,
        C.c_int64(n), C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
        C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream), n)

    nb = 10_000_000
    bk = torch.randint(0, nb, (nb,), dtype=torch.int64, device="cuda",
                       generator=g)
    pk = torch.randint(0, 2 * nb, (n,), dtype=torch.int64, device="cuda",
                       generator=g)
    L.otbx_join_ext_workspace_bytes(C.c_int64(nb), C.c_int64(n),
                                    C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    cap = 2 * n
    ob = torch.empty(cap, dtype=torch.int64, device="cuda")
    op = torch.empty(cap, dtype=torch.int64, device="cuda")
    npairs = torch.zeros(1, dtype=torch.int64, device="cuda")
    for jt, name in [(1, "left"), (2, "semi"), (3, "anti")]:
        timed(f"joinx {name:<5} nb=10M np=100M  ", lambda jt=jt: call(
            "otbx_join_i64_ext", C.c_void_p(bk.data_ptr()), None,
            C.c_int64(nb), C.c_void_p(pk.data_ptr()), None, C.c_int64(n),
            C.c_int32(jt), C.c_void_p(ws.data_ptr()),
            C.c_size_t(ws_bytes.value), C.c_void_p(ob.data_ptr()),
            C.c_void_p(op.data_ptr()), C.c_int64(cap),
            C.c_void_p(npairs.data_ptr()), stream), n)


COPY_CEILING = 6.29e12   # B/s, the measured copy ceiling (README)


def _best_of_5(fn):
    """warm-up, then 5 timed repetitions ending in a device synchronise;
    returns (best, worst) seconds"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        ts.append(time.time() - t0)
    return min(ts), max(ts)


def _varying_bytes(col):
    """radix passes otbx_sort_perm executes for this column: key bytes that
    are not constant over the rows (constant ones are skipped on the
    device). The normalisation maps each byte one-to-one, so the raw bit
    pattern tells (no NaN / -0 in the benchmark data)."""
    width = col.element_size()
    raw = col.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[width])
    n = 0
    for b in range(width):
        byte = (raw >> (8 * b)) & 0xff if width > 1 else raw
        n += int(byte.min().item() != byte.max().item())
    return n


class _SortCall:
    def __init__(self, keys, descending, limit=0):
        self.node = ex.GpuSort(keys, descending=descending, limit=limit)
        self.n, self.limit = len(keys[0]), limit
        L = lib()
        wsb = C.c_size_t(0)
        L.otbx_sort_workspace_bytes(C.c_int64(self.n), C.c_int32(len(keys)),
                                    C.c_int64(limit), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        cap = min(limit, self.n) if limit else self.n
        self.perm = torch.empty(cap, dtype=torch.int64, device="cuda")
        self.nout = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.spec = self.node.spec()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        call("otbx_sort_perm", C.byref(self.spec), C.c_int64(self.n),
             C.c_int64(self.limit), C.c_void_p(self.ws.data_ptr()),
             C.c_size_t(self.wsb), C.c_void_p(self.perm.data_ptr()),
             C.c_void_p(self.nout.data_ptr()), self.stream)


def _check_sorted(key, perm):
    """sorted ascending, and equal keys keep row order (stable)"""
    k = key[perm]
    ok = bool((k[1:] >= k[:-1]).all().item())
    tie = k[1:] == k[:-1]
    return ok and bool((perm[1:][tie] > perm[:-1][tie]).all().item())


def bench_sort(out_path):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --sort — best of 5 wall time after "
        "torch.cuda.synchronize()")
    say("# row-passes/s = n x executed radix passes / time; 24 B per row-pass "
        "(8 B key + 4 B row id, read and written)")
    g = torch.Generator(device="cuda").manual_seed(5)

    # (a) Q3-shaped groups: (revenue DESC, o_orderdate ASC), both operators
    n = 13_900_000
    rev = (torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
           * 5e5 + 1.0)
    date = torch.randint(0, 2400, (n,), dtype=torch.int32, device="cuda",
                         generator=g)
    rec = torch.zeros(n, 3, dtype=torch.int64, device="cuda")
    rec[:, 0] = torch.arange(n, device="cuda")
    rec[:, 1] = rev.view(torch.int64)
    rec[:, 2] = date.to(torch.int64)          # o_shippriority = 0 (high half)
    groups = rec.view(torch.uint8).reshape(-1)
    L = lib()
    wsb = C.c_size_t(0)
    L.otbx_order_groups_workspace_bytes(C.c_int64(n), C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 24, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def old():
        call("otbx_order_groups", C.c_void_p(groups.data_ptr()), C.c_int64(n),
             C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
             C.c_size_t(wsb.value), stream)

    new = _SortCall([rev, date], [True, False])
    ob, ow = _best_of_5(old)
    nb, nw = _best_of_5(new)
    ob2, ow2 = _best_of_5(old)                 # alternate: old, new, old
    ob, ow = min(ob, ob2), max(ow, ow2)
    passes = _varying_bytes(rev) + _varying_bytes(date)
    old_rate, new_rate = n * 10 / ob, n * passes / nb
    old_key = out.view(torch.int64).reshape(n, 3)[:, 0]
    same = bool((old_key == new.perm).all().item())
    say(f"(a) n={n:_} (f64 DESC, i32 ASC), same process")
    say(f"    otbx_order_groups: best {ob*1e3:8.2f} ms  worst {ow*1e3:8.2f} ms"
        f"  10 passes  {old_rate/1e9:6.2f} G row-passes/s "
        f"(spread {(ow-ob)/ob*100:.1f} %)")
    say(f"    otbx_sort_perm   : best {nb*1e3:8.2f} ms  worst {nw*1e3:8.2f} ms"
        f"  {passes} passes executed of 12  {new_rate/1e9:6.2f} G row-passes/s"
        f" (spread {(nw-nb)/nb*100:.1f} %)")
    say(f"    row-passes/s ratio new/old: {new_rate/old_rate:.2f}; "
        f"time ratio old/new: {ob/nb:.2f}; same row order: {same}")
    del rec, groups, ws, out, new, rev, date, old_key
    torch.cuda.empty_cache()

    # (b) 600 M uniform i64, (d) the same with LIMIT; (c) 600 M i32
    n = 600_000_000
    k64 = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda",
                        generator=g)
    full = _SortCall([k64], [False])
    fb, fw = _best_of_5(full)
    p = _varying_bytes(k64)
    say(f"(b) n={n:_} one uniform i64 key: best {fb*1e3:8.2f} ms  worst "
        f"{fw*1e3:8.2f} ms  {p} passes  {n*p/fb/1e9:6.2f} G row-passes/s  "
        f"{n*p*24/fb/1e12:5.2f} TB/s per pass = "
        f"{n*p*24/fb/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy ceiling; "
        f"sorted+stable: {_check_sorted(k64, full.perm)}")
    for limit in (10, 100_000):
        lim = _SortCall([k64], [False], limit)
        lb, lw = _best_of_5(lim)
        agree = bool((lim.perm == full.perm[:limit]).all().item())
        say(f"(d) n={n:_} i64 LIMIT {limit:_}: best {lb*1e3:8.2f} ms  worst "
            f"{lw*1e3:8.2f} ms  ratio to (b): {lb/fb:.3f}; "
            f"equals full-sort prefix: {agree}")
        del lim
    del full, k64
    torch.cuda.empty_cache()
    k32 = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32,
                        device="cuda", generator=g)
    c = _SortCall([k32], [False])
    cb, cw = _best_of_5(c)
    p = _varying_bytes(k32)
    say(f"(c) n={n:_} one uniform i32 key: best {cb*1e3:8.2f} ms  worst "
        f"{cw*1e3:8.2f} ms  {p} passes  {n*p/cb/1e9:6.2f} G row-passes/s  "
        f"{n*p*24/cb/1e12:5.2f} TB/s per pass = "
        f"{n*p*24/cb/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy ceiling; "
        f"sorted+stable: {_check_sorted(k32, c.perm)}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")

_WIN_RANKING = ("row_number", "rank", "dense_rank")
_WIN_ALL = ("row_number", "rank", "dense_rank", "count_star", "count_v",
            "sum_v", "part_rows")


class _WindowCall:
    """otbx_window on an already sorted permutation, buffers allocated once"""

    def __init__(self, srt, npart, vals, funcs):
        self.n, self.npart, self.vals = srt.n, npart, vals
        self.spec, self.perm, self.stream = srt.spec, srt.perm, srt.stream
        wsb = C.c_size_t(0)
        lib().otbx_window_workspace_bytes(C.c_int64(self.n), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.res, self.out = {}, WindowOutDev()
        names = list(funcs) + (["sum_isnull"] if "sum_v" in funcs else [])
        for f in names:
            dt = {"sum_v": torch.float64, "sum_isnull": torch.uint8}.get(
                f, torch.int64)
            self.res[f] = torch.empty(self.n, dtype=dt, device="cuda")
            setattr(self.out, f, self.res[f].data_ptr())

    def __call__(self):
        v = self.vals
        call("otbx_window", C.byref(self.spec), C.c_int32(self.npart),
             C.c_void_p(self.perm.data_ptr()) if self.perm is not None
             else None, C.c_int64(self.n),
             C.c_void_p(v.data_ptr()) if v is not None else None, None,
             C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.wsb),
             C.byref(self.out), self.stream)


def _window_bytes_per_row(key_bytes, funcs):
    """algorithmic bytes of one otbx_window call per row: perm and keys
    gathered once, values gathered once, every requested output written
    once, flag / scan workspace written and read back"""
    b = 8 + key_bytes + 2                      # perm, keys, flag byte w + r
    b += 8 * sum(f != "sum_v" for f in funcs)
    if "sum_v" in funcs or "count_v" in funcs:
        b += 8 + 8                             # running count, frame end: w + r
    if "sum_v" in funcs:
        b += 8 + 4 * 8 + 8 + 1    # vals; value w/r, running sum w/r; sum, null
    return b


def _torch_ranking(pk, ok, perm):
    """what a caller would write without the operator: the ranking functions
    from boundary masks, cummax and cumsum on the same sorted data"""
    n = len(perm)
    sp, so = pk[perm], ok[perm]
    ps = torch.ones(n, dtype=torch.bool, device="cuda")
    ps[1:] = sp[1:] != sp[:-1]
    gs = ps.clone()
    gs[1:] |= so[1:] != so[:-1]
    del sp, so
    pos = torch.arange(n, dtype=torch.int64, device="cuda")
    zero = torch.zeros((), dtype=torch.int64, device="cuda")
    pstart = torch.cummax(torch.where(ps, pos, zero), 0).values
    gstart = torch.cummax(torch.where(gs, pos, zero), 0).values
    cg = torch.cumsum(gs, 0)
    return {"row_number": pos - pstart + 1, "rank": gstart - pstart + 1,
            "dense_rank": cg - cg[pstart] + 1}


def bench_window(out_path):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --window — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), keys staged")
    say("# PARTITION BY an i64 key ORDER BY an i32 key (100 distinct values); "
        "the sort and otbx_window are timed apart")
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 600_000_000
    ok = torch.randint(0, 100, (n,), dtype=torch.int32, device="cuda",
                       generator=g)
    vals = torch.randint(-1000, 1001, (n,), dtype=torch.int64, device="cuda",
                         generator=g).to(torch.float64)
    pk_many = torch.randint(0, 1_000_000, (n,), dtype=torch.int64,
                            device="cuda", generator=g)
    pk_one = torch.zeros(n, dtype=torch.int64, device="cuda")
    cases = [("a", "ranking only, ~1 M partitions", pk_many, None,
              _WIN_RANKING),
             ("b", "all outputs, ~1 M partitions", pk_many, vals, _WIN_ALL),
             ("c", "all outputs, one partition", pk_one, vals, _WIN_ALL)]
    srt, srt_pk = None, None
    for tag, what, pk, v, funcs in cases:
        if srt_pk is not pk:
            del srt
            torch.cuda.empty_cache()
            srt = _SortCall([pk, ok], [False, False])
            sb, sw = _best_of_5(srt)
            srt_pk = pk
        win = _WindowCall(srt, 1, v, funcs)
        wb, ww = _best_of_5(win)
        bpr = _window_bytes_per_row(12, funcs)
        tbs = n * bpr / wb / 1e12
        say(f"({tag}) n={n:_} {what}: sort best {sb*1e3:8.2f} ms  worst "
            f"{sw*1e3:8.2f} ms | otbx_window best {wb*1e3:8.2f} ms  worst "
            f"{ww*1e3:8.2f} ms (spread {(ww-wb)/wb*100:.1f} %)  {bpr} B/row "
            f"algorithmic = {n*bpr/1e9:.1f} GB  {tbs:5.2f} TB/s = "
            f"{tbs*1e12/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy ceiling")
        if tag == "a":
            tb, tw = _best_of_5(lambda: _torch_ranking(pk, ok, srt.perm))
            ref = _torch_ranking(pk, ok, srt.perm)
            same = all(bool(torch.equal(ref[f], win.res[f])) for f in ref)
            parts = int((win.res["row_number"] == 1).sum().item())
            say(f"    plain torch (mask, cummax, cumsum) on the same sorted "
                f"data: best {tb*1e3:8.2f} ms  worst {tw*1e3:8.2f} ms; "
                f"torch / otbx_window time ratio: {tb/wb:.2f}; same values: "
                f"{same}; partitions: {parts:_}")
            del ref, win
            # the same call on pre-gathered keys with perm = NULL: what is
            # left when the loads through perm are sequential instead
            class _Sorted:
                pass
            pre = _Sorted()
            pre.keys = [pk[srt.perm], ok[srt.perm]]
            pre.n, pre.perm, pre.stream = n, None, srt.stream
            pre.spec = ex.GpuSort(pre.keys).spec()
            win = _WindowCall(pre, 1, None, funcs)
            ib, iw = _best_of_5(win)
            ibpr = bpr - 8
            say(f"    same call, keys pre-gathered, perm = NULL: best "
                f"{ib*1e3:8.2f} ms  worst {iw*1e3:8.2f} ms  {ibpr} B/row = "
                f"{n*ibpr/ib/1e12:5.2f} TB/s = "
                f"{n*ibpr/ib/COPY_CEILING*100:4.1f} % of the ceiling; the "
                f"gather through perm costs {(wb-ib)*1e3:.2f} ms of (a)")
            del pre
        else:
            tot = float(v.sum().item()) if tag == "c" else None
            last = float(win.res["sum_v"][-1].item())
            say(f"    count_v[-1]={int(win.res['count_v'][-1].item()):_} "
                f"part_rows[-1]={int(win.res['part_rows'][-1].item()):_} "
                f"sum_v[-1]={last}" +
                (f" (column total {tot})" if tot is not None else ""))
        del win
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _GroupAggCall:
    """otbx_group_agg on an already sorted permutation, buffers allocated
    once. aggs: [(func, col or None)] without masks."""

    def __init__(self, srt, aggs):
        self.n = srt.n
        self.spec, self.perm, self.stream = srt.spec, srt.perm, srt.stream
        wsb = C.c_size_t(0)
        lib().otbx_group_agg_workspace_bytes(C.c_int64(self.n), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.calls = AggCallsDev()
        self.calls.naggs = len(aggs)
        self.outs = []
        self.row_bytes, self.group_bytes = 0, 8          # first_row
        for i, (func, col) in enumerate(aggs):
            ac = self.calls.agg[i]
            ac.func = AGG_FUNCS[func]
            ac.type = ex._SORT_TYPE[col.dtype] if col is not None else 0
            ac.col = col.data_ptr() if col is not None else None
            wide = func == "sum" and col.dtype == torch.int64
            dt = torch.int64 if func in ("count_star", "count") or wide \
                else col.dtype
            o = [torch.empty(self.n, dtype=dt, device="cuda")]
            ac.out = o[0].data_ptr()
            if wide:
                o.append(torch.empty(self.n, dtype=torch.int64, device="cuda"))
                ac.out_hi = o[1].data_ptr()
            if func not in ("count_star", "count"):
                o.append(torch.empty(self.n, dtype=torch.uint8, device="cuda"))
                ac.out_null = o[-1].data_ptr()
            self.outs.append(o)
            # per aggregate and row: flag byte, perm, the value
            self.row_bytes += 1 + 8 + (col.element_size()
                                       if func not in ("count_star", "count")
                                       else 0)
            self.group_bytes += sum(t.element_size() for t in o)
        self.first = torch.empty(self.n, dtype=torch.int64, device="cuda")
        self.ng = torch.zeros(1, dtype=torch.int64, device="cuda")

    def __call__(self):
        call("otbx_group_agg", C.byref(self.spec),
             C.c_void_p(self.perm.data_ptr()) if self.perm is not None
             else None, C.c_int64(self.n), C.byref(self.calls),
             C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.wsb),
             C.c_void_p(self.first.data_ptr()),
             C.c_void_p(self.ng.data_ptr()), self.stream)

    def algorithmic_bytes(self, key_bytes, ngroups):
        """the boundary pass reads perm and gathers the keys
        once and writes one flag byte; first_row reads the flags; every
        aggregate reads flags and perm and gathers its value once; per group
        first_row and each output are written once"""
        per_row = 8 + key_bytes + 1 + 1 + self.row_bytes
        return self.n * per_row + ngroups * self.group_bytes


def _torch_group_sum(key, vals, perm):
    """what a caller would write without the operator: gather,
    unique_consecutive, segment_reduce"""
    sk, sv = key[perm], vals[perm]
    uk, counts = torch.unique_consecutive(sk, return_counts=True)
    sums = torch.segment_reduce(sv, "sum", lengths=counts)
    return uk, counts, sums


def _exact_group_sum(key, v64, perm):
    """counts and sums per key run from an int64 prefix sum: exact, and
    independent of both the operator and torch.segment_reduce"""
    n = len(perm)
    sk = key[perm]
    st = torch.ones(n, dtype=torch.bool, device="cuda")
    st[1:] = sk[1:] != sk[:-1]
    del sk
    starts = st.nonzero().flatten()
    del st
    ends = torch.cat([starts[1:], torch.tensor([n], device="cuda")])
    tot = torch.cumsum(v64[perm], 0)[ends - 1]
    sums = tot.clone()
    sums[1:] -= tot[:-1]
    return ends - starts, sums.to(torch.float64)


def bench_groupagg(out_path, n=600_000_000):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --groupagg — best / worst of 5 wall "
        "time after torch.cuda.synchronize(), columns staged")
    say("# GROUP BY one i64 key; the sort and otbx_group_agg are timed apart; "
        "set A = {count_star, sum f64}, set B = {count_star, sum f64, "
        "min f64, max f64, sum i64}")
    g = torch.Generator(device="cuda").manual_seed(11)
    v64 = torch.randint(-1000, 1001, (n,), dtype=torch.int64, device="cuda",
                        generator=g)
    vals = v64.to(torch.float64)
    ivals = torch.randint(-2**40, 2**40, (n,), dtype=torch.int64,
                          device="cuda", generator=g)
    set_a = [("count_star", None), ("sum", vals)]
    set_b = set_a + [("min", vals), ("max", vals), ("sum", ivals)]
    for groups in (4, 1_000_000, 100_000_000):
        key = torch.randint(0, groups, (n,), dtype=torch.int64, device="cuda",
                            generator=g)
        srt = _SortCall([key], [False])
        sb, sw = _best_of_5(srt)
        say(f"groups={groups:_} n={n:_}: sort best {sb*1e3:8.2f} ms  worst "
            f"{sw*1e3:8.2f} ms")
        res = {}
        for tag, aggs in (("A", set_a), ("B", set_b)):
            ga = _GroupAggCall(srt, aggs)
            gb, gw = _best_of_5(ga)
            ng = int(ga.ng.cpu().item())
            nbytes = ga.algorithmic_bytes(8, ng)
            tbs = nbytes / gb / 1e12
            say(f"  set {tag}: otbx_group_agg best {gb*1e3:8.2f} ms  worst "
                f"{gw*1e3:8.2f} ms (spread {(gw-gb)/gb*100:.1f} %)  ngroups="
                f"{ng:_}  {nbytes/1e9:.1f} GB algorithmic  {tbs:5.2f} TB/s = "
                f"{tbs*1e12/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy "
                f"ceiling")
            res[tag] = (gb, ga.outs[0][0][:ng].clone(),
                        ga.outs[1][0][:ng].clone())
            del ga
            torch.cuda.empty_cache()
        ga_best, ga_cnt, ga_sum = res["A"]
        xc, xs = _exact_group_sum(key, v64, srt.perm)
        say(f"  set A equals the exact int64 prefix-sum reference: counts "
            f"{bool(torch.equal(xc, ga_cnt))}, sums "
            f"{bool(torch.equal(xs, ga_sum))}")
        # (a) otbx_window asked for the same numbers at every row
        win = _WindowCall(srt, 1, vals, ("count_star", "sum_v"))
        wb, ww = _best_of_5(win)
        say(f"  (a) otbx_window count_star + sum_v, npart == nkeys: best "
            f"{wb*1e3:8.2f} ms  worst {ww*1e3:8.2f} ms; window / group_agg "
            f"(set A) time ratio: {wb/ga_best:.2f}")
        del win
        torch.cuda.empty_cache()
        # (b) the hash path end to end against sort + group_agg
        hb = bench_agg_on(key, vals)
        say(f"  (b) otbx_agg_i64 (hash) best {hb*1e3:8.2f} ms; sort + "
            f"group_agg (set A) {(sb+ga_best)*1e3:8.2f} ms; ratio sorted / "
            f"hash: {(sb+ga_best)/hb:.2f}")
        torch.cuda.empty_cache()
        # (c) plain torch on the same sorted permutation
        try:
            tb, tw = _best_of_5(lambda: _torch_group_sum(key, vals, srt.perm))
            uk, counts, sums = _torch_group_sum(key, vals, srt.perm)
            say(f"  (c) plain torch (gather, unique_consecutive, "
                f"segment_reduce): best {tb*1e3:8.2f} ms  worst "
                f"{tw*1e3:8.2f} ms; torch / group_agg (set A) time ratio: "
                f"{tb/ga_best:.2f}; torch equals the exact reference: counts "
                f"{bool(torch.equal(counts, xc))}, sums "
                f"{bool(torch.equal(sums, xs))} ("
                f"{int((sums != xs).sum().item()):_} sums differ)")
            del uk, counts, sums
        except RuntimeError as e:
            say(f"  (c) plain torch composition failed: {str(e)[:120]}")
        # the same call on pre-gathered columns with perm = NULL: what is
        # left when the loads through perm are sequential instead
        class _Sorted:
            pass
        pre = _Sorted()
        pre.keys = [key[srt.perm]]
        pv = vals[srt.perm]
        pre.n, pre.perm, pre.stream = n, None, srt.stream
        pre.spec = ex.GpuSort(pre.keys).spec()
        ga = _GroupAggCall(pre, [("count_star", None), ("sum", pv)])
        ib, iw = _best_of_5(ga)
        say(f"  (d) set A, columns pre-gathered, perm = NULL: best "
            f"{ib*1e3:8.2f} ms  worst {iw*1e3:8.2f} ms; the gathers through "
            f"perm cost {(ga_best-ib)*1e3:.2f} ms of set A")
        del ga, pre, pv, srt, key, res, ga_cnt, ga_sum, xc, xs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _OrdAggCall:
    """otbx_ordered_agg on a permutation sorted on (key, x), buffers
    allocated once. calls: [(func,) | (func, fraction)]"""

    def __init__(self, srt, ngroup, arg, calls):
        from opentenbase_amd._lib import OAGG_FUNCS, OAggCallsDev
        self.n, self.ngroup = srt.n, ngroup
        self.spec, self.perm, self.stream = srt.spec, srt.perm, srt.stream
        wsb = C.c_size_t(0)
        lib().otbx_ordered_agg_workspace_bytes(
            C.c_int64(self.n), C.c_int32(len(calls)), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.calls = OAggCallsDev()
        self.calls.ncalls = len(calls)
        self.outs = []
        self.group_bytes = 8                              # first_row
        funcs = [c[0] for c in calls]
        for i, c in enumerate(calls):
            oc = self.calls.call[i]
            oc.func = OAGG_FUNCS[c[0]]
            oc.fraction = c[1] if len(c) > 1 else 0.0
            wide = c[0] == "sum_distinct" and arg.dtype == torch.int64
            dt = torch.int64 if c[0] == "count_distinct" or wide else (
                torch.float64 if c[0] == "percentile_cont" else arg.dtype)
            o = [torch.empty(self.n, dtype=dt, device="cuda")]
            oc.out = o[0].data_ptr()
            if wide:
                o.append(torch.empty(self.n, dtype=torch.int64, device="cuda"))
                oc.out_hi = o[1].data_ptr()
            if c[0] != "count_distinct":
                o.append(torch.empty(self.n, dtype=torch.uint8, device="cuda"))
                oc.out_null = o[-1].data_ptr()
            self.outs.append(o)
            self.group_bytes += sum(t.element_size() for t in o)
            # the per-group value reads: perm entry + value
            reads = {"percentile_disc": 1, "percentile_cont": 2,
                     "mode": 1}.get(c[0], 0)
            self.group_bytes += reads * (8 + arg.element_size())
        # flag passes: one per kind of aggregate present
        self.flag_passes = sum((
            any(f in ("count_distinct", "percentile_disc", "percentile_cont")
                for f in funcs), "mode" in funcs, "sum_distinct" in funcs))
        self.sum_distinct = "sum_distinct" in funcs
        self.arg_bytes = arg.element_size()
        self.first = torch.empty(self.n, dtype=torch.int64, device="cuda")
        self.ng = torch.zeros(1, dtype=torch.int64, device="cuda")

    def __call__(self):
        call("otbx_ordered_agg", C.byref(self.spec), C.c_int32(self.ngroup),
             C.c_void_p(self.perm.data_ptr()), C.c_int64(self.n),
             C.byref(self.calls), C.c_void_p(self.ws.data_ptr()),
             C.c_size_t(self.wsb), C.c_void_p(self.first.data_ptr()),
             C.c_void_p(self.ng.data_ptr()), self.stream)

    def algorithmic_bytes(self, key_bytes, ngroups, nruns):
        """the boundary pass reads perm, gathers the keys and
        the argument once and writes one flag byte; first_row reads the
        flags; every kind of aggregate reads the flags once; sum_distinct
        reads perm and the value once per RUN; per group first_row, the
        outputs and the percentile / mode gathers"""
        per_row = 8 + key_bytes + self.arg_bytes + 1 + 1 + self.flag_passes
        per_run = (8 + self.arg_bytes) if self.sum_distinct else 0
        return self.n * per_row + nruns * per_run + ngroups * self.group_bytes


def _torch_count_distinct(key, x, perm):
    """what a caller would write without the operator: gather both columns,
    mark where the pair changes, and count the marks per key run (a cumsum
    read at the run ends). torch.unique_consecutive has no pair form short
    of stacking the columns, and torch.quantile no grouped form: the
    percentiles and the mode have no plain-torch comparator here."""
    sk, sx = key[perm], x[perm]
    n = len(perm)
    newk = torch.ones(n, dtype=torch.bool, device="cuda")
    newk[1:] = sk[1:] != sk[:-1]
    newp = newk.clone()
    newp[1:] |= sx[1:] != sx[:-1]
    del sk, sx
    starts = newk.nonzero().flatten()
    ends = torch.cat([starts[1:], torch.tensor([n], device="cuda")])
    tot = torch.cumsum(newp, 0)[ends - 1]
    cnt = tot.clone()
    cnt[1:] -= tot[:-1]
    return cnt


def bench_ordagg(out_path, n=600_000_000):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --ordagg — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), columns staged")
    say("# GROUP BY one i64 key, argument x = f64 with 1000 integer values; "
        "the sort on (key, x) and otbx_ordered_agg are timed apart; set C = "
        "{count_distinct}, set S = {count_distinct, sum_distinct}, set P = "
        "{percentile_disc 0.5, percentile_cont 0.5, mode}")
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randint(0, 1000, (n,), dtype=torch.int64, device="cuda",
                      generator=g).to(torch.float64)
    sets = (("C", [("count_distinct",)]),
            ("S", [("count_distinct",), ("sum_distinct",)]),
            ("P", [("percentile_disc", 0.5), ("percentile_cont", 0.5),
                   ("mode",)]))

    class _On:
        pass
    for groups in (4, 1_000_000, 100_000_000):
        key = torch.randint(0, groups, (n,), dtype=torch.int64, device="cuda",
                            generator=g)
        srt = _SortCall([key, x], [False, False])
        sb, sw = _best_of_5(srt)
        say(f"groups={groups:_} n={n:_}: sort on (key, x) best {sb*1e3:8.2f} "
            f"ms  worst {sw*1e3:8.2f} ms")
        best = {}
        cd = None
        for tag, calls in sets:
            oa = _OrdAggCall(srt, 1, x, calls)
            ob, ow = _best_of_5(oa)
            ng = int(oa.ng.cpu().item())
            if cd is None:
                cd = oa.outs[0][0][:ng].clone()
                nruns = int(cd.sum().item())
            nbytes = oa.algorithmic_bytes(8, ng, nruns)
            tbs = nbytes / ob / 1e12
            say(f"  set {tag}: otbx_ordered_agg best {ob*1e3:8.2f} ms  worst "
                f"{ow*1e3:8.2f} ms (spread {(ow-ob)/ob*100:.1f} %)  ngroups="
                f"{ng:_} runs={nruns:_}  {nbytes/1e9:.1f} GB algorithmic  "
                f"{tbs:5.2f} TB/s = {tbs*1e12/COPY_CEILING*100:4.1f} % of the "
                f"6.29 TB/s copy ceiling")
            best[tag] = ob
            del oa
            torch.cuda.empty_cache()
        # (a) the only route before this operator: DISTINCT on (key, x) with
        # otbx_group_agg, gather the keys, count per key — same sort
        pairs = _GroupAggCall(srt, [])
        one = _On()
        one.n, one.stream = n, srt.stream

        def two_step():
            pairs()
            npairs = int(pairs.ng.cpu().item())
            pk = ex.gather(key, pairs.first[:npairs])
            one.n, one.perm = npairs, None
            one.spec = ex.GpuSort([pk]).spec()
            cnt = _GroupAggCall(one, [("count_star", None)])
            cnt()
            return cnt
        ab, aw = _best_of_5(two_step)
        cnt = two_step()
        torch.cuda.synchronize()
        ng2 = int(cnt.ng.cpu().item())
        same = ng2 == len(cd) and bool(torch.equal(cnt.outs[0][0][:ng2], cd))
        say(f"  (a) two otbx_group_agg calls (DISTINCT on (key, x), gather, "
            f"count per key; buffers allocated inside): best {ab*1e3:8.2f} ms "
            f" worst {aw*1e3:8.2f} ms; two-step / ordered_agg (set C) time "
            f"ratio: {ab/best['C']:.2f}; same counts: {same}")
        del pairs, cnt
        torch.cuda.empty_cache()
        # (b) one boundary pass + one aggregate that gathers a value column
        one.n, one.perm = n, srt.perm
        one.spec = ex.GpuSort([key]).spec()
        ga = _GroupAggCall(one, [("count_star", None), ("sum", x)])
        gb, gw = _best_of_5(ga)
        say(f"  (b) otbx_group_agg set A {{count_star, sum f64}} on the same "
            f"permutation: best {gb*1e3:8.2f} ms  worst {gw*1e3:8.2f} ms; "
            f"ordered_agg / group_agg (set A) time ratio: C "
            f"{best['C']/gb:.2f}, S {best['S']/gb:.2f}, P {best['P']/gb:.2f}")
        del ga
        torch.cuda.empty_cache()
        # (c) plain torch, count_distinct only
        try:
            tb, tw = _best_of_5(lambda: _torch_count_distinct(key, x,
                                                              srt.perm))
            tc = _torch_count_distinct(key, x, srt.perm)
            say(f"  (c) plain torch count(DISTINCT) (gather, pair-change "
                f"marks, cumsum at the run ends): best {tb*1e3:8.2f} ms  "
                f"worst {tw*1e3:8.2f} ms; torch / ordered_agg (set C) time "
                f"ratio: {tb/best['C']:.2f}; same counts: "
                f"{bool(torch.equal(tc, cd))}")
            del tc
        except RuntimeError as e:
            say(f"  (c) plain torch composition failed: {str(e)[:120]}")
        del srt, key, cd
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _FrameCall:
    """otbx_window_frame on an already sorted permutation (or perm = NULL),
    buffers allocated once. calls: (func, col, param) with col a device
    tensor or None"""

    def __init__(self, srt, npart, frame, calls):
        from opentenbase_amd._lib import WIN_FUNCS, WinCallDev
        self.n, self.npart, self.frame = srt.n, npart, frame
        self.spec, self.perm, self.stream = srt.spec, srt.perm, srt.stream
        wsb = C.c_size_t(0)
        lib().otbx_window_frame_workspace_bytes(
            C.c_int64(self.n), C.c_int32(len(calls)), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.calls = (WinCallDev * 8)()
        self.ncalls = len(calls)
        self.outs, self.keep = [], []
        types = {torch.int64: 0, torch.float64: 1, torch.int32: 2,
                 torch.uint8: 3}
        for i, (func, col, param) in enumerate(calls):
            wc = self.calls[i]
            wc.func, wc.param, wc.def_isnull = WIN_FUNCS[func], param, 1
            if col is not None:
                wc.col, wc.type = col.data_ptr(), types[col.dtype]
                self.keep.append(col)
            dt = torch.int32 if func == "ntile" else (
                torch.int64 if func in ("count", "count_star") or
                col.dtype != torch.float64 else torch.float64)
            o = [torch.empty(self.n, dtype=dt, device="cuda")]
            wc.out = o[0].data_ptr()
            if func not in ("ntile", "count", "count_star"):
                o.append(torch.empty(self.n, dtype=torch.uint8, device="cuda"))
                wc.out_null = o[-1].data_ptr()
                if func == "sum" and col.dtype == torch.int64:
                    o.append(torch.empty(self.n, dtype=torch.int64,
                                         device="cuda"))
                    wc.out_hi = o[-1].data_ptr()
            self.outs.append(o)

    def __call__(self):
        call("otbx_window_frame", C.byref(self.spec), C.c_int32(self.npart),
             C.c_void_p(self.perm.data_ptr()) if self.perm is not None
             else None, C.c_int64(self.n), C.byref(self.frame), self.calls,
             C.c_int32(self.ncalls), C.c_void_p(self.ws.data_ptr()),
             C.c_size_t(self.wsb), self.stream)


# algorithmic bytes per row of the kernels of one otbx_window_frame call
# (DESIGN.md §8n): the bounds pass gathers perm and key and writes / reads
# the flag byte and two int64 bound arrays; a position function reads the two
# bounds, gathers perm + value and writes value + null byte; an aggregate
# gathers perm + value into 9 staged bytes, then either loops over them
# (direct: staged bytes read once from memory, the rest from cache) or runs
# one scan (staged bytes read twice, 12 state bytes written) per direction
# and reads the bounds and one or two states back
_WF_BOUNDS = 8 + 8 + 2 + 2 * 8
_WF_POS = 2 * 8 + 8 + 8 + 8 + 1
_WF_NTILE = 2 * 8 + 4
_WF_GATHER = 8 + 8 + 9
_WF_DIRECT = 2 * 8 + 9 + 8 + 1
_WF_SCAN = 2 * 9 + 2 + 12
_WF_FINAL1 = 2 * 8 + 12 + 8 + 1
_WF_FINAL2 = 2 * 8 + 2 * 12 + 8 + 1


def bench_winframe(out_path, n=600_000_000, ab_n=200_000_000):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def rate(nbytes, t):
        tbs = nbytes / t / 1e12
        return (f"{nbytes/1e9:.1f} GB algorithmic  {tbs:5.2f} TB/s = "
                f"{tbs*1e12/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy "
                f"ceiling")

    say("# tools/generic_ops_bench.py --winframe — best / worst of 5 wall "
        "time after torch.cuda.synchronize(), columns staged")
    say("# OVER (PARTITION BY one i64 key), f64 values; the sort and "
        "otbx_window_frame are timed apart")
    dflt = ex.window_frame_direct_default()
    g = torch.Generator(device="cuda").manual_seed(13)

    # ---- the direct cut-over: per-row loop against the two scans ----
    say(f"# cut-over A/B at n={ab_n:_}, 1_000_000 partitions, sum f64 over "
        f"ROWS (W-1) PRECEDING .. CURRENT ROW, perm given; "
        f"OTBX_WIN_FRAME_DIRECT=4097 (loop) against =0 (scans)")
    key = torch.randint(0, 1_000_000, (ab_n,), dtype=torch.int64,
                        device="cuda", generator=g)
    vals = torch.randint(-1000, 1001, (ab_n,), dtype=torch.int64,
                         device="cuda", generator=g).to(torch.float64)
    srt = _SortCall([key], [False])
    srt()
    torch.cuda.synchronize()
    for w in (2, 4, 8, 16, 32, 64, 128, 256):
        fc = _FrameCall(srt, 1, ex.rows_between(-(w - 1), 0),
                        [("sum", vals, 0)])
        os.environ["OTBX_WIN_FRAME_DIRECT"] = "4097"
        lb, lw = _best_of_5(fc)
        loop_out = fc.outs[0][0].clone()
        os.environ["OTBX_WIN_FRAME_DIRECT"] = "0"
        sb, sw = _best_of_5(fc)
        same = bool(torch.equal(loop_out, fc.outs[0][0]))
        del os.environ["OTBX_WIN_FRAME_DIRECT"]
        say(f"  W={w:4d}: loop best {lb*1e3:7.2f} ms worst {lw*1e3:7.2f} ms; "
            f"scans best {sb*1e3:7.2f} ms worst {sw*1e3:7.2f} ms; loop / "
            f"scans {lb/sb:.2f}; equal results (integer-valued): {same}")
        del fc, loop_out
        torch.cuda.empty_cache()
    say(f"# compiled default cut-over: {dflt}")
    del key, vals, srt
    torch.cuda.empty_cache()

    # ---- the operator at scale ----
    v64 = torch.randint(-1000, 1001, (n,), dtype=torch.int64, device="cuda",
                        generator=g)
    vals = v64.to(torch.float64)
    del v64
    cases = (
        ("lag(1)", ex.rows_between(None, 0), [("lag", vals, 1)],
         _WF_BOUNDS + _WF_POS),
        ("ntile(4)", ex.rows_between(None, 0), [("ntile", None, 4)],
         _WF_BOUNDS + _WF_NTILE),
        ("ROWS -6..0 sum + count", ex.rows_between(-6, 0),
         [("sum", vals, 0), ("count", vals, 0)],
         _WF_BOUNDS + _WF_GATHER + _WF_DIRECT + 2 * 8 + 8),
        ("ROWS unbounded..current sum", ex.rows_between(None, 0),
         [("sum", vals, 0)],
         _WF_BOUNDS + _WF_GATHER + _WF_SCAN + _WF_FINAL1),
        ("ROWS -1000..+1000 max", ex.rows_between(-1000, 1000),
         [("max", vals, 0)],
         _WF_BOUNDS + _WF_GATHER + 2 * _WF_SCAN + _WF_FINAL2),
    )
    for parts in (4, 1_000_000, 100_000_000):
        key = torch.randint(0, parts, (n,), dtype=torch.int64, device="cuda",
                            generator=g)
        srt = _SortCall([key], [False])
        sb, sw = _best_of_5(srt)
        say(f"partitions={parts:_} n={n:_}: sort best {sb*1e3:8.2f} ms  worst "
            f"{sw*1e3:8.2f} ms")
        win = _WindowCall(srt, 1, vals, ("sum_v",))
        wb, ww = _best_of_5(win)
        say(f"  otbx_window default-frame sum_v: best {wb*1e3:8.2f} ms  worst "
            f"{ww*1e3:8.2f} ms")
        win_sum = win.res["sum_v"].clone()
        del win
        torch.cuda.empty_cache()
        for name, frame, calls, bpr in cases:
            fc = _FrameCall(srt, 1, frame, calls)
            fb, fw = _best_of_5(fc)
            say(f"  {name}: otbx_window_frame best {fb*1e3:8.2f} ms  worst "
                f"{fw*1e3:8.2f} ms (spread {(fw-fb)/fb*100:.1f} %); with the "
                f"sort {(sb+fb)*1e3:8.2f} ms; frame / otbx_window sum_v "
                f"{fb/wb:.2f}; {rate(bpr * n, fb)}")
            if name == "ROWS unbounded..current sum":
                # with no order key the default frame is the whole partition:
                # its sum is this running sum at the partition's last row
                say(f"    integer-valued check against otbx_window: last row "
                    f"of the input equal: "
                    f"{bool(fc.outs[0][0][-1] == win_sum[-1])}")
            if name == "lag(1)":
                def torch_lag():
                    sk, sv = key[srt.perm], vals[srt.perm]
                    out = torch.roll(sv, 1)
                    first = torch.ones(n, dtype=torch.bool, device="cuda")
                    first[1:] = sk[1:] != sk[:-1]
                    return out, first
                try:
                    tb, tw = _best_of_5(torch_lag)
                    out, first = torch_lag()
                    ok = bool(torch.equal(first, fc.outs[0][1] != 0)) and \
                        bool(torch.equal(out[~first], fc.outs[0][0][~first]))
                    say(f"    plain torch (two gathers, roll, boundary mask): "
                        f"best {tb*1e3:8.2f} ms  worst {tw*1e3:8.2f} ms; torch "
                        f"/ frame time ratio {tb/fb:.2f}; equal: {ok}")
                    del out, first
                except RuntimeError as e:
                    say(f"    plain torch composition failed: {str(e)[:120]}")
            if name == "ROWS unbounded..current sum":
                def torch_running():
                    sk, sv = key[srt.perm], vals[srt.perm]
                    cs = torch.cumsum(sv, 0)
                    first = torch.ones(n, dtype=torch.bool, device="cuda")
                    first[1:] = sk[1:] != sk[:-1]
                    idx = torch.arange(n, device="cuda")
                    start = torch.cummax(torch.where(first, idx, 0), 0)[0]
                    return cs - (cs[start] - sv[start])
                try:
                    tb, tw = _best_of_5(torch_running)
                    ok = bool(torch.equal(torch_running(), fc.outs[0][0]))
                    say(f"    plain torch (gathers, cumsum, cummax, prefix "
                        f"difference): best {tb*1e3:8.2f} ms  worst "
                        f"{tw*1e3:8.2f} ms; torch / frame time ratio "
                        f"{tb/fb:.2f}; equal (integer-valued): {ok}")
                except RuntimeError as e:
                    say(f"    plain torch composition failed: {str(e)[:120]}")
            del fc
            torch.cuda.empty_cache()
        del srt, key, win_sum
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def bench_agg_on(keys, vals):
    """otbx_agg_i64 on given columns, best of 5 after a warm-up (seconds)"""
    n = len(keys)
    ws_bytes = C.c_size_t(0)
    lib().otbx_agg_i64_workspace_bytes(C.c_int64(n), C.byref(ws_bytes))
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * 40, dtype=torch.uint8, device="cuda")
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        call("otbx_agg_i64", C.c_void_p(keys.data_ptr()), None,
             C.c_void_p(vals.data_ptr()), None, C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), stream)
    return _best_of_5(run)[0]


class _FilterCall:
    """otbx_filter_sel with everything preallocated; clauses as GpuFilter
    takes them"""

    def __init__(self, clauses, count_only=False):
        self.node = ex.GpuFilter(clauses, count_only=count_only)
        self.n = self.node.n
        wsb = C.c_size_t(0)
        lib().otbx_filter_workspace_bytes(C.c_int64(self.n), C.byref(wsb))
        self.wsb = wsb.value
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.sel = None if count_only else \
            torch.empty(self.n, dtype=torch.int64, device="cuda")
        self.nsel = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.qual = self.node.qual()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # bytes of the columns and masks the qual references, each once
        seen = {}
        for c in clauses:
            for t in c:
                for x in (t.col, t.nulls, t.rnulls,
                          t.rhs if isinstance(t.rhs, torch.Tensor) else None):
                    if x is not None:
                        seen[x.data_ptr()] = x.element_size()
        self.col_bytes = sum(seen.values())

    def __call__(self):
        call("otbx_filter_sel", C.byref(self.qual), C.c_int64(self.n),
             C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.wsb),
             C.c_void_p(self.sel.data_ptr()) if self.sel is not None else None,
             C.c_void_p(self.nsel.data_ptr()), self.stream)

    def count(self):
        return int(self.nsel.item())

    def bytes_per_row(self):
        """referenced columns; when the selection is written also the
        bitmask (written and read back) and 8 B per selected row"""
        if self.sel is None:
            return self.col_bytes
        return self.col_bytes + 2 / 8 + 8 * self.count() / self.n


def bench_filter(out_path):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --filter — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), columns staged, workspace and "
        "selection preallocated")
    say("# algorithmic B/row = referenced columns and masks [+ 2/8 (bitmask "
        "written and read back) + 8 x selectivity when the selection is "
        "written]")
    g = torch.Generator(device="cuda").manual_seed(13)
    n = 600_000_000
    date = torch.randint(0, 2500, (n,), dtype=torch.int32, device="cuda",
                         generator=g)
    price = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    pnull = (torch.rand(n, device="cuda", generator=g) < 0.05).to(torch.uint8)
    flag = torch.randint(0, 25, (n,), dtype=torch.uint8, device="cuda",
                         generator=g)
    rare = torch.randint(0, 10_000, (n,), dtype=torch.int32, device="cuda",
                         generator=g)
    T = ex.qual_term

    def report(tag, what, fc, torch_fn, extra=""):
        fb, fw = _best_of_5(fc)
        cnt = fc.count()
        bpr = fc.bytes_per_row()
        tbs = n * bpr / fb / 1e12
        say(f"({tag}) n={n:_} {what}: otbx_filter_sel best {fb*1e3:8.3f} ms  "
            f"worst {fw*1e3:8.3f} ms (spread {(fw-fb)/fb*100:.1f} %)  "
            f"selected {cnt:_} ({cnt/n*100:.4f} %)  {bpr:.2f} B/row "
            f"algorithmic = {n*bpr/1e9:.2f} GB  {tbs:5.2f} TB/s = "
            f"{tbs*1e12/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy "
            f"ceiling{extra}")
        tb, tw = _best_of_5(torch_fn)
        ref = torch_fn()
        if fc.sel is None:
            same = int(ref.item()) == cnt
        else:
            same = len(ref) == cnt and bool(torch.equal(ref, fc.sel[:cnt]))
        say(f"    plain torch on the same columns: best {tb*1e3:8.3f} ms  "
            f"worst {tw*1e3:8.3f} ms; torch / otbx_filter_sel time ratio: "
            f"{tb/fb:.2f}; same result: {same}")
        assert same, f"case ({tag}): torch and otbx_filter_sel disagree"
        del ref
        torch.cuda.empty_cache()
        return fb, fw

    # (a) Q1-shaped count: date <= c, next to the specialised otbx_scan_count
    c98, c01 = 2449, 24
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scan_count():
        call("otbx_scan_count", C.c_void_p(date.data_ptr()), C.c_int64(n),
             C.c_int32(c98), C.c_void_p(out.data_ptr()), stream)

    sb, sw = _best_of_5(scan_count)
    say(f"(a) yardstick otbx_scan_count (date <= {c98}, 4 B/row): best "
        f"{sb*1e3:8.3f} ms  worst {sw*1e3:8.3f} ms (spread "
        f"{(sw-sb)/sb*100:.1f} %)  {n*4/sb/1e12:5.2f} TB/s = "
        f"{n*4/sb/COPY_CEILING*100:4.1f} % of the ceiling; count "
        f"{int(out.item()):_}")
    fc = _FilterCall([[T(date, "<=", c98)]], count_only=True)
    fb, fw = report("a", f"date <= {c98}, count only", fc,
                    lambda: (date <= c98).sum())
    assert fc.count() == int(out.item())
    say(f"    otbx_filter_sel / otbx_scan_count time ratio: {fb/sb:.2f} "
        f"(best / best; difference {(fb-sb)*1e3:+.3f} ms, spreads "
        f"{(fw-fb)*1e3:.3f} ms and {(sw-sb)*1e3:.3f} ms)")
    del fc

    # (b) the same qual with the selection written
    for c in (c98, c01):
        fc = _FilterCall([[T(date, "<=", c)]])
        report("b", f"date <= {c}, selection written", fc,
               lambda: (date <= c).nonzero().squeeze(1))
        del fc
        torch.cuda.empty_cache()

    # (c) four columns: i32, nullable f64, u8 twice in an OR
    def torch_c():
        return ((date <= c98) & (price < 0.5) & (pnull == 0) &
                ((flag == 3) | (flag == 7))).nonzero().squeeze(1)

    fc = _FilterCall([[T(date, "<=", c98)], [T(price, "<", 0.5, nulls=pnull)],
                      [T(flag, "=", 3), T(flag, "=", 7)]])
    report("c", f"date <= {c98} AND price < 0.5 (nullable) AND (flag = 3 OR "
           "flag = 7)", fc, torch_c)
    del fc
    torch.cuda.empty_cache()

    # (d) a 1-in-10^4 clause first: waves without a survivor skip the loads
    # of the later clauses; the same qual with that clause last reads all
    def torch_d():
        return ((rare == 0) & (price < 0.5) & (pnull == 0) &
                ((flag == 3) | (flag == 7))).nonzero().squeeze(1)

    lead = [[T(rare, "=", 0)], [T(price, "<", 0.5, nulls=pnull)],
            [T(flag, "=", 3), T(flag, "=", 7)]]
    fc = _FilterCall(lead)
    db, _ = report("d", "rare = 0 (1 in 10^4) AND price < 0.5 (nullable) AND "
                   "(flag = 3 OR flag = 7), selective clause FIRST", fc,
                   torch_d, extra=" (nominal: B/row counts every column)")
    del fc
    torch.cuda.empty_cache()
    fc = _FilterCall(lead[1:] + lead[:1])
    lb, _ = report("d", "the same qual, selective clause LAST", fc, torch_d)
    say(f"    clause order: last / first time ratio {lb/db:.2f}")
    del fc
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _ProjectCall:
    """otbx_project with everything preallocated; expr as GpuProject takes
    it. bytes_per_row is per OUTPUT row."""

    def __init__(self, expr, sel=None, out_dtype=None):
        self.expr, self.sel = expr, sel
        self.n = len(sel) if sel is not None else expr.n_src
        self.n_src = expr.n_src
        dt = out_dtype or ex._EX_OUT_DTYPE[expr.vtype]
        self.out = torch.empty(self.n, dtype=dt, device="cuda")
        self.nulls = torch.empty(self.n, dtype=torch.uint8, device="cuda") \
            if expr.nullable else None
        self.err = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.dev = expr.to_dev()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        seen = {}
        for ins in expr.program():
            if ins[0] == "col":
                for x in ins[1:]:
                    if x is not None:
                        seen[x.data_ptr()] = x.element_size()
        self.bytes_per_row = sum(seen.values()) + self.out.element_size() + \
            (1 if self.nulls is not None else 0) + (8 if sel is not None else 0)

    def __call__(self):
        call("otbx_project", C.byref(self.dev),
             C.c_void_p(self.sel.data_ptr()) if self.sel is not None else None,
             C.c_int64(self.n), C.c_int64(self.n_src),
             C.c_int32(ex._SORT_TYPE[self.out.dtype]),
             C.c_void_p(self.out.data_ptr()),
             C.c_void_p(self.nulls.data_ptr()) if self.nulls is not None
             else None, C.c_void_p(self.err.data_ptr()), self.stream)


def bench_project(out_path):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --project — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), columns staged, output, mask and "
        "error slot preallocated")
    say("# algorithmic B per output row = referenced columns and masks, each "
        "once + output width [+ 1 output mask] [+ 8 selection entry]")
    g = torch.Generator(device="cuda").manual_seed(17)
    n = 600_000_000
    price = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 1e5
    disc = torch.randint(0, 11, (n,), device="cuda", generator=g) \
        .to(torch.float64) / 100
    tax = torch.randint(0, 9, (n,), device="cuda", generator=g) \
        .to(torch.float64) / 100
    pnull = (torch.rand(n, device="cuda", generator=g) < 0.05).to(torch.uint8)
    flag = torch.randint(0, 25, (n,), dtype=torch.uint8, device="cuda",
                         generator=g)
    date = torch.randint(0, 2500, (n,), dtype=torch.int32, device="cuda",
                         generator=g)
    torch.cuda.empty_cache()
    col = ex.col

    def report(tag, what, pc, torch_fn):
        """torch_fn returns (values, mask-or-None)"""
        pb, pw = _best_of_5(pc)
        assert int(pc.err.item()) == -1, f"case ({tag}) raised"
        rows, bpr = pc.n, pc.bytes_per_row
        tbs = rows * bpr / pb / 1e12
        say(f"({tag}) rows={rows:_} {what}: otbx_project best {pb*1e3:8.3f} ms"
            f"  worst {pw*1e3:8.3f} ms (spread {(pw-pb)/pb*100:.1f} %)  "
            f"{bpr} B/row algorithmic = {rows*bpr/1e9:.2f} GB  {tbs:5.2f} TB/s"
            f" = {tbs*1e12/COPY_CEILING*100:4.1f} % of the 6.29 TB/s copy "
            "ceiling")
        tb, tw = _best_of_5(torch_fn)
        ref, refmask = torch_fn()
        same = bool(torch.equal(ref, pc.out)) and \
            (refmask is None or bool(torch.equal(refmask, pc.nulls)))
        say(f"    plain torch on the same columns: best {tb*1e3:8.3f} ms  "
            f"worst {tw*1e3:8.3f} ms; torch / otbx_project time ratio: "
            f"{tb/pb:.2f}; same result (bit for bit): {same}")
        assert same, f"case ({tag}): torch and otbx_project disagree"
        del ref, refmask
        torch.cuda.empty_cache()
        return pb

    # (a) the Q1 charge expression, no masks
    q1 = "price * (1 - disc) * (1 + tax)"
    pc = _ProjectCall(col(price) * (1 - col(disc)) * (1 + col(tax)))
    report("a", q1, pc, lambda: (price * (1 - disc) * (1 + tax), None))
    del pc
    torch.cuda.empty_cache()

    # (b) the same with a 5 % null mask on price
    def torch_b():
        v = price * (1 - disc) * (1 + tax)
        return v.masked_fill_(pnull != 0, 0.0), pnull.clone()

    pc = _ProjectCall(col(price, pnull) * (1 - col(disc)) * (1 + col(tax)))
    report("b", q1 + ", 5 % NULL price", pc, torch_b)
    del pc
    torch.cuda.empty_cache()

    # (c) a CASE
    pc = _ProjectCall(ex.case(col(flag).eq(3), col(price) * (1 - col(disc)),
                              0.0))
    report("c", "CASE WHEN flag = 3 THEN price * (1 - disc) ELSE 0 END", pc,
           lambda: (torch.where(flag == 3, price * (1 - disc), 0.0), None))
    del pc
    torch.cuda.empty_cache()

    # (d) case (a) through a selection from otbx_filter_sel
    for c in (24, 2449):
        fc = _FilterCall([[ex.qual_term(date, "<=", c)]])
        fc()
        sel = fc.sel[:fc.count()].clone()
        del fc
        torch.cuda.empty_cache()
        pc = _ProjectCall(col(price) * (1 - col(disc)) * (1 + col(tax)),
                          sel=sel)
        report("d", f"{q1} through the selection date <= {c} "
               f"({len(sel)/n*100:.2f} % of {n:_} rows)", pc,
               lambda: (price[sel] * (1 - disc[sel]) * (1 + tax[sel]), None))
        del pc, sel
        torch.cuda.empty_cache()

    # (e) integer division on the i32 column to an I32 output
    pc = _ProjectCall(col(date) / 365, out_dtype=torch.int32)
    report("e", "date / 365 (i32 column, I32 output)", pc,
           lambda: (torch.div(date, 365, rounding_mode="trunc"), None))
    del pc
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


# ---------------- text: LIKE / compare predicates and the gather ----------

P_NAME_WORDS = (
    "almond antique aquamarine azure beige bisque black blanched blue blush "
    "brown burlywood burnished chartreuse chiffon chocolate coral cornflower "
    "cornsilk cream cyan dark deep dim dodger drab firebrick floral forest "
    "frosted gainsboro ghost goldenrod green grey honeydew hot indian ivory "
    "khaki lace lavender lawn lemon light lime linen magenta maroon medium "
    "metallic midnight mint misty moccasin navajo navy olive orange orchid "
    "pale papaya peach peru pink plum powder puff purple red rose rosy royal "
    "saddle salmon sandy seashell sienna sky slate smoke snow spring steel "
    "tan thistle tomato turquoise violet wheat white yellow").split()
COMMENT_WORDS = (
    "special requests packages accounts deposits pending furiously carefully "
    "quickly slyly blithely ironic final regular express bold even silent "
    "unusual theodolites pinto beans foxes instructions dependencies excuses "
    "platelets asymptotes courts dolphins sleep wake nag haggle about above "
    "according across after against along the").split()
SHIP_MODES = ["REG AIR", "AIR", "RAIL", "SHIP", "TRUCK", "MAIL", "FOB"]


def _word_rows(words, per_row, n, gen):
    """n rows of per_row random words joined by single spaces, built on the
    device by the text gather itself: a dictionary column holds every word
    with and without a trailing space, one gathered entry per word, and the
    row offsets are every per_row-th offset of the gathered column. A 1 %
    null mask rides along (the NULL rows keep their bytes)."""
    d = ex.GpuText([w + " " for w in words] + list(words))
    ids = torch.randint(0, len(words), (n, per_row), device="cuda",
                        generator=gen)
    ids[:, per_row - 1] += len(words)            # last word: no space
    g = d.gather(ids.reshape(-1))
    del ids
    offs = g.offs[::per_row].contiguous()
    nulls = (torch.rand(n, device="cuda", generator=gen) < 0.01) \
        .to(torch.uint8)
    return ex.GpuText(bytes=g.bytes, offs=offs, nulls=nulls)


class _TextPredCall:
    """otbx_text_pred with the outputs preallocated."""

    def __init__(self, text, op, rhs, sel=None):
        self.node = ex.GpuTextPred(text, op, rhs, sel=sel)
        self.p, self.right = self.node.pred()
        self.n, self.n_src, self.sel = self.node.n, self.node.n_src, sel
        self.out = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        self.nulls = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        call("otbx_text_pred", C.byref(self.p),
             C.c_void_p(self.sel.data_ptr()) if self.sel is not None else None,
             C.c_int64(self.n), C.c_int64(self.n_src),
             C.c_void_p(self.out.data_ptr()),
             C.c_void_p(self.nulls.data_ptr()), self.stream)

    def count(self):
        return int(((self.out != 0) & (self.nulls == 0)).sum().item())


def _torch_text_gather(text, perm):
    """the gathered bytes and offsets built with plain torch"""
    starts, ends = text.offs[:-1][perm], text.offs[1:][perm]
    lens = ends - starts
    doffs = torch.zeros(len(perm) + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=doffs[1:])
    total = int(doffs[-1].item())
    src = torch.repeat_interleave(starts - doffs[:-1], lens) + \
        torch.arange(total, device="cuda")
    return text.bytes[src], doffs


def bench_text(out_path, sizes):
    import numpy as np
    sys.path.insert(0, os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from text_ref import like_rec
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# tools/generic_ops_bench.py --text — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), columns staged, outputs "
        "preallocated; every column carries a 1 % null mask")
    say("# predicate: algorithmic B per row = text bytes + 8 offsets + 1 mask "
        "+ 2 out (value, null) [+ 8 selection entry, per output row]")
    say("# gather: algorithmic B per output row = 2 x text bytes + 16 offsets "
        "(read, write) + 8 perm; offsets pass and byte pass timed together, "
        "with the one read-back of the total between them")
    say("# staged = OTBX_TEXT_STAGE=1, tile bytes copied to LDS first; direct "
        "= OTBX_TEXT_STAGE=0, every row read from global memory; default = "
        "unset, the library's rule (staged only for a LIKE with a % before "
        "the pattern's last token)")
    gen = torch.Generator(device="cuda").manual_seed(23)

    def pred_line(tag, what, text, op, rhs, sel=None):
        res = {}
        for mode in ("staged", "direct", "default"):
            if mode == "default":
                os.environ.pop("OTBX_TEXT_STAGE", None)
            else:
                os.environ["OTBX_TEXT_STAGE"] = "1" if mode == "staged" \
                    else "0"
            pc = _TextPredCall(text, op, rhs, sel=sel)
            b, w = _best_of_5(pc)
            res[mode] = (b, w, pc.count(), pc.out.clone())
            rows = pc.n
            if sel is None:
                tbytes = int((text.offs[-1] - text.offs[0]).item())
                alg = tbytes + rows * 11
            else:
                tbytes = int((text.offs[1:][sel] - text.offs[:-1][sel])
                             .sum().item())
                alg = tbytes + rows * 19
            tbs = alg / b / 1e12
            say(f"({tag}) rows={rows:_} {what} [{mode}]: best {b*1e3:8.3f} ms"
                f"  worst {w*1e3:8.3f} ms (spread {(w-b)/b*100:.1f} %)  "
                f"{alg/max(rows,1):.1f} B/row algorithmic = {alg/1e9:.2f} GB  "
                f"{tbs:5.2f} TB/s = {tbs*1e12/COPY_CEILING*100:4.1f} % of the "
                f"6.29 TB/s copy ceiling; TRUE rows {res[mode][2]:_}")
            del pc
        os.environ.pop("OTBX_TEXT_STAGE", None)
        same = bool(torch.equal(res["staged"][3], res["direct"][3])) and \
            bool(torch.equal(res["default"][3], res["direct"][3]))
        say("    staged / direct time ratio "
            f"{res['staged'][0]/res['direct'][0]:.2f}; same result in all "
            f"three: {same}")
        assert same, f"case ({tag}): staged and direct disagree"
        return res["staged"][3]

    def gather_line(tag, what, text, perm, verify):
        def run():
            return text.gather(perm)
        b, w = _best_of_5(run)
        g = run()
        rows, tbytes = len(perm), len(g.bytes)
        alg = 2 * tbytes + rows * 24
        tbs = alg / b / 1e12
        say(f"({tag}) rows={rows:_} {what}: best {b*1e3:8.3f} ms  worst "
            f"{w*1e3:8.3f} ms (spread {(w-b)/b*100:.1f} %)  "
            f"{alg/max(rows,1):.1f} B/row algorithmic = {alg/1e9:.2f} GB  "
            f"{tbs:5.2f} TB/s = {tbs*1e12/COPY_CEILING*100:4.1f} % of the "
            "6.29 TB/s copy ceiling")
        if verify:
            tb, toffs = _torch_text_gather(text, perm)
            same = bool(torch.equal(tb, g.bytes)) and \
                bool(torch.equal(toffs, g.offs))
            say(f"    byte-equal to the torch-built copy: {same}")
            assert same, f"case ({tag}): gather differs from torch"
            del tb, toffs
        else:
            say("    byte comparison with torch: not run at this size")
        del g
        torch.cuda.empty_cache()

    for n in sizes:
        say()
        say(f"## {n:_} rows")
        name = _word_rows(P_NAME_WORDS, 5, n, gen)
        nb = len(name.bytes)
        say(f"# part names: {nb/n:.1f} B/row, {nb/1e9:.2f} GB")
        green = pred_line("a", "p_name LIKE '%green%' (Q9)", name, "like",
                          "%green%")
        pred_line("b", "p_name LIKE 'forest%' (Q20)", name, "like", "forest%")

        if n == sizes[0]:
            # counted: the first 1 M rows against the reference's matcher
            # (the prefix is copied out first, so that only it goes to the
            # host)
            m = min(n, 1_000_000)
            host = name.slice(0, m).gather(
                torch.arange(m, device="cuda")).to_list()
            want = sum(1 for r in host if r is not None and
                       like_rec(r, b"%green%"))
            pm = _TextPredCall(name.slice(0, m), "like", "%green%")
            pm()
            say(f"    '%green%' on the first {m:_} rows: otbx_text_pred "
                f"selects {pm.count():_}, the reference loop {want:_}")
            assert pm.count() == want
            del pm, host

            # numpy on one core over the same bytes, as a fixed-width array
            width = int((name.offs[1:] - name.offs[:-1]).max().item())
            idx = name.offs[:-1, None] + torch.arange(width, device="cuda")
            keep = idx < name.offs[1:, None]
            fixed = torch.where(keep, name.bytes[idx.clamp_(max=nb - 1)],
                                torch.zeros((), dtype=torch.uint8,
                                            device="cuda"))
            arr = fixed.cpu().numpy().view(f"S{width}").reshape(-1)
            del idx, keep, fixed
            t0 = time.time()
            hit = np.char.find(arr, b"green") >= 0
            th = time.time() - t0
            valid = name.nulls.cpu().numpy() == 0
            same = bool(np.array_equal(hit & valid, green.cpu().numpy() != 0))
            say(f"    numpy np.char.find(names, 'green') >= 0 on one core, "
                f"S{width} array: {th*1e3:.0f} ms (one run); same rows: {same}")
            assert same
            del arr, hit

        key = torch.randint(0, 100, (n,), dtype=torch.int32, device="cuda",
                            generator=gen)
        fc = _FilterCall([[ex.qual_term(key, "<", 6)]])
        fc()
        sel = fc.sel[:fc.count()].clone()
        del fc
        pred_line("e", f"p_name LIKE '%green%' through a "
                  f"{len(sel)/n*100:.1f} % selection", name, "like",
                  "%green%", sel=sel)
        srt = ex.GpuSort([torch.randint(0, 2**62, (n,), device="cuda",
                                        generator=gen)])
        srt.BeginCustomScan()
        perm = srt.ExecCustomScan()
        srt.EndCustomScan()
        del srt
        torch.cuda.empty_cache()
        gather_line("f", "p_name gathered through a sort permutation", name,
                    perm, verify=n <= 20_000_000)
        del perm
        gather_line("g", f"p_name gathered through the "
                    f"{len(sel)/n*100:.1f} % selection", name, sel,
                    verify=True)
        del name, sel, key, green
        torch.cuda.empty_cache()

        comment = _word_rows(COMMENT_WORDS, 8, n, gen)
        say(f"# comments: {len(comment.bytes)/n:.1f} B/row")
        pred_line("c", "o_comment LIKE '%special%requests%' (Q13)", comment,
                  "like", "%special%requests%")
        del comment
        torch.cuda.empty_cache()
        mode = _word_rows(SHIP_MODES, 1, n, gen)
        say(f"# ship modes: {len(mode.bytes)/n:.1f} B/row")
        pred_line("d", "l_shipmode = 'MAIL' (Q12)", mode, "=", "MAIL")
        del mode
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


class _TextRankCall:
    """otbx_text_rank with the workspace and outputs preallocated."""

    def __init__(self, text):
        self.node = ex.GpuTextRank([text])
        self.ts = self.node.textset()
        self.n = n = len(text)
        wsb = C.c_size_t(0)
        lib().otbx_text_rank_workspace_bytes(C.c_int64(n), C.byref(wsb))
        self.ws_bytes = wsb.value
        self.ws = torch.empty((wsb.value + 7) // 8, dtype=torch.int64,
                              device="cuda")
        self.codes = torch.empty(n, dtype=torch.int64, device="cuda")
        self.drow = torch.empty(n, dtype=torch.int64, device="cuda")
        self.nd = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.rounds = C.c_int32(0)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def __call__(self):
        call("otbx_text_rank", C.byref(self.ts), C.c_void_p(self.ws.data_ptr()),
             C.c_size_t(self.ws_bytes), C.c_void_p(self.codes.data_ptr()),
             C.c_void_p(self.drow.data_ptr()), C.c_void_p(self.nd.data_ptr()),
             C.byref(self.rounds), self.stream)


def bench_textkey(out_path, name_sizes, mode_sizes, one=None, one_mode=None):
    import numpy as np
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator(device="cuda").manual_seed(29)
    if one is not None or one_mode is not None:
        # one call for a kernel tracer: no warm-up, no repetition
        text = _word_rows(P_NAME_WORDS, 5, one, gen) if one is not None \
            else _word_rows(SHIP_MODES, 1, one_mode, gen)
        rc = _TextRankCall(text)
        rc()
        print(f"rank of {rc.n:_} rows, {len(text.bytes)/rc.n:.1f} B/row: "
              f"rounds {rc.rounds.value}, {int(rc.nd.item()):_} distinct")
        return

    say("# tools/generic_ops_bench.py --textkey — best / worst of 5 wall time "
        "after torch.cuda.synchronize(), one warm-up, all in one process; "
        "columns staged, workspace and outputs preallocated; every column "
        "carries a 1 % null mask")
    say("# otbx_text_rank is synchronous (one int64 read back per round); the "
        "time is the whole call. Per-kernel split of the rounds: "
        "profiles/textkey_kernel_trace.txt")
    say("# extraction pass, algorithmic B per undecided row and round: 8 "
        "chunk bytes read (or what is left of the row) + 8 offset + 1 mask "
        "(round 0) + 4 row id and 4 group id (later rounds) read; 4 + 8 + 1 "
        "(+ 1) written")

    def rank_line(tag, what, text):
        rc = _TextRankCall(text)
        b, w = _best_of_5(rc)
        n, d, r = rc.n, int(rc.nd.item()), rc.rounds.value
        say(f"({tag}) rows={n:_} {what}: best {b*1e3:9.3f} ms  worst "
            f"{w*1e3:9.3f} ms (spread {(w-b)/b*100:.1f} %)  "
            f"{n/b/1e9:.3f} G rows/s; rounds {r}, distinct {d:_}, workspace "
            f"{rc.ws_bytes/max(n,1):.1f} B/row")
        return rc

    for n in name_sizes:
        say()
        say(f"## part names, {n:_} rows")
        name = _word_rows(P_NAME_WORDS, 5, n, gen)
        say(f"# {len(name.bytes)/n:.1f} B/row, {len(name.bytes)/1e9:.2f} GB")
        rc = rank_line("a", "rank of p_name", name)
        if n == name_sizes[0]:
            # numpy on one core over the same non-NULL names, as a
            # fixed-width array; also the check of the codes at this size
            nb = len(name.bytes)
            width = int((name.offs[1:] - name.offs[:-1]).max().item())
            idx = name.offs[:-1, None] + torch.arange(width, device="cuda")
            keep = idx < name.offs[1:, None]
            fixed = torch.where(keep, name.bytes[idx.clamp_(max=nb - 1)],
                                torch.zeros((), dtype=torch.uint8,
                                            device="cuda"))
            valid = name.nulls.cpu().numpy() == 0
            arr = fixed.cpu().numpy().view(f"S{width}").reshape(-1)[valid]
            del idx, keep, fixed
            t0 = time.time()
            uniq, inv = np.unique(arr, return_inverse=True)
            th = time.time() - t0
            codes = rc.codes.cpu().numpy()
            same = bool(np.array_equal(codes[valid], inv.reshape(-1))) and \
                bool((codes[~valid] == -1).all()) and \
                len(uniq) == int(rc.nd.item())
            say(f"    numpy np.unique(names, return_inverse=True) on one "
                f"core, S{width} array of the {len(arr):_} non-NULL names: "
                f"{th*1e3:.0f} ms (one run); codes equal: {same}")
            assert same
            del arr, uniq, inv, codes

        # ORDER BY p_name: rank + sort on the codes + gather of the text
        def order_by():
            r = name.rank()
            srt = ex.GpuSort([r.codes[0]], nulls=[name.nulls])
            srt.BeginCustomScan()
            perm = srt.ExecCustomScan()
            srt.EndCustomScan()
            return name.gather(perm)
        del rc
        torch.cuda.empty_cache()
        b, w = _best_of_5(order_by)
        say(f"(c) rows={n:_} ORDER BY p_name end to end (rank + GpuSort + text "
            f"gather, allocations included): best {b*1e3:9.3f} ms  worst "
            f"{w*1e3:9.3f} ms (spread {(w-b)/b*100:.1f} %)")
        if n == name_sizes[0]:
            g = order_by()
            m = min(n, 1_000_000)
            head = g.slice(0, m).gather(torch.arange(m, device="cuda"))
            host = head.to_list()
            ok = all(x <= y for x, y in zip(host, host[1:])
                     if x is not None and y is not None)
            say(f"    first {m:_} output rows ascending on the host: {ok}")
            assert ok
            del g, head, host
        del name
        torch.cuda.empty_cache()

    for n in mode_sizes:
        say()
        say(f"## ship modes, {n:_} rows")
        mode = _word_rows(SHIP_MODES, 1, n, gen)
        say(f"# {len(mode.bytes)/n:.1f} B/row")
        rc = rank_line("b", "rank of l_shipmode", mode)
        d = rc.drow[:int(rc.nd.item())].clone()
        assert mode.gather(d).to_list() == \
            sorted(w.encode() for w in SHIP_MODES)
        del rc
        torch.cuda.empty_cache()
        if n == mode_sizes[0]:
            ones = torch.ones(n, dtype=torch.float64, device="cuda")
            res = {}

            def group_by():
                r = mode.rank()
                agg = ex.GpuHashAgg(r.codes[0], ones, key_null=mode.nulls)
                agg.BeginCustomScan()
                res["rows"] = agg._run()
                agg.EndCustomScan()
                res["rank"] = r
            b, w = _best_of_5(group_by)
            say(f"(d) rows={n:_} GROUP BY l_shipmode count(*) end to end "
                f"(rank + hash aggregate, allocations included): best "
                f"{b*1e3:9.3f} ms  worst {w*1e3:9.3f} ms (spread "
                f"{(w-b)/b*100:.1f} %)")
            total = sum(int(g["count_star"]) for g in res["rows"])
            names = res["rank"].dictionary().to_list()
            say(f"    groups: {len(res['rows'])} (7 modes + NULL), rows "
                f"counted {total:_}; dictionary {names}")
            assert total == n and len(res["rows"]) == 8
            del ones, res
        del mode
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _sizes_arg(flag, default):
    if flag in sys.argv:
        return [int(x) for x in sys.argv[sys.argv.index(flag) + 1].split(",")]
    return default


if __name__ == "__main__":
    ex.init_device(0)
    if "--textkey" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "textkey_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        one = _sizes_arg("--one", [None])[0]
        one_mode = _sizes_arg("--one-mode", [None])[0]
        bench_textkey(out_path,
                      _sizes_arg("--rows", [20_000_000, 200_000_000]),
                      _sizes_arg("--mode-rows", [200_000_000, 600_000_000]),
                      one=one, one_mode=one_mode)
        sys.exit(0)
    if "--text" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "text_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        sizes = [20_000_000, 200_000_000]
        if "--rows" in sys.argv:
            sizes = [int(x) for x in
                     sys.argv[sys.argv.index("--rows") + 1].split(",")]
        bench_text(out_path, sizes)
        sys.exit(0)
    if "--project" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "project_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        bench_project(out_path)
        sys.exit(0)
    if "--filter" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "filter_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        bench_filter(out_path)
        sys.exit(0)
    if "--winframe" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "winframe_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        bench_winframe(out_path, _sizes_arg("--rows", [600_000_000])[0],
                       _sizes_arg("--ab-rows", [200_000_000])[0])
        sys.exit(0)
    if "--ordagg" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "ordagg_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        rows = 600_000_000
        if "--rows" in sys.argv:
            rows = int(sys.argv[sys.argv.index("--rows") + 1])
        bench_ordagg(out_path, rows)
        sys.exit(0)
    if "--groupagg" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "groupagg_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        rows = 600_000_000
        if "--rows" in sys.argv:
            rows = int(sys.argv[sys.argv.index("--rows") + 1])
        bench_groupagg(out_path, rows)
        sys.exit(0)
    if "--window" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "window_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        bench_window(out_path)
        sys.exit(0)
    if "--sort" in sys.argv:
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out_path = os.path.join(repo, "profiles", "sort_ops.txt")
        if "--out" in sys.argv:
            out_path = sys.argv[sys.argv.index("--out") + 1]
        bench_sort(out_path)
        sys.exit(0)
    if "--agg-var" in sys.argv:
        for groups in (4, 1_000_000, 100_000_000):
            t_agg = bench_agg(600_000_000, groups)
            torch.cuda.empty_cache()
            t_var = bench_agg_var(600_000_000, groups)
            torch.cuda.empty_cache()
            print(f"agg_var / agg time ratio at groups={groups:_}: "
                  f"{t_var / t_agg:.2f}")
        sys.exit(0)
    bench_agg(600_000_000, 4)
    bench_agg(600_000_000, 1_000_000)
    bench_agg(600_000_000, 100_000_000)
    bench_join(15_000_000, 600_000_000)
    bench_join(150_000_000, 600_000_000)
    if "--round2-ops" in sys.argv:
        bench_round2_ops()

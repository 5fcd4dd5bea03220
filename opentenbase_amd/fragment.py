"""Coordinator shard-merge over RCCL/xGMI — the MI355X-native replacement of
the reference's RemoteSubplan recv + FN transport (execFragment.c:3877,
forward/*; SURVEY §2 'Fragment exchange'). Semantics: per-shard partial-agg
streams are CONCATENATED at the CN and combined by the Finalize Aggregate
(float8pl / int8pl / float8_combine — nodeAgg.c:3912,4260).

One process per GPU (1 DN shard ↔ 1 GPU); collectives via torch.distributed —
backend "nccl" IS RCCL on ROCm (xGMI inside the node); CPU tests use "gloo"
with the same code path.
"""
import math

import torch
import torch.distributed as dist

from ._lib import OtbxError
from .executor import VAR_GROUP_DTYPE, q1_finalize, q1_rows_from_state


def is_dist():
    return dist.is_available() and dist.is_initialized()


def merge_q1_partials(sums, counts):
    """All-gather the dense per-rank Q1 partial states (6×5 sums + 6 counts —
    the 'Remote Subquery Scan' payload: 4 rows/DN) and combine on every rank
    (combine is cheap and keeping it symmetric avoids a broadcast back).

    Dense slot layout makes the combine a pure elementwise sum: float8pl for
    sums, int8pl for counts, slot-aligned groups."""
    if not is_dist() or dist.get_world_size() == 1:
        return q1_rows_from_state(sums, counts)
    if dist.get_backend() == "gloo" and sums.is_cuda:
        sums, counts = sums.cpu(), counts.cpu()
    world = dist.get_world_size()
    gs = [torch.empty_like(sums) for _ in range(world)]
    gc = [torch.empty_like(counts) for _ in range(world)]
    dist.all_gather(gs, sums)
    dist.all_gather(gc, counts)
    tot_s = torch.zeros_like(sums)
    tot_c = torch.zeros_like(counts)
    for s in gs:
        tot_s += s            # float8pl chain over shards
    for c in gc:
        tot_c += c            # int8pl
    return q1_rows_from_state(tot_s, tot_c)


def merge_q9_partials(sums, counts):
    """Q9-mix shard merge: all-gather + elementwise combine of the dense
    [7]-year partial states (same RemoteSubplan payload shape as Q1)."""
    from .executor import q9_rows_from_state
    if not is_dist() or dist.get_world_size() == 1:
        return q9_rows_from_state(sums, counts)
    if dist.get_backend() == "gloo" and sums.is_cuda:
        sums, counts = sums.cpu(), counts.cpu()
    dist.all_reduce(sums)      # float8pl over shards
    dist.all_reduce(counts)    # int8pl
    return q9_rows_from_state(sums, counts)


def allgather_variable(t):
    """All-gather a 1-D tensor with per-rank variable length (the FN-page
    concatenation semantics). Returns the concatenation over ranks."""
    if not is_dist() or dist.get_world_size() == 1:
        return t
    if dist.get_backend() == "gloo" and t.is_cuda:
        t = t.cpu()
    world = dist.get_world_size()
    n = torch.tensor([t.numel()], dtype=torch.int64, device=t.device)
    ns = [torch.empty_like(n) for _ in range(world)]
    dist.all_gather(ns, n)
    counts = [int(x.item()) for x in ns]
    mx = max(counts) if counts else 0
    pad = torch.empty(mx, dtype=t.dtype, device=t.device)
    pad[: t.numel()] = t
    outs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(outs, pad)
    return torch.cat([o[:c] for o, c in zip(outs, counts)])


def broadcast_customer_keys(local_keys):
    """Q3 replicated build side: all-gather each rank's filtered customer
    keys (reference analog: replicated distribution / 'Distribute results by'
    exchange, xl_join.out:13-20). Shards are disjoint (custkey % nranks), so
    concatenation = the full filtered key set."""
    return allgather_variable(local_keys)


def merge_q3_topk(candidates, k=10):
    """All-gather per-rank top-k candidate rows (as raw bytes) and take the
    global top-k (merge-sorted recv analog, execFragment.c:4035-4059)."""
    import numpy as np
    dt = np.dtype([("l_orderkey", "i8"), ("revenue", "f8"),
                   ("o_orderdate", "i4"), ("o_shippriority", "i4")])
    if is_dist() and dist.get_world_size() > 1:
        raw = torch.from_numpy(
            np.ascontiguousarray(candidates).view(np.uint8).reshape(-1).copy())
        dev = "cuda" if torch.cuda.is_available() and \
            dist.get_backend() == "nccl" else "cpu"
        raw = raw.to(dev)
        allraw = allgather_variable(raw).cpu().numpy().tobytes()
        cands = np.frombuffer(allraw, dtype=dt).copy()
    else:
        cands = np.asarray(candidates, dtype=dt)
    order = np.lexsort((cands["l_orderkey"], cands["o_orderdate"],
                        -cands["revenue"]))
    return cands[order][:k]


def _sort_norm_host(col, flags, null):
    """numpy restatement of the device key normalisation of otbx_sort_perm
    (DESIGN.md §8g.1): returns (null digit u8, radix key u64) whose
    ascending order is the column's ORDER BY order."""
    import numpy as np
    a = np.ascontiguousarray(col)
    top = np.uint64(1 << 63)
    if a.dtype == np.int64:
        k, mask = a.view(np.uint64) ^ top, np.uint64(0xffffffffffffffff)
    elif a.dtype == np.float64:
        b = a.view(np.uint64).copy()
        b[np.isnan(a)] = np.uint64(0x7ff8000000000000)  # one NaN, above +Inf
        b[a == 0] = np.uint64(0)                        # -0 == +0
        k = np.where((b >> np.uint64(63)) != 0, ~b, b ^ top)
        mask = np.uint64(0xffffffffffffffff)
    elif a.dtype == np.int32:
        k = (a.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
        mask = np.uint64(0xffffffff)
    elif a.dtype == np.uint8:
        k, mask = a.astype(np.uint64), np.uint64(0xff)
    else:
        raise OtbxError(3, f"sort: unsupported key dtype {a.dtype}")
    if flags & 1:                                       # OTBX_SORT_DESC
        k = k ^ mask
    isnull = np.zeros(len(a), dtype=bool) if null is None \
        else np.asarray(null) != 0
    k = np.where(isnull, np.uint64(0), k)
    nfirst = bool(flags & 2)                            # OTBX_SORT_NULLS_FIRST
    nd = np.where(isnull, 0 if nfirst else 1, 1 if nfirst else 0)
    return nd.astype(np.uint8), k


def merge_sorted_partials(key_cols, payload_cols, descending=None,
                          nulls_first=None, nulls=None, limit=0):
    """Coordinator merge of sorted DataNode streams (the merge-sorted recv of
    execFragment.c:4035-4059). Every rank passes its locally sorted rows
    (already cut to `limit` if set): key columns, payload columns and the
    optional per-key null masks, as 1-D tensors. They are all-gathered in
    rank order and ordered globally — by GpuSort when the gathered tensors
    are on the device (nccl), by a stable numpy lexsort over the same
    normalised keys when they are on the CPU (gloo). The result is, by
    definition, the stable sort of the rank-ordered concatenation, cut to
    `limit`. Returns (keys, payloads, nulls) as lists of tensors. With one
    rank or no process group the input is returned as is. All ranks must
    pass the same columns (a null mask on one rank = on every rank)."""
    from . import executor as ex
    key_cols, payload_cols = list(key_cols), list(payload_cols)
    nk = len(key_cols)
    nulls = [None] * nk if nulls is None else list(nulls)
    flags = ex.sort_flags(nk, descending, nulls_first)
    if not is_dist() or dist.get_world_size() == 1:
        return key_cols, payload_cols, nulls
    gk = [allgather_variable(k) for k in key_cols]
    gp = [allgather_variable(p) for p in payload_cols]
    gn = [None if m is None else allgather_variable(m) for m in nulls]
    if gk[0].is_cuda:
        node = ex.GpuSort(gk, [bool(f & 1) for f in flags],
                          [bool(f & 2) for f in flags], gn, limit)
        node.BeginCustomScan()
        perm = node.ExecCustomScan()
        node.EndCustomScan()

        def take(t):
            return ex.gather(t, perm)
    else:
        import numpy as np
        cols = []   # np.lexsort: LAST entry is the primary key
        for c in range(nk - 1, -1, -1):
            nd, k = _sort_norm_host(gk[c].numpy(), flags[c],
                                    None if gn[c] is None else gn[c].numpy())
            cols += [k, nd]
        order = np.lexsort(cols)
        if limit > 0:
            order = order[:limit]
        perm = torch.from_numpy(order.astype(np.int64))

        def take(t):
            return t[perm]
    return ([take(k) for k in gk], [take(p) for p in gp],
            [None if m is None else take(m) for m in gn])


def combine_var_state(a, b):
    """float8_combine (float.c:2725) on two [N, Sx, Sxx] transition states:
    the generalised Youngs-Cramer merge, in the reference's operation order
    (so the result is bit-identical to the C function). An empty side
    (N == 0) returns the other unchanged. A finite-input overflow is an
    error, as the reference's float_overflow_error()."""
    N1, Sx1, Sxx1 = float(a[0]), float(a[1]), float(a[2])
    N2, Sx2, Sxx2 = float(b[0]), float(b[1]), float(b[2])
    if N1 == 0.0:
        return (N2, Sx2, Sxx2)
    if N2 == 0.0:
        return (N1, Sx1, Sxx1)
    N = N1 + N2
    Sx = Sx1 + Sx2
    if math.isinf(Sx) and not math.isinf(Sx1) and not math.isinf(Sx2):
        raise OtbxError(4, "float8_combine: Sx overflow")
    tmp = Sx1 / N1 - Sx2 / N2
    Sxx = Sxx1 + Sxx2 + N1 * N2 * tmp * tmp / N
    if math.isinf(Sxx) and not math.isinf(Sxx1) and not math.isinf(Sxx2):
        raise OtbxError(4, "float8_combine: Sxx overflow")
    return (N, Sx, Sxx)


def merge_var_partials(rows):
    """Coordinator merge of a grouped variance: all-gather every rank's
    GpuHashAggVar rows (otbx_var_group records, as raw bytes — the
    merge_q3_topk pattern), then combine rows of equal (key_isnull, key) in
    rank order: float8_combine on [count_v, sum_v, sxx], int8pl on
    count_star. Returns rows sorted like the node's output. With one rank
    or no process group the input is returned as is."""
    if not is_dist() or dist.get_world_size() == 1:
        return rows
    import numpy as np
    dt = np.dtype(VAR_GROUP_DTYPE)
    local = np.array([tuple(r[f] for f in dt.names) for r in rows], dtype=dt)
    raw = torch.from_numpy(local.view(np.uint8).reshape(-1).copy())
    dev = "cuda" if torch.cuda.is_available() and \
        dist.get_backend() == "nccl" else "cpu"
    raw = raw.to(dev)
    allraw = allgather_variable(raw).cpu().numpy().tobytes()
    parts = np.frombuffer(allraw, dtype=dt)
    merged = {}  # (key_isnull, key) -> [count_star, (N, Sx, Sxx)]
    for r in parts:                       # concatenation is in rank order
        ident = (int(r["key_isnull"]), int(r["key"]))
        st = (float(r["count_v"]), float(r["sum_v"]), float(r["sxx"]))
        m = merged.get(ident)
        if m is None:
            merged[ident] = [int(r["count_star"]), st]
        else:
            m[0] += int(r["count_star"])
            m[1] = combine_var_state(m[1], st)
    out = np.zeros(len(merged), dtype=dt)
    for i, ident in enumerate(sorted(merged)):
        cs, (N, Sx, Sxx) = merged[ident]
        out[i] = (ident[1], cs, int(N), Sx, Sxx, ident[0], int(N == 0.0))
    return list(out)


def combine_group_partials(keys, key_nulls, flags, aggs):
    """The Finalize step of merge_group_partials on the gathered stream
    (host numpy; the inputs are group-sized). keys / key_nulls: the key
    columns and masks of every rank's group rows, concatenated in rank
    order; flags: the per-key OTBX_SORT_* words; aggs: one tuple per
    aggregate,
        ("count_star" | "count", val, None)
        ("sum" | "min" | "max", val, null)     val typed as the node's output
        ("sum128", lo, hi, null)               the int64 SUM's int128 state
    Rows are ordered by key (stable: rank order inside equal keys) and
    adjacent equal keys — equal under the sort's normalised key — are
    combined left to right, NULL partials skipped: counts by int8pl, F64
    sums by float8pl, integer sums exactly (int128 with carry), MIN / MAX
    under the operator's comparator, the later rank winning a tie. Returns
    (keys, key_nulls, aggs) of the combined rows; keys are those of each
    group's first row."""
    import numpy as np
    keys = [np.asarray(k) for k in keys]
    nk = len(keys)
    n = len(keys[0]) if nk else (len(aggs[0][1]) if aggs else 0)
    cols = []   # np.lexsort: LAST entry is the primary key
    norm = []
    for c in range(nk):
        m = None if key_nulls[c] is None else np.asarray(key_nulls[c])
        nd, k = _sort_norm_host(keys[c], flags[c], m)
        norm.append((nd, k))
    for nd, k in reversed(norm):
        cols += [k, nd]
    order = np.lexsort(cols) if cols else np.arange(n)
    start = np.zeros(n, dtype=bool)
    if n:
        start[0] = True
    for nd, k in norm:
        nd, k = nd[order], k[order]
        start[1:] |= (nd[1:] != nd[:-1]) | (k[1:] != k[:-1])
    starts = np.flatnonzero(start)
    ng = len(starts)
    gid = np.cumsum(start) - 1
    slot = np.arange(n) - starts[gid] if n else np.zeros(0, dtype=np.int64)
    width = int(slot.max()) + 1 if n else 0

    def fold(parts, null, step):
        """left-to-right over each group's partials; parts: arrays in
        gathered order. Returns (accumulators, isnull)."""
        parts = [np.asarray(p)[order] for p in parts]
        live = np.ones(n, dtype=bool) if null is None else \
            np.asarray(null)[order] == 0
        acc = [np.zeros(ng, dtype=p.dtype) for p in parts]
        has = np.zeros(ng, dtype=bool)
        for s in range(width):
            rows = np.flatnonzero((slot == s) & live)
            g = gid[rows]
            new = [p[rows] for p in parts]
            old = [a[g] for a in acc]
            both = has[g]
            res = step(old, new)
            for a, r, x in zip(acc, res, new):
                a[g] = np.where(both, r, x)
            has[g] = True
        return acc, (~has).astype(np.uint8)

    u64 = np.uint64

    def add(old, new):
        with np.errstate(invalid="ignore", over="ignore"):
            return [old[0] + new[0]]

    def add128(old, new):
        lo = old[0] + new[0]                       # uint64, wraps
        carry = (lo < old[0]).astype(np.int64)
        with np.errstate(over="ignore"):
            return [lo, old[1] + new[1] + carry]

    def pick(is_max):
        def step(old, new):
            a = _sort_norm_host(old[0], 0, None)[1]
            b = _sort_norm_host(new[0], 0, None)[1]
            keep = a > b if is_max else a < b      # strictly: a tie → later
            return [np.where(keep, old[0], new[0])]
        return step

    out = []
    for a in aggs:
        func = a[0]
        if func in ("count_star", "count"):
            acc, _ = fold([np.asarray(a[1]).astype(np.int64)], None, add)
            out.append((acc[0], None))
        elif func == "sum128":
            lo = np.asarray(a[1])
            lo = lo.view(u64) if lo.dtype == np.int64 else lo.astype(u64)
            acc, isnull = fold([lo, np.asarray(a[2]).astype(np.int64)], a[3],
                               add128)
            out.append((acc[0], acc[1], isnull))
        elif func == "sum":
            acc, isnull = fold([a[1]], a[2], add)
            out.append((acc[0], isnull))
        elif func in ("min", "max"):
            acc, isnull = fold([a[1]], a[2], pick(func == "max"))
            out.append((acc[0], isnull))
        else:
            raise OtbxError(3, f"merge_group_partials: unknown aggregate "
                               f"{func}")
    first = order[starts] if n else order[:0]
    return ([k[first] for k in keys],
            [None if m is None else np.asarray(m)[first] for m in key_nulls],
            out)


def merge_group_partials(keys, aggs, key_nulls=None, descending=None,
                         nulls_first=None):
    """Coordinator combine of a GpuGroupAgg (the Finalize Aggregate above
    the gathered Partial GroupAggregate rows): every rank passes its group
    rows — key columns, optional key masks, and per aggregate the tuple
    combine_group_partials describes (tensors or numpy arrays; an int64 SUM
    as ("sum128", lo, hi, null)). The rows are all-gathered in rank order
    with allgather_variable, ordered by key with the sort's own normalised
    key and combined by combine_group_partials. Host-side numpy, as
    merge_var_partials: the inputs are group-sized. Returns (keys,
    key_nulls, aggs) as numpy arrays in key order. With one rank or no
    process group the input is returned unchanged. All ranks must pass the
    same columns (a mask on one rank = on every rank)."""
    from . import executor as ex
    import numpy as np
    nk = len(keys)
    key_nulls = [None] * nk if key_nulls is None else list(key_nulls)
    flags = ex.sort_flags(nk, descending, nulls_first)
    if not is_dist() or dist.get_world_size() == 1:
        return keys, key_nulls, aggs
    dev = "cuda" if torch.cuda.is_available() and \
        dist.get_backend() == "nccl" else "cpu"

    def gathered(a):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a)
            dt = a.dtype
            if dt == np.uint64:                    # torch moves it as int64
                a = a.view(np.int64)
            out = allgather_variable(torch.from_numpy(a).to(dev))
            out = out.cpu().numpy()
            return out.view(np.uint64) if dt == np.uint64 else out
        return allgather_variable(a.to(dev)).cpu().numpy()

    gk = [gathered(k) for k in keys]
    gn = [gathered(m) for m in key_nulls]
    ga = [(a[0],) + tuple(gathered(x) for x in a[1:]) for a in aggs]
    return combine_group_partials(gk, gn, flags, ga)


def merge_text_dictionaries(local_dictionary):
    """Text codes (executor.GpuTextRank) are local to a DataNode: every rank
    ranks its own strings. This all-gathers the ranks' dictionaries (row
    lengths and bytes, through allgather_variable) and builds the global
    sorted distinct list on the host — dictionary-sized numpy / Python, like
    merge_group_partials. local_dictionary: the rank's distinct strings in
    code order, a GpuText (TextRank.dictionary()) or a list of bytes.
    Returns (global_dictionary, remap): the global list of bytes in C
    collation order (Python's bytes order: memcmp, then the shorter first)
    and an int64 numpy array with remap[local code] = global code. After
    codes = remap[codes] the text-keyed partials go through
    merge_group_partials / merge_sorted_partials unchanged. With one rank
    or no process group it is the identity."""
    import numpy as np
    rows = local_dictionary.to_list() if hasattr(local_dictionary, "to_list") \
        else [None if r is None else bytes(r) for r in local_dictionary]
    if any(r is None for r in rows):
        raise OtbxError(3, "text dictionary: a dictionary holds no NULL")
    if not is_dist() or dist.get_world_size() == 1:
        return rows, np.arange(len(rows), dtype=np.int64)
    dev = "cuda" if torch.cuda.is_available() and \
        dist.get_backend() == "nccl" else "cpu"
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    raw = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    glens = allgather_variable(torch.from_numpy(lens).to(dev)).cpu().numpy()
    graw = allgather_variable(torch.from_numpy(raw).to(dev)).cpu().numpy() \
        .tobytes()
    ends = np.cumsum(glens)
    merged = sorted({graw[e - l:e] for e, l in zip(ends.tolist(),
                                                   glens.tolist())})
    code = {s: i for i, s in enumerate(merged)}
    remap = np.fromiter((code[r] for r in rows), dtype=np.int64,
                        count=len(rows))
    return merged, remap


def finalize_q1(rows):
    return q1_finalize(rows)


def all_to_all_variable(t, send_counts):
    """All-to-all with per-rank variable segment lengths: rank r sends
    t[offsets[r]:offsets[r]+send_counts[r]] to rank r and receives the
    concatenation of every rank's segment addressed to it. The RCCL
    all-to-allv of the repartition exchange (FN-transport
    semantics of forward/*). nccl: dist.all_to_all_single with splits;
    gloo (CPU tests): emulated via all-gather + slicing (gloo has no
    all-to-all)."""
    if not is_dist() or dist.get_world_size() == 1:
        return t
    world = dist.get_world_size()
    assert len(send_counts) == world
    if dist.get_backend() == "nccl":
        sc = torch.tensor(send_counts, dtype=torch.int64, device=t.device)
        rc = torch.empty_like(sc)
        dist.all_to_all_single(rc, sc)
        recv_counts = [int(x) for x in rc.cpu()]
        out = torch.empty(sum(recv_counts), dtype=t.dtype, device=t.device)
        dist.all_to_all_single(out, t, output_split_sizes=recv_counts,
                               input_split_sizes=list(send_counts))
        return out
    # gloo emulation: gather everything + counts, slice my segments
    if t.is_cuda:
        t = t.cpu()
    rank = dist.get_rank()
    cnts = torch.tensor(send_counts, dtype=torch.int64)
    all_cnts = [torch.empty_like(cnts) for _ in range(world)]
    dist.all_gather(all_cnts, cnts)
    alldata = allgather_variable(t)
    out = []
    pos = 0
    for src in range(world):
        c = [int(x) for x in all_cnts[src]]
        seg_start = pos + sum(c[:rank])
        out.append(alldata[seg_start: seg_start + c[rank]])
        pos += sum(c)
    return torch.cat(out) if out else t[:0]


def exchange_rows(keys, payload_tensors):
    """Full repartition exchange: GPU partition by key % world, native
    gathers, all-to-allv of every column. Returns (keys', payloads') — the
    rows this rank owns after redistribution."""
    from . import executor as ex
    perm, counts = ex.partition_by_key(keys)
    out_keys = all_to_all_variable(ex.gather(keys, perm), counts)
    out_payloads = [all_to_all_variable(ex.gather(p, perm), counts)
                    for p in payload_tensors]
    return out_keys, out_payloads

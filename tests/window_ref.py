"""Reference results for the WindowAgg operator (a helper, not a test).

A spec is sort_ref's: a list of keys (col, nulls, desc, nulls_first), the
first npart of them the PARTITION BY columns, the rest the ORDER BY columns.
vals is a float64 array (or None), val_null a uint8/bool array (or None).
Both functions return a dict of numpy arrays INDEXED BY SORTED POSITION:
    perm, row_number, rank, dense_rank, count_star, part_rows   (int64)
and, when vals is given, count_v (int64), sum_v (float64, 0.0 under NULL),
sum_isnull (uint8).

loop_window: a literal row-by-row restatement of the reference executor:
             window_row_number / rank_up / window_rank / window_dense_rank
             (utils/adt/windowfuncs.c:48-133), are_peers
             (nodeWindowAgg.c:2960) over the literal ApplySortComparator of
             sort_ref, the default frame RANGE UNBOUNDED PRECEDING .. CURRENT
             ROW (row_is_in_frame, nodeWindowAgg.c:1472: through the last
             peer) and a left-to-right float8pl. For small n.
ref_window:  vectorised numpy: sort_ref.ref_perm, norm_key for the
             boundaries, one np.cumsum per partition. For large n.
             test_window_host.py pins ref_window == loop_window.
"""
import numpy as np

from sort_ref import (_apply_sort_comparator, _float8_cmp_internal, _int_cmp,
                      cmp_perm, norm_key, ref_perm)


def _nrows(spec, vals, n):
    if spec:
        return len(spec[0][0])
    if vals is not None:
        return len(vals)
    return int(n)


def loop_window(spec, npart, vals=None, val_null=None, n=None):
    spec = list(spec)
    n = _nrows(spec, vals, n)
    perm = cmp_perm(spec) if spec else np.arange(n, dtype=np.int64)
    cols = []
    for col, nulls, desc, nf in spec:
        col = np.asarray(col)
        cmp = _float8_cmp_internal if col.dtype == np.float64 else _int_cmp
        nl = [False] * n if nulls is None else \
            [bool(x) for x in np.asarray(nulls).tolist()]
        cols.append((col.tolist(), nl, bool(desc), bool(nf), cmp))

    def equal(i, j, lo, hi):
        for vv, nl, desc, nf, cmp in cols[lo:hi]:
            if _apply_sort_comparator(vv[i], nl[i], vv[j], nl[j], desc, nf,
                                      cmp) != 0:
                return False
        return True

    rows = perm.tolist()
    nk = len(cols)
    v = None if vals is None else np.asarray(vals, dtype=np.float64)
    vn = None if val_null is None else np.asarray(val_null).astype(bool)
    out = {k: np.zeros(n, dtype=np.int64) for k in
           ("row_number", "rank", "dense_rank", "count_star", "part_rows")}
    if v is not None:
        out["count_v"] = np.zeros(n, dtype=np.int64)
        out["sum_v"] = np.zeros(n, dtype=np.float64)
        out["sum_isnull"] = np.zeros(n, dtype=np.uint8)
    start = 0
    while start < n:
        end = start + 1          # one partition: [start, end)
        while end < n and equal(rows[end - 1], rows[end], 0, npart):
            end += 1
        rank = dense = 0
        for j in range(start, end):
            curpos = j - start
            # rank_up: the first row, or not a peer of the previous one
            up = curpos == 0 or not equal(rows[j - 1], rows[j], npart, nk)
            if up:
                rank = curpos + 1
                dense += 1
            out["row_number"][j] = curpos + 1
            out["rank"][j] = rank
            out["dense_rank"][j] = dense
            out["part_rows"][j] = end - start
            # frame: partition start through the last peer of row j
            fe = j
            while fe + 1 < end and equal(rows[j], rows[fe + 1], npart, nk):
                fe += 1
            out["count_star"][j] = fe - start + 1
            if v is not None:
                cnt, acc = 0, None
                for q in range(start, fe + 1):
                    r = rows[q]
                    if vn is not None and vn[r]:
                        continue
                    cnt += 1
                    acc = v[r] if acc is None else acc + v[r]   # float8pl
                out["count_v"][j] = cnt
                out["sum_isnull"][j] = 1 if acc is None else 0
                out["sum_v"][j] = 0.0 if acc is None else acc
        start = end
    out["perm"] = perm
    return out


def boundaries(spec, npart, perm):
    """(partition-start, peer-start) bool arrays over sorted positions."""
    n = len(perm)
    ps = np.zeros(n, dtype=bool)
    gs = np.zeros(n, dtype=bool)
    if n:
        ps[0] = gs[0] = True
    for c, (col, nulls, desc, nf) in enumerate(spec):
        nb, k = norm_key(col, nulls, desc, nf)
        nb, k = nb[perm], k[perm]
        d = (nb[1:] != nb[:-1]) | (k[1:] != k[:-1])
        if c < npart:
            ps[1:] |= d
        gs[1:] |= d
    gs |= ps
    return ps, gs


def ref_window(spec, npart, vals=None, val_null=None, n=None):
    spec = list(spec)
    n = _nrows(spec, vals, n)
    perm = ref_perm(spec) if spec else np.arange(n, dtype=np.int64)
    ps, gs = boundaries(spec, npart, perm)
    pos = np.arange(n, dtype=np.int64)
    pstart = np.maximum.accumulate(np.where(ps, pos, 0))
    gstart = np.maximum.accumulate(np.where(gs, pos, 0))
    # next start strictly after j (n if none)
    nxt_g = np.full(n + 1, n, dtype=np.int64)
    nxt_p = np.full(n + 1, n, dtype=np.int64)
    nxt_g[:n] = np.where(gs, pos, n)
    nxt_p[:n] = np.where(ps, pos, n)
    nxt_g = np.minimum.accumulate(nxt_g[::-1])[::-1][1:]
    nxt_p = np.minimum.accumulate(nxt_p[::-1])[::-1][1:]
    fend = nxt_g - 1
    cg = np.cumsum(gs.astype(np.int64))
    out = {
        "perm": perm,
        "row_number": pos - pstart + 1,
        "rank": gstart - pstart + 1,
        "dense_rank": cg - cg[pstart] + 1 if n else cg,
        "count_star": fend - pstart + 1,
        "part_rows": nxt_p - pstart,
    }
    if vals is not None:
        v = np.asarray(vals, dtype=np.float64)[perm]
        nn = np.ones(n, dtype=bool) if val_null is None else \
            ~np.asarray(val_null).astype(bool)[perm]
        cnt = np.zeros(n, dtype=np.int64)
        run = np.zeros(n, dtype=np.float64)
        starts = np.flatnonzero(ps)
        ends = np.append(starts[1:], n)
        for a, b in zip(starts.tolist(), ends.tolist()):
            m = nn[a:b]
            cnt[a:b] = np.cumsum(m)
            # left-to-right over the non-NULL values only, as float8pl sees
            # them (a NULL neither adds 0.0 nor starts the sum)
            s = np.zeros(b - a, dtype=np.float64)
            idx = np.flatnonzero(m)
            if len(idx):
                with np.errstate(invalid="ignore", over="ignore"):
                    cs = np.cumsum(v[a:b][idx])   # Inf - Inf = NaN is data
                # running value at each row = cumsum at the last non-NULL
                # row at or before it
                last = np.cumsum(m) - 1
                has = last >= 0
                s[has] = cs[last[has]]
            run[a:b] = s
        if n:
            out["count_v"] = cnt[fend]
            isnull = out["count_v"] == 0
            out["sum_isnull"] = isnull.astype(np.uint8)
            out["sum_v"] = np.where(isnull, 0.0, run[fend])
        else:
            out["count_v"] = cnt
            out["sum_isnull"] = np.zeros(0, dtype=np.uint8)
            out["sum_v"] = run
    return out


def frame_terms(res, vals, val_null=None):
    """For the tolerance test: (partition start, frame end) per sorted
    position plus the values / non-NULL mask in sorted order."""
    perm = res["perm"]
    n = len(perm)
    pos = np.arange(n, dtype=np.int64)
    pstart = pos - res["row_number"] + 1
    fend = pstart + res["count_star"] - 1
    v = np.asarray(vals, dtype=np.float64)[perm]
    nn = np.ones(n, dtype=bool) if val_null is None else \
        ~np.asarray(val_null).astype(bool)[perm]
    return pstart, fend, v, nn

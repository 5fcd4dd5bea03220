"""Reference results for the window-frame operator (a helper, not a test).

A spec is sort_ref's key list, the first npart keys the PARTITION BY columns.
A frame is (units, start, end): units "rows" or "range", a bound None
(unbounded), 0 (CURRENT ROW) or, under "rows", a signed offset. A call is
    ("ntile", buckets)
    ("lag" | "lead", col, nulls, offset, default)      default None = NULL
    ("first_value" | "last_value", col, nulls)
    ("nth_value", col, nulls, n)
    ("count_star",) | ("count", col, nulls)
    ("sum" | "min" | "max", col, nulls)
with col a numpy array of dtype int64, float64, int32 or uint8 and nulls a
uint8 array or None. Both functions return {"perm": ..., "calls": [...]},
one tuple per call INDEXED BY SORTED POSITION:
    ntile            (int32,  None)
    counts           (int64,  None)
    sum over int64   (lo uint64, hi int64, nulls uint8): the int128 sum
    everything else  (values in the result type, nulls uint8); 0 under NULL

loop_frame: a literal row loop restating the reference: window_ntile
            (windowfuncs.c:231), leadlag_common (:306), WinGetFuncArgInFrame
            (nodeWindowAgg.c:3368), the frame bounds of row_is_in_frame /
            update_frameheadpos (:1472-1560), and every aggregate restarted
            per frame and advanced left to right (eval_windowaggregates
            :919) with float8pl / float8larger / float8smaller. Small n.
ref_frame:  vectorised numpy for large n: prefix differences for the counts
            and integer sums, a sparse table of (key, position) for MIN / MAX.
            Float sums are added left to right per frame for bounded frames
            of at most REF_LOOP_WIDTH rows and with one cumsum per partition
            or peer group otherwise — exact on integer-valued doubles;
            tolerance tests bound the rest.
"""
import numpy as np

from sort_ref import _float8_cmp_internal
from window_ref import loop_window, ref_window

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
REF_LOOP_WIDTH = 64


def _sat(v):
    return max(INT64_MIN, min(INT64_MAX, v))


def _n_of(spec, calls, n):
    if spec:
        return len(spec[0][0])
    for c in calls:
        if len(c) > 1 and c[0] != "ntile" and c[1] is not None:
            return len(c[1])
    return int(n)


def _bounds(w, n):
    pos = np.arange(n, dtype=np.int64)
    ps = pos - w["row_number"] + 1
    pe = ps + w["part_rows"] - 1
    gs = ps + w["rank"] - 1
    ge = ps + w["count_star"] - 1
    return ps, pe, gs, ge


def frame_bounds(frame, ps, pe, gs, ge):
    """(lo, hi) int64 arrays per sorted position; empty where lo > hi"""
    units, start, end = frame
    n = len(ps)
    pos = np.arange(n, dtype=np.int64)
    if units == "rows":
        if start is None:
            lo = ps.copy()
        else:
            lo = np.maximum(ps, np.array([_sat(int(j) + start)
                                          for j in range(n)], dtype=np.int64)
                            if abs(start) > 2**61 else pos + start)
        if end is None:
            hi = pe.copy()
        else:
            hi = np.minimum(pe, np.array([_sat(int(j) + end)
                                          for j in range(n)], dtype=np.int64)
                            if abs(end) > 2**61 else pos + end)
    else:
        assert start in (None, 0) and end in (None, 0)
        lo = ps.copy() if start is None else gs.copy()
        hi = pe.copy() if end is None else ge.copy()
    return lo, hi


def _out_dtype(func, col):
    if func == "sum":
        return np.float64 if col.dtype == np.float64 else np.int64
    return col.dtype


def _split128(v):
    return v & (2**64 - 1), v >> 64


def _ntile_loop(total, nb):
    """window_ntile over one partition of `total` rows"""
    out = []
    ntile, rows_per_bucket, remainder = 1, 0, 0
    boundary = total // nb
    if boundary <= 0:
        boundary = 1
    else:
        remainder = total % nb
        if remainder != 0:
            boundary += 1
    for _ in range(total):
        rows_per_bucket += 1
        if boundary < rows_per_bucket:
            if remainder != 0 and ntile == remainder:
                remainder = 0
                boundary -= 1
            ntile += 1
            rows_per_bucket = 1
        out.append(ntile)
    return out


def ntile_closed(total, nb, i):
    """the closed form the kernel evaluates for 0-based row i"""
    q, r = total // nb, total % nb
    if q == 0:
        return i + 1
    if i < r * (q + 1):
        return i // (q + 1) + 1
    return r + (i - r * (q + 1)) // q + 1


def loop_frame(spec, npart, frame, calls, n=None):
    spec = list(spec)
    n = _n_of(spec, calls, n)
    w = loop_window(spec, npart, n=n)
    perm = w["perm"]
    ps, pe, gs, ge = _bounds(w, n)
    lo, hi = frame_bounds(frame, ps, pe, gs, ge)
    rows = perm.tolist()
    res = []
    for c in calls:
        func = c[0]
        if func == "ntile":
            out = np.zeros(n, dtype=np.int32)
            j = 0
            while j < n:
                t = int(pe[j] - ps[j] + 1)
                out[j:j + t] = _ntile_loop(t, int(c[1]))
                j += t
            res.append((out, None))
            continue
        if func == "count_star":
            res.append((np.array([max(0, int(h) - int(l) + 1)
                                  for l, h in zip(lo, hi)], dtype=np.int64),
                        None))
            continue
        col = None if c[1] is None else np.asarray(c[1])
        nl = None if len(c) < 3 or c[2] is None else \
            np.asarray(c[2]).astype(bool)

        def isnull(q):
            return nl is not None and bool(nl[rows[q]])

        if func == "count":
            res.append((np.array(
                [sum(0 if isnull(q) else 1 for q in range(int(l), int(h) + 1))
                 for l, h in zip(lo, hi)], dtype=np.int64), None))
            continue
        out = np.zeros(n, dtype=_out_dtype(func, col))
        onull = np.zeros(n, dtype=np.uint8)
        ohi = np.zeros(n, dtype=np.int64)
        is_f = col.dtype == np.float64
        for j in range(n):
            l, h = int(lo[j]), int(hi[j])
            if func in ("lag", "lead"):
                off, default = int(c[3]), c[4]
                src = _sat(j - off) if func == "lag" else _sat(j + off)
                if ps[j] <= src <= pe[j]:
                    if isnull(src):
                        onull[j] = 1
                    else:
                        out[j] = col[rows[src]]
                elif default is None:
                    onull[j] = 1
                else:
                    out[j] = np.array(default).astype(col.dtype)
            elif func in ("first_value", "last_value", "nth_value"):
                src = l if func == "first_value" else \
                    (h if func == "last_value" else _sat(l + int(c[3]) - 1))
                if l > h or src > h or isnull(src):
                    onull[j] = 1
                else:
                    out[j] = col[rows[src]]
            else:
                state = None        # strict: first non-NULL is the state
                for q in range(l, h + 1):
                    if isnull(q):
                        continue
                    r = rows[q]
                    if func == "sum":
                        v = float(col[r]) if is_f else int(col[r])
                        state = v if state is None else state + v
                    elif state is None:
                        state = r
                    elif is_f:
                        cmpv = _float8_cmp_internal(float(col[state]),
                                                    float(col[r]))
                        # float8larger / float8smaller return arg2 on a tie
                        keep = cmpv > 0 if func == "max" else cmpv < 0
                        state = state if keep else r
                    else:
                        a, b = int(col[state]), int(col[r])
                        keep = a > b if func == "max" else a < b
                        state = state if keep else r
                if state is None:
                    onull[j] = 1
                elif func != "sum":
                    out[j] = col[state]
                elif is_f:
                    out[j] = state
                elif col.dtype == np.int64:
                    l64, h64 = _split128(state)
                    out[j] = np.array(l64, dtype=np.uint64).view(np.int64)
                    ohi[j] = h64
                else:
                    out[j] = state
        if func == "sum" and col.dtype == np.int64:
            res.append((out.view(np.uint64), ohi, onull))
        else:
            res.append((out, onull))
    return {"perm": perm, "calls": res}


def _cmp_key(v):
    """float64 array -> uint64 key that orders as float8_cmp_internal and
    maps -0.0 / +0.0 and all NaNs to one key each"""
    v = np.where(np.isnan(v), np.nan, v) + 0.0      # canonical NaN, +0.0
    b = v.view(np.uint64)
    neg = (b >> np.uint64(63)) != 0
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def _minmax(func, key, nn, lo, hi):
    """index of the chosen row per frame (-1: none). key: uint64 order key;
    the later row wins a tie. Per frame argmin / argmax by a sparse table."""
    n = len(key)
    big = np.uint64(2**64 - 1)
    # fold "later row wins" and NULLs into one comparable pair (k, pos)
    k = key.copy()
    if func == "min":
        k = big - k                  # search a maximum in both cases
    k = np.where(nn, k, np.uint64(0))
    idx = np.where(nn, np.arange(n, dtype=np.int64), -1)
    # level tables: best over [i, i + 2^l)
    ks, ix = [k], [idx]
    span = 1
    while span * 2 <= n:
        pk, pi = ks[-1], ix[-1]
        m = n - 2 * span + 1
        a_k, a_i = pk[:m], pi[:m]
        b_k, b_i = pk[span:span + m], pi[span:span + m]
        # right half wins ties (later row), unless it is empty (-1)
        take_b = (b_i >= 0) & ((a_i < 0) | (b_k >= a_k))
        ks.append(np.where(take_b, b_k, a_k))
        ix.append(np.where(take_b, b_i, a_i))
        span *= 2
    out = np.full(n, -1, dtype=np.int64)
    ok = lo <= hi
    if not ok.any():
        return out
    l, h = lo[ok], hi[ok]
    ln = h - l + 1
    lvl = np.floor(np.log2(ln)).astype(np.int64)
    res_i = np.full(len(l), -1, dtype=np.int64)
    for v in np.unique(lvl).tolist():
        m = lvl == v
        sp = 1 << v
        a = l[m]
        b = h[m] - sp + 1
        a_k, a_i = ks[v][a], ix[v][a]
        b_k, b_i = ks[v][b], ix[v][b]
        # overlapping halves: the later INDEX wins a tie
        take_b = (b_i >= 0) & ((a_i < 0) | (b_k > a_k) |
                               ((b_k == a_k) & (b_i >= a_i)))
        res_i[m] = np.where(take_b, b_i, a_i)
    out[ok] = res_i
    return out


def ref_frame(spec, npart, frame, calls, n=None):
    spec = list(spec)
    n = _n_of(spec, calls, n)
    w = ref_window(spec, npart, n=n)
    perm = w["perm"]
    ps, pe, gs, ge = _bounds(w, n)
    lo, hi = frame_bounds(frame, ps, pe, gs, ge)
    ok = lo <= hi
    lc = np.clip(lo, 0, max(n - 1, 0))
    hc = np.clip(hi, 0, max(n - 1, 0))
    pos = np.arange(n, dtype=np.int64)
    res = []
    for c in calls:
        func = c[0]
        if func == "ntile":
            t, i, nb = pe - ps + 1, pos - ps, int(c[1])
            q, r = t // nb, t % nb
            qq = np.maximum(q, 1)
            out = np.where(q == 0, i + 1,
                           np.where(i < r * (q + 1), i // (q + 1) + 1,
                                    r + (i - r * (q + 1)) // qq + 1))
            res.append((out.astype(np.int32), None))
            continue
        if func == "count_star":
            res.append((np.where(ok, hc - lc + 1, 0).astype(np.int64), None))
            continue
        col = None if c[1] is None else np.asarray(c[1])
        nn = np.ones(n, dtype=bool) if len(c) < 3 or c[2] is None else \
            ~np.asarray(c[2]).astype(bool)[perm]
        cn = np.concatenate([[0], np.cumsum(nn.astype(np.int64))])
        cnt = np.where(ok, cn[hc + 1] - cn[lc], 0) if n else \
            np.zeros(0, dtype=np.int64)
        if func == "count":
            res.append((cnt.astype(np.int64), None))
            continue
        sv = col[perm] if n else col[:0]
        if func in ("lag", "lead", "first_value", "last_value", "nth_value"):
            if func in ("lag", "lead"):
                off, default = int(c[3]), c[4]
                src = pos - off if func == "lag" else pos + off
                have = (src >= ps) & (src <= pe)
            else:
                default = None
                src = lo if func == "first_value" else \
                    (hi if func == "last_value" else
                     np.array([_sat(int(x) + int(c[3]) - 1) for x in lo],
                              dtype=np.int64))
                have = ok & (src <= hi)
            s = np.clip(src, 0, max(n - 1, 0))
            out = np.zeros(n, dtype=col.dtype)
            onull = np.ones(n, dtype=np.uint8)
            if n:
                good = have & nn[s]
                out[good] = sv[s[good]]
                onull[good] = 0
                if default is not None:
                    out[~have] = np.array(default).astype(col.dtype)
                    onull[~have] = 0
            res.append((out, onull))
            continue
        onull = (cnt == 0).astype(np.uint8)
        if func in ("min", "max"):
            key = _cmp_key(sv.astype(np.float64)) \
                if col.dtype == np.float64 else \
                (sv.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63))
            pick = _minmax(func, key, nn, lc, np.where(ok, hc, lc - 1)) \
                if n else np.zeros(0, dtype=np.int64)
            out = np.zeros(n, dtype=col.dtype)
            good = pick >= 0
            out[good] = sv[pick[good]]
            res.append((out, onull))
            continue
        # sum
        if col.dtype != np.float64:
            vals = [int(x) if m else 0 for x, m in zip(sv.tolist(),
                                                       nn.tolist())]
            pre = [0]
            for x in vals:
                pre.append(pre[-1] + x)
            tot = [pre[h + 1] - pre[l] if o else 0
                   for l, h, o in zip(lc.tolist(), hc.tolist(), ok.tolist())]
            tot = [0 if z else t for t, z in zip(tot, onull.tolist())]
            if col.dtype == np.int64:
                l64 = np.array([_split128(t)[0] for t in tot], dtype=np.uint64)
                h64 = np.array([_split128(t)[1] for t in tot], dtype=np.int64)
                res.append((l64, h64, onull))
            else:
                res.append((np.array(tot, dtype=np.int64), onull))
            continue
        out = np.zeros(n, dtype=np.float64)
        units, start, end = frame
        bounded = units == "rows" and start is not None and end is not None
        v = np.where(nn, sv, 0.0)
        if bounded and end - start + 1 <= REF_LOOP_WIDTH:
            # left to right over the frame's non-NULL values: the first one
            # is the state, the others are added in position order
            acc = np.zeros(n, dtype=np.float64)
            has = np.zeros(n, dtype=bool)
            with np.errstate(invalid="ignore", over="ignore"):
                for d in range(start, end + 1):
                    q = pos + d
                    m = (q >= lo) & (q <= hi)
                    qc = np.clip(q, 0, max(n - 1, 0))
                    m &= nn[qc]
                    x = sv[qc]
                    acc = np.where(m, np.where(has, acc + x, x), acc)
                    has |= m
            out = np.where(has, acc, 0.0)
        elif n:
            # one left-to-right cumsum per frame start that occurs: exact
            # wherever every order is (integer-valued doubles)
            for a in np.unique(lc[ok]).tolist():
                m = ok & (lc == a)
                b = int(hc[m].max())
                idx = np.flatnonzero(nn[a:b + 1])
                if not len(idx):
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    cs = np.cumsum(sv[a:b + 1][idx])
                last = np.cumsum(nn[a:b + 1]) - 1
                hh = hc[m] - a
                o = np.zeros(m.sum(), dtype=np.float64)
                g = last[hh] >= 0
                o[g] = cs[last[hh][g]]
                out[m] = o
            out = np.where(onull == 1, 0.0, out)
        res.append((out, onull))
    return {"perm": perm, "calls": res}


def frame_terms(spec, npart, frame, col, nulls=None):
    """For tolerance tests: (lo, hi) per sorted position plus the values and
    the non-NULL mask in sorted order."""
    n = len(col)
    w = ref_window(list(spec), npart, n=n)
    ps, pe, gs, ge = _bounds(w, n)
    lo, hi = frame_bounds(frame, ps, pe, gs, ge)
    perm = w["perm"]
    nn = np.ones(n, dtype=bool) if nulls is None else \
        ~np.asarray(nulls).astype(bool)[perm]
    return lo, hi, np.asarray(col)[perm], nn


# ---- the golden cases of tests/golden/window_cases.json ----

def golden_load():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "window_cases.json")
    with open(path, encoding="utf-8") as f:
        return json.load(f)


def golden_inputs(gold, case):
    """(columns dict of int32 arrays in input order, spec, npart, frame,
    calls) of one golden case"""
    rows = list(gold["tables"][case["rows"]])
    if case["presort"]:
        rows.sort(key=lambda r: tuple(r[k] for k in case["presort"]))
    cols = {k: np.array([r[k] for r in rows], dtype=np.int32)
            for k in rows[0]}
    keys = case["partition"] + case["order"]
    spec = [(cols[k], None, False, False) for k in keys]
    calls = []
    for func, col, arg, default in case["calls"]:
        if func == "ntile":
            calls.append(("ntile", arg))
        elif func in ("lag", "lead"):
            calls.append((func, cols[col], None, arg, default))
        elif func == "nth_value":
            calls.append((func, cols[col], None, arg))
        else:
            calls.append((func, cols[col], None))
    return cols, spec, len(case["partition"]), tuple(case["frame"]), calls


def golden_rows(case, cols, perm, results):
    """the query's output rows as a sorted multiset: one (value or None) per
    call, then the shown columns"""
    perm = np.asarray(perm)
    out = []
    for j in range(len(perm)):
        row = []
        for r in results:
            v, nl = r[0], r[-1] if len(r) > 1 else None
            row.append(None if nl is not None and nl[j] else int(v[j]))
        row += [int(cols[k][perm[j]]) for k in case["shown"]]
        out.append(row)
    key = lambda r: [(x is None, 0 if x is None else x) for x in r]  # noqa
    return sorted(out, key=key), sorted(case["expected"], key=key)

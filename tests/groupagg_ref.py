"""Reference results for the GroupAggregate operator (a helper, not a test).

A spec is sort_ref's: a list of GROUP BY keys (col, nulls, desc, nulls_first).
aggs is a list of (func, col, nulls) with func one of "count_star", "count",
"sum", "min", "max", col a numpy array of dtype int64 / float64 / int32 /
uint8 (None for count_star) and nulls a uint8/bool array or None. perm is the
position order (None: the stable sort of the spec, identity without keys).

Both functions return
    {"ngroups": int, "first_row": int64[ngroups], "perm": int64[n],
     "aggs": [{"val", "null", "hi", "abs", "rows"}, ...]}
val:  counts int64; SUM(F64) float64; SUM(I32/U8) int64; SUM(I64) the low
      word as uint64 with "hi" the signed high word (int64); MIN/MAX the
      input dtype, floats with the chosen row's bit pattern. 0 under a NULL.
null: uint8, 1 where the group held no non-NULL input (None for counts).
abs / rows (SUM(F64) only): the group's sum|x| and its non-NULL row count,
      for the summation bound.

loop_groupagg: a literal row loop over the reference's transition functions,
               left to right: int8inc / int8inc_any, float8pl, int4_sum and
               int8_sum (Python ints), int8larger / int8smaller, and
               float8larger / float8smaller over float8_cmp_internal (on a
               tie the second argument, the later row, is returned). Group
               boundaries by the literal ApplySortComparator. For small n.
ref_groupagg:  vectorised numpy over the normalised keys. SUM(F64) is a
               left-to-right cumsum per group up to SUM_LOOP_GROUPS groups;
               above that np.add.reduceat, whose association order is
               numpy's own: exact for integer-valued data only.
               test_groupagg_host.py pins ref_groupagg == loop_groupagg.
"""
import numpy as np

from sort_ref import (_apply_sort_comparator, _float8_cmp_internal, _int_cmp,
                      norm_key, ref_perm)

SUM_LOOP_GROUPS = 20000
_MASK64 = (1 << 64) - 1


def _nrows(spec, aggs, perm, n):
    if spec:
        return len(spec[0][0])
    for _, col, _ in aggs:
        if col is not None:
            return len(col)
    if perm is not None:
        return len(perm)
    return int(n)


def _norm_aggs(aggs):
    out = []
    for a in aggs:
        a = tuple(a)
        out.append((a[0], a[1] if len(a) > 1 else None,
                    a[2] if len(a) > 2 else None))
    return out


def _empty(func, col):
    """One aggregate's output arrays for zero groups."""
    if func in ("count_star", "count"):
        return {"val": np.zeros(0, np.int64), "null": None}
    if func == "sum":
        dt = np.float64 if col.dtype == np.float64 else \
            (np.uint64 if col.dtype == np.int64 else np.int64)
    else:
        dt = col.dtype
    r = {"val": np.zeros(0, dt), "null": np.zeros(0, np.uint8)}
    if func == "sum" and col.dtype == np.int64:
        r["hi"] = np.zeros(0, np.int64)
    if func == "sum" and col.dtype == np.float64:
        r["abs"] = np.zeros(0, np.float64)
        r["rows"] = np.zeros(0, np.int64)
    return r


def _plain_empty(aggs):
    """AGG_PLAIN over no rows: one group, counts 0, the rest NULL."""
    res = []
    for func, col, _ in aggs:
        e = _empty(func, col)
        r = {}
        for k, v in e.items():
            if v is None:
                r[k] = None
            elif k == "null":
                r[k] = np.ones(1, np.uint8)
            else:
                r[k] = np.zeros(1, v.dtype)
        res.append(r)
    return {"ngroups": 1, "first_row": np.array([-1], dtype=np.int64),
            "perm": np.zeros(0, np.int64), "aggs": res}


def _split128(total):
    lo = total & _MASK64
    hi = (total >> 64)
    return lo, hi


def loop_groupagg(spec, aggs, perm=None, n=None):
    spec, aggs = list(spec), _norm_aggs(aggs)
    n = _nrows(spec, aggs, perm, n)
    if perm is None:
        perm = ref_perm(spec) if spec else np.arange(n, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    if n == 0:
        if not spec:
            return _plain_empty(aggs)
        return {"ngroups": 0, "first_row": np.zeros(0, np.int64),
                "perm": perm, "aggs": [_empty(f, c) for f, c, _ in aggs]}
    cols = []
    for col, nulls, desc, nf in spec:
        col = np.asarray(col)
        cmp = _float8_cmp_internal if col.dtype == np.float64 else _int_cmp
        nl = [False] * n if nulls is None else \
            [bool(x) for x in np.asarray(nulls).tolist()]
        cols.append((col.tolist(), nl, bool(desc), bool(nf), cmp))

    def equal(i, j):
        for vv, nl, desc, nf, cmp in cols:
            if _apply_sort_comparator(vv[i], nl[i], vv[j], nl[j], desc, nf,
                                      cmp) != 0:
                return False
        return True

    rows = perm.tolist()
    first = []
    # per aggregate: list of final states
    states = [[] for _ in aggs]
    extra = [[] for _ in aggs]      # (abs, rows) for SUM(F64)
    prepared = []
    for func, col, nulls in aggs:
        vals = None if col is None else np.asarray(col).tolist()
        nl = None if nulls is None else \
            [bool(x) for x in np.asarray(nulls).tolist()]
        isf = col is not None and np.asarray(col).dtype == np.float64
        prepared.append((func, vals, nl, isf))
    cur = None
    for j, r in enumerate(rows):
        if j == 0 or not equal(rows[j - 1], r):
            if cur is not None:
                for a in range(len(aggs)):
                    states[a].append(cur[a])
                    extra[a].append(ext[a])
            first.append(r)
            cur = [0 if p[0] in ("count_star", "count") else None
                   for p in prepared]
            ext = [[0.0, 0] for _ in prepared]
        for a, (func, vals, nl, isf) in enumerate(prepared):
            if func == "count_star":
                cur[a] += 1                              # int8inc
                continue
            if nl is not None and nl[r]:
                continue                                 # strict: skip NULL
            if func == "count":
                cur[a] += 1                              # int8inc_any
                continue
            v = vals[r]
            if func == "sum":
                if isf:
                    ext[a][0] += abs(v)
                    ext[a][1] += 1
                cur[a] = v if cur[a] is None else cur[a] + v
                continue
            # min / max: the state is the chosen ROW (its bits are the result)
            if cur[a] is None:
                cur[a] = r
                continue
            s = vals[cur[a]]
            c = _float8_cmp_internal(s, v) if isf else _int_cmp(s, v)
            if func == "max":
                cur[a] = cur[a] if c > 0 else r          # float8larger
            else:
                cur[a] = cur[a] if c < 0 else r          # float8smaller
    for a in range(len(aggs)):
        states[a].append(cur[a])
        extra[a].append(ext[a])
    ng = len(first)
    res = []
    for a, (func, col, nulls) in enumerate(aggs):
        st = states[a]
        if func in ("count_star", "count"):
            res.append({"val": np.array(st, dtype=np.int64), "null": None})
            continue
        col = np.asarray(col)
        isnull = np.array([1 if s is None else 0 for s in st], dtype=np.uint8)
        if func == "sum" and col.dtype == np.float64:
            val = np.array([0.0 if s is None else s for s in st],
                           dtype=np.float64)
            res.append({"val": val, "null": isnull,
                        "abs": np.array([e[0] for e in extra[a]]),
                        "rows": np.array([e[1] for e in extra[a]],
                                         dtype=np.int64)})
        elif func == "sum" and col.dtype == np.int64:
            parts = [_split128(0 if s is None else s) for s in st]
            res.append({"val": np.array([p[0] for p in parts],
                                        dtype=np.uint64),
                        "hi": np.array([p[1] for p in parts], dtype=np.int64),
                        "null": isnull})
        elif func == "sum":
            res.append({"val": np.array([0 if s is None else s for s in st],
                                        dtype=np.int64), "null": isnull})
        else:
            val = np.zeros(ng, dtype=col.dtype)
            for g, s in enumerate(st):
                if s is not None:
                    val[g] = col[s]      # element copy: bits preserved
            res.append({"val": val, "null": isnull})
    return {"ngroups": ng, "first_row": np.array(first, dtype=np.int64),
            "perm": perm, "aggs": res}


def group_starts(spec, perm):
    """bool array over positions: True where a group starts."""
    n = len(perm)
    st = np.zeros(n, dtype=bool)
    if n:
        st[0] = True
    for col, nulls, desc, nf in spec:
        nb, k = norm_key(col, nulls, desc, nf)
        nb, k = nb[perm], k[perm]
        st[1:] |= (nb[1:] != nb[:-1]) | (k[1:] != k[:-1])
    return st


def ref_groupagg(spec, aggs, perm=None, n=None):
    spec, aggs = list(spec), _norm_aggs(aggs)
    n = _nrows(spec, aggs, perm, n)
    if perm is None:
        perm = ref_perm(spec) if spec else np.arange(n, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    if n == 0:
        if not spec:
            return _plain_empty(aggs)
        return {"ngroups": 0, "first_row": np.zeros(0, np.int64),
                "perm": perm, "aggs": [_empty(f, c) for f, c, _ in aggs]}
    st = group_starts(spec, perm)
    starts = np.flatnonzero(st)
    ends = np.append(starts[1:], n)
    ng = len(starts)
    pos = np.arange(n, dtype=np.int64)
    res = []
    for func, col, nulls in aggs:
        nn = np.ones(n, dtype=bool) if nulls is None else \
            ~np.asarray(nulls).astype(bool)[perm]
        if func == "count_star":
            res.append({"val": (ends - starts).astype(np.int64),
                        "null": None})
            continue
        cnt = np.add.reduceat(nn.astype(np.int64), starts)
        if func == "count":
            res.append({"val": cnt, "null": None})
            continue
        isnull = (cnt == 0).astype(np.uint8)
        v = np.asarray(col)[perm]
        if func == "sum" and v.dtype == np.float64:
            val = np.zeros(ng, dtype=np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                if ng <= SUM_LOOP_GROUPS:
                    for g, (a, b) in enumerate(zip(starts.tolist(),
                                                   ends.tolist())):
                        x = v[a:b][nn[a:b]]
                        if len(x):
                            val[g] = np.cumsum(x)[-1]   # left to right
                else:
                    val = np.add.reduceat(np.where(nn, v, -0.0), starts)
                    val = np.where(isnull.astype(bool), 0.0, val)
                ab = np.add.reduceat(np.where(nn, np.abs(v), 0.0), starts)
            res.append({"val": val, "null": isnull, "abs": ab, "rows": cnt})
        elif func == "sum" and v.dtype == np.int64:
            # exact: 32-bit halves summed in int64, recombined mod 2^128
            x = np.where(nn, v, 0)
            hs = np.add.reduceat(x >> 32, starts)                 # signed
            ls = np.add.reduceat(x & 0xffffffff, starts)          # < 2^63
            a = hs.astype(np.uint64) << np.uint64(32)
            lo = a + ls.astype(np.uint64)
            hi = (hs >> 32) + (lo < a).astype(np.int64)
            res.append({"val": lo, "hi": hi, "null": isnull})
        elif func == "sum":
            res.append({"val": np.add.reduceat(
                np.where(nn, v.astype(np.int64), 0), starts),
                "null": isnull})
        else:
            # the extreme normalised key of the non-NULL rows, then the LAST
            # position holding it: on a tie the later row wins
            _, k = norm_key(v, None, False, False)
            if func == "max":
                ext = np.maximum.reduceat(np.where(nn, k, np.uint64(0)),
                                          starts)
            else:
                ext = np.minimum.reduceat(
                    np.where(nn, k, np.uint64(_MASK64)), starts)
            gid = np.cumsum(st) - 1
            hit = nn & (k == ext[gid])
            last = np.maximum.reduceat(np.where(hit, pos, -1), starts)
            val = np.zeros(ng, dtype=v.dtype)
            ok = last >= 0
            val[ok] = v[last[ok]]
            res.append({"val": val, "null": isnull})
    return {"ngroups": ng, "first_row": perm[starts], "perm": perm,
            "aggs": res}


def assert_same(a, b):
    """bit-equality of two results (abs / rows are not compared)."""
    assert a["ngroups"] == b["ngroups"]
    assert np.array_equal(a["first_row"], b["first_row"])
    assert len(a["aggs"]) == len(b["aggs"])
    for i, (x, y) in enumerate(zip(a["aggs"], b["aggs"])):
        assert x["val"].dtype == y["val"].dtype, i
        assert x["val"].tobytes() == y["val"].tobytes(), (i, x["val"],
                                                          y["val"])
        assert (x["null"] is None) == (y["null"] is None), i
        if x["null"] is not None:
            assert np.array_equal(x["null"], y["null"]), (i, x["null"],
                                                          y["null"])
        assert ("hi" in x) == ("hi" in y), i
        if "hi" in x:
            assert np.array_equal(x["hi"], y["hi"]), i

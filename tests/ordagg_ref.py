"""Reference results for the DISTINCT / ordered-set aggregates (a helper, not
a test).

A spec is sort_ref's: a list of keys (col, nulls, desc, nulls_first). The
first ngroup entries are the GROUP BY keys, entry ngroup is the argument x of
agg(DISTINCT x) / agg() WITHIN GROUP (ORDER BY x). calls is a list of
    ("count_distinct",) | ("sum_distinct",) | ("percentile_disc", p)
    | ("percentile_cont", p) | ("mode",)
perm is the position order (None: the stable sort of the whole spec).

Both functions return groupagg_ref's shape
    {"ngroups": int, "first_row": int64[ngroups], "perm": int64[n],
     "aggs": [{"val", "null", "hi", "abs", "rows"}, ...]}
val:  count_distinct int64; sum_distinct as groupagg_ref's sum (float64 /
      int64 / uint64 low word with "hi"); percentile_disc and mode the
      argument's dtype with the chosen row's bit pattern; percentile_cont
      float64. 0 under a NULL.
null: uint8, 1 where the group held no non-NULL argument (None for
      count_distinct).
abs / rows (sum_distinct over float64 only): the sum of |x| over the summed
      values and their number, for the summation bound.

loop_ordagg: a literal row loop. Per group the rows arrive in the order of
             perm, which is the order the reference's per-group tuplesort
             would deliver them in, and then
             - DISTINCT aggregates follow process_ordered_aggregate_single
               (nodeAgg.c:888): haveOldVal / oldIsNull / oldVal, skip a row
               equal to its predecessor, else advance the (strict)
               transition function: int8inc_any, float8pl, int4_sum,
               int8_sum;
             - ordered_set_transition keeps the non-NULL rows and
               number_of_rows; percentile_disc_final skips rownum - 1 rows
               and fetches one; percentile_cont_final_common fetches
               first_row / second_row and calls float8_lerp; mode_final
               walks the rows with mode_val / mode_freq / last_val /
               last_val_freq / last_val_is_mode.
             For small n.
ref_ordagg:  vectorised numpy over the normalised keys. The float sum is a
             left-to-right cumsum per group up to SUM_LOOP_GROUPS groups and
             np.add.reduceat above (exact for integer-valued data only).
             test_ordagg_host.py pins ref_ordagg == loop_ordagg.
"""
import math

import numpy as np

from groupagg_ref import SUM_LOOP_GROUPS, assert_same, group_starts  # noqa
from sort_ref import (_apply_sort_comparator, _float8_cmp_internal, _int_cmp,
                      norm_key, ref_perm)

_MASK64 = (1 << 64) - 1


def check_fraction(p):
    """the reference's argument check of both percentile finals"""
    if p < 0 or p > 1 or math.isnan(p):
        raise ValueError(f"percentile value {p:g} is not between 0 and 1")


def _norm_calls(calls):
    out = []
    for c in calls:
        c = tuple(c)
        p = float(c[1]) if len(c) > 1 else None
        if c[0] in ("percentile_disc", "percentile_cont"):
            check_fraction(p)
        out.append((c[0], p))
    return out


def _out_dtype(func, adt):
    if func == "count_distinct":
        return np.dtype(np.int64)
    if func == "sum_distinct":
        if adt == np.float64:
            return np.dtype(np.float64)
        return np.dtype(np.uint64 if adt == np.int64 else np.int64)
    if func == "percentile_cont":
        return np.dtype(np.float64)
    return np.dtype(adt)


def _blank(func, adt, ng, isnull):
    """one call's arrays for ng groups, every value 0"""
    r = {"val": np.zeros(ng, _out_dtype(func, adt)),
         "null": None if func == "count_distinct" else
         np.full(ng, 1 if isnull else 0, np.uint8)}
    if func == "sum_distinct" and adt == np.int64:
        r["hi"] = np.zeros(ng, np.int64)
    if func == "sum_distinct" and adt == np.float64:
        r["abs"] = np.zeros(ng, np.float64)
        r["rows"] = np.zeros(ng, np.int64)
    return r


def _no_rows(spec, ngroup, calls, perm):
    adt = np.asarray(spec[ngroup][0]).dtype
    if ngroup == 0:   # AGG_PLAIN over no rows: one group
        return {"ngroups": 1, "first_row": np.array([-1], dtype=np.int64),
                "perm": perm, "aggs": [_blank(f, adt, 1, True)
                                       for f, _ in calls]}
    return {"ngroups": 0, "first_row": np.zeros(0, np.int64), "perm": perm,
            "aggs": [_blank(f, adt, 0, True) for f, _ in calls]}


def _prep(spec, ngroup, calls, perm):
    spec, calls = list(spec), _norm_calls(calls)
    assert len(spec) == ngroup + 1
    n = len(spec[ngroup][0])
    if perm is None:
        perm = ref_perm(spec) if n else np.zeros(0, np.int64)
    return spec, calls, n, np.asarray(perm, dtype=np.int64)


def _i8tod(col, row):
    """the argument as float8: itself, or the integer converted"""
    return float(col[row])


def loop_ordagg(spec, ngroup, calls, perm=None):
    spec, calls, n, perm = _prep(spec, ngroup, calls, perm)
    if n == 0:
        return _no_rows(spec, ngroup, calls, perm)
    cols = []
    for col, nulls, desc, nf in spec:
        col = np.asarray(col)
        cmp = _float8_cmp_internal if col.dtype == np.float64 else _int_cmp
        nl = [False] * n if nulls is None else \
            [bool(x) for x in np.asarray(nulls).tolist()]
        cols.append((col.tolist(), nl, bool(desc), bool(nf), cmp))
    acol = np.asarray(spec[ngroup][0])
    adt = acol.dtype
    avals, anull, _, _, acmp = cols[ngroup]

    def same_group(i, j):
        for vv, nl, desc, nf, cmp in cols[:ngroup]:
            if _apply_sort_comparator(vv[i], nl[i], vv[j], nl[j], desc, nf,
                                      cmp) != 0:
                return False
        return True

    rows = perm.tolist()
    groups = []
    for j, r in enumerate(rows):
        if j == 0 or not same_group(rows[j - 1], r):
            groups.append([])
        groups[-1].append(r)
    ng = len(groups)
    res = [_blank(f, adt, ng, False) for f, _ in calls]

    for g, grows in enumerate(groups):
        # ---- process_ordered_aggregate_single, isDistinct ----
        have_old_val = False
        old_is_null = False
        old_val = None
        count = 0            # int8inc_any
        total = None         # float8pl / int4_sum / int8_sum (strict)
        sabs, srows = 0.0, 0
        for r in grows:
            new_val, is_null = avals[r], anull[r]
            if have_old_val and ((old_is_null and is_null) or
                                 (not old_is_null and not is_null and
                                  acmp(old_val, new_val) == 0)):
                continue     # equal to prior, so forget this one
            if not is_null:  # the transition functions are strict
                count += 1
                total = new_val if total is None else total + new_val
                if adt == np.float64:
                    sabs += abs(new_val)
                    srows += 1
            old_val, old_is_null, have_old_val = new_val, is_null, True
        # ---- ordered_set_transition: the non-NULL rows, in sort order ----
        sortstate = [r for r in grows if not anull[r]]
        number_of_rows = len(sortstate)

        for a, (func, p) in enumerate(calls):
            out = res[a]
            if func == "count_distinct":
                out["val"][g] = count
            elif func == "sum_distinct":
                if total is None:
                    out["null"][g] = 1
                elif adt == np.float64:
                    out["val"][g] = total
                    out["abs"][g], out["rows"][g] = sabs, srows
                elif adt == np.int64:
                    out["val"][g] = total & _MASK64
                    out["hi"][g] = total >> 64
                else:
                    out["val"][g] = total
            elif number_of_rows == 0:
                out["null"][g] = 1
            elif func == "percentile_disc":
                rownum = int(math.ceil(p * number_of_rows))
                at = 0
                if rownum > 1:
                    at += rownum - 1            # tuplesort_skiptuples
                out["val"][g] = acol[sortstate[at]]   # element copy: bits
            elif func == "percentile_cont":
                first_row = int(math.floor(p * (number_of_rows - 1)))
                second_row = int(math.ceil(p * (number_of_rows - 1)))
                first_val = _i8tod(acol, sortstate[first_row])
                if first_row == second_row:
                    val = first_val
                else:
                    second_val = _i8tod(acol, sortstate[first_row + 1])
                    proportion = (p * (number_of_rows - 1)) - first_row
                    # float8_lerp
                    val = first_val + (proportion * (second_val - first_val))
                out["val"][g] = val
            else:   # mode_final
                mode_val = None
                mode_freq = 0
                last_val = None
                last_val_freq = 0
                last_val_is_mode = False
                for r in sortstate:
                    if last_val_freq == 0:
                        mode_val = last_val = r
                        mode_freq = last_val_freq = 1
                        last_val_is_mode = True
                    elif acmp(avals[r], avals[last_val]) == 0:
                        if last_val_is_mode:
                            mode_freq += 1
                        else:
                            last_val_freq += 1
                            if last_val_freq > mode_freq:
                                mode_val = last_val
                                mode_freq = last_val_freq
                                last_val_is_mode = True
                    else:
                        last_val = r
                        last_val_freq = 1
                        last_val_is_mode = False
                out["val"][g] = acol[mode_val]
    return {"ngroups": ng,
            "first_row": np.array([gr[0] for gr in groups], dtype=np.int64),
            "perm": perm, "aggs": res}


def golden_case(doc, case):
    """(spec, ngroup, calls) of one case of tests/golden/ordagg_cases.json.
    Integer columns are int32 as in the reference's tables, float columns
    float64; a text column arrives as its rank codes (int64)."""
    t = doc["tables"][case["table"]]

    def col(name):
        v = t[name]
        if f"{case['table']}.{name}" in doc["text"]:
            return np.array(v, dtype=np.int64)
        if isinstance(v[0], float):
            return np.array(v, dtype=np.float64)
        return np.array(v, dtype=np.int32)
    spec = [(col(k), None, False, False) for k in case["keys"]]
    spec.append((col(case["arg"]), None, False, False))
    calls = [(f,) if p is None else (f, p) for f, p in case["calls"]]
    return spec, len(case["keys"]), calls


def golden_check(doc, case, res, decode=None):
    """res (this module's result shape, or any with the same "aggs" and
    "keys" = list of key arrays) against the case's expected rows. Floats are
    compared as the reference prints them: 15 significant digits. decode
    turns a text argument's values back into strings."""
    exp = case["expected"]
    nk = len(case["keys"])
    assert res["ngroups"] == len(exp)
    text = doc["text"].get(f"{case['table']}.{case['arg']}")
    for g, row in enumerate(exp):
        for c in range(nk):
            assert int(res["keys"][c][g]) == row[c]
        for a, (func, _) in enumerate(case["calls"]):
            out = res["aggs"][a]
            want = row[nk + a]
            assert out["null"] is None or out["null"][g] == 0
            got = out["val"][g]
            if isinstance(want, str):
                got = decode(got) if decode else text[int(got)]
                assert got == want, (case["name"], g, a)
            elif isinstance(want, float):
                assert float(f"{float(got):.15g}") == want, \
                    (case["name"], g, a, float(got))
            else:
                assert int(got) == want, (case["name"], g, a)


def flags(spec, ngroup, perm):
    """(group start, run start, argument is NULL) per position"""
    gst = group_starts(spec[:ngroup], perm)
    col, nulls, desc, nf = spec[ngroup]
    nb, k = norm_key(col, nulls, desc, nf)
    nb, k = nb[perm], k[perm]
    run = gst.copy()
    run[1:] |= (nb[1:] != nb[:-1]) | (k[1:] != k[:-1])
    isnull = np.zeros(len(perm), dtype=bool) if nulls is None else \
        np.asarray(nulls).astype(bool)[perm]
    return gst, run, isnull


def ref_ordagg(spec, ngroup, calls, perm=None):
    spec, calls, n, perm = _prep(spec, ngroup, calls, perm)
    if n == 0:
        return _no_rows(spec, ngroup, calls, perm)
    gst, run, isnull = flags(spec, ngroup, perm)
    nn = ~isnull
    starts = np.flatnonzero(gst)
    ends = np.append(starts[1:], n)
    ng = len(starts)
    pos = np.arange(n, dtype=np.int64)
    v = np.asarray(spec[ngroup][0])[perm]
    adt = v.dtype
    N = np.add.reduceat(nn.astype(np.int64), starts)
    has = N > 0
    lo = np.minimum.reduceat(np.where(nn, pos, n), starts)
    lo0 = np.where(has, lo, 0)
    first = run & nn          # the first position of a run of non-NULL values
    res = []
    for func, p in calls:
        out = _blank(func, adt, ng, False)
        if out["null"] is not None:
            out["null"][:] = (~has).astype(np.uint8)
        if func == "count_distinct":
            out["val"] = np.add.reduceat(first.astype(np.int64), starts)
        elif func == "sum_distinct" and adt == np.float64:
            val = np.zeros(ng, dtype=np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                if ng <= SUM_LOOP_GROUPS:
                    for g, (a, b) in enumerate(zip(starts.tolist(),
                                                   ends.tolist())):
                        x = v[a:b][first[a:b]]
                        if len(x):
                            val[g] = np.cumsum(x)[-1]   # left to right
                else:
                    val = np.add.reduceat(np.where(first, v, -0.0), starts)
                    val = np.where(has, val, 0.0)
                out["abs"] = np.add.reduceat(
                    np.where(first, np.abs(v), 0.0), starts)
            out["val"] = val
            out["rows"] = np.add.reduceat(first.astype(np.int64), starts)
        elif func == "sum_distinct" and adt == np.int64:
            x = np.where(first, v, 0)
            hs = np.add.reduceat(x >> 32, starts)
            ls = np.add.reduceat(x & 0xffffffff, starts)
            a = hs.astype(np.uint64) << np.uint64(32)
            lw = a + ls.astype(np.uint64)
            out["val"] = lw
            out["hi"] = (hs >> 32) + (lw < a).astype(np.int64)
        elif func == "sum_distinct":
            out["val"] = np.add.reduceat(
                np.where(first, v.astype(np.int64), 0), starts)
        elif func == "percentile_disc":
            K = np.ceil(p * N.astype(np.float64)).astype(np.int64)
            at = lo0 + np.maximum(K, 1) - 1
            out["val"][has] = v[at[has]]
        elif func == "percentile_cont":
            t = p * (N - 1).astype(np.float64)
            fl, ce = np.floor(t), np.ceil(t)
            i0 = np.where(has, lo0 + fl.astype(np.int64), 0)
            i1 = np.where(has, lo0 + ce.astype(np.int64), 0)
            with np.errstate(invalid="ignore", over="ignore"):
                v0 = v[i0].astype(np.float64)
                v1 = v[i1].astype(np.float64)
                lerp = v0 + ((t - fl) * (v1 - v0))
            val = np.where(fl == ce, v0, lerp)
            out["val"][has] = val[has]
        else:   # mode: the longest run, the earliest among equals
            b = np.flatnonzero(run)
            cex = np.concatenate(([0], np.cumsum(nn.astype(np.int64))))
            length = cex[np.append(b[1:], n)] - cex[b]
            gid = (np.cumsum(gst) - 1)[b]
            order = np.lexsort((b, -length, gid))
            pick = order[np.flatnonzero(np.append(
                True, gid[order][1:] != gid[order][:-1]))]
            assert len(pick) == ng
            ok = length[pick] > 0
            assert np.array_equal(ok, has)
            out["val"][ok] = v[b[pick][ok]]
        res.append(out)
    return {"ngroups": ng, "first_row": perm[starts], "perm": perm,
            "aggs": res}

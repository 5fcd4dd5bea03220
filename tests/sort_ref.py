"""Reference orderings for the generic Sort operator (a helper, not a test).

A spec is a list of keys, primary first; each key is a tuple
    (col, nulls, desc, nulls_first)
with col a numpy array of dtype int64 / float64 / int32 / uint8, nulls a
uint8/bool array (nonzero = NULL) or None, and two bools.

cmp_perm: a comparator sort that restates ApplySortComparator
          (include/utils/sortsupport.h:201) and float8_cmp_internal
          (utils/adt/float.c:1172) literally; O(n log n) Python calls, for
          small n.
ref_perm: a numpy stable lexsort over normalised (null bit, key) pairs, for
          large n. test_sort_host.py pins ref_perm == cmp_perm.
Both are stable, so the permutation is unique.
"""
import math
from functools import cmp_to_key

import numpy as np


def _float8_cmp_internal(a, b):
    # float.c:1172 — NaN == NaN, NaN > every non-NaN
    if math.isnan(a):
        return 0 if math.isnan(b) else 1
    if math.isnan(b):
        return -1
    if a > b:
        return 1
    if a < b:
        return -1
    return 0


def _int_cmp(a, b):
    # btint8cmp / btint4cmp (nbtcompare.c:129)
    return 1 if a > b else (-1 if a < b else 0)


def _apply_sort_comparator(d1, n1, d2, n2, desc, nulls_first, cmp):
    # sortsupport.h:201
    if n1:
        if n2:
            return 0                       # NULL "=" NULL
        return -1 if nulls_first else 1    # NULL "<" / ">" NOT_NULL
    if n2:
        return 1 if nulls_first else -1
    c = cmp(d1, d2)
    return -c if desc else c               # ssup_reverse


def cmp_perm(spec):
    cols = []
    for col, nulls, desc, nf in spec:
        col = np.asarray(col)
        cmp = _float8_cmp_internal if col.dtype == np.float64 else _int_cmp
        vals = col.tolist()
        nl = [False] * len(vals) if nulls is None else \
            [bool(x) for x in np.asarray(nulls).tolist()]
        cols.append((vals, nl, bool(desc), bool(nf), cmp))
    n = len(cols[0][0])

    def compare(i, j):
        for vals, nl, desc, nf, cmp in cols:
            c = _apply_sort_comparator(vals[i], nl[i], vals[j], nl[j], desc,
                                       nf, cmp)
            if c:
                return c
        return 0

    return np.array(sorted(range(n), key=cmp_to_key(compare)), dtype=np.int64)


def norm_key(col, nulls, desc, nulls_first):
    """(null bit, unsigned key): ascending order of the pair = the column's
    order under (desc, nulls_first)."""
    a = np.ascontiguousarray(col)
    top = np.uint64(1 << 63)
    if a.dtype == np.int64:
        k, full = a.view(np.uint64) ^ top, np.uint64(0xffffffffffffffff)
    elif a.dtype == np.float64:
        b = a.view(np.uint64).copy()
        b[a != a] = np.uint64(0x7ff8000000000000)
        b[a == 0.0] = np.uint64(0)
        neg = (b >> np.uint64(63)).astype(bool)
        k = np.where(neg, ~b, b ^ top)
        full = np.uint64(0xffffffffffffffff)
    elif a.dtype == np.int32:
        k = (a.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
        full = np.uint64(0xffffffff)
    elif a.dtype == np.uint8:
        k, full = a.astype(np.uint64), np.uint64(0xff)
    else:
        raise TypeError(a.dtype)
    if desc:
        k = k ^ full
    isnull = np.zeros(len(a), dtype=bool) if nulls is None \
        else np.asarray(nulls).astype(bool)
    k = np.where(isnull, np.uint64(0), k)
    if nulls_first:
        nb = np.where(isnull, 0, 1)
    else:
        nb = np.where(isnull, 1, 0)
    return nb.astype(np.uint8), k


def ref_perm(spec):
    cols = []   # np.lexsort sorts by the LAST entry first
    for col, nulls, desc, nf in reversed(list(spec)):
        nb, k = norm_key(col, nulls, desc, nf)
        cols += [k, nb]
    return np.lexsort(cols).astype(np.int64)

"""Reference for the Filter operator (otbx_filter_sel / GpuFilter): two
independent restatements of the reference's qual evaluation over numpy
columns. A qual is `clauses`, a list of lists of terms — the AND of ORs — and
a term is the tuple made by term():

    (col, op, rhs, nulls, rnulls)

col: numpy column (int64, float64, int32 or uint8); op: "=", "<>", "<", "<=",
">", ">=", "isnull" or "notnull"; rhs: a Python number, a column of col's
dtype, or None for the null tests; nulls / rnulls: uint8 masks, nonzero =
NULL, or None.

ref_sel   vectorised: every term becomes a (value, isnull) pair of boolean
          arrays, combined with Kleene OR inside a clause and Kleene AND over
          the clauses; a row is selected iff the result is TRUE and not NULL.
step_sel  one row at a time, restating the step machine of
          executor/execExprInterp.c: EEOP_FUNCEXPR_STRICT (:703, a NULL
          argument makes the result NULL without calling the operator),
          EEOP_NULLTEST_ISNULL / _ISNOTNULL (:973), EEOP_BOOL_OR_STEP_FIRST /
          _STEP / _STEP_LAST (:850-904, anynull tracking, jump out at the
          first TRUE) and EEOP_QUAL (:919, NULL or FALSE ends the qual with
          FALSE); floats compare through a restatement of
          float8_cmp_internal (utils/adt/float.c:1172).

Both return the ascending int64 array of selected row indices.
"""
import itertools
import math

import numpy as np

OPS = ("=", "<>", "<", "<=", ">", ">=", "isnull", "notnull")


def term(col, op, rhs=None, nulls=None, rnulls=None):
    return (col, op, rhs, nulls, rnulls)


def _nrows(clauses, n):
    for c in clauses:
        for t in c:
            return len(t[0])
    assert n is not None, "a qual without terms needs n"
    return n


# ---------------- vectorised: (value, isnull) pairs, Kleene ----------------

def _lt_eq(a, b, is_float):
    """elementwise (a < b, a == b) in the column type's order"""
    if not is_float:
        return a < b, a == b
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        eq = (an & bn) | (~an & ~bn & (a == b))
        lt = ~an & (bn | (a < b))
    return lt, eq


def _term_pair(t, n):
    col, op, rhs, nulls, rnulls = t
    isnull = np.zeros(n, dtype=bool) if nulls is None else nulls != 0
    if op == "isnull":
        return isnull.copy(), np.zeros(n, dtype=bool)
    if op == "notnull":
        return ~isnull, np.zeros(n, dtype=bool)
    is_float = col.dtype == np.float64
    if is_float:
        a = col
        b = rhs if isinstance(rhs, np.ndarray) else \
            np.full(n, float(rhs), dtype=np.float64)
    else:
        # exact: every column value and every int64 constant fits an int64
        a = col.astype(np.int64)
        b = rhs.astype(np.int64) if isinstance(rhs, np.ndarray) else \
            np.full(n, int(rhs), dtype=np.int64)
    if isinstance(rhs, np.ndarray) and rnulls is not None:
        isnull = isnull | (rnulls != 0)
    lt, eq = _lt_eq(a, b, is_float)
    val = {"=": eq, "<>": ~eq, "<": lt, "<=": lt | eq, ">": ~(lt | eq),
           ">=": ~lt}[op]
    # the value under a NULL is meaningless: blank it so nothing can use it
    return val & ~isnull, isnull


def _kleene_or(pairs, n):
    true = np.zeros(n, dtype=bool)
    anynull = np.zeros(n, dtype=bool)
    for v, nl in pairs:
        true |= v & ~nl
        anynull |= nl
    return true, ~true & anynull


def _kleene_and(pairs, n):
    false = np.zeros(n, dtype=bool)
    anynull = np.zeros(n, dtype=bool)
    for v, nl in pairs:
        false |= ~v & ~nl
        anynull |= nl
    isnull = ~false & anynull
    return ~false & ~isnull, isnull


def ref_sel(clauses, n=None):
    n = _nrows(clauses, n)
    ors = [_kleene_or([_term_pair(t, n) for t in c], n) for c in clauses]
    val, isnull = _kleene_and(ors, n)
    return np.flatnonzero(val & ~isnull).astype(np.int64)


# ---------------- row at a time: the EEOP_* step machine ----------------

def float8_cmp_internal(a, b):
    """utils/adt/float.c:1172: NaN == NaN, NaN > every non-NaN"""
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
    return (a > b) - (a < b)


_OP_ON_CMP = {"=": lambda c: c == 0, "<>": lambda c: c != 0,
              "<": lambda c: c < 0, "<=": lambda c: c <= 0,
              ">": lambda c: c > 0, ">=": lambda c: c >= 0}


def _step_term(t, r):
    """(value, isnull) of one term on row r"""
    col, op, rhs, nulls, rnulls = t
    lnull = nulls is not None and nulls[r] != 0
    if op == "isnull":                     # EEOP_NULLTEST_ISNULL: never NULL
        return lnull, False
    if op == "notnull":
        return not lnull, False
    is_col = isinstance(rhs, np.ndarray)
    rnull = is_col and rnulls is not None and rnulls[r] != 0
    if lnull or rnull:                     # EEOP_FUNCEXPR_STRICT
        return False, True
    if col.dtype == np.float64:
        c = float8_cmp_internal(float(col[r]),
                                float(rhs[r]) if is_col else float(rhs))
    else:
        c = _int_cmp(int(col[r]), int(rhs[r]) if is_col else int(rhs))
    return _OP_ON_CMP[op](c), False


def _step_or(clause, r):
    anynull = False                        # EEOP_BOOL_OR_STEP_FIRST
    for t in clause:
        v, nl = _step_term(t, r)
        if nl:
            anynull = True
        elif v:
            return True, False             # jump to the end: TRUE
    return False, anynull                  # EEOP_BOOL_OR_STEP_LAST


def step_sel(clauses, n=None):
    n = _nrows(clauses, n)
    out = []
    for r in range(n):
        ok = True
        for clause in clauses:
            v, nl = _step_or(clause, r)
            if nl or not v:                # EEOP_QUAL: done, FALSE
                ok = False
                break
        if ok:
            out.append(r)
    return np.array(out, dtype=np.int64)


# ---------------- the three-valued truth tables ----------------

TV = (True, False, None)


def k_or(a, b):
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def k_and(a, b):
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def truth_table(nterms):
    """columns realising every assignment: term i is `col_i = 1` with value
    1 (TRUE), 0 (FALSE) or a NULL over garbage"""
    rows = list(itertools.product(TV, repeat=nterms))
    cols, masks = [], []
    for i in range(nterms):
        cols.append(np.array([1 if r[i] is True else 0 if r[i] is False
                              else 1 for r in rows], dtype=np.int32))
        masks.append(np.array([r[i] is None for r in rows], dtype=np.uint8))
    return rows, cols, masks


def truth_cases():
    """(name, clauses, expected selection) for a OR b, a AND b,
    (a OR b) AND c: 9 + 9 + 27 rows"""
    out = []
    rows, c, m = truth_table(2)
    a, b = term(c[0], "=", 1, m[0]), term(c[1], "=", 1, m[1])
    out.append(("or", [[a, b]],
                [i for i, r in enumerate(rows) if k_or(*r) is True]))
    out.append(("and", [[a], [b]],
                [i for i, r in enumerate(rows) if k_and(*r) is True]))
    rows, c, m = truth_table(3)
    a, b, d = (term(c[i], "=", 1, m[i]) for i in range(3))
    out.append(("or_and", [[a, b], [d]],
                [i for i, r in enumerate(rows)
                 if k_and(k_or(r[0], r[1]), r[2]) is True]))
    return out

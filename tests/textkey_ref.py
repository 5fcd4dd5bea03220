"""Row-loop references for the text rank (otbx_text_rank; a helper, not a
test). Rows are lists of bytes / None, the host image text_ref.clamped_rows
gives of a column; several columns are ranked as their concatenation.

rank_cmp: sorts the non-NULL rows with a comparator that restates the C
          branch of varstr_cmp (utils/adt/varlena.c:1614-1629) byte by byte:
          memcmp over the common prefix with unsigned bytes, then the
          shorter string is smaller. Equality is comparator == 0.
rank_set: Python's own bytes order: sorted(set(rows)) and a dict.
Both return (codes, ndistinct, dict_rows): codes[i] = number of distinct
non-NULL strings strictly smaller than row i, -1 under a NULL; dict_rows[c]
= the first row holding code c. test_textkey_host.py pins them to each
other.
"""
from functools import cmp_to_key

from sort_ref import _apply_sort_comparator, _int_cmp
from text_ref import clamped_rows


def varstr_cmp_c(a, b):
    """varstr_cmp with lc_collate_is_c: memcmp(a, b, Min(len1, len2)), and
    on a tie the length decides."""
    m = len(a) if len(a) < len(b) else len(b)
    result = 0
    for i in range(m):                     # memcmp: unsigned bytes
        if a[i] != b[i]:
            result = -1 if a[i] < b[i] else 1
            break
    if result == 0 and len(a) != len(b):
        result = -1 if len(a) < len(b) else 1
    return result


def rank_cmp(rows):
    live = [i for i, r in enumerate(rows) if r is not None]
    # a stable sort keeps equal strings in row order: the first of a run is
    # the first occurrence
    order = sorted(live, key=cmp_to_key(
        lambda i, j: varstr_cmp_c(rows[i], rows[j])))
    codes = [-1] * len(rows)
    dict_rows = []
    for k, i in enumerate(order):
        if k == 0 or varstr_cmp_c(rows[order[k - 1]], rows[i]) != 0:
            dict_rows.append(i)
        codes[i] = len(dict_rows) - 1
    return codes, len(dict_rows), dict_rows


def rank_set(rows):
    d = sorted(set(r for r in rows if r is not None))
    code = {s: c for c, s in enumerate(d)}
    codes = [-1 if r is None else code[r] for r in rows]
    first = {}
    for i, r in enumerate(rows):
        if r is not None:
            first.setdefault(r, i)
    return codes, len(d), [first[s] for s in d]


def column_rows(raw, offs, nulls=None):
    """the host image of a column under the kernels' clamping policy"""
    return clamped_rows(raw, offs, nulls)


def text_sort_perm(rows, desc=False, nulls_first=None, then=None,
                   then_desc=False):
    """ORDER BY text [DESC] [NULLS FIRST|LAST] [, then [DESC]]: a stable
    comparator sort over the strings themselves through ApplySortComparator
    (sort_ref). `then` is an int list without NULLs."""
    if nulls_first is None:
        nulls_first = bool(desc)

    def compare(i, j):
        c = _apply_sort_comparator(rows[i], rows[i] is None, rows[j],
                                   rows[j] is None, desc, nulls_first,
                                   varstr_cmp_c)
        if c == 0 and then is not None:
            c = _apply_sort_comparator(then[i], False, then[j], False,
                                       then_desc, False, _int_cmp)
        return c

    return sorted(range(len(rows)), key=cmp_to_key(compare))

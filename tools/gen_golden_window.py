#!/usr/bin/env python3
"""Generate tests/golden/window_cases.json from the reference's regression
suite: window functions over explicit and default frames on tenk1.

    tools/gen_golden_window.py <reference>/src/test/regress

Input rows: the rows of data/tenk.data with unique2 < 10, and those with
unique1 < 10 (unique1, unique2, four, ten — columns 1, 2, 4 and 5 of the
tab-separated file). Expected: the result blocks of expected/window.out for
ntile(3), lag, lead, lead with a default, first_value, last_value over the
default frame and over a whole partition, the five sum(unique1) OVER (ROWS
BETWEEN ...) queries, and first_value / nth_value(.., 2) / last_value over a
RANGE CURRENT ROW .. UNBOUNDED FOLLOWING window. Queries with per-row
offsets (lag(ten, four), nth_value(ten, four + 1)) are not recorded. Every
recorded case either fixes its input order in the query ("presort") or has a
result multiset that does not depend on the order of tied rows; the tests
compare sorted multisets of output rows.

Runs where the reference tree exists; the committed fixture is what the tests
read. Data only.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                   "golden", "window_cases.json")

# name, first line of the query, rows filter, presort, partition keys, order
# keys, frame (units, start, end; None = unbounded, 0 = current row), calls
# (function, column, offset / n / buckets, default), shown columns.
# "ten2" is the expression ten * 2.
CASES = (
    ("ntile3", "SELECT ntile(3) OVER (ORDER BY ten, four), ten, four FROM",
     "unique2", None, [], ["ten", "four"], ["range", None, 0],
     [["ntile", None, 3, None]], ["ten", "four"]),
    ("lag", "SELECT lag(ten) OVER (PARTITION BY four ORDER BY ten), ten,",
     "unique2", None, ["four"], ["ten"], ["range", None, 0],
     [["lag", "ten", 1, None]], ["ten", "four"]),
    ("lead", "SELECT lead(ten) OVER (PARTITION BY four ORDER BY ten), ten,",
     "unique2", None, ["four"], ["ten"], ["range", None, 0],
     [["lead", "ten", 1, None]], ["ten", "four"]),
    ("lead_default", "SELECT lead(ten * 2, 1, -1) OVER (PARTITION BY four",
     "unique2", None, ["four"], ["ten"], ["range", None, 0],
     [["lead", "ten2", 1, -1]], ["ten", "four"]),
    ("first_value", "SELECT first_value(ten) OVER (PARTITION BY four ORDER",
     "unique2", None, ["four"], ["ten"], ["range", None, 0],
     [["first_value", "ten", None, None]], ["ten", "four"]),
    ("last_value_default_frame", "SELECT last_value(four) OVER (ORDER BY ten,",
     "unique2", None, [], ["ten", "four"], ["range", None, 0],
     [["last_value", "four", None, None]], ["ten", "four"]),
    ("last_value_partition", "SELECT last_value(ten) OVER (PARTITION BY four),",
     "unique2", ["four", "ten"], ["four"], [], ["range", None, 0],
     [["last_value", "ten", None, None]], ["ten", "four"]),
    ("sum_rows_current_unbounded",
     "SELECT sum(unique1) over (rows between current row and unbounded",
     "unique1", ["unique1", "four"], [], [], ["rows", 0, None],
     [["sum", "unique1", None, None]], ["unique1", "four"]),
    ("sum_rows_2p_2f",
     "SELECT sum(unique1) over (rows between 2 preceding and 2 following),",
     "unique1", ["unique1", "four"], [], [], ["rows", -2, 2],
     [["sum", "unique1", None, None]], ["unique1", "four"]),
    ("sum_rows_2p_1p",
     "SELECT sum(unique1) over (rows between 2 preceding and 1 preceding),",
     "unique1", ["unique1", "four"], [], [], ["rows", -2, -1],
     [["sum", "unique1", None, None]], ["unique1", "four"]),
    ("sum_rows_1f_3f",
     "SELECT sum(unique1) over (rows between 1 following and 3 following),",
     "unique1", ["unique1", "four"], [], [], ["rows", 1, 3],
     [["sum", "unique1", None, None]], ["unique1", "four"]),
    ("sum_rows_unbounded_1f",
     "SELECT sum(unique1) over (rows between unbounded preceding and 1",
     "unique1", ["unique1", "four"], [], [], ["rows", None, 1],
     [["sum", "unique1", None, None]], ["unique1", "four"]),
    ("first_nth_last_range_current_unbounded",
     "SELECT first_value(unique1) over w,",
     "unique1", None, [], ["four", "ten", "unique1"], ["range", 0, None],
     [["first_value", "unique1", None, None], ["nth_value", "unique1", 2, None],
      ["last_value", "unique1", None, None]], ["unique1", "four"]),
)


def result_block(lines, i):
    """rows of the first psql table at or after lines[i]; '' is NULL"""
    while not (lines[i] and set(lines[i]) <= set("-+")):
        i += 1
    rows = []
    i += 1
    while not lines[i].startswith("("):
        rows.append([int(c) if c.strip() else None
                     for c in lines[i].split("|")])
        i += 1
    assert lines[i] == f"({len(rows)} rows)", lines[i]
    return rows


def main(regress):
    table = {"unique1": [], "unique2": []}
    for line in open(os.path.join(regress, "data", "tenk.data")):
        f = line.rstrip("\n").split("\t")
        row = {"unique1": int(f[0]), "unique2": int(f[1]), "four": int(f[3]),
               "ten": int(f[4]), "ten2": int(f[4]) * 2}
        for k in table:
            if row[k] < 10:
                table[k].append(row)
    assert len(table["unique1"]) == 10 and len(table["unique2"]) == 10

    out = open(os.path.join(regress, "expected", "window.out")).read() \
        .split("\n")
    cases = []
    for name, first, filt, presort, part, order, frame, calls, shown in CASES:
        hits = [k for k, l in enumerate(out) if l.startswith(first)]
        assert len(hits) == 1, (name, hits)
        rows = result_block(out, hits[0])
        assert len(rows) == 10 and len(rows[0]) == len(calls) + len(shown)
        cases.append({"name": name, "line": hits[0] + 1, "rows": filt,
                      "presort": presort, "partition": part, "order": order,
                      "frame": frame, "calls": calls, "shown": shown,
                      "expected": rows})

    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "src/test/regress: data/tenk.data (unique1 < 10;"
                             " unique2 < 10), expected/window.out",
                   "tables": table, "cases": cases}, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

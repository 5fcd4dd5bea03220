#!/usr/bin/env python3
"""Generate tests/golden/text_order_cases.json from the reference's
regression suite: text ORDER BY / DISTINCT over onek.

    tools/gen_golden_text.py <reference>/src/test/regress

Input rows: the 19 rows of data/onek.data with unique1 > 980 (unique1,
stringu1, string4 — columns 1, 14 and 16 of the tab-separated file).
Expected: the three result blocks of expected/select.out
    ORDER BY stringu1 using <
    ORDER BY string4 using <, unique1 using >
    ORDER BY string4 using >, unique1 using <
and the four rows of SELECT DISTINCT string4 in expected/select_distinct.out.
Runs where the reference tree exists; the committed fixture is what the
tests read. Data only.
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                   "golden", "text_order_cases.json")

BLOCKS = (
    ("stringu1_asc", "ORDER BY stringu1 using <;"),
    ("string4_asc_unique1_desc", "ORDER BY string4 using <, unique1 using >;"),
    ("string4_desc_unique1_asc", "ORDER BY string4 using >, unique1 using <;"),
)


def result_block(lines, i):
    """rows of the psql table whose header line is lines[i]"""
    assert set(lines[i + 1]) <= set("-+"), lines[i + 1]
    rows = []
    i += 2
    while not lines[i].startswith("("):
        rows.append([c.strip() for c in lines[i].split("|")])
        i += 1
    assert lines[i] == f"({len(rows)} rows)", lines[i]
    return rows


def main(regress):
    rows = []
    for line in open(os.path.join(regress, "data", "onek.data")):
        f = line.rstrip("\n").split("\t")
        if int(f[0]) > 980:
            rows.append({"unique1": int(f[0]), "stringu1": f[13],
                         "string4": f[15]})
    assert len(rows) == 19

    sel = open(os.path.join(regress, "expected", "select.out")).read() \
        .split("\n")
    orders = {}
    for name, last in BLOCKS:
        i = next(k for k, l in enumerate(sel)
                 if l.strip() == last and "unique1 > 980" in sel[k - 1])
        got = result_block(sel, i + 1)
        assert len(got) == 19
        orders[name] = [[int(u), s] for u, s in got]

    dis = open(os.path.join(regress, "expected", "select_distinct.out")) \
        .read().split("\n")
    i = next(k for k, l in enumerate(dis)
             if l.strip() == "SELECT DISTINCT string4 FROM tmp ORDER BY 1;")
    distinct = [r[0] for r in result_block(dis, i + 1)]
    assert len(distinct) == 4

    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "src/test/regress: data/onek.data (unique1 > "
                             "980), expected/select.out, "
                             "expected/select_distinct.out",
                   "rows": rows, "orders": orders,
                   "distinct_string4": distinct}, f, indent=0)
        f.write("\n")
    print(f"{len(rows)} rows, {len(orders)} orders -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

#!/usr/bin/env python3
"""Generate tests/golden/ordagg_cases.json from the reference's regression
suite: DISTINCT and ordered-set aggregates of expected/aggregates.out.

    tools/gen_golden_ordagg.py <reference>/src/test/regress

Input columns: four and ten of data/onek.data; ten, thousand and string4 of
data/tenk.data (string4 as an index into its sorted list of distinct
strings); b of data/agg.data, a float4 column, stored as the float32-rounded
value widened to a double; generate_series(1,5) / (1,6) and the twelve names
of the unnest() query, which the queries themselves spell out. Expected: the
result blocks of the queries named in CASES. A case is
    name, line         where the query starts in aggregates.out
    table, keys, arg   the input: GROUP BY columns and the argument column
    calls              [function, fraction or null] in output order
    expected           one list per group, in key order: the key values, then
                       one value per call. Text values are strings.
count(four) of the "sum(DISTINCT four)" query is an ordinary aggregate and is
recorded as the extra column "count".

Runs where the reference tree exists; the committed fixture is what the tests
read. Data only.
"""
import json
import os
import struct
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                   "golden", "ordagg_cases.json")

NAMES = "fred,jim,fred,jack,jill,fred,jill,jim,jim,sheila,jim,sheila"
P9 = [0, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 1]
P11 = [0, 1, 0.25, 0.75, 0.5, 1, 0.3, 0.32, 0.35, 0.38, 0.4]


def block(lines, i):
    """cells of the first psql table at or after lines[i]"""
    while not (lines[i] and set(lines[i]) <= set("-+")):
        i += 1
    rows = []
    i += 1
    while not lines[i].startswith("("):
        rows.append([c.strip() for c in lines[i].split("|")])
        i += 1
    assert lines[i] in (f"({len(rows)} rows)", "(1 row)"), lines[i]
    return rows


def array(cell, conv):
    assert cell[0] == "{" and cell[-1] == "}"
    return [conv(x) for x in cell[1:-1].split(",")]


def main(regress):
    def data(name):
        return [line.rstrip("\n").split("\t")
                for line in open(os.path.join(regress, "data", name))]

    onek, tenk, agg = data("onek.data"), data("tenk.data"), data("agg.data")
    assert len(onek) == 1000 and len(tenk) == 10000
    strings = sorted({f[15] for f in tenk})
    names = NAMES.split(",")
    name_list = sorted(set(names))
    f32 = [struct.unpack("f", struct.pack("f", float(f[1])))[0] for f in agg]
    tables = {
        "onek": {"four": [int(f[3]) for f in onek],
                 "ten": [int(f[4]) for f in onek]},
        "tenk1": {"ten": [int(f[4]) for f in tenk],
                  "thousand": [int(f[7]) for f in tenk],
                  "string4": [strings.index(f[15]) for f in tenk]},
        "aggtest": {"b": f32},
        "series5": {"x": [1.0, 2.0, 3.0, 4.0, 5.0]},
        "series6": {"x": [1, 2, 3, 4, 5, 6]},
        "names": {"x": [name_list.index(s) for s in names]},
    }
    text = {"tenk1.string4": strings, "names.x": name_list}

    out = open(os.path.join(regress, "expected", "aggregates.out")).read() \
        .split("\n")

    def find(first, nth=0):
        hits = [k for k, l in enumerate(out) if l.startswith(first)]
        assert len(hits) > nth, first
        return hits[nth]

    cases = []

    def case(name, line, table, keys, arg, calls, expected, **more):
        cases.append(dict({"name": name, "line": line + 1, "table": table,
                           "keys": keys, "arg": arg, "calls": calls,
                           "expected": expected}, **more))

    i = find("SELECT count(DISTINCT four) AS cnt_4 FROM onek;")
    case("count_distinct_four", i, "onek", [], "four",
         [["count_distinct", None]], [[int(block(out, i)[0][0])]])

    i = find("select ten, count(four), sum(DISTINCT four) from onek")
    rows = [[int(c) for c in r] for r in block(out, i)]
    assert len(rows) == 10
    case("sum_distinct_four_by_ten", i, "onek", ["ten"], "four",
         [["sum_distinct", None]], [[r[0], r[2]] for r in rows],
         count=[r[1] for r in rows])

    i = find("select p, percentile_cont(p) within group (order by x::float8)")
    rows = block(out, i)
    assert [float(r[0]) for r in rows] == P9
    case("percentile_cont_series5", i, "series5", [], "x",
         [["percentile_cont", p] for p in P9],
         [[float(r[1]) for r in rows]])

    i = find("select percentile_cont(0.5) within group (order by b) from "
             "aggtest;")
    case("percentile_cont_aggtest_b", i, "aggtest", [], "b",
         [["percentile_cont", 0.5]], [[float(block(out, i)[0][0])]],
         digits=15)

    i = find("select percentile_cont(0.5) within group (order by thousand) "
             "from tenk1;")
    case("percentile_cont_thousand", i, "tenk1", [], "thousand",
         [["percentile_cont", 0.5]], [[float(block(out, i)[0][0])]])

    i = find("select percentile_disc(0.5) within group (order by thousand) "
             "from tenk1;")
    case("percentile_disc_thousand", i, "tenk1", [], "thousand",
         [["percentile_disc", 0.5]], [[int(block(out, i)[0][0])]])

    i = find("select percentile_disc(array[0,0.1,0.25,0.5,0.75,0.9,1]) "
             "within group (order by thousand)")
    case("percentile_disc_array_thousand", i, "tenk1", [], "thousand",
         [["percentile_disc", p] for p in [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1]],
         [array(block(out, i)[0][0], int)])

    i = find("select percentile_cont(array[0,0.25,0.5,0.75,1]) within group "
             "(order by thousand)")
    case("percentile_cont_array_thousand", i, "tenk1", [], "thousand",
         [["percentile_cont", p] for p in [0, 0.25, 0.5, 0.75, 1]],
         [array(block(out, i)[0][0], float)])

    i = find("select percentile_cont(array[0,1,0.25,0.75,0.5,1,0.3,0.32,0.35,"
             "0.38,0.4]) within group (order by x)")
    case("percentile_cont_array_series6", i, "series6", [], "x",
         [["percentile_cont", p] for p in P11],
         [array(block(out, i)[0][0], float)])

    i = find("select ten, mode() within group (order by string4) from tenk1 "
             "group by ten;")
    rows = block(out, i)
    assert len(rows) == 10
    case("mode_string4_by_ten", i, "tenk1", ["ten"], "string4",
         [["mode", None]], [[int(r[0]), r[1]] for r in rows])

    i = find("select percentile_disc(array[0.25,0.5,0.75]) within group "
             "(order by x)")
    assert NAMES in out[i + 1]
    case("percentile_disc_array_names", i, "names", [], "x",
         [["percentile_disc", p] for p in [0.25, 0.5, 0.75]],
         [array(block(out, i)[0][0], str)])

    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "src/test/regress: data/onek.data, "
                             "data/tenk.data, data/agg.data, "
                             "expected/aggregates.out",
                   "tables": tables, "text": text, "cases": cases}, f,
                  indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

#!/usr/bin/env python3
"""Generate tests/golden/like_cases.json from the reference's regression
output: every LIKE / NOT LIKE (with or without ESCAPE) of
src/test/regress/expected/strings.out, from "-- test LIKE" to "-- test
implicit type conversion" (ILIKE is out of scope and skipped).

    tools/gen_like_golden.py <reference>/src/test/regress/expected/strings.out

Each record is {text, pattern, escape, negate, expected}: escape is null
without an ESCAPE clause. Runs where the reference tree exists; the
committed fixture is what the tests read.
"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests",
                   "golden", "like_cases.json")
EXPR = re.compile(r"'((?:[^']|'')*)' (NOT )?LIKE '((?:[^']|'')*)'"
                  r"(?: ESCAPE '((?:[^']|'')*)')?")


def unquote(s):
    return s.replace("''", "'")


def main(path):
    lines = open(path, encoding="utf-8").read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.strip() == "-- test LIKE")
    end = next(i for i, l in enumerate(lines)
               if l.strip() == "-- test implicit type conversion")
    cases = []
    i = start
    while i < end:
        line = lines[i]
        if line.startswith("SELECT") and " LIKE " in line:
            exprs = EXPR.findall(line)
            assert exprs, line
            # header, dashes, the one result row
            assert set(lines[i + 2]) <= set("-+"), lines[i + 2]
            got = [c.strip() for c in lines[i + 3].split("|")]
            assert len(got) == len(exprs) and set(got) <= {"t", "f"}, line
            for (text, neg, pat, esc), res in zip(exprs, got):
                has_esc = " ESCAPE " in line
                cases.append({"text": unquote(text), "pattern": unquote(pat),
                              "escape": unquote(esc) if has_esc else None,
                              "negate": bool(neg), "expected": res == "t"})
            i += 4
        else:
            i += 1
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"source": "src/test/regress/expected/strings.out "
                             "(-- test LIKE .. %/_ combination cases)",
                   "cases": cases}, f, indent=0, ensure_ascii=False)
        f.write("\n")
    print(f"{len(cases)} cases -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

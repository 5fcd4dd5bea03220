"""The CPU oracle against a brute-force reference on hand-built tables (no
GPU needed). test_gpu_fragments_crafted.py compares the kernels with the
oracle on these same cases; this file pins the oracle itself first, so a GPU
mismatch there points at the kernels. Everything compares with ==: the
builders in fragment_ref.py keep every sum exact."""
import numpy as np
import pytest

import fragment_ref as fr
from oracle import oracle_py as ora


@pytest.mark.parametrize("name", list(fr.Q3_CASES))
def test_q3_oracle_equals_reference(name):
    case = fr.q3_case(name)
    exp, nhits = fr.q3_ref(case)
    rows = ora.q3_partial(fr.q3_oracle_tables(ora, case),
                          segment=case["segment"], date=case["date"])
    got = fr.q3_rows_to_dict(rows)
    assert set(got) == set(exp)
    assert got == exp          # revenue, o_orderdate, o_shippriority
    assert nhits >= len(exp)


@pytest.mark.parametrize("name", list(fr.Q9_CASES))
def test_q9_oracle_equals_reference(name):
    case = fr.q9_case_get(name)
    exp = fr.q9_ref(case)
    rows = ora.q9_partial(fr.q9_oracle_tables(ora, case),
                          typemod=case["typemod"], typeval=case["typeval"])
    got = {int(r.year): (float(r.revenue), int(r.count_rows)) for r in rows}
    assert got == exp


def test_cases_reach_what_they_claim():
    """The catalogue's own claims, checked on the reference so that a
    builder edited into harmlessness fails here."""
    g, _ = fr.q3_ref(fr.q3_case("day0"))
    assert g[1][1:] == (0, 0)                       # payload packs to 0
    assert g[2][1:] == (-1, -1)                     # payload all ones
    assert {g[3][2], g[4][2]} == {fr.I32_MIN, fr.I32_MAX}
    g, _ = fr.q3_ref(fr.q3_case("day0_negative_date"))
    assert g and all(v[1] < -3 for v in g.values())
    g, _ = fr.q3_ref(fr.q3_case("zero_revenue"))
    assert sorted(g) == [1, 2, 3, 6, 7, 8, 9, 10, 12]   # 4, 5, 11 unmatched
    assert [g[k][0] for k in (1, 2, 6, 7, 9, 10, 12)] == [0.0] * 7
    assert g[3][0] == 75.0 and g[8][0] == 8.0
    g, _ = fr.q3_ref(fr.q3_case("negative_revenue"))
    revs = [v[0] for v in g.values()]
    assert min(revs) < 0 < max(revs) and 0.0 in revs
    g, _ = fr.q3_ref(fr.q3_case("key_domain"))
    assert {0, -1, -2**40, 2**31, fr.I64_MAX - 1} <= set(g)
    assert 2**62 not in g and 1 not in g  # customers 9 and 4 are not kept
    g, _ = fr.q3_ref(fr.q3_case("dense_tile"))
    assert len(g) == 70000
    g, _ = fr.q3_ref(fr.q3_case("date_bounds"))
    assert list(g) == [1] and g[1][0] == 12.0
    assert fr.q3_ref(fr.q3_case("no_cust_in_segment"))[0] == {}
    assert fr.q3_ref(fr.q3_case("broadcast_empty"))[0] == {}
    g, _ = fr.q3_ref(fr.q3_case("broadcast_dups"))
    assert g and len(g) < len(fr.q3_ref(fr.q3_case("all_cust_in_segment"))[0])
    for b in (0, 1, 2, 3, 4, 255):
        assert fr.q3_ref(fr.q3_case(f"segment_byte_{b}"))[0]
    y = fr.q9_ref(fr.q9_case_get("year_bounds"))
    assert sorted(y) == list(range(7))
    assert fr.q9_ref(fr.q9_case_get("type_none")) == {}
    assert fr.q9_ref(fr.q9_case_get("day0"))[0][1] > 0
    assert [fr.year_of_day(d) for d in fr.YEAR_STARTS] == list(range(7))
    assert [fr.year_of_day(d) for d in fr.YEAR_ENDS] == list(range(7))
    li = fr.q9_case_get("bad_partkeys")["lineitem"]
    assert {0, -1, 301, fr.I64_MAX} <= set(li["l_partkey"].tolist())
    assert np.all(np.sort(fr.q9_case_get("day0")["part"]["p_partkey"])
                  == np.arange(1, 301))

"""Plain references and hand-built tables for the fused Q3 and Q9-mix
fragments (helper module, imported by test_fragment_ref_host.py and
test_gpu_fragments_crafted.py).

Two things live here:

* q3_ref / q9_ref: brute-force restatements of the two fragments written
  from the SQL, with Python dict joins and math.fsum. They share no code
  with the C oracle or the kernels.
* Q3_CASES / Q9_CASES: named builders of small crafted table sets that aim
  at what the project's own generator never produces: day-0 orders, groups
  whose revenue sums to zero, key 0 and negative keys, unclustered
  lineitems, runs of equal keys that straddle the 4-row vector loads and the
  64-lane waves, dangling lineitems, empty and odd-sized tables.

Every price is an integer multiple of 4 below 2^20 and every discount comes
from {0, 0.25, 0.5, 0.75, 1.0} (1.5 only where a negative revenue is
wanted), so each term price * (1 - discount) is an integer and every group
sum is an integer below 2^53: float64 addition is then exact in any order,
and all results are compared with ==. Each builder asserts that on the CPU.
"""
import math
from collections import defaultdict

import numpy as np

I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MAX = 2**63 - 1

DATE = 1000          # default Q3 date parameter of the crafted cases
SEG = 1              # default Q3 segment
DISCS = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
YEAR_STARTS = [0, 366, 731, 1096, 1461, 1827, 2192]   # 1992 .. 1998
YEAR_ENDS = [365, 730, 1095, 1460, 1826, 2191, 2556]


def year_of_day(d):
    """Calendar year index of a day number, day 0 = 1992-01-01, with the
    real year lengths (1992 and 1996 are leap years)."""
    y = 0
    for i, start in enumerate(YEAR_STARTS):
        if d >= start:
            y = i
    return y


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------

def q3_kept_customers(case):
    """The customer key SET of the build side: the broadcast keys when the
    case carries them, else the keys of the customer rows in the segment."""
    if case["cust_keys"] is not None:
        return {int(k) for k in case["cust_keys"]}
    cu = case["customer"]
    return {int(k) for k, s in zip(cu["c_custkey"], cu["c_mktsegment"])
            if int(s) == case["segment"]}


def q3_ref(case):
    """-> (groups, nhits): groups maps l_orderkey to (revenue, o_orderdate,
    o_shippriority); a group exists iff at least one lineitem matched.
    nhits is the number of matched lineitems."""
    date = case["date"]
    kept = q3_kept_customers(case)
    od = case["orders"]
    orders = {}
    for ok, ck, d, p in zip(od["o_orderkey"], od["o_custkey"],
                            od["o_orderdate"], od["o_shippriority"]):
        if int(d) < date and int(ck) in kept:
            orders[int(ok)] = (int(d), int(p))
    li = case["lineitem"]
    terms = defaultdict(list)
    for ok, price, disc, sd in zip(li["l_orderkey"], li["l_extendedprice"],
                                   li["l_discount"], li["l_shipdate"]):
        if int(sd) > date and int(ok) in orders:
            terms[int(ok)].append(float(price) * (1.0 - float(disc)))
    groups = {ok: (math.fsum(v),) + orders[ok] for ok, v in terms.items()}
    return groups, sum(len(v) for v in terms.values())


def q9_ref(case):
    """-> {year index: (sum revenue, count)} over lineitem ⋈ part[p_type %
    typemod == typeval] ⋈ orders, grouped by the order's year."""
    pt = case["part"]
    parts = {int(k) for k, t in zip(pt["p_partkey"], pt["p_type"])
             if int(t) % case["typemod"] == case["typeval"]}
    od = case["orders"]
    odate = {int(k): int(d) for k, d in zip(od["o_orderkey"],
                                            od["o_orderdate"])}
    li = case["lineitem"]
    terms = defaultdict(list)
    for pk, ok, price, disc in zip(li["l_partkey"], li["l_orderkey"],
                                   li["l_extendedprice"], li["l_discount"]):
        if int(pk) in parts and int(ok) in odate:
            terms[year_of_day(odate[int(ok)])].append(
                float(price) * (1.0 - float(disc)))
    return {y: (math.fsum(v), len(v)) for y, v in terms.items()}


def q3_rows_to_dict(rows):
    """Structured Q3 group rows (oracle or GPU) -> {key: (rev, date, prio)};
    asserts that no key is emitted twice."""
    out = {int(r["l_orderkey"]): (float(r["revenue"]), int(r["o_orderdate"]),
                                  int(r["o_shippriority"])) for r in rows}
    assert len(out) == len(rows), "an l_orderkey was emitted twice"
    return out


def q3_oracle_tables(ora, case):
    """tables_from_numpy for a Q3 case. The oracle has no broadcast input:
    a case with cust_keys hands it those keys as an all-in-segment customer
    table, which is what the broadcast build side means."""
    cu = case["customer"]
    if case["cust_keys"] is not None:
        ck = np.asarray(case["cust_keys"], dtype=np.int64)
        cu = {"c_custkey": ck,
              "c_mktsegment": np.full(len(ck), case["segment"], np.uint8)}
    return ora.tables_from_numpy(lineitem=case["lineitem"],
                                 orders=case["orders"], customer=cu)


def q9_oracle_tables(ora, case):
    return ora.tables_from_numpy(lineitem=case["lineitem"],
                                 orders=case["orders"], part=case["part"])


# --------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------

def _check_exact(okeys, price, disc):
    """Every term is an integer and every per-key |sum| stays below 2^53, so
    float64 sums are exact whatever the order of the additions."""
    price = np.asarray(price, dtype=np.float64)
    disc = np.asarray(disc, dtype=np.float64)
    assert np.all(price >= 0) and np.all(price < 2**20)
    assert np.all(price == 4.0 * np.rint(price / 4.0))
    assert np.all(np.isin(disc, [0.0, 0.25, 0.5, 0.75, 1.0, 1.5]))
    term = price * (1.0 - disc)
    assert np.all(term == np.rint(term))
    sums = defaultdict(int)
    for k, t in zip(okeys, term):
        sums[int(k)] += abs(int(t))
    assert all(v < 2**53 for v in sums.values())
    assert int(np.abs(term).sum()) < 2**53


def _lineitem(okeys, price, disc, ship, partkey=None):
    n = len(okeys)
    li = {
        "l_orderkey": np.asarray(okeys, dtype=np.int64),
        "l_quantity": np.ones(n, dtype=np.float64),
        "l_extendedprice": np.asarray(price, dtype=np.float64),
        "l_discount": np.asarray(disc, dtype=np.float64),
        "l_tax": np.zeros(n, dtype=np.float64),
        "l_returnflag": np.full(n, ord("N"), dtype=np.uint8),
        "l_linestatus": np.full(n, ord("O"), dtype=np.uint8),
        "l_shipdate": np.asarray(ship, dtype=np.int32),
        "l_partkey": np.asarray(np.ones(n) if partkey is None else partkey,
                                dtype=np.int64),
    }
    assert all(len(v) == n for v in li.values())
    _check_exact(li["l_orderkey"], li["l_extendedprice"], li["l_discount"])
    return li


def _orders(okeys, ckeys, dates, prios):
    od = {"o_orderkey": np.asarray(okeys, dtype=np.int64),
          "o_custkey": np.asarray(ckeys, dtype=np.int64),
          "o_orderdate": np.asarray(dates, dtype=np.int32),
          "o_shippriority": np.asarray(prios, dtype=np.int32)}
    n = len(od["o_orderkey"])
    assert all(len(v) == n for v in od.values())
    assert len(set(od["o_orderkey"].tolist())) == n, "o_orderkey is unique"
    return od


def _customer(ckeys, segs):
    cu = {"c_custkey": np.asarray(ckeys, dtype=np.int64),
          "c_mktsegment": np.asarray(segs, dtype=np.uint8)}
    assert len(cu["c_custkey"]) == len(cu["c_mktsegment"])
    return cu


def _q3(customer, orders, lineitem, segment=SEG, date=DATE, cust_keys=None):
    return {"customer": customer, "orders": orders, "lineitem": lineitem,
            "segment": segment, "date": date,
            "cust_keys": None if cust_keys is None
            else np.asarray(cust_keys, dtype=np.int64)}


def _rand_lines(rng, okeys, date=DATE, p_after=0.8):
    """Random exact price/discount/shipdate columns for the given keys."""
    n = len(okeys)
    price = 4.0 * rng.integers(1, 2**18, n)
    disc = DISCS[rng.integers(0, 5, n)]
    ship = np.where(rng.random(n) < p_after, date + 1 + rng.integers(0, 50, n),
                    date - rng.integers(0, 50, n))
    return _lineitem(okeys, price, disc, ship)


ONE_CUST = _customer([7], [SEG])


def q3_day0(date):
    """Orders placed on day 0 with priority 0 (packed payload 0), the
    all-ones payload (date -1, priority -1), the int32 priority extremes
    and negative dates. With date = 10 the day-0 orders qualify; with date
    = -3 only the earlier negative dates do."""
    def build():
        dates = [0, -1, 0, 0, -7, I32_MIN, -100, 5, 0, 0, -4, -3, -2]
        prios = [0, -1, I32_MIN, I32_MAX, 3, 0, 0, 0, 0, 1, 0, 0, 0]
        n = len(dates)
        okeys = np.arange(1, n + 1)
        od = _orders(okeys, [7] * n, dates, prios)
        # 1..3 lineitems per order after the date, one before it
        lk, pr, dc, sh = [], [], [], []
        for i, k in enumerate(okeys):
            for j in range(1 + i % 3):
                lk.append(k); pr.append(4.0 * (10 * i + j + 1))
                dc.append(DISCS[(i + j) % 4]); sh.append(date + 1 + j)
            lk.append(k); pr.append(400.0); dc.append(0.0); sh.append(date)
        return _q3(ONE_CUST, od, _lineitem(lk, pr, dc, sh), date=date)
    return build


def q3_zero_revenue():
    """Groups whose revenue sums to exactly zero must be emitted; orders no
    lineitem matched must not. Matched and unmatched orders sit next to
    each other, so they share bitmap words and compaction quads."""
    rows = []   # (okey, price, disc, ship)
    A, B = DATE + 1, DATE       # after / not after the date
    rows += [(1, 40.0, 1.0, A), (1, 80.0, 1.0, A), (1, 4.0, 1.0, A)]  # disc 1
    rows += [(2, 0.0, 0.25, A), (2, 0.0, 0.0, A)]                # price 0
    rows += [(3, 100.0, 0.25, A), (3, 0.0, 0.5, A), (3, 8.0, 1.0, A)]  # mixed
    rows += [(4, 100.0, 0.0, B), (4, 44.0, 0.5, B - 1)]  # all fail the date
    # order 5: no lineitems at all
    rows += [(6, 64.0, 0.0, B), (6, 12.0, 1.0, A)]   # only the zero line hits
    rows += [(7, 8.0, 0.5, A), (7, 8.0, 1.5, A)]     # +4 and -4 cancel
    rows += [(8, 16.0, 0.5, A)]                      # ordinary neighbour
    rows += [(9, 0.0, 1.5, A)]                       # the term is -0.0
    rows += [(10, 0.0, 1.5, A), (10, 0.0, 0.0, A)]   # -0.0 + +0.0
    # order 11: no lineitems; order 12: one zero line in the tail rows
    rows += [(12, 4.0, 1.0, A)]
    od = _orders(np.arange(1, 13), [7] * 12, [DATE - 1] * 12, [0] * 12)
    k, p, d, s = zip(*rows)
    return _q3(ONE_CUST, od, _lineitem(k, p, d, s))


def q3_negative_revenue():
    """Discount 1.5 gives negative revenue: groups below zero, at zero and
    above it; the top-k has to rank the negative ones last."""
    rng = np.random.default_rng(11)
    n = 40
    od = _orders(np.arange(1, n + 1), [7] * n, DATE - 1 - np.arange(n) % 5,
                 [0] * n)
    lk = np.repeat(np.arange(1, n + 1), 3)
    price = 4.0 * rng.integers(0, 1000, len(lk))
    disc = np.where(lk % 3 == 0, 1.5, DISCS[rng.integers(0, 5, len(lk))])
    disc = np.where(lk % 5 == 0, 1.0, disc)
    return _q3(ONE_CUST, od, _lineitem(lk, price, disc,
                                       [DATE + 1] * len(lk)))


KEY_DOMAIN_OKEYS = [0, -1, -2**40, 2**31, 2**31 + 5, 2**62, I64_MAX - 1, 17,
                    1, -2**62]


def q3_key_domain():
    """Key 0, negative keys, keys past 2^31 (which void the int32 caches)
    and INT64_MAX - 1, on both the customer and the order side, with probe
    keys that are near misses of each. INT64_MIN, the one reserved key
    (otbx.h), is not used."""
    cu = _customer([0, -5, 2**31 + 7, 3, -2**50, 9], [1, 1, 1, 1, 1, 0])
    ck = [0, -5, 2**31 + 7, 3, -2**50, 9, 0, -5, 4, 0]   # 9: not in seg, 4: none
    n = len(KEY_DOMAIN_OKEYS)
    od = _orders(KEY_DOMAIN_OKEYS, ck, [DATE - 1 - i for i in range(n)],
                 list(range(n)))
    lk = []
    for k in KEY_DOMAIN_OKEYS:
        lk += [k, k]
    lk += [2, -3, I64_MAX, 2**31 + 4, -2**40 + 1, 16, 18]   # dangling
    lk = np.array(lk, dtype=np.int64)
    rng = np.random.default_rng(5)
    rng.shuffle(lk)
    price = 4.0 * rng.integers(1, 1000, len(lk))
    return _q3(cu, od, _lineitem(lk, price, DISCS[rng.integers(0, 4, len(lk))],
                                 [DATE + 1] * len(lk)))


def q3_key0_dense():
    """Dense keys that start at 0 on both sides: the direct tables are
    based at key 0."""
    rng = np.random.default_rng(6)
    cu = _customer(np.arange(10), [1, 0] * 5)
    od = _orders(np.arange(50), np.arange(50) % 10, [DATE - 1] * 50,
                 np.arange(50) % 3)
    lk = np.sort(rng.integers(-1, 51, 300))
    return _q3(cu, od, _rand_lines(rng, lk))


def q3_shuffled():
    """Lineitem rows in random order: no clustering by orderkey at all."""
    rng = np.random.default_rng(7)
    cu = _customer(np.arange(1, 51), rng.integers(0, 3, 50))
    od = _orders(rng.permutation(np.arange(1, 501)), rng.integers(1, 56, 500),
                 DATE - 20 + rng.integers(0, 40, 500), rng.integers(0, 4, 500))
    lk = rng.integers(1, 520, 2000)
    return _q3(cu, od, _rand_lines(rng, lk))


RUNS = [1, 2, 3, 5, 63, 64, 65, 200]


def q3_run_lengths(offset, gaps):
    """Clustered lineitems: runs of equal orderkey of the lengths in RUNS,
    twice over, the first run starting at row `offset`, so runs straddle
    the 4-row quads and the 64-lane waves. gaps: every 7th row fails the
    date, which breaks the runs up in the candidate list."""
    def build():
        nk = 2 * len(RUNS)
        od = _orders(np.arange(1, nk + 1), [7] * nk, [DATE - 1] * nk,
                     np.arange(nk) % 2)
        lk = [nk + 5] * offset            # dangling rows in front
        for i, r in enumerate(RUNS + RUNS[::-1]):
            lk += [i + 1] * r
        lk = np.array(lk)
        n = len(lk)
        price = 4.0 * (1 + np.arange(n) % 977)
        disc = DISCS[np.arange(n) % 5]
        ship = np.full(n, DATE + 1)
        if gaps:
            ship[::7] = DATE
        return _q3(ONE_CUST, od, _lineitem(lk, price, disc, ship))
    return build


def q3_dangling():
    """Lineitems whose order does not exist: below the smallest order key,
    above the largest, and inside the range in a gap."""
    okeys = list(range(10, 20)) + list(range(30, 40))
    od = _orders(okeys, [7] * 20, [DATE - 1] * 20, [0] * 20)
    lk = np.array([5, 9, 10, 19, 20, 25, 29, 30, 39, 40, 45, 10**6, 15, 35, 0])
    rng = np.random.default_rng(8)
    lk = np.concatenate([lk, rng.integers(0, 50, 200)])
    return _q3(ONE_CUST, od, _rand_lines(rng, lk, p_after=1.0))


def q3_date_bounds():
    """o_orderdate and l_shipdate each one below, at and one above the
    date: only (date - 1, date + 1) joins."""
    od = _orders([1, 2, 3], [7] * 3, [DATE - 1, DATE, DATE + 1], [0] * 3)
    lk, sh = [], []
    for k in (1, 2, 3):
        for s in (DATE - 1, DATE, DATE + 1):
            lk.append(k); sh.append(s)
    return _q3(ONE_CUST, od, _lineitem(lk, [4.0 * (i + 1) for i in range(9)],
                                       [0.0] * 9, sh))


def _cust_side_tables(rng, ncust=24):
    od = _orders(np.arange(1, 101), 1 + np.arange(100) % (ncust + 2),
                 [DATE - 1] * 100, np.arange(100) % 2)
    li = _rand_lines(rng, np.repeat(np.arange(1, 101), 2), p_after=1.0)
    return od, li


def q3_dup_custkeys():
    """Customer keys repeat, once with rows both in and out of the segment:
    the build side is a key set."""
    rng = np.random.default_rng(9)
    od, li = _cust_side_tables(rng)
    ck = np.concatenate([np.arange(1, 25), np.arange(1, 25), [3, 3, 3]])
    segs = np.concatenate([np.arange(24) % 2, (np.arange(24) // 2) % 2,
                           [1, 0, 1]])
    return _q3(_customer(ck, segs), od, li)


def q3_segments(segs, segment):
    def build():
        rng = np.random.default_rng(10)
        od, li = _cust_side_tables(rng)
        return _q3(_customer(np.arange(1, 25), np.resize(segs, 24)), od, li,
                   segment=segment)
    return build


def q3_broadcast(keys):
    """The broadcast build side: cust_keys replaces the local customer
    filter. The local table says "every customer is in the segment", so a
    run that ignored cust_keys would emit every order."""
    def build():
        rng = np.random.default_rng(12)
        od, li = _cust_side_tables(rng)
        return _q3(_customer(np.arange(1, 25), [SEG] * 24), od, li,
                   cust_keys=keys)
    return build


SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1025]


def q3_sizes(norders, nlineitem):
    """Table sizes around the 4-row quads and the 256-thread blocks, the two
    tables varied independently. About one lineitem in eight dangles."""
    def build():
        rng = np.random.default_rng(1000 * norders + nlineitem)
        od = _orders(rng.permutation(np.arange(1, norders + 1)),
                     1 + np.arange(norders) % 3,
                     DATE - 1 + (np.arange(norders) % 4 == 3), [0] * norders)
        cu = _customer([1, 2, 3], [SEG, SEG, 0])
        lk = np.sort(rng.integers(0, norders + max(norders // 8, 2),
                                  nlineitem))
        return _q3(cu, od, _rand_lines(rng, lk))
    return build


def q3_dense_tile():
    """70 000 orders with contiguous keys, all matching, one lineitem each:
    more than half of a 65 536-entry compaction tile survives, and the
    range crosses a tile boundary."""
    n = 70000
    keys = 1000 + np.arange(n)
    od = _orders(keys, [7] * n, DATE - 1 - np.arange(n) % 300,
                 np.arange(n) % 5)
    price = 4.0 * (1 + np.arange(n) % 50021)
    return _q3(ONE_CUST, od, _lineitem(keys, price, DISCS[np.arange(n) % 4],
                                       [DATE + 1] * n))


def q3_sparse(key_range):
    """1 000 orders spread over a wide key range: about 2e5 reaches the
    grace multi-pass direct path, about 3e6 the hash path, without any
    test hook."""
    def build():
        rng = np.random.default_rng(key_range)
        keys = 50 + rng.choice(key_range, 1000, replace=False)
        od = _orders(keys, 1 + np.arange(1000) % 3, [DATE - 1] * 1000,
                     np.arange(1000) % 2)
        cu = _customer([1, 2, 3], [SEG, SEG, 0])
        lk = np.concatenate([rng.choice(keys, 2500),
                             rng.integers(0, key_range + 100, 500)])
        return _q3(cu, od, _rand_lines(rng, np.sort(lk)))
    return build


Q3_CASES = {
    "day0": q3_day0(10),
    "day0_negative_date": q3_day0(-3),
    "zero_revenue": q3_zero_revenue,
    "negative_revenue": q3_negative_revenue,
    "key_domain": q3_key_domain,
    "key0_dense": q3_key0_dense,
    "shuffled": q3_shuffled,
    "runs_off1": q3_run_lengths(1, False),
    "runs_off2": q3_run_lengths(2, False),
    "runs_off3": q3_run_lengths(3, False),
    "runs_off1_gaps": q3_run_lengths(1, True),
    "dangling": q3_dangling,
    "date_bounds": q3_date_bounds,
    "dup_custkeys": q3_dup_custkeys,
    "no_cust_in_segment": q3_segments([0, 1], 3),
    "all_cust_in_segment": q3_segments([SEG], SEG),
    "broadcast_dups": q3_broadcast([2, 5, 5, 2, 11, 11, 11, 24, 30]),
    "broadcast_empty": q3_broadcast([]),
    "dense_tile": q3_dense_tile,
    "sparse_2e5": q3_sparse(200_000),
    "sparse_3e6": q3_sparse(3_000_000),
}
for _b in (0, 1, 2, 3, 4, 255):
    Q3_CASES[f"segment_byte_{_b}"] = q3_segments([0, 1, 2, 3, 4, 255], _b)
for _no in SIZES:
    for _nl in SIZES:
        Q3_CASES[f"sizes_{_no}_{_nl}"] = q3_sizes(_no, _nl)

# the cases whose keys leave [1, 2^63): they confirm the key-domain fix and
# have no meaning on code from before it
Q3_KEY_DOMAIN_CASES = ("key_domain", "key0_dense")


# ---- Q9 ----

def _q9(part, orders, lineitem, typemod=17, typeval=0):
    return {"part": part, "orders": orders, "lineitem": lineitem,
            "typemod": typemod, "typeval": typeval}


def _part(rng, n):
    """p_partkey is a shuffled permutation of 1..n."""
    return {"p_partkey": rng.permutation(np.arange(1, n + 1)).astype(np.int64),
            "p_type": rng.integers(0, 256, n).astype(np.uint8)}


def _q9_tables(seed, nparts=300, norders=64, nlineitem=1500, key_base=1,
               dates=None, typemod=17, typeval=0, partkeys=None):
    rng = np.random.default_rng(seed)
    pt = _part(rng, nparts)
    if dates is None:
        dates = rng.integers(0, 2557, norders)
    od = _orders(key_base + rng.permutation(norders), [1] * norders,
                 np.resize(dates, norders), [0] * norders)
    lk = key_base + rng.integers(-2, norders + 2, nlineitem)   # some dangle
    pk = rng.integers(1, nparts + 1, nlineitem) if partkeys is None \
        else np.resize(partkeys, nlineitem)
    price = 4.0 * rng.integers(1, 2**18, nlineitem)
    li = _lineitem(lk, price, DISCS[rng.integers(0, 5, nlineitem)],
                   [0] * nlineitem, partkey=pk)
    # the year sums are exact too
    assert int(np.abs(li["l_extendedprice"]).sum()) < 2**53
    return _q9(pt, od, li, typemod, typeval)


def q9_case(**kw):
    return lambda: _q9_tables(**kw)


def q9_bad_partkeys():
    """l_partkey 0, -1, n + 1 and INT64_MAX must not match any part."""
    nparts = 300
    rng = np.random.default_rng(31)
    pk = rng.integers(1, nparts + 1, 1500)
    pk[::5] = np.resize([0, -1, nparts + 1, I64_MAX], len(pk[::5]))
    return _q9_tables(seed=31, nparts=nparts, partkeys=pk, typemod=1)


Q9_CASES = {
    "day0": q9_case(seed=21, dates=[0, 0, 1, 400, 0, 2556], typemod=1),
    "year_bounds": q9_case(seed=22, norders=56,
                           dates=YEAR_STARTS + YEAR_ENDS, typemod=1),
    "bad_partkeys": q9_bad_partkeys,
    "type_all": q9_case(seed=23, typemod=1, typeval=0),
    "type_17_0": q9_case(seed=23, typemod=17, typeval=0),
    "type_255_254": q9_case(seed=23, typemod=255, typeval=254),
    "type_none": q9_case(seed=23, typemod=5, typeval=7),
    "okeys_from_0": q9_case(seed=24, key_base=0, typemod=3),
    "okeys_large_offset": q9_case(seed=25, key_base=2**40, typemod=3),
}
for _nl in (0, 1, 7, 8, 9, 1023, 1025):
    Q9_CASES[f"nlineitem_{_nl}"] = q9_case(seed=40 + _nl, nlineitem=_nl,
                                           typemod=2)

_built = {}


def q3_case(name):
    if ("q3", name) not in _built:
        _built["q3", name] = Q3_CASES[name]()
    return _built["q3", name]


def q9_case_get(name):
    if ("q9", name) not in _built:
        _built["q9", name] = Q9_CASES[name]()
    return _built["q9", name]

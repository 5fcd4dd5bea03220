"""Host side of the Q1 kernel tests: the small Q1-shaped table the crafted
cases start from, and a numpy reference of the partial aggregate
(otbx_q1_partial_variant) whose sums are exact to the last rounding."""
import math

import numpy as np


def host_cols(n, seed=7, money=False, **over):
    """A small Q1-shaped host table; keyword arguments replace columns.
    money: l_extendedprice in whole cents (the packed price column builds),
    otherwise uniform random doubles (it does not)."""
    rng = np.random.default_rng(seed)
    cols = {
        "l_quantity": rng.integers(1, 51, n).astype(np.float64),
        "l_extendedprice": (rng.integers(90_000, 10_500_001, n) / 100.0
                            if money else rng.uniform(900.0, 105000.0, n)),
        "l_discount": rng.integers(0, 11, n) / 100.0,
        "l_tax": rng.integers(0, 9, n) / 100.0,
        "l_returnflag": rng.choice(np.frombuffer(b"ANR", np.uint8), n),
        "l_linestatus": rng.choice(np.frombuffer(b"FO", np.uint8), n),
        "l_shipdate": rng.integers(0, 2526, n).astype(np.int32),
    }
    cols.update(over)
    return cols


def gid_of(rf, ls):
    """Group slot of a (l_returnflag, l_linestatus) pair, as the kernels
    compute it: unexpected bytes fall into the 'R' / 'O' slots."""
    ri = np.where(rf == ord("A"), 0, np.where(rf == ord("N"), 1, 2))
    return (ri * 2 + np.where(ls == ord("F"), 0, 1)).astype(np.uint32)


def ref_q1_partial(cols, cutoff):
    """(sums[6][5], counts[6]) over the rows with l_shipdate <= cutoff. The
    per-row projection is element-wise f64, unfused, as in the kernels:
    dp = p * (1 - d), ch = dp * (1 + t). Each sum is math.fsum of its terms
    (the exact sum, rounded once), the counts are np.bincount."""
    p, d, t = cols["l_extendedprice"], cols["l_discount"], cols["l_tax"]
    dp = p * (1.0 - d)
    ch = dp * (1.0 + t)
    terms = (cols["l_quantity"], p, dp, ch, d)
    gid = gid_of(cols["l_returnflag"], cols["l_linestatus"])
    keep = cols["l_shipdate"].astype(np.int64) <= cutoff
    sums = np.zeros((6, 5))
    for g in range(6):
        rows = keep & (gid == g)
        for s, x in enumerate(terms):
            sums[g, s] = math.fsum(x[rows])
    counts = np.bincount(gid[keep], minlength=6).astype(np.int64)
    return sums, counts

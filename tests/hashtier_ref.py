"""Reference results and case builders for the multi-key hash joins and hash
aggregates of include/otbx.h (a helper, not a test): otbx_join_i64_ext,
otbx_join_i64x2, otbx_join_i64n, otbx_agg_i64x2, otbx_agg_i64n and
otbx_agg_i64_dec. Written from the header's contract, not from the kernels.

ref_join(bcols, bnulls, pcols, pnulls, jt)
    bcols / pcols: one int64 array per key column (1..8), bnulls / pnulls:
    None or one uint8 mask (or None) per column. jt 0 inner, 1 left, 2 semi,
    3 anti, 4 right, 5 full. Returns the sorted list of (bidx, pidx) pairs in
    the header's encoding: a match is (b, p); an unmatched or NULL-key probe
    row of left/full and every semi/anti emission is (-1, p); an unmatched or
    NULL-key build row of right/full is (b, -1). A row with any NULL key
    matches nothing, whatever value is stored under the NULL.

ref_agg(keycols, keynulls, vals, valnulls)
    Returns {identity: {"count_star", "count_v", "sum", "first_row"}} with
    identity = ((isnull, 0 if isnull else key), ...) per key column, so NULL
    groups with NULL and the value under a NULL is ignored. sum is a Python
    float sum (row order) for float64 values and a Python int for int64
    values (the decimal variant); a group without a non-NULL value has
    count_v == 0, which is the operators' sum_isnull.

The case builders below return JoinCase / AggCase objects of numpy inputs and
are named for the kernel branch they are built to reach. They are memoised:
the host test and the GPU test share one object per case, its reference is
computed once, and nobody may modify it. The shapes that depend on the launch
geometry take it from opentenbase_amd/csrc: grid_for() in otbx_common.h caps
a grid at 2048 blocks of 256 threads, waves are 64 lanes, and a probe wave
buffers 512 pairs before it flushes. They are written down here as numbers;
nothing is imported from the library.

Every float64 value is integer-valued and every group's sum of magnitudes is
far below 2^53, so each association order of the additions is exact and the
GPU's atomic sums can be compared bit for bit. The one exception is the
+Inf / -Inf pair of case_agg_identity, compared by class (sum_class).
"""
import functools
import math
import struct

import numpy as np

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
SPECIALS = [INT64_MIN, INT64_MAX, -1, 0, 1, 5]

WAVE = 64                       # lanes per wave (otbx_common.h)
PAIR_BUF = 512                  # BUF of k_joinx_probe / k_joinn_probe
GRID_THREADS = 2048 * 256       # grid_for(): at most 2048 blocks x 256 threads
STRIDE_NP = GRID_THREADS + 64 + 37   # a full second-iteration wave + a ragged one
STRIDE_N = GRID_THREADS + 101

JOIN_TYPES = {"inner": 0, "left": 1, "semi": 2, "anti": 3, "right": 4,
              "full": 5}


# ---------------------------------------------------------------- references

def _masks(nulls, nk):
    if nulls is None:
        return [None] * nk
    assert len(nulls) == nk
    return list(nulls)


def _rows(cols, nulls):
    """[(key tuple, anynull)] per row, Python ints"""
    nk = len(cols)
    n = len(cols[0])
    keys = list(zip(*[np.asarray(c, dtype=np.int64).tolist() for c in cols]))
    anynull = np.zeros(n, dtype=bool)
    for m in _masks(nulls, nk):
        if m is not None:
            anynull |= np.asarray(m).astype(bool)
    return list(zip(keys, anynull.tolist()))


def ref_join(bcols, bnulls, pcols, pnulls, jt):
    assert 1 <= len(bcols) <= 8 and len(bcols) == len(pcols)
    assert 0 <= jt <= 5
    table = {}
    brows = _rows(bcols, bnulls)
    for b, (key, anynull) in enumerate(brows):
        if not anynull:
            table.setdefault(key, []).append(b)
    matched = set()
    out = []
    for p, (key, anynull) in enumerate(_rows(pcols, pnulls)):
        ms = [] if anynull else table.get(key, [])
        if jt in (0, 1, 4, 5):
            for b in ms:
                out.append((b, p))
        if jt in (4, 5):
            matched.update(ms)
        if jt in (1, 3, 5) and not ms:
            out.append((-1, p))
        if jt == 2 and ms:
            out.append((-1, p))
    if jt in (4, 5):
        out.extend((b, -1) for b in range(len(brows)) if b not in matched)
    out.sort()
    return out


def identity_of(keycols, keynulls, i):
    """group identity of row i"""
    out = []
    for c, m in zip(keycols, _masks(keynulls, len(keycols))):
        isnull = m is not None and bool(m[i])
        out.append((isnull, 0 if isnull else int(c[i])))
    return tuple(out)


def ref_agg(keycols, keynulls, vals, valnulls):
    nk = len(keycols)
    assert 1 <= nk <= 8
    vals = np.asarray(vals)
    exact = vals.dtype.kind == "i"
    n = len(vals)
    lists = [np.asarray(c, dtype=np.int64).tolist() for c in keycols]
    ms = [None if m is None else np.asarray(m).astype(bool).tolist()
          for m in _masks(keynulls, nk)]
    vl = vals.tolist()
    vn = None if valnulls is None else np.asarray(valnulls).astype(bool).tolist()
    groups = {}
    for i in range(n):
        ident = tuple(
            (True, 0) if (m is not None and m[i]) else (False, col[i])
            for col, m in zip(lists, ms))
        g = groups.get(ident)
        if g is None:
            g = groups[ident] = {"count_star": 0, "count_v": 0,
                                 "sum": 0 if exact else 0.0, "first_row": i}
        g["count_star"] += 1
        if not (vn is not None and vn[i]):
            g["count_v"] += 1
            g["sum"] = g["sum"] + vl[i]
    return groups


def sum_class(x):
    """'nan', '+inf', '-inf' or None for a finite value"""
    if isinstance(x, float):
        if math.isnan(x):
            return "nan"
        if math.isinf(x):
            return "+inf" if x > 0 else "-inf"
    return None


def same_sum(got, exp):
    """Python ints: equal. Floats: the same non-finite class, or the same 64
    bits."""
    if isinstance(exp, int) and not isinstance(exp, bool) and \
            isinstance(got, int):
        return got == exp
    got, exp = float(got), float(exp)
    if sum_class(exp) is not None or sum_class(got) is not None:
        return sum_class(got) == sum_class(exp)
    return struct.pack("<d", got) == struct.pack("<d", exp)


def block_counts(pairs, np_rows, block=WAVE):
    """(matches, fills) of each aligned block of probe rows in a reference
    pair list: matches are (b >= 0, p), fills are (-1, p)."""
    nblk = (np_rows + block - 1) // block
    matches, fills = [0] * nblk, [0] * nblk
    for b, p in pairs:
        if p < 0:
            continue
        if b >= 0:
            matches[p // block] += 1
        else:
            fills[p // block] += 1
    return matches, fills


# --------------------------------------------------------------------- cases

class JoinCase:
    """nk key columns per side; masks are None or a list with one uint8 array
    (or None) per column"""

    def __init__(self, name, bcols, pcols, bnulls=None, pnulls=None):
        self.name = name
        self.bcols = [np.ascontiguousarray(c, dtype=np.int64) for c in bcols]
        self.pcols = [np.ascontiguousarray(c, dtype=np.int64) for c in pcols]
        self.nk = len(self.bcols)
        assert len(self.pcols) == self.nk
        self.bnulls = self._m(bnulls)
        self.pnulls = self._m(pnulls)
        self.nb, self.np = len(self.bcols[0]), len(self.pcols[0])
        self._ref = {}

    def _m(self, nulls):
        if nulls is None or all(m is None for m in nulls):
            return None
        assert len(nulls) == self.nk
        return [None if m is None else np.ascontiguousarray(m, dtype=np.uint8)
                for m in nulls]

    def ref(self, jt):
        """ref_join of this case, computed once per join type"""
        if jt not in self._ref:
            self._ref[jt] = ref_join(self.bcols, self.bnulls, self.pcols,
                                     self.pnulls, jt)
        return self._ref[jt]


class AggCase:
    def __init__(self, name, keycols, vals, keynulls=None, valnulls=None):
        self.name = name
        self.keycols = [np.ascontiguousarray(c, dtype=np.int64)
                        for c in keycols]
        self.nk = len(self.keycols)
        self.vals = np.ascontiguousarray(vals)
        assert self.vals.dtype in (np.float64, np.int64)
        if keynulls is None or all(m is None for m in keynulls):
            self.keynulls = None
        else:
            self.keynulls = [None if m is None else
                             np.ascontiguousarray(m, dtype=np.uint8)
                             for m in keynulls]
        self.valnulls = None if valnulls is None else \
            np.ascontiguousarray(valnulls, dtype=np.uint8)
        self.n = len(self.vals)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = ref_agg(self.keycols, self.keynulls, self.vals,
                                self.valnulls)
        return self._ref

    def identity(self, i):
        return identity_of(self.keycols, self.keynulls, i)


def _key_columns(ids, nk):
    """nk columns whose row tuples are distinct for distinct non-negative
    ids: column 0 alone for nk == 1, (id // 8, id % 8) for nk == 2, and a
    third column that repeats information for nk == 3."""
    ids = np.asarray(ids, dtype=np.int64)
    if nk == 1:
        return [ids * 3 - 50]
    cols = [ids // 8, ids % 8]
    if nk == 3:
        cols.append(-ids)
    return cols


@functools.lru_cache(maxsize=None)
def case_midwalk_flush(nk):
    """Every 64-row probe wave finds 64 x 16 = 1024 pairs, twice the 512-pair
    buffer: the flush inside the slot walk runs. 64 distinct keys with 16
    build copies each, shuffled; probe row i carries key i % 64."""
    rng = np.random.default_rng(101)
    bid = rng.permutation(np.repeat(np.arange(64), 16))
    pid = np.arange(128) % 64
    return JoinCase(f"midwalk_flush_nk{nk}", _key_columns(bid, nk),
                    _key_columns(pid, nk))


@functools.lru_cache(maxsize=None)
def case_fill_flush(nk, with_nulls=False):
    """One 64-row probe wave: rows 0..30 match 16 build copies each (496
    pairs, below the 512-pair buffer, so the walk does not flush), rows
    31..63 match nothing (33 fills): the buffer overflows when the fills are
    appended. The build side also holds 24 rows no probe row matches. With
    with_nulls, eleven of the non-matching rows are NULL-key rows instead
    whose stored key exists on the build side, and two build rows are NULL
    over a probed key."""
    rng = np.random.default_rng(102)
    bid = rng.permutation(np.concatenate([np.repeat(np.arange(31), 16),
                                          np.arange(200, 224)]))
    pid = np.concatenate([np.arange(31), np.arange(100, 133)])
    bcols, pcols = _key_columns(bid, nk), _key_columns(pid, nk)
    bnulls = pnulls = None
    if with_nulls:
        pnulls = [np.zeros(64, np.uint8) for _ in range(nk)]
        for j, r in enumerate(range(40, 51)):
            for c in range(nk):
                pcols[c][r] = _key_columns([j], nk)[c][0]   # a build key
            pnulls[j % nk][r] = 1
        bnulls = [np.zeros(len(bid), np.uint8) for _ in range(nk)]
        extra = np.flatnonzero(bid >= 200)[:2]
        for j, r in enumerate(extra):
            for c in range(nk):
                bcols[c][r] = _key_columns([j], nk)[c][0]   # a probed key
            bnulls[(nk - 1) if j else 0][r] = 1
    return JoinCase(f"fill_flush_nk{nk}{'_nulls' if with_nulls else ''}",
                    bcols, pcols, bnulls, pnulls)


@functools.lru_cache(maxsize=None)
def case_join_grid_stride(nk):
    """More probe rows than the largest grid has threads (2048 x 256): the
    first waves run a second loop iteration with pairs still buffered from
    the first, one wave's second iteration is ragged (37 rows), and the rest
    leave through the all-lanes-out-of-range exit. 1500 build rows over 1000
    distinct keys; a third of the probe keys are absent; NULLs on both
    sides."""
    rng = np.random.default_rng(103)
    nb = 1500
    bid = rng.permutation(np.concatenate([np.arange(1000),
                                          rng.integers(0, 1000, nb - 1000)]))
    pid = rng.integers(0, 1500, STRIDE_NP)
    bcols, pcols = _key_columns(bid, nk), _key_columns(pid, nk)
    bnulls = [None] * nk
    pnulls = [None] * nk
    bnulls[nk - 1] = (rng.random(nb) < 0.05).astype(np.uint8)
    pnulls[0] = (rng.random(STRIDE_NP) < 0.02).astype(np.uint8)
    return JoinCase(f"join_grid_stride_nk{nk}", bcols, pcols, bnulls, pnulls)


OVERFLOW_CAP = 300      # cap_pairs of the overflow tests


@functools.lru_cache(maxsize=None)
def case_overflow(nk):
    """Far more pairs than OVERFLOW_CAP for an inner join (2048 matches) and
    a full join (plus probe and build fills, NULL keys among them)."""
    rng = np.random.default_rng(104)
    bid = rng.permutation(np.concatenate([np.repeat(np.arange(64), 16),
                                          np.arange(300, 340)]))
    pid = np.concatenate([np.arange(128) % 64, np.arange(400, 464)])
    bcols, pcols = _key_columns(bid, nk), _key_columns(pid, nk)
    bnulls = [None] * nk
    pnulls = [None] * nk
    bnulls[0] = (rng.random(len(bid)) < 0.03).astype(np.uint8)
    pnulls[nk - 1] = (rng.random(len(pid)) < 0.05).astype(np.uint8)
    return JoinCase(f"overflow_nk{nk}", bcols, pcols, bnulls, pnulls)


X2_MASKS = ["b1", "b2", "p1", "p2", "all"]


@functools.lru_cache(maxsize=None)
def case_null_placement_x2(mask):
    """Two-key join at 200 rows per side. Both sides hold every pair of
    SPECIALS x SPECIALS (so (a, b) and (b, a), INT64_MIN, INT64_MAX, -1 and
    0), which makes the value stored under any NULL one that would match.
    mask names the column(s) that carry a 15 % NULL mask."""
    assert mask in X2_MASKS
    rng = np.random.default_rng(105 + X2_MASKS.index(mask))
    sp = np.array(SPECIALS, dtype=np.int64)
    n = 200

    def side():
        grid = np.array([(a, b) for a in SPECIALS for b in SPECIALS],
                        dtype=np.int64)
        rest = sp[rng.integers(0, len(sp), (n - len(grid), 2))]
        rows = rng.permutation(np.concatenate([grid, rest]))
        return [rows[:, 0].copy(), rows[:, 1].copy()]

    def m():
        return (rng.random(n) < 0.15).astype(np.uint8)

    bnulls = [m() if mask in ("b1", "all") else None,
              m() if mask in ("b2", "all") else None]
    pnulls = [m() if mask in ("p1", "all") else None,
              m() if mask in ("p2", "all") else None]
    return JoinCase(f"null_x2_{mask}", side(), side(), bnulls, pnulls)


@functools.lru_cache(maxsize=None)
def case_null_placement_n(nk):
    """N-key join (nk in 1, 2, 8) at 200 rows per side with NULL masks on
    the LAST build column and on probe columns 0 and nk - 1. For nk == 8
    most rows are identical in columns 0..6 and differ only in column 7; a
    few differ in column 0 only. Key values are SPECIALS, so every value
    under a NULL would match."""
    assert nk in (1, 2, 8)
    rng = np.random.default_rng(110 + nk)
    sp = np.array(SPECIALS, dtype=np.int64)
    n = 200

    def side():
        cols = []
        for c in range(nk):
            if c == nk - 1:
                col = sp[np.arange(n) % len(sp)]
                cols.append(rng.permutation(col))
            elif nk == 8:
                col = np.full(n, SPECIALS[c % len(SPECIALS)], dtype=np.int64)
                if c == 0:
                    col[rng.random(n) < 0.2] = 7
                cols.append(col)
            else:
                cols.append(sp[rng.integers(0, len(sp), n)])
        return cols

    bnulls = [None] * nk
    pnulls = [None] * nk
    bnulls[nk - 1] = (rng.random(n) < 0.15).astype(np.uint8)
    pnulls[nk - 1] = (rng.random(n) < 0.1).astype(np.uint8)
    pnulls[0] = (rng.random(n) < 0.1).astype(np.uint8) if nk > 1 \
        else pnulls[0]
    return JoinCase(f"null_n_nk{nk}", side(), side(), bnulls, pnulls)


EMPTY_SIDES = ["build", "probe", "both"]


@functools.lru_cache(maxsize=None)
def case_empty(nk, which):
    """nb == 0, np == 0 or both; the other side has 50 rows with NULL keys
    among them."""
    assert which in EMPTY_SIDES
    rng = np.random.default_rng(120 + nk)
    ids = rng.integers(0, 20, 50)
    full = _key_columns(ids, nk)
    fullnull = [None] * nk
    fullnull[nk - 1] = (rng.random(50) < 0.2).astype(np.uint8)
    empty = [np.empty(0, np.int64) for _ in range(nk)]
    if which == "build":
        return JoinCase(f"empty_build_nk{nk}", empty, full, None, fullnull)
    if which == "probe":
        return JoinCase(f"empty_probe_nk{nk}", full, empty, fullnull, None)
    return JoinCase(f"empty_both_nk{nk}", empty, empty)


@functools.lru_cache(maxsize=None)
def case_agg_empty(nk, dec=False):
    return AggCase(f"agg_empty_nk{nk}{'_dec' if dec else ''}",
                   [np.empty(0, np.int64) for _ in range(nk)],
                   np.empty(0, np.int64 if dec else np.float64))


@functools.lru_cache(maxsize=None)
def case_agg_grid_stride(dec=False):
    """More rows than the largest grid has threads (2048 x 256): the build
    loops run a second, ragged iteration. About 3000 groups; NULL keys and
    NULL values. Two key columns and float64 values for agg_i64x2 /
    agg_i64n; one key column and int64 values spread over +-2^62 for the
    decimal variant."""
    rng = np.random.default_rng(130 + int(dec))
    n = STRIDE_N
    vn = (rng.random(n) < 0.1).astype(np.uint8)
    if dec:
        k = rng.integers(-5, 3000, n)
        kn = (rng.random(n) < 0.01).astype(np.uint8)
        v = rng.integers(-2**62, 2**62, n)
        return AggCase("agg_grid_stride_dec", [k], v, [kn], vn)
    k1 = rng.integers(-3, 57, n)
    k2 = rng.integers(0, 50, n)
    n1 = (rng.random(n) < 0.02).astype(np.uint8)
    n2 = (rng.random(n) < 0.02).astype(np.uint8)
    v = rng.integers(-1000, 1001, n).astype(np.float64)
    return AggCase("agg_grid_stride", [k1, k2], v, [n1, n2], vn)


@functools.lru_cache(maxsize=None)
def case_agg_identity(nk):
    """Group identity at 400 rows, nk in (2, 8). The two interesting columns
    are the first and the last; for nk == 8 columns 1..6 are constant, so
    rows differ only in column 0 or only in column 7. Holds (NULL, 5),
    (5, NULL), (NULL, NULL), (0, 0) and (NULL, 0) as five groups, different
    garbage under each NULL, INT64_MIN / INT64_MAX / -1 as ordinary keys, a
    group whose values are all NULL (key (1, 1)), a group holding +Inf and
    -Inf (key (2, 2)) and one holding +Inf only (key (3, 3))."""
    assert nk in (2, 8)
    rng = np.random.default_rng(140 + nk)
    heads = [(None, 5), (5, None), (None, None), (0, 0), (None, 0),
             (INT64_MIN, INT64_MAX), (INT64_MAX, INT64_MIN), (-1, -1),
             (-1, 0), (0, -1), (INT64_MIN, INT64_MIN), (INT64_MAX, -1),
             (5, 5), (1, 1), (2, 2), (3, 3)]
    n = 400
    pick = np.concatenate([np.arange(len(heads)),
                           rng.integers(0, len(heads), n - len(heads))])
    pick = rng.permutation(pick)
    a = np.zeros(n, np.int64)
    b = np.zeros(n, np.int64)
    an = np.zeros(n, np.uint8)
    bn = np.zeros(n, np.uint8)
    garbage = np.array(SPECIALS + [5, 0, 7777], dtype=np.int64)
    for i, h in enumerate(pick):
        x, y = heads[h]
        if x is None:
            an[i] = 1
            a[i] = garbage[rng.integers(0, len(garbage))]
        else:
            a[i] = x
        if y is None:
            bn[i] = 1
            b[i] = garbage[rng.integers(0, len(garbage))]
        else:
            b[i] = y
    v = rng.integers(-1000, 1001, n).astype(np.float64)
    vn = (rng.random(n) < 0.2).astype(np.uint8)
    h11, h22, h33 = heads.index((1, 1)), heads.index((2, 2)), \
        heads.index((3, 3))
    vn[pick == h11] = 1
    r22 = np.flatnonzero(pick == h22)
    r33 = np.flatnonzero(pick == h33)
    assert len(r22) >= 2 and len(r33) >= 1
    vn[r22[:2]] = 0
    v[r22[0]], v[r22[1]] = np.inf, -np.inf
    vn[r33[0]] = 0
    v[r33[0]] = np.inf
    if nk == 2:
        return AggCase("agg_identity_nk2", [a, b], v, [an, bn], vn)
    cols = [a] + [np.full(n, SPECIALS[c % len(SPECIALS)], dtype=np.int64)
                  for c in range(1, 7)] + [b]
    nulls = [an] + [None] * 6 + [bn]
    return AggCase("agg_identity_nk8", cols, v, nulls, vn)


@functools.lru_cache(maxsize=None)
def case_agg_bounded(ngroups, dec=False):
    """20000 rows over about ngroups groups for the bounded first attempt of
    the aggregates (OTBX_NK_FORCE_CAP): with a 16-slot first table and 5000
    groups the attempt must abort and rerun; with 4096 slots and 100 groups
    it succeeds."""
    rng = np.random.default_rng(150 + ngroups % 97 + int(dec))
    n = 20000
    vn = (rng.random(n) < 0.1).astype(np.uint8)
    if dec:
        k = rng.integers(0, ngroups, n)
        kn = (rng.random(n) < 0.01).astype(np.uint8)
        v = rng.integers(-2**62, 2**62, n)
        return AggCase(f"agg_bounded_dec_{ngroups}", [k], v, [kn], vn)
    side = max(int(round(math.sqrt(ngroups))), 1)
    k1 = rng.integers(0, side, n)
    k2 = rng.integers(0, (ngroups + side - 1) // side, n)
    n1 = (rng.random(n) < 0.01).astype(np.uint8)
    v = rng.integers(-1000, 1001, n).astype(np.float64)
    return AggCase(f"agg_bounded_{ngroups}", [k1, k2], v, [n1, None], vn)


DEC_CARRY_LISTS = [
    [-1, 1],                                # borrow, then carry back
    [1, -1],
    [INT64_MIN] * 4,
    [INT64_MAX, 1],                         # crosses 2^63
    [-1] * 3,
    [INT64_MAX, INT64_MAX, 2],              # exactly 2^64
    [INT64_MIN, INT64_MIN],                 # exactly -2^64
    [INT64_MIN, INT64_MAX] * 500,           # 1000 rows, sum -500
]


@functools.lru_cache(maxsize=None)
def case_dec_carry():
    """One group per list of DEC_CARRY_LISTS (key = list index, rows in list
    order), each with two NULL-value rows mixed in, after the first value
    and at the end, that store INT64_MAX and INT64_MIN under the NULL."""
    keys, vals, vn = [], [], []
    for g, lst in enumerate(DEC_CARRY_LISTS):
        keys += [g] * (len(lst) + 2)
        vals += lst[:1] + [INT64_MAX] + lst[1:] + [INT64_MIN]
        vn += [0, 1] + [0] * (len(lst) - 1) + [1]
    return AggCase("dec_carry", [np.array(keys, dtype=np.int64)],
                   np.array(vals, dtype=np.int64), None,
                   np.array(vn, dtype=np.uint8))

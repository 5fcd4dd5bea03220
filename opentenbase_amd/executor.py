"""Host-side mirror of the reference's CustomScan provider contract.

The reference drives a custom executor node through CustomExecMethods
(include/nodes/extensible.h:117-152; nodeCustom.c:31-125):
BeginCustomScan(estate, eflags) → repeated ExecCustomScan(node) returning one
tuple per call (None = done) → ReScanCustomScan → EndCustomScan. The classes
here keep those names, argument meanings and the error convention (OtbxError ↔
ereport(ERROR)) so the parity tests read like the reference's node lifecycle;
INTEGRATION.md shows the C provider these map onto.

Device memory, streams: torch (plumbing only — all compute is in libotbx.so;
there is NO torch/CPU fallback for any operator here).
"""
import ctypes as C
import math

import torch

from ._lib import (AGG_FUNCS, FB_CURRENT, FB_OFFSET, FB_UNBOUNDED,
                   FRAME_RANGE, FRAME_ROWS, MAX_AGGS, MAX_TEXT_CONST,
                   MAX_TEXT_RANK_COLS, MAX_WINCALLS, OAGG_FUNCS, TEXT_ENCODINGS,
                   TXT_OPS, WIN_FUNCS, AggCallsDev, CustomerDev, ExprDev,
                   FrameDev, KeysetDev, LineitemDev, OAggCallsDev, OrdersDev,
                   OtbxError, PartDev,
                   Q1_DICT_MAX, Q1CodeDesc, Q1PriceDesc, QualDev, SortSpecDev,
                   TextColDev, TextPredDev, TextSetDev, WinCallDev,
                   WindowOutDev, call, check, lib)

Q1_SLOT_ORDER = [(b"A", b"F"), (b"A", b"O"), (b"N", b"F"),
                 (b"N", b"O"), (b"R", b"F"), (b"R", b"O")]
Q1_CUTOFF_DEFAULT = 2436   # date '1998-12-01' - interval '90 day'
Q3_DATE_DEFAULT = 1169     # date '1995-03-15'
SEED_DEFAULT = 42


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def init_device(device=0):
    torch.cuda.set_device(device)
    call("otbx_init", device)


def device_synchronize():
    torch.cuda.synchronize()


# ---------------- staged tables (device-resident column cache) -------------

def _build_key32(src_tensor, src_ptr=None):
    """Staging-time compact-key cache (otbx.h otbx_build_key32): int32 copy
    of an i64 key column, or None if any key falls outside [0, 2^31)."""
    n = src_tensor.numel()
    dst = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    ok = C.c_int32(0)
    call("otbx_build_key32",
         C.c_void_p(src_ptr or src_tensor.data_ptr()), C.c_int64(n),
         C.c_void_p(dst.data_ptr()), C.byref(ok), _stream())
    return dst if ok.value else None


class _Col:
    """Device column of n rows: .t is the n-row tensor, .ptr its address.
    An empty table still gets a one-element allocation behind it, because
    the C-ABI reads a NULL column pointer as "not staged" (and torch gives
    an empty tensor a NULL data_ptr)."""

    def __init__(self, n, dtype, device="cuda"):
        self.base = torch.empty(max(n, 1), dtype=dtype, device=device)
        self.t = self.base[:n]
        self.ptr = self.base.data_ptr()


def _h2d_cols(t, cols):
    """Copy host columns (dict of numpy arrays keyed like t.t) into the
    staged table's device columns: the otbx_stage_table flow of
    GpuLineitem.from_host. An absent device column (None) is skipped."""
    import numpy as np
    for name, dst in t.t.items():
        if dst is None:
            continue
        src = np.ascontiguousarray(
            cols[name], dtype=torch.empty(0, dtype=dst.dtype).numpy().dtype)
        assert len(src) == t.n, (name, len(src), t.n)
        if src.nbytes:
            call("otbx_memcpy_h2d", C.c_void_p(dst.data_ptr()),
                 src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes),
                 _stream())
    call("otbx_stream_sync", _stream())  # host buffers may be freed


class GpuLineitem:
    COLS = [("l_orderkey", torch.int64), ("l_quantity", torch.float64),
            ("l_extendedprice", torch.float64), ("l_discount", torch.float64),
            ("l_tax", torch.float64), ("l_returnflag", torch.uint8),
            ("l_linestatus", torch.uint8), ("l_shipdate", torch.int32),
            ("l_partkey", torch.int64)]

    def __init__(self, n, with_orderkey=True, with_partkey=False,
                 device="cuda"):
        self.n = n
        self.t = {}
        self._cols = {}
        for name, dt in self.COLS:
            if (name == "l_orderkey" and not with_orderkey) or                (name == "l_partkey" and not with_partkey):
                self.t[name] = None
                continue
            self._cols[name] = _Col(n, dt, device)
            self.t[name] = self._cols[name].t
        self.cstruct = LineitemDev(
            n=n, **{k: C.c_void_p(0 if v is None else self._cols[k].ptr)
                    for k, v in self.t.items()})

    @classmethod
    def generate(cls, n_global, rank=0, nranks=1, seed=SEED_DEFAULT,
                 with_orderkey=True, with_partkey=False):
        t = cls(n_global // nranks, with_orderkey=with_orderkey,
                with_partkey=with_partkey)
        call("otbx_gen_lineitem_dev", C.byref(t.cstruct), C.c_uint64(seed),
             C.c_int64(n_global), C.c_uint32(rank), C.c_uint32(nranks),
             _stream())
        t._stage_caches()
        return t

    @classmethod
    def from_host(cls, cols, with_orderkey=True, with_partkey=False):
        """The real otbx_stage_table flow: host columnar
        arrays (the provider's heap→SoA staging output) → device column
        cache via otbx_memcpy_h2d. cols: dict of numpy arrays keyed like
        COLS. Returns the staged table; PCIe-inclusive, one-time."""
        n = len(cols["l_shipdate"])
        t = cls(n, with_orderkey=with_orderkey, with_partkey=with_partkey)
        _h2d_cols(t, cols)
        t._stage_caches()
        return t

    def _stage_caches(self):
        """Staging-time derived layouts (built once, outside any timed
        region, like the zone-map metadata): the int32 compact-key cache
        (otbx.h l_orderkey32) and, when partkey is staged, the Q9
        probe-side AoS record cache (otbx.h q9rec); and, whenever the Q1
        columns are staged and their value domains fit, the packed Q1 code
        column (otbx.h q1code) that Q1 streams instead of the raw columns."""
        self._stage_q1codes()
        if self.t.get("l_orderkey") is not None:
            self._okey32 = _build_key32(self.t["l_orderkey"],
                                        self._cols["l_orderkey"].ptr)
            if self._okey32 is not None:
                self.cstruct.l_orderkey32 = C.c_void_p(
                    self._okey32.data_ptr())
        if self.t.get("l_partkey") is not None:
            self._pkey32 = _build_key32(self.t["l_partkey"],
                                        self._cols["l_partkey"].ptr)
            if self._pkey32 is not None:
                self.cstruct.l_partkey32 = C.c_void_p(
                    self._pkey32.data_ptr())
        if self.t.get("l_partkey") is None or self.t.get("l_orderkey") is None:
            return
        self._q9rec = torch.empty(max(self.n, 1) * 32, dtype=torch.uint8,
                                  device="cuda")
        self.cstruct.q9rec = C.c_void_p(self._q9rec.data_ptr())
        call("otbx_build_q9recs", C.byref(self.cstruct),
             C.c_void_p(self._q9rec.data_ptr()), _stream())

    Q1_COLS = ("l_quantity", "l_extendedprice", "l_discount", "l_tax",
               "l_returnflag", "l_linestatus", "l_shipdate")

    def _stage_q1codes(self):
        """Build the packed Q1 code column (otbx_build_q1codes). The struct
        fields are set only when the build reports success; otherwise
        q1code stays NULL and otbx_q1_partial reads the raw columns. After a
        successful build the packed price column (otbx_build_q1pcodes)
        follows by the same rule."""
        self._q1code = self._q1dict = self._q1pcode = None
        if self.n == 0 or any(self.t.get(c) is None for c in self.Q1_COLS):
            return
        codes = torch.empty(self.n, dtype=torch.int32, device="cuda")
        qdict = torch.empty(3 * Q1_DICT_MAX, dtype=torch.int64, device="cuda")
        desc = Q1CodeDesc()
        ok = C.c_int32(0)
        call("otbx_build_q1codes", C.byref(self.cstruct),
             C.c_void_p(codes.data_ptr()), C.c_void_p(qdict.data_ptr()),
             C.byref(desc), C.byref(ok), _stream())
        if not ok.value:
            return
        self._q1code, self._q1dict = codes, qdict   # keep the tensors alive
        self.cstruct.q1desc = desc
        self.cstruct.q1code = C.c_void_p(codes.data_ptr())
        # the packed price column (otbx.h q1pcode) is only used next to the
        # code column: 8 B/row instead of 12 when l_extendedprice is money
        pcodes = torch.empty(self.n, dtype=torch.int32, device="cuda")
        pdesc = Q1PriceDesc()
        ok = C.c_int32(0)
        call("otbx_build_q1pcodes", C.byref(self.cstruct),
             C.c_void_p(pcodes.data_ptr()), C.byref(pdesc), C.byref(ok),
             _stream())
        if not ok.value:
            return
        self._q1pcode = pcodes
        self.cstruct.q1pdesc = pdesc
        self.cstruct.q1pcode = C.c_void_p(pcodes.data_ptr())

    def bytes_staged(self):
        """HBM held by the table: the columns plus every derived cache."""
        caches = [getattr(self, a, None) for a in
                  ("_q9rec", "_okey32", "_pkey32", "_q1code", "_q1dict",
                   "_q1pcode")]
        return sum(v.numel() * v.element_size()
                   for v in list(self.t.values()) + caches if v is not None)


class GpuOrders:
    def __init__(self, n, device="cuda"):
        self.n = n
        self._cols = {
            "o_orderkey": _Col(n, torch.int64, device),
            "o_custkey": _Col(n, torch.int64, device),
            "o_orderdate": _Col(n, torch.int32, device),
            "o_shippriority": _Col(n, torch.int32, device),
        }
        self.t = {k: c.t for k, c in self._cols.items()}
        self.cstruct = OrdersDev(
            n=n, **{k: C.c_void_p(c.ptr) for k, c in self._cols.items()})

    @classmethod
    def generate(cls, n_global, ncust_global, rank=0, nranks=1,
                 seed=SEED_DEFAULT, skew=False):
        t = cls(n_global // nranks)
        call("otbx_gen_orders_dev", C.byref(t.cstruct), C.c_uint64(seed),
             C.c_int64(n_global), C.c_int64(ncust_global), C.c_uint32(rank),
             C.c_uint32(nranks), C.c_int(1 if skew else 0), _stream())
        t._stage_key32()
        return t

    @classmethod
    def from_host(cls, cols, minmax=True):
        """Stage an orders table from host columns (dict of numpy arrays:
        o_orderkey, o_custkey, o_orderdate, o_shippriority), as
        GpuLineitem.from_host does. minmax=True fills the zone-map metadata
        (okey_min/okey_max/has_minmax) from the host column, the way a
        provider computes it while walking pages; minmax=False leaves
        has_minmax = 0, so the fragments run their own minmax kernel."""
        import numpy as np
        t = cls(len(cols["o_orderkey"]))
        _h2d_cols(t, cols)
        if minmax and t.n > 0:
            ok = np.asarray(cols["o_orderkey"], dtype=np.int64)
            t.cstruct.okey_min = int(ok.min())
            t.cstruct.okey_max = int(ok.max())
            t.cstruct.has_minmax = 1
        t._stage_key32()
        return t

    def _stage_key32(self):
        self._okey32 = _build_key32(self.t["o_orderkey"],
                                    self._cols["o_orderkey"].ptr)
        self._ckey32 = _build_key32(self.t["o_custkey"],
                                    self._cols["o_custkey"].ptr)
        if self._okey32 is not None:
            self.cstruct.o_orderkey32 = C.c_void_p(self._okey32.data_ptr())
        if self._ckey32 is not None:
            self.cstruct.o_custkey32 = C.c_void_p(self._ckey32.data_ptr())


class GpuCustomer:
    def __init__(self, n, device="cuda"):
        self.n = n
        self._cols = {
            "c_custkey": _Col(n, torch.int64, device),
            "c_mktsegment": _Col(n, torch.uint8, device),
        }
        self.t = {k: c.t for k, c in self._cols.items()}
        self.cstruct = CustomerDev(
            n=n, **{k: C.c_void_p(c.ptr) for k, c in self._cols.items()})

    @classmethod
    def generate(cls, n_global, rank=0, nranks=1, seed=SEED_DEFAULT):
        t = cls(n_global // nranks)
        call("otbx_gen_customer_dev", C.byref(t.cstruct), C.c_uint64(seed),
             C.c_int64(n_global), C.c_uint32(rank), C.c_uint32(nranks),
             _stream())
        return t

    @classmethod
    def from_host(cls, cols):
        """Stage a customer table from host columns (c_custkey,
        c_mktsegment)."""
        t = cls(len(cols["c_custkey"]))
        _h2d_cols(t, cols)
        return t


class GpuPart:
    """Replicated dimension table (every rank holds all rows — the locator
    'R' / replicated-relation case of the reference's shard layout)."""

    def __init__(self, n, device="cuda"):
        self.n = n
        self._cols = {
            "p_partkey": _Col(n, torch.int64, device),
            "p_type": _Col(n, torch.uint8, device),
        }
        self.t = {k: c.t for k, c in self._cols.items()}
        self.cstruct = PartDev(
            n=n, **{k: C.c_void_p(c.ptr) for k, c in self._cols.items()})

    @classmethod
    def generate(cls, n_global, seed=SEED_DEFAULT):
        t = cls(n_global)
        call("otbx_gen_part_dev", C.byref(t.cstruct), C.c_uint64(seed),
             C.c_int64(n_global), _stream())
        return t

    @classmethod
    def from_host(cls, cols):
        """Stage a part table from host columns (p_partkey, p_type)."""
        t = cls(len(cols["p_partkey"]))
        _h2d_cols(t, cols)
        return t


# ---------------- CustomScan lifecycle ----------------

class CustomScanState:
    """Base lifecycle, mirroring CustomExecMethods (extensible.h:117-152)."""

    def __init__(self):
        self._begun = False

    def BeginCustomScan(self, estate=None, eflags=0):
        self._begun = True
        self._begin(estate, eflags)
        self._rows = None
        self._pos = 0

    def ExecCustomScan(self):
        """One tuple per call; None = end of stream (nodeCustom.c:104)."""
        if not self._begun:
            raise OtbxError(3, "ExecCustomScan before BeginCustomScan")
        if self._rows is None:
            self._rows = self._run()
        if self._pos >= len(self._rows):
            return None
        row = self._rows[self._pos]
        self._pos += 1
        return row

    def ReScanCustomScan(self):
        self._rows = None
        self._pos = 0

    def EndCustomScan(self):
        self._begun = False
        self._end()

    # subclass hooks
    def _begin(self, estate, eflags): pass
    def _run(self): raise NotImplementedError
    def _end(self): pass

    def explain(self):
        """EXPLAIN ANALYZE analog: per-kernel HIP-event timings for this
        node, mirroring the reference's per-plan-node Instrumentation
        (include/executor/instrument.h:45, merged at the CN by
        commands/explain_dist.c). Returns {phase: ms} or None before run."""
        return None


class GpuSeqScanCount(CustomScanState):
    """SeqScan + qual + COUNT(*) (BASELINE config 2). Replaces the
    SeqScan→Agg(count) fragment (execScan.c:140 + nodeAgg.c)."""

    def __init__(self, lineitem, cutoff=Q1_CUTOFF_DEFAULT):
        super().__init__()
        self.li = lineitem
        self.cutoff = cutoff

    def _run(self):
        out = torch.zeros(1, dtype=torch.int64, device="cuda")
        call("otbx_scan_count", C.c_void_p(self.li.t["l_shipdate"].data_ptr()),
             C.c_int64(self.li.n), C.c_int32(self.cutoff),
             C.c_void_p(out.data_ptr()), _stream())
        return [(int(out.cpu().item()),)]


class GpuQ1PartialAgg(CustomScanState):
    """The DN fragment of TPC-H Q1: SeqScan → qual → project → Partial
    HashAgg (AGGSPLIT_INITIAL_SERIAL), one fused kernel. Emits one partial
    group state per call, ordered by (l_returnflag, l_linestatus).

    partial_state_tensors() exposes the dense device buffers the Coordinator
    merge all-gathers (fragment.py)."""

    def __init__(self, lineitem, cutoff=Q1_CUTOFF_DEFAULT):
        super().__init__()
        self.li = lineitem
        self.cutoff = cutoff
        self.kernel_ms = None
        self.sums = None
        self.counts = None

    def _run(self):
        self.sums = torch.empty((6, 5), dtype=torch.float64, device="cuda")
        self.counts = torch.empty(6, dtype=torch.int64, device="cuda")
        ms = C.c_float(0.0)
        call("otbx_q1_partial", C.byref(self.li.cstruct), C.c_int32(self.cutoff),
             C.c_void_p(self.sums.data_ptr()), C.c_void_p(self.counts.data_ptr()),
             _stream(), C.byref(ms))
        self.kernel_ms = ms.value
        return q1_rows_from_state(self.sums, self.counts)

    def partial_state_tensors(self):
        return self.sums, self.counts

    def explain(self):
        if self.kernel_ms is None:
            return None
        return {"otbx_q1_partial (SeqScan+Qual+Project+PartialAgg, fused)":
                self.kernel_ms}


def q1_rows_from_state(sums, counts):
    """Dense [6,5] sums + [6] counts → partial group rows (host)."""
    s = sums.cpu().numpy() if hasattr(sums, "cpu") else sums
    c = counts.cpu().numpy() if hasattr(counts, "cpu") else counts
    rows = []
    for g, (rf, ls) in enumerate(Q1_SLOT_ORDER):
        if c[g] == 0:
            continue
        rows.append({
            "l_returnflag": rf.decode(), "l_linestatus": ls.decode(),
            "sum_qty": float(s[g][0]), "sum_base_price": float(s[g][1]),
            "sum_disc_price": float(s[g][2]), "sum_charge": float(s[g][3]),
            "sum_disc": float(s[g][4]), "count_order": int(c[g]),
        })
    return rows


def q1_finalize(rows):
    """Finalize Aggregate (CN): avg = Sx/N (float8_avg semantics)."""
    out = []
    for r in rows:
        n = r["count_order"]
        fin = dict(r)
        fin["avg_qty"] = r["sum_qty"] / n
        fin["avg_price"] = r["sum_base_price"] / n
        fin["avg_disc"] = r["sum_disc"] / n
        out.append(fin)
    return out


class GpuQ3Fragment(CustomScanState):
    """The DN fragment of TPC-H Q3: customer⋈orders⋈lineitem + Partial
    HashAgg keyed on l_orderkey. cust_keys: optional device int64 tensor of
    the REPLICATED (post-broadcast) filtered customer keys;
    without it, the local customer shard is filtered in-kernel."""

    NP_DTYPE = [("l_orderkey", "i8"), ("revenue", "f8"),
                ("o_orderdate", "i4"), ("o_shippriority", "i4")]

    def __init__(self, customer, orders, lineitem, segment=0,
                 date=Q3_DATE_DEFAULT, cust_keys=None, k=10):
        super().__init__()
        self.cu, self.od, self.li = customer, orders, lineitem
        self.segment, self.date = segment, date
        self.cust_keys = cust_keys
        self.k = k
        self.kernel_ms = None    # [keyset, orders, probe_agg, compact]
        self.probe_hits = None   # N_probe_hits (roofline formula)
        self.ngroups = None
        self.groups = None       # lazy: fetch_groups()
        self._groups_dev = None

    def _run(self):
        import numpy as np
        L = lib()
        ncust = self.cu.n if self.cust_keys is None else len(self.cust_keys)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_q3_workspace_bytes(C.c_int64(ncust), C.c_int64(self.od.n),
                                        C.c_int64(self.li.n), C.byref(ws_bytes)))
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
        cap = self.od.n if self.od.n > 0 else 1
        groups = torch.empty(cap * 24, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")
        stats = torch.zeros(1, dtype=torch.int64, device="cuda")
        ms = (C.c_float * 4)()
        ck = None
        if self.cust_keys is not None:
            # an EMPTY broadcast (no customer in the segment anywhere) is
            # still a broadcast: torch gives an empty tensor a NULL
            # data_ptr, which the C-ABI would read as "filter the local
            # customer table instead"
            ck_buf = self.cust_keys if len(self.cust_keys) else \
                torch.zeros(1, dtype=torch.int64, device="cuda")
            ck = C.c_void_p(ck_buf.data_ptr())
        nck = C.c_int64(0 if self.cust_keys is None else len(self.cust_keys))
        call("otbx_q3_partial", C.byref(self.cu.cstruct), C.byref(self.od.cstruct),
             C.byref(self.li.cstruct), ck, nck, C.c_uint8(self.segment),
             C.c_int32(self.date), C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws_bytes.value), C.c_void_p(groups.data_ptr()),
             C.c_int64(cap), C.c_void_p(ng.data_ptr()),
             C.c_void_p(stats.data_ptr()), _stream(), ms)
        self.kernel_ms = list(ms)
        self._groups_dev = groups
        self.ngroups = int(ng.cpu().item())
        self.probe_hits = int(stats.cpu().item())
        # GPU top-k pre-selection (LIMIT 10 below the merge); the final
        # ordering of the ≤ few-thousand candidates happens on host
        n = self.ngroups
        if n == 0:
            self.groups = np.empty(0, dtype=np.dtype(self.NP_DTYPE))
            return []
        # retry with a larger cap if the threshold histogram bin holds more
        # candidates than fit (ncand receives the TRUE count; silently
        # truncating could drop real top-k rows)
        cap_cand = 1 << 20
        while True:
            cand = torch.empty(cap_cand * 24, dtype=torch.uint8, device="cuda")
            ncand = torch.zeros(1, dtype=torch.int64, device="cuda")
            hist = torch.empty(16384, dtype=torch.int32, device="cuda")
            call("otbx_topk_by_revenue", C.c_void_p(groups.data_ptr()),
                 C.c_int64(n), C.c_int64(self.k), C.c_void_p(cand.data_ptr()),
                 C.c_int64(cap_cand), C.c_void_p(ncand.data_ptr()),
                 C.c_void_p(hist.data_ptr()), _stream())
            nc = int(ncand.cpu().item())
            if nc <= cap_cand:
                break
            cap_cand = max(cap_cand * 2, nc)
        cands = cand[: nc * 24].cpu().numpy().view(np.dtype(self.NP_DTYPE))
        return [tuple(r) for r in q3_topk(cands, self.k)]

    def explain(self):
        if self.kernel_ms is None:
            return None
        names = ["customer keyset build (Hash build side 1)",
                 "orders filter+probe+insert (HashJoin 1 + Hash build 2)",
                 "lineitem scan-filter + probe + partial agg (HashJoin 2 + PartialAgg)",
                 "group compaction (emit)"]
        return dict(zip(names, self.kernel_ms))

    def fetch_groups(self, ordered=False):
        """D2H copy of ALL partial groups (parity tests / debugging).
        ordered=True returns them fully sorted by (revenue DESC,
        o_orderdate ASC) via the GPU radix sort (the no-LIMIT ORDER BY
        path)."""
        import numpy as np
        if ordered:
            return order_groups(self._groups_dev, self.ngroups)
        if self.groups is None or len(self.groups) != self.ngroups:
            self.groups = self._groups_dev[: self.ngroups * 24].cpu().numpy() \
                .view(np.dtype(self.NP_DTYPE))
        return self.groups


def q3_topk(groups, k=10):
    """ORDER BY revenue DESC, o_orderdate ASC LIMIT k (host-side; the
    coordinator merge-sort analog, execFragment.c:4035)."""
    import numpy as np
    order = np.lexsort((groups["l_orderkey"], groups["o_orderdate"],
                        -groups["revenue"]))
    return groups[order][:k]


def order_groups(groups_dev_u8, n):
    """ORDER BY revenue DESC, o_orderdate ASC over device q3 groups (raw
    24-B-record uint8 tensor) — the full-sort operator.
    Returns a sorted structured numpy array."""
    import numpy as np
    L = lib()
    ws_bytes = C.c_size_t(0)
    check(L.otbx_order_groups_workspace_bytes(C.c_int64(n), C.byref(ws_bytes)))
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty(max(n, 1) * 24, dtype=torch.uint8, device="cuda")
    call("otbx_order_groups", C.c_void_p(groups_dev_u8.data_ptr()),
         C.c_int64(n), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
         C.c_size_t(ws_bytes.value), _stream())
    return out[: n * 24].cpu().numpy().view(np.dtype(GpuQ3Fragment.NP_DTYPE))


class GpuQ9Fragment(CustomScanState):
    """The DN fragment of the Q9-shaped mix query (BASELINE config 5):
    lineitem ⋈ part[p_type % typemod == typeval] ⋈ orders, partial agg
    keyed on year(o_orderdate) — two HashJoins under a Partial HashAgg
    with a tiny dense group domain (7 years). Emits one partial state row
    per year; the Coordinator merge is elementwise (fragment.py
    merge_q9_partials), exactly the Q1 pattern."""

    YEARS = list(range(1992, 1999))

    def __init__(self, part, orders, lineitem, typemod=17, typeval=0,
                 nranks=1):
        super().__init__()
        self.pt, self.od, self.li = part, orders, lineitem
        self.typemod, self.typeval = typemod, typeval
        self.nranks = nranks
        self.kernel_ms = None
        self.sums = None
        self.counts = None

    def _run(self):
        L = lib()
        ws_bytes = C.c_size_t(0)
        check(L.otbx_q9_workspace_bytes(C.c_int64(self.pt.n),
                                        C.c_int64(self.od.n),
                                        C.c_int64(self.li.n),
                                        C.c_uint32(self.nranks),
                                        C.byref(ws_bytes)))
        ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
        self.sums = torch.empty(7, dtype=torch.float64, device="cuda")
        self.counts = torch.empty(7, dtype=torch.int64, device="cuda")
        ms = C.c_float(0.0)
        call("otbx_q9_partial", C.byref(self.pt.cstruct),
             C.byref(self.od.cstruct), C.byref(self.li.cstruct),
             C.c_uint8(self.typemod), C.c_uint8(self.typeval),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(self.sums.data_ptr()),
             C.c_void_p(self.counts.data_ptr()), _stream(), C.byref(ms))
        self.kernel_ms = ms.value
        return q9_rows_from_state(self.sums, self.counts)

    def partial_state_tensors(self):
        return self.sums, self.counts

    def explain(self):
        if self.kernel_ms is None:
            return None
        return {"k_q9_fused (Scan+2×HashJoin probe+PartialAgg, fused)":
                self.kernel_ms}


def q9_rows_from_state(sums, counts):
    """Dense [7] sums + [7] counts → partial rows ordered by year."""
    s = sums.cpu().numpy() if hasattr(sums, "cpu") else sums
    c = counts.cpu().numpy() if hasattr(counts, "cpu") else counts
    return [{"o_year": 1992 + g, "sum_revenue": float(s[g]),
             "count_rows": int(c[g])}
            for g in range(7) if c[g] != 0]


def partition_by_key(keys):
    """Repartition exchange, GPU half (the 'Distribute results
    by H: col' exchange of make_remotesubplan, createplan.c:8671): returns
    (perm, counts) where perm groups row indices into contiguous per-rank
    segments (owner = key % world) and counts[r] is segment r's length.
    fragment.exchange_rows() moves the gathered segments over RCCL."""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and \
        dist.is_initialized() else 1
    n = len(keys)
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    counts = (C.c_int64 * max(world, 1))()
    call("otbx_partition_by_key", C.c_void_p(keys.data_ptr()), C.c_int64(n),
         C.c_uint32(world), C.c_void_p(perm.data_ptr()), counts, _stream())
    return perm, list(counts)


_GATHER_FN = {torch.int64: "otbx_gather_i64", torch.float64: "otbx_gather_f64",
              torch.int32: "otbx_gather_i32", torch.uint8: "otbx_gather_u8"}


def gather(src, perm):
    """dst[i] = src[perm[i]] via the native gather kernels."""
    dst = torch.empty(len(perm), dtype=src.dtype, device="cuda")
    call(_GATHER_FN[src.dtype], C.c_void_p(src.data_ptr()),
         C.c_void_p(perm.data_ptr()), C.c_int64(len(perm)),
         C.c_void_p(dst.data_ptr()), _stream())
    return dst


SORT_DESC = 1          # OTBX_SORT_DESC
SORT_NULLS_FIRST = 2   # OTBX_SORT_NULLS_FIRST
_SORT_TYPE = {torch.int64: 0, torch.float64: 1, torch.int32: 2, torch.uint8: 3}


def sort_flags(nkeys, descending=None, nulls_first=None):
    """Per-key OTBX_SORT_* flag words. An unspecified nulls_first (None, or
    None for one key) takes the SQL default: NULLS LAST for ASC, NULLS FIRST
    for DESC (the parser's SORTBY_NULLS_DEFAULT rule, parse_clause.c)."""
    desc = [False] * nkeys if descending is None else list(descending)
    nf = [None] * nkeys if nulls_first is None else list(nulls_first)
    if len(desc) != nkeys or len(nf) != nkeys:
        raise OtbxError(3, "sort: one descending/nulls_first entry per key")
    out = []
    for d, f in zip(desc, nf):
        if f is None:
            f = bool(d)
        out.append((SORT_DESC if d else 0) | (SORT_NULLS_FIRST if f else 0))
    return out


class GpuSort(CustomScanState):
    """The Sort node (nodeSort.c:49 → tuplesort.c) over 1..8 key columns
    (device tensors of dtype int64, float64, int32 or uint8): per-key
    direction, NULL placement and optional null mask (uint8, nonzero =
    NULL), optional LIMIT. Stable; ordering contract in include/otbx.h
    (otbx_sort_perm). Yields ONE tuple: the int64 permutation tensor (row j
    of the output is input row perm[j]); gather(col) applies it to a payload
    column through the native gather kernels."""

    def __init__(self, keys, descending=None, nulls_first=None, nulls=None,
                 limit=0):
        super().__init__()
        self.keys = list(keys)
        nk = len(self.keys)
        if not 1 <= nk <= 8:
            raise OtbxError(3, "sort: 1..8 keys")
        for k in self.keys:
            if k.dtype not in _SORT_TYPE:
                raise OtbxError(3, f"sort: unsupported key dtype {k.dtype}")
            if len(k) != len(self.keys[0]):
                raise OtbxError(3, "sort: key columns differ in length")
        self.nulls = [None] * nk if nulls is None else list(nulls)
        if len(self.nulls) != nk:
            raise OtbxError(3, "sort: one nulls entry per key")
        self.flags = sort_flags(nk, descending, nulls_first)
        self.limit = int(limit)
        self.n = len(self.keys[0])
        self.perm = None
        self.sort_ms = None

    def spec(self):
        """The otbx_sortspec handed to otbx_sort_perm."""
        sp = SortSpecDev()
        sp.nkeys = len(self.keys)
        for c, k in enumerate(self.keys):
            sp.key[c].col = k.data_ptr()
            nt = self.nulls[c]
            sp.key[c].nulls = nt.data_ptr() if nt is not None else None
            sp.key[c].type = _SORT_TYPE[k.dtype]
            sp.key[c].flags = self.flags[c]
        return sp

    def _run(self):
        L = lib()
        n, nk = self.n, len(self.keys)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_sort_workspace_bytes(C.c_int64(n), C.c_int32(nk),
                                          C.c_int64(self.limit),
                                          C.byref(ws_bytes)),
              "otbx_sort_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        cap = min(self.limit, n) if self.limit > 0 else n
        perm = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda")
        nout = torch.zeros(1, dtype=torch.int64, device="cuda")
        sp = self.spec()
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_sort_perm", C.byref(sp), C.c_int64(n),
             C.c_int64(self.limit), C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws_bytes.value), C.c_void_p(perm.data_ptr()),
             C.c_void_p(nout.data_ptr()), _stream())
        ev1.record()
        k = int(nout.cpu().item())
        self.sort_ms = ev0.elapsed_time(ev1)
        self.perm = perm[:k]
        return [self.perm]

    def gather(self, col):
        """col reordered by the sort (runs the node if it has not run)."""
        if self.perm is None:
            self.perm = self._run()[0]
        return gather(col, self.perm)

    def explain(self):
        if self.sort_ms is None:
            return None
        return {"sort": self.sort_ms}


WINDOW_FUNCS = ("row_number", "rank", "dense_rank", "count_star", "count_v",
                "sum_v", "part_rows")
_WINDOW_DTYPE = {"sum_v": torch.float64, "sum_isnull": torch.uint8}


class GpuWindowAgg(CustomScanState):
    """The WindowAgg node (nodeWindowAgg.c) for one window specification
    OVER (PARTITION BY partition_by ORDER BY order_by) with the default
    frame: row_number / rank / dense_rank / part_rows and count(*) /
    count(v) / sum(v) over RANGE UNBOUNDED PRECEDING .. CURRENT ROW.
    Partition keys sort ASC with the SQL-default NULL placement; order keys
    take descending / nulls_first as GpuSort does (sort_flags). Runs GpuSort
    on the combined key list (skipped with zero keys: perm = NULL), then
    otbx_window. Yields ONE tuple: a dict of device tensors, indexed by
    sorted position, for the requested funcs (WINDOW_FUNCS; "sum_v" also
    yields "sum_isnull") plus "perm". Contract in include/otbx.h
    (otbx_window); finalize percent_rank / cume_dist with the functions
    below."""

    def __init__(self, partition_by, order_by, descending=None,
                 nulls_first=None, part_nulls=None, order_nulls=None,
                 vals=None, val_null=None, funcs=None, n=None):
        super().__init__()
        self.partition_by, self.order_by = list(partition_by), list(order_by)
        self.keys = self.partition_by + self.order_by
        npart, nord = len(self.partition_by), len(self.order_by)
        if npart + nord > 8:
            raise OtbxError(3, "window: at most 8 keys")
        pn = [None] * npart if part_nulls is None else list(part_nulls)
        on = [None] * nord if order_nulls is None else list(order_nulls)
        if len(pn) != npart or len(on) != nord:
            raise OtbxError(3, "window: one nulls entry per key")
        self.nulls = pn + on
        self.flags = sort_flags(npart) + \
            sort_flags(nord, descending, nulls_first)
        self.vals, self.val_null = vals, val_null
        if funcs is None:
            funcs = WINDOW_FUNCS if vals is not None else \
                ("row_number", "rank", "dense_rank", "count_star", "part_rows")
        self.funcs = tuple(funcs)
        for f in self.funcs:
            if f not in WINDOW_FUNCS:
                raise OtbxError(3, f"window: unknown function {f}")
        if not self.funcs:
            raise OtbxError(3, "window: no function requested")
        if vals is None and ("sum_v" in self.funcs or "count_v" in self.funcs):
            raise OtbxError(3, "window: sum_v / count_v need vals")
        for k in self.keys:
            if k.dtype not in _SORT_TYPE:
                raise OtbxError(3, f"window: unsupported key dtype {k.dtype}")
        if n is None:
            if self.keys:
                n = len(self.keys[0])
            elif vals is not None:
                n = len(vals)
            else:
                raise OtbxError(3, "window: no keys and no vals — pass n")
        self.n = int(n)
        for k in self.keys:
            if len(k) != self.n:
                raise OtbxError(3, "window: key columns differ in length")
        self.perm = None
        self.sort_ms = None
        self.window_ms = None

    def _run(self):
        L = lib()
        n = self.n
        self.sort_ms = 0.0
        perm = None
        if self.keys:
            srt = GpuSort(self.keys, nulls=self.nulls)
            srt.flags = list(self.flags)
            srt.BeginCustomScan()
            perm = srt.ExecCustomScan()
            srt.EndCustomScan()
            self.sort_ms = srt.sort_ms
            sp = srt.spec()
        else:
            sp = SortSpecDev()
            sp.nkeys = 0
        ws_bytes = C.c_size_t(0)
        check(L.otbx_window_workspace_bytes(C.c_int64(n), C.byref(ws_bytes)),
              "otbx_window_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        names = list(self.funcs)
        if "sum_v" in names:
            names.append("sum_isnull")
        res = {f: torch.empty(max(n, 1),
                              dtype=_WINDOW_DTYPE.get(f, torch.int64),
                              device="cuda") for f in names}
        out = WindowOutDev()
        for f, t in res.items():
            setattr(out, f, t.data_ptr())

        def vp(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        # an empty tensor has no address: with no rows, hand the argument
        # check a placeholder so that "vals given" stays visible to it
        vals = self.vals
        if vals is not None and n == 0:
            vals = torch.zeros(1, dtype=torch.float64, device="cuda")
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_window", C.byref(sp), C.c_int32(len(self.partition_by)),
             vp(perm), C.c_int64(n), vp(vals), vp(self.val_null),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.byref(out), _stream())
        ev1.record()
        ev1.synchronize()
        self.window_ms = ev0.elapsed_time(ev1)
        res = {f: t[:n] for f, t in res.items()}
        self.perm = perm if perm is not None else \
            torch.arange(n, dtype=torch.int64, device="cuda")
        res["perm"] = self.perm
        return [res]

    def gather(self, col):
        """col in sorted order (runs the node if it has not run)."""
        if self.perm is None:
            self._run()
        return gather(col, self.perm)

    def explain(self):
        if self.window_ms is None:
            return None
        return {"sort": self.sort_ms, "window": self.window_ms}


# window-function finalizers over the node's integer outputs (scalars or
# numpy arrays in, float or float64 array out)

def percent_rank(rank, part_rows):
    """window_percent_rank (windowfuncs.c:140): (rank - 1) / (NP - 1), and 0
    when the partition has a single row."""
    import numpy as np
    r = np.asarray(rank, dtype=np.float64)
    tp = np.asarray(part_rows, dtype=np.float64)
    out = np.where(tp <= 1.0, 0.0, (r - 1.0) / np.where(tp <= 1.0, 1.0,
                                                         tp - 1.0))
    return float(out) if out.ndim == 0 else out


def cume_dist(count_star, part_rows):
    """window_cume_dist (windowfuncs.c:189): NP / partition rows, where NP
    (rows preceding or peer with the current row) is exactly the
    default-frame count(*)."""
    import numpy as np
    out = np.asarray(count_star, dtype=np.float64) / \
        np.asarray(part_rows, dtype=np.float64)
    return float(out) if out.ndim == 0 else out


def _frame_bound(b, units, what):
    if b is None:
        return FB_UNBOUNDED, 0
    if isinstance(b, str):
        if b != "current":
            raise OtbxError(3, f"frame: unknown {what} bound {b!r}")
        return FB_CURRENT, 0
    b = int(b)
    if b == 0:
        return FB_CURRENT, 0
    if units == FRAME_RANGE:
        raise OtbxError(3, "frame: RANGE takes no offset bound")
    if not -2**63 <= b < 2**63:
        raise OtbxError(3, "frame: offset outside int64")
    return FB_OFFSET, b


def _frame(units, start, end):
    f = FrameDev()
    f.units = units
    f.start_kind, f.start_off = _frame_bound(start, units, "start")
    f.end_kind, f.end_off = _frame_bound(end, units, "end")
    return f


def rows_between(start, end):
    """ROWS BETWEEN start AND end as an otbx_frame. A bound is None
    (UNBOUNDED PRECEDING as start, UNBOUNDED FOLLOWING as end), 0 or
    "current" (CURRENT ROW), or a signed row offset: -2 is 2 PRECEDING, 3 is
    3 FOLLOWING."""
    return _frame(FRAME_ROWS, start, end)


def range_between(start, end):
    """RANGE BETWEEN start AND end: each bound None (unbounded) or 0 /
    "current" (the first / last peer of the current row)."""
    return _frame(FRAME_RANGE, start, end)


def window_frame_direct_default():
    """The widest bounded ROWS frame otbx_window_frame reduces by its per-row
    loop when OTBX_WIN_FRAME_DIRECT is unset."""
    w = C.c_int64(0)
    check(lib().otbx_window_frame_direct_default(C.byref(w)),
          "otbx_window_frame_direct_default")
    return w.value


class GpuWindowFrame(CustomScanState):
    """The WindowAgg node (nodeWindowAgg.c) for one window specification
    OVER (PARTITION BY partition_by ORDER BY order_by <frame>) and up to 8
    function calls that share it. frame comes from rows_between /
    range_between (default: RANGE UNBOUNDED PRECEDING .. CURRENT ROW). A call
    is one of
        ("ntile", buckets)
        ("lag" | "lead", col[, nulls[, offset = 1[, default = None]]])
        ("first_value" | "last_value", col[, nulls])
        ("nth_value", col, nulls, n)
        ("count_star",) | ("count", col[, nulls])
        ("sum" | "min" | "max", col[, nulls])
    with col a device tensor of dtype int64, float64, int32 or uint8 and
    nulls a uint8 mask (nonzero = NULL) or None; a lag / lead default of None
    is NULL. Keys are taken as GpuWindowAgg takes them. Runs GpuSort on the
    combined key list (skipped with zero keys: perm = NULL), then
    otbx_window_frame. Yields ONE tuple, a dict indexed by sorted position:
        "calls"  [(values, nulls or None)] in call order; an int64 SUM
                 yields (lo, hi, nulls) as GpuGroupAgg does (int128_sums)
        <name>   the same tuple under the call's function name (the first
                 call of that name)
        "perm"   the sort's permutation
    Contract in include/otbx.h (otbx_window_frame)."""

    def __init__(self, partition_by, order_by, descending=None,
                 nulls_first=None, part_nulls=None, order_nulls=None,
                 frame=None, calls=(), n=None):
        super().__init__()
        self.partition_by, self.order_by = list(partition_by), list(order_by)
        self.keys = self.partition_by + self.order_by
        npart, nord = len(self.partition_by), len(self.order_by)
        if npart + nord > 8:
            raise OtbxError(3, "window frame: at most 8 keys")
        pn = [None] * npart if part_nulls is None else list(part_nulls)
        on = [None] * nord if order_nulls is None else list(order_nulls)
        if len(pn) != npart or len(on) != nord:
            raise OtbxError(3, "window frame: one nulls entry per key")
        self.nulls = pn + on
        self.flags = sort_flags(npart) + \
            sort_flags(nord, descending, nulls_first)
        for k in self.keys:
            if k.dtype not in _SORT_TYPE:
                raise OtbxError(
                    3, f"window frame: unsupported key dtype {k.dtype}")
        self.frame = range_between(None, 0) if frame is None else frame
        if not isinstance(self.frame, FrameDev):
            raise OtbxError(3, "window frame: frame comes from rows_between "
                               "/ range_between")
        self.calls = []
        for c in calls:
            c = tuple(c)
            if not c or c[0] not in WIN_FUNCS:
                raise OtbxError(3, f"window frame: unknown function {c[:1]}")
            func = c[0]
            col = nl = default = None
            param = 0
            if func == "ntile":
                if len(c) != 2:
                    raise OtbxError(3, "window frame: ntile takes buckets")
                param = int(c[1])
            else:
                col = c[1] if len(c) > 1 else None
                nl = c[2] if len(c) > 2 else None
                if func in ("lag", "lead"):
                    param = int(c[3]) if len(c) > 3 else 1
                    default = c[4] if len(c) > 4 else None
                elif func == "nth_value":
                    if len(c) != 4:
                        raise OtbxError(
                            3, "window frame: nth_value takes col, nulls, n")
                    param = int(c[3])
            if func not in ("ntile", "count_star", "count") and col is None:
                raise OtbxError(3, f"window frame: {func} needs a column")
            if col is not None and col.dtype not in _SORT_TYPE:
                raise OtbxError(
                    3, f"window frame: unsupported dtype {col.dtype}")
            self.calls.append((func, col, nl, param, default))
        if not 1 <= len(self.calls) <= MAX_WINCALLS:
            raise OtbxError(3, "window frame: 1..8 calls")
        if n is None:
            cols = self.keys + [c[1] for c in self.calls if c[1] is not None]
            if not cols:
                raise OtbxError(3, "window frame: no column to size by — "
                                   "pass n")
            n = len(cols[0])
        self.n = int(n)
        for k in self.keys:
            if len(k) != self.n:
                raise OtbxError(3, "window frame: key columns differ in "
                                   "length")
        self.perm = None
        self.sort_ms = None
        self.window_ms = None

    def _run(self):
        L = lib()
        n = self.n
        self.sort_ms = 0.0
        perm = None
        if self.keys:
            srt = GpuSort(self.keys, nulls=self.nulls)
            srt.flags = list(self.flags)
            srt.BeginCustomScan()
            perm = srt.ExecCustomScan()
            srt.EndCustomScan()
            self.sort_ms = srt.sort_ms
            sp = srt.spec()
        else:
            sp = SortSpecDev()
            sp.nkeys = 0
        ws_bytes = C.c_size_t(0)
        check(L.otbx_window_frame_workspace_bytes(
            C.c_int64(n), C.c_int32(len(self.calls)), C.byref(ws_bytes)),
            "otbx_window_frame_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        cap = max(n, 1)

        def new(dtype):
            return torch.empty(cap, dtype=dtype, device="cuda")

        # an empty tensor has no address: with no rows, hand the argument
        # check a placeholder so that "column given" stays visible to it
        hold = torch.zeros(1, dtype=torch.int64, device="cuda")
        calls = (WinCallDev * MAX_WINCALLS)()
        outs = []
        for i, (func, col, nl, param, default) in enumerate(self.calls):
            wc = calls[i]
            wc.func = WIN_FUNCS[func]
            wc.type = _SORT_TYPE[col.dtype] if col is not None else 0
            wc.param = param
            if col is not None:
                wc.col = col.data_ptr() if n > 0 else hold.data_ptr()
            wc.nulls = nl.data_ptr() if nl is not None and n > 0 else None
            wc.def_isnull = 1 if default is None else 0
            if default is not None:
                if col.dtype == torch.float64:
                    wc.def_f = float(default)
                else:
                    wc.def_i = int(default)
            if func == "ntile":
                o = (new(torch.int32),)
            elif func in ("count_star", "count"):
                o = (new(torch.int64),)
            elif func == "sum" and col.dtype == torch.int64:
                o = (new(torch.int64), new(torch.int64), new(torch.uint8))
                wc.out_hi = o[1].data_ptr()
            elif func == "sum":
                o = (new(torch.float64 if col.dtype == torch.float64
                         else torch.int64), new(torch.uint8))
            else:
                o = (new(col.dtype), new(torch.uint8))
            wc.out = o[0].data_ptr()
            if len(o) > 1:
                wc.out_null = o[-1].data_ptr()
            outs.append(o)
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_window_frame", C.byref(sp),
             C.c_int32(len(self.partition_by)),
             C.c_void_p(perm.data_ptr()) if perm is not None and n > 0
             else None,
             C.c_int64(n), C.byref(self.frame), calls,
             C.c_int32(len(self.calls)), C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws_bytes.value), _stream())
        ev1.record()
        ev1.synchronize()
        self.window_ms = ev0.elapsed_time(ev1)
        self.perm = perm if perm is not None else \
            torch.arange(n, dtype=torch.int64, device="cuda")
        res = {"calls": [tuple(t[:n] for t in o) if len(o) > 1
                         else (o[0][:n], None) for o in outs]}
        for (func, *_), r in zip(self.calls, res["calls"]):
            res.setdefault(func, r)
        res["perm"] = self.perm
        return [res]

    def gather(self, col):
        """col in sorted order (runs the node if it has not run)."""
        if self.perm is None:
            self._run()
        return gather(col, self.perm)

    def explain(self):
        if self.window_ms is None:
            return None
        return {"sort": self.sort_ms, "window_frame": self.window_ms}


class GpuGroupAgg(CustomScanState):
    """The Agg node's sorted strategies (AGG_SORTED; AGG_PLAIN with no keys:
    agg_retrieve_direct, nodeAgg.c:2249) for a target list of up to 8
    aggregates over 0..8 GROUP BY keys (device tensors of dtype int64,
    float64, int32 or uint8, with optional null masks). aggs is a list of
        ("count_star",) | ("count", col[, nulls])
        | ("sum" | "min" | "max", col[, nulls])
    Keys sort as GpuSort sorts them (descending / nulls_first / key_nulls).
    Runs GpuSort on the keys — skipped with zero keys, or when a sorted
    `perm` is passed — then otbx_group_agg. Yields ONE tuple, a dict:
        "ngroups"   int
        "first_row" int64 tensor: the input row of each group's first row
        "keys"      [(values, nulls or None)] gathered through first_row by
                    the native gather kernels
        "aggs"      [(values, nulls or None)] cut to ngroups, in target-list
                    order; an int64 SUM yields (lo, hi, nulls): the int128
                    sum, see int128_sums()
    Groups come out in key order. Contract in include/otbx.h
    (otbx_group_agg); AVG is a finalizer: avg_f64 below, dec_avg for the
    integer sums."""

    def __init__(self, keys, aggs, descending=None, nulls_first=None,
                 key_nulls=None, perm=None, n=None):
        super().__init__()
        self.keys = list(keys)
        nk = len(self.keys)
        if nk > 8:
            raise OtbxError(3, "group agg: at most 8 keys")
        self.nulls = [None] * nk if key_nulls is None else list(key_nulls)
        if len(self.nulls) != nk:
            raise OtbxError(3, "group agg: one key_nulls entry per key")
        self.flags = sort_flags(nk, descending, nulls_first)
        for k in self.keys:
            if k.dtype not in _SORT_TYPE:
                raise OtbxError(3, f"group agg: unsupported key dtype {k.dtype}")
        self.aggs = []
        for a in aggs:
            a = tuple(a)
            if not a or a[0] not in AGG_FUNCS:
                raise OtbxError(3, f"group agg: unknown aggregate {a[:1]}")
            func = a[0]
            col = a[1] if len(a) > 1 else None
            nl = a[2] if len(a) > 2 else None
            if func in ("sum", "min", "max"):
                if col is None:
                    raise OtbxError(3, f"group agg: {func} needs a column")
                if col.dtype not in _SORT_TYPE:
                    raise OtbxError(
                        3, f"group agg: unsupported dtype {col.dtype}")
            self.aggs.append((func, col, nl))
        if len(self.aggs) > MAX_AGGS:
            raise OtbxError(3, "group agg: at most 8 aggregates")
        if n is None:
            cols = self.keys + [c for _, c, _ in self.aggs if c is not None]
            if cols:
                n = len(cols[0])
            elif perm is not None:
                n = len(perm)
            else:
                raise OtbxError(3, "group agg: no column to size by — pass n")
        self.n = int(n)
        for k in self.keys:
            if len(k) != self.n:
                raise OtbxError(3, "group agg: key columns differ in length")
        self.perm = perm
        self.sort_ms = None
        self.group_agg_ms = None

    def spec(self):
        sp = SortSpecDev()
        sp.nkeys = len(self.keys)
        for c, k in enumerate(self.keys):
            sp.key[c].col = k.data_ptr()
            nt = self.nulls[c]
            sp.key[c].nulls = nt.data_ptr() if nt is not None else None
            sp.key[c].type = _SORT_TYPE[k.dtype]
            sp.key[c].flags = self.flags[c]
        return sp

    def _run(self):
        L = lib()
        n = self.n
        self.sort_ms = 0.0
        perm = self.perm
        if perm is None and self.keys:
            srt = GpuSort(self.keys, nulls=self.nulls)
            srt.flags = list(self.flags)
            srt.BeginCustomScan()
            perm = srt.ExecCustomScan()
            srt.EndCustomScan()
            self.sort_ms = srt.sort_ms
        sp = self.spec()
        ws_bytes = C.c_size_t(0)
        check(L.otbx_group_agg_workspace_bytes(C.c_int64(n),
                                               C.byref(ws_bytes)),
              "otbx_group_agg_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        cap = max(n, 1)

        def new(dtype):
            return torch.empty(cap, dtype=dtype, device="cuda")

        calls = AggCallsDev()
        calls.naggs = len(self.aggs)
        outs = []
        for i, (func, col, nl) in enumerate(self.aggs):
            ac = calls.agg[i]
            ac.func = AGG_FUNCS[func]
            ac.type = _SORT_TYPE[col.dtype] if col is not None else 0
            ac.col = col.data_ptr() if col is not None and n > 0 else None
            ac.nulls = nl.data_ptr() if nl is not None and n > 0 else None
            if func in ("count_star", "count"):
                o = (new(torch.int64),)
            elif func == "sum" and col.dtype == torch.int64:
                o = (new(torch.int64), new(torch.int64), new(torch.uint8))
                ac.out_hi = o[1].data_ptr()
            elif func == "sum":
                o = (new(torch.float64 if col.dtype == torch.float64
                         else torch.int64), new(torch.uint8))
            else:
                o = (new(col.dtype), new(torch.uint8))
            ac.out = o[0].data_ptr()
            if len(o) > 1:
                ac.out_null = o[-1].data_ptr()
            outs.append(o)
        first = new(torch.int64)
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_group_agg", C.byref(sp),
             C.c_void_p(perm.data_ptr()) if perm is not None and n > 0
             else None,
             C.c_int64(n), C.byref(calls), C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws_bytes.value), C.c_void_p(first.data_ptr()),
             C.c_void_p(ng.data_ptr()), _stream())
        ev1.record()
        ngroups = int(ng.cpu().item())
        self.group_agg_ms = ev0.elapsed_time(ev1)
        first = first[:ngroups]
        keys = []
        for k, m in zip(self.keys, self.nulls):
            if ngroups == 0:
                keys.append((k[:0], None if m is None else m[:0]))
            else:
                keys.append((gather(k, first),
                             None if m is None else gather(m, first)))
        return [{"ngroups": ngroups, "first_row": first, "keys": keys,
                 "aggs": [tuple(t[:ngroups] for t in o) if len(o) > 1
                          else (o[0][:ngroups], None) for o in outs]}]

    def explain(self):
        if self.group_agg_ms is None:
            return None
        return {"sort": self.sort_ms, "group_agg": self.group_agg_ms}


class GpuOrderedAgg(CustomScanState):
    """The aggregates that sort their argument inside each group:
    agg(DISTINCT x) (process_ordered_aggregate_single, nodeAgg.c:888) and
    percentile_disc / percentile_cont / mode() WITHIN GROUP (ORDER BY x)
    (orderedsetaggs.c), for 0..7 GROUP BY keys and ONE argument column `arg`
    (device tensors of dtype int64, float64, int32 or uint8, with optional
    null masks). aggs is a list of up to 8 of
        ("count_distinct",) | ("sum_distinct",)
        | ("percentile_disc", p) | ("percentile_cont", p) | ("mode",)
    with 0 <= p <= 1; several percentiles (percentile_disc(array[...])) are
    several entries. arg_descending / arg_nulls_first are the ORDER BY flags
    of the argument (arg_nulls_first=None takes the SQL default of the
    direction). Runs GpuSort on keys + [arg] unless a `perm` sorted that way
    is passed, then otbx_ordered_agg. Yields ONE tuple, a dict shaped like
    GpuGroupAgg's:
        "ngroups", "first_row", "keys"   as GpuGroupAgg yields them — the
                    same group numbering, so GpuGroupAgg(keys, ..., perm=
                    row["perm"]) gives the ordinary aggregates of the same
                    target list, side by side, from the one sort
        "aggs"      [(values, nulls or None)] cut to ngroups, in list order;
                    sum_distinct over int64 yields (lo, hi, nulls), see
                    int128_sums(); percentile_disc and mode have arg's dtype
                    and the chosen row's bit pattern, percentile_cont is
                    float64, count_distinct int64 without nulls
        "perm"      the permutation used
    avg(DISTINCT x) is avg_f64 / dec_avg over sum_distinct and
    count_distinct. A text argument needs no kernel of its own: rank the
    column with GpuText.rank, pass the codes as `arg`, and TextRank.decode
    turns percentile_disc / mode results back into strings (count_distinct
    of the codes is count(DISTINCT name)). Contract in include/otbx.h
    (otbx_ordered_agg)."""

    def __init__(self, keys, arg, aggs, arg_nulls=None, arg_descending=False,
                 arg_nulls_first=False, descending=None, nulls_first=None,
                 key_nulls=None, perm=None, n=None):
        super().__init__()
        self.keys = list(keys)
        nk = len(self.keys)
        if nk > 7:
            raise OtbxError(3, "ordered agg: at most 7 keys")
        self.nulls = [None] * nk if key_nulls is None else list(key_nulls)
        if len(self.nulls) != nk:
            raise OtbxError(3, "ordered agg: one key_nulls entry per key")
        self.flags = sort_flags(nk, descending, nulls_first) + \
            sort_flags(1, [arg_descending], [arg_nulls_first])
        if not isinstance(arg, torch.Tensor):
            raise OtbxError(3, "ordered agg: the argument is a device tensor")
        for k in self.keys + [arg]:
            if k.dtype not in _SORT_TYPE:
                raise OtbxError(
                    3, f"ordered agg: unsupported dtype {k.dtype}")
        self.arg, self.arg_nulls = arg, arg_nulls
        self.aggs = []
        for a in aggs:
            a = tuple(a)
            if not a or a[0] not in OAGG_FUNCS:
                raise OtbxError(3, f"ordered agg: unknown aggregate {a[:1]}")
            func, p = a[0], 0.0
            if func in ("percentile_disc", "percentile_cont"):
                if len(a) != 2:
                    raise OtbxError(3, f"ordered agg: {func} needs a fraction")
                p = float(a[1])
                if not 0.0 <= p <= 1.0:   # a NaN fails too
                    raise OtbxError(3, f"percentile value {p:g} is not "
                                       "between 0 and 1")
            elif len(a) != 1:
                raise OtbxError(3, f"ordered agg: {func} takes no parameter")
            self.aggs.append((func, p))
        if len(self.aggs) > MAX_AGGS:
            raise OtbxError(3, "ordered agg: at most 8 aggregates")
        self.n = len(arg) if n is None else int(n)
        for k in self.keys + [arg]:
            if len(k) != self.n:
                raise OtbxError(3, "ordered agg: columns differ in length")
        self.perm = perm
        self.sort_ms = None
        self.ordered_agg_ms = None

    def spec(self):
        sp = SortSpecDev()
        cols = self.keys + [self.arg]
        nulls = self.nulls + [self.arg_nulls]
        sp.nkeys = len(cols)
        for c, k in enumerate(cols):
            sp.key[c].col = k.data_ptr()
            nt = nulls[c]
            sp.key[c].nulls = nt.data_ptr() if nt is not None else None
            sp.key[c].type = _SORT_TYPE[k.dtype]
            sp.key[c].flags = self.flags[c]
        return sp

    def _run(self):
        L = lib()
        n = self.n
        self.sort_ms = 0.0
        perm = self.perm
        if perm is None:
            srt = GpuSort(self.keys + [self.arg],
                          nulls=self.nulls + [self.arg_nulls])
            srt.flags = list(self.flags)
            srt.BeginCustomScan()
            perm = srt.ExecCustomScan()
            srt.EndCustomScan()
            self.sort_ms = srt.sort_ms
        sp = self.spec()
        ws_bytes = C.c_size_t(0)
        check(L.otbx_ordered_agg_workspace_bytes(
            C.c_int64(n), C.c_int32(len(self.aggs)), C.byref(ws_bytes)),
            "otbx_ordered_agg_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        cap = max(n, 1)

        def new(dtype):
            return torch.empty(cap, dtype=dtype, device="cuda")

        adt = self.arg.dtype
        calls = OAggCallsDev()
        calls.ncalls = len(self.aggs)
        outs = []
        for i, (func, p) in enumerate(self.aggs):
            oc = calls.call[i]
            oc.func = OAGG_FUNCS[func]
            oc.fraction = p
            if func == "count_distinct":
                o = (new(torch.int64),)
            elif func == "sum_distinct" and adt == torch.int64:
                o = (new(torch.int64), new(torch.int64), new(torch.uint8))
                oc.out_hi = o[1].data_ptr()
            elif func == "sum_distinct":
                o = (new(torch.float64 if adt == torch.float64
                         else torch.int64), new(torch.uint8))
            elif func == "percentile_cont":
                o = (new(torch.float64), new(torch.uint8))
            else:
                o = (new(adt), new(torch.uint8))
            oc.out = o[0].data_ptr()
            if len(o) > 1:
                oc.out_null = o[-1].data_ptr()
            outs.append(o)
        first = new(torch.int64)
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_ordered_agg", C.byref(sp), C.c_int32(len(self.keys)),
             C.c_void_p(perm.data_ptr()) if perm is not None and n > 0
             else None,
             C.c_int64(n), C.byref(calls), C.c_void_p(ws.data_ptr()),
             C.c_size_t(ws_bytes.value), C.c_void_p(first.data_ptr()),
             C.c_void_p(ng.data_ptr()), _stream())
        ev1.record()
        ngroups = int(ng.cpu().item())
        self.ordered_agg_ms = ev0.elapsed_time(ev1)
        first = first[:ngroups]
        keys = []
        for k, m in zip(self.keys, self.nulls):
            if ngroups == 0:
                keys.append((k[:0], None if m is None else m[:0]))
            else:
                keys.append((gather(k, first),
                             None if m is None else gather(m, first)))
        self.perm = perm
        return [{"ngroups": ngroups, "first_row": first, "keys": keys,
                 "aggs": [tuple(t[:ngroups] for t in o) if len(o) > 1
                          else (o[0][:ngroups], None) for o in outs],
                 "perm": perm}]

    def explain(self):
        if self.ordered_agg_ms is None:
            return None
        return {"sort": self.sort_ms, "ordered_agg": self.ordered_agg_ms}


def int128_sums(lo, hi, nulls=None):
    """Python ints of an int64 SUM's (lo, hi) output — the Int128AggState
    encoding of otbx_group_agg: unsigned low word, signed high word. None
    where nulls is set. Tensors or numpy arrays in, a list out."""
    import numpy as np

    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else \
            np.asarray(a)
    lo, hi = host(lo), host(hi)
    nl = [0] * len(lo) if nulls is None else host(nulls).tolist()
    lo = lo.view(np.uint64) if lo.dtype == np.int64 else lo
    return [None if z else (int(h) << 64) | int(l)
            for l, h, z in zip(lo.tolist(), hi.tolist(), nl)]


def avg_f64(sum_v, count):
    """float8_avg (float.c:2949) over the SUM(F64) / COUNT outputs: Sx / N.
    AVG over no non-NULL input is NULL: None for scalars, NaN in an array
    result."""
    import numpy as np
    s = np.asarray(sum_v, dtype=np.float64)
    c = np.asarray(count, dtype=np.float64)
    if s.ndim == 0 and c.ndim == 0:
        return None if c == 0.0 else float(s / c)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c == 0.0, np.nan, s / np.where(c == 0.0, 1.0, c))


CMP_OPS = {"=": 0, "<>": 1, "<": 2, "<=": 3, ">": 4, ">=": 5,
           "isnull": 6, "notnull": 7}   # OTBX_CMP_*
MAX_QUAL_TERMS = 16                     # OTBX_MAX_QUAL_TERMS


class QualTerm:
    """One term of a qual; build it with qual_term()."""
    __slots__ = ("col", "op", "rhs", "nulls", "rnulls")

    def __init__(self, col, op, rhs, nulls, rnulls):
        self.col, self.op, self.rhs = col, op, rhs
        self.nulls, self.rnulls = nulls, rnulls


def qual_term(col, op, rhs=None, nulls=None, rnulls=None):
    """col OP rhs as a term of GpuFilter's qual. col: device tensor of dtype
    int64, float64, int32 or uint8. op: "=", "<>", "<", "<=", ">", ">=",
    "isnull" or "notnull". rhs: a Python number (an int for the integer
    dtypes), or a device tensor of col's dtype and length for a comparison
    of two columns; None for the null tests. nulls / rnulls: optional uint8
    null masks (nonzero = NULL) of col / of the rhs column."""
    if op not in CMP_OPS:
        raise OtbxError(3, f"filter: unknown operator {op!r}")
    if not isinstance(col, torch.Tensor) or col.dtype not in _SORT_TYPE:
        raise OtbxError(3, "filter: unsupported column dtype "
                           f"{getattr(col, 'dtype', type(col))}")
    n = len(col)
    if op in ("isnull", "notnull"):
        if rhs is not None or rnulls is not None:
            raise OtbxError(3, f"filter: {op} takes no right operand")
    elif isinstance(rhs, torch.Tensor):
        if rhs.dtype != col.dtype:
            raise OtbxError(3, f"filter: {col.dtype} column compared with a "
                               f"{rhs.dtype} column")
        if len(rhs) != n:
            raise OtbxError(3, "filter: columns differ in length")
    else:
        if rnulls is not None:
            raise OtbxError(3, "filter: rnulls without a right column")
        if isinstance(rhs, bool) or not isinstance(rhs, (int, float)):
            raise OtbxError(3, f"filter: {op} needs a number or a column")
        if col.dtype != torch.float64:
            if not isinstance(rhs, int):
                raise OtbxError(3, "filter: integer column compared with a "
                                   "non-integer constant")
            if not -2**63 <= rhs < 2**63:
                raise OtbxError(3, "filter: constant outside int64")
    for m in (nulls, rnulls):
        if m is not None and (m.dtype != torch.uint8 or len(m) != n):
            raise OtbxError(3, "filter: a null mask is a uint8 tensor of the "
                               "column's length")
    return QualTerm(col, op, rhs, nulls, rnulls)


class GpuFilter(CustomScanState):
    """SeqScan's qual for any plan shape (ExecScan → ExecQual,
    execScan.c:140): `clauses` is a list of lists of qual_term() terms, the
    AND of ORs; [] is no qual and selects every row (pass n then). At most
    16 terms in all. Yields ONE tuple: the int64 selection tensor — the
    passing row indices in ascending order — or, with count_only, the count
    (the selection is never written). `.count` holds the count after the
    run; gather(col) applies the selection through the native gather
    kernels. Contract in include/otbx.h (otbx_filter_sel)."""

    def __init__(self, clauses, count_only=False, n=None):
        super().__init__()
        self.clauses = [list(c) for c in clauses]
        terms = [t for c in self.clauses for t in c]
        if any(len(c) == 0 for c in self.clauses):
            raise OtbxError(3, "filter: an empty clause is FALSE for every "
                               "row — drop the scan instead")
        if len(terms) > MAX_QUAL_TERMS:
            raise OtbxError(3, f"filter: at most {MAX_QUAL_TERMS} terms")
        for t in terms:
            if not isinstance(t, QualTerm):
                raise OtbxError(3, "filter: build terms with qual_term()")
        if n is None:
            if not terms:
                raise OtbxError(3, "filter: no qual — pass n")
            n = len(terms[0].col)
        self.n = int(n)
        for t in terms:
            if len(t.col) != self.n:
                raise OtbxError(3, "filter: columns differ in length")
        self.count_only = bool(count_only)
        self.sel = None
        self.count = None
        self.filter_ms = None

    def qual(self):
        """The otbx_qual handed to otbx_filter_sel."""
        q = QualDev()
        i = 0
        for cid, clause in enumerate(self.clauses):
            for t in clause:
                d = q.term[i]
                d.col = t.col.data_ptr()
                d.nulls = t.nulls.data_ptr() if t.nulls is not None else None
                d.type = _SORT_TYPE[t.col.dtype]
                d.op = CMP_OPS[t.op]
                d.clause = cid
                if isinstance(t.rhs, torch.Tensor):
                    d.rcol = t.rhs.data_ptr()
                    d.rnulls = t.rnulls.data_ptr() \
                        if t.rnulls is not None else None
                elif t.rhs is not None:
                    if t.col.dtype == torch.float64:
                        d.cf = float(t.rhs)
                    else:
                        d.ci = t.rhs
                i += 1
        q.nterms = i
        return q

    def _run(self):
        L = lib()
        n = self.n
        ws_bytes = C.c_size_t(0)
        check(L.otbx_filter_workspace_bytes(C.c_int64(n), C.byref(ws_bytes)),
              "otbx_filter_workspace_bytes")
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        sel = None if self.count_only else \
            torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        nsel = torch.zeros(1, dtype=torch.int64, device="cuda")
        q = self.qual()
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_filter_sel", C.byref(q), C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(sel.data_ptr()) if sel is not None else None,
             C.c_void_p(nsel.data_ptr()), _stream())
        ev1.record()
        self.count = int(nsel.cpu().item())
        self.filter_ms = ev0.elapsed_time(ev1)
        if self.count_only:
            return [(self.count,)]
        self.sel = sel[:self.count]
        return [self.sel]

    def gather(self, col):
        """The passing rows of col (runs the node if it has not run)."""
        if self.count_only:
            raise OtbxError(3, "filter: count_only keeps no selection")
        if self.sel is None:
            self._run()
        return gather(col, self.sel)

    def explain(self):
        if self.filter_ms is None:
            return None
        return {"filter": self.filter_ms}


# ---------------- Project: typed scalar expressions ----------------

EX_OPS = {"col": 0, "const": 1, "+": 2, "-": 3, "*": 4, "/": 5, "%": 6,
          "neg": 7, "abs": 8, "cast": 9, "=": 10, "<>": 11, "<": 12,
          "<=": 13, ">": 14, ">=": 15, "and": 16, "or": 17, "not": 18,
          "isnull": 19, "notnull": 20, "case": 21,
          "coalesce": 22}                         # OTBX_EX_*
EX_TYPES = {"i64": 0, "f64": 1, "bool": 2}        # OTBX_EXT_*
MAX_EXPR_INSTRS = 32                              # OTBX_MAX_EXPR_INSTRS
MAX_EXPR_DEPTH = 8                                # OTBX_MAX_EXPR_DEPTH
PROJECT_TILE = 1024                               # rows per workgroup
PROJECT_ERRORS = {1: "division by zero", 2: "bigint out of range",
                  3: "value out of range: overflow",
                  4: "value out of range: underflow",
                  5: "integer out of range"}      # OTBX_EXERR_*
_EX_OUT_DTYPE = {"i64": torch.int64, "f64": torch.float64,
                 "bool": torch.uint8}


class Expr:
    """A typed scalar expression tree for GpuProject; build it with col(),
    const(), null(), case(), coalesce() and the operators below. vtype is
    "i64", "f64" or "bool"; nullable follows the rules of include/otbx.h.
    Where an i64 operand meets an f64 one the i64 side is cast (i8tod), as
    the reference's parser picks the float8 operator. `==` is NOT
    overloaded: use .eq()."""
    __slots__ = ("op", "args", "vtype", "nullable", "payload", "nulls",
                 "ninstr", "depth", "n_src")

    def __init__(self, op, args, vtype, nullable, payload=None, nulls=None,
                 n_src=None):
        self.op, self.args, self.vtype = op, tuple(args), vtype
        self.nullable, self.payload, self.nulls = nullable, payload, nulls
        self.ninstr = 1 + sum(a.ninstr for a in self.args)
        self.depth = max([1] + [i + a.depth for i, a in enumerate(self.args)])
        for a in self.args:
            if a.n_src is not None:
                if n_src is not None and a.n_src != n_src:
                    raise OtbxError(3, "project: columns differ in length")
                n_src = a.n_src
        self.n_src = n_src
        if self.ninstr > MAX_EXPR_INSTRS:
            raise OtbxError(3, "project: the expression needs more than "
                               f"{MAX_EXPR_INSTRS} instructions")
        if self.depth > MAX_EXPR_DEPTH:
            raise OtbxError(3, "project: the expression needs a stack deeper "
                               f"than {MAX_EXPR_DEPTH}")

    # ---- arithmetic ----
    def _arith(self, op, other, swap=False):
        a, b = _ex_unify(self, other, "project: " + op)
        if swap:
            a, b = b, a
        if a.vtype == "bool" or (op == "%" and a.vtype != "i64"):
            raise OtbxError(3, f"project: {op} on {a.vtype} operands")
        return Expr(op, (a, b), a.vtype, a.nullable or b.nullable)

    def __add__(self, o): return self._arith("+", o)
    def __radd__(self, o): return self._arith("+", o, True)
    def __sub__(self, o): return self._arith("-", o)
    def __rsub__(self, o): return self._arith("-", o, True)
    def __mul__(self, o): return self._arith("*", o)
    def __rmul__(self, o): return self._arith("*", o, True)
    def __truediv__(self, o): return self._arith("/", o)
    def __rtruediv__(self, o): return self._arith("/", o, True)
    def __mod__(self, o): return self._arith("%", o)
    def __rmod__(self, o): return self._arith("%", o, True)

    def _unary(self, op):
        if self.vtype == "bool":
            raise OtbxError(3, f"project: {op} on a bool operand")
        return Expr(op, (self,), self.vtype, self.nullable)

    def __neg__(self): return self._unary("neg")
    def __abs__(self): return self._unary("abs")

    def cast(self, to):
        """i8tod ("f64") on an i64 value, dtoi8 ("i64") on an f64 one."""
        if to not in ("i64", "f64"):
            raise OtbxError(3, f"project: cast to {to!r}")
        if self.vtype == "bool" or self.vtype == to:
            raise OtbxError(3, f"project: cast of {self.vtype} to {to}")
        return Expr("cast", (self,), to, self.nullable, payload=to)

    # ---- comparisons ----
    def _cmp(self, op, other):
        a, b = _ex_unify(self, other, "project: " + op)
        if a.vtype == "bool":
            raise OtbxError(3, f"project: {op} on bool operands")
        return Expr(op, (a, b), "bool", a.nullable or b.nullable)

    def eq(self, o): return self._cmp("=", o)
    def ne(self, o): return self._cmp("<>", o)
    def lt(self, o): return self._cmp("<", o)
    def le(self, o): return self._cmp("<=", o)
    def gt(self, o): return self._cmp(">", o)
    def ge(self, o): return self._cmp(">=", o)

    # ---- boolean ----
    def _bool2(self, op, other, swap=False):
        a, b = self, _ex_lift(other)
        if swap:
            a, b = b, a
        if a.vtype != "bool" or b.vtype != "bool":
            raise OtbxError(3, f"project: {op} needs bool operands")
        return Expr(op, (a, b), "bool", a.nullable or b.nullable)

    def __and__(self, o): return self._bool2("and", o)
    def __rand__(self, o): return self._bool2("and", o, True)
    def __or__(self, o): return self._bool2("or", o)
    def __ror__(self, o): return self._bool2("or", o, True)

    def __invert__(self):
        if self.vtype != "bool":
            raise OtbxError(3, "project: not needs a bool operand")
        return Expr("not", (self,), "bool", self.nullable)

    def isnull(self): return Expr("isnull", (self,), "bool", False)
    def notnull(self): return Expr("notnull", (self,), "bool", False)

    def __bool__(self):
        raise OtbxError(3, "project: an expression has no truth value — "
                           "combine with & | ~ and compare with .eq()")

    # ---- lowering ----
    def program(self):
        """The postfix instruction list: (op,) tuples, leaves and casts with
        their payload — ("col", tensor, nulls), ("const", vtype, value) with
        value None for the NULL constant, ("cast", vtype)."""
        out = []
        for a in self.args:
            out.extend(a.program())
        if self.op == "col":
            out.append(("col", self.payload, self.nulls))
        elif self.op == "const":
            out.append(("const", self.vtype, self.payload))
        elif self.op == "cast":
            out.append(("cast", self.vtype))
        else:
            out.append((self.op,))
        return out

    def to_dev(self):
        """The otbx_expr handed to otbx_project."""
        return program_to_dev(self.program())


def program_to_dev(program):
    """otbx_expr from an instruction list in Expr.program()'s form."""
    e = ExprDev()
    if len(program) > MAX_EXPR_INSTRS:
        raise OtbxError(3, f"project: more than {MAX_EXPR_INSTRS} instructions")
    for i, ins in enumerate(program):
        d = e.instr[i]
        d.op = EX_OPS[ins[0]]
        if ins[0] == "col":
            d.type = _SORT_TYPE[ins[1].dtype]
            d.col = ins[1].data_ptr()
            d.nulls = ins[2].data_ptr() if ins[2] is not None else None
        elif ins[0] == "const":
            d.type = EX_TYPES[ins[1]]
            if ins[2] is None:
                d.isnull = 1
            elif ins[1] == "f64":
                d.cf = ins[2]
            else:
                d.ci = int(ins[2])
        elif ins[0] == "cast":
            d.type = EX_TYPES[ins[1]]
    e.ninstr = len(program)
    return e


def _ex_lift(x):
    if isinstance(x, Expr):
        return x
    return const(x)


def _ex_unify(a, b, what):
    """Both operands as Expr of one numeric type: Python numbers lift to
    constants (an int beside an f64 operand to an f64 constant), and an i64
    operand beside an f64 one is cast."""
    if not isinstance(a, Expr) and isinstance(b, Expr) and \
            b.vtype == "f64" and isinstance(a, int) and not isinstance(a, bool):
        a = float(a)
    if not isinstance(b, Expr) and isinstance(a, Expr) and \
            a.vtype == "f64" and isinstance(b, int) and not isinstance(b, bool):
        b = float(b)
    a, b = _ex_lift(a), _ex_lift(b)
    if a.vtype != b.vtype:
        if {a.vtype, b.vtype} != {"i64", "f64"}:
            raise OtbxError(3, f"{what}: {a.vtype} with {b.vtype}")
        if a.vtype == "i64":
            a = a.cast("f64")
        else:
            b = b.cast("f64")
    return a, b


def col(tensor, nulls=None):
    """A column leaf: a device tensor of dtype int64, float64, int32 or uint8
    (the two narrow ones widen to i64) with an optional uint8 null mask."""
    if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _SORT_TYPE \
            or tensor.dim() != 1:
        raise OtbxError(3, "project: unsupported column "
                           f"{getattr(tensor, 'dtype', type(tensor))}")
    if nulls is not None and (not isinstance(nulls, torch.Tensor) or
                              nulls.dtype != torch.uint8 or
                              nulls.shape != tensor.shape):
        raise OtbxError(3, "project: a null mask is a uint8 tensor of the "
                           "column's length")
    return Expr("col", (), "f64" if tensor.dtype == torch.float64 else "i64",
                nulls is not None, payload=tensor, nulls=nulls,
                n_src=len(tensor))


def const(v):
    """A constant: bool → bool, int → i64, float → f64."""
    if isinstance(v, bool):
        return Expr("const", (), "bool", False, payload=v)
    if isinstance(v, int):
        if not -2**63 <= v < 2**63:
            raise OtbxError(3, "project: constant outside int64")
        return Expr("const", (), "i64", False, payload=v)
    if isinstance(v, float):
        return Expr("const", (), "f64", False, payload=v)
    raise OtbxError(3, f"project: no constant from {type(v).__name__}")


def null(vtype):
    """The NULL constant of type "i64", "f64" or "bool"."""
    if vtype not in EX_TYPES:
        raise OtbxError(3, f"project: unknown type {vtype!r}")
    return Expr("const", (), vtype, True, payload=None)


def case(cond, then, else_):
    """CASE WHEN cond THEN then ELSE else_ END; nest it for more arms."""
    cond = _ex_lift(cond)
    if cond.vtype != "bool":
        raise OtbxError(3, "project: CASE needs a bool condition")
    if isinstance(then, Expr) or isinstance(else_, Expr):
        t, f = _ex_unify(then, else_, "project: CASE arms")
    else:
        t, f = _ex_unify(_ex_lift(then), else_, "project: CASE arms")
    return Expr("case", (cond, t, f), t.vtype, t.nullable or f.nullable)


def coalesce(a, b):
    """The first operand if it is non-NULL, else the second."""
    if isinstance(a, Expr) or isinstance(b, Expr):
        a, b = _ex_unify(a, b, "project: COALESCE")
    else:
        a, b = _ex_unify(_ex_lift(a), b, "project: COALESCE")
    return Expr("coalesce", (a, b), a.vtype, a.nullable and b.nullable)


class GpuProject(CustomScanState):
    """One target-list expression for any plan shape (ExecProject over the
    expression interpreter, execExprInterp.c): evaluates `expr` for every
    row — with `sel`, the int64 selection GpuFilter yielded, only for the
    selected rows, read through it — into a new column. Yields ONE tuple
    (values, nulls): device tensors of n rows, nulls a uint8 mask or None
    when the expression cannot be NULL. They go unchanged into GpuHashAgg
    (vals / val_null), GpuSort and qual_term. `out`: an optional
    preallocated result tensor; an int32 one takes an i64 result through the
    int84 range check. `n`: the row count of an expression without columns.
    An error the reference would have raised (division by zero, bigint out
    of range, float8 overflow / underflow, integer out of range) is raised
    after the run as OtbxError(4) naming the first raising output row.
    Contract in include/otbx.h (otbx_project)."""

    def __init__(self, expr, sel=None, n=None, out=None):
        super().__init__()
        if not isinstance(expr, Expr):
            raise OtbxError(3, "project: build the expression with col(), "
                               "const(), ...")
        self.expr = expr
        if sel is not None and (not isinstance(sel, torch.Tensor) or
                                sel.dtype != torch.int64 or sel.dim() != 1):
            raise OtbxError(3, "project: sel is an int64 tensor of row ids")
        self.sel = sel
        if n is None:
            if sel is not None:
                n = len(sel)
            elif expr.n_src is not None:
                n = expr.n_src
            else:
                raise OtbxError(3, "project: no column — pass n")
        self.n = int(n)
        self.n_src = expr.n_src if expr.n_src is not None else self.n
        if self.n < 0 or (sel is not None and self.n > len(sel)) or \
                (sel is None and self.n > self.n_src) or \
                (self.n > 0 and self.n_src == 0):
            raise OtbxError(3, "project: n outside the input")
        want = _EX_OUT_DTYPE[expr.vtype]
        if out is not None:
            ok = isinstance(out, torch.Tensor) and out.dim() == 1 and \
                len(out) == self.n and \
                (out.dtype == want or
                 (out.dtype == torch.int32 and expr.vtype == "i64"))
            if not ok:
                raise OtbxError(3, f"project: out is a {want} tensor of n rows")
        self.out = out
        self.project_ms = None
        self.err = None

    def _run(self):
        n = self.n
        # an empty tensor has no address: with n == 0 the mask the call is
        # handed is one spare byte, and out (never written) stays NULL
        out = self.out if self.out is not None else \
            torch.empty(n, dtype=_EX_OUT_DTYPE[self.expr.vtype], device="cuda")
        nbuf = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda") \
            if self.expr.nullable else None
        nulls = nbuf[:n] if nbuf is not None else None
        err = torch.empty(1, dtype=torch.int64, device="cuda")
        e = self.expr.to_dev()
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_project", C.byref(e),
             C.c_void_p(self.sel.data_ptr()) if self.sel is not None else None,
             C.c_int64(n), C.c_int64(self.n_src),
             C.c_int32(_SORT_TYPE[out.dtype]),
             C.c_void_p(out.data_ptr()) if n > 0 else None,
             C.c_void_p(nbuf.data_ptr()) if nbuf is not None else None,
             C.c_void_p(err.data_ptr()), _stream())
        ev1.record()
        self.err = int(err.cpu().item())
        self.project_ms = ev0.elapsed_time(ev1)
        if self.err != -1:
            raise OtbxError(4, f"{PROJECT_ERRORS[self.err & 0xff]} at output "
                               f"row {self.err >> 8}")
        return [(out, nulls)]

    def explain(self):
        if self.project_ms is None:
            return None
        return {"project": self.project_ms}


# ---------------- text columns: LIKE / compare predicates, gather ----------

TEXT_TILE = 256           # rows per workgroup of otbx_text_pred
TEXT_LDS_BUDGET = 32768   # largest tile byte span the predicate stages in LDS
TEXT_GATHER_CHUNK = 256 * 1024   # rows per pass of the gather's offset scan


def _text_bytes(v, what):
    if isinstance(v, str):
        return v.encode("utf-8")
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    raise OtbxError(3, f"text: {what} is bytes or str, not {type(v).__name__}")


def like_escape(pattern, esc):
    """pattern LIKE ... ESCAPE esc → the equivalent pattern in the backslash
    convention (do_like_escape, like_match.c:247). An empty esc means no
    escape character: backslashes are doubled. esc == '\\' returns the
    pattern as it is. An esc longer than one character (UTF-8) is an error.
    Returns bytes."""
    p = _text_bytes(pattern, "a pattern")
    e = _text_bytes(esc, "an escape")
    if len(e) == 0:
        return p.replace(b"\\", b"\\\\")

    def next_char(b, i):
        i += 1
        while i < len(b) and (b[i] & 0xC0) == 0x80:
            i += 1
        return i

    if next_char(e, 0) != len(e):
        raise OtbxError(3, "invalid escape string: must be empty or one "
                           "character")
    if e == b"\\":
        return p
    out = bytearray()
    i, after = 0, False
    while i < len(p):
        j = next_char(p, i)
        if p[i:j] == e and not after:
            out += b"\\"
            after = True
        elif p[i] == 0x5C:
            out += b"\\" if after else b"\\\\"
            after = False
        else:
            out += p[i:j]
            after = False
        i = j
    return bytes(out)


class GpuText:
    """A variable-width text column on the device (otbx_textcol): `bytes`
    (uint8), `offs` (int64, n + 1 byte offsets; row i is
    bytes[offs[i]:offs[i+1]]) and `nulls` (uint8, nonzero = NULL, or None).
    GpuText(values) stages a list of bytes / str (UTF-8 encoded) / None;
    GpuText(bytes=, offs=, nulls=) adopts existing tensors, so offs[a:b+1]
    over the same bytes is a free slice."""

    def __init__(self, values=None, *, bytes=None, offs=None, nulls=None):
        if values is not None:
            if bytes is not None or offs is not None or nulls is not None:
                raise OtbxError(3, "text: values or tensors, not both")
            import numpy as np
            rows = [b"" if v is None else _text_bytes(v, "a value")
                    for v in values]
            lens = np.fromiter((len(r) for r in rows), dtype=np.int64,
                               count=len(rows))
            o = np.zeros(len(rows) + 1, dtype=np.int64)
            np.cumsum(lens, out=o[1:])
            flat = np.frombuffer(b"".join(rows), dtype=np.uint8)
            bytes = torch.from_numpy(flat.copy()).cuda()
            offs = torch.from_numpy(o).cuda()
            if any(v is None for v in values):
                m = np.fromiter((v is None for v in values), dtype=np.uint8,
                                count=len(rows))
                nulls = torch.from_numpy(m).cuda()
        for t, dt, what in ((bytes, torch.uint8, "bytes"),
                            (offs, torch.int64, "offs")):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or \
                    t.dim() != 1 or not t.is_contiguous():
                raise OtbxError(3, f"text: {what} is a contiguous 1-D {dt} "
                                   "tensor")
        if len(offs) < 1:
            raise OtbxError(3, "text: offs holds n + 1 entries")
        if nulls is not None and (not isinstance(nulls, torch.Tensor) or
                                  nulls.dtype != torch.uint8 or
                                  nulls.dim() != 1 or
                                  len(nulls) != len(offs) - 1 or
                                  not nulls.is_contiguous()):
            raise OtbxError(3, "text: a null mask is a uint8 tensor of the "
                               "column's length")
        self.bytes, self.offs, self.nulls = bytes, offs, nulls

    def __len__(self):
        return len(self.offs) - 1

    def col(self):
        """The otbx_textcol of this column."""
        c = TextColDev()
        c.bytes = self.bytes.data_ptr() if len(self.bytes) else None
        c.offs = self.offs.data_ptr()
        c.nulls = self.nulls.data_ptr() \
            if self.nulls is not None and len(self) else None
        c.nbytes = len(self.bytes)
        return c

    def slice(self, a, b):
        """Rows [a, b) as a view: no byte is copied."""
        n = len(self)
        if not (isinstance(a, int) and isinstance(b, int) and 0 <= a <= b <= n):
            raise OtbxError(3, "text: slice outside the column")
        return GpuText(bytes=self.bytes, offs=self.offs[a:b + 1],
                       nulls=None if self.nulls is None else self.nulls[a:b])

    def to_list(self):
        """The rows on the host: bytes, None under a NULL. Offsets are
        clamped exactly as the kernels clamp them."""
        raw = self.bytes.cpu().numpy().tobytes()
        o = self.offs.cpu().tolist()
        m = None if self.nulls is None else self.nulls.cpu().tolist()
        nb = len(raw)
        out = []
        for i in range(len(o) - 1):
            if m is not None and m[i]:
                out.append(None)
                continue
            s = min(max(o[i], 0), nb)
            e = min(max(o[i + 1], 0), nb)
            out.append(raw[s:e] if e > s else b"")
        return out

    def gather(self, perm):
        """Row perm[j] of this column as row j of a new GpuText (a selection
        from GpuFilter, a permutation from GpuSort, row ids of a join:
        entries may repeat and are clamped into the column). One host
        synchronisation: the total byte count, to size the new bytes."""
        if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 \
                or perm.dim() != 1 or not perm.is_contiguous():
            raise OtbxError(3, "text: perm is a contiguous int64 tensor of "
                               "row ids")
        n, n_src = len(perm), len(self)
        if n > 0 and n_src == 0:
            raise OtbxError(3, "text: gather from an empty column")
        L = lib()
        wsb = C.c_size_t(0)
        check(L.otbx_text_gather_workspace_bytes(C.c_int64(n), C.byref(wsb)),
              "otbx_text_gather_workspace_bytes")
        ws = torch.empty(max(wsb.value, 8) // 8, dtype=torch.int64,
                         device="cuda")
        doffs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        c = self.col()
        pp = C.c_void_p(perm.data_ptr()) if n > 0 else None
        call("otbx_text_gather_offsets", C.byref(c), C.c_int64(n_src), pp,
             C.c_int64(n), C.c_void_p(ws.data_ptr()), C.c_size_t(wsb.value),
             C.c_void_p(doffs.data_ptr()), _stream())
        total = int(doffs[n].cpu().item())
        dbytes = torch.empty(total, dtype=torch.uint8, device="cuda")
        call("otbx_text_gather_bytes", C.byref(c), C.c_int64(n_src), pp,
             C.c_int64(n), C.c_void_p(doffs.data_ptr()),
             C.c_void_p(dbytes.data_ptr()) if total > 0 else None,
             C.c_int64(total), _stream())
        nulls = None
        if self.nulls is not None:
            # otbx_gather_u8 does not clamp its row ids
            nulls = gather(self.nulls, torch.clamp(perm, 0, n_src - 1)) \
                if n > 0 else torch.empty(0, dtype=torch.uint8, device="cuda")
        return GpuText(bytes=dbytes, offs=doffs, nulls=nulls)

    def rank(self, *others):
        """Ordered dictionary codes of this column, ranked jointly with
        `others` (up to four columns in all): runs a GpuTextRank node and
        returns its TextRank."""
        node = GpuTextRank([self, *others])
        node.BeginCustomScan()
        try:
            return node.ExecCustomScan()
        finally:
            node.EndCustomScan()


class TextRank:
    """What GpuTextRank yields. `codes`: one int64 tensor per input column,
    views of one buffer — the dense rank of every row's string among the
    distinct non-NULL strings of all the columns, -1 under a NULL.
    `ndistinct`: D. `dict_rows`: int64[D], the first virtual row (the
    columns numbered through, column 0 first) holding each code. `rounds`:
    refinement rounds the kernels ran."""

    def __init__(self, columns, codes, ndistinct, dict_rows, rounds):
        self.columns = columns
        self.codes = codes
        self.ndistinct = ndistinct
        self.dict_rows = dict_rows
        self.rounds = rounds
        self._dict = None

    def dictionary(self):
        """The distinct strings in order, as a GpuText of D rows without a
        mask: row c is the string of code c. The inputs' bytes are not
        copied: each column gathers its own first occurrences, and the
        dictionary-sized pieces are put in order by one more gather."""
        if self._dict is not None:
            return self._dict
        d = self.ndistinct
        if d == 0:
            self._dict = GpuText(
                bytes=torch.empty(0, dtype=torch.uint8, device="cuda"),
                offs=torch.zeros(1, dtype=torch.int64, device="cuda"))
            return self._dict
        parts, where = [], []
        start = 0
        for col in self.columns:
            end = start + len(col)
            pos = torch.nonzero((self.dict_rows >= start) &
                                (self.dict_rows < end)).reshape(-1)
            if len(pos):
                g = col.gather((self.dict_rows[pos] - start).contiguous())
                parts.append(g)
                where.append(pos)
            start = end
        if len(parts) == 1:
            out = parts[0]
        else:
            base, offs = 0, []
            for g in parts:
                offs.append(g.offs[:-1] + base)
                base += int(len(g.bytes))
            offs.append(torch.tensor([base], dtype=torch.int64, device="cuda"))
            cat = GpuText(bytes=torch.cat([g.bytes for g in parts]),
                          offs=torch.cat(offs))
            inv = torch.empty(d, dtype=torch.int64, device="cuda")
            inv[torch.cat(where)] = torch.arange(d, dtype=torch.int64,
                                                 device="cuda")
            out = cat.gather(inv)
        self._dict = GpuText(bytes=out.bytes, offs=out.offs)
        return self._dict

    def decode(self, codes):
        """codes (int64 tensor) → GpuText: the dictionary's row per code,
        NULL for a code of -1 (what a NULL row got, and what MIN / MAX over
        no row leaves)."""
        if not isinstance(codes, torch.Tensor) or codes.dtype != torch.int64 \
                or codes.dim() != 1:
            raise OtbxError(3, "text rank: codes is an int64 tensor")
        codes = codes.contiguous()
        nulls = (codes < 0).to(torch.uint8)
        if self.ndistinct == 0:
            return GpuText(
                bytes=torch.empty(0, dtype=torch.uint8, device="cuda"),
                offs=torch.zeros(len(codes) + 1, dtype=torch.int64,
                                 device="cuda"),
                nulls=torch.ones(len(codes), dtype=torch.uint8,
                                 device="cuda"))
        g = self.dictionary().gather(codes)   # -1 is clamped to row 0
        return GpuText(bytes=g.bytes, offs=g.offs, nulls=nulls)


class GpuTextRank(CustomScanState):
    """Text as a sort, group or join key (otbx_text_rank): an
    order-preserving dictionary encoding of one to four GpuText columns,
    ranked jointly so that equal strings of different columns get one code.
    code(a) < code(b) ⇔ a < b under C collation (varstr_cmp with
    lc_collate_is_c, varlena.c:1614-1629; bttextcmp varlena.c:1998),
    code(a) == code(b) ⇔ texteq; NULL rows get -1 and keep their mask.
    Yields ONE tuple, a TextRank. The call is synchronous (one int64 read
    back per refinement round); build a dictionary once per column.

    The codes are an ordinary int64 key column, the column's mask is the
    mask the other nodes take, and those nodes do not change:
      ORDER BY t DESC NULLS FIRST, x
          GpuSort([r.codes[0], x], descending=[True, False],
                  nulls_first=[True, None], nulls=[t.nulls, None])
      GROUP BY t
          GpuGroupAgg([r.codes[0]], aggs, key_nulls=[t.nulls]) or
          GpuHashAgg(r.codes[0], vals, key_null=t.nulls), then
          r.decode(group keys)
      MIN(t) / MAX(t)  (text_smaller / text_larger, varlena.c:2819-2840)
          MIN / MAX over the codes with t.nulls as the value mask, then
          r.decode(result)
      a.t = b.t
          r = a.t.rank(b.t); GpuHashJoin(r.codes[0], r.codes[1],
          build_null=a.t.nulls, probe_null=b.t.nulls)
    Codes are local to this call (to one DataNode);
    fragment.merge_text_dictionaries maps them to global ones."""

    def __init__(self, columns):
        super().__init__()
        if isinstance(columns, GpuText):
            columns = [columns]
        self.columns = list(columns)
        if not 1 <= len(self.columns) <= MAX_TEXT_RANK_COLS:
            raise OtbxError(3, "text rank: 1..%d columns" % MAX_TEXT_RANK_COLS)
        for c in self.columns:
            if not isinstance(c, GpuText):
                raise OtbxError(3, "text rank: every column is a GpuText")
        self.n_total = sum(len(c) for c in self.columns)
        if self.n_total > 2**31 - 1:
            raise OtbxError(3, "text rank: more than 2^31 - 1 rows")
        self.result = None
        self.rank_ms = None

    def textset(self):
        """The otbx_textset handed to otbx_text_rank."""
        ts = TextSetDev()
        ts.ncols = len(self.columns)
        for i, c in enumerate(self.columns):
            ts.col[i] = c.col()
            ts.n[i] = len(c)
        return ts

    def _run(self):
        import time
        L = lib()
        n = self.n_total
        wsb = C.c_size_t(0)
        check(L.otbx_text_rank_workspace_bytes(C.c_int64(n), C.byref(wsb)),
              "otbx_text_rank_workspace_bytes")
        ws = torch.empty((wsb.value + 15) // 16 * 2, dtype=torch.int64,
                         device="cuda")
        # an empty tensor has no address: one spare entry behind each output
        codes = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        drow = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        nd = torch.zeros(1, dtype=torch.int64, device="cuda")
        rounds = C.c_int32(0)
        ts = self.textset()
        t0 = time.perf_counter()
        call("otbx_text_rank", C.byref(ts), C.c_void_p(ws.data_ptr()),
             C.c_size_t(wsb.value), C.c_void_p(codes.data_ptr()),
             C.c_void_p(drow.data_ptr()), C.c_void_p(nd.data_ptr()),
             C.byref(rounds), _stream())
        # the call returns with the stream drained: a host clock is exact
        self.rank_ms = (time.perf_counter() - t0) * 1e3
        d = int(nd.cpu().item())
        views, start = [], 0
        for c in self.columns:
            views.append(codes[start:start + len(c)])
            start += len(c)
        self.result = TextRank(self.columns, views, d, drow[:d], rounds.value)
        return [self.result]

    def explain(self):
        if self.result is None:
            return None
        return {"text_rank": self.rank_ms, "rounds": self.result.rounds}


class GpuTextPred(CustomScanState):
    """One predicate over a text column (textlike / textnlike, like.c:269;
    texteq … text_ge under C collation, varlena.c:1874): `text` OP `rhs`
    with op "like", "not like", "=", "<>", "<", "<=", ">" or ">="; rhs a
    constant (bytes / str, at most 256 bytes; a LIKE pattern in the backslash
    convention — see like_escape) or, for the comparisons, a second GpuText
    of the same length. With `sel`, the int64 selection GpuFilter yielded,
    only the selected rows are evaluated, read through it. encoding "utf8"
    or "sb" decides how `_` and the restart after `%` advance. Yields ONE
    tuple (bool_u8, nulls_or_None); term() is that as a GpuFilter term.
    Contract in include/otbx.h (otbx_text_pred)."""

    def __init__(self, text, op, rhs, sel=None, encoding="utf8"):
        super().__init__()
        if not isinstance(text, GpuText):
            raise OtbxError(3, "text predicate: the left operand is a GpuText")
        if op not in TXT_OPS:
            raise OtbxError(3, f"text predicate: unknown operator {op!r}")
        if encoding not in TEXT_ENCODINGS:
            raise OtbxError(3, f"text predicate: unknown encoding {encoding!r}")
        if isinstance(rhs, GpuText):
            if op in ("like", "not like"):
                raise OtbxError(3, "text predicate: a LIKE pattern is a "
                                   "constant")
            if len(rhs) != len(text):
                raise OtbxError(3, "text predicate: columns differ in length")
        else:
            rhs = _text_bytes(rhs, "the right operand")
            if len(rhs) > MAX_TEXT_CONST:
                raise OtbxError(3, "text predicate: a constant has at most "
                                   f"{MAX_TEXT_CONST} bytes")
            if op in ("like", "not like"):
                # a backslash that escapes nothing (odd run at the end)
                k = len(rhs) - len(rhs.rstrip(b"\\"))
                if k % 2 == 1:
                    raise OtbxError(3, "LIKE pattern must not end with "
                                       "escape character")
        if sel is not None and (not isinstance(sel, torch.Tensor) or
                                sel.dtype != torch.int64 or sel.dim() != 1 or
                                not sel.is_contiguous()):
            raise OtbxError(3, "text predicate: sel is an int64 tensor of "
                               "row ids")
        self.text, self.op, self.rhs = text, op, rhs
        self.sel, self.encoding = sel, encoding
        self.n_src = len(text)
        self.n = len(sel) if sel is not None else self.n_src
        if self.n > 0 and self.n_src == 0:
            raise OtbxError(3, "text predicate: sel over an empty column")
        self.nullable = text.nulls is not None or \
            (isinstance(rhs, GpuText) and rhs.nulls is not None)
        self.value = None
        self.nulls = None
        self.pred_ms = None

    def pred(self):
        """The otbx_textpred handed to otbx_text_pred (and the right column
        it points to, which must outlive the call)."""
        p = TextPredDev()
        p.left = self.text.col()
        p.op = TXT_OPS[self.op]
        p.encoding = TEXT_ENCODINGS[self.encoding]
        right = None
        if isinstance(self.rhs, GpuText):
            right = self.rhs.col()
            p.right = C.pointer(right)
        else:
            p.clen = len(self.rhs)
            C.memmove(p.cbytes, self.rhs, len(self.rhs))
        return p, right

    def _run(self):
        n = self.n
        # an empty tensor has no address: one spare byte behind each output
        obuf = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        nbuf = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda") \
            if self.nullable else None
        p, _right = self.pred()   # _right: what p.right points to
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
        call("otbx_text_pred", C.byref(p),
             C.c_void_p(self.sel.data_ptr())
             if self.sel is not None and n > 0 else None,
             C.c_int64(n), C.c_int64(self.n_src), C.c_void_p(obuf.data_ptr()),
             C.c_void_p(nbuf.data_ptr()) if nbuf is not None else None,
             _stream())
        ev1.record()
        # no synchronisation here: explain() reads the events when asked
        self._ev = (ev0, ev1)
        self.pred_ms = None
        self.value = obuf[:n]
        self.nulls = nbuf[:n] if nbuf is not None else None
        return [(self.value, self.nulls)]

    def term(self):
        """The predicate as a term of GpuFilter's qual: TRUE rows pass, FALSE
        and NULL rows do not (runs the node if it has not run)."""
        if self.value is None:
            self._run()
        return qual_term(self.value, "=", 1, nulls=self.nulls)

    def explain(self):
        if self.value is None:
            return None
        if self.pred_ms is None:
            self._ev[1].synchronize()
            self.pred_ms = self._ev[0].elapsed_time(self._ev[1])
        return {"text_pred": self.pred_ms}


class GpuHashAgg(CustomScanState):
    """Composable HashAggregate over i64 keys / f64 values with full NULL
    semantics (execGrouping.c:295 + nodeAgg.c:743). Inputs: device tensors;
    null bitmaps optional uint8 tensors (1 = NULL)."""

    def __init__(self, keys, vals, key_null=None, val_null=None):
        super().__init__()
        self.keys, self.vals = keys, vals
        self.key_null, self.val_null = key_null, val_null

    def _run(self):
        import numpy as np
        L = lib()
        n = len(self.keys)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_agg_i64_workspace_bytes(C.c_int64(n), C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device="cuda")
        out = torch.empty(max(n, 1) * 40, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")
        kn = C.c_void_p(self.key_null.data_ptr()) if self.key_null is not None else None
        vn = C.c_void_p(self.val_null.data_ptr()) if self.val_null is not None else None
        call("otbx_agg_i64", C.c_void_p(self.keys.data_ptr()), kn,
             C.c_void_p(self.vals.data_ptr()), vn, C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), _stream())
        ngroups = int(ng.cpu().item())
        dt = np.dtype([("key", "i8"), ("count_star", "i8"), ("count_v", "i8"),
                       ("sum_v", "f8"), ("key_isnull", "i4"), ("sum_isnull", "i4")])
        arr = out[: ngroups * 40].cpu().numpy().view(dt).copy()
        arr.sort(order=["key_isnull", "key"])
        return list(arr)


VAR_GROUP_DTYPE = [("key", "i8"), ("count_star", "i8"), ("count_v", "i8"),
                   ("sum_v", "f8"), ("sxx", "f8"),
                   ("key_isnull", "i4"), ("sum_isnull", "i4")]


class GpuHashAggVar(CustomScanState):
    """HashAggregate carrying the full float8_accum state [N, Sx, Sxx]
    (float.c:2823) per group — the partial state of var_pop / var_samp /
    stddev_pop / stddev_samp over a float8 column. Grouping and NULL
    semantics as GpuHashAgg; rows are otbx_var_group records sorted by
    (key_isnull, key). Finalize with var_pop(N, Sxx) etc. below."""

    def __init__(self, keys, vals, key_null=None, val_null=None):
        super().__init__()
        self.keys, self.vals = keys, vals
        self.key_null, self.val_null = key_null, val_null

    def _run(self):
        import numpy as np
        L = lib()
        n = len(self.keys)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_agg_i64_var_workspace_bytes(C.c_int64(n),
                                                 C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        out = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")

        def vp(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        call("otbx_agg_i64_var", vp(self.keys), vp(self.key_null),
             vp(self.vals), vp(self.val_null), C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), _stream())
        ngroups = int(ng.cpu().item())
        dt = np.dtype(VAR_GROUP_DTYPE)
        arr = out[: ngroups * 48].cpu().numpy().view(dt).copy()
        # (key_isnull, key) only: sxx may be NaN and must not take part
        arr = arr[np.lexsort((arr["key"], arr["key_isnull"]))]
        return list(arr)


# float8 variance finalizers over the [N, Sx, Sxx] state (float.c:3011-3096).
# None = SQL NULL. Sxx is non-negative (or NaN) by construction.

def var_pop(N, Sxx):
    """float8_var_pop (float.c:3011): NULL when N == 0."""
    N, Sxx = float(N), float(Sxx)
    if N == 0.0:
        return None
    return Sxx / N


def var_samp(N, Sxx):
    """float8_var_samp (float.c:3033): NULL when N <= 1."""
    N, Sxx = float(N), float(Sxx)
    if N <= 1.0:
        return None
    return Sxx / (N - 1.0)


def stddev_pop(N, Sxx):
    """float8_stddev_pop (float.c:3055): NULL when N == 0."""
    v = var_pop(N, Sxx)
    return None if v is None else math.sqrt(v)


def stddev_samp(N, Sxx):
    """float8_stddev_samp (float.c:3077): NULL when N <= 1."""
    v = var_samp(N, Sxx)
    return None if v is None else math.sqrt(v)


class GpuHashAggDec(CustomScanState):
    """Exact decimal aggregate: scaled-int64 values, int128 sum
    (Int128AggState semantics, numeric.c:5072/:4998/:5365). Bit-exact —
    rows carry .sum128 as a Python int."""

    def __init__(self, keys, vals, key_null=None, val_null=None):
        super().__init__()
        self.keys, self.vals = keys, vals
        self.key_null, self.val_null = key_null, val_null

    def _run(self):
        import numpy as np
        L = lib()
        n = len(self.keys)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_agg_i64_dec_workspace_bytes(C.c_int64(n),
                                                 C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        out = torch.empty(max(n, 1) * 48, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")

        def vp(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        call("otbx_agg_i64_dec", vp(self.keys), vp(self.key_null),
             vp(self.vals), vp(self.val_null), C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), _stream())
        ngroups = int(ng.cpu().item())
        dt = np.dtype([("key", "i8"), ("count_star", "i8"), ("count_v", "i8"),
                       ("sum_hi", "i8"), ("sum_lo", "u8"),
                       ("key_isnull", "i4"), ("sum_isnull", "i4")])
        arr = out[: ngroups * 48].cpu().numpy().view(dt).copy()
        arr.sort(order=["key_isnull", "key"])
        rows = []
        for r in arr:
            d = {k: int(r[k]) for k in dt.names}
            d["sum128"] = (int(r["sum_hi"]) << 64) | int(r["sum_lo"])
            rows.append(d)
        return rows


def _keyset_dev(key_tensors, null_tensors=None):
    """Build an otbx_keyset (device pointers) from torch tensors."""
    ks = KeysetDev()
    ks.nkeys = len(key_tensors)
    for c, k in enumerate(key_tensors):
        ks.keys[c] = k.data_ptr()
        nt = None if null_tensors is None else null_tensors[c]
        ks.nulls[c] = nt.data_ptr() if nt is not None else None
    return ks


class GpuHashAggN(CustomScanState):
    """N-key (1..8) composable HashAggregate: groups carry the defining
    ROW INDEX (the representative-tuple pattern, execGrouping.c
    firstTuple); the caller reads key values back through the index."""

    def __init__(self, key_tensors, vals, null_tensors=None, val_null=None):
        super().__init__()
        self.keys, self.vals = key_tensors, vals
        self.nulls, self.vn = null_tensors, val_null

    def _run(self):
        import numpy as np
        L = lib()
        n = len(self.vals)
        ks = _keyset_dev(self.keys, self.nulls)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_agg_i64n_workspace_bytes(C.c_int64(n),
                                              C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        out = torch.empty(max(n, 1) * 40, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")
        vn = C.c_void_p(self.vn.data_ptr()) if self.vn is not None else None
        call("otbx_agg_i64n", C.byref(ks),
             C.c_void_p(self.vals.data_ptr()), vn, C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), _stream())
        ngroups = int(ng.cpu().item())
        dt = np.dtype([("row_idx", "i8"), ("count_star", "i8"),
                       ("count_v", "i8"), ("sum_v", "f8"),
                       ("sum_isnull", "i4"), ("_pad", "i4")])
        arr = out[: ngroups * 40].cpu().numpy().view(dt).copy()
        arr.sort(order="row_idx")
        return list(arr)


class GpuHashJoinN(CustomScanState):
    """N-key (1..8) HashJoin, all six join types; pair encoding and
    overflow contract as GpuHashJoin."""

    def __init__(self, bkeys, pkeys, join_type=0, bnulls=None, pnulls=None,
                 cap_pairs=None):
        super().__init__()
        self.bkeys, self.pkeys = bkeys, pkeys
        self.bnulls, self.pnulls = bnulls, pnulls
        self.join_type = JOIN_TYPES.get(join_type, join_type) \
            if isinstance(join_type, str) else join_type
        self.cap_pairs = cap_pairs

    def _run(self):
        L = lib()
        nb = len(self.bkeys[0]) if self.bkeys else 0
        npr = len(self.pkeys[0]) if self.pkeys else 0
        bks = _keyset_dev(self.bkeys, self.bnulls)
        pks = _keyset_dev(self.pkeys, self.pnulls)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_join_i64n_workspace_bytes(C.c_int64(nb), C.c_int64(npr),
                                               C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8,
                         device="cuda")
        cap = self.cap_pairs if self.cap_pairs \
            else max(4 * max(nb, npr) + nb + npr, 64)
        ob = torch.empty(cap, dtype=torch.int64, device="cuda")
        op = torch.empty(cap, dtype=torch.int64, device="cuda")
        npairs = torch.zeros(1, dtype=torch.int64, device="cuda")
        call("otbx_join_i64n", C.byref(bks), C.c_int64(nb), C.byref(pks),
             C.c_int64(npr), C.c_int32(self.join_type),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(ob.data_ptr()), C.c_void_p(op.data_ptr()),
             C.c_int64(cap), C.c_void_p(npairs.data_ptr()), _stream())
        n = int(npairs.cpu().item())
        if n > cap:
            raise OtbxError(3, f"join pair overflow: {n} > cap {cap}")
        return list(zip(ob[:n].cpu().numpy().tolist(),
                        op[:n].cpu().numpy().tolist()))


def dec_avg(sum128, count, extra_scale=0):
    """Exact AVG finalizer for the decimal aggregate's int128 state
    (Int128AggState {N, sumX}, numeric.c:5072): returns the scaled-int64
    average round-half-up away from zero — the reference's numeric
    rounding (round_var HALF_ADJUST_ROUND, numeric.c:724,1743,7145 via
    div_var). extra_scale shifts the result scale by 10^extra_scale
    relative to the input scale (e.g. cents in -> tenth-cents out with
    extra_scale=1). Python ints are unbounded, so this is exact for any
    int128 state; the combine phase sums states exactly first. Raises on
    count == 0 (AVG over no rows is NULL at the SQL level — the caller
    checks sum_isnull/count first, nodeAgg.c finalize semantics)."""
    if count <= 0:
        raise OtbxError(3, "dec_avg: count must be positive (NULL AVG is "
                           "decided by the caller)")
    num = sum128 * (10 ** extra_scale)
    if num >= 0:
        return (2 * num + count) // (2 * count)
    return -((2 * (-num) + count) // (2 * count))


JOIN_TYPES = {"inner": 0, "left": 1, "semi": 2, "anti": 3, "right": 4,
              "full": 5}


class GpuHashJoin(CustomScanState):
    """Composable HashJoin on i64 keys (nodeHash.c/nodeHashjoin.c), all six
    join types (HJ_* fill states, nodeHashjoin.c:139-144) and an optional
    second key column (multi-key combine, nodeHash.c:2059). Emits
    (build_idx, probe_idx) pairs, -1 = NULL-fill side (see include/otbx.h);
    result-set parity (order-free). join_type 0/'inner' with a single key
    routes through the optimized partitioned inner-join path."""

    def __init__(self, build_keys, probe_keys, build_null=None, probe_null=None,
                 cap_pairs=None, join_type=0, build_keys2=None,
                 probe_keys2=None, build_null2=None, probe_null2=None):
        super().__init__()
        self.bk, self.pk = build_keys, probe_keys
        self.bn, self.pn = build_null, probe_null
        self.bk2, self.pk2 = build_keys2, probe_keys2
        self.bn2, self.pn2 = build_null2, probe_null2
        self.cap_pairs = cap_pairs
        self.join_type = JOIN_TYPES.get(join_type, join_type) \
            if isinstance(join_type, str) else join_type

    def _run(self):
        L = lib()
        nb, npr = len(self.bk), len(self.pk)
        jt = self.join_type
        two_key = self.bk2 is not None
        ext = jt != 0 or two_key
        ws_bytes = C.c_size_t(0)
        if ext:
            check(L.otbx_join_ext_workspace_bytes(
                C.c_int64(nb), C.c_int64(npr), C.byref(ws_bytes)))
        else:
            check(L.otbx_join_i64_workspace_bytes(
                C.c_int64(nb), C.c_int64(npr), C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device="cuda")
        # outer fills can exceed the match count: pairs <= matches + nb + np
        cap = self.cap_pairs if self.cap_pairs \
            else max(4 * max(nb, npr) + nb + npr, 64)
        ob = torch.empty(cap, dtype=torch.int64, device="cuda")
        op = torch.empty(cap, dtype=torch.int64, device="cuda")
        npairs = torch.zeros(1, dtype=torch.int64, device="cuda")

        def vp(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        if two_key:
            call("otbx_join_i64x2", vp(self.bk), vp(self.bn), vp(self.bk2),
                 vp(self.bn2), C.c_int64(nb), vp(self.pk), vp(self.pn),
                 vp(self.pk2), vp(self.pn2), C.c_int64(npr), C.c_int32(jt),
                 C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
                 vp(ob), vp(op), C.c_int64(cap), vp(npairs), _stream())
        elif ext:
            call("otbx_join_i64_ext", vp(self.bk), vp(self.bn), C.c_int64(nb),
                 vp(self.pk), vp(self.pn), C.c_int64(npr), C.c_int32(jt),
                 C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
                 vp(ob), vp(op), C.c_int64(cap), vp(npairs), _stream())
        else:
            call("otbx_join_i64", vp(self.bk), vp(self.bn), C.c_int64(nb),
                 vp(self.pk), vp(self.pn), C.c_int64(npr),
                 C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
                 vp(ob), vp(op), C.c_int64(cap), vp(npairs), _stream())
        n = int(npairs.cpu().item())
        if n > cap:
            raise OtbxError(3, f"join pair overflow: {n} > cap {cap}")
        return list(zip(ob[:n].cpu().numpy().tolist(),
                        op[:n].cpu().numpy().tolist()))


class GpuHashAgg2(CustomScanState):
    """Two-key composable HashAggregate (multi-key GROUP BY,
    execGrouping.c:295 with NULL==NULL grouping :525). Returns rows sorted
    by (k1_isnull, k1, k2_isnull, k2) for deterministic comparison."""

    def __init__(self, keys1, keys2, vals, key1_null=None, key2_null=None,
                 val_null=None):
        super().__init__()
        self.k1, self.k2, self.vals = keys1, keys2, vals
        self.n1, self.n2, self.vn = key1_null, key2_null, val_null

    def _run(self):
        import numpy as np
        L = lib()
        n = len(self.k1)
        ws_bytes = C.c_size_t(0)
        check(L.otbx_agg_i64x2_workspace_bytes(C.c_int64(n),
                                               C.byref(ws_bytes)))
        ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device="cuda")
        out = torch.empty(max(n, 1) * 56, dtype=torch.uint8, device="cuda")
        ng = torch.zeros(1, dtype=torch.int64, device="cuda")

        def vp(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        call("otbx_agg_i64x2", vp(self.k1), vp(self.n1), vp(self.k2),
             vp(self.n2), vp(self.vals), vp(self.vn), C.c_int64(n),
             C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes.value),
             C.c_void_p(out.data_ptr()), C.c_void_p(ng.data_ptr()), _stream())
        ngroups = int(ng.cpu().item())
        dt = np.dtype([("key1", "i8"), ("key2", "i8"), ("count_star", "i8"),
                       ("count_v", "i8"), ("sum_v", "f8"),
                       ("key1_isnull", "i4"), ("key2_isnull", "i4"),
                       ("sum_isnull", "i4"), ("_pad", "i4")])
        arr = out[: ngroups * 56].cpu().numpy().view(dt).copy()
        arr.sort(order=["key1_isnull", "key1", "key2_isnull", "key2"])
        return list(arr)

"""ctypes binding for libotbx.so (the C-ABI in include/otbx.h).

The .so is built in-tree (opentenbase_amd/csrc/Makefile, hipcc gfx950) and
travels with the repo snapshot. On a machine WITH a GPU, a missing or
unloadable extension is a hard error — the HIP path is the only compute path
(no CPU fallback; the oracle is test infrastructure only).
"""
import ctypes as C
import os
import subprocess

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.path.join(_DIR, "libotbx.so")

OTBX_OK = 0
_STATUS = {0: "ok", 1: "hip runtime error", 2: "out of memory",
           3: "invalid argument", 4: "value out of range", 5: "no gpu"}


class OtbxError(RuntimeError):
    """Analog of ereport(ERROR): any non-OK status from the C-ABI."""

    def __init__(self, status, what=""):
        self.status = status
        super().__init__(f"otbx error {status} ({_STATUS.get(status, '?')}) {what}")


Q1_DICT_MAX = 256   # OTBX_Q1_DICT_MAX


class Q1CodeDesc(C.Structure):
    """otbx_q1code_desc (include/otbx.h): layout of the packed Q1 code word,
    72 bytes."""
    _fields_ = [
        ("date_base", C.c_int32),
        ("date_off", C.c_int32), ("date_bits", C.c_int32),
        ("gid_off", C.c_int32), ("gid_bits", C.c_int32),
        ("qty_off", C.c_int32), ("qty_bits", C.c_int32),
        ("disc_off", C.c_int32), ("disc_bits", C.c_int32),
        ("tax_off", C.c_int32), ("tax_bits", C.c_int32),
        ("nqty", C.c_int32), ("ndisc", C.c_int32), ("ntax", C.c_int32),
        ("gid_present", C.c_int32),
        ("dict", C.c_void_p),
    ]


class Q1PriceDesc(C.Structure):
    """otbx_q1price_desc (include/otbx.h): layout of the packed Q1 price
    word, 40 bytes."""
    _fields_ = [
        ("scale_exp", C.c_int32),
        ("mul", C.c_double),
        ("k_base", C.c_int32), ("k_off", C.c_int32), ("k_bits", C.c_int32),
        ("d_base", C.c_int32), ("d_off", C.c_int32), ("d_bits", C.c_int32),
    ]


class LineitemDev(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("l_orderkey", C.c_void_p),
        ("l_quantity", C.c_void_p), ("l_extendedprice", C.c_void_p),
        ("l_discount", C.c_void_p), ("l_tax", C.c_void_p),
        ("l_returnflag", C.c_void_p), ("l_linestatus", C.c_void_p),
        ("l_shipdate", C.c_void_p),
        ("l_partkey", C.c_void_p),
        ("q9rec", C.c_void_p),
        ("l_orderkey32", C.c_void_p),
        ("l_partkey32", C.c_void_p),
        ("q1code", C.c_void_p),
        ("q1desc", Q1CodeDesc),
        ("q1pcode", C.c_void_p),
        ("q1pdesc", Q1PriceDesc),
    ]


class OrdersDev(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("o_orderkey", C.c_void_p), ("o_custkey", C.c_void_p),
        ("o_orderdate", C.c_void_p), ("o_shippriority", C.c_void_p),
        ("okey_min", C.c_int64), ("okey_max", C.c_int64),
        ("has_minmax", C.c_int32),
        ("o_orderkey32", C.c_void_p), ("o_custkey32", C.c_void_p),
    ]


class CustomerDev(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("c_custkey", C.c_void_p), ("c_mktsegment", C.c_void_p),
    ]


class KeysetDev(C.Structure):
    """otbx_keyset (include/otbx.h): up to 8 key columns (device ptrs)."""
    _fields_ = [("nkeys", C.c_int32),
                ("keys", C.c_void_p * 8),
                ("nulls", C.c_void_p * 8)]


class SortKeyDev(C.Structure):
    """otbx_sortkey (include/otbx.h)."""
    _fields_ = [("col", C.c_void_p), ("nulls", C.c_void_p),
                ("type", C.c_int32), ("flags", C.c_int32)]


class SortSpecDev(C.Structure):
    """otbx_sortspec: up to 8 sort keys, key[0] primary."""
    _fields_ = [("nkeys", C.c_int32), ("key", SortKeyDev * 8)]


class WindowOutDev(C.Structure):
    """otbx_window_out: one device array of n entries per requested window
    function, None = not wanted."""
    _fields_ = [("row_number", C.c_void_p), ("rank", C.c_void_p),
                ("dense_rank", C.c_void_p), ("count_star", C.c_void_p),
                ("count_v", C.c_void_p), ("sum_v", C.c_void_p),
                ("sum_isnull", C.c_void_p), ("part_rows", C.c_void_p)]


FRAME_ROWS, FRAME_RANGE = 0, 1               # OTBX_FRAME_*
FB_UNBOUNDED, FB_CURRENT, FB_OFFSET = 0, 1, 2   # OTBX_FB_*
WIN_FUNCS = {"ntile": 0, "lag": 1, "lead": 2, "first_value": 3,
             "last_value": 4, "nth_value": 5, "count_star": 6, "count": 7,
             "sum": 8, "min": 9, "max": 10}     # OTBX_WF_*
MAX_WINCALLS = 8                                # OTBX_MAX_WINCALLS


class FrameDev(C.Structure):
    """otbx_frame (include/otbx.h): one window frame, 32 bytes."""
    _fields_ = [("units", C.c_int32), ("start_kind", C.c_int32),
                ("end_kind", C.c_int32), ("_pad", C.c_int32),
                ("start_off", C.c_int64), ("end_off", C.c_int64)]


class WinCallDev(C.Structure):
    """otbx_wincall: one function call of a window-frame list, 80 bytes."""
    _fields_ = [("col", C.c_void_p), ("nulls", C.c_void_p),
                ("out", C.c_void_p), ("out_hi", C.c_void_p),
                ("out_null", C.c_void_p),
                ("param", C.c_int64), ("def_i", C.c_int64),
                ("def_f", C.c_double), ("def_isnull", C.c_int32),
                ("func", C.c_int32), ("type", C.c_int32),
                ("_pad", C.c_int32)]


assert C.sizeof(FrameDev) == 32 and C.sizeof(WinCallDev) == 80

AGG_FUNCS = {"count_star": 0, "count": 1, "sum": 2, "min": 3, "max": 4}
MAX_AGGS = 8   # OTBX_MAX_AGGS


class AggCallDev(C.Structure):
    """otbx_aggcall (include/otbx.h): one aggregate of a GroupAggregate
    target list, 48 bytes."""
    _fields_ = [("col", C.c_void_p), ("nulls", C.c_void_p),
                ("out", C.c_void_p), ("out_hi", C.c_void_p),
                ("out_null", C.c_void_p),
                ("func", C.c_int32), ("type", C.c_int32)]


class AggCallsDev(C.Structure):
    """otbx_aggcalls: up to 8 aggregates, 392 bytes."""
    _fields_ = [("naggs", C.c_int32), ("_pad", C.c_int32),
                ("agg", AggCallDev * MAX_AGGS)]


assert C.sizeof(AggCallDev) == 48 and C.sizeof(AggCallsDev) == 392

OAGG_FUNCS = {"count_distinct": 0, "sum_distinct": 1, "percentile_disc": 2,
              "percentile_cont": 3, "mode": 4}   # OTBX_OAGG_*


class OAggCallDev(C.Structure):
    """otbx_oaggcall (include/otbx.h): one DISTINCT / ordered-set aggregate,
    40 bytes."""
    _fields_ = [("out", C.c_void_p), ("out_hi", C.c_void_p),
                ("out_null", C.c_void_p), ("fraction", C.c_double),
                ("func", C.c_int32), ("_pad", C.c_int32)]


class OAggCallsDev(C.Structure):
    """otbx_oaggcalls: up to 8 calls on one argument column, 328 bytes."""
    _fields_ = [("ncalls", C.c_int32), ("_pad", C.c_int32),
                ("call", OAggCallDev * MAX_AGGS)]


assert C.sizeof(OAggCallDev) == 40 and C.sizeof(OAggCallsDev) == 328


class QualTermDev(C.Structure):
    """otbx_qualterm (include/otbx.h): one comparison of a qual, 64 bytes."""
    _fields_ = [("col", C.c_void_p), ("nulls", C.c_void_p),
                ("rcol", C.c_void_p), ("rnulls", C.c_void_p),
                ("ci", C.c_int64), ("cf", C.c_double),
                ("type", C.c_int32), ("op", C.c_int32),
                ("clause", C.c_int32), ("_pad", C.c_int32)]


class QualDev(C.Structure):
    """otbx_qual: up to 16 terms in conjunctive normal form, 1032 bytes."""
    _fields_ = [("nterms", C.c_int32), ("term", QualTermDev * 16)]


class ExprInstrDev(C.Structure):
    """otbx_exprinstr (include/otbx.h): one postfix instruction, 48 bytes."""
    _fields_ = [("col", C.c_void_p), ("nulls", C.c_void_p),
                ("ci", C.c_int64), ("cf", C.c_double),
                ("op", C.c_int32), ("type", C.c_int32),
                ("isnull", C.c_int32), ("_pad", C.c_int32)]


class ExprDev(C.Structure):
    """otbx_expr: a postfix program of up to 32 instructions, 1544 bytes."""
    _fields_ = [("ninstr", C.c_int32), ("_pad", C.c_int32),
                ("instr", ExprInstrDev * 32)]


TXT_OPS = {"like": 0, "not like": 1, "=": 2, "<>": 3, "<": 4, "<=": 5,
           ">": 6, ">=": 7}                  # OTBX_TXT_*
TEXT_ENCODINGS = {"sb": 0, "utf8": 1}        # OTBX_TEXT_*
MAX_TEXT_CONST = 256                         # OTBX_MAX_TEXT_CONST


class TextColDev(C.Structure):
    """otbx_textcol (include/otbx.h): a variable-width text column, 32 B."""
    _fields_ = [("bytes", C.c_void_p), ("offs", C.c_void_p),
                ("nulls", C.c_void_p), ("nbytes", C.c_int64)]


class TextPredDev(C.Structure):
    """otbx_textpred: one text predicate, 312 bytes. `right` is a host
    pointer to a TextColDev (keep that object alive over the call)."""
    _fields_ = [("left", TextColDev), ("right", C.POINTER(TextColDev)),
                ("op", C.c_int32), ("encoding", C.c_int32),
                ("clen", C.c_int32), ("_pad", C.c_int32),
                ("cbytes", C.c_uint8 * MAX_TEXT_CONST)]


assert C.sizeof(TextColDev) == 32 and C.sizeof(TextPredDev) == 312

MAX_TEXT_RANK_COLS = 4                       # OTBX_MAX_TEXT_RANK_COLS


class TextSetDev(C.Structure):
    """otbx_textset: the 1..4 text columns otbx_text_rank ranks jointly,
    168 bytes."""
    _fields_ = [("ncols", C.c_int32), ("_pad", C.c_int32),
                ("col", TextColDev * MAX_TEXT_RANK_COLS),
                ("n", C.c_int64 * MAX_TEXT_RANK_COLS)]


assert C.sizeof(TextSetDev) == 168


class PartDev(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("p_partkey", C.c_void_p), ("p_type", C.c_void_p),
    ]


def build():
    """Compile the extension (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", _DIR], check=True)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise OtbxError(5, f"HIP extension not built: {_SO} missing — "
                               "run __graft_entry__.build()")
        _lib = C.CDLL(_SO)
        _lib.otbx_version.restype = C.c_char_p
        _lib.otbx_status_str.restype = C.c_char_p
        # argtypes for the pure-host sizing functions: a wrong arity from
        # a caller becomes a ctypes error instead of a segfault (the
        # compute entry points keep the explicit-ctypes call style)
        i64, u32, szp = C.c_int64, C.c_uint32, C.POINTER(C.c_size_t)
        _lib.otbx_agg_i64_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_agg_i64_var_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_join_i64_workspace_bytes.argtypes = [i64, i64, szp]
        _lib.otbx_order_groups_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_q3_workspace_bytes.argtypes = [i64, i64, i64, szp]
        _lib.otbx_q9_workspace_bytes.argtypes = [i64, i64, i64, u32, szp]
        _lib.otbx_sort_workspace_bytes.argtypes = [i64, C.c_int32, i64, szp]
        _lib.otbx_window_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_window_frame_workspace_bytes.argtypes = [i64, C.c_int32,
                                                           szp]
        _lib.otbx_window_frame_direct_default.argtypes = [
            C.POINTER(C.c_int64)]
        _lib.otbx_filter_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_group_agg_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_ordered_agg_workspace_bytes.argtypes = [i64, C.c_int32,
                                                          szp]
        _lib.otbx_text_gather_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_text_rank_workspace_bytes.argtypes = [i64, szp]
        _lib.otbx_q1code_plan.argtypes = [
            C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
            C.POINTER(Q1CodeDesc), C.POINTER(C.c_int32)]
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        _lib.otbx_q1price_plan.argtypes = [
            i32p, i64p, i64p, i64p, i64p, C.POINTER(Q1PriceDesc), i32p]
    return _lib


def check(status, what=""):
    if status != OTBX_OK:
        raise OtbxError(status, what)


def call(name, *args):
    check(getattr(lib(), name)(*args), what=name)


EXPORTED_SYMBOLS = [
    "otbx_version", "otbx_status_str", "otbx_init", "otbx_finish",
    "otbx_device_malloc", "otbx_device_free", "otbx_memcpy_h2d",
    "otbx_memcpy_d2h", "otbx_stream_sync",
    "otbx_gen_lineitem_dev", "otbx_gen_orders_dev", "otbx_gen_customer_dev",
    "otbx_gen_part_dev", "otbx_q9_workspace_bytes", "otbx_q9_partial",
    "otbx_stage_pages", "otbx_build_q9recs", "otbx_build_key32",
    "otbx_build_q1codes", "otbx_q1code_plan",
    "otbx_build_q1pcodes", "otbx_q1price_plan",
    "otbx_scan_count", "otbx_q1_partial", "otbx_q1_partial_variant",
    "otbx_q3_workspace_bytes", "otbx_q3_partial", "otbx_filter_customer",
    "otbx_topk_by_revenue",
    "otbx_order_groups_workspace_bytes", "otbx_order_groups",
    "otbx_agg_i64_workspace_bytes", "otbx_agg_i64",
    "otbx_agg_i64_var_workspace_bytes", "otbx_agg_i64_var",
    "otbx_partition_by_key", "otbx_gather_i64", "otbx_gather_f64",
    "otbx_gather_i32", "otbx_gather_u8",
    "otbx_join_i64_workspace_bytes", "otbx_join_i64",
    "otbx_join_ext_workspace_bytes", "otbx_join_i64_ext", "otbx_join_i64x2",
    "otbx_agg_i64x2_workspace_bytes", "otbx_agg_i64x2",
    "otbx_agg_i64_dec_workspace_bytes", "otbx_agg_i64_dec",
    "otbx_agg_i64n_workspace_bytes", "otbx_agg_i64n",
    "otbx_join_i64n_workspace_bytes", "otbx_join_i64n",
    "otbx_sort_workspace_bytes", "otbx_sort_perm",
    "otbx_window_workspace_bytes", "otbx_window",
    "otbx_window_frame_direct_default", "otbx_window_frame_workspace_bytes",
    "otbx_window_frame",
    "otbx_filter_workspace_bytes", "otbx_filter_sel",
    "otbx_project",
    "otbx_group_agg_workspace_bytes", "otbx_group_agg",
    "otbx_ordered_agg_workspace_bytes", "otbx_ordered_agg",
    "otbx_text_pred", "otbx_text_gather_workspace_bytes",
    "otbx_text_gather_offsets", "otbx_text_gather_bytes",
    "otbx_text_rank_workspace_bytes", "otbx_text_rank",
]

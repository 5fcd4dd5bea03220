"""CPU-side tests of the Project operator's host layers: the two reference
implementations agree on every operator, the error tables and the laziness
rules; the argument and type checks of otbx_project (pure host code — no HIP
call is reached); the expression builder; the ctypes layout; and the seeded
program generator the GPU fuzz shares."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from opentenbase_amd import _lib
from opentenbase_amd import executor as ex
from opentenbase_amd._lib import ExprDev, ExprInstrDev, OtbxError
import project_ref as pr
from project_ref import (ARITH, CMP, DIV0, I64_MAX, I64_MIN, INT4_RANGE,
                         INT8_RANGE, OVERFLOW, UNDERFLOW, assert_same,
                         ref_eval, step_eval)
from test_gpu_sort import F64_EDGE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTBX_ERR_INVALID = 3
INT32_MAX = 2**31 - 1
PTR = 0x1000   # a dummy device pointer: never dereferenced on these paths


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib._SO):
        _lib.build()
    return _lib.lib()


def both(tree, cols, sel=None, out=None, n=None):
    """ref_eval, after checking that step_eval agrees with it."""
    a = ref_eval(tree, cols, sel, out, n)
    b = step_eval(tree, cols, sel, out, n)
    assert_same(b, a, repr(tree))
    return a


def err_of(tree, cols, **kw):
    return both(tree, cols, **kw)[2]


def code_at(j, code):
    return (j << 8) | code


# ---- every operator x operand type, 20 % NULLs ----

I64_EDGE = np.array([I64_MIN, I64_MIN + 1, -2**31, -3, -1, 0, 1, 2, 7, 2**31,
                     2**32 + 5, I64_MAX - 1, I64_MAX], dtype=np.int64)


def edge_cols(seed, n=600):
    rng = np.random.default_rng(seed)

    def mask():
        return (rng.random(n) < 0.2).astype(np.uint8)
    return {
        "a": (rng.choice(I64_EDGE, n), mask()),
        "b": (rng.choice(I64_EDGE, n), mask()),
        "x": (rng.choice(F64_EDGE, n), mask()),
        "y": (rng.choice(F64_EDGE, n), mask()),
        "d": (rng.integers(-2**31, 2**31, n).astype(np.int32), mask()),
        "f": (rng.integers(0, 256, n).astype(np.uint8), mask()),
        "p": (rng.integers(0, 2, n).astype(np.int64), mask()),
        "q": (rng.integers(0, 2, n).astype(np.int64), mask()),
    }


def every_row(tree, cols):
    """Evaluate row by row so that one raising row does not hide the rest:
    the two references must agree on every single row."""
    n = len(cols["a"][0])
    for j in range(n):
        sel = np.array([j], dtype=np.int64)
        assert_same(step_eval(tree, cols, sel), ref_eval(tree, cols, sel),
                    f"{tree!r} row {j}")


BOOL_P = ("=", ("col", "p"), ("const", "i64", 1))
BOOL_Q = ("=", ("col", "q"), ("const", "i64", 1))


@pytest.mark.parametrize("op,ty", [
    (op, ty) for op in ARITH + CMP + ("neg", "abs") for ty in ("i64", "f64")
    if (op, ty) != ("%", "f64")])          # there is no float8 modulo
def test_refs_agree_arith_and_compare(op, ty):
    l, r = (("col", "a"), ("col", "b")) if ty == "i64" else \
        (("col", "x"), ("col", "y"))
    tree = (op, l) if op in ("neg", "abs") else (op, l, r)
    every_row(tree, edge_cols(1))


@pytest.mark.parametrize("tree", [
    ("cast", "f64", ("col", "a")), ("cast", "i64", ("col", "x")),
    ("cast", "f64", ("col", "d")), ("cast", "f64", ("col", "f")),
    ("+", ("col", "d"), ("col", "f")),
    ("and", BOOL_P, BOOL_Q), ("or", BOOL_P, BOOL_Q), ("not", BOOL_P),
    ("isnull", ("col", "a")), ("notnull", ("col", "x")), ("isnull", BOOL_P),
    ("case", BOOL_P, ("col", "a"), ("col", "b")),
    ("case", BOOL_P, ("col", "x"), ("col", "y")),
    ("case", BOOL_P, BOOL_Q, ("const", "bool", None)),
    ("coalesce", ("col", "a"), ("col", "b")),
    ("coalesce", ("col", "x"), ("const", "f64", 0.0)),
    ("coalesce", BOOL_P, BOOL_Q),
    ("coalesce", ("col", "a"), ("const", "i64", None)),
], ids=repr)
def test_refs_agree_casts_booleans_and_lazy_forms(tree):
    every_row(tree, edge_cols(2))


def test_kleene_truth_tables():
    """AND / OR over {TRUE, FALSE, NULL}^2 against the SQL tables."""
    vals = [(1, 0), (0, 0), (0, 1)]          # (value, isnull)
    p = np.array([v for v, _ in vals for _ in vals], dtype=np.int64)
    pm = np.array([m for _, m in vals for _ in vals], dtype=np.uint8)
    q = np.array([v for _ in vals for v, _ in vals], dtype=np.int64)
    qm = np.array([m for _ in vals for _, m in vals], dtype=np.uint8)
    cols = {"p": (p, pm), "q": (q, qm)}
    T, F, N = (1, 0), (0, 0), (0, 1)
    v, m, e = both(("and", BOOL_P, BOOL_Q), cols)
    assert list(zip(v, m)) == [T, F, N, F, F, F, N, F, N] and e == -1
    v, m, e = both(("or", BOOL_P, BOOL_Q), cols)
    assert list(zip(v, m)) == [T, T, T, T, F, N, T, N, N] and e == -1
    v, m, e = both(("not", BOOL_P), cols)
    assert list(zip(v, m))[::3] == [F, T, N]


# ---- the error tables ----

def i64c(*v):
    return np.array(v, dtype=np.int64)


def f64c(*v):
    return np.array(v, dtype=np.float64)


def ab(a, b):
    return {"a": (a, None), "b": (b, None)}


A, B = ("col", "a"), ("col", "b")


@pytest.mark.parametrize("op,a,b,code", [
    ("+", I64_MAX, 1, INT8_RANGE), ("+", I64_MIN, -1, INT8_RANGE),
    ("+", I64_MAX, 0, 0), ("+", I64_MAX, I64_MIN, 0),
    ("-", I64_MIN, 1, INT8_RANGE), ("-", 0, I64_MIN, INT8_RANGE),
    ("-", -1, I64_MIN, 0), ("-", I64_MIN, 0, 0),
    ("*", 2**32, 2**31, INT8_RANGE), ("*", I64_MIN, -1, INT8_RANGE),
    ("*", -1, I64_MIN, INT8_RANGE), ("*", 2**32, 2**30, 0),
    ("*", I64_MIN, 1, 0), ("*", -2**32, 2**31, 0), ("*", 3037000500, 3037000500, INT8_RANGE),
    ("/", 1, 0, DIV0), ("/", 0, 0, DIV0), ("/", I64_MIN, -1, INT8_RANGE),
    ("/", I64_MAX, -1, 0), ("/", I64_MIN, 1, 0),
    ("%", 1, 0, DIV0), ("%", I64_MIN, -1, 0), ("%", 7, -1, 0),
])
def test_int8_error_table(op, a, b, code):
    e = err_of((op, A, B), ab(i64c(5, a), i64c(3, b)))
    assert e == (code_at(1, code) if code else -1)


def test_int8_values():
    cols = ab(i64c(7, -7, 7, -7, I64_MIN, 5), i64c(2, 2, -2, -2, -1, -1))
    v, _, e = both(("%", A, B), cols)
    assert list(v) == [1, -1, 1, -1, 0, 0] and e == -1    # dividend's sign
    v, _, e = both(("/", A, B), ab(i64c(7, -7, 7, -7), i64c(2, 2, -2, -2)))
    assert list(v) == [3, -3, -3, 3] and e == -1          # toward zero
    assert err_of(("neg", A), ab(i64c(1, I64_MIN), i64c(0, 0))) == \
        code_at(1, INT8_RANGE)
    assert err_of(("abs", A), ab(i64c(I64_MIN), i64c(0))) == \
        code_at(0, INT8_RANGE)
    v, _, e = both(("abs", A), ab(i64c(-I64_MAX, 3), i64c(0, 0)))
    assert list(v) == [I64_MAX, 3] and e == -1


@pytest.mark.parametrize("op,a,b,code", [
    ("/", 0.0, 0.0, DIV0), ("/", np.nan, 0.0, DIV0), ("/", 1.0, -0.0, DIV0),
    ("/", np.inf, 0.0, DIV0),
    ("*", 1e-200, 1e-200, UNDERFLOW), ("*", 0.0, 1e-200, 0),
    ("*", 1e200, 1e200, OVERFLOW), ("*", np.inf, 2.0, 0),
    ("+", 1e308, 1e308, OVERFLOW), ("+", np.inf, 1.0, 0),
    ("-", -1e308, 1e308, OVERFLOW), ("-", 1.0, 1.0, 0),
    ("-", np.inf, np.inf, 0),
    ("/", 1e-300, 1e300, UNDERFLOW), ("/", 0.0, 1e300, 0),
    ("/", 1e300, 1e-300, OVERFLOW), ("/", 1.0, np.inf, UNDERFLOW),
    ("/", np.inf, 3.0, 0), ("+", np.nan, 1.0, 0), ("*", np.nan, 0.0, 0),
])
def test_float8_error_table(op, a, b, code):
    e = err_of((op, A, B), ab(f64c(5.0, a), f64c(3.0, b)))
    assert e == (code_at(1, code) if code else -1)


def test_dtoi8_table():
    cols = ab(f64c(0.5, 1.5, 2.5, -0.5, -2.0**63, 2.0**63 - 1024), f64c(*[0] * 6))
    v, _, e = both(("cast", "i64", A), cols)
    assert list(v) == [0, 2, 2, 0, I64_MIN, 2**63 - 1024] and e == -1
    for bad in (np.nan, 1e19, 2.0**63, -1e19, np.inf, -np.inf):
        assert err_of(("cast", "i64", A), ab(f64c(1.0, bad), f64c(0, 0))) == \
            code_at(1, INT8_RANGE), bad


def test_int84_on_an_i32_output():
    cols = ab(i64c(2**31 - 1, -2**31, 2**31), i64c(0, 0, 0))
    assert err_of(A, cols, out="i32") == code_at(2, INT4_RANGE)
    v, _, e = both(A, ab(i64c(2**31 - 1, -2**31), i64c(0, 0)), out="i32")
    assert v.dtype == np.int32 and list(v) == [2**31 - 1, -2**31] and e == -1
    # an earlier error wins over the output check of the same row
    assert err_of(("/", A, B), ab(i64c(2**40), i64c(0)), out="i32") == \
        code_at(0, DIV0)


# ---- laziness ----

NZ = ("<>", B, ("const", "i64", 0))
DIV = ("/", A, B)
GT1 = (">", DIV, ("const", "i64", 1))
LAZY_CASES = [
    # (name, tree, code at the first zero row of b — 0 = never raises)
    ("case_guard", ("case", NZ, DIV, ("const", "i64", 0)), 0),
    ("no_guard", DIV, DIV0),
    ("and_guard", ("and", NZ, GT1), 0),
    ("and_swapped", ("and", GT1, NZ), DIV0),
    ("or_guard", ("or", ("=", B, ("const", "i64", 0)), GT1), 0),
    ("or_swapped", ("or", GT1, ("=", B, ("const", "i64", 0))), DIV0),
    ("coalesce_first", ("coalesce", A, DIV), 0),
    ("coalesce_swapped", ("coalesce", DIV, A), DIV0),
    ("case_else_arm", ("case", ("not", NZ), ("const", "i64", 0), DIV), 0),
    ("case_cond_raises", ("case", GT1, A, B), DIV0),
]


def lazy_cols(n, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.integers(-50, 50, n).astype(np.int64)
    b = rng.integers(-3, 4, n).astype(np.int64)
    b[:min(n, 5)] = [1, 2, -1, 3, 1][:min(n, 5)]
    return ab(a, b)


@pytest.mark.parametrize("name,tree,code", LAZY_CASES, ids=[c[0] for c in LAZY_CASES])
def test_laziness(name, tree, code):
    cols = lazy_cols(300)
    first_zero = int(np.flatnonzero(cols["b"][0] == 0)[0])
    assert first_zero >= 5
    e = err_of(tree, cols)
    assert e == (code_at(first_zero, code) if code else -1)


def test_null_left_of_and_still_evaluates_the_right():
    """A NULL left operand does not decide an AND: the right side runs."""
    cols = {"a": (i64c(4, 4), None), "b": (i64c(2, 0), None),
            "p": (i64c(1, 1), np.array([0, 1], dtype=np.uint8))}
    assert err_of(("and", BOOL_P, GT1), cols) == code_at(1, DIV0)
    assert err_of(("or", BOOL_P, GT1), cols) == code_at(1, DIV0)


def test_error_precedence_inside_one_row():
    cols = ab(i64c(I64_MAX), i64c(0))
    ovf, div = ("+", A, ("const", "i64", 1)), ("/", A, B)
    assert err_of(("+", ovf, div), cols) == code_at(0, INT8_RANGE)
    assert err_of(("+", div, ovf), cols) == code_at(0, DIV0)
    # a NULL sibling does not hide it, on either side
    nul = ("const", "i64", None)
    assert err_of(("+", nul, div), cols) == code_at(0, DIV0)
    assert err_of(("+", div, nul), cols) == code_at(0, DIV0)
    assert err_of(("isnull", div), cols) == code_at(0, DIV0)


def test_garbage_under_a_null_never_raises():
    m = np.array([1, 1, 0], dtype=np.uint8)
    cols = {"a": (i64c(I64_MIN, 5, 6), m), "b": (i64c(-1, 0, 3), m)}
    for tree in (("/", A, B), ("%", A, B), ("neg", A), ("abs", A),
                 ("*", A, B), ("-", B, A)):
        v, nl, e = both(tree, cols)
        assert e == -1 and list(nl) == [1, 1, 0] and list(v[:2]) == [0, 0]
    # NULL on one side only, garbage on the other
    cols = {"a": (i64c(1, 1), None),
            "b": (i64c(0, 1), np.array([1, 0], dtype=np.uint8))}
    v, nl, e = both(("/", A, B), cols)
    assert e == -1 and list(nl) == [1, 0] and list(v) == [0, 1]


def test_rows_outside_the_selection_never_raise():
    cols = ab(i64c(1, 2, 3, 4), i64c(1, 0, 1, 2))
    assert err_of(DIV, cols) == code_at(1, DIV0)
    v, _, e = both(DIV, cols, sel=i64c(0, 2, 3))
    assert e == -1 and list(v) == [1, 3, 2]
    assert err_of(DIV, cols, sel=i64c(3, 1)) == code_at(1, DIV0)


# ---- otbx_project: argument and type checks, no HIP call reached ----

OPS = ex.EX_OPS
I64T, F64T, I32T, U8T = 0, 1, 2, 3       # OTBX_SORT_*
EI, EF, EB = 0, 1, 2                     # OTBX_EXT_*


def prog(*instrs):
    """otbx_expr from (op, type[, isnull]) tuples; COLs get dummy pointers."""
    e = ExprDev()
    e.ninstr = len(instrs)
    for i, ins in enumerate(instrs[:32]):
        d = e.instr[i]
        d.op = OPS[ins[0]] if isinstance(ins[0], str) else ins[0]
        d.type = ins[1] if len(ins) > 1 else 0
        if ins[0] == "col":
            d.col = PTR
            d.nulls = PTR if len(ins) > 2 and ins[2] else None
        elif ins[0] == "const":
            d.isnull = 1 if len(ins) > 2 and ins[2] else 0
    return e


def project(so, e, n=100, n_src=100, sel=None, out_type=I64T, out=PTR,
            out_null=PTR, err=PTR):
    return so.otbx_project(
        None if e is None else C.byref(e),
        C.c_void_p(sel), C.c_int64(n), C.c_int64(n_src), C.c_int32(out_type),
        C.c_void_p(out), C.c_void_p(out_null), C.c_void_p(err), None)


COL_I, COL_F = ("col", I64T), ("col", F64T)
CONST_I, CONST_F, CONST_B = ("const", EI), ("const", EF), ("const", EB)

BAD_PROGRAMS = {
    "unknown_op": [COL_I, (23,)],
    "negative_op": [COL_I, (-1,)],
    "col_type4": [("col", 4)],
    "col_type_neg": [("col", -1)],
    "const_type3": [("const", 3)],
    "cast_type_bool": [COL_I, ("cast", EB)],
    "cast_to_own_type": [COL_I, ("cast", EI)],
    "cast_of_bool": [CONST_B, ("cast", EI)],
    "underflow_binary": [COL_I, ("+",)],
    "underflow_unary": [("neg",)],
    "underflow_case": [CONST_B, COL_I, ("case",)],
    "depth9": [COL_I] * 9 + [("+",)] * 8,
    "int_meets_float": [COL_I, COL_F, ("+",)],
    "cmp_int_float": [COL_I, COL_F, ("<",)],
    "mod_float": [COL_F, COL_F, ("%",)],
    "add_bool": [CONST_B, CONST_B, ("+",)],
    "neg_bool": [CONST_B, ("neg",)],
    "cmp_bool": [CONST_B, CONST_B, ("=",)],
    "and_int": [COL_I, CONST_B, ("and",), ("isnull",), ("cast", EI)],
    "and_nonbool": [COL_I, CONST_B, ("and",)],
    "or_nonbool": [CONST_B, COL_F, ("or",)],
    "not_int": [COL_I, ("not",)],
    "case_cond_int": [COL_I, COL_I, COL_I, ("case",)],
    "case_arms_differ": [CONST_B, COL_I, COL_F, ("case",)],
    "coalesce_types_differ": [COL_I, COL_F, ("coalesce",)],
    "two_values_left": [COL_I, COL_I],
    "three_values_left": [COL_I, COL_I, COL_I, ("+",), COL_I],
}


@pytest.mark.parametrize("name", sorted(BAD_PROGRAMS))
def test_project_refuses_malformed_programs(so, name):
    for out_type in (I64T, F64T, I32T, U8T):
        assert project(so, prog(*BAD_PROGRAMS[name]), out_type=out_type) == \
            OTBX_ERR_INVALID


GOOD = [COL_I, COL_I, ("+",)]


@pytest.mark.parametrize("case", [
    "null_expr", "null_err", "ninstr0", "ninstr_neg", "ninstr33",
    "out_f64_for_int", "out_u8_for_int", "out_i64_for_float",
    "out_i32_for_float", "out_i64_for_bool", "out_type4", "out_type_neg",
    "n_neg", "n_big", "n_src_neg", "n_above_n_src", "n_src_zero",
    "null_col", "null_out", "null_mask_nullable_col",
    "null_mask_null_const"])
def test_project_invalid_arguments(so, case):
    e, kw = prog(*GOOD), {}
    if case == "null_expr":
        e = None
    elif case == "null_err":
        kw["err"] = None
    elif case in ("ninstr0", "ninstr_neg", "ninstr33"):
        e.ninstr = {"ninstr0": 0, "ninstr_neg": -1, "ninstr33": 33}[case]
    elif case == "out_f64_for_int":
        kw["out_type"] = F64T
    elif case == "out_u8_for_int":
        kw["out_type"] = U8T
    elif case == "out_i64_for_float":
        e = prog(COL_F)
    elif case == "out_i32_for_float":
        e, kw["out_type"] = prog(COL_F), I32T
    elif case == "out_i64_for_bool":
        e = prog(CONST_B)
    elif case == "out_type4":
        kw["out_type"] = 4
    elif case == "out_type_neg":
        kw["out_type"] = -1
    elif case == "n_neg":
        kw["n"] = -1
    elif case == "n_big":
        kw["n"], kw["n_src"] = INT32_MAX + 1, 2**40
    elif case == "n_src_neg":
        kw["n"], kw["n_src"], kw["sel"] = 0, -1, PTR
    elif case == "n_above_n_src":
        kw["n"], kw["n_src"] = 101, 100
    elif case == "n_src_zero":
        kw["n"], kw["n_src"], kw["sel"] = 5, 0, PTR
    elif case == "null_col":
        e.instr[1].col = None
    elif case == "null_out":
        kw["out"] = None
    elif case == "null_mask_nullable_col":
        e, kw["out_null"] = prog(COL_I, ("col", I64T, True), ("+",)), None
    elif case == "null_mask_null_const":
        e, kw["out_null"] = prog(COL_I, ("const", EI, True), ("coalesce",),
                                 ("const", EI, True), ("+",)), None
    assert project(so, e, **kw) == OTBX_ERR_INVALID


def test_project_bad_instruction_in_the_last_slot_is_rejected(so):
    # 32 instructions: col, then 15 x (col +), then a broken last one
    ins = [COL_I] + [COL_I, ("+",)] * 15 + [("not",)]
    assert len(ins) == 32
    assert project(so, prog(*ins)) == OTBX_ERR_INVALID


# ---- the limits, through the builder (an accepted program would go on to
# a HIP call: that half is in test_gpu_project.py) ----

def cpu_col(dtype=torch.int64, n=8):
    return ex.col(torch.zeros(n, dtype=dtype))


def chain(k):
    """A left-deep sum: k columns, 2k - 1 instructions, depth 2."""
    e = cpu_col()
    for _ in range(k - 1):
        e = e + cpu_col()
    return e


def right_deep(k):
    """c + (c + (c + ...)): k columns, depth k."""
    e = cpu_col()
    for _ in range(k - 1):
        e = cpu_col() + e
    return e


def test_instruction_and_depth_limits():
    e = -chain(16)                       # 31 + 1
    assert e.ninstr == 32 and len(e.program()) == 32
    assert e.to_dev().ninstr == 32
    with pytest.raises(OtbxError) as ei:
        abs(e)                           # 33
    assert ei.value.status == 3
    d8 = right_deep(8)
    assert d8.depth == 8 and d8.ninstr == 15
    assert pr.tree_depth(("+", ("col", "a"), ("+", ("col", "a"), ("col", "a")))) == 3
    with pytest.raises(OtbxError) as ei:
        right_deep(9)
    assert ei.value.status == 3


# ---- the ctypes mirrors ----

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "otbx.h"
int main(void)
{
    printf("%zu %zu", sizeof(otbx_exprinstr), sizeof(otbx_expr));
    printf(" %zu %zu %zu %zu %zu %zu %zu",
           offsetof(otbx_exprinstr, col), offsetof(otbx_exprinstr, nulls),
           offsetof(otbx_exprinstr, ci), offsetof(otbx_exprinstr, cf),
           offsetof(otbx_exprinstr, op), offsetof(otbx_exprinstr, type),
           offsetof(otbx_exprinstr, isnull));
    printf(" %zu %zu", offsetof(otbx_expr, ninstr), offsetof(otbx_expr, instr));
    printf(" %d %d %d %d\n", OTBX_MAX_EXPR_INSTRS, OTBX_MAX_EXPR_DEPTH,
           OTBX_EX_COALESCE, OTBX_EXERR_INT4);
    return 0;
}
"""


def test_exprdev_matches_the_documented_layout():
    assert C.sizeof(ExprInstrDev) == 48
    assert C.sizeof(ExprDev) == 1544
    assert len(ExprDev().instr) == ex.MAX_EXPR_INSTRS == 32
    assert ex.MAX_EXPR_DEPTH == 8


def test_exprdev_matches_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(x) for x in subprocess.run(
        [str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = ExprInstrDev
    assert got == [C.sizeof(T), C.sizeof(ExprDev), T.col.offset,
                   T.nulls.offset, T.ci.offset, T.cf.offset, T.op.offset,
                   T.type.offset, T.isnull.offset, ExprDev.ninstr.offset,
                   ExprDev.instr.offset, ex.MAX_EXPR_INSTRS,
                   ex.MAX_EXPR_DEPTH, ex.EX_OPS["coalesce"],
                   max(ex.PROJECT_ERRORS)]


# ---- the builder ----

def test_builder_emits_the_q1_expression():
    price, disc, tax = (torch.zeros(8, dtype=torch.float64) for _ in range(3))
    e = ex.col(price) * (1 - ex.col(disc)) * (1 + ex.col(tax))
    assert e.vtype == "f64" and not e.nullable and e.depth == 3
    got = e.program()
    want = [("col", price, None), ("const", "f64", 1.0), ("col", disc, None),
            ("-",), ("*",), ("const", "f64", 1.0), ("col", tax, None),
            ("+",), ("*",)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0]
        if g[0] == "col":
            assert g[1] is w[1] and g[2] is None
        else:
            assert g == w
    d = e.to_dev()
    assert d.ninstr == 9
    assert [d.instr[i].op for i in range(9)] == [0, 1, 0, 3, 4, 1, 0, 2, 4]
    assert d.instr[0].col == price.data_ptr() and d.instr[0].type == F64T
    assert d.instr[1].type == EF and d.instr[1].cf == 1.0
    assert d.instr[1].isnull == 0


def test_builder_inserts_i8tod():
    i = ex.col(torch.zeros(8, dtype=torch.int32))
    f = ex.col(torch.zeros(8, dtype=torch.float64))
    assert [p[0] for p in (i * f).program()] == ["col", "cast", "col", "*"]
    assert [p[0] for p in (f * i).program()] == ["col", "col", "cast", "*"]
    assert (i * f).program()[1] == ("cast", "f64")
    assert [p[0] for p in i.lt(f).program()] == ["col", "cast", "col", "<"]
    assert (i + 1).program()[1] == ("const", "i64", 1)
    assert (i + 1.5).vtype == "f64"
    assert (2 - i).program()[0] == ("const", "i64", 2)
    c = ex.case(i.gt(0), i, 0.5)
    assert c.vtype == "f64" and c.program()[4] == ("cast", "f64")
    assert ex.coalesce(f, 0).program()[-2] == ("const", "f64", 0.0)
    assert f.cast("i64").vtype == "i64" and (-f).vtype == "f64"
    assert abs(i).program()[-1] == ("abs",) and (i % 3).vtype == "i64"


def test_builder_nullability():
    m = torch.zeros(8, dtype=torch.uint8)
    a = ex.col(torch.zeros(8, dtype=torch.int64), m)
    b = ex.col(torch.zeros(8, dtype=torch.int64))
    assert a.nullable and not b.nullable and (a + b).nullable
    assert not a.isnull().nullable and not (~b.gt(0)).nullable
    assert not ex.coalesce(a, b).nullable and ex.coalesce(a, a).nullable
    assert ex.case(b.gt(0), a, b).nullable
    assert not ex.case(a.gt(0), b, b).nullable
    assert ex.null("f64").nullable and ex.null("f64").vtype == "f64"
    n = ex.null("bool").to_dev()
    assert n.instr[0].isnull == 1 and n.instr[0].type == EB
    assert (a.gt(0) & True).nullable and (False | b.gt(0)).vtype == "bool"


def test_builder_argument_errors():
    i = ex.col(torch.zeros(8, dtype=torch.int64))
    f = ex.col(torch.zeros(8, dtype=torch.float64))
    b = i.gt(0)
    bad = [
        lambda: ex.col(torch.zeros(8, dtype=torch.float32)),
        lambda: ex.col([1, 2, 3]),
        lambda: ex.col(torch.zeros(8, dtype=torch.int64),
                       torch.zeros(8, dtype=torch.int64)),
        lambda: ex.col(torch.zeros(8, dtype=torch.int64),
                       torch.zeros(7, dtype=torch.uint8)),
        lambda: i + ex.col(torch.zeros(9, dtype=torch.int64)),
        lambda: ex.const("x"), lambda: ex.const(2**63), lambda: ex.null("i32"),
        lambda: f % f, lambda: f % 2, lambda: b + 1, lambda: -b, lambda: abs(b),
        lambda: b.eq(b), lambda: i & b, lambda: b | 1, lambda: ~i,
        lambda: i.cast("i64"), lambda: b.cast("i64"), lambda: i.cast("bool"),
        lambda: ex.case(i, i, i), lambda: ex.case(b, i, b),
        lambda: ex.coalesce(i, b), lambda: bool(b),
        lambda: ex.GpuProject("x"), lambda: ex.GpuProject(ex.const(1)),
        lambda: ex.GpuProject(i, sel=torch.zeros(3, dtype=torch.int32)),
        lambda: ex.GpuProject(i, n=9), lambda: ex.GpuProject(i, n=-1),
        lambda: ex.GpuProject(i, out=torch.zeros(8, dtype=torch.float64)),
        lambda: ex.GpuProject(i, out=torch.zeros(7, dtype=torch.int64)),
        lambda: ex.GpuProject(f, out=torch.zeros(8, dtype=torch.int32)),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(OtbxError) as ei:
            fn()
        assert ei.value.status == 3, k
    # and what must be accepted
    ex.GpuProject(i, out=torch.zeros(8, dtype=torch.int32))
    ex.GpuProject(i, sel=torch.zeros(3, dtype=torch.int64))
    ex.GpuProject(ex.const(1) + 2, n=5)
    node = ex.GpuProject(i)
    assert node.explain() is None
    with pytest.raises(OtbxError):
        node.ExecCustomScan()            # before BeginCustomScan


# ---- the generator ----

def test_fuzz_programs_are_well_typed_and_mixed():
    """For the seeds the GPU fuzz uses: every program is within the limits,
    the two references agree, at least half raise on no row and at least one
    in ten raises on some row — so the GPU fuzz compares values, not only
    error slots, and error slots too."""
    clean = raised = 0
    for seed in pr.FUZZ_SEEDS:
        tree, out = pr.fuzz_program(seed)
        assert pr.tree_ninstr(tree) <= 32 and pr.tree_depth(tree) <= 8
        cols = pr.fuzz_columns(seed, 300)
        a = both(tree, cols, out=out)
        sel = pr.fuzz_selection(seed, 300)
        both(tree, cols, sel=sel, out=out)
        full = ref_eval(tree, pr.fuzz_columns(seed), out=out)
        clean += full[2] == -1
        raised += full[2] != -1
        del a
    assert clean >= len(pr.FUZZ_SEEDS) / 2, (clean, raised)
    assert raised >= len(pr.FUZZ_SEEDS) / 10, (clean, raised)

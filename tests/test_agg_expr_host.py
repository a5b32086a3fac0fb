"""MI_AGG_SUM_EXPR without a GPU: the factor and product arithmetic the aggregate kernels compile
(duckdb-arrow_amd/csrc/agg_merge.hpp) under ASan + UBSan as a program of its own (tests/sanitize/agg_expr_check.cpp), the new
words of the header, the new structs against the binding, what the Python wrapper refuses before it calls anything, what
the library refuses without a device -- and the reference of the GPU tests (tests/agg_expr_cases.py) held to
pyarrow.compute's decimal arithmetic on TPC-H Q1 over the golden lineitem."""
import ctypes as C
import os
import re
import shutil
import subprocess
from decimal import Decimal
from fractions import Fraction

import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import agg_expr_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEITEM = os.path.join(ROOT, "tests", "golden", "lineitem_sf0_01_head.arrows")


def test_expression_arithmetic_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "agg_expr_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "agg_expr_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"(\d+) checks, 0 failed", run.stdout)
    assert m and int(m.group(1)) > 10000, run.stdout


def test_the_same_arithmetic_with_the_host_compilers_default_contraction(tmp_path):
    """-O2 and no -ffp-contract: the shared functions themselves keep a multiplication and an addition apart"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "agg_expr_check_o2")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sanitize", "agg_expr_check.cpp"), "-o", exe], check=True, capture_output=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and re.search(r"\d+ checks, 0 failed", run.stdout), (run.stdout[-1000:], run.stderr[-2000:])


def test_new_words_of_the_header():
    text = open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read()
    for word in ("MI_AGG_SUM_EXPR = 7", "MI_MAX_EXPR_FACTORS 4", "MI_AGG_CONST_INT = 0", "MI_AGG_CONST_DOUBLE = 1", "mi_agg_factor", "mi_agg_expr",
                 "mi_agg_vector_factor", "mi_agg_vector_expr", "const mi_agg_expr* expr", "const mi_agg_vector_expr* expr", "below 2^127",
                 "Overflow is not detected", "-0.0 included", "left to right"):
        assert word in text, word
    # the feature adds no exported function
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", code))
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mi_[a-z0-9_]+)", out))
    assert not [n for n in exported if "expr" in n] and not [n for n in declared if "expr" in n]
    assert _ffi.AGG_SUM_EXPR == 7 and _ffi.MAX_EXPR_FACTORS == 4 and (_ffi.AGG_CONST_INT, _ffi.AGG_CONST_DOUBLE) == (0, 1)


def test_new_structs_match_the_binding_and_the_old_ones_keep_their_size(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mi_arrow_ipc.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(mi_agg_factor), sizeof(mi_agg_expr), sizeof(mi_agg_vector_factor), sizeof(mi_agg_vector_expr));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(mi_agg_factor, column), offsetof(mi_agg_factor, mul), offsetof(mi_agg_factor, add),
         offsetof(mi_agg_factor, fmul), offsetof(mi_agg_factor, fadd), offsetof(mi_agg_factor, constants), offsetof(mi_agg_expr, factors));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(mi_agg_vector_factor, column), offsetof(mi_agg_vector_factor, mul), offsetof(mi_agg_vector_factor, add),
         offsetof(mi_agg_vector_factor, fmul), offsetof(mi_agg_vector_factor, fadd), offsetof(mi_agg_vector_factor, constants),
         offsetof(mi_agg_vector_expr, factors));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mi_agg_spec), sizeof(mi_agg_vector_spec), offsetof(mi_agg_spec, expr), offsetof(mi_agg_spec, reserved),
         offsetof(mi_agg_vector_spec, expr), offsetof(mi_agg_vector_spec, reserved));
  printf("%d %d %d %d\n", MI_AGG_SUM_EXPR, MI_MAX_EXPR_FACTORS, MI_AGG_CONST_INT, MI_AGG_CONST_DOUBLE);
  return 0;
}'''
    c = tmp_path / "s.c"
    c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    rows = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    F, E, VF, VE = _ffi.AggFactor, _ffi.AggExpr, _ffi.AggVectorFactor, _ffi.AggVectorExpr
    assert rows[0] == [C.sizeof(F), C.sizeof(E), C.sizeof(VF), C.sizeof(VE)]
    assert rows[1] == [F.column.offset, F.mul.offset, F.add.offset, F.fmul.offset, F.fadd.offset, F.constants.offset, E.factors.offset]
    assert rows[2] == [VF.column.offset, VF.mul.offset, VF.add.offset, VF.fmul.offset, VF.fadd.offset, VF.constants.offset, VE.factors.offset]
    # what the two spec structs were before the first reserved word became the pointer: 40 and 72 bytes, the word at 24 / 56
    assert rows[3] == [40, 72, 24, 32, 56, 64]
    assert rows[3] == [C.sizeof(_ffi.AggSpec), C.sizeof(_ffi.AggVectorSpec), _ffi.AggSpec.expr.offset, _ffi.AggSpec.reserved.offset,
                       _ffi.AggVectorSpec.expr.offset, _ffi.AggVectorSpec.reserved.offset]
    assert rows[4] == [_ffi.AGG_SUM_EXPR, _ffi.MAX_EXPR_FACTORS, _ffi.AGG_CONST_INT, _ffi.AGG_CONST_DOUBLE]
    assert rows[0] == [48, 8 + 4 * 48, 64, 8 + 4 * 64]


class _NoLibrary:
    """a relation / context whose handle must never be used: the wrapper refuses before it calls the library"""
    _h = None
    _initialised = False


CALLS = (lambda s: da.Relation.aggregate(_NoLibrary(), s), lambda s: da.Relation.group_aggregate(_NoLibrary(), ["k"], s),
         lambda s: da.aggregate_vectors(_NoLibrary(), s, 10), lambda s: da.group_aggregate_vectors(_NoLibrary(), [(1, 0, 4, "signed")], s, 10))


@pytest.mark.parametrize("call", range(len(CALLS)))
def test_the_wrapper_refuses_bad_expressions_without_a_gpu(call):
    call = CALLS[call]
    col = (4096, 0, 4, "signed")
    for spec, word in ((("sum_expr",), "1 to 4 factors, not 0"),
                       (("sum_expr", col, col, col, col, col), "1 to 4 factors, not 5"),
                       (("sum_expr", 3), "at least one factor with a column"),
                       (("sum_expr", (None, 3), 2.5, (None, -1)), "at least one factor with a column"),
                       (("sum_expr", None), "factor"),
                       (("sum_expr", col, (None, "x")), "constant"),
                       (("sum_expr", col, True), "factor"),
                       (("sum_expr", (col, 1 << 63, 0)), "does not fit an int64"),
                       (("sum_expr", (col, 1, -(1 << 63) - 1)), "does not fit an int64")):
        with pytest.raises(da.MiError) as e:
            call([spec])
        assert e.value.code == _ffi.MI_EINVAL and word in str(e.value), (spec, str(e.value))
    with pytest.raises(da.MiError) as e:       # an AVG is still no operation: an average is a sum divided by its count
        call([("avg", "c")])
    assert e.value.code == _ffi.MI_EINVAL and "unknown operation" in str(e.value)
    with pytest.raises(da.MiError) as e:
        call([("sum_expr", col)] * 9)
    assert e.value.code == _ffi.MI_EINVAL and "1 to 8" in str(e.value)


def test_the_factor_forms_the_wrapper_takes():
    checked = da._agg_check_specs([("sum_expr", "a", ("b", -1, 100), (None, 7), 2.5), ("SUM_EXPR", ((1, 0, 8, "float"), 1.0, 0.0)), ("sum", "a")])
    assert checked == [("sum_expr", (("a", 1, 0), ("b", -1, 100), (None, 1, 7), (None, 1, 2.5))), ("sum_expr", (((1, 0, 8, "float"), 1.0, 0.0),)),
                       ("sum", ("a",))]
    arr, keep = da._agg_scan_specs(checked[:1])
    e = arr[0].expr.contents
    assert arr[0].op == 7 and e.n_factors == 4
    assert [(f.column, f.mul, f.add, f.constants) for f in e.factors[:3]] == [(b"a", 1, 0, 0), (b"b", -1, 100, 0), (None, 1, 7, 0)]
    assert (e.factors[3].column, e.factors[3].fmul, e.factors[3].fadd, e.factors[3].constants) == (None, 1.0, 2.5, 1)
    varr, keep = da._agg_vector_specs(checked[1:2], {"float": _ffi.AGG_CLASS_FLOAT})
    f = varr[0].expr.contents.factors[0]
    assert (f.column.data, f.column.width, f.column.value_class, f.fmul, f.fadd, f.constants) == (1, 8, _ffi.AGG_CLASS_FLOAT, 1.0, 0.0, 1)


def test_the_library_refuses_a_null_handle_with_an_expression_without_a_gpu():
    L = _ffi.lib()
    out = (_ffi.AggValue * 2)()
    arr, keep = da._agg_scan_specs(da._agg_check_specs([("sum_expr", "a", ("b", -1, 100))]))
    assert L.mi_scan_aggregate(None, arr, 1, out, None, None) == _ffi.MI_EINVAL
    keys = (C.c_char_p * 1)(b"k")
    gk = (_ffi.GroupKeyValue * 2)()
    n = C.c_int32()
    assert L.mi_scan_group_aggregate(None, keys, 1, arr, 1, gk, out, 2, C.byref(n), None, None) == _ffi.MI_EINVAL
    varr, keep2 = da._agg_vector_specs(da._agg_check_specs([("sum_expr", (4096, 0, 4, "signed"))]), {"signed": _ffi.AGG_CLASS_SIGNED})
    assert L.mi_aggregate_vectors(None, varr, 1, None, None, 10, out, None) == _ffi.MI_EINVAL
    kc = (_ffi.GroupKeyColumn * 1)()
    assert L.mi_group_aggregate_vectors(None, kc, 1, varr, 1, None, None, 10, gk, out, 2, C.byref(n), None) == _ffi.MI_EINVAL


def build_q1_full_example(tmp_path):
    exe = str(tmp_path / "q1_full")
    libdir = os.path.join(ROOT, "duckdb-arrow_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "q1_full.c"),
                    "-L" + libdir, "-lmi_arrow_ipc", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_plain_c_client_of_the_whole_q1_builds_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/q1_full.c is C99 against include/mi_arrow_ipc.h alone; without a device the first call reports MI_ENODEV."""
    import torch
    exe = build_q1_full_example(tmp_path)
    text = open(os.path.join(ROOT, "examples", "q1_full.c")).read()
    assert "MI_AGG_SUM_EXPR" in text and text.count("mi_scan_group_aggregate(") == 1 and "l_tax" in text
    assert "needs the three-factor product" not in open(os.path.join(ROOT, "examples", "q1.c")).read()
    if torch.cuda.is_available():
        return      # its run on a GPU is test_gpu_scan_agg_expr.py's
    r = subprocess.run([exe, LINEITEM], capture_output=True, text=True)
    assert r.returncode == 1 and "mi_ctx_create failed (19)" in r.stderr and "no CPU fallback" in r.stderr


# ---- the reference of the GPU tests, held to something else
def test_the_integer_reference_against_pyarrow_decimal_arithmetic_on_q1():
    """Q1's four sums per (l_returnflag, l_linestatus) over the golden lineitem: tests/agg_expr_cases.py over the stored integers
    against pyarrow.compute's decimal subtract / add / multiply / sum (exact decimal arithmetic, a different program)"""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.ipc as ipc
    t = ipc.open_stream(LINEITEM).read_all()
    narrow = pa.decimal128(10, 2)      # (the products' precision must stay within 38 digits; every value fits 10)
    price, disc, tax = (pc.cast(t.column(n), narrow) for n in ("l_extendedprice", "l_discount", "l_tax"))
    one = pa.scalar(Decimal("1.00"), narrow)
    disc_price = pc.multiply(price, pc.subtract(one, disc))
    charge = pc.multiply(disc_price, pc.add(one, tax))
    assert disc_price.type.scale == 4 and charge.type.scale == 6
    tab = pa.table({"f": t.column("l_returnflag"), "s": t.column("l_linestatus"), "qty": t.column("l_quantity"), "price": t.column("l_extendedprice"),
                    "disc_price": disc_price, "charge": charge, "disc": t.column("l_discount")})
    g = tab.group_by(["f", "s"]).aggregate([("qty", "sum"), ("price", "sum"), ("disc_price", "sum"), ("charge", "sum"), ("disc", "sum"), ([], "count_all")])
    want = {}
    for row in g.to_pylist():
        want[(row["f"], row["s"])] = [int(row["qty_sum"].scaleb(2)), int(row["price_sum"].scaleb(2)), int(row["disc_price_sum"].scaleb(4)),
                                      int(row["charge_sum"].scaleb(6)), int(row["disc_sum"].scaleb(2)), row["count_all"]]
    got = ec.q1_reference(t)
    assert got == want and len(got) == 4
    assert all(v[3] > v[2] * 100 > 0 for v in got.values())      # a charge is at least the discounted price


def test_the_reference_wraps_and_applies_the_null_rule():
    a = ec.Factor([ec.I64_MIN, 5, 7], [True, True, False])
    b = ec.Factor([ec.I64_MIN, -2, 9], None, mul=ec.I64_MIN, add=ec.I64_MIN)
    value, count = ec.sum_expr_int([a, b, a, b], [0, 1, 2])
    assert count == 2      # row 2 is NULL in `a`
    terms = [(ec.I64_MIN * (ec.I64_MIN + ec.I64_MIN * ec.I64_MIN)) ** 2, (5 * (ec.I64_MIN + ec.I64_MIN * -2)) ** 2]
    assert abs(sum(terms)) > 1 << 128 and value == ec.wrap128(sum(terms)) and -(1 << 127) <= value < (1 << 127)
    assert ec.sum_expr_int([a], [2]) == (None, 0)
    assert ec.sum_expr_int([ec.Factor(None, None, add=3), ec.Factor([4, 5])], [0, 1]) == (27, 2)
    exact, total_abs, n = ec.sum_expr_float([ec.Factor([0.5, -0.25], None, mul=2.0, add=1.0), ec.Factor([3.0, 4.0])], [0, 1])
    assert (exact, total_abs, n) == (Fraction(8), Fraction(8), 2)
    assert ec.float_bound(2, 2, Fraction(8)) == 2 * 8 * Fraction(1, 1 << 53) * 8

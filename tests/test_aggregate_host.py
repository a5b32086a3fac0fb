"""mi_scan_aggregate / mi_aggregate_vectors without a GPU: the merge rules the aggregate kernels compile
(duckdb-arrow_amd/csrc/agg_merge.hpp) under ASan + UBSan as a program of their own (tests/sanitize/agg_merge_check.cpp),
the new symbols in the header, the library and the binding, and what the Python wrapper refuses before it calls anything."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mi_scan_aggregate", "mi_aggregate_vectors", "mi_aggregate_counters")


def test_merge_header_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "agg_merge_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "agg_merge_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"(\d+) checks, 0 failed", run.stdout)
    assert m and int(m.group(1)) > 2000, run.stdout


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mi_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _ffi.SIGNATURES and getattr(_ffi.lib(), name) is not None, name
    for word in ("MI_AGG_COUNT_STAR", "MI_AGG_COUNT", "MI_AGG_SUM", "MI_AGG_SUM_PRODUCT", "MI_AGG_MIN", "MI_AGG_MAX", "mi_agg_spec",
                 "mi_agg_value", "MI_ST_SEL_RANGE", "modulo 2^128"):
        assert word in open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read(), word
    # mi_scan_sum_product's declaration is where and what it was
    assert "int mi_scan_sum_product(mi_scan* s, const char* column_a, const char* column_b, const mi_range_filter* filters,\n" \
           "                        int32_t n_filters, mi_sum_product_result* out);" in open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read()


def test_struct_sizes_and_constants_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mi_arrow_ipc.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mi_agg_spec), sizeof(mi_agg_value), sizeof(mi_agg_column), sizeof(mi_agg_vector_spec),
         offsetof(mi_agg_value, count), offsetof(mi_agg_value, is_null), offsetof(mi_agg_vector_spec, b));
  printf("%d %d %d %d %d %d %d %d %d %u\n", MI_AGG_COUNT_STAR, MI_AGG_COUNT, MI_AGG_SUM, MI_AGG_SUM_PRODUCT, MI_AGG_MIN, MI_AGG_MAX,
         MI_MAX_AGGREGATES, MI_AGG_VALUE_DOUBLE, MI_AGG_CLASS_WIDE, MI_ST_SEL_RANGE);
  return 0;
}'''
    c = tmp_path / "s.c"
    c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    sizes, consts = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert sizes == [C.sizeof(_ffi.AggSpec), C.sizeof(_ffi.AggValue), C.sizeof(_ffi.AggColumn), C.sizeof(_ffi.AggVectorSpec),
                     _ffi.AggValue.count.offset, _ffi.AggValue.is_null.offset, _ffi.AggVectorSpec.b.offset]
    assert consts == [_ffi.AGG_COUNT_STAR, _ffi.AGG_COUNT, _ffi.AGG_SUM, _ffi.AGG_SUM_PRODUCT, _ffi.AGG_MIN, _ffi.AGG_MAX,
                      _ffi.MAX_AGGREGATES, _ffi.AGG_VALUE_DOUBLE, _ffi.AGG_CLASS_WIDE, _ffi.ST_SEL_RANGE]


class _NoLibrary:
    """a relation / context whose handle must never be used: the wrapper refuses before it calls the library"""
    _h = None
    _initialised = False


def test_the_wrapper_refuses_more_than_8_specs_and_unknown_operations_without_a_gpu():
    nine = [("count_star",)] * 9
    for call in (lambda s: da.Relation.aggregate(_NoLibrary(), s), lambda s: da.aggregate_vectors(_NoLibrary(), s, 10)):
        with pytest.raises(da.MiError) as e:
            call(nine)
        assert e.value.code == _ffi.MI_EINVAL and "1 to 8" in str(e.value)
        with pytest.raises(da.MiError) as e:
            call([])
        assert e.value.code == _ffi.MI_EINVAL
        with pytest.raises(da.MiError) as e:
            call([("avg", "c")])
        assert e.value.code == _ffi.MI_EINVAL and "unknown operation" in str(e.value) and "avg" in str(e.value)
        with pytest.raises(da.MiError) as e:
            call([("sum_product", "a")])
        assert e.value.code == _ffi.MI_EINVAL and "sum_product takes 2" in str(e.value)
        with pytest.raises(da.MiError) as e:
            call([("count_star", "a")])
        assert e.value.code == _ffi.MI_EINVAL


def test_the_library_refuses_bad_arguments_without_a_gpu():
    L = _ffi.lib()
    out = (_ffi.AggValue * 9)()
    spec = (_ffi.AggSpec * 9)()
    assert L.mi_scan_aggregate(None, spec, 1, out, None, None) == _ffi.MI_EINVAL
    vs = (_ffi.AggVectorSpec * 9)()
    assert L.mi_aggregate_vectors(None, vs, 1, None, None, 10, out, None) == _ffi.MI_EINVAL
    a, b, c, d = C.c_int64(-1), C.c_int64(-1), C.c_double(-1), C.c_double(-1)
    assert L.mi_aggregate_counters(C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == _ffi.MI_OK
    assert a.value >= 0 and b.value >= 0 and c.value >= 0 and d.value >= 0


def build_agg_example(tmp_path):
    exe = str(tmp_path / "agg")
    libdir = os.path.join(ROOT, "duckdb-arrow_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "agg.c"),
                    "-L" + libdir, "-lmi_arrow_ipc", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_plain_c_client_of_the_aggregates_builds_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/agg.c is C99 against include/mi_arrow_ipc.h alone; without a device the first call reports MI_ENODEV."""
    import torch
    exe = build_agg_example(tmp_path)
    if torch.cuda.is_available():
        return      # its run on a GPU is test_gpu_scan_aggregate.py's
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lineitem_sf0_01_q6.arrows")], capture_output=True, text=True)
    assert r.returncode == 1 and "mi_ctx_create failed (19)" in r.stderr and "no CPU fallback" in r.stderr

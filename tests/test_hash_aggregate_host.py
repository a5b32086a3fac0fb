"""mi_scan_hash_aggregate / mi_hash_aggregate_vectors without a GPU: the rules the hash GROUP BY kernels compile
(duckdb-arrow_amd/csrc/hash_group.hpp) under ASan + UBSan as a program of their own (tests/sanitize/hash_group_check.cpp),
the Python restatement of the hash held to that program's output, the case module's reference held to pyarrow's group_by,
the new symbols and constants in the header, the library and the binding, and what the wrapper and the library refuse
without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import hash_agg_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_arrow_ipc.h")
NEW_SYMBOLS = ("mi_scan_hash_aggregate", "mi_hash_aggregate_vectors", "mi_hash_aggregate_counters")


def test_hash_group_header_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hash_group_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "hash_group_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"(\d+) checks, 0 failed", run.stdout)
    assert m and int(m.group(1)) > 100000, run.stdout
    # the Python restatement of the hash, which the GPU tests build colliding keys from, is the C++ one
    printed = {int(k): int(h) for k, h in re.findall(r"^hash (\d+) (\d+)$", run.stdout, flags=re.M)}
    assert sorted(printed) == sorted(hc.HASH_PROBE_KEYS)
    for k in hc.HASH_PROBE_KEYS:
        assert hc.hash64(k) == printed[k], k


def test_the_case_modules_helpers():
    assert [hc.slots_for(g) for g in (1, 32, 33, 4096, 1 << 24)] == [64, 64, 128, 8192, 1 << 25]
    assert hc.table_bytes(32, 1) == 32 + 8 * 64 + 24 * 66
    last = hc.keys_in_slot(63, 64, 32)
    assert len(set(last)) == 32 and all(hc.hash64(k) & 63 == 63 for k in last)
    nan = float("nan")
    assert hc.bits(hc.canonical(-0.0)) == 0 and hc.bits(hc.canonical(-nan)) == hc.CANONICAL_NAN
    col = hc.HostColumn([1.0, nan, -0.0, float("inf"), float("-inf")], "float")
    assert hc.expected("max", [col], [0, 1, 2, 3, 4])[0] != hc.expected("max", [col], [0, 1, 2, 3, 4])[0]     # NaN, the greatest
    assert hc.expected("max", [col], [0, 2, 3, 4]) == (float("inf"), 4) and hc.expected("min", [col], [0, 1, 2, 3]) == (0.0, 4)
    assert hc.bits(hc.expected("min", [col], [1, 2])[0]) == 0      # -0.0 comes back as +0.0
    u = hc.HostColumn([(1 << 64) - 1, 1 << 63], "unsigned")
    assert hc.expected("sum", [u], [0, 1]) == ((1 << 64) - 1 + (1 << 63), 2)
    s = hc.HostColumn([-3, 4], "signed", [True, False])
    assert hc.expected("sum_expr", [(s, 2, 1), 10], [0, 1]) == (-50, 1) and hc.expected("sum", [s], [1]) == (None, 0)


def test_the_reference_agrees_with_pyarrow_group_by():
    """every case pyarrow can express: int64 sums without wrap, counts, min / max, NULL keys as a group"""
    cols, aggs, pa_aggs = hc.pyarrow_table_and_specs()
    want = hc.pyarrow_groups(hc.to_arrow(cols), "k", pa_aggs)
    got = hc.reference(cols["k"], aggs, range(len(cols["k"].py)))
    assert len(got) == len(want) > 800 and got[-1][0] is None
    for (gk, gv), (wk, wv) in zip(got, want):
        assert gk == wk
        for (g_val, g_cnt), w_val in zip(gv, wv):
            assert g_val == w_val, (gk, gv, wv)


def test_new_symbols_are_declared_exported_and_bound():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mi_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _ffi.SIGNATURES and getattr(_ffi.lib(), name) is not None, name
    assert "MI_MAX_HASH_GROUPS" in raw and "max_groups" in raw
    # mi_scan_group_aggregate's declaration and limits are where and what they were
    assert "int mi_scan_group_aggregate(mi_scan* s, const char* const* key_columns, int32_t n_keys, const mi_agg_spec* aggs, int32_t n_aggs,\n" in raw
    assert raw.index("int mi_group_aggregate_counters(") < raw.index("int mi_scan_hash_aggregate(")
    for name in ("hash_aggregate_vectors", "hash_aggregate_counters"):
        assert callable(getattr(da, name)), name
    assert callable(da.Relation.hash_aggregate)


def test_struct_sizes_and_constants_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include "mi_arrow_ipc.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mi_group_key_value), sizeof(mi_group_key_column), sizeof(mi_agg_spec), sizeof(mi_agg_value),
         sizeof(mi_agg_vector_spec), sizeof(mi_agg_column), sizeof(mi_scan_options));
  printf("%d %d %d %d %u\n", MI_MAX_HASH_GROUPS, MI_MAX_GROUPS, MI_GROUP_WINDOW_LIMIT, MI_MAX_AGGREGATES, MI_ST_GROUP_LIMIT);
  return 0;
}'''
    c = tmp_path / "s.c"
    c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    sizes, consts = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    # no existing struct changed size
    assert sizes == [24, 24, 40, 48, 72, 24, C.sizeof(_ffi.ScanOptions)]
    assert sizes[:6] == [C.sizeof(x) for x in (_ffi.GroupKeyValue, _ffi.GroupKeyColumn, _ffi.AggSpec, _ffi.AggValue, _ffi.AggVectorSpec, _ffi.AggColumn)]
    assert consts == [_ffi.MAX_HASH_GROUPS, 4096, 256, 8, _ffi.ST_GROUP_LIMIT] and _ffi.MAX_HASH_GROUPS == hc.MAX_HASH_GROUPS == 1 << 24
    hpp = open(os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "hash_group.hpp")).read()
    assert "constexpr uint32_t kMaxHashGroups = 1u << 24;" in hpp


class _NoLibrary:
    """a relation / context whose handle must never be used: the wrapper refuses before it calls the library"""
    _h = None
    _initialised = False
    fields = []


def test_the_wrapper_refuses_bad_arguments_without_a_gpu():
    good_key = (1, 0, 4, "signed")
    calls = (lambda k, s, m: da.Relation.hash_aggregate(_NoLibrary(), k, s, m),
             lambda k, s, m: da.hash_aggregate_vectors(_NoLibrary(), [good_key] * len(k) if isinstance(k, list) else good_key, s, 10, m))
    for call in calls:
        with pytest.raises(da.MiError) as e:
            call(["a", "b"], [("count_star",)], 100)
        assert e.value.code == _ffi.MI_ENOTSUP and "ONE key column" in str(e.value) and "group_aggregate" in str(e.value) and "few groups" in str(e.value)
        for bad in (0, -1, (1 << 24) + 1, 2.5, None, True):
            with pytest.raises(da.MiError) as e:
                call("a", [("count_star",)], bad)
            assert e.value.code == _ffi.MI_EINVAL and "max_groups" in str(e.value)
        with pytest.raises(da.MiError) as e:
            call("a", [("count_star",)] * 9, 100)
        assert e.value.code == _ffi.MI_EINVAL and "1 to 8" in str(e.value)
        with pytest.raises(da.MiError) as e:
            call("a", [], 100)
        assert e.value.code == _ffi.MI_EINVAL
        with pytest.raises(da.MiError) as e:
            call("a", [("median", "c")], 100)
        assert e.value.code == _ffi.MI_EINVAL and "unknown operation" in str(e.value)
    with pytest.raises(da.MiError) as e:
        da.hash_aggregate_vectors(_NoLibrary(), (1, 0, 8, "float"), [("count_star",)], 10, 100)
    assert e.value.code == _ffi.MI_EINVAL and "key class" in str(e.value)


def test_the_library_refuses_bad_arguments_without_a_gpu():
    L = _ffi.lib()
    spec = (_ffi.AggSpec * 9)()
    out_k = (_ffi.GroupKeyValue * 8)()
    out_v = (_ffi.AggValue * 8)()
    n = C.c_int32(-1)
    assert L.mi_scan_hash_aggregate(None, b"k", spec, 1, 100, out_k, out_v, 2, C.byref(n), None, None) == _ffi.MI_EINVAL
    assert n.value == 0 and b"NULL argument" in L.mi_last_error()
    kc = _ffi.GroupKeyColumn()
    vs = (_ffi.AggVectorSpec * 9)()
    n = C.c_int32(-1)
    assert L.mi_hash_aggregate_vectors(None, C.byref(kc), vs, 1, None, None, 10, 100, out_k, out_v, 2, C.byref(n), None) == _ffi.MI_EINVAL
    assert n.value == 0 and b"NULL argument" in L.mi_last_error()
    a, b, c, d = C.c_int64(-1), C.c_int64(-1), C.c_double(-1), C.c_double(-1)
    assert L.mi_hash_aggregate_counters(C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == _ffi.MI_OK
    assert a.value >= 0 and b.value >= 0 and c.value >= 0 and d.value >= 0
    assert L.mi_hash_aggregate_counters(None, None, None, None) == _ffi.MI_OK


def test_plain_c_client_builds_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/hash_agg.c is C99 against include/mi_arrow_ipc.h alone; without a device the first call reports MI_ENODEV."""
    import torch
    exe = str(tmp_path / "hash_agg")
    libdir = os.path.join(ROOT, "duckdb-arrow_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "hash_agg.c"),
                    "-L" + libdir, "-lmi_arrow_ipc", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    text = open(os.path.join(ROOT, "examples", "hash_agg.c")).read()
    assert "mi_scan_hash_aggregate" in text and "l_orderkey" in text and "l_quantity" in text
    if torch.cuda.is_available():
        return      # its run on a GPU is test_gpu_scan_hash_aggregate.py's
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lineitem_sf0_01_head.arrows")], capture_output=True, text=True)
    assert r.returncode == 1 and "mi_ctx_create failed (19)" in r.stderr and "no CPU fallback" in r.stderr

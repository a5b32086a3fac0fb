"""Bind time and result side of the fused aggregates (duckdb-arrow_amd/csrc/agg_bind.cpp, agg_result.cpp) are host code without
a HIP call or header: tests/sanitize/agg_bind_check.cpp is built with g++ from those two and ipc_format.cpp alone and run as a
program of its own under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_agg_bind_and_result_under_asan_and_ubsan(tmp_path):
    """Against literals written out from the rules of a bind and from the message texts of the three scan calls: every refusal a
    bind can give beside a twin that binds (unknown, constant, unsupported, dictionary and union columns; classes a sum, a
    MIN / MAX, a factor, a key, the hash table do not take; mixed factor families; the counts of aggregates, factors and keys;
    constants; max_groups), the class of every column type as an aggregate's input and as a key, the projection's slots, COUNT(*)'s
    choice of a column; then SortGroups, FillAggValue, FillGroupOutputs, K11's key builder, and the three multi-device merges
    over 1, 2 and 3 parts up to the group limits the parts cross only together."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / "agg_bind_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "agg_bind_check.cpp"),
         os.path.join(csrc, "agg_bind.cpp"), os.path.join(csrc, "agg_result.cpp"), os.path.join(csrc, "ipc_format.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "FAILED" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"^(\d+) checks, 0 failed$", run.stdout, re.M)
    assert m and int(m.group(1)) >= 876, run.stdout

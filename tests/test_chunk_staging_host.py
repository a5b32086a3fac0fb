"""The writer's chunk staging (duckdb-arrow_amd/csrc/chunk_staging.cpp: ChunkCollection) and the serializer's device staging
layout (writer_plan.cpp: LayOutStaging) are host code without a HIP call or header: tests/sanitize/chunk_staging_check.cpp is
built with g++ from chunk_staging.cpp, writer_plan.cpp and ipc_format.cpp alone and run as a program of its own under
AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_staging_under_asan_and_ubsan(tmp_path):
    """Staging memory is a malloc of exactly the bytes asked for and every source array a malloc of its exact size, so a byte
    read or written outside any of them is a report.  Against literals: validity bits of slices that start anywhere and cross
    words, growth and reset, strings at the 12 / 13 byte boundary and around the edges of a declared heap, NULL rows that hold
    garbage, list runs, the 2^31 list offset, groups, union member masks, null nodes, every message in full, LayOutStaging."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / "chunk_staging_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "chunk_staging_check.cpp"),
         os.path.join(csrc, "chunk_staging.cpp"), os.path.join(csrc, "writer_plan.cpp"), os.path.join(csrc, "ipc_format.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "FAILED" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"^(\d+) checks, 0 failed$", run.stdout, re.M)
    assert m and int(m.group(1)) > 500, run.stdout

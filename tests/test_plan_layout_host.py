"""The kind table and the plan layout (duckdb-arrow_amd/csrc/task_kind.hpp, plan_layout.cpp) are host code without a HIP call
or header: tests/sanitize/plan_layout_check.cpp is built with g++ from plan_layout.cpp and ipc_format.cpp alone and run as a
program of its own under AddressSanitizer + UBSan."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_layout_under_asan_and_ubsan(tmp_path):
    """Against literals written out from the rules of a plan and from the per-kind switches the table replaced: every kind's
    class, launch slot, misc group, gather support and output width; ArrowField::Plan's out_width against OutWidth for a field of
    every type it plans; slices, tile tables, order and statistics of a mixed decode plan at depths 0 to 2 and of an encode
    plan; empty, reused and oversized plans; and the full text of every validation message beside a valid twin."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / "plan_layout_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "plan_layout_check.cpp"),
         os.path.join(csrc, "plan_layout.cpp"), os.path.join(csrc, "ipc_format.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "FAILED" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"^(\d+) checks, 0 failed$", run.stdout, re.M)
    assert m and int(m.group(1)) > 1000, run.stdout

"""The writer's LZ4 compressor on the CPU: the block format rules and the serial restatement of the compress kernel
(duckdb-arrow_amd/csrc/lz4_encode_format.hpp) and the compressed body layout (writer_plan.cpp) are plain C++ shared with
the device build, so tests/sanitize/lz4_encode_check.cpp runs them under ASan + UBSan -- an index past a block's bound shows
here and not as a GPU fault -- and liblz4 and the host reader read back what they wrote.  The exported verification hook
(mi_lz4_frame_compress_host) is checked against pyarrow's LZ4 frame decoder."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from duckdb_arrow_amd import _ffi
from helpers import READER_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_and_body_layout_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / "lz4_encode_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "lz4_encode_check.cpp"),
         os.path.join(csrc, "writer_plan.cpp")] + READER_HOST_SOURCES + ["-ldl", "-lpthread", "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", MI_IO_THREADS="2"))
    if run.returncode == 77:
        pytest.skip("liblz4.so.1 not available")
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    m = re.search(r"(\d+) cases, (\d+) blocks \((\d+) stored\), (\d+) framed and (\d+) raw buffers, (\d+) checks, 0 failed", run.stdout)
    assert m, run.stdout
    cases, blocks, stored, framed, raw, checks = (int(x) for x in m.groups())
    assert cases >= 13 * 8 and 0 < stored < blocks and framed > 0 and raw > 0 and checks > 1000
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "FAILED" not in run.stderr, run.stderr[-3000:]


def compress_host(data):
    L = _ffi.lib()
    a = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, np.uint8)
    size = C.c_int64()
    _ffi.check(L.mi_lz4_frame_compress_host(a.ctypes.data if len(data) else None, len(data), None, 0, C.byref(size)))
    out = np.zeros(max(1, size.value), np.uint8)
    _ffi.check(L.mi_lz4_frame_compress_host(a.ctypes.data if len(data) else None, len(data), out.ctypes.data, size.value, C.byref(size)))
    return out[: size.value].tobytes()


def test_verification_hook_writes_buffers_any_lz4_reader_takes():
    import pyarrow as pa
    rng = np.random.default_rng(3)
    text = b" ".join([b"carefully", b"final", b"deposits", b"sleep"][i] for i in rng.integers(0, 4, 40000))
    cases = {"empty": b"", "short": b"abc", "zeros": bytes(200000), "text": text, "random": rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
             "ints": (np.arange(50000, dtype=np.int64) * 3).tobytes()}
    for name, data in cases.items():
        buf = compress_host(data)
        if not data:
            assert buf == b"", name
            continue
        prefix = int(np.frombuffer(buf[:8], dtype=np.int64)[0])
        if prefix == -1:
            assert buf[8:] == data and name in ("short", "random"), name
        else:
            assert prefix == len(data) and len(buf) < 8 + len(data), name
            assert buf[8:15] == bytes([0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82]) and buf[-4:] == bytes(4), name
            assert pa.Codec("lz4").decompress(buf[8:], decompressed_size=len(data), asbytes=True) == data, name
    assert len(compress_host(cases["zeros"])) < 2000 and len(compress_host(text)) < len(text) // 2
    # a room too small is reported, nothing is written
    size = C.c_int64()
    out = np.full(16, 7, np.uint8)
    a = np.frombuffer(text, dtype=np.uint8)
    _ffi.check(_ffi.lib().mi_lz4_frame_compress_host(a.ctypes.data, len(text), out.ctypes.data, 16, C.byref(size)))
    assert size.value > len(text) and (out == 7).all()

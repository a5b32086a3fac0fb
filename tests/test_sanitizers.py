"""AddressSanitizer + UBSan over the host IPC reader (CPU build only; GPU sanitizers are not available on the pool):
tests/sanitize/fuzz_reader.cpp is built with g++ from the reader's host sources alone (no HIP) and drains mutated fixtures,
touching every byte of every buffer span the reader hands out."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import READER_HOST_SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_reader_is_clean_under_asan_and_ubsan(tmp_path, golden_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_reader")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "fuzz_reader.cpp")] + READER_HOST_SOURCES +
        [os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "c_stream.cpp"), "-ldl", "-lpthread", "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    files = [os.path.join(golden_dir, f) for f in ("edge_nested.arrows", "ref_data/test.arrows", "edge_dict.arrows",
                                                   "edge_file_format.arrow", "edge_types2.arrows", "edge_empty.arrows")]
    # + ZSTD / LZ4 bodies, stream and file format (written here by pyarrow)
    import numpy as np
    import pyarrow as pa
    import pyarrow.ipc as ipc
    rng = np.random.default_rng(5)
    t = pa.table({"a": rng.integers(0, 50, 12000), "s": ["row %d" % (i % 97) for i in range(12000)],
                  "l": pa.array([[int(x) for x in rng.integers(0, 9, int(rng.integers(0, 4)))] for _ in range(12000)], pa.list_(pa.int32()))})
    for codec in ("zstd", "lz4"):
        p1, p2 = str(tmp_path / ("c_%s.arrows" % codec)), str(tmp_path / ("c_%s.arrow" % codec))
        with ipc.new_stream(p1, t.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
            w.write_table(t, max_chunksize=5000)
        with ipc.new_file(p2, t.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
            w.write_table(t, max_chunksize=5000)
        files += [p1, p2]
    # a flat LZ4 table whose buffers span several linked 64 KiB blocks: these record batches are DEFERRED (handed out
    # compressed with the block tables of the GPU decompressor); the harness restates the K8 kernels and compares with liblz4
    flat = pa.table({"k": np.arange(60000, dtype=np.int64) * 7, "z": np.zeros(60000, np.int32), "r": rng.integers(0, 1 << 60, 60000),
                     "s": ["comment %d %s" % (i % 311, "lorem ipsum"[: i % 11]) for i in range(60000)]})
    p3 = str(tmp_path / "flat_lz4.arrows")
    with ipc.new_stream(p3, flat.schema, options=ipc.IpcWriteOptions(compression="lz4")) as w:
        w.write_table(flat, max_chunksize=40000)
    files.append(p3)
    run = subprocess.run([exe, os.environ.get("MI_SANITIZE_ITERS", "400")] + files, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", MI_IO_THREADS="2",
                                  TMPDIR=str(tmp_path)))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    import re
    assert int(re.search(r"(\d+) deferred LZ4 batches", run.stdout).group(1)) >= 2, run.stdout
    assert "no sanitizer report" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_zstd_stages_on_the_cpu(tmp_path):
    """The entropy stage of the ZSTD kernels (duckdb-arrow_amd/csrc/zstd_format.hpp: FSE / Huffman tables, backward
    bitstreams, sequences, repeat offsets) and the host walk that feeds it are plain C++ shared with the device build:
    tests/sanitize/zstd_check.cpp runs them block by block in the kernels' order on frames written here by libzstd (through
    pyarrow) and compares with the bytes that went in -- under ASan + UBSan, so an out-of-range table index shows here and not
    as a GPU fault."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import numpy as np
    import pyarrow as pa
    exe = str(tmp_path / "zstd_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "zstd_check.cpp"),
         os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "frame_walk.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    rng = np.random.default_rng(7)
    words = [b"carefully", b"final", b"deposits", b"furiously", b"quickly", b"express", b"packages", b"sleep", b"blithely", b"regular"]
    text = b" ".join(words[i] for i in rng.integers(0, len(words), 60000))
    cases = {
        "empty": b"", "one": b"x", "zeros": bytes(300000),
        "rand_small": rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(),
        "rand_big": rng.integers(0, 256, 300000, dtype=np.uint8).tobytes(),                       # raw blocks
        "prices": rng.integers(90000, 10500000, 100000).astype(np.int64).tobytes(),
        "dates": np.sort(rng.integers(8000, 10600, 200000).astype(np.int32)).tobytes(),
        "text": text,
        "offsets": np.cumsum(rng.integers(10, 44, 200000)).astype(np.int32).tobytes(),
        "flags": rng.choice(np.frombuffer(b"ANR", dtype=np.uint8), 300000).tobytes(),            # 2-bit alphabet: direct weights
        "period": b"abcdefg" * 60000,
        "few": rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 3000, p=[0.9, 0.1]).tobytes(),
        "mixed": text[:150000] + rng.integers(0, 256, 50000, dtype=np.uint8).tobytes() + bytes(70000) + text[:90000],
    }
    args = []
    for name, data in cases.items():
        raw = str(tmp_path / (name + ".raw"))
        open(raw, "wb").write(data)
        for level in (1, 3, 19):
            z = str(tmp_path / ("%s_%d.zst" % (name, level)))
            open(z, "wb").write(pa.Codec("zstd", compression_level=level).compress(data, asbytes=True))
            args += [z, raw]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "%d frames, 0 failed" % (len(args) // 2) in run.stdout, run.stdout[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    # every table mode and literal type the format has was seen (the first printed line counts them)
    import re
    seen = [int(x) for x in re.findall(r"\d+", run.stdout.split("\n")[0])]
    assert all(v > 0 for v in seen[:3]), run.stdout


def test_readahead_orders_and_shards_under_tsan(tmp_path):
    """The scan's read-ahead (duckdb-arrow_amd/csrc/scan_readahead.cpp: producer threads, per-producer queues, staging
    leases) is host code with the GPU behind two hooks, so tests/sanitize/readahead_check.cpp runs it under ThreadSanitizer
    with malloc for pinned memory: for 1 to 4 producers and for world 1 and ranks 0..2 of world 3 every batch of the share
    comes out once, in stream order, byte-equal to a single-threaded read; a missing file in the middle of the list fails
    after the batches before it; stopping while the producers are blocked returns."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    import numpy as np
    import pyarrow as pa
    import pyarrow.ipc as ipc
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / "readahead_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "sanitize", "readahead_check.cpp"), os.path.join(csrc, "scan_readahead.cpp")] + READER_HOST_SOURCES +
        ["-ldl", "-lpthread", "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    rng = np.random.default_rng(11)

    def write(name, n_batches, compression=None, dictionary=False):
        rows = 400
        cols = {"k": np.arange(n_batches * rows, dtype=np.int64), "v": rng.integers(0, 1 << 40, n_batches * rows),
                "s": ["row %d of %s" % (i % 53, name) for i in range(n_batches * rows)]}
        t = pa.table(cols)
        if dictionary:
            t = t.append_column("d", pa.array(["tag %d" % (i % 7) for i in range(n_batches * rows)]).dictionary_encode())
        path = str(tmp_path / name)
        with ipc.new_stream(path, t.schema, options=ipc.IpcWriteOptions(compression=compression)) as w:
            w.write_table(t, max_chunksize=rows)
        return path

    cases = {
        "plain": ([write("p%d.arrows" % i, 30 + 3 * i) for i in range(4)], [], 1),
        # LZ4 bodies that the reader's host threads decompress: three producers unless told otherwise
        "lz4": ([write("z%d.arrows" % i, 28 + 5 * i, compression="lz4") for i in range(3)], [], 3),
        # dictionary batches order every later batch of their file: one producer, whatever is asked for
        "dict": ([write("d%d.arrows" % i, 32 + i, dictionary=True) for i in range(3)], ["--dict"], 1),
    }
    for name, (files, flags, producers) in cases.items():
        run = subprocess.run([exe] + flags + files, capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, MI_IO_THREADS="2", TSAN_OPTIONS="halt_on_error=0"))
        assert run.returncode == 0, (name, run.stdout[-1000:], run.stderr[-3000:])
        assert "ThreadSanitizer" not in run.stderr and "FAILED" not in run.stderr, (name, run.stderr[-3000:])
        assert "%d producers by default" % producers in run.stdout and "32 runs, 0 failed" in run.stdout, (name, run.stdout)


def test_writer_plan_under_asan_ubsan_and_tsan(tmp_path):
    """The writer's planning unit (duckdb-arrow_amd/csrc/writer_plan.cpp: IPC body layout, encode tasks, the COPY pumps' cut
    rule and batch ledger) is host code, so tests/sanitize/writer_plan_check.cpp runs it from that one source: buffer
    lengths and alignment against the Arrow columnar format for every node kind, the int32 offset limit, the cutter against
    a naive chunk-by-chunk cut, and the ledger with four closing threads -- once under ASan + UBSan, once under TSan."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for name, flags in (("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), ("tsan", ["-fsanitize=thread"])):
        exe = str(tmp_path / ("writer_plan_check_" + name))
        build = subprocess.run(
            ["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "include"),
             os.path.join(ROOT, "tests", "sanitize", "writer_plan_check.cpp"),
             os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "writer_plan.cpp"), "-lpthread", "-o", exe],
            capture_output=True, text=True)
        if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
            pytest.skip("sanitizer runtime not installed")
        assert build.returncode == 0, build.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=0"))
        assert run.returncode == 0, (name, run.stdout[-1000:], run.stderr[-3000:])
        assert " 0 failed" in run.stdout and "FAILED" not in run.stderr, (name, run.stdout, run.stderr[-3000:])
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (name, run.stderr[-3000:])


def test_io_pool_under_tsan_and_asan_ubsan(tmp_path):
    """The process-wide I/O pool and the NUMA binding (duckdb-arrow_amd/csrc/io_pool.cpp) serve every scan, every device and
    the host decompressors; tests/sanitize/io_pool_check.cpp runs them from that one source, once under TSan and once under
    ASan + UBSan: the serial path, six callers at once on four threads, a task that throws, a nested call, EnsureIoThreads
    against the CPU budget of this process, and BindThisThreadToNode / PreferNode (that they return and the pool still works,
    nothing about placement)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    for name, flags in (("tsan", ["-fsanitize=thread"]), ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / ("io_pool_check_" + name))
        build = subprocess.run(
            ["g++", "-std=c++17", "-O1", "-g"] + flags + [os.path.join(ROOT, "tests", "sanitize", "io_pool_check.cpp"),
             os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "io_pool.cpp"), "-lpthread", "-o", exe],
            capture_output=True, text=True)
        if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
            pytest.skip("sanitizer runtime not installed")
        assert build.returncode == 0, build.stderr[-2000:]
        # the pool reads MI_IO_THREADS once, when it is first used: one process per setting
        for threads, case in (("1", "serial"), ("4", "pool")):
            run = subprocess.run([exe, case], capture_output=True, text=True, timeout=300,
                                 env=dict(os.environ, MI_IO_THREADS=threads, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                          TSAN_OPTIONS="halt_on_error=0"))
            assert run.returncode == 0, (name, case, run.stdout[-1000:], run.stderr[-3000:])
            assert re.search(r"^\d+ checks, 0 failed$", run.stdout, re.M), (name, case, run.stdout, run.stderr[-3000:])
            assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, (name, case, run.stderr[-3000:])


def _build_and_run_check(tmp_path, name, sources):
    """g++ -fsanitize=address,undefined over tests/sanitize/<name>.cpp and `sources` (of csrc); the headers name HIP types,
    so the ROCm include directory is on the path, but nothing of HIP is called or linked."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "duckdb-arrow_amd", "csrc")
    exe = str(tmp_path / name)
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-I", os.path.join(ROOT, "include"), "-I", csrc, "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
         os.path.join(ROOT, "tests", "sanitize", name + ".cpp")] + [os.path.join(csrc, s) for s in sources] + ["-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr and "FAILED" not in run.stderr, run.stderr[-3000:]
    m = re.search(r"^(\d+) checks, 0 failed$", run.stdout, re.M)
    assert m, run.stdout
    return int(m.group(1))


def test_k8_scratch_arena_under_asan_and_ubsan(tmp_path):
    """The K8 staging's arithmetic (duckdb-arrow_amd/csrc/scan_k8.cpp: where every table, counter and scratch array of a
    compressed record batch lies, the pinned tables, the launch arguments) is host code without a HIP call;
    tests/sanitize/k8_scratch_check.cpp runs it over hand-built LZ4 and ZSTD bodies -- empty, 0 / 1 / 300 blocks, a raw buffer
    between compressed ones, stored blocks, a 1-byte and a 4 MiB block -- against offsets written out from the rule
    round_up(bytes + 16, 256), and fills the tables into an allocation of exactly the reported size."""
    assert _build_and_run_check(tmp_path, "k8_scratch_check", ["scan_k8.cpp"]) > 3000


def test_dictionary_host_side_under_asan_and_ubsan(tmp_path):
    """The host side of a dictionary version (duckdb-arrow_amd/csrc/scan_dictionary.cpp: validity words, host_valid,
    host_strings with their offset checks, host_values with the float16 widening) reads bytes that come from a file;
    tests/sanitize/dictionary_host_check.cpp runs it over hand-built DictionaryBatch bodies whose buffer under test ends the
    allocation: replace and delta, bitmaps, the word edges 0 / 1 / 63 / 64 / 65, STR32 / STR64 / FIXED_BINARY, float16 against
    numpy's bit patterns, float64, 128-bit values, and damaged inputs beside clean twins, each of which must raise."""
    assert _build_and_run_check(tmp_path, "dictionary_host_check", ["scan_dictionary.cpp"]) > 60000

"""The ZSTD frame corpus of tests/zstd_frames.py on the CPU, before a kernel sees it (tests/test_gpu_zstd_frames.py):
libzstd -- ZSTD_decompress, what host_codec.cpp calls, and pyarrow's codec -- must agree with the builder about what every
valid frame means and turn the invalid ones down; tests/sanitize/zstd_check.cpp, the CPU build of the kernels' stages
(zstd_format.hpp, WalkZstdFrame) under ASan + UBSan, must decode every valid frame to the same bytes and refuse every
other; and the hand-built corpus ALONE must reach every block type, literal type, stream count and table mode the format has.

Where libzstd 1.4.8 accepts what RFC 8878 forbids (LIBZSTD_ACCEPTS), the test says so and does not ask it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import lz4_frames as lf
import zstd_frames as zf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Invalid frames the one-shot decoder of libzstd 1.4.8 decodes all the same (later releases refuse some of them), so libzstd
# is not the judge of these; the CPU build of the stages is, and on the device each of them is an error:
#   rep0_minus_1_is_zero            RFC 8878 3.1.1.5: "an offset of 0 is invalid"; libzstd 1.4.8 turns it into 1
#   block_output_passes_128_kib     RFC 8878 3.1.1.2.4 Block_Maximum_Size; the one-shot decoder only knows the output's end
#   bitstream_one_byte_too_many     RFC 8878 3.1.1.4: "the bitstream must be consumed exactly"; 1.4.8 only counts sequences
#   bitstream_runs_out              as above: the last sequence reads zeros in front of the stream
#   block_larger_than_the_window    RFC 8878 3.1.1.2.4; the one-shot decoder has no window.  The walk refuses this one, the host
#                                   library decodes it: data, not an error -- the GPU expectation follows libzstd
LIBZSTD_ACCEPTS = ("rep0_minus_1_is_zero", "block_output_passes_128_kib", "bitstream_one_byte_too_many", "bitstream_runs_out",
                   "block_larger_than_the_window")


@pytest.fixture(scope="module")
def corpus():
    return zf.valid_cases()


def test_the_encoders_round_trip_known_bits():
    assert zf.ll_code(15) == (15, 0, 0) and zf.ll_code(16) == (16, 0, 1) and zf.ll_code(65536 + 5) == (35, 5, 16)
    assert zf.ml_code(3) == (0, 0, 0) and zf.ml_code(35) == (32, 0, 1) and zf.ml_code(131071 + 3) == (52, 65535, 16)
    assert zf.of_code(7) == (2, 3, 2)
    # RFC 8878 4.2.1.1's example: weights 4 3 2 0 1 and the implied 1 -> codes of 1, 2, 3, 4, 4 bits
    bits, codes = zf.huffman_codes([4, 3, 2, 0, 1, 1])
    assert bits == 4 and codes == {0: (1, 1), 1: (1, 2), 2: (1, 3), 4: (0, 4), 5: (1, 4)}
    assert zf.huffman_description([4, 3, 2, 0, 1, 1]) == bytes([127 + 5, 0x43, 0x20, 0x10])
    # the predefined offset table: 32 states, state 0 decodes code 0 with 5 bits (RFC 8878 appendix A)
    t = zf.fse_table(*zf.PREDEFINED[zf.OF])
    assert len(t) == 32 and t[0] == (0, 0, 5) and t[1] == (6, 0, 4) and t[31] == (24, 0, 5)
    t = zf.fse_table(*zf.PREDEFINED[zf.LL])
    assert t[0] == (0, 0, 4) and t[1] == (0, 16, 4) and t[63] == (32, 0, 6) and t[60] == (35, 0, 6)
    assert zf.frame_header(content_size=256, fcs_bytes=2) == zf.MAGIC + b"\x60\x00\x00"


@pytest.mark.parametrize("name", list(zf.valid_cases()))
def test_hand_built_frames_mean_to_libzstd_what_the_builder_says(corpus, name):
    c = corpus[name]
    assert zf.libzstd_decompress(c["frame"], len(c["want"])) == c["want"]
    assert pa.Codec("zstd").decompress(c["frame"], decompressed_size=len(c["want"])).to_pybytes() == c["want"]


def test_hand_built_frames_reach_what_they_are_about(corpus):
    assert {x % 4 for x in corpus["z2_raw_alignment"]["literals_at"]} == {0, 1, 2, 3}
    assert sorted(corpus["z7_fat_sequences_%d" % i]["bitstream_at"][-1] % 4 for i in range(4)) == [0, 1, 2, 3]
    for i in range(4):      # 220 sequences of > 55 bits: 1.5 KiB of bitstream, more than one window
        c = corpus["z7_fat_sequences_%d" % i]
        assert len(c["frame"]) - c["bitstream_at"][-1] > 220 * 55 // 8
    t = zf.huffman_tables()
    assert len(t["two"]) == 2 and len(t["full_128"]) == 129 and zf.huffman_codes(t["eleven_bits"])[0] == 11
    assert sum(1 for w in t["wave_fill"] if w == 8) == 3            # 128 cells each: the whole-wave fill
    q = [s for s, w in enumerate(t["quarters"]) if w == 3]
    assert min(q) < 64 and any(64 <= s < 128 for s in q) and max(q) == 128
    lib = zf.libzstd_all_quarters()
    assert lib["frame"][:4] == zf.MAGIC and len(set(lib["want"][i] >> 6 for i in range(len(lib["want"])))) == 4
    r = zf.refused_cases()
    assert r["content_checksum"]["frame"][4] & 0x04 and r["trailing_skippable_frame"]["frame"].endswith(zf.skippable_frame())
    assert r["two_frames"]["frame"].count(zf.MAGIC) == 2


@pytest.mark.parametrize("name", list(zf.refused_cases()))
def test_frames_the_walk_refuses_are_still_zstd_to_the_host(name):
    c = zf.refused_cases()[name]
    assert zf.libzstd_decompress(c["frame"], len(c["want"])) == c["want"]
    stream, table = lf.ipc_stream([c], [c["frame"]], codec="zstd")
    assert pa.ipc.open_stream(pa.py_buffer(stream)).read_all().equals(table)
    rd = da.Reader(buffers=[stream])      # the batch's body lives as long as its reader
    b = rd.next_batch()
    off, ln = b["buffers"][1]
    assert b["body"][off: off + ln].tobytes() == c["want"]


@pytest.mark.parametrize("name", list(zf.invalid_cases()))
def test_invalid_frames_are_turned_down(name):
    """libzstd rejects the frame (or is known not to: LIBZSTD_ACCEPTS), and so does the host reader, which decompresses with
    the same library and ends with the reference's I/O error."""
    frame, declared, on_device, why, want = zf.invalid_cases()[name]
    assert why
    if name in LIBZSTD_ACCEPTS:
        try:
            got = zf.libzstd_decompress(frame, declared)
        except ValueError:
            return          # a later libzstd that refuses it: all the better
        if want is not None:
            assert got == want
        return
    with pytest.raises(ValueError):
        zf.libzstd_decompress(frame, declared + 64)
    col = dict(dtype="uint8", want=bytes(declared))
    stream, _ = lf.ipc_stream([col], [frame], codec="zstd")
    with pytest.raises(da.MiError) as e:
        da.Reader(buffers=[stream]).next_batch()
    assert e.value.code == _ffi.MI_EIO


def test_host_reader_scans_a_rewritten_stream(corpus):
    for name in ("z1_block_types", "z2_treeless", "z4_three_sources", "z6_only_repeats", "z8_window_no_size"):
        c = corpus[name]
        stream, table = lf.ipc_stream([c], [c["frame"]], codec="zstd")
        assert pa.ipc.open_stream(pa.py_buffer(stream)).read_all().equals(table)
        rd = da.Reader(buffers=[stream])
        b = rd.next_batch()
        off, ln = b["buffers"][1]
        assert ln == len(c["want"]) and b["body"][off: off + ln].tobytes() == c["want"], name


# ------------------------------------------------------------------------------------- the CPU build of the kernels' stages
@pytest.fixture(scope="module")
def zstd_check(tmp_path_factory):
    """tests/sanitize/zstd_check.cpp as a stand-alone program under ASan + UBSan (the recipe of
    tests/test_sanitizers.py::test_zstd_stages_on_the_cpu)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("zstd_check") / "zstd_check")
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "zstd_check.cpp"),
         os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "frame_walk.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def _coverage(stdout):
    """The 23 counters zstd_check prints: name -> count."""
    names = ["block raw", "block rle", "block compressed", "literals raw", "literals rle", "literals huffman", "literals treeless",
             "1 stream", "4 streams", "weights fse", "weights direct"]
    line = next(l for l in stdout.split("\n") if l.startswith("blocks raw/rle/compressed"))
    nums = [int(x) for x in re.findall(r"\d+", line.replace("1/4 streams", "streams"))]
    assert len(nums) == 11, line
    seen = dict(zip(names, nums))
    for t, tn in enumerate(("ll", "of", "ml")):
        m = re.search(r"table %d predefined/rle/fse/repeat (\d+)/(\d+)/(\d+)/(\d+)" % t, stdout)
        for mode, v in zip(("predefined", "rle", "fse", "repeat"), m.groups()):
            seen["%s %s" % (tn, mode)] = int(v)
    assert len(seen) == 23
    return seen


def _run(exe, args):
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    return run


def test_the_cpu_build_of_the_stages_decodes_every_valid_frame(zstd_check, corpus, tmp_path):
    """... and the hand-built corpus alone reaches 22 of the 23 coverage counters; the 23rd, FSE-compressed Huffman weights,
    cannot be built here (zstd_frames.py writes direct weights only) and comes from the ONE libzstd-written frame of the run."""
    def args_of(cases):
        args = []
        for name, c in cases.items():
            f, w = str(tmp_path / (name + ".zst")), str(tmp_path / (name + ".raw"))
            open(f, "wb").write(c["frame"])
            open(w, "wb").write(c["want"])
            args += [f, w]
        return args
    run = _run(zstd_check, args_of(corpus))
    assert run.returncode == 0 and "%d frames, 0 failed" % len(corpus) in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    seen = _coverage(run.stdout)
    assert seen.pop("weights fse") == 0                       # direct weights only
    assert all(v > 0 for v in seen.values()), seen
    run = _run(zstd_check, args_of(dict(corpus, libzstd_all_quarters=zf.libzstd_all_quarters())))
    assert run.returncode == 0, run.stdout[-3000:]
    seen = _coverage(run.stdout)
    assert len(seen) == 23 and all(v > 0 for v in seen.values()), seen


def test_the_cpu_build_of_the_stages_refuses_every_other_frame(zstd_check, tmp_path):
    """The invalid frames (each stopped by the bound its `why` cites, none by a sanitizer) and the valid ones the walk leaves
    to the host library."""
    args, n = [], 0
    for name, (frame, declared, _, _, _) in zf.invalid_cases().items():
        f = str(tmp_path / (name + ".zst"))
        open(f, "wb").write(frame)
        args += ["--refuse", f, str(declared)]
        n += 1
    for name, c in zf.refused_cases().items():
        f = str(tmp_path / (name + ".zst"))
        open(f, "wb").write(c["frame"])
        args += ["--refuse", f, str(len(c["want"]))]
        n += 1
    run = _run(zstd_check, args)
    assert run.returncode == 0 and "%d frames refused as expected" % n in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    walk = re.findall(r"refused \S*/(\w+)\.zst: walk refused", run.stdout)
    assert sorted(walk) == sorted([k for k, v in zf.invalid_cases().items() if not v[2]] + list(zf.refused_cases())), run.stdout

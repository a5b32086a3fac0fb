"""K8 on LZ4 frames pyarrow never writes (tests/lz4_frames.py): 256 KiB to 4 MiB blocks, independent blocks, block and
content checksums, content size -- written by liblz4 (L) -- and frames built by hand (H) for the edges of the seven kernels of
kernels_lz4.hip: chains of chunk-to-chunk links around and far beyond what one skeleton round follows, blocks that begin at
positions that are no multiple of 4, length-extension bytes at their edges, overlapping matches across chunk boundaries,
the largest offsets, the densest and the emptiest blocks, stored blocks, and compressed block sizes on either side of the two
thresholds that pick the token-walk kernel.  tests/test_lz4_frames_host.py proves the same corpus against liblz4 on the CPU.

How a case runs: the bytes a frame stands for become an int64 (or uint8) column, pyarrow writes the table with
compression="lz4", helpers.rewrite_buffers puts the frame under test in place of pyarrow's.  Every valid case is read three
ways -- device resident, host consumer with host decompression (liblz4), host consumer with device decompression -- and all
three must return the bytes that went in, with the device-batch counter showing where the frame was decompressed.

The device path SKIPS the LZ4 block and content checksums (WalkLz4Frame steps over them); the host path checks them
(liblz4 does).  A frame with a wrong checksum and intact blocks is therefore data on the device and an error on the host."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import lz4_frames as lf
from test_lz4_frames_host import LIBLZ4_VARIANTS, liblz4_data

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


@pytest.fixture(scope="module")
def corpus():
    return lf.hand_built_cases()


@pytest.fixture(scope="module")
def data():
    return liblz4_data()


def _scan_bytes(con, path, **kw):
    """Every column of a scan as one uint8 array of its vectors' data (fixed-width columns without nulls), and the stats."""
    hip = C.CDLL("libamdhip64.so") if kw.get("device_resident") else None
    rel = con.read_arrow(path, **kw)
    parts = [[] for _ in rel.types]
    for ch in rel.chunks():
        for ci in range(len(parts)):
            v = ch.columns[ci]
            nbytes = ch.size * v.out_width
            assert v.kind != _ffi.K_DICT and nbytes > 0
            if hip is not None:
                buf = np.empty(nbytes, np.uint8)
                assert hip.hipMemcpy(C.c_void_p(buf.ctypes.data), C.c_void_p(v.data), C.c_size_t(nbytes), 2) == 0
            else:
                buf = np.ctypeslib.as_array(C.cast(v.data, C.POINTER(C.c_uint8)), shape=(nbytes,)).copy()
            parts[ci].append(buf)
    st = rel.stats()
    rel.close()
    return [np.concatenate(p) if p else np.zeros(0, np.uint8) for p in parts], st


def _same(got, want, what):
    want = np.frombuffer(want, np.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d of %d bytes differ, first at %d, last at %d" % (what, len(bad), len(want), bad[0], bad[-1]))


def check_valid(con, path, columns, frames, name):
    """The three readings of one rewritten stream; -> the stats of the device-resident scan."""
    stream, _ = lf.ipc_stream(columns, frames)
    with open(path, "wb") as f:
        f.write(stream)
    dev = None
    for kw in (dict(device_resident=True), dict(host_decompress=True), dict(host_decompress="gpu")):
        got, st = _scan_bytes(con, path, **kw)
        for ci, c in enumerate(columns):
            _same(got[ci], c["want"], (name, ci, kw))
        on_device = 0 if kw.get("host_decompress") is True else 1
        assert st["record_batches"] == 1 and st["lz4_batches_on_device"] == on_device, (name, kw, st)   # no silent fall-back
        dev = dev or st
    return dev


def check_hand_built(con, path, columns, name):
    st = check_valid(con, path, columns, [lf.column_frame(c) for c in columns], name)
    # every compressed block is walked by exactly one of the parse kernels (stored blocks by none)
    assert st["lz4_blocks"] == sum(len(c["blocks"]) - len(c["stored"]) for c in columns), (name, st)


# ------------------------------------------------------------------------------------------------ written by liblz4 (L)
@pytest.mark.parametrize("name", list(LIBLZ4_VARIANTS))
def test_frames_written_by_liblz4(con, data, tmp_path, name):
    """L1-L7: block sizes 64 KiB to 4 MiB, independent blocks, block checksum, content checksum, content size, all of them at
    once, and the compression levels 0, 9 and 12 (other parsers, other sequences), over ~5 MiB."""
    prefs, flg, bd = LIBLZ4_VARIANTS[name]
    frame, got_flg, got_bd = lf.liblz4_frame(data, **prefs)
    assert (got_flg, got_bd) == (flg, bd)
    check_valid(con, str(tmp_path / "l.arrows"), [dict(dtype="int64", want=data)], [frame], name)


def test_three_flavours_in_one_record_batch(con, data, tmp_path):
    n = 3 << 19
    cols = [dict(dtype="int64", want=data[i * n: (i + 1) * n]) for i in range(3)]
    made = [lf.liblz4_frame(cols[0]["want"], bsid=5, block_checksum=True),
            lf.liblz4_frame(cols[1]["want"], bsid=4, independent=True, content_checksum=True),
            lf.liblz4_frame(cols[2]["want"], bsid=6, content_size=True)]
    assert [(f, b) for _, f, b in made] == [(0x50, 0x50), (0x64, 0x40), (0x48, 0x60)]
    check_valid(con, str(tmp_path / "three.arrows"), cols, [m[0] for m in made], "three flavours")


# --------------------------------------------------------------------------------------------------- built by hand (H)
@pytest.mark.parametrize("name", list(lf.hand_built_cases()))
def test_hand_built_frames(con, corpus, tmp_path, name):
    """H1-H8, one case each; what a case is about is in the docstring of its builder in tests/lz4_frames.py."""
    check_hand_built(con, str(tmp_path / "h.arrows"), corpus[name], name)


def run_small_cases(tmp_dir):
    """H9, in a child process whose environment forces one parse kernel for every block."""
    con = da.Connection(0)
    cases = lf.hand_built_cases()
    for name in lf.SMALL_CASES:
        check_hand_built(con, os.path.join(tmp_dir, name + ".arrows"), cases[name], name)


@pytest.mark.parametrize("variant", ["MI_LZ4_PARSE_SPECULATIVE", "MI_LZ4_PARSE_GLOBAL"])
def test_small_cases_under_a_forced_parse_kernel(tmp_path, variant):
    """H9: H2 to H6 and H8 once more with lz4_parse<true> (MI_LZ4_PARSE_SPECULATIVE) and with lz4_parse<false>
    (MI_LZ4_PARSE_GLOBAL) walking every block; the launcher reads the variable once per process, hence a fresh child."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_lz4_frames as t; t.run_small_cases(%r); print('ok')"
            % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **{variant: "1"}), timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------ invalid frames
@pytest.fixture(scope="module")
def good_file(con, tmp_path_factory):
    want = np.arange(5000, dtype=np.int64).tobytes()
    path = str(tmp_path_factory.mktemp("lz4_good") / "good.arrows")
    stream, _ = lf.ipc_stream([dict(dtype="int64", want=want)], [None])
    with open(path, "wb") as f:
        f.write(stream)
    return path, want


@pytest.mark.parametrize("name", list(lf.invalid_cases()))
def test_invalid_frames_end_in_an_error_never_in_data(con, good_file, tmp_path, name):
    """A block-independent frame whose match reaches into the block before it (liblz4: ERROR_decompressionFailed), offset 0,
    an offset one byte in front of the buffer, a block that outgrows the frame's block maximum, blocks that add up to 8
    bytes fewer than declared: MI_EIO / MI_EINVAL from both device paths, and the connection reads a good file afterwards."""
    frame, declared = lf.invalid_cases()[name]
    col = dict(dtype="int64", want=np.random.default_rng(1).integers(0, 256, declared, dtype=np.uint8).tobytes())
    stream, _ = lf.ipc_stream([col], [frame])
    path = str(tmp_path / "bad.arrows")
    with open(path, "wb") as f:
        f.write(stream)
    for kw in (dict(device_resident=True), dict(host_decompress="gpu")):
        with pytest.raises(da.MiError) as e:
            _scan_bytes(con, path, **kw)
        assert e.value.code in (_ffi.MI_EIO, _ffi.MI_EINVAL), (name, kw, str(e.value))
    good, want = good_file
    got, st = _scan_bytes(con, good, device_resident=True)
    _same(got[0], want, "good file after " + name)
    assert st["lz4_batches_on_device"] == 1


# ------------------------------------------------------------------------------------------- frames the walk refuses
def test_a_dictionary_id_sends_the_batch_to_the_host(con, tmp_path):
    col = lf.refused_cases()["dictionary_id"]
    stream, _ = lf.ipc_stream([col], [lf.column_frame(col)])
    path = str(tmp_path / "dict_id.arrows")
    with open(path, "wb") as f:
        f.write(stream)
    for kw in (dict(device_resident=True), dict(host_decompress="gpu"), dict(host_decompress=True)):
        got, st = _scan_bytes(con, path, **kw)
        _same(got[0], col["want"], ("dictionary id", kw))
        assert st["lz4_batches_on_device"] == 0 and st["record_batches"] == 1, (kw, st)


def test_block_size_id_3_never_reaches_the_device(con, good_file, tmp_path):
    """BD with bsid 3 (reserved by lz4_Frame_format.md): the walk refuses it, so the host library gets the record batch --
    and liblz4 has no values for it either (ERROR_maxBlockSize_invalid, tests/test_lz4_frames_host.py): the scan ends with
    the host path's I/O error and nothing was launched."""
    frame, declared = lf.bsid3_frame()
    col = dict(dtype="int64", want=bytes(declared))
    stream, _ = lf.ipc_stream([col], [frame])
    path = str(tmp_path / "bsid3.arrows")
    with open(path, "wb") as f:
        f.write(stream)
    rel = con.read_arrow(path, device_resident=True)
    with pytest.raises(da.MiError, match="maxBlockSize") as e:
        for _ in rel.chunks():
            pass
    assert e.value.code == _ffi.MI_EIO
    assert rel.stats()["lz4_batches_on_device"] == 0
    rel.close()
    good, want = good_file
    _same(_scan_bytes(con, good, device_resident=True)[0][0], want, "good file after bsid 3")


# ------------------------------------------------------------------------------------- ZSTD: the shared copy stages
def test_zstd_periods_linked_across_many_chunks(con, tmp_path):
    """The stages behind the parse kernels are shared with ZSTD: a 200 KiB random period tiled 30 times, zstd level 3 -- every
    period is matches 25 chunks back into the period before it, 29 periods deep, more than one skeleton round follows."""
    period = np.random.default_rng(8).integers(0, 256, 200 << 10, dtype=np.uint8)
    want = np.tile(period, 30).tobytes()
    table = pa.table({"p": pa.array(np.frombuffer(want, np.int64))})
    path = str(tmp_path / "periods.arrows")
    with ipc.new_stream(path, table.schema, options=ipc.IpcWriteOptions(compression=pa.Codec("zstd", compression_level=3))) as w:
        w.write_table(table, max_chunksize=table.num_rows)
    assert os.path.getsize(path) < len(want) // 10          # the periods were found
    got, st = _scan_bytes(con, path, host_decompress="gpu")
    _same(got[0], want, "zstd periods")
    assert st["zstd_batches_on_device"] > 0
    got, st = _scan_bytes(con, path, host_decompress=True)
    _same(got[0], want, "zstd periods, host")
    assert st["zstd_batches_on_device"] == 0

"""K8 on ZSTD frames libzstd never writes (tests/zstd_frames.py), built by hand for the paths of kernels_zstd.inl the
libzstd-written corpus of test_gpu_zstd.py does not reach: RLE and raw blocks between compressed ones, RLE / treeless /
single-stream literals, direct Huffman weights up to 11 bits, Repeat_Mode and RLE_Mode sequence tables taken from three
different blocks, sequence counts around the 64-sequence group and the slice size, repeat codes at every boundary and a block
of nothing but repeat codes, the longest codes, the fattest bitstreams, every frame header.  What a case is about is in the
docstring of its builder.  tests/test_zstd_frames_host.py proves the same corpus against libzstd on the CPU.

How a case runs: the bytes a frame stands for become a uint8 (or int64) column, pyarrow writes the table with
compression="zstd", helpers.rewrite_buffers puts the frame under test in place of pyarrow's.  Every valid case is read three
ways -- device resident and host consumer, both with device decompression, and host decompression (libzstd) -- and all three
must return the bytes the builder computed, with the device-batch counter showing where the frame was decompressed.

The device path SKIPS nothing it accepts and accepts no frame with a content checksum, a dictionary id or anything behind the
last block: those go to the host library whole."""
import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import lz4_frames as lf
import zstd_frames as zf
from test_gpu_lz4_frames import _same, _scan_bytes
from test_zstd_frames_host import LIBZSTD_ACCEPTS

pytestmark = pytest.mark.gpu

READINGS = ((dict(device_resident=True, host_decompress="gpu"), 1), (dict(host_decompress="gpu"), 1), (dict(host_decompress=True), 0))


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


@pytest.fixture(scope="module")
def corpus():
    return zf.valid_cases()


def _write(path, col, frame):
    stream, _ = lf.ipc_stream([col], [frame], codec="zstd")
    with open(path, "wb") as f:
        f.write(stream)


def check_three_readings(con, path, case, name, on_device=True):
    _write(path, case, case["frame"])
    for kw, dev in READINGS:
        got, st = _scan_bytes(con, path, **kw)
        _same(got[0], case["want"], (name, kw))
        # no silent fall-back, in either direction
        assert st["record_batches"] == 1 and st["zstd_batches_on_device"] == (dev if on_device else 0) and st["lz4_batches_on_device"] == 0, (name, kw, st)


@pytest.mark.parametrize("name", list(zf.valid_cases()))
def test_hand_built_frames(con, corpus, tmp_path, name):
    """Z1-Z8, one case each."""
    check_three_readings(con, str(tmp_path / "z.arrows"), corpus[name], name)


def test_huffman_symbols_in_all_four_quarters(con, tmp_path):
    """The one libzstd-written frame: Huffman symbols 129..255, which direct weights cannot name (zstd_frames.py)."""
    check_three_readings(con, str(tmp_path / "q.arrows"), zf.libzstd_all_quarters(), "libzstd_all_quarters")


@pytest.mark.parametrize("name", list(zf.refused_cases()))
def test_frames_the_walk_refuses_go_to_the_host(con, tmp_path, name):
    """A content checksum (the device path has no XXH64), a skippable frame or a second frame behind the first."""
    check_three_readings(con, str(tmp_path / "r.arrows"), zf.refused_cases()[name], name, on_device=False)


@pytest.fixture(scope="module")
def good_file(con, tmp_path_factory):
    want = np.arange(5000, dtype=np.int64).tobytes()
    path = str(tmp_path_factory.mktemp("zstd_good") / "good.arrows")
    _write(path, dict(dtype="int64", want=want), None)
    return path, want


@pytest.mark.parametrize("name", list(zf.invalid_cases()))
def test_invalid_frames_end_in_an_error_never_in_data(con, good_file, tmp_path, name):
    """Every case of zstd_frames.invalid_cases(), whose `why` names the bound that stops it: MI_EIO / MI_EINVAL from both
    device paths -- from the kernels' status word where the walk takes the frame, from libzstd through the host path where the
    walk refuses it (nothing is launched then: the device counter stays 0) -- and the connection reads a good file afterwards.
    block_larger_than_the_window is the exception (LIBZSTD_ACCEPTS): the walk refuses it, libzstd's one-shot decoder knows no
    window and decodes it, so it is data from the host on every path."""
    frame, declared, on_device, why, want = zf.invalid_cases()[name]
    path = str(tmp_path / "bad.arrows")
    if not on_device and name in LIBZSTD_ACCEPTS:
        try:
            zf.libzstd_decompress(frame, declared)
            accepted = True
        except ValueError:
            accepted = False
        if accepted:
            check_three_readings(con, path, dict(dtype="uint8", frame=frame, want=want), name, on_device=False)
            return
    col = dict(dtype="uint8", want=np.random.default_rng(1).integers(0, 256, declared, dtype=np.uint8).tobytes())
    _write(path, col, frame)
    for kw in (dict(device_resident=True, host_decompress="gpu"), dict(host_decompress="gpu")):
        rel = None
        with pytest.raises(da.MiError) as e:
            rel = con.read_arrow(path, **kw)
            for _ in rel.chunks():
                pass
        assert e.value.code in (_ffi.MI_EIO, _ffi.MI_EINVAL), (name, kw, str(e.value))
        if rel is not None:
            assert on_device or rel.stats()["zstd_batches_on_device"] == 0
            rel.close()
    good, good_want = good_file
    got, st = _scan_bytes(con, good, device_resident=True, host_decompress="gpu")
    _same(got[0], good_want, "good file after " + name)
    assert st["zstd_batches_on_device"] == 1

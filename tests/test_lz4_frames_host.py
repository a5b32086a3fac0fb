"""The LZ4 frame corpus of tests/lz4_frames.py against liblz4, on the CPU: before a kernel sees a hand-built frame
(tests/test_gpu_lz4_frames.py), liblz4 -- through pyarrow's codec, through LZ4F_decompress and through the host reader --
must agree with the naive decoder about what it means, and must turn the invalid ones down."""
import numpy as np
import pyarrow as pa
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import lz4_frames as lf


@pytest.fixture(scope="module")
def corpus():
    return lf.hand_built_cases()


def test_xxh32_and_sequence_encoding():
    assert lf.xxh32(b"") == 0x02CC5D05 and lf.xxh32(b"abc") == 0x32D153FF            # the xxHash specification's vectors
    data = np.random.default_rng(0).integers(0, 256, 57 << 10, dtype=np.uint8).tobytes()
    frame, flg, _ = lf.liblz4_frame(data, content_checksum=True)                       # liblz4's own XXH32 of 57 KiB
    assert flg & 0x04 and int.from_bytes(frame[-4:], "little") == lf.xxh32(data)
    assert lf.seq(3, b"abc") == b"\x30abc"
    assert lf.seq(0, b"", 1, 4) == b"\x00\x01\x00"
    assert lf.seq(15, b"x" * 15, 0x1234, 19) == b"\xff\x00" + b"x" * 15 + b"\x34\x12\x00"          # 15 + 0 on both sides
    assert lf.seq(270, b"y" * 270, 7, 274)[:3] == b"\xff\xff\x00" and lf.seq(270, b"y" * 270, 7, 274)[-2:] == b"\xff\x00"
    assert lf.decode_blocks([lf.seq(2, b"ab", 2, 6) + lf.seq(5, b"vwxyz")]) == b"abababab" + b"vwxyz"


@pytest.mark.parametrize("name", list(lf.hand_built_cases()))
def test_hand_built_frames_mean_to_liblz4_what_the_naive_decoder_says(corpus, name):
    for col in corpus[name]:
        want = col["want"]
        frame = lf.column_frame(col)
        assert pa.Codec("lz4").decompress(frame, decompressed_size=len(want)).to_pybytes() == want
        assert lf.liblz4_decompress(frame, len(want)) == want
        assert max(len(b) for i, b in enumerate(col["blocks"])) <= 1 << (8 + 2 * col["bsid"])


def test_hand_built_frames_hit_the_sizes_they_are_about(corpus):
    comp = lambda name: [len(b) for i, b in enumerate(corpus[name][0]["blocks"]) if i not in corpus[name][0]["stored"]]
    for name, sizes in lf.H7_LAUNCHES.items():
        assert comp(name) == list(sizes)
    assert max(comp("h7_dp_only")) <= lf.DP_MAX
    assert min(comp("h7_dp_and_lds")) <= lf.DP_MAX < max(comp("h7_dp_and_lds")) <= lf.LDS_MAX
    assert min(comp("h7_dp_and_global")) <= lf.DP_MAX and max(comp("h7_dp_and_global")) > lf.LDS_MAX
    assert lf.DP_MAX < min(comp("h7_lds_only")) and max(comp("h7_lds_only")) <= lf.LDS_MAX
    assert min(comp("h7_global_only")) > lf.LDS_MAX
    assert comp("h6_tiny_blocks")[1:5] == [1, 2, 13, 255]
    assert comp("h6_dense")[1] == 3 * 16380 + 13 and comp("h6_dense_64k")[1] == 65536
    assert len(corpus["h2_odd_blocks"][1]["want"]) % 8 == 5
    for chunks in (24, 26, 27, 630):
        assert len(corpus["h1_chain_%d" % chunks][0]["want"]) == chunks * lf.CHUNK


@pytest.mark.parametrize("name", list(lf.invalid_cases()))
def test_invalid_frames_are_turned_down(name):
    """liblz4 rejects the frame, or -- the frame that is 8 bytes short -- decodes it to fewer bytes than declared, which the
    reader's length check catches.  offset 0: lz4_Block_format.md calls it invalid and the naive decoder refuses it, but the
    liblz4 releases differ (1.9.3 copies from the match's own position without complaint), so liblz4 is not asked; on the
    device it is an error whatever the host library thinks."""
    frame, declared = lf.invalid_cases()[name]
    if name == "offset_zero":
        b = lf.Blocks(901)
        b.lit(100)
        b.match(0, 40)
        b.finish()
        with pytest.raises(ValueError, match="offset 0"):
            lf.decode_blocks(b.blocks)
        return
    if name == "eight_bytes_short_of_the_declared_length":
        assert len(lf.liblz4_decompress(frame, declared)) == declared - 8
    else:
        with pytest.raises(ValueError, match="ERROR_"):
            lf.liblz4_decompress(frame, declared + 64)
        with pytest.raises(Exception, match="LZ4"):
            pa.Codec("lz4").decompress(frame, decompressed_size=declared)
    # and the host reader, which decompresses with the same library, ends with the reference's I/O error
    col = dict(dtype="int64", want=np.random.default_rng(1).integers(0, 256, declared, dtype=np.uint8).tobytes())
    stream, _ = lf.ipc_stream([col], [frame])
    with pytest.raises(da.MiError) as e:
        da.Reader(buffers=[stream]).next_batch()
    assert e.value.code == _ffi.MI_EIO


def test_frames_the_walk_refuses_are_still_lz4_to_the_host():
    col = lf.refused_cases()["dictionary_id"]
    frame = lf.column_frame(col)
    assert frame[4] & 0x01
    assert lf.liblz4_decompress(frame, len(col["want"])) == col["want"]      # a dictionary id is a hint, the blocks use none
    frame, n = lf.bsid3_frame()
    assert frame[5] == 0x30
    with pytest.raises(ValueError, match="maxBlockSize"):                   # lz4_Frame_format.md reserves ids 0 to 3
        lf.liblz4_decompress(frame, n)


LIBLZ4_VARIANTS = {   # name -> (preferences, FLG, BD) of the frame LZ4F_compressFrame writes for > 4 MiB of input
    "bsid4": (dict(bsid=4), 0x40, 0x40), "bsid5": (dict(bsid=5), 0x40, 0x50), "bsid6": (dict(bsid=6), 0x40, 0x60),
    "bsid7": (dict(bsid=7), 0x40, 0x70),
    "bsid4_independent": (dict(bsid=4, independent=True), 0x60, 0x40), "bsid7_independent": (dict(bsid=7, independent=True), 0x60, 0x70),
    "block_checksum": (dict(block_checksum=True), 0x50, 0x40), "content_checksum": (dict(content_checksum=True), 0x44, 0x40),
    "content_size": (dict(content_size=True), 0x48, 0x40),
    "everything_bsid7_independent": (dict(bsid=7, independent=True, block_checksum=True, content_checksum=True, content_size=True), 0x7C, 0x70),
    "level0": (dict(level=0), 0x40, 0x40), "level9": (dict(level=9), 0x40, 0x40), "level12": (dict(level=12), 0x40, 0x40),
}


def liblz4_data(n=5 << 20):
    """~5 MiB of mixed text, sorted int32 and random bytes (more than one 4 MiB block), a multiple of 8."""
    rng = np.random.default_rng(42)
    words = [b"alpha", b"beta", b"gamma delta", b"epsilon ", b"lorem ipsum dolor sit amet, ", b"0123456789", b"\n"]
    text = b"".join(words[i] for i in rng.integers(0, len(words), 170000))[: 2 << 20]
    ints = np.sort(rng.integers(0, 1 << 28, (n - len(text)) * 2 // 3 // 4).astype(np.int32)).tobytes()
    noise = rng.integers(0, 256, n - len(text) - len(ints), dtype=np.uint8).tobytes()
    third = len(text) // 2
    out = text[:third] + ints + noise + text[third:]      # text at both ends: matches 3 MiB apart are out of any window
    assert len(out) == n and n % 8 == 0
    return out


@pytest.fixture(scope="module")
def data():
    return liblz4_data()


@pytest.mark.parametrize("name", list(LIBLZ4_VARIANTS))
def test_liblz4_writes_the_flavour_the_case_names(data, name):
    prefs, flg, bd = LIBLZ4_VARIANTS[name]
    small = name.startswith("level")          # the high-compression levels take seconds per MiB of noise: 1 MiB is enough here
    src = data[: 1 << 20] if small else data
    frame, got_flg, got_bd = lf.liblz4_frame(src, **prefs)
    assert (got_flg, got_bd) == (flg, bd)
    assert pa.Codec("lz4").decompress(frame, decompressed_size=len(src)).to_pybytes() == src
    if name == "level9":
        assert len(frame) < len(lf.liblz4_frame(src, level=0)[0])     # the level reached the compressor


def test_liblz4_changes_block_size_and_mode_for_small_inputs():
    """Why callers assert on the FLG / BD bytes they get: 3000 bytes asked for as 4 MiB linked blocks come out as one 64 KiB
    independent block."""
    _, flg, bd = lf.liblz4_frame(b"abcd" * 750, bsid=7)
    assert (flg, bd) == (0x60, 0x40)


def test_host_reader_scans_a_rewritten_stream(corpus):
    """The host reader (no GPU) over streams whose frames were replaced: every hand-built flavour comes back as its bytes."""
    for name in ("h2_odd_blocks", "h5_offsets", "h8_stored_checksums", "h1_chain_26_one_block"):
        cols = corpus[name]
        stream, table = lf.ipc_stream(cols, [lf.column_frame(c) for c in cols])
        assert pa.ipc.open_stream(pa.py_buffer(stream)).read_all().equals(table)
        rd = da.Reader(buffers=[stream])      # the batch's body lives as long as its reader
        b = rd.next_batch()
        assert b["length"] == table.num_rows
        for i, c in enumerate(cols):
            off, ln = b["buffers"][3 * i + 1]      # three slots per top-level column: validity, data, (unused)
            assert ln == len(c["want"]) and b["body"][off: off + ln].tobytes() == c["want"], (name, i)
    col = lf.refused_cases()["dictionary_id"]
    stream, table = lf.ipc_stream([col], [lf.column_frame(col)])
    rd = da.Reader(buffers=[stream])
    b = rd.next_batch()
    off, ln = b["buffers"][1]
    assert b["body"][off: off + ln].tobytes() == col["want"]

"""COPY ... (FORMAT ARROWS, COMPRESSION lz4) on the GPU: the compress kernel (csrc/kernels_lz4_encode.hip) against its serial
restatement byte for byte, the files through pyarrow, the host reader and the device-resident scan (K8), the two COPY pumps
against the one-thread sink, and rotation."""
import ctypes as C
import decimal
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi
from helpers import canon_python

pytestmark = pytest.mark.gpu

GOLDEN = ["edge_types.arrows", "edge_types2.arrows", "edge_nested.arrows", "edge_empty.arrows", "lineitem_sf0_01_head.arrows"]


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """<= 300 000 rows: int64, decimal, date, short and long strings, a list, 10 % NULLs, one all-random binary column."""
    rng = np.random.default_rng(77)
    n = 150000
    nulls = lambda: rng.random(n) < 0.1
    lens = rng.integers(0, 4, n)
    flat = rng.integers(0, 50, int(lens.sum())).astype(np.int32)
    t = pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64) * 3, mask=nulls()),
        "d": pa.array([decimal.Decimal(int(v)) / 100 for v in rng.integers(90000, 10500000, n)], pa.decimal128(15, 2)),
        "dt": pa.array(np.sort(rng.integers(8000, 10600, n)).astype(np.int32), pa.date32(), mask=nulls()),
        "s": pa.array(["tag %d" % (i % 13) for i in range(n)], mask=nulls()),
        "ls": pa.array(["carefully final deposits %d sleep furiously %s" % (i % 311, "x" * (i % 29)) for i in range(n)], mask=nulls()),
        "l": pa.ListArray.from_arrays(pa.array(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)), pa.array(flat)),
        "r": pa.array([rng.bytes(24) for _ in range(n)], pa.binary()),
    })
    path = str(tmp_path_factory.mktemp("seeded") / "seeded.arrows")
    with ipc.new_stream(path, t.schema) as w:
        w.write_table(t, max_chunksize=60000)
    return t, path


# ---- Arrow IPC metadata, read without the library under test: RecordBatch.compression and RecordBatch.buffers
def _field(buf, table, idx):
    vt = table - struct.unpack_from("<i", buf, table)[0]
    if 4 + 2 * idx >= struct.unpack_from("<H", buf, vt)[0]:
        return None
    off = struct.unpack_from("<H", buf, vt + 4 + 2 * idx)[0]
    return table + off if off else None


def record_batches(path):
    """[(codec or -1, [(offset, length), ...], body bytes)] of every record batch of a stream file"""
    out = []
    for msg in ipc.MessageReader.open_stream(path):
        if msg.type != "record batch":
            continue
        meta = msg.metadata.to_pybytes()
        root = struct.unpack_from("<I", meta, 0)[0]
        h = _field(meta, root, 2)
        rb = h + struct.unpack_from("<I", meta, h)[0]
        c = _field(meta, rb, 3)
        codec = -1
        if c is not None:
            ct = c + struct.unpack_from("<I", meta, c)[0]
            f = _field(meta, ct, 0)
            codec = 0 if f is None else struct.unpack_from("<b", meta, f)[0]
        b = _field(meta, rb, 2)
        vec = b + struct.unpack_from("<I", meta, b)[0]
        n = struct.unpack_from("<I", meta, vec)[0]
        spans = [struct.unpack_from("<qq", meta, vec + 4 + 16 * i) for i in range(n)]
        out.append((codec, spans, msg.body.to_pybytes() if msg.body is not None else b""))
    return out


def tables_equal(a, b):
    """Table.equals, with NaN equal to NaN (edge_types2 has them)"""
    if a.schema != b.schema or a.num_rows != b.num_rows:
        return False
    for x, y in zip(a.columns, b.columns):
        if pa.types.is_floating(x.type):
            x, y = x.combine_chunks(), y.combine_chunks()
            if not x.is_null().equals(y.is_null()):
                return False
            if not np.array_equal(x.fill_null(0).to_numpy(zero_copy_only=False), y.fill_null(0).to_numpy(zero_copy_only=False), equal_nan=True):
                return False
        elif not x.equals(y):
            return False
    return True


def compress_host(data):
    L = _ffi.lib()
    if not len(data):
        return b""
    a = np.frombuffer(data, dtype=np.uint8)
    size = C.c_int64()
    _ffi.check(L.mi_lz4_frame_compress_host(a.ctypes.data, len(data), None, 0, C.byref(size)))
    out = np.zeros(size.value, np.uint8)
    _ffi.check(L.mi_lz4_frame_compress_host(a.ctypes.data, len(data), out.ctypes.data, size.value, C.byref(size)))
    return out[: size.value].tobytes()


def check_file_against_restatement(packed_path, plain_path):
    """every buffer of every record batch of the compressed file == the restatement over the uncompressed file's buffer"""
    packed, plain = record_batches(packed_path), record_batches(plain_path)
    assert len(packed) == len(plain) and len(packed) > 0
    n_buffers = 0
    for (codec, spans, body), (codec0, spans0, body0) in zip(packed, plain):
        assert codec == 0 and codec0 == -1 and len(spans) == len(spans0)
        end = 0
        for (off, ln), (off0, ln0) in zip(spans, spans0):
            assert off % 8 == 0 and off >= end and off + ln <= len(body)
            assert body[end:off] == bytes(off - end)                       # padding is zero
            assert body[off: off + ln] == compress_host(body0[off0: off0 + ln0]), (n_buffers, ln0)
            end = off + ln
            n_buffers += 1
        assert len(body) % 8 == 0 and len(body) - end < 8 and body[end:] == bytes(len(body) - end)
    return n_buffers


# ---------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("rgs", [2048, 5000, None])
@pytest.mark.parametrize("name", GOLDEN + ["seeded"])
def test_round_trip_through_three_readers(con, golden_dir, seeded, tmp_path, name, rgs):
    src = seeded[1] if name == "seeded" else os.path.join(golden_dir, name)
    opts = {} if rgs is None else {"row_group_size": rgs}
    out, plain = str(tmp_path / "packed.arrows"), str(tmp_path / "plain.arrows")
    keep = None
    if name == "edge_types2.arrows":   # it has columns this writer exports with no codec at all (INTERVAL, NULL, ...): the rest
        rel = con.read_arrow(src)
        keep = []
        for c in rel.columns:
            try:
                con.copy_to(con.read_arrow(src).project([c]), str(tmp_path / "probe.arrows"))
                keep.append(c)
            except da.MiError as e:
                assert e.code == _ffi.MI_ENOTSUP, (c, e)
        assert len(keep) >= 3

    def source():
        return con.read_arrow(src) if keep is None else con.read_arrow(src).project(keep)
    con.copy_to(source(), plain, **opts)
    con.copy_to(source(), out, compression="lz4", **opts)
    want = ipc.open_stream(plain).read_all()
    assert want.num_columns >= 3
    got = ipc.open_stream(out).read_all()                               # pyarrow
    assert got.schema == want.schema and tables_equal(got, want)
    if name == "seeded":
        assert got.equals(seeded[0])
    batches = record_batches(out)
    assert [c for c, _, _ in batches] == [0] * len(batches)
    canon = lambda rel: [canon_python(c) for c in rel.fetch_columns()]   # NaN-safe
    want_cols = canon(con.read_arrow(plain))
    host = con.read_arrow(out, host_decompress=True)                    # liblz4 on the reader's threads
    assert canon(host) == want_cols and host.stats()["lz4_batches_on_device"] == 0
    dev = con.read_arrow(out, host_decompress="gpu")                    # K8, where the scan defers (no list columns)
    assert canon(dev) == want_cols
    nonempty = sum(1 for b in ipc.open_stream(out) if b.num_rows)
    if name in ("lineitem_sf0_01_head.arrows", "edge_types.arrows"):
        assert dev.stats()["lz4_batches_on_device"] == nonempty > 0


def test_compression_is_declared_only_when_asked_for(con, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")
    for opts, codec in (({}, -1), ({"compression": "none"}, -1), ({"compression": "lz4"}, 0), ({"codec": "LZ4_FRAME"}, 0)):
        out = str(tmp_path / ("o_%d_%d.arrows" % (codec, len(opts))))
        con.copy_to(con.read_arrow(src), out, row_group_size=2048, **opts)
        batches = record_batches(out)
        assert len(batches) >= 2 and all(c == codec for c, _, _ in batches), opts
    with pytest.raises(da.MiError, match="ZSTD bodies are read but not written"):
        con.copy_to(con.read_arrow(src), str(tmp_path / "z.arrows"), compression="zstd")
    # to_arrow_ipc stays uncompressed
    t = da.Table(["a"], ["INTEGER"], [list(range(5000))])
    blobs = [b for b, _ in con.to_arrow_ipc(t)]
    assert ipc.open_stream(pa.BufferReader(b"".join(blobs) + b"\xff\xff\xff\xff\x00\x00\x00\x00")).read_all().num_rows == 5000
    p = str(tmp_path / "blobs.arrows")
    open(p, "wb").write(b"".join(blobs) + b"\xff\xff\xff\xff\x00\x00\x00\x00")
    assert all(c == -1 for c, _, _ in record_batches(p))


def test_random_buffers_are_stored_raw_and_empty_ones_stay_empty(con, seeded, tmp_path):
    out = str(tmp_path / "packed.arrows")
    con.copy_to(con.read_arrow(seeded[1]), out, compression="lz4", row_group_size=50000)
    n_cols_buffers = None
    for codec, spans, body in record_batches(out):
        assert codec == 0
        off, ln = spans[-1]                                              # "r": validity, offsets, data -- the last buffer
        assert struct.unpack_from("<q", body, off)[0] == -1 and ln > 8 + 24 * 40000
        off, ln = spans[0]                                               # a bitmap with 10 % NULLs is framed or raw, never empty
        assert ln > 8
        n_cols_buffers = len(spans)
    assert n_cols_buffers == 2 + 2 + 2 + 3 + 3 + 2 + 2 + 3
    # a column without rows has zero-length buffers, with no prefix
    empty = str(tmp_path / "empty.arrows")
    con.copy_to(da.Table(["l", "s"], ["INTEGER[]", "VARCHAR"], [[[], None, []], ["a", "b", "c"]]), empty, compression="lz4")
    (codec, spans, body), = record_batches(empty)
    assert codec == 0 and spans[3][1] == 0 and spans[2][1] == 0 and spans[0][1] > 0    # the list's child: validity and data
    assert ipc.open_stream(empty).read_all().to_pylist() == [{"l": [], "s": "a"}, {"l": None, "s": "b"}, {"l": [], "s": "c"}]


# ---------------------------------------------------------------------------------------- kernel == restatement
def test_kernel_equals_restatement_on_the_seeded_table(con, seeded, tmp_path):
    for rgs in (2048 * 9, 122880):
        out, plain = str(tmp_path / ("packed_%d.arrows" % rgs)), str(tmp_path / ("plain_%d.arrows" % rgs))
        con.copy_to(con.read_arrow(seeded[1]), plain, row_group_size=rgs)
        con.copy_to(con.read_arrow(seeded[1]), out, compression="lz4", row_group_size=rgs)
        assert check_file_against_restatement(out, plain) >= 19 * 2


def boundary_inputs():
    rng = np.random.default_rng(9)
    words = [b"carefully", b"final", b"deposits", b"furiously", b"quickly", b"express", b"packages", b"sleep", b"blithely", b"regular"]
    text = b" ".join(words[i] for i in rng.integers(0, 10, 30000))
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = []
    for n in (0, 1, 4, 5, 12, 13, 14, 64, 65, 65535, 65536, 65537, 3 * 65536 + 7):
        cases += [bytes(n), rnd(n), text[:n]]
        for period in (2, 3, 4, 7, 65535):
            unit = rnd(period)
            cases.append((unit * (n // period + 1))[:n])
    for m in (18, 19, 20, 273, 274, 275, 528, 529, 530):                 # all-zero blocks whose match has this length
        cases.append(bytes(64 + m + 5))
    phrase = rnd(40)
    runs = rnd(200) + phrase
    for k, run in enumerate((30, 14, 15, 269, 270)):                     # literal runs between matches
        runs += bytes([0x10 + k]) + rnd(run - 1) + phrase
    cases.append(runs + rnd(64))
    tail = bytearray(rnd(300))
    tail[290:300] = tail[20:30]                                          # a match that begins in the last 12 bytes
    cases.append(bytes(tail))
    tail = bytearray(rnd(300))
    tail[240:300] = tail[20:80]                                          # and one that runs into the last 5
    cases.append(bytes(tail))
    for phase in range(8):                                               # repeats that straddle a multiple of 64 positions
        v = bytearray(rnd(1000))
        v[567 + 3 * phase: 597 + 3 * phase] = v[100 + phase: 130 + phase]
        cases.append(bytes(v))
    v = bytearray(rnd(2 * 65536))                                        # repeats that straddle a block boundary
    v[65536 - 2000: 65536 + 2000] = text[:4000]
    v[65536 + 30000: 65536 + 34000] = text[:4000]
    v[1000:3000] = text[:2000]
    cases.append(bytes(v))
    return cases


def test_kernel_equals_restatement_on_boundary_inputs(con, tmp_path):
    """every boundary input as a binary column of one row, and as an int8 column of its length"""
    cases = boundary_inputs()
    out, plain = str(tmp_path / "packed.arrows"), str(tmp_path / "plain.arrows")
    names = ["b%d" % i for i in range(len(cases))]
    t = da.Table(names, ["BLOB"] * len(cases), [[c] for c in cases])
    con.copy_to(t, plain)
    con.copy_to(t, out, compression="lz4")
    assert check_file_against_restatement(out, plain) == 3 * len(cases)
    got = ipc.open_stream(out).read_all()
    assert [got.column(i)[0].as_py() for i in range(len(cases))] == cases
    for i, c in enumerate(cases):
        if not len(c):
            continue
        p8, o8 = str(tmp_path / ("p8_%d.arrows" % i)), str(tmp_path / ("o8_%d.arrows" % i))
        t8 = da.Table(["v"], ["TINYINT"], [np.frombuffer(c, dtype=np.int8).tolist()])
        con.copy_to(t8, p8, row_group_size=1 << 20)
        con.copy_to(t8, o8, compression="lz4", row_group_size=1 << 20)
        assert check_file_against_restatement(o8, p8) == 2, i
        assert ipc.open_stream(o8).read_all().column(0).to_numpy().astype(np.int8).tobytes() == c, i


# ---------------------------------------------------------------------------------------- determinism, pumps
def test_pumps_and_the_one_thread_sink_write_the_same_compressed_file(con, seeded, tmp_path, monkeypatch):
    t = seeded[0].drop(["l"])    # the fused pump takes flat schemas
    for chunk, rgs in ((9000, 9000), (25000, 8192), (3000, 10000), (7001, 5000), (70000, 20000)):
        src = str(tmp_path / ("src_%d.arrows" % chunk))
        with ipc.new_stream(src, t.schema) as w:
            w.write_table(t.slice(0, 70000), max_chunksize=chunk)
        outs = []
        for threads, fused in (("1", False), ("4", False), ("4", True), ("4", True)):
            monkeypatch.setenv("MI_WRITER_THREADS", threads)
            if fused:
                monkeypatch.delenv("MI_WRITER_NO_FUSED", raising=False)
            else:
                monkeypatch.setenv("MI_WRITER_NO_FUSED", "1")
            out = str(tmp_path / ("out_%d_%s_%d_%d.arrows" % (chunk, threads, fused, len(outs))))
            con.copy_to(con.read_arrow(src), out, row_group_size=rgs, compression="lz4")
            outs.append(open(out, "rb").read())
        assert outs[0] == outs[1] == outs[2] == outs[3], (chunk, rgs)
        assert all(c == 0 for c, _, _ in record_batches(out))
        assert ipc.open_stream(pa.BufferReader(outs[2])).read_all().equals(t.slice(0, 70000)), (chunk, rgs)


def test_the_compressor_compresses(con, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")
    plain, packed, ref = (str(tmp_path / n) for n in ("plain.arrows", "packed.arrows", "ref.arrows"))
    con.copy_to(con.read_arrow(src), plain)
    con.copy_to(con.read_arrow(src), packed, compression="lz4")
    t = ipc.open_stream(plain).read_all()
    with ipc.new_stream(ref, t.schema, options=ipc.IpcWriteOptions(compression="lz4")) as w:
        w.write_table(t)
    raw_size, ref_size, size = os.path.getsize(plain), os.path.getsize(ref), os.path.getsize(packed)
    print("lineitem head: uncompressed %d, this writer %d, pyarrow lz4 %d (ratio to pyarrow %.3f)" % (raw_size, size, ref_size, size / ref_size))
    assert ref_size < raw_size
    assert size < (raw_size + ref_size) / 2


# ---------------------------------------------------------------------------------------- rotation
def test_rotation_counts_compressed_bytes(con, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")
    want = ipc.open_stream(src).read_all()
    d = str(tmp_path / "per_group")
    files = con.copy_to(con.read_arrow(src), d, row_group_size=2048, row_groups_per_file=1, compression="lz4")
    assert len(files) > 2 and con.read_arrow(os.path.join(d, "*")).count() == want.num_rows
    for f in files:
        assert all(c == 0 for c, _, _ in record_batches(f))
        assert sum(1 for _ in ipc.open_stream(f)) <= 1
    plain_dir, packed_dir = str(tmp_path / "plain_size"), str(tmp_path / "packed_size")
    limit = 300000
    plain_files = con.copy_to(con.read_arrow(src), plain_dir, row_group_size=2048, file_size_bytes=limit)
    packed_files = con.copy_to(con.read_arrow(src), packed_dir, row_group_size=2048, file_size_bytes=limit, compression="lz4")
    assert 1 < len(packed_files) < len(plain_files)          # compressed bytes are what is counted
    assert con.read_arrow(os.path.join(packed_dir, "*")).count() == want.num_rows
    for f in packed_files:
        ipc.open_stream(f).read_all()
    # mi_writer_file_size == the file's size, row group by row group
    L = _ffi.lib()
    o = _ffi.WriteOptions()
    _ffi.check(L.mi_write_options_init(C.byref(o)))
    _ffi.check(L.mi_write_options_set(C.byref(o), b"row_group_size", b"2048"))
    _ffi.check(L.mi_write_options_set(C.byref(o), b"compression", b"lz4"))
    _ffi.check(L.mi_write_options_finalize(C.byref(o)))
    rel = con.read_arrow(src)
    p = str(tmp_path / "sized.arrows")
    w = C.c_void_p()
    _ffi.check(L.mi_writer_open(con.ctx._h, os.fsencode(p), da._c_fields(rel.columns, rel.types), len(rel.columns), C.byref(o), C.byref(w)))
    try:
        for ch in rel.chunks():
            _ffi.check(L.mi_writer_sink(w, C.byref(ch)))
        _ffi.check(L.mi_writer_finalize(w))
        assert L.mi_writer_file_size(w) == os.path.getsize(p) < os.path.getsize(src)
        assert L.mi_writer_row_groups(w) == sum(1 for _ in ipc.open_stream(p))
    finally:
        L.mi_writer_close(w)
    assert ipc.open_stream(p).read_all().num_rows == want.num_rows

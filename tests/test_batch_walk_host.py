"""How the host reader follows a record batch's field nodes, buffers and variadicBufferCounts (CPU only): the exact error
for each kind of table that does not match the schema, the bound on what a compressed buffer may declare, and
projections past string-view columns.  The metadata of pyarrow-written streams is patched in place: FieldNode and
Buffer are {int64, int64} structs, and a flatbuffer vector is its uint32 length followed by its elements."""
import struct

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from oracle import pyoracle as po


def stream_bytes(table, **kw):
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, table.schema, **kw) as w:
        w.write_table(table)
    return np.frombuffer(sink.getvalue(), np.uint8).copy()


def _message(buf, kind=po.MSG_RECORD_BATCH):
    m = [m for m in po.walk_stream(buf) if m["type"] == kind][0]
    return m, po.decode_record_batch(buf[m["meta_off"]: m["meta_off"] + m["meta_len"]])


def _vector(items, fmt, count=None):
    return struct.pack("<I", len(items) if count is None else count) + b"".join(struct.pack(fmt, *it) for it in items)


def _patch(buf, m, old, new):
    """`buf` with the only occurrence of `old` inside the metadata of message `m` replaced by `new`"""
    raw = buf.tobytes()
    lo, hi = m["meta_off"], m["meta_off"] + m["meta_len"]
    at = raw.find(old, lo, hi)
    assert at >= 0 and raw.find(old, at + 1, hi) < 0
    return np.frombuffer(raw[:at] + new + raw[at + len(old):], np.uint8).copy()


def _refused(buf, message, projection=None):
    rd = da.Reader(buffers=[buf])
    if projection:
        rd.set_projection(projection)
    with pytest.raises(da.MiError) as e:
        while rd.next_batch(accept_dictionaries=True) is not None:
            pass
    assert str(e.value) == message
    return e.value.code


def _two_ints():
    return pa.table({"a": pa.array(range(10), pa.int64()), "b": pa.array(range(10), pa.int64())})


def _views():
    long = ["a string longer than twelve bytes %d" % i for i in range(10)]
    return pa.table({"v": pa.array(long, pa.string_view()), "k": pa.array(range(10), pa.int32()),
                     "w": pa.array([x.encode() for x in long], pa.binary_view())})


def test_too_few_field_nodes():
    buf = stream_bytes(_two_ints())
    m, rb = _message(buf)
    buf = _patch(buf, m, _vector(rb["nodes"], "<qq"), _vector(rb["nodes"], "<qq", count=1))
    assert _refused(buf, "RecordBatch has too few field nodes") == da._ffi.MI_EINVAL


def _schema_only(schema):
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, schema):
        pass
    return sink.getvalue().to_pybytes()[:-8]   # without the end-of-stream marker


def test_more_field_nodes_than_the_schema_has():
    # the schema message of (a, b) in front of a record batch of (a, b, c)
    three = _two_ints().append_column("c", pa.array(range(10), pa.int64()))
    full = stream_bytes(three).tobytes()
    head = _schema_only(three.schema)
    assert full.startswith(head)
    buf = np.frombuffer(_schema_only(_two_ints().schema) + full[len(head):], np.uint8).copy()
    assert _refused(buf, "Expected 2 field nodes in message but found 3") == da._ffi.MI_EINVAL


def test_too_few_buffers():
    buf = stream_bytes(_two_ints())
    m, rb = _message(buf)
    buf = _patch(buf, m, _vector(rb["buffers"], "<qq"), _vector(rb["buffers"], "<qq", count=len(rb["buffers"]) - 1))
    assert _refused(buf, "RecordBatch has too few buffers") == da._ffi.MI_EINVAL


def test_too_few_variadic_buffer_counts():
    buf = stream_bytes(_views())
    m, rb = _message(buf)
    assert len(rb["variadic"]) == 2
    counts = [(c,) for c in rb["variadic"]]
    short = _patch(buf, m, _vector(counts, "<q"), _vector(counts, "<q", count=1))
    assert _refused(short, "RecordBatch has too few variadicBufferCounts") == da._ffi.MI_EINVAL
    # a projection that skips the view column with the missing count reads the whole body and reports the same
    assert _refused(short, "RecordBatch has too few variadicBufferCounts", projection=["v"]) == da._ffi.MI_EINVAL


@pytest.mark.parametrize("bad", [-1, (1 << 20) + 1])
def test_invalid_variadic_buffer_count(bad):
    buf = stream_bytes(_views())
    m, rb = _message(buf)
    counts = [(c,) for c in rb["variadic"]]
    buf = _patch(buf, m, _vector(counts, "<q"), _vector([(bad,)] + counts[1:], "<q"))
    assert _refused(buf, "Invalid variadic buffer count") == da._ffi.MI_EINVAL
    assert _refused(buf, "Invalid variadic buffer count", projection=["k"]) == da._ffi.MI_EINVAL


@pytest.mark.parametrize("cols", [["v"], ["k"], ["w"], ["w", "v"]])
def test_projection_past_string_view_columns(tmp_path, cols):
    t = _views()
    buf = stream_bytes(t)
    path = str(tmp_path / "v.arrows")
    buf.tofile(path)
    full = da.Reader(buffers=[buf]).next_batch()
    root = {n["name"]: n for n in full["nodes"] if n["depth"] == 0}
    for src in (dict(buffers=[buf]), dict(path=path)):
        rd = da.Reader(**src)
        rd.set_projection(cols)
        b = rd.next_batch()
        assert [b["nodes"][i]["spans"] for i in b["column_node"]] == [root[c]["spans"] for c in cols]
        rd = da.Reader(**src)
        rd.set_projection(cols)
        assert rd.export_stream().read_all().equals(t.select(cols))


def _compressed_table(n=1000):
    rng = np.random.default_rng(5)
    nulls = rng.random(n) < 0.1
    ints = pa.array(rng.integers(0, 1 << 40, n), pa.int64(), mask=nulls)
    strs = pa.array(["text %d" % (i % 37) for i in range(n)], mask=nulls)
    return pa.table({
        "i": ints,
        "s": strs,
        "b": pa.array(rng.random(n) < 0.5, mask=nulls),
        "l": pa.array([[int(x) for x in rng.integers(0, 9, i % 4)] for i in range(n)], pa.list_(pa.int32()), mask=nulls),
        "v": pa.array(["a string longer than twelve bytes %d" % (i % 37) for i in range(n)], pa.string_view(), mask=nulls),
        "m": pa.array([pa.MonthDayNano([i, i, i]) for i in range(n)], pa.month_day_nano_interval(), mask=nulls),
        "h": pa.array(rng.integers(-99, 99, n), pa.int16(), mask=nulls),
        "t": pa.array(rng.integers(0, 86400, n).astype(np.int32), pa.time32("s"), mask=nulls),
        "d": strs.dictionary_encode().cast(pa.dictionary(pa.int8(), pa.utf8())),
    })


def _expected_bounds(t):
    """Per RecordBatch.buffers entry: what its field node allows a compressed buffer to declare (64 bytes of slack)"""
    n = t.num_rows
    bitmap, loose = (n + 7) // 8 + 64, 1 << 40
    rows = lambda width, extra=0: (n + extra) * width + 64
    offsets = t.column("l").chunk(0).offsets
    child = offsets[-1].as_py() - offsets[0].as_py()
    return ([bitmap, rows(8)]                                  # i
            + [bitmap, rows(4, 1), (1 << 31) + 64]             # s
            + [bitmap, bitmap]                                 # b
            + [bitmap, rows(4, 1), (child + 7) // 8 + 64, child * 4 + 64]   # l and its int32 child
            + [bitmap, rows(16), loose]                        # v: validity, views, one variadic data buffer
            + [bitmap, rows(16)]                               # m
            + [bitmap, rows(2)]                                # h
            + [bitmap, rows(4)]                                # t
            + [bitmap, rows(1)])                               # d: validity, int8 indices


@pytest.mark.parametrize("codec", ["zstd", "lz4"])
def test_compressed_buffer_larger_than_its_field_node_is_refused(codec):
    t = _compressed_table()
    buf = stream_bytes(t, options=ipc.IpcWriteOptions(compression=codec))
    m, rb = _message(buf)
    bounds = _expected_bounds(t)
    assert len(bounds) == len(rb["buffers"])
    assert [i for i, (_, length) in enumerate(rb["buffers"]) if length == 0] == [9]   # the list child has no NULLs
    for i, ((off, length), bound) in enumerate(zip(rb["buffers"], bounds)):
        if length == 0:
            continue
        bad = buf.copy()
        at = m["body_off"] + off
        bad[at: at + 8] = np.array([bound + 1], np.int64).view(np.uint8)
        _refused(bad, "Compressed buffer %d declares an uncompressed length of %d bytes, more than its field node "
                      "(%d bytes at most) can hold" % (i, bound + 1, bound))
        bad[at: at + 8] = np.array([bound], np.int64).view(np.uint8)   # at the bound: past this check
        rd = da.Reader(buffers=[bad])
        with pytest.raises(da.MiError) as e:
            while rd.next_batch(accept_dictionaries=True) is not None:
                pass
        assert "more than its field node" not in str(e.value)


def test_compressed_dictionary_buffer_bound():
    t = _compressed_table()
    buf = stream_bytes(t, options=ipc.IpcWriteOptions(compression="zstd"))
    m, rb = _message(buf, po.MSG_DICTIONARY_BATCH)
    k = len(t.column("d").combine_chunks().dictionary)
    assert rb["nodes"] == [(k, 0)]
    for i, bound in [(1, (k + 1) * 4 + 64), (2, (1 << 31) + 64)]:   # the values' offsets and string data
        bad = buf.copy()
        at = m["body_off"] + rb["buffers"][i][0]
        bad[at: at + 8] = np.array([bound + 1], np.int64).view(np.uint8)
        _refused(bad, "Compressed buffer %d declares an uncompressed length of %d bytes, more than its field node "
                      "(%d bytes at most) can hold" % (i, bound + 1, bound))

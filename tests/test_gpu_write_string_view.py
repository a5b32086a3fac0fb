"""COPY ... (FORMAT ARROWS) with produce_arrow_string_view on the GPU: VARCHAR fields leave as Arrow string views (Utf8View).
The files go through pyarrow (full validation), this build's own reader (host consumer and device-resident) and a raw walk of
the record-batch metadata; with arrow_large_buffer_size and with COMPRESSION lz4; through both pumps of mi_writer_sink_scan, local
sink states and rotation.  The file written with the option off is pinned to the bytes the parent commit wrote.  Every test
but that last one fails on a build without the option."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi
from helpers import canon_python
from oracle import pyoracle as po

import test_gpu_write_compression as wc       # its readers of compressed bodies and its seeded table
from test_gpu_scan_operator import _mirror_device_vector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ["edge_types.arrows", "edge_nested.arrows", "edge_empty.arrows", "lineitem_sf0_01_head.arrows"]   # those with string columns
seeded = wc.seeded


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def leaf_types(t):
    """every type of a field tree, depth first"""
    out = [t]
    if pa.types.is_map(t):
        return out + leaf_types(t.key_type) + leaf_types(t.item_type)
    if pa.types.is_list(t) or pa.types.is_large_list(t) or pa.types.is_fixed_size_list(t):
        return out + leaf_types(t.value_type)
    if pa.types.is_struct(t):
        for i in range(t.num_fields):
            out += leaf_types(t.field(i).type)
    return out


def n_view_fields(schema):
    return sum(pa.types.is_string_view(t) for f in schema for t in leaf_types(f.type))


def check_schema(view_schema, offsets_schema):
    """VARCHAR at every depth is string_view, nothing else changed"""
    a = [t for f in view_schema for t in leaf_types(f.type)]
    b = [t for f in offsets_schema for t in leaf_types(f.type)]
    assert len(a) == len(b)
    n = 0
    for x, y in zip(a, b):
        if pa.types.is_string(y) or pa.types.is_large_string(y):
            assert pa.types.is_string_view(x), (x, y)
            n += 1
        elif not (pa.types.is_nested(x)):
            assert x == y and not pa.types.is_binary_view(x), (x, y)
    return n


def batches_meta(path):
    """[(RecordBatch metadata as the oracle decodes it, body bytes)] of a stream file: tests/helpers.py's readers"""
    a = np.fromfile(path, dtype=np.uint8)
    out = []
    for m in po.walk_stream(a):
        if m["type"] == po.MSG_RECORD_BATCH:
            out.append((po.decode_record_batch(a[m["meta_off"]: m["meta_off"] + m["meta_len"]]), a[m["body_off"]: m["body_off"] + m["body_len"]].tobytes()))
    return out


def walk_view_fields(t, arr, nodes, buffers, found):
    """One field of a record batch, depth first, in step with RecordBatch.nodes and RecordBatch.buffers (iterators); `arr` is
    pyarrow's array of it.  Every string-view field is checked: its node's length, three buffers -- bitmap, 16 bytes per row, a
    data buffer as long as its valid strings of more than 12 bytes -- and appended to `found`."""
    n, _ = next(nodes)
    assert n == len(arr), (t, n, len(arr))
    take = lambda k: [next(buffers)[1] for _ in range(k)]
    if pa.types.is_string_view(t):
        long_bytes = sum(len(v.encode()) for v in arr.to_pylist() if v is not None and len(v.encode()) > 12)
        assert take(3) == [(n + 7) // 8, 16 * n, long_bytes], t
        found.append(n)
    elif pa.types.is_struct(t):
        take(1)
        for i in range(t.num_fields):
            walk_view_fields(t.field(i).type, arr.field(i), nodes, buffers, found)
    elif pa.types.is_map(t):
        take(2)
        next(nodes)                                     # the entries struct
        take(1)
        walk_view_fields(t.key_type, arr.keys, nodes, buffers, found)
        walk_view_fields(t.item_type, arr.items, nodes, buffers, found)
    elif pa.types.is_list(t) or pa.types.is_large_list(t):
        take(2)
        walk_view_fields(t.value_type, arr.values, nodes, buffers, found)
    elif pa.types.is_fixed_size_list(t):
        take(1)
        walk_view_fields(t.value_type, arr.values, nodes, buffers, found)
    elif pa.types.is_binary(t) or pa.types.is_large_binary(t) or pa.types.is_string(t) or pa.types.is_large_string(t):
        take(3)
    elif not pa.types.is_null(t):
        take(2)


def device_columns(con, path, columns=None):
    """the columns as a device-resident scan hands them out, copied back through their device pointers"""
    hip = C.CDLL("libamdhip64.so")
    rel = con.read_arrow(path, device_resident=True)
    if columns is not None:
        rel = rel.project(columns)
    types = [da.parse_duck_type(t) for t in rel.types]
    got = [[] for _ in types]
    for ch in rel.chunks():
        keep = []
        for ci, ty in enumerate(types):
            got[ci].extend(da._vector_values(_mirror_device_vector(hip, ch.columns[ci], ty, ch.size, keep), ty, ch.size))
    return [canon_python(c) for c in got]


def same(a, b):
    """Python values of two readings, NaN equal to NaN"""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b


def values_equal(a, b):
    return a.num_rows == b.num_rows and a.num_columns == b.num_columns and all(same(x.to_pylist(), y.to_pylist()) for x, y in zip(a.columns, b.columns))


# ---------------------------------------------------------------------------------------- three readers
@pytest.mark.parametrize("rgs", [2048, 5000, None])
@pytest.mark.parametrize("name", GOLDEN + ["seeded"])
def test_three_readers(con, golden_dir, seeded, tmp_path, name, rgs):
    src = seeded[1] if name == "seeded" else os.path.join(golden_dir, name)
    opts = {} if rgs is None else {"row_group_size": rgs}
    source = lambda: con.read_arrow(src)
    out, plain = str(tmp_path / "views.arrows"), str(tmp_path / "offsets.arrows")
    con.copy_to(source(), plain, **opts)
    con.copy_to(source(), out, produce_arrow_string_view=True, **opts)
    want = ipc.open_stream(plain).read_all()
    reader = ipc.open_stream(out)
    n_views = check_schema(reader.schema, want.schema)
    assert n_views == n_view_fields(reader.schema) >= 1
    batches = list(reader)
    for b in batches:
        b.validate(full=True)
    got = pa.Table.from_batches(batches, reader.schema)
    assert [b.num_rows for b in batches] == [b.num_rows for b in ipc.open_stream(plain)]
    assert values_equal(got, want)
    # the raw walk: three buffers per view field -- bitmap, 16 * n, the long bytes --, one variadic data buffer each
    metas = batches_meta(out)
    assert len(metas) == sum(1 for b in batches if b.num_rows)
    for (rb, _), b in zip(metas, [b for b in batches if b.num_rows]):
        assert rb["variadic"] == [1] * n_views
        nodes, buffers, found = iter(rb["nodes"]), iter(rb["buffers"]), []
        for i, f in enumerate(b.schema):
            walk_view_fields(f.type, b.column(i), nodes, buffers, found)
        assert len(found) == n_views and next(nodes, None) is None and next(buffers, None) is None
    assert sum(len(rb["buffers"]) for rb, _ in batches_meta(out)) == sum(len(rb["buffers"]) for rb, _ in batches_meta(plain))
    assert all(rb["variadic"] == [] for rb, _ in batches_meta(plain))
    # this build's own reader
    canon = lambda rel: [canon_python(c) for c in rel.fetch_columns()]
    want_cols = canon(con.read_arrow(plain))
    assert canon(con.read_arrow(out)) == want_cols
    # ... device-resident (the seeded table's 150 000 long strings would come back one hipMemcpy each: its short columns)
    cols = ["k", "s", "dt"] if name == "seeded" else None
    assert device_columns(con, out, cols) == device_columns(con, plain, cols) == (want_cols if cols is None else want_cols[:1] + want_cols[3:4] + want_cols[2:3])


def test_a_batch_without_long_strings_has_an_empty_data_buffer(con, tmp_path):
    out = str(tmp_path / "short.arrows")
    t = da.Table(["s", "i", "t"], ["VARCHAR", "INTEGER", "VARCHAR"],
                 [["a", None, "twelve bytes", ""] * 1000, list(range(4000)), [None if i % 3 else "thirteen bytes %d" % i for i in range(4000)]])
    con.copy_to(t, out, produce_arrow_string_view=True, row_group_size=2048)
    metas = batches_meta(out)
    assert len(metas) == 2
    for rb, body in metas:
        n = rb["length"]
        assert rb["variadic"] == [1, 1] and len(rb["buffers"]) == 3 + 2 + 3
        assert [l for _, l in rb["buffers"][:3]] == [(n + 7) // 8, 16 * n, 0]                   # "s": bitmap, views, an empty data buffer
        long_ = sum(len("thirteen bytes %d" % i) for i in range(4000) if i % 3 == 0 and (i < 2048) == (rb is metas[0][0]))
        assert [l for _, l in rb["buffers"][5:]] == [(n + 7) // 8, 16 * n, long_]
        off = rb["buffers"][6][0]
        views = np.frombuffer(body[off: off + 16 * n], dtype=np.uint8).reshape(n, 16)
        nulls = np.array([(i + (0 if rb is metas[0][0] else 2048)) % 3 != 0 for i in range(n)])
        assert not views[nulls].any()                                                             # NULL: 16 zero bytes
    got = ipc.open_stream(out).read_all()
    got.validate(full=True)
    assert got.column("s").to_pylist() == ["a", None, "twelve bytes", ""] * 1000


def test_with_large_buffers_only_blob_and_list_follow(con, tmp_path):
    out = str(tmp_path / "large.arrows")
    t = da.Table(["s", "b", "l", "m"], ["VARCHAR", "BLOB", "VARCHAR[]", "MAP(VARCHAR, VARCHAR)"],
                 [["short", None, "a string of more than twelve bytes"], [b"\x00\x01", b"x" * 40, None],
                  [["in a list", "a list entry of more than twelve bytes"], None, []],
                  [[("key", "value of more than twelve bytes")], [], None]])
    con.copy_to(t, out, produce_arrow_string_view=True, arrow_large_buffer_size=True)
    got = ipc.open_stream(out).read_all()
    got.validate(full=True)
    assert got.schema.field("s").type == pa.string_view() and got.schema.field("b").type == pa.large_binary()
    assert got.schema.field("l").type == pa.large_list(pa.field("l", pa.string_view()))
    m = got.schema.field("m").type
    assert pa.types.is_map(m) and m.key_type == pa.string_view() and m.item_type == pa.string_view()
    assert got.column("s").to_pylist() == ["short", None, "a string of more than twelve bytes"]
    assert got.column("l").to_pylist() == [["in a list", "a list entry of more than twelve bytes"], None, []]
    assert got.column("m").to_pylist() == [[("key", "value of more than twelve bytes")], [], None]
    (rb, _), = batches_meta(out)
    assert rb["variadic"] == [1, 1, 1, 1]


# ---------------------------------------------------------------------------------------- LZ4
@pytest.mark.parametrize("name", ["lineitem_sf0_01_head.arrows", "seeded"])
def test_lz4_bodies_of_view_files(con, golden_dir, seeded, tmp_path, name):
    src = seeded[1] if name == "seeded" else os.path.join(golden_dir, name)
    plain, packed = str(tmp_path / "plain.arrows"), str(tmp_path / "packed.arrows")
    con.copy_to(con.read_arrow(src), plain, produce_arrow_string_view=True, row_group_size=20000)
    con.copy_to(con.read_arrow(src), packed, produce_arrow_string_view=True, row_group_size=20000, compression="lz4")
    assert wc.check_file_against_restatement(packed, plain) > 0
    assert [rb["variadic"] for rb, _ in batches_meta(packed)] == [rb["variadic"] for rb, _ in batches_meta(plain)]
    want = ipc.open_stream(plain).read_all()
    got = ipc.open_stream(packed).read_all()
    got.validate(full=True)
    assert got.schema == want.schema and n_view_fields(got.schema) >= 2 and got.equals(want)
    canon = lambda rel: [canon_python(c) for c in rel.fetch_columns()]
    want_cols = canon(con.read_arrow(plain))
    host = con.read_arrow(packed, host_decompress=True)
    assert canon(host) == want_cols and host.stats()["lz4_batches_on_device"] == 0
    assert canon(con.read_arrow(packed, host_decompress="gpu")) == want_cols


# ---------------------------------------------------------------------------------------- pumps, local states, rotation
_CHILD = """
import sys
import duckdb_arrow_amd as da
con = da.Connection(0)
con.copy_to(con.read_arrow(sys.argv[1]), sys.argv[2], row_group_size=int(sys.argv[3]), produce_arrow_string_view=True)
"""


def test_both_pumps_and_the_one_thread_sink_write_the_same_file(con, seeded, tmp_path, monkeypatch):
    """record batches larger than, equal to and no multiple of the row group; the sink-thread pump runs in a fresh child process
    with MI_WRITER_NO_FUSED set"""
    t = seeded[0].drop(["l"]).slice(0, 70000)    # the fused pump takes flat schemas
    monkeypatch.delenv("MI_WRITER_NO_FUSED", raising=False)
    for chunk, rgs in ((25000, 8192), (8192, 8192), (7001, 5000)):
        src = str(tmp_path / ("src_%d.arrows" % chunk))
        with ipc.new_stream(src, t.schema) as w:
            w.write_table(t, max_chunksize=chunk)
        # the one-thread sink: chunk by chunk through mi_writer_sink (a rotating copy_to with a limit it never reaches)
        one = con.copy_to(con.read_arrow(src), str(tmp_path / ("one_%d" % chunk)), row_group_size=rgs, produce_arrow_string_view=True, file_size_bytes=1 << 40)
        assert len(one) == 1
        want = open(one[0], "rb").read()
        monkeypatch.setenv("MI_WRITER_THREADS", "4")
        fused = str(tmp_path / ("fused_%d.arrows" % chunk))
        groups0, views0 = da.writer_fused_counts()
        con.copy_to(con.read_arrow(src), fused, row_group_size=rgs, produce_arrow_string_view=True)
        groups1, views1 = da.writer_fused_counts()
        # the fused pump took row groups where they lay in HBM, both string columns as view tasks (rows that straddle two record
        # batches take its host path: not every row group when the batch is no multiple of the row group)
        assert groups1 > groups0 and views1 - views0 == 2 * (groups1 - groups0), (chunk, rgs)
        if chunk == rgs:
            assert groups1 - groups0 == 70000 // rgs
        threads = str(tmp_path / ("threads_%d.arrows" % chunk))
        env = dict(os.environ, MI_WRITER_NO_FUSED="1", MI_WRITER_THREADS="4", PYTHONPATH=os.pathsep.join([ROOT] + sys.path))
        run = subprocess.run([sys.executable, "-c", _CHILD, src, threads, str(rgs)], env=env, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        assert open(fused, "rb").read() == want and open(threads, "rb").read() == want, (chunk, rgs)
        got = ipc.open_stream(fused).read_all()
        got.validate(full=True)
        assert n_view_fields(got.schema) == 2 and values_equal(got, t), (chunk, rgs)


@pytest.mark.parametrize("rows", [8192, 4096, 6000, 3000])
def test_two_local_states_write_the_one_thread_sink_s_row_groups(con, tmp_path, rows):
    """Two mi_writer_local states, one after the other, with more rows than a row group (a multiple of it and not), as many and
    fewer: a state flushes its tail when it is combined, so the file is the schema, then the record-batch messages the
    one-thread sink writes for the first state's rows alone, then those for the second's, byte for byte."""
    L = _ffi.lib()
    names, types = ["t", "s"], ["INTEGER", "VARCHAR"]
    o = _ffi.WriteOptions()
    _ffi.check(L.mi_write_options_init(C.byref(o)))
    _ffi.check(L.mi_write_options_set(C.byref(o), b"row_group_size", b"4096"))
    o.produce_arrow_string_view = 1
    _ffi.check(L.mi_write_options_finalize(C.byref(o)))
    text = lambda tid, i: None if i % 11 == 0 else ("t%d" % tid if i % 2 else "state %d row %d, more than twelve bytes" % (tid, i))
    tabs = [da.Table(names, types, [[tid] * rows, [text(tid, i) for i in range(rows)]]) for tid in range(2)]

    def write(path, groups):
        """groups: lists of tables; every group goes through a sink state of its own (None: the writer's one-thread sink)"""
        w = C.c_void_p()
        _ffi.check(L.mi_writer_open(con.ctx._h, path.encode(), da._c_fields(names, types), 2, C.byref(o), C.byref(w)))
        keep = []
        for local, tables in groups:
            loc = C.c_void_p()
            if local:
                _ffi.check(L.mi_writer_local_create(w, C.byref(loc)))
            for tab in tables:
                for ch in da._chunks_from_table(tab, keep):
                    _ffi.check(L.mi_writer_local_sink(loc, C.byref(ch)) if local else L.mi_writer_sink(w, C.byref(ch)))
            if local:
                _ffi.check(L.mi_writer_local_combine(loc))
                L.mi_writer_local_destroy(loc)
        _ffi.check(L.mi_writer_finalize(w))
        L.mi_writer_close(w)
        return open(path, "rb").read()

    both = write(str(tmp_path / "local.arrows"), [(True, [tabs[0]]), (True, [tabs[1]])])
    alone = [write(str(tmp_path / ("one_%d.arrows" % k)), [(False, [tabs[k]])]) for k in range(2)]
    first = po.walk_stream(np.frombuffer(alone[1], dtype=np.uint8))[0]
    schema_end = first["body_off"] + first["body_len"]
    assert first["type"] != po.MSG_RECORD_BATCH and alone[0][:schema_end] == alone[1][:schema_end]
    assert both == alone[0][:-8] + alone[1][schema_end:]
    got = ipc.open_stream(pa.BufferReader(both)).read_all()
    got.validate(full=True)
    assert got.schema.field("s").type == pa.string_view()
    assert got.column("s").to_pylist() == [text(tid, i) for tid in range(2) for i in range(rows)]
    metas = batches_meta(str(tmp_path / "local.arrows"))
    assert [rb["length"] for rb, _ in metas] == 2 * ([4096] * (rows // 4096) + ([rows % 4096] if rows % 4096 else []))
    assert all(rb["variadic"] == [1] for rb, _ in metas)


def test_rotation_cuts_where_the_file_sizes_say(con, golden_dir, tmp_path):
    src = os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")
    want = ipc.open_stream(src).read_all()
    limit = 300000
    files = con.copy_to(con.read_arrow(src), str(tmp_path / "rot"), row_group_size=2048, file_size_bytes=limit, produce_arrow_string_view=True)
    assert len(files) > 2
    rows = 0
    for f in files:
        t = ipc.open_stream(f).read_all()
        t.validate(full=True)
        assert n_view_fields(t.schema) >= 2
        rows += t.num_rows
        # a file is closed by the first row group that takes it past the limit: without its last record batch it is under it
        ends = [m["body_off"] + m["body_len"] for m in po.walk_stream(np.fromfile(f, dtype=np.uint8)) if m["type"] == po.MSG_RECORD_BATCH]
        if f is not files[-1]:
            assert os.path.getsize(f) > limit and (len(ends) < 2 or ends[-2] <= limit)
        else:
            assert len(ends) < 2 or ends[-2] <= limit
    assert rows == want.num_rows


# ---------------------------------------------------------------------------------------- the default
def test_the_default_file_is_the_parent_commit_s(con, golden_dir, tmp_path):
    """option off: the bytes of the file are those the commit before the option wrote (tests/golden/copy_default_sha256.json)"""
    pinned = json.load(open(os.path.join(golden_dir, "copy_default_sha256.json")))
    src = os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")
    for key, opts in (("default", {}), ("row_group_size_2048", {"row_group_size": 2048}), ("lz4", {"compression": "lz4"})):
        out = str(tmp_path / (key + ".arrows"))
        con.copy_to(con.read_arrow(src), out, **opts)
        assert hashlib.sha256(open(out, "rb").read()).hexdigest() == pinned[key], key
        other = str(tmp_path / (key + "_off.arrows"))
        con.copy_to(con.read_arrow(src), other, produce_arrow_string_view=False, **opts)
        assert open(other, "rb").read() == open(out, "rb").read()

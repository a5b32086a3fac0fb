"""K8: LZ4_FRAME bodies decompressed in HBM (kernels_lz4.hip).  The reference decompresses on the CPU before slicing the
body (base_stream_reader.cpp:11-50, zstd only; LZ4_FRAME is what pyarrow / Feather V2 write by default).  The check at this
boundary: a device-resident scan of an LZ4 stream -- compressed bytes over PCIe, the four K8 kernels, then the usual
transcode kernels -- yields the vectors of the host-consumer scan of the same file, whose bodies the host reader
decompresses with liblz4; and mi_scan_get_stats shows the GPU path was the one that ran."""
import ctypes as C
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from helpers import canon_python, pyarrow_columns, rewrite_buffers_raw
from test_gpu_scan_operator import _mirror_device_vector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


def _device_scan(con, path, **kw):
    hip = C.CDLL("libamdhip64.so")
    rel = con.read_arrow(path, accept_dictionaries=True, device_resident=True, **kw)
    types = [da.parse_duck_type(t) for t in rel.types]
    got = [[] for _ in types]
    for ch in rel.chunks():
        keep = []
        for ci, ty in enumerate(types):
            hv = _mirror_device_vector(hip, ch.columns[ci], ty, ch.size, keep)
            got[ci].extend(da._vector_values(hv, ty, ch.size))
    st = rel.stats()
    rel.close()
    return [canon_python(c) for c in got], st


def _write(path, table, chunk, codec="lz4"):
    with ipc.new_stream(path, table.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        w.write_table(table, max_chunksize=chunk)


def _tables():
    rng = np.random.default_rng(77)
    n = 300000
    words = ["alpha", "beta", "gamma delta epsilon", "", "zeta " * 9, "x"]
    yield "mixed", pa.table({
        "k": pa.array(np.arange(n, dtype=np.int64) * 3),                                   # matches at a fixed short distance
        "z": pa.array(np.zeros(n, np.int32)),                                              # one long overlapping run
        "r": pa.array(rng.integers(0, 1 << 62, n, dtype=np.int64)),                        # incompressible: stored raw
        "s": pa.array([words[i] for i in rng.integers(0, len(words), n)], mask=rng.random(n) < 0.05),
        "d": pa.array(rng.integers(8000, 11000, n).astype(np.int32), pa.date32()),
        "b": pa.array(rng.random(n) < 0.3, mask=rng.random(n) < 0.1),
        "t": pa.array(["comment %d %s" % (i % 977, "lorem ipsum dolor sit amet"[: i % 27]) for i in range(n)]),
    }), 131072
    yield "small_batches", pa.table({"a": pa.array(rng.integers(0, 5, 5000, dtype=np.int64)), "s": pa.array(["v%d" % (i % 7) for i in range(5000)])}), 700
    yield "empty", pa.table({"a": pa.array([], pa.int64()), "s": pa.array([], pa.string())}), 10
    period = np.tile(np.arange(97, dtype=np.uint8), 40000)                                # chains through many earlier matches
    yield "periodic", pa.table({"p": pa.array(period[:3000000].view(np.int32)[:700000])}), 700000


@pytest.mark.parametrize("case", ["mixed", "small_batches", "empty", "periodic"])
def test_lz4_bodies_decompressed_in_hbm_equal_the_host_decompressor(con, tmp_path, case):
    name, table, chunk = next(t for t in _tables() if t[0] == case)
    path = str(tmp_path / (name + ".arrows"))
    _write(path, table, chunk)
    want = [canon_python(c) for c in con.read_arrow(path, accept_dictionaries=True, host_decompress=True).fetch_columns()]   # liblz4 on host threads
    got, st = _device_scan(con, path)
    assert got == want
    assert got == pyarrow_columns(table)      # and both equal pyarrow's reading of the table that was written
    # a host consumer can take the K8 path too (host_decompress = -1): vectors and the string payloads (a pinned mirror of the
    # body) come back; by default its bodies are decompressed by the reader's host threads
    assert con.read_arrow(path, accept_dictionaries=True).count(detail=True)["rows"] == table.num_rows
    rel = con.read_arrow(path, accept_dictionaries=True, host_decompress="gpu")
    assert [canon_python(c) for c in rel.fetch_columns()] == want
    assert (rel.stats()["lz4_batches_on_device"] > 0) == (st["lz4_batches_on_device"] > 0)
    batches = len(list(ipc.open_stream(path)))
    nonempty = sum(1 for b in ipc.open_stream(path) if b.num_rows > 0)
    assert st["record_batches"] == batches
    assert st["lz4_batches_on_device"] >= (nonempty if table.num_columns else 0), st
    if nonempty:
        assert 0 < st["h2d_bytes"] and st["decompressed_bytes"] > 0
    got_host, st_host = _device_scan(con, path, host_decompress=True)                                   # same consumer, host decompression
    assert got_host == want and st_host["lz4_batches_on_device"] == 0


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_raw_buffers_inside_compressed_bodies(con, tmp_path, codec):
    """Buffers stored raw inside a compressed body (length prefix -1; Arrow C++ with min_space_savings, arrow-rs and Arrow
    Java write them for incompressible data, nanoarrow copies them so the reference reads such files): on the K8 path they
    are copied into place beside the buffers the kernels expand.  Every second buffer raw; all buffers raw; none."""
    name, table, chunk = next(t for t in _tables() if t[0] == "mixed")
    table = table.slice(0, 150000)
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, table.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        w.write_table(table, max_chunksize=60000)
    packed = sink.getvalue().to_pybytes()
    want = pyarrow_columns(table)
    gpu = {} if codec == "lz4" else {"host_decompress": "gpu"}
    for tag, pick in (("alternate", lambda bi, k, ln: k % 2 == 1), ("all", lambda bi, k, ln: True), ("first_batch", lambda bi, k, ln: bi == 0)):
        path = str(tmp_path / ("raw_%s_%s.arrows" % (codec, tag)))
        raw = rewrite_buffers_raw(packed, pick)
        assert ipc.open_stream(pa.py_buffer(raw)).read_all().equals(table)
        open(path, "wb").write(raw)
        got, st = _device_scan(con, path, **gpu)
        assert got == want, tag
        assert st["lz4_batches_on_device" if codec == "lz4" else "zstd_batches_on_device"] == 3, (tag, st)
        assert [canon_python(c) for c in con.read_arrow(path, host_decompress=True).fetch_columns()] == want, tag
        assert [canon_python(c) for c in con.read_arrow(path, host_decompress="gpu").fetch_columns()] == want, tag


def test_lz4_golden_files_and_projection(con, golden_dir, tmp_path):
    for rel_path in ("lineitem_sf0_01_head.arrows", "edge_types.arrows", "edge_nested.arrows", "edge_dict.arrows"):
        t = ipc.open_stream(os.path.join(golden_dir, rel_path)).read_all()
        path = str(tmp_path / ("lz4_" + rel_path))
        _write(path, t, 4096)
        want = [canon_python(c) for c in con.read_arrow(path, accept_dictionaries=True, host_decompress=True).fetch_columns()]
        got, st = _device_scan(con, path)
        assert got == want, rel_path
        if rel_path == "lineitem_sf0_01_head.arrows":
            assert got == pyarrow_columns(t)
        assert [canon_python(c) for c in con.read_arrow(path, accept_dictionaries=True, host_decompress="gpu").fetch_columns()] == want, rel_path
        # list / map columns keep the host decompressor: the planner samples their offsets on the host
        assert (st["lz4_batches_on_device"] > 0) == (rel_path != "edge_nested.arrows"), rel_path
    # projection: only the projected columns' frames cross PCIe
    t = ipc.open_stream(os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")).read_all()
    path = str(tmp_path / "lz4_proj.arrows")
    _write(path, t, 4096)
    hip = C.CDLL("libamdhip64.so")
    rel = con.read_arrow(path, device_resident=True).project(["l_shipdate", "l_comment"])
    want = con.read_arrow(path, host_decompress=True).project(["l_shipdate", "l_comment"]).fetch_columns()
    types = [da.parse_duck_type(x) for x in rel.types]
    got = [[] for _ in types]
    for ch in rel.chunks():
        keep = []
        for ci, ty in enumerate(types):
            got[ci].extend(da._vector_values(_mirror_device_vector(hip, ch.columns[ci], ty, ch.size, keep), ty, ch.size))
    assert [canon_python(c) for c in got] == [canon_python(c) for c in want]
    full = os.path.getsize(path)
    assert 0 < rel.stats()["h2d_bytes"] < full * 0.6


def test_lz4_fused_consumers_on_compressed_input(con, golden_dir, tmp_path):
    """Count with a pushed-down filter and the fused Q6 aggregate read LZ4 input without the body ever being decompressed
    on the host."""
    t = ipc.open_stream(os.path.join(golden_dir, "lineitem_sf0_01_q6.arrows")).read_all()
    path = str(tmp_path / "q6_lz4.arrows")
    _write(path, t, 8192)
    plain = os.path.join(golden_dir, "lineitem_sf0_01_q6.arrows")
    rel = con.read_arrow(path, device_resident=True)
    rel.filter_range("l_shipdate", 8766, 9130)
    a = rel.count(detail=True)
    assert rel.stats()["lz4_batches_on_device"] > 0
    rel2 = con.read_arrow(plain)
    rel2.filter_range("l_shipdate", 8766, 9130)
    b = rel2.count(detail=True)
    assert (a["rows"], a["selected"]) == (b["rows"], b["selected"])
    s1 = con.read_arrow(path, device_resident=True).sum_product("l_extendedprice", "l_discount", [("l_shipdate", 8766, 9130)])
    s2 = con.read_arrow(plain).sum_product("l_extendedprice", "l_discount", [("l_shipdate", 8766, 9130)])
    assert s1 == s2


def _frames(buf):
    """(offset, length) of every compressed buffer's LZ4 frame in an IPC stream written by pyarrow (walks the messages)."""
    out = []
    for e in da.Reader(buffers=[np.frombuffer(buf, np.uint8)]).index():
        if e["type"] == 3:
            out.append((e["body_offset"], e["body_len"]))
    return out


def test_damaged_lz4_input_is_an_error_not_a_crash(con, tmp_path):
    """Corrupt block data (a match offset that reaches in front of the buffer, a token chain that runs past the block, a wrong
    declared length): the K8 kernels bound every read and write, the scan ends with the EIO of base_stream_reader.cpp:24-29."""
    n = 200000
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64) % 1000), "s": pa.array(["row %d" % (i % 313) for i in range(n)])})
    path = str(tmp_path / "ok.arrows")
    _write(path, t, n)
    good = bytearray(open(path, "rb").read())
    (body_off, body_len), = _frames(bytes(good))
    rng = np.random.default_rng(3)
    outcomes = set()
    for trial in range(int(os.environ.get("MI_LZ4_FUZZ_TRIALS", "24"))):
        bad = bytearray(good)
        if trial == 0:   # the declared uncompressed length of the first buffer that has one
            for at in range(body_off, body_off + body_len - 8, 8):
                v = struct.unpack_from("<q", bad, at)[0]
                if 0 < v < (1 << 31) and bad[at + 8: at + 12] == b"\x04\x22\x4d\x18":
                    struct.pack_into("<q", bad, at, v - 8)
                    break
        else:            # random bytes inside the block data
            for _ in range(1 + trial % 5):
                at = body_off + 64 + int(rng.integers(0, body_len - 128))
                bad[at] = int(rng.integers(0, 256))
        p = str(tmp_path / ("bad_%d.arrows" % trial))
        open(p, "wb").write(bytes(bad))
        try:
            got, st = _device_scan(con, p)
            outcomes.add("ok")          # the damage hit literal bytes or padding: wrong values, valid structure
        except da.MiError as e:
            outcomes.add("error")
            assert e.code in (da._ffi.MI_EIO, da._ffi.MI_EINVAL), (trial, str(e))
    assert "error" in outcomes
    # the context still works
    got, _ = _device_scan(con, path)
    assert got == [canon_python(c) for c in con.read_arrow(path, host_decompress=True).fetch_columns()]


def test_lz4_file_list_sharded_filtered_and_compacted(con, golden_dir, tmp_path):
    """K8 under the rest of the operator: a list of LZ4 files, record batches dealt to two ranks, a pushed-down predicate
    with late materialisation (the gather kernels read the body the K8 kernels produced) -- equal to the same scan of the
    uncompressed files."""
    t = ipc.open_stream(os.path.join(golden_dir, "lineitem_sf0_01_head.arrows")).read_all()
    packed, plain = [], []
    third = t.num_rows // 3
    for i in range(3):
        part = t.slice(i * third, third if i < 2 else t.num_rows - 2 * third)
        p1, p2 = str(tmp_path / ("part%d_lz4.arrows" % i)), str(tmp_path / ("part%d.arrows" % i))
        _write(p1, part, 3000)
        with ipc.new_stream(p2, part.schema) as w:
            w.write_table(part, max_chunksize=3000)
        packed.append(p1)
        plain.append(p2)
    hip = C.CDLL("libamdhip64.so")

    def scan(paths, **kw):
        rel = con.read_arrow(paths, device_resident=True, filter_compact=True, **kw).project(["l_orderkey", "l_shipdate", "l_comment", "l_quantity"])
        rel.filter_range("l_shipdate", 8766, 9130)
        types = [da.parse_duck_type(x) for x in rel.types]
        got = [[] for _ in types]
        for ch in rel.chunks():
            keep = []
            for ci, ty in enumerate(types):
                got[ci].extend(da._vector_values(_mirror_device_vector(hip, ch.columns[ci], ty, ch.size, keep), ty, ch.size))
        st = rel.stats()
        rel.close()
        return [canon_python(c) for c in got], st

    want, _ = scan(plain)
    assert len(want[0]) > 0
    got, st = scan(packed)
    assert got == want and st["lz4_batches_on_device"] == st["record_batches"] > 3
    halves = [scan(packed, rank=r, world=2) for r in (0, 1)]
    assert sorted(halves[0][0][0] + halves[1][0][0]) == sorted(want[0])
    assert halves[0][1]["record_batches"] + halves[1][1]["record_batches"] == st["record_batches"]


def test_lz4_in_a_multi_device_scan(con, golden_dir, tmp_path):
    """mi_scan_open_files_multi over LZ4 files: every sub-scan ships and decompresses its own record batches (stats are summed
    over the devices); counts, the filter and the fused aggregate equal the single-context scan of the uncompressed file."""
    t = ipc.open_stream(os.path.join(golden_dir, "lineitem_sf0_01_q6.arrows")).read_all()
    paths = []
    half = t.num_rows // 2
    for i, part in enumerate((t.slice(0, half), t.slice(half))):
        p = str(tmp_path / ("q6_%d_lz4.arrows" % i))
        _write(p, part, 4096)
        paths.append(p)
    plain = os.path.join(golden_dir, "lineitem_sf0_01_q6.arrows")
    ref = con.read_arrow(plain)
    ref.filter_range("l_shipdate", 8766, 9130)
    want = ref.count(detail=True)
    rel = con.read_arrow(paths, contexts=[da.Context(0), da.Context(0), da.Context(0)], device_resident=True)
    rel.filter_range("l_shipdate", 8766, 9130)
    got = rel.count(detail=True)
    st = rel.stats()
    assert (got["rows"], got["selected"]) == (want["rows"], want["selected"])
    assert st["lz4_batches_on_device"] == st["record_batches"] == sum(len(list(ipc.open_stream(p))) for p in paths)
    s1 = con.read_arrow(paths, contexts=[da.Context(0), da.Context(0)], device_resident=True).sum_product(
        "l_extendedprice", "l_discount", [("l_shipdate", 8766, 9130)])
    s2 = con.read_arrow(plain).sum_product("l_extendedprice", "l_discount", [("l_shipdate", 8766, 9130)])
    assert s1 == s2


@pytest.mark.parametrize("variant", ["default", "MI_LZ4_PARSE_SPECULATIVE", "MI_LZ4_PARSE_GLOBAL"])
def test_lz4_parse_kernel_variants(tmp_path, variant):
    """The token walk has three kernels: lz4_parse_dp (exit tables, blocks of <= 50 KiB compressed bytes: the default), the
    speculative walk from an LDS copy (larger blocks; forced for every block by MI_LZ4_PARSE_SPECULATIVE) and the same from
    global memory (blocks too large for LDS, 4 MiB block frames; forced by MI_LZ4_PARSE_GLOBAL).  Column `h` (5 random bytes
    of every 8) compresses to > 50 KiB per 64 KiB block, so the default run uses two of them in one launch set."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        sys.path.insert(0, os.path.join(%r, "tests"))
        import numpy as np, pyarrow as pa, pyarrow.ipc as ipc
        import duckdb_arrow_amd as da
        rng = np.random.default_rng(5)
        n = 150000
        t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64) * 5), "s": pa.array(["text %%d %%s" %% (i %% 701, "z" * (i %% 23)) for i in range(n)]),
                      "q": pa.array(rng.integers(0, 50, n).astype(np.int32)),
                      "h": pa.array(rng.integers(0, 1 << 40, n, dtype=np.int64))})
        p = %r
        with ipc.new_stream(p, t.schema, options=ipc.IpcWriteOptions(compression="lz4")) as w:
            w.write_table(t, max_chunksize=60000)
        con = da.Connection(0)
        want = con.read_arrow(p, host_decompress=True).fetch_columns()
        rel = con.read_arrow(p, host_decompress="gpu")
        got = rel.fetch_columns()
        assert got == want and rel.stats()["lz4_batches_on_device"] == 3
        from helpers import pyarrow_columns, canon_python
        assert [canon_python(c) for c in got] == pyarrow_columns(t)
        print("ok")
    """) % (ROOT, ROOT, str(tmp_path / "g.arrows"))
    env = dict(os.environ) if variant == "default" else dict(os.environ, **{variant: "1"})
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_lz4_one_stream_per_slot_with_hardware_queues_to_spare(tmp_path):
    """With GPU_MAX_HW_QUEUES >= slots + 3 in the process environment the K8 kernels of every slot run on a stream of their
    own (scan_enqueue.cpp ChooseLz4Stream) instead of three shared ones: many small record batches in flight, the same vectors."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        import numpy as np, pyarrow as pa, pyarrow.ipc as ipc
        import duckdb_arrow_amd as da
        rng = np.random.default_rng(9)
        n = 200000
        t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64) * 3), "s": pa.array(["row %%d %%s" %% (i %% 977, "y" * (i %% 19)) for i in range(n)]),
                      "q": pa.array(rng.integers(0, 50, n).astype(np.int32)), "d": pa.array(rng.integers(8000, 10500, n).astype(np.int32), pa.date32())})
        p = %r
        with ipc.new_stream(p, t.schema, options=ipc.IpcWriteOptions(compression="lz4")) as w:
            w.write_table(t, max_chunksize=10000)       # 20 record batches over 8 or 12 slots
        con = da.Connection(0)
        want = con.read_arrow(p, host_decompress=True).fetch_columns()
        for depth in (8, 12):
            rel = con.read_arrow(p, host_decompress="gpu", pipeline_depth=depth)
            got = rel.fetch_columns()
            assert got == want and rel.stats()["lz4_batches_on_device"] == 20
            rel = con.read_arrow(p, device_resident=True, pipeline_depth=depth)
            assert rel.count(detail=True)["rows"] == n and rel.stats()["lz4_batches_on_device"] == 20
        print("ok")
    """) % (ROOT, str(tmp_path / "q.arrows"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, GPU_MAX_HW_QUEUES="20"), timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_host_consumer_of_a_body_expanded_in_hbm_gets_every_kind_of_string_payload(con, tmp_path):
    """A host consumer of LZ4 record batches that are expanded in HBM reads string_t rows that point into a pinned mirror of
    the body, into which the payload buffers are copied back: buffer 2 of utf8 / large_binary, buffer 1 of fixed_size_binary,
    every variadic buffer of a string view (here two).  Two record batches of 3000 rows, against pyarrow."""
    rng = np.random.default_rng(61)
    n = 6000
    t = pa.table({
        "u": pa.array(["utf8 %d %s" % (i, "past the inline twelve bytes" * (i % 3)) for i in range(n)], mask=rng.random(n) < 0.1),
        "lb": pa.array([b"\x00large %d" % i + b"\xff" * (i % 23) for i in range(n)], pa.large_binary(), mask=rng.random(n) < 0.1),
        "fb": pa.array([b"%013d" % i for i in range(n)], pa.binary(13), mask=rng.random(n) < 0.1),
        # 16 bytes each, an array per record batch: 48000 bytes of payload, which pyarrow keeps in two data buffers
        "sv": pa.chunked_array([pa.array(["view %011d" % i for i in range(lo, lo + 3000)], pa.string_view()) for lo in (0, 3000)]),
        "k": pa.array(np.arange(n, dtype=np.int64)),
    })
    path = str(tmp_path / "strings.arrows")
    _write(path, t, 3000)
    batches = list(ipc.open_stream(path))
    assert [b.num_rows for b in batches] == [3000, 3000] and all(len(b.column("sv").buffers()) == 4 for b in batches)
    rel = con.read_arrow(path, host_decompress="gpu")
    assert [canon_python(c) for c in rel.fetch_columns()] == pyarrow_columns(t)
    assert rel.stats()["lz4_batches_on_device"] == 2


def _messages(stream_bytes):
    out = []
    with pa.BufferReader(stream_bytes) as br:
        reader = ipc.MessageReader.open_stream(br)
        while True:
            try:
                out.append(reader.read_next_message().serialize().to_pybytes())
            except StopIteration:
                return out


def test_plain_and_lz4_batches_with_raw_buffers_in_one_scan_that_grows_its_slots(con, tmp_path):
    """One stream whose record batches are plain, plain, LZ4, LZ4, plain, LZ4, LZ4, plain (compression is a property of the
    message), the LZ4 ones with their second buffer stored raw.  With pipeline_depth left to the scan it starts with three
    slots and grows to eight at the first compressed body, while the plain batches in front of it are in flight; a GPU and a
    host consumer, against pyarrow."""
    rng = np.random.default_rng(67)
    n = 8 * 3000
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "r": pa.array(rng.integers(0, 1 << 62, n)),
                  "s": pa.array(["row %d %s" % (i % 101, "x" * (i % 17)) for i in range(n)], mask=rng.random(n) < 0.1)})

    def stream(codec):
        sink = pa.BufferOutputStream()
        with ipc.new_stream(sink, t.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
            w.write_table(t, max_chunksize=3000)
        return sink.getvalue().to_pybytes()

    plain, packed = _messages(stream(None)), _messages(rewrite_buffers_raw(stream("lz4"), lambda bi, k, ln: k == 1))
    assert len(plain) == len(packed) == 9       # the schema and eight record batches
    mixed = plain[0] + b"".join((plain if i in (1, 2, 5, 8) else packed)[i] for i in range(1, 9)) + b"\xff\xff\xff\xff\x00\x00\x00\x00"
    assert ipc.open_stream(pa.py_buffer(mixed)).read_all().equals(t)
    path = str(tmp_path / "mixed.arrows")
    open(path, "wb").write(mixed)
    want = pyarrow_columns(t)
    got, st = _device_scan(con, path, pipeline_depth=0)
    assert got == want and st["record_batches"] == 8 and st["lz4_batches_on_device"] == 4, st
    rel = con.read_arrow(path, host_decompress="gpu", pipeline_depth=0)
    assert [canon_python(c) for c in rel.fetch_columns()] == want
    assert rel.stats()["lz4_batches_on_device"] == 4

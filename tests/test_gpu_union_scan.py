"""Arrow union columns (sparse and dense) decoded on the MI355X into DuckDB UNION vectors (kernels_union.hip), through every
consumer of the planner: the scan operator for host and device-resident consumers, scan_arrow_ipc, the HBM-resident mode,
compressed bodies, projection, two files.  fetch_columns() equals pyarrow's to_pylist(); the vector tree of the HBM-resident
mode equals union_cases.union_reference bit for bit (held to pyarrow in test_union_reference_host.py); the unions the path
refuses are refused at bind by name, and the two damaged-file errors leave the connection usable.
(Whole unions only: see test_union_reference_host.py on what pyarrow writes for a sliced dense union.)"""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd.hbm import HbmStream

import union_cases as uc

pytestmark = pytest.mark.gpu

BATCH_ROWS = [4000, 4000, 1000]          # several tiles each, the last one ragged
N = sum(BATCH_ROWS)


@pytest.fixture(scope="module")
def con():
    c = da.Connection(0)
    yield c
    c.close()


def write(path, table, compression=None):
    """one message per chunk of the table, as it is: the record batches are built whole (a dense union is never sliced here)"""
    opts = ipc.IpcWriteOptions(compression=compression) if compression else None
    with ipc.new_stream(path, table.schema, options=opts) as w:
        for b in table.to_batches():
            w.write_batch(b)
    return path


def norm(v):
    """pyarrow python values -> what fetch_columns() returns: stored integers for decimals"""
    if isinstance(v, decimal.Decimal):
        return int(v.scaleb(2))
    if isinstance(v, dict):
        return {k: norm(x) for k, x in v.items()}
    if isinstance(v, list):
        return [norm(x) for x in v]
    return v


def member_array(kind, n, rng):
    null = rng.random(n) < 0.1
    ints = rng.integers(-10**6, 10**6, n)
    if kind == "int32":
        return pa.array(ints.astype(np.int32), pa.int32(), mask=null)
    if kind == "int64":
        return pa.array(ints * 10**9, pa.int64(), mask=null)
    if kind == "dec":
        return pa.array([None if z else decimal.Decimal(int(v)).scaleb(-2) for v, z in zip(ints, null)], pa.decimal128(15, 2))
    if kind == "utf8":       # inline strings and rows over 12 bytes
        return pa.array([None if z else ("s%d" % v if v % 2 else "a string of more than twelve bytes %d" % v) for v, z in zip(ints, null)])
    if kind == "list":
        return pa.array([None if z else [int(v), int(v) + 1][: v % 3] for v, z in zip(ints, null)], pa.list_(pa.int64()))
    if kind == "struct":
        return pa.StructArray.from_arrays([pa.array(ints.astype(np.int16), pa.int16()), member_array("utf8", n, rng)], ["x", "y"], mask=pa.array(null))
    assert kind == "union"
    ids = pa.array(np.asarray((5, 7), np.int8)[rng.integers(0, 2, n)], pa.int8())
    return pa.UnionArray.from_sparse(ids, [member_array("int32", n, rng), member_array("utf8", n, rng)], ["i", "s"], [5, 7])


def make_union(mode, kinds, codes, n, rng):
    tag = rng.integers(0, len(kinds), n)
    ids = pa.array(np.asarray(codes, np.int8)[tag], pa.int8())
    names = ["m%d_%s" % (k, kind) for k, kind in enumerate(kinds)]
    if mode == "sparse":
        return pa.UnionArray.from_sparse(ids, [member_array(kind, n, rng) for kind in kinds], names, list(codes))
    lengths = [n // 3 + 11 * k for k in range(len(kinds))]          # shorter than the union: rows share child rows, some are skipped
    offsets = np.array([2 * rng.integers(0, (lengths[k] + 1) // 2) for k in tag], np.int32)
    return pa.UnionArray.from_dense(ids, pa.array(offsets, pa.int32()), [member_array(kind, ln, rng) for kind, ln in zip(kinds, lengths)], names, list(codes))


def make_batch(n, first, rng):
    sparse_kinds = ["int32", "int64", "dec", "utf8", "list", "struct", "union"]
    dense_kinds = ["int32", "int64", "dec", "utf8"]
    us = make_union("sparse", ["int32", "utf8"], (5, 7), n, rng)
    ud = make_union("dense", ["int64", "utf8"], (5, 7), n, rng)
    st = pa.StructArray.from_arrays([make_union("sparse", ["int32", "utf8"], (5, 7), n, rng), make_union("dense", ["int64", "dec"], (5, 7), n, rng),
                                     pa.array(np.arange(n), pa.int32())], ["a", "b", "k"], mask=pa.array(np.arange(n) % 7 == 3))
    return pa.record_batch({"k": pa.array(first + np.arange(n), pa.int64()), "us": us, "ud": ud,
                            "ub": make_union("sparse", sparse_kinds, (3, 9, 27, 81, 6, 8, 100), n, rng),
                            "dd": make_union("dense", dense_kinds, (100, 0, 64, 127), n, rng), "st": st})


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2024)
    firsts = np.cumsum([0] + BATCH_ROWS[:-1])
    return pa.Table.from_batches([make_batch(n, int(f), rng) for n, f in zip(BATCH_ROWS, firsts)])


@pytest.fixture(scope="module")
def expected(table):
    return {name: [norm(v) for chunk in table.column(name).chunks for v in chunk.to_pylist()] for name in table.column_names}


@pytest.fixture(scope="module")
def path(table, tmp_path_factory):
    return write(str(tmp_path_factory.mktemp("union") / "u.arrows"), table)


def _columns(rel):
    return dict(zip(rel.columns, rel.fetch_columns()))


@pytest.mark.parametrize("options", [{}, {"device_resident": True}, {"unset_all_valid": True}, {"zero_copy_direct": -1}], ids=str)
def test_scan_equals_pyarrow(con, path, expected, options):
    rel = con.read_arrow(path, **options)
    assert rel.types[1] == "UNION(m0_int32 INTEGER, m1_utf8 VARCHAR)" and rel.types[2] == "UNION(m0_int64 BIGINT, m1_utf8 VARCHAR)"
    got = _columns(rel)
    for name, want in expected.items():
        assert got[name] == want, (name, options)


def test_fetchall_and_scan_arrow_ipc(con, path, expected):
    with open(path, "rb") as fh:
        blob = fh.read()
    rel = con.scan_arrow_ipc([np.frombuffer(blob, np.uint8)])
    assert rel.fetchall() == list(zip(*[expected[name] for name in rel.columns]))


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compressed_bodies(con, table, expected, tmp_path, codec):
    p = write(str(tmp_path / "c.arrows"), table, compression=codec)
    for options in ({}, {"device_resident": True}):
        got = _columns(con.read_arrow(p, **options))
        assert all(got[name] == want for name, want in expected.items()), (codec, options)


def test_projection_and_two_files(con, table, path, expected, tmp_path):
    assert con.read_arrow(path).project(["dd"]).fetch_columns()[0] == expected["dd"]
    got = con.read_arrow(path).project(["st", "k", "us"]).fetch_columns()
    assert got == [expected["st"], expected["k"], expected["us"]]
    second = write(str(tmp_path / "second.arrows"), table)
    both = _columns(con.read_arrow([path, second]).project(["k", "ud", "ub"]))
    assert both["k"] == expected["k"] * 2 and both["ud"] == expected["ud"] * 2 and both["ub"] == expected["ub"] * 2


# ------------------------------------------------------------------------------------------------ the vector tree, bit for bit
def _reference_of(arr):
    """union_reference of one record batch's union array (members: flat types), from pyarrow's own view of the buffers"""
    mode = "dense" if arr.type.mode == "dense" else "sparse"
    members = [arr.field(k) for k in range(arr.type.num_fields)]
    recs = [(len(m), ~np.asarray(m.is_null()) if m.null_count else None, False) for m in members]
    return mode, members, uc.union_reference(mode, np.asarray(arr.type_codes), np.asarray(arr.offsets) if mode == "dense" else None,
                                             uc.id_map_of(arr.type.type_codes), recs)


def _fixed_bytes(m):
    """(rows, w) bytes of an int32 / int64 member array as its Arrow data buffer holds them -- the bytes under its own NULLs
    included --, None for other types"""
    if m.type in (pa.int32(), pa.int64()):
        w = m.type.bit_width // 8
        raw = np.frombuffer(m.buffers()[1], np.uint8)[m.offset * w: (m.offset + len(m)) * w]
        return raw.reshape(len(m), w)
    return None


@pytest.mark.parametrize("unset_all_valid", [False, True])
def test_hbm_resident_tree_equals_the_reference(table, path, unset_all_valid):
    buf = np.frombuffer(open(path, "rb").read(), np.uint8).copy()
    ctx = da.Context(0)
    hs = HbmStream(ctx, buf, unset_all_valid=unset_all_valid)
    hs.launch()
    assert hs.status() == 0
    hs.launch()                       # decoded again on every launch
    assert hs.status() == 0
    batches = table.select(["us", "ud", "dd"]).to_batches()
    assert [b.num_rows for b in batches] == BATCH_ROWS
    for got, rb in zip(hs.fetch(), batches):
        by = {c["name"]: c for c in got["columns"]}
        n = rb.num_rows
        for name in ("us", "ud", "dd"):
            arr = rb.column(rb.schema.get_field_index(name))
            mode, members, ref = _reference_of(arr)
            node = by[name]
            m = len(members)
            assert node["kind"] == da._ffi.K_UNION and node["width"] == 1 and len(node["children"]) == m + 1
            tags = node["children"][0]
            assert tags["kind"] == da._ffi.K_COPY and tags["width"] == 1 and tags["validity_unset"]
            assert np.array_equal(node["data"][:n], ref["tags"]) and np.array_equal(tags["data"][:n], ref["tags"])
            assert np.array_equal(node["validity"], uc.words_of(ref["valid"])), name
            for k, mem in enumerate(members):
                child = node["children"][1 + k]
                assert (child["kind"] == da._ffi.K_UNION_DENSE) == (mode == "dense"), (name, k, child["kind"])
                assert np.array_equal(child["validity"], uc.words_of(ref["member_ok"][k])), (name, k)
                raw = _fixed_bytes(mem)
                if raw is None:
                    continue
                w = raw.shape[1]
                have = child["data"][: n * w].reshape(n, w)
                want = uc.member_rows(raw, ref["member_src"][k])
                ok = ref["member_ok"][k]
                assert np.array_equal(have[ok], want[ok]), (name, k)
                if mode == "dense":      # an expanded member holds zero wherever it is NULL
                    assert not have[~ok].any(), (name, k)
                else:
                    # a sparse int32 / int64 member is a struct child decoded by transcode_copy (DirectConversion): every slot,
                    # NULL or not, holds the member array's own bytes of that row (the stated departure)
                    assert child["kind"] == da._ffi.K_COPY and np.array_equal(have, raw), (name, k)
                    assert (~ok).any() and raw[~ok].any()
    hs.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ refusals
def _u(members, mode="sparse", n=4):
    ids = pa.array([0] * n, pa.int8())
    names = ["m%d" % k for k in range(len(members))]
    if mode == "sparse":
        return pa.UnionArray.from_sparse(ids, members, names)
    return pa.UnionArray.from_dense(ids, pa.array(range(n), pa.int32()), members, names)


def _refused(con, tmp_path, tbl, name, **options):
    p = write(str(tmp_path / ("%s.arrows" % name)), tbl)
    with pytest.raises(da.MiError) as e:
        con.read_arrow(p, **options).fetch_columns()
    assert e.value.code == da._ffi.MI_ENOTSUP and name in str(e.value), str(e.value)


def test_refused_unions_are_named_at_bind_and_the_connection_goes_on(con, tmp_path, path, expected):
    ints = pa.array(range(4))
    u = _u([ints])
    off = pa.array([0, 2, 4], pa.int32())
    _refused(con, tmp_path, pa.table({"in_list": pa.ListArray.from_arrays(off, u)}), "in_list")
    _refused(con, tmp_path, pa.table({"in_large": pa.LargeListArray.from_arrays(pa.array([0, 2, 4], pa.int64()), u)}), "in_large")
    _refused(con, tmp_path, pa.table({"in_fixed": pa.FixedSizeListArray.from_arrays(u, 2)}), "in_fixed")
    _refused(con, tmp_path, pa.table({"in_map": pa.MapArray.from_arrays(off, pa.array(["a", "b", "c", "d"]), u)}), "in_map")
    _refused(con, tmp_path, pa.table({"many": _u([pa.array(range(4), pa.int8())] * 33)}), "many")
    _refused(con, tmp_path, pa.table({"ree": _u([pa.RunEndEncodedArray.from_arrays(pa.array([2, 4], pa.int32()), pa.array([1, 2], pa.int64()))])}), "ree")
    _refused(con, tmp_path, pa.table({"dict": _u([pa.array(["a", "b", "a", "b"]).dictionary_encode()])}), "dict", accept_dictionaries=True)
    _refused(con, tmp_path, pa.table({"d_null": _u([ints, pa.nulls(4)], "dense")}), "d_null")
    _refused(con, tmp_path, pa.table({"d_list": _u([pa.array([[1], [2], [3], [4]], pa.list_(pa.int64()))], "dense")}), "d_list")
    _refused(con, tmp_path, pa.table({"d_struct": _u([pa.StructArray.from_arrays([ints], ["x"])], "dense")}), "d_struct")
    _refused(con, tmp_path, pa.table({"d_union": _u([u], "dense")}), "d_union")
    _refused(con, tmp_path, pa.table({"d_in_s": _u([_u([ints], "dense")])}), "d_in_s")
    _refused(con, tmp_path, pa.table({"in_ree": pa.RunEndEncodedArray.from_arrays(pa.array([1, 4], pa.int32()), _u([pa.array(range(2))], n=2))}), "in_ree")
    # consumers that need flat columns name the union too
    for kw, call in (({"filter_compact": True}, lambda r: r.filter(("k", "<", 10))), ({}, lambda r: r.filter(("us", "=", 1)))):
        with pytest.raises(da.MiError) as e:
            call(con.read_arrow(path, **kw).project(["k", "us"])).fetch_columns()
        assert e.value.code == da._ffi.MI_ENOTSUP and "'us'" in str(e.value), str(e.value)
    # no aggregate -- COUNT included -- and no GROUP BY key reads a union's vector tree
    for spec in (("count", "us"), ("sum", "us"), ("min", "ud"), ("max", "us"), ("sum_product", "k", "us"), ("sum_expr", "k", "ud")):
        with pytest.raises(da.MiError) as e:
            con.read_arrow(path).aggregate([spec])
        assert e.value.code == da._ffi.MI_ENOTSUP and "union column '%s'" % spec[-1] in str(e.value), (spec, str(e.value))
    for keys in (["us"], ["k", "ud"]):
        with pytest.raises(da.MiError) as e:
            con.read_arrow(path).group_aggregate(keys, [("count_star",)])
        assert e.value.code == da._ffi.MI_ENOTSUP and "GROUP BY on the union column '%s'" % keys[-1] in str(e.value), str(e.value)
    with pytest.raises(da.MiError) as e:
        con.read_arrow(path).sum_product("k", "us")
    assert "'us'" in str(e.value)
    # ... while the same file's other columns aggregate beside them, and the connection goes on
    assert con.read_arrow(path).aggregate([("count_star",), ("count", "k"), ("max", "k")]) == [N, N, N - 1]
    assert con.read_arrow(path).project(["k"]).fetch_columns()[0] == expected["k"]


# ------------------------------------------------------------------------------------------------ damaged files
def test_damaged_type_ids_and_offsets_are_data_errors_and_the_connection_goes_on(con, tmp_path, path, expected):
    ids = np.array([5, 7, 5, 7, 7, 5, 5, 7], np.int8)
    offs = np.array([0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    t = pa.table({"d": pa.UnionArray.from_dense(pa.array(ids, pa.int8()), pa.array(offs, pa.int32()),
                                                [pa.array([10, 11, 12, 13], pa.int64()), pa.array(["a", "b", "c", "d"])], ["i", "s"], [5, 7])})
    raw = open(write(str(tmp_path / "ok.arrows"), t), "rb").read()
    assert raw.count(ids.tobytes()) == 1 and raw.count(offs.tobytes()) == 1
    assert _columns(con.scan_arrow_ipc([np.frombuffer(raw, np.uint8)]))["d"] == t.column("d").to_pylist()

    def damaged(old, new):
        return np.frombuffer(raw.replace(old.tobytes(), new.tobytes()), np.uint8)
    for bad in (-1, 6, 127):
        ids2 = ids.copy()
        ids2[3] = bad
        for options in ({}, {"device_resident": True}):
            with pytest.raises(da.MiError) as e:
                con.scan_arrow_ipc([damaged(ids, ids2)], **options).fetch_columns()
            assert e.value.code == da._ffi.MI_EINVAL and "Arrow union tag out of range" in str(e.value)
    for bad in (-1, 4, 2**31 - 1):
        offs2 = offs.copy()
        offs2[3] = bad
        with pytest.raises(da.MiError) as e:
            con.scan_arrow_ipc([damaged(offs, offs2)]).fetch_columns()
        assert e.value.code == da._ffi.MI_EINVAL and str(e.value).startswith("Arrow IPC validation failed: union offsets")
    assert con.read_arrow(path).project(["us"]).fetch_columns()[0] == expected["us"]

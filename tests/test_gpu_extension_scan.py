"""Arrow canonical extension types through the scan and the writer on the MI355X.

Scan: one file of 5000 rows in record batches of 2048 + 7 with arrow.uuid, arrow.bool8 and arrow.json columns -- plain,
under a struct, a list and a fixed-size list, as members of a sparse and of a dense union, run-end encoded, and
dictionary-encoded with a dictionary delta -- read by the host consumer, the device-resident consumer and scan_arrow_ipc,
from LZ4 and ZSTD bodies, under projection and as two files.  Expected values are pyarrow's own reading of the same file
(uuid.UUID, bool, str) and, for the dictionary column pyarrow cannot build, the Python list it was made from.  Filters,
aggregates and GROUP BY on UUID columns against a Python evaluation.

Writer: UUID columns leave as utf8 text (DuckDB's default, arrow_lossless_conversion = false), JSON columns as arrow.json on
utf8; pyarrow reads both back."""
import uuid

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

import duckdb_arrow_amd as da

import extension_cases as ec

pytestmark = pytest.mark.gpu

BATCH_ROWS = [2048 + 7, 2048 + 7, 890]
N = sum(BATCH_ROWS)
EXT = {"ARROW:extension:name": "arrow.uuid", "ARROW:extension:metadata": ""}


@pytest.fixture(scope="module")
def con():
    c = da.Connection(0)
    yield c
    c.close()


def _uuid_array(values):
    return pa.array([None if v is None else v.bytes for v in values], pa.uuid())


def _bool8_array(raw, null):
    return pa.ExtensionArray.from_storage(pa.bool8(), pa.array(raw, pa.int8(), mask=null))


class Data:
    """the columns as Python lists, and the record batches pyarrow writes for them"""

    def __init__(self):
        rng = np.random.default_rng(2025)
        pool = ec.random_uuids(300, rng)
        self.pool = pool
        self.groups = sorted(pool[20:25], key=str)
        self.cols = {k: [] for k in ("k", "u", "b", "j", "g", "du", "r", "rb")}
        self.batches = []
        dict_type = pa.dictionary(pa.int16(), pa.binary(16))
        first = 0
        for bi, n in enumerate(BATCH_ROWS):
            u = [None if rng.random() < 0.1 else pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
            raw = rng.choice(np.array(ec.BOOL8_BYTES, np.uint8).view(np.int8), n)
            bnull = rng.random(n) < 0.1
            b = [None if z else bool(v) for v, z in zip(raw, bnull)]
            j = [None if rng.random() < 0.1 else ('{"k": %d, "pad": "%s"}' % (first + i, "x" * (i % 20))) for i in range(n)]
            g = [None if rng.random() < 0.05 else self.groups[int(rng.integers(0, 5))] for _ in range(n)]
            # dictionary-encoded: the dictionary grows from batch to batch (a delta), indices and entries can be NULL
            dict_len = 40 + 30 * bi
            dvals = [None if e == 7 else pool[e] for e in range(dict_len)]
            idx = rng.integers(0, dict_len, n)
            inull = rng.random(n) < 0.1
            du = [None if z else dvals[int(e)] for e, z in zip(idx, inull)]
            darr = pa.DictionaryArray.from_arrays(pa.array(idx.astype(np.int16), pa.int16(), mask=inull),
                                                  pa.array([None if v is None else v.bytes for v in dvals], pa.binary(16)))
            # run-end encoded: runs of 1 .. 300 rows, NULL runs among them
            ends, rv, rbv = [], [], []
            while (ends[-1] if ends else 0) < n:
                ends.append(min(n, (ends[-1] if ends else 0) + int(rng.integers(1, 300))))
                rv.append(None if rng.random() < 0.15 else pool[int(rng.integers(0, len(pool)))])
                rbv.append(None if rng.random() < 0.15 else int(rng.choice(ec.BOOL8_BYTES)))
            lens = np.diff([0] + ends)
            r = [v for v, ln in zip(rv, lens) for _ in range(ln)]
            rb = [None if v is None else v != 0 for v, ln in zip(rbv, lens) for _ in range(ln)]
            ua, ba, ja = _uuid_array(u), _bool8_array(raw, bnull), pa.array(j, pa.json_())
            st = pa.StructArray.from_arrays([ua, ba, ja], ["u", "b", "j"], mask=pa.array(np.arange(n) % 7 == 3))
            lst = pa.ListArray.from_arrays(pa.array(np.minimum(np.arange(n + 1) * 2, n), pa.int32()), ua)
            fl = pa.FixedSizeListArray.from_arrays(pa.concat_arrays([ba, ba]), 2)
            tag = rng.integers(0, 3, n)
            us = pa.UnionArray.from_sparse(pa.array(tag.astype(np.int8), pa.int8()), [ua, ba, ja], ["u", "b", "j"])
            dtag = rng.integers(0, 2, n)
            offs = np.array([2 * rng.integers(0, n // 2) for _ in range(n)], np.int32)
            ud = pa.UnionArray.from_dense(pa.array(dtag.astype(np.int8), pa.int8()), pa.array(offs, pa.int32()), [ua, ba], ["u", "b"])
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), _uuid_array(rv))
            ree_b = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int16()), _bool8_array(np.array([v or 0 for v in rbv], np.uint8).view(np.int8),
                                                                                                np.array([v is None for v in rbv])))
            arrays = {"k": pa.array(first + np.arange(n), pa.int64()), "u": ua, "b": ba, "j": ja, "g": _uuid_array(g), "du": darr, "r": ree, "rb": ree_b,
                      "st": st, "l": lst, "fl": fl, "us": us, "ud": ud}
            fields = [pa.field(name, a.type, metadata=EXT) if name == "du" else pa.field(name, a.type) for name, a in arrays.items()]
            self.batches.append(pa.record_batch(list(arrays.values()), schema=pa.schema(fields)))
            for name, vals in (("k", list(range(first, first + n))), ("u", u), ("b", b), ("j", j), ("g", g), ("du", du), ("r", r), ("rb", rb)):
                self.cols[name] += vals
            first += n
        assert dict_type == self.batches[0].schema.field("du").type
        # pyarrow's own reading of the nested columns (everything but the dictionary column, which it cannot build)
        for name in ("st", "l", "fl", "us", "ud"):
            self.cols[name] = [v for rb_ in self.batches for v in rb_.column(rb_.schema.get_field_index(name)).to_pylist()]
        for name in ("u", "b", "j", "g", "r", "rb"):
            assert self.cols[name] == [v for rb_ in self.batches for v in rb_.column(rb_.schema.get_field_index(name)).to_pylist()], name

    def stream(self, **options):
        return ec.ipc_stream(self.batches, self.batches[0].schema, emit_dictionary_deltas=True, **options)


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def path(data, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ext") / "ext.arrows")
    with open(p, "wb") as fh:
        fh.write(data.stream())
    return p


def _columns(rel):
    return dict(zip(rel.columns, rel.fetch_columns()))


def _check(got, data, names=None):
    for name in names or data.cols:
        assert got[name] == data.cols[name], name


@pytest.mark.parametrize("options", [{}, {"device_resident": True}, {"unset_all_valid": True}, {"zero_copy_direct": -1}], ids=str)
def test_scan_equals_pyarrow(con, path, data, options):
    rel = con.read_arrow(path, accept_dictionaries=True, **options)
    types = dict(zip(rel.columns, rel.types))
    assert [types[k] for k in ("u", "b", "j", "g", "du", "r", "rb")] == ["UUID", "BOOLEAN", "JSON", "UUID", "UUID", "UUID", "BOOLEAN"]
    assert types["st"] == "STRUCT(u UUID, b BOOLEAN, j JSON)" and types["l"] == "UUID[]" and types["fl"] == "BOOLEAN[2]"
    assert types["us"] == "UNION(u UUID, b BOOLEAN, j JSON)" and types["ud"] == "UNION(u UUID, b BOOLEAN)"
    _check(_columns(rel), data)


def test_scan_arrow_ipc_and_fetchall(con, data):
    rel = con.scan_arrow_ipc([np.frombuffer(data.stream(), np.uint8)], accept_dictionaries=True)
    assert rel.fetchall() == list(zip(*[data.cols[name] for name in rel.columns]))


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compressed_bodies(con, data, tmp_path, codec):
    p = str(tmp_path / "c.arrows")
    with open(p, "wb") as fh:
        fh.write(data.stream(compression=codec))
    for options in ({}, {"device_resident": True}):
        _check(_columns(con.read_arrow(p, accept_dictionaries=True, **options)), data)


def test_projection_and_two_files(con, data, path, tmp_path):
    assert con.read_arrow(path, accept_dictionaries=True).project(["b"]).fetch_columns()[0] == data.cols["b"]
    got = con.read_arrow(path, accept_dictionaries=True).project(["r", "du", "k", "u"]).fetch_columns()
    assert got == [data.cols[k] for k in ("r", "du", "k", "u")]
    second = str(tmp_path / "second.arrows")
    with open(second, "wb") as fh:
        fh.write(data.stream())
    both = _columns(con.read_arrow([path, second], accept_dictionaries=True).project(["u", "rb", "du"]))
    assert all(both[k] == data.cols[k] * 2 for k in ("u", "rb", "du"))


# ------------------------------------------------------------------------------------------------ filters
def _filter_cases(data):
    """(expression for the column, Python predicate on a value that is not NULL)"""
    pool = sorted(data.pool, key=str)
    lo, mid, hi = pool[0], pool[len(pool) // 2], pool[-1]
    absent = uuid.UUID(int=(mid.int + 1) % (1 << 128))
    some = [pool[3], pool[77], absent, pool[200]]
    key = lambda v: v.int       # the order of the canonical text
    return [
        (lambda c: (c, "=", mid), lambda v: v == mid), (lambda c: (c, "=", str(mid)), lambda v: v == mid),
        (lambda c: (c, "=", absent), lambda v: False), (lambda c: (c, "<>", mid), lambda v: v != mid),
        (lambda c: (c, "<", mid), lambda v: key(v) < key(mid)), (lambda c: (c, "<=", mid), lambda v: key(v) <= key(mid)),
        (lambda c: (c, ">", mid), lambda v: key(v) > key(mid)), (lambda c: (c, ">=", mid), lambda v: key(v) >= key(mid)),
        (lambda c: (c, "<", lo), lambda v: False), (lambda c: (c, ">=", lo), lambda v: True), (lambda c: (c, "<=", hi), lambda v: True),
        (lambda c: (c, "in", some), lambda v: v in some), (lambda c: (c, "in", [str(s) for s in some]), lambda v: v in some),
        (lambda c: ("and", (c, ">", pool[50]), (c, "<=", pool[250])), lambda v: key(pool[50]) < key(v) <= key(pool[250])),
        (lambda c: ("or", (c, "<", pool[50]), (c, "=", hi)), lambda v: key(v) < key(pool[50]) or v == hi),
    ]


@pytest.mark.parametrize("column", ["u", "du", "r"])
@pytest.mark.parametrize("options", [{}, {"filter_compact": True}], ids=str)
def test_filters_on_uuid_columns(con, path, data, column, options):
    """every comparison, IN and IS [NOT] NULL on the plain, the dictionary-encoded and the run-end encoded column"""
    values, ks = data.cols[column], data.cols["k"]
    for expr, pred in _filter_cases(data):
        rel = con.read_arrow(path, accept_dictionaries=True, **options).project(["k"]).filter(expr(column))
        assert rel.fetch_columns()[0] == [k for k, v in zip(ks, values) if v is not None and pred(v)], expr(column)
    for op, want in (("is null", lambda v: v is None), ("is not null", lambda v: v is not None)):
        rel = con.read_arrow(path, accept_dictionaries=True, **options).project(["k"]).filter((column, op))
        assert rel.fetch_columns()[0] == [k for k, v in zip(ks, values) if want(v)]
    # the 0 / 1 byte of a bool8 column filters as a BOOLEAN column's does
    rel = con.read_arrow(path, accept_dictionaries=True, **options).project(["k"]).filter(("and", ("b", "=", 1), ("u", "is not null")))
    assert rel.fetch_columns()[0] == [k for k, b, u in zip(ks, data.cols["b"], data.cols["u"]) if b and u is not None]


def test_filter_constants_that_do_not_fit_are_refused_by_column(con, path, data):
    """an int64 is no UUID (sign-extended it names a value no text maps to); a 128-bit integer is the hugeint_t image itself"""
    for column in ("u", "du", "r"):
        for expr in ((column, "=", 5), (column, "in", [1, 2]), (column, ">=", -1)):
            with pytest.raises(da.MiError) as e:
                con.read_arrow(path, accept_dictionaries=True).filter(expr).count()
            assert e.value.code == da._ffi.MI_EINVAL and "'%s'" % column in str(e.value) and "UUID" in str(e.value), str(e.value)
    values = data.cols["u"]
    image = da.uuid_to_hugeint(sorted(data.pool, key=str)[100])
    assert abs(image) >= 1 << 63
    rel = con.read_arrow(path, accept_dictionaries=True).filter(("u", "<", image))
    assert rel.count() == sum(1 for v in values if v is not None and da.uuid_to_hugeint(v) < image)


# ------------------------------------------------------------------------------------------------ aggregates
def test_count_min_max_and_the_sum_refusal(con, path, data):
    for column in ("u", "r"):
        vals = [v for v in data.cols[column] if v is not None]
        got = con.read_arrow(path, accept_dictionaries=True).aggregate([("count", column), ("min", column), ("max", column), ("count_star",)])
        assert got == [len(vals), min(vals, key=str), max(vals, key=str), N], column
    mid = sorted(data.pool, key=str)[150]
    vals = [v for v in data.cols["u"] if v is not None and v.int > mid.int]
    got = con.read_arrow(path, accept_dictionaries=True).filter(("u", ">", mid)).aggregate([("count", "u"), ("min", "u"), ("max", "u"), ("count", "b")])
    assert got == [len(vals), min(vals, key=str), max(vals, key=str),
                   sum(1 for u, b in zip(data.cols["u"], data.cols["b"]) if u is not None and u.int > mid.int and b is not None)]
    for spec in (("sum", "u"), ("sum_product", "k", "u"), ("min", "b"), ("max", "rb")):
        with pytest.raises(da.MiError) as e:
            con.read_arrow(path, accept_dictionaries=True).aggregate([spec])
        assert e.value.code == da._ffi.MI_ENOTSUP and "'%s'" % spec[-1] in str(e.value) and spec[0].split("_")[0].upper() in str(e.value), (spec, str(e.value))


def test_group_by_a_uuid_key_with_a_bool8_key_beside_it(con, path, data):
    want = {}
    for g, b, k, u in zip(data.cols["g"], data.cols["b"], data.cols["k"], data.cols["u"]):
        cnt, ksum, nu, umax = want.get((g, b), (0, 0, 0, None))
        umax = u if u is not None and (umax is None or u.int > umax.int) else umax
        want[(g, b)] = (cnt + 1, ksum + k, nu + (u is not None), umax)
    order = lambda key: tuple((v is None, (v.int if isinstance(v, uuid.UUID) else int(v)) if v is not None else 0) for v in key)
    rows = con.read_arrow(path, accept_dictionaries=True).group_aggregate(["g", "b"], [("count_star",), ("sum", "k"), ("count", "u"), ("max", "u")])
    assert rows == [(key, list(want[key])) for key in sorted(want, key=order)]
    assert len(rows) == 6 * 3 and all(isinstance(key[0], (uuid.UUID, type(None))) and isinstance(key[1], (bool, type(None))) for key, _ in rows)


# ------------------------------------------------------------------------------------------------ writer
def _uuid_table(n, rng, nulls=True):
    us = ec.random_uuids(n, rng)
    u = [None if nulls and rng.random() < 0.2 else v for v in us]
    if nulls and n > 2200:
        u[1990:2110] = [None] * 120        # a NULL run across the first tile seam
    j = [None if rng.random() < 0.1 else ('{"row": %d, "text": "%s"}' % (i, "y" * (i % 30))) for i in range(n)]
    return da.Table(["k", "u", "j", "v"], ["BIGINT", "UUID", "JSON", "VARCHAR"], [list(range(n)), u, j, ["v%d" % i for i in range(n)]]), u, j


def _read_back(paths):
    return pa.concat_tables([ipc.open_stream(p).read_all() for p in paths])


@pytest.mark.parametrize("options", [{}, {"compression": "lz4"}, {"arrow_large_buffer_size": True}, {"produce_arrow_string_view": True},
                                     {"produce_arrow_string_view": True, "arrow_large_buffer_size": True}, {"row_group_size": 3000},
                                     {"row_group_size": 2048, "row_groups_per_file": 2}], ids=str)
def test_copy_to_of_uuid_and_json_columns(con, tmp_path, options):
    rng = np.random.default_rng(31)
    n = 7000
    table, u, j = _uuid_table(n, rng)
    files = con.copy_to(table, str(tmp_path / "out.arrows"), **options)
    got = _read_back(files)
    got.validate(full=True)
    large, views = options.get("arrow_large_buffer_size", False), options.get("produce_arrow_string_view", False)
    # a UUID column is text, and never a view: DuckDB's switch for UUID looks at the offset size alone
    assert got.schema.field("u").type == (pa.large_string() if large else pa.string()) and not got.schema.field("u").metadata
    assert got.schema.field("j").type == pa.json_(pa.string_view() if views else pa.large_string() if large else pa.string())
    assert got.schema.field("v").type == (pa.string_view() if views else pa.large_string() if large else pa.string())
    assert got.column("u").to_pylist() == [None if v is None else str(v) for v in u]
    assert got.column("j").to_pylist() == j and got.column("k").to_pylist() == list(range(n))
    assert got.column("u").null_count == sum(v is None for v in u)
    # ... and this project reads its own file back as VARCHAR and JSON
    rel = con.read_arrow(files)
    assert dict(zip(rel.columns, rel.types))["j"] == "JSON" and dict(zip(rel.columns, rel.types))["u"] == "VARCHAR"
    assert _columns(rel)["j"] == j


def test_to_arrow_ipc_of_uuid_and_json_columns(con):
    rng = np.random.default_rng(32)
    table, u, j = _uuid_table(5000, rng)
    rows = con.to_arrow_ipc(table, chunk_size=2048)
    assert rows[0][1] and not any(h for _, h in rows[1:]) and len(rows) == 1 + 3
    got = ipc.open_stream(pa.BufferReader(b"".join(blob for blob, _ in rows) + b"\xff\xff\xff\xff\x00\x00\x00\x00")).read_all()
    got.validate(full=True)
    assert got.column("u").to_pylist() == [None if v is None else str(v) for v in u] and got.column("j").to_pylist() == j


@pytest.mark.parametrize("compression", [None, "lz4"])
def test_read_copy_read_of_a_uuid_file_through_both_pumps(con, tmp_path, monkeypatch, compression):
    """COPY (FROM read_arrow('uuid.arrows')) TO: the fused pump encodes the decoded hugeint_t rows where they lie in HBM, the
    sink-thread pump stages them on the host; both write the file the one-thread sink writes, and pyarrow reads the UUIDs
    back as text.  Record batches larger than, equal to and no multiple of the row group."""
    rng = np.random.default_rng(33)
    n = 30000
    us = ec.random_uuids(n, rng)
    u = [None if rng.random() < 0.15 else v for v in us]
    u[4000:4200] = [None] * 200
    raw = rng.choice(np.array(ec.BOOL8_BYTES, np.uint8).view(np.int8), n)
    t = pa.table({"k": pa.array(np.arange(n), pa.int64()), "u": _uuid_array(u), "j": pa.array(['{"k": %d}' % i for i in range(n)], pa.json_()),
                  "b": _bool8_array(raw, rng.random(n) < 0.1), "all": _uuid_array(us)})
    extra = {"compression": compression} if compression else {}
    for chunk, rgs in ((10000, 4096), (4096, 4096), (7001, 5000)):
        src = str(tmp_path / ("src_%d.arrows" % chunk))
        with ipc.new_stream(src, t.schema) as w:
            w.write_table(t, max_chunksize=chunk)
        monkeypatch.delenv("MI_WRITER_NO_FUSED", raising=False)
        one = con.copy_to(con.read_arrow(src), str(tmp_path / ("one_%d" % chunk)), row_group_size=rgs, file_size_bytes=1 << 40, **extra)
        want = open(one[0], "rb").read()
        outs = []
        for threads, fused in (("1", False), ("4", False), ("4", True)):
            monkeypatch.setenv("MI_WRITER_THREADS", threads)
            if fused:
                monkeypatch.delenv("MI_WRITER_NO_FUSED", raising=False)
            else:
                monkeypatch.setenv("MI_WRITER_NO_FUSED", "1")
            out = str(tmp_path / ("out_%d_%s_%d.arrows" % (chunk, threads, fused)))
            groups0, _ = da.writer_fused_counts()
            con.copy_to(con.read_arrow(src), out, row_group_size=rgs, **extra)
            groups1, _ = da.writer_fused_counts()
            assert (groups1 > groups0) == fused, (chunk, threads, fused)
            outs.append(open(out, "rb").read())
        assert outs[0] == want and outs[1] == want and outs[2] == want, (chunk, rgs)
        got = ipc.open_stream(pa.BufferReader(outs[2])).read_all()
        got.validate(full=True)
        assert got.schema.field("u").type == pa.string() and got.schema.field("j").type == pa.json_() and got.schema.field("b").type == pa.bool_()
        assert got.column("u").to_pylist() == [None if v is None else str(v) for v in u]
        assert got.column("all").to_pylist() == [str(v) for v in us]
        assert got.column("b").to_pylist() == t.column("b").to_pylist() and got.column("j").to_pylist() == t.column("j").to_pylist()
    monkeypatch.delenv("MI_WRITER_NO_FUSED", raising=False)

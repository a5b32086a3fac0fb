"""Arrow canonical extension types without a GPU: what the host reader binds for pyarrow-written streams (UUID, BOOLEAN, JSON
at the top level, under structs and lists, as the values of a run-end array, as a union member, dictionary-encoded), the
names and storage types that are NOT honoured, the schema message the writer side encodes for UUID and JSON columns, the
constants of the header, and extension_format.hpp under ASan + UBSan as a program of its own
(tests/sanitize/extension_format_check.cpp).  No sanitizer touches code loaded into Python."""
import os
import shutil
import subprocess
import uuid

import numpy as np
import pyarrow as pa
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import extension_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6
UUIDS = [uuid.UUID(int=(k * 0x1234567890ABCDEF1122334455667788 + k) % (1 << 128)) for k in range(N)]


def _uuid_array():
    return pa.array([u.bytes for u in UUIDS], pa.uuid())


def _bool8_array():
    return pa.ExtensionArray.from_storage(pa.bool8(), pa.array([0, 1, 2, -1, None, 0x7F], pa.int8()))


def _json_array(storage=pa.string()):
    return pa.ExtensionArray.from_storage(pa.json_(storage), pa.array(['{"a": 1}', None, "[]", "1", '"x"', "null"], storage))


def _schema(table):
    r = da.Reader(buffers=[ec.ipc_stream(table)])
    try:
        return {f["name"]: f for f in r.schema()}
    finally:
        r.close()


def test_top_level_fields_bind_as_uuid_boolean_and_json():
    f = _schema(pa.table({"u": _uuid_array(), "b": _bool8_array(), "j": _json_array(), "jl": _json_array(pa.large_string()),
                          "jv": _json_array(pa.string_view())}))
    assert (f["u"]["duck_type"], f["u"]["kind"], f["u"]["out_width"], f["u"]["param"]) == ("UUID", _ffi.K_UUID, 16, 16)
    assert (f["b"]["duck_type"], f["b"]["kind"], f["b"]["out_width"]) == ("BOOLEAN", _ffi.K_BOOL8, 1)
    assert (f["j"]["duck_type"], f["j"]["kind"]) == ("JSON", _ffi.K_STR32)
    assert (f["jl"]["duck_type"], f["jl"]["kind"]) == ("JSON", _ffi.K_STR64)
    assert (f["jv"]["duck_type"], f["jv"]["kind"]) == ("JSON", _ffi.K_STRVIEW)
    # the storage type is what the Arrow C format and the buffer layout keep saying
    assert [f[k]["format"] for k in ("u", "b", "j", "jl", "jv")] == ["w:16", "c", "u", "U", "vu"]
    assert [f[k]["n_buffers"] for k in ("u", "b", "j")] == [2, 2, 3]


def test_children_of_structs_lists_maps_run_ends_and_unions():
    u, b, j = _uuid_array(), _bool8_array(), _json_array()
    offsets = pa.array(range(N + 1), pa.int32())
    ree = pa.RunEndEncodedArray.from_arrays(pa.array([2, 5, 6], pa.int32()), u[:3])
    ree_b = pa.RunEndEncodedArray.from_arrays(pa.array([2, 5, 6], pa.int16()), b[:3])
    sparse = pa.UnionArray.from_sparse(pa.array([0, 1, 2] * 2, pa.int8()), [u, b, j], ["u", "b", "j"])
    dense = pa.UnionArray.from_dense(pa.array([0, 1] * 3, pa.int8()), pa.array([0, 0, 1, 1, 2, 2], pa.int32()), [u, b], ["u", "b"])
    f = _schema(pa.table({
        "s": pa.StructArray.from_arrays([u, b, j], ["u", "b", "j"]),
        "l": pa.ListArray.from_arrays(offsets, u),
        "fl": pa.FixedSizeListArray.from_arrays(pa.concat_arrays([b, b]), 2),
        "m": pa.MapArray.from_arrays(offsets, pa.array(range(N), pa.int32()), u),
        "r": ree, "rb": ree_b, "us": sparse, "ud": dense,
    }))
    assert f["s"]["duck_type"] == "STRUCT(u UUID, b BOOLEAN, j JSON)"
    assert f["l"]["duck_type"] == "UUID[]"
    assert f["fl"]["duck_type"] == "BOOLEAN[2]"
    assert f["m"]["duck_type"] == "MAP(INTEGER, UUID)"
    assert (f["r"]["duck_type"], f["r"]["kind"], f["r"]["out_width"]) == ("UUID", _ffi.K_RUN_END, 16)
    assert (f["rb"]["duck_type"], f["rb"]["kind"], f["rb"]["out_width"]) == ("BOOLEAN", _ffi.K_RUN_END, 1)
    assert (f["us"]["duck_type"], f["us"]["kind"]) == ("UNION(u UUID, b BOOLEAN, j JSON)", _ffi.K_UNION)
    assert (f["ud"]["duck_type"], f["ud"]["kind"]) == ("UNION(u UUID, b BOOLEAN)", _ffi.K_UNION)


def test_batch_nodes_carry_the_kinds_at_every_depth():
    t = pa.table({"s": pa.StructArray.from_arrays([_uuid_array(), _bool8_array()], ["u", "b"])})
    r = da.Reader(buffers=[ec.ipc_stream(t)])
    nodes = {n["name"]: n for n in r.next_batch()["nodes"]}
    assert (nodes["u"]["kind"], nodes["u"]["out_width"]) == (_ffi.K_UUID, 16)
    assert (nodes["b"]["kind"], nodes["b"]["out_width"]) == (_ffi.K_BOOL8, 1)
    r.close()


def _extension_field(name, storage, ext_name):
    return pa.field(name, storage, metadata={"ARROW:extension:name": ext_name, "ARROW:extension:metadata": ""})


def test_dictionary_encoded_uuid_binds_by_hand_written_metadata():
    """pyarrow builds no dictionary array of an extension type, but writes field metadata as it is given"""
    values = pa.array([u.bytes for u in UUIDS[:3]], pa.binary(16))
    arr = pa.DictionaryArray.from_arrays(pa.array([0, 1, 2, None, 1, 0], pa.int8()), values)
    schema = pa.schema([_extension_field("du", arr.type, "arrow.uuid"), pa.field("plain", arr.type)])
    f = _schema(pa.Table.from_arrays([arr, arr], schema=schema))
    assert (f["du"]["duck_type"], f["du"]["kind"], f["du"]["has_dictionary"]) == ("UUID", _ffi.K_DICT, 1)
    assert (f["plain"]["duck_type"], f["plain"]["kind"]) == ("BLOB", _ffi.K_DICT)


def test_other_names_and_other_storage_types_read_as_before():
    eight = pa.array([bytes(8)] * N, pa.binary(8))
    sixteen = pa.array([u.bytes for u in UUIDS], pa.binary(16))
    i8, u8, i16 = (pa.array(range(N), t) for t in (pa.int8(), pa.uint8(), pa.int16()))
    text, blob = pa.array(["{}"] * N), pa.array([b"{}"] * N)
    schema = pa.schema([
        _extension_field("unknown", sixteen.type, "acme.uuid"), _extension_field("opaque", sixteen.type, "arrow.opaque"),
        _extension_field("uuid8", eight.type, "arrow.uuid"), _extension_field("uuid_text", text.type, "arrow.uuid"),
        _extension_field("bool_u8", u8.type, "arrow.bool8"), _extension_field("bool_i16", i16.type, "arrow.bool8"),
        _extension_field("json_blob", blob.type, "arrow.json"), _extension_field("json_int", i8.type, "arrow.json"),
        pa.field("no_metadata", sixteen.type), pa.field("other_key", i8.type, metadata={"ARROW:extension:metadata": "arrow.bool8", "k": "arrow.uuid"}),
    ])
    f = _schema(pa.Table.from_arrays([sixteen, sixteen, eight, text, u8, i16, blob, i8, sixteen, i8], schema=schema))
    want = {"unknown": ("BLOB", _ffi.K_FIXED_BINARY), "opaque": ("BLOB", _ffi.K_FIXED_BINARY), "uuid8": ("BLOB", _ffi.K_FIXED_BINARY),
            "uuid_text": ("VARCHAR", _ffi.K_STR32), "bool_u8": ("UTINYINT", _ffi.K_COPY), "bool_i16": ("SMALLINT", _ffi.K_COPY),
            "json_blob": ("BLOB", _ffi.K_STR32), "json_int": ("TINYINT", _ffi.K_COPY), "no_metadata": ("BLOB", _ffi.K_FIXED_BINARY),
            "other_key": ("TINYINT", _ffi.K_COPY)}
    assert {k: (f[k]["duck_type"], f[k]["kind"]) for k in want} == want


def test_encode_schema_of_uuid_and_json_columns_read_back_by_pyarrow():
    msg = bytes(da.encode_schema(["u", "j", "v", "s", "l"], ["UUID", "JSON", "VARCHAR", "STRUCT(u UUID, j JSON)", "JSON[]"]))
    s = pa.ipc.read_schema(pa.py_buffer(msg))
    # DuckDB's default (arrow_lossless_conversion = false): a UUID column leaves as plain utf8 text, JSON as arrow.json on utf8
    assert s.field("u").type == pa.string() and not s.field("u").metadata
    assert s.field("j").type == pa.json_() and s.field("v").type == pa.string()
    assert s.field("s").type == pa.struct([pa.field("u", pa.string()), pa.field("j", pa.json_())])
    assert s.field("l").type == pa.list_(pa.field("l", pa.json_()))
    # ... and the reader of this project binds that schema as VARCHAR and JSON
    r = da.Reader(buffers=[msg + b"\xff\xff\xff\xff\x00\x00\x00\x00"])
    f = {x["name"]: x["duck_type"] for x in r.schema()}
    r.close()
    assert f == {"u": "VARCHAR", "j": "JSON", "v": "VARCHAR", "s": "STRUCT(u VARCHAR, j JSON)", "l": "JSON[]"}


def test_parse_duck_type_and_python_values():
    assert da.parse_duck_type("STRUCT(u UUID, j JSON)[]") == ("list", ("struct", [("u", ("leaf", "UUID")), ("j", ("leaf", "JSON"))]))
    u = UUIDS[3]
    assert da.uuid_from_hugeint(da.uuid_to_hugeint(u)) == u and da.uuid_to_hugeint(uuid.UUID(int=0)) == -(1 << 127)


def test_header_binding_and_kernel_header_agree():
    raw = open(os.path.join(ROOT, "include", "mi_arrow_ipc.h")).read()
    for text in ("MI_K_UUID = 25", "MI_K_BOOL8 = 26", "MI_K_ENC_UUID_TEXT = 39"):
        assert text in raw, text
    assert (_ffi.K_UUID, _ffi.K_BOOL8, _ffi.K_ENC_UUID_TEXT) == (25, 26, 39) == (ec.K_UUID, ec.K_BOOL8, ec.K_ENC_UUID_TEXT)
    hpp = open(os.path.join(ROOT, "duckdb-arrow_amd", "csrc", "extension_format.hpp")).read()
    assert "kUuidBytes = 16" in hpp and "kUuidTextBytes = 36" in hpp


def test_extension_format_header_alone_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "extension_format_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "extension_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "extension_format: ok" in run.stdout

"""The reference of the encode tests (encode_tasks.encode_reference, a numpy restatement of ArrowAppender), checked without
a GPU on the very columns test_gpu_encode_tasks.py runs (all of encode_tasks.CASES but the two 8 MiB strings):

  * against the oracle's per-kind functions where it has one: orc_enc_validity (bitmap, NULL count), orc_enc_decimal_widen,
    orc_enc_bool, orc_enc_varchar32 (int32 offsets and data, with the case's ptr_base);
  * against pyarrow for every kind: pa.Array.from_buffers of the reference's buffers passes validate(full=True), its
    null_count is the reference's and its to_pylist() is what the builder started from -- the only check there is for lists,
    int64 offsets and validity alone;
  * against the builder itself: the validity the reference reads from the words is the one the builder meant, and the data
    buffer of a string column is the builder's text.

Lists whose offsets pass 2**31 cannot be materialised: their int64 offsets are compared with a running sum of Python
integers, and with int32 offsets the reference has to stop at the first offset that does not fit and raise the overflow bit."""
import ctypes as C
import decimal

import numpy as np
import pyarrow as pa
import pytest

from oracle import pyoracle as po

from encode_tasks import (CASES, EXPECTED_STATUS, GPU_ONLY, INT32_MAX, K_ENC_BOOL, K_ENC_COPY, K_ENC_DEC128, K_ENC_LIST32, K_ENC_STR32,
                          K_ENC_VALIDITY, ST_OFFSET_OVERFLOW, case_columns, ragged_copy)

HOST_CASES = [name for name in CASES if name not in GPU_ONLY]


def test_the_host_runs_every_case_but_the_two_8_mib_strings():
    assert GPU_ONLY == ["eight_mib_boundary"] and len(HOST_CASES) == len(CASES) - 1


def test_ragged_copy_equals_a_loop_over_the_rows():
    rng = np.random.default_rng(1)
    lens = np.concatenate([rng.integers(0, 50, 300), [1023, 1024, 1025, 5000]])
    rng.shuffle(lens)
    sstart = np.cumsum(lens) - lens + 3
    dstart = (np.cumsum(lens[::-1]) - lens[::-1])[::-1]            # the rows in reverse order
    src = rng.integers(0, 256, int(lens.sum()) + 3, dtype=np.uint8)
    got, want = np.zeros(int(lens.sum()), np.uint8), np.zeros(int(lens.sum()), np.uint8)
    ragged_copy(got, dstart, src, sstart, lens)
    for d, s, l in zip(dstart, sstart, lens):
        want[d: d + l] = src[s: s + l]
    assert np.array_equal(got, want)


def _oracle(col, ref):
    """the oracle's functions on the column's own buffers"""
    L, n = po.lib(), col["n"]
    words = col["words"]
    wp = words.ctypes.data if words is not None else None
    if ref["bitmap"] is not None:
        bitmap, nulls = np.full((n + 7) // 8, 0xFF, np.uint8), C.c_int64(0)
        L.orc_enc_validity(wp, n, 0, bitmap.ctypes.data, C.byref(nulls))
        assert np.array_equal(bitmap, ref["bitmap"]) and nulls.value == ref["nulls"], col["name"]
    if n == 0:
        return
    src = col["src"]
    if col["kind"] == K_ENC_DEC128:
        want = np.zeros(16 * n, np.uint8)
        L.orc_enc_decimal_widen(src.ctypes.data, col["width"], n, want.ctypes.data)
        assert np.array_equal(want, ref["data"]), col["name"]
    elif col["kind"] == K_ENC_BOOL:
        want = np.full((n + 7) // 8, 0xFF, np.uint8)
        L.orc_enc_bool(src.ctypes.data, wp, n, 0, want.ctypes.data)
        assert np.array_equal(want, ref["data"]), col["name"]
    elif col["kind"] == K_ENC_STR32 and not col["large"]:
        off, data = np.zeros(n + 1, np.int32), np.zeros(len(ref["aux"]) + 1, np.uint8)
        rc = L.orc_enc_varchar32(src.ctypes.data, wp, n, 0, col["ptr_base"], col["heap"].ctypes.data, off.ctypes.data, data.ctypes.data)
        assert rc == 0 and ref["status"] == 0, col["name"]
        assert np.array_equal(off.view(np.uint8), ref["data"]) and np.array_equal(data[:-1], ref["aux"]), col["name"]


def _arrow_type(col):
    if col["kind"] == K_ENC_COPY:
        return pa.binary(16) if col["width"] == 16 else {1: pa.uint8(), 2: pa.uint16(), 4: pa.uint32(), 8: pa.uint64()}[col["width"]]
    if col["kind"] == K_ENC_LIST32:
        child = pa.int32() if col["values"] is not None else pa.null()
        return pa.large_list(child) if col["large"] else pa.list_(child)
    if col["kind"] == K_ENC_STR32:
        return pa.large_binary() if col["large"] else pa.binary()
    return {K_ENC_DEC128: pa.decimal128(38, 0), K_ENC_BOOL: pa.bool_(), K_ENC_VALIDITY: pa.int8()}[col["kind"]]


def _pyarrow(col, ref):
    """the reference's buffers as an Arrow array"""
    n, kind = col["n"], col["kind"]
    if n == 0:       # nothing is defined, not even offsets[0]
        assert all(ref[k] is None or len(ref[k]) == 0 for k in ("bitmap", "data", "aux")) and ref["nulls"] == 0 and ref["status"] == 0
        return
    bitmap = pa.py_buffer(ref["bitmap"].tobytes()) if ref["bitmap"] is not None else None
    data = np.zeros(n, np.uint8) if kind == K_ENC_VALIDITY else ref["data"]       # validity alone: any data buffer will do
    buffers, children = [bitmap, pa.py_buffer(data.tobytes())], []
    if kind == K_ENC_STR32:
        buffers.append(pa.py_buffer(ref["aux"].tobytes()))
    if kind == K_ENC_LIST32:
        total = int(data.view("<i8" if col["large"] else "<i4")[-1])
        children = [pa.array(np.arange(total, dtype=np.int32)) if col["values"] is not None else pa.nulls(total)]
    arr = pa.Array.from_buffers(_arrow_type(col), n, buffers, children=children)
    if col["values"] is not None:
        arr.validate(full=True)
        got = arr.to_pylist()
        if kind == K_ENC_DEC128:
            got = [None if v is None else int(v) for v in got]
        if kind == K_ENC_VALIDITY:
            got = [None if v is None else 0 for v in got]
        assert got == col["values"](), col["name"]
    else:            # lists too long for a child array: the structure and the offsets
        arr.validate()
        assert arr.offsets.to_pylist() == [0] + col["ends"], col["name"]
    assert arr.null_count == ref["nulls"], col["name"]


@pytest.mark.parametrize("case", HOST_CASES)
def test_reference_equals_the_oracle_pyarrow_and_the_builder(case):
    decimal.getcontext().prec = 50
    cols, refs = case_columns(case)
    status = 0
    for col, ref in zip(cols, refs):
        status |= ref["status"]
        ok = np.ones(col["n"], bool) if col["ok"] is None else col["ok"]
        assert ref["nulls"] == (col["n"] - int(ok.sum()) if ref["bitmap"] is not None else 0), col["name"]
        if ref["bitmap"] is not None:
            assert np.array_equal(np.unpackbits(ref["bitmap"], bitorder="little")[: col["n"]].astype(bool), ok), col["name"]
        if col["kind"] == K_ENC_STR32:
            assert np.array_equal(ref["aux"], col["text"]), col["name"]
        _oracle(col, ref)
        if ref["status"] == 0:
            assert ref["loose"] == 0
            _pyarrow(col, ref)
        else:        # int32 offsets that do not fit: exact up to the last one that does, then the bit
            assert col["kind"] == K_ENC_LIST32 and not col["large"] and ref["status"] == ST_OFFSET_OVERFLOW
            fits = [e for e in [0] + col["ends"] if e <= INT32_MAX]
            assert 0 < len(fits) <= col["n"] and col["ends"][-1] > INT32_MAX
            assert ref["data"].view("<i4").tolist() == fits and ref["loose"] == 4 * (col["n"] + 1 - len(fits)), col["name"]
    assert status == EXPECTED_STATUS.get(case, 0)

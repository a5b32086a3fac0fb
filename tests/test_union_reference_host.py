"""union_cases.union_reference -- the numpy restatement the GPU union tests are held to -- against pyarrow, without a GPU:
UnionArray.from_sparse / from_dense(...).to_pylist() gives the selected member's value or None per row, .field(k) the member
arrays.  Type codes (0, 1), (5, 7) and (127, 0, 64); 1, 2 and 32 members; NULLs in members; slices written through IPC; dense
offsets that share and that skip child rows; a member of length 0; and the status rule on hand-written columns."""
import numpy as np
import pyarrow as pa
import pytest

from duckdb_arrow_amd import _ffi

import union_cases as uc


def _int_members(lengths, rng, null_every=0):
    """int32 member arrays; every null_every-th row NULL"""
    arrays, recs, values = [], [], []
    for k, n in enumerate(lengths):
        v = rng.integers(-1000, 1000, n).astype(np.int32) + 10000 * k
        ok = np.ones(n, bool)
        if null_every:
            ok[k % null_every:: null_every] = False
        arrays.append(pa.array(v, pa.int32(), mask=~ok))
        recs.append((n, ok if null_every else None, False))
        values.append(v)
    return arrays, recs, values


def _expect_pylist(ref, values):
    out = []
    for r in range(len(ref["tags"])):
        out.append(int(values[ref["tags"][r]][ref["member_src"][ref["tags"][r]][r]]) if ref["valid"][r] else None)
    return out


def _check_against_pyarrow(arr, mode, codes, ids, offsets, recs, values):
    ref = uc.union_reference(mode, ids, offsets, uc.id_map_of(codes), recs)
    assert ref["status"] == 0
    assert arr.to_pylist() == _expect_pylist(ref, values)
    # the tag is the member index of the row's type id (Arrow's rule), a NULL row's tag is 0
    codes_arr = np.asarray(codes)
    want_tag = np.array([int(np.nonzero(codes_arr == i)[0][0]) for i in ids], np.uint8)
    assert np.array_equal(ref["tags"][ref["valid"]], want_tag[ref["valid"]]) and (ref["tags"][~ref["valid"]] == 0).all()
    # every member: the value where it is selected and valid, NULL in every other row; exactly one member per valid row
    count = np.zeros(len(ids), int)
    for k in range(len(codes)):
        field = arr.field(k).to_pylist()
        ok, src = ref["member_ok"][k], ref["member_src"][k]
        count += ok
        for r in np.nonzero(ok)[0]:
            assert field[src[r]] == int(values[k][src[r]])
            if mode == "sparse":
                assert src[r] == r
    assert np.array_equal(count, ref["valid"].astype(int))
    return ref


@pytest.mark.parametrize("codes", [(0, 1), (5, 7), (127, 0, 64)], ids=str)
@pytest.mark.parametrize("null_every", [0, 3])
def test_sparse_against_pyarrow(codes, null_every):
    rng = np.random.default_rng(11)
    n = 300
    arrays, recs, values = _int_members([n] * len(codes), rng, null_every)
    ids = np.asarray(codes, np.int8)[rng.integers(0, len(codes), n)]
    arr = pa.UnionArray.from_sparse(pa.array(ids, pa.int8()), arrays, ["m%d" % k for k in range(len(codes))], list(codes))
    ref = _check_against_pyarrow(arr, "sparse", codes, ids, None, recs, values)
    assert ref["valid"].all() == (null_every == 0)


@pytest.mark.parametrize("codes", [(0, 1), (5, 7), (127, 0, 64)], ids=str)
@pytest.mark.parametrize("null_every", [0, 3])
def test_dense_against_pyarrow_with_shared_and_skipped_child_rows(codes, null_every):
    rng = np.random.default_rng(12)
    n, lengths = 300, [40, 7, 90][: len(codes)]
    arrays, recs, values = _int_members(lengths, rng, null_every)
    tag = rng.integers(0, len(codes), n)
    ids = np.asarray(codes, np.int8)[tag]
    # offsets drawn from the even child rows only: many rows share one, the odd ones nobody names
    offsets = np.array([2 * rng.integers(0, (lengths[k] + 1) // 2) for k in tag], np.int32)
    assert len(set(zip(tag.tolist(), offsets.tolist()))) < n and (offsets % 2 == 0).all()
    arr = pa.UnionArray.from_dense(pa.array(ids, pa.int8()), pa.array(offsets, pa.int32()), arrays, ["m%d" % k for k in range(len(codes))], list(codes))
    _check_against_pyarrow(arr, "dense", codes, ids, offsets, recs, values)


@pytest.mark.parametrize("m", [1, 2, 32])
@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_member_counts(m, mode):
    rng = np.random.default_rng(13 + m)
    n = 200
    codes = tuple(range(m))
    lengths = [n] * m if mode == "sparse" else [5 + k for k in range(m)]
    arrays, recs, values = _int_members(lengths, rng, 4)
    tag = rng.integers(0, m, n)
    ids = np.asarray(codes, np.int8)[tag]
    names = ["m%d" % k for k in range(m)]
    if mode == "sparse":
        arr, offsets = pa.UnionArray.from_sparse(pa.array(ids, pa.int8()), arrays, names, list(codes)), None
    else:
        offsets = np.array([rng.integers(0, lengths[k]) for k in tag], np.int32)
        arr = pa.UnionArray.from_dense(pa.array(ids, pa.int8()), pa.array(offsets, pa.int32()), arrays, names, list(codes))
    _check_against_pyarrow(arr, mode, codes, ids, offsets, recs, values)


def test_a_member_of_length_0_that_no_row_selects():
    rng = np.random.default_rng(14)
    arrays, recs, values = _int_members([10, 0], rng)
    ids = np.full(50, 5, np.int8)
    offsets = rng.integers(0, 10, 50).astype(np.int32)
    arr = pa.UnionArray.from_dense(pa.array(ids, pa.int8()), pa.array(offsets, pa.int32()), arrays, ["a", "b"], [5, 7])
    ref = _check_against_pyarrow(arr, "dense", (5, 7), ids, offsets, recs, values)
    assert not ref["member_ok"][1].any()


def test_sparse_slices_written_through_ipc_are_rebased_to_offset_0():
    """pyarrow writes a sliced union with its buffers cut to the slice: what a reader sees has offset 0 -- the row_offset of
    a planned task is always 0, other offsets are reachable through hand-built tasks alone.  (Sparse only: the stream
    pyarrow 25 writes for a sliced DENSE union holds offsets that it rebased wrongly, negative ones among them, and reading
    it back through pyarrow itself ends the process.  test_gpu_union_scan.py therefore writes whole dense unions.)"""
    rng = np.random.default_rng(15)
    n = 500
    arrays, _, _ = _int_members([n, n], rng, 5)
    ids = np.asarray((5, 7), np.int8)[rng.integers(0, 2, n)]
    arr = pa.UnionArray.from_sparse(pa.array(ids, pa.int8()), arrays, ["a", "b"], [5, 7])
    sl = arr.slice(67, 301)
    sink = pa.BufferOutputStream()
    tbl = pa.table({"u": sl})
    with pa.ipc.new_stream(sink, tbl.schema) as w:
        w.write_table(tbl)
    back = pa.ipc.open_stream(sink.getvalue()).read_all().column("u").chunk(0)
    assert back.offset == 0 and len(back) == 301 and back.to_pylist() == sl.to_pylist()
    got_ids = np.asarray(back.type_codes)
    assert np.array_equal(got_ids, ids[67: 368])
    members = [back.field(k) for k in range(2)]
    vals = [np.asarray(m.fill_null(0)) for m in members]
    recs2 = [(len(m), ~np.asarray(m.is_null()), False) for m in members]
    ref = uc.union_reference("sparse", got_ids, None, uc.id_map_of((5, 7)), recs2)
    assert ref["status"] == 0 and back.to_pylist() == _expect_pylist(ref, vals)


def test_status_rule_on_hand_written_columns():
    assert (uc.ST_BAD_UNION_TAG, uc.ST_BAD_UNION_OFFSET) == (_ffi.ST_BAD_UNION_TAG, _ffi.ST_BAD_UNION_OFFSET) == (8192, 16384)
    assert uc.MAX_MEMBERS == _ffi.MAX_UNION_MEMBERS == 32 and (_ffi.K_UNION, _ffi.K_UNION_DENSE) == (23, 24)
    table = uc.id_map_of((5, 7))
    members = [(4, None, False), (2, np.array([True, False]), False)]
    clean = uc.union_reference("dense", [5, 7, 7, 5], [3, 0, 1, 0], table, members)
    assert clean["status"] == 0 and clean["tags"].tolist() == [0, 1, 0, 0] and clean["valid"].tolist() == [True, True, False, True]
    assert clean["member_src"][0].tolist() == [3, -1, -1, 0] and clean["member_src"][1].tolist() == [-1, 0, -1, -1]
    for bad_id in (-1, -128, 0, 6, 127):
        r = uc.union_reference("dense", [5, bad_id, 7, 5], [3, 0, 0, 0], table, members)
        assert r["status"] == uc.ST_BAD_UNION_TAG and not r["valid"][1] and r["tags"][1] == 0
        assert r["valid"].tolist() == [True, False, True, True] and not any(ok[1] for ok in r["member_ok"])
    for bad_off in (-1, 2, 2**31 - 1):
        r = uc.union_reference("dense", [5, 7, 7, 5], [3, bad_off, 0, 0], table, members)
        assert r["status"] == uc.ST_BAD_UNION_OFFSET and r["valid"].tolist() == [True, False, True, True] and r["tags"][1] == 0
    # sparse rows have no offsets to damage; a parent's NULL clears the row and raises nothing; a null-type member is NULL
    r = uc.union_reference("sparse", [5, 7, 5], None, table, [(3, None, False), (3, None, True)], parent=np.array([True, True, False]))
    assert r["status"] == 0 and r["valid"].tolist() == [True, False, False] and r["tags"].tolist() == [0, 0, 0]
    both = uc.union_reference("dense", [6, 5], [0, 9], table, members)
    assert both["status"] == uc.ST_BAD_UNION_TAG | uc.ST_BAD_UNION_OFFSET

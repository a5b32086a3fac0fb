"""The numpy restatement of MI_K_ENC_UNION and MI_K_ENC_INTERVAL (union_encode_cases.py) held against pyarrow, without a GPU:
the type ids and the members' buffers under their effective masks, read through pa.UnionArray.from_buffers, are the union
column the case was built from; the interval buffer, read as month_day_nano, is the interval_t rows.  And a proof that the
case list reaches what the GPU test relies on: every mask path, NULL union rows, a member never selected, a tag >= m."""
import numpy as np
import pyarrow as pa
import pytest

import encode_tasks as et
import union_encode_cases as uc


def _buf(a):
    return None if a is None else pa.py_buffer(np.ascontiguousarray(a).tobytes())


def _arrow_member(col, ref):
    """-> (pyarrow array over the reference's buffers, python values -> comparable values) or None for a kind this proof leaves out"""
    n, kind = col["n"], col["kind"]
    bm, data, aux = _buf(ref["bitmap"]), _buf(ref["data"]), _buf(ref["aux"])
    if kind == et.K_ENC_COPY and col["width"] in (1, 2, 4, 8):
        return pa.Array.from_buffers({1: pa.uint8(), 2: pa.uint16(), 4: pa.uint32(), 8: pa.uint64()}[col["width"]], n, [bm, data])
    if kind == et.K_ENC_STR32:
        return pa.Array.from_buffers(pa.large_binary() if col["large"] else pa.binary(), n, [bm, data, aux])
    if kind == et.K_ENC_LIST32:
        child = pa.array(range(col["ends"][-1] if col["ends"] else 0), pa.int64())
        return pa.Array.from_buffers(pa.large_list(pa.int64()) if col["large"] else pa.list_(pa.int64()), n, [bm, data], children=[child])
    if kind == uc.K_ENC_INTERVAL:
        return pa.Array.from_buffers(pa.month_day_nano_interval(), n, [bm, data])
    return None


def _interval_py(v):
    return None if v is None else (v.months, v.days, v.nanoseconds)


@pytest.mark.parametrize("case", list(uc.CASES))
def test_pyarrow_reads_the_restated_buffers_as_the_logical_union(case):
    unions, urefs = uc.case_items(case)
    proved = 0
    for u, ur in zip(unions, urefs):
        arrays = [_arrow_member(c, r) for c, r in zip(u["members"], ur["members"])]
        if any(a is None for a in arrays):
            continue
        for a in arrays:
            a.validate(full=True)
        typ = pa.sparse_union([pa.field("m%d" % k, a.type) for k, a in enumerate(arrays)], list(range(u["m"])))
        arr = pa.UnionArray.from_buffers(typ, u["n"], [None, _buf(ur["type_ids"])], children=arrays)
        arr.validate(full=True)
        got = arr.to_pylist()
        want = uc.logical_values(u, ur)
        for r, (g, w) in enumerate(zip(got, want)):
            if w is None:
                assert g is None, (u["name"], r, g)
                continue
            k, v = w
            if u["members"][k]["kind"] == uc.K_ENC_INTERVAL:
                g, v = _interval_py(g), (v[0], v[1], ((v[2] * 1000 + 2**63) % 2**64) - 2**63)
            assert g == v, (u["name"], r, k, g, v)
            assert int(ur["type_ids"][r]) == k == int(u["tags"][r])
        # the same through from_sparse: type ids as an array
        again = pa.UnionArray.from_sparse(pa.array(ur["type_ids"], pa.int8()), arrays, ["m%d" % k for k in range(u["m"])])
        assert again.to_pylist() == got
        # every member's NULL count is the number of rows its mask leaves out
        for a, r, eff in zip(arrays, ur["members"], ur["effective"]):
            assert a.null_count == r["nulls"] == u["n"] - int(eff.sum())
        proved += 1
    assert proved >= 3


def test_pyarrow_reads_the_interval_buffers_as_the_rows():
    cols, refs = uc.interval_columns()
    for col, ref in zip(cols, refs):
        arr = pa.Array.from_buffers(pa.month_day_nano_interval(), col["n"], [_buf(ref["bitmap"]), _buf(ref["data"])])
        arr.validate(full=True)
        want = col["values"]()
        got = [_interval_py(v) for v in arr.to_pylist()]
        assert got == [None if w is None else (w[0], w[1], ((w[2] * 1000 + 2**63) % 2**64) - 2**63) for w in want], col["name"]
        assert arr.null_count == ref["nulls"]
        ok = et._row_bits(col)
        assert not ref["data"].reshape(-1, 16)[~ok].any(), "a NULL row is 16 zero bytes"
    # the wrapping products are there, under valid rows, and differ from the exact product
    seen = set()
    for col in cols:
        rows = col["src"].view(uc.INTERVAL)
        for m in rows["micros"][et._row_bits(col)].tolist():
            if m in uc.WRAPPING_MICROS:
                seen.add(m)
                assert not -2**63 <= m * 1000 < 2**63
    assert seen == set(uc.WRAPPING_MICROS)
    assert {(uc.I32_MIN, uc.I32_MAX), (uc.I32_MAX, uc.I32_MIN)} <= {(int(r["months"]), int(r["days"])) for c in cols for r in c["src"].view(uc.INTERVAL)}


def test_the_cases_reach_every_path():
    every = [(u, r) for case in uc.CASES for u, r in zip(*uc.case_items(case))]
    assert {u["n"] for u, _ in every} >= set(uc.ROWS) and {u["m"] for u, _ in every} >= {1, 2, 32}
    paths = set()
    for u, ur in every:
        n = u["n"]
        valid = uc._bits(u["words"], n) & uc._bits(u["pwords"], n)
        paths.add(("union words", u["words"] is not None))
        paths.add(("parent words", u["pwords"] is not None))
        if u["pwords"] is not None and (uc._bits(u["words"], n) & ~uc._bits(u["pwords"], n)).any():
            paths.add("a NULL by the parent alone")
        if (~valid).any():
            paths.add("NULL union rows")
            assert (ur["type_ids"][~valid] == 0).all()
        if n > 2048 and not valid[2047] and not valid[2048]:
            paths.add("NULL rows across a tile seam")
        if n > 64 and not valid[63] and not valid[64]:
            paths.add("NULL rows across a word seam")
        for k, (mem, eff) in enumerate(zip(u["members"], ur["effective"])):
            paths.add(("member words", mem["words"] is not None))
            picked = valid & (u["tags"][:n] == k)
            if not picked.any() and n > 100:
                paths.add("a member never selected")
                assert not eff.any() and ur["members"][k]["nulls"] == n
            if picked.all() and n > 100:
                paths.add("all rows one member")
            if mem["words"] is not None:
                own = uc._bits(mem["words"], n)
                if (picked & ~own).any():
                    paths.add("a NULL of the selected member")
                if (own & ~picked).any():
                    paths.add("the member's own bit set on a row it does not own")
            paths.add(("kind", mem["kind"], bool(mem["large"])))
        bad = valid & (u["tags"][:n] >= u["m"])
        if bad.any():
            paths.add("a tag >= m under a valid row")
            assert ur["status"] == uc.ST_BAD_UNION_TAG and (ur["type_ids"][bad] == 0).all() and not any(e[bad].any() for e in ur["effective"])
        if ((u["tags"][:n] >= u["m"]) & ~valid).any() and not bad.any():
            paths.add("a tag >= m under a NULL row alone")
            assert ur["status"] == 0
        if n % 64:
            assert all(int(m[-1]) >> (n % 64) == (1 << (64 - n % 64)) - 1 for m in ur["masks"]), "pad bits ones"
    want = {("union words", True), ("union words", False), ("parent words", True), ("parent words", False), ("member words", True), ("member words", False),
            "a NULL by the parent alone", "NULL union rows", "NULL rows across a tile seam", "NULL rows across a word seam", "a member never selected",
            "all rows one member", "a NULL of the selected member", "the member's own bit set on a row it does not own", "a tag >= m under a valid row",
            "a tag >= m under a NULL row alone", ("kind", et.K_ENC_STR32, False), ("kind", et.K_ENC_STR32, True), ("kind", et.K_ENC_LIST32, False),
            ("kind", et.K_ENC_LIST32, True), ("kind", et.K_ENC_COPY, False), ("kind", uc.K_ENC_INTERVAL, False)}
    assert want <= paths, want - paths
    assert {u["name"] for u, _ in every} >= {"bad_tag/clean", "bad_tag/damaged"}


def test_constants_agree_with_the_header_and_the_binding():
    import os
    from duckdb_arrow_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "include", "mi_arrow_ipc.h")).read()
    for text in ("MI_K_ENC_INTERVAL = 41", "MI_K_ENC_UNION = 42", "#define MI_ST_BAD_UNION_TAG 8192u"):
        assert text in raw, text
    assert (_ffi.K_ENC_INTERVAL, _ffi.K_ENC_UNION) == (uc.K_ENC_INTERVAL, uc.K_ENC_UNION) == (41, 42)
    assert uc.MAX_MEMBERS == _ffi.MAX_UNION_MEMBERS and uc.ST_BAD_UNION_TAG == _ffi.ST_BAD_UNION_TAG

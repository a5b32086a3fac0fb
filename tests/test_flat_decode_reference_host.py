"""The reference of the flat decode tests (helpers.decode_column_reference, every decode kind), checked where it can be:
without a GPU.  Half floats against numpy, the kinds pyarrow can write against the oracle's stream decode and against
pyarrow's own values, array offsets against slices of the offset-0 decode, the parent mask against a loop over rows."""
import decimal

import numpy as np
import pytest

from oracle import pyoracle as po

from decode_tasks import FLAT_VARIANTS, VARIANTS, make_column
from helpers import _words_of, canon_oracle_column, canon_python, decode_column_reference, gather_reference, pyarrow_columns

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def test_half_floats_equal_numpy_for_all_65536_bit_patterns():
    """numpy converts float16 -> float32 exactly and keeps NaN payloads as sign | 0x7F800000 | man << 13."""
    h = np.arange(65536, dtype=np.uint16)
    data, ok, err = decode_column_reference(po.K_HALF_FLOAT, 65536, h)
    want = h.view(np.float16).astype(np.float32).view(np.uint32)
    nan = (h & 0x7C00 == 0x7C00) & (h & 0x3FF != 0)
    assert nan.sum() == 2046
    assert np.array_equal(want[nan], ((h[nan].astype(np.uint32) & 0x8000) << 16) | 0x7F800000 | ((h[nan].astype(np.uint32) & 0x3FF) << 13))
    assert np.array_equal(data.reshape(-1).view(np.uint32), want) and ok.all() and not err.any()


# ------------------------------------------------------------------------------------------------ pyarrow-written streams
N = 4500      # two record batches of 2250 rows: list columns get a second window inside a batch


def _table(views):
    """views False: every column but the string / binary views; True: those two alone"""
    import pyarrow as pa
    rng = np.random.default_rng(8)
    nul = lambda p=0.2: rng.random(N) < p
    i64 = lambda lo, hi: rng.integers(lo, hi, N)
    words = ["", "a", "twelve bytes", "thirteen byte", "a much longer string than fits inline"]
    strs = ["%s%d" % (words[int(k)], i) if k else "" for i, k in enumerate(rng.integers(0, len(words), N))]
    if views:
        return pa.table({"sv": pa.array(strs, pa.string_view(), mask=nul()), "bv": pa.array([s.encode() for s in strs], pa.binary_view(), mask=nul())})
    cols = {}
    for unit, lim in (("s", 9 * 10**12), ("ms", 9 * 10**15), ("us", 2**63 - 1), ("ns", 2**63 - 1)):
        v = i64(-lim, lim)
        v[:6] = [-1, -999, -1000, -1001, 999, lim]
        cols["dur_" + unit] = pa.array(v, pa.duration(unit), mask=nul())
    nanos = i64(-2**63, 2**63 - 1)
    nanos[:8] = [-1, -999, -1000, -1001, 999, 1000, -2**63, 2**63 - 1]
    mdn = [None if x else pa.MonthDayNano([int(m), int(d), int(ns)]) for x, m, d, ns in zip(nul(), i64(-2**31, 2**31), i64(-2**31, 2**31), nanos)]
    cols["mdn"] = pa.array(mdn, pa.month_day_nano_interval())
    dec = lambda digits, t: pa.array([None if x else decimal.Decimal(int(v)).scaleb(-t.scale) for x, v in zip(nul(), i64(-10**digits + 1, 10**digits))], t)
    small = hasattr(pa, "decimal32") and hasattr(pa, "decimal64")       # decimal32 / decimal64 where this pyarrow has them
    if small:
        cols["dec32_4"] = dec(4, pa.decimal32(4, 1))
        cols["dec64_4"] = dec(4, pa.decimal64(4, 2))
        cols["dec64_9"] = dec(9, pa.decimal64(9, 0))
    cols["f16"] = pa.array(rng.integers(0, 65536, N).astype(np.uint16).view(np.float16), mask=nul())
    lists = [None if x else [int(v) for v in rng.integers(-99, 99, int(k))] for x, k in zip(nul(), rng.choice([0, 0, 1, 2, 7, 30], N))]
    cols["list"] = pa.array(lists, pa.list_(pa.int32()))
    cols["large_list"] = pa.array(lists[::-1], pa.large_list(pa.int32()))
    cols["list_of_lists"] = pa.array([None if x else [lists[(i + j) % N] for j in range(i % 4)] for i, x in enumerate(nul())], pa.list_(pa.list_(pa.int32())))
    cols["null"] = pa.nulls(N)
    kids = [pa.array(i64(-2**31, 2**31).astype(np.int32), mask=nul()), pa.array(strs, mask=nul()), dec(4, pa.decimal128(4, 2)),
            pa.array(rng.random(N) < 0.5, mask=nul()), cols["dur_ms"]] + ([cols["dec32_4"]] if small else [])
    cols["struct"] = pa.StructArray.from_arrays(kids, names=["i", "s", "d", "b", "dur", "d32"][: len(kids)], mask=pa.array(nul()))
    fsl = lambda t, values: pa.FixedSizeListArray.from_arrays(values, type=pa.list_(values.type, 3), mask=pa.array(nul()))
    cols["fsl_i64"] = fsl(pa.int64(), pa.array(rng.integers(-2**62, 2**62, 3 * N), mask=rng.random(3 * N) < 0.2))
    cols["fsl_str"] = fsl(pa.string(), pa.array((strs * 3), mask=rng.random(3 * N) < 0.2))
    cols["fsl_dec"] = fsl(pa.decimal128(9, 2), pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**9 + 1, 10**9, 3 * N)],
                                                      pa.decimal128(9, 2), mask=rng.random(3 * N) < 0.2))
    return pa.table(cols)


def _trunc(v, d):
    return None if v is None else (abs(v) // d) * (1 if v >= 0 else -1)      # C division


def _expected(table):
    """pyarrow's to_pylist() of every column in canonical form; durations as stored microseconds, month_day_nano as
    [months, days, microseconds]"""
    import pyarrow as pa
    out = {}
    for name in table.schema.names:
        col, t = table.column(name).combine_chunks(), table.schema.field(name).type
        if pa.types.is_duration(t):
            mul, div = {"s": (10**6, 1), "ms": (1000, 1), "us": (1, 1), "ns": (1, 1000)}[t.unit]
            out[name] = [None if v is None else _trunc(v * mul, div) for v in col.cast(pa.int64()).to_pylist()]
        elif pa.types.is_interval(t):
            out[name] = [None if v is None else [v.months, v.days, _trunc(v.nanoseconds, 1000)] for v in col.to_pylist()]
        elif name == "struct":       # its duration child as above
            vals = pyarrow_columns(pa.table({name: pa.StructArray.from_arrays(
                [col.field(i) if col.type.field(i).name != "dur" else col.field(i).cast(pa.int64()) for i in range(col.type.num_fields)],
                names=[f.name for f in col.type], mask=col.is_null())}))[0]
            out[name] = [None if v is None else dict(v, dur=None if v["dur"] is None else v["dur"] * 1000) for v in vals]
        else:
            out[name] = pyarrow_columns(pa.table({name: col}))[0]
    return out


def _reference_node(a, body_off, node, parent=None):
    """The node with data and validity from decode_column_reference (row_offset 0) instead of the oracle's stream decode;
    asserts that the two are equal on the way."""
    spans, kind, n = node["buffers"], node["kind"], node["nrows"]
    buf = lambda k: a[body_off + spans[k][0]: body_off + spans[k][0] + spans[k][1]]
    args = dict(param=node["param"], null_count=node["null_count"], parent=parent)
    if spans and spans[0][1]:
        args["validity"] = buf(0)
    buf1 = buf(1) if len(spans) > 1 else None
    if kind == po.K_STRVIEW:
        args.update(buf2=np.array([[body_off + off, ln] for off, ln in spans[2:]], np.uint64).reshape(-1), buf2_len=len(spans) - 2)
    elif kind in (po.K_LIST32, po.K_LIST64):
        args.update(param=node["children"][0]["nrows"], window_starts=node["win"][:-1])
    elif kind in (po.K_STR32, po.K_STR64):
        args.update(buf2=buf(2), buf2_len=spans[2][1], ptr_base=node["ptr_base"])
    elif kind == po.K_FIXED_BINARY:
        args.update(ptr_base=node["ptr_base"])
    data, ok, err = decode_column_reference(kind, n, buf1, **args)
    assert not err.any(), node["name"]
    assert np.array_equal(data.reshape(-1), node["data"]), node["name"]
    assert np.array_equal(ok, po.valid_bits(node["validity"], n)), node["name"]
    words = _words_of(ok)
    if kind != po.K_NULL and n:
        assert np.array_equal(words, node["validity"]), (node["name"], "pad bits")
    out = dict(node, data=data.reshape(-1).copy(), validity=words if n else node["validity"])
    if kind == po.K_STRUCT:
        div = int(node["param"]) if node["field"]["type"] == po.T_FIXED_LIST else 1
        out["children"] = [_reference_node(a, body_off, c, parent=(node["validity"], div)) for c in node["children"]]
    else:
        out["children"] = [_reference_node(a, body_off, c) for c in node["children"]]
    return out


def _stream_equals_the_oracle_and_pyarrow(table):
    """-> the kinds met.  The reference at row_offset 0 is pyoracle.decode_stream, bytes and bits, and its canonical values
    are pyarrow's."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, table.schema) as w:
        w.write_table(table, max_chunksize=N // 2)
    a = np.frombuffer(sink.getvalue().to_pybytes(), np.uint8)
    fields, batches = po.decode_stream(a)
    assert len(batches) == 2
    kinds = set()
    got = {f["name"]: [] for f in fields}

    def note(node):
        kinds.add(node["kind"])
        for c in node["children"]:
            note(c)
    for b in batches:
        for f, node in zip(fields, b["columns"]):
            ref = _reference_node(a, b["body_off"], node)
            note(ref)
            got[f["name"]].extend(canon_oracle_column(f, ref, b["nrows"], a))
    want = _expected(table)
    for name in table.schema.names:
        assert canon_python(got[name]) == want[name], name
    return kinds


def test_reference_equals_the_stream_decode_of_the_oracle_and_pyarrow():
    """DURATION in all four units, month_day_nano, decimal32 / decimal64 (where this pyarrow has them), half floats, list,
    large_list, a list of lists (window starts inside tiles), null, and children of a struct and of fixed-size lists
    with parent NULLs.  (pyarrow cannot write the year_month interval of INTERVAL_MONTHS: see below.)"""
    import pyarrow as pa
    kinds = _stream_equals_the_oracle_and_pyarrow(_table(views=False))
    assert kinds >= {po.K_DURATION, po.K_INTERVAL_MDN, po.K_HALF_FLOAT, po.K_LIST32, po.K_LIST64, po.K_NULL, po.K_STRUCT}
    assert po.K_NARROW in kinds or not hasattr(pa, "decimal32")


def test_string_views_equal_the_stream_decode_of_the_oracle_and_pyarrow():
    import pyarrow as pa
    if not (hasattr(pa, "string_view") and hasattr(pa, "binary_view")):
        pytest.skip("this pyarrow has no string_view / binary_view type")
    assert _stream_equals_the_oracle_and_pyarrow(_table(views=True)) == {po.K_STRVIEW}


def test_gather_reference_refuses_exactly_the_kinds_a_selection_vector_cannot_take():
    """KindCanGather (kernels_gather.hip): COPY, DEC128, STR32, STR64, FIXED_BINARY, BOOL, DATE64, MUL_I32, MUL_I64, DIV_I64,
    DICT.  This pins helpers.GATHER_KINDS against a second hand-written copy of that list, not against the kernel: the
    kernel side is test_gather_tasks_the_plan_refuses and the per-kind plans of test_gpu_gather.py."""
    can = {po.K_COPY, po.K_DEC128, po.K_STR32, po.K_STR64, po.K_FIXED_BINARY, po.K_BOOL, po.K_DATE64, po.K_MUL_I32, po.K_MUL_I64, po.K_DIV_I64,
           po.K_DICT}
    assert {v["kind"] for v in VARIANTS.values()} == can
    rng = np.random.default_rng(1)
    seen = set()
    for variant in FLAT_VARIANTS:
        col = make_column(variant, 10, 3, "bitmap", rng)
        args = {k: col[k] for k in ("param", "param2", "validity", "null_count", "row_offset", "buf2", "buf2_len", "ptr_base") if k in col}
        seen.add(col["kind"])
        if col["kind"] in can:
            gather_reference(col["kind"], 10, col["buf1"], [np.arange(10)], **args)
        else:
            with pytest.raises(NotImplementedError, match="selection vector"):
                gather_reference(col["kind"], 10, col["buf1"], [np.arange(10)], **args)
    assert seen == set(range(po.K_COPY, po.K_STRUCT + 1))     # every decode kind was asked


def test_interval_months_is_the_month_count_and_twelve_zero_bytes():
    src = np.array([0, 1, -1, 2**31 - 1, -2**31, 14], np.int32)
    data, ok, err = decode_column_reference(po.K_INTERVAL_MONTHS, 5, src, row_offset=1, validity=np.array([0b101010], np.uint8))
    assert np.array_equal(data.view(np.int32), [[1, 0, 0, 0], [-1, 0, 0, 0], [2**31 - 1, 0, 0, 0], [-2**31, 0, 0, 0], [14, 0, 0, 0]])
    assert ok.tolist() == [True, False, True, False, True] and not err.any()      # NULL rows keep their source value, like upstream


# ------------------------------------------------------------------------------------------------ array offsets
NEW_VARIANTS = [v for v in FLAT_VARIANTS if v not in VARIANTS]


@pytest.mark.parametrize("variant", NEW_VARIANTS)
def test_array_offsets_give_the_rows_of_the_offset_0_decode(variant):
    """decode_column_reference(kind, n, buf, row_offset=o) = rows [o, o + n) of the decode at offset 0: data, validity bits
    and per-row status.  List entries are relative to their window, so there the offset-0 decode gets the windows of the
    sliced column (o, o + 2048, ...)."""
    rng = np.random.default_rng(NEW_VARIANTS.index(variant))
    n = 2500
    for o in (1, 33, 2051):
        col = make_column(variant, o + n, 0, "bitmap", rng)
        args = {k: col[k] for k in ("param", "validity", "null_count", "buf2", "buf2_len") if k in col}
        is_list = col["kind"] in (po.K_LIST32, po.K_LIST64)
        if is_list:
            args["param"] = int(col["buf1"][o + n]) - 3 * (o % 2)       # some rows end behind the child
        if col["kind"] == po.K_STRVIEW:
            col["buf1"].view(np.int32).reshape(-1, 4)[o + 7: o + 9, 3] = 5000      # valid or not: past every buffer
        wins = col.get("window_starts")
        whole = decode_column_reference(col["kind"], o + n, col["buf1"], **args,
                                        window_starts=(([0] if o > 0 else []) + list(o + (np.arange(0, n, 2048) if wins is None else wins))) if is_list else None)
        part = decode_column_reference(col["kind"], n, col["buf1"], row_offset=o, **args, window_starts=wins)
        for w, p, what in zip(whole, part, ("data", "validity", "status")):
            assert np.array_equal(w[o:], p), (variant, o, what)


# ------------------------------------------------------------------------------------------------ the parent mask
@pytest.mark.parametrize("div", [1, 3, 64])
def test_parent_mask_equals_a_loop_over_the_rows(div):
    rng = np.random.default_rng(div)
    parents = 300
    n = parents * div
    pwords = rng.integers(0, 256, (parents + 63) // 64 * 8, dtype=np.uint8).view(np.uint64)
    for variant in ("copy4", "dec128_i32", "narrow_8_2", "duration_mul_1e3", "duration_div_1000", "interval_mdn", "strview_1buf", "null", "struct"):
        for nulls in ("bitmap", "none"):
            col = make_column(variant, n, 5, nulls, rng, parent=(pwords, div))
            args = {k: col[k] for k in ("param", "validity", "null_count", "row_offset", "buf2", "buf2_len") if k in col}
            data, ok, err = decode_column_reference(col["kind"], n, col["buf1"], parent=(pwords, div), **args)
            own_data, own, _ = decode_column_reference(col["kind"], n, col["buf1"], **args)
            assert not err.any(), variant         # the rows the parent makes NULL hold offending values
            keeps = variant in ("copy4", "duration_div_1000", "interval_mdn")       # source-derived values under NULL
            for r in range(n):
                p = r // div
                want = bool(own[r]) and bool((int(pwords[p >> 6]) >> (p & 63)) & 1)
                assert ok[r] == want, (variant, r)
                if want or keeps:
                    assert np.array_equal(data[r], own_data[r]), (variant, r)
                else:
                    assert not data[r].any(), (variant, r)

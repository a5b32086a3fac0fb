"""Late materialisation (kernels_gather.hip) against the flat decode: every gather task kind through the kernel-level ABI
(mi_col_task.sel / sel_count) and every gatherable Arrow type through the scan operator's filter_compact.

Reference (helpers.gather_reference, checked without a GPU in test_gather_reference_host.py): the oracle decodes the
whole column, numpy takes rows 2048 * w + sel[w][i] and packs them.  NULL slots are compared too: no kind needed masking,
the kernel's NULL slots are the oracle's for every kind (source bytes for COPY / BOOL / DATE64 / DIV_I64, canonical
zero -- dict_len for DICT -- for the others).

Buffers follow the host's contract (ArrowScan::EnqueueStageB): 2048 sel slots per window of which the first count[w] mean
something, validity preset to ones for ceil(total / 64) words plus one guard word.  On top of that the output is filled
with a sentinel and over-allocated, and the unused sel slots hold 2048: a row of the NEXT window.  Every source buffer
is generated PAD_ROWS rows longer than the column, so a kernel that did follow such a slot would read defined bytes of
the same allocation and show up as a wrong value, never as an access outside the buffers."""
import decimal

import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

from decode_tasks import (ONES, PAD_ROWS, PTR_BASE, SEL_FILL, SENTINEL, STATUS_CASES, VARIANTS, WIN, _sel_arrays, _status_column, _width,
                          check_job, make_column, make_sel, run_plan)
from helpers import canon_python, gather_take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def con():
    return da.Connection(0)


# ------------------------------------------------------------------------------------------------ every kind
ROW_OFFSETS = [0, 1, 7, 13, 64, 2051]
# per-window counts by row count, one pattern per row offset: together 0, 1, 63, 64, 65, 255, 256, 257, 2047 and 2048 rows in a window
# (the seams of gather_rows: one wave, one pass of 256 lanes, several passes); the short last window is fully selected
COUNT_PATTERNS = {
    1: [[None]] * 6,
    2047: [[None]] * 6,
    2048: [[2048], [1], [63], [64], [65], [255]],
    2049: [[256, None], [257, None], [2047, None], [0, None], [2048, None], [1, None]],
    5000: [[0, 2048, None], [1, 63, None], [64, 65, None], [255, 256, None], [257, 2047, None], [2048, 0, None]],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_kind_equals_the_flat_decode(ctx, torch, variant):
    """One plan per kind variant: 5 row counts x 6 array offsets x 3 validity forms = 90 gather tasks over 30 selections.
    Data rows, sentinel tail, validity words with pad bits and the guard word of every task, and status 0 (the NULL rows
    of the bitmap form hold out-of-range values that must not be looked at)."""
    rng = np.random.default_rng(sorted(VARIANTS).index(variant))
    jobs, sels = [], {}
    for nrows, patterns in COUNT_PATTERNS.items():
        for row_offset, counts in zip(ROW_OFFSETS, patterns):
            sels[(nrows, row_offset)] = make_sel(nrows, counts, rng)
            for nulls in ("bitmap", "count0", "none"):
                jobs.append((make_column(variant, nrows, row_offset, nulls, rng), (nrows, row_offset)))
    got, status = run_plan(ctx, torch, jobs, sels)
    for (col, key), g in zip(jobs, got):
        assert check_job(col, sels[key], g) == 0, col["name"]
    assert status == 0


WINDOW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 0, 0, 2048, 2048, 1, None]


@pytest.mark.parametrize("variant", ["copy4", "dec128_i64", "str32", "bool", "dict_i32"])
def test_window_counts_at_the_loop_seams_in_one_column(ctx, torch, variant):
    """All the seam counts in consecutive windows of ONE column, so every window's output range starts at an odd position
    left by the windows before it (window_base) and shares validity words with its neighbours."""
    rng = np.random.default_rng(77)
    nrows = (len(WINDOW_COUNTS) - 1) * WIN + 77
    sel = make_sel(nrows, WINDOW_COUNTS, rng)
    col = make_column(variant, nrows, 13, "bitmap", rng)
    got, status = run_plan(ctx, torch, [(col, "s")], {"s": sel})
    assert check_job(col, sel, got[0]) == 0 and status == 0


def test_single_rows_of_many_windows_share_validity_words(ctx, torch):
    """150 windows with one selected row each, alternately NULL: 64 windows clear their bit of one output word, each with
    its own atomicAnd.  Then the same with 65 rows per window, where every wave's word straddles two output words."""
    rng = np.random.default_rng(5)
    nw = 150
    nrows = nw * WIN
    jobs, sels = [], {}
    for name, per in (("one", 1), ("sixty-five", 65)):
        sel = [np.sort(rng.choice(WIN, per, replace=False)).astype(np.int64) for _ in range(nw)]
        col = make_column("copy8", nrows, 3, "bitmap", rng)
        bits = np.unpackbits(col["validity"], bitorder="little")
        for w, s in enumerate(sel):
            bits[3 + w * WIN + s] = (w + np.arange(per)) % 2      # alternately NULL along the output
        col["validity"] = np.packbits(bits, bitorder="little")
        jobs.append((col, name))
        sels[name] = sel
    got, status = run_plan(ctx, torch, jobs, sels)
    for (col, key), g in zip(jobs, got):
        check_job(col, sels[key], g)
        if key == "one":
            assert g[1][0] == np.uint64(0xAAAAAAAAAAAAAAAA) and g[1][1] == np.uint64(0xAAAAAAAAAAAAAAAA)
    assert status == 0


def test_long_column_runs_the_carry_loop_of_the_window_bases(ctx, torch):
    """2 * 2048 + 3 windows (8.4 M rows): gather_window_bases scans 2048 windows per step, so this column takes two full
    steps and a partial third, with the carry handed from step to step.  A COPY 1 and a COPY 8 task with NULLs share the
    selection; the counts vary and include runs of empty and of full windows, also across the step boundaries."""
    rng = np.random.default_rng(9)
    nw = 2 * 2048 + 3
    nrows = nw * WIN - 1000
    p = rng.choice([0.0, 0.003, 0.05, 0.4, 1.0], nw, p=[0.2, 0.3, 0.2, 0.2, 0.1])
    p[100:140], p[140:170] = 0.0, 1.0
    p[2040:2047], p[2047:2050], p[4090:4096] = 1.0, 0.0, 1.0
    p[-3:] = [0.0, 0.5, 1.0]
    keep = rng.random(nw * WIN, dtype=np.float32) < np.repeat(p, WIN).astype(np.float32)
    keep[nrows:] = False
    rows = np.nonzero(keep)[0]
    counts = np.bincount(rows >> 11, minlength=nw)
    assert counts.max() == WIN and counts.min() == 0 and counts[-1] == WIN - 1000
    starts = np.concatenate([[0], np.cumsum(counts)])
    flat = np.full(nw * WIN, SEL_FILL, np.uint32)
    flat[(rows >> 11) * WIN + (np.arange(len(rows)) - starts[rows >> 11])] = rows & 2047
    sel = np.split(rows & 2047, starts[1:-1])
    assert np.array_equal(_sel_arrays(sel)[0], flat)
    cols = [make_column("copy1", nrows, 5, "bitmap", rng), make_column("copy8", nrows, 2051, "bitmap", rng)]
    got, status = run_plan(ctx, torch, [(c, "s") for c in cols], {"s": sel})
    for col, g in zip(cols, got):
        w, o = _width(col), col["row_offset"]
        src = col["buf1"].reshape(-1, w)[o: o + nrows]
        ok = np.unpackbits(col["validity"], bitorder="little")[o: o + nrows].astype(bool)
        want = gather_take(src, ok, np.zeros(nrows, np.uint32), sel)     # COPY: the source bytes (helpers.decode_column_reference)
        check_job(col, sel, g, want=want)
    assert status == 0


# ------------------------------------------------------------------------------------------------ plans
def test_plan_with_gather_tasks_over_two_selections_and_flat_tasks(ctx, torch):
    """window_base is indexed by the tile inside the gather slice: four gather tasks (two selections of different row
    counts, a task of one selection between two of the other) and two ordinary tasks in one plan give what each gives in
    a plan of its own."""
    rng = np.random.default_rng(21)
    na, nb = 3 * WIN + 500, 5 * WIN + 1
    sels = {"a": make_sel(na, [700, 0, 2048, None], rng), "b": make_sel(nb, [1, 2047, 65, 0, 300, None], rng)}
    jobs = [(make_column("str32", na, 7, "bitmap", rng), "a"), (make_column("copy2", nb, 0, "none", rng), None),
            (make_column("dec128_i32", nb, 64, "bitmap", rng), "b"), (make_column("bool", na, 13, "bitmap", rng), "a"),
            (make_column("dict_u16", nb, 1, "bitmap", rng), None), (make_column("fixed13", nb, 2051, "count0", rng), "b")]
    got, status = run_plan(ctx, torch, jobs, sels)
    assert status == 0
    for (col, key), g in zip(jobs, got):
        check_job(col, sels[key] if key else None, g)
        alone, st = run_plan(ctx, torch, [(col, key)], {key: sels[key]} if key else {})
        assert st == 0 and np.array_equal(alone[0][0], g[0]) and np.array_equal(alone[0][1], g[1]), col["name"]


@pytest.mark.parametrize("variant", ["copy8", "str64", "dec128_i16", "dict_i8"])
def test_nothing_selected_and_empty_columns_write_nothing(ctx, torch, variant):
    rng = np.random.default_rng(2)
    sels = {"none": make_sel(5000, [0], rng), "empty": []}
    jobs = [(make_column(variant, 5000, 7, "bitmap", rng), "none"), (make_column(variant, 0, 0, "bitmap", rng), "empty")]
    got, status = run_plan(ctx, torch, jobs, sels)
    for (col, key), (data, words) in zip(jobs, got):
        check_job(col, sels[key], (data, words))
        assert (data == SENTINEL).all() and len(words) == 1 and words[0] == ONES
    assert status == 0


# ------------------------------------------------------------------------------------------------ status
BAD_ROWS = [0, 70, WIN + 255, 2 * WIN + 99]       # lane 0 of a wave, inside a wave, second pass of a window, last window


@pytest.mark.parametrize("case", list(STATUS_CASES))
def test_value_checks_look_at_selected_valid_rows_only(ctx, torch, case):
    """DECIMAL_RANGE / MUL_OVERFLOW / INDEX_RANGE / DICT_INDEX: raised when the offending row is selected and valid, not
    raised when it is unselected, and not raised when it is selected but NULL.  Data (the DICT slot holds dict_len) and
    validity equal the reference in all three."""
    make, flag, _ = STATUS_CASES[case]
    rng = np.random.default_rng(3)
    nrows = 2 * WIN + 100
    for bad_row in BAD_ROWS:
        w, r = divmod(bad_row, WIN)
        with_row = make_sel(nrows, [300, 300, None], rng)
        if r not in with_row[w]:
            with_row[w] = np.sort(np.concatenate([with_row[w][:-2], [r], with_row[w][-1:]]))
        without = [s[s != r] if i == w else s for i, s in enumerate(with_row)]
        col = _status_column(make, bad_row, nrows, rng)
        col["name"] = "%s/row%d" % (case, bad_row)
        null = dict(col, validity=col["validity"].copy())
        null["validity"][bad_row >> 3] &= 0xFF ^ (1 << (bad_row & 7))
        for c, sel, want in ((col, with_row, flag), (col, without, 0), (null, with_row, 0)):
            got, status = run_plan(ctx, torch, [(c, "s")], {"s": sel})
            assert check_job(c, sel, got[0]) == want, c["name"]
            assert status == want, (c["name"], status)


def _strings(kind, nrows, rng, long_row):
    lens = rng.choice([0, 3, 12, 13, 30], nrows + PAD_ROWS)
    lens[long_row] = 13                                  # the row to damage is not empty: no other row ends where it ends
    off = 5 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int32 if kind == _ffi.K_STR32 else np.int64)
    return dict(kind=kind, buf1=off, buf2=rng.integers(1, 256, int(off[-1]), dtype=np.uint8), buf2_len=int(off[nrows]), nrows=nrows, row_offset=0,
                validity=rng.integers(0, 256, (nrows + PAD_ROWS + 63) // 64 * 8 + 8, dtype=np.uint8), null_count=-1, ptr_base=PTR_BASE)


@pytest.mark.parametrize("kind,damage", [(_ffi.K_STR32, "decreasing"), (_ffi.K_STR32, "past_the_data"), (_ffi.K_STR64, "decreasing"),
                                         (_ffi.K_STR64, "past_the_data"), (_ffi.K_STR64, "too_large")],
                         ids=["str32-decreasing", "str32-past_the_data", "str64-decreasing", "str64-past_the_data", "str64-too_large"])
def test_offsets_are_validated_for_selected_rows_only(ctx, torch, kind, damage):
    """Only the rows the selection names are read, so only they are validated (kernels_gather.hip, gather_string): a
    damaged offset raises BAD_OFFSETS / STRING_TOO_LARGE when its row is selected -- NULL or not, like the flat kernel --
    and nothing when it is not; the damaged row decodes to 16 zero bytes.  No selected row has an offset outside the
    payload that the kernel would follow: end < start and end > buf2_len are refused by the kernel's own bound check
    before any payload byte is read, and an end offset past 4 GB is refused before the payload is touched as well."""
    rng = np.random.default_rng(4)
    nrows = 2 * WIN + 100
    for bad_row in BAD_ROWS:
        col = _strings(kind, nrows, rng, bad_row)
        col["name"] = "%s/row%d" % (damage, bad_row)
        w, r = divmod(bad_row, WIN)
        flag = _ffi.ST_BAD_OFFSETS
        if damage == "decreasing":
            col["buf1"][bad_row + 1] = col["buf1"][bad_row] - 1                  # ends before it starts; the next row starts early, which is legal
        elif damage == "past_the_data":
            col["buf2_len"] = int(col["buf1"][bad_row + 1]) - 1                  # this row and every later one end past the data
        else:
            col["buf1"][bad_row + 1:] += 2**32                                   # this row and every later one end past 4 GB ...
            col["buf2_len"] = 2**33                                              # ... of a payload said to be that long: no payload byte of them is read
            flag = _ffi.ST_STRING_TOO_LARGE
        with_row = make_sel(nrows, [300, 300, None], rng)
        if r not in with_row[w]:
            with_row[w] = np.sort(np.concatenate([with_row[w][:-2], [r], with_row[w][-1:]]))
        if damage != "decreasing":                                                # rows behind the damaged one are damaged too
            with_row = [s[s <= r] if i == w else (s if i < w else s[:0]) for i, s in enumerate(with_row)]
        without = [s[s != r] if i == w else s for i, s in enumerate(with_row)]
        for sel, want in ((with_row, flag), (without, 0)):
            got, status = run_plan(ctx, torch, [(col, "s")], {"s": sel})
            assert check_job(col, sel, got[0]) == want, col["name"]
            assert status == want, (col["name"], status)


def test_gather_tasks_the_plan_refuses(ctx):
    """ValidateTask; nothing is launched (the addresses are made up)."""
    ok = dict(param=8, sel=4096, sel_count=8192)
    da.Plan(ctx, [da.make_task(_ffi.K_COPY, 0, 16, 32, **ok)])
    for match, kw, kind in (("need sel_count", dict(ok, sel_count=0), _ffi.K_COPY),
                            ("cannot be decoded through a selection vector", dict(ok, param=1000), _ffi.K_DURATION),
                            ("cannot be decoded through a selection vector", dict(ok, param=4 | (2 << 8)), _ffi.K_NARROW),
                            ("cannot be decoded through a selection vector", dict(ok), _ffi.K_STRVIEW),
                            ("top-level columns", dict(ok, out_aux=64), _ffi.K_COPY),
                            ("top-level columns", dict(ok, depth=1), _ffi.K_COPY),
                            ("selection vector misaligned", dict(ok, sel=4098), _ffi.K_COPY),
                            ("selection vector misaligned", dict(ok, sel_count=8194), _ffi.K_COPY)):
        with pytest.raises(da.MiError, match=match):
            da.Plan(ctx, [da.make_task(kind, 10, 16, 32, **kw)])


# ------------------------------------------------------------------------------------------------ the scan operator
N_TABLE = 9000


def _table():
    """A column of every Arrow type the planner decodes with a gatherable kind, each with NULLs, and a row id."""
    import pyarrow as pa
    rng = np.random.default_rng(31)
    n = N_TABLE
    nul = lambda p=0.15: rng.random(n) < p
    ints = lambda lo, hi, dt: rng.integers(lo, hi, n).astype(dt)
    dec = lambda digits, p, s: pa.array([None if x else decimal.Decimal(int(v)).scaleb(-s) for x, v in zip(nul(), rng.integers(
        -10**digits + 1, 10**digits, n))], pa.decimal128(p, s))
    words = ["", "a", "twelve bytes", "thirteen byte", "a much longer string than fits inline"]
    strs = ["%s%d" % (words[int(k)], i) if k else "" for i, k in enumerate(rng.integers(0, len(words), n))]
    f32 = rng.standard_normal(n).astype(np.float32)
    f32[:4] = [np.inf, -np.inf, -0.0, np.nan]
    cols = {
        "k": pa.array(np.arange(n, dtype=np.int64)),
        "i8": pa.array(ints(-128, 128, np.int8), mask=nul()), "u8": pa.array(ints(0, 256, np.uint8), mask=nul()),
        "i16": pa.array(ints(-2**15, 2**15, np.int16), mask=nul()), "i32": pa.array(ints(-1000, 1000, np.int32), mask=nul(0.2)),
        "i64": pa.array(ints(-2**62, 2**62, np.int64), mask=nul()), "u64": pa.array(ints(0, 2**63, np.uint64), mask=nul()),
        "f32": pa.array(f32, mask=nul()), "f64": pa.array(rng.standard_normal(n), mask=nul()),
        "flag": pa.array(rng.random(n) < 0.5, mask=nul(0.3)),
        "d32": pa.array(ints(-20000, 40000, np.int32), pa.date32(), mask=nul()),
        "d64": pa.array(ints(-20000, 40000, np.int64) * 86400000, pa.date64(), mask=nul()),
        "t32s": pa.array(ints(0, 86400, np.int32), pa.time32("s"), mask=nul()),
        "t32ms": pa.array(ints(0, 86400000, np.int32), pa.time32("ms"), mask=nul()),
        "t64us": pa.array(ints(0, 86400 * 10**6, np.int64), pa.time64("us"), mask=nul()),
        "t64ns": pa.array(ints(0, 86400 * 10**9, np.int64), pa.time64("ns"), mask=nul()),
        "ts_s": pa.array(ints(-2**31, 2**32, np.int64), pa.timestamp("s", tz="UTC"), mask=nul()),
        "ts_ms": pa.array(ints(-2**41, 2**42, np.int64), pa.timestamp("ms", tz="UTC"), mask=nul()),
        "ts_us": pa.array(ints(-2**51, 2**52, np.int64), pa.timestamp("us", tz="UTC"), mask=nul()),
        "ts_ns": pa.array(ints(-2**61, 2**62, np.int64), pa.timestamp("ns", tz="UTC"), mask=nul()),
        "ts_plain": pa.array(ints(-2**51, 2**52, np.int64), pa.timestamp("ms"), mask=nul()),
        "dec4": dec(4, 4, 1), "dec9": dec(9, 9, 2), "dec18": dec(18, 18, 0), "dec30": dec(18, 30, 3),
        "s": pa.array(strs, mask=nul(0.25)), "ls": pa.array(strs[::-1], pa.large_string(), mask=nul(0.25)),
        "bin": pa.array([s.encode() for s in strs], pa.binary(), mask=nul()),
        "fsb": pa.array([bytes(r) for r in rng.integers(0, 256, (n, 13), dtype=np.uint8)], pa.binary(13), mask=nul()),
        "dict": pa.DictionaryArray.from_arrays(pa.array(ints(0, 5, np.int8), mask=nul()), pa.array(words[1:] + ["zz"])),
    }
    return pa.table(cols)


def _stored(table):
    """pyarrow's values of every column in the form the Python binding returns: stored integers in DuckDB's unit for
    temporal and decimal types."""
    import pyarrow as pa
    import pyarrow.compute as pc
    trunc = lambda c, d: pc.multiply(pc.sign(c), pc.divide(pc.abs(c), d))       # C division, not floor
    out = []
    for f in table.schema:
        c, t = table.column(f.name).combine_chunks(), f.type
        if pa.types.is_dictionary(t):
            c = c.cast(t.value_type)
        elif pa.types.is_date32(t):
            c = c.cast(pa.int32())
        elif pa.types.is_date64(t):
            c = trunc(c.cast(pa.int64()), 86400000)
        elif pa.types.is_time(t) or pa.types.is_timestamp(t):
            c = c.cast(pa.int32() if pa.types.is_time32(t) else pa.int64()).cast(pa.int64())
            plain = pa.types.is_timestamp(t) and t.tz is None                    # stays in its own unit (TIMESTAMP_S / _MS / _NS)
            c = c if plain else {"s": lambda: pc.multiply(c, 1000000), "ms": lambda: pc.multiply(c, 1000), "us": lambda: c,
                                 "ns": lambda: trunc(c, 1000)}[t.unit]()
        vals = c.to_pylist()
        if pa.types.is_decimal(t):
            vals = [None if v is None else int(v.scaleb(t.scale)) for v in vals]
        out.append(canon_python(vals))
    return out


def _write_table(table, path, codec=None):
    import pyarrow.ipc as ipc
    opts = ipc.IpcWriteOptions(compression=codec) if codec else None
    with ipc.new_stream(path, table.schema, options=opts) as w:
        w.write_table(table, max_chunksize=N_TABLE // 3)
    return path


@pytest.fixture(scope="module")
def table_file(tmp_path_factory):
    t = _table()
    return t, _write_table(t, str(tmp_path_factory.mktemp("gather") / "t.arrows"))


def _i32_mask(t, f):
    col = t.column("i32").combine_chunks()
    return f(np.asarray(col.fill_null(0))) & ~np.asarray(col.is_null())


PREDICATES = {
    "none_pass": (("i32", "<", -5000), lambda t: _i32_mask(t, lambda v: v < -5000)),
    "all_pass": (("k", ">=", 0), lambda t: np.ones(N_TABLE, bool)),
    "one_percent": (("i32", "<", -975), lambda t: _i32_mask(t, lambda v: v < -975)),
    "half": (("i32", ">=", 0), lambda t: _i32_mask(t, lambda v: v >= 0)),
    # record batch 1 holds rows 3000 .. 5999: its first window passes whole, every other window of the file is empty
    "one_full_window": (("and", ("k", ">=", 3000), ("k", "<", 3000 + WIN)), lambda t: (np.arange(N_TABLE) >= 3000) & (np.arange(N_TABLE) < 3000 + WIN)),
}


def _scan_equals_pyarrow(con, t, path, name):
    import pyarrow as pa
    expr, mask_of = PREDICATES[name]
    mask = mask_of(t)
    names = t.schema.names
    flat, compact = (canon_python(con.read_arrow(path, filter_compact=c, accept_dictionaries=True).project(names).filter(expr).fetch_columns())
                     for c in (False, True))
    want = _stored(t.filter(pa.array(mask)))
    assert compact[0] == np.nonzero(mask)[0].tolist()
    for nm, c, f, w in zip(names, compact, flat, want):
        assert c == f, nm
        assert c == w, nm


@pytest.mark.parametrize("name", list(PREDICATES))
def test_compacted_scan_equals_the_selection_vector_scan_for_every_type(con, table_file, name):
    """read_arrow(filter_compact=True) returns, column by column, what filter_compact=False returns for the same filter,
    and both return pyarrow's filtered table; the row ids are numpy's."""
    t, path = table_file
    _scan_equals_pyarrow(con, t, path, name)


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_compacted_scan_of_a_compressed_body(con, table_file, tmp_path, codec):
    """The gather kernel reads a body that was decompressed in HBM."""
    t, _ = table_file
    _scan_equals_pyarrow(con, t, _write_table(t, str(tmp_path / "z.arrows"), codec), "half")


@pytest.mark.parametrize("device_resident", [False, True], ids=["host", "device_resident"])
def test_compacted_scan_with_a_column_absent_from_the_second_file(con, tmp_path, device_resident):
    """filter_compact with union_by_name over two files, the second without column `x`: both stages plan the output columns
    (stage A when a batch is empty, stage B for the rows that survived) and zero the absent column's all-NULL vector.  Three
    record batches of 5000 rows per file -- three windows, the last one ragged -- of which the first keeps every row, the
    second none and the third about half; equal to pyarrow's reading of the two files, a host consumer and vectors in HBM."""
    import ctypes as C
    import pyarrow as pa
    import pyarrow.ipc as ipc
    from helpers import pyarrow_columns
    from test_gpu_scan_operator import _mirror_device_vector
    rng = np.random.default_rng(41)
    rows, tables, paths = 5000, [], []
    for fi in range(2):
        n = 3 * rows
        keep = np.concatenate([np.ones(rows, np.int8), np.zeros(rows, np.int8), (rng.random(rows) < 0.5).astype(np.int8)])
        cols = {"k": pa.array(np.arange(n, dtype=np.int64) + fi * n), "keep": pa.array(keep),
                "s": pa.array(["row %d %s" % (i, "long enough to leave the inline form" * (i % 3)) for i in range(n)], mask=rng.random(n) < 0.1),
                "v": pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=rng.random(n) < 0.2)}
        if fi == 0:
            cols["x"] = pa.array(rng.integers(0, 1 << 40, n), mask=rng.random(n) < 0.3)
        t = pa.table(cols)
        p = str(tmp_path / ("f%d.arrows" % fi))
        with ipc.new_stream(p, t.schema) as w:
            w.write_table(t, max_chunksize=rows)
        tables.append(t)
        paths.append(p)
    names = ["k", "x", "s", "v"]
    whole = pa.concat_tables([tables[0], tables[1].append_column("x", pa.nulls(3 * rows, pa.int64()))]).select(names + ["keep"])
    want = pyarrow_columns(whole.filter(pa.array(np.asarray(whole.column("keep")) == 1)).select(names))
    assert len(want[0]) > 2 * rows and want[1][-1] is None
    rel = con.read_arrow(paths, union_by_name=True, filter_compact=True, device_resident=device_resident).project(names).filter(("keep", "=", 1))
    if not device_resident:
        assert canon_python(rel.fetch_columns()) == want
        return
    hip = C.CDLL("libamdhip64.so")
    types = [da.parse_duck_type(x) for x in rel.types]
    got = [[] for _ in types]
    for ch in rel.chunks():
        held = []
        for ci, ty in enumerate(types):
            got[ci].extend(da._vector_values(_mirror_device_vector(hip, ch.columns[ci], ty, ch.size, held), ty, ch.size))
    assert canon_python(got) == want


def test_compacted_scan_reports_what_the_gather_kernel_found(con, tmp_path):
    """The status word of stage B's gather plan travels home beside stage A's: a string column with one decreasing offset,
    projected but not filtered on, is decoded by the gather kernel alone when the scan compacts -- the scan fails as the
    selection-vector scan of the same file does, and the undamaged twin reads."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    n = 3000
    t = pa.table({"k": pa.array(np.arange(n, dtype=np.int64)), "s": pa.array(["value %d of a string column" % i for i in range(n)])})
    good = str(tmp_path / "good.arrows")
    with ipc.new_stream(good, t.schema) as w:
        w.write_table(t)
    raw = bytearray(open(good, "rb").read())
    offsets = np.asarray(t.column("s").chunk(0).buffers()[1]).view(np.int32)[: n + 1].copy()
    at = bytes(raw).find(offsets.tobytes())
    assert at > 0 and bytes(raw).find(offsets.tobytes(), at + 1) < 0
    offsets[1500] = offsets[1501] + 7            # row 1499 ends behind the start of row 1501: row 1500 has a negative length
    raw[at: at + 4 * (n + 1)] = offsets.tobytes()
    bad = str(tmp_path / "bad.arrows")
    open(bad, "wb").write(bytes(raw))
    scan = lambda path, compact: con.read_arrow(path, filter_compact=compact).project(["k", "s"]).filter(("k", ">=", 1000)).fetch_columns()
    assert scan(good, True) == scan(good, False) and len(scan(good, True)[0]) == 2000
    with pytest.raises(da.MiError) as flat:
        scan(bad, False)
    with pytest.raises(da.MiError) as compact:
        scan(bad, True)
    assert str(compact.value) == str(flat.value) and compact.value.code == flat.value.code

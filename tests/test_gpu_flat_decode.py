"""The flat decode kernels (kernels_decode.hip) at the task level, every decode kind against the oracle's per-kind
functions (helpers.decode_column_reference, checked without a GPU in test_flat_decode_reference_host.py).

Per task (decode_tasks.check_job): every data row equals the reference, NULL slots included; the sentinel bytes behind
the last row are untouched; the validity words equal the reference, pad bits ones (the Arrow null type: zero words, like
the oracle's memset); the guard word behind them is intact.  Per plan: the status is the OR of the per-row bits of the
reference over all its tasks; where a flag is expected the plan holds one task, so the task's status is the plan's.

The shapes follow the loops of the kernels: light_map moves 4 rows per lane and 256 per pass in groups of 4 or 8 passes
with a scalar tail; validity arrives as 32-bit dwords (misc_light) or 64-bit words (the others), realigned when
(row_offset + row0) is no multiple of 32 / 64, with a guarded read of the next word; dec128 runs in groups of 1024 rows;
the string kernel takes off[r + 1] from the neighbour lane except at lane 63 and at the last row; tiles are 2048 rows."""
import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

from decode_tasks import (FLAT_VARIANTS, I64_MAX, ONES, PAD_ROWS, STATUS_CASES, VIEW_BASE, WIN, _status_column, check_job, flat_reference,
                          make_column, run_plan)

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
ROW_OFFSETS = [0, 1, 7, 13, 31, 32, 33, 63, 64, 2051]
AT_EVERY_OFFSET = (65, 1025, 2049)


def _shapes():
    """(row count, array offset): every row count at three offsets at least -- two of the first nine in rotation, of which
    one at least is no multiple of 32, and 2051, which is >= 64 and a multiple of neither 32 nor 64 --, the row counts 65,
    1025 and 2049 at every offset."""
    shapes = []
    for i, n in enumerate(ROW_COUNTS):
        offsets = ROW_OFFSETS if n in AT_EVERY_OFFSET else [ROW_OFFSETS[i % 9], ROW_OFFSETS[(i + 2) % 9], 2051]
        shapes += [(n, o) for o in offsets]
    return shapes


SHAPES = _shapes()
for _n in ROW_COUNTS:      # the rotation gives every row count a second offset that is no multiple of 32, beside 2051
    _offs = [o for n, o in SHAPES if n == _n]
    assert len(set(_offs)) >= 3 and sum(1 for o in set(_offs) if o % 32) >= 2 and any(o >= 64 and o % 64 for o in _offs)
for _o in ROW_OFFSETS:
    assert {n for n, o in SHAPES if o == _o} >= set(AT_EVERY_OFFSET)


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run_and_check(ctx, torch, cols, **kw):
    """One plan of ordinary flat tasks; every task against the reference, the plan's status against the OR of theirs."""
    got, status = run_plan(ctx, torch, [(c, None) for c in cols], {}, **kw)
    want_status = 0
    for col, g in zip(cols, got):
        want_status |= check_job(col, None, g, want=flat_reference(col))
    assert status == want_status, (status, want_status)
    return got, status


# ------------------------------------------------------------------------------------------------ every kind, every seam
def seam_columns(variant, rng):
    cols = []
    for n, o in SHAPES:
        forms = ["bitmap", "count0", "none"] + (["all_valid", "all_null"] if n in (65, 2049) else [])
        cols += [make_column(variant, n, o, nulls, rng) for nulls in forms]
    return cols


N_SEAM_TASKS = sum(3 + (2 if n in (65, 2049) else 0) for n, o in SHAPES)       # 81 shapes: 283 tasks per variant


@pytest.mark.parametrize("variant", list(FLAT_VARIANTS))
def test_every_kind_at_the_loop_seams(ctx, torch, variant):
    """One plan per variant: 20 row counts x 3 or 10 array offsets x the validity forms bitmap / count0 / none (and an
    all-valid and an all-NULL bitmap for 65 and 2049 rows) = 283 tasks.  Status 0: the NULL rows hold values that would raise
    a flag (or, for string views, a buffer index of -1) if they were looked at."""
    rng = np.random.default_rng(1000 + sorted(FLAT_VARIANTS).index(variant))
    cols = seam_columns(variant, rng)
    assert len(cols) == N_SEAM_TASKS == 283
    _, status = _run_and_check(ctx, torch, cols)
    assert status == 0


def test_half_float_column_of_all_65536_bit_patterns(ctx, torch):
    """Zeros, subnormals (the clz path), normals, infinities and all 2046 NaN payloads, at array offsets 0 and 13."""
    rng = np.random.default_rng(16)
    cols = []
    for o in (0, 13):
        col = make_column("half_float", 65536, o, "bitmap", rng)
        col["buf1"] = ((np.arange(len(col["buf1"])) - o) & 0xFFFF).astype(np.uint16)
        cols.append(col)
    _, status = _run_and_check(ctx, torch, cols)
    assert status == 0


# ------------------------------------------------------------------------------------------------ children
def _parent_words(rows, rng):
    """random validity words of a parent vector of `rows` rows, and two words more: the fixed-size-list paths rebuild whole
    64-bit child words, so they look at parent rows up to 63 / div behind the last one"""
    return rng.integers(0, 256, ((rows + 63) // 64 + 2) * 8, dtype=np.uint8).view(np.uint64)


def struct_child_columns(variant, rng):
    cols = []
    for n, o in zip((65, 2049, 4099, 65, 2049, 4099), (0, 13, 2051, 2051, 0, 13)):
        for div in (0, 1):
            for nulls in ("bitmap", "none"):
                cols.append(make_column(variant, n, o, nulls, rng, parent=(_parent_words(n, rng), div)))
    return cols


def list_child_columns(variant, rng):
    cols = []
    for div in (2, 3, 64, 100):
        for k, parents in enumerate((1, 33, 700)):
            for nulls in ("bitmap", "none"):
                cols.append(make_column(variant, parents * div, (0, 13)[(k + div) % 2], nulls, rng, parent=(_parent_words(parents, rng), div)))
    return cols


@pytest.mark.parametrize("variant", list(FLAT_VARIANTS))
def test_children_of_structs_and_the_parent_word(ctx, torch, variant):
    """out_aux = the parent's validity words, rows per parent row 0 and 1, depth 1: 24 tasks per variant (65, 2049 and 4099
    rows at offsets 0, 13 and 2051, with and without a bitmap of their own).  The rows the parent makes NULL hold the same
    offending values as the column's own NULL rows: status 0."""
    rng = np.random.default_rng(2000 + sorted(FLAT_VARIANTS).index(variant))
    cols = struct_child_columns(variant, rng)
    assert len(cols) == 24
    _, status = _run_and_check(ctx, torch, cols)
    assert status == 0


@pytest.mark.parametrize("variant", list(FLAT_VARIANTS))
def test_children_of_fixed_size_lists_rebuild_the_parent_bits(ctx, torch, variant):
    """2, 3, 64 and 100 child rows per parent row over 1, 33 and 700 parent rows (child tiles end inside a parent word):
    24 tasks per variant; tile_validity, lane_validity_end and the LDS path of the dec128 and string kernels."""
    rng = np.random.default_rng(3000 + sorted(FLAT_VARIANTS).index(variant))
    cols = list_child_columns(variant, rng)
    assert len(cols) == 24
    _, status = _run_and_check(ctx, torch, cols)
    assert status == 0


# ------------------------------------------------------------------------------------------------ no output validity
def _some_valid_row(col):
    bits = np.unpackbits(col["validity"], bitorder="little")[col["row_offset"]: col["row_offset"] + col["nrows"]]
    return col["row_offset"] + int(np.nonzero(bits)[0][70])


@pytest.mark.parametrize("variant", ["copy8", "dec128_i64", "str32", "fixed13", "bool", "mul_i64_1e6", "duration_mul_1e6", "list32"])
def test_without_out_validity_data_and_status_are_the_same(ctx, torch, variant):
    """One variant per kernel, with a bitmap.  For the kinds that check valid rows, one valid row offends, so the status
    compared is not 0."""
    rng = np.random.default_rng(41)
    col = make_column(variant, 4099, 13, "bitmap", rng)
    flag = 0
    if variant == "dec128_i64":
        col["buf1"][2 * _some_valid_row(col) + 1], flag = 5, _ffi.ST_DECIMAL_RANGE
    elif variant in ("mul_i64_1e6", "duration_mul_1e6"):
        col["buf1"][_some_valid_row(col)], flag = 2**62, _ffi.ST_MUL_OVERFLOW
    (with_words,), status = _run_and_check(ctx, torch, [col])
    (without,), status_without = run_plan(ctx, torch, [(col, None)], {}, out_validity=False)
    assert status == flag and status_without == flag
    assert np.array_equal(without[0], with_words[0])
    assert (without[1] == ONES).all(), "validity words were written without out_validity"


# ------------------------------------------------------------------------------------------------ status
STATUS_ROWS = [0, 70, 1024, 2047, WIN + 255]      # lane 0, inside a wave, the second dec128 group, the last row of a tile, the second tile
STATUS_NROWS = 4099


def _view(length, bi, bo):
    v = np.full(16, 0x5A, np.uint8)
    v.view(np.int32)[[0, 2, 3]] = [length, bi, bo]
    return v


def _view_case(bad_view, nbuf=2):
    table = np.array([[VIEW_BASE + (k << 32), 100] for k in range(nbuf)], np.uint64).reshape(-1)
    return lambda bad: dict(kind=_ffi.K_STRVIEW, buf1=bad_view if bad else _view(20, 1, 80), buf2=table, buf2_len=nbuf)


def _flat_status_cases():
    cases = {name: (make, flag) for name, (make, flag, _) in STATUS_CASES.items()}       # dec128, mul_i64, dict
    big = I64_MAX // 1000
    dur = lambda v: dict(kind=_ffi.K_DURATION, param=1000, buf1=np.array([v], np.int64))
    cases["duration_mul_above"] = (lambda bad: dur(big + 1 if bad else big), _ffi.ST_MUL_OVERFLOW)
    cases["duration_mul_below"] = (lambda bad: dur(-big - 1 if bad else -big), _ffi.ST_MUL_OVERFLOW)
    for sw, dw in ((4, 2), (8, 2), (8, 4)):
        lim = 1 << (8 * dw - 1)
        nar = lambda v, sw=sw, dw=dw: dict(kind=_ffi.K_NARROW, param=sw | (dw << 8), buf1=np.array([v], np.int32 if sw == 4 else np.int64))
        cases["narrow_%d_%d_above" % (sw, dw)] = (lambda bad, nar=nar, lim=lim: nar(lim if bad else lim - 1), _ffi.ST_DECIMAL_RANGE)
        cases["narrow_%d_%d_below" % (sw, dw)] = (lambda bad, nar=nar, lim=lim: nar(-lim - 1 if bad else -lim), _ffi.ST_DECIMAL_RANGE)
    cases["narrow_8_4_high_half_only"] = (lambda bad: dict(kind=_ffi.K_NARROW, param=8 | (4 << 8), buf1=np.array([2**32 + 5 if bad else 5], np.int64)),
                                          _ffi.ST_DECIMAL_RANGE)
    cases["strview_buffer_index_minus_1"] = (_view_case(_view(20, -1, 0)), _ffi.ST_BAD_OFFSETS)
    cases["strview_buffer_index_equal_to_nbuf"] = (_view_case(_view(20, 2, 0)), _ffi.ST_BAD_OFFSETS)
    cases["strview_negative_offset"] = (_view_case(_view(20, 0, -1)), _ffi.ST_BAD_OFFSETS)
    cases["strview_one_byte_past_the_buffer"] = (_view_case(_view(20, 1, 81)), _ffi.ST_BAD_OFFSETS)
    return cases


FLAT_STATUS_CASES = _flat_status_cases()


@pytest.mark.parametrize("case", list(FLAT_STATUS_CASES))
def test_value_checks_look_at_valid_rows_only(ctx, torch, case):
    """One offending row in a column of 4099 good ones: the flag is raised when the row is valid and not when it is NULL;
    the row's slot and its neighbours equal the reference in both."""
    make, flag = FLAT_STATUS_CASES[case]
    rng = np.random.default_rng(3)
    for bad_row in STATUS_ROWS:
        col = _status_column(make, bad_row, STATUS_NROWS, rng)
        col["name"] = "%s/row%d" % (case, bad_row)
        null = dict(col, validity=col["validity"].copy())
        null["validity"][bad_row >> 3] &= 0xFF ^ (1 << (bad_row & 7))
        for c, want in ((col, flag), (null, 0)):
            got, status = run_plan(ctx, torch, [(c, None)], {})
            assert check_job(c, None, got[0], want=flat_reference(c)) == want, c["name"]
            assert status == want, (c["name"], status)


def _list_column(kind, windows, rng):
    n = STATUS_NROWS
    lens = rng.choice([1, 2, 3], n + PAD_ROWS)           # no empty list: no other row starts or ends where the damaged one does
    off = (5 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32 if kind == _ffi.K_LIST32 else np.int64)
    col = dict(kind=kind, buf1=off, param=int(off[n]), nrows=n, row_offset=0, null_count=-1,
               validity=rng.integers(0, 256, (n + PAD_ROWS + 63) // 64 * 8 + 8, dtype=np.uint8))
    if windows:
        col["window_starts"] = np.array([0, 40, 700, 2047, 2348, 4000], np.int64)
    return col


@pytest.mark.parametrize("damage", ["end_before_start", "end_past_the_child", "negative_start", "start_before_the_window"])
@pytest.mark.parametrize("kind,windows", [(_ffi.K_LIST32, False), (_ffi.K_LIST64, True)], ids=["list32", "list64_windows"])
def test_list_offsets_are_validated_for_every_row(ctx, torch, kind, windows, damage):
    """b < a, b > child length, a < 0 and a < the window's base raise BAD_OFFSETS whether the row is valid or NULL (the
    whole-array validation upstream does not look at the bitmap); entries equal the oracle's arithmetic either way.  The
    offsets are only computed with, never followed."""
    rng = np.random.default_rng(6)
    for row in STATUS_ROWS:
        for valid in (True, False):
            bad_row = row
            col = _list_column(kind, windows, rng)
            col["name"] = "%s/row%d/%s" % (damage, bad_row, "valid" if valid else "NULL")
            off = col["buf1"]
            if damage == "end_before_start":
                off[bad_row + 1] = off[bad_row] - 1
            elif damage == "end_past_the_child":
                col["param"] = int(off[bad_row + 1]) - 1
            elif damage == "negative_start":
                off[bad_row] = -1
            else:
                start = max(int(w) for w in col.get("window_starts", range(0, STATUS_NROWS, WIN)) if w <= bad_row)
                bad_row += start == bad_row               # the first row of a window starts at its base
                off[bad_row] = off[start] - 1
            col["validity"][bad_row >> 3] = (col["validity"][bad_row >> 3] & (0xFF ^ (1 << (bad_row & 7)))) | (int(valid) << (bad_row & 7))
            want = flat_reference(col)
            assert want[2] == _ffi.ST_BAD_OFFSETS
            got, status = run_plan(ctx, torch, [(col, None)], {})
            assert check_job(col, None, got[0], want=want) == _ffi.ST_BAD_OFFSETS, col["name"]
            assert status == _ffi.ST_BAD_OFFSETS, (col["name"], status)


# ------------------------------------------------------------------------------------------------ one plan of everything
def test_one_plan_of_every_variant_gives_what_each_task_gives_alone(ctx, torch):
    """One task of every variant -- flat, struct child and fixed-size-list child in turn, depths 0 and 1 -- in a single
    plan: the slice tables, the grouping by depth and kernel class and the misc groups of the engine."""
    rng = np.random.default_rng(51)
    cols = []
    for i, variant in enumerate(FLAT_VARIANTS):
        n, o = 2049 + 97 * (i % 5), ROW_OFFSETS[i % len(ROW_OFFSETS)]
        if i % 3 == 0:
            cols.append(make_column(variant, n, o, ("bitmap", "none")[i % 2], rng))
        elif i % 3 == 1:
            cols.append(make_column(variant, n, o, ("bitmap", "none")[i % 2], rng, parent=(_parent_words(n, rng), i % 2)))
        else:
            cols.append(make_column(variant, 3 * (n // 3), o, ("bitmap", "none")[i % 2], rng, parent=(_parent_words(n // 3, rng), 3)))
    got, status = _run_and_check(ctx, torch, cols)
    assert status == 0
    for col, g in zip(cols, got):
        alone, st = run_plan(ctx, torch, [(col, None)], {})
        assert st == 0 and np.array_equal(alone[0][0], g[0]) and np.array_equal(alone[0][1], g[1]), col["name"]

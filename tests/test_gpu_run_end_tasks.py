"""The run-end decode kernel (transcode_run_end, kernels_run_end.hip) at the task level: hand-built MI_K_RUN_END tasks
through mi_plan against run_end_tasks.run_end_reference (numpy, held to pyarrow in test_run_end_reference_host.py).

Per task (run_end_tasks.check_case): every row equals the reference, the bytes behind the last row are still SENTINEL, the
validity words equal the reference (pad bits ones), the guard word is intact.  Per plan: the status equals the
reference's; where MI_ST_BAD_RUN_ENDS is expected the plan holds one task.

The cases follow the kernel: the 64-ary wave search (A; test_run_end_reference_host.py proves that the probes reach
every path of it), the staged window of a tile and array offsets (B), widths (C), validity (D), 64-bit positions (E), the
plan's promise that the values task runs first (F) and FULL validation of damaged run ends (G)."""
import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import run_end_tasks as rt
from run_end_tasks import ONES, WIDTHS, WIN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run_and_check(ctx, torch, cases, **kw):
    """one plan of clean tasks: every task against the reference, status 0"""
    got, status = rt.run_plan(ctx, torch, cases, **kw)
    for case, g in zip(cases, got):
        rt.check_case(case, g)
    assert status == 0, status
    return got


def _run_damaged(ctx, torch, case, **kw):
    """a plan of one damaged task: the reference's status, and nothing outside the two columns was read or written"""
    assert rt.case_reference(case) == (None, None, _ffi.ST_BAD_RUN_ENDS), case["name"]
    got, status = rt.run_plan(ctx, torch, [case], **kw)
    rt.check_damaged(case, got[0])
    assert status == _ffi.ST_BAD_RUN_ENDS, (case["name"], status)


# ------------------------------------------------------------------------------------------------ A: the wave search
@pytest.mark.parametrize("n_runs,rw,unit", rt.probe_configs(), ids=lambda v: str(int(v)))
def test_search_probes(ctx, torch, n_runs, rw, unit):
    """One plan of some hundreds of tasks of 1 to 3 rows, row_offset = the probed position, over one run-ends buffer: both
    searching waves of every tile at the seams of the first round's probes.  Then the position at the last run end, which
    no run holds (the answer n_runs): one task, MI_ST_BAD_RUN_ENDS, and the row is still a value of the column."""
    cases, damaged = rt.probe_cases(n_runs, rw, unit)
    up = rt.Uploads(torch)
    _run_and_check(ctx, torch, cases, up=up)
    _run_damaged(ctx, torch, damaged, up=up)


# ------------------------------------------------------------------------------------------------ B: tiles and offsets
@pytest.mark.parametrize("profile", rt.TILE_PROFILES)
def test_tile_shapes(ctx, torch, profile):
    """11 row counts x 3 or 7 array offsets, each with the last run ending at the last row and with runs that begin well
    before the first row and end well behind the last."""
    _run_and_check(ctx, torch, rt.tile_cases(profile))


# ------------------------------------------------------------------------------------------------ C: widths
def test_every_value_width_with_every_run_end_width(ctx, torch):
    """random bytes, 16-byte rows included: out unchanged"""
    rng = np.random.default_rng(31)
    cases = []
    for rw in (2, 4, 8):
        for w in WIDTHS:
            ends = rt.tile_ends("geometric_3", 13, 4099, True, rng)
            cases.append(rt.make_case(ends, rw, w, 13, 4099, rng, bits=rt.make_bits(len(ends), rng), name="widths"))
    _run_and_check(ctx, torch, cases)


# ------------------------------------------------------------------------------------------------ D: validity
SEAM_RUNS = (63, 64, 127, 128)
VALIDITY_ROWS = 4099        # ends inside a word: 4099 = 64 * 64 + 3


def _validity_cases(rng, **kw):
    """unit runs (run = row) and runs of mean 3 at offsets 0 and 13; the runs 63, 64, 127 and 128 are NULL, their
    neighbours valid, the others random"""
    cases = []
    for profile in ("unit_runs", "geometric_3"):
        for ro in (0, 13):
            ends = rt.tile_ends(profile, ro, VALIDITY_ROWS, False, rng)
            bits = rt.make_bits(len(ends), rng, null_runs=SEAM_RUNS)
            for k in (62, 65, 126, 129):
                bits[k >> 3] |= 1 << (k & 7)
            cases.append(rt.make_case(ends, 4, 8, ro, VALIDITY_ROWS, rng, bits=bits, name="validity/" + profile, **kw))
    return cases


def test_validity_of_runs_at_the_word_seams(ctx, torch):
    cases = _validity_cases(np.random.default_rng(41))
    for c in cases:
        ok = rt.bits_of(rt.case_reference(c)[1], c["nrows"])
        assert not ok.all() and ok.any()
    _run_and_check(ctx, torch, cases)


def test_null_count_0_ignores_the_bitmap_and_no_bitmap_is_all_valid(ctx, torch):
    rng = np.random.default_rng(42)
    cases = _validity_cases(rng, null_count=0)
    cases += [dict(c, bits=None, null_count=nc, name=c["name"] + "/no_bitmap") for c in cases for nc in (-1, 7)]
    for c in cases:
        assert (rt.case_reference(c)[1] == ONES).all()
    _run_and_check(ctx, torch, cases)


def test_without_out_validity_the_preset_words_stay(ctx, torch):
    cases = _validity_cases(np.random.default_rng(43))
    with_words = _run_and_check(ctx, torch, cases)
    without, status = rt.run_plan(ctx, torch, cases, out_validity=False)
    assert status == 0
    for c, a, b in zip(cases, with_words, without):
        assert np.array_equal(a[0], b[0]), c["name"]
        assert (b[1] == ONES).all(), (c["name"], "validity words were written without out_validity")


@pytest.mark.parametrize("parent_div", [0, 1])
def test_struct_parent_words_are_anded_in(ctx, torch, parent_div):
    """out_aux = random parent words (their pad bits random too: the task's pad bits are ones all the same); a parent-NULL
    row over a valid run comes out NULL.  Row counts that end inside a word, at a word's end and at a tile's end.
    (expand_tile used to AND the parent's word in and store it as it was: the last word took the parent's pad bits, where
    tile_valid_word of the flat kernels makes them ones.  This test showed it: "got 3f3a06e1f11cee09 want fffffffffffffff9".)"""
    rng = np.random.default_rng(44 + parent_div)
    cases = []
    for n, ro in ((VALIDITY_ROWS, 13), (65, 0), (64, 1), (WIN, 63), (WIN + 1, 2051), (1, 0)):
        for bits in (True, False):
            ends = rt.tile_ends("geometric_3", ro, n, True, rng)
            cases.append(rt.make_case(ends, 8, 4, ro, n, rng, bits=rt.make_bits(len(ends), rng) if bits else None,
                                      parent=rt.parent_words(n, rng), parent_div=parent_div, name="parent_div%d" % parent_div))
    c = cases[0]
    own = rt.bits_of(rt.run_end_reference(c["ends"][: c["n_runs"]], c["values"][: c["n_runs"]], rt.case_value_ok(c), c["row_offset"], c["nrows"])[1], c["nrows"])
    both = rt.bits_of(rt.case_reference(c)[1], c["nrows"])
    assert (own & ~both).any() and both.any() and (~own).any()
    assert any(int(c["parent"][c["nrows"] >> 6]) >> (c["nrows"] & 63) != int(ONES) >> (c["nrows"] & 63) for c in cases if c["nrows"] % 64), \
        "some parent has a zero among its pad bits"
    _run_and_check(ctx, torch, cases)


# ------------------------------------------------------------------------------------------------ E: wide positions
def test_positions_behind_2_to_the_40(ctx, torch):
    """row_offset = 2^40 + 5, int64 run ends around it: only the arithmetic is that wide, no address is"""
    rng = np.random.default_rng(51)
    ro, n = 2**40 + 5, 5000
    cases = []
    for past in (False, True):
        body = ro - 700 + np.cumsum(rng.geometric(1 / 3.0, 4000))
        body = [int(e) for e in body if e < ro + n]
        ends = [2**31 - 1, 2**31, 2**32 + 1, 2**40 - 3000] + body + [ro + n + (2**33 if past else 0)]
        cases.append(rt.make_case(ends, 8, 8, ro, n, rng, bits=rt.make_bits(len(ends), rng), name="wide64"))
        assert cases[-1]["n_runs"] > 1500 and sum(e <= ro for e in ends) > 64
    _run_and_check(ctx, torch, cases)


def test_int32_run_ends_up_to_the_largest_int32(ctx, torch):
    """row_offset + nrows = 2^31 - 1 = the last run end"""
    rng = np.random.default_rng(52)
    n = 5000
    ro = 2**31 - 1 - n
    body = ro - 700 + np.cumsum(rng.geometric(1 / 3.0, 4000))
    ends = [5, 2**30, 2**31 - 20000] + [int(e) for e in body if e < ro + n] + [ro + n]
    case = rt.make_case(ends, 4, 8, ro, n, rng, bits=rt.make_bits(len(ends), rng), name="wide32")
    assert case["ends"].dtype == np.int32 and int(case["ends"][case["n_runs"] - 1]) == 2**31 - 1
    _run_and_check(ctx, torch, [case])


# ------------------------------------------------------------------------------------------------ F: values from the same plan
@pytest.mark.parametrize("where", ["before", "after"])
def test_values_task_of_the_same_plan_runs_first(ctx, torch, where):
    """The values vector is scratch preset to POISON; a K_COPY task of the plan fills it, standing before or after the
    run-end tasks in the task array.  A run-end kernel that ran first would expand POISON."""
    rng = np.random.default_rng(61)
    cases = []
    for w in WIDTHS:
        ends = rt.tile_ends("geometric_3", 13, 3 * WIN + 7, True, rng)
        cases.append(rt.make_case(ends, 4, w, 13, 3 * WIN + 7, rng, name="values_%s" % where))
    _run_and_check(ctx, torch, cases, values_task=where)


# ------------------------------------------------------------------------------------------------ G: damaged run ends
DAMAGE_CASES = rt.damage_cases()


@pytest.mark.parametrize("name", list(DAMAGE_CASES))
def test_damaged_run_ends_raise_the_flag_and_read_nothing_else(ctx, torch, name):
    """The clean twin (one entry differs) gives the reference and status 0; the damaged column gives MI_ST_BAD_RUN_ENDS,
    leaves the sentinel tail and the guard word alone and writes only values of the column.  (Every search of the kernel is
    clamped to [0, n_runs) and every staged window to 2048 entries, so the damaged ends move no read outside the column.)"""
    clean, damaged = DAMAGE_CASES[name]
    for rw in (4, 8):
        rng = np.random.default_rng(71)
        mk = lambda ends: rt.make_case(ends, rw, 8, rt.DAMAGE_OFFSET, rt.DAMAGE_ROWS, rng, bits=rt.make_bits(len(ends), rng), name=name)
        _run_and_check(ctx, torch, [mk(clean)])
        _run_damaged(ctx, torch, mk(damaged))

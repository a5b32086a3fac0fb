"""The reference and the case lists of test_gpu_run_end_tasks.py (run_end_tasks.py), checked where they can be: without a
GPU.  The reference against pyarrow.compute.run_end_decode on logical slices, its status rule on hand-written columns,
the model of the kernel's wave search against numpy at every probe -- and the assertions that the probe lists and the
tile shapes reach the paths they were written for, so that nobody thins them without noticing."""
import numpy as np
import pytest

from duckdb_arrow_amd import _ffi

import run_end_tasks as rt
from run_end_tasks import WIN

BAD = _ffi.ST_BAD_RUN_ENDS


def test_the_status_bit_is_the_library_s():
    assert rt._ST_BAD == _ffi.ST_BAD_RUN_ENDS == 512 and _ffi.K_RUN_END == 22


# ------------------------------------------------------------------------------------------------ reference against pyarrow
def _fixed_bytes(arr, w):
    """the data buffer of a fixed-width pyarrow array as rows of w bytes"""
    raw = np.frombuffer(arr.buffers()[1], np.uint8)
    return raw[arr.offset * w: (arr.offset + len(arr)) * w].reshape(len(arr), w)


@pytest.mark.parametrize("ret", ["int16", "int32", "int64"])
def test_reference_equals_pyarrow_run_end_decode_on_slices(ret):
    """Values of 1, 2, 4, 8 and 16 bytes with NULLs; slices that begin inside a run and end before their last run does."""
    import decimal
    import pyarrow as pa
    import pyarrow.compute as pc
    rng = np.random.default_rng(5)
    value_types = [(pa.int8(), 1), (pa.int16(), 2), (pa.int32(), 4), (pa.int64(), 8), (pa.decimal128(38, 0), 16)]
    for (typ, w), mean in zip(value_types, (1.5, 3, 3, 40, 7)):
        lens = rng.geometric(1.0 / mean, 9000)
        ends = np.cumsum(lens)
        ends = ends[ends <= 20000]
        total, n_runs = int(ends[-1]), len(ends)
        ints = rng.integers(-100, 100, n_runs) if w == 1 else rng.integers(-2**(8 * min(w, 8) - 1), 2**(8 * min(w, 8) - 1) - 1, n_runs)
        mask = rng.random(n_runs) < 0.3
        if w == 16:
            values = pa.array([None if m else decimal.Decimal(int(v) * 1234567891) for v, m in zip(ints, mask)], typ)
        else:
            values = pa.array(ints, pa.int64(), mask=mask).cast(typ)
        arr = pa.RunEndEncodedArray.from_arrays(pa.array(ends, getattr(pa, ret)()), values)
        inside = int(ends[n_runs // 2]) - 1           # the last row of a run: the next row starts one
        slices = [(0, total), (1, total - 1), (inside, 1), (inside, 2), (inside + 1, 4099), (int(ends[3]), WIN), (total - 1, 1), (5, 0)]
        slices += [(int(o), int(rng.integers(1, total - o + 1))) for o in rng.integers(0, total, 12)]
        met_inside = met_short = 0
        for o, n in slices:
            part = arr.slice(o, n)
            assert part.offset == o and len(part.run_ends) == n_runs
            vals = part.values
            ok = np.array(vals.is_valid())
            got_data, got_words, status = rt.run_end_reference(part.run_ends.to_numpy(), _fixed_bytes(vals, w), ok, part.offset, n)
            assert status == 0
            flat = pc.run_end_decode(part)
            want_ok = np.array(flat.is_valid(), bool) if n else np.zeros(0, bool)
            assert np.array_equal(rt.bits_of(got_words, n), want_ok), (typ, o, n)
            assert len(got_words) == (n + 63) // 64 and (n % 64 == 0 or int(got_words[-1]) >> (n % 64) == 2**(64 - n % 64) - 1), "pad bits"
            if n:
                assert np.array_equal(got_data.reshape(n, w)[want_ok], _fixed_bytes(flat, w)[want_ok]), (typ, o, n)
                met_inside += o not in ends and o > 0
                met_short += (o + n) not in ends
        assert met_inside >= 3 and met_short >= 3


def test_reference_keeps_the_value_bytes_under_null_and_ands_the_parent_row_by_row():
    rng = np.random.default_rng(6)
    ends = np.cumsum(rng.integers(1, 5, 400))
    vals = rng.integers(0, 256, (400, 16), dtype=np.uint8)
    ok = rng.random(400) < 0.6
    o, n = 37, 700
    parent = rt.parent_words(n, rng)
    data, words, status = rt.run_end_reference(ends, vals, ok, o, n, parent)
    assert status == 0 and len(words) == 11
    for r in range(n):
        run = next(k for k in range(400) if ends[k] > o + r)
        assert bytes(data[16 * r: 16 * r + 16]) == bytes(vals[run])
        assert bool((int(words[r >> 6]) >> (r & 63)) & 1) == (bool(ok[run]) and bool((int(parent[r >> 6]) >> (r & 63)) & 1)), r
    assert int(words[-1]) >> (n & 63) == 2**(64 - (n & 63)) - 1, "pad bits are ones whatever the parent's are"
    assert int(parent[10]) >> (n & 63) != 2**(64 - (n & 63)) - 1


# ------------------------------------------------------------------------------------------------ status rule
@pytest.mark.parametrize("ends,ro,n,want", [
    ([3, 5, 10], 0, 10, 0), ([3, 5, 10], 2, 8, 0), ([3, 5, 10], 4, 1, 0), ([1], 0, 1, 0), ([3, 5, 10], 10, 0, 0),
    ([0, 5, 10], 0, 10, BAD), ([-1, 5, 10], 0, 10, BAD), ([3, 3, 10], 0, 10, BAD), ([3, 2, 10], 0, 10, BAD),
    ([3, 2, 10], 6, 2, BAD),                        # the decrease lies before the first row: still damaged
    ([3, 5, 10], 0, 11, BAD), ([3, 5, 10], 9, 2, BAD), ([3, 5, 10], 10, 1, BAD), ([3, 5, 4], 0, 4, BAD),
    ([2**40, 2**40 + 1], 2**40, 1, 0), ([2**40, 2**40 + 1], 2**40, 2, BAD),
])
def test_status_rule(ends, ro, n, want):
    assert rt.run_end_status(ends, ro, n) == want
    data, words, status = rt.run_end_reference(np.array(ends, np.int64), np.zeros((len(ends), 4), np.uint8), None, ro, n)
    assert status == want and (data is None) == (words is None) == bool(want)


def test_damage_cases_are_damaged_and_their_twins_differ_in_one_entry():
    cases = rt.damage_cases()
    assert len(cases) == 10
    per = rt.DAMAGE_PER
    assert per == 334 == -(-rt.DAMAGE_RUNS // 3) and -(-rt.DAMAGE_ROWS // WIN) == 3
    for name, (clean, damaged) in cases.items():
        assert len(clean) == len(damaged) == rt.DAMAGE_RUNS
        assert sum(a != b for a, b in zip(clean, damaged)) == 1, name
        assert rt.run_end_status(clean, rt.DAMAGE_OFFSET, rt.DAMAGE_ROWS) == 0, name
        assert rt.run_end_status(damaged, rt.DAMAGE_OFFSET, rt.DAMAGE_ROWS) == BAD, name
    where = lambda name: next(k for k, (a, b) in enumerate(zip(*cases[name])) if a != b)
    assert [where("decrease_at_share_seam_%d" % i) for i in (1, 2)] == [per, 2 * per]
    assert [where("decrease_before_share_seam_%d" % i) for i in (1, 2)] == [per - 1, 2 * per - 1]
    k = where("decrease_in_a_run_no_row_touches")
    assert cases["decrease_in_a_run_no_row_touches"][0][k + 1] < rt.DAMAGE_OFFSET
    assert cases["last_end_one_short"][1][-1] == rt.DAMAGE_OFFSET + rt.DAMAGE_ROWS - 1


# ------------------------------------------------------------------------------------------------ the search model
def _all_searches():
    """[(run count, Search, position, damaged)] of every search the probe plans make: the first and the last row of every task"""
    out = []
    for n_runs, rw, unit in rt.probe_configs():
        if rw != 8 and not unit:
            continue          # the int32 and int16 plans probe the same positions of the same ends
        ends = rt.probe_ends(n_runs, unit)
        tasks, last = rt.probe_tasks(ends)
        for p in sorted({q for p, n in tasks for q in (p, p + n - 1)}):
            out.append((n_runs, ends, rt.search_model(ends, n_runs, p), p, False))
        out.append((n_runs, ends, rt.search_model(ends, n_runs, last), last, True))
    return out


@pytest.fixture(scope="module")
def searches():
    return _all_searches()


def test_probe_configs_use_every_run_end_type_where_it_fits():
    cfg = rt.probe_configs()
    assert {n for n, rw, u in cfg if rw == 8} == set(rt.RUN_COUNTS) and len(rt.RUN_COUNTS) == 15
    assert {n for n, rw, u in cfg if rw == 4} == {n for n in rt.RUN_COUNTS if n <= 4161}
    assert {n for n, rw, u in cfg if rw == 2} == {n for n in rt.RUN_COUNTS if n <= 4161} | {32767}
    for n, rw, unit in cfg:
        ends = rt.probe_ends(n, unit)
        assert len(ends) == n and int(ends[-1]) < 2 ** (8 * rw - 1)
        assert unit or n < 3 or (set(np.diff(ends)) == {1, 2, 3} if n > 60 else ends[-1] > n)
    assert int(rt.probe_ends(32767, True)[-1]) == 32767
    tasks, last = rt.probe_tasks(rt.probe_ends(266305, False))
    assert 300 < len(tasks) < 700 and all(1 <= n <= 3 and p + n <= last for p, n in tasks)


def test_search_model_equals_numpy_at_every_probe(searches):
    assert len(searches) > 5000
    for n_runs, ends, s, p, damaged in searches:
        assert s.answer == int(np.searchsorted(ends, p, side="right")), (n_runs, p)
        assert (s.answer == n_runs) == damaged


def test_search_model_on_unsorted_ends_stays_inside_the_column():
    """what the kernel's clamps rely on: whatever the ends hold, the answer lies in [0, n_runs]"""
    rng = np.random.default_rng(3)
    for n_runs in (1, 64, 65, 4097, 266305):
        ends = rng.integers(-5, 1000, n_runs)
        for p in (-1, 0, 500, 999, 2000):
            assert 0 <= rt.search_model(ends, n_runs, p).answer <= n_runs


def test_probes_reach_every_path_of_the_search(searches):
    clean = [s for _, _, s, _, damaged in searches if not damaged]
    assert {s.rounds for s in clean} >= {0, 1, 2, 3}
    narrowing = {f for s in clean for f in s.lanes}
    assert 0 in narrowing and 63 in narrowing
    final = {s.final_lane for s in clean}
    assert 0 in final and 63 in final
    assert any(s.past_hi for s in clean), "a narrowing round decided by a lane that probes k >= hi"
    assert any(s.final_past_hi for s in clean)
    # the early exit: in the first round only behind the last end (128, 4096, 262 144 runs: a damaged task); 262 145 runs leave
    # 4096 after the first round, and a clean position whose answer is that window's hi leaves the second round early
    early = [(n, s, damaged) for n, _, s, _, damaged in searches if s.early_exit]
    assert {n for n, s, damaged in early if damaged} >= {128, 4096, 262144}
    assert any(s.rounds == 1 and s.answer < n for n, s, damaged in early if not damaged)
    for n_runs in rt.RUN_COUNTS:
        answers = {s.answer for n, _, s, _, _ in searches if n == n_runs}
        assert {0, n_runs - 1, n_runs} <= answers, n_runs
    # both positions around every probe index of the first round, and around its neighbours
    for n_runs in (65, 4161, 266305):
        ends = rt.probe_ends(n_runs, False)
        probed = {p for n, _, _, p, _ in searches if n == n_runs}
        for k in rt.search_model(ends, n_runs, 0).first_probes:
            for j in (k - 1, k, k + 1):
                if 0 <= j < n_runs - 1:
                    assert {int(ends[j]) - 1, int(ends[j])} <= probed, (n_runs, j)


# ------------------------------------------------------------------------------------------------ the tile shapes
def test_tile_shapes_meet_every_row_count_at_three_offsets():
    shapes = rt.tile_shapes()
    assert {n for n, o in shapes} == set(rt.TILE_ROW_COUNTS) == {1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099}
    assert {o for n, o in shapes} == set(rt.TILE_OFFSETS) == {0, 1, 63, 64, 2047, 2048, 2051}
    for n in rt.TILE_ROW_COUNTS:
        assert len({o for m, o in shapes if m == n}) >= 3


def test_tile_cases_are_clean_and_reach_the_window_shapes():
    cnts, on, below, above = set(), 0, 0, 0
    for profile in rt.TILE_PROFILES:
        cases = rt.tile_cases(profile)
        assert len(cases) == 2 * len(rt.tile_shapes())
        for i, c in enumerate(cases):
            ends = c["ends"][: c["n_runs"]].astype(np.int64)
            assert rt.run_end_status(ends, c["row_offset"], c["nrows"]) == 0, c["name"]
            assert (c["ends"][c["n_runs"]:] <= 0).all() and (c["values"][c["n_runs"]:] == rt.POISON).all()
            assert (c["values"][: c["n_runs"], 0] != rt.POISON).all()
            total = c["row_offset"] + c["nrows"]
            if i % 2:            # the first row's run begins before it (where there are rows before it), the last run goes on
                assert int(ends[-1]) == total + rt.PAST
                assert c["row_offset"] < 3 or profile == "unit_runs" or c["row_offset"] not in ends
            else:
                assert int(ends[-1]) == total
            seen = set(int(e) for e in ends)
            for p0, cnt in rt.tile_windows(c):
                cnts.add(cnt)
                assert 1 <= cnt <= WIN
                on += p0 in seen
                below += p0 - 1 in seen
                above += p0 + 1 in seen
    assert 1 in cnts and WIN in cnts and 2 in cnts and WIN - 1 in cnts
    assert on > 10 and below > 10 and above > 10
    # the broadcast path also in a tile that is neither the first nor the last of its task
    mids = [rt.tile_windows(c)[1][1] for c in rt.tile_cases("long_middle_run") if c["nrows"] == 4099]
    assert mids and set(mids) == {1}

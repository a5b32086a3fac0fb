"""Kernel-level run-end tasks (MI_K_RUN_END, transcode_run_end in kernels_run_end.hip) for test_gpu_run_end_tasks.py:
the reference, a model of the kernel's 64-ary wave search that picks the search probes, the case lists, and the runner.

The reference is numpy and Python ints only (np.searchsorted(ends, row_offset + p, side="right")); it is held to
pyarrow.compute.run_end_decode in test_run_end_reference_host.py.  The model of the search never supplies an expected
value: it says which positions make the search take which path, and the host file asserts that the probe lists cover them.

Buffers follow decode_tasks.py: output data filled with SENTINEL and over-allocated, output validity preset to ones plus
one guard word.  The run ends are generated PAD_RUNS entries longer than the column (zeros and negative numbers, which
would turn a search that read them) and the values PAD_RUNS rows longer (POISON bytes; the first byte of a real value is
never POISON), so a read past either column is a wrong row, never an access outside an allocation."""
import collections

import numpy as np

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

WIN = 2048
PAD_RUNS = WIN + 64
SENTINEL = 0xA5
POISON = 0xEE
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
WIDTHS = (1, 2, 4, 8, 16)
END_TYPES = {2: np.int16, 4: np.int32, 8: np.int64}


# ------------------------------------------------------------------------------------------------ reference
def words_of(ok):
    """bool per row -> validity words, pad bits of the last word ones"""
    n = len(ok)
    return np.packbits(np.concatenate([np.asarray(ok, bool), np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()


def bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def run_end_status(ends, row_offset, nrows):
    """ST_BAD_RUN_ENDS exactly when some ends[k] <= ends[k-1] (ends[-1] taken as 0) or the last end < row_offset + nrows"""
    e = np.asarray(ends).astype(np.int64)
    bad = int(e[0]) <= 0 or bool((e[1:] <= e[:-1]).any()) or int(e[-1]) < int(row_offset) + int(nrows)
    return _ST_BAD if bad else 0


_ST_BAD = 512      # MI_ST_BAD_RUN_ENDS, restated: test_run_end_reference_host.py holds it to _ffi.ST_BAD_RUN_ENDS


def run_end_reference(ends, values, value_ok, row_offset, nrows, parent_words=None):
    """Rows [row_offset, row_offset + nrows) of the run-end encoded array (ends, values), flat.
    ends: the n_runs run ends; values: n_runs rows of 1, 2, 4, 8 or 16 bytes (any array with n_runs rows); value_ok: bool
    per run or None (every run valid); parent_words: validity words of a struct parent with the same row numbering.
    -> (data bytes, validity words with pad bits ones, status); (None, None, status) for damaged run ends."""
    ends = np.asarray(ends).astype(np.int64)
    n_runs = len(ends)
    status = run_end_status(ends, row_offset, nrows)
    if status:
        return None, None, status
    vals = np.ascontiguousarray(values).view(np.uint8).reshape(n_runs, -1)
    assert vals.shape[1] in WIDTHS
    run = np.searchsorted(ends, int(row_offset) + np.arange(nrows, dtype=np.int64), side="right")
    ok = np.ones(nrows, bool) if value_ok is None else np.asarray(value_ok, bool)[run]
    if parent_words is not None:
        ok = ok & bits_of(parent_words, nrows)
    return vals[run].reshape(-1).copy(), words_of(ok), 0


# ------------------------------------------------------------------------------------------------ model of the search
Search = collections.namedtuple("Search", "answer rounds lanes final_lane early_exit past_hi final_past_hi first_probes")


def search_model(ends, n_runs, p):
    """wave_upper_bound(p) restated lane for lane: the first k in [0, n_runs) with ends[k] > p, n_runs when there is none.
    rounds = narrowing rounds that ran to their end, lanes = the first-true lane of each, final_lane = that of the last
    64-wide probe (None when no lane was true), early_exit = a narrowing round found no true lane and returned hi,
    past_hi = a narrowing round whose first true lane probed k >= hi, final_past_hi = the same of the last probe,
    first_probes = the indices below hi that the first round looked at."""
    lane = np.arange(64, dtype=np.int64)
    lo, hi = 0, int(n_runs)
    lanes, past_hi, first_probes = [], False, None
    while hi - lo > 64:
        step = (hi - lo + 63) // 64
        k = lo + (lane + 1) * step - 1
        m = (k >= hi) | (ends[np.minimum(k, hi - 1)] > p)
        if first_probes is None:
            first_probes = [int(x) for x in k[k < hi]]
        if not m.any():
            return Search(hi, len(lanes), lanes, None, True, past_hi, False, first_probes)
        f = int(np.argmax(m))
        past_hi |= bool(k[f] >= hi)
        lanes.append(f)
        nhi = lo + (f + 1) * step - 1
        lo, hi = lo + f * step, min(nhi, hi)
    k = lo + lane
    m = (k >= hi) | (ends[np.minimum(k, max(hi - 1, 0))] > p)
    if first_probes is None:
        first_probes = [int(x) for x in k[k < hi]]
    if not m.any():
        return Search(hi, len(lanes), lanes, None, False, past_hi, False, first_probes)
    f = int(np.argmax(m))
    return Search(lo + f, len(lanes), lanes, f, False, past_hi, bool(k[f] >= hi), first_probes)


# ------------------------------------------------------------------------------------------------ columns
def poison_ends(ends, rw):
    """the run ends as the kernel's type, PAD_RUNS poison entries behind them: 0, -1, 0, -3, ..."""
    pad = np.where(np.arange(PAD_RUNS) % 2 == 0, 0, -np.arange(PAD_RUNS))
    out = np.concatenate([np.asarray(ends, np.int64), pad])
    assert np.abs(out).max() < 2 ** (8 * rw - 1)
    return out.astype(END_TYPES[rw])


def make_values(n_runs, w, rng):
    """n_runs random rows of w bytes whose first byte is never POISON, PAD_RUNS rows of POISON behind them"""
    v = rng.integers(0, 256, (n_runs + PAD_RUNS, w), dtype=np.uint8)
    v[v[:, 0] == POISON, 0] = POISON ^ 0xFF
    v[n_runs:] = POISON
    return v


def make_bits(n_runs, rng, null_runs=()):
    """random validity words over the runs (and over the padding), bytes; `null_runs` are NULL"""
    b = rng.integers(0, 256, (n_runs + PAD_RUNS + 63) // 64 * 8 + 8, dtype=np.uint8)
    for k in null_runs:
        if k < n_runs:
            b[k >> 3] &= 0xFF ^ (1 << (k & 7))
    return b


def make_case(ends, rw, w, row_offset, nrows, rng, *, values=None, bits=None, null_count=-1, parent=None, parent_div=0, name="",
              dev_ends=None):
    """One task.  ends = the real run ends (python ints or an array); dev_ends = an already poisoned buffer that holds them
    (shared between cases); values = a make_values() array to share, None = fresh."""
    n_runs = len(ends)
    return dict(ends=dev_ends if dev_ends is not None else poison_ends(ends, rw), n_runs=n_runs, rw=rw, w=w,
                values=values if values is not None else make_values(n_runs, w, rng), bits=bits, null_count=null_count,
                row_offset=int(row_offset), nrows=int(nrows), parent=parent, parent_div=parent_div,
                name="%s/rw%d/w%d/n%d/o%d" % (name, rw, w, nrows, row_offset))


def case_value_ok(case):
    if case["bits"] is None or case["null_count"] == 0:
        return None
    return np.unpackbits(case["bits"], bitorder="little")[: case["n_runs"]].astype(bool)


def case_reference(case):
    n = case["n_runs"]
    return run_end_reference(case["ends"][:n], case["values"][:n], case_value_ok(case), case["row_offset"], case["nrows"], case["parent"])


def parent_words(rows, rng):
    """random validity words of a struct parent of `rows` rows, pad bits included, and one word more"""
    return rng.integers(0, 256, ((rows + 63) // 64 + 1) * 8, dtype=np.uint8).view(np.uint64)


# ------------------------------------------------------------------------------------------------ A: search probes
RUN_COUNTS = [1, 2, 63, 64, 65, 66, 128, 129, 4096, 4097, 4160, 4161, 262144, 262145, 266305]
UNIT_INT16 = 32767       # one int16 column of 32 767 unit runs: the last end is the largest int16


def probe_configs():
    """(run count, run-end width, unit runs): int64 throughout, int32 up to 4161 runs, int16 wherever the last end fits"""
    out = [(n, 8, False) for n in RUN_COUNTS] + [(n, 4, False) for n in RUN_COUNTS if n <= 4161]
    out += [(n, 2, False) for n in RUN_COUNTS if 3 * n <= 32767] + [(UNIT_INT16, 2, True)]
    return out


def probe_ends(n_runs, unit):
    """run lengths 1 to 3, mixed (ends are not indices); or unit runs"""
    rng = np.random.default_rng(7000 + n_runs)
    return np.cumsum(np.ones(n_runs, np.int64) if unit else rng.integers(1, 4, n_runs))


def probe_positions(ends):
    """-> (valid positions, ascending; the damaged position = the last end, which no run holds).  ends[k] - 1 and ends[k]
    for k at the first round's probe indices of the model and at their neighbours, position 0, the last valid position
    and a seeded random sample."""
    n_runs, last = len(ends), int(ends[-1])
    ks = set()
    for k in search_model(ends, n_runs, 0).first_probes:
        ks.update(j for j in (k - 1, k, k + 1) if 0 <= j < n_runs)
    ks.update((0, n_runs - 1))
    pos = {0, last - 1}
    for k in ks:
        pos.update((int(ends[k]) - 1, int(ends[k])))
    rng = np.random.default_rng(n_runs)
    pos.update(int(x) for x in rng.integers(0, last, 64))
    return sorted(p for p in pos if 0 <= p < last), last


def probe_cases(n_runs, rw, unit):
    """-> (cases of one plan, the damaged case).  One task of 1 to 3 rows per probed position, row_offset = the position;
    one run-ends buffer and one values buffer per width, shared; the value width rotates."""
    ends = probe_ends(n_runs, unit)
    rng = np.random.default_rng(n_runs + rw)
    dev_ends = poison_ends(ends, rw)
    values = {w: make_values(n_runs, w, rng) for w in WIDTHS}
    bits = make_bits(n_runs, rng)
    mk = lambda i, p, n: make_case(ends, rw, WIDTHS[i % 5], p, n, rng, values=values[WIDTHS[i % 5]], bits=bits, dev_ends=dev_ends,
                                   name="probe%d" % n_runs)
    tasks, last = probe_tasks(ends)
    return [mk(i, p, n) for i, (p, n) in enumerate(tasks)], mk(3, last, 1)


def probe_tasks(ends):
    """-> ([(row_offset, nrows)] of the clean tasks of a probe plan, row_offset of the damaged one-row task)"""
    positions, last = probe_positions(ends)
    return [(p, min(1 + i % 3, last - p)) for i, p in enumerate(positions)], last


# ------------------------------------------------------------------------------------------------ B: tile shapes
TILE_ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099]
TILE_OFFSETS = [0, 1, 63, 64, 2047, 2048, 2051]
TILE_PROFILES = ["one_run", "unit_runs", "long_middle_run", "ends_on_seams", "ends_below_seams", "ends_above_seams", "geometric_3",
                 "geometric_300"]
PAST = 3000      # "well past": the last run goes on for this many rows behind the task


def tile_shapes():
    """(row count, array offset): every row count at three offsets in rotation, 2049 and 4099 at every offset"""
    shapes = []
    for i, n in enumerate(TILE_ROW_COUNTS):
        offs = TILE_OFFSETS if n in (2049, 4099) else [TILE_OFFSETS[(i + j) % 7] for j in (0, 2, 4)]
        shapes += [(n, o) for o in offs]
    return shapes


def tile_ends(profile, ro, n, past, rng):
    """The run ends of one tile-shape case.  past False: a run ends at `ro` (when ro > 0) and the last one at ro + n.
    past True: the run of the first row begins well before ro (at 2 ro / 3) and the last one ends PAST rows behind ro + n."""
    final = ro + n + (PAST if past else 0)
    begin = 2 * ro // 3 if past else ro
    pts = {ro // 3, begin}
    seams = [ro + WIN * i for i in range((n + WIN - 1) // WIN + 1)]
    if profile == "unit_runs":
        pts.update(range(1, final))
    elif profile == "long_middle_run":       # rows [2040, 4097) of the task are one run: the tile of rows 2048 .. 4095 lies inside
        pts.update(ro + e for e in (7, 2040, 4097))
    elif profile == "ends_on_seams":
        pts.update(seams[1:])
        pts.update(range(begin + 97, final, 97))
    elif profile == "ends_below_seams":
        pts.update(s - 1 for s in seams)
        pts.update(range(begin + 97, final, 97))
    elif profile == "ends_above_seams":
        pts.update(s + 1 for s in seams)
        pts.update(range(begin + 97, final, 97))
    elif profile.startswith("geometric"):
        mean = int(profile.split("_")[1])
        pts.update(int(x) for x in begin + np.cumsum(rng.geometric(1.0 / mean, (final - begin) // mean + 8)))
    else:
        assert profile == "one_run"
    if past and profile != "unit_runs":
        pts -= set(range(begin + 1, ro + 1))       # the first row's run begins at `begin`
    return sorted(p for p in pts if 0 < p < final) + [final]


def tile_cases(profile):
    """every shape x {last end = ro + n, last end well past it}; run-end and value widths rotate; every other task has NULL runs"""
    rng = np.random.default_rng(8000 + TILE_PROFILES.index(profile))
    cases = []
    for i, (n, ro) in enumerate(tile_shapes()):
        for past in (False, True):
            ends = tile_ends(profile, ro, n, past, rng)
            j = 2 * i + past
            cases.append(make_case(ends, (2, 4, 8)[j % 3], WIDTHS[j % 5], ro, n, rng, bits=make_bits(len(ends), rng) if j % 2 else None,
                                   name="%s/%s" % (profile, "past" if past else "exact")))
    return cases


def tile_windows(case):
    """(first array position, number of staged run ends) of every tile of a clean case, from the reference's own search"""
    ends = case["ends"][: case["n_runs"]].astype(np.int64)
    out = []
    for row0 in range(0, case["nrows"], WIN):
        p0 = case["row_offset"] + row0
        p1 = case["row_offset"] + min(row0 + WIN, case["nrows"]) - 1
        first, last = np.searchsorted(ends, [p0, p1], side="right")
        out.append((p0, int(last - first + 1)))
    return out


# ------------------------------------------------------------------------------------------------ G: damaged run ends
DAMAGE_ROWS, DAMAGE_OFFSET, DAMAGE_RUNS = 3 * WIN - 5, 3000, 1000      # three tiles; per = ceil(1000 / 3) = 334 run ends per tile
DAMAGE_PER = (DAMAGE_RUNS + 2) // 3


def _damage_base():
    """1000 runs of 2 rows or more: the first 100 (2 to 4 rows each) end far before the array's offset, the others end at
    random even distances behind them, the last one at row_offset + nrows"""
    rng = np.random.default_rng(9000)
    head = np.cumsum(rng.integers(2, 5, 100))
    total = DAMAGE_OFFSET + DAMAGE_ROWS
    assert head[-1] < DAMAGE_OFFSET - 2000
    tail = np.sort(rng.choice(np.arange(int(head[-1]) + 2, total - 1, 2), DAMAGE_RUNS - 101, replace=False))
    return [int(e) for e in head] + [int(e) for e in tail] + [total]


def damage_cases():
    """name -> (clean run ends, damaged run ends): the two differ in one entry"""
    base = _damage_base()
    assert all(b - a >= 2 for a, b in zip([0] + base[:-1], base)), "every entry can move down by one and stay clean"
    out = {}

    def put(name, k, bad, clean=None):
        c, d = list(base), list(base)
        if clean is not None:
            c[k] = clean
        d[k] = bad
        assert sum(x != y for x, y in zip(c, d)) == 1
        out[name] = (c, d)
    put("first_end_is_0", 0, 0, clean=1)
    put("first_end_negative", 0, -5)
    put("equal_neighbours", 500, base[499])
    put("decrease", 500, base[499] - 1)
    for i in (1, 2):
        put("decrease_at_share_seam_%d" % i, DAMAGE_PER * i, base[DAMAGE_PER * i - 1] - 1)
        put("decrease_before_share_seam_%d" % i, DAMAGE_PER * i - 1, base[DAMAGE_PER * i - 2] - 1)
    put("decrease_in_a_run_no_row_touches", 40, base[39] - 1)
    put("last_end_one_short", DAMAGE_RUNS - 1, base[-1] - 1)
    return out


# ------------------------------------------------------------------------------------------------ running a plan
class Uploads:
    """numpy array -> device bytes, once per array (padded to 8 bytes and never empty, as IPC buffers are)"""

    def __init__(self, torch):
        self.torch, self.dev, self.keep = torch, {}, []

    def __call__(self, a):
        if id(a) not in self.dev:
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            self.dev[id(a)] = self.torch.from_numpy(np.concatenate([b, np.zeros(16 - len(b) % 8, np.uint8)])).cuda()
            self.keep.append(a)
        return self.dev[id(a)]


def run_plan(ctx, torch, cases, out_validity=True, up=None, values_task=None):
    """One Plan of K_RUN_END tasks, one launch.  All outputs live in two arenas (one download each).
    values_task "before" / "after": every case's values vector is device scratch preset to POISON that a K_COPY task of the
    same plan (depth 1, standing before / after the run-end tasks in the task array) fills from the case's values.
    -> ([(data bytes incl. the 64 sentinel bytes, validity words incl. the guard word) per case], status)"""
    up = up or Uploads(torch)
    data_at, words_at, nd, nw = [], [], 0, 0
    for c in cases:
        data_at.append(nd)
        words_at.append(nw)
        nd += (c["nrows"] * c["w"] + 15) // 16 * 16 + 64
        nw += (c["nrows"] + 63) // 64 + 1
    out = torch.full((nd,), SENTINEL, dtype=torch.uint8, device="cuda")
    outv = torch.full((nw * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    tasks, copies, keep = [], [], []
    for c, da_, wa in zip(cases, data_at, words_at):
        if values_task:
            vals = torch.full((c["values"].size,), POISON, dtype=torch.uint8, device="cuda")
            keep.append(vals)
            copies.append(da.make_task(_ffi.K_COPY, c["n_runs"], up(c["values"]).data_ptr(), vals.data_ptr(), param=c["w"], depth=1))
        else:
            vals = up(c["values"])
        assert vals.data_ptr() % 16 == 0
        tasks.append(da.make_task(_ffi.K_RUN_END, c["nrows"], up(c["ends"]).data_ptr(), out.data_ptr() + da_,
                                  validity=up(c["bits"]).data_ptr() if c["bits"] is not None else 0, buf2=vals.data_ptr(),
                                  out_validity=outv.data_ptr() + 8 * wa if out_validity else 0,
                                  out_aux=up(c["parent"]).data_ptr() if c["parent"] is not None else 0, parent_div=c["parent_div"],
                                  depth=1 if c["parent"] is not None else 0, row_offset=c["row_offset"],
                                  param=c["rw"] | (c["w"] << 8), param2=c["n_runs"], null_count=c["null_count"]))
    plan = da.Plan(ctx, copies + tasks if values_task == "before" else tasks + copies)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    status = plan.status()
    h, hv = out.cpu().numpy(), outv.cpu().numpy().view(np.uint64)
    plan.close()
    ends_at = data_at[1:] + [nd], words_at[1:] + [nw]
    return [(h[a:b], hv[c:d]) for a, b, c, d in zip(data_at, ends_at[0], words_at, ends_at[1])], status


def check_case(case, got, want=None):
    """The four assertions of decode_tasks.check_job on one clean task: rows, sentinel tail, validity words, guard word."""
    data, words = got
    want_data, want_words, want_status = want if want is not None else case_reference(case)
    assert want_status == 0, case["name"]
    w, n, where = case["w"], case["nrows"], case["name"]
    if not np.array_equal(data[: n * w], want_data):
        bad = np.nonzero(np.any(data[: n * w].reshape(-1, w) != want_data.reshape(-1, w), axis=1))[0]
        raise AssertionError("%s: %d of %d output rows differ, first %d: got %s want %s" % (
            where, len(bad), n, bad[0], data[bad[0] * w: bad[0] * w + w].tolist(), want_data[bad[0] * w: bad[0] * w + w].tolist()))
    assert (data[n * w:] == SENTINEL).all(), (where, "bytes behind the last output row were written")
    assert len(words) == (n + 63) // 64 + 1
    if not np.array_equal(words[:-1], want_words):
        bad = np.nonzero(words[:-1] != want_words)[0]
        raise AssertionError("%s: %d validity words differ, first %d of %d: got %016x want %016x" % (
            where, len(bad), bad[0], len(want_words), int(words[bad[0]]), int(want_words[bad[0]])))
    assert words[-1] == ONES, (where, "the guard word behind the validity words lost bits")


def check_damaged(case, got):
    """A damaged task: the sentinel tail, the guard word, and every output row is one of values[0 : n_runs]."""
    data, words = got
    w, n, where = case["w"], case["nrows"], case["name"]
    assert (data[n * w:] == SENTINEL).all(), (where, "bytes behind the last output row were written")
    assert len(words) == (n + 63) // 64 + 1 and words[-1] == ONES, (where, "the guard word behind the validity words lost bits")
    real = {bytes(r) for r in case["values"][: case["n_runs"]]}
    strange = [r for r in range(n) if bytes(data[r * w: r * w + w]) not in real]
    assert not strange, (where, "rows that are no value of the column", strange[:5], data[strange[0] * w: strange[0] * w + w].tolist())

"""Kernel-level decode tasks for the GPU suites (test_gpu_gather.py, test_gpu_flat_decode.py): source columns of every
decode kind with values chosen to hurt, one Plan per list of tasks, and the assertions on a task's output.

Buffers follow the host's contract: validity preset to ones for ceil(total / 64) words plus one guard word.  On top of
that the output is filled with a sentinel and over-allocated, and every source buffer is generated PAD_ROWS rows longer
than the column, so a kernel that read past the column's last row would read defined bytes of the same allocation and
show up as a wrong value, never as an access outside the buffers."""
import numpy as np

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi
from oracle import pyoracle as po

from helpers import _words_of, decode_column_reference, gather_reference

WIN = 2048
PAD_ROWS = WIN + 64
SEL_FILL = 2048
SENTINEL = 0xA5
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
PTR_BASE = 0x7000_0000_1003


# ------------------------------------------------------------------------------------------------ columns
def _dict_variant(iw, signed):
    dict_len = {(1, 1): 100, (1, 0): 250, (2, 1): 30000, (2, 0): 60000, (4, 1): 2 * 10**9, (4, 0): 4 * 10**9}.get((iw, signed), 2**32 - 1)
    return dict(kind=_ffi.K_DICT, param=iw | (signed << 8), param2=dict_len)


VARIANTS = {
    "copy1": dict(kind=_ffi.K_COPY, param=1), "copy2": dict(kind=_ffi.K_COPY, param=2), "copy4": dict(kind=_ffi.K_COPY, param=4),
    "copy8": dict(kind=_ffi.K_COPY, param=8), "copy16": dict(kind=_ffi.K_COPY, param=16),
    "dec128_i16": dict(kind=_ffi.K_DEC128, param=2), "dec128_i32": dict(kind=_ffi.K_DEC128, param=4),
    "dec128_i64": dict(kind=_ffi.K_DEC128, param=8),
    "str32": dict(kind=_ffi.K_STR32), "str64": dict(kind=_ffi.K_STR64),
    "fixed1": dict(kind=_ffi.K_FIXED_BINARY, param=1), "fixed12": dict(kind=_ffi.K_FIXED_BINARY, param=12),
    "fixed13": dict(kind=_ffi.K_FIXED_BINARY, param=13), "fixed16": dict(kind=_ffi.K_FIXED_BINARY, param=16),
    "bool": dict(kind=_ffi.K_BOOL), "date64": dict(kind=_ffi.K_DATE64),
    "mul_i32_1e6": dict(kind=_ffi.K_MUL_I32, param=1000000), "mul_i32_1e3": dict(kind=_ffi.K_MUL_I32, param=1000),
    "mul_i64_1e6": dict(kind=_ffi.K_MUL_I64, param=1000000),
    "div_i64_1000": dict(kind=_ffi.K_DIV_I64, param=1000), "div_i64_86400": dict(kind=_ffi.K_DIV_I64, param=86400),
}
for _iw in (1, 2, 4, 8):
    for _signed in (1, 0):
        VARIANTS["dict_%s%d" % ("i" if _signed else "u", 8 * _iw)] = _dict_variant(_iw, _signed)


# VARIANTS = what a selection vector can take (the gather suite runs them all); FLAT_VARIANTS = every decode kind
FLAT_VARIANTS = dict(VARIANTS)
FLAT_VARIANTS.update({
    "duration_mul_1e6": dict(kind=_ffi.K_DURATION, param=1000000), "duration_mul_1e3": dict(kind=_ffi.K_DURATION, param=1000),
    "duration_mul_1": dict(kind=_ffi.K_DURATION, param=1), "duration_div_1000": dict(kind=_ffi.K_DURATION, param=-1000),
    "duration_div_7": dict(kind=_ffi.K_DURATION, param=-7),
    "div_i64_1": dict(kind=_ffi.K_DIV_I64, param=1), "div_i64_1e6": dict(kind=_ffi.K_DIV_I64, param=1000000),
    "interval_months": dict(kind=_ffi.K_INTERVAL_MONTHS), "interval_mdn": dict(kind=_ffi.K_INTERVAL_MDN),
    "narrow_4_2": dict(kind=_ffi.K_NARROW, param=4 | (2 << 8)), "narrow_8_2": dict(kind=_ffi.K_NARROW, param=8 | (2 << 8)),
    "narrow_8_4": dict(kind=_ffi.K_NARROW, param=8 | (4 << 8)),
    "half_float": dict(kind=_ffi.K_HALF_FLOAT), "null": dict(kind=_ffi.K_NULL),
    "strview_0buf": dict(kind=_ffi.K_STRVIEW, nbuf=0), "strview_1buf": dict(kind=_ffi.K_STRVIEW, nbuf=1),
    "strview_3buf": dict(kind=_ffi.K_STRVIEW, nbuf=3),
    "list32": dict(kind=_ffi.K_LIST32), "list64": dict(kind=_ffi.K_LIST64),
    "list32_windows": dict(kind=_ffi.K_LIST32, windows=True), "list64_windows": dict(kind=_ffi.K_LIST64, windows=True),
    "struct": dict(kind=_ffi.K_STRUCT),
})
I64_MIN, I64_MAX = -2**63, 2**63 - 1
NANOS = [-1, -999, -1000, -1001, 999, 1000, I64_MIN, I64_MAX]      # where a division truncating toward zero differs from its neighbours
VIEW_BUFFERS = [64, 41, 1000]                                      # lengths of the variadic buffers of a string-view column
VIEW_BASE = 0x7100_0000_0000                                       # their addresses are made up: the kernel never follows them


def _scatter(buf, values, rows, rng):
    """the special values onto rows picked from `rows` (the column's own valid rows), each at least once while rows last"""
    if len(rows):
        values = np.array(values * 4, buf.dtype)
        picked = rng.permutation(rows)[: len(values)]
        buf[picked] = values[: len(picked)]


def parent_rows(parent, total):
    """validity of rows [0, total) of a child under parent = (words, rows per parent row)"""
    bits = np.unpackbits(np.ascontiguousarray(parent[0]).view(np.uint8), bitorder="little").astype(bool)
    idx = np.minimum(np.arange(total) // max(parent[1], 1), len(bits) - 1)
    return bits[idx]


def make_column(variant, nrows, row_offset, nulls, rng, parent=None):
    """One source column of FLAT_VARIANTS[variant]: `nrows` rows at Arrow array offset `row_offset`.  nulls: "bitmap" (random
    bitmap, null_count -1; the NULL rows hold values that would raise a status flag if they were looked at), "count0" (a
    random bitmap the kernel has to ignore: null_count 0), "none", "all_valid" or "all_null" (bitmaps of ones / of zeros,
    null_count -1).  parent = (validity words, rows per parent row) makes it the child of a struct (0 or 1 rows per parent
    row) or of a fixed-size list: the rows the parent makes NULL hold the same offending values as the column's own."""
    col = dict(FLAT_VARIANTS[variant], nrows=nrows, row_offset=row_offset, name="%s/%s/n%d/o%d" % (variant, nulls, nrows, row_offset))
    kind, param = col["kind"], col.get("param", 0)
    total = row_offset + nrows + PAD_ROWS
    bitmap = rng.integers(0, 256, (total + 63) // 64 * 8 + 8, dtype=np.uint8)
    if nulls in ("all_valid", "all_null"):
        bitmap[:] = 0xFF if nulls == "all_valid" else 0
    null = ~np.unpackbits(bitmap, bitorder="little")[:total].astype(bool) if nulls in ("bitmap", "all_null") else np.zeros(total, bool)
    if nulls != "none":
        col.update(validity=bitmap, null_count=0 if nulls == "count0" else -1)
    if parent is not None:
        col.update(out_aux=np.ascontiguousarray(parent[0]), parent_div=parent[1], depth=1,
                   name=col["name"] + "/parent_div%d" % parent[1])
        null[row_offset: row_offset + nrows] |= ~parent_rows(parent, nrows)
    mine = row_offset + np.nonzero(~null[row_offset: row_offset + nrows])[0]      # the column's own rows that are valid
    if kind == _ffi.K_COPY:
        buf1 = rng.integers(0, 256, total * param, dtype=np.uint8)
    elif kind == _ffi.K_FIXED_BINARY:
        buf1 = rng.integers(0, 256, total * param, dtype=np.uint8)
        col["ptr_base"] = PTR_BASE
    elif kind == _ffi.K_BOOL:
        buf1 = rng.integers(0, 256, (total + 7) // 8, dtype=np.uint8)
    elif kind == _ffi.K_DEC128:
        lim = 1 << (8 * param - 1)
        v = rng.integers(-lim, lim - 1, total, endpoint=True).astype(np.int64)
        _scatter(v, [-lim, lim - 1, 0, -1, 1, -2], mine, rng)                      # both limits on valid rows
        halves = np.stack([v, v >> 63], axis=1)
        halves[null] = rng.integers(-2**63, 2**63 - 1, (int(null.sum()), 2), endpoint=True)   # out of range, bad upper half
        buf1 = halves.reshape(-1)
    elif kind in (_ffi.K_STR32, _ffi.K_STR64):
        lens = rng.choice([0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16, 29, 40], total)
        off = 5 + np.concatenate([[0], np.cumsum(lens)])      # every length at every payload misalignment
        buf1 = off.astype(np.int32 if kind == _ffi.K_STR32 else np.int64)
        col.update(buf2=rng.integers(1, 256, int(off[-1]), dtype=np.uint8), buf2_len=int(off[row_offset + nrows]), ptr_base=PTR_BASE)
    elif kind == _ffi.K_DATE64:
        buf1 = rng.integers(-3 * 10**14, 3 * 10**14, total).astype(np.int64)      # +- 9500 years of milliseconds
        buf1[rng.integers(0, total, 6)] = [-1, 0, 86400000, -86400000, 86399999, -86400001]
    elif kind == _ffi.K_MUL_I32:
        buf1 = rng.integers(-2**31, 2**31 - 1, total, endpoint=True).astype(np.int32)
    elif kind == _ffi.K_MUL_I64:
        lim = (2**63 - 1) // param
        buf1 = rng.integers(-lim, lim, total, endpoint=True).astype(np.int64)
        _scatter(buf1, [-lim, lim], mine, rng)                                     # the last values that do not overflow, on valid rows
        buf1[null] = rng.integers(2**62, 2**63 - 1, int(null.sum()))              # would overflow
    elif kind == _ffi.K_DIV_I64:
        buf1 = rng.integers(-2**63, 2**63 - 1, total, endpoint=True).astype(np.int64)
        buf1[rng.integers(0, total, 6)] = [-1, 0, param, -param, param - 1, 1 - param]
    elif kind == _ffi.K_DICT:
        iw, signed, dict_len = param & 0xFF, (param >> 8) & 1, col["param2"]
        v = rng.integers(0, dict_len, total).astype(np.uint64)
        v[rng.integers(0, total, 2)] = [0, dict_len - 1]
        v[null] = ONES if (signed or iw == 8) else np.uint64(2**(8 * iw) - 1)        # -1, or past the dictionary
        buf1 = v.astype(np.dtype("u%d" % iw))
    elif kind == _ffi.K_DURATION and param > 0:
        lim = I64_MAX // param
        buf1 = rng.integers(-lim, lim, total, endpoint=True).astype(np.int64)
        _scatter(buf1, [-lim, lim], mine, rng)                                     # the last values that do not overflow
        if param > 1:
            buf1[null] = rng.integers(2**62, I64_MAX, int(null.sum())) * rng.choice([-1, 1], int(null.sum()))   # would overflow
    elif kind == _ffi.K_DURATION:
        buf1 = rng.integers(I64_MIN, I64_MAX, total, endpoint=True).astype(np.int64)
        _scatter(buf1, NANOS + [param, -param, -param - 1, param + 1, 0], np.arange(row_offset, row_offset + nrows), rng)
    elif kind == _ffi.K_INTERVAL_MONTHS:
        buf1 = rng.integers(-2**31, 2**31 - 1, total, endpoint=True).astype(np.int32)
    elif kind == _ffi.K_INTERVAL_MDN:
        nanos = rng.integers(I64_MIN, I64_MAX, total, endpoint=True).astype(np.int64)
        _scatter(nanos, NANOS + [0, 1, 1001], np.arange(row_offset, row_offset + nrows), rng)
        buf1 = np.stack([rng.integers(I64_MIN, I64_MAX, total, endpoint=True).astype(np.int64), nanos], axis=1).reshape(-1)   # months | days, nanos
    elif kind == _ffi.K_NARROW:
        sw, dw = param & 0xFF, (param >> 8) & 0xFF
        lim, src_lim = 1 << (8 * dw - 1), 1 << (8 * sw - 1)
        v = rng.integers(-lim, lim - 1, total, endpoint=True).astype(np.int64)
        _scatter(v, [-lim, lim - 1, 0, -1], mine, rng)                             # both limits of the destination
        mag = rng.integers(lim, src_lim - 1, int(null.sum()), endpoint=True)
        v[null] = np.where(rng.random(len(mag)) < 0.5, mag, -mag - 1)              # out of range on either side
        buf1 = v.astype(np.int32 if sw == 4 else np.int64)
    elif kind == _ffi.K_HALF_FLOAT:
        buf1 = ((int(rng.integers(0, 65536)) + np.arange(total)) & 0xFFFF).astype(np.uint16)       # consecutive bit patterns
    elif kind in (_ffi.K_NULL, _ffi.K_STRUCT):
        buf1 = None
    elif kind == _ffi.K_STRVIEW:
        nbuf = col.pop("nbuf")
        sizes = VIEW_BUFFERS[:nbuf]
        lens = np.array(list(range(17)) + [40])[(int(rng.integers(0, 18)) + np.arange(total)) % 18]     # every length 0..16 and 40
        if nbuf == 0:
            lens = np.where(null, lens, lens % 13)                                  # without data buffers only inline views are sound
        views = rng.integers(1, 256, (total, 16), dtype=np.uint8)                   # inline views: pad bytes are non-zero garbage
        words = views.view(np.int32)                                                # [len, prefix, buffer index, offset]
        words[:, 0] = lens
        long = lens > 12
        bi = rng.integers(0, max(nbuf, 1), total)
        room = np.array(sizes + [0])[bi if nbuf else np.full(total, 0)] - lens
        at = np.where(rng.random(total) < 0.4, 0, np.where(rng.random(total) < 0.6, room, rng.integers(0, 25, total) % (np.abs(room) + 1)))
        words[long, 2], words[long, 3] = bi[long], at[long]                         # at the first and at the last byte of each buffer
        gone = null & long                                                          # NULL rows: must not be followed, must not raise status
        words[gone, 2] = np.where(rng.random(total) < 0.5, -1, nbuf)[gone]
        words[gone, 3] = np.where(rng.random(total) < 0.5, -7, 2**31 - 1)[gone]
        buf1 = views.reshape(-1)
        if nbuf:
            col.update(buf2=np.array([[VIEW_BASE + (k << 32) + 3, size] for k, size in enumerate(sizes)], np.uint64).reshape(-1))
        col["buf2_len"] = nbuf
    elif kind in (_ffi.K_LIST32, _ffi.K_LIST64):
        lens = rng.choice([0, 0, 1, 2, 3, 17, 900], total)                          # empty and long lists mixed
        off = 5 + np.concatenate([[0], np.cumsum(lens)])
        buf1 = off.astype(np.int32 if kind == _ffi.K_LIST32 else np.int64)
        col["param"] = int(off[row_offset + nrows])                                 # child length
        if col.pop("windows", False):      # a list inside lists: its windows start where the outer offsets say, also inside tiles
            col["window_starts"] = np.array([0] + [r for r in (3, 40, 700, 2047, 2348, 2349, 4000) if r < nrows], np.int64)
    else:
        raise AssertionError(kind)
    col["buf1"] = buf1
    return col


def _width(col):
    return po.out_width(col["kind"], col.get("param", 0))


def _reference_args(col):
    args = {k: col[k] for k in ("param", "param2", "validity", "null_count", "row_offset", "buf2", "buf2_len", "ptr_base", "window_starts") if k in col}
    if "out_aux" in col:
        args["parent"] = (col["out_aux"], col["parent_div"])
    return args


def flat_reference(col):
    """What check_job expects of an ordinary flat task: (data bytes, validity words with pad bits ones, status = the OR of the
    reference's per-row bits).  The Arrow null type clears whole words, pad bits included, like the oracle's memset."""
    data, ok, err = decode_column_reference(col["kind"], col["nrows"], col["buf1"], **_reference_args(col))
    words = _words_of(ok)
    if col["kind"] == _ffi.K_NULL:
        words[:] = 0
    return data.reshape(-1), words, int(np.bitwise_or.reduce(err)) if len(err) else 0


# ------------------------------------------------------------------------------------------------ selections
def make_sel(nrows, counts, rng):
    """One ascending index list per 2048-row window with the wanted number of rows (clipped to the window's size; None =
    every row).  A window with two rows or more selects its first and its last row, single rows alternate between them."""
    sel = []
    for w in range((nrows + WIN - 1) // WIN):
        m = min(WIN, nrows - w * WIN)
        c = m if counts[w % len(counts)] is None else min(counts[w % len(counts)], m)
        if c == m:
            s = np.arange(m)
        elif c == 0:
            s = np.zeros(0, np.int64)
        elif c == 1:
            s = np.array([0 if w % 2 else m - 1])
        else:
            s = np.sort(np.concatenate([[0, m - 1], 1 + rng.choice(m - 2, c - 2, replace=False)]))
        sel.append(s.astype(np.int64))
    return sel


def _sel_arrays(sel):
    flat = np.full(max(len(sel), 1) * WIN, SEL_FILL, np.uint32)
    for w, s in enumerate(sel):
        flat[w * WIN: w * WIN + len(s)] = s
    return flat, np.array([len(s) for s in sel] + [0], np.uint32)


# ------------------------------------------------------------------------------------------------ running a plan
def _dev(torch, a):
    """numpy array -> device bytes, padded as IPC buffers are (to 8 bytes, and never empty)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(16 - len(b) % 8, np.uint8)])).cuda()


def run_plan(ctx, torch, jobs, sels, out_validity=True):
    """jobs = [(column, key into sels or None for an ordinary flat task)], sels = {key: index lists per window}.  One Plan,
    one launch.  -> ([(data bytes incl. the sentinel tail, validity words incl. the guard word) per job], status).
    out_validity=False: the tasks get no out_validity (the preset words come back untouched)."""
    keep, dsel = [], {}
    for key, sel in sels.items():
        flat, counts = _sel_arrays(sel)
        dsel[key] = (torch.from_numpy(flat.view(np.int32)).cuda(), torch.from_numpy(counts.view(np.int32)).cuda(), sum(len(s) for s in sel))
    tasks, outs = [], []
    for col, key in jobs:
        total = dsel[key][2] if key is not None else col["nrows"]
        d1, dv, d2 = (_dev(torch, col["buf1"]) if col["buf1"] is not None else None), (_dev(torch, col["validity"]) if "validity" in col else None), \
            (_dev(torch, col["buf2"]) if "buf2" in col else None)
        if "window_starts" in col:      # a nested list: buf2 = the window starts, buf2_len = their number
            d2 = _dev(torch, col["window_starts"])
        daux = _dev(torch, col["out_aux"]) if "out_aux" in col else None
        out = torch.full((total * _width(col) + 64 + (-total * _width(col)) % 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        outv = torch.full(((total + 63) // 64 * 8 + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        keep += [d1, dv, d2, daux]
        outs.append((out, outv))
        tasks.append(da.make_task(col["kind"], col["nrows"], d1.data_ptr() if d1 is not None else 0, out.data_ptr(),
                                  validity=dv.data_ptr() if dv is not None else 0,
                                  buf2=d2.data_ptr() if d2 is not None else 0, out_validity=outv.data_ptr() if out_validity else 0,
                                  out_aux=daux.data_ptr() if daux is not None else 0, parent_div=col.get("parent_div", 0), depth=col.get("depth", 0),
                                  ptr_base=col.get("ptr_base", 0), row_offset=col["row_offset"],
                                  buf2_len=len(col["window_starts"]) if "window_starts" in col else col.get("buf2_len", 0), param=col.get("param", 0),
                                  param2=col.get("param2", 0), null_count=col.get("null_count", -1),
                                  sel=dsel[key][0].data_ptr() if key is not None else 0,
                                  sel_count=dsel[key][1].data_ptr() if key is not None else 0))
    plan = da.Plan(ctx, tasks)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    status = plan.status()
    got = [(out.cpu().numpy(), outv.cpu().numpy().view(np.uint64)) for out, outv in outs]
    plan.close()
    return got, status


def check_job(col, sel, got, want=None):
    """The four assertions on one task's output.  sel None = an ordinary flat task (every row, in place).  Returns the
    expected status of the task."""
    data, words = got
    if sel is None:
        sel = make_sel(col["nrows"], [None], None)
    want_data, want_words, want_status = want if want is not None else gather_reference(col["kind"], col["nrows"], col["buf1"], sel, **_reference_args(col))
    w, total, where = _width(col), sum(len(s) for s in sel), col.get("name", "")
    if not np.array_equal(data[: total * w], want_data):
        bad = np.nonzero(np.any(data[: total * w].reshape(-1, w) != want_data.reshape(-1, w), axis=1))[0]
        raise AssertionError("%s: %d of %d output rows differ, first %d: got %s want %s" % (
            where, len(bad), total, bad[0], data[bad[0] * w: bad[0] * w + w].tolist(), want_data[bad[0] * w: bad[0] * w + w].tolist()))
    assert (data[total * w:] == SENTINEL).all(), (where, "bytes behind the last output row were written")
    assert len(words) == (total + 63) // 64 + 1
    if not np.array_equal(words[:-1], want_words):
        bad = np.nonzero(words[:-1] != want_words)[0]
        raise AssertionError("%s: %d validity words differ, first %d of %d: got %016x want %016x" % (
            where, len(bad), bad[0], len(want_words), int(words[bad[0]]), int(want_words[bad[0]])))
    assert words[-1] == ONES, (where, "the guard word behind the validity words lost bits")
    return want_status


# ------------------------------------------------------------------------------------------------ status
def _dec(values, width):
    """python ints -> decimal128 halves; (lower, upper) tuples are taken as they are"""
    out = []
    for v in values:
        out += list(v) if isinstance(v, tuple) else [v & (2**64 - 1), (v >> 64) & (2**64 - 1)]
    return dict(kind=_ffi.K_DEC128, param=width, buf1=np.array(out, np.uint64))


def _status_cases():
    cases = {}
    for w in (2, 4, 8):
        lim = 1 << (8 * w - 1)
        cases["dec128_i%d_above" % (8 * w)] = (lambda bad, w=w, lim=lim: _dec([lim if bad else lim - 1], w), _ffi.ST_DECIMAL_RANGE, True)
        cases["dec128_i%d_below" % (8 * w)] = (lambda bad, w=w, lim=lim: _dec([-lim - 1 if bad else -lim], w), _ffi.ST_DECIMAL_RANGE, True)
        cases["dec128_i%d_upper_half" % (8 * w)] = (lambda bad, w=w: _dec([(5, 1) if bad else 5], w), _ffi.ST_DECIMAL_RANGE, True)
    cases["dec128_i64_upper_half_of_a_negative"] = (lambda bad: _dec([(2**64 - 5, 2**64 - 2) if bad else -5], 8), _ffi.ST_DECIMAL_RANGE, True)
    big = (2**63 - 1) // 1000
    cases["mul_i64_above"] = (lambda bad: dict(kind=_ffi.K_MUL_I64, param=1000, buf1=np.array([big + 1 if bad else big], np.int64)), _ffi.ST_MUL_OVERFLOW, True)
    cases["mul_i64_below"] = (lambda bad: dict(kind=_ffi.K_MUL_I64, param=1000, buf1=np.array([-big - 2 if bad else -big], np.int64)), _ffi.ST_MUL_OVERFLOW, True)
    for iw in (1, 2, 4):
        cases["dict_i%d_negative" % (8 * iw)] = (lambda bad, iw=iw: dict(kind=_ffi.K_DICT, param=iw | 256, param2=90, buf1=np.array(
            [-1 if bad else 3], np.dtype("i%d" % iw))), _ffi.ST_INDEX_RANGE, True)
        cases["dict_u%d_past_the_dictionary" % (8 * iw)] = (lambda bad, iw=iw: dict(kind=_ffi.K_DICT, param=iw, param2=90, buf1=np.array(
            [200 if bad else 89], np.dtype("u%d" % iw))), _ffi.ST_DICT_INDEX, True)
    cases["dict_u64_wider_than_uint32"] = (lambda bad: dict(kind=_ffi.K_DICT, param=8, param2=90, buf1=np.array([2**32 if bad else 3], np.uint64)),
                                           _ffi.ST_INDEX_RANGE, True)
    cases["dict_i64_negative"] = (lambda bad: dict(kind=_ffi.K_DICT, param=8 | 256, param2=90, buf1=np.array([-1 if bad else 3], np.int64)),
                                  _ffi.ST_INDEX_RANGE, True)
    cases["dict_i32_equal_to_dict_len"] = (lambda bad: dict(kind=_ffi.K_DICT, param=4 | 256, param2=90, buf1=np.array([90 if bad else 89], np.int32)),
                                           _ffi.ST_DICT_INDEX, True)
    return cases


STATUS_CASES = _status_cases()


def _status_column(make, flag_row, nrows, rng):
    """`nrows` good rows (the case's good value) with the case's bad value at `flag_row`; every row valid except where the
    caller clears bits afterwards."""
    good, bad = make(False), make(True)
    per = len(good["buf1"])
    buf1 = np.tile(good["buf1"], nrows + PAD_ROWS)
    buf1[flag_row * per: (flag_row + 1) * per] = bad["buf1"]
    return dict(good, buf1=buf1, nrows=nrows, row_offset=0, validity=np.full((nrows + PAD_ROWS + 63) // 64 * 8 + 8, 0xFF, np.uint8), null_count=-1)

"""Kernel-level encode tasks (kernels_encode.hip) for test_encode_reference_host.py and test_gpu_encode_tasks.py: DuckDB
vectors built to hurt, a plain numpy restatement of ArrowAppender (encode_reference: it calls neither the package nor the
oracle), one Plan per list of columns (run_plan) and the assertions on a task's output (check_task).

A column is a dict: kind, n, large (int64 offsets), words (DuckDB validity words, None = pointer 0), src (the vector's
bytes), heap / ptr_base (strings), width (COPY / DEC128), bitmap (False = no out_validity: the list-offsets form of
COPY), vpos (byte phase of out_validity), and what the builder started from -- ok (the rows it meant to be valid) and
values() (their Python values) --, which only the host test looks at.

CASES maps a name to a builder of one plan's columns; both test files run the same names (the host test leaves out
GPU_ONLY, the two 8 MiB strings).  The shapes follow the kernels: 8 rows per thread (bool), 64 rows per bitmap lane, 256
rows per sub-block, 2048 per tile, LDS windows of 8192 - (position & 15) bytes, 4 look-back predecessors per step."""
import zlib

import numpy as np

K_ENC_COPY, K_ENC_DEC128, K_ENC_BOOL, K_ENC_STR32, K_ENC_VALIDITY, K_ENC_LIST32 = 32, 33, 34, 35, 36, 37
ST_OFFSET_OVERFLOW = 32
INT32_MAX = 2**31 - 1

SENTINEL = 0xEE
GUARD = 64                 # sentinel bytes in front of and behind every output buffer
TILE, SUB, WINDOW = 2048, 256, 8192
ROWS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4095, 4097, 6145]
FORMS = ["none", "all_valid", "random", "all_null", "first_null", "last_null"]
VPOS = [0, 1, 3, 5]
PTR_BASE = 0x7F0000001000
HEAP_PHASE = 1             # the heap's first byte sits at an odd address
HEAP_FIRST = 7             # ... and its first string at an odd position inside it
FAR_POINTER = 0x6EAD00000000


# ------------------------------------------------------------------------------------------------ the reference
def ragged_copy(dst, dstart, src, sstart, lens):
    """dst[dstart[i]: dstart[i] + lens[i]] = src[sstart[i]: sstart[i] + lens[i]] for every i"""
    dstart, sstart, lens = (np.asarray(a, np.int64) for a in (dstart, sstart, lens))
    big = lens >= 1024
    for i in np.nonzero(big)[0]:
        dst[dstart[i]: dstart[i] + lens[i]] = src[sstart[i]: sstart[i] + lens[i]]
    small = ~big & (lens > 0)
    ln = lens[small]
    if ln.size:
        k = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        dst[np.repeat(dstart[small], ln) + k] = src[np.repeat(sstart[small], ln) + k]


def _row_bits(col):
    """validity of the n rows as the words say it (the pad bits behind row n are not looked at)"""
    if col["words"] is None:
        return np.ones(col["n"], bool)
    return np.unpackbits(col["words"].view(np.uint8), bitorder="little")[: col["n"]].astype(bool)


def _offsets(lens, large):
    """-> (offset bytes, bytes behind them that may hold anything, status, offsets).  int32 offsets are defined up to the last
    one that fits: ArrowAppender throws at the first that does not, and a plan with the overflow bit is refused whatever
    the rest holds."""
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    if large:
        return off.astype("<i8").view(np.uint8), 0, 0, off
    fits = int(np.searchsorted(off, INT32_MAX, side="right"))
    return off[:fits].astype("<i4").view(np.uint8), 4 * (len(off) - fits), (ST_OFFSET_OVERFLOW if fits < len(off) else 0), off


def encode_reference(col):
    """ArrowAppender on one column -> dict(bitmap, data, aux: uint8 arrays or None = no such buffer; loose: bytes of the
    data buffer behind `data` that are allocated but may hold anything; nulls; status).  A column of 0 rows defines no
    byte of any buffer, and VALIDITY alone none of its (mandatory) data buffer."""
    n, kind = col["n"], col["kind"]
    empty = np.zeros(0, np.uint8)
    out = dict(bitmap=None, data=empty, aux=None, loose=0, nulls=0, status=0)
    ok = _row_bits(col)
    if col.get("bitmap", True):
        nb = (n + 7) // 8
        bm = np.full(nb, 0xFF, np.uint8) if col["words"] is None else col["words"].view(np.uint8)[:nb].copy()
        if n & 7:
            bm[-1] |= (0xFF << (n & 7)) & 0xFF
        out.update(bitmap=bm, nulls=n - int(ok.sum()))
    src = col["src"]
    if kind == K_ENC_VALIDITY:
        return out
    if n == 0:
        out.update(aux=empty if kind == K_ENC_STR32 else None)
        return out
    if kind == K_ENC_COPY:
        out["data"] = src[: n * col["width"]].copy()
    elif kind == K_ENC_DEC128:
        v = src[: n * col["width"]].view("<i%d" % col["width"]).astype(np.int64)
        out["data"] = np.stack([v, v >> 63], axis=1).astype("<i8").view(np.uint8).reshape(-1)
    elif kind == K_ENC_BOOL:
        bit = ~(ok & (src[:n] == 0))
        out["data"] = np.packbits(np.concatenate([bit, np.ones(-n % 8, bool)]), bitorder="little")
    elif kind == K_ENC_LIST32:
        ln = src.view("<u8").reshape(n, 2)[:, 1].astype(np.int64)       # the full 64-bit length field
        ln[~ok] = 0
        out["data"], out["loose"], out["status"], _ = _offsets(ln, col["large"])
    elif kind == K_ENC_STR32:
        s = src.reshape(n, 16)
        ln = s.view("<u4")[:, 0].astype(np.int64)
        ln[~ok] = 0
        out["data"], out["loose"], out["status"], off = _offsets(ln, col["large"])
        data = np.zeros(int(off[-1]), np.uint8)
        r = np.nonzero(ok & (ln <= 12))[0]
        ragged_copy(data, off[r], src, 16 * r + 4, ln[r])                                # inline: bytes 4.. of the string_t
        r = np.nonzero(ok & (ln > 12))[0]
        ptr = s.view("<u8")[r, 1]
        ragged_copy(data, off[r], col["heap"], (ptr - np.uint64(col["ptr_base"])).astype(np.int64), ln[r])
        out["aux"] = data
    else:
        raise AssertionError(kind)
    return out


# ------------------------------------------------------------------------------------------------ columns
def validity_form(form, n, rng):
    """-> the rows meant to be valid, or None for a column without validity words"""
    if form == "none":
        return None
    ok = np.ones(n, bool)
    if form == "random":
        ok = rng.random(n) < 0.8
    elif form == "all_null":
        ok[:] = False
    elif form == "first_null":
        ok[:1] = False
    elif form == "last_null":
        ok[-1:] = False
    else:
        assert form == "all_valid", form
    return ok


def _words(ok, rng):
    """DuckDB validity words of a vector; the bits behind its last row are whatever the last word held"""
    if ok is None:
        return None
    pad = rng.random(-len(ok) % 64) < 0.5
    return np.packbits(np.concatenate([ok, pad]), bitorder="little").view(np.uint64).copy()


def _column(kind, n, ok, rng, name, **kw):
    col = dict(kind=kind, n=n, large=False, ok=ok, words=_words(ok, rng), heap=None, ptr_base=0, width=0, bitmap=True, vpos=0, name=name)
    col.update(kw)
    return col


def _null_to_none(values, ok):
    return values if ok is None else [v if o else None for v, o in zip(values, ok)]


def fixed_column(spec, n, ok, rng, name, vpos=0):
    """spec: copy1..copy16, offsets1..offsets16 (COPY without a bitmap), dec2 / dec4 / dec8, bool, validity"""
    if spec.startswith("copy") or spec.startswith("offsets"):
        w = int(spec.lstrip("copyoffsets"))
        src = rng.integers(0, 256, n * w, dtype=np.uint8)
        vals = (lambda: [bytes(r) for r in src.reshape(n, 16)]) if w == 16 else (lambda: src.view("<u%d" % w).tolist())
        return _column(K_ENC_COPY, n, ok, rng, name, src=src, width=w, bitmap=spec.startswith("copy"), vpos=vpos,
                       values=lambda: _null_to_none(vals(), ok if spec.startswith("copy") else None))
    if spec.startswith("dec"):
        w = int(spec[3:])
        lim = 1 << (8 * w - 1)
        v = rng.integers(-lim, lim - 1, n, endpoint=True).astype("<i%d" % w)
        special = np.array([-lim, lim - 1, -1, 0], v.dtype)
        at = rng.permutation(n)[:4]
        v[at] = special[: len(at)]
        return _column(K_ENC_DEC128, n, ok, rng, name, src=v.view(np.uint8).copy(), width=w, vpos=vpos,
                       values=lambda: _null_to_none([int(x) for x in v], ok))
    if spec == "bool":
        src = rng.choice(np.array([0, 1, 2, 0xFF], np.uint8), n)
        return _column(K_ENC_BOOL, n, ok, rng, name, src=src, vpos=vpos, values=lambda: _null_to_none((src != 0).tolist(), ok))
    assert spec == "validity", spec
    return _column(K_ENC_VALIDITY, n, ok, rng, name, src=np.zeros(16, np.uint8), vpos=vpos, values=lambda: _null_to_none([0] * n, ok))


def string_column(lens, ok, rng, name, large=False, ptr_base=0, owners="long", order=None, vpos=0):
    """string_t rows of the given lengths.  The valid rows' bytes are `text`, in row order: what the data buffer has to hold.
    owners: which rows own heap bytes -- "long" (DuckDB's own heaps: the valid rows longer than 12 bytes) or "all" (every
    valid row, as in a vector decoded from Arrow buffers; the heap bytes of an inline row differ from its inline bytes, which
    must win).  order: the rows in heap order (None = row order).  Inline pad bytes and the prefix of long rows are noise.
    NULL rows hold a length of 0xFFFFFFFF, or of 13..40 with a pointer far outside the heap."""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    valid = np.ones(n, bool) if ok is None else ok
    eff = np.where(valid, lens, 0)
    tstart = np.cumsum(eff) - eff
    text = rng.integers(0, 256, int(eff.sum()), dtype=np.uint8)
    long_ = valid & (eff > 12)
    hlen = np.where(long_ if owners == "long" else valid, eff, 0)
    order = np.arange(n) if order is None else np.asarray(order)
    hstart = np.zeros(n, np.int64)
    hstart[order] = HEAP_FIRST + np.cumsum(hlen[order]) - hlen[order]
    heap = rng.integers(0, 256, HEAP_FIRST + int(hlen.sum()) + 16, dtype=np.uint8)
    rows = np.nonzero(long_)[0]
    ragged_copy(heap, hstart[rows], text, tstart[rows], eff[rows])
    s = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    s.view("<u4")[:, 0] = eff
    s.view("<u8")[rows, 1] = (ptr_base + hstart[rows]).astype(np.uint64)
    flat = s.reshape(-1)
    rows = np.nonzero(valid & (eff <= 12))[0]
    ragged_copy(flat, 16 * rows + 4, text, tstart[rows], eff[rows])
    gone = np.nonzero(~valid)[0]
    junk = rng.random(len(gone)) < 0.5
    s.view("<u4")[gone, 0] = np.where(junk, 0xFFFFFFFF, rng.integers(13, 41, len(gone))).astype(np.uint32)
    s.view("<u8")[gone, 1] = np.uint64(FAR_POINTER) + rng.integers(0, 2**30, len(gone)).astype(np.uint64)
    return _column(K_ENC_STR32, n, ok, rng, name, src=flat, heap=heap, ptr_base=ptr_base, large=large, vpos=vpos, text=text, hstart=hstart,
                   values=lambda: [text[a: a + l].tobytes() if v else None for a, l, v in zip(tstart.tolist(), eff.tolist(), valid.tolist())])


def list_column(lens, ok, rng, name, large=False, vpos=0):
    """list_entry_t rows {offset, length}.  NULL rows hold a length of 2**40.  `lens` are Python ints or an integer array."""
    n = len(lens)
    valid = np.ones(n, bool) if ok is None else ok
    want = [int(l) if v else 0 for l, v in zip(lens, valid.tolist())]
    e = np.zeros((n, 2), "<u8")
    e[:, 0] = rng.integers(0, 2**62, n)                       # the kernel has no use for the child offset
    e[:, 1] = np.where(valid, np.array([int(l) for l in lens], np.uint64), np.uint64(2**40))
    ends = []
    for l in want:                                            # Python integers: exact whatever the lengths
        ends.append((ends[-1] if ends else 0) + l)
    starts = [0] + ends[:-1]
    small = (ends[-1] if ends else 0) < 10**6
    return _column(K_ENC_LIST32, n, ok, rng, name, src=e.view(np.uint8).reshape(-1), large=large, vpos=vpos, ends=ends,
                   values=(lambda: [list(range(a, b)) if v else None for a, b, v in zip(starts, ends, valid.tolist())]) if small else None)


# ------------------------------------------------------------------------------------------------ the cases
def _every_other_wave_shuffled(n, rng):
    order = np.arange(n)
    for w in range(0, n // 64, 2):
        order[64 * w: 64 * w + 64] = rng.permutation(order[64 * w: 64 * w + 64])
    return order


def fixed_kinds(rng):
    """COPY at every width with and without a bitmap, DEC128 from 2, 4 and 8 bytes, BOOL and VALIDITY alone, at every row
    count and validity form: 1620 tasks for one launch of encode_fixed.  out_validity takes the byte phases 0, 1, 3 and 5."""
    specs = ["copy%d" % w for w in (1, 2, 4, 8, 16)] + ["offsets%d" % w for w in (1, 2, 4, 8, 16)] + ["dec2", "dec4", "dec8", "bool", "validity"]
    cols = []
    for i, n in enumerate(ROWS):
        for j, form in enumerate(FORMS):
            for k, spec in enumerate(specs):
                cols.append(fixed_column(spec, n, validity_form(form, n, rng), rng, "%s/%s/n%d" % (spec, form, n), vpos=VPOS[(i + j + k) % 4]))
    for n in ROWS:       # the 8-byte store exists from 64 rows on: every such row count meets every phase, with every kind of bitmap
        for spec in ("copy4", "dec8", "bool", "validity"):
            assert {c["vpos"] for c in cols if c["n"] == n and c["name"].startswith(spec + "/")} == set(VPOS) or n < 64
    return cols


def _mixed(n, rng):
    return rng.integers(0, 41, n)


def string_seams(rng):
    """Strings of 0..40 bytes at every row count and validity form, int32 and int64 offsets, the three heap layouts in turn."""
    cols = []
    for i, n in enumerate(ROWS):
        for j, form in enumerate(FORMS):
            for large in (False, True):
                k = i + j + large
                layout = ("row_order", "shuffled", "long_only")[k % 3]
                cols.append(string_column(_mixed(n, rng), validity_form(form, n, rng), rng, "str/%s/%s/n%d/%d" % (layout, form, n, 64 if large else 32),
                                          large=large, ptr_base=PTR_BASE if k % 2 else 0, owners="long" if layout == "long_only" else "all",
                                          order=_every_other_wave_shuffled(n, rng) if layout == "shuffled" else None, vpos=VPOS[k % 4]))
    return cols


def list_seams(rng):
    """Lists of 0..5 entries at every row count and validity form, int32 and int64 offsets."""
    return [list_column(rng.integers(0, 6, n), validity_form(form, n, rng), rng, "list/%s/n%d/%d" % (form, n, 64 if large else 32), large=large,
                        vpos=VPOS[(i + j + large) % 4])
            for i, n in enumerate(ROWS) for j, form in enumerate(FORMS) for large in (False, True)]


def _both_widths(make):
    """one family with int32 and with int64 offsets; ptr_base is non-zero in one of the two"""
    def build(rng):
        cols = []
        for large in (False, True):
            made = make(rng, dict(large=large, ptr_base=0 if large else PTR_BASE, vpos=VPOS[1 + large]))
            cols += made if isinstance(made, list) else [made]
        for c in cols:
            c["name"] += "/%d" % (64 if c["large"] else 32)
        return cols
    build.__doc__ = make.__doc__
    return build


def _tiny(rng, kw):
    """All strings 0..4 bytes (the tile's payload comes from the length pass's registers); a tiny tile between two that are
    not; tiles that are tiny but for one row of 5 bytes in one wave of one sub-block, and one where that row is NULL."""
    ok = rng.random(6145) < 0.8
    cols = [string_column(rng.integers(0, 5, 6145), ok, rng, "tiny/all", **kw)]
    lens = rng.integers(0, 5, 3 * TILE + 100)
    lens[:TILE] = _mixed(TILE, rng)
    lens[2 * TILE:] = _mixed(TILE + 100, rng)
    cols.append(string_column(lens, None, rng, "tiny/between", owners="all", **kw))
    lens = rng.integers(0, 5, 5 * TILE)
    ok = np.ones(5 * TILE, bool)
    for j in range(5):                   # tile j: sub-block j + 1, wave j % 4, lane 17
        lens[j * TILE + SUB * (j + 1) + 64 * (j % 4) + 17] = 5
    ok[4 * TILE + SUB * 5 + 17] = False   # the fifth tile's long row is NULL: the tile stays tiny
    cols.append(string_column(lens, ok, rng, "tiny/one_row_of_5", **kw))
    return cols


def _inline(rng, kw):
    """Lengths 0..12: no heap at all."""
    return string_column(rng.integers(0, 13, 6145), rng.random(6145) < 0.8, rng, "inline", **kw)


def _mixed_row_order(rng, kw):
    """0..40 bytes, the heap holds every row's bytes in row order: the wave-wide coalesced copy."""
    return string_column(_mixed(6145, rng), rng.random(6145) < 0.9, rng, "mixed/row_order", owners="all", **kw)


def _mixed_shuffled(rng, kw):
    """0..40 bytes, the pointers of every other wave shuffled: contiguous waves next to per-row waves."""
    return string_column(_mixed(6145, rng), rng.random(6145) < 0.9, rng, "mixed/shuffled", owners="all", order=_every_other_wave_shuffled(6145, rng), **kw)


def _mixed_long_only(rng, kw):
    """0..40 bytes, a heap of the long strings alone (DuckDB's own), with runs of long strings back to back."""
    lens = _mixed(6145, rng)
    lens[rng.random(6145) < 0.4] = 20
    lens[TILE: TILE + 640] = 33
    return string_column(lens, rng.random(6145) < 0.9, rng, "mixed/long_only", **kw)


def _no_payload(rng, kw):
    """tile_total == 0: all NULL, all empty, and an empty tile (half NULL, half empty) between two full ones."""
    n = 6145
    between = _mixed(n, rng)
    between[TILE: 2 * TILE] = 0
    ok = np.ones(n, bool)
    ok[TILE: 2 * TILE: 2] = False
    return [string_column(_mixed(n, rng), np.zeros(n, bool), rng, "all_null", **kw),
            string_column(np.zeros(n, np.int64), np.ones(n, bool), rng, "all_empty", **kw),
            string_column(between, ok, rng, "empty_tile_between", **kw)]


def _spanning_lens(rng):
    n = 700
    lens = _mixed(n, rng)
    at = rng.permutation(n)[:25]
    lens[at[:24]] = rng.choice(np.concatenate([np.arange(WINDOW - 40, WINDOW + 41), [16384] * 20, [70000] * 20]), 24)
    lens[at[:3]] = [WINDOW - 40, WINDOW + 40, 70000]
    lens[at[24]] = 1 << 20
    ok = rng.random(n) < 0.9
    ok[at] = True
    return lens, ok


def _spanning_contiguous(rng, kw):
    """Strings of 8 KiB +- 40, 16384 and 70 000 bytes and one of 1 MiB among short rows, heap in row order: one string spans
    up to 129 LDS windows of the coalesced copy."""
    return string_column(*_spanning_lens(rng), rng, "spanning/contiguous", owners="all", **kw)


def _spanning_shuffled(rng, kw):
    """The same lengths with shuffled pointers: every long row brings its own bytes, window by window."""
    return string_column(*_spanning_lens(rng), rng, "spanning/shuffled", owners="all", order=rng.permutation(700), **kw)


VICTIMS = [12, 13, 16, 17, 33, 49, 65, 100]


def _window_edges(far):
    def make(rng, kw):
        """Every 256-row sub-block = a heap filler of F bytes, a victim, zero-length rows (some of them NULL).  A sub-block
        that starts at output position p has its first window end 8192 - (p & 15) bytes in; F is chosen so that this end
        falls c bytes into the victim for every c from -1 (the filler's last byte is cut off) to len + 1 (one spare byte: a
        single window).  Adjacent: victim behind the filler in the heap (one contiguous copy; an inline victim places
        itself).  Far: shuffled heap (per-row pieces); the inline victim's filler is two rows (13 + F - 13 bytes) there, since
        one long row alone in a wave is always contiguous."""
        lens, produced, phases, base = [], set(), set(), 0
        for v in VICTIMS:
            for c in range(-1, v + 2):
                room = WINDOW - (base & 15)
                fill = room - c
                rows = [13, fill - 13, v] if (far and v <= 12) else [fill, v]
                lens += rows + [0] * (SUB - len(rows))
                produced.add((v, c))
                phases.add(base & 15)
                base += fill + v
        assert produced == {(v, c) for v in VICTIMS for c in range(-1, v + 2)} and phases == set(range(16))
        n = len(lens)
        assert n == SUB * sum(v + 3 for v in VICTIMS)
        lens = np.array(lens)
        ok = (lens > 0) | (rng.random(n) < 0.7)
        col = string_column(lens, ok, rng, "window_edges/%s" % ("far" if far else "adjacent"), order=rng.permutation(n) if far else None, **kw)
        first = np.arange(0, n, SUB)
        touching = col["hstart"][first + 1] == col["hstart"][first] + lens[first]
        assert not touching[lens[first + 1] > 12].any() if far else touching[lens[first + 1] > 12].all()
        return col
    return make


def eight_mib_boundary(rng):
    """A string of 2**23 - 1 bytes (the fast kernel's largest; alone among inline rows in its wave, so it travels as the
    coalesced copy) and one of 2**23 (its tile goes to encode_string_slow), each among short rows, in a plan with a list
    task: encode_string_slow runs one workgroup per tile."""
    n = 3000
    a = _mixed(n, rng)
    a[2432: 2496] = rng.integers(0, 13, 64)
    a[2450] = 2**23 - 1
    b = _mixed(n, rng)
    b[700] = 2**23
    ok_a, ok_b = rng.random(n) < 0.9, rng.random(n) < 0.9
    ok_a[2450] = ok_b[700] = True
    return [string_column(a, ok_a, rng, "8mib/minus_1/32", ptr_base=PTR_BASE, vpos=1),
            list_column(rng.integers(0, 6, 5000), rng.random(5000) < 0.8, rng, "8mib/list/32"),
            string_column(b, ok_b, rng, "8mib/exact/64", large=True, vpos=3)]


def lookback_long_column(rng):
    """150 000 rows of 0..6 bytes = 74 tiles: more predecessors than a wave has lanes, many look-back steps of 4; tiles 20..29
    are all NULL (ten sums of zero in a row)."""
    cols = []
    for large in (False, True):
        n = 150000
        ok = rng.random(n) < 0.9
        ok[20 * TILE: 30 * TILE] = False
        cols.append(string_column(rng.integers(0, 7, n), ok, rng, "lookback/long/%d" % (64 if large else 32), large=large, ptr_base=PTR_BASE if large else 0))
    return cols


def lookback_many_columns(rng):
    """18 string columns at every row count in mixed order, a list column behind every third, and 0-row tasks first, in the
    middle and last: columns start at tiles other than 0 and tile_begin holds equal neighbours."""
    cols = [string_column([], None, rng, "lookback/empty_first")]
    for i, n in enumerate(rng.permutation(ROWS).tolist()):
        large = i % 2 == 1
        cols.append(string_column(_mixed(n, rng), validity_form(FORMS[i % 6], n, rng), rng, "lookback/str%d/n%d" % (i, n), large=large,
                                  ptr_base=PTR_BASE if i % 4 < 2 else 0, owners=("all", "long")[i % 2], vpos=VPOS[i % 4]))
        if i % 3 == 2:
            m = ROWS[(5 * i) % len(ROWS)]
            cols.append(list_column(rng.integers(0, 6, m), validity_form(FORMS[(i + 2) % 6], m, rng), rng, "lookback/list%d/n%d" % (i, m), large=not large))
        if i == 8:
            cols.append(string_column([], None, rng, "lookback/empty_middle", large=True))
            cols.append(list_column([], None, rng, "lookback/empty_list"))
    cols.append(string_column([], None, rng, "lookback/empty_last"))
    assert sum(c["kind"] == K_ENC_STR32 and c["n"] > 0 for c in cols) >= 12 and sum(c["n"] == 0 for c in cols) >= 3
    return cols


# Three long lists pass 2**31 with no payload at all; without the last one the offsets still fit.  (Two lists of exactly
# 2**30 entries already end at 2**31 = INT32_MAX + 1, hence the middle one: the short rows add up to less than 2**16.)
LONG_LISTS = [2**30, 2**30 - 2**16, 2**30]


def _long_lists(large, last_null, shapes=("one_tile", "three_tiles")):
    def build(rng):
        cols = []
        for shape in shapes:
            n = 100 if shape == "one_tile" else 2 * TILE + 10
            at = [10, 20, 30] if shape == "one_tile" else [5, TILE + 5, 2 * TILE + 5]
            lens = [int(x) for x in rng.integers(0, 6, n)]
            ok = rng.random(n) < 0.8
            for r, long_ in zip(at, LONG_LISTS):
                lens[r], ok[r] = long_, True
            ok[at[2]] = not last_null
            cols.append(list_column(lens, ok, rng, "list/2p30/%s/%d%s" % (shape, 64 if large else 32, "/last_null" if last_null else ""), large=large))
        return cols
    build.__doc__ = """Lists of 0..5 entries and three long ones (LONG_LISTS) in one tile / one in each of three tiles: the running offset
    passes 2**31 with no payload.  int64 offsets are exact; int32 offsets raise the overflow bit (the look-back's last
    tile decides) unless the last long list is NULL."""
    return build


def _lists_ending_at(end, large=False):
    def build(rng):
        n = TILE + 9
        lens = [0] * n
        lens[7], lens[TILE + 3] = 2**30, end - 2**30
        ok = rng.random(n) < 0.8
        ok[[7, TILE + 3]] = True
        return [list_column(lens, ok, rng, "list/ends_at_%d/%d" % (end, 64 if large else 32), large=large)]
    build.__doc__ = "Two lists in two tiles whose last offset is exactly %d: INT32_MAX fits, INT32_MAX + 1 does not." % end
    return build


def _one_huge_list(large):
    def build(rng):
        lens = [int(x) for x in rng.integers(0, 6, 10)]
        lens[3] = 2**32 + 5
        return [list_column(lens, None, rng, "list/2p32_plus_5/%d" % (64 if large else 32), large=large)]
    build.__doc__ = """One list of 2**32 + 5 entries among short ones: the length is 64 bits wide (summing low dwords would give 5, and no
    overflow with int32 offsets)."""
    return build


CASES = {
    "fixed_kinds": fixed_kinds,
    "string_seams": string_seams,
    "list_seams": list_seams,
    "tiny": _both_widths(_tiny),
    "inline_only": _both_widths(_inline),
    "mixed_row_order": _both_widths(_mixed_row_order),
    "mixed_every_other_wave_shuffled": _both_widths(_mixed_shuffled),
    "mixed_long_strings_only": _both_widths(_mixed_long_only),
    "no_payload": _both_widths(_no_payload),
    "spanning_windows_contiguous": _both_widths(_spanning_contiguous),
    "spanning_windows_shuffled": _both_widths(_spanning_shuffled),
    "window_edges_adjacent": _both_widths(_window_edges(False)),
    "window_edges_far": _both_widths(_window_edges(True)),
    "eight_mib_boundary": eight_mib_boundary,
    "lookback_long_column": lookback_long_column,
    "lookback_many_columns": lookback_many_columns,
    "lists_of_2p30_int64": _long_lists(True, False),
    "lists_of_2p30_int32_one_tile": _long_lists(False, False, ("one_tile",)),
    "lists_of_2p30_int32_three_tiles": _long_lists(False, False, ("three_tiles",)),
    "lists_of_2p30_int32_last_null": _long_lists(False, True),
    "lists_ending_at_int32_max": _lists_ending_at(INT32_MAX),
    "lists_ending_at_int32_max_plus_1": _lists_ending_at(INT32_MAX + 1),
    "list_of_2p32_plus_5_int64": _one_huge_list(True),
    "list_of_2p32_plus_5_int32": _one_huge_list(False),
}
GPU_ONLY = ["eight_mib_boundary"]
# the status of the plans above; every other plan ends with 0
EXPECTED_STATUS = {"lists_of_2p30_int32_one_tile": ST_OFFSET_OVERFLOW, "lists_of_2p30_int32_three_tiles": ST_OFFSET_OVERFLOW,
                   "lists_ending_at_int32_max_plus_1": ST_OFFSET_OVERFLOW, "list_of_2p32_plus_5_int32": ST_OFFSET_OVERFLOW}

_built = {}


def case_columns(name):
    """the columns of a case and their references, built once and shared (nobody writes to them)"""
    if name not in _built:
        cols = CASES[name](np.random.default_rng(zlib.crc32(name.encode())))
        _built[name] = (cols, [encode_reference(c) for c in cols])
    return _built[name]


# ------------------------------------------------------------------------------------------------ running a plan
class _Arena:
    """buffers laid out in one allocation, each at a multiple of 256 bytes plus its phase, GUARD bytes apart at least"""

    def __init__(self):
        self.size, self.parts = 256, []

    def add(self, nbytes, phase=0, content=None):
        at = self.size + phase
        self.size = (at + nbytes + GUARD + 255) // 256 * 256 + 256
        if content is not None:
            self.parts.append((at, content))
        return at


def run_plan(ctx, torch, cols, refs, launches=1):
    """One Plan of all the columns, launched `launches` times.  Every output buffer lies in one arena filled with SENTINEL,
    out_data and out_aux at multiples of 256 bytes, out_validity col["vpos"] bytes behind one.
    -> (the arena's bytes after the last launch, [dict(bitmap=, data=, aux=) of (position, length, loose bytes) per task],
        [(status, NULL counts) per launch])"""
    import duckdb_arrow_amd as da
    src, dst, where, tasks = _Arena(), _Arena(), [], []
    for col, ref in zip(cols, refs):
        at = {}
        for key, phase in (("bitmap", col["vpos"]), ("data", 0), ("aux", 0)):
            if ref[key] is not None:
                loose = ref["loose"] if key == "data" else 0
                at[key] = (dst.add(len(ref[key]) + loose, phase), len(ref[key]), loose)
        where.append(at)
        tasks.append(dict(src=src.add(len(col["src"]), content=col["src"]),
                          words=src.add(8 * len(col["words"]), content=col["words"].view(np.uint8)) if col["words"] is not None else None,
                          heap=src.add(len(col["heap"]), HEAP_PHASE, col["heap"]) if col["heap"] is not None else None))
    host = np.zeros(src.size, np.uint8)
    for at, content in src.parts:
        host[at: at + len(content)] = content
    d_src = torch.from_numpy(host).cuda()
    # behind the arena, as many spare bytes as all the string data together: a string tile that took another column's prefix for
    # its own would still write inside the allocation, and show up as wrong bytes
    spare = sum(len(ref["aux"]) for ref in refs if ref["aux"] is not None) + 4096
    d_dst = torch.full((dst.size + spare,), SENTINEL, dtype=torch.uint8, device="cuda")
    s0, d0 = d_src.data_ptr(), d_dst.data_ptr()
    assert s0 % 256 == 0 and d0 % 256 == 0
    made = []
    for col, at, t in zip(cols, where, tasks):
        made.append(da.make_task(col["kind"], col["n"], s0 + t["src"], d0 + at["data"][0] if "data" in at else 0,
                                 validity=s0 + t["words"] if t["words"] is not None else 0,
                                 out_validity=d0 + at["bitmap"][0] if "bitmap" in at else 0, out_aux=d0 + at["aux"][0] if "aux" in at else 0,
                                 buf2=s0 + t["heap"] if t["heap"] is not None else 0, ptr_base=col["ptr_base"],
                                 buf2_len=len(col["heap"]) if col["heap"] is not None else 0, param=col["width"], parent_div=int(col["large"])))
    plan = da.Plan(ctx, made)
    runs = []
    for _ in range(launches):
        plan.launch(torch.cuda.current_stream().cuda_stream)
        runs.append((plan.status(), plan.null_counts()))
    got = d_dst.cpu().numpy()
    assert (got[dst.size:] == SENTINEL).all(), "bytes behind the last buffer were written"
    plan.close()
    return got, where, runs


def check_task(col, ref, got, at):
    """Every buffer equals the reference byte for byte; every other byte of the arena between this task's buffers and their
    neighbours is still the sentinel (a task of 0 rows has written nothing at all)."""
    seen = np.zeros(0, np.uint8)
    for key in ("bitmap", "data", "aux"):
        if ref[key] is None:
            continue
        pos, size, loose = at[key]
        if not np.array_equal(got[pos: pos + size], ref[key]):
            bad = np.nonzero(got[pos: pos + size] != ref[key])[0]
            raise AssertionError("%s: %d of %d %s bytes differ, first at %d: got %s want %s" % (
                col["name"], len(bad), size, key, bad[0], got[pos + bad[0]: pos + bad[0] + 8].tolist(), ref[key][bad[0]: bad[0] + 8].tolist()))
        lo, hi = pos - pos % 256 - 256, (pos + size + loose + GUARD + 255) // 256 * 256 + 256
        seen = np.concatenate([seen, got[lo: pos], got[pos + size + loose: hi]])
    assert (seen == SENTINEL).all(), (col["name"], "bytes outside the buffers were written")


def check_plan(cols, refs, got, where, runs):
    """check_task for every task; per launch, the status is the OR of the tasks' and the NULL counts are theirs, in the
    caller's order"""
    for col, ref, at in zip(cols, refs, where):
        check_task(col, ref, got, at)
    want_status = 0
    for ref in refs:
        want_status |= ref["status"]
    for status, nulls in runs:
        assert status == want_status, (status, want_status)
        assert nulls == [ref["nulls"] for ref in refs]
    return want_status

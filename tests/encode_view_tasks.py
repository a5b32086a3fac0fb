"""Kernel-level string-view encode tasks (MI_K_ENC_STRVIEW, kernels_encode_view.hip) for test_encode_view_reference_host.py
and test_gpu_encode_view_tasks.py: the columns come from encode_tasks' builders (string_column, validity_form, the arena
and run_plan / check_plan), the reference is view_reference below -- a numpy restatement of the four rules of DuckDB's
ArrowVarcharToStringViewData that calls neither the package nor the oracle:

  1. three buffers: the bitmap (always there, pad bits 1), 16 bytes of view per row, ONE data buffer;
  2. a valid row of <= 12 bytes is {int32 length, its bytes, zeros up to 16} whatever the source slot holds behind them;
  3. a longer valid row is {length, the string_t's 4 prefix bytes, buffer index 0, int32 offset}, and the data buffer is
     those rows' bytes back to back in row order (two rows that share heap bytes each get a copy);
  4. a NULL row is 16 zero bytes and adds nothing; the offsets are int32 and there is no large variant (MI_ST_OFFSET_OVERFLOW).

The shapes follow the kernel: 64 rows per wave and bitmap lane, 8 rows per thread, 2048 per tile, 4 look-back predecessors
per step, long rows of >= WAVE_COPY bytes copied by their wave in rounds of WAVE_ROUND bytes, a tile whose long strings lie
back to back in the heap copied by the workgroup in rounds of BLOCK_ROUND bytes that start at the first 16-byte boundary of
the data buffer at or behind the tile's first byte.  The kernel stages nothing in LDS, so these rounds are its windows."""
import os
import re
import zlib

import numpy as np

import encode_tasks as et
from encode_tasks import FORMS, PTR_BASE, TILE, VPOS, string_column, list_column, validity_form

K_ENC_STRVIEW = 38
INLINE = 12


def _kernel_constant(file, name):
    """`constexpr <type> <name> = <integer>;` as the kernel source has it: the seams below move with the kernel"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "duckdb-arrow_amd", "csrc", file)).read()
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


WAVE_COPY = _kernel_constant("kernels_encode_view.hip", "kViewWaveCopy")
WAVE_ROUND, BLOCK_ROUND = 16 * 64, 16 * _kernel_constant("kernels.hpp", "kBlockThreads")   # 16 bytes per lane of a wave / of the workgroup
assert _kernel_constant("kernels.hpp", "kTileRows") == TILE
ROWS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6145]
LENGTHS = [0, 1, 4, 5, 11, 12, 13, 16, 17, 100]


# ------------------------------------------------------------------------------------------------ the reference
def view_reference(col):
    """-> dict(bitmap, data = the views, aux = the data buffer, loose, nulls, status), the keys of encode_tasks.encode_reference"""
    n = col["n"]
    out = et.encode_reference(dict(col, kind=et.K_ENC_VALIDITY))        # rule 1's bitmap and the NULL count: K7a as for every kind
    out.update(data=np.zeros(0, np.uint8), aux=np.zeros(0, np.uint8))
    if n == 0:
        return out
    ok = et._row_bits(col)
    s = col["src"].reshape(n, 16)
    ln = s.view("<u4")[:, 0].astype(np.int64)
    views = np.zeros((n, 16), np.uint8)
    short = np.nonzero(ok & (ln <= INLINE))[0]
    views.view("<u4")[short, 0] = ln[short]
    flat = views.reshape(-1)
    et.ragged_copy(flat, 16 * short + 4, col["src"], 16 * short + 4, ln[short])               # rule 2: the bytes and nothing behind them
    long_ = np.nonzero(ok & (ln > INLINE))[0]
    off = np.cumsum(ln[long_]) - ln[long_]
    total = int(ln[long_].sum())
    if total > et.INT32_MAX:
        out["status"] = et.ST_OFFSET_OVERFLOW
        return out
    views.view("<u4")[long_, 0] = ln[long_]
    views[long_, 4:8] = s[long_, 4:8]                                                          # rule 3: the string_t's own prefix
    views.view("<i4")[long_, 3] = off
    data = np.zeros(total, np.uint8)
    et.ragged_copy(data, off, col["heap"], (s.view("<u8")[long_, 1] - np.uint64(col["ptr_base"])).astype(np.int64), ln[long_])
    out.update(data=flat, aux=data)
    return out


def reference(col):
    return view_reference(col) if col["kind"] == K_ENC_STRVIEW else et.encode_reference(col)


# ------------------------------------------------------------------------------------------------ columns
def view_column(lens, ok, rng, name, **kw):
    """encode_tasks.string_column as a view task: its text made 7-bit (Utf8View must validate; the noise in inline padding,
    under NULL rows and in unowned heap bytes stays as it is) and the prefix of every long row set to its first four bytes,
    DuckDB's invariant."""
    col = string_column(lens, ok, rng, name, **kw)
    n = col["n"]
    col["text"] &= 0x7F
    col["heap"] &= 0x7F
    s = col["src"].reshape(n, 16)
    valid = np.ones(n, bool) if col["ok"] is None else col["ok"]
    ln = np.where(valid, s.view("<u4")[:, 0].astype(np.int64), 0)
    short = np.nonzero(valid & (ln <= INLINE))[0]
    if len(short):
        k = np.arange(int(ln[short].sum())) - np.repeat(np.cumsum(ln[short]) - ln[short], ln[short])
        col["src"][np.repeat(16 * short + 4, ln[short]) + k] &= 0x7F
    long_ = np.nonzero(valid & (ln > INLINE))[0]
    start = (s.view("<u8")[long_, 1] - np.uint64(col["ptr_base"])).astype(np.int64)
    for j in range(4):
        s[long_, 4 + j] = col["heap"][start + j]
    col.update(kind=K_ENC_STRVIEW, long_rows=long_, long_bytes=int(ln[long_].sum()))
    return col


def _mixed(n, rng):
    return rng.integers(0, 41, n)


def _every_other_wave_shuffled(n, rng):
    return et._every_other_wave_shuffled(n, rng)


LAYOUTS = ("long_only", "row_order", "shuffled")


def _layout_kw(layout, n, rng):
    return dict(owners="long" if layout == "long_only" else "all", order=_every_other_wave_shuffled(n, rng) if layout == "shuffled" else None)


def row_seams(rng):
    """Strings of 0..40 bytes at the row counts around a wave, a sub-block and a tile, in every validity form, the three heap
    layouts in turn; the bitmap at byte positions 0, 1, 3, 5."""
    cols = []
    for i, n in enumerate(ROWS):
        for j, form in enumerate(FORMS):
            layout = LAYOUTS[(i + j) % 3]
            cols.append(view_column(_mixed(n, rng), validity_form(form, n, rng), rng, "view/%s/%s/n%d" % (layout, form, n),
                                    ptr_base=PTR_BASE if (i + j) % 2 else 0, vpos=VPOS[(i + j) % 4], **_layout_kw(layout, n, rng)))
    for n in ROWS:
        assert {c["vpos"] for c in cols if c["n"] == n} == set(VPOS)
    return cols


def length_seams(rng):
    """Every length of LENGTHS in every lane position (a permutation per wave), once with random and once with 0xFF padding
    behind the inline bytes; NULL rows hold a length of 0xFFFFFFFF or of 13..40 and a pointer outside the heap."""
    cols = []
    for pad in ("noise", "ff"):
        n = 6145
        lens = rng.choice(np.array(LENGTHS), n)
        ok = rng.random(n) < 0.8
        col = view_column(lens, ok, rng, "view/lengths/%s" % pad, ptr_base=PTR_BASE, vpos=3)
        s = col["src"].reshape(n, 16)
        if pad == "ff":
            for r in np.nonzero(ok & (lens <= INLINE))[0]:
                s[r, 4 + lens[r]:] = 0xFF
            assert (s[ok & (lens == 0), 4:] == 0xFF).all()
        assert set(lens[ok].tolist()) == set(LENGTHS)
        gone = s.view("<u4")[~ok, 0]
        assert (gone == 0xFFFFFFFF).any() and ((gone >= 13) & (gone <= 40)).any()
        assert (s.view("<u8")[~ok, 1] >= et.FAR_POINTER).all()
        cols.append(col)
    return cols


def heap_layouts(rng):
    """0..40 bytes with runs of long rows: a heap of the long strings alone, back to back (the workgroup's one copy); every
    string in the heap, inline ones between the long ones; every other wave shuffled; ptr_base zero and not; the heap
    starts at an odd address (encode_tasks.HEAP_PHASE) and its first string at an odd position inside it."""
    cols = []
    for i, layout in enumerate(LAYOUTS):
        for ptr_base in (0, PTR_BASE):
            n = 6145
            lens = _mixed(n, rng)
            lens[rng.random(n) < 0.3] = 20
            lens[TILE: TILE + 640] = 33
            col = view_column(lens, rng.random(n) < 0.9, rng, "view/heap/%s/%x" % (layout, ptr_base), ptr_base=ptr_base, vpos=VPOS[i], **_layout_kw(layout, n, rng))
            h = col["hstart"][col["long_rows"]]
            ln = lens[col["long_rows"]]
            touching = h[1:] == h[:-1] + ln[:-1]
            assert touching.all() if layout == "long_only" else not touching.all()
            cols.append(col)
    assert et.HEAP_PHASE % 2 == 1 and et.HEAP_FIRST % 2 == 1
    return cols


def shared_strings(rng):
    """Pairs of rows whose string_t are the same 16 bytes (one heap string, two views): next to each other, a wave apart and
    a tile apart.  Each gets its own copy in the data buffer."""
    n = 2 * TILE + 300
    lens = _mixed(n, rng)
    pairs = [(10, 11), (100, 164), (500, TILE + 500), (TILE + 7, 2 * TILE + 7), (2 * TILE + 100, 2 * TILE + 299)]
    for a, b in pairs:
        lens[a] = lens[b] = 13 + (a % 50)
    ok = rng.random(n) < 0.9
    ok[[r for p in pairs for r in p]] = True
    col = view_column(lens, ok, rng, "view/shared", ptr_base=PTR_BASE)
    s = col["src"].reshape(n, 16)
    values = col["values"]()
    for a, b in pairs:
        s[b] = s[a]
        values[b] = values[a]
    assert all((s[a] == s[b]).all() and s.view("<u4")[a, 0] > INLINE for a, b in pairs)
    col["values"] = lambda: values
    col["text"] = None       # the data buffer is no longer the builder's text: the host test compares with the values
    return [col]


def _long_string(length):
    def build(rng):
        n = 3000
        lens = _mixed(n, rng)
        lens[700], lens[701] = length, 13
        ok = rng.random(n) < 0.9
        ok[700:702] = True
        cols = [view_column(lens, ok, rng, "view/long%d/contiguous" % length, ptr_base=PTR_BASE, vpos=1),
                view_column(lens, ok, rng, "view/long%d/shuffled" % length, owners="all", order=rng.permutation(n), vpos=5)]
        for c in cols:
            s = c["src"].reshape(n, 16).view("<u4")
            assert s[700, 0] == length and s[701, 0] == 13
        return cols
    build.__doc__ = """One string of %d bytes with a 13-byte neighbour behind it, among rows of 0..40 bytes: once in a heap of the long strings
    alone (the workgroup's copy), once with shuffled pointers (the string's own wave copies it).  Positions are 64 bits wide and
    no other kernel takes over.""" % length
    return build


def piece_seams(rng):
    """Lengths around the 16-byte piece, kViewWaveCopy and the rounds of the wave's and the workgroup's copies, back to back in the
    heap and shuffled."""
    edge = [13, 14, 15, 16, 17, 31, 32, 33, 47, 48, 49]
    for m in (WAVE_COPY, WAVE_ROUND, WAVE_ROUND + 16, BLOCK_ROUND, BLOCK_ROUND + 16):
        edge += [m - 1, m, m + 1]
    lens = np.array(edge * 3)
    rng.shuffle(lens)
    n = len(lens)
    assert n <= TILE and {WAVE_COPY - 1, WAVE_COPY, WAVE_COPY + 1} <= set(lens.tolist())
    return [view_column(lens, None, rng, "view/pieces/contiguous"),
            view_column(lens, None, rng, "view/pieces/shuffled", owners="all", order=rng.permutation(n), ptr_base=PTR_BASE)]


def wave_rounds(rng):
    """Rows a wave copies on its own (>= kViewWaveCopy bytes, shuffled pointers) whose lengths lie 17 bytes to either side of one,
    two and three rounds of the wave's stream (WAVE_ROUND bytes from the row's first 16-byte boundary in the data buffer), each
    behind a row of 13..28 bytes, so that the boundary takes every phase: the round's last piece, the clamped piece that ends
    where the string ends, and the first piece of the next round, on every byte."""
    lens, at = [], 0
    for m in (1, 2, 3):
        for d in range(-17, 18):
            short = 13 + (len(lens) // 2 - at - 13) % 16          # the long row behind it starts at phase (its index) % 16
            lens += [short, m * WAVE_ROUND + d]
            at += short + m * WAVE_ROUND + d
    n = len(lens)
    assert n <= TILE and min(lens[1::2]) >= WAVE_COPY
    col = view_column(np.array(lens), None, rng, "view/wave_rounds", owners="all", order=rng.permutation(n), ptr_base=PTR_BASE)
    starts = np.cumsum(lens) - np.array(lens)
    assert len({int(x) % 16 for x in starts[1::2]}) == 16          # the long rows start at every phase of the data buffer
    return [col]


VICTIMS = [13, 16, 17, 33, 49, 65, 100]


def _round_edges(first_tile_bytes, far):
    def build(rng):
        lens, produced = [], set()
        if first_tile_bytes:      # a tile in front: the victims' tile starts at that byte of the data buffer
            lens = [first_tile_bytes] + [0] * (TILE - 1)
        origin = -first_tile_bytes % 16       # where the first round of the victims' tile starts, counted from the tile's first byte
        p = 0
        for v in VICTIMS:
            for c in range(-1, v + 2):
                fill = (origin - p - c) % BLOCK_ROUND
                fill += BLOCK_ROUND if fill < 13 else 0
                lens += [fill, v]
                p += fill
                assert (p + c - origin) % BLOCK_ROUND == 0     # a round ends c bytes into the victim
                produced.add((v, c))
                p += v
        assert produced == {(v, c) for v in VICTIMS for c in range(-1, v + 2)} and len(lens) - (TILE if first_tile_bytes else 0) <= TILE
        n = len(lens)
        col = view_column(np.array(lens), None, rng, "view/round_edges/%d/%s" % (first_tile_bytes, "far" if far else "adjacent"),
                          order=rng.permutation(n) if far else None, ptr_base=PTR_BASE if far else 0)
        h, ln = col["hstart"][col["long_rows"]], np.array(lens)[col["long_rows"]]
        assert (h[1:] == h[:-1] + ln[:-1]).all() != far
        return [col]
    build.__doc__ = """One tile of (filler, victim) pairs of long rows, the filler chosen so that a round of the workgroup's copy (BLOCK_ROUND
    bytes from the first 16-byte boundary of the data buffer inside the tile) ends c bytes into the victim, for every victim
    of 13..100 bytes and every c from -1 to len + 1.  %s%s""" % (
        "A tile of %d long bytes lies in front, so the rounds start %d bytes into the tile.  " % (first_tile_bytes, -first_tile_bytes % 16) if first_tile_bytes else "",
        "Shuffled pointers: every row by its own lane or wave." if far else "Heap in row order: the one copy.")
    return build


def lookback_one_column(rng):
    """74 tiles.  First column: only tile 0 and tile 73 hold long strings -- tile 73 walks through 72 published zeros, which never
    wait for anybody.  Second column: long strings in every tile."""
    n = 73 * TILE + 900
    lens = rng.integers(0, 13, n)
    lens[[5, 70, 1999]] = [13, 40, 300]
    lens[[73 * TILE + 1, 73 * TILE + 64, n - 1]] = [17, 100, 13]
    ok = rng.random(n) < 0.95
    ok[[5, 73 * TILE + 1]] = True
    sparse = view_column(lens, ok, rng, "view/lookback/sparse", ptr_base=PTR_BASE)
    tiles = np.unique(sparse["long_rows"] // TILE)
    assert set(tiles.tolist()) <= {0, 73} and (n + TILE - 1) // TILE == 74
    dense = view_column(rng.integers(0, 20, n), rng.random(n) < 0.9, rng, "view/lookback/dense", vpos=1)
    assert len(np.unique(dense["long_rows"] // TILE)) == 74
    return [sparse, dense]


def lookback_many_columns(rng):
    """18 view columns at every row count of encode_tasks.ROWS in mixed order, a STR32 column behind every second, a list
    column behind every third, and 0-row tasks first, in the middle and last: view columns start at tiles other than 0,
    tile_begin holds equal neighbours, and encode_string_1p, encode_string_slow and encode_string_view run in one plan."""
    cols = [view_column([], None, rng, "view/many/empty_first")]
    for i, n in enumerate(rng.permutation(et.ROWS).tolist()):
        layout = LAYOUTS[i % 3]
        cols.append(view_column(_mixed(n, rng), validity_form(FORMS[i % 6], n, rng), rng, "view/many/view%d/n%d" % (i, n),
                                ptr_base=PTR_BASE if i % 4 < 2 else 0, vpos=VPOS[i % 4], **_layout_kw(layout, n, rng)))
        if i % 2 == 1:
            m = et.ROWS[(7 * i) % len(et.ROWS)]
            cols.append(string_column(_mixed(m, rng), validity_form(FORMS[(i + 1) % 6], m, rng), rng, "view/many/str%d/n%d" % (i, m), large=i % 4 == 1, owners="all"))
        if i % 3 == 2:
            m = et.ROWS[(5 * i) % len(et.ROWS)]
            cols.append(list_column(rng.integers(0, 6, m), validity_form(FORMS[(i + 2) % 6], m, rng), rng, "view/many/list%d/n%d" % (i, m)))
        if i == 8:
            cols.append(view_column([], None, rng, "view/many/empty_middle"))
            cols.append(string_column([], None, rng, "view/many/empty_str"))
    cols.append(view_column([], None, rng, "view/many/empty_last"))
    kinds = [c["kind"] for c in cols if c["n"] > 0]
    assert kinds.count(K_ENC_STRVIEW) == 18 and kinds.count(et.K_ENC_STR32) >= 6 and kinds.count(et.K_ENC_LIST32) >= 4
    assert sum(c["n"] == 0 for c in cols) >= 4
    return cols


CASES = {
    "row_seams": row_seams,
    "length_seams": length_seams,
    "heap_layouts": heap_layouts,
    "shared_strings": shared_strings,
    "long_string_70000": _long_string(70000),
    "long_string_8mib_minus_1": _long_string(2**23 - 1),
    "long_string_8mib": _long_string(2**23),
    "piece_seams": piece_seams,
    "wave_rounds": wave_rounds,
    "round_edges_adjacent": _round_edges(0, False),
    "round_edges_adjacent_behind_29_bytes": _round_edges(29, False),
    "round_edges_far": _round_edges(0, True),
    "lookback_one_column": lookback_one_column,
    "lookback_many_columns": lookback_many_columns,
}

_built = {}


def case_columns(name):
    """the columns of a case and their references, built once and shared (nobody writes to them)"""
    if name not in _built:
        cols = CASES[name](np.random.default_rng(zlib.crc32(("view/" + name).encode())))
        _built[name] = (cols, [reference(c) for c in cols])
    return _built[name]

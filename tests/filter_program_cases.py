"""Hand-built programs for the filter kernel (K6, filter_program<EXT, PAT>) at the program level: resident columns of every
kind a leaf can read, the constant tables in the layouts csrc/kernels.hpp documents, programs in conjunctive normal form that
mi_scan_set_filter's front end never emits, and a numpy evaluator of them.

A leaf here is a dict of *meanings*: {"col", "op", "validity", "negate"} and the constants of its form as Python values --
integers (uint64 columns: 0 .. 2^64 - 1), floats, byte strings.  evaluate() works on those meanings alone: integers exactly,
floats by the total order written out below (NaN greatest, all NaNs equal, -0.0 = +0.0), 128-bit values as Python ints,
strings as bytes in memcmp order, patterns through Python's re.  What the kernel is handed -- keys, biased integers, tables,
flag bits -- is derived from the same leaf by device_fields() and table_image(); no expected row comes from there.
Nothing in this module calls the library."""
import re

import numpy as np

import filter_string_cases as sc

# the kernel's leaf forms and flag bits (csrc/kernels.hpp kLeaf*, include/mi_arrow_ipc.h MI_FL_* / MI_FLF_*)
RANGE, IS_NULL, IS_NOT_NULL, IN, STR_IN, DICT_MAP, STR_RANGE, WIDE_RANGE, WIDE_IN, STR_MATCH = range(1, 11)
F_UNSIGNED, F_NEGATE, F_ENDS_CLAUSE, F_BIAS, F_FLOAT = 1, 2, 4, 8, 16
MAX_LEAVES = 24
WINDOW = 2048
PAD_ROWS = 2048 + 64        # every data buffer is this much longer than nrows: a read past the last row stays inside it
SENTINEL = -1
P63, P64 = 1 << 63, 1 << 64
NAN, INF = float("nan"), float("inf")

SHAPES = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 5 * 2048 + 5)
SMALL_SHAPES = SHAPES[:-3]   # one workgroup (four windows) at the most

# the forms the non-vacuity counts are kept by: the ten ops, RANGE and IN once more on floats
FORMS = ("range", "in", "is_null", "is_not_null", "str_in", "dict_map", "str_range", "wide_range", "wide_in", "str_match",
         "float_range", "float_in")
NEGATABLE = ("range", "in", "str_in", "str_range", "wide_range", "wide_in", "str_match", "float_range", "float_in")

WIDE_POOL = [0, 1, -1, 12345, P63 - 1, P63, P63 + 1, -P63, -P63 - 1, -P63 + 1, P64 - 1, P64, P64 + 1, -P64, -P64 - 1, -P64 + 1,
             (1 << 127) - 1, -(1 << 127)]
DICT_ENTRIES = 40            # the dictionary column's indices: 0 .. 39 entries, 40 the extra NULL entry, 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- columns
class Column:
    """kind "int" (values: numpy of the stored dtype), "float" (float32 / float64), "wide" (object array of Python ints),
    "str" (list of bytes, b"" where the row is NULL; `layout` and `ptr_base` for the packer), "dict" (uint32 indices).
    `values` covers nrows + PAD_ROWS rows in a generated column; evaluate() reads the first nrows."""

    def __init__(self, name, kind, values, layout=None, ptr_base=0):
        self.name, self.kind, self.values, self.layout, self.ptr_base = name, kind, values, layout, ptr_base

    @property
    def width(self):
        return {"wide": 16, "str": 16, "dict": 4}.get(self.kind) or self.values.dtype.itemsize

    def type_flags(self):
        if self.kind == "float":
            return F_FLOAT
        if self.kind == "int" and self.values.dtype.kind == "u":
            return F_UNSIGNED | (F_BIAS if self.values.dtype == np.uint64 else 0)
        return 0


class Columns:
    """columns by name and validity bitmaps by name (bool arrays, True = valid; a column's own bitmap bears its name)"""

    def __init__(self, nrows):
        self.nrows, self.col, self.valid = nrows, {}, {}

    def add(self, column, valid=None):
        self.col[column.name] = column
        if valid is not None:
            self.valid[column.name] = np.asarray(valid, bool)
        return column


def _pad(values, total):
    """the rows past nrows repeat the column's first rows: whatever leaf keeps some row keeps some of these too, were they read"""
    reps = -(-total // len(values))
    return np.concatenate([values] * reps)[:total] if isinstance(values, np.ndarray) else (list(values) * reps)[:total]


def _int_values(rng, dtype, n):
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    if lo == 0:
        pool = [0, 1, 2, hi // 2, hi // 2 + 1, hi - 1, hi]
        near = rng.integers(0, 7, n)
    else:
        pool = [lo, lo + 1, -1, 0, 1, hi - 1, hi]
        near = rng.integers(-3, 4, n)
    pick, from_pool = rng.integers(0, 7, n), rng.random(n) < 0.5
    if dtype == np.uint64:   # the narrow range sits at 0 and at 2^63, the pool around 2^63 and 2^64
        pool = [0, 1, P63 - 1, P63, P63 + 1, P64 - 2, P64 - 1]
        out = [pool[int(p)] if f else (int(v) if v % 2 else P63 + int(v)) for p, v, f in zip(pick, near, from_pool)]
    else:
        out = [pool[int(p)] if f else int(v) for p, v, f in zip(pick, near, from_pool)]
    out[: min(7, n)] = pool[: min(7, n)]
    out[n - 1] = pool[6]     # the maximum closes the last lane
    return np.array(out, dtype)


def _wide_values(rng, n):
    out = []
    for i in range(n):
        if i < len(WIDE_POOL):
            out.append(WIDE_POOL[i])
        elif rng.random() < 0.6:
            out.append(WIDE_POOL[int(rng.integers(0, len(WIDE_POOL)))])
        else:
            v = int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 64)) | int(rng.integers(0, 1 << 20))
            out.append(-v if rng.random() < 0.5 else v)
    return out


def object_array(values):
    out = np.empty(len(values), object)
    out[:] = list(values)
    return out


def float_column(rng, f, n):
    """the specials of test_gpu_filters_float._float_column (NaNs of both signs and three payloads, +-0, subnormals, +-inf,
    the extremes) and quarters, so that 1.5 is present and 1.3 is absent"""
    from test_gpu_filters_float import _float_column
    return _float_column(rng, f, max(n, 16))[:n]


STRING_POOL = None


def string_pool():
    global STRING_POOL
    if STRING_POOL is None:
        STRING_POOL = sc.pool(False)
    return STRING_POOL


def make_columns(nrows, seed=20250915, null_fraction=0.15):
    """every resident column at `nrows` rows (+ PAD_ROWS), each with its own bitmap, and the four shared bitmaps"""
    rng = np.random.default_rng(seed + nrows)
    total = nrows + PAD_ROWS
    cols = Columns(nrows)

    def bitmap(fraction=null_fraction):
        ok = rng.random(nrows) >= fraction
        return np.concatenate([ok, np.ones(total - nrows, bool)])    # the pad bits are ones, as a real vector has them

    for name, dtype in (("i8", np.int8), ("i16", np.int16), ("i32", np.int32), ("i64", np.int64), ("u8", np.uint8), ("u16", np.uint16),
                        ("u32", np.uint32), ("u64", np.uint64)):
        cols.add(Column(name, "int", _pad(_int_values(rng, dtype, nrows), total)), bitmap())
    for name, f in (("f32", np.float32), ("f64", np.float64)):
        cols.add(Column(name, "float", _pad(float_column(rng, f, nrows), total)), bitmap())
    cols.add(Column("hug", "wide", object_array(_pad(_wide_values(rng, nrows), total))), bitmap())
    pool = string_pool()
    for name, layout in (("s_arrow", "arrow"), ("s_shuf", "far_base")):
        ok = bitmap()
        picks = rng.integers(0, len(pool), nrows)
        vals = [pool[int(p)] for p in picks]
        for j in range(min(nrows, len(pool))):       # the whole pool, when there is room for it
            vals[j] = pool[(j * 7) % len(pool)]
        vals = _pad(vals, total)
        vals = [v if o else b"" for v, o in zip(vals, ok)]   # a NULL row is sixteen zero bytes: the empty string
        placement, ptr_base = sc.LAYOUTS[layout]
        cols.add(Column(name, "str", vals, placement, ptr_base), ok)
    idx = rng.integers(0, DICT_ENTRIES, nrows).astype(np.uint32)
    special = rng.random(nrows)
    idx[special < 0.10] = DICT_ENTRIES               # the extra NULL entry: index == n_in
    idx[special < 0.04] = 0xFFFFFFFF
    idx[(special >= 0.10) & (special < 0.16)] = DICT_ENTRIES - 1
    for j, v in enumerate((DICT_ENTRIES - 1, DICT_ENTRIES, 0xFFFFFFFF)[: nrows]):
        idx[nrows - 1 - j] = v
    cols.add(Column("dict", "dict", _pad(idx, total)), bitmap())
    # shared bitmaps: all valid, all NULL (all-zero words, pad bits included), and one with NULLs on the last row and on both
    # sides of every word seam
    cols.valid["all_valid"] = np.ones(total, bool)
    cols.valid["all_null"] = np.zeros(total + (-total) % 64, bool)
    seams = bitmap(0.3)
    seams[nrows - 1] = False
    for r in range(64, nrows, 64):
        seams[r - 1] = seams[r] = False
    cols.valid["seams"] = seams
    last = np.ones(total, bool)                       # the last row alone is valid
    last[: nrows - 1] = False
    cols.valid["last"] = last
    return cols


_columns = {}


def columns(nrows):
    """make_columns(nrows), built once and never changed"""
    if nrows not in _columns:
        _columns[nrows] = make_columns(nrows)
    return _columns[nrows]


def validity_words(ok):
    return sc.validity_words(ok)


# ---------------------------------------------------------------------------------------------------- the float key, restated
def float_key(c, width):
    """the order-preserving key of csrc/filter_key.hpp in numpy: NaN -> MAX, +-0 -> 0, else the bits b >= 0 ? b : b ^ MAX.  Used
    for the constants handed to the kernel only; tests/test_filter_program_reference_host.py holds it to mi_filter_float_key."""
    with np.errstate(over="ignore", invalid="ignore"):
        if width == 4:
            b, mx, exp = int(np.array([c], np.float32).view(np.int32)[0]), 0x7FFFFFFF, 0x7F800000
        else:
            b, mx, exp = int(np.array([c], np.float64).view(np.int64)[0]), 0x7FFFFFFFFFFFFFFF, 0x7FF0000000000000
    mag = b & mx
    if mag > exp:
        return mx
    if mag == 0:
        return 0
    return b if b >= 0 else b ^ mx


# ---------------------------------------------------------------------------------------------------- the evaluator
def _int_ge(v, c):
    info = np.iinfo(v.dtype)
    return np.ones(len(v), bool) if c <= int(info.min) else np.zeros(len(v), bool) if c > int(info.max) else v >= v.dtype.type(c)


def _int_le(v, c):
    info = np.iinfo(v.dtype)
    return np.ones(len(v), bool) if c >= int(info.max) else np.zeros(len(v), bool) if c < int(info.min) else v <= v.dtype.type(c)


def _int_eq(v, c):
    info = np.iinfo(v.dtype)
    return v == v.dtype.type(c) if int(info.min) <= c <= int(info.max) else np.zeros(len(v), bool)


def _float_eq(v, c):
    """the total order: every NaN equals every NaN, -0.0 = +0.0 (IEEE ==)"""
    with np.errstate(invalid="ignore"):
        return (np.isnan(v) & bool(np.isnan(c))) | (v == c)


def _float_lt(a, b):
    """a < b in the total order, a and b arrays or scalars: NaN is the greatest and equals itself"""
    with np.errstate(invalid="ignore"):
        return ~np.isnan(a) & (np.isnan(b) | (a < b))


def like_pattern(segments, head, tail):
    """the LIKE pattern a kLeafStrMatch leaf stands for"""
    assert segments and all(s and b"%" not in s for s in segments)
    return (b"" if head else b"%") + b"%".join(segments) + (b"" if tail else b"%")


def like_regex(pattern):
    """as test_gpu_pattern_filters.like_regex: each % is .* under re.DOTALL, every other byte is itself"""
    return re.compile(b"".join(b".*" if c == 0x25 else re.escape(bytes([c])) for c in pattern), re.DOTALL)


def _by_distinct(values, fn):
    """fn over the distinct byte strings, spread back to the rows"""
    distinct = sorted(set(values))
    where = {v: i for i, v in enumerate(distinct)}
    table = np.array([bool(fn(v)) for v in distinct], bool)
    return table[np.fromiter((where[v] for v in values), np.int64, len(values))]


def compare(leaf, cols, nrows):
    """the comparison of a leaf on every row, validity and negation aside"""
    c, op = cols.col[leaf["col"]], leaf["op"]
    if c.kind == "int":
        v = c.values[:nrows]
        v = v if v.dtype == np.uint64 else v.astype(np.int64)
        if op == RANGE:
            return _int_ge(v, leaf["lo"]) & _int_le(v, leaf["hi"])
        assert op == IN, leaf
        m = np.zeros(nrows, bool)
        for x in leaf["values"]:
            m |= _int_eq(v, x)
        return m
    if c.kind == "float":
        v, f = c.values[:nrows], c.values.dtype.type
        with np.errstate(over="ignore"):
            if op == RANGE:
                lo, hi = f(leaf["lo"]), f(leaf["hi"])     # a constant is cast to the column's type
                return ~_float_lt(v, lo) & ~_float_lt(hi, v)
            assert op == IN, leaf
            m = np.zeros(nrows, bool)
            for x in leaf["values"]:
                m |= _float_eq(v, f(x))
            return m
    if c.kind == "wide":
        v = c.values[:nrows]
        if op == WIDE_RANGE:
            return ((v >= leaf["lo"]) & (v <= leaf["hi"])).astype(bool) if nrows else np.zeros(0, bool)
        assert op == WIDE_IN, leaf
        wanted = set(leaf["values"])
        return np.fromiter((x in wanted for x in v), bool, nrows)
    assert c.kind == "str", leaf
    v = c.values[:nrows]
    if op == STR_IN:
        wanted = set(leaf["values"])
        return _by_distinct(v, lambda x: x in wanted)
    if op == STR_RANGE:
        lower, lo_incl, upper, hi_incl = leaf["lower"], leaf["lo_incl"], leaf["upper"], leaf["hi_incl"]
        # bytes compare as memcmp over the common length, then the shorter first
        return _by_distinct(v, lambda x: (lower is None or x > lower or (lo_incl and x == lower)) and
                            (upper is None or x < upper or (hi_incl and x == upper)))
    assert op == STR_MATCH, leaf
    rx = like_regex(like_pattern(leaf["segments"], leaf["head"], leaf["tail"]))
    return _by_distinct(v, lambda x: rx.fullmatch(x) is not None)


def leaf_mask(leaf, cols, nrows):
    """the rows a leaf is true on"""
    op = leaf["op"]
    if op == DICT_MAP:       # the map alone: an index >= n_in counts as code 2, the validity pointer is ignored
        idx, table, mode = cols.col[leaf["col"]].values[:nrows].astype(np.int64), np.asarray(leaf["map"], np.uint8), leaf["mode"]
        code = np.full(nrows, 2, np.uint8)
        inside = idx < len(table)
        code[inside] = table[idx[inside]]
        return {0: code == 1, 1: code == 0, 2: code == 2, 3: code != 2}[mode]
    valid = cols.valid[leaf["validity"]][:nrows] if leaf.get("validity") else np.ones(nrows, bool)   # no pointer: all valid
    if op == IS_NULL:
        return ~valid
    if op == IS_NOT_NULL:
        return valid.copy()
    m = compare(leaf, cols, nrows)
    return (~m if leaf.get("negate") else m) & valid


def evaluate(program, cols, nrows):
    """the rows a program keeps: the AND of its clauses, each the OR of its leaves; no clause keeps every row"""
    keep = np.ones(nrows, bool)
    for clause in program:
        assert clause, "an empty clause"
        m = np.zeros(nrows, bool)
        for leaf in clause:
            m |= leaf_mask(leaf, cols, nrows)
        keep &= m
    return keep


def n_leaves(program):
    return sum(len(c) for c in program)


def form_of(leaf, cols):
    name = {RANGE: "range", IN: "in", IS_NULL: "is_null", IS_NOT_NULL: "is_not_null", STR_IN: "str_in", DICT_MAP: "dict_map",
            STR_RANGE: "str_range", WIDE_RANGE: "wide_range", WIDE_IN: "wide_in", STR_MATCH: "str_match"}[leaf["op"]]
    return "float_" + name if leaf["op"] in (RANGE, IN) and cols.col[leaf["col"]].kind == "float" else name


def forms_of(program, cols):
    return {form_of(leaf, cols) for clause in program for leaf in clause}


# ---------------------------------------------------------------------------------------------------- what the kernel is handed
def _signed(v):
    v &= P64 - 1
    return v - P64 if v >= P63 else v


def string_t_words(c, address):
    """a string constant in kLeafStrIn's layout: {length | dword1 << 32, dword2 | dword3 << 32, device address of the bytes}"""
    image = np.zeros(16, np.uint8)
    image[0:4] = np.frombuffer(np.uint32(len(c)).tobytes(), np.uint8)
    if len(c) <= 12:
        image[4: 4 + len(c)] = np.frombuffer(c, np.uint8)
    else:
        image[4:8] = np.frombuffer(c[:4], np.uint8)      # prefix + 0 + 0
    w = image.view(np.int64)
    return [int(w[0]), int(w[1]), _signed(address)]


def _string_table(constants, base):
    """3 words per constant, then the bytes of all of them, each where its third word says, padded to 8 bytes"""
    words, blob, at = [], b"", 24 * len(constants)
    for c in constants:
        words += string_t_words(c, base + at + len(blob))
        blob += c
    out = np.array(words, np.int64).view(np.uint8).tobytes() + blob
    return np.frombuffer(out + b"\xee" * ((-len(out)) % 8 + 8), np.uint8).copy()


def table_image(leaf, cols, base):
    """the constant table of a leaf as it lies in HBM at device address `base` (its size does not depend on `base`), or None"""
    op, c = leaf["op"], cols.col[leaf["col"]] if leaf.get("col") else None
    if op == IN:
        if c.kind == "float":
            vals = [float_key(x, c.width) for x in leaf["values"]]
        else:
            vals = [_signed(x ^ P63) if c.type_flags() & F_BIAS else x for x in leaf["values"]]
        return np.array(vals + [0], np.int64).view(np.uint8).copy()
    if op == WIDE_RANGE:
        return np.array([_signed(x) for v in (leaf["lo"], leaf["hi"]) for x in (v, v >> 64)], np.int64).view(np.uint8).copy()
    if op == WIDE_IN:
        return np.array([_signed(x) for v in leaf["values"] for x in (v, v >> 64)] + [0, 0], np.int64).view(np.uint8).copy()
    if op == STR_IN:
        return _string_table(list(leaf["values"]), base)
    if op == STR_RANGE:
        return _string_table([leaf["lower"] or b"", leaf["upper"] or b""], base)
    if op == STR_MATCH:
        return _string_table(list(leaf["segments"]), base)
    if op == DICT_MAP:       # the map, then 64 bytes that would pass if they were read
        passing = {0: 1, 1: 0, 2: 2, 3: 1}[leaf["mode"]]
        return np.concatenate([np.asarray(leaf["map"], np.uint8), np.full(64, passing, np.uint8)])
    return None


def device_fields(leaf, cols, ends_clause, data, validity, in_values, heap=0):
    """the mi_filter_vector_leaf of a leaf, given the device addresses of its column, bitmap, table and (strings) heap"""
    op = leaf["op"]
    c = cols.col[leaf["col"]] if leaf.get("col") else None
    flags = (F_ENDS_CLAUSE if ends_clause else 0) | (F_NEGATE if leaf.get("negate") else 0)
    out = {"data": data, "validity": validity, "in_values": in_values, "op": op, "lo": 0, "hi": 0, "n_in": 0, "width": c.width if c else 0}
    if op in (RANGE, IN):
        flags |= c.type_flags()
    if op == RANGE:
        if c.kind == "float":
            out["lo"], out["hi"] = float_key(leaf["lo"], c.width), float_key(leaf["hi"], c.width)
        elif flags & F_BIAS:
            out["lo"], out["hi"] = _signed(leaf["lo"] ^ P63), _signed(leaf["hi"] ^ P63)
        else:
            out["lo"], out["hi"] = leaf["lo"], leaf["hi"]
    elif op in (IN, WIDE_IN, STR_IN):
        out["n_in"] = len(leaf["values"])
    elif op == STR_RANGE:
        out["n_in"] = (1 if leaf["lower"] is not None else 0) | (2 if leaf["lo_incl"] else 0) | (4 if leaf["upper"] is not None else 0) | \
            (8 if leaf["hi_incl"] else 0)
    elif op == STR_MATCH:
        out["n_in"] = len(leaf["segments"]) | (0x100 if leaf["head"] else 0) | (0x200 if leaf["tail"] else 0)
    elif op == DICT_MAP:
        out["n_in"], out["lo"] = len(leaf["map"]), leaf["mode"]
    if c is not None and c.kind == "str":
        out["lo"], out["hi"] = _signed(heap), _signed(c.ptr_base)
    out["flags"] = flags
    return out


def within_limits(program):
    """what mi_filter_program_vectors takes: at most 24 leaves, IN-lists of at most 256 constants, patterns of 1 .. 8 segments"""
    leaves = [leaf for clause in program for leaf in clause]
    return len(leaves) <= MAX_LEAVES and all(len(leaf.get("values", ())) <= 256 and 1 <= len(leaf.get("segments", (b"x",))) <= 8 and
                                             len(leaf.get("map", ())) < P63 for leaf in leaves)


def float_constants(program, cols):
    """(constant, width) of every float constant a program hands the kernel as a key"""
    out = []
    for clause in program:
        for leaf in clause:
            if leaf["op"] in (RANGE, IN) and cols.col[leaf["col"]].kind == "float":
                w = cols.col[leaf["col"]].width
                out += [(x, w) for x in (leaf["values"] if leaf["op"] == IN else (leaf["lo"], leaf["hi"]))]
    return out


# ---------------------------------------------------------------------------------------------------- the outputs
def check_outputs(sel, counts, keep, nrows, what=()):
    """sel: (windows + 1) * 2048 entries, counts: windows + 1, both filled with SENTINEL before the launch.  Every window's count
    and first `count` slots are the reference's ascending window-relative rows, the slots behind them, the guard window and the
    guard count still hold the sentinel."""
    windows = (nrows + WINDOW - 1) // WINDOW
    assert len(sel) == (windows + 1) * WINDOW and len(counts) == windows + 1 and len(keep) == nrows
    for w in range(windows):
        want = np.flatnonzero(keep[w * WINDOW: (w + 1) * WINDOW])
        assert counts[w] == len(want), what + (nrows, "window %d: the kernel keeps %d rows, the reference %d" % (w, counts[w], len(want)))
        got = sel[w * WINDOW: w * WINDOW + len(want)]
        if not np.array_equal(got, want):
            first = int(np.flatnonzero(got != want)[0])
            raise AssertionError(what + (nrows, "window %d slot %d: row %d, the reference has %d" % (w, first, got[first], want[first])))
        assert (sel[w * WINDOW + len(want): (w + 1) * WINDOW] == SENTINEL).all(), what + (nrows, "window %d: slots past the count were written" % w)
    assert (sel[windows * WINDOW:] == SENTINEL).all(), what + (nrows, "the guard window was written")
    assert counts[windows] == SENTINEL, what + (nrows, "the guard count was written")
    return int(keep.sum())


# ---------------------------------------------------------------------------------------------------- leaves with a wanted pass rate
INT_COLUMNS = ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64")
FLOAT_COLUMNS = ("f32", "f64")
STRING_COLUMNS = ("s_arrow", "s_shuf")


def _sorted_distinct(c, nrows):
    """(distinct values in the column's order, their share of the rows)"""
    v = c.values[:nrows]
    if c.kind == "float":
        with np.errstate(invalid="ignore"):
            u, n = np.unique(v, return_counts=True, equal_nan=True)     # NaN last, -0.0 = +0.0: the total order
        return list(u), n / nrows
    if c.kind == "int":
        u, n = np.unique(v, return_counts=True)
        return [int(x) for x in u], n / nrows
    counts = {}
    for x in v:
        counts[x] = counts.get(x, 0) + 1
    u = sorted(counts)
    return u, np.array([counts[x] for x in u]) / nrows


def _run(rng, share, p):
    """a run [i, j] of sorted distinct values whose share of the rows is about p"""
    i = int(rng.integers(0, len(share)))
    while i > 0 and share[i:].sum() < p:
        i -= 1
    j, got = i, share[i]
    while got < p and j + 1 < len(share):
        j += 1
        got += share[j]
    return i, j


def _subset(rng, share, p):
    order, got, out = rng.permutation(len(share)), 0.0, []
    for i in order:
        if got >= p and out:
            break
        out.append(int(i))
        got += share[i]
    return out


def random_leaf(rng, cols, nrows, form, p):
    """a leaf of `form` that is true on about the share p of the rows; which column, bitmap and constants is drawn"""
    pick = lambda names: names[int(rng.integers(len(names)))]
    negate = form in NEGATABLE and rng.random() < 0.35
    q = min(max(1.0 - p if negate else p, 0.0), 1.0)
    if form in ("is_null", "is_not_null"):
        name = pick(INT_COLUMNS + FLOAT_COLUMNS + ("hug",) + STRING_COLUMNS)
        return {"col": name, "op": IS_NULL if form == "is_null" else IS_NOT_NULL, "validity": name if rng.random() < 0.8 else pick(("seams", None))}
    if form == "dict_map":
        mode = int(rng.integers(0, 4))
        share = {0: q, 1: 1.0 - q, 2: 0.0, 3: 0.0}[mode]
        table = (rng.random(DICT_ENTRIES) < share).astype(np.uint8)
        table[rng.random(DICT_ENTRIES) < (q if mode == 2 else 1.0 - q if mode == 3 else 0.1)] = 2
        return {"col": "dict", "op": DICT_MAP, "map": table, "mode": mode, "validity": pick(("dict", "all_null", None))}
    name = pick({"range": INT_COLUMNS, "in": INT_COLUMNS, "float_range": FLOAT_COLUMNS, "float_in": FLOAT_COLUMNS, "wide_range": ("hug",),
                 "wide_in": ("hug",)}.get(form, STRING_COLUMNS))
    c = cols.col[name]
    leaf = {"col": name, "negate": negate, "validity": name if rng.random() < 0.6 and p < 0.8 else None}   # (NULL rows cap the pass rate)
    u, share = _sorted_distinct(c, nrows)
    if form in ("range", "float_range", "wide_range"):
        i, j = _run(rng, share, q)
        leaf.update(op=WIDE_RANGE if form == "wide_range" else RANGE, lo=u[i], hi=u[j])
        if form == "float_range":
            leaf.update(lo=float(u[i]), hi=float(u[j]))
    elif form in ("in", "float_in", "wide_in", "str_in"):
        vals = [u[i] for i in _subset(rng, share, q)][:255]
        if form == "float_in":
            vals = [float(x) for x in vals]
        leaf.update(op={"in": IN, "float_in": IN, "wide_in": WIDE_IN, "str_in": STR_IN}[form], values=vals + vals[:1])   # one of them twice
    elif form == "str_range":
        i, j = _run(rng, share, q)
        kind = int(rng.integers(0, 4))
        leaf.update(op=STR_RANGE, lower=None if kind == 1 and i == 0 else u[i], lo_incl=True, upper=None if kind == 2 and j == len(u) - 1 else u[j],
                    hi_incl=True)
        if kind == 3 and j + 1 < len(u):
            leaf.update(upper=u[j + 1], hi_incl=False)
    else:                    # str_match: one to three pieces of a value the column holds, in their order
        long_enough = [x for x in u if len(x) >= 3] or [b"abc"]
        v = long_enough[int(rng.integers(len(long_enough)))]
        cuts = sorted(int(x) for x in rng.integers(0, len(v) + 1, 2 * int(rng.integers(1, 4))))
        segs = [v[a:b] for a, b in zip(cuts[::2], cuts[1::2]) if b > a and b"%" not in v[a:b]] or [v[:1]]
        leaf.update(op=STR_MATCH, segments=segs, head=bool(cuts[0] == 0 and rng.random() < 0.5), tail=bool(cuts[-1] == len(v) and rng.random() < 0.5))
    return leaf


def clause_sizes(rng, leaves, clauses):
    """`clauses` sizes >= 1 that add up to `leaves`"""
    cuts = sorted(int(x) for x in rng.choice(np.arange(1, leaves), clauses - 1, replace=False)) if clauses > 1 else []
    return [b - a for a, b in zip([0] + cuts, cuts + [leaves])]


def random_program(rng, cols, nrows, sizes, forms):
    """a CNF with clauses of `sizes` leaves, the forms dealt out in turn from `forms` (an iterator), every leaf's pass rate set
    so that the program keeps about half of the rows"""
    clause_rate = 0.5 ** (1.0 / len(sizes))
    program = []
    for size in sizes:
        p = 1.0 - (1.0 - clause_rate) ** (1.0 / size)
        program.append([random_leaf(rng, cols, nrows, next(forms), p) for _ in range(size)])
    return program


RANDOM_SEED = 20250917
RANDOM_SHAPES = (9, 65, 2047, 2049, 8193, 5 * 2048 + 5)


_random = {}


def random_programs(seed=RANDOM_SEED):
    """random_cnfs(seed), made once and never changed"""
    if seed not in _random:
        _random[seed] = random_cnfs(seed)
    return _random[seed]


def random_cnfs(seed):
    """[(nrows, program)]: 96 seeded CNFs -- every leaf count 1 .. 24 four times over, clause counts from one clause of all leaves
    to one clause per leaf, 24 leaves in one clause and 24 clauses of one leaf among them -- over the columns of six shapes"""
    rng = np.random.default_rng(seed)

    def deal():
        while True:
            for i in rng.permutation(len(FORMS)):
                yield FORMS[int(i)]
    forms = deal()
    out = []
    for rep in range(4):
        for leaves in range(1, MAX_LEAVES + 1):
            clauses = (1, leaves, max(1, leaves // 2), int(rng.integers(1, leaves + 1)))[rep]
            nrows = RANDOM_SHAPES[(leaves + rep) % len(RANDOM_SHAPES)]
            out.append((nrows, random_program(rng, columns(nrows), nrows, clause_sizes(rng, leaves, clauses), forms)))
    return out


def vacuity(programs):
    """(programs that keep neither no row nor every row, {form: programs it appears in})"""
    mixed, seen = 0, {f: 0 for f in FORMS}
    for nrows, program in programs:
        kept = int(evaluate(program, columns(nrows), nrows).sum())
        mixed += 0 < kept < nrows
        for f in forms_of(program, columns(nrows)):
            seen[f] += 1
    return mixed, seen


# ---------------------------------------------------------------------------------------------------- programs written by hand
def L(col, op, validity="own", negate=False, **constants):
    """a leaf; validity "own" = the column's own bitmap, None = no pointer"""
    return dict(constants, col=col, op=op, validity=col if validity == "own" else validity, negate=negate)


def _both(name, leaf):
    """a one-leaf program, plain and negated"""
    return [(name, [[leaf]]), (name + " negated", [[dict(leaf, negate=True)]])]


LONG_STRINGS = (sc.BASE[:13], sc.BASE[:12] + b"\x80", sc.BASE[:16] + b"\xff")


def unemitted_programs():
    """[(name, program)] of what NormaliseFilter never hands the kernel: ranges on one column it would merge or drop, a leaf
    twice in a clause, lo > hi, kLeafNegate on every form that takes it, IN-lists of 0, 1 and 256 values, uint64 ranges at the
    ends of both halves, unsigned ranges at their maxima"""
    R = lambda lo, hi, col="i32", **kw: L(col, RANGE, lo=lo, hi=hi, **kw)
    out = [("overlapping", [[R(-2, 1)], [R(0, 3)]]), ("touching", [[R(-3, 0)], [R(0, 3)]]), ("contradictory", [[R(-3, -1)], [R(1, 3)]]),
           ("three ranges", [[R(-3, 2)], [R(-1, 3, validity=None)], [R(0, 0)]]), ("three ranges, none left", [[R(-3, 0)], [R(0, 3)], [R(1, 2)]]),
           ("touching, 64 bits", [[R(-P63, 0, "i64")], [R(0, P63 - 1, "i64")]]),
           ("a leaf twice", [[R(0, 1), R(0, 1)]]), ("a leaf twice, and its negation", [[R(0, 1), R(0, 1), R(0, 1, negate=True)]])]
    out += _both("lo > hi", R(5, -5)) + _both("lo > hi, no validity", R(5, -5, validity=None)) + _both("lo > hi, 8 bits", R(1, 0, "i8"))
    out += _both("in", L("i16", IN, values=[-1, 0, 32767, -32768]))
    out += _both("in, none", L("i16", IN, values=[])) + _both("in, one", L("i16", IN, values=[1]))
    out += _both("in, 256", L("i16", IN, values=list(range(-120, 135)) + [32767])) + _both("in, 256, 64 bits", L("u64", IN, values=[P64 - 1, P63] + list(range(254))))
    out += _both("wide in", L("hug", WIDE_IN, values=[P63, -P64 - 1, 0, P64])) + _both("wide in, none", L("hug", WIDE_IN, values=[]))
    out += _both("wide range", L("hug", WIDE_RANGE, lo=-P63 - 1, hi=P64)) + _both("wide range, lo > hi", L("hug", WIDE_RANGE, lo=P64, hi=-P64))
    out += _both("wide range at 2^64", L("hug", WIDE_RANGE, lo=P64 - 1, hi=P64 - 1))
    for col in STRING_COLUMNS:
        out += _both("str in " + col, L(col, STR_IN, values=[b"", sc.BASE[:4], LONG_STRINGS[0], LONG_STRINGS[2], b"absent"]))
        out += _both("str in, none " + col, L(col, STR_IN, values=[]))
        out += _both("str range " + col, L(col, STR_RANGE, lower=sc.BASE[:4], lo_incl=False, upper=LONG_STRINGS[1], hi_incl=True))
        out += _both("str range, lower above upper " + col, L(col, STR_RANGE, lower=b"tail", lo_incl=True, upper=b"L", hi_incl=True))
        out += _both("str range, one end " + col, L(col, STR_RANGE, lower=None, lo_incl=False, upper=sc.BASE[:12], hi_incl=False))
        out += _both("str match " + col, L(col, STR_MATCH, segments=[b"kji", b"e"], head=True, tail=False))
        out += _both("str match, tail " + col, L(col, STR_MATCH, segments=[b"\xff"], head=False, tail=True))
        out += _both("str match, 13 bytes " + col, L(col, STR_MATCH, segments=[LONG_STRINGS[0]], head=False, tail=False))
    for col in FLOAT_COLUMNS:
        out += _both("NaN .. NaN " + col, L(col, RANGE, lo=NAN, hi=NAN)) + _both("-inf .. -0.0 " + col, L(col, RANGE, lo=-INF, hi=-0.0))
        out += _both("inf .. NaN " + col, L(col, RANGE, lo=INF, hi=NAN)) + _both("float lo > hi " + col, L(col, RANGE, lo=NAN, hi=1.5))
        out += _both("float in " + col, L(col, IN, values=[NAN, -0.0, 1.5, 1.3, -INF]))
    for lo, hi in ((0, 0), (0, P63 - 1), (P63 - 1, P63 - 1), (P63 - 1, P63), (P63, P63), (P63, P64 - 1), (P64 - 1, P64 - 1), (1, P64 - 2), (P63, P63 - 1)):
        out += _both("uint64 %#x .. %#x" % (lo, hi), R(lo, hi, "u64"))
    for col, top in (("u8", 255), ("u16", 65535), ("u32", P64 >> 32)):
        top = top - (col == "u32")
        out += _both("%s at its maximum" % col, R(top, top, col)) + _both("%s upper half" % col, R(top // 2 + 1, top, col))
        out += _both("%s below its maximum" % col, R(0, top - 1, col)) + _both("%s in" % col, L(col, IN, values=[top, 0, top // 2 + 1]))
    return out


VALIDITY_LEAVES = (L("i32", RANGE, lo=-1, hi=2), L("f64", RANGE, lo=-2.5, hi=NAN), L("hug", WIDE_RANGE, lo=-P64, hi=P63),
                   L("s_arrow", STR_RANGE, lower=sc.BASE[:3], lo_incl=True, upper=None, hi_incl=False), L("i8", IN, values=[-128, 127, 0]))
BITMAPS = ("all_valid", None, "all_null", "seams")


def validity_programs():
    """the same leaf under all-valid words, no pointer, all-NULL words and the seam bitmap; negated; beside IS NULL; IS NULL alone"""
    out = []
    for leaf in VALIDITY_LEAVES:
        for b in BITMAPS:
            tag = "%s under %s" % (leaf["col"], b)
            out += _both(tag, dict(leaf, validity=b))
            out.append((tag + ": is null", [[L(leaf["col"], IS_NULL, validity=b)]]))
            out.append((tag + ": is not null", [[L(leaf["col"], IS_NOT_NULL, validity=b)]]))
            out.append((tag + ": is null or", [[L(leaf["col"], IS_NULL, validity=b), dict(leaf, validity=b)]]))
            out.append((tag + ": is null or not", [[dict(leaf, validity=b, negate=True), L(leaf["col"], IS_NULL, validity=b)]]))
    return out


def dict_map_programs():
    """modes 0 .. 3 under no pointer, the column's bitmap and all-zero words: the bitmap changes nothing.  The last entry of the
    map (index n_in - 1) has a code of its own; index n_in and 0xFFFFFFFF are past the map, where bytes lie that would pass"""
    out = []
    for mode in range(4):
        for j, table in enumerate((np.array([1, 0, 2, 1, 0] * 8, np.uint8), np.array([0] * 39 + [1], np.uint8), np.array([2] * 39 + [0], np.uint8),
                                   np.array([1] * 20, np.uint8), np.zeros(0, np.uint8))):
            for b in (None, "dict", "all_null"):
                out.append(("dict map %d, mode %d, under %s" % (j, mode, b), [[L("dict", DICT_MAP, validity=b, map=table, mode=mode)]]))
    return out


def neutral_leaf(kind):
    """a leaf every row passes, for a clause of its own: it changes the instance the launcher picks and no row"""
    return {"float": L("f32", RANGE, validity=None, lo=-INF, hi=NAN), "wide": L("hug", WIDE_RANGE, validity=None, lo=-(1 << 127), hi=(1 << 127) - 1),
            "pattern": L("s_shuf", STR_MATCH, validity=None, negate=True, segments=[b"no row holds this"], head=False, tail=False)}[kind]


def base_program():
    """integer, string and dictionary leaves: what filter_program<false> runs"""
    return [[L("i32", RANGE, lo=-2, hi=1), L("s_arrow", STR_IN, values=[sc.BASE[:4], LONG_STRINGS[0], b""]), L("u64", RANGE, lo=P63, hi=P64 - 1, negate=True)],
            [L("dict", DICT_MAP, validity=None, map=np.array([1, 0, 2, 1, 0] * 8, np.uint8), mode=3), L("i8", IS_NULL)],
            [L("s_shuf", STR_RANGE, lower=sc.BASE[:1], lo_incl=True, upper=sc.BASE[:13], hi_incl=False, negate=True), L("u16", IN, values=[65535, 0, 1])]]


def instance_programs():
    """[(name, program, instance)]: instance 0 = filter_program<false>, 1 = <true>, 2 = <true, true>"""
    base = base_program()
    return [("base", base, 0), ("base + float", base + [[neutral_leaf("float")]], 1), ("base + wide", [[neutral_leaf("wide")]] + base, 1),
            ("base + pattern", base + [[neutral_leaf("pattern")]], 2),
            ("base + float + wide + pattern", [[neutral_leaf("float")]] + base + [[neutral_leaf("pattern")], [neutral_leaf("wide")]], 2)]


def handwritten_programs():
    """every (name, program) above"""
    return unemitted_programs() + validity_programs() + dict_map_programs() + [(n, p) for n, p, _ in instance_programs()]

"""K10 at the kernel level (mi_group_aggregate_vectors): group_windows + group_combine over resident vectors, with key
columns, validity words and selection vectors built by hand, against a Python dict loop over Python ints, math.fsum and
Python's sort with NULLS LAST.  Expected values never come from the library.

Float sums are compared with math.fsum per group under the bound of test_gpu_aggregate_vectors.py, which holds for ANY
summation order of n doubles: |err| <= 2 n 2^-53 sum|x_i| (Higham 4.2, rounded up).  Everything else is exact."""
import math
import struct

import numpy as np
import pytest
import torch

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

W = 2048
INT_TYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _words(ok):
    bits = np.zeros((len(ok) + 63) // 64 * 64 + 64, np.uint8)
    bits[: len(ok)] = ok
    return np.packbits(bits, bitorder="little").view(np.uint64)


def string_rows(values, pad=0xFF):
    """bytes per row -> 16-byte string_t images: uint32 length, then the bytes and `pad` behind them; a value longer than 12
    bytes gets its 4-byte prefix and a pointer that names no memory of this process"""
    out = np.full((len(values), 16), pad, np.uint8)
    for i, v in enumerate(values):
        out[i, :4] = np.frombuffer(struct.pack("<I", len(v)), np.uint8)
        if len(v) <= 12:
            out[i, 4: 4 + len(v)] = np.frombuffer(v, np.uint8)
        else:
            out[i, 4:8] = np.frombuffer(v[:4], np.uint8)
            out[i, 8:16] = np.frombuffer(struct.pack("<Q", 0xDEAD00000000BEE0 + i), np.uint8)
    return out


class Column:
    """values, which rows are valid, and the copies in HBM.  cls: signed / unsigned / float (numpy), wide (Python ints),
    string (bytes; `raw` overrides the 16-byte rows)"""

    def __init__(self, values, cls, ok=None, offset=0, raw=None):
        if cls == "wide":
            self.py = [int(v) for v in values]
            payload = np.array([[v & ((1 << 64) - 1), (v >> 64) & ((1 << 64) - 1)] for v in self.py], np.uint64).reshape(-1, 2)
            self.width = 16
        elif cls == "string":
            self.py = [bytes(v) for v in values]
            payload = string_rows(self.py) if raw is None else raw
            self.width = 16
        else:
            values = np.asarray(values)
            self.py = [float(v) for v in values] if cls == "float" else [int(v) for v in values]
            payload = values
            self.width = values.dtype.itemsize
        self.cls = cls
        self.ok = np.ones(len(self.py), bool) if ok is None else np.asarray(ok, bool)
        flat = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self._data = _dev(np.concatenate([np.zeros(offset, np.uint8), flat]))
        self.ptr = self._data.data_ptr() + offset
        self._valid = None if ok is None else _dev(_words(self.ok))

    def spec(self):
        return (self.ptr, 0 if self._valid is None else self._valid.data_ptr(), self.width, self.cls)

    def key(self, r):
        return self.py[r] if self.ok[r] else None


class Selection:
    def __init__(self, per_window, slots=None):
        self.per_window = per_window
        sel = np.full(slots if slots is not None else len(per_window) * W, 0xFFFFFFFF, np.uint32)   # slots never read hold a poison index
        for w, rows in enumerate(per_window):
            sel[w * W: w * W + len(rows)] = rows
        self._sel, self._cnt = _dev(sel), _dev(np.array([len(r) for r in per_window], np.uint32))
        self.ptrs = (self._sel.data_ptr(), self._cnt.data_ptr())

    def rows(self):
        return [w * W + r for w, rows in enumerate(self.per_window) for r in rows]


def _wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def expected(op, cols, rows):
    """-> (kind, value, contributing rows); kind 'exact' or 'sum' (the doubles that were summed)"""
    if op == "count_star":
        return "exact", len(rows), len(rows)
    rows = [r for r in rows if all(c.ok[r] for c in cols)]
    a = cols[0]
    if op == "count":
        return "exact", len(rows), len(rows)
    vals = [a.py[r] for r in rows]
    if op == "sum_product":
        vals = [x * cols[1].py[r] for x, r in zip(vals, rows)]
    if not rows:
        return "exact", None, 0
    if a.cls == "float":
        if op in ("sum", "sum_product"):
            return "sum", vals, len(rows)
        return "exact", (min if op == "min" else max)(vals) + 0.0, len(rows)      # (no NaN in these tables)
    if op in ("sum", "sum_product"):
        return "exact", _wrap128(sum(vals)), len(rows)
    return "exact", (min if op == "min" else max)(vals), len(rows)


def check(got, want, what):
    kind, value, count = want
    got_value, got_count = got
    assert got_count == count, (what, got, count)
    if kind == "sum":
        exact = math.fsum(value)
        bound = 2 * len(value) * 2.0 ** -53 * math.fsum(abs(v) for v in value)
        assert abs(got_value - exact) <= bound, (what, got_value, exact, bound)
    elif isinstance(value, float):
        assert isinstance(got_value, float) and _bits(got_value) == _bits(value), (what, got_value, value)
    else:
        assert got_value == value and (value is None or isinstance(got_value, int)), (what, got_value, value)


def order_key(key):
    """ascending part by part, NULLS LAST; ints by value, bytes bytewise and then shorter first (Python's order of bytes)"""
    return tuple((1, 0) if k is None else (0, k) for k in key)


def group_rows(keys, rows):
    groups = {}
    for r in rows:
        groups.setdefault(tuple(k.key(r) for k in keys), []).append(r)
    return groups


def run_and_check(ctx, keys, aggs, nrows, selection=None, what=""):
    rows = selection.rows() if selection is not None else list(range(nrows))
    groups = group_rows(keys, rows)
    want_keys = sorted(groups, key=order_key)
    specs = [(op,) + tuple(c.spec() for c in cols) for op, *cols in aggs]
    sel_ptr, cnt_ptr = selection.ptrs if selection is not None else (0, 0)
    got = da.group_aggregate_vectors(ctx, [k.spec() for k in keys], specs, nrows, sel_ptr, cnt_ptr, detail=True)
    assert [g[0] for g in got] == want_keys, (what, [g[0] for g in got][:8], want_keys[:8])
    for key, values in got:
        assert len(values) == len(aggs)
        for (op, *cols), g in zip(aggs, values):
            check(g, expected(op, cols, groups[key]), "%s group %r %s" % (what, key, op))
    return got


NMAX = 2 * W + 5


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2026)
    t = {}
    k32 = rng.integers(-2, 3, NMAX).astype(np.int32)
    k32[NMAX - 1] = 999                                     # a group that occurs only in the ragged last window
    ok32 = rng.random(NMAX) >= 0.1
    ok32[NMAX - 1] = True
    t["k32"] = Column(k32, "signed", ok32)
    t["ks"] = Column([(b"", b"A", b"N", b"abcdefghijkl")[i] for i in rng.integers(0, 4, NMAX)], "string", rng.random(NMAX) >= 0.1)
    t["i64"] = Column(rng.integers(-(1 << 62), 1 << 62, NMAX), "signed", rng.random(NMAX) >= 0.15)
    t["i32"] = Column(rng.integers(-1000, 1000, NMAX).astype(np.int32), "signed")
    t["u64"] = Column(rng.integers(0, (1 << 64) - 1, NMAX, dtype=np.uint64), "unsigned", rng.random(NMAX) >= 0.15)
    t["u16"] = Column(rng.integers(0, 65535, NMAX).astype(np.uint16), "unsigned")
    t["f64"] = Column(rng.normal(0, 1, NMAX) * 10.0 ** rng.integers(-12, 13, NMAX), "float", rng.random(NMAX) >= 0.15)
    t["f32"] = Column(rng.normal(0, 1e3, NMAX).astype(np.float32), "float")
    wide = [(int(rng.integers(-(1 << 62), 1 << 62)) << 60) + int(rng.integers(0, 1 << 60)) for _ in range(NMAX)]
    t["wide"] = Column(wide, "wide", rng.random(NMAX) >= 0.15)
    return t


def _few(t):
    return [("count_star",), ("count", t["wide"]), ("sum", t["i64"]), ("sum", t["f64"]), ("min", t["wide"]), ("max", t["f32"]),
            ("sum_product", t["i32"], t["u64"]), ("min", t["u16"])]


@pytest.mark.parametrize("nrows", [1, 2047, 2048, 2049, 2 * W + 5])
def test_row_count_seams_with_and_without_a_selection(ctx, table, nrows):
    keys = [table["k32"], table["ks"]]
    got = run_and_check(ctx, keys, _few(table), nrows, what="every row, n=%d" % nrows)
    if nrows == NMAX:
        assert any(k[0] == 999 for k, _ in got)
    rng = np.random.default_rng(nrows)
    per_window = []
    for w in range((nrows + W - 1) // W):
        n = min(W, nrows - w * W)
        per_window.append(sorted(rng.choice(n, max(1, n // 3), replace=False).tolist()))
    if nrows == NMAX:
        per_window[-1] = [0, 4]                             # row NMAX - 1: the group of the ragged last window alone
    got = run_and_check(ctx, keys, _few(table), nrows, Selection(per_window), what="selection, n=%d" % nrows)
    if nrows == NMAX:
        assert any(k[0] == 999 for k, _ in got)


def test_a_window_without_selected_rows_between_two_populated_ones(ctx, table):
    rng = np.random.default_rng(3)
    for per_window in ([sorted(rng.choice(W, 700, replace=False).tolist()), [], [0, 2, 4]], [list(range(W)), [], list(range(5))],
                       [[], [], [4]], [list(range(W - 1, -1, -1)), [], [4, 3, 3, 0]]):          # descending, a row twice
        run_and_check(ctx, [table["ks"], table["k32"]], _few(table), NMAX, Selection(per_window), what="empty middle window")
    nothing = Selection([[], [], []])          # (named: device memory lives as long as the object)
    assert da.group_aggregate_vectors(ctx, [table["k32"].spec()], [("count_star",)], NMAX, *nothing.ptrs) == []
    assert da.group_aggregate_vectors(ctx, [table["k32"].spec()], [("count_star",)], 0) == []


@pytest.mark.parametrize("size", [1, 63, 64, 65, 255, 256, 257, 2048])
def test_group_sizes_at_the_lane_and_wave_seams_of_the_fold(ctx, size):
    """a group of `size` rows scattered among the rows of a second group (for 2048: the whole window, the second group in the next)"""
    rng = np.random.default_rng(size)
    n = W if size < W else W + 300
    key = np.full(n, 7, np.int16)
    key[rng.choice(W, size, replace=False)] = -3
    if size == W:
        key[W + rng.choice(300, 100, replace=False)] = -3
    f = Column(rng.normal(0, 1, n) * 10.0 ** rng.integers(-10, 11, n), "float", rng.random(n) >= 0.1)
    i = Column(rng.integers(-(1 << 62), 1 << 62, n), "signed")
    k = Column(key, "signed")
    aggs = [("count_star",), ("sum", f), ("sum", i), ("min", i), ("max", f), ("count", f)]
    got = run_and_check(ctx, [k], aggs, n, what="group of %d" % size)
    assert got[0][0] == (-3,) and got[0][1][0][0] == size + (100 if size == W else 0)
    again = da.group_aggregate_vectors(ctx, [k.spec()], [(op,) + tuple(c.spec() for c in cols) for op, *cols in aggs], n, detail=True)
    sums = lambda result: [None if g[1][1][0] is None else _bits(g[1][1][0]) for g in result]
    assert sums(again) == sums(got)


def _fresh_keys(n_windows, per_window, rows_per_key):
    """window w holds keys w * per_window .. (w + 1) * per_window - 1, each rows_per_key times, shuffled"""
    rng = np.random.default_rng(per_window)
    out = []
    for w in range(n_windows):
        block = np.repeat(np.arange(w * per_window, (w + 1) * per_window), rows_per_key)
        block = np.concatenate([block, np.full(W - len(block), w * per_window)])
        rng.shuffle(block)
        out.append(block)
    return np.concatenate(out).astype(np.int32)


@pytest.mark.parametrize("distinct", [1, 2, 255, 256])
def test_distinct_keys_in_one_window_up_to_the_limit(ctx, distinct):
    key = Column(_fresh_keys(2, distinct, W // distinct), "signed")
    v = Column(np.arange(2 * W, dtype=np.int64), "signed")
    got = run_and_check(ctx, [key], [("count_star",), ("sum", v), ("max", v)], 2 * W, what="%d keys per window" % distinct)
    assert len(got) == 2 * distinct


def test_one_key_past_the_window_limit_is_refused_without_a_fault(ctx):
    assert _ffi.GROUP_WINDOW_LIMIT == 256
    k = np.zeros(2 * W, np.int32)
    k[W: W + 257] = np.arange(257)                           # window 1: 257 distinct keys
    key, v = Column(k, "signed"), Column(np.arange(2 * W, dtype=np.int64), "signed")
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("sum", v.spec())], 2 * W)
    assert e.value.code == _ffi.MI_ENOTSUP and "GROUP BY with more than" in str(e.value) and "stays above the scan" in str(e.value)
    # every row a key of its own: far past the limit in every window
    key = Column(np.arange(2 * W, dtype=np.int64), "signed")
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("count_star",)], 2 * W)
    assert e.value.code == _ffi.MI_ENOTSUP
    # the same context goes on: the 257 keys spread over two windows are fine
    k = np.zeros(2 * W, np.int32)
    k[W - 128: W + 129] = np.arange(257)
    key = Column(k, "signed")
    assert len(run_and_check(ctx, [key], [("sum", v)], 2 * W, what="257 keys over two windows")) == 257


def test_exactly_4096_groups_succeed_one_more_is_refused_and_a_short_capacity_says_so(ctx):
    assert _ffi.MAX_GROUPS == 4096
    n = 17 * W
    k = _fresh_keys(17, 256, 8)
    k[16 * W:] = np.repeat(np.arange(0, 4096, 16), 8)        # the 17th window meets 256 keys of the 16 before it
    key, v = Column(k, "signed"), Column(np.arange(n, dtype=np.int64) - 5000, "signed")
    got = run_and_check(ctx, [key], [("count_star",), ("sum", v), ("min", v)], n, what="4096 groups")
    assert len(got) == 4096 and got[0][1][0][0] == 16 and got[1][1][0][0] == 8
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("count_star",)], n, capacity=4095)
    assert e.value.code == _ffi.MI_EINVAL and "4096" in str(e.value) and "4095" in str(e.value)
    last = np.arange(0, 4096, 16)
    last[-1] = 4096                                           # one key more, in a window that stays inside its own limit
    k[16 * W:] = np.repeat(last, 8)
    key = Column(k, "signed")
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("count_star",)], n)
    assert e.value.code == _ffi.MI_ENOTSUP and "GROUP BY with more than" in str(e.value)


def test_a_short_capacity_sets_n_groups(ctx):
    import ctypes as C
    key = Column(np.arange(10, dtype=np.int32) % 5, "signed")
    karr = (_ffi.GroupKeyColumn * 1)()
    karr[0].data, karr[0].validity, karr[0].width, karr[0].key_class = key.ptr, None, 4, _ffi.GROUP_KEY_CLASS_SIGNED
    arr = (_ffi.AggVectorSpec * 1)()
    arr[0].op = _ffi.AGG_COUNT_STAR
    out_k, out_v, n_groups = (_ffi.GroupKeyValue * 4)(), (_ffi.AggValue * 4)(), C.c_int32(-1)
    rc = _ffi.lib().mi_group_aggregate_vectors(ctx._h, karr, 1, arr, 1, None, None, 10, out_k, out_v, 4, C.byref(n_groups), None)
    assert rc == _ffi.MI_EINVAL and n_groups.value == 5
    out_k, out_v = (_ffi.GroupKeyValue * 5)(), (_ffi.AggValue * 5)()
    rc = _ffi.lib().mi_group_aggregate_vectors(ctx._h, karr, 1, arr, 1, None, None, 10, out_k, out_v, 5, C.byref(n_groups), None)
    assert rc == _ffi.MI_OK and n_groups.value == 5 and [v.lo for v in out_v] == [2] * 5
    assert [int.from_bytes(bytes(k.bytes), "little", signed=True) for k in out_k] == [0, 1, 2, 3, 4]
    assert all(k.kind == _ffi.GROUP_KEY_INT128 and not k.is_null for k in out_k)


@pytest.mark.parametrize("name", sorted(INT_TYPES))
def test_integer_keys_at_their_minima_and_maxima(ctx, name):
    t = INT_TYPES[name]
    info = np.iinfo(t)
    rng = np.random.default_rng(len(name))
    pool = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1, info.max // 2 + 1, info.max // 2], dtype=t)
    k = pool[rng.integers(0, len(pool), W + 9)]
    key = Column(k, "unsigned" if name[0] == "u" else "signed", rng.random(len(k)) >= 0.05)
    v = Column(rng.integers(-100, 100, len(k)), "signed")
    got = run_and_check(ctx, [key], [("count_star",), ("sum", v)], len(k), what=name)
    ints = [g[0][0] for g in got if g[0][0] is not None]
    assert ints == sorted(ints) and ints[0] == int(info.min) and ints[-1] == int(info.max) and got[-1][0] == (None,)


def test_minus_one_as_int8_and_255_as_uint8_and_uint64_past_int64(ctx):
    v = Column(np.arange(6, dtype=np.int64), "signed")
    raw = np.array([0xFF, 0x7F, 0x80, 0, 0xFF, 1], np.uint8)
    as_i8, as_u8 = Column(raw.view(np.int8), "signed"), Column(raw, "unsigned")      # (named: device memory lives as long as the object)
    assert [g[0] for g in da.group_aggregate_vectors(ctx, [as_i8.spec()], [("count_star",)], 6)] == [(-128,), (-1,), (0,), (1,), (127,)]
    assert [g[0] for g in da.group_aggregate_vectors(ctx, [as_u8.spec()], [("count_star",)], 6)] == [(0,), (1,), (127,), (128,), (255,)]
    u = np.array([(1 << 63) - 1, 1 << 63, (1 << 64) - 1, 0, 1 << 63, (1 << 63) - 1], np.uint64)
    as_u64 = Column(u, "unsigned")
    got = run_and_check(ctx, [as_u64], [("count_star",), ("sum", v)], 6, what="u64")
    assert [g[0][0] for g in got] == [0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
    as_i64 = Column(u.view(np.int64), "signed")
    assert [g[0][0] for g in da.group_aggregate_vectors(ctx, [as_i64.spec()], [("count_star",)], 6)] == [-(1 << 63), -1, 0, (1 << 63) - 1]


def test_wide_keys_at_8_mod_16(ctx):
    rng = np.random.default_rng(13)
    n = W + 77
    pool = [-(1 << 127), (1 << 127) - 1, 0, -1, (1 << 64), (1 << 64) - 1, -(1 << 64), (1 << 64) + 3, -(1 << 64) - 3, 1 << 100]
    k = Column([pool[i] for i in rng.integers(0, len(pool), n)], "wide", rng.random(n) > 0.1, offset=8)
    assert k.ptr % 16 == 8
    v = Column(rng.integers(-100, 100, n), "signed")
    got = run_and_check(ctx, [k], [("count_star",), ("sum", v), ("min", k), ("max", k)], n, what="wide 8 mod 16")
    assert [g[0][0] for g in got] == sorted(pool) + [None]


def test_string_keys_lengths_padding_empty_against_null_and_a_trailing_zero(ctx):
    rng = np.random.default_rng(21)
    pool = [b"", b"a", b"a\0", b"abcd", b"abcde", b"abcdefghijkl", b"abcdefghijk\0", b"\xff", b"b", b"\0"]
    n = W + 50
    values = [pool[i] for i in rng.integers(0, len(pool), n)]
    ok = rng.random(n) >= 0.1
    raw = string_rows(values, pad=0xFF)
    # NULL rows carry a length of 0xFFFFFFFF and pointers outside any heap: they are the NULL group and raise no flag
    raw[~ok] = 0xFF
    # and valid rows of one value carry different paddings: one group all the same
    alt = string_rows(values, pad=0x5A)
    swap = ok & (rng.random(n) < 0.5)
    raw[swap] = alt[swap]
    key = Column(values, "string", ok, raw=raw)
    v = Column(rng.integers(-100, 100, n), "signed")
    got = run_and_check(ctx, [key], [("count_star",), ("sum", v)], n, what="strings")
    assert [g[0][0] for g in got] == sorted(pool) + [None]
    assert sorted(pool).index(b"a") + 1 == sorted(pool).index(b"a\0") and sorted(pool)[0] == b""


def test_a_selected_string_key_of_13_bytes_is_refused_and_the_same_row_deselected_is_not(ctx):
    values = [b"N", b"O", b"thirteen bytes", b"N", b"O"] * 3
    key = Column(values, "string")
    v = Column(np.arange(15, dtype=np.int64), "signed")
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("sum", v.spec())], 15)
    assert e.value.code == _ffi.MI_ENOTSUP and "a VARCHAR / BLOB group key longer than 12 bytes stays above the scan" in str(e.value)
    keep = Selection([[r for r in range(15) if r % 5 != 2]])
    got = run_and_check(ctx, [key], [("sum", v), ("count_star",)], 15, keep, what="long string deselected")
    assert [g[0] for g in got] == [(b"N",), (b"O",)]
    # a NULL row of 13 bytes is no long key either
    ok = np.array([r % 5 != 2 for r in range(15)])
    under_null = Column(values, "string", ok)
    got = run_and_check(ctx, [under_null], [("count_star",)], 15, what="long string under NULL")
    assert [g[0] for g in got] == [(b"N",), (b"O",), (None,)]


@pytest.mark.parametrize("n_keys", [2, 3, 4])
def test_key_combinations_with_nulls_in_every_position(ctx, n_keys):
    rng = np.random.default_rng(n_keys)
    n = W + 200
    cols = [Column(rng.integers(1, 3, n).astype(np.int32), "signed", rng.random(n) >= 0.3),
            Column([(b"x", b"y")[i] for i in rng.integers(0, 2, n)], "string", rng.random(n) >= 0.3),
            Column(rng.integers(1, 3, n).astype(np.uint8), "unsigned", rng.random(n) >= 0.3),
            Column([int(x) << 70 for x in rng.integers(-1, 1, n)], "wide", rng.random(n) >= 0.3)][:n_keys]
    v = Column(rng.integers(-100, 100, n), "signed", rng.random(n) >= 0.2)
    got = run_and_check(ctx, cols, [("count_star",), ("sum", v), ("count", v)], n, what="%d keys" % n_keys)
    keys = [g[0] for g in got]
    assert len(keys) == 3 ** n_keys and keys[-1] == (None,) * n_keys
    if n_keys == 2:      # (NULL, x), (NULL, y), (1, NULL), (NULL, NULL) are four groups
        assert {(None, b"x"), (None, b"y"), (1, None), (None, None)} <= set(keys)


def test_every_operation_and_class_per_group_with_an_all_null_group(ctx, table):
    rng = np.random.default_rng(99)
    n = NMAX
    k = rng.integers(0, 4, n).astype(np.int8)
    key = Column(k, "signed")
    cols = {}
    for name, t in INT_TYPES.items():
        info = np.iinfo(t)
        cols[name] = Column(rng.integers(info.min, info.max, n, dtype=t, endpoint=True), "unsigned" if name[0] == "u" else "signed", (rng.random(n) >= 0.15) & (k != 3))
    cols["f32"] = Column(rng.normal(0, 1e3, n).astype(np.float32), "float", (rng.random(n) >= 0.15) & (k != 3))
    cols["f64"] = Column(rng.normal(0, 1e6, n) * rng.choice([1e-9, 1.0, 1e9], n), "float", (rng.random(n) >= 0.15) & (k != 3))
    cols["wide"] = Column([int(rng.integers(-(1 << 62), 1 << 62)) << int(rng.integers(0, 65)) for _ in range(n)], "wide", (rng.random(n) >= 0.15) & (k != 3))
    aggs = [("count_star",)]
    for name, c in cols.items():
        aggs += [("count", c), ("min", c), ("max", c)]
        if c.cls != "wide":
            aggs.append(("sum", c))
    aggs += [("sum_product", cols["i64"], cols["i32"]), ("sum_product", cols["u64"], cols["i8"]), ("sum_product", cols["f32"], cols["f64"]),
             ("sum_product", cols["f64"], cols["f64"])]
    for first in range(0, len(aggs), 8):
        part = aggs[first: first + 8]
        got = run_and_check(ctx, [key], part, n, what="all classes")
        null_group = dict(got)[(3,)]          # every input of group 3 is NULL: present, SUM / MIN / MAX NULL, COUNT 0
        for (op, *_), g in zip(part, null_group):
            assert (g[0] > 0) if op == "count_star" else g == ((0, 0) if op == "count" else (None, 0)), (op, g)


def test_double_sums_per_group_are_bit_reproducible(ctx):
    rng = np.random.default_rng(11)
    for n in (257, 2048, NMAX, 5 * W + 1):
        x = Column(rng.normal(0, 1, n) * 10.0 ** rng.integers(-12, 13, n), "float", rng.random(n) > 0.1)
        y = Column(rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 7, n), "float")
        key = Column(rng.integers(0, 5, n).astype(np.int64), "signed")
        specs = [("sum", x.spec()), ("sum_product", x.spec(), y.spec())]
        first = run_and_check(ctx, [key], [("sum", x), ("sum_product", x, y)], n, what="mixed magnitudes")
        for _ in range(2):
            again = da.group_aggregate_vectors(ctx, [key.spec()], specs, n, detail=True)
            bits = lambda result: [(k, [(None if v is None else _bits(v), c) for v, c in vals]) for k, vals in result]
            assert bits(again) == bits(first)


def test_a_selection_index_outside_its_window_is_an_error_and_the_context_goes_on(ctx):
    alloc, nrows = 2 * W, 3000
    rng = np.random.default_rng(17)
    key = Column(rng.integers(0, 3, alloc).astype(np.int32), "signed")
    a = Column(rng.integers(-100, 100, alloc), "signed")
    good = Selection([[5, 6, 7], [0, 951]])
    run_and_check(ctx, [key], [("sum", a), ("count_star",)], nrows, good, what="good selection")
    bad = Selection([[5, 6, 7], [0, 1452]])          # row 2048 + 1452 = 3500: inside the allocation, not a row of the 3000
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [key.spec()], [("sum", a.spec())], nrows, *bad.ptrs)
    assert e.value.code == _ffi.MI_EINVAL and "selection index" in str(e.value)
    past = Selection([[W], [0]])
    with pytest.raises(da.MiError):                   # 2048 is no row of a full window either
        da.group_aggregate_vectors(ctx, [key.spec()], [("sum", a.spec())], nrows, *past.ptrs)
    run_and_check(ctx, [key], [("sum", a), ("count_star",)], nrows, good, what="after the refusal")
    # both counts say 3000: window 0 is clamped to 2048, window 1 to its 952 rows
    identity = Selection([list(range(W)), list(range(W))])
    identity._cnt = _dev(np.array([3000, 3000], np.uint32))
    got = da.group_aggregate_vectors(ctx, [key.spec()], [("sum", a.spec()), ("count_star",)], nrows, identity._sel.data_ptr(), identity._cnt.data_ptr())
    assert got == da.group_aggregate_vectors(ctx, [key.spec()], [("sum", a.spec()), ("count_star",)], nrows) and sum(g[1][1] for g in got) == nrows


def test_refusals_of_the_kernel_level_entry(ctx):
    c = Column(np.arange(10, dtype=np.int32), "signed")
    f = Column(np.arange(10, dtype=np.float64), "float")
    for keys, specs in (([(c.ptr, 0, 3, "signed")], [("count_star",)]), ([(c.ptr, 0, 4, "wide")], [("count_star",)]), ([(c.ptr, 0, 8, "string")], [("count_star",)]),
                        ([(0, 0, 4, "signed")], [("count_star",)]), ([c.spec()], [("sum_product", c.spec(), f.spec())])):
        with pytest.raises(da.MiError) as e:
            da.group_aggregate_vectors(ctx, keys, specs, 3)
        assert e.value.code == _ffi.MI_EINVAL
    before = da.group_aggregate_counters()
    assert da.group_aggregate_vectors(ctx, [c.spec()], [("count_star",), ("sum", c.spec())], 3) == [((0,), [1, 0]), ((1,), [1, 1]), ((2,), [1, 2])]
    after = da.group_aggregate_counters()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1

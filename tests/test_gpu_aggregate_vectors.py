"""K9 at the kernel level (mi_aggregate_vectors): agg_windows + agg_combine over resident vectors, with and without validity
words, with selection vectors built by hand -- counts and positions no filter would produce on a small table -- against
Python integers, math.fsum and DuckDB's float order written out here.  Expected values never come from the library.

Float sums are compared with math.fsum (the correctly rounded sum) under the bound that holds for ANY summation order of n
doubles (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: |err| <= (n - 1) u sum|x_i| + O(u^2), u = 2^-53),
rounded up to 2 n 2^-53 sum|x_i|: derived, not measured.  Everything else is exact."""
import math
import struct

import numpy as np
import pytest
import torch

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

W = 2048
NMAX = 2 * W + 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAN, INF = float("nan"), float("inf")
CANONICAL_NAN = 0x7FF8000000000000
INT_TYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _words(ok):
    """bool per row -> validity words (uint64, bit r & 63 of word r >> 6), padded with one spare word"""
    bits = np.zeros((len(ok) + 63) // 64 * 64 + 64, np.uint8)
    bits[: len(ok)] = ok
    return np.packbits(bits, bitorder="little").view(np.uint64)


class Column:
    """values (numpy, or Python ints for the 16-byte class), which rows are valid, and the copies in HBM"""

    def __init__(self, values, cls, ok=None, offset=0):
        if cls == "wide":
            self.py = [int(v) for v in values]
            raw = np.array([[v & ((1 << 64) - 1), (v >> 64) & ((1 << 64) - 1)] for v in self.py], np.uint64).reshape(-1, 2)
            self.width = 16
        else:
            values = np.asarray(values)
            self.py = [float(v) for v in values] if cls == "float" else [int(v) for v in values]
            raw = values
            self.width = values.dtype.itemsize
        self.cls = cls
        self.ok = np.ones(len(self.py), bool) if ok is None else np.asarray(ok, bool)
        payload = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        self._data = _dev(np.concatenate([np.zeros(offset, np.uint8), payload]))   # offset: a start that is 8 but not 0 mod 16
        self.ptr = self._data.data_ptr() + offset
        self._valid = None if ok is None else _dev(_words(self.ok))

    def spec(self):
        return (self.ptr, 0 if self._valid is None else self._valid.data_ptr(), self.width, self.cls)


def _wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _float_key(x):
    """DuckDB's total order: NaN greatest, -0.0 = +0.0"""
    return (1, 0.0) if math.isnan(x) else (0, x + 0.0)


def expected(op, cols, rows):
    """-> (kind, value, contributing rows); kind: 'exact' (ints, None, float bits) or 'sum' (the doubles that were summed)"""
    if op == "count_star":
        return "exact", len(rows), len(rows)
    rows = [r for r in rows if all(c.ok[r] for c in cols)]
    a = cols[0]
    if op == "count":
        return "exact", len(rows), len(rows)
    vals = [a.py[r] for r in rows]
    if op == "sum_product":
        vals = [x * cols[1].py[r] for x, r in zip(vals, rows)]      # float * float rounds once, as the kernel's product does
    if not rows:
        return "exact", None, 0
    if a.cls == "float":
        if op in ("sum", "sum_product"):
            return "sum", vals, len(rows)
        best = (min if op == "min" else max)(vals, key=_float_key)
        return "exact", NAN if math.isnan(best) else best + 0.0, len(rows)
    if op in ("sum", "sum_product"):
        return "exact", _wrap128(sum(vals)), len(rows)
    return "exact", (min if op == "min" else max)(vals), len(rows)


def check(got, want, what):
    kind, value, count = want
    got_value, got_count = got
    assert got_count == count, (what, got, want[1:] if kind == "exact" else count)
    if kind == "sum":
        if any(math.isnan(v) for v in value) or (INF in value and -INF in value):
            assert math.isnan(got_value), (what, got_value)
        elif INF in value or -INF in value:
            assert got_value == (INF if INF in value else -INF), (what, got_value)
        else:
            exact = math.fsum(value)
            bound = 2 * len(value) * 2.0 ** -53 * math.fsum(abs(v) for v in value)
            print("%s: got %r, fsum %r, |err| %.3g, bound %.3g" % (what, got_value, exact, abs(got_value - exact), bound))
            assert abs(got_value - exact) <= bound, (what, got_value, exact, bound)
    elif isinstance(value, float):
        assert isinstance(got_value, float), (what, got_value)
        assert _bits(got_value) == (CANONICAL_NAN if math.isnan(value) else _bits(value)), (what, got_value, value)
    else:
        assert got_value == value and (value is None or isinstance(got_value, int)), (what, got_value, value)


class Selection:
    """per-window row lists -> sel / sel_count in the filter's layout"""

    def __init__(self, per_window, slots=None):
        self.per_window = per_window
        n_windows = len(per_window)
        sel = np.full(slots if slots is not None else n_windows * W, 0xFFFFFFFF, np.uint32)   # slots never read hold a poison index
        for w, rows in enumerate(per_window):
            sel[w * W: w * W + len(rows)] = rows
        self._sel, self._cnt = _dev(sel), _dev(np.array([len(r) for r in per_window], np.uint32))
        self.ptrs = (self._sel.data_ptr(), self._cnt.data_ptr())

    def rows(self):
        return [w * W + r for w, rows in enumerate(self.per_window) for r in rows]


def run_and_check(ctx, aggs, nrows, selection=None, what=""):
    """aggs: [(op, Column...)]; at most 8 per call"""
    rows = selection.rows() if selection is not None else list(range(nrows))
    for first in range(0, len(aggs), 8):
        part = aggs[first: first + 8]
        specs = [(op,) + tuple(c.spec() for c in cols) for op, *cols in part]
        sel_ptr, cnt_ptr = selection.ptrs if selection is not None else (0, 0)
        got = da.aggregate_vectors(ctx, specs, nrows, sel_ptr, cnt_ptr, detail=True)
        assert len(got) == len(part)
        for (op, *cols), g in zip(part, got):
            check(g, expected(op, cols, rows), "%s %s(%s) n=%d" % (what, op, ",".join("%s%d" % (c.cls, c.width) for c in cols), nrows))


@pytest.fixture(scope="module")
def table():
    """one column of every value class, NMAX rows, without and with validity (about 15 % NULL)"""
    rng = np.random.default_rng(2024)
    out = {}
    for with_nulls in (False, True):
        cols = {}
        ok = lambda: (rng.random(NMAX) >= 0.15) if with_nulls else None
        for name, t in INT_TYPES.items():
            info = np.iinfo(t)
            v = rng.integers(info.min, info.max, NMAX, dtype=t, endpoint=True)
            v[:4] = [info.min, info.max, 0, info.max]
            cols[name] = Column(v, "unsigned" if name[0] == "u" else "signed", ok())
        cols["f32"] = Column((rng.normal(0, 1e3, NMAX)).astype(np.float32), "float", ok())
        cols["f64"] = Column(rng.normal(0, 1e6, NMAX) * rng.choice([1e-9, 1.0, 1e9], NMAX), "float", ok())
        wide = [int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 65)) for _ in range(NMAX)]
        wide = [(-v - 1 if rng.random() < 0.5 else v) for v in wide]
        wide[:4] = [-(1 << 127), (1 << 127) - 1, (1 << 64) + 3, -(1 << 64) - 3]
        cols["wide"] = Column(wide, "wide", ok())
        out[with_nulls] = cols
    return out


def _all_aggregates(cols):
    aggs = [("count_star",)]
    for name, c in cols.items():
        aggs += [("count", c), ("min", c), ("max", c)]
        if c.cls != "wide":
            aggs.append(("sum", c))
    aggs += [("sum_product", cols["i64"], cols["i32"]), ("sum_product", cols["u64"], cols["i8"]), ("sum_product", cols["u32"], cols["u64"]),
             ("sum_product", cols["i16"], cols["i16"]), ("sum_product", cols["f32"], cols["f64"]), ("sum_product", cols["f32"], cols["f32"]),
             ("sum_product", cols["f64"], cols["f64"])]
    return aggs


@pytest.mark.parametrize("nrows", [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096 + 5])
def test_row_count_seams(ctx, table, nrows):
    for with_nulls in (False, True):
        run_and_check(ctx, _all_aggregates(table[with_nulls]), nrows, what="nulls" if with_nulls else "dense")


def _few(cols):
    return [("count_star",), ("count", cols["wide"]), ("sum", cols["i64"]), ("sum", cols["f64"]), ("min", cols["wide"]), ("max", cols["f32"]),
            ("sum_product", cols["i32"], cols["u64"]), ("min", cols["u16"])]


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048])
def test_selection_count_seams(ctx, table, count):
    rng = np.random.default_rng(count)
    picks = [sorted(rng.choice(W, count, replace=False).tolist())]
    if count == 1:
        picks = [[0], [W - 1]]          # the first row only; the last row only
    for rows in picks:
        for with_nulls in (False, True):
            run_and_check(ctx, _few(table[with_nulls]), W, Selection([rows]), what="count %d" % count)


def test_selection_three_windows_empty_middle_ragged_last(ctx, table):
    rng = np.random.default_rng(5)
    nrows = 2 * W + 5
    sels = [[sorted(rng.choice(W, 700, replace=False).tolist()), [], [0, 2, 4]],
            [list(range(W)), [], list(range(5))],
            [[W - 1], [], [4]],
            [list(range(W - 1, -1, -1)), [], [4, 3, 3, 0]]]          # descending, a row twice: any index inside the window is a row
    for per_window in sels:
        for with_nulls in (False, True):
            run_and_check(ctx, _few(table[with_nulls]), nrows, Selection(per_window), what="three windows")


def test_all_null_column_and_one_valid_row_at_wave_boundaries(ctx):
    n = W + 300
    rng = np.random.default_rng(9)
    i64 = rng.integers(-1000, 1000, n)
    f64 = rng.normal(0, 1, n)
    wide = [int(v) << 70 for v in i64]
    partner = Column(rng.integers(-5, 5, n).astype(np.int32), "signed")
    for valid_rows in ([], [0], [63], [64], [127], [128], [191], [192], [255], [256], [W - 1], [W], [n - 1]):
        ok = np.zeros(n, bool)
        ok[valid_rows] = True
        a, f, w = Column(i64, "signed", ok), Column(f64, "float", ok), Column(wide, "wide", ok)
        aggs = [("count_star",), ("count", a), ("sum", a), ("min", a), ("max", a), ("sum", f), ("min", f), ("max", f),
                ("count", w), ("min", w), ("max", w), ("sum_product", a, partner), ("sum_product", partner, a)]
        rows = list(range(n))
        for first in range(0, len(aggs), 8):
            part = aggs[first: first + 8]
            got = da.aggregate_vectors(ctx, [(op,) + tuple(c.spec() for c in cols) for op, *cols in part], n, detail=True)
            for (op, *cols), g in zip(part, got):
                check(g, expected(op, cols, rows), "valid rows %s: %s" % (valid_rows, op))
                if not valid_rows and op not in ("count_star",):
                    assert g == ((0, 0) if op == "count" else (None, 0)), (op, g)      # SUM / MIN / MAX are NULL, COUNT is 0


def test_exact_sums_at_the_ends_of_int64(ctx):
    n = 5000
    top, bottom = Column(np.full(n, I64_MAX, np.int64), "signed"), Column(np.full(n, I64_MIN, np.int64), "signed")
    got = da.aggregate_vectors(ctx, [("sum", top.spec()), ("sum", bottom.spec()), ("sum_product", top.spec(), bottom.spec())], n)
    assert got == [5000 * I64_MAX, 5000 * I64_MIN, _wrap128(5000 * I64_MAX * I64_MIN)]      # the last one wraps modulo 2^128
    a = np.array([I64_MIN, -3, 7, -(1 << 40), I64_MAX, -1], np.int64)
    b = np.array([I64_MIN, 5, -9, (1 << 22), 3, I64_MAX], np.int64)
    want = sum(int(x) * int(y) for x, y in zip(a, b))
    assert want > (1 << 125)
    ca, cb = Column(a, "signed"), Column(b, "signed")      # (named: a column's device memory lives as long as the object)
    assert da.aggregate_vectors(ctx, [("sum_product", ca.spec(), cb.spec())], len(a)) == [want]
    rng = np.random.default_rng(3)
    u = rng.integers(1 << 63, (1 << 64) - 1, 4101, dtype=np.uint64, endpoint=True)
    u[:2] = [(1 << 64) - 1, 1 << 63]
    cu = Column(u, "unsigned")
    want_sum = sum(int(x) for x in u)
    got = da.aggregate_vectors(ctx, [("sum", cu.spec()), ("min", cu.spec()), ("max", cu.spec()), ("sum_product", cu.spec(), cu.spec())], len(u))
    assert got == [want_sum, int(u.min()), (1 << 64) - 1, _wrap128(sum(int(x) * int(x) for x in u))] and want_sum > (1 << 74)


@pytest.mark.parametrize("where", [0, 63, 2047, 2 * 2048 + 4])
def test_the_row_that_carries_the_extreme(ctx, where):
    """lane 0, lane 63, row 2047, and the last row of a ragged last window"""
    n = 2 * W + 5
    for lowest in (True, False):
        i = np.full(n, 10, np.int64)
        f = np.full(n, 10.0)
        wide = [10 << 64] * n
        i[where] = I64_MIN if lowest else I64_MAX
        f[where] = -1e300 if lowest else 1e300
        wide[where] = -(1 << 127) if lowest else (1 << 127) - 1
        op = "min" if lowest else "max"
        ci, cf, cw = Column(i, "signed"), Column(f, "float"), Column(wide, "wide")
        got = da.aggregate_vectors(ctx, [(op, ci.spec()), (op, cf.spec()), (op, cw.spec())], n)
        assert got == [int(i[where]), float(f[where]), wide[where]]


def test_floats_nan_zero_and_infinity(ctx):
    def agg(values, dtype=np.float64, ok=None):
        c = Column(np.array(values, dtype), "float", ok)
        return da.aggregate_vectors(ctx, [("sum", c.spec()), ("min", c.spec()), ("max", c.spec()), ("count", c.spec())], len(values))

    for dtype in (np.float64, np.float32):
        s, mn, mx, n = agg([NAN], dtype)                                   # NaN alone
        assert math.isnan(s) and _bits(mn) == CANONICAL_NAN and _bits(mx) == CANONICAL_NAN and n == 1
        s, mn, mx, n = agg([1.5, -NAN, -2.0, 7.25] * 300, dtype)          # NaN among numbers: MAX is NaN, MIN ignores it
        assert math.isnan(s) and mn == -2.0 and _bits(mx) == CANONICAL_NAN and n == 1200
        s, mn, mx, n = agg([NAN, -NAN] * 200, dtype)                       # all NaN: MIN is NaN too, the canonical one
        assert math.isnan(s) and _bits(mn) == CANONICAL_NAN and _bits(mx) == CANONICAL_NAN
        s, mn, mx, n = agg([-0.0, 0.0, -0.0], dtype)                       # -0.0 = +0.0, returned as +0.0
        assert _bits(mn) == 0 and _bits(mx) == 0 and s == 0.0
        s, mn, mx, n = agg([-0.0] * 70, dtype)
        assert _bits(mn) == 0 and _bits(mx) == 0 and s == 0.0
        s, mn, mx, n = agg([INF, 1.0, -INF] * 100, dtype)                  # the sum of both infinities is NaN
        assert math.isnan(s) and mn == -INF and mx == INF
        s, mn, mx, n = agg([INF, 1.0, 3.0] * 100, dtype)
        assert s == INF and mn == 1.0 and mx == INF
        s, mn, mx, n = agg([NAN, 4.0, NAN], dtype, ok=[False, True, False])   # a NULL NaN is no NaN
        assert s == 4.0 and mn == 4.0 and mx == 4.0 and n == 1
    bits = np.array([0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000], np.uint64).view(np.float64)   # signalling, negative, quiet
    s, mn, mx, n = agg(list(bits))
    assert _bits(mn) == CANONICAL_NAN and _bits(mx) == CANONICAL_NAN


def test_double_sum_of_mixed_sign_within_the_bound_of_any_order_and_bit_reproducible(ctx):
    rng = np.random.default_rng(11)
    for n in (257, 2048, 2 * W + 5, 20000):
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-12, 13, n)
        c = Column(x, "float", rng.random(n) > 0.1)
        rows = list(range(n))
        first = da.aggregate_vectors(ctx, [("sum", c.spec())], n, detail=True)[0]
        check(first, expected("sum", [c], rows), "mixed-sign doubles")
        again = da.aggregate_vectors(ctx, [("sum", c.spec())], n, detail=True)[0]
        assert _bits(first[0]) == _bits(again[0]) and first[1] == again[1]


def test_16_byte_column_at_8_mod_16(ctx):
    rng = np.random.default_rng(13)
    n = W + 77
    values = [(int(rng.integers(-(1 << 62), 1 << 62)) << 60) + int(rng.integers(0, 1 << 60)) for _ in range(n)]
    c = Column(values, "wide", rng.random(n) > 0.2, offset=8)
    assert c.ptr % 16 == 8
    run_and_check(ctx, [("min", c), ("max", c), ("count", c)], n, what="8 mod 16")


def test_a_selection_index_outside_its_window_is_an_error_and_a_count_past_the_rows_is_clamped(ctx):
    alloc, nrows = 2 * W, 3000
    rng = np.random.default_rng(17)
    a = Column(rng.integers(-100, 100, alloc), "signed")
    f = Column(rng.normal(0, 1, alloc), "float")
    specs = [("sum", a.spec()), ("count_star",), ("min", f.spec())]
    good = Selection([[5, 6, 7], [0, 951]])
    assert da.aggregate_vectors(ctx, specs, nrows, *good.ptrs)[:2] == [sum(a.py[r] for r in good.rows()), 5]
    bad = Selection([[5, 6, 7], [0, 1452]])          # row 2048 + 1452 = 3500: inside the allocation, not a row of the 3000
    with pytest.raises(da.MiError) as e:
        da.aggregate_vectors(ctx, specs, nrows, *bad.ptrs)
    assert e.value.code == _ffi.MI_EINVAL and "selection index" in str(e.value)
    past = Selection([[W], [0]])
    with pytest.raises(da.MiError):                   # 2048 is no row of a full window either
        da.aggregate_vectors(ctx, specs, nrows, *past.ptrs)
    # every slot names its own row; both counts say 3000: window 0 is clamped to 2048, window 1 to its 952 rows
    identity = Selection([list(range(W)), list(range(W))])
    identity._cnt = _dev(np.array([3000, 3000], np.uint32))
    got = da.aggregate_vectors(ctx, specs, nrows, identity._sel.data_ptr(), identity._cnt.data_ptr())
    assert got[:2] == [sum(a.py[:nrows]), nrows] and got[2] == min(f.py[:nrows])
    assert got == da.aggregate_vectors(ctx, specs, nrows)


def test_refusals_of_the_kernel_level_entry(ctx):
    c = Column(np.arange(10, dtype=np.int32), "signed")
    w = Column([1, 2, 3], "wide")
    f = Column(np.arange(10, dtype=np.float64), "float")
    for specs in ([("sum", w.spec())], [("sum_product", c.spec(), f.spec())], [("sum", (c.ptr, 0, 3, "signed"))], [("min", (c.ptr, 0, 4, "any"))],
                  [("sum", (c.ptr, 0, 2, "float"))], [("max", (0, 0, 4, "signed"))]):
        with pytest.raises(da.MiError) as e:
            da.aggregate_vectors(ctx, specs, 3)
        assert e.value.code == _ffi.MI_EINVAL
    assert da.aggregate_vectors(ctx, [("count_star",), ("sum", c.spec())], 0) == [0, None]      # no rows at all

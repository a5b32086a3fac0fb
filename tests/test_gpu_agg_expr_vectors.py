"""MI_AGG_SUM_EXPR at the kernel level (mi_aggregate_vectors, mi_group_aggregate_vectors): the expression fold of agg_windows
and group_windows over hand-built vectors -- every width and signedness mixed inside one expression, the same column
twice, constant factors, constants at the ends of int64, products and sums that wrap modulo 2^128, NULLs over garbage
bytes, selection vectors -- against tests/agg_expr_cases.py (Python ints modulo 2^128, Fractions), which
tests/test_agg_expr_host.py holds to pyarrow.  Expected values never come from the library.

Integer results are exact.  Double results are within 2 (n + 3 F) 2^-53 sum|term| of the exact sum of the exact terms (the
derivation is in agg_expr_cases.py) and bit-identical between two runs.  SUM_EXPR[a] and SUM(a), SUM_EXPR[a, b] and
SUM_PRODUCT(a, b) are compared as bits."""
import math
import struct

import numpy as np
import pytest
import torch

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import agg_expr_cases as ec

pytestmark = pytest.mark.gpu

W = ec.W
I64_MIN, I64_MAX = ec.I64_MIN, ec.I64_MAX
NMAX = 2 * W + 5
NROWS = [1, 63, 64, 65, 2047, 2048, 2049, 4096 + 5]


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _words(ok):
    bits = np.zeros((len(ok) + 63) // 64 * 64 + 64, np.uint8)
    bits[: len(ok)] = ok
    return np.packbits(bits, bitorder="little").view(np.uint64)


class Column:
    """numpy values, which rows are valid, and the copies in HBM"""

    def __init__(self, values, ok=None, cls=None):
        values = np.asarray(values)
        self.cls = cls or ("float" if values.dtype.kind == "f" else "unsigned" if values.dtype.kind == "u" else "signed")
        self.py = [float(v) for v in values] if self.cls == "float" else [int(v) for v in values]
        self.width = values.dtype.itemsize
        self.ok = None if ok is None else np.asarray(ok, bool)
        self._data = _dev(values)
        self._valid = None if ok is None else _dev(_words(self.ok))

    def spec(self):
        return (self._data.data_ptr(), 0 if self._valid is None else self._valid.data_ptr(), self.width, self.cls)


class Selection:
    """per-window row lists -> sel / sel_count in the filter's layout"""

    def __init__(self, per_window, slots=None):
        self.per_window = per_window
        sel = np.full(slots if slots is not None else len(per_window) * W, 0xFFFFFFFF, np.uint32)   # slots never read hold a poison index
        for w, rows in enumerate(per_window):
            sel[w * W: w * W + len(rows)] = rows
        self._sel, self._cnt = _dev(sel), _dev(np.array([len(r) for r in per_window], np.uint32))
        self.ptrs = (self._sel.data_ptr(), self._cnt.data_ptr())

    def rows(self):
        return [w * W + r for w, rows in enumerate(self.per_window) for r in rows]


def build(cols, expr):
    """expr: a list of factors -- a column name, (name, mul, add), or a number -> (the library's spec, the reference's Factors)"""
    spec, factors = ["sum_expr"], []
    for f in expr:
        if isinstance(f, str):
            f = (f, 1, 0)
        if isinstance(f, tuple):
            c = cols[f[0]]
            spec.append((c.spec(), f[1], f[2]))
            factors.append(ec.Factor(c.py, c.ok, f[1], f[2]))
        else:
            spec.append(f)
            factors.append(ec.Factor(None, None, 1, f))
    return tuple(spec), factors


INT_EXPRS = [
    ["i64"],                                                        # F = 1
    ["u8", ("i16", -1, 100)],                                       # F = 2, widths 1 and 2, unsigned and signed
    ["i32", ("u16", -1, 100), ("u32", 1, 100)],                     # F = 3: the shape of Q1's sum_charge
    ["i8", "u64", ("i16", 0, 7), "i64"],                            # F = 4, all four widths, a mul of 0
    ["i32", "i32"],                                                 # the same column twice: sum(x * x)
    ["u64", 3, ("i8", -1, I64_MIN)],                                # a constant factor; add = INT64_MIN
    ["i64", "i64", "u64", ("i64", -1, I64_MIN)],                    # the true product of four 64-bit factors is far past 2^128
    ["top", "top"],                                                 # 2^126 a row: the product fits, the sum wraps from two rows on
]
FLOAT_EXPRS = [
    ["f64"],
    ["f32", "f64"],
    ["f64", ("g64", -1.0, 1.0), ("f32", 1.0, 1.0)],
    ["f32", "g64", 0.5, ("f64", 2.0, -3.0)],
    ["g64", "g64"],
    [("f64", 3, 1), ("f32", 0, -2)],                                # integer constants are converted; a mul of 0
]


@pytest.fixture(scope="module")
def tables():
    """with_nulls -> name -> Column, NMAX rows: every integer type, the extremes in the first rows; three float columns.  The
    bytes under a NULL are whatever was drawn, the extremes included, and NaN in the float columns"""
    out = {}
    for with_nulls in (False, True):
        cols = {}
        for name, (v, ok) in ec.int_columns(NMAX, 31, with_nulls).items():
            cols[name] = Column(v, ok)
        cols["top"] = Column(np.full(NMAX, I64_MAX, np.int64), None)
        for name, (v, ok) in ec.float_columns(NMAX, 32, with_nulls).items():
            if ok is not None:
                v = v.copy()
                v[~ok] = np.nan      # garbage under a NULL: it must not reach the sum
            cols[name] = Column(v, ok)
        out[with_nulls] = cols
    return out


def run_ints(ctx, cols, nrows, selection=None, what=""):
    rows = selection.rows() if selection is not None else list(range(nrows))
    built = [build(cols, e) for e in INT_EXPRS]
    got = da.aggregate_vectors(ctx, [b[0] for b in built], nrows, *(selection.ptrs if selection is not None else (0, 0)), detail=True)
    for e, (_, factors), g in zip(INT_EXPRS, built, got):
        assert g == ec.sum_expr_int(factors, rows), (what, nrows, e, g)
    return got


def run_floats(ctx, cols, nrows, selection=None, what=""):
    rows = selection.rows() if selection is not None else list(range(nrows))
    built = [build(cols, e) for e in FLOAT_EXPRS]
    ptrs = selection.ptrs if selection is not None else (0, 0)
    got = da.aggregate_vectors(ctx, [b[0] for b in built], nrows, *ptrs, detail=True)
    for e, (_, factors), g in zip(FLOAT_EXPRS, built, got):
        ec.check_float(g, factors, rows, "%s n=%d %s" % (what, nrows, e))
    again = da.aggregate_vectors(ctx, [b[0] for b in built], nrows, *ptrs, detail=True)
    assert [(None if v is None else ec.bits(v), c) for v, c in got] == [(None if v is None else ec.bits(v), c) for v, c in again], what
    return got


@pytest.mark.parametrize("nrows", NROWS)
def test_integer_expressions_at_the_row_count_seams(ctx, tables, nrows):
    for with_nulls in (False, True):
        got = run_ints(ctx, tables[with_nulls], nrows, what="nulls" if with_nulls else "dense")
    # what the cases are there for: the product of four factors left 128 bits, and the sum of 2^126 a row wrapped
    cols = tables[False]
    if nrows >= 2:
        assert sum(I64_MAX * I64_MAX for _ in range(nrows)) >= 1 << 127 and got[7][0] == ec.wrap128(nrows * I64_MAX * I64_MAX)
        i, u = cols["i64"].py[1], cols["u64"].py[1]      # row 1 holds the types' maxima
        assert abs(i * i * u * (I64_MIN - i)) >= 1 << 128


@pytest.mark.parametrize("nrows", NROWS)
def test_float_expressions_at_the_row_count_seams(ctx, tables, nrows):
    for with_nulls in (False, True):
        run_floats(ctx, tables[with_nulls], nrows, what="nulls" if with_nulls else "dense")


def test_nulls_in_the_first_the_last_and_every_factor_column_over_garbage(ctx):
    n = W + 300
    rng = np.random.default_rng(41)
    a, b, c = (rng.integers(-1000, 1000, n).astype(t) for t in (np.int64, np.int16, np.uint32))
    x, y = rng.normal(0, 1, n), rng.normal(0, 1, n).astype(np.float32)
    masks = {"none": None, "some": rng.random(n) >= 0.3, "other": rng.random(n) >= 0.3, "all null": np.zeros(n, bool),
             "row 0 only": np.arange(n) == 0, "last row only": np.arange(n) == n - 1, "row 2047 and 2048": (np.arange(n) == W - 1) | (np.arange(n) == W)}

    def garbage(v, ok, worst):
        v = v.copy()
        if ok is not None:
            v[~ok] = worst
        return v

    for ma, mb, mc in (("some", "none", "none"), ("none", "none", "some"), ("some", "other", "some"), ("all null", "none", "none"),
                       ("none", "none", "all null"), ("row 0 only", "none", "none"), ("none", "last row only", "none"),
                       ("row 2047 and 2048", "some", "none")):
        cols = {"a": Column(garbage(a, masks[ma], I64_MIN), masks[ma]), "b": Column(garbage(b, masks[mb], -32768), masks[mb]),
                "c": Column(garbage(c, masks[mc], 0xFFFFFFFF), masks[mc]),
                "x": Column(garbage(x, masks[ma], np.nan), masks[ma]), "y": Column(garbage(y, masks[mc], np.inf), masks[mc])}
        rows = list(range(n))
        exprs = [["a", ("b", -1, 100), ("c", 1, 100)], ["c", "a"], ["b"], [("a", 1, 0), 5, "c", "b"]]
        built = [build(cols, e) for e in exprs]
        fbuilt = [build(cols, e) for e in (["x", ("y", -1.0, 1.0)], ["y", "x", "x"])]
        got = da.aggregate_vectors(ctx, [s for s, _ in built + fbuilt], n, detail=True)
        for e, (_, factors), g in zip(exprs, built, got):
            assert g == ec.sum_expr_int(factors, rows), ((ma, mb, mc), e, g)
        for (_, factors), g in zip(fbuilt, got[len(built):]):
            ec.check_float(g, factors, rows, "nulls %s" % ((ma, mb, mc),))
        if ma == "all null":
            assert got[0] == (None, 0) and got[1] == (None, 0) and got[4] == (None, 0)      # count == 0 is NULL
            assert got[2][1] == n                                                           # `b` alone is not touched by a's NULLs


def test_selection_vectors_with_an_empty_window_between_full_ones(ctx, tables):
    rng = np.random.default_rng(43)
    nrows = 2 * W + 5
    sels = [[sorted(rng.choice(W, 700, replace=False).tolist()), [], [0, 2, 4]],
            [list(range(W)), [], list(range(5))],
            [[W - 1], [], [4]],
            [list(range(W - 1, -1, -1)), [], [4, 3, 3, 0]]]          # descending, a row twice: any index inside the window is a row
    for per_window in sels:
        for with_nulls in (False, True):
            run_ints(ctx, tables[with_nulls], nrows, Selection(per_window), what="three windows")
            run_floats(ctx, tables[with_nulls], nrows, Selection(per_window), what="three windows")
    for count in (0, 1, 63, 64, 65, 2048):
        picks = sorted(rng.choice(W, count, replace=False).tolist())
        run_ints(ctx, tables[True], W, Selection([picks]), what="count %d" % count)
        run_floats(ctx, tables[True], W, Selection([picks]), what="count %d" % count)


def test_a_selection_index_outside_its_window_fails_the_call(ctx):
    """the construction of test_gpu_aggregate_vectors.py: row 2048 + 1452 = 3500 lies inside the 4096-row allocation and is no
    row of the 3000; the index is skipped, never used as an address, and the call fails"""
    alloc, nrows = 2 * W, 3000
    rng = np.random.default_rng(17)
    cols = {"a": Column(rng.integers(-100, 100, alloc)), "b": Column(rng.integers(0, 10, alloc).astype(np.uint8)), "f": Column(rng.normal(0, 1, alloc))}
    built = [build(cols, ["a", ("b", -1, 100)]), build(cols, ["f", "f"])]
    specs = [s for s, _ in built]
    good = Selection([[5, 6, 7], [0, 951]])
    got = da.aggregate_vectors(ctx, specs, nrows, *good.ptrs, detail=True)
    assert got[0] == ec.sum_expr_int(built[0][1], good.rows())
    bad = Selection([[5, 6, 7], [0, 1452]])
    for call in (lambda: da.aggregate_vectors(ctx, specs, nrows, *bad.ptrs),
                 lambda: da.group_aggregate_vectors(ctx, [cols["b"].spec()[:3] + ("unsigned",)], specs, nrows, *bad.ptrs)):
        with pytest.raises(da.MiError) as e:
            call()
        assert e.value.code == _ffi.MI_EINVAL and "selection index" in str(e.value)
    # a count past the rows is clamped: both counts say 3000, window 1 has 952 rows
    identity = Selection([list(range(W)), list(range(W))])
    identity._cnt = _dev(np.array([3000, 3000], np.uint32))
    assert da.aggregate_vectors(ctx, specs, nrows, identity._sel.data_ptr(), identity._cnt.data_ptr()) == da.aggregate_vectors(ctx, specs, nrows)


# ---- grouped
def run_grouped(ctx, cols, key, nrows, selection=None, what=""):
    rows = selection.rows() if selection is not None else list(range(nrows))
    ptrs = selection.ptrs if selection is not None else (0, 0)
    groups = {}
    for r in rows:
        groups.setdefault(key.py[r], []).append(r)
    kspec = [key.spec()]
    ibuilt, fbuilt = [build(cols, e) for e in INT_EXPRS[:5]], [build(cols, e) for e in FLOAT_EXPRS[:3]]
    got = da.group_aggregate_vectors(ctx, kspec, [s for s, _ in ibuilt + fbuilt], nrows, *ptrs, detail=True)
    assert [k for (k,), _ in got] == sorted(groups), what
    for (k,), values in got:
        for (_, factors), g in zip(ibuilt, values):
            assert g == ec.sum_expr_int(factors, groups[k]), (what, k, g)
        for (_, factors), g in zip(fbuilt, values[len(ibuilt):]):
            ec.check_float(g, factors, groups[k], "%s group %s" % (what, k))
    again = da.group_aggregate_vectors(ctx, kspec, [s for s, _ in ibuilt + fbuilt], nrows, *ptrs, detail=True)
    flat = lambda res: [(k, [(ec.bits(v) if isinstance(v, float) else v, c) for v, c in vals]) for k, vals in res]
    assert flat(got) == flat(again), what
    return got


def test_grouped_one_group_256_groups_in_a_window_and_a_group_that_spans_windows(ctx, tables):
    rng = np.random.default_rng(47)
    for with_nulls in (False, True):
        cols = tables[with_nulls]
        for nrows in (1, 65, 2049, NMAX):
            run_grouped(ctx, cols, Column(np.zeros(NMAX, np.int32)), nrows, what="one group")                          # spans every window
        run_grouped(ctx, cols, Column((np.arange(NMAX) % 256).astype(np.uint8)), NMAX, what="256 groups in every window")
        run_grouped(ctx, cols, Column(rng.integers(-3, 4, NMAX).astype(np.int64)), NMAX, what="seven groups, each in every window")
        few = Column((np.arange(NMAX) // 1500).astype(np.int16))                                                            # group 1 spans windows 0 and 1
        run_grouped(ctx, cols, few, NMAX, what="runs of 1500 rows")
        sel = Selection([sorted(rng.choice(W, 900, replace=False).tolist()), [], [0, 1, 4]])
        run_grouped(ctx, cols, few, NMAX, sel, what="runs of 1500 rows, selected")


# ---- the two equivalences, as bits
def _same_bits(x, y):
    (a, ca), (b, cb) = x, y
    if isinstance(a, float) or isinstance(b, float):
        return ca == cb and isinstance(a, float) and isinstance(b, float) and ec.bits(a) == ec.bits(b)
    return x == y


def test_sum_expr_of_one_and_two_plain_columns_is_sum_and_sum_product_bit_for_bit(ctx, tables):
    rng = np.random.default_rng(53)
    n = NMAX
    special = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    special[rng.choice(n, 40, replace=False)] = -0.0
    zeros = Column(np.full(n, -0.0), rng.random(n) >= 0.1)                  # a sum of -0.0 alone is -0.0: nothing may add +0.0 to it
    with_nan = special.copy()
    with_nan[[5, 700, 3000]] = [np.nan, np.inf, -np.inf]
    with_inf = special.copy()
    with_inf[[64, 2048]] = np.inf
    nan_payload = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    lone = np.full(n, 1.0)
    lone[0] = nan_payload
    for with_nulls in (False, True):
        cols = dict(tables[with_nulls])
        ok = (lambda: rng.random(n) >= 0.2) if with_nulls else (lambda: None)
        cols.update({"special": Column(special, ok()), "zeros": zeros, "nan": Column(with_nan, ok()), "inf": Column(with_inf, ok()),
                     "lone": Column(lone, None)})
        singles = ["i8", "u16", "i32", "u64", "i64", "f32", "f64", "special", "zeros", "nan", "inf", "lone"]
        pairs = [("i64", "i32"), ("u64", "i8"), ("u32", "u64"), ("i16", "i16"), ("f32", "f64"), ("special", "special"), ("zeros", "f64"), ("nan", "inf"),
                 ("inf", "zeros"), ("g64", "special")]
        key = Column((np.arange(n) // 1500).astype(np.int16))
        sel = Selection([sorted(rng.choice(W, 900, replace=False).tolist()), [], [0, 1, 4]])
        for nrows, selection in ((n, None), (65, None), (1, None), (n, sel)):
            ptrs = selection.ptrs if selection is not None else (0, 0)
            for names in [singles[i: i + 4] for i in range(0, len(singles), 4)]:
                specs = [("sum_expr", cols[c].spec()) for c in names] + [("sum", cols[c].spec()) for c in names]
                got = da.aggregate_vectors(ctx, specs, nrows, *ptrs, detail=True)
                for i, c in enumerate(names):
                    assert _same_bits(got[i], got[i + len(names)]), ("sum", c, nrows, got[i], got[i + len(names)])
                grouped = da.group_aggregate_vectors(ctx, [key.spec()], specs, nrows, *ptrs, detail=True)
                for k, vals in grouped:
                    for i, c in enumerate(names):
                        assert _same_bits(vals[i], vals[i + len(names)]), ("grouped sum", c, k, vals[i], vals[i + len(names)])
            for some in [pairs[i: i + 4] for i in range(0, len(pairs), 4)]:
                specs = [("sum_expr", cols[a].spec(), cols[b].spec()) for a, b in some] + [("sum_product", cols[a].spec(), cols[b].spec()) for a, b in some]
                got = da.aggregate_vectors(ctx, specs, nrows, *ptrs, detail=True)
                for i, c in enumerate(some):
                    assert _same_bits(got[i], got[i + len(some)]), ("sum_product", c, nrows, got[i], got[i + len(some)])
                grouped = da.group_aggregate_vectors(ctx, [key.spec()], specs, nrows, *ptrs, detail=True)
                for k, vals in grouped:
                    for i, c in enumerate(some):
                        assert _same_bits(vals[i], vals[i + len(some)]), ("grouped sum_product", c, k, vals[i], vals[i + len(some)])
        # and the values that make the comparison worth something
        got = da.aggregate_vectors(ctx, [("sum_expr", cols["zeros"].spec()), ("sum_expr", cols["lone"].spec()), ("sum_expr", cols["nan"].spec())], n)
        assert ec.bits(got[0]) == 0x8000000000000000 and math.isnan(got[1]) and math.isnan(got[2])
        assert ec.bits(da.aggregate_vectors(ctx, [("sum_expr", cols["lone"].spec())], 1)[0]) == 0x7FF8000000000123      # one row: its bits


def test_constants_of_a_float_expression_and_the_shortcuts(ctx):
    x = Column(np.array([-0.0, 0.0, -0.0]))
    spec = x.spec()
    got = da.aggregate_vectors(ctx, [("sum_expr", spec), ("sum_expr", (spec, 1.0, 0.0)), ("sum_expr", (spec, 1, 0)), ("sum_expr", (spec, 1.0, -0.0)),
                                     ("sum_expr", (spec, -1.0, 0.0))], 1)
    # one row of -0.0: plain, mul 1.0 / add +0.0 skipped (doubles or converted ints), -0.0 + -0.0, -1.0 * -0.0
    assert [ec.bits(v) for v in got] == [1 << 63, 1 << 63, 1 << 63, 1 << 63, 0]
    y = Column(np.array([1.0 + 2.0 ** -30] * 3))
    fused = da.aggregate_vectors(ctx, [("sum_expr", (y.spec(), 1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -29)))], 3)
    assert fused == [0.0]      # the product is rounded before the addition: an fma would give 3 * 2^-60


def test_refusals_of_the_kernel_level_entries(ctx):
    i = Column(np.arange(10, dtype=np.int32))
    f = Column(np.arange(10, dtype=np.float64))
    wide = (i._data.data_ptr(), 0, 16, "wide")
    key = [i.spec()]
    cases = [([("sum_expr", i.spec(), f.spec())], _ffi.MI_ENOTSUP, "integer-like or both floating point"),
             ([("sum_expr", f.spec(), 2, i.spec())], _ffi.MI_ENOTSUP, "integer-like or both floating point"),
             ([("sum_expr", (i.spec(), 1.0, 0.0))], _ffi.MI_ENOTSUP, "double constants"),
             ([("sum_expr", i.spec(), 2.5)], _ffi.MI_ENOTSUP, "double constants"),
             ([("sum_expr", (f.spec(), (1 << 53) + 1, 0))], _ffi.MI_EINVAL, "not exactly representable"),
             ([("sum_expr", (f.spec(), 1, I64_MAX))], _ffi.MI_EINVAL, "not exactly representable"),
             ([("sum_expr", wide)], _ffi.MI_EINVAL, ""),
             ([("sum_expr", i.spec(), wide)], _ffi.MI_EINVAL, ""),
             ([("sum_expr", (i._data.data_ptr(), 0, 3, "signed"))], _ffi.MI_EINVAL, ""),
             ([("sum_expr", (f._data.data_ptr(), 0, 2, "float"))], _ffi.MI_EINVAL, ""),
             ([("sum_expr", i.spec(), (0, 0, 4, "signed"))], _ffi.MI_EINVAL, ""),
             ([("sum_expr", (i._data.data_ptr(), 0, 4, "any"))], _ffi.MI_EINVAL, "")]
    for specs, code, word in cases:
        for call in (lambda: da.aggregate_vectors(ctx, specs, 3), lambda: da.group_aggregate_vectors(ctx, key, specs, 3)):
            with pytest.raises(da.MiError) as e:
                call()
            assert e.value.code == code and word in str(e.value), (specs, e.value.code, str(e.value))
    # (2^53 is exact, and so is INT64_MIN) and the entry still answers
    assert da.aggregate_vectors(ctx, [("sum_expr", (f.spec(), 1 << 53, I64_MIN)), ("count_star",)], 2) == [float(I64_MIN) + float((1 << 53) + I64_MIN), 2]
    assert da.aggregate_vectors(ctx, [("sum_expr", i.spec())], 0) == [None]

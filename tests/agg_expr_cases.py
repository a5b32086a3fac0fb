"""The one reference for MI_AGG_SUM_EXPR, SUM(f_0 * ... * f_{F-1}) with a factor add + mul * column or a constant, and the
hand-built vectors the kernel-level tests run it on.  Nothing here calls the library.

Integers: Python ints, reduced modulo 2^128 once at the end and read back as two's complement -- reduction is a ring
homomorphism, so this is what the kernels' wrapping 128-bit arithmetic gives at every step.
Doubles: fractions.Fraction.  A term is the exact product of the exact factors; a result is held to
    |got - sum(terms)| <= 2 * (n + 3 F) * 2^-53 * sum(|term|)
-- at most 3 F - 1 roundings go into a term (a multiplication and an addition per factor, a multiplication per further
factor) and n - 1 into the sum, each relative 2^-53, first order; doubled, as the 2 n 2^-53 sum|x| rule of the plain sums is.
tests/test_agg_expr_host.py holds this module to pyarrow.compute's decimal arithmetic on TPC-H Q1."""
import struct
from fractions import Fraction

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
W = 2048


def wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


class Factor:
    """add + mul * values[row], or the constant add (values None).  values: Python numbers; ok: bool per row or None"""

    def __init__(self, values=None, ok=None, mul=1, add=0):
        self.values, self.ok, self.mul, self.add = values, ok, mul, add

    def valid(self, row):
        return self.values is None or self.ok is None or bool(self.ok[row])

    def at(self, row, number=int):
        if self.values is None:
            return number(self.add)
        return number(self.add) + number(self.mul) * number(self.values[row])


def contributing(factors, rows):
    """the NULL rule: every column a factor names is not NULL in the row"""
    return [r for r in rows if all(f.valid(r) for f in factors)]


def sum_expr_int(factors, rows):
    """-> (sum modulo 2^128 as two's complement, or None without a contributor; contributing rows)"""
    rows = contributing(factors, rows)
    if not rows:
        return None, 0
    total = 0
    for r in rows:
        term = 1
        for f in factors:
            term *= f.at(r)
        total += term
    return wrap128(total), len(rows)


def sum_expr_float(factors, rows):
    """-> (exact sum, sum of |term|, contributing rows) as Fractions; the values must be finite"""
    rows = contributing(factors, rows)
    total, total_abs = Fraction(0), Fraction(0)
    for r in rows:
        term = Fraction(1)
        for f in factors:
            term *= f.at(r, Fraction)
        total += term
        total_abs += abs(term)
    return total, total_abs, len(rows)


def float_bound(n, n_factors, total_abs):
    return 2 * (n + 3 * n_factors) * Fraction(1, 1 << 53) * total_abs


def check_float(got, factors, rows, what=""):
    """got: (value, count) of the library"""
    exact, total_abs, n = sum_expr_float(factors, rows)
    value, count = got
    assert count == n, (what, got, n)
    if n == 0:
        assert value is None, (what, got)
        return
    err, bound = abs(Fraction(value) - exact), float_bound(n, len(factors), total_abs)
    print("%s: got %r, exact %r, |err| %.3g, bound %.3g" % (what, value, float(exact), float(err), float(bound)))
    assert err <= bound, (what, value, float(exact), float(err), float(bound))


# ---- TPC-H Q1's sums over the stored integers of DECIMAL(15, 2) columns: scale 2, 2, 4, 6
def q1_factor_lists(quantity, price, discount, tax):
    """four Factor lists -- sum_qty, sum_base_price, sum_disc_price, sum_charge -- over columns of stored integers"""
    return [[Factor(quantity)],
            [Factor(price)],
            [Factor(price), Factor(discount, mul=-1, add=100)],
            [Factor(price), Factor(discount, mul=-1, add=100), Factor(tax, mul=1, add=100)]]


Q1_SPECS = [("sum", "l_quantity"),
            ("sum", "l_extendedprice"),
            ("sum_expr", "l_extendedprice", ("l_discount", -1, 100)),
            ("sum_expr", "l_extendedprice", ("l_discount", -1, 100), ("l_tax", 1, 100)),
            ("sum", "l_discount"),
            ("count_star",)]


def q1_reference(table):
    """pyarrow table of lineitem -> {(returnflag, linestatus): [sum_qty, sum_base_price, sum_disc_price, sum_charge, sum_disc, count]}
    in stored integers, by this module's integer reference"""
    from decimal import Decimal

    def stored(name):
        return [int(v.scaleb(2)) for v in table.column(name).to_pylist()]

    qty, price, disc, tax = stored("l_quantity"), stored("l_extendedprice"), stored("l_discount"), stored("l_tax")
    assert all(isinstance(v, Decimal) for v in table.column("l_tax").to_pylist()[:3])
    flags, status = table.column("l_returnflag").to_pylist(), table.column("l_linestatus").to_pylist()
    groups = {}
    for r, key in enumerate(zip(flags, status)):
        groups.setdefault(key, []).append(r)
    out = {}
    for key, rows in groups.items():
        sums = [sum_expr_int(fs, rows)[0] for fs in q1_factor_lists(qty, price, disc, tax)]
        out[key] = sums + [sum(disc[r] for r in rows), len(rows)]
    return out


# ---- the hand-built vectors of the kernel-level tests
INT_TYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}


def int_columns(n, seed, with_nulls, garbage=True):
    """name -> (numpy values, ok or None): every width and signedness, the type's extremes in the first rows; under a NULL
    the bytes are garbage (whatever the generator drew: nothing is zeroed)"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, t in INT_TYPES.items():
        info = np.iinfo(t)
        v = rng.integers(info.min, info.max, n, dtype=t, endpoint=True)
        v[: min(4, n)] = [info.min, info.max, 0, info.max][: min(4, n)]
        ok = (rng.random(n) >= 0.2) if with_nulls else None
        out[name] = (v, ok)
    return out


def float_columns(n, seed, with_nulls):
    rng = np.random.default_rng(seed)
    out = {}
    out["f32"] = (rng.normal(0, 1e3, n).astype(np.float32), (rng.random(n) >= 0.2) if with_nulls else None)
    out["f64"] = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 7, n), (rng.random(n) >= 0.2) if with_nulls else None)
    out["g64"] = (rng.normal(1, 0.5, n), (rng.random(n) >= 0.2) if with_nulls else None)
    return out

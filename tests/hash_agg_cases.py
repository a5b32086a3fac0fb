"""Shared cases and the reference of the hash GROUP BY tests (K11: mi_scan_hash_aggregate, mi_hash_aggregate_vectors).
Nothing here touches the library or a GPU: expected values come from a Python dict loop over Python ints, the hash is a
restatement of hashgroup::Hash (held to the C++ by test_hash_aggregate_host.py), and the GPU tests build colliding keys
from it.  test_hash_aggregate_host.py holds `reference` itself to pyarrow's group_by on what pyarrow can express."""
import math
import struct

import numpy as np

W = 2048
M64 = (1 << 64) - 1
EMPTY_KEY = M64                     # hashgroup::kEmptyKey as an unsigned word: the int64 -1
MAX_HASH_GROUPS = 1 << 24
CANONICAL_NAN = 0x7FF8000000000000
INT_TYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
# a fixed key list whose hashes tests/sanitize/hash_group_check.cpp prints
HASH_PROBE_KEYS = [0, 1, 2, 63, 64, 0xFFFFFFFF, 1 << 32, (1 << 63) - 1, 1 << 63, M64 - 1, 0x0123456789ABCDEF, 0xDEADBEEFCAFEF00D]


def hash64(key):
    """hashgroup::Hash over the key word (an int of 0 .. 2^64 - 1)"""
    x = key & M64
    x ^= x >> 31
    x = (x * 0x6A09E667F3BCC909) & M64
    x ^= x >> 29
    x = (x * 0xBB67AE8584CAA73B) & M64
    x ^= x >> 32
    return x


def slots_for(max_groups):
    s = 64
    while s < 2 * max_groups:
        s <<= 1
    return s


def table_bytes(max_groups, n_aggs):
    s = slots_for(max_groups)
    return 32 + 8 * s + 24 * (s + 2) * n_aggs


def keys_in_slot(slot, slots, count, start=1):
    """the first `count` non-negative int64 keys from `start` on whose home slot is `slot`"""
    out, k = [], start
    while len(out) < count:
        if hash64(k) & (slots - 1) == slot:
            out.append(k)
        k += 1
    return out


def wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def canonical(x):
    """a double as MIN / MAX return it: every NaN the one quiet NaN, -0.0 as +0.0"""
    if x != x:
        return struct.unpack("<d", struct.pack("<Q", CANONICAL_NAN))[0]
    return x + 0.0 if x == 0 else x


def float_order(x):
    """the total order of filter_key.hpp: NaN greatest (above +inf), -0.0 = +0.0"""
    return (1, 0.0) if x != x else (0, x + 0.0 if x == 0 else x)


class HostColumn:
    """values (numpy) with the rows that are valid; cls: signed / unsigned / float / wide (Python ints)"""

    def __init__(self, values, cls, ok=None):
        if cls == "wide":
            self.py = [int(v) for v in values]
            self.np = np.array([[v & M64, (v >> 64) & M64] for v in self.py], np.uint64).reshape(-1, 2)
            self.width = 16
        else:
            self.np = np.ascontiguousarray(values)
            self.py = [float(v) for v in self.np] if cls == "float" else [int(v) for v in self.np]
            self.width = self.np.dtype.itemsize
        self.cls = cls
        self.has_validity = ok is not None
        self.ok = np.ones(len(self.py), bool) if ok is None else np.asarray(ok, bool)

    def key(self, r):
        return self.py[r] if self.ok[r] else None


def _factor(f):
    """a sum_expr factor -> (column or None, mul, add)"""
    if isinstance(f, (int, float)):
        return None, 1, f
    if isinstance(f, tuple):
        return (None, 1, f[1]) if f[0] is None else f
    return f, 1, 0


def expected(op, args, rows):
    """one aggregate over the rows of one group -> (value, contributing rows); integer sums wrap modulo 2^128"""
    if op == "count_star":
        return len(rows), len(rows)
    if op == "sum_expr":
        factors = [_factor(f) for f in args]
        cols = [c for c, _, _ in factors if c is not None]
        rows = [r for r in rows if all(c.ok[r] for c in cols)]
        total = 0
        for r in rows:
            prod = 1
            for c, mul, add in factors:
                prod *= add if c is None else add + mul * c.py[r]
            total += prod
        return (wrap128(total) if rows else None), len(rows)
    rows = [r for r in rows if all(c.ok[r] for c in args)]
    a = args[0]
    if op == "count":
        return len(rows), len(rows)
    if not rows:
        return None, 0
    vals = [a.py[r] for r in rows]
    if op == "sum_product":
        vals = [x * args[1].py[r] for x, r in zip(vals, rows)]
    if op in ("sum", "sum_product"):
        assert a.cls != "float", "the hash GROUP BY takes no floating-point sum"
        return wrap128(sum(vals)), len(rows)
    if a.cls == "float":
        return canonical((min if op == "min" else max)(vals, key=float_order)), len(rows)
    return (min if op == "min" else max)(vals), len(rows)


def order_key(key):
    """ascending, NULLS LAST"""
    return (1, 0) if key is None else (0, key)


def reference(key, aggs, rows):
    """the dict loop: [(key value or None, [(value, contributing rows), ...]), ...] sorted ascending by key, NULLS LAST.
    `aggs`: (op, column, ...) with HostColumns; sum_expr factors as Relation.aggregate takes them, columns as HostColumns"""
    groups = {}
    for r in rows:
        groups.setdefault(key.key(r), []).append(r)
    return [(k, [expected(op, args, groups[k]) for op, *args in aggs]) for k in sorted(groups, key=order_key)]


def same_value(got, want):
    """ints by value and type, floats by their bits, None by identity"""
    if isinstance(want, float):
        return isinstance(got, float) and bits(got) == bits(want)
    if want is None:
        return got is None
    return isinstance(got, int) and not isinstance(got, bool) and got == want


def assert_same(got, want, what=""):
    """`got`: [((key,), [(value, count), ...]), ...] as hash_aggregate_vectors(detail=True) returns it"""
    assert [g[0][0] for g in got] == [w[0] for w in want], (what, [g[0] for g in got][:6], [w[0] for w in want][:6])
    for (gk, gv), (wk, wv) in zip(got, want):
        assert len(gv) == len(wv)
        for a, ((g_val, g_cnt), (w_val, w_cnt)) in enumerate(zip(gv, wv)):
            assert g_cnt == w_cnt and same_value(g_val, w_val), (what, "group", wk, "aggregate", a, (g_val, g_cnt), (w_val, w_cnt))


def words(ok):
    """validity words (uint64, one spare word) of a boolean vector"""
    b = np.zeros((len(ok) + 63) // 64 * 64 + 64, np.uint8)
    b[: len(ok)] = ok
    return np.packbits(b, bitorder="little").view(np.uint64)


def type_edges(name):
    """0, the type's minimum and maximum, the empty mark's image and its two neighbours (-2, -1, 0 for a signed type; for
    uint64 the words 2^64 - 2, 2^64 - 1 and 0), as values of the numpy type"""
    dt = INT_TYPES[name]
    info = np.iinfo(dt)
    vals = [0, info.min, info.max, 1]
    vals += [-2, -1] if info.min < 0 else [info.max - 1]
    return np.array(vals, dt)


def pyarrow_table_and_specs(seed=7, n=5000, n_keys=900):
    """a table pyarrow's group_by can aggregate exactly (int64 sums that do not wrap, counts, min / max), as HostColumns"""
    rng = np.random.default_rng(seed)
    key = HostColumn(rng.integers(-n_keys // 2, n_keys // 2, n).astype(np.int64), "signed", rng.random(n) >= 0.05)
    i64 = HostColumn(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), "signed", rng.random(n) >= 0.2)
    i32 = HostColumn(rng.integers(-1000, 1000, n).astype(np.int32), "signed")
    f64 = HostColumn(rng.normal(0, 100, n), "float", rng.random(n) >= 0.2)
    cols = {"k": key, "i64": i64, "i32": i32, "f64": f64}
    aggs = [("count_star",), ("count", i64), ("sum", i64), ("sum", i32), ("min", i64), ("max", i32), ("min", f64), ("max", f64)]
    pa_aggs = [([], "count_all"), ("i64", "count"), ("i64", "sum"), ("i32", "sum"), ("i64", "min"), ("i32", "max"), ("f64", "min"), ("f64", "max")]
    return cols, aggs, pa_aggs


def to_arrow(cols):
    import pyarrow as pa
    return pa.table({name: pa.array(c.np, mask=~c.ok) for name, c in cols.items()})


def pyarrow_groups(table, key, pa_aggs):
    """pyarrow's group_by as [(key or None, [value, ...]), ...] in the reference's order"""
    out = table.group_by(key, use_threads=False).aggregate(pa_aggs)
    names = [c for c in out.column_names if c != key]
    rows = [(k, [out[nm][i].as_py() for nm in names]) for i, k in enumerate(out[key].to_pylist())]
    return sorted(rows, key=lambda r: order_key(r[0]))

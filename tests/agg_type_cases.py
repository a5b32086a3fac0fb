"""The type matrix of the fused aggregates (mi_scan_aggregate K9, mi_scan_group_aggregate K10, mi_scan_hash_aggregate K11):
one column of every Arrow type the scan's bind code takes or refuses, and the reference the scan-level tests hold the
library to.  Plain Python, numpy and pyarrow: nothing here calls the library or needs a GPU.

Every entry is written down twice.  First its STORED values -- what the scan holds after the decode: the unscaled integer of
a DECIMAL, days of a DATE, microseconds of a TIME / TIMESTAMP WITH TIME ZONE, the Arrow unit of a plain TIMESTAMP, the float a
half widens to, the hugeint_t of a UUID, the byte of a BOOLEAN, the bytes of a VARCHAR / BLOB -- as Python values, None for NULL.
Then the Arrow array, built from the stored values by the INVERSE of the decode (raw little-endian integers under a validity
bitmap), so that tests/golden/make_golden.py::canon_column of the array must give the stored values back
(test_agg_type_cases_host.py).

N = 2 * 2048 + 904 rows in record batches of 3000 and 2000: a batch that ends inside a window, a ragged last window.  Every
column has 10 - 20 % NULLs (the run-end entries: NULL runs); its edge values sit on valid rows among the first 40.

The reference is a dict loop over Python ints: SUM wraps at 128 bits (wrap128, as _wrap128 of test_gpu_scan_aggregate.py),
MIN / MAX of floats follow DuckDB's total order (NaN greatest, -0.0 = +0.0, the canonical NaN), float sums are held to
2 n 2^-53 fsum|v| against math.fsum, the bound of test_gpu_scan_aggregate.py::check; everything else is exact."""
import math
import struct
import uuid
import zlib

import numpy as np
import pyarrow as pa

import extension_cases as ec

W = 2048
N = 2 * W + 904
BATCHES = (3000, 2000)
EDGE_ROWS = 40
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
CANONICAL_NAN = 0x7FF8000000000000
FILTER = ("or", ("k", "<", 1500), ("k", ">=", 2600))        # two windows partly selected
FILTER_ROWS = [r for r in range(N) if r < 1500 or r >= 2600]
ENTRY_POINTS = ("aggregate", "group_key", "hash_key")

# what a column is to the aggregates
INT, UINT, FLOAT, WIDE, BOOL, STRING, REFUSED = "int", "uint", "float", "wide", "bool", "string", "refused"


class Takes:
    takes = True

    def __repr__(self):
        return "takes"


class Refuses:
    takes = False

    def __init__(self, *words):
        self.words = words

    def __repr__(self):
        return "refuses%r" % (self.words,)


class Entry:
    """name, pyarrow type, stored values, Arrow array (one chunk, or one per record batch for a run-end entry), class,
    DuckDB type, and per entry point Takes() or Refuses(words the message must contain)"""

    def __init__(self, name, type, stored, array, cls, duck, canon=None, low=None, file="main", raw=None):
        self.name, self.type, self.stored, self.array, self.cls, self.duck, self.file = name, type, stored, array, cls, duck, file
        self.canon = stored if canon is None else canon   # what canon_column gives: the stored values but for extension types
        self.low = low                                    # Entry of the low-cardinality variant (a K10 key), or None
        self.raw = raw                                    # uuid: stored hugeint -> the 16 bytes of the text order
        col = "'%s'" % name
        if cls in (INT, UINT):
            self.expect = dict(aggregate=Takes(), group_key=Takes(), hash_key=Takes())
        elif cls == FLOAT:
            self.expect = dict(aggregate=Takes(), group_key=Refuses(col, "GROUP BY", "(%s)" % duck, "stays above the scan"),
                               hash_key=Refuses(col, "hash GROUP BY", "(%s)" % duck, "stays above the scan"))
        elif cls == WIDE:      # COUNT / MIN / MAX; SUM is the documented refusal (sum_words)
            self.expect = dict(aggregate=Takes(), group_key=Takes(), hash_key=Refuses(col, "(%s)" % duck, "a 16-byte key is not one 64-bit word"))
        elif cls == BOOL:      # COUNT; SUM / MIN / MAX are refused
            self.expect = dict(aggregate=Refuses(col, "(%s)" % duck), group_key=Takes(), hash_key=Takes())
        elif cls == STRING:
            self.expect = dict(aggregate=Refuses(col, "(%s)" % duck), group_key=Takes(), hash_key=Refuses(col, "(%s)" % duck, "a VARCHAR / BLOB key is not one 64-bit word"))
        else:
            self.expect = dict(aggregate=Refuses(col, "(%s)" % duck), group_key=Refuses(col, "GROUP BY", "(%s)" % duck),
                               hash_key=Refuses(col, "GROUP BY", "(%s)" % duck))
        self.sum_words = (col, "SUM", "(%s)" % duck) if cls == WIDE else None
        self.count_works = True          # COUNT(col) is taken even where SUM / MIN / MAX are refused (decimal256: nothing is)
        self.long_key = False            # fixed_size_binary(13): a selected valid row has no inline image

    @property
    def is_ree(self):
        return isinstance(self.type, pa.RunEndEncodedType)

    def chunks(self):
        """the column per record batch"""
        if isinstance(self.array, list):
            return self.array
        return [self.array.slice(0, BATCHES[0]), self.array.slice(BATCHES[0], BATCHES[1])]

    def key_out(self, v):
        """a stored value as Relation.group_aggregate / hash_aggregate return it as a key"""
        if v is None:
            return None
        if self.duck == "UUID":
            return uuid.UUID(bytes=self.raw[v])
        if self.duck == "BOOLEAN":
            return bool(v)
        if self.duck == "VARCHAR":
            return v.decode()
        return v


# ------------------------------------------------------------------------------------------------ building blocks
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _ok(rng, n=N, edges=EDGE_ROWS):
    """row validity: 10 - 20 % NULLs, the odd rows below `edges` valid (the edge values sit there)"""
    ok = np.ones(n, bool)
    ok[rng.permutation(np.arange(edges, n))[: int(n * rng.uniform(0.11, 0.19))]] = False
    ok[0:edges:2] = False
    return ok


def _place(values, edge_values):
    """edge value i on row 2 i + 1"""
    assert 2 * len(edge_values) <= EDGE_ROWS, len(edge_values)
    for i, v in enumerate(edge_values):
        values[2 * i + 1] = v
    return values


def _bitmap(ok):
    return pa.py_buffer(np.packbits(np.asarray(ok, bool), bitorder="little").tobytes())


def _fixed(t, raw, ok):
    """a fixed-width array from its raw little-endian bytes and the row validity"""
    ok = np.asarray(ok, bool)
    return pa.Array.from_buffers(t, len(ok), [_bitmap(ok), pa.py_buffer(raw)], null_count=int(len(ok) - ok.sum()))


def _le(values, width, ok):
    """ints -> little-endian two's complement of `width` bytes per row (zero under a NULL)"""
    mask = (1 << (8 * width)) - 1
    return b"".join(((int(v) & mask) if o else 0).to_bytes(width, "little") for v, o in zip(values, ok))


def _masked(values, ok):
    return [v if o else None for v, o in zip(values, ok)]


def _int_entry(name, t, width, stored, ok, cls=INT, duck=None, raw=None, **more):
    """an integer-like column whose Arrow integers are `raw` (default: the stored values themselves)"""
    arr = _fixed(t, _le(stored if raw is None else raw, width, ok), ok)
    return Entry(name, t, _masked([int(v) for v in stored], ok), arr, cls, duck, **more)


def _random_ints(rng, lo, hi, n=N):
    """n Python ints in [lo, hi], any size: magnitudes spread over the bit lengths"""
    span = hi - lo
    bits = max(span.bit_length(), 1)
    out = []
    for b, x in zip(rng.integers(1, bits + 1, n), rng.random(n)):
        out.append(lo + min(span, int(x * (1 << int(b)))) if rng.random() < 0.5 else hi - min(span, int(x * (1 << int(b)))))
    return out


def _low(entry, build, keep=24):
    """the low-cardinality variant of `entry` for a K10 key: the edge values where they were, `keep` of the column's values
    elsewhere -- at most EDGE_ROWS / 2 + keep distinct values and NULL in every window"""
    rng = _rng(entry.name + "/low")
    live = [v for v in entry.stored[EDGE_ROWS:] if v is not None]
    pool = [live[i] for i in rng.integers(0, len(live), keep)]
    values = [pool[i] for i in rng.integers(0, keep, N)]
    for r in range(1, EDGE_ROWS, 2):
        if entry.stored[r] is not None:
            values[r] = entry.stored[r]
    ok = _ok(rng)
    low = build(entry.name + "_low", values, ok)
    assert len({v for v in low.stored}) <= EDGE_ROWS // 2 + keep + 1
    return low


MATRIX = []


def _add(entry, low_build=None):
    if low_build is not None:
        entry.low = _low(entry, low_build)
    elif entry.cls in (BOOL, STRING) or entry.is_ree:
        entry.low = entry            # few distinct values already
    MATRIX.append(entry)
    return entry


# ------------------------------------------------------------------------------------------------ plain integers, DATE
def _plain(name, t, dtype, duck):
    info = np.iinfo(dtype)
    width = np.dtype(dtype).itemsize
    cls = UINT if info.min == 0 else INT

    def build(nm, values, ok):
        return _int_entry(nm, t, width, values, ok, cls, duck)

    rng = _rng(name)
    values = _place([int(v) for v in rng.integers(info.min, info.max, N, dtype=dtype, endpoint=True)], [info.min, info.max, 0, info.max - 1, -1 & info.max if cls == UINT else -1])
    _add(build(name, values, _ok(rng)), build)


_plain("i8", pa.int8(), np.int8, "TINYINT")
_plain("i16", pa.int16(), np.int16, "SMALLINT")
_plain("u16", pa.uint16(), np.uint16, "USMALLINT")
_plain("i32", pa.int32(), np.int32, "INTEGER")
_plain("i64", pa.int64(), np.int64, "BIGINT")
_plain("u64", pa.uint64(), np.uint64, "UBIGINT")


def _date32():
    def build(nm, values, ok):
        return _int_entry(nm, pa.date32(), 4, values, ok, INT, "DATE")
    rng = _rng("date32")
    values = _place([int(v) for v in rng.integers(-30000, 30000, N)], [-(1 << 31), (1 << 31) - 1, 0, -1])
    _add(build("date32", values, _ok(rng)), build)


def _date64():
    """stored days; the Arrow milliseconds are days * 86 400 000 (pyarrow validates whole days)"""
    day = 86400000

    def build(nm, values, ok):
        return _int_entry(nm, pa.date64(), 8, values, ok, INT, "DATE", raw=[d * day for d in values])
    rng = _rng("date64")
    values = _place([int(v) for v in rng.integers(-40000, 40000, N)], [-1, 1, -(1 << 31), (1 << 31) - 1, -25567, 0])   # (DATE is 32 bits of days)
    _add(build("date64", values, _ok(rng)), build)


_date32()
_date64()


# ------------------------------------------------------------------------------------------------ TIME
def _time(name, t, width, ticks_per_day, to_us):
    """stored microseconds; to_us > 0: stored = ticks * to_us, to_us < 0: stored = ticks / -to_us (time64[ns])"""
    def build(nm, values, ok):
        if to_us > 0:
            raw = [v // to_us for v in values]
            assert all(r * to_us == v for r, v in zip(raw, values))
        else:                                       # ns: microseconds plus 0 .. 999 ns that the division drops
            rng = _rng(nm + "/ns")
            raw = [v * -to_us + int(p) for v, p in zip(values, rng.integers(0, -to_us, len(values)))]
            raw[1] = ticks_per_day - 1               # the day's last tick: 86 399 999 999 999 ns
            assert values[1] == (ticks_per_day - 1) // -to_us
        return _int_entry(nm, t, width, values, ok, INT, "TIME", raw=raw)
    rng = _rng(name)
    scale = to_us if to_us > 0 else 1
    last = (ticks_per_day - 1) * scale if to_us > 0 else (ticks_per_day - 1) // -to_us
    ticks = [int(v) for v in rng.integers(0, ticks_per_day if to_us > 0 else ticks_per_day // -to_us, N)]
    values = _place([v * scale for v in ticks], [last, 0, scale, last - scale])
    _add(build(name, values, _ok(rng)), build)


_time("time32_s", pa.time32("s"), 4, 86400, 1000000)
_time("time32_ms", pa.time32("ms"), 4, 86400000, 1000)
_time("time64_us", pa.time64("us"), 8, 86400000000, 1)
_time("time64_ns", pa.time64("ns"), 8, 86400000000000, -1000)


# ------------------------------------------------------------------------------------------------ TIMESTAMP
# (raw Arrow value, stored with tz="UTC") of the edges; without a time zone the stored value is the raw one
_TS_EDGES = {
    "s": [(9223372036854, 9223372036854000000), (-9223372036854, -9223372036854000000), (0, 0), (-1, -1000000), (1, 1000000)],
    "ms": [(9223372036854775, 9223372036854775000), (-9223372036854775, -9223372036854775000), (0, 0), (-1, -1000), (1, 1000)],
    "us": [(I64_MIN + 1, I64_MIN + 1), (I64_MAX, I64_MAX), (0, 0), (-1, -1), (1, 1)],
    "ns": [(I64_MIN, -9223372036854775), (I64_MAX, 9223372036854775), (-1, 0), (-999, 0), (-1000, -1), (-1001, -1), (999, 0), (1000, 1)],
}
_TS_RANGE = {"s": 4 * 10 ** 9, "ms": 4 * 10 ** 12, "us": 4 * 10 ** 15, "ns": 4 * 10 ** 18}


def _timestamp(unit, tz):
    name = "ts_%s%s" % (unit, "_utc" if tz else "")
    t = pa.timestamp(unit, tz=tz)
    duck = "TIMESTAMP WITH TIME ZONE" if tz else {"s": "TIMESTAMP_S", "ms": "TIMESTAMP_MS", "us": "TIMESTAMP", "ns": "TIMESTAMP_NS"}[unit]
    factor = {"s": 1000000, "ms": 1000, "us": 1, "ns": 0}[unit]

    def stored_of(raw):
        if not tz or unit == "us":
            return raw
        if unit == "ns":
            return -(-raw // 1000) if raw < 0 else raw // 1000      # truncation toward zero
        return raw * factor

    def build(nm, raws, ok):
        return _int_entry(nm, t, 8, [stored_of(r) for r in raws], ok, INT, duck, raw=raws)

    rng = _rng(name)
    raws = [int(v) for v in rng.integers(-_TS_RANGE[unit], _TS_RANGE[unit], N)]
    _place(raws, [r for r, _ in _TS_EDGES[unit]])
    e = build(name, raws, _ok(rng))
    for i, (r, s) in enumerate(_TS_EDGES[unit]):                    # the literals above, not stored_of, are the record
        assert e.stored[2 * i + 1] == (s if tz else r), (name, r, s)

    def low_build(nm, values, ok):                                   # a key variant is built from stored values: map back
        if not tz or unit == "us":
            back = values
        elif unit == "ns":
            back = [v * 1000 + (int(p) if v > 0 else -int(p) if v < 0 else 0) for v, p in zip(values, _rng(nm).integers(0, 1000, len(values)))]
            back = [max(I64_MIN, min(I64_MAX, b)) for b in back]
        else:
            back = [v // factor for v in values]
        low = build(nm, back, ok)
        assert low.stored == _masked(values, ok), nm
        return low
    _add(e, low_build)


for _unit in ("s", "ms", "us", "ns"):
    _timestamp(_unit, None)
    _timestamp(_unit, "UTC")


# ------------------------------------------------------------------------------------------------ DECIMAL
def _decimal(name, t, width, cls=None):
    p = t.precision
    top = 10 ** p - 1
    duck = "DECIMAL(%d,%d)" % (p, t.scale)
    cls = cls or (INT if p <= 18 else WIDE)

    def build(nm, values, ok):
        return _int_entry(nm, t, width, values, ok, cls, duck)
    rng = _rng(name)
    values = _place(_random_ints(rng, -top, top), [top, -top, 0, -1, 1, -(top // 2 + 1)])
    e = build(name, values, _ok(rng))
    if cls == REFUSED:
        e.count_works = False
        _add(e)
    else:
        _add(e, build)


_decimal("dec128_1", pa.decimal128(1, 0), 16)
_decimal("dec128_4", pa.decimal128(4, 1), 16)
_decimal("dec128_5", pa.decimal128(5, 2), 16)
_decimal("dec128_9", pa.decimal128(9, 2), 16)
_decimal("dec128_10", pa.decimal128(10, 3), 16)
_decimal("dec128_18", pa.decimal128(18, 4), 16)
_decimal("dec128_19", pa.decimal128(19, 0), 16)
_decimal("dec128_38", pa.decimal128(38, 10), 16)
_decimal("dec32_4", pa.decimal32(4, 2), 4)
_decimal("dec32_9", pa.decimal32(9, 0), 4)
_decimal("dec64_4", pa.decimal64(4, 0), 8)
_decimal("dec64_9", pa.decimal64(9, 3), 8)
_decimal("dec64_18", pa.decimal64(18, 6), 8)
_decimal("dec256_40", pa.decimal256(40, 0), 32, REFUSED)


# ------------------------------------------------------------------------------------------------ floats
def _float(name, t, dtype, duck, edges):
    rng = _rng(name)
    values = (np.round(rng.normal(0, 40, N) * 4) / 4).astype(dtype) if dtype == np.float16 else (rng.normal(0, 1e4, N) * rng.choice([1e-6, 1.0, 1e6], N)).astype(dtype)
    values[1:2 * len(edges):2] = np.array(edges, dtype)
    assert 2 * len(edges) <= EDGE_ROWS
    ok = _ok(rng)
    arr = _fixed(t, np.where(ok, values, dtype(0)).astype(dtype).tobytes(), ok)
    _add(Entry(name, t, _masked([float(v) for v in values], ok), arr, FLOAT, duck))


_NAN16 = np.array([0x7E00, 0xFE01], np.uint16).view(np.float16)       # NaNs of both signs
_float("f16", pa.float16(), np.float16, "FLOAT", [65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 0.0, -0.0, np.inf, -np.inf, _NAN16[0], _NAN16[1]])
_float("f32", pa.float32(), np.float32, "FLOAT", [1e9, -1e9, 1e-45, 0.0, -0.0])
_float("f64", pa.float64(), np.float64, "DOUBLE", [1e9, -1e9, 5e-324, 0.0, -0.0])


# ------------------------------------------------------------------------------------------------ BOOLEAN, bool8, UUID
def _bool():
    rng = _rng("bool")
    values = rng.random(N) < 0.5
    ok = _ok(rng)
    arr = pa.Array.from_buffers(pa.bool_(), N, [_bitmap(ok), _bitmap(values & ok)], null_count=int(N - ok.sum()))
    _add(Entry("bool", pa.bool_(), _masked([int(v) for v in values], ok), arr, BOOL, "BOOLEAN", canon=_masked([bool(v) for v in values], ok)))


def _bool8_values(rng, n):
    raw = rng.integers(0, 2, n).astype(np.int8)
    raw[rng.integers(0, n, n // 4)] = rng.choice(np.array(ec.BOOL8_BYTES, np.uint8).view(np.int8), n // 4)
    return raw


def _bool8():
    rng = _rng("bool8")
    raw = _bool8_values(rng, N)
    raw[1:9:2] = [0, 1, 2, -1]
    ok = _ok(rng)
    storage = _fixed(pa.int8(), np.where(ok, raw, 0).astype(np.int8).tobytes(), ok)
    stored = _masked([int(v) for v in ec.bool8(raw)], ok)
    _add(Entry("bool8", pa.bool8(), stored, pa.ExtensionArray.from_storage(pa.bool8(), storage), BOOL, "BOOLEAN", canon=_masked([int(v) for v in raw], ok)))


def _uuid_rows(rng, n, pool=None):
    """n x 16 random bytes, or rows drawn from `pool`"""
    return rng.integers(0, 256, (n, 16), dtype=np.uint8) if pool is None else pool[rng.integers(0, len(pool), n)]


def _uuid_entry(name, raw, ok):
    stored = ec.hugeint_of(ec.uuid_from_arrow(raw))
    storage = _fixed(pa.binary(16), np.where(ok[:, None], raw, 0).astype(np.uint8).tobytes(), ok)
    rows = [r.tobytes() for r in raw]
    return Entry(name, pa.uuid(), _masked(stored, ok), pa.ExtensionArray.from_storage(pa.uuid(), storage), WIDE, "UUID", canon=_masked(rows, ok),
                 raw={s: b for s, b in zip(stored, rows)})


def _uuid():
    rng = _rng("uuid")
    raw = _uuid_rows(rng, N)
    edges = np.frombuffer(b"".join(ec.UUID_EDGES), np.uint8).reshape(-1, 16)
    raw[1:2 * len(edges):2] = edges
    e = _uuid_entry("uuid", raw, _ok(rng))
    assert e.stored[1] == -(1 << 127) and e.stored[3] == (1 << 127) - 1 and e.stored[5] == -1 and e.stored[7] == 0   # 00.., ff.., 7f ff.., 80 00..
    rng = _rng("uuid/low")
    low_raw = _uuid_rows(rng, N, pool=raw[EDGE_ROWS:EDGE_ROWS + 24])
    low_raw[1:EDGE_ROWS:2] = raw[1:EDGE_ROWS:2]
    e.low = _uuid_entry("uuid_low", low_raw, _ok(rng))
    MATRIX.append(e)


_bool()
_bool8()
_uuid()


# ------------------------------------------------------------------------------------------------ key-only types
_WORDS = [b"", b"a", b"a\0", b"MAIL", b"SHIP", b"REG AIR", b"\xc3\xa9t\xc3\xa9", b"twelve bytes", b"eleven byte", b"abcd", b"abcde", b"zzzzzzzzzzzz"]


def _strings(name, t, duck):
    rng = _rng(name)
    values = _place([_WORDS[i] for i in rng.integers(0, len(_WORDS), N)], _WORDS)
    ok = _ok(rng)
    stored = _masked(values, ok)
    arr = pa.array([v.decode() if v is not None and duck == "VARCHAR" else v for v in stored], t)
    _add(Entry(name, t, stored, arr, STRING, duck, canon=[v.decode() if v is not None and duck == "VARCHAR" else v for v in stored]))


def _fixed_binary(name, width):
    rng = _rng(name)
    pool = [bytes(width), b"\xff" * width, b"a" * width, b"a" * (width - 1) + b"\0", b"\0" + b"a" * (width - 1)] + [rng.integers(0, 256, width, dtype=np.uint8).tobytes() for _ in range(12)]
    values = _place([pool[i] for i in rng.integers(0, len(pool), N)], pool[:5])
    ok = _ok(rng)
    arr = _fixed(pa.binary(width), b"".join(v if o else bytes(width) for v, o in zip(values, ok)), ok)
    e = Entry(name, pa.binary(width), _masked(values, ok), arr, STRING, "BLOB")
    if width > 12:
        e.long_key = True
    _add(e)


_strings("str", pa.string(), "VARCHAR")
_strings("large_string", pa.large_string(), "VARCHAR")
_strings("string_view", pa.string_view(), "VARCHAR")
_strings("large_binary", pa.large_binary(), "BLOB")
_fixed_binary("fsb3", 3)
_fixed_binary("fsb12", 12)
_fixed_binary("fsb13", 13)


# ------------------------------------------------------------------------------------------------ refused: INTERVAL
def _duration(unit):
    """refused by every aggregate; the stored values are the microseconds canon_column gives (ns: truncated toward zero)"""
    name = "dur_" + unit
    rng = _rng(name)
    factor = {"s": 1000000, "ms": 1000, "us": 1, "ns": 0}[unit]
    raws = [int(v) for v in rng.integers(-10 ** 9, 10 ** 9, N)]
    stored = [r * factor if factor else (-(-r // 1000) if r < 0 else r // 1000) for r in raws]
    _add(_int_entry(name, pa.duration(unit), 8, stored, _ok(rng), REFUSED, "INTERVAL", raw=raws))


def _interval():
    rng = _rng("interval")
    months, days, us = rng.integers(-100, 100, N), rng.integers(-1000, 1000, N), rng.integers(-10 ** 9, 10 ** 9, N)
    ok = _ok(rng)
    raw = b"".join(struct.pack("<iiq", int(m), int(d), int(u) * 1000 + (int(u) % 7 if u > 0 else -(int(-u) % 7))) if o else bytes(16) for m, d, u, o in zip(months, days, us, ok))
    stored = _masked([[int(m), int(d), int(u)] for m, d, u in zip(months, days, us)], ok)
    _add(Entry("interval", pa.month_day_nano_interval(), stored, _fixed(pa.month_day_nano_interval(), raw, ok), REFUSED, "INTERVAL"))


for _unit in ("s", "ms", "us", "ns"):
    _duration(_unit)
_interval()


# ------------------------------------------------------------------------------------------------ run-end encoded
def _runs(rng, n, run_end_type):
    """run ends of one record batch: runs of 1 .. 40 rows"""
    ends = np.cumsum(rng.integers(1, 40, n))
    ends = ends[ends < n].tolist() + [n]
    return ends, pa.array(ends, run_end_type)


def _ree(base, run_end_type, make_values):
    """base: the name of the flat entry whose values the runs take.  make_values(stored per run, ok per run) -> (values
    array, stored per run as the scan holds them)"""
    name = "ree_" + base
    src = next(e for e in MATRIX if e.name == base)
    rng = _rng(name)
    live = [v for v in src.stored if v is not None and not (isinstance(v, float) and not math.isfinite(v))]
    edges = [src.stored[r] for r in range(1, EDGE_ROWS, 2) if src.stored[r] is not None]    # (non-finite halves: in these runs alone)
    arrays, stored = [], []
    for b, n in enumerate(BATCHES):
        ends, run_ends = _runs(rng, n, run_end_type)
        per_run = [live[i] for i in rng.integers(0, len(live), len(ends))]
        if b == 0:
            per_run[1:2 * len(edges):2] = edges[: len(per_run[1:2 * len(edges):2])]
        ok = rng.random(len(ends)) >= 0.15
        ok[1:2 * len(edges):2] = True
        values = make_values(per_run, ok)
        arrays.append(pa.RunEndEncodedArray.from_arrays(run_ends, values))
        start = 0
        for end, v, o in zip(ends, per_run, ok):
            stored += [v if o else None] * (end - start)
            start = end
    assert len(stored) == N
    e = Entry(name, arrays[0].type, stored, arrays, src.cls, src.duck, file="ree", raw=src.raw)
    if src.canon is not src.stored:          # extension values: canon_column sees the storage
        back = {s: c for s, c in zip(src.stored, src.canon) if s is not None}
        if src.duck == "BOOLEAN":
            back = {0: 0, 1: 1}              # (the run values below are written as 0 / 1)
        e.canon = [None if v is None else back[v] for v in stored]
    if src.cls == STRING:
        e.canon = [None if v is None else v.decode() for v in stored]
    _add(e)


def _values_int(t, width):
    return lambda per_run, ok: _fixed(t, _le(per_run, width, ok), ok)


_ree("i16", pa.int16(), _values_int(pa.int16(), 2))
_ree("dec128_9", pa.int32(), _values_int(pa.decimal128(9, 2), 16))
_ree("ts_ns", pa.int64(), _values_int(pa.timestamp("ns"), 8))
_ree("f16", pa.int16(), lambda per_run, ok: _fixed(pa.float16(), np.where(ok, np.array(per_run, np.float16), np.float16(0)).astype(np.float16).tobytes(), ok))
_ree("bool8", pa.int32(), lambda per_run, ok: pa.ExtensionArray.from_storage(pa.bool8(), _fixed(pa.int8(), _le(per_run, 1, ok), ok)))
_ree("uuid", pa.int64(), lambda per_run, ok: pa.ExtensionArray.from_storage(
    pa.uuid(), _fixed(pa.binary(16), b"".join(next(e for e in MATRIX if e.name == "uuid").raw[v] if o else bytes(16) for v, o in zip(per_run, ok)), ok)))
_ree("str", pa.int16(), lambda per_run, ok: pa.array([v.decode() if o else None for v, o in zip(per_run, ok)], pa.string()))

BY_NAME = {e.name: e for e in MATRIX}
assert len(BY_NAME) == len(MATRIX)


# ------------------------------------------------------------------------------------------------ twins without NULLs
# Not matrix entries.  Under zero_copy_direct the planner aliases a column into the body only where the decode is a plain copy
# and the record batch holds no NULL, and unset_all_valid drops the validity words of such a batch: a matrix column, with its
# NULLs, reaches neither path.  One twin whose decode is a copy, one whose decode narrows (and so must NOT be aliased); few
# distinct values, so that both serve as K10 keys too.
def _twin(base, width):
    src = BY_NAME[base]
    rng = _rng(base + "/twin")
    pool = sorted({v for v in src.low.stored if v is not None})
    values = [pool[i] for i in rng.integers(0, len(pool), N)]
    data = pa.py_buffer(_le(values, width, [True] * N))
    e = Entry(base + "_nn", src.type, values, pa.Array.from_buffers(src.type, N, [None, data], null_count=0), src.cls, src.duck)
    e.low = e
    return e


TWINS = [_twin("dec64_18", 8), _twin("dec128_4", 16)]
BY_NAME.update({e.name: e for e in TWINS})
FINITE_FILTER = ("k", ">=", 800)                # behind the edge rows of the flat and of the run-end float entries
FINITE_ROWS = list(range(800, N))


# ------------------------------------------------------------------------------------------------ the files' other columns
def companions():
    """k: the row number; g: the int16 grouping column of 40 values with NULLs; p32 / pf: the second factor of SUM_PRODUCT for
    the integer and for the float class -> {name: (stored values, array)}"""
    rng = _rng("companions")
    out = {"k": (list(range(N)), pa.array(np.arange(N, dtype=np.int64)))}
    ok = rng.random(N) >= 0.1
    g = (rng.integers(0, 40, N) * 37 - 700).astype(np.int16)
    out["g"] = (_masked([int(v) for v in g], ok), pa.array(g, mask=~ok))
    ok = rng.random(N) >= 0.1
    p = rng.integers(-1000, 1000, N).astype(np.int32)
    out["p32"] = (_masked([int(v) for v in p], ok), pa.array(p, mask=~ok))
    ok = rng.random(N) >= 0.1
    f = (rng.integers(-64, 64, N) / 8.0).astype(np.float32)
    out["pf"] = (_masked([float(v) for v in f], ok), pa.array(f, mask=~ok))
    return out


def tables():
    """{file: (schema, [record batch, record batch])} and {column: stored values} over both files"""
    comp = companions()
    stored = {name: s for name, (s, _) in comp.items()}
    files = {}
    for file in ("main", "ree"):
        entries = [e for e in MATRIX if e.file == file]
        extra = [e.low for e in entries if e.low is not None and e.low is not e] + (TWINS if file == "main" else [])
        cols = [(n, [a.slice(0, BATCHES[0]), a.slice(BATCHES[0], BATCHES[1])]) for n, (_, a) in comp.items()] + [(e.name, e.chunks()) for e in entries + extra]
        schema = pa.schema([pa.field(n, c[0].type) for n, c in cols])
        files[file] = (schema, [pa.record_batch([c[b] for _, c in cols], schema=schema) for b in range(len(BATCHES))])
        for e in entries + extra:
            stored[e.name] = e.stored
    return files, stored


# ------------------------------------------------------------------------------------------------ the reference
def wrap128(v):
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _float_key(x):
    return (1, 0.0) if math.isnan(x) else (0, x + 0.0)


def term(spec, stored, r):
    """the value row r adds to a SUM / SUM_PRODUCT / SUM_EXPR, or None when a column of the spec is NULL in the row.
    sum_expr specs: ("sum_expr", (column, mul, add), constant)"""
    op = spec[0]
    if op == "sum_expr":
        (c, mul, add), const = spec[1], spec[2]
        v = stored[c][r]
        return None if v is None else (add + mul * v) * const
    vals = [stored[c][r] for c in spec[1:]]
    if any(v is None for v in vals):
        return None
    return vals[0] * vals[1] if op == "sum_product" else vals[0]


def expected(spec, stored, rows):
    """("exact", value) or ("sum", [float terms]) of one aggregate over `rows`"""
    op = spec[0]
    if op == "count_star":
        return "exact", len(rows)
    terms = [t for t in (term(spec, stored, r) for r in rows) if t is not None]
    if op == "count":
        return "exact", len(terms)
    if not terms:
        return "exact", None
    if isinstance(terms[0], float):
        if op in ("sum", "sum_product", "sum_expr"):
            return "sum", terms
        best = (min if op == "min" else max)(terms, key=_float_key)
        return "exact", float("nan") if math.isnan(best) else best + 0.0
    if op in ("sum", "sum_product", "sum_expr"):
        return "exact", wrap128(sum(terms))
    return "exact", (min if op == "min" else max)(terms)


def check(got, want, what):
    """test_gpu_scan_aggregate.py::check, and for terms that are not all finite the IEEE outcome, which no order changes:
    NaN when a term is NaN or both infinities occur, else the infinity"""
    kind, value = want
    if kind == "sum":
        print(what, "got", got, "over", len(value), "terms")
        assert isinstance(got, float), (what, got)
        if not all(math.isfinite(v) for v in value):
            if any(math.isnan(v) for v in value) or {v for v in value if math.isinf(v)} == {math.inf, -math.inf}:
                assert math.isnan(got), (what, got)
            else:
                assert got == next(v for v in value if math.isinf(v)), (what, got)
            return
        exact = math.fsum(value)
        bound = 2 * len(value) * 2.0 ** -53 * math.fsum(abs(v) for v in value)
        assert abs(got - exact) <= bound, (what, got, exact, bound)
    elif isinstance(value, float):
        assert isinstance(got, float) and bits(got) == (CANONICAL_NAN if math.isnan(value) else bits(value)), (what, got, value)
    else:
        assert got == value and (value is None or isinstance(got, (int, uuid.UUID))), (what, got, value)


def order_key(v):
    """ascending by stored value, NULLS LAST"""
    return (1, 0) if v is None else (0, v)


def expected_groups(key, specs, stored, rows):
    """[(stored key value, [expected(spec) per spec])] in the order the library returns the groups"""
    groups = {}
    for r in rows:
        groups.setdefault(stored[key][r], []).append(r)
    return [(k, [expected(sp, stored, groups[k]) for sp in specs]) for k in sorted(groups, key=order_key)]

"""The integer filter leaves at their edges: one table with a column for every Arrow type the scan stores as a fixed-width
integer (ArrowField::Plan + IsIntegerLike), the stored integers of every row in exact Python integers, an evaluator of
predicate trees over them, and the cases the host test and the GPU tests share.

The table holds the rows where leaf_compare<int8/16/32/64> and the host code in front of it (LeafOf, ToCnf, the range merge
of NormaliseFilter, the uint64 mapping of BoundFilter::Program) can go wrong: every type's stored minimum and maximum and
their neighbours, the uint64 values around 2^63 and 2^64, at the rows where a lane, a validity byte, a window or a workgroup
ends, in record batches whose row counts are no multiple of 8.  Nothing here touches the GPU or the library."""
import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc

P63, P64 = 1 << 63, 1 << 64
I64_MIN, I64_MAX = -P63, P63 - 1
DAY_MS = 86400000

# 8197: a second workgroup (4 windows each) whose first window has five rows and whose other three are absent; 2047: the last
# lane of the window keeps seven rows; an empty batch in the middle; one row; 4096: exactly two windows; 2049; 63
BATCH_ROWS = (8197, 2047, 0, 1, 4096, 2049, 63)
N_ROWS = sum(BATCH_ROWS)
EDGE_ROWS = (0, 7, 8, 63, 64, 2047, 2048)   # of the first batch: lane, validity-byte, word and window seams
NULL_FRACTION = 0.15
OPS = ("=", "<>", "<", "<=", ">", ">=")


def _edges(lo, hi):
    return [lo, lo + 1, -1, 0, 1, hi - 1, hi]


def _trunc_div(v, d):
    """C's integer division (towards zero), which the decode kernels use for date64 and ns -> us"""
    q = abs(v) // d
    return -q if v < 0 else q


class Column:
    """name, Arrow type, the seven source values of the edge pool, how a source value becomes the stored integer"""

    def __init__(self, name, arrow_type, source, stored, pool, convert=None, fill=(-3, 4), nullable=True):
        self.name, self.arrow_type, self.source, self.stored_dtype = name, arrow_type, source, np.dtype(stored)
        self.pool, self.convert, self.fill, self.nullable = list(pool), convert or (lambda v: v), fill, nullable
        self.is_u64 = self.stored_dtype == np.uint64

    @property
    def domain(self):
        """the least and greatest integer the stored type can hold"""
        if self.arrow_type == pa.bool_():
            return 0, 1
        info = np.iinfo(self.stored_dtype)
        return int(info.min), int(info.max)

    def twin(self):
        return Column(self.name + "_nn", self.arrow_type, self.source, self.stored_dtype, self.pool, self.convert, self.fill, nullable=False)


def _int(name, ty, dtype):
    info = np.iinfo(dtype)
    unsigned = info.min == 0
    pool = [0, 1, 2, info.max // 2, info.max // 2 + 1, info.max - 1, info.max] if unsigned else _edges(int(info.min), int(info.max))
    if dtype == np.uint64:
        pool = [0, 1, P63 - 1, P63, P63 + 1, P64 - 2, P64 - 1]
    return Column(name, ty, dtype, dtype, pool, fill=(0, 7) if unsigned else (-3, 4))


def _decimal(name, ty, stored):
    top = 10 ** ty.precision - 1
    source = {32: np.int32, 64: np.int64, 128: "dec128"}[ty.bit_width]
    return Column(name, ty, source, stored, _edges(-top, top))


def _has_small_decimals():
    return hasattr(pa, "decimal32") and hasattr(pa, "decimal64")


def columns():
    i32, i64 = np.iinfo(np.int32), np.iinfo(np.int64)
    i32e = _edges(int(i32.min), int(i32.max))
    i64e = _edges(int(i64.min), int(i64.max))
    mul = lambda f: (lambda v: v * f)
    fits = lambda f: _edges(-(I64_MAX // f), I64_MAX // f)   # sources whose product with f stays an int64 (MI_K_MUL_I64 checks)
    # date64: milliseconds -> days, truncated towards zero; the sources sit off the day boundaries on purpose
    date64 = [int(i32.min) * DAY_MS, (int(i32.min) + 1) * DAY_MS - 5, -DAY_MS - 7, -1, DAY_MS + 123, (int(i32.max) - 1) * DAY_MS + 1,
              int(i32.max) * DAY_MS + DAY_MS - 1]
    ns = [int(i64.min), int(i64.min) + 1, -1001, -999, 1999, int(i64.max) - 1, int(i64.max)]   # / 1000, towards zero
    cols = [
        _int("i8", pa.int8(), np.int8), _int("i16", pa.int16(), np.int16), _int("i32", pa.int32(), np.int32), _int("i64", pa.int64(), np.int64),
        _int("u8", pa.uint8(), np.uint8), _int("u16", pa.uint16(), np.uint16), _int("u32", pa.uint32(), np.uint32), _int("u64", pa.uint64(), np.uint64),
        Column("flag", pa.bool_(), np.uint8, np.uint8, [0, 1, 0, 0, 1, 0, 1], fill=(0, 2)),
        Column("date32", pa.date32(), np.int32, np.int32, i32e),
        Column("date64", pa.date64(), np.int64, np.int32, date64, lambda v: _trunc_div(v, DAY_MS), fill=(-3 * DAY_MS, 4 * DAY_MS)),
        Column("time32_s", pa.time32("s"), np.int32, np.int64, i32e, mul(1000000)),
        Column("time32_ms", pa.time32("ms"), np.int32, np.int64, i32e, mul(1000)),
        Column("time64_us", pa.time64("us"), np.int64, np.int64, i64e),
        Column("time64_ns", pa.time64("ns"), np.int64, np.int64, ns, lambda v: _trunc_div(v, 1000), fill=(-3000, 4000)),
        # with a time zone seconds and milliseconds are scaled to microseconds (MI_K_MUL_I64) and nanoseconds divided
        # (MI_K_DIV_I64); without one the stored value is the file's (MI_K_COPY)
        Column("ts_s_tz", pa.timestamp("s", tz="UTC"), np.int64, np.int64, fits(1000000), mul(1000000)),
        Column("ts_ms_tz", pa.timestamp("ms", tz="UTC"), np.int64, np.int64, fits(1000), mul(1000)),
        Column("ts_us", pa.timestamp("us"), np.int64, np.int64, i64e),
        Column("ts_ns_tz", pa.timestamp("ns", tz="UTC"), np.int64, np.int64, ns, lambda v: _trunc_div(v, 1000), fill=(-3000, 4000)),
        Column("ts_s", pa.timestamp("s"), np.int64, np.int64, i64e),
        _decimal("dec128_4", pa.decimal128(4, 0), np.int16), _decimal("dec128_9", pa.decimal128(9, 2), np.int32),
        _decimal("dec128_18", pa.decimal128(18, 3), np.int64),
    ]
    if _has_small_decimals():
        cols += [_decimal("dec32_4", pa.decimal32(4, 1), np.int16), _decimal("dec32_9", pa.decimal32(9, 2), np.int32),
                 _decimal("dec64_9", pa.decimal64(9, 0), np.int32), _decimal("dec64_18", pa.decimal64(18, 3), np.int64)]
    twins = [c.twin() for c in cols if c.name in ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "date32", "dec128_9")]
    return cols + twins


def filter_column_names():
    """every column but `k`, without building the table (for parametrising)"""
    return [c.name for c in columns()]


def _pack_bits(ok):
    return np.packbits(np.concatenate([ok, np.zeros((-len(ok)) % 8, bool)]), bitorder="little")


def validity_words(ok):
    """the validity words of a DuckDB vector (bits past the last row set)"""
    n = len(ok)
    return np.packbits(np.concatenate([ok, np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()


def _arrow_array(col, source, ok):
    n = len(source)
    if col.arrow_type == pa.bool_():
        return pa.array(np.array(source, bool), mask=None if ok.all() else ~ok)
    if col.source == "dec128":
        data = np.array([[v & (P64 - 1), (v >> 64) & (P64 - 1)] for v in source], np.uint64)
    else:
        data = np.array(source, col.source)
    validity = None if ok.all() else pa.py_buffer(_pack_bits(ok).tobytes())
    return pa.Array.from_buffers(col.arrow_type, n, [validity, pa.py_buffer(data.tobytes())], null_count=int((~ok).sum()))


class Fixture:
    """the table, and per column the stored integers (numpy, of the stored type; made from Python integers) and valid mask"""

    def __init__(self, seed=20240607):
        rng = np.random.default_rng(seed)
        self.columns = {c.name: c for c in columns()}
        self.batch_offsets = [int(x) for x in np.concatenate([[0], np.cumsum(BATCH_ROWS)])]
        forced = {}   # row -> index into the pool
        for i, r in enumerate(EDGE_ROWS):
            forced[r] = i
        for b, rows in enumerate(BATCH_ROWS):
            if rows:
                forced[self.batch_offsets[b] + rows - 1] = 6 - b % 7   # the maximum closes the five-row window of the first batch
        self.forced = forced
        arrays, self.stored, self.valid, self.source = [], {}, {}, {}
        for c in self.columns.values():
            pick = rng.integers(0, 7, N_ROWS)
            near = rng.integers(c.fill[0], c.fill[1], N_ROWS)
            from_pool = rng.random(N_ROWS) < 0.5
            if c.is_u64:   # the narrow range sits at 0 and at 2^63
                src = [c.pool[int(p)] if f else (int(v) if v % 2 else P63 + int(v)) for p, v, f in zip(pick, near, from_pool)]
            else:
                src = [c.pool[int(p)] if f else int(v) for p, v, f in zip(pick, near, from_pool)]
            ok = rng.random(N_ROWS) >= NULL_FRACTION if c.nullable else np.ones(N_ROWS, bool)
            for r, i in forced.items():
                src[r] = c.pool[i]
                ok[r] = True
            stored = [c.convert(v) for v in src]
            lo, hi = c.domain
            assert all(lo <= v <= hi for v in stored), c.name
            self.source[c.name] = src
            self.stored[c.name] = np.array(stored, c.stored_dtype)
            assert [int(v) for v in self.stored[c.name][:64]] == stored[:64]
            self.valid[c.name] = ok
            arrays.append(_arrow_array(c, src, ok))
        self.columns["k"] = Column("k", pa.int64(), np.int64, np.int64, [0] * 7, nullable=False)
        self.stored["k"] = np.arange(N_ROWS, dtype=np.int64)
        self.valid["k"] = np.ones(N_ROWS, bool)
        arrays.append(pa.array(self.stored["k"]))
        self.names = list(self.columns)
        self.batch = pa.record_batch(arrays, names=self.names)

    def filter_columns(self):
        return [n for n in self.names if n != "k"]

    def write(self, path):
        """one IPC stream, record batches of BATCH_ROWS rows"""
        with ipc.new_stream(path, self.batch.schema) as w:
            for off, rows in zip(self.batch_offsets, BATCH_ROWS):
                w.write_batch(self.batch.slice(off, rows))
        return path

    def pool(self, name):
        """the stored values of the column's edge pool"""
        c = self.columns[name]
        return [c.convert(v) for v in c.pool]

    def oracle_columns(self, names):
        """{name: (stored integers, validity words)} as oracle.pyoracle.filter_cnf takes them"""
        return {n: (self.stored[n], validity_words(self.valid[n])) for n in names}


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture


# ---------------------------------------------------------------------------------------------------- the evaluator
def compare(values, op, c):
    """values <op> c, exactly: `values` holds int64-representable or uint64 integers, `c` is any Python integer"""
    if values.dtype != np.uint64:
        values = values.astype(np.int64)
    info = np.iinfo(values.dtype)
    if c < int(info.min) or c > int(info.max):   # a constant no value can reach: the comparison does not depend on the row
        below = c < int(info.min)
        const = {"=": False, "<>": True, "<": not below, "<=": not below, ">": below, ">=": below}[op]
        return np.full(len(values), const)
    cc = values.dtype.type(c)
    return {"=": values == cc, "<>": values != cc, "<": values < cc, "<=": values <= cc, ">": values > cc, ">=": values >= cc}[op]


def is_leaf(expr):
    return not (expr[0] in ("and", "or") and len(expr) > 1 and isinstance(expr[1], tuple))


def evaluate(fx, expr):
    """the rows `expr` keeps (a boolean mask), SQL semantics: a comparison with NULL is not true"""
    if not is_leaf(expr):
        parts = [evaluate(fx, e) for e in expr[1:]]
        out = parts[0].copy()
        for p in parts[1:]:
            out = (out & p) if expr[0] == "and" else (out | p)
        return out
    name, op = expr[0], expr[1].lower()
    ok = fx.valid[name]
    if op == "is null":
        return ~ok
    if op == "is not null":
        return ok.copy()
    if op == "in":
        m = np.zeros(N_ROWS, bool)
        for c in set(expr[2]):
            m |= compare(fx.stored[name], "=", c)
        return m & ok
    return compare(fx.stored[name], op, expr[2]) & ok


def cnf_of(expr):
    """AND-of-ORs of leaves when `expr` is written that way already, else None"""
    if is_leaf(expr):
        return [[expr]]
    if expr[0] == "or":
        return [list(expr[1:])] if all(is_leaf(e) for e in expr[1:]) else None
    out = []
    for e in expr[1:]:
        if is_leaf(e):
            out.append([e])
        elif e[0] == "or" and all(is_leaf(x) for x in e[1:]):
            out.append(list(e[1:]))
        elif e[0] == "and":
            sub = cnf_of(e)
            if sub is None:
                return None
            out.extend(sub)
        else:
            return None
    return out


def cnf_size(expr):
    """(clauses, leaves) of `expr` in conjunctive normal form before any merging: AND adds its children, OR takes one clause
    of every child per clause -- the clause counts multiply, the leaves of the chosen clauses are concatenated"""
    if is_leaf(expr):
        return 1, 1
    kids = [cnf_size(e) for e in expr[1:]]
    if expr[0] == "and":
        return sum(c for c, _ in kids), sum(l for _, l in kids)
    clauses = 1
    for c, _ in kids:
        clauses *= c
    return clauses, sum(l * (clauses // c) for c, l in kids)


def needs_distribution(expr):
    """an OR above an AND"""
    if is_leaf(expr):
        return False
    if expr[0] == "or" and any(not is_leaf(e) and e[0] == "and" for e in expr[1:]):
        return True
    return any(needs_distribution(e) for e in expr[1:])


# ---------------------------------------------------------------------------------------------------- the cases
def edge_constants(fx, name):
    """What section `every op at every edge` asks for, sorted: the stored type's minimum - 1 .. maximum + 1, -1, 0, 1, the int64
    ends, and the column's own edge pool (which differs from the type's ends on scaled and decimal columns); those that fit an
    int64 (larger ones travel as 128-bit constants, which narrow columns refuse)."""
    lo, hi = fx.columns[name].domain
    cs = {lo - 1, lo, lo + 1, -1, 0, 1, hi - 1, hi, hi + 1, I64_MIN, I64_MAX}
    cs.update(fx.pool(name))
    if fx.columns[name].is_u64:
        cs.update([-2, -5, I64_MIN + 1])
    return sorted(c for c in cs if I64_MIN <= c <= I64_MAX)


def single_leaf_cases(fx, name):
    out = [(name, op, c) for op in OPS for c in edge_constants(fx, name)]
    return out + [(name, "is null"), (name, "is not null")]


def in_list_cases(fx):
    cases = []
    for name in ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "i64_nn", "u64_nn", "dec128_4", "date64", "ts_s_tz"):
        lo, hi = fx.columns[name].domain
        pool = [min(c, I64_MAX) for c in fx.pool(name)]
        cases += [(name, "in", []), (name, "in", [pool[6]]), (name, "in", [pool[0]]),
                  (name, "in", [pool[6], pool[0], pool[6], 1, 0, 1, pool[3]]),            # duplicates, unsorted
                  (name, "in", [c for c in (hi + 1, lo - 1, 0) if I64_MIN <= c <= I64_MAX] + [pool[5]])]   # outside the domain
    for name in ("u8", "u16", "u32", "u64", "u64_nn"):
        hi = fx.columns[name].domain[1]
        cases += [(name, "in", [-1, 5]), (name, "in", [-1, -2]), (name, "in", [-1]), (name, "in", [-hi - 1 if hi < I64_MAX else I64_MIN, -1, 1, hi if hi <= I64_MAX else I64_MAX]),
                  (name, "in", [I64_MIN, I64_MAX, 0])]
    # exactly 256 distinct values, the pool's among them
    for name in ("i16", "u64", "i64"):
        pool = [c for c in fx.pool(name) if I64_MIN <= c <= I64_MAX]
        vals = list(dict.fromkeys(pool + list(range(-120, 400))))[:256]
        assert len(set(vals)) == 256
        cases.append((name, "in", vals[::-1]))
    return cases


def too_long_in_list():
    return ("i32", "in", list(range(257)))


def merge_cases(fx):
    """the range merge of NormaliseFilter: conjuncts on one column that fold into one leaf, and those that must not"""
    cases = []
    for name in ("i8", "i32", "i64", "u8", "u16", "u32", "u64", "u64_nn", "date64", "dec128_18"):
        p = [min(c, I64_MAX) for c in fx.pool(name)]   # (a uint64 constant past INT64_MAX travels as 128 bits and is refused)
        cases += [
            ("and", (name, ">=", -1), (name, "<", p[6]), (name, ">=", 0), (name, "<=", p[5])),
            ("and", (name, ">=", p[0]), (name, "<", p[1]), (name, ">=", p[0]), (name, "<=", p[6])),
            ("and", (name, "<", 5), (name, ">", 10)),                                      # a contradiction
            ("and", (name, "<", I64_MIN), (name, "<=", 1)),
            ("and", (name, ">=", 0), (name, "<", I64_MIN)),
            ("and", (name, ">", I64_MAX), (name, ">=", 0)),
            ("and", (name, ">=", 0), (name, ">", I64_MAX)),
            ("and", (name, ">", I64_MAX), (name, "<", 5)),
            ("and", (name, ">", I64_MAX), (name, ">", I64_MAX)),
            ("and", (name, "<>", 5), (name, ">=", 3)),                                     # a negated leaf is no range
            ("and", (name, "<>", I64_MAX), (name, ">", I64_MAX - 1)),
            ("or", (name, "<", 1), (name, ">", 1)),                                        # two ranges under an OR
            ("or", ("and", (name, ">=", 0), (name, "<=", 1)), ("and", (name, ">", I64_MAX - 1), (name, "<=", I64_MAX))),
            ("or", (name, ">", I64_MAX), (name, "<", 1)),
            ("and", ("or", (name, ">", I64_MAX), (name, "=", 0)), (name, "<=", 0)),
        ]
    for name in ("u64", "u64_nn"):
        cases += [
            ("and", (name, ">", -5), (name, "<", 10)),
            ("and", (name, ">=", 0), (name, "<", -1)),                                     # zero rows
            ("and", (name, ">", I64_MAX), (name, ">=", 5)),
            ("and", (name, ">=", 5), (name, ">", I64_MAX)),
            ("and", (name, ">=", I64_MAX), (name, "<=", I64_MAX)),
            ("and", (name, ">", I64_MAX), ("i8", ">=", 0)),
            ("and", (name, ">", -1), (name, "<=", I64_MAX)),
        ]
    return cases


def _random_leaf(fx, rng, names):
    name = names[int(rng.integers(len(names)))]
    pool = [c for c in fx.pool(name) if I64_MIN <= c <= I64_MAX]
    near = pool + [c + d for c in pool for d in (-1, 1) if I64_MIN <= c + d <= I64_MAX] + [-2, 2, 3, I64_MIN, I64_MAX]
    form = int(rng.integers(10))
    if form < 6:
        return (name, OPS[form], near[int(rng.integers(len(near)))])
    if form == 6:
        return (name, "is null")
    if form == 7:
        return (name, "is not null")
    k = int(rng.integers(0, 5))
    return (name, "in", [near[int(i)] for i in rng.integers(0, len(near), k)])


def _random_tree(fx, rng, names, depth):
    if depth == 0 or rng.random() < 0.25:
        return _random_leaf(fx, rng, names)
    op = "and" if rng.random() < 0.5 else "or"
    return (op,) + tuple(_random_tree(fx, rng, names, depth - 1) for _ in range(int(rng.integers(2, 4))))


def generated_trees(fx, seed=7, want=44, want_distributed=12):
    """AND / OR trees of depth <= 3 with every leaf form, kept when their conjunctive normal form has at most 24 leaves"""
    rng = np.random.default_rng(seed)
    names = fx.filter_columns()
    trees, distributed = [], 0
    while len(trees) < want or distributed < want_distributed:
        t = _random_tree(fx, rng, names, 3)
        if is_leaf(t) or cnf_size(t)[1] > 24:
            continue
        d = needs_distribution(t)
        if len(trees) >= want and not d:
            continue
        trees.append(t)
        distributed += d
    return trees


def refused_trees():
    """trees whose distribution into conjunctive normal form passes 96 leaves"""
    a = lambda col, i: ("and", (col, ">", i), (col, "<", i + 3), ("i8", "<>", i))
    return [
        ("or",) + tuple(a("i32", i) for i in range(5)),                                    # 3^5 clauses of 5 leaves
        ("and", ("i64", ">=", 0), ("or",) + tuple(a("u64", i) for i in range(4)) + (("u8", "=", 1),)),
        ("or", ("and",) + tuple(("or", ("i16", "=", i), ("u16", "=", i)) for i in range(10)),
         ("and",) + tuple(("or", ("i16", "=", -i), ("u32", "=", i)) for i in range(10))),   # 100 clauses of 4 leaves
    ]


def delivery_cases(fx):
    """about ten of the expressions above for the ways a chunk is delivered: one per width, uint64, negated, IN, a tree"""
    return [
        ("i8", ">=", -1), ("i16_nn", "<", 1), ("u32", ">", 1), ("i64", "<=", 0),
        ("u64", ">", I64_MAX), ("u64_nn", ">=", 1), ("i32_nn", "<>", 0), ("u16", "in", [0, 1, 65535, -1]),
        ("u64", "in", [-1, 5, 0, I64_MAX]), ("date64", "is null"),
        ("or", ("and", ("i8_nn", ">", 0), ("u64", ">", I64_MAX)), ("and", ("dec128_9", "<=", 0), ("ts_ns_tz", "is not null")), ("flag", "=", 1)),
    ]

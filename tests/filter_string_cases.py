"""The string filter leaves at their edges: a pool of byte strings built from families, three files whose columns hold it
(plain VARCHAR / BLOB columns, dictionary-encoded ones, run-end encoded ones), an evaluator of predicate trees over Python
bytes, a packer of DuckDB string_t vectors, and the cases the host test and the GPU tests share.

The pool holds the values where leaf_strin, strrow_compare (kLeafStrRange), leaf_dictmap and the host code in front of them
(LeafOf's prefix successor, DictMatchMap, the heap binding of BoundFilter::Program) can go wrong: bytes 0x00, 0x7F, 0x80 and 0xFF
behind a shared prefix that ends at every dword and on either side of the 12-byte inline limit, a value and the same value
with a zero byte behind it, long values that differ in their last 1 .. 4 bytes only, and values of nothing but 0xFF.
Nothing here touches the GPU or the library."""
import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc

BATCH_ROWS = (8197, 2047, 0, 1, 4096, 2049, 63)   # the integer cases' cut (filter_integer_cases.BATCH_ROWS)
N_ROWS = sum(BATCH_ROWS)
EDGE_ROWS = (0, 7, 8, 63, 64, 2047, 2048, 4095, 4096, 8191, 8192, 8196)   # of the first batch: lane, byte, word, window, workgroup seams
NULL_FRACTION = 0.10
OPS = ("=", "<>", "<", "<=", ">", ">=", "starts_with")
RANGE_OPS = ("<", "<=", ">", ">=")

# ---------------------------------------------------------------------------------------------------- the pool
LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14, 16, 17, 31, 32, 33, 64, 300)
SIBLING_PREFIXES = (0, 1, 3, 4, 5, 7, 8, 11, 12, 13, 16)
BASE = b"kjihgfedcbaZYXWVUTSR"                     # the shared prefixes are nested: family 4 is a prefix of family 5, ...
BINARY_TAILS = (b"", b"\x00", b"\x01", b"\x7f", b"\x80", b"\xff", b"\xff\x00")
# utf8 columns hold valid text: U+0080, U+10FFFF and U+07FF stand in for the bytes 0x80 and 0xFF (their first byte is >= 0xC2,
# so a signed comparison still puts them below 0x7F)
TEXT_TAILS = (b"", b"\x00", b"\x01", b"\x7f", "\u0080".encode(), "\U0010ffff".encode(), "\u07ff\x00".encode())
TAIL_LENGTHS = (13, 14, 15, 16, 17, 20)
FF_LENGTHS = (1, 4, 12, 13)
UTF8_TEXT = ["é", "été", "€uro", "\U0001d11eclef", "naïve café", "日本語のテキスト",
             "kjihé", "kjihgfedcbaé", "kjihgfedcbaZ\U0001d11e"]


def _of_length(n):
    head = b"L%03d:" % n
    return (head + bytes(97 + (i * 7 + n) % 26 for i in range(n)))[:n]


def _tail_family(n):
    """a value of n bytes and four that share its first n - j bytes (j = 1 .. 4) and differ in byte n - j alone"""
    a = (b"tail%02d-" % n + bytes(65 + (i * 5 + n) % 26 for i in range(n)))[:n]
    return [a] + [a[: n - j] + b"~" + a[n - j + 1:] for j in (1, 2, 3, 4)]


def families(text):
    """{family: [values]}: `text` leaves out what is no valid UTF-8 (and takes TEXT_TAILS for the sibling families)"""
    out = {"lengths": [_of_length(n) for n in LENGTHS]}
    for k in SIBLING_PREFIXES:
        out["siblings%d" % k] = [BASE[:k] + t for t in (TEXT_TAILS if text else BINARY_TAILS)]
    for n in TAIL_LENGTHS:
        out["tail%d" % n] = _tail_family(n)
    if not text:
        out["all_ff"] = [b"\xff" * n for n in FF_LENGTHS]
    out["utf8"] = [s.encode() for s in UTF8_TEXT]
    return out


def pool(text):
    """the distinct values of every family, in family order"""
    return list(dict.fromkeys(v for vs in families(text).values() for v in vs))


def thin_families(text):
    """a pool of at most 100 values for dictionaries with 8-bit indices: four sibling families, two tail families, both seams"""
    full = families(text)
    keep = ["siblings0", "siblings4", "siblings12", "siblings13", "tail13", "tail17", "utf8"] + ([] if text else ["all_ff"])
    out = {f: full[f] for f in keep}
    out["lengths"] = [_of_length(n) for n in (0, 1, 4, 12, 13, 300)]
    return out


def successor(v):
    """the least byte string above v"""
    return v + b"\x00"


def predecessor(v):
    """a byte string below v with no pool value in between: v without its last zero byte, else v's last byte decremented
    and 0xFF 0xFF behind it (the empty string has none)"""
    if not v:
        return None
    if v[-1] == 0:
        return v[:-1]
    return v[:-1] + bytes([v[-1] - 1]) + b"\xff\xff"


def prefix_successor(p):
    """the exclusive upper end of the strings that begin with p (None: no upper end), as LeafOf builds it"""
    p = p.rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


# ---------------------------------------------------------------------------------------------------- the string_t packer
def validity_words(ok):
    """the validity words of a DuckDB vector (bits past the last row set)"""
    n = len(ok)
    return np.packbits(np.concatenate([np.asarray(ok, bool), np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()


FAR_BASE = 0xFEDCBA9876543211
LAYOUTS = {"arrow": ("arrow", 0x10000), "shuffled": ("shuffled", 0x7008), "far_base": ("shuffled", FAR_BASE)}


def pack_string_t(values, ptr_base, layout, seed=5):
    """DuckDB string_t rows of `values` (None = NULL) -> (images uint8[n, 16], heap uint8[], validity words).
    A value of <= 12 bytes sits inline, zero padded; a longer one holds its length, its first four bytes and ptr_base + its
    offset in the heap.  A NULL row is sixteen zero bytes: the kernel may follow the pointer of any row, valid or not.
    layout "arrow": the heap is Arrow's data buffer, every valid value in row order, inline ones included.
    layout "shuffled": long values only, in another order than the rows, with gaps of 0 .. 7 bytes of 0xA5 in front of each so
    that they begin at every address modulo 8, and 0xA5 at both ends of the heap.
    Every pointer lies in [ptr_base, ptr_base + len(heap) - length]."""
    n = len(values)
    images = np.zeros((n, 16), np.uint8)
    offsets = {}
    if layout == "arrow":
        heap, at = [], 0
        for i, v in enumerate(values):
            if v is not None:
                offsets[i] = at
                heap.append(v)
                at += len(v)
        heap = b"".join(heap)
    elif layout == "shuffled":
        rng = np.random.default_rng(seed)
        long_rows = [i for i, v in enumerate(values) if v is not None and len(v) > 12]
        heap = bytearray(b"\xa5" * 8)
        for j, i in enumerate(rng.permutation(len(long_rows))):
            row = long_rows[int(i)]
            heap += b"\xa5" * ((j % 8 - len(heap)) % 8 if j < 64 else int(rng.integers(0, 8)))   # the first 64: every residue
            offsets[row] = len(heap)
            heap += values[row]
        heap += b"\xa5" * 8
        heap = bytes(heap)
    else:
        raise ValueError(layout)
    for i, v in enumerate(values):
        if v is None:
            continue
        images[i, 0:4] = np.frombuffer(np.uint32(len(v)).tobytes(), np.uint8)
        if len(v) <= 12:
            images[i, 4: 4 + len(v)] = np.frombuffer(v, np.uint8)
        else:
            images[i, 4:8] = np.frombuffer(v[:4], np.uint8)
            images[i, 8:16] = np.frombuffer(np.uint64(ptr_base + offsets[i]).tobytes(), np.uint8)
            assert 0 <= offsets[i] and offsets[i] + len(v) <= len(heap)
    ok = np.array([v is not None for v in values], bool)
    return images, np.frombuffer(heap, np.uint8).copy() if heap else np.zeros(0, np.uint8), validity_words(ok)


# ---------------------------------------------------------------------------------------------------- the table
class Column:
    """name, kind ("plain" / "dict" / "ree"), the families its rows are drawn from, the row values (bytes or None) and, per
    record batch, the Arrow array"""

    def __init__(self, name, kind, arrow_type, fams, text):
        self.name, self.kind, self.arrow_type, self.families, self.text = name, kind, arrow_type, fams, text
        self.pool = list(dict.fromkeys(v for vs in fams.values() for v in vs))
        self.values, self.arrays = [], []

    def index(self):
        """distinct row values (sorted) and per row the index of its value, -1 for NULL"""
        return index_values(self.values)


def _width_families(text, width):
    fams = {f: [v for v in vs if len(v) == width] for f, vs in families(text).items()}
    return {f: vs for f, vs in fams.items() if vs}


def _draw(rng, pool_values, rows, null_fraction=NULL_FRACTION, sticky=0.0):
    """`rows` values from the pool, about null_fraction NULLs; `sticky`: the chance that a row repeats the one before (runs)"""
    out = []
    for i in range(rows):
        if out and rng.random() < sticky:
            out.append(out[-1])
        elif rng.random() < null_fraction:
            out.append(None)
        else:
            out.append(pool_values[int(rng.integers(len(pool_values)))])
    return out


def _force_seams(values, pool_values, batch_offsets, start=0):
    """pool values, one after the other, at the seam rows of the first batch and at the first and last row of every batch"""
    rows = list(EDGE_ROWS)
    for b, n in enumerate(BATCH_ROWS):
        if n:
            rows += [batch_offsets[b], batch_offsets[b] + n - 1]
    for j, r in enumerate(dict.fromkeys(rows)):
        values[r] = pool_values[(start + j) % len(pool_values)]
    return rows


def _plain_array(values, ty):
    return pa.array(values, ty)


def _ree_array(values, run_end_type, value_type):
    ends, vals = [], []
    for i, v in enumerate(values):
        if vals and vals[-1] == v:
            ends[-1] = i + 1
        else:
            ends.append(i + 1)
            vals.append(v)
    as_text = [None if v is None else v.decode() for v in vals]
    return pa.RunEndEncodedArray.from_arrays(pa.array(ends, run_end_type), pa.array(as_text, value_type))


DICT_INDEX_TYPES = (pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64())
DICT_VALUE_TYPES = (pa.utf8(), pa.large_utf8(), pa.binary(), pa.binary(13))


def _is_text(ty):
    return ty in (pa.utf8(), pa.large_utf8())


def _dict_array(rng, entries, rows, index_type, value_type, used, seam_start, null_index_fraction=0.05):
    """`rows` indices into `entries` (None = a NULL entry) among the entries `used`; -> (array, row values)"""
    idx = [None if rng.random() < null_index_fraction else used[int(rng.integers(len(used)))] for _ in range(rows)]
    for j, r in enumerate(r for r in (0, 7, 8, 63, 64, rows - 1) if 0 <= r < rows):
        idx[r] = used[(seam_start + j) % len(used)]
    values = [None if i is None else entries[i] for i in idx]
    as_arrow = [None if v is None else (v.decode() if _is_text(value_type) else v) for v in entries]
    arr = pa.DictionaryArray.from_arrays(pa.array(idx, index_type), pa.array(as_arrow, value_type))
    return arr, values


class Fixture:
    """Three groups of columns over the same N_ROWS rows and record batches, each written to a file of its own (`k` = the row
    number and `q` = an int32 column ride in each): "plain", "dict" and "ree"."""

    def __init__(self, seed=20250311):
        rng = np.random.default_rng(seed)
        self.batch_offsets = [int(x) for x in np.concatenate([[0], np.cumsum(BATCH_ROWS)])]
        self.k = np.arange(N_ROWS, dtype=np.int64)
        self.q = rng.integers(-5, 50, N_ROWS).astype(np.int32)
        self.q_valid = rng.random(N_ROWS) >= NULL_FRACTION
        self.columns = {}
        # ---- plain
        plain = [("utf8", pa.utf8(), families(True), True), ("large_utf8", pa.large_utf8(), families(True), True),
                 ("binary", pa.binary(), families(False), False), ("large_binary", pa.large_binary(), families(False), False)]
        plain += [("fsb%d" % w, pa.binary(w), _width_families(False, w), False) for w in (1, 4, 12, 13, 16)]
        for j, (name, ty, fams, text) in enumerate(plain):
            c = Column(name, "plain", ty, fams, text)
            c.values = _draw(rng, c.pool, N_ROWS)
            self.seam_rows = _force_seams(c.values, c.pool, self.batch_offsets, start=5 * j)
            as_arrow = [None if v is None else (v.decode() if text else v) for v in c.values]
            c.arrays = [_plain_array(as_arrow[o: o + n], ty) for o, n in zip(self.batch_offsets, BATCH_ROWS)]
            self.columns[name] = c
        # ---- run-end encoded
        for j, (ret, vt) in enumerate([(pa.int16(), pa.utf8()), (pa.int32(), pa.large_utf8()), (pa.int64(), pa.utf8()), (pa.int32(), pa.utf8())]):
            name = "ree_%s_%s" % (ret, "large_utf8" if vt == pa.large_utf8() else "utf8")
            c = Column(name, "ree", pa.run_end_encoded(ret, vt), families(True), True)
            c.values = _draw(rng, c.pool, N_ROWS, sticky=0.7)
            _force_seams(c.values, c.pool, self.batch_offsets, start=11 * j)
            c.arrays = [_ree_array(c.values[o: o + n], ret, vt) for o, n in zip(self.batch_offsets, BATCH_ROWS)]
            self.columns[name] = c
        # ---- dictionary-encoded: one column per index type (the value types take turns), then the special ones
        for j, it in enumerate(DICT_INDEX_TYPES):
            vt = DICT_VALUE_TYPES[j % 4]
            fams = thin_families(_is_text(vt))
            if vt == pa.binary(13):
                fams = _width_families(False, 13)
            name = "dict_%s_%s" % (it, {pa.utf8(): "utf8", pa.large_utf8(): "large_utf8", pa.binary(): "binary"}.get(vt, "fsb13"))
            c = Column(name, "dict", pa.dictionary(it, vt), fams, _is_text(vt))
            # one dictionary for the whole file: a NULL entry in the middle, the last three entries never referenced
            entries = c.pool[: len(c.pool) // 2] + [None] + c.pool[len(c.pool) // 2:]
            assert len(entries) <= 127
            used = list(range(len(entries) - 3))
            for b, n in enumerate(BATCH_ROWS):
                arr, vals = _dict_array(rng, entries, n, it, vt, used, seam_start=7 * b + j)
                c.arrays.append(arr)
                c.values += vals
            self.columns[name] = c
        thin_b, thin_t = thin_families(False), thin_families(True)
        # replaced: every batch brings another order and another subset of the entries
        c = Column("dict_replaced", "dict", pa.dictionary(pa.int16(), pa.binary()), thin_b, False)
        for b, n in enumerate(BATCH_ROWS):
            order = [c.pool[int(i)] for i in rng.permutation(len(c.pool))][: 20 + 9 * b]
            entries = order[:5] + [None] + order[5:]
            arr, vals = _dict_array(rng, entries, n, pa.int16(), pa.binary(), list(range(len(entries))), seam_start=b)
            c.arrays.append(arr)
            c.values += vals
        self.columns[c.name] = c
        # delta: every batch's dictionary is the one before with more entries behind it
        c = Column("dict_delta", "dict", pa.dictionary(pa.int32(), pa.utf8()), thin_t, True)
        grown = [c.pool[int(i)] for i in rng.permutation(len(c.pool))]
        for b, n in enumerate(BATCH_ROWS):
            entries = grown[: min(12 + 8 * b, len(grown))]
            arr, vals = _dict_array(rng, entries, n, pa.int32(), pa.utf8(), list(range(len(entries))), seam_start=3 * b)
            c.arrays.append(arr)
            c.values += vals
        self.columns[c.name] = c
        # empty: no entry at all, every row NULL through its index
        c = Column("dict_empty", "dict", pa.dictionary(pa.int8(), pa.utf8()), {}, True)
        for n in BATCH_ROWS:
            c.arrays.append(pa.DictionaryArray.from_arrays(pa.array([None] * n, pa.int8()), pa.array([], pa.utf8())))
            c.values += [None] * n
        self.columns[c.name] = c
        # 300 entries: the whole pool and fillers, two NULL entries, a fifth of the entries never referenced
        fams = dict(families(False))
        fams["fillers"] = [b"filler-%03d-%s" % (i, b"x" * (i % 9)) for i in range(300 - 2 - len(pool(False)))]
        c = Column("dict_300", "dict", pa.dictionary(pa.uint16(), pa.binary()), fams, False)
        entries = c.pool[:100] + [None] + c.pool[100:] + [None]
        assert len(entries) == 300
        used = [i for i in range(300) if i % 5 != 4 or entries[i] is None]
        for b, n in enumerate(BATCH_ROWS):
            arr, vals = _dict_array(rng, entries, n, pa.uint16(), pa.binary(), used, seam_start=31 * b)
            c.arrays.append(arr)
            c.values += vals
        self.columns[c.name] = c
        for c in self.columns.values():
            assert len(c.values) == N_ROWS and len(c.arrays) == len(BATCH_ROWS), c.name
        self._index = {}

    # ---- what the tests ask for
    def names(self, kind=None):
        return [n for n, c in self.columns.items() if kind is None or c.kind == kind]

    def index(self, name):
        if name not in self._index:
            self._index[name] = self.columns[name].index()
        return self._index[name]

    def write(self, path, kind, compression=None, names=None):
        """one IPC stream of the columns of `kind` (or `names`), k and q, in record batches of BATCH_ROWS rows; dictionaries
        travel as deltas where they can.  Returns the writer's statistics."""
        cols = [self.columns[n] for n in (names if names is not None else self.names(kind))]
        schema = pa.schema([pa.field("k", pa.int64())] + [pa.field(c.name, c.arrow_type) for c in cols] + [pa.field("q", pa.int32())])
        options = ipc.IpcWriteOptions(compression=compression, emit_dictionary_deltas=True)
        with ipc.new_stream(path, schema, options=options) as w:
            for b, (o, n) in enumerate(zip(self.batch_offsets, BATCH_ROWS)):
                q = pa.array(self.q[o: o + n], mask=~self.q_valid[o: o + n])
                w.write_batch(pa.record_batch([pa.array(self.k[o: o + n])] + [c.arrays[b] for c in cols] + [q], schema=schema))
        return w.stats


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = Fixture()
    return _fixture


COLUMN_KINDS = {"plain": ["utf8", "large_utf8", "binary", "large_binary", "fsb1", "fsb4", "fsb12", "fsb13", "fsb16"],
                "ree": ["ree_int16_utf8", "ree_int32_large_utf8", "ree_int64_utf8", "ree_int32_utf8"],
                "dict": ["dict_int8_utf8", "dict_uint8_large_utf8", "dict_int16_binary", "dict_uint16_fsb13", "dict_int32_utf8",
                         "dict_uint32_large_utf8", "dict_int64_binary", "dict_uint64_fsb13", "dict_replaced", "dict_delta", "dict_empty",
                         "dict_300"]}


def kind_of(name):
    return [k for k, names in COLUMN_KINDS.items() if name in names][0]


# ---------------------------------------------------------------------------------------------------- the evaluator
def compare(v, op, c):
    """does the byte string v pass `op` with the constant c: byte-wise order, a proper prefix first (Python's bytes order)"""
    if op == "starts_with":
        return v.startswith(c)
    if op == "not starts_with":
        return not v.startswith(c)
    return {"=": v == c, "<>": v != c, "<": v < c, "<=": v <= c, ">": v > c, ">=": v >= c}[op]


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
    if name == "q":
        v, c = fx.q.astype(np.int64), expr[2] if len(expr) > 2 else None
        if op == "is null":
            return ~fx.q_valid
        if op == "is not null":
            return fx.q_valid.copy()
        m = np.isin(v, list(c)) if op == "in" else {"=": v == c, "<>": v != c, "<": v < c, "<=": v <= c, ">": v > c, ">=": v >= c}[op]
        return m & fx.q_valid
    distinct, codes = fx.index(name)
    if op == "is null":
        return codes < 0
    if op == "is not null":
        return codes >= 0
    if op == "in":
        wanted = set(expr[2])
        table = np.array([v in wanted for v in distinct] + [False], bool)   # the last entry: NULL (code -1)
    else:
        table = np.array([compare(v, op, expr[2]) for v in distinct] + [False], bool)
    return table[codes]


def index_values(values):
    """(distinct values sorted, per row the index of its value or -1 for NULL) of a list of values"""
    distinct = sorted({v for v in values if v is not None})
    where = {v: i for i, v in enumerate(distinct)}
    return distinct, np.array([-1 if v is None else where[v] for v in values], np.int64)


def evaluate_indexed(index, op, c):
    """the same rule over index_values(values), for the packed vectors of the kernel-level tests"""
    distinct, codes = index
    return np.array([compare(v, op, c) for v in distinct] + [False], bool)[codes]


def cnf_of(expr):
    """AND-of-ORs of leaves when `expr` is written that way already, else None"""
    if is_leaf(expr):
        return [[expr]]
    if expr[0] == "or":
        return [list(expr[1:])] if all(is_leaf(e) for e in expr[1:]) else None
    out = []
    for e in expr[1:]:
        sub = cnf_of(e)
        if sub is None or (not is_leaf(e) and e[0] == "or" and len(sub) != 1):
            return None
        out.extend(sub)
    return out


def cnf_size(expr):
    """(clauses, leaves) of `expr` in conjunctive normal form before any merging (filter_integer_cases.cnf_size)"""
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
    if is_leaf(expr):
        return False
    if expr[0] == "or" and any(not is_leaf(e) and e[0] == "and" for e in expr[1:]):
        return True
    return any(needs_distribution(e) for e in expr[1:])


# ---------------------------------------------------------------------------------------------------- the cases
def edge_constants(fx, name):
    """the whole binary pool, and the successor and a near predecessor in byte order of every value the column holds"""
    cs = set(pool(False)) | set(pool(True))
    for v in fx.index(name)[0]:
        cs.add(successor(v))
        if predecessor(v) is not None:
            cs.add(predecessor(v))
    return sorted(cs)


def scan_constants(fx, name):
    """edge_constants thinned for the scans of one column.  No family and no kind of member is dropped: of every family the
    column holds, two members -- which two moves on from family to family, so that the seven kinds of sibling (the prefix
    alone, + 0x00, 0x01, 0x7F, 0x80, 0xFF, 0xFF 0x00) all occur, at different prefixes -- with the successor of the first and the
    predecessor of the second; of every other family of the pool one member.  The host file asserts the seven kinds per
    column; the kernel-level tests run every constant."""
    c = fx.columns[name]
    held = set(fx.index(name)[0])
    cs = set()
    for i, vs in enumerate(c.families.values()):
        vs = [v for v in vs if v in held] or vs
        first, second = vs[i % len(vs)], vs[(i + len(vs) // 2) % len(vs)]
        cs.update(x for x in (first, successor(first), second, predecessor(second)) if x is not None)
    for text in (False, True):
        for j, vs in enumerate(families(text).values()):
            cs.add(vs[(j + 3) % len(vs)])
    return sorted(cs)


def single_leaf_cases(fx, name, constants=None):
    cs = scan_constants(fx, name) if constants is None else constants
    return [(name, op, c) for op in OPS for c in cs] + [(name, "is null"), (name, "is not null")]


def reduced_constants():
    """for the row-count seams: '', an inline constant, a 12-byte and a 13-byte one, one no row matches"""
    return [b"", BASE[:4] + b"\x80", BASE[:12], BASE[:13], b"no row holds this value"]


def in_list_cases(fx, name):
    """empty, one value, duplicates, inline and long constants mixed, one tail family, exactly 256 values"""
    held = fx.index(name)[0] or [b""]
    inline = [v for v in held if len(v) <= 12] or [b"x"]
    long_ = [v for v in held if len(v) > 12] or [b"no such long value......."]
    many = list(dict.fromkeys(list(held) + [b"absent-%03d" % i + b"z" * (i % 17) for i in range(256)]))[:256]
    assert len(set(many)) == 256
    return [(name, "in", []), (name, "in", [held[0]]), (name, "in", [held[-1], held[0], held[-1], held[0]]),
            (name, "in", [inline[0], long_[0], inline[-1], long_[-1], b"", b"nothing"]),
            (name, "in", _tail_family(13) + _tail_family(17)[1:3]), (name, "in", many[::-1])]


def too_long_in_list(name):
    return (name, "in", [b"v%03d" % i for i in range(257)])


def prefix_cases(fx, name):
    """prefixes: '', ending in 0xFF, all 0xFF, 12 and 13 bytes long, a whole row, longer than every row (none holds % or _)"""
    held = fx.index(name)[0] or [b""]
    longest = max(held, key=len)
    ps = [b"", BASE[:4] + b"\xff", BASE[:12] + b"\xff", b"\xff", b"\xff" * 4, b"\xff" * 12, BASE[:12], BASE[:13], BASE[:3], held[len(held) // 2],
          held[-1], longest, longest + b"!", b"k", b"tail17-", "é".encode()]
    return list(dict.fromkeys(ps))


def _random_leaf(fx, rng, names):
    if rng.random() < 0.25:
        form = int(rng.integers(8))
        c = int(rng.integers(-6, 51))
        return ("q", ("=", "<>", "<", "<=", ">", ">=")[form], c) if form < 6 else ("q", "in", [c, c + 1, 7]) if form == 6 else ("q", "is null")
    name = names[int(rng.integers(len(names)))]
    held = fx.index(name)[0] or [b""]
    v = held[int(rng.integers(len(held)))]
    c = (v, successor(v), predecessor(v) or b"", v[: max(len(v) - 1, 0)])[int(rng.integers(4))]
    form = int(rng.integers(10))
    if form < 7:
        return (name, OPS[form], c)
    if form == 7:
        return (name, "is null")
    if form == 8:
        return (name, "is not null")
    return (name, "in", [c] + [held[int(i)] for i in rng.integers(0, len(held), int(rng.integers(0, 4)))])


def _random_tree(fx, rng, names, depth):
    if depth == 0 or rng.random() < 0.25:
        return _random_leaf(fx, rng, names)
    op = "and" if rng.random() < 0.5 else "or"
    return (op,) + tuple(_random_tree(fx, rng, names, depth - 1) for _ in range(int(rng.integers(2, 4))))


def generated_trees(fx, kind, seed=19, want=40, want_distributed=10):
    """AND / OR trees of depth <= 3 with string leaves on two or three columns of one file and integer leaves on q, kept when
    their conjunctive normal form has at most 24 leaves"""
    rng = np.random.default_rng(seed)
    all_names = [n for n in fx.names(kind) if n != "dict_empty"]
    trees, distributed = [], 0
    while len(trees) < want or distributed < want_distributed:
        names = [all_names[int(i)] for i in rng.choice(len(all_names), int(rng.integers(2, 4)), replace=False)]
        t = _random_tree(fx, rng, names, 3)
        used = {l for l in _leaf_columns(t)}
        if is_leaf(t) or cnf_size(t)[1] > 24 or len(used - {"q"}) < 2:
            continue
        d = needs_distribution(t)
        if len(trees) >= want and not d:
            continue
        trees.append(t)
        distributed += d
    return trees


def _leaf_columns(expr):
    if is_leaf(expr):
        return [expr[0]]
    return [c for e in expr[1:] for c in _leaf_columns(e)]


def refused_tree():
    """an OR of five ANDs of three string leaves: 3^5 clauses of 5 leaves, past the 96-leaf limit"""
    a = lambda i: ("and", ("utf8", ">", b"k%d" % i), ("binary", "<", b"tail%d" % i), ("fsb4", "<>", b"kji%d" % i))
    return ("or",) + tuple(a(i) for i in range(5))


def delivery_cases():
    """one tree per column kind"""
    return {"plain": ("or", ("and", ("binary", ">=", BASE[:12]), ("binary", "<", BASE[:12] + b"\xff\x00"), ("q", ">=", 0)),
                      ("utf8", "starts_with", b"tail"), ("fsb13", "=", BASE[:12] + b"\x80")),
            "dict": ("and", ("or", ("dict_300", "starts_with", BASE[:4]), ("dict_delta", "is null")), ("dict_int8_utf8", "<>", BASE[:13])),
            "ree": ("or", ("ree_int16_utf8", "<", BASE[:12]), ("and", ("ree_int64_utf8", "in", [BASE[:13], b""]), ("q", "<", 25)))}

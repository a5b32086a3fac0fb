"""tests/filter_program_cases.py without a GPU: its evaluator against the evaluators the project already trusts, on their own
fixtures; its restatement of the float key against mi_filter_float_key (the one place the library is consulted, and it is the
library that is held to the restatement); and the non-vacuity counts tests/test_gpu_filter_programs.py relies on, on the
reference alone."""
import numpy as np

import duckdb_arrow_amd as da
import filter_integer_cases as ic
import filter_program_cases as pc
import filter_string_cases as sc
from test_gpu_filters_float import _compare_float, _compare_int, _float_column, _wide_column
from test_gpu_pattern_filters import python_says

L = pc.L


# ---------------------------------------------------------------------------------------------------- CNF -> the tree form
def tree_of_leaf(leaf):
    """a leaf of the program form as the AND / OR tree of (column, op, constant) the older evaluators take"""
    col, op, neg = leaf["col"], leaf["op"], leaf.get("negate")
    if op == pc.IS_NULL:
        return (col, "is null")
    if op == pc.IS_NOT_NULL:
        return (col, "is not null")
    if op in (pc.RANGE, pc.WIDE_RANGE):
        lo, hi = leaf["lo"], leaf["hi"]
        return ("or", (col, "<", lo), (col, ">", hi)) if neg else ("and", (col, ">=", lo), (col, "<=", hi))
    if op in (pc.IN, pc.WIDE_IN, pc.STR_IN):
        if not neg:
            return (col, "in", list(leaf["values"]))
        return ("and", (col, "is not null")) + tuple((col, "<>", v) for v in leaf["values"])
    if op == pc.STR_RANGE:
        parts = []
        if leaf["lower"] is not None:
            parts.append((col, ("<" if leaf["lo_incl"] else "<=") if neg else (">=" if leaf["lo_incl"] else ">"), leaf["lower"]))
        if leaf["upper"] is not None:
            parts.append((col, (">" if leaf["hi_incl"] else ">=") if neg else ("<=" if leaf["hi_incl"] else "<"), leaf["upper"]))
        return (("or",) if neg else ("and", (col, "is not null"))) + tuple(parts)
    assert op == pc.STR_MATCH and len(leaf["segments"]) == 1 and leaf["head"] and not leaf["tail"], leaf
    return (col, "not starts_with" if neg else "starts_with", leaf["segments"][0])


def tree_of(program):
    return ("and",) + tuple(("or",) + tuple(tree_of_leaf(leaf) for leaf in clause) for clause in program)


# ---------------------------------------------------------------------------------------------------- integers
def test_integer_programs_agree_with_the_integer_evaluator():
    """RANGE, IN, IS [NOT] NULL, plain and negated, uint64 included, on the integer suite's table: filter_integer_cases.evaluate,
    which tests/test_filter_integer_reference_host.py holds to the oracle"""
    fx = ic.fixture()
    cols = pc.Columns(ic.N_ROWS)
    for name in ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "date64", "dec128_18"):
        cols.add(pc.Column(name, "int", fx.stored[name]), fx.valid[name])
    I64_MAX = ic.I64_MAX
    programs = [
        [[L("i32", pc.RANGE, lo=-1, hi=1)], [L("i32", pc.RANGE, lo=0, hi=5)]],
        [[L("i8", pc.RANGE, lo=5, hi=-5)]], [[L("i8", pc.RANGE, lo=5, hi=-5, negate=True)]],
        [[L("i8", pc.RANGE, lo=-128, hi=0, negate=True), L("u8", pc.IN, values=[255, 0])], [L("i16", pc.IS_NOT_NULL), L("u16", pc.IS_NULL)]],
        [[L("u64", pc.RANGE, lo=0, hi=I64_MAX)]], [[L("u64", pc.RANGE, lo=I64_MAX, hi=I64_MAX, negate=True)]],
        [[L("u64", pc.IN, values=[0, 1, I64_MAX, 5])], [L("u32", pc.RANGE, lo=0, hi=(1 << 32) - 2)]],
        [[L("u64", pc.IN, values=[], negate=True)]], [[L("i64", pc.IN, values=[ic.I64_MIN, I64_MAX, 0], negate=True)]],
        [[L("i64", pc.RANGE, lo=ic.I64_MIN, hi=-1), L("date64", pc.RANGE, lo=0, hi=1 << 40)], [L("dec128_18", pc.RANGE, lo=-10 ** 18, hi=0, negate=True)]],
        [[L("u16", pc.RANGE, lo=65535, hi=65535), L("u16", pc.RANGE, lo=65535, hi=65535), L("i16", pc.IN, values=[-32768])]],
    ]
    kept = []
    for program in programs:
        got, want = pc.evaluate(program, cols, ic.N_ROWS), ic.evaluate(fx, tree_of(program))
        assert np.array_equal(got, want), program
        kept.append(int(got.sum()))
    assert sum(1 for k in kept if 0 < k < ic.N_ROWS) >= 8, kept
    # a uint64 constant past INT64_MAX, which the older evaluator takes too
    program = [[L("u64", pc.RANGE, lo=pc.P63, hi=pc.P64 - 1)]]
    assert np.array_equal(pc.evaluate(program, cols, ic.N_ROWS), ic.evaluate(fx, ("u64", ">", I64_MAX)))


# ---------------------------------------------------------------------------------------------------- strings and dictionaries
def test_string_programs_agree_with_the_string_evaluator():
    """STR_IN, STR_RANGE, a head-anchored STR_MATCH and IS [NOT] NULL on the string suite's plain columns, NULL rows as the
    empty string the packer makes of them: filter_string_cases.evaluate"""
    fx = sc.fixture()
    cols = pc.Columns(sc.N_ROWS)
    for name in ("binary", "utf8", "fsb13"):
        values = fx.columns[name].values
        cols.add(pc.Column(name, "str", [b"" if v is None else v for v in values]), [v is not None for v in values])
    B = sc.BASE
    programs = [
        [[L("binary", pc.STR_IN, values=[b"", B[:4], B[:13], B[:12] + b"\x80"])]],
        [[L("binary", pc.STR_IN, values=[b"", B[:13]], negate=True)]], [[L("utf8", pc.STR_IN, values=[], negate=True)]],
        [[L("binary", pc.STR_RANGE, lower=B[:4], lo_incl=False, upper=B[:12] + b"\xff", hi_incl=True)]],
        [[L("binary", pc.STR_RANGE, lower=B[:4], lo_incl=True, upper=B[:13], hi_incl=False, negate=True)]],
        [[L("utf8", pc.STR_RANGE, lower=None, lo_incl=False, upper=B[:8], hi_incl=False), L("fsb13", pc.IS_NULL)],
         [L("binary", pc.STR_MATCH, segments=[B[:3]], head=True, tail=False, negate=True), L("utf8", pc.STR_MATCH, segments=[b"tail"], head=True, tail=False)]],
        [[L("fsb13", pc.STR_RANGE, lower=b"tail13", lo_incl=True, upper=None, hi_incl=False)], [L("fsb13", pc.IS_NOT_NULL)]],
        [[L("binary", pc.STR_RANGE, lower=b"tail", lo_incl=True, upper=b"L", hi_incl=True, negate=True)]],
    ]
    kept = []
    for program in programs:
        got, want = pc.evaluate(program, cols, sc.N_ROWS), sc.evaluate(fx, tree_of(program))
        assert np.array_equal(got, want), program
        kept.append(int(got.sum()))
    assert sum(1 for k in kept if 0 < k < sc.N_ROWS) >= 6, kept


def test_pattern_leaves_agree_with_the_pattern_suites_python():
    """STR_MATCH with several segments and both anchors: test_gpu_pattern_filters.python_says over the LIKE pattern the leaf stands for"""
    values = [v for v in sc.pool(False) if b"%" not in v and b"_" not in v] + [None, b"kjikji", b"ekji", b"kji-e-kji"]
    cols = pc.Columns(len(values))
    cols.add(pc.Column("s", "str", [b"" if v is None else v for v in values]), [v is not None for v in values])
    kept = []
    for segments, head, tail in (([b"kji"], False, False), ([b"kji"], True, True), ([b"kji", b"e"], True, False), ([b"j", b"kji"], False, True),
                                 ([b"k", b"j", b"i"], False, False), ([b"\xff"], False, True), ([sc.BASE[:13]], True, False), ([b"tail", b"~"], True, False)):
        for negate in (False, True):
            leaf = L("s", pc.STR_MATCH, segments=segments, head=head, tail=tail, negate=negate)
            expr = ("s", "not like" if negate else "like", pc.like_pattern(segments, head, tail))
            want = np.array([python_says(expr, {"s": values}, i) for i in range(len(values))], bool)
            got = pc.evaluate([[leaf]], cols, len(values))
            assert np.array_equal(got, want), leaf
            kept.append(int(got.sum()))
    assert min(kept) < 5 and sum(1 for k in kept if 0 < k < len(values) - 1) >= 12, kept


def test_dictionary_maps_agree_with_the_string_evaluator():
    """DICT_MAP over a dictionary column of the string suite: the map made entry by entry with filter_string_cases.compare,
    a NULL entry coded 2, a NULL row pointing at index n_in -- against filter_string_cases.evaluate on the row values"""
    fx = sc.fixture()
    name = "dict_int16_binary"
    values = fx.columns[name].values
    entries = sorted({v for v in values if v is not None}) + [None]     # the last entry is a NULL entry of the dictionary itself
    where = {v: i for i, v in enumerate(entries)}
    rng = np.random.default_rng(3)
    idx = np.array([where[v] if v is not None or rng.random() < 0.5 else len(entries) for v in values], np.uint32)   # NULL: either way
    cols = pc.Columns(sc.N_ROWS)
    cols.add(pc.Column(name, "dict", idx), np.zeros(sc.N_ROWS, bool))
    c = entries[len(entries) // 3]
    for op in sc.OPS:
        table = np.array([2 if e is None else int(sc.compare(e, op, c)) for e in entries], np.uint8)
        inverse = {"=": "<>", "<>": "=", "<": ">=", "<=": ">", ">": "<=", ">=": "<", "starts_with": "not starts_with"}[op]
        for mode, expr in ((0, (name, op, c)), (1, (name, inverse, c)), (2, (name, "is null")), (3, (name, "is not null"))):
            for b in (None, name):   # the bitmap, all NULL here, is not read
                got = pc.evaluate([[L(name, pc.DICT_MAP, validity=b, map=table, mode=mode)]], cols, sc.N_ROWS)
                assert np.array_equal(got, sc.evaluate(fx, expr)), (op, mode)


# ---------------------------------------------------------------------------------------------------- floats and 128 bits
def test_float_and_wide_programs_agree_with_the_float_suites_comparisons():
    """RANGE / IN on FLOAT and DOUBLE and WIDE_RANGE / WIDE_IN, plain and negated, in a CNF with IS NULL: _compare_float and
    _compare_int of tests/test_gpu_filters_float.py, combined here as the tree says"""
    n = 3000
    rng = np.random.default_rng(77)
    data = {"f32": _float_column(rng, np.float32, n), "f64": _float_column(rng, np.float64, n), "hug": _wide_column(rng, n, 10 ** 38 - 1, 120)}
    valid = {name: rng.random(n) >= 0.1 for name in data}
    cols = pc.Columns(n)
    for name in ("f32", "f64"):
        cols.add(pc.Column(name, "float", data[name]), valid[name])
    cols.add(pc.Column("hug", "wide", pc.object_array(data["hug"])), valid["hug"])

    def cmp(col, op, c):
        if col == "hug":
            return _compare_int(data[col], op, c)
        return _compare_float(data[col], op, c, col == "f32")

    def leaf(e):
        col, op = e[0], e[1]
        if op == "is null":
            return ~valid[col]
        if op == "is not null":
            return valid[col]
        if op == "in":
            return np.logical_or.reduce([cmp(col, "=", c) for c in e[2]] + [np.zeros(n, bool)]) & valid[col]
        return cmp(col, op, e[2]) & valid[col]

    def tree(e):
        if e[0] in ("and", "or") and len(e) > 1 and isinstance(e[1], tuple):
            parts = [tree(k) for k in e[1:]]
            return np.logical_and.reduce(parts) if e[0] == "and" else np.logical_or.reduce(parts)
        return leaf(e)

    NAN, INF, P63, P64 = pc.NAN, pc.INF, pc.P63, pc.P64
    programs = [[[L(c, pc.RANGE, lo=lo, hi=hi, negate=neg)]] for c in ("f32", "f64") for neg in (False, True)
                for lo, hi in ((NAN, NAN), (-INF, -0.0), (0.0, 1.5), (1.3, INF), (INF, NAN), (NAN, 1.5), (-5e-324, 5e-324), (-1.5, 1.3))]
    programs += [[[L(c, pc.IN, values=vals, negate=neg)]] for c in ("f32", "f64") for neg in (False, True) for vals in ([NAN, -0.0, 7.25], [1.3], [], [INF, -INF, 1.5])]
    programs += [[[L("hug", pc.WIDE_RANGE, lo=lo, hi=hi, negate=neg)]] for neg in (False, True)
                 for lo, hi in ((-P63 - 1, P63), (P64, P64), (-P64 - 1, -P64 + 1), (P64, -P64), (-(1 << 127), -1), (P63, (1 << 127) - 1))]
    programs += [[[L("hug", pc.WIDE_IN, values=vals, negate=neg)]] for neg in (False, True) for vals in ([0, P64, -P64 - 1], [P63, 7], [], [12345, -1, 1])]
    programs += [[[L("f32", pc.RANGE, lo=-2.0, hi=NAN), L("hug", pc.IS_NULL)], [L("f64", pc.IN, values=[NAN, 0.0, 2.5], negate=True), L("hug", pc.WIDE_RANGE, lo=0, hi=P64)],
                  [L("f64", pc.IS_NOT_NULL)]]]
    kept = []
    for program in programs:
        got = pc.evaluate(program, cols, n)
        assert np.array_equal(got, tree(tree_of(program))), program
        kept.append(int(got.sum()))
    assert sum(1 for k in kept if 0 < k < n) >= len(kept) // 2, kept


def test_the_float_key_restatement_is_the_librarys():
    """every float constant of every program the GPU suite launches, and the specials: mi_filter_float_key gives the key
    filter_program_cases.float_key restates"""
    constants = {(x, w) for nrows, program in pc.random_programs() for x, w in pc.float_constants(program, pc.columns(nrows))}
    constants |= {(x, w) for _, program in pc.handwritten_programs() for x, w in pc.float_constants(program, pc.columns(9))}
    rng = np.random.default_rng(1)
    for w, f in ((4, np.float32), (8, np.float64)):
        constants |= {(float(x), w) for x in _float_column(rng, f, 400)}
    assert len(constants) > 200 and any(x != x for x, _ in constants)
    for x, w in sorted(constants, key=repr):
        assert pc.float_key(x, w) == da.filter_float_key(x, w), (x, w)
    for w in (4, 8):   # the order it stands for
        keys = [pc.float_key(x, w) for x in (-pc.INF, -1.5, -5e-324 if w == 8 else -1e-45, -0.0, 0.0, 1e-45, 1.5, pc.INF, pc.NAN)]
        assert keys == sorted(keys) and keys[3] == keys[4] == 0 and pc.float_key(-pc.NAN, w) == keys[-1]


# ---------------------------------------------------------------------------------------------------- the tables
def test_string_tables_and_device_fields():
    """the layouts csrc/kernels.hpp documents: 3 words per string constant, the third the address of its bytes inside the table's
    own allocation; {lower, upper} pairs; the biased uint64 constants; the flag bits"""
    cols = pc.columns(9)
    leaf = L("s_shuf", pc.STR_IN, values=[b"abc", pc.LONG_STRINGS[0], b""])
    base = 0x7F0000001000
    image = pc.table_image(leaf, cols, base)
    assert len(image) == len(pc.table_image(leaf, cols, 0)) and len(image) % 8 == 0
    words = image[:72].view(np.int64)
    assert words[0] == 3 | (int.from_bytes(b"abc", "little") << 32) and words[1] == 0
    assert words[3] == 13 | (int.from_bytes(pc.LONG_STRINGS[0][:4], "little") << 32) and words[4] == 0
    for j, c in enumerate(leaf["values"]):
        at = int(words[3 * j + 2]) - base
        assert 72 <= at <= len(image) - len(c) and image[at: at + len(c)].tobytes() == c
    f = pc.device_fields(leaf, cols, True, 8, 16, base, heap=0x5000)
    assert (f["op"], f["width"], f["n_in"], f["flags"], f["lo"]) == (pc.STR_IN, 16, 3, pc.F_ENDS_CLAUSE, 0x5000)
    assert f["hi"] == pc._signed(sc.FAR_BASE)
    wide = pc.table_image(L("hug", pc.WIDE_RANGE, lo=-1, hi=pc.P64), cols, 0).view(np.int64)
    assert wide.tolist() == [-1, -1, 0, 1]
    f = pc.device_fields(L("u64", pc.RANGE, lo=0, hi=pc.P64 - 1, negate=True), cols, False, 8, 0, 0)
    assert (f["lo"], f["hi"], f["flags"], f["width"]) == (-pc.P63, pc.P63 - 1, pc.F_UNSIGNED | pc.F_BIAS | pc.F_NEGATE, 8)
    f = pc.device_fields(L("f32", pc.RANGE, lo=-0.0, hi=pc.NAN), cols, True, 8, 0, 0)
    assert (f["lo"], f["hi"], f["flags"], f["width"]) == (0, 0x7FFFFFFF, pc.F_FLOAT | pc.F_ENDS_CLAUSE, 4)
    f = pc.device_fields(L("s_arrow", pc.STR_MATCH, segments=[b"a", b"b"], head=True, tail=True), cols, True, 8, 0, 0)
    assert f["n_in"] == 2 | 0x300
    f = pc.device_fields(L("s_arrow", pc.STR_RANGE, lower=b"a", lo_incl=False, upper=None, hi_incl=True), cols, True, 8, 0, 0)
    assert f["n_in"] == 1 | 8
    assert pc.table_image(L("u64", pc.IN, values=[pc.P64 - 1, 0]), cols, 0).view(np.int64).tolist() == [pc.P63 - 1, -pc.P63, 0]


def test_columns_are_what_the_suite_says_they_are():
    """pad rows and pad bits, NULL strings, pointers inside the heap, the dictionary indices past the map, NULLs at the seams"""
    for nrows in (1, 65, 2049):
        cols = pc.columns(nrows)
        total = nrows + pc.PAD_ROWS
        for name, c in cols.col.items():
            assert len(c.values) == total and len(cols.valid[name]) == total and cols.valid[name][nrows:].all(), name
        for name in pc.STRING_COLUMNS:
            c = cols.col[name]
            assert all(v == b"" for v, ok in zip(c.values, cols.valid[name]) if not ok)
            images, heap, words = sc.pack_string_t([v if ok else None for v, ok in zip(c.values, cols.valid[name])], c.ptr_base, c.layout)
            assert not images[~cols.valid[name]].any()                     # sixteen zero bytes (and the packer asserts every pointer)
        seams = cols.valid["seams"]
        assert not seams[nrows - 1] and all(not seams[r - 1] and not seams[r] for r in range(64, nrows, 64))
        assert not pc.validity_words(cols.valid["all_null"]).any() and (pc.validity_words(cols.valid["all_valid"]) == np.uint64(pc.P64 - 1)).all()
    idx = pc.columns(2049).col["dict"].values[:2049]
    assert {pc.DICT_ENTRIES - 1, pc.DICT_ENTRIES, 0xFFFFFFFF} <= set(idx.tolist())


# ---------------------------------------------------------------------------------------------------- non-vacuity
def test_the_random_programs_are_not_vacuous():
    """what section `clause logic` of the GPU suite relies on, on the reference alone: at most 150 programs, every leaf count
    1 .. 24, 24 leaves in one clause and 24 clauses of one leaf, at least half of the programs keep neither no row nor every
    row, every leaf form in at least 10 programs, validity pointers present and absent in one program"""
    programs = pc.random_programs()
    assert len(programs) <= 150 and all(pc.within_limits(p) for _, p in programs) and all(pc.within_limits(p) for _, p in pc.handwritten_programs())
    assert {pc.n_leaves(p) for _, p in programs} == set(range(1, 25))
    assert any(len(p) == 1 and len(p[0]) == 24 for _, p in programs) and any(len(p) == 24 and all(len(c) == 1 for c in p) for _, p in programs)
    mixed, seen = pc.vacuity(programs)
    assert mixed * 2 >= len(programs), mixed
    assert all(n >= 10 for n in seen.values()), seen
    both = sum(1 for _, p in programs if {leaf.get("validity") is None for c in p for leaf in c if leaf["op"] != pc.DICT_MAP} == {True, False})
    assert both >= len(programs) // 2, both
    negated = {pc.form_of(leaf, pc.columns(n)) for n, p in programs for c in p for leaf in c if leaf.get("negate")}
    assert negated == set(pc.NEGATABLE)
    assert {n for n, _ in programs} >= {8193, 5 * 2048 + 5}               # more than one window, more than one workgroup


def test_the_handwritten_programs_are_not_vacuous():
    """at 2049 rows: plain and negated halves complement each other on the valid rows, a negated leaf keeps no NULL row,
    IS NULL OR <comparison> keeps every NULL row, IS NULL under no pointer keeps nothing, and most programs keep some rows"""
    n = 2049
    cols = pc.columns(n)
    programs = dict(pc.handwritten_programs())
    assert len(programs) == len(pc.handwritten_programs())                  # the names are distinct
    kept = {name: pc.evaluate(p, cols, n) for name, p in programs.items()}
    assert sum(1 for m in kept.values() if 0 < m.sum() < n) * 2 >= len(kept)
    for name, p in programs.items():
        if name.endswith(" negated") and len(p) == 1 and len(p[0]) == 1:
            leaf = p[0][0]
            valid = cols.valid[leaf["validity"]][:n] if leaf["validity"] else np.ones(n, bool)
            plain = kept[name[: -len(" negated")]]
            assert not (plain & kept[name]).any() and np.array_equal(plain | kept[name], valid), name
            assert not (kept[name] & ~valid).any()
    for leaf in pc.VALIDITY_LEAVES:
        for b in pc.BITMAPS:
            tag = "%s under %s" % (leaf["col"], b)
            nulls = ~cols.valid[b][:n] if b else np.zeros(n, bool)
            assert np.array_equal(kept[tag + ": is null"], nulls)
            assert np.array_equal(kept[tag + ": is null or"], nulls | kept[tag]) and np.array_equal(kept[tag + ": is null or not"], nulls | kept[tag + " negated"])
        assert not kept["%s under None: is null" % leaf["col"]].any() and not kept["%s under all_null" % leaf["col"]].any()
        assert 0 < kept["%s under seams" % leaf["col"]].sum() < kept["%s under None" % leaf["col"]].sum() < n
    for mode in range(4):
        for j in range(5):
            a, b, c = (kept["dict map %d, mode %d, under %s" % (j, mode, x)] for x in (None, "dict", "all_null"))
            assert np.array_equal(a, b) and np.array_equal(a, c)
    base = kept["base"]
    assert 100 < base.sum() < n - 100
    for name, _, _ in pc.instance_programs():
        assert np.array_equal(kept[name], base), name                         # the added leaves are neutral
    for name in ("contradictory", "lo > hi", "in, none", "NaN .. NaN f32 negated", "uint64 0x8000000000000000 .. 0x7fffffffffffffff"):
        assert (kept[name].sum() == 0) == (name != "NaN .. NaN f32 negated"), name
    assert 0 < kept["NaN .. NaN f64"].sum() < 200 and 0 < kept["in, 256"].sum() < n and 0 < kept["u32 at its maximum"].sum() < n

"""The evaluator and the string_t packer behind tests/test_gpu_string_filter_leaves.py against references that share no code
with them: pyarrow.compute over the columns read back from the files, the oracle's CNF evaluator, the oracle's string decode
and its string_t reader.  What makes the expected rows and the packed vectors trustworthy before a kernel is involved.
No GPU and no library."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.ipc as ipc
import pytest

import filter_string_cases as sc
from oracle import pyoracle as po

ALL_COLUMNS = [n for names in sc.COLUMN_KINDS.values() for n in names]


@pytest.fixture(scope="module")
def fx():
    return sc.fixture()


@pytest.fixture(scope="module")
def read_back(fx, tmp_path_factory):
    """{column: the binary array pyarrow reads back from the file}, and the writer's statistics per file"""
    d = tmp_path_factory.mktemp("string_cases")
    cols, stats = {}, {}
    for kind in sc.COLUMN_KINDS:
        path = str(d / (kind + ".arrows"))
        stats[kind] = fx.write(path, kind)
        with ipc.open_stream(path) as r:
            assert [b.num_rows for b in r] == list(sc.BATCH_ROWS)
        t = ipc.open_stream(path).read_all()
        assert t.column("k").to_pylist() == list(range(sc.N_ROWS))
        for name in fx.names(kind):
            chunks = []
            for ch in t.column(name).chunks:
                if kind == "ree":
                    ch = pc.run_end_decode(ch)
                if kind == "dict":
                    ch = ch.dictionary_decode()
                chunks.append(ch.cast(pa.large_binary()).cast(pa.binary()) if ch.type in (pa.large_utf8(), pa.large_binary()) else ch.cast(pa.binary()))
            cols[name] = pa.concat_arrays(chunks)
    return cols, stats


def test_the_files_hold_the_rows_the_cases_are_about(fx, read_back):
    cols, stats = read_back
    assert fx.names("plain") == sc.COLUMN_KINDS["plain"] and fx.names("dict") == sc.COLUMN_KINDS["dict"] and fx.names("ree") == sc.COLUMN_KINDS["ree"]
    for name in ALL_COLUMNS:
        c = fx.columns[name]
        assert cols[name].to_pylist() == c.values, name   # what pyarrow reads back is what the evaluator works on
        if name == "dict_empty":
            assert c.values == [None] * sc.N_ROWS
            continue
        nulls = sum(v is None for v in c.values)
        assert 0.04 * sc.N_ROWS < nulls < 0.15 * sc.N_ROWS, name
        held = set(fx.index(name)[0])
        for r in fx.seam_rows:   # a value at every lane, word, window, workgroup and batch seam
            assert c.values[r] is not None or c.kind == "dict", (name, r)
        if c.kind != "dict":
            assert held == set(c.pool), name   # every pool value occurs
            assert [c.values[r] for r in sc.EDGE_ROWS] != [c.values[sc.EDGE_ROWS[0]]] * len(sc.EDGE_ROWS)
    # the pool itself: bytes on both sides of 0x80, both sides of the inline limit, the length ties, no LIKE wildcard
    binary = sc.pool(False)
    assert all(b"%" not in v and b"_" not in v for v in binary + sc.pool(True))
    assert {len(v) for v in binary} >= set(sc.LENGTHS) | {12, 13, 15, 20}
    for k in sc.SIBLING_PREFIXES:
        p = sc.BASE[:k]
        assert {p, p + b"\x00", p + b"\x01", p + b"\x7f", p + b"\x80", p + b"\xff", p + b"\xff\x00"} <= set(binary)
    assert all(v.decode() is not None for v in sc.pool(True))   # valid UTF-8
    assert any(len(ch.encode()) == w for w in (2, 3, 4) for v in sc.pool(True) for ch in v.decode()) and \
        {len(ch.encode()) for v in sc.pool(True) for ch in v.decode()} == {1, 2, 3, 4}
    # dictionaries: delta and replacement messages, NULL entries and unused entries, 300 entries, every index type
    assert stats["dict"].num_dictionary_deltas >= 3 and stats["dict"].num_replaced_dictionaries >= 3
    assert len(fx.columns["dict_300"].arrays[0].dictionary) == 300 and fx.columns["dict_300"].arrays[0].dictionary.null_count == 2
    assert len(fx.columns["dict_empty"].arrays[0].dictionary) == 0
    assert {fx.columns[n].arrow_type.index_type for n in sc.COLUMN_KINDS["dict"]} == set(sc.DICT_INDEX_TYPES)
    assert {fx.columns[n].arrow_type.value_type for n in sc.COLUMN_KINDS["dict"]} == set(sc.DICT_VALUE_TYPES)
    for name in sc.COLUMN_KINDS["dict"][:8]:
        arr = fx.columns[name].arrays[0]
        assert arr.dictionary.null_count == 1 and arr.indices.null_count > 0
        used = set(arr.indices.drop_null().to_pylist())
        assert len(used) < len(arr.dictionary) and arr.dictionary.to_pylist().index(None) in used   # NULL through the entry
    assert {fx.columns[n].arrow_type.run_end_type for n in sc.COLUMN_KINDS["ree"]} == {pa.int16(), pa.int32(), pa.int64()}
    assert all(len(fx.columns[n].arrays[0].run_ends) < sc.BATCH_ROWS[0] // 2 for n in sc.COLUMN_KINDS["ree"])


PC_OPS = {"=": pc.equal, "<>": pc.not_equal, "<": pc.less, "<=": pc.less_equal, ">": pc.greater, ">=": pc.greater_equal}


def _arrow_rows(column, leaf):
    """the rows pyarrow.compute keeps: a NULL result is not true"""
    op = leaf[1]
    if op == "is null":
        out = pc.is_null(column)
    elif op == "is not null":
        out = pc.is_valid(column)
    elif op == "in":
        out = pc.is_in(column, value_set=pa.array(list(leaf[2]), pa.binary())) if len(leaf[2]) else pa.array(np.zeros(len(column), bool))
        out = pc.and_(out, pc.is_valid(column))
    elif op == "starts_with":
        out = pc.starts_with(column, pattern=leaf[2])
    elif op == "not starts_with":
        out = pc.invert(pc.starts_with(column, pattern=leaf[2]))
    else:
        out = PC_OPS[op](column, pa.scalar(leaf[2], pa.binary()))
    return np.flatnonzero(out.fill_null(False).to_numpy(zero_copy_only=False))


def leaves_of(fx, name):
    """every single leaf the GPU file runs on this column"""
    leaves = sc.single_leaf_cases(fx, name) + sc.in_list_cases(fx, name)
    for p in sc.prefix_cases(fx, name):
        leaves += [(name, "starts_with", p), (name, "not starts_with", p)]
    return leaves


@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_single_leaves_equal_pyarrow_compute(fx, read_back, name):
    """= <> < <= > >= starts_with at every constant of the column, the IN-lists, the prefixes and their negation, IS [NOT] NULL"""
    column = read_back[0][name]
    kept = []
    for leaf in leaves_of(fx, name):
        got, want = np.flatnonzero(sc.evaluate(fx, leaf)), _arrow_rows(column, leaf)
        assert np.array_equal(got, want), "%r: the evaluator keeps %d rows, pyarrow.compute %d" % (leaf, len(got), len(want))
        kept.append(len(got))
    assert 0 in kept and (max(kept) > sc.N_ROWS // 2 or name == "dict_empty")


def test_edge_constants_on_the_packed_vector_equal_pyarrow_compute(fx):
    """the kernel-level test's vector (the binary column's first 8193 rows) with every pool constant, successor and predecessor"""
    values = fx.columns["binary"].values[:8193]
    column, index = pa.array(values, pa.binary()), sc.index_values(values)
    for c in sc.edge_constants(fx, "binary"):
        for op in sc.OPS:
            assert np.array_equal(np.flatnonzero(sc.evaluate_indexed(index, op, c)), _arrow_rows(column, ("binary", op, c))), (op, c)
    assert set(sc.reduced_constants()) - {b"no row holds this value"} <= set(sc.edge_constants(fx, "binary"))
    assert [len(c) for c in sc.reduced_constants()[:4]] == [0, 5, 12, 13]


def test_successors_and_predecessors_are_neighbours_in_byte_order():
    values = sorted(set(sc.pool(False)) | set(sc.pool(True)))
    for v in values:
        s, p = sc.successor(v), sc.predecessor(v)
        assert s > v and not any(v < x < s for x in values)
        if v:
            assert p < v and not any(p < x < v for x in values)
    assert sc.predecessor(b"") is None
    # the prefix successor: popping 0xFF, then a carry-free increment
    assert sc.prefix_successor(b"ab\xff\xff") == b"ac" and sc.prefix_successor(b"\xff\xff") is None and sc.prefix_successor(b"") is None
    for p in (b"", b"k", b"kji\xff", b"\xff", b"\xff" * 12, sc.BASE[:12] + b"\xff", sc.BASE[:13]):
        up = sc.prefix_successor(p)
        for v in values:
            assert v.startswith(p) == (v >= p and (up is None or v < up)), (p, v)


ORACLE_ROWS = 2100   # the oracle's string evaluator is a Python loop over the rows: the first window and the next 52 rows


@pytest.mark.parametrize("kind", list(sc.COLUMN_KINDS))
def test_trees_in_conjunctive_form_equal_the_oracle(fx, kind):
    trees = sc.generated_trees(fx, kind) + [sc.delivery_cases()[kind]]
    assert len(trees) >= 40 and sum(sc.needs_distribution(t) for t in trees) >= 10 and all(sc.cnf_size(t)[1] <= 24 for t in trees)
    columns = {n: fx.columns[n].values[:ORACLE_ROWS] for n in fx.names(kind)}
    columns["q"] = (fx.q[:ORACLE_ROWS], sc.validity_words(fx.q_valid[:ORACLE_ROWS]))
    checked, kept = 0, []
    for expr in trees:
        kept.append(int(sc.evaluate(fx, expr).sum()))
        assert {c for c in sc._leaf_columns(expr)} <= set(fx.names(kind)) | {"q"}
        clauses = sc.cnf_of(expr)
        if clauses is None or checked >= 12:
            continue
        want = po.filter_cnf(clauses, columns, ORACLE_ROWS).tolist()
        assert np.flatnonzero(sc.evaluate(fx, expr)[:ORACLE_ROWS]).tolist() == want, expr
        checked += 1
    assert checked >= 8
    assert sum(1 for n in kept if 0 < n < sc.N_ROWS) >= 20   # most trees are neither empty nor everything
    assert sc.cnf_size(sc.refused_tree())[1] > 96


def test_single_leaves_equal_the_oracle(fx):
    """one column of every kind, every op, at the constants of the two seams"""
    for name in ("binary", "utf8", "fsb13", "dict_300", "ree_int16_utf8"):
        columns = {name: fx.columns[name].values[:ORACLE_ROWS]}
        for c in (b"", sc.BASE[:12], sc.BASE[:12] + b"\x00", sc.BASE[:12] + b"\x80", sc.BASE[:13], sc.BASE[:4] + b"\xff"):
            for op in sc.OPS:
                want = po.filter_cnf([[(name, op, c)]], columns, ORACLE_ROWS).tolist()
                assert np.flatnonzero(sc.evaluate(fx, (name, op, c))[:ORACLE_ROWS]).tolist() == want, (name, op, c)


# ---------------------------------------------------------------------------------------------------- the packer
@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_the_packer_round_trips_through_the_oracle(fx, layout):
    """po.strings_to_pylist resolves every packed row to the value it was made from; every pointer stays inside the heap"""
    placement, ptr_base = sc.LAYOUTS[layout]
    for n in (0, 1, 9, 8193):
        values = fx.columns["binary"].values[:n]
        images, heap, words = sc.pack_string_t(values, ptr_base, placement)
        assert images.shape == (n, 16) and len(words) == (n + 63) // 64
        assert po.strings_to_pylist(images.reshape(-1), words, n, heap, ptr_base, as_bytes=True) == values if n else True
        lens = images[:, 0:4].copy().view(np.uint32).reshape(-1)
        ptrs = images[:, 8:16].copy().view(np.uint64).reshape(-1)
        for i in np.flatnonzero(lens > 12):
            off = int(ptrs[i]) - ptr_base
            assert 0 <= off and off + int(lens[i]) <= len(heap)
        nulls = [i for i, v in enumerate(values) if v is None]
        assert not images[nulls].any()   # a NULL row holds no pointer
        if placement == "shuffled" and n == 8193:
            starts = {(int(ptrs[i]) - ptr_base) % 8 for i in np.flatnonzero(lens > 12)}
            assert starts == set(range(8))
            order = [int(ptrs[i]) for i in np.flatnonzero(lens > 12)]
            assert order != sorted(order)
    assert sc.FAR_BASE % 2 == 1 and sc.FAR_BASE > 1 << 63


@pytest.mark.parametrize("arrow_type", [pa.binary(), pa.large_binary()], ids=str)
def test_the_arrow_layout_equals_the_oracles_decode(fx, arrow_type):
    """one binary column through the oracle's decode, the pointer base given: the same sixteen bytes per row, the same validity
    words, and the heap is the Arrow data buffer"""
    ptr_base = sc.LAYOUTS["arrow"][1]
    for n in (1, 9, 2048, 8193):
        values = fx.columns["binary"].values[:n]
        sink = pa.BufferOutputStream()
        arr = pa.array(values, arrow_type)
        with ipc.new_stream(sink, pa.schema([("s", arrow_type)])) as w:
            w.write_batch(pa.record_batch([arr], names=["s"]))
        _, batches = po.decode_stream(sink.getvalue().to_pybytes(), ptr_base_of=lambda bi, body_off, boff: ptr_base)
        node = batches[0]["columns"][0]
        assert node["rc"] == 0
        images, heap, words = sc.pack_string_t(values, ptr_base, "arrow")
        assert np.array_equal(node["data"].reshape(-1, 16), images)
        assert np.array_equal(node["validity"], words)
        data = arr.buffers()[2]
        assert heap.tobytes() == (data.to_pybytes()[: len(heap)] if data is not None else b"")


# ---------------------------------------------------------------------------------------------------- non-vacuity
@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_every_op_and_every_family_separates_rows(fx, name):
    """For every op some constant keeps between 1 and n - 1 rows, and every family the column holds at least two values of has,
    among the constants that are its own members, one under which the op keeps a row of the family and one under which it
    drops a row of the family.  (dict_empty holds no value: there every comparison keeps nothing and IS NULL everything.)"""
    c = fx.columns[name]
    constants = sc.scan_constants(fx, name)
    distinct, codes = fx.index(name)
    if name == "dict_empty":
        assert all(not sc.evaluate(fx, (name, op, k)).any() for op in sc.OPS for k in constants)
        assert sc.evaluate(fx, (name, "is null")).all()
        return
    rows_of = {v: int((codes == i).sum()) for i, v in enumerate(distinct)}
    for op in sc.OPS + ("not starts_with",):
        assert any(0 < int(sc.evaluate(fx, (name, op, k)).sum()) < sc.N_ROWS - 1 for k in constants), (name, op)
        for fam, members in c.families.items():
            held = [v for v in members if rows_of.get(v, 0) > 0]
            if len(held) < 2:
                continue
            mine = [k for k in members if k in constants]
            assert any(sc.compare(v, op, k) for k in mine for v in held), (name, op, fam, "keeps none")
            assert any(not sc.compare(v, op, k) for k in mine for v in held), (name, op, fam, "drops none")


@pytest.mark.parametrize("name", ALL_COLUMNS)
def test_the_thinned_constants_keep_every_kind_of_sibling(fx, name):
    """scan_constants drops no kind of sibling: the prefix alone, + 0x00, 0x01, 0x7F, 0x80, 0xFF and 0xFF 0x00 (in text, U+0080,
    U+10FFFF and U+07FF 0x00 for the last three) each occur behind some prefix among the constants of every column"""
    constants = set(sc.scan_constants(fx, name))
    kinds = set()
    for text in (False, True):
        for fam, members in sc.families(text).items():
            if fam.startswith("siblings"):
                kinds.update(j for j, v in enumerate(members) if v in constants)
    assert kinds == set(range(len(sc.BINARY_TAILS))), (name, sorted(kinds))

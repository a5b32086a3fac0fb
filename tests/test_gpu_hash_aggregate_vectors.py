"""K11 at the kernel level (mi_hash_aggregate_vectors): hash_group_clear + hash_group_rows + hash_group_collect over resident
vectors built by hand -- key columns of every class and width, validity words, selection vectors, keys that collide by
construction -- against the dict loop of hash_agg_cases.py over Python ints.  Expected values never come from the library,
and every comparison is exact: the hash GROUP BY takes only merges that are exact in any order."""
import numpy as np
import pytest
import torch

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import hash_agg_cases as hc
from hash_agg_cases import W

pytestmark = pytest.mark.gpu

NMAX = 3 * W + 5      # 6149 rows: every row its own group is past MI_MAX_GROUPS = 4096


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


class Column(hc.HostColumn):
    """a HostColumn and its copies in HBM"""

    def __init__(self, values, cls, ok=None):
        super().__init__(values, cls, ok)
        self._data = _dev(self.np)
        self._valid = None if ok is None else _dev(hc.words(self.ok))

    def spec(self):
        return (self._data.data_ptr(), 0 if self._valid is None else self._valid.data_ptr(), self.width, self.cls)


class Selection:
    """per_window: the row numbers (inside the window) of every window; counts: what sel_count says, when it is not their
    number.  Slots never read hold a poison index."""

    def __init__(self, per_window, counts=None):
        self.per_window = per_window
        sel = np.full(len(per_window) * W, 0xFFFFFFFF, np.uint32)
        for w, rows in enumerate(per_window):
            sel[w * W: w * W + len(rows)] = rows
        self._sel, self._cnt = _dev(sel), _dev(np.array(counts if counts is not None else [len(r) for r in per_window], np.uint32))
        self.ptrs = (self._sel.data_ptr(), self._cnt.data_ptr())

    def rows(self):
        return [w * W + r for w, rows in enumerate(self.per_window) for r in rows]


def _spec(agg):
    def factor(f):
        if isinstance(f, Column):
            return f.spec()
        if isinstance(f, tuple) and isinstance(f[0], Column):
            return (f[0].spec(),) + tuple(f[1:])
        return f
    op, *args = agg
    return (op,) + tuple(factor(a) for a in args)


def run(ctx, key, aggs, nrows, max_groups, selection=None, **kw):
    sel_ptr, cnt_ptr = selection.ptrs if selection is not None else (0, 0)
    return da.hash_aggregate_vectors(ctx, key.spec(), [_spec(a) for a in aggs], nrows, max_groups, sel_ptr, cnt_ptr, detail=True, **kw)


def run_and_check(ctx, key, aggs, nrows, max_groups, selection=None, what=""):
    rows = selection.rows() if selection is not None else list(range(nrows))
    want = hc.reference(key, aggs, rows)
    got = run(ctx, key, aggs, nrows, max_groups, selection)
    hc.assert_same(got, want, what)
    return got


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2026)
    t = {}
    t["row"] = Column(np.arange(NMAX, dtype=np.int64) * 7 - 1000, "signed")              # every row its own group
    t["i64"] = Column(rng.integers(-(1 << 62), 1 << 62, NMAX), "signed", rng.random(NMAX) >= 0.15)
    t["i32"] = Column(rng.integers(-1000, 1000, NMAX).astype(np.int32), "signed")
    t["i16"] = Column(rng.integers(-32768, 32767, NMAX).astype(np.int16), "signed", rng.random(NMAX) >= 0.5)
    t["i8"] = Column(rng.integers(-128, 127, NMAX).astype(np.int8), "signed")
    t["big"] = Column(rng.integers(1 << 63, (1 << 64) - 1, NMAX, dtype=np.uint64, endpoint=True), "unsigned")    # lo wraps on every second add
    t["u64"] = Column(rng.integers(0, (1 << 64) - 1, NMAX, dtype=np.uint64), "unsigned", rng.random(NMAX) >= 0.15)
    t["u32"] = Column(rng.integers(0, (1 << 32) - 1, NMAX, dtype=np.uint32), "unsigned")
    t["u16"] = Column(rng.integers(0, 65535, NMAX).astype(np.uint16), "unsigned")
    t["u8"] = Column(rng.integers(0, 255, NMAX).astype(np.uint8), "unsigned", rng.random(NMAX) >= 0.1)
    f64 = rng.normal(0, 1, NMAX) * 10.0 ** rng.integers(-12, 13, NMAX)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0])
    f64[rng.integers(0, NMAX, 600)] = special[rng.integers(0, 6, 600)]
    t["f64"] = Column(f64, "float", rng.random(NMAX) >= 0.15)
    f32 = rng.normal(0, 1e3, NMAX).astype(np.float32)
    f32[rng.integers(0, NMAX, 600)] = special.astype(np.float32)[rng.integers(0, 6, 600)]
    t["f32"] = Column(f32, "float")
    t["k40"] = Column(rng.integers(-20, 20, NMAX).astype(np.int32), "signed", rng.random(NMAX) >= 0.1)         # few groups
    t["k900"] = Column(rng.integers(0, 900, NMAX).astype(np.uint16), "unsigned")
    return t


def _eight(t):
    return [("count_star",), ("count", t["f64"]), ("sum", t["big"]), ("sum", t["i64"]), ("sum_product", t["i32"], t["u64"]),
            ("min", t["f64"]), ("max", t["f32"]), ("sum_expr", (t["i32"], -3, 7), t["u16"], 5, (t["i8"], 1, 1))]


def _eight_more(t):
    return [("sum", t["i8"]), ("sum", t["u8"]), ("min", t["i64"]), ("max", t["u64"]), ("min", t["u8"]), ("max", t["i16"]),
            ("sum_expr", t["i64"]), ("sum_expr", t["i16"], t["i32"])]


def _third(t):
    return [("max", t["f64"]), ("min", t["f32"]), ("min", t["u32"]), ("max", t["i8"]), ("sum_product", t["i16"], t["i16"]),
            ("sum_expr", t["u64"], (None, -2), t["i32"]), ("count", t["u8"]), ("sum", t["u32"])]


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 2047, 2048, 2049, NMAX])
def test_every_row_its_own_group_at_the_row_count_seams(ctx, table, nrows):
    aggs = [("count_star",), ("sum", table["i64"]), ("max", table["i32"])]
    got = run_and_check(ctx, table["row"], aggs, nrows, max_groups=nrows, what="nrows %d" % nrows)
    assert len(got) == nrows


def test_more_groups_than_k10_takes_is_the_gap_this_closes(ctx, table):
    """6149 groups: mi_group_aggregate_vectors refuses them (its limits stand), mi_hash_aggregate_vectors answers"""
    with pytest.raises(da.MiError) as e:
        da.group_aggregate_vectors(ctx, [table["row"].spec()], [("count_star",)], NMAX)
    assert e.value.code == _ffi.MI_ENOTSUP and "stays above the scan" in str(e.value)
    assert NMAX > _ffi.MAX_GROUPS
    got = run_and_check(ctx, table["row"], [("count_star",)], NMAX, max_groups=NMAX)
    assert len(got) == NMAX


@pytest.mark.parametrize("with_validity", [False, True])
@pytest.mark.parametrize("name", sorted(hc.INT_TYPES))
def test_key_classes_widths_and_edges(ctx, table, name, with_validity):
    """0, the type's minimum and maximum, the empty mark with its neighbours, NULL keys with garbage under them"""
    rng = np.random.default_rng(sum(map(ord, name)) * 2 + with_validity)
    edges = hc.type_edges(name)
    n = W + 77
    vals = edges[rng.integers(0, len(edges), n)]
    info = np.iinfo(hc.INT_TYPES[name])
    some = rng.integers(max(info.min, -50), min(info.max, 50), n, endpoint=True).astype(hc.INT_TYPES[name])
    vals = np.where(rng.random(n) < 0.5, vals, some)
    vals[: len(edges)] = edges
    ok = None
    if with_validity:
        ok = rng.random(n) >= 0.2
        ok[: len(edges)] = True
        vals[~ok] = edges[rng.integers(0, len(edges), int((~ok).sum()))]      # garbage under the NULLs: other groups' keys
    key = Column(vals, "unsigned" if name.startswith("u") else "signed", ok)
    got = run_and_check(ctx, key, [("count_star",), ("sum", table["i32"]), ("min", table["u16"])], n, max_groups=256, what=name)
    keys = [g[0][0] for g in got]
    assert set(int(v) for v in edges) <= set(keys) and (None in keys) == with_validity


def test_u64_keys_come_back_zero_extended(ctx, table):
    key = Column(np.array([(1 << 64) - 1, (1 << 64) - 2, 0, 1 << 63], np.uint64), "unsigned")
    raw = da.hash_aggregate_vectors(ctx, key.spec(), [("count_star",)], 4, 16)
    # _group_key_value reads the 16 bytes as a signed 128-bit integer: zero extension keeps 2^64 - 1 positive
    assert [k[0] for k, _ in raw] == [0, 1 << 63, (1 << 64) - 2, (1 << 64) - 1]


@pytest.mark.parametrize("home", [63, 0])
def test_colliding_keys_fill_the_table_and_one_more_is_refused(ctx, table, home):
    """max_groups = 32 -> 64 slots.  32 keys with one home slot: from the last slot the probe wraps around the table's end;
    from slot 0 it is one chain.  Exactly max_groups keys succeed; one more is the limit error, and the call fails cleanly."""
    assert hc.slots_for(32) == 64
    keys = hc.keys_in_slot(home, 64, 33)
    rng = np.random.default_rng(home)
    n = W + 300
    pick = rng.integers(0, 32, n)
    pick[:32] = np.arange(32)
    full = Column(np.array(keys[:32], np.int64)[pick], "signed")
    got = run_and_check(ctx, full, _eight(table), n, max_groups=32, what="home %d" % home)
    assert len(got) == 32
    over = full.np.copy()
    over[n - 1] = keys[32]
    with pytest.raises(da.MiError) as e:
        run(ctx, Column(over, "signed"), [("count_star",)], n, 32)
    assert e.value.code == _ffi.MI_ENOTSUP and "max_groups = 32" in str(e.value)
    # the context is as good as before
    assert len(run_and_check(ctx, full, [("count_star",)], n, max_groups=32)) == 32


def test_max_groups_counts_the_null_key_and_the_empty_mark(ctx, table):
    key = Column(np.array([-1, 5, 0, -1, 5], np.int64), "signed", [True, True, False, True, True])      # -1 is the empty mark
    assert len(run_and_check(ctx, key, [("count_star",)], 5, max_groups=3)) == 3
    with pytest.raises(da.MiError) as e:
        run(ctx, key, [("count_star",)], 5, 2)
    assert e.value.code == _ffi.MI_ENOTSUP and "max_groups = 2" in str(e.value)


@pytest.mark.parametrize("shape", ["one_group", "two_alternating", "all_null"])
def test_contention(ctx, table, shape):
    """every row into one record, or two: the carry of the uint64 sums is exercised in every lane at once"""
    if shape == "one_group":
        key = Column(np.full(NMAX, 42, np.int64), "signed")
    elif shape == "two_alternating":
        key = Column((np.arange(NMAX) % 2).astype(np.uint8), "unsigned")
    else:
        key = Column(np.arange(NMAX, dtype=np.int32), "signed", np.zeros(NMAX, bool))
    for aggs in (_eight(table), _eight_more(table)):
        got = run_and_check(ctx, key, aggs, NMAX, max_groups=4, what=shape)
        assert len(got) == (2 if shape == "two_alternating" else 1)
    if shape == "one_group":      # the sum of 6149 values of 2^63 .. 2^64 - 1 is far past 64 bits: hi counts lo's wraps
        total = run(ctx, key, [("sum", table["big"])], NMAX, 4)[0][1][0][0]
        assert total == sum(table["big"].py) and total >> 64 > 3000


@pytest.mark.parametrize("aggs", [_eight, _eight_more, _third], ids=["eight", "eight_more", "third"])
@pytest.mark.parametrize("key", ["k40", "k900", "row"])
def test_every_operation_over_every_class(ctx, table, key, aggs):
    run_and_check(ctx, table[key], aggs(table), NMAX, max_groups=NMAX, what=key)


def test_a_group_whose_aggregate_column_is_null_throughout_is_present(ctx, table):
    n = 500
    key = Column((np.arange(n) % 5).astype(np.int16), "signed")
    ok = (np.arange(n) % 5) != 3
    val = Column(np.arange(n, dtype=np.int64) - 250, "signed", ok)
    fl = Column(np.arange(n, dtype=np.float64), "float", ok)
    aggs = [("sum", val), ("min", val), ("max", fl), ("count", val), ("count_star",), ("sum_expr", val, 2)]
    got = run_and_check(ctx, key, aggs, n, max_groups=8)
    assert got[3] == ((3,), [(None, 0), (None, 0), (None, 0), (0, 0), (100, 100), (None, 0)])


def test_selection_vectors(ctx, table):
    rng = np.random.default_rng(5)
    tail = NMAX - 3 * W
    per_window = [sorted(rng.choice(W, 700, replace=False).tolist()), [], rng.permutation(W).tolist(), [4, 0, 2]]
    assert tail == 5
    run_and_check(ctx, table["row"], _eight(table), NMAX, NMAX, Selection(per_window), "mixed windows")
    run_and_check(ctx, table["k40"], _eight_more(table), NMAX, 64, Selection([[], [], [], []]), "nothing selected")
    # a count past the window's rows is clamped to them: the last window has 5 rows, its count says 2048
    clamped = Selection([[1], [], [], [0, 1, 2, 3, 4]], counts=[1, 0, 0, 2048])
    run_and_check(ctx, table["row"], [("count_star",), ("sum", table["i64"])], NMAX, 16, clamped, "clamped")
    # one index past its window: skipped, never dereferenced, and the call fails
    for bad in ([0, 5], [W - 1 + 1]):
        with pytest.raises(da.MiError) as e:
            run(ctx, table["row"], [("count_star",)], NMAX, 16, Selection([[1], [], [], bad]))
        assert e.value.code == _ffi.MI_EINVAL and "selection index" in str(e.value)
    with pytest.raises(da.MiError) as e:
        run(ctx, table["row"], [("count_star",)], NMAX, 16, Selection([[0xFFFFFFFF], [], [], []]))
    assert e.value.code == _ffi.MI_EINVAL


def test_the_same_call_twice_gives_the_same_bytes(ctx, table):
    a = run(ctx, table["k900"], _eight(table), NMAX, 1024)
    b = run(ctx, table["k900"], _eight(table), NMAX, 1024)
    assert len(a) == len(set(table["k900"].py)) > 800 and repr(a) == repr(b)
    c = run(ctx, table["k900"], _eight(table), NMAX, 1 << 16)      # another table size, other slots: the same result
    assert repr(a) == repr(c)


def test_agreement_with_k10_bit_for_bit(ctx, table):
    for key in ("k40", "u8"):
        for aggs in (_eight(table), _eight_more(table), _third(table)):
            specs = [_spec(a) for a in aggs]
            k10 = da.group_aggregate_vectors(ctx, [table[key].spec()], specs, NMAX, detail=True)
            k11 = da.hash_aggregate_vectors(ctx, table[key].spec(), specs, NMAX, 256, detail=True)
            assert len(k10) <= 256 and repr(k10) == repr(k11)


def test_capacity_too_small_sets_the_group_count(ctx, table):
    L = _ffi.lib()
    kcol = _ffi.GroupKeyColumn()
    kcol.data, kcol.validity, kcol.width, kcol.key_class = table["k900"].spec()[0], None, 2, _ffi.GROUP_KEY_CLASS_UNSIGNED
    spec = (_ffi.AggVectorSpec * 1)()
    spec[0].op = _ffi.AGG_COUNT_STAR
    out_k, out_v = (_ffi.GroupKeyValue * 10)(), (_ffi.AggValue * 10)()
    import ctypes as C
    n = C.c_int32(-1)
    rc = L.mi_hash_aggregate_vectors(ctx._h, C.byref(kcol), spec, 1, None, None, NMAX, 1024, out_k, out_v, 10, C.byref(n), None)
    assert rc == _ffi.MI_EINVAL and n.value == len(set(table["k900"].py)) > 10


def test_refusals(ctx, table):
    wide = Column([1 << 100, -5, 7], "wide")
    strings = Column([1, 2, 3], "wide")
    strings.cls = "string"
    f = Column(np.array([1.5, 2.5, 3.5]), "float")
    k = Column(np.array([1, 2, 3], np.int32), "signed")
    i = Column(np.array([1, 2, 3], np.int64), "signed")
    for key, what in ((wide, "a 16-byte key"), (strings, "a VARCHAR / BLOB key")):
        with pytest.raises(da.MiError) as e:
            run(ctx, key, [("count_star",)], 3, 8)
        assert e.value.code == _ffi.MI_ENOTSUP and what in str(e.value) and "mi_scan_group_aggregate takes" in str(e.value) and "few groups" in str(e.value)
    for agg in (("sum", f), ("sum_product", f, f), ("sum_expr", f, 2.0)):
        with pytest.raises(da.MiError) as e:
            run(ctx, k, [("count_star",), agg], 3, 8)
        assert e.value.code == _ffi.MI_ENOTSUP and "arrival order" in str(e.value) and "aggregate 1" in str(e.value)
    for op in ("min", "max"):
        with pytest.raises(da.MiError) as e:
            run(ctx, k, [(op, wide)], 3, 8)
        assert e.value.code == _ffi.MI_ENOTSUP and "128-bit atomic" in str(e.value)
    with pytest.raises(da.MiError) as e:      # a key width that is no integer's
        da.hash_aggregate_vectors(ctx, (k.spec()[0], 0, 3, "signed"), [("count_star",)], 3, 8)
    assert e.value.code == _ffi.MI_EINVAL and "does not fit" in str(e.value)
    # what it takes of the same columns
    assert run(ctx, k, [("min", f), ("count", wide), ("sum", i)], 3, 8)[0] == ((1,), [(1.5, 1), (1, 1), (1, 1)])

"""K6 at the program level (mi_filter_program_vectors): filter_program<EXT, PAT> on hand-built programs over resident vectors,
programs mi_scan_set_filter's front end never emits among them -- ranges on one column it would merge, contradictions, lo > hi,
kLeafNegate on every leaf form, validity pointers present and absent in one program, 24 leaves in one clause.

Columns, constant tables, programs and the expected rows come from tests/filter_program_cases.py, whose evaluator is numpy and
Python over the leaves' meanings and is itself held to the older evaluators by tests/test_filter_program_reference_host.py.
Every comparison is exact: per window the count, the ascending window-relative rows, the sentinel in every slot behind them,
and an untouched guard window and guard count behind the last window.  Every data buffer is 2048 + 64 rows longer than nrows
(rows that repeat the column's first rows, pad validity bits set), so a read past the last row shows as a wrong row."""

import numpy as np
import pytest

import duckdb_arrow_amd as da
import filter_program_cases as pc
import filter_string_cases as sc
from duckdb_arrow_amd import _ffi

pytestmark = pytest.mark.gpu

L = pc.L


class Resident:
    """the columns of one shape in HBM: data at 0 or 8 bytes past a 64-byte boundary, validity words, heaps, outputs"""

    def __init__(self, ctx, nrows, offset=0):
        import torch
        self.torch, self.ctx, self.nrows, self.cols = torch, ctx, nrows, pc.columns(nrows)
        self.keep = []
        self.data, self.heap, self.valid = {}, {}, {}
        for name, c in self.cols.col.items():
            if c.kind == "str":
                ok = self.cols.valid[name]
                images, heap, _ = sc.pack_string_t([v if o else None for v, o in zip(c.values, ok)], c.ptr_base, c.layout)
                raw = images.reshape(-1)
                heap = np.concatenate([heap, np.full((-len(heap)) % 8 + 8, 0xA5, np.uint8)])     # padded to 8 bytes
                self.heap[name] = self._upload(heap, 0)
            elif c.kind == "wide":
                raw = np.array([[v & (pc.P64 - 1), (v >> 64) & (pc.P64 - 1)] for v in c.values], np.uint64).view(np.uint8).reshape(-1)
            else:
                raw = np.ascontiguousarray(c.values).view(np.uint8).reshape(-1)
            self.data[name] = self._upload(raw, offset)
            assert self.data[name] % 64 == offset and self.data[name] % 16 == offset % 16
        for name, ok in self.cols.valid.items():
            self.valid[name] = self._upload(pc.validity_words(ok).view(np.uint8), 0)
        self.windows = (nrows + pc.WINDOW - 1) // pc.WINDOW
        self.sel = torch.empty(((self.windows + 1) * pc.WINDOW,), dtype=torch.int32, device="cuda")
        self.cnt = torch.empty((self.windows + 1,), dtype=torch.int32, device="cuda")

    def _upload(self, raw, offset):
        """`raw` at `offset` bytes into an allocation of its own (64 spare bytes of 0xEE around it); -> the device address"""
        buf = np.full(len(raw) + 128, 0xEE, np.uint8)
        buf[offset: offset + len(raw)] = raw
        t = self.torch.from_numpy(buf).cuda()
        self.keep.append(t)
        assert t.data_ptr() % 64 == 0
        return t.data_ptr() + offset

    def leaves(self, program):
        """(the mi_filter_vector_leaf dicts of a program, the tensor that holds its constant tables)"""
        flat = [(leaf, i == len(clause) - 1) for clause in program for i, leaf in enumerate(clause)]
        sizes = [len(t) if t is not None else 0 for t in (pc.table_image(leaf, self.cols, 0) for leaf, _ in flat)]
        starts = np.concatenate([[0], np.cumsum([(s + 7) & ~7 for s in sizes])]).astype(np.int64)
        tables = self.torch.empty((int(starts[-1]) + 8,), dtype=self.torch.uint8, device="cuda")
        host = np.full(int(starts[-1]) + 8, 0xEE, np.uint8)
        out = []
        for (leaf, ends), size, start in zip(flat, sizes, starts):
            address = 0
            if size:
                address = tables.data_ptr() + int(start)      # the addresses a table holds come from its own allocation
                host[start: start + size] = pc.table_image(leaf, self.cols, address)
            name = leaf.get("col")
            out.append(pc.device_fields(leaf, self.cols, ends, self.data[name], self.valid[leaf["validity"]] if leaf.get("validity") else 0, address,
                                        heap=self.heap.get(name, 0)))
        tables.copy_(self.torch.from_numpy(host))
        return out, tables

    def launch(self, program, nrows=None, refill=True, stream=0):
        """one launch; -> (sel, counts) on the host"""
        torch = self.torch
        leaves, tables = self.leaves(program)
        if refill:
            self.sel.fill_(pc.SENTINEL)
            self.cnt.fill_(pc.SENTINEL)
        torch.cuda.synchronize()          # tables and sentinels are in place before the kernel runs on another stream
        da.filter_program(self.ctx, leaves, self.nrows if nrows is None else nrows, self.sel.data_ptr(), self.cnt.data_ptr(), stream=stream)
        torch.cuda.synchronize()          # the call does not wait
        del tables
        return self.sel.cpu().numpy(), self.cnt.cpu().numpy()

    def check(self, program, what=()):
        sel, cnt = self.launch(program)
        return pc.check_outputs(sel, cnt, pc.evaluate(program, self.cols, self.nrows), self.nrows, tuple(what))


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def resident(ctx):
    """Resident(nrows, offset), built once per shape"""
    made = {}

    def get(nrows, offset=0):
        if (nrows, offset) not in made:
            made[(nrows, offset)] = Resident(ctx, nrows, offset)
        return made[(nrows, offset)]
    yield get
    made.clear()


def _launches():
    base, ext = da.filter_launch_counts()
    return np.array([base, ext, da.filter_pattern_launches()])


# ---------------------------------------------------------------------------------------------------- the empty program
@pytest.mark.parametrize("nrows", pc.SHAPES)
def test_the_empty_program_keeps_every_row(resident, nrows):
    """no leaf: the initial acc mask alone, ragged for the 1 .. 7 rows of a last lane, every window's rows 0 .. n - 1"""
    assert resident(nrows).check([]) == nrows


# ---------------------------------------------------------------------------------------------------- clause logic
@pytest.mark.parametrize("nrows", pc.RANDOM_SHAPES)
def test_random_cnfs(resident, nrows):
    """seeded CNFs of 1 .. 24 leaves in 1 .. 24 clauses over every column and leaf form, validity pointers on some leaves and
    none on others: clause |= m, acc &= clause on kLeafEndsClause (non-vacuity is asserted on the reference by the host test)"""
    r = resident(nrows)
    kept = [r.check(program, (i,)) for i, (n, program) in enumerate(pc.random_programs()) if n == nrows]
    assert len(kept) == len(pc.random_programs()) // len(pc.RANDOM_SHAPES) and any(0 < k < nrows for k in kept)


def test_24_leaves_in_one_clause_and_24_clauses_of_one_leaf(resident):
    one = [(n, p) for n, p in pc.random_programs() if len(p) == 1 and len(p[0]) == 24]
    many = [(n, p) for n, p in pc.random_programs() if len(p) == 24 and all(len(c) == 1 for c in p)]
    assert one and many
    for n, p in one + many:
        resident(n).check(p)
    # the same at the other end of the pass rates: 24 clauses every row passes, one clause of 24 leaves no row passes
    r = resident(2049)
    assert r.check([[L("i32", pc.RANGE, validity=None, lo=-pc.P63, hi=pc.P63 - 1)] for _ in range(24)]) == 2049
    assert r.check([[L("i32", pc.RANGE, lo=5, hi=-5) for _ in range(24)]]) == 0
    want = int(pc.columns(2049).valid["i32"][:2049].sum())
    assert r.check([[L("i32", pc.RANGE, lo=5, hi=-5) for _ in range(23)] + [L("i32", pc.IS_NOT_NULL)]]) == want


# ---------------------------------------------------------------------------------------------------- what the normaliser cannot emit
@pytest.mark.parametrize("nrows", pc.SMALL_SHAPES)
def test_programs_the_normaliser_cannot_emit(resident, nrows):
    """ranges on one column in separate clauses (overlapping, touching, contradictory), a leaf twice in a clause, lo > hi,
    kLeafNegate on IN, wide, string, pattern and float leaves with NaN bounds, IN-lists of 0, 1 and 256 values, uint64 ranges
    under kLeafBias at 0, 2^63 - 1, 2^63 and 2^64 - 1, kLeafUnsigned alone at the maxima of widths 1, 2 and 4"""
    r = resident(nrows)
    kept = {name: r.check(program, (name,)) for name, program in pc.unemitted_programs()}
    assert kept["contradictory"] == 0 and kept["lo > hi, no validity negated"] == nrows
    assert nrows < 64 or sum(1 for k in kept.values() if 0 < k < nrows) > len(kept) // 2


# ---------------------------------------------------------------------------------------------------- validity
@pytest.mark.parametrize("nrows", pc.SMALL_SHAPES)
def test_validity(resident, nrows):
    """the same leaf under all-valid words, no pointer, all-NULL words and a bitmap with NULLs on the last row and on both
    sides of every word seam; IS NULL under no pointer keeps nothing, IS NULL OR <comparison> keeps the NULL rows, a negated
    leaf keeps no NULL row (the host test asserts those on the reference; here the kernel equals the reference)"""
    r = resident(nrows)
    kept = {name: r.check(program, (name,)) for name, program in pc.validity_programs()}
    for leaf in pc.VALIDITY_LEAVES:
        col = leaf["col"]
        assert kept["%s under None: is null" % col] == 0 and kept["%s under all_null" % col] == 0 and kept["%s under all_null negated" % col] == 0
        assert kept["%s under all_valid" % col] == kept["%s under None" % col]
        assert kept["%s under all_null: is null or" % col] == nrows


# ---------------------------------------------------------------------------------------------------- kLeafDictMap
@pytest.mark.parametrize("nrows", pc.SMALL_SHAPES)
def test_dictionary_maps(resident, nrows):
    """modes 0 .. 3; indices n_in - 1, n_in and 0xFFFFFFFF; a validity pointer of all-zero words changes nothing; behind the
    map lie bytes that would pass"""
    r = resident(nrows)
    idx = r.cols.col["dict"].values[:nrows]
    assert nrows < 3 or {pc.DICT_ENTRIES - 1, pc.DICT_ENTRIES, 0xFFFFFFFF} <= set(idx.tolist())
    kept = {name: r.check(program, (name,)) for name, program in pc.dict_map_programs()}
    for mode in range(4):
        for j in range(5):
            assert len({kept["dict map %d, mode %d, under %s" % (j, mode, b)] for b in (None, "dict", "all_null")}) == 1
    assert kept["dict map 4, mode 2, under None"] == nrows and kept["dict map 4, mode 3, under None"] == 0     # an empty map: every index is past it


# ---------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("nrows", (9, 2049, 8193))
def test_data_at_8_bytes_past_a_64_byte_boundary(resident, nrows):
    """what an aliased Arrow buffer gives: every width starting at 8 mod 64, 16-byte rows at 8 mod 16"""
    r = resident(nrows, offset=8)
    programs = [(name, p) for name, p in pc.unemitted_programs() if not name.endswith(" negated")] + [(n, p) for n, p, _ in pc.instance_programs()]
    programs += [("random %d" % i, p) for i, (n, p) in enumerate(pc.random_programs()) if n == nrows][:8]
    assert {c for _, p in programs for clause in p for c in (leaf["col"] for leaf in clause)} == set(r.cols.col)
    for name, p in programs:
        r.check(p, (name,))


# ---------------------------------------------------------------------------------------------------- instances
def test_the_instance_a_program_launches(resident):
    """integer, string and dictionary leaves launch filter_program<false>; one float or one wide leaf more filter_program<true>;
    one kLeafStrMatch leaf more filter_program<true, true>; the rows are the reference's under each"""
    for nrows in (65, 2049, 8193):
        r = resident(nrows)
        kept = set()
        for name, program, instance in pc.instance_programs():
            before = _launches()
            kept.add(r.check(program, (name,)))
            delta = _launches() - before
            assert delta.tolist() == [int(i == instance) for i in range(3)], (name, delta)
        assert len(kept) == 1 and 0 < kept.pop() < nrows
    for nrows in (2049,):        # every leaf form alone under the widest instance
        r = resident(nrows)
        for name, program in pc.unemitted_programs()[::7]:
            before = _launches()
            r.check(program + [[pc.neutral_leaf("pattern")]], (name, "+ pattern"))
            assert (_launches() - before).tolist() == [0, 0, 1]


# ---------------------------------------------------------------------------------------------------- outputs
@pytest.mark.parametrize("nrows", pc.SHAPES)
def test_output_positions_at_every_shape(resident, nrows):
    """a program that keeps about half of the rows, one that keeps the last row alone, one that keeps all but the last: the
    positions across the four windows of a workgroup and the workgroups behind it, sentinels and guards"""
    r = resident(nrows)
    kept = r.check(pc.base_program())
    assert nrows < 65 or 0 < kept < nrows
    top = int(r.cols.col["i64"].values[nrows - 1])
    assert r.check([[L("i64", pc.RANGE, validity="last", lo=top, hi=top)]]) == 1
    assert r.check([[L("i64", pc.IS_NULL, validity="last")]]) == nrows - 1


def test_zero_rows_touch_nothing(resident):
    r = resident(9)
    for program in ([], pc.base_program()):
        sel, cnt = r.launch(program, nrows=0)
        assert (sel == pc.SENTINEL).all() and (cnt == pc.SENTINEL).all()


def test_leaves_as_tuples(resident):
    """da.filter_program takes a leaf as a tuple in the struct's field order too"""
    import torch
    r = resident(65)
    program = pc.base_program()
    leaves, tables = r.leaves(program)
    fields = ("data", "validity", "in_values", "lo", "hi", "op", "width", "flags", "n_in")
    r.sel.fill_(pc.SENTINEL)
    r.cnt.fill_(pc.SENTINEL)
    torch.cuda.synchronize()
    da.filter_program(r.ctx, [tuple(leaf[f] for f in fields) for leaf in leaves], r.nrows, r.sel.data_ptr(), r.cnt.data_ptr())
    torch.cuda.synchronize()
    del tables
    pc.check_outputs(r.sel.cpu().numpy(), r.cnt.cpu().numpy(), pc.evaluate(program, r.cols, r.nrows), r.nrows)


def test_two_launches_into_the_same_buffers_give_the_same_bytes(resident):
    """the second launch overwrites what the first wrote with the same values and nothing else, on the context's stream and
    on a stream of the caller's"""
    import torch
    program = pc.base_program() + [[pc.neutral_leaf("float")]]
    r = resident(5 * 2048 + 5)
    first = [a.copy() for a in r.launch(program)]
    for stream in (0, torch.cuda.Stream().cuda_stream):
        second = r.launch(program, refill=False, stream=stream)
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    pc.check_outputs(first[0], first[1], pc.evaluate(program, r.cols, r.nrows), r.nrows)
    other = r.launch([], refill=False)                   # and a program that keeps more rows leaves none of the old ones behind
    pc.check_outputs(other[0], other[1], np.ones(r.nrows, bool), r.nrows)


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(ctx, r, leaves, match, n_leaves=None):
    arr = (_ffi.FilterVectorLeaf * max(len(leaves), 1))()
    for slot, leaf in zip(arr, leaves):
        for k, v in leaf.items():
            setattr(slot, k, (v or None) if k in ("data", "validity", "in_values") else v)
    rc = _ffi.lib().mi_filter_program_vectors(ctx._h, arr, len(leaves) if n_leaves is None else n_leaves, r.nrows, r.sel.data_ptr(), r.cnt.data_ptr(), None)
    assert rc == _ffi.MI_EINVAL, (match, rc)
    with pytest.raises(da.MiError, match=match) as e:
        _ffi.check(rc)
    assert e.value.code == _ffi.MI_EINVAL


def test_refusals(ctx, resident):
    """every validation is MI_EINVAL and names the leaf; nothing is launched and nothing written; the context then runs a good
    program"""
    r = resident(2049)
    r.sel.fill_(pc.SENTINEL)
    r.cnt.fill_(pc.SENTINEL)
    good = r.leaves([[L("i32", pc.RANGE, lo=-1, hi=1)]])[0][0]
    tables = [r.leaves(p) for p in ([[L("i16", pc.IN, values=[1, 2])]], [[L("hug", pc.WIDE_IN, values=[1])]], [[L("s_arrow", pc.STR_IN, values=[b"a"])]],
                                    [[L("s_arrow", pc.STR_RANGE, lower=b"a", lo_incl=True, upper=None, hi_incl=False)]],
                                    [[L("s_arrow", pc.STR_MATCH, segments=[b"a"], head=False, tail=False)]],
                                    [[L("dict", pc.DICT_MAP, map=np.ones(4, np.uint8), mode=0, validity=None)]], [[L("hug", pc.WIDE_RANGE, lo=0, hi=1)]],
                                    [[L("f32", pc.RANGE, lo=0.0, hi=1.0)]], [[L("i32", pc.IS_NULL)]])]
    in_leaf, wide_in, str_in, str_range, str_match, dict_map, wide_range, float_range, is_null = (t[0][0] for t in tables)
    before = _launches()
    second = lambda leaf: [good_open, leaf]
    good_open = dict(good, flags=good["flags"] & ~pc.F_ENDS_CLAUSE)
    _refused(ctx, r, [good] * 25, "0 to 24 leaves")
    _refused(ctx, r, [good], "0 to 24 leaves", n_leaves=-1)
    _refused(ctx, r, second(good_open), "leaf 1: the last leaf does not end its clause")
    for op in (0, 11, -1):
        _refused(ctx, r, second(dict(good, op=op)), "leaf 1: unknown op")
    for leaf in (good, in_leaf, str_in, str_range, str_match, dict_map, wide_range, wide_in, float_range):
        _refused(ctx, r, second(dict(leaf, data=0)), "leaf 1: NULL data")
    for leaf, widths in ((good, (0, 3, 16)), (in_leaf, (16, -4)), (float_range, (1, 2, 16)), (wide_range, (8,)), (wide_in, (4,)), (str_in, (8,)), (str_range, (4,)),
                         (str_match, (8,)), (dict_map, (8, 16, 1))):
        for w in widths:
            _refused(ctx, r, second(dict(leaf, width=w)), "leaf 1: width")
    for leaf in (in_leaf, str_in, str_range, str_match, dict_map, wide_range, wide_in):
        _refused(ctx, r, second(dict(leaf, in_values=0)), "leaf 1: NULL in_values")
    for leaf in (in_leaf, str_in, wide_in):
        _refused(ctx, r, second(dict(leaf, n_in=257)), "leaf 1: more than 256")
    for leaf in (in_leaf, str_in, wide_in, dict_map, good):
        _refused(ctx, r, second(dict(leaf, n_in=-1)), "leaf 1: negative n_in")
    for mode in (-1, 4):
        _refused(ctx, r, second(dict(dict_map, lo=mode)), "leaf 1: dictionary map mode")
    for leaf in (dict_map, is_null, dict(is_null, op=pc.IS_NOT_NULL)):
        _refused(ctx, r, second(dict(leaf, flags=leaf["flags"] | pc.F_NEGATE)), "leaf 1: MI_FLF_NEGATE")
    for shift in (1, 2, 4):
        _refused(ctx, r, second(dict(good, data=good["data"] + shift)), "leaf 1: data is not 8-byte aligned")
        _refused(ctx, r, second(dict(good, validity=good["validity"] + shift)), "leaf 1: validity is not 8-byte aligned")
        _refused(ctx, r, [dict(is_null, validity=is_null["validity"] + shift)], "leaf 0: validity is not 8-byte aligned")
    for n_in in (0, 9, 0x401):   # what the launcher refuses: a pattern of no segment, of nine, of a bit it does not know
        _refused(ctx, r, second(dict(str_match, n_in=n_in)), "leaf 1: a pattern leaf")
    assert (_launches() == before).all()
    import torch
    torch.cuda.synchronize()
    assert (r.sel.cpu().numpy() == pc.SENTINEL).all() and (r.cnt.cpu().numpy() == pc.SENTINEL).all()
    assert 0 < r.check(pc.base_program()) < r.nrows           # the context is as good as before
    del tables

"""The union kernels (transcode_union and transcode_union_dense, kernels_union.hip) at the task level: hand-built
MI_K_UNION / MI_K_UNION_DENSE tasks through mi_plan -- the contract in mi_arrow_ipc.h -- against
union_cases.union_reference (numpy, held to pyarrow in test_union_reference_host.py).

Per task (union_cases.check_union_case): every tag, the sentinel bytes behind the tags, the union's validity words between
two guard words, every member's mask and the guard word behind it (pad bits of every word ones), and for a dense union every
member vector (the value where its mask selects, zero elsewhere), its sentinel tail, its words and their guard word.  Type
ids and offsets are followed by entries no member owns (-9; 2^31 - 1), member arrays by POISON rows: a read past a buffer is
a wrong row, never an access outside an allocation.  No input here makes the device fault: every damaged value is one the
kernel must refuse before it uses it."""
import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import union_cases as uc
from union_cases import WIN

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 4099]
WIDTHS = (1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run_and_check(ctx, torch, cases, **kw):
    got, status = uc.run_union_plan(ctx, torch, cases, **kw)
    for c, g in zip(cases, got):
        uc.check_union_case(c, g, out_validity=kw.get("out_validity", True))
    assert status == 0, status
    return got


def _codes(m):
    """m type ids that are not their own indices: 127 first, then descending odd steps"""
    return [127 - 3 * k for k in range(m)]


def _members(mode, m, n, rng, *, nulls=True, widths=(4,), null_count=-1):
    """sparse: m arrays of n rows; dense: lengths 5, 42, 79 ... (shorter than most unions here: rows share child rows)"""
    out = []
    for k in range(m):
        length = n if mode == "sparse" else 5 + 37 * k
        out.append(uc.make_member(length, widths[k % len(widths)], rng, nulls=nulls and k % 2 == 0, null_count=null_count))
    return out


def _case(mode, m, n, rng, *, row_offset=0, parent=False, absent=(), name="", **kw):
    members = _members(mode, m, n + (row_offset if mode == "sparse" else 0), rng, **kw)
    if mode == "sparse":
        for mem in members:       # a sparse member is as long as the union: row_offset + n bits of its bitmap count
            mem["length"] = n
    codes = _codes(m)
    ids, offs = uc.random_rows(mode, codes, members, n, rng, absent)
    return uc.make_union_case(mode, codes, members, ids, offs, row_offset=row_offset, parent=uc.parent_words(n, rng) if parent else None, name=name)


@pytest.mark.parametrize("mode", ["sparse", "dense"])
@pytest.mark.parametrize("m", [1, 2, 32])
def test_row_counts_and_member_counts(ctx, torch, mode, m):
    rng = np.random.default_rng(100 + m)
    cases = [_case(mode, m, n, rng, name="rows") for n in ROW_COUNTS]
    for c in cases:
        ref = uc.case_reference(c)
        assert ref["status"] == 0 and (ref["valid"].any() or c["nrows"] < 64)
    _run_and_check(ctx, torch, cases)


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_a_tile_without_one_member_and_a_tile_of_one_tag(ctx, torch, mode):
    """rows 0 .. 2047 never select member 1; rows 2048 .. 4095 all select member 2; the last 3 rows are mixed"""
    rng = np.random.default_rng(110)
    n, m = 2 * WIN + 3, 4
    c = _case(mode, m, n, rng, name="tiles")
    tag = np.concatenate([rng.choice([0, 2, 3], WIN), np.full(WIN, 2), rng.integers(0, m, 3)])
    ids = np.asarray(c["codes"], np.int8)[tag]
    offs = None if mode == "sparse" else np.array([rng.integers(0, c["members"][k]["length"]) for k in tag], np.int32)
    c = uc.make_union_case(mode, c["codes"], c["members"], ids, offs, name="tiles")
    ref = uc.case_reference(c)
    assert not ref["member_ok"][1][:WIN].any() and not any(ref["member_ok"][k][WIN: 2 * WIN].any() for k in (0, 1, 3))
    _run_and_check(ctx, torch, [c])


@pytest.mark.parametrize("row_offset", [0, 1, 63, 64, 65])
def test_member_bitmaps_at_array_offsets(ctx, torch, row_offset):
    """type ids, offsets and a sparse member's bitmap are read at row_offset + r; a dense member's bitmap at offsets[r]"""
    rng = np.random.default_rng(120 + row_offset)
    cases = [_case(mode, 3, n, rng, row_offset=row_offset, name="offset") for mode in ("sparse", "dense") for n in (65, WIN + 1)]
    for c in cases:
        ref = uc.case_reference(c)
        assert ref["valid"].any() and not ref["valid"].all()
    _run_and_check(ctx, torch, cases)


def test_struct_parent_words_are_anded_in_and_pad_bits_are_ones(ctx, torch):
    rng = np.random.default_rng(130)
    cases = [_case(mode, 2, n, rng, parent=True, name="parent") for mode in ("sparse", "dense") for n in (1, 64, 65, WIN, WIN + 1, 4099)]
    assert any(int(c["parent"][c["nrows"] >> 6]) >> (c["nrows"] & 63) != int(uc.ONES) >> (c["nrows"] & 63) for c in cases if c["nrows"] % 64), \
        "some parent has a zero among its pad bits"
    c = cases[-1]
    own = uc.union_reference(c["mode"], c["ids"], c["offsets"], uc.id_map_of(c["codes"]),
                             [(m["length"], uc.member_ok(m), m["null_type"]) for m in c["members"]])["valid"]
    both = uc.case_reference(c)["valid"]
    assert (own & ~both).any() and both.any()
    _run_and_check(ctx, torch, cases)


def test_null_count_0_ignores_the_bitmap_no_bitmap_is_all_valid_and_a_null_type_member_is_null(ctx, torch):
    rng = np.random.default_rng(140)
    cases = []
    for mode in ("sparse", "dense"):
        cases.append(_case(mode, 3, 4099, rng, null_count=0, name="null_count_0"))
        cases.append(_case(mode, 3, 4099, rng, nulls=False, name="no_bitmap"))
        assert all(uc.case_reference(c)["valid"].all() for c in cases[-2:])
    c = _case("sparse", 3, 4099, rng, name="null_type")
    c["members"][1]["null_type"] = True
    ref = uc.case_reference(c)
    assert not ref["member_ok"][1].any() and ref["member_ok"][2].any()
    cases.append(c)
    _run_and_check(ctx, torch, cases)


def test_without_out_validity_the_preset_words_stay(ctx, torch):
    rng = np.random.default_rng(150)
    cases = [_case(mode, 2, 4099, rng, name="no_out_validity") for mode in ("sparse", "dense")]
    _run_and_check(ctx, torch, cases, out_validity=False)


@pytest.mark.parametrize("where", ["before", "after"])
def test_dense_every_width_shared_and_skipped_rows_and_a_member_of_length_1(ctx, torch, where):
    """Five members of 1, 2, 4, 8 and 16 bytes a value; member 0 has one row, which every row that selects it shares; the
    others are shorter than the union, so rows share child rows, and offsets are even only, so odd child rows are skipped.
    The member arrays are decoded into scratch (preset to POISON) by K_COPY tasks of the same plan that stand before or
    after the union tasks in the task array: the expansion must run behind them either way."""
    rng = np.random.default_rng(160)
    n, codes = 3 * WIN + 7, _codes(5)
    members = [uc.make_member(1 if k == 0 else 50 * k, WIDTHS[k], rng, nulls=k % 2 == 1) for k in range(5)]
    tag = rng.integers(0, 5, n)
    offs = np.array([2 * rng.integers(0, (members[k]["length"] + 1) // 2) for k in tag], np.int32)
    c = uc.make_union_case("dense", codes, members, np.asarray(codes, np.int8)[tag], offs, name="dense_widths_" + where)
    ref = uc.case_reference(c)
    assert all(ok.any() for ok in ref["member_ok"])
    _run_and_check(ctx, torch, [c], dense_member_task=where)


def test_dense_string_t_members_keep_their_heap_pointers(ctx, torch):
    """16-byte rows that are string_t images with a pointer (length > 12): the expansion copies them bit for bit"""
    rng = np.random.default_rng(170)
    n = WIN + 9
    mem = uc.make_member(40, 16, rng)
    rows = mem["values"][:40].view(np.uint32).reshape(40, 4)
    rows[:, 0] = rng.integers(13, 5000, 40)                                 # length > 12: prefix + pointer
    rows[:, 2:] = (0x7F0000000000 + rng.integers(0, 2**30, 40)).astype(np.uint64).view(np.uint32).reshape(40, 2)
    c = uc.make_union_case("dense", [9], [mem], np.full(n, 9, np.int8), rng.integers(0, 40, n).astype(np.int32), name="string_t")
    _run_and_check(ctx, torch, [c])


# ------------------------------------------------------------------------------------------------ damaged inputs
DAMAGE_ROW = WIN + 70          # in the second tile, in its second word
DAMAGED = {
    "type_id_minus_1": ("ids", -1, _ffi.ST_BAD_UNION_TAG),
    "type_id_minus_128": ("ids", -128, _ffi.ST_BAD_UNION_TAG),
    "type_id_not_in_the_map": ("ids", 5, _ffi.ST_BAD_UNION_TAG),
    "type_id_127_absent": ("ids", 127, _ffi.ST_BAD_UNION_TAG),
    "offset_minus_1": ("offsets", -1, _ffi.ST_BAD_UNION_OFFSET),
    "offset_is_the_member_length": ("offsets", None, _ffi.ST_BAD_UNION_OFFSET),
    "offset_2_to_the_31_minus_1": ("offsets", 2**31 - 1, _ffi.ST_BAD_UNION_OFFSET),
}


def _damage_twins(name, mode, rng):
    what, value, status = DAMAGED[name]
    n, codes = 2 * WIN + 11, [126, 0, 64]
    members = [uc.make_member(n if mode == "sparse" else 33 + k, 8, rng) for k in range(3)]       # no bitmaps: every clean row is valid
    ids, offs = uc.random_rows(mode, codes, members, n, rng)
    clean = uc.make_union_case(mode, codes, members, ids, offs, name=name + "/clean")
    ids2, offs2 = ids.copy(), None if offs is None else offs.copy()
    if what == "ids":
        ids2[DAMAGE_ROW] = value
    else:
        k = codes.index(int(ids[DAMAGE_ROW]))
        offs2[DAMAGE_ROW] = members[k]["length"] if value is None else value
    damaged = uc.make_union_case(mode, codes, members, ids2, offs2, name=name + "/damaged")
    assert (ids != ids2).sum() + (0 if offs is None else (offs != offs2).sum()) == 1
    return clean, damaged, status


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_rows_raise_their_flag_become_null_and_are_never_used(ctx, torch, name):
    """126, 0 and 64 are the members here; 127 and 5 are none.  The clean twin gives the reference and status 0; the damaged column (one
    entry differs) gives the reference too -- the damaged row NULL with tag 0 in the union and in every member, every other
    row unchanged, sentinels and guard words intact -- and the status bit."""
    for mode in ("sparse", "dense") if DAMAGED[name][0] == "ids" else ("dense",):
        rng = np.random.default_rng(180)
        clean, damaged, status = _damage_twins(name, mode, rng)
        _run_and_check(ctx, torch, [clean])
        ref_clean, ref = uc.case_reference(clean), uc.case_reference(damaged)
        assert ref_clean["status"] == 0 and ref_clean["valid"].all() and ref["status"] == status
        assert np.array_equal(np.nonzero(~ref["valid"])[0], [DAMAGE_ROW])
        got, st = uc.run_union_plan(ctx, torch, [damaged])
        uc.check_union_case(damaged, got[0], want=ref, damaged_rows=[DAMAGE_ROW])
        assert st == status, (name, mode, st)


def test_hand_built_tasks_are_validated(ctx, torch):
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = dict(buf2=p + 1024, param=2, param2=512, buf2_len=8)
    bad = [dict(ok, param=0), dict(ok, param=33), dict(ok, buf2=0), dict(ok, buf2=p + 1028), dict(ok, param2=0), dict(ok, param2=516),
           dict(ok, param2=8), dict(ok, buf2_len=0), dict(ok, buf2_len=12), dict(ok, ptr_base=p + 2050), dict(ok, parent_div=2, out_aux=p + 3072)]
    da.Plan(ctx, [da.make_task(_ffi.K_UNION, 64, p, p + 2048, **ok)]).close()
    for kw in bad:
        with pytest.raises(_ffi.MiError) as e:
            da.Plan(ctx, [da.make_task(_ffi.K_UNION, 64, p, p + 2048, **kw)])
        assert e.value.code == _ffi.MI_EINVAL and "UNION" in str(e.value), kw
    okd = dict(buf2=p + 1024, buf2_len=4, param=4, out_aux=p + 3072)
    da.Plan(ctx, [da.make_task(_ffi.K_UNION_DENSE, 64, p, p + 2048, **okd)]).close()
    for kw in [dict(okd, param=3), dict(okd, buf2=0), dict(okd, buf2=p + 1032), dict(okd, out_aux=0), dict(okd, buf2_len=-1), dict(okd, parent_div=2)]:
        with pytest.raises(_ffi.MiError) as e:
            da.Plan(ctx, [da.make_task(_ffi.K_UNION_DENSE, 64, p, p + 2048, **kw)])
        assert e.value.code == _ffi.MI_EINVAL and "UNION_DENSE" in str(e.value), kw

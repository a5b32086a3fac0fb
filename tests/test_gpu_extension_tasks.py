"""MI_K_UUID, MI_K_BOOL8 (tile_uuid / tile_bool8 in transcode_misc<2>, and the gather kernel) and MI_K_ENC_UUID_TEXT
(encode_uuid_text) at the task level, against the numpy restatement of extension_cases.py (held to Python's uuid module and
to pyarrow in test_extension_reference_host.py).

Decode, per task (extension_cases.check_decode): every data row equals the restatement, the rows under a NULL included
(they are converted like the others); the sentinel behind the last row is untouched; the validity words equal the
reference with pad bits ones; the guard word is intact.  Encode, per task (encode_tasks.check_plan): offsets, text, bitmap
and NULL count equal the restatement byte for byte and nothing outside the buffers is written.

The shapes follow the loops: tile_bool8 moves four rows per lane and 1024 per pass with a scalar tail, tile_uuid one row
per lane; tiles are 2048 rows; the text encoder works in sub-blocks of 256 rows, ranks rows by the popcount of the tile's
validity words, and takes its first byte from the popcount of the words in front of the tile."""
import numpy as np
import pytest

import duckdb_arrow_amd as da

import encode_tasks as et
import extension_cases as ec

pytestmark = pytest.mark.gpu

KINDS = {"uuid": ec.K_UUID, "bool8": ec.K_BOOL8}
FORMS = ["none", "all_valid", "all_null", "random"]


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _parent_words(rows, rng):
    return rng.integers(0, 256, ((rows + 63) // 64 + 2) * 8, dtype=np.uint8).view(np.uint64)


def flat_columns(kind, rng):
    """every row count at array offset 0 and at 13 (no multiple of 8), every validity form"""
    return [ec.make_column(kind, n, o, form, rng) for n in ec.ROWS for o in (0, 13) for form in FORMS]


@pytest.mark.parametrize("name", list(KINDS))
def test_flat_decode_at_the_loop_seams(ctx, torch, name):
    cols = flat_columns(KINDS[name], np.random.default_rng(100 + KINDS[name]))
    assert len(cols) == 9 * 2 * 4
    got, status = ec.run_decode(ctx, torch, cols)
    assert status == 0
    for col, g in zip(cols, got):
        ec.check_decode(col, g)


@pytest.mark.parametrize("name", list(KINDS))
def test_children_of_structs_and_fixed_size_lists(ctx, torch, name):
    """a struct parent (0 or 1 child rows per parent row: the same word of the parent) and a fixed-size-list parent (3 and 64
    child rows per parent row: the parent's bits are rebuilt), with and without a bitmap of the child's own"""
    rng = np.random.default_rng(200 + KINDS[name])
    cols = []
    for n, o in ((65, 0), (2049, 13), (3 * 2048 + 17, 7)):
        for div in (0, 1):
            for form in ("random", "none"):
                cols.append(ec.make_column(KINDS[name], n, o, form, rng, parent=(_parent_words(n, rng), div)))
    for div in (3, 64):
        for parents in (1, 33, 700):
            for form in ("random", "none"):
                cols.append(ec.make_column(KINDS[name], parents * div, (0, 13)[parents % 2], form, rng, parent=(_parent_words(parents, rng), div)))
    got, status = ec.run_decode(ctx, torch, cols)
    assert status == 0
    for col, g in zip(cols, got):
        ec.check_decode(col, g)


def test_bool8_every_byte_value_under_valid_and_null_rows(ctx, torch):
    rng = np.random.default_rng(8)
    col = ec.make_column(ec.K_BOOL8, 4 * 256 * 6 + 3, 5, "random", rng)
    raw = col["buf1"]
    raw[5: 5 + col["n"]] = np.resize(np.repeat(np.arange(256, dtype=np.uint8), 6), col["n"])       # each value on 6 rows in a row
    col["want"] = ec.bool8(raw[5: 5 + col["n"]])
    for v in ec.BOOL8_BYTES:
        rows = np.nonzero(raw[5: 5 + col["n"]] == v)[0]
        assert col["ok"][rows].any() and (~col["ok"][rows]).any(), v
    (g,), status = ec.run_decode(ctx, torch, [col])
    assert status == 0
    ec.check_decode(col, g)
    assert set(np.unique(g[0][: col["n"]]).tolist()) == {0, 1}


def test_uuid_edges_under_valid_and_null_rows(ctx, torch):
    rng = np.random.default_rng(9)
    n = 2 * len(ec.UUID_EDGES)
    col = ec.make_column(ec.K_UUID, n, 3, "random", rng, edges=False)
    raw = col["buf1"].reshape(-1, 16)
    raw[3: 3 + n] = np.frombuffer(b"".join(ec.UUID_EDGES * 2), np.uint8).reshape(-1, 16)
    bits = np.unpackbits(col["validity"], bitorder="little")
    bits[3: 3 + n] = [1] * len(ec.UUID_EDGES) + [0] * len(ec.UUID_EDGES)
    col["validity"] = np.packbits(bits, bitorder="little")
    col["ok"] = bits[3: 3 + n].astype(bool)
    col["want"] = ec.uuid_from_arrow(raw[3: 3 + n]).reshape(-1)
    (g,), status = ec.run_decode(ctx, torch, [col])
    assert status == 0
    ec.check_decode(col, g)
    image = ec.hugeint_of(g[0][: n * 16])
    assert image[0] == -(1 << 127) and image[1] == (1 << 127) - 1 and image[2] == -1 and image[3] == 0


@pytest.mark.parametrize("name", list(KINDS))
def test_gather_equals_the_flat_result(ctx, torch, name):
    """the same columns through a selection vector: full windows, empty windows, single rows, the first and the last row"""
    from decode_tasks import make_sel
    rng = np.random.default_rng(300 + KINDS[name])
    cols, sels = [], []
    for n, o in ((1, 0), (65, 13), (2048, 0), (2049, 13), (3 * 2048 + 17, 5)):
        for form in ("none", "random", "all_null"):
            for counts in ([None], [0, 1, 700], [1, 2047, 2]):
                cols.append(ec.make_column(KINDS[name], n, o, form, rng))
                sels.append(make_sel(n, counts, rng))
    flat, status = ec.run_decode(ctx, torch, cols)
    assert status == 0
    got, status = ec.run_decode(ctx, torch, cols, sels)
    assert status == 0
    for col, g, f, sel in zip(cols, got, flat, sels):
        ec.check_decode(col, f)
        ec.check_decode(col, g, sel)
        rows = np.concatenate([k * ec.WIN + s for k, s in enumerate(sel)] + [np.zeros(0, np.int64)]).astype(np.int64)
        w = col["width"]
        assert np.array_equal(g[0][: len(rows) * w].reshape(-1, w), f[0][: col["n"] * w].reshape(-1, w)[rows])


# ------------------------------------------------------------------------------------------------ UUID -> text
def _ok(form, n, rng):
    if form == "none":
        return None
    ok = np.ones(n, bool)
    if form == "random":
        ok = rng.random(n) < 0.75
    elif form == "all_null":
        ok[:] = False
    elif form == "null_run_over_the_seam":
        ok[max(0, min(n, 2048) - 100): 2048 + 100] = False
    elif form == "first_null_after_two_tiles":       # every word in front of the third tile is all ones: the popcount base
        ok[2 * 2048 + 5:] = rng.random(max(0, n - 2 * 2048 - 5)) < 0.5
        if n > 2 * 2048 + 5:
            ok[2 * 2048 + 5] = False
    else:
        assert form == "all_valid"
    return ok


TEXT_FORMS = ["none", "all_valid", "random", "all_null", "null_run_over_the_seam", "first_null_after_two_tiles"]


@pytest.mark.parametrize("large", [False, True], ids=["int32", "int64"])
def test_uuid_text_encoder(ctx, torch, large):
    rng = np.random.default_rng(400 + large)
    cols, refs = [], []
    for n in ec.ROWS:
        for k, form in enumerate(TEXT_FORMS):
            col, ref = ec.text_column(n, _ok(form, n, rng), rng, "%s/n%d/%s" % (form, n, "i64" if large else "i32"), large=large, vpos=(0, 1, 3, 5)[k % 4])
            cols.append(col)
            refs.append(ref)
    got, where, runs = et.run_plan(ctx, torch, cols, refs, launches=2)
    assert et.check_plan(cols, refs, got, where, runs) == 0
    # pyarrow reads the buffers of the largest random column as the strings Python's uuid module prints
    import pyarrow as pa
    import uuid
    col, ref, at = next((c, r, a) for c, r, a in zip(cols, refs, where) if c["name"].startswith("random/n%d" % ec.ROWS[-1]))
    bufs = [pa.py_buffer(got[at[k][0]: at[k][0] + at[k][1]].tobytes()) for k in ("bitmap", "data", "aux")]
    arr = pa.Array.from_buffers(pa.large_string() if large else pa.string(), col["n"], bufs)
    arr.validate(full=True)
    assert arr.to_pylist() == [str(uuid.UUID(bytes=r.tobytes())) if v else None for r, v in zip(col["arrow"], col["ok"])]


def test_uuid_text_beside_the_other_encode_kinds(ctx, torch):
    """one plan with fixed-width, string and UUID text tasks: each kernel takes its own tiles and counts its own NULLs"""
    rng = np.random.default_rng(77)
    base_cols, base_refs = et.case_columns("fixed_kinds")
    cols, refs = list(base_cols), list(base_refs)
    for n, form in ((2049, "random"), (65, "none"), (3 * 2048 + 17, "first_null_after_two_tiles")):
        col, ref = ec.text_column(n, _ok(form, n, rng), rng, "mixed/%s/n%d" % (form, n))
        cols.insert(len(cols) // 2, col)
        refs.insert(len(refs) // 2, ref)
    got, where, runs = et.run_plan(ctx, torch, cols, refs)
    et.check_plan(cols, refs, got, where, runs)

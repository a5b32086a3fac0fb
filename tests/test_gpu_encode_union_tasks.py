"""MI_K_ENC_UNION (encode_union, kernels_encode_union.hip) and MI_K_ENC_INTERVAL (enc_tile_interval in encode_fixed) task by
task through the plan entry, against the numpy restatement of union_encode_cases.py (held to pyarrow in
test_union_encode_reference_host.py), bit for bit.

Per union: the int8 type ids, every member's effective mask (pad bits ones), and the buffers and NULL count of every member's
ordinary encode task run under its mask equal the restatement; the bytes around every buffer and between the masks are
untouched; the union's own NULL counter stays 0.  The member tasks stand IN FRONT of their union's task in the plan: that the
union pass runs first is the plan's business.

The shapes follow the kernel: a row per lane, 64 rows per ballot, 256 rows per step, 2048 per tile, one LDS mask row per
member (1, 2 and 32 members)."""
import numpy as np
import pytest

import duckdb_arrow_amd as da

import encode_tasks as et
import union_encode_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("case", ["rows", "shapes"])
def test_union_pass_and_members_under_their_masks(ctx, torch, case):
    unions, urefs = uc.case_items(case)
    result = uc.run_plan(ctx, torch, unions, urefs, launches=2)
    assert uc.check_plan(unions, urefs, (), (), result) == 0


def test_a_bad_tag_raises_the_status_bit_and_leaves_the_clean_twin_alone(ctx, torch):
    unions, urefs = uc.case_items("bad_tags")
    assert [u["name"] for u in unions[:2]] == ["bad_tag/clean", "bad_tag/damaged"] and urefs[0]["status"] == 0 and urefs[1]["status"] == uc.ST_BAD_UNION_TAG
    result = uc.run_plan(ctx, torch, unions, urefs)
    assert uc.check_plan(unions, urefs, (), (), result) == uc.ST_BAD_UNION_TAG
    # without the damaged one the status is clean (a tag >= m under a NULL row is not looked at)
    rest = [0, 2]
    result = uc.run_plan(ctx, torch, [unions[i] for i in rest], [urefs[i] for i in rest])
    assert uc.check_plan([unions[i] for i in rest], [urefs[i] for i in rest], (), (), result) == 0
    with pytest.raises(da.MiError, match="Arrow union tag out of range"):
        da._ffi.check(da._ffi.lib().mi_status_to_error(uc.ST_BAD_UNION_TAG))


def test_interval_rows(ctx, torch):
    cols, refs = uc.interval_columns()
    got, where, runs = et.run_plan(ctx, torch, cols, refs, launches=2)
    assert et.check_plan(cols, refs, got, where, runs) == 0


def test_beside_the_other_encode_kinds_in_one_plan(ctx, torch):
    """unions, intervals, fixed-width, string and list tasks in one plan: every kernel takes its own tiles and counts its own NULLs"""
    unions, urefs = uc.case_items("shapes")
    icols, irefs = uc.interval_columns()
    fcols, frefs = et.case_columns("fixed_kinds")
    scols, srefs = et.case_columns("tiny")
    cols = list(fcols[::7]) + list(icols[::5]) + list(scols[::3])
    refs = list(frefs[::7]) + list(irefs[::5]) + list(srefs[::3])
    result = uc.run_plan(ctx, torch, unions[::2], urefs[::2], cols, refs)
    assert uc.check_plan(unions[::2], urefs[::2], cols, refs, result) == 0


def test_plans_refuse_malformed_union_tasks(ctx, torch):
    d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()

    def union(**kw):
        args = dict(validity=0, buf2=p + 4096, buf2_len=64, out_aux=p + 8192, param=2)
        args.update(kw)
        return da.make_task(uc.K_ENC_UNION, 100, p, p + 1024, **args)

    da.Plan(ctx, [union()]).close()
    for kw, text in ((dict(param=0), "number of members"), (dict(param=33), "number of members"), (dict(buf2=0), "validity addresses"),
                     (dict(out_aux=0), "masks"), (dict(out_aux=p + 8196), "masks"), (dict(buf2_len=8), "distance between masks"),
                     (dict(buf2_len=60), "distance between masks"), (dict(ptr_base=p + 4), "parent words misaligned")):
        with pytest.raises(da.MiError, match=text):
            da.Plan(ctx, [union(**kw)])
    with pytest.raises(da.MiError, match="unknown kind 40"):
        da.Plan(ctx, [da.make_task(40, 100, p, p + 1024, out_validity=p + 2048)])
    with pytest.raises(da.MiError, match="16-byte aligned"):
        da.Plan(ctx, [da.make_task(uc.K_ENC_INTERVAL, 100, p + 8, p + 4096, out_validity=p + 2048, param=16)])

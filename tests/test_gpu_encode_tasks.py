"""The encode kernels (kernels_encode.hip: encode_fixed, encode_string_1p, encode_string_slow) at the task level against
encode_tasks.encode_reference, a numpy restatement of ArrowAppender that test_encode_reference_host.py checks without a
GPU on the same columns.

Per task (encode_tasks.check_task): every output buffer -- bitmap, offsets / data, string data -- lies in one arena
pre-filled with 0xEE and equals the reference byte for byte, offsets[0] == 0 included; every byte between the buffers is
still 0xEE; a task of 0 rows has written nothing.  Per plan (check_plan): the NULL counts are the reference's in the
caller's task order, the status is the OR of the tasks' (MI_ST_OFFSET_OVERFLOW exactly where int32 offsets pass INT32_MAX).

What the cases aim at is in the docstrings of their builders (encode_tasks.CASES), printed with a failing case."""
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import encode_tasks as et

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return da.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_constants_are_the_library_s():
    assert (et.K_ENC_COPY, et.K_ENC_DEC128, et.K_ENC_BOOL, et.K_ENC_STR32, et.K_ENC_VALIDITY, et.K_ENC_LIST32, et.ST_OFFSET_OVERFLOW) == \
        (_ffi.K_ENC_COPY, _ffi.K_ENC_DEC128, _ffi.K_ENC_BOOL, _ffi.K_ENC_STR32, _ffi.K_ENC_VALIDITY, _ffi.K_ENC_LIST32, _ffi.ST_OFFSET_OVERFLOW)


@pytest.mark.parametrize("case", list(et.CASES))
def test_every_task_of_the_plan_equals_the_reference(ctx, torch, case):
    cols, refs = et.case_columns(case)
    print(et.CASES[case].__doc__)
    got, where, runs = et.run_plan(ctx, torch, cols, refs)
    assert et.check_plan(cols, refs, got, where, runs) == et.EXPECTED_STATUS.get(case, 0)


@pytest.mark.parametrize("case", ["lookback_many_columns", "fixed_kinds"])
def test_null_counts_are_reset_by_reading_them(ctx, torch, case):
    """The same plan launched twice, the counts read after each launch: both readings are the reference's (a counter that
    survived the first reading would show twice its value), and so are the bytes after the second launch."""
    cols, refs = et.case_columns(case)
    assert sum(ref["nulls"] for ref in refs) > 0
    got, where, runs = et.run_plan(ctx, torch, cols, refs, launches=2)
    assert len(runs) == 2 and runs[0] == runs[1]
    et.check_plan(cols, refs, got, where, runs)


def test_the_2p32_plus_5_list_is_not_taken_for_5(ctx, torch):
    """The last offset of the LargeList column whose fourth list has 2**32 + 5 entries, read back as a number: a kernel that
    summed the low dwords of the lengths would end 2**32 short of the reference."""
    cols, refs = et.case_columns("list_of_2p32_plus_5_int64")
    got, where, _ = et.run_plan(ctx, torch, cols, refs)
    pos, size, _ = where[0]["data"]
    assert int(got[pos: pos + size].view("<i8")[-1]) == cols[0]["ends"][-1] >= 2**32 + 5

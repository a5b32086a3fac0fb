"""encode_string_view (kernels_encode_view.hip, MI_K_ENC_STRVIEW) at the task level against encode_view_tasks.view_reference, a
numpy restatement of DuckDB's string-view appender that test_encode_view_reference_host.py checks with pyarrow on the same
columns.  The plans run through encode_tasks.run_plan: every output buffer -- bitmap, views, data buffer -- lies in one arena
pre-filled with 0xEE with guards in front of and behind it and equals the reference byte for byte, every other byte is still
0xEE, and the NULL counts and the status are the reference's (encode_tasks.check_plan).

What the cases aim at is in the docstrings of their builders (encode_view_tasks.CASES), printed with a failing case; each
builder asserts its own precondition.  MI_ST_OFFSET_OVERFLOW takes 2 GiB of output to reach on the device and is not run
here: the host layout refuses such a record batch before anything is launched (tests/sanitize/writer_view_plan_check.cpp)."""
import numpy as np
import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

import encode_tasks as et
import encode_view_tasks as vt

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
    assert vt.K_ENC_STRVIEW == _ffi.K_ENC_STRVIEW == 38


@pytest.mark.parametrize("case", list(vt.CASES))
def test_every_task_of_the_plan_equals_the_reference(ctx, torch, case):
    cols, refs = vt.case_columns(case)
    print(vt.CASES[case].__doc__)
    assert any(c["kind"] == vt.K_ENC_STRVIEW and c["n"] > 0 for c in cols)
    got, where, runs = et.run_plan(ctx, torch, cols, refs)
    assert et.check_plan(cols, refs, got, where, runs) == 0


def test_a_column_without_long_strings_has_an_empty_data_buffer(ctx, torch):
    """Inline rows only, three tiles: every tile publishes a sum of 0 and leaves; the data buffer is there and 0 bytes long, and
    not one byte behind its position is written."""
    rng = np.random.default_rng(11)
    n = 2 * et.TILE + 77
    cols = [vt.view_column(rng.integers(0, 13, n), rng.random(n) < 0.8, rng, "view/inline_only", vpos=5)]
    refs = [vt.reference(c) for c in cols]
    assert len(refs[0]["aux"]) == 0 and len(cols[0]["long_rows"]) == 0
    got, where, runs = et.run_plan(ctx, torch, cols, refs)
    et.check_plan(cols, refs, got, where, runs)


@pytest.mark.parametrize("case", ["lookback_many_columns"])
def test_null_counts_are_reset_by_reading_them(ctx, torch, case):
    """The same plan launched twice, the counts read after each launch: both readings are the reference's, and so are the bytes
    after the second launch (the look-back words are zeroed by every launch)."""
    cols, refs = vt.case_columns(case)
    assert sum(ref["nulls"] for ref in refs) > 0
    got, where, runs = et.run_plan(ctx, torch, cols, refs, launches=2)
    assert len(runs) == 2 and runs[0] == runs[1]
    et.check_plan(cols, refs, got, where, runs)

"""Handles that depend on a Context must go before it.  An HbmStream holds its Context, so plain reference counting frees
them in that order -- as long as the HbmStream is not part of a reference cycle: the cycle collector finalises a group of
objects in any order, and the library would close a stream whose context is already destroyed."""
import gc
import weakref

import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import hbm


class _Owner:
    n_tasks = 3


def test_plan_view_does_not_keep_its_owner_alive():
    gc.disable()
    try:
        owner = _Owner()
        owner.plan = hbm._PlanView(owner)
        assert owner.plan.n_tasks == 3
        gone = weakref.ref(owner)
        del owner
        assert gone() is None, "the owner is freed by its reference count, without the cycle collector"
    finally:
        gc.enable()


@pytest.mark.gpu
def test_hbm_stream_is_freed_by_its_reference_count_before_its_context():
    buf, _ = da.synth_lineitem_stream(scale_factor=0.001, seed=3, rows_per_batch=2000)
    gc.disable()
    try:
        ctx = da.Context(0)
        hs = hbm.HbmStream(ctx, buf)
        assert hs.plan.n_tasks == hs.n_tasks > 0
        gone, ctx_gone = weakref.ref(hs), weakref.ref(ctx)
        del ctx
        assert ctx_gone() is not None, "the stream keeps its context"
        del hs
        assert gone() is None and ctx_gone() is None
    finally:
        gc.enable()

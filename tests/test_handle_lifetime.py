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


class _CountingLib:
    """stands in for the library: records the order in which handles are destroyed"""

    def __init__(self):
        self.calls = []

    def mi_ctx_destroy(self, h):
        self.calls.append("ctx")

    def mi_scan_close(self, h):
        self.calls.append("scan")


@pytest.mark.parametrize("context_first", [True, False])
def test_a_relation_finalised_after_its_context_still_finds_it_alive(monkeypatch, context_first):
    """the cycle collector may finalise a context before a relation that is still open on it (both hang on the frame a
    traceback keeps): the scan is closed first all the same, and the context is destroyed exactly once"""
    import ctypes as C
    lib = _CountingLib()
    monkeypatch.setattr(da._ffi, "lib", lambda: lib)
    ctx = da.Context.__new__(da.Context)
    ctx._h, ctx._users, ctx._orphaned = C.c_void_p(1), 0, False
    con = da.Connection.__new__(da.Connection)
    con.ctx = ctx
    rel = da.Relation.__new__(da.Relation)
    rel._conn, rel._h, rel._keep, rel._contexts = con, C.c_void_p(2), None, [ctx]
    ctx._retain()
    for finalise in ((ctx.__del__, rel.__del__) if context_first else (rel.__del__, ctx.__del__)):
        finalise()
    assert lib.calls == ["scan", "ctx"]
    rel.close(), ctx.close()
    assert lib.calls == ["scan", "ctx"]

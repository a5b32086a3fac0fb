"""The reference of the string-view encode tests (encode_view_tasks.view_reference), checked without a GPU on the very columns
test_gpu_encode_view_tasks.py runs.  pyarrow is the independent reader: pa.Array.from_buffers(pa.string_view(), n, [bitmap,
views, data]) must pass validate(full=True) -- which refuses non-zero inline padding, a prefix that differs from the data, a
range outside the data buffer and a buffer index other than 0 -- and give back the builder's values.  Full validation accepts
anything under a NULL row, so the zero row is asserted here; so is the data buffer: exactly the long strings of the valid rows,
joined in row order."""
import numpy as np
import pyarrow as pa
import pytest

import encode_tasks as et
from encode_view_tasks import CASES, INLINE, K_ENC_STRVIEW, case_columns, view_column, view_reference


@pytest.mark.parametrize("case", list(CASES))
def test_view_reference_equals_pyarrow_and_the_builder(case):
    cols, refs = case_columns(case)
    seen = 0
    for col, ref in zip(cols, refs):
        if col["kind"] != K_ENC_STRVIEW:
            continue
        seen += 1
        n = col["n"]
        assert ref["status"] == 0 and ref["loose"] == 0
        if n == 0:
            assert len(ref["bitmap"]) == len(ref["data"]) == len(ref["aux"]) == 0 and ref["nulls"] == 0
            continue
        ok = np.ones(n, bool) if col["ok"] is None else col["ok"]
        values = col["values"]()
        assert len(ref["data"]) == 16 * n and ref["nulls"] == n - int(ok.sum())
        arr = pa.Array.from_buffers(pa.string_view(), n, [pa.py_buffer(ref["bitmap"].tobytes()), pa.py_buffer(ref["data"].tobytes()), pa.py_buffer(ref["aux"].tobytes())])
        arr.validate(full=True)
        assert arr.null_count == ref["nulls"], col["name"]
        assert arr.to_pylist() == [None if v is None else v.decode() for v in values], col["name"]
        views = ref["data"].reshape(n, 16)
        assert not views[~ok].any(), col["name"]                                            # NULL: 16 zero bytes
        long_ = [v for v in values if v is not None and len(v) > INLINE]
        assert ref["aux"].tobytes() == b"".join(long_), col["name"]
        assert len(ref["aux"]) == col["long_bytes"] and len(long_) == len(col["long_rows"])
        if col["text"] is not None:      # ... which is the builder's text without the inline rows
            assert sum(len(v) for v in values if v is not None) == len(col["text"])
    assert seen > 0


def test_pyarrow_refuses_what_the_reference_must_not_produce():
    """the four defects full validation is relied on for, each planted in a good reference"""
    rng = np.random.default_rng(5)
    col = view_column([3, 20, 12, 30, 0], None, rng, "view/defects")
    ref = view_reference(col)

    def check(views, data):
        pa.Array.from_buffers(pa.string_view(), 5, [pa.py_buffer(ref["bitmap"].tobytes()), pa.py_buffer(views.tobytes()), pa.py_buffer(data.tobytes())]).validate(full=True)

    check(ref["data"], ref["aux"])
    for row, byte, what in ((0, 4 + 3, "padding"), (1, 4, "prefix"), (3, 8, "buffer index"), (3, 12 + 1, "range")):
        bad = ref["data"].copy()
        bad[16 * row + byte] ^= 0x40
        with pytest.raises((pa.ArrowInvalid, pa.ArrowIndexError)):
            check(bad, ref["aux"])


def test_the_int32_limit_raises_the_overflow_bit():
    """two long rows whose lengths add up to INT32_MAX + 1: the reference materialises nothing and raises the bit.  (A total of
    exactly INT32_MAX fits; that side is the stand-alone layout check's, which needs no 2 GiB.)"""
    src = np.zeros((2, 16), np.uint8)
    src.view("<u4")[:, 0] = [2**30, et.INT32_MAX - 2**30 + 1]
    col = dict(kind=K_ENC_STRVIEW, n=2, words=None, src=src.reshape(-1), heap=np.zeros(0, np.uint8), ptr_base=0, bitmap=True, vpos=0)
    assert view_reference(col)["status"] == et.ST_OFFSET_OVERFLOW

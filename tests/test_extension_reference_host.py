"""The numpy restatement of the extension-type rules (extension_cases.py) against what does not come from this project:
Python's uuid module, pyarrow's own buffers, and the plain definition of bool8.  No GPU, no library call: the GPU suites
compare the kernels with this restatement, so it is checked on its own first."""
import uuid

import numpy as np
import pyarrow as pa
import pytest

import extension_cases as ec


def _uuids(n=3000, seed=7):
    rng = np.random.default_rng(seed)
    us = ec.random_uuids(n, rng)
    return us, np.frombuffer(b"".join(u.bytes for u in us), np.uint8).reshape(-1, 16)


def test_uuid_image_is_the_uuid_integer_with_the_top_bit_flipped():
    us, raw = _uuids()
    got = ec.hugeint_of(ec.uuid_from_arrow(raw))
    for u, g in zip(us, got):
        assert uuid.UUID(bytes=u.bytes) == u
        want = u.int ^ (1 << 127)
        assert g == (want - (1 << 128) if want >= (1 << 127) else want)


def test_signed_order_of_the_image_is_the_order_of_the_text():
    us, raw = _uuids()
    image = ec.hugeint_of(ec.uuid_from_arrow(raw))
    by_image = sorted(range(len(us)), key=lambda i: image[i])
    by_text = sorted(range(len(us)), key=lambda i: str(us[i]))
    assert [us[i] for i in by_image] == [us[i] for i in by_text]
    assert image[0] == -(1 << 127) and image[1] == (1 << 127) - 1      # all zero is the least, all ones the greatest


def test_text_of_the_image_is_str_of_the_uuid():
    us, raw = _uuids()
    text = ec.uuid_text(ec.uuid_from_arrow(raw))
    assert [t.tobytes().decode() for t in text] == [str(u) for u in us]


def test_package_helpers_agree_with_the_restatement():
    import duckdb_arrow_amd as da
    us, raw = _uuids(200)
    image = ec.hugeint_of(ec.uuid_from_arrow(raw))
    assert [da.uuid_to_hugeint(u) for u in us] == image
    assert [da.uuid_to_hugeint(str(u)) for u in us] == image
    assert [da.uuid_from_hugeint(v) for v in image] == us


def test_bool8_over_all_256_byte_values():
    raw = np.arange(256, dtype=np.uint8)
    want = pa.ExtensionArray.from_storage(pa.bool8(), pa.array(raw.view(np.int8), pa.int8())).to_pylist()
    assert ec.bool8(raw).astype(bool).tolist() == want
    assert ec.bool8(raw.view(np.int8)).tolist() == [0] + [1] * 255


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("form", ["none", "random", "all_null", "null_run"])
def test_text_encoder_against_pyarrow_string_buffers(form, large):
    n = 2 * 2048 + 300
    us, raw = _uuids(n, seed=11)
    rng = np.random.default_rng(5)
    ok = {"none": None, "random": rng.random(n) < 0.7, "all_null": np.zeros(n, bool), "null_run": np.ones(n, bool)}[form]
    if form == "null_run":
        ok[2000:2100] = False      # crosses the first tile seam
    off, text, bitmap, nulls = ec.uuid_text_reference(ec.uuid_from_arrow(raw), ok, large)
    valid = np.ones(n, bool) if ok is None else ok
    arr = pa.array([str(u) if v else None for u, v in zip(us, valid)], pa.large_string() if large else pa.string())
    bufs = arr.buffers()
    w = 8 if large else 4
    assert off.tobytes() == bufs[1].to_pybytes()[: (n + 1) * w]
    assert text.tobytes() == (bufs[2].to_pybytes() if bufs[2] is not None else b"")[: len(text)]
    assert len(text) == 36 * int(valid.sum()) and nulls == arr.null_count
    if bufs[0] is not None:
        want = np.frombuffer(bufs[0].to_pybytes(), np.uint8)[: (n + 7) // 8].copy()
        if n % 8:
            want[-1] |= (0xFF << (n % 8)) & 0xFF
        assert np.array_equal(bitmap, want)
    else:
        assert (bitmap == 0xFF).all()
    assert pa.Array.from_buffers(arr.type, n, [pa.py_buffer(bitmap.tobytes()), pa.py_buffer(off.tobytes()), pa.py_buffer(text.tobytes())]).to_pylist() == arr.to_pylist()


def test_text_column_reference_has_the_encode_suite_shape():
    rng = np.random.default_rng(3)
    col, ref = ec.text_column(65, rng.random(65) < 0.5, rng, "c")
    assert col["kind"] == ec.K_ENC_UUID_TEXT and len(col["src"]) == 65 * 16 and len(ref["data"]) == 66 * 4
    assert len(ref["aux"]) == 36 * int(col["ok"].sum()) and ref["nulls"] == 65 - int(col["ok"].sum())
    col, ref = ec.text_column(0, None, rng, "empty")
    assert len(ref["data"]) == 0 and len(ref["aux"]) == 0 and len(ref["bitmap"]) == 0

"""The order the pushed-down filter (K6) gives FLOAT / DOUBLE values, without a GPU: mi_filter_float_key exports the key
function the kernel compiles (duckdb-arrow_amd/csrc/filter_key.hpp).  Keys compare as signed integers the way DuckDB orders
the values -- every NaN equals every other NaN and is greater than everything else, -0.0 = +0.0 -- which is also the order
of np.sort (NaN last).  tests/sanitize/filter_key_check.cpp builds the same header with g++ under ASan + UBSan, walks the
same corpus against a naive comparison (and the 128-bit comparison against __int128) and hands its keys back."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import duckdb_arrow_amd as da

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _specials(width):
    """bit patterns: +-0.0, +-denormal min, +-FLT/DBL_MIN, +-max, +-inf, NaNs of both signs and three payloads"""
    f, u = (np.float32, np.uint32) if width == 4 else (np.float64, np.uint64)
    fi = np.finfo(f)
    vals = np.array([0.0, fi.smallest_subnormal, fi.tiny, fi.max, np.inf], f)
    bits = list(vals.view(u)) + list((-vals).view(u))
    exp_all_ones = vals[-1:].view(u)[0]
    sign = u(1) << u(8 * width - 1)
    quiet = u(1) << u(22 if width == 4 else 51)
    for payload in (quiet, u(1), quiet | u(0x1234)):
        bits += [exp_all_ones | payload, exp_all_ones | payload | sign]
    return np.array(bits, u)


def _corpus(width):
    u = np.uint32 if width == 4 else np.uint64
    rng = np.random.default_rng(width)
    return np.concatenate([_specials(width), rng.integers(0, 1 << (8 * width), 10000, dtype=u, endpoint=False)])


def _keys(bits, width):
    vals = bits.view(np.float32 if width == 4 else np.float64)
    return np.array([da.filter_float_key(float(v), width) for v in vals], np.int64)


@pytest.mark.parametrize("width", [4, 8])
def test_key_order_is_the_order_of_the_values(width):
    bits = _corpus(width)
    vals = bits.view(np.float32 if width == 4 else np.float64)
    keys = _keys(bits, width)
    nan = np.isnan(vals)
    assert nan.sum() >= 6 and (~nan).sum() > 9000
    # all NaN keys are equal, and the greatest key of the width
    assert set(keys[nan].tolist()) == {(1 << (8 * width - 1)) - 1}
    assert keys[~nan].max() < keys[nan][0]
    # -0.0 and +0.0 share a key
    zeros = vals == 0
    assert zeros.sum() >= 2 and np.signbit(vals[zeros]).any() and not np.signbit(vals[zeros]).all()
    assert set(keys[zeros].tolist()) == {0}
    # sorting by key is np.sort (which puts NaN last): the sorted values agree wherever neither is NaN, NaNs sit at the same places
    by_key = vals[np.argsort(keys, kind="stable")]
    by_value = np.sort(vals)
    assert np.array_equal(np.isnan(by_key), np.isnan(by_value))
    assert np.array_equal(by_key[~np.isnan(by_key)], by_value[~np.isnan(by_value)])
    # strictly monotone elsewhere: distinct non-NaN values have distinct keys in the order of the values, equal ones equal keys
    v, k = vals[~nan].astype(np.float64), keys[~nan]
    order = np.argsort(v, kind="stable")
    v, k = v[order], k[order]
    assert np.array_equal(np.diff(v) > 0, np.diff(k) > 0) and np.array_equal(np.diff(v) == 0, np.diff(k) == 0)


def test_a_float_constant_is_rounded_to_float32_first():
    """DuckDB casts the constant to the column's type: on a FLOAT column 10.50000001 is 10.5."""
    assert da.filter_float_key(10.50000001, 4) == da.filter_float_key(10.5, 4)
    assert da.filter_float_key(10.50000001, 8) > da.filter_float_key(10.5, 8)
    assert da.filter_float_key(1e-60, 4) == 0 == da.filter_float_key(-1e-60, 4)    # rounds to +-0.0
    with pytest.raises(da.MiError):
        da.filter_float_key(1.0, 2)


def test_key_header_under_asan_and_ubsan_agrees_with_the_library(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filter_key_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(ROOT, "tests", "sanitize", "filter_key_check.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    c32, c64 = _corpus(4), _corpus(8)
    p32, p64, out = str(tmp_path / "c32.bin"), str(tmp_path / "c64.bin"), str(tmp_path / "keys.bin")
    c32.tofile(p32)
    c64.tofile(p64)
    run = subprocess.run([exe, p32, p64, out], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "%d + %d patterns" % (len(c32), len(c64)) in run.stdout and " 0 failed" in run.stdout, run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    # the keys g++ computed from the header are the keys of the library (the same header through hipcc)
    keys = np.fromfile(out, np.int64)
    assert np.array_equal(keys[: len(c32)], _keys(c32, 4)) and np.array_equal(keys[len(c32):], _keys(c64, 8))

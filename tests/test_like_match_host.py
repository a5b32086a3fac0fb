"""contains / ends_with / %-pattern LIKE as the pushed-down filter (K6) evaluates them, without a GPU: mi_filter_like_match
exports the matcher the kernel compiles (duckdb-arrow_amd/csrc/like_match.hpp) for one row.  Every answer is compared with
Python's own: `needle in row`, `row.endswith(suffix)`, re.fullmatch of the pattern with each `%` -> `.*` under re.DOTALL.
tests/sanitize/like_match_check.cpp builds the same header alone with g++ under ASan + UBSan and matches a fixed list of
patterns against rows that each sit in a heap allocation of exactly their length."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"contains": _ffi.F_CONTAINS, "ends_with": _ffi.F_ENDS_WITH, "like": _ffi.F_LIKE, "not like": _ffi.F_NOT_LIKE}


def like_regex(pattern):
    return re.compile(b"".join(b".*" if c == 0x25 else re.escape(bytes([c])) for c in pattern), re.DOTALL)


def python_says(op, pattern, row):
    """the reference: Python's own evaluation (`op` a number of enum mi_filter_op)"""
    if op == _ffi.F_CONTAINS:
        return pattern in row
    if op == _ffi.F_ENDS_WITH:
        return row.endswith(pattern)
    hit = like_regex(pattern).fullmatch(row) is not None
    return hit if op == _ffi.F_LIKE else not hit


def library_says(op, pattern, row):
    result = C.c_int32(-1)
    rc = _ffi.lib().mi_filter_like_match(op, pattern, len(pattern), row, len(row), C.byref(result))
    assert rc == _ffi.MI_OK and result.value in (0, 1), (op, pattern, row, rc)
    return bool(result.value)


def words(alphabet, up_to):
    return [bytes(w) for n in range(up_to + 1) for w in itertools.product(alphabet, repeat=n)]


ROWS = words(b"ab", 8)


def test_the_symbols_exist():
    assert da.filter_pattern_launches() >= 0
    assert da.filter_like_match("like", "%b%", "abc") and not da.filter_like_match("not like", "%b%", "abc")


@pytest.mark.parametrize("op", ["like", "not like"])
def test_every_small_pattern_on_every_small_row_equals_re_fullmatch(op):
    patterns = words(b"ab%", 6)
    assert len(patterns) == sum(3 ** n for n in range(7)) and len(ROWS) == 2 ** 9 - 1
    fn, code, result = _ffi.lib().mi_filter_like_match, OPS[op], C.c_int32()
    for pattern in patterns:
        rx = like_regex(pattern)
        for row in ROWS:
            assert fn(code, pattern, len(pattern), row, len(row), C.byref(result)) == 0
            want = rx.fullmatch(row) is not None
            assert bool(result.value) == (want if op == "like" else not want), (op, pattern, row)


@pytest.mark.parametrize("op", ["contains", "ends_with"])
def test_every_small_needle_on_every_small_row(op):
    for needle in words(b"ab", 4):
        for row in ROWS:
            assert library_says(OPS[op], needle, row) == python_says(OPS[op], needle, row), (op, needle, row)


@pytest.mark.parametrize("op", ["contains", "ends_with"])
def test_needles_are_literal_bytes(op):
    """0x00, 0xFF, % and _ are bytes like any other in a needle and in a row"""
    pieces = [b"\x00", b"\xff", b"%", b"_", b"a"]
    strings = [b"".join(w) for n in range(4) for w in itertools.product(pieces, repeat=n)]
    hits = 0
    for needle in strings:
        for row in strings:
            got = library_says(OPS[op], needle, row)
            assert got == python_says(OPS[op], needle, row), (op, needle, row)
            hits += got
    assert 0 < hits < len(strings) ** 2


@pytest.mark.parametrize("n", [1, 3, 4, 5, 12, 13, 16, 17, 300])
@pytest.mark.parametrize("op", ["contains", "ends_with", "like"])
def test_needle_lengths(op, n):
    needle = bytes((7 * i + 3) % 251 % 26 + 0x61 for i in range(n))    # no % and no _ in it
    other = needle[:-1] + bytes([needle[-1] ^ 1])
    rows = [needle, other, needle[:-1], needle[1:], b"x" + needle, needle + b"x", b"xy" + needle + b"z", needle + needle,
            needle[:-1] + needle, b"q" * 40 + needle[: n // 2] + needle + b"q" * 3, b"q" * 40 + other + needle, b""]
    pattern = b"%" + needle + b"%x" if op == "like" else needle
    answers = []
    for row in rows:
        got = library_says(OPS[op], pattern, row)
        assert got == python_says(OPS[op], pattern, row), (op, n, row)
        answers.append(got)
    assert True in answers and False in answers


def test_refusals():
    result = C.c_int32(7)
    fn = _ffi.lib().mi_filter_like_match
    for op in (_ffi.F_LIKE, _ffi.F_NOT_LIKE):
        assert fn(op, b"a_c", 3, b"abc", 3, C.byref(result)) == _ffi.MI_ENOTSUP      # `_` steps over characters, these are bytes
        message = _ffi.lib().mi_last_error().decode()
        assert "_" in message and "UTF-8" in message and "above the scan" in message
        eight, nine = b"%".join([b"s"] * 8), b"%".join([b"s"] * 9)
        assert fn(op, eight, len(eight), b"s", 1, C.byref(result)) == _ffi.MI_OK
        assert fn(op, nine, len(nine), b"s", 1, C.byref(result)) == _ffi.MI_ENOTSUP  # a ninth segment
        nine = b"%%s%%" * 9
        assert fn(op, nine, len(nine), b"s", 1, C.byref(result)) == _ffi.MI_ENOTSUP
    # `_` is a byte in a needle
    assert fn(_ffi.F_CONTAINS, b"a_c", 3, b"xa_cx", 5, C.byref(result)) == _ffi.MI_OK and result.value == 1
    for op in (0, _ffi.F_EQ, _ffi.F_STARTS_WITH, _ffi.F_AND, 15, 99, -1):                # not one of the four
        assert fn(op, b"a", 1, b"a", 1, C.byref(result)) == _ffi.MI_EINVAL
    with pytest.raises(da.MiError) as e:
        da.filter_like_match("like", "a_c", "abc")
    assert e.value.code == _ffi.MI_ENOTSUP


def test_like_header_alone_under_asan_and_ubsan_equals_python(tmp_path):
    exe = str(tmp_path / "like_match_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I", os.path.join(ROOT, "duckdb-arrow_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sanitize", "like_match_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.split("\n")[:-1]
    unhex = lambda h: b"" if h == "-" else bytes.fromhex(h)
    seen = {"1": 0, "0": 0, "E1": 0, "E2": 0, "E3": 0}
    for line in lines:
        op, pattern, row, answer = line.split(" ")
        op, pattern, row = int(op), unhex(pattern), unhex(row)
        if op not in OPS.values():
            want = "E1"                                   # not one of the four operators
        elif op in (_ffi.F_LIKE, _ffi.F_NOT_LIKE) and b"_" in pattern:
            want = "E2"
        elif op in (_ffi.F_LIKE, _ffi.F_NOT_LIKE) and len([s for s in pattern.split(b"%") if s]) > 8:
            want = "E3"
        else:
            want = "1" if python_says(op, pattern, row) else "0"
        assert answer == want, line
        seen[answer] += 1
    assert len(lines) > 5000 and all(n > 0 for n in seen.values()), seen

"""The reference of the late-materialisation (gather) tests, checked where it can be: without a GPU.

helpers.gather_reference decodes the whole column with the oracle and takes the selected rows with numpy.  Here the same
rows are produced one at a time by a plain Python loop (one oracle call per selected row, bits packed by hand), and the
whole-column half is compared with pyoracle.decode_column where that applies (array offset 0)."""
import numpy as np
import pytest

from oracle import pyoracle as po

from helpers import ST_BAD_OFFSETS, ST_DECIMAL_RANGE, ST_DICT_INDEX, ST_MUL_OVERFLOW, decode_column_reference, gather_reference

NROWS = 3 * 2048 + 300      # windows of 2048, 2048, 2048 and a short last one


def _selection(rng):
    """counts 0, 1 and full, a few hundred scattered rows, and the short last window fully selected"""
    some = np.sort(rng.choice(2048, 300, replace=False))
    some[0], some[-1] = 0, 2047
    return [np.zeros(0, np.int64), np.array([2047]), np.arange(2048), np.arange(300)], \
           [some, np.zeros(0, np.int64), np.array([0]), np.arange(300)]


def _columns(rng, row_offset):
    total = row_offset + NROWS
    bitmap = rng.integers(0, 256, (total + 7) // 8 + 8, dtype=np.uint8)
    for r in (2047, 2 * 2048 + 5, 2 * 2048 + 9):                # the rows damaged below are valid
        bitmap[(row_offset + r) >> 3] |= 1 << ((row_offset + r) & 7)
    lens = rng.choice([0, 1, 12, 13, 30], total)
    off = (3 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    dec = rng.integers(-2**31, 2**31, total).astype(np.int64)
    dec128 = np.stack([dec, dec >> 63], axis=1).reshape(-1).copy()
    dec128[2 * (row_offset + 2047)] = 2**40                     # selected by the first selection, not by the second
    mul = rng.integers(-10**12, 10**12, total).astype(np.int64)
    mul[row_offset + 2 * 2048 + 5] = 2**62
    idx = rng.integers(0, 50, total).astype(np.int16)
    idx[row_offset + 2 * 2048 + 9] = 50                         # == dict_len
    bad_off = off.copy()
    bad_off[row_offset + 2 * 2048 + 2] -= 40                    # row 1 of window 2 ends before it starts
    return bitmap, [
        dict(kind=po.K_COPY, buf1=rng.integers(0, 2**63, total).astype(np.int64), param=8),
        dict(kind=po.K_BOOL, buf1=rng.integers(0, 256, (total + 7) // 8, dtype=np.uint8)),
        dict(kind=po.K_DEC128, buf1=dec128, param=4),
        dict(kind=po.K_STR32, buf1=off, buf2=rng.integers(32, 127, int(off[-1]), dtype=np.uint8), ptr_base=0x7000_0000_0000),
        dict(kind=po.K_STR32, buf1=bad_off, buf2=rng.integers(32, 127, int(off[-1]), dtype=np.uint8)),
        dict(kind=po.K_MUL_I64, buf1=mul, param=1000000),
        dict(kind=po.K_DICT, buf1=idx, param=2 | (1 << 8), param2=50),
    ]


@pytest.mark.parametrize("row_offset", [5, 64])
def test_take_and_pack_equals_a_row_by_row_loop(row_offset):
    rng = np.random.default_rng(row_offset)
    bitmap, columns = _columns(rng, row_offset)
    flags = set()
    for sel in _selection(rng):
        for col in columns:
            col = dict(col)
            kind, buf1 = col.pop("kind"), col.pop("buf1")
            modes = (dict(validity=bitmap, null_count=-1), dict(validity=bitmap, null_count=0), dict())
            for nulls in modes if kind in (po.K_COPY, po.K_DEC128) else modes[:1]:   # the row loop is slow: all three for two kinds
                data, words, status = gather_reference(kind, NROWS, buf1, sel, row_offset=row_offset, **nulls, **col)
                want_data, want_bits, want_status = [], [], 0
                for w, s in enumerate(sel):
                    for r in s:
                        one, ok, err = decode_column_reference(kind, 1, buf1, row_offset=row_offset + 2048 * w + int(r), **nulls, **col)
                        want_data.append(one.reshape(-1).tobytes())
                        want_bits.append(bool(ok[0]))
                        want_status |= int(err[0])
                total = len(want_bits)
                assert total == sum(len(s) for s in sel) and len(words) == (total + 63) // 64
                assert data.tobytes() == b"".join(want_data)
                for i in range(64 * len(words)):
                    assert (int(words[i >> 6]) >> (i & 63)) & 1 == (want_bits[i] if i < total else 1), i
                assert status == want_status
                flags.add(status)
                if "validity" not in nulls or nulls["null_count"] == 0:
                    assert (words == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    # the damaged rows were selected by one selection and skipped by the other, so both outcomes were compared
    assert flags >= {0, ST_BAD_OFFSETS, ST_DECIMAL_RANGE, ST_DICT_INDEX, ST_MUL_OVERFLOW}


def test_whole_column_half_equals_the_window_loop_of_the_oracle():
    rng = np.random.default_rng(11)
    bitmap, columns = _columns(rng, 0)
    for col in columns:
        col = dict(col)
        kind, buf1 = col.pop("kind"), col.pop("buf1")
        if kind == po.K_STR32 and "ptr_base" not in col:
            continue    # damaged offsets: the oracle's window loop would follow them
        data, ok, _ = decode_column_reference(kind, NROWS, buf1, validity=bitmap, **col)
        want, words, _ = po.decode_column(kind, col.get("param", 0), NROWS, bitmap, buf1, col.get("buf2"), ptr_base=col.get("ptr_base", 0),
                                          param2=col.get("param2", 0))
        assert np.array_equal(data.reshape(-1), want) and np.array_equal(ok, po.valid_bits(words, NROWS))

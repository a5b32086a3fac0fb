"""bench.py --dump-outputs: a fixed, seeded sample of the vectors the timed path left in HBM, as float .npy files that two
builds can compare file for file.  The CPU test checks the writer on the oracle's decode of the same synthetic stream; the
GPU test runs a plain benchmark and checks its files against the oracle."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import duckdb_arrow_amd as da
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _check_against_oracle(out_dir, buf, first_row=0):
    """Every dumped word and validity bit equals the oracle's vector for that row."""
    _, want = po.decode_stream(buf)
    starts = np.concatenate([[0], np.cumsum([b["nrows"] for b in want])]) + first_row
    files = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(out_dir, "*.npy"))}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_BUDGET
    rows = files.pop("row_index").astype(np.int64)
    assert len(rows) > 0 and np.array_equal(rows, np.unique(rows))
    bi = np.searchsorted(starts, rows, side="right") - 1
    names = [c["name"] for c in want[0]["columns"]]
    assert sorted(files) == sorted(names + [n + "_valid" for n in names])
    for k, name in enumerate(names):
        got_words, got_valid = files[name], files[name + "_valid"]
        assert got_words.shape[0] == got_valid.shape[0] == len(rows)
        for b in np.unique(bi):
            c = want[b]["columns"][k]
            n, sel = want[b]["nrows"], bi == b
            pos = rows[sel] - starts[b]
            words = c["data"].view(np.uint32).reshape(n, c["width"] // 4)[pos]
            assert np.array_equal(got_words[sel], words.astype(np.float64)), (name, b)
            assert np.array_equal(got_valid[sel], po.valid_bits(c["validity"], n)[pos].astype(np.float32)), (name, b)
    return rows


def test_the_sample_is_fixed_and_fits_the_budget():
    sf10 = [122880] * 488 + [59986052 - 488 * 122880]
    s1, s2 = bench.dump_sample(sf10), bench.dump_sample(sf10)
    assert list(s1) == list(s2) and all(np.array_equal(s1[b], s2[b]) for b in s1)
    assert len(s1) == bench.DUMP_BATCHES and 0 in s1 and len(sf10) - 1 in s1
    # lineitem's vectors: 7 x 8-byte integers / decimals, 3 x 4-byte dates, 6 x 16-byte string_t
    words_per_row = 7 * 2 + 3 * 1 + 6 * 4
    rows = sum(len(p) for p in s1.values())
    assert rows * (8 * words_per_row + 4 * 16 + 8) <= bench.DUMP_BUDGET
    one = bench.dump_sample([1000])   # a table smaller than the sample: every row
    assert list(one) == [0] and np.array_equal(one[0], np.arange(1000))


def test_written_outputs_are_the_vectors(tmp_path):
    """The writer on the oracle's decode (the same layout the kernels produce, bit for bit): words and validity come back."""
    buf, info = da.synth_lineitem_stream(scale_factor=10.0, seed=7, n_rows=40000, rows_per_batch=8192, with_validity=True)
    _, want = po.decode_stream(buf)
    sample = bench.dump_sample([b["nrows"] for b in want])
    starts = 1000 + np.concatenate([[0], np.cumsum([b["nrows"] for b in want])[:-1]])
    total = bench.write_outputs(str(tmp_path), [want[b] if b in sample else None for b in range(len(want))], sample, starts)
    assert 0 < total <= bench.DUMP_BUDGET
    rows = _check_against_oracle(str(tmp_path), buf, first_row=1000)
    assert len(rows) == sum(len(p) for p in sample.values())


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    """A plain run: exactly --steps timed steps, ms_per_step consistent with value, no secondary blocks, and the dumped
    vectors equal the oracle's decode of the stream the run generated."""
    out = str(tmp_path / "out")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "300000", "--steps", "3",
                          "--warmup", "1", "--prewarm-seconds", "0.2", "--dump-outputs", out],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    z = json.loads([ln for ln in run.stdout.split("\n") if ln.startswith("{")][-1])
    assert z["steps"] == 3 and z["warmup"] == 1 and z["full"] is False
    assert z["ms_per_step"] > 0 and z["value"] == pytest.approx(300000 / (z["ms_per_step"] * 1e-3), rel=1e-9)
    assert z["roofline"] is None and z["parity"] is None and z["operator_path"] is None and z["cpu_baseline"] is None
    buf, _ = da.synth_lineitem_stream(scale_factor=10.0, seed=42, n_rows=300000, rows_per_batch=122880, with_validity=True)
    rows = _check_against_oracle(out, buf)
    assert rows.min() < 122880 and rows.max() >= 2 * 122880   # the first and the last (partial) record batch

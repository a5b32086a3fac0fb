#!/usr/bin/env python3
"""Run-end encoded decode (transcode_run_end) on a table resident in HBM, next to the same column stored plain.

One column per run: 60 M rows (--rows), runs of mean length 1, 4, 16, 256 and 4096 (geometric), 10 % NULL runs, values
int32, int64, decimal(15,2) or utf8, run ends int32.  Each case is opened twice with mi_hbm_open -- run-end encoded and
plain -- and timed with mi_hbm_launch_timed (median of --iters launches).  The run-end kernel's time is the misc class of
the run-end plan (its values decode in the copy / dec128 / string class); the plain column's time is its own class
(transcode_copy for the integers).  Algorithmic bytes of the expansion: rows x out_width + rows / 8 (validity words) +
runs x (run-end width + value out width).  One JSON line per case.  For kernel times from the trace, run it under
`rocprofv3 --kernel-trace --stats -- python tools/ree_bench.py ...`."""
import argparse
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import duckdb_arrow_amd as da  # noqa: E402
from duckdb_arrow_amd import _ffi  # noqa: E402
from duckdb_arrow_amd.hbm import HbmStream  # noqa: E402

CLASS_NAMES = ["copy", "dec128", "string", "misc", "enc_fixed", "enc_string", "gather"]
OUT_WIDTH = {"int32": 4, "int64": 8, "decimal": 8, "utf8": 16}
PLAIN_CLASS = {"int32": 0, "int64": 0, "decimal": 1, "utf8": 2}


def runs(n, mean, rng):
    if mean <= 1:
        return np.arange(1, n + 1, dtype=np.int32)
    lens = rng.geometric(1.0 / mean, size=int(n / mean * 1.2) + 16)
    ends = np.cumsum(lens)
    ends = ends[ends < n]
    return np.append(ends, n).astype(np.int32)


def values(kind, m, rng):
    null = rng.random(m) < 0.1
    mask = pa.py_buffer(np.packbits(~null, bitorder="little").tobytes())
    v = rng.integers(0, 1 << 30, m)
    if kind == "int32":
        return pa.Array.from_buffers(pa.int32(), m, [mask, pa.py_buffer(v.astype(np.int32).tobytes())], int(null.sum()))
    if kind == "int64":
        return pa.Array.from_buffers(pa.int64(), m, [mask, pa.py_buffer(v.astype(np.int64).tobytes())], int(null.sum()))
    if kind == "decimal":
        d = np.zeros((m, 2), np.int64)
        d[:, 0] = v
        return pa.Array.from_buffers(pa.decimal128(15, 2), m, [mask, pa.py_buffer(d.tobytes())], int(null.sum()))
    lens = (v % 24).astype(np.int32)   # inline and long strings
    offs = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwx" * 2, np.uint8)
    pos = np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1].astype(np.int64), lens)
    return pa.Array.from_buffers(pa.utf8(), m, [mask, pa.py_buffer(offs.tobytes()), pa.py_buffer(data[pos % 24].tobytes())],
                                 int(null.sum()))


def stream(col, rows_per_batch):
    t = pa.table({"c": col})
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, t.schema) as w:
        w.write_table(t, max_chunksize=rows_per_batch)
    return np.frombuffer(sink.getvalue(), np.uint8)


def time_stream(ctx, buf, iters):
    hs = HbmStream(ctx, buf)
    hs.launch()
    assert hs.status() == 0
    ms = [hs.plan.launch_timed() for _ in range(iters)]
    assert hs.status() == 0
    stats = hs.plan.class_stats()
    hs.close()
    return [float(np.median([m[c] for m in ms])) for c in range(_ffi.NUM_KERNEL_CLASSES)], stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60_000_000)
    ap.add_argument("--rows-per-batch", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", default="1,4,16,256,4096")
    ap.add_argument("--values", default="int32,int64,decimal,utf8")
    a = ap.parse_args()
    ctx = da.Context(0)
    rng = np.random.default_rng(7)
    for kind in a.values.split(","):
        for mean in [int(x) for x in a.runs.split(",")]:
            ends = runs(a.rows, mean, rng)
            vals = values(kind, len(ends), rng)
            ree = pa.RunEndEncodedArray.from_arrays(pa.array(ends, pa.int32()), vals)
            idx = np.searchsorted(ends, np.arange(a.rows, dtype=np.int64), side="right")
            plain = vals.take(pa.array(idx))
            del idx
            ree_ms, ree_stats = time_stream(ctx, stream(ree, a.rows_per_batch), a.iters)
            plain_ms, _ = time_stream(ctx, stream(plain, a.rows_per_batch), a.iters)
            w = OUT_WIDTH[kind]
            alg = a.rows * w + a.rows // 8 + len(ends) * (4 + w)
            k_ms = ree_ms[3]
            p_ms = plain_ms[PLAIN_CLASS[kind]]
            print(json.dumps(dict(values=kind, mean_run=mean, rows=a.rows, runs=len(ends), run_end_ms=round(k_ms, 4),
                                  algorithmic_bytes=alg, tb_per_s=round(alg / k_ms / 1e9, 3) if k_ms else None,
                                  share_of_8tbs=round(alg / k_ms / 1e9 / 8, 3) if k_ms else None,
                                  values_decode_ms=round(ree_ms[PLAIN_CLASS[kind]], 4),
                                  misc_class_bytes=ree_stats[3]["bytes_read"] + ree_stats[3]["bytes_written"],
                                  plain_kernel=CLASS_NAMES[PLAIN_CLASS[kind]], plain_ms=round(p_ms, 4),
                                  ratio_to_plain=round(k_ms / p_ms, 3) if p_ms else None)), flush=True)
            del ree, plain, vals
    ctx.close()


if __name__ == "__main__":
    main()

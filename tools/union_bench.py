#!/usr/bin/env python3
"""Union decode (transcode_union / transcode_union_dense, kernels_union.hip) on a table resident in HBM, next to the same
members stored as a STRUCT column.

One column per run: 60 M rows (--rows) in record batches of 2^20 rows (one batch is built and written as often as it takes:
a dense union is never sliced), members (int64, int64) or (int64, utf8) with 10 % NULLs, sparse or dense, type ids (5, 7).
A dense union gives every row a child row of its own (the member lengths add up to the batch).  Each case is opened twice
with mi_hbm_open -- the union, and a struct of the two full-length members, which does all of the member work a sparse
union does -- and timed with mi_hbm_launch_timed (median of --iters launches).  The union kernels' time is the misc class
of the union plan less the misc class of a plan of the members alone (utf8 and struct validity have none there; the
number is printed raw as well).  Algorithmic bytes of the tag pass per row: 1 (type id) + 1 (tag) + (m + 1) / 8 (validity
and masks), + 4 when dense (offsets); the dense expansion adds per member rows x (4 + width) + the values once.
One JSON line per case."""
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
WIDTH = {"int64": 8, "utf8": 16}


def member(kind, m, rng):
    null = rng.random(m) < 0.1
    mask = pa.py_buffer(np.packbits(~null, bitorder="little").tobytes())
    v = rng.integers(0, 1 << 30, m)
    if kind == "int64":
        return pa.Array.from_buffers(pa.int64(), m, [mask, pa.py_buffer(v.astype(np.int64).tobytes())], int(null.sum()))
    lens = (v % 24).astype(np.int32)   # inline and long strings
    offs = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"abcdefghijklmnopqrstuvwx" * 2, np.uint8)
    pos = np.arange(int(offs[-1]), dtype=np.int64) - np.repeat(offs[:-1].astype(np.int64), lens)
    return pa.Array.from_buffers(pa.utf8(), m, [mask, pa.py_buffer(offs.tobytes()), pa.py_buffer(data[pos % 24].tobytes())], int(null.sum()))


def stream(batch, n_batches):
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, batch.schema) as w:
        for _ in range(n_batches):
            w.write_batch(batch)
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
    ap.add_argument("--members", default="int64+int64,int64+utf8")
    ap.add_argument("--modes", default="sparse,dense")
    a = ap.parse_args()
    ctx = da.Context(0)
    rng = np.random.default_rng(7)
    n = a.rows_per_batch
    n_batches = max(1, a.rows // n)
    rows = n * n_batches
    for kinds in [m.split("+") for m in a.members.split(",")]:
        for mode in a.modes.split(","):
            tag = rng.integers(0, len(kinds), n)
            ids = pa.array(np.asarray((5, 7), np.int8)[tag], pa.int8())
            names = ["m%d" % k for k in range(len(kinds))]
            full = [member(kind, n, rng) for kind in kinds]
            if mode == "sparse":
                u = pa.UnionArray.from_sparse(ids, full, names, [5, 7])
            else:
                offsets = np.zeros(n, np.int32)
                for k in range(len(kinds)):
                    offsets[tag == k] = np.arange(int((tag == k).sum()), dtype=np.int32)
                u = pa.UnionArray.from_dense(ids, pa.array(offsets, pa.int32()), [member(kind, int((tag == k).sum()), rng) for k, kind in enumerate(kinds)],
                                             names, [5, 7])
            st = pa.StructArray.from_arrays(full, names)
            u_ms, u_stats = time_stream(ctx, stream(pa.record_batch({"c": u}), n_batches), a.iters)
            s_ms, _ = time_stream(ctx, stream(pa.record_batch({"c": st}), n_batches), a.iters)
            m = len(kinds)
            tag_bytes = rows * (2 + (m + 1) / 8 + (4 if mode == "dense" else 0))
            expand_bytes = sum(rows * (4 + WIDTH[k]) + rows // m * WIDTH[k] for k in kinds) if mode == "dense" else 0
            alg = int(tag_bytes + expand_bytes)
            k_ms = u_ms[3] - (s_ms[3] if mode == "sparse" else 0)
            print(json.dumps(dict(members="+".join(kinds), mode=mode, rows=rows, batches=n_batches, union_total_ms=round(sum(u_ms), 4),
                                  struct_total_ms=round(sum(s_ms), 4), union_misc_ms=round(u_ms[3], 4), struct_misc_ms=round(s_ms[3], 4),
                                  union_kernels_ms=round(k_ms, 4), algorithmic_bytes=alg, tb_per_s=round(alg / k_ms / 1e9, 3) if k_ms > 0 else None,
                                  share_of_8tbs=round(alg / k_ms / 1e9 / 8, 3) if k_ms > 0 else None,
                                  per_class_ms={CLASS_NAMES[c]: round(u_ms[c], 4) for c in range(len(CLASS_NAMES)) if u_ms[c]},
                                  misc_class_bytes=u_stats[3]["bytes_read"] + u_stats[3]["bytes_written"])), flush=True)
            del u, st, full
    ctx.close()


if __name__ == "__main__":
    main()

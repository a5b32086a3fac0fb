#!/usr/bin/env python3
"""Arrow extension-type columns on a table resident in HBM: decode of an arrow.uuid column (tile_uuid) and of an arrow.bool8
column (tile_bool8), and the encode of the decoded UUID vectors as text (encode_uuid_text).

One column per case: 40 M rows (--rows; config 5's row count) in record batches of 122 880 rows (a row group of the
writer: one batch is built and written as often as it takes), 10 % NULLs.  Each case is opened with mi_hbm_open and timed
with mi_hbm_launch_timed: --runs runs (3) of the median of --iters launches each, so the spread between runs is printed
beside the figure.  Next to each extension column the same bytes WITHOUT the extension name: fixed_size_binary(16), which
binds as BLOB (string_t rows that point into the body, the string kernel) -- what the column was read as before the name was
honoured -- and int8, which binds as TINYINT (transcode_copy).  Algorithmic bytes per row: uuid 16 in + 16 out, bool8 1 + 1,
blob 16 out (the bytes stay where they are), + 2 / 8 for the bitmap and the validity words; the text encoder 16 in + 36 out
per valid row + 4 (int32 offsets) + 2 / 8.
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


def column(case, n, rng):
    null = rng.random(n) < 0.1
    mask = pa.py_buffer(np.packbits(~null, bitorder="little").tobytes())
    if case in ("uuid", "blob16"):
        storage = pa.Array.from_buffers(pa.binary(16), n, [mask, pa.py_buffer(rng.integers(0, 256, 16 * n, dtype=np.uint8).tobytes())], int(null.sum()))
        return pa.ExtensionArray.from_storage(pa.uuid(), storage) if case == "uuid" else storage
    storage = pa.Array.from_buffers(pa.int8(), n, [mask, pa.py_buffer(rng.integers(0, 256, n, dtype=np.uint8).tobytes())], int(null.sum()))
    return pa.ExtensionArray.from_storage(pa.bool8(), storage) if case == "bool8" else storage


def stream(batch, n_batches):
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, batch.schema) as w:
        for _ in range(n_batches):
            w.write_batch(batch)
    return np.frombuffer(sink.getvalue(), np.uint8)


def spread(runs):
    return dict(ms=round(float(np.median(runs)), 4), runs_ms=[round(float(r), 4) for r in runs],
                spread_pct=round(100 * (max(runs) - min(runs)) / float(np.median(runs)), 2))


def encode_text(torch, ctx, hs, a):
    """MI_K_ENC_UUID_TEXT over the decoded vectors of `hs`, one task per record batch (= row group), one plan"""
    spans, total = [], 0
    for lay in hs.layout:
        n, e = lay["nrows"], lay["columns"][0]
        sizes = [(n + 7) // 8, (n + 1) * 4, 36 * n]
        offs = []
        for s in sizes:
            offs.append(total)
            total += (s + 63) // 64 * 64 + 64
        spans.append((n, e, offs))
    arena = torch.zeros(total + 256, dtype=torch.uint8, device="cuda")
    ab = arena.data_ptr()
    tasks = [da.make_task(_ffi.K_ENC_UUID_TEXT, n, hs.out_ptr + e["data_off"], ab + offs[1], validity=hs.out_ptr + e["valid_off"],
                          out_validity=ab + offs[0], out_aux=ab + offs[2], param=16) for n, e, offs in spans]
    plan = da.Plan(ctx, tasks)
    s = torch.cuda.current_stream().cuda_stream
    plan.launch(s)
    assert plan.status() == 0
    nulls = sum(plan.null_counts())
    runs = [float(np.median([plan.launch_timed(s)[4] for _ in range(a.iters)])) for _ in range(a.runs)]
    # the first row group, read back by pyarrow
    n, e, offs = spans[0]
    host = arena[: offs[2] + 36 * n].cpu().numpy()
    got = pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(host[offs[0]: offs[0] + (n + 7) // 8].tobytes()),
                                                  pa.py_buffer(host[offs[1]: offs[1] + 4 * (n + 1)].tobytes()), pa.py_buffer(host[offs[2]:].tobytes())])
    got.validate(full=True)
    plan.close()
    rows = sum(n for n, _, _ in spans)
    return runs, rows, nulls, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40_000_000)
    ap.add_argument("--rows-per-batch", type=int, default=122_880)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default="uuid,blob16,bool8,int8")
    a = ap.parse_args()
    import torch
    ctx = da.Context(0)
    rng = np.random.default_rng(11)
    n = a.rows_per_batch
    n_batches = max(1, a.rows // n)
    rows = n * n_batches
    for case in a.cases.split(","):
        arr = column(case, n, rng)
        hs = HbmStream(ctx, stream(pa.record_batch({"c": arr}), n_batches))
        hs.launch()
        assert hs.status() == 0
        runs = []
        for _ in range(a.runs):
            ms = [hs.plan.launch_timed() for _ in range(a.iters)]
            runs.append(float(np.median([sum(m) for m in ms])))
        per_class = {CLASS_NAMES[c]: round(float(np.median([m[c] for m in ms])), 4) for c in range(len(CLASS_NAMES)) if ms[-1][c]}
        per_row = {"uuid": 32, "blob16": 16, "bool8": 2, "int8": 2}[case] + 0.25
        t = spread(runs)
        print(json.dumps(dict(case="decode_" + case, kind=hs.layout[0]["columns"][0]["kind"], rows=rows, batches=n_batches, **t,
                              algorithmic_bytes=int(rows * per_row), gb_per_s=round(rows * per_row / t["ms"] / 1e6, 1), per_class_ms=per_class)), flush=True)
        if case == "uuid":
            eruns, erows, nulls, got = encode_text(torch, ctx, hs, a)
            want = [None if v is None else str(v) for v in arr.to_pylist()]
            assert got.to_pylist() == want, "the first row group's text differs from str(uuid.UUID)"
            alg = erows * (16 + 4 + 0.25) + (erows - nulls) * 36
            t = spread(eruns)
            print(json.dumps(dict(case="encode_uuid_text", rows=erows, nulls=int(nulls), tasks=n_batches, **t, algorithmic_bytes=int(alg),
                                  gb_per_s=round(alg / t["ms"] / 1e6, 1), first_row_group_equals_python=True)), flush=True)
        hs.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Kernel-level timing of K6 on resident values: the one-leaf range (mi_filter_range on int32 / int64, mi_filter_between on
float32 / float64 / int128 -- the same rows pass in every dtype) and, for int32, a compacting gather (transcode_gather)
behind it through the scan operator's own entry points; for int128, transcode_copy over the same column as its yardstick.
HIP-event-free: wall clock around 20 launches.
--dtype string: one string leaf (--op contains | ends_with | like | not_like | starts_with, --pattern) over a VARCHAR column
resident in HBM: --column l_comment or l_shipinstruct of the seeded lineitem (csrc/synth_lineitem.cpp), decoded once by
transcode_string into string_t rows that point into the stream's HBM copy.  Times are device events around 20 launches
(mi_filter_string); TB/s is over 16 bytes per row plus the payload bytes of the rows longer than 12, the bytes such a leaf
has to read.  transcode_string over the same column (its own timed launch) is reported beside it as the ceiling: it reads the
same rows' offsets and payload once and writes the 16 bytes the leaf reads."""
import argparse, sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import duckdb_arrow_amd as da
from duckdb_arrow_amd import _ffi
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["int32", "int64", "float32", "float64", "int128", "string"], default="int32")
ap.add_argument("--rows", type=int, default=None, help="default 240 M, 30 M for --dtype string")
ap.add_argument("--op", choices=["contains", "ends_with", "like", "not_like", "starts_with"], default="contains")
ap.add_argument("--pattern", default="special")
ap.add_argument("--column", choices=["l_comment", "l_shipinstruct"], default="l_comment")
args = ap.parse_args()
ctx = da.Context(0)
n = args.rows or (30_000_000 if args.dtype == "string" else 240_000_000)
out = {"rows": n}


def string_leaf():
    from duckdb_arrow_amd.hbm import HbmStream
    buf, info = da.synth_lineitem_stream(n_rows=n, rows_per_batch=n, seed=42, with_validity=False)   # one record batch
    hs = HbmStream(ctx, buf, columns=[args.column], pointer_mode=_ffi.HBM_PTR_DEVICE)
    del buf
    hs.launch()
    assert hs.status() == 0
    col = hs.layout[0]["columns"][0]
    assert col["name"] == args.column and col["nrows"] == n and col["width"] == 16 and col["valid_off"] < 0
    rows = torch.from_numpy(hs._d2h(col["data_off"], 16 * n).view(np.uint32).reshape(n, 4).astype(np.int64))
    lens = rows[:, 0]
    long_rows = lens > 12
    payload = int(lens[long_rows].sum().item())
    heap = hs.in_ptr + col["body_off"] + col["buffers"][2][0]
    sel = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((n + 2047) // 2048, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    op = args.op.replace("_", " ") if args.op == "not_like" else args.op
    launches = lambda: da.filter_pattern_launches() + sum(da.filter_launch_counts())
    before = (da.filter_pattern_launches(), launches())
    da.filter_string(ctx, hs.out_ptr + col["data_off"], 0, n, heap, col["ptr_base"], op, args.pattern, sel.data_ptr(), cnt.data_ptr(), launches=3)
    ms = da.filter_string(ctx, hs.out_ptr + col["data_off"], 0, n, heap, col["ptr_base"], op, args.pattern, sel.data_ptr(), cnt.data_ptr(), launches=20)
    k = int(cnt.sum().item())
    alg = 16 * n + payload
    out["column"] = {"name": args.column, "rows_longer_than_12": int(long_rows.sum().item()), "payload_bytes_of_those": payload,
                     "mean_length": float(lens.double().mean().item())}
    out["filter_program_string"] = {"op": op, "pattern": args.pattern, "ms": ms, "selected": k, "selectivity": k / n, "algorithmic_bytes": alg,
                                    "TBps": alg / ms / 1e9, "pattern_instance": da.filter_pattern_launches() > before[0],
                                    "launches": launches() - before[1]}
    # the ceiling: the decode of the same column, timed by the plan (offsets and payload in, 16 bytes per row out)
    hs.plan.launch_timed()
    ms_classes = hs.plan.launch_timed()
    stats = [c for c in hs.plan.class_stats() if c["rows"] > 0]
    assert len(stats) == 1, stats
    t_ms = max(ms_classes)
    out["transcode_string"] = {"kernel": stats[0]["kernel"], "ms": t_ms, "bytes_read": stats[0]["bytes_read"], "bytes_written": stats[0]["bytes_written"],
                               "TBps": (stats[0]["bytes_read"] + stats[0]["bytes_written"]) / t_ms / 1e9,
                               "leaf_bytes_TBps": alg / t_ms / 1e9}
    out["filter_ms_over_transcode_ms"] = ms / t_ms
    print(json.dumps(out))


if args.dtype == "string":
    string_leaf()
    sys.exit(0)
width = {"int32": 4, "int64": 8, "float32": 4, "float64": 8, "int128": 16}[args.dtype]
ints = torch.randint(8036, 10562, (n,), dtype=torch.int64 if width > 4 else torch.int32, device="cuda")
if args.dtype == "int128":     # hugeint_t{uint64 lower; int64 upper}, upper = 0
    vals = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    vals[:, 0] = ints
    del ints
elif args.dtype.startswith("float"):
    vals = ints.to(torch.float32 if width == 4 else torch.float64)
    del ints
else:
    vals = ints
sel = torch.empty(n, dtype=torch.int32, device="cuda")
cnt = torch.zeros((n + 2047) // 2048, dtype=torch.int32, device="cuda")
s = torch.cuda.current_stream().cuda_stream
if args.dtype in ("int32", "int64"):
    launch = lambda: da.filter_range(ctx, vals.data_ptr(), width, 0, n, 8766, 9131, sel.data_ptr(), cnt.data_ptr(), s)
else:   # lo <= v <= hi: the rows of 8766 <= v < 9131
    launch = lambda: da.filter_between(ctx, vals.data_ptr(), width, 0, n, 8766, 9130, sel.data_ptr(), cnt.data_ptr(), s)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


ms = timed(launch)
k = int(cnt.sum().item())
alg = width * n + 4 * k + cnt.numel() * 4
out["filter_program_range_" + args.dtype] = {"ms": ms, "G_rows_per_s": n / ms / 1e6, "selectivity": k / n, "algorithmic_bytes": alg, "GBps": alg / ms / 1e6}
out["filter_launches_base_extended"] = list(da.filter_launch_counts())
if args.dtype == "int128":
    out["filter_program_range_int128"]["note"] = "every launch uploads its 32 bytes of bounds and waits for the kernel (mi_filter_between)"
    # the yardstick: the flat copy of the same column (16 bytes in, 16 bytes out per row)
    dst = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    plan = da.Plan(ctx, [da.make_task(_ffi.K_COPY, n, vals.data_ptr(), dst.data_ptr(), param=16, null_count=0)])
    ms = timed(lambda: plan.launch(s))
    assert plan.status() == 0 and torch.equal(dst[:4096], vals[:4096])
    out["transcode_copy_int128"] = {"ms": ms, "algorithmic_bytes": 32 * n, "GBps": 32 * n / ms / 1e6}
if args.dtype == "int32":
    # late materialisation behind it: an int64 column gathered through the selection vector into a dense array
    src = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device="cuda")
    dst = torch.empty(k + 64, dtype=torch.int64, device="cuda")
    task = da.make_task(_ffi.K_COPY, n, src.data_ptr(), dst.data_ptr(), param=8, null_count=0, sel=sel.data_ptr(), sel_count=cnt.data_ptr())
    plan = da.Plan(ctx, [task])
    ms = timed(lambda: plan.launch(s))
    assert plan.status() == 0
    # spot check against torch
    w0 = int(cnt[0].item())
    want = src[:2048][sel[:w0].long()]
    assert torch.equal(dst[:w0], want)
    alg = 4 * k + 8 * k + 8 * k + cnt.numel() * 4   # sel + the selected values in and out
    out["transcode_gather_int64"] = {"ms": ms, "selected": k, "algorithmic_bytes": alg, "GBps": alg / ms / 1e6,
                                     "note": "the source column is touched sector-wise: at 14 % selectivity nearly every 64-byte line holds a selected row"}
print(json.dumps(out))

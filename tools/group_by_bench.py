#!/usr/bin/env python3
"""mi_scan_group_aggregate beside mi_scan_aggregate (*Grouped aggregates*): the TPC-H Q1 shape -- GROUP BY
l_returnflag, l_linestatus, eight aggregates, l_shipdate <= 1998-09-02 -- over lineitem SF as 8 files, device-resident scan, one
process, against the ungrouped call with the same eight aggregates and the same filter; the variants alternate, --runs runs each
after one warm-up, MI_AGG_TIMING=1 (wall time per run, device time per launch of the kernels).  Then the window-limit case: a
synthetic table whose every 2048-row window holds 256 distinct keys, grouped and ungrouped.  --q1 adds a third variant to the
first part, alternating with the other two: TPC-H Q1 whole, the same keys and filter with Q1's own six aggregates, two of them
expression sums of two and three factors (MI_AGG_SUM_EXPR).  Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MI_AGG_TIMING"] = "1"

AGGS = [("sum", "l_quantity"), ("sum", "l_extendedprice"), ("sum_product", "l_extendedprice", "l_discount"), ("sum_product", "l_extendedprice", "l_tax"),
        ("count_star",), ("min", "l_shipdate"), ("max", "l_shipdate"), ("count", "l_comment")]
Q1_AGGS = [("sum", "l_quantity"), ("sum", "l_extendedprice"), ("sum_expr", "l_extendedprice", ("l_discount", -1, 100)),
           ("sum_expr", "l_extendedprice", ("l_discount", -1, 100), ("l_tax", 1, 100)), ("sum", "l_discount"), ("count_star",)]
KEYS = ["l_returnflag", "l_linestatus"]
CUTOFF = 10471      # DATE '1998-09-02'


def timed(make, call, counters):
    rel = make()
    before = counters()
    t0 = time.perf_counter()
    got = call(rel)
    dt = time.perf_counter() - t0
    after = counters()
    rel.close()
    launches = after[0] - before[0]
    return dt, got, {"launches": launches, "windows_ms": after[2] - before[2], "combine_ms": after[3] - before[3]}


def alternate(variants, runs):
    """variants: {name: (make, call, counters)}; one warm-up each, then `runs` rounds in which the variants alternate"""
    out = {name: {"wall_s": [], "kernels": []} for name in variants}
    for name, v in variants.items():
        timed(*v)
    for _ in range(runs):
        for name, v in variants.items():
            dt, got, k = timed(*v)
            out[name]["wall_s"].append(round(dt, 4))
            out[name]["kernels"].append({a: round(b, 3) if isinstance(b, float) else b for a, b in k.items()})
            out[name]["result"] = got
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit-rows", type=int, default=122880 * 130)
    ap.add_argument("--q1", action="store_true", help="also run TPC-H Q1 whole: six aggregates, two of them expression sums")
    args = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.ipc as ipc
    import duckdb_arrow_amd as da
    buf, info = da.synth_lineitem_stream(scale_factor=args.sf, seed=42)
    d = os.path.join(args.dir, "mi_group_bench_%d" % os.getpid())
    os.makedirs(d, exist_ok=True)
    n_files = 8
    paths = [os.path.join(d, "lineitem_%d.arrows" % i) for i in range(n_files)]
    limit_path = os.path.join(d, "limit.arrows")
    out = {"rows": info["n_rows"], "files": n_files}
    try:
        offs, nb = info["batch_offsets"], info["n_batches"]
        per = (nb + n_files - 1) // n_files
        for i, p in enumerate(paths):
            lo, hi = offs[min(nb, i * per)], offs[min(nb, (i + 1) * per)]
            with open(p, "wb") as f:
                f.write(buf[: offs[0]].tobytes())
                f.write(memoryview(buf[lo:hi]))
                f.write(b"\xff\xff\xff\xff\x00\x00\x00\x00")
        del buf
        con = da.Connection(0)
        expr = ("l_shipdate", "<=", CUTOFF)
        make = lambda: con.read_arrow(paths, device_resident=True).filter(expr)
        variants = {"ungrouped": (make, lambda r: r.aggregate(AGGS, detail=True), da.aggregate_counters),
                    "grouped": (make, lambda r: r.group_aggregate(KEYS, AGGS, detail=True), da.group_aggregate_counters)}
        if args.q1:
            variants["q1_whole"] = (make, lambda r: r.group_aggregate(KEYS, Q1_AGGS, detail=True), da.group_aggregate_counters)
        q1 = alternate(variants, args.runs)
        whole = q1["q1_whole"].pop("result") if args.q1 else None
        groups, scanned, selected = q1["grouped"].pop("result")
        totals, scanned_u, selected_u = q1["ungrouped"].pop("result")
        assert (scanned, selected) == (scanned_u, selected_u)
        # the groups add up to the ungrouped call's sums and counts
        for a in (0, 1, 2, 3, 4, 7):
            assert sum(g[1][a] for g in groups) == totals[a], (a, totals[a])
        assert min(g[1][5] for g in groups) == totals[5] and max(g[1][6] for g in groups) == totals[6]
        out["q1"] = dict(q1, scanned=scanned, selected=selected, groups=[[list(k), v] for k, v in groups])
        if whole is not None:
            wgroups, wscanned, wselected = whole
            assert (wscanned, wselected) == (scanned, selected) and [k for k, _ in wgroups] == [k for k, _ in groups]
            # sum(price * (100 - disc)) is 100 sum(price) - sum(price * disc), group by group; the counts are the other variant's
            for (_, w), (_, g) in zip(wgroups, groups):
                assert w[0] == g[0] and w[1] == g[1] and w[2] == 100 * g[1] - g[2] and w[5] == g[4], (w, g)
            out["q1"]["whole_groups"] = [[list(k), v] for k, v in wgroups]

        # ---- the window-limit case: 256 distinct keys in every 2048-row window
        n = args.limit_rows
        schema = pa.schema([("k", pa.int32()), ("v", pa.int64()), ("x", pa.float64())])
        rng = np.random.default_rng(1)
        with ipc.new_stream(limit_path, schema) as w:
            for first in range(0, n, 122880):
                m = min(122880, n - first)
                rows = np.arange(first, first + m)
                w.write_batch(pa.record_batch([pa.array((rows % 256).astype(np.int32)), pa.array(rows.astype(np.int64)), pa.array(rng.normal(0, 1, m))], schema=schema))
        aggs = [("count_star",), ("sum", "v"), ("min", "v"), ("max", "v"), ("sum", "x"), ("min", "x"), ("max", "x"), ("count", "x")]
        make = lambda: con.read_arrow(limit_path, device_resident=True)
        lim = alternate({"ungrouped": (make, lambda r: r.aggregate(aggs, detail=True), da.aggregate_counters),
                         "grouped_256_keys_per_window": (make, lambda r: r.group_aggregate(["k"], aggs, detail=True), da.group_aggregate_counters)}, args.runs)
        groups, scanned, _ = lim["grouped_256_keys_per_window"].pop("result")
        totals, _, _ = lim["ungrouped"].pop("result")
        assert len(groups) == 256 and sum(g[1][0] for g in groups) == n == totals[0] and sum(g[1][1] for g in groups) == totals[1] == n * (n - 1) // 2
        out["window_limit"] = dict(lim, rows=n)
    finally:
        for p in paths + [limit_path]:
            if os.path.exists(p):
                os.unlink(p)
        os.rmdir(d)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

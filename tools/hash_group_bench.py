#!/usr/bin/env python3
"""mi_hash_aggregate_vectors on resident synthetic lineitem vectors (*Hash GROUP BY*): device time of
hash_group_rows / hash_group_collect from MI_AGG_TIMING=1 and the rows/s and atomic bytes/s they imply, for
  group by l_orderkey   sorted, ~4 rows per group
  group by l_suppkey    scattered
  a 4-group key         worst contention
each with 1 and with 8 integer aggregates; the cases alternate, --runs runs each after one warm-up.  Beside them: K10
(mi_group_aggregate_vectors) on the 4-group key, which is the call to use for few groups, and pyarrow's Table.group_by on the
same host as the only CPU yardstick at hand.  Every result is checked against numpy before it is reported.  Prints one JSON line."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MI_AGG_TIMING"] = "1"

VALUE_DTYPE = [("lo", "<u8"), ("hi", "<i8"), ("count", "<i8"), ("kind", "<i4"), ("is_null", "<i4"), ("reserved", "<i8", 2)]
KEY_DTYPE = [("lo", "<i8"), ("hi", "<i8"), ("kind", "<i4"), ("is_null", "<i4")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6000000, help="lineitem rows (SF1 has 6 M)")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.ipc as ipc
    import torch
    import duckdb_arrow_amd as da
    from duckdb_arrow_amd import _ffi, _agg_check_specs, _agg_vector_specs

    buf, info = da.synth_lineitem_stream(scale_factor=max(args.rows / 6.0e6, 0.001), seed=42, n_rows=args.rows, with_validity=False)
    table = ipc.open_stream(pa.py_buffer(buf)).read_all()
    n = table.num_rows

    def stored(name):
        col = table.column(name).combine_chunks()
        if pa.types.is_decimal(col.type):      # the unscaled integers (DECIMAL(15,2): the scan stores them in 8 bytes): the low words
            return np.frombuffer(col.buffers()[1], np.int64)[col.offset * 2: (col.offset + n) * 2: 2].copy()
        if pa.types.is_date32(col.type):
            return col.cast(pa.int32()).to_numpy()
        return col.to_numpy()

    host = {name: np.ascontiguousarray(stored(name)) for name in ("l_orderkey", "l_suppkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_shipdate")}
    host["four"] = (np.arange(n) % 4).astype(np.int32)
    dev = {name: torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).cuda() for name, v in host.items()}
    col = lambda name: (dev[name].data_ptr(), 0, host[name].dtype.itemsize, "signed")
    one = [("sum", col("l_quantity"))]
    eight = [("sum", col("l_quantity")), ("sum", col("l_extendedprice")), ("sum_product", col("l_extendedprice"), col("l_discount")),
             ("sum_product", col("l_extendedprice"), col("l_tax")), ("count_star",), ("min", col("l_shipdate")), ("max", col("l_shipdate")),
             ("count", col("l_discount"))]
    agg_classes = {"any": _ffi.AGG_CLASS_ANY, "signed": _ffi.AGG_CLASS_SIGNED, "unsigned": _ffi.AGG_CLASS_UNSIGNED, "float": _ffi.AGG_CLASS_FLOAT,
                   "wide": _ffi.AGG_CLASS_WIDE}
    ctx = da.Context(0)
    L = _ffi.lib()
    distinct = {k: int(len(np.unique(host[k]))) for k in ("l_orderkey", "l_suppkey", "four")}
    qty_total = int(host["l_quantity"].sum())

    def hash_call(key, specs):
        """one mi_hash_aggregate_vectors through ctypes: the result stays in ctypes arrays (no Python object per group)"""
        checked = _agg_check_specs(specs)
        arr, keep = _agg_vector_specs(checked, agg_classes)
        max_groups = distinct[key]
        kcol = _ffi.GroupKeyColumn()
        kcol.data, kcol.validity, kcol.width, kcol.key_class = dev[key].data_ptr(), None, host[key].dtype.itemsize, _ffi.GROUP_KEY_CLASS_SIGNED
        out_k, out_v, ng = (_ffi.GroupKeyValue * max_groups)(), (_ffi.AggValue * (max_groups * len(checked)))(), C.c_int32()

        def run():
            before = da.hash_aggregate_counters()
            t0 = time.perf_counter()
            _ffi.check(L.mi_hash_aggregate_vectors(ctx._h, C.byref(kcol), arr, len(checked), None, None, n, max_groups, out_k, out_v, max_groups,
                                                   C.byref(ng), None))
            wall = time.perf_counter() - t0
            after = da.hash_aggregate_counters()
            values = np.frombuffer(out_v, VALUE_DTYPE).reshape(max_groups, len(checked))
            keys = np.frombuffer(out_k, KEY_DTYPE)
            assert ng.value == max_groups and int(values["lo"][:, 0].sum()) == qty_total and (np.diff(keys["lo"]) > 0).all()
            if len(checked) == 8:
                assert int(values["lo"][:, 4].sum()) == n and int(values["lo"][:, 5].astype(np.int64).min()) == int(host["l_shipdate"].min())
            return {"wall_s": round(wall, 4), "rows_ms": round(after[2] - before[2], 4), "collect_ms": round(after[3] - before[3], 4)}
        # what a row sends to the table: the claim, and per aggregate a count and (all but the counts) a value word
        atomic_bytes = n * (8 + sum(8 if name in ("count_star", "count") else 16 for name, _ in checked))
        return run, atomic_bytes, keep

    def k10_call(specs):
        def run():
            t0 = time.perf_counter()
            got = da.group_aggregate_vectors(ctx, [col("four")], specs, n)
            wall = time.perf_counter() - t0
            assert len(got) == 4 and sum(g[1][0] for g in got) == qty_total
            return {"wall_s": round(wall, 4)}
        return run

    cases = {}
    for key in ("l_orderkey", "l_suppkey", "four"):
        for label, specs in (("1", one), ("8", eight)):
            cases["%s/%s" % (key, label)] = hash_call(key, specs)
    out = {"rows": n, "groups": distinct, "runs": args.runs, "hash": {}, "k10_four": {}}
    for name, (run, _, _) in cases.items():
        run()      # warm-up
    results = {name: [] for name in cases}
    for _ in range(args.runs):      # the cases alternate
        for name, (run, _, _) in cases.items():
            results[name].append(run())
    for name, (_, atomic_bytes, _) in cases.items():
        best = min(r["rows_ms"] for r in results[name])
        out["hash"][name] = {"runs": results[name], "best_rows_ms": best, "rows_per_s": round(n / (best * 1e-3)) if best > 0 else None,
                             "atomic_GB_per_s": round(atomic_bytes / (best * 1e-3) / 1e9, 1) if best > 0 else None}
    # K10 on the 4-group key: WALL time of the vector call (its device time is reported by the scan entry alone), to be
    # held against the hash cases' wall_s, not against their device milliseconds
    for label, specs in (("1", one), ("8", eight)):
        run = k10_call(specs)
        run()
        out["k10_four"][label] = [run() for _ in range(args.runs)]
    # pyarrow on the same host
    pat = pa.table({"l_orderkey": host["l_orderkey"], "l_suppkey": host["l_suppkey"], "four": host["four"], "l_quantity": host["l_quantity"]})
    out["pyarrow_group_by_sum_s"] = {}
    for key in ("l_orderkey", "l_suppkey", "four"):
        t0 = time.perf_counter()
        g = pat.group_by(key).aggregate([("l_quantity", "sum")])
        out["pyarrow_group_by_sum_s"][key] = round(time.perf_counter() - t0, 4)
        assert g.num_rows == distinct[key]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

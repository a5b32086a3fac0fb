/* TPC-H Q6 and five more aggregates in one pass over lineitem.arrows, through the C ABI alone: the predicates go to
 * mi_scan_set_filter, the aggregates to mi_scan_aggregate, and only the results leave the GPU.
 *
 *   gcc -std=c99 -Iinclude examples/agg.c -Lduckdb-arrow_amd -lmi_arrow_ipc -Wl,-rpath,$PWD/duckdb-arrow_amd -o agg
 *   ./agg lineitem.arrows [more files...]
 *
 * SELECT sum(l_extendedprice * l_discount), count(*), min(l_shipdate), max(l_shipdate), sum(l_quantity),
 *        sum(l_extendedprice * (1 - l_discount))
 *   FROM read_arrow(files)
 *  WHERE l_shipdate >= DATE '1994-01-01' AND l_shipdate < DATE '1995-01-01'
 *    AND l_discount BETWEEN 0.05 AND 0.07 AND l_quantity < 24
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_arrow_ipc.h"

static void check(int rc, const char* what) {
  if (rc != MI_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, mi_last_error());
    exit(1);
  }
}

static mi_filter_node leaf(int32_t op, const char* column, int64_t value) {
  mi_filter_node n;
  memset(&n, 0, sizeof(n));
  n.op = op;
  n.column = column;
  n.value = value;
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.arrows [file.arrows ...]\n", argv[0]);
    return 2;
  }
  mi_ctx* ctx = NULL;
  check(mi_ctx_create(0, &ctx), "mi_ctx_create");
  mi_scan_options opts;
  memset(&opts, 0, sizeof(opts));
  opts.device_resident = 1; /* nothing is handed back as vectors */
  mi_scan* scan = NULL;
  check(mi_scan_open_files(ctx, (const char* const*)(argv + 1), argc - 1, &opts, &scan), "mi_scan_open_files");
  int32_t n_fields = 0;
  check(mi_scan_bind(scan, NULL, 0, &n_fields), "mi_scan_bind");

  /* stored integers: DATE = days since 1970-01-01, DECIMAL(15,2) 0.05 = 5 */
  mi_filter_node nodes[6];
  memset(&nodes[0], 0, sizeof(nodes[0]));
  nodes[0].op = MI_F_AND;
  nodes[0].first_child = 1;
  nodes[0].n_children = 5;
  nodes[1] = leaf(MI_F_GE, "l_shipdate", 8766);
  nodes[2] = leaf(MI_F_LT, "l_shipdate", 9131);
  nodes[3] = leaf(MI_F_GE, "l_discount", 5);
  nodes[4] = leaf(MI_F_LE, "l_discount", 7);
  nodes[5] = leaf(MI_F_LT, "l_quantity", 2400);
  check(mi_scan_set_filter(scan, nodes, 6, 0), "mi_scan_set_filter");

  /* an expression: the product of up to four factors add + mul * column over the stored integers; at scale 2,
   * 1 - l_discount is 100 + (-1) * l_discount */
  mi_agg_expr net;
  memset(&net, 0, sizeof(net));
  net.n_factors = 2;
  net.factors[0].column = "l_extendedprice";
  net.factors[0].mul = 1;
  net.factors[1].column = "l_discount";
  net.factors[1].mul = -1;
  net.factors[1].add = 100;

  mi_agg_spec aggs[6];
  memset(aggs, 0, sizeof(aggs));
  aggs[0].op = MI_AGG_SUM_PRODUCT;
  aggs[0].column_a = "l_extendedprice";
  aggs[0].column_b = "l_discount";
  aggs[1].op = MI_AGG_COUNT_STAR;
  aggs[2].op = MI_AGG_MIN;
  aggs[2].column_a = "l_shipdate";
  aggs[3].op = MI_AGG_MAX;
  aggs[3].column_a = "l_shipdate";
  aggs[4].op = MI_AGG_SUM;
  aggs[4].column_a = "l_quantity";
  aggs[5].op = MI_AGG_SUM_EXPR;
  aggs[5].expr = &net;
  mi_agg_value v[6];
  int64_t scanned = 0, selected = 0;
  check(mi_scan_aggregate(scan, aggs, 6, v, &scanned, &selected), "mi_scan_aggregate");

  if (v[0].is_null) {
    printf("revenue = NULL  (0 of %" PRId64 " rows pass)\n", scanned);
  } else if (v[0].hi != 0 && v[0].hi != -1) {
    printf("revenue does not fit 64 bits: hi=%" PRId64 " lo=%" PRIu64 "\n", v[0].hi, v[0].lo);
  } else {
    const int64_t scaled = (int64_t)v[0].lo; /* DECIMAL(15,2) * DECIMAL(15,2): scale 4 */
    printf("revenue = %" PRId64 ".%04" PRId64 "  (%" PRId64 " of %" PRId64 " rows pass)\n", scaled / 10000, scaled % 10000, selected, scanned);
  }
  printf("count(*) = %" PRIu64 "\n", v[1].lo);
  if (!v[2].is_null) printf("l_shipdate in [%" PRId64 ", %" PRId64 "] days since 1970-01-01\n", (int64_t)v[2].lo, (int64_t)v[3].lo);
  if (!v[4].is_null) printf("sum(l_quantity) = %" PRId64 ".%02" PRId64 " over %" PRId64 " rows\n", (int64_t)v[4].lo / 100, (int64_t)v[4].lo % 100, v[4].count);
  if (!v[5].is_null && (v[5].hi == 0 || v[5].hi == -1))
    printf("sum(l_extendedprice * (1 - l_discount)) = %" PRId64 ".%04" PRId64 "\n", (int64_t)v[5].lo / 10000, (int64_t)v[5].lo % 10000);
  mi_scan_close(scan);
  mi_ctx_destroy(ctx);
  return 0;
}

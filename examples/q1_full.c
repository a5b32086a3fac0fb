/* TPC-H Q1, whole, over lineitem.arrows, through the C ABI alone: the predicate goes to mi_scan_set_filter, the keys and
 * six aggregates to ONE mi_scan_group_aggregate call, and only the groups leave the GPU.
 *
 *   gcc -std=c99 -Iinclude examples/q1_full.c -Lduckdb-arrow_amd -lmi_arrow_ipc -Wl,-rpath,$PWD/duckdb-arrow_amd -o q1_full
 *   ./q1_full lineitem.arrows [more files...]
 *
 * SELECT l_returnflag, l_linestatus, sum(l_quantity) AS sum_qty, sum(l_extendedprice) AS sum_base_price,
 *        sum(l_extendedprice * (1 - l_discount)) AS sum_disc_price,
 *        sum(l_extendedprice * (1 - l_discount) * (1 + l_tax)) AS sum_charge,
 *        avg(l_quantity) AS avg_qty, avg(l_extendedprice) AS avg_price, avg(l_discount) AS avg_disc, count(*) AS count_order
 *   FROM read_arrow(files)
 *  WHERE l_shipdate <= DATE '1998-09-02'
 *  GROUP BY l_returnflag, l_linestatus ORDER BY l_returnflag, l_linestatus
 *
 * The four columns are DECIMAL(15, 2): the scan sums their stored integers, so 1 - l_discount is the factor
 * 100 + (-1) * l_discount and 1 + l_tax the factor 100 + 1 * l_tax (MI_AGG_SUM_EXPR); sum_disc_price comes back at scale 4 and
 * sum_charge at scale 6, exact in 128 bits.  The three averages are a sum divided by its count, here on the client: the
 * scan has no AVG.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_arrow_ipc.h"

#define N_KEYS 2
#define N_AGGS 6
#define CAPACITY 64

static void check(int rc, const char* what) {
  if (rc != MI_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, mi_last_error());
    exit(1);
  }
}

static void print_key(const mi_group_key_value* k) {
  if (k->is_null) {
    printf("NULL");
  } else {
    uint32_t len;
    memcpy(&len, k->bytes, 4);
    printf("%.*s", (int)len, (const char*)k->bytes + 4);
  }
}

/* a DECIMAL sum of `digits` digits behind the point that fits 64 bits */
static void print_decimal(const mi_agg_value* v, int64_t unit, int digits) {
  if (v->is_null) {
    printf("  NULL");
  } else if (v->hi != 0 && v->hi != -1) {
    printf("  (beyond 64 bits: hi=%" PRId64 " lo=%" PRIu64 ")", v->hi, v->lo);
  } else {
    const int64_t s = (int64_t)v->lo;
    printf("  %" PRId64 ".%0*" PRId64, s / unit, digits, (s < 0 ? -s : s) % unit);
  }
}

/* avg of a DECIMAL(15, 2) column: its sum over its count of values that are not NULL */
static void print_average(const mi_agg_value* v) {
  if (v->is_null || v->count == 0) printf("  NULL");
  else printf("  %.6f", (double)(int64_t)v->lo / 100.0 / (double)v->count);
}

static mi_agg_factor column_factor(const char* column, int64_t mul, int64_t add) {
  mi_agg_factor f;
  memset(&f, 0, sizeof(f));
  f.column = column;
  f.mul = mul;
  f.add = add;
  f.constants = MI_AGG_CONST_INT;
  return f;
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

  /* the stored integer of a DATE is days since 1970-01-01: 1998-09-02 = 10471 */
  mi_filter_node node;
  memset(&node, 0, sizeof(node));
  node.op = MI_F_LE;
  node.column = "l_shipdate";
  node.value = 10471;
  check(mi_scan_set_filter(scan, &node, 1, 0), "mi_scan_set_filter");

  mi_agg_expr disc_price, charge;
  memset(&disc_price, 0, sizeof(disc_price));
  memset(&charge, 0, sizeof(charge));
  disc_price.n_factors = 2;
  disc_price.factors[0] = column_factor("l_extendedprice", 1, 0);
  disc_price.factors[1] = column_factor("l_discount", -1, 100); /* 1.00 - l_discount */
  charge.n_factors = 3;
  charge.factors[0] = disc_price.factors[0];
  charge.factors[1] = disc_price.factors[1];
  charge.factors[2] = column_factor("l_tax", 1, 100);           /* 1.00 + l_tax */

  const char* keys[N_KEYS] = {"l_returnflag", "l_linestatus"};
  mi_agg_spec aggs[N_AGGS];
  memset(aggs, 0, sizeof(aggs));
  aggs[0].op = MI_AGG_SUM;
  aggs[0].column_a = "l_quantity";
  aggs[1].op = MI_AGG_SUM;
  aggs[1].column_a = "l_extendedprice";
  aggs[2].op = MI_AGG_SUM_EXPR;
  aggs[2].expr = &disc_price;
  aggs[3].op = MI_AGG_SUM_EXPR;
  aggs[3].expr = &charge;
  aggs[4].op = MI_AGG_SUM;
  aggs[4].column_a = "l_discount";
  aggs[5].op = MI_AGG_COUNT_STAR;

  static mi_group_key_value out_keys[CAPACITY * N_KEYS];
  static mi_agg_value out_values[CAPACITY * N_AGGS];
  int32_t n_groups = 0;
  int64_t scanned = 0, selected = 0;
  check(mi_scan_group_aggregate(scan, keys, N_KEYS, aggs, N_AGGS, out_keys, out_values, CAPACITY, &n_groups, &scanned, &selected),
        "mi_scan_group_aggregate");

  printf("%d groups, %" PRId64 " of %" PRId64 " rows pass\n", (int)n_groups, selected, scanned);
  printf("flag status  sum_qty  sum_base_price  sum_disc_price  sum_charge  avg_qty  avg_price  avg_disc  count_order\n");
  for (int32_t g = 0; g < n_groups; g++) {
    const mi_agg_value* v = out_values + (size_t)g * N_AGGS;
    print_key(&out_keys[g * N_KEYS]);
    printf(" ");
    print_key(&out_keys[g * N_KEYS + 1]);
    print_decimal(&v[0], 100, 2);     /* DECIMAL(15,2) */
    print_decimal(&v[1], 100, 2);
    print_decimal(&v[2], 10000, 4);   /* two DECIMAL(., 2) factors: scale 4 */
    print_decimal(&v[3], 1000000, 6); /* three: scale 6 */
    print_average(&v[0]);
    print_average(&v[1]);
    print_average(&v[4]);
    printf("  %" PRIu64 "\n", v[5].lo);
  }
  mi_scan_close(scan);
  mi_ctx_destroy(ctx);
  return 0;
}

/* A TPC-H Q1-shaped query over lineitem.arrows, through the C ABI alone: the predicate goes to mi_scan_set_filter, the
 * keys and aggregates to mi_scan_group_aggregate, and only the groups leave the GPU.
 *
 *   gcc -std=c99 -Iinclude examples/q1.c -Lduckdb-arrow_amd -lmi_arrow_ipc -Wl,-rpath,$PWD/duckdb-arrow_amd -o q1
 *   ./q1 lineitem.arrows [more files...]
 *
 * SELECT l_returnflag, l_linestatus, sum(l_quantity), sum(l_extendedprice), sum(l_extendedprice * l_discount),
 *        sum(l_extendedprice * l_tax), count(*), min(l_shipdate), max(l_shipdate), count(l_comment)
 *   FROM read_arrow(files)
 *  WHERE l_shipdate <= DATE '1998-09-02'
 *  GROUP BY l_returnflag, l_linestatus ORDER BY l_returnflag, l_linestatus
 *
 * This is the shape of Q1 with every kind of aggregate in it (sums, products, a count, a minimum, a maximum, a COUNT of
 * a string column).  Q1 itself, whole -- sum_disc_price = sum(price * (1 - discount)), sum_charge = sum(price * (1 -
 * discount) * (1 + tax)) and the three averages, in one call -- is examples/q1_full.c, through MI_AGG_SUM_EXPR.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_arrow_ipc.h"

#define N_KEYS 2
#define N_AGGS 8
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
  } else if (k->kind == MI_GROUP_KEY_STRING) {
    uint32_t len;
    memcpy(&len, k->bytes, 4);
    printf("%.*s", (int)len, (const char*)k->bytes + 4);
  } else {
    int64_t lo;
    memcpy(&lo, k->bytes, 8);
    printf("%" PRId64, lo);
  }
}

/* a DECIMAL sum of `scale` digits that fits 64 bits */
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

  const char* keys[N_KEYS] = {"l_returnflag", "l_linestatus"};
  mi_agg_spec aggs[N_AGGS];
  memset(aggs, 0, sizeof(aggs));
  aggs[0].op = MI_AGG_SUM;
  aggs[0].column_a = "l_quantity";
  aggs[1].op = MI_AGG_SUM;
  aggs[1].column_a = "l_extendedprice";
  aggs[2].op = MI_AGG_SUM_PRODUCT;
  aggs[2].column_a = "l_extendedprice";
  aggs[2].column_b = "l_discount";
  aggs[3].op = MI_AGG_SUM_PRODUCT;
  aggs[3].column_a = "l_extendedprice";
  aggs[3].column_b = "l_tax";
  aggs[4].op = MI_AGG_COUNT_STAR;
  aggs[5].op = MI_AGG_MIN;
  aggs[5].column_a = "l_shipdate";
  aggs[6].op = MI_AGG_MAX;
  aggs[6].column_a = "l_shipdate";
  aggs[7].op = MI_AGG_COUNT;
  aggs[7].column_a = "l_comment";

  static mi_group_key_value out_keys[CAPACITY * N_KEYS];
  static mi_agg_value out_values[CAPACITY * N_AGGS];
  int32_t n_groups = 0;
  int64_t scanned = 0, selected = 0;
  check(mi_scan_group_aggregate(scan, keys, N_KEYS, aggs, N_AGGS, out_keys, out_values, CAPACITY, &n_groups, &scanned, &selected),
        "mi_scan_group_aggregate");

  printf("%d groups, %" PRId64 " of %" PRId64 " rows pass\n", (int)n_groups, selected, scanned);
  printf("flag status  sum_qty  sum_base_price  sum(price*disc)  sum(price*tax)  count  min_ship  max_ship  comments\n");
  for (int32_t g = 0; g < n_groups; g++) {
    const mi_agg_value* v = out_values + (size_t)g * N_AGGS;
    print_key(&out_keys[g * N_KEYS]);
    printf(" ");
    print_key(&out_keys[g * N_KEYS + 1]);
    print_decimal(&v[0], 100, 2);   /* DECIMAL(15,2) */
    print_decimal(&v[1], 100, 2);
    print_decimal(&v[2], 10000, 4); /* DECIMAL(15,2) * DECIMAL(15,2): scale 4 */
    print_decimal(&v[3], 10000, 4);
    printf("  %" PRIu64, v[4].lo);
    if (v[5].is_null) printf("  NULL  NULL");
    else printf("  %" PRId64 "  %" PRId64, (int64_t)v[5].lo, (int64_t)v[6].lo);
    printf("  %" PRIu64 "\n", v[7].lo);
  }
  mi_scan_close(scan);
  mi_ctx_destroy(ctx);
  return 0;
}

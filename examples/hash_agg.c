/* The inner query of TPC-H Q18 over lineitem.arrows, through the C ABI alone: a GROUP BY with one group per order -- far
 * more groups than mi_scan_group_aggregate takes -- goes to mi_scan_hash_aggregate, and only the groups leave the GPU.
 *
 *   gcc -std=c99 -Iinclude examples/hash_agg.c -Lduckdb-arrow_amd -lmi_arrow_ipc -Wl,-rpath,$PWD/duckdb-arrow_amd -o hash_agg
 *   ./hash_agg [-q quantity] lineitem.arrows [more files...]
 *
 * SELECT l_orderkey, sum(l_quantity), count(*)
 *   FROM read_arrow(files)
 *  GROUP BY l_orderkey HAVING sum(l_quantity) > quantity        -- Q18: 300
 *
 * The scan has no HAVING: the client applies it to the groups it gets back, which come sorted by l_orderkey.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi_arrow_ipc.h"

#define N_AGGS 2
#define MAX_GROUPS (1 << 22) /* orders this client is prepared for; SF10 has 15 M: MI_MAX_HASH_GROUPS is 2^24 */

static void check(int rc, const char* what) {
  if (rc != MI_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, mi_last_error());
    exit(1);
  }
}

int main(int argc, char** argv) {
  int64_t quantity = 300;
  int first = 1;
  if (argc >= 3 && strcmp(argv[1], "-q") == 0) {
    quantity = strtoll(argv[2], NULL, 10);
    first = 3;
  }
  if (argc <= first) {
    fprintf(stderr, "usage: %s [-q quantity] file.arrows [file.arrows ...]\n", argv[0]);
    return 2;
  }
  mi_ctx* ctx = NULL;
  check(mi_ctx_create(0, &ctx), "mi_ctx_create");
  mi_scan_options opts;
  memset(&opts, 0, sizeof(opts));
  opts.device_resident = 1; /* nothing is handed back as vectors */
  mi_scan* scan = NULL;
  check(mi_scan_open_files(ctx, (const char* const*)(argv + first), argc - first, &opts, &scan), "mi_scan_open_files");
  int32_t n_fields = 0;
  check(mi_scan_bind(scan, NULL, 0, &n_fields), "mi_scan_bind");

  mi_agg_spec aggs[N_AGGS];
  memset(aggs, 0, sizeof(aggs));
  aggs[0].op = MI_AGG_SUM;
  aggs[0].column_a = "l_quantity";
  aggs[1].op = MI_AGG_COUNT_STAR;

  mi_group_key_value* out_keys = (mi_group_key_value*)calloc(MAX_GROUPS, sizeof(mi_group_key_value));
  mi_agg_value* out_values = (mi_agg_value*)calloc((size_t)MAX_GROUPS * N_AGGS, sizeof(mi_agg_value));
  if (!out_keys || !out_values) {
    fprintf(stderr, "out of memory\n");
    return 1;
  }
  int32_t n_groups = 0;
  int64_t scanned = 0, selected = 0;
  check(mi_scan_hash_aggregate(scan, "l_orderkey", aggs, N_AGGS, MAX_GROUPS, out_keys, out_values, MAX_GROUPS, &n_groups, &scanned, &selected),
        "mi_scan_hash_aggregate");

  /* l_quantity is DECIMAL(15,2): the sum is in hundredths */
  const int64_t threshold = quantity * 100;
  int64_t kept = 0;
  printf("%d orders in %" PRId64 " rows\n", (int)n_groups, scanned);
  printf("l_orderkey  sum_qty  lines\n");
  for (int32_t g = 0; g < n_groups; g++) {
    const mi_agg_value* v = out_values + (size_t)g * N_AGGS;
    if (v[0].is_null || v[0].hi != 0 || (int64_t)v[0].lo <= threshold) continue; /* HAVING (a sum past 64 bits is not a lineitem) */
    int64_t key;
    memcpy(&key, out_keys[g].bytes, 8);
    const int64_t s = (int64_t)v[0].lo;
    if (out_keys[g].is_null) printf("NULL");
    else printf("%" PRId64, key);
    printf("  %" PRId64 ".%02" PRId64 "  %" PRIu64 "\n", s / 100, s % 100, v[1].lo);
    kept++;
  }
  printf("%" PRId64 " orders with sum(l_quantity) > %" PRId64 "\n", kept, quantity);
  free(out_keys);
  free(out_values);
  mi_scan_close(scan);
  mi_ctx_destroy(ctx);
  return 0;
}

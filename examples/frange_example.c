/* frange_example.c -- range search through the forest, beside the exact one, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/frange_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o frange_example
 *   ./frange_example
 * Appends rows, builds the forest, takes the first B stored rows as queries and each query's own K-th exact key as its threshold, counts the
 * forest range search's hits with capacity 0, allocates, searches, and prints the share of zh_search_range_batch's hits that the visited leaves
 * held: the hit recall of the forest setting at that radius and probe. */
#include <stdio.h>
#include <stdlib.h>

#include "zebra_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        int rc_ = (call);                                                    \
        if (rc_ != ZH_OK) {                                                  \
            fprintf(stderr, "%s: %d: %s\n", #call, rc_, zh_last_error());    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main(void) {
    enum { N = 20000, D = 256, B = 64, K = 16, PROBE = 1 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    opt.max_node_size = 512;
    opt.num_trees = 8;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 2)); /* clustered rows */
    CHECK(zh_index_build(ix));

    /* queries: the first B stored rows; thresholds: each query's K-th smallest exact key */
    float *q = malloc(sizeof(float) * B * D);
    uint64_t *kids = malloc(sizeof(uint64_t) * B * K), *kkeys = malloc(sizeof(uint64_t) * B * K), *max_keys = malloc(sizeof(uint64_t) * B);
    uint32_t *kcounts = malloc(sizeof(uint32_t) * B);
    uint64_t *offsets = malloc(sizeof(uint64_t) * (B + 1)), *exact_offsets = malloc(sizeof(uint64_t) * (B + 1));
    if (!q || !kids || !kkeys || !max_keys || !kcounts || !offsets || !exact_offsets) return 1;
    CHECK(zh_index_read_rows(ix, 0, B, q));
    CHECK(zh_search_exact_batch(ix, q, B, K, ZH_L2SQ, 0, kids, kkeys, kcounts));
    for (size_t i = 0; i < B; i++) max_keys[i] = kcounts[i] ? kkeys[i * K + kcounts[i] - 1] : 0;

    /* count with capacity 0 (ZH_ELIMIT with the exact total and offsets unless there is no hit), allocate, search */
    uint64_t total = 0, exact_total = 0;
    int rc = zh_search_range_forest_batch(ix, q, B, max_keys, PROBE, ZH_L2SQ, 0, 0, offsets, NULL, NULL, &total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "count: %d: %s\n", rc, zh_last_error()); return 1; }
    uint64_t *ids = malloc(sizeof(uint64_t) * (total + 1)), *keys = malloc(sizeof(uint64_t) * (total + 1));
    if (!ids || !keys) return 1;
    CHECK(zh_search_range_forest_batch(ix, q, B, max_keys, PROBE, ZH_L2SQ, 0, total, offsets, ids, keys, &total));
    zh_range_forest_info info;
    CHECK(zh_search_range_forest_info(ix, &info));

    /* the exact range search's count at the same thresholds: every forest hit is one of its hits */
    rc = zh_search_range_batch(ix, q, B, max_keys, ZH_L2SQ, 0, 0, exact_offsets, NULL, NULL, &exact_total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "exact count: %d: %s\n", rc, zh_last_error()); return 1; }
    printf("forest range search, probe %u: %llu of the exact search's %llu hits (%.4f) on path %u; %u trees, %llu leaf visits holding %llu rows "
           "against %llu of the full scan, %llu candidates, %llu tile products\n",
           info.probe, (unsigned long long)total, (unsigned long long)exact_total, exact_total ? (double)total / (double)exact_total : 1.0, info.path,
           info.trees, (unsigned long long)info.visits, (unsigned long long)info.leaf_rows, (unsigned long long)B * N,
           (unsigned long long)info.candidates, (unsigned long long)info.tiles);
    if (total) printf("query 0: %llu hits, the first is id %llu\n", (unsigned long long)(offsets[1] - offsets[0]), (unsigned long long)ids[0]);
    free(q); free(kids); free(kkeys); free(max_keys); free(kcounts); free(offsets); free(exact_offsets); free(ids); free(keys);
    zh_index_destroy(ix);
    return 0;
}

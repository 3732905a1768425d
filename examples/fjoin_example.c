/* fjoin_example.c -- the forest self-join of an index's own rows, beside the exact one, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/fjoin_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o fjoin_example
 *   ./fjoin_example
 * Appends rows, builds the forest, takes a threshold key from a small slab of the forest k-NN graph (the median 8th-nearest key), counts the
 * forest join's pairs with capacity 0, allocates, joins, and prints the share of zh_self_join's pairs that the forest's leaves found: the pair
 * recall of the forest setting at that threshold. */
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

static int by_key(const void *x, const void *y) {
    const uint64_t a = *(const uint64_t *)x, b = *(const uint64_t *)y;
    return a < b ? -1 : a > b;
}

int main(void) {
    enum { N = 20000, D = 256, K = 8, S = 512 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    opt.max_node_size = 512;
    opt.num_trees = 8;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 2)); /* clustered rows */
    CHECK(zh_index_build(ix));

    /* the threshold: the median K-th nearest key of the first S rows */
    uint64_t *gids = malloc(sizeof(uint64_t) * S * K), *gkeys = malloc(sizeof(uint64_t) * S * K), *kth = malloc(sizeof(uint64_t) * S);
    uint32_t *gcounts = malloc(sizeof(uint32_t) * S);
    if (!gids || !gkeys || !kth || !gcounts) return 1;
    CHECK(zh_knn_graph_forest(ix, 0, S, K, ZH_L2SQ, 0, gids, gkeys, gcounts));
    size_t have = 0;
    for (size_t i = 0; i < S; i++)
        if (gcounts[i] == K) kth[have++] = gkeys[i * K + K - 1];
    if (!have) { fprintf(stderr, "no row of the slab has %d leaf-mates\n", K); return 1; }
    qsort(kth, have, sizeof(uint64_t), by_key);
    const uint64_t max_key = kth[have / 2];

    /* count with capacity 0 (ZH_ELIMIT with the exact total unless there is no pair), allocate, join */
    uint64_t total = 0, exact_total = 0;
    int rc = zh_self_join_forest(ix, max_key, ZH_L2SQ, 0, 0, NULL, NULL, NULL, &total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "count: %d: %s\n", rc, zh_last_error()); return 1; }
    uint64_t *a = malloc(sizeof(uint64_t) * (total + 1)), *b = malloc(sizeof(uint64_t) * (total + 1)), *keys = malloc(sizeof(uint64_t) * (total + 1));
    if (!a || !b || !keys) return 1;
    CHECK(zh_self_join_forest(ix, max_key, ZH_L2SQ, 0, total, a, b, keys, &total));
    zh_join_forest_info info;
    CHECK(zh_self_join_forest_info(ix, &info));

    /* the exact join's count at the same threshold: every pair of the forest join is one of its pairs */
    rc = zh_self_join(ix, max_key, ZH_L2SQ, 0, 0, NULL, NULL, NULL, &exact_total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "exact count: %d: %s\n", rc, zh_last_error()); return 1; }
    printf("forest join: %llu of the exact join's %llu pairs (%.4f) on path %u; %u trees, %llu leaf pairs against %llu of the full triangle, "
           "%llu candidates, %llu tile products\n",
           (unsigned long long)total, (unsigned long long)exact_total, exact_total ? (double)total / (double)exact_total : 1.0, info.path, info.trees,
           (unsigned long long)info.leaf_pairs, (unsigned long long)N * (N - 1) / 2, (unsigned long long)info.candidates,
           (unsigned long long)info.tiles);
    if (total) printf("first pair: %llu %llu\n", (unsigned long long)a[0], (unsigned long long)b[0]);
    free(gids); free(gkeys); free(kth); free(gcounts); free(a); free(b); free(keys);
    zh_index_destroy(ix);
    return 0;
}

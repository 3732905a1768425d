/* knn_forest_example.c -- the forest k-NN graph of an index's own rows, beside the exact one, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/knn_forest_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o knn_forest_example
 *   ./knn_forest_example
 * Appends rows, builds the forest, asks both graphs for the same slab and counts how many of the exact neighbours the forest's leaves found:
 * the recall of the forest setting on the index's own rows, with no held-out queries and no walk. */
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
    enum { N = 20000, D = 256, K = 8 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    opt.max_node_size = 512;
    opt.num_trees = 8;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 2)); /* clustered rows */
    CHECK(zh_index_build(ix));

    uint64_t *ids = malloc(sizeof(uint64_t) * N * K), *keys = malloc(sizeof(uint64_t) * N * K);
    uint64_t *fids = malloc(sizeof(uint64_t) * N * K), *fkeys = malloc(sizeof(uint64_t) * N * K);
    uint32_t *counts = malloc(sizeof(uint32_t) * N), *fcounts = malloc(sizeof(uint32_t) * N);
    if (!ids || !keys || !fids || !fkeys || !counts || !fcounts) return 1;
    CHECK(zh_knn_graph(ix, 0, N, K, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_knn_graph_forest(ix, 0, N, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    unsigned long long exact = 0, found = 0;
    for (size_t i = 0; i < N; i++) {
        exact += counts[i];
        for (uint32_t a = 0; a < counts[i]; a++)
            for (uint32_t b = 0; b < fcounts[i]; b++)
                if (ids[i * K + a] == fids[i * K + b]) { found++; break; }
    }
    zh_knn_forest_info info;
    CHECK(zh_knn_graph_forest_info(ix, &info));
    printf("recall@%d of the forest graph: %.4f (%llu lines on path %u, %u trees, %llu leaf pairs against %llu of the full rectangle, %llu tile products)\n",
           K, exact ? (double)found / (double)exact : 0.0, (unsigned long long)info.lines, info.path, info.trees, (unsigned long long)info.pairs,
           (unsigned long long)N * (N - 1), (unsigned long long)info.tiles);
    free(ids); free(keys); free(fids); free(fkeys); free(counts); free(fcounts);
    zh_index_destroy(ix);
    return 0;
}

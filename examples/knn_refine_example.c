/* knn_refine_example.c -- one refinement round over the forest k-NN graph, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/knn_refine_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o knn_refine_example
 *   ./knn_refine_example
 * Appends rows, builds the forest, makes the forest graph (leaf-mates only), refines it once (each row's neighbours' neighbours) and counts
 * how many of the exact graph's neighbours either graph holds: the recall before and after, and the round's `updates`. */
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

enum { N = 20000, D = 256, K = 8 };

static double recall(const uint64_t *ids, const uint32_t *counts, const uint64_t *gids, const uint32_t *gcounts) {
    unsigned long long exact = 0, found = 0;
    for (size_t i = 0; i < N; i++) {
        exact += counts[i];
        for (uint32_t a = 0; a < counts[i]; a++)
            for (uint32_t b = 0; b < gcounts[i]; b++)
                if (ids[i * K + a] == gids[i * K + b]) { found++; break; }
    }
    return exact ? (double)found / (double)exact : 0.0;
}

int main(void) {
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    opt.max_node_size = 64;
    opt.num_trees = 3;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 2)); /* clustered rows */
    CHECK(zh_index_build(ix));

    uint64_t *ids = malloc(sizeof(uint64_t) * N * K), *keys = malloc(sizeof(uint64_t) * N * K);
    uint64_t *fids = malloc(sizeof(uint64_t) * N * K), *fkeys = malloc(sizeof(uint64_t) * N * K);
    uint64_t *rids = malloc(sizeof(uint64_t) * N * K), *rkeys = malloc(sizeof(uint64_t) * N * K);
    uint32_t *counts = malloc(sizeof(uint32_t) * N), *fcounts = malloc(sizeof(uint32_t) * N), *rcounts = malloc(sizeof(uint32_t) * N);
    if (!ids || !keys || !fids || !fkeys || !rids || !rkeys || !counts || !fcounts || !rcounts) return 1;
    CHECK(zh_knn_graph(ix, 0, N, K, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_knn_graph_forest(ix, 0, N, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    /* the forest graph of the WHOLE table is the input (in_k = K); its keys are not passed: the round computes its own */
    CHECK(zh_knn_graph_refine(ix, fids, fcounts, K, 0, N, K, ZH_L2SQ, 0, rids, rkeys, rcounts));
    zh_knn_refine_info info;
    CHECK(zh_knn_graph_refine_info(ix, &info));
    printf("recall@%d: forest graph %.4f, after one round %.4f (%llu lines, %llu entries listed, %llu pairs keyed, %llu updates)\n", K,
           recall(ids, counts, fids, fcounts), recall(ids, counts, rids, rcounts), (unsigned long long)info.lines, (unsigned long long)info.listed,
           (unsigned long long)info.keyed, (unsigned long long)info.updates);
    free(ids); free(keys); free(fids); free(fkeys); free(rids); free(rkeys); free(counts); free(fcounts); free(rcounts);
    zh_index_destroy(ix);
    return 0;
}

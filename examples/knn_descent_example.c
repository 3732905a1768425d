/* knn_descent_example.c -- NN-descent on the device over the forest k-NN graph, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/knn_descent_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o knn_descent_example
 *   ./knn_descent_example
 * Appends rows, builds the forest, makes the exact graph and the forest graph (leaf-mates only), then asks zh_knn_graph_descent for 1, 2, ..
 * rounds from the same input -- each call is bit for bit the loop over zh_knn_graph_refine_rev with that many rounds -- and prints, round by
 * round, the recall against the exact graph beside what the round keyed (keyed_round), how many lines it had to touch (active_round) and its
 * updates, until a round changes nothing. */
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

enum { N = 20000, D = 256, K = 8, REV_K = 4, ROUNDS = 12 };

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

    const size_t line = sizeof(uint64_t) * N * K;
    uint64_t *ids = malloc(line), *keys = malloc(line), *fids = malloc(line), *fkeys = malloc(line), *out = malloc(line), *okeys = malloc(line);
    uint32_t *counts = malloc(sizeof(uint32_t) * N), *fcounts = malloc(sizeof(uint32_t) * N), *ocounts = malloc(sizeof(uint32_t) * N);
    if (!ids || !keys || !fids || !fkeys || !out || !okeys || !counts || !fcounts || !ocounts) return 1;
    CHECK(zh_knn_graph(ix, 0, N, K, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_knn_graph_forest(ix, 0, N, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    printf("recall@%d of the forest graph: %.4f\n", K, recall(ids, counts, fids, fcounts));

    for (size_t rounds = 1; rounds <= ROUNDS; rounds++) {
        zh_knn_descent_info info;
        CHECK(zh_knn_graph_descent(ix, fids, fcounts, K, REV_K, K, rounds, ZH_L2SQ, 0, out, okeys, ocounts));
        CHECK(zh_knn_graph_descent_info(ix, &info));
        if (info.rounds_run < rounds) break; /* the call before reached the fixed point */
        printf("round %2u: recall@%d %.4f  keyed %llu  active lines %llu of %llu  updates %llu\n", (unsigned)info.rounds_run, K,
               recall(ids, counts, out, ocounts), (unsigned long long)info.keyed_round[rounds - 1], (unsigned long long)info.active_round[rounds - 1],
               (unsigned long long)info.rows_live, (unsigned long long)info.updates_round[rounds - 1]);
        if (!info.updates) break; /* a fixed point */
    }
    free(ids); free(keys); free(fids); free(fkeys); free(out); free(okeys);
    free(counts); free(fcounts); free(ocounts);
    zh_index_destroy(ix);
    return 0;
}

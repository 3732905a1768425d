/* knn_reverse_example.c -- refinement rounds with and without reverse neighbours over the forest k-NN graph, through the C ABI
 * (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/knn_reverse_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o knn_reverse_example
 *   ./knn_reverse_example
 * Appends rows, builds the forest, makes the exact graph and the forest graph (leaf-mates only), prints the forest graph's hubness (the
 * in-degrees zh_knn_graph_reverse returns), then runs ROUNDS rounds of zh_knn_graph_refine and of zh_knn_graph_refine_rev from the same input and
 * prints, round by round, how many of the exact graph's neighbours either arm holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zebra_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        int rc_ = (call);                                                    \
        if (rc_ != ZH_OK) {                                                  \
            fprintf(stderr, "%s: %d: %s\n", #call, rc_, zh_last_error());    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

enum { N = 20000, D = 256, K = 8, REV_K = 8, ROUNDS = 3 };

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
    uint64_t *ids = malloc(line), *keys = malloc(line), *fids = malloc(line), *fkeys = malloc(line);
    uint64_t *in = malloc(line), *out = malloc(line), *okeys = malloc(line), *rev = malloc(sizeof(uint64_t) * N * REV_K);
    uint32_t *counts = malloc(sizeof(uint32_t) * N), *fcounts = malloc(sizeof(uint32_t) * N), *icounts = malloc(sizeof(uint32_t) * N);
    uint32_t *ocounts = malloc(sizeof(uint32_t) * N), *rcounts = malloc(sizeof(uint32_t) * N), *degree = malloc(sizeof(uint32_t) * N);
    if (!ids || !keys || !fids || !fkeys || !in || !out || !okeys || !rev || !counts || !fcounts || !icounts || !ocounts || !rcounts || !degree) return 1;
    CHECK(zh_knn_graph(ix, 0, N, K, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_knn_graph_forest(ix, 0, N, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    printf("recall@%d of the forest graph: %.4f\n", K, recall(ids, counts, fids, fcounts));

    /* the capped reverse graph on its own: up to REV_K sampled in-neighbours per row, and every row's uncapped in-degree */
    CHECK(zh_knn_graph_reverse(ix, fids, fcounts, K, REV_K, 0, N, rev, rcounts, degree));
    zh_knn_reverse_info rinfo;
    CHECK(zh_knn_graph_reverse_info(ix, &rinfo));
    printf("forest graph transposed: %llu edges, largest in-degree %llu, %llu reverse neighbours kept (none of them mutual)\n",
           (unsigned long long)rinfo.edges, (unsigned long long)rinfo.max_degree, (unsigned long long)rinfo.kept);

    for (int arm = 0; arm < 2; arm++) { /* 0: forward only, 1: with reverse neighbours; the same input for both */
        memcpy(in, fids, line);
        memcpy(icounts, fcounts, sizeof(uint32_t) * N);
        for (int r = 1; r <= ROUNDS; r++) {
            unsigned long long updates, keyed;
            if (arm == 0) {
                zh_knn_refine_info info;
                CHECK(zh_knn_graph_refine(ix, in, icounts, K, 0, N, K, ZH_L2SQ, 0, out, okeys, ocounts));
                CHECK(zh_knn_graph_refine_info(ix, &info));
                updates = info.updates; keyed = info.keyed;
            } else {
                zh_knn_refine_rev_info info;
                CHECK(zh_knn_graph_refine_rev(ix, in, icounts, K, REV_K, 0, N, K, ZH_L2SQ, 0, out, okeys, ocounts));
                CHECK(zh_knn_graph_refine_rev_info(ix, &info));
                updates = info.updates; keyed = info.keyed;
            }
            printf("%s round %d: recall@%d %.4f (%llu pairs keyed, %llu updates)\n", arm ? "with reverse" : "forward only", r, K,
                   recall(ids, counts, out, ocounts), keyed, updates);
            if (!updates) break; /* a fixed point */
            memcpy(in, out, line);
            memcpy(icounts, ocounts, sizeof(uint32_t) * N);
        }
    }
    free(ids); free(keys); free(fids); free(fkeys); free(in); free(out); free(okeys); free(rev);
    free(counts); free(fcounts); free(icounts); free(ocounts); free(rcounts); free(degree);
    zh_index_destroy(ix);
    return 0;
}

/* graph_steered_example.c -- filter-steered graph search through the C ABI (include/zebra_hip.h): a selective "this tenant's records" filter.
 *   cc -std=c99 -I include examples/graph_steered_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o graph_steered_example
 *   ./graph_steered_example
 * Appends rows and builds the forest, makes a k-NN graph (forest graph, NN-descent) and attaches it (zh_index_set_graph).  Then one filter --
 * every fiftieth row is the tenant's -- serves four calls from the same allowed seeds: zh_search_graph_filtered_batch walks the graph through
 * EVERY row and answers from the allowed rows it happened to key; zh_search_graph_steered_batch keeps its beam to allowed rows, with hops = 1
 * following only edges between allowed rows and with hops = 2 also hopping over one disallowed row; zh_search_exact_filtered_batch ranks all
 * allowed rows.  Prints each walk's recall@10 against the exact answer and the rows it keyed per query. */
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

enum { N = 20000, D = 256, K = 16, REV_K = 8, ROUNDS = 8, B = 256, TOP = 10, N_SEED = 32, EVERY = 50, BEAM = 64, WIDTH = 4 };

static double recall(const uint64_t *ids, const uint32_t *counts, const uint64_t *gids, const uint32_t *gcounts) {
    unsigned long long exact = 0, found = 0;
    for (size_t i = 0; i < B; i++) {
        exact += counts[i];
        for (uint32_t a = 0; a < counts[i]; a++)
            for (uint32_t b = 0; b < gcounts[i]; b++)
                if (ids[i * TOP + a] == gids[i * TOP + b]) { found++; break; }
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

    /* the graph: leaf-mates first, then NN-descent's rounds on the device */
    const size_t line = sizeof(uint64_t) * N * K;
    uint64_t *fids = malloc(line), *fkeys = malloc(line), *gids = malloc(line), *gkeys = malloc(line);
    uint32_t *fcounts = malloc(sizeof(uint32_t) * N), *gcounts = malloc(sizeof(uint32_t) * N);
    if (!fids || !fkeys || !gids || !gkeys || !fcounts || !gcounts) return 1;
    CHECK(zh_knn_graph_forest(ix, 0, N, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    CHECK(zh_knn_graph_descent(ix, fids, fcounts, K, REV_K, K, ROUNDS, ZH_L2SQ, 0, gids, gkeys, gcounts));
    CHECK(zh_index_set_graph(ix, gids, gcounts, N, K));

    /* the filter: bit r & 31 of word r >> 5 set = stored row r is allowed; here every fiftieth row */
    const uint64_t n_bits = N;
    uint32_t *filter = calloc((N + 31) / 32, sizeof(uint32_t));
    if (!filter) return 1;
    for (uint64_t r = 0; r < N; r += EVERY) filter[r >> 5] |= 1u << (r & 31);

    /* the queries: stored rows, each moved a little; the seeds: N_SEED allowed rows strided over the table, the same for every query (the
     * steered walk ignores a seed that is not allowed) */
    float *q = malloc(sizeof(float) * B * D);
    uint64_t *seeds = malloc(sizeof(uint64_t) * B * N_SEED);
    uint64_t *eids = malloc(sizeof(uint64_t) * B * TOP), *ekeys = malloc(sizeof(uint64_t) * B * TOP);
    uint64_t *ids = malloc(sizeof(uint64_t) * B * TOP), *keys = malloc(sizeof(uint64_t) * B * TOP);
    uint32_t *ecounts = malloc(sizeof(uint32_t) * B), *counts = malloc(sizeof(uint32_t) * B);
    if (!q || !seeds || !eids || !ekeys || !ids || !keys || !ecounts || !counts) return 1;
    for (size_t i = 0; i < B; i++) {
        CHECK(zh_index_read_rows(ix, (uint64_t)(i * 77 + 5) % N, 1, q + i * D));
        for (size_t j = 0; j < D; j++) q[i * D + j] += 0.05f * (float)((i * 31 + j * 17) % 13) - 0.3f;
        for (size_t j = 0; j < N_SEED; j++) seeds[i * N_SEED + j] = (uint64_t)(j * (N / EVERY) / N_SEED) * EVERY;
    }
    CHECK(zh_search_exact_filtered_batch(ix, q, B, TOP, ZH_L2SQ, 0, filter, n_bits, eids, ekeys, ecounts));

    zh_graph_filtered_info blind;
    CHECK(zh_search_graph_filtered_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, WIDTH, 0, ZH_L2SQ, 0, filter, n_bits, ids, keys, counts));
    CHECK(zh_search_graph_filtered_info(ix, &blind));
    printf("%llu of %d rows allowed, beam %d, width %d\n", (unsigned long long)blind.rows_allowed, N, BEAM, WIDTH);
    printf("blind walk: recall@%d %.4f  (per query keyed %.1f, of them allowed %.1f)\n", TOP, recall(eids, ecounts, ids, counts),
           (double)blind.keyed / B, (double)blind.offered / B);
    for (int hops = 1; hops <= 2; hops++) {
        zh_graph_steered_info info;
        CHECK(zh_search_graph_steered_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, WIDTH, 0, ZH_L2SQ, 0, filter, n_bits, hops, ids, keys, counts));
        CHECK(zh_search_graph_steered_info(ix, &info));
        printf("hops = %d:   recall@%d %.4f  (per query keyed %.1f: %.1f direct, %.1f over %.1f bridges; %llu full candidate lists)\n", hops, TOP,
               recall(eids, ecounts, ids, counts), (double)info.keyed / B, (double)info.direct / B, (double)info.via_bridge / B,
               (double)info.bridges / B, (unsigned long long)info.cand_full);
    }
    CHECK(zh_index_drop_graph(ix));
    free(fids); free(fkeys); free(gids); free(gkeys); free(fcounts); free(gcounts); free(filter);
    free(q); free(seeds); free(eids); free(ekeys); free(ids); free(keys); free(ecounts); free(counts);
    zh_index_destroy(ix);
    return 0;
}

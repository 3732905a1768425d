/* graph_prune_example.c -- k-NN graph pruning through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/graph_prune_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o graph_prune_example
 *   ./graph_prune_example
 * Appends rows (no forest is built), makes the exact k-NN graph (zh_knn_graph), attaches it and walks it (zh_search_graph_batch), then prunes it
 * with reverse edges (zh_knn_graph_prune: a line keeps a neighbour only if no neighbour kept before it is closer to it than the row itself),
 * attaches the pruned graph and walks that from the same seeds.  Prints the mean degree, and recall@10 against zh_search_exact_batch and the rows
 * a query keyed, before and after. */
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

enum { N = 20000, D = 256, K = 32, REV_K = 16, DEGREE = 16, B = 256, TOP = 10, N_SEED = 32, BEAM = 64 };

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

static double mean_degree(const uint32_t *counts) {
    unsigned long long s = 0;
    for (size_t i = 0; i < N; i++) s += counts[i];
    return (double)s / N;
}

int main(void) {
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 0)); /* iid rows */

    uint64_t *gids = malloc(sizeof(uint64_t) * N * K), *gkeys = malloc(sizeof(uint64_t) * N * K);
    uint64_t *pids = malloc(sizeof(uint64_t) * N * DEGREE), *pkeys = malloc(sizeof(uint64_t) * N * DEGREE);
    uint32_t *gcounts = malloc(sizeof(uint32_t) * N), *pcounts = malloc(sizeof(uint32_t) * N);
    float *q = malloc(sizeof(float) * B * D);
    uint64_t *seeds = malloc(sizeof(uint64_t) * B * N_SEED);
    uint64_t *eids = malloc(sizeof(uint64_t) * B * TOP), *ekeys = malloc(sizeof(uint64_t) * B * TOP);
    uint64_t *ids = malloc(sizeof(uint64_t) * B * TOP), *keys = malloc(sizeof(uint64_t) * B * TOP);
    uint32_t *ecounts = malloc(sizeof(uint32_t) * B), *counts = malloc(sizeof(uint32_t) * B);
    if (!gids || !gkeys || !pids || !pkeys || !gcounts || !pcounts || !q || !seeds || !eids || !ekeys || !ids || !keys || !ecounts || !counts) return 1;

    /* the queries: stored rows, each moved a little; the seeds: N_SEED rows strided over the table, the same for every query */
    for (size_t i = 0; i < B; i++) {
        CHECK(zh_index_read_rows(ix, (uint64_t)(i * 77 + 5) % N, 1, q + i * D));
        for (size_t j = 0; j < D; j++) q[i * D + j] += 0.05f * (float)((i * 31 + j * 17) % 13) - 0.3f;
        for (size_t j = 0; j < N_SEED; j++) seeds[i * N_SEED + j] = opt.id_base + (uint64_t)j * N / N_SEED;
    }
    CHECK(zh_search_exact_batch(ix, q, B, TOP, ZH_L2SQ, 0, eids, ekeys, ecounts));

    /* the exact graph, walked as it is */
    zh_graph_search_info sinfo;
    CHECK(zh_knn_graph(ix, 0, N, K, ZH_L2SQ, 0, gids, gkeys, gcounts));
    CHECK(zh_index_set_graph(ix, gids, gcounts, N, K));
    CHECK(zh_search_graph_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, 1, 0, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_search_graph_info(ix, &sinfo));
    printf("exact %d-NN graph:  mean degree %5.2f  recall@%d %.4f  keyed per query %.1f\n", K, mean_degree(gcounts), TOP,
           recall(eids, ecounts, ids, counts), (double)sinfo.keyed / B);

    /* pruned over each row's line and up to REV_K of the rows that name it, down to DEGREE unoccluded neighbours */
    zh_knn_prune_info pinfo;
    CHECK(zh_knn_graph_prune(ix, gids, gcounts, K, REV_K, 0, N, DEGREE, 0, ZH_L2SQ, 0, pids, pkeys, pcounts));
    CHECK(zh_knn_graph_prune_info(ix, &pinfo));
    printf("pruned: %llu candidates, %llu kept, %llu occluded, %llu lines cut at %d, %llu keys computed\n", (unsigned long long)pinfo.candidates,
           (unsigned long long)pinfo.kept, (unsigned long long)pinfo.occluded, (unsigned long long)pinfo.cut, DEGREE, (unsigned long long)pinfo.keyed);
    CHECK(zh_index_set_graph(ix, pids, pcounts, N, DEGREE));
    CHECK(zh_search_graph_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, 1, 0, ZH_L2SQ, 0, ids, keys, counts));
    CHECK(zh_search_graph_info(ix, &sinfo));
    printf("pruned to %d (+%d reverse): mean degree %5.2f  recall@%d %.4f  keyed per query %.1f\n", DEGREE, REV_K, mean_degree(pcounts), TOP,
           recall(eids, ecounts, ids, counts), (double)sinfo.keyed / B);

    CHECK(zh_index_drop_graph(ix));
    free(gids); free(gkeys); free(pids); free(pkeys); free(gcounts); free(pcounts);
    free(q); free(seeds); free(eids); free(ekeys); free(ids); free(keys); free(ecounts); free(counts);
    zh_index_destroy(ix);
    return 0;
}

/* graph_extend_example.c -- keeping the attached graph up to date while rows are appended, through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/graph_extend_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o graph_extend_example
 *   ./graph_extend_example
 * Builds the graph (forest k-NN graph, NN-descent, zh_index_set_graph) on the first N0 rows of a table, appends the other N1, and answers queries
 * planted at appended rows by zh_search_graph_batch before and after zh_index_extend_graph.  Before it no line names an appended row: a walk
 * returns only those among its seeds.  The rows are clustered, so a walk needs seeds near its query: queries and new rows alike start from the LSH
 * search's answer (zh_search_batch), for which the appended rows are added to the trees (zh_index_add would do both at once).  Rows of one
 * chunk never name each other and the appended rows are clusters of 128 of their own, so the chunks are kept below a cluster: BATCH = 32.  Prints
 * recall@10 against zh_search_exact_batch, what the extension did, and the table read back (zh_index_get_graph). */
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

enum { N0 = 18000, N1 = 2000, N = N0 + N1, D = 256, K = 16, REV_K = 8, ROUNDS = 8, B = 256, TOP = 10, N_SEED = 32, BEAM = 64, BATCH = 32 };

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
    CHECK(zh_index_append_synthetic(ix, N0, 1, 0, 2)); /* clustered rows */
    CHECK(zh_index_build(ix));

    /* the graph of the first N0 rows */
    const size_t line = sizeof(uint64_t) * N * K;
    uint64_t *fids = malloc(line), *fkeys = malloc(line), *gids = malloc(line), *gkeys = malloc(line);
    uint32_t *fcounts = malloc(sizeof(uint32_t) * N), *gcounts = malloc(sizeof(uint32_t) * N);
    if (!fids || !fkeys || !gids || !gkeys || !fcounts || !gcounts) return 1;
    CHECK(zh_knn_graph_forest(ix, 0, N0, K, ZH_L2SQ, 0, fids, fkeys, fcounts));
    CHECK(zh_knn_graph_descent(ix, fids, fcounts, K, REV_K, K, ROUNDS, ZH_L2SQ, 0, gids, gkeys, gcounts));
    CHECK(zh_index_set_graph(ix, gids, gcounts, N0, K));

    /* the other N1 rows arrive; the forest is built again so that the LSH search, the source of every seed here, sees them */
    CHECK(zh_index_append_synthetic(ix, N1, 1, N0, 2));
    CHECK(zh_index_build(ix));

    /* the queries: appended rows, each moved a little */
    float *q = malloc(sizeof(float) * B * D), *fresh = malloc(sizeof(float) * N1 * D);
    uint64_t *seeds = malloc(sizeof(uint64_t) * B * N_SEED), *nseeds = malloc(sizeof(uint64_t) * N1 * N_SEED), *skeys = malloc(sizeof(uint64_t) * N1 * N_SEED);
    uint64_t *eids = malloc(sizeof(uint64_t) * B * TOP), *ekeys = malloc(sizeof(uint64_t) * B * TOP);
    uint64_t *ids = malloc(sizeof(uint64_t) * B * TOP), *keys = malloc(sizeof(uint64_t) * B * TOP);
    uint32_t *ecounts = malloc(sizeof(uint32_t) * B), *counts = malloc(sizeof(uint32_t) * B), *ncounts = malloc(sizeof(uint32_t) * N1);
    if (!q || !fresh || !seeds || !nseeds || !skeys || !eids || !ekeys || !ids || !keys || !ecounts || !counts || !ncounts) return 1;
    for (size_t i = 0; i < B; i++) {
        CHECK(zh_index_read_rows(ix, N0 + (uint64_t)(i * 7 + 3) % N1, 1, q + i * D));
        for (size_t j = 0; j < D; j++) q[i * D + j] += 0.05f * (float)((i * 31 + j * 17) % 13) - 0.3f;
    }
    CHECK(zh_search_exact_batch(ix, q, B, TOP, ZH_L2SQ, 0, eids, ekeys, ecounts));
    CHECK(zh_search_batch(ix, q, B, N_SEED, ZH_L2SQ, 0, seeds, skeys, counts));
    CHECK(zh_search_graph_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, 1, 0, ZH_L2SQ, 0, ids, keys, counts));
    printf("before the extension: recall@%d %.4f (no line names an appended row: the seeds are all a walk can return of them)\n", TOP,
           recall(eids, ecounts, ids, counts));

    /* the extension: every new row starts from the LSH search's answer for it (a seed naming a row without a line yet is ignored) */
    CHECK(zh_index_read_rows(ix, N0, N1, fresh));
    CHECK(zh_search_batch(ix, fresh, N1, N_SEED, ZH_L2SQ, 0, nseeds, skeys, ncounts));
    CHECK(zh_index_extend_graph(ix, nseeds, N1, N_SEED, BEAM, 1, 0, BATCH, ZH_L2SQ, 0));
    zh_graph_extend_info xi;
    zh_graph_info ginfo;
    CHECK(zh_index_extend_graph_info(ix, &xi));
    CHECK(zh_index_graph_info(ix, &ginfo));
    printf("extended: %llu rows in %llu chunks, %.1f rows keyed per new row; %llu old lines re-ranked, %llu of %llu offered rows kept; %llu lines now\n",
           (unsigned long long)xi.rows_added, (unsigned long long)xi.chunks, xi.rows_added ? (double)xi.keyed / (double)xi.rows_added : 0.0,
           (unsigned long long)xi.reverse_rows, (unsigned long long)xi.reverse_kept, (unsigned long long)xi.reverse_offered,
           (unsigned long long)ginfo.g_rows);
    CHECK(zh_search_graph_batch(ix, q, B, seeds, N_SEED, TOP, BEAM, 1, 0, ZH_L2SQ, 0, ids, keys, counts));
    printf("after the extension:  recall@%d %.4f\n", TOP, recall(eids, ecounts, ids, counts));

    /* the table read back: what a descent round, or a file beside a snapshot, would take */
    CHECK(zh_index_get_graph(ix, 0, N, gids, gcounts));
    unsigned long long entries = 0;
    for (size_t r = 0; r < N; r++) entries += gcounts[r];
    printf("read back: %llu entries in %d lines\n", entries, (int)N);

    CHECK(zh_index_drop_graph(ix));
    free(fids); free(fkeys); free(gids); free(gkeys); free(fcounts); free(gcounts);
    free(q); free(fresh); free(seeds); free(nseeds); free(skeys); free(eids); free(ekeys); free(ids); free(keys); free(ecounts); free(counts); free(ncounts);
    zh_index_destroy(ix);
    return 0;
}

/* knn_graph_example.c -- the exact k-NN graph of an index's own rows through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/knn_graph_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o knn_graph_example
 *   ./knn_graph_example
 * Appends rows (no forest is needed), removes one, and asks for the graph slab by slab: line i of a slab belongs to stored row first_row + i. */
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
    enum { N = 10000, D = 256, K = 8, SLAB = 4096 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    zh_index *ix = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 0));
    const uint64_t gone = 17;
    CHECK(zh_index_remove(ix, &gone, 1, NULL, NULL));

    uint64_t *ids = malloc(sizeof(uint64_t) * SLAB * K), *keys = malloc(sizeof(uint64_t) * SLAB * K);
    uint32_t *counts = malloc(sizeof(uint32_t) * SLAB);
    if (!ids || !keys || !counts) return 1;
    unsigned long long edges = 0;
    for (uint64_t first = 0; first < N; first += SLAB) {
        const uint64_t n = N - first < SLAB ? N - first : SLAB;
        CHECK(zh_knn_graph(ix, first, n, K, ZH_L2SQ, 0, ids, keys, counts));
        for (uint64_t i = 0; i < n; i++) edges += counts[i]; /* 0 for the removed row, K for every other */
        if (first == 0)
            printf("row 0: nearest other row %llu, row 17 (removed): %u neighbours\n", (unsigned long long)ids[0], counts[17]);
    }
    zh_knn_info info;
    CHECK(zh_knn_graph_info(ix, &info));
    printf("%llu edges; the last slab: %llu lines on path %u, %llu survivors, %u panels redone\n", edges, (unsigned long long)info.lines, info.path,
           (unsigned long long)info.survivors, info.redone);
    free(ids);
    free(keys);
    free(counts);
    zh_index_destroy(ix);
    return edges == (unsigned long long)(N - 1) * K ? 0 : 1;
}

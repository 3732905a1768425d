/* xknn_example.c -- the k-NN join between two indexes through the C ABI (include/zebra_hip.h): k-NN classification of an incoming batch.
 *   cc -std=c99 -I include examples/xknn_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o xknn_example
 *   ./xknn_example
 * The corpus holds synthetic rows 0 .. NB - 1, each with a label (here: row number modulo LABELS, a stand-in for what an application keeps
 * beside its vectors).  The batch holds rows NB - DUP .. NB - DUP + NA - 1 of the same series: its first DUP rows are bit-identical to the
 * corpus's last DUP rows, so their nearest corpus row is known.  Every row of the batch is labelled by the majority label of its K nearest
 * corpus rows (ties: the label whose first neighbour is nearest); the two id bases differ, as those of two collections do. */
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
    enum { NA = 64, NB = 20000, D = 256, DUP = 12, K = 5, LABELS = 7 };
    const uint64_t corpus_base = 5000000;
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    zh_index *corpus = NULL, *batch = NULL;
    opt.id_base = corpus_base;
    CHECK(zh_index_create(&opt, &corpus));
    opt.id_base = 0;
    CHECK(zh_index_create(&opt, &batch));
    CHECK(zh_index_append_synthetic(corpus, NB, 1, 0, 0));
    CHECK(zh_index_append_synthetic(batch, NA, 1, NB - DUP, 0)); /* no forest is needed on either side */

    uint64_t *ids = malloc(sizeof(uint64_t) * NA * K), *keys = malloc(sizeof(uint64_t) * NA * K);
    uint32_t *counts = malloc(sizeof(uint32_t) * NA);
    if (!ids || !keys || !counts) return 1;
    CHECK(zh_cross_knn(batch, corpus, 0, NA, K, ZH_L2SQ, 0, ids, keys, counts));
    zh_xknn_info info;
    CHECK(zh_cross_knn_info(batch, &info));
    printf("%llu rows of the batch against %llu rows of the corpus, k = %u: path %u, %llu survivors, %llu tile products\n",
           (unsigned long long)info.lines, (unsigned long long)info.rows_live_b, info.k, info.path, (unsigned long long)info.survivors,
           (unsigned long long)info.tiles);
    int wrong = 0;
    for (int i = 0; i < NA; i++) {
        int votes[LABELS] = {0}, first[LABELS], best = -1;
        for (int l = 0; l < LABELS; l++) first[l] = K;
        for (uint32_t j = 0; j < counts[i]; j++) {
            const int l = (int)((ids[(size_t)i * K + j] - corpus_base) % LABELS); /* the corpus row's label */
            votes[l]++;
            if (first[l] == K) first[l] = (int)j;
        }
        for (int l = 0; l < LABELS; l++)
            if (votes[l] && (best < 0 || votes[l] > votes[best] || (votes[l] == votes[best] && first[l] < first[best]))) best = l;
        if (i < 8)
            printf("batch row %d: label %d; nearest corpus id %llu at key %llu\n", i, best, (unsigned long long)ids[(size_t)i * K],
                   (unsigned long long)keys[(size_t)i * K]);
        /* a planted duplicate's nearest corpus row is its twin, at key 0 */
        if (i < DUP && (counts[i] != K || ids[(size_t)i * K] != corpus_base + NB - DUP + i || keys[(size_t)i * K] != 0)) wrong++;
    }
    free(ids); free(keys); free(counts);
    zh_index_destroy(batch);
    zh_index_destroy(corpus);
    return wrong ? 2 : 0;
}

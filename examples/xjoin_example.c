/* xjoin_example.c -- the join between two indexes through the C ABI (include/zebra_hip.h): which rows of an incoming batch does the corpus
 * already hold?
 *   cc -std=c99 -I include examples/xjoin_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o xjoin_example
 *   ./xjoin_example
 * The corpus B holds synthetic rows 0 .. NB - 1, the batch A rows NB - DUP .. NB - DUP + NA - 1 of the same series: its first DUP rows are
 * bit-identical duplicates of the corpus's last DUP rows.  Counts the pairs at key 0 (L2SQ: distance 0) with capacity 0, allocates, joins,
 * prints the pairs; the two id bases differ, as those of two collections do. */
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
    enum { NA = 4096, NB = 20000, D = 256, DUP = 12 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    zh_index *corpus = NULL, *batch = NULL;
    opt.id_base = 0;
    CHECK(zh_index_create(&opt, &corpus));
    opt.id_base = 1000000;
    CHECK(zh_index_create(&opt, &batch));
    CHECK(zh_index_append_synthetic(corpus, NB, 1, 0, 0));
    CHECK(zh_index_append_synthetic(batch, NA, 1, NB - DUP, 0)); /* no forest is needed on either side */

    /* count with capacity 0 (ZH_ELIMIT with the exact total unless there is no pair), allocate, join */
    const uint64_t max_key = 0;
    uint64_t total = 0;
    int rc = zh_cross_join(batch, corpus, max_key, ZH_L2SQ, 0, 0, NULL, NULL, NULL, &total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "count: %d: %s\n", rc, zh_last_error()); return 1; }
    uint64_t *a = malloc(sizeof(uint64_t) * (total + 1)), *b = malloc(sizeof(uint64_t) * (total + 1)), *keys = malloc(sizeof(uint64_t) * (total + 1));
    if (!a || !b || !keys) return 1;
    CHECK(zh_cross_join(batch, corpus, max_key, ZH_L2SQ, 0, total, a, b, keys, &total));
    zh_cross_info info;
    CHECK(zh_cross_join_info(batch, &info));
    printf("%llu of the batch's %llu rows are in the corpus of %llu already (planted: %d); path %u, %llu candidates, %llu tile products\n",
           (unsigned long long)total, (unsigned long long)info.rows_live_a, (unsigned long long)info.rows_live_b, DUP, info.path,
           (unsigned long long)info.candidates, (unsigned long long)info.tiles);
    for (uint64_t i = 0; i < total; i++)
        printf("batch id %llu = corpus id %llu (key %llu)\n", (unsigned long long)a[i], (unsigned long long)b[i], (unsigned long long)keys[i]);
    free(a); free(b); free(keys);
    zh_index_destroy(batch);
    zh_index_destroy(corpus);
    return total == DUP ? 0 : 2;
}

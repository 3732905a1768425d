/* Plain C99 user of the C ABI (include/zebra_hip.h): insert vectors, search a batch, grow the index, remove, compact, filter, range, self-join.
 *   gcc -std=c99 -Iinclude examples/search_example.c -Lzebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o /tmp/ex && /tmp/ex
 * Mirrors what Database::insert_records / query_vectors do in the reference (src/database/core.rs:245-254, 290-313). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zebra_hip.h"

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != ZH_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, zh_last_error()); return 1; } \
    } while (0)

static float noise(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (float)((*s >> 8) & 0xFFFF) / 65536.0f - 0.5f; }

int main(void) {
    enum { N = 20000, D = 384, B = 8, K = 10 };
    zh_options opt;
    zh_options_default(&opt);          /* max_node_size 5, num_trees 15: the reference defaults (lsh.rs:131-138) */
    opt.dim = D;
    opt.max_node_size = 256;
    zh_index *idx = NULL;
    CHECK(zh_index_create(&opt, &idx));

    float *rows = malloc(sizeof(float) * N * D), *q = malloc(sizeof(float) * B * D);
    unsigned seed = 1;
    for (size_t i = 0; i < (size_t)N * D; i++) rows[i] = noise(&seed);
    for (int b = 0; b < B; b++)
        for (int c = 0; c < D; c++) q[b * D + c] = rows[(size_t)(b * 997) * D + c] + 0.05f * noise(&seed);

    CHECK(zh_index_add(idx, rows, N, NULL));             /* first add builds the forest on the GPU */
    uint64_t ids[B * K], keys[B * K];
    uint32_t counts[B];
    CHECK(zh_search_batch(idx, q, B, K, ZH_L2SQ, 0, ids, keys, counts));
    int hits = 0;
    for (int b = 0; b < B; b++) hits += counts[b] > 0 && ids[b * K] == (uint64_t)(b * 997);
    printf("planted neighbour first for %d of %d queries; %llu vectors, %u trees\n", hits, B,
           (unsigned long long)zh_index_count(idx), zh_index_num_trees(idx));

    CHECK(zh_index_add(idx, rows, 100, NULL));           /* trees exist: incremental insert (duplicates of rows 0..99) */
    size_t removed = 0;
    CHECK(zh_index_deduplicate(idx, NULL, 0, &removed)); /* ...which deduplicate finds again */
    uint64_t gone[2] = {997, 123456789};
    uint8_t found[2];
    CHECK(zh_index_remove(idx, gone, 2, found, NULL));
    printf("deduplicate removed %zu, remove found [%d %d], %llu vectors left\n", removed, found[0], found[1],
           (unsigned long long)zh_index_count(idx));
    int ok = hits == B && removed == 100 && found[0] == 1 && found[1] == 0 && zh_index_count(idx) == (uint64_t)N - 1;

    /* the 101 removed vectors still occupy device memory: compact, and the neighbours' ids follow the returned old -> new map */
    uint64_t ids2[B * K], keys2[B * K];
    uint32_t counts2[B];
    CHECK(zh_search_batch(idx, q, B, K, ZH_L2SQ, 0, ids, keys, counts));
    uint64_t stored = zh_index_stored_rows(idx);
    uint64_t *new_ids = malloc(sizeof(uint64_t) * stored);
    zh_compact_info ci;
    CHECK(zh_index_compact(idx, new_ids, stored, &ci));
    CHECK(zh_search_batch(idx, q, B, K, ZH_L2SQ, 0, ids2, keys2, counts2));
    int follow = 1;
    for (int b = 0; b < B; b++) {
        follow &= counts2[b] == counts[b];
        for (uint32_t j = 0; j < counts[b] && follow; j++) follow &= ids2[b * K + j] == new_ids[ids[b * K + j]] && keys2[b * K + j] == keys[b * K + j];
    }
    printf("compact: %llu -> %llu stored rows, %llu moved in %.3f ms; neighbours %s the id map\n", (unsigned long long)ci.rows_before,
           (unsigned long long)ci.rows_after, (unsigned long long)ci.rows_moved, ci.ms, follow ? "follow" : "DO NOT follow");
    ok = ok && follow && ci.rows_before == (uint64_t)N + 100 && ci.rows_after == (uint64_t)N - 1 && zh_index_stored_rows(idx) == (uint64_t)N - 1 &&
         new_ids[997] == UINT64_MAX && new_ids[998] == 997;
    free(new_ids);

    /* filtered search: the exact nearest neighbours among the even stored rows only (one bit per stored row, set = allowed) */
    stored = zh_index_stored_rows(idx);
    uint32_t *filter = calloc((stored + 31) / 32, sizeof(uint32_t));
    for (uint64_t r = 0; r < stored; r += 2) filter[r >> 5] |= 1u << (r & 31);
    CHECK(zh_search_exact_filtered_batch(idx, q, B, K, ZH_L2SQ, 0, filter, stored, ids, keys, counts));
    zh_filtered_info fi;
    CHECK(zh_search_filtered_info(idx, &fi));
    int even = fi.rows_allowed == (stored + 1) / 2;
    for (int b = 0; b < B; b++)
        for (uint32_t j = 0; j < counts[b]; j++) even &= ids[b * K + j] % 2 == 0;
    printf("filtered: %llu of %llu rows allowed, path %u; neighbours %s\n", (unsigned long long)fi.rows_allowed,
           (unsigned long long)fi.rows_live, fi.path, even ? "all allowed" : "NOT all allowed");
    ok = ok && even;
    free(filter);

    /* range search, a near-duplicate pass: every live row within L2^2 <= 1.0 of a query, however many there are.  A threshold is a KEY (for L2^2
     * the bits of the f64 distance); a first call with capacity 0 counts, the second one fetches.  Deduplicating a whole table is this loop over
     * batches of its own rows. */
    const double radius = 1.0;
    uint64_t max_keys[B], offsets[B + 1], total = 0;
    for (int b = 0; b < B; b++) memcpy(&max_keys[b], &radius, sizeof radius);
    int rc = zh_search_range_batch(idx, q, B, max_keys, ZH_L2SQ, 0, 0, offsets, NULL, NULL, &total);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "zh_search_range_batch failed (%d): %s\n", rc, zh_last_error()); return 1; }
    uint64_t *near_ids = malloc(sizeof(uint64_t) * (total + 1)), *near_keys = malloc(sizeof(uint64_t) * (total + 1));
    CHECK(zh_search_range_batch(idx, q, B, max_keys, ZH_L2SQ, 0, total, offsets, near_ids, near_keys, &total));
    int near = total >= 1 && total <= (uint64_t)B && offsets[0] == 0 && offsets[B] == total;
    for (uint64_t i = 0; i < total; i++) near &= near_keys[i] <= max_keys[0];
    printf("range: %llu rows within L2^2 <= %.1f of the %d queries; %s\n", (unsigned long long)total, radius, B, near ? "as planted" : "NOT as planted");
    ok = ok && near;
    free(near_ids);
    free(near_keys);

    /* self-join: the near-duplicate pass over the whole table as ONE call -- every pair of live rows (a, b), a < b, within the same radius, each
     * pair once and no row against itself.  One threshold key for the call; capacity 0 counts, the second call fetches. */
    uint64_t join_key, n_pairs = 0;
    memcpy(&join_key, &radius, sizeof radius);
    rc = zh_self_join(idx, join_key, ZH_L2SQ, 0, 0, NULL, NULL, NULL, &n_pairs);
    if (rc != ZH_OK && rc != ZH_ELIMIT) { fprintf(stderr, "zh_self_join failed (%d): %s\n", rc, zh_last_error()); return 1; }
    uint64_t *pa = malloc(sizeof(uint64_t) * (n_pairs + 1)), *pb = malloc(sizeof(uint64_t) * (n_pairs + 1)), *pk = malloc(sizeof(uint64_t) * (n_pairs + 1));
    CHECK(zh_self_join(idx, join_key, ZH_L2SQ, 0, n_pairs, pa, pb, pk, &n_pairs));
    zh_join_info ji;
    CHECK(zh_self_join_info(idx, &ji));
    int joined = ji.pairs == n_pairs;
    for (uint64_t i = 0; i < n_pairs; i++) joined &= pa[i] < pb[i] && pk[i] <= join_key && (i == 0 || pa[i - 1] <= pa[i]);
    printf("self-join: %llu pairs within L2^2 <= %.1f among %llu live rows, path %u; %s\n", (unsigned long long)n_pairs, radius,
           (unsigned long long)ji.rows_live, ji.path, joined ? "ordered and within the radius" : "NOT as specified");
    ok = ok && joined;
    free(pa);
    free(pb);
    free(pk);
    zh_index_destroy(idx);
    free(rows);
    free(q);
    printf(ok ? "example ok\n" : "example FAILED\n");
    return ok ? 0 : 1;
}

/* snapshot_example.c -- save an index to one file and load it back through the C ABI (include/zebra_hip.h).
 *   cc -std=c99 -I include examples/snapshot_example.c -L zebra_amd/lib -lzebra_hip -Wl,-rpath,$PWD/zebra_amd/lib -o snapshot_example
 *   ./snapshot_example /tmp/example.zhs
 * Builds a small index, saves it, inspects the file on the host, loads it as a second index and checks that both answer alike. */
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

int main(int argc, char **argv) {
    const char *path = argc > 1 ? argv[1] : "example.zhs";
    enum { N = 5000, D = 64, B = 4, K = 5 };
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = D;
    opt.max_node_size = 32;
    opt.num_trees = 4;
    zh_index *ix = NULL, *loaded = NULL;
    CHECK(zh_index_create(&opt, &ix));
    CHECK(zh_index_append_synthetic(ix, N, 1, 0, 0));
    CHECK(zh_index_build(ix));

    zh_snapshot_info info;
    CHECK(zh_index_save(ix, path, &info));
    printf("saved %llu rows, %llu bytes in %.1f ms (%.1f ms on the device)\n", (unsigned long long)info.stored_rows,
           (unsigned long long)info.file_bytes, info.ms, info.ms_device);
    CHECK(zh_snapshot_inspect(path, 1, &info)); /* host code only: every section checksum recomputed */
    printf("inspected: version %u, dim %u, %u trees, verified %u\n", info.version, info.dim, info.n_trees, info.verified);
    CHECK(zh_index_load(path, -1, 0, &loaded, &info));

    static float q[B * D];
    CHECK(zh_index_read_rows(ix, 100, B, q)); /* four stored rows as queries */
    uint64_t ids[2][B * K], keys[2][B * K];
    uint32_t counts[2][B];
    CHECK(zh_search_batch(ix, q, B, K, ZH_L2SQ, 0, ids[0], keys[0], counts[0]));
    CHECK(zh_search_batch(loaded, q, B, K, ZH_L2SQ, 0, ids[1], keys[1], counts[1]));
    const int same = !memcmp(ids[0], ids[1], sizeof ids[0]) && !memcmp(keys[0], keys[1], sizeof keys[0]) && !memcmp(counts[0], counts[1], sizeof counts[0]);
    printf("the loaded index answers %s\n", same ? "bit for bit as the saved one" : "DIFFERENTLY");
    zh_index_destroy(loaded);
    zh_index_destroy(ix);
    return same ? 0 : 1;
}

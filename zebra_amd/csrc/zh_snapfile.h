// zh_snapfile.h -- the snapshot FILE: layout, checksum and the host-side reader / writer pieces shared by zh_snapfile.cpp (host
// code only, builds stand-alone), zh_snapshot.hip (the device <-> file pipeline) and zh_api.hip (zh_index_save / zh_index_load).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zebra_hip.h"

#define ZH_SNAP_BLOCK 4096u          // the header block; every section starts on a multiple of it
#define ZH_SNAP_TABLE_OFF 128u       // the section table inside the header block: 32 bytes per section
#define ZH_SNAP_SUM_OFF 4088u        // the header block's own checksum: over its bytes [0, 4088)
#define ZH_SNAP_MAX_SECTIONS 16u
#define ZH_SNAP_MAX_LEVELS 256u      // entries of the LEVELS section (a tree is at most 63 levels deep)
#define ZH_SNAP_MAGIC "ZEBRAHIP"     // 8 bytes, no terminator

enum ZhSnapKind {
    ZH_SEC_ROWS = 1,        // stored_rows x dim f32, row-major: the rows as zh_index_read_rows returns them, removed ones included
    ZH_SEC_REMOVED = 2,     // ceil(stored_rows / 8) bytes: bit r % 8 of byte r / 8 = row r was removed; bits at and past stored_rows zero
    ZH_SEC_NODE_PLANE = 3,  // n_nodes i32   \.
    ZH_SEC_NODE_LEFT = 4,   // n_nodes i32    | the flat forest of zh_forest_view, in the index's own numbering
    ZH_SEC_NODE_RIGHT = 5,  // n_nodes i32    |
    ZH_SEC_ROOTS = 6,       // n_trees u32    |
    ZH_SEC_PLANES = 7,      // n_planes x dim f32
    ZH_SEC_CONSTS = 8,      // n_planes f32   |
    ZH_SEC_LEAF_IDS = 9,    // n_leaf_ids u32 /
    ZH_SEC_LEVELS = 10,     // n_levels u32: [L] = planes of the first L levels of the forest as it was BUILT (what the dense hash may take)
    ZH_SEC_SAMPLES = 11     // n_planes x 2 u32: the two stored rows every plane was made from (UINT32_MAX: the zero vector); only with flags & 1
};

struct ZhSnapSection {
    uint32_t kind;
    uint64_t offset, length, checksum;
};
struct ZhSnapHeader {
    zh_snapshot_info info;  // the header's fields (ms, ms_device, verified: the call's, not the file's)
    uint32_t max_leaf_len;  // the longest leaf (of any node record that is a leaf)
    uint32_t n_levels;
    ZhSnapSection sec[ZH_SNAP_MAX_SECTIONS];
};

#if defined(__HIPCC__)
#define ZH_SNAP_HD __host__ __device__
#else
#define ZH_SNAP_HD
#endif
// one word's term of the section checksum: mix(w + 0x9E3779B97F4A7C15 (i + 1)), mix = the splitmix64 finaliser (a bijection of u64)
static inline ZH_SNAP_HD uint64_t zh_snap_term(uint64_t w, uint64_t i) {
    uint64_t z = w + 0x9E3779B97F4A7C15ull * (i + 1);
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// sum of the terms of the n_bytes at p, whose first word is word `first_word` of its section; a trailing partial word is padded with zero bytes
// (only the last piece of a section may have one)
uint64_t zh_snap_sum(const void *p, uint64_t n_bytes, uint64_t first_word);
// sections (kinds, lengths, offsets), row_bytes and file_bytes from the header's counts; n_levels and max_leaf_len are the caller's
void zh_snap_plan(ZhSnapHeader *h);
// the 4096-byte header block (the sections' checksums must be final)
void zh_snap_encode(const ZhSnapHeader *h, uint8_t *out);
// open + every host-side test of the header block, the section table and the padding (nothing is allocated from the file's numbers); *fd is
// open for reading on ZH_OK, -1 otherwise
int zh_snap_open(const char *path, int *fd, ZhSnapHeader *h);
void zh_snap_close(int fd);
int zh_snap_pread(int fd, void *dst, uint64_t n, uint64_t off);
int zh_snap_pwrite(int fd, const void *src, uint64_t n, uint64_t off, const char *path);
// a whole (small) section into dst (s->length bytes), its checksum recomputed and compared
int zh_snap_read_section(int fd, const ZhSnapSection *s, void *dst);
const ZhSnapSection *zh_snap_find(const ZhSnapHeader *h, uint32_t kind);
// the writer's file: path + ".zhtmp" created (truncated) at its final length, zero-filled; commit = fsync, rename over path, fsync of the
// directory; abort = close and unlink.  tmp: at least strlen(path) + 8 bytes
int zh_snap_create(const char *path, uint64_t file_bytes, char *tmp, int *fd);
int zh_snap_commit(int fd, const char *tmp, const char *path);
void zh_snap_abort(int fd, const char *tmp);

// zh_snapfile.cpp -- the snapshot file of zh_index_save / zh_index_load, host code only: the layout, the checksum, every test
// of a header from an unknown source, and zh_snapshot_inspect.  No HIP in this file, so that it also builds stand-alone with
// g++ -fsanitize=address,undefined (tests/test_snapshot_format.py) -- it parses untrusted on-disk bytes.  Nothing here allocates from a number
// the file states: the header block is 4096 bytes on the stack, sections are summed through a fixed buffer.
//
// Header block (4096 bytes, little endian; this code assumes a little-endian host, as the rest of the library does):
//     0  magic "ZEBRAHIP"          8  u32 version            12  u32 dim               16  u32 max_node_size    20  u32 num_trees_option
//    24  u64 seed                 32  u64 id_base            40  u64 stored_rows       48  u64 live_rows
//    56  u32 n_trees              60  u32 n_nodes            64  u32 n_planes          68  u32 flags            72  u64 n_leaf_ids
//    80  u64 file_bytes           88  u64 row_bytes          96  u32 n_sections       100  u32 max_leaf_len    104  u32 n_levels
//   108  zero up to 128
//   128  n_sections x { u32 kind, u32 zero, u64 offset, u64 length, u64 checksum }, zero up to 4088
//  4088  u64 checksum of bytes [0, 4088) (the section checksum over those 511 words)
// Sections: kinds 1 .. 10 in that order, then 11 when flags & 1; lengths follow from the header's counts; the first starts at 4096, each next one
// at the previous end rounded up to 4096; the file ends with the last section's last byte (file_bytes).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "zh_snapfile.h"

int zh_set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));  // zh_api.hip (stand-alone builds: a stub)

uint64_t zh_snap_sum(const void *p, uint64_t n_bytes, uint64_t first_word) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    const uint64_t nw = n_bytes / 8;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < nw; i++) {
        uint64_t w;
        memcpy(&w, b + 8 * i, 8);
        sum += zh_snap_term(w, first_word + i);
    }
    if (n_bytes & 7) {
        uint64_t w = 0;
        memcpy(&w, b + 8 * nw, n_bytes & 7);
        sum += zh_snap_term(w, first_word + nw);
    }
    return sum;
}

static uint64_t round_up_block(uint64_t v) { return (v + (ZH_SNAP_BLOCK - 1)) & ~(uint64_t)(ZH_SNAP_BLOCK - 1); }

void zh_snap_plan(ZhSnapHeader *h) {
    zh_snapshot_info &f = h->info;
    const uint64_t lens[12] = {0,
                               f.stored_rows * f.dim * 4,
                               (f.stored_rows + 7) / 8,
                               (uint64_t)f.n_nodes * 4,
                               (uint64_t)f.n_nodes * 4,
                               (uint64_t)f.n_nodes * 4,
                               (uint64_t)f.n_trees * 4,
                               (uint64_t)f.n_planes * f.dim * 4,
                               (uint64_t)f.n_planes * 4,
                               f.n_leaf_ids * 4,
                               (uint64_t)h->n_levels * 4,
                               (uint64_t)f.n_planes * 8};
    const uint32_t n = (f.flags & 1u) ? 11 : 10;
    uint64_t off = ZH_SNAP_BLOCK, end = ZH_SNAP_BLOCK;
    for (uint32_t i = 0; i < n; i++) {
        h->sec[i].kind = i + 1;
        h->sec[i].offset = off;
        h->sec[i].length = lens[i + 1];
        end = off + lens[i + 1];
        off = round_up_block(end);
    }
    f.n_sections = n;
    f.row_bytes = lens[1];
    f.file_bytes = end;
}

static void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
static void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
static uint32_t get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

void zh_snap_encode(const ZhSnapHeader *h, uint8_t *o) {
    const zh_snapshot_info &f = h->info;
    memset(o, 0, ZH_SNAP_BLOCK);
    memcpy(o, ZH_SNAP_MAGIC, 8);
    put32(o + 8, f.version); put32(o + 12, f.dim); put32(o + 16, f.max_node_size); put32(o + 20, f.num_trees_option);
    put64(o + 24, f.seed); put64(o + 32, f.id_base); put64(o + 40, f.stored_rows); put64(o + 48, f.live_rows);
    put32(o + 56, f.n_trees); put32(o + 60, f.n_nodes); put32(o + 64, f.n_planes); put32(o + 68, f.flags);
    put64(o + 72, f.n_leaf_ids); put64(o + 80, f.file_bytes); put64(o + 88, f.row_bytes);
    put32(o + 96, f.n_sections); put32(o + 100, h->max_leaf_len); put32(o + 104, h->n_levels);
    for (uint32_t i = 0; i < f.n_sections; i++) {
        uint8_t *e = o + ZH_SNAP_TABLE_OFF + 32 * i;
        put32(e, h->sec[i].kind); put64(e + 8, h->sec[i].offset); put64(e + 16, h->sec[i].length); put64(e + 24, h->sec[i].checksum);
    }
    put64(o + ZH_SNAP_SUM_OFF, zh_snap_sum(o, ZH_SNAP_SUM_OFF, 0));
}

int zh_snap_pread(int fd, void *dst, uint64_t n, uint64_t off) {
    uint8_t *p = static_cast<uint8_t *>(dst);
    while (n) {
        const ssize_t r = pread(fd, p, n > (1u << 30) ? (1u << 30) : (size_t)n, (off_t)off);
        if (r < 0) {
            if (errno == EINTR) continue;
            return zh_set_error(ZH_EIO, "snapshot: read failed: %s", strerror(errno));
        }
        if (r == 0) return zh_set_error(ZH_ECORRUPT, "snapshot: the file ends at byte %llu, inside its stated contents", (unsigned long long)off);
        p += r; off += (uint64_t)r; n -= (uint64_t)r;
    }
    return ZH_OK;
}

int zh_snap_pwrite(int fd, const void *src, uint64_t n, uint64_t off, const char *path) {
    const uint8_t *p = static_cast<const uint8_t *>(src);
    while (n) {
        const ssize_t r = pwrite(fd, p, n > (1u << 30) ? (1u << 30) : (size_t)n, (off_t)off);
        if (r < 0) {
            if (errno == EINTR) continue;
            return zh_set_error(ZH_EIO, "snapshot: write to %s failed: %s", path, strerror(errno));
        }
        if (r == 0) return zh_set_error(ZH_EIO, "snapshot: write to %s made no progress", path);
        p += r; off += (uint64_t)r; n -= (uint64_t)r;
    }
    return ZH_OK;
}

void zh_snap_close(int fd) {
    if (fd >= 0) close(fd);
}

const ZhSnapSection *zh_snap_find(const ZhSnapHeader *h, uint32_t kind) {
    for (uint32_t i = 0; i < h->info.n_sections && i < ZH_SNAP_MAX_SECTIONS; i++)
        if (h->sec[i].kind == kind) return &h->sec[i];
    return nullptr;
}

// the header block's numbers against the format, the ABI's limits and the file's length
static int check_header(const uint8_t *o, uint64_t file_len, ZhSnapHeader *h) {
    if (memcmp(o, ZH_SNAP_MAGIC, 8) != 0) return zh_set_error(ZH_ECORRUPT, "snapshot: not a snapshot file (magic)");
    const uint32_t version = get32(o + 8);
    if (version == 0) return zh_set_error(ZH_ECORRUPT, "snapshot: version 0");
    if (version > ZH_SNAPSHOT_VERSION)
        return zh_set_error(ZH_EUNSUPPORTED, "snapshot: version %u is newer than this library's (%u)", version, ZH_SNAPSHOT_VERSION);
    if (get64(o + ZH_SNAP_SUM_OFF) != zh_snap_sum(o, ZH_SNAP_SUM_OFF, 0)) return zh_set_error(ZH_ECORRUPT, "snapshot: header checksum mismatch");
    memset(h, 0, sizeof *h);
    zh_snapshot_info &f = h->info;
    f.version = version; f.dim = get32(o + 12); f.max_node_size = get32(o + 16); f.num_trees_option = get32(o + 20);
    f.seed = get64(o + 24); f.id_base = get64(o + 32); f.stored_rows = get64(o + 40); f.live_rows = get64(o + 48);
    f.n_trees = get32(o + 56); f.n_nodes = get32(o + 60); f.n_planes = get32(o + 64); f.flags = get32(o + 68);
    f.n_leaf_ids = get64(o + 72);
    const uint64_t file_bytes = get64(o + 80), row_bytes = get64(o + 88);
    const uint32_t n_sections = get32(o + 96);
    h->max_leaf_len = get32(o + 100); h->n_levels = get32(o + 104);
    for (uint32_t i = 108; i < ZH_SNAP_TABLE_OFF; i++)
        if (o[i]) return zh_set_error(ZH_ECORRUPT, "snapshot: reserved header byte %u is not zero", i);
    if (f.dim == 0 || f.dim > ZH_MAX_DIM) return zh_set_error(ZH_ECORRUPT, "snapshot: dim %u outside 1 .. ZH_MAX_DIM", f.dim);
    if (f.num_trees_option > 4096) return zh_set_error(ZH_ECORRUPT, "snapshot: num_trees option %u > 4096", f.num_trees_option);
    if (f.stored_rows > 0xFFFFFFFFull) return zh_set_error(ZH_ECORRUPT, "snapshot: %llu stored rows (more than 2^32-1)", (unsigned long long)f.stored_rows);
    if (f.live_rows > f.stored_rows) return zh_set_error(ZH_ECORRUPT, "snapshot: more live rows than stored rows");
    if (f.n_leaf_ids > 0xFFFFFFFFull) return zh_set_error(ZH_ECORRUPT, "snapshot: %llu leaf entries (more than 2^32-1)", (unsigned long long)f.n_leaf_ids);
    if (f.flags & ~3u) return zh_set_error(ZH_ECORRUPT, "snapshot: unknown flag bits %#x", f.flags);
    if (f.n_trees > f.n_nodes) return zh_set_error(ZH_ECORRUPT, "snapshot: more trees than nodes");
    if (h->n_levels > ZH_SNAP_MAX_LEVELS) return zh_set_error(ZH_ECORRUPT, "snapshot: %u levels", h->n_levels);
    // (stored_rows < 2^32, dim <= 2^20, counts < 2^32: no product below passes 2^55)
    zh_snap_plan(h);
    if (n_sections != f.n_sections) return zh_set_error(ZH_ECORRUPT, "snapshot: %u sections where the flags call for %u", n_sections, f.n_sections);
    if (row_bytes != f.row_bytes) return zh_set_error(ZH_ECORRUPT, "snapshot: row_bytes does not match stored_rows x dim");
    if (file_bytes != f.file_bytes) return zh_set_error(ZH_ECORRUPT, "snapshot: file_bytes does not match the sections");
    if (file_len != f.file_bytes)
        return zh_set_error(ZH_ECORRUPT, "snapshot: the file has %llu bytes, its header states %llu (truncated?)", (unsigned long long)file_len,
                            (unsigned long long)f.file_bytes);
    for (uint32_t i = 0; i < f.n_sections; i++) {
        const uint8_t *e = o + ZH_SNAP_TABLE_OFF + 32 * i;
        if (get32(e) != h->sec[i].kind || get32(e + 4) != 0 || get64(e + 8) != h->sec[i].offset || get64(e + 16) != h->sec[i].length)
            return zh_set_error(ZH_ECORRUPT, "snapshot: section %u is not {kind %u, offset %llu, length %llu}", i, h->sec[i].kind,
                                (unsigned long long)h->sec[i].offset, (unsigned long long)h->sec[i].length);
        h->sec[i].checksum = get64(e + 24);
    }
    for (uint32_t i = ZH_SNAP_TABLE_OFF + 32 * f.n_sections; i < ZH_SNAP_SUM_OFF; i++)
        if (o[i]) return zh_set_error(ZH_ECORRUPT, "snapshot: header padding byte %u is not zero", i);
    return ZH_OK;
}

// the bytes between a section's end and the next section's start
static int check_padding(int fd, const ZhSnapHeader *h) {
    uint8_t pad[ZH_SNAP_BLOCK];
    for (uint32_t i = 0; i + 1 < h->info.n_sections; i++) {
        const uint64_t a = h->sec[i].offset + h->sec[i].length, b = h->sec[i + 1].offset;
        if (b == a) continue;
        int rc = zh_snap_pread(fd, pad, b - a, a);  // (b - a < 4096 by construction)
        if (rc) return rc;
        for (uint64_t j = 0; j < b - a; j++)
            if (pad[j]) return zh_set_error(ZH_ECORRUPT, "snapshot: padding byte at %llu is not zero", (unsigned long long)(a + j));
    }
    return ZH_OK;
}

int zh_snap_open(const char *path, int *out_fd, ZhSnapHeader *h) {
    *out_fd = -1;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return zh_set_error(ZH_EIO, "snapshot: cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        const int e = errno;
        close(fd);
        return zh_set_error(ZH_EIO, "snapshot: cannot stat %s: %s", path, strerror(e));
    }
    if (!S_ISREG(st.st_mode)) {
        close(fd);
        return zh_set_error(ZH_EIO, "snapshot: %s is not a regular file: %s", path, strerror(S_ISDIR(st.st_mode) ? EISDIR : EINVAL));
    }
    const uint64_t file_len = (uint64_t)st.st_size;
    if (file_len < ZH_SNAP_BLOCK) {
        close(fd);
        return zh_set_error(ZH_ECORRUPT, "snapshot: %s has %llu bytes, less than a header block", path, (unsigned long long)file_len);
    }
    uint8_t block[ZH_SNAP_BLOCK];
    int rc = zh_snap_pread(fd, block, ZH_SNAP_BLOCK, 0);
    if (!rc) rc = check_header(block, file_len, h);
    if (!rc) rc = check_padding(fd, h);
    if (rc) { close(fd); return rc; }
    *out_fd = fd;
    return ZH_OK;
}

static int sum_section(int fd, const ZhSnapSection *s, uint64_t *out) {
    static const size_t kBuf = 1u << 16;  // (a multiple of 8: pieces start on word boundaries)
    uint8_t buf[kBuf];
    uint64_t sum = 0;
    for (uint64_t at = 0; at < s->length; at += kBuf) {
        const uint64_t n = s->length - at < kBuf ? s->length - at : kBuf;
        int rc = zh_snap_pread(fd, buf, n, s->offset + at);
        if (rc) return rc;
        sum += zh_snap_sum(buf, n, at / 8);
    }
    *out = sum;
    return ZH_OK;
}

int zh_snap_read_section(int fd, const ZhSnapSection *s, void *dst) {
    int rc = zh_snap_pread(fd, dst, s->length, s->offset);
    if (rc) return rc;
    if (zh_snap_sum(dst, s->length, 0) != s->checksum) return zh_set_error(ZH_ECORRUPT, "snapshot: checksum mismatch in section %u", s->kind);
    return ZH_OK;
}

int zh_snap_create(const char *path, uint64_t file_bytes, char *tmp, int *out_fd) {
    *out_fd = -1;
    sprintf(tmp, "%s.zhtmp", path);
    const int fd = open(tmp, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return zh_set_error(ZH_EIO, "snapshot: cannot create %s: %s", tmp, strerror(errno));
    if (ftruncate(fd, (off_t)file_bytes) != 0) {  // the final length, zero-filled: the padding is never written
        const int e = errno;
        close(fd);
        unlink(tmp);
        return zh_set_error(ZH_EIO, "snapshot: cannot size %s to %llu bytes: %s", tmp, (unsigned long long)file_bytes, strerror(e));
    }
    *out_fd = fd;
    return ZH_OK;
}

void zh_snap_abort(int fd, const char *tmp) {
    if (fd >= 0) close(fd);
    unlink(tmp);
}

int zh_snap_commit(int fd, const char *tmp, const char *path) {
    if (fsync(fd) != 0) {
        const int e = errno;
        zh_snap_abort(fd, tmp);
        return zh_set_error(ZH_EIO, "snapshot: fsync of %s failed: %s", tmp, strerror(e));
    }
    if (close(fd) != 0) {
        const int e = errno;
        unlink(tmp);
        return zh_set_error(ZH_EIO, "snapshot: close of %s failed: %s", tmp, strerror(e));
    }
    if (rename(tmp, path) != 0) {
        const int e = errno;
        unlink(tmp);
        return zh_set_error(ZH_EIO, "snapshot: cannot rename %s to %s: %s", tmp, path, strerror(e));
    }
    // the directory entry as well (best effort: the file itself is already whole under its final name)
    char dir[4096];
    const char *slash = strrchr(path, '/');
    const size_t n = slash ? (size_t)(slash - path) : 0;
    if (n + 2 < sizeof dir) {
        if (slash && n) { memcpy(dir, path, n); dir[n] = 0; }
        else strcpy(dir, slash ? "/" : ".");
        const int dfd = open(dir, O_RDONLY | O_DIRECTORY | O_CLOEXEC);
        if (dfd >= 0) { fsync(dfd); close(dfd); }
    }
    return ZH_OK;
}

extern "C" ZH_API int zh_snapshot_inspect(const char *path, int verify, zh_snapshot_info *info) {
    if (!path || !info) return zh_set_error(ZH_EINVAL, "zh_snapshot_inspect: null argument");
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    memset(info, 0, sizeof *info);
    ZhSnapHeader h;
    int fd;
    int rc = zh_snap_open(path, &fd, &h);
    if (rc) return rc;
    if (verify) {
        for (uint32_t i = 0; i < h.info.n_sections && !rc; i++) {
            uint64_t sum = 0;
            rc = sum_section(fd, &h.sec[i], &sum);
            if (!rc && sum != h.sec[i].checksum) rc = zh_set_error(ZH_ECORRUPT, "snapshot: checksum mismatch in section %u", h.sec[i].kind);
        }
        if (!rc) h.info.verified = 1;
    }
    close(fd);
    if (rc) return rc;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    *info = h.info;
    info->ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
    info->ms_device = 0;
    return ZH_OK;
}

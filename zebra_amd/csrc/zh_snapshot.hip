// zh_snapshot.hip -- the device side of zh_index_save / zh_index_load (zh_api.hip): the checksum kernel and the pipeline that moves the row table
// between device memory and the snapshot file in chunks, through two pinned buffers, without ever holding it whole on the host.
// The file itself -- layout, header tests, host checksum -- is zh_snapfile.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "zh_internal.h"
#include "zh_snapfile.h"

// ---- the section checksum of a piece of device memory ------------------------------------------------------------------------------
// *out += sum over the piece's words w_i of zh_snap_term(w_i, word0 + i) (mod 2^64).  p is 8-byte aligned; the words are read two at a time (16
// bytes per lane, consecutive lanes consecutive pairs: whole cache lines per wave), four pairs in flight per lane; a leading word that is not
// 16-byte aligned, a trailing odd word and the zero-padded tail bytes go to one lane.  Every lane's sum is folded across its wave with shuffles and
// lane 0 adds it to *out with ONE 64-bit atomic: addition mod 2^64 commutes, so neither the order of the waves nor the cut into pieces matters.
typedef unsigned long long zs_u64;
typedef zs_u64 zs_u64x2 __attribute__((ext_vector_type(2)));
#define ZH_SNAP_UNROLL 4

__global__ __launch_bounds__(256) void snap_sum_kernel(const uint8_t *__restrict__ p, uint64_t n_bytes, uint64_t word0, zs_u64 *__restrict__ out) {
    const uint64_t n_words = n_bytes / 8;
    const uint64_t head = ((reinterpret_cast<uintptr_t>(p) & 8u) && n_words) ? 1 : 0;
    const uint64_t n_pairs = (n_words - head) / 2;
    const zs_u64x2 *__restrict__ q = reinterpret_cast<const zs_u64x2 *>(p + 8 * head);
    const uint64_t first = word0 + head;
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    zs_u64 sum = 0;
    for (uint64_t base = tid; base < n_pairs; base += stride * ZH_SNAP_UNROLL) {
        zs_u64x2 v[ZH_SNAP_UNROLL];
#pragma unroll
        for (int u = 0; u < ZH_SNAP_UNROLL; u++) {
            const uint64_t i = base + (uint64_t)u * stride;
            v[u] = i < n_pairs ? __builtin_nontemporal_load(q + i) : zs_u64x2{0, 0};
        }
#pragma unroll
        for (int u = 0; u < ZH_SNAP_UNROLL; u++) {
            const uint64_t i = base + (uint64_t)u * stride;
            if (i < n_pairs) sum += zh_snap_term(v[u].x, first + 2 * i) + zh_snap_term(v[u].y, first + 2 * i + 1);
        }
    }
    if (tid == 0) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(p);
        if (head) sum += zh_snap_term(w[0], word0);
        if ((n_words - head) & 1) sum += zh_snap_term(w[n_words - 1], word0 + n_words - 1);
        if (n_bytes & 7) {
            uint64_t t = 0;
            for (uint32_t j = 0; j < (uint32_t)(n_bytes & 7); j++) t |= (uint64_t)p[8 * n_words + j] << (8 * j);
            sum += zh_snap_term(t, word0 + n_words);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(out, sum);
}

hipError_t zh_launch_snap_sum(const void *dBytes, uint64_t n_bytes, uint64_t word0, uint64_t *dSum, hipStream_t s) {
    if (!n_bytes) return hipSuccess;
    if (reinterpret_cast<uintptr_t>(dBytes) & 7u) return hipErrorInvalidValue;
    const uint64_t pairs = n_bytes / 16 + 1;
    const uint64_t blocks = std::min<uint64_t>((pairs + 256 * ZH_SNAP_UNROLL - 1) / (256 * ZH_SNAP_UNROLL), 4096);
    hipLaunchKernelGGL(snap_sum_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, static_cast<const uint8_t *>(dBytes), n_bytes, word0,
                       reinterpret_cast<zs_u64 *>(dSum));
    return hipGetLastError();
}

// ---- the pipeline --------------------------------------------------------------------------------------------------------------------
uint64_t zh_snap_chunk_bytes() {
    uint64_t chunk = 64ull << 20;
    if (const char *e = getenv("ZH_SNAPSHOT_CHUNK_BYTES")) {
        const long long v = atoll(e);
        if (v >= 8) chunk = std::min<uint64_t>((uint64_t)v & ~7ull, 1ull << 30);
    }
    return chunk;
}

namespace {
struct Pipe {  // two pinned buffers, an event each, the device sum, start / stop events: released whatever way the call ends
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr}, t0 = nullptr, t1 = nullptr;
    uint64_t *dSum = nullptr;
    hipStream_t s = nullptr;
    int init(uint64_t chunk) {
        hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            e = hipHostMalloc(&pin[i], std::max<uint64_t>(chunk, 8), hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventCreate(&t0);
        if (e == hipSuccess) e = hipEventCreate(&t1);
        if (e == hipSuccess) e = hipMalloc((void **)&dSum, 8);
        if (e == hipSuccess) e = hipMemsetAsync(dSum, 0, 8, s);
        if (e != hipSuccess) return zh_set_error(e == hipErrorOutOfMemory ? ZH_ENOMEM : ZH_EHIP, "snapshot: pipeline set-up: %s", hipGetErrorString(e));
        return ZH_OK;
    }
    ~Pipe() {
        if (s) hipStreamSynchronize(s);  // nothing of ours is left reading or writing the pinned buffers
        for (int i = 0; i < 2; i++) {
            if (pin[i]) hipHostFree(pin[i]);
            if (ev[i]) hipEventDestroy(ev[i]);
        }
        if (t0) hipEventDestroy(t0);
        if (t1) hipEventDestroy(t1);
        if (dSum) hipFree(dSum);
        if (s) hipStreamDestroy(s);
    }
};
#define SNAPCHK(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return zh_set_error(ZH_EHIP, "snapshot: %s: %s", #expr, hipGetErrorString(e_));           \
    } while (0)
}  // namespace

// n_bytes of device memory at dSrc -> the file at file_off.  Chunk i is summed on the device and copied to pinned buffer i % 2 behind it; the
// host writes chunk i once its copy has landed, with chunk i + 1 already enqueued.  *out_sum: the section checksum as the device computed it.
int zh_snap_rows_out(int fd, const char *path, uint64_t file_off, const void *dSrc, uint64_t n_bytes, uint64_t *out_sum, double *ms_device) {
    *out_sum = 0;
    *ms_device = 0;
    if (!n_bytes) return ZH_OK;
    const uint64_t chunk = std::min<uint64_t>(zh_snap_chunk_bytes(), (n_bytes + 7) & ~7ull);
    const uint64_t n_chunks = (n_bytes + chunk - 1) / chunk;
    Pipe pp;
    int rc = pp.init(chunk);
    if (rc) return rc;
    const uint8_t *src = static_cast<const uint8_t *>(dSrc);
    auto issue = [&](uint64_t i) -> hipError_t {
        const uint64_t off = i * chunk, n = std::min(chunk, n_bytes - off);
        hipError_t e = zh_launch_snap_sum(src + off, n, off / 8, pp.dSum, pp.s);
        if (e == hipSuccess) e = hipMemcpyAsync(pp.pin[i & 1], src + off, n, hipMemcpyDeviceToHost, pp.s);
        if (e == hipSuccess) e = hipEventRecord(pp.ev[i & 1], pp.s);
        return e;
    };
    SNAPCHK(hipEventRecord(pp.t0, pp.s));
    SNAPCHK(issue(0));
    for (uint64_t i = 0; i < n_chunks; i++) {
        if (i + 1 < n_chunks) SNAPCHK(issue(i + 1));  // (buffer (i + 1) % 2 was written out in the previous turn)
        SNAPCHK(hipEventSynchronize(pp.ev[i & 1]));
        const uint64_t off = i * chunk, n = std::min(chunk, n_bytes - off);
        if ((rc = zh_snap_pwrite(fd, pp.pin[i & 1], n, file_off + off, path))) return rc;
    }
    SNAPCHK(hipEventRecord(pp.t1, pp.s));
    SNAPCHK(hipMemcpyAsync(pp.pin[0], pp.dSum, 8, hipMemcpyDeviceToHost, pp.s));
    SNAPCHK(hipStreamSynchronize(pp.s));
    memcpy(out_sum, pp.pin[0], 8);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pp.t0, pp.t1) == hipSuccess) *ms_device = ms;
    return ZH_OK;
}

// the mirror image: the file's bytes at file_off -> device memory at dDst, read into pinned buffer i % 2 while the copy of chunk i - 1 is in
// flight; the checksum kernel runs on what ARRIVED in device memory.  *out_sum is for the caller to compare: nothing may trust dDst before.
int zh_snap_rows_in(int fd, uint64_t file_off, void *dDst, uint64_t n_bytes, uint64_t *out_sum, double *ms_device) {
    *out_sum = 0;
    *ms_device = 0;
    if (!n_bytes) return ZH_OK;
    const uint64_t chunk = std::min<uint64_t>(zh_snap_chunk_bytes(), (n_bytes + 7) & ~7ull);
    const uint64_t n_chunks = (n_bytes + chunk - 1) / chunk;
    Pipe pp;
    int rc = pp.init(chunk);
    if (rc) return rc;
    uint8_t *dst = static_cast<uint8_t *>(dDst);
    SNAPCHK(hipEventRecord(pp.t0, pp.s));
    for (uint64_t i = 0; i < n_chunks; i++) {
        const uint64_t off = i * chunk, n = std::min(chunk, n_bytes - off);
        if (i >= 2) SNAPCHK(hipEventSynchronize(pp.ev[i & 1]));  // chunk i - 2 has left this buffer
        if ((rc = zh_snap_pread(fd, pp.pin[i & 1], n, file_off + off))) return rc;
        SNAPCHK(hipMemcpyAsync(dst + off, pp.pin[i & 1], n, hipMemcpyHostToDevice, pp.s));
        SNAPCHK(zh_launch_snap_sum(dst + off, n, off / 8, pp.dSum, pp.s));
        SNAPCHK(hipEventRecord(pp.ev[i & 1], pp.s));
    }
    SNAPCHK(hipEventRecord(pp.t1, pp.s));
    SNAPCHK(hipStreamSynchronize(pp.s));
    SNAPCHK(hipMemcpy(out_sum, pp.dSum, 8, hipMemcpyDeviceToHost));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pp.t0, pp.t1) == hipSuccess) *ms_device = ms;
    return ZH_OK;
}

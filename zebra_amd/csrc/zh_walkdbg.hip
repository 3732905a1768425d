// zh_walkdbg.hip -- test / debug read-out of the held-tile walk (zh_debug_walk_pairs, driver in zh_api.hip): the interval of EVERY pair of a
// rectangle of tiles, as the joins' and the graphs' matrix-core scans (path 2) form it, one record per pair.  Not a product path.
//
// The kernel is the cross join's geometry (zh_xjoin.hip) over held_tile, held_walk and the record sink of zh_device.h: the same tile_dot, the same
// crow / cqm travelling one tile ahead through the same two LDS buffers, the same call of approx_interval -- what it reads back is what PoolSink and
// ListSink judge.  The held side may be the column side's own copy (the self-join's, the graphs' view) or another index's (the cross join's).
#include "zh_internal.h"
#include "zh_device.h"

// Block (ab, c): held tiles tileA0 + 4 ab .. + 3 of A's copy (those below TA), chunk c of ZH_JOIN_CHUNK tiles of B's copy, cut at TB; blockIdx.x =
// ab + n_ab c.  Records for the held positions [p0, p1) only, ncol = 16 TB a row of them.
template <int D, int KINDA>
__global__ __launch_bounds__(256) void walk_debug_kernel(const u32x4 *__restrict__ XhA, const float2 *__restrict__ rowMetaA,
                                                         const uint32_t *__restrict__ cidA, const u32x4 *__restrict__ XhB, const float4 *__restrict__ qmB,
                                                         const uint32_t *__restrict__ cidB, uint64_t TA, uint64_t TB, uint64_t tileA0, uint32_t n_ab,
                                                         float Kc, float rhoA, uint64_t p0, uint64_t p1, zh_debug_walk_pair *__restrict__ out, uint64_t cap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ab = blockIdx.x % n_ab, c = blockIdx.x / n_ab;  // (block-uniform)
    const uint64_t I = tileA0 + 4ull * ab + wid;
    const uint64_t Jb = (uint64_t)c * ZH_JOIN_CHUNK, Je = Jb + ZH_JOIN_CHUNK < TB ? Jb + ZH_JOIN_CHUNK : TB;  // (the host launches no chunk with Jb >= TB)
    const bool active = I < TA && I * 16 < p1;  // (wave-uniform)
    f16x8 A[D / 32];
    held_tile<D>(A, XhA, (size_t)I, active, lane);
    RecordSink<KINDA, uint64_t> sink(lane, I, Kc, rhoA, out, cap, p0, p1, TB * 16);
    sink.hold(active, cidA, rowMetaA);
    held_walk<D>(A, active, XhB, cidB, qmB, Jb, Je, sink);
}

// held positions [p0, p1) of A's copy (p0 a multiple of 64, p1 - p0 <= ZH_DEBUG_WALK_ROWS, p1 <= 16 TA) against all of B's; dOut: (p1 - p0) * 16 TB
// records, of which those below `cap` are stored
hipError_t zh_launch_walk_debug(uint32_t d, int metric, int mode, const void *dXhA, const float2 *dRowMetaA, const uint32_t *dCidA, uint64_t n_rows_a,
                                const void *dXhB, const float4 *dQmB, const uint32_t *dCidB, uint64_t n_rows_b, uint64_t p0, uint64_t p1, float Kc, float rhoA,
                                zh_debug_walk_pair *dOut, uint64_t cap, hipStream_t s) {
    const uint64_t TA = (n_rows_a + 15) / 16, TB = (n_rows_b + 15) / 16;
    if (!zh_mfma_dim(d) || (metric != ZH_L2SQ && metric != ZH_L2 && metric != ZH_COSINE)) return hipErrorInvalidValue;
    if (p0 % 64 || p0 >= p1 || p1 > TA * 16 || p1 - p0 > ZH_DEBUG_WALK_ROWS || !TB) return hipErrorInvalidValue;
    const uint64_t tileA0 = p0 / 16, held = (p1 + 15) / 16 - tileA0, chunks = (TB + ZH_JOIN_CHUNK - 1) / ZH_JOIN_CHUNK;
    const uint32_t n_ab = (uint32_t)((held + 3) / 4);
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((walk_debug_kernel<D, K>), dim3((uint32_t)(n_ab * chunks)), dim3(256), 0, s, (const u32x4 *)dXhA, dRowMetaA, dCidA,
                           (const u32x4 *)dXhB, dQmB, dCidB, TA, TB, tileA0, n_ab, Kc, rhoA, p0, p1, dOut, cap);
    });
}

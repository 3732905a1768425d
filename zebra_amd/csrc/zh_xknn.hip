// zh_xknn.hip -- exact k-NN join between TWO indexes (zh_cross_knn, driver in zh_api.hip beside the graph's): for every live stored row a of a slab
// [first_row, first_row + n) of index A its exact top-k by (key, id) over every live row of index B.  The key of (a, b) is the key zh_distance_batch
// gives for STORED row b of B against a QUERY equal to the f32 values of row a of A; that orientation is the definition.  Nothing is excluded: a row
// of B that is bit-identical to row a is an ordinary neighbour.  Output line i belongs to stored row first_row + i of A; ids are B's id_base + row.
// DESIGN.md s30.
//
// The work goes panel by panel as in zh_knn.hip: up to ZH_KNN_PANEL_ROWS live rows of A's slab, ascending by row number.
//   path 1  join_gather_kernel gathers the panel's f32 rows out of A's table, the exact search's path 1 ranks B's live list against them with k,
//           xknn_emit_kernel puts each line at its place.
//   path 2  knn_panel_kernel (zh_knn.hip) gathers the panel's tiles out of A's fp16 copy, join_prep_kernel gives B's positions their qm (with B's
//           rho) and id-or-masked word, and xknn_mfma_kernel is the held-tile walk of zh_device.h with the list sink WITHOUT the self-skip: the
//           held row is A's (A's rowMeta, A's rho), the LDS row is B's.  The row numbers of the two sides are unrelated, so no column is skipped
//           for its number.  Column schedule, prune, survivor keys and final are the exact search's; the survivors' rows are read out of B's f32
//           table, the queries out of the gathered f32 panel of A.  A panel whose list runs over is answered by path 1.
// This file holds what is the call's own: the scan's geometry and the emit.  All scratch is on the LEFT index.
#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

// grid (chunks of `ch` column tiles of [Jt0, Jt1) of B's copy, held blocks of four panel tiles of A).  XhB / qmB / cidB: B's copy and
// join_prep_kernel's view of it; PA / pmeta / pid: knn_panel_kernel's gather out of A's copy (pid: A's row number, all ones past the panel).  Every
// offset into B's copy is 64-bit (held_walk's size_t); the panel's own offsets are below 2^32 by its size.
template <int D, int KINDA>
__global__ __launch_bounds__(256) void xknn_mfma_kernel(const u32x4 *__restrict__ XhB, const float4 *__restrict__ qmB, const uint32_t *__restrict__ cidB,
                                                        uint64_t Jt0, uint64_t Jt1, uint32_t ch, const u32x4 *__restrict__ PA,
                                                        const float2 *__restrict__ pmeta, const uint32_t *__restrict__ pid, uint32_t PT, float Kc, float rhoA,
                                                        const uint32_t *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ lid,
                                                        uint32_t *__restrict__ llo, uint32_t *__restrict__ lhi, uint32_t cap, uint32_t *__restrict__ over) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t I = blockIdx.y * 4 + wid;  // the wave's panel tile
    const uint64_t Jb = Jt0 + (uint64_t)blockIdx.x * ch, Je = Jb + ch < Jt1 ? Jb + ch : Jt1;
    const bool active = I < PT;  // (wave-uniform: the panel's last block may hold fewer than four tiles)
    f16x8 A[D / 32];
    held_tile<D>(A, PA, (size_t)I, active, lane);
    ListSink<KINDA, false> sink{lane, Kc, rhoA, cnt, lid, llo, lhi, cap, cap, over};
    sink.hold(active, I * 16, pid, pmeta, tau);
    held_walk<D>(A, active, XhB, cidB, qmB, Jb, Je, sink);
}

hipError_t zh_launch_xknn_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, const float4 *dQmB, const uint32_t *dCidB, uint64_t p_begin, uint64_t p_end,
                               const void *dA, const float2 *dPMeta, const uint32_t *dPid, hipStream_t s) {
    if (p_begin >= p_end || !e.B) return hipSuccess;
    if (p_begin % 16 || e.B > ZH_KNN_PANEL_ROWS) return hipErrorInvalidValue;
    const uint64_t Jt0 = p_begin / 16, Jt1 = (p_end + 15) / 16;
    const uint32_t PT = (e.B + 15) / 16, n_ab = (PT + 3) / 4, ch = zh_knn_chunk(Jt1 - Jt0, n_ab);
    const dim3 grid((uint32_t)((Jt1 - Jt0 + ch - 1) / ch), n_ab);
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((xknn_mfma_kernel<D, K>), grid, dim3(256), 0, s, (const u32x4 *)e.Xh, dQmB, dCidB, Jt0, Jt1, ch, (const u32x4 *)dA, dPMeta, dPid, PT,
                           e.Kc, e.rho, e.tau, e.cnt, e.lid, e.llo, e.lhi, e.cap, e.over);
    });
}

// A panel's answer to its lines' places: a wave per line b.  in_*: [B][k] as final_kernel (or the exact search's path 1) wrote them -- ids = B's
// id_base + row, ascending by (key, id), counts[b] entries; the line of A's row rows[b] gets them as they are, UINT64_MAX past the count.
__global__ __launch_bounds__(256) void xknn_emit_kernel(const uint64_t *__restrict__ in_ids, const uint64_t *__restrict__ in_keys,
                                                        const uint32_t *__restrict__ in_counts, const uint32_t *__restrict__ rows, uint32_t B,
                                                        uint64_t first_row, uint32_t k, uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys,
                                                        uint32_t *__restrict__ out_counts) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;  // (wave-uniform)
    const uint64_t line = rows[b] - first_row;
    const uint32_t take = in_counts[b] < k ? in_counts[b] : k;
    const size_t i = (size_t)b * k, o = (size_t)line * k;
    for (uint32_t j = lane; j < k; j += 64) {
        out_ids[o + j] = j < take ? in_ids[i + j] : ~0ull;
        out_keys[o + j] = j < take ? in_keys[i + j] : ~0ull;
    }
    if (lane == 0) out_counts[line] = take;
}

hipError_t zh_launch_xknn_emit(const uint64_t *dInIds, const uint64_t *dInKeys, const uint32_t *dInCounts, const uint32_t *dRows, uint32_t B,
                               uint64_t first_row, uint32_t k, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(xknn_emit_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dInIds, dInKeys, dInCounts, dRows, B, first_row, k, dOutIds, dOutKeys, dOutCounts);
    return hipGetLastError();
}

// zh_xjoin.hip -- exact join between TWO indexes (zh_cross_join, driver in zh_api.hip beside the self-join's): every pair (live row a of index A,
// live row b of index B) whose key is <= ONE threshold key.  The key of a pair is the key zh_distance_batch gives for STORED row b of B against a
// QUERY equal to the f32 values of row a of A; that orientation is the definition, and every key below is computed in it.  The answer is three
// parallel arrays ascending by (a, key, b), out_a = A's id_base + row, out_b = B's id_base + row.  DESIGN.md s20.
//
// A hit is (a, b, key), pooled as in the self-join and by its kernels (zh_join.hip): v = a << 32 | b and the key, two u64 arrays on the LEFT index,
// counted in *ctr whether or not the pool still has room.  This file holds what is the cross join's own: the scan of path 2 and its geometry.
//   path 1  a panel of up to 1024 live rows of A is gathered device-to-device into a query buffer (zh_launch_join_gather over A's table),
//           exact_score_kernel (zh_exact.hip) keys B's live-row chunks against it, pair_collect_kernel takes every key <= max_key: the full
//           rectangle, no `row > a` condition.
//   path 2  xjoin_mfma_kernel: the A operand of v_mfma_f32_16x16x32_f16 is a tile of A's fp16 row copy, the B operand a tile of B's (both copies
//           hold a tile in the same per-lane order: lane l holds line l % 16, k-chunk l / 16), so a 16 x 16 block of A B^T needs no conversion.
//           The held-tile walk of zh_device.h with the pool sink over the full rectangle: four consecutive A tiles held, B's
//           tiles through LDS, so a tile of B crosses L2 -> CU once per 64 held rows.  approx_interval (unchanged) gives the
//           pair's interval: the held A row is its "stored row" x (A's rowMeta, A's rho), the LDS row of B its "query" q, whose qm comes from
//           zh_launch_join_prep over B's rowMeta with B's rho.  The interval does not care which side the canonical key calls "stored" (s20).
//           Pairs with lo <= tau go to a candidate pool as a_row << 32 | b_row; pair_survivors_kernel gives every candidate the canonical key of
//           (stored row b of B's f32 table, query = row a of A's f32 table), judges key <= max_key, counts and compacts.
// Then, while the capacity holds, the pool is ordered by (a, key, b) with three stable LSD radix sorts (the b bits, the key, the a bits) and
// pair_emit_kernel writes the three arrays with the two id bases.
#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

// ---- path 2.  Block (ab, c) of a panel that starts at tile tileA0 of A's copy: held tiles tileA0 + 4 ab .. + 3 (those below TA), chunk c of
// ZH_JOIN_CHUNK tiles of B's copy, cut at TB.  blockIdx.x = ab + n_ab c: ab is the FAST index, so that the blocks resident together walk the
// same chunk of B (1.5 MiB at d = 768) and find it in L2 -- reasoned from the dispatch order, not measured (s20).  The whole rectangle is computed:
// no diagonal.  cidA / cidB: join_prep_kernel's id-or-masked word per position of either copy (the row number through that index's own perm, all
// ones for a removed row and for the tail of the last tile).  Every offset into either copy is 64-bit: both tables may pass 2^32 elements. ----
template <int D, int KINDA>
__global__ __launch_bounds__(256) void xjoin_mfma_kernel(const u32x4 *__restrict__ XhA, const float2 *__restrict__ rowMetaA,
                                                         const uint32_t *__restrict__ cidA, const u32x4 *__restrict__ XhB, const float4 *__restrict__ qmB,
                                                         const uint32_t *__restrict__ cidB, uint64_t TA, uint64_t TB, uint64_t tileA0, uint32_t n_ab,
                                                         float Kc, float rhoA, const uint32_t *__restrict__ tau, uint64_t *__restrict__ cand, uint64_t cap,
                                                         unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t ab = blockIdx.x % n_ab, c = blockIdx.x / n_ab;  // (block-uniform)
    const uint64_t I = tileA0 + 4ull * ab + wid;
    const uint64_t Jb = (uint64_t)c * ZH_JOIN_CHUNK, Je = Jb + ZH_JOIN_CHUNK < TB ? Jb + ZH_JOIN_CHUNK : TB;  // (the host launches no chunk with Jb >= TB)
    const bool active = I < TA;  // (wave-uniform: A's last block may hold fewer than four tiles)
    f16x8 A[D / 32];
    held_tile<D>(A, XhA, (size_t)I, active, lane);
    PoolSink<KINDA, false, uint64_t> sink{lane, I, tau[0], Kc, rhoA, cand, cap, ctr};
    sink.hold(active, cidA, rowMetaA);
    held_walk<D>(A, active, XhB, cidB, qmB, Jb, Je, sink);
}

// The launch geometry of a panel of held tiles [tileA0, min(tileA1, TA)) against all TB tiles of B: *n_ab held blocks of four tiles, each walking
// every chunk of B.  Returns the tile products the panel issues -- the `tiles` of zh_cross_info, from the geometry alone (T_A x T_B over the panels).
uint64_t zh_xjoin_geometry(uint64_t TA, uint64_t TB, uint64_t tileA0, uint64_t tileA1, uint32_t *n_ab, uint32_t *blocks) {
    const uint64_t held = std::min(tileA1, TA) - tileA0, chunks = (TB + ZH_JOIN_CHUNK - 1) / ZH_JOIN_CHUNK;
    *n_ab = (uint32_t)((held + 3) / 4);
    *blocks = (uint32_t)(*n_ab * chunks);
    return held * TB;
}

hipError_t zh_launch_xjoin_mfma(uint32_t d, int metric, int mode, const void *dXhA, const float2 *dRowMetaA, const uint32_t *dCidA, uint64_t n_rows_a,
                                const void *dXhB, const float4 *dQmB, const uint32_t *dCidB, uint64_t n_rows_b, uint64_t tileA0, uint64_t tileA1, float Kc,
                                float rhoA, const uint32_t *dTau, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s) {
    const uint64_t TA = (n_rows_a + 15) / 16, TB = (n_rows_b + 15) / 16;
    if (!TB || tileA0 >= tileA1) return hipSuccess;
    if (tileA0 % 4 || tileA0 >= TA || (tileA1 % 4 && tileA1 < TA) || (tileA1 - tileA0) * 16 > ZH_JOIN_PANEL_ROWS) return hipErrorInvalidValue;
    uint32_t n_ab = 0, blocks = 0;
    zh_xjoin_geometry(TA, TB, tileA0, tileA1, &n_ab, &blocks);
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((xjoin_mfma_kernel<D, K>), dim3(blocks), dim3(256), 0, s, (const u32x4 *)dXhA, dRowMetaA, dCidA, (const u32x4 *)dXhB, dQmB, dCidB, TA,
                           TB, tileA0, n_ab, Kc, rhoA, dTau, dCand, cand_cap, dCandCtr);
    });
}

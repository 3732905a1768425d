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
//           hold a tile in the same per-lane order: lane l holds line l % 16, k-chunk l / 16), so a 16 x 16 block of A B^T needs no conversion.  A
//           wave holds its 16-row tile of A in registers; the four waves of a block hold four consecutive A tiles and share every tile of B's
//           copy through LDS exactly as join_mfma_kernel does (two buffers of 32 d bytes: 64 KiB at d = 1024; lane l reads the 16 bytes at 16 l
//           of a 1-KiB step: no bank conflict, no padding), so a tile of B crosses L2 -> CU once per 64 held rows.  The sum is
//           (acc0 + acc1) + (acc2 + acc3): zh_approx_bound(metric, d, 1) stays the accumulation bound.  approx_interval (unchanged) gives the
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
    constexpr int NS = D / 32;        // MFMA steps of a tile (K = 32 each) = its KiB
    constexpr int PIECES = NS * 64;   // 16-byte pieces of a tile
    constexpr int PT = PIECES / 256;  // ... per thread of the block
    __shared__ u32x4 sB[2][PIECES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, h = lane >> 4;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t ab = blockIdx.x % n_ab, c = blockIdx.x / n_ab;  // (block-uniform)
    const uint64_t I = tileA0 + 4ull * ab + wid;
    const uint64_t Jb = (uint64_t)c * ZH_JOIN_CHUNK, Je = Jb + ZH_JOIN_CHUNK < TB ? Jb + ZH_JOIN_CHUNK : TB;  // (the host launches no chunk with Jb >= TB)
    const bool active = I < TA;  // (wave-uniform; an idle wave of A's last block still moves tiles and meets the barriers)
    f16x8 A[NS];
    uint32_t id[4];
    float2 meta[4];
    if (active) {
        const u32x4 *tp = XhA + (size_t)I * PIECES + lane;
#pragma unroll
        for (int st = 0; st < NS; st++) A[st] = __builtin_bit_cast(f16x8, tp[64 * st]);
        // this lane's outputs: rows 4 h + i of the held tile (register i), column c16 = row c16 of B's tile J
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t p = I * 16 + 4 * h + i;
            id[i] = cidA[p];
            meta[i] = id[i] != 0xFFFFFFFFu ? rowMetaA[p] : make_float2(0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int st = 0; st < NS; st++) A[st] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) { id[i] = 0xFFFFFFFFu; meta[i] = make_float2(0.f, 0.f); }
    }
    const uint32_t tq = tau[0];
    {
        const u32x4 *src = XhB + (size_t)Jb * PIECES + tid;
#pragma unroll
        for (int k = 0; k < PT; k++) sB[0][k * 256 + tid] = src[k * 256];
    }
    // the column rows' id-or-masked word and qm travel one tile ahead, like the tile itself: nothing of tile J is fetched in its compute phase
    uint32_t cb_next = cidB[Jb * 16 + c16];
    float4 qb_next = qmB[Jb * 16 + c16];
    __syncthreads();
    for (uint64_t J = Jb; J < Je; J++) {
        const uint32_t cur = (uint32_t)(J - Jb) & 1u;
        const bool more = J + 1 < Je;  // (block-uniform)
        const uint32_t cb = cb_next;
        const float4 qb = qb_next;
        u32x4 pf[PT];
        if (more) {
            const u32x4 *src = XhB + (size_t)(J + 1) * PIECES + tid;
#pragma unroll
            for (int k = 0; k < PT; k++) pf[k] = src[k * 256];
            cb_next = cidB[(J + 1) * 16 + c16];
            qb_next = qmB[(J + 1) * 16 + c16];
        }
        if (active) {  // (wave-uniform)
            const u32x4 *bp = &sB[cur][lane];
            f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int st = 0; st < NS; st++)
                acc[st & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[st], __builtin_bit_cast(f16x8, bp[64 * st]), acc[st & 3], 0, 0, 0);
            const f32x4 t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bool pass = false;
                if (id[i] != 0xFFFFFFFFu && cb != 0xFFFFFFFFu)
                    pass = (uint32_t)approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qb, Kc, rhoA, 0.f) <= tq;
                const uint64_t m = __ballot(pass);
                if (m) {  // (wave-uniform)
                    const unsigned long long slot = wave_slots(ctr, m, lane);
                    if (pass && slot < cap) cand[slot] = ((uint64_t)id[i] << 32) | cb;
                }
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < PT; k++) sB[cur ^ 1][k * 256 + tid] = pf[k];
        }
        __syncthreads();  // buffer cur ^ 1 was last read in the step before, which every wave left through this barrier
    }
}

template <int KINDA>
static hipError_t launch_xjoin_mfma_kinda(uint32_t d, const void *XhA, const float2 *rowMetaA, const uint32_t *cidA, const void *XhB, const float4 *qmB,
                                          const uint32_t *cidB, uint64_t TA, uint64_t TB, uint64_t tileA0, uint32_t n_ab, uint32_t blocks, float Kc,
                                          float rhoA, const uint32_t *dTau, uint64_t *dCand, uint64_t cap, unsigned long long *dCtr, hipStream_t s) {
#define ZH_XJ_CASE(DD)                                                                                                                                    \
    case DD:                                                                                                                                               \
        hipLaunchKernelGGL((xjoin_mfma_kernel<DD, KINDA>), dim3(blocks), dim3(256), 0, s, (const u32x4 *)XhA, rowMetaA, cidA, (const u32x4 *)XhB, qmB, cidB, TA, \
                           TB, tileA0, n_ab, Kc, rhoA, dTau, dCand, cap, dCtr);                                                                            \
        break
    switch (d) {
        ZH_XJ_CASE(256);
        ZH_XJ_CASE(384);
        ZH_XJ_CASE(512);
        ZH_XJ_CASE(768);
        ZH_XJ_CASE(1024);
    default: return hipErrorInvalidValue;
    }
#undef ZH_XJ_CASE
    return hipGetLastError();
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
    if (metric != ZH_COSINE)
        return launch_xjoin_mfma_kinda<0>(d, dXhA, dRowMetaA, dCidA, dXhB, dQmB, dCidB, TA, TB, tileA0, n_ab, blocks, Kc, rhoA, dTau, dCand, cand_cap, dCandCtr, s);
    if (mode == ZH_COSINE_PARITY)
        return launch_xjoin_mfma_kinda<2>(d, dXhA, dRowMetaA, dCidA, dXhB, dQmB, dCidB, TA, TB, tileA0, n_ab, blocks, Kc, rhoA, dTau, dCand, cand_cap, dCandCtr, s);
    return launch_xjoin_mfma_kinda<1>(d, dXhA, dRowMetaA, dCidA, dXhB, dQmB, dCidB, TA, TB, tileA0, n_ab, blocks, Kc, rhoA, dTau, dCand, cand_cap, dCandCtr, s);
}

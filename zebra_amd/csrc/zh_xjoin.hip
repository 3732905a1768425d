// zh_xjoin.hip -- exact join between TWO indexes (zh_cross_join, driver in zh_api.hip beside the self-join's): every pair (live row a of index A,
// live row b of index B) whose key is <= ONE threshold key.  The key of a pair is the key zh_distance_batch gives for STORED row b of B against a
// QUERY equal to the f32 values of row a of A; that orientation is the definition, and every key below is computed in it.  The answer is three
// parallel arrays ascending by (a, key, b), out_a = A's id_base + row, out_b = B's id_base + row.  DESIGN.md s20.
//
// A hit is (a, b, key), pooled as in the self-join (zh_join.hip): v = a << 32 | b and the key, two u64 arrays on the LEFT index, counted in *ctr
// whether or not the pool still has room.  A pool slot is taken with one atomic per WAVE (join_wave_slots's pattern, restated: zh_join.hip is left
// alone).
//   path 1  a panel of up to 1024 live rows of A is gathered device-to-device into a query buffer (zh_launch_join_gather over A's table),
//           exact_score_kernel (zh_exact.hip) keys B's live-row chunks against it, xjoin_collect_kernel takes every key <= max_key: the full
//           rectangle, no `row > a` condition.
//   path 2  xjoin_mfma_kernel: the A operand of v_mfma_f32_16x16x32_f16 is a tile of A's fp16 row copy, the B operand a tile of B's (both copies
//           hold a tile in the same per-lane order: lane l holds line l % 16, k-chunk l / 16), so a 16 x 16 block of A B^T needs no conversion.  A
//           wave holds its 16-row tile of A in registers; the four waves of a block hold four consecutive A tiles and share every tile of B's
//           copy through LDS exactly as join_mfma_kernel does (two buffers of 32 d bytes: 64 KiB at d = 1024; lane l reads the 16 bytes at 16 l
//           of a 1-KiB step: no bank conflict, no padding), so a tile of B crosses L2 -> CU once per 64 held rows.  The sum is
//           (acc0 + acc1) + (acc2 + acc3): zh_approx_bound(metric, d, 1) stays the accumulation bound.  approx_interval (unchanged) gives the
//           pair's interval: the held A row is its "stored row" x (A's rowMeta, A's rho), the LDS row of B its "query" q, whose qm comes from
//           zh_launch_join_prep over B's rowMeta with B's rho.  The interval does not care which side the canonical key calls "stored" (s20).
//           Pairs with lo <= tau go to a candidate pool as a_row << 32 | b_row; xjoin_survivors_kernel gives every candidate the canonical key of
//           (stored row b of B's f32 table, query = row a of A's f32 table), judges key <= max_key, counts and compacts.
// Then, while the capacity holds, the pool is ordered by (a, key, b) with three stable LSD radix sorts (the b bits, the key, the a bits) and
// xjoin_emit_kernel writes the three arrays with the two id bases.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

typedef _Float16 f16x8x __attribute__((ext_vector_type(8)));
typedef float f32x4x __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4x __attribute__((ext_vector_type(4)));

// the lanes of `m` (a ballot) get consecutive pool slots: one atomic for the wave, taken by lane 0 (every lane of the wave is active at the call);
// the counter runs on past the pool
__device__ __forceinline__ unsigned long long xjoin_wave_slots(unsigned long long *__restrict__ ctr, uint64_t m, uint32_t lane) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
    return (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// ---- path 1: the hits of a keyed chunk of B's live rows: every key <= max_key.  grid (ceil(nr / 256), B) ----
__global__ __launch_bounds__(256) void xjoin_collect_kernel(const uint64_t *__restrict__ keys, uint64_t ld, const uint32_t *__restrict__ liveB, uint64_t p0,
                                                            uint32_t nr, const uint32_t *__restrict__ qrows, uint64_t max_key,
                                                            unsigned long long *__restrict__ ctr, uint64_t *__restrict__ pv, uint64_t *__restrict__ pk,
                                                            uint64_t cap) {
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t rl = blockIdx.x * 256 + threadIdx.x;
    const uint32_t a = qrows[b];
    uint64_t key = 0;
    uint32_t row = 0;
    bool hit = false;
    if (rl < nr) {
        row = liveB[p0 + rl];
        key = keys[(size_t)b * ld + rl];
        hit = key <= max_key;
    }
    const uint64_t m = __ballot(hit);
    if (!m) return;  // (wave-uniform)
    const unsigned long long slot = xjoin_wave_slots(ctr, m, lane);  // always: the count stays exact when the pool is full
    if (hit && slot < cap) {
        pv[slot] = ((uint64_t)a << 32) | row;
        pk[slot] = key;
    }
}

hipError_t zh_launch_xjoin_collect(const uint64_t *dKeys, uint64_t ld, const uint32_t *dLiveB, uint64_t p0, uint32_t nr, const uint32_t *dQRows, uint32_t B,
                                   uint64_t max_key, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s) {
    if (!nr || !B) return hipSuccess;
    hipLaunchKernelGGL(xjoin_collect_kernel, dim3((nr + 255) / 256, B), dim3(256), 0, s, dKeys, ld, dLiveB, p0, nr, dQRows, max_key, dHitCtr, dPoolV, dPoolK,
                       pool_cap);
    return hipGetLastError();
}

// ---- path 2.  Block (ab, c) of a panel that starts at tile tileA0 of A's copy: held tiles tileA0 + 4 ab .. + 3 (those below TA), chunk c of
// ZH_JOIN_CHUNK tiles of B's copy, cut at TB.  blockIdx.x = ab + n_ab c: ab is the FAST index, so that the blocks resident together walk the
// same chunk of B (1.5 MiB at d = 768) and find it in L2 -- reasoned from the dispatch order, not measured (s20).  The whole rectangle is computed:
// no diagonal.  cidA / cidB: join_prep_kernel's id-or-masked word per position of either copy (the row number through that index's own perm, all
// ones for a removed row and for the tail of the last tile).  Every offset into either copy is 64-bit: both tables may pass 2^32 elements. ----
template <int D, int KINDA>
__global__ __launch_bounds__(256) void xjoin_mfma_kernel(const u32x4x *__restrict__ XhA, const float2 *__restrict__ rowMetaA,
                                                         const uint32_t *__restrict__ cidA, const u32x4x *__restrict__ XhB, const float4 *__restrict__ qmB,
                                                         const uint32_t *__restrict__ cidB, uint64_t TA, uint64_t TB, uint64_t tileA0, uint32_t n_ab,
                                                         float Kc, float rhoA, const uint32_t *__restrict__ tau, uint64_t *__restrict__ cand, uint64_t cap,
                                                         unsigned long long *__restrict__ ctr) {
    constexpr int NS = D / 32;        // MFMA steps of a tile (K = 32 each) = its KiB
    constexpr int PIECES = NS * 64;   // 16-byte pieces of a tile
    constexpr int PT = PIECES / 256;  // ... per thread of the block
    __shared__ u32x4x sB[2][PIECES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, h = lane >> 4;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t ab = blockIdx.x % n_ab, c = blockIdx.x / n_ab;  // (block-uniform)
    const uint64_t I = tileA0 + 4ull * ab + wid;
    const uint64_t Jb = (uint64_t)c * ZH_JOIN_CHUNK, Je = Jb + ZH_JOIN_CHUNK < TB ? Jb + ZH_JOIN_CHUNK : TB;  // (the host launches no chunk with Jb >= TB)
    const bool active = I < TA;  // (wave-uniform; an idle wave of A's last block still moves tiles and meets the barriers)
    f16x8x A[NS];
    uint32_t id[4];
    float2 meta[4];
    if (active) {
        const u32x4x *tp = XhA + (size_t)I * PIECES + lane;
#pragma unroll
        for (int st = 0; st < NS; st++) A[st] = __builtin_bit_cast(f16x8x, tp[64 * st]);
        // this lane's outputs: rows 4 h + i of the held tile (register i), column c16 = row c16 of B's tile J
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t p = I * 16 + 4 * h + i;
            id[i] = cidA[p];
            meta[i] = id[i] != 0xFFFFFFFFu ? rowMetaA[p] : make_float2(0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int st = 0; st < NS; st++) A[st] = f16x8x{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) { id[i] = 0xFFFFFFFFu; meta[i] = make_float2(0.f, 0.f); }
    }
    const uint32_t tq = tau[0];
    {
        const u32x4x *src = XhB + (size_t)Jb * PIECES + tid;
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
        u32x4x pf[PT];
        if (more) {
            const u32x4x *src = XhB + (size_t)(J + 1) * PIECES + tid;
#pragma unroll
            for (int k = 0; k < PT; k++) pf[k] = src[k * 256];
            cb_next = cidB[(J + 1) * 16 + c16];
            qb_next = qmB[(J + 1) * 16 + c16];
        }
        if (active) {  // (wave-uniform)
            const u32x4x *bp = &sB[cur][lane];
            f32x4x acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int st = 0; st < NS; st++)
                acc[st & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[st], __builtin_bit_cast(f16x8x, bp[64 * st]), acc[st & 3], 0, 0, 0);
            const f32x4x t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bool pass = false;
                if (id[i] != 0xFFFFFFFFu && cb != 0xFFFFFFFFu)
                    pass = (uint32_t)approx_interval<KINDA>(t[i] * meta[i].y, meta[i].x, qb, Kc, rhoA, 0.f) <= tq;
                const uint64_t m = __ballot(pass);
                if (m) {  // (wave-uniform)
                    const unsigned long long slot = xjoin_wave_slots(ctr, m, lane);
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
        hipLaunchKernelGGL((xjoin_mfma_kernel<DD, KINDA>), dim3(blocks), dim3(256), 0, s, (const u32x4x *)XhA, rowMetaA, cidA, (const u32x4x *)XhB, qmB, cidB, TA, \
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

// The candidates' canonical keys and their judgement: join_survivors_kernel's scheme over two tables.  A candidate is a << 32 | b: the key is that of
// STORED row b, read from B's f32 table, against the QUERY row a, read from A's; the cosine's query norm is qnorm_kernel's sum (the canonical one) of
// row a.  A wave takes 64 candidates at a time: pair j's sums wait in lane j, so that key_of, the comparison and the pool's atomic run once for all 64.
template <int D, int KIND>
__global__ __launch_bounds__(256) void xjoin_survivors_kernel(const float *__restrict__ XA, const float *__restrict__ XB, int metric, int param,
                                                              const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ candCtr,
                                                              uint64_t cand_cap, uint64_t max_key, unsigned long long *__restrict__ ctr,
                                                              uint64_t *__restrict__ pv, uint64_t *__restrict__ pk, uint64_t cap) {
    constexpr int NV = RowVec<D>::NV;
    const uint64_t n = *candCtr;
    if (n > cand_cap) return;  // (the pool ran over: the panel is answered by path 1)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4;
    for (uint64_t g = wave * 64; g < n; g += n_waves * 64) {
        const uint32_t m = n - g < 64 ? (uint32_t)(n - g) : 64u;
        const uint64_t mine = lane < m ? cand[g + lane] : 0ull;
        const uint32_t my_b = (uint32_t)mine, my_a = (uint32_t)(mine >> 32);
        float m0 = 0.f, m1 = 0.f, mq = 0.f;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)my_b, (int)j), qrow = (uint32_t)__builtin_amdgcn_readlane((int)my_a, (int)j);
            float4 v[NV], q[NV];
            load_row<D>(XB + (size_t)row * D, lane, v);
            load_row<D>(XA + (size_t)qrow * D, lane, q);
            float s0 = 0.f, s1 = 0.f, qq = 0.f;
            row_pair_sums<D, KIND>(v, q, lane, param, s0, s1);
            if (KIND == K_COS) {
                float4 cs = make_float4(0.f, 0.f, 0.f, 0.f), cq = cs;
#pragma unroll
                for (int jj = 0; jj < NV; jj++) {
                    const bool act = (jj < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
                    if (act) { sq4(v[jj], cs); sq4(q[jj], cq); }
                }
                s1 = wave_sum_canonical((cs.x + cs.y) + (cs.z + cs.w));
                qq = wave_sum_canonical((cq.x + cq.y) + (cq.z + cq.w));
            }
            if (lane == j) { m0 = s0; m1 = s1; mq = qq; }
        }
        uint64_t key = 0;
        bool hit = false;
        if (lane < m) {
            key = key_of(metric, param, m0, m1, mq);
            hit = key <= max_key;
        }
        const uint64_t hm = __ballot(hit);
        if (hm) {  // (wave-uniform)
            const unsigned long long slot = xjoin_wave_slots(ctr, hm, lane);
            if (hit && slot < cap) { pv[slot] = mine; pk[slot] = key; }
        }
    }
}

template <int D>
static void launch_xjoin_surv_d(const float *dXA, const float *dXB, int metric, int mode, const uint64_t *dCand, const unsigned long long *dCandCtr,
                                uint64_t cand_cap, uint64_t max_key, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                uint32_t blocks, hipStream_t s) {
    if (metric == ZH_COSINE)
        hipLaunchKernelGGL((xjoin_survivors_kernel<D, K_COS>), dim3(blocks), dim3(256), 0, s, dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, max_key, dHitCtr,
                           dPoolV, dPoolK, pool_cap);
    else
        hipLaunchKernelGGL((xjoin_survivors_kernel<D, K_L2>), dim3(blocks), dim3(256), 0, s, dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, max_key, dHitCtr,
                           dPoolV, dPoolK, pool_cap);
}

hipError_t zh_launch_xjoin_survivors(const float *dXA, const float *dXB, uint32_t d, int metric, int mode, const uint64_t *dCand,
                                     const unsigned long long *dCandCtr, uint64_t cand_cap, uint64_t max_key, unsigned long long *dHitCtr, uint64_t *dPoolV,
                                     uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s) {
    // the candidate count is known on the device only: enough waves for 64 candidates each up to the pool's size, at most 4096 of them
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, (cand_cap + 255) / 256));
#define ZH_XJ_SURV(DD) case DD: launch_xjoin_surv_d<DD>(dXA, dXB, metric, mode, dCand, dCandCtr, cand_cap, max_key, dHitCtr, dPoolV, dPoolK, pool_cap, blocks, s); break
    switch (d) {
        ZH_XJ_SURV(256);
        ZH_XJ_SURV(384);
        ZH_XJ_SURV(512);
        ZH_XJ_SURV(768);
        ZH_XJ_SURV(1024);
    default: return hipErrorInvalidValue;
    }
#undef ZH_XJ_SURV
    return hipGetLastError();
}

// ---- both paths: the order.  Three stable LSD sorts of the pool: by the b bits of v, by the key, by the a bits of v -> (a, key, b); the emit adds
// each side's own id base (join_emit_kernel has one) ----
__global__ __launch_bounds__(256) void xjoin_emit_kernel(const uint64_t *__restrict__ v, const uint64_t *__restrict__ k, uint64_t n, uint64_t id_base_a,
                                                         uint64_t id_base_b, uint64_t *__restrict__ out_a, uint64_t *__restrict__ out_b,
                                                         uint64_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { out_a[i] = id_base_a + (v[i] >> 32); out_b[i] = id_base_b + (v[i] & 0xFFFFFFFFull); keys[i] = k[i]; }
}

static int xjoin_bits(uint64_t values) {  // bits that hold 0 .. values - 1
    int b = 1;
    while (b < 32 && (1ull << b) < values) b++;
    return b;
}

// dTmp == nullptr: *tmp_bytes = what the three sorts of n entries need at most
hipError_t zh_launch_xjoin_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t n_rows_a, uint64_t n_rows_b, void *dTmp, size_t *tmp_bytes,
                                uint64_t id_base_a, uint64_t id_base_b, uint64_t *dOutA, uint64_t *dOutB, uint64_t *dOutKeys, hipStream_t s) {
    hipcub::DoubleBuffer<uint64_t> v(dV[0], dV[1]), k(dK[0], dK[1]);
    const int ra = xjoin_bits(n_rows_a), rb = xjoin_bits(n_rows_b);
    hipError_t e;
    if (!dTmp) {
        size_t a = 0, b = 0, c = 0;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, v, k, n, 0, rb, s)) != hipSuccess) return e;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, v, n, 0, 64, s)) != hipSuccess) return e;
        if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, c, v, k, n, 32, 32 + ra, s)) != hipSuccess) return e;
        *tmp_bytes = std::max<size_t>(std::max(a, b), std::max<size_t>(c, 1));
        return hipSuccess;
    }
    if (!n) return hipSuccess;
    size_t bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, v, k, n, 0, rb, s)) != hipSuccess) return e;
    bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, k, v, n, 0, 64, s)) != hipSuccess) return e;
    bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(dTmp, bytes, v, k, n, 32, 32 + ra, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(xjoin_emit_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const uint64_t *)v.Current(), (const uint64_t *)k.Current(), n,
                       id_base_a, id_base_b, dOutA, dOutB, dOutKeys);
    return hipGetLastError();
}

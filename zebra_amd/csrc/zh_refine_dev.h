// zh_refine_dev.h -- what the graph family's block-per-line kernels share on the device: refine_line_kernel (zh_refine.hip), nnd_line_kernel
// (zh_nnd.hip) and gsearch_kernel (zh_gsearch.hip).  The key of a candidate row against the line's row (refine_key) serves all three; the stage
// that keys a whole candidate list with it (refine_key_list), the u32 sort, the block sum and the compaction of a sorted list to its distinct kept
// rows (refine_compact) serve the two line kernels.  One copy, because NN-descent carries a key from one round to the next and a carried key has to
// be the key a round would compute again, and graph search promises zh_search_exact_batch's keys (s24).  DESIGN.md s25.
#pragma once
#include "zh_internal.h"
#include "zh_device.h"

#ifndef ZH_REFINE_INFLIGHT
#define ZH_REFINE_INFLIGHT 4  // candidate rows a wave has in flight (build-time knob)
#endif

#define RF_NONE 0xFFFFFFFFu

// ascending LDS bitonic sort of n u32 words, n a power of two
__device__ __forceinline__ void block_bitonic_sort_u32(uint32_t *sv, uint32_t n) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t size = 2; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < (n >> 1); i += 256) {
                const uint32_t lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const uint32_t a = sv[lo], b = sv[hi];
                if ((a > b) == asc) { sv[lo] = b; sv[hi] = a; }
            }
        }
    }
    __syncthreads();
}

// the sum of v over the block's 256 threads, for every thread (red: 4 words; the barrier before it also closes what the caller did to LDS)
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t *red) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the key of one candidate row, loaded (D > 0: v, the canonical lane layout) or still in memory (D == 0), against the line's row: exact_key's arithmetic
template <int D, int KIND>
__device__ __forceinline__ uint64_t refine_key(const float4 *v, const float *__restrict__ xrow, const float *__restrict__ q, const float4 *qreg, float qq,
                                               uint32_t d, uint32_t lane, int metric, int param) {
    float s0 = 0.f, s1 = 0.f;
    if constexpr (D > 0) {
        constexpr int NV = RowVec<D>::NV;
        row_pair_sums<D, KIND>(v, qreg, lane, param, s0, s1);
        if (KIND == K_COS) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const bool act = (j < RowVec<D>::NJ) || (lane < (uint32_t)RowVec<D>::REM4);
                if (act) sq4(v[j], c);
            }
            s1 = wave_sum_canonical((c.x + c.y) + (c.z + c.w));
        }
    } else
        lane_sums_generic<KIND>(xrow, q, d, lane, param, s0, s1);
    return key_of(metric, param, s0, s1, qq);
}

// the registers load_row<D> fills with a row (D > 0); one unused register for the generic D = 0, whose rows stay in memory
template <int D>
using RowRegs = float4[D > 0 ? RowVec<(D > 0 ? D : 256)>::NV : 1];

// The keying stage of the two line kernels: the block's four waves key the n candidate rows of `list` (LDS) against the row q (qreg: load_row's
// registers of it, loaded by the caller, D > 0; qq its squared norm, K_COS), lane 0 storing keys[i].  Wave wv takes candidates 4 R t + 4 c + wv,
// c < R = ZH_REFINE_INFLIGHT at a time.  No barrier: the caller closes `keys`.  (gsearch_kernel's step (5) is this loop written out: DESIGN.md s25.)
template <int D, int KIND>
__device__ __forceinline__ void refine_key_list(const float *X, uint32_t d, const uint32_t *list, uint32_t n, const float *q,
                                                const float4 *qreg, float qq, uint32_t lane, uint32_t wv, int metric, int param, uint64_t *keys) {
    if constexpr (D > 0) {
        constexpr int R = ZH_REFINE_INFLIGHT, NV = RowVec<D>::NV;
        for (uint32_t i0 = wv; i0 < n; i0 += 4 * R) {
            float4 v[R][NV];
#pragma unroll
            for (int c = 0; c < R; c++) {
                const uint32_t i = i0 + 4 * c < n ? i0 + 4 * c : i0;  // (a slot past the list loads slot 0's row again: straight-line loads)
                load_row<D>(X + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)list[i]) * D, lane, v[c]);
            }
#pragma unroll
            for (int c = 0; c < R; c++) {
                const uint64_t key = refine_key<D, KIND>(v[c], nullptr, q, qreg, qq, d, lane, metric, param);
                if (lane == 0 && i0 + 4 * c < n) keys[i0 + 4 * c] = key;
            }
        }
    } else {
        for (uint32_t i = wv; i < n; i += 4) {
            const uint64_t key = refine_key<0, KIND>(nullptr, X + (size_t)list[i] * d, q, nullptr, qq, d, lane, metric, param);
            if (lane == 0) keys[i] = key;
        }
    }
}

// The compaction: of the sorted s_id[0 .. np2) (np2 <= CAP, a power of two; RF_NONE last) the first entry of every row number whose slot i has
// keep(i), moved to the front -- a thread counts its stretch of CAP / 256 slots, the stretches' exclusive sums (s_scan: 256 words), then the ranks
// into s_key's words (the keys come later).  -> U, the count; s_id[U .. next_pow2(U)) = RF_NONE and s_key[U .. next_pow2(U)) = all ones, the tail
// the (key, id) sort wants.  The caller's barrier stands before it (the sort's last); the last writes are closed by the caller's next barrier.
template <uint32_t CAP, class Keep>
__device__ __forceinline__ uint32_t refine_compact(uint32_t *s_id, uint64_t *s_key, uint32_t *s_scan, uint32_t np2, Keep keep) {
    constexpr uint32_t PER = CAP / 256;
    const uint32_t tid = threadIdx.x;
    uint32_t *tmp = reinterpret_cast<uint32_t *>(s_key);
    const auto first = [&](uint32_t i) { return i < np2 && s_id[i] != RF_NONE && (i == 0 || s_id[i] != s_id[i - 1]) && keep(i); };
    uint32_t mine = 0;
    for (uint32_t j = 0; j < PER; j++) mine += first(tid * PER + j) ? 1u : 0u;
    s_scan[tid] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t t = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += t;
        __syncthreads();
    }
    const uint32_t U = s_scan[255];
    uint32_t rank = s_scan[tid] - mine;
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t i = tid * PER + j;
        if (first(i)) tmp[rank++] = s_id[i];
    }
    __syncthreads();
    const uint32_t up2 = next_pow2(U);  // (<= np2 <= CAP)
    for (uint32_t i = tid; i < up2; i += 256) s_id[i] = i < U ? tmp[i] : RF_NONE;
    __syncthreads();  // (tmp is read: its words become the keys)
    for (uint32_t i = U + tid; i < up2; i += 256) s_key[i] = ~0ull;
    return U;
}

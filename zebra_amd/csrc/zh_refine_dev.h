// zh_refine_dev.h -- what the line kernels of zh_refine.hip (refine_line_kernel) and zh_nnd.hip (nnd_line_kernel) share on the device: the key of a
// candidate row against the line's row, the u32 LDS sort and the block sum.  One copy, because NN-descent carries a key from one round to the next
// and a carried key has to be the key a round would compute again.
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

// zh_refine.hip -- k-NN graph refinement (zh_knn_graph_refine, driver in zh_api.hip): for every live stored row a of a slab the first k by (key, id) of
//   C(a) = ( N'(a)  union  N'(u) for u in N'(a) ) minus a,
// N'(x) = the set of live stored rows that line x of the caller's graph names.  Keys, orientation, ids, tails and counts as zh_knn.hip (DESIGN.md
// s16): what is approximate is the candidate set, never the arithmetic.  DESIGN.md s21.
//
//   refine_rows_kernel   once per call: the u64 graph -> a table of u32 row numbers [stored rows][in_k], UINT32_MAX for every entry that is past the
//                        line's count, out of range, not live or a repetition inside its line.  What N'(x) is, is settled here and not per expansion.
//   refine_line_kernel   a 256-thread block per live line, nothing per pair leaves the block: (a) N'(a) and every N'(u) out of the table into LDS,
//                        a dropped, ids sorted, adjacent equals compacted -> U distinct rows; (b) the four waves stride over them with the line's
//                        row in registers, ZH_REFINE_INFLIGHT candidate rows in flight per wave, exact_key's arithmetic (zh_approx.hip), keys to LDS;
//                        (c) block_bitonic_sort by (key, id), the first min(k, U) written with id_base, tails and the count; `updates` = written
//                        rows that N'(a) does not hold.  The table may be zh_reverse.hip's union table (N'(x) then the kept reverse
//                        neighbours, in_k + rev_k wide): in_k is then that width, and N'(a) the line's first fwd_k entries.
#include "zh_refine_dev.h"  // refine_key, block_bitonic_sort_u32, block_sum_u32, RF_NONE, ZH_REFINE_INFLIGHT: shared with zh_nnd.hip

// a wave per line, lane j its entry j (in_k <= 64)
__global__ __launch_bounds__(256) void refine_rows_kernel(const uint64_t *__restrict__ in, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ bits, uint64_t id_base, uint64_t n_rows, uint32_t in_k, uint64_t l0,
                                                          uint64_t nl, uint32_t *__restrict__ tab) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl) return;  // (wave-uniform)
    const uint64_t x = l0 + i;
    const uint32_t c = counts[x], take = c < in_k ? c : in_k;
    uint32_t v = RF_NONE;
    if (lane < take) {
        const uint64_t r = in[i * in_k + lane] - id_base;  // (an id below id_base wraps past every row number)
        if (r < n_rows && ((bits[r >> 5] >> (r & 31)) & 1u)) v = (uint32_t)r;
    }
    bool dup = false;
    for (uint32_t j = 0; j + 1 < take; j++) {  // (wave-uniform bound)
        const uint32_t o = (uint32_t)__shfl((int)v, (int)j, 64);
        dup = dup || (j < lane && o == v);
    }
    if (lane < in_k) tab[x * in_k + lane] = dup ? RF_NONE : v;
}

hipError_t zh_launch_refine_rows(const uint64_t *dIn, const uint32_t *dCounts, const uint32_t *dBits, uint64_t id_base, uint64_t n_rows, uint32_t in_k,
                                 uint64_t l0, uint64_t nl, uint32_t *dTab, hipStream_t s) {
    if (!in_k || in_k > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    const uint64_t step = 1ull << 24;  // lines of one launch: 2^30 threads
    for (uint64_t b0 = 0; b0 < nl; b0 += step) {
        const uint64_t m = nl - b0 < step ? nl - b0 : step;
        hipLaunchKernelGGL(refine_rows_kernel, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, s, dIn + b0 * in_k, dCounts, dBits, id_base, n_rows, in_k, l0 + b0, m,
                           dTab);
    }
    return hipGetLastError();
}

template <int D, int KIND, int CAP>
__global__ __launch_bounds__(256) void refine_line_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ tab, uint32_t in_k,
                                                          uint32_t fwd_k, const uint32_t *__restrict__ rows, const float *__restrict__ Q, const float *__restrict__ QQ,
                                                          int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k,
                                                          uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts,
                                                          unsigned long long *__restrict__ ctr) {
    constexpr int R = ZH_REFINE_INFLIGHT;
    __shared__ uint64_t s_key[CAP];
    __shared__ uint32_t s_id[CAP];
    __shared__ uint32_t s_own[ZH_REFINE_MAX_IN_K], s_scan[256], s_red[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t b = blockIdx.x, a = rows[b];
    // ---- (a) the candidates: N'(a), then N'(u) of its every member; in_k + in_k^2 <= CAP (the host's choice of CAP)
    if (tid < in_k) s_own[tid] = tab[(size_t)a * in_k + tid];
    __syncthreads();
    const uint32_t raw = in_k + in_k * in_k, np2 = next_pow2(raw);
    uint32_t mine = 0;
    for (uint32_t e = tid; e < np2; e += 256) {
        uint32_t v = RF_NONE;
        if (e < in_k) v = s_own[e];
        else if (e < raw) {
            const uint32_t u = s_own[(e - in_k) / in_k];
            if (u != RF_NONE) v = tab[(size_t)u * in_k + (e - in_k) % in_k];
        }
        mine += v != RF_NONE ? 1u : 0u;
        s_id[e] = v == a ? RF_NONE : v;
    }
    const uint32_t listed = block_sum_u32(mine, s_red);
    block_bitonic_sort_u32(s_id, np2);
    // the first entry of every row number, compacted to the front: a thread counts its stretch, the stretches' exclusive sums, then the ranks
    constexpr uint32_t PER = CAP / 256;
    uint32_t *tmp = reinterpret_cast<uint32_t *>(s_key);  // (the keys come later)
    mine = 0;
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t i = tid * PER + j;
        if (i < np2 && s_id[i] != RF_NONE && (i == 0 || s_id[i] != s_id[i - 1])) mine++;
    }
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
        if (i < np2 && s_id[i] != RF_NONE && (i == 0 || s_id[i] != s_id[i - 1])) tmp[rank++] = s_id[i];
    }
    __syncthreads();
    const uint32_t up2 = next_pow2(U);  // (<= np2 <= CAP)
    for (uint32_t i = tid; i < up2; i += 256) s_id[i] = i < U ? tmp[i] : RF_NONE;
    __syncthreads();  // (tmp is read: its words become the keys)
    for (uint32_t i = U + tid; i < up2; i += 256) s_key[i] = ~0ull;
    // ---- (b) the keys: wave wv takes candidates 4 R t + 4 c + wv, c < R at a time
    if (U) {  // (block-uniform)
        const float *q = Q + (size_t)b * d;
        const float qq = KIND == K_COS ? QQ[b] : 0.f;
        if constexpr (D > 0) {
            constexpr int NV = RowVec<D>::NV;
            float4 qreg[NV];
            load_row<D>(q, lane, qreg);
            for (uint32_t i0 = wv; i0 < U; i0 += 4 * R) {
                float4 v[R][NV];
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const uint32_t i = i0 + 4 * c < U ? i0 + 4 * c : U - 1;  // (a slot past the list loads the last row again: straight-line loads)
                    load_row<D>(X + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)s_id[i]) * D, lane, v[c]);
                }
#pragma unroll
                for (int c = 0; c < R; c++) {
                    const uint64_t key = refine_key<D, KIND>(v[c], nullptr, q, qreg, qq, d, lane, metric, param);
                    if (lane == 0 && i0 + 4 * c < U) s_key[i0 + 4 * c] = key;
                }
            }
        } else {
            for (uint32_t i = wv; i < U; i += 4) {
                const uint64_t key = refine_key<0, KIND>(nullptr, X + (size_t)s_id[i] * d, q, nullptr, qq, d, lane, metric, param);
                if (lane == 0) s_key[i] = key;
            }
        }
    }
    // ---- (c) rank by (key, id); the slots from U to up2 hold (all ones, UINT32_MAX) and stay last
    block_bitonic_sort<uint32_t>(s_key, s_id, up2);
    const uint32_t have = U < k ? U : k;
    const size_t o = (size_t)(a - first_row) * k;
    mine = 0;
    for (uint32_t i = tid; i < k; i += 256) {
        uint64_t id = ~0ull, key = ~0ull;
        if (i < have) {
            const uint32_t r = s_id[i];
            id = id_base + r; key = s_key[i];
            bool old = false;
            for (uint32_t j = 0; j < fwd_k; j++) old = old || s_own[j] == r;
            mine += old ? 0u : 1u;
        }
        out_ids[o + i] = id; out_keys[o + i] = key;
    }
    const uint32_t updates = block_sum_u32(mine, s_red);
    if (tid == 0) {
        out_counts[a - first_row] = have;
        if (listed) atomicAdd(&ctr[0], (unsigned long long)listed);
        if (U) atomicAdd(&ctr[1], (unsigned long long)U);
        if (updates) atomicAdd(&ctr[2], (unsigned long long)updates);
    }
}

template <int D, int KIND>
static hipError_t launch_lines_d(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, const uint32_t *dRows, uint32_t B, const float *dQ,
                                 const float *dQQ, int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds,
                                 uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (in_k + in_k * in_k <= ZH_REFINE_CAP_SMALL)
        hipLaunchKernelGGL((refine_line_kernel<D, KIND, ZH_REFINE_CAP_SMALL>), dim3(B), dim3(256), 0, s, dX, d, dTab, in_k, fwd_k, dRows, dQ, dQQ, metric, param, id_base,
                           first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr);
    else
        hipLaunchKernelGGL((refine_line_kernel<D, KIND, ZH_REFINE_CAP_LARGE>), dim3(B), dim3(256), 0, s, dX, d, dTab, in_k, fwd_k, dRows, dQ, dQQ, metric, param, id_base,
                           first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr);
    return hipGetLastError();
}

// the dimensions zh_launch_exact_score specialises: 128 / 384 / 768 for every kind, 256 / 512 / 1024 as well for the two simsimd kinds
template <int KIND>
static hipError_t launch_lines_kind(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, const uint32_t *dRows, uint32_t B, const float *dQ,
                                    const float *dQQ, int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds,
                                    uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
#define ZH_RF_CASE(DD) \
    case DD: return launch_lines_d<DD, KIND>(dX, d, dTab, in_k, fwd_k, dRows, B, dQ, dQQ, metric, param, id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr, s)
    if constexpr (KIND == K_L2 || KIND == K_COS) {
        switch (d) {
            ZH_RF_CASE(256);
            ZH_RF_CASE(512);
            ZH_RF_CASE(1024);
        default: break;
        }
    }
    switch (d) {
        ZH_RF_CASE(128);
        ZH_RF_CASE(384);
        ZH_RF_CASE(768);
    default: break;
    }
#undef ZH_RF_CASE
    return launch_lines_d<0, KIND>(dX, d, dTab, in_k, fwd_k, dRows, B, dQ, dQQ, metric, param, id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr, s);
}

hipError_t zh_launch_refine_lines(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, const uint32_t *dRows, uint32_t B, const float *dQ,
                                  const float *dQQ, int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds,
                                  uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!in_k || in_k > ZH_REFINE_MAX_IN_K || in_k + in_k * in_k > ZH_REFINE_CAP_LARGE || fwd_k > in_k || !k) return hipErrorInvalidValue;
#define ZH_RF_KIND(K) \
    case K: return launch_lines_kind<K>(dX, d, dTab, in_k, fwd_k, dRows, B, dQ, dQQ, metric, param, id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr, s)
    switch (zh_kind_of(metric)) {
        ZH_RF_KIND(K_COS);
        ZH_RF_KIND(K_MAX);
        ZH_RF_KIND(K_CANB);
        ZH_RF_KIND(K_BRAY);
        ZH_RF_KIND(K_ABS);
        ZH_RF_KIND(K_P3);
        ZH_RF_KIND(K_P4);
        ZH_RF_KIND(K_HAMM);
        ZH_RF_KIND(K_PP);
    default: return launch_lines_kind<K_L2>(dX, d, dTab, in_k, fwd_k, dRows, B, dQ, dQQ, metric, param, id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr, s);
    }
#undef ZH_RF_KIND
}

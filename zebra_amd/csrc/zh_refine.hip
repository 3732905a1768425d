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
// The compaction of (a) and the keying stage (b) are zh_refine_dev.h's refine_compact and refine_key_list, shared with nnd_line_kernel; which
// instantiation a call gets is zh_dispatch_kind_dim's table (zh_device.h).  DESIGN.md s25.
#include "zh_refine_dev.h"  // refine_key_list, refine_compact, block_bitonic_sort_u32, block_sum_u32, RF_NONE, ZH_REFINE_INFLIGHT

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
    zh_for_line_pieces(nl, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(refine_rows_kernel, dim3(blocks), dim3(256), 0, s, dIn + b0 * in_k, dCounts, dBits, id_base, n_rows, in_k, l0 + b0, m, dTab);
    });
    return hipGetLastError();
}

template <int D, int KIND, int CAP>
__global__ __launch_bounds__(256) void refine_line_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ tab, uint32_t in_k,
                                                          uint32_t fwd_k, const uint32_t *__restrict__ rows, const float *__restrict__ Q, const float *__restrict__ QQ,
                                                          int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k,
                                                          uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts,
                                                          unsigned long long *__restrict__ ctr) {
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
    // the first entry of every row number, compacted to the front
    const uint32_t U = refine_compact<CAP>(s_id, s_key, s_scan, np2, [](uint32_t) { return true; }), up2 = next_pow2(U);
    // ---- (b) the keys: wave wv takes candidates 4 R t + 4 c + wv, c < R at a time
    if (U) {  // (block-uniform)
        const float *q = Q + (size_t)b * d;
        RowRegs<D> qreg;
        if constexpr (D > 0) load_row<D>(q, lane, qreg);
        refine_key_list<D, KIND>(X, d, s_id, U, q, qreg, KIND == K_COS ? QQ[b] : 0.f, lane, wv, metric, param, s_key);
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

hipError_t zh_launch_refine_lines(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, const uint32_t *dRows, uint32_t B, const float *dQ,
                                  const float *dQQ, int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds,
                                  uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!in_k || in_k > ZH_REFINE_MAX_IN_K || in_k + in_k * in_k > ZH_REFINE_CAP_LARGE || fwd_k > in_k || !k) return hipErrorInvalidValue;
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        constexpr int KIND = decltype(kind)::value, D = decltype(dim)::value;
        if (in_k + in_k * in_k <= ZH_REFINE_CAP_SMALL)
            hipLaunchKernelGGL((refine_line_kernel<D, KIND, ZH_REFINE_CAP_SMALL>), dim3(B), dim3(256), 0, s, dX, d, dTab, in_k, fwd_k, dRows, dQ, dQQ, metric, param,
                               id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr);
        else
            hipLaunchKernelGGL((refine_line_kernel<D, KIND, ZH_REFINE_CAP_LARGE>), dim3(B), dim3(256), 0, s, dX, d, dTab, in_k, fwd_k, dRows, dQ, dQQ, metric, param,
                               id_base, first_row, k, dOutIds, dOutKeys, dOutCounts, dCtr);
        return hipGetLastError();
    });
}

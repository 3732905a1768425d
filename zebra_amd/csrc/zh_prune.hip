// zh_prune.hip -- k-NN graph pruning (zh_knn_graph_prune, driver in zh_api.hip): for every live stored row a of a slab, its candidates
//   P(a) = ( N'(a)  union  R'(a) ) minus a
// in (key_a, id) order, kept unless OCCLUDED: a candidate c is dropped if some p kept before it has key_p(c) < key_a(c), unsigned and strict; the
// walk stops at `degree` kept rows, and with `fill` the first dropped candidates make up a line that came short.  N', R' and every key as
// zh_refine.hip and zh_reverse.hip have them: what is pruned is the line, never the arithmetic.  DESIGN.md s29.
//
//   prune_line_kernel   a 256-thread block per live line, nothing per pair leaves the block: (1) wave 0 takes the line of the table (the caller's
//                       graph masked by zh_launch_refine_rows, or zh_launch_reverse_select's union table; at most 64 words, no row twice) and
//                       drops the masked words and a by ballot and popcount; (2) the four waves key the m candidates against a
//                       (refine_key_list), block_bitonic_sort orders them by (key, id); (3) the greedy rounds over a 64-bit alive mask: the
//                       first alive candidate p is kept, its row becomes the query (load_row, its norm from the all-rows table), the candidates
//                       still alive behind it are keyed against p and lose their bit where that key is below their key_a -- at most `degree`
//                       rounds, two barriers each, the masks wave-uniform in every wave; (4) wave 0 writes the line and adds the counters.
// A candidate dropped here in round r may stand BEHIND the row the walk stops at; the definition never looks at it, so (4) counts as occluded
// only what stands before the last kept row when the walk stopped at `degree`.
#include "zh_refine_dev.h"  // refine_key_list, RowRegs, RF_NONE

// the bits below position i
__device__ __forceinline__ unsigned long long prune_below(uint32_t i) { return i >= 64 ? ~0ull : (1ull << i) - 1ull; }

// dCtr[0..5] += candidates, kept, occluded, filled, cut lines, keyed
template <int D, int KIND>
__global__ __launch_bounds__(256) void prune_line_kernel(const float *__restrict__ X, uint32_t d, const uint32_t *__restrict__ tab, uint32_t w,
                                                         const uint32_t *__restrict__ rows, const float *__restrict__ QQ, int metric, int param, uint64_t id_base,
                                                         uint64_t first_row, uint32_t degree, uint32_t fill, uint64_t *__restrict__ out_ids,
                                                         uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ ctr) {
    __shared__ uint64_t s_key[ZH_REFINE_MAX_IN_K], s_pk[ZH_REFINE_MAX_IN_K];
    __shared__ uint32_t s_id[ZH_REFINE_MAX_IN_K], s_list[ZH_REFINE_MAX_IN_K];
    __shared__ uint32_t s_m;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t a = rows[blockIdx.x];
    // ---- (1) P(a): the line's kept words but a, in the line's order
    if (wv == 0) {
        const uint32_t e = lane < w ? tab[(size_t)a * w + lane] : RF_NONE;
        const bool keep = e != RF_NONE && e != a;
        const unsigned long long mk = __ballot(keep);
        if (keep) s_id[__popcll(mk & prune_below(lane))] = e;
        if (lane == 0) s_m = (uint32_t)__popcll(mk);
    }
    __syncthreads();
    const uint32_t m = s_m;
    if (!m) return;  // (block-uniform; the host has written the empty line)
    const uint32_t up2 = next_pow2(m);
    if (tid >= m && tid < up2) { s_id[tid] = RF_NONE; s_key[tid] = ~0ull; }
    __syncthreads();
    // ---- (2) key_a of every candidate, then the order (key_a, id)
    {
        const float *q = X + (size_t)a * d;
        RowRegs<D> qreg;
        if constexpr (D > 0) load_row<D>(q, lane, qreg);
        refine_key_list<D, KIND>(X, d, s_id, m, q, qreg, KIND == K_COS ? QQ[a] : 0.f, lane, wv, metric, param, s_key);
    }
    block_bitonic_sort<uint32_t>(s_key, s_id, up2);  // (its first barrier closes the keys)
    // ---- (3) the greedy rounds; alive, kept and occ are the same in every wave
    unsigned long long alive = prune_below(m), kept = 0, occ = 0;
    uint32_t nk = 0, last = 0, keyed = m;
    while (alive) {
        const uint32_t p = (uint32_t)__ffsll((long long)alive) - 1;
        alive &= alive - 1;
        kept |= 1ull << p;
        last = p;
        if (++nk == degree || !alive) break;
        const uint32_t n = (uint32_t)__popcll(alive);
        if (wv == 0 && ((alive >> lane) & 1ull)) s_list[__popcll(alive & prune_below(lane))] = s_id[lane];
        __syncthreads();
        {
            const uint32_t pr = s_id[p];
            const float *q = X + (size_t)pr * d;
            RowRegs<D> qreg;
            if constexpr (D > 0) load_row<D>(q, lane, qreg);
            refine_key_list<D, KIND>(X, d, s_list, n, q, qreg, KIND == K_COS ? QQ[pr] : 0.f, lane, wv, metric, param, s_pk);
        }
        __syncthreads();
        const bool on = (alive >> lane) & 1ull;
        const unsigned long long lost = __ballot(on && s_pk[__popcll(alive & prune_below(lane))] < s_key[lane]);
        alive &= ~lost;
        occ |= lost;
        keyed += n;
    }
    // ---- (4) the line: what the walk examined, the fill, the counters
    if (wv != 0) return;
    const bool stopped = nk == degree;  // (at `degree`: nothing behind the last kept row was examined)
    if (stopped) occ &= prune_below(last);
    const uint32_t n_occ = (uint32_t)__popcll(occ);
    uint32_t filled = 0;
    unsigned long long line = kept;
    if (fill && nk < degree) {
        filled = degree - nk < n_occ ? degree - nk : n_occ;
        const unsigned long long take = __ballot(((occ >> lane) & 1ull) && (uint32_t)__popcll(occ & prune_below(lane)) < filled);
        line |= take;
    }
    const uint32_t have = nk + filled;
    const size_t o = (size_t)(a - first_row) * degree;
    if ((line >> lane) & 1ull) {
        const uint32_t at = (uint32_t)__popcll(line & prune_below(lane));
        out_ids[o + at] = id_base + s_id[lane];
        out_keys[o + at] = s_key[lane];
    }
    if (lane >= have && lane < degree) { out_ids[o + lane] = ~0ull; out_keys[o + lane] = ~0ull; }
    if (lane == 0) {
        out_counts[a - first_row] = have;
        atomicAdd(&ctr[0], (unsigned long long)m);
        atomicAdd(&ctr[1], (unsigned long long)nk);
        if (n_occ) atomicAdd(&ctr[2], (unsigned long long)n_occ);
        if (filled) atomicAdd(&ctr[3], (unsigned long long)filled);
        if (stopped && last + 1 < m) atomicAdd(&ctr[4], 1ull);
        atomicAdd(&ctr[5], (unsigned long long)keyed);
    }
}

hipError_t zh_launch_prune_lines(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t w, const uint32_t *dRows, uint32_t B, const float *dQQ, int metric,
                                 int param, uint64_t id_base, uint64_t first_row, uint32_t degree, uint32_t fill, uint64_t *dOutIds, uint64_t *dOutKeys,
                                 uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!w || w > ZH_REFINE_MAX_IN_K || !degree || degree > ZH_REFINE_MAX_IN_K || fill > 1) return hipErrorInvalidValue;
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        hipLaunchKernelGGL((prune_line_kernel<decltype(dim)::value, decltype(kind)::value>), dim3(B), dim3(256), 0, s, dX, d, dTab, w, dRows, dQQ, metric, param,
                           id_base, first_row, degree, fill, dOutIds, dOutKeys, dOutCounts, dCtr);
        return hipGetLastError();
    });
}

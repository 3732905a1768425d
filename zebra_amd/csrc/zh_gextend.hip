// zh_gextend.hip -- extending the attached graph over the rows stored since the attach (zh_index_extend_graph, driver in zh_api.hip), and reading the
// attached table back (zh_index_get_graph).  The new rows G .. N-1 go in chunks [lo, hi) of `batch` stored rows; while a chunk is processed the table
// covers [0, lo).  A chunk: (1) every live row a of it is a query of zh_launch_gsearch over the [lo][g_k] table (n_rows = g_rows = lo: a seed naming
// a row >= lo is no seed), and line(a) = the first g_k of its final beam; (2) for every live row r < lo that some line(a) names, with R(r) those a,
// line r becomes the first g_k of L'(r) union R(r) by (key_r(x), x): L'(r) the kept entries of line r that are live now, key_r the key of stored row
// x against a query equal to row r.  A row r that no line names keeps its line word for word.  DESIGN.md s27.
//
//   gext_seeds_kernel    the caller's seed lines of the chunk's LIVE rows, gathered behind one another: the walk's block b is live row b of the chunk
//   gext_lines_kernel    a thread per entry: the walk's ids -> u32 row numbers in lines [lo, hi) of the table, UINT32_MAX past the count
//   (zh_launch_reverse_csr_lines, zh_reverse.hip, transposes the chunk's lines: R(r) = csr[off[r] .. off[r + 1]), in no particular order)
//   gext_touched_kernel  a thread per entry: the entry (a -> r) whose a stands first in R(r) puts r on the list of touched rows, so each r once
//   gext_rerank_kernel   a 256-thread block per touched row r, nothing per candidate leaves the block: L'(r) (wave 0, the liveness test on the old
//                        entries) and R(r) into LDS -- all distinct: a line holds no row twice, the members of R(r) are >= lo, those of L'(r) below
//                        -- the four waves key them against r in registers (refine_key_list), block_bitonic_sort by (key, row), g_k words written
//                        in place.  A block reads no line but its own, so the writes disturb nobody; the next chunk's walk starts after them.
//   gext_read_kernel     zh_index_get_graph: a wave per line, the kept entries compacted to the front as id_base + row, 2^64-1 behind them
#include "zh_refine_dev.h"  // refine_key_list, RowRegs, RF_NONE

#define GX_CAP ZH_REFINE_CAP_SMALL  // candidate slots of a re-ranked line: g_k + batch <= 64 + 1024
static_assert(ZH_REFINE_MAX_IN_K + ZH_GRAPH_EXTEND_MAX_BATCH <= GX_CAP, "a re-ranked line fits the line kernels' small capacity");

__global__ __launch_bounds__(256) void gext_seeds_kernel(const uint64_t *__restrict__ seeds, const uint32_t *__restrict__ rows, uint32_t B, uint64_t g0,
                                                         uint32_t n_seed, uint64_t *__restrict__ out) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * n_seed) return;
    const uint32_t b = t / n_seed;
    out[t] = seeds[((uint64_t)rows[b] - g0) * n_seed + (t - b * n_seed)];
}

__global__ __launch_bounds__(256) void gext_lines_kernel(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ rows,
                                                         uint32_t B, uint32_t g_k, uint64_t id_base, uint32_t *__restrict__ tab) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * g_k) return;
    const uint32_t b = t / g_k, j = t - b * g_k;
    tab[(size_t)rows[b] * g_k + j] = j < counts[b] ? (uint32_t)(ids[t] - id_base) : RF_NONE;
}

// entry t of the lines from lo: ctr[0] = the touched rows
__global__ __launch_bounds__(256) void gext_touched_kernel(const uint32_t *__restrict__ tab, uint32_t g_k, uint64_t lo, uint32_t m, const uint64_t *__restrict__ off,
                                                           const uint32_t *__restrict__ csr, uint32_t *__restrict__ touched, unsigned long long *__restrict__ ctr) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint32_t r = tab[lo * g_k + t];
    if (r == RF_NONE || csr[off[r]] != (uint32_t)(lo + t / g_k)) return;
    touched[atomicAdd(&ctr[0], 1ull)] = r;
}

// ctr[0]: the touched rows (final: gext_touched_kernel is done); ctr[1..3] += rows re-ranked, |R(r)|, chunk rows written
template <int D, int KIND>
__global__ __launch_bounds__(256) void gext_rerank_kernel(const float *__restrict__ X, uint32_t d, uint32_t *__restrict__ tab, uint32_t g_k, uint32_t lo,
                                                          const uint32_t *__restrict__ bits, const float *__restrict__ QQ, const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ csr, const uint32_t *__restrict__ touched, int metric, int param,
                                                          unsigned long long *__restrict__ ctr) {
    __shared__ uint64_t s_key[GX_CAP];
    __shared__ uint32_t s_id[GX_CAP];
    __shared__ uint32_t s_nl;
    if (blockIdx.x >= ctr[0]) return;  // (block-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t r = touched[blockIdx.x];
    uint32_t *line = tab + (size_t)r * g_k;
    const uint64_t o0 = off[r];
    // (|R(r)| <= the chunk's rows <= ZH_GRAPH_EXTEND_MAX_BATCH, a line names r at most once: the bound only keeps a broken table inside the LDS)
    const uint32_t deg = (uint32_t)std::min<uint64_t>(off[(size_t)r + 1] - o0, ZH_GRAPH_EXTEND_MAX_BATCH);
    // ---- L'(r): the kept entries of the line that are live now, in the line's order
    if (wv == 0) {
        const uint32_t e = lane < g_k ? line[lane] : RF_NONE;
        const bool keep = e != RF_NONE && ((bits[e >> 5] >> (e & 31)) & 1u);
        const unsigned long long m = __ballot(keep);
        if (keep) s_id[__popcll(m & ((1ull << lane) - 1ull))] = e;
        if (lane == 0) s_nl = (uint32_t)__popcll(m);
    }
    __syncthreads();
    const uint32_t nl = s_nl, n = nl + deg, up2 = next_pow2(n);
    // ---- R(r) behind it, then the tail the sort wants
    for (uint32_t i = tid; i < deg; i += 256) s_id[nl + i] = csr[o0 + i];
    for (uint32_t i = n + tid; i < up2; i += 256) { s_id[i] = RF_NONE; s_key[i] = ~0ull; }
    __syncthreads();
    // ---- the keys against r: wave wv takes candidates 4 R t + 4 c + wv
    {
        const float *q = X + (size_t)r * d;
        RowRegs<D> qreg;
        if constexpr (D > 0) load_row<D>(q, lane, qreg);
        refine_key_list<D, KIND>(X, d, s_id, n, q, qreg, KIND == K_COS ? QQ[r] : 0.f, lane, wv, metric, param, s_key);
    }
    block_bitonic_sort<uint32_t>(s_key, s_id, up2);  // (its first barrier closes the keys)
    if (wv == 0) {
        const uint32_t v = lane < g_k && lane < n ? s_id[lane] : RF_NONE;
        if (lane < g_k) line[lane] = v;
        const uint32_t kept = (uint32_t)__popcll(__ballot(v != RF_NONE && v >= lo));
        if (lane == 0) {
            atomicAdd(&ctr[1], 1ull);
            atomicAdd(&ctr[2], (unsigned long long)deg);
            if (kept) atomicAdd(&ctr[3], (unsigned long long)kept);
        }
    }
}

// a wave per line x0 + i, lane j its entry j (g_k <= 64)
__global__ __launch_bounds__(256) void gext_read_kernel(const uint32_t *__restrict__ tab, uint32_t g_k, uint64_t x0, uint64_t nl, uint64_t id_base,
                                                        uint64_t *__restrict__ out_ids, uint32_t *__restrict__ out_counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nl) return;  // (wave-uniform)
    const uint32_t e = lane < g_k ? tab[(x0 + i) * g_k + lane] : RF_NONE;
    const unsigned long long m = __ballot(e != RF_NONE);
    const uint32_t c = (uint32_t)__popcll(m);
    if (e != RF_NONE) out_ids[i * g_k + __popcll(m & ((1ull << lane) - 1ull))] = id_base + e;
    if (lane >= c && lane < g_k) out_ids[i * g_k + lane] = ~0ull;
    if (lane == 0) out_counts[i] = c;
}

hipError_t zh_launch_gext_seeds(const uint64_t *dSeeds, const uint32_t *dRows, uint32_t B, uint64_t g0, uint32_t n_seed, uint64_t *dOut, hipStream_t s) {
    if (!B) return hipSuccess;
    if (!n_seed || n_seed > ZH_GRAPH_MAX_SEEDS || B > ZH_GRAPH_EXTEND_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gext_seeds_kernel, dim3((B * n_seed + 255) / 256), dim3(256), 0, s, dSeeds, dRows, B, g0, n_seed, dOut);
    return hipGetLastError();
}

hipError_t zh_launch_gext_lines(const uint64_t *dIds, const uint32_t *dCounts, const uint32_t *dRows, uint32_t B, uint32_t g_k, uint64_t id_base, uint32_t *dTab,
                                hipStream_t s) {
    if (!B) return hipSuccess;
    if (!g_k || g_k > ZH_REFINE_MAX_IN_K || B > ZH_GRAPH_EXTEND_MAX_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gext_lines_kernel, dim3((B * g_k + 255) / 256), dim3(256), 0, s, dIds, dCounts, dRows, B, g_k, id_base, dTab);
    return hipGetLastError();
}

hipError_t zh_launch_gext_rerank(const float *dX, uint32_t d, uint32_t *dTab, uint32_t g_k, uint64_t lo, uint32_t n_chunk, const uint32_t *dBits, const float *dQQ,
                                 const uint64_t *dOff, const uint32_t *dCsr, uint32_t *dTouched, int metric, int param, unsigned long long *dCtr, hipStream_t s) {
    if (!n_chunk || !lo) return hipSuccess;
    if (!g_k || g_k > ZH_REFINE_MAX_IN_K || n_chunk > ZH_GRAPH_EXTEND_MAX_BATCH || lo >= (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t m = n_chunk * g_k;
    hipLaunchKernelGGL(gext_touched_kernel, dim3((m + 255) / 256), dim3(256), 0, s, dTab, g_k, lo, m, dOff, dCsr, dTouched, dCtr);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(m, lo);  // (the touched rows are at most that many; a block past their count leaves at once)
    return zh_dispatch_kind_dim(metric, d, [&](auto kind, auto dim) {
        hipLaunchKernelGGL((gext_rerank_kernel<decltype(dim)::value, decltype(kind)::value>), dim3(blocks), dim3(256), 0, s, dX, d, dTab, g_k, (uint32_t)lo, dBits, dQQ,
                           dOff, dCsr, dTouched, metric, param, dCtr);
        return hipGetLastError();
    });
}

hipError_t zh_launch_gext_read(const uint32_t *dTab, uint32_t g_k, uint64_t x0, uint64_t nl, uint64_t id_base, uint64_t *dOutIds, uint32_t *dOutCounts, hipStream_t s) {
    if (!g_k || g_k > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    zh_for_line_pieces(nl, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(gext_read_kernel, dim3(blocks), dim3(256), 0, s, dTab, g_k, x0 + b0, m, id_base, dOutIds + b0 * g_k, dOutCounts + b0);
    });
    return hipGetLastError();
}

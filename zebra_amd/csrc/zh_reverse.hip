// zh_reverse.hip -- the capped reverse graph (zh_knn_graph_reverse and zh_knn_graph_refine_rev, drivers in zh_api.hip): for every stored row x
//   In(x) = { u live, u != x : x in N'(u) },   R'(x) = the first min(rev_k, |In(x) - N'(x)|) of In(x) - N'(x) by (h(u, x), u),
// N'(x) as zh_refine.hip's table holds it (refine_rows_kernel: validity, liveness and repeats are settled there, once).  DESIGN.md s22.
//
//   rev_edges_kernel<false>  a thread per entry of the table: deg[v]++ for the entry v of a LIVE row's line u, u != v (vector atomics; the table
//                            holds a removed row's line too, and nobody is its neighbour)
//   rev_sums / rev_scan_sums / rev_offsets   the exclusive scan of deg into 64-bit offsets (the library's other scan, zh_launch_scan_u32, is 32-bit):
//                            4096 rows a block, the block sums by one block, then every block its own rows again
//   rev_edges_kernel<true>   the same walk: csr[off[v] + cur[v]++] = u.  The order inside a segment is whatever the atomics gave
//   rev_select_kernel        a wave per line streams its segment 64 members at a time: a member of N'(x) is dropped, h << 32 | u is the key, the
//                            running best 64 live one per lane, sorted; a chunk none of whose keys is below the rev_k-th best is not sorted at
//                            all.  No LDS; the answer is the rev_k smallest keys of a set, whatever the segment's order.  A line whose in-degree
//                            is above ZH_REVERSE_HEAVY only puts its row on a list ...
//   rev_select_heavy_kernel  ... that blocks of four waves walk: every wave the same stream over a quarter of the chunks, the four sorted bests
//                            merged through 2 KiB of LDS.  Any in-degree up to rows - 1 is served with that.
// Both write R'(x) behind N'(x) into the union table [stored rows][in_k + rev_k] (the fused call: refine_line_kernel then runs at that width) and /
// or as ids with counts and in-degrees into the caller's arrays (zh_knn_graph_reverse).
#include "zh_internal.h"
#include "zh_device.h"

#define RV_NONE 0xFFFFFFFFu
#define RV_SCAN_PER 16u      // rows a thread of the scan owns
#define RV_SCAN_ROWS 4096u   // rows a block of the scan owns

// h(u, x) = fmix32(u + 0x9E3779B9 (x + 1)), murmur3's finaliser
__host__ __device__ __forceinline__ uint32_t rev_hash(uint32_t u, uint32_t x) {
    uint32_t h = u + 0x9E3779B9u * (x + 1u);
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// entry t of the m entries of the lines from r0 (m <= 2^30): line u = r0 + t / in_k names v
template <bool FILL>
__global__ __launch_bounds__(256) void rev_edges_kernel(const uint32_t *__restrict__ tab, const uint32_t *__restrict__ bits, uint32_t in_k, uint64_t r0,
                                                        uint32_t m, uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint32_t *__restrict__ csr) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const uint64_t u = r0 + t / in_k;
    const uint32_t v = tab[r0 * in_k + t];
    if (v == RV_NONE || v == (uint32_t)u || !((bits[u >> 5] >> (u & 31)) & 1u)) return;
    const uint32_t p = atomicAdd(&cnt[v], 1u);
    if (FILL) csr[off[v] + p] = (uint32_t)u;
}

// the sum of a block's 256 u64 values, for every thread (sh: 256 words)
__device__ __forceinline__ uint64_t rev_block_sum(uint64_t v, uint64_t *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const uint64_t r = sh[0];
    __syncthreads();
    return r;
}

// the inclusive sums of a block's 256 u64 values (sh: 256 words, left holding them)
__device__ __forceinline__ uint64_t rev_block_scan(uint64_t v, uint64_t *sh) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint64_t t = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    return sh[tid];
}

// sums[b] = the in-degrees of block b's rows; ctr[1] = the largest in-degree
__global__ __launch_bounds__(256) void rev_sums_kernel(const uint32_t *__restrict__ deg, uint64_t n, uint64_t *__restrict__ sums,
                                                       unsigned long long *__restrict__ ctr) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * RV_SCAN_ROWS + threadIdx.x * RV_SCAN_PER;
    uint64_t s = 0;
    uint32_t mx = 0;
    for (uint32_t j = 0; j < RV_SCAN_PER; j++) {
        const uint32_t v = base + j < n ? deg[base + j] : 0u;
        s += v;
        mx = v > mx ? v : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = t > mx ? t : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctr[1], (unsigned long long)mx);
    s = rev_block_sum(s, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// one block: the nb block sums -> their exclusive sums in place; the total to *total and ctr[0]
__global__ __launch_bounds__(256) void rev_scan_sums_kernel(uint64_t *__restrict__ sums, uint64_t nb, uint64_t *__restrict__ total,
                                                            unsigned long long *__restrict__ ctr) {
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        const uint64_t v = i < nb ? sums[i] : 0;
        const uint64_t inc = rev_block_scan(v, sh);
        if (i < nb) sums[i] = carry + inc - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = carry;
        ctr[0] = carry;
    }
}

// off[x] = the in-degrees of the rows before x
__global__ __launch_bounds__(256) void rev_offsets_kernel(const uint32_t *__restrict__ deg, uint64_t n, const uint64_t *__restrict__ sums,
                                                          uint64_t *__restrict__ off) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * RV_SCAN_ROWS + threadIdx.x * RV_SCAN_PER;
    uint32_t v[RV_SCAN_PER];
    uint64_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < RV_SCAN_PER; j++) {
        v[j] = base + j < n ? deg[base + j] : 0u;
        s += v[j];
    }
    uint64_t run = sums[blockIdx.x] + rev_block_scan(s, sh) - s;
#pragma unroll
    for (uint32_t j = 0; j < RV_SCAN_PER; j++) {
        if (base + j < n) off[base + j] = run;
        run += v[j];
    }
}

// the lines [r0, r0 + n_lines) of the table transposed over the rows [0, n_rows) they name (zh_launch_reverse_csr: every line; the graph extension: a
// chunk of new lines over the rows before it)
hipError_t zh_launch_reverse_csr_lines(const uint32_t *dTab, const uint32_t *dBits, uint64_t n_rows, uint32_t in_k, uint64_t r0, uint64_t n_lines, uint32_t *dDeg,
                                       uint32_t *dCur, uint64_t *dOff, uint64_t *dSums, uint32_t *dCsr, unsigned long long *dCtr, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    if (!in_k || in_k > ZH_REFINE_MAX_IN_K || n_rows >= RV_NONE || r0 + n_lines >= RV_NONE) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(dDeg, 0, n_rows * 4, s)) != hipSuccess || (e = hipMemsetAsync(dCur, 0, n_rows * 4, s)) != hipSuccess) return e;
    const uint64_t step = (1ull << 30) / in_k;  // lines of one launch: at most 2^30 threads
    for (uint64_t l0 = 0; l0 < n_lines; l0 += step) {
        const uint32_t m = (uint32_t)(std::min(step, n_lines - l0) * in_k);
        hipLaunchKernelGGL(rev_edges_kernel<false>, dim3((m + 255) / 256), dim3(256), 0, s, dTab, dBits, in_k, r0 + l0, m, dDeg, nullptr, nullptr);
    }
    const uint64_t nb = (n_rows + RV_SCAN_ROWS - 1) / RV_SCAN_ROWS;  // (< 2^20)
    hipLaunchKernelGGL(rev_sums_kernel, dim3((uint32_t)nb), dim3(256), 0, s, dDeg, n_rows, dSums, dCtr);
    hipLaunchKernelGGL(rev_scan_sums_kernel, dim3(1), dim3(256), 0, s, dSums, nb, dOff + n_rows, dCtr);
    hipLaunchKernelGGL(rev_offsets_kernel, dim3((uint32_t)nb), dim3(256), 0, s, dDeg, n_rows, dSums, dOff);
    for (uint64_t l0 = 0; l0 < n_lines; l0 += step) {
        const uint32_t m = (uint32_t)(std::min(step, n_lines - l0) * in_k);
        hipLaunchKernelGGL(rev_edges_kernel<true>, dim3((m + 255) / 256), dim3(256), 0, s, dTab, dBits, in_k, r0 + l0, m, dCur, dOff, dCsr);
    }
    return hipGetLastError();
}

hipError_t zh_launch_reverse_csr(const uint32_t *dTab, const uint32_t *dBits, uint64_t n_rows, uint32_t in_k, uint32_t *dDeg, uint32_t *dCur, uint64_t *dOff, uint64_t *dSums,
                                 uint32_t *dCsr, unsigned long long *dCtr, hipStream_t s) {
    return zh_launch_reverse_csr_lines(dTab, dBits, n_rows, in_k, 0, n_rows, dDeg, dCur, dOff, dSums, dCsr, dCtr, s);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// one value per lane -> ascending over the lanes
__device__ __forceinline__ uint64_t wave_sort_u64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            const uint64_t o = shfl_u64(v, lane ^ stride);
            const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
            v = (o < v) == keep_min ? o : v;
        }
    }
    return v;
}

// two ascending runs of 64 -> the 64 smallest of both, ascending
__device__ __forceinline__ uint64_t wave_merge_low(uint64_t best, uint64_t c, uint32_t lane) {
    const uint64_t r = shfl_u64(c, 63u - lane);
    uint64_t v = r < best ? r : best;  // (bitonic)
#pragma unroll
    for (uint32_t stride = 32; stride > 0; stride >>= 1) {
        const uint64_t o = shfl_u64(v, lane ^ stride);
        const bool keep_min = (lane & stride) == 0;
        v = (o < v) == keep_min ? o : v;
    }
    return v;
}

// A wave's stream over chunks w, w + G, ... of x's segment seg[0 .. deg): -> the 64 smallest keys h << 32 | u of the members it saw that own (lane
// j: entry j of N'(x), RV_NONE from in_k on) does not hold, ascending, all ones where there are fewer.  Only what is below the rev_k-th best so far
// can matter, so a chunk without such a key costs its loads and hashes.
__device__ __forceinline__ uint64_t rev_stream(const uint32_t *__restrict__ seg, uint32_t deg, uint32_t x, uint32_t own, uint32_t in_k, uint32_t rev_k,
                                               uint32_t w, uint32_t G, uint32_t lane) {
    uint64_t best = ~0ull;
    for (uint64_t c0 = (uint64_t)w * 64; c0 < deg; c0 += (uint64_t)G * 64) {  // (wave-uniform)
        const uint64_t i = c0 + lane;
        uint32_t u = RV_NONE;
        uint64_t key = ~0ull;
        if (i < deg) {
            u = seg[i];
            key = ((uint64_t)rev_hash(u, x) << 32) | u;  // (u < stored rows < 2^32 - 1: never all ones)
        }
        bool cand = key < shfl_u64(best, rev_k - 1);
        if (__ballot(cand) == 0) continue;
        for (uint32_t j = 0; j < in_k; j++) {
            const uint32_t o = (uint32_t)__shfl((int)own, (int)j, 64);  // (by every lane: a lane that sat the shuffle out would be read as 0)
            cand = cand && o != u;
        }
        if (__ballot(cand) == 0) continue;
        best = wave_merge_low(best, wave_sort_u64(cand ? key : ~0ull, lane), lane);
    }
    return best;
}

struct RevOut {
    uint32_t *uni;         // [stored rows][in_k + rev_k], or null
    uint64_t *ids;         // [n][rev_k] of the slab, or null
    uint32_t *counts, *degree;
    uint64_t first_row, n, id_base;
};

// one wave writes line x: best as rev_stream leaves it
__device__ __forceinline__ void rev_write(const RevOut &o, uint32_t x, uint32_t deg, uint32_t own, uint64_t best, uint32_t in_k, uint32_t rev_k, uint32_t lane,
                                          unsigned long long *__restrict__ ctr) {
    const uint32_t cnt = (uint32_t)__popcll(__ballot(lane < rev_k && best != ~0ull));
    const uint32_t u = lane < cnt ? (uint32_t)best : RV_NONE;
    if (o.uni) {
        uint32_t *line = o.uni + (size_t)x * (in_k + rev_k);
        if (lane < in_k) line[lane] = own;
        if (lane < rev_k) line[in_k + lane] = u;
    }
    const uint64_t i = (uint64_t)x - o.first_row;  // (wraps past n below the slab)
    if (i < o.n) {
        if (o.ids && lane < rev_k) o.ids[i * rev_k + lane] = lane < cnt ? o.id_base + u : ~0ull;
        if (lane == 0) {
            if (o.ids) { o.counts[i] = cnt; o.degree[i] = deg; }
            if (cnt) atomicAdd(&ctr[2], (unsigned long long)cnt);
        }
    }
}

// a wave per line x0 + i, i < nx
__global__ __launch_bounds__(256) void rev_select_kernel(const uint32_t *__restrict__ tab, uint32_t in_k, uint32_t rev_k, const uint64_t *__restrict__ off,
                                                         const uint32_t *__restrict__ csr, uint64_t x0, uint64_t nx, RevOut o, uint32_t *__restrict__ heavy,
                                                         unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nx) return;  // (wave-uniform; no barrier below)
    const uint32_t x = (uint32_t)(x0 + i);
    const uint64_t b = off[x];
    const uint32_t deg = (uint32_t)(off[(uint64_t)x + 1] - b);
    if (deg > ZH_REVERSE_HEAVY) {
        if (lane == 0) heavy[atomicAdd(&ctr[3], 1ull)] = x;
        return;
    }
    const uint32_t own = lane < in_k ? tab[(size_t)x * in_k + lane] : RV_NONE;
    const uint64_t best = rev_stream(csr + b, deg, x, own, in_k, rev_k, 0, 1, lane);
    rev_write(o, x, deg, own, best, in_k, rev_k, lane, ctr);
}

// a block per listed line, the blocks striding over the list
__global__ __launch_bounds__(256) void rev_select_heavy_kernel(const uint32_t *__restrict__ tab, uint32_t in_k, uint32_t rev_k, const uint64_t *__restrict__ off,
                                                               const uint32_t *__restrict__ csr, RevOut o, const uint32_t *__restrict__ heavy,
                                                               unsigned long long *__restrict__ ctr) {
    __shared__ uint64_t s_best[4][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long nh = ctr[3];  // (final: the launches that list are done)
    for (unsigned long long h = blockIdx.x; h < nh; h += gridDim.x) {  // (block-uniform)
        const uint32_t x = heavy[h];
        const uint64_t b = off[x];
        const uint32_t deg = (uint32_t)(off[(uint64_t)x + 1] - b);
        const uint32_t own = lane < in_k ? tab[(size_t)x * in_k + lane] : RV_NONE;
        uint64_t best = rev_stream(csr + b, deg, x, own, in_k, rev_k, wv, 4, lane);
        s_best[wv][lane] = best;
        __syncthreads();
        if (wv == 0) {
            for (uint32_t w = 1; w < 4; w++) best = wave_merge_low(best, s_best[w][lane], lane);
            rev_write(o, x, deg, own, best, in_k, rev_k, lane, ctr);
        }
        __syncthreads();  // (s_best is read)
    }
}

hipError_t zh_launch_reverse_select(const uint32_t *dTab, uint32_t in_k, uint32_t rev_k, const uint64_t *dOff, const uint32_t *dCsr, uint64_t n_rows, uint64_t x0,
                                    uint64_t nx, uint64_t first_row, uint64_t n, uint64_t id_base, uint32_t *dUni, uint64_t *dOutIds, uint32_t *dOutCounts,
                                    uint32_t *dOutDegree, uint32_t *dHeavy, unsigned long long *dCtr, hipStream_t s) {
    if (!nx) return hipSuccess;
    if (!in_k || in_k > ZH_REFINE_MAX_IN_K || !rev_k || rev_k > ZH_REFINE_MAX_IN_K) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemsetAsync(&dCtr[3], 0, 8, s)) != hipSuccess) return e;
    const RevOut o{dUni, dOutIds, dOutCounts, dOutDegree, first_row, n, id_base};
    zh_for_line_pieces(nx, [&](uint64_t b0, uint64_t m, uint32_t blocks) {
        hipLaunchKernelGGL(rev_select_kernel, dim3(blocks), dim3(256), 0, s, dTab, in_k, rev_k, dOff, dCsr, x0 + b0, m, o, dHeavy, dCtr);
    });
    const uint64_t cap = std::min(nx, n_rows * in_k / ZH_REVERSE_HEAVY) + 1;  // (the list's lines share the table's n_rows in_k entries)
    hipLaunchKernelGGL(rev_select_heavy_kernel, dim3((uint32_t)std::min<uint64_t>(cap, 2048)), dim3(256), 0, s, dTab, in_k, rev_k, dOff, dCsr, o, dHeavy, dCtr);
    return hipGetLastError();
}

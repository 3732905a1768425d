// zh_filter.hip -- the filter pass of zh_search_exact_filtered_batch (zh_api.hip): the caller's bitmap ANDed with the index's live-row bitmap
// and counted, the same bitmap by POSITION of the matrix-core scan's row order, and the ascending list of its rows.
// A block owns ZH_FILTER_BLOCK_ROWS rows (256 words): its count goes to block_count, zh_launch_scan_u32 turns the counts into the exclusive
// sums the host places path 2's chunks by and filter_list_kernel scatters the list by; the 16-row tiles that hold an allowed row are counted on
// the way (*tiles: what path 2 would load, the path rule's input).  zh_compact.hip's rank pass counts the same way but
// hands out the INVERSE map (new_row[r], 4 bytes for every stored row); the list wanted here has one entry per ALLOWED row, so it gets its own
// scatter instead of a pass that inverts that map.
#include "zh_internal.h"

// c: allowed rows (a block holds at most 8192), t: tiles with an allowed row (at most 512) -- summed together, t in the upper half
__device__ __forceinline__ void filter_block_sum(uint32_t c, uint32_t t, uint32_t *__restrict__ block_count, uint32_t *__restrict__ tiles) {
    __shared__ uint32_t sm[256];
    sm[threadIdx.x] = c | (t << 16);
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_count[blockIdx.x] = sm[0] & 0xFFFFu;
        if (sm[0] >> 16) atomicAdd(tiles, sm[0] >> 16);
    }
}

// out[w] = filter[w] & live[w]; rows at and past n_bits are not allowed (bits of the filter's last word past n_bits are ignored)
__global__ __launch_bounds__(256) void filter_and_kernel(const uint32_t *__restrict__ filter, uint64_t n_bits, const uint32_t *__restrict__ live,
                                                          uint64_t n_words, uint32_t *__restrict__ out, uint32_t *__restrict__ block_count,
                                                          uint32_t *__restrict__ tiles) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t a = 0;
    if (w < n_words && w * 32 < n_bits) {
        a = filter[w];
        if (n_bits - w * 32 < 32) a &= (1u << (uint32_t)(n_bits - w * 32)) - 1u;
        a &= live[w];
    }
    if (w < n_words) out[w] = a;
    filter_block_sum((uint32_t)__popc(a), ((a & 0xFFFFu) != 0u) + ((a >> 16) != 0u), block_count, tiles);
}

// bit p of out = bit (p < perm_rows ? perm[p] : p) of bits, for p < n_rows (out: an even number of words, written whole)
__global__ __launch_bounds__(256) void filter_permute_kernel(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ perm, uint64_t perm_rows,
                                                              uint64_t n_rows, uint64_t *__restrict__ out, uint32_t *__restrict__ block_count,
                                                              uint32_t *__restrict__ tiles) {
    const uint64_t p_blk = (uint64_t)blockIdx.x * ZH_FILTER_BLOCK_ROWS;
    uint32_t c = 0, t = 0;
    for (uint32_t i = 0; i < ZH_FILTER_BLOCK_ROWS / 256; i++) {
        const uint64_t p = p_blk + i * 256 + threadIdx.x;
        bool on = false;
        if (p < n_rows) {
            const uint32_t r = p < perm_rows ? perm[p] : (uint32_t)p;
            on = (bits[r >> 5] >> (r & 31)) & 1u;
        }
        const uint64_t m = __ballot(on);
        if ((threadIdx.x & 63) == 0 && p < n_rows) {  // (p: the wave's first position)
            out[p >> 6] = m;
            c += (uint32_t)__popcll(m);
            for (int j = 0; j < 4; j++) t += ((m >> (16 * j)) & 0xFFFFull) != 0ull;
        }
    }
    filter_block_sum(c, t, block_count, tiles);
}

// list[block_excl[block] + rank within the block] = row, ascending
__global__ __launch_bounds__(256) void filter_list_kernel(const uint32_t *__restrict__ bits, uint64_t n_words, const uint32_t *__restrict__ block_excl,
                                                           uint32_t *__restrict__ list) {
    __shared__ uint32_t s_base[256];
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t word = w < n_words ? bits[w] : 0u;
    const uint32_t c = (uint32_t)__popc(word);
    s_base[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {  // inclusive scan of the words' counts
        const uint32_t x = threadIdx.x >= off ? s_base[threadIdx.x - off] : 0u;
        __syncthreads();
        s_base[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t at = block_excl[blockIdx.x] + s_base[threadIdx.x] - c;
    while (word) {
        list[at++] = (uint32_t)(w * 32) + (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
    }
}

static uint32_t filter_blocks(uint64_t n_rows) { return (uint32_t)((n_rows + ZH_FILTER_BLOCK_ROWS - 1) / ZH_FILTER_BLOCK_ROWS); }

hipError_t zh_launch_filter_and(const uint32_t *dFilter, uint64_t n_bits, const uint32_t *dLiveBits, uint64_t n_rows, uint32_t *dOut,
                                uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp, uint32_t *dTiles, hipStream_t s) {
    hipError_t e = hipMemsetAsync(dTiles, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (!n_rows) return hipMemsetAsync(dBlockExcl, 0, sizeof(uint32_t), s);
    const uint32_t nb = filter_blocks(n_rows);
    hipLaunchKernelGGL(filter_and_kernel, dim3(nb), dim3(256), 0, s, dFilter, n_bits, dLiveBits, (n_rows + 31) / 32, dOut, dBlockCount, dTiles);
    return zh_launch_scan_u32(dBlockCount, dBlockExcl, nb, dScanTmp, s);
}

hipError_t zh_launch_filter_permute(const uint32_t *dBits, const uint32_t *dPerm, uint64_t perm_rows, uint64_t n_rows, uint32_t *dOut,
                                    uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp, uint32_t *dTiles, hipStream_t s) {
    hipError_t e = hipMemsetAsync(dTiles, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (!n_rows) return hipMemsetAsync(dBlockExcl, 0, sizeof(uint32_t), s);
    const uint32_t nb = filter_blocks(n_rows);
    hipLaunchKernelGGL(filter_permute_kernel, dim3(nb), dim3(256), 0, s, dBits, dPerm, perm_rows, n_rows, (uint64_t *)dOut, dBlockCount, dTiles);
    return zh_launch_scan_u32(dBlockCount, dBlockExcl, nb, dScanTmp, s);
}

hipError_t zh_launch_filter_list(const uint32_t *dBits, uint64_t n_rows, const uint32_t *dBlockExcl, uint32_t *dList, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    hipLaunchKernelGGL(filter_list_kernel, dim3(filter_blocks(n_rows)), dim3(256), 0, s, dBits, (n_rows + 31) / 32, dBlockExcl, dList);
    return hipGetLastError();
}

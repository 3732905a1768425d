// zh_compact.hip -- kernels of zh_index_compact (zh_api.hip): the rank of every stored row among the live ones, the move of the live
// rows down over the removed ones, and the renumbering of whatever names a row (leaf_ids, the planes' sample rows).
#include "zh_internal.h"

#define ZH_ROW_GONE 0xFFFFFFFFu

// ---- rank: new_row[r] = live rows before r for a live row, ZH_ROW_GONE for a removed one ---------------------------------------
// The live rows come as a bitmap (bit r % 32 of word r / 32; bits at and past n_rows are zero).  A block owns ZH_COMPACT_RANK_ROWS
// rows = 256 words: rank_count_kernel counts them, zh_launch_scan_u32 scans the blocks' counts, rank_apply_kernel hands out the ranks.
__global__ __launch_bounds__(256) void rank_count_kernel(const uint32_t *__restrict__ bits, uint64_t n_words, uint32_t *__restrict__ block_count) {
    __shared__ uint32_t sm[256];
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    sm[threadIdx.x] = w < n_words ? (uint32_t)__popc(bits[w]) : 0u;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_count[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(256) void rank_apply_kernel(const uint32_t *__restrict__ bits, uint64_t n_words, uint64_t n_rows,
                                                          const uint32_t *__restrict__ block_excl, uint32_t *__restrict__ new_row) {
    __shared__ uint32_t s_word[256], s_base[256];
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t word = w < n_words ? bits[w] : 0u, c = (uint32_t)__popc(word);
    s_base[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {  // inclusive scan of the words' counts
        const uint32_t x = threadIdx.x >= off ? s_base[threadIdx.x - off] : 0u;
        __syncthreads();
        s_base[threadIdx.x] += x;
        __syncthreads();
    }
    const uint32_t excl = block_excl[blockIdx.x] + s_base[threadIdx.x] - c;
    __syncthreads();
    s_word[threadIdx.x] = word;
    s_base[threadIdx.x] = excl;
    __syncthreads();
    const uint64_t row0 = (uint64_t)blockIdx.x * ZH_COMPACT_RANK_ROWS;
    for (uint32_t i = 0; i < 32; i++) {  // consecutive lanes write consecutive rows
        const uint32_t rl = i * 256 + threadIdx.x, wd = s_word[rl >> 5], bit = rl & 31u;
        if (row0 + rl < n_rows)
            new_row[row0 + rl] = ((wd >> bit) & 1u) ? s_base[rl >> 5] + (uint32_t)__popc(wd & ((1u << bit) - 1u)) : ZH_ROW_GONE;
    }
}

hipError_t zh_launch_compact_rank(const uint32_t *dLiveBits, uint64_t n_rows, uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp,
                                  uint32_t *dNewRow, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    const uint64_t n_words = (n_rows + 31) / 32;
    const uint32_t nb = (uint32_t)((n_rows + ZH_COMPACT_RANK_ROWS - 1) / ZH_COMPACT_RANK_ROWS);
    hipLaunchKernelGGL(rank_count_kernel, dim3(nb), dim3(256), 0, s, dLiveBits, n_words, dBlockCount);
    hipError_t e = zh_launch_scan_u32(dBlockCount, dBlockExcl, nb, dScanTmp, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rank_apply_kernel, dim3(nb), dim3(256), 0, s, dLiveBits, n_words, n_rows, dBlockExcl, dNewRow);
    return hipGetLastError();
}

// ---- the move ---------------------------------------------------------------------------------------------------------------------
// Source rows [r0, r0 + n) of `src` go to row (map ? map[r] : r) - sub of `dst`; a row whose map entry is ZH_ROW_GONE goes nowhere.  One wave
// per ZH_MOVE_ROWS consecutive source rows (= consecutive destination rows, less the gaps).  The wave's rows are ONE flat run of
// ZH_MOVE_ROWS * vec_per_row vectors (the source rows are contiguous) dealt to the lanes 64 at a time, so that every lane works whatever the
// row length (a 512-byte row is 32 vectors: lane by vector alone would idle half the wave); a lane finds its vector's row by one division and
// the row's destination by a select over the wave's ZH_MOVE_ROWS entries.  ZH_MOVE_UNROLL loads are issued before the first store, in the
// widest vector the row length and the alignment allow, nontemporal on both sides (nothing is read twice).
// The CALLER keeps a launch's source and destination ranges apart (zh_api.hip, zh_index_compact): nothing here orders a read after a write.
#define ZH_MOVE_ROWS 8
#define ZH_MOVE_UNROLL 4
typedef float zc_f32x4 __attribute__((ext_vector_type(4)));
typedef float zc_f32x2 __attribute__((ext_vector_type(2)));

template <typename V>
__global__ __launch_bounds__(256) void move_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, const uint32_t *__restrict__ map,
                                                         uint64_t r0, uint64_t n, uint64_t sub, uint32_t vec_per_row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = r0 + ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ZH_MOVE_ROWS;
    if (first >= r0 + n) return;
    const uint32_t rows = (uint32_t)(r0 + n - first < ZH_MOVE_ROWS ? r0 + n - first : ZH_MOVE_ROWS);
    uint64_t to[ZH_MOVE_ROWS];  // destination row, or ~0: not moved
#pragma unroll
    for (int j = 0; j < ZH_MOVE_ROWS; j++) {
        to[j] = ~0ull;
        if ((uint32_t)j < rows) {
            const uint64_t r = first + j;
            const uint32_t mv = map ? map[r] : 0u;
            if (!map) to[j] = r - sub;
            else if (mv != ZH_ROW_GONE) to[j] = (uint64_t)mv - sub;
        }
    }
    const V *__restrict__ s = reinterpret_cast<const V *>(src) + first * vec_per_row;
    V *__restrict__ t = reinterpret_cast<V *>(dst);
    const uint32_t total = rows * vec_per_row;
    for (uint32_t base = 0; base < total; base += 64 * ZH_MOVE_UNROLL) {
        V v[ZH_MOVE_UNROLL];
        uint64_t at[ZH_MOVE_UNROLL];  // destination vector, or ~0
#pragma unroll
        for (int u = 0; u < ZH_MOVE_UNROLL; u++) {
            const uint32_t i = base + u * 64 + lane;
            at[u] = ~0ull;
            if (i < total) {
                const uint32_t j = i / vec_per_row, c = i - j * vec_per_row;
                uint64_t tj = to[0];
#pragma unroll
                for (int q = 1; q < ZH_MOVE_ROWS; q++) tj = j == (uint32_t)q ? to[q] : tj;
                if (tj != ~0ull) {
                    at[u] = tj * vec_per_row + c;
                    v[u] = __builtin_nontemporal_load(s + i);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ZH_MOVE_UNROLL; u++)
            if (at[u] != ~0ull) __builtin_nontemporal_store(v[u], t + at[u]);
    }
}

hipError_t zh_launch_move_rows(const float *dSrc, float *dDst, uint32_t d, const uint32_t *dMap, uint64_t r0, uint64_t n, uint64_t sub, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + 4 * ZH_MOVE_ROWS - 1) / (4 * ZH_MOVE_ROWS);
    if (blocks > 0x7FFFFFFFull || (uint64_t)d * ZH_MOVE_ROWS > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // rows of d floats start at multiples of 4 d bytes from 256-byte aligned bases
    const bool a16 = (d & 3u) == 0 && (((uintptr_t)dSrc | (uintptr_t)dDst) & 15u) == 0;
    const bool a8 = (d & 1u) == 0 && (((uintptr_t)dSrc | (uintptr_t)dDst) & 7u) == 0;
    if (a16)
        hipLaunchKernelGGL(move_rows_kernel<zc_f32x4>, dim3((uint32_t)blocks), dim3(256), 0, s, dSrc, dDst, dMap, r0, n, sub, d / 4);
    else if (a8)
        hipLaunchKernelGGL(move_rows_kernel<zc_f32x2>, dim3((uint32_t)blocks), dim3(256), 0, s, dSrc, dDst, dMap, r0, n, sub, d / 2);
    else
        hipLaunchKernelGGL(move_rows_kernel<float>, dim3((uint32_t)blocks), dim3(256), 0, s, dSrc, dDst, dMap, r0, n, sub, d);
    return hipGetLastError();
}

// ---- renumbering --------------------------------------------------------------------------------------------------------------------
// Every slot of leaf_ids, the slack between the leaves' runs included (relocated and shrunken runs leave stale ids behind: they name rows that
// were stored once, possibly removed since -- those become row 0, so that a pass over every slot still reads inside the table).
__global__ __launch_bounds__(256) void renumber_ids_kernel(uint32_t *__restrict__ ids, uint64_t n, const uint32_t *__restrict__ new_row, uint64_t rows_before) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = ids[i];
    if (v >= rows_before) return;
    const uint32_t m = new_row[v];
    ids[i] = m == ZH_ROW_GONE ? 0u : m;
}
hipError_t zh_launch_renumber_ids(uint32_t *dIds, uint64_t n, const uint32_t *dNewRow, uint64_t rows_before, hipStream_t s) {
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(renumber_ids_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, dIds, n, dNewRow, rows_before);
    return hipGetLastError();
}

// The planes' sample rows (UINT32_MAX = the default zero vector stays).  A plane made from a row that was removed since keeps its values but has
// no sample row any more: *flag |= 1, and the row-score hash (which reads the samples' scores) is off until the forest is rebuilt.
__global__ __launch_bounds__(256) void renumber_samples_kernel(uint2 *__restrict__ samples, uint32_t n, const uint32_t *__restrict__ new_row,
                                                                uint64_t rows_before, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint2 v = samples[i];
    bool lost = false;
    if (v.x != 0xFFFFFFFFu) {
        const uint32_t m = v.x < rows_before ? new_row[v.x] : ZH_ROW_GONE;
        lost |= m == ZH_ROW_GONE;
        v.x = m == ZH_ROW_GONE ? 0u : m;
    }
    if (v.y != 0xFFFFFFFFu) {
        const uint32_t m = v.y < rows_before ? new_row[v.y] : ZH_ROW_GONE;
        lost |= m == ZH_ROW_GONE;
        v.y = m == ZH_ROW_GONE ? 0u : m;
    }
    samples[i] = v;
    if (lost) atomicOr(flag, 1u);
}
hipError_t zh_launch_renumber_samples(uint2 *dSamples, uint32_t n, const uint32_t *dNewRow, uint64_t rows_before, uint32_t *dFlag, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(renumber_samples_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dSamples, n, dNewRow, rows_before, dFlag);
    return hipGetLastError();
}

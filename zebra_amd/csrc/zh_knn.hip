// zh_knn.hip -- exact k-NN graph (zh_knn_graph, driver in zh_api.hip): for every live stored row a of a slab [first_row, first_row + n) its exact
// top-k by (key, id) over every live row EXCEPT a itself.  The key of (a, b) is the key zh_distance_batch gives for stored row b against a query
// equal to the f32 values of row a -- the self-join's orientation.  Only the row with the same row number is excluded: a bit-identical duplicate
// is an ordinary neighbour, ties order by id.  Output line i belongs to stored row first_row + i; a removed row's line has count 0.  DESIGN.md s16.
//
// The work goes panel by panel: up to ZH_KNN_PANEL_ROWS live rows of the slab, ascending by row number.
//   path 1  join_gather_kernel gathers the panel's f32 rows into the exact search's query buffer, the exact search's path 1 answers it with k + 1
//           over the live list, knn_emit_kernel writes each line's first k entries that are not the line's own id.  Right whatever self's key is:
//           if self is among the k + 1 it is taken out, if it is not the first k never held it.
//   path 2  knn_panel_kernel gathers the panel's tiles out of the fp16 row copy into scratch, in the MFMA operand's own order (the copy's own bits:
//           its measured rho holds), with their rowMeta and row numbers.  knn_mfma_kernel is the held-tile walk of zh_device.h
//           with the list sink: a block's four waves hold four consecutive panel tiles and walk a chunk of column tiles of the copy.  The held
//           row is approx_interval's "stored row", the column its "query" (qm from join_prep_kernel); self is excluded by row number, a masked
//           row on either side is skipped.  Every held row has its own tau, count and (row, lo, hi) list -- ZhExact2's layout with B = the
//           panel's lines.  The columns come in the exact search's schedule (max(k + 1, 4096) positions,
//           then ZH_EXACT_GROWTH times as many each launch) with exact_prune_kernel after each launch; then qnorm_kernel on the gathered f32
//           panel, exact_survivor_keys_kernel, final_kernel -- all unchanged -- and knn_emit_kernel puts the lines at their places.  A panel
//           whose flag is raised is answered by path 1.
// Scratch (all per call, released before return).  Path 2: 20 bytes per position of the copy (qm and the id-or-masked word), 4 bytes per stored row
// under a row order (row -> position), and for ONE panel of P <= 1024 lines: P (2 d + 12) bytes of tiles, rowMeta and row numbers, 4 P d of f32
// rows, 36 P cap bytes of lists, prune scratch and survivor keys (cap = 16384 + 8 k), 16 P k + 4 P of panel answer.  Path 1: the exact search's
// query buffer, key scratch (<= 1 GiB) and candidates, 16 P (k + 1) + 4 P of panel answer.  The host call: 16 k + 4 bytes per line of a sub-slab
// of at most 65536 lines as staging.
#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

// under a row order: pos[row] = the position of live row `row` in the copy (cid: join_prep_kernel's id-or-masked word per position)
__global__ __launch_bounds__(256) void knn_rowpos_kernel(const uint32_t *__restrict__ cid, uint64_t n_pos, uint32_t *__restrict__ pos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pos) return;
    const uint32_t id = cid[p];
    if (id != 0xFFFFFFFFu) pos[id] = (uint32_t)p;
}

hipError_t zh_launch_knn_rowpos(const uint32_t *dCid, uint64_t n_pos, uint32_t *dPos, hipStream_t s) {
    if (!n_pos) return hipSuccess;
    hipLaunchKernelGGL(knn_rowpos_kernel, dim3((uint32_t)((n_pos + 255) / 256)), dim3(256), 0, s, dCid, n_pos, dPos);
    return hipGetLastError();
}

// The panel's tiles: line b (live row rows[b], b < B) of panel tile b / 16 gets the 16-byte pieces of its position in the copy.  A tile is NS * 64
// pieces, piece 64 st + 16 h + line: thread t of the grid writes piece t of the panel's tiles (line = t % 16 runs fastest: the stores are
// contiguous, and so are the loads where the panel's rows are).  Lines past B (the last tile's tail) are zero and masked (pid = UINT32_MAX).
__global__ __launch_bounds__(256) void knn_panel_kernel(const u32x4 *__restrict__ Xh, const float2 *__restrict__ rowMeta, const uint32_t *__restrict__ pos,
                                                        const uint32_t *__restrict__ rows, uint32_t B, uint32_t PT, uint32_t pieces, u32x4 *__restrict__ A,
                                                        float2 *__restrict__ pmeta, uint32_t *__restrict__ pid) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)PT * pieces) return;
    const uint32_t tile = (uint32_t)(t / pieces), w = (uint32_t)(t % pieces), b = tile * 16 + (w & 15);
    u32x4 v = {0u, 0u, 0u, 0u};
    uint32_t row = 0xFFFFFFFFu;
    float2 rm = make_float2(0.f, 0.f);
    if (b < B) {
        row = rows[b];
        const uint64_t p = pos ? pos[row] : row;
        v = Xh[(p >> 4) * pieces + (w & ~15u) + (p & 15)];
        if (w < 16) rm = rowMeta[p];
    }
    A[t] = v;
    if (w < 16) { pid[b] = row; pmeta[b] = rm; }
}

hipError_t zh_launch_knn_panel(uint32_t d, const void *dXh, const float2 *dRowMeta, const uint32_t *dPos, const uint32_t *dRows, uint32_t B, void *dA,
                               float2 *dPMeta, uint32_t *dPid, hipStream_t s) {
    if (!B) return hipSuccess;
    const uint32_t PT = (B + 15) / 16, pieces = d / 32 * 64;
    const uint64_t n = (uint64_t)PT * pieces;
    hipLaunchKernelGGL(knn_panel_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const u32x4 *)dXh, dRowMeta, dPos, dRows, B, PT, pieces,
                       (u32x4 *)dA, dPMeta, dPid);
    return hipGetLastError();
}

// grid (chunks of `ch` column tiles of [Jt0, Jt1), held blocks of four panel tiles)
template <int D, int KINDA>
__global__ __launch_bounds__(256) void knn_mfma_kernel(const u32x4 *__restrict__ Xh, const float4 *__restrict__ qm, const uint32_t *__restrict__ cid,
                                                       uint64_t Jt0, uint64_t Jt1, uint32_t ch, const u32x4 *__restrict__ PA,
                                                       const float2 *__restrict__ pmeta, const uint32_t *__restrict__ pid, uint32_t PT, float Kc, float rho,
                                                       const uint32_t *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ lid,
                                                       uint32_t *__restrict__ llo, uint32_t *__restrict__ lhi, uint32_t cap, uint32_t *__restrict__ over) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t I = blockIdx.y * 4 + wid;  // the wave's panel tile
    const uint64_t Jb = Jt0 + (uint64_t)blockIdx.x * ch, Je = Jb + ch < Jt1 ? Jb + ch : Jt1;
    const bool active = I < PT;  // (wave-uniform: the panel's last block may hold fewer than four tiles)
    f16x8 A[D / 32];
    held_tile<D>(A, PA, (size_t)I, active, lane);
    ListSink<KINDA> sink{lane, Kc, rho, cnt, lid, llo, lhi, cap, cap, over};
    sink.hold(active, I * 16, pid, pmeta, tau);
    held_walk<D>(A, active, Xh, cid, qm, Jb, Je, sink);
}

// column tiles a block walks: ZH_KNN_CHUNK, fewer in a short launch so that it still fills the device (about 1024 blocks), never under 8
uint32_t zh_knn_chunk(uint64_t tiles, uint32_t n_ab) {
    const uint64_t c = tiles * n_ab / 1024;
    return (uint32_t)std::min<uint64_t>(ZH_KNN_CHUNK, std::max<uint64_t>(8, c));
}

hipError_t zh_launch_knn_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, const float4 *dQm, const uint32_t *dCid, uint64_t p_begin, uint64_t p_end,
                              const void *dA, const float2 *dPMeta, const uint32_t *dPid, hipStream_t s) {
    if (p_begin >= p_end || !e.B) return hipSuccess;
    if (p_begin % 16 || e.B > ZH_KNN_PANEL_ROWS) return hipErrorInvalidValue;
    const uint64_t Jt0 = p_begin / 16, Jt1 = (p_end + 15) / 16;
    const uint32_t PT = (e.B + 15) / 16, n_ab = (PT + 3) / 4, ch = zh_knn_chunk(Jt1 - Jt0, n_ab);
    const dim3 grid((uint32_t)((Jt1 - Jt0 + ch - 1) / ch), n_ab);
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((knn_mfma_kernel<D, K>), grid, dim3(256), 0, s, (const u32x4 *)e.Xh, dQm, dCid, Jt0, Jt1, ch, (const u32x4 *)dA, dPMeta, dPid, PT, e.Kc,
                           e.rho, e.tau, e.cnt, e.lid, e.llo, e.lhi, e.cap, e.over);
    });
}

// A panel's answer to its lines' places: a wave per line b.  in_*: [B][w] as final_kernel wrote them (ids = id_base + row, ascending by (key, id),
// counts[b] entries); the line of row rows[b] gets the first k entries whose id is not the row's own, the count, and UINT64_MAX past it.
__global__ __launch_bounds__(256) void knn_emit_kernel(const uint64_t *__restrict__ in_ids, const uint64_t *__restrict__ in_keys,
                                                       const uint32_t *__restrict__ in_counts, uint32_t w, const uint32_t *__restrict__ rows, uint32_t B,
                                                       uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *__restrict__ out_ids,
                                                       uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;  // (wave-uniform)
    const uint32_t row = rows[b];
    const uint64_t own = id_base + row;
    const uint32_t n = in_counts[b] < w ? in_counts[b] : w;
    const uint64_t *ii = in_ids + (size_t)b * w, *ik = in_keys + (size_t)b * w;
    uint32_t self = n;  // the position of the line's own id (n: not there)
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
        const uint64_t m = __ballot(j0 + lane < n && ii[j0 + lane] == own);
        if (m) { self = j0 + (uint32_t)__builtin_ctzll(m); break; }  // (wave-uniform)
    }
    const uint32_t left = self < n ? n - 1 : n, take = left < k ? left : k;
    const size_t o = (size_t)(row - first_row) * k;
    for (uint32_t j = lane; j < k; j += 64) {
        const uint32_t src = j < self ? j : j + 1;
        out_ids[o + j] = j < take ? ii[src] : ~0ull;
        out_keys[o + j] = j < take ? ik[src] : ~0ull;
    }
    if (lane == 0) out_counts[row - first_row] = take;
}

hipError_t zh_launch_knn_emit(const uint64_t *dInIds, const uint64_t *dInKeys, const uint32_t *dInCounts, uint32_t w, const uint32_t *dRows, uint32_t B,
                              uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(knn_emit_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dInIds, dInKeys, dInCounts, w, dRows, B, id_base, first_row, k, dOutIds, dOutKeys,
                       dOutCounts);
    return hipGetLastError();
}

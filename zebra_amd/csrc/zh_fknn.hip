// zh_fknn.hip -- forest k-NN graph (zh_knn_graph_forest, driver in zh_api.hip): for every stored row a of a slab [first_row, first_row + n) the first k by
// (key, id) of C(a) = the union over the trees of the members of a's leaf, minus a itself.  Keys, orientation, ids, tails and counts as zh_knn.hip
// (DESIGN.md s16); what is approximate is the candidate set, never the arithmetic.  DESIGN.md s17.
//
//   path 1  every metric, every dimension, every leaf shape, and the redo of a path-2 batch whose lists ran over.  A sub-slab's row -> leaf table
//           (fknn_rowleaf_kernel: {offset into leaf_ids, length} per (row, tree)), its lines (rows that some tree holds: fknn_lines_kernel, a scan,
//           fknn_compact_kernel), then panel by panel: join_gather_kernel gathers the panel's f32 rows as queries, fknn_visits_kernel writes one
//           ZhVisit and one ZhGroup of a single member per (line, tree) -- the line's own leaf, no walk -- the leaf-major f32 sweep keys them,
//           select_kernel takes each visit's first k + 1, final_kernel ranks a line's T visits by (key, id) with duplicates across trees dropped
//           by id, and knn_emit_kernel writes the first k that are not the line's own id.
//   path 2  leaf-major on the matrix cores from the fp16 row copy, one tree at a time, a tree in batches of leaves (of segments: a window of
//           at most ZH_FKNN_HELD_ROWS members of one leaf as held rows, the whole leaf as columns).  fknn_cols_kernel lists a batch's column rows
//           (a leaf padded to whole tiles), fknn_held_kernel compacts each segment's members that lie in the slab into its held rows (stable: the
//           leaf's order) and counts them, fknn_gather_kernel copies either list's tiles out of the copy by row number (through the row ->
//           position map under a scan order) into the MFMA operand's order with rowMeta and the row as approx_interval's query.  fknn_mfma_kernel
//           is knn_mfma_kernel's scheme (the held-tile walk with the list sink) over MANY leaves in one launch: a block finds
//           its segment in the batch's block table, holds up to four tiles of that segment's held rows and walks a chunk of the segment's
//           column tiles.  A line's tau starts from its running answer
//           (the k-th key after the earlier trees, through range_tau_kernel; all ones while it holds fewer than k) and is lowered by
//           exact_prune_kernel from THIS tree's list alone, whose rows are distinct.  The survivors get the canonical key, the running answer is
//           appended to them (fknn_seed_kernel), final_kernel ranks both with duplicates dropped by id, fknn_store_kernel writes the line back.
// Scratch: the header's comment on zh_knn_graph_forest and DESIGN.md s17 state the bounds.
#include <algorithm>

#include "zh_internal.h"
#include "zh_device.h"

// ---- both paths: the row -> leaf table of a sub-slab [r0, r0 + m), its lines and the pairs they stand for ----
// a block per node: a leaf of tree t writes {offset into leaf_ids, length} for its members that lie in the sub-slab
__global__ __launch_bounds__(64) void fknn_rowleaf_kernel(const int4 *__restrict__ node_pack, const uint32_t *__restrict__ node_tree,
                                                          const uint32_t *__restrict__ leaf_ids, uint32_t T, uint64_t r0, uint32_t m, uint32_t node0,
                                                          uint2 *__restrict__ rl) {
    const uint32_t node = node0 + blockIdx.x;
    const int4 rec = node_pack[node];
    if (rec.x >= 0) return;  // inner node
    const uint32_t t = node_tree[node];
    if (t >= T) return;      // not reachable from a root
    const uint32_t off = (uint32_t)rec.y, len = (uint32_t)rec.z;
    for (uint32_t i = threadIdx.x; i < len; i += 64) {
        const uint64_t r = leaf_ids[(size_t)off + i];
        if (r >= r0 && r - r0 < m) rl[(size_t)(r - r0) * T + t] = make_uint2(off, len);
    }
}

hipError_t zh_launch_fknn_rowleaf(const int4 *dNodePack, const uint32_t *dNodeTree, uint32_t n_nodes, const uint32_t *dLeafIds, uint32_t T, uint64_t r0,
                                  uint32_t m, uint2 *dRl, hipStream_t s) {
    if (!m || !T) return hipSuccess;
    hipError_t e = hipMemsetAsync(dRl, 0xFF, (size_t)m * T * sizeof(uint2), s);  // {-1, -1}: the row is not in that tree
    if (e != hipSuccess) return e;
    for (uint32_t n0 = 0; n0 < n_nodes; n0 += (1u << 22)) {
        const uint32_t nb = n_nodes - n0 < (1u << 22) ? n_nodes - n0 : (1u << 22);
        hipLaunchKernelGGL(fknn_rowleaf_kernel, dim3(nb), dim3(64), 0, s, dNodePack, dNodeTree, dLeafIds, T, r0, m, n0, dRl);
    }
    return hipGetLastError();
}

// flag[i] = row r0 + i is in some tree; *pairs += the sum over its trees of (length of its leaf - 1)
__global__ __launch_bounds__(256) void fknn_lines_kernel(const uint2 *__restrict__ rl, uint32_t T, uint32_t m, uint32_t *__restrict__ flag,
                                                         unsigned long long *__restrict__ pairs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long sum = 0;
    if (i < m) {
        uint32_t any = 0;
        for (uint32_t t = 0; t < T; t++) {
            const uint2 e = rl[(size_t)i * T + t];
            if (e.x != 0xFFFFFFFFu) { any = 1; sum += e.y - 1u; }
        }
        flag[i] = any;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(pairs, sum);
}

__global__ __launch_bounds__(256) void fknn_compact_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl, uint32_t m, uint64_t r0,
                                                           uint32_t *__restrict__ rows) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m && flag[i]) rows[excl[i]] = (uint32_t)(r0 + i);
}

hipError_t zh_launch_fknn_lines(const uint2 *dRl, uint32_t T, uint64_t r0, uint32_t m, uint32_t *dFlag, uint32_t *dExcl, uint32_t *dScanTmp, uint32_t *dRows,
                                unsigned long long *dPairs, hipStream_t s) {
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(fknn_lines_kernel, dim3((m + 255) / 256), dim3(256), 0, s, dRl, T, m, dFlag, dPairs);
    hipError_t e = zh_launch_scan_u32(dFlag, dExcl, m, dScanTmp, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fknn_compact_kernel, dim3((m + 255) / 256), dim3(256), 0, s, dFlag, dExcl, m, r0, dRows);
    return hipGetLastError();
}

// ---- path 1: a panel's visits.  Line b = row rows[b]; its visit of tree t is its own leaf there (none: length 0) ----
// lens / takes [B * T]: the visits' leaf lengths and min(w, length)
__global__ __launch_bounds__(256) void fknn_visit_sizes_kernel(const uint2 *__restrict__ rl, uint32_t T, uint64_t r0, const uint32_t *__restrict__ rows,
                                                               uint32_t B, uint32_t w, uint32_t *__restrict__ lens, uint32_t *__restrict__ takes) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= B * T) return;
    const uint2 e = rl[(size_t)(rows[v / T] - r0) * T + v % T];
    const uint32_t len = e.x != 0xFFFFFFFFu ? e.y : 0u;
    lens[v] = len;
    takes[v] = len < w ? len : w;
}

// ... and from their exclusive sums (B * T + 1 entries each) the visits, a group of ONE member per visit for the sweep, the groups' first flat rows
// and the candidates' bases as final_kernel reads them
__global__ __launch_bounds__(256) void fknn_visits_kernel(const uint2 *__restrict__ rl, uint32_t T, uint64_t r0, const uint32_t *__restrict__ rows,
                                                          uint32_t B, uint32_t w, const uint32_t *__restrict__ rowBase, const uint32_t *__restrict__ candBase,
                                                          ZhVisit *__restrict__ visits, ZhGroup *__restrict__ groups, uint64_t *__restrict__ groupRowOff,
                                                          uint64_t *__restrict__ candBase64) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v > B * T) return;
    candBase64[v] = candBase[v];
    if (v == B * T) return;
    const uint32_t b = v / T;
    const uint2 e = rl[(size_t)(rows[b] - r0) * T + v % T];
    const bool in = e.x != 0xFFFFFFFFu;
    const uint32_t off = in ? e.x : 0u, len = in ? e.y : 0u;
    ZhVisit vis;
    vis.b = b; vis.leaf_off = off; vis.len = len; vis.take = len < w ? len : w;
    vis.row_off = rowBase[v]; vis.cand_off = candBase[v]; vis.node = 0; vis.pad = 0;
    visits[v] = vis;
    ZhGroup g;
    g.leaf_off = off; g.len = len; g.gsize = 1; g.take4 = 0;
    for (int j = 0; j < ZH_GROUP_MAX; j++) { g.b[j] = b; g.key_off[j] = rowBase[v]; }
    groups[v] = g;
    groupRowOff[v] = rowBase[v];
}

hipError_t zh_launch_fknn_visit_sizes(const uint2 *dRl, uint32_t T, uint64_t r0, const uint32_t *dRows, uint32_t B, uint32_t w, uint32_t *dLens,
                                      uint32_t *dTakes, hipStream_t s) {
    if (!B || !T) return hipSuccess;
    hipLaunchKernelGGL(fknn_visit_sizes_kernel, dim3((B * T + 255) / 256), dim3(256), 0, s, dRl, T, r0, dRows, B, w, dLens, dTakes);
    return hipGetLastError();
}

hipError_t zh_launch_fknn_visits(const uint2 *dRl, uint32_t T, uint64_t r0, const uint32_t *dRows, uint32_t B, uint32_t w, const uint32_t *dRowBase,
                                 const uint32_t *dCandBase, ZhVisit *dVisits, ZhGroup *dGroups, uint64_t *dGroupRowOff, uint64_t *dCandBase64, hipStream_t s) {
    if (!B || !T) return hipSuccess;
    hipLaunchKernelGGL(fknn_visits_kernel, dim3((B * T + 256) / 256), dim3(256), 0, s, dRl, T, r0, dRows, B, w, dRowBase, dCandBase, dVisits, dGroups,
                       dGroupRowOff, dCandBase64);
    return hipGetLastError();
}

// ---- path 2 ----
// under a row order: pos[row] = the row's position in the copy (position p < perm_rows holds row perm[p], a later one row p)
__global__ __launch_bounds__(256) void fknn_rowpos_kernel(const uint32_t *__restrict__ perm, uint64_t perm_rows, uint64_t n_rows, uint32_t *__restrict__ pos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_rows) return;
    pos[p < perm_rows ? perm[p] : (uint32_t)p] = (uint32_t)p;
}

hipError_t zh_launch_fknn_rowpos(const uint32_t *dPerm, uint64_t perm_rows, uint64_t n_rows, uint32_t *dPos, hipStream_t s) {
    if (!n_rows) return hipSuccess;
    hipLaunchKernelGGL(fknn_rowpos_kernel, dim3((uint32_t)((n_rows + 255) / 256)), dim3(256), 0, s, dPerm, perm_rows, n_rows, dPos);
    return hipGetLastError();
}

// the batch's column rows: column tile c of the batch holds members [src[c].x, src[c].x + src[c].y) of leaf_ids (y <= 16), UINT32_MAX past them
__global__ __launch_bounds__(256) void fknn_cols_kernel(const uint2 *__restrict__ src, uint32_t n_tiles, const uint32_t *__restrict__ leaf_ids, uint64_t n_rows,
                                                        uint32_t *__restrict__ crow) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tiles * 16) return;
    const uint2 e = src[t >> 4];
    uint32_t row = 0xFFFFFFFFu;
    if ((t & 15) < e.y) {
        row = leaf_ids[(size_t)e.x + (t & 15)];
        if (row >= n_rows) row = 0xFFFFFFFFu;
    }
    crow[t] = row;
}

// a block per segment: the members [held_off, held_off + held_len) of leaf_ids that lie in [first_row, first_row + n), in the leaf's order, as the
// segment's held rows hrow[line0 ..] (UINT32_MAX past them, up to the segment's 16 * held_tiles lines); held[seg] = their number; *tiles += the tile
// products the segment's blocks issue (held tiles in use x column tiles)
__global__ __launch_bounds__(256) void fknn_held_kernel(const ZhFknnSeg *__restrict__ segs, const uint32_t *__restrict__ leaf_ids, uint64_t first_row, uint64_t n,
                                                        uint32_t *__restrict__ hrow, uint32_t *__restrict__ held, unsigned long long *__restrict__ tiles) {
    __shared__ uint32_t sc[256], s_base;
    const ZhFknnSeg sg = segs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < sg.held_len; j0 += 256) {
        const uint32_t j = j0 + tid;
        uint32_t row = 0xFFFFFFFFu;
        if (j < sg.held_len) {
            const uint64_t r = leaf_ids[(size_t)sg.held_off + j];
            if (r >= first_row && r - first_row < n) row = (uint32_t)r;
        }
        const uint32_t f = row != 0xFFFFFFFFu ? 1u : 0u;
        sc[tid] = f;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const uint32_t a = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += a;
            __syncthreads();
        }
        const uint32_t base = s_base;
        if (f) hrow[sg.line0 + base + sc[tid] - 1] = row;
        __syncthreads();
        if (tid == 255) s_base = base + sc[255];
        __syncthreads();
    }
    const uint32_t cnt = s_base;
    for (uint32_t i = cnt + tid; i < sg.held_tiles * 16; i += 256) hrow[sg.line0 + i] = 0xFFFFFFFFu;
    if (tid == 0) {
        held[blockIdx.x] = cnt;
        if (cnt) atomicAdd(tiles, (unsigned long long)((cnt + 15) / 16) * sg.ct);
    }
}

// The tiles of a row list (n_tiles * 16 rows, UINT32_MAX = no row: zero and masked) out of the fp16 copy, in the MFMA operand's own order (the copy's own
// bits), as knn_panel_kernel: a tile is NS * 64 pieces of 16 bytes, piece 64 st + 16 h + line; thread t writes piece t.  Per row its rowMeta and, when
// qm is asked for, the row as approx_interval's query (join_prep_kernel's values).
__global__ __launch_bounds__(256) void fknn_gather_kernel(const u32x4 *__restrict__ Xh, const float2 *__restrict__ rowMeta, const uint32_t *__restrict__ pos,
                                                          const uint32_t *__restrict__ rows, uint32_t n_tiles, uint32_t pieces, float rho, u32x4 *__restrict__ A,
                                                          float2 *__restrict__ meta, float4 *__restrict__ qm) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_tiles * pieces) return;
    const uint32_t tile = (uint32_t)(t / pieces), w = (uint32_t)(t % pieces), b = tile * 16 + (w & 15);
    u32x4 v = {0u, 0u, 0u, 0u};
    float2 rm = make_float2(0.f, 0.f);
    float4 o = make_float4(NAN, NAN, NAN, NAN);
    const uint32_t row = rows[b];
    if (row != 0xFFFFFFFFu) {
        const uint64_t p = pos ? pos[row] : row;
        v = Xh[(p >> 4) * pieces + (w & ~15u) + (p & 15)];
        if (w < 16) {
            rm = rowMeta[p];
            o = row_as_query(rm, rho);
        }
    }
    A[t] = v;
    if (w < 16) {
        meta[b] = rm;
        if (qm) qm[b] = o;
    }
}

hipError_t zh_launch_fknn_cols(const uint2 *dSrc, uint32_t n_tiles, const uint32_t *dLeafIds, uint64_t n_rows, uint32_t *dCRow, hipStream_t s) {
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL(fknn_cols_kernel, dim3((n_tiles * 16 + 255) / 256), dim3(256), 0, s, dSrc, n_tiles, dLeafIds, n_rows, dCRow);
    return hipGetLastError();
}

hipError_t zh_launch_fknn_held(const ZhFknnSeg *dSegs, uint32_t n_segs, const uint32_t *dLeafIds, uint64_t first_row, uint64_t n, uint32_t *dHRow,
                               uint32_t *dHeld, unsigned long long *dTiles, hipStream_t s) {
    if (!n_segs) return hipSuccess;
    hipLaunchKernelGGL(fknn_held_kernel, dim3(n_segs), dim3(256), 0, s, dSegs, dLeafIds, first_row, n, dHRow, dHeld, dTiles);
    return hipGetLastError();
}

hipError_t zh_launch_fknn_gather(uint32_t d, const void *dXh, const float2 *dRowMeta, const uint32_t *dPos, const uint32_t *dRows, uint32_t n_tiles, float rho,
                                 void *dA, float2 *dMeta, float4 *dQm, hipStream_t s) {
    if (!n_tiles) return hipSuccess;
    const uint32_t pieces = d / 32 * 64;
    const uint64_t n = (uint64_t)n_tiles * pieces;
    hipLaunchKernelGGL(fknn_gather_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, (const u32x4 *)dXh, dRowMeta, dPos, dRows, n_tiles, pieces, rho,
                       (u32x4 *)dA, dMeta, dQm);
    return hipGetLastError();
}

// per held line b: qrow[b] = its row (0 for no row: a row that may be gathered), maxk[b] = the k-th key of its running answer, all ones while the
// answer holds fewer than k
__global__ __launch_bounds__(256) void fknn_bound_kernel(const uint32_t *__restrict__ hrow, uint32_t B, uint64_t first_row, uint32_t k,
                                                         const uint64_t *__restrict__ out_keys, const uint32_t *__restrict__ out_counts,
                                                         uint32_t *__restrict__ qrow, uint64_t *__restrict__ maxk) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const uint32_t row = hrow[b];
    uint64_t mk = ~0ull;
    if (row != 0xFFFFFFFFu) {
        const uint64_t i = row - first_row;
        if (out_counts[i] >= k) mk = out_keys[i * k + (k - 1)];
    }
    qrow[b] = row != 0xFFFFFFFFu ? row : 0u;
    maxk[b] = mk;
}

hipError_t zh_launch_fknn_bound(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint32_t k, const uint64_t *dOutKeys, const uint32_t *dOutCounts,
                                uint32_t *dQRow, uint64_t *dMaxK, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(fknn_bound_kernel, dim3((B + 255) / 256), dim3(256), 0, s, dHRow, B, first_row, k, dOutKeys, dOutCounts, dQRow, dMaxK);
    return hipGetLastError();
}

// One launch over every segment of a batch.  Block x finds its segment sg (first_block <= x, the table ends with a sentinel of n_blocks), then
// lb = x - first_block: held block lb % n_hb (four held tiles, a wave each), column chunk lb / n_hb (ch tiles) -- neighbours share a chunk.  A block
// whose held tiles are past the segment's held rows (held[seg], counted on the device) leaves at once.
template <int D, int KINDA>
__global__ __launch_bounds__(256) void fknn_mfma_kernel(const ZhFknnSeg *__restrict__ segs, uint32_t n_segs, const uint32_t *__restrict__ held, uint32_t ch,
                                                        const u32x4 *__restrict__ CA, const float4 *__restrict__ cqm, const uint32_t *__restrict__ crow,
                                                        const u32x4 *__restrict__ HA, const float2 *__restrict__ hmeta, const uint32_t *__restrict__ hrow,
                                                        float Kc, float rho, const uint32_t *__restrict__ tau, uint32_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ lid, uint32_t *__restrict__ llo, uint32_t *__restrict__ lhi, uint32_t cap,
                                                        uint32_t lim, uint32_t *__restrict__ over) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t seg = last_le(n_segs, blockIdx.x, [&](uint32_t i) { return segs[i].first_block; });  // (block-uniform)
    const ZhFknnSeg sg = segs[seg];
    const uint32_t n_held = held[seg], ht = (n_held + 15) / 16, n_hb = (sg.held_tiles + 3) / 4;
    const uint32_t lb = blockIdx.x - sg.first_block, hb = lb % n_hb, chunk = lb / n_hb;
    if (4 * hb >= ht) return;  // (block-uniform) no held row of the slab here
    const uint32_t I = 4 * hb + wid;   // the wave's held tile of the segment
    const uint32_t Jb = sg.col0 + chunk * ch, Jend = sg.col0 + sg.ct, Je = Jb + ch < Jend ? Jb + ch : Jend;
    if (Jb >= Je) return;  // (block-uniform; the host's geometry launches no such block)
    const bool active = I < ht;  // (wave-uniform)
    f16x8 A[D / 32];
    held_tile<D>(A, HA, (size_t)(sg.line0 >> 4) + I, active, lane);
    ListSink<KINDA> sink{lane, Kc, rho, cnt, lid, llo, lhi, cap, lim, over};
    sink.hold(active, sg.line0 + I * 16, hrow, hmeta, tau);
    held_walk<D>(A, active, CA, crow, cqm, Jb, Je, sink);
}

hipError_t zh_launch_fknn_mfma(uint32_t d, int metric, int mode, const ZhFknnSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, const uint32_t *dHeld, uint32_t ch,
                               const void *dCA, const float4 *dCQm, const uint32_t *dCRow, const void *dHA, const float2 *dHMeta, const uint32_t *dHRow,
                               const ZhExact2 &e, uint32_t lim, hipStream_t s) {
    if (!n_segs || !n_blocks) return hipSuccess;
    if (!ch || lim > e.cap) return hipErrorInvalidValue;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((fknn_mfma_kernel<D, K>), dim3(n_blocks), dim3(256), 0, s, dSegs, n_segs, dHeld, ch, (const u32x4 *)dCA, dCQm, dCRow, (const u32x4 *)dHA,
                           dHMeta, dHRow, e.Kc, e.rho, e.tau, e.cnt, e.lid, e.llo, e.lhi, e.cap, lim, e.over);
    });
}

// a wave per held line b: its running answer (the line's count entries of the outputs) goes behind its cnt[b] survivors in the candidate slots
// (cnt[b] <= lim = cap - k: there is room), as (key, row)
__global__ __launch_bounds__(256) void fknn_seed_kernel(const uint32_t *__restrict__ hrow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k,
                                                        const uint64_t *__restrict__ out_ids, const uint64_t *__restrict__ out_keys,
                                                        const uint32_t *__restrict__ out_counts, const uint32_t *__restrict__ cnt, uint32_t cap,
                                                        uint64_t *__restrict__ ckeys, uint32_t *__restrict__ cids, const uint32_t *__restrict__ over) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B || *over) return;
    const uint32_t row = hrow[b];
    if (row == 0xFFFFFFFFu) return;
    const uint64_t i = row - first_row;
    const uint32_t have = out_counts[i] < k ? out_counts[i] : k, c = cnt[b];
    if (c + have > cap) return;  // (never: c <= cap - k)
    for (uint32_t j = lane; j < have; j += 64) {
        ckeys[(size_t)b * cap + c + j] = out_keys[i * k + j];
        cids[(size_t)b * cap + c + j] = (uint32_t)(out_ids[i * k + j] - id_base);
    }
}

// a wave per held line b: the batch's answer [B][k] (final_kernel's) becomes the line's running answer.  final_kernel reads the empty candidate slots
// as ONE more entry, (UINT64_MAX, id_base + UINT32_MAX), ranked last: a line with fewer than k candidates holds it, and it is not counted
__global__ __launch_bounds__(256) void fknn_store_kernel(const uint32_t *__restrict__ hrow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k,
                                                         const uint64_t *__restrict__ in_ids, const uint64_t *__restrict__ in_keys,
                                                         uint64_t *__restrict__ out_ids, uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_counts,
                                                         const uint32_t *__restrict__ over) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B || *over) return;  // (wave-uniform)
    const uint32_t row = hrow[b];
    if (row == 0xFFFFFFFFu) return;
    const uint64_t i = row - first_row, none = id_base + 0xFFFFFFFFull;
    uint32_t count = 0;
    for (uint32_t j0 = 0; j0 < k; j0 += 64) {
        const uint32_t j = j0 + lane;
        uint64_t id = ~0ull, key = ~0ull;
        if (j < k) {
            id = in_ids[(size_t)b * k + j]; key = in_keys[(size_t)b * k + j];
            if (id == none) { id = ~0ull; key = ~0ull; }
            out_ids[i * k + j] = id; out_keys[i * k + j] = key;
        }
        count += (uint32_t)__popcll(__ballot(id != ~0ull));
    }
    if (lane == 0) out_counts[i] = count;
}

hipError_t zh_launch_fknn_seed(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k, const uint64_t *dOutIds,
                               const uint64_t *dOutKeys, const uint32_t *dOutCounts, const ZhExact2 &e, uint64_t *dCKeys, uint32_t *dCIds, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(fknn_seed_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dHRow, B, first_row, id_base, k, dOutIds, dOutKeys, dOutCounts, e.cnt, e.cap, dCKeys,
                       dCIds, (const uint32_t *)e.over);
    return hipGetLastError();
}

hipError_t zh_launch_fknn_store(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k, const uint64_t *dInIds,
                                const uint64_t *dInKeys, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, const uint32_t *dOver, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(fknn_store_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dHRow, B, first_row, id_base, k, dInIds, dInKeys, dOutIds, dOutKeys, dOutCounts,
                       dOver);
    return hipGetLastError();
}

// the sub-slabs of a batch whose lists ran over: path 1 answers them afterwards
__global__ __launch_bounds__(256) void fknn_mark_kernel(const uint32_t *__restrict__ hrow, uint32_t B, uint64_t first_row, uint32_t *__restrict__ redo) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < B && hrow[b] != 0xFFFFFFFFu) redo[(hrow[b] - first_row) / ZH_FKNN_SLAB] = 1u;
}

hipError_t zh_launch_fknn_mark(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint32_t *dRedo, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(fknn_mark_kernel, dim3((B + 255) / 256), dim3(256), 0, s, dHRow, B, first_row, dRedo);
    return hipGetLastError();
}

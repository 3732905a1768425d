// zh_fjoin.hip -- forest self-join (zh_self_join_forest, driver in zh_api.hip): every unordered pair of distinct stored rows (a, b), a < b by row
// number, that are members of the SAME leaf in at least one tree and whose key is <= ONE threshold key, each pair once however many trees put the
// two rows together.  Key, orientation, order, threshold and output are zh_join.hip's: the key of (a, b) is that of stored row b
// against a query equal to the f32 row a, hits go to ONE pool per call (v = a << 32 | b and the key) and are counted whether or not the pool has
// room, zh_launch_pair_sort orders the pool by (a, key, b).  What is approximate is the candidate set, never the arithmetic.  DESIGN.md s18.
//
// Each pair once: leaf_of[row][tree] = the offset into leaf_ids of the row's leaf in that tree (UINT32_MAX: the tree does not hold the row), built
// once per call by fjoin_rowleaf_kernel.  A pair met in tree t is kept only if leaf_of[a][t'] != leaf_of[b][t'] for every t' < t: the FIRST tree
// that puts the two rows together owns the pair.  Ownership depends on the forest alone -- not on a path, a batch or a position of the scan's row
// order -- so any set of leaves may be answered by either path and the hit counter may run on past the pool.  The comparisons (at most T - 1) are
// paid by candidates (path 2) or by keys already at or below the threshold (path 1), never per product.
//
//   path 1  every metric, dimension and leaf shape, and the redo of a path-2 batch whose candidate pool ran over.  A panel is a list of pieces
//           {leaf, a range of its members as lines}: fjoin_groups_kernel writes the lines' rows and groups of up to ZH_GROUP_MAX lines that visit
//           the one leaf, join_gather_kernel gathers the lines' f32 rows as queries, the leaf-major f32 sweep keys the leaf's rows against them,
//           fjoin_collect_kernel takes the keys <= max_key whose row number is above the line's and that pass the first-tree rule.
//   path 2  a batch of one tree's leaves, each padded to whole tiles by masked rows, is gathered ONCE out of the fp16 copy (zh_fknn.hip's cols /
//           gather kernels).  fjoin_mfma_kernel is join_mfma_kernel's triangle over MANY leaves in one launch: a block finds its segment (a leaf's
//           four held tiles from I0) by binary search over the segments' first blocks, holds tiles I0 .. I0 + 3 of that leaf, one per wave, and
//           walks ONE chunk of the leaf's tiles counted from its own diagonal (the held-tile walk with the pool sink's upper-triangle rule,
//           DESIGN.md s15a); a gathered tile serves as either MFMA operand (s15).  The held row is approx_interval's "stored row", the LDS row
//           its "query": s15's argument for two rounded operands applies word for word.  Pairs with lo <= tau go to the
//           batch's candidate pool as min(row) << 32 | max(row); pair_survivors_kernel (zh_join.hip; OWNED) applies the first-tree rule, gives the
//           rest the canonical key of (row b, query = f32 row a), judges key <= max_key, counts and pools.
// Scratch (all per call, released before return): leaf_of is 4 bytes per (stored row, tree) -- 4 N T, 600 MB at 10M rows x 15 trees, not chunked
// -- and the node -> tree map 4 bytes per node; path 2 per batch of at most max(ZH_FKNN_COL_TILES tiles, the longest leaf) gathered rows 2 d + 28
// bytes per row, 16 bytes per segment and 8 bytes per candidate slot (at most max(1.25 x the capacity left, 256 per gathered row), never more than
// the batch's leaf pairs), plus 4 bytes per stored row under a scan order that is not id order; path 1 per panel of at most ZH_FJOIN_PANEL_LINES
// lines 4 d + 24 bytes per line, 56 bytes per group and 8 bytes per key of at most max(2^25, the longest leaf) keys; both 16 bytes per hit-pool
// slot (<= the capacity), for the order as much again plus hipCUB's temporary storage, and 24 bytes per pair of staging for the host call.
#include "zh_internal.h"
#include "zh_device.h"

// ---- both paths: leaf_of.  A block per node: a leaf of tree t writes its offset for its members; *leaf_pairs += len (len - 1) / 2 ----
__global__ __launch_bounds__(64) void fjoin_rowleaf_kernel(const int4 *__restrict__ node_pack, const uint32_t *__restrict__ node_tree,
                                                           const uint32_t *__restrict__ leaf_ids, uint32_t T, uint64_t n_rows, uint32_t node0,
                                                           uint32_t *__restrict__ leaf_of, unsigned long long *__restrict__ leaf_pairs) {
    const uint32_t node = node0 + blockIdx.x;
    const int4 rec = node_pack[node];
    if (rec.x >= 0) return;  // inner node
    const uint32_t t = node_tree[node];
    if (t >= T) return;      // not reachable from a root
    const uint32_t off = (uint32_t)rec.y, len = (uint32_t)rec.z;
    for (uint32_t i = threadIdx.x; i < len; i += 64) {
        const uint64_t r = leaf_ids[(size_t)off + i];
        if (r < n_rows) leaf_of[(size_t)r * T + t] = off;
    }
    if (threadIdx.x == 0 && len >= 2) atomicAdd(leaf_pairs, (unsigned long long)len * (len - 1) / 2);
}

hipError_t zh_launch_fjoin_rowleaf(const int4 *dNodePack, const uint32_t *dNodeTree, uint32_t n_nodes, const uint32_t *dLeafIds, uint32_t T, uint64_t n_rows,
                                   uint32_t *dLeafOf, unsigned long long *dLeafPairs, hipStream_t s) {
    if (!T) return hipSuccess;
    if (n_rows) {
        hipError_t e = hipMemsetAsync(dLeafOf, 0xFF, (size_t)n_rows * T * 4, s);  // UINT32_MAX: the row is not in that tree
        if (e != hipSuccess) return e;
    }
    for (uint32_t n0 = 0; n0 < n_nodes; n0 += (1u << 22)) {
        const uint32_t nb = n_nodes - n0 < (1u << 22) ? n_nodes - n0 : (1u << 22);
        hipLaunchKernelGGL(fjoin_rowleaf_kernel, dim3(nb), dim3(64), 0, s, dNodePack, dNodeTree, dLeafIds, T, n_rows, n0, dLeafOf, dLeafPairs);
    }
    return hipGetLastError();
}

// ---- path 1: a panel's lines and groups.  Group g belongs to the last piece whose group0 <= g; it holds up to ZH_GROUP_MAX consecutive lines of the
// piece, which all visit the piece's leaf ----
__global__ __launch_bounds__(256) void fjoin_groups_kernel(const ZhFjoinPiece *__restrict__ pieces, uint32_t n_pieces, uint32_t n_groups,
                                                           const uint32_t *__restrict__ leaf_ids, uint64_t n_rows, uint32_t *__restrict__ rows,
                                                           uint2 *__restrict__ lineLeaf, uint64_t *__restrict__ lineKey, ZhGroup *__restrict__ groups,
                                                           uint64_t *__restrict__ groupRowOff) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const ZhFjoinPiece pc = pieces[last_le(n_pieces, g, [&](uint32_t i) { return pieces[i].group0; })];
    const uint32_t gi = g - pc.group0, j0 = gi * ZH_GROUP_MAX, left = pc.nl - j0, gsize = left < ZH_GROUP_MAX ? left : ZH_GROUP_MAX;
    ZhGroup gr;
    gr.leaf_off = pc.off; gr.len = pc.len; gr.gsize = gsize; gr.take4 = 0;
    for (uint32_t m = 0; m < ZH_GROUP_MAX; m++) {
        const uint32_t j = j0 + (m < gsize ? m : 0u), line = pc.line0 + j;
        const uint64_t ko = pc.key0 + (uint64_t)j * pc.len;
        gr.b[m] = line;
        gr.key_off[m] = ko;
        if (m < gsize) {
            const uint32_t row = leaf_ids[(size_t)pc.off + pc.i0 + j];
            const bool ok = row < n_rows;  // (always, for a forest this library built: a line that is no stored row collects nothing)
            rows[line] = ok ? row : 0u;
            lineLeaf[line] = make_uint2(pc.off, ok ? pc.len : 0u);
            lineKey[line] = ko;
        }
    }
    groups[g] = gr;
    groupRowOff[g] = pc.flat0 + (uint64_t)gi * pc.len;
}

hipError_t zh_launch_fjoin_groups(const ZhFjoinPiece *dPieces, uint32_t n_pieces, uint32_t n_groups, const uint32_t *dLeafIds, uint64_t n_rows, uint32_t *dRows,
                                  uint2 *dLineLeaf, uint64_t *dLineKey, ZhGroup *dGroups, uint64_t *dGroupRowOff, hipStream_t s) {
    if (!n_pieces || !n_groups) return hipSuccess;
    hipLaunchKernelGGL(fjoin_groups_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, s, dPieces, n_pieces, n_groups, dLeafIds, n_rows, dRows, dLineLeaf,
                       dLineKey, dGroups, dGroupRowOff);
    return hipGetLastError();
}

// a block per line: the hits among its leaf's keys -- key <= max_key, the member's row number above the line's, the pair owned by tree t
__global__ __launch_bounds__(256) void fjoin_collect_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rows,
                                                            const uint2 *__restrict__ lineLeaf, const uint64_t *__restrict__ lineKey,
                                                            const uint32_t *__restrict__ leaf_ids, uint64_t n_rows, const uint32_t *__restrict__ leaf_of,
                                                            uint32_t T, uint32_t t, uint64_t max_key, unsigned long long *__restrict__ ctr,
                                                            uint64_t *__restrict__ pv, uint64_t *__restrict__ pk, uint64_t cap) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63;
    const uint32_t a = rows[b];
    const uint2 lf = lineLeaf[b];
    const uint64_t ko = lineKey[b];
    for (uint32_t i0 = 0; i0 < lf.y; i0 += 256) {  // (block-uniform)
        const uint32_t i = i0 + threadIdx.x;
        uint64_t key = 0;
        uint32_t row = 0;
        bool hit = false;
        if (i < lf.y) {
            row = leaf_ids[(size_t)lf.x + i];
            key = keys[ko + i];
            hit = row > a && row < n_rows && key <= max_key && fjoin_owned(leaf_of, T, t, a, row);
        }
        const uint64_t m = __ballot(hit);
        if (!m) continue;  // (wave-uniform)
        const unsigned long long slot = wave_slots(ctr, m, lane);  // always: the count stays exact when the pool is full
        if (hit && slot < cap) {
            pv[slot] = ((uint64_t)a << 32) | row;
            pk[slot] = key;
        }
    }
}

hipError_t zh_launch_fjoin_collect(const uint64_t *dKeys, const uint32_t *dRows, const uint2 *dLineLeaf, const uint64_t *dLineKey, uint32_t B,
                                   const uint32_t *dLeafIds, uint64_t n_rows, const uint32_t *dLeafOf, uint32_t T, uint32_t t, uint64_t max_key,
                                   unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s) {
    if (!B) return hipSuccess;
    hipLaunchKernelGGL(fjoin_collect_kernel, dim3(B), dim3(256), 0, s, dKeys, dRows, dLineLeaf, dLineKey, dLeafIds, n_rows, dLeafOf, T, t, max_key, dHitCtr,
                       dPoolV, dPoolK, pool_cap);
    return hipGetLastError();
}

// ---- path 2 ----
// The launch geometry of a batch (the host's, fjoin_batch2 in zh_api.hip): a leaf of ct tiles at column tile col0 of the batch gives one segment per
// held block I0 = 0, 4, 8, ... < ct, whose ceil((ct - I0) / ch) blocks walk the chunks [I0 + ch c, I0 + ch (c + 1)) cut at ct: chunks are counted from
// the held block's own diagonal, so none lies wholly below it.  Wave I issues ct - I tile products, the leaf ct (ct + 1) / 2.
// One launch over every segment of a batch.  Block x finds its segment sg (the last whose first_block <= x), then chunk = x - first_block.  CA / meta /
// qm / crow are the batch's gathered tiles, rowMeta, query views and row-or-masked words (zh_launch_fknn_gather, zh_launch_fknn_cols).
template <int D, int KINDA>
__global__ __launch_bounds__(256) void fjoin_mfma_kernel(const ZhFjoinSeg *__restrict__ segs, uint32_t n_segs, uint32_t ch, const u32x4 *__restrict__ CA,
                                                         const float2 *__restrict__ cmeta, const float4 *__restrict__ cqm, const uint32_t *__restrict__ crow,
                                                         float Kc, float rho, const uint32_t *__restrict__ tau, uint64_t *__restrict__ cand, uint64_t cap,
                                                         unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ZhFjoinSeg sg = segs[last_le(n_segs, blockIdx.x, [&](uint32_t i) { return segs[i].first_block; })];  // (block-uniform)
    // tiles of the batch: the leaf's are [col0, Tend); the wave holds I, the block walks [Jb, Je)
    const uint32_t Tend = sg.col0 + sg.ct, I = sg.col0 + sg.I0 + wid;
    const uint32_t Jb = sg.col0 + sg.I0 + (blockIdx.x - sg.first_block) * ch;
    if (Jb >= Tend) return;  // (block-uniform; the host's geometry launches no such block)
    const uint32_t Je = Jb + ch < Tend ? Jb + ch : Tend;
    const bool active = I < Tend;  // (wave-uniform: a leaf's last held block may hold fewer than four tiles)
    f16x8 A[D / 32];
    held_tile<D>(A, CA, (size_t)I, active, lane);
    PoolSink<KINDA, true, uint32_t> sink{lane, I, tau[0], Kc, rho, cand, cap, ctr};
    sink.hold(active, crow, cmeta);
    held_walk<D>(A, active, CA, crow, cqm, Jb, Je, sink);  // (in its first chunk wave w skips the w tiles before its own)
}

hipError_t zh_launch_fjoin_mfma(uint32_t d, int metric, int mode, const ZhFjoinSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, uint32_t ch, const void *dCA,
                                const float2 *dCMeta, const float4 *dCQm, const uint32_t *dCRow, float Kc, float rho, const uint32_t *dTau, uint64_t *dCand,
                                uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s) {
    if (!n_segs || !n_blocks) return hipSuccess;
    if (!ch) return hipErrorInvalidValue;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((fjoin_mfma_kernel<D, K>), dim3(n_blocks), dim3(256), 0, s, dSegs, n_segs, ch, (const u32x4 *)dCA, dCMeta, dCQm, dCRow, Kc, rho, dTau,
                           dCand, cand_cap, dCandCtr);
    });
}

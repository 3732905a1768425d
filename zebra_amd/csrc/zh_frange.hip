// zh_frange.hip -- forest range search (zh_search_range_forest_batch, driver in zh_api.hip): for every query, every stored row that is a member of a
// leaf the walk (tree_result, lsh.rs:290-348, with n = probe) visits for that query in some tree and whose canonical key is <= the query's threshold
// key, as a CSR over the queries, each segment ascending by (key, id).  Keys, order, thresholds, pool and output are zh_range.hip's:
// hits go to ONE pool per internal batch (v = query << 32 | row and the key), are counted per query in cnt[] whether or not the pool has room, and
// zh_launch_range_offsets / zh_launch_range_sort finish the batch.  What is approximate is the candidate set, never the arithmetic.  DESIGN.md s19.
//
// Front end (both paths): the LSH search's own launchers (zh_search.hip), unchanged, on scratch of this family: batch_init, walk_count with every
// sign on demand, leaf_scan / pair_scan, then expand (or walk_emit when the visit log ran over) -> the ZhVisit list, pair (query b, tree t) at
// [visitBase[b T + t], visitBase[b T + t + 1]), and the per-leaf groups.  The walk records a visit where it takes rows: an empty leaf is passed
// through and is no visit.
//
// Each hit once: a row may be a member of several visited leaves, one per tree at most (within a tree the walk visits no leaf twice).  With
// leaf_of[row][tree] (zh_fjoin.hip's table, built per call) a pair (query, row) met in a visited leaf of tree t is kept only if for every earlier
// tree t' < t the row's leaf in t' is NOT among the leaves the query visited in t': the first tree that offers the row owns the pair.  The lookup is
// the visit list itself: frange_visit_index sorts the words pair << 32 | leaf offset, which leaves every pair's slice where visitBase puts it,
// ordered by leaf offset, and frange_owned searches the slice of (b, t') for the row's leaf.  Ownership depends on the forest and the walk alone, so
// cnt[] and the hit counter stay exact past the pool and either path may answer any internal batch.  The check is paid by pairs that passed the
// threshold (path 1) or the interval test (path 2), never per scored pair.
//
//   path 1  every metric, dimension and leaf shape, and the redo of a path-2 batch whose candidate pool ran over.  zh_launch_sweep writes the
//           canonical key of every visited row into the visits' key slices; frange_collect_kernel reads them, a wave per visit, 64 rows at a time.
//   path 2  L2SQ / L2 / cosine at d = 256 .. 1024 (forest_path2's rule).  Per internal batch the visited leaves are listed on the host from the
//           per-leaf visit counts; a leaf's visitors are the members of its groups, visitor j = member j % G of group group0 + j / G.  Batches of
//           at most ZH_FKNN_COL_TILES row tiles are gathered ONCE from the fp16 copy (zh_fknn.hip's cols / gather kernels: operand order, rowMeta,
//           position map under a row order).  frange_mfma_kernel: a block holds four 16-row tiles of one leaf in registers, one per wave, and walks
//           a chunk of the leaf's 16-visitor column tiles, the queries' halves read from zh_launch_qhalf's copy exactly as range_mfma_kernel does:
//           a leaf's rows are read once per 16 visitors (once per chunk, in fact).  The sum is tile_dot's (zh_device.h), the bound
//           zh_approx_bound(metric, d, 1), so approx_interval and the s14 argument "key <= max_key implies lo <= tau_q" apply unchanged.  A pair
//           with lo <= tau_q that passes the ownership rule goes to the candidate pool as query << 32 | row; nothing is stored per scored pair.
//           zh_launch_range_survivors then gives the candidates the canonical key, judges, counts and pools, as it is.
//           Leaf-major work pays where leaves are shared: the host keeps an internal batch on path 1 unless its visited leaves have
//           ZH_FRANGE_MIN_VISITORS visitors on average (zh_api.hip; DESIGN.md s19 has the measurements).
// Scratch (all per call, released before return): leaf_of 4 bytes per (stored row, tree) and the node -> tree map 4 bytes per node, as the forest
// join; per internal batch of at most ZH_EXACT_BATCH queries the walk's 16 bytes per node, (32 * 40 + 44) bytes per (query, tree) pair, the visit
// log, and 40 + 16 bytes per visit, 56 bytes per group; path 1: 8 bytes per visited row -- an internal batch whose visits hold more than
// ZH_FRANGE_KEY_ROWS rows (2^25: 256 MiB of keys) is cut in half, query-wise, until it fits or is one query; path 2: per batch of leaves
// 2 d + 12 bytes per gathered row (at most max(ZH_FKNN_COL_TILES tiles, the longest leaf)), 32 bytes per leaf, 2 d + 24 bytes per query, 8 bytes
// per candidate slot (at most max(1.25 x the capacity left, ZH_RANGE_CAND_FLOOR per query), never more than the visited rows), 4 bytes per stored
// row under a scan order that is not id order; both 16 bytes per hit-pool slot (<= the capacity), for the order as much again plus hipCUB's
// temporary storage, and 16 bytes per hit of staging for the host call.
#include <hipcub/hipcub.hpp>

#include "zh_internal.h"
#include "zh_device.h"

// ---- both paths: the lookup of visited leaves.  vkey[i] = (b T + t) << 32 | leaf offset of visit i, then sorted ----
__global__ __launch_bounds__(256) void frange_vkeys_kernel(const ZhVisit *__restrict__ visits, uint64_t n, const uint32_t *__restrict__ node_tree, uint32_t T,
                                                           uint64_t *__restrict__ vkey) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ZhVisit v = visits[i];
    vkey[i] = ((uint64_t)(v.b * T + node_tree[v.node]) << 32) | v.leaf_off;
}

hipError_t zh_launch_frange_visit_index(const ZhVisit *dVisits, uint64_t n_visits, const uint32_t *dNodeTree, uint32_t T, uint64_t n_pairs, uint64_t *dKeys[2],
                                        void *dTmp, size_t *tmp_bytes, const uint64_t **dSorted, hipStream_t s) {
    hipcub::DoubleBuffer<uint64_t> k(dKeys[0], dKeys[1]);
    const int end_bit = 32 + field_bits(n_pairs);
    hipError_t e;
    if (!dTmp) {
        size_t a = 0;
        if ((e = hipcub::DeviceRadixSort::SortKeys(nullptr, a, k, n_visits, 0, end_bit, s)) != hipSuccess) return e;
        *tmp_bytes = std::max<size_t>(a, 1);
        return hipSuccess;
    }
    *dSorted = dKeys[0];
    if (!n_visits) return hipSuccess;
    hipLaunchKernelGGL(frange_vkeys_kernel, dim3((uint32_t)((n_visits + 255) / 256)), dim3(256), 0, s, dVisits, n_visits, dNodeTree, T, dKeys[0]);
    size_t bytes = *tmp_bytes;
    if ((e = hipcub::DeviceRadixSort::SortKeys(dTmp, bytes, k, n_visits, 0, end_bit, s)) != hipSuccess) return e;
    *dSorted = k.Current();
    return hipGetLastError();
}

// tree t owns the pair (query b, row) when no earlier tree's visited leaves hold the row
__device__ __forceinline__ bool frange_owned(const uint64_t *__restrict__ vsorted, const uint64_t *__restrict__ visitBase, const uint32_t *__restrict__ leaf_of,
                                             uint32_t T, uint32_t t, uint32_t b, uint32_t row) {
    const uint32_t *lr = leaf_of + (size_t)row * T;
    for (uint32_t u = 0; u < t; u++) {
        const uint32_t x = lr[u];
        if (x == 0xFFFFFFFFu) continue;
        const uint32_t pair = b * T + u;
        const uint64_t want = ((uint64_t)pair << 32) | x;
        uint64_t lo = visitBase[pair], hi = visitBase[pair + 1];  // the first entry >= want of the pair's slice
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (vsorted[mid] < want) lo = mid + 1; else hi = mid;
        }
        if (lo < visitBase[pair + 1] && vsorted[lo] == want) return false;
    }
    return true;
}

// ---- path 1: the hits among the swept keys.  A wave per visit, 64 consecutive rows of its leaf at a time ----
__global__ __launch_bounds__(256) void frange_collect_kernel(const ZhVisit *__restrict__ visits, uint64_t n_visits, const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ leaf_ids, uint64_t n_rows, const uint32_t *__restrict__ node_tree,
                                                             const uint64_t *__restrict__ vsorted, const uint64_t *__restrict__ visitBase,
                                                             const uint32_t *__restrict__ leaf_of, uint32_t T, const uint64_t *__restrict__ maxk,
                                                             uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr, uint64_t *__restrict__ pv,
                                                             uint64_t *__restrict__ pk, uint64_t cap) {
    const uint64_t vi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (vi >= n_visits) return;  // (wave-uniform)
    const ZhVisit v = visits[vi];
    const uint32_t t = node_tree[v.node];
    const uint64_t mk = maxk[v.b];
    for (uint32_t i0 = 0; i0 < v.len; i0 += 64) {  // (wave-uniform)
        const uint32_t i = i0 + lane;
        uint64_t key = 0;
        uint32_t row = 0;
        bool hit = false;
        if (i < v.len) {
            key = keys[v.row_off + i];
            row = leaf_ids[(size_t)v.leaf_off + i];
            hit = key <= mk && row < n_rows && frange_owned(vsorted, visitBase, leaf_of, T, t, v.b, row);
        }
        const uint64_t m = __ballot(hit);
        if (!m) continue;  // (wave-uniform)
        if (lane == 0) atomicAdd(&cnt[v.b], (uint32_t)__popcll(m));  // always: the count stays exact when the pool is full
        const unsigned long long slot = wave_slots(ctr, m, lane);
        if (hit && slot < cap) {
            pv[slot] = ((uint64_t)v.b << 32) | row;
            pk[slot] = key;
        }
    }
}

hipError_t zh_launch_frange_collect(const ZhVisit *dVisits, uint64_t n_visits, const uint64_t *dKeys, const uint32_t *dLeafIds, uint64_t n_rows,
                                    const uint32_t *dNodeTree, const uint64_t *dVSorted, const uint64_t *dVisitBase, const uint32_t *dLeafOf, uint32_t T,
                                    const uint64_t *dMaxKeys, uint32_t *dCnt, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                    hipStream_t s) {
    if (!n_visits) return hipSuccess;
    hipLaunchKernelGGL(frange_collect_kernel, dim3((uint32_t)((n_visits + 3) / 4)), dim3(256), 0, s, dVisits, n_visits, dKeys, dLeafIds, n_rows, dNodeTree,
                       dVSorted, dVisitBase, dLeafOf, T, dMaxKeys, dCnt, dHitCtr, dPoolV, dPoolK, pool_cap);
    return hipGetLastError();
}

// ---- path 2 ----
// The launch geometry of a batch of leaves (the host's, frange_leaves2 in zh_api.hip): leaf sg of rt row tiles and vt = ceil(visitors / 16) column
// tiles gives ceil(rt / 4) * ceil(vt / ch) blocks from first_block on; block k of them holds row tiles 4 (k / nch) .. + 3 and walks column tiles
// [ch (k % nch), ...) cut at vt, nch = ceil(vt / ch).  Block x finds its leaf by binary search over the first blocks.  No LDS and no barrier: a wave
// past the leaf's last row tile leaves at once.
template <int D, int KINDA>
__global__ __launch_bounds__(256) void frange_mfma_kernel(const ZhFrangeSeg *__restrict__ segs, uint32_t n_segs, uint32_t ch, uint32_t G,
                                                          const u32x4 *__restrict__ CA, const float2 *__restrict__ cmeta, const uint32_t *__restrict__ crow,
                                                          const ZhGroup *__restrict__ groups, const u32x4 *__restrict__ Qh, const float4 *__restrict__ qmeta,
                                                          float Kc, float rho, const uint32_t *__restrict__ tau, const uint64_t *__restrict__ vsorted,
                                                          const uint64_t *__restrict__ visitBase, const uint32_t *__restrict__ leaf_of, uint32_t T,
                                                          uint64_t *__restrict__ cand, uint64_t cap, unsigned long long *__restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63, c16 = lane & 15, h = lane >> 4;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const ZhFrangeSeg sg = segs[last_le(n_segs, blockIdx.x, [&](uint32_t i) { return segs[i].first_block; })];  // the block's leaf (block-uniform)
    const uint32_t vt = (sg.visitors + 15) / 16, nch = (vt + ch - 1) / ch, k = blockIdx.x - sg.first_block;
    const uint32_t rtile = 4 * (k / nch) + wid;
    if (rtile >= sg.rt) return;  // (wave-uniform)
    const uint32_t Jb = (k % nch) * ch, Je = Jb + ch < vt ? Jb + ch : vt;
    const uint32_t I = sg.col0 + rtile;
    f16x8 A[D / 32];
    tile_load<D>(A, CA, (size_t)I, lane);
    // this lane's outputs: rows 4 h + i of the tile (register i), column c16 = visitor 16 J + c16
    uint32_t id[4];
    float2 meta[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t p = I * 16 + 4 * h + i;
        id[i] = crow[p];
        meta[i] = id[i] != 0xFFFFFFFFu ? cmeta[p] : make_float2(0.f, 0.f);
    }
    for (uint32_t J = Jb; J < Je; J++) {
        const uint32_t j = J * 16 + c16;
        const bool col = j < sg.visitors;
        const uint32_t jj = col ? j : sg.visitors - 1;  // (a padding column repeats the leaf's last visitor and passes nothing)
        const uint32_t b = groups[sg.group0 + jj / G].b[jj % G];
        const u32x4 *qp = Qh + (size_t)b * (D / 8) + h;  // step st: piece 4 st + h of the query (qhalf layout 1 = the A operand's k order)
        const TileSums tt = tile_dot<D / 32, 4>(A, qp);
        const float4 qm = qmeta[b];
        const uint32_t tq = tau[b];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            bool pass = false;
            if (col && id[i] != 0xFFFFFFFFu) pass = (uint32_t)approx_interval<KINDA>(tt[i] * meta[i].y, meta[i].x, qm, Kc, rho, 0.f) <= tq;
            if (!__ballot(pass)) continue;  // (wave-uniform)
            if (pass) pass = frange_owned(vsorted, visitBase, leaf_of, T, sg.tree, b, id[i]);
            pool_push(ctr, cand, cap, pass, ((uint64_t)b << 32) | id[i], lane);
        }
    }
}

hipError_t zh_launch_frange_mfma(uint32_t d, int metric, int mode, const ZhFrangeSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, uint32_t ch, uint32_t group,
                                 const void *dCA, const float2 *dCMeta, const uint32_t *dCRow, const ZhGroup *dGroups, const void *dQh, const float4 *dQmeta,
                                 float Kc, float rho, const uint32_t *dTau, const uint64_t *dVSorted, const uint64_t *dVisitBase, const uint32_t *dLeafOf,
                                 uint32_t T, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s) {
    if (!n_segs || !n_blocks) return hipSuccess;
    if (!ch || !group) return hipErrorInvalidValue;
    return zh_mfma_dispatch(d, metric, mode, [&](auto D, auto K) {
        hipLaunchKernelGGL((frange_mfma_kernel<D, K>), dim3(n_blocks), dim3(256), 0, s, dSegs, n_segs, ch, group, (const u32x4 *)dCA, dCMeta, dCRow, dGroups,
                           (const u32x4 *)dQh, dQmeta, Kc, rho, dTau, dVSorted, dVisitBase, dLeafOf, T, dCand, cand_cap, dCandCtr);
    });
}

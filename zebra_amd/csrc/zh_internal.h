// zh_internal.h -- shared declarations between the kernel translation units and the C ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zebra_hip.h"

// sets zh_last_error() for the calling thread and returns `code`
int zh_set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// (zh_shard.hip) leaf visits per (query, tree) pair, running mean of the index's batches so far (0 before the first)
double zh_index_visits_per_pair(zh_index *ix);
// (zh_shard.hip) a context whose batch was begun and will never be finished goes back to idle
void zh_search_ctx_abandon(zh_search_ctx *c);
// the caller consumes a batch's outputs in STREAM order, before zh_search_wait has returned (the sharded search enqueues its
// all-gather behind finish): the context then never takes a path that may redo the batch from the host (the prefilter)
void zh_search_ctx_stream_ordered(zh_search_ctx *c);

// ---- one leaf visit of the walk (tree_result, lsh.rs:290-348): score `len` rows of a leaf for
// query `b`, keep the `take` smallest.  row_off / cand_off are the visit's slices of the key
// scratch and of the candidate pool.
struct ZhVisit {
    uint32_t b;
    uint32_t leaf_off;  // offset into leaf_ids
    uint32_t len;
    uint32_t take;      // min(n, len)
    uint64_t row_off;
    uint64_t cand_off;
    uint32_t node;      // the leaf's node index
    uint32_t pad;
};

// Visits of one leaf by different queries of the batch (or window) are swept together, `group` at a time (zh_group_size):
// the leaf's rows cross HBM once per group instead of once per query.
#define ZH_GROUP_MAX 4
struct ZhGroup {
    uint32_t leaf_off, len, gsize;
    uint32_t take4;  // byte j = min(take of member j, 255) (join_group)
    uint32_t b[ZH_GROUP_MAX];
    uint64_t key_off[ZH_GROUP_MAX];  // the member visits' row_off (slice of the key scratch)
};
// 4 queries per group (2 measured no better, profiles/r02_ab_sweep128.txt); the sweep kernels take groups of up to 4.
uint32_t zh_group_size(uint32_t dim);

// per (query, tree) pair counts produced by the walk's first pass, then their exclusive scans
struct ZhPairCounts {
    uint32_t visits, rows, takes, pad;
};
struct ZhTotals {
    uint64_t visits, rows, takes, flags;  // flags bit 0: the visit log overflowed (the emit walk must run)
    uint64_t groups, group_rows;  // filled by the leaf scan
    unsigned long long hash_fixups;  // signs the row-score hash (zh_score.hip) recomputed exactly
};

// Visit log of the walk's (single) pass: a pair's visits beyond the ZH_INLINE_VISITS inline ones are appended as
// {leaf node, take} to 512-byte chunks handed out by a bump allocator; entry 0 of a chunk is {next chunk, unused}.
#define ZH_LOG_CHUNK 64
struct ZhLogCtl {
    uint32_t next_chunk, overflow;
};
struct ZhWalkLog {
    uint2 *pool;          // capacity * ZH_LOG_CHUNK entries
    uint32_t capacity;    // chunks
    uint32_t *head;       // first chunk of every pair (valid when the pair has more than ZH_INLINE_VISITS visits)
    ZhLogCtl *ctl;
    uint32_t leaf_entries;  // 1: entries are {offset into leaf_ids, take | length << 16} (a prefiltered batch: its reader needs no node record)
};

// Blocked view of the forest for walks that find every sign precomputed (ZH_BLOCK_NODES, zh_api.hip build_blocks): every
// maximal subtree of at most ZH_BLOCK_NODES nodes is one BLOCK, its nodes stored contiguously in pre-order as 16-byte
// records {plane | -1, inner: left_local | right_local << 16 / leaf: offset into leaf_ids, inner: nodes in the block (root
// record only) / leaf: length, global node id}.  The nodes above the blocks ("upper" nodes, all inner, numbered densely)
// keep two 16-byte records: {plane, left ref, right ref, 0} and {plane of the left child, plane of the right child, 0, 0}
// -- a child's sign can be requested together with its record.  A ref is >= 0 for an upper node and -(offset of the
// block's first record + 1) for a block: no directory lookup between a ref and its data.
#define ZH_BLOCK_NODES 64
// Round 5 (inner_only): a block = a maximal subtree of at most ZH_BLOCK_INNER INNER nodes, one 32-byte record (two int4) per inner node in
// pre-order; its leaves live in their parent's record (zh_api.hip build_blocks_inner); a ref is -(index of the block's first 32-byte record + 1).
#define ZH_BLOCK_INNER 63
struct ZhBlocksDev {
    const int4 *recs;           // all blocks' node records (+ ZH_BLOCK_NODES records of padding: a wave always loads 64)
    const int4 *upper;          // 2 records per upper node
    const int2 *root;           // per tree: {ref, plane of the root when it is an upper node}
    uint32_t n_blocks, n_upper;
    uint32_t inner_only;        // 1: the round-5 records
    const int4 *recs_b;         // ... their second halves (same indices as recs)
};

struct ZhForestDev {
    const int32_t *node_plane, *node_left, *node_right;
    // one 16-byte record per node for the walk: {plane, left, right, bits of the plane's constant} for an internal node,
    // {-1, leaf offset, leaf length, 0} for a leaf -- one dependent load per step instead of four
    const int4 *node_pack;
    const uint32_t *roots;
    const float *planes, *consts;
    const uint32_t *leaf_ids;
    uint32_t n_nodes, n_planes, n_trees;
    uint32_t group;  // queries per sweep group (zh_group_size)
};

#if defined(__HIPCC__)
// point_is_above's dot product: sequential k-ascending fma chain from +0 (the order contract of the hash);
// loads are issued 16 at a time ahead of the chain
__device__ __forceinline__ bool zh_plane_above(const float *__restrict__ w, float c, const float *__restrict__ x,
                                               uint32_t d) {
    float acc = 0.0f;
    if ((d & 3u) == 0) {
        const float4 *w4 = reinterpret_cast<const float4 *>(w);
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        const uint32_t n4 = d / 4;
        uint32_t k = 0;
        for (; k + 8 <= n4; k += 8) {
            float4 a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { a[u] = w4[k + u]; b[u] = x4[k + u]; }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                acc = __builtin_fmaf(a[u].x, b[u].x, acc);
                acc = __builtin_fmaf(a[u].y, b[u].y, acc);
                acc = __builtin_fmaf(a[u].z, b[u].z, acc);
                acc = __builtin_fmaf(a[u].w, b[u].w, acc);
            }
        }
        for (; k < n4; k++) {
            float4 a = w4[k], b = x4[k];
            acc = __builtin_fmaf(a.x, b.x, acc);
            acc = __builtin_fmaf(a.y, b.y, acc);
            acc = __builtin_fmaf(a.z, b.z, acc);
            acc = __builtin_fmaf(a.w, b.w, acc);
        }
    } else {
        for (uint32_t k = 0; k < d; k++) acc = __builtin_fmaf(w[k], x[k], acc);
    }
    return ((double)acc + (double)c) >= 0.0;  // lsh.rs:40-42; NaN -> false
}
#endif

#define ZH_INLINE_VISITS 32    // visits a pair may record in the walk's first pass

// ---- launchers (zh_search.hip) ---------------------------------------------------------------
hipError_t zh_launch_hash_dense(const float *dQ, uint32_t B, const float *dPlanes, const float *dConsts,
                                uint32_t P, uint32_t d, uint32_t *dBits, uint32_t words_per_q, float *dDots,
                                hipStream_t s);
hipError_t zh_launch_qnorm(const float *dQ, uint32_t B, uint32_t d, float *dQQ, hipStream_t s);
hipError_t zh_launch_walk_count(ZhForestDev f, const float *dQ, uint32_t B, uint32_t d, int32_t n,
                                const uint32_t *dBits, uint32_t words_per_q, uint32_t P_dense, ZhPairCounts *dCounts,
                                ZhVisit *dInline, uint32_t *dLeafCount, ZhWalkLog log, hipStream_t s);
// the counting pass for all-dense signs over the blocked forest: one memory round trip per BLOCK instead of per node
hipError_t zh_launch_walk_blocked(ZhForestDev f, ZhBlocksDev blk, uint32_t B, int32_t n, const uint32_t *dBits,
                                  uint32_t words_per_q, ZhPairCounts *dCounts, ZhVisit *dInline, uint32_t *dLeafCount,
                                  ZhWalkLog log, const uint32_t *dUnc /* null, or the row-score hash's flagged signs */, const float *dQ,
                                  uint32_t d, hipStream_t s);
// places every visit recorded by the counting pass (inline + log) and joins the leaf groups: the cheap, flat
// replacement of the emit walk whenever the log did not overflow
hipError_t zh_launch_expand(ZhForestDev f, uint32_t B, const ZhPairCounts *dCounts, const ZhVisit *dInline,
                            const uint64_t *dRowBase, const uint64_t *dCandBase, const uint64_t *dVisitBase,
                            ZhVisit *dVisits, const uint32_t *dLeafCount, uint32_t *dLeafFill,
                            const uint32_t *dGroupBase, const uint64_t *dGroupRowBase, ZhGroup *dGroups,
                            uint64_t *dGroupRowOff, ZhWalkLog log, hipStream_t s);
// zeroes what a batch starts from zero: leaf visit counts / fill cursors, the log allocator, the packed leaf counter
hipError_t zh_launch_batch_init(uint32_t *dLeafCount, uint32_t *dLeafFill, uint32_t n_nodes, ZhLogCtl *dLogCtl,
                                ZhTotals *dTotals, hipStream_t s);
// per leaf node: visits -> groups; exclusive scans of groups and of groups * len over the nodes
hipError_t zh_launch_leaf_scan(ZhForestDev f, const uint32_t *dLeafCount, uint32_t *dGroupBase,
                               uint64_t *dGroupRowBase, ZhTotals *dTotals, hipStream_t s);
// exclusive scans over the pairs; the three base arrays have n_pairs + 1 entries
hipError_t zh_launch_pair_scan(const ZhPairCounts *dCounts, uint32_t n_pairs, uint64_t *dRowBase,
                               uint64_t *dCandBase, uint64_t *dVisitBase, ZhTotals *dTotals, const ZhLogCtl *dLogCtl,
                               hipStream_t s);
hipError_t zh_launch_walk_emit(ZhForestDev f, const float *dQ, uint32_t B, uint32_t d, int32_t n,
                               const uint32_t *dBits, uint32_t words_per_q, uint32_t P_dense,
                               const ZhPairCounts *dCounts, const ZhVisit *dInline, const uint64_t *dRowBase,
                               const uint64_t *dCandBase, const uint64_t *dVisitBase, ZhVisit *dVisits,
                               const uint32_t *dLeafCount, uint32_t *dLeafFill, const uint32_t *dGroupBase,
                               const uint64_t *dGroupRowBase, ZhGroup *dGroups, uint64_t *dGroupRowOff, hipStream_t s);
// dWaveGroup: the wave-start table of zh_launch_wave_groups (ceil(R_grouped / 64) entries), or nullptr
hipError_t zh_launch_sweep(const float *dX, uint32_t d, const float *dQ, const float *dQQ, const ZhGroup *dGroups,
                           const uint64_t *dGroupRowOff, uint64_t n_groups, const uint32_t *dWaveGroup,
                           const uint32_t *dLeafIds, uint64_t R_grouped, int metric, int mode, uint64_t *dKeys,
                           hipStream_t s, const uint32_t *dRunIf = nullptr);
bool zh_sweep_has_predicate(uint32_t d, int metric);
// waveGroup[w] = group of flat row 64 w, for every wave start of [0, R_grouped)
hipError_t zh_launch_wave_groups(const ZhGroup *dGroups, const uint64_t *dGroupRowOff, uint64_t n_groups, uint32_t *dWaveGroup,
                                 hipStream_t s);
// ---- the table-scan sweep (zh_search.hip): the stored rows streamed once, each scored against every query that visits
// one of its leaves.  rowLeaf is n_rows x T {leaf node, position in the leaf}, built per forest by zh_launch_row_leaf from
// node_pack, a node -> tree map (UINT32_MAX for nodes no root reaches) and leaf_ids.
#define ZH_SCAN_NE 4     // (row, tree) entries per lane of a table-scan wave: RW * T <= 64 * ZH_SCAN_NE
bool zh_scan_sweep_supported(uint32_t d, uint32_t T, int metric);
uint32_t zh_scan_rows_per_wave(uint32_t T);
hipError_t zh_launch_row_leaf(const int4 *dNodePack, const uint32_t *dNodeTree, uint32_t n_nodes, const uint32_t *dLeafIds,
                              uint32_t T, uint64_t n_rows, uint2 *dRowLeaf, hipStream_t s);
// per batch (after the groups are filled): bit n of dBits = leaf node n is visited; dNodeVisit[n] = {visits, first group, query and
// key slice of the first visit} of the visited leaves
hipError_t zh_launch_node_visits(const uint32_t *dLeafCount, const uint32_t *dGroupBase, const ZhGroup *dGroups, uint32_t n_nodes,
                                 uint32_t *dBits, uint4 *dNodeVisit, hipStream_t s);
hipError_t zh_launch_scan_sweep(const float *dX, uint32_t d, uint64_t n_rows, const float *dQ, const float *dQQ,
                                const uint2 *dRowLeaf, uint32_t T, const uint32_t *dVisitBits, const uint4 *dNodeVisit,
                                const ZhGroup *dGroups, uint32_t group, int metric, int param, uint64_t *dKeys,
                                const uint32_t *dRunIf /* null, or: run only when this device word is nonzero */, hipStream_t s);
// flat rows covered by one sweep launch (a batch is issued as ceil(R / this) launches)
uint64_t zh_sweep_rows_per_launch(uint32_t d);
// max_leaf_len: the longest leaf of the forest (picks the LDS footprint of the select blocks)
hipError_t zh_launch_select(const ZhVisit *dVisits, uint64_t n_visits, const uint32_t *dLeafIds,
                            const uint64_t *dKeys, uint64_t *dCandKeys, uint32_t *dCandIds, uint32_t max_leaf_len,
                            const uint32_t *dRunIf, hipStream_t s);
hipError_t zh_launch_final(const uint64_t *dCandBase, uint32_t B, uint32_t T, uint32_t k, const uint64_t *dCandKeys,
                           const uint32_t *dCandIds, uint64_t id_base, uint64_t *dOutIds, uint64_t *dOutKeys,
                           uint32_t *dOutCounts, const uint32_t *dRunIf, hipStream_t s);
// stride64 / stride32: distance between consecutive shards' ids (= keys) in u64 units and counts in u32 units
// (0 = contiguous [S][B][k] / [S][B])
hipError_t zh_launch_merge(uint32_t S, uint32_t B, uint32_t k, const uint64_t *dIds, const uint64_t *dKeys,
                           const uint32_t *dCounts, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts,
                           uint64_t stride64, uint64_t stride32, hipStream_t s);
// plain distance of n contiguous rows against one query (zh_distance_batch)
#define ZH_DISTANCE_SCRATCH_BYTES (sizeof(ZhGroup) + 16)
hipError_t zh_launch_distance_rows(const float *dX, uint64_t n, uint32_t d, const float *dq, int metric, int mode,
                                   uint64_t *dKeys, void *dScratch, hipStream_t s);

// ---- the table scan with half-width queries (zh_approx.inl): intervals instead of keys, exact keys for the few rows they cannot
// decide.  ctl[0] = visits sent to the exact path, ctl[1] = overflow bits (1 a query's candidate list, 2 a query's survivors,
// 4 the table of exact visits, 8 the exact visits' key scratch) -- nonzero: the exact scan + select + final enqueued behind
// redo the batch (their predicate), ctl[2] = key scratch handed out, ctl[3] = survivors scored exactly, ctl[4] = list entries,
// ctl[5] / ctl[6] = tile columns / pairs of the matrix-core scan's listed waves (a column per distinct query: how much the pairs share).
#define ZH_APX_CTL_WORDS 8
struct ZhApprox {
    const void *Qh;          // the fp16 copy of the batch's queries (2 * d bytes each, qhalf_kernel's layout)
    const float4 *qmeta;     // per query {1 / sigma, |q|^2, upper estimate of |q|, upper estimate of |q - h / sigma|}
    uint64_t *iv;            // per (row, query) pair, in the pair's key slot: from the scan {x . h, |x|^2} (f32 bits); select_tau_kernel
                             // turns a visit's entries into sortable lo | sortable hi << 32 in place
    uint32_t *list_lo, *list_hi, *list_id;  // per query: capq slots
    uint32_t *qcount;
    uint32_t capq;
    uint32_t *tauv;          // per visit: the take-th smallest hi (sortable) of a visit that takes top_k rows of a longer leaf
    uint32_t *qtau;          // per query: the smallest of them -- top_k candidates of the query have keys at or below it
    uint2 *ex_visits;        // the visits for the exact path: {index, their slice of the key scratch}
    uint32_t ex_cap;
    uint64_t *ex_keys, *ex_ckeys;  // their rows' canonical keys; the `take` chosen
    uint32_t *ex_cids;
    uint32_t ex_rows_cap;
    uint32_t *ctl;
    // the scan on the matrix cores (scan_mfma_kernel): the stored rows are rounded to fp16 as well
    const void *row_half;    // the fp16 copy of the stored rows, tiles of 16 rows in the A operand's order (row_half_kernel)
    const float2 *row_meta;  // per stored row {|x|^2, 1 / sigma_x (NaN: nothing certain about the row)}
    float row_rho;           // |x - xh / sigma_x| <= row_rho |x| for every usable stored row (0 with f32 rows)
    float rho_norm;          // = row_rho where |x|^2 itself comes from the rounded row (sweep128h_kernel), else 0
    uint32_t mfma;           // zh_approx_bound's kind: 0 VALU scans, 1 scan_mfma_kernel, 2 sweep128h_kernel
    uint32_t n_queries;      // queries of the internal batch, entries of iv (diagnostic builds check every index against them: -DZH_SCAN_GUARD)
    uint64_t iv_cap;
    float nx_max;            // > 0: no stored row's norm estimate (approx_interval's nx) exceeds it -- the byte copy: sqrt(128) * 255 (fused sweep's pre-test)
};
uint32_t zh_approx_groups(uint32_t d);
bool zh_approx_pays(uint32_t d);
float zh_approx_bound(int metric, uint32_t d, int mfma);
bool zh_scan_mfma_supported(uint32_t d, uint32_t T);
// the fp16 copy of rows [row0, row0 + n_rows) in scan_mfma_kernel's operand order (2 * d bytes per row, tiles of 16 rows), per row {|x|^2,
// 1 / sigma_x}; *dRhoMax = the largest relative rounding error of a row (f32 bits, atomicMax)
hipError_t zh_launch_row_half(const float *dX, uint64_t row0, uint64_t n_rows, uint32_t d, void *dXh, float2 *dRowMeta, uint32_t *dRhoMax,
                              const uint32_t *dPerm /* null, or: position p < perm_rows holds row dPerm[p] */, uint64_t perm_rows, hipStream_t s);
// the matrix-core scan's row order: the permutation (zh_order.hip) and the row -> leaf table gathered into it
// (zh_order.hip) dPerm[p] = the row at position p of the order (leaf in tree 0, leaf in tree 1[, leaf in tree 2], row id); synchronises the stream
hipError_t zh_launch_scan_order(const uint2 *dRowLeaf, uint64_t n_rows, uint32_t T, uint32_t n_keys, uint32_t *dPerm, hipStream_t s);
// ... and what an order is worth: (adjacent positions, tree) combinations in the same leaf (dPerm null: id order)
hipError_t zh_launch_order_agreement(const uint2 *dRowLeaf, const uint32_t *dPerm, uint64_t n_rows, uint32_t T, unsigned long long *dOut, hipStream_t s);
hipError_t zh_launch_permute_row_leaf(const uint2 *dRowLeaf, const uint32_t *dPerm, uint64_t perm_rows, uint64_t n_rows, uint32_t T, uint2 *dOut, hipStream_t s);
bool zh_scan_approx_supported(uint32_t d, uint32_t T, int metric);
hipError_t zh_launch_qhalf(const float *dQ, uint32_t B, uint32_t d, void *dQh, float4 *dQmeta, int layout, hipStream_t s);
// d = 128, leaf by leaf at half width (sweep128h_kernel): the table's common scale from its largest finite element, the row-major fp16 copy, the sweep
hipError_t zh_launch_absmax(const float *dX, uint64_t n, uint32_t *dOut, hipStream_t s);
hipError_t zh_launch_row_half128(const float *dX, uint64_t row0, uint64_t n_rows, float sigma, void *dXh, uint32_t *dRhoMax, hipStream_t s);
hipError_t zh_launch_sweep128h(const void *dXh, const void *dQh, float inv, const ZhGroup *dGroups, const uint64_t *dGroupRowOff, uint64_t n_groups,
                               const uint32_t *dWaveGroup, const uint32_t *dLeafIds, uint64_t R_grouped, uint64_t *dIv, hipStream_t s,
                               const ZhApprox *fuse = nullptr, int fuse_kinda = 0, uint32_t k_top = 0, float Kc = 0.f, bool byte_rows = false);
// ... and of a table whose every element is an integer in 0 .. 255 (SIFT descriptors): an EXACT copy of 128 bytes per row (*dNotBytes |= 1 when an
// element of rows row0 .. is anything else: the copy is then void); byte_rows above = dXh is that copy (the lean kernels only)
uint64_t zh_sweep128h_rows_per_launch(bool lean, bool byte_rows);  // stored rows one launch of the sweep takes (the host's launch accounting)
hipError_t zh_launch_row_byte128(const float *dX, uint64_t row0, uint64_t n_rows, void *dXb, uint32_t *dNotBytes, hipStream_t s);
// (fused sweep) the exact path's visits, as select_tau_kernel lists them
hipError_t zh_launch_exact_register(const ZhVisit *dVisits, uint64_t n_visits, uint32_t k, ZhApprox ap, hipStream_t s);
hipError_t zh_launch_scan_approx(const float *dX, uint32_t d, uint64_t n_rows, ZhApprox ap, const uint2 *dRowLeaf, uint32_t T,
                                 const uint32_t *dVisitBits, const uint4 *dNodeVisit, const ZhGroup *dGroups, uint32_t group, int metric,
                                 int mode, hipStream_t s);
hipError_t zh_launch_select_interval(const ZhVisit *dVisits, uint64_t n_visits, uint32_t k, const uint32_t *dLeafIds, ZhApprox ap,
                                     int metric, int mode, uint32_t d, hipStream_t s);
// the exact visits, then per query: duplicates out, tau, the survivors' canonical keys, top_k
hipError_t zh_launch_final_interval(const ZhVisit *dVisits, const float *dX, uint32_t d, const float *dQ, const float *dQQ, uint32_t B,
                                    uint32_t k, const uint32_t *dLeafIds, int metric, int mode, uint64_t id_base, ZhApprox ap,
                                    uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, uint32_t max_leaf_len, hipStream_t s);

// ---- the exact search (zh_exact.hip): keys of every (live row, query) pair of a row chunk, the per-(query, sub-chunk) visits for select /
// final, and the answer of a batch with no live rows
// keys[b * ld + (p - p0)] = key of (stored row dLive[p], query b), p in [p0, p0 + nr)
hipError_t zh_launch_exact_score(const float *dX, uint32_t d, const uint32_t *dLive, uint64_t p0, uint32_t nr, const float *dQ,
                                 const float *dQQ, uint32_t B, int metric, int param, uint64_t *dKeys, uint64_t ld, hipStream_t s);
// visit b * nsub + j = positions [p0 + j L, p0 + min((j + 1) L, nr)) for query b, take min(k, len); dCandBase: B * nsub + 1 entries
hipError_t zh_launch_exact_visits(uint32_t B, uint32_t nsub, uint32_t nr, uint32_t L, uint32_t k, uint64_t p0, uint64_t ld, ZhVisit *dVisits,
                                  uint64_t *dCandBase, hipStream_t s);
// path 2 (L2SQ, L2, cosine at d = 256 .. 1024): the matrix-core scan's view of one internal batch -- the index's fp16 row copy, the queries' fp16 copy,
// and per query tau (sortable f32, starts at ~0), a list of cap (row, lo, hi) entries and its count; *over != 0: a list ran over (path 1 answers)
struct ZhExact2 {
    const void *Xh; const float2 *rowMeta; const uint32_t *perm; uint64_t perm_rows; const uint32_t *liveBits;
    const void *Qh; const float4 *qmeta; uint32_t B; float Kc, rho;
    uint32_t *tau, *cnt, *lid, *llo, *lhi; uint32_t cap; uint32_t *over;
};
bool zh_exact_mfma_supported(uint32_t d, int metric);
// filtered (zh_search_exact_filtered_batch): e.liveBits is the allowed-and-live bitmap BY POSITION (zh_launch_filter_permute under a row order), a
// wave whose 16 positions are all masked returns before it loads its tile and counts itself in e.over[1]
hipError_t zh_launch_exact_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, uint64_t p_begin, uint64_t p_end, hipStream_t s,
                                bool filtered = false);
// dScratch: 3 * B * cap words
hipError_t zh_launch_exact_prune(const ZhExact2 &e, uint32_t k, uint32_t *dScratch, hipStream_t s);
hipError_t zh_launch_exact_survivor_keys(const float *dX, uint32_t d, const float *dQ, const float *dQQ, int metric, int mode, const ZhExact2 &e,
                                         uint64_t *dCKeys, uint32_t *dCIds, hipStream_t s);
hipError_t zh_launch_exact_empty(uint32_t B, uint32_t k, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s);

// ---- the filter pass of the filtered exact search (zh_filter.hip).  Bitmaps: bit r % 32 of word r / 32; n_blocks = ceil(n_rows / ZH_FILTER_BLOCK_ROWS);
// dBlockCount: n_blocks entries, dBlockExcl: n_blocks + 1 (the last one the total), dScanTmp: n_blocks / 1024 + 2; *dTiles = 16-row tiles (of
// rows, or of positions) that hold a set bit
#define ZH_FILTER_BLOCK_ROWS 8192u
// dOut = dFilter (n_bits bits, rows past them not allowed; may be null for n_bits = 0) AND dLiveBits, ceil(n_rows / 32) words
hipError_t zh_launch_filter_and(const uint32_t *dFilter, uint64_t n_bits, const uint32_t *dLiveBits, uint64_t n_rows, uint32_t *dOut,
                                uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp, uint32_t *dTiles, hipStream_t s);
// bit p of dOut = bit (p < perm_rows ? dPerm[p] : p) of dBits; dOut: 8-byte aligned, ceil(n_rows / 64) * 2 words
hipError_t zh_launch_filter_permute(const uint32_t *dBits, const uint32_t *dPerm, uint64_t perm_rows, uint64_t n_rows, uint32_t *dOut,
                                    uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp, uint32_t *dTiles, hipStream_t s);
// dList = the set bits of dBits, ascending (dBlockExcl as zh_launch_filter_and left it)
hipError_t zh_launch_filter_list(const uint32_t *dBits, uint64_t n_rows, const uint32_t *dBlockExcl, uint32_t *dList, hipStream_t s);

// ---- the exact range search (zh_range.hip): every live row with key <= a per-query threshold key.  A hit pool is two u64 arrays, v = query << 32 | row
// and the key; dCnt: the hits per query of the internal batch, counted whether or not the pool has room; *dHitCtr: all of them
hipError_t zh_launch_range_collect(const uint64_t *dKeys, uint64_t ld, const uint32_t *dLive, uint64_t p0, uint32_t nr, uint32_t B,
                                   const uint64_t *dMaxKeys, uint32_t *dCnt, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK,
                                   uint64_t pool_cap, hipStream_t s);
// path 2: dTau[b] = the threshold key of query b in approx_interval's sortable-f32 domain, rounded towards admitting more
hipError_t zh_launch_range_tau(const uint64_t *dMaxKeys, uint32_t B, int metric, int mode, uint32_t *dTau, hipStream_t s);
// exact_mfma_kernel's scan against e.tau (fixed); pairs with lo <= tau to dCand as query << 32 | row; *dCandCtr counts all of them (> cand_cap: ran over).
// Of e it reads Xh, rowMeta, perm, perm_rows, liveBits, Qh, qmeta, B, Kc, rho, tau.
hipError_t zh_launch_range_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, uint64_t p_begin, uint64_t p_end, uint64_t *dCand, uint64_t cand_cap,
                                unsigned long long *dCandCtr, hipStream_t s);
// the candidates' canonical keys, judged against the thresholds, counted and appended to the hit pool (nothing when the candidate pool ran over)
hipError_t zh_launch_range_survivors(const float *dX, uint32_t d, const float *dQ, const float *dQQ, int metric, int mode, const uint64_t *dCand,
                                     const unsigned long long *dCandCtr, uint64_t cand_cap, const uint64_t *dMaxKeys, uint32_t *dCnt,
                                     unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s);
// dOff[i] = base + hits of the queries before i, i <= B (B <= 1024)
hipError_t zh_launch_range_offsets(const uint32_t *dCnt, uint32_t B, uint64_t base, uint64_t *dOff, hipStream_t s);
// every pool's order: n entries of (v, k) by (the high field of v, k, the low field of v), the fields holding hi_values / lo_values values; skip_high
// leaves the last of the three passes out.  dV / dK: the pool and a second buffer of the same size each; *v_out / *k_out = where the result is.
// dTmp == nullptr: only *tmp_bytes is set, to what the sorts of n entries need
hipError_t zh_launch_pool_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t lo_values, uint64_t hi_values, bool skip_high, void *dTmp,
                               size_t *tmp_bytes, const uint64_t **v_out, const uint64_t **k_out, hipStream_t s);
// ... of the pool of an internal batch, by (query, key, row), written out as ids (id_base + row) and keys; dTmp == nullptr as above
hipError_t zh_launch_range_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t n_rows, uint32_t B, void *dTmp, size_t *tmp_bytes, uint64_t id_base,
                                uint64_t *dOutIds, uint64_t *dOutKeys, hipStream_t s);

// ---- the exact self-join (zh_join.hip): every pair of live rows a < b with key(stored b, query a) <= one threshold key.  A hit pool is two u64
// arrays, v = a << 32 | b (row numbers) and the key; *dHitCtr counts every hit whether or not the pool has room.  The launchers named `pair` serve
// the join between two indexes and the forest join too: two tables, row counts and id bases, which the self-join passes as the same one twice
#define ZH_JOIN_CHUNK 64u          // tiles J one block of the matrix-core scan walks
#define ZH_JOIN_PANEL_ROWS 16384u  // positions of the copy one launch holds (256 blocks of four tiles); a panel is the unit path 1 redoes
// path 1: dQ[b] = the f32 row dRows[b]
hipError_t zh_launch_join_gather(const float *dX, uint32_t d, const uint32_t *dRows, uint32_t B, float *dQ, hipStream_t s);
// ... and of the keys [b][p - p0] (zh_launch_exact_score) those <= max_key -- upper: whose row dLive[p] is above the query row dQRows[b] (the
// self-join); otherwise all of them (the full rectangle of two indexes)
hipError_t zh_launch_pair_collect(const uint64_t *dKeys, uint64_t ld, const uint32_t *dLive, uint64_t p0, uint32_t nr, const uint32_t *dQRows, uint32_t B,
                                  bool upper, uint64_t max_key, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                  hipStream_t s);
// path 2: per position of the fp16 copy (ceil(n_rows / 16) * 16 of them) dQm = the row as approx_interval's query, dCid = its row number or
// UINT32_MAX (removed, or past the table)
hipError_t zh_launch_join_prep(const float2 *dRowMeta, const uint32_t *dPerm, uint64_t perm_rows, const uint32_t *dLiveBits, uint64_t n_rows, float rho,
                               float4 *dQm, uint32_t *dCid, hipStream_t s);
// the blocks of a panel of held tiles [tileA0, tileA1) of T: first[ab] = blocks before held block ab (n_ab + 1 entries, caller's array); returns the
// 16 x 16 tile products the panel issues
uint64_t zh_join_geometry(uint64_t T, uint64_t tileA0, uint64_t tileA1, uint32_t *first);
// the scan of one panel against *dTau (zh_launch_range_tau of the one threshold); pairs with lo <= tau to dCand as min(row) << 32 | max(row);
// *dCandCtr counts all of them (> cand_cap: ran over)
hipError_t zh_launch_join_mfma(uint32_t d, int metric, int mode, const void *dXh, const float2 *dRowMeta, const float4 *dQm, const uint32_t *dCid,
                               uint64_t n_rows, uint64_t tileA0, const uint32_t *dFirst, uint32_t n_ab, uint32_t blocks, float Kc, float rho,
                               const uint32_t *dTau, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s);
// the candidates' canonical keys (stored row b of dXB, query row a of dXA), judged, counted and appended to the hit pool (nothing when the
// candidate pool ran over).  dLeafOf != nullptr (the forest join, candidates met in tree t): the first-tree rule first; *dKeyed += those that got a key
hipError_t zh_launch_pair_survivors(const float *dXA, const float *dXB, uint32_t d, int metric, int mode, const uint64_t *dCand,
                                    const unsigned long long *dCandCtr, uint64_t cand_cap, const uint32_t *dLeafOf, uint32_t T, uint32_t t, uint64_t max_key,
                                    unsigned long long *dHitCtr, unsigned long long *dKeyed, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                    hipStream_t s);
// dList = the live rows at positions [p_begin, p_end), any order; *dCount += their number
hipError_t zh_launch_join_panel_rows(const uint32_t *dCid, uint64_t p_begin, uint64_t p_end, uint32_t *dList, unsigned long long *dCount, hipStream_t s);
// the pool's n entries ordered by (a, key, b) and written out as ids (each side's id base + row) and keys; n_rows_a / n_rows_b: the row numbers the
// two fields of v hold.  dV / dK, dTmp == nullptr: as zh_launch_pool_sort
hipError_t zh_launch_pair_sort(uint64_t *dV[2], uint64_t *dK[2], uint64_t n, uint64_t n_rows_a, uint64_t n_rows_b, void *dTmp, size_t *tmp_bytes,
                               uint64_t id_base_a, uint64_t id_base_b, uint64_t *dOutA, uint64_t *dOutB, uint64_t *dOutKeys, hipStream_t s);

// ---- the exact join between two indexes (zh_xjoin.hip): every pair (live row a of A, live row b of B) with key(stored b, query a) <= one threshold
// key.  Hit pool, counter and their launchers are the self-join's, v = a << 32 | b with a a row number of A and b one of B
// path 2: the launch of a panel of held tiles [tileA0, min(tileA1, TA)) of A's copy against all TB tiles of B's: *n_ab held blocks of four tiles,
// *blocks = n_ab * ceil(TB / ZH_JOIN_CHUNK); returns the 16 x 16 tile products the panel issues
uint64_t zh_xjoin_geometry(uint64_t TA, uint64_t TB, uint64_t tileA0, uint64_t tileA1, uint32_t *n_ab, uint32_t *blocks);
// the scan of one panel (tileA0 a multiple of 4; tileA1 one too, or past A's last tile) against *dTau; dCidA / dCidB, dQmB: zh_launch_join_prep of
// either side; pairs with lo <= tau to dCand as a << 32 | b; *dCandCtr counts all of them (> cand_cap: ran over)
hipError_t zh_launch_xjoin_mfma(uint32_t d, int metric, int mode, const void *dXhA, const float2 *dRowMetaA, const uint32_t *dCidA, uint64_t n_rows_a,
                                const void *dXhB, const float4 *dQmB, const uint32_t *dCidB, uint64_t n_rows_b, uint64_t tileA0, uint64_t tileA1, float Kc,
                                float rhoA, const uint32_t *dTau, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s);

// ---- test / debug (zh_walkdbg.hip): the held-tile walk's interval of every pair of held positions [p0, p1) of A's copy (p0 a multiple of 64,
// p1 <= 16 ceil(n_rows_a / 16), at most ZH_DEBUG_WALK_ROWS of them) x all positions of B's; record (p - p0) * 16 ceil(n_rows_b / 16) + column position,
// stored where that is below `cap`.  dCidA / dCidB, dQmB: zh_launch_join_prep of either side
#define ZH_DEBUG_WALK_ROWS 1024u
hipError_t zh_launch_walk_debug(uint32_t d, int metric, int mode, const void *dXhA, const float2 *dRowMetaA, const uint32_t *dCidA, uint64_t n_rows_a,
                                const void *dXhB, const float4 *dQmB, const uint32_t *dCidB, uint64_t n_rows_b, uint64_t p0, uint64_t p1, float Kc, float rhoA,
                                zh_debug_walk_pair *dOut, uint64_t cap, hipStream_t s);

// ---- the exact k-NN graph (zh_knn.hip): each live row's k nearest other live rows, panel by panel
#define ZH_KNN_PANEL_ROWS 1024u  // live rows one panel holds (= the exact search's internal batch: every reused launcher sees a batch it already serves)
#define ZH_KNN_CHUNK 64u         // column tiles one block of the matrix-core scan walks at most
static_assert(ZH_KNN_PANEL_ROWS % 64 == 0, "a held block is four tiles of 16 lines");
// under a row order: dPos[row] = the position of live row `row` (dCid: zh_launch_join_prep's id-or-masked word per position)
hipError_t zh_launch_knn_rowpos(const uint32_t *dCid, uint64_t n_pos, uint32_t *dPos, hipStream_t s);
// the panel's tiles (ceil(B / 16) of them, 32 d bytes each) gathered out of the fp16 copy in the MFMA operand's order, with per line the position's
// rowMeta and the row number (UINT32_MAX past B); dRows: the panel's B live rows; dPos: null in id order
hipError_t zh_launch_knn_panel(uint32_t d, const void *dXh, const float2 *dRowMeta, const uint32_t *dPos, const uint32_t *dRows, uint32_t B, void *dA,
                               float2 *dPMeta, uint32_t *dPid, hipStream_t s);
// column tiles per block of a launch over `tiles` column tiles and n_ab held blocks
uint32_t zh_knn_chunk(uint64_t tiles, uint32_t n_ab);
// the scan of the panel (e.B lines; e.tau / cnt / lid / llo / lhi / cap / over per LINE) against positions [p_begin, p_end) of the copy (e.Xh); self is
// excluded by row number.  Of e it reads Xh, B, Kc, rho and the lists
hipError_t zh_launch_knn_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, const float4 *dQm, const uint32_t *dCid, uint64_t p_begin, uint64_t p_end,
                              const void *dA, const float2 *dPMeta, const uint32_t *dPid, hipStream_t s);
// a panel's answer [B][w] (zh_launch_final's) to the lines' places: line dRows[b] - first_row gets the first k entries that are not its own id
hipError_t zh_launch_knn_emit(const uint64_t *dInIds, const uint64_t *dInKeys, const uint32_t *dInCounts, uint32_t w, const uint32_t *dRows, uint32_t B,
                              uint64_t id_base, uint64_t first_row, uint32_t k, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s);

// ---- the exact k-NN join between two indexes (zh_xknn.hip): each live row of A's k nearest live rows of B, panel by panel of A.  Panels, their
// gather (zh_launch_knn_panel over A's copy), chunks and lists are the graph's
// the scan of the panel (e.B lines of A; the lists per LINE) against positions [p_begin, p_end) of B's copy (e.Xh); dQmB / dCidB: zh_launch_join_prep
// of B; no column is skipped for its number.  Of e it reads Xh (B's copy), B, Kc, rho (A's) and the lists
hipError_t zh_launch_xknn_mfma(uint32_t d, int metric, int mode, const ZhExact2 &e, const float4 *dQmB, const uint32_t *dCidB, uint64_t p_begin, uint64_t p_end,
                               const void *dA, const float2 *dPMeta, const uint32_t *dPid, hipStream_t s);
// a panel's answer [B][k] (zh_launch_final's) to the lines' places: line dRows[b] - first_row gets the first min(count, k) entries as they are
hipError_t zh_launch_xknn_emit(const uint64_t *dInIds, const uint64_t *dInKeys, const uint32_t *dInCounts, const uint32_t *dRows, uint32_t B,
                               uint64_t first_row, uint32_t k, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s);

// ---- the forest k-NN graph (zh_fknn.hip): each row's k nearest rows among its leaf-mates over all trees
#define ZH_FKNN_SLAB 65536u       // lines of a sub-slab: the unit of the row -> leaf table, of path 1 and of a redo
#define ZH_FKNN_HELD_ROWS 4096u   // path 2: members of one leaf a segment holds at most; held lines of a batch (256 tiles)
#define ZH_FKNN_COL_TILES 2048u   // path 2: column tiles a batch gathers (more only for ONE leaf that is longer)
#define ZH_FKNN_CHUNK 64u         // path 2: column tiles one block walks at most
static_assert(ZH_FKNN_HELD_ROWS % 64 == 0, "a held block is four tiles of 16 lines");
// one segment of a path-2 batch: members [held_off, held_off + held_len) of leaf_ids (one leaf's, or a window of them) as candidates for held rows,
// against the whole leaf as columns
struct ZhFknnSeg {
    uint32_t col0, ct;             // the leaf's column tiles in the batch's column scratch
    uint32_t held_off, held_len;   // the window of leaf_ids the held rows come from
    uint32_t line0, held_tiles;    // its lines in the batch: [line0, line0 + 16 * held_tiles), line0 % 16 == 0, held_tiles = ceil(held_len / 16)
    uint32_t first_block, pad;     // blocks of the launch before this segment's ceil(held_tiles / 4) * ceil(ct / ch)
};
// dRl[(r - r0) * T + t] = {offset into leaf_ids, length} of the leaf of row r in tree t, {UINT32_MAX, UINT32_MAX} for none; r in [r0, r0 + m)
hipError_t zh_launch_fknn_rowleaf(const int4 *dNodePack, const uint32_t *dNodeTree, uint32_t n_nodes, const uint32_t *dLeafIds, uint32_t T, uint64_t r0,
                                  uint32_t m, uint2 *dRl, hipStream_t s);
// dRows = the sub-slab's rows that some tree holds, ascending (dExcl[m] = their number; dFlag m, dExcl m + 1, dScanTmp m / 1024 + 2 words);
// *dPairs += the sum over them and over their trees of (leaf length - 1)
hipError_t zh_launch_fknn_lines(const uint2 *dRl, uint32_t T, uint64_t r0, uint32_t m, uint32_t *dFlag, uint32_t *dExcl, uint32_t *dScanTmp, uint32_t *dRows,
                                unsigned long long *dPairs, hipStream_t s);
// path 1: visit b * T + t = line dRows[b]'s leaf in tree t; sizes first (for the two exclusive scans), then the visits, their one-member groups,
// the groups' flat row offsets and the candidate bases (B * T + 1 entries), w = entries a visit takes at most
hipError_t zh_launch_fknn_visit_sizes(const uint2 *dRl, uint32_t T, uint64_t r0, const uint32_t *dRows, uint32_t B, uint32_t w, uint32_t *dLens,
                                      uint32_t *dTakes, hipStream_t s);
hipError_t zh_launch_fknn_visits(const uint2 *dRl, uint32_t T, uint64_t r0, const uint32_t *dRows, uint32_t B, uint32_t w, const uint32_t *dRowBase,
                                 const uint32_t *dCandBase, ZhVisit *dVisits, ZhGroup *dGroups, uint64_t *dGroupRowOff, uint64_t *dCandBase64, hipStream_t s);
// path 2.  dPos[row] = the row's position in the fp16 copy under a row order
hipError_t zh_launch_fknn_rowpos(const uint32_t *dPerm, uint64_t perm_rows, uint64_t n_rows, uint32_t *dPos, hipStream_t s);
// dCRow[16 c + j] = leaf_ids[dSrc[c].x + j] for j < dSrc[c].y, else UINT32_MAX
hipError_t zh_launch_fknn_cols(const uint2 *dSrc, uint32_t n_tiles, const uint32_t *dLeafIds, uint64_t n_rows, uint32_t *dCRow, hipStream_t s);
// per segment its members inside [first_row, first_row + n) as held rows (dHRow, UINT32_MAX past them), dHeld[seg] their number; *dTiles += the
// 16 x 16 tile products its blocks issue
hipError_t zh_launch_fknn_held(const ZhFknnSeg *dSegs, uint32_t n_segs, const uint32_t *dLeafIds, uint64_t first_row, uint64_t n, uint32_t *dHRow,
                               uint32_t *dHeld, unsigned long long *dTiles, hipStream_t s);
// the tiles of a row list (16 n_tiles entries, UINT32_MAX = none) out of the fp16 copy in the MFMA operand's order, their rowMeta, and (dQm not null)
// the rows as approx_interval's queries
hipError_t zh_launch_fknn_gather(uint32_t d, const void *dXh, const float2 *dRowMeta, const uint32_t *dPos, const uint32_t *dRows, uint32_t n_tiles, float rho,
                                 void *dA, float2 *dMeta, float4 *dQm, hipStream_t s);
// per held line: dQRow = its row (0 for none), dMaxK = the k-th key of its running answer (the outputs), all ones while that holds fewer than k
hipError_t zh_launch_fknn_bound(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint32_t k, const uint64_t *dOutKeys, const uint32_t *dOutCounts,
                                uint32_t *dQRow, uint64_t *dMaxK, hipStream_t s);
// every segment of a batch in one launch of n_blocks blocks; lists per held LINE in e (stride e.cap, at most lim entries each); of e it reads Kc, rho
// and the lists
hipError_t zh_launch_fknn_mfma(uint32_t d, int metric, int mode, const ZhFknnSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, const uint32_t *dHeld, uint32_t ch,
                               const void *dCA, const float4 *dCQm, const uint32_t *dCRow, const void *dHA, const float2 *dHMeta, const uint32_t *dHRow,
                               const ZhExact2 &e, uint32_t lim, hipStream_t s);
// the lines' running answers appended to their survivors' candidate slots; the batch's answer [B][k] written back as the running answer (an entry
// whose id is id_base + UINT32_MAX is final_kernel's reading of an empty slot: not counted)
hipError_t zh_launch_fknn_seed(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k, const uint64_t *dOutIds,
                               const uint64_t *dOutKeys, const uint32_t *dOutCounts, const ZhExact2 &e, uint64_t *dCKeys, uint32_t *dCIds, hipStream_t s);
hipError_t zh_launch_fknn_store(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint64_t id_base, uint32_t k, const uint64_t *dInIds,
                                const uint64_t *dInKeys, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, const uint32_t *dOver, hipStream_t s);
// dRedo[(row - first_row) / ZH_FKNN_SLAB] = 1 for every held row of a batch whose lists ran over
hipError_t zh_launch_fknn_mark(const uint32_t *dHRow, uint32_t B, uint64_t first_row, uint32_t *dRedo, hipStream_t s);

// ---- k-NN graph refinement (zh_refine.hip): each live row's neighbours and their neighbours, ranked by the canonical key
#define ZH_REFINE_SLAB 65536u      // stored rows of a sub-slab: one launch of the line kernel
#define ZH_REFINE_CAP_SMALL 2048u  // candidate slots of the small instantiation of the line kernel (in_k + in_k^2 <= 2048: in_k <= 44) ...
#define ZH_REFINE_CAP_LARGE 8192u  // ... and of the large one (in_k <= ZH_REFINE_MAX_IN_K)
// The graph family's wave-per-line kernels (a 256-thread block serves 4 lines) take at most ZH_LINES_PER_LAUNCH lines a launch: 2^30 threads.
#define ZH_LINES_PER_LAUNCH (1ull << 24)
inline uint64_t zh_line_launches(uint64_t n) { return (n + ZH_LINES_PER_LAUNCH - 1) / ZH_LINES_PER_LAUNCH; }  // launches that n lines take
template <class F>
inline void zh_for_line_pieces(uint64_t n, F f) {  // f(b0, m, blocks): the lines [b0, b0 + m) in one launch of `blocks` blocks
    for (uint64_t b0 = 0; b0 < n; b0 += ZH_LINES_PER_LAUNCH) {
        const uint64_t m = n - b0 < ZH_LINES_PER_LAUNCH ? n - b0 : ZH_LINES_PER_LAUNCH;
        f(b0, m, (uint32_t)((m + 3) / 4));
    }
}
// lines [l0, l0 + nl) of the input graph (dIn holds THEIR in_k entries each, from its start) into the table dTab [stored rows][in_k] of row numbers:
// UINT32_MAX for an entry past the line's count, outside [id_base, id_base + n_rows), not live by dBits, or equal to an earlier entry of its line
hipError_t zh_launch_refine_rows(const uint64_t *dIn, const uint32_t *dCounts, const uint32_t *dBits, uint64_t id_base, uint64_t n_rows, uint32_t in_k,
                                 uint64_t l0, uint64_t nl, uint32_t *dTab, hipStream_t s);
// a block per line b (row dRows[b], its f32 values dQ[b], its squared norm dQQ[b]): the first k of C(row) by (key, id) to line row - first_row of the
// outputs; dCtr[0] += listed, dCtr[1] += keyed, dCtr[2] += updates.  dTab's lines are in_k wide; `updates` counts against their first fwd_k entries
// (the caller's own line: in_k for zh_knn_graph_refine, the forward part of the union table for zh_knn_graph_refine_rev)
hipError_t zh_launch_refine_lines(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, const uint32_t *dRows, uint32_t B,
                                  const float *dQ, const float *dQQ, int metric, int param, uint64_t id_base, uint64_t first_row, uint32_t k,
                                  uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s);

// ---- the capped reverse graph (zh_reverse.hip) over zh_launch_refine_rows' table: In(x) = the rows u != x, live by dBits, whose line names x
#define ZH_REVERSE_HEAVY 1024u  // in-degree above which a block of four waves, not one wave, selects a line's reverse neighbours
// dDeg[x] = |In(x)|, dOff[x] = the in-degrees before x (n_rows + 1 entries, the last one the edge count), dCsr[dOff[x] ..] = In(x) in no
// particular order; dCtr[0] = edges, dCtr[1] = max in-degree (dCtr zeroed by the caller).  dCur: n_rows words, dSums: n_rows / 4096 + 1 u64,
// dCsr: n_rows * in_k words at most
hipError_t zh_launch_reverse_csr(const uint32_t *dTab, const uint32_t *dBits, uint64_t n_rows, uint32_t in_k, uint32_t *dDeg, uint32_t *dCur, uint64_t *dOff, uint64_t *dSums,
                                 uint32_t *dCsr, unsigned long long *dCtr, hipStream_t s);
// the same over the lines [r0, r0 + n_lines) only, which name rows of [0, n_rows): dDeg / dCur / dOff as above, dCsr: n_lines * in_k words at most
hipError_t zh_launch_reverse_csr_lines(const uint32_t *dTab, const uint32_t *dBits, uint64_t n_rows, uint32_t in_k, uint64_t r0, uint64_t n_lines, uint32_t *dDeg,
                                       uint32_t *dCur, uint64_t *dOff, uint64_t *dSums, uint32_t *dCsr, unsigned long long *dCtr, hipStream_t s);
// R'(x) of the lines x0 .. x0 + nx: the first rev_k of In(x) - N'(x) by (h(u, x), u).  dUni (or null): line x of the union table [n_rows][in_k +
// rev_k] = N'(x)'s line, then R'(x), UINT32_MAX tails.  dOutIds (or null; then the next two as well): for x in [first_row, first_row + n) line x -
// first_row of [n][rev_k] ids, counts and in-degrees.  dCtr[2] += |R'(x)| over that slab; dCtr[3] and dHeavy (n_rows * in_k / ZH_REVERSE_HEAVY + 1
// words) are the call's list of heavy lines
hipError_t zh_launch_reverse_select(const uint32_t *dTab, uint32_t in_k, uint32_t rev_k, const uint64_t *dOff, const uint32_t *dCsr, uint64_t n_rows, uint64_t x0,
                                    uint64_t nx, uint64_t first_row, uint64_t n, uint64_t id_base, uint32_t *dUni, uint64_t *dOutIds, uint32_t *dOutCounts,
                                    uint32_t *dOutDegree, uint32_t *dHeavy, unsigned long long *dCtr, hipStream_t s);

// ---- NN-descent's incremental rounds (zh_nnd.hip) over u32 tables of row numbers: the forward table [stored rows][k] with its keys [stored rows][k],
// and the table a round ranks over, dU [stored rows][w] (the forward table itself, w = k, or zh_launch_reverse_select's union table, w = k + rev_k)
#define ZH_NND_CTRS 6u  // a round's counters: listed, keyed, updates, active lines, lines on the list's front (small), lines on its back (large)
// lines of u64 ids (2^64 - 1 tails, id_base + row otherwise: a round's own output) -> row numbers, UINT32_MAX tails
hipError_t zh_launch_nnd_rows(const uint64_t *dIds, uint64_t id_base, uint64_t nl, uint32_t k, uint32_t *dTab, hipStream_t s);
// and back at the end: ids with id_base, keys, 2^64 - 1 tails in both, counts
hipError_t zh_launch_nnd_emit(const uint32_t *dTab, const uint64_t *dKeys, uint32_t k, uint64_t id_base, uint64_t nl, uint64_t *dOutIds, uint64_t *dOutKeys,
                              uint32_t *dOutCounts, hipStream_t s);
// dMask[x] bit j = entry j of dCur's line x (wc wide) is a row that dPrev's line x (wp wide) does not hold
hipError_t zh_launch_nnd_flag(const uint32_t *dPrev, uint32_t wp, const uint32_t *dCur, uint32_t wc, uint64_t n_rows, uint64_t *dMask, hipStream_t s);
// per live row (dRows, n_live of them): a line that gathers nothing is copied to dTabNext / dKeysNext, any other goes on dList (n_live words) -- from
// the front (dCtr[4]) if its raw gather count is <= ZH_REFINE_CAP_SMALL, from the back (dCtr[5]) if not
hipError_t zh_launch_nnd_plan(const uint32_t *dU, uint32_t w, uint32_t k, const uint64_t *dMask, const uint32_t *dRows, uint64_t n_live, const uint64_t *dKeys,
                              uint32_t *dTabNext, uint64_t *dKeysNext, uint32_t *dList, unsigned long long *dCtr, hipStream_t s);
// the listed lines: the first k by (key, id) of the keyed candidates and the forward line to dTabNext / dKeysNext; dCtr[0..3] += listed, keyed,
// updates, lines that keyed something.  dQQ: the squared norm of every stored row (read for the cosine kinds only)
hipError_t zh_launch_nnd_lines(const float *dX, uint32_t d, const uint32_t *dU, uint32_t w, uint32_t k, const uint64_t *dMask, const uint64_t *dKeys, const float *dQQ,
                               const uint32_t *dList, uint64_t n_live, int metric, int param, uint32_t *dTabNext, uint64_t *dKeysNext, unsigned long long *dCtr,
                               hipStream_t s);

// ---- graph search (zh_gsearch.hip): beam search over the index's attached graph, dTab = zh_launch_refine_rows' table [g_rows][g_k].  A block per
// query: seeds [B][n_seed] ids, the first top_k of the final beam to the outputs (zh_search_exact_batch's layout); dCtr[0..4] += valid seeds,
// iterations, expanded, keyed, capped queries.  n_rows < 2^31, width * g_k <= 256.  dAllow (zh_search_graph_filtered_batch; null: none) is the
// allowed-AND-live bitmap zh_launch_filter_and made: the walk is the same, the outputs are the first top_k of the ALLOWED rows that got a key, and
// dCtr[5..6] += allowed rows offered (repeats included), entries returned
hipError_t zh_launch_gsearch(const float *dX, uint32_t d, uint64_t n_rows, const uint32_t *dTab, uint64_t g_rows, uint32_t g_k, const uint32_t *dBits,
                             const uint32_t *dAllow, const float *dQ, const float *dQQ, const uint64_t *dSeeds, uint32_t n_seed, uint32_t B, uint64_t id_base, uint32_t top_k,
                             uint32_t beam, uint32_t width, uint32_t max_iters, int metric, int param, uint64_t *dOutIds, uint64_t *dOutKeys,
                             uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s);
// the steered walk (zh_search_graph_steered_batch): the beam holds rows of dAllow (never null) only; hops == 2 reaches them through the lines of the
// disallowed live rows a parent's line names.  The outputs are the first top_k of the final beam; dCtr[0..4] as above, dCtr[5..9] += direct rows,
// rows reached over a bridge, bridges, iterations whose candidate list was full (256), entries returned
hipError_t zh_launch_gsearch_steered(const float *dX, uint32_t d, uint64_t n_rows, const uint32_t *dTab, uint64_t g_rows, uint32_t g_k, const uint32_t *dBits,
                                     const uint32_t *dAllow, const float *dQ, const float *dQQ, const uint64_t *dSeeds, uint32_t n_seed, uint32_t B, uint64_t id_base,
                                     uint32_t top_k, uint32_t beam, uint32_t width, uint32_t max_iters, uint32_t hops, int metric, int param, uint64_t *dOutIds,
                                     uint64_t *dOutKeys, uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s);

// ---- the graph extension and read-back (zh_gextend.hip): dRows = the B live rows of a chunk [lo, hi) of new lines, ascending
// the seed lines of those rows out of the caller's [new rows][n_seed] (row g0 is its line 0), one behind the other
hipError_t zh_launch_gext_seeds(const uint64_t *dSeeds, const uint32_t *dRows, uint32_t B, uint64_t g0, uint32_t n_seed, uint64_t *dOut, hipStream_t s);
// the walk's answer [B][g_k] (ids with id_base, counts) -> lines dRows[b] of the table, UINT32_MAX past the count
hipError_t zh_launch_gext_lines(const uint64_t *dIds, const uint32_t *dCounts, const uint32_t *dRows, uint32_t B, uint32_t g_k, uint64_t id_base, uint32_t *dTab,
                                hipStream_t s);
// every row r < lo that a line of [lo, lo + n_chunk) names (dOff / dCsr: zh_launch_reverse_csr_lines of those lines) re-ranked in place against
// itself: the first g_k of its kept live entries and R(r) by (key, row).  dQQ: the squared norm of every stored row (cosine only).  dTouched:
// min(n_chunk g_k, lo) words.  dCtr[0] (zeroed by the caller) = the rows re-ranked; dCtr[1..3] += the same, the sum of |R(r)|, chunk rows written
hipError_t zh_launch_gext_rerank(const float *dX, uint32_t d, uint32_t *dTab, uint32_t g_k, uint64_t lo, uint32_t n_chunk, const uint32_t *dBits, const float *dQQ,
                                 const uint64_t *dOff, const uint32_t *dCsr, uint32_t *dTouched, int metric, int param, unsigned long long *dCtr, hipStream_t s);
// lines [x0, x0 + nl) of the table as ids: the kept entries in table order at the front (id_base + row), 2^64 - 1 behind them, and their counts
hipError_t zh_launch_gext_read(const uint32_t *dTab, uint32_t g_k, uint64_t x0, uint64_t nl, uint64_t id_base, uint64_t *dOutIds, uint32_t *dOutCounts, hipStream_t s);

// ---- k-NN graph pruning (zh_prune.hip): a block per line b (row dRows[b]) of dTab, w <= ZH_REFINE_MAX_IN_K wide (zh_launch_refine_rows' table or
// zh_launch_reverse_select's union table): the unoccluded candidates in (key, id) order, at most `degree` of them, with fill the first occluded
// ones behind a short line, to line row - first_row of the [..][degree] outputs.  dQQ: the squared norm of every stored row (cosine only).
// dCtr[0..5] += candidates, kept, occluded, filled, lines cut at degree, keyed
hipError_t zh_launch_prune_lines(const float *dX, uint32_t d, const uint32_t *dTab, uint32_t w, const uint32_t *dRows, uint32_t B, const float *dQQ, int metric,
                                 int param, uint64_t id_base, uint64_t first_row, uint32_t degree, uint32_t fill, uint64_t *dOutIds, uint64_t *dOutKeys,
                                 uint32_t *dOutCounts, unsigned long long *dCtr, hipStream_t s);

// ---- the forest self-join (zh_fjoin.hip): every pair of leaf-mates whose key is <= one threshold key, each pair once (the first tree that puts
// the two rows together owns it).  Hit pool, counter and order as the exact self-join's
#define ZH_FJOIN_PANEL_LINES 16384u  // path 1: lines of one panel at most
// path 1: members [i0, i0 + nl) of the leaf {off, len} of leaf_ids as lines line0 .. of the panel, in groups group0 .. (ceil(nl / ZH_GROUP_MAX)
// of them, each sweeping the whole leaf: flat rows from flat0, len per group); line j's keys at key0 + j len
struct ZhFjoinPiece {
    uint32_t off, len, i0, nl;
    uint32_t line0, group0;
    uint64_t flat0, key0;
};
// path 2: held block I0 (tiles I0 .. I0 + 3) of a leaf whose ct tiles start at column tile col0 of the batch; first_block = the launch's blocks
// before this segment's ceil((ct - I0) / ch)
struct ZhFjoinSeg {
    uint32_t col0, ct, I0, first_block;
};
// dLeafOf[r * T + t] = the offset into leaf_ids of the leaf of stored row r in tree t, UINT32_MAX for none; *dLeafPairs += the sum over the
// reachable leaves of len (len - 1) / 2
hipError_t zh_launch_fjoin_rowleaf(const int4 *dNodePack, const uint32_t *dNodeTree, uint32_t n_nodes, const uint32_t *dLeafIds, uint32_t T, uint64_t n_rows,
                                   uint32_t *dLeafOf, unsigned long long *dLeafPairs, hipStream_t s);
// path 1: a panel's lines (dRows, {leaf offset, length} and key offset per line) and its n_groups groups with their flat row offsets
hipError_t zh_launch_fjoin_groups(const ZhFjoinPiece *dPieces, uint32_t n_pieces, uint32_t n_groups, const uint32_t *dLeafIds, uint64_t n_rows, uint32_t *dRows,
                                  uint2 *dLineLeaf, uint64_t *dLineKey, ZhGroup *dGroups, uint64_t *dGroupRowOff, hipStream_t s);
// ... and its hits: the swept keys <= max_key of members above the line's row, for the pairs tree t owns
hipError_t zh_launch_fjoin_collect(const uint64_t *dKeys, const uint32_t *dRows, const uint2 *dLineLeaf, const uint64_t *dLineKey, uint32_t B,
                                   const uint32_t *dLeafIds, uint64_t n_rows, const uint32_t *dLeafOf, uint32_t T, uint32_t t, uint64_t max_key,
                                   unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap, hipStream_t s);
// path 2: every segment of a batch in one launch of n_blocks blocks, chunks of ch tiles, against *dTau (zh_launch_range_tau of the one threshold);
// pairs with lo <= tau to dCand as min(row) << 32 | max(row); *dCandCtr counts them all
hipError_t zh_launch_fjoin_mfma(uint32_t d, int metric, int mode, const ZhFjoinSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, uint32_t ch, const void *dCA,
                                const float2 *dCMeta, const float4 *dCQm, const uint32_t *dCRow, float Kc, float rho, const uint32_t *dTau, uint64_t *dCand,
                                uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s);

// ---- the forest range search (zh_frange.hip): every member of the leaves the walk visits for a query whose key is <= the query's threshold key,
// each (query, row) once (the first tree that offers the row owns the pair).  Hit pool, counters and order as the exact range search's
#define ZH_FRANGE_KEY_ROWS (uint64_t(1) << 25)  // visited rows (path-1 keys) of one internal batch at most, unless it is one query
// path 2: one visited leaf of a batch of leaves: its rt row tiles start at tile col0 of the batch's gathered tiles; its visitors are the members of
// groups group0 .., visitor j = member j % G of group group0 + j / G; first_block = the launch's blocks before this leaf's
struct ZhFrangeSeg {
    uint32_t col0, rt, group0, visitors;
    uint32_t tree, first_block, pad0, pad1;
};
// the lookup of visited leaves: (b T + t) << 32 | leaf offset of every visit, sorted -- pair p's slice stays at [visitBase[p], visitBase[p + 1]).
// dKeys: two buffers of n_visits words; dTmp == nullptr: only *tmp_bytes is set; *dSorted = the buffer that holds the result
hipError_t zh_launch_frange_visit_index(const ZhVisit *dVisits, uint64_t n_visits, const uint32_t *dNodeTree, uint32_t T, uint64_t n_pairs, uint64_t *dKeys[2],
                                        void *dTmp, size_t *tmp_bytes, const uint64_t **dSorted, hipStream_t s);
// path 1: the swept keys (at the visits' row_off) <= the visit's query's threshold that pass the ownership rule, counted and pooled
hipError_t zh_launch_frange_collect(const ZhVisit *dVisits, uint64_t n_visits, const uint64_t *dKeys, const uint32_t *dLeafIds, uint64_t n_rows,
                                    const uint32_t *dNodeTree, const uint64_t *dVSorted, const uint64_t *dVisitBase, const uint32_t *dLeafOf, uint32_t T,
                                    const uint64_t *dMaxKeys, uint32_t *dCnt, unsigned long long *dHitCtr, uint64_t *dPoolV, uint64_t *dPoolK, uint64_t pool_cap,
                                    hipStream_t s);
// path 2: every leaf of a batch in one launch of n_blocks blocks, column chunks of ch tiles, against dTau (zh_launch_range_tau); pairs with
// lo <= tau that pass the rule to dCand as query << 32 | row; *dCandCtr counts them all
hipError_t zh_launch_frange_mfma(uint32_t d, int metric, int mode, const ZhFrangeSeg *dSegs, uint32_t n_segs, uint32_t n_blocks, uint32_t ch, uint32_t group,
                                 const void *dCA, const float2 *dCMeta, const uint32_t *dCRow, const ZhGroup *dGroups, const void *dQh, const float4 *dQmeta,
                                 float Kc, float rho, const uint32_t *dTau, const uint64_t *dVSorted, const uint64_t *dVisitBase, const uint32_t *dLeafOf,
                                 uint32_t T, uint64_t *dCand, uint64_t cand_cap, unsigned long long *dCandCtr, hipStream_t s);

// ---- launchers (zh_score.hip): every sign of a forest built from stored rows, from N row scores per query --------
// Prefilter (zh_search.hip, "Prefilter"): a batch hashed from row scores picks the rows that can be among a pair's k best from
// those scores; only they are scored with the reference's arithmetic.  Lists: one per (tree, query), `cap` slots, list (t, b) at
// (t * B + b) * cap.  ctl[0] = ambiguous visits appended, ctl[1] = overflow bits (1 a list, 2 a list in the exact pass, 4 the
// ambiguous-visit table, 8 a leaf longer than a wave, 16 a query's lists together longer than the final sort), ctl[2] = rows scored exactly.
struct ZhPrefilter {
    const float *S;            // row scores S[row * Bp + b]
    uint32_t Bp;
    const float4 *leaf_meta;   // per slot of leaf_ids: {the row id (its bits), |r|^2 / 2, |r|, 0} of the row stored there
    const float *qnorm;        // |q| per query
    uint32_t *rows, *counts;
    float *tau;                // per list: k of the pair's rows have keys at or below this value (the scale of the prefilter's v); +inf: fewer than k
    uint32_t cap;
    uint4 *amb;                // {pair, leaf_off, len, take}
    uint32_t amb_cap;
    uint32_t *ctl;
};
float zh_prefilter_bound(int metric, uint32_t d);
hipError_t zh_launch_leaf_meta(const uint32_t *dLeafIds, uint64_t n, const float *dHalfN2, const float *dNorm, float4 *dOut, hipStream_t s);
hipError_t zh_launch_prefilter(ZhForestDev f, uint32_t d, uint32_t B, uint32_t k, int metric, int mode, const ZhPairCounts *dCounts,
                               const ZhVisit *dInline, ZhWalkLog log, ZhPrefilter pf, hipStream_t s);
hipError_t zh_launch_prefilter_exact(ZhForestDev f, uint32_t d, const float *dX, const float *dQ, const float *dQQ, uint32_t B, int metric,
                                     int mode, uint64_t id_base, ZhPrefilter pf, uint64_t *dKeys, uint64_t *dIds, hipStream_t s);
hipError_t zh_launch_final_lists(uint32_t T, uint32_t B, uint32_t k, uint32_t cap, const uint64_t *dKeys, const uint64_t *dIds,
                                 const uint32_t *dCounts, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts,
                                 uint32_t *dOver /* the prefilter's overflow word: bit 16 = a query's lists hold more than the final sort */, hipStream_t s);
hipError_t zh_launch_row_norms(const float *dX, uint64_t n, uint32_t d, float *dHalfN2 /* may be null */, float *dNorm, hipStream_t s);
// the score table of exactly four queries (dQ4: 4 x d): dS[row][0..3]
hipError_t zh_launch_row_scores4(const float *dX, uint64_t n, uint32_t d, const float *dQ4, float *dS, hipStream_t s);
// dS: scores [n_rows][B] (row . query, from zh_launch_hash_dense with the roles swapped); dSamples: the two sample rows of every
// plane (UINT32_MAX = a default zero vector); writes the sign words of all P planes for the B queries (B % 4 == 0), the signs
// inside the rounding bound recomputed exactly (list of fix_cap entries; *dFixCount must be 0 on entry and receives their number)
// dPlaneHab: per plane {|a|^2/2, |b|^2/2, |a| + |b|, 0} of its sample rows (zh_launch_plane_hab), read in plane order by the signs kernel
hipError_t zh_launch_plane_hab(const uint2 *dSamples, uint32_t P, const float *dHalfN2, const float *dRowNorm, float4 *dOut, hipStream_t s);
hipError_t zh_launch_score_unc_fix(const float *dQ, uint32_t B, uint32_t d, const float *dPlanes, const float *dConsts, uint32_t P,
                                   uint32_t *dBits, const uint32_t *dUnc, uint32_t wpq, hipStream_t s);
hipError_t zh_launch_score_signs(const float *dS, uint32_t B, const uint2 *dSamples, uint32_t P, const float *dHalfN2, const float *dRowNorm,
                                 const float4 *dPlaneHab, const float *dQNorm, const float *dQ, uint32_t d, const float *dPlanes, const float *dConsts,
                                 uint32_t *dBits, uint32_t wpq, uint2 *dFixList, uint32_t fix_cap, unsigned long long *dFixCount, uint32_t *dUnc /* null: list + fix-up kernel */,
                                 hipStream_t s);

// ---- launchers (zh_build.hip) ----------------------------------------------------------------
struct ZhBuildNode {   // an active (to be split) node of the current level
    uint64_t seg_start;  // global position in perm (tree * N + offset)
    uint32_t len;
    uint32_t plane;      // plane index this node's hyperplane is written to
    uint64_t sample_a, sample_b;  // row numbers; UINT64_MAX = the all-zero default vector
    uint32_t first_chunk, n_chunks;
};
struct ZhBuildChunk {
    uint32_t node;       // index into the level's ZhBuildNode array
    uint32_t count;      // <= 256
    uint64_t pos;        // global position of the chunk's first row in perm
};

// incremental insert (lsh.rs:350-382): descend a stored row from `node` to a leaf
struct ZhDescend {
    uint32_t row, node, depth, tree;
    uint64_t path;
};
// node_pack from the three node arrays and the plane constants
hipError_t zh_launch_pack_nodes(const int32_t *dPlane, const int32_t *dLeft, const int32_t *dRight, const float *dConsts,
                                int4 *dPack, uint32_t n_nodes, hipStream_t s);
hipError_t zh_launch_descend(ZhForestDev f, const float *dX, uint32_t d, ZhDescend *dItems, uint32_t n, hipStream_t s);

// 64-bit content hash of every stored row (order-sensitive, exact integer arithmetic): deduplicate
hipError_t zh_launch_row_hash(const float *dX, uint64_t n, uint32_t d, uint64_t *dHash, hipStream_t s);

// out[i] = 1 when rows pairs[2i] and pairs[2i+1] have identical f32 bit patterns
hipError_t zh_launch_rows_equal(const float *dX, uint32_t d, const uint32_t *dPairs, uint32_t n_pairs, uint8_t *dOut,
                                hipStream_t s);

hipError_t zh_launch_synth_rows(float *dX, uint64_t n, uint32_t d, uint64_t seed, uint64_t row0, int kind,
                                hipStream_t s);
hipError_t zh_launch_synth_queries(float *dOut, uint64_t seed_rows, uint64_t seed_q, uint64_t n_rows, uint64_t b0,
                                   uint64_t b, uint32_t d, int kind, hipStream_t s);
hipError_t zh_launch_iota_perm(uint32_t *dPerm, uint64_t N, uint32_t T, hipStream_t s);
hipError_t zh_launch_make_planes(const float *dX, uint32_t d, const ZhBuildNode *dNodes, uint32_t n_nodes,
                                 float *dPlanes, float *dConsts, hipStream_t s);
hipError_t zh_launch_classify(const float *dX, uint32_t d, const uint32_t *dPerm, const ZhBuildNode *dNodes,
                              const ZhBuildChunk *dChunks, uint32_t n_chunks, const float *dPlanes,
                              const float *dConsts, uint8_t *dFlags, uint32_t *dChunkAbove, hipStream_t s);
hipError_t zh_launch_scan_u32(const uint32_t *dIn, uint32_t *dOut /* n+1 */, uint64_t n, uint32_t *dTmp /* >= n/1024+2 */,
                              hipStream_t s);
hipError_t zh_launch_scatter(const uint32_t *dPermIn, uint32_t *dPermOut, const ZhBuildNode *dNodes,
                             const ZhBuildChunk *dChunks, uint32_t n_chunks, const uint8_t *dFlags,
                             const uint32_t *dChunkScan, uint32_t *dNodeAbove, hipStream_t s);

// ---- launchers (zh_compact.hip): zh_index_compact ---------------------------------------------------------------------------------
#define ZH_COMPACT_RANK_ROWS 8192u  // rows per block of the rank pass (256 words of the live bitmap)
// dNewRow[r] = live rows before r, or UINT32_MAX for a removed row, from the live bitmap (bits at and past n_rows zero).  dBlockCount: n_blocks
// entries, dBlockExcl: n_blocks + 1, dScanTmp: n_blocks / 1024 + 2, for n_blocks = ceil(n_rows / ZH_COMPACT_RANK_ROWS)
hipError_t zh_launch_compact_rank(const uint32_t *dLiveBits, uint64_t n_rows, uint32_t *dBlockCount, uint32_t *dBlockExcl, uint32_t *dScanTmp,
                                  uint32_t *dNewRow, hipStream_t s);
// rows [r0, r0 + n) of dSrc -> row (dMap ? dMap[r] : r) - sub of dDst (a UINT32_MAX entry: not moved); source and destination must not overlap
hipError_t zh_launch_move_rows(const float *dSrc, float *dDst, uint32_t d, const uint32_t *dMap, uint64_t r0, uint64_t n, uint64_t sub, hipStream_t s);
hipError_t zh_launch_renumber_ids(uint32_t *dIds, uint64_t n, const uint32_t *dNewRow, uint64_t rows_before, hipStream_t s);
// *dFlag |= 1 when a sample row was removed
hipError_t zh_launch_renumber_samples(uint2 *dSamples, uint32_t n, const uint32_t *dNewRow, uint64_t rows_before, uint32_t *dFlag, hipStream_t s);

// ---- snapshots (zh_snapshot.hip): zh_index_save / zh_index_load ----------------------------------------------------------------------
// *dSum += the section checksum's terms (zh_snapfile.h) of the n_bytes at dBytes (8-byte aligned), whose first word is word `word0` of its section
hipError_t zh_launch_snap_sum(const void *dBytes, uint64_t n_bytes, uint64_t word0, uint64_t *dSum, hipStream_t s);
// the row table between device memory and the file, in chunks of ZH_SNAPSHOT_CHUNK_BYTES through two pinned buffers on a stream of the call's
// own; *out_sum = the checksum of the bytes as they were (out) / arrived (in) in DEVICE memory, *ms_device the hipEvent time of the device work
int zh_snap_rows_out(int fd, const char *path, uint64_t file_off, const void *dSrc, uint64_t n_bytes, uint64_t *out_sum, double *ms_device);
int zh_snap_rows_in(int fd, uint64_t file_off, void *dDst, uint64_t n_bytes, uint64_t *out_sum, double *ms_device);

// zh_api.hip -- the C ABI of include/zebra_hip.h: index lifetime, device memory, forest build
// orchestration and the per-batch search pipeline.  Host code only; kernels live in
// zh_search.hip / zh_build.hip.  There is no CPU compute path in this file: every entry point
// that produces distances, signs or neighbours launches gfx950 kernels.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <deque>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "zh_internal.h"
#include "zh_snapfile.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return fail(e_ == hipErrorOutOfMemory ? ZH_ENOMEM : ZH_EHIP, "%s: %s (%s:%d)", #expr,          \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                        \
    } while (0)

// the same thread-local message for the host-only translation units
int zh_set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *zh_last_error(void) { return g_err.c_str(); }
extern "C" const char *zh_version(void) { return "zebra-hip 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------
// growable device buffer
// ------------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // hipFree waits for EVERY stream of the device to drain.  A per-batch scratch buffer that outgrows its capacity while other
    // batches are in flight would stall the host until their sweeps, selects and finals have run -- and the sweep queue runs dry
    // meanwhile (rocprofv3 kernel trace, r03: a 1.3-2.9 ms hole in front of the next window's sweep each time).  Buffers of a
    // search context therefore keep the outgrown allocation (geometric growth: at most twice the final size in total) until
    // the context is released, and ask for 1/8 more than a batch needs so that batch-to-batch variation rarely grows them at all.
    // ... but not without bound: a score table grows to 12 GB per context, and three generations of it would be held until the
    // context is destroyed.  Past 2 GiB of outgrown allocations they are freed on the spot (one drain, rare).
    bool defer = false;
    std::vector<void *> old;
    size_t old_bytes = 0;
    int ensure(size_t bytes, bool keep = false, hipStream_t s = nullptr) {
        if (bytes <= cap) return ZH_OK;
        if (defer) bytes += bytes / 8;
        if (defer && old_bytes + cap > (size_t(2) << 30)) {
            for (void *o : old) hipFree(o);
            old.clear();
            old_bytes = 0;
        }
        size_t ncap = std::max(bytes, cap + cap / 2);
        ncap = (ncap + 255) & ~size_t(255);
        void *np = nullptr;
        hipError_t e = hipMalloc(&np, ncap);
        if (e != hipSuccess) {
            ncap = (bytes + 255) & ~size_t(255);
            e = hipMalloc(&np, ncap);
        }
        if (e != hipSuccess) return fail(ZH_ENOMEM, "hipMalloc(%zu bytes): %s", ncap, hipGetErrorString(e));
        if (keep && p && cap) {
            e = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { hipFree(np); return fail(ZH_EHIP, "grow copy: %s", hipGetErrorString(e)); }
        }
        if (p) { if (defer) { old.push_back(p); old_bytes += cap; } else hipFree(p); }
        p = np;
        cap = ncap;
        return ZH_OK;
    }
    void release() {
        if (p) hipFree(p);
        for (void *o : old) hipFree(o);
        old.clear();
        old_bytes = 0;
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// One in-flight search batch: its own workspace, events and (borrowed) stream, so that several batches can be
// in flight on different streams (zh_search_begin / zh_search_finish / zh_search_wait).
struct zh_search_ctx {
    zh_index *ix = nullptr;
    DevBuf wQQ, wBits, wCounts, wInline, wRowBase, wCandBase, wVisitBase, wTotals, wVisits, wKeys, wCandKeys, wCandIds,
        wLeafCount, wLeafFill, wGroupBase, wGroupRowBase, wGroups, wGroupRowOff, wWaveGroup, wVisitBits, wNodeVisit, wScore, wJunkBits, wZeros, wQnorm, wQpad, wFixList, wLogPool, wLogHead, wLogCtl,
        wPfRows, wPfCounts, wPfKeys, wPfIds, wPfAmb, wPfCtl, wUnc, wQh, wQmeta, wApList, wApCount, wApEx, wApExKeys, wApCtl, wRaw;
    // test / debug (zh_debug_scan_pairs): the half-width batch this context ran last -- its ZhApprox, and (zh_debug_keep_raw) the scan's raw pairs
    ZhApprox dbg_ap{};
    bool dbg_valid = false, dbg_raw = false;
    size_t log_chunks = 0;  // capacity of wLogPool for the batch in flight
    ZhTotals *h_totals = nullptr;  // pinned
    hipEvent_t ev[6] = {};         // stage boundaries: hash | walk | sweep | select | final
    hipEvent_t ev_totals = nullptr, ev_emit = nullptr, ev_sw0 = nullptr, ev_sw1 = nullptr;
    bool ev_ok = false;
    // the batch in flight
    int state = 0;  // 0 idle, 1 begun (first half enqueued), 2 finished (second half enqueued, results pending)
    bool trivial = false;
    const float *dQ = nullptr;
    size_t B = 0, k = 0;       // B = every query of the window
    size_t nwin = 1, bwin = 0;  // a window = nwin API batches of bwin queries handled as ONE internal batch
    DevBuf wQwin, wOutWin;      // the window's queries side by side / its results before they are handed out per batch
    int metric = 0, mode = 0;
    uint32_t P_dense = 0, wpq = 0;
    hipStream_t s = nullptr;
    ZhTotals tot{};
    bool scan = false;  // the batch in flight was swept by the table scan (rows streamed once) instead of leaf by leaf
    // ... with half-width queries (zh_approx.hip): intervals from the scan, the reference's keys for the few rows they cannot
    // decide.  Its control words come back pinned for the statistics only: an overflow is redone on the device, in stream order.
    bool approx_f32rows = false;  // (approx_mfma without an fp16 copy of the table: scan_mfma_kernel<D, true>)
    bool approx_fused = false;  // (approx_leaf, round 6: intervals, bounds and lists inside the sweep kernel)
    bool approx_bytes = false;  // (approx_leaf, round 6: the sweep reads the copy of BYTES -- a table of integers 0 .. 255)
    bool approx = false, approx_mfma = false, approx_leaf = false;  // (approx_leaf: the d = 128 leaf-major sweep at half width, sweep128h_kernel)
    uint32_t *h_ap = nullptr;
    bool score_hash = false;  // its signs came from row scores (zh_score.hip) instead of one dot product per plane
    uint32_t score_Bp = 0;    // ... for this many (padded) queries per stored row
    bool lazy_fix = false;    // ... with the uncertain signs flagged (wUnc) for the blocked walk to recompute when it meets one
    // prefilter (zh_search.hip): the batch's candidates are picked from those row scores and only they are scored exactly.  Its
    // control words come back pinned; a list that ran over makes zh_search_wait redo the batch the classic way, from these:
    bool prefilter = false, prefilter_off_once = false, stream_ordered = false;
    uint32_t pf_cap = 0;
    uint32_t *h_pf = nullptr;
    std::vector<const float *> sv_q;
    std::vector<uint64_t *> sv_ids, sv_keys;
    std::vector<uint32_t *> sv_counts;
    hipStream_t sv_heavy = nullptr;
    std::vector<DevBuf *> all_bufs() {
        return {&wQQ, &wBits, &wCounts, &wInline, &wRowBase, &wCandBase, &wVisitBase, &wTotals, &wVisits, &wKeys,
                &wCandKeys, &wCandIds, &wLeafCount, &wLeafFill, &wGroupBase, &wGroupRowBase, &wGroups, &wGroupRowOff, &wWaveGroup, &wVisitBits, &wNodeVisit, &wScore, &wJunkBits, &wZeros, &wQnorm, &wQpad, &wFixList,
                &wLogPool, &wLogHead, &wLogCtl, &wQwin, &wOutWin, &wPfRows, &wPfCounts, &wPfKeys, &wPfIds, &wPfAmb, &wPfCtl, &wUnc,
                &wQh, &wQmeta, &wApList, &wApCount, &wApEx, &wApExKeys, &wApCtl, &wRaw};
    }
    void release_all() {
        for (DevBuf *b : all_bufs()) b->release();
        if (ev_ok) { for (auto &e : ev) hipEventDestroy(e); hipEventDestroy(ev_totals); hipEventDestroy(ev_emit); hipEventDestroy(ev_sw0); hipEventDestroy(ev_sw1); ev_ok = false; }
        if (h_totals) { hipHostFree(h_totals); h_totals = nullptr; }
        if (h_pf) { hipHostFree(h_pf); h_pf = nullptr; }
        if (h_ap) { hipHostFree(h_ap); h_ap = nullptr; }
    }
};

struct zh_index {
    zh_options opt{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t sweep_stream = nullptr;  // lowest priority: shared by the sweeps of pipelined contexts
    // exclusive: everything that changes the index or uses its one blocking context (dctx); shared: the combining front end's lanes,
    // which search on contexts of their own (searches on different contexts run side by side, as the pipelined calls do)
    std::shared_mutex mu;

    // stored vectors: n_rows x dim row-major f32 (Embedding<N>, lib.rs:18)
    DevBuf X;
    uint64_t n_rows = 0;

    // forest
    DevBuf node_plane, node_left, node_right, node_pack, roots, planes, consts, leaf_ids;
    uint32_t n_nodes = 0, n_planes = 0, n_trees = 0;
    uint64_t n_leaf_ids = 0;
    std::vector<int32_t> h_plane, h_left, h_right;
    std::vector<uint32_t> h_roots;
    std::vector<uint32_t> planes_below_level;  // [L] = planes whose level < L ; planes are stored level-major
    std::vector<uint32_t> h_leaf_ids;          // host mirror of leaf_ids, materialised by the first incremental add
    std::vector<uint8_t> h_dead;               // rows removed by zh_index_remove (their vectors stay in X)
    uint64_t n_dead = 0;
    // Caches derived from the stored rows are keyed on a generation as well as on a count: clear() followed by a refill to the
    // same count must not find them valid.  rows_gen: bumped whenever the CONTENT of rows [0, n_rows) may have changed (clear, compact);
    // dead_gen: whenever the set of removed rows changed (remove, clear, compact).  Both start at 1: a stamp of generation 0 names no table.
    uint64_t rows_gen = 1, dead_gen = 1;
    uint32_t max_leaf_len = 0;
    std::mutex blk_mu;

    // ---------------------------------------------------------------------------------------------------------------------------------------
    // Derived views of the rows and the forest: built lazily, one record each -- its buffers, its state, the ONE place its "is it current" test
    // is written, and how it is marked and dropped.  What every mutation does to every view is the event routines below the struct
    // (views_trees_dropped ...; the table is in DESIGN.md s4): nothing else assigns a view's state.
    // The rule for the state: whatever the per-batch choices and the two halves of a batch read WITHOUT a lock (ctx_begin, ctx_finish, choose_scan,
    // use_approx, use_approx_leaf, mfma_wanted, use_score_hash, use_prefilter, launch_score_hash) is a std::atomic -- another context may be
    // building the view under blk_mu at that moment.  The buffers themselves are only touched under blk_mu (or under `mu` held exclusively).
    // ---------------------------------------------------------------------------------------------------------------------------------------
    struct Stamp {  // "built for which rows": their count and the generation of their content (or, for the live-row lists, of the removed set)
        std::atomic<uint64_t> rows{0}, gen{0};
        bool is(uint64_t r, uint64_t g) const { return rows == r && gen == g; }
        void set(uint64_t r, uint64_t g) { rows = r; gen = g; }
    };
    // blocked view of the forest (ZhBlocksDev) for all-dense walks: built on first use, not valid once the trees change
    struct BlocksView {
        DevBuf recs, upper, roots;
        std::atomic<uint32_t> n_blocks{0}, n_upper{0};
        std::atomic<bool> valid{false};
        std::atomic<bool> inner{false};   // the view holds blocks of INNER nodes only (round 5; ZhBlocksDev::inner_only)
        std::atomic<size_t> recs_b{0};    // ... whose records' second halves start at this index of recs
        void mark_built(uint32_t blocks, uint32_t uppers, bool inner_only, size_t second_halves) {
            n_blocks = blocks; n_upper = uppers; inner = inner_only; recs_b = second_halves; valid = true;
        }
        void invalidate() { valid = false; }  // (the buffers stay for the next build)
        void drop() { recs.release(); upper.release(); roots.release(); n_blocks = 0; n_upper = 0; inner = false; recs_b = 0; valid = false; }
    } blocks;
    // row -> (leaf, position) per tree for the table-scan sweep (zh_launch_row_leaf): built on first use, for the trees and the stored rows of that
    // moment (rows appended since are in no tree yet, but must not be scanned past it); a failed allocation is remembered until the trees change
    struct RowLeafView {
        DevBuf table;
        std::atomic<bool> valid{false}, failed{false};
        std::atomic<uint64_t> rows{0};  // stored rows the table was built for (read only where valid)
        uint64_t version = 0;           // counts the builds (never reset): ScanOrder's gathered copy names the one it was made from
        bool current(const zh_index *ix) const { return valid && rows == ix->n_rows; }
        void mark_built(uint64_t n) { valid = true; rows = n; version++; }
        void mark_failed() { failed = true; }
        void invalidate() { valid = false; failed = false; }  // (the trees changed: the table is stale, and a failed allocation gets another try)
        void drop() { table.release(); invalidate(); }
    } row_leaf;
    // the MFMA table scan's view of the stored rows (zh_launch_row_half): their fp16 copy in the A operand's order (2 * d bytes per row), per
    // row {|x|^2, 1 / scale}, and the largest relative rounding error of any row; for the rows `at` names, extended when rows are appended; a
    // failed allocation is remembered until the rows change (the VALU kernel serves the index).  tiles released and meta kept: the per-row scales
    // alone (scan_mfma_kernel<D, true> converts the f32 rows itself).  rho_dev: the builders' few words of device scratch (RowHalf128View's too).
    struct RowHalfView {
        DevBuf tiles, meta, rho_dev;
        Stamp at;
        std::atomic<bool> failed{false};
        std::atomic<float> rho{0.f};
        bool current(const zh_index *ix) const { return at.is(ix->n_rows, ix->rows_gen); }   // made -- or found impossible -- for the rows stored now
        bool known_failed(const zh_index *ix) const { return failed && current(ix); }
        void mark_built(const zh_index *ix, float r) { rho = r; at.set(ix->n_rows, ix->rows_gen); }
        void mark_failed(const zh_index *ix) { failed = true; at.set(ix->n_rows, ix->rows_gen); }
        void retry() { failed = false; }
        void remake() { at.gen = 0; }  // (the copy is made again from row 0 by the next batch that wants it; `rows` and the buffers stay)
        void drop() { at.set(0, 0); rho = 0.f; tiles.release(); meta.release(); failed = false; }  // (rho_dev goes with the index)
    } half;
    // Round 5 (VERDICT r4 #4b): the matrix-core scan's OWN view of the rows -- the fp16 tiles, their {|x|^2, 1 / scale} and the row -> leaf entries --
    // is kept sorted by (leaf in tree 0, leaf in tree 1, leaf in tree 2, id): position p holds row perm[p] (zh_order.hip).  The scan never needs
    // a row's id (its outputs go to key slots that the row -> leaf entries name), so nothing else changes; a wave's 16 rows then share tree 0's leaf --
    // its visitors are ONE tile column each for all 16 -- and, on data with structure, most other trees' too, whatever order the rows were inserted
    // in.  Made with the copy, from the row -> leaf table; rows appended later keep position = id; the f32 rows and every other kernel stay in id
    // order.  row_leaf_p = the row -> leaf table gathered into that order: for build p_table of RowLeafView and order p_order.  All under blk_mu.
    struct ScanOrder {
        DevBuf perm, row_leaf_p;
        bool off = false;       // given up for lack of room: id order until the trees or the table are replaced
        uint32_t keys = 0;      // trees whose leaves the kept order sorts by (0: id order)
        double worth = 0;       // share of (adjacent positions, tree) combinations in the same leaf under the kept order
        uint64_t rows = 0;      // rows the order covers (0: id order -- it won, there is no table, the order is off, or there was no room for the sort)
        uint64_t version = 0;   // counts the orders made and given up (never reset)
        uint64_t p_table = 0, p_order = 0;
        bool table_current(const RowLeafView &rl) const { return p_table == rl.version && p_order == version; }
        void mark_table(const RowLeafView &rl) { p_table = rl.version; p_order = version; }
        void begin() { rows = 0; version++; keys = 0; }  // (id order, until mark_built says otherwise)
        void mark_built(uint32_t k, double w, uint64_t n) { keys = k; worth = w; if (k) rows = n; }
        void no_room_for_table() { rows = 0; }
        void switch_off() { off = true; }
        void allow() { off = false; }
        bool used() const { return rows || keys; }
        void drop() { rows = 0; version++; perm.release(); row_leaf_p.release(); }  // (keys, worth and off stay: DESIGN.md s4, "kept as found")
    } order;
    // d = 128, leaf by leaf at half width (sweep128h_kernel): a row-major fp16 copy under ONE power-of-two scale (2^(14 - ex)), same life cycle as
    // RowHalfView's ... or, for a table of integers 0 .. 255 (SIFT descriptors), an EXACT copy of 128 bytes per row in the same buffer
    // (row_byte128_kernel): bytes = the current copy is that one; not_bytes = some stored row is known not to qualify (until the rows are replaced)
    struct RowHalf128View {
        DevBuf copy;
        Stamp at;
        std::atomic<int> ex{0};
        std::atomic<float> rho{0.f};
        std::atomic<bool> failed{false};
        bool bytes = false, not_bytes = false;  // (blk_mu)
        bool current(const zh_index *ix) const { return at.is(ix->n_rows, ix->rows_gen); }
        bool known_failed(const zh_index *ix) const { return failed && current(ix); }
        uint64_t extend_from(const zh_index *ix, bool as_bytes) const {  // first row a copy of that kind still lacks (0: made from scratch)
            return at.gen == ix->rows_gen && at.rows <= ix->n_rows && bytes == as_bytes ? at.rows.load() : 0;
        }
        void set_scale(int e) { ex = e; }  // (of a copy of halves about to be made from the first row)
        void mark_bytes(const zh_index *ix) { bytes = true; rho = 0.f; ex = 14; at.set(ix->n_rows, ix->rows_gen); }
        void mark_halves(const zh_index *ix, float r) { rho = r; bytes = false; at.set(ix->n_rows, ix->rows_gen); }
        void mark_failed(const zh_index *ix) { failed = true; bytes = false; at.set(ix->n_rows, ix->rows_gen); }
        void retry() { failed = false; }
        void found_not_bytes() { not_bytes = true; bytes = false; at.gen = 0; }  // the copy of halves, from the first row, now and from now on
        void drop() { at.set(0, 0); rho = 0.f; copy.release(); failed = false; bytes = false; }  // (not_bytes and ex stay: see the events)
    } half128;

    // the blocking entry points run on this context (under `mu`); staging buffers of the host-pointer variant
    zh_search_ctx dctx;
    DevBuf wQ, wOutIds, wOutKeys, wOutCounts;
    // the exact search (zh_search_exact_*, zh_exact.hip): scratch of its own, so that pipelined search contexts are never touched (its live rows
    // on the device: LiveRowsDev below)
    DevBuf ex_QQ, ex_keys, ex_visits, ex_cbase, ex_ckeys, ex_cids, ex_run_ids, ex_run_keys, ex_run_counts, ex_Q, ex_ids, ex_kout, ex_counts,
        ex_Qh, ex_qmeta, ex_tau, ex_cnt, ex_lid, ex_llo, ex_lhi, ex_scr, ex_over;
    zh_exact_info ex_info{};  // (stats_mu)
    // the filtered exact search's per-call scratch (all released before the call returns): the caller's filter, allowed AND live by row and by
    // position of the scan's row order, the blocks' counts and their exclusive sums, the ascending list of allowed live rows
    DevBuf fl_filter, fl_bits, fl_pos, fl_bcount, fl_bexcl, fl_tmp, fl_list;
    zh_filtered_info fl_info{};  // (stats_mu)
    // the range search's per-call scratch (all released before the call returns): thresholds, counts per query, {hit, candidate} counters, the hit
    // pool and its sort partner (v and key), path 2's candidate pool, the sort's temporary storage, offsets and outputs staged for the host call
    DevBuf rg_maxk, rg_cnt, rg_ctr, rg_pv0, rg_pv1, rg_pk0, rg_pk1, rg_cand, rg_tmp, rg_off, rg_oids, rg_okeys;
    zh_range_info rg_info{};  // (stats_mu)
    // the joins' per-call scratch (all released before the call returns; the forest join's and the cross-join's too, which hold mu exclusively as the
    // self-join does; the cross-join's is on its LEFT index): {hit, candidate, panel-row} counters, the threshold's bound, the hit pool and its sort
    // partner, path 2's per-position views, block table and candidate pool, a redone panel's row list, the sort's temporary storage and the outputs
    // staged for the host call
    DevBuf jn_ctr, jn_maxk, jn_tau, jn_pv0, jn_pv1, jn_pk0, jn_pk1, jn_qm, jn_cid, jn_first, jn_cand, jn_rows, jn_tmp, jn_oa, jn_ob, jn_okeys;
    zh_join_info jn_info{};  // (stats_mu)
    // what the cross-join holds beside them, on the LEFT index too: path 2's per-position views of A (id word; the query view zh_launch_join_prep
    // writes beside it is not read) and of B (query view, id word)
    DevBuf xj_qma, xj_cida, xj_qmb, xj_cidb;
    zh_cross_info xj_info{};  // (stats_mu)
    // the k-NN graph's per-call scratch (all released before the call returns): path 2's per-position views and row -> position map, one panel's
    // tiles, rowMeta and row numbers, the lists' bases, the panel's answer, and the outputs staged for the host call
    DevBuf kn_qm, kn_cid, kn_pos, kn_A, kn_pmeta, kn_pid, kn_cbase, kn_pids, kn_pkeys, kn_pcounts, kn_oids, kn_okeys, kn_ocounts;
    zh_knn_info kn_info{};  // (stats_mu)
    // what the k-NN join between two indexes holds beside the graph's, on the LEFT index: path 2's per-position views of B (query view, id word)
    DevBuf xk_qmb, xk_cidb;
    zh_xknn_info xk_info{};  // (stats_mu)
    // the forest k-NN graph's per-call scratch (all released before the call returns): the node -> tree map, a sub-slab's row -> leaf table, line
    // flags, their exclusive sums and the lines, {pairs, tiles} counters, a path-1 panel's visit sizes, bases, groups and their row offsets, and
    // path 2's batch: segments, column sources, column and held rows, held counts, both sides' tiles, rowMeta and queries, the lines' rows and
    // bounds, the sub-slabs to redo, the row -> position map
    DevBuf fk_ntree, fk_rl, fk_flag, fk_excl, fk_tmp, fk_rows, fk_ctr, fk_lens, fk_takes, fk_rbase, fk_cbase, fk_groups, fk_groff, fk_segs, fk_colsrc, fk_crow,
        fk_hrow, fk_held, fk_CA, fk_cmeta, fk_cqm, fk_HA, fk_hmeta, fk_qrow, fk_maxk, fk_redo, fk_pos;
    zh_knn_forest_info fk_info{};  // (stats_mu)
    // the graph refinement's per-call scratch beside the graph's staging and the exact search's query rows (all released before the call returns):
    // the table of row numbers, the lines' counts, one chunk of the host call's u64 input, {listed, keyed, updates}
    DevBuf rf_tab, rf_cnt, rf_stage, rf_ctr;
    zh_knn_refine_info rf_info{};  // (stats_mu)
    // the capped reverse graph's per-call scratch beside the refinement's (all released before the call returns): in-degrees, fill cursors, 64-bit
    // offsets, the scan's block sums, the in-neighbours, the heavy lines, the union table, {edges, max degree, kept, heavy lines}, the host call's staging
    DevBuf rv_deg, rv_cur, rv_off, rv_sums, rv_csr, rv_heavy, rv_uni, rv_ctr, rv_oids, rv_ocounts, rv_odeg;
    zh_knn_reverse_info rv_info{};          // (stats_mu)
    zh_knn_refine_rev_info rfr_info{};      // (stats_mu)
    // NN-descent's per-call scratch beside the reverse graph's (all released before the call returns): the two forward tables of row numbers and
    // their keys, the two union tables, the new-mask of every line, the list of active lines, every stored row's squared norm, a round's counters
    DevBuf nd_tab[2], nd_key[2], nd_uni[2], nd_mask, nd_list, nd_qq, nd_ctr;
    zh_knn_descent_info nd_info{};          // (stats_mu)
    // the graph pruning's per-call scratch beside the reverse graph's (all released before the call returns): every stored row's squared norm,
    // {candidates, kept, occluded, filled, cut, keyed}
    DevBuf pr_qq, pr_ctr;
    zh_knn_prune_info pr_info{};            // (stats_mu)
    // the forest self-join's per-call scratch beside the self-join's and the forest graph's (all released before the call returns): leaf_of, a path-1
    // panel's pieces and per-line {leaf, key offset}, path 2's segments and candidate pool
    DevBuf fj_leafof, fj_pieces, fj_linel, fj_linek, fj_segs, fj_cand;
    zh_join_forest_info fj_info{};  // (stats_mu)
    // the forest range search's per-call scratch beside the range search's and the forest join's (all released before the call returns): the walk's
    // workspace of one internal batch (what a search context keeps in its w* buffers: pair counts, inline visits, the three bases, totals, per-leaf
    // counts / fill cursors / group bases, the visit log), its visits and groups, the sorted visit words and their sort partner and temporary
    // storage, and path 2's leaves
    DevBuf fr_counts, fr_inline, fr_rowbase, fr_candbase, fr_visitbase, fr_totals, fr_leafcount, fr_leaffill, fr_groupbase, fr_grouprowbase, fr_loghead,
        fr_logctl, fr_logpool, fr_visits, fr_groups, fr_groupoff, fr_vk0, fr_vk1, fr_vtmp, fr_segs;
    zh_range_forest_info fr_info{};  // (stats_mu)

    bool broken = false;  // an incremental add failed half way: trees are stale until zh_index_build
    bool rows_torn = false;  // ... or a compaction failed after rows had begun to move (set with broken): the TABLE is inconsistent until zh_index_clear
    int dense_levels = -1;
    bool debug_keep_raw = false;  // zh_debug_keep_raw
    std::atomic<int> sweep_mode{0};  // zh_set_sweep_mode (atomic: set by one thread while pipelined contexts read it per batch): 0 cost model (prefilter where the batch has row scores), 1 leaf-major, 2 table scan (exact), 3 = 0, 4 table scan with half-width queries wherever it applies, 5 = 4 with the VALU kernel only (no fp16 copy of the rows)
    int hash_mode = 0;   // zh_set_hash_mode: 0 chosen per batch, 1 one dot product per plane, 2 row scores where the forest allows
    // the two sample rows of every plane (build_hyperplane, lsh.rs:197-225), kept for forests this library built or grew: the
    // row-score hash derives signs from them.  An injected forest (zh_index_set_forest) has arbitrary planes: not valid.
    struct PlaneSamples {
        DevBuf pairs;
        std::atomic<bool> valid{false};
        void mark(bool known) { valid = known; }
        void drop() { pairs.release(); valid = false; }
    } samples;
    // |r|^2 / 2 and |r| of the stored rows
    struct RowNorms {
        DevBuf hn2, norm;
        Stamp at;
        bool current(const zh_index *ix) const { return at.is(ix->n_rows, ix->rows_gen); }  // (rows added, or replaced, since they were taken?)
        void mark_built(const zh_index *ix) { at.set(ix->n_rows, ix->rows_gen); }
        void drop() { at.set(0, 0); hn2.release(); norm.release(); }
    } norms;
    // ... the same per PLANE (its two sample rows): for the first `planes` planes, from the norms of stamp `of`
    struct PlaneNorms {
        DevBuf hab;
        std::atomic<uint32_t> planes{0};
        Stamp of;
        bool current(const zh_index *ix) const { return planes == ix->n_planes && of.is(ix->norms.at.rows, ix->norms.at.gen); }  // (planes added, or the norms retaken?)
        void mark_built(const zh_index *ix) { planes = ix->n_planes; of.set(ix->norms.at.rows, ix->norms.at.gen); }
        void forget() { planes = 0; of.set(0, 0); }  // (the buffer stays for the next build)
        void drop() { hab.release(); forget(); }
    } plane_norms;
    // {|r|^2/2, |r|} of the row in every slot of leaf_ids, for the prefilter: built on first use from the norms of stamp `of`, for the trees of
    // that moment
    struct LeafMeta {
        DevBuf slots;
        std::atomic<bool> valid{false};
        Stamp of;
        bool current(const zh_index *ix) const { return valid && of.is(ix->norms.at.rows, ix->norms.at.gen); }
        void mark_built(const zh_index *ix) { valid = true; of.set(ix->norms.at.rows, ix->norms.at.gen); }
        void invalidate() { valid = false; }  // (the buffer stays for the next build)
        void drop() { slots.release(); valid = false; }
    } leaf_meta;
    // ascending live rows on the host, for hyperplane sampling once rows were removed: for (n_rows, dead_gen) and n_dead (under mu, exclusive)
    struct LiveRowsHost {
        std::vector<uint32_t> rows;
        Stamp at;
        uint64_t dead = 0;
        bool current(const zh_index *ix) const { return at.is(ix->n_rows, ix->dead_gen) && dead == ix->n_dead; }
        void mark_built(const zh_index *ix) { at.set(ix->n_rows, ix->dead_gen); dead = ix->n_dead; }
        void drop() { rows.clear(); rows.shrink_to_fit(); at.set(0, 0); dead = 0; }
    } live_host;
    // ... and on the device, as a list (path 1) and as a bitmap (path 2), for the exact family -- removed rows are never scored: for
    // (n_rows, dead_gen) (under mu, exclusive).  They survive every call; remove, clear and append leave the buffers to be refilled.
    struct LiveRowsDev {
        DevBuf rows, bits;
        Stamp at;
        uint64_t n_live = 0;  // (read only after exact_live_rows made the lists current)
        bool current(const zh_index *ix) const { return at.is(ix->n_rows, ix->dead_gen); }
        void mark_built(const zh_index *ix, uint64_t n) { n_live = n; at.set(ix->n_rows, ix->dead_gen); }
        void drop() { at.set(0, 0); rows.release(); bits.release(); }
    } live_dev;
    // The k-NN graph a caller attached for graph search (zh_index_set_graph, zh_gsearch.hip): zh_launch_refine_rows' table of u32 row numbers,
    // [g_rows][g_k], for the row numbering of the moment of the attach.  Not derived from anything the index holds: nothing re-makes it, an event
    // that renumbers or drops the rows drops it, every other event leaves it (rows keep their numbers; the search judges liveness itself).
    // Under mu: written exclusively, read by the search under the same lock and by zh_index_graph_info under the shared one.
    struct GraphView {
        DevBuf tab;
        bool attached = false;
        uint64_t rows = 0;
        uint32_t k = 0;
        void mark_attached(uint64_t g_rows, uint32_t g_k) { attached = true; rows = g_rows; k = g_k; }
        void drop() { tab.release(); attached = false; rows = 0; k = 0; }
    } graph;
    // graph search's per-call scratch (all released before the call returns): the queries' squared norms, {seeds, iterations, expanded, keyed,
    // capped}, and the host entry's staged batch: queries, seeds, ids, keys, counts
    DevBuf gs_QQ, gs_ctr, gs_Q, gs_seeds, gs_oids, gs_okeys, gs_ocounts;
    zh_graph_search_info gs_info{};  // (stats_mu)
    zh_graph_filtered_info gf_info{};  // (stats_mu)
    zh_graph_steered_info gt_info{};  // (stats_mu)
    // the graph extension's per-call scratch beside graph search's (all released before the call returns): a chunk's gathered seed lines and the
    // walk's answer for it, every stored row's squared norm, in-degrees, fill cursors, 64-bit offsets and the scan's block sums over the rows before
    // the chunk, the chunk's transposed edges, the touched rows, {the walk's five counters, touched rows of the chunk, rows re-ranked, offered, kept,
    // the transposition's two}; zh_index_get_graph's host entry stages through graph search's gs_oids / gs_ocounts
    DevBuf ge_seeds, ge_ids, ge_keys, ge_counts, ge_qq, ge_deg, ge_cur, ge_off, ge_sums, ge_csr, ge_touched, ge_ctr;
    zh_graph_extend_info ge_info{};  // (stats_mu)
    // What the index remembers of paths that did not pay on its data, and how long its forest has stood.
    struct Fallbacks {
        // Both derived views of the forest cost host time per build (a traversal of every node: ~0.35 s for the 13M nodes of a 1M-row forest at the
        // default leaf size), so a forest that changes between searches (insert, search, insert, ...) keeps the pointer walk / the
        // leaf-major sweep: the views are built once the forest has served a few batches unchanged.
        std::atomic<uint32_t> batches_since_change{0};
        // batches in a row that the prefilter handed back to the sweep (a list ran over: rows the bound cannot tell apart, many long
        // leaves): after two the forest is swept until it changes -- such data would pay for both every batch
        std::atomic<uint32_t> prefilter_strikes{0};
        // a batch whose half-width scan ran over was redone by the f32 scan: both scans paid.  Data whose keys are dense around the cut (the
        // parity cosine key on iid rows in 20k-row leaves: thousands of rows per query inside the bound) would do so batch after batch:
        // after the first such batch -- or one whose lists came close -- the per-query lists get 8192 slots instead of 4096 (a final
        // kernel with twice the LDS); after the second the index keeps the f32 scan until its trees change
        std::atomic<uint32_t> approx_strikes{0};
        // the matrix-core scan on f32 rows (no fp16 copy) rounds the rows as well: wider intervals, longer lists.  Lists that run over at 8192 slots send the
        // index back to the VALU half-width scan (which rounds the queries only) instead of all the way to the f32 scan
        std::atomic<bool> mfma_f32_off{false};
        // ... and a FUSED d = 128 sweep whose lists ran over (it hands on what the bounds known at the time cannot rule out: more than the select pass's exact
        // per-visit bounds would) goes back to the unfused half-width sweep first, not to the f32 sweep
        std::atomic<bool> fused_off{false};
        void prefilter_ran_over() { prefilter_strikes.fetch_add(1); }
        void prefilter_held() { prefilter_strikes = 0; }
        void approx_ran_over(bool mfma_on_f32_rows, bool fused_leaf) {
            if (mfma_on_f32_rows && approx_strikes.load() >= 1) mfma_f32_off = true;  // (8192-slot lists ran over: the VALU scan next)
            else if (fused_leaf && !fused_off) fused_off = true;                     // (the fused sweep's lists ran over: the select pass next)
            else approx_strikes.fetch_add(1);
        }
        void approx_nearly_ran_over() { approx_strikes.fetch_add(1); }
        void new_trees() { prefilter_strikes = 0; approx_strikes = 0; mfma_f32_off = false; fused_off = false; }  // (they were measured on the old ones)
        void trees_settle_again() { batches_since_change = 0; }
    } fb;
    bool scan_unsafe = false;  // an injected forest lists a row twice in one tree: rowLeaf holds one slot per (row, tree) -> leaf-major only
    double visits_per_pair = 0;  // leaf visits per (query, tree) pair, running mean over the batches so far (stats_mu)
    int profiling = 0;
    std::mutex stats_mu;
    zh_stats_t stats{};
    // Combining front end of zh_search_batch (the crate calls LSHIndex::search with ONE query from many rayon workers,
    // core.rs:299-303): callers that arrive while a batch is on the GPU queue their requests; the thread that finds the engine
    // idle leads -- it runs every compatible queued request (same top_k, metric, mode) as ONE internal batch and hands out the
    // results -- and the others sleep on the condition variable until theirs is done.
    struct CombineReq {
        const float *q; size_t b, k; int metric, mode;
        uint64_t *ids, *keys; uint32_t *counts;
        int rc = 0; std::string err;
        // completion and the appointment as next leader travel on the request's OWN mutex / condition variable: a finished round
        // wakes its callers side by side (one shared condition variable made 64 woken threads queue for one mutex)
        std::mutex m; std::condition_variable cv; bool done = false, lead = false;
    };
    // The lane a round runs on: a search context, a stream and staging of its own (not the index's blocking context: zh_search_batch
    // holds the index lock SHARED, zh_search_batch_device / add / remove exclusively).  One lane: a second one, so that one round's
    // host work overlaps the other's kernels, was measured slower (67 k against 80 k calls/s from 64 threads: rounds half the
    // size, and the HIP runtime serialises the two host threads' launches anyway).
    struct Lane {
        zh_search_ctx ctx;
        bool init = false, busy = false;
        hipStream_t s = nullptr;
        // a large host-resident batch is cut into windows that alternate between two contexts (search_host_windows): the second one
        zh_search_ctx ctx2;
        bool init2 = false;
        hipStream_t s2 = nullptr;
        // ... and, where hash + walk of a window outweigh its sweep (the crate's default options: thousands of leaf visits per pair), a third:
        // window w + 1 is BEGUN before window w is finished (its hash runs beside w's walk), as bench.py's look-ahead loop does (round 6)
        zh_search_ctx ctx3;
        bool init3 = false;
        hipStream_t s3 = nullptr;
        // ... and a fourth for TWO windows begun ahead (the finish of window w + 1 -- its walk -- is then queued before window w's results are
        // waited for: w's prefilter and select run beside it)
        zh_search_ctx ctx4;
        bool init4 = false;
        hipStream_t s4 = nullptr;
        hipEvent_t ev_d2h[4] = {nullptr, nullptr, nullptr, nullptr};
        DevBuf wQ, wOutIds, wOutKeys, wOutCounts;
        void *h_stage = nullptr;  // pinned staging of a combined batch: queries in, results out (one H2D, three D2H per round)
        size_t h_stage_cap = 0;
    };
    std::mutex cmu;
    std::deque<CombineReq *> cpend;
    bool cleader = false;   // some thread is leading (running rounds or about to)
    size_t clast = 0;       // callers served by the previous round
    Lane lanes[1];
};

// ------------------------------------------------------------------------------------------------
// What each mutation of the index does to its derived views: one routine per event, every view it touches named in it (DESIGN.md s4 has the
// same as a table).  The callers hold `mu` exclusively.  A view that is not named keeps its state through the event.
// ------------------------------------------------------------------------------------------------
// the fp16 copies' device bytes (zh_stats, zh_compact_info): the tiles and per-row scales, the d = 128 copy, the scan's row order and its view
// of row -> leaf (under blk_mu)
static uint64_t row_copy_bytes(const zh_index *ix) {
    return ix->half.tiles.cap + ix->half.meta.cap + ix->half128.copy.cap + ix->order.perm.cap + ix->order.row_leaf_p.cap;
}

// The trees are gone (before a build, a set_forest, a load; clear; destroy).
static void views_trees_dropped(zh_index *ix) {
    ix->blocks.drop();
    ix->leaf_meta.drop();
    ix->fb.new_trees();  // (batches_since_change is not reset here: upload_nodes, which every new forest goes through, does it)
    ix->row_leaf.drop();
    {
        // the matrix-core scan's row order was measured on THIS forest's leaves: the next half-width batch re-makes the copy in the new forest's
        // order, and an order given up for lack of room gets another chance.  A copy in id order is as good under the next forest.
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if (ix->order.used()) ix->half.remake();
        ix->order.allow();
    }
    ix->samples.drop();
    ix->plane_norms.drop();
}

// The trees changed in place or were just uploaded (build, set_forest, load, every incremental add and remove: the tail of upload_nodes).  The
// views' buffers stay -- the next build of each reuses them.
static void views_trees_changed(zh_index *ix) {
    ix->blocks.invalidate();
    ix->leaf_meta.invalidate();
    ix->fb.new_trees();
    ix->row_leaf.invalidate();
    ix->fb.trees_settle_again();  // (the forest's views wait until it has served a few batches unchanged)
}

// The table was emptied (zh_index_clear, after views_trees_dropped and after rows_gen and dead_gen were bumped): everything derived from the
// rows that were just dropped.  (The row norms and the sampler's live rows were once keyed on counts alone: a refill to the same count found
// them "valid".)  LiveRowsDev is not named: dead_gen moved, so its stamp is stale, and its buffers are refilled in place.
static void views_table_emptied(zh_index *ix) {
    ix->norms.drop();
    ix->graph.drop();  // (its lines name rows that are gone)
    std::lock_guard<std::mutex> lb(ix->blk_mu);  // (the fp16 copies' state is blk_mu's: zh_stats reads it under that lock)
    ix->half.drop();
    ix->order.drop();
    ix->order.allow();  // (a new table gets a new chance at the scan's row order)
    ix->half128.drop();
    ix->half128.not_bytes = false;  // (the row that was not of bytes went with the others)
    ix->live_host.drop();
}

// The rows moved (zh_index_compact, after rows_gen and dead_gen were bumped): the trees stand, with their leaf ids renumbered.  lost_sample: some
// plane's sample row was among the removed.  -> the device bytes of the fp16 copies that were released.
static uint64_t views_rows_moved(zh_index *ix, bool lost_sample) {
    ix->live_host.drop();
    ix->live_dev.drop();  // (the buffers too: they were sized by the old row count; re-made by the next exact search)
    ix->graph.drop();     // (its lines hold the old row numbers: the caller attaches a graph of the new ones)
    ix->norms.drop();
    ix->plane_norms.forget();
    if (lost_sample) ix->samples.mark(false);  // (no row scores for that plane's sign until the forest is rebuilt)
    ix->leaf_meta.drop();
    ix->row_leaf.drop();
    ix->row_leaf.rows = 0;
    std::lock_guard<std::mutex> lb(ix->blk_mu);  // (the fp16 copies' state is blk_mu's: zh_stats reads it under that lock)
    ix->blocks.invalidate();
    const uint64_t released = row_copy_bytes(ix);
    ix->half.drop();
    ix->order.drop();    // (order.off stays: DESIGN.md s4, "kept as found")
    ix->half128.drop();  // (not_bytes stays: a table with a row that is not of bytes still has one, or lost it and finds out when the copy is next made)
    return released;
}

static const char *const k_torn_msg = "an earlier zh_index_compact failed after rows had begun to move: the stored rows are inconsistent; "
                                      "zh_index_clear the index and store them again";
static int set_device(const zh_index *ix) {
    hipError_t e = hipSetDevice(ix->device);
    if (e != hipSuccess) return fail(ZH_EHIP, "hipSetDevice(%d): %s", ix->device, hipGetErrorString(e));
    return ZH_OK;
}

static ZhForestDev forest_dev(const zh_index *ix) {
    ZhForestDev f;
    f.node_plane = ix->node_plane.as<int32_t>();
    f.node_left = ix->node_left.as<int32_t>();
    f.node_right = ix->node_right.as<int32_t>();
    f.node_pack = ix->node_pack.as<int4>();
    f.roots = ix->roots.as<uint32_t>();
    f.planes = ix->planes.as<float>();
    f.consts = ix->consts.as<float>();
    f.leaf_ids = ix->leaf_ids.as<uint32_t>();
    f.n_nodes = ix->n_nodes;
    f.n_planes = ix->n_planes;
    f.n_trees = ix->n_trees;
    f.group = zh_group_size(ix->opt.dim);
    return f;
}

static int ctx_init(zh_search_ctx *c, zh_index *ix) {
    c->ix = ix;
    for (DevBuf *b : c->all_bufs()) b->defer = true;  // never hipFree (a device-wide drain) between batches
    hipError_t e = hipHostMalloc((void **)&c->h_totals, sizeof(ZhTotals), hipHostMallocDefault);
    if (e != hipSuccess) return fail(ZH_ENOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    e = hipHostMalloc((void **)&c->h_pf, 4 * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(ZH_ENOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    memset(c->h_pf, 0, 4 * sizeof(uint32_t));
    e = hipHostMalloc((void **)&c->h_ap, ZH_APX_CTL_WORDS * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) return fail(ZH_ENOMEM, "hipHostMalloc: %s", hipGetErrorString(e));
    memset(c->h_ap, 0, ZH_APX_CTL_WORDS * sizeof(uint32_t));
    for (auto &ev : c->ev) HIPCHK(hipEventCreate(&ev));
    HIPCHK(hipEventCreateWithFlags(&c->ev_totals, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_emit, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&c->ev_sw0));
    HIPCHK(hipEventCreate(&c->ev_sw1));
    c->ev_ok = true;
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" void zh_options_default(zh_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_node_size = 5;  // lsh.rs:134
    o->num_trees = 15;     // lsh.rs:135
    o->seed = 0x5EB2A003ull;
    o->device = -1;
}

extern "C" int zh_index_create(const zh_options *opt, zh_index **out) {
    if (!opt || !out) return fail(ZH_EINVAL, "zh_index_create: null argument");
    if (opt->dim == 0) return fail(ZH_EINVAL, "zh_index_create: dim must be > 0");
    if (opt->dim > ZH_MAX_DIM) return fail(ZH_ELIMIT, "zh_index_create: dim %u > ZH_MAX_DIM (%u)", opt->dim, ZH_MAX_DIM);
    if (opt->num_trees > 4096) return fail(ZH_ELIMIT, "zh_index_create: num_trees > 4096");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(ZH_EHIP, "no usable HIP device (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    zh_index *ix = new (std::nothrow) zh_index();
    if (!ix) return fail(ZH_ENOMEM, "out of host memory");
    ix->opt = *opt;
    if (opt->device < 0) {
        if (hipGetDevice(&ix->device) != hipSuccess) ix->device = 0;
    } else
        ix->device = opt->device;
    if (ix->device >= ndev) { delete ix; return fail(ZH_EINVAL, "device %d out of range (%d devices)", opt->device, ndev); }
    int rc = set_device(ix);
    if (rc) { delete ix; return rc; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ix->device) == hipSuccess) {
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            delete ix;
            return fail(ZH_EHIP, "device %d is %s; this library is built for gfx950 only", opt->device, prop.gcnArchName);
        }
    }
    e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ix; return fail(ZH_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
        e = hipStreamCreateWithPriority(&ix->sweep_stream, hipStreamNonBlocking, least);
        if (e != hipSuccess) { hipStreamDestroy(ix->stream); delete ix; return fail(ZH_EHIP, "hipStreamCreateWithPriority: %s", hipGetErrorString(e)); }
    }
    rc = ctx_init(&ix->dctx, ix);
    if (rc) { hipStreamDestroy(ix->sweep_stream); hipStreamDestroy(ix->stream); delete ix; return rc; }
    if (opt->reserve_rows) {
        rc = ix->X.ensure((size_t)opt->reserve_rows * opt->dim * sizeof(float));
        if (rc) { zh_index_destroy(ix); return rc; }
    }
    *out = ix;
    return ZH_OK;
}

static void free_forest(zh_index *ix) {
    ix->node_plane.release(); ix->node_left.release(); ix->node_right.release(); ix->node_pack.release(); ix->roots.release();
    ix->planes.release(); ix->consts.release(); ix->leaf_ids.release();
    views_trees_dropped(ix);
    ix->scan_unsafe = false;  // (a property of the forest that is going, not of a view: set_forest and load say what the next one is)
    ix->n_nodes = ix->n_planes = ix->n_trees = 0;
    ix->n_leaf_ids = 0;
    ix->h_plane.clear(); ix->h_left.clear(); ix->h_right.clear(); ix->h_roots.clear();
    ix->planes_below_level.clear();
    ix->h_leaf_ids.clear();
    ix->max_leaf_len = 0;
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->visits_per_pair = 0;
    }
}

static void release_scratch(zh_index *ix, unsigned families);  // (the exact family's per-call scratch, below)
extern "C" void zh_index_destroy(zh_index *ix) {
    if (ix)
        for (auto &ln : ix->lanes) {
            if (ln.init) { hipSetDevice(ix->device); ln.ctx.release_all(); }
            if (ln.init2) { hipSetDevice(ix->device); ln.ctx2.release_all(); }
            if (ln.init3) { hipSetDevice(ix->device); ln.ctx3.release_all(); }
            if (ln.init4) { hipSetDevice(ix->device); ln.ctx4.release_all(); }
            if (ln.s2) hipStreamDestroy(ln.s2);
            if (ln.s3) hipStreamDestroy(ln.s3);
            if (ln.s4) hipStreamDestroy(ln.s4);
            for (auto &ev : ln.ev_d2h) if (ev) hipEventDestroy(ev);
            ln.wQ.release(); ln.wOutIds.release(); ln.wOutKeys.release(); ln.wOutCounts.release();
            if (ln.s) hipStreamDestroy(ln.s);
            if (ln.h_stage) hipHostFree(ln.h_stage);
        }
    if (!ix) return;
    hipSetDevice(ix->device);
    if (ix->stream) hipStreamSynchronize(ix->stream);
    if (ix->sweep_stream) hipStreamSynchronize(ix->sweep_stream);
    free_forest(ix);
    ix->X.release();
    ix->norms.drop(); ix->half.drop(); ix->half.rho_dev.release(); ix->half128.drop(); ix->order.drop(); ix->live_dev.drop();
    ix->graph.drop();
    ix->dctx.release_all();
    DevBuf *ws[] = {&ix->wQ, &ix->wOutIds, &ix->wOutKeys, &ix->wOutCounts};
    release_scratch(ix, ~0u);  // every family's
    for (DevBuf *b : ws) b->release();
    if (ix->sweep_stream) hipStreamDestroy(ix->sweep_stream);
    if (ix->stream) hipStreamDestroy(ix->stream);
    delete ix;
}

extern "C" int zh_index_clear(zh_index *ix) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    hipStreamSynchronize(ix->stream);
    free_forest(ix);
    ix->broken = false; ix->rows_torn = false;
    ix->n_rows = 0;
    ix->h_dead.clear();
    ix->n_dead = 0;
    ix->rows_gen++; ix->dead_gen++;
    views_table_emptied(ix);
    return ZH_OK;
}

extern "C" uint64_t zh_index_count(const zh_index *ix) { return ix ? ix->n_rows - ix->n_dead : 0; }
extern "C" uint32_t zh_index_num_trees(const zh_index *ix) { return ix ? ix->n_trees : 0; }
extern "C" uint64_t zh_index_stored_rows(const zh_index *ix) { return ix ? ix->n_rows : 0; }
extern "C" uint32_t zh_index_dim(const zh_index *ix) { return ix ? ix->opt.dim : 0; }
extern "C" int32_t zh_index_device(const zh_index *ix) { return ix ? ix->device : -1; }
extern "C" uint64_t zh_index_id_base(const zh_index *ix) { return ix ? ix->opt.id_base : 0; }
extern "C" const float *zh_index_rows_device(const zh_index *ix) { return ix ? ix->X.as<float>() : nullptr; }
extern "C" void *zh_index_sweep_stream(const zh_index *ix) { return ix ? (void *)ix->sweep_stream : nullptr; }

// ------------------------------------------------------------------------------------------------
// rows
// ------------------------------------------------------------------------------------------------
static int grow_rows(zh_index *ix, size_t n_more) {
    size_t need = (size_t)(ix->n_rows + n_more) * ix->opt.dim * sizeof(float);
    if (ix->n_rows + n_more > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "more than 2^32-1 rows in one index (shard it)");
    return ix->X.ensure(need, true, ix->stream);
}

static int append_locked(zh_index *ix, const float *rows, size_t n, uint64_t *out_ids) {
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if ((rc = grow_rows(ix, n))) return rc;
    if (n) {
        HIPCHK(hipMemcpyAsync(ix->X.as<float>() + (size_t)ix->n_rows * ix->opt.dim, rows,
                              n * ix->opt.dim * sizeof(float), hipMemcpyHostToDevice, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
    }
    if (out_ids) for (size_t i = 0; i < n; i++) out_ids[i] = ix->opt.id_base + ix->n_rows + i;
    ix->n_rows += n;
    return ZH_OK;
}
extern "C" int zh_index_append(zh_index *ix, const float *rows, size_t n, uint64_t *out_ids) {
    if (!ix || (!rows && n)) return fail(ZH_EINVAL, "zh_index_append: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    return append_locked(ix, rows, n, out_ids);
}

extern "C" int zh_index_read_rows(zh_index *ix, uint64_t first, size_t n, float *out) {
    if (!ix || (n && !out)) return fail(ZH_EINVAL, "zh_index_read_rows: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (first + n > ix->n_rows) return fail(ZH_EINVAL, "zh_index_read_rows: rows [%llu, %llu) out of range (%llu stored)",
                                            (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)ix->n_rows);
    if (n) HIPCHK(hipMemcpy(out, ix->X.as<float>() + (size_t)first * ix->opt.dim, n * ix->opt.dim * sizeof(float), hipMemcpyDeviceToHost));
    return ZH_OK;
}

extern "C" int zh_index_append_device(zh_index *ix, const float *d_rows, size_t n) {
    if (!ix || (!d_rows && n)) return fail(ZH_EINVAL, "zh_index_append_device: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if ((rc = grow_rows(ix, n))) return rc;
    if (n) {
        HIPCHK(hipMemcpyAsync(ix->X.as<float>() + (size_t)ix->n_rows * ix->opt.dim, d_rows,
                              n * ix->opt.dim * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
    }
    ix->n_rows += n;
    return ZH_OK;
}

extern "C" int zh_index_append_synthetic(zh_index *ix, size_t n, uint64_t seed, uint64_t first_row, int kind) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if ((rc = grow_rows(ix, n))) return rc;
    HIPCHK(zh_launch_synth_rows(ix->X.as<float>() + (size_t)ix->n_rows * ix->opt.dim, n, ix->opt.dim, seed, first_row,
                                kind, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->n_rows += n;
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// forest upload (shared by set_forest and build): node arrays on the host, planes level-major
// ------------------------------------------------------------------------------------------------
static int upload_nodes(zh_index *ix) {
    size_t nn = ix->h_plane.size();
    int rc;
    if ((rc = ix->node_plane.ensure(std::max<size_t>(nn, 1) * 4))) return rc;
    if ((rc = ix->node_left.ensure(std::max<size_t>(nn, 1) * 4))) return rc;
    if ((rc = ix->node_right.ensure(std::max<size_t>(nn, 1) * 4))) return rc;
    if ((rc = ix->node_pack.ensure(std::max<size_t>(nn, 1) * sizeof(int4)))) return rc;
    if ((rc = ix->roots.ensure(std::max<size_t>(ix->h_roots.size(), 1) * 4))) return rc;
    if (nn) {
        HIPCHK(hipMemcpyAsync(ix->node_plane.p, ix->h_plane.data(), nn * 4, hipMemcpyHostToDevice, ix->stream));
        HIPCHK(hipMemcpyAsync(ix->node_left.p, ix->h_left.data(), nn * 4, hipMemcpyHostToDevice, ix->stream));
        HIPCHK(hipMemcpyAsync(ix->node_right.p, ix->h_right.data(), nn * 4, hipMemcpyHostToDevice, ix->stream));
        // the plane constants are final on this stream by now (set_forest's copy, make_planes of build / insert)
        HIPCHK(zh_launch_pack_nodes(ix->node_plane.as<int32_t>(), ix->node_left.as<int32_t>(), ix->node_right.as<int32_t>(),
                                    ix->consts.as<float>(), ix->node_pack.as<int4>(), (uint32_t)nn, ix->stream));
    }
    if (!ix->h_roots.empty())
        HIPCHK(hipMemcpyAsync(ix->roots.p, ix->h_roots.data(), ix->h_roots.size() * 4, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->n_nodes = (uint32_t)nn;
    ix->n_trees = (uint32_t)ix->h_roots.size();
    views_trees_changed(ix);
    ix->max_leaf_len = 0;
    for (size_t i = 0; i < nn; i++)
        if (ix->h_plane[i] < 0) ix->max_leaf_len = std::max(ix->max_leaf_len, (uint32_t)ix->h_right[i]);
    return ZH_OK;
}

// What zh_index_set_forest requires of a forest over n_rows stored rows (zh_index_load applies the same tests to a snapshot's forest): every
// node reachable once, indices and leaf ranges in bounds, leaf ids below the stored rows, at most 63 levels.  Leaves behind the level of every
// node, the inner nodes per level, and whether a tree lists a row twice.
struct ForestCheck {
    std::vector<int32_t> level;
    std::vector<std::vector<uint32_t>> by_level;
    bool dup_in_tree = false;
};
static int check_forest(const zh_forest_view *fv, uint64_t n_rows, ForestCheck &fc) {
    const uint32_t nn = fv->n_nodes, np = fv->n_planes, nt = fv->n_trees;
    std::vector<int32_t> &level = fc.level;
    std::vector<std::vector<uint32_t>> &by_level = fc.by_level;
    bool &dup_in_tree = fc.dup_in_tree;
    if (nt && (!fv->roots || !fv->plane || !fv->left || !fv->right)) return fail(ZH_EINVAL, "set_forest: null arrays");
    if (np && (!fv->planes || !fv->consts)) return fail(ZH_EINVAL, "set_forest: null plane arrays");
    if (fv->n_leaf_ids && !fv->leaf_ids) return fail(ZH_EINVAL, "set_forest: null leaf_ids");
    if (fv->n_leaf_ids > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "set_forest: more than 2^32-1 leaf entries");
    // validate + level of every node (BFS per tree)
    level.assign(nn, -1);
    by_level.clear();
    std::vector<std::pair<uint32_t, uint32_t>> tree_leaves;  // (tree, leaf node)
    for (uint32_t t = 0; t < nt; t++) {
        if (fv->roots[t] >= nn) return fail(ZH_EINVAL, "set_forest: root %u out of range", t);
        std::vector<uint32_t> cur{fv->roots[t]}, nxt;
        int32_t lv = 0;
        while (!cur.empty()) {
            if ((size_t)lv >= by_level.size()) by_level.resize(lv + 1);
            for (uint32_t n : cur) {
                if (level[n] >= 0) return fail(ZH_EINVAL, "set_forest: node %u reachable twice", n);
                level[n] = lv;
                if (fv->plane[n] >= 0) {
                    if ((uint32_t)fv->plane[n] >= np) return fail(ZH_EINVAL, "set_forest: plane index out of range at node %u", n);
                    if (fv->left[n] < 0 || (uint32_t)fv->left[n] >= nn || fv->right[n] < 0 || (uint32_t)fv->right[n] >= nn)
                        return fail(ZH_EINVAL, "set_forest: child index out of range at node %u", n);
                    by_level[lv].push_back(n);
                    nxt.push_back((uint32_t)fv->left[n]);
                    nxt.push_back((uint32_t)fv->right[n]);
                } else {
                    uint64_t off = (uint32_t)fv->left[n], len = (uint32_t)fv->right[n];
                    if (fv->right[n] < 0 || off + len > fv->n_leaf_ids) return fail(ZH_EINVAL, "set_forest: leaf range out of bounds at node %u", n);
                    tree_leaves.push_back({t, n});
                }
            }
            cur.swap(nxt);
            nxt.clear();
            lv++;
            if (lv > 63) return fail(ZH_ELIMIT, "set_forest: tree deeper than 63 levels");
        }
    }
    for (uint64_t i = 0; i < fv->n_leaf_ids; i++)
        if (fv->leaf_ids[i] >= n_rows) return fail(ZH_EINVAL, "set_forest: leaf id %u >= stored rows %llu", fv->leaf_ids[i], (unsigned long long)n_rows);
    // A row listed twice inside ONE tree (a repeated id, or two leaves of a tree over the same leaf_ids range) is legal input --
    // the leaf-major sweep scores every listed occurrence -- but the table scan keeps one {leaf, position} per (row, tree): such
    // a forest is served leaf by leaf only, whatever the cost model or zh_set_sweep_mode say, so results never depend on the sweep.
    dup_in_tree = false;
    {
        std::vector<uint32_t> stamp(n_rows, 0xFFFFFFFFu);
        for (size_t i = 0; i < tree_leaves.size() && !dup_in_tree; i++) {
            const uint32_t t = tree_leaves[i].first, n = tree_leaves[i].second;
            const uint32_t off = (uint32_t)fv->left[n], len = (uint32_t)fv->right[n];
            for (uint32_t j = 0; j < len; j++) {
                const uint32_t r = fv->leaf_ids[(size_t)off + j];
                if (stamp[r] == t) { dup_in_tree = true; break; }
                stamp[r] = t;
            }
        }
    }
    return ZH_OK;
}

extern "C" int zh_index_set_forest(zh_index *ix, const zh_forest_view *fv) {
    if (!ix || !fv) return fail(ZH_EINVAL, "zh_index_set_forest: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    const uint32_t nn = fv->n_nodes, np = fv->n_planes, nt = fv->n_trees, d = ix->opt.dim;
    ForestCheck fc;
    if ((rc = check_forest(fv, ix->n_rows, fc))) return rc;
    const std::vector<int32_t> &level = fc.level;
    const std::vector<std::vector<uint32_t>> &by_level = fc.by_level;
    const bool dup_in_tree = fc.dup_in_tree;
    // renumber planes level-major
    std::vector<int32_t> new_of_old(np, -1);
    std::vector<uint32_t> old_of_new;
    std::vector<uint32_t> below{0};
    for (auto &lvl : by_level) {
        for (uint32_t n : lvl) {
            uint32_t op = (uint32_t)fv->plane[n];
            if (new_of_old[op] < 0) { new_of_old[op] = (int32_t)old_of_new.size(); old_of_new.push_back(op); }
        }
        below.push_back((uint32_t)old_of_new.size());
    }
    hipStreamSynchronize(ix->stream);
    free_forest(ix);
    ix->h_plane.assign(fv->plane, fv->plane + nn);
    ix->h_left.assign(fv->left, fv->left + nn);
    ix->h_right.assign(fv->right, fv->right + nn);
    ix->h_roots.assign(fv->roots, fv->roots + nt);
    for (uint32_t n = 0; n < nn; n++)
        if (ix->h_plane[n] >= 0) ix->h_plane[n] = level[n] >= 0 ? new_of_old[ix->h_plane[n]] : 0;
    const uint32_t np_used = (uint32_t)old_of_new.size();
    std::vector<float> hp((size_t)std::max<uint32_t>(np_used, 1) * d), hc(std::max<uint32_t>(np_used, 1));
    for (uint32_t i = 0; i < np_used; i++) {
        memcpy(&hp[(size_t)i * d], fv->planes + (size_t)old_of_new[i] * d, d * sizeof(float));
        hc[i] = fv->consts[old_of_new[i]];
    }
    if ((rc = ix->planes.ensure(hp.size() * 4))) return rc;
    if ((rc = ix->consts.ensure(hc.size() * 4))) return rc;
    if ((rc = ix->leaf_ids.ensure(std::max<uint64_t>(fv->n_leaf_ids, 1) * 4))) return rc;
    HIPCHK(hipMemcpyAsync(ix->planes.p, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(ix->consts.p, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, ix->stream));
    if (fv->n_leaf_ids)
        HIPCHK(hipMemcpyAsync(ix->leaf_ids.p, fv->leaf_ids, fv->n_leaf_ids * 4, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->n_planes = np_used;
    ix->n_leaf_ids = fv->n_leaf_ids;
    ix->planes_below_level = below;
    ix->scan_unsafe = dup_in_tree;
    return upload_nodes(ix);
}

extern "C" int zh_index_forest_sizes(zh_index *ix, zh_forest_sizes *out) {
    if (!ix || !out) return fail(ZH_EINVAL, "null argument");
    out->n_nodes = ix->n_nodes; out->n_planes = ix->n_planes; out->n_trees = ix->n_trees; out->n_leaf_ids = ix->n_leaf_ids;
    return ZH_OK;
}

extern "C" int zh_index_get_forest(zh_index *ix, int32_t *plane, int32_t *left, int32_t *right, uint32_t *roots,
                                   float *planes, float *consts, uint32_t *leaf_ids) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (plane) memcpy(plane, ix->h_plane.data(), ix->h_plane.size() * 4);
    if (left) memcpy(left, ix->h_left.data(), ix->h_left.size() * 4);
    if (right) memcpy(right, ix->h_right.data(), ix->h_right.size() * 4);
    if (roots) memcpy(roots, ix->h_roots.data(), ix->h_roots.size() * 4);
    if (planes && ix->n_planes) HIPCHK(hipMemcpy(planes, ix->planes.p, (size_t)ix->n_planes * ix->opt.dim * 4, hipMemcpyDeviceToHost));
    if (consts && ix->n_planes) HIPCHK(hipMemcpy(consts, ix->consts.p, (size_t)ix->n_planes * 4, hipMemcpyDeviceToHost));
    if (leaf_ids && ix->n_leaf_ids) HIPCHK(hipMemcpy(leaf_ids, ix->leaf_ids.p, ix->n_leaf_ids * 4, hipMemcpyDeviceToHost));
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// GPU forest build (build_index, lsh.rs:411-429 -> build_a_tree lsh.rs:250-267), level-synchronous
// ------------------------------------------------------------------------------------------------
static inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// two distinct rows uniform over the whole database (lsh.rs:197-201), keyed by (seed, tree, heap path)
static void sample_pair(uint64_t seed, uint32_t tree, uint64_t path, uint64_t n_rows, uint64_t *i, uint64_t *j) {
    uint64_t h = splitmix64(seed ^ splitmix64(0x7EE5ull + tree) ^ splitmix64(path * 0xC2B2AE3D27D4EB4Full));
    uint64_t h1 = splitmix64(h), h2 = splitmix64(h1);
    if (n_rows < 2) { *i = 0; *j = 0; return; }
    *i = h1 % n_rows;
    *j = h2 % (n_rows - 1);
    if (*j >= *i) (*j)++;
}

// The two sample rows of a split come from the LIVE rows among the first n_sample: LSHIndex::remove deletes the embedding from
// the store (lsh.rs:495) and build_hyperplane samples the stored embeddings only (lsh.rs:197-201), so a removed row never
// defines a plane.  Returns the live count (< 2: default zero vectors, lsh.rs:203-220).  Same mapping as the oracle's.
static uint64_t sample_live_pair(zh_index *ix, uint32_t tree, uint64_t path, uint64_t n_sample, uint64_t *si, uint64_t *sj) {
    if (ix->n_dead == 0) { sample_pair(ix->opt.seed, tree, path, n_sample, si, sj); return n_sample; }
    std::vector<uint32_t> &live = ix->live_host.rows;
    if (!ix->live_host.current(ix)) {
        live.clear();
        live.reserve(ix->n_rows - ix->n_dead);
        for (uint64_t r = 0; r < ix->n_rows; r++)
            if (!(r < ix->h_dead.size() && ix->h_dead[r])) live.push_back((uint32_t)r);
        ix->live_host.mark_built(ix);
    }
    const uint64_t n_live = (uint64_t)(std::lower_bound(live.begin(), live.end(), n_sample,
                                                        [](uint32_t a, uint64_t b) { return (uint64_t)a < b; }) - live.begin());
    sample_pair(ix->opt.seed, tree, path, n_live, si, sj);
    if (n_live) { *si = live[*si]; *sj = live[*sj]; }
    return n_live;
}

struct ActiveNode {   // a node whose id list (a segment of a perm array) is to be split
    uint32_t node, tree, len, depth;
    uint64_t seg_start, path, n_sample;  // n_sample: size of the database the two sample rows are drawn from
};

// Split every active node, level after level, until all descendants are leaves (build_a_tree,
// lsh.rs:250-267).  d_perm holds the id lists as segments; leaves become runs of d_perm and get
// offset leaf_base + position.  New planes are appended to ix->planes from index n_planes on.
static int grow_segments(zh_index *ix, uint32_t *d_perm, uint64_t perm_len, std::vector<ActiveNode> active,
                         uint64_t leaf_base, uint32_t &n_planes, bool record_levels) {
    const uint32_t M = ix->opt.max_node_size, d = ix->opt.dim;
    hipStream_t s = ix->stream;
    int rc;
    DevBuf tmp, flags, dNodes, dChunks, dChunkAbove, dChunkScan, dScanTmp, dNodeAbove;
    struct Guard {
        std::vector<DevBuf *> v;
        ~Guard() { for (auto *b : v) b->release(); }
    } guard;
    guard.v = {&tmp, &flags, &dNodes, &dChunks, &dChunkAbove, &dChunkScan, &dScanTmp, &dNodeAbove};
    if (active.empty()) return ZH_OK;
    if ((rc = tmp.ensure(std::max<uint64_t>(perm_len, 1) * 4))) return rc;
    if ((rc = flags.ensure(std::max<uint64_t>(perm_len, 1)))) return rc;
    auto new_node = [&]() { ix->h_plane.push_back(-1); ix->h_left.push_back(0); ix->h_right.push_back(0); return (uint32_t)(ix->h_plane.size() - 1); };
    auto make_leaf = [&](uint32_t node, uint64_t start, uint32_t len) {
        ix->h_plane[node] = -1; ix->h_left[node] = (int32_t)(uint32_t)(leaf_base + start); ix->h_right[node] = (int32_t)len;
    };
    std::vector<ActiveNode> next;
    std::vector<ZhBuildNode> hn;
    std::vector<ZhBuildChunk> hc;
    std::vector<uint32_t> h_above;
    for (uint32_t round = 0; !active.empty(); round++) {
        hn.clear(); hc.clear();
        for (size_t i = 0; i < active.size(); i++) {
            const ActiveNode &a = active[i];
            ZhBuildNode bn;
            bn.seg_start = a.seg_start; bn.len = a.len; bn.plane = n_planes + (uint32_t)i;
            uint64_t si, sj;
            const uint64_t n_live = sample_live_pair(ix, a.tree, a.path, a.n_sample, &si, &sj);
            bn.sample_a = n_live >= 1 ? si : ~0ull;   // lsh.rs:203-220: a missing sample decodes to the zero vector
            bn.sample_b = n_live >= 2 ? sj : ~0ull;
            bn.first_chunk = (uint32_t)hc.size();
            bn.n_chunks = (a.len + 255) / 256;
            for (uint32_t c = 0; c < bn.n_chunks; c++) {
                ZhBuildChunk ch;
                ch.node = (uint32_t)i; ch.pos = a.seg_start + (uint64_t)c * 256;
                ch.count = std::min<uint32_t>(256, a.len - c * 256);
                hc.push_back(ch);
            }
            hn.push_back(bn);
        }
        const uint32_t na = (uint32_t)hn.size(), nc = (uint32_t)hc.size();
        if ((rc = ix->planes.ensure((size_t)(n_planes + na) * d * 4, true, s))) return rc;
        if ((rc = ix->consts.ensure((size_t)(n_planes + na) * 4, true, s))) return rc;
        if ((rc = dNodes.ensure(na * sizeof(ZhBuildNode)))) return rc;
        if ((rc = dChunks.ensure(std::max<uint32_t>(nc, 1) * sizeof(ZhBuildChunk)))) return rc;
        if ((rc = dChunkAbove.ensure((size_t)std::max<uint32_t>(nc, 1) * 4))) return rc;
        if ((rc = dChunkScan.ensure((size_t)(nc + 1) * 4))) return rc;
        if ((rc = dScanTmp.ensure(((size_t)nc / 1024 + 4) * 4))) return rc;
        if ((rc = dNodeAbove.ensure((size_t)na * 4))) return rc;
        {   // the planes' sample rows, for the row-score hash
            std::vector<uint2> hs(na);
            for (uint32_t i = 0; i < na; i++)
                hs[i] = make_uint2(hn[i].sample_a == ~0ull ? 0xFFFFFFFFu : (uint32_t)hn[i].sample_a,
                                   hn[i].sample_b == ~0ull ? 0xFFFFFFFFu : (uint32_t)hn[i].sample_b);
            if ((rc = ix->samples.pairs.ensure((size_t)(n_planes + na) * sizeof(uint2), true, s))) return rc;
            HIPCHK(hipMemcpy(ix->samples.pairs.as<uint2>() + n_planes, hs.data(), na * sizeof(uint2), hipMemcpyHostToDevice));
        }
        hipError_t e = hipMemcpyAsync(dNodes.p, hn.data(), na * sizeof(ZhBuildNode), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && nc) e = hipMemcpyAsync(dChunks.p, hc.data(), nc * sizeof(ZhBuildChunk), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(dNodeAbove.p, 0, (size_t)na * 4, s);
        if (e == hipSuccess) e = zh_launch_make_planes(ix->X.as<float>(), d, dNodes.as<ZhBuildNode>(), na, ix->planes.as<float>(), ix->consts.as<float>(), s);
        if (e == hipSuccess) e = zh_launch_classify(ix->X.as<float>(), d, d_perm, dNodes.as<ZhBuildNode>(), dChunks.as<ZhBuildChunk>(), nc, ix->planes.as<float>(), ix->consts.as<float>(), flags.as<uint8_t>(), dChunkAbove.as<uint32_t>(), s);
        if (e == hipSuccess) e = zh_launch_scan_u32(dChunkAbove.as<uint32_t>(), dChunkScan.as<uint32_t>(), nc, dScanTmp.as<uint32_t>(), s);
        if (e == hipSuccess) e = zh_launch_scatter(d_perm, tmp.as<uint32_t>(), dNodes.as<ZhBuildNode>(), dChunks.as<ZhBuildChunk>(), nc, flags.as<uint8_t>(), dChunkScan.as<uint32_t>(), dNodeAbove.as<uint32_t>(), s);
        h_above.resize(na);
        if (e == hipSuccess) e = hipMemcpyAsync(h_above.data(), dNodeAbove.p, (size_t)na * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(ZH_EHIP, "forest build round %u: %s", round, hipGetErrorString(e));
        next.clear();
        for (size_t i = 0; i < active.size(); i++) {
            const ActiveNode &a = active[i];
            uint32_t nA = h_above[i], nB = a.len - nA;
            uint32_t l = new_node(), r = new_node();
            ix->h_plane[a.node] = (int32_t)(n_planes + i);
            ix->h_left[a.node] = (int32_t)l;   // below  (lsh.rs:262)
            ix->h_right[a.node] = (int32_t)r;  // above  (lsh.rs:263)
            bool child_can_split = a.depth + 1 < ZH_MAX_DEPTH;
            if (nB >= M && child_can_split) next.push_back({l, a.tree, nB, a.depth + 1, a.seg_start, 2 * a.path, a.n_sample});
            else make_leaf(l, a.seg_start, nB);
            if (nA >= M && child_can_split) next.push_back({r, a.tree, nA, a.depth + 1, a.seg_start + nB, 2 * a.path + 1, a.n_sample});
            else make_leaf(r, a.seg_start + nB, nA);
        }
        n_planes += na;
        if (record_levels) ix->planes_below_level.push_back(n_planes);
        active.swap(next);
    }
    return ZH_OK;
}

static int build_forest_locked(zh_index *ix) {
    const uint64_t N = ix->n_rows;
    const uint32_t T = ix->opt.num_trees, M = ix->opt.max_node_size;
    int rc;
    hipStreamSynchronize(ix->stream);
    free_forest(ix);
    ix->broken = false;
    if ((uint64_t)T * N > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "num_trees * rows exceeds 2^32-1 leaf entries; shard the index");
    const uint64_t NL = N - ix->n_dead;  // removed rows stay out of a rebuild, as leaf members and as hyperplane samples
    const uint64_t total = (uint64_t)T * NL;
    DevBuf perm;
    if ((rc = perm.ensure(std::max<uint64_t>(total, 1) * 4))) return rc;
    if (total && ix->n_dead == 0) {
        hipError_t e = zh_launch_iota_perm(perm.as<uint32_t>(), N, T, ix->stream);
        if (e != hipSuccess) { perm.release(); return fail(ZH_EHIP, "iota_perm: %s", hipGetErrorString(e)); }
    } else if (total) {
        if (ix->h_dead.size() < N) ix->h_dead.resize(N, 0);  // rows appended after the last removal are alive
        std::vector<uint32_t> live;
        live.reserve(NL);
        for (uint64_t i = 0; i < N; i++) if (!ix->h_dead[i]) live.push_back((uint32_t)i);
        for (uint32_t t = 0; t < T; t++) {
            hipError_t e = hipMemcpy(perm.as<uint32_t>() + (size_t)t * NL, live.data(), NL * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) { perm.release(); return fail(ZH_EHIP, "perm upload: %s", hipGetErrorString(e)); }
        }
    }
    std::vector<ActiveNode> active;
    ix->planes_below_level.assign(1, 0);
    for (uint32_t t = 0; t < T; t++) {
        ix->h_plane.push_back(-1); ix->h_left.push_back(0); ix->h_right.push_back(0);
        uint32_t n = (uint32_t)(ix->h_plane.size() - 1);
        ix->h_roots.push_back(n);
        if (NL < M) { ix->h_left[n] = (int32_t)(uint32_t)((uint64_t)t * NL); ix->h_right[n] = (int32_t)NL; }  // lsh.rs:251-252
        else active.push_back({n, t, (uint32_t)NL, 0, (uint64_t)t * NL, 1, N});
    }
    uint32_t n_planes = 0;
    rc = grow_segments(ix, perm.as<uint32_t>(), total, active, 0, n_planes, true);
    if (rc) { perm.release(); free_forest(ix); return rc; }
    if (n_planes == 0) {
        if ((rc = ix->planes.ensure(4 * (size_t)ix->opt.dim)) || (rc = ix->consts.ensure(4))) { perm.release(); free_forest(ix); return rc; }
    }
    ix->n_planes = n_planes;
    ix->samples.mark(true);  // every plane of this forest was made from two stored rows, recorded in samples.pairs
    ix->leaf_ids = perm;  // perm is the concatenation of all leaves
    perm.p = nullptr; perm.cap = 0;
    ix->n_leaf_ids = total;
    rc = upload_nodes(ix);
    if (rc) free_forest(ix);
    return rc;
}

// LSHIndex::add on an index that already has trees (lsh.rs:445-462) for rows [n_prev, n_prev + n_new), as the
// sequential execution "one row after another, each into every tree".  A leaf's fate depends only on its own
// arrivals in id order, so the rows are processed in rounds: descend all pending (row, tree) pairs on the GPU,
// append to leaves with room, split the leaves that overflow (GPU classification through grow_segments) and
// send the arrivals that came after a split down the new subtree in the next round.
static int insert_rows_locked(zh_index *ix, uint64_t n_prev, uint64_t n_new) {
    const uint32_t T = ix->n_trees, M = ix->opt.max_node_size, d = ix->opt.dim;
    hipStream_t s = ix->stream;
    int rc;
    if (!n_new) return ZH_OK;
    if (ix->h_leaf_ids.size() != ix->n_leaf_ids) {  // host mirror of the leaf lists (bookkeeping only)
        ix->h_leaf_ids.resize(ix->n_leaf_ids);
        if (ix->n_leaf_ids) HIPCHK(hipMemcpy(ix->h_leaf_ids.data(), ix->leaf_ids.p, ix->n_leaf_ids * 4, hipMemcpyDeviceToHost));
    }
    std::vector<ZhDescend> pending;
    pending.reserve(n_new * T);
    for (uint64_t r = 0; r < n_new; r++)
        for (uint32_t t = 0; t < T; t++) pending.push_back({(uint32_t)(n_prev + r), ix->h_roots[t], 0, t, 1});
    DevBuf dItems, dTemp;
    struct G { DevBuf *a, *b; ~G() { a->release(); b->release(); } } g{&dItems, &dTemp};
    uint32_t n_planes = ix->n_planes;
    while (!pending.empty()) {
        if (pending.size() > 0x7FFFFFFFull) return fail(ZH_ELIMIT, "too many rows in one add call");
        if ((rc = dItems.ensure(pending.size() * sizeof(ZhDescend)))) return rc;
        HIPCHK(hipMemcpyAsync(dItems.p, pending.data(), pending.size() * sizeof(ZhDescend), hipMemcpyHostToDevice, s));
        HIPCHK(zh_launch_descend(forest_dev(ix), ix->X.as<float>(), d, dItems.as<ZhDescend>(), (uint32_t)pending.size(), s));
        HIPCHK(hipMemcpyAsync(pending.data(), dItems.p, pending.size() * sizeof(ZhDescend), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::sort(pending.begin(), pending.end(), [](const ZhDescend &a, const ZhDescend &b) {
            return a.node != b.node ? a.node < b.node : a.row < b.row;
        });
        std::vector<ZhDescend> next;
        std::vector<ActiveNode> splits;
        std::vector<uint32_t> temp;  // id lists of the nodes to split, one segment each
        const size_t old_leaf_size = ix->h_leaf_ids.size();
        for (size_t i = 0; i < pending.size();) {
            size_t j = i;
            while (j < pending.size() && pending[j].node == pending[i].node) j++;
            const ZhDescend &first = pending[i];
            const uint32_t node = first.node;
            const uint32_t off = (uint32_t)ix->h_left[node], len = (uint32_t)ix->h_right[node];
            std::vector<uint32_t> cur(ix->h_leaf_ids.begin() + off, ix->h_leaf_ids.begin() + off + len);
            size_t a = i;
            const bool can_split = first.depth < ZH_MAX_DEPTH;
            while (a < j && (cur.size() + 1 <= M || !can_split)) cur.push_back(pending[a++].row);  // lsh.rs:368-369
            if (a == j) {  // the leaf just grew: relocate its run to the end of leaf_ids
                ix->h_left[node] = (int32_t)(uint32_t)ix->h_leaf_ids.size();
                ix->h_right[node] = (int32_t)cur.size();
                ix->h_leaf_ids.insert(ix->h_leaf_ids.end(), cur.begin(), cur.end());
            } else {       // lsh.rs:370-377: this arrival overflows the leaf -> build_a_tree(leaf ids + id)
                cur.push_back(pending[a].row);
                splits.push_back({node, first.tree, (uint32_t)cur.size(), first.depth, (uint64_t)temp.size(), first.path,
                                  (uint64_t)pending[a].row + 1});
                temp.insert(temp.end(), cur.begin(), cur.end());
                for (size_t r = a + 1; r < j; r++) next.push_back(pending[r]);  // they arrive after the split
            }
            i = j;
        }
        if (ix->h_leaf_ids.size() + temp.size() > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "leaf storage exceeds 2^32-1 entries; rebuild the index");
        if (!splits.empty()) {
            if ((rc = dTemp.ensure(temp.size() * 4))) return rc;
            HIPCHK(hipMemcpyAsync(dTemp.p, temp.data(), temp.size() * 4, hipMemcpyHostToDevice, s));
            const uint64_t leaf_base = ix->h_leaf_ids.size();
            if ((rc = grow_segments(ix, dTemp.as<uint32_t>(), temp.size(), splits, leaf_base, n_planes, false))) return rc;
            HIPCHK(hipMemcpy(temp.data(), dTemp.p, temp.size() * 4, hipMemcpyDeviceToHost));
            ix->h_leaf_ids.insert(ix->h_leaf_ids.end(), temp.begin(), temp.end());
        }
        // mirror -> device (appended tail only), nodes -> device
        if (ix->h_leaf_ids.size() > old_leaf_size) {
            if ((rc = ix->leaf_ids.ensure(ix->h_leaf_ids.size() * 4, true, s))) return rc;
            HIPCHK(hipMemcpyAsync(ix->leaf_ids.as<uint32_t>() + old_leaf_size, ix->h_leaf_ids.data() + old_leaf_size,
                                  (ix->h_leaf_ids.size() - old_leaf_size) * 4, hipMemcpyHostToDevice, s));
        }
        ix->n_leaf_ids = ix->h_leaf_ids.size();
        ix->n_planes = n_planes;
        if ((rc = upload_nodes(ix))) return rc;
        pending.swap(next);
    }
    // compaction: relocated runs leave dead entries behind; rewrite the lists when they dominate
    const uint64_t live = (uint64_t)T * ix->n_rows;
    if (ix->h_leaf_ids.size() > 2 * live + 1024) {
        std::vector<uint32_t> compact;
        compact.reserve(live);
        for (size_t n = 0; n < ix->h_plane.size(); n++)
            if (ix->h_plane[n] < 0) {
                uint32_t off = (uint32_t)ix->h_left[n], len = (uint32_t)ix->h_right[n];
                ix->h_left[n] = (int32_t)(uint32_t)compact.size();
                compact.insert(compact.end(), ix->h_leaf_ids.begin() + off, ix->h_leaf_ids.begin() + off + len);
            }
        ix->h_leaf_ids.swap(compact);
        ix->n_leaf_ids = ix->h_leaf_ids.size();
        if (ix->n_leaf_ids) HIPCHK(hipMemcpyAsync(ix->leaf_ids.p, ix->h_leaf_ids.data(), ix->n_leaf_ids * 4, hipMemcpyHostToDevice, s));
        if ((rc = upload_nodes(ix))) return rc;
    }
    return ZH_OK;
}

extern "C" int zh_index_build(zh_index *ix) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    if (ix->opt.max_node_size == 0) return fail(ZH_EINVAL, "max_node_size must be >= 1");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    return build_forest_locked(ix);
}

extern "C" int zh_index_add(zh_index *ix, const float *rows, size_t n, uint64_t *out_ids) {
    if (!ix || (!rows && n)) return fail(ZH_EINVAL, "zh_index_add: null argument");
    if (ix->opt.max_node_size == 0) return fail(ZH_EINVAL, "max_node_size must be >= 1");
    std::unique_lock<std::shared_mutex> lk(ix->mu);  // one critical section: state is read, rows stored and trees updated under it
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (ix->broken) return fail(ZH_ESTATE, "an earlier add failed half way: call zh_index_build before adding or searching");
    const bool had_trees = ix->n_trees != 0;  // lsh.rs:441: no_trees() decides between build_index and insert
    const uint64_t n_prev = ix->n_rows;
    // capacity checks BEFORE anything is mutated: the rows, and (incremental path) the leaf entries of the new rows
    if (n_prev + n > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "more than 2^32-1 rows in one index (shard it)");
    if ((uint64_t)ix->opt.num_trees * (n_prev + n) > 0xFFFFFFFFull)
        return fail(ZH_ELIMIT, "num_trees * rows exceeds 2^32-1 leaf entries; shard the index");
    if (had_trees && n * (uint64_t)ix->n_trees > 0x7FFFFFFFull) return fail(ZH_ELIMIT, "too many rows in one add call");
    int rc = append_locked(ix, rows, n, out_ids);
    if (rc) return rc;  // nothing changed
    if (!had_trees) return build_forest_locked(ix);  // lsh.rs:441-443; on failure: rows stored, no trees (a consistent state)
    rc = insert_rows_locked(ix, n_prev, n);          // lsh.rs:445-462
    if (rc) {
        // the host mirrors of the trees may be ahead of the device copy: the rows stay stored (their ids were handed out),
        // the forest is declared stale until zh_index_build rebuilds it; searches say so instead of missing rows silently
        ix->broken = true;
    }
    return rc;
}

// LSHIndex::remove (lsh.rs:473-503) as it is meant: the reference only edits trees whose root is a leaf, so an id
// stays in every inner tree while its embedding is gone.  Here every tree drops the id: the row's
// leaf is found on the GPU by descending with the row's own vector, the leaf's run shrinks in place.
static int remove_rows_locked(zh_index *ix, const std::vector<uint32_t> &rows, std::vector<uint8_t> &found) {
    const uint32_t T = ix->n_trees, d = ix->opt.dim;
    hipStream_t s = ix->stream;
    int rc;
    found.assign(rows.size(), 0);
    if (rows.empty()) return ZH_OK;
    if (ix->h_dead.size() < ix->n_rows) ix->h_dead.resize(ix->n_rows, 0);
    if (T) {
        if (ix->h_leaf_ids.size() != ix->n_leaf_ids) {
            ix->h_leaf_ids.resize(ix->n_leaf_ids);
            if (ix->n_leaf_ids) HIPCHK(hipMemcpy(ix->h_leaf_ids.data(), ix->leaf_ids.p, ix->n_leaf_ids * 4, hipMemcpyDeviceToHost));
        }
        std::vector<ZhDescend> items;
        items.reserve(rows.size() * T);
        for (size_t r = 0; r < rows.size(); r++)
            for (uint32_t t = 0; t < T; t++) items.push_back({rows[r], ix->h_roots[t], (uint32_t)r, t, 1});  // depth field carries r
        DevBuf dItems;
        struct G { DevBuf *a; ~G() { a->release(); } } g{&dItems};
        if ((rc = dItems.ensure(items.size() * sizeof(ZhDescend)))) return rc;
        HIPCHK(hipMemcpyAsync(dItems.p, items.data(), items.size() * sizeof(ZhDescend), hipMemcpyHostToDevice, s));
        std::vector<uint32_t> slot(items.size());
        for (size_t i = 0; i < items.size(); i++) slot[i] = items[i].depth;
        HIPCHK(zh_launch_descend(forest_dev(ix), ix->X.as<float>(), d, dItems.as<ZhDescend>(), (uint32_t)items.size(), s));
        HIPCHK(hipMemcpyAsync(items.data(), dItems.p, items.size() * sizeof(ZhDescend), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        auto drop = [&](uint32_t node, uint32_t id) {  // remove id from a leaf's run (in place), true if it was there
            uint32_t off = (uint32_t)ix->h_left[node], len = (uint32_t)ix->h_right[node];
            uint32_t *run = ix->h_leaf_ids.data() + off;
            for (uint32_t i = 0; i < len; i++)
                if (run[i] == id) {
                    memmove(run + i, run + i + 1, (len - i - 1) * sizeof(uint32_t));
                    ix->h_right[node] = (int32_t)(len - 1);
                    return true;
                }
            return false;
        };
        std::vector<uint32_t> touched;
        for (size_t i = 0; i < items.size(); i++) {
            const uint32_t r = slot[i], id = items[i].row, t = items[i].tree;
            uint32_t node = items[i].node;
            bool hit = drop(node, id);
            if (!hit) {  // an injected forest may keep the id elsewhere: scan this tree's leaves
                std::vector<uint32_t> st{ix->h_roots[t]};
                while (!st.empty() && !hit) {
                    uint32_t m = st.back(); st.pop_back();
                    if (ix->h_plane[m] < 0) { if (drop(m, id)) { hit = true; node = m; } }
                    else { st.push_back((uint32_t)ix->h_left[m]); st.push_back((uint32_t)ix->h_right[m]); }
                }
            }
            if (hit) { found[r] = 1; touched.push_back(node); }
        }
        std::sort(touched.begin(), touched.end());
        touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
        for (uint32_t node : touched) {  // shrunken runs back to the device
            uint32_t off = (uint32_t)ix->h_left[node], len = (uint32_t)ix->h_right[node];
            if (len) HIPCHK(hipMemcpyAsync(ix->leaf_ids.as<uint32_t>() + off, ix->h_leaf_ids.data() + off, (size_t)len * 4, hipMemcpyHostToDevice, s));
        }
        if ((rc = upload_nodes(ix))) return rc;
    } else {
        for (size_t r = 0; r < rows.size(); r++) found[r] = 1;  // vectors without trees: just forget them
    }
    for (size_t r = 0; r < rows.size(); r++)
        if (found[r] && !ix->h_dead[rows[r]]) { ix->h_dead[rows[r]] = 1; ix->n_dead++; ix->dead_gen++; }
    return ZH_OK;
}

extern "C" int zh_index_remove(zh_index *ix, const uint64_t *ids, size_t n, uint8_t *out_found, size_t *out_n_removed) {
    if (!ix || (n && !ids)) return fail(ZH_EINVAL, "zh_index_remove: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    std::vector<uint32_t> rows;
    std::vector<size_t> where;
    std::vector<uint8_t> seen(ix->n_rows, 0);
    for (size_t i = 0; i < n; i++) {
        if (out_found) out_found[i] = 0;
        if (ids[i] < ix->opt.id_base) continue;
        uint64_t r = ids[i] - ix->opt.id_base;
        if (r >= ix->n_rows || seen[r] || (r < ix->h_dead.size() && ix->h_dead[r])) continue;
        seen[r] = 1;
        rows.push_back((uint32_t)r);
        where.push_back(i);
    }
    std::vector<uint8_t> found;
    if ((rc = remove_rows_locked(ix, rows, found))) return rc;
    size_t cnt = 0;
    for (size_t j = 0; j < rows.size(); j++)
        if (found[j]) { cnt++; if (out_found) out_found[where[j]] = 1; }
    if (out_n_removed) *out_n_removed = cnt;
    return ZH_OK;
}

// LSHIndex::deduplicate (lsh.rs:270-288): every live row whose f32 bit pattern equals an earlier live row's is
// removed.  Rows are hashed on the GPU (one pass over the stored vectors), equal hashes are confirmed byte for byte.
extern "C" int zh_index_deduplicate(zh_index *ix, uint64_t *out_ids, size_t cap, size_t *out_n_removed) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    const uint64_t N = ix->n_rows;
    const uint32_t d = ix->opt.dim;
    if (out_n_removed) *out_n_removed = 0;
    if (N < 2) return ZH_OK;
    DevBuf dh;
    struct G { DevBuf *a; ~G() { a->release(); } } g{&dh};
    if ((rc = dh.ensure(N * 8))) return rc;
    HIPCHK(zh_launch_row_hash(ix->X.as<float>(), N, d, dh.as<uint64_t>(), ix->stream));
    std::vector<uint64_t> hh(N);
    HIPCHK(hipMemcpyAsync(hh.data(), dh.p, N * 8, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    std::vector<std::pair<uint64_t, uint32_t>> hv;
    hv.reserve(N - ix->n_dead);
    for (uint64_t i = 0; i < N; i++)
        if (!(i < ix->h_dead.size() && ix->h_dead[i])) hv.push_back({hh[i], (uint32_t)i});
    std::sort(hv.begin(), hv.end());
    // runs of equal hash: every member is compared (on the GPU, bit for bit) with the run's current representative;
    // members that differ from it -- a hash collision -- form the next round against the next representative
    std::vector<uint32_t> dups;
    std::vector<std::vector<uint32_t>> runs;
    for (size_t i = 0; i < hv.size();) {
        size_t j = i + 1;
        while (j < hv.size() && hv[j].first == hv[i].first) j++;
        if (j - i > 1) {
            std::vector<uint32_t> r;
            for (size_t p = i; p < j; p++) r.push_back(hv[p].second);  // ascending ids (sorted by (hash, id))
            runs.push_back(std::move(r));
        }
        i = j;
    }
    DevBuf dPairs, dEq;
    struct G2 { DevBuf *a, *b; ~G2() { a->release(); b->release(); } } g2{&dPairs, &dEq};
    while (!runs.empty()) {
        std::vector<uint32_t> pairs;
        for (auto &r : runs)
            for (size_t p = 1; p < r.size(); p++) { pairs.push_back(r[0]); pairs.push_back(r[p]); }
        const uint32_t np = (uint32_t)(pairs.size() / 2);
        std::vector<uint8_t> eq(np);
        if ((rc = dPairs.ensure(pairs.size() * 4)) || (rc = dEq.ensure(np))) return rc;
        HIPCHK(hipMemcpyAsync(dPairs.p, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, ix->stream));
        HIPCHK(zh_launch_rows_equal(ix->X.as<float>(), d, dPairs.as<uint32_t>(), np, dEq.as<uint8_t>(), ix->stream));
        HIPCHK(hipMemcpyAsync(eq.data(), dEq.p, np, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        std::vector<std::vector<uint32_t>> next;
        size_t q = 0;
        for (auto &r : runs) {
            std::vector<uint32_t> rest;
            for (size_t p = 1; p < r.size(); p++, q++) {
                if (eq[q]) dups.push_back(r[p]); else rest.push_back(r[p]);
            }
            if (rest.size() > 1) next.push_back(std::move(rest));
        }
        runs.swap(next);
    }
    std::sort(dups.begin(), dups.end());
    std::vector<uint8_t> found;
    if ((rc = remove_rows_locked(ix, dups, found))) return rc;
    size_t cnt = 0;
    for (size_t i = 0; i < dups.size(); i++) {
        if (out_ids && cnt < cap) out_ids[cnt] = ix->opt.id_base + dups[i];
        cnt++;
    }
    if (out_n_removed) *out_n_removed = cnt;
    return ZH_OK;
}

// zh_index_compact: the live rows move down over the removed ones, in place and in their order; everything that names a row is renumbered.
// Steps: (1) rank -- new_row[r] for every old row, from the live bitmap (zh_compact.hip); (2) the move, in stream-ordered chunks of old rows
// [a, b): the chunk's live rows go to [new(a), new(b)).  new(r) <= r, so a chunk whose destination ends at or before its source begins
// (new(b) <= a) is one launch that reads and writes disjoint ranges; any other chunk is gathered into the bounce buffer first and copied to its
// destination by a second launch.  Either way a chunk writes below new(b) <= b only: never into the source of a LATER chunk, and the stream
// runs the chunks in order.  Rows before the first removed row stay where they are.  (3) leaf_ids and the planes' sample rows through new_row.
// (4) the host's view: counts, generations, and every derived copy of the rows let go (re-made at the new size by the batch that next wants it).
extern "C" int zh_index_compact(zh_index *ix, uint64_t *out_new_ids, size_t cap, zh_compact_info *info) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (ix->broken) return fail(ZH_ESTATE, "an earlier add failed half way: call zh_index_build before compacting");
    const uint64_t N = ix->n_rows, NL = N - ix->n_dead, id_base = ix->opt.id_base;
    const uint32_t d = ix->opt.dim;
    const size_t row_bytes = (size_t)d * sizeof(float);
    if (out_new_ids && cap < N)
        return fail(ZH_EINVAL, "zh_index_compact: out_new_ids holds %zu entries, %llu rows are stored", cap, (unsigned long long)N);
    zh_compact_info ci{};
    ci.rows_before = N; ci.rows_after = NL; ci.capacity_rows = ix->X.cap / row_bytes;
    if (ix->n_dead == 0) {  // nothing to reclaim: no generation moves, no copy is released
        if (out_new_ids) for (uint64_t r = 0; r < N; r++) out_new_ids[r] = id_base + r;
        if (info) *info = ci;
        return ZH_OK;
    }
    if (ix->scan_unsafe)
        return fail(ZH_EUNSUPPORTED, "zh_index_compact: the injected forest lists a row twice in one tree and may still list a removed row; rebuild it first");
    HIPCHK(hipDeviceSynchronize());  // nothing of an earlier batch is left reading the rows or the copies
    hipStream_t s = ix->stream;
    if (ix->h_dead.size() < N) ix->h_dead.resize(N, 0);

    // the live bitmap; the chunks of old rows from the first removed row on, with their live counts
    std::vector<uint32_t> bits((N + 31) / 32 + 1, 0u);
    uint64_t first_dead = N;
    for (uint64_t r = 0; r < N; r++) {
        if (!ix->h_dead[r]) bits[r >> 5] |= 1u << (r & 31);
        else if (first_dead == N) first_dead = r;
    }
    const uint64_t chunk_max = std::max<uint64_t>(1, ZH_COMPACT_BOUNCE_BYTES / row_bytes);  // what the bounce buffer holds
    uint64_t chunk_rows = chunk_max;
    if (const char *e = getenv("ZH_COMPACT_CHUNK_ROWS")) {
        const long long v = atoll(e);
        if (v > 0) chunk_rows = std::min<uint64_t>((uint64_t)v, chunk_max);
    }
    struct Chunk { uint64_t a, n, to, live; bool direct; };
    std::vector<Chunk> chunks;
    uint64_t bounce_rows = 0;
    {
        uint64_t to = first_dead;  // = new(first_dead): every row before it is live
        for (uint64_t a = first_dead; a < N; a += chunk_rows) {
            const uint64_t n = std::min(chunk_rows, N - a);
            uint64_t live = 0;
            for (uint64_t r = a; r < a + n; r++) live += !ix->h_dead[r];
            if (live) {
                const bool direct = to + live <= a;
                chunks.push_back({a, n, to, live, direct});
                if (!direct) bounce_rows = std::max(bounce_rows, live);
                ci.rows_moved += live;
                ci.bytes_moved += (direct ? 2 : 4) * live * (uint64_t)row_bytes;
            }
            to += live;
        }
    }

    const uint64_t nb = (N + ZH_COMPACT_RANK_ROWS - 1) / ZH_COMPACT_RANK_ROWS;
    DevBuf dBits, dNew, dCount, dExcl, dTmp, dFlag, dBounce;
    struct G { std::vector<DevBuf *> v; ~G() { for (auto *b : v) b->release(); } } g;
    g.v = {&dBits, &dNew, &dCount, &dExcl, &dTmp, &dFlag, &dBounce};
    if ((rc = dBits.ensure(bits.size() * 4)) || (rc = dNew.ensure(N * 4)) || (rc = dCount.ensure(nb * 4)) || (rc = dExcl.ensure((nb + 1) * 4)) ||
        (rc = dTmp.ensure((nb / 1024 + 4) * 4)) || (rc = dFlag.ensure(4)) || (bounce_rows && (rc = dBounce.ensure(bounce_rows * row_bytes))))
        return rc;
    for (DevBuf *b : g.v) ci.scratch_bytes += b->cap;
    std::vector<uint32_t> h_new;
    const bool want_host_map = out_new_ids != nullptr;  // (4 bytes per stored row back over PCIe: only for a caller who wants the map)
    if (want_host_map) h_new.resize(N);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIPCHK(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { hipEventDestroy(ev0); return fail(ZH_EHIP, "hipEventCreate failed"); }
    struct GE { hipEvent_t a, b; ~GE() { hipEventDestroy(a); hipEventDestroy(b); } } ge{ev0, ev1};

    // (1) rank: nothing of the index has changed yet
    HIPCHK(hipMemcpyAsync(dBits.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dFlag.p, 0, 4, s));
    HIPCHK(hipEventRecord(ev0, s));
    HIPCHK(zh_launch_compact_rank(dBits.as<uint32_t>(), N, dCount.as<uint32_t>(), dExcl.as<uint32_t>(), dTmp.as<uint32_t>(), dNew.as<uint32_t>(), s));
    HIPCHK(hipStreamSynchronize(s));

    // (2) + (3): from here on a failure leaves rows half moved
    float *X = ix->X.as<float>();
    const uint32_t *dMap = dNew.as<uint32_t>();
    hipError_t e = hipSuccess;
    for (size_t c = 0; c < chunks.size() && e == hipSuccess; c++) {
        const Chunk &ch = chunks[c];
        if (ch.direct) {
            e = zh_launch_move_rows(X, X, d, dMap, ch.a, ch.n, 0, s);
        } else {
            e = zh_launch_move_rows(X, dBounce.as<float>(), d, dMap, ch.a, ch.n, ch.to, s);
            if (e == hipSuccess) e = zh_launch_move_rows(dBounce.as<float>(), X + ch.to * d, d, nullptr, 0, ch.live, 0, s);
        }
    }
    if (e == hipSuccess) e = zh_launch_renumber_ids(ix->leaf_ids.as<uint32_t>(), ix->n_leaf_ids, dMap, N, s);
    const bool had_samples = ix->samples.valid && ix->n_planes && ix->samples.pairs.cap >= (size_t)ix->n_planes * sizeof(uint2);
    if (e == hipSuccess && had_samples) e = zh_launch_renumber_samples(ix->samples.pairs.as<uint2>(), ix->n_planes, dMap, N, dFlag.as<uint32_t>(), s);
    if (e == hipSuccess) e = hipEventRecord(ev1, s);
    uint32_t lost_sample = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&lost_sample, dFlag.p, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && want_host_map) e = hipMemcpyAsync(h_new.data(), dNew.p, N * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        ix->broken = true; ix->rows_torn = true;
        return fail(ZH_EHIP, "zh_index_compact failed after rows had begun to move (%s): the stored rows are inconsistent; zh_index_clear the index and store them again",
                    hipGetErrorString(e));
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) ci.ms = ms;

    // (4) the host's view
    if (out_new_ids)
        for (uint64_t r = 0; r < N; r++) out_new_ids[r] = h_new[r] == 0xFFFFFFFFu ? ~0ull : id_base + h_new[r];
    if (want_host_map && ix->n_leaf_ids && ix->h_leaf_ids.size() == ix->n_leaf_ids) {
        for (uint32_t &v : ix->h_leaf_ids)
            if (v < N) v = h_new[v] == 0xFFFFFFFFu ? 0u : h_new[v];
    } else {
        ix->h_leaf_ids.clear();  // (the next incremental add or remove reads the mirror back from the device)
    }
    ix->n_rows = NL;
    ix->h_dead.clear();
    ix->n_dead = 0;
    ix->rows_gen++; ix->dead_gen++;
    ci.copy_bytes_released = views_rows_moved(ix, lost_sample != 0);
    if (info) *info = ci;
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// snapshots: zh_index_save / zh_index_load (the file: zh_snapfile.cpp; the row pipeline and the checksum kernel: zh_snapshot.hip)
// ------------------------------------------------------------------------------------------------
static int no_device_for_snapshot(const char *who) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(ZH_EHIP, "%s: no usable HIP device (%s); this library has no CPU fallback", who, e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return ZH_OK;
}
static double wall_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" int zh_index_save(zh_index *ix, const char *path, zh_snapshot_info *info) {
    const auto t_begin = std::chrono::steady_clock::now();
    if (info) memset(info, 0, sizeof *info);
    int rc = no_device_for_snapshot("zh_index_save");
    if (rc) return rc;
    if (!ix || !path || !*path) return fail(ZH_EINVAL, "zh_index_save: null argument");
    if (strlen(path) > 4000) return fail(ZH_EINVAL, "zh_index_save: path longer than 4000 bytes");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if ((rc = set_device(ix))) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (ix->broken) return fail(ZH_ESTATE, "an earlier add failed half way: call zh_index_build before saving");
    HIPCHK(hipStreamSynchronize(ix->stream));
    const uint64_t N = ix->n_rows;
    const uint32_t d = ix->opt.dim, np = ix->n_planes;
    ZhSnapHeader h{};
    zh_snapshot_info &f = h.info;
    f.version = ZH_SNAPSHOT_VERSION; f.dim = d; f.max_node_size = ix->opt.max_node_size; f.num_trees_option = ix->opt.num_trees;
    f.seed = ix->opt.seed; f.id_base = ix->opt.id_base; f.stored_rows = N; f.live_rows = N - ix->n_dead;
    f.n_trees = ix->n_trees; f.n_nodes = ix->n_nodes; f.n_planes = np; f.n_leaf_ids = ix->n_leaf_ids;
    f.flags = (ix->samples.valid ? 1u : 0u) | (ix->scan_unsafe ? 2u : 0u);
    h.max_leaf_len = ix->max_leaf_len;
    h.n_levels = (uint32_t)ix->planes_below_level.size();
    if (h.n_levels > ZH_SNAP_MAX_LEVELS) return fail(ZH_ELIMIT, "zh_index_save: %u forest levels", h.n_levels);
    zh_snap_plan(&h);

    // the small sections, through the host
    std::vector<uint8_t> removed((N + 7) / 8, 0);
    for (uint64_t r = 0; r < N && r < ix->h_dead.size(); r++)
        if (ix->h_dead[r]) removed[r >> 3] |= (uint8_t)(1u << (r & 7));
    std::vector<float> hp((size_t)np * d), hc(np);
    std::vector<uint32_t> hl(ix->n_leaf_ids), hs(f.flags & 1u ? (size_t)np * 2 : 0);
    if (np) {
        HIPCHK(hipMemcpy(hp.data(), ix->planes.p, hp.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc.data(), ix->consts.p, hc.size() * 4, hipMemcpyDeviceToHost));
    }
    if (!hl.empty()) HIPCHK(hipMemcpy(hl.data(), ix->leaf_ids.p, hl.size() * 4, hipMemcpyDeviceToHost));
    if (!hs.empty()) {
        if (ix->samples.pairs.cap < hs.size() * 4) return fail(ZH_ESTATE, "zh_index_save: the planes' sample rows are incomplete");
        HIPCHK(hipMemcpy(hs.data(), ix->samples.pairs.p, hs.size() * 4, hipMemcpyDeviceToHost));
    }
    const void *small[ZH_SNAP_MAX_SECTIONS] = {};
    small[ZH_SEC_REMOVED] = removed.data(); small[ZH_SEC_NODE_PLANE] = ix->h_plane.data(); small[ZH_SEC_NODE_LEFT] = ix->h_left.data();
    small[ZH_SEC_NODE_RIGHT] = ix->h_right.data(); small[ZH_SEC_ROOTS] = ix->h_roots.data(); small[ZH_SEC_PLANES] = hp.data();
    small[ZH_SEC_CONSTS] = hc.data(); small[ZH_SEC_LEAF_IDS] = hl.data(); small[ZH_SEC_LEVELS] = ix->planes_below_level.data();
    small[ZH_SEC_SAMPLES] = hs.data();
    if (ix->h_plane.size() != ix->n_nodes || ix->h_roots.size() != ix->n_trees) return fail(ZH_ESTATE, "zh_index_save: the forest's host mirror is stale");

    std::vector<char> tmp(strlen(path) + 16);
    int fd;
    if ((rc = zh_snap_create(path, f.file_bytes, tmp.data(), &fd))) return rc;
    double ms_device = 0;
    for (uint32_t i = 0; i < f.n_sections && !rc; i++) {
        ZhSnapSection &s = h.sec[i];
        if (s.kind == ZH_SEC_ROWS) {
            rc = zh_snap_rows_out(fd, tmp.data(), s.offset, ix->X.p, s.length, &s.checksum, &ms_device);
        } else {
            s.checksum = zh_snap_sum(small[s.kind], s.length, 0);
            if (s.length) rc = zh_snap_pwrite(fd, small[s.kind], s.length, s.offset, tmp.data());
        }
    }
    if (!rc) {
        uint8_t block[ZH_SNAP_BLOCK];
        zh_snap_encode(&h, block);
        rc = zh_snap_pwrite(fd, block, ZH_SNAP_BLOCK, 0, tmp.data());
    }
    if (rc) { zh_snap_abort(fd, tmp.data()); return rc; }
    if ((rc = zh_snap_commit(fd, tmp.data(), path))) return rc;
    if (info) {
        *info = f;
        info->verified = 1;  // every checksum in the table was computed from the index's own memory by this call
        info->ms_device = ms_device;
        info->ms = wall_ms_since(t_begin);
    }
    return ZH_OK;
}

// everything of a snapshot but the rows, read into host memory and tested; then installed into a fresh index
static int load_forest(zh_index *ix, int fd, const ZhSnapHeader &h) {
    const zh_snapshot_info &f = h.info;
    const uint64_t N = f.stored_rows;
    const uint32_t nn = f.n_nodes, np = f.n_planes, nt = f.n_trees, d = f.dim;
    int rc;
    auto corrupt = [&](const char *what) { return fail(ZH_ECORRUPT, "zh_index_load: %s", what); };
    // removed rows
    std::vector<uint8_t> removed((N + 7) / 8);
    if ((rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_REMOVED), removed.data()))) return rc;
    uint64_t n_dead = 0;
    for (uint8_t b : removed) n_dead += (uint64_t)__builtin_popcount(b);
    if ((N & 7) && (removed.back() >> (N & 7))) return corrupt("the removed-row bitmap names rows past the stored ones");
    if (n_dead != N - f.live_rows) return corrupt("the removed-row bitmap does not match the live count");
    // forest
    std::vector<int32_t> plane(nn), left(nn), right(nn);
    std::vector<uint32_t> roots(nt), leaf_ids(f.n_leaf_ids), levels(h.n_levels), samples(f.flags & 1u ? (size_t)np * 2 : 0);
    std::vector<float> planes((size_t)np * d), consts(np);
    if ((rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_NODE_PLANE), plane.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_NODE_LEFT), left.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_NODE_RIGHT), right.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_ROOTS), roots.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_PLANES), planes.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_CONSTS), consts.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_LEAF_IDS), leaf_ids.data())) ||
        (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_LEVELS), levels.data())))
        return rc;
    if ((f.flags & 1u) && (rc = zh_snap_read_section(fd, zh_snap_find(&h, ZH_SEC_SAMPLES), samples.data()))) return rc;
    zh_forest_view fv{};
    fv.n_nodes = nn; fv.n_planes = np; fv.n_trees = nt; fv.n_leaf_ids = f.n_leaf_ids;
    fv.plane = plane.data(); fv.left = left.data(); fv.right = right.data(); fv.roots = roots.data();
    fv.planes = planes.data(); fv.consts = consts.data(); fv.leaf_ids = leaf_ids.data();
    ForestCheck fc;
    if (check_forest(&fv, N, fc)) {
        const std::string why = g_err;
        return fail(ZH_ECORRUPT, "zh_index_load: the forest fails zh_index_set_forest's tests (%s)", why.c_str());
    }
    uint32_t max_leaf_len = 0;
    for (uint32_t n = 0; n < nn; n++) {
        // (set_forest's tests cover the nodes a root reaches; pack_nodes and the leaf-length pass read EVERY record)
        if (plane[n] >= 0 && (uint32_t)plane[n] >= std::max(np, 1u)) return corrupt("a node names a plane past the last one");
        if (plane[n] < -1) return corrupt("a node record is neither inner nor leaf");
        if (plane[n] < 0) max_leaf_len = std::max(max_leaf_len, (uint32_t)right[n]);
    }
    if (max_leaf_len != h.max_leaf_len) return corrupt("max_leaf_len does not match the leaves");
    for (uint32_t l = 0; l < h.n_levels; l++)
        if (levels[l] > np || (l && levels[l] < levels[l - 1]) || (!l && levels[0] != 0)) return corrupt("the forest's level table is not 0 <= ... <= n_planes, ascending");
    for (uint32_t v : samples)
        if (v != 0xFFFFFFFFu && v >= N) return corrupt("a plane's sample row is past the stored rows");
    if (nt == 0 && (nn || np || f.n_leaf_ids || h.n_levels || (f.flags & 3u))) return corrupt("forest arrays without trees");

    // install: what build / insert / set_forest leave behind, with the planes in the file's numbering
    if (n_dead) {
        ix->h_dead.assign(N, 0);
        for (uint64_t r = 0; r < N; r++) ix->h_dead[r] = (removed[r >> 3] >> (r & 7)) & 1u;
    }
    ix->n_dead = n_dead;
    if (nt == 0) return ZH_OK;  // rows only: appended and never built, or empty
    ix->h_plane.swap(plane); ix->h_left.swap(left); ix->h_right.swap(right); ix->h_roots.swap(roots);
    if ((rc = ix->planes.ensure((size_t)std::max(np, 1u) * d * 4)) || (rc = ix->consts.ensure((size_t)std::max(np, 1u) * 4)) ||
        (rc = ix->leaf_ids.ensure(std::max<uint64_t>(f.n_leaf_ids, 1) * 4)))
        return rc;
    if (np) {
        HIPCHK(hipMemcpyAsync(ix->planes.p, planes.data(), planes.size() * 4, hipMemcpyHostToDevice, ix->stream));
        HIPCHK(hipMemcpyAsync(ix->consts.p, consts.data(), consts.size() * 4, hipMemcpyHostToDevice, ix->stream));
    }
    if (f.n_leaf_ids) HIPCHK(hipMemcpyAsync(ix->leaf_ids.p, leaf_ids.data(), leaf_ids.size() * 4, hipMemcpyHostToDevice, ix->stream));
    if (f.flags & 1u) {
        if ((rc = ix->samples.pairs.ensure((size_t)std::max(np, 1u) * sizeof(uint2)))) return rc;
        if (np) HIPCHK(hipMemcpyAsync(ix->samples.pairs.p, samples.data(), samples.size() * 4, hipMemcpyHostToDevice, ix->stream));
    }
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->n_planes = np;
    ix->n_leaf_ids = f.n_leaf_ids;
    ix->planes_below_level.swap(levels);
    ix->samples.mark((f.flags & 1u) != 0);
    rc = upload_nodes(ix);
    ix->scan_unsafe = (f.flags & 2u) != 0 || fc.dup_in_tree;
    return rc;
}

extern "C" int zh_index_load(const char *path, int32_t device, uint64_t reserve_rows, zh_index **out, zh_snapshot_info *info) {
    const auto t_begin = std::chrono::steady_clock::now();
    if (out) *out = nullptr;
    if (info) memset(info, 0, sizeof *info);
    int rc = no_device_for_snapshot("zh_index_load");
    if (rc) return rc;
    if (!path || !out) return fail(ZH_EINVAL, "zh_index_load: null argument");
    ZhSnapHeader h;
    int fd;
    if ((rc = zh_snap_open(path, &fd, &h))) return rc;  // every size tested against the file's length and the limits: nothing allocated yet
    struct FdGuard { int fd; ~FdGuard() { zh_snap_close(fd); } } fg{fd};
    const zh_snapshot_info &f = h.info;
    zh_options opt;
    zh_options_default(&opt);
    opt.dim = f.dim; opt.max_node_size = f.max_node_size; opt.num_trees = f.num_trees_option; opt.seed = f.seed; opt.id_base = f.id_base;
    opt.device = device;
    opt.reserve_rows = std::max<uint64_t>(reserve_rows, f.stored_rows);
    zh_index *ix = nullptr;
    if ((rc = zh_index_create(&opt, &ix))) return rc;
    opt.reserve_rows = reserve_rows;
    ix->opt.reserve_rows = reserve_rows;
    double ms_device = 0;
    uint64_t sum = 0;
    const ZhSnapSection *rows = zh_snap_find(&h, ZH_SEC_ROWS);
    rc = zh_snap_rows_in(fd, rows->offset, ix->X.p, rows->length, &sum, &ms_device);
    if (!rc && sum != rows->checksum)
        rc = fail(ZH_ECORRUPT, "zh_index_load: checksum mismatch in the rows as they arrived in device memory (section %u)", rows->kind);
    if (!rc) {
        ix->n_rows = f.stored_rows;
        rc = load_forest(ix, fd, h);
    }
    if (rc) {
        const std::string why = g_err;  // (destroy may overwrite the message)
        zh_index_destroy(ix);
        g_err = why;
        return rc;
    }
    *out = ix;
    if (info) {
        *info = f;
        info->verified = 1;
        info->ms_device = ms_device;
        info->ms = wall_ms_since(t_begin);
    }
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
extern "C" int zh_set_profiling(zh_index *ix, int level) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    ix->profiling = level;
    return ZH_OK;
}
extern "C" int zh_set_dense_levels(zh_index *ix, int levels) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    ix->dense_levels = levels;
    return ZH_OK;
}
extern "C" int zh_set_hash_mode(zh_index *ix, int mode) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    if (mode < 0 || mode > 2) return fail(ZH_EINVAL, "hash mode %d (0 = choose per batch, 1 = one dot product per plane, 2 = row scores)", mode);
    ix->hash_mode = mode;
    return ZH_OK;
}
extern "C" int zh_set_sweep_mode(zh_index *ix, int mode) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    if (mode < 0 || mode > 6)
        return fail(ZH_EINVAL, "sweep mode %d (0 = choose per batch, 1 = leaf by leaf, 2 = table scan with f32 queries, 3 = as 0: prefilter where row scores exist, "
                               "4 = table scan with half-width queries wherever it applies, 5 = as 4 without the fp16 copy of the rows: the VALU kernel, "
                               "6 = leaf by leaf at half width where that kernel exists (dim 128))", mode);
    ix->sweep_mode = mode;
    return ZH_OK;
}
extern "C" int zh_stats(zh_index *ix, zh_stats_t *out) {
    if (!ix || !out) return fail(ZH_EINVAL, "null argument");
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        *out = ix->stats;
    }
    std::lock_guard<std::mutex> lk(ix->blk_mu);  // (the copies are made and dropped under it)
    out->row_copy_bytes = row_copy_bytes(ix);
    out->scan_order_keys = ix->order.rows ? ix->order.keys : 0;
    out->scan_order_share_permille = (uint64_t)(ix->order.worth * 1000.0 + 0.5);
    return ZH_OK;
}
extern "C" int zh_stats_reset(zh_index *ix) {
    if (!ix) return fail(ZH_EINVAL, "null index");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    memset(&ix->stats, 0, sizeof ix->stats);
    return ZH_OK;
}

// The host mirror of the forest in pre-order, tree after tree: visit(node, its tree) (iterative: trees may be 60 levels deep).
template <typename Visit>
static void forest_preorder(const zh_index *ix, Visit visit) {
    std::vector<uint32_t> st;
    for (uint32_t t = 0; t < (uint32_t)ix->h_roots.size(); t++) {
        st.assign(1, ix->h_roots[t]);
        while (!st.empty()) {
            const uint32_t n = st.back(); st.pop_back();
            visit(n, t);
            if (ix->h_plane[n] >= 0) { st.push_back((uint32_t)ix->h_right[n]); st.push_back((uint32_t)ix->h_left[n]); }
        }
    }
}

// ... walked once -> node_tree[node] = the tree that holds it (0xFFFFFFFF: none) and, where asked for, every tree's non-empty leaves.
static std::vector<uint32_t> forest_walk(const zh_index *ix, std::vector<std::vector<uint2>> *leaves) {
    std::vector<uint32_t> node_tree(std::max<size_t>(ix->h_plane.size(), 1), 0xFFFFFFFFu);
    if (leaves) leaves->resize(ix->h_roots.size());
    forest_preorder(ix, [&](uint32_t nd, uint32_t t) {
        node_tree[nd] = t;
        if (leaves && ix->h_plane[nd] < 0 && ix->h_right[nd] > 0) (*leaves)[t].push_back(make_uint2((uint32_t)ix->h_left[nd], (uint32_t)ix->h_right[nd]));
    });
    return node_tree;
}

// Blocked view of the forest (zh_internal.h, ZhBlocksDev): every maximal subtree of at most ZH_BLOCK_NODES nodes becomes
// one block with its nodes in pre-order; the nodes above keep pointer records whose child refs say "upper node" or
// "block".  Host pass over the node mirrors (iterative: trees may be 60 levels deep), then four uploads.
// Round 5: blocks of INNER nodes only.  A block of the round-2 view spends half of its 64 records on leaves; here a block is a maximal subtree of at
// most ZH_BLOCK_INNER inner nodes, one 32-byte record per inner node in pre-order -- {plane, code of the left child | code of the right child << 8 |
// inner nodes of the block << 16 (root record), left leaf: offset into leaf_ids, length} {left leaf: node id, right leaf: offset, length, node id} --
// and its leaves live in their parent's record: a child code is the child's record (0 .. 62) or 0x80 | side << 6 | the parent's record for a leaf.
// Twice the tree nodes per block: half the blocks, half the upper nodes, and the walk's dependent round trips with them (1M x 384 at the
// reference's default options: 346k blocks / 346k upper nodes -> see tests/probes/refdefault_shape.py).  A leaf hanging directly off an upper node
// (or a tree that is one leaf) is a block of zero inner nodes: record {-1, 0, offset, length} {node id, 0, 0, 0}.
//
// the size of every subtree, by the measure its kind of block is limited in: all of its nodes, or its inner nodes only (the pre-order, then a
// reverse pass: children before parents)
static std::vector<uint32_t> subtree_sizes(const zh_index *ix, bool inner_only) {
    const size_t nn = ix->h_plane.size();
    std::vector<uint32_t> size(nn, 0), order;
    order.reserve(nn);
    forest_preorder(ix, [&](uint32_t n, uint32_t) { order.push_back(n); });
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t n = order[i];
        const bool inner = ix->h_plane[n] >= 0;
        size[n] = (inner_only ? (inner ? 1u : 0u) : 1u) + (inner ? size[(uint32_t)ix->h_left[n]] + size[(uint32_t)ix->h_right[n]] : 0u);
    }
    return size;
}

// Every maximal subtree of at most `limit` (by `size`) becomes a block -- emit_block(root) writes its records and returns its ref -- and the
// nodes above them get pointer records: upper nodes get dense ids in the order they are met; a child's ref is final once the child has been
// classified.
template <typename Emit>
static void place_blocks(const zh_index *ix, const std::vector<uint32_t> &size, uint32_t limit, Emit emit_block, std::vector<int4> &upper,
                         std::vector<int2> &roots) {
    std::vector<std::pair<uint32_t, uint32_t>> todo;  // (node, its upper id)
    for (uint32_t t = 0; t < (uint32_t)ix->h_roots.size(); t++) {
        const uint32_t rt = ix->h_roots[t];
        if (size[rt] <= limit) { roots[t] = make_int2(emit_block(rt), 0); continue; }
        roots[t] = make_int2((int32_t)(upper.size() / 2), ix->h_plane[rt]);
        upper.push_back(make_int4(0, 0, 0, 0)); upper.push_back(make_int4(0, 0, 0, 0));
        todo.assign(1, {rt, (uint32_t)(upper.size() / 2 - 1)});
        while (!todo.empty()) {
            const auto [n, uid] = todo.back(); todo.pop_back();
            const uint32_t ch[2] = {(uint32_t)ix->h_left[n], (uint32_t)ix->h_right[n]};
            int32_t ref[2], cpl[2];
            for (int e = 0; e < 2; e++) {
                if (size[ch[e]] <= limit) { ref[e] = emit_block(ch[e]); cpl[e] = 0; }
                else {
                    ref[e] = (int32_t)(upper.size() / 2); cpl[e] = ix->h_plane[ch[e]];
                    upper.push_back(make_int4(0, 0, 0, 0)); upper.push_back(make_int4(0, 0, 0, 0));
                    todo.push_back({ch[e], (uint32_t)ref[e]});
                }
            }
            upper[2 * (size_t)uid] = make_int4(ix->h_plane[n], ref[0], ref[1], 0);
            upper[2 * (size_t)uid + 1] = make_int4(cpl[0], cpl[1], 0, 0);
        }
    }
}

static int build_blocks(zh_index *ix) {
    // ZH_WALK_BLOCKS=inner (read when a forest's view is built): the round-5 blocks of inner nodes only.  Measured and NOT the default: half the
    // blocks and upper nodes, 27 % fewer block entries and 31 % fewer upper steps per pair -- and the same 8.5 ms per batch (DESIGN.md s9,
    // profiles/r05_walk_prof.txt): the walk's time is its instruction stream and the exact sign chains, not its round trips.
    const char *bv = getenv("ZH_WALK_BLOCKS");
    const bool inner_only = bv && bv[0] == 'i';
    const size_t nn = ix->h_plane.size();
    const uint32_t T = (uint32_t)ix->h_roots.size();
    const std::vector<uint32_t> size = subtree_sizes(ix, inner_only);
    std::vector<int4> recs, recsB, upper;  // inner only: recs / recsB = the first / second int4 of every inner node's record (two arrays: a wave's two loads
                                           // of a block are 1 KiB contiguous each -- interleaved 32-byte records made a block load 3404 cycles against 1795)
    std::vector<int2> roots(std::max<uint32_t>(T, 1), make_int2(0, 0));
    recs.reserve((inner_only ? nn / 2 : nn) + ZH_BLOCK_NODES);
    if (inner_only) recsB.reserve(nn / 2 + ZH_BLOCK_NODES);
    std::vector<uint32_t> nodes, st;
    uint32_t n_blocks = 0;
    auto emit_inner = [&](uint32_t root) -> int32_t {  // the subtree's INNER nodes in pre-order; a ref is -(first 32-byte record + 1)
        const std::vector<uint32_t> &isize = size;
        const size_t base = recs.size();
        n_blocks++;
        if (ix->h_plane[root] < 0) {  // a leaf by itself
            recs.push_back(make_int4(-1, 0, ix->h_left[root], ix->h_right[root]));
            recsB.push_back(make_int4((int)root, 0, 0, 0));
            return -(int32_t)base - 1;
        }
        nodes.clear();
        st.assign(1, root);
        while (!st.empty()) {
            const uint32_t n = st.back(); st.pop_back();
            nodes.push_back(n);
            const uint32_t l = (uint32_t)ix->h_left[n], r = (uint32_t)ix->h_right[n];
            if (ix->h_plane[r] >= 0) st.push_back(r);
            if (ix->h_plane[l] >= 0) st.push_back(l);
        }
        // inner pre-order: the left child (when inner) is i + 1, the right child i + 1 + (inner nodes of the left subtree)
        for (uint32_t i = 0; i < nodes.size(); i++) {
            const uint32_t n = nodes[i], l = (uint32_t)ix->h_left[n], r = (uint32_t)ix->h_right[n];
            const bool li = ix->h_plane[l] >= 0, ri = ix->h_plane[r] >= 0;
            const uint32_t cl = li ? i + 1 : (0x80u | i), cr = ri ? i + 1 + isize[l] : (0x80u | 0x40u | i);
            const uint32_t word = cl | (cr << 8) | (i == 0 ? (uint32_t)nodes.size() << 16 : 0u);
            recs.push_back(make_int4(ix->h_plane[n], (int)word, li ? 0 : ix->h_left[l], li ? 0 : ix->h_right[l]));
            recsB.push_back(make_int4(li ? 0 : (int)l, ri ? 0 : ix->h_left[r], ri ? 0 : ix->h_right[r], ri ? 0 : (int)r));
        }
        return -(int32_t)base - 1;
    };
    auto emit_whole = [&](uint32_t root) -> int32_t {  // nodes of the subtree in pre-order, children as local indices
        const size_t base = recs.size();
        nodes.clear();
        st.assign(1, root);
        while (!st.empty()) {
            const uint32_t n = st.back(); st.pop_back();
            nodes.push_back(n);
            if (ix->h_plane[n] >= 0) { st.push_back((uint32_t)ix->h_right[n]); st.push_back((uint32_t)ix->h_left[n]); }
        }
        // in pre-order the left child of local i is i + 1 and the right child i + 1 + size(left)
        for (uint32_t i = 0; i < nodes.size(); i++) {
            const uint32_t n = nodes[i];
            if (ix->h_plane[n] >= 0) {
                const uint32_t l = i + 1, r = i + 1 + size[(uint32_t)ix->h_left[n]];
                recs.push_back(make_int4(ix->h_plane[n], (int)(l | (r << 16)), i == 0 ? (int)nodes.size() : 0, (int)n));
            } else
                recs.push_back(make_int4(-1, ix->h_left[n], ix->h_right[n], (int)n));
        }
        n_blocks++;
        return -(int32_t)base - 1;
    };
    if (inner_only) place_blocks(ix, size, ZH_BLOCK_INNER, emit_inner, upper, roots);
    else place_blocks(ix, size, ZH_BLOCK_NODES, emit_whole, upper, roots);
    if (recs.size() > 0x7FFFFFF0ull || upper.size() > 0x7FFFFFF0ull) return fail(ZH_ELIMIT, "forest too large for the blocked view");
    recs.resize(recs.size() + ZH_BLOCK_NODES, make_int4(-1, 0, 0, 0));  // a wave always reads 64 records
    const size_t second_halves = inner_only ? recs.size() : 0;
    if (inner_only) {
        recsB.resize(recs.size(), make_int4(0, 0, 0, 0));
        recs.insert(recs.end(), recsB.begin(), recsB.end());  // one buffer: [first halves][second halves]
        std::vector<int4>().swap(recsB);
    }
    if (upper.empty()) upper.assign(2, make_int4(0, 0, 0, 0));
    zh_index::BlocksView &v = ix->blocks;
    int rc;
    if ((rc = v.recs.ensure(recs.size() * sizeof(int4)))) return rc;
    if ((rc = v.upper.ensure(upper.size() * sizeof(int4)))) return rc;
    if ((rc = v.roots.ensure(roots.size() * sizeof(int2)))) return rc;
    HIPCHK(hipMemcpy(v.recs.p, recs.data(), recs.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(v.upper.p, upper.data(), upper.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(v.roots.p, roots.data(), roots.size() * sizeof(int2), hipMemcpyHostToDevice));
    v.mark_built(n_blocks, (uint32_t)(upper.size() / 2), inner_only, second_halves);
    return ZH_OK;
}

// row -> {leaf node, position in the leaf} for every tree (the table-scan sweep's view of the forest): host pass for the
// node -> tree map (forest_walk), then one kernel over the leaves.  A failed allocation is remembered: the
// leaf-major sweep serves the index until the trees change.
static int build_row_leaf(zh_index *ix) {
    const size_t nn = ix->h_plane.size();
    const uint32_t T = (uint32_t)ix->h_roots.size();
    if (ix->row_leaf.table.ensure(std::max<uint64_t>(ix->n_rows * T, 1) * sizeof(uint2)) != ZH_OK) { ix->row_leaf.mark_failed(); return ZH_OK; }
    const std::vector<uint32_t> node_tree = forest_walk(ix, nullptr);
    DevBuf dTree;
    int rc = dTree.ensure(node_tree.size() * 4);
    if (rc) { ix->row_leaf.mark_failed(); return ZH_OK; }
    hipError_t e = hipMemcpy(dTree.p, node_tree.data(), node_tree.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = zh_launch_row_leaf(ix->node_pack.as<int4>(), dTree.as<uint32_t>(), (uint32_t)nn, ix->leaf_ids.as<uint32_t>(), T, ix->n_rows,
                               ix->row_leaf.table.as<uint2>(), ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    dTree.release();
    if (e != hipSuccess) return fail(ZH_EHIP, "row -> leaf table: %s", hipGetErrorString(e));
    ix->row_leaf.mark_built(ix->n_rows);
    return ZH_OK;
}

// the matrix-core scan's row order (under blk_mu; zh_order.hip), from the row -> leaf table, which must be valid for the stored rows.  Candidates:
// id order (rows inserted cluster by cluster are best left alone), sorted by (leaf in tree 0, leaf in tree 1, id), and by three trees' leaves; each
// is MEASURED -- (adjacent positions, tree) combinations that share a leaf = visitors a tile fetches once -- and the best one kept.
// order.rows = 0: id order (it won, there is no table, the order is switched off, or there is no room for the sort).  ZH_ROW_ORDER=0|2|3 forces one.
static int build_scan_perm(zh_index *ix) {
    const char *env_o = getenv("ZH_ROW_ORDER");  // (read when a copy is made: tests and A/B switch it)
    const int forced = env_o ? atoi(env_o) : -1;
    ix->order.begin();
    if (forced == 0 || ix->order.off || !ix->row_leaf.current(ix) || ix->n_rows < 32 || ix->n_rows > 0x7FFFFFF0ull) return ZH_OK;
    size_t mem_free = 0, mem_total = 0;  // the sort's scratch: ~28 bytes per row, released before the copy is made
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess || mem_free < ix->n_rows * 48 + mem_total / 16) return ZH_OK;
    DevBuf cand, dsum;
    if (ix->order.perm.ensure(ix->n_rows * 4) || cand.ensure(ix->n_rows * 4) || dsum.ensure(8)) { cand.release(); dsum.release(); return ZH_OK; }
    const uint2 *rl = ix->row_leaf.table.as<uint2>();
    const uint32_t T = ix->n_trees;
    auto worth = [&](const uint32_t *perm, unsigned long long *out) -> hipError_t {
        hipError_t e = zh_launch_order_agreement(rl, perm, ix->n_rows, T, dsum.as<unsigned long long>(), ix->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, dsum.p, 8, hipMemcpyDeviceToHost, ix->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
        return e;
    };
    unsigned long long best = 0, w = 0;
    hipError_t e = forced > 0 ? hipSuccess : worth(nullptr, &best);
    uint32_t best_keys = 0;
    for (uint32_t keys = 2; keys <= 3 && e == hipSuccess; keys++) {
        if (forced > 0 && (uint32_t)forced != keys) continue;
        if ((e = zh_launch_scan_order(rl, ix->n_rows, T, keys, cand.as<uint32_t>(), ix->stream)) != hipSuccess) break;
        if ((e = worth(cand.as<uint32_t>(), &w)) != hipSuccess) break;
        if (forced > 0 || w > best + best / 50) {  // (an order must be worth 2 % more than what there is)
            best = w; best_keys = keys;
            e = hipMemcpyAsync(ix->order.perm.p, cand.p, ix->n_rows * 4, hipMemcpyDeviceToDevice, ix->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
        }
    }
    cand.release(); dsum.release();
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return ZH_OK; }
    if (e != hipSuccess) return fail(ZH_EHIP, "row order of the scan: %s", hipGetErrorString(e));
    ix->order.mark_built(best_keys, (double)best / ((double)(ix->n_rows - 1) * T), ix->n_rows);
    return ZH_OK;
}
// The scan's inputs (half.tiles / half.meta, order.row_leaf_p, half128.copy) are rewritten IN PLACE when rows were appended, the forest changed or the row
// order is given up.  blk_mu orders the host threads that do it, not the GPU work of other contexts: a scan another pipelined context queued on the
// shared sweep stream (or its own) before this batch got here would read half-rewritten tiles.  Rewrites are rare (the first batch after an add /
// a rebuild): wait for everything the device has queued, then rewrite.  
static int quiesce_before_rewrite() {
    HIPCHK(hipDeviceSynchronize());
    return ZH_OK;
}
// the row -> leaf table in the scan's row order (under blk_mu; row_leaf must be valid)
static int ensure_row_leaf_p(zh_index *ix) {
    if (!ix->order.rows) return ZH_OK;
    if (ix->order.table_current(ix->row_leaf)) return ZH_OK;
    const uint32_t T = ix->n_trees;
    // the same headroom rule as the copies themselves: a sixteenth of the device stays free for the batches' scratch
    const uint64_t want_p = std::max<uint64_t>(ix->n_rows * T, 1) * sizeof(uint2);
    size_t mem_free = 0, mem_total = 0;
    if (want_p > ix->order.row_leaf_p.cap && (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess || mem_free < want_p + mem_total / 16)) { ix->order.no_room_for_table(); return ZH_OK; }
    int rc = quiesce_before_rewrite();
    if (rc) return rc;
    rc = ix->order.row_leaf_p.ensure(want_p);
    if (rc) { ix->order.no_room_for_table(); return ZH_OK; }  // (no room: the scan reads the table in id order -- but its tiles are in tree-0 order: the copy is remade)
    hipError_t e = zh_launch_permute_row_leaf(ix->row_leaf.table.as<uint2>(), ix->order.perm.as<uint32_t>(), ix->order.rows, ix->n_rows, T, ix->order.row_leaf_p.as<uint2>(), ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return fail(ZH_EHIP, "row -> leaf table in the scan's order: %s", hipGetErrorString(e));
    ix->order.mark_table(ix->row_leaf);
    return ZH_OK;
}

// The fp16 copy of the stored rows for the MFMA table scan (under blk_mu): rows appended since the last call only.  false: no room for it.
static int ensure_row_half(zh_index *ix, bool *ok) {
    *ok = false;
    if (ix->half.current(ix)) { *ok = !ix->half.failed; return ZH_OK; }
    const uint64_t d = ix->opt.dim, tiles = (ix->n_rows + 15) / 16;
    ix->half.retry();
    // room for it?  (a copy that grows is allocated anew before the old one is freed; a sixteenth of the device stays free for the batches' scratch)
    size_t mem_free = 0, mem_total = 0;
    const uint64_t want = std::max<uint64_t>(tiles, 1) * 16 * (d * 2 + sizeof(float2));
    const bool room = want <= ix->half.tiles.cap + ix->half.meta.cap ||
                      (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && mem_free >= want + want / 2 + mem_total / 16);
    // No room for the copy (64M x 768 on one GPU: 196 GB of rows + 98 GB), or ZH_ROW_HALF_META_ONLY=1 (tests; read per call): the per-row scales and
    // norms alone (8 bytes per row) -- scan_mfma_kernel<D, true> then converts the f32 rows itself, to the bits the copy would hold (round 6: the
    // same matrix-core scan at every N of the series)
    const char *mo_e = getenv("ZH_ROW_HALF_META_ONLY");
    const bool meta_only = !room || (mo_e && mo_e[0] == '1');
    if (meta_only) {
        const uint64_t want_meta = std::max<uint64_t>(tiles, 1) * 16 * sizeof(float2);
        const bool room_meta = want_meta <= ix->half.meta.cap || (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && mem_free >= want_meta + mem_total / 16);
        ix->half.tiles.release();
        if (!room_meta || ix->half.meta.ensure(want_meta, false, ix->stream) != ZH_OK || ix->half.rho_dev.ensure(4) != ZH_OK) {
            ix->half.meta.release();
            ix->half.mark_failed(ix);
            return ZH_OK;
        }
        int rcq = quiesce_before_rewrite();
        if (rcq) return rcq;
        ix->order.begin();  // (the f32 rows are in id order)
        HIPCHK(hipMemsetAsync(ix->half.rho_dev.p, 0, 4, ix->stream));
        HIPCHK(zh_launch_row_half(ix->X.as<float>(), 0, ix->n_rows, (uint32_t)d, nullptr, ix->half.meta.as<float2>(), ix->half.rho_dev.as<uint32_t>(), nullptr, 0, ix->stream));
        float rho_m = 0.f;
        HIPCHK(hipMemcpyAsync(&rho_m, ix->half.rho_dev.p, 4, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        ix->half.mark_built(ix, rho_m);
        *ok = true;
        return ZH_OK;
    }
    // a copy that was released (the meta-only state, or no room at all) holds none of the rows its stamp speaks of: made again from row 0
    const bool had_copy = ix->half.tiles.p && ix->half.meta.p;
    if (ix->half.tiles.ensure(std::max<uint64_t>(tiles, 1) * 16 * d * 2, true, ix->stream) != ZH_OK ||
        ix->half.meta.ensure(std::max<uint64_t>(tiles, 1) * 16 * sizeof(float2), true, ix->stream) != ZH_OK || ix->half.rho_dev.ensure(4) != ZH_OK) {
        ix->half.tiles.release(); ix->half.meta.release();
        ix->half.mark_failed(ix);
        return ZH_OK;
    }
    uint64_t from = ix->half.at.rows;
    {
        const int rcq = quiesce_before_rewrite();
        if (rcq) return rcq;
    }
    // rows appended since the order was made keep position = id and share no tile with their leaf mates: once they are a quarter of the table
    // the copy is made again, in an order measured on all of it
    const bool stale_order = ix->order.rows && ix->n_rows - ix->order.rows > ix->order.rows / 4;
    if (!had_copy || ix->half.at.gen != ix->rows_gen || from > ix->n_rows || stale_order) {
        from = 0;
        HIPCHK(hipMemsetAsync(ix->half.rho_dev.p, 0, 4, ix->stream));
    }
    if (from == 0) {  // a copy made from scratch: in tree-0 leaf order where the forest allows (rows appended later keep position = id)
        int rcp = build_scan_perm(ix);
        if (rcp) return rcp;
    }
    HIPCHK(zh_launch_row_half(ix->X.as<float>(), from, ix->n_rows - from, (uint32_t)d, ix->half.tiles.p, ix->half.meta.as<float2>(),
                              ix->half.rho_dev.as<uint32_t>(), ix->order.rows ? ix->order.perm.as<uint32_t>() : nullptr, ix->order.rows, ix->stream));
    float rho = 0.f;
    HIPCHK(hipMemcpyAsync(&rho, ix->half.rho_dev.p, 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->half.mark_built(ix, rho);
    *ok = true;
    return ZH_OK;
}

// The row-major fp16 copy of a d = 128 table under one scale (under blk_mu).  Appended rows that fit the scale are added; a larger element
// than the scale allows re-makes the copy.  want_bytes: the caller's kernels can read the 128-byte copy of a table of integers 0 .. 255 -- made
// instead whenever every stored row qualifies (an appended row that does not re-makes the copy in halves); the two kinds share the buffer, and a
// caller that wants the other kind than the one present (tests switching kernels) gets the copy re-made.
static int ensure_row_half128(zh_index *ix, bool *ok, bool want_bytes) {
    *ok = false;
    zh_index::RowHalf128View &v = ix->half128;
    const bool bytes = want_bytes && !v.not_bytes;
    if (v.current(ix) && (v.failed || v.bytes == bytes)) { *ok = !v.failed; return ZH_OK; }
    v.retry();
    size_t mem_free = 0, mem_total = 0;
    const uint64_t want = std::max<uint64_t>(ix->n_rows, 1) * (bytes ? 128 : 256);
    const bool room = want <= ix->half128.copy.cap || (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && mem_free >= want + want / 2 + mem_total / 16);
    if (!room || ix->half128.copy.ensure(want, true, ix->stream) != ZH_OK || ix->half.rho_dev.ensure(12) != ZH_OK) {
        ix->half128.copy.release();
        v.mark_failed(ix);
        return ZH_OK;
    }
    uint64_t from = v.extend_from(ix, bytes);
    {
        const int rcq = quiesce_before_rewrite();
        if (rcq) return rcq;
    }
    if (bytes) {
        uint32_t *dflag = ix->half.rho_dev.as<uint32_t>() + 2, flag = 0;
        HIPCHK(hipMemsetAsync(dflag, 0, 4, ix->stream));
        HIPCHK(zh_launch_row_byte128(ix->X.as<float>(), from, ix->n_rows - from, ix->half128.copy.p, dflag, ix->stream));
        HIPCHK(hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        if (!flag) {
            v.mark_bytes(ix);
            *ok = true;
            return ZH_OK;
        }
        v.found_not_bytes();  // some row is not a row of bytes: the copy of halves, from the first row, now and from now on
        return ensure_row_half128(ix, ok, false);
    }
    uint32_t *dmax = ix->half.rho_dev.as<uint32_t>() + 1;
    for (int pass = 0; pass < 2; pass++) {
        uint32_t mbits = 0;
        HIPCHK(hipMemsetAsync(dmax, 0, 4, ix->stream));
        HIPCHK(zh_launch_absmax(ix->X.as<float>() + from * 128, (ix->n_rows - from) * 128, dmax, ix->stream));
        HIPCHK(hipMemcpyAsync(&mbits, dmax, 4, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        float m;
        memcpy(&m, &mbits, 4);
        int ex = 14;
        if (m > 0.f) (void)frexpf(m, &ex);
        ex = std::min(std::max(ex, -100), 100);
        if (from == 0) { v.set_scale(ex); break; }
        if (ex <= v.ex) break;
        from = 0;  // the appended rows do not fit the scale: the whole copy again, under theirs
    }
    if (from == 0) HIPCHK(hipMemsetAsync(ix->half.rho_dev.p, 0, 4, ix->stream));
    HIPCHK(zh_launch_row_half128(ix->X.as<float>(), from, ix->n_rows - from, ldexpf(1.f, 14 - v.ex), ix->half128.copy.p,
                                 ix->half.rho_dev.as<uint32_t>(), ix->stream));
    float rho = 0.f;
    HIPCHK(hipMemcpyAsync(&rho, ix->half.rho_dev.p, 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    v.mark_halves(ix, from == 0 ? rho : std::max(rho, v.rho.load()));
    *ok = true;
    return ZH_OK;
}

// Leaf by leaf or the whole table once?  The leaf-major sweep gathers group_rows rows from HBM (5.9-6.1 TB/s of 3-KB rows,
// 5.5 TB/s of 512-byte ones); the table scan streams every stored row once (plus 8 bytes per tree of row -> leaf entries) and
// fetches one query from L2 per scored (row, query) pair -- measured 0.075 + 0.00022 d ns per pair chip-wide (4.1 G pairs/s
// at d = 768 = what the L2s deliver; 10 G pairs/s at d = 128 with the paired kernel, where the leaf-major sweep still wins at the BASELINE shapes), slower once the window's queries no
// longer fit beside the stream in the 8 x 4 MB of L2.  zh_set_sweep_mode / ZH_SWEEP_MODE=leaf|scan force one of them.
static bool use_approx(const zh_index *ix, const ZhTotals &tot, size_t B, size_t k, int metric);
// The half-width scan on the matrix cores (scan_mfma_kernel) where it has a kernel and the index can keep an fp16 copy of its rows
// (+50 % of the row table; ensure_row_half): mode 5 keeps the VALU kernel, which reads the f32 rows.
static bool mfma_wanted(const zh_index *ix) {
    return ix->sweep_mode != 5 && zh_scan_mfma_supported(ix->opt.dim, ix->n_trees) && !ix->fb.mfma_f32_off && !ix->half.known_failed(ix);
}
// the sweep a batch is asked for: zh_set_sweep_mode where it names one (0 and 3 leave the choice open), else ZH_SWEEP_MODE=leaf|scan|approx (read
// once); 5 asks for what 4 does (only mfma_wanted tells them apart).  0: chosen per batch
static int asked_sweep_mode(const zh_index *ix) {
    static const int forced = [] { const char *e = getenv("ZH_SWEEP_MODE"); return !e ? 0 : (e[0] == 's' ? 2 : (e[0] == 'a' ? 4 : 1)); }();
    const int sm_ = ix->sweep_mode.load();
    const int mode = sm_ == 3 ? forced : (sm_ ? sm_ : forced);
    return mode == 5 ? 4 : mode;
}
static bool choose_scan(const zh_index *ix, const ZhTotals &tot, int metric, size_t B, size_t k) {
    const uint32_t d = ix->opt.dim, T = ix->n_trees;
    int mode = asked_sweep_mode(ix);
    if (mode == 6) mode = 1;
    if (mode == 1 || !zh_scan_sweep_supported(d, T, metric) || ix->row_leaf.failed || ix->scan_unsafe) return false;
    if (mode == 2 || mode == 4) return true;
    if (!ix->row_leaf.valid && ix->fb.batches_since_change.load() < 3) return false;  // (the row -> leaf table is built for a forest that stays)
    const double row_b = 4.0 * d;
    const double t_leaf = (double)tot.group_rows * row_b / (d >= 256 ? 6.0e12 : 5.5e12);
    // with half-width queries (zh_approx.hip) a pair pulls 2 d bytes through the vector L1 instead of 4 d: measured 0.157 ns per pair at
    // d = 768 (cfg3, window 2, profiles/r04_*), and twice the queries fit beside the stream in L2
    const bool half = use_approx(ix, tot, B, k, metric), mfma = half && mfma_wanted(ix);
    const double q_bytes = (double)B * row_b * (half ? 0.5 : 1.0);
    // (on the matrix cores: 3.4-3.5 ms per 3.33M rows + 28.6M pairs at d = 768, window 2 -- the L2s' rate for 2 d bytes per pair; the rows are fp16 too)
    const double pair_s = mfma ? 0.02e-9 + 0.00011e-9 * d
                        : half ? 0.05e-9 + 0.00014e-9 * d
                               : (d == 128 ? 0.10e-9 : 0.075e-9 + 0.00022e-9 * d);  // (d = 128: the paired kernel, two pairs per step)
    const double t_pairs = (double)tot.rows * pair_s * (q_bytes > 8e6 ? 1.25 : 1.0);
    const double t_scan = std::max((double)ix->n_rows * (row_b * (mfma ? 0.5 : 1.0) + 8.0 * T) / 6.0e12, t_pairs) + 20e-6;
    return t_scan < 0.92 * t_leaf;
}

// The table scan with half-width queries (zh_approx.hip) instead of the f32 one?  Wherever it applies: the metrics whose key a dot
// product determines, the dimensions its groups divide, batches in the few-visits-per-pair regime (long leaves) whose candidate
// lists fit the per-query sort.  ZH_SWEEP_MODE=scan / zh_set_sweep_mode(2) keep the f32 scan; =approx / mode 4 say so explicitly.
static bool use_approx(const zh_index *ix, const ZhTotals &tot, size_t B, size_t k, int metric) {
    const int mode = asked_sweep_mode(ix);
    if (mode == 2 || mode == 1 || mode == 6) return false;
    if (!zh_scan_approx_supported(ix->opt.dim, ix->n_trees, metric) || k > 256 || B == 0 || B >= (1u << 24)) return false;  // (24 bits of a packed pair record)
    if (tot.takes > 2048ull * B || tot.visits > 8ull * B * ix->n_trees) return false;
    // by itself only where it pays: per pair it moves half the bytes, but a window of ONE cfg3 batch (4.3 pairs per stored row) gains 4 % on
    // the scan (3.28 against 3.42 ms per launch) and pays more than that for the interval stages: from ~5 pairs per stored row on
    // (the matrix-core kernel reads half the row bytes as well and multiplies for nothing: measured from d = 256 and ~2 pairs per stored row on)
    const bool mfma = mfma_wanted(ix);
    if (mode != 4 && (ix->fb.approx_strikes.load() >= 2 || !(mfma ? ix->opt.dim >= 256 : zh_approx_pays(ix->opt.dim)) ||
                      tot.rows < (mfma ? 2 : 5) * ix->n_rows))
        return false;
    return true;
}

// The leaf-major sweep of a d = 128 table at half width (sweep128h_kernel)?  Where the f32 sweep is what HBM gives random 512-byte rows: long
// leaves, many scored rows; the same list limits as the half-width scan.  zh_set_sweep_mode(6) asks for it wherever it is implemented,
// (1) keeps the f32 sweep.
static bool use_approx_leaf(const zh_index *ix, const ZhTotals &tot, size_t B, size_t k, int metric) {
    static const bool env_sweep = getenv("ZH_SWEEP_MODE") != nullptr;
    if (ix->opt.dim != 128 || !zh_sweep_has_predicate(128, metric)) return false;
    if (ix->sweep_mode != 6 && (env_sweep || (ix->sweep_mode != 0 && ix->sweep_mode != 3))) return false;
    if (k > 256 || B == 0 || B >= (1u << 24) || tot.takes > 2048ull * B || tot.visits > 8ull * B * ix->n_trees) return false;
    if (ix->half128.known_failed(ix)) return false;
    if (ix->sweep_mode != 6 && (ix->fb.approx_strikes.load() >= 2 || tot.group_rows < (4u << 20))) return false;
    return true;
}

static bool use_score_hash(const zh_index *ix, size_t B, uint32_t P_dense);
// estimated time of the row-score hash of a batch: the score GEMM (or its row-streaming bound), the gather of two score rows per
// plane (>= one 64-byte sector each), the exact fix-ups
static double score_hash_seconds(const zh_index *ix, size_t B) {
    const size_t Bp = (B + 3) & ~(size_t)3;
    const double d = ix->opt.dim, P = ix->n_planes, N = ix->n_rows;
    return std::max(2.0 * Bp * N * d / 9e13, N * d * 4.0 / 5e12) + P * 2.0 * std::max(64.0, Bp * 4.0) / 4e12 + 0.003 * B * P * 0.55e-9 + 30e-6;
}
// number of leading planes hashed densely (MFMA kernel, before the walk) for a batch of B queries asking for k neighbours
static uint32_t choose_dense_planes(zh_index *ix, size_t B, size_t k) {
    const auto &below = ix->planes_below_level;
    if (below.size() <= 1 || ix->n_planes == 0) return 0;
    if (ix->dense_levels >= 0) return below[std::min<size_t>((size_t)ix->dense_levels, below.size() - 1)];
    // The top levels, shared by every query, always go to the MFMA kernel (a 2 GFLOP budget: tens of microseconds).
    const double d = ix->opt.dim, per_plane = 2.0 * (double)B * d;
    uint32_t top = 0;
    for (size_t L = 1; L < below.size(); L++)
        if ((double)below[L] * per_plane <= 2e9) top = below[L];
    // Below them a pair either hashes the planes it meets on demand (a 16-lane ordered fma chain per plane) or finds every
    // sign precomputed.  With leaves comfortably >= k a pair meets ~depth planes and on demand is all but free; with
    // small leaves (the reference's defaults, max_node_size 5 < top_k) the walk wanders over a good part of every tree
    //  and the dense kernel, ~20x cheaper per sign, wins although it hashes planes nobody asks for.  The
    // visits per pair of the previous batches decide; measured constants (MI355X): 90 TF for the dense kernel, 1.4 us per
    // step of the slowest pair (~5x the mean visit count) or 0.7 us of a SIMD per four steps when waves queue.
    double vpp;
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        vpp = ix->visits_per_pair;
    }
    if (vpp <= 0) vpp = (size_t)ix->opt.max_node_size < 2 * k + 2 ? 1000.0 : 2.0;
    const double pairs = (double)B * ix->n_trees;
    const double t_chain = std::max(1.4e-6 * 5.0 * vpp, pairs / 4.0 * 2.3 * vpp * 0.7e-6 * (d / 384.0) / 1024.0);
    // the dense kernel: MFMA-bound for real batches, a plane-streaming GEMV (HBM-bound) for a handful of queries
    const double t_dense = std::max((double)ix->n_planes * per_plane / 9e13, (double)ix->n_planes * d * 4.0 / 5e12);
    const double bits_bytes = (double)ix->n_planes * (double)B / 8.0;
    // ... or every sign from the row scores (zh_score.hip) -- counted only where use_score_hash would in fact take that path for an
    // all-dense batch (same mode switch, same ZH_HASH_MODE, same limits, same threshold: ONE decision), so that "all-dense because the
    // scores are cheap" is never followed by the per-plane dense hash
    double t_all = t_dense;
    if (use_score_hash(ix, B, ix->n_planes)) t_all = std::min(t_all, score_hash_seconds(ix, B));
    if (t_all < t_chain && bits_bytes < 2e9) return ix->n_planes;  // (every context in flight holds its own sign bits)
    return top;
}

// All signs of the batch from N row scores per query instead of P dot products (zh_score.hip)?  Only for forests whose planes
// are known differences of stored rows, when every plane is hashed anyway, and when the score table fits.
static bool use_score_hash(const zh_index *ix, size_t B, uint32_t P_dense) {
    static const int forced = [] { const char *e = getenv("ZH_HASH_MODE"); return !e ? 0 : (e[0] == 's' ? 2 : 1); }();
    const int mode = ix->hash_mode ? ix->hash_mode : forced;
    if (mode == 1 || !ix->samples.valid || ix->n_planes == 0 || P_dense < ix->n_planes) return false;
    const size_t Bp = (B + 3) & ~(size_t)3;  // (the kernels take queries four at a time: the batch is padded with zero queries)
    if ((uint64_t)ix->n_rows * Bp * 4 > (12ull << 30) || ix->n_rows > 0xFFFFFFF0ull) return false;  // the score table of ONE context (288 GB of HBM)
    if (mode == 2) return true;
    // per-plane hash: MFMA-bound for real batches, a plane-streaming GEMV for a handful of queries; row scores: the same two
    // bounds over the ROWS, + the gather of two score rows per plane (>= one 64-byte sector each) + the exact fix-ups
    const double d = ix->opt.dim, P = ix->n_planes;
    const double t_dense = std::max(2.0 * B * P * d / 9e13, P * d * 4.0 / 5e12);
    return score_hash_seconds(ix, B) < 0.7 * t_dense;
}

static int launch_score_hash(zh_search_ctx *c, const float *dQ, size_t B, bool lazy, hipStream_t s) {
    zh_index *ix = c->ix;
    const uint32_t d = ix->opt.dim;
    int rc;
    if (!ix->norms.current(ix)) {  // rows were added (or replaced: clear) since the norms were taken
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if (!ix->norms.current(ix)) {
            if ((rc = ix->norms.hn2.ensure(ix->n_rows * 4)) || (rc = ix->norms.norm.ensure(ix->n_rows * 4))) return rc;
            HIPCHK(zh_launch_row_norms(ix->X.as<float>(), ix->n_rows, d, ix->norms.hn2.as<float>(), ix->norms.norm.as<float>(), ix->stream));
            HIPCHK(hipStreamSynchronize(ix->stream));
            ix->norms.mark_built(ix);
        }
    }
    if (!ix->plane_norms.current(ix)) {  // planes were added, or the norms retaken
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if (!ix->plane_norms.current(ix)) {
            if ((rc = ix->plane_norms.hab.ensure(std::max<size_t>(ix->n_planes, 1) * sizeof(float4)))) return rc;
            HIPCHK(zh_launch_plane_hab(ix->samples.pairs.as<uint2>(), ix->n_planes, ix->norms.hn2.as<float>(), ix->norms.norm.as<float>(),
                                       ix->plane_norms.hab.as<float4>(), ix->stream));
            HIPCHK(hipStreamSynchronize(ix->stream));
            ix->plane_norms.mark_built(ix);
        }
    }
    if (B % 4) {  // pad the batch with zero queries to a multiple of four (their signs are computed and never read)
        const size_t Bp = (B + 3) & ~(size_t)3;
        if ((rc = c->wQpad.ensure(Bp * d * 4)) || (rc = c->wBits.ensure(Bp * c->wpq * 4))) return rc;
        if (lazy && (rc = c->wUnc.ensure(Bp * c->wpq * 4))) return rc;
        HIPCHK(hipMemcpyAsync(c->wQpad.p, dQ, B * d * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemsetAsync(c->wQpad.as<float>() + B * d, 0, (Bp - B) * d * 4, s));
        dQ = c->wQpad.as<float>();
        B = Bp;
    }
    c->score_Bp = (uint32_t)B;
    const uint32_t wq = (uint32_t)((B + 63) / 64 * 2);  // sign words per ROW of the score GEMM's (unused) bit output
    const uint64_t cap64 = (uint64_t)B * ix->n_planes / 64 + (1u << 16);  // ~1.6 % of the signs: 4x the share seen on ~N(0,1) rows
    const uint32_t fix_cap = (uint32_t)std::min<uint64_t>(cap64, 0x7FFFFFFFull);
    if ((rc = c->wScore.ensure((size_t)ix->n_rows * B * 4))) return rc;
    if ((rc = c->wJunkBits.ensure((size_t)ix->n_rows * wq * 4))) return rc;
    if ((rc = c->wQnorm.ensure(B * 4))) return rc;
    if ((rc = c->wFixList.ensure((size_t)fix_cap * sizeof(uint2)))) return rc;
    if (c->wZeros.cap < B * 4) {
        if ((rc = c->wZeros.ensure(B * 4))) return rc;
        HIPCHK(hipMemsetAsync(c->wZeros.p, 0, c->wZeros.cap, s));
    }
    // S[row][q] = row . query: the MFMA hash kernel with the roles swapped (stored rows as "queries", the batch as B "planes");
    // a batch of <= 4 queries: one stream over the stored rows
    if (B == 4)
        HIPCHK(zh_launch_row_scores4(ix->X.as<float>(), ix->n_rows, d, dQ, c->wScore.as<float>(), s));
    else
        HIPCHK(zh_launch_hash_dense(ix->X.as<float>(), (uint32_t)ix->n_rows, dQ, c->wZeros.as<float>(), (uint32_t)B, d, c->wJunkBits.as<uint32_t>(), wq,
                                    c->wScore.as<float>(), s));
    HIPCHK(zh_launch_row_norms(dQ, B, d, nullptr, c->wQnorm.as<float>(), s));
    ZhTotals *tot = c->wTotals.as<ZhTotals>();
    HIPCHK(zh_launch_score_signs(c->wScore.as<float>(), (uint32_t)B, ix->samples.pairs.as<uint2>(), ix->n_planes, ix->norms.hn2.as<float>(),
                                 ix->norms.norm.as<float>(), ix->plane_norms.hab.as<float4>(), c->wQnorm.as<float>(), dQ, d, ix->planes.as<float>(), ix->consts.as<float>(),
                                 c->wBits.as<uint32_t>(), c->wpq, c->wFixList.as<uint2>(), fix_cap, &tot->hash_fixups,
                                 lazy ? c->wUnc.as<uint32_t>() : nullptr, s));
    return ZH_OK;
}

int ctx_wait(zh_search_ctx *c);

// A batch hashed from row scores can pick its candidates from them (zh_search.hip, "Prefilter"): for the metrics the scores
// determine, leaves short enough for the per-lane selection, and forests this library built (a row is in one leaf per tree).
static bool use_prefilter(const zh_index *ix, const zh_search_ctx *c, size_t k, int metric) {
    // (mode 3 keeps trying past two strikes -- a caller who knows the overflows are rare -- but not past eight in a row: every one is a batch computed twice)
    const uint32_t strikes = ix->fb.prefilter_strikes.load();
    if (!c->score_hash || c->prefilter_off_once || c->stream_ordered || (strikes >= 2 && ix->sweep_mode != 3) || strikes >= 8) return false;
    static const bool env_sweep = getenv("ZH_SWEEP_MODE") != nullptr;
    if ((ix->sweep_mode != 0 && ix->sweep_mode != 3) || (env_sweep && ix->sweep_mode != 3)) return false;  // a sweep was asked for
    if (metric != ZH_L2SQ && metric != ZH_L2 && metric != ZH_COSINE) return false;
    // leaves of <= 8 rows are judged per lane; the odd longer one (rows a split could not separate) is a visit for the exact path
    if (ix->opt.max_node_size > 8 || ix->max_leaf_len == 0 || ix->max_leaf_len > 64 || k > 64 || ix->scan_unsafe || !ix->n_leaf_ids) return false;
    return true;
}

static int build_leaf_meta(zh_index *ix) {  // under blk_mu; the norms are those launch_score_hash just validated
    int rc;
    if ((rc = ix->leaf_meta.slots.ensure(ix->n_leaf_ids * sizeof(float4)))) return rc;
    HIPCHK(zh_launch_leaf_meta(ix->leaf_ids.as<uint32_t>(), ix->n_leaf_ids, ix->norms.hn2.as<float>(), ix->norms.norm.as<float>(),
                               ix->leaf_meta.slots.as<float4>(), ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->leaf_meta.mark_built(ix);
    return ZH_OK;
}

static ZhWalkLog walk_log(const zh_search_ctx *c) {
    ZhWalkLog l;
    l.pool = c->wLogPool.as<uint2>();
    l.capacity = (uint32_t)std::min<size_t>(c->log_chunks, 0xFFFFFFFEu);
    l.head = c->wLogHead.as<uint32_t>();
    l.ctl = c->wLogCtl.as<ZhLogCtl>();
    // a prefiltered batch with leaves the entry's 16 bits can hold logs {leaf offset, take | length << 16}: prefilter_kernel then
    // reads no node record per visit (1.1 GB of 64-byte sectors and a dependent round trip per 63 visits at the reference's defaults)
    l.leaf_entries = c->prefilter && c->ix->max_leaf_len <= 64 && c->k <= 0xFFFF ? 1u : 0u;
    return l;
}

// first half of a batch: hash, the walk's counting pass, scans; the three totals travel to the host
static int ctx_begin(zh_search_ctx *c, const float *const *dQs, size_t nwin, size_t bwin, size_t k, int metric, int mode,
                     hipStream_t s) {
    zh_index *ix = c->ix;
    const uint32_t d = ix->opt.dim, T = ix->n_trees;
    const size_t B = nwin * bwin;
    const float *dQ = dQs[0];
    int rc;
    if (c->state == 1) return fail(ZH_ESTATE, "zh_search_begin: the context already has a batch begun; finish it first");
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (ix->broken) return fail(ZH_ESTATE, "an earlier zh_index_add failed half way: call zh_index_build before searching");
    if (c->state == 2 && (rc = ctx_wait(c))) return rc;  // the previous batch was never waited for: retire it
    c->dQ = dQ; c->B = B; c->k = k; c->metric = metric; c->mode = mode; c->s = s;
    c->nwin = nwin; c->bwin = bwin;
    c->trivial = (B == 0 || k == 0 || ix->n_rows == 0 || T == 0);  // core.rs:295-297: empty index -> no neighbours
    c->approx = false; c->approx_leaf = false; c->approx_mfma = false; c->approx_fused = false; c->approx_bytes = false;
    c->state = 1;
    if (c->trivial) return ZH_OK;
    const uint64_t pairs = (uint64_t)B * T;
    if (pairs >= (1ull << 26)) { c->state = 0; return fail(ZH_ELIMIT, "batch * num_trees >= 2^26"); }
    c->P_dense = choose_dense_planes(ix, B, k);
    const uint32_t seen = ix->fb.batches_since_change.fetch_add(1);
    if (c->P_dense >= ix->n_planes && ix->n_planes && !ix->blocks.valid && seen >= 2) {  // the forest has been stable for a few batches
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if (!ix->blocks.valid && (rc = build_blocks(ix))) { c->state = 0; return rc; }
    }
    c->wpq = (c->P_dense + 255) / 256 * 8;  // sign words per query, a multiple of eight: score_signs_kernel stores whole 32-byte sectors
    const size_t nn = std::max<uint32_t>(ix->n_nodes, 1);
    c->state = 0;  // a failure below leaves the context idle
    if (nwin > 1) {  // the window's batches side by side: the kernels address query b of the window as Q + b * d
        if ((rc = c->wQwin.ensure(B * d * 4))) return rc;
        for (size_t j = 0; j < nwin; j++)
            HIPCHK(hipMemcpyAsync(c->wQwin.as<float>() + j * bwin * d, dQs[j], bwin * d * 4, hipMemcpyDeviceToDevice, s));
        c->dQ = dQ = c->wQwin.as<float>();
    }
    if ((rc = c->wQQ.ensure(B * 4))) return rc;
    if ((rc = c->wBits.ensure(std::max<size_t>((size_t)B * c->wpq * 4, 4)))) return rc;
    if ((rc = c->wCounts.ensure(pairs * sizeof(ZhPairCounts)))) return rc;
    if ((rc = c->wInline.ensure(pairs * ZH_INLINE_VISITS * sizeof(ZhVisit)))) return rc;
    if ((rc = c->wRowBase.ensure((pairs + 1) * 8))) return rc;
    if ((rc = c->wCandBase.ensure((pairs + 1) * 8))) return rc;
    if ((rc = c->wVisitBase.ensure((pairs + 1) * 8))) return rc;
    if ((rc = c->wTotals.ensure(sizeof(ZhTotals)))) return rc;
    if ((rc = c->wLeafCount.ensure(nn * 4))) return rc;
    if ((rc = c->wLeafFill.ensure(nn * 4))) return rc;
    if ((rc = c->wGroupBase.ensure(nn * 4))) return rc;
    if ((rc = c->wGroupRowBase.ensure(nn * 8))) return rc;
    if ((rc = c->wLogHead.ensure(pairs * 4))) return rc;
    if ((rc = c->wLogCtl.ensure(sizeof(ZhLogCtl)))) return rc;
    if (!c->wLogPool.p) {
        static const size_t first_env = [] { const char *e = getenv("ZH_WALK_LOG_CHUNKS"); return e ? (size_t)atoll(e) : (size_t)0; }();
        size_t first = first_env ? first_env : 8192;
        if (!first_env) {  // a context created after the index has served batches starts with a log that fits what those batches logged
            std::lock_guard<std::mutex> lk(ix->stats_mu);
            const double v = ix->visits_per_pair * (double)pairs;
            if (v > 0) first = std::max<size_t>(first, (size_t)(1.5 * (v / (ZH_LOG_CHUNK - 1) + (double)pairs)) + 16);
        }
        if ((rc = c->wLogPool.ensure(std::max<size_t>(first, 1) * ZH_LOG_CHUNK * sizeof(uint2)))) return rc;
        c->log_chunks = std::max<size_t>(first, 1);
    }
    c->score_hash = use_score_hash(ix, B, c->P_dense);
    c->prefilter = use_prefilter(ix, c, k, metric);
    c->sv_q.assign(dQs, dQs + nwin);
    // a prefiltered batch forms no leaf groups: no per-leaf visit counts to zero, to bump from the walk, or to scan afterwards
    uint32_t *leaf_count = c->prefilter ? nullptr : c->wLeafCount.as<uint32_t>();
    HIPCHK(zh_launch_batch_init(c->wLeafCount.as<uint32_t>(), c->wLeafFill.as<uint32_t>(), c->prefilter ? 0u : (uint32_t)nn, c->wLogCtl.as<ZhLogCtl>(),
                                c->wTotals.as<ZhTotals>(), s));
    ZhForestDev f = forest_dev(ix);
    HIPCHK(hipEventRecord(c->ev[0], s));
    if (metric == ZH_COSINE) HIPCHK(zh_launch_qnorm(dQ, (uint32_t)B, d, c->wQQ.as<float>(), s));
    const bool blocked = c->P_dense >= ix->n_planes && ix->n_planes && ix->blocks.valid;
    c->lazy_fix = c->score_hash && blocked && ((B + 3) & ~(size_t)3) != 4 && d % 4 == 0;  // (plane_above_wave's shape)
    if (c->lazy_fix && (rc = c->wUnc.ensure(std::max<size_t>((size_t)B * c->wpq * 4, 4)))) return rc;
    if (c->score_hash) {
        if ((rc = launch_score_hash(c, dQ, B, c->lazy_fix, s))) return rc;
    } else if (c->P_dense)
        HIPCHK(zh_launch_hash_dense(dQ, (uint32_t)B, f.planes, f.consts, c->P_dense, d, c->wBits.as<uint32_t>(), c->wpq, nullptr, s));
    HIPCHK(hipEventRecord(c->ev[1], s));
    if (blocked) {
        ZhBlocksDev bd;
        bd.recs = ix->blocks.recs.as<int4>(); bd.upper = ix->blocks.upper.as<int4>(); bd.root = ix->blocks.roots.as<int2>();
        bd.n_blocks = ix->blocks.n_blocks; bd.n_upper = ix->blocks.n_upper; bd.inner_only = ix->blocks.inner ? 1u : 0u;
        bd.recs_b = ix->blocks.inner ? bd.recs + ix->blocks.recs_b.load() : nullptr;
        HIPCHK(zh_launch_walk_blocked(f, bd, (uint32_t)B, (int32_t)k, c->wBits.as<uint32_t>(), c->wpq, c->wCounts.as<ZhPairCounts>(),
                                      c->wInline.as<ZhVisit>(), leaf_count, walk_log(c), c->lazy_fix ? c->wUnc.as<uint32_t>() : nullptr, dQ, d, s));
    } else
        HIPCHK(zh_launch_walk_count(f, dQ, (uint32_t)B, d, (int32_t)k, c->wBits.as<uint32_t>(), c->wpq, c->P_dense,
                                    c->wCounts.as<ZhPairCounts>(), c->wInline.as<ZhVisit>(), leaf_count, walk_log(c), s));
    if (!c->prefilter)
        HIPCHK(zh_launch_leaf_scan(f, c->wLeafCount.as<uint32_t>(), c->wGroupBase.as<uint32_t>(),
                                   c->wGroupRowBase.as<uint64_t>(), c->wTotals.as<ZhTotals>(), s));
    HIPCHK(zh_launch_pair_scan(c->wCounts.as<ZhPairCounts>(), (uint32_t)pairs, c->wRowBase.as<uint64_t>(),
                               c->wCandBase.as<uint64_t>(), c->wVisitBase.as<uint64_t>(), c->wTotals.as<ZhTotals>(),
                               c->wLogCtl.as<ZhLogCtl>(), s));
    HIPCHK(hipMemcpyAsync(c->h_totals, c->wTotals.p, sizeof(ZhTotals), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(c->ev_totals, s));
    c->state = 1;
    return ZH_OK;
}

// second half of a prefiltered batch: candidates from the row scores -> the exact path for what they cannot decide -> exact keys
// of the few survivors -> final top-k over num_trees short lists per query
static int finish_prefilter(zh_search_ctx *c, uint64_t *dOutIds, uint64_t *dOutKeys, uint32_t *dOutCounts, uint64_t *const *outIds,
                            uint64_t *const *outKeys, uint32_t *const *outCounts) {
    zh_index *ix = c->ix;
    const uint32_t d = ix->opt.dim, T = ix->n_trees;
    const size_t B = c->B, k = c->k, nwin = c->nwin, bwin = c->bwin;
    hipStream_t s = c->s;
    int rc;
    if (!ix->leaf_meta.current(ix)) {
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if (!ix->leaf_meta.current(ix) && (rc = build_leaf_meta(ix))) return rc;
    }
    const char *cap_e = getenv("ZH_PREFILTER_CAP");  // tests: lists that run over (read per batch)
    const uint32_t cap_env = cap_e ? (uint32_t)atoi(cap_e) : 0u;
    const uint32_t cap = cap_env ? std::max<uint32_t>(cap_env, 1) : (k <= 16 && c->metric != ZH_COSINE ? 64u : (k <= 32 ? 128u : 256u));
    // (cosine with parity keys: "nearest" is the smallest non-negative cosine, where candidates are densest, and every row within the
    // bound of ZERO is a legitimate top candidate from the exact pass: ~49 rows per list at d = 768, batch 196 -- 64 slots ran over)
    const uint64_t lists = (uint64_t)B * T;
    const uint32_t amb_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096, c->tot.visits / 32 + 1024), 1u << 26);
    c->pf_cap = cap;
    if ((rc = c->wPfRows.ensure(lists * cap * 4)) || (rc = c->wPfCounts.ensure(lists * 8)) || (rc = c->wPfKeys.ensure(lists * cap * 8)) ||
        (rc = c->wPfIds.ensure(lists * cap * 8)) || (rc = c->wPfAmb.ensure((size_t)amb_cap * sizeof(uint4))) || (rc = c->wPfCtl.ensure(16)))
        return rc;
    HIPCHK(hipMemsetAsync(c->wPfCtl.p, 0, 16, s));
    ZhPrefilter pf;
    pf.S = c->wScore.as<float>(); pf.Bp = c->score_Bp; pf.leaf_meta = ix->leaf_meta.slots.as<float4>(); pf.qnorm = c->wQnorm.as<float>();
    pf.rows = c->wPfRows.as<uint32_t>(); pf.counts = c->wPfCounts.as<uint32_t>(); pf.tau = reinterpret_cast<float *>(pf.counts + lists); pf.cap = cap;
    pf.amb = c->wPfAmb.as<uint4>(); pf.amb_cap = amb_cap; pf.ctl = c->wPfCtl.as<uint32_t>();
    ZhForestDev f = forest_dev(ix);
    HIPCHK(hipEventRecord(c->ev[2], s));
    HIPCHK(hipEventRecord(c->ev_sw0, s));
    HIPCHK(zh_launch_prefilter(f, d, (uint32_t)B, (uint32_t)k, c->metric, c->mode, c->wCounts.as<ZhPairCounts>(), c->wInline.as<ZhVisit>(),
                               walk_log(c), pf, s));
    HIPCHK(hipEventRecord(c->ev_sw1, s));
    HIPCHK(hipEventRecord(c->ev[3], s));
    HIPCHK(zh_launch_prefilter_exact(f, d, ix->X.as<float>(), c->dQ, c->wQQ.as<float>(), (uint32_t)B, c->metric, c->mode, ix->opt.id_base, pf,
                                     c->wPfKeys.as<uint64_t>(), c->wPfIds.as<uint64_t>(), s));
    HIPCHK(hipEventRecord(c->ev[4], s));
    HIPCHK(zh_launch_final_lists(T, (uint32_t)B, (uint32_t)k, cap, c->wPfKeys.as<uint64_t>(), c->wPfIds.as<uint64_t>(), c->wPfCounts.as<uint32_t>(),
                                 dOutIds, dOutKeys, dOutCounts, pf.ctl + 1, s));
    for (size_t j = 0; j < nwin && nwin > 1; j++) {
        HIPCHK(hipMemcpyAsync(outIds[j], dOutIds + j * bwin * k, bwin * k * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(outKeys[j], dOutKeys + j * bwin * k, bwin * k * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(outCounts[j], dOutCounts + j * bwin, bwin * 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(c->h_pf, c->wPfCtl.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(c->ev[5], s));
    c->state = 2;
    return ZH_OK;
}

// second half: waits (host side) for the totals only, sizes the scratch, enqueues emit -> sweep -> select -> final
static int ctx_finish(zh_search_ctx *c, uint64_t *const *outIds, uint64_t *const *outKeys, uint32_t *const *outCounts,
                      hipStream_t heavy) {
    zh_index *ix = c->ix;
    if (c->state != 1) return fail(ZH_ESTATE, "zh_search_finish without zh_search_begin");
    const uint32_t d = ix->opt.dim, T = ix->n_trees;
    const size_t B = c->B, k = c->k, nwin = c->nwin, bwin = c->bwin;
    hipStream_t s = c->s;
    int rc;
    c->state = 0;
    if (c->trivial) {
        for (size_t j = 0; j < nwin && bwin; j++) {
            HIPCHK(hipMemsetAsync(outCounts[j], 0, bwin * 4, s));
            if (k) {
                HIPCHK(hipMemsetAsync(outIds[j], 0xFF, bwin * k * 8, s));
                HIPCHK(hipMemsetAsync(outKeys[j], 0xFF, bwin * k * 8, s));
            }
        }
        HIPCHK(hipEventRecord(c->ev[5], s));
        c->state = 2;
        return ZH_OK;
    }
    // one batch: the final kernel writes straight into the caller's buffers; a window: into the context's own, handed out
    // per batch by small device copies afterwards
    uint64_t *dOutIds = outIds[0], *dOutKeys = outKeys[0];
    uint32_t *dOutCounts = outCounts[0];
    if (nwin > 1) {
        if ((rc = c->wOutWin.ensure(B * k * 16 + B * 4))) { return rc; }
        dOutIds = c->wOutWin.as<uint64_t>();
        dOutKeys = dOutIds + B * k;
        dOutCounts = reinterpret_cast<uint32_t *>(dOutKeys + B * k);
    }
    HIPCHK(hipEventSynchronize(c->ev_totals));
    const ZhTotals tot = c->tot = *c->h_totals;
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        const double v = (double)tot.visits / (double)((uint64_t)B * T);
        ix->visits_per_pair = ix->visits_per_pair > 0 ? 0.5 * (ix->visits_per_pair + v) : v;
    }
    if (tot.visits > 0xFFFFFFFull || tot.rows >= (1ull << 36))
        return fail(ZH_ELIMIT, "more than 2^28 leaf visits or 2^36 scored rows in one batch; use a smaller batch");
    c->sv_ids.assign(outIds, outIds + nwin); c->sv_keys.assign(outKeys, outKeys + nwin); c->sv_counts.assign(outCounts, outCounts + nwin);
    c->sv_heavy = heavy;
    if (c->prefilter && (tot.flags & 1u)) {
        // the visit log ran out (an index's first wandering batches): this batch again the classic way -- its emit walk needs the
        // per-leaf counts a prefiltered first half does not take -- and with a log that fits the next one
        const std::vector<const float *> q = c->sv_q;
        c->prefilter_off_once = true;
        rc = ctx_begin(c, q.data(), nwin, bwin, k, c->metric, c->mode, s);
        c->prefilter_off_once = false;
        if (rc) return rc;
        return ctx_finish(c, outIds, outKeys, outCounts, heavy);
    }
    if (c->prefilter) return finish_prefilter(c, dOutIds, dOutKeys, dOutCounts, outIds, outKeys, outCounts);
    if ((rc = c->wVisits.ensure(std::max<uint64_t>(tot.visits, 1) * sizeof(ZhVisit)))) return rc;
    if ((rc = c->wGroups.ensure(std::max<uint64_t>(tot.groups, 1) * sizeof(ZhGroup)))) return rc;
    if ((rc = c->wGroupRowOff.ensure(std::max<uint64_t>(tot.groups, 1) * 8))) return rc;
    if ((rc = c->wWaveGroup.ensure((tot.group_rows / 64 + 2) * 4))) return rc;
    if ((rc = c->wKeys.ensure(std::max<uint64_t>(tot.rows, 1) * 8))) return rc;
    if ((rc = c->wCandKeys.ensure(std::max<uint64_t>(tot.takes, 1) * 8))) return rc;
    if ((rc = c->wCandIds.ensure(std::max<uint64_t>(tot.takes, 1) * 4))) return rc;
    ZhForestDev f = forest_dev(ix);
    if (!(tot.flags & 1u)) {
        // the counting pass logged every visit: place them (no second walk)
        HIPCHK(zh_launch_expand(f, (uint32_t)B, c->wCounts.as<ZhPairCounts>(), c->wInline.as<ZhVisit>(),
                                c->wRowBase.as<uint64_t>(), c->wCandBase.as<uint64_t>(), c->wVisitBase.as<uint64_t>(),
                                c->wVisits.as<ZhVisit>(), c->wLeafCount.as<uint32_t>(), c->wLeafFill.as<uint32_t>(),
                                c->wGroupBase.as<uint32_t>(), c->wGroupRowBase.as<uint64_t>(), c->wGroups.as<ZhGroup>(),
                                c->wGroupRowOff.as<uint64_t>(), walk_log(c), s));
    } else {
        // the visit log ran out of chunks: walk again, emitting this time, and give the next batch a log that fits
        if (c->lazy_fix)  // the pointer walk reads plain sign bits: the flagged ones are recomputed first
            HIPCHK(zh_launch_score_unc_fix(c->dQ, (uint32_t)B, d, f.planes, f.consts, ix->n_planes, c->wBits.as<uint32_t>(), c->wUnc.as<uint32_t>(), c->wpq, s));
        HIPCHK(zh_launch_walk_emit(f, c->dQ, (uint32_t)B, d, (int32_t)k, c->wBits.as<uint32_t>(), c->wpq, c->P_dense,
                                   c->wCounts.as<ZhPairCounts>(), c->wInline.as<ZhVisit>(), c->wRowBase.as<uint64_t>(),
                                   c->wCandBase.as<uint64_t>(), c->wVisitBase.as<uint64_t>(), c->wVisits.as<ZhVisit>(),
                                   c->wLeafCount.as<uint32_t>(), c->wLeafFill.as<uint32_t>(), c->wGroupBase.as<uint32_t>(),
                                   c->wGroupRowBase.as<uint64_t>(), c->wGroups.as<ZhGroup>(), c->wGroupRowOff.as<uint64_t>(), s));
        const uint64_t pairs = (uint64_t)B * T;
        const uint64_t want = tot.visits / (ZH_LOG_CHUNK - 1) + std::min<uint64_t>(pairs, tot.visits / (ZH_INLINE_VISITS + 1)) + 16;
        static const bool fixed = getenv("ZH_WALK_LOG_FIXED") != nullptr;  // tests: keep the log small, always fall back
        if (!fixed && want > c->log_chunks) {
            const size_t chunks = (size_t)(want + want / 2);
            // the pool is idle: the counting pass has completed (its totals are here) and the emit walk does not use it
            if (c->wLogPool.ensure(chunks * ZH_LOG_CHUNK * sizeof(uint2)) == ZH_OK) c->log_chunks = chunks;
        }
    }
    c->scan = choose_scan(ix, tot, c->metric, B, k);
    if (c->scan && !ix->row_leaf.current(ix)) {  // first table scan since the trees (or the row count) changed
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if (!ix->row_leaf.current(ix) && !ix->row_leaf.failed && (rc = build_row_leaf(ix))) return rc;
        if (!ix->row_leaf.current(ix)) c->scan = false;
    }
    if (c->scan) {
        const size_t nn = std::max<uint32_t>(ix->n_nodes, 1);
        if ((rc = c->wVisitBits.ensure((nn + 31) / 32 * 4))) return rc;
        if ((rc = c->wNodeVisit.ensure(nn * sizeof(uint4)))) return rc;
        HIPCHK(zh_launch_node_visits(c->wLeafCount.as<uint32_t>(), c->wGroupBase.as<uint32_t>(), c->wGroups.as<ZhGroup>(), ix->n_nodes,
                                     c->wVisitBits.as<uint32_t>(), c->wNodeVisit.as<uint4>(), s));
    }
    if (!c->scan)
        HIPCHK(zh_launch_wave_groups(c->wGroups.as<ZhGroup>(), c->wGroupRowOff.as<uint64_t>(), tot.groups, c->wWaveGroup.as<uint32_t>(), s));
    c->approx = c->scan && use_approx(ix, tot, B, k, c->metric);
    c->approx_leaf = false; c->approx_bytes = false;
    if (!c->scan && use_approx_leaf(ix, tot, B, k, c->metric)) {
        bool ok = false;
        // rows of bytes (integers 0 .. 255: SIFT descriptors) are copied as bytes -- half the sweep's bytes, no rounding -- for the lean kernels;
        // ZH_S128H_BYTES=0 (read per batch: tests) keeps the copy of halves
        const char *be = getenv("ZH_S128H_BYTES"), *ke = getenv("ZH_S128H_KERNEL"), *de = getenv("ZH_S128H_DMA");
        const bool want_bytes = !(be && be[0] == '0') && !(ke && ke[0] == 'r') && !(de && de[0] == '1');
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if ((rc = ensure_row_half128(ix, &ok, want_bytes))) return rc;
        c->approx = c->approx_leaf = ok;
        c->approx_bytes = ok && ix->half128.bytes;
    }
    ZhApprox ap{};
    // the scan on the matrix cores, from an fp16 copy of the stored rows (+50 % of the row table, made on first use); no room for it, or mode 5:
    // the VALU kernel on the f32 rows
    bool mfma = c->approx && !c->approx_leaf && mfma_wanted(ix) && B < (1u << 23) - 1;  // (the column pass packs query + 1 into 23 bits of an LDS word)
    const uint2 *scan_row_leaf = ix->row_leaf.table.as<uint2>();
    if (mfma) {
        std::lock_guard<std::mutex> lk(ix->blk_mu);
        if ((rc = ensure_row_half(ix, &mfma))) return rc;
        if (mfma && ix->order.rows) {
            if ((rc = ensure_row_leaf_p(ix))) return rc;
            if (!ix->order.rows) {  // no room for the table in the scan's order: the copy again, in id order, and no further attempt
                ix->order.switch_off();
                ix->half.remake();
                if ((rc = ensure_row_half(ix, &mfma))) return rc;
            } else
                scan_row_leaf = ix->order.row_leaf_p.as<uint2>();
        }
    }
    c->approx_mfma = mfma;
    c->approx_f32rows = mfma && ix->half.tiles.p == nullptr;
    if (c->approx) {
        // per query: what final_interval_kernel's sort holds (48 KB per query of HBM).  A visit hands on the rows its intervals cannot
        // rule out: a few more than `take` -- or dozens more where the keys are dense around the cut: the parity cosine key on iid
        // rows, whose "nearest" are the similarities just above zero, sends ~100 rows per visit of a 20k-row leaf.  The exact path
        // for visits that take fewer than top_k rows: its table and key scratch sized from the batch
        const char *cap_e = getenv("ZH_APX_CAPS");  // tests: "capq,ex_cap,ex_rows" -- lists and tables that run over (read per batch)
        unsigned e_capq = 0, e_excap = 0, e_exrows = 0;
        if (cap_e) sscanf(cap_e, "%u,%u,%u", &e_capq, &e_excap, &e_exrows);
        const uint32_t capq = e_capq ? std::min(e_capq, 8192u) : (ix->fb.approx_strikes.load() ? 8192u : 4096u);
        const uint32_t ex_cap = e_excap ? e_excap : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096, tot.visits / 4 + 1024), 1u << 24);
        const uint32_t ex_rows = e_exrows ? e_exrows : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, tot.rows / 16), 1u << 26);
        if ((rc = c->wQh.ensure(B * d * 2)) || (rc = c->wQmeta.ensure(B * sizeof(float4))) || (rc = c->wApList.ensure((size_t)B * capq * 12)) ||
            (rc = c->wApCount.ensure(B * 8 + std::max<uint64_t>(tot.visits, 1) * 4)) || (rc = c->wApEx.ensure((size_t)ex_cap * 8)) || (rc = c->wApExKeys.ensure((size_t)ex_rows * 20)) ||
            (rc = c->wApCtl.ensure(ZH_APX_CTL_WORDS * 4)))
            return rc;
        ap.Qh = c->wQh.p; ap.qmeta = c->wQmeta.as<float4>(); ap.iv = c->wKeys.as<uint64_t>();
        ap.list_lo = c->wApList.as<uint32_t>(); ap.list_hi = ap.list_lo + (size_t)B * capq; ap.list_id = ap.list_hi + (size_t)B * capq;
        ap.qcount = c->wApCount.as<uint32_t>(); ap.capq = capq; ap.qtau = ap.qcount + B; ap.tauv = ap.qtau + B;
        ap.ex_visits = c->wApEx.as<uint2>(); ap.ex_cap = ex_cap;
        ap.ex_keys = c->wApExKeys.as<uint64_t>(); ap.ex_ckeys = ap.ex_keys + ex_rows; ap.ex_cids = reinterpret_cast<uint32_t *>(ap.ex_ckeys + ex_rows);
        ap.ex_rows_cap = ex_rows; ap.ctl = c->wApCtl.as<uint32_t>();
        ap.n_queries = (uint32_t)B; ap.iv_cap = tot.rows;
        ap.mfma = mfma ? 1u : 0u; ap.row_half = mfma ? ix->half.tiles.p : nullptr; ap.row_meta = mfma ? ix->half.meta.as<float2>() : nullptr;  // (row_half null with mfma: the scan converts the f32 rows itself)
        ap.row_rho = mfma ? ix->half.rho.load() : 0.f;
        if (c->approx_leaf) { ap.mfma = 2u; ap.row_rho = ap.rho_norm = c->approx_bytes ? 0.f : ix->half128.rho.load(); }
        // (a row of bytes: |x|^2 <= 128 * 255^2 exactly, approx_interval's nx = sqrtf of it * (1 + 1e-5) < 2885.1; ZH_S128H_PRETEST=0, read per batch: tests)
        const char *pte = getenv("ZH_S128H_PRETEST");
        ap.nx_max = c->approx_leaf && c->approx_bytes && !(pte && pte[0] == '0') ? 2885.1f : 0.f;
        HIPCHK(hipMemsetAsync(c->wApCount.p, 0, B * 4, s));
        HIPCHK(hipMemsetAsync(ap.qtau, 0xFF, B * 4, s));
        HIPCHK(hipMemsetAsync(c->wApCtl.p, 0, ZH_APX_CTL_WORDS * 4, s));
        HIPCHK(zh_launch_qhalf(c->dQ, (uint32_t)B, d, c->wQh.p, c->wQmeta.as<float4>(), c->approx_leaf ? 2 : (mfma ? 1 : 0), s));
    }
    HIPCHK(hipEventRecord(c->ev[2], s));
    // the HBM-bound sweep may run on a different ("heavy") stream shared by all contexts, so that sweeps of
    // successive batches execute back to back while everything else overlaps them on the contexts' own streams
    hipStream_t hs = heavy ? heavy : s;
    if (hs != s) { HIPCHK(hipEventRecord(c->ev_emit, s)); HIPCHK(hipStreamWaitEvent(hs, c->ev_emit, 0)); }
    HIPCHK(hipEventRecord(c->ev_sw0, hs));
    // d = 128 leaf by leaf at half width: FUSED (intervals, bounds and the queries' lists inside the sweep: no raw pairs, no select pass) when the
    // leaves are long -- a bound is derived per 64-row chunk that lies inside one leaf group, and the lists must hold what the first waves of a visit
    // hand on before any bound has spread -- and top_k fits a chunk.  ZH_S128H_FUSED=0 / 1 (read per batch: tests) forbids / forces it;
    // zh_debug_keep_raw wants the raw pairs
    c->approx_fused = false;
    if (c->approx_leaf && k <= 64 && !ix->debug_keep_raw) {
        const char *fe = getenv("ZH_S128H_FUSED"), *ke = getenv("ZH_S128H_KERNEL"), *de = getenv("ZH_S128H_DMA");
        const bool lean = !(ke && ke[0] == 'r') && !(de && de[0] == '1');
        c->approx_fused = lean && (fe ? fe[0] == '1' : (!ix->fb.fused_off && tot.rows >= 1024 * std::max<uint64_t>(tot.visits, 1)));
    }
    const int kinda = c->metric != ZH_COSINE ? 0 : (c->mode == ZH_COSINE_PARITY ? 2 : 1);
    if (c->approx_leaf)
        HIPCHK(zh_launch_sweep128h(ix->half128.copy.p, c->wQh.p, ldexpf(1.f, ix->half128.ex - 14), c->wGroups.as<ZhGroup>(), c->wGroupRowOff.as<uint64_t>(),
                                   tot.groups, c->wWaveGroup.as<uint32_t>(), f.leaf_ids, tot.group_rows, c->wKeys.as<uint64_t>(), hs,
                                   c->approx_fused ? &ap : nullptr, kinda, (uint32_t)k, zh_approx_bound(c->metric, d, 2), c->approx_bytes));
    else if (c->approx)
        HIPCHK(zh_launch_scan_approx(ix->X.as<float>(), d, ix->n_rows, ap, mfma ? scan_row_leaf : ix->row_leaf.table.as<uint2>(), T, c->wVisitBits.as<uint32_t>(),
                                     c->wNodeVisit.as<uint4>(), c->wGroups.as<ZhGroup>(), f.group, c->metric, c->mode, hs));
    else if (c->scan)
        HIPCHK(zh_launch_scan_sweep(ix->X.as<float>(), d, ix->n_rows, c->dQ, c->wQQ.as<float>(), ix->row_leaf.table.as<uint2>(), T,
                                    c->wVisitBits.as<uint32_t>(), c->wNodeVisit.as<uint4>(), c->wGroups.as<ZhGroup>(), f.group,
                                    c->metric, c->mode, c->wKeys.as<uint64_t>(), nullptr, hs));
    else
        HIPCHK(zh_launch_sweep(ix->X.as<float>(), d, c->dQ, c->wQQ.as<float>(), c->wGroups.as<ZhGroup>(),
                               c->wGroupRowOff.as<uint64_t>(), tot.groups, c->wWaveGroup.as<uint32_t>(), f.leaf_ids,
                               tot.group_rows, c->metric, c->mode, c->wKeys.as<uint64_t>(), hs));
    HIPCHK(hipEventRecord(c->ev_sw1, hs));
    if (hs != s) HIPCHK(hipStreamWaitEvent(s, c->ev_sw1, 0));
    HIPCHK(hipEventRecord(c->ev[3], s));
    const uint32_t *run_if = nullptr;
    c->dbg_valid = c->approx;
    c->dbg_raw = false;
    if (c->approx) {
        c->dbg_ap = ap;
        if (ix->debug_keep_raw && tot.rows) {  // tests: the scan's raw pairs, before select_tau_kernel turns them into intervals in place
            if ((rc = c->wRaw.ensure(tot.rows * 8))) return rc;
            HIPCHK(hipMemcpyAsync(c->wRaw.p, c->wKeys.p, tot.rows * 8, hipMemcpyDeviceToDevice, s));
            c->dbg_raw = true;
        }
        if (c->approx_fused) HIPCHK(zh_launch_exact_register(c->wVisits.as<ZhVisit>(), tot.visits, (uint32_t)k, ap, s));
        else HIPCHK(zh_launch_select_interval(c->wVisits.as<ZhVisit>(), tot.visits, (uint32_t)k, f.leaf_ids, ap, c->metric, c->mode, d, s));
        HIPCHK(hipEventRecord(c->ev[4], s));
        HIPCHK(zh_launch_final_interval(c->wVisits.as<ZhVisit>(), ix->X.as<float>(), d, c->dQ, c->wQQ.as<float>(), (uint32_t)B, (uint32_t)k,
                                        f.leaf_ids, c->metric, c->mode, ix->opt.id_base, ap, dOutIds, dOutKeys, dOutCounts, ix->max_leaf_len, s));
        HIPCHK(hipMemcpyAsync(c->h_ap, c->wApCtl.p, ZH_APX_CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
        // A list or table ran over (ctl[1] != 0): the f32 scan, select and final, enqueued here with that word as their predicate,
        // redo the batch in stream order -- kernels that return at once otherwise.  On the context's own stream: the shared sweep
        // stream must not wait for this batch's light kernels.
        run_if = ap.ctl + 1;
        if (c->approx_leaf)
            HIPCHK(zh_launch_sweep(ix->X.as<float>(), d, c->dQ, c->wQQ.as<float>(), c->wGroups.as<ZhGroup>(), c->wGroupRowOff.as<uint64_t>(), tot.groups,
                                   c->wWaveGroup.as<uint32_t>(), f.leaf_ids, tot.group_rows, c->metric, c->mode, c->wKeys.as<uint64_t>(), s, run_if));
        else
            HIPCHK(zh_launch_scan_sweep(ix->X.as<float>(), d, ix->n_rows, c->dQ, c->wQQ.as<float>(), ix->row_leaf.table.as<uint2>(), T,
                                        c->wVisitBits.as<uint32_t>(), c->wNodeVisit.as<uint4>(), c->wGroups.as<ZhGroup>(), f.group,
                                        c->metric, c->mode, c->wKeys.as<uint64_t>(), run_if, s));
    }
    HIPCHK(zh_launch_select(c->wVisits.as<ZhVisit>(), tot.visits, f.leaf_ids, c->wKeys.as<uint64_t>(),
                            c->wCandKeys.as<uint64_t>(), c->wCandIds.as<uint32_t>(), ix->max_leaf_len, run_if, s));
    if (!c->approx) HIPCHK(hipEventRecord(c->ev[4], s));
    HIPCHK(zh_launch_final(c->wCandBase.as<uint64_t>(), (uint32_t)B, T, (uint32_t)k, c->wCandKeys.as<uint64_t>(),
                           c->wCandIds.as<uint32_t>(), ix->opt.id_base, dOutIds, dOutKeys, dOutCounts, run_if, s));
    for (size_t j = 0; j < nwin && nwin > 1; j++) {
        HIPCHK(hipMemcpyAsync(outIds[j], dOutIds + j * bwin * k, bwin * k * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(outKeys[j], dOutKeys + j * bwin * k, bwin * k * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(outCounts[j], dOutCounts + j * bwin, bwin * 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipEventRecord(c->ev[5], s));
    c->state = 2;
    return ZH_OK;
}

// block until the batch's results are complete; fold its counters and stage timings into the index's stats
int ctx_wait(zh_search_ctx *c) {
    zh_index *ix = c->ix;
    if (c->state == 1) return fail(ZH_ESTATE, "zh_search_wait: the batch was begun but not finished");
    if (c->state != 2) return ZH_OK;
    c->state = 0;
    HIPCHK(hipEventSynchronize(c->ev[5]));
    if (c->trivial) return ZH_OK;
    const bool pf = c->prefilter;
    const uint32_t pf_amb = pf ? c->h_pf[0] : 0, pf_flags = pf ? c->h_pf[1] : 0, pf_exact = pf ? c->h_pf[2] : 0;
    if (pf_flags) {  // a candidate list (or the ambiguous-visit table) ran over: this batch again, swept the classic way
        {
            std::lock_guard<std::mutex> lk(ix->stats_mu);
            ix->stats.prefilter_fallbacks_accum++;
            ix->stats.prefilter_last_overflow = pf_flags;
        }
        ix->fb.prefilter_ran_over();
        const std::vector<const float *> q = c->sv_q;
        const std::vector<uint64_t *> ids = c->sv_ids, keys = c->sv_keys;
        const std::vector<uint32_t *> counts = c->sv_counts;
        c->prefilter_off_once = true;
        int rc = ctx_begin(c, q.data(), c->nwin, c->bwin, c->k, c->metric, c->mode, c->s);
        if (!rc) rc = ctx_finish(c, ids.data(), keys.data(), counts.data(), c->sv_heavy);
        c->prefilter_off_once = false;
        if (rc) return rc;
        return ctx_wait(c);
    }
    if (pf) ix->fb.prefilter_held();
    const ZhTotals tot = c->tot;
    uint64_t uniq = 0;
    if (ix->profiling >= 2 && tot.visits && !pf) {  // R_unique: rows of the distinct leaves touched by the batch
        std::vector<ZhVisit> hv(tot.visits);
        HIPCHK(hipMemcpy(hv.data(), c->wVisits.p, tot.visits * sizeof(ZhVisit), hipMemcpyDeviceToHost));
        std::vector<std::pair<uint32_t, uint32_t>> leaves(hv.size());
        for (size_t i = 0; i < hv.size(); i++) leaves[i] = {hv[i].leaf_off, hv[i].len};
        std::sort(leaves.begin(), leaves.end());
        leaves.erase(std::unique(leaves.begin(), leaves.end()), leaves.end());
        for (auto &l : leaves) uniq += l.second;
    }
    float ms[5] = {0, 0, 0, 0, 0};
    if (ix->profiling > 0) {
        for (int i = 0; i < 5; i++) HIPCHK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
        HIPCHK(hipEventElapsedTime(&ms[2], c->ev_sw0, c->ev_sw1));  // the sweep kernel alone, on the stream it ran on
    }
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    zh_stats_t &st = ix->stats;
    st.batch = c->B; st.window_batches = c->nwin; st.visits = tot.visits; st.rows_scored = tot.rows; st.candidates = tot.takes;
    st.planes_dense = c->P_dense; st.planes_total = ix->n_planes;
    const uint64_t swept = pf ? pf_exact : (c->scan ? ix->n_rows : tot.group_rows);
    st.rows_swept = swept;
    st.sweep_bytes = pf ? tot.rows * 64 + (uint64_t)pf_exact * 4 * ix->opt.dim  // one 64-byte sector of the score table per scored row
                        : (c->scan ? ix->n_rows * ((uint64_t)4 * ix->opt.dim + 8 * ix->n_trees) + tot.rows * 8
                                   : tot.group_rows * ((uint64_t)4 * ix->opt.dim + 4) + tot.rows * 8);
    st.table_scan = c->scan && !pf ? 1 : 0;
    const bool apx = c->approx && !pf;
    st.approx_scan = apx ? (c->approx_leaf ? 3 : (c->approx_mfma ? 2 : 1)) : 0;
    st.approx_fused = apx && c->approx_leaf && c->approx_fused ? 1 : 0;
    st.approx_byte_rows = apx && c->approx_leaf && c->approx_bytes ? 1 : 0;
    st.approx_exact_visits = apx ? c->h_ap[0] : 0;
    st.approx_survivors = apx ? c->h_ap[3] : 0;
    st.approx_list_entries = apx ? c->h_ap[4] : 0;
    if (apx && c->h_ap[7]) fprintf(stderr, "zebra_hip: scan guard tripped, bits %u (diagnostic build)\n", c->h_ap[7]);
    st.approx_columns = apx && c->approx_mfma ? c->h_ap[5] : 0;
    st.approx_column_pairs = apx && c->approx_mfma ? c->h_ap[6] : 0;
    if (apx && c->h_ap[1]) {
        st.approx_fallbacks_accum++;
        st.approx_last_overflow = c->h_ap[1];
        ix->fb.approx_ran_over(c->approx_mfma && c->approx_f32rows, c->approx_leaf && c->approx_fused);
    } else if (apx && (uint64_t)c->h_ap[4] > (uint64_t)c->B * (ix->fb.approx_strikes.load() ? 5600 : 2800))  // lists 70 % full on average: some query's will run over
        ix->fb.approx_nearly_ran_over();
    st.prefiltered = pf ? 1 : 0;
    st.prefilter_exact_visits = pf_amb;
    st.prefilter_exact_rows = pf_exact;
    st.hash_from_scores = c->score_hash ? 1 : 0;
    st.hash_exact_fixups = c->score_hash ? tot.hash_fixups : 0;
    if (ix->profiling >= 2) st.rows_unique = uniq;
    if (ix->profiling > 0) {
        st.ms_hash += ms[0]; st.ms_walk += ms[1]; st.ms_sweep += ms[2]; st.ms_select += ms[3]; st.ms_final += ms[4];
        st.ms_total += ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
        st.timed_batches++;
        st.sweep_rows_accum += tot.rows;
        st.swept_rows_accum += swept;
        // (the half-width d = 128 sweep's lean kernels take two or four times the rows per launch: 256- or 128-byte rows -- launch_sweep128h_lean)
        const char *ke = getenv("ZH_S128H_KERNEL"), *de = getenv("ZH_S128H_DMA");
        const bool lean128 = apx && c->approx_leaf && !(ke && ke[0] == 'r') && !(de && de[0] == '1');
        const uint64_t rpl = apx && c->approx_leaf ? zh_sweep128h_rows_per_launch(lean128, c->approx_bytes) : zh_sweep_rows_per_launch(ix->opt.dim);
        st.sweep_launches_accum += (swept + rpl - 1) / rpl;
        st.scan_batches_accum += c->scan && !pf ? 1 : 0;
        st.approx_batches_accum += apx ? 1 : 0;
    }
    return ZH_OK;
}

static int search_once(zh_index *ix, const float *dQ, size_t B, size_t k, int metric, int mode, uint64_t *dOutIds,
                       uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s, zh_search_ctx *c) {
    int rc = ctx_begin(c, &dQ, 1, B, k, metric, mode, s);
    if (rc) return rc;
    if ((rc = ctx_finish(c, &dOutIds, &dOutKeys, &dOutCounts, nullptr))) return rc;
    return ctx_wait(c);
}

// The blocking entry points take any batch: a batch that would pass a per-launch limit (batch * num_trees < 2^26 pairs,
// <= 2^28 - 1 leaf visits, < 2^36 scored rows -- reached by a few thousand queries under the reference's default options,
// where a query visits ~10^4..10^5 leaves) is split into sub-batches whose outputs land side by side.  The
// first split is sized from the visits per pair seen so far; a sub-batch that still overflows is halved and retried.
static int search_locked(zh_index *ix, const float *dQ, size_t B, size_t k, int metric, int mode, uint64_t *dOutIds,
                         uint64_t *dOutKeys, uint32_t *dOutCounts, hipStream_t s, zh_search_ctx *c = nullptr) {
    if (!c) c = &ix->dctx;
    const uint32_t T = ix->n_trees, d = ix->opt.dim;
    if (B == 0 || T == 0) return search_once(ix, dQ, B, k, metric, mode, dOutIds, dOutKeys, dOutCounts, s, c);
    size_t chunk = std::min<size_t>(B, ((1ull << 26) - 1) / T);
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        if (ix->visits_per_pair > 0) {
            const double per_query = ix->visits_per_pair * T;
            chunk = std::min<size_t>(chunk, (size_t)std::max(1.0, (double)(1ull << 27) / per_query));  // half the cap: headroom
        }
    }
    if (chunk == 0) chunk = 1;
    for (size_t b0 = 0; b0 < B;) {
        const size_t nb = std::min(chunk, B - b0);
        const int rc = search_once(ix, dQ + b0 * d, nb, k, metric, mode, dOutIds + b0 * k, dOutKeys + b0 * k, dOutCounts + b0, s, c);
        if (rc == ZH_ELIMIT && nb > 1) { chunk = (nb + 1) / 2; continue; }  // the context is idle again: retry smaller
        if (rc) return rc;
        b0 += nb;
    }
    return ZH_OK;
}

static int check_metric(int metric, int mode) {
    if (metric < ZH_COSINE || metric > ZH_PNORM) return fail(ZH_EINVAL, "unknown metric %d", metric);
    if (metric == ZH_COSINE && mode != ZH_COSINE_PARITY && mode != ZH_COSINE_CORRECTED) return fail(ZH_EINVAL, "unknown cosine mode %d", mode);
    // ZH_MINKOWSKI / ZH_PNORM: `mode` is the struct's i32 power and every value is legal (distance.rs:160-190; Default = 0)
    return ZH_OK;
}

extern "C" int zh_search_batch_device(zh_index *ix, const float *d_q, size_t b, size_t k, int metric, int mode,
                                      uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    if (!ix || (b && (!d_q || !d_out_counts || (k && (!d_out_ids || !d_out_keys))))) return fail(ZH_EINVAL, "zh_search_batch_device: null argument");
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k %zu > ZH_MAX_TOPK (%u)", k, ZH_MAX_TOPK);
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if ((rc = set_device(ix))) return rc;
    return search_locked(ix, d_q, b, k, metric, mode, d_out_ids, d_out_keys, d_out_counts,
                         stream ? (hipStream_t)stream : ix->stream);
}

// ---- pipelined form: several batches in flight, each on its own context and stream ----------------------
extern "C" int zh_search_ctx_create(zh_index *ix, zh_search_ctx **out) {
    if (!ix || !out) return fail(ZH_EINVAL, "zh_search_ctx_create: null argument");
    int rc = set_device(ix);
    if (rc) return rc;
    zh_search_ctx *c = new (std::nothrow) zh_search_ctx();
    if (!c) return fail(ZH_ENOMEM, "out of host memory");
    if ((rc = ctx_init(c, ix))) { c->release_all(); delete c; return rc; }
    *out = c;
    return ZH_OK;
}
extern "C" void zh_search_ctx_destroy(zh_search_ctx *c) {
    if (!c) return;
    hipSetDevice(c->ix->device);
    if (c->state == 2) hipEventSynchronize(c->ev[5]);
    else if (c->state == 1 && c->s) hipStreamSynchronize(c->s);
    c->release_all();
    delete c;
}
extern "C" int zh_search_begin(zh_search_ctx *c, const float *d_q, size_t b, size_t k, int metric, int mode, void *stream) {
    if (!c || (b && !d_q)) return fail(ZH_EINVAL, "zh_search_begin: null argument");
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k %zu > ZH_MAX_TOPK (%u)", k, ZH_MAX_TOPK);
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    if ((rc = set_device(c->ix))) return rc;
    return ctx_begin(c, &d_q, 1, b, k, metric, mode, stream ? (hipStream_t)stream : c->ix->stream);
}
extern "C" int zh_search_begin_window(zh_search_ctx *c, const float *const *d_q, size_t n_batches, size_t b, size_t k, int metric,
                                      int mode, void *stream) {
    if (!c || !d_q || n_batches == 0 || n_batches > ZH_MAX_WINDOW) return fail(ZH_EINVAL, "zh_search_begin_window: bad argument (1..%u batches)", ZH_MAX_WINDOW);
    for (size_t j = 0; j < n_batches; j++)
        if (b && !d_q[j]) return fail(ZH_EINVAL, "zh_search_begin_window: null query pointer");
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k %zu > ZH_MAX_TOPK (%u)", k, ZH_MAX_TOPK);
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    if ((rc = set_device(c->ix))) return rc;
    return ctx_begin(c, d_q, n_batches, b, k, metric, mode, stream ? (hipStream_t)stream : c->ix->stream);
}
extern "C" int zh_search_finish(zh_search_ctx *c, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                void *sweep_stream) {
    if (!c) return fail(ZH_EINVAL, "zh_search_finish: null context");
    if (c->B && (!d_out_counts || (c->k && (!d_out_ids || !d_out_keys)))) return fail(ZH_EINVAL, "zh_search_finish: null output");
    if (c->nwin != 1) return fail(ZH_ESTATE, "zh_search_finish: the context holds a window; use zh_search_finish_window");
    int rc = set_device(c->ix);
    if (rc) return rc;
    return ctx_finish(c, &d_out_ids, &d_out_keys, &d_out_counts, (hipStream_t)sweep_stream);
}
extern "C" int zh_search_finish_window(zh_search_ctx *c, uint64_t *const *d_out_ids, uint64_t *const *d_out_keys,
                                       uint32_t *const *d_out_counts, void *sweep_stream) {
    if (!c || !d_out_ids || !d_out_keys || !d_out_counts) return fail(ZH_EINVAL, "zh_search_finish_window: null argument");
    for (size_t j = 0; j < c->nwin && c->bwin; j++)
        if (!d_out_counts[j] || (c->k && (!d_out_ids[j] || !d_out_keys[j]))) return fail(ZH_EINVAL, "zh_search_finish_window: null output");
    int rc = set_device(c->ix);
    if (rc) return rc;
    return ctx_finish(c, d_out_ids, d_out_keys, d_out_counts, (hipStream_t)sweep_stream);
}
double zh_index_visits_per_pair(zh_index *ix) {
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    return ix->visits_per_pair;
}
void zh_search_ctx_stream_ordered(zh_search_ctx *c) {
    if (c) c->stream_ordered = true;
}
void zh_search_ctx_abandon(zh_search_ctx *c) {
    if (c && c->state == 1) c->state = 0;  // what was enqueued by begin completes on its stream; its results are never used
}
extern "C" int zh_search_wait(zh_search_ctx *c) {
    if (!c) return fail(ZH_EINVAL, "zh_search_wait: null context");
    int rc = set_device(c->ix);
    if (rc) return rc;
    return ctx_wait(c);
}

// ---- test / debug access (include/zebra_hip.h, "test / debug access") ----
extern "C" int zh_trim_device_memory(void) {
    return ZH_OK;  // (the library caches no device memory: every buffer goes back to the driver when it is freed)
}

extern "C" int zh_debug_keep_raw(zh_index *ix, int on) {
    if (!ix) return fail(ZH_EINVAL, "zh_debug_keep_raw: null index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->debug_keep_raw = on != 0;
    return ZH_OK;
}
extern "C" int zh_debug_scan_pairs(zh_index *ix, zh_search_ctx *ctx, zh_debug_scan_info *info, zh_debug_pair *out, size_t cap, float *qmeta) {
    if (!ix || !info || (cap && !out)) return fail(ZH_EINVAL, "zh_debug_scan_pairs: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu, std::defer_lock);
    if (!ctx) lk.lock();
    zh_search_ctx *c = ctx ? ctx : &ix->dctx;
    if (c->ix != ix) return fail(ZH_EINVAL, "zh_debug_scan_pairs: the context belongs to another index");
    if (c->state != 0) return fail(ZH_ESTATE, "zh_debug_scan_pairs: the context has a batch in flight");
    int rc = set_device(ix);
    if (rc) return rc;
    memset(info, 0, sizeof(*info));
    if (!c->dbg_valid) return ZH_OK;  // (approx_scan 0: the last batch was not a half-width one)
    if (c->approx_leaf && c->approx_fused)  // (a fused sweep leaves no interval per pair anywhere: zh_debug_keep_raw keeps the sweep unfused)
        return fail(ZH_ESTATE, "zh_debug_scan_pairs: the batch's sweep was fused (no per-pair results exist); call zh_debug_keep_raw(idx, 1) first");
    const ZhTotals tot = c->tot;
    const ZhApprox &ap = c->dbg_ap;
    info->approx_scan = c->approx_leaf ? 3 : (c->approx_mfma ? 2 : 1);
    info->queries = (uint32_t)c->B; info->top_k = (uint32_t)c->k; info->metric = c->metric; info->cosine_mode = c->mode;
    info->raw_kept = c->dbg_raw ? 1 : 0; info->overflow = c->h_ap[1];
    info->bound_const = zh_approx_bound(c->metric, ix->opt.dim, (int)ap.mfma);
    info->row_rho = ap.row_rho; info->rho_norm = ap.rho_norm;
    info->pairs = tot.rows; info->visits = tot.visits;
    HIPCHK(hipDeviceSynchronize());
    if (qmeta) HIPCHK(hipMemcpy(qmeta, ap.qmeta, c->B * sizeof(float4), hipMemcpyDeviceToHost));
    if (!cap) return ZH_OK;
    if (cap < tot.rows) return fail(ZH_ELIMIT, "zh_debug_scan_pairs: %llu pairs, room for %zu", (unsigned long long)tot.rows, cap);
    std::vector<ZhVisit> hv(tot.visits);
    std::vector<uint64_t> iv(tot.rows), raw(c->dbg_raw ? tot.rows : 0);
    std::vector<uint32_t> lids(ix->n_leaf_ids);
    if (tot.visits) HIPCHK(hipMemcpy(hv.data(), c->wVisits.p, tot.visits * sizeof(ZhVisit), hipMemcpyDeviceToHost));
    if (tot.rows) HIPCHK(hipMemcpy(iv.data(), c->wKeys.p, tot.rows * 8, hipMemcpyDeviceToHost));
    if (c->dbg_raw && tot.rows) HIPCHK(hipMemcpy(raw.data(), c->wRaw.p, tot.rows * 8, hipMemcpyDeviceToHost));
    if (ix->n_leaf_ids) HIPCHK(hipMemcpy(lids.data(), ix->leaf_ids.p, ix->n_leaf_ids * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tot.rows; i++) { out[i].row = out[i].query = 0xFFFFFFFFu; out[i].flags = 0; out[i].visit = 0xFFFFFFFFu; }
    for (size_t v = 0; v < hv.size(); v++) {
        const ZhVisit &z = hv[v];
        if (z.row_off + z.len > tot.rows || (uint64_t)z.leaf_off + z.len > ix->n_leaf_ids) return fail(ZH_ESTATE, "zh_debug_scan_pairs: visit %zu out of range", v);
        const uint32_t fl = (z.take ? 1u : 0u) | ((z.take && z.take < z.len && z.take < c->k) ? 2u : 0u);
        for (uint32_t i = 0; i < z.len; i++) {
            zh_debug_pair &o = out[z.row_off + i];
            o.row = lids[(size_t)z.leaf_off + i]; o.query = z.b; o.visit = (uint32_t)v; o.flags = fl;
            const uint64_t w = iv[z.row_off + i];
            o.lo = (uint32_t)w; o.hi = (uint32_t)(w >> 32);
            o.raw_s = o.raw_a2 = 0.f;
            if (c->dbg_raw) { const uint64_t r = raw[z.row_off + i]; uint32_t a = (uint32_t)r, b2 = (uint32_t)(r >> 32); memcpy(&o.raw_s, &a, 4); memcpy(&o.raw_a2, &b2, 4); }
        }
    }
    return ZH_OK;
}

// ---- a large HOST-resident batch (zh_search_batch; Database::query_vectors -> the shim's search_batch, core.rs:290-313): windows over two contexts ----
// The device-pointer context API keeps two windows in flight (bench.py's loop: one sweeping, the next in its light phases, the copies beside both);
// a blocking host-pointer call used to run H2D -> one internal batch -> D2H back to back (132 k against 185-192 k QPS at
// cfg3).  Here the call cuts its batch into windows of `wq` queries (the size at which the half-width scan's query halves still fit the L2s beside
// the streamed rows), alternates them between the lane's two contexts -- light kernels on the contexts' own high-priority streams, the sweeps back
// to back on the index's sweep stream -- stages queries and results through pinned memory window by window, and hands out results as windows
// complete.  Same ids / keys / counts as one batch: the queries of a batch never interact.  Only in the few-visits-per-pair regime (long leaves):
// the wandering walk of small-leaf forests has its own limits per internal batch (search_locked splits by visits) and stays on the classic path.
// Queries per window of a large host batch.  Few visits per (query, tree) pair (leaves >= top_k): what keeps the scan's query halves in the L2s, by
// dimension.  The wandering walk of small-leaf forests (the reference's default options: thousands of visits per pair): what keeps the row-score
// hash's score table (n_rows x window x 4 bytes per context) at 1 GiB -- 256 queries at 1M rows; the classic path's own split there is by the visit
// log alone (~2000 queries: a 7.8-GB score table per chunk, one chunk at a time: 7 k QPS where windows over two contexts reach the pipelined rate).
static size_t host_window_queries(const zh_index *ix, bool wander) {
    const char *e = getenv("ZH_HOST_WINDOW");  // tests / A-B, read per call (unset or 0: by regime and dimension)
    const size_t forced = e ? (size_t)atoll(e) : (size_t)0;
    if (forced) return forced;
    const uint32_t d = ix->opt.dim;
    if (wander) {
        const size_t w = ((size_t)1 << 28) / std::max<uint64_t>(ix->n_rows, 1) / 64 * 64;
        return std::min<size_t>(std::max<size_t>(w, 64), 1024);
    }
    return d >= 512 ? 2048 : (d >= 256 ? 1024 : 4096);
}
// the window size for this call, or 0: the classic path (one internal batch, split only by its own limits)
static size_t host_windows_wanted(zh_index *ix, size_t B, size_t k, bool *wander) {
    const bool off = getenv("ZH_NO_HOST_WINDOWS") != nullptr;  // (read per call: tests switch it)
    if (off || ix->n_trees == 0 || ix->n_rows == 0) return 0;
    double vpp;
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        vpp = ix->visits_per_pair;  // (known from earlier batches)
    }
    // the first batch of an index: leaves below top_k wander (the guess choose_dense_planes makes too: lsh.rs:131-138's defaults against any
    // top_k >= 2) -- windows at once, the one-chunk classic path is four times slower there; otherwise the classic way, once
    if (!(vpp > 0)) {
        if ((size_t)ix->opt.max_node_size >= 2 * k + 2) return 0;
        vpp = 1000.0;
    }
    const size_t wq = host_window_queries(ix, vpp > 4.0);
    if (B < 2 * wq && B < wq + wq / 2) return 0;
    *wander = vpp > 4.0;
    return wq;
}
// returns ZH_OK with every result in the caller's buffers, or an error after which BOTH contexts are idle and nothing is in flight (the caller
// then runs the classic path: a window that passes a per-batch limit is not an error of the call)
#ifndef ZH_HOST_AHEAD_WANDER
#define ZH_HOST_AHEAD_WANDER 2   // windows begun ahead in the wandering regime (profiles/r06_host_calls_refdefault.txt: 1M x 384, default options, queries per
                                 // second at 1024 / 4096 / 8192 queries per call: none 17.2 / 17.4 / 17.4 k, one 23.1 / 25.1 / 25.5 k, two 23.7 / 28.4 / 29.1 k)
#endif
static int search_host_windows(zh_index *ix, zh_index::Lane &ln, size_t wq, int ahead, const float *q, size_t B, size_t k, int metric, int mode, uint64_t *out_ids,
                               uint64_t *out_keys, uint32_t *out_counts) {
    const uint32_t d = ix->opt.dim;
    int rc;
    auto init_ctx = [&](zh_search_ctx *c, hipStream_t *st, bool *flag) -> int {
        if (*flag) return ZH_OK;
        int r = ctx_init(c, ix);
        if (r) { c->release_all(); return r; }
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        hipError_t e = hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi);
        for (auto &ev : ln.ev_d2h)
            if (e == hipSuccess && !ev) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            c->release_all();
            if (*st) { hipStreamDestroy(*st); *st = nullptr; }
            return fail(ZH_EHIP, "host windows: %s", hipGetErrorString(e));
        }
        *flag = true;
        return ZH_OK;
    };
    if ((rc = init_ctx(&ln.ctx2, &ln.s2, &ln.init2))) return rc;
    if (ahead >= 1 && init_ctx(&ln.ctx3, &ln.s3, &ln.init3) != ZH_OK) ahead = 0;  // (no room for a third context: two, begin + finish back to back)
    if (ahead >= 2 && init_ctx(&ln.ctx4, &ln.s4, &ln.init4) != ZH_OK) ahead = 1;
    const int NC = 2 + ahead;                     // contexts the windows rotate through
    const size_t A = (size_t)ahead;               // windows begun ahead of the one being finished
    const size_t nw = (B + wq - 1) / wq, per = (B + nw - 1) / nw;
    const size_t off_ids = B * d * 4, off_keys = off_ids + B * k * 8, off_counts = off_keys + B * k * 8, need = off_counts + B * 4;
    if (need > ln.h_stage_cap) {
        if (ln.h_stage) hipHostFree(ln.h_stage);
        ln.h_stage = nullptr; ln.h_stage_cap = 0;
        const size_t cap = need + need / 2;
        hipError_t e = hipHostMalloc(&ln.h_stage, cap, hipHostMallocDefault);
        if (e != hipSuccess) return fail(ZH_ENOMEM, "hipHostMalloc(%zu): %s", cap, hipGetErrorString(e));
        ln.h_stage_cap = cap;
    }
    uint8_t *hs = static_cast<uint8_t *>(ln.h_stage);
    float *dQ = ln.wQ.as<float>();
    uint64_t *dIds = ln.wOutIds.as<uint64_t>(), *dKeys = ln.wOutKeys.as<uint64_t>();
    uint32_t *dCounts = ln.wOutCounts.as<uint32_t>();
    uint64_t *hIds = reinterpret_cast<uint64_t *>(hs + off_ids), *hKeys = reinterpret_cast<uint64_t *>(hs + off_keys);
    uint32_t *hCounts = reinterpret_cast<uint32_t *>(hs + off_counts);
    zh_search_ctx *ctxs[4] = {&ln.ctx, &ln.ctx2, &ln.ctx3, &ln.ctx4};
    hipStream_t str[4] = {ln.s, ln.s2, ln.s3, ln.s4};
    auto win = [&](size_t w, size_t *b0, size_t *nb) { *b0 = w * per; *nb = std::min(per, B - *b0); };
    auto bail = [&](int code) {  // leave nothing in flight: what was begun is abandoned, what was finished is retired, every stream drained
        const std::string why = g_err;
        for (int i = 0; i < NC; i++) {
            zh_search_ctx_abandon(ctxs[i]);
            if (ctxs[i]->state == 2) ctx_wait(ctxs[i]);
            hipStreamSynchronize(str[i]);
        }
        hipStreamSynchronize(ix->sweep_stream);
        g_err = why;
        return code;
    };
    auto retire = [&](size_t w) -> int {  // window w: wait (its outputs are complete only then), results -> pinned staging, behind them an event
        const int i = (int)(w % NC);
        size_t b0, nb;
        win(w, &b0, &nb);
        int r = ctx_wait(ctxs[i]);
        if (r) return r;
        hipError_t e = hipSuccess;
        if (k) {
            e = hipMemcpyAsync(hIds + b0 * k, dIds + b0 * k, nb * k * 8, hipMemcpyDeviceToHost, str[i]);
            if (e == hipSuccess) e = hipMemcpyAsync(hKeys + b0 * k, dKeys + b0 * k, nb * k * 8, hipMemcpyDeviceToHost, str[i]);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(hCounts + b0, dCounts + b0, nb * 4, hipMemcpyDeviceToHost, str[i]);
        if (e == hipSuccess) e = hipEventRecord(ln.ev_d2h[i], str[i]);
        return e == hipSuccess ? ZH_OK : fail(ZH_EHIP, "host windows, D2H: %s", hipGetErrorString(e));
    };
    auto hand_out = [&](size_t w) -> int {  // window w's results, once its copies have landed, into the caller's buffers
        size_t b0, nb;
        win(w, &b0, &nb);
        hipError_t e = hipEventSynchronize(ln.ev_d2h[w % NC]);
        if (e != hipSuccess) return fail(ZH_EHIP, "host windows: %s", hipGetErrorString(e));
        if (k) { memcpy(out_ids + b0 * k, hIds + b0 * k, nb * k * 8); memcpy(out_keys + b0 * k, hKeys + b0 * k, nb * k * 8); }
        memcpy(out_counts + b0, hCounts + b0, nb * 4);
        return ZH_OK;
    };
    // window w is BEGUN at step w (its context: that of window w - NC, retired first; that window's results are handed out one step later, before
    // its pinned event is recorded again) and FINISHED at step w + A
    for (size_t step = 0; step < nw + A; step++) {
        if (step < nw) {
            const size_t w = step;
            const int i = (int)(w % NC);
            size_t b0, nb;
            win(w, &b0, &nb);
            if (w >= (size_t)NC) {
                if (w >= (size_t)NC + 1 && (rc = hand_out(w - NC - 1))) return bail(rc);  // (its copies were queued one step ago: landed long since)
                if ((rc = retire(w - NC))) return bail(rc);
            }
            memcpy(hs + b0 * d * 4, q + b0 * d, nb * d * 4);  // (pageable -> pinned: the copy engine then runs beside the other windows' kernels)
            hipError_t e = hipMemcpyAsync(dQ + b0 * d, hs + b0 * d * 4, nb * d * 4, hipMemcpyHostToDevice, str[i]);
            if (e != hipSuccess) return bail(fail(ZH_EHIP, "host windows, H2D: %s", hipGetErrorString(e)));
            const float *dq = dQ + b0 * d;
            if ((rc = ctx_begin(ctxs[i], &dq, 1, nb, k, metric, mode, str[i]))) return bail(rc);
        }
        if (step >= A) {
            const size_t w = step - A;
            size_t b0, nb;
            win(w, &b0, &nb);
            uint64_t *oi = dIds + b0 * k, *ok = dKeys + b0 * k;
            uint32_t *oc = dCounts + b0;
            if ((rc = ctx_finish(ctxs[w % NC], &oi, &ok, &oc, ix->sweep_stream))) return bail(rc);
        }
    }
    // what is still in flight: the last NC windows were never retired, the one before them not handed out
    const size_t first_unretired = nw > (size_t)NC ? nw - NC : 0;
    if (first_unretired >= 1 && (rc = hand_out(first_unretired - 1))) return bail(rc);
    for (size_t w = first_unretired; w < nw; w++) {
        if ((rc = retire(w))) return bail(rc);
        if ((rc = hand_out(w))) return bail(rc);
    }
    return ZH_OK;
}

// one round of the combining front end: the requests of `grp` (same top_k, metric, mode) as ONE internal batch on lane `ln`
static void run_group(zh_index *ix, zh_index::Lane &ln, const std::vector<zh_index::CombineReq *> &grp) {
    auto all_fail = [&](int rc) {
        const std::string why = g_err;
        for (auto *r : grp) { r->rc = rc; r->err = why; }
    };
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return all_fail(rc);
    hipError_t e;
    auto hip_fail = [&](hipError_t err, const char *what) { all_fail(fail(ZH_EHIP, "%s: %s", what, hipGetErrorString(err))); };
    if (!ln.init) {  // (`init` only once BOTH the context and its stream exist; a partial lane is taken down again)
        if ((rc = ctx_init(&ln.ctx, ix))) { ln.ctx.release_all(); return all_fail(rc); }
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);  // (hi = the numerically lowest = highest priority: the light kernels' pool, as the pipelined callers')
        if ((e = hipStreamCreateWithPriority(&ln.s, hipStreamNonBlocking, hi)) != hipSuccess) { ln.ctx.release_all(); ln.s = nullptr; return hip_fail(e, "hipStreamCreate"); }
        ln.init = true;
    }
    hipStream_t s = ln.s;
    const uint32_t d = ix->opt.dim;
    const size_t k = grp[0]->k;
    size_t B = 0;
    for (auto *r : grp) B += r->b;
    if ((rc = ln.wQ.ensure(B * d * 4)) || (rc = ln.wOutIds.ensure(std::max<size_t>(B * k, 1) * 8)) ||
        (rc = ln.wOutKeys.ensure(std::max<size_t>(B * k, 1) * 8)) || (rc = ln.wOutCounts.ensure(B * 4)))
        return all_fail(rc);
    bool wander = false;
    const size_t wq = grp.size() == 1 ? host_windows_wanted(ix, B, k, &wander) : 0;
    if (wq) {  // one large batch: windows over two contexts (three, one begun ahead, where the walk wanders), copies beside the kernels
        const char *la_e = getenv("ZH_HOST_LOOKAHEAD");  // tests / A-B, read per call: 0 never, 1 / 2 always, that many windows begun ahead
        const int ahead = la_e ? (la_e[0] == '2' ? 2 : (la_e[0] == '1' ? 1 : 0)) : (wander ? ZH_HOST_AHEAD_WANDER : 0);
        if (search_host_windows(ix, ln, wq, ahead, grp[0]->q, B, k, grp[0]->metric, grp[0]->mode, grp[0]->ids, grp[0]->keys, grp[0]->counts) == ZH_OK) {
            std::lock_guard<std::mutex> ls(ix->stats_mu);
            ix->stats.host_window_calls_accum++;
            return;
        }
        // (a window passed a per-batch limit, or an allocation failed: nothing is in flight; the classic path below decides what the call returns)
    }
    const bool staged = grp.size() > 1;  // a lone caller's buffers are used as they are
    uint8_t *hs = nullptr;
    const size_t off_ids = B * d * 4, off_keys = off_ids + B * k * 8, off_counts = off_keys + B * k * 8, need = off_counts + B * 4;
    if (staged) {
        if (need > ln.h_stage_cap) {
            if (ln.h_stage) hipHostFree(ln.h_stage);
            ln.h_stage = nullptr; ln.h_stage_cap = 0;
            const size_t cap = need + need / 2;
            if ((e = hipHostMalloc(&ln.h_stage, cap, hipHostMallocDefault)) != hipSuccess) { all_fail(fail(ZH_ENOMEM, "hipHostMalloc(%zu): %s", cap, hipGetErrorString(e))); return; }
            ln.h_stage_cap = cap;
        }
        hs = static_cast<uint8_t *>(ln.h_stage);
        size_t o = 0;
        for (auto *r : grp) { memcpy(hs + o, r->q, r->b * d * 4); o += r->b * d * 4; }
        if ((e = hipMemcpyAsync(ln.wQ.p, hs, B * d * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, "H2D");
    } else if ((e = hipMemcpyAsync(ln.wQ.p, grp[0]->q, B * d * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
        return hip_fail(e, "H2D");
    rc = search_locked(ix, ln.wQ.as<float>(), B, k, grp[0]->metric, grp[0]->mode, ln.wOutIds.as<uint64_t>(), ln.wOutKeys.as<uint64_t>(),
                       ln.wOutCounts.as<uint32_t>(), s, &ln.ctx);
    if (rc) return all_fail(rc);
    uint64_t *hi = staged ? reinterpret_cast<uint64_t *>(hs + off_ids) : grp[0]->ids;
    uint64_t *hk = staged ? reinterpret_cast<uint64_t *>(hs + off_keys) : grp[0]->keys;
    uint32_t *hc = staged ? reinterpret_cast<uint32_t *>(hs + off_counts) : grp[0]->counts;
    e = hipSuccess;
    if (k) {
        e = hipMemcpyAsync(hi, ln.wOutIds.p, B * k * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hk, ln.wOutKeys.p, B * k * 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hc, ln.wOutCounts.p, B * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "D2H");
    if (staged) {
        size_t b0 = 0;
        for (auto *r : grp) {
            if (k) { memcpy(r->ids, hi + b0 * k, r->b * k * 8); memcpy(r->keys, hk + b0 * k, r->b * k * 8); }
            memcpy(r->counts, hc + b0, r->b * 4);
            b0 += r->b;
        }
        std::lock_guard<std::mutex> ls(ix->stats_mu);
        ix->stats.combined_batches_accum++;
        ix->stats.combined_calls_accum += grp.size();
    }
}

extern "C" int zh_search_batch(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode,
                               uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    if (!ix || (b && (!q || !out_counts || (k && (!out_ids || !out_keys))))) return fail(ZH_EINVAL, "zh_search_batch: null argument");
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k %zu > ZH_MAX_TOPK (%u)", k, ZH_MAX_TOPK);
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (b == 0) return ZH_OK;
    zh_index::CombineReq me;
    me.q = q; me.b = b; me.k = k; me.metric = metric; me.mode = mode; me.ids = out_ids; me.keys = out_keys; me.counts = out_counts;
    bool lead;
    {
        std::lock_guard<std::mutex> lk(ix->cmu);
        ix->cpend.push_back(&me);
        lead = !ix->cleader;  // nobody leads: this caller does, at once
        if (lead) ix->cleader = true;
    }
    for (;;) {
        if (!lead) {  // sleep until my request is done, or until a finishing leader hands me the lead
            std::unique_lock<std::mutex> l(me.m);
            me.cv.wait(l, [&] { return me.done || me.lead; });
            if (me.done) break;
            me.lead = false;
        }
        // ---- lead one round ----
        std::unique_lock<std::mutex> lk(ix->cmu);
        if (ix->clast >= 2) {
            // The round before served a crowd whose threads are on their way back with their next requests.  Taking the queue as it
            // stands would split a crowd of N into two cohorts of N / 2 that take turns (one is served while the other queues), and a
            // round costs about the same for 30 queries as for 60: wait until the arrivals pause (nothing new for ~10 us), 120 us at most.
            // (polled with yields: sleep_for(10 us) takes ~60 us with the default timer slack)
            const auto t0 = std::chrono::steady_clock::now();
            auto tq = t0;
            size_t n0 = ix->cpend.size();
            for (;;) {
                lk.unlock();
                std::this_thread::yield();
                lk.lock();
                const auto now = std::chrono::steady_clock::now();
                if (ix->cpend.size() != n0) { n0 = ix->cpend.size(); tq = now; }
                if (now - tq > std::chrono::microseconds(10) || now - t0 > std::chrono::microseconds(120)) break;
            }
        }
        // the head of the queue and everything behind it that can share its batch (same top_k, metric, mode; arrival order kept)
        // (nothing between taking requests off the queue and handing the lead on may throw across the extern "C" boundary or leave
        // `cleader` set with nobody leading: the list's room is reserved BEFORE anything is taken, and a round that throws fails its requests)
        std::vector<zh_index::CombineReq *> grp;
        try {
            grp.reserve(ix->cpend.size());
        } catch (...) {  // no memory to even list the round: my own request fails, the lead goes to whoever heads the queue without me
            for (auto it = ix->cpend.begin(); it != ix->cpend.end(); ++it)
                if (*it == &me) { ix->cpend.erase(it); break; }
            me.rc = ZH_ENOMEM;
            if (ix->cpend.empty()) ix->cleader = false;
            else {
                zh_index::CombineReq *nx = ix->cpend.front();
                std::lock_guard<std::mutex> l(nx->m);
                nx->lead = true;
                nx->cv.notify_one();
            }
            break;
        }
        const zh_index::CombineReq *head = ix->cpend.front();  // (never empty: the leader's own request is in it until served)
        size_t total = 0;
        for (auto it = ix->cpend.begin(); it != ix->cpend.end();) {
            zh_index::CombineReq *r = *it;
            if (r->k == head->k && r->metric == head->metric && r->mode == head->mode && (grp.empty() || total + r->b <= 8192)) {
                grp.push_back(r);
                total += r->b;
                it = ix->cpend.erase(it);
            } else
                ++it;
        }
        lk.unlock();
        try {
            run_group(ix, ix->lanes[0], grp);
        } catch (...) {  // (bad_alloc in a message copy or a host vector: the round's requests fail, the queue lives on)
            for (auto *r : grp) r->rc = ZH_ENOMEM;
        }
        bool mine = false;
        for (auto *r : grp) {
            if (r == &me) { mine = true; continue; }
            std::lock_guard<std::mutex> l(r->m);  // (notify under the lock: the owner destroys r as soon as it sees done)
            r->done = true;
            r->cv.notify_one();
        }
        lk.lock();
        ix->clast = grp.size();
        if (!mine) { lk.unlock(); lead = true; continue; }  // my own request waits in the queue (it could not share the head's batch): lead on
        // served: hand the lead to the head of the queue, or retire it
        if (ix->cpend.empty()) ix->cleader = false;
        else {
            zh_index::CombineReq *nx = ix->cpend.front();
            std::lock_guard<std::mutex> l(nx->m);
            nx->lead = true;
            nx->cv.notify_one();
        }
        break;
    }
    if (me.rc) return fail(me.rc, "%s", me.err.empty() ? "zh_search_batch: out of host memory" : me.err.c_str());
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// exact search (zh_exact.hip): every live row against every query, canonical keys, top_k by (key, id)
// ------------------------------------------------------------------------------------------------
#define ZH_EXACT_BATCH 1024u             // queries per internal batch
#define ZH_EXACT_KEY_BYTES (size_t(1) << 30)  // key scratch of one row chunk: queries x rows x 8 bytes

// ---- what the families below share: exact, filtered and range search, self-join, k-NN graph, forest k-NN graph, forest self-join, forest range search ----
static hipStream_t call_stream(const zh_index *ix, void *stream) { return stream ? (hipStream_t)stream : ix->stream; }

// the score kernels' parameter: the mode, for the metrics that have one
static int score_param(int metric, int mode) { return (metric == ZH_COSINE || metric == ZH_MINKOWSKI || metric == ZH_PNORM) ? mode : 0; }

// The per-call scratch, each family's buffers listed once.  The guard of a call gives its set back to the driver however the call returns: an idle
// index holds only the live-row views (live_dev's list and bitmap survive every call; zh_index_destroy frees them).  Every family scans with the exact
// search's buffers, the forest graph with the graph's as well, the forest join with the join's and the forest graph's, the forest range search with
// the range search's and the forest join's, the cross-join (all on its LEFT index) with the join's and its own views.
enum : unsigned { SCR_EX = 1, SCR_FL = 2, SCR_RG = 4, SCR_JN = 8, SCR_KN = 16, SCR_FK = 32, SCR_FJ = 64, SCR_FR = 128, SCR_XJ = 256, SCR_RF = 512, SCR_RV = 1024, SCR_ND = 2048, SCR_GS = 4096, SCR_GE = 8192, SCR_PR = 16384, SCR_XK = 32768 };  // one bit per list
enum : unsigned {
    SCRATCH_EXACT = SCR_EX,
    SCRATCH_FILTER = SCR_FL | SCRATCH_EXACT,
    SCRATCH_RANGE = SCR_RG | SCRATCH_EXACT,
    SCRATCH_JOIN = SCR_JN | SCRATCH_EXACT,
    SCRATCH_KNN = SCR_KN | SCRATCH_EXACT,
    SCRATCH_FKNN = SCR_FK | SCRATCH_KNN,
    SCRATCH_REFINE = SCR_RF | SCRATCH_KNN,
    SCRATCH_REVERSE = SCR_RV | SCRATCH_REFINE,
    SCRATCH_DESCENT = SCR_ND | SCRATCH_REVERSE,
    SCRATCH_PRUNE = SCR_PR | SCRATCH_REVERSE,
    SCRATCH_GRAPH_ATTACH = SCR_RF,  // (the host entry's counts and staged chunk of ids)
    SCRATCH_GSEARCH = SCR_GS,
    SCRATCH_GSEARCH_FILTERED = SCR_GS | SCR_FL,  // (the filter pass writes the filtered exact search's buffers)
    SCRATCH_GEXTEND = SCR_GE | SCR_GS,  // (the walk's staged queries, their norms and the host entry's seeds are graph search's)
    SCRATCH_FJOIN = SCR_FJ | SCRATCH_JOIN | SCRATCH_FKNN,
    SCRATCH_FRANGE = SCR_FR | SCRATCH_RANGE | SCRATCH_FJOIN,
    SCRATCH_XJOIN = SCR_XJ | SCRATCH_JOIN,  // (on the left index)
    SCRATCH_XKNN = SCR_XK | SCRATCH_KNN,    // (on the left index)
};
static void release_scratch(zh_index *ix, unsigned families) {
    auto drop = [&](unsigned list, std::initializer_list<DevBuf *> bs) {
        if (families & list)
            for (DevBuf *b : bs) b->release();
    };
    drop(SCR_EX, {&ix->ex_QQ, &ix->ex_keys, &ix->ex_visits, &ix->ex_cbase, &ix->ex_ckeys, &ix->ex_cids, &ix->ex_run_ids, &ix->ex_run_keys, &ix->ex_run_counts,
                  &ix->ex_Q, &ix->ex_ids, &ix->ex_kout, &ix->ex_counts, &ix->ex_Qh, &ix->ex_qmeta, &ix->ex_tau, &ix->ex_cnt, &ix->ex_lid, &ix->ex_llo,
                  &ix->ex_lhi, &ix->ex_scr, &ix->ex_over});
    drop(SCR_FL, {&ix->fl_filter, &ix->fl_bits, &ix->fl_pos, &ix->fl_bcount, &ix->fl_bexcl, &ix->fl_tmp, &ix->fl_list});
    drop(SCR_RG, {&ix->rg_maxk, &ix->rg_cnt, &ix->rg_ctr, &ix->rg_pv0, &ix->rg_pv1, &ix->rg_pk0, &ix->rg_pk1, &ix->rg_cand, &ix->rg_tmp, &ix->rg_off,
                  &ix->rg_oids, &ix->rg_okeys});
    drop(SCR_JN, {&ix->jn_ctr, &ix->jn_maxk, &ix->jn_tau, &ix->jn_pv0, &ix->jn_pv1, &ix->jn_pk0, &ix->jn_pk1, &ix->jn_qm, &ix->jn_cid, &ix->jn_first,
                  &ix->jn_cand, &ix->jn_rows, &ix->jn_tmp, &ix->jn_oa, &ix->jn_ob, &ix->jn_okeys});
    drop(SCR_XJ, {&ix->xj_qma, &ix->xj_cida, &ix->xj_qmb, &ix->xj_cidb});
    drop(SCR_XK, {&ix->xk_qmb, &ix->xk_cidb});
    drop(SCR_KN, {&ix->kn_qm, &ix->kn_cid, &ix->kn_pos, &ix->kn_A, &ix->kn_pmeta, &ix->kn_pid, &ix->kn_cbase, &ix->kn_pids, &ix->kn_pkeys, &ix->kn_pcounts,
                  &ix->kn_oids, &ix->kn_okeys, &ix->kn_ocounts});
    drop(SCR_FK, {&ix->fk_ntree, &ix->fk_rl, &ix->fk_flag, &ix->fk_excl, &ix->fk_tmp, &ix->fk_rows, &ix->fk_ctr, &ix->fk_lens, &ix->fk_takes, &ix->fk_rbase,
                  &ix->fk_cbase, &ix->fk_groups, &ix->fk_groff, &ix->fk_segs, &ix->fk_colsrc, &ix->fk_crow, &ix->fk_hrow, &ix->fk_held, &ix->fk_CA,
                  &ix->fk_cmeta, &ix->fk_cqm, &ix->fk_HA, &ix->fk_hmeta, &ix->fk_qrow, &ix->fk_maxk, &ix->fk_redo, &ix->fk_pos});
    drop(SCR_RF, {&ix->rf_tab, &ix->rf_cnt, &ix->rf_stage, &ix->rf_ctr});
    drop(SCR_RV, {&ix->rv_deg, &ix->rv_cur, &ix->rv_off, &ix->rv_sums, &ix->rv_csr, &ix->rv_heavy, &ix->rv_uni, &ix->rv_ctr, &ix->rv_oids, &ix->rv_ocounts,
                  &ix->rv_odeg});
    drop(SCR_ND, {&ix->nd_tab[0], &ix->nd_tab[1], &ix->nd_key[0], &ix->nd_key[1], &ix->nd_uni[0], &ix->nd_uni[1], &ix->nd_mask, &ix->nd_list, &ix->nd_qq,
                  &ix->nd_ctr});
    drop(SCR_PR, {&ix->pr_qq, &ix->pr_ctr});
    drop(SCR_GS, {&ix->gs_QQ, &ix->gs_ctr, &ix->gs_Q, &ix->gs_seeds, &ix->gs_oids, &ix->gs_okeys, &ix->gs_ocounts});
    drop(SCR_GE, {&ix->ge_seeds, &ix->ge_ids, &ix->ge_keys, &ix->ge_counts, &ix->ge_qq, &ix->ge_deg, &ix->ge_cur, &ix->ge_off, &ix->ge_sums, &ix->ge_csr,
                  &ix->ge_touched, &ix->ge_ctr});
    drop(SCR_FJ, {&ix->fj_leafof, &ix->fj_pieces, &ix->fj_linel, &ix->fj_linek, &ix->fj_segs, &ix->fj_cand});
    drop(SCR_FR, {&ix->fr_counts, &ix->fr_inline, &ix->fr_rowbase, &ix->fr_candbase, &ix->fr_visitbase, &ix->fr_totals, &ix->fr_leafcount, &ix->fr_leaffill,
                  &ix->fr_groupbase, &ix->fr_grouprowbase, &ix->fr_loghead, &ix->fr_logctl, &ix->fr_logpool, &ix->fr_visits, &ix->fr_groups, &ix->fr_groupoff,
                  &ix->fr_vk0, &ix->fr_vk1, &ix->fr_vtmp, &ix->fr_segs});
}
struct ScratchGuard {
    zh_index *ix;
    unsigned families;
    ~ScratchGuard() { release_scratch(ix, families); }
};

// what the last call of a family left for its zh_*_info export
template <typename Info>
static int get_info(const zh_index *ix, Info zh_index::*slot, Info *out, const char *who) {
    if (!ix || !out) return fail(ZH_EINVAL, "%s: null argument", who);
    zh_index *m = const_cast<zh_index *>(ix);
    std::lock_guard<std::mutex> lk(m->stats_mu);
    *out = m->*slot;
    return ZH_OK;
}

// Path 2's view of the fp16 copy of the rows: made if need be, and read, under blk_mu -- the caller holds it, for as long as it reads order.perm on
// the device.  *have = false: no copy (no room for it, or the per-row scales alone) and path 1 answers.
struct HalfView {
    const void *Xh = nullptr;
    const float2 *rowMeta = nullptr;
    float rho = 0.f;
    const uint32_t *perm = nullptr;  // position -> row under a row order, else null
    uint64_t perm_rows = 0;
};
static int half_view(zh_index *ix, HalfView *v, bool *have) {
    bool ok = false;
    *have = false;
    int rc = ensure_row_half(ix, &ok);
    if (rc) return rc;
    if (!ok || !ix->half.tiles.p) return ZH_OK;
    *have = true;
    v->Xh = ix->half.tiles.p; v->rowMeta = ix->half.meta.as<float2>(); v->rho = ix->half.rho;
    v->perm = ix->order.rows ? ix->order.perm.as<uint32_t>() : nullptr; v->perm_rows = ix->order.rows;
    return ZH_OK;
}

// Path 2's per-line lists, B lines of cap slots (exact_batch2, knn_panel2, fknn_batch2): lists_ensure sizes them (and the base table, where the
// caller's final_kernel reads ex_cbase) and fills e's list members, lists_reset empties them on the stream, list_bases writes a base table, and
// lists_end reads the counts back and waits.  The tau each line starts from is the caller's.
static int lists_ensure(zh_index *ix, uint32_t B, uint32_t cap, bool cbase, ZhExact2 *e) {
    int rc;
    if ((rc = ix->ex_tau.ensure((size_t)B * 4)) || (rc = ix->ex_cnt.ensure((size_t)B * 4)) || (rc = ix->ex_lid.ensure((size_t)B * cap * 4)) ||
        (rc = ix->ex_llo.ensure((size_t)B * cap * 4)) || (rc = ix->ex_lhi.ensure((size_t)B * cap * 4)) || (rc = ix->ex_scr.ensure((size_t)B * cap * 12)) ||
        (rc = ix->ex_over.ensure(8)) || (rc = ix->ex_ckeys.ensure((size_t)B * cap * 8)) || (rc = ix->ex_cids.ensure((size_t)B * cap * 4)) ||
        (cbase && (rc = ix->ex_cbase.ensure(((size_t)B + 1) * 8))))
        return rc;
    e->B = B; e->cap = cap;
    e->tau = ix->ex_tau.as<uint32_t>(); e->cnt = ix->ex_cnt.as<uint32_t>(); e->over = ix->ex_over.as<uint32_t>();
    e->lid = ix->ex_lid.as<uint32_t>(); e->llo = ix->ex_llo.as<uint32_t>(); e->lhi = ix->ex_lhi.as<uint32_t>();
    return ZH_OK;
}
static int lists_reset(const ZhExact2 &e, hipStream_t s) {
    HIPCHK(hipMemsetAsync(e.cnt, 0, (size_t)e.B * 4, s));
    HIPCHK(hipMemsetAsync(e.over, 0, 8, s));  // (word 1: the filtered scan's skipped tiles)
    return ZH_OK;
}
// the base table of B lines: cb[b] = b * cap for its B + 1 entries, copied to dst.  cb is the caller's: it lives until the caller has waited for the stream
static int list_bases(void *dst, std::vector<uint64_t> &cb, uint32_t cap, hipStream_t s) {
    for (size_t b = 0; b < cb.size(); b++) cb[b] = (uint64_t)b * cap;
    HIPCHK(hipMemcpyAsync(dst, cb.data(), cb.size() * 8, hipMemcpyHostToDevice, s));
    return ZH_OK;
}
// *overflowed: a list ran over and the batch's answer is not valid; otherwise the lines' survivors are added to *survivors
static int lists_end(const ZhExact2 &e, hipStream_t s, bool *overflowed, uint64_t *survivors, uint64_t *tiles_skipped = nullptr) {
    const uint32_t B = e.B;
    std::vector<uint32_t> h_cnt((size_t)B + 2);
    HIPCHK(hipMemcpyAsync(h_cnt.data(), e.cnt, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_cnt.data() + B, e.over, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *overflowed = h_cnt[B] != 0;
    if (tiles_skipped) *tiles_skipped += h_cnt[B + 1];
    if (!*overflowed)
        for (uint32_t b = 0; b < B; b++) *survivors += h_cnt[b];
    return ZH_OK;
}

// live rows before stored row `row`; the cursor makes a call's ascending questions one walk over h_dead
struct LiveCursor {
    uint64_t row = 0, rank = 0;
};
static uint64_t live_before(const zh_index *ix, uint64_t row, LiveCursor *c) {
    if (row < c->row) *c = LiveCursor{};
    for (; c->row < row; c->row++) c->rank += !(c->row < ix->h_dead.size() && ix->h_dead[c->row]);
    return c->rank;
}

// The forest scans' column tiles per chunk: ZH_FKNN_CHUNK, halved while the launch would not fill the device (about 1024 blocks), never under 8.
// blocks_at(ch) = the launch's blocks at ch tiles per chunk; its last call is the one for the chunk returned.
template <typename Blocks>
static uint32_t fill_chunk(Blocks blocks_at) {
    uint32_t ch = ZH_FKNN_CHUNK;
    while (blocks_at(ch) < 1024 && ch > 8) ch /= 2;
    return ch;
}

// the ascending live rows (path 1) and the live-row bitmap (path 2) on the device (under mu, exclusive), rebuilt when rows were appended or
// removed since
static int exact_live_rows(zh_index *ix) {
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    if (ix->live_dev.current(ix)) return ZH_OK;
    std::vector<uint32_t> live;
    live.reserve(ix->n_rows - ix->n_dead);
    for (uint64_t r = 0; r < ix->n_rows; r++)
        if (!(r < ix->h_dead.size() && ix->h_dead[r])) live.push_back((uint32_t)r);
    int rc = ix->live_dev.rows.ensure(std::max<size_t>(live.size(), 1) * 4);
    if (rc) return rc;
    if (!live.empty()) HIPCHK(hipMemcpy(ix->live_dev.rows.p, live.data(), live.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> bits((ix->n_rows + 31) / 32 + 1, 0u);
    for (uint32_t r : live) bits[r >> 5] |= 1u << (r & 31);
    if ((rc = ix->live_dev.bits.ensure(bits.size() * 4))) return rc;
    HIPCHK(hipMemcpy(ix->live_dev.bits.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
    ix->live_dev.mark_built(ix, live.size());
    return ZH_OK;
}

// one internal batch (B <= ZH_EXACT_BATCH) on device pointers, enqueued on s.  Row chunk after row chunk: keys of all queries into the
// scratch, each query's top_k of every sub-chunk of L positions (select_kernel), a query's sub-chunks merged (final_kernel), the chunk's
// answer merged into the running one (the caller's outputs) -- merge_wave_kernel / final_kernel<true>.
// st (the k-NN join between two indexes): the index whose table and id base the rows dLive are of, all scratch staying on ix; null: ix itself.
static int exact_batch(zh_index *ix, const uint32_t *dLive, uint64_t n_live, const float *dQ, uint32_t B, uint32_t k, int metric, int mode,
                       uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, uint64_t *launches, const zh_index *st = nullptr) {
    const uint32_t d = ix->opt.dim;
    if (!st) st = ix;
    if (k == 0) { HIPCHK(hipMemsetAsync(dCounts, 0, (size_t)B * 4, s)); return ZH_OK; }
    if (n_live == 0) { HIPCHK(zh_launch_exact_empty(B, k, dIds, dKeys, dCounts, s)); return ZH_OK; }
    const uint32_t L = k <= 512 ? 2048u : 4096u, kk = std::min(k, L);
    uint64_t rc_rows = std::max<uint64_t>(L, ZH_EXACT_KEY_BYTES / 8 / B / L * L);
    rc_rows = std::min<uint64_t>(rc_rows, (n_live + L - 1) / L * L);
    const uint32_t nsub_max = (uint32_t)(rc_rows / L);
    int rc;
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_keys.ensure((size_t)B * rc_rows * 8)) ||
        (rc = ix->ex_visits.ensure((size_t)B * nsub_max * sizeof(ZhVisit))) || (rc = ix->ex_cbase.ensure(((size_t)B * nsub_max + 1) * 8)) ||
        (rc = ix->ex_ckeys.ensure((size_t)B * nsub_max * kk * 8)) || (rc = ix->ex_cids.ensure((size_t)B * nsub_max * kk * 4)) ||
        (rc = ix->ex_run_ids.ensure((size_t)2 * B * k * 8)) || (rc = ix->ex_run_keys.ensure((size_t)2 * B * k * 8)) ||
        (rc = ix->ex_run_counts.ensure((size_t)2 * B * 4)))
        return rc;
    const int param = score_param(metric, mode);
    uint64_t *runIds = ix->ex_run_ids.as<uint64_t>(), *runKeys = ix->ex_run_keys.as<uint64_t>();
    uint32_t *runCounts = ix->ex_run_counts.as<uint32_t>();
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    for (uint64_t p0 = 0; p0 < n_live; p0 += rc_rows) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(rc_rows, n_live - p0), nsub = (nr + L - 1) / L;
        HIPCHK(zh_launch_exact_score(st->X.as<float>(), d, dLive, p0, nr, dQ, ix->ex_QQ.as<float>(), B, metric, param, ix->ex_keys.as<uint64_t>(),
                                     rc_rows, s));
        HIPCHK(zh_launch_exact_visits(B, nsub, nr, L, k, p0, rc_rows, ix->ex_visits.as<ZhVisit>(), ix->ex_cbase.as<uint64_t>(), s));
        HIPCHK(zh_launch_select(ix->ex_visits.as<ZhVisit>(), (uint64_t)B * nsub, dLive, ix->ex_keys.as<uint64_t>(), ix->ex_ckeys.as<uint64_t>(),
                                ix->ex_cids.as<uint32_t>(), L, nullptr, s));
        if (p0 == 0) {
            HIPCHK(zh_launch_final(ix->ex_cbase.as<uint64_t>(), B, nsub, k, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), st->opt.id_base,
                                   dIds, dKeys, dCounts, nullptr, s));
        } else {  // this chunk's answer into slot 1, the running one (the outputs) into slot 0, both merged back into the outputs
            HIPCHK(zh_launch_final(ix->ex_cbase.as<uint64_t>(), B, nsub, k, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), st->opt.id_base,
                                   runIds + (size_t)B * k, runKeys + (size_t)B * k, runCounts + B, nullptr, s));
            HIPCHK(hipMemcpyAsync(runIds, dIds, (size_t)B * k * 8, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(runKeys, dKeys, (size_t)B * k * 8, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(runCounts, dCounts, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(zh_launch_merge(2, B, k, runIds, runKeys, runCounts, dIds, dKeys, dCounts, 0, 0, s));
        }
        (*launches)++;
    }
    return ZH_OK;
}

// Path 2 of one internal batch: the matrix-core interval scan in geometrically growing row chunks, a per-query tau and list, canonical keys for
// the survivors, final_kernel's (key, id) top_k.  *used = false: path 2 does not serve this index / batch (path 1 answers); *overflowed: a list
// ran over and the outputs are not valid (the caller answers the batch by path 1).
// Under a filter (f; filter_prepare below) the scan reads f->dPos, the allowed-and-live bitmap by position, in place of the live bitmap, and the
// chunks are placed by the cumulative count of ALLOWED rows (f->cum, per ZH_FILTER_BLOCK_ROWS positions): the first one ends where max(k, 4096) of
// them have been seen, each later one holds ZH_EXACT_GROWTH times as many -- wherever in the table they sit, every query has its tau before a
// large chunk arrives, exactly as without a filter.
#define ZH_EXACT_GROWTH 4
struct ExactFilter {
    uint64_t n_allowed = 0;           // rows allowed and live
    uint64_t tiles = 0;               // 16-position tiles of the scan that hold one (by position under a row order)
    const uint32_t *dList = nullptr;  // ... ascending, for path 1 (made when path 1 is first needed: filter_list)
    bool path2 = false;               // the path rule chose path 2 and the fp16 copy is there
    const uint32_t *dPos = nullptr;   // path 2: the bitmap by position, made for the row order of this view:
    HalfView v;
    std::vector<uint32_t> cum;       // exclusive sums of the allowed rows per block of positions (blocks + 1 entries)
};
static int exact_batch2(zh_index *ix, const float *dQ, uint32_t B, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts,
                        hipStream_t s, bool *used, bool *overflowed, uint64_t *survivors, uint64_t *launches, const ExactFilter *f = nullptr,
                        uint64_t *tiles_skipped = nullptr) {
    *used = false; *overflowed = false;
    const uint32_t d = ix->opt.dim;
    if (k == 0 || !zh_exact_mfma_supported(d, metric) || (f ? f->n_allowed : ix->live_dev.n_live) < std::max<uint64_t>(k, 8192)) return ZH_OK;
    int rc;
    HalfView v;
    bool have = false;
    {
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if ((rc = half_view(ix, &v, &have))) return rc;
    }
    if (!have) return ZH_OK;
    if (f && (v.perm != f->v.perm || v.perm_rows != f->v.perm_rows)) return ZH_OK;  // (the row order changed since f->dPos was made: path 1)
    const uint32_t cap = 16384 + 8 * k;  // first chunk (<= max(k, 4096) rows, all listed) + a few growth steps' worth of k
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_Qh.ensure((size_t)B * d * 2)) || (rc = ix->ex_qmeta.ensure((size_t)B * 16))) return rc;
    ZhExact2 e{v.Xh, v.rowMeta, v.perm, v.perm_rows, f ? f->dPos : ix->live_dev.bits.as<uint32_t>(), ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), B,
               zh_approx_bound(metric, d, 1), v.rho};
    if ((rc = lists_ensure(ix, B, cap, true, &e))) return rc;
    std::vector<uint64_t> cb((size_t)B + 1);
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_qhalf(dQ, B, d, ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), 1, s));
    HIPCHK(hipMemsetAsync(e.tau, 0xFF, (size_t)B * 4, s));
    if ((rc = lists_reset(e, s)) || (rc = list_bases(ix->ex_cbase.p, cb, cap, s))) return rc;
    const uint64_t n = ix->n_rows;  // positions of the copy; removed rows are masked by the bitmap
    uint64_t chunk = (std::max<uint64_t>(k, 4096) + 15) / 16 * 16;
    for (uint64_t p0 = 0; p0 < n && !f; p0 += chunk, chunk *= ZH_EXACT_GROWTH) {
        const uint64_t p1 = std::min(n, p0 + chunk);
        HIPCHK(zh_launch_exact_mfma(d, metric, mode, e, p0, p1, s));
        HIPCHK(zh_launch_exact_prune(e, k, ix->ex_scr.as<uint32_t>(), s));
        (*launches)++;
    }
    if (f) {  // chunks of whole blocks, ended by the allowed rows seen (the first lists at most its target + a block's rows: below cap)
        const size_t nb = f->cum.size() - 1;
        uint64_t target = std::max<uint64_t>(k, 4096);
        for (size_t j0 = 0; j0 < nb; target *= ZH_EXACT_GROWTH) {
            size_t j1 = j0 + 1;
            while (j1 < nb && f->cum[j1] - f->cum[j0] < target) j1++;
            HIPCHK(zh_launch_exact_mfma(d, metric, mode, e, (uint64_t)j0 * ZH_FILTER_BLOCK_ROWS, std::min<uint64_t>(n, (uint64_t)j1 * ZH_FILTER_BLOCK_ROWS), s, true));
            HIPCHK(zh_launch_exact_prune(e, k, ix->ex_scr.as<uint32_t>(), s));
            (*launches)++;
            j0 = j1;
        }
    }
    HIPCHK(zh_launch_exact_survivor_keys(ix->X.as<float>(), d, dQ, ix->ex_QQ.as<float>(), metric, mode, e, ix->ex_ckeys.as<uint64_t>(),
                                         ix->ex_cids.as<uint32_t>(), s));
    HIPCHK(zh_launch_final(ix->ex_cbase.as<uint64_t>(), B, 1, k, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), ix->opt.id_base, dIds, dKeys,
                           dCounts, nullptr, s));
    if ((rc = lists_end(e, s, overflowed, survivors, tiles_skipped))) return rc;  // (cb is this frame's)
    *used = true;
    return ZH_OK;
}

// one internal batch: path 2 where it serves, path 1 otherwise and for a batch whose path-2 lists ran over
static int exact_one(zh_index *ix, const float *dQ, uint32_t B, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts,
                     hipStream_t s, zh_exact_info *inf) {
    bool used = false, overflowed = false;
    int rc = exact_batch2(ix, dQ, B, k, metric, mode, dIds, dKeys, dCounts, s, &used, &overflowed, &inf->survivors, &inf->launches);
    if (rc) return rc;
    if (used) inf->path = 2;
    if (used && !overflowed) return ZH_OK;
    if (overflowed) inf->redone++;
    return exact_batch(ix, ix->live_dev.rows.as<uint32_t>(), ix->live_dev.n_live, dQ, B, k, metric, mode, dIds, dKeys, dCounts, s, &inf->launches);
}

static int exact_args(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, const void *ids, const void *keys,
                      const void *counts, const char *who) {
    if (!ix || (b && (!q || !counts || (k && (!ids || !keys))))) return fail(ZH_EINVAL, "%s: null argument", who);
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k %zu > ZH_MAX_TOPK (%u)", k, ZH_MAX_TOPK);
    return check_metric(metric, mode);
}

static void exact_record(zh_index *ix, size_t b, zh_exact_info inf) {
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    inf.batch = b;
    inf.rows_live = ix->live_dev.n_live;
    ix->ex_info = inf;
}

// the host entry points' staging: one internal batch of queries in, its answer out
static int exact_stage(zh_index *ix, size_t b, size_t k) {
    const size_t nb_max = std::min<size_t>(ZH_EXACT_BATCH, b), d = ix->opt.dim;
    int rc;
    if ((rc = ix->ex_Q.ensure(nb_max * d * 4)) || (rc = ix->ex_ids.ensure(std::max<size_t>(nb_max * k, 1) * 8)) ||
        (rc = ix->ex_kout.ensure(std::max<size_t>(nb_max * k, 1) * 8)) || (rc = ix->ex_counts.ensure(nb_max * 4)))
        return rc;
    return ZH_OK;
}

// The exact and the filtered search's loop over internal batches of at most ZH_EXACT_BATCH queries; one(dQ, nb, dIds, dKeys, dCounts) answers a
// batch on device pointers.  host: q and the outputs are HOST arrays -- each batch goes through the staging (exact_stage has run) and is waited
// for; otherwise they are device arrays, waited for once after the last batch.
template <typename One>
static int exact_batches(zh_index *ix, const float *q, size_t b, size_t k, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host,
                         hipStream_t s, One one) {
    const uint32_t d = ix->opt.dim;
    int rc;
    for (size_t b0 = 0; b0 < b; b0 += ZH_EXACT_BATCH) {
        const uint32_t nb = (uint32_t)std::min<size_t>(ZH_EXACT_BATCH, b - b0);
        if (!host) {
            if ((rc = one(q + b0 * d, nb, out_ids + b0 * k, out_keys + b0 * k, out_counts + b0))) return rc;
            continue;
        }
        HIPCHK(hipMemcpyAsync(ix->ex_Q.p, q + b0 * d, (size_t)nb * d * 4, hipMemcpyHostToDevice, s));
        if ((rc = one(ix->ex_Q.as<float>(), nb, ix->ex_ids.as<uint64_t>(), ix->ex_kout.as<uint64_t>(), ix->ex_counts.as<uint32_t>()))) return rc;
        if (k) {
            HIPCHK(hipMemcpyAsync(out_ids + b0 * k, ix->ex_ids.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_keys + b0 * k, ix->ex_kout.p, (size_t)nb * k * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipMemcpyAsync(out_counts + b0, ix->ex_counts.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (!host) HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

// both entry points once the arguments have been judged (b > 0)
static int exact_call(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts,
                      bool host, void *stream) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    ScratchGuard guard{ix, SCRATCH_EXACT};
    const hipStream_t s = call_stream(ix, stream);
    if (host && (rc = exact_stage(ix, b, k))) return rc;
    zh_exact_info inf{};
    inf.path = 1;
    rc = exact_batches(ix, q, b, k, out_ids, out_keys, out_counts, host, s, [&](const float *dQ, uint32_t nb, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
        return exact_one(ix, dQ, nb, (uint32_t)k, metric, mode, dIds, dKeys, dCounts, s, &inf);
    });
    if (rc) return rc;
    exact_record(ix, b, inf);
    return ZH_OK;
}

extern "C" int zh_search_exact_batch_device(zh_index *ix, const float *d_q, size_t b, size_t k, int metric, int mode, uint64_t *d_out_ids,
                                            uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = exact_args(ix, d_q, b, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_search_exact_batch_device");
    if (rc || b == 0) return rc;
    return exact_call(ix, d_q, b, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false, stream);
}

extern "C" int zh_search_exact_batch(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, uint64_t *out_ids,
                                     uint64_t *out_keys, uint32_t *out_counts) {
    int rc = exact_args(ix, q, b, k, metric, mode, out_ids, out_keys, out_counts, "zh_search_exact_batch");
    if (rc || b == 0) return rc;
    return exact_call(ix, q, b, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr);
}

extern "C" int zh_search_exact_info(const zh_index *ix, zh_exact_info *out) { return get_info(ix, &zh_index::ex_info, out, "zh_search_exact_info"); }

// ------------------------------------------------------------------------------------------------
// filtered exact search (zh_filter.hip + the exact search's two paths): only the rows a caller's bitmap allows are ranked
// ------------------------------------------------------------------------------------------------
// The path rule.  Path 1 gathers the allowed rows alone: its cost follows the allowed rows.  Path 2 streams every 16-row tile of the fp16 copy that
// holds an allowed row and skips the others: its cost follows the rows of the tiles it loads, plus about one row's worth per skipped tile.  Per
// row, path 1 costs ZH_FILTER_PATH1_ROW_COST times what path 2 does, so path 2 is taken when
//     16 * loaded tiles + skipped tiles <= ZH_FILTER_PATH1_ROW_COST * allowed rows.
// Measured with tests/probes/filter_probe.py on one MI355X at 10M x 768, 1024 queries, k = 100, L2SQ (table: DESIGN.md s13): all rows allowed,
// path 1 633.3 ms against path 2 109.9 ms = 5.76; a skipped tile 7 - 18 ns against 11.0 ns per loaded row.  A random tenth of the rows leaves
// few tiles empty and goes to path 1 (64.8 ms against 88.9); a contiguous tenth goes to path 2 (21.2 ms against 64.6).
#define ZH_FILTER_PATH1_ROW_COST 5.75

// the ascending list of allowed live rows, from the row bitmap and the blocks' exclusive sums filter_prepare left
static int filter_list(zh_index *ix, ExactFilter *f, hipStream_t s) {
    int rc = ix->fl_list.ensure(std::max<uint64_t>(f->n_allowed, 1) * 4);
    if (rc) return rc;
    HIPCHK(zh_launch_filter_list(ix->fl_bits.as<uint32_t>(), ix->n_rows, ix->fl_bexcl.as<uint32_t>(), ix->fl_list.as<uint32_t>(), s));
    f->dList = ix->fl_list.as<uint32_t>();
    return ZH_OK;
}

// The filter pass of one call (under mu, exclusive; exact_live_rows has run): allowed AND live and its count, the path, and what that path reads --
// the list (path 1), or the bitmap by position and the blocks' sums the chunks are placed by (path 2).  dFilter: n_bits bits in device memory.
// Nothing comes from the host but the call's arguments; two small copies come back (the blocks' sums).  ZH_FILTER_PATH=1|2 (probes and tests,
// read per call) forces a path where it can serve.
static int filter_prepare(zh_index *ix, const uint32_t *dFilter, uint64_t n_bits, uint32_t k, int metric, hipStream_t s, ExactFilter *f) {
    const uint64_t n = ix->n_rows;
    if (!n) return ZH_OK;
    const size_t nb = (size_t)((n + ZH_FILTER_BLOCK_ROWS - 1) / ZH_FILTER_BLOCK_ROWS);
    int rc;
    if ((rc = ix->fl_bits.ensure((n + 63) / 64 * 8)) || (rc = ix->fl_bcount.ensure(nb * 4)) || (rc = ix->fl_bexcl.ensure((2 * (nb + 1) + 1) * 4)) ||
        (rc = ix->fl_tmp.ensure((nb / 1024 + 2) * 4)))
        return rc;
    uint32_t *excl = ix->fl_bexcl.as<uint32_t>();  // [0, nb]: by row; [nb + 1, 2 nb + 1]: by position under a row order; then the tile count
    uint32_t *dTiles = excl + 2 * (nb + 1), h_tiles = 0;
    HIPCHK(zh_launch_filter_and(dFilter, n_bits, ix->live_dev.bits.as<uint32_t>(), n, ix->fl_bits.as<uint32_t>(), ix->fl_bcount.as<uint32_t>(), excl,
                                ix->fl_tmp.as<uint32_t>(), dTiles, s));
    f->cum.resize(nb + 1);
    HIPCHK(hipMemcpyAsync(f->cum.data(), excl, (nb + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_tiles, dTiles, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    f->n_allowed = f->cum[nb];
    f->tiles = h_tiles;
    const char *env_p = getenv("ZH_FILTER_PATH");
    const int forced = env_p ? atoi(env_p) : 0;
    f->path2 = forced != 1 && k && zh_exact_mfma_supported(ix->opt.dim, metric) && f->n_allowed >= std::max<uint64_t>(k, 8192);
    if (f->path2) {
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if ((rc = half_view(ix, &f->v, &f->path2))) return rc;
    }
    f->dPos = ix->fl_bits.as<uint32_t>();
    if (f->path2 && f->v.perm) {  // position p holds row perm[p]: the mask once per call in that order, counted per block of positions
        if ((rc = ix->fl_pos.ensure((n + 63) / 64 * 8))) return rc;
        HIPCHK(zh_launch_filter_permute(ix->fl_bits.as<uint32_t>(), f->v.perm, f->v.perm_rows, n, ix->fl_pos.as<uint32_t>(), ix->fl_bcount.as<uint32_t>(),
                                        excl + nb + 1, ix->fl_tmp.as<uint32_t>(), dTiles, s));
        HIPCHK(hipMemcpyAsync(f->cum.data(), excl + nb + 1, (nb + 1) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&h_tiles, dTiles, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        f->tiles = h_tiles;
        f->dPos = ix->fl_pos.as<uint32_t>();
    }
    if (f->path2 && forced != 2) {
        const uint64_t all_tiles = (n + 15) / 16;
        f->path2 = (double)(16 * f->tiles + (all_tiles - f->tiles)) <= ZH_FILTER_PATH1_ROW_COST * (double)f->n_allowed;
    }
    return f->path2 ? ZH_OK : filter_list(ix, f, s);
}

// one internal batch under a filter: path 2 where the rule chose it, path 1 over the list otherwise and for a batch whose path-2 lists ran over
static int filtered_one(zh_index *ix, ExactFilter *f, const float *dQ, uint32_t B, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys,
                        uint32_t *dCounts, hipStream_t s, zh_filtered_info *inf) {
    int rc;
    if (f->path2) {
        bool used = false, overflowed = false;
        if ((rc = exact_batch2(ix, dQ, B, k, metric, mode, dIds, dKeys, dCounts, s, &used, &overflowed, &inf->survivors, &inf->launches, f,
                               &inf->tiles_skipped)))
            return rc;
        if (used) inf->path = 2;
        if (used && !overflowed) return ZH_OK;
        if (overflowed) inf->redone++;
        if (!f->dList && (rc = filter_list(ix, f, s))) return rc;
    }
    return exact_batch(ix, f->dList, f->n_allowed, dQ, B, k, metric, mode, dIds, dKeys, dCounts, s, &inf->launches);
}

static int filtered_args(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, const uint32_t *filter, uint64_t n_bits, const void *ids,
                         const void *keys, const void *counts, const char *who) {
    int rc = exact_args(ix, q, b, k, metric, mode, ids, keys, counts, who);
    if (rc) return rc;
    if (n_bits && !filter) return fail(ZH_EINVAL, "%s: null filter for %llu rows", who, (unsigned long long)n_bits);
    return ZH_OK;
}

static int filtered_bits_fit(zh_index *ix, uint64_t n_bits) {
    if (n_bits > ix->n_rows)
        return fail(ZH_EINVAL, "filter of %llu rows for a table of %llu: made for another table?", (unsigned long long)n_bits, (unsigned long long)ix->n_rows);
    return ZH_OK;
}

static void filtered_record(zh_index *ix, size_t b, const ExactFilter &f, zh_filtered_info inf) {
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    inf.batch = b;
    inf.rows_live = ix->live_dev.n_live;
    inf.rows_allowed = f.n_allowed;
    ix->fl_info = inf;
}

// both entry points once the arguments have been judged (b > 0).  host: q, filter and the outputs are HOST arrays
static int filtered_call(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, const uint32_t *filter, uint64_t n_bits, uint64_t *out_ids,
                         uint64_t *out_keys, uint32_t *out_counts, bool host, void *stream) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = filtered_bits_fit(ix, n_bits))) return rc;
    ScratchGuard guard{ix, SCRATCH_FILTER};
    const hipStream_t s = call_stream(ix, stream);
    if (host) {
        const size_t fwords = (size_t)((n_bits + 31) / 32);
        if ((rc = exact_stage(ix, b, k)) || (rc = ix->fl_filter.ensure(std::max<size_t>(fwords, 1) * 4))) return rc;
        if (fwords) HIPCHK(hipMemcpyAsync(ix->fl_filter.p, filter, fwords * 4, hipMemcpyHostToDevice, s));  // the call's only upload besides the queries
        filter = ix->fl_filter.as<uint32_t>();
    }
    ExactFilter f;
    if ((rc = filter_prepare(ix, filter, n_bits, (uint32_t)k, metric, s, &f))) return rc;
    zh_filtered_info inf{};
    inf.path = 1;
    rc = exact_batches(ix, q, b, k, out_ids, out_keys, out_counts, host, s, [&](const float *dQ, uint32_t nb, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
        return filtered_one(ix, &f, dQ, nb, (uint32_t)k, metric, mode, dIds, dKeys, dCounts, s, &inf);
    });
    if (rc) return rc;
    filtered_record(ix, b, f, inf);
    return ZH_OK;
}

extern "C" int zh_search_exact_filtered_batch_device(zh_index *ix, const float *d_q, size_t b, size_t k, int metric, int mode, const uint32_t *d_filter,
                                                     uint64_t n_bits, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = filtered_args(ix, d_q, b, k, metric, mode, d_filter, n_bits, d_out_ids, d_out_keys, d_out_counts, "zh_search_exact_filtered_batch_device");
    if (rc || b == 0) return rc;
    return filtered_call(ix, d_q, b, k, metric, mode, d_filter, n_bits, d_out_ids, d_out_keys, d_out_counts, false, stream);
}

extern "C" int zh_search_exact_filtered_batch(zh_index *ix, const float *q, size_t b, size_t k, int metric, int mode, const uint32_t *filter,
                                              uint64_t n_bits, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = filtered_args(ix, q, b, k, metric, mode, filter, n_bits, out_ids, out_keys, out_counts, "zh_search_exact_filtered_batch");
    if (rc || b == 0) return rc;
    return filtered_call(ix, q, b, k, metric, mode, filter, n_bits, out_ids, out_keys, out_counts, true, nullptr);
}

extern "C" int zh_search_filtered_info(const zh_index *ix, zh_filtered_info *out) {
    return get_info(ix, &zh_index::fl_info, out, "zh_search_filtered_info");
}

// ------------------------------------------------------------------------------------------------
// exact range search (zh_range.hip + the exact search's scan kernels): every live row with key <= a per-query threshold key, as a CSR
// ------------------------------------------------------------------------------------------------
#define ZH_RANGE_CAND_FLOOR 4096u  // path 2: candidate slots per query that are there whatever the capacity (a count-only call still lists candidates)

struct RangeRun {
    uint64_t capacity = 0;
    uint64_t total = 0;  // hits of the internal batches so far
    bool over = false;   // they passed the capacity: the batches after count only
};

// path 1 of one internal batch: row chunk after row chunk, exact_score_kernel's keys into the key scratch, range_collect_kernel over them
static int range_batch1(zh_index *ix, const float *dQ, uint32_t B, const uint64_t *dMaxK, int metric, int mode, uint64_t pool_cap, hipStream_t s,
                        uint64_t *launches) {
    const uint32_t d = ix->opt.dim;
    const uint64_t n_live = ix->live_dev.n_live;
    const uint64_t rc_rows = std::min<uint64_t>(std::max<uint64_t>(256, ZH_EXACT_KEY_BYTES / 8 / B), n_live);
    int rc;
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_keys.ensure((size_t)B * rc_rows * 8))) return rc;
    const int param = score_param(metric, mode);
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(hipMemsetAsync(ix->rg_cnt.p, 0, (size_t)B * 4, s));
    HIPCHK(hipMemsetAsync(ix->rg_ctr.p, 0, 16, s));
    for (uint64_t p0 = 0; p0 < n_live; p0 += rc_rows) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(rc_rows, n_live - p0);
        HIPCHK(zh_launch_exact_score(ix->X.as<float>(), d, ix->live_dev.rows.as<uint32_t>(), p0, nr, dQ, ix->ex_QQ.as<float>(), B, metric, param,
                                     ix->ex_keys.as<uint64_t>(), rc_rows, s));
        HIPCHK(zh_launch_range_collect(ix->ex_keys.as<uint64_t>(), rc_rows, ix->live_dev.rows.as<uint32_t>(), p0, nr, B, dMaxK, ix->rg_cnt.as<uint32_t>(),
                                       ix->rg_ctr.as<unsigned long long>(), ix->rg_pv0.as<uint64_t>(), ix->rg_pk0.as<uint64_t>(), pool_cap, s));
        (*launches)++;
    }
    return ZH_OK;
}

// Path 2 of one internal batch: the thresholds as fixed bounds, ONE matrix-core scan of the whole table into the candidate pool, canonical keys and
// the judgement for the candidates.  *used = false: path 2 does not serve this index (path 1 answers).  On return with *used the stream has been
// waited for and h_ctr = {hits, candidates}; candidates > cand_cap: the pool ran over and nothing was counted (path 1 answers).
static int range_batch2(zh_index *ix, const float *dQ, uint32_t B, const uint64_t *dMaxK, int metric, int mode, uint64_t pool_cap, uint64_t cand_cap,
                        hipStream_t s, bool *used, unsigned long long h_ctr[2], uint64_t *launches) {
    *used = false;
    const uint32_t d = ix->opt.dim;
    if (!zh_exact_mfma_supported(d, metric) || ix->live_dev.n_live < 8192) return ZH_OK;
    int rc;
    HalfView v;
    bool have = false;
    {
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if ((rc = half_view(ix, &v, &have))) return rc;
    }
    if (!have) return ZH_OK;
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_Qh.ensure((size_t)B * d * 2)) || (rc = ix->ex_qmeta.ensure((size_t)B * 16)) ||
        (rc = ix->ex_tau.ensure((size_t)B * 4)) || (rc = ix->rg_cand.ensure(cand_cap * 8)))
        return rc;
    ZhExact2 e{v.Xh, v.rowMeta, v.perm, v.perm_rows, ix->live_dev.bits.as<uint32_t>(), ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), B, zh_approx_bound(metric, d, 1), v.rho,
               ix->ex_tau.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    unsigned long long *ctr = ix->rg_ctr.as<unsigned long long>();
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_qhalf(dQ, B, d, ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), 1, s));
    HIPCHK(zh_launch_range_tau(dMaxK, B, metric, mode, e.tau, s));
    HIPCHK(hipMemsetAsync(ix->rg_cnt.p, 0, (size_t)B * 4, s));
    HIPCHK(hipMemsetAsync(ctr, 0, 16, s));
    HIPCHK(zh_launch_range_mfma(d, metric, mode, e, 0, ix->n_rows, ix->rg_cand.as<uint64_t>(), cand_cap, ctr + 1, s));
    (*launches)++;
    HIPCHK(zh_launch_range_survivors(ix->X.as<float>(), d, dQ, ix->ex_QQ.as<float>(), metric, mode, ix->rg_cand.as<uint64_t>(), ctr + 1, cand_cap, dMaxK,
                                     ix->rg_cnt.as<uint32_t>(), ctr, ix->rg_pv0.as<uint64_t>(), ix->rg_pk0.as<uint64_t>(), pool_cap, s));
    HIPCHK(hipMemcpyAsync(h_ctr, ctr, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *used = true;
    return ZH_OK;
}

// Both range families, once an internal batch's hits are counted (rg_cnt) and pooled (rg_pv0 / rg_pk0): dOff[0 .. B] = run->total + the exclusive
// sums of the counts; and, while the capacity holds, the pool ordered by (query, key, id) into dIds / dKeys at run->total (host_out: into staging
// and from there to the HOST arrays dIds / dKeys).
static int range_emit(zh_index *ix, uint32_t B, uint64_t hits, uint64_t pool_cap, RangeRun *run, uint64_t *dOff, uint64_t *dIds, uint64_t *dKeys,
                      bool host_out, hipStream_t s) {
    int rc;
    HIPCHK(zh_launch_range_offsets(ix->rg_cnt.as<uint32_t>(), B, run->total, dOff, s));
    if (!run->over && hits > pool_cap) run->over = true;  // (pool_cap = the capacity left, or every pair there is)
    if (!run->over && hits) {
        uint64_t *dV[2] = {nullptr, nullptr}, *dK[2] = {nullptr, nullptr};
        size_t tmp_bytes = 0;
        HIPCHK(zh_launch_range_sort(dV, dK, hits, ix->n_rows, B, nullptr, &tmp_bytes, 0, nullptr, nullptr, s));
        if ((rc = ix->rg_pv1.ensure(hits * 8)) || (rc = ix->rg_pk1.ensure(hits * 8)) || (rc = ix->rg_tmp.ensure(tmp_bytes))) return rc;
        if (host_out && ((rc = ix->rg_oids.ensure(hits * 8)) || (rc = ix->rg_okeys.ensure(hits * 8)))) return rc;
        dV[0] = ix->rg_pv0.as<uint64_t>(); dV[1] = ix->rg_pv1.as<uint64_t>();
        dK[0] = ix->rg_pk0.as<uint64_t>(); dK[1] = ix->rg_pk1.as<uint64_t>();
        uint64_t *oi = host_out ? ix->rg_oids.as<uint64_t>() : dIds + run->total, *ok = host_out ? ix->rg_okeys.as<uint64_t>() : dKeys + run->total;
        HIPCHK(zh_launch_range_sort(dV, dK, hits, ix->n_rows, B, ix->rg_tmp.p, &tmp_bytes, ix->opt.id_base, oi, ok, s));
        if (host_out) {
            HIPCHK(hipMemcpyAsync(dIds + run->total, oi, hits * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(dKeys + run->total, ok, hits * 8, hipMemcpyDeviceToHost, s));
        }
    }
    run->total += hits;
    return ZH_OK;
}

// One internal batch (B <= ZH_EXACT_BATCH) on device pointers: its hits counted and pooled by path 2 where it serves, by path 1 otherwise and
// when path 2's candidates ran over; dOff[0 .. B] = run->total + the exclusive sums of the counts; and, while the capacity holds, the pool
// ordered by (query, key, id) into dIds / dKeys at run->total (host_out: into staging and from there to the HOST arrays dIds / dKeys).
static int range_one(zh_index *ix, const float *dQ, uint32_t B, const uint64_t *dMaxK, int metric, int mode, RangeRun *run, uint64_t *dOff,
                     uint64_t *dIds, uint64_t *dKeys, bool host_out, hipStream_t s, zh_range_info *inf) {
    const uint64_t n_live = ix->live_dev.n_live, pairs = (uint64_t)B * n_live;
    const uint64_t pool_cap = run->over ? 0 : std::min<uint64_t>(run->capacity - run->total, pairs);
    int rc;
    if ((rc = ix->rg_cnt.ensure((size_t)B * 4)) || (rc = ix->rg_ctr.ensure(16)) || (rc = ix->rg_pv0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)) ||
        (rc = ix->rg_pk0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)))
        return rc;
    unsigned long long h_ctr[2] = {0, 0};
    if (n_live == 0) HIPCHK(hipMemsetAsync(ix->rg_cnt.p, 0, (size_t)B * 4, s));
    else {
        const char *env_p = getenv("ZH_RANGE_PATH");
        bool done = false;
        if (!(env_p && atoi(env_p) == 1)) {
            const uint64_t cand_cap = std::min<uint64_t>(pairs, std::max<uint64_t>(pool_cap + pool_cap / 4, (uint64_t)ZH_RANGE_CAND_FLOOR * B));
            bool used = false;
            if ((rc = range_batch2(ix, dQ, B, dMaxK, metric, mode, pool_cap, cand_cap, s, &used, h_ctr, &inf->launches))) return rc;
            if (used) {
                inf->path = 2;
                if (h_ctr[1] > cand_cap) inf->redone++;
                else { inf->candidates += h_ctr[1]; done = true; }
            }
        }
        if (!done) {
            if ((rc = range_batch1(ix, dQ, B, dMaxK, metric, mode, pool_cap, s, &inf->launches))) return rc;
            HIPCHK(hipMemcpyAsync(h_ctr, ix->rg_ctr.p, 16, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    if ((rc = range_emit(ix, B, h_ctr[0], pool_cap, run, dOff, dIds, dKeys, host_out, s))) return rc;
    inf->hits += h_ctr[0];
    return ZH_OK;
}

static int range_args(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, int metric, int mode, uint64_t capacity, const void *offsets,
                      const void *ids, const void *keys, const void *total, const char *who) {
    int rc = exact_args(ix, q, b, capacity ? 1 : 0, metric, mode, ids, keys, offsets, who);
    if (rc) return rc;
    if (!offsets || !total || (b && !max_keys) || (capacity && (!ids || !keys))) return fail(ZH_EINVAL, "%s: null argument", who);
    return ZH_OK;
}

static int range_finish(zh_index *ix, size_t b, const RangeRun &run, zh_range_info inf, const char *who) {
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        inf.batch = b;
        inf.rows_live = ix->live_dev.n_live;
        ix->rg_info = inf;
    }
    if (run.over)
        return fail(ZH_ELIMIT, "%s: %llu hits exceed the capacity of %llu; out_total and the offsets are exact, call again with that capacity", who,
                    (unsigned long long)run.total, (unsigned long long)run.capacity);
    return ZH_OK;
}

// Both range families' loop over internal batches of at most ZH_EXACT_BATCH queries; one(dQ, nb, dMaxK, dOff) answers a batch on device pointers
// (range_one / frange_one: nb + 1 offsets at dOff).  host: q, max_keys and out_offsets are HOST arrays -- each batch goes through the staging
// (ex_Q, rg_maxk, rg_off) and is waited for; otherwise they are device arrays and the caller waits once, after the total (put_total).
template <typename One>
static int range_batches(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, uint64_t *out_offsets, bool host, hipStream_t s, One one) {
    const size_t nb_max = std::min<size_t>(ZH_EXACT_BATCH, b), d = ix->opt.dim;
    int rc;
    if (host && ((rc = ix->ex_Q.ensure(nb_max * d * 4)) || (rc = ix->rg_maxk.ensure(nb_max * 8)) || (rc = ix->rg_off.ensure((nb_max + 1) * 8)))) return rc;
    for (size_t b0 = 0; b0 < b; b0 += ZH_EXACT_BATCH) {
        const uint32_t nb = (uint32_t)std::min<size_t>(ZH_EXACT_BATCH, b - b0);
        if (!host) {
            if ((rc = one(q + b0 * d, nb, max_keys + b0, out_offsets + b0))) return rc;
            continue;
        }
        HIPCHK(hipMemcpyAsync(ix->ex_Q.p, q + b0 * d, (size_t)nb * d * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ix->rg_maxk.p, max_keys + b0, (size_t)nb * 8, hipMemcpyHostToDevice, s));
        if ((rc = one(ix->ex_Q.as<float>(), nb, ix->rg_maxk.as<uint64_t>(), ix->rg_off.as<uint64_t>()))) return rc;
        HIPCHK(hipMemcpyAsync(out_offsets + b0, ix->rg_off.p, ((size_t)nb + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return ZH_OK;
}

// A call's total to its caller: *out_total on the host; otherwise over the stream into device memory, and the call's one wait (`total` is this
// frame's until then).
static int put_total(uint64_t total, uint64_t *out_total, bool host, hipStream_t s) {
    if (host) {
        *out_total = total;
        return ZH_OK;
    }
    HIPCHK(hipMemcpyAsync(out_total, &total, 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

// both entry points once the arguments have been judged.  host: b > 0, and the caller has zeroed out_offsets[0] and the total; the device call
// comes here with b == 0 too and zeroes them on its stream
static int range_call(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, int metric, int mode, uint64_t capacity, uint64_t *out_offsets,
                      uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    ScratchGuard guard{ix, SCRATCH_RANGE};
    const hipStream_t s = call_stream(ix, stream);
    RangeRun run;
    run.capacity = capacity;
    zh_range_info inf{};
    inf.path = 1;
    if (!host) HIPCHK(hipMemsetAsync(out_offsets, 0, 8, s));
    rc = range_batches(ix, q, b, max_keys, out_offsets, host, s, [&](const float *dQ, uint32_t nb, const uint64_t *dMaxK, uint64_t *dOff) {
        return range_one(ix, dQ, nb, dMaxK, metric, mode, &run, dOff, out_ids, out_keys, host, s, &inf);
    });
    if (rc || (rc = put_total(run.total, out_total, host, s))) return rc;
    return range_finish(ix, b, run, inf, who);
}

extern "C" int zh_search_range_batch_device(zh_index *ix, const float *d_q, size_t b, const uint64_t *d_max_keys, int metric, int mode, uint64_t capacity,
                                            uint64_t *d_out_offsets, uint64_t *d_out_ids, uint64_t *d_out_keys, uint64_t *d_out_total, void *stream) {
    const char *who = "zh_search_range_batch_device";
    int rc = range_args(ix, d_q, b, d_max_keys, metric, mode, capacity, d_out_offsets, d_out_ids, d_out_keys, d_out_total, who);
    if (rc) return rc;
    return range_call(ix, d_q, b, d_max_keys, metric, mode, capacity, d_out_offsets, d_out_ids, d_out_keys, d_out_total, false, stream, who);
}

extern "C" int zh_search_range_batch(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, int metric, int mode, uint64_t capacity,
                                     uint64_t *out_offsets, uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total) {
    const char *who = "zh_search_range_batch";
    int rc = range_args(ix, q, b, max_keys, metric, mode, capacity, out_offsets, out_ids, out_keys, out_total, who);
    if (rc) return rc;
    out_offsets[0] = 0;
    *out_total = 0;
    if (b == 0) return ZH_OK;
    return range_call(ix, q, b, max_keys, metric, mode, capacity, out_offsets, out_ids, out_keys, out_total, true, nullptr, who);
}

extern "C" int zh_search_range_info(const zh_index *ix, zh_range_info *out) { return get_info(ix, &zh_index::rg_info, out, "zh_search_range_info"); }

// ------------------------------------------------------------------------------------------------
// exact self-join (zh_join.hip + the exact search's score kernel): every pair of live rows a < b with key(stored b, query a) <= one threshold key,
// as three arrays ascending by (a, key, b).  DESIGN.md s15
// ------------------------------------------------------------------------------------------------
#define ZH_JOIN_CAND_FLOOR 256u  // path 2: candidate slots per held row of a panel that are there whatever the capacity (a count-only call still lists candidates)

// Path 1 of the self-join and the cross-join, for the B <= ZH_EXACT_BATCH query rows dQRows (row numbers of iq, device) against the stored rows of
// `is` (the self-join: iq itself): gathered out of iq's table into iq's query buffer, exact_score_kernel's keys of is's live rows from position
// p_from of its ascending live list on, pair_collect_kernel over them.  upper (the self-join): only the rows above the query row count, and no live
// row before p_from is above any of the query rows; the cross-join takes every live row of is.  Hits are counted in iq's jn_ctr[0] and pooled there
// while the pool has room.
static int pair_batch1(zh_index *iq, zh_index *is, const uint32_t *dQRows, uint32_t B, uint64_t p_from, bool upper, uint64_t max_key, int metric, int mode,
                       uint64_t pool_cap, hipStream_t s, uint64_t *launches) {
    const uint32_t d = iq->opt.dim;
    const uint64_t n_live = is->live_dev.n_live;
    if (!B || p_from >= n_live) return ZH_OK;
    const uint64_t rc_rows = std::min<uint64_t>(std::max<uint64_t>(256, ZH_EXACT_KEY_BYTES / 8 / B), n_live - p_from);
    int rc;
    if ((rc = iq->ex_Q.ensure((size_t)B * d * 4)) || (rc = iq->ex_QQ.ensure((size_t)B * 4)) || (rc = iq->ex_keys.ensure((size_t)B * rc_rows * 8))) return rc;
    const int param = score_param(metric, mode);
    HIPCHK(zh_launch_join_gather(iq->X.as<float>(), d, dQRows, B, iq->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(iq->ex_Q.as<float>(), B, d, iq->ex_QQ.as<float>(), s));
    for (uint64_t p0 = p_from; p0 < n_live; p0 += rc_rows) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(rc_rows, n_live - p0);
        HIPCHK(zh_launch_exact_score(is->X.as<float>(), d, is->live_dev.rows.as<uint32_t>(), p0, nr, iq->ex_Q.as<float>(), iq->ex_QQ.as<float>(), B, metric, param,
                                     iq->ex_keys.as<uint64_t>(), rc_rows, s));
        HIPCHK(zh_launch_pair_collect(iq->ex_keys.as<uint64_t>(), rc_rows, is->live_dev.rows.as<uint32_t>(), p0, nr, dQRows, B, upper, max_key,
                                      iq->jn_ctr.as<unsigned long long>(), iq->jn_pv0.as<uint64_t>(), iq->jn_pk0.as<uint64_t>(), pool_cap, s));
        (*launches)++;
    }
    return ZH_OK;
}

// The tail of a path-2 panel (the forest join: batch of leaves) whose survivors are launched: the first n counters of jn_ctr -- {hits, the panel's
// candidates, ...} -- are read into h_ctr and waited for.  *kept: the candidates fitted their pool and were judged, *hits = the hits so far.
// Otherwise nothing of the panel was counted and ++*redone; what answers it instead is the caller's, because it differs: a whole-call rewind under
// a row order, a panel redo, a leaf redo.
static int panel_tail(zh_index *ix, uint32_t n, uint64_t cand_cap, hipStream_t s, unsigned long long *h_ctr, uint64_t *hits, uint32_t *redone, bool *kept) {
    HIPCHK(hipMemcpyAsync(h_ctr, ix->jn_ctr.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *kept = h_ctr[1] <= cand_cap;
    if (*kept) *hits = h_ctr[0];
    else (*redone)++;
    return ZH_OK;
}

// Path 2 of the whole call: the threshold as a fixed bound, the copy's rows as approx_interval's queries, then panel after panel of
// ZH_JOIN_PANEL_ROWS held positions: one matrix-core launch over the panel's blocks on or above the diagonal, canonical keys and the judgement for
// its candidates.  A panel whose candidates outgrow the pool (nothing of it was counted) is answered by path 1 from its rows' list -- in id order;
// under a row order the first such panel ends path 2 and the whole call is answered by path 1.  *used = false: path 2 does not serve this index,
// or was given up (inf->path says 2 then): nothing is counted or pooled and path 1 answers everything.  *hits = jn_ctr[0] on return with *used.
static int join_path2(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t pool_cap, hipStream_t s, zh_join_info *inf, bool *used, uint64_t *hits) {
    *used = false;
    const uint32_t d = ix->opt.dim;
    if (!zh_exact_mfma_supported(d, metric) || ix->live_dev.n_live < 8192) return ZH_OK;
    int rc;
    HalfView v;
    bool have = false;
    {
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if ((rc = half_view(ix, &v, &have))) return rc;
    }
    if (!have) return ZH_OK;
    const uint64_t n = ix->n_rows, T = (n + 15) / 16, n_pos = T * 16;
    const uint32_t n_ab_max = ZH_JOIN_PANEL_ROWS / 64;
    if ((rc = ix->jn_qm.ensure(n_pos * 16)) || (rc = ix->jn_cid.ensure(n_pos * 4)) || (rc = ix->jn_tau.ensure(4)) || (rc = ix->jn_maxk.ensure(8)) ||
        (rc = ix->jn_first.ensure((n_ab_max + 1) * 4)))
        return rc;
    unsigned long long *ctr = ix->jn_ctr.as<unsigned long long>();  // {hits, the panel's candidates, a redone panel's rows}
    HIPCHK(hipMemcpyAsync(ix->jn_maxk.p, &max_key, 8, hipMemcpyHostToDevice, s));
    HIPCHK(zh_launch_range_tau(ix->jn_maxk.as<uint64_t>(), 1, metric, mode, ix->jn_tau.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_prep(v.rowMeta, v.perm, v.perm_rows, ix->live_dev.bits.as<uint32_t>(), n, v.rho, ix->jn_qm.as<float4>(), ix->jn_cid.as<uint32_t>(), s));
    HIPCHK(hipStreamSynchronize(s));  // (max_key is the caller's stack)
    *used = true;
    inf->path = 2;
    const float Kc = zh_approx_bound(metric, d, 1);
    std::vector<uint32_t> first(n_ab_max + 1);
    LiveCursor live;  // (id order: a redone panel's first chunk)
    for (uint64_t P0 = 0; P0 < n; P0 += ZH_JOIN_PANEL_ROWS) {
        const uint64_t P1 = std::min<uint64_t>(n, P0 + ZH_JOIN_PANEL_ROWS), tileA0 = P0 / 16, tileA1 = (P1 + 15) / 16;
        const uint32_t n_ab = (uint32_t)((tileA1 - tileA0 + 3) / 4);
        const uint64_t products = zh_join_geometry(T, tileA0, tileA1, first.data());
        const uint64_t panel_rows = P1 - P0, pairs_bound = panel_rows * (n - P0), pool_left = pool_cap > *hits ? pool_cap - *hits : 0;
        const uint64_t cand_cap = std::min<uint64_t>(pairs_bound, std::max<uint64_t>(pool_left + pool_left / 4, (uint64_t)ZH_JOIN_CAND_FLOOR * panel_rows));
        if ((rc = ix->jn_cand.ensure(cand_cap * 8))) return rc;
        HIPCHK(hipMemcpyAsync(ix->jn_first.p, first.data(), ((size_t)n_ab + 1) * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(ctr + 1, 0, 16, s));
        HIPCHK(zh_launch_join_mfma(d, metric, mode, v.Xh, v.rowMeta, ix->jn_qm.as<float4>(), ix->jn_cid.as<uint32_t>(), n, tileA0, ix->jn_first.as<uint32_t>(), n_ab,
                                   first[n_ab], Kc, v.rho, ix->jn_tau.as<uint32_t>(), ix->jn_cand.as<uint64_t>(), cand_cap, ctr + 1, s));
        inf->launches++;
        inf->tiles += products;
        HIPCHK(zh_launch_pair_survivors(ix->X.as<float>(), ix->X.as<float>(), d, metric, mode, ix->jn_cand.as<uint64_t>(), ctr + 1, cand_cap, nullptr, 0, 0,
                                        max_key, ctr, nullptr, ix->jn_pv0.as<uint64_t>(), ix->jn_pk0.as<uint64_t>(), pool_cap, s));
        unsigned long long h_ctr[3] = {0, 0, 0};
        bool kept = false;
        if ((rc = panel_tail(ix, 3, cand_cap, s, h_ctr, hits, &inf->redone, &kept))) return rc;
        if (kept) {
            inf->candidates += h_ctr[1];
            continue;
        }
        if (v.perm_rows) {
            // Under a row order a panel owns its pairs by POSITION (the lower position lies in it), and path 1 owns pairs by row number: the
            // redo below would count a different set.  So nothing of path 2 is kept: counters and pool rewound, the whole call answered by path 1.
            HIPCHK(hipMemsetAsync(ctr, 0, 32, s));
            inf->candidates = 0;
            *hits = 0;
            *used = false;
            return ZH_OK;
        }
        if ((rc = ix->jn_rows.ensure(panel_rows * 4))) return rc;
        HIPCHK(zh_launch_join_panel_rows(ix->jn_cid.as<uint32_t>(), P0, P1, ix->jn_rows.as<uint32_t>(), ctr + 2, s));
        HIPCHK(hipMemcpyAsync(h_ctr, ctr, 24, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // positions are row numbers here: the panel's pairs by position are its pairs by row number, and the live rows before the panel are
        // below every row of it
        const uint64_t p_from = live_before(ix, P0, &live);
        for (uint64_t b0 = 0; b0 < h_ctr[2]; b0 += ZH_EXACT_BATCH) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(ZH_EXACT_BATCH, h_ctr[2] - b0);
            if ((rc = pair_batch1(ix, ix, ix->jn_rows.as<uint32_t>() + b0, nb, p_from, true, max_key, metric, mode, pool_cap, s, &inf->launches))) return rc;
        }
        HIPCHK(hipMemcpyAsync(h_ctr, ctr, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *hits = h_ctr[0];
    }
    return ZH_OK;
}

static int join_args(zh_index *ix, int metric, int mode, uint64_t capacity, const void *a, const void *b, const void *keys, const void *total,
                     const char *who) {
    if (!ix || !total || (capacity && (!a || !b || !keys))) return fail(ZH_EINVAL, "%s: null argument", who);
    return check_metric(metric, mode);
}

// What the three joins do once the hits are pooled in ix's jn_pv0 / jn_pk0 and counted: *total = hits, exact whatever the capacity; within it, the pool
// ordered into outA / outB / outKeys (host_out: HOST arrays, filled through staging; otherwise device arrays) and waited for; the info written into
// ix's slot; ZH_ELIMIT past the capacity.  ib = the index the b side's rows are numbered in and whose id base they get: ix itself but for the
// cross-join.
template <typename Info>
static int join_finish(zh_index *ix, const zh_index *ib, uint64_t hits, uint64_t capacity, uint64_t *outA, uint64_t *outB, uint64_t *outKeys, bool host_out,
                       hipStream_t s, uint64_t *total, Info inf, Info zh_index::*slot, const char *who) {
    *total = hits;
    inf.pairs = hits;
    const bool over = hits > capacity;
    int rc;
    if (!over && hits) {
        uint64_t *dV[2] = {nullptr, nullptr}, *dK[2] = {nullptr, nullptr};
        size_t tmp_bytes = 0;
        HIPCHK(zh_launch_pair_sort(dV, dK, hits, ix->n_rows, ib->n_rows, nullptr, &tmp_bytes, 0, 0, nullptr, nullptr, nullptr, s));
        if ((rc = ix->jn_pv1.ensure(hits * 8)) || (rc = ix->jn_pk1.ensure(hits * 8)) || (rc = ix->jn_tmp.ensure(tmp_bytes))) return rc;
        if (host_out && ((rc = ix->jn_oa.ensure(hits * 8)) || (rc = ix->jn_ob.ensure(hits * 8)) || (rc = ix->jn_okeys.ensure(hits * 8)))) return rc;
        dV[0] = ix->jn_pv0.as<uint64_t>(); dV[1] = ix->jn_pv1.as<uint64_t>();
        dK[0] = ix->jn_pk0.as<uint64_t>(); dK[1] = ix->jn_pk1.as<uint64_t>();
        uint64_t *oa = host_out ? ix->jn_oa.as<uint64_t>() : outA, *ob = host_out ? ix->jn_ob.as<uint64_t>() : outB;
        uint64_t *ok = host_out ? ix->jn_okeys.as<uint64_t>() : outKeys;
        HIPCHK(zh_launch_pair_sort(dV, dK, hits, ix->n_rows, ib->n_rows, ix->jn_tmp.p, &tmp_bytes, ix->opt.id_base, ib->opt.id_base, oa, ob, ok, s));
        if (host_out) {
            HIPCHK(hipMemcpyAsync(outA, oa, hits * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(outB, ob, hits * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(outKeys, ok, hits * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
    }
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->*slot = inf;
    }
    if (over)
        return fail(ZH_ELIMIT, "%s: %llu pairs exceed the capacity of %llu; out_total is exact, call again with that capacity", who,
                    (unsigned long long)hits, (unsigned long long)capacity);
    return ZH_OK;
}

// How the three joins' entry points end, rc being their *_run's: past the capacity (ZH_ELIMIT) the total still goes to the caller, as put_total does it.
static int join_total(int rc, uint64_t total, uint64_t *out_total, bool host, hipStream_t s) {
    if (rc && rc != ZH_ELIMIT) return rc;
    const int rt = put_total(total, out_total, host, s);
    return rt ? rt : rc;
}

// The call on the index's device (under mu, exclusive; exact_live_rows has run).  host_out: outA / outB / outKeys are HOST arrays, filled through
// staging; otherwise device arrays.  *total = the pairs, exact whatever the capacity.
static int join_run(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *outA, uint64_t *outB, uint64_t *outKeys, bool host_out,
                    hipStream_t s, uint64_t *total, const char *who) {
    zh_join_info inf{};
    inf.path = 1;
    inf.rows_live = ix->live_dev.n_live;
    const uint64_t n_live = ix->live_dev.n_live;
    uint64_t hits = 0;
    int rc;
    if (n_live >= 2) {
        const uint64_t pool_cap = std::min<uint64_t>(capacity, n_live * (n_live - 1) / 2);
        if ((rc = ix->jn_ctr.ensure(32)) || (rc = ix->jn_pv0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)) ||
            (rc = ix->jn_pk0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)))
            return rc;
        HIPCHK(hipMemsetAsync(ix->jn_ctr.p, 0, 32, s));
        const char *env_p = getenv("ZH_JOIN_PATH");
        bool used = false;
        if (!(env_p && atoi(env_p) == 1) && (rc = join_path2(ix, max_key, metric, mode, pool_cap, s, &inf, &used, &hits))) return rc;
        if (!used) {  // panels of the ascending live list: panel [a0, a0 + B) against the live rows from a0 on
            for (uint64_t a0 = 0; a0 + 1 < n_live; a0 += ZH_EXACT_BATCH) {
                const uint32_t B = (uint32_t)std::min<uint64_t>(ZH_EXACT_BATCH, n_live - a0);
                if ((rc = pair_batch1(ix, ix, ix->live_dev.rows.as<uint32_t>() + a0, B, a0, true, max_key, metric, mode, pool_cap, s, &inf.launches))) return rc;
            }
            unsigned long long h = 0;
            HIPCHK(hipMemcpyAsync(&h, ix->jn_ctr.p, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            hits = h;
        }
    }
    return join_finish(ix, ix, hits, capacity, outA, outB, outKeys, host_out, s, total, inf, &zh_index::jn_info, who);
}

// both entry points once the arguments have been judged (host: the caller has zeroed the total)
static int join_call(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b, uint64_t *out_keys,
                     uint64_t *out_total, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    ScratchGuard guard{ix, SCRATCH_JOIN};
    const hipStream_t s = call_stream(ix, stream);
    uint64_t total = 0;
    rc = join_run(ix, max_key, metric, mode, capacity, out_a, out_b, out_keys, host, s, &total, who);
    return join_total(rc, total, out_total, host, s);
}

extern "C" int zh_self_join_device(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *d_out_a, uint64_t *d_out_b,
                                   uint64_t *d_out_keys, uint64_t *d_out_total, void *stream) {
    int rc = join_args(ix, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, "zh_self_join_device");
    if (rc) return rc;
    return join_call(ix, max_key, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, false, stream, "zh_self_join_device");
}

extern "C" int zh_self_join(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b, uint64_t *out_keys,
                            uint64_t *out_total) {
    int rc = join_args(ix, metric, mode, capacity, out_a, out_b, out_keys, out_total, "zh_self_join");
    if (rc) return rc;
    *out_total = 0;
    return join_call(ix, max_key, metric, mode, capacity, out_a, out_b, out_keys, out_total, true, nullptr, "zh_self_join");
}

extern "C" int zh_self_join_info(const zh_index *ix, zh_join_info *out) { return get_info(ix, &zh_index::jn_info, out, "zh_self_join_info"); }

// ------------------------------------------------------------------------------------------------
// exact join between two indexes (zh_xjoin.hip, the self-join's pool and the exact search's score kernel): every pair (live row a of A, live row
// b of B) with key(stored b of B, query a of A) <= one threshold key, as three arrays ascending by (a, key, b).  All scratch and the info on A.
// DESIGN.md s20
// ------------------------------------------------------------------------------------------------
#define ZH_XJOIN_GATE_PAIRS (uint64_t(1) << 25)  // live(A) x live(B) from which path 2 is taken: the pair work at which the self-join switches (8192^2 / 2)

// Path 2 of the whole call: the threshold as a fixed bound, either side's positions through zh_launch_join_prep (A's id word; B's id word and its
// rows as approx_interval's queries, with B's rho), then panel after panel of ZH_JOIN_PANEL_ROWS positions of A's copy: one matrix-core launch of
// the panel against all of B's copy, canonical keys and the judgement for its candidates.  A panel whose candidates outgrow the pool (nothing of
// it was counted) is answered by path 1 from the list of its live rows, against all of B.  That redo is valid under a row order of either side
// too, unlike the self-join's: a panel owns the pairs (a, b) of the A rows at its positions, whatever those rows' numbers and wherever b sits in
// B's copy, and path 1 for exactly those A rows against every live b is the same set -- no pair of the rectangle belongs to two panels, none to a
// panel by anything but its A row, so no whole-call rewind is needed.  *used = false: path 2 does not serve this pair of indexes and path 1
// answers everything.  *hits = jn_ctr[0] on return with *used.
static int xjoin_path2(zh_index *ia, zh_index *ib, bool forced, uint64_t max_key, int metric, int mode, uint64_t pool_cap, hipStream_t s, zh_cross_info *inf,
                       bool *used, uint64_t *hits) {
    *used = false;
    const uint32_t d = ia->opt.dim;
    if (!zh_exact_mfma_supported(d, metric)) return ZH_OK;
    if (!forced && ia->live_dev.n_live * ib->live_dev.n_live < ZH_XJOIN_GATE_PAIRS) return ZH_OK;  // (both counts are below 2^32)
    int rc;
    HalfView va, vb;
    bool have_a = false, have_b = false;
    {
        std::lock_guard<std::mutex> lb(ia->blk_mu);
        if ((rc = half_view(ia, &va, &have_a))) return rc;
    }
    if (!have_a) return ZH_OK;
    {
        std::lock_guard<std::mutex> lb(ib->blk_mu);
        if ((rc = half_view(ib, &vb, &have_b))) return rc;  // (a copy made now is complete on return: ensure_row_half waits for ib's stream)
    }
    if (!have_b) return ZH_OK;
    const uint64_t na = ia->n_rows, nb = ib->n_rows, TA = (na + 15) / 16, TB = (nb + 15) / 16;
    if ((rc = ia->xj_qma.ensure(TA * 16 * 16)) || (rc = ia->xj_cida.ensure(TA * 16 * 4)) || (rc = ia->xj_qmb.ensure(TB * 16 * 16)) ||
        (rc = ia->xj_cidb.ensure(TB * 16 * 4)) || (rc = ia->jn_tau.ensure(4)) || (rc = ia->jn_maxk.ensure(8)))
        return rc;
    unsigned long long *ctr = ia->jn_ctr.as<unsigned long long>();  // {hits, the panel's candidates, a redone panel's rows}
    HIPCHK(hipMemcpyAsync(ia->jn_maxk.p, &max_key, 8, hipMemcpyHostToDevice, s));
    HIPCHK(zh_launch_range_tau(ia->jn_maxk.as<uint64_t>(), 1, metric, mode, ia->jn_tau.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_prep(va.rowMeta, va.perm, va.perm_rows, ia->live_dev.bits.as<uint32_t>(), na, va.rho, ia->xj_qma.as<float4>(), ia->xj_cida.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_prep(vb.rowMeta, vb.perm, vb.perm_rows, ib->live_dev.bits.as<uint32_t>(), nb, vb.rho, ia->xj_qmb.as<float4>(), ia->xj_cidb.as<uint32_t>(), s));
    HIPCHK(hipStreamSynchronize(s));  // (max_key is the caller's stack)
    *used = true;
    inf->path = 2;
    const float Kc = zh_approx_bound(metric, d, 1);
    for (uint64_t P0 = 0; P0 < na; P0 += ZH_JOIN_PANEL_ROWS) {
        const uint64_t P1 = std::min<uint64_t>(na, P0 + ZH_JOIN_PANEL_ROWS), tileA0 = P0 / 16, tileA1 = (P1 + 15) / 16;
        uint32_t n_ab = 0, blocks = 0;
        const uint64_t products = zh_xjoin_geometry(TA, TB, tileA0, tileA1, &n_ab, &blocks);
        const uint64_t panel_rows = P1 - P0, pairs_bound = panel_rows * nb, pool_left = pool_cap > *hits ? pool_cap - *hits : 0;
        const uint64_t cand_cap = std::min<uint64_t>(pairs_bound, std::max<uint64_t>(pool_left + pool_left / 4, (uint64_t)ZH_JOIN_CAND_FLOOR * panel_rows));
        if ((rc = ia->jn_cand.ensure(cand_cap * 8))) return rc;
        HIPCHK(hipMemsetAsync(ctr + 1, 0, 16, s));
        HIPCHK(zh_launch_xjoin_mfma(d, metric, mode, va.Xh, va.rowMeta, ia->xj_cida.as<uint32_t>(), na, vb.Xh, ia->xj_qmb.as<float4>(), ia->xj_cidb.as<uint32_t>(),
                                    nb, tileA0, tileA1, Kc, va.rho, ia->jn_tau.as<uint32_t>(), ia->jn_cand.as<uint64_t>(), cand_cap, ctr + 1, s));
        inf->launches++;
        inf->tiles += products;
        HIPCHK(zh_launch_pair_survivors(ia->X.as<float>(), ib->X.as<float>(), d, metric, mode, ia->jn_cand.as<uint64_t>(), ctr + 1, cand_cap, nullptr, 0, 0,
                                        max_key, ctr, nullptr, ia->jn_pv0.as<uint64_t>(), ia->jn_pk0.as<uint64_t>(), pool_cap, s));
        unsigned long long h_ctr[3] = {0, 0, 0};
        bool kept = false;
        if ((rc = panel_tail(ia, 3, cand_cap, s, h_ctr, hits, &inf->redone, &kept))) return rc;
        if (kept) {
            inf->candidates += h_ctr[1];
            continue;
        }
        if ((rc = ia->jn_rows.ensure(panel_rows * 4))) return rc;
        HIPCHK(zh_launch_join_panel_rows(ia->xj_cida.as<uint32_t>(), P0, P1, ia->jn_rows.as<uint32_t>(), ctr + 2, s));
        HIPCHK(hipMemcpyAsync(h_ctr, ctr, 24, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint64_t b0 = 0; b0 < h_ctr[2]; b0 += ZH_EXACT_BATCH) {
            const uint32_t nq = (uint32_t)std::min<uint64_t>(ZH_EXACT_BATCH, h_ctr[2] - b0);
            if ((rc = pair_batch1(ia, ib, ia->jn_rows.as<uint32_t>() + b0, nq, 0, false, max_key, metric, mode, pool_cap, s, &inf->launches))) return rc;
        }
        HIPCHK(hipMemcpyAsync(h_ctr, ctr, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *hits = h_ctr[0];
    }
    return ZH_OK;
}

// judged before any device is touched (and before either handle is followed)
static int xjoin_args(const zh_index *ia, const zh_index *ib, int metric, int mode, uint64_t capacity, const void *a, const void *b, const void *keys,
                      const void *total, const char *who) {
    if (!ia || !ib) return fail(ZH_EINVAL, "%s: null argument", who);
    if (ia == ib) return fail(ZH_EINVAL, "%s: the two indexes are the same one; zh_self_join joins an index with itself", who);
    if (!total || (capacity && (!a || !b || !keys))) return fail(ZH_EINVAL, "%s: null argument", who);
    return check_metric(metric, mode);
}

// Both indexes' mu, exclusively (exact_live_rows and half_view re-make caches on either side), taken with std::lock: its try-and-back-off takes the
// two in no fixed order and holds neither while it waits for the other, so zh_cross_join(A, B) and zh_cross_join(B, A) on two threads cannot
// deadlock.  Then what can only be judged under the locks.
struct XjoinLocks {
    std::unique_lock<std::shared_mutex> la, lb;
    XjoinLocks(zh_index *ia, zh_index *ib) : la(ia->mu, std::defer_lock), lb(ib->mu, std::defer_lock) { std::lock(la, lb); }
};
static int xjoin_state(zh_index *ia, zh_index *ib, const char *who) {
    if (ia->opt.dim != ib->opt.dim) return fail(ZH_EINVAL, "%s: the indexes have different dim (%u and %u)", who, ia->opt.dim, ib->opt.dim);
    if (ia->device != ib->device) return fail(ZH_EINVAL, "%s: the indexes live on different devices (%d and %d)", who, ia->device, ib->device);
    int rc;
    if ((rc = set_device(ia)) || (rc = exact_live_rows(ia)) || (rc = exact_live_rows(ib))) return rc;
    return ZH_OK;
}

// The call on the indexes' device (under both mu, exclusive; xjoin_state has run).  host_out as join_run.  ZH_XJOIN_PATH (read per call): 1 keeps
// everything on path 1, 2 takes path 2 at any size where it is supported.
static int xjoin_run(zh_index *ia, zh_index *ib, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *outA, uint64_t *outB, uint64_t *outKeys,
                     bool host_out, hipStream_t s, uint64_t *total, const char *who) {
    zh_cross_info inf{};
    inf.path = 1;
    inf.rows_live_a = ia->live_dev.n_live;
    inf.rows_live_b = ib->live_dev.n_live;
    const uint64_t la = ia->live_dev.n_live, lb = ib->live_dev.n_live;
    uint64_t hits = 0;
    int rc;
    if (la && lb) {
        const uint64_t pool_cap = std::min<uint64_t>(capacity, la * lb);
        if ((rc = ia->jn_ctr.ensure(32)) || (rc = ia->jn_pv0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)) ||
            (rc = ia->jn_pk0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)))
            return rc;
        HIPCHK(hipMemsetAsync(ia->jn_ctr.p, 0, 32, s));
        const char *env_p = getenv("ZH_XJOIN_PATH");
        const int env_path = env_p ? atoi(env_p) : 0;
        bool used = false;
        if (env_path != 1 && (rc = xjoin_path2(ia, ib, env_path == 2, max_key, metric, mode, pool_cap, s, &inf, &used, &hits))) return rc;
        if (!used) {  // panels of A's ascending live list against all of B's
            for (uint64_t a0 = 0; a0 < la; a0 += ZH_EXACT_BATCH) {
                const uint32_t B = (uint32_t)std::min<uint64_t>(ZH_EXACT_BATCH, la - a0);
                if ((rc = pair_batch1(ia, ib, ia->live_dev.rows.as<uint32_t>() + a0, B, 0, false, max_key, metric, mode, pool_cap, s, &inf.launches))) return rc;
            }
            unsigned long long h = 0;
            HIPCHK(hipMemcpyAsync(&h, ia->jn_ctr.p, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            hits = h;
        }
    }
    return join_finish(ia, ib, hits, capacity, outA, outB, outKeys, host_out, s, total, inf, &zh_index::xj_info, who);
}

// both entry points once the arguments have been judged (host: the caller has zeroed the total)
static int xjoin_call(zh_index *ia, zh_index *ib, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b,
                      uint64_t *out_keys, uint64_t *out_total, bool host, void *stream, const char *who) {
    XjoinLocks locks(ia, ib);
    int rc = xjoin_state(ia, ib, who);
    if (rc) return rc;
    ScratchGuard guard{ia, SCRATCH_XJOIN};
    const hipStream_t s = call_stream(ia, stream);
    uint64_t total = 0;
    rc = xjoin_run(ia, ib, max_key, metric, mode, capacity, out_a, out_b, out_keys, host, s, &total, who);
    return join_total(rc, total, out_total, host, s);
}

extern "C" int zh_cross_join_device(zh_index *ia, zh_index *ib, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *d_out_a,
                                    uint64_t *d_out_b, uint64_t *d_out_keys, uint64_t *d_out_total, void *stream) {
    int rc = xjoin_args(ia, ib, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, "zh_cross_join_device");
    if (rc) return rc;
    return xjoin_call(ia, ib, max_key, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, false, stream, "zh_cross_join_device");
}

extern "C" int zh_cross_join(zh_index *ia, zh_index *ib, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b,
                             uint64_t *out_keys, uint64_t *out_total) {
    int rc = xjoin_args(ia, ib, metric, mode, capacity, out_a, out_b, out_keys, out_total, "zh_cross_join");
    if (rc) return rc;
    *out_total = 0;
    return xjoin_call(ia, ib, max_key, metric, mode, capacity, out_a, out_b, out_keys, out_total, true, nullptr, "zh_cross_join");
}

extern "C" int zh_cross_join_info(const zh_index *ia, zh_cross_info *out) { return get_info(ia, &zh_index::xj_info, out, "zh_cross_join_info"); }

// ---- test / debug access (include/zebra_hip.h): the held-tile walk's interval of every pair of a slab of `ia`'s positions x all of `ib`'s, through
// the inputs path 2 of the joins prepares and by the host functions it prepares them with -- the copy's view, zh_launch_join_prep per side,
// zh_approx_bound(metric, d, 1), the held side's rho -- and the walk itself under a recording sink (zh_walkdbg.hip).  ia == ib: the self-join's view
extern "C" int zh_debug_walk_pairs(zh_index *ia, zh_index *ib, int metric, int mode, uint64_t first_pos, uint64_t n_pos, zh_debug_walk_info *info,
                                   zh_debug_walk_pair *out, size_t cap) {
    if (!ia || !ib || !info || (cap && !out)) return fail(ZH_EINVAL, "zh_debug_walk_pairs: null argument");
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    std::unique_lock<std::shared_mutex> la(ia->mu, std::defer_lock), lb(ib->mu, std::defer_lock);
    if (ia == ib) la.lock();
    else std::lock(la, lb);
    memset(info, 0, sizeof(*info));
    const uint32_t d = ia->opt.dim;
    if (ib->opt.dim != d) return fail(ZH_EINVAL, "zh_debug_walk_pairs: the indexes have different dim (%u and %u)", d, ib->opt.dim);
    if (ia->device != ib->device) return fail(ZH_EINVAL, "zh_debug_walk_pairs: the indexes live on different devices (%d and %d)", ia->device, ib->device);
    if (!zh_exact_mfma_supported(d, metric)) return fail(ZH_EINVAL, "zh_debug_walk_pairs: no matrix-core scan for dim %u, metric %d", d, metric);
    if ((rc = set_device(ia)) || (rc = exact_live_rows(ia)) || (ib != ia && (rc = exact_live_rows(ib)))) return rc;
    HalfView va, vb;
    bool have_a = false, have_b = false;
    {
        std::lock_guard<std::mutex> lk(ia->blk_mu);
        if ((rc = half_view(ia, &va, &have_a))) return rc;
    }
    if (ib == ia) { vb = va; have_b = have_a; }
    else {
        std::lock_guard<std::mutex> lk(ib->blk_mu);
        if ((rc = half_view(ib, &vb, &have_b))) return rc;  // (complete on return: ensure_row_half waits for ib's stream)
    }
    if (!have_a || !have_b) return fail(ZH_ESTATE, "zh_debug_walk_pairs: an index has no fp16 copy of its rows");
    const uint64_t na = ia->n_rows, nb = ib->n_rows, TA = (na + 15) / 16, TB = (nb + 15) / 16;
    if (first_pos % 64 || !n_pos || n_pos > ZH_DEBUG_WALK_ROWS || first_pos + n_pos > TA * 16)
        return fail(ZH_EINVAL, "zh_debug_walk_pairs: a slab starts on a multiple of 64 positions, holds 1 .. %u and ends inside the copy (%llu positions)",
                    ZH_DEBUG_WALK_ROWS, (unsigned long long)(TA * 16));
    const float Kc = zh_approx_bound(metric, d, 1);
    info->held_positions = n_pos; info->col_positions = TB * 16; info->pairs = n_pos * TB * 16;
    info->bound_const = Kc; info->rho_left = va.rho; info->rho_right = vb.rho;
    info->order_left = va.perm ? 1u : 0u; info->order_right = vb.perm ? 1u : 0u;
    if (!out && !cap) return ZH_OK;
    if (cap < info->pairs) return fail(ZH_ELIMIT, "zh_debug_walk_pairs: %llu pairs, room for %zu", (unsigned long long)info->pairs, cap);
    if (!info->pairs) return ZH_OK;
    struct Scratch {
        DevBuf qma, cida, qmb, cidb, rec;
        ~Scratch() { qma.release(); cida.release(); qmb.release(); cidb.release(); rec.release(); }
    } w;
    const size_t rec_bytes = (size_t)info->pairs * sizeof(zh_debug_walk_pair);
    if ((rc = w.qma.ensure(TA * 16 * 16)) || (rc = w.cida.ensure(TA * 16 * 4)) || (rc = w.rec.ensure(rec_bytes))) return rc;
    if (ib != ia && ((rc = w.qmb.ensure(TB * 16 * 16)) || (rc = w.cidb.ensure(TB * 16 * 4)))) return rc;
    const hipStream_t s = ia->stream;
    HIPCHK(zh_launch_join_prep(va.rowMeta, va.perm, va.perm_rows, ia->live_dev.bits.as<uint32_t>(), na, va.rho, w.qma.as<float4>(), w.cida.as<uint32_t>(), s));
    if (ib != ia)
        HIPCHK(zh_launch_join_prep(vb.rowMeta, vb.perm, vb.perm_rows, ib->live_dev.bits.as<uint32_t>(), nb, vb.rho, w.qmb.as<float4>(), w.cidb.as<uint32_t>(), s));
    const DevBuf &qmB = ib != ia ? w.qmb : w.qma, &cidB = ib != ia ? w.cidb : w.cida;
    HIPCHK(hipMemsetAsync(w.rec.p, 0xFF, rec_bytes, s));  // (a record the walk did not write: positions all ones)
    HIPCHK(zh_launch_walk_debug(d, metric, mode, va.Xh, va.rowMeta, w.cida.as<uint32_t>(), na, vb.Xh, qmB.as<float4>(), cidB.as<uint32_t>(), nb, first_pos,
                                first_pos + n_pos, Kc, va.rho, w.rec.as<zh_debug_walk_pair>(), info->pairs, s));
    HIPCHK(hipMemcpyAsync(out, w.rec.p, rec_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// exact k-NN graph (zh_knn.hip + the exact search's two paths): each live row's k nearest OTHER live rows, slab by slab.  DESIGN.md s16
// ------------------------------------------------------------------------------------------------
#define ZH_KNN_HOST_SLAB 65536u  // lines the host call stages at a time

struct KnnRun {  // what a call settles once, before its slabs
    bool path2 = false;
    HalfView v;
    const uint32_t *pos = nullptr;  // row -> position under a row order, else null
    float Kc = 0.f;
    uint32_t cap = 0;               // list slots per line
    LiveCursor live;                // (the slabs of a call ascend)
};

// The gate of path 2 and its per-call views: the copy's rows as approx_interval's queries (zh_launch_join_prep), the row -> position map under a
// row order, the lists' bases.
static int knn_setup(zh_index *ix, uint32_t k, int metric, int mode, hipStream_t s, KnnRun *run) {
    const uint32_t d = ix->opt.dim;
    const char *env_p = getenv("ZH_KNN_PATH");
    if (env_p && atoi(env_p) == 1) return ZH_OK;
    if (!zh_exact_mfma_supported(d, metric) || ix->live_dev.n_live < std::max<uint64_t>((uint64_t)k + 1, 8192)) return ZH_OK;
    int rc;
    HalfView &v = run->v;
    bool have = false;
    {
        std::lock_guard<std::mutex> lb(ix->blk_mu);
        if ((rc = half_view(ix, &v, &have))) return rc;
    }
    if (!have) return ZH_OK;
    const uint64_t n = ix->n_rows, n_pos = (n + 15) / 16 * 16;
    run->cap = 16384 + 8 * k;
    const char *env_c = getenv("ZH_KNN_LIST_CAP");
    if (env_c && atoi(env_c) > 0) run->cap = std::min<uint32_t>(run->cap, (uint32_t)atoi(env_c));
    if ((rc = ix->kn_qm.ensure(n_pos * 16)) || (rc = ix->kn_cid.ensure(n_pos * 4)) || (rc = ix->kn_cbase.ensure((ZH_KNN_PANEL_ROWS + 1) * 8))) return rc;
    HIPCHK(zh_launch_join_prep(v.rowMeta, v.perm, v.perm_rows, ix->live_dev.bits.as<uint32_t>(), n, v.rho, ix->kn_qm.as<float4>(), ix->kn_cid.as<uint32_t>(), s));
    if (v.perm_rows) {
        if ((rc = ix->kn_pos.ensure(n * 4))) return rc;
        HIPCHK(zh_launch_knn_rowpos(ix->kn_cid.as<uint32_t>(), n_pos, ix->kn_pos.as<uint32_t>(), s));
        run->pos = ix->kn_pos.as<uint32_t>();
    }
    std::vector<uint64_t> cb(ZH_KNN_PANEL_ROWS + 1);
    if ((rc = list_bases(ix->kn_cbase.p, cb, run->cap, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));  // (cb is this frame's)
    run->Kc = zh_approx_bound(metric, d, 1);
    run->path2 = true;
    return ZH_OK;
}

// Path 2 of one panel (the B live rows dRows, ascending): its answer [B][k] into kn_pids / kn_pkeys / kn_pcounts.  *overflowed: a line's list ran
// over and the answer is not valid (the caller answers the panel by path 1).
static int knn_panel2(zh_index *ix, const KnnRun &run, const uint32_t *dRows, uint32_t B, uint32_t k, int metric, int mode, hipStream_t s, bool *overflowed,
                      zh_knn_info *inf) {
    const uint32_t d = ix->opt.dim, cap = run.cap, PT = (B + 15) / 16;
    ZhExact2 e{run.v.Xh, run.v.rowMeta, nullptr, 0, ix->live_dev.bits.as<uint32_t>(), nullptr, nullptr, B, run.Kc, run.v.rho};
    int rc;
    if ((rc = ix->kn_A.ensure((size_t)PT * 16 * d * 2)) || (rc = ix->kn_pmeta.ensure((size_t)PT * 16 * 8)) || (rc = ix->kn_pid.ensure((size_t)PT * 16 * 4)) ||
        (rc = ix->ex_Q.ensure((size_t)B * d * 4)) || (rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = lists_ensure(ix, B, cap, false, &e)))
        return rc;
    HIPCHK(zh_launch_knn_panel(d, run.v.Xh, run.v.rowMeta, run.pos, dRows, B, ix->kn_A.p, ix->kn_pmeta.as<float2>(), ix->kn_pid.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, dRows, B, ix->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(ix->ex_Q.as<float>(), B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(hipMemsetAsync(e.tau, 0xFF, (size_t)B * 4, s));
    if ((rc = lists_reset(e, s))) return rc;
    const uint64_t n = ix->n_rows;  // positions of the copy; removed rows are masked by the id word
    uint64_t chunk = (std::max<uint64_t>((uint64_t)k + 1, 4096) + 15) / 16 * 16;
    for (uint64_t p0 = 0; p0 < n; p0 += chunk, chunk *= ZH_EXACT_GROWTH) {
        const uint64_t p1 = std::min(n, p0 + chunk);
        HIPCHK(zh_launch_knn_mfma(d, metric, mode, e, ix->kn_qm.as<float4>(), ix->kn_cid.as<uint32_t>(), p0, p1, ix->kn_A.p, ix->kn_pmeta.as<float2>(),
                                  ix->kn_pid.as<uint32_t>(), s));
        HIPCHK(zh_launch_exact_prune(e, k, ix->ex_scr.as<uint32_t>(), s));
        inf->launches++;
        inf->tiles += (uint64_t)PT * ((p1 + 15) / 16 - p0 / 16);
    }
    HIPCHK(zh_launch_exact_survivor_keys(ix->X.as<float>(), d, ix->ex_Q.as<float>(), ix->ex_QQ.as<float>(), metric, mode, e, ix->ex_ckeys.as<uint64_t>(),
                                         ix->ex_cids.as<uint32_t>(), s));
    HIPCHK(zh_launch_final(ix->kn_cbase.as<uint64_t>(), B, 1, k, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), ix->opt.id_base,
                           ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), nullptr, s));
    return lists_end(e, s, overflowed, &inf->survivors);
}

// One slab on device outputs (under mu, exclusive; exact_live_rows and knn_setup have run; k > 0, n > 0): every line filled as "no neighbours", then
// panel after panel of the slab's live rows.
static int knn_slab(zh_index *ix, KnnRun *run, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys,
                    uint32_t *dCounts, hipStream_t s, zh_knn_info *inf) {
    const uint32_t d = ix->opt.dim;
    int rc;
    HIPCHK(zh_launch_exact_empty((uint32_t)n, k, dIds, dKeys, dCounts, s));
    const uint64_t lo = live_before(ix, first_row, &run->live), hi = live_before(ix, first_row + n, &run->live);
    inf->lines += hi - lo;
    if ((rc = ix->kn_pids.ensure((size_t)ZH_KNN_PANEL_ROWS * (k + 1) * 8)) || (rc = ix->kn_pkeys.ensure((size_t)ZH_KNN_PANEL_ROWS * (k + 1) * 8)) ||
        (rc = ix->kn_pcounts.ensure((size_t)ZH_KNN_PANEL_ROWS * 4)))
        return rc;
    for (uint64_t a0 = lo; a0 < hi; a0 += ZH_KNN_PANEL_ROWS) {
        const uint32_t B = (uint32_t)std::min<uint64_t>(ZH_KNN_PANEL_ROWS, hi - a0);
        const uint32_t *dRows = ix->live_dev.rows.as<uint32_t>() + a0;
        if (run->path2) {
            bool overflowed = false;
            if ((rc = knn_panel2(ix, *run, dRows, B, k, metric, mode, s, &overflowed, inf))) return rc;
            if (!overflowed) {
                HIPCHK(zh_launch_knn_emit(ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), k, dRows, B, ix->opt.id_base,
                                          first_row, k, dIds, dKeys, dCounts, s));
                continue;
            }
            inf->redone++;
        }
        // path 1: the panel as queries, k + 1 over the live list, self taken out of each line
        if ((rc = ix->ex_Q.ensure((size_t)B * d * 4))) return rc;
        HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, dRows, B, ix->ex_Q.as<float>(), s));
        if ((rc = exact_batch(ix, ix->live_dev.rows.as<uint32_t>(), ix->live_dev.n_live, ix->ex_Q.as<float>(), B, k + 1, metric, mode, ix->kn_pids.as<uint64_t>(),
                              ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), s, &inf->launches)))
            return rc;
        HIPCHK(zh_launch_knn_emit(ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), k + 1, dRows, B, ix->opt.id_base,
                                  first_row, k, dIds, dKeys, dCounts, s));
    }
    return ZH_OK;
}

static int knn_args(zh_index *ix, uint64_t n, size_t k, int metric, int mode, const void *ids, const void *keys, const void *counts, const char *who) {
    if (!ix || (n && (!counts || (k && (!ids || !keys))))) return fail(ZH_EINVAL, "%s: null argument", who);
    if (k > ZH_MAX_TOPK - 1) return fail(ZH_ELIMIT, "%s: k %zu > ZH_MAX_TOPK - 1 (%u)", who, k, ZH_MAX_TOPK - 1);
    return check_metric(metric, mode);
}

static int knn_range(zh_index *ix, uint64_t first_row, uint64_t n, const char *who) {
    if (first_row > ix->n_rows || n > ix->n_rows - first_row)
        return fail(ZH_EINVAL, "%s: rows [%llu, %llu + %llu) pass the %llu stored rows", who, (unsigned long long)first_row, (unsigned long long)first_row,
                    (unsigned long long)n, (unsigned long long)ix->n_rows);
    return ZH_OK;
}

// both graphs' host calls: a slab's [m][k] answer from the staging (kn_oids / kn_okeys / kn_ocounts) out to the lines from r0, and waited for
static int knn_stage_out(zh_index *ix, uint64_t r0, uint64_t m, size_t k, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(out_ids + r0 * k, ix->kn_oids.p, m * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_keys + r0 * k, ix->kn_okeys.p, m * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_counts + r0, ix->kn_ocounts.p, m * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

static void knn_record(zh_index *ix, uint32_t k, zh_knn_info inf) {
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    inf.k = k;
    inf.rows_live = ix->live_dev.n_live;
    ix->kn_info = inf;
}

// Both graphs' loop over slabs of lines (k > 0, n > 0); slab(r0, m, dIds, dKeys, dCounts) answers the lines of the rows [r0, r0 + m) on device
// pointers (knn_slab / fknn_slab).  host: the outputs are HOST arrays -- host_slab lines at a time go through the staging (kn_oids, kn_okeys,
// kn_ocounts) and are waited for (knn_stage_out); otherwise ONE slab over the whole range, straight into the caller's device arrays, and one wait.
template <typename Slab>
static int knn_slabs(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, uint64_t host_slab,
                     bool host, hipStream_t s, Slab slab) {
    int rc;
    if (!host) {
        if ((rc = slab(first_row, n, out_ids, out_keys, out_counts))) return rc;
        HIPCHK(hipStreamSynchronize(s));
        return ZH_OK;
    }
    const uint64_t m_max = std::min(n, host_slab);
    if ((rc = ix->kn_oids.ensure(m_max * k * 8)) || (rc = ix->kn_okeys.ensure(m_max * k * 8)) || (rc = ix->kn_ocounts.ensure(m_max * 4))) return rc;
    for (uint64_t r0 = 0; r0 < n; r0 += host_slab) {
        const uint64_t m = std::min(host_slab, n - r0);
        if ((rc = slab(first_row + r0, m, ix->kn_oids.as<uint64_t>(), ix->kn_okeys.as<uint64_t>(), ix->kn_ocounts.as<uint32_t>())) ||
            (rc = knn_stage_out(ix, r0, m, k, out_ids, out_keys, out_counts, s)))
            return rc;
    }
    return ZH_OK;
}

// both graphs with k == 0: the counts alone are the answer
static int knn_no_neighbours(uint64_t n, uint32_t *out_counts, bool host, hipStream_t s) {
    if (host) {
        memset(out_counts, 0, n * 4);
        return ZH_OK;
    }
    HIPCHK(hipMemsetAsync(out_counts, 0, n * 4, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

// both entry points once the arguments have been judged (n > 0)
static int knn_call(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts,
                    bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = knn_range(ix, first_row, n, who))) return rc;
    ScratchGuard guard{ix, SCRATCH_KNN};
    const hipStream_t s = call_stream(ix, stream);
    zh_knn_info inf{};
    inf.path = 1;
    if (k == 0) {
        if ((rc = knn_no_neighbours(n, out_counts, host, s))) return rc;
    } else {
        KnnRun run;
        if ((rc = knn_setup(ix, (uint32_t)k, metric, mode, s, &run))) return rc;
        if (run.path2) inf.path = 2;
        rc = knn_slabs(ix, first_row, n, k, out_ids, out_keys, out_counts, ZH_KNN_HOST_SLAB, host, s,
                       [&](uint64_t r0, uint64_t m, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
                           return knn_slab(ix, &run, r0, m, (uint32_t)k, metric, mode, dIds, dKeys, dCounts, s, &inf);
                       });
        if (rc) return rc;
    }
    knn_record(ix, (uint32_t)k, inf);
    return ZH_OK;
}

extern "C" int zh_knn_graph_device(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                   uint32_t *d_out_counts, void *stream) {
    int rc = knn_args(ix, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_device");
    if (rc || n == 0) return rc;
    return knn_call(ix, first_row, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false, stream, "zh_knn_graph_device");
}

extern "C" int zh_knn_graph(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys,
                            uint32_t *out_counts) {
    int rc = knn_args(ix, n, k, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph");
    if (rc || n == 0) return rc;
    return knn_call(ix, first_row, n, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr, "zh_knn_graph");
}

extern "C" int zh_knn_graph_info(const zh_index *ix, zh_knn_info *out) { return get_info(ix, &zh_index::kn_info, out, "zh_knn_graph_info"); }

// ------------------------------------------------------------------------------------------------
// exact k-NN join between two indexes (zh_xknn.hip, the graph's panels and the exact search's two paths): each live row of A's k nearest live rows
// of B, slab by slab of A.  All scratch and the info on A.  DESIGN.md s30
// ------------------------------------------------------------------------------------------------
struct XknnRun {  // what a call settles once, before its slabs
    bool path2 = false;
    HalfView va, vb;
    const uint32_t *posA = nullptr;  // row -> position of A under A's row order, else null
    float Kc = 0.f;
    uint32_t cap = 0;                // list slots per line
    LiveCursor live;                 // (the slabs of a call ascend)
};

// The gate of path 2 and its per-call views: B's positions as approx_interval's queries with B's rho (zh_launch_join_prep), A's row -> position map
// under a row order of A, the lists' bases.  ZH_XKNN_PATH (read per call): 1 keeps everything on path 1, 2 takes path 2 wherever it is supported
// and B has at least k live rows.
static int xknn_setup(zh_index *ia, zh_index *ib, uint32_t k, int metric, int mode, hipStream_t s, XknnRun *run) {
    const uint32_t d = ia->opt.dim;
    const char *env_p = getenv("ZH_XKNN_PATH");
    const int env_path = env_p ? atoi(env_p) : 0;
    if (env_path == 1 || !zh_exact_mfma_supported(d, metric)) return ZH_OK;
    const uint64_t lb = ib->live_dev.n_live;
    if (!lb || lb < (env_path == 2 ? (uint64_t)k : std::max<uint64_t>(k, 8192))) return ZH_OK;
    int rc;
    bool have_a = false, have_b = false;
    {
        std::lock_guard<std::mutex> lk(ia->blk_mu);
        if ((rc = half_view(ia, &run->va, &have_a))) return rc;
    }
    if (!have_a) return ZH_OK;
    {
        std::lock_guard<std::mutex> lk(ib->blk_mu);
        if ((rc = half_view(ib, &run->vb, &have_b))) return rc;  // (a copy made now is complete on return: ensure_row_half waits for ib's stream)
    }
    if (!have_b) return ZH_OK;
    const uint64_t na = ia->n_rows, nb = ib->n_rows, nb_pos = (nb + 15) / 16 * 16;
    run->cap = 16384 + 8 * k;
    const char *env_c = getenv("ZH_XKNN_LIST_CAP");
    if (env_c && atoi(env_c) > 0) run->cap = std::min<uint32_t>(run->cap, (uint32_t)atoi(env_c));
    if ((rc = ia->xk_qmb.ensure(nb_pos * 16)) || (rc = ia->xk_cidb.ensure(nb_pos * 4)) || (rc = ia->kn_cbase.ensure((ZH_KNN_PANEL_ROWS + 1) * 8))) return rc;
    const HalfView &vb = run->vb;
    HIPCHK(zh_launch_join_prep(vb.rowMeta, vb.perm, vb.perm_rows, ib->live_dev.bits.as<uint32_t>(), nb, vb.rho, ia->xk_qmb.as<float4>(), ia->xk_cidb.as<uint32_t>(), s));
    if (run->va.perm_rows) {
        if ((rc = ia->kn_pos.ensure(na * 4))) return rc;
        HIPCHK(zh_launch_fknn_rowpos(run->va.perm, run->va.perm_rows, na, ia->kn_pos.as<uint32_t>(), s));
        run->posA = ia->kn_pos.as<uint32_t>();
    }
    std::vector<uint64_t> cb(ZH_KNN_PANEL_ROWS + 1);
    if ((rc = list_bases(ia->kn_cbase.p, cb, run->cap, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));  // (cb is this frame's)
    run->Kc = zh_approx_bound(metric, d, 1);
    run->path2 = true;
    return ZH_OK;
}

// Path 2 of one panel (the B live rows dRows of A, ascending): its answer [B][k] into ia's kn_pids / kn_pkeys / kn_pcounts.  *overflowed: a line's
// list ran over and the answer is not valid (the caller answers the panel by path 1).  The held side is A (its copy's bits, rowMeta and rho), the
// columns are B's; the survivors' keys are those of (stored row of B's table, query = the gathered f32 row of A): the contract's orientation.
static int xknn_panel2(zh_index *ia, zh_index *ib, const XknnRun &run, const uint32_t *dRows, uint32_t B, uint32_t k, int metric, int mode, hipStream_t s,
                       bool *overflowed, zh_xknn_info *inf) {
    const uint32_t d = ia->opt.dim, cap = run.cap, PT = (B + 15) / 16;
    ZhExact2 e{run.vb.Xh, run.vb.rowMeta, nullptr, 0, ib->live_dev.bits.as<uint32_t>(), nullptr, nullptr, B, run.Kc, run.va.rho};
    int rc;
    if ((rc = ia->kn_A.ensure((size_t)PT * 16 * d * 2)) || (rc = ia->kn_pmeta.ensure((size_t)PT * 16 * 8)) || (rc = ia->kn_pid.ensure((size_t)PT * 16 * 4)) ||
        (rc = ia->ex_Q.ensure((size_t)B * d * 4)) || (rc = ia->ex_QQ.ensure((size_t)B * 4)) || (rc = lists_ensure(ia, B, cap, false, &e)))
        return rc;
    HIPCHK(zh_launch_knn_panel(d, run.va.Xh, run.va.rowMeta, run.posA, dRows, B, ia->kn_A.p, ia->kn_pmeta.as<float2>(), ia->kn_pid.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_gather(ia->X.as<float>(), d, dRows, B, ia->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(ia->ex_Q.as<float>(), B, d, ia->ex_QQ.as<float>(), s));
    HIPCHK(hipMemsetAsync(e.tau, 0xFF, (size_t)B * 4, s));
    if ((rc = lists_reset(e, s))) return rc;
    const uint64_t n = ib->n_rows;  // positions of B's copy; removed rows are masked by the id word
    uint64_t chunk = (std::max<uint64_t>(k, 4096) + 15) / 16 * 16;
    for (uint64_t p0 = 0; p0 < n; p0 += chunk, chunk *= ZH_EXACT_GROWTH) {
        const uint64_t p1 = std::min(n, p0 + chunk);
        HIPCHK(zh_launch_xknn_mfma(d, metric, mode, e, ia->xk_qmb.as<float4>(), ia->xk_cidb.as<uint32_t>(), p0, p1, ia->kn_A.p, ia->kn_pmeta.as<float2>(),
                                   ia->kn_pid.as<uint32_t>(), s));
        HIPCHK(zh_launch_exact_prune(e, k, ia->ex_scr.as<uint32_t>(), s));
        inf->launches++;
        inf->tiles += (uint64_t)PT * ((p1 + 15) / 16 - p0 / 16);
    }
    HIPCHK(zh_launch_exact_survivor_keys(ib->X.as<float>(), d, ia->ex_Q.as<float>(), ia->ex_QQ.as<float>(), metric, mode, e, ia->ex_ckeys.as<uint64_t>(),
                                         ia->ex_cids.as<uint32_t>(), s));
    HIPCHK(zh_launch_final(ia->kn_cbase.as<uint64_t>(), B, 1, k, ia->ex_ckeys.as<uint64_t>(), ia->ex_cids.as<uint32_t>(), ib->opt.id_base,
                           ia->kn_pids.as<uint64_t>(), ia->kn_pkeys.as<uint64_t>(), ia->kn_pcounts.as<uint32_t>(), nullptr, s));
    return lists_end(e, s, overflowed, &inf->survivors);
}

// One slab of A on device outputs (under both mu, exclusive; xjoin_state and xknn_setup have run; k > 0, n > 0): every line filled as "no
// neighbours", then panel after panel of the slab's live rows.  A B without a live row leaves it at that.
static int xknn_slab(zh_index *ia, zh_index *ib, XknnRun *run, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds,
                     uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, zh_xknn_info *inf) {
    const uint32_t d = ia->opt.dim;
    int rc;
    HIPCHK(zh_launch_exact_empty((uint32_t)n, k, dIds, dKeys, dCounts, s));
    const uint64_t lo = live_before(ia, first_row, &run->live), hi = live_before(ia, first_row + n, &run->live);
    inf->lines += hi - lo;
    if (!ib->live_dev.n_live) return ZH_OK;
    if ((rc = ia->kn_pids.ensure((size_t)ZH_KNN_PANEL_ROWS * k * 8)) || (rc = ia->kn_pkeys.ensure((size_t)ZH_KNN_PANEL_ROWS * k * 8)) ||
        (rc = ia->kn_pcounts.ensure((size_t)ZH_KNN_PANEL_ROWS * 4)))
        return rc;
    for (uint64_t a0 = lo; a0 < hi; a0 += ZH_KNN_PANEL_ROWS) {
        const uint32_t B = (uint32_t)std::min<uint64_t>(ZH_KNN_PANEL_ROWS, hi - a0);
        const uint32_t *dRows = ia->live_dev.rows.as<uint32_t>() + a0;
        bool answered = false;
        if (run->path2) {
            bool overflowed = false;
            if ((rc = xknn_panel2(ia, ib, *run, dRows, B, k, metric, mode, s, &overflowed, inf))) return rc;
            answered = !overflowed;
            if (overflowed) inf->redone++;
        }
        if (!answered) {  // path 1: the panel as queries, k over B's live list
            if ((rc = ia->ex_Q.ensure((size_t)B * d * 4))) return rc;
            HIPCHK(zh_launch_join_gather(ia->X.as<float>(), d, dRows, B, ia->ex_Q.as<float>(), s));
            if ((rc = exact_batch(ia, ib->live_dev.rows.as<uint32_t>(), ib->live_dev.n_live, ia->ex_Q.as<float>(), B, k, metric, mode, ia->kn_pids.as<uint64_t>(),
                                  ia->kn_pkeys.as<uint64_t>(), ia->kn_pcounts.as<uint32_t>(), s, &inf->launches, ib)))
                return rc;
        }
        HIPCHK(zh_launch_xknn_emit(ia->kn_pids.as<uint64_t>(), ia->kn_pkeys.as<uint64_t>(), ia->kn_pcounts.as<uint32_t>(), dRows, B, first_row, k, dIds, dKeys,
                                   dCounts, s));
    }
    return ZH_OK;
}

// judged before any device is touched (and before either handle is followed)
static int xknn_args(const zh_index *ia, const zh_index *ib, uint64_t n, size_t k, int metric, int mode, const void *ids, const void *keys, const void *counts,
                     const char *who) {
    if (!ia || !ib) return fail(ZH_EINVAL, "%s: null argument", who);
    if (ia == ib) return fail(ZH_EINVAL, "%s: the two indexes are the same one; zh_knn_graph ranks an index's rows against its own", who);
    if (n && (!counts || (k && (!ids || !keys)))) return fail(ZH_EINVAL, "%s: null argument", who);
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "%s: k %zu > ZH_MAX_TOPK (%u)", who, k, ZH_MAX_TOPK);
    return ZH_OK;
}

// both entry points once the arguments have been judged (n > 0)
static int xknn_call(zh_index *ia, zh_index *ib, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys,
                     uint32_t *out_counts, bool host, void *stream, const char *who) {
    XjoinLocks locks(ia, ib);
    int rc;
    if ((rc = xjoin_state(ia, ib, who)) || (rc = knn_range(ia, first_row, n, who))) return rc;
    ScratchGuard guard{ia, SCRATCH_XKNN};
    const hipStream_t s = call_stream(ia, stream);
    zh_xknn_info inf{};
    inf.path = 1;
    if (k == 0) {
        if ((rc = knn_no_neighbours(n, out_counts, host, s))) return rc;
    } else {
        XknnRun run;
        if ((rc = xknn_setup(ia, ib, (uint32_t)k, metric, mode, s, &run))) return rc;
        if (run.path2) inf.path = 2;
        rc = knn_slabs(ia, first_row, n, k, out_ids, out_keys, out_counts, ZH_KNN_HOST_SLAB, host, s,
                       [&](uint64_t r0, uint64_t m, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
                           return xknn_slab(ia, ib, &run, r0, m, (uint32_t)k, metric, mode, dIds, dKeys, dCounts, s, &inf);
                       });
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(ia->stats_mu);
    inf.k = (uint32_t)k;
    inf.rows_live_a = ia->live_dev.n_live;
    inf.rows_live_b = ib->live_dev.n_live;
    ia->xk_info = inf;
    return ZH_OK;
}

extern "C" int zh_cross_knn_device(zh_index *ia, zh_index *ib, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *d_out_ids,
                                   uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = xknn_args(ia, ib, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_cross_knn_device");
    if (rc || n == 0) return rc;
    return xknn_call(ia, ib, first_row, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false, stream, "zh_cross_knn_device");
}

extern "C" int zh_cross_knn(zh_index *ia, zh_index *ib, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys,
                            uint32_t *out_counts) {
    int rc = xknn_args(ia, ib, n, k, metric, mode, out_ids, out_keys, out_counts, "zh_cross_knn");
    if (rc || n == 0) return rc;
    return xknn_call(ia, ib, first_row, n, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr, "zh_cross_knn");
}

extern "C" int zh_cross_knn_info(const zh_index *ia, zh_xknn_info *out) { return get_info(ia, &zh_index::xk_info, out, "zh_cross_knn_info"); }

// ------------------------------------------------------------------------------------------------
// forest k-NN graph (zh_fknn.hip): each row's k nearest rows among its leaf-mates over all trees.  DESIGN.md s17
// ------------------------------------------------------------------------------------------------
#define ZH_FKNN_KEY_BUDGET (uint64_t(1) << 25)  // keys one path-1 panel's sweep may write (256 MiB), unless one line's leaves alone hold more

struct ForestRun {  // what a call of either forest family settles once
    uint32_t T = 0;
    bool path2 = false;
    HalfView v;
    const uint32_t *pos = nullptr;  // row -> position under a row order, else null
    float Kc = 0.f;
    std::vector<std::vector<uint2>> leaves;  // per tree the non-empty leaves {offset into leaf_ids, length}, in the host mirror's order
};
struct FknnRun : ForestRun {
    uint32_t env_cap = 0;  // ZH_FKNN_LIST_CAP (0: not set)
};

// The forest families' path rule (env_path: ZH_FKNN_PATH / ZH_FJOIN_PATH, read per call) and path 2's per-call views: the fp16 copy and, under a row
// order, the row -> position map -- made and waited for inside blk_mu, because order.perm is read under blk_mu only.
static int forest_path2(zh_index *ix, const char *env_path, int metric, hipStream_t s, ForestRun *run) {
    const uint32_t d = ix->opt.dim;
    run->T = (uint32_t)ix->h_roots.size();
    const char *env_p = getenv(env_path);
    if ((env_p && atoi(env_p) == 1) || !zh_exact_mfma_supported(d, metric) || ix->opt.max_node_size < 64) return ZH_OK;
    std::lock_guard<std::mutex> lb(ix->blk_mu);
    bool have = false;
    int rc = half_view(ix, &run->v, &have);
    if (rc || !have) return rc;
    if (ix->order.rows) {
        if ((rc = ix->fk_pos.ensure(ix->n_rows * 4))) return rc;
        HIPCHK(zh_launch_fknn_rowpos(ix->order.perm.as<uint32_t>(), ix->order.rows, ix->n_rows, ix->fk_pos.as<uint32_t>(), s));
        HIPCHK(hipStreamSynchronize(s));
        run->pos = ix->fk_pos.as<uint32_t>();
    }
    run->Kc = zh_approx_bound(metric, d, 1);
    run->path2 = true;
    return ZH_OK;
}

// The node -> tree map on the device (both paths' row -> leaf table), the path rule, and path 2's per-call views (its leaves among them).
static int fknn_setup(zh_index *ix, uint32_t k, int metric, int mode, hipStream_t s, FknnRun *run) {
    int rc;
    if ((rc = forest_path2(ix, "ZH_FKNN_PATH", metric, s, run))) return rc;
    const std::vector<uint32_t> node_tree = forest_walk(ix, run->path2 ? &run->leaves : nullptr);
    if ((rc = ix->fk_ntree.ensure(node_tree.size() * 4)) || (rc = ix->fk_ctr.ensure(32))) return rc;
    HIPCHK(hipMemcpyAsync(ix->fk_ntree.p, node_tree.data(), node_tree.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ix->fk_ctr.p, 0, 32, s));
    HIPCHK(hipStreamSynchronize(s));  // (node_tree is this frame's)
    const char *env_c = getenv("ZH_FKNN_LIST_CAP");
    if (env_c && atoi(env_c) > 0) run->env_cap = (uint32_t)atoi(env_c);
    return ZH_OK;
}

// Path 1 of one panel: the B lines dRows (rows of the sub-slab [r0, ...) that some tree holds) -> their lines of the outputs.
static int fknn_panel1(zh_index *ix, const FknnRun &run, uint64_t r0, const uint32_t *dRows, uint32_t B, uint32_t k, int metric, int mode, uint64_t first_row,
                       uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, zh_knn_forest_info *inf) {
    const uint32_t d = ix->opt.dim, T = run.T, w = k + 1;
    const size_t V = (size_t)B * T;
    const uint2 *rl = ix->fk_rl.as<uint2>();
    int rc;
    if ((rc = ix->fk_lens.ensure(V * 4)) || (rc = ix->fk_takes.ensure(V * 4)) || (rc = ix->fk_rbase.ensure((V + 1) * 4)) || (rc = ix->fk_cbase.ensure((V + 1) * 4)) ||
        (rc = ix->fk_tmp.ensure((V / 1024 + 2) * 4)) || (rc = ix->ex_visits.ensure(V * sizeof(ZhVisit))) || (rc = ix->fk_groups.ensure(V * sizeof(ZhGroup))) ||
        (rc = ix->fk_groff.ensure(V * 8)) || (rc = ix->ex_cbase.ensure((V + 1) * 8)) || (rc = ix->ex_Q.ensure((size_t)B * d * 4)) ||
        (rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->kn_pids.ensure((size_t)B * w * 8)) || (rc = ix->kn_pkeys.ensure((size_t)B * w * 8)) ||
        (rc = ix->kn_pcounts.ensure((size_t)B * 4)))
        return rc;
    HIPCHK(zh_launch_fknn_visit_sizes(rl, T, r0, dRows, B, w, ix->fk_lens.as<uint32_t>(), ix->fk_takes.as<uint32_t>(), s));
    HIPCHK(zh_launch_scan_u32(ix->fk_lens.as<uint32_t>(), ix->fk_rbase.as<uint32_t>(), V, ix->fk_tmp.as<uint32_t>(), s));
    HIPCHK(zh_launch_scan_u32(ix->fk_takes.as<uint32_t>(), ix->fk_cbase.as<uint32_t>(), V, ix->fk_tmp.as<uint32_t>(), s));
    HIPCHK(zh_launch_fknn_visits(rl, T, r0, dRows, B, w, ix->fk_rbase.as<uint32_t>(), ix->fk_cbase.as<uint32_t>(), ix->ex_visits.as<ZhVisit>(),
                                 ix->fk_groups.as<ZhGroup>(), ix->fk_groff.as<uint64_t>(), ix->ex_cbase.as<uint64_t>(), s));
    uint32_t tot[2] = {0, 0};  // keys the sweep writes, candidates select keeps
    HIPCHK(hipMemcpyAsync(&tot[0], ix->fk_rbase.as<uint32_t>() + V, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&tot[1], ix->fk_cbase.as<uint32_t>() + V, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = ix->ex_keys.ensure(std::max<size_t>(tot[0], 1) * 8)) || (rc = ix->ex_ckeys.ensure(std::max<size_t>(tot[1], 1) * 8)) ||
        (rc = ix->ex_cids.ensure(std::max<size_t>(tot[1], 1) * 4)))
        return rc;
    const int param = score_param(metric, mode);
    HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, dRows, B, ix->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(ix->ex_Q.as<float>(), B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_sweep(ix->X.as<float>(), d, ix->ex_Q.as<float>(), ix->ex_QQ.as<float>(), ix->fk_groups.as<ZhGroup>(), ix->fk_groff.as<uint64_t>(), V, nullptr,
                           ix->leaf_ids.as<uint32_t>(), tot[0], metric, param, ix->ex_keys.as<uint64_t>(), s));
    HIPCHK(zh_launch_select(ix->ex_visits.as<ZhVisit>(), V, ix->leaf_ids.as<uint32_t>(), ix->ex_keys.as<uint64_t>(), ix->ex_ckeys.as<uint64_t>(),
                            ix->ex_cids.as<uint32_t>(), ix->max_leaf_len, nullptr, s));
    HIPCHK(zh_launch_final(ix->ex_cbase.as<uint64_t>(), B, T, w, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), ix->opt.id_base,
                           ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), nullptr, s));
    HIPCHK(zh_launch_knn_emit(ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), w, dRows, B, ix->opt.id_base, first_row, k,
                              dIds, dKeys, dCounts, s));
    inf->launches++;
    return ZH_OK;
}

// One sub-slab [r0, r0 + m) of the slab that starts at first_row: its row -> leaf table and lines (count: into lines / pairs of the info), and
// (answer) its lines by path 1, panel after panel.
static int fknn_subslab(zh_index *ix, const FknnRun &run, uint64_t r0, uint32_t m, bool count, bool answer, uint32_t k, int metric, int mode,
                        uint64_t first_row, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, zh_knn_forest_info *inf) {
    const uint32_t T = run.T;
    int rc;
    if ((rc = ix->fk_rl.ensure((size_t)m * T * sizeof(uint2))) || (rc = ix->fk_flag.ensure((size_t)m * 4)) || (rc = ix->fk_excl.ensure(((size_t)m + 1) * 4)) ||
        (rc = ix->fk_tmp.ensure(((size_t)m / 1024 + 2) * 4)) || (rc = ix->fk_rows.ensure((size_t)m * 4)))
        return rc;
    unsigned long long *ctr = ix->fk_ctr.as<unsigned long long>();
    HIPCHK(zh_launch_fknn_rowleaf(ix->node_pack.as<int4>(), ix->fk_ntree.as<uint32_t>(), ix->n_nodes, ix->leaf_ids.as<uint32_t>(), T, r0, m, ix->fk_rl.as<uint2>(), s));
    HIPCHK(zh_launch_fknn_lines(ix->fk_rl.as<uint2>(), T, r0, m, ix->fk_flag.as<uint32_t>(), ix->fk_excl.as<uint32_t>(), ix->fk_tmp.as<uint32_t>(),
                                ix->fk_rows.as<uint32_t>(), count ? ctr : ctr + 2, s));
    uint32_t L = 0;
    HIPCHK(hipMemcpyAsync(&L, ix->fk_excl.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (count) inf->lines += L;
    if (!answer || !L) return ZH_OK;
    // lines per panel: their T leaves' keys within the budget (a line's own leaves are the least a panel can hold)
    const uint64_t per_line = (uint64_t)T * std::max<uint32_t>(ix->max_leaf_len, 1);
    const uint32_t P = (uint32_t)std::min<uint64_t>(ZH_KNN_PANEL_ROWS, std::max<uint64_t>(1, ZH_FKNN_KEY_BUDGET / per_line));
    for (uint32_t a0 = 0; a0 < L; a0 += P) {
        const uint32_t B = std::min(P, L - a0);
        if ((rc = fknn_panel1(ix, run, r0, ix->fk_rows.as<uint32_t>() + a0, B, k, metric, mode, first_row, dIds, dKeys, dCounts, s, inf))) return rc;
    }
    return ZH_OK;
}

// Path 2 of one batch of segments of one tree (first: no line has a running answer from an earlier tree yet, so the lists hold whole leaves).
// *overflowed: a list ran over; the batch changed nothing and its lines' sub-slabs are marked in fk_redo.
static int fknn_batch2(zh_index *ix, const FknnRun &run, std::vector<ZhFknnSeg> &segs, const std::vector<uint2> &colsrc, uint32_t held_tiles, uint32_t longest,
                       bool first, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts,
                       hipStream_t s, bool *overflowed, zh_knn_forest_info *inf) {
    const uint32_t d = ix->opt.dim, NT = (uint32_t)colsrc.size(), HB = held_tiles * 16, n_segs = (uint32_t)segs.size();
    // column tiles per block, and with them every segment's first block
    uint32_t n_blocks = 0;
    const uint32_t ch = fill_chunk([&](uint32_t c) {
        n_blocks = 0;
        for (ZhFknnSeg &sg : segs) { sg.first_block = n_blocks; n_blocks += (sg.held_tiles + 3) / 4 * ((sg.ct + c - 1) / c); }
        return n_blocks;
    });
    // list slots per line: a line lists at most its leaf-mates (longest - 1 <= lim): only the ceilings and the test switch can make a list run over
    uint32_t cap = std::min<uint32_t>(longest + k, first ? 16384 + 8 * k : 1024 + 4 * k), lim = cap - k;
    if (run.env_cap) { lim = std::min(lim, run.env_cap); cap = lim + k; }
    ZhExact2 e{run.v.Xh, run.v.rowMeta, nullptr, 0, ix->live_dev.bits.as<uint32_t>(), nullptr, nullptr, HB, run.Kc, run.v.rho};
    int rc;
    if ((rc = ix->fk_segs.ensure((size_t)n_segs * sizeof(ZhFknnSeg))) || (rc = ix->fk_colsrc.ensure((size_t)NT * 8)) || (rc = ix->fk_crow.ensure((size_t)NT * 64)) ||
        (rc = ix->fk_hrow.ensure((size_t)HB * 4)) || (rc = ix->fk_held.ensure((size_t)n_segs * 4)) || (rc = ix->fk_CA.ensure((size_t)NT * 32 * d)) ||
        (rc = ix->fk_cmeta.ensure((size_t)NT * 128)) || (rc = ix->fk_cqm.ensure((size_t)NT * 256)) || (rc = ix->fk_HA.ensure((size_t)HB * 2 * d)) ||
        (rc = ix->fk_hmeta.ensure((size_t)HB * 8)) || (rc = ix->fk_qrow.ensure((size_t)HB * 4)) || (rc = ix->fk_maxk.ensure((size_t)HB * 8)) ||
        (rc = ix->ex_Q.ensure((size_t)HB * d * 4)) || (rc = ix->ex_QQ.ensure((size_t)HB * 4)) || (rc = lists_ensure(ix, HB, cap, true, &e)) ||
        (rc = ix->kn_pids.ensure((size_t)HB * k * 8)) || (rc = ix->kn_pkeys.ensure((size_t)HB * k * 8)) || (rc = ix->kn_pcounts.ensure((size_t)HB * 4)))
        return rc;
    std::vector<uint64_t> cb((size_t)HB + 1);
    const ZhFknnSeg *dSegs = ix->fk_segs.as<ZhFknnSeg>();
    uint32_t *crow = ix->fk_crow.as<uint32_t>(), *hrow = ix->fk_hrow.as<uint32_t>(), *held = ix->fk_held.as<uint32_t>();
    unsigned long long *ctr = ix->fk_ctr.as<unsigned long long>();
    HIPCHK(hipMemcpyAsync(ix->fk_segs.p, segs.data(), (size_t)n_segs * sizeof(ZhFknnSeg), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->fk_colsrc.p, colsrc.data(), (size_t)NT * 8, hipMemcpyHostToDevice, s));
    if ((rc = list_bases(ix->ex_cbase.p, cb, cap, s))) return rc;
    HIPCHK(zh_launch_fknn_cols(ix->fk_colsrc.as<uint2>(), NT, ix->leaf_ids.as<uint32_t>(), ix->n_rows, crow, s));
    HIPCHK(zh_launch_fknn_held(dSegs, n_segs, ix->leaf_ids.as<uint32_t>(), first_row, n, hrow, held, ctr + 1, s));
    HIPCHK(zh_launch_fknn_gather(d, run.v.Xh, run.v.rowMeta, run.pos, crow, NT, run.v.rho, ix->fk_CA.p, ix->fk_cmeta.as<float2>(), ix->fk_cqm.as<float4>(), s));
    HIPCHK(zh_launch_fknn_gather(d, run.v.Xh, run.v.rowMeta, run.pos, hrow, held_tiles, run.v.rho, ix->fk_HA.p, ix->fk_hmeta.as<float2>(), nullptr, s));
    HIPCHK(zh_launch_fknn_bound(hrow, HB, first_row, k, dKeys, dCounts, ix->fk_qrow.as<uint32_t>(), ix->fk_maxk.as<uint64_t>(), s));
    HIPCHK(zh_launch_range_tau(ix->fk_maxk.as<uint64_t>(), HB, metric, mode, e.tau, s));
    if ((rc = lists_reset(e, s))) return rc;
    HIPCHK(zh_launch_fknn_mfma(d, metric, mode, dSegs, n_segs, n_blocks, held, ch, ix->fk_CA.p, ix->fk_cqm.as<float4>(), crow, ix->fk_HA.p,
                               ix->fk_hmeta.as<float2>(), hrow, e, lim, s));
    HIPCHK(zh_launch_exact_prune(e, k, ix->ex_scr.as<uint32_t>(), s));
    HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, ix->fk_qrow.as<uint32_t>(), HB, ix->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(ix->ex_Q.as<float>(), HB, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_exact_survivor_keys(ix->X.as<float>(), d, ix->ex_Q.as<float>(), ix->ex_QQ.as<float>(), metric, mode, e, ix->ex_ckeys.as<uint64_t>(),
                                         ix->ex_cids.as<uint32_t>(), s));
    HIPCHK(zh_launch_fknn_seed(hrow, HB, first_row, ix->opt.id_base, k, dIds, dKeys, dCounts, e, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), s));
    HIPCHK(zh_launch_final(ix->ex_cbase.as<uint64_t>(), HB, 1, k, ix->ex_ckeys.as<uint64_t>(), ix->ex_cids.as<uint32_t>(), ix->opt.id_base,
                           ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), ix->kn_pcounts.as<uint32_t>(), nullptr, s));
    HIPCHK(zh_launch_fknn_store(hrow, HB, first_row, ix->opt.id_base, k, ix->kn_pids.as<uint64_t>(), ix->kn_pkeys.as<uint64_t>(), dIds, dKeys, dCounts,
                                e.over, s));
    if ((rc = lists_end(e, s, overflowed, &inf->survivors))) return rc;  // (segs, colsrc and cb are the caller's and this frame's)
    inf->launches++;
    if (*overflowed) HIPCHK(zh_launch_fknn_mark(hrow, HB, first_row, ix->fk_redo.as<uint32_t>(), s));
    return ZH_OK;
}

// Path 2 of the slab: tree after tree, a tree's leaves in batches of segments (at most ZH_FKNN_HELD_ROWS held lines and ZH_FKNN_COL_TILES column
// tiles, or ONE longer leaf's); then the sub-slabs of the batches whose lists ran over, by path 1.
static int fknn_path2(zh_index *ix, const FknnRun &run, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys,
                      uint32_t *dCounts, hipStream_t s, zh_knn_forest_info *inf) {
    const uint32_t n_sub = (uint32_t)((n + ZH_FKNN_SLAB - 1) / ZH_FKNN_SLAB), HT_MAX = ZH_FKNN_HELD_ROWS / 16;
    int rc;
    if ((rc = ix->fk_redo.ensure((size_t)n_sub * 4))) return rc;
    HIPCHK(hipMemsetAsync(ix->fk_redo.p, 0, (size_t)n_sub * 4, s));
    std::vector<ZhFknnSeg> segs;
    std::vector<uint2> colsrc;
    uint32_t held_tiles = 0, longest = 0;
    bool any_over = false;
    auto flush = [&](bool first) -> int {
        if (segs.empty()) return ZH_OK;
        bool over = false;
        const int r = fknn_batch2(ix, run, segs, colsrc, held_tiles, longest, first, first_row, n, k, metric, mode, dIds, dKeys, dCounts, s, &over, inf);
        any_over = any_over || over;
        segs.clear(); colsrc.clear(); held_tiles = 0; longest = 0;
        return r;
    };
    for (uint32_t t = 0; t < run.T; t++) {
        for (const uint2 leaf : run.leaves[t]) {
            const uint32_t off = leaf.x, len = leaf.y, ct = (len + 15) / 16;
            uint32_t col0 = 0xFFFFFFFFu;  // the leaf's columns in the batch being filled (none yet)
            for (uint32_t w0 = 0; w0 < len; w0 += ZH_FKNN_HELD_ROWS) {
                const uint32_t hl = std::min<uint32_t>(ZH_FKNN_HELD_ROWS, len - w0), ht = (hl + 15) / 16;
                if (!segs.empty() && (held_tiles + ht > HT_MAX || (col0 == 0xFFFFFFFFu && colsrc.size() + ct > ZH_FKNN_COL_TILES))) {
                    if ((rc = flush(t == 0))) return rc;
                    col0 = 0xFFFFFFFFu;
                }
                if (col0 == 0xFFFFFFFFu) {
                    col0 = (uint32_t)colsrc.size();
                    for (uint32_t c = 0; c < ct; c++) colsrc.push_back(make_uint2(off + 16 * c, std::min<uint32_t>(16, len - 16 * c)));
                }
                segs.push_back(ZhFknnSeg{col0, ct, off + w0, hl, held_tiles * 16, ht, 0, 0});
                held_tiles += ht;
                longest = std::max(longest, len);
            }
        }
        if ((rc = flush(t == 0))) return rc;  // (a batch holds one tree's leaves: a line is in it once)
    }
    if (!any_over) return ZH_OK;
    std::vector<uint32_t> redo(n_sub);
    HIPCHK(hipMemcpyAsync(redo.data(), ix->fk_redo.p, (size_t)n_sub * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t j = 0; j < n_sub; j++) {
        if (!redo[j]) continue;
        const uint64_t r0 = first_row + (uint64_t)j * ZH_FKNN_SLAB;
        const uint32_t m = (uint32_t)std::min<uint64_t>(ZH_FKNN_SLAB, first_row + n - r0);
        inf->redone++;
        if ((rc = fknn_subslab(ix, run, r0, m, false, true, k, metric, mode, first_row, dIds, dKeys, dCounts, s, inf))) return rc;
    }
    return ZH_OK;
}

// One slab on device outputs (under mu, exclusive; fknn_setup has run; k > 0, n > 0): every line filled as "no neighbours", the sub-slabs' lines
// and pairs counted, and the lines answered -- sub-slab by sub-slab on path 1, leaf-major over the whole slab on path 2.
static int fknn_slab(zh_index *ix, const FknnRun &run, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds, uint64_t *dKeys,
                     uint32_t *dCounts, hipStream_t s, zh_knn_forest_info *inf) {
    int rc;
    HIPCHK(zh_launch_exact_empty((uint32_t)n, k, dIds, dKeys, dCounts, s));
    for (uint64_t r0 = first_row; r0 < first_row + n; r0 += ZH_FKNN_SLAB) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(ZH_FKNN_SLAB, first_row + n - r0);
        if ((rc = fknn_subslab(ix, run, r0, m, true, !run.path2, k, metric, mode, first_row, dIds, dKeys, dCounts, s, inf))) return rc;
    }
    if (run.path2 && (rc = fknn_path2(ix, run, first_row, n, k, metric, mode, dIds, dKeys, dCounts, s, inf))) return rc;
    return ZH_OK;
}

static int fknn_finish(zh_index *ix, uint32_t k, zh_knn_forest_info inf, hipStream_t s) {
    unsigned long long ctr[2] = {0, 0};
    if (ix->fk_ctr.p) {
        HIPCHK(hipMemcpyAsync(ctr, ix->fk_ctr.p, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    inf.k = k;
    inf.rows_live = ix->live_dev.n_live;
    inf.trees = ix->n_trees;
    inf.pairs = ctr[0];
    inf.tiles = ctr[1];
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->fk_info = inf;
    return ZH_OK;
}

// judged before any device is touched, in this order of kinds: null index (even for n = 0), null outputs of a non-empty request, the metric, the k limit
static int fknn_args(zh_index *ix, uint64_t n, size_t k, int metric, int mode, const void *ids, const void *keys, const void *counts, const char *who) {
    if (!ix || (n && (!counts || (k && (!ids || !keys))))) return fail(ZH_EINVAL, "%s: null argument", who);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (k > ZH_MAX_TOPK - 1) return fail(ZH_ELIMIT, "%s: k %zu > ZH_MAX_TOPK - 1 (%u)", who, k, ZH_MAX_TOPK - 1);
    return ZH_OK;
}

// the state checks both entry points share once the index is locked and the range has been judged (n > 0, k > 0)
static int fknn_state(zh_index *ix, const char *who) {
    if (ix->broken) return fail(ZH_ESTATE, "%s: an incremental add failed: the trees are stale until zh_index_build", who);
    if (!ix->n_trees || ix->h_roots.empty()) return fail(ZH_ESTATE, "%s: the index has no trees (zh_index_build)", who);
    return ZH_OK;
}

// both entry points once the arguments have been judged (n > 0)
static int fknn_call(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts,
                     bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = knn_range(ix, first_row, n, who))) return rc;
    ScratchGuard guard{ix, SCRATCH_FKNN};
    const hipStream_t s = call_stream(ix, stream);
    zh_knn_forest_info inf{};
    inf.path = 1;
    if (k == 0) {
        if ((rc = knn_no_neighbours(n, out_counts, host, s))) return rc;
    } else {
        FknnRun run;
        if ((rc = fknn_state(ix, who)) || (rc = fknn_setup(ix, (uint32_t)k, metric, mode, s, &run))) return rc;
        if (run.path2) inf.path = 2;
        // the staged sub-slab: large, because path 2 serves a slab at the cost of every leaf that holds one of its rows
        const uint64_t host_slab = std::max<uint64_t>(ZH_FKNN_SLAB, (uint64_t(1) << 25) / k / ZH_FKNN_SLAB * ZH_FKNN_SLAB);
        rc = knn_slabs(ix, first_row, n, k, out_ids, out_keys, out_counts, host_slab, host, s,
                       [&](uint64_t r0, uint64_t m, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
                           return fknn_slab(ix, run, r0, m, (uint32_t)k, metric, mode, dIds, dKeys, dCounts, s, &inf);
                       });
        if (rc) return rc;
    }
    return fknn_finish(ix, (uint32_t)k, inf, s);
}

extern "C" int zh_knn_graph_forest_device(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *d_out_ids,
                                          uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = fknn_args(ix, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_forest_device");
    if (rc || n == 0) return rc;
    return fknn_call(ix, first_row, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false, stream, "zh_knn_graph_forest_device");
}

extern "C" int zh_knn_graph_forest(zh_index *ix, uint64_t first_row, uint64_t n, size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys,
                                   uint32_t *out_counts) {
    int rc = fknn_args(ix, n, k, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph_forest");
    if (rc || n == 0) return rc;
    return fknn_call(ix, first_row, n, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr, "zh_knn_graph_forest");
}

extern "C" int zh_knn_graph_forest_info(const zh_index *ix, zh_knn_forest_info *out) {
    return get_info(ix, &zh_index::fk_info, out, "zh_knn_graph_forest_info");
}

// ------------------------------------------------------------------------------------------------
// k-NN graph refinement (zh_refine.hip): each live row's neighbours and their neighbours, ranked by the canonical key.  DESIGN.md s21
// ------------------------------------------------------------------------------------------------
// bytes of the u64 input one pinned buffer holds (the host entry): 64 MiB, ZH_REFINE_CHUNK_BYTES in the environment lowers it (read per call; tests)
static uint64_t refine_chunk_bytes() {
    uint64_t chunk = 64ull << 20;
    if (const char *e = getenv("ZH_REFINE_CHUNK_BYTES")) {
        const long long v = atoll(e);
        if (v >= 8) chunk = std::min<uint64_t>((uint64_t)v, chunk);
    }
    return chunk;
}

struct RefinePins {  // two pinned buffers and an event each: released whatever way the call ends, after the stream has drained
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t s = nullptr;
    ~RefinePins() {
        if (pin[0] || pin[1]) hipStreamSynchronize(s);
        for (int i = 0; i < 2; i++) {
            if (pin[i]) hipHostFree(pin[i]);
            if (ev[i]) hipEventDestroy(ev[i]);
        }
    }
};

// The caller's graph -> rf_tab, the table of row numbers (zh_launch_refine_rows), once per call.  host: in_ids / in_counts are HOST arrays -- the ids
// go chunk by chunk (whole lines) through two pinned buffers and one device chunk, never as a whole u64 copy on the device.
// dst (zh_index_set_graph): the first `lines` lines only, into that table instead of rf_tab; entries are still judged against all stored rows.
static int refine_table(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, bool host, hipStream_t s, uint32_t *dst = nullptr,
                        uint64_t lines = 0) {
    const uint64_t stored = ix->n_rows, N = dst ? lines : stored, id_base = ix->opt.id_base;
    int rc;
    if (!dst) {
        if ((rc = ix->rf_tab.ensure(std::max<size_t>((size_t)N * in_k * 4, 4))) || (rc = ix->rf_ctr.ensure(24))) return rc;
        HIPCHK(hipMemsetAsync(ix->rf_ctr.p, 0, 24, s));
        dst = ix->rf_tab.as<uint32_t>();
    }
    if (!N) return ZH_OK;
    const uint32_t *dBits = ix->live_dev.bits.as<uint32_t>();
    if (!host) {
        HIPCHK(zh_launch_refine_rows(in_ids, in_counts, dBits, id_base, stored, in_k, 0, N, dst, s));
        return ZH_OK;
    }
    const uint64_t line_bytes = (uint64_t)in_k * 8, chunk_lines = std::min<uint64_t>(N, std::max<uint64_t>(1, refine_chunk_bytes() / line_bytes));
    if ((rc = ix->rf_cnt.ensure((size_t)N * 4)) || (rc = ix->rf_stage.ensure(chunk_lines * line_bytes))) return rc;
    HIPCHK(hipMemcpyAsync(ix->rf_cnt.p, in_counts, (size_t)N * 4, hipMemcpyHostToDevice, s));
    RefinePins pp;
    pp.s = s;
    for (int i = 0; i < 2 && (i == 0 || chunk_lines < N); i++) {
        hipError_t e = hipHostMalloc(&pp.pin[i], chunk_lines * line_bytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(ZH_ENOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)(chunk_lines * line_bytes), hipGetErrorString(e));
        HIPCHK(hipEventCreateWithFlags(&pp.ev[i], hipEventDisableTiming));
    }
    uint64_t i = 0;
    for (uint64_t l0 = 0; l0 < N; l0 += chunk_lines, i++) {
        const uint64_t nl = std::min(chunk_lines, N - l0);
        const int b = (int)(i & 1);
        if (i >= 2) HIPCHK(hipEventSynchronize(pp.ev[b]));  // the copy out of this buffer two chunks ago is done
        memcpy(pp.pin[b], in_ids + l0 * in_k, nl * line_bytes);
        HIPCHK(hipMemcpyAsync(ix->rf_stage.p, pp.pin[b], nl * line_bytes, hipMemcpyHostToDevice, s));  // (behind the kernel that read the chunk before)
        HIPCHK(hipEventRecord(pp.ev[b], s));
        HIPCHK(zh_launch_refine_rows(ix->rf_stage.as<uint64_t>(), ix->rf_cnt.as<uint32_t>(), dBits, id_base, stored, in_k, l0, nl, dst, s));
    }
    return ZH_OK;
}

// One slab on device outputs (under mu, exclusive; exact_live_rows and refine_table have run; k > 0, n > 0; dTab's lines are in_k wide, the first
// fwd_k of them the caller's own: rf_tab at in_k twice, or the union table): every line filled as "no neighbours",
// then sub-slab by sub-slab the live lines (a stretch of live_dev.rows), their f32 rows as the query side, their norms, and a block per line.
static int refine_slab(zh_index *ix, LiveCursor *live, const uint32_t *dTab, uint32_t in_k, uint32_t fwd_k, uint64_t first_row, uint64_t n, uint32_t k, int metric, int mode, uint64_t *dIds,
                       uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, zh_knn_refine_info *inf) {
    const uint32_t d = ix->opt.dim;
    int rc;
    HIPCHK(zh_launch_exact_empty((uint32_t)n, k, dIds, dKeys, dCounts, s));
    for (uint64_t r0 = first_row; r0 < first_row + n; r0 += ZH_REFINE_SLAB) {
        const uint64_t m = std::min<uint64_t>(ZH_REFINE_SLAB, first_row + n - r0);
        const uint64_t lo = live_before(ix, r0, live), hi = live_before(ix, r0 + m, live);
        const uint32_t B = (uint32_t)(hi - lo);
        if (!B) continue;
        const uint32_t *dRows = ix->live_dev.rows.as<uint32_t>() + lo;
        if ((rc = ix->ex_Q.ensure((size_t)B * d * 4)) || (rc = ix->ex_QQ.ensure((size_t)B * 4))) return rc;
        HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, dRows, B, ix->ex_Q.as<float>(), s));
        HIPCHK(zh_launch_qnorm(ix->ex_Q.as<float>(), B, d, ix->ex_QQ.as<float>(), s));
        HIPCHK(zh_launch_refine_lines(ix->X.as<float>(), d, dTab, in_k, fwd_k, dRows, B, ix->ex_Q.as<float>(), ix->ex_QQ.as<float>(), metric,
                                      score_param(metric, mode), ix->opt.id_base, first_row, k, dIds, dKeys, dCounts, ix->rf_ctr.as<unsigned long long>(), s));
        inf->lines += B;
        inf->launches++;
    }
    return ZH_OK;
}

// rows a staged piece of a round's output holds (the host entries): 2^25 entries, in whole sub-slabs
static uint64_t refine_host_slab(size_t k) { return std::max<uint64_t>(ZH_REFINE_SLAB, (uint64_t(1) << 25) / k / ZH_REFINE_SLAB * ZH_REFINE_SLAB); }

// every refinement entry, with rev_k = 0 for the plain ones (the limit of the sum then cannot fire behind in_k's).  Judged before any device is
// touched, in this order of kinds: null index (even for n = 0), null inputs or outputs of a non-empty request, the metric, the limits (k, in_k,
// in_k + rev_k), in_k = 0
static int refine_rev_args(zh_index *ix, const void *in_ids, const void *in_counts, size_t in_k, size_t rev_k, uint64_t n, size_t k, int metric, int mode,
                           const void *ids, const void *keys, const void *counts, const char *who) {
    if (!ix || (n && (!in_ids || !in_counts || !counts || (k && (!ids || !keys))))) return fail(ZH_EINVAL, "%s: null argument", who);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (k > ZH_MAX_TOPK - 1) return fail(ZH_ELIMIT, "%s: k %zu > ZH_MAX_TOPK - 1 (%u)", who, k, ZH_MAX_TOPK - 1);
    if (in_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: in_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, ZH_REFINE_MAX_IN_K);
    if (rev_k > ZH_REFINE_MAX_IN_K - in_k) return fail(ZH_ELIMIT, "%s: in_k %zu + rev_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, rev_k, ZH_REFINE_MAX_IN_K);
    if (n && !in_k) return fail(ZH_EINVAL, "%s: in_k is 0", who);
    return ZH_OK;
}

// the transposition's buffers for forward tables up to w wide
static int reverse_ensure(zh_index *ix, uint32_t w) {
    const uint64_t N = ix->n_rows;
    int rc;
    if ((rc = ix->rv_deg.ensure((size_t)N * 4)) || (rc = ix->rv_cur.ensure((size_t)N * 4)) || (rc = ix->rv_off.ensure((size_t)(N + 1) * 8)) ||
        (rc = ix->rv_sums.ensure((size_t)(N / 4096 + 1) * 8)) || (rc = ix->rv_csr.ensure((size_t)N * w * 4)) ||
        (rc = ix->rv_heavy.ensure((size_t)(N * w / ZH_REVERSE_HEAVY + 1) * 4)) || (rc = ix->rv_ctr.ensure(32)))
        return rc;
    return ZH_OK;
}

// The in-neighbours of every stored row out of the forward table dTab, w wide (n_rows > 0): rv_deg, rv_off, rv_csr; rv_ctr = {edges, max in-degree, 0, 0}
static int reverse_csr(zh_index *ix, const uint32_t *dTab, uint32_t w, hipStream_t s) {
    int rc;
    if ((rc = reverse_ensure(ix, w))) return rc;
    HIPCHK(hipMemsetAsync(ix->rv_ctr.p, 0, 32, s));
    HIPCHK(zh_launch_reverse_csr(dTab, ix->live_dev.bits.as<uint32_t>(), ix->n_rows, w, ix->rv_deg.as<uint32_t>(), ix->rv_cur.as<uint32_t>(), ix->rv_off.as<uint64_t>(),
                                 ix->rv_sums.as<uint64_t>(), ix->rv_csr.as<uint32_t>(), ix->rv_ctr.as<unsigned long long>(), s));
    return ZH_OK;
}
// what the multi-round descent adds to `launches` for a transposition beside its selection's count: with that count (which has the heavy-line
// launch in it) the figure the field has always had, 5 + 2 ceil(N w / 2^30) + ceil(N / 2^24).  The one-round calls never counted these passes.
static uint64_t reverse_csr_launches(uint64_t N, uint32_t w) { return 4 + 2 * ((N * w + (1ull << 30) - 1) >> 30); }

// R'(x) of the lines [x0, x0 + nx) of dTab (reverse_csr has run over it): behind N'(x) into the union table dUni (or null) and / or, for the lines of
// [first_row, first_row + n), as ids, counts and in-degrees on device pointers; rv_ctr[2] += the slab's kept entries; *launches += the selection's
static int reverse_select(zh_index *ix, const uint32_t *dTab, uint32_t w, uint32_t rev_k, uint64_t x0, uint64_t nx, uint64_t first_row, uint64_t n, uint32_t *dUni,
                          uint64_t *dIds, uint32_t *dCounts, uint32_t *dDegree, hipStream_t s, uint64_t *launches) {
    HIPCHK(zh_launch_reverse_select(dTab, w, rev_k, ix->rv_off.as<uint64_t>(), ix->rv_csr.as<uint32_t>(), ix->n_rows, x0, nx, first_row, n, ix->opt.id_base, dUni, dIds,
                                    dCounts, dDegree, ix->rv_heavy.as<uint32_t>(), ix->rv_ctr.as<unsigned long long>(), s));
    *launches += zh_line_launches(nx) + 1;
    return ZH_OK;
}

// U(x) of a forward table dTab (w wide): N'(x), then R'(x) -- the transposition and the selection over every stored row into dUni (w + rev_k wide);
// rv_ctr's `kept` counts the lines of [first_row, first_row + n)
static int reverse_union(zh_index *ix, const uint32_t *dTab, uint32_t w, uint32_t rev_k, uint64_t first_row, uint64_t n, uint32_t *dUni, hipStream_t s,
                         uint64_t *launches) {
    int rc;
    if ((rc = reverse_csr(ix, dTab, w, s))) return rc;
    return reverse_select(ix, dTab, w, rev_k, 0, ix->n_rows, first_row, n, dUni, nullptr, nullptr, nullptr, s, launches);
}

// what a first round ranks over: the caller's graph as rf_tab (refine_table), or with rev_k its union table in dUni (in_k + rev_k wide)
static int refine_first_table(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, uint64_t first_row, uint64_t n, bool host,
                              hipStream_t s, uint32_t *dUni, const uint32_t **dTab, uint64_t *rev_launches) {
    int rc;
    if ((rc = refine_table(ix, in_ids, in_counts, in_k, host, s))) return rc;
    *dTab = ix->rf_tab.as<uint32_t>();
    if (!rev_k) return ZH_OK;
    if ((rc = reverse_union(ix, *dTab, in_k, rev_k, first_row, n, dUni, s, rev_launches))) return rc;
    *dTab = dUni;
    return ZH_OK;
}

// A refinement round into the caller's arrays (k > 0, n > 0; under mu, exact_live_rows has run): the table, with rev_k the union (rv_uni), the slabs,
// then the counters -- ctr: rf_ctr's listed / keyed / updates; rctr (or null): rv_ctr -- and the wait for all of it
static int refine_round(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, uint64_t first_row, uint64_t n, uint32_t k,
                        int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host, hipStream_t s, zh_knn_refine_info *inf,
                        unsigned long long *ctr, unsigned long long *rctr, uint64_t *rev_launches) {
    int rc;
    const uint32_t *dTab = nullptr;
    if (rev_k && (rc = ix->rv_uni.ensure((size_t)ix->n_rows * (in_k + rev_k) * 4))) return rc;
    if ((rc = refine_first_table(ix, in_ids, in_counts, in_k, rev_k, first_row, n, host, s, ix->rv_uni.as<uint32_t>(), &dTab, rev_launches))) return rc;
    if (rev_k && rctr) HIPCHK(hipMemcpyAsync(rctr, ix->rv_ctr.p, 32, hipMemcpyDeviceToHost, s));  // (waited for with the slabs)
    LiveCursor live;
    rc = knn_slabs(ix, first_row, n, k, out_ids, out_keys, out_counts, refine_host_slab(k), host, s,
                   [&](uint64_t r0, uint64_t m, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
                       return refine_slab(ix, &live, dTab, in_k + rev_k, in_k, r0, m, k, metric, mode, dIds, dKeys, dCounts, s, inf);
                   });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctr, ix->rf_ctr.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZH_OK;
}

// both entry points of both refinements once the arguments have been judged (n > 0).  rev: zh_knn_graph_refine_rev*, which with rev_k > 0 ranks over
// the union table (N'(x) then R'(x), in_k + rev_k wide) and always records rfr_info; zh_knn_graph_refine* records rf_info
static int refine_call(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, bool rev, uint64_t first_row, uint64_t n,
                       size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = knn_range(ix, first_row, n, who))) return rc;
    ScratchGuard guard{ix, rev ? SCRATCH_REVERSE : SCRATCH_REFINE};
    const hipStream_t s = call_stream(ix, stream);
    zh_knn_refine_info inf{};
    unsigned long long ctr[3] = {0, 0, 0}, rctr[4] = {0, 0, 0, 0};
    uint64_t rev_launches = 0;  // (the fused call's `launches` are the line kernel's)
    if (k == 0) rc = knn_no_neighbours(n, out_counts, host, s);
    else
        rc = refine_round(ix, in_ids, in_counts, in_k, rev_k, first_row, n, (uint32_t)k, metric, mode, out_ids, out_keys, out_counts, host, s, &inf, ctr, rctr,
                          &rev_launches);
    if (rc) return rc;
    inf.rows_live = ix->live_dev.n_live;
    inf.in_k = in_k;
    inf.k = (uint32_t)k;
    inf.listed = ctr[0]; inf.keyed = ctr[1]; inf.updates = ctr[2];
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    if (!rev) {
        ix->rf_info = inf;
        return ZH_OK;
    }
    zh_knn_refine_rev_info r{};
    r.rows_live = inf.rows_live; r.lines = inf.lines; r.in_k = inf.in_k; r.k = inf.k;
    r.listed = inf.listed; r.keyed = inf.keyed; r.updates = inf.updates; r.launches = inf.launches;
    r.rev_k = rev_k; r.edges = rctr[0]; r.kept = rctr[2]; r.max_degree = rctr[1];
    ix->rfr_info = r;
    return ZH_OK;
}

extern "C" int zh_knn_graph_refine_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, uint64_t first_row, uint64_t n,
                                          size_t k, int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = refine_rev_args(ix, d_in_ids, d_in_counts, in_k, 0, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_refine_device");
    if (rc || n == 0) return rc;
    return refine_call(ix, d_in_ids, d_in_counts, (uint32_t)in_k, 0, false, first_row, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false, stream,
                       "zh_knn_graph_refine_device");
}

extern "C" int zh_knn_graph_refine(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, uint64_t first_row, uint64_t n, size_t k,
                                   int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = refine_rev_args(ix, in_ids, in_counts, in_k, 0, n, k, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph_refine");
    if (rc || n == 0) return rc;
    return refine_call(ix, in_ids, in_counts, (uint32_t)in_k, 0, false, first_row, n, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr,
                       "zh_knn_graph_refine");
}

extern "C" int zh_knn_graph_refine_info(const zh_index *ix, zh_knn_refine_info *out) {
    return get_info(ix, &zh_index::rf_info, out, "zh_knn_graph_refine_info");
}

// ------------------------------------------------------------------------------------------------
// reverse neighbours (zh_reverse.hip): the capped transposed graph on its own, and the refinement over N'(x) union R'(x).  DESIGN.md s22
// ------------------------------------------------------------------------------------------------
extern "C" int zh_knn_graph_refine_rev_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                              uint64_t n, size_t k, int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                              void *stream) {
    int rc = refine_rev_args(ix, d_in_ids, d_in_counts, in_k, rev_k, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_refine_rev_device");
    if (rc || n == 0) return rc;
    return refine_call(ix, d_in_ids, d_in_counts, (uint32_t)in_k, (uint32_t)rev_k, true, first_row, n, k, metric, mode, d_out_ids, d_out_keys, d_out_counts, false,
                       stream, "zh_knn_graph_refine_rev_device");
}

extern "C" int zh_knn_graph_refine_rev(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                                       size_t k, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = refine_rev_args(ix, in_ids, in_counts, in_k, rev_k, n, k, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph_refine_rev");
    if (rc || n == 0) return rc;
    return refine_call(ix, in_ids, in_counts, (uint32_t)in_k, (uint32_t)rev_k, true, first_row, n, k, metric, mode, out_ids, out_keys, out_counts, true, nullptr,
                       "zh_knn_graph_refine_rev");
}

extern "C" int zh_knn_graph_refine_rev_info(const zh_index *ix, zh_knn_refine_rev_info *out) {
    return get_info(ix, &zh_index::rfr_info, out, "zh_knn_graph_refine_rev_info");
}

// judged before any device is touched, in this order of kinds: null index (even for n = 0), null inputs or outputs of a non-empty request, the two
// limits, in_k = 0, rev_k = 0
static int reverse_args(zh_index *ix, const void *in_ids, const void *in_counts, size_t in_k, size_t rev_k, uint64_t n, const void *ids, const void *counts,
                        const void *degree, const char *who) {
    if (!ix || (n && (!in_ids || !in_counts || !ids || !counts || !degree))) return fail(ZH_EINVAL, "%s: null argument", who);
    if (in_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: in_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, ZH_REFINE_MAX_IN_K);
    if (rev_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: rev_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, rev_k, ZH_REFINE_MAX_IN_K);
    if (n && !in_k) return fail(ZH_EINVAL, "%s: in_k is 0", who);
    if (n && !rev_k) return fail(ZH_EINVAL, "%s: rev_k is 0", who);
    return ZH_OK;
}

// both entry points once the arguments have been judged (n > 0).  host: the outputs are HOST arrays and go piece by piece through the staging
static int reverse_call(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, uint64_t first_row, uint64_t n,
                        uint64_t *out_ids, uint32_t *out_counts, uint32_t *out_degree, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = knn_range(ix, first_row, n, who))) return rc;
    ScratchGuard guard{ix, SCRATCH_REVERSE};
    const hipStream_t s = call_stream(ix, stream);
    zh_knn_reverse_info inf{};
    unsigned long long rctr[4] = {0, 0, 0, 0};
    if ((rc = refine_table(ix, in_ids, in_counts, in_k, host, s))) return rc;
    const uint32_t *dTab = ix->rf_tab.as<uint32_t>();
    if ((rc = reverse_csr(ix, dTab, in_k, s))) return rc;
    if (!host) {
        if ((rc = reverse_select(ix, dTab, in_k, rev_k, first_row, n, first_row, n, nullptr, out_ids, out_counts, out_degree, s, &inf.launches))) return rc;
    } else {
        const uint64_t piece = std::min<uint64_t>(n, std::max<uint64_t>(ZH_REFINE_SLAB, (uint64_t(1) << 25) / rev_k));
        if ((rc = ix->rv_oids.ensure(piece * rev_k * 8)) || (rc = ix->rv_ocounts.ensure(piece * 4)) || (rc = ix->rv_odeg.ensure(piece * 4))) return rc;
        for (uint64_t r0 = 0; r0 < n; r0 += piece) {
            const uint64_t m = std::min(piece, n - r0);
            if ((rc = reverse_select(ix, dTab, in_k, rev_k, first_row + r0, m, first_row + r0, m, nullptr, ix->rv_oids.as<uint64_t>(), ix->rv_ocounts.as<uint32_t>(),
                                     ix->rv_odeg.as<uint32_t>(), s, &inf.launches)))
                return rc;
            HIPCHK(hipMemcpyAsync(out_ids + r0 * rev_k, ix->rv_oids.p, m * rev_k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_counts + r0, ix->rv_ocounts.p, m * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_degree + r0, ix->rv_odeg.p, m * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    HIPCHK(hipMemcpyAsync(rctr, ix->rv_ctr.p, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    LiveCursor live;
    inf.rows_live = ix->live_dev.n_live;
    inf.lines = live_before(ix, first_row + n, &live) - live_before(ix, first_row, &live);
    inf.in_k = in_k;
    inf.rev_k = rev_k;
    inf.edges = rctr[0]; inf.kept = rctr[2]; inf.max_degree = rctr[1];
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    ix->rv_info = inf;
    return ZH_OK;
}

extern "C" int zh_knn_graph_reverse_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                           uint64_t n, uint64_t *d_out_ids, uint32_t *d_out_counts, uint32_t *d_out_degree, void *stream) {
    int rc = reverse_args(ix, d_in_ids, d_in_counts, in_k, rev_k, n, d_out_ids, d_out_counts, d_out_degree, "zh_knn_graph_reverse_device");
    if (rc || n == 0) return rc;
    return reverse_call(ix, d_in_ids, d_in_counts, (uint32_t)in_k, (uint32_t)rev_k, first_row, n, d_out_ids, d_out_counts, d_out_degree, false, stream,
                        "zh_knn_graph_reverse_device");
}

extern "C" int zh_knn_graph_reverse(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                                    uint64_t *out_ids, uint32_t *out_counts, uint32_t *out_degree) {
    int rc = reverse_args(ix, in_ids, in_counts, in_k, rev_k, n, out_ids, out_counts, out_degree, "zh_knn_graph_reverse");
    if (rc || n == 0) return rc;
    return reverse_call(ix, in_ids, in_counts, (uint32_t)in_k, (uint32_t)rev_k, first_row, n, out_ids, out_counts, out_degree, true, nullptr,
                        "zh_knn_graph_reverse");
}

extern "C" int zh_knn_graph_reverse_info(const zh_index *ix, zh_knn_reverse_info *out) {
    return get_info(ix, &zh_index::rv_info, out, "zh_knn_graph_reverse_info");
}

// ------------------------------------------------------------------------------------------------
// k-NN graph pruning (zh_prune.hip): each live row's unoccluded neighbours out of its line, with rev_k out of N'(a) union R'(a).  DESIGN.md s29
// ------------------------------------------------------------------------------------------------
// refine_rev_args' kinds in its order, `degree` where k stands and `fill` behind in_k = 0.  Judged before any device is touched
static int prune_args(zh_index *ix, const void *in_ids, const void *in_counts, size_t in_k, size_t rev_k, uint64_t n, size_t degree, int fill, int metric, int mode,
                      const void *ids, const void *keys, const void *counts, const char *who) {
    if (!ix || (n && (!in_ids || !in_counts || !counts || (degree && (!ids || !keys))))) return fail(ZH_EINVAL, "%s: null argument", who);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (degree > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: degree %zu > ZH_REFINE_MAX_IN_K (%u)", who, degree, ZH_REFINE_MAX_IN_K);
    if (in_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: in_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, ZH_REFINE_MAX_IN_K);
    if (rev_k > ZH_REFINE_MAX_IN_K - in_k) return fail(ZH_ELIMIT, "%s: in_k %zu + rev_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, rev_k, ZH_REFINE_MAX_IN_K);
    if (n && !in_k) return fail(ZH_EINVAL, "%s: in_k is 0", who);
    if (fill != 0 && fill != 1) return fail(ZH_EINVAL, "%s: fill %d is neither 0 nor 1", who, fill);
    return ZH_OK;
}

// One slab on device outputs (under mu, exclusive; exact_live_rows and refine_first_table have run; degree > 0, n > 0; dTab's lines are w wide):
// every line filled as "no neighbours", then refine_slab's sub-slabs, a block per live line.  The line's row and the kept rows that become the
// query are read where they are stored, their norms out of pr_qq: nothing is gathered.
static int prune_slab(zh_index *ix, LiveCursor *live, const uint32_t *dTab, uint32_t w, uint64_t first_row, uint64_t n, uint32_t degree, uint32_t fill, int metric,
                      int mode, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts, hipStream_t s, zh_knn_prune_info *inf) {
    HIPCHK(zh_launch_exact_empty((uint32_t)n, degree, dIds, dKeys, dCounts, s));
    for (uint64_t r0 = first_row; r0 < first_row + n; r0 += ZH_REFINE_SLAB) {
        const uint64_t m = std::min<uint64_t>(ZH_REFINE_SLAB, first_row + n - r0);
        const uint64_t lo = live_before(ix, r0, live), hi = live_before(ix, r0 + m, live);
        const uint32_t B = (uint32_t)(hi - lo);
        if (!B) continue;
        HIPCHK(zh_launch_prune_lines(ix->X.as<float>(), ix->opt.dim, dTab, w, ix->live_dev.rows.as<uint32_t>() + lo, B, ix->pr_qq.as<float>(), metric,
                                     score_param(metric, mode), ix->opt.id_base, first_row, degree, fill, dIds, dKeys, dCounts,
                                     ix->pr_ctr.as<unsigned long long>(), s));
        inf->lines += B;
        inf->launches++;
    }
    return ZH_OK;
}

// both entry points once the arguments have been judged (n > 0)
static int prune_call(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, uint64_t first_row, uint64_t n, uint32_t degree,
                      uint32_t fill, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix)) || (rc = knn_range(ix, first_row, n, who))) return rc;
    ScratchGuard guard{ix, SCRATCH_PRUNE};
    const hipStream_t s = call_stream(ix, stream);
    zh_knn_prune_info inf{};
    unsigned long long ctr[6] = {0, 0, 0, 0, 0, 0};
    if (degree == 0) {
        if ((rc = knn_no_neighbours(n, out_counts, host, s))) return rc;
    } else {
        const uint64_t N = ix->n_rows;
        const uint32_t d = ix->opt.dim;
        const uint32_t *dTab = nullptr;
        uint64_t rev_launches = 0;  // (`launches` are the line kernel's)
        if (rev_k && (rc = ix->rv_uni.ensure((size_t)N * (in_k + rev_k) * 4))) return rc;
        if ((rc = refine_first_table(ix, in_ids, in_counts, in_k, rev_k, first_row, n, host, s, ix->rv_uni.as<uint32_t>(), &dTab, &rev_launches))) return rc;
        if ((rc = ix->pr_ctr.ensure(48))) return rc;
        HIPCHK(hipMemsetAsync(ix->pr_ctr.p, 0, 48, s));
        if (metric == ZH_COSINE) {  // every stored row's squared norm: a kept row's as the query, as zh_launch_qnorm gives it to the exact search
            if ((rc = ix->pr_qq.ensure((size_t)N * 4))) return rc;
            for (uint64_t r0 = 0; r0 < N; r0 += 1ull << 30)
                HIPCHK(zh_launch_qnorm(ix->X.as<float>() + r0 * d, (uint32_t)std::min<uint64_t>(1ull << 30, N - r0), d, ix->pr_qq.as<float>() + r0, s));
        }
        LiveCursor live;
        rc = knn_slabs(ix, first_row, n, degree, out_ids, out_keys, out_counts, refine_host_slab(degree), host, s,
                       [&](uint64_t r0, uint64_t m, uint64_t *dIds, uint64_t *dKeys, uint32_t *dCounts) {
                           return prune_slab(ix, &live, dTab, in_k + rev_k, r0, m, degree, fill, metric, mode, dIds, dKeys, dCounts, s, &inf);
                       });
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctr, ix->pr_ctr.p, 48, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    inf.rows_live = ix->live_dev.n_live;
    inf.in_k = in_k; inf.rev_k = rev_k; inf.degree = degree; inf.fill = fill;
    inf.candidates = ctr[0]; inf.kept = ctr[1]; inf.occluded = ctr[2]; inf.filled = ctr[3]; inf.cut = ctr[4]; inf.keyed = ctr[5];
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    ix->pr_info = inf;
    return ZH_OK;
}

extern "C" int zh_knn_graph_prune_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                         uint64_t n, size_t degree, int fill, int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                         uint32_t *d_out_counts, void *stream) {
    int rc = prune_args(ix, d_in_ids, d_in_counts, in_k, rev_k, n, degree, fill, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_prune_device");
    if (rc || n == 0) return rc;
    return prune_call(ix, d_in_ids, d_in_counts, (uint32_t)in_k, (uint32_t)rev_k, first_row, n, (uint32_t)degree, (uint32_t)fill, metric, mode, d_out_ids,
                      d_out_keys, d_out_counts, false, stream, "zh_knn_graph_prune_device");
}

extern "C" int zh_knn_graph_prune(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                                  size_t degree, int fill, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = prune_args(ix, in_ids, in_counts, in_k, rev_k, n, degree, fill, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph_prune");
    if (rc || n == 0) return rc;
    return prune_call(ix, in_ids, in_counts, (uint32_t)in_k, (uint32_t)rev_k, first_row, n, (uint32_t)degree, (uint32_t)fill, metric, mode, out_ids, out_keys,
                      out_counts, true, nullptr, "zh_knn_graph_prune");
}

extern "C" int zh_knn_graph_prune_info(const zh_index *ix, zh_knn_prune_info *out) {
    return get_info(ix, &zh_index::pr_info, out, "zh_knn_graph_prune_info");
}

// ------------------------------------------------------------------------------------------------
// NN-descent (zh_nnd.hip): the refinement's rounds on the device, keying from round 2 on only what a new entry brings up.  DESIGN.md s23
// ------------------------------------------------------------------------------------------------
// refine_rev_args' order with the rounds and k = 0 behind the metric, and k + rev_k's limit behind in_k + rev_k's.  Whole table: the pointers are
// judged whatever the table holds
static int descent_args(zh_index *ix, const void *in_ids, const void *in_counts, size_t in_k, size_t rev_k, size_t k, size_t rounds, int metric, int mode,
                        const void *ids, const void *keys, const void *counts, const char *who) {
    if (!ix || !in_ids || !in_counts || !ids || !keys || !counts) return fail(ZH_EINVAL, "%s: null argument", who);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (rounds < 1 || rounds > ZH_DESCENT_MAX_ROUNDS) return fail(ZH_EINVAL, "%s: rounds %zu outside 1 .. %u", who, rounds, ZH_DESCENT_MAX_ROUNDS);
    if (!k) return fail(ZH_EINVAL, "%s: k is 0", who);
    if (in_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: in_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, ZH_REFINE_MAX_IN_K);
    if (rev_k > ZH_REFINE_MAX_IN_K - in_k) return fail(ZH_ELIMIT, "%s: in_k %zu + rev_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, in_k, rev_k, ZH_REFINE_MAX_IN_K);
    if (k > ZH_REFINE_MAX_IN_K || rev_k > ZH_REFINE_MAX_IN_K - k)
        return fail(ZH_ELIMIT, "%s: k %zu + rev_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, k, rev_k, ZH_REFINE_MAX_IN_K);
    if (!in_k) return fail(ZH_EINVAL, "%s: in_k is 0", who);
    return ZH_OK;
}

// both entry points once the arguments have been judged
static int descent_call(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint32_t in_k, uint32_t rev_k, uint32_t k, uint32_t rounds, int metric,
                        int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    const uint64_t N = ix->n_rows, n_live = ix->live_dev.n_live;
    if (!N) return ZH_OK;
    ScratchGuard guard{ix, SCRATCH_DESCENT};
    const hipStream_t s = call_stream(ix, stream);
    const uint32_t d = ix->opt.dim, w1 = in_k + rev_k, w = k + rev_k, wmax = std::max(in_k, k);
    const int param = score_param(metric, mode);
    zh_knn_descent_info inf{};
    inf.rows_live = n_live; inf.in_k = in_k; inf.rev_k = rev_k; inf.k = k; inf.rounds = rounds;
    unsigned long long ctr[ZH_NND_CTRS] = {0, 0, 0, 0, 0, 0};
    const auto first_round = [&](uint64_t lines, uint64_t launches) {  // what round 1 leaves in the info (ctr: rf_ctr's three words)
        inf.launches += launches;
        if (w1 + w1 * w1 > ZH_REFINE_CAP_SMALL) inf.large_lines += lines;
        inf.listed = ctr[0]; inf.keyed = ctr[1]; inf.updates = ctr[2]; inf.lines_active = n_live;
        inf.keyed_round[0] = ctr[1]; inf.updates_round[0] = ctr[2]; inf.active_round[0] = n_live;
        inf.rounds_run = 1;
    };
    zh_knn_refine_info one{};
    if (rounds == 1) {  // one round is zh_knn_graph_refine_rev and nothing else: its passes, straight into the caller's arrays, no state of the call's own
        if ((rc = refine_round(ix, in_ids, in_counts, in_k, rev_k, 0, N, k, metric, mode, out_ids, out_keys, out_counts, host, s, &one, ctr, nullptr, &inf.launches)))
            return rc;
        first_round(one.lines, one.launches);
        std::lock_guard<std::mutex> ls(ix->stats_mu);
        ix->nd_info = inf;
        return ZH_OK;
    }
    // ---- the call's state: everything a later round reads is there before the first one starts, so that ZH_ENOMEM comes before any work
    for (int i = 0; i < 2; i++)
        if ((rc = ix->nd_tab[i].ensure((size_t)N * k * 4)) || (rc = ix->nd_key[i].ensure((size_t)N * k * 8)) ||
            (rev_k && (rc = ix->nd_uni[i].ensure((size_t)N * (wmax + rev_k) * 4))))
            return rc;
    if ((rc = ix->nd_mask.ensure((size_t)N * 8)) || (rc = ix->nd_list.ensure(std::max<size_t>((size_t)n_live * 4, 4))) || (rc = ix->nd_qq.ensure((size_t)N * 4)) ||
        (rc = ix->nd_ctr.ensure(ZH_NND_CTRS * 8)))
        return rc;
    if (rev_k && (rc = reverse_ensure(ix, wmax))) return rc;
    const uint64_t piece = std::min<uint64_t>(N, refine_host_slab(k));
    if ((rc = ix->kn_oids.ensure(piece * k * 8)) || (rc = ix->kn_ocounts.ensure(piece * 4)) || (host && (rc = ix->kn_okeys.ensure(piece * k * 8)))) return rc;
    uint32_t *tab[2] = {ix->nd_tab[0].as<uint32_t>(), ix->nd_tab[1].as<uint32_t>()};
    uint64_t *key[2] = {ix->nd_key[0].as<uint64_t>(), ix->nd_key[1].as<uint64_t>()};
    uint32_t *uni[2] = {ix->nd_uni[0].as<uint32_t>(), ix->nd_uni[1].as<uint32_t>()};
    unsigned long long *dCtr = ix->nd_ctr.as<unsigned long long>();
    for (int i = 0; i < 2; i++) {  // (a removed row's line is never written again: empty in both tables)
        HIPCHK(hipMemsetAsync(tab[i], 0xFF, (size_t)N * k * 4, s));
        HIPCHK(hipMemsetAsync(key[i], 0xFF, (size_t)N * k * 8, s));
    }
    if (metric == ZH_COSINE)
        for (uint64_t r0 = 0; r0 < N; r0 += 1ull << 30)
            HIPCHK(zh_launch_qnorm(ix->X.as<float>() + r0 * d, (uint32_t)std::min<uint64_t>(1ull << 30, N - r0), d, ix->nd_qq.as<float>() + r0, s));
    // ---- round 1: zh_knn_graph_refine_rev's passes; the keys go straight to key[0], the ids piece by piece through the staging into tab[0]
    const uint32_t *Uprev = nullptr;  // U_0, w1 wide
    if ((rc = refine_first_table(ix, in_ids, in_counts, in_k, rev_k, 0, N, host, s, uni[0], &Uprev, &inf.launches))) return rc;
    if (rev_k) inf.launches += reverse_csr_launches(N, in_k);
    {
        LiveCursor live;
        for (uint64_t r0 = 0; r0 < N; r0 += piece) {
            const uint64_t m = std::min(piece, N - r0);
            if ((rc = refine_slab(ix, &live, Uprev, w1, in_k, r0, m, k, metric, mode, ix->kn_oids.as<uint64_t>(), key[0] + r0 * k, ix->kn_ocounts.as<uint32_t>(), s,
                                  &one)))
                return rc;
            HIPCHK(zh_launch_nnd_rows(ix->kn_oids.as<uint64_t>(), ix->opt.id_base, m, k, tab[0] + r0 * k, s));
            inf.launches++;
        }
    }
    HIPCHK(hipMemcpyAsync(ctr, ix->rf_ctr.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    first_round(one.lines, one.launches);
    // ---- rounds 2 ..: G_r is tab[(r - 1) & 1] with key[(r - 1) & 1], U_r is that table or uni[r & 1]; the round writes the other pair
    uint32_t wp = w1;
    for (uint32_t r = 1; r < rounds && inf.updates; r++) {
        const int c = (int)((r - 1) & 1), nx = (int)(r & 1);
        const uint32_t *Ucur = tab[c];
        if (rev_k) {
            if ((rc = reverse_union(ix, tab[c], k, rev_k, 0, N, uni[r & 1], s, &inf.launches))) return rc;
            inf.launches += reverse_csr_launches(N, k);
            Ucur = uni[r & 1];
        }
        HIPCHK(hipMemsetAsync(dCtr, 0, ZH_NND_CTRS * 8, s));
        HIPCHK(zh_launch_nnd_flag(Uprev, wp, Ucur, w, N, ix->nd_mask.as<uint64_t>(), s));
        HIPCHK(zh_launch_nnd_plan(Ucur, w, k, ix->nd_mask.as<uint64_t>(), ix->live_dev.rows.as<uint32_t>(), n_live, key[c], tab[nx], key[nx],
                                  ix->nd_list.as<uint32_t>(), dCtr, s));
        HIPCHK(zh_launch_nnd_lines(ix->X.as<float>(), d, Ucur, w, k, ix->nd_mask.as<uint64_t>(), key[c], ix->nd_qq.as<float>(), ix->nd_list.as<uint32_t>(), n_live,
                                   metric, param, tab[nx], key[nx], dCtr, s));
        inf.launches += 2 * zh_line_launches(N) + (w + w * w > ZH_REFINE_CAP_SMALL ? 2 : 1);
        HIPCHK(hipMemcpyAsync(ctr, dCtr, ZH_NND_CTRS * 8, hipMemcpyDeviceToHost, s));  // the round's one readback: it decides the early stop
        HIPCHK(hipStreamSynchronize(s));
        inf.listed += ctr[0]; inf.keyed += ctr[1]; inf.updates = ctr[2]; inf.lines_active += ctr[3]; inf.large_lines += ctr[5];
        inf.keyed_round[r] = ctr[1]; inf.updates_round[r] = ctr[2]; inf.active_round[r] = ctr[3];
        inf.rounds_run = r + 1;
        Uprev = Ucur;
        wp = w;
    }
    // ---- the answer: G_{rounds_run}
    const int f = (int)((inf.rounds_run - 1) & 1);
    if (!host) {
        HIPCHK(zh_launch_nnd_emit(tab[f], key[f], k, ix->opt.id_base, N, out_ids, out_keys, out_counts, s));
        HIPCHK(hipStreamSynchronize(s));
        inf.launches += zh_line_launches(N);
    } else {
        for (uint64_t r0 = 0; r0 < N; r0 += piece) {
            const uint64_t m = std::min(piece, N - r0);
            HIPCHK(zh_launch_nnd_emit(tab[f] + r0 * k, key[f] + r0 * k, k, ix->opt.id_base, m, ix->kn_oids.as<uint64_t>(), ix->kn_okeys.as<uint64_t>(),
                                      ix->kn_ocounts.as<uint32_t>(), s));
            if ((rc = knn_stage_out(ix, r0, m, k, out_ids, out_keys, out_counts, s))) return rc;
            inf.launches++;
        }
    }
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    ix->nd_info = inf;
    return ZH_OK;
}

extern "C" int zh_knn_graph_descent_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, size_t k, size_t rounds,
                                           int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    int rc = descent_args(ix, d_in_ids, d_in_counts, in_k, rev_k, k, rounds, metric, mode, d_out_ids, d_out_keys, d_out_counts, "zh_knn_graph_descent_device");
    if (rc) return rc;
    return descent_call(ix, d_in_ids, d_in_counts, (uint32_t)in_k, (uint32_t)rev_k, (uint32_t)k, (uint32_t)rounds, metric, mode, d_out_ids, d_out_keys, d_out_counts,
                        false, stream, "zh_knn_graph_descent_device");
}

extern "C" int zh_knn_graph_descent(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, size_t k, size_t rounds, int metric,
                                    int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = descent_args(ix, in_ids, in_counts, in_k, rev_k, k, rounds, metric, mode, out_ids, out_keys, out_counts, "zh_knn_graph_descent");
    if (rc) return rc;
    return descent_call(ix, in_ids, in_counts, (uint32_t)in_k, (uint32_t)rev_k, (uint32_t)k, (uint32_t)rounds, metric, mode, out_ids, out_keys, out_counts, true,
                        nullptr, "zh_knn_graph_descent");
}

extern "C" int zh_knn_graph_descent_info(const zh_index *ix, zh_knn_descent_info *out) {
    return get_info(ix, &zh_index::nd_info, out, "zh_knn_graph_descent_info");
}

// ------------------------------------------------------------------------------------------------
// graph search (zh_gsearch.hip): a k-NN graph kept on the index (GraphView) and the beam search over it.  DESIGN.md s24
// ------------------------------------------------------------------------------------------------
// both attach entry points.  Judged before any device is touched: null index, null arrays of a non-empty graph, g_k = 0, g_k's limit; under the
// lock: g_rows against the stored rows, the table against 2^31 rows.  The new table is made beside the old one: a failure leaves what was attached.
static int graph_attach(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint64_t g_rows, size_t g_k, bool host, void *stream, const char *who) {
    if (!ix || (g_rows && (!in_ids || !in_counts))) return fail(ZH_EINVAL, "%s: null argument", who);
    if (!g_k) return fail(ZH_EINVAL, "%s: g_k is 0", who);
    if (g_k > ZH_REFINE_MAX_IN_K) return fail(ZH_ELIMIT, "%s: g_k %zu > ZH_REFINE_MAX_IN_K (%u)", who, g_k, ZH_REFINE_MAX_IN_K);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    if (g_rows > ix->n_rows) return fail(ZH_EINVAL, "%s: g_rows %llu > the %llu stored rows", who, (unsigned long long)g_rows, (unsigned long long)ix->n_rows);
    if (ix->n_rows >= (1ull << 31)) return fail(ZH_ELIMIT, "%s: %llu stored rows; graph search serves tables below 2^31 rows", who, (unsigned long long)ix->n_rows);
    ScratchGuard guard{ix, SCRATCH_GRAPH_ATTACH};
    const hipStream_t s = call_stream(ix, stream);
    DevBuf tab;
    if ((rc = tab.ensure(std::max<size_t>((size_t)g_rows * g_k * 4, 4)))) return rc;
    rc = refine_table(ix, in_ids, in_counts, (uint32_t)g_k, host, s, tab.as<uint32_t>(), g_rows);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(ZH_EHIP, "%s: the table of row numbers failed", who);
    if (rc) { tab.release(); return rc; }
    ix->graph.drop();
    ix->graph.tab = tab;
    ix->graph.mark_attached(g_rows, (uint32_t)g_k);
    return ZH_OK;
}

extern "C" int zh_index_set_graph(zh_index *ix, const uint64_t *in_ids, const uint32_t *in_counts, uint64_t g_rows, size_t g_k) {
    return graph_attach(ix, in_ids, in_counts, g_rows, g_k, true, nullptr, "zh_index_set_graph");
}

extern "C" int zh_index_set_graph_device(zh_index *ix, const uint64_t *d_in_ids, const uint32_t *d_in_counts, uint64_t g_rows, size_t g_k, void *stream) {
    return graph_attach(ix, d_in_ids, d_in_counts, g_rows, g_k, false, stream, "zh_index_set_graph_device");
}

extern "C" int zh_index_drop_graph(zh_index *ix) {
    if (!ix) return fail(ZH_EINVAL, "zh_index_drop_graph: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->graph.attached) HIPCHK(hipDeviceSynchronize());  // (nothing of an earlier call on a caller's stream is left reading the table)
    ix->graph.drop();
    return ZH_OK;
}

extern "C" int zh_index_graph_info(const zh_index *ix, zh_graph_info *out) {
    if (!ix || !out) return fail(ZH_EINVAL, "zh_index_graph_info: null argument");
    zh_index *m = const_cast<zh_index *>(ix);
    std::shared_lock<std::shared_mutex> lk(m->mu);
    zh_graph_info g{};
    g.attached = m->graph.attached ? 1u : 0u;
    g.g_k = m->graph.k;
    g.g_rows = m->graph.rows;
    g.bytes = m->graph.attached ? m->graph.tab.cap : 0;
    *out = g;
    return ZH_OK;
}

// judged before any device is touched, in this order of kinds: null index (even for b = 0), null pointers of a non-empty request, the metric, a zero
// top_k / beam / width / n_seed, then the limits: beam, top_k against beam, n_seed, width (against 256: g_k is only known under the lock), max_iters
// (the filtered entries: a null filter that speaks for rows is one of the null pointers, whatever b; the unfiltered ones pass null and 0), and last,
// for the steered entries, hops (ZH_EINVAL unless 1 or 2; the others pass 1)
static int gsearch_args(zh_index *ix, const void *q, size_t b, const void *seeds, size_t n_seed, size_t top_k, size_t beam, size_t width, size_t max_iters,
                        int metric, int mode, const void *filter, uint64_t n_bits, const void *ids, const void *keys, const void *counts, const char *who,
                        int hops = 1) {
    if (!ix || (b && (!q || !seeds || !ids || !keys || !counts))) return fail(ZH_EINVAL, "%s: null argument", who);
    if (n_bits && !filter) return fail(ZH_EINVAL, "%s: null filter for %llu rows", who, (unsigned long long)n_bits);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (!top_k) return fail(ZH_EINVAL, "%s: top_k is 0", who);
    if (!beam) return fail(ZH_EINVAL, "%s: beam is 0", who);
    if (!width) return fail(ZH_EINVAL, "%s: width is 0", who);
    if (!n_seed) return fail(ZH_EINVAL, "%s: n_seed is 0", who);
    if (beam > ZH_GRAPH_MAX_BEAM) return fail(ZH_ELIMIT, "%s: beam %zu > ZH_GRAPH_MAX_BEAM (%u)", who, beam, ZH_GRAPH_MAX_BEAM);
    if (top_k > beam) return fail(ZH_ELIMIT, "%s: top_k %zu > beam %zu", who, top_k, beam);
    if (n_seed > ZH_GRAPH_MAX_SEEDS) return fail(ZH_ELIMIT, "%s: n_seed %zu > ZH_GRAPH_MAX_SEEDS (%u)", who, n_seed, ZH_GRAPH_MAX_SEEDS);
    if (width > 256) return fail(ZH_ELIMIT, "%s: width %zu > 256", who, width);
    if (max_iters > ZH_GRAPH_MAX_ITERS) return fail(ZH_ELIMIT, "%s: max_iters %zu > ZH_GRAPH_MAX_ITERS (%u)", who, max_iters, ZH_GRAPH_MAX_ITERS);
    if (hops != 1 && hops != 2) return fail(ZH_EINVAL, "%s: hops %d is neither 1 nor 2", who, hops);
    return ZH_OK;
}

// all six entry points once the arguments have been judged (b > 0).  host: q, seeds, the filter and the outputs are HOST arrays -- each internal batch
// goes through the staging and is waited for; otherwise they are device arrays, waited for once after the last batch.  flt (the filtered entries):
// the caller's bitmap; the filter pass runs once, on the call's stream, into the filtered exact search's buffers, and its count comes back with the
// counters.  Without flt nothing of that is touched.  flt->hops (the steered entries): the walk itself reads the pass's bitmap, 1 or 2 hops wide;
// 0 is the blind walk answered from the allowed rows.
struct GsearchFilter {
    const uint32_t *words;
    uint64_t n_bits;
    uint32_t hops;
};
static int gsearch_call(zh_index *ix, const float *q, size_t b, const uint64_t *seeds, uint32_t n_seed, uint32_t top_k, uint32_t beam, uint32_t width,
                        uint32_t max_iters, int metric, int mode, const GsearchFilter *flt, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts, bool host,
                        void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix))) return rc;
    if (!ix->graph.attached) return fail(ZH_ESTATE, "%s: no graph is attached to the index (zh_index_set_graph)", who);
    const uint32_t g_k = ix->graph.k, d = ix->opt.dim;
    if ((uint64_t)width * g_k > 256) return fail(ZH_ELIMIT, "%s: width %u * g_k %u > 256", who, width, g_k);
    if (ix->n_rows >= (1ull << 31)) return fail(ZH_ELIMIT, "%s: %llu stored rows; graph search serves tables below 2^31 rows", who, (unsigned long long)ix->n_rows);
    if (flt && (rc = filtered_bits_fit(ix, flt->n_bits))) return rc;
    if ((rc = exact_live_rows(ix))) return rc;
    ScratchGuard guard{ix, flt ? SCRATCH_GSEARCH_FILTERED : SCRATCH_GSEARCH};
    const hipStream_t s = call_stream(ix, stream);
    const bool steer = flt && flt->hops;
    const size_t nb_max = std::min<size_t>(ZH_GRAPH_BATCH, b), ctr_bytes = steer ? 80 : flt ? 56 : 40;  // (five counters, seven under a filter, ten steered)
    if ((rc = ix->gs_QQ.ensure(nb_max * 4)) || (rc = ix->gs_ctr.ensure(ctr_bytes))) return rc;
    if (host && ((rc = ix->gs_Q.ensure(nb_max * d * 4)) || (rc = ix->gs_seeds.ensure(nb_max * n_seed * 8)) || (rc = ix->gs_oids.ensure(nb_max * top_k * 8)) ||
                 (rc = ix->gs_okeys.ensure(nb_max * top_k * 8)) || (rc = ix->gs_ocounts.ensure(nb_max * 4))))
        return rc;
    HIPCHK(hipMemsetAsync(ix->gs_ctr.p, 0, ctr_bytes, s));
    const uint32_t *dAllow = nullptr, *dAllowed = nullptr;  // the allowed-AND-live bitmap; its count
    if (flt) {
        const uint64_t n = ix->n_rows;
        const size_t fblocks = (size_t)((n + ZH_FILTER_BLOCK_ROWS - 1) / ZH_FILTER_BLOCK_ROWS), fwords = (size_t)((flt->n_bits + 31) / 32);
        if ((rc = ix->fl_bits.ensure(std::max<size_t>((n + 63) / 64 * 8, 8))) || (rc = ix->fl_bcount.ensure(std::max<size_t>(fblocks, 1) * 4)) ||
            (rc = ix->fl_bexcl.ensure((fblocks + 2) * 4)) || (rc = ix->fl_tmp.ensure((fblocks / 1024 + 2) * 4)))
            return rc;
        const uint32_t *dFilter = flt->words;
        if (host) {
            if ((rc = ix->fl_filter.ensure(std::max<size_t>(fwords, 1) * 4))) return rc;
            if (fwords) HIPCHK(hipMemcpyAsync(ix->fl_filter.p, flt->words, fwords * 4, hipMemcpyHostToDevice, s));
            dFilter = ix->fl_filter.as<uint32_t>();
        }
        uint32_t *excl = ix->fl_bexcl.as<uint32_t>();  // [0, fblocks]: the blocks' exclusive sums, the last one the count; then the tile count (not read)
        HIPCHK(zh_launch_filter_and(dFilter, flt->n_bits, ix->live_dev.bits.as<uint32_t>(), n, ix->fl_bits.as<uint32_t>(), ix->fl_bcount.as<uint32_t>(), excl,
                                    ix->fl_tmp.as<uint32_t>(), excl + fblocks + 1, s));
        dAllow = ix->fl_bits.as<uint32_t>();
        dAllowed = excl + fblocks;
    }
    zh_graph_filtered_info inf{};
    const int param = score_param(metric, mode);
    for (size_t b0 = 0; b0 < b; b0 += ZH_GRAPH_BATCH) {
        const uint32_t nb = (uint32_t)std::min<size_t>(ZH_GRAPH_BATCH, b - b0);
        const float *dQ = q + b0 * d;
        const uint64_t *dSeeds = seeds + b0 * n_seed;
        uint64_t *dIds = out_ids + b0 * top_k, *dKeys = out_keys + b0 * top_k;
        uint32_t *dCounts = out_counts + b0;
        if (host) {
            HIPCHK(hipMemcpyAsync(ix->gs_Q.p, dQ, (size_t)nb * d * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(ix->gs_seeds.p, dSeeds, (size_t)nb * n_seed * 8, hipMemcpyHostToDevice, s));
            dQ = ix->gs_Q.as<float>(); dSeeds = ix->gs_seeds.as<uint64_t>();
            dIds = ix->gs_oids.as<uint64_t>(); dKeys = ix->gs_okeys.as<uint64_t>(); dCounts = ix->gs_ocounts.as<uint32_t>();
        }
        if (metric == ZH_COSINE) HIPCHK(zh_launch_qnorm(dQ, nb, d, ix->gs_QQ.as<float>(), s));  // (the exact search's norm of the query)
        if (steer)
            HIPCHK(zh_launch_gsearch_steered(ix->X.as<float>(), d, ix->n_rows, ix->graph.tab.as<uint32_t>(), ix->graph.rows, g_k, ix->live_dev.bits.as<uint32_t>(),
                                             dAllow, dQ, ix->gs_QQ.as<float>(), dSeeds, n_seed, nb, ix->opt.id_base, top_k, beam, width, max_iters, flt->hops, metric,
                                             param, dIds, dKeys, dCounts, ix->gs_ctr.as<unsigned long long>(), s));
        else
            HIPCHK(zh_launch_gsearch(ix->X.as<float>(), d, ix->n_rows, ix->graph.tab.as<uint32_t>(), ix->graph.rows, g_k, ix->live_dev.bits.as<uint32_t>(), dAllow,
                                     dQ, ix->gs_QQ.as<float>(), dSeeds, n_seed, nb, ix->opt.id_base, top_k, beam, width, max_iters, metric, param, dIds, dKeys,
                                     dCounts, ix->gs_ctr.as<unsigned long long>(), s));
        inf.launches++;
        if (host) {
            HIPCHK(hipMemcpyAsync(out_ids + b0 * top_k, dIds, (size_t)nb * top_k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_keys + b0 * top_k, dKeys, (size_t)nb * top_k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_counts + b0, dCounts, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    unsigned long long ctr[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t allowed = 0;
    HIPCHK(hipMemcpyAsync(ctr, ix->gs_ctr.p, ctr_bytes, hipMemcpyDeviceToHost, s));
    if (flt) HIPCHK(hipMemcpyAsync(&allowed, dAllowed, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    inf.queries = b;
    inf.seeds = ctr[0]; inf.iterations = ctr[1]; inf.expanded = ctr[2]; inf.keyed = ctr[3]; inf.capped = ctr[4];
    inf.rows_allowed = allowed; inf.offered = ctr[5]; inf.returned = ctr[6];
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    if (steer) {
        zh_graph_steered_info g{};
        g.queries = inf.queries; g.seeds = inf.seeds; g.iterations = inf.iterations; g.expanded = inf.expanded; g.keyed = inf.keyed; g.capped = inf.capped;
        g.launches = inf.launches; g.rows_allowed = allowed;
        g.direct = ctr[5]; g.via_bridge = ctr[6]; g.bridges = ctr[7]; g.cand_full = ctr[8]; g.returned = ctr[9];
        ix->gt_info = g;
    } else if (flt) {
        ix->gf_info = inf;
    } else {
        zh_graph_search_info g{};
        g.queries = inf.queries; g.seeds = inf.seeds; g.iterations = inf.iterations; g.expanded = inf.expanded; g.keyed = inf.keyed; g.capped = inf.capped;
        g.launches = inf.launches;
        ix->gs_info = g;
    }
    return ZH_OK;
}

extern "C" int zh_search_graph_batch_device(zh_index *ix, const float *d_q, size_t b, const uint64_t *d_seeds, size_t n_seed, size_t top_k, size_t beam,
                                            size_t width, size_t max_iters, int metric, int mode, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                            uint32_t *d_out_counts, void *stream) {
    int rc = gsearch_args(ix, d_q, b, d_seeds, n_seed, top_k, beam, width, max_iters, metric, mode, nullptr, 0, d_out_ids, d_out_keys, d_out_counts,
                          "zh_search_graph_batch_device");
    if (rc || b == 0) return rc;
    return gsearch_call(ix, d_q, b, d_seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, nullptr,
                        d_out_ids, d_out_keys, d_out_counts, false, stream, "zh_search_graph_batch_device");
}

extern "C" int zh_search_graph_batch(zh_index *ix, const float *q, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k, size_t beam, size_t width,
                                     size_t max_iters, int metric, int mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts) {
    int rc = gsearch_args(ix, q, b, seeds, n_seed, top_k, beam, width, max_iters, metric, mode, nullptr, 0, out_ids, out_keys, out_counts, "zh_search_graph_batch");
    if (rc || b == 0) return rc;
    return gsearch_call(ix, q, b, seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, nullptr, out_ids,
                        out_keys, out_counts, true, nullptr, "zh_search_graph_batch");
}

extern "C" int zh_search_graph_info(const zh_index *ix, zh_graph_search_info *out) {
    return get_info(ix, &zh_index::gs_info, out, "zh_search_graph_info");
}

// filtered graph search: the same walk, answered from the allowed rows it keyed.  DESIGN.md s26
extern "C" int zh_search_graph_filtered_batch_device(zh_index *ix, const float *d_q, size_t b, const uint64_t *d_seeds, size_t n_seed, size_t top_k, size_t beam,
                                                     size_t width, size_t max_iters, int metric, int mode, const uint32_t *d_filter, uint64_t n_bits,
                                                     uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    const char *who = "zh_search_graph_filtered_batch_device";
    int rc = gsearch_args(ix, d_q, b, d_seeds, n_seed, top_k, beam, width, max_iters, metric, mode, d_filter, n_bits, d_out_ids, d_out_keys, d_out_counts, who);
    if (rc || b == 0) return rc;
    const GsearchFilter flt{d_filter, n_bits, 0};
    return gsearch_call(ix, d_q, b, d_seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, &flt, d_out_ids,
                        d_out_keys, d_out_counts, false, stream, who);
}

extern "C" int zh_search_graph_filtered_batch(zh_index *ix, const float *q, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k, size_t beam, size_t width,
                                              size_t max_iters, int metric, int mode, const uint32_t *filter, uint64_t n_bits, uint64_t *out_ids,
                                              uint64_t *out_keys, uint32_t *out_counts) {
    const char *who = "zh_search_graph_filtered_batch";
    int rc = gsearch_args(ix, q, b, seeds, n_seed, top_k, beam, width, max_iters, metric, mode, filter, n_bits, out_ids, out_keys, out_counts, who);
    if (rc || b == 0) return rc;
    const GsearchFilter flt{filter, n_bits, 0};
    return gsearch_call(ix, q, b, seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, &flt, out_ids,
                        out_keys, out_counts, true, nullptr, who);
}

extern "C" int zh_search_graph_filtered_info(const zh_index *ix, zh_graph_filtered_info *out) {
    return get_info(ix, &zh_index::gf_info, out, "zh_search_graph_filtered_info");
}

// filter-steered graph search: the walk keeps to the allowed rows and hops over the others.  DESIGN.md s28
extern "C" int zh_search_graph_steered_batch_device(zh_index *ix, const float *d_q, size_t b, const uint64_t *d_seeds, size_t n_seed, size_t top_k, size_t beam,
                                                    size_t width, size_t max_iters, int metric, int mode, const uint32_t *d_filter, uint64_t n_bits, int hops,
                                                    uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    const char *who = "zh_search_graph_steered_batch_device";
    int rc = gsearch_args(ix, d_q, b, d_seeds, n_seed, top_k, beam, width, max_iters, metric, mode, d_filter, n_bits, d_out_ids, d_out_keys, d_out_counts, who, hops);
    if (rc || b == 0) return rc;
    const GsearchFilter flt{d_filter, n_bits, (uint32_t)hops};
    return gsearch_call(ix, d_q, b, d_seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, &flt, d_out_ids,
                        d_out_keys, d_out_counts, false, stream, who);
}

extern "C" int zh_search_graph_steered_batch(zh_index *ix, const float *q, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k, size_t beam, size_t width,
                                             size_t max_iters, int metric, int mode, const uint32_t *filter, uint64_t n_bits, int hops, uint64_t *out_ids,
                                             uint64_t *out_keys, uint32_t *out_counts) {
    const char *who = "zh_search_graph_steered_batch";
    int rc = gsearch_args(ix, q, b, seeds, n_seed, top_k, beam, width, max_iters, metric, mode, filter, n_bits, out_ids, out_keys, out_counts, who, hops);
    if (rc || b == 0) return rc;
    const GsearchFilter flt{filter, n_bits, (uint32_t)hops};
    return gsearch_call(ix, q, b, seeds, (uint32_t)n_seed, (uint32_t)top_k, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, metric, mode, &flt, out_ids,
                        out_keys, out_counts, true, nullptr, who);
}

extern "C" int zh_search_graph_steered_info(const zh_index *ix, zh_graph_steered_info *out) {
    return get_info(ix, &zh_index::gt_info, out, "zh_search_graph_steered_info");
}

// ------------------------------------------------------------------------------------------------
// extending the attached graph over the rows stored since the attach, and reading the table back (zh_gextend.hip).  DESIGN.md s27
// ------------------------------------------------------------------------------------------------
// judged before any device is touched, in this order of kinds: null index, null seeds of new rows, the metric, a zero beam / width / n_seed / batch,
// then the limits: beam, n_seed, width (against 256: g_k is only known under the lock), max_iters, batch
static int gextend_args(zh_index *ix, const void *seeds, uint64_t n_new, size_t n_seed, size_t beam, size_t width, size_t max_iters, size_t batch, int metric,
                        int mode, const char *who) {
    if (!ix || (n_new && !seeds)) return fail(ZH_EINVAL, "%s: null argument", who);
    const int rc = check_metric(metric, mode);
    if (rc) return rc;
    if (!beam) return fail(ZH_EINVAL, "%s: beam is 0", who);
    if (!width) return fail(ZH_EINVAL, "%s: width is 0", who);
    if (!n_seed) return fail(ZH_EINVAL, "%s: n_seed is 0", who);
    if (!batch) return fail(ZH_EINVAL, "%s: batch is 0", who);
    if (beam > ZH_GRAPH_MAX_BEAM) return fail(ZH_ELIMIT, "%s: beam %zu > ZH_GRAPH_MAX_BEAM (%u)", who, beam, ZH_GRAPH_MAX_BEAM);
    if (n_seed > ZH_GRAPH_MAX_SEEDS) return fail(ZH_ELIMIT, "%s: n_seed %zu > ZH_GRAPH_MAX_SEEDS (%u)", who, n_seed, ZH_GRAPH_MAX_SEEDS);
    if (width > 256) return fail(ZH_ELIMIT, "%s: width %zu > 256", who, width);
    if (max_iters > ZH_GRAPH_MAX_ITERS) return fail(ZH_ELIMIT, "%s: max_iters %zu > ZH_GRAPH_MAX_ITERS (%u)", who, max_iters, ZH_GRAPH_MAX_ITERS);
    if (batch > ZH_GRAPH_EXTEND_MAX_BATCH) return fail(ZH_ELIMIT, "%s: batch %zu > ZH_GRAPH_EXTEND_MAX_BATCH (%u)", who, batch, ZH_GRAPH_EXTEND_MAX_BATCH);
    return ZH_OK;
}

// The chunks (under mu, exclusive; exact_live_rows has run; N > G): tab [N][g_k] receives the old table, then chunk by chunk the new lines and the
// re-ranked old ones.  dSeeds: the [N - G][n_seed] seeds on the device.  Everything is enqueued on s and nothing is waited for but the counters.
static int gextend_chunks(zh_index *ix, uint32_t *tab, const uint64_t *dSeeds, uint32_t n_seed, uint32_t beam, uint32_t width, uint32_t max_iters, uint32_t batch,
                          int metric, int mode, hipStream_t s, zh_graph_extend_info *inf) {
    const uint64_t G = ix->graph.rows, N = ix->n_rows;
    const uint32_t g_k = ix->graph.k, d = ix->opt.dim;
    const int param = score_param(metric, mode);
    const size_t nb_max = (size_t)std::min<uint64_t>(batch, N - G), edges = nb_max * g_k;
    int rc;
    if ((rc = ix->gs_Q.ensure(nb_max * d * 4)) || (rc = ix->gs_QQ.ensure(nb_max * 4)) || (rc = ix->ge_seeds.ensure(nb_max * n_seed * 8)) ||
        (rc = ix->ge_ids.ensure(edges * 8)) || (rc = ix->ge_keys.ensure(edges * 8)) || (rc = ix->ge_counts.ensure(nb_max * 4)) || (rc = ix->ge_deg.ensure(N * 4)) ||
        (rc = ix->ge_cur.ensure(N * 4)) || (rc = ix->ge_off.ensure((N + 1) * 8)) || (rc = ix->ge_sums.ensure((N / 4096 + 1) * 8)) || (rc = ix->ge_csr.ensure(edges * 4)) ||
        (rc = ix->ge_touched.ensure(edges * 4)) || (rc = ix->ge_ctr.ensure(88)))
        return rc;
    unsigned long long *dCtr = ix->ge_ctr.as<unsigned long long>();  // [0..4] the walk's, [5] a chunk's touched rows, [6..8] re-ranked / offered / kept, [9..10] the transposition's
    HIPCHK(hipMemsetAsync(dCtr, 0, 88, s));
    if (G) HIPCHK(hipMemcpyAsync(tab, ix->graph.tab.p, (size_t)G * g_k * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemsetAsync(tab + (size_t)G * g_k, 0xFF, (size_t)(N - G) * g_k * 4, s));  // (a removed new row's line stays empty)
    if (metric == ZH_COSINE) {  // every stored row's squared norm: a re-ranked row's, as zh_launch_qnorm gives it to the exact search
        if ((rc = ix->ge_qq.ensure(N * 4))) return rc;
        for (uint64_t r0 = 0; r0 < N; r0 += 1ull << 30)
            HIPCHK(zh_launch_qnorm(ix->X.as<float>() + r0 * d, (uint32_t)std::min<uint64_t>(1ull << 30, N - r0), d, ix->ge_qq.as<float>() + r0, s));
    }
    const uint32_t *dBits = ix->live_dev.bits.as<uint32_t>();
    LiveCursor live;
    for (uint64_t lo = G; lo < N; lo += batch) {
        const uint64_t hi = std::min<uint64_t>(N, lo + batch), l0 = live_before(ix, lo, &live), l1 = live_before(ix, hi, &live);
        const uint32_t B = (uint32_t)(l1 - l0);
        inf->chunks++;
        inf->rows_added += B;
        inf->rows_removed += (hi - lo) - B;
        if (!B) continue;
        const uint32_t *dRows = ix->live_dev.rows.as<uint32_t>() + l0;
        // ---- step 1: the chunk's live rows as queries of the walk over [0, lo)
        HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, dRows, B, ix->gs_Q.as<float>(), s));
        HIPCHK(zh_launch_gext_seeds(dSeeds, dRows, B, G, n_seed, ix->ge_seeds.as<uint64_t>(), s));
        if (metric == ZH_COSINE) HIPCHK(zh_launch_qnorm(ix->gs_Q.as<float>(), B, d, ix->gs_QQ.as<float>(), s));
        HIPCHK(zh_launch_gsearch(ix->X.as<float>(), d, lo, tab, lo, g_k, dBits, nullptr, ix->gs_Q.as<float>(), ix->gs_QQ.as<float>(), ix->ge_seeds.as<uint64_t>(), n_seed,
                                 B, ix->opt.id_base, g_k, beam, width, max_iters, metric, param, ix->ge_ids.as<uint64_t>(), ix->ge_keys.as<uint64_t>(),
                                 ix->ge_counts.as<uint32_t>(), dCtr, s));
        HIPCHK(zh_launch_gext_lines(ix->ge_ids.as<uint64_t>(), ix->ge_counts.as<uint32_t>(), dRows, B, g_k, ix->opt.id_base, tab, s));
        inf->launches++;
        if (!lo) continue;  // (no row before the chunk: every line of it is empty)
        // ---- step 2: the chunk's lines transposed over [0, lo), the rows they name re-ranked
        HIPCHK(hipMemsetAsync(dCtr + 5, 0, 8, s));
        HIPCHK(zh_launch_reverse_csr_lines(tab, dBits, lo, g_k, lo, hi - lo, ix->ge_deg.as<uint32_t>(), ix->ge_cur.as<uint32_t>(), ix->ge_off.as<uint64_t>(),
                                           ix->ge_sums.as<uint64_t>(), ix->ge_csr.as<uint32_t>(), dCtr + 9, s));
        HIPCHK(zh_launch_gext_rerank(ix->X.as<float>(), d, tab, g_k, lo, (uint32_t)(hi - lo), dBits, ix->ge_qq.as<float>(), ix->ge_off.as<uint64_t>(),
                                     ix->ge_csr.as<uint32_t>(), ix->ge_touched.as<uint32_t>(), metric, param, dCtr + 5, s));
        inf->launches++;
    }
    unsigned long long ctr[9];
    HIPCHK(hipMemcpyAsync(ctr, dCtr, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    inf->seeds = ctr[0]; inf->iterations = ctr[1]; inf->expanded = ctr[2]; inf->keyed = ctr[3]; inf->capped = ctr[4];
    inf->reverse_rows = ctr[6]; inf->reverse_offered = ctr[7]; inf->reverse_kept = ctr[8];
    return ZH_OK;
}

// both entry points once the arguments have been judged.  host: seeds is a HOST array, staged whole
static int gextend_call(zh_index *ix, const uint64_t *seeds, uint64_t n_new, uint32_t n_seed, uint32_t beam, uint32_t width, uint32_t max_iters, uint32_t batch,
                        int metric, int mode, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix))) return rc;
    if (!ix->graph.attached) return fail(ZH_ESTATE, "%s: no graph is attached to the index (zh_index_set_graph)", who);
    const uint64_t G = ix->graph.rows, N = ix->n_rows;
    const uint32_t g_k = ix->graph.k;
    if (g_k > beam) return fail(ZH_ELIMIT, "%s: g_k %u > beam %u", who, g_k, beam);
    if ((uint64_t)width * g_k > 256) return fail(ZH_ELIMIT, "%s: width %u * g_k %u > 256", who, width, g_k);
    if (N >= (1ull << 31)) return fail(ZH_ELIMIT, "%s: %llu stored rows; graph search serves tables below 2^31 rows", who, (unsigned long long)N);
    if (n_new != N - G)
        return fail(ZH_EINVAL, "%s: n_new %llu, but %llu rows were stored since the graph's %llu", who, (unsigned long long)n_new, (unsigned long long)(N - G),
                    (unsigned long long)G);
    zh_graph_extend_info inf{};
    if (N > G) {
        if ((rc = exact_live_rows(ix))) return rc;
        ScratchGuard guard{ix, SCRATCH_GEXTEND};
        const hipStream_t s = call_stream(ix, stream);
        DevBuf tab;
        if ((rc = tab.ensure((size_t)N * g_k * 4))) return rc;
        const uint64_t *dSeeds = seeds;
        if (host && !(rc = ix->gs_seeds.ensure((size_t)n_new * n_seed * 8))) {
            if (hipMemcpyAsync(ix->gs_seeds.p, seeds, (size_t)n_new * n_seed * 8, hipMemcpyHostToDevice, s) != hipSuccess) rc = fail(ZH_EHIP, "%s: the seeds' copy failed", who);
            dSeeds = ix->gs_seeds.as<uint64_t>();
        }
        if (!rc) rc = gextend_chunks(ix, tab.as<uint32_t>(), dSeeds, n_seed, beam, width, max_iters, batch, metric, mode, s, &inf);
        if (rc) {  // what was attached stays
            hipStreamSynchronize(s);
            tab.release();
            return rc;
        }
        ix->graph.drop();
        ix->graph.tab = tab;
        ix->graph.mark_attached(N, g_k);
    }
    std::lock_guard<std::mutex> ls(ix->stats_mu);
    ix->ge_info = inf;
    return ZH_OK;
}

extern "C" int zh_index_extend_graph_device(zh_index *ix, const uint64_t *d_seeds, uint64_t n_new, size_t n_seed, size_t beam, size_t width, size_t max_iters,
                                            size_t batch, int metric, int mode, void *stream) {
    const char *who = "zh_index_extend_graph_device";
    int rc = gextend_args(ix, d_seeds, n_new, n_seed, beam, width, max_iters, batch, metric, mode, who);
    if (rc) return rc;
    return gextend_call(ix, d_seeds, n_new, (uint32_t)n_seed, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, (uint32_t)batch, metric, mode, false, stream, who);
}

extern "C" int zh_index_extend_graph(zh_index *ix, const uint64_t *seeds, uint64_t n_new, size_t n_seed, size_t beam, size_t width, size_t max_iters, size_t batch,
                                     int metric, int mode) {
    const char *who = "zh_index_extend_graph";
    int rc = gextend_args(ix, seeds, n_new, n_seed, beam, width, max_iters, batch, metric, mode, who);
    if (rc) return rc;
    return gextend_call(ix, seeds, n_new, (uint32_t)n_seed, (uint32_t)beam, (uint32_t)width, (uint32_t)max_iters, (uint32_t)batch, metric, mode, true, nullptr, who);
}

extern "C" int zh_index_extend_graph_info(const zh_index *ix, zh_graph_extend_info *out) {
    return get_info(ix, &zh_index::ge_info, out, "zh_index_extend_graph_info");
}

#define ZH_GRAPH_READ_SLAB (1ull << 18)  // lines the host entry of zh_index_get_graph stages at a time
// both read-back entry points.  host: the outputs are HOST arrays, answered slab by slab through graph search's staging
static int graph_read(zh_index *ix, uint64_t first_row, uint64_t n, uint64_t *out_ids, uint32_t *out_counts, bool host, void *stream, const char *who) {
    if (!ix || (n && (!out_ids || !out_counts))) return fail(ZH_EINVAL, "%s: null argument", who);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix))) return rc;
    if (!ix->graph.attached) return fail(ZH_ESTATE, "%s: no graph is attached to the index (zh_index_set_graph)", who);
    if (first_row > ix->graph.rows || n > ix->graph.rows - first_row)
        return fail(ZH_EINVAL, "%s: lines [%llu, %llu + %llu) of a graph of %llu", who, (unsigned long long)first_row, (unsigned long long)first_row,
                    (unsigned long long)n, (unsigned long long)ix->graph.rows);
    if (!n) return ZH_OK;
    const uint32_t g_k = ix->graph.k;
    const hipStream_t s = call_stream(ix, stream);
    const uint32_t *tab = ix->graph.tab.as<uint32_t>();
    if (!host) {
        HIPCHK(zh_launch_gext_read(tab, g_k, first_row, n, ix->opt.id_base, out_ids, out_counts, s));
        HIPCHK(hipStreamSynchronize(s));
        return ZH_OK;
    }
    ScratchGuard guard{ix, SCRATCH_GSEARCH};
    const uint64_t slab = std::min<uint64_t>(n, ZH_GRAPH_READ_SLAB);
    if ((rc = ix->gs_oids.ensure((size_t)slab * g_k * 8)) || (rc = ix->gs_ocounts.ensure((size_t)slab * 4))) return rc;
    for (uint64_t r0 = 0; r0 < n; r0 += slab) {
        const uint64_t m = std::min(slab, n - r0);
        HIPCHK(zh_launch_gext_read(tab, g_k, first_row + r0, m, ix->opt.id_base, ix->gs_oids.as<uint64_t>(), ix->gs_ocounts.as<uint32_t>(), s));
        HIPCHK(hipMemcpyAsync(out_ids + r0 * g_k, ix->gs_oids.p, (size_t)m * g_k * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_counts + r0, ix->gs_ocounts.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return ZH_OK;
}

extern "C" int zh_index_get_graph(zh_index *ix, uint64_t first_row, uint64_t n, uint64_t *out_ids, uint32_t *out_counts) {
    return graph_read(ix, first_row, n, out_ids, out_counts, true, nullptr, "zh_index_get_graph");
}

extern "C" int zh_index_get_graph_device(zh_index *ix, uint64_t first_row, uint64_t n, uint64_t *d_out_ids, uint32_t *d_out_counts, void *stream) {
    return graph_read(ix, first_row, n, d_out_ids, d_out_counts, false, stream, "zh_index_get_graph_device");
}

// ------------------------------------------------------------------------------------------------
// forest self-join (zh_fjoin.hip): every pair of leaf-mates whose key is <= one threshold key, each pair once.  DESIGN.md s18
// ------------------------------------------------------------------------------------------------
#define ZH_FJOIN_CAND_FLOOR 256u  // path 2: candidate slots per gathered row of a batch that are there whatever the capacity

struct FjoinRun : ForestRun {
    int metric = 0, mode = 0;
    uint64_t max_key = 0, pool_cap = 0;
    bool env_cand = false;          // ZH_FJOIN_CAND_CAP is set ...
    uint64_t env_cand_cap = 0;      // ... to this
};

// The path rule and path 2's views, every tree's leaves (both paths go by them), the node -> tree map and each row's leaf per tree on the device.
// jn_ctr: {hits, the batch's candidates, the forest's leaf pairs, candidates that got a key}
static int fjoin_setup(zh_index *ix, int metric, int mode, hipStream_t s, FjoinRun *run) {
    int rc;
    if ((rc = forest_path2(ix, "ZH_FJOIN_PATH", metric, s, run))) return rc;
    const std::vector<uint32_t> node_tree = forest_walk(ix, &run->leaves);
    if ((rc = ix->fk_ntree.ensure(node_tree.size() * 4)) || (rc = ix->jn_ctr.ensure(32)) ||
        (rc = ix->fj_leafof.ensure(std::max<size_t>((size_t)ix->n_rows * run->T * 4, 4))))
        return rc;
    HIPCHK(hipMemcpyAsync(ix->fk_ntree.p, node_tree.data(), node_tree.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ix->jn_ctr.p, 0, 32, s));
    HIPCHK(zh_launch_fjoin_rowleaf(ix->node_pack.as<int4>(), ix->fk_ntree.as<uint32_t>(), ix->n_nodes, ix->leaf_ids.as<uint32_t>(), run->T, ix->n_rows,
                                   ix->fj_leafof.as<uint32_t>(), ix->jn_ctr.as<unsigned long long>() + 2, s));
    HIPCHK(hipStreamSynchronize(s));  // (node_tree is this frame's)
    const char *env_c = getenv("ZH_FJOIN_CAND_CAP");
    if (env_c && atoll(env_c) > 0) { run->env_cand = true; run->env_cand_cap = (uint64_t)atoll(env_c); }
    return ZH_OK;
}

// Path 1 of one panel: its pieces' lines against their leaves.
static int fjoin_panel1(zh_index *ix, const FjoinRun &run, uint32_t t, const std::vector<ZhFjoinPiece> &pieces, uint32_t lines, uint32_t groups, uint64_t flat,
                        uint64_t keys, hipStream_t s, zh_join_forest_info *inf) {
    const uint32_t d = ix->opt.dim;
    int rc;
    if ((rc = ix->fj_pieces.ensure(pieces.size() * sizeof(ZhFjoinPiece))) || (rc = ix->fk_rows.ensure((size_t)lines * 4)) ||
        (rc = ix->fj_linel.ensure((size_t)lines * 8)) || (rc = ix->fj_linek.ensure((size_t)lines * 8)) ||
        (rc = ix->fk_groups.ensure((size_t)groups * sizeof(ZhGroup))) || (rc = ix->fk_groff.ensure((size_t)groups * 8)) ||
        (rc = ix->ex_Q.ensure((size_t)lines * d * 4)) || (rc = ix->ex_QQ.ensure((size_t)lines * 4)) || (rc = ix->ex_keys.ensure(std::max<uint64_t>(keys, 1) * 8)))
        return rc;
    const int param = score_param(run.metric, run.mode);
    HIPCHK(hipMemcpyAsync(ix->fj_pieces.p, pieces.data(), pieces.size() * sizeof(ZhFjoinPiece), hipMemcpyHostToDevice, s));
    HIPCHK(zh_launch_fjoin_groups(ix->fj_pieces.as<ZhFjoinPiece>(), (uint32_t)pieces.size(), groups, ix->leaf_ids.as<uint32_t>(), ix->n_rows,
                                  ix->fk_rows.as<uint32_t>(), ix->fj_linel.as<uint2>(), ix->fj_linek.as<uint64_t>(), ix->fk_groups.as<ZhGroup>(),
                                  ix->fk_groff.as<uint64_t>(), s));
    HIPCHK(zh_launch_join_gather(ix->X.as<float>(), d, ix->fk_rows.as<uint32_t>(), lines, ix->ex_Q.as<float>(), s));
    HIPCHK(zh_launch_qnorm(ix->ex_Q.as<float>(), lines, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_sweep(ix->X.as<float>(), d, ix->ex_Q.as<float>(), ix->ex_QQ.as<float>(), ix->fk_groups.as<ZhGroup>(), ix->fk_groff.as<uint64_t>(), groups,
                           nullptr, ix->leaf_ids.as<uint32_t>(), flat, run.metric, param, ix->ex_keys.as<uint64_t>(), s));
    HIPCHK(zh_launch_fjoin_collect(ix->ex_keys.as<uint64_t>(), ix->fk_rows.as<uint32_t>(), ix->fj_linel.as<uint2>(), ix->fj_linek.as<uint64_t>(), lines,
                                   ix->leaf_ids.as<uint32_t>(), ix->n_rows, ix->fj_leafof.as<uint32_t>(), run.T, t, run.max_key,
                                   ix->jn_ctr.as<unsigned long long>(), ix->jn_pv0.as<uint64_t>(), ix->jn_pk0.as<uint64_t>(), run.pool_cap, s));
    HIPCHK(hipStreamSynchronize(s));  // (pieces is the caller's)
    inf->launches++;
    return ZH_OK;
}

// Path 1 for n leaves of tree t: every member of a leaf of two or more rows is a line that visits that leaf; panels of at most ZH_FJOIN_PANEL_LINES
// lines and ZH_FKNN_KEY_BUDGET keys (a longer leaf's lines are spread over panels; one line's leaf is the least a panel can hold).
static int fjoin_leaves1(zh_index *ix, const FjoinRun &run, uint32_t t, const uint2 *leaves, size_t n, hipStream_t s, zh_join_forest_info *inf) {
    std::vector<ZhFjoinPiece> pieces;
    uint32_t lines = 0, groups = 0;
    uint64_t flat = 0, keys = 0;
    int rc;
    auto flush = [&]() -> int {
        if (pieces.empty()) return ZH_OK;
        const int r = fjoin_panel1(ix, run, t, pieces, lines, groups, flat, keys, s, inf);
        pieces.clear(); lines = 0; groups = 0; flat = 0; keys = 0;
        return r;
    };
    for (size_t l = 0; l < n; l++) {
        const uint32_t off = leaves[l].x, len = leaves[l].y;
        if (len < 2) continue;
        for (uint32_t i0 = 0; i0 < len;) {
            uint64_t room = std::min<uint64_t>(ZH_FJOIN_PANEL_LINES - lines, (ZH_FKNN_KEY_BUDGET - std::min<uint64_t>(keys, ZH_FKNN_KEY_BUDGET)) / len);
            if (!room) {
                if (!pieces.empty()) { if ((rc = flush())) return rc; continue; }
                room = 1;
            }
            const uint32_t nl = (uint32_t)std::min<uint64_t>(len - i0, room), ng = (nl + ZH_GROUP_MAX - 1) / ZH_GROUP_MAX;
            pieces.push_back(ZhFjoinPiece{off, len, i0, nl, lines, groups, flat, keys});
            lines += nl; groups += ng; flat += (uint64_t)ng * len; keys += (uint64_t)nl * len;
            i0 += nl;
        }
    }
    return flush();
}

// Path 2 of one batch of leaves of tree t (leaves[l] at column tile col0[l] of the batch's NT tiles).  *hits = jn_ctr[0] afterwards.
static int fjoin_batch2(zh_index *ix, const FjoinRun &run, uint32_t t, const std::vector<uint2> &leaves, const std::vector<uint2> &colsrc, hipStream_t s,
                        zh_join_forest_info *inf, uint64_t *hits) {
    const uint32_t d = ix->opt.dim, NT = (uint32_t)colsrc.size();
    // tiles per chunk.  A leaf of ct tiles gives one segment per held block I0 = 0, 4, ... < ct with ceil((ct - I0) / ch) blocks: chunks are counted
    // from the held block's own diagonal
    const uint32_t ch = fill_chunk([&](uint32_t c) {
        uint32_t n_blocks = 0;
        for (const uint2 lf : leaves) {
            const uint32_t ct = (lf.y + 15) / 16;
            for (uint32_t I0 = 0; I0 < ct; I0 += 4) n_blocks += (ct - I0 + c - 1) / c;
        }
        return n_blocks;
    });
    std::vector<ZhFjoinSeg> segs;
    uint64_t products = 0, batch_pairs = 0;
    uint32_t col0 = 0, blocks = 0;
    for (const uint2 lf : leaves) {
        const uint32_t ct = (lf.y + 15) / 16;
        for (uint32_t I0 = 0; I0 < ct; I0 += 4) {
            segs.push_back(ZhFjoinSeg{col0, ct, I0, blocks});
            blocks += (ct - I0 + ch - 1) / ch;
        }
        products += (uint64_t)ct * (ct + 1) / 2;  // wave I issues ct - I
        batch_pairs += (uint64_t)lf.y * (lf.y - 1) / 2;
        col0 += ct;
    }
    const uint64_t pool_left = run.pool_cap > *hits ? run.pool_cap - *hits : 0;
    uint64_t cand_cap = std::min<uint64_t>(batch_pairs, std::max<uint64_t>(pool_left + pool_left / 4, (uint64_t)ZH_FJOIN_CAND_FLOOR * NT * 16));
    if (run.env_cand) cand_cap = run.env_cand_cap;
    int rc;
    if ((rc = ix->fj_segs.ensure(segs.size() * sizeof(ZhFjoinSeg))) || (rc = ix->fk_colsrc.ensure((size_t)NT * 8)) || (rc = ix->fk_crow.ensure((size_t)NT * 64)) ||
        (rc = ix->fk_CA.ensure((size_t)NT * 32 * d)) || (rc = ix->fk_cmeta.ensure((size_t)NT * 128)) || (rc = ix->fk_cqm.ensure((size_t)NT * 256)) ||
        (rc = ix->fj_cand.ensure(std::max<uint64_t>(cand_cap, 1) * 8)))
        return rc;
    unsigned long long *ctr = ix->jn_ctr.as<unsigned long long>();
    uint32_t *crow = ix->fk_crow.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(ix->fj_segs.p, segs.data(), segs.size() * sizeof(ZhFjoinSeg), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->fk_colsrc.p, colsrc.data(), (size_t)NT * 8, hipMemcpyHostToDevice, s));
    HIPCHK(zh_launch_fknn_cols(ix->fk_colsrc.as<uint2>(), NT, ix->leaf_ids.as<uint32_t>(), ix->n_rows, crow, s));
    HIPCHK(zh_launch_fknn_gather(d, run.v.Xh, run.v.rowMeta, run.pos, crow, NT, run.v.rho, ix->fk_CA.p, ix->fk_cmeta.as<float2>(), ix->fk_cqm.as<float4>(), s));
    HIPCHK(hipMemsetAsync(ctr + 1, 0, 8, s));
    HIPCHK(zh_launch_fjoin_mfma(d, run.metric, run.mode, ix->fj_segs.as<ZhFjoinSeg>(), (uint32_t)segs.size(), blocks, ch, ix->fk_CA.p, ix->fk_cmeta.as<float2>(),
                                ix->fk_cqm.as<float4>(), crow, run.Kc, run.v.rho, ix->jn_tau.as<uint32_t>(), ix->fj_cand.as<uint64_t>(), cand_cap, ctr + 1, s));
    inf->launches++;
    inf->tiles += products;
    HIPCHK(zh_launch_pair_survivors(ix->X.as<float>(), ix->X.as<float>(), d, run.metric, run.mode, ix->fj_cand.as<uint64_t>(), ctr + 1, cand_cap,
                                    ix->fj_leafof.as<uint32_t>(), run.T, t, run.max_key, ctr, ctr + 3, ix->jn_pv0.as<uint64_t>(), ix->jn_pk0.as<uint64_t>(),
                                    run.pool_cap, s));
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    bool kept = false;
    if ((rc = panel_tail(ix, 4, cand_cap, s, h_ctr, hits, &inf->redone, &kept))) return rc;  // (it waits: segs and colsrc are this frame's and the caller's)
    if (kept) {
        inf->candidates = h_ctr[3];
        return ZH_OK;
    }
    // the pool ran over: nothing of the batch was counted (pair_survivors_kernel left at once); ownership does not depend on the path, so path 1
    // over the same leaves counts exactly the batch's pairs
    if ((rc = fjoin_leaves1(ix, run, t, leaves.data(), leaves.size(), s, inf))) return rc;
    HIPCHK(hipMemcpyAsync(h_ctr, ctr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *hits = h_ctr[0];
    return ZH_OK;
}

// Path 2 of one tree: its non-empty leaves, in the host mirror's order, in batches of at most ZH_FKNN_COL_TILES tiles, or ONE longer leaf alone.
static int fjoin_tree2(zh_index *ix, const FjoinRun &run, uint32_t t, hipStream_t s, zh_join_forest_info *inf, uint64_t *hits) {
    std::vector<uint2> leaves, colsrc;
    int rc;
    for (const uint2 leaf : run.leaves[t]) {
        const uint32_t ct = (leaf.y + 15) / 16;
        if (!leaves.empty() && colsrc.size() + ct > ZH_FKNN_COL_TILES) {
            if ((rc = fjoin_batch2(ix, run, t, leaves, colsrc, s, inf, hits))) return rc;
            leaves.clear(); colsrc.clear();
        }
        leaves.push_back(leaf);
        for (uint32_t c = 0; c < ct; c++) colsrc.push_back(make_uint2(leaf.x + 16 * c, std::min<uint32_t>(16, leaf.y - 16 * c)));
    }
    if (!leaves.empty() && (rc = fjoin_batch2(ix, run, t, leaves, colsrc, s, inf, hits))) return rc;
    return ZH_OK;
}

// The call on the index's device (under mu, exclusive; exact_live_rows has run; the index has live rows and trees).  host_out as join_run.
static int fjoin_run(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *outA, uint64_t *outB, uint64_t *outKeys, bool host_out,
                     hipStream_t s, uint64_t *total, const char *who) {
    zh_join_forest_info inf{};
    inf.path = 1;
    inf.rows_live = ix->live_dev.n_live;
    inf.trees = ix->n_trees;
    FjoinRun run;
    run.metric = metric; run.mode = mode; run.max_key = max_key;
    int rc;
    if ((rc = fjoin_setup(ix, metric, mode, s, &run))) return rc;
    unsigned long long *ctr = ix->jn_ctr.as<unsigned long long>();
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h_ctr, ctr, 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    inf.leaf_pairs = h_ctr[2];
    uint64_t hits = 0;
    if (inf.leaf_pairs) {
        run.pool_cap = std::min<uint64_t>(capacity, inf.leaf_pairs);
        if ((rc = ix->jn_pv0.ensure(std::max<uint64_t>(run.pool_cap, 1) * 8)) || (rc = ix->jn_pk0.ensure(std::max<uint64_t>(run.pool_cap, 1) * 8))) return rc;
        if (run.path2) {
            inf.path = 2;
            if ((rc = ix->jn_tau.ensure(4)) || (rc = ix->jn_maxk.ensure(8))) return rc;
            HIPCHK(hipMemcpyAsync(ix->jn_maxk.p, &max_key, 8, hipMemcpyHostToDevice, s));
            HIPCHK(zh_launch_range_tau(ix->jn_maxk.as<uint64_t>(), 1, metric, mode, ix->jn_tau.as<uint32_t>(), s));
            HIPCHK(hipStreamSynchronize(s));  // (max_key is this frame's)
        }
        for (uint32_t t = 0; t < run.T; t++) {
            if (run.path2) { if ((rc = fjoin_tree2(ix, run, t, s, &inf, &hits))) return rc; }
            else if ((rc = fjoin_leaves1(ix, run, t, run.leaves[t].data(), run.leaves[t].size(), s, &inf))) return rc;
        }
        HIPCHK(hipMemcpyAsync(h_ctr, ctr, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        hits = h_ctr[0];
    }
    return join_finish(ix, ix, hits, capacity, outA, outB, outKeys, host_out, s, total, inf, &zh_index::fj_info, who);
}

// an index without live rows has no pair: total 0 (and the info says so) whatever its trees; otherwise the forest graph's state checks
static int fjoin_state(zh_index *ix, bool *empty, const char *who) {
    *empty = ix->live_dev.n_live == 0;
    if (*empty) {
        zh_join_forest_info inf{};
        inf.path = 1;
        inf.trees = ix->n_trees;
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->fj_info = inf;
        return ZH_OK;
    }
    return fknn_state(ix, who);
}

// both entry points once the arguments have been judged (host: the caller has zeroed the total, so an empty index ends the host call at once; the
// device call still writes its total of 0 on the stream)
static int fjoin_call(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b, uint64_t *out_keys,
                      uint64_t *out_total, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    bool empty = false;
    if ((rc = fjoin_state(ix, &empty, who)) || (empty && host)) return rc;
    ScratchGuard guard{ix, SCRATCH_FJOIN};
    const hipStream_t s = call_stream(ix, stream);
    uint64_t total = 0;
    if (!empty) rc = fjoin_run(ix, max_key, metric, mode, capacity, out_a, out_b, out_keys, host, s, &total, who);
    return join_total(rc, total, out_total, host, s);
}

extern "C" int zh_self_join_forest_device(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *d_out_a, uint64_t *d_out_b,
                                          uint64_t *d_out_keys, uint64_t *d_out_total, void *stream) {
    int rc = join_args(ix, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, "zh_self_join_forest_device");
    if (rc) return rc;
    return fjoin_call(ix, max_key, metric, mode, capacity, d_out_a, d_out_b, d_out_keys, d_out_total, false, stream, "zh_self_join_forest_device");
}

extern "C" int zh_self_join_forest(zh_index *ix, uint64_t max_key, int metric, int mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b, uint64_t *out_keys,
                                   uint64_t *out_total) {
    int rc = join_args(ix, metric, mode, capacity, out_a, out_b, out_keys, out_total, "zh_self_join_forest");
    if (rc) return rc;
    *out_total = 0;
    return fjoin_call(ix, max_key, metric, mode, capacity, out_a, out_b, out_keys, out_total, true, nullptr, "zh_self_join_forest");
}

extern "C" int zh_self_join_forest_info(const zh_index *ix, zh_join_forest_info *out) {
    return get_info(ix, &zh_index::fj_info, out, "zh_self_join_forest_info");
}

// ------------------------------------------------------------------------------------------------
// forest range search (zh_frange.hip): every member of the leaves the walk visits for a query whose key is <= the query's threshold key, each
// (query, row) once, as the range search's CSR.  DESIGN.md s19
// ------------------------------------------------------------------------------------------------
#define ZH_FRANGE_MIN_VISITORS 32u  // path 2 serves an internal batch whose visited leaves have at least this many visitors on average (s19: it lost at 4 and 15, won at 64)

struct FrangeRun : ForestRun {
    RangeRun rr;
    int metric = 0, mode = 0;
    uint32_t probe = 0;
    bool force2 = false;        // ZH_FRANGE_PATH=2: path 2 wherever the path rule admits it, whatever the visit gate says
    bool env_cand = false;      // ZH_FRANGE_CAND_CAP is set ...
    uint64_t env_cand_cap = 0;  // ... to this
    size_t log_chunks = 8192;   // the visit log's chunks (ZH_WALK_LOG_CHUNKS, read per call): a batch that logs more walks again, emitting
    std::vector<uint32_t> node_tree;
    const uint64_t *vsorted = nullptr;  // the internal batch's sorted visit words
    zh_range_forest_info inf{};
};

// The path rule and path 2's views, the node -> tree map on both sides and each row's leaf per tree on the device (the forest join's table).
static int frange_setup(zh_index *ix, hipStream_t s, FrangeRun *run) {
    int rc;
    if ((rc = forest_path2(ix, "ZH_FRANGE_PATH", run->metric, s, run))) return rc;
    run->node_tree = forest_walk(ix, nullptr);
    if ((rc = ix->fk_ntree.ensure(run->node_tree.size() * 4)) || (rc = ix->jn_ctr.ensure(32)) ||
        (rc = ix->fj_leafof.ensure(std::max<size_t>((size_t)ix->n_rows * run->T * 4, 4))))
        return rc;
    HIPCHK(hipMemcpyAsync(ix->fk_ntree.p, run->node_tree.data(), run->node_tree.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ix->jn_ctr.p, 0, 32, s));
    HIPCHK(zh_launch_fjoin_rowleaf(ix->node_pack.as<int4>(), ix->fk_ntree.as<uint32_t>(), ix->n_nodes, ix->leaf_ids.as<uint32_t>(), run->T, ix->n_rows,
                                   ix->fj_leafof.as<uint32_t>(), ix->jn_ctr.as<unsigned long long>() + 2, s));
    HIPCHK(hipStreamSynchronize(s));
    const char *env_c = getenv("ZH_FRANGE_CAND_CAP"), *env_l = getenv("ZH_WALK_LOG_CHUNKS"), *env_p = getenv("ZH_FRANGE_PATH");
    run->force2 = env_p && atoi(env_p) == 2;
    if (env_c && atoll(env_c) > 0) { run->env_cand = true; run->env_cand_cap = (uint64_t)atoll(env_c); }
    if (env_l && atoll(env_l) > 0) run->log_chunks = (size_t)atoll(env_l);
    return ZH_OK;
}

static ZhWalkLog frange_log(const zh_index *ix, const FrangeRun &run) {
    ZhWalkLog l;
    l.pool = ix->fr_logpool.as<uint2>();
    l.capacity = (uint32_t)std::min<size_t>(run.log_chunks, 0xFFFFFFFEu);
    l.head = ix->fr_loghead.as<uint32_t>();
    l.ctl = ix->fr_logctl.as<ZhLogCtl>();
    l.leaf_entries = 0;
    return l;
}

// The walk's first half for B queries, as ctx_begin runs it, with n = probe and every sign on demand: counts, scans, *tot on the host.
static int frange_walk(zh_index *ix, const FrangeRun &run, const float *dQ, uint32_t B, hipStream_t s, ZhTotals *tot) {
    const uint32_t d = ix->opt.dim;
    const uint64_t pairs = (uint64_t)B * run.T;
    const size_t nn = std::max<uint32_t>(ix->n_nodes, 1);
    if (pairs >= (1ull << 26)) return fail(ZH_ELIMIT, "batch * num_trees >= 2^26");
    int rc;
    if ((rc = ix->fr_counts.ensure(pairs * sizeof(ZhPairCounts))) || (rc = ix->fr_inline.ensure(pairs * ZH_INLINE_VISITS * sizeof(ZhVisit))) ||
        (rc = ix->fr_rowbase.ensure((pairs + 1) * 8)) || (rc = ix->fr_candbase.ensure((pairs + 1) * 8)) || (rc = ix->fr_visitbase.ensure((pairs + 1) * 8)) ||
        (rc = ix->fr_totals.ensure(sizeof(ZhTotals))) || (rc = ix->fr_leafcount.ensure(nn * 4)) || (rc = ix->fr_leaffill.ensure(nn * 4)) ||
        (rc = ix->fr_groupbase.ensure(nn * 4)) || (rc = ix->fr_grouprowbase.ensure(nn * 8)) || (rc = ix->fr_loghead.ensure(pairs * 4)) ||
        (rc = ix->fr_logctl.ensure(sizeof(ZhLogCtl))) || (rc = ix->fr_logpool.ensure(run.log_chunks * ZH_LOG_CHUNK * sizeof(uint2))))
        return rc;
    const ZhForestDev f = forest_dev(ix);
    HIPCHK(zh_launch_batch_init(ix->fr_leafcount.as<uint32_t>(), ix->fr_leaffill.as<uint32_t>(), (uint32_t)nn, ix->fr_logctl.as<ZhLogCtl>(),
                                ix->fr_totals.as<ZhTotals>(), s));
    HIPCHK(zh_launch_walk_count(f, dQ, B, d, (int32_t)run.probe, nullptr, 0, 0, ix->fr_counts.as<ZhPairCounts>(), ix->fr_inline.as<ZhVisit>(),
                                ix->fr_leafcount.as<uint32_t>(), frange_log(ix, run), s));
    HIPCHK(zh_launch_leaf_scan(f, ix->fr_leafcount.as<uint32_t>(), ix->fr_groupbase.as<uint32_t>(), ix->fr_grouprowbase.as<uint64_t>(),
                               ix->fr_totals.as<ZhTotals>(), s));
    HIPCHK(zh_launch_pair_scan(ix->fr_counts.as<ZhPairCounts>(), (uint32_t)pairs, ix->fr_rowbase.as<uint64_t>(), ix->fr_candbase.as<uint64_t>(),
                               ix->fr_visitbase.as<uint64_t>(), ix->fr_totals.as<ZhTotals>(), ix->fr_logctl.as<ZhLogCtl>(), s));
    HIPCHK(hipMemcpyAsync(tot, ix->fr_totals.p, sizeof(ZhTotals), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (tot->visits > 0xFFFFFFFull || tot->rows >= (1ull << 36))
        return fail(ZH_ELIMIT, "more than 2^28 leaf visits or 2^36 visited rows in one batch; use a smaller batch");
    return ZH_OK;
}

// ... and its second half, as ctx_finish runs it: the visits placed (or walked again when the log ran over) and the leaf groups joined; then the
// lookup of visited leaves.
static int frange_place(zh_index *ix, FrangeRun *run, const float *dQ, uint32_t B, const ZhTotals &tot, hipStream_t s) {
    const uint32_t d = ix->opt.dim;
    const uint64_t nv = std::max<uint64_t>(tot.visits, 1), ng = std::max<uint64_t>(tot.groups, 1);
    int rc;
    if ((rc = ix->fr_visits.ensure(nv * sizeof(ZhVisit))) || (rc = ix->fr_groups.ensure(ng * sizeof(ZhGroup))) || (rc = ix->fr_groupoff.ensure(ng * 8)) ||
        (rc = ix->fr_vk0.ensure(nv * 8)) || (rc = ix->fr_vk1.ensure(nv * 8)))
        return rc;
    const ZhForestDev f = forest_dev(ix);
    if (!(tot.flags & 1u))
        HIPCHK(zh_launch_expand(f, B, ix->fr_counts.as<ZhPairCounts>(), ix->fr_inline.as<ZhVisit>(), ix->fr_rowbase.as<uint64_t>(),
                                ix->fr_candbase.as<uint64_t>(), ix->fr_visitbase.as<uint64_t>(), ix->fr_visits.as<ZhVisit>(), ix->fr_leafcount.as<uint32_t>(),
                                ix->fr_leaffill.as<uint32_t>(), ix->fr_groupbase.as<uint32_t>(), ix->fr_grouprowbase.as<uint64_t>(),
                                ix->fr_groups.as<ZhGroup>(), ix->fr_groupoff.as<uint64_t>(), frange_log(ix, *run), s));
    else
        HIPCHK(zh_launch_walk_emit(f, dQ, B, d, (int32_t)run->probe, nullptr, 0, 0, ix->fr_counts.as<ZhPairCounts>(), ix->fr_inline.as<ZhVisit>(),
                                   ix->fr_rowbase.as<uint64_t>(), ix->fr_candbase.as<uint64_t>(), ix->fr_visitbase.as<uint64_t>(), ix->fr_visits.as<ZhVisit>(),
                                   ix->fr_leafcount.as<uint32_t>(), ix->fr_leaffill.as<uint32_t>(), ix->fr_groupbase.as<uint32_t>(),
                                   ix->fr_grouprowbase.as<uint64_t>(), ix->fr_groups.as<ZhGroup>(), ix->fr_groupoff.as<uint64_t>(), s));
    uint64_t *vk[2] = {ix->fr_vk0.as<uint64_t>(), ix->fr_vk1.as<uint64_t>()};
    size_t tmp_bytes = 0;
    HIPCHK(zh_launch_frange_visit_index(nullptr, tot.visits, nullptr, run->T, (uint64_t)B * run->T, vk, nullptr, &tmp_bytes, &run->vsorted, s));
    if ((rc = ix->fr_vtmp.ensure(tmp_bytes))) return rc;
    HIPCHK(zh_launch_frange_visit_index(ix->fr_visits.as<ZhVisit>(), tot.visits, ix->fk_ntree.as<uint32_t>(), run->T, (uint64_t)B * run->T, vk, ix->fr_vtmp.p,
                                        &tmp_bytes, &run->vsorted, s));
    return ZH_OK;
}

// path 1 of one internal batch: the f32 leaf sweep over the walk's groups keys every visited row; frange_collect_kernel reads the visits' slices
static int frange_batch1(zh_index *ix, FrangeRun *run, const float *dQ, uint32_t B, const uint64_t *dMaxK, const ZhTotals &tot, uint64_t pool_cap,
                         hipStream_t s) {
    const uint32_t d = ix->opt.dim;
    int rc;
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_keys.ensure(std::max<uint64_t>(tot.rows, 1) * 8))) return rc;
    HIPCHK(hipMemsetAsync(ix->rg_cnt.p, 0, (size_t)B * 4, s));
    HIPCHK(hipMemsetAsync(ix->rg_ctr.p, 0, 16, s));
    if (!tot.visits) return ZH_OK;
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_sweep(ix->X.as<float>(), d, dQ, ix->ex_QQ.as<float>(), ix->fr_groups.as<ZhGroup>(), ix->fr_groupoff.as<uint64_t>(), tot.groups, nullptr,
                           ix->leaf_ids.as<uint32_t>(), tot.group_rows, run->metric, score_param(run->metric, run->mode), ix->ex_keys.as<uint64_t>(), s));
    HIPCHK(zh_launch_frange_collect(ix->fr_visits.as<ZhVisit>(), tot.visits, ix->ex_keys.as<uint64_t>(), ix->leaf_ids.as<uint32_t>(), ix->n_rows,
                                    ix->fk_ntree.as<uint32_t>(), run->vsorted, ix->fr_visitbase.as<uint64_t>(), ix->fj_leafof.as<uint32_t>(), run->T, dMaxK,
                                    ix->rg_cnt.as<uint32_t>(), ix->rg_ctr.as<unsigned long long>(), ix->rg_pv0.as<uint64_t>(), ix->rg_pk0.as<uint64_t>(), pool_cap,
                                    s));
    run->inf.launches++;
    return ZH_OK;
}

// Path 2 of one internal batch: the queries' halves and bounds, the visited leaves listed from the per-leaf visit counts (node order) and scored
// in batches of at most ZH_FKNN_COL_TILES row tiles (or ONE longer leaf alone) into one candidate pool -- every batch's leaves and tile sources
// go to the device once, then per batch the gather and ONE launch, nothing waited for in between -- then the range search's survivor pass.
// *used = false: the visit gate keeps the batch on path 1 (fewer than ZH_FRANGE_MIN_VISITORS visits per visited leaf on average: the tile columns
// would be mostly padding and the gather would cost more bytes than the f32 sweep reads; ZH_FRANGE_PATH=2 skips the gate).  On return with *used
// the stream has been waited for and h_ctr = {hits, candidates}; candidates > cand_cap: the pool ran over and nothing was counted.
static int frange_batch2(zh_index *ix, FrangeRun *run, const float *dQ, uint32_t B, const uint64_t *dMaxK, const ZhTotals &tot, uint64_t pool_cap,
                         uint64_t cand_cap, hipStream_t s, bool *used, unsigned long long h_ctr[2]) {
    *used = false;
    const uint32_t d = ix->opt.dim, nn = ix->n_nodes;
    int rc;
    std::vector<uint32_t> h_cnt(nn), h_gb(nn);
    HIPCHK(hipMemcpyAsync(h_cnt.data(), ix->fr_leafcount.p, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_gb.data(), ix->fr_groupbase.p, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // the visited leaves (the walk counts visits of non-empty leaves only), cut into batches: batch k = leaves [cut[k].x, cut[k + 1].x), tiles
    // [cut[k].y, cut[k + 1].y); a leaf's col0 counts from its batch's first tile
    std::vector<ZhFrangeSeg> segs;
    std::vector<uint2> colsrc, cut(1, make_uint2(0, 0));
    uint64_t tiles = 0;
    uint32_t batch_tiles = 0, most_tiles = 0;
    for (uint32_t nd = 0; nd < nn; nd++) {
        if (!h_cnt[nd] || ix->h_plane[nd] >= 0 || ix->h_right[nd] <= 0) continue;
        const uint32_t off = (uint32_t)ix->h_left[nd], len = (uint32_t)ix->h_right[nd], rt = (len + 15) / 16;
        if (batch_tiles && batch_tiles + rt > ZH_FKNN_COL_TILES) {
            cut.push_back(make_uint2((uint32_t)segs.size(), (uint32_t)colsrc.size()));
            batch_tiles = 0;
        }
        segs.push_back(ZhFrangeSeg{batch_tiles, rt, h_gb[nd], h_cnt[nd], run->node_tree[nd], 0, 0, 0});
        for (uint32_t c = 0; c < rt; c++) colsrc.push_back(make_uint2(off + 16 * c, std::min<uint32_t>(16, len - 16 * c)));
        batch_tiles += rt;
        most_tiles = std::max(most_tiles, batch_tiles);
        tiles += (uint64_t)rt * ((h_cnt[nd] + 15) / 16);
    }
    cut.push_back(make_uint2((uint32_t)segs.size(), (uint32_t)colsrc.size()));
    if (segs.empty() || (!run->force2 && tot.visits < (uint64_t)ZH_FRANGE_MIN_VISITORS * segs.size())) return ZH_OK;
    // per batch the column tiles per block and every leaf's first block
    std::vector<uint2> geo(cut.size() - 1);  // {blocks, ch}
    for (size_t k = 0; k + 1 < cut.size(); k++) {
        uint32_t n_blocks = 0;
        const uint32_t ch = fill_chunk([&](uint32_t c) {
            n_blocks = 0;
            for (uint32_t l = cut[k].x; l < cut[k + 1].x; l++) {
                segs[l].first_block = n_blocks;
                n_blocks += (segs[l].rt + 3) / 4 * (((segs[l].visitors + 15) / 16 + c - 1) / c);
            }
            return n_blocks;
        });
        geo[k] = make_uint2(n_blocks, ch);
    }
    const size_t NT = colsrc.size();
    if ((rc = ix->ex_QQ.ensure((size_t)B * 4)) || (rc = ix->ex_Qh.ensure((size_t)B * d * 2)) || (rc = ix->ex_qmeta.ensure((size_t)B * 16)) ||
        (rc = ix->ex_tau.ensure((size_t)B * 4)) || (rc = ix->rg_cand.ensure(std::max<uint64_t>(cand_cap, 1) * 8)) ||
        (rc = ix->fr_segs.ensure(segs.size() * sizeof(ZhFrangeSeg))) || (rc = ix->fk_colsrc.ensure(NT * 8)) || (rc = ix->fk_crow.ensure((size_t)most_tiles * 64)) ||
        (rc = ix->fk_CA.ensure((size_t)most_tiles * 32 * d)) || (rc = ix->fk_cmeta.ensure((size_t)most_tiles * 128)))
        return rc;
    unsigned long long *ctr = ix->rg_ctr.as<unsigned long long>();
    uint32_t *crow = ix->fk_crow.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(ix->fr_segs.p, segs.data(), segs.size() * sizeof(ZhFrangeSeg), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ix->fk_colsrc.p, colsrc.data(), NT * 8, hipMemcpyHostToDevice, s));
    HIPCHK(zh_launch_qnorm(dQ, B, d, ix->ex_QQ.as<float>(), s));
    HIPCHK(zh_launch_qhalf(dQ, B, d, ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), 1, s));
    HIPCHK(zh_launch_range_tau(dMaxK, B, run->metric, run->mode, ix->ex_tau.as<uint32_t>(), s));
    HIPCHK(hipMemsetAsync(ix->rg_cnt.p, 0, (size_t)B * 4, s));
    HIPCHK(hipMemsetAsync(ctr, 0, 16, s));
    for (size_t k = 0; k + 1 < cut.size(); k++) {
        const uint32_t l0 = cut[k].x, nl = cut[k + 1].x - l0, c0 = cut[k].y, nt = cut[k + 1].y - c0;
        HIPCHK(zh_launch_fknn_cols(ix->fk_colsrc.as<uint2>() + c0, nt, ix->leaf_ids.as<uint32_t>(), ix->n_rows, crow, s));
        HIPCHK(zh_launch_fknn_gather(d, run->v.Xh, run->v.rowMeta, run->pos, crow, nt, run->v.rho, ix->fk_CA.p, ix->fk_cmeta.as<float2>(), nullptr, s));
        HIPCHK(zh_launch_frange_mfma(d, run->metric, run->mode, ix->fr_segs.as<ZhFrangeSeg>() + l0, nl, geo[k].x, geo[k].y, zh_group_size(d), ix->fk_CA.p,
                                     ix->fk_cmeta.as<float2>(), crow, ix->fr_groups.as<ZhGroup>(), ix->ex_Qh.p, ix->ex_qmeta.as<float4>(), run->Kc,
                                     run->v.rho, ix->ex_tau.as<uint32_t>(), run->vsorted, ix->fr_visitbase.as<uint64_t>(), ix->fj_leafof.as<uint32_t>(),
                                     run->T, ix->rg_cand.as<uint64_t>(), cand_cap, ctr + 1, s));
        run->inf.launches++;
    }
    run->inf.tiles += tiles;
    HIPCHK(zh_launch_range_survivors(ix->X.as<float>(), d, dQ, ix->ex_QQ.as<float>(), run->metric, run->mode, ix->rg_cand.as<uint64_t>(), ctr + 1, cand_cap, dMaxK,
                                     ix->rg_cnt.as<uint32_t>(), ctr, ix->rg_pv0.as<uint64_t>(), ix->rg_pk0.as<uint64_t>(), pool_cap, s));
    HIPCHK(hipMemcpyAsync(h_ctr, ctr, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (segs and colsrc are this frame's)
    *used = true;
    return ZH_OK;
}

// B <= ZH_EXACT_BATCH queries on device pointers, as range_one: the walk; a batch whose visits hold more rows than path 1 may key
// (ZH_FRANGE_KEY_ROWS) is cut in half -- up front where path 1 answers, and where path 2 ran over -- and each half walks for itself; otherwise path
// 2 where it serves (allow2), path 1 else and when path 2's candidates ran over; then the range search's offsets, order and output.
static int frange_one(zh_index *ix, FrangeRun *run, const float *dQ, uint32_t B, const uint64_t *dMaxK, uint64_t *dOff, uint64_t *dIds, uint64_t *dKeys,
                      bool host_out, bool allow2, hipStream_t s) {
    const uint32_t d = ix->opt.dim;
    ZhTotals tot{};
    int rc;
    if ((rc = frange_walk(ix, *run, dQ, B, s, &tot))) return rc;
    const bool p2 = allow2 && run->path2, too_long = tot.rows > ZH_FRANGE_KEY_ROWS && B > 1;
    auto halves = [&](bool a2) -> int {
        const uint32_t h = B / 2;
        int r = frange_one(ix, run, dQ, h, dMaxK, dOff, dIds, dKeys, host_out, a2, s);
        return r ? r : frange_one(ix, run, dQ + (size_t)h * d, B - h, dMaxK + h, dOff + h, dIds, dKeys, host_out, a2, s);
    };
    if (!p2 && too_long) return halves(allow2);
    if ((rc = frange_place(ix, run, dQ, B, tot, s))) return rc;
    RangeRun *rr = &run->rr;
    const uint64_t pool_cap = rr->over ? 0 : std::min<uint64_t>(rr->capacity - rr->total, tot.rows);
    if ((rc = ix->rg_cnt.ensure((size_t)B * 4)) || (rc = ix->rg_ctr.ensure(16)) || (rc = ix->rg_pv0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)) ||
        (rc = ix->rg_pk0.ensure(std::max<uint64_t>(pool_cap, 1) * 8)))
        return rc;
    unsigned long long h_ctr[2] = {0, 0};
    bool done = false;
    if (p2 && tot.visits) {
        uint64_t cand_cap = std::min<uint64_t>(tot.rows, std::max<uint64_t>(pool_cap + pool_cap / 4, (uint64_t)ZH_RANGE_CAND_FLOOR * B));
        if (run->env_cand) cand_cap = run->env_cand_cap;
        bool used = false;
        if ((rc = frange_batch2(ix, run, dQ, B, dMaxK, tot, pool_cap, cand_cap, s, &used, h_ctr))) return rc;
        if (used) {
            run->inf.path = 2;
            if (h_ctr[1] > cand_cap) run->inf.redone++;
            else { run->inf.candidates += h_ctr[1]; done = true; }
        }
        if (!done && too_long) return halves(false);
    }
    if (!done) {
        if ((rc = frange_batch1(ix, run, dQ, B, dMaxK, tot, pool_cap, s))) return rc;
        HIPCHK(hipMemcpyAsync(h_ctr, ix->rg_ctr.p, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    run->inf.visits += tot.visits;
    run->inf.leaf_rows += tot.rows;
    run->inf.hits += h_ctr[0];
    return range_emit(ix, B, h_ctr[0], pool_cap, rr, dOff, dIds, dKeys, host_out, s);
}

static int frange_args(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, uint32_t probe, int metric, int mode, uint64_t capacity,
                       const void *offsets, const void *ids, const void *keys, const void *total, const char *who) {
    int rc = range_args(ix, q, b, max_keys, metric, mode, capacity, offsets, ids, keys, total, who);
    if (rc) return rc;
    if (!probe) return fail(ZH_EINVAL, "%s: probe must be at least 1", who);
    if (probe > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "%s: probe %u > ZH_MAX_TOPK (%u)", who, probe, ZH_MAX_TOPK);
    return ZH_OK;
}

// what the call starts from: no query, or an index without live rows, answers nothing (*empty; no trees needed), otherwise the forest graph's state checks
static int frange_begin(zh_index *ix, size_t b, uint32_t probe, int metric, int mode, uint64_t capacity, FrangeRun *run, bool *empty, const char *who) {
    run->metric = metric; run->mode = mode; run->probe = probe;
    run->rr.capacity = capacity;
    run->inf.path = 1;
    run->inf.probe = probe;
    run->inf.trees = ix->n_trees;
    *empty = b == 0 || ix->live_dev.n_live == 0;
    return *empty ? ZH_OK : fknn_state(ix, who);
}

static int frange_finish(zh_index *ix, size_t b, const FrangeRun &run, const char *who) {
    {
        zh_range_forest_info inf = run.inf;
        inf.batch = b;
        inf.rows_live = ix->live_dev.n_live;
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->fr_info = inf;
    }
    if (run.rr.over)
        return fail(ZH_ELIMIT, "%s: %llu hits exceed the capacity of %llu; out_total and the offsets are exact, call again with that capacity", who,
                    (unsigned long long)run.rr.total, (unsigned long long)run.rr.capacity);
    return ZH_OK;
}

// Both entry points once the arguments have been judged, as range_call.  An empty call (no query -- the device call's alone -- or no live row) asks
// for no trees and takes no batch: the host call zeroes its b + 1 offsets and ends without scratch, the device call zeroes them on its stream.
static int frange_call(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, uint32_t probe, int metric, int mode, uint64_t capacity,
                       uint64_t *out_offsets, uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total, bool host, void *stream, const char *who) {
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc;
    if ((rc = set_device(ix)) || (rc = exact_live_rows(ix))) return rc;
    FrangeRun run;
    bool empty = false;
    if ((rc = frange_begin(ix, b, probe, metric, mode, capacity, &run, &empty, who))) return rc;
    if (empty && host) {
        memset(out_offsets, 0, (b + 1) * 8);
        return frange_finish(ix, b, run, who);
    }
    ScratchGuard guard{ix, SCRATCH_FRANGE};
    const hipStream_t s = call_stream(ix, stream);
    if (!host) HIPCHK(hipMemsetAsync(out_offsets, 0, (empty ? b + 1 : 1) * 8, s));
    if (!empty) {
        if ((rc = frange_setup(ix, s, &run))) return rc;
        rc = range_batches(ix, q, b, max_keys, out_offsets, host, s, [&](const float *dQ, uint32_t nb, const uint64_t *dMaxK, uint64_t *dOff) {
            return frange_one(ix, &run, dQ, nb, dMaxK, dOff, out_ids, out_keys, host, true, s);
        });
        if (rc) return rc;
    }
    if ((rc = put_total(run.rr.total, out_total, host, s))) return rc;
    return frange_finish(ix, b, run, who);
}

extern "C" int zh_search_range_forest_batch_device(zh_index *ix, const float *d_q, size_t b, const uint64_t *d_max_keys, uint32_t probe, int metric, int mode,
                                                   uint64_t capacity, uint64_t *d_out_offsets, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                                   uint64_t *d_out_total, void *stream) {
    const char *who = "zh_search_range_forest_batch_device";
    int rc = frange_args(ix, d_q, b, d_max_keys, probe, metric, mode, capacity, d_out_offsets, d_out_ids, d_out_keys, d_out_total, who);
    if (rc) return rc;
    return frange_call(ix, d_q, b, d_max_keys, probe, metric, mode, capacity, d_out_offsets, d_out_ids, d_out_keys, d_out_total, false, stream, who);
}

extern "C" int zh_search_range_forest_batch(zh_index *ix, const float *q, size_t b, const uint64_t *max_keys, uint32_t probe, int metric, int mode,
                                            uint64_t capacity, uint64_t *out_offsets, uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total) {
    const char *who = "zh_search_range_forest_batch";
    int rc = frange_args(ix, q, b, max_keys, probe, metric, mode, capacity, out_offsets, out_ids, out_keys, out_total, who);
    if (rc) return rc;
    out_offsets[0] = 0;
    *out_total = 0;
    if (b == 0) return ZH_OK;
    return frange_call(ix, q, b, max_keys, probe, metric, mode, capacity, out_offsets, out_ids, out_keys, out_total, true, nullptr, who);
}

extern "C" int zh_search_range_forest_info(const zh_index *ix, zh_range_forest_info *out) {
    return get_info(ix, &zh_index::fr_info, out, "zh_search_range_forest_info");
}

extern "C" int zh_hash_signs(zh_index *ix, const float *q, size_t b, uint32_t *out_bits, float *out_dots) {
    if (!ix || (b && (!q || !out_bits))) return fail(ZH_EINVAL, "zh_hash_signs: null argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = set_device(ix);
    if (rc) return rc;
    if (ix->rows_torn) return fail(ZH_ESTATE, "%s", k_torn_msg);
    const uint32_t P = ix->n_planes, d = ix->opt.dim;
    if (!b || !P) return ZH_OK;
    hipStream_t s = ix->stream;
    const uint32_t wpq = (P + 255) / 256 * 8, words = (P + 31) / 32;
    DevBuf dq, dbits, ddots;
    struct G { DevBuf *a, *b, *c; ~G() { a->release(); b->release(); c->release(); } } g{&dq, &dbits, &ddots};
    size_t chunk = std::max<size_t>(1, std::min<size_t>(b, (size_t)(256u << 20) / ((size_t)P * 4 + 1)));
    if (chunk >= 4) chunk &= ~(size_t)3;  // (the row-score path takes queries four at a time)
    if ((rc = dq.ensure(chunk * d * 4))) return rc;
    if ((rc = dbits.ensure(chunk * wpq * 4))) return rc;
    if (out_dots && (rc = ddots.ensure(chunk * P * 4))) return rc;
    std::vector<uint32_t> hb(chunk * wpq);
    for (size_t b0 = 0; b0 < b; b0 += chunk) {
        size_t nb = std::min(chunk, b - b0);
        HIPCHK(hipMemcpyAsync(dq.p, q + b0 * d, nb * d * 4, hipMemcpyHostToDevice, s));
        // zh_set_hash_mode(2): the signs (not the dots) through the row-score path where the forest allows -- the whole sign matrix of
        // both paths can then be compared bit for bit (tests/test_gpu_score_hash.py)
        if (!out_dots && ix->hash_mode == 2 && use_score_hash(ix, nb, P)) {
            zh_search_ctx *c = &ix->dctx;
            if (c->state == 2 && (rc = ctx_wait(c))) return rc;
            c->wpq = wpq;
            if ((rc = c->wTotals.ensure(sizeof(ZhTotals))) || (rc = c->wBits.ensure(nb * wpq * 4))) return rc;
            HIPCHK(hipMemsetAsync(c->wTotals.p, 0, sizeof(ZhTotals), s));
            if ((rc = launch_score_hash(c, dq.as<float>(), nb, false, s))) return rc;
            HIPCHK(hipMemcpyAsync(hb.data(), c->wBits.p, nb * wpq * 4, hipMemcpyDeviceToHost, s));
            ZhTotals ht;
            HIPCHK(hipMemcpyAsync(&ht, c->wTotals.p, sizeof ht, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            std::lock_guard<std::mutex> lks(ix->stats_mu);
            ix->stats.hash_from_scores = 1;
            ix->stats.hash_exact_fixups = ht.hash_fixups;
        } else {
            HIPCHK(zh_launch_hash_dense(dq.as<float>(), (uint32_t)nb, ix->planes.as<float>(), ix->consts.as<float>(), P, d,
                                        dbits.as<uint32_t>(), wpq, out_dots ? ddots.as<float>() : nullptr, s));
            HIPCHK(hipMemcpyAsync(hb.data(), dbits.p, nb * wpq * 4, hipMemcpyDeviceToHost, s));
        }
        if (out_dots) HIPCHK(hipMemcpyAsync(out_dots + b0 * P, ddots.p, nb * P * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t i = 0; i < nb; i++) {
            memcpy(out_bits + (b0 + i) * words, &hb[i * wpq], words * 4);
            if (P & 31) out_bits[(b0 + i) * words + words - 1] &= (1u << (P & 31)) - 1;
        }
    }
    return ZH_OK;
}

// ------------------------------------------------------------------------------------------------
// stand-alone metric calls (src/distance.rs), multi-GPU merge, synthetic queries
// ------------------------------------------------------------------------------------------------
static int pick_device(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(ZH_EHIP, "no usable HIP device; this library has no CPU fallback");
    if (device >= ndev) return fail(ZH_EINVAL, "device %d out of range", device);
    if (device >= 0) { e = hipSetDevice(device); if (e != hipSuccess) return fail(ZH_EHIP, "hipSetDevice: %s", hipGetErrorString(e)); }
    return ZH_OK;
}

// Stand-alone metric calls keep their device buffers per calling thread (and device): Metric::distance is called pair by
// pair from the crate's own code paths, and six hipMalloc / hipFree per call cost far more than the kernels.
struct DistScratch {
    int device = -1;
    DevBuf in, keys, small;  // [rows | query] staged together, the keys, the sweep's one-group record
    void drop() { in.release(); keys.release(); small.release(); device = -1; }
    ~DistScratch() { drop(); }
};
static thread_local DistScratch g_dist;

extern "C" int zh_distance_batch(int metric, int mode, const float *a, const float *q, size_t n, size_t dim,
                                 uint64_t *out_keys, int device) {
    if ((n && (!a || !out_keys)) || !q || !dim) return fail(ZH_EINVAL, "zh_distance_batch: null argument");
    if (n > 0xFFFFFFFFull) return fail(ZH_ELIMIT, "zh_distance_batch: n > 2^32-1");
    int rc = check_metric(metric, mode);
    if (rc) return rc;
    if ((rc = pick_device(device))) return rc;
    if (!n) return ZH_OK;
    int cur = 0;
    HIPCHK(hipGetDevice(&cur));
    DistScratch &sc = g_dist;
    if (sc.device != cur) { sc.drop(); sc.device = cur; }
    if ((rc = sc.in.ensure((n + 1) * dim * 4))) return rc;
    if ((rc = sc.keys.ensure(n * 8))) return rc;
    if ((rc = sc.small.ensure(ZH_DISTANCE_SCRATCH_BYTES))) return rc;
    float *da = sc.in.as<float>(), *dq = da + n * dim;
    HIPCHK(hipMemcpyAsync(da, a, n * dim * 4, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dq, q, dim * 4, hipMemcpyHostToDevice, nullptr));
    HIPCHK(zh_launch_distance_rows(da, n, (uint32_t)dim, dq, metric, mode, sc.keys.as<uint64_t>(), sc.small.p, nullptr));
    HIPCHK(hipMemcpy(out_keys, sc.keys.p, n * 8, hipMemcpyDeviceToHost));  // synchronises the null stream
    return ZH_OK;
}

extern "C" int zh_distance_pair(int metric, int mode, const float *a, const float *b, size_t dim, uint64_t *out_key, int device) {
    return zh_distance_batch(metric, mode, a, b, 1, dim, out_key, device);
}

extern "C" int zh_merge_topk_device(int device, uint32_t n_shards, size_t b, size_t k, const uint64_t *d_ids,
                                    const uint64_t *d_keys, const uint32_t *d_counts, uint64_t *d_out_ids,
                                    uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    if (b && (!d_ids || !d_keys || !d_counts || !d_out_ids || !d_out_keys || !d_out_counts)) return fail(ZH_EINVAL, "zh_merge_topk_device: null argument");
    if (k == 0 || k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k must be in 1..%u", ZH_MAX_TOPK);
    if (n_shards == 0 || n_shards > 1024) return fail(ZH_EINVAL, "n_shards must be in 1..1024");
    int rc = pick_device(device);
    if (rc) return rc;
    HIPCHK(zh_launch_merge(n_shards, (uint32_t)b, (uint32_t)k, d_ids, d_keys, d_counts, d_out_ids, d_out_keys, d_out_counts, 0, 0, (hipStream_t)stream));
    return ZH_OK;  // enqueued on `stream`; the caller synchronises
}

// one buffer per shard: [ids b*k u64][keys b*k u64][counts b u32, padded to 8 bytes] -- what ONE all-gather of
// every rank's packed result produces
extern "C" size_t zh_packed_result_words(size_t b, size_t k) { return 2 * b * k + (b + 1) / 2; }
extern "C" int zh_merge_topk_packed_device(int device, uint32_t n_shards, size_t b, size_t k, const uint64_t *d_packed,
                                           uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream) {
    if (b && (!d_packed || !d_out_ids || !d_out_keys || !d_out_counts)) return fail(ZH_EINVAL, "zh_merge_topk_packed_device: null argument");
    if (k == 0 || k > ZH_MAX_TOPK) return fail(ZH_ELIMIT, "top_k must be in 1..%u", ZH_MAX_TOPK);
    if (n_shards == 0 || n_shards > 1024) return fail(ZH_EINVAL, "n_shards must be in 1..1024");
    int rc = pick_device(device);
    if (rc) return rc;
    const uint64_t words = zh_packed_result_words(b, k);
    HIPCHK(zh_launch_merge(n_shards, (uint32_t)b, (uint32_t)k, d_packed, d_packed + b * k,
                           reinterpret_cast<const uint32_t *>(d_packed + 2 * b * k), d_out_ids, d_out_keys, d_out_counts,
                           words, 2 * words, (hipStream_t)stream));
    return ZH_OK;
}

extern "C" int zh_synth_queries_device(int device, float *d_out, uint64_t seed_rows, uint64_t seed_q, uint64_t n_rows,
                                       uint64_t b0, size_t b, uint32_t dim, int kind, void *stream) {
    if (b && !d_out) return fail(ZH_EINVAL, "null output");
    if (!n_rows) return fail(ZH_EINVAL, "n_rows must be > 0");
    int rc = pick_device(device);
    if (rc) return rc;
    HIPCHK(zh_launch_synth_queries(d_out, seed_rows, seed_q, n_rows, b0, b, dim, kind, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return ZH_OK;
}

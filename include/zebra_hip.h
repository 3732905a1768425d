/*
 * zebra_hip.h -- C ABI of the MI355X (gfx950) implementation of Zebra's LSH bucket-scan + distance
 * hot path.  This is the drop-in boundary: what the reference crate's FFI for this path binds
 * (INTEGRATION.md shows the Rust `extern "C"` block and the shim that keeps `space::Metric`,
 * `LSHIndex<N>` and `Database<N,Met,Mod>` signatures on top of it).
 *
 * Reference interfaces replaced (all paths relative to /root/reference):
 *   zh_index_create / zh_index_destroy   LSHIndex::new            src/database/index/lsh.rs:162-167
 *   zh_index_add                         LSHIndex::add            src/database/index/lsh.rs:440-466
 *                                        (first call = build_index, lsh.rs:411-429)
 *   zh_index_build                       build_a_tree x num_trees src/database/index/lsh.rs:250-267
 *   zh_search_batch[_device]             LSHIndex::search         src/database/index/lsh.rs:544-565
 *                                        driven per batch as Database::query_vectors does,
 *                                        src/database/core.rs:290-313
 *   zh_hash_signs                        Hyperplane::point_is_above  src/database/index/lsh.rs:39-43
 *   zh_distance_batch / zh_distance_pair Metric::distance for CosineDistance, L2SquaredDistance,
 *                                        L2Distance               src/distance.rs:19-49, 103-114
 *   zh_index_count / zh_index_num_trees  LSHIndex::no_vectors / no_trees / is_empty  lsh.rs:389-409
 *   zh_index_clear                       LSHIndex::clear          src/database/index/lsh.rs:506-529
 *   zh_index_remove / zh_index_deduplicate  LSHIndex::remove / deduplicate  src/database/index/lsh.rs:473-503, 270-288
 *   zh_index_compact                     (new) what the reference's store does by itself after lsh.rs:495: the device memory of removed
 *                                        rows is reclaimed in place, ids are renumbered under a returned old -> new map
 *   zh_shard_group_* / zh_shard_search_* (new) the loop of Database::query_vectors (src/database/core.rs:299-303) over an index
 *                                        whose rows are sharded across GPUs (README.md:31 "can be sharded"): local search on
 *                                        this rank's shard, ONE RCCL all-gather of the packed top-k, merge on every rank
 *   zh_merge_topk_device                 (new) the shard merge alone
 *   zh_search_exact_batch[_device]       (new) exact top-k over every live row under the same keys: recall ground truth
 *   zh_search_exact_filtered_batch[_device] (new) the exact top-k among the live rows a caller's bitmap allows
 *   zh_search_range_batch[_device]       (new) every live row whose key is at or below a per-query threshold key, as a CSR
 *   zh_self_join[_device]                (new) every pair of live rows whose key is at or below one threshold key, each pair once
 *   zh_cross_join[_device]               (new) every pair (live row of one index, live row of another) whose key is at or below one threshold key
 *   zh_knn_graph[_device]                (new) every live row's exact k nearest OTHER live rows, slab by slab
 *   zh_cross_knn[_device]                (new) every live row of one index's exact k nearest live rows of ANOTHER index, slab by slab
 *   zh_knn_graph_forest[_device]         (new) every row's k nearest rows among its leaf-mates in the forest: exact keys, approximate candidates
 *   zh_knn_graph_refine[_device]         (new) one NN-descent join round over a caller's graph: every row's neighbours and their neighbours, ranked
 *                                        by the exact key
 *   zh_knn_graph_reverse[_device]        (new) the capped reverse graph: for every row a deterministic sample of the rows that name it, and its
 *                                        in-degree
 *   zh_knn_graph_refine_rev[_device]     (new) zh_knn_graph_refine over each row's neighbours AND sampled reverse neighbours
 *   zh_knn_graph_descent[_device]        (new) the rounds of zh_knn_graph_refine_rev in one call on the device, keying from the second round on
 *                                        only what a new entry brings up: the loop's answer bit for bit
 *   zh_knn_graph_prune[_device]          (new) the occlusion rule of the graph indexes over a caller's graph: a line keeps a neighbour only if no
 *                                        neighbour kept before it is closer to it than the row itself
 *   zh_index_set_graph[_device] / zh_index_drop_graph / zh_index_graph_info  (new) a k-NN graph over the stored rows, kept on the device between calls
 *   zh_search_graph_batch[_device]       (new) beam search over that graph: a best-first walk from caller-given seeds, exact keys, an approximate
 *                                        visited set
 *   zh_search_graph_filtered_batch[_device] (new) the same walk, answered from the rows a caller's bitmap allows among those it keyed
 *   zh_search_graph_steered_batch[_device] (new) a walk that sees the bitmap: the beam holds allowed rows only, disallowed rows are hopped over
 *   zh_index_extend_graph[_device]       (new) lines for the rows stored since the attach, found by that walk, and the old lines they should be in
 *                                        re-ranked to name them: the attached graph follows add / append without a rebuild
 *   zh_index_get_graph[_device]          (new) the attached table read back as ids and counts
 *   zh_self_join_forest[_device]         (new) every pair of leaf-mates whose key is at or below one threshold key, each pair once: exact keys,
 *                                        approximate candidates
 *   zh_search_range_forest_batch[_device] (new) every member of the leaves the walk visits for a query whose key is at or below the query's
 *                                        threshold key, as a CSR: exact keys, approximate candidates
 *   zh_index_save / zh_index_load        (new) a snapshot of an index in ONE file of this library's own format (the reference persists through
 *                                        fjall, lsh.rs:62-120, whose files are not read here): rows, removals, forest and the planes' sample rows
 *
 * Conventions
 *   - Every function returns ZH_OK (0) or a negative zh_status; zh_last_error() gives the message
 *     of the calling thread's last failure.  Nothing throws or aborts across this boundary.
 *   - The caller owns every buffer it passes; the library owns all device memory behind zh_index.
 *   - ids are dense row numbers in insertion order (the Rust shim keeps row -> Uuid, lsh.rs:415);
 *     results carry id_base + row so that shards of one logical index return global ids.
 *   - keys are the reference's DistanceUnit (distance.rs:13): the IEEE-754 bit pattern of the f64
 *     distance, compared as an unsigned integer; ties order by id.
 *   - search/hash/distance calls on one index may come from several host threads (the reference
 *     calls search from rayon workers, core.rs:299-303); they serialise on an internal lock.
 *     add/build/set_forest/clear/destroy need external exclusion, like any &mut in the crate.
 *   - There is NO CPU fallback: every entry point that computes runs gfx950 kernels and fails with
 *     ZH_EHIP when no device is usable.
 */
#ifndef ZEBRA_HIP_H
#define ZEBRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define ZH_API __attribute__((visibility("default")))
#else
#define ZH_API
#endif

typedef struct zh_index zh_index;

typedef enum zh_status {
    ZH_OK = 0,
    ZH_EINVAL = -1,       /* bad argument */
    ZH_ENOMEM = -2,       /* host or device allocation failed */
    ZH_EHIP = -3,         /* HIP runtime / no usable gfx950 device */
    ZH_ESTATE = -4,       /* call not valid in the index's current state */
    ZH_ELIMIT = -5,       /* a documented limit was exceeded (e.g. top_k > ZH_MAX_TOPK) */
    ZH_EUNSUPPORTED = -6,
    ZH_EPEER = -7,        /* sharded search: ANOTHER rank of the group failed its part of the batch (or died); the exchange
                           * completed (or was aborted after a timeout), the batch's results are not valid on any rank */
    ZH_EIO = -8,          /* snapshots: the operating system refused an open, read, write, rename or fsync (the message carries strerror) */
    ZH_ECORRUPT = -9      /* snapshots: the file is not a snapshot, is truncated, or fails a size, range or checksum test */
} zh_status;

/* the 13 metric structs of src/distance.rs.  0-2 are the simsimd path (key = f64 bits); 3-11 the `distances`
 * crate path (key = f32 bits widened, distance.rs:59; Hamming an integer count, distance.rs:144-158) */
typedef enum zh_metric {
    ZH_COSINE = 0,      /* CosineDistance      distance.rs:15-32  */
    ZH_L2SQ = 1,        /* L2SquaredDistance   distance.rs:34-49  */
    ZH_L2 = 2,          /* L2Distance          distance.rs:99-114 */
    ZH_CHEBYSHEV = 3,   /* ChebyshevDistance   distance.rs:51-61  */
    ZH_CANBERRA = 4,    /* CanberraDistance    distance.rs:63-73  */
    ZH_BRAY_CURTIS = 5, /* BrayCurtisDistance  distance.rs:75-85  */
    ZH_MANHATTAN = 6,   /* ManhattanDistance   distance.rs:87-97  */
    ZH_L3 = 7,          /* L3Distance          distance.rs:116-126 */
    ZH_L4 = 8,          /* L4Distance          distance.rs:128-138 */
    ZH_HAMMING = 9,     /* HammingDistance     distance.rs:140-158 (low byte of each f32's bits) */
    ZH_MINKOWSKI = 10,  /* MinkowskiDistance { power }  distance.rs:160-174 */
    ZH_PNORM = 11       /* PNormDistance { power }      distance.rs:176-190 */
} zh_metric;
/* `power` is the struct's i32 field and every value is served, as in the reference: the DEFAULT-constructed metric
 * (`Met::default()`, core.rs:115,146; #[derive(Default)], distance.rs:160-165,176-181) has power 0 -- p-norm(0) = d,
 * Minkowski(0) = d^(1/0) = +inf (1 at d = 1) --, negative powers go through powi's reciprocal and pow's IEEE cases. */

/* distance.rs:23-25 applies `1.0 - c` to simsimd's cosine, which is already a distance, so the
 * reference key is the bit pattern of the cosine SIMILARITY.  PARITY reproduces that literally;
 * CORRECTED keys on the distance.  The `cosine_mode` argument of the calls below is this mode for ZH_COSINE,
 * the `power` field for ZH_MINKOWSKI / ZH_PNORM, and ignored by the other metrics. */
typedef enum zh_cosine_mode { ZH_COSINE_PARITY = 0, ZH_COSINE_CORRECTED = 1 } zh_cosine_mode;

#define ZH_MAX_TOPK 1024u
#define ZH_MAX_DEPTH 60u /* the reference recurses without bound on an unsplittable node */
#define ZH_MAX_DIM (1u << 20) /* zh_options.dim beyond this is refused with ZH_ELIMIT (row offsets stay far below 2^63) */

typedef struct zh_options {
    uint32_t dim;           /* N of Embedding<N>, lib.rs:18 */
    uint32_t max_node_size; /* LSHIndexOptions::max_node_size, default 5  (lsh.rs:126,134) */
    uint32_t num_trees;     /* LSHIndexOptions::num_trees,     default 15 (lsh.rs:128,135) */
    uint64_t seed;          /* hyperplane sampling seed (the reference uses an unseeded RNG, lsh.rs:201) */
    int32_t device;         /* HIP device ordinal; -1 = the calling thread's current device */
    uint64_t id_base;       /* global id of local row 0 (shard offset) */
    uint64_t reserve_rows;  /* capacity hint: avoids a reallocating copy on growth */
} zh_options;

/* Flat forest (host pointers).  Node i is inner when plane[i] >= 0: left[i] is the child holding
 * the rows BELOW the plane, right[i] the rows ABOVE (lsh.rs:260-264).  It is a leaf when
 * plane[i] == -1: (uint32_t)left[i] is an offset into leaf_ids and right[i] the leaf's length.
 * planes is n_planes x dim row-major, consts the matching offsets (Hyperplane, lsh.rs:16-25). */
typedef struct zh_forest_view {
    uint32_t n_nodes, n_planes, n_trees;
    uint64_t n_leaf_ids;
    const int32_t *plane, *left, *right;
    const uint32_t *roots;
    const float *planes, *consts;
    const uint32_t *leaf_ids;
} zh_forest_view;

typedef struct zh_forest_sizes {
    uint32_t n_nodes, n_planes, n_trees;
    uint64_t n_leaf_ids;
} zh_forest_sizes;

/* Counters and timings of the most recent search batch on this index (zh_stats). */
typedef struct zh_stats_t {
    uint64_t batch;            /* queries in the batch */
    uint64_t visits;           /* leaf visits (bucket probes) */
    uint64_t rows_scored;      /* R_total: stored rows whose distance was computed */
    uint64_t rows_unique;      /* R_unique: rows of the distinct leaves touched (0 unless stats level >= 2) */
    uint64_t rows_swept;       /* rows the sweep kernel actually loaded: queries that probe the same leaf share them */
    uint64_t candidates;       /* ids handed to the final top-k (before de-duplication) */
    uint64_t planes_dense;     /* hyperplanes hashed by the dense MFMA kernel, per query */
    uint64_t planes_total;     /* hyperplanes in the forest */
    uint64_t sweep_bytes;      /* bytes the sweep moves: (4*dim + 4) * rows_swept + 8 * rows_scored */
    /* accumulated since zh_stats_reset, in milliseconds, measured with hipEvents on the stream the
     * kernels run on (only when profiling is enabled with zh_set_profiling) */
    double ms_hash, ms_walk, ms_sweep, ms_select, ms_final, ms_total;
    uint64_t timed_batches;
    uint64_t sweep_rows_accum;  /* rows_scored summed over the timed batches */
    uint64_t swept_rows_accum;  /* rows_swept summed over the timed batches */
    uint64_t sweep_launches_accum; /* sweep_kernel launches over the timed batches (a batch is several launches) */
    uint64_t window_batches;    /* API batches handled together in the most recent internal batch (zh_search_begin_window) */
    uint64_t table_scan;        /* 1: the most recent batch was swept by the table scan (every stored row streamed once, scored
                                 * against every query that visits one of its leaves; rows_swept = stored rows), 0: leaf by leaf */
    uint64_t scan_batches_accum; /* timed internal batches swept by the table scan */
    uint64_t hash_from_scores;  /* 1: the most recent batch took every sign of the forest from row scores (zh_set_hash_mode) */
    uint64_t hash_exact_fixups; /* ... and this many of its signs lay inside the rounding bound and were recomputed exactly */
    uint64_t prefiltered;       /* 1: the most recent batch picked its candidates from the row scores (zh_set_sweep_mode): rows_scored
                                 * rows were judged on their scores, rows_swept of them scored with the reference's arithmetic */
    uint64_t prefilter_exact_visits; /* ... leaf visits whose `take` nearest rows the scores could not decide (scored exactly) */
    uint64_t prefilter_exact_rows;   /* ... rows scored exactly in total (= rows_swept) */
    uint64_t prefilter_fallbacks_accum; /* batches redone with the sweep because a candidate list ran over (since zh_stats_reset) */
    uint64_t prefilter_last_overflow;   /* ... what ran over in the most recent of them: 1 | 2 a (query, tree) list, 4 the table of
                                         * visits to score exactly, 8 a leaf longer than 64 rows, 16 a query's lists together hold more than the final sort */
    uint64_t approx_scan;           /* 1: the most recent batch's table scan read HALF-WIDTH (fp16) copies of the queries: every (row, query)
                                     * pair got an interval that contains the reference's key, the intervals picked the candidates, and only
                                     * the rows they could not rule out were scored with the reference's arithmetic (zh_set_sweep_mode);
                                     * 2: the same with the products on the matrix cores, from the index's fp16 copy of the stored rows;
                                     * 3: 128-d rows leaf by leaf from their fp16 copy (table_scan = 0) */
    uint64_t approx_exact_visits;   /* ... leaf visits that take fewer than top_k rows: scored and ranked exactly */
    uint64_t approx_survivors;      /* ... rows (over all queries) that got the reference's key for the final top_k */
    uint64_t approx_list_entries;   /* ... candidates handed to the per-query stage (before de-duplication) */
    uint64_t approx_columns;        /* ... approx_scan 2: a tile column of the matrix-core scan is a DISTINCT query of a wave's pairs; columns and pairs of */
    uint64_t approx_column_pairs;   /*     (a 1-in-64 sample of) the waves of the most recent such batch: what the pairs share (1.0 = nothing) */
    uint64_t approx_batches_accum;  /* timed internal batches scanned this way */
    uint64_t approx_fallbacks_accum; /* batches redone by the f32 scan ON THE DEVICE, in stream order, because a list ran over */
    uint64_t approx_last_overflow;  /* ... what ran over: 1 a query's candidate list, 2 a query's survivors, 4 the table of exact
                                     * visits, 8 their key scratch */
    uint64_t combined_batches_accum; /* zh_search_batch: internal batches that served MORE than one concurrent caller (since reset) */
    uint64_t combined_calls_accum;   /* ... and the calls they served */
    uint64_t host_window_calls_accum; /* zh_search_batch calls whose (large, host-resident) batch ran as windows over two contexts, copies beside
                                      * the kernels (since reset) */
    uint64_t scan_order_keys;        /* the matrix-core scan keeps ITS view of the rows (fp16 tiles, row -> leaf entries) in the order that lets a tile's 16 rows
                                      * share the most leaves: 0 id order, 2 / 3 sorted by the leaves in that many trees -- measured when the copy is made */
    uint64_t scan_order_share_permille; /* ... (adjacent rows, tree) combinations in the same leaf under the kept order, per thousand */
    uint64_t row_copy_bytes;         /* device memory the index holds for fp16 copies of its stored rows (the half-width sweeps: zh_set_sweep_mode);
                                     * 0 until a batch has used one, and with modes 1 / 2 / 5 */
    uint64_t approx_fused;           /* 1: approx_scan 3 and the most recent batch's sweep was FUSED -- intervals, bounds and the queries' candidate
                                     * lists inside the sweep kernel (no raw pairs written, no select pass; round 6) */
    uint64_t approx_byte_rows;       /* 1: approx_scan 3 and the sweep read an EXACT copy of 128 BYTES per stored row: every element of the table is an
                                     * integer in 0 .. 255 (SIFT descriptors), checked when the copy is made; any other row and the copy is of halves */
} zh_stats_t;

/* ---- lifecycle ------------------------------------------------------------------------------ */
ZH_API void zh_options_default(zh_options *opt); /* dim 0, max_node_size 5, num_trees 15 (lsh.rs:131-138) */
ZH_API int zh_index_create(const zh_options *opt, zh_index **out);
ZH_API void zh_index_destroy(zh_index *idx);
ZH_API int zh_index_clear(zh_index *idx); /* drops vectors AND trees (what lsh.rs:506-529 intends) */

/* ---- insert --------------------------------------------------------------------------------- */
/* LSHIndex::add: rows is n x dim row-major host memory.  If the index has no trees the forest is
 * built over everything stored so far plus these rows (build_index); otherwise the rows descend
 * the existing trees and split full leaves (insert, lsh.rs:350-382) -- as the sequential execution
 * "one row after another, each into every tree" of the reference's racy par_iter (lsh.rs:445-462).
 * out_row_ids (may be NULL) receives id_base + row for each new row. */
ZH_API int zh_index_add(zh_index *idx, const float *rows, size_t n, uint64_t *out_row_ids);
/* staged loading for large shards: append without building, then zh_index_build once */
ZH_API int zh_index_append(zh_index *idx, const float *rows, size_t n, uint64_t *out_row_ids);
/* The same with the rows already in device memory.  This call takes NO stream: the rows are copied on the index's own (non-blocking) stream and the
 * call waits for that copy, so d_rows must be COMPLETE before the call -- work still pending on a stream of the caller's that writes d_rows is
 * ordered against nothing here; wait for it (or for an event of it) first. */
ZH_API int zh_index_append_device(zh_index *idx, const float *d_rows, size_t n);
/* append n synthetic rows generated on the device (bit-identical to oracle zo_synth_rows);
 * kind 0 = ~N(0,1), kind 1 = integer-valued "SIFT-style" in [0,255], kind 2 = clustered (128 consecutive rows
 * share a centre: centre + 0.25 * noise) */
ZH_API int zh_index_append_synthetic(zh_index *idx, size_t n, uint64_t seed, uint64_t first_row, int kind);
ZH_API int zh_index_build(zh_index *idx); /* (re)build all trees on the GPU */
/* LSHIndex::remove (lsh.rs:473-503) as intended: the ids leave every tree (the reference only edits trees whose root
 * is a leaf) and zh_index_count drops; later splits no longer sample them (lsh.rs:495, 197-201).  out_found (may be
 * NULL): 1 per id that was present.  LSHIndex::deduplicate (lsh.rs:270-288): rows bit-identical to an earlier row are
 * removed; out_ids (may be NULL) receives up to cap removed ids, ascending. */
ZH_API int zh_index_remove(zh_index *idx, const uint64_t *ids, size_t n, uint8_t *out_found, size_t *out_n_removed);
ZH_API int zh_index_deduplicate(zh_index *idx, uint64_t *out_ids, size_t cap, size_t *out_n_removed);

/* Compaction (new; the reference's store deletes a removed embedding, lsh.rs:495, and compacts by itself): remove / deduplicate only take ids
 * out of the trees -- the vectors stay in device memory, and every kernel that streams the table by position still streams them.  This call
 * moves the live rows down over the removed ones, IN PLACE and in their order (stable), renumbers the forest's leaf ids, and makes the live
 * count the stored count.  Rows keep their relative order, so the old -> new map is strictly increasing on the live rows: a compacted index
 * answers every later call as the uncompacted one would, under that map -- ids, keys, counts, later splits and rebuilds (the hyperplane sampler
 * draws the i-th LIVE row, which is new row i).  Nothing compacts by itself.
 *   - Needs external exclusion like add / build / remove; pipelined contexts must be idle.  Contexts and shard groups made before the call
 *     stay usable.  ZH_ESTATE on an index whose last add failed half way.  With nothing removed: a no-op that returns the identity map and
 *     releases nothing.
 *   - The f32 table keeps its capacity (capacity_rows): later appends reuse the freed tail.  The derived copies of the rows (the fp16 tiles and
 *     their per-row scales, the 128-d half / byte copy, the scan's row order and row -> leaf tables) are released and re-made at the new size
 *     by the next batch that wants them.
 *   - Rows move in stream-ordered chunks: a chunk whose destination ends at or before its source begins is copied directly, any other one
 *     through a bounce buffer.  Device scratch (released before return): scratch_bytes <= ZH_COMPACT_BOUNCE_BYTES + 4.25 * rows_before + 4096
 *     -- the bounce buffer, 4 bytes per stored row for the ranks, a bit per row, block sums.  ZH_COMPACT_CHUNK_ROWS (environment, read per
 *     call; tests) sets the rows per chunk, at most what the bounce buffer holds.
 *   - A forest injected with zh_index_set_forest that lists a row twice in one tree may still list a removed row: ZH_EUNSUPPORTED (rebuild it).
 *   - A device failure after rows have begun to move leaves the table inconsistent: every call that reads or adds rows (add / append* /
 *     build / remove / deduplicate / read_rows / hash_signs / search / exact search / compact) then fails with ZH_ESTATE until zh_index_clear.
 *   - Speed of later searches: answers are the same, the path to them may not be.  A forest whose plane was made from a row that has been
 *     removed loses the row-score hash and the prefilter on top of it (zh_set_hash_mode / zh_set_sweep_mode) when it is compacted -- the
 *     sample row's score no longer exists -- and hashes with one dot product per plane until zh_index_build; zh_stats_t::hash_from_scores
 *     shows it.  The table scans and sweeps get shorter by the removed share.
 *   - info->ms is the device work only; the call also spends host time proportional to the stored rows (the live bitmap, the chunk plan,
 *     and, when out_new_ids is given, 4 bytes per row back from the device).
 * out_new_ids (may be NULL; else cap >= rows_before, ZH_EINVAL otherwise): for every OLD local row r, out_new_ids[r] = id_base + new row, or
 * UINT64_MAX if r had been removed.  info may be NULL. */
#define ZH_COMPACT_BOUNCE_BYTES (256u << 20)
typedef struct zh_compact_info {
    uint64_t rows_before;     /* stored rows (live + removed) before the call */
    uint64_t rows_after;      /* = live rows = zh_index_count, before and after */
    uint64_t rows_moved;      /* live rows whose position changed (0: nothing was removed, or only a tail) */
    uint64_t bytes_moved;     /* bytes the move read + wrote in device memory (bounce copies counted) */
    uint64_t scratch_bytes;   /* peak device scratch the call allocated (released before it returns) */
    uint64_t capacity_rows;   /* rows the f32 table has room for after the call (kept: later appends reuse it) */
    uint64_t copy_bytes_released; /* zh_stats_t::row_copy_bytes before the call: the fp16 / byte copies and the scan's order, let go and re-made at
                                   * the new size on next use (the smaller per-row tables -- norms, row -> leaf, live lists -- go too, uncounted) */
    double   ms;              /* hipEvent time of the device work, on the index's stream */
} zh_compact_info;
ZH_API int zh_index_compact(zh_index *idx, uint64_t *out_new_ids, size_t cap, zh_compact_info *info);

/* ---- snapshots (new): an index saved to ONE file and loaded back ------------------------------------------------------------------
 * A loaded index is indistinguishable from the saved one for every later call: ids, keys and counts of every search, zh_hash_signs,
 * zh_index_read_rows, zh_index_get_forest, the counts, which path a batch takes where that depends on index state (zh_stats_t::hash_from_scores,
 * prefiltered), and the effect of every later add / append / build / remove / deduplicate / compact.  Saved: the options, the f32 rows (removed
 * ones included: ids are row numbers), the removed-row set, the forest arrays in the index's own numbering, the planes' sample rows and whether
 * they are valid (zh_index_set_forest could not restore them: the row-score hash and the prefilter survive a snapshot), scan_unsafe, the levels
 * of the built forest.  NOT saved: everything derived from those (the fp16 / byte copies of the rows, norms, row -> leaf tables, the scan order, the
 * blocked view, exact-search scratch: re-made on first use, as after zh_index_compact) and the tuning state (sweep / hash mode, dense levels,
 * strikes, statistics, profiling: a loaded index starts with the defaults).
 * The file (byte for byte): little endian; a 4096-byte header block -- magic, version, the fields of zh_snapshot_info, a table of
 * {kind, offset, length, checksum} per section, the block's own checksum last --, then the sections, each on a 4096-byte boundary, padding zero.
 * A section's checksum is the sum mod 2^64 over its 8-byte words w_i (zero padded) of mix(w_i + 0x9E3779B97F4A7C15 (i + 1)), mix the splitmix64
 * finaliser: computable in any order and in pieces, on the GPU and on the host alike.
 * ZH_EIO: the operating system refused an open / read / write / rename / fsync; ZH_ECORRUPT: not a snapshot, truncated, or a size, range, padding
 * or checksum test failed; ZH_EUNSUPPORTED: a version newer than ZH_SNAPSHOT_VERSION. */
#define ZH_SNAPSHOT_VERSION 1u
typedef struct zh_snapshot_info {
    uint32_t version, dim, max_node_size, num_trees_option;
    uint64_t seed, id_base;
    uint64_t stored_rows, live_rows;          /* zh_index_stored_rows / zh_index_count */
    uint32_t n_trees, n_nodes, n_planes, flags; /* flags: 1 plane samples present (row-score hash survives), 2 scan_unsafe forest */
    uint64_t n_leaf_ids;
    uint64_t file_bytes, row_bytes;
    uint32_t n_sections, verified;            /* verified: 1 when every section checksum was recomputed and matched */
    double   ms, ms_device;                   /* wall time of the call; hipEvent time of its device work (0 for inspect) */
} zh_snapshot_info;
/* Writes the index to `path`: to path + ".zhtmp" in the same directory first, fsync, then rename over path -- a failed save leaves no file at
 * the temporary name and an older file at path intact.  The rows are never staged whole on the host: chunks of ZH_SNAPSHOT_CHUNK_BYTES
 * (environment, read per call, rounded down to a multiple of 8; default 64 MiB) go device -> host through two pinned buffers on a stream of the
 * call's own, the host writes chunk i while chunk i + 1 is in flight, and a gfx950 kernel sums each chunk on the device before it leaves: the
 * rows' checksum vouches for what was in device memory.  The file does not depend on the chunk size.  Holds the index lock exclusively
 * (searches wait) and needs the same external exclusion as zh_index_add; pipelined contexts must be idle.  ZH_ESTATE on an index whose last add
 * or compaction failed half way.  An empty index, one filled by zh_index_append and never built, and one with an injected forest all save.
 * info may be NULL. */
ZH_API int zh_index_save(zh_index *idx, const char *path, zh_snapshot_info *info);
/* Makes a new index from the file at `path` on `device` (-1: the calling thread's current device); reserve_rows is zh_options::reserve_rows.
 * Every size in the header is tested against the file's length and the ABI's limits (ZH_MAX_DIM, 2^32-1 rows and leaf entries) before anything
 * is allocated; the rows go up through the same two pinned buffers and the checksum kernel runs on what ARRIVED in device memory, so the
 * comparison with the table vouches for the bytes the GPU will read.  The forest passes the tests of zh_index_set_forest (and its planes keep
 * their numbering and their sample rows) before the index is handed out.  On any failure *out is NULL and everything allocated is released.
 * info may be NULL.  Loading one file twice gives two independent indexes. */
ZH_API int zh_index_load(const char *path, int32_t device, uint64_t reserve_rows, zh_index **out, zh_snapshot_info *info);
/* Host code only (no GPU needed): the header of the file at `path`, after every test zh_index_load applies to the header block, the section
 * table and the padding; verify != 0: every section's checksum is recomputed on the host as well (info->verified = 1). */
ZH_API int zh_snapshot_inspect(const char *path, int verify, zh_snapshot_info *info);

/* ---- forest exchange (parity tests inject / extract the exact same forest) ----------------- */
ZH_API int zh_index_set_forest(zh_index *idx, const zh_forest_view *forest);
ZH_API int zh_index_forest_sizes(zh_index *idx, zh_forest_sizes *out);
/* caller-allocated arrays of the sizes reported above */
ZH_API int zh_index_get_forest(zh_index *idx, int32_t *plane, int32_t *left, int32_t *right, uint32_t *roots,
                        float *planes, float *consts, uint32_t *leaf_ids);

/* ---- queries -------------------------------------------------------------------------------- */
ZH_API uint64_t zh_index_count(const zh_index *idx);     /* stored vectors (0 <=> no_vectors) */
ZH_API uint32_t zh_index_num_trees(const zh_index *idx); /* built trees    (0 <=> no_trees)   */
ZH_API uint64_t zh_index_stored_rows(const zh_index *idx); /* rows the table holds, live + removed (= zh_index_count after zh_index_compact):
                                                            * the next row's local number, and the length of zh_index_compact's map */
ZH_API uint32_t zh_index_dim(const zh_index *idx);
ZH_API int32_t zh_index_device(const zh_index *idx);     /* HIP device ordinal the index lives on */
ZH_API uint64_t zh_index_id_base(const zh_index *idx);
ZH_API const float *zh_index_rows_device(const zh_index *idx); /* device pointer to the stored rows (read-only) */
/* copy n stored rows starting at local row `first` back to host memory (KeyValue::embedding, lsh.rs:107-119) */
ZH_API int zh_index_read_rows(zh_index *idx, uint64_t first, size_t n, float *out);

/* point_is_above for every plane of the forest (numbered as zh_index_get_forest returns them) and
 * every query: out_bits is b x ceil(n_planes/32) words, bit p%32 of word p/32 = above.
 * out_dots (may be NULL) is b x n_planes raw f32 dot products.  q is b x dim host memory.  With zh_set_hash_mode(2) and
 * out_dots == NULL the signs are taken through the row-score path where the forest allows (b % 4 == 0): same bits. */
ZH_API int zh_hash_signs(zh_index *idx, const float *q, size_t b, uint32_t *out_bits, float *out_dots);

/* LSHIndex::search for a batch: q is b x dim; out_ids/out_keys are b x k (entries past
 * out_counts[i] are set to UINT64_MAX); ascending by (key, id).  Host pointers.
 * Callable from many threads at once -- the crate calls search with ONE query from every rayon worker (core.rs:299-303) -- and
 * built for that: callers that arrive while a batch is on the GPU queue up, the thread that finds the engine idle leads a round
 * and runs every queued request with the same top_k / metric / mode as ONE internal batch (answers are those of separate calls,
 * bit for bit: the queries of a batch never interact); the others sleep until theirs is done.  No timer: a lone caller is served
 * at once, a crowd is batched by the time the batch before it takes.  zh_stats_t::combined_* count it. */
ZH_API int zh_search_batch(zh_index *idx, const float *q, size_t b, size_t k, int metric, int cosine_mode,
                    uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with queries and results already resident in device memory; kernels are enqueued on
 * `stream` (a hipStream_t; NULL = the index's own stream) and have completed on return. */
ZH_API int zh_search_batch_device(zh_index *idx, const float *d_q, size_t b, size_t k, int metric, int cosine_mode,
                           uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);

/* EXACT top-k over every live stored row (rows removed by zh_index_remove / zh_index_deduplicate excluded); no forest needed: an index
 * filled by zh_index_append and never built is served.  Same arguments, limits, key arithmetic and output convention as zh_search_batch:
 * ids = id_base + row, ascending by (key, id), out_counts[i] = min(k, live rows), entries past it UINT64_MAX; k = 0 gives counts of 0.
 * Every key is the one zh_distance_batch returns for that (row, query) pair, for every metric, power and cosine mode, so the answer
 * is the ground truth of a recall measurement under the library's own keys.  Thread-safe against concurrent searches on the same
 * index (it serialises on the index's internal lock); never concurrent with add / build / remove / clear.  It does not join the
 * combining front end of zh_search_batch and leaves zh_stats_t alone: zh_search_exact_info describes the most recent call.
 * Two paths, same answers: path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, at least max(k, 8192) live rows, room for the
 * index's fp16 row copy: + 2 * dim + 8 bytes per stored row, kept and shared with the search) scans on the matrix cores for an interval per pair
 * and gives only the rows the intervals cannot rule out the canonical key; everything else, and an internal batch whose per-query lists run over,
 * takes path 1 (canonical sums for every pair).  Device scratch is allocated per call and released before it returns: at 1024 queries up to
 * ~1.1 GiB (path 1) or (16384 + 8 k) * 44 bytes per query (path 2). */
ZH_API int zh_search_exact_batch(zh_index *idx, const float *q, size_t b, size_t k, int metric, int cosine_mode,
                                 uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with queries and results in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_search_exact_batch_device(zh_index *idx, const float *d_q, size_t b, size_t k, int metric, int cosine_mode,
                                        uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_exact_info {  /* the most recent zh_search_exact_* call on this index */
    uint64_t batch;       /* queries */
    uint64_t rows_live;   /* rows ranked */
    uint32_t path;        /* 1: canonical sums for every pair; 2: matrix-core intervals, canonical keys for the survivors only */
    uint32_t redone;      /* path-2 internal batches whose lists ran over and were answered by path 1 instead */
    uint64_t survivors;   /* path 2: (row, query) pairs that got the canonical key, over all queries */
    uint64_t launches;    /* row-chunk launches of the scan */
} zh_exact_info;
ZH_API int zh_search_exact_info(const zh_index *idx, zh_exact_info *out);

/* Filtered exact search (new; the reference has no filter): zh_search_exact_batch over the rows a bitmap allows.  Bit r of the filter is bit
 * r & 31 of filter_words[r >> 5]; set: stored row r (id zh_index_id_base + r) may be returned.  n_bits is how many rows the bitmap speaks for:
 * rows at and past it are not allowed (a filter made before a later append stays valid), bits of the last word past it are ignored, and
 * n_bits > zh_index_stored_rows is ZH_EINVAL (a bitmap made for another table, for instance before zh_index_compact renumbered the rows).  A NULL
 * filter with n_bits > 0 is ZH_EINVAL.  The answer is exactly what zh_search_exact_batch gives on an index that holds only the rows that are both
 * allowed and live: the same ids, canonical keys and (key, id) order for every metric, power and cosine mode; out_counts[i] = min(k, allowed live
 * rows), entries past it UINT64_MAX; k = 0, an empty filter and an empty index give counts of 0; k > ZH_MAX_TOPK is ZH_ELIMIT; no forest needed.
 * One filter serves the whole batch.  Locking as for the exact search; zh_stats_t and zh_exact_info are left alone (zh_search_filtered_info
 * describes the most recent filtered call), and so are the index's cached live-row views.
 * The filter pass runs on the device (allowed AND live, counted, ranked into the ascending list of allowed live rows): nothing is uploaded
 * but the filter itself.  Path 1 scores that list, so its cost follows the allowed rows.  Path 2 (same dims and metrics as the exact search, at
 * least max(k, 8192) allowed live rows) scans the fp16 copy in chunks placed by the cumulative count of ALLOWED rows, and a 16-row tile with no
 * allowed row is skipped before it is loaded; it is taken when the tiles it would load cost less than gathering the allowed rows (the measured
 * rule: DESIGN.md s13).  Same answers either way. */
ZH_API int zh_search_exact_filtered_batch(zh_index *idx, const float *q, size_t b, size_t k, int metric, int cosine_mode,
                                          const uint32_t *filter_words, uint64_t n_bits, uint64_t *out_ids, uint64_t *out_keys,
                                          uint32_t *out_counts);
/* The same with queries, filter and results in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_search_exact_filtered_batch_device(zh_index *idx, const float *d_q, size_t b, size_t k, int metric, int cosine_mode,
                                                 const uint32_t *d_filter_words, uint64_t n_bits, uint64_t *d_out_ids,
                                                 uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_filtered_info {  /* the most recent zh_search_exact_filtered_* call on this index */
    uint64_t batch;         /* queries */
    uint64_t rows_live;     /* live rows of the index */
    uint64_t rows_allowed;  /* ... of them allowed by the filter: the rows ranked */
    uint32_t path;          /* 1: canonical sums for every (allowed row, query) pair; 2: matrix-core intervals over the table, masked */
    uint32_t redone;        /* path-2 internal batches whose lists ran over and were answered by path 1 instead */
    uint64_t survivors;     /* path 2: (row, query) pairs that got the canonical key, over all queries */
    uint64_t launches;      /* row-chunk launches of the scan */
    uint64_t tiles_skipped; /* path 2: 16-row tiles with no allowed row, returned from before they were loaded (over all internal batches) */
} zh_filtered_info;
ZH_API int zh_search_filtered_info(const zh_index *idx, zh_filtered_info *out);

/* Exact RANGE search (new; the reference has none): every live stored row within a radius of each query, however many there are.  The hits of query
 * i are the live rows (rows removed by zh_index_remove / zh_index_deduplicate excluded; no forest needed) whose key is <= max_keys[i], where the
 * key is the one zh_distance_batch returns for that (row, query) pair and keys compare as everywhere in this library: the u64 bit pattern,
 * unsigned.  A row is in exactly when zh_search_exact_batch would rank it at or before a row with key max_keys[i].  The threshold is a KEY, one per
 * query (zebra_amd.radius_key turns a distance into one); UINT64_MAX returns every live row.  For the parity cosine key (ZH_COSINE_PARITY: the bits
 * of the similarity 1 - distance, which may be negative) the unsigned order is the definition: non-negative similarities ascending, then the
 * negative ones by magnitude.
 * The result is a CSR: the hits of query i are out_ids / out_keys [out_offsets[i], out_offsets[i + 1]), ascending by (key, id), ids = id_base +
 * row; out_offsets[0] = 0 and *out_total = out_offsets[b].  out_offsets (b + 1 entries) and out_total must not be NULL.  If the hits exceed
 * `capacity` (the entries out_ids and out_keys have room for) the call returns ZH_ELIMIT: *out_total and ALL of out_offsets are still exact -- allocate
 * *out_total entries and call again -- and out_ids / out_keys are unspecified.  capacity = 0 with NULL out_ids / out_keys is the supported way to
 * count only.  b = 0, an empty index and an index of removed rows only give all-zero offsets and ZH_OK.  A NULL index, q or max_keys with b > 0,
 * NULL out_ids / out_keys with capacity > 0 and an unknown metric are refused before any device is touched.  All 13 metric / mode / power
 * combinations and every dimension are served.  Locking and thread-safety as for zh_search_exact_batch; zh_stats_t, zh_exact_info,
 * zh_filtered_info and the index's cached live-row views are left alone: zh_search_range_info describes the most recent call.
 * Internal batches of 1024 queries, two paths, same answers.  Path 1 keys every pair with the canonical sums, row chunk by row chunk, and collects
 * the keys at or below the threshold.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, at least 8192 live rows, the fp16 row
 * copy present) scans on the matrix cores for an interval per pair, takes the pairs whose interval reaches down to the threshold as candidates, and
 * gives only them the canonical key; a batch whose candidates outgrow their pool is answered by path 1 (`redone`).  ZH_RANGE_PATH=1 in the
 * environment (read per call) keeps every batch on path 1.
 * Device scratch is allocated per call and released before it returns.  Per internal batch, with P = min(capacity left, queries x live rows) hit
 * slots: 32 P bytes of hit pool and sort buffers + the sort's temporary storage (a few MiB), 8 bytes per candidate slot on path 2 (max(1.25 P,
 * 4096 per query) of them), up to 1 GiB of key scratch on path 1, and for the host call 16 bytes per hit of the batch as staging. */
ZH_API int zh_search_range_batch(zh_index *idx, const float *q, size_t b, const uint64_t *max_keys, int metric, int cosine_mode, uint64_t capacity,
                                 uint64_t *out_offsets, uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total);
/* The same with queries, thresholds and every output (out_total included) in device memory; enqueued on `stream` (NULL = the index's own stream),
 * complete on return. */
ZH_API int zh_search_range_batch_device(zh_index *idx, const float *d_q, size_t b, const uint64_t *d_max_keys, int metric, int cosine_mode,
                                        uint64_t capacity, uint64_t *d_out_offsets, uint64_t *d_out_ids, uint64_t *d_out_keys, uint64_t *d_out_total,
                                        void *stream);
typedef struct zh_range_info {  /* the most recent zh_search_range_* call on this index */
    uint64_t batch;       /* queries */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t hits;        /* (row, query) pairs within their query's threshold, over all queries (exact whatever the capacity) */
    uint32_t path;        /* 1: canonical sums for every pair; 2: matrix-core intervals, canonical keys for the candidates only */
    uint32_t redone;      /* path-2 internal batches whose candidate pool ran over and were answered by path 1 instead */
    uint64_t candidates;  /* path 2: (row, query) pairs that got the canonical key, over all internal batches path 2 completed */
    uint64_t launches;    /* launches of the scan (row chunks on path 1, one per internal batch on path 2) */
} zh_range_info;
ZH_API int zh_search_range_info(const zh_index *idx, zh_range_info *out);

/* Exact SELF-JOIN (new; the reference's deduplicate removes bit-identical rows only): every unordered pair of distinct live stored rows (a, b),
 * a < b by row number, whose key is <= max_key.  Rows removed by zh_index_remove / zh_index_deduplicate are excluded; no forest is needed.
 * The key of a pair is the key zh_distance_batch gives for stored row b against a query equal to the f32 values of row a: the pairs starting at a
 * are exactly the hits of zh_search_range_batch(rows[a], max_keys = {max_key}) with id > a.  That orientation is the definition; nothing relies on
 * the key being the same with the roles swapped (DESIGN.md s15 says, metric by metric, that the canonical sums do give the same bits).  ONE
 * threshold key for the whole call, a key as for the range search: zebra_amd.radius_key gives it, UINT64_MAX returns all L (L - 1) / 2 pairs of L
 * live rows, and the parity cosine key's unsigned order is the definition.
 * The result is three parallel arrays out_a, out_b, out_keys of *out_total entries, ids = id_base + row, ascending by (a, key, b).  If the pairs
 * exceed `capacity` (the entries each array has room for) the call returns ZH_ELIMIT with *out_total exact -- allocate that many and call again --
 * and the arrays unspecified.  capacity = 0 with NULL arrays is the supported way to count only.  An empty index, one live row and removed rows only
 * give *out_total = 0 and ZH_OK.  A NULL index or out_total, NULL arrays with capacity > 0 and an unknown metric are refused before any device is
 * touched.  All 13 metric / mode / power combinations and every dimension are served.  Locking and thread-safety as for zh_search_range_batch;
 * zh_stats_t, zh_exact_info, zh_filtered_info, zh_range_info and the index's cached live-row views are left alone: zh_self_join_info describes the
 * most recent call.
 * Two paths, same answers.  Path 1 gathers panels of up to 1024 live rows as queries, keys the row chunks from the panel's first row on with the
 * canonical sums and collects the keys at or below the threshold whose row is above the query row.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 /
 * 384 / 512 / 768 / 1024, at least 8192 live rows, the fp16 row copy present) multiplies tiles of the fp16 row copy by each other on the matrix
 * cores, the blocks on or above the diagonal only, for an interval per pair; the pairs whose interval reaches down to the threshold are candidates
 * and only they get the canonical key.  The copy is scanned in panels of 16384 rows; a panel whose candidates outgrow their pool is answered by
 * path 1 alone (`redone`); under a scan order that is not id order the first such panel sends the whole call to path 1.  ZH_JOIN_PATH=1 in the
 * environment (read per call) keeps every panel on path 1.
 * Device scratch is allocated per call and released before it returns.  With P = min(capacity, L (L - 1) / 2) hit slots: 32 P bytes of hit pool and
 * sort buffers + the sort's temporary storage; on path 2 20 bytes per stored row and 8 bytes per candidate slot of one panel (max(1.25 x the
 * capacity left, 256 per row of the panel) of them, never more than the panel's pairs); on path 1 the panel's rows and up to 1 GiB of key scratch;
 * for the host call 24 bytes per pair as staging. */
ZH_API int zh_self_join(zh_index *idx, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b,
                        uint64_t *out_keys, uint64_t *out_total);
/* The same with every output (out_total included) in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_self_join_device(zh_index *idx, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *d_out_a, uint64_t *d_out_b,
                               uint64_t *d_out_keys, uint64_t *d_out_total, void *stream);
typedef struct zh_join_info {  /* the most recent zh_self_join* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t pairs;       /* pairs within the threshold (exact whatever the capacity) */
    uint32_t path;        /* 1: canonical sums for every pair; 2: matrix-core intervals, canonical keys for the candidates only */
    uint32_t redone;      /* path-2 panels whose candidate pool ran over and were answered by path 1 instead */
    uint64_t candidates;  /* path 2: pairs that got the canonical key, over all panels path 2 completed */
    uint64_t launches;    /* launches of the scan (row chunks on path 1, one per panel on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (T (T + 1) / 2 for T tiles: nothing below the diagonal) */
} zh_join_info;
ZH_API int zh_self_join_info(const zh_index *idx, zh_join_info *out);

/* Exact JOIN BETWEEN TWO INDEXES (new; the reference has no such call): every pair (live stored row a of index `a`, live stored row b of index
 * `b`) whose key is <= max_key.  It replaces the loop "zh_index_read_rows of A back to the host, zh_search_range_batch on B 1024 rows at a time":
 * drop from an incoming batch what the corpus already holds, record linkage between two collections, the pairs between two snapshots.
 * The key of a pair is the key zh_distance_batch gives for STORED row b of B against a QUERY equal to the f32 values of row a of A: the pairs of
 * row a are exactly the hits of zh_search_range_batch(B, rows_A[a], max_keys = {max_key}).  That orientation is the definition; nothing relies on
 * the key being the same with the roles swapped, and zh_cross_join(b, a) is a different call with its own keys and order.  ONE threshold key for
 * the whole call, a key as for the range search and the self-join; UINT64_MAX returns all live(A) x live(B) pairs.
 * The result is three parallel arrays out_a, out_b, out_keys of *out_total entries, ascending by (a, key, b); out_a = A's id_base + row,
 * out_b = B's id_base + row (the two bases may differ).  If the pairs exceed `capacity` the call returns ZH_ELIMIT with *out_total exact --
 * allocate that many and call again -- and the arrays unspecified.  capacity = 0 with NULL arrays is the supported way to count only.  Either side
 * empty or without a live row gives *out_total = 0 and ZH_OK; no forest is needed on either side.
 * Refused with ZH_EINVAL before any device is touched: a NULL index on either side, a == b (use zh_self_join), a NULL out_total, NULL arrays with
 * capacity > 0, an unknown metric.  Refused with ZH_EINVAL after that: different dim, indexes on different devices.  All 13 metric / mode / power
 * combinations and every dimension are served.
 * Locking: the call holds BOTH indexes' internal locks exclusively, taken together without a lock order of the caller's (cross_join(A, B) on one
 * thread and cross_join(B, A) on another do not deadlock); never concurrent with add / build / remove / clear of either index.  All per-call
 * scratch and zh_cross_info live on the LEFT index `a`; B lends its rows, its fp16 row copy and its cached live-row views.  zh_stats_t, every
 * sibling info struct of both indexes and search contexts are left alone.
 * Two paths, same answers.  Path 1 gathers panels of up to 1024 live rows of A as queries, keys B's live rows against them with the canonical sums
 * and collects the keys at or below the threshold.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, the fp16 row copy
 * present on BOTH sides, live(A) x live(B) >= 2^25) multiplies tiles of A's fp16 copy by tiles of B's on the matrix cores for an interval per
 * pair; the pairs whose interval reaches down to the threshold are candidates and only they get the canonical key.  A is scanned in panels of
 * 16384 positions; a panel whose candidates outgrow their pool is answered by path 1 against all of B (`redone`) -- under any scan order of
 * either side, since a panel owns its pairs by A row.  ZH_XJOIN_PATH in the environment (read per call): 1 keeps every panel on path 1, 2 takes
 * path 2 at any size where it is supported.
 * Device scratch is allocated per call on A's device and released before it returns.  With P = min(capacity, live(A) x live(B)) hit slots: 32 P
 * bytes of hit pool and sort buffers + the sort's temporary storage; on path 2 20 bytes per stored row of either side and 8 bytes per candidate
 * slot of one panel (max(1.25 x the capacity left, 256 per row of the panel) of them, never more than the panel's rows x B's stored rows); on
 * path 1 the panel's rows and up to 1 GiB of key scratch; for the host call 24 bytes per pair as staging. */
ZH_API int zh_cross_join(zh_index *a, zh_index *b, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b,
                         uint64_t *out_keys, uint64_t *out_total);
/* The same with every output (out_total included) in device memory; enqueued on `stream` (NULL = A's own stream), complete on return. */
ZH_API int zh_cross_join_device(zh_index *a, zh_index *b, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *d_out_a,
                                uint64_t *d_out_b, uint64_t *d_out_keys, uint64_t *d_out_total, void *stream);
typedef struct zh_cross_info {  /* the most recent zh_cross_join* call with this index on the LEFT */
    uint64_t rows_live_a; /* live rows of the left index */
    uint64_t rows_live_b; /* live rows of the right index */
    uint64_t pairs;       /* pairs within the threshold (exact whatever the capacity) */
    uint32_t path;        /* 1: canonical sums for every pair; 2: matrix-core intervals, canonical keys for the candidates only */
    uint32_t redone;      /* path-2 panels of A whose candidate pool ran over and were answered by path 1 instead */
    uint64_t candidates;  /* path 2: pairs that got the canonical key, over all panels path 2 completed */
    uint64_t launches;    /* launches of the scan (row chunks of B on path 1, one per panel of A on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (T_A x T_B: the full rectangle) */
} zh_cross_info;
ZH_API int zh_cross_join_info(const zh_index *a, zh_cross_info *out);

/* Exact k-NN GRAPH (new; the reference has no such call): for every live stored row a of the slab [first_row, first_row + n) its exact top-k by
 * (key, id) over every live row EXCEPT a itself.  It replaces the loop "zh_index_read_rows back to the host, zh_search_exact_batch with k + 1,
 * 1024 rows at a time, find and drop self on the host": that loop converts every batch of rows to fp16 again although the index's fp16 copy holds
 * them, and "drop the first result" is wrong when a row has bit-identical duplicates with smaller ids, and wrong again under the parity cosine
 * key, where self has the LARGEST key.
 * The key of (a, b) is the key zh_distance_batch gives for stored row b against a query equal to the f32 values of row a (zh_self_join's
 * orientation); the line of a equals zh_search_exact_filtered_batch(rows[a], k, allowed = every row but a).  Only the row with the same row number
 * is excluded: bit-identical duplicates are ordinary neighbours, ties order by id.
 * Output line i belongs to STORED row first_row + i, 0 <= i < n: out_ids / out_keys are [n][k] u64, out_counts [n] u32; ids = id_base + row;
 * out_counts[i] = min(k, live rows - 1); entries past the count are UINT64_MAX in both arrays; a removed row's line has count 0 and is filled the
 * same way.  The interface is a slab on purpose (10M rows x k = 32 are 5 GB of output): call it slab after slab.  first_row + n > stored rows is
 * ZH_EINVAL; n = 0 is ZH_OK; k = 0 zeroes the counts and touches nothing else; k > ZH_MAX_TOPK - 1 is ZH_ELIMIT (one slot is kept so that path 1
 * may ask the exact search for k + 1).  A NULL index, NULL outputs for a non-empty request, an unknown metric and the k limit are refused before
 * any device is touched.  All 13 metric / mode / power combinations and every dimension are served.  Locking and thread-safety as for
 * zh_search_exact_batch_device; zh_stats_t, zh_exact_info, zh_filtered_info, zh_range_info, zh_join_info and the index's cached live-row views are
 * left alone: zh_knn_graph_info describes the most recent call.
 * The work goes panel by panel (up to 1024 live rows of the slab, ascending).  Two paths, same answers.  Path 1 gathers the panel as queries,
 * asks the exact search's path 1 for k + 1 and writes each line's first k entries that are not the line's own id.  Path 2 (ZH_L2SQ, ZH_L2,
 * ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, at least max(k + 1, 8192) live rows, the fp16 row copy present) gathers the panel's tiles out of
 * the fp16 copy and multiplies them by every tile of the copy on the matrix cores for an interval per pair, with a falling bound per line as in
 * the exact search; only the survivors get the canonical key.  A panel whose candidate list runs over is answered by path 1 (`redone`).
 * ZH_KNN_PATH=1 in the environment (read per call) keeps every panel on path 1; ZH_KNN_LIST_CAP=n (read per call; tests) lowers the list capacity.
 * Device scratch is allocated per call and released before it returns: on path 2 20 bytes per stored row (24 under a scan order that is not id
 * order) and per panel of P <= 1024 lines P (6 dim + 12) bytes of rows and 36 P (16384 + 8 k) bytes of lists; on path 1 the panel's rows and up
 * to 1 GiB of key scratch; both 16 P (k + 1) bytes of panel answer; for the host call 16 k + 4 bytes per line of a sub-slab of 65536 lines. */
ZH_API int zh_knn_graph(zh_index *idx, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys,
                        uint32_t *out_counts);
/* The same with every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return.  It replaces the same
 * loop run on the device: zh_search_exact_batch_device over the index's own rows with k + 1 and a kernel of the caller's that drops self. */
ZH_API int zh_knn_graph_device(zh_index *idx, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *d_out_ids,
                               uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_knn_info {  /* the most recent zh_knn_graph* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t lines;       /* live rows answered (the slab's live rows) */
    uint32_t k;
    uint32_t path;        /* 1: the exact search's path 1 with k + 1; 2: matrix-core intervals, canonical keys for the survivors only */
    uint32_t redone;      /* path 2: panels whose list ran over and that path 1 answered again */
    uint64_t survivors;   /* path 2: pairs that got the canonical key, over the panels path 2 completed */
    uint64_t launches;    /* launches of the scan (row chunks on path 1, column chunks on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (panel tiles x column tiles: the full rectangle) */
} zh_knn_info;
/* What the host loop that zh_knn_graph replaces could only count by hand. */
ZH_API int zh_knn_graph_info(const zh_index *idx, zh_knn_info *out);

/* Exact k-NN JOIN BETWEEN TWO INDEXES (new; the reference has no such call): for every live stored row a of the slab [first_row, first_row + n) of
 * index `a` its exact top-k by (key, id) over every live row of index `b`.  It replaces the loop "zh_index_read_rows of A back to the host,
 * zh_search_exact_batch on B 1024 rows at a time": link an incoming batch to its k nearest corpus rows, k-NN classification and label transfer,
 * ground truth for what a graph walk found, without a radius the caller does not know.
 * Lines.  Output line i belongs to STORED row first_row + i of A, 0 <= i < n: out_ids / out_keys are [n][k] u64, out_counts [n] u32.  A slab
 * interface for zh_knn_graph's reason.  first_row + n > A's stored rows is ZH_EINVAL; n = 0 is ZH_OK.
 * Neighbours.  The key of (a, b) is the key zh_distance_batch gives for STORED row b of B against a QUERY equal to the f32 values of row a of A:
 * the line of a is zh_search_exact_batch(B, rows_A[a], k) bit for bit -- ids (B's id_base + row), keys, (key, id) order.  That orientation is the
 * definition; zh_cross_knn(b, a) is a different call.  Nothing is excluded: a row of B that is bit-identical to row a is an ordinary neighbour.
 * Counts and tails.  out_counts[i] = min(k, live rows of B) for a live row of A, 0 for a removed one; entries past the count are UINT64_MAX in both
 * arrays.  An empty B, or one without a live row, gives count 0 everywhere with ZH_OK.
 * Limits.  k = 0 zeroes the counts and touches nothing else; k > ZH_MAX_TOPK is ZH_ELIMIT (no slot has to be spared here, unlike zh_knn_graph).
 * Refused before any device is touched and before either handle is followed: a NULL index on either side, a == b (ZH_EINVAL; use zh_knn_graph),
 * NULL outputs for a non-empty request, an unknown metric, the k limit.  Refused with ZH_EINVAL under the locks: different dim, indexes on
 * different devices.  All 13 metric / mode / power combinations and every dimension are served.
 * Locking: BOTH indexes' internal locks, exclusively, taken together as for zh_cross_join (cross_knn(A, B) on one thread and cross_knn(B, A) on
 * another do not deadlock); never concurrent with add / build / remove / clear of either index.  All per-call scratch and zh_xknn_info live
 * on the LEFT index `a`; B lends its f32 rows, its fp16 row copy and rowMeta, its live bitmap and its live list.  zh_stats_t, every sibling info
 * struct of BOTH indexes, the search contexts and the contents of the cached live-row views are left alone.
 * The work goes panel by panel (up to 1024 live rows of A's slab, ascending).  Two paths, same answers.  Path 1 gathers the panel out of A's f32
 * table as queries and lets the exact search's path 1 rank B's live list against it with k.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 /
 * 512 / 768 / 1024, the fp16 row copy present on BOTH sides, B with at least max(k, 8192) live rows) gathers the panel's tiles out of A's fp16 copy
 * and multiplies them by every tile of B's on the matrix cores for an interval per pair, with a falling bound per line as in the exact search;
 * only the survivors get the canonical key.  A panel whose candidate list runs over is answered by path 1 (`redone`).  ZH_XKNN_PATH in the
 * environment (read per call): 1 keeps every panel on path 1, 2 takes path 2 wherever it is supported and B has at least k live rows;
 * ZH_XKNN_LIST_CAP=n (read per call; tests) lowers the list capacity.
 * Device scratch is allocated per call on A's device and released before it returns: on path 2 20 bytes per stored row of B, 4 per stored row of A
 * under a scan order of A that is not id order, and per panel of P <= 1024 lines P (6 dim + 12) bytes of rows and 36 P (16384 + 8 k) bytes of
 * lists; on path 1 the panel's rows and up to 1 GiB of key scratch; both 16 P k bytes of panel answer; for the host call 16 k + 4 bytes per line
 * of a sub-slab of 65536 lines. */
ZH_API int zh_cross_knn(zh_index *a, zh_index *b, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *out_ids,
                        uint64_t *out_keys, uint32_t *out_counts);
/* The same with every output in device memory; enqueued on `stream` (NULL = A's own stream), complete on return. */
ZH_API int zh_cross_knn_device(zh_index *a, zh_index *b, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *d_out_ids,
                               uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_xknn_info {  /* the most recent zh_cross_knn* call with this index on the LEFT */
    uint64_t rows_live_a; /* live rows of the left index */
    uint64_t rows_live_b; /* live rows of the right index */
    uint64_t lines;       /* live rows of A answered (the slab's live rows) */
    uint32_t k;
    uint32_t path;        /* 1: the exact search's path 1 over B's live list; 2: matrix-core intervals, canonical keys for the survivors only */
    uint32_t redone;      /* path 2: panels whose list ran over and that path 1 answered again */
    uint64_t survivors;   /* path 2: pairs that got the canonical key, over the panels path 2 completed */
    uint64_t launches;    /* launches of the scan (row chunks of B on path 1, column chunks of B on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (panel tiles of A x column tiles of B) */
} zh_xknn_info;
ZH_API int zh_cross_knn_info(const zh_index *a, zh_xknn_info *out);

/* ---- forest k-NN graph (new): each stored row's k nearest rows AMONG ITS LEAF-MATES -------------------------------------------------------
 * zh_knn_graph multiplies every row by every row; this call multiplies a row only by the rows the random-projection forest puts beside it.
 * Arguments, output layout, slab meaning, ids, keys, tails and refusals are zh_knn_graph's.  The candidates of stored row a are
 *   C(a) = the union, over all trees, of the members of the leaf that holds a in that tree, minus a itself,
 * with membership as zh_index_get_forest's leaf_ids has it at the time of the call: removed rows have left every tree, rows appended since the
 * last build are in none.  Only the row with the same row number is excluded; a pair that shares leaves in several trees counts once.  Line i is
 * the first k of C(first_row + i) by (key, id), out_counts[i] = min(k, |C(a)|); a removed row and a live row that no tree holds have count 0.
 * Every id, key and count is bit for bit what that definition gives with zh_distance_batch's keys, for all 13 metric / mode / power combinations,
 * whatever the path, the slabs, the scan's row order or the run: what is approximate is the candidate set, never the arithmetic.  On a forest of
 * ONE tree whose root is a leaf the answer is zh_knn_graph's.  Compared line by line with zh_knn_graph it is the recall of a forest setting on
 * the index's own rows.
 * An index without trees is ZH_ESTATE for a request with n > 0 and k > 0; the other refusals, n = 0 and k = 0 as for zh_knn_graph, judged in the
 * same order.  Locking as zh_knn_graph_device; zh_stats_t, the five sibling info structs (zh_knn_info included) and the cached live-row views
 * are left alone: zh_knn_graph_forest_info describes the most recent call.
 * Path 1 (every metric, dimension and leaf shape): a line's visits are its own leaf in each tree; the leaf-major f32 sweep keys them, each
 * visit's first k + 1 are merged by (key, id) with duplicates dropped by id, and self is taken out.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim
 * 256 / 384 / 512 / 768 / 1024, the fp16 row copy present, zh_options.max_node_size >= 64): tree by tree, batches of leaves are gathered out of the
 * copy and ONE launch multiplies many leaves by themselves on the matrix cores for an interval per pair; a line's bound comes from its running
 * answer after the earlier trees and from the current tree's list alone (DESIGN.md s17 has the argument); survivors get the canonical key and are
 * merged into the running answer with duplicates dropped by id.  A batch whose list runs over has its sub-slabs of 65536 lines answered again by
 * path 1 (`redone`).  ZH_FKNN_PATH=1 in the environment (read per call) forces path 1; ZH_FKNN_LIST_CAP=n (read per call; tests) lowers the list
 * capacity.  Path 2 serves a slab at the cost of every leaf that holds one of its rows: few large slabs are cheaper than many small ones.
 * Device scratch is per call, released before return, and bounded whatever the table's size except where stated: 4 bytes per tree node (the
 * node -> tree map); per sub-slab of 65536 lines 8 trees + 12 bytes per line; path 1 per panel of P <= 1024 lines 4 P dim bytes of rows, 104 bytes
 * per (line, tree), 8 bytes per key of at most max(2^25, trees x longest leaf) keys and 16 P (k + 1) of answer; path 2 per batch of at most 4096
 * held lines and max(2048 tiles, the longest leaf) of columns 2 dim + 28 bytes per column row, 6 dim + 24 per held line and 36 bytes per list
 * slot of (longest leaf of the batch + k, at most 16384 + 8 k; after the first tree at most 1024 + 4 k) slots per line, plus 4 bytes per stored
 * row under a scan order that is not id order; for the host call 16 k + 4 bytes per line of a sub-slab of at most max(65536, 2^25 / k) lines. */
ZH_API int zh_knn_graph_forest(zh_index *idx, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *out_ids,
                               uint64_t *out_keys, uint32_t *out_counts);
/* The same with every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_knn_graph_forest_device(zh_index *idx, uint64_t first_row, uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *d_out_ids,
                                      uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_knn_forest_info {  /* the most recent zh_knn_graph_forest* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t lines;       /* the slab's rows that some tree holds */
    uint32_t k;
    uint32_t path;        /* 1: the f32 leaf sweep over each line's own leaves; 2: matrix-core intervals leaf by leaf, canonical keys for survivors */
    uint32_t trees;
    uint64_t pairs;       /* sum over the trees and over the slab's lines of (length of the line's leaf - 1): from the forest, not from the answer */
    uint64_t survivors;   /* path 2: pairs that got the canonical key, over the batches path 2 completed */
    uint32_t redone;      /* path 2: sub-slabs that path 1 answered again because a list ran over */
    uint64_t launches;    /* path 1: panels swept; path 2: batches (one matrix-core launch each) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (held tiles in use x the leaf's column tiles); 0 on path 1 */
} zh_knn_forest_info;
ZH_API int zh_knn_graph_forest_info(const zh_index *idx, zh_knn_forest_info *out);

/* ---- k-NN graph refinement (new): rank each row's neighbours' neighbours -------------------------------------------------------------------
 * One join round of NN-descent over a graph the caller already has: the forest graph's recall is limited by what the leaves hold, and the
 * neighbours of a row's neighbours are where the missing rows usually are.  The INPUT is a graph over ALL stored rows of the index: in_ids
 * [stored rows][in_k] in the id space of the outputs (id_base + row), in_counts [stored rows] -- what zh_knn_graph or zh_knn_graph_forest
 * returns for the whole table with k = in_k.  Keys are not taken: every returned key is computed here.
 *   N'(x) = the SET of rows named by the first min(in_counts[x], in_k) entries of line x that are live stored rows of this index.  An entry
 *           outside [id_base, id_base + stored rows) (UINT64_MAX included) is ignored, not an error; an entry that names a removed row is
 *           ignored: no candidate, not expanded; duplicates inside a line count once; order inside a line means nothing.  A graph made before
 *           a later zh_index_remove therefore stays valid; after zh_index_compact, re-keying it with the id map is the caller's job.
 *   C(a)  = ( N'(a)  union  N'(u) for every u in N'(a) ) minus a.  Only the row with the same row number is excluded; bit-identical
 *           duplicates are ordinary neighbours, as for zh_knn_graph.
 * The outputs have zh_knn_graph's layout and slab meaning: line i belongs to stored row a = first_row + i and holds the first k of C(a) by
 * (key, id), the key being zh_distance_batch's for stored row b against a query equal to the f32 values of row a; out_counts[i] =
 * min(k, |C(a)|), tails UINT64_MAX in both arrays, a removed a has count 0.  Ids, keys and counts are bit for bit what this definition gives,
 * for all 13 metric / mode / power combinations and every dimension, whatever the order or repetition of the input entries, the slabs or the
 * run.  No forest is needed: an index filled by zh_index_append and never built is served.
 * What follows from the definition:
 *   - N'(a) is a subset of C(a), so position by position the answer's (key, id) is never above that of the input line re-keyed;
 *   - refining the exact graph with k <= in_k returns the exact graph's first k;
 *   - on a table of at most in_k + 1 live rows with complete lists the answer is zh_knn_graph's.
 * Limits: k <= ZH_MAX_TOPK - 1 and in_k <= ZH_REFINE_MAX_IN_K (a line then gathers at most 64 + 64^2 = 4160 entries), else ZH_ELIMIT; in_k = 0
 * with n > 0 is ZH_EINVAL.  Judged before any device is touched, in this order of kinds: a null index (even for n = 0), null input or output
 * pointers of a request with n > 0, an unknown metric, the two limits, in_k = 0.  Then: first_row + n > stored rows is ZH_EINVAL, n = 0 is
 * ZH_OK, k = 0 zeroes the counts and touches nothing else.  Locking as zh_knn_graph_device; zh_stats_t, every sibling info struct and the
 * cached live-row views are left alone: zh_knn_graph_refine_info describes the most recent call.
 * The input is turned once per call into a table of u32 row numbers with everything invalid, removed or repeated masked (the host entry
 * streams in_ids through two pinned buffers of at most 64 MiB, ZH_REFINE_CHUNK_BYTES in the environment lowers that for tests), then a block
 * per live line gathers, sorts and de-duplicates its candidates in LDS, keys them with the canonical sums and sorts them by (key, id).
 * Device scratch is per call and released before return: 4 in_k + 4 bytes per stored row (the table and the counts), one chunk of the u64
 * input for the host entry, per sub-slab of 65536 lines 4 dim + 4 bytes per live line, and for the host call 16 k + 4 bytes per line of a
 * staged slab of at most max(65536, 2^25 / k) lines.  DESIGN.md s21. */
#define ZH_REFINE_MAX_IN_K 64u
ZH_API int zh_knn_graph_refine(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, uint64_t first_row, uint64_t n, size_t k,
                               int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with the graph and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_knn_graph_refine_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, uint64_t first_row, uint64_t n,
                                      size_t k, int metric, int cosine_mode, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                      void *stream);
typedef struct zh_knn_refine_info {  /* the most recent zh_knn_graph_refine* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t lines;       /* live rows of the slab */
    uint32_t in_k;
    uint32_t k;
    uint64_t listed;      /* entries gathered before de-duplication: the sum over the lines a of |N'(a)| + the sum over u in N'(a) of |N'(u)| */
    uint64_t keyed;       /* the sum of |C(a)|: the pairs that got a key */
    uint64_t updates;     /* output entries whose row is not in the line's own N'(a): NN-descent's convergence signal, 0 at a fixed point */
    uint64_t launches;    /* launches of the line kernel: one per sub-slab of 65536 stored rows that holds a live row */
} zh_knn_refine_info;
ZH_API int zh_knn_graph_refine_info(const zh_index *idx, zh_knn_refine_info *out);

/* ---- reverse neighbours (new): the capped transposed graph, alone and inside the refinement -------------------------------------------------
 * zh_knn_graph_refine ranks what a row's line names and what those lines name, never the rows that name IT: half of an NN-descent join.  With
 * N'(x) as defined above (the same rules for out-of-range, removed and repeated entries):
 *   In(x)   = { u live, u != x : x in N'(u) }, deg(x) = |In(x)| -- 0 for a removed x, which N' never names.
 *   h(u, x) = fmix32((u + 0x9E3779B9 * (x + 1)) mod 2^32) on the 32-bit row numbers, fmix32 murmur3's finaliser (h ^= h >> 16; h *= 0x85EBCA6B;
 *             h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16).  h(0,0) = 0x92CA2F0E, h(12345,678) = 0x44199268.
 *   R'(x)   = the first min(rev_k, |In(x) - N'(x)|) members of In(x) - N'(x), ascending by (h(u, x), u): mutual neighbours are left out (the line
 *             holds them), and the pick is a deterministic pseudo-random sample -- no seed, no dependence on the order of entries, the run or
 *             the slab.
 *   B(x)    = N'(x) union R'(x);   C_r(a) = ( B(a)  union  B(u) for every u in B(a) ) minus a.
 * zh_knn_graph_reverse: the input is the graph over ALL stored rows as for zh_knn_graph_refine; the slab selects output lines only.  Line i
 * belongs to x = first_row + i: out_ids [n][rev_k] holds R'(x) as id_base + row in (h, u) order with tails UINT64_MAX, out_counts[i] = |R'(x)|,
 * out_degree[i] = deg(x), the uncapped in-degree (the hubness score).  No metric and no keys are involved.  Limits: in_k and rev_k at most
 * ZH_REFINE_MAX_IN_K, else ZH_ELIMIT; 0 for either with n > 0 is ZH_EINVAL.  Judged before any device is touched, in this order of kinds: a
 * null index (even for n = 0), null pointers of a request with n > 0, the two limits (in_k, rev_k), in_k = 0, rev_k = 0.  Then first_row + n >
 * stored rows is ZH_EINVAL and n = 0 is ZH_OK.  Locking, stream semantics and "no forest needed" as zh_knn_graph_refine.
 * zh_knn_graph_refine_rev: zh_knn_graph_refine's arguments with rev_k behind in_k, and its answer, layout, keys, slabs and counts with C_r(a)
 * in place of C(a).  in_k + rev_k <= ZH_REFINE_MAX_IN_K, else ZH_ELIMIT (judged right after in_k's own limit); rev_k = 0 is allowed and is
 * zh_knn_graph_refine bit for bit (edges, kept and max_degree are then 0: nothing is transposed).  `updates` counts the answer's entries that
 * are not in N'(a) -- the FORWARD line -- so it stays the convergence signal, 0 at a fixed point.  C(a) is a subset of C_r(a): position by
 * position the answer's (key, id) is never above zh_knn_graph_refine's; refining the exact graph with k <= in_k still returns its first k.
 * The transposition runs on the refinement's table of row numbers: a pass of vector atomics counts the in-degrees, a scan makes 64-bit offsets,
 * a scatter fills the in-neighbours (their order inside a row's segment is not deterministic, the selection does not depend on it), a wave per
 * line -- a block for a line of more than 1024 in-neighbours -- keeps the rev_k smallest (h, u).  Device scratch is per call and released
 * before return: beside zh_knn_graph_refine's, per stored row 4 in_k (the in-neighbours) + 16 (in-degree, cursor, offset) + in_k / 256 + 1
 * bytes, for the fused call 4 (in_k + rev_k) more (the union table), and for zh_knn_graph_reverse's host call 8 rev_k + 8 bytes per line of a
 * staged piece of at most max(65536, 2^25 / rev_k) lines.  DESIGN.md s22. */
ZH_API int zh_knn_graph_reverse(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                                uint64_t *out_ids, uint32_t *out_counts, uint32_t *out_degree);
ZH_API int zh_knn_graph_reverse_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                       uint64_t n, uint64_t *d_out_ids, uint32_t *d_out_counts, uint32_t *d_out_degree, void *stream);
typedef struct zh_knn_reverse_info {  /* the most recent zh_knn_graph_reverse* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t lines;       /* live rows of the slab */
    uint32_t in_k;
    uint32_t rev_k;
    uint64_t edges;       /* the sum of deg(x) over ALL stored rows */
    uint64_t kept;        /* the sum of |R'(x)| over the slab */
    uint64_t max_degree;  /* the largest deg(x) over ALL stored rows */
    uint64_t launches;    /* launches of the two selection kernels: per staged piece one per 2^24 lines and one for the heavy lines */
} zh_knn_reverse_info;
ZH_API int zh_knn_graph_reverse_info(const zh_index *idx, zh_knn_reverse_info *out);

ZH_API int zh_knn_graph_refine_rev(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                                   size_t k, int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
ZH_API int zh_knn_graph_refine_rev_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                          uint64_t n, size_t k, int metric, int cosine_mode, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                          uint32_t *d_out_counts, void *stream);
typedef struct zh_knn_refine_rev_info {  /* the most recent zh_knn_graph_refine_rev* call on this index; the first eight fields are zh_knn_refine_info's */
    uint64_t rows_live;
    uint64_t lines;
    uint32_t in_k;
    uint32_t k;
    uint64_t listed;      /* the sum over the lines a of |B(a)| + the sum over u in B(a) of |B(u)| */
    uint64_t keyed;       /* the sum of |C_r(a)| */
    uint64_t updates;     /* output entries whose row is not in the FORWARD line N'(a) */
    uint64_t launches;    /* launches of the line kernel */
    uint64_t rev_k;
    uint64_t edges;       /* the sum of deg(x) over ALL stored rows; 0 when rev_k = 0 */
    uint64_t kept;        /* the sum of |R'(x)| over the slab */
    uint64_t max_degree;  /* the largest deg(x) over ALL stored rows */
} zh_knn_refine_rev_info;
ZH_API int zh_knn_graph_refine_rev_info(const zh_index *idx, zh_knn_refine_rev_info *out);

/* ---- k-NN graph pruning (new): keep only a line's unoccluded neighbours ---------------------------------------------------------------------
 * A k-NN line names the k nearest rows, and most of them lie in the same direction as an earlier one.  HNSW, NSG and Vamana drop a neighbour
 * that is closer to an already kept neighbour than to the row itself; this call is that rule, written in keys.  The INPUT is a graph over ALL
 * stored rows exactly as zh_knn_graph_refine_rev takes it; N'(x) and R'(x) are that call's and zh_knn_graph_reverse's sets, word for word
 * (out-of-range, removed and repeated entries are ignored; R'(x) is zh_knn_graph_reverse's line at rev_k, empty for rev_k = 0).
 *   P(a)     = ( N'(a) union R'(a) ) minus a.  Only the row with a's own row number is excluded; bit-identical duplicates are ordinary candidates.
 *   key_q(x) = zh_distance_batch's key of stored row x against a query equal to the f32 values of stored row q: zh_knn_graph's orientation.
 *   Order P(a) by (key_a(c), id): c_1 .. c_m.  Walk that order with S = O = (), and stop as soon as |S| == degree.  Candidate c is OCCLUDED and
 *   goes to O if some p already in S has key_p(c) < key_a(c) -- on the u64 keys, unsigned and strict, so a tie does not occlude; otherwise c
 *   goes to S.  If fill != 0 and |S| < degree, the first degree - |S| members of O, in their order, join S (HNSW's "keep pruned connections").
 * Line i of the slab, for row a = first_row + i, is S ordered by (key_a, id): out_ids [n][degree] as id_base + row, out_keys the keys key_a,
 * out_counts[i] = |S|, tails UINT64_MAX in both arrays, a removed a has count 0: zh_knn_graph's layout and slab meaning at k = degree.  Ids,
 * keys and counts are bit for bit what this definition gives, for all 13 metric / mode / power combinations and every dimension, whatever the
 * order or repetition of the input entries, the slabs or the run.  Under the parity cosine key (ZH_COSINE_PARITY), whose value is the
 * SIMILARITY, the rule is still the unsigned order of the keys, as for zh_search_range_batch: "closer" there means the smaller key, and the
 * line that comes out is what that key's own ranking calls unoccluded.  No forest is needed.
 * What follows from the definition:
 *   - c_1 is always kept;
 *   - with fill and degree >= |P(a)| the line is P(a) re-keyed;
 *   - with fill = 0 and rev_k = 0 pruning is idempotent: pruning the output at the same degree returns it;
 *   - for a row a inside a block of identical rows its duplicates never occlude each other (key_p(c) == key_a(c): a tie);
 *   - for a row outside such a block the first duplicate occludes the rest (key_p(c) is the key of a row against itself).
 * Limits: degree, in_k and in_k + rev_k at most ZH_REFINE_MAX_IN_K, else ZH_ELIMIT.  Judged before any device is touched, in this order: a null
 * index (even for n = 0), null input or output pointers of a request with n > 0, an unknown metric, degree's limit, in_k's, in_k + rev_k's,
 * in_k = 0 with n > 0 (ZH_EINVAL), a fill other than 0 or 1 (ZH_EINVAL).  Then: first_row + n > stored rows is ZH_EINVAL, n = 0 is ZH_OK,
 * degree = 0 zeroes the counts and touches nothing else.  Locking and stream semantics as zh_knn_graph_refine_device; zh_stats_t, every sibling
 * info struct, the cached live-row views and the attached graph are left alone: zh_knn_graph_prune_info describes the most recent call.
 * A block per live line orders its at most 64 candidates by key_a in LDS, then runs the walk as greedy rounds: the next surviving candidate is
 * kept, becomes the query, and the survivors behind it are keyed against it -- at most degree rounds, nothing per pair leaves the block.
 * Device scratch is per call and released before return: zh_knn_graph_refine_rev's tables, 4 bytes per stored row for the cosine kinds (the
 * rows' norms: computed over ALL stored rows in EVERY call, as the table of row numbers is, whatever the slab -- a caller that prunes slab by
 * slab pays both passes per slab, so few large slabs are cheaper than many small ones), and for the host call 16 degree + 4 bytes per line of a staged slab of at most max(65536, 2^25 / degree) lines.  DESIGN.md s29. */
ZH_API int zh_knn_graph_prune(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, uint64_t first_row, uint64_t n,
                              size_t degree, int fill, int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with the graph and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_knn_graph_prune_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, uint64_t first_row,
                                     uint64_t n, size_t degree, int fill, int metric, int cosine_mode, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                     uint32_t *d_out_counts, void *stream);
typedef struct zh_knn_prune_info {  /* the most recent zh_knn_graph_prune* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint64_t lines;       /* live rows of the slab */
    uint64_t in_k;
    uint64_t rev_k;
    uint64_t degree;
    uint64_t fill;
    uint64_t candidates;  /* the sum of |P(a)| */
    uint64_t kept;        /* the sum of |S| before filling */
    uint64_t occluded;    /* the sum of |O|: candidates the walk examined and dropped */
    uint64_t filled;      /* entries of O that joined a short line */
    uint64_t cut;         /* lines that stopped at `degree` with candidates still unexamined */
    uint64_t keyed;       /* keys computed: candidates <= keyed <= candidates + the sum of |P(a)| (|P(a)| - 1); depends on the schedule */
    uint64_t launches;    /* launches of the line kernel: one per sub-slab of 65536 stored rows that holds a live row */
} zh_knn_prune_info;
ZH_API int zh_knn_graph_prune_info(const zh_index *idx, zh_knn_prune_info *out);

/* ---- NN-descent (new): incremental rounds on the device, to a fixed point --------------------------------------------------------------------
 * A loop over zh_knn_graph_refine_rev keys every pair again in every round and moves the graph through the host between rounds.  This call runs
 * the rounds in one go, keeps the graph on the device, and from the second round on keys only what a NEW entry of a line brings up.  Nothing
 * about the answer is approximate: let G_0 be the caller's graph (all stored rows, in_k wide, judged as zh_knn_graph_refine judges it) and G_r
 * what zh_knn_graph_refine_rev(G_{r-1}, in_k_r, rev_k, k) returns for the whole table, in_k_1 = in_k and in_k_r = k afterwards (rev_k = 0:
 * zh_knn_graph_refine).  The call returns G_rounds, or G_r for the first r whose `updates` is 0 -- ids, keys, tails, counts, a removed row's
 * empty line and the meaning of `updates` (answer entries that the FORWARD input line does not hold) are that call's, bit for bit.
 * Which candidates round r + 1 >= 2 keys (this fixes `keyed`): U_r(x) is the line it ranks over -- N'(G_r)(x), then the kept reverse neighbours
 * R'(x) of G_r.  An entry of U_r(x) is OLD if U_{r-1}(x) holds it, NEW otherwise; every entry of U_0 is new.  For a live row a, S(a) is the set
 * of rows c != a, c not in N'(G_r)(a), such that c is a new entry of U_r(a), or c is in U_r(b) for a new entry b of U_r(a), or c is a new entry
 * of U_r(b) for an old entry b of U_r(a).  The line of a is the first k by (key, id) of S(a) together with N'(G_r)(a), whose entries carry the
 * keys round r wrote (a key is a pure function of the pair).  A line with empty S(a) is inactive: copied, nothing keyed, no updates.  What only
 * old hops reach was a candidate of round r and lost to k rows that are candidates again, so the line equals the full round's.  This needs one k
 * for all rounds and the same live rows throughout: the call holds the index's exclusive lock.
 * Whole table only; outputs [stored rows][k] u64 twice and [stored rows] u32.  Judged before any device is touched, in this order of kinds: a
 * null index, null pointers, an unknown metric, rounds outside 1 .. ZH_DESCENT_MAX_ROUNDS (ZH_EINVAL), k = 0 (ZH_EINVAL), in_k + rev_k or
 * k + rev_k above ZH_REFINE_MAX_IN_K (ZH_ELIMIT), in_k = 0 (ZH_EINVAL).  An empty table is ZH_OK with nothing written.  Any metric, any
 * dimension, no forest needed.  Locking and stream semantics as zh_knn_graph_refine_device; the sibling info structs are left alone.
 * Round 1 is zh_knn_graph_refine_rev's kernels; its ids become u32 row numbers once, and no u64 id leaves the device until the end.  Every later
 * round: (rev_k > 0: transpose and select as zh_knn_graph_reverse,) a wave per line flags its new entries, a wave per live line counts what it
 * would gather and copies a line that gathers nothing, a block per remaining line gathers, de-duplicates, keys and merges with the carried
 * forward line into the OTHER table; one readback of the round's counters decides the early stop.  Device scratch is per call and released
 * before return: beside zh_knn_graph_refine_rev's (with max(in_k, k) for in_k), per stored row 24 k (two u32 tables and two key arrays), 8 (the
 * new-mask), 4 (the squared norms) and, with rev_k > 0, 4 (max(in_k, k) + rev_k) for the second union table; 4 bytes per live row for the list
 * of active lines; round 1's ids and the host entry's answer go through a staged piece of at most max(65536, 2^25 / k) lines of 16 k + 4 bytes.
 * ZH_ENOMEM leaves nothing allocated.  DESIGN.md s23. */
#define ZH_DESCENT_MAX_ROUNDS 32u
ZH_API int zh_knn_graph_descent(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, size_t in_k, size_t rev_k, size_t k, size_t rounds,
                                int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with the graph and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_knn_graph_descent_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, size_t in_k, size_t rev_k, size_t k,
                                       size_t rounds, int metric, int cosine_mode, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts,
                                       void *stream);
typedef struct zh_knn_descent_info {  /* the most recent zh_knn_graph_descent* call on this index */
    uint64_t rows_live;     /* live rows of the index */
    uint32_t in_k;
    uint32_t rev_k;
    uint32_t k;
    uint32_t rounds;        /* asked for */
    uint32_t rounds_run;    /* run: the first round without updates, or `rounds` */
    uint64_t launches;      /* kernel launches of the call's own passes and of the line kernels */
    uint64_t listed;        /* entries gathered before de-duplication, summed over the rounds run */
    uint64_t keyed;         /* pairs that got a key, summed over the rounds run */
    uint64_t lines_active;  /* the sum of active_round */
    uint64_t updates;       /* of the last round run */
    uint64_t large_lines;   /* lines that ran in the large instantiation of a line kernel, over all rounds */
    uint64_t keyed_round[32];    /* per round run: the sum of |S(a)| (round 1: of |C_r(a)|) */
    uint64_t updates_round[32];  /* per round run */
    uint64_t active_round[32];   /* per round run: lines with a non-empty S(a); [0] = the live rows */
} zh_knn_descent_info;
ZH_API int zh_knn_graph_descent_info(const zh_index *idx, zh_knn_descent_info *out);

/* ---- graph search (new): beam search over a k-NN graph kept on the index --------------------------------------------------------------------
 * The graph calls above make a graph and hand it back; these calls keep one on the index and answer queries by walking it.  What is approximate
 * is the set of rows that get a key, never the arithmetic: key(r) below is zh_distance_batch's key of stored row r against the query --
 * zh_search_exact_batch's key, bit for bit, for every metric, mode, power and dimension.
 * The attached graph.  zh_index_set_graph[_device](idx, in_ids, in_counts, g_rows, g_k) takes a graph over the first g_rows stored rows (g_rows <=
 * stored rows; the usual case is all of them), in_ids [g_rows][g_k] u64 in the id space id_base + row and in_counts [g_rows] u32, exactly as
 * zh_knn_graph_refine takes them, and keeps it on the device as the table of u32 row numbers that call makes: entries past the line's count,
 * outside [id_base, id_base + stored rows) (2^64-1 included), naming a removed row or repeated inside their line are masked.  N'(p) at search time
 * is the LIVE rows among line p's unmasked entries, judged against the live rows of the moment of the search: a zh_index_remove after the attach
 * needs no re-attach, a removed row is no candidate and is never expanded, and a row p >= g_rows (appended since the attach) has an empty line
 * until zh_index_extend_graph gives it one.
 * A second set_graph replaces the first; zh_index_drop_graph releases it (ZH_OK with none attached); zh_index_graph_info reports it.  The graph
 * survives append, add, remove, deduplicate, build and set_forest -- rows keep their numbers -- and is dropped by zh_index_compact (rows move) and
 * zh_index_clear.  It is never part of a snapshot: a loaded index has none.  The host entry streams the ids through the pinned chunks of
 * zh_knn_graph_refine's host entry (ZH_REFINE_CHUNK_BYTES).  Judged before any device is touched, in this order: a null index, null arrays with
 * g_rows > 0, g_k = 0 (ZH_EINVAL), g_k > ZH_REFINE_MAX_IN_K (ZH_ELIMIT); under the index's lock: g_rows above the stored rows (ZH_EINVAL), a
 * table of 2^31 rows or more (ZH_ELIMIT: the search keeps a flag beside a row number in one word).  Attach and drop take the lock as a mutation
 * does.  Device memory: 4 g_rows g_k bytes kept; per call, released before return, the host entry's 4 g_rows bytes of counts and one chunk of ids.
 * The search.  For each of the b queries (queries [b][dim] f32, seeds [b][n_seed] u64 in the id space):
 *   1. S(q) = the live stored rows the query's seeds name; a seed that is out of range, removed or repeated is ignored, a seed >= g_rows is
 *      allowed.  The beam B = the first `beam` of S(q) by (key, id), every entry unexpanded.
 *   2. Iteration t = 0, 1, ... stops when t == max_iters (max_iters = 0: no cap) or when B has no unexpanded entry.  Otherwise P = the first
 *      `width` unexpanded entries of B in (key, id) order, marked expanded; cand = the union of N'(p) for p in P, each row once, minus the rows
 *      in B now (the members of P included); cand is keyed, and B becomes the first `beam` of B union cand by (key, id), flags travelling with
 *      their rows.
 *   3. The answer is the first top_k of B in zh_search_exact_batch's layout: out_ids / out_keys [b][top_k], out_counts [b] = min(top_k, |B|),
 *      2^64-1 tails in both arrays, ids carry id_base.  A query with no valid seed has count 0.
 * A row that was keyed and fell out of B can be keyed again; that never changes B (a row only leaves, or fails to enter, a FULL beam, and a full
 * beam's last (key, id) never rises), so answer and iteration count are those of the textbook rule "minus every row keyed so far" -- only
 * `keyed` is larger.  There is no visited set.
 * Limits: 1 <= top_k <= beam <= ZH_GRAPH_MAX_BEAM, 1 <= width with width * g_k <= 256, 1 <= n_seed <= ZH_GRAPH_MAX_SEEDS, max_iters <=
 * ZH_GRAPH_MAX_ITERS.  Judged before any device is touched, in this order of kinds: a null index, null pointers of a request with b > 0, an
 * unknown metric, a zero top_k, beam, width or n_seed (ZH_EINVAL), then the limits (ZH_ELIMIT: beam, top_k > beam, n_seed, width > 256,
 * max_iters); under the lock: no attached graph (ZH_ESTATE), width * g_k > 256 (ZH_ELIMIT).  b = 0 is ZH_OK.  Locking and stream semantics
 * as zh_search_exact_batch_device.  One 256-thread block per query, launches of at most ZH_GRAPH_BATCH queries.  Device scratch is per call and
 * released before return: 4 bytes per query of an internal batch (the cosine norms), 40 bytes of counters, and for the host entry the staged
 * batch: per query 4 dim + 8 n_seed + 16 top_k + 4 bytes.  zh_stats_t and every sibling info struct are left alone.  DESIGN.md s24. */
#define ZH_GRAPH_MAX_BEAM 256u
#define ZH_GRAPH_MAX_SEEDS 64u
#define ZH_GRAPH_MAX_ITERS 65535u
#define ZH_GRAPH_BATCH 16384u  /* queries of one launch */
ZH_API int zh_index_set_graph(zh_index *idx, const uint64_t *in_ids, const uint32_t *in_counts, uint64_t g_rows, size_t g_k);
/* The same with the graph in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_index_set_graph_device(zh_index *idx, const uint64_t *d_in_ids, const uint32_t *d_in_counts, uint64_t g_rows, size_t g_k, void *stream);
ZH_API int zh_index_drop_graph(zh_index *idx);
typedef struct zh_graph_info {  /* the graph attached to this index now */
    uint32_t attached;  /* 1: a graph is attached */
    uint32_t g_k;       /* its line width */
    uint64_t g_rows;    /* its lines */
    uint64_t bytes;     /* device bytes it holds */
} zh_graph_info;
ZH_API int zh_index_graph_info(const zh_index *idx, zh_graph_info *out);
ZH_API int zh_search_graph_batch(zh_index *idx, const float *queries, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k, size_t beam,
                                 size_t width, size_t max_iters, int metric, int cosine_mode, uint64_t *out_ids, uint64_t *out_keys,
                                 uint32_t *out_counts);
/* The same with queries, seeds and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_search_graph_batch_device(zh_index *idx, const float *d_queries, size_t b, const uint64_t *d_seeds, size_t n_seed, size_t top_k,
                                        size_t beam, size_t width, size_t max_iters, int metric, int cosine_mode, uint64_t *d_out_ids,
                                        uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);
typedef struct zh_graph_search_info {  /* the most recent zh_search_graph_batch* call on this index; every field a sum over the batch */
    uint64_t queries;
    uint64_t seeds;       /* valid seeds: the sum of |S(q)| */
    uint64_t iterations;
    uint64_t expanded;    /* the sum of |P| */
    uint64_t keyed;       /* |S(q)| plus every |cand| */
    uint64_t capped;      /* queries stopped by max_iters with an unexpanded entry left */
    uint64_t launches;    /* launches of the search kernel: ceil(b / ZH_GRAPH_BATCH) */
} zh_graph_search_info;
ZH_API int zh_search_graph_info(const zh_index *idx, zh_graph_search_info *out);

/* Filtered graph search (new): zh_search_graph_batch's walk, answered from the rows a bitmap allows.  The arguments are zh_search_graph_batch's
 * plus filter_words / n_bits, which follow zh_search_exact_filtered_batch's convention to the letter: bit r & 31 of filter_words[r >> 5] set =
 * stored row r may be returned; rows at and past n_bits are not allowed; bits of the last word past n_bits are ignored; n_bits >
 * zh_index_stored_rows is ZH_EINVAL; a NULL filter with n_bits > 0 is ZH_EINVAL; one filter serves the batch.
 * THE WALK DOES NOT SEE THE FILTER: S(q), B, P, cand, the flags, the stop rule and max_iters are zh_search_graph_batch's, and navigation goes
 * through every live row, allowed or not.  Let K(q) be the rows that ever get a key: S(q) and every iteration's cand.  The answer is the first
 * top_k by (key, id) of the rows of K(q) that are allowed and live at the time of the search, in zh_search_exact_batch's layout: out_counts[q] =
 * min(top_k, allowed rows in K(q)), entries past it UINT64_MAX, ids carry id_base, every key is zh_distance_batch's.  A row appended since the
 * attach can be a seed and is returned if the mask covers it; a row removed since the attach is neither walked nor returned.  With every stored
 * row allowed the ids, keys and counts are zh_search_graph_batch's bit for bit (B is always the first `beam` of K(q), and top_k <= beam).
 * n_bits = 0, or a filter that allows nothing, gives counts of 0 with the walk still run.
 * The block keeps a second list R beside the beam, the first top_k allowed rows met so far sorted by (key, id): an iteration's candidates whose
 * bit in the allowed-AND-live bitmap is set are merged into it, minus the rows R holds now.  There is no visited set, so an allowed row can be
 * offered again: it is either in R (dropped by that test), or it lost to a full R whose last entry never rises and loses again -- the beam's
 * argument, one list further.
 * Limits and judgement order are zh_search_graph_batch's, top_k <= beam included; the NULL filter is judged with the null pointers (before any
 * device is touched, for any b); n_bits against the stored rows is judged under the lock, after ZH_ESTATE and the width * g_k check.  b = 0 is
 * ZH_OK.  Locking and stream semantics as zh_search_graph_batch_device.  The filter pass (allowed AND live, counted) runs once per call on the
 * call's stream; nothing of it comes back to the host before the launches.  Device scratch is per call and released before return:
 * zh_search_graph_batch's (56 bytes of counters for its 40), the allowed-AND-live bitmap (stored rows / 8 bytes) with 8 bytes per 8192 stored
 * rows of block counts, and for the host entry the staged filter (n_bits / 8 bytes).  zh_search_graph_info, zh_stats_t and every sibling info
 * struct are left alone: zh_search_graph_filtered_info describes the most recent filtered call. */
ZH_API int zh_search_graph_filtered_batch(zh_index *idx, const float *queries, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k,
                                          size_t beam, size_t width, size_t max_iters, int metric, int cosine_mode, const uint32_t *filter_words,
                                          uint64_t n_bits, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with queries, seeds, filter and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_search_graph_filtered_batch_device(zh_index *idx, const float *d_queries, size_t b, const uint64_t *d_seeds, size_t n_seed,
                                                 size_t top_k, size_t beam, size_t width, size_t max_iters, int metric, int cosine_mode,
                                                 const uint32_t *d_filter_words, uint64_t n_bits, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                                 uint32_t *d_out_counts, void *stream);
typedef struct zh_graph_filtered_info {  /* the most recent zh_search_graph_filtered_batch* call on this index */
    uint64_t queries;       /* the first seven: zh_graph_search_info's, and equal to the unfiltered call's at the same arguments */
    uint64_t seeds;
    uint64_t iterations;
    uint64_t expanded;
    uint64_t keyed;
    uint64_t capped;
    uint64_t launches;
    uint64_t rows_allowed;  /* rows both allowed and live: the filter pass's count */
    uint64_t offered;       /* the allowed rows among S(q) and every cand, summed over the batch, repeats included */
    uint64_t returned;      /* the sum of out_counts */
} zh_graph_filtered_info;
ZH_API int zh_search_graph_filtered_info(const zh_index *idx, zh_graph_filtered_info *out);

/* Filter-steered graph search (new): a walk that sees the filter.  The arguments are zh_search_graph_filtered_batch's, in the same positions, plus
 * `hops` (1 or 2) directly after n_bits; the filter convention is the same to the letter (bit r & 31 of filter_words[r >> 5]; rows at and past
 * n_bits are not allowed; spare bits of the last word are ignored; n_bits > zh_index_stored_rows is ZH_EINVAL; a NULL filter with n_bits > 0 is
 * ZH_EINVAL; one filter serves the batch).  A = the rows both allowed and live at the time of the search; a KEPT entry of a line is one the
 * attached table does not mask.  Per query:
 *   1. S(q) = the rows of A the seeds name: a seed that is out of range, removed, NOT ALLOWED or repeated is ignored; a seed >= g_rows is fine.
 *      B = the first `beam` of S(q) by (key, id), every entry unexpanded.  B only ever holds rows of A.
 *   2. Iteration t stops as zh_search_graph_batch's (t == max_iters with max_iters != 0, or no unexpanded entry).  Otherwise P = the first `width`
 *      unexpanded entries of B, marked expanded, and the emission sequence E is built in this order.  First hop: for the parents in P's order, and
 *      per parent its line's kept entries n in table order (a parent >= g_rows has an empty line): n in A is emitted (a DIRECT row); otherwise, if
 *      hops == 2 and n is live, n joins the bridge list H, in this order, each row once; a removed n is skipped.  Second hop (hops == 2): for the
 *      bridges of H in order, and per bridge its line's kept entries m in table order (a bridge >= g_rows has none): m in A is emitted.
 *      cand = E with every repeat after a row's first emission dropped and every row in B now dropped, TRUNCATED TO ITS FIRST 256 ROWS
 *      (ZH_GRAPH_MAX_CAND); width * g_k <= 256, so direct rows are never truncated.  cand is keyed and B = the first `beam` of B union cand by
 *      (key, id), flags travelling with their rows.
 *   3. The answer is the first top_k of B in zh_search_exact_batch's layout: out_counts[q] = min(top_k, |B|), tails UINT64_MAX, ids carry id_base,
 *      every key is zh_distance_batch's.
 * B is still the first `beam` of a superset of itself, so an expanded row that leaves never returns and the walk ends within `stored rows`
 * iterations.  Truncation makes cand depend on B: zh_search_graph_batch's visited-set equivalence does NOT carry over; the definition above is the
 * definition.  With every stored row allowed the ids, keys, counts and the seven walk figures are zh_search_graph_batch's, for either `hops`.
 * n_bits = 0, or a filter that allows nothing, gives counts of 0 and no seed, with the kernel still launched.
 * Limits and judgement order are zh_search_graph_filtered_batch's; hops other than 1 or 2 is ZH_EINVAL, judged last of the scalar limits (after
 * max_iters) and before any device is touched.  No attached graph is ZH_ESTATE.  b = 0 is ZH_OK.  Locking, stream semantics, the filter pass and
 * device scratch as zh_search_graph_filtered_batch (80 bytes of counters for its 56).  zh_search_graph_info, zh_search_graph_filtered_info,
 * zh_stats_t and every sibling info struct are left alone.  DESIGN.md s28. */
#define ZH_GRAPH_MAX_CAND 256u  /* the rows one iteration can key */
ZH_API int zh_search_graph_steered_batch(zh_index *idx, const float *queries, size_t b, const uint64_t *seeds, size_t n_seed, size_t top_k,
                                         size_t beam, size_t width, size_t max_iters, int metric, int cosine_mode, const uint32_t *filter_words,
                                         uint64_t n_bits, int hops, uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* The same with queries, seeds, filter and every output in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_search_graph_steered_batch_device(zh_index *idx, const float *d_queries, size_t b, const uint64_t *d_seeds, size_t n_seed,
                                                size_t top_k, size_t beam, size_t width, size_t max_iters, int metric, int cosine_mode,
                                                const uint32_t *d_filter_words, uint64_t n_bits, int hops, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                                uint32_t *d_out_counts, void *stream);
typedef struct zh_graph_steered_info {  /* the most recent zh_search_graph_steered_batch* call on this index; sums over the batch */
    uint64_t queries;       /* the first seven: zh_graph_search_info's meanings under this walk */
    uint64_t seeds;         /* the sum of |S(q)| */
    uint64_t iterations;
    uint64_t expanded;
    uint64_t keyed;         /* seeds + direct + via_bridge */
    uint64_t capped;
    uint64_t launches;
    uint64_t rows_allowed;  /* rows both allowed and live: the filter pass's count */
    uint64_t direct;        /* first-hop members of every cand */
    uint64_t via_bridge;    /* second-hop members of every cand */
    uint64_t bridges;       /* the sum over iterations of |H|, read or not */
    uint64_t cand_full;     /* iterations whose |cand| == ZH_GRAPH_MAX_CAND */
    uint64_t returned;      /* the sum of out_counts */
} zh_graph_steered_info;
ZH_API int zh_search_graph_steered_info(const zh_index *idx, zh_graph_steered_info *out);

/* Extending the attached graph (new): lines for the rows stored since the attach, and reverse edges to them.  G = the rows the attached table
 * covers (zh_graph_info.g_rows), N = the stored rows at the time of the call, g_k = the table's width.  The new rows G .. N-1 are taken in chunks
 * of `batch` consecutive stored rows: chunk c is [lo, hi), lo = G + c batch, hi = min(N, lo + batch).  While chunk c is processed the table covers
 * [0, lo): the earlier chunks' lines and every change they made to older lines included.  A chunk has two steps.
 *   1. Search.  For every live row a of [lo, hi): zh_search_graph_batch's walk, bit for bit, with stored row a as the query, the [lo][g_k] table,
 *      liveness as of now, and the caller's n_seed seeds for a (seeds [n_new][n_seed], line a - G) -- but a seed naming a row >= lo is ignored: such
 *      a row has no line yet.  That covers a itself and the rows of its chunk, and no line names a row >= lo, so a line never holds its own row.
 *      line(a) = the first min(g_k, |B|) rows of the final beam in (key, id) order.  A removed row of the chunk gets an empty line.
 *   2. Reverse edges.  For every live row r < lo let R(r) = the live rows a of the chunk whose line(a) holds r.  If R(r) is empty, line r is left
 *      untouched word for word: masked entries and entries naming rows removed since the attach stay.  Otherwise line r becomes the first g_k of
 *      L'(r) union R(r) by (key_r(x), x), the rest UINT32_MAX: L'(r) = the kept entries of line r that are live now, key_r(x) = the key
 *      zh_search_exact_batch gives stored row x against a query equal to stored row r (zh_knn_graph's orientation).
 * ROWS OF ONE CHUNK NEVER NAME EACH OTHER, and a chunk's old rows are re-ranked against that chunk only: the price of walking a chunk's rows in
 * parallel.  batch = 1 is the fully sequential rule.  zh_index_get_graph, a round of zh_knn_graph_descent over it and zh_index_set_graph close
 * what is left.  The metric is the caller's, as for the search: the graph records none.
 * Limits: 1 <= g_k <= beam <= ZH_GRAPH_MAX_BEAM (the walk's top_k is g_k), width * g_k <= 256, 1 <= n_seed <= ZH_GRAPH_MAX_SEEDS, max_iters <=
 * ZH_GRAPH_MAX_ITERS, 1 <= batch <= ZH_GRAPH_EXTEND_MAX_BATCH (a re-ranked line then holds at most 64 + 1024 candidates).  Judged before any
 * device is touched, in this order: a null index, null seeds with n_new > 0, an unknown metric, a zero beam, width, n_seed or batch (ZH_EINVAL),
 * then the limits (ZH_ELIMIT: beam, n_seed, width > 256, max_iters, batch); under the lock: no attached graph (ZH_ESTATE), g_k > beam, width * g_k
 * > 256, a table of 2^31 rows or more (ZH_ELIMIT), n_new != N - G (ZH_EINVAL: the table changed between the caller's sizing and the call).  N == G
 * (and n_new == 0) is ZH_OK with nothing done.  The new [N][g_k] table is made beside the old one -- a copy, then the chunks -- and swapped in at
 * the end: a failed call leaves what was attached.  Afterwards zh_graph_info.g_rows = N, and every rule of the attached graph above holds for the
 * extended one as it is.  The call takes the lock as a mutation does; the device entry takes seeds in device memory and is enqueued on `stream`
 * (NULL = the index's own), complete on return.  Device scratch is per call and released before return: the walk's staged chunk (per row of a
 * chunk 4 dim + 8 n_seed + 16 g_k + 8 bytes), 16 bytes per stored row of in-degrees, cursors and offsets, 4 bytes per stored row of norms
 * (cosine), 8 batch g_k bytes of edges and touched rows, and for the host entry the staged seeds.  DESIGN.md s27. */
#define ZH_GRAPH_EXTEND_MAX_BATCH 1024u
ZH_API int zh_index_extend_graph(zh_index *idx, const uint64_t *seeds, uint64_t n_new, size_t n_seed, size_t beam, size_t width, size_t max_iters,
                                 size_t batch, int metric, int cosine_mode);
ZH_API int zh_index_extend_graph_device(zh_index *idx, const uint64_t *d_seeds, uint64_t n_new, size_t n_seed, size_t beam, size_t width,
                                        size_t max_iters, size_t batch, int metric, int cosine_mode, void *stream);
typedef struct zh_graph_extend_info {  /* the most recent zh_index_extend_graph* call on this index */
    uint64_t rows_added;       /* live new rows: each got a line */
    uint64_t rows_removed;     /* new rows that were removed already: each got an empty line */
    uint64_t chunks;
    uint64_t seeds;            /* the next five: zh_graph_search_info's, summed over the walks of the live new rows */
    uint64_t iterations;
    uint64_t expanded;
    uint64_t keyed;
    uint64_t capped;
    uint64_t reverse_rows;     /* old rows re-ranked, summed over the chunks */
    uint64_t reverse_offered;  /* the sum of |R(r)| */
    uint64_t reverse_kept;     /* chunk rows that ended inside a re-ranked line */
    uint64_t launches;         /* launches of the walk and of the re-ranking kernel */
} zh_graph_extend_info;
ZH_API int zh_index_extend_graph_info(const zh_index *idx, zh_graph_extend_info *out);
/* Reading the attached table (new).  Line i of out_ids [n][g_k] holds the kept entries of line first_row + i in table order, compacted to the front
 * as id_base + row; out_counts[i] is their number and the tail is 2^64-1.  Entries are as stored: a row removed since the attach is still listed
 * (the search and zh_knn_graph_refine skip it themselves).  zh_index_set_graph of the answer attaches the same kept entries in the same order,
 * less those naming rows removed since (which it masks, and which no walk saw): every search answers alike, and a table of compact lines (every line
 * the extension wrote is one) without such entries comes back word for word.  A null index, null outputs with n > 0 (ZH_EINVAL); under
 * the lock: no graph (ZH_ESTATE), first_row + n > g_rows (ZH_EINVAL).  n = 0 is ZH_OK.  The host entry stages slabs of 2^18 lines. */
ZH_API int zh_index_get_graph(zh_index *idx, uint64_t first_row, uint64_t n, uint64_t *out_ids, uint32_t *out_counts);
ZH_API int zh_index_get_graph_device(zh_index *idx, uint64_t first_row, uint64_t n, uint64_t *d_out_ids, uint32_t *d_out_counts, void *stream);

/* ---- forest self-join (new): all near-duplicate pairs AMONG LEAF-MATES ---------------------------------------------------------------------
 * zh_self_join multiplies every tile of the table by every tile at or above it; this call multiplies a leaf only by itself.  Arguments, key,
 * orientation, threshold, output arrays, order, ids and the capacity contract are zh_self_join's.  Let
 *   F = the unordered pairs {a, b} of distinct stored rows that are members of the SAME leaf in at least one tree,
 * with membership as zh_index_get_forest's leaf_ids has it at the time of the call: removed rows have left every tree, rows appended since the
 * last build are in none.  The answer is every pair of F whose key is <= max_key, EACH PAIR ONCE however many trees put the two rows together:
 * three parallel arrays out_a, out_b, out_keys of *out_total entries, a < b by row number, ids = id_base + row, ascending by (a, key, b).  The
 * key of (a, b) is the key zh_distance_batch gives for stored row b against a query equal to the f32 values of row a.  ONE threshold key per
 * call (zebra_amd.radius_key); UINT64_MAX returns all of F; the parity cosine key's unsigned order is the definition.
 * Only the candidate set is approximate: ids, keys, order and total are bit for bit what that definition gives with zh_distance_batch's keys, for
 * all 13 metric / mode / power combinations, whatever the path, the scan's row order or the run.  On a forest of ONE tree whose root is a leaf
 * the answer is zh_self_join's; for any forest it is the subset of zh_self_join's pairs that lie in F, and the quotient of the two totals is the
 * pair recall of the forest setting.
 * More pairs than `capacity`: ZH_ELIMIT with *out_total EXACT (a pair that several trees repeat is counted once) and the arrays unspecified;
 * capacity = 0 with NULL arrays counts only.  A NULL index or out_total, NULL arrays with capacity > 0 and an unknown metric are refused before
 * any device is touched; after them an index without live rows has no pair (*out_total = 0, ZH_OK), and one with live rows and no trees, or
 * with trees an interrupted insert left stale, is ZH_ESTATE, as for zh_knn_graph_forest.  A forest whose leaves all hold fewer than two rows
 * gives *out_total = 0 and ZH_OK.  Locking as zh_self_join_device;
 * zh_stats_t, the six sibling info structs and the cached live-row views are left alone: zh_self_join_forest_info describes the most recent call.
 * Each pair once: the call builds leaf_of[row][tree], the row's leaf in that tree, on the device, and a pair met in tree t is kept only if the
 * two rows share no leaf in any tree t' < t -- the first tree that puts them together owns the pair.  The rule is paid only by
 * candidates (path 2) or by keys already at or below the threshold (path 1).
 * Both paths work tree after tree into ONE hit pool.  Path 1 (every metric, dimension and leaf shape): the rows a tree holds are lines, each
 * visits its own leaf in that tree; the leaf-major f32 sweep keys the leaf's rows against the line and the keys <= max_key whose row number is
 * above the line's and that pass the rule are hits.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, the fp16 row copy
 * present, zh_options.max_node_size >= 64): a tree's non-empty leaves are cut into batches of at most 2048 tiles of 16 rows (or one longer leaf
 * alone), a batch is gathered once out of the copy and ONE launch multiplies every leaf of it by itself on the matrix cores, the tiles on or
 * above each leaf's diagonal only, for an interval per pair; pairs whose interval reaches down to the threshold are candidates, and those the
 * rule leaves get the canonical key.  A batch whose candidates outgrow their pool has nothing counted and its leaves are answered by path 1
 * (`redone`).  ZH_FJOIN_PATH=1 in the environment (read per call) forces path 1; ZH_FJOIN_CAND_CAP=n (read per call; tests) sets the candidate
 * pool's slots per batch.
 * Device scratch is per call and released before return: 4 bytes per (stored row, tree) of leaf_of -- 4 N T, 600 MB at 10M rows x 15 trees, not
 * chunked -- and 4 bytes per tree node; with P = min(capacity, the forest's leaf pairs) hit slots 32 P bytes of hit pool and sort buffers + the
 * sort's temporary storage; path 2 per batch 2 dim + 28 bytes per gathered row (at most max(32768, the longest leaf padded to tiles)), 16 bytes
 * per 64 gathered rows of segments and 8 bytes per candidate slot (max(1.25 x the capacity left, 256 per gathered row), never more than the
 * batch's leaf pairs), plus 4 bytes per stored row under a scan order that is not id order; path 1 per panel of at most 16384 lines 4 dim + 24
 * bytes per line, 56 bytes per 4 lines and 8 bytes per key of at most max(2^25, the longest leaf) keys; for the host call 24 bytes per pair. */
ZH_API int zh_self_join_forest(zh_index *idx, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *out_a, uint64_t *out_b,
                               uint64_t *out_keys, uint64_t *out_total);
/* The same with every output (out_total included) in device memory; enqueued on `stream` (NULL = the index's own stream), complete on return. */
ZH_API int zh_self_join_forest_device(zh_index *idx, uint64_t max_key, int metric, int cosine_mode, uint64_t capacity, uint64_t *d_out_a,
                                      uint64_t *d_out_b, uint64_t *d_out_keys, uint64_t *d_out_total, void *stream);
typedef struct zh_join_forest_info {  /* the most recent zh_self_join_forest* call on this index */
    uint64_t rows_live;   /* live rows of the index */
    uint32_t trees;       /* trees of the forest */
    uint32_t path;        /* 1: the f32 leaf sweep, each line over its own leaf; 2: matrix-core intervals leaf by leaf, canonical keys for candidates */
    uint64_t leaf_pairs;  /* sum over all trees' leaves of len (len - 1) / 2, counted from the forest on the device: repeats across trees included */
    uint64_t pairs;       /* pairs within the threshold, each once (exact whatever the capacity) */
    uint64_t candidates;  /* path 2: pairs that got the canonical key, over the batches path 2 completed */
    uint64_t launches;    /* launches of the scan (panels swept on path 1, one matrix-core launch per batch on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued, from the launch geometry (t (t + 1) / 2 per leaf of t tiles); 0 on path 1 */
    uint32_t redone;      /* path-2 batches whose candidate pool ran over and were answered by path 1 */
} zh_join_forest_info;
ZH_API int zh_self_join_forest_info(const zh_index *idx, zh_join_forest_info *out);

/* ---- forest range search (new): all rows within a radius AMONG THE VISITED LEAVES ------------------------------------------------------------
 * zh_search_range_batch multiplies every query by every live row; this call scores a query only against the leaves the forest's walk visits for
 * it.  The arguments, the CSR result, the keys, the (key, id) order, id_base, UINT64_MAX = "every candidate" and the capacity contract (ZH_ELIMIT
 * with *out_total and ALL offsets exact; capacity = 0 with NULL arrays counts only) are zh_search_range_batch's; `probe` comes after max_keys.
 * Candidate set.  The candidates of query i are every member of every leaf that the reference's walk (tree_result, lsh.rs:290-348: what
 * zh_search_batch(top_k = probe) performs) visits for that query with n = probe, the union over all trees taken as a set.  A visited leaf
 * contributes ALL its rows, not only the rows a top-k search would keep of it.  The visit sequence depends on leaf lengths and plane signs only,
 * never on the metric.  probe = 1 .. ZH_MAX_TOPK; probe = 1 is the leaf the query hashes to in each tree (plus the backups of empty leaves).
 * Known behaviour of the walk: once probe exceeds the typical leaf length the backups cascade and most of a tree is visited -- at
 * max_node_size 5, 15 trees and 2000 rows, probe = 10 visits about 5400 leaves per query.  Removed rows are in no leaf and are never hits; rows
 * appended since the last build are in no leaf and are never hits.
 * Only the candidate set is approximate: the answer is exactly the subset of zh_search_range_batch's hits that are candidates, bit for bit, for
 * all 13 metric / mode / power combinations and every dimension, whatever the path, the scan's row order or the run.  A row that several trees or
 * several visited leaves offer comes once.  On a forest of ONE tree whose root is a leaf the answer is zh_search_range_batch's.
 * A NULL index, q or max_keys with b > 0, NULL out_offsets / out_total, NULL out_ids / out_keys with capacity > 0, an unknown metric, probe = 0
 * (ZH_EINVAL) and probe > ZH_MAX_TOPK (ZH_ELIMIT) are refused before any device is touched.  b = 0, an empty index and an index of removed rows
 * only give all-zero offsets and ZH_OK; an index with live rows and no trees, or with trees an interrupted insert left stale, is ZH_ESTATE, as
 * for zh_self_join_forest.  Locking as zh_search_range_batch_device; zh_stats_t, every sibling info struct, the cached live-row views and the
 * search contexts of the LSH search (their running means included) are left alone: zh_search_range_forest_info describes the most recent call.
 * Internal batches of at most 1024 queries.  The walk runs with the LSH search's own kernels on scratch of this call; its totals reach the host
 * before the scoring is sized, and an internal batch whose visits hold more than 2^25 rows (256 MiB of path-1 keys) is cut in half, query-wise,
 * until it fits or is one query.  Each hit once: with leaf_of[row][tree] (as zh_self_join_forest) a pair (query, row) met in a visited leaf of
 * tree t is kept only if the row's leaf in no earlier tree is among the leaves the query visited there; the lookup is the query's own visit list,
 * ordered by leaf.  Path 1 (every metric, dimension and leaf shape): the f32 leaf sweep keys every visited row, and the keys at
 * or below the threshold that pass the rule are hits.  Path 2 (ZH_L2SQ, ZH_L2, ZH_COSINE at dim 256 / 384 / 512 / 768 / 1024, the fp16 row copy
 * present, zh_options.max_node_size >= 64): the visited leaves, in batches of at most 2048 tiles of 16 rows (or one longer leaf alone), are
 * gathered once out of the copy and ONE launch per batch multiplies each leaf's row tiles by the 16-query column tiles of that leaf's visitors on
 * the matrix cores, for an interval per pair; pairs whose interval reaches down to the threshold and that pass the rule are candidates and get
 * the canonical key (zh_search_range_batch's survivor pass).  Path 2 is leaf-major: it pays where leaves are shared, so an internal batch whose
 * visited leaves have fewer than 32 visitors on average stays on path 1 (its tile columns would be mostly padding and the gather would move more
 * bytes than the sweep reads; DESIGN.md s19, measured).  An internal batch whose candidates outgrow their pool is answered by path 1 (`redone`).
 * ZH_FRANGE_PATH in the environment (read per call): 1 forces path 1, 2 takes path 2 wherever the rule above admits it, whatever the visitor
 * count; ZH_FRANGE_CAND_CAP=n (read per call; tests) sets the candidate pool's slots per internal batch.
 * Device scratch is per call and released before return: 4 bytes per (stored row, tree) of leaf_of and 4 bytes per tree node; per internal batch
 * 16 bytes per tree node, about 1.3 KB per (query, tree) pair, 56 bytes per leaf visit and 14 bytes per (leaf, visitor); path 1 8 bytes per
 * visited row (at most 2^25 of them, or one query's); path 2 per batch of leaves 2 dim + 12 bytes per gathered row (at most max(32768, the
 * longest leaf padded to tiles)), 2 dim + 24 bytes per query and 8 bytes per candidate slot (max(1.25 x the capacity left, 4096 per query), never
 * more than the visited rows); with P = min(capacity left, visited rows) hit slots 32 P bytes of hit pool and sort buffers + the sort's temporary
 * storage; for the host call 16 bytes per hit of the batch. */
ZH_API int zh_search_range_forest_batch(zh_index *idx, const float *q, size_t b, const uint64_t *max_keys, uint32_t probe, int metric, int cosine_mode,
                                        uint64_t capacity, uint64_t *out_offsets, uint64_t *out_ids, uint64_t *out_keys, uint64_t *out_total);
/* The same with queries, thresholds and every output (out_total included) in device memory; enqueued on `stream` (NULL = the index's own stream),
 * complete on return. */
ZH_API int zh_search_range_forest_batch_device(zh_index *idx, const float *d_q, size_t b, const uint64_t *d_max_keys, uint32_t probe, int metric,
                                               int cosine_mode, uint64_t capacity, uint64_t *d_out_offsets, uint64_t *d_out_ids, uint64_t *d_out_keys,
                                               uint64_t *d_out_total, void *stream);
typedef struct zh_range_forest_info {  /* the most recent zh_search_range_forest_* call on this index */
    uint64_t batch;       /* queries */
    uint64_t rows_live;   /* live rows of the index */
    uint32_t trees;       /* trees of the forest */
    uint32_t probe;       /* the walk's n */
    uint32_t path;        /* 1: the f32 leaf sweep over the visits; 2: matrix-core intervals leaf by leaf, canonical keys for candidates */
    uint32_t redone;      /* path-2 internal batches answered by path 1 because the candidate pool ran over */
    uint64_t visits;      /* leaf visits over all queries and trees, from the walk (it records a visit where it takes rows: no empty leaf) */
    uint64_t leaf_rows;   /* sum of the visited leaves' lengths over all visits: the work before sharing and de-duplication */
    uint64_t hits;        /* (row, query) pairs within their query's threshold, each once (exact whatever the capacity) */
    uint64_t candidates;  /* path 2: pairs that got the canonical key, over the internal batches path 2 completed */
    uint64_t launches;    /* launches of the scoring kernel (the sweep on path 1, one matrix-core launch per batch of leaves on path 2) */
    uint64_t tiles;       /* path 2: 16 x 16 tile products issued: per internal batch the sum over visited leaves of ceil(len / 16) x
                             ceil(visitors / 16); 0 on path 1 */
} zh_range_forest_info;
ZH_API int zh_search_range_forest_info(const zh_index *idx, zh_range_forest_info *out);

/* Pipelined form of zh_search_batch_device (new; the reference has one blocking search per query): a context
 * is one in-flight batch with its own scratch.  The context calls do NOT take the index's internal lock (the blocking
 * calls do): contexts of one index may be driven from several threads, one thread per context at a time, concurrently with
 * each other and with blocking searches -- they share only read-only index state and the statistics of zh_stats (guarded
 * separately) -- but never concurrently with add / build / set_forest / remove / clear / destroy on that index.
 * begin enqueues the hash and the walk's counting pass on
 * `stream` and returns; finish waits (host side) only for three totals, then enqueues the distance sweep,
 * the selection and the final top-k and returns; wait blocks until the results are complete.  With two
 * contexts on two streams one host thread keeps the sweep of batch i and the small latency-bound kernels of
 * batches i and i+1 on the GPU together.  Queries and outputs must stay valid until wait, and the outputs are complete only
 * when wait has returned -- a stream sync is not enough: a prefiltered batch (zh_set_sweep_mode) whose candidate lists ran over is
 * redone with the sweep inside wait. */
typedef struct zh_search_ctx zh_search_ctx;
ZH_API int zh_search_ctx_create(zh_index *idx, zh_search_ctx **out);
ZH_API void zh_search_ctx_destroy(zh_search_ctx *ctx);
ZH_API int zh_search_begin(zh_search_ctx *ctx, const float *d_q, size_t b, size_t k, int metric, int cosine_mode,
                    void *stream);
/* A lowest-priority, non-blocking stream owned by the index, meant to be passed as `sweep_stream` below: light kernels
 * (high-priority streams) and collectives (normal priority) then never share a hardware queue with the sweeps. */
ZH_API void *zh_index_sweep_stream(const zh_index *idx);
/* sweep_stream (may be NULL = the begin stream): the stream the HBM-bound distance sweep is enqueued on; sharing
 * one sweep stream between contexts runs the sweeps of successive batches back to back while the other kernels of
 * each batch overlap them on the contexts' own streams (the library inserts the event dependencies). */
ZH_API int zh_search_finish(zh_search_ctx *ctx, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts,
                     void *sweep_stream);
ZH_API int zh_search_wait(zh_search_ctx *ctx);
/* A WINDOW: n_batches batches (same b, k and metric; queries at n_batches device pointers) handled as ONE internal batch.
 * The walk, the leaf groups and the sweep span the whole window, so a stored row crosses HBM once per group of queries of
 * the WINDOW that score it -- with b << leaves per tree, two batches share rows a single batch cannot -- and the light
 * kernels are launched once per window.  Results are delivered per batch (n_batches output pointers each), bit-identical
 * to n_batches separate calls; the price is latency: no batch of the window completes before the whole window has.
 * zh_search_wait as for a single batch.  The counters of zh_stats then describe the window (batch = n_batches * b). */
#define ZH_MAX_WINDOW 64u
ZH_API int zh_search_begin_window(zh_search_ctx *ctx, const float *const *d_q, size_t n_batches, size_t b, size_t k, int metric,
                                  int cosine_mode, void *stream);
ZH_API int zh_search_finish_window(zh_search_ctx *ctx, uint64_t *const *d_out_ids, uint64_t *const *d_out_keys,
                                   uint32_t *const *d_out_counts, void *sweep_stream);

/* Metric::distance(stored=a[i], query=q) for n stored rows against one query (host pointers).  Device buffers are kept
 * per calling thread between calls (a pair costs two small copies in, three small kernels, one copy out).
 * COST of the single-pair forms (n = 1, zh_distance_pair): tens of microseconds -- a host -> device copy, three launches and a
 * blocking copy back -- where the crate's Metric::distance spends ~100 ns in simsimd (distance.rs:21-31).  There is deliberately
 * no host-side arithmetic behind this ABI (every key this library returns comes from the gfx950 kernels: one implementation
 * to hold bit-exact, and nothing that could pass for a CPU fallback): a caller that needs isolated pairs at CPU speed keeps the
 * crate's own metric for them (the shim routes Metric::distance to the crate, batches to this library). */
ZH_API int zh_distance_batch(int metric, int cosine_mode, const float *a, const float *q, size_t n, size_t dim,
                      uint64_t *out_keys, int device);
ZH_API int zh_distance_pair(int metric, int cosine_mode, const float *a, const float *b, size_t dim, uint64_t *out_key,
                     int device);

/* Shard merge: S lists of b x k (ids, keys) with counts S x b, all in device memory (e.g. the
 * output of an RCCL all-gather of every rank's zh_search_batch_device result) -> b x k merged.
 * The kernel is enqueued on `stream` and the call returns; synchronise the stream before reading.
 * The contract, per query, of this call and of zh_merge_topk_packed_device:
 *   - list s contributes its entries j < min(d_counts[s*b + q], k).  Slots past a list's count are never read,
 *     whatever they hold, and a count above k is treated as k;
 *   - the answer is the k smallest of those entries by (key, id) as unsigned 64-bit pairs; identical (key, id)
 *     pairs from different lists appear once (a repeated id is expected to carry the same key, as one row does);
 *   - d_out_counts[q] is the number of entries kept; output slots past it are UINT64_MAX in ids and in keys;
 *   - an entry whose key AND id are both UINT64_MAX is that marker of an empty slot and is dropped;
 *   - the inputs are not written, and nothing outside the b*k ids, b*k keys and b counts of the outputs is.
 * top_k outside 1..1024 is ZH_ELIMIT, n_shards outside 1..1024 and a null pointer with b > 0 are ZH_EINVAL, all judged
 * before a device is touched; b = 0 is ZH_OK and launches nothing. */
ZH_API int zh_merge_topk_device(int device, uint32_t n_shards, size_t b, size_t k, const uint64_t *d_ids,
                         const uint64_t *d_keys, const uint32_t *d_counts, uint64_t *d_out_ids,
                         uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);

/* The same merge over ONE buffer per shard -- [ids b*k u64][keys b*k u64][counts b u32, padded to 8 bytes],
 * zh_packed_result_words(b, k) u64 words -- so that a batch needs a single all-gather: point
 * zh_search_batch_device / zh_search_finish at the three sections of such a buffer. */
ZH_API size_t zh_packed_result_words(size_t b, size_t k);
ZH_API int zh_merge_topk_packed_device(int device, uint32_t n_shards, size_t b, size_t k, const uint64_t *d_packed,
                                uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts, void *stream);

/* ---- sharded search: rows partitioned over GPUs, one RCCL all-gather per batch ---------------------------------
 * One process per GPU (the harness' model) -- or several groups in one process, one per device.  Every rank owns an
 * ordinary zh_index over its rows (its own forest, options.id_base = global id of its first row) and joins a group;
 * a search on the group is then ONE call per batch on every rank, with the same queries everywhere:
 *     local zh_search on this rank's shard -> ncclAllGather of the packed [ids | keys | counts] result (in place,
 *     b*k*16 + b*4 bytes per rank) -> merge_wave_kernel on every rank -> every rank holds the global top-k.
 * top-k(union of the shards' top-k) == top-k(union of the shards' candidates), so the result is bit-identical to the
 * reference searching S independent LSHIndex instances and merging by (key, id).
 * The library links librccl itself; the caller only moves the 128-byte unique id from rank 0 to the other ranks
 * (any host channel: a file, MPI, a torch.distributed store).
 * Calls on one group must come from one thread at a time and in the same order on every rank (they are collectives).
 *
 * Errors are a GROUP outcome (the reference swallows a failed query, core.rs:303; a collective cannot): a rank whose local
 * search fails still joins the all-gather, with an empty slot and its code in a status word that travels with the packed
 * result (zh_shard_exchange_words = zh_packed_result_words + 1).  zh_shard_search_wait -- and the blocking calls -- then
 * return the rank's own code, or ZH_EPEER where only other ranks failed: the same verdict everywhere, nobody hangs, the group
 * stays usable.  The blocking calls split a batch that passes a per-launch limit IDENTICALLY on every rank (a ZH_ELIMIT
 * anywhere makes every rank halve the chunk and repeat it; the first size comes from the largest visits-per-query any rank
 * reported).  Pipelined calls: after a begin that returned an error, STILL call finish (it joins the exchange and returns the
 * error) and wait.  A rank that dies or cannot join is bounded by ZH_SHARD_TIMEOUT_MS (environment, default 300000): wait
 * aborts the communicator, returns ZH_EPEER, and the group is dead (later calls fail fast; destroy it). */
typedef struct zh_shard_group zh_shard_group;
#define ZH_UNIQUE_ID_BYTES 128
ZH_API int zh_shard_unique_id(uint8_t out_id[ZH_UNIQUE_ID_BYTES]); /* rank 0: ncclGetUniqueId */
/* collective over the n_ranks callers (ncclCommInitRank on the shard's device).  The group borrows `shard`, which must
 * outlive it; rows may still be added to the shard between searches. */
ZH_API int zh_shard_group_create(zh_index *shard, const uint8_t id[ZH_UNIQUE_ID_BYTES], uint32_t n_ranks, uint32_t rank,
                                 zh_shard_group **out);
ZH_API void zh_shard_group_destroy(zh_shard_group *grp);
ZH_API uint32_t zh_shard_group_ranks(const zh_shard_group *grp); /* ncclCommCount: the ranks RCCL actually connected */
ZH_API uint32_t zh_shard_group_rank(const zh_shard_group *grp);
/* Blocking search over the whole sharded index; queries / results in device memory on every rank (d_out_* receive the
 * MERGED global top-k, same layout as zh_search_batch_device). */
ZH_API int zh_shard_search_batch_device(zh_shard_group *grp, const float *d_q, size_t b, size_t k, int metric, int cosine_mode,
                                        uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts);
/* The same from / to host memory (what a Rust Database::query_vectors over a sharded index calls). */
ZH_API int zh_shard_search_batch(zh_shard_group *grp, const float *q, size_t b, size_t k, int metric, int cosine_mode,
                                 uint64_t *out_ids, uint64_t *out_keys, uint32_t *out_counts);
/* Pipelined form, as zh_search_begin / finish / wait: a context is one batch in flight with its own streams (light
 * kernels: high priority; exchange + merge: normal priority, beside the next batch's sweep on the index's sweep stream).
 * finish enqueues sweep, select, final, the all-gather and the merge and returns; wait blocks until the merged results
 * are complete.  zh_shard_ctx_stream is the stream they complete on (enqueue result copies behind it). */
typedef struct zh_shard_ctx zh_shard_ctx;
ZH_API int zh_shard_ctx_create(zh_shard_group *grp, zh_shard_ctx **out);
ZH_API void zh_shard_ctx_destroy(zh_shard_ctx *ctx);
ZH_API int zh_shard_search_begin(zh_shard_ctx *ctx, const float *d_q, size_t b, size_t k, int metric, int cosine_mode);
ZH_API int zh_shard_search_finish(zh_shard_ctx *ctx, uint64_t *d_out_ids, uint64_t *d_out_keys, uint32_t *d_out_counts);
ZH_API int zh_shard_search_wait(zh_shard_ctx *ctx);
/* windows, as zh_search_begin_window / zh_search_finish_window: one all-gather and one merge per window */
ZH_API int zh_shard_search_begin_window(zh_shard_ctx *ctx, const float *const *d_q, size_t n_batches, size_t b, size_t k,
                                        int metric, int cosine_mode);
ZH_API int zh_shard_search_finish_window(zh_shard_ctx *ctx, uint64_t *const *d_out_ids, uint64_t *const *d_out_keys,
                                         uint32_t *const *d_out_counts);
ZH_API void *zh_shard_ctx_stream(const zh_shard_ctx *ctx);
/* this rank's own (unmerged) packed result of the context's last finished batch: zh_packed_result_words(b, k) words */
ZH_API const uint64_t *zh_shard_ctx_local_result(const zh_shard_ctx *ctx);
/* The status protocol, as pure host arithmetic (no GPU needed; tests carry it over gloo).  Words per rank in the exchange;
 * a rank's status word = its local status (low 32 bits, sign-extended zh_status) | leaf visits per query it has seen << 32;
 * the verdict every rank derives from the n_ranks gathered words: ZH_OK, status_words[rank]'s own code, or ZH_EPEER.
 * out_* may be NULL: first failed rank (n_ranks if none), largest visits-per-query reported, 1 if every failure is ZH_ELIMIT. */
ZH_API size_t zh_shard_exchange_words(size_t b, size_t k);
ZH_API uint64_t zh_shard_status_word(int status, uint32_t visits_per_query);
ZH_API int zh_shard_verdict(const uint64_t *status_words, uint32_t n_ranks, uint32_t rank, uint32_t *out_first_failed_rank,
                            uint32_t *out_max_visits_per_query, int *out_all_elimit);

/* synthetic queries on the device (bit-identical to oracle zo_synth_queries) */
ZH_API int zh_synth_queries_device(int device, float *d_out, uint64_t seed_rows, uint64_t seed_q, uint64_t n_rows,
                            uint64_t b0, size_t b, uint32_t dim, int kind, void *stream);

/* ---- the reference's on-disk VALUES ------------------------------------------------
 * The reference stores an index in two fjall partitions (lsh.rs:62-120): "<uuid>-embeddings" maps a vector's 16 uuid
 * bytes to bincode(legacy) Embedding<N> -- exactly the N little-endian f32 that zh_index_append takes, no codec
 * needed (lsh.rs:91-97, lib.rs:15-18) -- and "<uuid>-trees" maps a tree's uuid to bincode(legacy) Node<N>
 * (lsh.rs:46-60,99-105).  The host shim, which links fjall, iterates the partitions; these functions turn the tree
 * values into the flat forest of zh_index_set_forest and back, so an existing database can be served by the GPU
 * path and a GPU-built forest can be saved in the reference's format.  Host code only (no GPU needed).  fjall's own
 * file layout is not read.  Byte layout: zebra_amd/csrc/zh_refformat.cpp (FORMAT UNVERIFIED against the crates).
 *
 * decode: `uuids` holds the keys of the n_vectors stored rows in row order (row i of zh_index_append <-> uuids[16 i]);
 * leaf ids that are not among them (vectors removed by the reference, whose trees keep them, lsh.rs:473-503) are
 * dropped and counted in out_unknown_ids (may be NULL). */
typedef struct zh_ref_forest zh_ref_forest;
ZH_API int zh_ref_forest_decode(uint32_t dim, size_t n_trees, const uint8_t *const *values, const size_t *lens,
                                size_t n_vectors, const uint8_t *uuids, zh_ref_forest **out, uint64_t *out_unknown_ids);
/* borrowed pointers, valid until zh_ref_forest_free */
ZH_API int zh_ref_forest_view(const zh_ref_forest *forest, zh_forest_view *out);
ZH_API void zh_ref_forest_free(zh_ref_forest *forest);
/* one tree of a flat forest as bincode(legacy) Node<N>; uuids = 16 bytes per row.  out == NULL: only *out_len (the
 * size needed) is written. */
ZH_API int zh_ref_tree_encode(const zh_forest_view *forest, uint32_t dim, uint32_t tree, const uint8_t *uuids,
                              uint64_t n_rows, uint8_t *out, size_t cap, size_t *out_len);

/* The database header, the `.zebra` file (core.rs:19-29 DatabaseInner, written by save_database core.rs:183-190, read by open
 * core.rs:92-102): bincode(legacy) { uuid, model: Mod, metric: Met, index_options }.  Met and Mod are type parameters of the
 * crate, so the file does not record them: the caller states the metric (only MinkowskiDistance / PNormDistance carry bytes:
 * their i32 power) and the length of the model's serialisation (0 for the reference's three unit-struct models).  Host code. */
typedef struct zh_ref_header {
    uint8_t uuid[16];         /* DatabaseInner::uuid: the prefix of the two partition names "<uuid>-embeddings" / "<uuid>-trees" */
    uint64_t max_node_size;   /* LSHIndexOptions (lsh.rs:124-129), usize as u64 */
    uint64_t num_trees;
    int32_t metric;           /* zh_metric as stated by the caller */
    int32_t power;            /* MinkowskiDistance / PNormDistance { power } (distance.rs:160-190); 0 for the other metrics */
    uint64_t model_off, model_len; /* where the model's own bytes sit inside the file */
} zh_ref_header;
ZH_API int zh_ref_header_decode(const uint8_t *bytes, size_t len, int metric, size_t model_len, zh_ref_header *out);
/* out == NULL: only *out_len (the size needed) is written */
ZH_API int zh_ref_header_encode(const zh_ref_header *header, const uint8_t *model_bytes, uint8_t *out, size_t cap, size_t *out_len);

/* ---- test / debug access: what the half-width scans computed for EVERY scored pair --------------------------------
 * The half-width scans (zh_set_sweep_mode 4 / 5 / 6) give every member of every visited leaf -- every (stored row, query) pair that
 * tree_result scores with Metric::distance (lsh.rs:310-323; distance.rs:23,41,106) -- an interval that must CONTAIN the reference's key; only
 * then are the returned ids / keys the reference's.  These two calls let a test check that claim pair by pair on the device's own numbers
 * (tests/test_gpu_intervals.py) instead of end to end: zh_debug_keep_raw(idx, 1) makes every later half-width batch keep a copy of the
 * scan's raw output {x^ . h^ / sigma_x, |x|^2} (the intervals overwrite it in place); zh_debug_scan_pairs returns, for the most recent
 * batch of `ctx` (NULL: the index's blocking context, i.e. the last zh_search_batch_device call; the context must be idle), one record per
 * scored pair.  lo / hi are f32 values in the scale the scan ranks in, mapped to order-preserving u32 ("sortable": bits ^ (sign ? ~0 :
 * 0x80000000)): L2 family: the canonical f32 sum of (x_i - q_i)^2; cosine, corrected key: the clipped distance 1 - cos; the reference's
 * literal key (distance.rs:23-25): key > 0 ? key : 2 - key for key = 1 - distance.  (lo, hi) = (0, ~0): nothing is certain about the pair
 * (it takes the exact path).  Not a product path: host-side copies of the whole batch's scratch.  While zh_debug_keep_raw is on, the d = 128
 * half-width sweep is never FUSED (a fused sweep -- zh_stats_t::approx_fused -- writes no per-pair result at all: zh_debug_scan_pairs after one
 * returns ZH_ESTATE). */
typedef struct zh_debug_pair {
    uint32_t row;          /* stored row (local: without id_base) */
    uint32_t query;        /* query of the batch (of the window: batch * b + i) */
    uint32_t lo, hi;       /* the interval, sortable f32 (valid when flags & 1) */
    float raw_s, raw_a2;   /* the scan's raw output for the pair (valid when zh_debug_scan_info::raw_kept) */
    uint32_t flags;        /* 1: the visit's raw pairs were turned into intervals (every visit that hands rows on); 2: a visit that takes FEWER
                            * than top_k rows of a longer leaf -- ranked by the reference's arithmetic, its intervals only gate the query's list */
    uint32_t visit;        /* index of the leaf visit the pair belongs to */
} zh_debug_pair;
typedef struct zh_debug_scan_info {
    uint32_t approx_scan;  /* as zh_stats_t::approx_scan: 1 VALU scan, 2 matrix-core scan, 3 leaf-major at half width; 0: the batch was not half-width */
    uint32_t queries, top_k;
    int32_t metric, cosine_mode;
    uint32_t raw_kept;     /* 1: raw_s / raw_a2 are valid */
    uint32_t overflow;     /* the batch's overflow word (non-zero: it was redone by the f32 path; the intervals are still what the scan made) */
    float bound_const;     /* zh_approx_bound for the batch ("Half-width scan: the bound") */
    float row_rho, rho_norm; /* the measured relative rounding error of the stored rows' fp16 copy (0 with f32 rows) */
    uint64_t pairs, visits;
} zh_debug_scan_info;
ZH_API int zh_debug_keep_raw(zh_index *idx, int on);
/* out (cap records; NULL with cap 0 to size: info->pairs) in key-slot order; qmeta (may be NULL): queries x 4 floats {1 / sigma_q, f32 |q|^2,
 * upper estimate of |q|, upper estimate of |q - h / sigma_q|} (NaN: nothing certain about the query) */
ZH_API int zh_debug_scan_pairs(zh_index *idx, zh_search_ctx *ctx, zh_debug_scan_info *info, zh_debug_pair *out, size_t cap, float *qmeta);

/* ---- test / debug access: the intervals of the joins' and the graphs' matrix-core scans, pair by pair -------------------
 * zh_self_join, zh_cross_join, zh_knn_graph, zh_knn_graph_forest and zh_self_join_forest (their path 2) never compute the key of most pairs: a
 * 16 x 16 block of dot products of two tiles of the fp16 row copies gives every pair an interval, the "query" of the pair being a STORED row of
 * the copy (its rounding assumed from the copy's rho, not measured), and only pairs whose interval reaches the threshold get the canonical key.
 * The answers are the reference's only if every interval contains the key.  zh_debug_walk_pairs lets a test check that pair by pair
 * (tests/test_gpu_pair_intervals.py): it runs the same held-tile walk -- the same tile product, LDS double buffer, per-position views and interval
 * arithmetic -- with a sink that RECORDS instead of judging, over the rectangle
 *     held positions [first_pos, first_pos + n_pos) of `left`'s copy  x  every position of `right`'s copy (16 * ceil(stored rows / 16) of them),
 * one record per pair, at (held_pos - first_pos) * info->col_positions + col_pos.  `right` == `left`: the self-join's and the graphs' view; another
 * index: the cross join's (the held side takes left's rho, right's rho goes into the column rows' query view).  A position is a place in the
 * copy: row number = position unless the copy is in a row order.  held_row / col_row = the row number at the position, UINT32_MAX for a removed row
 * and for the tail of the last tile (masked: the product scans make no pair of it; lo / hi / raw_s of such a record mean nothing).  lo / hi: as
 * zh_debug_pair's, (0, ~0) = nothing certain.  raw_s = the block's sum for the pair times the held row's 1 / sigma, i.e. x^ . y^ / sigma_x with the
 * column row still scaled.  first_pos must be a multiple of 64, n_pos at most 1024, the slab inside the copy; dim and metric those the
 * matrix-core scans serve (else ZH_EINVAL).  out == NULL with cap 0: only *info.  cap < info->pairs: ZH_ELIMIT, *info is set and nothing is
 * stored.  Not a product path: both indexes are locked for the call, the records are staged in device memory and copied out. */
typedef struct zh_debug_walk_pair {
    uint32_t held_pos, col_pos;  /* positions in left's / right's copy */
    uint32_t held_row, col_row;  /* local row numbers (without id_base), or UINT32_MAX: masked */
    uint32_t lo, hi;             /* the interval, sortable f32 */
    float raw_s;
} zh_debug_walk_pair;
typedef struct zh_debug_walk_info {
    uint64_t pairs;              /* records of the rectangle = held_positions * col_positions */
    uint64_t held_positions, col_positions;
    float bound_const;           /* zh_approx_bound of the family scans */
    float rho_left, rho_right;   /* the two copies' measured relative rounding error */
    uint32_t order_left, order_right; /* 1: that copy is in a row order (positions are not row numbers) */
} zh_debug_walk_info;
ZH_API int zh_debug_walk_pairs(zh_index *left, zh_index *right, int metric, int cosine_mode, uint64_t first_pos, uint64_t n_pos,
                               zh_debug_walk_info *info, zh_debug_walk_pair *out, size_t cap);

/* ---- instrumentation ------------------------------------------------------------------------ */
ZH_API int zh_set_profiling(zh_index *idx, int level); /* 0 off, 1 per-stage hipEvent timing, 2 + unique-row count */
ZH_API int zh_stats(zh_index *idx, zh_stats_t *out);
ZH_API int zh_stats_reset(zh_index *idx);
/* number of leading tree levels hashed by the dense MFMA kernel; -1 = choose per batch (default) */
ZH_API int zh_set_dense_levels(zh_index *idx, int levels);
/* How the distance sweep of a batch is organised: 1 = leaf by leaf (the rows of every visited leaf are gathered from HBM once
 * per group of <= 4 queries that visit it), 2 = table scan (every stored row is streamed from HBM once per batch window, in
 * address order, and scored against every query that visits one of its num_trees leaves; the queries come from L2), 0 = the
 * library chooses per batch from the counted work (default).  Results are bit-identical in both.
 * A batch whose hash came from row scores (zh_set_hash_mode) holds row . query for every stored row, i.e. every L2 / L2^2 / cosine
 * distance of the batch up to rounding.  In mode 0 (and 3 = the same, stated) such a batch is PREFILTERED instead of swept: per
 * (query, tree) the visited leaves' rows are judged on their scores with a rigorous rounding bound -- which `take` rows a leaf
 * hands over (lsh.rs:300-330), and which of those can still be among the k nearest -- and only the survivors, plus every visit the
 * bound cannot decide, are scored with the reference's arithmetic; ids, keys and counts stay bit-identical.  Modes 1 and 2 always
 * sweep.  (max_node_size <= 8 and no leaf longer than 64 rows, top_k <= 64, forests built by this library.)
 * The table scan of mode 0 reads HALF-WIDTH (fp16) copies of the queries where that pays (L2 / L2^2 / cosine keys, dim 256 / 384 /
 * 512 / 768 / 1024, top_k <= 256, two or more scored (row, query) pairs per stored row): 2 * dim instead of 4 * dim bytes per pair, an
 * INTERVAL per pair that contains the reference's key (the fp16 roundings measured, every f32 rounding bounded), the candidates
 * picked on the intervals and only the rows they cannot rule out scored with the reference's arithmetic -- ids, keys and counts
 * stay bit-identical.  With up to 16 trees the products run on the matrix cores from an fp16 copy of the STORED ROWS that the
 * index makes on first use and extends as rows are appended: + 2 * dim + 8 bytes per stored row of device memory (+50 % of the row
 * table; skipped, and the f32 rows read by a VALU kernel instead, when less than that plus a sixteenth of the device is free).
 * A list that runs over is redone by the f32 scan on the device, in stream order (no host round trip: safe for callers that
 * consume results in stream order).  Mode 2 keeps the f32 scan; 4 = the half-width scan wherever it is implemented (dim 128 ...
 * 1024), whatever the cost model says; 5 = as 4 with the VALU kernel only (no copy of the rows).
 * 128-d tables (SIFT-style shards) whose batches score 4M rows or more leaf by leaf get the same treatment on the leaf-major sweep: a row-major
 * fp16 copy of the rows under ONE power-of-two scale (+ 256 bytes per stored row; exact for integer-valued rows; rows the scale does not serve
 * are scored exactly), 16-row tiles on the matrix cores, the same intervals and exact passes behind; 6 = that sweep wherever it is
 * implemented, 1 keeps the f32 sweep.  zh_stats_t::approx_* report it. */
ZH_API int zh_set_sweep_mode(zh_index *idx, int mode);
/* How a batch that needs EVERY sign of the forest (small leaves: the reference's default max_node_size 5) gets them:
 * 1 = one dot product per (query, plane), 2 * b * planes * dim flop on the matrix cores; 2 = from row scores: a plane is built from
 * two stored rows a, b (build_hyperplane, lsh.rs:192-225), and in exact arithmetic w.x + c = (b.x - |b|^2/2) - (a.x - |a|^2/2),
 * so b * rows dot products decide all planes (planes / rows ~ 6.5x fewer flop at the default options); a sign closer to zero than
 * a rigorous bound on the rounding that separates the two computations is recomputed with point_is_above's own arithmetic, so
 * the bits are identical.  Only for forests built or grown by this library (an injected forest has arbitrary planes);
 * 0 = chosen per batch (default). */
ZH_API int zh_set_hash_mode(zh_index *idx, int mode);

ZH_API const char *zh_last_error(void);
ZH_API const char *zh_version(void);
/* Device memory.  The library caches no device memory: every buffer an index or a search context lets go of goes back to the driver.  This call
 * does nothing and returns ZH_OK; it stays in the ABI for callers that already use it. */
ZH_API int zh_trim_device_memory(void);

#ifdef __cplusplus
}
#endif
#endif /* ZEBRA_HIP_H */

// zebra.hpp -- C++17 host-side mirror of the reference crate's interface for the hot path, over the C ABI
// of zebra_hip.h.  The reference is Rust; no Rust toolchain exists in the build image, so the host layer
// above the ABI is written in C++ with the crate's names, argument meaning and error behaviour
// (anyhow::Result<T> -> zebra::Error thrown).
//
//   reference                                   here
//   Embedding<N>            src/lib.rs:15-46                     zebra::Embedding<N>
//   EmbeddingPrecision=f32  src/lib.rs:48                        zebra::EmbeddingPrecision
//   DistanceUnit = u64      src/distance.rs:13                   zebra::DistanceUnit
//   space::Metric<Embedding<N>>::distance  src/distance.rs:19-21 Met::distance(a, b) const
//   CosineDistance<N>       src/distance.rs:15-32                zebra::CosineDistance<N>
//   L2SquaredDistance<N>    src/distance.rs:34-49                zebra::L2SquaredDistance<N>
//   L2Distance<N>           src/distance.rs:99-114               zebra::L2Distance<N>
//   LSHIndexOptions<N>      src/database/index/lsh.rs:122-139    zebra::LSHIndexOptions<N>
//   LSHIndex<N>             src/database/index/lsh.rs:144-565    zebra::LSHIndex<N>
//   Database<N,Met,Mod>     src/database/core.rs:45-313          zebra::Database<N,Met> (insert_records/query_vectors)
//
// Ids are dense row numbers (uint64_t) where the crate uses Uuid v7 (lsh.rs:415); a shim that needs Uuids
// keeps a row -> Uuid table.
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "zebra_hip.h"

namespace zebra {

using EmbeddingPrecision = float;   // lib.rs:48
using DistanceUnit = std::uint64_t; // distance.rs:13
using Id = std::uint64_t;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
    if (rc != ZH_OK) throw Error(rc, zh_last_error());
}

template <std::size_t N>
struct Embedding : std::array<EmbeddingPrecision, N> {  // lib.rs:18; Default = zeros (lib.rs:30-34)
    Embedding() { this->fill(0.0f); }
    explicit Embedding(const std::array<EmbeddingPrecision, N> &a) : std::array<EmbeddingPrecision, N>(a) {}
};

// ---- src/distance.rs: zero-sized metric structs implementing space::Metric with Unit = u64 ------------
namespace detail {
template <std::size_t N>
DistanceUnit metric_pair(int metric, int mode, const Embedding<N> &a, const Embedding<N> &b, int device) {
    DistanceUnit out = 0;
    check(zh_distance_pair(metric, mode, a.data(), b.data(), N, &out, device));
    return out;
}
}  // namespace detail

template <std::size_t N>
struct CosineDistance {
    // parity = true keeps distance.rs:23-25 literally (key = bits of 1.0 - simsimd cosine distance)
    bool parity = true;
    int device = -1;
    static constexpr int metric = ZH_COSINE;
    int mode() const { return parity ? ZH_COSINE_PARITY : ZH_COSINE_CORRECTED; }
    DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {
        return detail::metric_pair<N>(metric, mode(), a, b, device);
    }
};
template <std::size_t N>
struct L2SquaredDistance {
    int device = -1;
    static constexpr int metric = ZH_L2SQ;
    int mode() const { return ZH_COSINE_PARITY; }
    DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {
        return detail::metric_pair<N>(metric, mode(), a, b, device);
    }
};
template <std::size_t N>
struct L2Distance {
    int device = -1;
    static constexpr int metric = ZH_L2;
    int mode() const { return ZH_COSINE_PARITY; }
    DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {
        return detail::metric_pair<N>(metric, mode(), a, b, device);
    }
};

// the `distances`-crate metrics (distance.rs:51-98,116-190): key = f32 bits widened; Hamming an integer count
#define ZEBRA_SIMPLE_METRIC(NAME, CODE)                                                         \
    template <std::size_t N>                                                                    \
    struct NAME {                                                                               \
        int device = -1;                                                                        \
        static constexpr int metric = CODE;                                                     \
        int mode() const { return 0; }                                                          \
        DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {             \
            return detail::metric_pair<N>(metric, 0, a, b, device);                             \
        }                                                                                       \
    };
ZEBRA_SIMPLE_METRIC(ChebyshevDistance, ZH_CHEBYSHEV)
ZEBRA_SIMPLE_METRIC(CanberraDistance, ZH_CANBERRA)
ZEBRA_SIMPLE_METRIC(BrayCurtisDistance, ZH_BRAY_CURTIS)
ZEBRA_SIMPLE_METRIC(ManhattanDistance, ZH_MANHATTAN)
ZEBRA_SIMPLE_METRIC(L3Distance, ZH_L3)
ZEBRA_SIMPLE_METRIC(L4Distance, ZH_L4)
ZEBRA_SIMPLE_METRIC(HammingDistance, ZH_HAMMING)
#undef ZEBRA_SIMPLE_METRIC
template <std::size_t N>
struct MinkowskiDistance {  // distance.rs:160-174; #[derive(Default)] -> power 0, any i32 is legal
    int power = 0;
    int device = -1;
    static constexpr int metric = ZH_MINKOWSKI;
    int mode() const { return power; }
    DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {
        return detail::metric_pair<N>(metric, power, a, b, device);
    }
};
template <std::size_t N>
struct PNormDistance {  // distance.rs:176-190; #[derive(Default)] -> power 0, any i32 is legal
    int power = 0;
    int device = -1;
    static constexpr int metric = ZH_PNORM;
    int mode() const { return power; }
    DistanceUnit distance(const Embedding<N> &a, const Embedding<N> &b) const {
        return detail::metric_pair<N>(metric, power, a, b, device);
    }
};

// ---- src/database/index/lsh.rs ------------------------------------------------------------------------
template <std::size_t N>
struct LSHIndexOptions {  // lsh.rs:122-139
    std::size_t max_node_size = 5;
    std::size_t num_trees = 15;
};

template <std::size_t N>
class LSHIndex {  // Clone in the crate shares the store (lsh.rs:144-148): copies share one zh_index
  public:
    // LSHIndex::new (lsh.rs:162-167); seed/device/id_base are the knobs the crate does not have
    explicit LSHIndex(const LSHIndexOptions<N> &options = {}, std::uint64_t seed = 0x5EB2A003ull, int device = -1,
                      std::uint64_t id_base = 0) {
        zh_options o;
        zh_options_default(&o);
        o.dim = (std::uint32_t)N;
        o.max_node_size = (std::uint32_t)options.max_node_size;
        o.num_trees = (std::uint32_t)options.num_trees;
        o.seed = seed;
        o.device = device;
        o.id_base = id_base;
        zh_index *h = nullptr;
        check(zh_index_create(&o, &h));
        h_.reset(h, zh_index_destroy);
    }
    void save() const {}  // the crate's own persistence goes through fjall (lsh.rs:170-172): not this path; snapshots are below
    // (new) zh_index_save: the index as ONE snapshot file -- rows (removed ones included), removals, forest, the planes' sample rows -- written
    // beside `path` first and renamed over it.  Needs the exclusion of add.
    zh_snapshot_info save(const std::string &path) const {
        zh_snapshot_info info;
        check(zh_index_save(h_.get(), path.c_str(), &info));
        return info;
    }
    // (new) zh_index_load: a new index from a snapshot, indistinguishable from the saved one for every later call (N must be the file's dim)
    static LSHIndex load(const std::string &path, int device = -1, std::uint64_t reserve_rows = 0, zh_snapshot_info *info = nullptr) {
        zh_snapshot_info seen;
        check(zh_snapshot_inspect(path.c_str(), 0, &seen));
        if (seen.dim != N) throw Error(ZH_EINVAL, "zebra: snapshot " + path + " holds vectors of another dimension");
        zh_index *h = nullptr;
        check(zh_index_load(path.c_str(), device, reserve_rows, &h, info));
        LSHIndex out(Adopt{}, h);
        return out;
    }

    bool no_vectors() const { return zh_index_count(h_.get()) == 0; }     // lsh.rs:398-400
    bool no_trees() const { return zh_index_num_trees(h_.get()) == 0; }   // lsh.rs:407-409
    bool is_empty() const { return no_vectors() || no_trees(); }          // lsh.rs:389-391

    // lsh.rs:440-466 -> ids of the added vectors
    std::vector<Id> add(const std::vector<Embedding<N>> &embeddings) const {
        std::vector<Id> ids(embeddings.size());
        check(zh_index_add(h_.get(), embeddings.empty() ? nullptr : embeddings[0].data(), embeddings.size(), ids.data()));
        return ids;
    }
    void clear() const { check(zh_index_clear(h_.get())); }  // lsh.rs:506-529
    // lsh.rs:473-503 (as intended: the ids leave every tree) -> the ids that were present
    std::vector<Id> remove(const std::vector<Id> &embedding_ids) const {
        std::vector<std::uint8_t> found(embedding_ids.size());
        std::size_t n = 0;
        check(zh_index_remove(h_.get(), embedding_ids.data(), embedding_ids.size(), found.data(), &n));
        std::vector<Id> out;
        for (std::size_t i = 0; i < found.size(); i++) if (found[i]) out.push_back(embedding_ids[i]);
        return out;
    }
    // lsh.rs:270-288 -> ids removed because an earlier vector has the same bits
    std::vector<Id> deduplicate() const {
        std::vector<Id> out(zh_index_count(h_.get()) + 1);
        std::size_t n = 0;
        check(zh_index_deduplicate(h_.get(), out.data(), out.size(), &n));
        out.resize(n < out.size() ? n : out.size());
        return out;
    }
    // (new) zh_index_compact: the device memory of removed vectors is reclaimed in place -> for every OLD local row its new id, or
    // UINT64_MAX for a removed one (stable: strictly increasing on the live rows); every later call answers as before under that map
    std::vector<Id> compact(zh_compact_info *info = nullptr) const {
        std::vector<Id> new_ids(zh_index_stored_rows(h_.get()));
        check(zh_index_compact(h_.get(), new_ids.data(), new_ids.size(), info));
        return new_ids;
    }

    // lsh.rs:544-565: approximate k nearest neighbours, ascending by (distance key, id)
    template <class Met>
    std::vector<std::pair<Id, DistanceUnit>> search(const Embedding<N> &query, std::size_t top_k, const Met &metric) const {
        return std::move(search_batch(std::vector<Embedding<N>>{query}, top_k, metric)[0]);
    }
    // the rayon loop of core.rs:299-303 as one call
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_batch(const std::vector<Embedding<N>> &queries,
                                                                         std::size_t top_k, const Met &metric) const {
        const std::size_t b = queries.size();
        std::vector<Id> ids(b * top_k);
        std::vector<DistanceUnit> keys(b * top_k);
        std::vector<std::uint32_t> counts(b);
        check(zh_search_batch(h_.get(), b ? queries[0].data() : nullptr, b, top_k, Met::metric, metric.mode(), ids.data(),
                              keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    // exact k nearest neighbours over every live stored row (zh_search_exact_batch): same keys and order as search_batch, no forest needed
    template <class Met>
    std::vector<std::pair<Id, DistanceUnit>> search_exact(const Embedding<N> &query, std::size_t top_k, const Met &metric) const {
        return std::move(search_exact_batch(std::vector<Embedding<N>>{query}, top_k, metric)[0]);
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_exact_batch(const std::vector<Embedding<N>> &queries,
                                                                               std::size_t top_k, const Met &metric) const {
        const std::size_t b = queries.size();
        std::vector<Id> ids(b * top_k);
        std::vector<DistanceUnit> keys(b * top_k);
        std::vector<std::uint32_t> counts(b);
        check(zh_search_exact_batch(h_.get(), b ? queries[0].data() : nullptr, b, top_k, Met::metric, metric.mode(), ids.data(),
                                    keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    // the exact k nearest neighbours among the live rows a bitmap allows (zh_search_exact_filtered_batch): bit r & 31 of filter_words[r >> 5]
    // set = stored row r may be returned; n_bits rows are spoken for, rows past them are not allowed.  One filter for the whole batch.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_exact_filtered_batch(const std::vector<Embedding<N>> &queries, std::size_t top_k,
                                                                                        const Met &metric,
                                                                                        const std::vector<std::uint32_t> &filter_words,
                                                                                        std::uint64_t n_bits) const {
        const std::size_t b = queries.size();
        if (filter_words.size() < (n_bits + 31) / 32) throw std::invalid_argument("search_exact_filtered_batch: filter shorter than n_bits");
        std::vector<Id> ids(b * top_k);
        std::vector<DistanceUnit> keys(b * top_k);
        std::vector<std::uint32_t> counts(b);
        check(zh_search_exact_filtered_batch(h_.get(), b ? queries[0].data() : nullptr, b, top_k, Met::metric, metric.mode(),
                                             n_bits ? filter_words.data() : nullptr, n_bits, ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    zh_filtered_info filtered_info() const {
        zh_filtered_info info{};
        check(zh_search_filtered_info(h_.get(), &info));
        return info;
    }
    // every live row whose key is <= the query's threshold key (zh_search_range_batch), ascending by (key, id): one call that counts, one that
    // fetches.  max_keys: one key per query (~0 = every live row); for L2 squared, L2 and cosine a key is the f64 bit pattern of the distance.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_range_batch(const std::vector<Embedding<N>> &queries,
                                                                               const std::vector<DistanceUnit> &max_keys, const Met &metric) const {
        const std::size_t b = queries.size();
        if (max_keys.size() != b) throw std::invalid_argument("search_range_batch: one threshold key per query");
        std::vector<std::uint64_t> offsets(b + 1);
        std::uint64_t total = 0;
        const int rc = zh_search_range_batch(h_.get(), b ? queries[0].data() : nullptr, b, max_keys.data(), Met::metric, metric.mode(), 0,
                                             offsets.data(), nullptr, nullptr, &total);
        if (rc != ZH_ELIMIT) check(rc);
        std::vector<Id> ids(total + 1);
        std::vector<DistanceUnit> keys(total + 1);
        if (total)
            check(zh_search_range_batch(h_.get(), queries[0].data(), b, max_keys.data(), Met::metric, metric.mode(), total, offsets.data(), ids.data(),
                                        keys.data(), &total));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint64_t j = offsets[i]; j < offsets[i + 1]; j++) out[i].emplace_back(ids[j], keys[j]);
        return out;
    }
    zh_range_info range_info() const {
        zh_range_info info{};
        check(zh_search_range_info(h_.get(), &info));
        return info;
    }
    // every pair of distinct live rows (a, b), a < b, whose key (stored row b against a query equal to row a) is <= max_key (zh_self_join),
    // ascending by (a, key, b): one call that counts, one that fetches.  max_key: ~0 = every pair.
    struct JoinedPair {
        Id a, b;
        DistanceUnit key;
    };
    template <class Met>
    std::vector<JoinedPair> self_join(DistanceUnit max_key, const Met &metric) const {
        std::uint64_t total = 0;
        const int rc = zh_self_join(h_.get(), max_key, Met::metric, metric.mode(), 0, nullptr, nullptr, nullptr, &total);
        if (rc != ZH_ELIMIT) check(rc);
        std::vector<Id> a(total + 1), b(total + 1);
        std::vector<DistanceUnit> keys(total + 1);
        if (total) check(zh_self_join(h_.get(), max_key, Met::metric, metric.mode(), total, a.data(), b.data(), keys.data(), &total));
        std::vector<JoinedPair> out(total);
        for (std::uint64_t i = 0; i < total; i++) out[i] = JoinedPair{a[i], b[i], keys[i]};
        return out;
    }
    zh_join_info join_info() const {
        zh_join_info info{};
        check(zh_self_join_info(h_.get(), &info));
        return info;
    }
    // the join between two indexes (zh_cross_join): every pair (live row a of this index, live row b of `other`) whose key (stored row b of
    // `other` against a query equal to row a) is <= max_key, ascending by (a, key, b); a carries this index's id_base, b other's.  One call that
    // counts, one that fetches.  `other` must be a different index of the same dim on the same device.
    template <class Met>
    std::vector<JoinedPair> cross_join(const LSHIndex &other, DistanceUnit max_key, const Met &metric) const {
        std::uint64_t total = 0;
        const int rc = zh_cross_join(h_.get(), other.h_.get(), max_key, Met::metric, metric.mode(), 0, nullptr, nullptr, nullptr, &total);
        if (rc != ZH_ELIMIT) check(rc);
        std::vector<Id> a(total + 1), b(total + 1);
        std::vector<DistanceUnit> keys(total + 1);
        if (total) check(zh_cross_join(h_.get(), other.h_.get(), max_key, Met::metric, metric.mode(), total, a.data(), b.data(), keys.data(), &total));
        std::vector<JoinedPair> out(total);
        for (std::uint64_t i = 0; i < total; i++) out[i] = JoinedPair{a[i], b[i], keys[i]};
        return out;
    }
    zh_cross_info cross_info() const {
        zh_cross_info info{};
        check(zh_cross_join_info(h_.get(), &info));
        return info;
    }
    // the exact k-NN graph of the slab of stored rows [first_row, first_row + n) (zh_knn_graph): element i = the k nearest OTHER live rows of stored
    // row first_row + i by (key, id), the key that of the neighbour against a query equal to the row; empty for a removed row.  k <= ZH_MAX_TOPK - 1.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph(std::size_t k, const Met &metric, std::uint64_t first_row, std::uint64_t n) const {
        std::vector<Id> ids(n * k + 1);
        std::vector<DistanceUnit> keys(n * k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_knn_graph(h_.get(), first_row, n, k, Met::metric, metric.mode(), ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph(std::size_t k, const Met &metric) const {
        return knn_graph(k, metric, 0, zh_index_stored_rows(h_.get()));
    }
    zh_knn_info knn_info() const {
        zh_knn_info info{};
        check(zh_knn_graph_info(h_.get(), &info));
        return info;
    }
    // the k-NN join between two indexes over the slab of this index's stored rows [first_row, first_row + n) (zh_cross_knn): element i = the k
    // nearest live rows of `other` to stored row first_row + i by (key, id), the key that of other's stored row against a query equal to the row
    // (other.search_exact's answer); ids carry other's id_base; empty for a removed row.  `other` must be a different index of the same dim on the
    // same device.  k <= ZH_MAX_TOPK.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> cross_knn(const LSHIndex &other, std::size_t k, const Met &metric, std::uint64_t first_row,
                                                                    std::uint64_t n) const {
        std::vector<Id> ids(n * k + 1);
        std::vector<DistanceUnit> keys(n * k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_cross_knn(h_.get(), other.h_.get(), first_row, n, k, Met::metric, metric.mode(), ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> cross_knn(const LSHIndex &other, std::size_t k, const Met &metric) const {
        return cross_knn(other, k, metric, 0, zh_index_stored_rows(h_.get()));
    }
    zh_xknn_info cross_knn_info() const {
        zh_xknn_info info{};
        check(zh_cross_knn_info(h_.get(), &info));
        return info;
    }
    // the forest k-NN graph of the slab (zh_knn_graph_forest): knn_graph's shape, the candidates of a row being the rows that share a leaf with it
    // in some tree; empty for a removed row and for a row no tree holds.  Needs a built forest.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_forest(std::size_t k, const Met &metric, std::uint64_t first_row, std::uint64_t n) const {
        std::vector<Id> ids(n * k + 1);
        std::vector<DistanceUnit> keys(n * k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_knn_graph_forest(h_.get(), first_row, n, k, Met::metric, metric.mode(), ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_forest(std::size_t k, const Met &metric) const {
        return knn_graph_forest(k, metric, 0, zh_index_stored_rows(h_.get()));
    }
    zh_knn_forest_info knn_forest_info() const {
        zh_knn_forest_info info{};
        check(zh_knn_graph_forest_info(h_.get(), &info));
        return info;
    }
    // One refinement round over a graph of ALL stored rows (zh_knn_graph_refine): in_ids [stored rows][in_k] in the outputs' id space, in_counts
    // [stored rows] -- what knn_graph / knn_graph_forest give for the whole table, flattened.  Element i = the first k by (key, id) of stored row
    // first_row + i's neighbours and their neighbours, the row itself excluded; entries that are out of range, removed or repeated are ignored.
    // k <= ZH_MAX_TOPK - 1, in_k <= ZH_REFINE_MAX_IN_K.  No forest needed.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_refine(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                           std::size_t in_k, std::size_t k, const Met &metric, std::uint64_t first_row,
                                                                           std::uint64_t n) const {
        const std::uint64_t stored = zh_index_stored_rows(h_.get());
        if (in_counts.size() != stored || in_ids.size() != stored * in_k) throw std::invalid_argument("knn_graph_refine: the graph must cover every stored row");
        std::vector<Id> ids(n * k + 1);
        std::vector<DistanceUnit> keys(n * k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_knn_graph_refine(h_.get(), in_ids.data(), in_counts.data(), in_k, first_row, n, k, Met::metric, metric.mode(), ids.data(), keys.data(),
                                  counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_refine(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                           std::size_t in_k, std::size_t k, const Met &metric) const {
        return knn_graph_refine(in_ids, in_counts, in_k, k, metric, 0, zh_index_stored_rows(h_.get()));
    }
    // the same with the graph and the outputs in device memory, enqueued on `stream` (nullptr: the index's own), complete on return
    template <class Met>
    void knn_graph_refine_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::size_t in_k, std::uint64_t first_row, std::uint64_t n,
                                 std::size_t k, const Met &metric, Id *d_out_ids, DistanceUnit *d_out_keys, std::uint32_t *d_out_counts,
                                 void *stream = nullptr) const {
        check(zh_knn_graph_refine_device(h_.get(), d_in_ids, d_in_counts, in_k, first_row, n, k, Met::metric, metric.mode(), d_out_ids, d_out_keys,
                                         d_out_counts, stream));
    }
    zh_knn_refine_info knn_refine_info() const {
        zh_knn_refine_info info{};
        check(zh_knn_graph_refine_info(h_.get(), &info));
        return info;
    }
    // The same round with up to rev_k sampled reverse neighbours of every row -- the rows that name it, picked by a hash of the pair -- and THEIR
    // lines among the candidates (zh_knn_graph_refine_rev).  in_k + rev_k <= ZH_REFINE_MAX_IN_K; rev_k = 0 is knn_graph_refine bit for bit.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_refine_rev(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                               std::size_t in_k, std::size_t rev_k, std::size_t k, const Met &metric,
                                                                               std::uint64_t first_row, std::uint64_t n) const {
        const std::uint64_t stored = zh_index_stored_rows(h_.get());
        if (in_counts.size() != stored || in_ids.size() != stored * in_k)
            throw std::invalid_argument("knn_graph_refine_rev: the graph must cover every stored row");
        std::vector<Id> ids(n * k + 1);
        std::vector<DistanceUnit> keys(n * k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_knn_graph_refine_rev(h_.get(), in_ids.data(), in_counts.data(), in_k, rev_k, first_row, n, k, Met::metric, metric.mode(), ids.data(),
                                      keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    void knn_graph_refine_rev_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::size_t in_k, std::size_t rev_k, std::uint64_t first_row,
                                     std::uint64_t n, std::size_t k, const Met &metric, Id *d_out_ids, DistanceUnit *d_out_keys,
                                     std::uint32_t *d_out_counts, void *stream = nullptr) const {
        check(zh_knn_graph_refine_rev_device(h_.get(), d_in_ids, d_in_counts, in_k, rev_k, first_row, n, k, Met::metric, metric.mode(), d_out_ids,
                                             d_out_keys, d_out_counts, stream));
    }
    zh_knn_refine_rev_info knn_refine_rev_info() const {
        zh_knn_refine_rev_info info{};
        check(zh_knn_graph_refine_rev_info(h_.get(), &info));
        return info;
    }
    // The occlusion rule of the graph indexes over a graph of ALL stored rows (zh_knn_graph_prune; the graph as knn_graph_refine_rev takes it): element
    // i = the candidates of stored row first_row + i -- its line and up to rev_k sampled reverse neighbours, the row itself excluded -- in (key, id)
    // order, each kept unless one kept before it is closer to it than the row is (its key against that kept row strictly below its key against the
    // row), at most `degree` of them; fill: a line that came short takes the first dropped candidates.  degree and in_k + rev_k <= ZH_REFINE_MAX_IN_K.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_prune(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                          std::size_t in_k, std::size_t rev_k, std::size_t degree, bool fill, const Met &metric,
                                                                          std::uint64_t first_row, std::uint64_t n) const {
        const std::uint64_t stored = zh_index_stored_rows(h_.get());
        if (in_counts.size() != stored || in_ids.size() != stored * in_k) throw std::invalid_argument("knn_graph_prune: the graph must cover every stored row");
        std::vector<Id> ids(n * degree + 1);
        std::vector<DistanceUnit> keys(n * degree + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_knn_graph_prune(h_.get(), in_ids.data(), in_counts.data(), in_k, rev_k, first_row, n, degree, fill ? 1 : 0, Met::metric, metric.mode(),
                                 ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(n);
        for (std::uint64_t i = 0; i < n; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * degree + j], keys[i * degree + j]);
        return out;
    }
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_prune(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                          std::size_t in_k, std::size_t rev_k, std::size_t degree, bool fill,
                                                                          const Met &metric) const {
        return knn_graph_prune(in_ids, in_counts, in_k, rev_k, degree, fill, metric, 0, zh_index_stored_rows(h_.get()));
    }
    template <class Met>
    void knn_graph_prune_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::size_t in_k, std::size_t rev_k, std::uint64_t first_row,
                                std::uint64_t n, std::size_t degree, bool fill, const Met &metric, Id *d_out_ids, DistanceUnit *d_out_keys,
                                std::uint32_t *d_out_counts, void *stream = nullptr) const {
        check(zh_knn_graph_prune_device(h_.get(), d_in_ids, d_in_counts, in_k, rev_k, first_row, n, degree, fill ? 1 : 0, Met::metric, metric.mode(),
                                        d_out_ids, d_out_keys, d_out_counts, stream));
    }
    zh_knn_prune_info knn_prune_info() const {
        zh_knn_prune_info info{};
        check(zh_knn_graph_prune_info(h_.get(), &info));
        return info;
    }
    // NN-descent on the device (zh_knn_graph_descent): up to `rounds` rounds of knn_graph_refine_rev over the whole table in one call that keeps the
    // graph on the device and, from the second round on, keys only what a new entry of a line brings up -- the loop's answer bit for bit, early
    // stop at the first round without updates included.  1 <= rounds <= 32, k >= 1, in_k + rev_k and k + rev_k <= ZH_REFINE_MAX_IN_K.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> knn_graph_descent(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts,
                                                                            std::size_t in_k, std::size_t rev_k, std::size_t k, std::size_t rounds,
                                                                            const Met &metric) const {
        const std::uint64_t stored = zh_index_stored_rows(h_.get());
        if (in_counts.size() != stored || in_ids.size() != stored * in_k)
            throw std::invalid_argument("knn_graph_descent: the graph must cover every stored row");
        std::vector<Id> ids(stored * k + 1);
        std::vector<DistanceUnit> keys(stored * k + 1);
        std::vector<std::uint32_t> counts(stored + 1);
        const Id none = 0;
        check(zh_knn_graph_descent(h_.get(), stored ? in_ids.data() : &none, stored ? in_counts.data() : counts.data(), in_k, rev_k, k, rounds, Met::metric,
                                   metric.mode(), ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(stored);
        for (std::uint64_t i = 0; i < stored; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * k + j], keys[i * k + j]);
        return out;
    }
    template <class Met>
    void knn_graph_descent_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::size_t in_k, std::size_t rev_k, std::size_t k, std::size_t rounds,
                                  const Met &metric, Id *d_out_ids, DistanceUnit *d_out_keys, std::uint32_t *d_out_counts, void *stream = nullptr) const {
        check(zh_knn_graph_descent_device(h_.get(), d_in_ids, d_in_counts, in_k, rev_k, k, rounds, Met::metric, metric.mode(), d_out_ids, d_out_keys,
                                          d_out_counts, stream));
    }
    zh_knn_descent_info knn_descent_info() const {
        zh_knn_descent_info info{};
        check(zh_knn_graph_descent_info(h_.get(), &info));
        return info;
    }
    // Graph search (zh_index_set_graph, zh_search_graph_batch): a k-NN graph over the first g_rows stored rows kept on the device (4 g_rows g_k bytes)
    // through append, add, remove, deduplicate, build and set_forest; replaced by a second set_graph, dropped by drop_graph, compact (once rows
    // move) and clear, never saved.  in_ids [g_rows * g_k] / in_counts [g_rows] as knn_graph_refine takes them.
    void set_graph(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts, std::size_t g_k) {
        const std::uint64_t g_rows = in_counts.size();
        if (in_ids.size() != g_rows * g_k) throw std::invalid_argument("set_graph: in_ids holds g_k entries per line of in_counts");
        check(zh_index_set_graph(h_.get(), g_rows ? in_ids.data() : nullptr, g_rows ? in_counts.data() : nullptr, g_rows, g_k));
    }
    void set_graph_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::uint64_t g_rows, std::size_t g_k, void *stream = nullptr) {
        check(zh_index_set_graph_device(h_.get(), d_in_ids, d_in_counts, g_rows, g_k, stream));
    }
    void drop_graph() { check(zh_index_drop_graph(h_.get())); }
    zh_graph_info graph_info() const {
        zh_graph_info info{};
        check(zh_index_graph_info(h_.get(), &info));
        return info;
    }
    // beam search over the attached graph under search_exact_batch's keys: seeds holds n_seed ids per query (invalid, removed and repeated ones are
    // ignored); the beam keeps the `beam` best rows met, an iteration expands its first `width` unexpanded ones, until none is left or max_iters
    // (0: no cap) iterations ran.  1 <= top_k <= beam <= ZH_GRAPH_MAX_BEAM, width * g_k <= 256, n_seed <= ZH_GRAPH_MAX_SEEDS.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_graph_batch(const std::vector<Embedding<N>> &queries, const std::vector<Id> &seeds,
                                                                               std::size_t n_seed, std::size_t top_k, const Met &metric,
                                                                               std::size_t beam = 64, std::size_t width = 1,
                                                                               std::size_t max_iters = 0) const {
        const std::size_t b = queries.size();
        if (seeds.size() != b * n_seed) throw std::invalid_argument("search_graph_batch: seeds holds n_seed ids per query");
        std::vector<Id> ids(b * top_k + 1);
        std::vector<DistanceUnit> keys(b * top_k + 1);
        std::vector<std::uint32_t> counts(b + 1);
        check(zh_search_graph_batch(h_.get(), b ? queries[0].data() : nullptr, b, seeds.data(), n_seed, top_k, beam, width, max_iters, Met::metric,
                                    metric.mode(), ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    // ... with the same strided rows of the attached graph as every query's seeds: id_base + j * g_rows / n_seed
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_graph_batch(const std::vector<Embedding<N>> &queries, std::size_t top_k, const Met &metric,
                                                                               std::size_t beam = 64, std::size_t width = 1, std::size_t max_iters = 0,
                                                                               std::size_t n_seed = 32) const {
        const std::uint64_t g_rows = graph_info().g_rows, base = zh_index_id_base(h_.get());
        std::vector<Id> seeds(queries.size() * n_seed);
        for (std::size_t i = 0; i < seeds.size(); i++) seeds[i] = base + (i % n_seed) * g_rows / n_seed;
        return search_graph_batch(queries, seeds, n_seed, top_k, metric, beam, width, max_iters);
    }
    template <class Met>
    void search_graph_batch_device(const float *d_queries, std::size_t b, const Id *d_seeds, std::size_t n_seed, std::size_t top_k, std::size_t beam,
                                   std::size_t width, std::size_t max_iters, const Met &metric, Id *d_out_ids, DistanceUnit *d_out_keys,
                                   std::uint32_t *d_out_counts, void *stream = nullptr) const {
        check(zh_search_graph_batch_device(h_.get(), d_queries, b, d_seeds, n_seed, top_k, beam, width, max_iters, Met::metric, metric.mode(), d_out_ids,
                                           d_out_keys, d_out_counts, stream));
    }
    zh_graph_search_info search_graph_info() const {
        zh_graph_search_info info{};
        check(zh_search_graph_info(h_.get(), &info));
        return info;
    }
    // Filtered graph search (zh_search_graph_filtered_batch): search_graph_batch's walk -- it goes through every live row -- answered with the first
    // top_k by (key, id) of the rows it keyed that `filter_words` allows (bit r & 31 of word r >> 5 = stored row r; n_bits <= stored_rows(), rows at
    // and past it are not allowed).  With every row allowed it is search_graph_batch's answer.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_graph_filtered_batch(const std::vector<Embedding<N>> &queries, const std::vector<Id> &seeds,
                                                                                        std::size_t n_seed, std::size_t top_k, const Met &metric,
                                                                                        const std::vector<std::uint32_t> &filter_words, std::uint64_t n_bits,
                                                                                        std::size_t beam = 64, std::size_t width = 1,
                                                                                        std::size_t max_iters = 0) const {
        const std::size_t b = queries.size();
        if (seeds.size() != b * n_seed) throw std::invalid_argument("search_graph_filtered_batch: seeds holds n_seed ids per query");
        if (filter_words.size() < (n_bits + 31) / 32) throw std::invalid_argument("search_graph_filtered_batch: filter_words holds n_bits bits");
        std::vector<Id> ids(b * top_k + 1);
        std::vector<DistanceUnit> keys(b * top_k + 1);
        std::vector<std::uint32_t> counts(b + 1);
        check(zh_search_graph_filtered_batch(h_.get(), b ? queries[0].data() : nullptr, b, seeds.data(), n_seed, top_k, beam, width, max_iters, Met::metric,
                                             metric.mode(), n_bits ? filter_words.data() : nullptr, n_bits, ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    template <class Met>
    void search_graph_filtered_batch_device(const float *d_queries, std::size_t b, const Id *d_seeds, std::size_t n_seed, std::size_t top_k, std::size_t beam,
                                            std::size_t width, std::size_t max_iters, const Met &metric, const std::uint32_t *d_filter_words,
                                            std::uint64_t n_bits, Id *d_out_ids, DistanceUnit *d_out_keys, std::uint32_t *d_out_counts,
                                            void *stream = nullptr) const {
        check(zh_search_graph_filtered_batch_device(h_.get(), d_queries, b, d_seeds, n_seed, top_k, beam, width, max_iters, Met::metric, metric.mode(),
                                                    d_filter_words, n_bits, d_out_ids, d_out_keys, d_out_counts, stream));
    }
    zh_graph_filtered_info search_graph_filtered_info() const {
        zh_graph_filtered_info info{};
        check(zh_search_graph_filtered_info(h_.get(), &info));
        return info;
    }
    // Filter-steered graph search (zh_search_graph_steered_batch): a walk that sees the filter.  The beam only ever holds rows `filter_words` allows
    // (search_graph_filtered_batch's bitmap) -- seeds that are not allowed are ignored -- and an iteration's candidates are the allowed entries of the
    // parents' lines and, with hops = 2, those of the lines of the disallowed live rows the parents name, in line order, at most 256 an iteration.
    // With every row allowed it is search_graph_batch's answer.  hops is 1 or 2.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_graph_steered_batch(const std::vector<Embedding<N>> &queries, const std::vector<Id> &seeds,
                                                                                       std::size_t n_seed, std::size_t top_k, const Met &metric,
                                                                                       const std::vector<std::uint32_t> &filter_words, std::uint64_t n_bits,
                                                                                       int hops = 2, std::size_t beam = 64, std::size_t width = 1,
                                                                                       std::size_t max_iters = 0) const {
        const std::size_t b = queries.size();
        if (seeds.size() != b * n_seed) throw std::invalid_argument("search_graph_steered_batch: seeds holds n_seed ids per query");
        if (filter_words.size() < (n_bits + 31) / 32) throw std::invalid_argument("search_graph_steered_batch: filter_words holds n_bits bits");
        std::vector<Id> ids(b * top_k + 1);
        std::vector<DistanceUnit> keys(b * top_k + 1);
        std::vector<std::uint32_t> counts(b + 1);
        check(zh_search_graph_steered_batch(h_.get(), b ? queries[0].data() : nullptr, b, seeds.data(), n_seed, top_k, beam, width, max_iters, Met::metric,
                                            metric.mode(), n_bits ? filter_words.data() : nullptr, n_bits, hops, ids.data(), keys.data(), counts.data()));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint32_t j = 0; j < counts[i]; j++) out[i].emplace_back(ids[i * top_k + j], keys[i * top_k + j]);
        return out;
    }
    template <class Met>
    void search_graph_steered_batch_device(const float *d_queries, std::size_t b, const Id *d_seeds, std::size_t n_seed, std::size_t top_k, std::size_t beam,
                                           std::size_t width, std::size_t max_iters, const Met &metric, const std::uint32_t *d_filter_words,
                                           std::uint64_t n_bits, int hops, Id *d_out_ids, DistanceUnit *d_out_keys, std::uint32_t *d_out_counts,
                                           void *stream = nullptr) const {
        check(zh_search_graph_steered_batch_device(h_.get(), d_queries, b, d_seeds, n_seed, top_k, beam, width, max_iters, Met::metric, metric.mode(),
                                                   d_filter_words, n_bits, hops, d_out_ids, d_out_keys, d_out_counts, stream));
    }
    zh_graph_steered_info search_graph_steered_info() const {
        zh_graph_steered_info info{};
        check(zh_search_graph_steered_info(h_.get(), &info));
        return info;
    }
    // Extending the attached graph (zh_index_extend_graph): lines for the rows stored since the attach -- each found by search_graph_batch's walk over
    // the table before its chunk of `batch` rows, seeds holding n_seed ids per new row -- and the old lines those name re-ranked to name them.  Rows of
    // one chunk never name each other (batch = 1 is the sequential rule).  g_k <= beam, 1 <= batch <= ZH_GRAPH_EXTEND_MAX_BATCH.
    template <class Met>
    zh_graph_extend_info extend_graph(const std::vector<Id> &seeds, std::size_t n_seed, const Met &metric, std::size_t beam = 64, std::size_t width = 1,
                                      std::size_t max_iters = 0, std::size_t batch = ZH_GRAPH_EXTEND_MAX_BATCH) {
        const std::uint64_t n_new = n_seed ? seeds.size() / n_seed : 0;
        if (seeds.size() != n_new * n_seed) throw std::invalid_argument("extend_graph: seeds holds n_seed ids per new row");
        check(zh_index_extend_graph(h_.get(), n_new ? seeds.data() : nullptr, n_new, n_seed, beam, width, max_iters, batch, Met::metric, metric.mode()));
        return extend_graph_info();
    }
    // ... with the same strided rows of the graph before the call as every new row's seeds: id_base + j * g_rows / n_seed
    template <class Met>
    zh_graph_extend_info extend_graph(const Met &metric, std::size_t beam = 64, std::size_t width = 1, std::size_t max_iters = 0, std::size_t n_seed = 32,
                                      std::size_t batch = ZH_GRAPH_EXTEND_MAX_BATCH) {
        const std::uint64_t g_rows = graph_info().g_rows, stored = zh_index_stored_rows(h_.get()), base = zh_index_id_base(h_.get());
        std::vector<Id> seeds((stored > g_rows ? stored - g_rows : 0) * n_seed);
        for (std::size_t i = 0; i < seeds.size(); i++) seeds[i] = base + (i % n_seed) * g_rows / n_seed;
        return extend_graph(seeds, n_seed, metric, beam, width, max_iters, batch);
    }
    template <class Met>
    void extend_graph_device(const Id *d_seeds, std::uint64_t n_new, std::size_t n_seed, std::size_t beam, std::size_t width, std::size_t max_iters,
                             std::size_t batch, const Met &metric, void *stream = nullptr) {
        check(zh_index_extend_graph_device(h_.get(), d_seeds, n_new, n_seed, beam, width, max_iters, batch, Met::metric, metric.mode(), stream));
    }
    zh_graph_extend_info extend_graph_info() const {
        zh_graph_extend_info info{};
        check(zh_index_extend_graph_info(h_.get(), &info));
        return info;
    }
    // The attached table read back (zh_index_get_graph) as set_graph takes it: ids [n * g_k] with 2^64-1 tails, counts [n]
    std::pair<std::vector<Id>, std::vector<std::uint32_t>> get_graph(std::uint64_t first_row, std::uint64_t n) const {
        const std::size_t g_k = graph_info().g_k;
        std::vector<Id> ids(n * g_k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        check(zh_index_get_graph(h_.get(), first_row, n, ids.data(), counts.data()));
        ids.resize(n * g_k);
        counts.resize(n);
        return {std::move(ids), std::move(counts)};
    }
    void get_graph_device(std::uint64_t first_row, std::uint64_t n, Id *d_out_ids, std::uint32_t *d_out_counts, void *stream = nullptr) const {
        check(zh_index_get_graph_device(h_.get(), first_row, n, d_out_ids, d_out_counts, stream));
    }
    // The capped reverse graph on its own (zh_knn_graph_reverse): element i = up to rev_k of the live rows that name stored row first_row + i and
    // that its own line does not name, in (hash, row) order; degree[i] = its uncapped in-degree.  No metric, no keys, no forest.
    struct ReverseGraph {
        std::vector<std::vector<Id>> lines;
        std::vector<std::uint32_t> degree;
    };
    ReverseGraph knn_graph_reverse(const std::vector<Id> &in_ids, const std::vector<std::uint32_t> &in_counts, std::size_t in_k, std::size_t rev_k,
                                   std::uint64_t first_row, std::uint64_t n) const {
        const std::uint64_t stored = zh_index_stored_rows(h_.get());
        if (in_counts.size() != stored || in_ids.size() != stored * in_k) throw std::invalid_argument("knn_graph_reverse: the graph must cover every stored row");
        std::vector<Id> ids(n * rev_k + 1);
        std::vector<std::uint32_t> counts(n + 1);
        ReverseGraph out{std::vector<std::vector<Id>>(n), std::vector<std::uint32_t>(n + 1)};
        check(zh_knn_graph_reverse(h_.get(), in_ids.data(), in_counts.data(), in_k, rev_k, first_row, n, ids.data(), counts.data(), out.degree.data()));
        out.degree.resize(n);
        for (std::uint64_t i = 0; i < n; i++) out.lines[i].assign(ids.begin() + i * rev_k, ids.begin() + i * rev_k + counts[i]);
        return out;
    }
    void knn_graph_reverse_device(const Id *d_in_ids, const std::uint32_t *d_in_counts, std::size_t in_k, std::size_t rev_k, std::uint64_t first_row,
                                  std::uint64_t n, Id *d_out_ids, std::uint32_t *d_out_counts, std::uint32_t *d_out_degree, void *stream = nullptr) const {
        check(zh_knn_graph_reverse_device(h_.get(), d_in_ids, d_in_counts, in_k, rev_k, first_row, n, d_out_ids, d_out_counts, d_out_degree, stream));
    }
    zh_knn_reverse_info knn_reverse_info() const {
        zh_knn_reverse_info info{};
        check(zh_knn_graph_reverse_info(h_.get(), &info));
        return info;
    }
    // the forest self-join (zh_self_join_forest): self_join's pairs among the rows that share a leaf in at least one tree, each pair once; exact
    // keys on an approximate candidate set.  One call that counts, one that fetches.  Needs a built forest.
    template <class Met>
    std::vector<JoinedPair> self_join_forest(DistanceUnit max_key, const Met &metric) const {
        std::uint64_t total = 0;
        const int rc = zh_self_join_forest(h_.get(), max_key, Met::metric, metric.mode(), 0, nullptr, nullptr, nullptr, &total);
        if (rc != ZH_ELIMIT) check(rc);
        std::vector<Id> a(total + 1), b(total + 1);
        std::vector<DistanceUnit> keys(total + 1);
        if (total) check(zh_self_join_forest(h_.get(), max_key, Met::metric, metric.mode(), total, a.data(), b.data(), keys.data(), &total));
        std::vector<JoinedPair> out(total);
        for (std::uint64_t i = 0; i < total; i++) out[i] = JoinedPair{a[i], b[i], keys[i]};
        return out;
    }
    zh_join_forest_info join_forest_info() const {
        zh_join_forest_info info{};
        check(zh_self_join_forest_info(h_.get(), &info));
        return info;
    }
    // the forest range search (zh_search_range_forest_batch): search_range_batch's hits among the members of the leaves the walk visits for each
    // query with n = probe (1: the leaf the query hashes to in each tree); exact keys on an approximate candidate set, each hit once.  One call that
    // counts, one that fetches.  Needs a built forest.
    template <class Met>
    std::vector<std::vector<std::pair<Id, DistanceUnit>>> search_range_forest_batch(const std::vector<Embedding<N>> &queries,
                                                                                      const std::vector<DistanceUnit> &max_keys, const Met &metric,
                                                                                      std::uint32_t probe = 1) const {
        const std::size_t b = queries.size();
        if (max_keys.size() != b) throw std::invalid_argument("search_range_forest_batch: one threshold key per query");
        std::vector<std::uint64_t> offsets(b + 1);
        std::uint64_t total = 0;
        const int rc = zh_search_range_forest_batch(h_.get(), b ? queries[0].data() : nullptr, b, max_keys.data(), probe, Met::metric, metric.mode(), 0,
                                                    offsets.data(), nullptr, nullptr, &total);
        if (rc != ZH_ELIMIT) check(rc);
        std::vector<Id> ids(total + 1);
        std::vector<DistanceUnit> keys(total + 1);
        if (total)
            check(zh_search_range_forest_batch(h_.get(), queries[0].data(), b, max_keys.data(), probe, Met::metric, metric.mode(), total, offsets.data(),
                                               ids.data(), keys.data(), &total));
        std::vector<std::vector<std::pair<Id, DistanceUnit>>> out(b);
        for (std::size_t i = 0; i < b; i++)
            for (std::uint64_t j = offsets[i]; j < offsets[i + 1]; j++) out[i].emplace_back(ids[j], keys[j]);
        return out;
    }
    zh_range_forest_info range_forest_info() const {
        zh_range_forest_info info{};
        check(zh_search_range_forest_info(h_.get(), &info));
        return info;
    }
    zh_index *handle() const { return h_.get(); }

  private:
    struct Adopt {};
    LSHIndex(Adopt, zh_index *h) { h_.reset(h, zh_index_destroy); }
    std::shared_ptr<zh_index> h_;
};

// ---- src/database/core.rs (the two calls on the hot path; documents live in memory) -----------------------
template <std::size_t N, class Met>
class Database {
  public:
    explicit Database(const LSHIndexOptions<N> &index_options = {}, Met metric = Met{}) : index(index_options), metric_(metric) {}
    LSHIndex<N> index;  // pub field (core.rs:62)

    // core.rs:245-254
    void insert_records(const std::vector<Embedding<N>> &embeddings, const std::vector<std::string> &documents) {
        auto ids = index.add(embeddings);
        for (std::size_t i = 0; i < ids.size() && i < documents.size(); i++) documents_[ids[i]] = documents[i];
    }
    // core.rs:205-214 / 216-225 / 194-198
    void remove(const std::vector<Id> &embedding_ids) {
        for (Id i : index.remove(embedding_ids)) documents_.erase(i);
    }
    void deduplicate() {
        for (Id i : index.deduplicate()) documents_.erase(i);
    }
    // (new) compact the index and re-key the documents with the old -> new id map.  Rows move, so the database is left WITHOUT a graph
    // (build_graph again before query_vectors_graph) -- unless nothing was removed and nothing moved.
    void compact() {
        const Id base = zh_index_id_base(index.handle());
        const std::vector<Id> new_ids = index.compact();
        std::map<Id, std::string> docs;
        for (auto &kv : documents_)
            if (kv.first >= base && kv.first - base < new_ids.size() && new_ids[kv.first - base] != ~Id(0))
                docs[new_ids[kv.first - base]] = std::move(kv.second);
        documents_.swap(docs);
    }
    void clear_database() {
        index.clear();
        documents_.clear();
    }
    // core.rs:290-313: query index -> {id -> document}; order and distances are dropped (core.rs:304-305).
    // core.rs:303's unwrap_or_default turns a PER-QUERY search failure into an empty entry; here a batch is one call that
    // has no per-query failure mode (over-long batches are split inside zh_search_batch), so a library error -- out of
    // memory, no device, top_k > ZH_MAX_TOPK -- is thrown like in the Python mirror, never reported as "no neighbours"
    std::map<std::size_t, std::map<Id, std::string>> query_vectors(const std::vector<Embedding<N>> &vectors,
                                                                   std::size_t number_of_results) const {
        std::map<std::size_t, std::map<Id, std::string>> results;
        if (index.no_vectors()) return results;  // core.rs:295-297
        const auto nb = index.search_batch(vectors, number_of_results, metric_);
        for (std::size_t i = 0; i < nb.size(); i++) {
            auto &m = results[i];
            for (auto &p : nb[i]) {
                auto it = documents_.find(p.first);
                m[p.first] = it == documents_.end() ? std::string() : it->second;
            }
        }
        return results;
    }

    // (new) make the graph query_vectors_graph walks and attach it: the forest graph, NN-descent, LSHIndex::set_graph.  Needs trees.
    zh_graph_info build_graph(std::size_t k = 32, std::size_t rounds = 8, std::size_t reverse = 0) {
        const std::uint64_t stored = zh_index_stored_rows(index.handle());
        if (!stored) return index.graph_info();
        std::vector<Id> fids(stored * k), fkeys(stored * k), ids(stored * k), keys(stored * k);
        std::vector<std::uint32_t> fcounts(stored), counts(stored);
        auto ok = [](int rc) { if (rc != ZH_OK) throw std::runtime_error(zh_last_error()); };
        ok(zh_knn_graph_forest(index.handle(), 0, stored, k, Met::metric, metric_.mode(), fids.data(), fkeys.data(), fcounts.data()));
        ok(zh_knn_graph_descent(index.handle(), fids.data(), fcounts.data(), k, reverse, k, rounds, Met::metric, metric_.mode(), ids.data(), keys.data(),
                                counts.data()));
        index.set_graph(ids, counts, k);
        return index.graph_info();
    }
    // (new) query_vectors answered by LSHIndex::search_graph_batch over the attached graph, strided seeds
    std::map<std::size_t, std::map<Id, std::string>> query_vectors_graph(const std::vector<Embedding<N>> &vectors, std::size_t number_of_results,
                                                                         std::size_t beam = 64, std::size_t width = 1, std::size_t max_iters = 0,
                                                                         std::size_t n_seed = 32) const {
        std::map<std::size_t, std::map<Id, std::string>> results;
        if (index.no_vectors()) return results;
        const auto nb = index.search_graph_batch(vectors, number_of_results, metric_, beam < number_of_results ? number_of_results : beam, width, max_iters,
                                                 n_seed);
        for (std::size_t i = 0; i < nb.size(); i++) {
            auto &m = results[i];
            for (auto &p : nb[i]) {
                auto it = documents_.find(p.first);
                m[p.first] = it == documents_.end() ? std::string() : it->second;
            }
        }
        return results;
    }

    // (new) every record whose key is <= max_key for each query (LSHIndex::search_range_batch): query index -> its records, nearest first
    std::map<std::size_t, std::vector<std::pair<Id, std::string>>> query_vectors_within(const std::vector<Embedding<N>> &vectors,
                                                                                        DistanceUnit max_key) const {
        std::map<std::size_t, std::vector<std::pair<Id, std::string>>> results;
        if (index.no_vectors()) return results;
        const auto hits = index.search_range_batch(vectors, std::vector<DistanceUnit>(vectors.size(), max_key), metric_);
        for (std::size_t i = 0; i < hits.size(); i++) {
            auto &v = results[i];
            for (auto &p : hits[i]) {
                auto it = documents_.find(p.first);
                v.emplace_back(p.first, it == documents_.end() ? std::string() : it->second);
            }
        }
        return results;
    }

  private:
    Met metric_;
    std::map<Id, std::string> documents_;
};

}  // namespace zebra

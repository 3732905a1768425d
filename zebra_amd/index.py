"""Host-side mirror of the reference's metric / index / database interface for the hot path.

Names, argument meaning and error behaviour follow the reference (file:line in each docstring);
all arithmetic happens in libzebra_hip.so on the GPU."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a, d=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if d is not None and (a.ndim != 2 or a.shape[1] != d):
        raise ValueError(f"expected an (n, {d}) float32 array, got {a.shape}")
    return a


def _with_capacity(cap, n_arrays, call):
    """the range searches' and the joins' host calls: call(cap, arrays, total) -> rc with `n_arrays` u64 output arrays of a guessed capacity; when
    the hits exceed it (ZH_ELIMIT), ONE more call with the exact total the first one reported -> the arrays, cut to the total"""
    total = C.c_uint64(0)
    for attempt in range(2):
        out = [np.empty(max(cap, 1), np.uint64) for _ in range(n_arrays)]
        rc = call(cap, out, total)
        if rc == _ffi.ZH_ELIMIT and attempt == 0 and total.value > cap:
            cap = int(total.value)
            continue
        check(rc)
        break
    return tuple(a[:int(total.value)] for a in out)


def _count(call):
    """the same calls with capacity 0 (nothing is ordered or written): call(total) -> rc, and ZH_ELIMIT is the ordinary answer -> the total"""
    total = C.c_uint64(0)
    rc = call(total)
    if rc != _ffi.ZH_ELIMIT:
        check(rc)
    return int(total.value)


# ---------------------------------------------------------------------------- src/distance.rs
class _Metric:
    """space::Metric<Embedding<N>> with Unit = u64 (src/distance.rs:19-21)."""
    metric = None
    mode = _ffi.COSINE_PARITY

    def __init__(self, device=-1):
        self.device = device

    def distance(self, a, b):
        """Metric::distance(a, b) -> DistanceUnit: the f64 bit pattern as u64."""
        a, b = _f32(a).ravel(), _f32(b).ravel()
        if a.size != b.size:
            raise ValueError("vectors differ in length")
        out = C.c_uint64()
        check(lib().zh_distance_pair(self.metric, self.mode, _p(a), _p(b), a.size, C.byref(out), self.device))
        return int(out.value)

    def distance_batch(self, rows, query):
        rows, query = _f32(rows), _f32(query).ravel()
        out = np.empty(rows.shape[0], np.uint64)
        check(lib().zh_distance_batch(self.metric, self.mode, _p(rows), _p(query), rows.shape[0], rows.shape[1],
                                      _p(out), self.device))
        return out


class CosineDistance(_Metric):
    """src/distance.rs:15-32.  `parity=True` (default) keeps the reference's literal key
    bits(1.0 - simsimd_cosine) = bits of the SIMILARITY; `parity=False` keys on the distance."""
    metric = _ffi.COSINE

    def __init__(self, parity=True, device=-1):
        super().__init__(device)
        self.mode = _ffi.COSINE_PARITY if parity else _ffi.COSINE_CORRECTED


class L2SquaredDistance(_Metric):
    """src/distance.rs:34-49"""
    metric = _ffi.L2SQ


class L2Distance(_Metric):
    """src/distance.rs:99-114"""
    metric = _ffi.L2


class ChebyshevDistance(_Metric):
    """src/distance.rs:51-61"""
    metric = _ffi.CHEBYSHEV


class CanberraDistance(_Metric):
    """src/distance.rs:63-73"""
    metric = _ffi.CANBERRA


class BrayCurtisDistance(_Metric):
    """src/distance.rs:75-85"""
    metric = _ffi.BRAY_CURTIS


class ManhattanDistance(_Metric):
    """src/distance.rs:87-97"""
    metric = _ffi.MANHATTAN


class L3Distance(_Metric):
    """src/distance.rs:116-126"""
    metric = _ffi.L3


class L4Distance(_Metric):
    """src/distance.rs:128-138"""
    metric = _ffi.L4


class HammingDistance(_Metric):
    """src/distance.rs:140-158: bitwise Hamming distance of the low bytes of the f32 bit patterns"""
    metric = _ffi.HAMMING


class MinkowskiDistance(_Metric):
    """src/distance.rs:160-174; `power` is the struct's i32 field (#[derive(Default)]: 0, what `Met::default()` of
    core.rs:115,146 constructs; any i32 is legal)"""
    metric = _ffi.MINKOWSKI

    def __init__(self, power=0, device=-1):
        super().__init__(device)
        self.power = self.mode = int(power)


class PNormDistance(_Metric):
    """src/distance.rs:176-190; default power 0 as the reference's derived Default"""
    metric = _ffi.PNORM

    def __init__(self, power=0, device=-1):
        super().__init__(device)
        self.power = self.mode = int(power)


_F64_KEYED = (_ffi.COSINE, _ffi.L2SQ, _ffi.L2)  # key = the f64 bit pattern (key_cosine / key_l2); HAMMING: the integer count; the rest: f32 bits widened


def radius_key(metric, radius):
    """The largest key that means "distance <= radius" under `metric` (a metric object or a ZH_* metric number), for the range searches'
    max_keys: the f64 bit pattern of the radius for cosine, L2 squared and L2, the bits of the largest f32 at or below it for the metrics whose
    key is an f32 widened to 64 bits, floor(radius) for Hamming's integer count.  `radius` may be a scalar or one value per query (-> a
    uint64 array); NaN or a negative radius raises ValueError.  The radius is compared with the VALUE THE KEY HOLDS: for the parity cosine key
    (CosineDistance(parity=True)) that value is the similarity 1 - distance and keys compare as unsigned bit patterns, so the hits of a
    non-negative radius r are the rows with 0 <= similarity <= r."""
    m = getattr(metric, "metric", metric)
    r = np.asarray(radius, dtype=np.float64) + 0.0  # (-0.0 -> +0.0)
    if np.isnan(r).any() or (r < 0).any():
        raise ValueError("a radius must be a non-negative number")
    if m in _F64_KEYED:
        out = r.view(np.uint64) if r.ndim else np.float64(r).reshape(1).view(np.uint64)[0]
    elif m == _ffi.HAMMING:
        out = np.floor(np.minimum(r, 1.8e19)).astype(np.uint64)
    else:
        with np.errstate(over="ignore"):
            f = r.astype(np.float32)
        f = np.where(f.astype(np.float64) > r, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)
        out = f.reshape(-1).view(np.uint32).astype(np.uint64).reshape(f.shape)
    return np.ascontiguousarray(out) if r.ndim else np.uint64(out)


def snapshot_info(path, verify=False):
    """zh_snapshot_inspect (host code only, no GPU needed): the header of a snapshot file after every test a load applies to the header block,
    the section table and the padding; verify=True recomputes every section's checksum on the host as well."""
    info = _ffi.SnapshotInfo()
    check(lib().zh_snapshot_inspect(os.fsencode(path), 1 if verify else 0, C.byref(info)))
    return info.as_dict()


# ------------------------------------------------------------------- src/database/index/lsh.rs
@dataclass
class LSHIndexOptions:
    """lsh.rs:122-139; defaults max_node_size = 5, num_trees = 15."""
    max_node_size: int = 5
    num_trees: int = 15


class LSHIndex:
    """LSHIndex<N> (lsh.rs:144-565) for the hot path: new / add / search / is_empty / no_vectors /
    no_trees / clear, plus search_batch (the loop of core.rs:299-303 as one call)."""

    def __init__(self, dim, options=None, seed=0x5EB2A003, device=-1, id_base=0, reserve_rows=0):
        options = options or LSHIndexOptions()
        o = _ffi.Options()
        lib().zh_options_default(C.byref(o))
        o.dim, o.max_node_size, o.num_trees = dim, options.max_node_size, options.num_trees
        o.seed, o.device, o.id_base, o.reserve_rows = seed, device, id_base, reserve_rows
        self._h = C.c_void_p()
        check(lib().zh_index_create(C.byref(o), C.byref(self._h)))
        self.dim, self.options, self.id_base = dim, options, id_base

    def close(self):
        if getattr(self, "_h", None):
            # contexts (and shard groups) hold a pointer to the index: they go first, whatever order the garbage collector would pick
            for c in list(getattr(self, "_children", ())):
                c.close()
            lib().zh_index_destroy(self._h)
            self._h = None

    __del__ = close

    def _adopt(self, child):
        import weakref
        if not hasattr(self, "_children"):
            self._children = weakref.WeakSet()
        self._children.add(child)

    # lsh.rs:389-409
    def no_vectors(self):
        return lib().zh_index_count(self._h) == 0

    def no_trees(self):
        return lib().zh_index_num_trees(self._h) == 0

    def is_empty(self):
        return self.no_vectors() or self.no_trees()

    def __len__(self):
        return int(lib().zh_index_count(self._h))

    def stored_rows(self):
        """rows the table holds, live + removed (zh_index_stored_rows); equals len() after compact()"""
        return int(lib().zh_index_stored_rows(self._h))

    def add(self, embeddings):
        """lsh.rs:440-466: returns the ids of the added vectors (dense row ids, not Uuids)."""
        e = _f32(embeddings, self.dim)
        ids = np.empty(e.shape[0], np.uint64)
        check(lib().zh_index_add(self._h, _p(e), e.shape[0], _p(ids)))
        return ids

    def append(self, embeddings):
        e = _f32(embeddings, self.dim)
        ids = np.empty(e.shape[0], np.uint64)
        check(lib().zh_index_append(self._h, _p(e), e.shape[0], _p(ids)))
        return ids

    def append_synthetic(self, n, seed=0x5EB2A001, first_row=0, kind=0):
        check(lib().zh_index_append_synthetic(self._h, n, seed, first_row, kind))

    def build(self):
        check(lib().zh_index_build(self._h))

    def clear(self):
        check(lib().zh_index_clear(self._h))

    def remove(self, embedding_ids):
        """lsh.rs:473-503 (as intended: the ids leave every tree) -> the ids that were present"""
        ids = np.ascontiguousarray(embedding_ids, np.uint64)
        found = np.zeros(ids.size, np.uint8)
        n = C.c_size_t()
        check(lib().zh_index_remove(self._h, _p(ids), ids.size, _p(found), C.byref(n)))
        return ids[found.astype(bool)]

    def deduplicate(self):
        """lsh.rs:270-288 -> ids removed because an earlier vector has the same bits"""
        out = np.zeros(max(len(self), 1), np.uint64)
        n = C.c_size_t()
        check(lib().zh_index_deduplicate(self._h, _p(out), out.size, C.byref(n)))
        return out[:n.value]

    def compact(self):
        """zh_index_compact: the live rows move down over the removed ones on the device, in their order; the forest's leaf ids follow.
        -> (new_ids [rows_before] u64: id_base + new row of every OLD local row, 2^64-1 for a removed one; info dict of zh_compact_info).
        Every later call answers as the uncompacted index would, under that map.  With nothing removed: the identity, nothing released."""
        n = self.stored_rows()
        new_ids = np.empty(n, np.uint64)
        info = _ffi.CompactInfo()
        check(lib().zh_index_compact(self._h, _p(new_ids), n, C.byref(info)))
        return new_ids, info.as_dict()

    def save(self, path):
        """zh_index_save: the index as ONE snapshot file at `path` (written beside it first, then renamed over it) -> dict of zh_snapshot_info.
        Rows (removed ones included), removals, the forest and the planes' sample rows are saved; derived copies and tuning state are not."""
        info = _ffi.SnapshotInfo()
        check(lib().zh_index_save(self._h, os.fsencode(path), C.byref(info)))
        return info.as_dict()

    @classmethod
    def load(cls, path, device=-1, reserve_rows=0):
        """zh_index_load: a new index from a snapshot file, indistinguishable from the saved one for every later call (its options come
        from the file).  The dict of zh_snapshot_info is kept as .snapshot."""
        info = _ffi.SnapshotInfo()
        h = C.c_void_p()
        check(lib().zh_index_load(os.fsencode(path), device, reserve_rows, C.byref(h), C.byref(info)))
        self = cls.__new__(cls)
        self._h = h
        self.dim, self.id_base = int(info.dim), int(info.id_base)
        self.options = LSHIndexOptions(int(info.max_node_size), int(info.num_trees_option))
        self.snapshot = info.as_dict()
        return self

    def set_forest(self, arrays):
        a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        keep = [a["plane"].astype(np.int32), a["left"].astype(np.int32), a["right"].astype(np.int32),
                a["roots"].astype(np.uint32), _f32(a["planes"]).reshape(-1, self.dim), _f32(a["consts"]),
                a["leaf_ids"].astype(np.uint32)]
        fv = _ffi.ForestView(keep[0].size, keep[5].size, keep[3].size, keep[6].size, *[_p(x).value for x in keep])
        check(lib().zh_index_set_forest(self._h, C.byref(fv)))

    def get_forest(self):
        s = _ffi.ForestSizes()
        check(lib().zh_index_forest_sizes(self._h, C.byref(s)))
        out = dict(plane=np.empty(s.n_nodes, np.int32), left=np.empty(s.n_nodes, np.int32),
                   right=np.empty(s.n_nodes, np.int32), roots=np.empty(s.n_trees, np.uint32),
                   planes=np.empty((s.n_planes, self.dim), np.float32), consts=np.empty(s.n_planes, np.float32),
                   leaf_ids=np.empty(s.n_leaf_ids, np.uint32))
        check(lib().zh_index_get_forest(self._h, *[_p(out[k]) for k in
                                                  ("plane", "left", "right", "roots", "planes", "consts", "leaf_ids")]))
        return out

    def hash_signs(self, queries, dots=False):
        """point_is_above (lsh.rs:39-43) of every plane for every query -> bool array [b, n_planes]."""
        q = _f32(queries, self.dim)
        s = _ffi.ForestSizes()
        check(lib().zh_index_forest_sizes(self._h, C.byref(s)))
        words = (s.n_planes + 31) // 32
        bits = np.zeros((q.shape[0], max(words, 1)), np.uint32)
        dd = np.zeros((q.shape[0], s.n_planes), np.float32) if dots else None
        check(lib().zh_hash_signs(self._h, _p(q), q.shape[0], _p(bits), _p(dd) if dots else None))
        signs = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :s.n_planes].astype(bool)
        return (signs, dd) if dots else signs

    def search_batch(self, queries, top_k, metric):
        """LSHIndex::search for every query: (ids [b,k] u64, keys [b,k] u64, counts [b] u32);
        entries past counts[i] are 2^64-1."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        ids = np.empty((b, top_k), np.uint64)
        keys = np.empty((b, top_k), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_batch(self._h, _p(q), b, top_k, metric.metric, metric.mode, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search(self, query, top_k, metric):
        """lsh.rs:544-565 -> list of (id, distance key), ascending."""
        ids, keys, counts = self.search_batch(_f32(query).reshape(1, -1), top_k, metric)
        n = int(counts[0])
        return list(zip(ids[0, :n].tolist(), keys[0, :n].tolist()))

    def search_batch_device(self, d_q_ptr, b, top_k, metric, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """Queries and results already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_search_batch_device(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode, d_ids_ptr,
                                           d_keys_ptr, d_counts_ptr, stream))

    def search_exact_batch(self, queries, top_k, metric):
        """EXACT top_k over every live stored row under the same keys as search_batch (no forest needed; removed rows excluded):
        (ids [b,k] u64, keys [b,k] u64, counts [b] u32); entries past counts[i] are 2^64-1.  The ground truth for recall."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        ids = np.empty((b, top_k), np.uint64)
        keys = np.empty((b, top_k), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_exact_batch(self._h, _p(q), b, top_k, metric.metric, metric.mode, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_exact(self, query, top_k, metric):
        """the exact top_k of one query -> list of (id, distance key), ascending"""
        ids, keys, counts = self.search_exact_batch(_f32(query).reshape(1, -1), top_k, metric)
        n = int(counts[0])
        return list(zip(ids[0, :n].tolist(), keys[0, :n].tolist()))

    def search_exact_batch_device(self, d_q_ptr, b, top_k, metric, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """search_exact_batch with queries and results already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_search_exact_batch_device(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode, d_ids_ptr,
                                                 d_keys_ptr, d_counts_ptr, stream))

    def _info(self, struct, entry):
        """what the most recent call of a family on this index did: its zh_*_info export as a dict"""
        info = struct()
        check(entry(self._h, C.byref(info)))
        return info.as_dict()

    def exact_info(self):
        """what the most recent exact search on this index did (zh_search_exact_info): batch, rows_live, path, redone, survivors, launches"""
        return self._info(_ffi.ExactInfo, lib().zh_search_exact_info)

    def filter_bitmap(self, allowed):
        """a filter for the filtered searches from a boolean mask over the stored rows (length up to stored_rows(); rows past it are not
        allowed) or an integer array of ids -> (words u32, n_bits): bit r & 31 of word r >> 5 set = stored row r (id id_base + r) allowed"""
        a = np.asarray(allowed)
        if a.dtype == np.bool_:
            mask = a.reshape(-1)
        else:
            rows = a.reshape(-1).astype(np.uint64) - np.uint64(self.id_base)
            stored = self.stored_rows()
            if rows.size and int(rows.max()) >= stored:
                raise ValueError("an allowed id is outside this index's %d stored rows" % stored)
            mask = np.zeros(stored, np.bool_)
            mask[rows.astype(np.int64)] = True
        words = np.packbits(mask, bitorder="little")
        words = np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)
        return np.ascontiguousarray(words), int(mask.size)

    def search_exact_filtered_batch(self, queries, top_k, metric, allowed):
        """search_exact_batch among the live rows `allowed` names (a boolean mask over the stored rows, or an array of ids): exactly the
        answer of an index that held only those rows.  One filter for the whole batch; no forest needed."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        words, n_bits = self.filter_bitmap(allowed)
        ids = np.empty((b, top_k), np.uint64)
        keys = np.empty((b, top_k), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_exact_filtered_batch(self._h, _p(q), b, top_k, metric.metric, metric.mode, _p(words) if n_bits else None, n_bits,
                                                   _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_exact_filtered(self, query, top_k, metric, allowed):
        """the exact top_k of one query among the allowed rows -> list of (id, distance key), ascending"""
        ids, keys, counts = self.search_exact_filtered_batch(_f32(query).reshape(1, -1), top_k, metric, allowed)
        n = int(counts[0])
        return list(zip(ids[0, :n].tolist(), keys[0, :n].tolist()))

    def search_exact_filtered_batch_device(self, d_q_ptr, b, top_k, metric, d_filter_ptr, n_bits, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """search_exact_filtered_batch with queries, the filter's u32 words (filter_bitmap's layout) and results already in device memory"""
        check(lib().zh_search_exact_filtered_batch_device(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode, d_filter_ptr, n_bits, d_ids_ptr,
                                                          d_keys_ptr, d_counts_ptr, stream))

    def filtered_info(self):
        """what the most recent filtered exact search on this index did (zh_search_filtered_info): batch, rows_live, rows_allowed, path,
        redone, survivors, launches, tiles_skipped"""
        return self._info(_ffi.FilteredInfo, lib().zh_search_filtered_info)

    def _range_keys(self, b, radius, metric, max_keys):
        if (radius is None) == (max_keys is None):
            raise ValueError("give either a radius or max_keys")
        mk = np.asarray(radius_key(metric, radius) if max_keys is None else max_keys, dtype=np.uint64)
        mk = np.ascontiguousarray(np.broadcast_to(mk, (b,)) if mk.ndim == 0 else mk.reshape(-1))
        if mk.size != b:
            raise ValueError("expected one threshold per query (%d), got %d" % (b, mk.size))
        return mk

    def search_range_batch(self, queries, radius=None, metric=None, max_keys=None, capacity=None):
        """EXACT range search: every live stored row whose key is <= the query's threshold, under the same keys as search_exact_batch (no
        forest needed; removed rows excluded).  The threshold is `radius` (a scalar or one per query, turned into keys by radius_key) or
        `max_keys` (u64 keys, one per query; 2^64-1 = every live row).  -> (offsets [b + 1] u64, ids u64, keys u64): the hits of query i are
        ids / keys [offsets[i], offsets[i + 1]), ascending by (key, id).  One call with a guessed capacity; when the hits exceed it, one more
        with the exact total the first call reported."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        mk = self._range_keys(b, radius, metric, max_keys)
        cap = int(capacity) if capacity is not None else max(1024, 64 * b)
        offsets = np.zeros(b + 1, np.uint64)
        return (offsets,) + _with_capacity(cap, 2, lambda cap, o, total: lib().zh_search_range_batch(
            self._h, _p(q), b, _p(mk), metric.metric, metric.mode, cap, _p(offsets), _p(o[0]), _p(o[1]), C.byref(total)))


    def search_range(self, query, radius=None, metric=None, max_keys=None):
        """the hits of one query -> list of (id, distance key), ascending"""
        _, ids, keys = self.search_range_batch(_f32(query).reshape(1, -1), radius, metric, max_keys)
        return list(zip(ids.tolist(), keys.tolist()))

    def range_count_batch(self, queries, radius=None, metric=None, max_keys=None):
        """how many hits search_range_batch would return for every query (a call with capacity 0: nothing is ordered or written) -> [b] u64"""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        mk = self._range_keys(b, radius, metric, max_keys)
        offsets = np.zeros(b + 1, np.uint64)
        _count(lambda total: lib().zh_search_range_batch(
            self._h, _p(q), b, _p(mk), metric.metric, metric.mode, 0, _p(offsets), None, None, C.byref(total)))

        return np.diff(offsets)

    def search_range_batch_device(self, d_q_ptr, b, d_max_keys_ptr, metric, capacity, d_offsets_ptr, d_ids_ptr, d_keys_ptr, d_total_ptr, stream=None):
        """search_range_batch with queries, threshold keys, offsets (b + 1), ids / keys (`capacity` each) and the total (one u64) in device
        memory (raw pointers, e.g. torch .data_ptr()).  Hits beyond the capacity raise ZhError with code ZH_ELIMIT; the offsets and the total
        are exact even then."""
        check(lib().zh_search_range_batch_device(self._h, d_q_ptr, b, d_max_keys_ptr, metric.metric, metric.mode, capacity, d_offsets_ptr, d_ids_ptr,
                                                 d_keys_ptr, d_total_ptr, stream))

    def range_info(self):
        """what the most recent range search on this index did (zh_search_range_info): batch, rows_live, hits, path, redone, candidates, launches"""
        return self._info(_ffi.RangeInfo, lib().zh_search_range_info)

    def search_range_forest_batch(self, queries, radius=None, metric=None, max_keys=None, probe=1, capacity=None):
        """FOREST range search: search_range_batch among the members of the leaves the walk visits for each query with n = `probe` (what
        search_batch(top_k = probe) walks; 1 = the leaf the query hashes to in each tree).  Exact keys, approximate candidates: the answer is
        the subset of search_range_batch's hits that are members of a visited leaf, each once.  Arguments and result as search_range_batch."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        mk = self._range_keys(b, radius, metric, max_keys)
        cap = int(capacity) if capacity is not None else max(1024, 64 * b)
        offsets = np.zeros(b + 1, np.uint64)
        return (offsets,) + _with_capacity(cap, 2, lambda cap, o, total: lib().zh_search_range_forest_batch(
            self._h, _p(q), b, _p(mk), int(probe), metric.metric, metric.mode, cap, _p(offsets), _p(o[0]), _p(o[1]), C.byref(total)))


    def search_range_forest(self, query, radius=None, metric=None, max_keys=None, probe=1):
        """the forest hits of one query -> list of (id, distance key), ascending"""
        _, ids, keys = self.search_range_forest_batch(_f32(query).reshape(1, -1), radius, metric, max_keys, probe)
        return list(zip(ids.tolist(), keys.tolist()))

    def range_forest_count_batch(self, queries, radius=None, metric=None, max_keys=None, probe=1):
        """how many hits search_range_forest_batch would return for every query (a call with capacity 0: nothing is ordered or written) -> [b] u64"""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        mk = self._range_keys(b, radius, metric, max_keys)
        offsets = np.zeros(b + 1, np.uint64)
        _count(lambda total: lib().zh_search_range_forest_batch(
            self._h, _p(q), b, _p(mk), int(probe), metric.metric, metric.mode, 0, _p(offsets), None, None, C.byref(total)))

        return np.diff(offsets)

    def search_range_forest_batch_device(self, d_q_ptr, b, d_max_keys_ptr, probe, metric, capacity, d_offsets_ptr, d_ids_ptr, d_keys_ptr, d_total_ptr,
                                         stream=None):
        """search_range_forest_batch with queries, threshold keys, offsets (b + 1), ids / keys (`capacity` each) and the total (one u64) in
        device memory (raw pointers, e.g. torch .data_ptr()).  Hits beyond the capacity raise ZhError with code ZH_ELIMIT; the offsets and the
        total are exact even then."""
        check(lib().zh_search_range_forest_batch_device(self._h, d_q_ptr, b, d_max_keys_ptr, int(probe), metric.metric, metric.mode, capacity, d_offsets_ptr,
                                                        d_ids_ptr, d_keys_ptr, d_total_ptr, stream))

    def range_forest_info(self):
        """what the most recent forest range search on this index did (zh_search_range_forest_info): batch, rows_live, trees, probe, path,
        redone, visits, leaf_rows, hits, candidates, launches, tiles"""
        return self._info(_ffi.RangeForestInfo, lib().zh_search_range_forest_info)

    def _join_key(self, radius, metric, max_key):
        if metric is None:
            raise ValueError("the self-join needs a metric")
        if (radius is None) == (max_key is None):
            raise ValueError("give either a radius or max_key")
        mk = np.asarray(radius_key(metric, radius) if max_key is None else max_key, dtype=np.uint64)
        if mk.size != 1:
            raise ValueError("the self-join takes one threshold for the whole call, got %d" % mk.size)
        return int(mk.reshape(-1)[0])

    def self_join(self, radius=None, metric=None, max_key=None, capacity=None):
        """EXACT self-join: every pair of distinct live stored rows (a, b), a < b, whose key is <= ONE threshold -- `radius` (turned into a
        key by radius_key) or `max_key` (a u64 key; 2^64-1 = every pair).  The key of a pair is search_range_batch's for stored row b against
        a query equal to row a.  -> (a u64, b u64, keys u64), ascending by (a, key, b).  One call with a guessed capacity; when the pairs
        exceed it, one more with the exact total the first call reported."""
        mk = self._join_key(radius, metric, max_key)
        cap = int(capacity) if capacity is not None else max(1024, 16 * len(self))
        return _with_capacity(cap, 3, lambda cap, o, total: lib().zh_self_join(
            self._h, mk, metric.metric, metric.mode, cap, _p(o[0]), _p(o[1]), _p(o[2]), C.byref(total)))


    def self_join_count(self, radius=None, metric=None, max_key=None):
        """how many pairs self_join would return (a call with capacity 0: nothing is ordered or written)"""
        mk = self._join_key(radius, metric, max_key)
        return _count(lambda total: lib().zh_self_join(
            self._h, mk, metric.metric, metric.mode, 0, None, None, None, C.byref(total)))


    def self_join_device(self, max_key, metric, capacity, d_a_ptr, d_b_ptr, d_keys_ptr, d_total_ptr, stream=None):
        """self_join with a, b, keys (`capacity` each) and the total (one u64) in device memory (raw pointers, e.g. torch .data_ptr()).
        Pairs beyond the capacity raise ZhError with code ZH_ELIMIT; the total is exact even then."""
        check(lib().zh_self_join_device(self._h, int(max_key), metric.metric, metric.mode, capacity, d_a_ptr, d_b_ptr, d_keys_ptr, d_total_ptr, stream))

    def join_info(self):
        """what the most recent self-join on this index did (zh_self_join_info): rows_live, pairs, path, redone, candidates, launches, tiles"""
        return self._info(_ffi.JoinInfo, lib().zh_self_join_info)

    def _cross_other(self, other):
        if not isinstance(other, LSHIndex):
            raise TypeError("the join between two indexes takes another LSHIndex")
        return other._h

    def cross_join(self, other, radius=None, metric=None, max_key=None, capacity=None):
        """EXACT join between two indexes: every pair (live row a of self, live row b of `other`) whose key is <= ONE threshold -- `radius` or
        `max_key`, as self_join (2^64-1 = every pair of the rectangle).  The key of a pair is other.search_range_batch's for STORED row b of
        `other` against a QUERY equal to row a of self; other.cross_join(self) is a different call, with its own keys and order.
        -> (a u64, b u64, keys u64), ascending by (a, key, b); a carries self's id_base, b other's.  One call with a guessed capacity; when the
        pairs exceed it, one more with the exact total the first call reported."""
        mk = self._join_key(radius, metric, max_key)
        h = self._cross_other(other)
        cap = int(capacity) if capacity is not None else max(1024, 16 * len(self))
        return _with_capacity(cap, 3, lambda cap, o, total: lib().zh_cross_join(
            self._h, h, mk, metric.metric, metric.mode, cap, _p(o[0]), _p(o[1]), _p(o[2]), C.byref(total)))


    def cross_join_count(self, other, radius=None, metric=None, max_key=None):
        """how many pairs cross_join would return (a call with capacity 0: nothing is ordered or written)"""
        mk = self._join_key(radius, metric, max_key)
        return _count(lambda total: lib().zh_cross_join(
            self._h, self._cross_other(other), mk, metric.metric, metric.mode, 0, None, None, None, C.byref(total)))


    def cross_join_device(self, other, max_key, metric, capacity, d_a_ptr, d_b_ptr, d_keys_ptr, d_total_ptr, stream=None):
        """cross_join with a, b, keys (`capacity` each) and the total (one u64) in device memory (raw pointers, e.g. torch .data_ptr()).
        Pairs beyond the capacity raise ZhError with code ZH_ELIMIT; the total is exact even then."""
        check(lib().zh_cross_join_device(self._h, self._cross_other(other), int(max_key), metric.metric, metric.mode, capacity, d_a_ptr, d_b_ptr,
                                         d_keys_ptr, d_total_ptr, stream))

    def cross_info(self):
        """what the most recent cross_join with this index on the left did (zh_cross_join_info): rows_live_a, rows_live_b, pairs, path, redone,
        candidates, launches, tiles"""
        return self._info(_ffi.CrossInfo, lib().zh_cross_join_info)

    def cross_knn(self, other, k, metric, first_row=0, n=None):
        """EXACT k-NN join between two indexes over the slab of self's stored rows [first_row, first_row + n) (default: to the last stored row):
        line i holds the k nearest live rows of `other` to stored row first_row + i of self by (key, id) -- other.search_exact_batch's answer for
        that row's f32 values as the query, bit for bit; nothing is excluded.  other.cross_knn(self) is a different call.
        -> (ids [n,k] u64 with other's id_base, keys [n,k] u64, counts [n] u32); counts = min(k, live rows of other), 0 for a removed row of
        self; entries past the count are 2^64-1."""
        h = self._cross_other(other)
        return self._graph(lambda me, *rest: lib().zh_cross_knn(me, h, *rest), k, metric, first_row, n)

    def cross_knn_device(self, other, k, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """cross_knn with the outputs ([n,k] u64 twice, [n] u32) already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_cross_knn_device(self._h, self._cross_other(other), int(first_row), int(n), k, metric.metric, metric.mode, d_ids_ptr,
                                        d_keys_ptr, d_counts_ptr, stream))

    def cross_knn_info(self):
        """what the most recent cross_knn with this index on the left did (zh_cross_knn_info): rows_live_a, rows_live_b, lines, k, path, redone,
        survivors, launches, tiles"""
        return self._info(_ffi.CrossKnnInfo, lib().zh_cross_knn_info)

    def remove_within(self, other, radius, metric):
        """drop what the corpus already has: every live row of self that has a live row of `other` within `radius` is removed from self (the
        distinct a of cross_join's pairs; `other` is left alone) -> the removed ids, ascending"""
        a, _, _ = self.cross_join(other, radius, metric)
        removed = matched_rule(a)
        if removed.size:
            self.remove(removed)
        return removed

    def knn_graph(self, k, metric, first_row=0, n=None):
        """EXACT k-NN graph of the slab of stored rows [first_row, first_row + n) (default: from first_row to the last stored row): line i holds the
        k nearest OTHER live rows of stored row first_row + i by (key, id) -- the key search_exact_batch gives for that row's f32 values as the
        query; only the row itself is excluded, a bit-identical duplicate is a neighbour.  -> (ids [n,k] u64, keys [n,k] u64, counts [n] u32);
        counts = min(k, live rows - 1), 0 for a removed row; entries past the count are 2^64-1."""
        return self._graph(lib().zh_knn_graph, k, metric, first_row, n)

    def _graph(self, entry, k, metric, first_row, n):
        """either graph's host call over the slab [first_row, first_row + n) (n None: to the last stored row)"""
        stored = self.stored_rows()
        n = max(stored - first_row, 0) if n is None else int(n)
        ids = np.empty((n, k), np.uint64)
        keys = np.empty((n, k), np.uint64)
        counts = np.zeros(n, np.uint32)
        check(entry(self._h, int(first_row), n, k, metric.metric, metric.mode, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def knn_graph_device(self, k, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """knn_graph with the outputs ([n,k] u64 twice, [n] u32) already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_knn_graph_device(self._h, int(first_row), int(n), k, metric.metric, metric.mode, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def knn_info(self):
        """what the most recent k-NN graph call on this index did (zh_knn_graph_info): rows_live, lines, k, path, redone, survivors, launches, tiles"""
        return self._info(_ffi.KnnInfo, lib().zh_knn_graph_info)

    def knn_graph_forest(self, k, metric, first_row=0, n=None):
        """FOREST k-NN graph of the slab of stored rows [first_row, first_row + n) (default: from first_row to the last stored row): line i holds the
        first k by (key, id) of the rows that share a leaf with stored row first_row + i in some tree (get_forest()'s leaf_ids), the row itself
        excluded -- knn_graph's keys, ids and layout, exact arithmetic on an approximate candidate set.  -> (ids [n,k] u64, keys [n,k] u64,
        counts [n] u32); counts = min(k, leaf-mates), 0 for a removed row and for a row no tree holds (appended since the last build); entries
        past the count are 2^64-1.  Needs a built forest."""
        return self._graph(lib().zh_knn_graph_forest, k, metric, first_row, n)

    def knn_graph_forest_device(self, k, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """knn_graph_forest with the outputs ([n,k] u64 twice, [n] u32) already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_knn_graph_forest_device(self._h, int(first_row), int(n), k, metric.metric, metric.mode, d_ids_ptr, d_keys_ptr, d_counts_ptr,
                                               stream))

    def knn_forest_info(self):
        """what the most recent forest k-NN graph call on this index did (zh_knn_graph_forest_info): rows_live, lines, k, path, trees, pairs,
        survivors, redone, launches, tiles"""
        return self._info(_ffi.KnnForestInfo, lib().zh_knn_graph_forest_info)

    def _graph_arrays(self, graph, who, cover=True):
        """an input graph -- (ids, counts) or a graph call's 3-tuple -- as contiguous (in_ids u64 [lines, in_k], in_counts u32 [lines]) and the
        number of stored rows; cover: the lines must be the stored rows (otherwise the rows are not asked for: None)"""
        in_ids = np.ascontiguousarray(graph[0], np.uint64)
        in_counts = np.ascontiguousarray(graph[-1], np.uint32)
        shaped = in_ids.ndim == 2 and in_counts.ndim == 1
        if not cover:
            if not shaped:
                raise _ffi.ZhError(_ffi.ZH_EINVAL, "%s: the graph is ids [g_rows, g_k] and counts [g_rows]" % who)
            return in_ids, in_counts, None
        stored = self.stored_rows()
        if not shaped or in_ids.shape[0] != stored or in_counts.shape[0] != stored:
            raise _ffi.ZhError(_ffi.ZH_EINVAL, "%s: the graph must cover the %d stored rows: ids [%d, in_k], counts [%d]" % (who, stored, stored, stored))
        return in_ids, in_counts, stored

    def knn_graph_refine(self, graph, k, metric, first_row=0, n=None, rounds=1, reverse=0):
        """one join round of NN-descent over a graph of ALL stored rows: `graph` is (ids [stored rows, in_k] u64, counts [stored rows] u32) or the
        3-tuple knn_graph / knn_graph_forest return (its keys are not read: every returned key is computed here).  Line i of the answer holds the
        first k by (key, id) of stored row first_row + i's neighbours and their neighbours, the row itself excluded; entries that are out of range,
        removed or repeated in a line are ignored.  rounds > 1 (the whole table only) feeds each round's output to the next and stops early
        once a round changes nothing (knn_refine_info()['updates'] == 0).  -> (ids [n,k] u64, keys [n,k] u64, counts [n] u32), knn_graph's
        layout.  No forest needed.  reverse > 0: every round also ranks up to `reverse` sampled reverse neighbours of each row (the rows that
        name it, knn_graph_reverse) and THEIR lists -- zh_knn_graph_refine_rev, in_k + reverse <= 64; knn_refine_rev_info() then describes the
        call, and its 'updates' is the early stop.  reverse = 0 is today's call and path exactly."""
        in_ids, in_counts, stored = self._graph_arrays(graph, "knn_graph_refine")
        rounds = int(rounds)
        if rounds < 1:
            raise _ffi.ZhError(_ffi.ZH_EINVAL, "knn_graph_refine: rounds must be at least 1")
        n = max(stored - first_row, 0) if n is None else int(n)
        if rounds > 1 and (first_row != 0 or n != stored):
            raise _ffi.ZhError(_ffi.ZH_EINVAL, "knn_graph_refine: rounds > 1 needs the whole table (a round's output is the next round's input)")
        for _ in range(rounds):
            ids = np.empty((n, k), np.uint64)
            keys = np.empty((n, k), np.uint64)
            counts = np.zeros(n, np.uint32)
            if reverse:
                check(lib().zh_knn_graph_refine_rev(self._h, _p(in_ids), _p(in_counts), in_ids.shape[1], int(reverse), int(first_row), n, k, metric.metric,
                                                    metric.mode, _p(ids), _p(keys), _p(counts)))
                info = self.knn_refine_rev_info
            else:
                check(lib().zh_knn_graph_refine(self._h, _p(in_ids), _p(in_counts), in_ids.shape[1], int(first_row), n, k, metric.metric, metric.mode,
                                                _p(ids), _p(keys), _p(counts)))
                info = self.knn_refine_info
            if rounds > 1 and (k == 0 or info()["updates"] == 0):
                break
            in_ids, in_counts = ids, counts
        return ids, keys, counts

    def knn_graph_refine_device(self, d_in_ids_ptr, d_in_counts_ptr, in_k, k, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """one round of knn_graph_refine with the graph ([stored rows, in_k] u64, [stored rows] u32) and the outputs ([n,k] u64 twice, [n] u32)
        already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_knn_graph_refine_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(in_k), int(first_row), int(n), k, metric.metric, metric.mode,
                                               d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def knn_refine_info(self):
        """what the most recent graph refinement call on this index did (zh_knn_graph_refine_info): rows_live, lines, in_k, k, listed, keyed,
        updates, launches"""
        return self._info(_ffi.KnnRefineInfo, lib().zh_knn_graph_refine_info)

    def knn_graph_refine_rev_device(self, d_in_ids_ptr, d_in_counts_ptr, in_k, rev_k, k, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """knn_graph_refine_device with up to rev_k sampled reverse neighbours per row in the candidate set (rev_k = 0: the same answer)"""
        check(lib().zh_knn_graph_refine_rev_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(in_k), int(rev_k), int(first_row), int(n), k, metric.metric,
                                                   metric.mode, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def knn_refine_rev_info(self):
        """what the most recent knn_graph_refine(reverse > 0) / knn_graph_refine_rev_device call did (zh_knn_graph_refine_rev_info):
        knn_refine_info's fields, then rev_k, edges, kept, max_degree"""
        return self._info(_ffi.KnnRefineRevInfo, lib().zh_knn_graph_refine_rev_info)

    def knn_graph_descent(self, graph, k, metric, rounds=8, reverse=0):
        """NN-descent over a graph of ALL stored rows (`graph` as for knn_graph_refine): up to `rounds` rounds of knn_graph_refine(reverse=reverse)
        in ONE call that keeps the graph on the device and, from the second round on, keys only the candidates a NEW entry of a line brings up.
        The answer is bit for bit knn_graph_refine(graph, k, metric, rounds=rounds, reverse=reverse)'s, early stop at the first round without
        updates included; knn_descent_info() describes the call round by round.  Whole table only, 1 <= rounds <= 32, k >= 1,
        in_k + reverse <= 64 and k + reverse <= 64.  -> (ids [stored rows, k] u64, keys [stored rows, k] u64, counts [stored rows] u32)."""
        in_ids, in_counts, stored = self._graph_arrays(graph, "knn_graph_descent")
        k = int(k)
        ids = np.empty((stored, max(k, 0)), np.uint64)
        keys = np.empty((stored, max(k, 0)), np.uint64)
        counts = np.zeros(stored, np.uint32)
        check(lib().zh_knn_graph_descent(self._h, _p(in_ids), _p(in_counts), in_ids.shape[1], int(reverse), k, int(rounds), metric.metric, metric.mode,
                                         _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def knn_graph_descent_device(self, d_in_ids_ptr, d_in_counts_ptr, in_k, rev_k, k, rounds, metric, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream=None):
        """knn_graph_descent with the graph ([stored rows, in_k] u64, [stored rows] u32) and the outputs ([stored rows, k] u64 twice,
        [stored rows] u32) already in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_knn_graph_descent_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(in_k), int(rev_k), int(k), int(rounds), metric.metric, metric.mode,
                                                d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def knn_descent_info(self):
        """what the most recent knn_graph_descent call on this index did (zh_knn_graph_descent_info): rows_live, in_k, rev_k, k, rounds, rounds_run,
        launches, listed, keyed, lines_active (sums over the rounds run), updates (of the last round run), large_lines, and per round run the
        lists keyed_round, updates_round and active_round"""
        return self._info(_ffi.KnnDescentInfo, lib().zh_knn_graph_descent_info)

    def knn_graph_prune(self, graph, degree, metric, reverse=0, fill=False, first_row=0, n=None):
        """the occlusion rule of the graph indexes over a graph of ALL stored rows (`graph` as for knn_graph_refine; zh_knn_graph_prune): the
        candidates of stored row a = first_row + i are the live rows its line names and, with reverse > 0, up to `reverse` sampled reverse
        neighbours (knn_graph_reverse's line), a itself excluded.  In (key, id) order under the key of row a as the query, a candidate is kept
        unless a candidate kept before it is closer to it than a is -- its key against that kept row as the query is strictly below its key
        against a -- until `degree` are kept; fill=True then makes up a short line with the first dropped candidates.  -> (ids [n, degree] u64,
        keys [n, degree] u64, counts [n] u32), knn_graph's layout, each line ordered by (key, id).  degree and in_k + reverse at most 64.  No
        forest needed; knn_prune_info() describes the call."""
        in_ids, in_counts, stored = self._graph_arrays(graph, "knn_graph_prune")
        n = max(stored - first_row, 0) if n is None else int(n)
        degree = int(degree)
        ids = np.empty((n, max(degree, 0)), np.uint64)
        keys = np.empty((n, max(degree, 0)), np.uint64)
        counts = np.zeros(n, np.uint32)
        check(lib().zh_knn_graph_prune(self._h, _p(in_ids), _p(in_counts), in_ids.shape[1], int(reverse), int(first_row), n, degree, int(fill),
                                       metric.metric, metric.mode, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def knn_graph_prune_device(self, d_in_ids_ptr, d_in_counts_ptr, in_k, rev_k, degree, fill, metric, first_row, n, d_ids_ptr, d_keys_ptr, d_counts_ptr,
                               stream=None):
        """knn_graph_prune with the graph ([stored rows, in_k] u64, [stored rows] u32) and the outputs ([n, degree] u64 twice, [n] u32) already
        in device memory (raw pointers, e.g. torch .data_ptr())."""
        check(lib().zh_knn_graph_prune_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(in_k), int(rev_k), int(first_row), int(n), int(degree), int(fill),
                                              metric.metric, metric.mode, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def knn_prune_info(self):
        """what the most recent knn_graph_prune call on this index did (zh_knn_graph_prune_info): rows_live, lines, in_k, rev_k, degree, fill,
        candidates, kept (before filling), occluded, filled, cut (lines that stopped at degree with candidates unexamined), keyed, launches"""
        return self._info(_ffi.KnnPruneInfo, lib().zh_knn_graph_prune_info)

    def prune_graph(self, degree, metric, reverse=0, fill=False):
        """prune the ATTACHED graph in place of itself: get_graph -> knn_graph_prune -> set_graph, a composition of those three calls through the
        host and nothing more.  The graph must cover every stored row (extend_graph first if rows were added).  -> graph_info()"""
        self.set_graph(self.knn_graph_prune(self.get_graph(), degree, metric, reverse=reverse, fill=fill))
        return self.graph_info()

    def set_graph(self, graph, rows=None):
        """attach a k-NN graph for search_graph_batch (zh_index_set_graph): `graph` is (ids [g_rows, g_k] u64, counts [g_rows] u32) or the 3-tuple
        a graph call returns (its keys are not read), over the first g_rows = `rows` stored rows (default: as many as the arrays hold; at most
        stored_rows()), ids in the id space id_base + row.  Entries past a line's count, out of range, removed or repeated in their line are
        ignored.  The index keeps the graph on the device (4 g_rows g_k bytes) through append, add, remove, deduplicate, build and set_forest;
        a second set_graph replaces it; compact() (once it moves rows) and clear() drop it, and a snapshot never holds it."""
        in_ids, in_counts, _ = self._graph_arrays(graph, "set_graph", cover=False)
        g_rows = in_ids.shape[0] if rows is None else int(rows)
        if g_rows < 0 or g_rows > in_ids.shape[0] or g_rows > in_counts.shape[0]:
            raise _ffi.ZhError(_ffi.ZH_EINVAL, "set_graph: rows %d, but the arrays hold %d and %d lines" % (g_rows, in_ids.shape[0], in_counts.shape[0]))
        check(lib().zh_index_set_graph(self._h, _p(in_ids), _p(in_counts), g_rows, in_ids.shape[1]))

    def set_graph_device(self, d_in_ids_ptr, d_in_counts_ptr, g_rows, g_k, stream=None):
        """set_graph with the graph ([g_rows, g_k] u64, [g_rows] u32) already in device memory (raw pointers, e.g. torch .data_ptr())"""
        check(lib().zh_index_set_graph_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(g_rows), int(g_k), stream))

    def drop_graph(self):
        """release the attached graph (zh_index_drop_graph); nothing happens without one"""
        check(lib().zh_index_drop_graph(self._h))

    def graph_info(self):
        """the attached graph (zh_index_graph_info): attached (0 / 1), g_k, g_rows, bytes"""
        return self._info(_ffi.GraphInfo, lib().zh_index_graph_info)

    def _graph_seeds(self, seeds, q, metric, n_seed):
        """the [b, n_seed] u64 seed ids of search_graph_batch"""
        b = q.shape[0]
        if seeds is None:  # the same strided rows of the attached graph for every query
            g_rows, n_seed = self.graph_info()["g_rows"], int(n_seed)
            row = np.array([j * g_rows // n_seed for j in range(n_seed)], np.uint64) + np.uint64(self.id_base)
            return np.ascontiguousarray(np.broadcast_to(row, (b, n_seed)))
        if isinstance(seeds, str):
            if seeds != "lsh":
                raise ValueError("seeds is None, 'lsh' or an array of ids")
            return np.ascontiguousarray(self.search_batch(q, int(n_seed), metric)[0])  # (tails are 2^64-1: ignored as out of range)
        a = np.asarray(seeds).astype(np.uint64, copy=False)
        if a.ndim == 1:
            a = np.broadcast_to(a, (b, a.shape[0]))
        if a.ndim != 2 or a.shape[0] != b:
            raise _ffi.ZhError(_ffi.ZH_EINVAL, "search_graph_batch: seeds is [n_seed] or [%d, n_seed]" % b)
        return np.ascontiguousarray(a)

    def search_graph_batch(self, queries, top_k, metric, beam=64, width=1, max_iters=0, seeds=None, n_seed=32):
        """beam search over the attached graph (set_graph; zh_search_graph_batch) under search_exact_batch's keys: from each query's seeds, the
        beam holds the `beam` best rows met so far; an iteration expands the first `width` unexpanded ones (their lines' live rows are keyed
        and merged in) until none is left or `max_iters` (0: no cap) iterations ran -> (ids [b,k] u64, keys [b,k] u64, counts [b] u32), the
        first top_k of the beam, entries past counts[i] 2^64-1.  seeds: None = the same n_seed strided rows id_base + j * g_rows // n_seed for
        every query; "lsh" = search_batch(queries, n_seed, metric)'s ids (needs trees); an array [b, n_seed] of ids, or [n_seed] for every
        query.  Seeds that are out of range, removed or repeated are ignored; a query without a valid seed has count 0.
        1 <= top_k <= beam <= 256, width * g_k <= 256, 1 <= n_seed <= 64, max_iters <= 65535.  search_graph_info() describes the call."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        sd = self._graph_seeds(seeds, q, metric, n_seed)
        top_k = int(top_k)
        ids = np.empty((b, max(top_k, 0)), np.uint64)
        keys = np.empty((b, max(top_k, 0)), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_graph_batch(self._h, _p(q), b, _p(sd), sd.shape[1], top_k, int(beam), int(width), int(max_iters), metric.metric, metric.mode,
                                          _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_graph(self, query, top_k, metric, **kw):
        """search_graph_batch of one query -> list of (id, distance key), ascending"""
        ids, keys, counts = self.search_graph_batch(_f32(query).reshape(1, -1), top_k, metric, **kw)
        n = int(counts[0])
        return list(zip(ids[0, :n].tolist(), keys[0, :n].tolist()))

    def search_graph_batch_device(self, d_q_ptr, b, d_seeds_ptr, n_seed, top_k, metric, d_ids_ptr, d_keys_ptr, d_counts_ptr, beam=64, width=1, max_iters=0,
                                  stream=None):
        """search_graph_batch with queries ([b, dim] f32), seeds ([b, n_seed] u64) and results already in device memory (raw pointers)"""
        check(lib().zh_search_graph_batch_device(self._h, d_q_ptr, int(b), d_seeds_ptr, int(n_seed), int(top_k), int(beam), int(width), int(max_iters),
                                                 metric.metric, metric.mode, d_ids_ptr, d_keys_ptr, d_counts_ptr, stream))

    def search_graph_info(self):
        """what the most recent search_graph_batch call on this index did (zh_search_graph_info), summed over its queries: queries, seeds (valid
        ones), iterations, expanded, keyed, capped (stopped by max_iters with an unexpanded entry left), launches"""
        return self._info(_ffi.SearchGraphInfo, lib().zh_search_graph_info)

    def _allowed_seeds(self, words, n_bits, b, n_seed):
        """seeds="allowed": n_seed rows strided over the mask's set positions, rows[j * len(rows) // n_seed], the same for every query; a mask
        with fewer set positions than n_seed gives every one of them, padded with repeats (which the kernel ignores)"""
        n_seed = int(n_seed)
        rows = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits])
        if rows.size == 0:
            row = np.full(max(n_seed, 0), 2 ** 64 - 1, np.uint64)  # (out of range: no seed)
        elif rows.size < n_seed:
            row = rows[np.arange(n_seed) % rows.size].astype(np.uint64) + np.uint64(self.id_base)
        else:
            row = rows[[j * rows.size // n_seed for j in range(n_seed)]].astype(np.uint64) + np.uint64(self.id_base)
        return np.ascontiguousarray(np.broadcast_to(row, (b, row.size)))

    def search_graph_filtered_batch(self, queries, top_k, metric, allowed, beam=64, width=1, max_iters=0, seeds=None, n_seed=32):
        """search_graph_batch's walk, answered from the rows `allowed` names (whatever filter_bitmap takes; zh_search_graph_filtered_batch): the
        walk does not see the filter and goes through every live row; the answer is the first top_k by (key, id) of the allowed live rows among
        those that got a key -> (ids [b,k] u64, keys [b,k] u64, counts [b] u32), entries past counts[i] 2^64-1.  With every row allowed it is
        search_graph_batch's answer.  seeds as in search_graph_batch, and "allowed" = n_seed rows strided over the mask's set positions, the same
        for every query.  Limits as search_graph_batch.  search_graph_filtered_info() describes the call."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        words, n_bits = self.filter_bitmap(allowed)
        if isinstance(seeds, str) and seeds == "allowed":
            sd = self._allowed_seeds(words, n_bits, b, n_seed)
        else:
            sd = self._graph_seeds(seeds, q, metric, n_seed)
        top_k = int(top_k)
        ids = np.empty((b, max(top_k, 0)), np.uint64)
        keys = np.empty((b, max(top_k, 0)), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_graph_filtered_batch(self._h, _p(q), b, _p(sd), sd.shape[1], top_k, int(beam), int(width), int(max_iters), metric.metric,
                                                   metric.mode, _p(words) if n_bits else None, n_bits, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_graph_filtered_batch_device(self, d_q_ptr, b, d_seeds_ptr, n_seed, top_k, metric, d_filter_ptr, n_bits, d_ids_ptr, d_keys_ptr, d_counts_ptr,
                                           beam=64, width=1, max_iters=0, stream=None):
        """search_graph_filtered_batch with queries, seeds, the filter's u32 words (filter_bitmap's layout) and results already in device memory"""
        check(lib().zh_search_graph_filtered_batch_device(self._h, d_q_ptr, int(b), d_seeds_ptr, int(n_seed), int(top_k), int(beam), int(width),
                                                          int(max_iters), metric.metric, metric.mode, d_filter_ptr, int(n_bits), d_ids_ptr, d_keys_ptr,
                                                          d_counts_ptr, stream))

    def search_graph_filtered_info(self):
        """what the most recent search_graph_filtered_batch call on this index did (zh_search_graph_filtered_info): search_graph_info's seven
        fields (equal to the unfiltered call's at the same arguments), rows_allowed (allowed and live), offered (allowed rows among the seeds
        and every iteration's candidates, repeats included), returned (the sum of counts)"""
        return self._info(_ffi.SearchGraphFilteredInfo, lib().zh_search_graph_filtered_info)

    def search_graph_steered_batch(self, queries, top_k, metric, allowed, hops=2, beam=64, width=1, max_iters=0, seeds="allowed", n_seed=32):
        """a walk over the attached graph that sees the filter (zh_search_graph_steered_batch): the beam only ever holds rows `allowed` names
        (whatever filter_bitmap takes) that are live.  An iteration expands the first `width` unexpanded beam entries: an allowed live entry of
        a parent's line is a candidate; with hops=2 a disallowed live entry is a bridge, and the allowed live entries of the bridges' lines are
        candidates too, in line order behind the direct ones; at most 256 candidates an iteration, the rest of the bridges' entries dropped.
        -> (ids [b,k] u64, keys [b,k] u64, counts [b] u32), the first top_k of the beam, entries past counts[i] 2^64-1.  With every row allowed
        it is search_graph_batch's answer.  seeds: "allowed" (the default) = n_seed rows strided over the mask's set positions, the same for
        every query; None, "lsh" and arrays as in search_graph_filtered_batch -- but seeds that are NOT ALLOWED are ignored here, like removed,
        repeated and out-of-range ones.  hops is 1 or 2; the other limits as search_graph_batch.  search_graph_steered_info() describes the
        call."""
        q = _f32(queries, self.dim)
        b = q.shape[0]
        words, n_bits = self.filter_bitmap(allowed)
        if isinstance(seeds, str) and seeds == "allowed":
            sd = self._allowed_seeds(words, n_bits, b, n_seed)
        else:
            sd = self._graph_seeds(seeds, q, metric, n_seed)
        top_k = int(top_k)
        ids = np.empty((b, max(top_k, 0)), np.uint64)
        keys = np.empty((b, max(top_k, 0)), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_search_graph_steered_batch(self._h, _p(q), b, _p(sd), sd.shape[1], top_k, int(beam), int(width), int(max_iters), metric.metric,
                                                  metric.mode, _p(words) if n_bits else None, n_bits, int(hops), _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_graph_steered_batch_device(self, d_q_ptr, b, d_seeds_ptr, n_seed, top_k, metric, d_filter_ptr, n_bits, d_ids_ptr, d_keys_ptr, d_counts_ptr,
                                          hops=2, beam=64, width=1, max_iters=0, stream=None):
        """search_graph_steered_batch with queries, seeds, the filter's u32 words (filter_bitmap's layout) and results already in device memory"""
        check(lib().zh_search_graph_steered_batch_device(self._h, d_q_ptr, int(b), d_seeds_ptr, int(n_seed), int(top_k), int(beam), int(width),
                                                         int(max_iters), metric.metric, metric.mode, d_filter_ptr, int(n_bits), int(hops), d_ids_ptr,
                                                         d_keys_ptr, d_counts_ptr, stream))

    def search_graph_steered_info(self):
        """what the most recent search_graph_steered_batch call on this index did (zh_search_graph_steered_info): search_graph_info's seven
        fields under this walk, rows_allowed (allowed and live), direct and via_bridge (candidates a parent's line named / a bridge's line
        named: keyed = seeds + direct + via_bridge), bridges (disallowed live rows hopped over, summed over the iterations), cand_full
        (iterations that filled all 256 candidate slots), returned (the sum of counts)"""
        return self._info(_ffi.SearchGraphSteeredInfo, lib().zh_search_graph_steered_info)

    def extend_graph(self, metric, beam=64, width=1, max_iters=0, seeds=None, n_seed=32, batch=1024):
        """give the rows stored since set_graph lines of their own and let the old lines name them (zh_index_extend_graph): the new rows go in
        chunks of `batch` stored rows; each live row of a chunk is a query of search_graph_batch's walk over the table as it stands before the
        chunk (top_k = g_k, so g_k <= beam), its line the first g_k of the final beam; then every old row that one of those lines names is
        re-ranked over its live entries and the chunk rows that name it, under the key of that old row as the query.  Rows of one chunk never
        name each other (batch=1 is the sequential rule); get_graph, a knn_graph_descent round and set_graph close what is left.  seeds: None =
        the strided rows id_base + j * G // n_seed of the graph before the call for every new row; "lsh" = search_batch of the new rows read
        back (needs trees; a seed naming a row without a line yet is ignored by the rule); an array [new rows, n_seed] of ids, or [n_seed] for
        every row.  1 <= batch <= 1024, the other limits as search_graph_batch.  -> extend_graph_info()"""
        g_rows = self.graph_info()["g_rows"]
        n_new = max(self.stored_rows() - g_rows, 0)
        n_seed = int(n_seed)
        if seeds is None:
            row = np.array([j * g_rows // n_seed for j in range(n_seed)] if n_seed > 0 else [], np.uint64) + np.uint64(self.id_base)
            sd = np.ascontiguousarray(np.broadcast_to(row, (n_new, row.size)))
        elif isinstance(seeds, str):
            if seeds != "lsh":
                raise ValueError("seeds is None, 'lsh' or an array of ids")
            sd = np.empty((n_new, n_seed), np.uint64)
            for r0 in range(0, n_new, 65536):  # (tails are 2^64-1: ignored as out of range)
                m = min(65536, n_new - r0)
                sd[r0:r0 + m] = self.search_batch(self.read_rows(g_rows + r0, m), n_seed, metric)[0]
        else:
            a = np.asarray(seeds).astype(np.uint64, copy=False)
            if a.ndim == 1:
                a = np.broadcast_to(a, (n_new, a.shape[0]))
            if a.ndim != 2 or a.shape[0] != n_new:
                raise _ffi.ZhError(_ffi.ZH_EINVAL, "extend_graph: seeds is [n_seed] or [%d, n_seed]" % n_new)
            sd = np.ascontiguousarray(a)
        check(lib().zh_index_extend_graph(self._h, _p(sd) if n_new else None, n_new, sd.shape[1], int(beam), int(width), int(max_iters), int(batch),
                                          metric.metric, metric.mode))
        return self.extend_graph_info()

    def extend_graph_device(self, d_seeds_ptr, n_new, n_seed, metric, beam=64, width=1, max_iters=0, batch=1024, stream=None):
        """extend_graph with the seeds ([n_new, n_seed] u64, n_new = the rows stored since the attach) already in device memory (raw pointer)"""
        check(lib().zh_index_extend_graph_device(self._h, d_seeds_ptr, int(n_new), int(n_seed), int(beam), int(width), int(max_iters), int(batch),
                                                 metric.metric, metric.mode, stream))

    def extend_graph_info(self):
        """what the most recent extend_graph call on this index did (zh_index_extend_graph_info): rows_added (live new rows), rows_removed (new
        rows with an empty line), chunks, the walks' seeds, iterations, expanded, keyed and capped, reverse_rows (old rows re-ranked, summed over
        the chunks), reverse_offered (new rows offered to them), reverse_kept (new rows that ended inside a re-ranked line), launches"""
        return self._info(_ffi.GraphExtendInfo, lib().zh_index_extend_graph_info)

    def get_graph(self, first_row=0, n=None):
        """the attached graph's lines [first_row, first_row + n) (default: to its last line) as set_graph takes them (zh_index_get_graph): the kept
        entries of each line in table order as ids, 2^64-1 behind them -> (ids [n, g_k] u64, counts [n] u32).  A row removed since the attach
        is still listed."""
        g = self.graph_info()
        n = max(g["g_rows"] - int(first_row), 0) if n is None else int(n)
        ids = np.empty((n, g["g_k"]), np.uint64)
        counts = np.zeros(n, np.uint32)
        check(lib().zh_index_get_graph(self._h, int(first_row), n, _p(ids) if n else None, _p(counts) if n else None))
        return ids, counts

    def get_graph_device(self, first_row, n, d_ids_ptr, d_counts_ptr, stream=None):
        """get_graph with the outputs ([n, g_k] u64, [n] u32) already in device memory (raw pointers)"""
        check(lib().zh_index_get_graph_device(self._h, int(first_row), int(n), d_ids_ptr, d_counts_ptr, stream))

    def knn_graph_reverse(self, graph, rev_k, first_row=0, n=None):
        """the capped reverse graph of a graph of ALL stored rows (`graph` as for knn_graph_refine): line i holds up to rev_k of the live rows that
        name stored row first_row + i and that its own line does not name -- a deterministic pseudo-random sample by a hash of the pair, the same
        whatever the order of entries, the run or the slab -> (ids [n, rev_k] u64 with tails 2^64-1, counts [n] u32, degree [n] u32: the uncapped
        in-degree, the hubness score).  No metric, no keys, no forest."""
        in_ids, in_counts, stored = self._graph_arrays(graph, "knn_graph_reverse")
        n = max(stored - first_row, 0) if n is None else int(n)
        ids = np.empty((n, rev_k), np.uint64)
        counts = np.zeros(n, np.uint32)
        degree = np.zeros(n, np.uint32)
        check(lib().zh_knn_graph_reverse(self._h, _p(in_ids), _p(in_counts), in_ids.shape[1], int(rev_k), int(first_row), n, _p(ids), _p(counts), _p(degree)))
        return ids, counts, degree

    def knn_graph_reverse_device(self, d_in_ids_ptr, d_in_counts_ptr, in_k, rev_k, first_row, n, d_ids_ptr, d_counts_ptr, d_degree_ptr, stream=None):
        """knn_graph_reverse with the graph and the outputs ([n, rev_k] u64, [n] u32 twice) already in device memory (raw pointers)"""
        check(lib().zh_knn_graph_reverse_device(self._h, d_in_ids_ptr, d_in_counts_ptr, int(in_k), int(rev_k), int(first_row), int(n), d_ids_ptr, d_counts_ptr,
                                                d_degree_ptr, stream))

    def knn_reverse_info(self):
        """what the most recent knn_graph_reverse call on this index did (zh_knn_graph_reverse_info): rows_live, lines, in_k, rev_k, edges, kept,
        max_degree, launches"""
        return self._info(_ffi.KnnReverseInfo, lib().zh_knn_graph_reverse_info)

    def deduplicate_within(self, radius, metric):
        """near-duplicate removal: rows are taken in ascending id, and row b is removed exactly when some KEPT row a < b forms a joined pair
        with it (self_join at `radius`).  Decided on the host from the sorted pair list, then passed to remove -> the removed ids, ascending."""
        a, b, _ = self.self_join(radius, metric)
        removed = dedup_rule(a, b)
        if removed.size:
            self.remove(removed)
        return removed

    def self_join_forest(self, radius=None, metric=None, max_key=None, capacity=None):
        """FOREST self-join: every pair of distinct stored rows (a, b), a < b, that share a leaf in at least one tree (get_forest()'s leaf_ids)
        and whose key is <= ONE threshold -- `radius` or `max_key`, as self_join -- each pair once however many trees put the two rows together.
        self_join's keys, ids and order on an approximate candidate set: the answer is the subset of self_join's pairs that are leaf-mates.
        -> (a u64, b u64, keys u64), ascending by (a, key, b).  One call with a guessed capacity; when the pairs exceed it, one more with the
        exact total the first call reported.  Needs a built forest."""
        mk = self._join_key(radius, metric, max_key)
        cap = int(capacity) if capacity is not None else max(1024, 16 * len(self))
        return _with_capacity(cap, 3, lambda cap, o, total: lib().zh_self_join_forest(
            self._h, mk, metric.metric, metric.mode, cap, _p(o[0]), _p(o[1]), _p(o[2]), C.byref(total)))


    def self_join_forest_count(self, radius=None, metric=None, max_key=None):
        """how many pairs self_join_forest would return (a call with capacity 0: nothing is ordered or written)"""
        mk = self._join_key(radius, metric, max_key)
        return _count(lambda total: lib().zh_self_join_forest(
            self._h, mk, metric.metric, metric.mode, 0, None, None, None, C.byref(total)))


    def self_join_forest_device(self, max_key, metric, capacity, d_a_ptr, d_b_ptr, d_keys_ptr, d_total_ptr, stream=None):
        """self_join_forest with a, b, keys (`capacity` each) and the total (one u64) in device memory (raw pointers, e.g. torch .data_ptr()).
        Pairs beyond the capacity raise ZhError with code ZH_ELIMIT; the total is exact even then."""
        check(lib().zh_self_join_forest_device(self._h, int(max_key), metric.metric, metric.mode, capacity, d_a_ptr, d_b_ptr, d_keys_ptr, d_total_ptr,
                                               stream))

    def join_forest_info(self):
        """what the most recent forest self-join on this index did (zh_self_join_forest_info): rows_live, trees, path, leaf_pairs, pairs,
        candidates, launches, tiles, redone"""
        return self._info(_ffi.JoinForestInfo, lib().zh_self_join_forest_info)

    def deduplicate_within_forest(self, radius, metric):
        """deduplicate_within's rule over the forest self-join's pairs (self_join_forest at `radius`): near-duplicates that no tree puts into
        one leaf are not seen -> the removed ids, ascending."""
        a, b, _ = self.self_join_forest(radius, metric)
        removed = dedup_rule(a, b)
        if removed.size:
            self.remove(removed)
        return removed

    def debug_keep_raw(self, on=True):
        """tests: half-width batches keep a copy of the scan's raw pairs (zh_debug_keep_raw)"""
        check(lib().zh_debug_keep_raw(self._h, 1 if on else 0))

    def debug_scan_pairs(self, ctx=None):
        """tests: every scored (row, query) pair of the most recent half-width batch of `ctx` (None: the blocking context, i.e. the last
        search_batch_device call) as the scan made it -> (info dict, structured array of zh_debug_pair, qmeta [queries x 4]); zh_debug_scan_pairs"""
        info = _ffi.DebugScanInfo()
        h = ctx._h if ctx is not None else None
        check(lib().zh_debug_scan_pairs(self._h, h, C.byref(info), None, 0, None))
        dt = np.dtype([("row", "<u4"), ("query", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("raw_s", "<f4"), ("raw_a2", "<f4"), ("flags", "<u4"), ("visit", "<u4")])
        assert dt.itemsize == C.sizeof(_ffi.DebugPair)
        pairs = np.zeros(int(info.pairs), dt)
        qmeta = np.zeros((int(info.queries), 4), np.float32)
        if info.approx_scan:
            check(lib().zh_debug_scan_pairs(self._h, h, C.byref(info), pairs.ctypes.data_as(C.c_void_p), pairs.shape[0], qmeta.ctypes.data_as(C.c_void_p)))
        return info.as_dict(), pairs, qmeta

    def debug_walk_pairs(self, metric, first_pos, n_pos, right=None):
        """tests: the interval of EVERY pair of the rectangle held positions [first_pos, first_pos + n_pos) of this index's fp16 copy x every
        position of `right`'s (None: this index itself -- the self-join's and the graphs' view; another index: the cross join's), as the joins'
        and the graphs' matrix-core scans form it -> (info dict, structured array of zh_debug_walk_pair, record (held_pos - first_pos) *
        col_positions + col_pos); zh_debug_walk_pairs"""
        info = _ffi.DebugWalkInfo()
        rh = self._h if right is None else right._h
        check(lib().zh_debug_walk_pairs(self._h, rh, metric.metric, metric.mode, int(first_pos), int(n_pos), C.byref(info), None, 0))
        dt = np.dtype([("held_pos", "<u4"), ("col_pos", "<u4"), ("held_row", "<u4"), ("col_row", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("raw_s", "<f4")])
        assert dt.itemsize == C.sizeof(_ffi.DebugWalkPair)
        pairs = np.zeros(int(info.pairs), dt)
        if info.pairs:
            check(lib().zh_debug_walk_pairs(self._h, rh, metric.metric, metric.mode, int(first_pos), int(n_pos), C.byref(info),
                                            pairs.ctypes.data_as(C.c_void_p), pairs.shape[0]))
        return info.as_dict(), pairs

    def read_rows(self, first, n):
        """KeyValue::embedding (lsh.rs:107-119) for a run of rows."""
        out = np.empty((n, self.dim), np.float32)
        check(lib().zh_index_read_rows(self._h, first, n, _p(out)))
        return out

    def search_context(self):
        """one in-flight batch (zh_search_begin / finish / wait); create two to software-pipeline batches"""
        return SearchContext(self)

    def sweep_stream(self):
        """the index's lowest-priority stream (raw hipStream_t) for SearchContext.finish(..., sweep_stream=)"""
        return lib().zh_index_sweep_stream(self._h)

    def rows_device_ptr(self):
        return lib().zh_index_rows_device(self._h)

    def set_profiling(self, level):
        check(lib().zh_set_profiling(self._h, level))

    def set_dense_levels(self, levels):
        check(lib().zh_set_dense_levels(self._h, levels))

    def set_sweep_mode(self, mode):
        """0 = chosen per batch (default: a batch hashed from row scores is prefiltered, not swept), 1 = leaf by leaf, 2 = table
        scan with f32 queries, 3 = as 0, 4 = table scan with half-width queries wherever it applies, 5 = as 4 with the VALU kernel only, no fp16 copy of the rows, 6 = leaf by leaf at half width where implemented: dim 128 (zh_set_sweep_mode)"""
        check(lib().zh_set_sweep_mode(self._h, {"auto": 0, "leaf": 1, "scan": 2, "prefilter": 3, "approx": 4, "approx-valu": 5, "leaf-half": 6}.get(mode, mode)))

    def set_hash_mode(self, mode):
        """0 = chosen per batch (default), 1 = one dot product per plane, 2 = from row scores (zh_set_hash_mode)"""
        check(lib().zh_set_hash_mode(self._h, {"auto": 0, "dense": 1, "scores": 2}.get(mode, mode)))

    def stats(self, reset=False):
        s = _ffi.Stats()
        check(lib().zh_stats(self._h, C.byref(s)))
        if reset:
            check(lib().zh_stats_reset(self._h))
        return s.as_dict()


class SearchContext:
    """Pipelined search (include/zebra_hip.h, zh_search_begin/finish/wait) on raw device pointers."""

    def __init__(self, index):
        self._index = index  # keeps the index alive
        self._h = C.c_void_p()
        check(lib().zh_search_ctx_create(index._h, C.byref(self._h)))
        index._adopt(self)

    def begin(self, d_q_ptr, b, top_k, metric, stream=None):
        check(lib().zh_search_begin(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode, stream))

    def finish(self, d_ids_ptr, d_keys_ptr, d_counts_ptr, sweep_stream=None):
        check(lib().zh_search_finish(self._h, d_ids_ptr, d_keys_ptr, d_counts_ptr, sweep_stream))

    def begin_window(self, d_q_ptrs, b, top_k, metric, stream=None):
        """len(d_q_ptrs) batches of b queries handled as one internal batch (zh_search_begin_window)"""
        arr = (C.c_void_p * len(d_q_ptrs))(*d_q_ptrs)
        check(lib().zh_search_begin_window(self._h, arr, len(d_q_ptrs), b, top_k, metric.metric, metric.mode, stream))

    def finish_window(self, d_ids_ptrs, d_keys_ptrs, d_counts_ptrs, sweep_stream=None):
        n = len(d_ids_ptrs)
        a, b_, c = (C.c_void_p * n)(*d_ids_ptrs), (C.c_void_p * n)(*d_keys_ptrs), (C.c_void_p * n)(*d_counts_ptrs)
        check(lib().zh_search_finish_window(self._h, a, b_, c, sweep_stream))

    def wait(self):
        check(lib().zh_search_wait(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().zh_search_ctx_destroy(self._h)
            self._h = None

    __del__ = close


UNIQUE_ID_BYTES = 128


def shard_unique_id():
    """rank 0: the 128-byte id every rank passes to ShardGroup (ncclGetUniqueId inside the library)"""
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    check(lib().zh_shard_unique_id(buf))
    return bytes(buf)


class ShardGroup:
    """This rank's shard (an LSHIndex over its rows, id_base = its first global row) joined with the other ranks'
    through RCCL inside libzebra_hip.so: search_batch over the WHOLE sharded index is one call per batch on every rank
    (local search -> one all-gather of the packed top-k -> merge), the loop of core.rs:299-303 for sharded rows."""

    def __init__(self, index, unique_id, n_ranks, rank):
        self.index = index  # borrowed by the group: keep it alive
        self._h = C.c_void_p()
        uid = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().zh_shard_group_create(index._h, uid, n_ranks, rank, C.byref(self._h)))

    def ranks(self):
        return int(lib().zh_shard_group_ranks(self._h))

    def rank(self):
        return int(lib().zh_shard_group_rank(self._h))

    def search_batch(self, queries, top_k, metric):
        """merged global top-k of every query: (ids [b,k] u64, keys [b,k] u64, counts [b] u32)"""
        q = _f32(queries, self.index.dim)
        b = q.shape[0]
        ids = np.empty((b, top_k), np.uint64)
        keys = np.empty((b, top_k), np.uint64)
        counts = np.zeros(b, np.uint32)
        check(lib().zh_shard_search_batch(self._h, _p(q), b, top_k, metric.metric, metric.mode, _p(ids), _p(keys), _p(counts)))
        return ids, keys, counts

    def search_batch_device(self, d_q_ptr, b, top_k, metric, d_ids_ptr, d_keys_ptr, d_counts_ptr):
        check(lib().zh_shard_search_batch_device(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode, d_ids_ptr,
                                                 d_keys_ptr, d_counts_ptr))

    def search_context(self):
        return ShardContext(self)

    def close(self):
        if getattr(self, "_h", None):
            lib().zh_shard_group_destroy(self._h)
            self._h = None

    __del__ = close


class ShardContext:
    """one sharded batch in flight (zh_shard_search_begin / finish / wait) on raw device pointers"""

    def __init__(self, group):
        self._group = group
        self._h = C.c_void_p()
        check(lib().zh_shard_ctx_create(group._h, C.byref(self._h)))

    def begin(self, d_q_ptr, b, top_k, metric):
        check(lib().zh_shard_search_begin(self._h, d_q_ptr, b, top_k, metric.metric, metric.mode))

    def finish(self, d_ids_ptr, d_keys_ptr, d_counts_ptr):
        check(lib().zh_shard_search_finish(self._h, d_ids_ptr, d_keys_ptr, d_counts_ptr))

    def begin_window(self, d_q_ptrs, b, top_k, metric):
        arr = (C.c_void_p * len(d_q_ptrs))(*d_q_ptrs)
        check(lib().zh_shard_search_begin_window(self._h, arr, len(d_q_ptrs), b, top_k, metric.metric, metric.mode))

    def finish_window(self, d_ids_ptrs, d_keys_ptrs, d_counts_ptrs):
        n = len(d_ids_ptrs)
        a, b_, c = (C.c_void_p * n)(*d_ids_ptrs), (C.c_void_p * n)(*d_keys_ptrs), (C.c_void_p * n)(*d_counts_ptrs)
        check(lib().zh_shard_search_finish_window(self._h, a, b_, c))

    def wait(self):
        check(lib().zh_shard_search_wait(self._h))

    def stream(self):
        """raw hipStream_t the merged results complete on"""
        return lib().zh_shard_ctx_stream(self._h)

    def local_result_ptr(self):
        return lib().zh_shard_ctx_local_result(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().zh_shard_ctx_destroy(self._h)
            self._h = None

    __del__ = close


def merge_topk_device(device, n_shards, b, k, d_ids, d_keys, d_counts, d_out_ids, d_out_keys, d_out_counts, stream=None):
    check(lib().zh_merge_topk_device(device, n_shards, b, k, d_ids, d_keys, d_counts, d_out_ids, d_out_keys,
                                     d_out_counts, stream))


def packed_result_words(b, k):
    """u64 words of one rank's packed result: [ids b*k][keys b*k][counts b u32, padded]"""
    return int(lib().zh_packed_result_words(b, k))


def merge_topk_packed_device(device, n_shards, b, k, d_packed, d_out_ids, d_out_keys, d_out_counts, stream=None):
    check(lib().zh_merge_topk_packed_device(device, n_shards, b, k, d_packed, d_out_ids, d_out_keys, d_out_counts, stream))


def synth_queries_device(device, d_out, n_rows, b, dim, b0=0, seed_rows=0x5EB2A001, seed_q=0x5EB2A002, kind=0, stream=None):
    check(lib().zh_synth_queries_device(device, d_out, seed_rows, seed_q, n_rows, b0, b, dim, kind, stream))


# ------------------------------------------------------------------------ src/database/core.rs
def trim_device_memory():
    """zh_trim_device_memory: does nothing (the library caches no device memory; freed buffers go back to the driver at once)"""
    check(lib().zh_trim_device_memory())


def dedup_rule(a, b):
    """deduplicate_within's rule on a pair list sorted by a (self_join's order): b is removed exactly when a kept a < b is paired with it.
    Every pair has a < b, so when the pairs of a are reached, whether a is kept is already final -> the removed ids (u64), ascending."""
    removed = set()
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        if x not in removed:
            removed.add(y)
    return np.array(sorted(removed), np.uint64)


def matched_rule(a):
    """remove_within's rule on cross_join's left ids: a row of the left index goes when it is in at least one pair -> the distinct a (u64),
    ascending"""
    return np.unique(np.asarray(a, dtype=np.uint64))


class Database:
    """Database<N, Met, Mod> restricted to the two calls on the hot path: insert_records
    (core.rs:245-254) and query_vectors (core.rs:290-313).  Documents are kept in memory (the lz4
    files and the embedding model are out of scope)."""

    def __init__(self, dim, metric, index_options=None, **index_kwargs):
        # a metric CLASS is default-constructed, as Database::new / open do with `Met::default()` (core.rs:115,146)
        self.metric = metric() if isinstance(metric, type) else metric
        self.index = LSHIndex(dim, index_options, **index_kwargs)  # pub field `index`, core.rs:62
        self._documents = {}

    def insert_records(self, embeddings, documents):
        ids = self.index.add(embeddings)
        for i, doc in zip(ids.tolist(), documents):
            self._documents[i] = doc

    def remove(self, embedding_ids):
        """core.rs:205-214: index.remove, then the removed ids' documents go too"""
        for i in self.index.remove(embedding_ids).tolist():
            self._documents.pop(i, None)

    def deduplicate(self):
        """core.rs:216-225"""
        for i in self.index.deduplicate().tolist():
            self._documents.pop(i, None)

    def compact(self):
        """reclaim the device memory of removed vectors (LSHIndex.compact) and re-key the documents with the old -> new id map.  Rows move, so the
        database is left WITHOUT a graph (build_graph again before query_vectors_graph) -- unless nothing was removed and nothing moved."""
        new_ids, info = self.index.compact()
        base, gone = self.index.id_base, np.uint64(0xFFFFFFFFFFFFFFFF)
        docs = {}
        for i, doc in self._documents.items():
            r = i - base
            if 0 <= r < new_ids.size and new_ids[r] != gone:
                docs[int(new_ids[r])] = doc
        self._documents = docs
        return info

    def clear_database(self):
        """core.rs:194-198"""
        self.index.clear()
        self._documents.clear()

    def query_vectors(self, vectors, number_of_results):
        """-> {query index: {id: document}} ; order and distances are dropped as in core.rs:304-305."""
        if self.index.no_vectors():
            return {}
        ids, _, counts = self.index.search_batch(vectors, number_of_results, self.metric)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[b, :counts[b]]} for b in range(ids.shape[0])}

    def query_vectors_where(self, vectors, number_of_results, predicate):
        """query_vectors among the records whose document satisfies predicate(document): the exact nearest neighbours of every query among
        them (LSHIndex.search_exact_filtered_batch) -> {query index: {id: document}}"""
        if self.index.no_vectors():
            return {}
        allowed = np.fromiter((i for i, doc in self._documents.items() if predicate(doc)), np.uint64)
        ids, _, counts = self.index.search_exact_filtered_batch(vectors, number_of_results, self.metric, allowed)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[b, :counts[b]]} for b in range(ids.shape[0])}

    def query_vectors_within(self, vectors, radius):
        """every record within `radius` of each query (LSHIndex.search_range_batch: exact, however many there are)
        -> {query index: {id: document}}, each query's records in ascending (key, id) order"""
        if self.index.no_vectors():
            return {}
        offsets, ids, _ = self.index.search_range_batch(vectors, radius, self.metric)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[int(offsets[b]):int(offsets[b + 1])]} for b in range(offsets.size - 1)}

    def query_vectors_within_forest(self, vectors, radius, probe=1):
        """query_vectors_within among the records in the leaves the forest's walk visits for each query (LSHIndex.search_range_forest_batch:
        exact keys, approximate candidates) -> what query_vectors_within returns, for the records the forest finds"""
        if self.index.no_vectors():
            return {}
        offsets, ids, _ = self.index.search_range_forest_batch(vectors, radius, self.metric, probe=probe)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[int(offsets[b]):int(offsets[b + 1])]} for b in range(offsets.size - 1)}

    def near_duplicates(self, radius):
        """every pair of records within `radius` of each other (LSHIndex.self_join: exact) -> [(document_a, document_b, distance)], in
        ascending (id a, key, id b) order.  The distance is the number the key holds (for the parity cosine key: the similarity)."""
        a, b, keys = self.index.self_join(radius, self.metric)
        dist = self._key_numbers(keys)
        return [(self._documents.get(x), self._documents.get(y), float(v)) for x, y, v in zip(a.tolist(), b.tolist(), dist.tolist())]

    def near_duplicates_forest(self, radius):
        """near_duplicates among the records that share a leaf of the forest (LSHIndex.self_join_forest: exact keys, approximate candidates)
        -> what near_duplicates returns, for the pairs the forest finds"""
        if self.index.no_vectors():
            return []
        a, b, keys = self.index.self_join_forest(radius, self.metric)
        dist = self._key_numbers(keys)
        return [(self._documents.get(x), self._documents.get(y), float(v)) for x, y, v in zip(a.tolist(), b.tolist(), dist.tolist())]

    def matches(self, other_db, radius):
        """every pair (record of this database, record of `other_db`) within `radius` (LSHIndex.cross_join: exact; the key is other_db's
        stored vector against this database's as the query, under this database's metric) -> [(document, other document, distance)], in
        ascending (id, key, other id) order.  The distance is the number the key holds, as in near_duplicates."""
        a, b, keys = self.index.cross_join(other_db.index, radius, self.metric)
        dist = self._key_numbers(keys)
        return [(self._documents.get(x), other_db._documents.get(y), float(v)) for x, y, v in zip(a.tolist(), b.tolist(), dist.tolist())]

    def nearest_in(self, other_db, k):
        """every record's k nearest records of `other_db` (LSHIndex.cross_knn: exact; the key is other_db's stored vector against this
        database's as the query, under this database's metric) -> {document: [(other document, distance), ...]}, nearest first, one entry per
        live record.  The distance is the number the key holds, as in near_duplicates."""
        if self.index.no_vectors():
            return {}
        return self._graph_documents(*self.index.cross_knn(other_db.index, k, self.metric), neighbours=other_db._documents)

    def remove_within(self, other_db, radius):
        """LSHIndex.remove_within against other_db's index, then the removed ids' documents go too -> the removed ids"""
        removed = self.index.remove_within(other_db.index, radius, self.metric)
        for i in removed.tolist():
            self._documents.pop(i, None)
        return removed

    def _key_numbers(self, keys):
        """the number each key holds, as f64 (for the parity cosine key: the similarity)"""
        if self.metric.metric in _F64_KEYED:
            return keys.view(np.float64)
        if self.metric.metric == _ffi.HAMMING:
            return keys.astype(np.float64)
        return keys.astype(np.uint32).view(np.float32).astype(np.float64)

    def knn_graph(self, k):
        """every record's k nearest other records (LSHIndex.knn_graph: exact) -> {document: [(neighbour document, distance)], nearest first},
        one entry per live record.  The distance is the number the key holds, as in near_duplicates."""
        return self._graph_documents(*self.index.knn_graph(k, self.metric))

    def knn_graph_forest(self, k):
        """every record's k nearest records among those that share a leaf of the forest with it (LSHIndex.knn_graph_forest) -> what knn_graph
        returns"""
        if self.index.no_vectors():
            return {}
        return self._graph_documents(*self.index.knn_graph_forest(k, self.metric))

    def knn_graph_refined(self, k, rounds=1, reverse=0):
        """knn_graph_forest, then `rounds` rounds of LSHIndex.knn_graph_refine (each row's neighbours' neighbours, until a round changes
        nothing; reverse > 0: with that many sampled reverse neighbours per row as well) -> what knn_graph returns"""
        if self.index.no_vectors():
            return {}
        graph = self.index.knn_graph_forest(k, self.metric)
        return self._graph_documents(*self.index.knn_graph_refine(graph, k, self.metric, rounds=rounds, reverse=reverse))

    def knn_graph_descent(self, k, rounds=8, reverse=0):
        """knn_graph_forest, then LSHIndex.knn_graph_descent: the rounds of knn_graph_refined in one call on the device, keying only what is new
        from the second round on -- the same answer -> what knn_graph returns"""
        if self.index.no_vectors():
            return {}
        graph = self.index.knn_graph_forest(k, self.metric)
        return self._graph_documents(*self.index.knn_graph_descent(graph, k, self.metric, rounds=rounds, reverse=reverse))

    def build_graph(self, k=32, rounds=8, reverse=0, prune=0, prune_reverse=0, fill=False):
        """make the graph query_vectors_graph walks and attach it to the index: knn_graph_forest(k), LSHIndex.knn_graph_descent(rounds, reverse),
        LSHIndex.set_graph.  prune > 0: LSHIndex.knn_graph_prune(degree=prune, reverse=prune_reverse, fill=fill) between the descent and the
        attach; prune = 0 is the call without it.  Needs trees.  Records added later are found only as seeds until extend_graph gives them lines (or the graph is built
        again); removed ones are skipped at once.  -> LSHIndex.graph_info()"""
        if self.index.no_vectors():
            return self.index.graph_info()
        graph = self.index.knn_graph_forest(k, self.metric)
        graph = self.index.knn_graph_descent(graph, k, self.metric, rounds=rounds, reverse=reverse)
        if prune:
            graph = self.index.knn_graph_prune(graph, prune, self.metric, reverse=prune_reverse, fill=fill)
        self.index.set_graph(graph)
        return self.index.graph_info()

    def extend_graph(self, beam=64, **kw):
        """lines for the records added since build_graph (or the last extend_graph), and the old lines re-ranked to name them:
        LSHIndex.extend_graph under the database's metric (width, max_iters, seeds, n_seed, batch as there; beam is raised to the graph's
        width).  Far cheaper than build_graph while the added records are few; see the README for where the rebuild takes over.
        -> LSHIndex.extend_graph_info()"""
        if self.index.no_vectors() or not self.index.graph_info()["attached"]:
            return self.index.extend_graph_info()
        return self.index.extend_graph(self.metric, beam=max(int(beam), self.index.graph_info()["g_k"]), **kw)

    def query_vectors_graph(self, vectors, number_of_results, beam=64, **kw):
        """query_vectors answered by LSHIndex.search_graph_batch over the graph build_graph attached (beam, width, max_iters, seeds, n_seed as
        there; beam is raised to number_of_results) -> {query index: {id: document}}"""
        if self.index.no_vectors():
            return {}
        ids, _, counts = self.index.search_graph_batch(vectors, number_of_results, self.metric, beam=max(int(beam), int(number_of_results)), **kw)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[b, :counts[b]]} for b in range(ids.shape[0])}

    def query_vectors_graph_where(self, vectors, number_of_results, predicate, beam=64, hops=0, **kw):
        """query_vectors_graph among the records whose document satisfies predicate(document).  hops=0: LSHIndex.search_graph_filtered_batch
        (the walk goes through every record, the answer holds only those; seeds="allowed" starts it from them); hops=1 or 2:
        LSHIndex.search_graph_steered_batch (the walk keeps to those records and, with 2, hops over the others: the call for a selective
        predicate) -> what query_vectors_graph returns"""
        if self.index.no_vectors():
            return {}
        allowed = np.fromiter((i for i, doc in self._documents.items() if predicate(doc)), np.uint64)
        if hops:
            ids, _, counts = self.index.search_graph_steered_batch(vectors, number_of_results, self.metric, allowed, hops=hops,
                                                                   beam=max(int(beam), int(number_of_results)), **kw)
        else:
            ids, _, counts = self.index.search_graph_filtered_batch(vectors, number_of_results, self.metric, allowed,
                                                                    beam=max(int(beam), int(number_of_results)), **kw)
        return {b: {int(i): self._documents.get(int(i)) for i in ids[b, :counts[b]]} for b in range(ids.shape[0])}

    def _graph_documents(self, ids, keys, counts, neighbours=None):
        """lines of this database's rows as documents; neighbours: the documents the ids name (default: this database's own)"""
        neighbours = self._documents if neighbours is None else neighbours
        dist = self._key_numbers(np.ascontiguousarray(keys)).reshape(keys.shape)
        base = self.index.id_base
        out = {}
        for r in range(ids.shape[0]):
            if (base + r) not in self._documents:
                continue  # a removed row's line
            c = int(counts[r])
            out[self._documents[base + r]] = [(neighbours.get(i), float(v)) for i, v in zip(ids[r, :c].tolist(), dist[r, :c].tolist())]
        return out

    def deduplicate_within(self, radius):
        """LSHIndex.deduplicate_within, then the removed ids' documents go too -> the removed ids"""
        removed = self.index.deduplicate_within(radius, self.metric)
        for i in removed.tolist():
            self._documents.pop(i, None)
        return removed

    def deduplicate_within_forest(self, radius):
        """LSHIndex.deduplicate_within_forest, then the removed ids' documents go too -> the removed ids"""
        if self.index.no_vectors():
            return np.empty(0, np.uint64)
        removed = self.index.deduplicate_within_forest(radius, self.metric)
        for i in removed.tolist():
            self._documents.pop(i, None)
        return removed

"""The forest range search (zh_search_range_forest_batch): for every query, every member of every leaf the walk visits for it with n = probe whose key
is <= the query's threshold key, each row once, as search_range_batch's CSR.  The reference is built here from existing pieces only: the oracle's
walk on the index's own forest (Forest.from_arrays(X, M, ix.get_forest()).tree_result(t, q, probe, ...)) gives the visits (off, len, _), the
candidates are np.unique of the concatenated leaf_ids[off:off + len], the keys are distance_batch(X[cands], q), the hits key <= max_key in
np.lexsort((id, key)) order.  visits / leaf_rows / tiles come from the same visit lists; the library's walk records a visit where it takes rows,
so the oracle's visits of EMPTY leaves (len 0: it passes through them to the backup) are not counted.  Every comparison is bit for bit on
offsets, ids, keys, dtypes and the total.  Thresholds are keys of the reference's own candidate keys, each query's own j-th smallest -- the
tightest case for the tau map -- and UINT64_MAX.  The shapes are test_gpu_fjoin.py's; the indexes are filled with add, shared per module and
never changed by a test that shares them."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

ALL = np.uint64(2**64 - 1)
EINVAL, ESTATE, ELIMIT = -1, -4, -5
NB, DB = 4096 + 37, 256


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def thirteen_metrics(za):
    """every metric and cosine mode, the two parametrised ones at one power each"""
    return [(za.L2SquaredDistance(), zo.L2SQ, 0), (za.L2Distance(), zo.L2, 0), (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
            (za.CosineDistance(parity=False), zo.COSINE, zo.CORRECTED), (za.ChebyshevDistance(), zo.CHEBYSHEV, 0),
            (za.CanberraDistance(), zo.CANBERRA, 0), (za.BrayCurtisDistance(), zo.BRAY_CURTIS, 0), (za.ManhattanDistance(), zo.MANHATTAN, 0),
            (za.L3Distance(), zo.L3, 0), (za.L4Distance(), zo.L4, 0), (za.HammingDistance(), zo.HAMMING, 0),
            (za.MinkowskiDistance(3), zo.MINKOWSKI, 3), (za.PNormDistance(65), zo.PNORM, 65)]


# ---------------------------------------------------------------- the reference
class Walk:
    """the oracle's visit lists of a query set on a forest: per query and tree the (off, len) of every visited leaf, and what follows from them"""

    def __init__(self, X, M, forest, Q, probe, cap_visits=1 << 14):
        f = zo.Forest.from_arrays(X, M, forest)
        self.leaf_ids = np.asarray(forest["leaf_ids"]).astype(np.int64)
        self.T = int(np.asarray(forest["roots"]).size)
        self.raw_visits = []  # per query: the oracle's visits over all trees, empty leaves included
        self.lists = []       # per query and tree: (off, len) of the visited NON-EMPTY leaves
        for q in Q:
            per_tree, raw = [], 0
            for t in range(self.T):
                _, _, v = f.tree_result(t, q, probe, zo.L2SQ, 0, cap_visits=cap_visits)  # (the visit sequence never depends on the metric)
                assert v.shape[0] < cap_visits
                raw += v.shape[0]
                per_tree.append([(int(o), int(n)) for o, n, _ in v.tolist() if n > 0])
            self.raw_visits.append(raw)
            self.lists.append(per_tree)
        self.cands = [np.unique(np.concatenate([self.leaf_ids[o:o + n] for pt in per for o, n in pt] + [np.zeros(0, np.int64)])) for per in self.lists]
        self.visits = sum(len(pt) for per in self.lists for pt in per)
        self.leaf_rows = sum(n for per in self.lists for pt in per for _, n in pt)
        visitors = {}
        for per in self.lists:
            for pt in per:
                for o, n in pt:
                    visitors[(o, n)] = visitors.get((o, n), 0) + 1
        self.visitors = visitors  # (off, len) of a visited leaf -> queries that visit it (a leaf belongs to one tree; a query visits it once)
        self.tiles = sum(((n + 15) // 16) * ((v + 15) // 16) for (_, n), v in visitors.items())


def keyed(X, Q, walk, om, omode):
    """per query (candidate ids, their oracle keys), ascending by (key, id)"""
    out = []
    for q, c in zip(Q, walk.cands):
        k = np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[c]), q), np.uint64) if c.size else np.zeros(0, np.uint64)
        o = np.lexsort((c, k))
        out.append((c[o].astype(np.uint64), k[o]))
    return out


def jth_keys(ref, j):
    """each query's own j-th smallest candidate key (its largest when it has fewer)"""
    return np.array([k[min(j, k.size - 1)] if k.size else 0 for _, k in ref], np.uint64)


def within(ref, mk, id_base=0):
    """the reference at per-query thresholds -> (offsets, ids, keys)"""
    mk = np.broadcast_to(np.asarray(mk, np.uint64), (len(ref),))
    ids, keys, off = [], [], [0]
    for (c, k), t in zip(ref, mk):
        m = k <= t
        ids.append(c[m] + np.uint64(id_base))
        keys.append(k[m])
        off.append(off[-1] + int(m.sum()))
    return np.array(off, np.uint64), np.concatenate(ids + [np.zeros(0, np.uint64)]), np.concatenate(keys + [np.zeros(0, np.uint64)])


def same(got, want):
    for g, r, what in zip(got, want, ("offsets", "ids", "keys")):
        assert g.dtype == np.uint64 and g.shape == r.shape and (g == r).all(), what


def each_hit_once(got):
    off, ids, _ = got
    return all(np.unique(ids[int(off[i]):int(off[i + 1])]).size == int(off[i + 1] - off[i]) for i in range(off.size - 1))


def raw_call(ix, Q, mk, probe, m, capacity, with_arrays=True):
    """the host entry point itself -> (rc, total, offsets)"""
    from zebra_amd import _ffi
    Q = np.ascontiguousarray(Q, np.float32)
    b = Q.shape[0]
    mk = np.ascontiguousarray(np.broadcast_to(np.asarray(mk, np.uint64), (b,)))
    ids, keys = (np.zeros(max(capacity, 1), np.uint64) for _ in range(2))
    off = np.full(b + 1, 777, np.uint64)
    total = C.c_uint64(777)
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    A = lambda x: P(x) if with_arrays else None  # noqa: E731
    rc = _ffi.lib().zh_search_range_forest_batch(ix._h, P(Q), b, P(mk), probe, m.metric, m.mode, capacity, P(off), A(ids), A(keys), C.byref(total))
    return rc, int(total.value), off


def on_path(monkeypatch, path):
    monkeypatch.delenv("ZH_FRANGE_CAND_CAP", raising=False)
    monkeypatch.delenv("ZH_WALK_LOG_CHUNKS", raising=False)
    if path:  # 1: path 1; 2: path 2 wherever the path rule admits it, whatever the visit gate says
        monkeypatch.setenv("ZH_FRANGE_PATH", str(path))
    else:     # the path rule and the visit gate
        monkeypatch.delenv("ZH_FRANGE_PATH", raising=False)


# ---------------------------------------------------------------- shapes (an index per shape, shared; no test changes one)
_SHARED = {}  # the shared indexes, closed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()


@functools.lru_cache(maxsize=None)
def rows_b(d=DB, n=NB):
    return zo.synth_rows(n, d)


@functools.lru_cache(maxsize=None)
def rows_bdup():
    X = rows_b().copy()
    X[1000:1400] = X[1000]  # 400 bit-identical rows: one unsplittable leaf of 400 at max_node_size 256, many tiny and empty leaves around it
    return X


NEAR = [(i, 100 + i) for i in range(60)]


@functools.lru_cache(maxsize=None)
def planted_rows(uncertain):
    """tests/test_gpu_join.py's planted rows, restated"""
    X = rows_b().copy()
    for i, j in NEAR:  # near-duplicates below fp16 resolution: the copy's two rows are the same halves, only the canonical key tells them apart
        X[j] = X[i] * np.float32(1.0 + 2.0**-12)
    X[200:220] = X[300:320]  # bit-identical pairs
    X[400:410] *= np.float32(2.0**40)
    X[410:420] *= np.float32(2.0**-40)
    X[500:510] = np.round(X[500:510] * 100.0)  # integer-valued rows
    X[600] = 0.0
    if uncertain:  # one row with an infinite element and one whose |x|^2 overflows: nothing certain means always a candidate
        X[700, 5] = np.inf
        X[701] = np.float32(1e30)
    return X


SHAPES = {"A": (lambda: zo.synth_rows(1500, 30), 30, (64, 4)), "B": (rows_b, DB, (256, 3)), "Bdup": (rows_bdup, DB, (256, 3)),
          "C": (lambda: zo.synth_rows(2000, 30), 30, (5, 15)), "planted": (lambda: planted_rows(False), DB, (256, 3)),
          "uncertain": (lambda: planted_rows(True), DB, (256, 3))}


def built(name):
    """(index, X, its forest) of a shape, the index filled with add"""
    import zebra_amd as za
    if name in _SHARED:
        return _SHARED[name]
    X, d, opts = SHAPES[name]
    X = X()
    ix = za.LSHIndex(d, za.LSHIndexOptions(*opts), device=0)
    ix.add(X)
    _SHARED[name] = (ix, X, ix.get_forest())
    return _SHARED[name]


def queries_b(X):
    """64 synthetic queries, 40 copies of X[5] scaled by 1 + j 2^-12 (one leaf per tree with more than 16 visitors), stored rows 0, 17, n - 1"""
    n, d = X.shape
    near = np.stack([X[5] * np.float32(1.0 + j * 2.0**-12) for j in range(40)])
    return np.ascontiguousarray(np.concatenate([zo.synth_queries(64, d, n), near, X[[0, 17, n - 1]]]), np.float32)


@functools.lru_cache(maxsize=None)
def query_set(name, kind):
    _, X, _ = built(name)
    n, d = X.shape
    if kind == "b":
        return queries_b(X)
    if kind == "planted":  # the planted rows themselves and a zero query
        rows = sorted({i for p in NEAR for i in p}) + list(range(200, 220)) + list(range(400, 420)) + list(range(500, 510)) + [600]
        return np.ascontiguousarray(np.concatenate([X[rows], np.zeros((1, d), np.float32)]), np.float32)
    return zo.synth_queries(int(kind), d, n)


@functools.lru_cache(maxsize=None)
def walk_of(name, kind, probe):
    _, X, forest = built(name)
    return Walk(X, SHAPES[name][2][0], forest, query_set(name, kind), probe)


@functools.lru_cache(maxsize=None)
def reference(name, kind, probe, mi):
    import zebra_amd as za
    _, X, _ = built(name)
    _, om, omode = thirteen_metrics(za)[mi]
    return keyed(X, query_set(name, kind), walk_of(name, kind, probe), om, omode)


def expect_info(ix, path, walk, hits, trees, probe, batch, rows_live):
    info = ix.range_forest_info()
    assert info["path"] == path and info["redone"] == 0 and info["hits"] == hits and info["batch"] == batch, info
    assert info["visits"] == walk.visits and info["leaf_rows"] == walk.leaf_rows, (info, walk.visits, walk.leaf_rows)
    assert info["trees"] == trees and info["probe"] == probe and info["rows_live"] == rows_live, info
    if path == 1:
        assert info["tiles"] == 0 and info["candidates"] == 0, info
    else:
        assert info["tiles"] == walk.tiles and info["candidates"] >= info["hits"], (info, walk.tiles)
    return info


# ---------------------------------------------------------------- 1. path 1, every metric
@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, monkeypatch, mi):
    ix, X, _ = built("A")
    m = thirteen_metrics(za)[mi][0]
    Q = query_set("A", "48")
    on_path(monkeypatch, 2)  # (d = 30: the path rule itself chooses path 1)
    for probe in (1, 10):
        walk, ref = walk_of("A", "48", probe), reference("A", "48", probe, mi)
        assert walk.leaf_rows > sum(c.size for c in walk.cands)  # (the shape: trees offer the same row to a query more than once)
        for mk in (jth_keys(ref, 20), jth_keys(ref, 0), ALL):
            got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=probe)
            want = within(ref, mk)
            same(got, want)
            expect_info(ix, 1, walk, want[1].size, 4, probe, 48, 1500)
            assert each_hit_once(got)
            assert (ix.range_forest_count_batch(Q, metric=m, max_keys=mk, probe=probe) == np.diff(want[0])).all()
        assert got[1].size == sum(c.size for c in walk.cands)  # UINT64_MAX: exactly the candidates


# ---------------------------------------------------------------- 2. the default regime
@pytest.mark.parametrize("mi", [0, 2])
def test_default_regime(za, monkeypatch, mi):
    """max_node_size 5, 15 trees: thousands of leaves of 0 .. 4 rows.  probe = 1 meets empty leaves and takes their backups; probe = 10 wanders
    through thousands of leaves per query, past the walk's inline visits into its log -- and, with a log of one chunk, into the
    emit walk"""
    ix, X, _ = built("C")
    m = thirteen_metrics(za)[mi][0]
    on_path(monkeypatch, 2)
    Q = query_set("C", "48")
    walk, ref = walk_of("C", "48", 1), reference("C", "48", 1, mi)
    assert max(walk.raw_visits) > 15  # (the shape: some query passed through an empty leaf to its backup)
    for mk in (jth_keys(ref, 3), ALL):
        got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
        same(got, within(ref, mk))
        expect_info(ix, 1, walk, got[1].size, 15, 1, 48, 2000)
    Q = query_set("C", "16")
    walk, ref = walk_of("C", "16", 10), reference("C", "16", 10, mi)
    assert walk.visits > 16 * 1000 and max(len(pt) for per in walk.lists for pt in per) > 32  # (thousands per query; more than ZH_INLINE_VISITS per pair)
    for chunks in (None, "1"):
        if chunks:
            monkeypatch.setenv("ZH_WALK_LOG_CHUNKS", chunks)
        for mk in (jth_keys(ref, 50), ALL):
            got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=10)
            same(got, within(ref, mk))
            expect_info(ix, 1, walk, got[1].size, 15, 10, 16, 2000)
            assert each_hit_once(got)


# ---------------------------------------------------------------- 3. states
def test_states(za, monkeypatch):
    from zebra_amd import _ffi
    X = zo.synth_rows(64, 30)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    got = ix.search_range_forest_batch(X[:3], metric=m, max_keys=ALL)  # an empty index: no row, no hit
    assert (got[0] == 0).all() and got[0].size == 4 and got[1].size == 0 and got[1].dtype == np.uint64 and ix.range_forest_info()["hits"] == 0
    ix.append(X[:3])
    with pytest.raises(za.ZhError) as e:  # rows, but no trees
        ix.search_range_forest_batch(X[:3], metric=m, max_keys=ALL)
    assert e.value.code == ESTATE
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    q, mk, off, tot = np.ascontiguousarray(X[:3]), np.full(3, ALL), np.zeros(4, np.uint64), C.c_uint64(0)
    call = lambda probe, metric: _ffi.lib().zh_search_range_forest_batch(ix._h, P(q), 3, P(mk), probe, metric, 0, 0, P(off), None, None, C.byref(tot))  # noqa: E731
    assert call(1, 99) == EINVAL and call(0, 1) == EINVAL and call(1025, 1) == ELIMIT  # the argument checks come first
    assert call(1, 1) == ESTATE
    got = ix.search_range_forest_batch(np.zeros((0, 30), np.float32), metric=m, max_keys=np.zeros(0, np.uint64))  # b = 0: whatever the state
    assert got[0].tolist() == [0] and got[1].size == 0
    ix.close()
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.add(X[:1])
    got = ix.search_range_forest_batch(X[:2], metric=m, max_keys=ALL)  # one row: every query's only candidate
    info = ix.range_forest_info()
    assert got[0].tolist() == [0, 1, 2] and got[1].tolist() == [0, 0] and info["rows_live"] == 1 and info["trees"] == 4 and info["visits"] == 8, info
    ix.add(X[1:])
    got = ix.search_range_forest_batch(X[7:8], metric=m, max_keys=ALL, probe=1)  # a stored row as the query: its own leaf in every tree
    info = ix.range_forest_info()
    assert info["visits"] == info["trees"] == 4, info
    ids, keys, _ = ix.search_exact_batch(X[7:8], 1, m)
    assert got[1][0] == 7 == ids[0, 0] and got[2][0] == keys[0, 0]  # it finds itself, first, with the exact search's key
    ix.remove(list(range(64)))
    got = ix.search_range_forest_batch(X[:3], metric=m, max_keys=ALL)  # removed rows only
    assert (got[0] == 0).all() and got[1].size == 0 and ix.range_forest_info()["rows_live"] == 0
    ix.close()


# ---------------------------------------------------------------- 4. path 2
def check_path2(za, monkeypatch, name, kind, mi, probes, thresholds, trees=3, rows_live=NB):
    ix, X, _ = built(name)
    m = thirteen_metrics(za)[mi][0]
    Q = query_set(name, kind)
    out = []
    for probe in probes:
        walk, ref = walk_of(name, kind, probe), reference(name, kind, probe, mi)
        for mk in thresholds(ref):
            on_path(monkeypatch, 2)
            got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=probe)
            want = within(ref, mk)
            same(got, want)
            expect_info(ix, 2, walk, want[1].size, trees, probe, Q.shape[0], rows_live)
            assert each_hit_once(got)
            same(ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=probe), got)  # twice: identical
            on_path(monkeypatch, 1)
            forced = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=probe)
            expect_info(ix, 1, walk, want[1].size, trees, probe, Q.shape[0], rows_live)
            same(forced, got)
            out.append(got)
    return out


@pytest.mark.parametrize("mi", range(4))
@pytest.mark.parametrize("name", ["B", "Bdup"])
def test_path2_against_the_oracle_and_path1(za, monkeypatch, name, mi):
    """B: every leaf between 16 and 256 rows, most of them no multiple of 16.  Bdup: leaves under 16 rows as well, and an unsplittable leaf of 400"""
    walk = walk_of(name, "b", 1)
    vis = list(walk.visitors.values())
    assert max(vis) > 16 and min(vis) == 1  # (the shape, on the index's own forest: several column tiles for one leaf, one visitor for another)
    assert sum(1 for (_, n) in walk.visitors if n % 16) > 0
    if name == "Bdup":
        lens = [n for (_, n) in walk_of(name, "b", 100).visitors]
        assert min(lens) < 16 and max(lens) == 400  # (visited: a leaf under one tile, and the unsplittable one)
    check_path2(za, monkeypatch, name, "b", mi, (1, 100), lambda ref: (jth_keys(ref, 30), jth_keys(ref, 1)))


@pytest.mark.parametrize("mi", [0, 2])
def test_threshold_among_tied_keys(za, monkeypatch, mi):
    """400 bit-identical rows in one leaf per tree: a query equal to them ties 400 keys; the threshold is that key -- all of them, each once"""
    ix, X, _ = built("Bdup")
    m, om, omode = thirteen_metrics(za)[mi]
    Q = np.ascontiguousarray(np.concatenate([X[1000:1001], X[1200:1201] * np.float32(1.0 + 2.0**-12), X[[3]]]), np.float32)
    walk = Walk(X, 256, ix.get_forest(), Q, 1)
    ref = keyed(X, Q, walk, om, omode)
    dup = (ref[0][0] >= 1000) & (ref[0][0] < 1400)
    assert dup.sum() == 400 and np.unique(ref[0][1][dup]).size == 1
    mk = np.array([ref[0][1][dup][0], ref[1][1][(ref[1][0] >= 1000) & (ref[1][0] < 1400)][0], ref[2][1][0]], np.uint64)
    for path in (2, 1):
        on_path(monkeypatch, path)
        got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
        same(got, within(ref, mk))
        assert ix.range_forest_info()["path"] == path
        first = got[1][:int(got[0][1])]
        assert ((first >= 1000) & (first < 1400)).sum() == 400


def test_visit_gate(za, monkeypatch):
    """left to itself the call takes path 2 only for an internal batch whose visited leaves have 32 visitors or more on average: B's query set
    (321 visits over some 70 leaves) stays on path 1, one leaf with 107 visitors goes to path 2; the arrays are the same either way"""
    ix, X, _ = built("B")
    m = za.L2SquaredDistance()
    Q = query_set("B", "b")
    walk, ref = walk_of("B", "b", 1), reference("B", "b", 1, 0)
    assert walk.visits < 32 * len(walk.visitors)
    mk = jth_keys(ref, 30)
    on_path(monkeypatch, 0)
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    expect_info(ix, 1, walk, got[1].size, 3, 1, Q.shape[0], NB)
    same(got, within(ref, mk))
    Q1 = np.ascontiguousarray(Q[64:104])  # the 40 near-copies of one row: one leaf per tree, 40 visitors each
    walk1 = Walk(X, 256, ix.get_forest(), Q1, 1)
    assert walk1.visits == 120 and len(walk1.visitors) == 3  # (40 >= 32)
    ref1 = keyed(X, Q1, walk1, zo.L2SQ, 0)
    got = ix.search_range_forest_batch(Q1, metric=m, max_keys=jth_keys(ref1, 30))
    expect_info(ix, 2, walk1, got[1].size, 3, 1, 40, NB)
    same(got, within(ref1, jth_keys(ref1, 30)))


# ---------------------------------------------------------------- 5. path 2, every dimension
@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    n = 1100
    X = rows_b(d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(128, 2), device=0)
    ix.add(X)
    Q = queries_b(X)
    walk = Walk(X, 128, ix.get_forest(), Q, 1)
    ref = keyed(X, Q, walk, zo.L2SQ, 0)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    for mk in (jth_keys(ref, 30), jth_keys(ref, 1)):
        got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
        same(got, within(ref, mk))
        expect_info(ix, 2, walk, got[1].size, 2, 1, Q.shape[0], n)
    on_path(monkeypatch, 1)
    same(ix.search_range_forest_batch(Q, metric=m, max_keys=mk), got)
    ix.close()


# ---------------------------------------------------------------- 6. adversarial rows
@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    """the queries are the planted rows themselves and a zero query; a planted row's threshold is its near-duplicate's own key (L2SQ, L2 and the
    literal cosine key; the parity key orders similarities ascending, so each query's 30th smallest key stands in, as in test_gpu_join.py): a
    bound that forgets the row's rounding loses hits here"""
    ix, X, _ = built("planted")
    m, om, omode = thirteen_metrics(za)[mi]
    Q = query_set("planted", "planted")
    ref = reference("planted", "planted", 1, mi)
    walk = walk_of("planted", "planted", 1)
    parity = om == zo.COSINE and omode == zo.PARITY
    rows = sorted({i for p in NEAR for i in p})
    partner = {i: j for i, j in NEAR}
    partner.update({j: i for i, j in NEAR})
    mk = jth_keys(ref, 30)
    mates = 0
    if not parity:
        for qi, r in enumerate(rows):
            c, k = ref[qi]
            at = np.flatnonzero(c == partner[r])
            if at.size:  # the planted partner is a leaf-mate of the query's leaves
                mk[qi] = k[at[0]]
                mates += 1
        assert mates >= 60  # (the shape: most planted partners are met in some tree)
    (got,) = check_path2(za, monkeypatch, "planted", "planted", mi, (1,), lambda ref: (mk,))
    if not parity:
        for qi, r in enumerate(rows):
            if (ref[qi][0] == partner[r]).any():
                assert partner[r] in got[1][int(got[0][qi]):int(got[0][qi + 1])].tolist()
    assert walk.visits >= Q.shape[0] * 3 - 3


@pytest.mark.parametrize("mi", [0, 3])
def test_rows_and_queries_nothing_is_certain_about(za, monkeypatch, mi):
    """path 2 against path 1: the device's own arithmetic on both sides (a NaN's sign differs between host and GPU).  Stored rows 700 (an inf) and
    701 (|x|^2 overflows), a query holding a NaN and one holding an inf: every candidate pair with one of them gets the canonical key"""
    ix, X, _ = built("uncertain")
    m = thirteen_metrics(za)[mi][0]
    Q = queries_b(X).copy()
    Q[1, 3] = np.nan
    Q[2, 9] = np.inf
    Q = np.ascontiguousarray(np.concatenate([Q, X[[700, 701]]]))
    walk = Walk(X, 256, ix.get_forest(), Q, 1)
    pairs = sum(int(np.isin(c, (700, 701)).sum()) for c in walk.cands) + walk.cands[1].size + walk.cands[2].size
    assert pairs > 0
    mk = jth_keys(reference("planted", "b", 1, mi), 30)
    mk = np.concatenate([mk, mk[:2]])
    on_path(monkeypatch, 2)
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    info = ix.range_forest_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["candidates"] >= pairs, (info, pairs)
    assert info["visits"] == walk.visits and info["tiles"] == walk.tiles, info
    on_path(monkeypatch, 1)
    same(ix.search_range_forest_batch(Q, metric=m, max_keys=mk), got)
    assert ix.range_forest_info()["path"] == 1 and each_hit_once(got)


# ---------------------------------------------------------------- 7. relations
@pytest.mark.parametrize("path", [1, 2])
def test_one_leaf_equals_the_exact_range_search(za, monkeypatch, path):
    """one tree whose root is a leaf of 8229 rows = 515 tiles: every row is a candidate of every query"""
    n = 8192 + 37
    if "one" not in _SHARED:
        X = zo.synth_rows(n, DB)
        ix = za.LSHIndex(DB, za.LSHIndexOptions(16384, 1), device=0)
        ix.add(X)
        _SHARED["one"] = (ix, X, None)
    ix, X, _ = _SHARED["one"]
    m = za.L2SquaredDistance()
    Q = queries_b(X)
    monkeypatch.delenv("ZH_RANGE_PATH", raising=False)
    _, keys, _ = ix.search_exact_batch(Q, 40, m)
    mk = np.ascontiguousarray(keys[:, 39])
    exact = ix.search_range_batch(Q, metric=m, max_keys=mk)
    assert exact[1].size >= 40 * Q.shape[0]
    on_path(monkeypatch, path)
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
    info = ix.range_forest_info()
    assert info["path"] == path and info["visits"] == Q.shape[0] and info["leaf_rows"] == Q.shape[0] * n and info["hits"] == exact[1].size, info
    if path == 2:
        assert info["tiles"] == 515 * ((Q.shape[0] + 15) // 16) and info["launches"] == 1, info
    same(got, exact)


@pytest.mark.parametrize("path", [1, 2])
def test_relations_to_the_exact_range_search(za, monkeypatch, path):
    ix, X, _ = built("B")
    m = za.L2SquaredDistance()
    Q = query_set("B", "b")
    monkeypatch.delenv("ZH_RANGE_PATH", raising=False)
    _, keys, _ = ix.search_exact_batch(Q, 30, m)
    mk = np.ascontiguousarray(keys[:, 29])
    exact = ix.search_range_batch(Q, metric=m, max_keys=mk)
    on_path(monkeypatch, path)
    # (b) probe = 1: the exact hits restricted to the reference candidates, a strict subset for some query
    walk = walk_of("B", "b", 1)
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
    ids, ks, off, strict = [], [], [0], 0
    for i in range(Q.shape[0]):
        s, e = int(exact[0][i]), int(exact[0][i + 1])
        keep = np.isin(exact[1][s:e], walk.cands[i].astype(np.uint64))
        strict += int(keep.sum() < e - s)
        ids.append(exact[1][s:e][keep]); ks.append(exact[2][s:e][keep]); off.append(off[-1] + int(keep.sum()))
    assert strict > 0
    same(got, (np.array(off, np.uint64), np.concatenate(ids), np.concatenate(ks)))
    # (c) probe = 1024: every row is a candidate of every query, so the answer is the exact one
    walk = walk_of("B", "8", 1024)
    assert all(c.size == NB for c in walk.cands)
    Q8 = query_set("B", "8")
    same(ix.search_range_forest_batch(Q8, metric=m, max_keys=mk[:8], probe=1024), ix.search_range_batch(Q8, metric=m, max_keys=mk[:8]))


@pytest.mark.parametrize("path", [1, 2])
def test_relations_to_the_forest_join_and_the_search(za, monkeypatch, path):
    ix, X, _ = built("B")
    m = za.L2SquaredDistance()
    on_path(monkeypatch, path)
    monkeypatch.delenv("ZH_FJOIN_PATH", raising=False)
    # (d) stored rows a as queries at probe = 1: the hits with id > a are exactly the forest join's pairs with that a, keys included
    rows = np.arange(0, NB, 97)
    walk = Walk(X, 256, ix.get_forest(), X[rows], 1)
    assert walk.visits == rows.size * 3  # (a stored row's walk at n = 1 ends in its own leaf)
    ref = keyed(X, X[rows], walk, zo.L2SQ, 0)
    mk = np.sort(np.concatenate([k for _, k in ref]))[rows.size * 8]
    ja, jb, jk = ix.self_join_forest(metric=m, max_key=mk)
    off, ids, keys = ix.search_range_forest_batch(X[rows], metric=m, max_keys=np.full(rows.size, mk), probe=1)
    pairs = 0
    for i, a in enumerate(rows.tolist()):
        s, e = int(off[i]), int(off[i + 1])
        above = ids[s:e] > a
        sel = ja == a
        assert (ids[s:e][above] == jb[sel]).all() and (keys[s:e][above] == jk[sel]).all() and above.sum() == sel.sum()
        pairs += int(sel.sum())
    assert pairs > 20
    # (e) probe = k = 10 with UINT64_MAX: every id search_batch returns is among the query's hits, the i-th hit key <= the i-th search key
    Q = query_set("B", "b")
    sid, skey, scount = ix.search_batch(Q, 10, m)
    off, ids, keys = ix.search_range_forest_batch(Q, metric=m, max_keys=ALL, probe=10)
    for i in range(Q.shape[0]):
        s, e, c = int(off[i]), int(off[i + 1]), int(scount[i])
        assert c > 0 and e - s >= c and np.isin(sid[i, :c], ids[s:e]).all() and (keys[s:s + c] <= skey[i, :c]).all()


# ---------------------------------------------------------------- 8. mutations
@pytest.mark.parametrize("path", [1, 2])
def test_mutations(za, monkeypatch, path):
    base = 1 << 40
    extra = zo.synth_rows(NB + 350, DB)[NB:]
    X = rows_b()
    m, om, omode = thirteen_metrics(za)[0]
    on_path(monkeypatch, path)
    ix = za.LSHIndex(DB, za.LSHIndexOptions(256, 3), device=0, id_base=base)
    ix.add(X)
    Q = queries_b(X)

    def step(rows, dead, outside=()):
        """the search against the oracle on the forest as it is now; `outside`: rows no tree holds"""
        walk = Walk(rows, 256, ix.get_forest(), Q, 1)
        ref = keyed(rows, Q, walk, om, omode)
        mk = jth_keys(ref, 30)
        got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
        same(got, within(ref, mk, base))
        expect_info(ix, path, walk, got[1].size, 3, 1, Q.shape[0], rows.shape[0] - len(dead))
        gone = np.array(list(dead) + list(outside), np.uint64) + np.uint64(base)
        every = ix.search_range_forest_batch(Q, metric=m, max_keys=ALL)
        assert every[1].size == sum(c.size for c in walk.cands) and not np.isin(every[1], gone).any()
        return got, mk

    gone = list(range(80, 96, 3)) + list(range(112, 128)) + [NB - 1]  # every third row of a tile, one whole tile, the last row
    ix.remove([g + base for g in gone])
    step(X, gone)
    ix.add(extra[:300])  # they descend the trees and split leaves
    X1 = np.concatenate([X, extra[:300]])
    step(X1, gone)
    ix.append(extra[300:])  # in no tree: never a hit
    X2 = np.concatenate([X1, extra[300:]])
    n2 = X2.shape[0]
    step(X2, gone, outside=range(n2 - 50, n2))
    ix.build()  # ... and now they take part
    got, mk = step(X2, gone)
    new_ids, _ = ix.compact()
    after = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)  # the old answer under the id map (compaction keeps the rows' order)
    same(after, (got[0], new_ids[(got[1] - np.uint64(base)).astype(np.int64)], got[2]))
    ix.close()


# ---------------------------------------------------------------- 9. a scan order that is not id order; the candidate pool
def test_scan_order_that_is_not_id_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): leaves are gathered by row number through the position map; the same
    again with the batch redone by path 1"""
    X = rows_b()
    m = za.L2SquaredDistance()
    Q = queries_b(X)
    on_path(monkeypatch, 2)
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    plain = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    plain.add(X)
    walk = Walk(X, 300, plain.get_forest(), Q, 1)
    full = keyed(X, Q, walk, zo.L2SQ, 0)
    mk = jth_keys(full, 30)
    ref = plain.search_range_forest_batch(Q, metric=m, max_keys=mk)
    assert plain.range_forest_info()["path"] == 2
    same(ref, within(full, mk))
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, DB, NB), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    assert zo.canonical_forest(ix.get_forest(), DB) == zo.canonical_forest(plain.get_forest(), DB)  # the same forest
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    expect_info(ix, 2, walk, ref[1].size, 9, 1, Q.shape[0], NB)
    same(got, ref)
    monkeypatch.setenv("ZH_FRANGE_CAND_CAP", "16")
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    info = ix.range_forest_info()
    assert info["path"] == 2 and info["redone"] > 0 and info["hits"] == ref[1].size and info["candidates"] == 0, info
    same(got, ref)
    ix.close()
    plain.close()


@pytest.mark.parametrize("name", ["B", "Bdup"])
def test_candidate_pool_overflow_is_redone_by_path1(za, monkeypatch, name):
    ix, X, _ = built(name)
    m = za.L2SquaredDistance()
    Q = query_set(name, "b")
    walk, ref = walk_of(name, "b", 1), reference(name, "b", 1, 0)
    mk = jth_keys(ref, 30)
    want = within(ref, mk)
    on_path(monkeypatch, 2)
    monkeypatch.setenv("ZH_FRANGE_CAND_CAP", "16")
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    info = ix.range_forest_info()
    assert info == {"batch": Q.shape[0], "rows_live": NB, "trees": 3, "probe": 1, "path": 2, "redone": 1, "visits": walk.visits,
                    "leaf_rows": walk.leaf_rows, "hits": want[1].size, "candidates": 0, "launches": info["launches"], "tiles": walk.tiles}, info
    same(got, want)
    monkeypatch.setenv("ZH_FRANGE_CAND_CAP", "1000000")  # room for everything
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk)
    assert ix.range_forest_info()["redone"] == 0
    same(got, want)


# ---------------------------------------------------------------- 10. capacity
@pytest.mark.parametrize("path", [1, 2])
def test_capacity(za, monkeypatch, path):
    from zebra_amd import _ffi
    ix, X, _ = built("B")
    m = za.L2SquaredDistance()
    Q = query_set("B", "b")
    ref = reference("B", "b", 1, 0)
    mk = jth_keys(ref, 30)
    want = within(ref, mk)
    total = want[1].size
    on_path(monkeypatch, path)
    for cap, arrays in ((total - 1, True), (1, True), (0, False)):
        rc, tot, off = raw_call(ix, Q, mk, 1, m, cap, arrays)
        assert rc == ELIMIT and tot == total and (off == want[0]).all(), (cap, rc, tot)
        info = ix.range_forest_info()
        assert info["path"] == path and info["hits"] == total and info["redone"] == 0, info
    rc, tot, off = raw_call(ix, Q, mk, 1, m, total)
    assert rc == 0 and tot == total and (off == want[0]).all()
    same(ix.search_range_forest_batch(Q, metric=m, max_keys=mk, capacity=5), want)  # the wrapper's second call
    P = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    off = np.zeros(Q.shape[0] + 1, np.uint64)
    assert _ffi.lib().zh_search_range_forest_batch(ix._h, P(Q), Q.shape[0], P(mk), 1, m.metric, m.mode, 5, P(off), None, None,
                                                   C.byref(C.c_uint64(0))) == EINVAL


# ---------------------------------------------------------------- 11. more than one internal batch
def test_more_than_one_internal_batch(za, monkeypatch):
    ix, X, _ = built("A")
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    Q = query_set("A", "1061")
    ref = reference("A", "1061", 1, 0)
    walk = walk_of("A", "1061", 1)
    mk = jth_keys(ref, 5)
    got = ix.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
    same(got, within(ref, mk))  # the offsets of 1024 + 37 queries, concatenated
    info = ix.range_forest_info()
    assert info["batch"] == 1061 and info["visits"] == walk.visits and info["leaf_rows"] == walk.leaf_rows and info["launches"] == 2, info
    rc, tot, off = raw_call(ix, Q, mk, 1, m, 7)  # the capacity runs out inside the first internal batch: every offset still exact
    assert rc == ELIMIT and tot == got[1].size and (off == got[0]).all()


# ---------------------------------------------------------------- 12. the device entry point and the siblings
def test_device_entry_point_and_siblings(za, monkeypatch):
    import torch
    ix, X, _ = built("B")
    Q = query_set("B", "b")
    b = Q.shape[0]
    m = za.L2SquaredDistance()
    ref = reference("B", "b", 1, 0)
    mk = jth_keys(ref, 30)
    want = within(ref, mk)
    total = want[1].size
    on_path(monkeypatch, 2)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    mask = np.zeros(NB, bool)
    mask[::2] = True
    Q8 = zo.synth_queries(8, DB, NB)
    ix.search_exact_batch(Q8, 10, m)
    ix.search_exact_filtered_batch(Q8, 10, m, mask)
    ix.search_range_batch(Q8, 1.0, m)
    ix.self_join_count(metric=m, max_key=np.uint64(0))
    ix.knn_graph(10, m, 0, 64)
    ix.knn_graph_forest(10, m, 0, 64)
    ix.self_join_forest_count(metric=m, max_key=np.uint64(0))
    searched = ix.search_batch(Q8, 10, m)
    siblings = lambda: (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.knn_info(), ix.knn_forest_info(),  # noqa: E731
                        ix.join_forest_info(), ix.stats())
    before = siblings()
    dev = torch.device("cuda", 0)
    cap = total + 100
    dq = torch.from_numpy(Q).to(dev)
    dmk = torch.from_numpy(mk.view(np.int64)).to(dev)
    off = torch.full((b + 1,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    keys = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ix.search_range_forest_batch_device(dq.data_ptr(), b, dmk.data_ptr(), 1, m, cap, off.data_ptr(), ids.data_ptr(), keys.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize()
    assert int(tot.item()) == total and ix.range_forest_info()["path"] == 2
    same((off.cpu().numpy().view(np.uint64),) + tuple(t.cpu().numpy().view(np.uint64)[:total] for t in (ids, keys)), want)
    assert (ids.cpu().numpy()[total:] == -7).all() and (keys.cpu().numpy()[total:] == -7).all()
    off.fill_(-7)
    with pytest.raises(za.ZhError) as e:
        ix.search_range_forest_batch_device(dq.data_ptr(), b, dmk.data_ptr(), 1, m, total - 1, off.data_ptr(), ids.data_ptr(), keys.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == ELIMIT and int(tot.item()) == total and (off.cpu().numpy().view(np.uint64) == want[0]).all()
    tot.zero_()
    off.fill_(-7)
    with pytest.raises(za.ZhError) as e:  # count only
        ix.search_range_forest_batch_device(dq.data_ptr(), b, dmk.data_ptr(), 1, m, 0, off.data_ptr(), None, None, tot.data_ptr())
    assert e.value.code == ELIMIT and int(tot.item()) == total and (off.cpu().numpy().view(np.uint64) == want[0]).all()
    assert siblings() == before
    again = ix.search_batch(Q8, 10, m)
    assert all((x == y).all() for x, y in zip(again, searched))


# ---------------------------------------------------------------- 13. the database
def test_database_query_vectors_within_forest(za):
    X = zo.synth_rows(60, 30)[:50].copy()
    X[40:45] = X[3:8]
    docs = ["doc%d" % i for i in range(50)]
    db = za.Database(30, za.L2Distance, za.LSHIndexOptions(16, 4), device=0)
    assert db.query_vectors_within_forest(X[:2], 0.5) == {}
    db.insert_records(X, docs)
    db.remove([7])
    Q = np.ascontiguousarray(X[[3, 4, 7, 20]])
    radius = 0.9
    walk = Walk(X, 16, db.index.get_forest(), Q, 1)
    ref = within(keyed(X, Q, walk, zo.L2, 0), za.radius_key(db.metric, radius))
    got = db.query_vectors_within_forest(Q, radius)
    assert list(got) == [0, 1, 2, 3]
    for i in range(4):
        ids = ref[1][int(ref[0][i]):int(ref[0][i + 1])].tolist()
        assert list(got[i].items()) == [(int(j), docs[int(j)]) for j in ids]
    exact = db.query_vectors_within(Q, radius)
    assert all(set(got[i].items()) <= set(exact[i].items()) for i in range(4))
    assert 3 in got[0] and 40 in got[0] and 7 not in got[2] and sum(len(v) for v in got.values()) >= 6
    got2 = db.query_vectors_within_forest(Q, radius, probe=16)
    assert all(set(got[i].items()) <= set(got2[i].items()) for i in range(4))

"""The forest k-NN graph (zh_knn_graph_forest): line i of a slab holds the first k by (key, id) of C(a), a = first_row + i: the union over the trees
of the members of a's leaf, minus a itself.  The reference is built here from ix.get_forest() -- each reachable leaf's run of leaf_ids gives C(a) --
and the oracle: distance_batch(X[C], X[a]), a lexsort by (key, id), the first k.  Every comparison is bit for bit on ids, keys and counts.  The index
is filled with add, so that it is built.  Shapes (module docstring of each fixture) are the smallest that reach each mechanism: leaves that are no
multiple of 16, leaves under 16 rows, empty leaves, a leaf longer than max_node_size, a leaf longer than one window of held rows, several trees."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

NONE = np.uint64(2**64 - 1)
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
def forest_leaves(f):
    """per tree the leaves reachable from its root, as runs of leaf_ids"""
    out = []
    for root in f["roots"].tolist():
        leaves, st = [], [root]
        while st:
            nd = st.pop()
            if f["plane"][nd] >= 0:
                st += [int(f["right"][nd]), int(f["left"][nd])]
            else:
                off, ln = int(f["left"][nd]), int(f["right"][nd])
                leaves.append(f["leaf_ids"][off:off + ln].astype(np.int64))
        out.append(leaves)
    return out


def candidates(f, n):
    """C(a) for every stored row a < n (ascending, a itself out; a row no tree holds: empty) and the info's `pairs` for the slab of all rows"""
    per = [[] for _ in range(n)]
    pairs = 0
    for leaves in forest_leaves(f):
        for ids in leaves:
            pairs += ids.size * (ids.size - 1)
            for a in ids.tolist():
                per[a].append(ids)
    C = []
    for a in range(n):
        c = np.unique(np.concatenate(per[a])) if per[a] else np.zeros(0, np.int64)
        C.append(c[c != a])
    return C, pairs, sum(1 for p in per if p)


def ranked(X, C, rows, om, omode, id_base=0):
    """per row a of `rows`: (ids, keys) of ALL of C(a) by (key, id) -- the first k of it is the line at any k"""
    out = {}
    for a in rows:
        c = C[a]
        ks = np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[c]), X[a]), np.uint64) if c.size else np.zeros(0, np.uint64)
        o = np.lexsort((c, ks))
        out[a] = (c[o].astype(np.uint64) + np.uint64(id_base), ks[o])
    return out


def check_lines(got, ref, k, first_row=0):
    ids, keys, counts = got
    assert ids.dtype == np.uint64 and keys.dtype == np.uint64 and counts.dtype == np.uint32
    for a, (rid, rkey) in ref.items():
        i, c = a - first_row, min(k, rid.size)
        assert counts[i] == c, (a, counts[i], c)
        assert (ids[i, :c] == rid[:c]).all() and (keys[i, :c] == rkey[:c]).all(), a
        assert (ids[i, c:] == NONE).all() and (keys[i, c:] == NONE).all(), a


def same(got, ref):
    for g, r, what in zip(got, ref, ("ids", "keys", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), what


def no_own_id(got, id_base=0, first_row=0):
    ids = got[0]
    return not (ids == (np.arange(first_row, first_row + ids.shape[0], dtype=np.uint64) + np.uint64(id_base))[:, None]).any()


def on_path(monkeypatch, path):
    monkeypatch.delenv("ZH_FKNN_LIST_CAP", raising=False)
    if path == 1:
        monkeypatch.setenv("ZH_FKNN_PATH", "1")
    else:
        monkeypatch.delenv("ZH_FKNN_PATH", raising=False)


# ---------------------------------------------------------------- shapes (an index per shape, shared; no test changes one)
_SHARED = {}  # the shared indexes, closed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()


@functools.lru_cache(maxsize=None)
def rows_a():
    return zo.synth_rows(1500, 30)


@functools.lru_cache(maxsize=None)
def rows_b(d=DB):
    return zo.synth_rows(NB, d)


@functools.lru_cache(maxsize=None)
def rows_bdup():
    X = rows_b().copy()
    X[1000:1400] = X[1000]  # 400 bit-identical rows: one unsplittable leaf of 400 at max_node_size 256, many tiny and empty leaves around it
    return X


@functools.lru_cache(maxsize=None)
def rows_c():
    return zo.synth_rows(2000, 30)


def built(name):
    """(index, X, C, pairs, lines) of a shape, the index filled with add"""
    import zebra_amd as za
    if name in _SHARED:
        return _SHARED[name]
    X, d, opts = {"A": (rows_a(), 30, (64, 4)), "B": (rows_b(), DB, (256, 3)), "Bdup": (rows_bdup(), DB, (256, 3)), "C": (rows_c(), 30, (5, 15)),
                  "one": (zo.synth_rows(8192 + 37, DB), DB, (16384, 1))}[name]
    ix = za.LSHIndex(d, za.LSHIndexOptions(*opts), device=0)
    ix.add(X)
    C, pairs, lines = candidates(ix.get_forest(), X.shape[0])
    _SHARED[name] = (ix, X, C, pairs, lines)
    return _SHARED[name]


@functools.lru_cache(maxsize=None)
def reference(name, mi):
    import zebra_amd as za
    _, X, C, _, _ = built(name)
    _, om, omode = thirteen_metrics(za)[mi]
    return ranked(X, C, range(X.shape[0]), om, omode)


# ---------------------------------------------------------------- path 1
@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, monkeypatch, mi):
    ix, X, C, pairs, lines = built("A")
    n, k = X.shape[0], 10
    on_path(monkeypatch, 2)  # (d = 30: the path rule itself chooses path 1)
    got = ix.knn_graph_forest(k, thirteen_metrics(za)[mi][0])
    info = ix.knn_forest_info()
    assert info == {"rows_live": n, "lines": n, "k": k, "path": 1, "trees": 4, "pairs": pairs, "survivors": 0, "redone": 0,
                    "launches": info["launches"], "tiles": 0}, info
    assert min(c.size for c in C) >= 65  # (the shape: every line has more than k candidates)
    assert (got[2] == k).all() and no_own_id(got)
    check_lines(got, reference("A", mi), k)


def test_path1_largest_k(za, monkeypatch):
    ix, X, C, _, _ = built("A")
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(1023, thirteen_metrics(za)[0][0])
    assert (got[2] == np.array([c.size for c in C])).all() and no_own_id(got)  # |C(a)| <= 223 < k: every candidate, the tails filled
    check_lines(got, reference("A", 0), 1023)
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_forest(1024, thirteen_metrics(za)[0][0])
    assert e.value.code == ELIMIT


@pytest.mark.parametrize("k", [10, 64])
def test_default_regime(za, monkeypatch, k):
    """max_node_size 5, 15 trees: thousands of leaves of 0 .. 4 rows"""
    ix, X, C, pairs, lines = built("C")
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(k, thirteen_metrics(za)[0][0])
    info = ix.knn_forest_info()
    assert info["path"] == 1 and info["trees"] == 15 and info["pairs"] == pairs and info["lines"] == X.shape[0], info
    sizes = np.array([c.size for c in C])
    assert (got[2] == np.minimum(sizes, k)).all() and no_own_id(got)
    if k == 64:
        assert (got[2] == sizes).all()  # |C(a)| <= 42
    check_lines(got, reference("C", 0), k)


def test_small_and_empty_indexes(za, monkeypatch):
    X = rows_a()
    m = thirteen_metrics(za)[0][0]
    on_path(monkeypatch, 2)
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ids, keys, counts = ix.knn_graph_forest(5, m)  # an empty index: no lines, nothing asked of the forest
    assert ids.shape == (0, 5) and counts.shape == (0,)
    ix.append(X[:3])
    with pytest.raises(za.ZhError) as e:  # rows, but no trees
        ix.knn_graph_forest(5, m)
    assert e.value.code == ESTATE
    ids, keys, counts = ix.knn_graph_forest(0, m)  # k = 0 is judged first
    assert ids.shape == (3, 0) and (counts == 0).all() and ix.knn_forest_info()["k"] == 0
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.add(X[:1])
    ids, keys, counts = ix.knn_graph_forest(5, m)  # one row: a leaf-mate of nobody
    assert counts.tolist() == [0] and (ids == NONE).all() and (keys == NONE).all()
    assert ix.knn_forest_info()["lines"] == 1 and ix.knn_forest_info()["pairs"] == 0
    ix.add(X[1:40])
    got = ix.knn_graph_forest(64, m)  # 40 rows in one leaf per tree, k = 64: 39 neighbours each
    assert (got[2] == 39).all() and no_own_id(got)
    C, pairs, _ = candidates(ix.get_forest(), 40)
    check_lines(got, ranked(X, C, range(40), zo.L2SQ, 0), 64)
    ix.remove(list(range(40)))
    ids, keys, counts = ix.knn_graph_forest(5, m)  # removed rows only
    assert ids.shape == (40, 5) and (counts == 0).all() and (ids == NONE).all() and (keys == NONE).all()
    info = ix.knn_forest_info()
    assert info["lines"] == 0 and info["rows_live"] == 0 and info["pairs"] == 0, info


# ---------------------------------------------------------------- path 2
def check_path2(za, monkeypatch, name, mi, k):
    ix, X, C, pairs, lines = built(name)
    n = X.shape[0]
    m = thirteen_metrics(za)[mi][0]
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(k, m)
    info = ix.knn_forest_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live"] == n and info["lines"] == lines and info["k"] == k, info
    assert info["pairs"] == pairs and info["tiles"] * 256 >= pairs and info["tiles"] * 4 < ((n + 15) // 16) ** 2, info  # block-diagonal work
    assert no_own_id(got)
    check_lines(got, reference(name, mi), k)
    same(ix.knn_graph_forest(k, m), got)  # twice: identical
    on_path(monkeypatch, 1)
    forced = ix.knn_graph_forest(k, m)
    info = ix.knn_forest_info()
    assert info["path"] == 1 and info["tiles"] == 0 and info["survivors"] == 0 and info["pairs"] == pairs, info
    same(forced, got)
    return got


@pytest.mark.parametrize("mi", range(4))
@pytest.mark.parametrize("k", [1, 10, 100])
def test_path2_against_the_oracle_and_path1(za, monkeypatch, mi, k):
    check_path2(za, monkeypatch, "B", mi, k)


@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    X = rows_b(d)
    ix = za.LSHIndex(d, za.LSHIndexOptions(256, 3), device=0)
    ix.add(X)
    C, pairs, lines = candidates(ix.get_forest(), NB)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(10, m)
    info = ix.knn_forest_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["pairs"] == pairs and info["lines"] == lines, info
    check_lines(got, ranked(X, C, range(NB), zo.L2SQ, 0), 10)
    on_path(monkeypatch, 1)
    same(ix.knn_graph_forest(10, m), got)
    ix.close()


@pytest.mark.parametrize("mi", [0, 2])
def test_odd_leaves(za, monkeypatch, mi):
    """400 bit-identical rows: one leaf of 400 at max_node_size 256, leaves under 16 rows and empty leaves around it"""
    ix, X, C, _, _ = built("Bdup")
    lens = [ids.size for leaves in forest_leaves(ix.get_forest()) for ids in leaves]
    assert max(lens) >= 400 and min(lens) == 0 and sum(1 for v in lens if 0 < v < 16) > 0  # (the shape)
    got = check_path2(za, monkeypatch, "Bdup", mi, 10)
    if mi == 0:
        assert got[0][1203, :4].tolist() == [1000, 1001, 1002, 1003] and (got[1][1203, :4] == 0).all()


NEAR = [(i, 100 + i) for i in range(60)]
PLANTED = sorted(set([i for i, _ in NEAR] + [j for _, j in NEAR] + list(range(200, 220)) + list(range(300, 320)) + list(range(400, 420)) +
                     list(range(500, 510)) + [600]))


@functools.lru_cache(maxsize=None)
def planted_rows():
    """tests/test_gpu_knn.py's planted rows, restated"""
    X = rows_b().copy()
    for i, j in NEAR:  # near-duplicates below fp16 resolution: the copy's two rows are the same halves, only the canonical key orders them
        X[j] = X[i] * np.float32(1.0 + 2.0**-12)
    X[200:220] = X[300:320]  # 20 bit-identical pairs
    X[400:410] *= np.float32(2.0**40)
    X[410:420] *= np.float32(2.0**-40)
    X[500:510] = np.round(X[500:510] * 100.0)  # integer-valued rows
    X[600] = 0.0
    return X


def planted_index(uncertain):
    import zebra_amd as za
    if ("planted", uncertain) in _SHARED:
        return _SHARED[("planted", uncertain)]
    X = planted_rows().copy()
    if uncertain:  # one row with an infinite element and one whose |x|^2 overflows: nothing certain means always listed
        X[700, 5] = np.inf
        X[701] = np.float32(1e30)
    ix = za.LSHIndex(DB, za.LSHIndexOptions(256, 3), device=0)
    ix.add(X)
    _SHARED[("planted", uncertain)] = (ix, X, candidates(ix.get_forest(), NB)[0])
    return _SHARED[("planted", uncertain)]


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    ix, X, C = planted_index(False)
    m, om, omode = thirteen_metrics(za)[mi]
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(10, m)
    assert ix.knn_forest_info()["path"] == 2 and ix.knn_forest_info()["redone"] == 0
    check_lines(got, ranked(X, C, PLANTED, om, omode), 10)
    on_path(monkeypatch, 1)
    same(ix.knn_graph_forest(10, m), got)


@pytest.mark.parametrize("mi", [0, 3])
def test_rows_nothing_is_certain_about(za, monkeypatch, mi):
    """path 2 against path 1: the device's own arithmetic on both sides (a NaN's sign differs between host and GPU)"""
    ix, X, C = planted_index(True)
    m = thirteen_metrics(za)[mi][0]
    on_path(monkeypatch, 2)
    got = ix.knn_graph_forest(10, m)
    assert ix.knn_forest_info()["path"] == 2
    on_path(monkeypatch, 1)
    same(ix.knn_graph_forest(10, m), got)


# ---------------------------------------------------------------- both paths
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("mi", [0, 2])
def test_one_leaf_equals_the_exact_graph(za, monkeypatch, path, mi):
    """one tree whose root is a leaf of 8229 rows: C(a) is every other row.  Also the long-leaf case: three windows of held rows, 515 column tiles"""
    ix, X, C, pairs, lines = built("one")
    n = X.shape[0]
    assert pairs == n * (n - 1) and lines == n
    m = thirteen_metrics(za)[mi][0]
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    exact = ix.knn_graph(10, m)
    on_path(monkeypatch, path)
    got = ix.knn_graph_forest(10, m)
    info = ix.knn_forest_info()
    assert info["path"] == path and info["redone"] == 0 and info["pairs"] == pairs, info
    if path == 2:
        assert info["tiles"] == ((n + 15) // 16) ** 2 and info["launches"] == 3, info
    same(got, exact)


@pytest.mark.parametrize("path", [1, 2])
def test_never_nearer_than_exact(za, monkeypatch, path):
    ix, X, C, _, _ = built("B")
    m = za.L2SquaredDistance()
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    exact = ix.knn_graph(10, m)
    on_path(monkeypatch, path)
    ids, keys, counts = ix.knn_graph_forest(10, m)
    assert (counts == 10).all() and (exact[2] == 10).all()
    for a in range(NB):
        assert np.isin(ids[a].astype(np.int64), C[a]).all(), a
    assert (keys >= exact[1]).all()  # entry for entry, in the keys' unsigned order


@pytest.mark.parametrize("path", [1, 2])
def test_mutations(za, monkeypatch, path):
    base = 1 << 40
    extra = zo.synth_rows(NB + 350, DB)[NB:]
    X = rows_b()
    k = 10
    m, om, omode = thirteen_metrics(za)[0]
    on_path(monkeypatch, path)
    ix = za.LSHIndex(DB, za.LSHIndexOptions(256, 3), device=0, id_base=base)
    ix.add(X)

    def step(rows, dead, outside=()):
        """the whole graph against the oracle on the forest as it is now; `outside`: rows no tree holds"""
        n = rows.shape[0]
        C, pairs, lines = candidates(ix.get_forest(), n)
        got = ix.knn_graph_forest(k, m)
        info = ix.knn_forest_info()
        assert info["path"] == path and info["redone"] == 0 and info["pairs"] == pairs and info["lines"] == lines, info
        assert info["rows_live"] == n - len(dead)
        check_lines(got, ranked(rows, C, range(n), om, omode, base), k)
        for r in list(dead) + list(outside):
            assert got[2][r] == 0
        gone = np.array(list(dead) + list(outside), np.uint64) + np.uint64(base)
        assert not np.isin(got[0], gone).any() and no_own_id(got, base)
        return got

    gone = list(range(80, 96, 3)) + list(range(112, 128)) + [NB - 1]  # every third row of a tile, one whole tile, the last row
    ix.remove([g + base for g in gone])
    step(X, gone)
    ix.add(extra[:300])  # they descend the trees and split leaves
    X1 = np.concatenate([X, extra[:300]])
    step(X1, gone)
    ix.append(extra[300:])  # in no tree: count 0, nobody's neighbour
    X2 = np.concatenate([X1, extra[300:]])
    n2 = X2.shape[0]
    step(X2, gone, outside=range(n2 - 50, n2))
    ix.build()  # ... and now they take part
    got = step(X2, gone)
    assert (got[2][n2 - 50:] == k).all()
    live = np.array([r for r in range(n2) if r not in set(gone)])
    new_ids, _ = ix.compact()
    after = ix.knn_graph_forest(k, m)
    assert after[0].shape == (live.size, k)
    new_rows = (new_ids[live] - np.uint64(base)).astype(np.int64)
    assert (after[0][new_rows] == new_ids[(got[0][live] - np.uint64(base)).astype(np.int64)]).all()  # the old answer under the id map
    assert (after[1][new_rows] == got[1][live]).all() and (after[2][new_rows] == got[2][live]).all()
    ix.close()


def test_scan_order_that_is_not_id_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): leaves are gathered by row number, the answer is the plain index's"""
    X = rows_b()
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    plain = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    plain.add(X)
    ref = plain.knn_graph_forest(10, m)
    assert plain.knn_forest_info()["path"] == 2
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, DB, NB), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    assert zo.canonical_forest(ix.get_forest(), DB) == zo.canonical_forest(plain.get_forest(), DB)  # the same forest
    got = ix.knn_graph_forest(10, m)
    info = ix.knn_forest_info()
    assert info["path"] == 2 and info["redone"] == 0, info
    same(got, ref)
    C, _, _ = candidates(ix.get_forest(), NB)
    sample = list(range(0, NB, 41))
    check_lines(got, ranked(X, C, sample, zo.L2SQ, 0), 10)
    ix.close()
    plain.close()


@pytest.mark.parametrize("path", [1, 2])
def test_slabs(za, monkeypatch, path):
    ix, X, C, pairs, _ = built("B")
    m = za.L2SquaredDistance()
    on_path(monkeypatch, path)
    whole = ix.knn_graph_forest(10, m)
    parts = [ix.knn_graph_forest(10, m, 0, 1000), ix.knn_graph_forest(10, m, 1000, 2048), ix.knn_graph_forest(10, m, 3048)]
    info = ix.knn_forest_info()
    assert info["path"] == path and info["lines"] == NB - 3048, info
    assert info["pairs"] == sum(ids.size - 1 for leaves in forest_leaves(ix.get_forest()) for ids in leaves for a in ids.tolist() if a >= 3048)
    same(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), whole)
    mid = ix.knn_graph_forest(10, m, 8, 100)  # starts in the middle of a tile
    assert ix.knn_forest_info()["lines"] == 100 and no_own_id(mid, first_row=8)
    same(mid, tuple(w[8:108] for w in whole))
    same(ix.knn_graph_forest(10, m, NB, 0), tuple(w[:0] for w in whole))
    for first, n in ((NB - 5, 6), (NB + 1, 1), (0, NB + 1)):
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_forest(10, m, first, n)
        assert e.value.code == EINVAL


def test_list_overflow_is_redone_by_path1(za, monkeypatch):
    ix, X, C, pairs, _ = built("B")
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    ref = ix.knn_graph_forest(10, m)
    assert ix.knn_forest_info()["redone"] == 0
    monkeypatch.setenv("ZH_FKNN_LIST_CAP", "16")  # the first tree lists every leaf-mate of a line: leaves of 27 rows and more run over
    got = ix.knn_graph_forest(10, m)
    info = ix.knn_forest_info()
    assert info["path"] == 2 and info["redone"] == 1 and info["lines"] == NB and info["pairs"] == pairs, info  # (one sub-slab holds every line)
    same(got, ref)


def test_device_entry_point_and_siblings(za, monkeypatch):
    import torch
    ix, X, C, _, _ = built("B")
    Q = zo.synth_queries(8, DB, NB)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    mask = np.zeros(NB, bool)
    mask[::2] = True
    ix.knn_graph_forest(10, m)
    ix.search_exact_batch(Q, 10, m)
    ix.search_exact_filtered_batch(Q, 10, m, mask)
    ix.search_range_batch(Q, 1.0, m)
    ix.self_join_count(metric=m, max_key=np.uint64(0))
    ix.knn_graph(10, m, 0, 64)
    before = (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.knn_info(), ix.stats())
    host = ix.knn_graph_forest(10, m, 500, 3000)
    dev = torch.device("cuda", 0)
    ids = torch.zeros((3000, 10), dtype=torch.int64, device=dev)
    keys = torch.zeros_like(ids)
    counts = torch.full((3000,), 7, dtype=torch.int32, device=dev)
    ix.knn_graph_forest_device(10, m, 500, 3000, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    assert ix.knn_forest_info()["path"] == 2 and ix.knn_forest_info()["lines"] == 3000
    same((ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)), host)
    ids.fill_(-7)
    ix.knn_graph_forest_device(0, m, 500, 3000, None, None, counts.data_ptr())  # k = 0: the counts alone
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 0).all() and (ids.cpu().numpy() == -7).all()
    assert (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.knn_info(), ix.stats()) == before


def test_database_knn_graph_forest(za):
    X = rows_a()[:50]
    docs = ["doc%d" % i for i in range(50)]
    db = za.Database(30, za.L2Distance, za.LSHIndexOptions(16, 4), device=0)
    db.insert_records(X, docs)
    db.remove([7])
    live = [r for r in range(50) if r != 7]
    graph = db.knn_graph_forest(3)
    assert sorted(graph) == sorted(docs[r] for r in live)
    C, _, _ = candidates(db.index.get_forest(), 50)
    ref = ranked(X, C, live, zo.L2, 0)
    for a in live:
        rid, rkey = ref[a]
        assert [d for d, _ in graph[docs[a]]] == [docs[int(i)] for i in rid[:3]]
        assert [v for _, v in graph[docs[a]]] == zo.key_to_float(rkey[:3]).tolist()


@pytest.mark.parametrize("name", ["l2sq", "cos_corrected"])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, name):
    """the held-tile walk (zh_device.h) at its edges, against the family fuzz's reference: one tree whose root is a leaf of 1040 rows = 65 column
    tiles, a slab of 17 lines = two held tiles, the second with one line: two waves of the one held block that has lines are idle.  So small a
    launch walks chunks of 8 column tiles (fill_chunk): eight full chunks (even: the last tile in the second LDS buffer) and a chunk of ONE
    tile (odd, no prefetch at all).  A near-duplicate of a line is planted in that last tile"""
    from tests import family_cases as fc
    n, k, first = 1040, 10, 500
    spec = fc.metric_spec(name)
    m = za.L2SquaredDistance() if name == "l2sq" else za.CosineDistance(parity=False)
    X = zo.synth_rows(n, DB).copy()
    X[1033] = X[first + 16] * np.float32(1.0 + 2.0**-12)
    slab = np.arange(first, first + 17)
    ref = fc.graph_ref(fc.key_matrix(spec, X, X[slab]), slab, np.ones(n, bool), k, 0, mates=np.ones((17, n), bool))
    assert ref[0][16, 0] == 1033
    ix = za.LSHIndex(DB, za.LSHIndexOptions(16384, 1), device=0)
    ix.add(X)
    monkeypatch.delenv("ZH_FKNN_PATH", raising=False)
    monkeypatch.delenv("ZH_FKNN_LIST_CAP", raising=False)
    got = ix.knn_graph_forest(k, m, first, 17)
    info = ix.knn_forest_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["lines"] == 17 and info["trees"] == 1 and info["tiles"] == 2 * 65, info
    for g, r, what in zip(got, ref, ("ids", "keys", "counts")):
        assert g.shape == r.shape and (g == r).all(), what
    ix.close()

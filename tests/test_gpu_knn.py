"""The exact k-NN graph (zh_knn_graph): line i of a slab holds the exact top-k by (key, id) of stored row first_row + i over every live row except
that row itself, the key being the one of stored row b against a query equal to the line's f32 row.  The reference is built here from the oracle
(oracle.distance_batch(X[others], X[a]), lexsorted by (key, id), first k); at the path-2 shape every line is also compared against
search_exact_batch(X, k + 1) with the line's own id taken out (test_gpu_exact.py pins that call to the oracle).  Every comparison is bit for bit on
ids, keys and counts.  Data are finite (a NaN's sign differs between host and GPU, as test_gpu_exact notes) except in the one case that says
otherwise.  Shapes are the smallest that reach each mechanism: path 2 wants 8192 live rows at d >= 256; 8192 + 37 rows are 515 tiles, the last one
partial, nine panels, the last of 37 lines (a partial block of held tiles), and two column launches (4096 positions, then the rest)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

NONE = np.uint64(2**64 - 1)
EINVAL, ELIMIT = -1, -5
N2, D2 = 8192 + 37, 256
T2 = (N2 + 15) // 16


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


def oracle_lines(X, live, a_list, om, omode, k, id_base=0):
    """per live row a of a_list: (ids, keys) of its first k other live rows by (key, id), from the oracle"""
    out = []
    for a in a_list:
        others = live[live != a]
        ks = np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[others]), X[a]), np.uint64) if others.size else np.zeros(0, np.uint64)
        o = np.lexsort((others, ks))[:k]
        out.append((others[o].astype(np.uint64) + np.uint64(id_base), ks[o]))
    return out


def check_lines(got, lines, ref, k):
    """`lines`: the indices into got of the rows ref speaks of, in ref's order"""
    ids, keys, counts = got
    assert ids.dtype == np.uint64 and keys.dtype == np.uint64 and counts.dtype == np.uint32
    for i, (rid, rkey) in zip(lines, ref):
        c = rid.size
        assert counts[i] == c, (i, counts[i], c)
        assert (ids[i, :c] == rid).all() and (keys[i, :c] == rkey).all(), i
        assert (ids[i, c:] == NONE).all() and (keys[i, c:] == NONE).all(), i


def same(got, ref):
    for g, r, what in zip(got, ref, ("ids", "keys", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), what


def drop_self(ids, keys, counts, own, k):
    """a [b][k + 1] answer of the exact search with each line's own id taken out -> [b][k]"""
    mine = ids == own[:, None]
    order = np.argsort(mine, axis=1, kind="stable")  # the own id (at most one per line) goes last, everything else keeps its order
    oi, ok = np.take_along_axis(ids, order, 1)[:, :k], np.take_along_axis(keys, order, 1)[:, :k]
    oc = np.minimum(counts - mine.any(axis=1), k).astype(np.uint32)
    return np.ascontiguousarray(oi), np.ascontiguousarray(ok), oc


def exact_reference(ix, X, live, k, m, id_base=0):
    """search_exact_batch over the live rows as queries with k + 1, self taken out -> the graph's lines of the live rows"""
    ids, keys, counts = ix.search_exact_batch(np.ascontiguousarray(X[live]), k + 1, m)
    return drop_self(ids, keys, counts, live.astype(np.uint64) + np.uint64(id_base), k)


def no_own_id(got, id_base=0):
    ids = got[0]
    return not (ids == (np.arange(ids.shape[0], dtype=np.uint64) + np.uint64(id_base))[:, None]).any()


# ---------------------------------------------------------------- path 1
@functools.lru_cache(maxsize=None)
def small_rows():
    return zo.synth_rows(1500, 30)


@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, mi):
    X = small_rows()
    n, k = X.shape[0], 10
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = ix.knn_graph(k, m)
    info = ix.knn_info()
    assert info == {"rows_live": n, "lines": n, "k": k, "path": 1, "redone": 0, "survivors": 0, "launches": info["launches"], "tiles": 0}, info
    assert (got[2] == k).all() and no_own_id(got)
    rows = np.arange(n)
    check_lines(got, rows, oracle_lines(X, rows, rows.tolist(), om, omode, k), k)


def test_path1_largest_k(za):
    X = small_rows()
    n, k = X.shape[0], 1023
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = ix.knn_graph(k, m)
    assert ix.knn_info()["path"] == 1 and (got[2] == k).all() and no_own_id(got)
    sample = [0, 1, 511, 1024, n - 1]
    check_lines(got, sample, oracle_lines(X, np.arange(n), sample, om, omode, k), k)
    from zebra_amd import _ffi
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph(1024, m)
    assert e.value.code == _ffi.ZH_ELIMIT


def test_small_and_empty_indexes(za):
    X = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ids, keys, counts = ix.knn_graph(5, m)  # an empty index: no lines
    assert ids.shape == (0, 5) and counts.shape == (0,)
    ix.append(X[:1])
    ids, keys, counts = ix.knn_graph(5, m)  # one live row: nothing else to name
    assert counts.tolist() == [0] and (ids == NONE).all() and (keys == NONE).all()
    assert ix.knn_info()["lines"] == 1
    ix.append(X[1:40])
    got = ix.knn_graph(64, m)  # 40 rows, k = 64: 39 neighbours each, the tails filled
    assert (got[2] == 39).all() and no_own_id(got)
    rows = np.arange(40)
    check_lines(got, rows, oracle_lines(X, rows, rows.tolist(), om, omode, 64), 64)
    ids, keys, counts = ix.knn_graph(0, m)  # k = 0
    assert ids.shape == (40, 0) and (counts == 0).all() and ix.knn_info()["k"] == 0
    ix.remove(list(range(40)))
    ids, keys, counts = ix.knn_graph(5, m)  # removed rows only
    assert ids.shape == (40, 5) and (counts == 0).all() and (ids == NONE).all() and (keys == NONE).all()
    assert ix.knn_info()["lines"] == 0 and ix.knn_info()["rows_live"] == 0


@pytest.mark.parametrize("mi", [0, 2])
def test_duplicates_are_neighbours(za, mi):
    """8 bit-identical rows at ids 200 .. 207: each one's nearest rows are the other seven, in id order -- "drop the first result" of a k + 1
    search names row 200 for every one of them.  Under the parity cosine key self has the largest key and is not among the first at all."""
    X = small_rows().copy()
    X[200:208] = X[200]
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = ix.knn_graph(4, m)
    assert no_own_id(got)
    if mi == 0:
        assert got[0][203].tolist() == [200, 201, 202, 204] and (got[1][203] == 0).all()
        assert got[0][200].tolist() == [201, 202, 203, 204]
    rows = np.arange(X.shape[0])
    sample = list(range(196, 212))
    check_lines(got, sample, oracle_lines(X, rows, sample, om, omode, 4), 4)


# ---------------------------------------------------------------- path 2
@functools.lru_cache(maxsize=None)
def wide_rows(d):
    return zo.synth_rows(N2, d)


SAMPLE = np.sort(np.random.default_rng(7).choice(N2, 128, replace=False)).tolist()


def check_path2(za, ix, X, m, om, omode, k, monkeypatch, sample=SAMPLE, oracle=True):
    n = X.shape[0]
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    monkeypatch.delenv("ZH_KNN_LIST_CAP", raising=False)
    got = ix.knn_graph(k, m)
    info = ix.knn_info()
    T = (n + 15) // 16
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live"] == n and info["lines"] == n and info["k"] == k, info
    assert info["tiles"] == T * T, info  # the full rectangle (from the launch geometry)
    assert info["survivors"] >= n * k and info["launches"] == 2 * ((n + 1023) // 1024), info
    assert (got[2] == k).all() and no_own_id(got)
    rows = np.arange(n)
    same(got, exact_reference(ix, X, rows, k, m))
    if oracle:
        check_lines(got, sample, oracle_lines(X, rows, sample, om, omode, k), k)
    same(ix.knn_graph(k, m), got)  # twice: identical
    monkeypatch.setenv("ZH_KNN_PATH", "1")
    forced = ix.knn_graph(k, m)
    info = ix.knn_info()
    assert info["path"] == 1 and info["tiles"] == 0 and info["survivors"] == 0 and info["redone"] == 0, info
    same(forced, got)
    monkeypatch.delenv("ZH_KNN_PATH")
    return got


@pytest.mark.parametrize("mi", range(4))
def test_path2_against_the_exact_search_and_the_oracle(za, monkeypatch, mi):
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    check_path2(za, ix, X, m, om, omode, 10, monkeypatch)


@pytest.mark.parametrize("k", [1, 100])
def test_path2_other_k(za, monkeypatch, k):
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    check_path2(za, ix, X, m, om, omode, k, monkeypatch)


@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    X = wide_rows(d)
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    check_path2(za, ix, X, m, om, omode, 10, monkeypatch)


# ---------------------------------------------------------------- adversarial rows (test_gpu_join.py's planted set, restated)
NEAR = [(i, 100 + i) for i in range(60)]


@functools.lru_cache(maxsize=None)
def planted_rows():
    X = wide_rows(D2).copy()
    for i, j in NEAR:  # near-duplicates below fp16 resolution: the copy's two rows are the same halves, only the canonical key orders them
        X[j] = X[i] * np.float32(1.0 + 2.0**-12)
    X[200:220] = X[300:320]  # 20 bit-identical pairs
    X[400:410] *= np.float32(2.0**40)
    X[410:420] *= np.float32(2.0**-40)
    X[500:510] = np.round(X[500:510] * 100.0)  # integer-valued rows
    X[600] = 0.0
    return X


PLANTED = sorted(set([i for i, _ in NEAR] + [j for _, j in NEAR] + list(range(200, 220)) + list(range(300, 320)) + list(range(400, 420)) +
                     list(range(500, 510)) + [600]))


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    X = planted_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = check_path2(za, ix, X, m, om, omode, 10, monkeypatch, sample=PLANTED)
    if mi == 0:  # a bit-identical pair: each is the other's nearest, at key 0
        assert got[0][200, 0] == 300 and got[0][300, 0] == 200 and got[1][200, 0] == 0


def test_rows_nothing_is_certain_about(za, monkeypatch):
    """one row with an infinite element and one whose |x|^2 overflows: nothing certain means always listed, and the canonical key decides.
    Compared against search_exact_batch (the device's own arithmetic on both sides), not the oracle."""
    X = planted_rows().copy()
    X[700, 5] = np.inf
    X[701] = np.float32(1e30)
    for m in (za.L2SquaredDistance(), za.CosineDistance(parity=False)):
        ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
        ix.append(X)
        check_path2(za, ix, X, m, None, None, 10, monkeypatch, oracle=False)


# ---------------------------------------------------------------- removed rows, ids, compaction, row order
def test_removed_rows_id_base_and_compact(za, monkeypatch):
    base = 1 << 40
    X = wide_rows(D2)
    k = 10
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    ix.add(X)
    gone = np.array(list(range(80, 96, 3)) + list(range(112, 128)) + [N2 - 1])  # every third row of a tile, one whole tile, the last row
    ix.remove((gone + base).tolist())
    alive = np.ones(N2, bool)
    alive[gone] = False
    live = np.flatnonzero(alive)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    got = ix.knn_graph(k, m)
    info = ix.knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live"] == live.size and info["lines"] == live.size, info
    assert info["tiles"] == ((live.size + 15) // 16) * T2, info
    assert (got[2][gone] == 0).all() and (got[0][gone] == NONE).all() and (got[1][gone] == NONE).all()
    assert (got[2][live] == k).all()
    assert not np.isin(got[0][live] - np.uint64(base), gone).any() and no_own_id(got, base)
    ref = exact_reference(ix, X, live, k, m, base)
    same((got[0][live], got[1][live], got[2][live]), ref)
    sample = sorted(set([a for a in SAMPLE if alive[a]] + [79, 81, 82, 94, 111, 128, N2 - 3, N2 - 2]))  # ... and the removed rows' tile-mates
    check_lines(got, sample, oracle_lines(X, live, sample, om, omode, k, base), k)
    new_ids, _ = ix.compact()
    after = ix.knn_graph(k, m)
    assert after[0].shape == (live.size, k)
    new_rows = (new_ids[live] - np.uint64(base)).astype(np.int64)
    assert (after[0][new_rows] == new_ids[(got[0][live] - np.uint64(base)).astype(np.int64)]).all()
    assert (after[1][new_rows] == got[1][live]).all() and (after[2][new_rows] == got[2][live]).all()


def test_scan_order_that_is_not_id_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): a panel is defined by row numbers, the answer is the plain index's"""
    X = wide_rows(D2)
    m = za.L2SquaredDistance()
    plain = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    plain.append(X)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    ref = plain.knn_graph(10, m)
    assert plain.knn_info()["path"] == 2
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(D2, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, D2, N2), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    got = ix.knn_graph(10, m)
    info = ix.knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == T2 * T2, info
    same(got, ref)
    ix.close()


# ---------------------------------------------------------------- slabs, overflow, the device entry point
def test_slabs(za, monkeypatch):
    X = wide_rows(D2)
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    whole = ix.knn_graph(10, m)
    parts = [ix.knn_graph(10, m, 0, 1000), ix.knn_graph(10, m, 1000, 4096), ix.knn_graph(10, m, 5096)]
    assert ix.knn_info()["path"] == 2 and ix.knn_info()["lines"] == N2 - 5096
    same(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), whole)
    mid = ix.knn_graph(10, m, 8, 100)  # starts in the middle of a tile
    assert ix.knn_info()["lines"] == 100 and ix.knn_info()["tiles"] == 7 * T2
    same(mid, tuple(w[8:108] for w in whole))
    same(ix.knn_graph(10, m, N2, 0), tuple(w[:0] for w in whole))
    for first, n in ((N2 - 5, 6), (N2 + 1, 1), (0, N2 + 1)):
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph(10, m, first, n)
        assert e.value.code == EINVAL


def test_list_overflow_is_redone_by_path1(za, monkeypatch):
    X = wide_rows(D2)
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    monkeypatch.delenv("ZH_KNN_LIST_CAP", raising=False)
    ref = ix.knn_graph(10, m)
    assert ix.knn_info()["redone"] == 0
    monkeypatch.setenv("ZH_KNN_LIST_CAP", "512")  # the first launch lists 4095 rows per line: every panel's lists run over
    got = ix.knn_graph(10, m)
    info = ix.knn_info()
    assert info["path"] == 2 and info["redone"] == 9 and info["survivors"] == 0 and info["lines"] == N2, info
    same(got, ref)


def test_device_entry_point_and_siblings(za, monkeypatch):
    import torch
    X = wide_rows(D2)
    Q = zo.synth_queries(8, D2, N2)
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    mask = np.zeros(N2, bool)
    mask[::2] = True
    ix.search_exact_batch(Q, 10, m)
    ix.search_exact_filtered_batch(Q, 10, m, mask)
    ix.search_range_batch(Q, 1.0, m)
    ix.self_join_count(metric=m, max_key=np.uint64(0))
    before = (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.stats())
    host = ix.knn_graph(10, m, 500, 3000)
    dev = torch.device("cuda", 0)
    ids = torch.zeros((3000, 10), dtype=torch.int64, device=dev)
    keys = torch.zeros_like(ids)
    counts = torch.full((3000,), 7, dtype=torch.int32, device=dev)
    ix.knn_graph_device(10, m, 500, 3000, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    assert ix.knn_info()["path"] == 2 and ix.knn_info()["lines"] == 3000
    same((ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)), host)
    ix.knn_graph_device(0, m, 500, 3000, None, None, counts.data_ptr())  # k = 0: the counts alone
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 0).all()
    assert (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.stats()) == before


def test_database_knn_graph(za):
    X = small_rows()[:50]
    docs = ["doc%d" % i for i in range(50)]
    db = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db.insert_records(X, docs)
    db.remove([7])
    live = np.array([r for r in range(50) if r != 7])
    graph = db.knn_graph(3)
    assert sorted(graph) == sorted(docs[r] for r in live)
    ref = oracle_lines(X, live, live.tolist(), zo.L2, 0, 3)
    for a, (rid, rkey) in zip(live.tolist(), ref):
        assert [d for d, _ in graph[docs[a]]] == [docs[int(i)] for i in rid]
        assert [v for _, v in graph[docs[a]]] == zo.key_to_float(rkey).tolist()


@pytest.mark.parametrize("name", ["l2sq", "cos_corrected"])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, name):
    """the held-tile walk (zh_device.h) at its edges, against the family fuzz's reference: a slab of 17 lines is two held tiles, the second with
    one line -- two waves of the one held block are idle; a short launch walks chunks of 8 column tiles (zh_knn_chunk), and of 8200 rows the
    second launch takes tiles 256 .. 512, 257 = 32 x 8 + 1 of them: full chunks (even: the last tile in the second LDS buffer) and a chunk of
    ONE tile (odd, no prefetch at all).  A near-duplicate of a line is planted in that last tile"""
    from tests import family_cases as fc
    n, k, first = 8200, 10, 4000
    spec = fc.metric_spec(name)
    m = za.L2SquaredDistance() if name == "l2sq" else za.CosineDistance(parity=False)
    X = wide_rows(D2)[:n].copy()
    X[8197] = X[first + 16] * np.float32(1.0 + 2.0**-12)
    slab = np.arange(first, first + 17)
    ref = fc.graph_ref(fc.key_matrix(spec, X, X[slab]), slab, np.ones(n, bool), k, 0)
    assert ref[0][16, 0] == 8197
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    got = ix.knn_graph(k, m, first, 17)
    info = ix.knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["lines"] == 17 and info["launches"] == 2 and info["tiles"] == 2 * 513, info
    for g, r, what in zip(got, ref, ("ids", "keys", "counts")):
        assert g.shape == r.shape and (g == r).all(), what

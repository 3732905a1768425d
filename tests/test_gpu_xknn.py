"""The exact k-NN join between two indexes (zh_cross_knn): line i of A.cross_knn(B) holds the k nearest live rows of B to STORED row
first_row + i of A by (key, id), the key that of STORED row b of B against a QUERY equal to row a of A.  The reference is built here from the
oracle's keys (oracle.distance_batch(B[live rows], A[a]) per live a, lexsorted by (key, b), first k); beside it stands B.search_exact_batch with
A's rows as queries.  Every comparison is bit for bit on ids, keys and counts.  Data are finite (a NaN's sign differs between host and GPU)
except in the one case that says otherwise; A and B are disjoint slices of one synth_rows call.  Shapes are the smallest that reach each
mechanism: A of 83 rows is 6 tiles, the last one partial, in 2 blocks of four held tiles with the second one half idle; B of 4133 rows is 259
tiles, the last of 5 rows, in two column launches (4096 positions, then the rest)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

FILL = np.uint64(2**64 - 1)
ELIMIT, EINVAL = -5, -1
NA, NB, D2 = 83, 4133, 256
TA, TB = 6, 259


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    from zebra_amd import _ffi
    assert _ffi.ZH_ELIMIT == ELIMIT and _ffi.ZH_EINVAL == EINVAL
    return zebra_amd


def thirteen_metrics(za):
    """every metric and cosine mode, the two parametrised ones at one power each"""
    return [(za.L2SquaredDistance(), zo.L2SQ, 0), (za.L2Distance(), zo.L2, 0), (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
            (za.CosineDistance(parity=False), zo.COSINE, zo.CORRECTED), (za.ChebyshevDistance(), zo.CHEBYSHEV, 0),
            (za.CanberraDistance(), zo.CANBERRA, 0), (za.BrayCurtisDistance(), zo.BRAY_CURTIS, 0), (za.ManhattanDistance(), zo.MANHATTAN, 0),
            (za.L3Distance(), zo.L3, 0), (za.L4Distance(), zo.L4, 0), (za.HammingDistance(), zo.HAMMING, 0),
            (za.MinkowskiDistance(3), zo.MINKOWSKI, 3), (za.PNormDistance(65), zo.PNORM, 65)]


def oracle_keys(XA, rows_a, XB, rows_b, om, omode):
    """[rows_a][rows_b]: the oracle's key of stored row b of B against the query row a of A"""
    Bl = np.ascontiguousarray(XB[np.asarray(rows_b, np.int64)])
    if not len(rows_a) or not len(rows_b):
        return np.zeros((len(rows_a), len(rows_b)), np.uint64)
    return np.stack([np.asarray(zo.distance_batch(om, omode, Bl, XA[a]), np.uint64) for a in rows_a])


def lines_from(K, rows_b, k, base_b=0):
    """the lines of the key matrix's rows: each one's first k of rows_b by (key, b) -> (ids [n,k], keys [n,k], counts [n])"""
    n, nb = K.shape
    ids, keys, counts = np.full((n, k), FILL), np.full((n, k), FILL), np.full(n, min(k, nb), np.uint32)
    if n and nb and k:
        b = np.broadcast_to(np.asarray(rows_b, np.uint64) + np.uint64(base_b), K.shape)
        o = np.lexsort((b, K), axis=1)[:, :k]
        ids[:, :o.shape[1]] = np.take_along_axis(b, o, 1)
        keys[:, :o.shape[1]] = np.take_along_axis(K, o, 1)
    return ids, keys, counts


def answer_from(n_lines, rows_a, K, rows_b, k, base_b=0, first_row=0):
    """the whole slab's answer: the lines of rows_a at their places, every other line (a removed row's) empty"""
    ids, keys, counts = np.full((n_lines, k), FILL), np.full((n_lines, k), FILL), np.zeros(n_lines, np.uint32)
    at = np.asarray(rows_a, np.int64) - first_row
    ids[at], keys[at], counts[at] = lines_from(K, rows_b, k, base_b)
    return ids, keys, counts


def same(got, ref):
    for g, r, what in zip(got, ref, ("ids", "keys", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), what


def rows_of(got, rows):
    rows = np.asarray(rows, np.int64)
    return got[0][rows], got[1][rows], got[2][rows]


def make(za, X, opts=(64, 4), **kw):
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(*opts), device=0, **kw)
    if X.shape[0]:
        ix.append(X)
    return ix


def ordered(za, X, opts, monkeypatch):
    """an index whose fp16 copy is in a sorted row order (position p holds row perm[p]), as test_gpu_xjoin.py makes it"""
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(*opts), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, X.shape[1], X.shape[0]), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    monkeypatch.delenv("ZH_ROW_ORDER")
    return ix


def exact_reference(ib, XA, rows_a, n_lines, k, m, first_row=0):
    """ib.search_exact_batch over the rows `rows_a` of XA as queries, each line at its place"""
    rows = np.asarray(rows_a, np.int64)
    ids, keys, counts = np.full((n_lines, k), FILL), np.full((n_lines, k), FILL), np.zeros(n_lines, np.uint32)
    if rows.size:
        ids[rows - first_row], keys[rows - first_row], counts[rows - first_row] = ib.search_exact_batch(np.ascontiguousarray(XA[rows]), k, m)
    return ids, keys, counts


# ---------------------------------------------------------------- (1) path 1
@functools.lru_cache(maxsize=None)
def small_rows():
    X = zo.synth_rows(1000, 30)
    return X[:300], X[300:]


@functools.lru_cache(maxsize=None)
def small_oracle(om, omode):
    XA, XB = small_rows()
    return oracle_keys(XA, range(300), XB, range(700), om, omode)


@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, mi, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    ref = answer_from(300, range(300), small_oracle(om, omode), range(700), 10)
    ia, ib = make(za, XA), make(za, XB)
    got = ia.cross_knn(ib, 10, m)
    same(got, ref)
    assert ia.cross_knn_info() == {"rows_live_a": 300, "rows_live_b": 700, "lines": 300, "k": 10, "path": 1, "redone": 0, "survivors": 0,
                                   "launches": 1, "tiles": 0}
    same(got, exact_reference(ib, XA, range(300), 300, 10, m))  # the definition


# ---------------------------------------------------------------- (2) the largest k
def test_path1_largest_k(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    X = zo.synth_rows(1300, 30)
    XA, XB = X[:100], X[100:]
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = make(za, XA), make(za, XB)
    got = ia.cross_knn(ib, 1024, m)
    assert got[0].shape == (100, 1024) and (got[2] == 1024).all()
    sample = [0, 41, 99]
    same(rows_of(got, sample), lines_from(oracle_keys(XA, sample, XB, range(1200), om, omode), range(1200), 1024))
    with pytest.raises(za.ZhError) as e:
        ia.cross_knn(ib, 1025, m)
    assert e.value.code == ELIMIT


# ---------------------------------------------------------------- (3) degenerate and refused
def test_degenerate_and_refused(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    full = make(za, XB[:50])
    empty = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    # an empty A: shape (0, k)
    ids, keys, counts = empty.cross_knn(full, 10, m)
    assert ids.shape == (0, 10) and keys.shape == (0, 10) and counts.shape == (0,)
    # an empty B: count 0 everywhere, the tails filled
    got = full.cross_knn(empty, 10, m)
    same(got, (np.full((50, 10), FILL), np.full((50, 10), FILL), np.zeros(50, np.uint32)))
    assert full.cross_knn_info() == {"rows_live_a": 50, "rows_live_b": 0, "lines": 50, "k": 10, "path": 1, "redone": 0, "survivors": 0,
                                     "launches": 0, "tiles": 0}
    # a B without a live row
    dead = make(za, XA[:20])
    dead.remove(list(range(20)))
    same(full.cross_knn(dead, 10, m), got)
    # B with 7 live rows and k = 10: counts 7, the tails filled
    seven = make(za, XB[:9])
    seven.remove([2, 5])
    live7 = [0, 1, 3, 4, 6, 7, 8]
    got7 = full.cross_knn(seven, 10, m)
    assert (got7[2] == 7).all() and (got7[0][:, 7:] == FILL).all() and (got7[1][:, 7:] == FILL).all()
    same(got7, answer_from(50, range(50), oracle_keys(XB[:50], range(50), XB, live7, om, omode), live7, 10))
    # k = 0 zeroes the counts and touches nothing else
    from zebra_amd import _ffi
    counts = np.full(50, 9, np.uint32)
    assert _ffi.lib().zh_cross_knn(full._h, seven._h, 0, 50, 0, m.metric, m.mode, None, None, counts.ctypes.data_as(C.c_void_p)) == 0
    assert (counts == 0).all() and full.cross_knn_info()["k"] == 0
    # every row of A removed: every line empty
    same(dead.cross_knn(full, 10, m), (np.full((20, 10), FILL), np.full((20, 10), FILL), np.zeros(20, np.uint32)))
    assert dead.cross_knn_info()["lines"] == 0 and dead.cross_knn_info()["rows_live_a"] == 0
    # n = 0 anywhere up to the end, a slab past the end
    assert full.cross_knn(seven, 10, m, first_row=50, n=0)[0].shape == (0, 10)
    for first, n in ((51, 1), (45, 6), (0, 51)):
        with pytest.raises(za.ZhError) as e:
            full.cross_knn(seven, 10, m, first_row=first, n=n)
        assert e.value.code == EINVAL, (first, n)
    # different dims, the same index twice
    other_dim = make(za, zo.synth_rows(10, 31))
    with pytest.raises(za.ZhError) as e:
        full.cross_knn(other_dim, 10, m)
    assert e.value.code == EINVAL and "dim" in str(e.value)
    with pytest.raises(za.ZhError) as e:
        full.cross_knn(full, 10, m)
    assert e.value.code == EINVAL and "zh_knn_graph" in str(e.value)


# ---------------------------------------------------------------- (4) path 2 forced
@functools.lru_cache(maxsize=None)
def wide_rows(d):
    X = zo.synth_rows(NA + NB, d)
    return X[:NA], X[NA:]


@functools.lru_cache(maxsize=None)
def wide_oracle(d, om, omode):
    XA, XB = wide_rows(d)
    return oracle_keys(XA, range(NA), XB, range(NB), om, omode)


def check_path2(ia, ib, XA, m, k, ref, monkeypatch, lines=NA, la=NA, lb=NB, launches=2, tiles=TA * TB):
    monkeypatch.setenv("ZH_XKNN_PATH", "2")
    got = ia.cross_knn(ib, k, m)
    info = ia.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == tiles and info["launches"] == launches, info
    assert info["rows_live_a"] == la and info["rows_live_b"] == lb and info["lines"] == lines and info["k"] == k, info
    assert info["survivors"] >= lines * min(k, lb), info
    if ref is not None:
        same(got, ref)
    monkeypatch.setenv("ZH_XKNN_PATH", "1")
    forced = ia.cross_knn(ib, k, m)
    info = ia.cross_knn_info()
    assert info["path"] == 1 and info["survivors"] == 0 and info["tiles"] == 0, info
    same(forced, got)
    monkeypatch.delenv("ZH_XKNN_PATH")
    return got


@pytest.mark.parametrize("mi", range(4))
def test_path2_against_the_full_oracle_and_the_exact_search(za, monkeypatch, mi):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    K = wide_oracle(D2, om, omode)
    assert K.shape == (NA, NB)
    ia, ib = make(za, XA), make(za, XB)
    got = check_path2(ia, ib, XA, m, 10, answer_from(NA, range(NA), K, range(NB), 10), monkeypatch)
    same(got, exact_reference(ib, XA, range(NA), NA, 10, m))


@pytest.mark.parametrize("k", [1, 100])
def test_path2_other_k(za, monkeypatch, k):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = make(za, XA), make(za, XB)
    check_path2(ia, ib, XA, m, k, answer_from(NA, range(NA), wide_oracle(D2, om, omode), range(NB), k), monkeypatch)


@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    XA, XB = wide_rows(d)
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = make(za, XA), make(za, XB)
    check_path2(ia, ib, XA, m, 10, answer_from(NA, range(NA), wide_oracle(d, om, omode), range(NB), 10), monkeypatch)


# ---------------------------------------------------------------- (5) orientation
@pytest.mark.parametrize("mi", range(4))
def test_orientation_is_the_definition(za, monkeypatch, mi):
    """A.cross_knn(B) and B.cross_knn(A), each against the oracle computed in its own orientation (B's lines sampled)"""
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    ia, ib = make(za, XA), make(za, XB)
    monkeypatch.setenv("ZH_XKNN_PATH", "2")
    same(ia.cross_knn(ib, 10, m), answer_from(NA, range(NA), wide_oracle(D2, om, omode), range(NB), 10))
    got = ib.cross_knn(ia, 10, m)
    info = ib.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live_a"] == NB and info["rows_live_b"] == NA and info["lines"] == NB, info
    assert info["launches"] == 5 and info["tiles"] == TB * TA, info  # five panels of B, one column launch each
    sample = np.sort(np.concatenate([np.random.default_rng(5).choice(NB, 60, replace=False), [0, 1023, 1024, NB - 1]]))
    same(rows_of(got, sample), lines_from(oracle_keys(XB, sample, XA, range(NA), om, omode), range(NA), 10))
    same(got, exact_reference(ia, XB, range(NB), NB, 10, m))


# ---------------------------------------------------------------- (6) mutation and layout
def test_removed_rows_two_id_bases_and_compact(za, monkeypatch):
    base_a, base_b = 1 << 40, 7 << 33
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ia = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base_a)
    ib = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base_b)
    ia.add(XA)
    ib.add(XB)
    gone_a = np.array([0, 17, 18, 19, 64, NA - 1])
    gone_b = np.array(list(range(80, 96, 3)) + list(range(112, 128)) + [4096, NB - 1])  # every third row of a tile, one whole tile, the tail
    ia.remove((gone_a + base_a).tolist())
    ib.remove((gone_b + base_b).tolist())
    rows_a = np.setdiff1d(np.arange(NA), gone_a)
    rows_b = np.setdiff1d(np.arange(NB), gone_b)
    K = oracle_keys(XA, rows_a, XB, rows_b, om, omode)
    ref = answer_from(NA, rows_a, K, rows_b, 10, base_b)
    got = check_path2(ia, ib, XA, m, 10, ref, monkeypatch, lines=rows_a.size, la=rows_a.size, lb=rows_b.size,
                      tiles=((rows_a.size + 15) // 16) * TB)  # (a panel holds live rows only: 77 of them are 5 tiles)
    assert (got[2][gone_a] == 0).all() and (got[0][rows_a] >= np.uint64(base_b)).all() and (got[0][rows_a] < np.uint64(base_a)).all()
    assert not np.isin(got[0][rows_a] - np.uint64(base_b), gone_b).any()
    # B compacted: the same lines under the returned id map (compaction keeps the rows' order, so the map keeps each line's)
    new_b, _ = ib.compact()
    mapped_ids = got[0].copy()
    mapped_ids[rows_a] = new_b[(got[0][rows_a] - np.uint64(base_b)).astype(np.int64)]
    for p in ("1", "2"):
        monkeypatch.setenv("ZH_XKNN_PATH", p)
        same(ia.cross_knn(ib, 10, m), (mapped_ids, got[1], got[2]))
        assert ia.cross_knn_info()["path"] == int(p) and ia.cross_knn_info()["rows_live_b"] == rows_b.size
    # A compacted: its live rows' lines move to the rows the map names, nothing else changes
    new_a, _ = ia.compact()
    at = (new_a[rows_a] - np.uint64(base_a)).astype(np.int64)
    assert at.tolist() == list(range(rows_a.size))
    for p in ("1", "2"):
        monkeypatch.setenv("ZH_XKNN_PATH", p)
        same(ia.cross_knn(ib, 10, m), (mapped_ids[rows_a], got[1][rows_a], got[2][rows_a]))


N_ORD = 8192 + 37  # the shape at which test_gpu_join.py makes an ordered copy


@functools.lru_cache(maxsize=None)
def order_rows():
    X = zo.synth_rows(2 * N_ORD + NB + NA, D2)
    return X[:N_ORD], X[N_ORD:2 * N_ORD], X[2 * N_ORD:2 * N_ORD + NB], X[2 * N_ORD + NB:]


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_row_orders(za, monkeypatch, which):
    """the fp16 copy of A, of B, or of both in a sorted row order: lines and ids are still row numbers.  The ordered side has 8229 rows (a
    forest that gives the order something to sort); the other side is small.  A slab of A's rows is asked for where A is the large side."""
    XL, XL2, XM, XS = order_rows()
    m, om, omode = thirteen_metrics(za)[0]
    XA, XB = {"a": (XL, XM), "b": (XS, XL), "both": (XL, XL2)}[which]
    first, n = (4000, 1100) if which != "b" else (0, NA)  # (two panels of an ordered A)
    sample = first + np.sort(np.random.default_rng(3).choice(n, 24, replace=False))
    ia = ordered(za, XA, (300, 9), monkeypatch) if which in ("a", "both") else make(za, XA)
    ib = ordered(za, XB, (300, 9), monkeypatch) if which in ("b", "both") else make(za, XB)
    monkeypatch.setenv("ZH_XKNN_PATH", "2")
    got = ia.cross_knn(ib, 10, m, first_row=first, n=n)
    info = ia.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["lines"] == n, info
    same(rows_of(got, sample - first), lines_from(oracle_keys(XA, sample, XB, range(XB.shape[0]), om, omode), range(XB.shape[0]), 10))
    same(got, exact_reference(ib, XA, range(first, first + n), n, 10, m, first_row=first))
    ia.close()
    ib.close()


# ---------------------------------------------------------------- (7) duplicates and hard rows
@pytest.mark.parametrize("mi", [0, 2])
def test_duplicates_are_ordinary_neighbours(za, monkeypatch, mi):
    """eight bit-identical copies of A[5] planted in B, some in the second column launch: nothing is excluded, they are listed in id order under
    L2SQ (key 0) and where the oracle puts them under the parity cosine key"""
    XA, XB = (x.copy() for x in wide_rows(D2))
    at = [3, 700, 701, 2048, 4095, 4096, 4100, NB - 1]
    XB[at] = XA[5]
    XB[5] = XA[5] * np.float32(0.5)  # (the row with A's own row number is a neighbour like any other)
    m, om, omode = thirteen_metrics(za)[mi]
    K = oracle_keys(XA, range(NA), XB, range(NB), om, omode)
    ref = answer_from(NA, range(NA), K, range(NB), 10)
    ia, ib = make(za, XA), make(za, XB)
    got = check_path2(ia, ib, XA, m, 10, ref, monkeypatch)
    if mi == 0:
        assert got[0][5, :8].tolist() == at and (got[1][5, :8] == 0).all()
    else:
        line = ref[0][5].tolist()  # (the oracle's: the eight share one key, so they stand together or not at all, in id order)
        pos = [line.index(b) for b in at if b in line]
        assert len(pos) in (0, 8) and pos == sorted(pos)


NEAR = [(i, 100 + i) for i in range(60)]


@functools.lru_cache(maxsize=None)
def planted_rows():
    """test_gpu_knn.py's planted set, restated across two indexes: row NEAR[j] of B is a near-duplicate of row i of A below fp16 resolution (the
    copies' rows are the same halves, only the canonical key orders them), and steps of one ulp around one of them"""
    XA, XB = (x.copy() for x in wide_rows(D2))
    for i, j in NEAR:
        XB[j] = XA[i] * np.float32(1.0 + 2.0**-12)
        XB[2000 + j] = XA[i] * np.float32(1.0 - 2.0**-12)
    XB[200:220] = XA[60:80]  # 20 bit-identical pairs
    XB[400:410] *= np.float32(2.0**40)
    XB[410:420] *= np.float32(2.0**-40)
    XA[80] *= np.float32(2.0**40)
    XA[81] *= np.float32(2.0**-40)
    XB[500:510] = np.round(XB[500:510] * 100.0)  # integer-valued rows
    XB[600] = 0.0
    XA[82] = 0.0
    near = XA[5] * np.float32(1.0 + 2.0**-12)
    for t in range(-4, 5):
        r = near.copy()
        for _ in range(abs(t)):
            r[7] = np.nextafter(r[7], np.float32(np.inf if t > 0 else -np.inf))
        XB[4100 + 4 + t] = r  # (in the second column launch)
    return XA, XB


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    XA, XB = planted_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    K = oracle_keys(XA, range(NA), XB, range(NB), om, omode)
    ia, ib = make(za, XA), make(za, XB)
    got = check_path2(ia, ib, XA, m, 10, answer_from(NA, range(NA), K, range(NB), 10), monkeypatch)
    if mi == 0:
        assert got[0][60, 0] == 200 and got[1][60, 0] == 0


def test_rows_nothing_is_certain_about(za, monkeypatch):
    """a row of A with an infinite element and a row of B whose |x|^2 overflows: nothing certain means always listed, and the canonical key
    decides.  Compared against path 1 and search_exact_batch (the device's own arithmetic on both sides), not the oracle."""
    XA, XB = (x.copy() for x in wide_rows(D2))
    XA[40, 5] = np.inf
    XB[701] = np.float32(1e30)
    for mi in (0, 3):
        m, om, omode = thirteen_metrics(za)[mi]
        ia, ib = make(za, XA), make(za, XB)
        got = check_path2(ia, ib, XA, m, 10, None, monkeypatch)
        same(got, exact_reference(ib, XA, range(NA), NA, 10, m))
        if mi == 0:  # the overflowing row's key is +inf to every line: nobody's neighbour, and the other lines are the oracle's without it
            others = np.setdiff1d(np.arange(NA), [40])
            K = np.delete(wide_oracle(D2, om, omode)[others], 701, 1)
            same(rows_of(got, others), lines_from(K, np.delete(np.arange(NB), 701), 10))


# ---------------------------------------------------------------- (8) redo and panels
def check_redo(ia, ib, XA, m, ref, monkeypatch):
    monkeypatch.setenv("ZH_XKNN_PATH", "2")
    monkeypatch.setenv("ZH_XKNN_LIST_CAP", "512")  # the first launch lists all of its 4096 columns for every line: the panel MUST be redone
    got = ia.cross_knn(ib, 10, m)
    info = ia.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 1 and info["survivors"] == 0 and info["lines"] == NA, info
    same(got, ref)
    monkeypatch.delenv("ZH_XKNN_LIST_CAP")
    same(ia.cross_knn(ib, 10, m), ref)
    assert ia.cross_knn_info()["redone"] == 0


def test_list_overflow_is_redone_by_path1(za, monkeypatch):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    check_redo(make(za, XA), make(za, XB), XA, m, answer_from(NA, range(NA), wide_oracle(D2, om, omode), range(NB), 10), monkeypatch)


def test_redo_under_a_row_order_on_both_sides(za, monkeypatch):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = ordered(za, XA, (40, 9), monkeypatch), ordered(za, XB, (300, 9), monkeypatch)
    check_redo(ia, ib, XA, m, answer_from(NA, range(NA), wide_oracle(D2, om, omode), range(NB), 10), monkeypatch)
    ia.close()
    ib.close()


N2 = 1043  # two panels of A: 1024 live rows, then the rest


@functools.lru_cache(maxsize=None)
def two_panel_rows():
    X = zo.synth_rows(N2 + NB, D2)
    return X[:N2], X[N2:]


def test_two_panels_of_a(za, monkeypatch):
    XA, XB = two_panel_rows()
    m, om, omode = thirteen_metrics(za)[0]
    gone = np.array([5] + list(range(100, 116)))  # 17 rows the first panel skips: it ends at row 1040, the second holds two rows
    rows_a = np.setdiff1d(np.arange(N2), gone)
    ia, ib = make(za, XA), make(za, XB)
    ia.remove(gone.tolist())
    monkeypatch.setenv("ZH_XKNN_PATH", "2")
    got = ia.cross_knn(ib, 10, m)
    info = ia.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["launches"] == 4 and info["tiles"] == (64 + 1) * TB, info
    assert info["lines"] == rows_a.size == 1026 and info["rows_live_a"] == 1026, info
    assert (got[2][gone] == 0).all() and (got[0][gone] == FILL).all()
    same(got, exact_reference(ib, XA, rows_a, N2, 10, m))
    sample = np.sort(np.concatenate([np.random.default_rng(11).choice(rows_a, 40, replace=False), [0, 1039, 1040, 1041, N2 - 1]]))
    same(rows_of(got, sample), lines_from(oracle_keys(XA, sample, XB, range(NB), om, omode), range(NB), 10))


# ---------------------------------------------------------------- (9) slabs
def test_slabs(za, monkeypatch):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ref = answer_from(NA, range(1, NA), wide_oracle(D2, om, omode)[1:], range(NB), 10)
    ia, ib = make(za, XA), make(za, XB)
    ia.remove([0])
    for p in ("2", "1"):
        monkeypatch.setenv("ZH_XKNN_PATH", p)
        parts = [ia.cross_knn(ib, 10, m, first_row=f, n=n) for f, n in ((0, 17), (17, 47), (64, NA - 64))]
        assert ia.cross_knn_info()["lines"] == NA - 64
        same(tuple(np.concatenate([q[i] for q in parts]) for i in range(3)), ref)
        same(ia.cross_knn(ib, 10, m, first_row=30), rows_of(ref, range(30, NA)))  # (n defaults to the rest)


# ---------------------------------------------------------------- (10) the gate without the variable
def test_gate_small_takes_path1(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    m = thirteen_metrics(za)[0][0]
    XA, XB = small_rows()
    ia, ib = make(za, XA), make(za, XB)
    ia.cross_knn(ib, 10, m)
    assert ia.cross_knn_info()["path"] == 1
    WA, WB = wide_rows(D2)  # a supported dimension below 8192 live rows of B stays on path 1 as well
    ja, jb = make(za, WA), make(za, WB)
    ja.cross_knn(jb, 10, m)
    assert ja.cross_knn_info()["path"] == 1


def test_gate_large_takes_path2(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    XL, _, _, XS = order_rows()  # B = 8229 x 256
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = make(za, XS), make(za, XL)
    got = ia.cross_knn(ib, 10, m)
    info = ia.cross_knn_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["launches"] == 2 and info["tiles"] == TA * ((N_ORD + 15) // 16), info
    same(got, exact_reference(ib, XS, range(NA), NA, 10, m))
    sample = list(range(0, NA, 8))
    same(rows_of(got, sample), lines_from(oracle_keys(XS, sample, XL, range(N_ORD), om, omode), range(N_ORD), 10))
    ib.remove(list(range(100, 138)))  # 8191 live rows: below the gate
    ia.cross_knn(ib, 10, m)
    assert ia.cross_knn_info()["path"] == 1


# ---------------------------------------------------------------- (11) edges of the walk
@pytest.mark.parametrize("mi", [0, 3])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, mi):
    """B of 4229 rows: the second column launch is 133 positions, 9 tiles -- at 8 tiles a chunk (a short launch's) one chunk of 8 (an even
    number: its last tile lies in the second LDS buffer) and a chunk of ONE tile (no prefetch at all), which is also B's partial last tile.  A of
    17 rows is two held tiles, the second with one row: two waves of the one held block are idle.  Near-duplicates are planted so that the
    one-tile chunk and the one-row tile both hold a nearest neighbour"""
    nb = 4096 + 8 * 16 + 5
    X = zo.synth_rows(17 + nb, D2)
    XA, XB = X[:17].copy(), X[17:].copy()
    XB[nb - 2], XB[4100] = XA[3] * np.float32(1.0 + 2.0**-12), XA[16] * np.float32(1.0 + 2.0**-12)
    m, om, omode = thirteen_metrics(za)[mi]
    ref = answer_from(17, range(17), oracle_keys(XA, range(17), XB, range(nb), om, omode), range(nb), 10)
    assert ref[0][3, 0] == nb - 2 and ref[0][16, 0] == 4100
    ia, ib = make(za, XA), make(za, XB)
    check_path2(ia, ib, XA, m, 10, ref, monkeypatch, lines=17, la=17, lb=nb, tiles=2 * ((nb + 15) // 16))


# ---------------------------------------------------------------- (12) entry points and siblings
def test_device_entry_point_on_a_callers_stream_with_work_pending(za, monkeypatch):
    """the device entry is bit-equal to the host entry, on the index's own stream and on a caller's stream S that still has work pending when
    the library is entered: a delay, then fills of the outputs.  A call that ran on another stream would be overwritten by the fills.  The
    case is tests/stream_cases.py's (its left index of 300 rows against its large one), its reference made here from its key matrix"""
    import torch
    from tests import family_cases as fc
    from tests import stream_cases as sc
    case = sc.case()
    refs = case.refs["l2sq"]
    k = case.p["k"]
    nl = case.p["b_rows"]
    rows_l = np.flatnonzero(case.aliveL)
    ids, keys, counts = fc.topk_ref(refs.KX[rows_l], case.alive, k, case.base)
    ref = (np.full((nl, k), FILL), np.full((nl, k), FILL), np.zeros(nl, np.uint32))
    ref[0][rows_l], ref[1][rows_l], ref[2][rows_l] = ids, keys, counts
    m = za.L2SquaredDistance()
    big = za.LSHIndex(case.p["d"], za.LSHIndexOptions(64, 4), device=0, id_base=case.base)
    left = za.LSHIndex(case.p["d"], za.LSHIndexOptions(64, 4), device=0, id_base=case.baseL)
    big.append(np.asarray(case.X))
    left.append(np.asarray(case.XL))
    big.remove((case.gone + np.uint64(case.base)).tolist())
    left.remove((case.goneL + np.uint64(case.baseL)).tolist())
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    for path in ("2", "1"):
        monkeypatch.setenv("ZH_XKNN_PATH", path)
        host = left.cross_knn(big, k, m)
        assert left.cross_knn_info()["path"] == int(path)
        same(host, ref)
        for pending in (False, True):
            d_ids = torch.zeros((nl, k), dtype=torch.int64, device=dev)
            d_keys, d_counts = torch.zeros_like(d_ids), torch.zeros(nl, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            if pending:
                with torch.cuda.stream(side):
                    torch.cuda._sleep(20_000_000)  # (some 10 ms of device time: the fills below are still pending when the call is made)
                    d_ids.fill_(7), d_keys.fill_(7), d_counts.fill_(7)
            left.cross_knn_device(big, k, m, 0, nl, d_ids.data_ptr(), d_keys.data_ptr(), d_counts.data_ptr(), side.cuda_stream if pending else None)
            got = (d_ids.cpu().numpy().view(np.uint64), d_keys.cpu().numpy().view(np.uint64), d_counts.cpu().numpy().view(np.uint32))
            torch.cuda.synchronize()
            same(got, host)


def test_siblings_are_left_alone(za, monkeypatch):
    XA, XB = wide_rows(D2)
    Q = zo.synth_queries(8, D2, NA + NB)
    m = za.L2SquaredDistance()
    ia, ib = make(za, XA), make(za, XB)
    for ix in (ia, ib):
        ix.search_exact_batch(Q, 10, m)
        ix.knn_graph(3, m, 0, 20)
        ix.self_join_count(metric=m, max_key=np.uint64(0))
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    monkeypatch.setenv("ZH_XKNN_PATH", "2")  # (either side's fp16 copy is made by its first path-2 call: stats() reports its size)
    ia.cross_join_count(ib, metric=m, max_key=np.uint64(0))
    ib.cross_join_count(ia, metric=m, max_key=np.uint64(0))
    ib.cross_knn(ia, 3, m)
    snapshot = lambda: [(ix.knn_info(), ix.cross_info(), ix.exact_info(), ix.join_info(), ix.range_info(), ix.stats()) for ix in (ia, ib)]  # noqa: E731
    before = snapshot()
    xk_b_before = ib.cross_knn_info()
    assert xk_b_before["rows_live_a"] == NB and xk_b_before["k"] == 3
    for path in ("1", "2"):
        monkeypatch.setenv("ZH_XKNN_PATH", path)
        ia.cross_knn(ib, 10, m)
        assert ia.cross_knn_info()["path"] == int(path) and ia.cross_knn_info()["lines"] == NA
        assert snapshot() == before
        assert ib.cross_knn_info() == xk_b_before  # (the info lives on the LEFT index)
    mine = ia.cross_knn_info()
    graph_before = ia.knn_graph(3, m, 0, 20)
    ia.search_exact_batch(Q, 10, m)
    assert ia.cross_knn_info() == mine  # (and the siblings leave it alone)
    same(ia.knn_graph(3, m, 0, 20), graph_before)


# ---------------------------------------------------------------- (13) lock order
def test_two_threads_join_in_opposite_directions(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    ref_ab = answer_from(300, range(300), small_oracle(om, omode), range(700), 10)
    ref_ba = answer_from(700, range(700), oracle_keys(XB, range(700), XA, range(300), om, omode), range(300), 10)
    ia, ib = make(za, XA), make(za, XB)
    results = {"ab": [], "ba": []}

    def run(name, left, right):
        for _ in range(8):
            results[name].append(left.cross_knn(right, 10, m))

    threads = [threading.Thread(target=run, args=("ab", ia, ib), daemon=True), threading.Thread(target=run, args=("ba", ib, ia), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)  # (a bounded wait: a deadlock fails the test instead of hanging it)
    assert not any(t.is_alive() for t in threads)
    assert len(results["ab"]) == 8 and len(results["ba"]) == 8
    for got in results["ab"]:
        same(got, ref_ab)
    for got in results["ba"]:
        same(got, ref_ba)


# ---------------------------------------------------------------- (14) the Database form
def test_database_nearest_in(za, monkeypatch):
    monkeypatch.delenv("ZH_XKNN_PATH", raising=False)
    XA, XB = small_rows()
    XA, XB = XA[:12], XB[:40]
    docs_a, docs_b = ["a%d" % i for i in range(12)], ["b%d" % i for i in range(40)]
    db_a = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db_b = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db_a.insert_records(XA, docs_a)
    db_b.insert_records(XB, docs_b)
    db_a.remove([7])
    db_b.remove([3, 20])
    live_a = [r for r in range(12) if r != 7]
    live_b = [r for r in range(40) if r not in (3, 20)]
    near = db_a.nearest_in(db_b, 3)
    assert sorted(near) == sorted(docs_a[r] for r in live_a)
    rid, rkey, _ = lines_from(oracle_keys(XA, live_a, XB, live_b, zo.L2, 0), live_b, 3)
    for j, a in enumerate(live_a):
        assert [d for d, _ in near[docs_a[a]]] == [docs_b[int(i)] for i in rid[j]]
        assert [v for _, v in near[docs_a[a]]] == zo.key_to_float(rkey[j]).tolist()
    empty = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    assert empty.nearest_in(db_b, 3) == {}
    assert all(v == [] for v in db_a.nearest_in(empty, 3).values()) and len(db_a.nearest_in(empty, 3)) == 11

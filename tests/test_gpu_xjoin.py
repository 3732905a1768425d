"""The exact join between two indexes (zh_cross_join): every pair (live row a of A, live row b of B) whose key -- that of STORED row b of B against
a QUERY equal to row a of A -- is <= one threshold key, as three arrays ascending by (a, key, b), a with A's id base and b with B's.  The
reference is built here from the oracle's keys (oracle.distance_batch(B[live rows], A[a]) per live a: hits <= max_key, ordered by (key, b));
beside it stands B.search_range_batch with A's rows as queries (pinned to the oracle by test_gpu_range.py).  Every comparison is bit for bit on
a, b, keys and the total.  Data are finite (a NaN's sign differs between host and GPU) except in the one case that says otherwise; A and B are
disjoint slices of one synth_rows call.  Every threshold is the key of an existing pair, taken from the oracle's keys: ties at the threshold are
hits and every case is known on the CPU to have pairs.  Shapes are the smallest that reach each mechanism: A of 83 rows is 6 tiles, the last one
partial, in 2 blocks of four held tiles with the second one half idle; B of 1045 rows is 66 tiles, two chunks of 64, the last tile of 5 rows."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

ALL = np.uint64(2**64 - 1)
ELIMIT, EINVAL = -5, -1
NA, NB, D2 = 83, 1045, 256
TA, TB = 6, 66


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
    """[live a][live b]: the oracle's key of stored row b of B against the query row a of A"""
    Bl = np.ascontiguousarray(XB[rows_b])
    if not len(rows_a) or not len(rows_b):
        return np.zeros((len(rows_a), len(rows_b)), np.uint64)
    return np.stack([np.asarray(zo.distance_batch(om, omode, Bl, XA[a]), np.uint64) for a in rows_a])


def pairs_from(K, rows_a, rows_b, max_key, base_a=0, base_b=0):
    """the join's answer from the key matrix: hits <= max_key, ordered by (a, key, b)"""
    ai, bi = np.nonzero(K <= np.uint64(max_key))
    a = np.asarray(rows_a, np.uint64)[ai] + np.uint64(base_a)
    b = np.asarray(rows_b, np.uint64)[bi] + np.uint64(base_b)
    k = K[ai, bi]
    o = np.lexsort((b, k, a))
    return a[o], b[o], k[o]


def kth_key(K, kth):
    """the kth-smallest key (1-based) of the matrix: an existing pair's key"""
    flat = K.reshape(-1)
    return np.partition(flat, kth - 1)[kth - 1]


def same(got, ref):
    for g, r, what in zip(got, ref, ("a", "b", "keys")):
        assert g.dtype == np.uint64 and g.shape == r.shape and (g == r).all(), what


def restrict(got, a_ids):
    m = np.isin(got[0], np.asarray(a_ids, np.uint64))
    return got[0][m], got[1][m], got[2][m]


def make(za, X, opts=(64, 4), **kw):
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(*opts), device=0, **kw)
    if X.shape[0]:
        ix.append(X)
    return ix


def ordered(za, X, opts, monkeypatch):
    """an index whose fp16 copy is in a sorted row order (position p holds row perm[p]), as test_scan_order_that_is_not_id_order makes it"""
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(*opts), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, X.shape[1], X.shape[0]), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    monkeypatch.delenv("ZH_ROW_ORDER")
    return ix


def raw_call(ia, ib, max_key, m, capacity, with_arrays=True):
    """the host entry point itself -> (rc, a, b, keys, total)"""
    from zebra_amd import _ffi
    a, b, keys = (np.zeros(max(capacity, 1), np.uint64) for _ in range(3))
    total = C.c_uint64(777)
    P = lambda x: x.ctypes.data_as(C.c_void_p) if with_arrays else None  # noqa: E731
    rc = _ffi.lib().zh_cross_join(ia._h, ib._h, int(max_key), m.metric, m.mode, capacity, P(a), P(b), P(keys), C.byref(total))
    return rc, a[:capacity], b[:capacity], keys[:capacity], int(total.value)


def range_reference(ia_rows, XA, ib, mk, m, base_a=0):
    """ib.search_range_batch over the rows `ia_rows` of XA as queries -> (a, b, keys) in the join's order"""
    rows = np.asarray(ia_rows)
    offs, ids, keys = ib.search_range_batch(np.ascontiguousarray(XA[rows]), metric=m, max_keys=np.full(rows.size, mk, np.uint64))
    a = np.repeat(rows.astype(np.uint64) + np.uint64(base_a), np.diff(offs).astype(np.int64))
    return a, ids, keys


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
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    K = small_oracle(om, omode)
    assert K.size == 210000
    mk = kth_key(K, 3000)
    ref = pairs_from(K, range(300), range(700), mk)
    total = ref[0].size
    assert total >= 3000
    ia, ib = make(za, XA), make(za, XB)
    got = ia.cross_join(ib, metric=m, max_key=mk)
    same(got, ref)
    info = ia.cross_info()
    assert info["path"] == 1 and info["tiles"] == 0 and info["pairs"] == total and info["redone"] == 0 and info["candidates"] == 0, info
    assert info["rows_live_a"] == 300 and info["rows_live_b"] == 700, info
    assert ia.cross_join_count(ib, metric=m, max_key=mk) == total
    rc, _, _, _, tot = raw_call(ia, ib, mk, m, total - 1)
    assert rc == ELIMIT and tot == total and ia.cross_info()["pairs"] == total
    rc, _, _, _, tot = raw_call(ia, ib, mk, m, 0, with_arrays=False)
    assert rc == ELIMIT and tot == total
    rc, a, b, k, tot = raw_call(ia, ib, mk, m, total)
    assert rc == 0 and tot == total
    same((a, b, k), ref)
    # the definition: the pairs of a are the hits of a range search on B for row a of A
    for a0 in (0, 137, 299):
        _, ids, keys = ib.search_range_batch(XA[a0:a0 + 1], metric=m, max_keys=np.array([mk], np.uint64))
        sel = got[0] == a0
        assert (got[1][sel] == ids).all() and (got[2][sel] == keys).all()


# ---------------------------------------------------------------- (2), (3) path 2 forced
@functools.lru_cache(maxsize=None)
def wide_rows(d):
    X = zo.synth_rows(NA + NB, d)
    return X[:NA], X[NA:]


@functools.lru_cache(maxsize=None)
def wide_oracle(d, om, omode):
    XA, XB = wide_rows(d)
    return oracle_keys(XA, range(NA), XB, range(NB), om, omode)


def check_path2(ia, ib, m, mk, ref, monkeypatch, la=NA, lb=NB):
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == TA * TB and info["launches"] == 1, info
    assert info["pairs"] == got[0].size and info["candidates"] >= info["pairs"], info
    assert info["rows_live_a"] == la and info["rows_live_b"] == lb, info
    assert got[0].size >= 1
    same(got, ref)
    monkeypatch.setenv("ZH_XJOIN_PATH", "1")
    forced = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 1 and info["candidates"] == 0 and info["tiles"] == 0, info
    same(forced, got)
    monkeypatch.delenv("ZH_XJOIN_PATH")
    return got


@pytest.mark.parametrize("mi", range(4))
def test_path2_forced_against_the_full_oracle(za, monkeypatch, mi):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    K = wide_oracle(D2, om, omode)
    assert K.size == 86735
    mk = kth_key(K, 1000)
    ia, ib = make(za, XA), make(za, XB)
    check_path2(ia, ib, m, mk, pairs_from(K, range(NA), range(NB), mk), monkeypatch)


@pytest.mark.parametrize("d", [256, 384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    XA, XB = wide_rows(d)
    m, om, omode = thirteen_metrics(za)[0]
    K = wide_oracle(d, om, omode)
    mk = kth_key(K, 1000)
    ia, ib = make(za, XA), make(za, XB)
    check_path2(ia, ib, m, mk, pairs_from(K, range(NA), range(NB), mk), monkeypatch)


# ---------------------------------------------------------------- (4) orientation
@pytest.mark.parametrize("mi", range(4))
def test_orientation_is_the_definition(za, monkeypatch, mi):
    """B.cross_join(A): stored rows of A against query rows of B -- the oracle computed in that orientation, not the transpose of the other call"""
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    K = oracle_keys(XB, range(NB), XA, range(NA), om, omode)  # [b][a]
    mk = kth_key(K, 1000)
    ref = pairs_from(K, range(NB), range(NA), mk)
    ia, ib = make(za, XA), make(za, XB)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ib.cross_join(ia, metric=m, max_key=mk)
    info = ib.cross_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == TB * TA and info["rows_live_a"] == NB and info["rows_live_b"] == NA, info
    assert got[0].size >= 1
    same(got, ref)
    o = np.lexsort((got[1], got[2], got[0]))
    assert (o == np.arange(o.size)).all()  # sorted by its own (a, key, b)


# ---------------------------------------------------------------- (5) removed rows, two id bases, compaction
def test_removed_rows_two_id_bases_and_compact(za, monkeypatch):
    base_a, base_b = 1 << 40, 7 << 33
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ia = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base_a)
    ib = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base_b)
    ia.add(XA)
    ib.add(XB)
    gone_a = np.array([0, 17, 18, 19, 64, NA - 1])
    gone_b = np.array(list(range(80, 96, 3)) + list(range(112, 128)) + [1024, NB - 1])  # every third row of a tile, one whole tile, the tail
    ia.remove((gone_a + base_a).tolist())
    ib.remove((gone_b + base_b).tolist())
    rows_a = np.setdiff1d(np.arange(NA), gone_a)
    rows_b = np.setdiff1d(np.arange(NB), gone_b)
    K = oracle_keys(XA, rows_a, XB, rows_b, om, omode)
    mk = kth_key(K, 1000)
    ref = pairs_from(K, rows_a, rows_b, mk, base_a, base_b)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live_a"] == rows_a.size and info["rows_live_b"] == rows_b.size, info
    assert got[0].size >= 1 and (got[0] >= np.uint64(base_a)).all() and (got[1] >= np.uint64(base_b)).all() and (got[1] < np.uint64(base_a)).all()
    assert not np.isin(got[0] - np.uint64(base_a), gone_a).any() and not np.isin(got[1] - np.uint64(base_b), gone_b).any()
    same(got, ref)
    monkeypatch.setenv("ZH_XJOIN_PATH", "1")
    same(ia.cross_join(ib, metric=m, max_key=mk), ref)
    # B compacted: the old answer under the returned map, on either path
    new_b, _ = ib.compact()
    mapped = (got[0], new_b[(got[1] - np.uint64(base_b)).astype(np.int64)], got[2])
    o = np.lexsort((mapped[1], mapped[2], mapped[0]))
    assert (o == np.arange(o.size)).all()  # (compaction keeps the rows' order, so the map keeps the answer's)
    same(ia.cross_join(ib, metric=m, max_key=mk), mapped)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    same(ia.cross_join(ib, metric=m, max_key=mk), mapped)
    assert ia.cross_info()["path"] == 2 and ia.cross_info()["rows_live_b"] == rows_b.size


# ---------------------------------------------------------------- (6) row orders
N_ORD = 8192 + 37  # the shape at which test_gpu_join.py makes an ordered copy


@functools.lru_cache(maxsize=None)
def order_rows():
    X = zo.synth_rows(2 * N_ORD + NB + NA, D2)
    return X[:N_ORD], X[N_ORD:2 * N_ORD], X[2 * N_ORD:2 * N_ORD + NB], X[2 * N_ORD + NB:]


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_row_orders(za, monkeypatch, which):
    """the fp16 copy of A, of B, or of both in a sorted row order: the pairs are still row numbers, in id order.  The ordered side has 8229 rows
    (a forest that gives the order something to sort); the other side is small."""
    XL, XL2, XM, XS = order_rows()
    m, om, omode = thirteen_metrics(za)[0]
    XA, XB = {"a": (XL, XM), "b": (XS, XL), "both": (XL, XL2)}[which]
    sample = np.sort(np.random.default_rng(3).choice(XA.shape[0], min(32, XA.shape[0]), replace=False))
    Ks = oracle_keys(XA, sample, XB, range(XB.shape[0]), om, omode)
    mk = kth_key(Ks, max(1, int(round(3000 * Ks.size / (XA.shape[0] * XB.shape[0])))))
    pa, pb = make(za, XA), make(za, XB)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    ref = pa.cross_join(pb, metric=m, max_key=mk)
    assert pa.cross_info()["path"] == 2 and ref[0].size >= 1
    same(restrict(ref, sample), pairs_from(Ks, sample, range(XB.shape[0]), mk))
    ia = ordered(za, XA, (300, 9), monkeypatch) if which in ("a", "both") else make(za, XA)
    ib = ordered(za, XB, (300, 9), monkeypatch) if which in ("b", "both") else make(za, XB)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] == 0, info
    same(got, ref)
    ia.close()
    ib.close()


# ---------------------------------------------------------------- (7) rows nothing is certain about
def test_rows_nothing_is_certain_about(za, monkeypatch):
    """a row of A with an infinite element and a row of B whose |x|^2 overflows: nothing certain means always a candidate, and the canonical key
    decides.  Compared against path 1 (the device's own arithmetic on both sides), not the oracle."""
    XA, XB = (x.copy() for x in wide_rows(D2))
    XA[40, 5] = np.inf
    XB[701] = np.float32(1e30)
    for mi in (0, 3):
        m, om, omode = thirteen_metrics(za)[mi]
        mk = kth_key(np.delete(np.delete(wide_oracle(D2, om, omode), 40, 0), 701, 1), 1000)  # (the key of a pair of two unchanged rows)
        ia, ib = make(za, XA), make(za, XB)
        monkeypatch.setenv("ZH_XJOIN_PATH", "2")
        got = ia.cross_join(ib, metric=m, max_key=mk)
        info = ia.cross_info()
        assert info["path"] == 2 and info["redone"] == 0 and info["candidates"] >= NB + NA - 1, info  # both rows' every pair was keyed
        assert got[0].size >= 1000
        monkeypatch.setenv("ZH_XJOIN_PATH", "1")
        same(ia.cross_join(ib, metric=m, max_key=mk), got)
        assert ia.cross_info()["path"] == 1
        monkeypatch.delenv("ZH_XJOIN_PATH")


# ---------------------------------------------------------------- (8) adversarial pairs
@functools.lru_cache(maxsize=None)
def planted_rows():
    """bit-identical duplicates across A and B; near-duplicates of A[5] below fp16 resolution in B, one element moved in steps of one ulp"""
    XA, XB = (x.copy() for x in wide_rows(D2))
    XB[200:220] = XA[30:50]
    XB[1040:1045] = XA[78:83]  # (B's partial last tile against A's partial last tile)
    near = XA[5] * np.float32(1.0 + 2.0**-12)
    for t in range(-4, 5):
        r = near.copy()
        r[7] = np.nextafter(r[7], np.float32(np.inf if t > 0 else -np.inf)) if t else r[7]
        for _ in range(abs(t) - 1):
            r[7] = np.nextafter(r[7], np.float32(np.inf if t > 0 else -np.inf))
        XB[600 + 4 + t] = r
    return XA, XB


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_pairs(za, monkeypatch, mi):
    """the threshold is the key of the planted pair (A[5], B[604]): its neighbours at one-ulp steps fall on either side of it, and a bound that
    forgets either operand's rounding loses hits here.  Under the parity cosine key that threshold admits every pair of positive similarity;
    the comparison with the full oracle holds all the same."""
    XA, XB = planted_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    K = oracle_keys(XA, range(NA), XB, range(NB), om, omode)
    mk = K[5, 604]
    ref = pairs_from(K, range(NA), range(NB), mk)
    assert ref[0].size >= 1
    ia, ib = make(za, XA), make(za, XB)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    assert ia.cross_info()["path"] == 2
    same(got, ref)
    have = set(zip(got[0].tolist(), got[1].tolist()))
    assert (5, 604) in have
    if om != zo.COSINE:  # (a duplicate's key is 0 there, below every other key)
        assert all((30 + i, 200 + i) in have for i in range(20)) and all((78 + i, 1040 + i) in have for i in range(5))
    monkeypatch.setenv("ZH_XJOIN_PATH", "1")
    same(ia.cross_join(ib, metric=m, max_key=mk), ref)


# ---------------------------------------------------------------- (9) redo
def check_redo(ia, ib, m, K, monkeypatch):
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    # count only: the panel's pool is its floor of 256 slots per row, 256 * 83 < the 86 735 candidates: the panel MUST be redone by path 1
    assert ia.cross_join_count(ib, metric=m, max_key=ALL) == NA * NB
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] >= 1 and info["pairs"] == NA * NB and info["candidates"] == 0, info
    # the full capacity: the whole rectangle, in order
    rc, a, b, k, tot = raw_call(ia, ib, ALL, m, NA * NB)
    assert rc == 0 and tot == NA * NB
    same((a, b, k), pairs_from(K, range(NA), range(NB), ALL))
    # a first guess far too small (the panel runs over on the first call), then the exact total
    mk = kth_key(K, 30000)
    same(ia.cross_join(ib, metric=m, max_key=mk, capacity=100), pairs_from(K, range(NA), range(NB), mk))


def test_redo(za, monkeypatch):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    check_redo(make(za, XA), make(za, XB), m, wide_oracle(D2, om, omode), monkeypatch)


def test_redo_under_a_row_order_on_both_sides(za, monkeypatch):
    """a panel owns its pairs by A row whatever the order of either copy: the redo holds under a row order too"""
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = ordered(za, XA, (40, 9), monkeypatch), ordered(za, XB, (300, 9), monkeypatch)
    check_redo(ia, ib, m, wide_oracle(D2, om, omode), monkeypatch)
    ia.close()
    ib.close()


# ---------------------------------------------------------------- (10) two panels of A
N3 = 16384 + 37


@functools.lru_cache(maxsize=None)
def two_panel_rows():
    X = zo.synth_rows(N3 + 100, D2)
    return X[:N3], X[N3:]


def test_two_panels_of_a(za, monkeypatch):
    XA, XB = two_panel_rows()
    m, om, omode = thirteen_metrics(za)[0]
    gone = np.array([5] + list(range(100, 116)) + [16383])  # rows of the first panel
    rows_a = np.setdiff1d(np.arange(N3), gone)
    sample = np.sort(np.concatenate([np.random.default_rng(11).choice(rows_a, 60, replace=False), [16382, 16384, 16400, N3 - 1]]))
    Ks = oracle_keys(XA, sample, XB, range(100), om, omode)
    # about 20 / 64 of a pair per row of A, some 5000 pairs -- and at least the nearest pair of row 16400, in the second panel
    mk = max(kth_key(Ks, 20), Ks[sample.tolist().index(16400)].min())
    ia, ib = make(za, XA), make(za, XB)
    ia.remove(gone.tolist())
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    T3 = (N3 + 15) // 16
    assert info["path"] == 2 and info["redone"] == 0 and info["launches"] == 2 and info["tiles"] == T3 * 7, info
    assert info["rows_live_a"] == rows_a.size and info["rows_live_b"] == 100 and info["pairs"] == got[0].size >= 1, info
    assert not np.isin(got[0], gone).any()
    same(got, range_reference(rows_a, XA, ib, mk, m))
    same(restrict(got, sample), pairs_from(Ks, sample, range(100), mk))
    assert (got[0] >= 16384).any() and (got[0] < 16384).any()  # both panels have pairs


# ---------------------------------------------------------------- (11) the gate
def test_gate_small_takes_path1(za, monkeypatch):
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    ia, ib = make(za, XA), make(za, XB)
    assert ia.cross_join_count(ib, metric=m, max_key=kth_key(small_oracle(om, omode), 3000)) >= 3000
    assert ia.cross_info()["path"] == 1
    # a supported dimension below the gate's pair work stays on path 1 as well
    WA, WB = wide_rows(D2)
    ja, jb = make(za, WA), make(za, WB)
    assert ja.cross_join_count(jb, metric=m, max_key=kth_key(wide_oracle(D2, om, omode), 1000)) >= 1000
    assert ja.cross_info()["path"] == 1


def test_gate_large_takes_path2(za, monkeypatch):
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    n_a, n_b = 8192, 8192 + 37
    X = zo.synth_rows(n_a + n_b, D2)
    XA, XB = X[:n_a], X[n_a:]
    m, om, omode = thirteen_metrics(za)[0]
    s128 = np.sort(np.random.default_rng(13).choice(n_a, 128, replace=False))
    s16 = s128[::8]
    Ks = oracle_keys(XA, s16, XB, range(n_b), om, omode)
    mk = kth_key(Ks, 8)  # about half a pair per row of A
    ia, ib = make(za, XA), make(za, XB)
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == (n_a // 16) * ((n_b + 15) // 16) and info["launches"] == 1, info
    assert got[0].size >= 1 and info["pairs"] == got[0].size
    same(restrict(got, s128), range_reference(s128, XA, ib, mk, m))
    same(restrict(got, s16), pairs_from(Ks, s16, range(n_b), mk))
    o = np.lexsort((got[1], got[2], got[0]))
    assert (o == np.arange(o.size)).all()


# ---------------------------------------------------------------- (12) the device entry point
def test_device_entry_point(za, monkeypatch):
    import torch
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[3]
    K = wide_oracle(D2, om, omode)
    mk = kth_key(K, 1000)
    ref = pairs_from(K, range(NA), range(NB), mk)
    total = ref[0].size
    ia, ib = make(za, XA), make(za, XB)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for path in ("2", "1"):
        monkeypatch.setenv("ZH_XJOIN_PATH", path)
        for cap, st in ((total, stream.cuda_stream), (total - 1, stream.cuda_stream), (total + 7, None), (0, None)):
            a = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
            b, keys = torch.zeros_like(a), torch.zeros_like(a)
            tot = torch.full((1,), 9, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            try:
                ia.cross_join_device(ib, mk, m, cap, a.data_ptr() if cap else None, b.data_ptr() if cap else None, keys.data_ptr() if cap else None,
                                     tot.data_ptr(), st)
                assert cap >= total
            except za.ZhError as e:
                assert e.code == ELIMIT and cap < total, e
            torch.cuda.synchronize()
            assert int(tot.cpu()[0]) == total
            if cap >= total:
                for t, h in zip((a, b, keys), ref):
                    assert (t.cpu().numpy().view(np.uint64)[:total] == h).all()


# ---------------------------------------------------------------- (13) siblings
def test_siblings_are_left_alone(za, monkeypatch):
    XA, XB = wide_rows(D2)
    Q = zo.synth_queries(8, D2, NA + NB)
    m = za.L2SquaredDistance()
    ia, ib = make(za, XA), make(za, XB)
    for ix in (ia, ib):
        ix.search_exact_batch(Q, 10, m)
        ix.search_range_batch(Q, 1.0, m)
        ix.self_join_count(metric=m, max_key=np.uint64(0))
    mk = kth_key(wide_oracle(D2, zo.L2SQ, 0), 1000)
    self_before = ia.self_join(metric=m, max_key=mk)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")  # (either side's fp16 copy is made by its first path-2 call: stats() reports its size)
    ia.cross_join_count(ib, metric=m, max_key=mk)
    ib.cross_join_count(ia, metric=m, max_key=mk)
    before =[(ix.join_info(), ix.range_info(), ix.exact_info(), ix.stats()) for ix in (ia, ib)]
    cross_b_before = ib.cross_info()
    assert cross_b_before["rows_live_a"] == NB
    for path in ("1", "2"):
        monkeypatch.setenv("ZH_XJOIN_PATH", path)
        assert ia.cross_join_count(ib, metric=m, max_key=mk) >= 1000
        assert [(ix.join_info(), ix.range_info(), ix.exact_info(), ix.stats()) for ix in (ia, ib)] == before
        assert ib.cross_info() == cross_b_before  # (the info lives on the LEFT index)
    cross_before = ia.cross_info()
    assert cross_before["path"] == 2 and cross_before["pairs"] >= 1000
    same(ia.self_join(metric=m, max_key=mk), self_before)
    assert ia.cross_info() == cross_before


# ---------------------------------------------------------------- (14) lock order
def test_two_threads_join_in_opposite_directions(za, monkeypatch):
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    K = small_oracle(om, omode)
    Kt = oracle_keys(XB, range(700), XA, range(300), om, omode)
    mk = kth_key(K, 3000)
    ref_ab = pairs_from(K, range(300), range(700), mk)
    ref_ba = pairs_from(Kt, range(700), range(300), mk)
    assert ref_ab[0].size >= 3000 and ref_ba[0].size >= 1
    ia, ib = make(za, XA), make(za, XB)
    results = {"ab": [], "ba": []}

    def run(name, left, right):
        for _ in range(8):
            results[name].append(left.cross_join(right, metric=m, max_key=mk))

    threads = [threading.Thread(target=run, args=("ab", ia, ib), daemon=True), threading.Thread(target=run, args=("ba", ib, ia), daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    assert len(results["ab"]) == 8 and len(results["ba"]) == 8
    for got in results["ab"]:
        same(got, ref_ab)
    for got in results["ba"]:
        same(got, ref_ba)


# ---------------------------------------------------------------- (15) degenerate and refused
def test_degenerate_and_refused(za, monkeypatch):
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    XA, XB = small_rows()
    m, om, omode = thirteen_metrics(za)[0]
    full = make(za, XB[:50])
    empty = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)

    def nothing(ia, ib, la, lb):
        a, b, k = ia.cross_join(ib, metric=m, max_key=ALL)
        assert a.size == 0 and b.size == 0 and k.size == 0 and ia.cross_join_count(ib, metric=m, max_key=ALL) == 0
        rc, _, _, _, tot = raw_call(ia, ib, ALL, m, 0, with_arrays=False)
        assert rc == 0 and tot == 0
        assert ia.cross_info() == {"rows_live_a": la, "rows_live_b": lb, "pairs": 0, "path": 1, "redone": 0, "candidates": 0, "launches": 0,
                                   "tiles": 0}

    nothing(empty, full, 0, 50)  # an empty A
    nothing(full, empty, 50, 0)  # an empty B
    dead = make(za, XA[:20])
    dead.remove(list(range(20)))
    nothing(dead, full, 0, 50)  # all rows removed, on either side
    nothing(full, dead, 50, 0)
    one_a, one_b = make(za, XA[7:8]), make(za, XB[9:10])
    a, b, k = one_a.cross_join(one_b, metric=m, max_key=ALL)
    assert a.tolist() == [0] and b.tolist() == [0] and k.tolist() == [int(small_oracle(om, omode)[7, 9])]
    other_dim = make(za, zo.synth_rows(10, 31))
    with pytest.raises(za.ZhError) as e:
        full.cross_join(other_dim, metric=m, max_key=ALL)
    assert e.value.code == EINVAL and "dim" in str(e.value)
    with pytest.raises(za.ZhError) as e:
        full.cross_join(full, metric=m, max_key=ALL)
    assert e.value.code == EINVAL and "zh_self_join" in str(e.value)
    # appended and never built: no forest is needed on either side
    ia, ib = make(za, XA), make(za, XB)
    assert ia.no_trees() and ib.no_trees()
    got = ia.cross_join(ib, metric=m, max_key=ALL)
    assert got[0].size == 300 * 700
    same(got, pairs_from(small_oracle(om, omode), range(300), range(700), ALL))


# ---------------------------------------------------------------- (16) remove_within and the Database forms
def test_remove_within_and_database_forms(za, monkeypatch):
    monkeypatch.delenv("ZH_XJOIN_PATH", raising=False)
    XA, XB = (x.copy() for x in small_rows())
    dup = [3, 40, 41, 299]
    XA[dup] = XB[[10, 500, 500, 699]]  # rows of A that the corpus B already holds (one of B's rows twice)
    m = za.L2Distance()
    K = oracle_keys(XA, range(300), XB, range(700), zo.L2, 0)
    assert sorted(set(np.nonzero(K == 0)[0].tolist())) == dup
    radius = float(zo.key_to_float(np.array([np.sort(K.reshape(-1))[4]], np.uint64))[0]) / 2  # half the smallest non-zero distance
    assert np.sort(K.reshape(-1))[3] == 0 and 0.0 < radius
    db_a = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db_b = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db_a.insert_records(XA, ["a%d" % i for i in range(300)])
    db_b.insert_records(XB, ["b%d" % i for i in range(700)])
    trip = db_a.matches(db_b, radius)
    assert [(x, y) for x, y, _ in trip] == [("a3", "b10"), ("a40", "b500"), ("a41", "b500"), ("a299", "b699")]
    assert all(v == 0.0 for _, _, v in trip)
    ia = make(za, XA)
    assert ia.remove_within(db_b.index, radius, m).tolist() == dup and len(ia) == 296
    assert ia.cross_join_count(db_b.index, radius, m) == 0
    removed = db_a.remove_within(db_b, radius)
    assert removed.dtype == np.uint64 and removed.tolist() == dup
    assert len(db_a.index) == 296 and all(("a%d" % r) not in db_a._documents.values() for r in dup) and len(db_a._documents) == 296
    assert len(db_b.index) == 700 and len(db_b._documents) == 700  # B is untouched
    assert db_a.matches(db_b, radius) == []
    assert db_a.remove_within(db_b, radius).size == 0


# ---------------------------------------------------------------- (17) a loaded snapshot of B
def test_loaded_snapshot_of_b_answers_as_b(za, monkeypatch, tmp_path):
    XA, XB = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    K = wide_oracle(D2, om, omode)
    mk = kth_key(K, 1000)
    ref = pairs_from(K, range(NA), range(NB), mk)
    ia = make(za, XA)
    ib = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ib.add(XB)
    path = str(tmp_path / "b.zhs")
    ib.save(path)
    loaded = za.LSHIndex.load(path, device=0)
    for p in ("2", "1"):
        monkeypatch.setenv("ZH_XJOIN_PATH", p)
        same(ia.cross_join(ib, metric=m, max_key=mk), ref)
        same(ia.cross_join(loaded, metric=m, max_key=mk), ref)
        assert ia.cross_info()["path"] == int(p)
        same(loaded.cross_join(ia, metric=m, max_key=mk), ib.cross_join(ia, metric=m, max_key=mk))


@pytest.mark.parametrize("name", ["l2sq", "cos_corrected"])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, name):
    """the held-tile walk (zh_device.h) at its edges, against the family fuzz's reference: B of 1040 rows is 65 column tiles -- a full chunk of
    ZH_JOIN_CHUNK = 64 (an even number: its last tile lies in the second LDS buffer) and a chunk of ONE tile (odd, no prefetch at all); A of 17
    rows is two held tiles, the second with one row: two waves of the one held block are idle.  Near-duplicates are planted so that the
    one-tile chunk and the one-row tile both have pairs"""
    from tests import family_cases as fc
    spec = fc.metric_spec(name)
    m = za.L2SquaredDistance() if name == "l2sq" else za.CosineDistance(parity=False)
    XB = zo.synth_rows(1040, D2)
    XA = zo.synth_rows(17, D2, row0=10**6).copy()
    XA[3], XA[16] = XB[1030] * np.float32(1.0 + 2.0**-12), XB[70] * np.float32(1.0 + 2.0**-12)
    K = fc.key_matrix(spec, XB, XA)
    mk = fc.quantile_threshold(K, np.ones(K.shape, bool), 300, K.size)
    ref = fc.join_ref(K, np.arange(17), np.ones(17, bool), np.ones(1040, bool), mk, 0, 0, False)
    assert ((ref[0] == 3) & (ref[1] == 1030)).any() and ((ref[0] == 16) & (ref[1] == 70)).any() and ref[0].size >= 300
    ia, ib = make(za, XA), make(za, XB)
    monkeypatch.setenv("ZH_XJOIN_PATH", "2")
    got = ia.cross_join(ib, metric=m, max_key=mk)
    info = ia.cross_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == 2 * 65 and info["pairs"] == ref[0].size, info
    same(got, ref)

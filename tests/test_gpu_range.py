"""The exact range search (zh_search_range_batch): every live stored row whose key is <= a per-query threshold key, as a CSR ascending by
(key, id).  The reference answer is built here from the oracle's keys (oracle.distance_batch over the live rows: hits = keys <= max_key, ordered
by (key, id), offsets by cumulative count) and every comparison is bit for bit on offsets, ids and keys.  Data are finite, so no NaN key
arises (a NaN's sign bit differs between the host's and the GPU's arithmetic, as test_gpu_exact notes).  Shapes are the smallest that reach each
mechanism: path 2 wants 8192 live rows at d >= 256, an internal batch is 1024 queries."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

ALL = np.uint64(2**64 - 1)
ELIMIT = -5


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


def key_matrix(X, rows, Q, om, omode):
    """[query][live row] the oracle's keys (rows: the ascending live rows)"""
    Xs = np.ascontiguousarray(X[rows])
    return np.stack([zo.distance_batch(om, omode, Xs, Q[b]) for b in range(Q.shape[0])])


def reference(K, rows, max_keys, id_base=0):
    """K = key_matrix(...) -> (offsets, ids, keys) of the range search"""
    offs, ids, keys = [0], [], []
    for b in range(K.shape[0]):
        hit = K[b] <= max_keys[b]
        r, k = rows[hit].astype(np.uint64), K[b][hit]
        o = np.lexsort((r, k))
        ids.append(r[o] + np.uint64(id_base))
        keys.append(k[o])
        offs.append(offs[-1] + int(hit.sum()))
    return np.array(offs, np.uint64), np.concatenate(ids), np.concatenate(keys)


def same(got, ref):
    assert got[0].dtype == np.uint64 and (got[0] == ref[0]).all(), "offsets"
    assert got[1].shape == ref[1].shape and (got[1] == ref[1]).all(), "ids"
    assert got[2].shape == ref[2].shape and (got[2] == ref[2]).all(), "keys"


def kth_keys(K, kth):
    """per query the key of its kth-nearest row: the boundary key is itself a hit, and rows tied with it are hits too"""
    return np.sort(K, axis=1)[:, kth - 1].copy()


# ---------------------------------------------------------------- path 1
@functools.lru_cache(maxsize=None)
def small_case(d):
    n = 1500
    return zo.synth_rows(n, d), zo.synth_queries(20, d, n)


@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, mi):
    X, Q = small_case(30)
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(X.shape[0])
    K = key_matrix(X, rows, Q, om, omode)
    mk = kth_keys(K, 40)
    got = ix.search_range_batch(Q, metric=m, max_keys=mk)
    ref = reference(K, rows, mk)
    assert (np.diff(ref[0]) >= 40).all()
    same(got, ref)
    info = ix.range_info()
    assert info["path"] == 1 and info["redone"] == 0 and info["batch"] == 20 and info["rows_live"] == 1500 and info["hits"] == int(ref[0][-1]), info
    assert (ix.range_count_batch(Q, metric=m, max_keys=mk) == np.diff(ref[0])).all()
    pairs = ix.search_range(Q[3], metric=m, max_keys=mk[3:4])
    lo, hi = int(ref[0][3]), int(ref[0][4])
    assert [p[0] for p in pairs] == ref[1][lo:hi].tolist() and [p[1] for p in pairs] == ref[2][lo:hi].tolist()


def test_path1_second_dimension_and_radius(za):
    X, Q = small_case(128)
    m, om = za.L2Distance(), zo.L2
    ix = za.LSHIndex(128, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(X.shape[0])
    K = key_matrix(X, rows, Q, om, 0)
    mk = kth_keys(K, 40)
    same(ix.search_range_batch(Q, metric=m, max_keys=mk), reference(K, rows, mk))
    # a radius: the distance of every query's 40th row, and one radius for all
    r = zo.key_to_float(mk)
    same(ix.search_range_batch(Q, r, m), reference(K, rows, mk))
    r1 = float(np.median(r))
    same(ix.search_range_batch(Q, r1, m), reference(K, rows, np.full(20, za.radius_key(m, r1), np.uint64)))


def test_duplicated_rows(za):
    d, n = 30, 2000
    X = zo.synth_rows(n, d).copy()
    dup = np.random.default_rng(3).choice(n, 300, replace=False)
    X[dup] = X[dup[0]]
    Q = np.concatenate([X[dup[0]:dup[0] + 1] + np.float32(0.25), zo.synth_queries(3, d, n)])
    m, om = za.L2SquaredDistance(), zo.L2SQ
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(n)
    K = key_matrix(X, rows, Q, om, 0)
    mk = K[:, dup[0]].copy()  # the copies' key
    ref = reference(K, rows, mk)
    got = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(got, ref)
    seg = got[1][int(got[0][0]):int(got[0][1])]
    tied = seg[got[2][int(got[0][0]):int(got[0][1])] == mk[0]]
    assert set(np.sort(dup).tolist()) <= set(tied.tolist()) and (np.diff(tied.astype(np.int64)) > 0).all()  # every copy, in id order


def test_removed_rows_then_compact(za):
    d, n, base = 30, 1500, 1 << 40
    X, Q = small_case(d)
    m, om = za.ManhattanDistance(), zo.MANHATTAN
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    ix.add(X)
    gone = np.arange(0, n, 3)
    ix.remove((gone + base).tolist())
    alive = np.ones(n, bool)
    alive[gone] = False
    rows = np.flatnonzero(alive)
    K = key_matrix(X, rows, Q, om, 0)
    mk = kth_keys(K, 40)
    ref = reference(K, rows, mk, base)
    got = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(got, ref)
    assert not np.isin(got[1] - np.uint64(base), gone).any() and ix.range_info()["rows_live"] == len(rows)
    new_ids, _ = ix.compact()
    after = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(after, (ref[0], new_ids[(ref[1] - np.uint64(base)).astype(np.int64)], ref[2]))


def test_empty_cases(za):
    d = 30
    X, Q = small_case(d)
    m = za.L2SquaredDistance()
    mk = np.full(20, ALL, np.uint64)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    for emptied in (False, True):  # an empty index, then one emptied by removals
        if emptied:
            ix.add(X[:50])
            ix.remove(list(range(50)))
        offs, ids, keys = ix.search_range_batch(Q, metric=m, max_keys=mk)
        assert offs.shape == (21,) and (offs == 0).all() and ids.size == 0 and keys.size == 0
        assert (ix.range_count_batch(Q, metric=m, max_keys=mk) == 0).all()
        assert ix.range_info()["hits"] == 0 and ix.range_info()["rows_live"] == 0 and ix.range_info()["batch"] == 20
    offs, ids, _ = ix.search_range_batch(Q[:0], metric=m, max_keys=mk[:0])
    assert offs.tolist() == [0] and ids.size == 0
    # appended only, never built: served
    ap = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ap.append(X)
    rows = np.arange(X.shape[0])
    K = key_matrix(X, rows, Q, zo.L2SQ, 0)
    same(ap.search_range_batch(Q, metric=m, max_keys=kth_keys(K, 5)), reference(K, rows, kth_keys(K, 5)))


def test_whole_table_and_nothing(za):
    d, n = 30, 1500
    X, Q = small_case(d)
    m, om = za.L2SquaredDistance(), zo.L2SQ
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(n)
    K = key_matrix(X, rows, Q, om, 0)
    mk = np.full(20, ALL, np.uint64)
    got = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(got, reference(K, rows, mk))
    assert (np.diff(got[0]) == n).all()
    ei, ek, ec = ix.search_exact_batch(Q, 1024, m)
    for b in range(20):
        lo = int(got[0][b])
        assert (got[1][lo:lo + 1024] == ei[b]).all() and (got[2][lo:lo + 1024] == ek[b]).all() and ec[b] == 1024
    # thresholds below a query's nearest key: empty segments in the middle of the CSR
    mk = kth_keys(K, 7)
    for b in (0, 5, 6, 19):
        mk[b] = K[b].min() - np.uint64(1)
    ref = reference(K, rows, mk)
    assert ref[0][5] == ref[0][6] == ref[0][7] and ref[0][8] > ref[0][7]
    same(ix.search_range_batch(Q, metric=m, max_keys=mk), ref)


def raw_call(za, ix, Q, mk, m, capacity, with_arrays=True):
    """the host entry point itself -> (rc, offsets, ids, keys, total)"""
    import ctypes as C
    from zebra_amd import _ffi
    b = Q.shape[0]
    offs = np.full(b + 1, 12345, np.uint64)
    ids, keys = np.zeros(max(capacity, 1), np.uint64), np.zeros(max(capacity, 1), np.uint64)
    total = C.c_uint64(777)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _ffi.lib().zh_search_range_batch(ix._h, P(Q), b, P(mk), m.metric, m.mode, capacity, P(offs), P(ids) if with_arrays else None,
                                          P(keys) if with_arrays else None, C.byref(total))
    return rc, offs, ids[:capacity], keys[:capacity], int(total.value)


@pytest.mark.parametrize("path1", [True, False])
def test_capacity(za, monkeypatch, path1):
    """one below the total and capacity 0 with NULL arrays: ZH_ELIMIT with the total and ALL offsets exact; the exact capacity succeeds.  On
    both paths (path 2: 20 011 x 256)."""
    if path1:
        X, Q = small_case(30)
        d = 30
    else:
        X, Q, d = wide_case(256)[0], wide_case(256)[1][:20], 256
    m, om = za.L2SquaredDistance(), zo.L2SQ
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(X.shape[0])
    K = key_matrix(X, rows, Q, om, 0) if path1 else wide_keys(256, om, 0)[:20]
    mk = kth_keys(K, 40)
    ref = reference(K, rows, mk)
    total = int(ref[0][-1])
    for cap, arrays in ((total - 1, True), (0, False), (total // 2, True)):
        rc, offs, _, _, tot = raw_call(za, ix, Q, mk, m, cap, arrays)
        assert rc == ELIMIT and tot == total and (offs == ref[0]).all(), (cap, rc, tot)
        assert ix.range_info()["hits"] == total and ix.range_info()["path"] == (1 if path1 else 2) and ix.range_info()["redone"] == 0
    rc, offs, ids, keys, tot = raw_call(za, ix, Q, mk, m, total)
    assert rc == 0 and tot == total
    same((offs, ids, keys), ref)
    # the wrapper's two calls: a guess that is too small, then the exact total
    same(ix.search_range_batch(Q, metric=m, max_keys=mk, capacity=3), ref)


def test_many_batches(za):
    d, n, B = 30, 1500, 1030  # crosses the internal batch of 1024
    X = small_case(d)[0]
    Q = zo.synth_queries(B, d, n)
    m, om = za.L2SquaredDistance(), zo.L2SQ
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(n)
    K = key_matrix(X, rows, Q, om, 0)
    mk = kth_keys(K, 3)
    mk[1025] = ALL
    ref = reference(K, rows, mk)
    got = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(got, ref)
    assert ix.range_info()["batch"] == B and ix.range_info()["launches"] == 2
    # ... and when the capacity runs out inside the first internal batch, the second one's offsets are still exact
    rc, offs, _, _, tot = raw_call(za, ix, Q, mk, m, 100)
    assert rc == ELIMIT and tot == int(ref[0][-1]) and (offs == ref[0]).all()


# ---------------------------------------------------------------- path 2
@functools.lru_cache(maxsize=None)
def wide_case(d):
    n = 20011  # not a multiple of 16; 40 queries: not one either
    return zo.synth_rows(n, d), zo.synth_queries(40, d, n)


@functools.lru_cache(maxsize=None)
def wide_keys(d, om, omode):
    X, Q = wide_case(d)
    return key_matrix(X, np.arange(X.shape[0]), Q, om, omode)


def wide_thresholds(K):
    """exactly an existing pair's key per query: the 40th nearest, for a few queries the 1st, the 1000th, and one above every row"""
    mk = kth_keys(K, 40)
    mk[1] = kth_keys(K, 1)[1]
    mk[2] = kth_keys(K, 1000)[2]
    mk[3] = K[3].max()
    return mk


def check_path2(za, ix, d, cases, monkeypatch):
    X, Q = wide_case(d)
    rows = np.arange(X.shape[0])
    for m, om, omode in cases:
        K = wide_keys(d, om, omode)
        mk = wide_thresholds(K)
        ref = reference(K, rows, mk)
        monkeypatch.delenv("ZH_RANGE_PATH", raising=False)
        got = ix.search_range_batch(Q, metric=m, max_keys=mk)
        info = ix.range_info()
        assert info["path"] == 2 and info["redone"] == 0 and info["launches"] == 1, info
        assert info["hits"] == int(ref[0][-1]) and info["candidates"] >= info["hits"], info
        same(got, ref)
        monkeypatch.setenv("ZH_RANGE_PATH", "1")
        forced = ix.search_range_batch(Q, metric=m, max_keys=mk)
        assert ix.range_info()["path"] == 1 and ix.range_info()["candidates"] == 0
        same(forced, ref)
        monkeypatch.delenv("ZH_RANGE_PATH")


def test_path2_against_path1_and_the_oracle(za, monkeypatch):
    d = 256
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(wide_case(d)[0])
    check_path2(za, ix, d, thirteen_metrics(za)[:4], monkeypatch)


def test_path2_d768(za, monkeypatch):
    d = 768
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(wide_case(d)[0])
    check_path2(za, ix, d, thirteen_metrics(za)[:1], monkeypatch)


def test_path2_under_a_row_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): candidates still name the right rows"""
    d = 256
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    X, Q = wide_case(d)
    ix = za.LSHIndex(d, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(Q, 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    if ix.stats()["scan_order_keys"] == 0:
        pytest.skip("the index kept no row order at 20 011 rows (scan_order_keys == 0): nothing to permute")
    check_path2(za, ix, d, thirteen_metrics(za)[:3], monkeypatch)
    assert ix.stats()["scan_order_keys"] == 2
    ix.close()


def test_path2_pool_overflow_is_handled(za, capsys):
    """a threshold admitting every row with capacity = the exact total: path 2 completes, or its candidate pool ran over and path 1 answered
    (redone > 0) -- the answer is bit-equal either way.  Then capacity 0: the candidate pool is its floor of 4096 per query, far below the
    20 011 candidates per query, so path 2 MUST run over and the counts come from path 1."""
    d = 256
    X, Q = wide_case(d)
    Q = Q[:6]
    m, om = za.L2SquaredDistance(), zo.L2SQ
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    rows = np.arange(X.shape[0])
    K = wide_keys(d, om, 0)[:6]
    mk = np.full(6, ALL, np.uint64)
    ref = reference(K, rows, mk)
    rc, offs, ids, keys, tot = raw_call(za, ix, Q, mk, m, int(ref[0][-1]))
    info = ix.range_info()
    with capsys.disabled():
        print("\n[range] every row admitted, capacity = total: path %d, redone %d, candidates %d" % (info["path"], info["redone"], info["candidates"]))
    assert rc == 0 and tot == int(ref[0][-1]) and info["path"] == 2 and (info["redone"] > 0 or info["candidates"] == tot)
    same((offs, ids, keys), ref)
    assert (ix.range_count_batch(Q, metric=m, max_keys=mk) == X.shape[0]).all()
    info = ix.range_info()
    assert info["path"] == 2 and info["redone"] == 1 and info["candidates"] == 0 and info["hits"] == tot, info


# ---------------------------------------------------------------- entry points and neighbours
def test_device_entry_point(za):
    import torch
    d = 256
    X, Q = wide_case(d)
    m, om = za.CosineDistance(parity=False), zo.COSINE
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    K = wide_keys(d, om, zo.CORRECTED)
    mk = wide_thresholds(K)
    host = ix.search_range_batch(Q, metric=m, max_keys=mk)
    same(host, reference(K, np.arange(X.shape[0]), mk))
    total = int(host[0][-1])
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    dmk = torch.from_numpy(mk.view(np.int64)).to(dev)
    for cap in (total, total + 100, total - 1, 0):
        offs = torch.full((Q.shape[0] + 1,), 5, dtype=torch.int64, device=dev)
        ids = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        keys = torch.zeros_like(ids)
        tot = torch.full((1,), 9, dtype=torch.int64, device=dev)
        try:
            ix.search_range_batch_device(dq.data_ptr(), Q.shape[0], dmk.data_ptr(), m, cap, offs.data_ptr(), ids.data_ptr() if cap else None,
                                         keys.data_ptr() if cap else None, tot.data_ptr())
            assert cap >= total
        except za.ZhError as e:
            assert e.code == ELIMIT and cap < total, e
        torch.cuda.synchronize()
        assert int(tot.cpu()[0]) == total and (offs.cpu().numpy().view(np.uint64) == host[0]).all()
        if cap >= total:
            assert (ids.cpu().numpy().view(np.uint64)[:total] == host[1]).all() and (keys.cpu().numpy().view(np.uint64)[:total] == host[2]).all()


def test_siblings_are_left_alone(za):
    d, k = 256, 10
    X, Q = wide_case(d)
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    mask = np.zeros(X.shape[0], bool)
    mask[::2] = True
    e1, ei1 = ix.search_exact_batch(Q, k, m), ix.exact_info()
    f1, fi1 = ix.search_exact_filtered_batch(Q, k, m, mask), ix.filtered_info()
    st1 = ix.stats()
    ix.search_range_batch(Q, metric=m, max_keys=wide_thresholds(wide_keys(d, zo.L2SQ, 0)))
    assert ix.range_info()["path"] == 2
    assert ix.exact_info() == ei1 and ix.filtered_info() == fi1 and ix.stats() == st1
    e2, f2 = ix.search_exact_batch(Q, k, m), ix.search_exact_filtered_batch(Q, k, m, mask)
    for a, b in zip(e1 + f1, e2 + f2):
        assert (a == b).all()
    assert ix.exact_info() == ei1 and ix.filtered_info() == fi1


def test_database_query_vectors_within(za):
    d, n = 30, 1500
    X, Q = small_case(d)
    db = za.Database(d, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db.insert_records(X, ["doc%d" % i for i in range(n)])
    K = key_matrix(X, np.arange(n), Q, zo.L2, 0)
    r = float(np.median(zo.key_to_float(kth_keys(K, 10))))
    ref = reference(K, np.arange(n), np.full(20, za.radius_key(db.metric, r), np.uint64))
    got = db.query_vectors_within(Q, r)
    assert sorted(got) == list(range(20))
    for b in range(20):
        want = ref[1][int(ref[0][b]):int(ref[0][b + 1])].tolist()
        assert list(got[b]) == want and list(got[b].values()) == ["doc%d" % i for i in want]
    assert za.Database(d, za.L2Distance, za.LSHIndexOptions(64, 4), device=0).query_vectors_within(Q, r) == {}

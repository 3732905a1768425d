"""The exact self-join (zh_self_join): every pair of distinct live rows (a, b), a < b, whose key -- that of stored row b against a query equal to
row a -- is <= one threshold key, as three arrays ascending by (a, key, b).  The reference is built here from the oracle's keys
(oracle.distance_batch(X[live rows > a], X[a]) per live a: hits <= max_key, ordered by (key, b)); at the path-2 shape from search_range_batch over
all rows as queries (pinned to the oracle by test_gpu_range.py), kept where id > query index, and from the oracle on sampled rows a.  Every
comparison is bit for bit on a, b, keys and the total.  Data are finite (a NaN's sign differs between host and GPU, as test_gpu_exact notes)
except in the one case that says otherwise.  Shapes are the smallest that reach each mechanism: path 2 wants 8192 live rows at d >= 256; 8192 + 37
rows are 515 tiles, the last one partial, and 129 blocks of four held tiles, the last one partial too."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

ALL = np.uint64(2**64 - 1)
ELIMIT = -5
N2, D2 = 8192 + 37, 256


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


def oracle_rows(X, rows, a_list, om, omode):
    """per a of a_list (live rows): (the live rows b > a, the oracle's keys of stored b against query a)"""
    out = []
    for a in a_list:
        bs = rows[rows > a]
        ks = zo.distance_batch(om, omode, np.ascontiguousarray(X[bs]), X[a]) if bs.size else np.zeros(0, np.uint64)
        out.append((bs.astype(np.uint64), np.asarray(ks, np.uint64)))
    return out


def pairs_from(a_list, per_a, max_key, id_base=0):
    """the join's answer restricted to the rows a of a_list (ascending): hits <= max_key, ordered by (a, key, b)"""
    A, B, K = [], [], []
    for a, (bs, ks) in zip(a_list, per_a):
        hit = ks <= max_key
        b, k = bs[hit], ks[hit]
        o = np.lexsort((b, k))
        A.append(np.full(b.size, a + id_base, np.uint64))
        B.append(b[o] + np.uint64(id_base))
        K.append(k[o])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.uint64)  # noqa: E731
    return cat(A), cat(B), cat(K)


def same(got, ref):
    for g, r, what in zip(got, ref, ("a", "b", "keys")):
        assert g.dtype == np.uint64 and g.shape == r.shape and (g == r).all(), what


def restrict(got, a_list, id_base=0):
    m = np.isin(got[0], np.asarray(a_list, np.uint64) + np.uint64(id_base))
    return got[0][m], got[1][m], got[2][m]


def raw_call(ix, max_key, m, capacity, with_arrays=True):
    """the host entry point itself -> (rc, a, b, keys, total)"""
    from zebra_amd import _ffi
    a, b, keys = (np.zeros(max(capacity, 1), np.uint64) for _ in range(3))
    total = C.c_uint64(777)
    P = lambda x: x.ctypes.data_as(C.c_void_p) if with_arrays else None  # noqa: E731
    rc = _ffi.lib().zh_self_join(ix._h, int(max_key), m.metric, m.mode, capacity, P(a), P(b), P(keys), C.byref(total))
    return rc, a[:capacity], b[:capacity], keys[:capacity], int(total.value)


# ---------------------------------------------------------------- path 1
@functools.lru_cache(maxsize=None)
def small_rows():
    return zo.synth_rows(1500, 30)


@functools.lru_cache(maxsize=None)
def small_oracle(om, omode):
    X = small_rows()
    rows = np.arange(X.shape[0])
    return oracle_rows(X, rows, rows.tolist(), om, omode)


@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, mi):
    X = small_rows()
    n = X.shape[0]
    m, om, omode = thirteen_metrics(za)[mi]
    per_a = small_oracle(om, omode)
    allk = np.concatenate([ks for _, ks in per_a])
    assert allk.size == n * (n - 1) // 2
    mk = np.partition(allk, 2999)[2999]  # the key of the 3000th-smallest pair: itself a hit, and so are the pairs tied with it
    ref = pairs_from(list(range(n)), per_a, mk)
    total = ref[0].size
    assert total >= 3000
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = ix.self_join(metric=m, max_key=mk)
    same(got, ref)
    info = ix.join_info()
    assert info["path"] == 1 and info["redone"] == 0 and info["rows_live"] == n and info["pairs"] == total and info["tiles"] == 0, info
    assert ix.self_join_count(metric=m, max_key=mk) == total
    rc, _, _, _, tot = raw_call(ix, mk, m, total - 1)
    assert rc == ELIMIT and tot == total and ix.join_info()["pairs"] == total
    rc, _, _, _, tot = raw_call(ix, mk, m, 0, with_arrays=False)
    assert rc == ELIMIT and tot == total
    rc, a, b, k, tot = raw_call(ix, mk, m, total)
    assert rc == 0 and tot == total
    same((a, b, k), ref)
    # the definition: the pairs starting at a are the hits of a range search for row a with id > a
    for a0 in (0, 700, n - 2):
        _, ids, keys = ix.search_range_batch(X[a0:a0 + 1], metric=m, max_keys=np.array([mk], np.uint64))
        sel = got[0] == a0
        assert (got[1][sel] == ids[ids > a0]).all() and (got[2][sel] == keys[ids > a0]).all()


# ---------------------------------------------------------------- path 2
@functools.lru_cache(maxsize=None)
def wide_rows(d):
    return zo.synth_rows(N2, d)


SAMPLE = np.sort(np.random.default_rng(7).choice(N2 - 1, 128, replace=False)).tolist()


def threshold_from_sample(per_a, want_pairs, n):
    """exactly an existing pair's key: the sampled pairs are a share s of all n (n - 1) / 2, so the (want_pairs * s)-th smallest sampled key
    admits about want_pairs pairs"""
    allk = np.concatenate([ks for _, ks in per_a])
    kth = max(1, int(round(want_pairs * allk.size / (n * (n - 1) / 2))))
    return np.partition(allk, kth - 1)[kth - 1]


def range_reference(ix, X, mk, m, id_base=0, rows=None):
    """search_range_batch over all LIVE rows (`rows`, ascending; default: every row) as queries, hits kept where id > the query's id
    -> (a, b, keys) in the join's order"""
    rows = np.arange(X.shape[0]) if rows is None else rows
    offs, ids, keys = ix.search_range_batch(np.ascontiguousarray(X[rows]), metric=m, max_keys=np.full(rows.size, mk, np.uint64))
    a = np.repeat(rows.astype(np.uint64) + np.uint64(id_base), np.diff(offs).astype(np.int64))
    keep = ids > a
    return a[keep], ids[keep], keys[keep]


def check_path2(za, ix, X, m, om, omode, mk, monkeypatch, sample=SAMPLE, want_redone=0):
    n = X.shape[0]
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    got = ix.self_join(metric=m, max_key=mk)
    info = ix.join_info()
    T = (n + 15) // 16
    assert info["path"] == 2 and info["redone"] == want_redone and info["rows_live"] == n, info
    assert info["tiles"] == T * (T + 1) // 2, info  # nothing below the diagonal (from the launch geometry)
    assert info["pairs"] == got[0].size and info["candidates"] >= info["pairs"] and info["launches"] == 1, info
    assert (got[0] < got[1]).all()
    same(got, range_reference(ix, X, mk, m))
    rows = np.arange(n)
    same(restrict(got, sample), pairs_from(sample, oracle_rows(X, rows, sample, om, omode), mk))
    monkeypatch.setenv("ZH_JOIN_PATH", "1")
    forced = ix.self_join(metric=m, max_key=mk)
    assert ix.join_info()["path"] == 1 and ix.join_info()["candidates"] == 0 and ix.join_info()["tiles"] == 0
    same(forced, got)
    monkeypatch.delenv("ZH_JOIN_PATH")
    return got


@pytest.mark.parametrize("mi", range(4))
def test_path2_against_the_range_search_and_the_oracle(za, monkeypatch, mi):
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[mi]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    mk = threshold_from_sample(oracle_rows(X, np.arange(N2), SAMPLE, om, omode), 3000, N2)
    got = check_path2(za, ix, X, m, om, omode, mk, monkeypatch)
    assert 500 <= got[0].size <= 20000  # a few thousand pairs
    assert ix.self_join_count(metric=m, max_key=mk) == got[0].size and ix.join_info()["path"] == 2


@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    X = wide_rows(d)
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    mk = threshold_from_sample(oracle_rows(X, np.arange(N2), SAMPLE, om, omode), 3000, N2)
    check_path2(za, ix, X, m, om, omode, mk, monkeypatch)


# ---------------------------------------------------------------- adversarial rows
NEAR = [(i, 100 + i) for i in range(60)]


@functools.lru_cache(maxsize=None)
def planted_rows():
    X = wide_rows(D2).copy()
    for i, j in NEAR:  # near-duplicates below fp16 resolution: the copy's two rows are the same halves
        X[j] = X[i] * np.float32(1.0 + 2.0**-12)
    X[200:220] = X[300:320]  # bit-identical duplicates: key 0 (the parity cosine key: similarity 1)
    X[400:410] *= np.float32(2.0**40)
    X[410:420] *= np.float32(2.0**-40)
    X[500:510] = np.round(X[500:510] * 100.0)  # integer-valued rows
    X[600] = 0.0
    return X


PLANTED = sorted(set([i for i, _ in NEAR] + list(range(200, 220)) + list(range(300, 320)) + list(range(400, 420)) + list(range(500, 510)) + [600]))


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    """the threshold is the near-duplicates' own largest key: a bound that forgets the second operand's rounding loses hits here.  That claim
    is made for L2SQ, L2 and the literal cosine key ONLY.  The parity cosine key is the similarity 1 - distance and positive similarities
    compare ascending: the near-duplicates (similarity ~1) are the LAST of them, so a threshold at their key admits every pair of positive
    similarity, about half of the table's 33.8 M, and no threshold isolates them.  There the threshold is a sampled small key and the case
    checks the planted rows' pairs against the oracle, not the second operand's rounding."""
    X = planted_rows()
    m, om, omode = thirteen_metrics(za)[mi]
    rows = np.arange(N2)
    per = oracle_rows(X, rows, [i for i, _ in NEAR], om, omode)
    near_keys = np.array([ks[bs == j][0] for (i, j), (bs, ks) in zip(NEAR, per)], np.uint64)
    if omode == zo.PARITY and om == zo.COSINE:
        mk = threshold_from_sample(oracle_rows(X, rows, SAMPLE, om, omode), 3000, N2)
    else:
        mk = near_keys.max()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    got = check_path2(za, ix, X, m, om, omode, mk, monkeypatch, sample=PLANTED)
    have = set(zip(got[0].tolist(), got[1].tolist()))
    if not (omode == zo.PARITY and om == zo.COSINE):
        assert all(p in have for p in NEAR)
        assert all((200 + i, 300 + i) in have for i in range(20))


def test_rows_nothing_is_certain_about(za, monkeypatch):
    """one row with an infinite element and one whose |x|^2 overflows: nothing certain means always a candidate, and the canonical key decides.
    Compared against search_range_batch (the device's own arithmetic on both sides), not the oracle."""
    X = planted_rows().copy()
    X[700, 5] = np.inf
    X[701] = np.float32(1e30)
    for m in (za.L2SquaredDistance(), za.CosineDistance(parity=False)):
        om = zo.L2SQ if m.metric == 1 else zo.COSINE
        per = oracle_rows(X, np.arange(N2), [i for i, _ in NEAR], om, zo.CORRECTED if om == zo.COSINE else 0)
        mk = max(ks[bs == j][0] for (i, j), (bs, ks) in zip(NEAR, per))
        ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
        ix.append(X)
        monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
        got = ix.self_join(metric=m, max_key=mk)
        info = ix.join_info()
        assert info["path"] == 2 and info["redone"] == 0 and info["candidates"] >= 2 * (N2 - 2), info  # both rows' every pair was keyed
        same(got, range_reference(ix, X, mk, m))


# ---------------------------------------------------------------- removed rows, order, ids
def test_removed_rows_compact_and_id_base(za, monkeypatch):
    base = 1 << 40
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    ix.add(X)
    gone = np.array(list(range(80, 96, 3)) + list(range(112, 128)) + [N2 - 1])  # every third row of a tile, one whole tile, the last row
    ix.remove((gone + base).tolist())
    alive = np.ones(N2, bool)
    alive[gone] = False
    rows = np.flatnonzero(alive)
    sample = [a for a in SAMPLE if alive[a]] + [79, 81, 111, 128, N2 - 3]
    sample = sorted(set(sample))
    per = oracle_rows(X, rows, sample, om, omode)
    mk = threshold_from_sample(per, 3000, N2)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    got = ix.self_join(metric=m, max_key=mk)
    info = ix.join_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_live"] == rows.size, info
    assert not np.isin(got[0] - np.uint64(base), gone).any() and not np.isin(got[1] - np.uint64(base), gone).any()
    same(restrict(got, sample, base), pairs_from(sample, per, mk, base))
    same(got, range_reference(ix, X, mk, m, base, rows))  # (a removed row is no query: the reference asks for the live ones only)
    new_ids, _ = ix.compact()
    after = ix.self_join(metric=m, max_key=mk)
    same(after, (new_ids[(got[0] - np.uint64(base)).astype(np.int64)], new_ids[(got[1] - np.uint64(base)).astype(np.int64)], got[2]))


def test_scan_order_that_is_not_id_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): the pairs are still (min id, max id), in id order"""
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[0]
    plain = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    plain.append(X)
    mk = threshold_from_sample(oracle_rows(X, np.arange(N2), SAMPLE, om, omode), 3000, N2)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    ref = plain.self_join(metric=m, max_key=mk)
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(D2, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, D2, N2), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    got = ix.self_join(metric=m, max_key=mk)
    assert ix.join_info()["path"] == 2 and ix.join_info()["redone"] == 0
    same(got, ref)
    ix.close()


# ---------------------------------------------------------------- more than one panel
N3 = 16384 + 1024 + 21  # the copy is scanned in panels of 16384 positions: a second panel of 1045 rows, its last tile partial
GONE3 = np.array([5] + list(range(100, 116)) + [16390, 17000, N3 - 1])  # rows removed in both panels


@functools.lru_cache(maxsize=None)
def two_panel_rows():
    """the last 1045 rows are one tight cluster: at a radius far above its diameter and far below the distance of two unrelated rows, its
    ~545 000 pairs are the hits of the second panel -- more than that panel's candidate floor of 256 * 1045 slots"""
    X = zo.synth_rows(N3, D2).copy()
    c = X[16384].copy()
    X[16384:] = c + np.float32(1e-3) * X[:N3 - 16384]
    return X


def two_panel_key(za, m):
    c = two_panel_rows()[16384].astype(np.float64)
    return za.radius_key(m, 1e-3 * float(c @ c))


def check_two_panels(za, ix, X, m, rows, monkeypatch, under_row_order):
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    mk = two_panel_key(za, m)
    ref = range_reference(ix, X, mk, m, 0, rows)
    total = ref[0].size
    cluster = int((rows >= 16384).sum())
    assert total >= cluster * (cluster - 1) // 2 > 256 * 1045
    T = (N3 + 15) // 16
    # the exact capacity: both panels complete on path 2 (the pool left is 1.25 x the pairs still to come)
    rc, a, b, k, tot = raw_call(ix, mk, m, total)
    info = ix.join_info()
    assert rc == 0 and tot == total
    assert info["path"] == 2 and info["redone"] == 0 and info["launches"] == 2 and info["tiles"] == T * (T + 1) // 2, info
    assert info["rows_live"] == rows.size and info["pairs"] == total and info["candidates"] >= total, info
    same((a, b, k), ref)
    # count only: a panel's pool is its floor of 256 slots per row.  In id order the first panel has few candidates and completes, the second one
    # (the cluster) runs over and is redone by path 1 from the live rows before it on: redone == 1.  Under a row order a panel that runs over ends
    # path 2 and the whole call is answered by path 1, wherever the cluster's rows sit: redone <= 1, nothing counted twice or lost.
    assert ix.self_join_count(metric=m, max_key=mk) == total
    info = ix.join_info()
    assert info["path"] == 2 and info["pairs"] == total and (info["redone"] <= 1 if under_row_order else info["redone"] == 1), info
    # every pair admitted: each panel runs over
    L = rows.size
    assert ix.self_join_count(metric=m, max_key=ALL) == L * (L - 1) // 2
    info = ix.join_info()
    assert info["path"] == 2 and info["candidates"] == 0 and info["redone"] == (1 if under_row_order else 2), info
    # a first guess far too small (the second panel runs over on the first call), then the exact total
    same(ix.self_join(metric=m, max_key=mk, capacity=1000), ref)


def test_two_panels_with_removed_rows(za, monkeypatch):
    X = two_panel_rows()
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    ix.remove(GONE3.tolist())
    alive = np.ones(N3, bool)
    alive[GONE3] = False
    check_two_panels(za, ix, X, m, np.flatnonzero(alive), monkeypatch, False)


def test_two_panels_under_a_row_order(za, monkeypatch):
    """positions are not ids: a panel that runs over cannot be redone by row number (it owns its pairs by position), so the whole call goes
    to path 1 -- compared against search_range_batch like everything else"""
    X = two_panel_rows()
    m = za.L2SquaredDistance()
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(D2, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, D2, N3), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    ix.remove(GONE3.tolist())
    alive = np.ones(N3, bool)
    alive[GONE3] = False
    check_two_panels(za, ix, X, m, np.flatnonzero(alive), monkeypatch, True)
    ix.close()


# ---------------------------------------------------------------- pools
def test_many_pairs_from_one_panel(za, monkeypatch):
    """300 bit-identical rows: 44 850 pairs of key 0, all from the table's one panel.  The candidate pool holds max(1.25 x the capacity left,
    256 per row of the panel) = at least 256 * 8229 slots, and at threshold key 0 the candidates are the pairs whose interval reaches 0: the
    44 850 and at most a few more -- the pool does not run over, whatever the first capacity: redone == 0.  With every pair admitted and
    capacity 0 the pool is that floor, far below the 33.8 M pairs: the panel MUST be redone by path 1, which counts them all."""
    X = wide_rows(D2).copy()
    dup = np.sort(np.random.default_rng(5).choice(N2, 300, replace=False))
    X[dup] = X[dup[0]]
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    got = ix.self_join(metric=m, max_key=np.uint64(0), capacity=100)  # (the wrapper's second call has the exact total)
    info = ix.join_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["pairs"] == 300 * 299 // 2, info
    ia, ib = np.triu_indices(300, 1)
    same(got, (dup[ia].astype(np.uint64), dup[ib].astype(np.uint64), np.zeros(ia.size, np.uint64)))
    rc, _, _, _, tot = raw_call(ix, 0, m, 100)
    assert rc == ELIMIT and tot == 300 * 299 // 2 and ix.join_info()["redone"] == 0
    assert ix.self_join_count(metric=m, max_key=ALL) == N2 * (N2 - 1) // 2
    info = ix.join_info()
    assert info["path"] == 2 and info["redone"] == 1 and info["candidates"] == 0, info


def test_device_entry_point(za, monkeypatch):
    import torch
    X = wide_rows(D2)
    m, om, omode = thirteen_metrics(za)[3]
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    mk = threshold_from_sample(oracle_rows(X, np.arange(N2), SAMPLE, om, omode), 3000, N2)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    host = ix.self_join(metric=m, max_key=mk)
    total = host[0].size
    dev = torch.device("cuda", 0)
    for cap in (total, total + 100, total - 1, 0):
        a = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        b, keys = torch.zeros_like(a), torch.zeros_like(a)
        tot = torch.full((1,), 9, dtype=torch.int64, device=dev)
        try:
            ix.self_join_device(mk, m, cap, a.data_ptr() if cap else None, b.data_ptr() if cap else None, keys.data_ptr() if cap else None, tot.data_ptr())
            assert cap >= total
        except za.ZhError as e:
            assert e.code == ELIMIT and cap < total, e
        torch.cuda.synchronize()
        assert int(tot.cpu()[0]) == total
        if cap >= total:
            for t, h in zip((a, b, keys), host):
                assert (t.cpu().numpy().view(np.uint64)[:total] == h).all()


def test_siblings_are_left_alone(za):
    X = wide_rows(D2)
    Q = zo.synth_queries(8, D2, N2)
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    mask = np.zeros(N2, bool)
    mask[::2] = True
    ix.search_exact_batch(Q, 10, m)
    ix.search_exact_filtered_batch(Q, 10, m, mask)
    ix.search_range_batch(Q, 1.0, m)
    before = (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.stats())
    ix.self_join_count(metric=m, max_key=np.uint64(0))
    assert ix.join_info()["path"] == 2
    assert (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.stats()) == before


# ---------------------------------------------------------------- deduplicate_within, degenerate inputs, the full triangle
def test_deduplicate_within_chain(za):
    """a ~ b, b ~ c, a !~ c keeps a and c"""
    d = 30
    X = np.zeros((3, d), np.float32)
    X[1, 0], X[2, 0] = 1.0, 2.0  # distances: a-b 1, b-c 1, a-c 2
    m = za.L2Distance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    a, b, _ = ix.self_join(1.0, m)
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (1, 2)]
    assert ix.deduplicate_within(1.0, m).tolist() == [1]
    assert len(ix) == 2 and ix.self_join_count(1.0, m) == 0


def test_deduplicate_within_against_the_rule(za):
    X = small_rows()
    n = X.shape[0]
    m, om, omode = thirteen_metrics(za)[1]
    per_a = small_oracle(om, omode)
    mk = np.partition(np.concatenate([ks for _, ks in per_a]), 2999)[2999]
    radius = float(zo.key_to_float(np.array([mk], np.uint64))[0])
    assert za.radius_key(m, radius) == mk
    ra, rb, _ = pairs_from(list(range(n)), per_a, mk)
    partners = {}
    for a, b in zip(ra.tolist(), rb.tolist()):
        partners.setdefault(b, []).append(a)
    kept, removed = set(), []
    for r in range(n):  # the rule, restated: in ascending id, r goes exactly when a kept earlier row is paired with it
        if any(a in kept for a in partners.get(r, ())):
            removed.append(r)
        else:
            kept.add(r)
    db = za.Database(30, za.L2Distance, za.LSHIndexOptions(64, 4), device=0)
    db.insert_records(X, ["doc%d" % i for i in range(n)])
    trip = db.near_duplicates(radius)
    assert [(x, y) for x, y, _ in trip] == [("doc%d" % a, "doc%d" % b) for a, b in zip(ra.tolist(), rb.tolist())]
    assert all(0.0 <= v <= radius for _, _, v in trip)
    assert db.deduplicate_within(radius).tolist() == removed and len(removed) > 0
    assert len(db.index) == n - len(removed) and all(("doc%d" % r) not in db._documents.values() for r in removed)
    # what is left holds no kept pair any more
    ka, kb, _ = db.index.self_join(radius, db.metric)
    assert ka.size == 0 and kb.size == 0


def test_degenerate_inputs(za):
    d = 30
    X = small_rows()
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)

    def nothing(rows_live):
        a, b, k = ix.self_join(metric=m, max_key=ALL)
        assert a.size == 0 and b.size == 0 and k.size == 0 and ix.self_join_count(metric=m, max_key=ALL) == 0
        rc, _, _, _, tot = raw_call(ix, ALL, m, 0, with_arrays=False)
        assert rc == 0 and tot == 0
        assert ix.join_info() == {"rows_live": rows_live, "pairs": 0, "path": 1, "redone": 0, "candidates": 0, "launches": 0, "tiles": 0}

    nothing(0)  # an empty index
    ix.append(X[:1])
    nothing(1)  # one row
    ix.append(X[1:50])
    ix.remove(list(range(50)))
    nothing(0)  # removed rows only
    ix.append(X[50:52])
    a, b, _ = ix.self_join(metric=m, max_key=ALL)
    assert a.tolist() == [50] and b.tolist() == [51]


def test_full_triangle(za):
    n = 300
    X = small_rows()[:n]
    m, om, omode = thirteen_metrics(za)[0]
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    ix.remove([7, 150])
    rows = np.array([r for r in range(n) if r not in (7, 150)])
    L = rows.size
    got = ix.self_join(metric=m, max_key=ALL)
    assert got[0].size == L * (L - 1) // 2
    same(got, pairs_from(rows.tolist(), oracle_rows(X, rows, rows.tolist(), om, omode), ALL))


@pytest.mark.parametrize("name", ["l2sq", "cos_corrected"])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, name):
    """the held-tile walk (zh_device.h) at its edges, against the family fuzz's reference: 8200 rows are 513 = 8 x 64 + 1 tiles, so the first
    held block walks eight full chunks of ZH_JOIN_CHUNK = 64 tiles (even: the last tile in the second LDS buffer) and a chunk of ONE tile (odd,
    no prefetch at all), the later blocks' last chunks have 61, 57, ... tiles, in every first chunk waves 1 to 3 skip the tiles before their
    diagonal, and the last held block holds one tile of 8 rows: three idle waves.  Near-duplicates are planted so that the one-tile chunk and
    the last block's diagonal tile both have pairs"""
    from tests import family_cases as fc
    n = 8200
    spec = fc.metric_spec(name)
    m = za.L2SquaredDistance() if name == "l2sq" else za.CosineDistance(parity=False)
    X = wide_rows(D2)[:n].copy()
    X[8195], X[8199] = X[20] * np.float32(1.0 + 2.0**-12), X[8193] * np.float32(1.0 + 2.0**-12)
    sample = np.array([0, 20, 33, 63, 64, 250, 4097, 8191, 8192, 8193, 8198])
    alive = np.ones(n, bool)
    K = fc.key_matrix(spec, X, X[sample])
    upper = np.arange(n)[None, :] > sample[:, None]
    mk = fc.quantile_threshold(K, upper, 3000, n * (n - 1) / 2)
    ref = fc.join_ref(K, sample, alive, alive, mk, 0, 0, True)
    assert ((ref[0] == 20) & (ref[1] == 8195)).any() and ((ref[0] == 8193) & (ref[1] == 8199)).any()
    ix = za.LSHIndex(D2, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    got = ix.self_join(metric=m, max_key=mk)
    info = ix.join_info()
    assert info["path"] == 2 and info["redone"] == 0 and info["tiles"] == 513 * 514 // 2 and info["launches"] == 1, info
    assert (got[0] < got[1]).all() and info["pairs"] == got[0].size
    same(fc.restrict(got, sample, 0), ref)

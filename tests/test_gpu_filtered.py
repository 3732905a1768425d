"""The filtered exact search (zh_search_exact_filtered_batch): the exact top-k among the live rows a caller's bitmap allows.  Every comparison
is bit-exact on ids, keys and counts against the oracle's brute force over X[allowed & alive] with the ids mapped back -- the answer of an
index that held only those rows.  Shapes are the smallest that reach each mechanism (thresholds as in zh_api.hip: path 2 wants max(k, 8192)
allowed rows, its chunks are made of blocks of 8192 positions, an internal batch is 1024 queries)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

NONE = np.uint64(2**64 - 1)
EINVAL = -1


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


def same_keys(got, want, om):
    """bit-equal, or both NaN: a NaN key's sign bit differs between the host's and the GPU's arithmetic (as in test_gpu_exact)"""
    if om < zo.CHEBYSHEV:
        nan = np.isnan(got.view(np.float64)) & np.isnan(want.view(np.float64))
    else:
        nan = np.isnan(got.astype(np.uint32).view(np.float32)) & np.isnan(want.astype(np.uint32).view(np.float32))
    return (got == want) | nan


def brute(X, rows, Q, k, om, omode):
    """the oracle's answer over X[rows] (rows ascending: allowed and alive), ids mapped back to stored rows -> per query (ids, keys)"""
    if len(rows) == 0:
        return [(np.zeros(0, np.uint64), np.zeros(0, np.uint64))] * Q.shape[0]
    Xs = np.ascontiguousarray(X[rows])
    out = []
    for b in range(Q.shape[0]):
        oi, ok = zo.brute_force(Xs, Q[b], k, om, omode)
        out.append((rows[oi.astype(np.int64)].astype(np.uint64), ok))
    return out


def check(got, ref, k, om, id_base=0):
    """got = (ids, keys, counts) for top_k = k; ref = brute(...) for some top_k >= k (its prefix is the top-k: the order is (key, id))"""
    ids, keys, counts = got
    assert ids.shape[1] == k
    for b, (oi, ok) in enumerate(ref):
        n = min(k, len(oi))
        assert counts[b] == n, (b, counts[b], n)
        assert (ids[b, :n] == oi[:n] + np.uint64(id_base)).all(), b
        assert same_keys(keys[b, :n], ok[:n], om).all(), b
        assert (ids[b, n:] == NONE).all() and (keys[b, n:] == NONE).all(), b


def random_half(n, seed=11):
    return np.random.default_rng(seed).random(n) < 0.5


@pytest.mark.parametrize("d", [3, 128])
def test_path1_every_metric(za, d):
    n, k = 20000, 100
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(3, d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    every = np.zeros(n, bool)
    every[::1000] = True
    one = np.zeros(n, bool)
    one[12345] = True
    masks = [random_half(n), every, one, np.ones(n, bool), np.zeros(n, bool)]
    for mask in masks:
        rows = np.flatnonzero(mask)
        for m, om, omode in thirteen_metrics(za):
            got = ix.search_exact_filtered_batch(Q, k, m, mask)
            info = ix.filtered_info()
            assert info["rows_allowed"] == len(rows) and info["rows_live"] == n and info["path"] == 1 and info["batch"] == 3, info
            check(got, brute(X, rows, Q, k, om, omode), k, om)
    # the same filter as ids, and one query
    m, om, omode = thirteen_metrics(za)[0]
    got = ix.search_exact_filtered_batch(Q, k, m, np.flatnonzero(every).astype(np.uint64))
    ref = brute(X, np.flatnonzero(every), Q, k, om, omode)
    check(got, ref, k, om)
    pairs = ix.search_exact_filtered(Q[1], 5, m, every)
    assert [p[0] for p in pairs] == ref[1][0][:5].tolist() and [p[1] for p in pairs] == ref[1][1][:5].tolist()


def test_removals_id_base_and_short_filter(za):
    d, n, base = 128, 9000, 1 << 40
    X = zo.synth_rows(n, d)
    X[500:900] = X[400]  # a planted run for deduplicate
    Q = zo.synth_queries(5, d, n)
    m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    # an empty index: counts 0, every slot 2^64 - 1
    ids, keys, counts = ix.search_exact_filtered_batch(Q, 10, m, np.zeros(0, bool))
    assert (counts == 0).all() and (ids == NONE).all() and (keys == NONE).all()
    ix.add(X)
    alive = np.ones(n, bool)
    gone = np.arange(0, n, 7)
    ix.remove((gone + base).tolist())
    alive[gone] = False
    ix.deduplicate()
    alive &= ~zo.find_duplicates(X, alive.astype(np.uint8))
    # a mask shorter than the table (rows past it are not allowed) that also allows removed rows
    mask = np.zeros(6000, bool)
    mask[::3] = True       # row 0, 21, 42 ... were removed
    mask[450:1000] = True  # the planted run: all but its first row deduplicated away
    assert (mask & ~alive[:6000]).any()
    full = np.zeros(n, bool)
    full[:6000] = mask
    rows = np.flatnonzero(full & alive)
    check(ix.search_exact_filtered_batch(Q, 50, m, mask), brute(X, rows, Q, 50, om, omode), 50, om, id_base=base)
    info = ix.filtered_info()
    assert info["rows_allowed"] == len(rows) and info["rows_live"] == int(alive.sum()), info
    # the same filter by id
    check(ix.search_exact_filtered_batch(Q, 50, m, np.flatnonzero(full).astype(np.uint64) + np.uint64(base)),
          brute(X, rows, Q, 50, om, omode), 50, om, id_base=base)
    # k above the allowed live rows: counts say how many there are
    few = np.zeros(3000, bool)
    few[[0, 1, 2, 3, 10, 14, 700, 2999]] = True  # 0, 14 removed; 700 a duplicate
    frows = np.flatnonzero(np.concatenate([few, np.zeros(n - 3000, bool)]) & alive)
    got = ix.search_exact_filtered_batch(Q, 30, m, few)
    assert (got[2] == len(frows)).all() and len(frows) == 5
    check(got, brute(X, frows, Q, 30, om, omode), 30, om, id_base=base)
    # k = 0, k above the limit, a mask longer than the table
    assert (ix.search_exact_filtered_batch(Q, 0, m, mask)[2] == 0).all()
    with pytest.raises(za.ZhError) as e:
        ix.search_exact_filtered_batch(Q, 1025, m, mask)
    assert e.value.code == -5
    with pytest.raises(za.ZhError) as e:
        ix.search_exact_filtered_batch(Q, 10, m, np.ones(n + 1, bool))
    assert e.value.code == EINVAL
    # after compact the rows have new numbers: a fresh mask in the new ids answers for the compacted table
    ix.compact()
    live = np.flatnonzero(alive)
    Xc = X[live]
    assert ix.stored_rows() == len(live)
    with pytest.raises(za.ZhError) as e:  # the old mask of the whole table speaks for more rows than there are now
        ix.search_exact_filtered_batch(Q, 10, m, full)
    assert e.value.code == EINVAL
    cmask = random_half(len(live), seed=3)
    check(ix.search_exact_filtered_batch(Q, 50, m, cmask), brute(Xc, np.flatnonzero(cmask), Q, 50, om, omode), 50, om, id_base=base)


@functools.lru_cache(maxsize=None)
def half_case(d):
    """the path-2 random-half case: rows, queries, mask and the oracle's top-1024 per simsimd metric / mode (computed once, never changed)"""
    n, B = 60000, 8
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    mask = random_half(n)
    rows = np.flatnonzero(mask)
    refs = {(om, omode): brute(X, rows, Q, 1024, om, omode) for om, omode in ((zo.L2SQ, 0), (zo.L2, 0), (zo.COSINE, zo.PARITY), (zo.COSINE, zo.CORRECTED))}
    return X, Q, mask, refs


def run_half_case(za, ix, d):
    X, Q, mask, refs = half_case(d)
    for m, om, omode in thirteen_metrics(za)[:4]:
        for k in (10, 1024):
            got = ix.search_exact_filtered_batch(Q, k, m, mask)
            info = ix.filtered_info()
            assert info["path"] == 2 and info["redone"] == 0 and info["rows_allowed"] == int(mask.sum()), (k, info)
            assert info["launches"] >= 2 and info["survivors"] >= k * Q.shape[0], (k, info)
            check(got, refs[(om, omode)], k, om)


@pytest.mark.parametrize("d", [256, 768])
def test_path2_random_half(za, d):
    X = half_case(d)[0]
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    run_half_case(za, ix, d)


def test_path2_filter_in_the_tail(za):
    """every allowed row sits in the second half of the table.  Chunks placed by POSITION would reach it with a huge chunk and no bound
    (every allowed row listed: the lists run over, redone > 0); placed by the count of allowed rows the first chunk ends 4096 allowed rows
    into the tail.  The odd start leaves a partly masked tile on the edge; the 6250 tiles before it are skipped unloaded."""
    d, n, lo, k, B = 256, 200_000, 100_003, 100, 8
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    mask = np.zeros(n, bool)
    mask[lo:] = True
    got = ix.search_exact_filtered_batch(Q, k, za.L2SquaredDistance(), mask)
    info = ix.filtered_info()
    print(info)
    assert info["path"] == 2 and info["redone"] == 0 and info["rows_allowed"] == n - lo, info
    assert info["tiles_skipped"] >= 100_000 // 16 - 1, info
    check(got, brute(X, np.flatnonzero(mask), Q, k, zo.L2SQ, 0), k, zo.L2SQ)


def test_sparse_filter_takes_path1(za):
    """600 allowed rows on an index whose unfiltered search takes path 2: below the 8192 rows path 2 needs, so the list is gathered by path 1 in
    ONE row-chunk launch (path 2 over the table would be three chunks or more)"""
    d, n, k = 256, 60000, 10
    X, Q = half_case(d)[0], half_case(d)[1]
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    ix.search_exact_batch(Q, k, za.L2SquaredDistance())
    assert ix.exact_info()["path"] == 2 and ix.exact_info()["launches"] >= 3
    mask = np.zeros(n, bool)
    mask[::100] = True
    got = ix.search_exact_filtered_batch(Q, k, za.L2SquaredDistance(), mask)
    info = ix.filtered_info()
    assert info["path"] == 1 and info["rows_allowed"] == 600 and info["launches"] == 1 and info["tiles_skipped"] == 0, info
    check(got, brute(X, np.flatnonzero(mask), Q, k, zo.L2SQ, 0), k, zo.L2SQ)


def test_path2_under_a_row_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): the mask is permuted once per call and still names the right rows"""
    d = 256
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    X, Q = half_case(d)[0], half_case(d)[1]
    ix = za.LSHIndex(d, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(Q, 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    run_half_case(za, ix, d)
    assert ix.stats()["scan_order_keys"] == 2
    ix.close()


def test_device_entry_point_and_batch_split(za):
    import torch
    d, n, B, k = 768, 20000, 1100, 20  # B > the internal batch of 1024: split
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    Q = zo.synth_queries(B, d, n)
    mask = random_half(n, seed=5)
    m = za.CosineDistance(parity=False)
    hi, hk, hc = ix.search_exact_filtered_batch(Q, k, m, mask)
    hinfo = ix.filtered_info()
    assert hinfo["batch"] == B and hinfo["rows_allowed"] == int(mask.sum())
    words, n_bits = ix.filter_bitmap(mask)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    df = torch.from_numpy(words.view(np.int32)).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys = torch.empty_like(ids)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ix.search_exact_filtered_batch_device(dq.data_ptr(), B, k, m, df.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    assert (ids.cpu().numpy().view(np.uint64) == hi).all() and (keys.cpu().numpy().view(np.uint64) == hk).all()
    assert (counts.cpu().numpy().view(np.uint32) == hc).all()
    assert ix.filtered_info() == hinfo
    X = zo.synth_rows(n, d)
    rows = np.flatnonzero(mask)
    check((hi[:4], hk[:4], hc[:4]), brute(X, rows, Q[:4], k, zo.COSINE, zo.CORRECTED), k, zo.COSINE)
    check((hi[-3:], hk[-3:], hc[-3:]), brute(X, rows, Q[-3:], k, zo.COSINE, zo.CORRECTED), k, zo.COSINE)


def test_neighbours_undisturbed(za):
    """a filtered call between two unfiltered ones changes neither their answers nor zh_exact_info, and leaves the LSH search alone; the
    all-ones filter gives the unfiltered answer"""
    d, n, B, k = 384, 20000, 16, 10
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 8), device=0)
    ix.add(X)
    ix.remove(list(range(5, n, 50)))
    m = za.L2SquaredDistance()
    lsh_before = ix.search_batch(Q, k, m)
    ex_before = ix.search_exact_batch(Q, k, m)
    einfo = ix.exact_info()
    stats = ix.stats()
    filt = ix.search_exact_filtered_batch(Q, k, m, random_half(n))
    ones = ix.search_exact_filtered_batch(Q, k, m, np.ones(n, bool))
    assert ix.filtered_info()["rows_allowed"] == len(ix) and ix.filtered_info()["path"] == 2
    assert ix.exact_info() == einfo and ix.stats() == stats
    ex_after = ix.search_exact_batch(Q, k, m)
    assert ix.exact_info() == einfo
    lsh_after = ix.search_batch(Q, k, m)
    assert all((a == b).all() for a, b in zip(ex_before, ex_after))
    assert all((a == b).all() for a, b in zip(ex_before, ones))
    assert all((a == b).all() for a, b in zip(lsh_before, lsh_after))
    assert not (filt[0] == ex_before[0]).all()


def test_database_query_vectors_where(za):
    d, n, B, k = 32, 3000, 4, 5
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    db = za.Database(d, za.L2SquaredDistance, za.LSHIndexOptions(64, 4), device=0)
    docs = [{"lang": ("de", "en", "fr")[i % 3], "n": i} for i in range(n)]
    db.insert_records(X, docs)
    db.remove([3, 6, 9])
    got = db.query_vectors_where(Q, k, lambda doc: doc["lang"] == "de")
    want_rows = np.array([i for i in range(n) if i % 3 == 0 and i not in (3, 6, 9)])
    ids, _, counts = db.index.search_exact_filtered_batch(Q, k, db.metric, want_rows.astype(np.uint64))
    ref = brute(X, want_rows, Q, k, zo.L2SQ, 0)
    assert sorted(got) == list(range(B))
    for b in range(B):
        assert counts[b] == k and list(got[b]) == ids[b].tolist() == ref[b][0].tolist()
        assert all(doc["lang"] == "de" and doc["n"] == i for i, doc in got[b].items())
    assert db.query_vectors_where(Q, k, lambda doc: doc["lang"] == "xx") == {b: {} for b in range(B)}

"""The exact search (zh_search_exact_batch): every live row ranked with the library's keys.  Every comparison is bit-exact on ids,
keys and counts against the oracle's brute force (zo.brute_force: the reference's arithmetic, ranked by (key, id)), query by query."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def all_metrics(za):
    """the 13 metric / mode combinations, Minkowski / PNorm at powers that reach every branch of the root"""
    out = [(za.L2SquaredDistance(), zo.L2SQ, 0), (za.L2Distance(), zo.L2, 0), (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
           (za.CosineDistance(parity=False), zo.COSINE, zo.CORRECTED), (za.ChebyshevDistance(), zo.CHEBYSHEV, 0),
           (za.CanberraDistance(), zo.CANBERRA, 0), (za.BrayCurtisDistance(), zo.BRAY_CURTIS, 0), (za.ManhattanDistance(), zo.MANHATTAN, 0),
           (za.L3Distance(), zo.L3, 0), (za.L4Distance(), zo.L4, 0), (za.HammingDistance(), zo.HAMMING, 0)]
    for p in (0, -1, 3, 65, -2**31):
        out += [(za.MinkowskiDistance(p), zo.MINKOWSKI, p), (za.PNormDistance(p), zo.PNORM, p)]
    return out


def same_keys(got, want, om):
    """bit-equal, or both NaN: a NaN key's sign bit differs between the host's and the GPU's arithmetic (as in test_gpu_parity)"""
    if om < zo.CHEBYSHEV:
        nan = np.isnan(got.view(np.float64)) & np.isnan(want.view(np.float64))
    else:
        nan = np.isnan(got.astype(np.uint32).view(np.float32)) & np.isnan(want.astype(np.uint32).view(np.float32))
    return (got == want) | nan


def check_exact(got, X, Q, k, om, omode, ids_of=None, id_base=0):
    """got = (ids, keys, counts) of search_exact_batch; X the live rows; ids_of maps a row of X to its stored row (removals)"""
    ids, keys, counts = got
    for b in range(Q.shape[0]):
        oi, ok = zo.brute_force(X, Q[b], k, om, omode)
        if ids_of is not None:
            oi = ids_of[oi.astype(np.int64)].astype(np.uint64)
        n = len(oi)
        assert counts[b] == n, (b, counts[b], n)
        assert (ids[b, :n] == oi + np.uint64(id_base)).all(), b
        assert same_keys(keys[b, :n], ok, om).all(), b
        assert (ids[b, n:] == np.uint64(2**64 - 1)).all() and (keys[b, n:] == np.uint64(2**64 - 1)).all(), b


@pytest.mark.parametrize("d", [1, 3, 100, 128])
def test_all_metrics(za, d):
    n = 20000
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(3, d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    for m, om, omode in all_metrics(za):
        got100 = ix.search_exact_batch(Q, 100, m)
        assert ix.exact_info()["path"] == 1 and ix.exact_info()["rows_live"] == n
        check_exact(got100, X, Q, 100, om, omode)
        for k in (1, 10):  # the (key, id) order makes the top-k a prefix of the top-100
            ids, keys, counts = ix.search_exact_batch(Q, k, m)
            assert (counts == k).all()
            assert (ids == got100[0][:, :k]).all() and (keys == got100[1][:, :k]).all()


@pytest.mark.parametrize("d", [256, 768, 1024])
def test_simsimd_metrics_wide(za, d):
    n, B = 30000 if d < 1024 else 20000, 8
    X = zo.synth_rows(n, d, kind=2)
    Q = zo.synth_queries(B, d, n, kind=2)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n, kind=2)
    for m, om, omode in all_metrics(za)[:4]:
        got = ix.search_exact_batch(Q, 1024, m)
        check_exact(got, X, Q, 1024, om, omode)
        ids, keys, counts = ix.search_exact_batch(Q, 10, m)
        assert (ids == got[0][:, :10]).all() and (keys == got[1][:, :10]).all() and (counts == 10).all()


def test_degenerate_rows_and_queries(za):
    """thousands of duplicate rows, a query with a NaN, rows of huge magnitude: still the brute force's answer"""
    d, n = 384, 12000
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[1000:6000] = X[999]
    X[7000:7100] *= np.float32(1e30)
    X[7200] = 0
    Q = np.concatenate([X[999:1000], rng.standard_normal((2, d)).astype(np.float32), X[7000:7001]])
    Q[1, 5] = np.nan
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    for m, om, omode in all_metrics(za)[:8]:
        check_exact(ix.search_exact_batch(Q, 100, m), X, Q, 100, om, omode)


def test_removals_id_base_and_edges(za):
    d, n, base = 128, 9000, 1 << 40
    X = zo.synth_rows(n, d)
    X[500:900] = X[400]  # duplicates for deduplicate
    Q = zo.synth_queries(5, d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
    # empty index: counts 0, every slot UINT64_MAX
    ids, keys, counts = ix.search_exact_batch(Q, 10, m)
    assert (counts == 0).all() and (ids == np.uint64(2**64 - 1)).all() and (keys == np.uint64(2**64 - 1)).all()
    ix.add(X)
    alive = np.ones(n, bool)
    gone = np.arange(0, n, 7)
    ix.remove((gone + base).tolist())
    alive[gone] = False
    ix.deduplicate()
    alive &= ~zo.find_duplicates(X, alive.astype(np.uint8))
    live = np.flatnonzero(alive)
    assert ix.exact_info()["batch"] == 5 and ix.exact_info()["rows_live"] == 0
    check_exact(ix.search_exact_batch(Q, 50, m), X[live], Q, 50, om, omode, ids_of=live, id_base=base)
    assert ix.exact_info()["rows_live"] == len(live)
    # k = 0: no neighbours; k > ZH_MAX_TOPK: ZH_ELIMIT
    ids, keys, counts = ix.search_exact_batch(Q, 0, m)
    assert (counts == 0).all()
    with pytest.raises(za.ZhError) as e:
        ix.search_exact_batch(Q, 1025, m)
    assert e.value.code == -5
    # k above the live rows: a small index
    small = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=3)
    small.append(X[:20])
    small.remove([3 + 4])
    sl = np.array([i for i in range(20) if i != 4])
    got = small.search_exact_batch(Q, 30, m)
    assert (got[2] == 19).all()
    check_exact(got, X[sl], Q, 30, om, omode, ids_of=sl, id_base=3)


def test_device_entry_point_and_host_split(za):
    import torch
    d, n, B, k = 768, 20000, 1100, 20  # B > the internal batch: split
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    Q = zo.synth_queries(B, d, n)
    m = za.CosineDistance(parity=False)
    hi, hk, hc = ix.search_exact_batch(Q, k, m)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys = torch.empty_like(ids)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ix.search_exact_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    assert (ids.cpu().numpy().view(np.uint64) == hi).all() and (keys.cpu().numpy().view(np.uint64) == hk).all()
    assert (counts.cpu().numpy().view(np.uint32) == hc).all()
    X = zo.synth_rows(n, d)
    check_exact((hi[:4], hk[:4], hc[:4]), X, Q[:4], k, zo.COSINE, zo.CORRECTED)
    check_exact((hi[-3:], hk[-3:], hc[-3:]), X, Q[-3:], k, zo.COSINE, zo.CORRECTED)


def test_shards_merge_to_the_union(za):
    import torch
    d, n, S, B, k = 256, 16000, 4, 6, 32
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.empty((S, B, k), dtype=torch.int64, device=dev)
    keys = torch.empty_like(ids)
    counts = torch.empty((S, B), dtype=torch.int32, device=dev)
    per = n // S
    shards = []
    for s in range(S):
        sh = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=s * per)
        sh.append(X[s * per:(s + 1) * per])
        sh.search_exact_batch_device(dq.data_ptr(), B, k, za.L2Distance(), ids[s].data_ptr(), keys[s].data_ptr(), counts[s].data_ptr())
        shards.append(sh)
    oids, okeys = torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev)
    ocounts = torch.empty(B, dtype=torch.int32, device=dev)
    za.merge_topk_device(0, S, B, k, ids.data_ptr(), keys.data_ptr(), counts.data_ptr(), oids.data_ptr(), okeys.data_ptr(), ocounts.data_ptr())
    torch.cuda.synchronize()
    got = (oids.cpu().numpy().view(np.uint64), okeys.cpu().numpy().view(np.uint64), ocounts.cpu().numpy().view(np.uint32))
    check_exact(got, X, Q, k, zo.L2, 0)


def test_search_undisturbed_and_threads(za):
    d, n, B, k = 384, 20000, 16, 10
    X = zo.synth_rows(n, d)
    Q = zo.synth_queries(B, d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 8), device=0)
    ix.add(X)
    m = za.L2SquaredDistance()
    before = ix.search_batch(Q, k, m)
    ex = ix.search_exact_batch(Q, k, m)
    check_exact(ex, X, Q, k, zo.L2SQ, 0)
    after = ix.search_batch(Q, k, m)
    assert all((a == b).all() for a, b in zip(before, after))
    # 8 threads mix exact and LSH searches on one index: each gets its single-threaded answer
    errors = []

    def work(t):
        try:
            for i in range(6):
                q = Q[(t + i) % B:(t + i) % B + 1]
                b = (t + i) % B
                if (t + i) % 2:
                    got = ix.search_exact_batch(q, k, m)
                    ref = ex
                else:
                    got = ix.search_batch(q, k, m)
                    ref = before
                if not ((got[0][0] == ref[0][b]).all() and (got[1][0] == ref[1][b]).all() and got[2][0] == ref[2][b]):
                    errors.append((t, i))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_scale_1m_768(za):
    d, n, B, k = 768, 1_000_000, 16, 100
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    Q = zo.synth_queries(B, d, n)
    got = ix.search_exact_batch(Q, k, za.L2SquaredDistance())
    info = ix.exact_info()
    assert info["rows_live"] == n and info["batch"] == B and info["launches"] >= 1 and info["path"] == 2 and info["redone"] == 0
    X = zo.synth_rows(n, d)
    check_exact(got, X, Q, k, zo.L2SQ, 0)


@pytest.mark.parametrize("d,kind", [(256, 2), (768, 0), (1024, 2)])
def test_path2_matrix_core(za, d, kind):
    """L2SQ, L2 and both cosine modes on the matrix-core path: 200k rows, 64 queries, k = 1024 checked against the oracle for 16 of them (the
    (key, id) order makes k = 1, 10, 100 prefixes of it).  Survivors per query -- rows whose interval could not be told from the k-th key --
    stay below 4 k + 1024 for the L2 family and corrected cosine: the interval's half-width (zh_approx_bound plus the measured fp16 rounding of
    rows and queries) is a few 1e-4 of the key, far below the gap between neighbouring keys near the k-th on these rows.  The literal cosine
    key (PARITY) ranks by similarity, which clusters near 0 where no interval decides its sign: up to 3 % of the rows (measured below 1 %)."""
    n, B, nchk = 200_000, 64, 16
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n, kind=kind)
    X = zo.synth_rows(n, d, kind=kind)
    Q = zo.synth_queries(B, d, n, kind=kind)
    for m, om, omode in all_metrics(za)[:4]:
        got = ix.search_exact_batch(Q, 1024, m)
        info = ix.exact_info()
        bound = 0.03 * n if (om == zo.COSINE and omode == zo.PARITY) else 4 * 1024 + 1024
        assert info["path"] == 2 and info["redone"] == 0, info
        assert info["survivors"] / B <= bound, info
        check_exact(tuple(a[:nchk] for a in got), X, Q[:nchk], 1024, om, omode)
        for k in (1, 10, 100):
            ids, keys, counts = ix.search_exact_batch(Q, k, m)
            info = ix.exact_info()
            assert info["path"] == 2 and info["redone"] == 0, (k, info)
            bound = 0.03 * n if (om == zo.COSINE and omode == zo.PARITY) else 4 * k + 1024
            assert info["survivors"] / B <= bound, (k, info)
            assert (counts == k).all() and (ids == got[0][:, :k]).all() and (keys == got[1][:, :k]).all(), k


def test_path2_lists_run_over(za):
    """40k identical rows (identical intervals: all of them stay inside tau) and a query with a NaN (every interval 'nothing certain'): the
    per-query lists run over, the internal batch is answered by path 1 (redone > 0), and the answers are still the brute force's"""
    d, n = 256, 60000
    X = zo.synth_rows(n, d)
    X[1000:41000] = X[999]
    Q = np.concatenate([X[999:1000] + np.float32(0.01), zo.synth_queries(2, d, n)])
    Q[2, 7] = np.nan
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    for m, om, omode in all_metrics(za)[:4]:
        got = ix.search_exact_batch(Q, 100, m)
        info = ix.exact_info()
        assert info["path"] == 2 and info["redone"] >= 1, info
        check_exact(got, X, Q, 100, om, omode)
    # the batch without them stays on path 2
    got = ix.search_exact_batch(Q[1:2], 100, za.L2SquaredDistance())
    assert ix.exact_info()["redone"] == 0 and ix.exact_info()["path"] == 2
    check_exact(got, X, Q[1:2], 100, zo.L2SQ, 0)

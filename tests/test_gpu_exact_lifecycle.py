"""The exact search's matrix-core path (path 2: L2SQ, L2 and cosine at d = 256 .. 1024, at least max(k, 8192) live rows) across the life of an
index.  Path 2 reads the index's fp16 row copy (ensure_row_half), the same copy the matrix-core LSH scan reads, and masks removed rows with a
live-row bitmap.  Here that copy changes state under it: the meta-only state and back, removals and duplicates, the scan's row order (positions
= perm[p], rows appended after the order at position = id, a stale order, a new forest, clear + refill), row counts around the 16-row tiles,
the row chunks and the 8192-row threshold, and rows whose fp16 scale is out of range.

Every comparison is bit-exact on ids, keys and counts: the exact search against the oracle's brute force (check_exact), the LSH search under
sweep mode "approx" against an oracle forest kept in step with the index (check).  exact_info()["path"] is asserted at every step, so that a
search that fell back to path 1 cannot pass as a path-2 test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker)
from tests.test_gpu_approx import _adversarial_rows, check  # noqa: E402
from tests.test_gpu_exact import all_metrics, check_exact, same_keys  # noqa: E402
from tests.test_gpu_intervals import special_queries, special_rows  # noqa: E402


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def path2_metrics(za):
    return all_metrics(za)[:4]  # L2SQ, L2, cosine (parity), cosine (corrected)


def exact_path(ix, want, redone=0):
    info = ix.exact_info()
    assert info["path"] == want and info["redone"] == redone, info
    return info


def check_rows(ix, Q, rows, k, m, om, omode, X, ids_of=None, id_base=0):
    """the exact search of the whole batch; the brute force for the queries `rows` only"""
    got = ix.search_exact_batch(Q, k, m)
    sel = np.asarray(rows)
    check_exact(tuple(a[sel] for a in got), X, Q[sel], k, om, omode, ids_of=ids_of, id_base=id_base)
    return got


def check_ks(ix, Q, rows, ks, m, om, omode, X, path, ids_of=None, id_base=0):
    """the largest k against the brute force, every smaller k a prefix of it (the (key, id) order), each on the expected path"""
    kmax = max(ks)
    got = check_rows(ix, Q, rows, kmax, m, om, omode, X, ids_of, id_base)
    exact_path(ix, path)
    for k in ks:
        if k == kmax:
            continue
        ids, keys, counts = ix.search_exact_batch(Q, k, m)
        exact_path(ix, path)
        n = min(k, X.shape[0])
        assert (counts == n).all(), (k, counts)
        assert (ids[:, :n] == got[0][:, :n]).all() and same_keys(keys[:, :n], got[1][:, :n], om).all(), k


@pytest.mark.parametrize("how", ["append", "add"])
@pytest.mark.parametrize("d", [512, 768])
def test_copy_is_whole_after_meta_only(za, monkeypatch, d, how):
    """An index in the meta-only state (ZH_ROW_HALF_META_ONLY=1, or no room for the copy) keeps per-row scales and norms only.  Once rows are
    appended and the copy fits again, the copy must hold EVERY row: one made only from the appended rows leaves tiles [0, old n) unwritten,
    and both the exact path 2 and the LSH scan would prune true neighbours on intervals built from them."""
    monkeypatch.delenv("ZH_ROW_ORDER", raising=False)
    monkeypatch.setenv("ZH_ROW_HALF_META_ONLY", "1")
    seed = 0x5EB2B000 + d + (1 if how == "add" else 0)  # (rows no earlier index of the process held a copy of)
    n, n2, M, T, B, k, kl = 20005, 3000, 256, 6, 8, 100, 10
    Xall = zo.synth_rows(n + n2, d, seed=seed)
    X = Xall[:n]
    Q = np.concatenate([zo.synth_queries(B // 2, d, n, seed_rows=seed), zo.synth_queries(B // 2, d, n + n2, seed_rows=seed, b0=B // 2)])
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.set_hash_mode("dense")
    f = zo.Forest.build(X, M, T)
    m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
    st = check(ix, f, Q, kl, m, om, omode, "meta-only")
    assert st["approx_scan"] == 2 and 0 < st["row_copy_bytes"] < n * d, st
    check_exact(ix.search_exact_batch(Q, k, m), X, Q, k, om, omode)
    exact_path(ix, 1)
    assert ix.stats()["row_copy_bytes"] < n * d
    # room again, rows appended: the copy is made, all of it -- by the exact path after `append`, by the LSH scan after `add`
    monkeypatch.delenv("ZH_ROW_HALF_META_ONLY")
    N = n + n2
    assert N % 16

    def exact_all():
        for mm, omm, omo in path2_metrics(za):
            check_exact(ix.search_exact_batch(Q, k, mm), Xall, Q, k, omm, omo)
            exact_path(ix, 2)
        assert ix.stats()["row_copy_bytes"] >= N * (2 * d + 8)

    def lsh_all(f):
        for mm, omm, omo in (path2_metrics(za)[0], path2_metrics(za)[3]):
            st = check(ix, f, Q, kl, mm, omm, omo, "after the copy came back")
            assert st["approx_scan"] == 2 and st["row_copy_bytes"] >= N * (2 * d + 8), st

    if how == "append":
        ix.append(Xall[n:])
        exact_all()
        ix.build()
        lsh_all(zo.Forest.build(Xall, M, T))
    else:
        ix.add(Xall[n:])
        f.insert(Xall, n)
        lsh_all(f)
        exact_all()
    ix.close()


@pytest.mark.parametrize("d", [256, 768])
def test_path2_removals(za, d):
    """removed rows (every 5th, the checked queries' planted neighbours, all but a few rows of the first row chunk so that it holds fewer
    than k live rows) and deduplicated ones are masked by the live-row bitmap; ids carry id_base; 8192 live rows take path 2, 8191 path 1"""
    n, B, base, seed = 40009, 12, 1 << 40, 0x5EB2B100 + d
    X = zo.synth_rows(n, d, seed=seed)
    X[30000:30040] = X[29999]      # duplicates for deduplicate
    X[31000:31003] = X[12345]
    Q = zo.synth_queries(B, d, n, seed_rows=seed)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=base)
    ix.append(X)
    alive = np.ones(n, bool)
    planted = np.array([zo.synth_query_row(b, n) for b in range(B)])
    first = np.arange(4096)
    gone = np.unique(np.concatenate([planted, np.arange(0, n, 5), first[first % 97 != 0]]))
    assert len(ix.remove(gone + base)) == len(gone)
    alive[gone] = False
    assert 0 < alive[:4096].sum() < 100
    ix.deduplicate()
    dup = zo.find_duplicates(X, alive.astype(np.uint8))
    assert dup.sum() >= 30
    alive &= ~dup
    live = np.flatnonzero(alive)
    rows = list(range(B))
    for m, om, omode in path2_metrics(za):
        check_ks(ix, Q, rows, (1, 100, 1024), m, om, omode, X[live], 2, ids_of=live, id_base=base)
        assert ix.exact_info()["rows_live"] == len(live)
    # down to exactly 8192 live rows (path 2), then 8191 (path 1)
    rng = np.random.default_rng(d)
    keep = np.sort(rng.choice(live, 8192, replace=False))
    ix.remove(np.setdiff1d(live, keep) + base)
    for want, live in ((2, keep), (1, keep[1:])):
        if want == 1:
            ix.remove(keep[:1] + base)
        for m, om, omode in (path2_metrics(za)[0], path2_metrics(za)[3]):
            check_rows(ix, Q, [0, B // 2, B - 1], 100, m, om, omode, X[live], ids_of=live, id_base=base)
            assert exact_path(ix, want)["rows_live"] == len(live)
    ix.close()


@pytest.mark.parametrize("order", ["2", "3", None])
@pytest.mark.parametrize("d", [256, 768])
def test_path2_over_the_scan_row_order(za, monkeypatch, d, order):
    """The copy in the scan's row order (position p holds row perm[p] for p < perm_rows, row p beyond), shared by the exact path 2 and the
    LSH scan.  At each step both search the same index, the one that meets the change first alternating, and both must be right."""
    if order is None:
        monkeypatch.delenv("ZH_ROW_ORDER", raising=False)
    else:
        monkeypatch.setenv("ZH_ROW_ORDER", order)
    monkeypatch.delenv("ZH_ROW_HALF_META_ONLY", raising=False)
    n0, a1, a2, M, T, B, k, kl, seed = 12003, 1001, 3005, 300, 6, 16, 100, 10, 0x5EB2B200 + d
    N = n0 + a1 + a2
    Xall = zo.synth_rows(N, d, seed=seed)
    Q = zo.synth_queries(B, d, n0, seed_rows=seed)
    rows = [0, 5, 10, B - 1]
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.set_sweep_mode("approx")
    ix.set_hash_mode("dense")
    lsh = (path2_metrics(za)[1], path2_metrics(za)[3])

    def lsh_check(f, Qs, what):
        for m, om, omode in lsh:
            st = check(ix, f, Qs, kl, m, om, omode, what)
            assert st["approx_scan"] == 2, (what, st)
        return st

    def exact_check(X, Qs, ids_of=None):
        for m, om, omode in path2_metrics(za):
            check_rows(ix, Qs, rows, k, m, om, omode, X, ids_of=ids_of)
            exact_path(ix, 2)

    def sorted_order(st):
        if order is not None:
            assert st["scan_order_keys"] == int(order), st

    # the first copy: made by the LSH scan, in the order measured on the forest's leaves
    ix.add(Xall[:n0])
    f = zo.Forest.build(Xall[:n0], M, T)
    sorted_order(lsh_check(f, Q, "first copy"))
    exact_check(Xall[:n0], Q)
    # fewer than a quarter appended: the order stays, the new rows at position = id -- the exact path meets them first
    ix.add(Xall[n0:n0 + a1])
    f.insert(Xall[:n0 + a1], n0)
    exact_check(Xall[:n0 + a1], Q)
    sorted_order(lsh_check(f, Q, "appended after the order"))
    # past a quarter: the copy is made again, in an order measured on all of it
    ix.add(Xall[n0 + a1:])
    f.insert(Xall, n0 + a1)
    sorted_order(lsh_check(f, Q, "order made again"))
    exact_check(Xall, Q)
    # removed rows (planted neighbours among them)
    gone = np.unique(np.concatenate([np.arange(3, N, 7), [zo.synth_query_row(b, n0) for b in range(0, B, 2)]])).astype(np.uint64)
    ix.remove(gone)
    f.remove(gone)
    live = np.setdiff1d(np.arange(N), gone.astype(np.int64))
    exact_check(Xall[live], Q, ids_of=live)
    lsh_check(f, Q, "removed")
    # a new forest: the copy is made again in its order
    ix.build()
    f = zo.Forest.from_arrays(Xall, M, ix.get_forest())
    sorted_order(lsh_check(f, Q, "rebuilt"))
    exact_check(Xall[live], Q, ids_of=live)
    # clear and refill to the same row count, on another scale: nothing of the old copy, order or live rows may survive
    ix.clear()
    s = np.float32(2.0 ** -30)
    Y = Xall * s
    ix.add(Y)
    fy = zo.Forest.build(Y, M, T)
    exact_check(Y, Q * s)
    lsh_check(fy, Q * s, "refilled")
    assert ix.exact_info()["rows_live"] == N
    ix.close()


def test_path2_tails_and_chunk_edges(za):
    """row counts at the path-1 / path-2 threshold (8191 / 8192 live rows), around the row-chunk boundaries (4096, 20480, 86016 for k <= 4096)
    and with a partial last tile; queries planted on the rows at those boundaries.  The index grows through the counts (each append converts
    the new rows only)."""
    d, B = 256, 17
    counts = (8191, 8192, 8193, 20479, 20480, 20481, 86017)
    X = zo.synth_rows(counts[-1], d)
    edges = [0, 4095, 4096, 8190, 8191, 8192, 20479, 20480, 20481, 86015, 86016, 15, 16, 40000]
    rng = np.random.default_rng(3)
    Q = np.concatenate([X[edges] + np.float32(0.3) * rng.standard_normal((len(edges), d)).astype(np.float32),
                        zo.synth_queries(B - len(edges), d, counts[-1])])
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    have = 0
    for n in counts:
        ix.append_synthetic(n - have, first_row=have)
        have = n
        # first, middle, last, and the queries planted just below and above a boundary inside the table
        rows = sorted({0, B // 2, B - 1} | {i for i, r in enumerate(edges) if r < n and r not in (0, 15, 16, 40000)})
        for m, om, omode in path2_metrics(za):
            check_ks(ix, Q, rows, (1, 100, 1024), m, om, omode, X[:n], 1 if n < 8192 else 2)
            assert ix.exact_info()["rows_live"] == n
    ix.close()


@pytest.mark.parametrize("d", [256, 768, 1024])
def test_path2_adversarial_rows(za, d):
    """huge, tiny, subnormal-heavy (in fp16), integer-valued, duplicate and near-duplicate rows, zero rows, rows whose |x|^2 overflows, a NaN
    row and an inf row (no usable fp16 scale: every interval of theirs is 'nothing certain'), and queries next to them.  With fewer live rows
    than a query's list holds (16384 + 8 k) no list can run over, so every batch must be answered by path 2 itself (redone = 0) -- the zero
    query's cosine intervals included, which decide nothing."""
    n, B, k = 9000, 10, 100
    rng = np.random.default_rng(d)
    X = special_rows(zo.synth_rows(n, d, seed=0x5EB2B300 + d), d, rng)
    X[4000:5000] = _adversarial_rows(1000, d, rng)
    assert np.isnan(X[4730]).any() and np.isinf(X[4731]).any()
    Q = special_queries(zo.synth_queries(B, d, n, seed_rows=0x5EB2B300 + d), X)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    for m, om, omode in path2_metrics(za):
        check_exact(ix.search_exact_batch(Q, k, m), X, Q, k, om, omode)
        assert exact_path(ix, 2)["rows_live"] == n
    ix.close()

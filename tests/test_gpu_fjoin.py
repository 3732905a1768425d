"""The forest self-join (zh_self_join_forest): every unordered pair of distinct stored rows that share a leaf in at least one tree and whose key is
<= one threshold key, each pair ONCE, as three arrays ascending by (a, key, b).  The reference is built here from ix.get_forest() -- the union over
the reachable leaves of their member pairs is F, the sum of len (len - 1) / 2 is leaf_pairs -- and the oracle: distance_batch(X[b's], X[a]), the keys
<= max_key, a lexsort by (a, key, b).  Every comparison is bit for bit on the three arrays, their dtypes and the total.  Thresholds are keys of the
reference's own key list.  The indexes are filled with add, so that they are built; the shapes are test_gpu_fknn.py's."""
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


def forest_pairs(f):
    """F as (a, b) with a < b, ascending by (a, b) and unique; leaf_pairs; the tile products of path 2; the leaves' lengths"""
    codes, leaf_pairs, tiles, lens = [], 0, 0, []
    for leaves in forest_leaves(f):
        for ids in leaves:
            n = ids.size
            lens.append(n)
            leaf_pairs += n * (n - 1) // 2
            t = (n + 15) // 16
            tiles += t * (t + 1) // 2
            if n >= 2:
                i, j = np.triu_indices(n, 1)
                codes.append((np.minimum(ids[i], ids[j]) << 32) | np.maximum(ids[i], ids[j]))
    code = np.unique(np.concatenate(codes)) if codes else np.zeros(0, np.int64)
    return code >> 32, code & 0xFFFFFFFF, leaf_pairs, tiles, lens


def keyed(X, fa, fb, om, omode, id_base=0):
    """every pair of F with the oracle's key of stored row b against the query row a, ascending by (a, key, b)"""
    keys = np.zeros(fa.size, np.uint64)
    starts = np.flatnonzero(np.r_[True, fa[1:] != fa[:-1]]) if fa.size else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], fa.size]
    for s, e in zip(starts.tolist(), ends.tolist()):
        keys[s:e] = np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[fb[s:e]]), X[fa[s]]), np.uint64)
    o = np.lexsort((fb, keys, fa))
    return fa[o].astype(np.uint64) + np.uint64(id_base), fb[o].astype(np.uint64) + np.uint64(id_base), keys[o]


def within(ref, mk):
    """the reference at a threshold (a subset of an (a, key, b) order keeps it)"""
    m = ref[2] <= np.uint64(mk)
    return ref[0][m], ref[1][m], ref[2][m]


def quantile_key(ref, keep):
    """a key of the reference's own list that keeps about `keep` pairs"""
    ks = np.sort(ref[2])
    return ks[min(keep, ks.size - 1)]


def same(got, ref):
    for g, r, what in zip(got, ref, ("a", "b", "keys")):
        assert g.dtype == np.uint64 and g.shape == r.shape and (g == r).all(), what


def each_pair_once(got):
    code = (got[0] << np.uint64(32)) | got[1]
    return np.unique(code).size == code.size and (got[0] < got[1]).all()


def raw_call(ix, max_key, m, capacity, with_arrays=True):
    """the host entry point itself -> (rc, total)"""
    from zebra_amd import _ffi
    a, b, keys = (np.zeros(max(capacity, 1), np.uint64) for _ in range(3))
    total = C.c_uint64(777)
    P = lambda x: x.ctypes.data_as(C.c_void_p) if with_arrays else None  # noqa: E731
    rc = _ffi.lib().zh_self_join_forest(ix._h, int(max_key), m.metric, m.mode, capacity, P(a), P(b), P(keys), C.byref(total))
    return rc, int(total.value)


def on_path(monkeypatch, path):
    monkeypatch.delenv("ZH_FJOIN_CAND_CAP", raising=False)
    if path == 1:
        monkeypatch.setenv("ZH_FJOIN_PATH", "1")
    else:
        monkeypatch.delenv("ZH_FJOIN_PATH", raising=False)


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


def built(name):
    """(index, X, F's a, F's b, leaf_pairs, tiles, leaf lengths) of a shape, the index filled with add"""
    import zebra_amd as za
    if name in _SHARED:
        return _SHARED[name]
    X, d, opts = {"A": (lambda: zo.synth_rows(1500, 30), 30, (64, 4)), "B": (rows_b, DB, (256, 3)), "Bdup": (rows_bdup, DB, (256, 3)),
                  "C": (lambda: zo.synth_rows(2000, 30), 30, (5, 15)), "planted": (lambda: planted_rows(False), DB, (256, 3)),
                  "uncertain": (lambda: planted_rows(True), DB, (256, 3))}[name]
    X = X()
    ix = za.LSHIndex(d, za.LSHIndexOptions(*opts), device=0)
    ix.add(X)
    _SHARED[name] = (ix, X) + forest_pairs(ix.get_forest())
    return _SHARED[name]


@functools.lru_cache(maxsize=None)
def reference(name, mi):
    import zebra_amd as za
    _, X, fa, fb, _, _, _ = built(name)
    _, om, omode = thirteen_metrics(za)[mi]
    return keyed(X, fa, fb, om, omode)


def expect_info(ix, path, leaf_pairs, pairs, trees, rows_live):
    info = ix.join_forest_info()
    assert info["path"] == path and info["redone"] == 0 and info["leaf_pairs"] == leaf_pairs and info["pairs"] == pairs, info
    assert info["trees"] == trees and info["rows_live"] == rows_live, info
    if path == 1:
        assert info["tiles"] == 0 and info["candidates"] == 0, info
    return info


# ---------------------------------------------------------------- path 1
@pytest.mark.parametrize("mi", range(13))
def test_path1_every_metric(za, monkeypatch, mi):
    ix, X, fa, fb, leaf_pairs, _, _ = built("A")
    m = thirteen_metrics(za)[mi][0]
    ref = reference("A", mi)
    on_path(monkeypatch, 2)  # (d = 30: the path rule itself chooses path 1)
    assert 0 < fa.size < leaf_pairs  # (the shape: some pairs share leaves in several trees)
    for mk in (quantile_key(ref, 3000), quantile_key(ref, 10), ALL):
        got = ix.self_join_forest(metric=m, max_key=mk)
        want = within(ref, mk)
        same(got, want)
        expect_info(ix, 1, leaf_pairs, want[0].size, 4, 1500)
        assert each_pair_once(got)
        assert ix.self_join_forest_count(metric=m, max_key=mk) == want[0].size
    assert got[0].size == fa.size  # UINT64_MAX: exactly F


def test_default_regime(za, monkeypatch):
    """max_node_size 5, 15 trees: thousands of leaves of 0 .. 4 rows"""
    ix, X, fa, fb, leaf_pairs, _, lens = built("C")
    assert max(lens) <= 5 and min(lens) == 0 and len(lens) > 3000  # (the shape)
    on_path(monkeypatch, 2)
    for mi in (0, 2):
        m = thirteen_metrics(za)[mi][0]
        ref = reference("C", mi)
        for mk in (quantile_key(ref, 3000), ALL):
            got = ix.self_join_forest(metric=m, max_key=mk)
            same(got, within(ref, mk))
            expect_info(ix, 1, leaf_pairs, got[0].size, 15, 2000)
        assert got[0].size == fa.size and each_pair_once(got)


def test_states(za, monkeypatch):
    X = zo.synth_rows(64, 30)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    got = ix.self_join_forest(metric=m, max_key=ALL)  # an empty index: no row, no pair
    assert all(g.size == 0 and g.dtype == np.uint64 for g in got) and ix.join_forest_info()["pairs"] == 0
    ix.append(X[:3])
    with pytest.raises(za.ZhError) as e:  # rows, but no trees
        ix.self_join_forest(metric=m, max_key=ALL)
    assert e.value.code == ESTATE
    from zebra_amd import _ffi
    tot = C.c_uint64(0)
    assert _ffi.lib().zh_self_join_forest(ix._h, int(ALL), 99, 0, 0, None, None, None, C.byref(tot)) == EINVAL  # the argument checks come first
    ix.close()
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.add(X[:1])
    got = ix.self_join_forest(metric=m, max_key=ALL)  # one row: a leaf-mate of nobody
    info = ix.join_forest_info()
    assert got[0].size == 0 and info["pairs"] == 0 and info["leaf_pairs"] == 0 and info["rows_live"] == 1 and info["trees"] == 4, info
    ix.add(X[1:40])  # 40 rows in one leaf per tree: every pair, met four times, once
    got = ix.self_join_forest(metric=m, max_key=ALL)
    fa, fb, leaf_pairs, _, _ = forest_pairs(ix.get_forest())
    assert leaf_pairs == 4 * 780 and fa.size == 780
    same(got, keyed(X, fa, fb, zo.L2SQ, 0))
    same(got, ix.self_join(metric=m, max_key=ALL))  # ... which is the exact join's answer
    assert ix.join_forest_info()["leaf_pairs"] == leaf_pairs
    ix.remove(list(range(40)))
    got = ix.self_join_forest(metric=m, max_key=ALL)  # removed rows only
    assert got[0].size == 0 and ix.join_forest_info()["rows_live"] == 0
    ix.close()


# ---------------------------------------------------------------- path 2
def check_path2(za, monkeypatch, name, mi, thresholds):
    ix, X, fa, fb, leaf_pairs, tiles, lens = built(name)
    m = thirteen_metrics(za)[mi][0]
    ref = reference(name, mi)
    out = []
    for mk in thresholds(ref):
        on_path(monkeypatch, 2)
        got = ix.self_join_forest(metric=m, max_key=mk)
        want = within(ref, mk)
        same(got, want)
        info = expect_info(ix, 2, leaf_pairs, want[0].size, 3, NB)
        assert info["tiles"] == tiles and info["launches"] == 3 and info["candidates"] >= info["pairs"], info  # (one batch per tree)
        assert info["tiles"] * 2 < ((NB + 15) // 16) * ((NB + 15) // 16 + 1) // 2, info  # block-diagonal work: under half the exact join's triangle
        assert each_pair_once(got)
        same(ix.self_join_forest(metric=m, max_key=mk), got)  # twice: identical
        on_path(monkeypatch, 1)
        forced = ix.self_join_forest(metric=m, max_key=mk)
        expect_info(ix, 1, leaf_pairs, want[0].size, 3, NB)
        same(forced, got)
        out.append(got)
    return out


@pytest.mark.parametrize("mi", range(4))
@pytest.mark.parametrize("name", ["B", "Bdup"])
def test_path2_against_the_oracle_and_path1(za, monkeypatch, name, mi):
    """B: every leaf between 16 and 256 rows, most of them no multiple of 16.  Bdup (400 bit-identical rows, whose planes cut nothing off): leaves
    under 16 rows and empty leaves as well, and a quantile that falls among 79 800 tied keys"""
    _, _, _, _, _, _, lens = built(name)
    assert sum(1 for v in lens if v % 16) > 0  # (the shapes)
    if name == "B":
        assert 16 <= min(lens) and max(lens) <= 256
    else:
        assert min(lens) == 0 and sum(1 for v in lens if 0 < v < 16) > 0 and max(lens) == 400
    check_path2(za, monkeypatch, name, mi, lambda ref: (quantile_key(ref, 3000), quantile_key(ref, 10)))


@pytest.mark.parametrize("mi", [0, 2])
def test_tied_pairs_of_an_unsplittable_leaf(za, monkeypatch, mi):
    """400 bit-identical rows: one leaf of 400 at max_node_size 256 in EVERY tree: 79 800 tied pairs, each once, in (a, key, b) order"""
    ix, X, fa, fb, leaf_pairs, _, lens = built("Bdup")
    assert sorted(lens)[-3:] == [400, 400, 400] and min(lens) == 0  # (the shape)
    ref = reference("Bdup", mi)
    dup = (ref[0] >= 1000) & (ref[0] < 1400) & (ref[1] >= 1000) & (ref[1] < 1400)
    assert dup.sum() == 79800 and np.unique(ref[2][dup]).size == 1
    tie = ref[2][dup][0]
    (got,) = check_path2(za, monkeypatch, "Bdup", mi, lambda ref: (tie,))
    g = (got[0] >= 1000) & (got[0] < 1400) & (got[1] >= 1000) & (got[1] < 1400) & (got[2] == tie)
    assert g.sum() == 79800


@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_path2_every_dimension(za, monkeypatch, d):
    n = 1100
    X = rows_b(d, n)
    ix = za.LSHIndex(d, za.LSHIndexOptions(128, 2), device=0)
    ix.add(X)
    fa, fb, leaf_pairs, tiles, _ = forest_pairs(ix.get_forest())
    ref = keyed(X, fa, fb, zo.L2SQ, 0)
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    for mk in (quantile_key(ref, 3000), quantile_key(ref, 10)):
        got = ix.self_join_forest(metric=m, max_key=mk)
        same(got, within(ref, mk))
        info = expect_info(ix, 2, leaf_pairs, got[0].size, 2, n)
        assert info["tiles"] == tiles, info
    on_path(monkeypatch, 1)
    same(ix.self_join_forest(metric=m, max_key=mk), got)
    ix.close()


@pytest.mark.parametrize("mi", range(4))
def test_adversarial_rows(za, monkeypatch, mi):
    """the threshold is the near-duplicates' own largest key among those that are leaf-mates (L2SQ, L2 and the literal cosine key; the parity key
    orders similarities ascending, so a sampled small key stands in, as in test_gpu_join.py): a bound that forgets the second operand's rounding
    loses hits here"""
    ix, X, fa, fb, leaf_pairs, _, _ = built("planted")
    m, om, omode = thirteen_metrics(za)[mi]
    ref = reference("planted", mi)
    near = set(NEAR)
    is_near = np.array([(a, b) in near for a, b in zip(ref[0].tolist(), ref[1].tolist())])
    assert is_near.sum() >= 30  # (the shape: most planted pairs share a leaf in some tree)
    parity = om == zo.COSINE and omode == zo.PARITY
    mk = quantile_key(ref, 3000) if parity else ref[2][is_near].max()
    (got,) = check_path2(za, monkeypatch, "planted", mi, lambda ref: (mk,))
    if not parity:
        have = set(zip(got[0].tolist(), got[1].tolist()))
        assert all(p in have for p in zip(ref[0][is_near].tolist(), ref[1][is_near].tolist()))


@pytest.mark.parametrize("mi", [0, 3])
def test_rows_nothing_is_certain_about(za, monkeypatch, mi):
    """path 2 against path 1: the device's own arithmetic on both sides (a NaN's sign differs between host and GPU)"""
    ix, X, fa, fb, leaf_pairs, _, _ = built("uncertain")
    m = thirteen_metrics(za)[mi][0]
    mk = quantile_key(reference("planted", mi), 3000)
    on_path(monkeypatch, 2)
    got = ix.self_join_forest(metric=m, max_key=mk)
    info = ix.join_forest_info()
    mates = int(((fa == 700) | (fb == 700) | (fa == 701) | (fb == 701)).sum())
    assert info["path"] == 2 and info["redone"] == 0 and info["candidates"] >= mates > 0, info  # both rows' every pair was keyed
    on_path(monkeypatch, 1)
    same(ix.self_join_forest(metric=m, max_key=mk), got)
    assert ix.join_forest_info()["path"] == 1 and each_pair_once(got)


# ---------------------------------------------------------------- both paths
def sampled_key(X, om, omode, keep):
    """a key that keeps about `keep` of all n (n - 1) / 2 pairs, from the oracle's keys of 128 sampled rows against the rows above them"""
    n = X.shape[0]
    ks = np.sort(np.concatenate([np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[a + 1:]), X[a]), np.uint64)
                                 for a in range(0, n - 1, n // 128)]))
    return ks[int(keep / (n * (n - 1) / 2) * ks.size)]


@pytest.mark.parametrize("path", [1, 2])
def test_one_leaf_equals_the_exact_join(za, monkeypatch, path):
    """one tree whose root is a leaf of 8229 rows = 515 tiles: F is every pair.  Several held blocks, several chunks counted from the diagonal,
    the last tile partial"""
    n = 8192 + 37
    if "one" not in _SHARED:
        X = zo.synth_rows(n, DB)
        ix = za.LSHIndex(DB, za.LSHIndexOptions(16384, 1), device=0)
        ix.add(X)
        _SHARED["one"] = (ix, X, sampled_key(X, zo.L2SQ, 0, 3000))
    ix, X, mk = _SHARED["one"]
    m = za.L2SquaredDistance()
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    exact = ix.self_join(metric=m, max_key=mk)
    assert 500 < exact[0].size < 20000
    on_path(monkeypatch, path)
    got = ix.self_join_forest(metric=m, max_key=mk)
    info = expect_info(ix, path, n * (n - 1) // 2, exact[0].size, 1, n)
    if path == 2:
        assert info["tiles"] == 515 * 516 // 2 and info["launches"] == 1, info
    same(got, exact)


@pytest.mark.parametrize("path", [1, 2])
def test_subset_of_the_exact_join(za, monkeypatch, path):
    ix, X, fa, fb, _, _, _ = built("B")
    m = za.L2SquaredDistance()
    mk = quantile_key(reference("B", 0), 3000)
    monkeypatch.delenv("ZH_JOIN_PATH", raising=False)
    exact = ix.self_join(metric=m, max_key=mk)
    on_path(monkeypatch, path)
    got = ix.self_join_forest(metric=m, max_key=mk)
    in_f = np.isin((exact[0] << np.uint64(32)) | exact[1], ((fa << 32) | fb).astype(np.uint64))
    assert 0 < in_f.sum() < exact[0].size  # (the forest misses some pairs)
    same(got, tuple(e[in_f] for e in exact))


@pytest.mark.parametrize("path", [1, 2])
def test_mutations(za, monkeypatch, path):
    base = 1 << 40
    extra = zo.synth_rows(NB + 350, DB)[NB:]
    X = rows_b()
    m, om, omode = thirteen_metrics(za)[0]
    on_path(monkeypatch, path)
    ix = za.LSHIndex(DB, za.LSHIndexOptions(256, 3), device=0, id_base=base)
    ix.add(X)

    def step(rows, dead, outside=()):
        """the join against the oracle on the forest as it is now; `outside`: rows no tree holds"""
        fa, fb, leaf_pairs, _, _ = forest_pairs(ix.get_forest())
        ref = keyed(rows, fa, fb, om, omode, base)
        mk = quantile_key(ref, 3000)
        got = ix.self_join_forest(metric=m, max_key=mk)
        same(got, within(ref, mk))
        expect_info(ix, path, leaf_pairs, got[0].size, 3, rows.shape[0] - len(dead))
        gone = np.array(list(dead) + list(outside), np.uint64) + np.uint64(base)
        assert not np.isin(got[0], gone).any() and not np.isin(got[1], gone).any()
        all_f = ix.self_join_forest(metric=m, max_key=ALL)
        assert all_f[0].size == fa.size and not np.isin(all_f[1], gone).any()
        return got, mk

    gone = list(range(80, 96, 3)) + list(range(112, 128)) + [NB - 1]  # every third row of a tile, one whole tile, the last row
    ix.remove([g + base for g in gone])
    step(X, gone)
    ix.add(extra[:300])  # they descend the trees and split leaves
    X1 = np.concatenate([X, extra[:300]])
    step(X1, gone)
    ix.append(extra[300:])  # in no tree: in no pair
    X2 = np.concatenate([X1, extra[300:]])
    n2 = X2.shape[0]
    step(X2, gone, outside=range(n2 - 50, n2))
    ix.build()  # ... and now they take part
    got, mk = step(X2, gone)
    new_ids, _ = ix.compact()
    after = ix.self_join_forest(metric=m, max_key=mk)  # the old answer under the id map (compaction keeps the rows' order)
    same(after, (new_ids[(got[0] - np.uint64(base)).astype(np.int64)], new_ids[(got[1] - np.uint64(base)).astype(np.int64)], got[2]))
    ix.close()


def test_scan_order_that_is_not_id_order(za, monkeypatch):
    """the fp16 copy in a sorted row order (position p holds row perm[p]): leaves are gathered by row number, pairs are (min row, max row); the
    same again with a batch redone by path 1"""
    X = rows_b()
    m = za.L2SquaredDistance()
    on_path(monkeypatch, 2)
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    plain = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    plain.add(X)
    fa, fb, leaf_pairs, _, _ = forest_pairs(plain.get_forest())
    full = keyed(X, fa, fb, zo.L2SQ, 0)
    mk = quantile_key(full, 3000)
    ref = plain.self_join_forest(metric=m, max_key=mk)
    assert plain.join_forest_info()["path"] == 2
    same(ref, within(full, mk))
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(DB, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(8, DB, NB), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    assert zo.canonical_forest(ix.get_forest(), DB) == zo.canonical_forest(plain.get_forest(), DB)  # the same forest
    got = ix.self_join_forest(metric=m, max_key=mk)
    expect_info(ix, 2, leaf_pairs, ref[0].size, 9, NB)
    same(got, ref)
    monkeypatch.setenv("ZH_FJOIN_CAND_CAP", "64")
    got = ix.self_join_forest(metric=m, max_key=mk)
    info = ix.join_forest_info()
    assert info["path"] == 2 and info["redone"] > 0 and info["pairs"] == ref[0].size, info
    same(got, ref)
    ix.close()
    plain.close()


@pytest.mark.parametrize("name", ["B", "Bdup"])
def test_candidate_pool_overflow_is_redone_by_path1(za, monkeypatch, name):
    ix, X, fa, fb, leaf_pairs, tiles, _ = built(name)
    m = za.L2SquaredDistance()
    ref = reference(name, 0)
    mk = quantile_key(ref, 3000)
    want = within(ref, mk)
    on_path(monkeypatch, 2)
    monkeypatch.setenv("ZH_FJOIN_CAND_CAP", "16")  # every tree's batch runs over
    got = ix.self_join_forest(metric=m, max_key=mk)
    info = ix.join_forest_info()
    assert info == {"rows_live": NB, "trees": 3, "path": 2, "leaf_pairs": leaf_pairs, "pairs": want[0].size, "candidates": 0,
                    "launches": info["launches"], "tiles": tiles, "redone": 3}, info
    same(got, want)
    monkeypatch.setenv("ZH_FJOIN_CAND_CAP", "1000000")  # room for everything
    got = ix.self_join_forest(metric=m, max_key=mk)
    assert ix.join_forest_info()["redone"] == 0
    same(got, want)


@pytest.mark.parametrize("path", [1, 2])
def test_capacity(za, monkeypatch, path):
    from zebra_amd import _ffi
    ix, X, fa, fb, leaf_pairs, _, _ = built("B")
    m = za.L2SquaredDistance()
    ref = reference("B", 0)
    mk = quantile_key(ref, 3000)
    total = within(ref, mk)[0].size
    on_path(monkeypatch, path)
    for cap, arrays in ((total - 1, True), (1, True), (0, False)):
        rc, tot = raw_call(ix, mk, m, cap, arrays)
        assert rc == ELIMIT and tot == total, (cap, rc, tot)
        info = ix.join_forest_info()
        assert info["path"] == path and info["pairs"] == total and info["redone"] == 0, info
    rc, tot = raw_call(ix, mk, m, total)
    assert rc == 0 and tot == total
    rc, tot = raw_call(ix, ALL, m, 0, False)  # duplicates across trees are not counted
    assert rc == ELIMIT and tot == fa.size
    assert ix.self_join_forest_count(metric=m, max_key=mk) == total
    same(ix.self_join_forest(metric=m, max_key=mk, capacity=5), within(ref, mk))  # the wrapper's second call
    assert _ffi.lib().zh_self_join_forest(ix._h, int(mk), m.metric, m.mode, 5, None, None, None, C.byref(C.c_uint64(0))) == EINVAL


def test_device_entry_point_and_siblings(za, monkeypatch):
    import torch
    ix, X, fa, fb, leaf_pairs, _, _ = built("B")
    Q = zo.synth_queries(8, DB, NB)
    m = za.L2SquaredDistance()
    ref = reference("B", 0)
    mk = quantile_key(ref, 3000)
    want = within(ref, mk)
    total = want[0].size
    on_path(monkeypatch, 2)
    monkeypatch.delenv("ZH_KNN_PATH", raising=False)
    mask = np.zeros(NB, bool)
    mask[::2] = True
    ix.search_exact_batch(Q, 10, m)
    ix.search_exact_filtered_batch(Q, 10, m, mask)
    ix.search_range_batch(Q, 1.0, m)
    ix.self_join_count(metric=m, max_key=np.uint64(0))
    ix.knn_graph(10, m, 0, 64)
    ix.knn_graph_forest(10, m, 0, 64)
    before = (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.knn_info(), ix.knn_forest_info(), ix.stats())
    dev = torch.device("cuda", 0)
    cap = total + 100
    a = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    b = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    keys = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    ix.self_join_forest_device(mk, m, cap, a.data_ptr(), b.data_ptr(), keys.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize()
    assert int(tot.item()) == total and ix.join_forest_info()["path"] == 2
    same(tuple(t.cpu().numpy().view(np.uint64)[:total] for t in (a, b, keys)), want)
    assert (a.cpu().numpy()[total:] == -7).all()
    with pytest.raises(za.ZhError) as e:
        ix.self_join_forest_device(mk, m, total - 1, a.data_ptr(), b.data_ptr(), keys.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == ELIMIT and int(tot.item()) == total
    tot.zero_()
    with pytest.raises(za.ZhError) as e:  # count only
        ix.self_join_forest_device(mk, m, 0, None, None, None, tot.data_ptr())
    assert e.value.code == ELIMIT and int(tot.item()) == total
    assert (ix.exact_info(), ix.filtered_info(), ix.range_info(), ix.join_info(), ix.knn_info(), ix.knn_forest_info(), ix.stats()) == before


def test_deduplicate_within_forest_against_the_rule(za):
    from zebra_amd.index import dedup_rule
    X = rows_b()[:1200].copy()
    X[300:340] = X[20:60] * np.float32(1.0 + 2.0**-10)  # near-duplicates of rows 20 .. 59
    X[700:720] = X[20:40]                                # and exact copies of some of them
    m = za.L2Distance()
    ix = za.LSHIndex(DB, za.LSHIndexOptions(128, 4), device=0)
    ix.add(X)
    radius = 0.05
    fa, fb, _, _, _ = forest_pairs(ix.get_forest())
    want = within(keyed(X, fa, fb, zo.L2, 0), za.radius_key(m, radius))
    assert 20 <= want[0].size < 1000
    removed = ix.deduplicate_within_forest(radius, m)
    assert removed.dtype == np.uint64 and (removed == dedup_rule(want[0], want[1])).all() and removed.size >= 20
    assert len(ix) == 1200 - removed.size
    a, b, _ = ix.self_join_forest(radius, m)  # what is left holds no joined pair
    assert a.size == 0
    ix.close()


def test_database_near_duplicates_forest(za):
    X = zo.synth_rows(60, 30)[:50].copy()
    X[40:45] = X[3:8]
    docs = ["doc%d" % i for i in range(50)]
    db = za.Database(30, za.L2Distance, za.LSHIndexOptions(16, 4), device=0)
    assert db.near_duplicates_forest(0.5) == [] and db.deduplicate_within_forest(0.5).size == 0
    db.insert_records(X, docs)
    db.remove([7])
    fa, fb, _, _, _ = forest_pairs(db.index.get_forest())
    ref = within(keyed(X, fa, fb, zo.L2, 0), za.radius_key(db.metric, 1e-3))
    got = db.near_duplicates_forest(1e-3)
    assert [(x, y) for x, y, _ in got] == [(docs[int(i)], docs[int(j)]) for i, j in zip(ref[0], ref[1])]
    assert [v for _, _, v in got] == zo.key_to_float(ref[2]).tolist()
    exact = db.near_duplicates(1e-3)
    assert set(got) <= set(exact) and len(exact) == 4  # rows 3 .. 7 and their copies, 7 removed
    removed = db.deduplicate_within_forest(1e-3)
    assert removed.tolist() == sorted(set(ref[1].tolist())) and all(int(i) not in db._documents for i in removed)


@pytest.mark.parametrize("name", ["l2sq", "cos_corrected"])
def test_walk_edges_a_chunk_of_one_tile_and_idle_waves(za, monkeypatch, name):
    """the held-tile walk (zh_device.h) at its edges, against the family fuzz's reference: one tree whose root is a leaf of 1040 rows = 65 tiles.
    So small a launch walks chunks of 8 tiles (fill_chunk), counted from each held block's diagonal: the blocks from tile 0, 8, ... walk eight
    full chunks (even: the last tile in the second LDS buffer) and a chunk of ONE tile (odd, no prefetch at all), the others end in chunks of
    5 tiles; in every first chunk waves 1 to 3 skip the tiles before their diagonal; the last held block holds one tile: three idle waves.
    Near-duplicates are planted so that the one-tile chunk and the last block's diagonal tile both have pairs"""
    from tests import family_cases as fc
    n = 1040
    spec = fc.metric_spec(name)
    m = za.L2SquaredDistance() if name == "l2sq" else za.CosineDistance(parity=False)
    X = zo.synth_rows(n, DB).copy()
    X[1030], X[1039] = X[5] * np.float32(1.0 + 2.0**-12), X[1025] * np.float32(1.0 + 2.0**-12)
    rows, alive = np.arange(n), np.ones(n, bool)
    K = fc.key_matrix(spec, X, X)
    upper = rows[None, :] > rows[:, None]
    mk = fc.quantile_threshold(K, upper, 3000, n * (n - 1) / 2)
    ref = fc.join_ref(K, rows, alive, alive, mk, 0, 0, True)
    assert ((ref[0] == 5) & (ref[1] == 1030)).any() and ((ref[0] == 1025) & (ref[1] == 1039)).any() and ref[0].size >= 3000
    ix = za.LSHIndex(DB, za.LSHIndexOptions(16384, 1), device=0)
    ix.add(X)
    on_path(monkeypatch, 2)
    got = ix.self_join_forest(metric=m, max_key=mk)
    info = expect_info(ix, 2, n * (n - 1) // 2, ref[0].size, 1, n)
    assert info["tiles"] == 65 * 66 // 2 and info["launches"] == 1, info
    same(got, ref)
    ix.close()

"""The exact and the forest query families on ONE table whose offsets do not fit 32 bits: 4 198 437 x 1024 synthetic rows (kind 2), 17.2 GB of f32
rows and 8.6 GB of fp16 copy.  At d = 1024 the f32 byte offset of a row reaches 2^32 at row 2^20, the fp16 byte offset and the element offset 2^32
and 2^31 at row 2^21, the element offset 2^32 at row 2^22; n = 2^22 + 4096 + 37 is no multiple of 16, so the copy's last tile is a partial one at a
high address.  An offset narrowed to 32 bits anywhere in these families wraps to a lower address INSIDE the allocation: nothing faults, the answer
names the wrong rows -- and every other test of these families stops at 1 000 000 x 768 (exact search) or a few tens of thousands of rows.

Every comparison is bit for bit on ids, keys, counts and offsets against the oracle, and every call's *_info() must name the path that was meant.
The references are local: under kind 2, 128 consecutive rows share a centre (oracle/zebra_oracle.c), so the near neighbours of a row of cluster c
are the rows [128 c, 128 c + 128), which zo.synth_rows regenerates.  PROBE CLUSTERS: cluster 0 (a control), the cluster below and the one starting
at each of the rows 2^20, 2^21, 2^22, and the last full cluster.  PROBE QUERIES, two per probe cluster: one bit-equal to a stored row, one a stored
row plus 0.05 x fixed noise.  METRICS: L2 squared and corrected cosine (the two matrix-core kinds), Manhattan (no specialised instance at d = 1024:
exact_score_generic_kernel), and L2 squared with the family's ZH_*_PATH=1 switch (the specialised D = 1024 f32 instance).  The parity cosine key
ranks by similarity, its nearest rows by key are the least similar rows of the whole table, and no local reference exists for that: left out.

THE CONDITION THE REFERENCES REST ON: for every probe query and metric the smallest key over all rows OUTSIDE the query's cluster exceeds the
largest key INSIDE it; then every top-k with k <= 127 and every radius up to the cluster's largest key is decided by the 128 regenerated rows.
tests/probes/large_table_margin.py scans the whole table on the CPU with the oracle's keys and prints, per metric, the minimum over the 16 probe
queries of (smallest outside key) / (largest inside key):

    L2 squared        12.07
    corrected cosine  12.12
    Manhattan         3.41

and, for the 768 lines of the exact k-NN graph's slabs (the stored rows of the six boundary clusters as queries), the same ratio from f32 matrix
products (not the oracle's arithmetic; the ratio is far from 1): L2 squared 11.58, corrected cosine 11.89.  The condition only guards
against false alarms: every assertion is an equality, so a row that wrongly qualified fails the test.  The filtered search under the selective mask
and the three forest families need no such condition: their references take every allowed row / every leaf-mate (from ix.get_forest()).

THE GRAPH FAMILY (section 7; zh_knn_graph_refine, _refine_rev, _reverse, _descent, zh_index_set_graph with zh_search_graph_batch and
zh_search_graph_filtered_batch) needs no such condition: its input graph is tests/seam_cases.py's group-local one over the 128-row clusters --
line 128 c + j of a probe cluster names 128 c + (j + o_t) mod 128, t < 8, every other line has count 0 -- so every answer on a probe cluster is
the family's numpy reference on the 128 regenerated rows, and a read that wraps to a low row finds an empty line, another cluster's line or another
row's values where the reference has the right ones.  The graph goes in as a HOST array of 268 MB, which takes the host entries' 64 MiB pinned
chunks (8 388 608 entries each) through their loop at its real size; the section leaves the table as it found it (no removals, no graph attached).

NOT COVERED, so that the gap stays visible: the exact self-join (zh_join.hip) -- quadratic, about 50 s at this size, and it has no slab form --
and snapshots of a 17 GB table.  Nor does this table reach an offset counted in 16-byte vectors (the fp16 copy's u32x4e units): that one stays
below 2^32 until 33.5M rows of d = 1024.

The module takes half a minute on one MI355X (the slowest tests, 5 to 6 s each: the forest self-join's f32 leaf sweep over 1.76e10 leaf pairs,
and the forest graph's matrix-core path, which visits every leaf of the forest for a slab of 32 lines; the graph family's section adds 4 s: a
descent over the whole table 0.3 to 0.4 s a case, the slab refinements 0.2 s a case with their four 268 MB uploads, the searches 0.1 s).  Run alone, give it a limit of its own:
timeout 600 pytest -m gpu tests/test_gpu_large_table.py"""
import concurrent.futures
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)

D, KIND, CL = 1024, 2, 128
N = 2**22 + 4096 + 37
BOUNDARIES = (2**20, 2**21, 2**22)
PROBE_CLUSTERS = [0] + [c for b in BOUNDARIES for c in (b // CL - 1, b // CL)] + [N // CL - 1]
NOISE_SEED = 0x1A26E7AB
NONE = np.uint64(2**64 - 1)
METRICS = ("l2sq", "cos", "manhattan")


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def metric_of(za, name):
    return {"l2sq": (za.L2SquaredDistance(), zo.L2SQ, 0), "cos": (za.CosineDistance(parity=False), zo.COSINE, zo.CORRECTED),
            "manhattan": (za.ManhattanDistance(), zo.MANHATTAN, 0)}[name]


def oracle_metric(name):
    return {"l2sq": (zo.L2SQ, 0), "cos": (zo.COSINE, zo.CORRECTED), "manhattan": (zo.MANHATTAN, 0)}[name]


# ---------------------------------------------------------------- rows, queries, local references (computed once, never changed)
@functools.lru_cache(maxsize=None)
def cluster_rows(c):
    return zo.synth_rows(CL, D, row0=CL * c, kind=KIND)


@functools.lru_cache(maxsize=None)
def probe_queries():
    """(Q [16, D], the cluster of every query): per probe cluster a stored row and another stored row plus 0.05 x noise"""
    noise = zo.synth_rows(len(PROBE_CLUSTERS), D, seed=NOISE_SEED, kind=0)
    Q = np.empty((2 * len(PROBE_CLUSTERS), D), np.float32)
    for j, c in enumerate(PROBE_CLUSTERS):
        X = cluster_rows(c)
        Q[2 * j] = X[(37 * j + 5) % CL]
        Q[2 * j + 1] = X[(53 * j + 71) % CL] + np.float32(0.05) * noise[j]
    return Q, np.repeat(PROBE_CLUSTERS, 2)


def rows_by_id(ids):
    """the stored rows of ascending ids, regenerated run by run"""
    out = np.empty((ids.size, D), np.float32)
    brk = np.flatnonzero(np.diff(ids) != 1) + 1
    for s, e in zip(np.r_[0, brk].tolist(), np.r_[brk, ids.size].tolist()):
        out[s:e] = zo.synth_rows(e - s, D, row0=int(ids[s]), kind=KIND)
    return out


def ranked(X, ids, q, om, omode):
    """(ids, keys) of the rows X (stored rows `ids`) against q, ascending by (key, id)"""
    keys = np.asarray(zo.distance_batch(om, omode, X, q), np.uint64)
    o = np.lexsort((ids, keys))
    return ids[o].astype(np.uint64), keys[o]


@functools.lru_cache(maxsize=None)
def cluster_ranking(name, keep=None):
    """per probe query: its cluster's rows ranked by (key, id); keep: 'even' (the rows the dense mask allows), 'live' (rows 100 .. 199 removed)"""
    om, omode = oracle_metric(name)
    Q, cl = probe_queries()
    out = []
    for q, c in zip(Q, cl.tolist()):
        ids = np.arange(CL * c, CL * c + CL, dtype=np.int64)
        sel = np.ones(CL, bool)
        if keep == "even":
            sel = ids % 2 == 0
        elif keep == "live":
            sel = (ids < 100) | (ids >= 200)
        out.append(ranked(np.ascontiguousarray(cluster_rows(c)[sel]), ids[sel], q, om, omode))
    return out


def check_topk(got, ref, k, id_map=None):
    """got = (ids, keys, counts) at top_k = k; ref: per query the ranked (ids, keys) of every row that can be in the answer"""
    ids, keys, counts = got
    assert ids.shape == (len(ref), k) and ids.dtype == np.uint64 and keys.dtype == np.uint64
    for b, (rid, rkey) in enumerate(ref):
        c = min(k, rid.size)
        want = rid[:c] if id_map is None else id_map[rid[:c].astype(np.int64)]
        assert counts[b] == c, (b, counts[b], c)
        assert (ids[b, :c] == want).all(), (b, ids[b, :c][ids[b, :c] != want][:4], want[ids[b, :c] != want][:4])
        assert (keys[b, :c] == rkey[:c]).all(), b
        assert (ids[b, c:] == NONE).all() and (keys[b, c:] == NONE).all(), b


def csr(ref, max_keys, id_map=None):
    """the range search's (offsets, ids, keys) from per-query ranked candidates"""
    offs, ids, keys = [0], [], []
    for (rid, rkey), mk in zip(ref, max_keys):
        hit = rkey <= mk
        ids.append(rid[hit] if id_map is None else id_map[rid[hit].astype(np.int64)])
        keys.append(rkey[hit])
        offs.append(offs[-1] + int(hit.sum()))
    return np.array(offs, np.uint64), np.concatenate(ids), np.concatenate(keys)


def same_csr(got, want):
    for g, r, what in zip(got, want, ("offsets", "ids", "keys")):
        assert g.dtype == np.uint64 and g.shape == r.shape and (g == r).all(), what


def hundredth_keys(name):
    """each probe query's 100th in-cluster key"""
    return np.array([rkey[99] for _, rkey in cluster_ranking(name)], np.uint64)


# ---------------------------------------------------------------- the forest's leaves
def leaf_tables(f, n):
    """per tree (the leaf of every row [n] or -1, the members of its reachable leaves: test_gpu_fknn.py's forest_leaves)"""
    from tests.test_gpu_fknn import forest_leaves
    out = []
    for leaves in forest_leaves(f):
        leaf_of = np.full(n, -1, np.int32)
        for j, ids in enumerate(leaves):
            leaf_of[ids] = j
        out.append((leaf_of, leaves))
    return out


def leaf_mates(tables, a):
    """ascending: the union over the trees of the members of row a's leaf, a itself included; and the sum of the leaves' lengths"""
    parts = [leaves[leaf_of[a]] for leaf_of, leaves in tables if leaf_of[a] >= 0]
    return np.unique(np.concatenate(parts + [np.zeros(0, np.int64)])), sum(p.size for p in parts)


class Mates:
    """the leaf-mates of a set of rows with their f32 values: the union is regenerated once, a row's mates are views into it"""

    def __init__(self, tables, rows):
        self.mates, self.leaf_rows = {}, {}
        for a in rows:
            self.mates[a], self.leaf_rows[a] = leaf_mates(tables, a)
        self.union = np.unique(np.concatenate([np.zeros(0, np.int64)] + list(self.mates.values())))
        self.X = rows_by_id(self.union)

    def row(self, a):
        return self.X[np.searchsorted(self.union, a)]

    def ranked(self, a, om, omode, q=None, keep=lambda c, a: c != a):
        """(ids, keys) by (key, id) of a's mates that `keep` admits, against the query q (default: row a itself)"""
        c = self.mates[a]
        c = c[keep(c, a)]
        if c.size == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        return ranked(np.ascontiguousarray(self.X[np.searchsorted(self.union, c)]), c, self.row(a) if q is None else q, om, omode)


# ---------------------------------------------------------------- the table
@pytest.fixture(scope="module")
def table(za):
    ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 3), device=0, reserve_rows=N)
    ix.append_synthetic(N, kind=KIND)
    assert ix.stored_rows() == N and len(ix) == N
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def forest(table):
    """the table built; -> leaf_tables of its forest"""
    table.build()
    tables = leaf_tables(table.get_forest(), N)
    assert len(tables) == 3 and all((leaf_of >= 0).all() for leaf_of, _ in tables)  # every row in one leaf of every tree
    return tables


def on_path(monkeypatch, var, path):
    for v in ("ZH_FILTER_PATH", "ZH_RANGE_PATH", "ZH_KNN_PATH", "ZH_KNN_LIST_CAP", "ZH_FKNN_PATH", "ZH_FKNN_LIST_CAP", "ZH_FJOIN_PATH",
              "ZH_FJOIN_CAND_CAP", "ZH_FRANGE_PATH", "ZH_FRANGE_CAND_CAP", "ZH_WALK_LOG_CHUNKS", "ZH_ROW_ORDER"):
        monkeypatch.delenv(v, raising=False)
    if path:
        monkeypatch.setenv(var, str(path))


# ---------------------------------------------------------------- 1. rows at the boundaries
def test_rows_at_the_boundaries(table):
    for b in BOUNDARIES:
        assert (table.read_rows(b - 16, 32).view(np.uint32) == zo.synth_rows(32, D, row0=b - 16, kind=KIND).view(np.uint32)).all(), b
    assert (table.read_rows(N - 37, 37).view(np.uint32) == zo.synth_rows(37, D, row0=N - 37, kind=KIND).view(np.uint32)).all()


# ---------------------------------------------------------------- 2. exact search
@pytest.mark.parametrize("name", METRICS)
def test_exact_search(za, table, monkeypatch, name):
    on_path(monkeypatch, None, 0)
    m = metric_of(za, name)[0]
    Q, _ = probe_queries()
    got = table.search_exact_batch(Q, 100, m)
    info = table.exact_info()
    assert info["rows_live"] == N and info["batch"] == 16 and info["redone"] == 0 and info["path"] == (1 if name == "manhattan" else 2), info
    check_topk(got, cluster_ranking(name), 100)


# ---------------------------------------------------------------- 3. filtered search
def dense_mask():
    mask = np.ones(N, bool)
    for c in PROBE_CLUSTERS:
        mask[CL * c + 1:CL * c + CL:2] = False
    return mask


@pytest.mark.parametrize("name,forced", [("l2sq", 0), ("cos", 0), ("manhattan", 0), ("l2sq", 1)])
def test_filtered_search_dense_mask(za, table, monkeypatch, name, forced):
    """every row allowed but the odd rows of the probe clusters: the answer is the top-50 of the cluster's 64 even rows"""
    on_path(monkeypatch, "ZH_FILTER_PATH", forced)
    m = metric_of(za, name)[0]
    Q, _ = probe_queries()
    got = table.search_exact_filtered_batch(Q, 50, m, dense_mask())
    info = table.filtered_info()
    path = 1 if (forced or name == "manhattan") else 2
    assert info["rows_live"] == N and info["rows_allowed"] == N - len(PROBE_CLUSTERS) * CL // 2 and info["batch"] == 16, info
    assert info["path"] == path and info["redone"] == 0 and info["tiles_skipped"] == 0, info
    check_topk(got, cluster_ranking(name, "even"), 50)


@pytest.mark.parametrize("name", METRICS)
def test_filtered_search_selective_mask(za, table, monkeypatch, name):
    """only the eight probe clusters allowed (1024 rows: path 1 gathers them); the reference is the brute force over exactly these rows"""
    on_path(monkeypatch, None, 0)
    m, om, omode = metric_of(za, name)
    Q, _ = probe_queries()
    ids = np.concatenate([np.arange(CL * c, CL * c + CL, dtype=np.int64) for c in PROBE_CLUSTERS])
    X = np.concatenate([cluster_rows(c) for c in PROBE_CLUSTERS])
    mask = np.zeros(N, bool)
    mask[ids] = True
    got = table.search_exact_filtered_batch(Q, 50, m, mask)
    info = table.filtered_info()
    assert info["rows_live"] == N and info["rows_allowed"] == ids.size and info["path"] == 1 and info["redone"] == 0, info
    check_topk(got, [ranked(X, ids, q, om, omode) for q in Q], 50)


# ---------------------------------------------------------------- 4. range search
@pytest.mark.parametrize("name,forced", [("l2sq", 0), ("cos", 0), ("manhattan", 0), ("l2sq", 1)])
def test_range_search(za, table, monkeypatch, name, forced):
    on_path(monkeypatch, "ZH_RANGE_PATH", forced)
    m = metric_of(za, name)[0]
    Q, _ = probe_queries()
    mk = hundredth_keys(name)
    want = csr(cluster_ranking(name), mk)
    assert (np.diff(want[0]) >= 100).all()
    got = table.search_range_batch(Q, metric=m, max_keys=mk)
    info = table.range_info()
    path = 1 if (forced or name == "manhattan") else 2
    assert info["rows_live"] == N and info["batch"] == 16 and info["path"] == path and info["redone"] == 0 and info["hits"] == want[1].size, info
    same_csr(got, want)
    assert (table.range_count_batch(Q, metric=m, max_keys=mk) == np.diff(want[0])).all()
    assert table.range_info()["path"] == path and table.range_info()["hits"] == want[1].size


# ---------------------------------------------------------------- 5. exact k-NN graph
@pytest.mark.parametrize("forced", [0, 1])
@pytest.mark.parametrize("name", ["l2sq", "cos"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_knn_graph_slab(za, table, monkeypatch, boundary, name, forced):
    """256 lines, the cluster below the boundary and the one starting at it; per line the brute force over its own cluster, itself taken out"""
    on_path(monkeypatch, "ZH_KNN_PATH", forced)
    m, om, omode = metric_of(za, name)
    first, k = boundary - CL, 32
    ids, keys, counts = table.knn_graph(k, m, first, 2 * CL)
    info = table.knn_info()
    assert info["rows_live"] == N and info["lines"] == 2 * CL and info["k"] == k and info["path"] == (1 if forced else 2) and info["redone"] == 0, info
    assert ids.shape == (2 * CL, k) and (counts == k).all()
    for i in range(2 * CL):
        a = first + i
        c = a // CL
        own = np.arange(CL * c, CL * c + CL, dtype=np.int64)
        rid, rkey = ranked(np.ascontiguousarray(cluster_rows(c)[own != a]), own[own != a], cluster_rows(c)[a - CL * c], om, omode)
        assert (ids[i] == rid[:k]).all() and (keys[i] == rkey[:k]).all(), (a, ids[i][:4], rid[:4])


# ---------------------------------------------------------------- 6. the forest families
def test_small_forest_a_stored_row_reaches_its_own_leaves(za, monkeypatch):
    """what the large forest range test rests on, checked against test_gpu_frange.py's full reference (the oracle's walk): a query bit-equal to
    a stored row reaches, at probe = 1, that row's own leaf in every tree of a built forest -- its candidates are the row and its leaf-mates"""
    from tests.test_gpu_frange import Walk, jth_keys, keyed, within
    n, d = 4096 + 37, 256
    X = zo.synth_rows(n, d)
    ix = za.LSHIndex(d, za.LSHIndexOptions(256, 3), device=0)
    ix.add(X)
    f = ix.get_forest()
    tables = leaf_tables(f, n)
    rows = list(range(0, n, 61)) + [n - 1]
    Q = np.ascontiguousarray(X[rows])
    walk = Walk(X, 256, f, Q, 1)
    assert walk.visits == 3 * len(rows)
    for a, cands in zip(rows, walk.cands):
        mates, leaf_rows = leaf_mates(tables, a)
        assert (cands == mates).all() and a in mates.tolist(), a
    assert walk.leaf_rows == sum(leaf_mates(tables, a)[1] for a in rows)
    ref = keyed(X, Q, walk, zo.L2SQ, 0)
    mk = jth_keys(ref, 30)
    for path in (2, 1):
        on_path(monkeypatch, "ZH_FRANGE_PATH", path)
        same_csr(ix.search_range_forest_batch(Q, metric=za.L2SquaredDistance(), max_keys=mk, probe=1), within(ref, mk))
        assert ix.range_forest_info()["path"] == path
    ix.close()


@pytest.mark.parametrize("forced", [0, 1])
@pytest.mark.parametrize("boundary", [2**22, 2**21])
def test_forest_knn_graph_slab(za, table, forest, monkeypatch, boundary, forced):
    """32 lines straddling the boundary; per line its leaf-mates over the trees, regenerated by id, duplicates across trees dropped"""
    tables = forest
    first, n, k = boundary - 16, 32, 32
    mates = Mates(tables, range(first, first + n))
    on_path(monkeypatch, "ZH_FKNN_PATH", forced)
    for name in ("l2sq", "cos"):
        m, om, omode = metric_of(za, name)
        ids, keys, counts = table.knn_graph_forest(k, m, first, n)
        info = table.knn_forest_info()
        assert info["rows_live"] == N and info["lines"] == n and info["k"] == k and info["trees"] == 3, info
        assert info["path"] == (1 if forced else 2) and info["redone"] == 0, info
        assert info["pairs"] == sum(mates.leaf_rows[a] - 3 for a in range(first, first + n)), info
        for i in range(n):
            rid, rkey = mates.ranked(first + i, om, omode)
            c = min(k, rid.size)
            assert c == k and counts[i] == c and (ids[i, :c] == rid[:c]).all() and (keys[i, :c] == rkey[:c]).all(), (name, first + i)


@pytest.mark.parametrize("forced", [2, 1])
def test_forest_range_search(za, table, forest, monkeypatch, forced):
    """queries bit-equal to the stored rows on both sides of every boundary and to the last row, probe = 1: the row and its leaf-mates"""
    tables = forest
    rows = [r for b in BOUNDARIES for r in (b - 1, b)] + [N - 1]
    mates = Mates(tables, rows)
    Q = np.ascontiguousarray(np.stack([mates.row(a) for a in rows]))
    on_path(monkeypatch, "ZH_FRANGE_PATH", forced)
    for name in ("l2sq", "cos"):
        m, om, omode = metric_of(za, name)
        ref = [mates.ranked(a, om, omode, keep=lambda c, a: np.ones(c.size, bool)) for a in rows]
        assert all(rid[0] == a for (rid, _), a in zip(ref, rows))  # a row is its own nearest
        mk = np.array([rkey[99] for _, rkey in ref], np.uint64)
        want = csr(ref, mk)
        got = table.search_range_forest_batch(Q, metric=m, max_keys=mk, probe=1)
        info = table.range_forest_info()
        assert info["rows_live"] == N and info["batch"] == len(rows) and info["trees"] == 3 and info["probe"] == 1, info
        assert info["path"] == forced and info["redone"] == 0 and info["hits"] == want[1].size, info
        assert info["visits"] == 3 * len(rows) and info["leaf_rows"] == sum(mates.leaf_rows[a] for a in rows), info
        same_csr(got, want)
        assert (table.range_forest_count_batch(Q, metric=m, max_keys=mk, probe=1) == np.diff(want[0])).all()


@functools.lru_cache(maxsize=None)
def join_threshold():
    """the key below which about one pair in a thousand of the probe clusters' own 8 x 8128 pairs falls"""
    keys = []
    for c in PROBE_CLUSTERS:
        X = cluster_rows(c)
        keys += [np.asarray(zo.distance_batch(zo.L2SQ, 0, np.ascontiguousarray(X[a + 1:]), X[a]), np.uint64) for a in range(CL - 1)]
    keys = np.sort(np.concatenate(keys))
    return keys[keys.size // 1000]


def join_path2(za, table, monkeypatch):
    """the whole table's forest self-join on path 2: the count first, then the arrays at exactly that capacity -> (a, b, keys), info"""
    m = metric_of(za, "l2sq")[0]
    mk = join_threshold()
    on_path(monkeypatch, "ZH_FJOIN_PATH", 0)
    total = table.self_join_forest_count(metric=m, max_key=mk)
    assert table.join_forest_info()["path"] == 2 and table.join_forest_info()["pairs"] == total
    got = table.self_join_forest(metric=m, max_key=mk, capacity=total)
    info = table.join_forest_info()
    assert got[0].size == total and info["pairs"] == total and info["rows_live"] == N and info["trees"] == 3, info
    assert info["path"] == 2 and info["redone"] == 0 and info["candidates"] >= total, info
    return got, info


def test_forest_self_join_against_the_oracle(za, table, forest, monkeypatch, capsys):
    """the whole table on path 2; compared: every pair whose a lies in a probe cluster, against a's leaf-mates with b > a"""
    tables = forest
    _, om, omode = metric_of(za, "l2sq")
    mk = join_threshold()
    got, info = join_path2(za, table, monkeypatch)
    with capsys.disabled():
        print("\n[large table] forest self-join: %d pairs in all, %d leaf pairs" % (got[0].size, info["leaf_pairs"]))
    assert info["leaf_pairs"] == sum(ids.size * (ids.size - 1) // 2 for _, leaves in tables for ids in leaves), info
    assert (got[0] < got[1]).all() and got[1].max() < N
    # the reference: neighbouring probe clusters share most of their leaves, so their leaf-mates are regenerated together
    ra, rb, rk = [], [], []
    for group in ([0], [1, 2], [3, 4], [5, 6], [7]):
        rows = [r for j in group for r in range(CL * PROBE_CLUSTERS[j], CL * PROBE_CLUSTERS[j] + CL)]
        mates = Mates(tables, rows)
        with concurrent.futures.ThreadPoolExecutor(8) as pool:
            per = list(pool.map(lambda a: mates.ranked(a, om, omode, keep=lambda c, a: c > a), rows))
        for a, (rid, rkey) in zip(rows, per):
            hit = rkey <= mk
            ra.append(np.full(int(hit.sum()), a, np.uint64)); rb.append(rid[hit]); rk.append(rkey[hit])
    ra, rb, rk = np.concatenate(ra), np.concatenate(rb), np.concatenate(rk)
    assert ra.size >= 8  # (the threshold keeps pairs of the probe clusters)
    sel = np.isin(got[0] // np.uint64(CL), np.array(PROBE_CLUSTERS, np.uint64))
    assert sel.sum() == ra.size and (got[0][sel] == ra).all() and (got[1][sel] == rb).all() and (got[2][sel] == rk).all()


def test_forest_self_join_paths_agree(za, table, forest, monkeypatch):
    """the whole table again with the f32 leaf sweep forced: the same three arrays, the same leaf pairs"""
    got, info2 = join_path2(za, table, monkeypatch)
    on_path(monkeypatch, "ZH_FJOIN_PATH", 1)
    forced = table.self_join_forest(metric=metric_of(za, "l2sq")[0], max_key=join_threshold(), capacity=got[0].size)
    info = table.join_forest_info()
    assert info["path"] == 1 and info["redone"] == 0 and info["pairs"] == got[0].size and info["leaf_pairs"] == info2["leaf_pairs"], info
    assert info["rows_live"] == N and info["tiles"] == 0 and info["candidates"] == 0, info
    for g, p in zip(got, forced):
        assert g.dtype == np.uint64 and g.shape == p.shape and (g == p).all()


# ---------------------------------------------------------------- 7. the graph family
G_K = 8  # in_k = g_k of the cluster-local graph


@functools.lru_cache(maxsize=None)
def cluster_graph():
    """(the table as seam_cases sees it, the graph on the host: lines of the probe clusters full, every other line count 0)"""
    from tests import seam_cases as sc
    tb = sc.Table(N, D, 0, kind=KIND, group=CL)
    ids, counts = np.full((N, G_K), NONE, np.uint64), np.zeros(N, np.uint32)
    for c in PROBE_CLUSTERS:
        ids[CL * c:CL * c + CL], counts[CL * c:CL * c + CL] = sc.graph(N, G_K, 0, CL * c, CL * c + CL, group=CL)
    # five chunks of the host entries' pinned staging (the size is the library's: tests/test_seam_reference.py); the info counts no chunks
    assert -(-ids.nbytes // sc.REFINE_CHUNK_BYTES) == 5 and sc.REFINE_CHUNK_BYTES // 8 == 8388608
    for b in BOUNDARIES:  # probe rows on both sides of every boundary
        assert counts[b - 1] == G_K and counts[b] == G_K and (ids[b - 1] < b).all() and (ids[b] >= b).all()
    ids.setflags(write=False); counts.setflags(write=False)
    return tb, (ids, counts)


def graph_slabs():
    """the 256 lines around each boundary and the last probe cluster: (first row, lines)"""
    return [(b - CL, 2 * CL) for b in BOUNDARIES] + [(CL * PROBE_CLUSTERS[-1], CL)]


def cluster_lines(graph, c):
    return graph[0][CL * c:CL * c + CL], graph[1][CL * c:CL * c + CL]


def same_lines(got, ref, what):
    for g, r, name in zip(got, ref, ("first", "second", "third")):
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), (what, name, np.argwhere(g != r)[:3].tolist())


@pytest.mark.parametrize("rev_k", [0, 4])
@pytest.mark.parametrize("name", METRICS)
def test_graph_refinement_slabs(za, table, monkeypatch, name, rev_k):
    from tests import seam_cases as sc
    on_path(monkeypatch, None, 0)
    m, om, omode = metric_of(za, name)
    tb, graph = cluster_graph()
    k = 16
    for first, n in graph_slabs():
        got = table.knn_graph_refine(graph, k, m, first, n, reverse=rev_k)
        info = table.knn_refine_rev_info() if rev_k else table.knn_refine_info()
        assert info["rows_live"] == N and info["lines"] == n and info["in_k"] == G_K and info["k"] == k and info["launches"] == 1, info
        assert info["keyed"] > n * G_K and (got[2] == k).all()
        for c in range(first // CL, (first + n) // CL):
            ref, _ = sc.local_refine(tb, *cluster_lines(graph, c), c, k, om, omode, rev_k)
            same_lines(tuple(a[CL * c - first:CL * c - first + CL] for a in got), ref, (name, rev_k, c))


def test_graph_reverse_slabs(table):
    from tests import seam_cases as sc
    tb, graph = cluster_graph()
    rev_k = 4
    for first, n in graph_slabs():
        got = table.knn_graph_reverse(graph, rev_k, first, n)
        info = table.knn_reverse_info()
        assert info["rows_live"] == N and info["lines"] == n and info["edges"] == len(PROBE_CLUSTERS) * CL * G_K and info["max_degree"] == G_K, info
        assert info["kept"] == int(got[1].sum()) > 0 and (got[2] == G_K).all()
        for c in range(first // CL, (first + n) // CL):
            ref, _ = sc.local_reverse(tb, *cluster_lines(graph, c), c, rev_k)
            same_lines(tuple(a[CL * c - first:CL * c - first + CL] for a in got), ref, ("reverse", c))


@pytest.mark.parametrize("rev_k", [0, 4])
@pytest.mark.parametrize("name", METRICS)
def test_graph_descent_whole_table(za, table, monkeypatch, name, rev_k):
    """the whole table on the device entry: the probe clusters' lines against the local reference, every other count 0"""
    import torch
    from tests import seam_cases as sc
    on_path(monkeypatch, None, 0)
    m, om, omode = metric_of(za, name)
    tb, graph = cluster_graph()
    k, rounds = 8, 3
    d_ids, d_counts = torch.from_numpy(graph[0].view(np.int64).copy()).cuda(), torch.from_numpy(graph[1].view(np.int32).copy()).cuda()
    out = [torch.full((N, k), 0x5A5A5A5A, dtype=torch.int64, device="cuda"), torch.full((N, k), 0x5A5A5A5A, dtype=torch.int64, device="cuda"),
           torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    table.knn_graph_descent_device(d_ids.data_ptr(), d_counts.data_ptr(), G_K, rev_k, k, rounds, m, *[o.data_ptr() for o in out])
    info = table.knn_descent_info()
    assert info["rows_live"] == N and info["rounds_run"] >= 2 and info["active_round"][0] == N, info
    total = 0
    for c in PROBE_CLUSTERS:
        got = (out[0][CL * c:CL * c + CL].cpu().numpy().view(np.uint64), out[1][CL * c:CL * c + CL].cpu().numpy().view(np.uint64),
               out[2][CL * c:CL * c + CL].cpu().numpy().view(np.uint32))
        same_lines(got, sc.local_descent(tb, *cluster_lines(graph, c), c, rev_k, k, info["rounds_run"], om, omode), (name, rev_k, c))
        total += int(got[2].sum())
    assert int(out[2].sum(dtype=torch.int64)) == total == len(PROBE_CLUSTERS) * CL * k
    assert int((out[0] != -1).sum()) == total and int((out[1] != -1).sum()) == total  # (every other line: no neighbours)
    del d_ids, d_counts, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", METRICS)
def test_graph_search_and_filtered_search(za, table, monkeypatch, name):
    """the module's 16 probe queries, each seeded inside its cluster; the filter allows the even rows"""
    from tests import seam_cases as sc
    on_path(monkeypatch, None, 0)
    m, om, omode = metric_of(za, name)
    tb, graph = cluster_graph()
    Q, cl = probe_queries()
    top_k, beam, n_seed = 10, 64, 4
    seeds = np.array([[CL * c + (29 * i + 41 * t + 3) % CL for t in range(n_seed)] for i, c in enumerate(cl.tolist())], np.uint64)
    even = np.arange(N) % 2 == 0
    table.set_graph(graph)
    try:
        assert table.graph_info()["attached"] == 1 and table.graph_info()["g_rows"] == N and table.graph_info()["g_k"] == G_K
        for allowed in (None, even):
            if allowed is None:
                got = table.search_graph_batch(Q, top_k, m, beam=beam, seeds=seeds)
                info = table.search_graph_info()
            else:
                got = table.search_graph_filtered_batch(Q, top_k, m, allowed, beam=beam, seeds=seeds)
                info = table.search_graph_filtered_info()
            fields = ("seeds", "iterations", "expanded", "keyed") + (() if allowed is None else ("offered", "returned"))
            total = {f: 0 for f in fields}
            for i, c in enumerate(cl.tolist()):
                ref, rinfo = sc.local_search(tb, *cluster_lines(graph, c), c, Q[i:i + 1], seeds[i:i + 1], top_k, beam, 1, 0, om, omode, allowed)
                same_lines(tuple(a[i:i + 1] for a in got), ref, (name, allowed is not None, i))
                for f in fields:
                    total[f] += rinfo[f]
            assert {f: info[f] for f in fields} == total and info["queries"] == len(cl) and info["launches"] == 1, (info, total)
            assert (got[2] == top_k).all()
    finally:
        table.drop_graph()
    assert table.graph_info()["attached"] == 0


# ---------------------------------------------------------------- 8. compaction (last: it changes the table)
def test_compaction(za, table, monkeypatch):
    on_path(monkeypatch, None, 0)
    m = metric_of(za, "l2sq")[0]
    Q, cl = probe_queries()
    mk = hundredth_keys("l2sq")
    before = table.search_exact_batch(Q, 100, m)
    before_range = table.search_range_batch(Q, metric=m, max_keys=mk)
    gone = np.arange(100, 200, dtype=np.uint64)
    assert table.remove(gone).size == 100
    new_ids, cinfo = table.compact()
    assert cinfo["rows_before"] == N and cinfo["rows_after"] == N - 100 and table.stored_rows() == N - 100
    old = np.arange(N, dtype=np.uint64)
    assert (new_ids[gone.astype(np.int64)] == NONE).all() and (new_ids[:100] == old[:100]).all() and (new_ids[200:] == old[200:] - np.uint64(100)).all()
    for b in BOUNDARIES:
        p = b - 100 - 16
        assert (table.read_rows(p, 32).view(np.uint32) == zo.synth_rows(32, D, row0=p + 100, kind=KIND).view(np.uint32)).all(), b
    assert (table.read_rows(N - 137, 37).view(np.uint32) == zo.synth_rows(37, D, row0=N - 37, kind=KIND).view(np.uint32)).all()
    # the searches again: the brute force over the live rows of the query's cluster under the id map (cluster 0 keeps its rows 0 .. 99) ...
    ref = cluster_ranking("l2sq", "live")
    after = table.search_exact_batch(Q, 100, m)
    info = table.exact_info()
    assert info["rows_live"] == N - 100 and info["path"] == 2 and info["redone"] == 0, info
    check_topk(after, ref, 100, new_ids)
    after_range = table.search_range_batch(Q, metric=m, max_keys=mk)
    assert table.range_info()["rows_live"] == N - 100 and table.range_info()["path"] == 2 and table.range_info()["redone"] == 0
    same_csr(after_range, csr(ref, mk, new_ids))
    # ... which for every query outside cluster 0 is the earlier answer under the map
    far = cl != 0
    assert far.sum() == 14
    assert (after[0][far] == new_ids[before[0][far].astype(np.int64)]).all() and (after[1][far] == before[1][far]).all()
    for b in np.flatnonzero(far).tolist():
        s, e, s2, e2 = int(before_range[0][b]), int(before_range[0][b + 1]), int(after_range[0][b]), int(after_range[0][b + 1])
        assert (after_range[1][s2:e2] == new_ids[before_range[1][s:e].astype(np.int64)]).all() and (after_range[2][s2:e2] == before_range[2][s:e]).all()

"""Every query family on a loaded snapshot against its saved twin (tests/test_gpu_snapshot.py states the contract: a loaded index is
indistinguishable from the saved one for every later call).  The families merged after snapshots -- the filtered exact search, the exact range
search, self-join and k-NN graph, the forest k-NN graph, self-join and range search -- read state that zh_index_load sets up by another route than
add / build / remove / compact do: the tombstones (the live list and the live-row bitmap are first made from them), the forest's host mirror, the
derived copies that are not in the file (the fp16 rows, their scales, the scan's row order and the row -> position map) and counters that start
over.  Every call here is made on a twin pair and compared four ways: the twins' arrays byte for byte and their infos field for field; the
loaded index's arrays bit for bit against the family's own oracle-built reference (imported from the family's module, never restated); the
path the call took against the one that was forced (`redone` 0); and, per family and path, as the FIRST call a freshly loaded index answers.

Shapes.  B is the forest families' shape B (4096 + 37 rows, d = 256, max_node_size 256, 3 trees, id_base 2^40) with the 400 bit-identical rows
of their `Bdup`; the forest families take path 2 on it.  The exact-side families (exact, filtered, range, join, k-NN graph) take path 2 only from
8192 live -- filtered: allowed -- rows on, and no switch lowers that: ZH_FILTER_PATH=2 skips the cost rule alone, the other switches only know 1.
On B their rule refuses path 2 and path 1 is asserted under both values of the switch.  So that their path 2 is met on a loaded index at all,
state W is B's recipe at 16384 + 512 + 37 rows (the random-half filter then allows 8606 of them): a 17 MB file, loaded in milliseconds.  The
dimension sweep has a 2000-row index (forest path 2) and an 8192 + 37-row one (range and filtered path 2) per dimension for the same reason.

References.  Exact and filtered: the oracle's brute force per query.  Range: the oracle's key matrix.  Exact join and graph: the oracle on
sampled rows a (the removed rows' tile-mates, the bit-identical block and the table's ends among them) -- every pair / line of those rows, as
the family modules do at their path-2 shape; the full arrays are compared between the paths and the twins.  Forest families: from
ld.get_forest().  Thresholds are the reference's own keys: each query's 30th smallest, UINT64_MAX for three stored rows as queries, and for the
joins the key that keeps a few hundred pairs of the sample's share -- which is the key of the bit-identical block, 79 800 tied pairs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker)
from tests import test_gpu_fjoin as fj  # noqa: E402  (forest_pairs, keyed, within, quantile_key, each_pair_once)
from tests import test_gpu_fknn as fk  # noqa: E402  (candidates, ranked, check_lines)
from tests import test_gpu_frange as fr  # noqa: E402  (Walk, keyed, within, jth_keys, each_hit_once, queries_b, rows_bdup)
from tests.test_gpu_exact import all_metrics, check_exact  # noqa: E402
from tests.test_gpu_filtered import brute, check as check_filtered, random_half  # noqa: E402
from tests.test_gpu_join import oracle_rows, pairs_from, restrict, threshold_from_sample  # noqa: E402
from tests.test_gpu_knn import check_lines, oracle_lines  # noqa: E402
from tests.test_gpu_range import key_matrix, kth_keys, reference as range_reference  # noqa: E402
from tests.test_gpu_snapshot import roundtrip, same_state  # noqa: E402

NONE = np.uint64(2**64 - 1)
ESTATE = -4
K = 10
BASE = 1 << 40
NB, DB, OPT_B = 4096 + 37, 256, (256, 3)
NW = 16384 + 512 + 37
METRICS = {0: (zo.L2SQ, 0), 1: (zo.L2, 0), 2: (zo.COSINE, zo.PARITY), 3: (zo.COSINE, zo.CORRECTED)}  # index into all_metrics -> the oracle's metric / mode
PATH_SWITCHES = ("ZH_FILTER_PATH", "ZH_RANGE_PATH", "ZH_JOIN_PATH", "ZH_KNN_PATH", "ZH_FKNN_PATH", "ZH_FJOIN_PATH", "ZH_FRANGE_PATH")
OTHER_SWITCHES = ("ZH_ROW_ORDER", "ZH_ROW_HALF_META_ONLY", "ZH_SNAPSHOT_CHUNK_BYTES", "ZH_KNN_LIST_CAP", "ZH_FKNN_LIST_CAP", "ZH_FJOIN_CAND_CAP",
                  "ZH_FRANGE_CAND_CAP", "ZH_WALK_LOG_CHUNKS")
FAMILIES = ("exact", "filtered", "range", "join", "knn", "fknn", "fjoin", "frange", "counts")
EXACT_SIDE = ("exact", "filtered", "range", "join", "knn")
FOREST_SIDE = ("fknn", "fjoin", "frange")
# Fields of an info that legitimately differ between twins driven through the same calls: none was found.  (The list may never name path,
# redone, rows_live, hits, pairs, lines, visits, leaf_rows or tiles.)
INFO_EXCLUDED = ()


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


@pytest.fixture(scope="module")
def snapdir(tmp_path_factory):
    return tmp_path_factory.mktemp("snapshot_families")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in PATH_SWITCHES + OTHER_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def force(monkeypatch, path):
    """every family's switch to `path` (1 or 2; read per call), or the library's own rule (None)"""
    for name in PATH_SWITCHES:
        if path is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(path))


def family(name):
    return name.split("/")[0]


# --------------------------------------------------------------------------------------------------------------------- the host's side
class Case:
    """what the host knows of an index state: the stored rows, which of them are removed or outside every tree, the ids' base, the options,
    the queries, the two filters and the sampled rows of the exact join's and graph's reference"""

    def __init__(self, X, dead, d, opts, Q, base=BASE, outside=(), masks=None):
        n = X.shape[0]
        self.X, self.n, self.d, self.opts, self.Q, self.base = X, n, d, opts, np.ascontiguousarray(Q, np.float32), base
        self.alive = np.ones(n, bool)
        self.alive[np.asarray(sorted(dead), np.int64)] = False
        self.live = np.flatnonzero(self.alive)
        self.dead = np.flatnonzero(~self.alive)
        self.outside = np.asarray(sorted(outside), np.int64)
        if masks is None:
            last = np.zeros(n, bool)
            last[n - 40:] = True
            masks = {"half": random_half(n), "last40": last}
        self.masks = masks
        picked = set(np.random.default_rng(7).choice(n, min(96, n), replace=False).tolist())
        picked |= {r for r in (0, 79, 81, 82, 94, 111, 128, 999, 1000, 1001, 1203, 1399, 1400, n - 3, n - 2) if r < n}
        self.sample = sorted(r for r in picked if self.alive[r])
        self.lines = sorted(set(range(0, n, 5)) | picked | set(self.dead.tolist()) | set(self.outside.tolist()))  # the forest graph's checked lines

    @property
    def mfma(self):
        return self.d in (256, 384, 512, 768, 1024)  # (zh_exact_mfma_supported, for the metrics used here)


class Thresholds:
    range = join = fjoin = None
    frange = None


class Reference:
    """the oracle-built answers of every family for one case and metric; `forest`: the LOADED index's get_forest()"""

    def __init__(self, c, forest, om, omode, parts=FAMILIES):
        X, live, Q, base = c.X, c.live, c.Q, c.base
        self.om, self.omode, self.parts = om, omode, parts
        self.built = forest["roots"].size > 0
        self.leaf_ids = forest["leaf_ids"].tobytes()
        t = self.t = Thresholds()
        all3 = np.full(3, NONE, np.uint64)
        t.frange = {1: np.zeros(Q.shape[0], np.uint64), 2: np.zeros(Q.shape[0], np.uint64)}
        t.join = t.fjoin = np.uint64(0)
        if "filtered" in parts:
            self.allowed = {name: np.flatnonzero(mask & c.alive) for name, mask in c.masks.items()}
            self.filtered = {name: brute(X, rows, Q, K, om, omode) for name, rows in self.allowed.items()}
        if "range" in parts:
            keys = key_matrix(X, live, Q, om, omode)
            t.range = kth_keys(keys, 30)
            self.range = range_reference(keys, live, t.range, base)
            self.range_all = range_reference(keys[-3:], live, all3, base)
        if "join" in parts:
            per = oracle_rows(X, live, c.sample, om, omode)
            t.join = threshold_from_sample(per, 300, live.size)
            self.join = pairs_from(c.sample, per, t.join, base)
        if "knn" in parts:
            self.knn = oracle_lines(X, live, c.sample, om, omode, K, base)
        if not self.built:
            return
        if "fknn" in parts:
            cands, self.fknn_pairs, self.fknn_lines = fk.candidates(forest, c.n)
            self.fknn = fk.ranked(X, cands, c.lines, om, omode, base)
        if "fjoin" in parts:
            fa, fb, self.leaf_pairs, _, _ = fj.forest_pairs(forest)
            full = fj.keyed(X, fa, fb, om, omode, base)
            t.fjoin = fj.quantile_key(full, 300)
            self.fjoin = fj.within(full, t.fjoin)
        if "frange" in parts:
            self.frange = {}
            for probe in (1, 2):
                walk = fr.Walk(X, c.opts[0], forest, Q, probe)
                ref = fr.keyed(X, Q, walk, om, omode)
                t.frange[probe] = fr.jth_keys(ref, 30)
                self.frange[probe] = (walk, fr.within(ref, t.frange[probe], base))
                if probe == 1:
                    self.frange_all = fr.within(ref[-3:], all3, base)


# ------------------------------------------------------------------------------------------------------------------------- the calls
def family_calls(za, ix, c, t, m):
    """(name, call, info) of the nine calls, in one order; `t`: the thresholds (Reference.t), `m`: the metric.  A name is family[/variant];
    call() -> the tuple of output arrays; info() -> the info dict (a tuple of dicts for the count calls)"""
    Q, Q3 = c.Q, np.ascontiguousarray(c.Q[-3:])
    all3 = np.full(3, NONE, np.uint64)
    yield "exact", lambda: ix.search_exact_batch(Q, K, m), ix.exact_info
    for name, mask in c.masks.items():
        yield "filtered/" + name, lambda mask=mask: ix.search_exact_filtered_batch(Q, K, m, mask), ix.filtered_info
    yield "range", lambda: ix.search_range_batch(Q, metric=m, max_keys=t.range), ix.range_info
    yield "range/all", lambda: ix.search_range_batch(Q3, metric=m, max_keys=all3), ix.range_info
    yield "join", lambda: ix.self_join(metric=m, max_key=t.join), ix.join_info
    yield "knn", lambda: ix.knn_graph(K, m), ix.knn_info
    yield "fknn", lambda: ix.knn_graph_forest(K, m), ix.knn_forest_info
    yield "fjoin", lambda: ix.self_join_forest(metric=m, max_key=t.fjoin), ix.join_forest_info
    for probe in (1, 2):
        yield ("frange/p%d" % probe, lambda probe=probe: ix.search_range_forest_batch(Q, metric=m, max_keys=t.frange[probe], probe=probe),
               ix.range_forest_info)
    yield "frange/all", lambda: ix.search_range_forest_batch(Q3, metric=m, max_keys=all3, probe=1), ix.range_forest_info
    yield ("counts/exact", lambda: (ix.range_count_batch(Q, metric=m, max_keys=t.range), np.array([ix.self_join_count(metric=m, max_key=t.join)], np.uint64)),
           lambda: (ix.range_info(), ix.join_info()))
    yield ("counts/forest", lambda: (ix.range_forest_count_batch(Q, metric=m, max_keys=t.frange[1], probe=1),
                                     ix.range_forest_count_batch(Q, metric=m, max_keys=t.frange[2], probe=2),
                                     np.array([ix.self_join_forest_count(metric=m, max_key=t.fjoin)], np.uint64)),
           lambda: (ix.range_forest_info(), ix.join_forest_info()))


def answers(za, calls, only=None):
    """name -> (arrays, info) of every call (`only`: of these families or names), or (("error", code), None) where the library refused"""
    out = {}
    for name, call, info in calls:
        if only is not None and family(name) not in only and name not in only:
            continue
        try:
            got = call()
        except za.ZhError as e:
            out[name] = (("error", e.code), None)
            continue
        out[name] = (tuple(np.asarray(a) for a in got), info())
    return out


def same_twins(a, b):
    """two indexes' answers(): the same refusals, the same bytes in every array, the same infos field by field"""
    assert list(a) == list(b)
    for name in a:
        (ga, ia), (gb, ib) = a[name], b[name]
        if ia is None or ib is None:
            assert ga == gb, (name, ga if ia is None else "answered", gb if ib is None else "answered")
            continue
        assert len(ga) == len(gb), name
        for j, (x, y) in enumerate(zip(ga, gb)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, j)
        for da, db in zip(ia if isinstance(ia, tuple) else (ia,), ib if isinstance(ib, tuple) else (ib,)):
            assert {f: v for f, v in da.items() if f not in INFO_EXCLUDED} == {f: v for f, v in db.items() if f not in INFO_EXCLUDED}, (name, da, db)


def same_arrays(a, b, names=None):
    """the arrays alone (two indexes whose infos may differ: another row order, another history)"""
    for name in (names or a):
        assert a[name][1] is not None and b[name][1] is not None, name
        for j, (x, y) in enumerate(zip(a[name][0], b[name][0])):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, j)


def expected_path(name, forced, c, r):
    """the path the library's rules give the call when every switch is `forced` (1 or 2)"""
    fam = family(name)
    wide = c.mfma and c.live.size >= max(K + 1, 8192)
    if fam == "exact":
        return 2 if wide else 1  # (its own rule; no switch)
    if fam == "filtered":
        return 2 if c.mfma and forced == 2 and r.allowed[name.split("/")[1]].size >= 8192 else 1
    if fam in ("range", "join", "knn"):
        return 2 if wide and forced != 1 else 1
    return 2 if c.mfma and c.opts[0] >= 64 and forced != 1 else 1


def u64(*arrays):
    assert all(a.dtype == np.uint64 for a in arrays)


def same_csr(got, want, what):
    assert len(got) == len(want) == 3
    for g, w, part in zip(got, want, ("0", "1", "2")):
        assert g.dtype == np.uint64 and g.shape == w.shape and (g == w).all(), (what, part)


def answer_ids(name, got):
    fam = family(name)
    if fam in ("exact", "filtered", "knn", "fknn"):
        return [got[0]]
    if fam in ("range", "frange"):
        return [got[1]]
    return [got[0], got[1]] if fam in ("join", "fjoin") else []


def check_reference(name, got, info, c, r, forced):
    """one call's answer on the LOADED index against the family's reference, bit for bit; the path it took against the forced one (None: the
    library's rule, not asserted); rows_live; no removed row -- for the forest families no row outside the trees either -- in any answer"""
    fam, base = family(name), c.base
    infos = info if isinstance(info, tuple) else (info,)
    for i in infos:
        assert i["redone"] == 0 and i["rows_live"] == c.live.size, (name, i)
    gone = c.dead if fam in EXACT_SIDE or name == "counts/exact" else np.concatenate([c.dead, c.outside])
    for ids in answer_ids(name, got):
        assert not np.isin(ids, gone.astype(np.uint64) + np.uint64(base)).any(), name
    if forced is not None:
        if fam == "counts":
            want = [expected_path(f, forced, c, r) for f in (("range", "join") if name == "counts/exact" else ("frange", "fjoin"))]
            assert [i["path"] for i in infos] == want, (name, infos, want)
        else:
            assert info["path"] == expected_path(name, forced, c, r), (name, info)
    if name == "exact":
        assert got[2].dtype == np.uint32
        u64(got[0], got[1])
        check_exact(got, c.X[c.live], c.Q, K, r.om, r.omode, ids_of=c.live, id_base=base)
    elif fam == "filtered":
        which = name.split("/")[1]
        assert got[2].dtype == np.uint32 and info["rows_allowed"] == r.allowed[which].size, info
        u64(got[0], got[1])
        check_filtered(got, r.filtered[which], K, r.om, id_base=base)
    elif fam == "range":
        want = r.range if name == "range" else r.range_all
        same_csr(got, want, name)
        assert info["hits"] == want[1].size and info["batch"] == want[0].size - 1, info
    elif fam == "join":
        u64(*got)
        assert (got[0] < got[1]).all() and info["pairs"] == got[0].size, info
        same_csr(restrict(got, c.sample, base), r.join, name)
    elif fam == "knn":
        assert got[0].shape == (c.n, K) and info["lines"] == c.live.size and info["k"] == K, info
        check_lines(got, c.sample, r.knn, K)
        assert (got[2][c.dead] == 0).all() and (got[0][c.dead] == NONE).all() and (got[1][c.dead] == NONE).all()
        assert (got[2][c.live] == min(K, c.live.size - 1)).all()
    elif fam == "fknn":
        assert got[0].shape == (c.n, K) and info["pairs"] == r.fknn_pairs and info["lines"] == r.fknn_lines and info["k"] == K, info
        fk.check_lines(got, r.fknn, K)
        assert (got[2][c.dead] == 0).all() and (got[2][c.outside] == 0).all()
    elif fam == "fjoin":
        same_csr(got, r.fjoin, name)
        local = (got[0] - np.uint64(base), got[1] - np.uint64(base), got[2])  # (each_pair_once packs a pair into one word: rows, not ids)
        assert fj.each_pair_once(local) and info["pairs"] == got[0].size and info["leaf_pairs"] == r.leaf_pairs, info
    elif fam == "frange":
        probe = 2 if name == "frange/p2" else 1
        walk, want = r.frange[probe]
        if name == "frange/all":
            want = r.frange_all
        else:
            assert info["visits"] == walk.visits and info["leaf_rows"] == walk.leaf_rows, (info, walk.visits, walk.leaf_rows)
        same_csr(got, want, name)
        assert fr.each_hit_once(got) and info["hits"] == want[1].size and info["probe"] == probe, info
    elif name == "counts/exact":
        assert (got[0] == np.diff(r.range[0])).all() and infos[0]["hits"] == r.range[1].size, infos
        assert infos[1]["pairs"] == int(got[1][0]), infos  # (the full call's size is compared by the caller: the reference is a sample)
    elif name == "counts/forest":
        assert (got[0] == np.diff(r.frange[1][1][0])).all() and (got[1] == np.diff(r.frange[2][1][0])).all()
        assert int(got[2][0]) == r.fjoin[0].size and infos[1]["pairs"] == r.fjoin[0].size, infos
    else:
        raise AssertionError(name)


def check_all(got, c, r, forced):
    for name, (arrays, info) in got.items():
        assert info is not None, (name, arrays)
        check_reference(name, arrays, info, c, r, forced)
    if "join" in got and "counts/exact" in got:  # the counts are the sizes the full calls returned
        assert int(got["counts/exact"][0][1][0]) == got["join"][0][0].size
        assert (got["counts/exact"][0][0] == np.diff(got["range"][0][0])).all()
    if "fjoin" in got and "counts/forest" in got:
        assert int(got["counts/forest"][0][2][0]) == got["fjoin"][0][0].size
        assert (got["counts/forest"][0][0] == np.diff(got["frange/p1"][0][0])).all() and (got["counts/forest"][0][1] == np.diff(got["frange/p2"][0][0])).all()


def drive(za, monkeypatch, ix, ld, c, r, m, forced, only=None):
    """both twins through the same calls in the same order; the twins against each other, the loaded one against the reference"""
    force(monkeypatch, forced)
    a = answers(za, family_calls(za, ix, c, r.t, m), only)
    b = answers(za, family_calls(za, ld, c, r.t, m), only)
    same_twins(a, b)
    check_all(b, c, r, forced)
    return a, b


# ------------------------------------------------------------------------------------------------------------------------ the states
GONE_B = list(range(80, 96, 3)) + list(range(112, 128))  # every third row of a 16-row tile, one whole tile (and, per state, the last row)
_SHARED = {}  # state -> (the saved index, its file, the case): made once per module, never changed
_REFS = {}    # (state, metric) -> Reference


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()
    _REFS.clear()


def rows_w():
    if "rows_w" not in _REFS:
        X = zo.synth_rows(NW, DB).copy()
        X[1000:1400] = X[1000]  # the bit-identical block, as in B
        _REFS["rows_w"] = X
    return _REFS["rows_w"]


def make(za, state):
    """a fresh index in `state` (as add / append / remove left it, never searched) and its case"""
    if state in ("S1", "S2", "W"):
        X = fr.rows_bdup() if state != "W" else rows_w()
        n = X.shape[0]
        gone = GONE_B + [n - 1]
        ix = za.LSHIndex(DB, za.LSHIndexOptions(*OPT_B), device=0, id_base=BASE)
        ix.add(X[:n // 2])
        ix.add(X[n // 2:])
        assert len(ix.remove(np.array(gone, np.uint64) + np.uint64(BASE))) == len(gone)
        Q = fr.queries_b(X)
        outside = ()
        if state == "S2":  # 50 rows appended after the last build: in no tree
            X = np.concatenate([X, zo.synth_rows(n + 50, DB)[n:]])
            ix.append(X[n:])
            outside = range(n, n + 50)
        return ix, Case(X, gone, DB, OPT_B, Q if state != "W" else Q[40:], outside=outside)
    if state == "S3":  # never built
        X = zo.synth_rows(1500, 30)
        ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0, id_base=BASE)
        ix.append(X)
        assert len(ix.remove(np.array([3, 1498], np.uint64) + np.uint64(BASE))) == 2
        return ix, Case(X, [3, 1498], 30, (64, 4), fr.queries_b(X))
    if state == "S6":  # a forest the CPU checker built, injected: arbitrary planes, no samples
        X = zo.synth_rows(4000, 64, seed=0x5EB2D800)
        ix = za.LSHIndex(64, za.LSHIndexOptions(50, 4), device=0)
        ix.append(X)
        ix.set_forest(zo.Forest.build(X, 50, 4, seed=123).arrays())
        return ix, Case(X, [], 64, (50, 4), fr.queries_b(X), base=0)
    raise KeyError(state)


def pair(za, state, tmp_path):
    ix, c = make(za, state)
    ld, p, info = roundtrip(za, ix, tmp_path, state + ".zhs")
    assert info["live_rows"] == c.live.size and info["stored_rows"] == c.n
    same_state(ix, ld)
    return ix, ld, c


def shared(za, snapdir, state):
    if state not in _SHARED:
        ix, c = make(za, state)
        ld, p, _ = roundtrip(za, ix, snapdir, state + ".zhs")
        same_state(ix, ld)
        ld.close()
        _SHARED[state] = (ix, p, c)
    return _SHARED[state]


def reference(za, state, c, ld, mi, parts=FAMILIES):
    """the state's reference for all_metrics[mi], made once (on the loaded index's forest; every index of a state has the same one)"""
    forest = ld.get_forest()
    if (state, mi) not in _REFS:
        _REFS[(state, mi)] = Reference(c, forest, *METRICS[mi], parts=parts)
    r = _REFS[(state, mi)]
    assert r.leaf_ids == forest["leaf_ids"].tobytes() and set(parts) <= set(r.parts)
    return r


def close(*indexes):
    for ix in indexes:
        ix.close()


# ----------------------------------------------------------------------------------------------------------------- S1 and its wide twin
@pytest.mark.parametrize("mi", [0, 1, 2, 3])
def test_s1_built_with_tombstones(za, tmp_path, monkeypatch, mi):
    """shape B filled by two adds, 23 rows removed, the bit-identical block: all nine calls under both values of every switch, for each metric
    the matrix-core paths serve (the other states: L2^2; the wide one and the dimension sweep: L2^2 and corrected cosine)"""
    ix, ld, c = pair(za, "S1", tmp_path)
    assert c.live.size == NB - 23
    r = reference(za, "S1", c, ld, mi)
    lens = [ids.size for leaves in fk.forest_leaves(ld.get_forest()) for ids in leaves]
    assert max(lens) >= 400 and min(lens) == 0  # (the shape: the unsplittable leaf, empty leaves around it)
    walk = r.frange[1][0]
    assert max(walk.visitors.values()) > 16  # (the shape: one leaf with more than 16 visitors)
    m = all_metrics(za)[mi][0]
    for forced in (2, 1):
        a, b = drive(za, monkeypatch, ix, ld, c, r, m, forced)
        assert b["fknn"][1]["path"] == b["fjoin"][1]["path"] == b["frange/p1"][1]["path"] == b["frange/p2"][1]["path"] == forced
        assert b["filtered/last40"][1]["path"] == 1 and b["filtered/last40"][1]["rows_allowed"] == 39  # (row n - 1 is removed)
    close(ix, ld)


@pytest.mark.parametrize("mi", [0, 3])
def test_wide_exact_side_path2(za, tmp_path, monkeypatch, mi):
    """state W: the exact-side families where their rule admits path 2, on a loaded index that never answered anything else"""
    ix, ld, c = pair(za, "W", tmp_path)
    assert c.live.size >= 8192
    r = reference(za, "W", c, ld, mi, parts=EXACT_SIDE)
    assert r.allowed["half"].size >= 8192 and r.allowed["last40"].size == 39
    m = all_metrics(za)[mi][0]
    only = EXACT_SIDE + ("counts/exact",)
    two = drive(za, monkeypatch, ix, ld, c, r, m, 2, only)[1]
    for name in ("exact", "filtered/half", "range", "range/all", "join", "knn"):
        assert two[name][1]["path"] == 2 and two[name][1]["redone"] == 0, (name, two[name][1])
    assert [i["path"] for i in two["counts/exact"][1]] == [2, 2] and two["filtered/last40"][1]["path"] == 1
    one = drive(za, monkeypatch, ix, ld, c, r, m, 1, only)[1]
    for name in ("filtered/half", "range", "range/all", "join", "knn"):
        assert one[name][1]["path"] == 1, (name, one[name][1])
    same_arrays(one, two)  # the full arrays of both paths (the join's and the graph's reference is a sample of rows)
    close(ix, ld)


# --------------------------------------------------------------------------------------------------------- a pristine load per family
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("fam", FAMILIES)
def test_first_call_on_a_fresh_load(za, snapdir, monkeypatch, fam, path):
    """the file loaded afresh; the first call the index ever answers is this family on this path: it makes every piece of derived state it
    needs itself -- the live list, the fp16 copy, the position map, the row -> leaf and group tables -- and leaves the siblings' alone.
    The exact-side families run on W (path 2 needs 8192 rows); the exact search has no switch: W is its path 2, S1 its path 1."""
    mi = 0
    m = all_metrics(za)[mi][0]
    todo = []
    if fam in EXACT_SIDE or fam == "counts":
        wide = not (fam == "exact" and path == 1)
        todo.append(("W" if wide else "S1", "counts/exact" if fam == "counts" else fam, EXACT_SIDE if wide else FAMILIES))
    if fam in FOREST_SIDE or fam == "counts":
        todo.append(("S1", "counts/forest" if fam == "counts" else fam, FAMILIES))
    for state, only, parts in todo:
        ix, p, c = shared(za, snapdir, state)
        ld = za.LSHIndex.load(p, device=0)
        r = reference(za, state, c, ld, mi, parts=parts)
        force(monkeypatch, path)
        got = answers(za, family_calls(za, ld, c, r.t, m), (only,))
        assert got and all(family(name) == fam for name in got)
        check_all(got, c, r, path)
        for name, (_, info) in got.items():
            for i in info if isinstance(info, tuple) else (info,):
                want = 1 if name == "filtered/last40" or (fam == "exact" and path == 1) else 2 if fam == "exact" else path
                assert i["path"] == want and i["redone"] == 0, (name, i)  # a path-2 case that ran on path 1 fails here
        same_twins(answers(za, family_calls(za, ix, c, r.t, m), (only,)), got)
        force(monkeypatch, None)
        for search in ("search_batch", "search_exact_batch"):
            x, y = getattr(ix, search)(c.Q, K, m), getattr(ld, search)(c.Q, K, m)
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y)), search
        assert ix.exact_info() == ld.exact_info()
        ld.close()


# ---------------------------------------------------------------------------------------------------------- S2: rows outside every tree
def test_s2_rows_outside_every_tree(za, tmp_path, monkeypatch):
    ix, ld, c = pair(za, "S2", tmp_path)
    assert c.n == NB + 50 and c.outside.size == 50
    r = reference(za, "S2", c, ld, 0)
    m = all_metrics(za)[0][0]
    for forced in (2, 1):
        a, b = drive(za, monkeypatch, ix, ld, c, r, m, forced)
        assert (b["fknn"][0][2][c.outside] == 0).all() and (b["knn"][0][2][c.outside] == K).all()  # no forest line; an exact line each
        assert b["filtered/last40"][1]["rows_allowed"] == 40 and np.isin(b["filtered/last40"][0][0], c.outside + BASE).all()  # the exact side ranks them
    # built on both: they take part
    ix.build()
    ld.build()
    same_state(ix, ld)
    built = Case(c.X, c.dead, DB, OPT_B, c.Q)
    rb = Reference(built, ld.get_forest(), *METRICS[0])
    for forced in (2, 1):
        a, b = drive(za, monkeypatch, ix, ld, built, rb, m, forced)
        assert (b["fknn"][0][2][c.outside] == K).all()
    close(ix, ld)


# ------------------------------------------------------------------------------------------------------------------ S3: never built
def test_s3_never_built(za, tmp_path, monkeypatch):
    ix, ld, c = pair(za, "S3", tmp_path)
    r = reference(za, "S3", c, ld, 0)
    assert not r.built
    m = all_metrics(za)[0][0]
    for forced in (2, 1):
        force(monkeypatch, forced)
        a = answers(za, family_calls(za, ix, c, r.t, m))
        b = answers(za, family_calls(za, ld, c, r.t, m))
        same_twins(a, b)
        for name in ("fknn", "fjoin", "frange/p1", "frange/p2", "frange/all", "counts/forest"):
            assert b.pop(name) == (("error", ESTATE), None), name  # rows, but no trees: refused, by both
        check_all(b, c, r, forced)
        assert all(i["path"] == 1 for _, info in b.values() for i in (info if isinstance(info, tuple) else (info,)))  # d = 30
    close(ix, ld)


# ------------------------------------------------------------------------------------------------------------- S4: compacted, then saved
def test_s4_compacted_then_saved(za, tmp_path, monkeypatch):
    """every answer of the loaded index is the pre-compaction answer under compact()'s id map, and the reference's on the compacted rows"""
    ix, c = make(za, "S1")
    m = all_metrics(za)[0][0]
    r0 = reference(za, "S1", c, ix, 0)
    force(monkeypatch, 2)
    before = answers(za, family_calls(za, ix, c, r0.t, m))
    new_ids, _ = ix.compact()
    assert (new_ids[c.dead] == NONE).all() and (new_ids[c.live] == np.arange(c.live.size, dtype=np.uint64) + np.uint64(BASE)).all()
    ld, p, info = roundtrip(za, ix, tmp_path, "S4.zhs")
    assert info["stored_rows"] == info["live_rows"] == c.live.size
    same_state(ix, ld)
    cc = Case(np.ascontiguousarray(c.X[c.live]), [], DB, OPT_B, c.Q, masks={name: mask[c.live] for name, mask in c.masks.items()})
    rc = Reference(cc, ld.get_forest(), *METRICS[0])
    a, b = drive(za, monkeypatch, ix, ld, cc, rc, m, 2)
    # compaction keeps the rows' order and every key: the thresholds of before still stand, and so does each answer, under the id map
    after = answers(za, family_calls(za, ld, cc, r0.t, m))

    def moved(ids):
        out = ids.copy()
        at = ids != NONE
        out[at] = new_ids[(ids[at] - np.uint64(BASE)).astype(np.int64)]
        return out

    for name, (old, _) in before.items():
        new = after[name][0]
        fam = family(name)
        if fam in ("exact", "filtered"):
            want = (moved(old[0]), old[1], old[2])
        elif fam in ("knn", "fknn"):
            want = tuple(x[c.live] for x in (moved(old[0]), old[1], old[2]))
        elif fam in ("range", "frange"):
            want = (old[0], moved(old[1]), old[2])
        elif fam in ("join", "fjoin"):
            want = (moved(old[0]), moved(old[1]), old[2])
        else:
            want = old
        for j, (x, y) in enumerate(zip(new, want)):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (name, j)
    drive(za, monkeypatch, ix, ld, cc, rc, m, 1)
    close(ix, ld)


# ------------------------------------------------------------------------------------------------------------ S5: under a scan row order
@pytest.mark.parametrize("order", ["2", "3"])
@pytest.mark.parametrize("state", ["S1", "W"])
def test_s5_under_a_scan_row_order(za, snapdir, tmp_path, monkeypatch, state, order):
    """saved with no order set; both twins then make the fp16 copy in a forced row order (the matrix-core LSH scan makes it, as in
    test_gpu_exact_lifecycle.test_path2_over_the_scan_row_order): the order and the row -> position map are derived on the loaded index.
    Path-2 answers equal the reference and the answers without an order.  S1: the forest families (and the exact side on path 1); W: the
    exact side on path 2."""
    m = all_metrics(za)[0][0]
    plain, _, c = shared(za, snapdir, state)
    only = None if state == "S1" else EXACT_SIDE + ("counts/exact",)
    r = reference(za, state, c, plain, 0, parts=FAMILIES if state == "S1" else EXACT_SIDE)
    force(monkeypatch, 2)
    unordered = answers(za, family_calls(za, plain, c, r.t, m), only)
    ix, ld, _ = pair(za, state, tmp_path)
    monkeypatch.setenv("ZH_ROW_ORDER", order)
    Q8 = zo.synth_queries(8, DB, c.n)
    first = []
    for t in (ix, ld):
        t.set_sweep_mode("approx")  # (tuning state is not saved: set on both)
        t.set_hash_mode("dense")
        first.append(t.search_batch(Q8, K, za.L2Distance()))
        assert t.stats()["scan_order_keys"] == int(order), t.stats()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*first))
    a, b = drive(za, monkeypatch, ix, ld, c, r, m, 2, only)
    for t in (ix, ld):
        assert t.stats()["scan_order_keys"] == int(order)
    paths = {name: info["path"] for name, (_, info) in b.items() if isinstance(info, dict)}
    if state == "S1":
        assert paths["fknn"] == paths["fjoin"] == paths["frange/p1"] == paths["frange/p2"] == 2, paths
    else:
        assert paths["exact"] == paths["filtered/half"] == paths["range"] == paths["join"] == paths["knn"] == 2, paths
    same_arrays(b, unordered)
    close(ix, ld)


# ------------------------------------------------------------------------------------------------------------------ S6: injected forests
def test_s6_injected_forest(za, tmp_path, monkeypatch):
    ix, ld, c = pair(za, "S6", tmp_path)
    assert ld.snapshot["flags"] == 0  # no samples
    r = reference(za, "S6", c, ld, 0)
    m = all_metrics(za)[0][0]
    for forced in (2, 1):
        a, b = drive(za, monkeypatch, ix, ld, c, r, m, forced)
        assert all(i["path"] == 1 for _, info in b.values() for i in (info if isinstance(info, tuple) else (info,)))  # d = 64
    close(ix, ld)


def test_s6_forest_that_lists_a_row_twice(za, tmp_path, monkeypatch):
    """test_gpu_snapshot.test_injected_forests' 64-row forest whose single leaf lists row 5 twice (scan_unsafe travels in the file): whatever the
    saved index answers or refuses for a family, the loaded one does too; where it answers, each row or pair appears once"""
    n, d = 64, 16
    X = zo.synth_rows(n, d, seed=0x5EB2D810)
    ix = za.LSHIndex(d, za.LSHIndexOptions(128, 1), device=0)
    ix.append(X)
    ids = np.concatenate([np.arange(n), [5]]).astype(np.uint32)
    ix.set_forest(dict(plane=[-1], left=[0], right=[n + 1], roots=[0], planes=np.zeros((0, d), np.float32), consts=np.zeros(0, np.float32), leaf_ids=ids))
    ix.remove(np.array([5, 9], np.uint64))
    ld, p, info = roundtrip(za, ix, tmp_path, "twice.zhs")
    assert info["flags"] == 2
    same_state(ix, ld)
    c = Case(X, [5, 9], d, (128, 1), np.ascontiguousarray(X[[0, 5, 17, 63]]), base=0)
    t = Thresholds()
    t.range = np.full(4, NONE, np.uint64)
    t.join = t.fjoin = NONE
    t.frange = {1: t.range, 2: t.range}
    m = all_metrics(za)[0][0]
    for forced in (2, 1):
        force(monkeypatch, forced)
        a = answers(za, family_calls(za, ix, c, t, m))
        b = answers(za, family_calls(za, ld, c, t, m))
        same_twins(a, b)
        for name, (got, info) in b.items():
            if info is None:
                continue
            if family(name) == "fknn":
                for line, count in zip(got[0], got[2]):
                    assert np.unique(line[:count]).size == count
            elif family(name) == "fjoin":
                assert fj.each_pair_once(got)
            elif family(name) == "frange":
                assert fr.each_hit_once(got)
    close(ix, ld)


# -------------------------------------------------------------------------------------------------------------------- S7: future equality
def test_s7_twins_across_later_mutations(za, tmp_path):
    """test_gpu_snapshot.test_twins_across_later_mutations' script -- add, remove, deduplicate, compact, build, add -- with all nine calls compared
    between the twins after every step, on the library's own path rule; the reference after the last step; the two final snapshots byte-identical"""
    n0, n2, n3 = 3600, 533, 300
    X = zo.synth_rows(n0 + n2 + n3, DB).copy()
    X[n0 + 100:n0 + 130] = X[17]
    Q = fr.queries_b(X[:n0])
    m = all_metrics(za)[0][0]
    rng = np.random.default_rng(3)
    ix = za.LSHIndex(DB, za.LSHIndexOptions(*OPT_B), device=0, id_base=BASE)
    ix.add(X[:2000])
    ix.add(X[2000:n0])
    first = rng.choice(n0, 300, replace=False)
    first = first[first != 17]
    ix.remove(first.astype(np.uint64) + np.uint64(BASE))
    ld, p, info = roundtrip(za, ix, tmp_path)
    twins = (ix, ld)
    # thresholds for the steps that are compared between the twins only: the oracle's keys on the saved state
    c0 = Case(X[:n0], first.tolist(), DB, OPT_B, Q)
    t = Reference(c0, dict(roots=np.zeros(0, np.uint32), leaf_ids=np.zeros(0, np.uint32)), *METRICS[0], parts=("range", "join")).t
    t.fjoin = t.join
    t.frange = {1: t.range, 2: t.range}

    def step(what, results, rows, dead):
        assert all(np.asarray(results[0]).tobytes() == np.asarray(x).tobytes() for x in results[1:]), what
        same_state(ix, ld)
        c = Case(rows, dead, DB, OPT_B, Q)
        a, b = (answers(za, family_calls(za, tw, c, t, m)) for tw in twins)
        assert all(info is not None for _, info in b.values()), what
        same_twins(a, b)
        return c

    dead = set(first.tolist())
    step("loaded", [0, 0], X[:n0], dead)
    step("add", [tw.add(X[n0:n0 + n2]) for tw in twins], X[:n0 + n2], dead)
    alive = np.ones(n0 + n2, bool)
    alive[first] = False
    rm = rng.choice(np.flatnonzero(alive), 400, replace=False)
    rm = rm[rm != 17]
    dead |= set(rm.tolist())
    step("remove", [tw.remove(rm.astype(np.uint64) + np.uint64(BASE)) for tw in twins], X[:n0 + n2], dead)
    alive[rm] = False
    dups = np.flatnonzero(zo.find_duplicates(X[:n0 + n2], alive.astype(np.uint8)))
    assert dups.size >= 20
    dead |= set(dups.tolist())
    alive[dups] = False
    step("deduplicate", [tw.deduplicate() for tw in twins], X[:n0 + n2], dead)
    maps = [tw.compact()[0] for tw in twins]
    assert (maps[0] == NONE).sum() == len(dead)
    Xc = np.ascontiguousarray(X[:n0 + n2][alive])
    step("compact", maps, Xc, ())
    step("build", [tw.build() or 0 for tw in twins], Xc, ())
    Xf = np.concatenate([Xc, X[n0 + n2:]])
    c = step("add", [tw.add(X[n0 + n2:]) for tw in twins], Xf, ())
    # after the last step: the reference, with thresholds of its own
    r = Reference(c, ld.get_forest(), *METRICS[0])
    a = answers(za, family_calls(za, ix, c, r.t, m))
    b = answers(za, family_calls(za, ld, c, r.t, m))
    same_twins(a, b)
    check_all(b, c, r, None)
    pa, pb = str(tmp_path / "a.zhs"), str(tmp_path / "b.zhs")
    ix.save(pa)
    ld.save(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    close(ix, ld)


# --------------------------------------------------------------------------------------------------------------------- dimension sweep
@pytest.mark.parametrize("d", [384, 512, 768, 1024])
def test_dimension_sweep(za, tmp_path, monkeypatch, d):
    """each dimension instantiates its own fp16-copy and matrix-core kernels; the copy's first build on a loaded index is under test.  Path 2
    forced, L2^2 and corrected cosine, a fresh load per metric.  A 2000-row index: the forest k-NN graph answers first, on path 2; there the
    range and the filtered search are refused path 2 by their rule (8192 rows) and path 1 is asserted.  An 8192 + 37-row index: the range
    search (L2^2) or the filtered search (cosine) answers first, on path 2."""
    n, N2 = 2000, 8192 + 37
    Xs = zo.synth_rows(N2, d)
    small = Case(Xs[:n], [5, 100, n - 1], d, OPT_B, fr.queries_b(Xs[:n])[48:])
    most = np.arange(N2) % 300 != 7
    wide = Case(Xs, [3, N2 - 1], d, OPT_B, fr.queries_b(Xs)[-20:], masks={"most": most})  # (no leaves here: 17 of the near-copies, rows 0, 17, n - 1)
    force(monkeypatch, 2)
    for c, name, parts, orders in ((small, "small.zhs", ("fknn", "range", "filtered"), (("fknn", "range", "filtered/half"),) * 2),
                                   (wide, "wide.zhs", ("range", "filtered"), (("range", "filtered/most"), ("filtered/most", "range")))):
        ix = za.LSHIndex(d, za.LSHIndexOptions(*OPT_B), device=0, id_base=BASE)
        ix.add(c.X)
        ix.remove(c.dead.astype(np.uint64) + np.uint64(BASE))
        p = str(tmp_path / name)
        ix.save(p)
        ix.close()
        for mi, order in zip((0, 3), orders):
            ld = za.LSHIndex.load(p, device=0)
            assert ld.stats()["row_copy_bytes"] == 0
            r = Reference(c, ld.get_forest(), *METRICS[mi], parts=parts)
            m = all_metrics(za)[mi][0]
            calls = {nm: (call, info) for nm, call, info in family_calls(za, ld, c, r.t, m)}
            for nm in order:
                got = tuple(np.asarray(x) for x in calls[nm][0]())
                info = calls[nm][1]()
                check_reference(nm, got, info, c, r, 2)
                assert info["path"] == (2 if c is wide or nm == "fknn" else 1) and info["redone"] == 0, (nm, info)
            assert ld.stats()["row_copy_bytes"] >= c.n * 2 * d
            ld.close()

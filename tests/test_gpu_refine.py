"""k-NN graph refinement (zh_knn_graph_refine): line i of a slab holds the first k by (key, id) of C(a), a = first_row + i -- a's neighbours in the
caller's graph and their neighbours, a itself out.  The reference is tests/refine_cases.py (pinned on the CPU by tests/test_refine_reference.py):
the definition in numpy and the oracle's distance_batch keys.  Every comparison is bit for bit on ids, keys and counts, and the info fields lines,
listed, keyed and updates are compared with the reference.  Shapes are the smallest that reach each mechanism: 1500 x 30 the generic row loop,
1500 x 256 and 1200 x 768 the specialised row loads, 4200 x 256 only for the two graphs that fill every slot a line can gather."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import refine_cases as rc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ELIMIT = -1, -5
# name -> (rows, dim, id_base, the block of identical rows, rows removed, built with add (max_node_size, trees) or None = append only)
TABLES = {"A": (1500, 30, 1000, True, True, None), "A13": (1500, 30, 0, False, False, None), "B": (1500, 256, 0, True, True, None),
          "B13": (1500, 256, 1 << 40, False, False, None), "C": (1200, 768, 7, True, True, None), "D": (4200, 256, 0, False, False, None),
          "F": (1500, 256, 0, False, False, (64, 3)), "F768": (1200, 768, 0, False, False, (64, 3)), "tiny": (60, 30, 5, False, False, None)}


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


_SHARED = {}  # the shared indexes, closed when the module is done; no test changes one


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()
    keys_of.cache_clear()


@functools.lru_cache(maxsize=None)
def rows_of(name):
    n, d, _, block, _, _ = TABLES[name]
    X = rc.table(n, d, block)
    X.setflags(write=False)
    return X


def make(name, za):
    """a fresh index of a table: (index, X, live, id_base)"""
    n, d, base, _, removed, opts = TABLES[name]
    X = rows_of(name)
    ix = za.LSHIndex(d, za.LSHIndexOptions(*(opts or (64, 3))), device=0, id_base=base)
    (ix.add if opts else ix.append)(X)
    live = np.ones(n, bool)
    if removed:
        gone = rc.removed_rows(n)
        live[gone] = False
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
    return ix, X, live, base


def table(name):
    import zebra_amd
    if name not in _SHARED:
        _SHARED[name] = make(name, zebra_amd)
    return _SHARED[name]


@functools.lru_cache(maxsize=None)
def keys_of(name, mi, rows=None):
    """the oracle's keys of every stored row of a table against each of its rows (or the listed ones) as the query, once per (table, metric)"""
    import zebra_amd
    _, om, omode = thirteen_metrics(zebra_amd)[mi]
    X = rows_of(name)
    return rc.key_rows(X, om, omode, range(X.shape[0]) if rows is None else rows)


def same(got, ref, what=""):
    for g, r, name in zip(got, ref, ("ids", "keys", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        if not (g == r).all():
            at = np.argwhere(g != r)[0].tolist()
            raise AssertionError("%s %s: first difference at %s, got %d, want %d, %d differ" % (what, name, at, g[tuple(at)], r[tuple(at)], int((g != r).sum())))


def info_is(ix, rinfo, live, in_k, k, what=""):
    info = ix.knn_refine_info()
    want = dict(rinfo, rows_live=int(live.sum()), in_k=in_k, k=k, launches=info["launches"])
    assert info == want, (what, info, want)
    assert (info["launches"] >= 1) == (info["lines"] > 0)
    return info


def check(name, za, graph, in_k, k, mi=0, first_row=0, n=None, rows=None, what=""):
    """one host call on a shared table against the reference, info included"""
    ix, X, live, base = table(name)
    m, om, omode = thirteen_metrics(za)[mi]
    got = ix.knn_graph_refine(graph, k, m, first_row, n)
    ref, rinfo = rc.reference(X, graph, in_k, k, live, base, om, omode, first_row, n, keys_of(name, mi, rows))
    same(got, ref, what)
    info_is(ix, rinfo, live, in_k, k, what)
    return got, rinfo


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", ["F", "F768"])
def test_forest_graph_refined(za, name):
    """the forest graph of a built index (max_node_size 64, 3 trees), in_k = k = 8"""
    ix, X, live, base = table(name)
    m = thirteen_metrics(za)[0][0]
    graph = ix.knn_graph_forest(8, m)
    got, rinfo = check(name, za, graph, 8, 8)
    assert rinfo["updates"] > 0 and rinfo["keyed"] < rinfo["listed"]  # (the round found rows the leaves did not hold)


@pytest.mark.parametrize("in_k", rc.IN_KS)
@pytest.mark.parametrize("graph", sorted(rc.GRAPHS))
def test_adversarial_graphs(za, graph, in_k):
    """1500 x 30, id_base 1000, removed rows, 40 identical rows, never built: every input graph at in_k on either side of the instantiation boundary"""
    _, X, live, base = table("A")
    check("A", za, rc.GRAPHS[graph](X.shape[0], in_k, live, base), in_k, min(in_k, 10) + 3, what="%s in_k %d" % (graph, in_k))


@pytest.mark.parametrize("name,graph,in_k", [("B", "block", 32), ("B", "out_of_range", 45), ("B", "self_loops", 5), ("C", "removed", 32),
                                             ("C", "zero_counts", 64), ("C", "ring", 1)])
def test_specialised_row_loads(za, name, graph, in_k):
    _, X, live, base = table(name)
    check(name, za, rc.GRAPHS[graph](X.shape[0], in_k, live, base), in_k, 10, what="%s %s in_k %d" % (name, graph, in_k))


@pytest.mark.parametrize("in_k", [44, 64])
def test_every_slot_of_a_line(za, in_k):
    """4200 x 256: row 0's neighbours' lists are pairwise disjoint -- in_k + in_k^2 candidates, 1980 of the small instantiation's 2048 slots and
    4160 of the large one's 8192; the slab is the first 48 lines (the reference keys 48 x up to 4160 pairs)"""
    _, X, live, base = table("D")
    graph = rc.g_disjoint(X.shape[0], in_k, live, base)
    rows = tuple(range(48))
    got, rinfo = check("D", za, graph, in_k, 1023, first_row=0, n=48, rows=rows)
    assert got[2][0] == 1023 and rinfo["keyed"] >= in_k + in_k * in_k
    C, _, keyed, _ = rc.candidates(graph[0], graph[1], in_k, live, base)
    assert keyed[0] == in_k + in_k * in_k


@pytest.mark.parametrize("k", [1, 5, 32, 40, 1023])
def test_k_below_at_and_above_in_k(za, k):
    """in_k = 32; k = 1023 on lines with fewer candidates: every candidate, the tails filled"""
    _, X, live, base = table("A")
    graph = rc.g_out_of_range(X.shape[0], 32, live, base)
    got, rinfo = check("A", za, graph, 32, k)
    if k == 1023:
        assert int(got[2].sum()) == rinfo["keyed"] and got[2].max() < 1023
    ix = table("A")[0]
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine(graph, 1024, thirteen_metrics(za)[0][0])
    assert e.value.code == ELIMIT
    wide = (np.zeros((X.shape[0], 65), np.uint64), np.zeros(X.shape[0], np.uint32))
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine(wide, 4, thirteen_metrics(za)[0][0])
    assert e.value.code == ELIMIT
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine((np.zeros((X.shape[0], 0), np.uint64), np.zeros(X.shape[0], np.uint32)), 4, thirteen_metrics(za)[0][0])
    assert e.value.code == EINVAL


# ---------------------------------------------------------------- all 13 metric / mode / power combinations
@pytest.mark.parametrize("mi", range(13))
@pytest.mark.parametrize("name", ["A13", "B13"])
def test_every_metric(za, name, mi):
    _, X, live, base = table(name)
    check(name, za, rc.g_self_loops(X.shape[0], 8, live, base), 8, 10, mi=mi, what="%s metric %d" % (name, mi))


# ---------------------------------------------------------------- slabs
def test_slabs(za):
    ix, X, live, base = table("A")
    n, in_k, k = X.shape[0], 5, 7
    m = thirteen_metrics(za)[0][0]
    graph = rc.g_removed(n, in_k, live, base)
    whole, _ = check("A", za, graph, in_k, k)
    check("A", za, graph, in_k, k, first_row=411, n=613, what="a slab in the middle")
    a = ix.knn_graph_refine(graph, k, m, 0, 700)
    b = ix.knn_graph_refine(graph, k, m, 700, n - 700)
    same([np.concatenate([x, y]) for x, y in zip(a, b)], whole, "two slabs")
    gone = int(rc.removed_rows(n)[5])
    got, rinfo = check("A", za, graph, in_k, k, first_row=gone, n=1, what="a slab of one removed row")
    assert got[2][0] == 0 and rinfo == {"lines": 0, "listed": 0, "keyed": 0, "updates": 0}
    got = ix.knn_graph_refine(graph, k, m, 100, 0)
    assert got[0].shape == (0, k) and got[2].shape == (0,)
    got = ix.knn_graph_refine(graph, k, m, n, None)  # (the slab from the end: empty)
    assert got[2].shape == (0,)
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine(graph, k, m, 1000, 501)
    assert e.value.code == EINVAL


def test_k_zero_touches_the_counts_only(za):
    from zebra_amd import _ffi
    ix, X, live, base = table("A")
    n = X.shape[0]
    graph = rc.g_ring(n, 3, live, base)
    ids, keys, counts = np.full((n, 1), 77, np.uint64), np.full((n, 1), 78, np.uint64), np.full(n, 79, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc_ = _ffi.lib().zh_knn_graph_refine(ix._h, P(graph[0]), P(graph[1]), 3, 0, n, 0, 1, 0, P(ids), P(keys), P(counts))
    assert rc_ == 0 and (counts == 0).all() and (ids == 77).all() and (keys == 78).all()
    info = ix.knn_refine_info()
    assert info["k"] == 0 and info["lines"] == 0 and info["keyed"] == 0 and info["launches"] == 0


def test_the_host_entry_streams_the_graph_in_chunks(za, monkeypatch):
    """ZH_REFINE_CHUNK_BYTES lowers the pinned buffers' 64 MiB: 1500 lines of 5 entries go in chunks of 7 lines through both buffers"""
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    graph = rc.g_big_counts(X.shape[0], 5, live, base)
    whole = ix.knn_graph_refine(graph, 6, m)
    monkeypatch.setenv("ZH_REFINE_CHUNK_BYTES", str(7 * 5 * 8 + 3))
    same(ix.knn_graph_refine(graph, 6, m), whole, "chunked")
    monkeypatch.setenv("ZH_REFINE_CHUNK_BYTES", "8")  # (less than a line: a line at a time)
    same(ix.knn_graph_refine(graph, 6, m, 0, 40), [x[:40] for x in whole], "a line per chunk")


# ---------------------------------------------------------------- lifecycle
def test_rows_removed_appended_and_compacted_after_the_graph(za):
    ix, X, live, base = make("F", za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        n, k = X.shape[0], 8
        graph = ix.knn_graph_forest(k, m)
        gone = rc.removed_rows(n)
        live = live.copy()
        live[gone] = False
        assert ix.remove(gone.astype(np.uint64)).size == gone.size
        got = ix.knn_graph_refine(graph, k, m)  # the graph still names the removed rows: ignored, not expanded
        ref, rinfo = rc.reference(X, graph, k, k, live, base, om, omode, K=keys_of("F", 0))
        same(got, ref, "removed after")
        info_is(ix, rinfo, live, k, k)
        assert (got[2][gone] == 0).all()
        # rows appended after: the graph covers fewer lines than the stored rows
        extra = zo.synth_rows(37, X.shape[1], seed=zo.SEED_ROWS + 9)
        ix.append(extra)
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_refine(graph, k, m)
        assert e.value.code == EINVAL
        X2, live2 = np.concatenate([X, extra]), np.concatenate([live, np.ones(37, bool)])
        padded = (np.concatenate([graph[0], np.full((37, k), NONE, np.uint64)]), np.concatenate([graph[2], np.zeros(37, np.uint32)]))
        got = ix.knn_graph_refine(padded, k, m)
        ref, rinfo = rc.reference(X2, padded, k, k, live2, base, om, omode)
        same(got, ref, "appended after")
        info_is(ix, rinfo, live2, k, k)
        assert (got[2][n:] == 0).all()
        # compact: the caller re-keys the graph with the id map
        new_ids, _ = ix.compact()
        keep = np.flatnonzero(live2)
        assert (new_ids[keep] == np.arange(keep.size, dtype=np.uint64)).all() and (new_ids[~live2] == NONE).all()
        rows = padded[0].copy()
        ok = rows < np.uint64(n + 37)
        rows[ok] = new_ids[rows[ok].astype(np.int64)]  # (a removed row's id becomes 2^64-1: ignored)
        rekeyed = (rows[keep], padded[1][keep])
        got = ix.knn_graph_refine(rekeyed, k, m)
        ref, rinfo = rc.reference(X2[keep], rekeyed, k, k, np.ones(keep.size, bool), base, om, omode)
        same(got, ref, "compacted")
        info_is(ix, rinfo, np.ones(keep.size, bool), k, k)
    finally:
        ix.close()


# ---------------------------------------------------------------- properties
def test_refining_the_exact_graph_returns_it(za):
    ix, X, live, base = table("B")
    m = thirteen_metrics(za)[0][0]
    exact = ix.knn_graph(12, m)
    for k in (12, 5):
        got = ix.knn_graph_refine(exact, k, m)
        same(got, (exact[0][:, :k], exact[1][:, :k], np.minimum(exact[2], k).astype(np.uint32)), "k %d" % k)


def test_never_above_the_input_line(za):
    ix, X, live, base = table("C")
    m, om, omode = thirteen_metrics(za)[2]
    in_k, k = 9, 9
    graph = rc.g_zero_counts(X.shape[0], in_k, live, base)
    got = ix.knn_graph_refine(graph, k, m)
    inp = rc.rekey(graph, in_k, live, base, X, om, omode, keys_of("C", 2))
    for a, (iid, ikey) in inp.items():
        c = min(iid.size, k)
        assert got[2][a] >= c
        g = np.lexsort((got[0][a, :c], got[1][a, :c]))  # (the line is sorted: the identity)
        assert (g == np.arange(c)).all()
        above = (got[1][a, :c] > ikey[:c]) | ((got[1][a, :c] == ikey[:c]) & (got[0][a, :c] > iid[:c]))
        assert not above.any(), a


def test_rounds(za):
    ix, X, live, base = table("F")
    m, om, omode = thirteen_metrics(za)[0]
    k = 8
    graph = ix.knn_graph_forest(k, m)
    K = keys_of("F", 0)
    r1 = ix.knn_graph_refine(graph, k, m)
    u1 = ix.knn_refine_info()["updates"]
    r2 = ix.knn_graph_refine(r1, k, m)
    ref2, rinfo2 = rc.reference(X, r1, k, k, live, base, om, omode, K=K)
    same(r2, ref2, "second round")
    i2 = info_is(ix, rinfo2, live, k, k)
    assert u1 > 0 and i2["updates"] == rinfo2["updates"]
    r3 = ix.knn_graph_refine(r2, k, m)
    same(ix.knn_graph_refine(graph, k, m, rounds=3), r3, "rounds=3")
    same(ix.knn_graph_refine(graph, k, m, rounds=1), r1, "rounds=1")
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine(graph, k, m, first_row=1, rounds=2)
    assert e.value.code == EINVAL


def test_complete_graph_is_a_fixed_point(za):
    """60 rows, every line lists the other 59: at most in_k + 1 live rows with complete lists -- the answer is knn_graph's, a second round has no updates"""
    ix, X, live, base = table("tiny")
    m, om, omode = thirteen_metrics(za)[0]
    n = X.shape[0]
    complete = ix.knn_graph(n - 1, m)
    assert (complete[2] == n - 1).all()
    for k in (n - 1, 10):
        got = ix.knn_graph_refine(complete, k, m)
        same(got, ix.knn_graph(k, m), "k %d" % k)
        info = ix.knn_refine_info()
        assert info["updates"] == 0 and info["keyed"] == n * (n - 1) and info["listed"] == n * (n - 1) * n
    got = ix.knn_graph_refine(complete, n - 1, m, rounds=5)  # stops after the first round
    same(got, complete, "rounds")
    # a ring refined to k = 2 is not a fixed point: row x gains x + 2
    ring = rc.g_ring(n, 1, live, base)
    got = ix.knn_graph_refine(ring, 2, m)
    assert ix.knn_refine_info()["updates"] == n and (got[2] == 2).all()


# ---------------------------------------------------------------- entry twins and the caller's stream
def test_device_entry_on_a_callers_busy_stream(za):
    """The device entry agrees with the host entry, and it does so entered on a side stream that still has the uploads of its inputs and fills of
    its outputs pending behind a delay (the protocol of tests/test_gpu_caller_stream.py: stale but valid inputs and sentinel A in place, then on S a
    delay, the copies of the real graph, fills with sentinel B; S must be busy at the call and idle on return; the outputs are read through a third
    stream).  Not probed here: whether S shares a hardware queue with the index's own stream (that module's pick_streams does)."""
    import torch
    from tests.test_gpu_caller_stream import SENT_A, SENT_B, sentinel, u64
    ix, X, live, base = table("B")
    m, om, omode = thirteen_metrics(za)[0]
    n, in_k, k, first_row, nl = X.shape[0], 32, 10, 100, 1203
    graph = rc.g_block(n, in_k, live, base)
    host = ix.knn_graph_refine(graph, k, m, first_row, nl)
    ref, rinfo = rc.reference(X, graph, in_k, k, live, base, om, omode, first_row, nl, keys_of("B", 0))
    same(host, ref, "host")
    dev = torch.device("cuda", 0)
    S, R = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    real_ids, real_counts = torch.from_numpy(graph[0].view(np.int64)).to(dev), torch.from_numpy(graph[1].view(np.int32)).to(dev)
    d_ids, d_counts = torch.zeros_like(real_ids), torch.zeros_like(real_counts)  # the stale input: a valid graph of empty lines
    out = [torch.empty((nl, k), dtype=torch.int64, device=dev), torch.empty((nl, k), dtype=torch.int64, device=dev),
           torch.empty(nl, dtype=torch.int32, device=dev)]
    # idle first: the plain device call, and its wall time for the delay
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_ids.copy_(real_ids); d_counts.copy_(real_counts)
    torch.cuda.synchronize()
    ix.knn_graph_refine_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, k, m, first_row, nl, *[o.data_ptr() for o in out])
    same((u64(out[0].cpu().numpy()), u64(out[1].cpu().numpy()), out[2].cpu().numpy().view(np.uint32)), host, "device, idle")
    info_is(ix, rinfo, live, in_k, k)
    with torch.cuda.stream(S):
        e[0].record(S)
        torch.cuda._sleep(20_000_000)
        e[1].record(S)
    S.synchronize()
    cycles = int(20_000_000 / max(e[0].elapsed_time(e[1]), 1e-3) * 40.0)  # 40 ms
    d_ids.zero_(); d_counts.zero_()
    for o in out:
        o.fill_(sentinel(o, SENT_A))
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        d_ids.copy_(real_ids, non_blocking=True)
        d_counts.copy_(real_counts, non_blocking=True)
        for o in out:
            o.fill_(sentinel(o, SENT_B))
    assert not S.query()
    ix.knn_graph_refine_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, k, m, first_row, nl, *[o.data_ptr() for o in out], stream=S.cuda_stream)
    assert S.query()  # complete on return
    with torch.cuda.stream(R):
        got = [o.to("cpu", non_blocking=True) for o in out]
    R.synchronize()
    same((u64(got[0].numpy()), u64(got[1].numpy()), got[2].numpy().view(np.uint32)), host, "device, busy stream")
    info_is(ix, rinfo, live, in_k, k)


# ---------------------------------------------------------------- the database
def test_database_refined_graph(za):
    X = rows_of("F")[:600]
    db = za.Database(X.shape[1], za.L2SquaredDistance(), za.LSHIndexOptions(64, 3), device=0)
    try:
        docs = ["doc%d" % i for i in range(X.shape[0])]
        db.insert_records(X, docs)
        k, rounds = 6, 2
        forest = db.index.knn_graph_forest(k, db.metric)
        want = db._graph_documents(*db.index.knn_graph_refine(forest, k, db.metric, rounds=rounds))
        got = db.knn_graph_refined(k, rounds)
        assert got == want and set(got) == set(docs)
        live = np.ones(X.shape[0], bool)
        ref = forest
        for _ in range(rounds):
            ref, _ = rc.reference(X, ref, k, k, live, db.index.id_base, zo.L2SQ, 0)
        dist = ref[1].astype(np.uint64).view(np.float64)
        for r in (0, 17, 599):
            c = int(ref[2][r])
            assert got[docs[r]] == [(docs[int(i) - db.index.id_base], float(v)) for i, v in zip(ref[0][r, :c], dist[r, :c])]
    finally:
        db.index.close()

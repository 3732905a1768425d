"""Reverse neighbours (zh_knn_graph_reverse, zh_knn_graph_refine_rev): the capped transposed graph on its own and inside the refinement.  The
reference is tests/reverse_cases.py (pinned on the CPU by tests/test_reverse_reference.py): the definition in numpy and the oracle's
distance_batch keys.  Every comparison is bit for bit on ids, keys, counts and in-degrees, and the info fields the definition fixes are compared
with the reference.  Shapes are the smallest that reach each mechanism: 1500 x 30 (removed rows, id_base 1000, never built) holds lines on both
sides of the in-degree above which a block, not a wave, selects (1024: `same_rows` and `hub` are above it there, the others below), 20 000 x 30
a line of in-degree rows - 1, 1500 x 256 and 1200 x 768 the line kernel's specialised row loads."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_cases as rc  # noqa: E402
from tests import reverse_cases as rv  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_refine import TABLES as REFINE_TABLES, keys_of, rows_of, same  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ELIMIT = -1, -5
HEAVY = 1024  # ZH_REVERSE_HEAVY
PAIRS_REVERSE = [(1, 1), (5, 3), (32, 8), (64, 64), (1, 64)]
PAIRS_FUSED = [(1, 1), (5, 3), (32, 12), (32, 13), (32, 32), (1, 63), (63, 1)]  # 32 + 12 | 32 + 13: the line kernel's two instantiations


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


def make(name, za):
    """a fresh index of one of tests/test_gpu_refine.py's tables, or of H: 20 000 x 30, id_base 1000, every row live -> (index, X, live, id_base)"""
    if name == "H":
        n, d, base, removed, opts = 20000, 30, 1000, False, None
        X = rc.table(n, d, False)
    else:
        n, d, base, _, removed, opts = REFINE_TABLES[name]
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


def same_reverse(got, ref, what=""):
    for g, r, name in zip(got, ref, ("ids", "counts", "degree")):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        if not (g == r).all():
            at = np.argwhere(g != r)[0].tolist()
            raise AssertionError("%s %s: first difference at %s, got %d, want %d, %d differ" % (what, name, at, g[tuple(at)], r[tuple(at)], int((g != r).sum())))


def reverse_info_is(ix, rinfo, live, in_k, rev_k, what=""):
    info = ix.knn_reverse_info()
    want = dict(rinfo, rows_live=int(live.sum()), in_k=in_k, rev_k=rev_k, launches=2)  # (one piece: the wave kernel once, the block kernel once)
    assert info == want, (what, info, want)
    return info


def check_reverse(name, graph, in_k, rev_k, first_row=0, n=None, what=""):
    ix, X, live, base = table(name)
    got = ix.knn_graph_reverse(graph, rev_k, first_row, n)
    ref, rinfo = rv.reference_reverse(graph, in_k, rev_k, live, base, first_row, n)
    same_reverse(got, ref, what)
    reverse_info_is(ix, rinfo, live, in_k, rev_k, what)
    return got, rinfo


def fused_info_is(ix, rinfo, live, in_k, k, what=""):
    info = ix.knn_refine_rev_info()
    want = dict(rinfo, rows_live=int(live.sum()), in_k=in_k, k=k, launches=info["launches"])
    assert info == want, (what, info, want)
    assert (info["launches"] >= 1) == (info["lines"] > 0)
    return info


def check_fused(name, za, graph, in_k, rev_k, k, mi=0, first_row=0, n=None, what=""):
    ix, X, live, base = table(name)
    m, om, omode = thirteen_metrics(za)[mi]
    got = ix.knn_graph_refine(graph, k, m, first_row, n, reverse=rev_k)
    ref, rinfo = rv.reference_rev(X, graph, in_k, rev_k, k, live, base, om, omode, first_row, n, keys_of(name, mi))
    same(got, ref, what)
    fused_info_is(ix, rinfo, live, in_k, k, what)
    return got, rinfo


# ---------------------------------------------------------------- the reverse call
@pytest.mark.parametrize("in_k,rev_k", PAIRS_REVERSE)
@pytest.mark.parametrize("graph", sorted(rv.ALL_GRAPHS))
def test_reverse_of_every_graph(za, graph, in_k, rev_k):
    _, X, live, base = table("A")
    got, rinfo = check_reverse("A", rv.ALL_GRAPHS[graph](X.shape[0], in_k, live, base), in_k, rev_k, what="%s in_k %d rev_k %d" % (graph, in_k, rev_k))
    assert (got[1][~live] == 0).all() and (got[2][~live] == 0).all()  # (nobody names a removed row)
    if graph == "mutual":
        assert rinfo["kept"] == 0 and rinfo["edges"] > 0
    if graph in ("hub", "same_rows"):
        assert rinfo["max_degree"] > HEAVY  # (the block's path)
    if graph == "capped":
        assert rinfo["max_degree"] == 65 < HEAVY


@pytest.mark.parametrize("rev_k", [1, 64])
def test_hub_of_twenty_thousand_rows(za, rev_k):
    """in-degree rows - 1 = 19 999: 78 rounds of the block's four 64-member chunks, all but rev_k of the members must lose"""
    _, X, live, base = table("H")
    n = X.shape[0]
    got, rinfo = check_reverse("H", rv.g_hub(n, 4, live, base), 4, rev_k)
    assert rinfo["max_degree"] == n - 1 and got[2][0] == n - 1 and got[1][0] == rev_k


def test_degrees_on_both_sides_of_the_block_threshold(za):
    """rows 0 .. 3 named by exactly 1023, 1024, 1025 and 1100 lines: the last in-degree a wave serves, and the first ones a block does"""
    _, X, live, base = table("H")
    n = X.shape[0]
    ids = np.full((n, 1), NONE, np.uint64)
    counts = np.zeros(n, np.uint32)
    at = 10
    for t, d in enumerate((HEAVY - 1, HEAVY, HEAVY + 1, 1100)):
        ids[at:at + d, 0] = base + t
        counts[at:at + d] = 1
        at += d
    got, rinfo = check_reverse("H", (ids, counts), 1, 64)
    assert got[2][:4].tolist() == [HEAVY - 1, HEAVY, HEAVY + 1, 1100] and (got[1][:4] == 64).all()


def test_reverse_slabs(za):
    ix, X, live, base = table("A")
    n, in_k, rev_k = X.shape[0], 5, 3
    graph = rv.g_orphan(n, in_k, live, base)
    whole, _ = check_reverse("A", graph, in_k, rev_k)
    check_reverse("A", graph, in_k, rev_k, 0, 1, "the first line")
    check_reverse("A", graph, in_k, rev_k, n - 2, 2, "the last lines")  # (the very last row is removed)
    check_reverse("A", graph, in_k, rev_k, 97, 40, "a slab crossing removed rows")
    a, b = ix.knn_graph_reverse(graph, rev_k, 0, 700), ix.knn_graph_reverse(graph, rev_k, 700, n - 700)
    same_reverse([np.concatenate([x, y]) for x, y in zip(a, b)], whole, "two slabs")
    got = ix.knn_graph_reverse(graph, rev_k, 100, 0)
    assert got[0].shape == (0, rev_k) and got[1].shape == (0,) and got[2].shape == (0,)
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_reverse(graph, rev_k, 1000, 501)
    assert e.value.code == EINVAL
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_reverse(graph, 65)
    assert e.value.code == ELIMIT
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_reverse(graph, 0)
    assert e.value.code == EINVAL


def test_the_host_entry_streams_the_graph_in_chunks(za, monkeypatch):
    ix, X, live, base = table("A")
    graph = rv.g_hub(X.shape[0], 5, live, base)
    whole = ix.knn_graph_reverse(graph, 8)
    monkeypatch.setenv("ZH_REFINE_CHUNK_BYTES", str(7 * 5 * 8 + 3))
    same_reverse(ix.knn_graph_reverse(graph, 8), whole, "chunked")
    monkeypatch.setenv("ZH_REFINE_CHUNK_BYTES", "8")  # (less than a line: a line at a time)
    same_reverse(ix.knn_graph_reverse(graph, 8, 0, 40), [x[:40] for x in whole], "a line per chunk")


def test_device_entries_equal_the_host_entries(za):
    import torch
    ix, X, live, base = table("A")
    m, om, omode = thirteen_metrics(za)[0]
    n, in_k, rev_k, k, first_row, nl = X.shape[0], 5, 3, 7, 100, 1203
    graph = rv.g_orphan(n, in_k, live, base)
    dev = torch.device("cuda", 0)
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    d_ids, d_counts = torch.from_numpy(graph[0].view(np.int64)).to(dev), torch.from_numpy(graph[1].view(np.int32)).to(dev)
    host = ix.knn_graph_reverse(graph, rev_k, first_row, nl)
    hinfo = ix.knn_reverse_info()
    out = [torch.full((nl, rev_k), 5, dtype=torch.int64, device=dev), torch.full((nl,), 5, dtype=torch.int32, device=dev),
           torch.full((nl,), 5, dtype=torch.int32, device=dev)]
    ix.knn_graph_reverse_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, first_row, nl, *[o.data_ptr() for o in out])
    same_reverse((u64(out[0]), u32(out[1]), u32(out[2])), host, "reverse, device")
    assert ix.knn_reverse_info() == hinfo
    host = ix.knn_graph_refine(graph, k, m, first_row, nl, reverse=rev_k)
    hinfo = ix.knn_refine_rev_info()
    out = [torch.full((nl, k), 5, dtype=torch.int64, device=dev), torch.full((nl, k), 5, dtype=torch.int64, device=dev),
           torch.full((nl,), 5, dtype=torch.int32, device=dev)]
    S = torch.cuda.Stream(device=dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    ix.knn_graph_refine_rev_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, k, m, first_row, nl, *[o.data_ptr() for o in out],
                                   stream=S.cuda_stream)
    assert S.query()  # complete on return
    same((u64(out[0]), u64(out[1]), u32(out[2])), host, "fused, device")
    assert ix.knn_refine_rev_info() == hinfo


# ---------------------------------------------------------------- the fused call
@pytest.mark.parametrize("in_k,rev_k", PAIRS_FUSED)
@pytest.mark.parametrize("graph", ["hub", "orphan", "zero_counts", "removed_namers"])
def test_fused_on_the_generic_loop(za, graph, in_k, rev_k):
    _, X, live, base = table("A")
    check_fused("A", za, rv.ALL_GRAPHS[graph](X.shape[0], in_k, live, base), in_k, rev_k, min(in_k, 10) + 3, what="%s %d + %d" % (graph, in_k, rev_k))


@pytest.mark.parametrize("name,graph,in_k,rev_k,mi", [("B", "orphan", 32, 12, 0), ("B", "capped", 32, 13, 2), ("B", "block", 5, 3, 3),
                                                      ("C", "hub", 32, 13, 0), ("C", "removed", 32, 32, 2), ("C", "orphan", 1, 63, 7),
                                                      ("B13", "self_loops", 63, 1, 3), ("B13", "orphan", 5, 3, 0)])
def test_fused_on_the_specialised_row_loads(za, name, graph, in_k, rev_k, mi):
    """1500 x 256 and 1200 x 768; L2 squared, cosine in both modes, Manhattan; B13 has id_base 2^40"""
    _, X, live, base = table(name)
    check_fused(name, za, rv.ALL_GRAPHS[graph](X.shape[0], in_k, live, base), in_k, rev_k, 10, mi=mi, what="%s %s %d + %d" % (name, graph, in_k, rev_k))


def test_fused_slabs(za):
    ix, X, live, base = table("A")
    n, in_k, rev_k, k = X.shape[0], 5, 3, 7
    m = thirteen_metrics(za)[0][0]
    graph = rv.g_orphan(n, in_k, live, base)
    whole, winfo = check_fused("A", za, graph, in_k, rev_k, k)
    _, sinfo = check_fused("A", za, graph, in_k, rev_k, k, first_row=411, n=613, what="a slab in the middle")
    assert 0 < sinfo["kept"] < winfo["kept"] and sinfo["edges"] == winfo["edges"]  # kept is the slab's, edges every row's
    a = ix.knn_graph_refine(graph, k, m, 0, 700, reverse=rev_k)
    b = ix.knn_graph_refine(graph, k, m, 700, n - 700, reverse=rev_k)
    same([np.concatenate([x, y]) for x, y in zip(a, b)], whole, "two slabs")
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_refine(rv.g_hub(n, 33, live, base), k, m, reverse=32)
    assert e.value.code == ELIMIT


def test_forest_graph_with_reverse_finds_more(za):
    """the forest graph of a built index (max_node_size 64, 3 trees), in_k = k = 8: the round with reverse neighbours keys strictly more pairs
    (the reference's own figure, on the CPU) and ends on lines that are nowhere above the forward round's and somewhere below"""
    ix, X, live, base = table("F")
    m, om, omode = thirteen_metrics(za)[0]
    graph = ix.knn_graph_forest(8, m)
    K = keys_of("F", 0)
    _, finfo = rc.reference(X, graph, 8, 8, live, base, om, omode, K=K)
    rev, rinfo = check_fused("F", za, graph, 8, 8, 8)
    assert rinfo["keyed"] > finfo["keyed"] and rinfo["kept"] > 0
    fwd = ix.knn_graph_refine(graph, 8, m)
    found = sum(int((~np.isin(rev[0][a, :rev[2][a]], fwd[0][a, :fwd[2][a]])).sum()) for a in range(X.shape[0]))
    assert found > 0  # rows the forward round did not reach


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("graph,in_k", [("zero_counts", 5), ("hub", 45), ("block", 64)])
def test_rev_k_zero_is_the_forward_call(za, graph, in_k):
    from zebra_amd import _ffi
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    g = rv.ALL_GRAPHS[graph](X.shape[0], in_k, live, base)
    k = 9
    fwd = ix.knn_graph_refine(g, k, m)
    finfo = ix.knn_refine_info()
    ids, keys, counts = np.empty((X.shape[0], k), np.uint64), np.empty((X.shape[0], k), np.uint64), np.zeros(X.shape[0], np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert _ffi.lib().zh_knn_graph_refine_rev(ix._h, P(g[0]), P(g[1]), in_k, 0, 0, X.shape[0], k, m.metric, m.mode, P(ids), P(keys), P(counts)) == 0
    same((ids, keys, counts), fwd, "rev_k = 0")
    assert ix.knn_refine_rev_info() == dict(finfo, rev_k=0, edges=0, kept=0, max_degree=0)
    assert ix.knn_refine_info() == finfo  # (the fused call leaves the forward call's info alone)


@pytest.mark.parametrize("in_k", [1, 5, 32])
def test_mutual_graph_is_the_forward_call(za, in_k):
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    g = rv.g_mutual(X.shape[0], in_k, live, base)
    fwd = ix.knn_graph_refine(g, 6, m)
    finfo = ix.knn_refine_info()
    same(ix.knn_graph_refine(g, 6, m, reverse=8), fwd, "mutual")
    info = ix.knn_refine_rev_info()
    assert info["kept"] == 0 and info["edges"] > 0 and all(info[f] == finfo[f] for f in finfo)


def test_runs_and_entry_order_change_nothing(za):
    """the scatter's order inside a segment differs from run to run, and a line's entries may come in any order: two runs agree bit for bit, and so
    does a run on the graph with every line shuffled -- on lines a wave selects and on lines a block does"""
    ix, X, live, base = table("H")
    m = thirteen_metrics(za)[0][0]
    n, in_k = X.shape[0], 6
    g = rv.g_hub(n, in_k, live, base)
    rng = np.random.default_rng(7)
    shuffled = (rng.permuted(g[0], axis=1), g[1])
    a = ix.knn_graph_reverse(g, 8)
    same_reverse(ix.knn_graph_reverse(g, 8), a, "second run")
    same_reverse(ix.knn_graph_reverse(shuffled, 8), a, "shuffled")
    f = ix.knn_graph_refine(g, 6, m, 0, 3000, reverse=8)
    info = ix.knn_refine_rev_info()
    same(ix.knn_graph_refine(g, 6, m, 0, 3000, reverse=8), f, "second run, fused")
    assert ix.knn_refine_rev_info() == info
    same(ix.knn_graph_refine(shuffled, 6, m, 0, 3000, reverse=8), f, "shuffled, fused")
    assert ix.knn_refine_rev_info() == info


def test_never_above_the_forward_call(za):
    ix, X, live, base = table("C")
    m = thirteen_metrics(za)[2][0]
    in_k, k = 9, 9
    g = rv.g_orphan(X.shape[0], in_k, live, base)
    fwd = ix.knn_graph_refine(g, k, m)
    rev = ix.knn_graph_refine(g, k, m, reverse=5)
    assert (rev[2] >= fwd[2]).all() and (rev[2] > fwd[2]).any()
    for a in range(X.shape[0]):
        c = int(fwd[2][a])
        above = (rev[1][a, :c] > fwd[1][a, :c]) | ((rev[1][a, :c] == fwd[1][a, :c]) & (rev[0][a, :c] > fwd[0][a, :c]))
        assert not above.any(), a


def test_the_exact_graph_is_a_fixed_point(za):
    ix, X, live, base = table("B")
    m = thirteen_metrics(za)[0][0]
    exact = ix.knn_graph(12, m)
    for k in (12, 5):
        got = ix.knn_graph_refine(exact, k, m, reverse=8)
        same(got, (exact[0][:, :k], exact[1][:, :k], np.minimum(exact[2], k).astype(np.uint32)), "k %d" % k)
        info = ix.knn_refine_rev_info()
        assert info["updates"] == 0 and info["kept"] > 0
    same(ix.knn_graph_refine(exact, 12, m, rounds=5, reverse=8), exact, "rounds stop at once")


def test_rounds_with_reverse(za):
    ix, X, live, base = table("F")
    m, om, omode = thirteen_metrics(za)[0]
    k = 8
    graph = ix.knn_graph_forest(k, m)
    r1 = ix.knn_graph_refine(graph, k, m, reverse=8)
    r2 = ix.knn_graph_refine(r1, k, m, reverse=8)
    ref2, rinfo2 = rv.reference_rev(X, r1, k, 8, k, live, base, om, omode, K=keys_of("F", 0))
    same(r2, ref2, "second round")
    fused_info_is(ix, rinfo2, live, k, k)
    r3 = ix.knn_graph_refine(r2, k, m, reverse=8)
    same(ix.knn_graph_refine(graph, k, m, rounds=3, reverse=8), r3, "rounds=3")
    same(ix.knn_graph_refine(graph, k, m, rounds=1, reverse=8), r1, "rounds=1")


def test_compacted_and_loaded_indexes_answer_the_same(za):
    """after compact() with the graph re-keyed through the id map, and on an index loaded from a snapshot of the uncompacted one"""
    ix, X, live, base = make("F", za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        n, in_k, rev_k, k = X.shape[0], 5, 3, 7
        gone = rc.removed_rows(n)
        live = live.copy()
        live[gone] = False
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
        graph = rv.g_orphan(n, in_k, live, base)
        want_rev = ix.knn_graph_reverse(graph, rev_k)
        want = ix.knn_graph_refine(graph, k, m, reverse=rev_k)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "a.snap")
            ix.save(path)
            twin = za.LSHIndex.load(path, device=0)
            try:
                same_reverse(twin.knn_graph_reverse(graph, rev_k), want_rev, "loaded")
                same(twin.knn_graph_refine(graph, k, m, reverse=rev_k), want, "loaded, fused")
            finally:
                twin.close()
        new_ids, _ = ix.compact()
        keep = np.flatnonzero(live)
        rows = graph[0] - np.uint64(base)
        ok = rows < np.uint64(n)
        rows[ok] = new_ids[rows[ok].astype(np.int64)]  # (id_base + new row; a removed row's becomes 2^64-1: ignored)
        rows[~ok] = NONE
        rekeyed = (rows[keep], graph[1][keep])
        all_live = np.ones(keep.size, bool)
        got_rev = ix.knn_graph_reverse(rekeyed, rev_k)
        ref_rev, _ = rv.reference_reverse(rekeyed, in_k, rev_k, all_live, base)
        same_reverse(got_rev, ref_rev, "compacted")
        assert (got_rev[2] == want_rev[2][keep]).all()  # the in-degrees move with their rows (the sample is a hash of the NEW row numbers)
        got = ix.knn_graph_refine(rekeyed, k, m, reverse=rev_k)
        ref, rinfo = rv.reference_rev(X[keep], rekeyed, in_k, rev_k, k, all_live, base, om, omode)
        same(got, ref, "compacted, fused")
        fused_info_is(ix, rinfo, all_live, in_k, k)
    finally:
        ix.close()


def test_database_refined_graph_with_reverse(za):
    X = rows_of("F")[:600]
    db = za.Database(X.shape[1], za.L2SquaredDistance(), za.LSHIndexOptions(64, 3), device=0)
    try:
        docs = ["doc%d" % i for i in range(X.shape[0])]
        db.insert_records(X, docs)
        forest = db.index.knn_graph_forest(6, db.metric)
        want = db._graph_documents(*db.index.knn_graph_refine(forest, 6, db.metric, rounds=2, reverse=4))
        assert db.knn_graph_refined(6, 2, reverse=4) == want and set(want) == set(docs)
        assert db.knn_graph_refined(6, 2) == db._graph_documents(*db.index.knn_graph_refine(forest, 6, db.metric, rounds=2))
    finally:
        db.index.close()

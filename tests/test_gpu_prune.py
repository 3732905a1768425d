"""k-NN graph pruning (zh_knn_graph_prune): line i of a slab holds the unoccluded candidates of a = first_row + i -- P(a) = N'(a) union R'(a)
minus a in (key_a, id) order, a candidate dropped if one kept before it has key_p(c) < key_a(c), at most `degree` kept, `fill` making up a short
line from the dropped ones.  The reference is tests/prune_cases.py (pinned on the CPU by tests/test_prune_reference.py).  Every comparison is bit
for bit on ids, keys and counts and on the six info fields the definition fixes; `keyed` is held to its bounds.  The tables are
tests/test_gpu_refine.py's by their definitions: 1500 x 30 the generic row loop, 1500 x 256 and 1200 x 768 the specialised row loads."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gsearch_cases as gc  # noqa: E402
from tests import prune_cases as pc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests import seam_cases as sc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_refine import keys_of, make, rows_of, same  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ELIMIT = -1, -5


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
    exact.cache_clear()


def table(name):
    import zebra_amd
    if name not in _SHARED:
        _SHARED[name] = make(name, zebra_amd)
    return _SHARED[name]


@functools.lru_cache(maxsize=None)
def exact(name, mi=0, k=64):
    """the exact k-NN graph of a table out of the oracle's keys"""
    _, _, live, base = table(name)
    return pc.exact_graph(keys_of(name, mi), live, base, k)


def graph_of(name, gname, in_k, mi=0):
    _, X, live, base = table(name)
    if gname == "exact":
        ids, _, counts = exact(name, mi)
        return np.ascontiguousarray(ids[:, :in_k]), np.minimum(counts, in_k).astype(np.uint32)
    return pc.GRAPHS[gname](X.shape[0], in_k, live, base)


def info_is(ix, rinfo, prep, live, in_k, rev_k, degree, fill, first_row=0, n=None, what=""):
    info = ix.knn_prune_info()
    n = live.size - first_row if n is None else n
    want = dict(rinfo, rows_live=int(live.sum()), in_k=in_k, rev_k=rev_k, degree=degree, fill=int(fill), keyed=info["keyed"], launches=info["launches"])
    assert info == want, (what, info, want)
    assert (info["launches"] >= 1) == (info["lines"] > 0)
    lo, hi = pc.keyed_bounds(prep, live, first_row, n) if degree else (0, 0)
    assert lo <= info["keyed"] <= hi, (what, lo, info["keyed"], hi)
    assert info["kept"] + info["occluded"] <= info["candidates"] and info["filled"] <= info["occluded"]
    return info


def check(name, za, graph, in_k, degree, fill=0, rev_k=0, mi=0, first_row=0, n=None, prep=None, what=""):
    """one host call on a shared table against the reference, info included"""
    ix, X, live, base = table(name)
    m, om, omode = thirteen_metrics(za)[mi]
    got = ix.knn_graph_prune(graph, degree, m, reverse=rev_k, fill=bool(fill), first_row=first_row, n=n)
    if prep is None:
        prep = pc.prepare(X, graph, in_k, rev_k, live, base, om, omode, keys_of(name, mi))
    ref, rinfo = pc.reference(prep, X.shape[0], degree, fill, live, base, first_row, n)
    same(got, ref, what)
    return got, info_is(ix, rinfo, prep, live, in_k, rev_k, degree, fill, first_row, n, what), prep


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("in_k", pc.IN_KS)
@pytest.mark.parametrize("gname", sorted(pc.GRAPHS) + ["exact"])
def test_every_graph(za, gname, in_k):
    """1500 x 30, id_base 1000, removed rows, 40 identical rows: every input graph at every width, degree below, at and above it, fill off and on"""
    graph = graph_of("A", gname, in_k)
    prep = None
    for degree in pc.degrees(in_k):
        for fill in (0, 1):
            _, _, prep = check("A", za, graph, in_k, degree, fill=fill, prep=prep, what="%s in_k %d degree %d fill %d" % (gname, in_k, degree, fill))


@pytest.mark.parametrize("gname", ["exact", "removed", "self_loops", "all_block"])
@pytest.mark.parametrize("name", ["B", "C"])
def test_specialised_row_loads(za, name, gname):
    graph = graph_of(name, gname, 32)
    _, info, prep = check(name, za, graph, 32, 16, what="%s %s" % (name, gname))
    check(name, za, graph, 32, 8, fill=1, prep=prep, what="%s %s fill" % (name, gname))
    if gname == "exact":
        assert info["occluded"] > info["lines"] and info["kept"] > info["lines"]  # both branches of the rule, many times a line


@pytest.mark.parametrize("gname", sorted(pc.SPECIAL))
def test_lines_with_rows_of_their_own(za, gname):
    """nothing occluded along the axes (degree 30 reached on the LAST candidate, 1 on the first), 30 candidates tied in key_a, m = 64 exactly"""
    X = pc.special_table()
    ix = za.LSHIndex(pc.SPECIAL_DIM, za.LSHIndexOptions(64, 3), device=0)
    try:
        ix.append(X)
        live = np.ones(X.shape[0], bool)
        m = za.L2SquaredDistance()
        graph = pc.special_graph(gname)
        prep = pc.prepare(X, graph, 64, 0, live, 0, zo.L2SQ, 0)
        for degree in pc.SPECIAL[gname][1]:
            for fill in (0, 1):
                got = ix.knn_graph_prune(graph, degree, m, fill=bool(fill))
                ref, rinfo = pc.reference(prep, X.shape[0], degree, fill, live, 0)
                same(got, ref, "%s degree %d fill %d" % (gname, degree, fill))
                info_is(ix, rinfo, prep, live, 64, 0, degree, fill)
                assert got[2][0] == min(degree, len(pc.SPECIAL[gname][0])) or gname == "full64"
    finally:
        ix.close()


# ---------------------------------------------------------------- all 13 metric / mode / power combinations
@pytest.mark.parametrize("mi", range(13))
@pytest.mark.parametrize("name", ["A13", "B13"])
def test_every_metric(za, name, mi):
    """the exact 16-NN graph under each metric's own keys, pruned to 8 with 4 reverse neighbours; B13's ids start at 2^40"""
    graph = graph_of(name, "exact", 16, mi)
    _, info, _ = check(name, za, graph, 16, 8, rev_k=4, mi=mi, what="%s metric %d" % (name, mi))
    assert info["kept"] > info["lines"]


# ---------------------------------------------------------------- reverse neighbours
@pytest.mark.parametrize("gname,in_k,rev_k", [("exact", 32, 0), ("exact", 32, 8), ("exact", 32, 32), ("removed", 5, 8), ("zero_counts", 44, 20),
                                              ("self_loops", 56, 8)])
def test_reverse_neighbours_join_the_candidates(za, gname, in_k, rev_k):
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    graph = graph_of("A", gname, in_k)
    got, info, prep = check("A", za, graph, in_k, 16, rev_k=rev_k, what="%s rev_k %d" % (gname, rev_k))
    if rev_k == 0:
        same(got, ix.knn_graph_prune(graph, 16, m), "reverse=0 is the call without it")
        return
    # the union's candidates against knn_graph_reverse's own output
    rid, rcount, _ = ix.knn_graph_reverse(graph, rev_k)
    N = rc.neighbour_sets(graph[0], graph[1], in_k, live, base)
    total = 0
    for a in np.flatnonzero(live).tolist():
        mine = set(N[a].tolist()) | set((rid[a, :rcount[a]] - np.uint64(base)).astype(np.int64).tolist())
        mine.discard(a)
        assert set(prep[a][0].tolist()) == mine, a
        total += len(mine)
    assert info["candidates"] == total
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_prune(graph, 16, m, reverse=65 - in_k)
    assert e.value.code == ELIMIT


# ---------------------------------------------------------------- fill
def test_fill(za):
    ix, X, live, base = table("B")
    m, om, omode = thirteen_metrics(za)[0]
    graph = graph_of("B", "exact", 32)
    off, ioff, prep = check("B", za, graph, 32, 16)
    on, ion, _ = check("B", za, graph, 32, 16, fill=1, prep=prep)
    assert ioff["filled"] == 0 and ion["filled"] > 0
    for f in ("kept", "occluded", "cut", "candidates", "lines"):
        assert ioff[f] == ion[f], f
    assert int(off[2].sum()) == ioff["kept"] and int(on[2].sum()) == ion["kept"] + ion["filled"]
    assert (on[2] >= off[2]).all() and (on[2] <= 16).all()
    # fill at degree 64: P(a) re-keyed, whatever was occluded
    full, ifull, _ = check("B", za, graph, 32, 64, fill=1, prep=prep)
    inp = rc.rekey(graph, 32, live, base, X, om, omode, keys_of("B", 0))
    for a, (iid, ikey) in inp.items():
        assert full[2][a] == iid.size and (full[0][a, :iid.size] == iid).all() and (full[1][a, :iid.size] == ikey).all(), a
    assert ifull["kept"] + ifull["filled"] == ifull["candidates"] and ifull["filled"] == ifull["occluded"] and ifull["cut"] == 0


# ---------------------------------------------------------------- slabs, limits, degree 0
def test_slabs(za):
    ix, X, live, base = table("A")
    n, in_k, degree = X.shape[0], 32, 8
    m = thirteen_metrics(za)[0][0]
    graph = graph_of("A", "exact", in_k)
    whole, winfo, prep = check("A", za, graph, in_k, degree, rev_k=8)
    cuts = [0, 411, 1024, n]
    parts = [ix.knn_graph_prune(graph, degree, m, reverse=8, first_row=a, n=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    same([np.concatenate(x) for x in zip(*parts)], whole, "three uneven slabs")
    check("A", za, graph, in_k, degree, rev_k=8, first_row=cuts[2], n=n - cuts[2], prep=prep, what="the info describes the last call")
    gone = int(rc.removed_rows(n)[5])
    got, info, _ = check("A", za, graph, in_k, degree, rev_k=8, first_row=gone, n=1, prep=prep, what="a slab of one removed row")
    assert got[2][0] == 0 and info["lines"] == 0 and info["launches"] == 0 and info["keyed"] == 0
    got = ix.knn_graph_prune(graph, degree, m, first_row=100, n=0)
    assert got[0].shape == (0, degree) and got[2].shape == (0,)
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_prune(graph, degree, m, first_row=1000, n=501)
    assert e.value.code == EINVAL
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_prune(graph, 65, m)
    assert e.value.code == ELIMIT


def test_degree_zero_touches_the_counts_only(za):
    from zebra_amd import _ffi
    ix, X, live, base = table("A")
    n = X.shape[0]
    graph = rc.g_ring(n, 3, live, base)
    ids, keys, counts = np.full((n, 1), 77, np.uint64), np.full((n, 1), 78, np.uint64), np.full(n, 79, np.uint32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L = _ffi.lib()
    assert L.zh_knn_graph_prune(ix._h, P(graph[0]), P(graph[1]), 3, 0, 0, n + 1, 0, 0, 1, 0, P(ids), P(keys), P(counts)) == EINVAL  # the range comes first
    assert (counts == 79).all()
    assert L.zh_knn_graph_prune(ix._h, P(graph[0]), P(graph[1]), 3, 2, 0, n, 0, 1, 1, 0, None, None, P(counts)) == 0
    assert (counts == 0).all() and (ids == 77).all() and (keys == 78).all()
    info = ix.knn_prune_info()
    assert info == dict.fromkeys(pc.FIXED + ("keyed", "launches", "degree"), 0) | {"rows_live": int(live.sum()), "in_k": 3, "rev_k": 2, "fill": 1}


# ---------------------------------------------------------------- the sub-slab seam of prune_slab
def test_the_sub_slab_seam(za):
    """70 000 x 8 with seam_cases' group-local graph (groups of 97, the rows around 65 536 removed): two sub-slabs; the groups on both sides of
    65 536, and the first and last, against the reference on their 97-row sub-tables"""
    n, d, in_k, rev_k, degree = 70000, 8, 12, 4, 6
    pos = (sc.REFINE_SLAB,)
    tb = sc.Table(n, d, sc.ID_BASE, sc.removed(n, pos))
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 3), device=0, id_base=sc.ID_BASE, reserve_rows=n)
    try:
        ix.append_synthetic(n)
        gone = tb.gone.astype(np.uint64) + np.uint64(sc.ID_BASE)
        assert ix.remove(gone).size == gone.size
        ids, counts = sc.graph(n, in_k, sc.ID_BASE)
        seam = sc.seam_groups(n, pos)
        sc.adversarial(ids, counts, n, sc.ID_BASE, tb.live, seam)
        m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
        got = ix.knn_graph_prune((ids, counts), degree, m, reverse=rev_k)
        info = ix.knn_prune_info()
        assert info["launches"] == 2 == sc.sub_slabs(0, n, tb.live) and info["lines"] == int(tb.live.sum())
        groups = sorted(set(seam) | {seam[0] - 1, seam[-1] + 1, 0, sc.groups(n) - 1})
        assert any(tb.span(g)[0] < sc.REFINE_SLAB < tb.span(g)[1] for g in groups)  # a group straddles the seam
        for g in groups:
            s, e = tb.span(g)
            lg = tb.local(ids[s:e], counts[s:e], g)
            prep = pc.prepare(tb.rows(g), lg, in_k, rev_k, tb.live[s:e], 0, om, omode, row0=s)
            (rid, rkey, rcount), _ = pc.reference(prep, e - s, degree, 0, tb.live[s:e], 0)
            same(tuple(a[s:e] for a in got), (tb.rebase(rid, g), rkey, rcount), "group %d" % g)
        assert (got[2][~tb.live] == 0).all() and (got[0][~tb.live] == NONE).all()
        dev = sc.device_outputs(n, degree)
        import torch
        d_ids, d_counts = torch.from_numpy(ids.view(np.int64)).cuda(), torch.from_numpy(counts.view(np.int32)).cuda()
        torch.cuda.synchronize()
        ix.knn_graph_prune_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, degree, 0, m, 0, n, *[o.data_ptr() for o in dev])
        same(sc.host_arrays(dev), got, "device entry over the seam")
        assert ix.knn_prune_info() == info
    finally:
        ix.close()


# ---------------------------------------------------------------- entry twins and the caller's stream
def test_device_entry_on_a_callers_busy_stream(za):
    """The device entry agrees with the host entry, and it does so entered on a side stream that still has the uploads of its inputs and fills of
    its outputs pending behind a delay (the protocol of tests/test_gpu_caller_stream.py: stale but valid inputs and sentinel A in place, then on S a
    delay, the copies of the real graph, fills with sentinel B; S must be busy at the call and idle on return; the outputs are read through a third
    stream)."""
    import torch
    from tests.test_gpu_caller_stream import SENT_A, SENT_B, sentinel, u64
    ix, X, live, base = table("B")
    m = thirteen_metrics(za)[0][0]
    n, in_k, rev_k, degree, first_row, nl = X.shape[0], 32, 8, 16, 100, 1203
    graph = graph_of("B", "exact", in_k)
    host, hinfo, _ = check("B", za, graph, in_k, degree, fill=1, rev_k=rev_k, first_row=first_row, n=nl)
    dev = torch.device("cuda", 0)
    S, R = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    real_ids, real_counts = torch.from_numpy(graph[0].view(np.int64)).to(dev), torch.from_numpy(graph[1].view(np.int32)).to(dev)
    d_ids, d_counts = torch.zeros_like(real_ids), torch.zeros_like(real_counts)  # the stale input: a valid graph of empty lines
    out = [torch.empty((nl, degree), dtype=torch.int64, device=dev), torch.empty((nl, degree), dtype=torch.int64, device=dev),
           torch.empty(nl, dtype=torch.int32, device=dev)]
    call = lambda **kw: ix.knn_graph_prune_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, degree, 1, m, first_row, nl,  # noqa: E731
                                                  *[o.data_ptr() for o in out], **kw)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_ids.copy_(real_ids); d_counts.copy_(real_counts)
    torch.cuda.synchronize()
    call()
    same((u64(out[0].cpu().numpy()), u64(out[1].cpu().numpy()), out[2].cpu().numpy().view(np.uint32)), host, "device, idle")
    assert ix.knn_prune_info() == hinfo
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
    call(stream=S.cuda_stream)
    assert S.query()  # complete on return
    with torch.cuda.stream(R):
        got = [o.to("cpu", non_blocking=True) for o in out]
    R.synchronize()
    same((u64(got[0].numpy()), u64(got[1].numpy()), got[2].numpy().view(np.uint32)), host, "device, busy stream")
    assert ix.knn_prune_info() == hinfo


def test_idempotent_on_the_device(za):
    """1200 x 768: pruning the pruned graph at the same degree (fill = 0, no reverse neighbours) returns it, with nothing occluded and nothing cut"""
    ix, X, live, base = table("C")
    m = thirteen_metrics(za)[0][0]
    once, info, _ = check("C", za, graph_of("C", "exact", 32), 32, 16)
    assert info["occluded"] > 0
    again = ix.knn_graph_prune(once, 16, m)
    same(again, once, "pruned twice")
    info = ix.knn_prune_info()
    assert info["occluded"] == 0 and info["cut"] == 0 and info["kept"] == info["candidates"] == int(once[2].sum())


# ---------------------------------------------------------------- lifecycle
def test_rows_removed_appended_and_compacted_after_the_graph(za):
    ix, X, live, base = make("B13", za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        n, in_k, degree = X.shape[0], 16, 8
        K = keys_of("B13", 0)
        graph = pc.exact_graph(K, live, base, in_k)
        gone = rc.removed_rows(n)
        live = live.copy()
        live[gone] = False
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size

        def run(Xc, g, lv, what, K=None):
            got = ix.knn_graph_prune(g, degree, m, reverse=4)
            prep = pc.prepare(Xc, g, in_k, 4, lv, base, om, omode, K)
            ref, rinfo = pc.reference(prep, lv.size, degree, 0, lv, base)
            same(got, ref, what)
            info_is(ix, rinfo, prep, lv, in_k, 4, degree, 0, what=what)
            return got

        got = run(X, graph, live, "removed after", K)  # the graph still names the removed rows: ignored
        assert (got[2][gone] == 0).all()
        extra = zo.synth_rows(37, X.shape[1], seed=zo.SEED_ROWS + 9)
        ix.append(extra)
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_prune(graph, degree, m)
        assert e.value.code == EINVAL
        X2, live2 = np.concatenate([X, extra]), np.concatenate([live, np.ones(37, bool)])
        padded = (np.concatenate([graph[0], np.full((37, in_k), NONE, np.uint64)]), np.concatenate([graph[2], np.zeros(37, np.uint32)]))
        got = run(X2, padded, live2, "appended after")
        assert (got[2][n:] == 0).all()
        new_ids, _ = ix.compact()  # the caller re-keys the graph with the id map
        keep = np.flatnonzero(live2)
        rows = padded[0] - np.uint64(base)
        ok = rows < np.uint64(n + 37)
        rows[ok] = new_ids[rows[ok].astype(np.int64)]  # (a removed row's id becomes 2^64-1: ignored)
        rows[~ok] = NONE
        run(X2[keep], (rows[keep], padded[1][keep]), np.ones(keep.size, bool), "compacted")
    finally:
        ix.close()


def test_prune_graph_on_the_attached_graph_then_search(za):
    ix, X, live, base = make("A", za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        n, in_k, degree = X.shape[0], 32, 12
        graph = graph_of("A", "exact", in_k)
        ix.set_graph(graph)
        want = ix.knn_graph_prune(ix.get_graph(), degree, m, reverse=8)
        ginfo = ix.prune_graph(degree, m, reverse=8)
        assert ginfo["attached"] and ginfo["g_k"] == degree and ginfo["g_rows"] == n
        pruned = ix.get_graph()
        assert (pruned[1] == want[2]).all() and (pruned[0] == want[0]).all()
        Q = zo.synth_queries(24, X.shape[1], n)
        seeds = gc.default_seeds(24, 8, n, base)
        got = ix.search_graph_batch(Q, 5, m, beam=16, width=2, seeds=seeds)
        ref, rinfo = gc.reference(X, pruned, n, degree, live, base, Q, seeds, 5, 16, 2, 0, om, omode)
        same(got, ref, "the walk over the pruned table")
        assert ix.search_graph_info()["keyed"] == rinfo["keyed"]
    finally:
        ix.close()


def test_database_build_graph(za):
    """prune = 0 is the call as it was: forest graph, descent, attach -- held by equality of get_graph(); prune > 0 puts knn_graph_prune between"""
    X = rows_of("F")[:600]
    db = za.Database(X.shape[1], za.L2SquaredDistance(), za.LSHIndexOptions(64, 3), device=0)
    try:
        db.insert_records(X, ["doc%d" % i for i in range(X.shape[0])])
        ix = db.index
        forest = ix.knn_graph_forest(12, db.metric)
        descent = ix.knn_graph_descent(forest, 12, db.metric, rounds=3, reverse=4)
        ix.set_graph(descent)
        before = ix.get_graph()
        for kw in ({}, {"prune": 0}, {"prune": 0, "prune_reverse": 8, "fill": True}):
            info = db.build_graph(k=12, rounds=3, reverse=4, **kw)
            after = ix.get_graph()
            assert info["g_k"] == 12 and (after[0] == before[0]).all() and (after[1] == before[1]).all(), kw
        want = ix.knn_graph_prune(descent, 6, db.metric, reverse=8, fill=True)
        info = db.build_graph(k=12, rounds=3, reverse=4, prune=6, prune_reverse=8, fill=True)
        after = ix.get_graph()
        assert info["g_k"] == 6 and (after[0] == want[0]).all() and (after[1] == want[2]).all()
        assert ix.knn_prune_info()["degree"] == 6 and ix.knn_prune_info()["occluded"] > 0
    finally:
        db.index.close()

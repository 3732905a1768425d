"""NN-descent on the device (zh_knn_graph_descent): incremental rounds to a fixed point.  The answer is bit for bit the loop's --
LSHIndex.knn_graph_refine(rounds=, reverse=) on the same index -- and the numpy reference's (tests/descent_cases.py, pinned on the CPU by
tests/test_descent_reference.py); the info's per-round figures are the incremental definition's.  Tables are tests/test_gpu_refine.py's: 1500 x 30
(the generic row loop, removed rows, id_base 1000), 1500 x 256 and 1200 x 768 (specialised loads; id_base 7 and the block of identical rows),
and a built 1500 x 256 index for the forest graph."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import descent_cases as dc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests import reverse_cases as rv  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_refine import keys_of, rows_of, same  # noqa: E402
from tests.test_gpu_reverse import make  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ELIMIT = -1, -5
CASE_TABLE = {1: "B", 2: "A", 3: "C", 4: "A"}  # L2 squared at 256 and 768: the specialised loads; Manhattan and the ring at 30: the generic loop


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


def table(name):
    import zebra_amd
    if name not in _SHARED:
        _SHARED[name] = make(name, zebra_amd)
    return _SHARED[name]


def loop(ix, graph, k, m, rounds, rev):
    """the existing loop, round by round on the host -> (answer, [the info of every round run])"""
    infos = []
    g = graph
    for _ in range(rounds):
        g = ix.knn_graph_refine(g, k, m, reverse=rev)
        infos.append(ix.knn_refine_rev_info() if rev else ix.knn_refine_info())
        if infos[-1]["updates"] == 0:
            break
    return g, infos


def info_is(ix, ref, live, in_k, rev_k, k, rounds, what=""):
    info = ix.knn_descent_info()
    want = {"rows_live": int(live.sum()), "in_k": in_k, "rev_k": rev_k, "k": k, "rounds": rounds, "rounds_run": ref["rounds_run"],
            "listed": sum(ref["listed_round"]), "keyed": sum(ref["keyed_round"]), "lines_active": sum(ref["active_round"]),
            "updates": ref["updates_round"][-1], "keyed_round": ref["keyed_round"], "updates_round": ref["updates_round"],
            "active_round": ref["active_round"]}
    got = {f: info[f] for f in want}
    assert got == want, (what, got, want)
    assert info["launches"] > 0
    return info


def check(name, za, graph, in_k, rev_k, k, rounds, mi=0, what=""):
    """one host call on a shared table against the loop on the same index and against the numpy reference, info included"""
    ix, X, live, base = table(name)
    m, om, omode = thirteen_metrics(za)[mi]
    got = ix.knn_graph_descent(graph, k, m, rounds=rounds, reverse=rev_k)
    info = ix.knn_descent_info()
    same(got, ix.knn_graph_refine(graph, k, m, rounds=rounds, reverse=rev_k), what + " (the loop)")
    _, infos = loop(ix, graph, k, m, rounds, rev_k)
    ref, rinfo, _, _ = dc.descent(X, graph, in_k, rev_k, k, rounds, live, base, om, omode, keys_of(name, mi))
    same(got, ref, what + " (numpy)")
    assert ix.knn_descent_info() == info  # (the loop's calls leave the descent's info alone)
    info_is(ix, rinfo, live, in_k, rev_k, k, rounds, what)
    assert len(infos) == info["rounds_run"] and info["keyed_round"][0] == infos[0]["keyed"]
    assert [i["updates"] for i in infos] == info["updates_round"]
    assert [i["keyed"] for i in infos] == rinfo["full_keyed_round"]
    inactive = [r for r in range(info["rounds_run"]) if info["active_round"][r] < info["rows_live"]]
    for r in range(inactive[0] if inactive else info["rounds_run"], info["rounds_run"]):
        assert info["keyed_round"][r] < infos[r]["keyed"], (what, r)
    return got, info


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("number", sorted(dc.CASES))
def test_the_four_cases(za, number):
    name = CASE_TABLE[number]
    _, X, live, base = table(name)
    n, gname, mi, in_k, k, rev_k = dc.CASES[number]
    assert X.shape[0] == n
    graph = rv.ALL_GRAPHS[gname](n, in_k, live, base)
    _, info = check(name, za, graph, in_k, rev_k, k, 12, mi, "case %d" % number)
    assert min(info["active_round"]) < info["rows_live"]  # (a round with inactive lines)
    if number == 3:  # width 64: early rounds in the large instantiation, late ones in the small
        assert 0 < info["large_lines"] < info["lines_active"] + info["rows_live"]
        assert info["large_lines"] > info["rows_live"]  # (round 1 alone is every live line)
    if number in (1, 4):
        assert info["large_lines"] == 0
    if number == 4:
        assert info["rounds_run"] == 12 and info["updates"] > 0  # the rounds limit ends the call


@pytest.mark.parametrize("rev_k", [0, 4])
def test_forest_graph(za, rev_k):
    """the forest graph of a built index (max_node_size 64, 3 trees), in_k = k = 8"""
    ix, X, live, base = table("F")
    m = thirteen_metrics(za)[0][0]
    check("F", za, ix.knn_graph_forest(8, m), 8, rev_k, 8, 8, what="forest, reverse %d" % rev_k)


@pytest.mark.parametrize("mi", range(13))
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_metric(za, name, mi):
    ix, X, live, base = table(name)
    m = thirteen_metrics(za)[mi][0]
    graph = rv.g_orphan(X.shape[0], 5, live, base)
    for rev_k in (0, 3):
        got = ix.knn_graph_descent(graph, 7, m, rounds=4, reverse=rev_k)
        info = ix.knn_descent_info()
        want, infos = loop(ix, graph, 7, m, 4, rev_k)
        same(got, want, "%s metric %d reverse %d" % (name, mi, rev_k))
        assert info["updates_round"] == [i["updates"] for i in infos] and info["keyed_round"][0] == infos[0]["keyed"]
        assert all(a <= i["keyed"] for a, i in zip(info["keyed_round"], infos))


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("name,graph,in_k,rev_k", [("A", "hub", 5, 0), ("A", "hub", 5, 8), ("C", "block", 32, 0), ("C", "orphan", 45, 19)])
def test_one_round_is_the_refinement(za, name, graph, in_k, rev_k):
    ix, X, live, base = table(name)
    m = thirteen_metrics(za)[0][0]
    g = rv.ALL_GRAPHS[graph](X.shape[0], in_k, live, base)
    got = ix.knn_graph_descent(g, 9, m, rounds=1, reverse=rev_k)
    info = ix.knn_descent_info()
    same(got, ix.knn_graph_refine(g, 9, m, reverse=rev_k), "rounds = 1")
    one = ix.knn_refine_rev_info() if rev_k else ix.knn_refine_info()
    assert info["rounds_run"] == 1 and info["keyed_round"] == [one["keyed"]] and info["updates_round"] == [one["updates"]]
    assert info["listed"] == one["listed"] and info["active_round"] == [int(live.sum())]
    assert info["large_lines"] == (int(live.sum()) if in_k + rev_k > 44 else 0)


def test_refining_the_exact_graph_returns_it(za):
    ix, X, live, base = table("B")
    m = thirteen_metrics(za)[0][0]
    exact = ix.knn_graph(12, m)
    for k, rev_k in ((12, 0), (12, 8), (5, 3)):
        got = ix.knn_graph_descent(exact, k, m, rounds=6, reverse=rev_k)
        same(got, (exact[0][:, :k], exact[1][:, :k], np.minimum(exact[2], k).astype(np.uint32)), "k %d" % k)
        info = ix.knn_descent_info()
        assert info["rounds_run"] == 1 and info["updates"] == 0 and info["rounds"] == 6


def test_complete_graph_is_a_fixed_point(za):
    """60 rows, every line lists the other 59"""
    ix, X, live, base = table("tiny")
    m = thirteen_metrics(za)[0][0]
    n = X.shape[0]
    complete = ix.knn_graph(n - 1, m)
    for k in (n - 1, 10):
        same(ix.knn_graph_descent(complete, k, m, rounds=5), ix.knn_graph(k, m), "k %d" % k)
        info = ix.knn_descent_info()
        assert info["rounds_run"] == 1 and info["updates"] == 0 and info["keyed"] == n * (n - 1)
    # a ring is not: it takes rounds, and the call runs them
    ring = rc.g_ring(n, 1, live, base)
    got = ix.knn_graph_descent(ring, 2, m, rounds=32)
    info = ix.knn_descent_info()
    want, infos = loop(ix, ring, 2, m, 32, 0)
    same(got, want, "ring")
    assert info["rounds_run"] == len(infos) > 1 and info["updates_round"] == [i["updates"] for i in infos]


@pytest.mark.parametrize("k", [5, 32, 40])
@pytest.mark.parametrize("graph", ["out_of_range", "all_ones", "zero_counts", "self_loops"])
def test_adversarial_inputs(za, graph, k):
    """in_k = 32, k below, at and above it; 1500 x 30, id_base 1000, removed rows"""
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    g = rc.GRAPHS[graph](X.shape[0], 32, live, base)
    for rev_k in (0, 5):
        got = ix.knn_graph_descent(g, k, m, rounds=3, reverse=rev_k)
        info = ix.knn_descent_info()
        want, infos = loop(ix, g, k, m, 3, rev_k)
        same(got, want, "%s k %d reverse %d" % (graph, k, rev_k))
        assert info["updates_round"] == [i["updates"] for i in infos]
        assert (got[2][~live] == 0).all() and (got[0][~live] == NONE).all() and (got[1][~live] == NONE).all()


def test_limits_and_shapes(za):
    ix, X, live, base = table("A")
    m = thirteen_metrics(za)[0][0]
    n = X.shape[0]
    g = rc.g_ring(n, 8, live, base)
    for kwargs, code in (({"rounds": 0}, EINVAL), ({"rounds": 33}, EINVAL), ({"reverse": 57}, ELIMIT)):
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_descent(g, 8, m, **kwargs)
        assert e.value.code == code, kwargs
    for k, code in ((0, EINVAL), (65, ELIMIT)):
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_descent(g, k, m)
        assert e.value.code == code, k
    with pytest.raises(za.ZhError) as e:
        ix.knn_graph_descent((g[0][:100], g[1][:100]), 8, m)
    assert e.value.code == EINVAL
    empty = za.LSHIndex(30, za.LSHIndexOptions(64, 3), device=0)
    try:
        got = empty.knn_graph_descent((np.zeros((0, 8), np.uint64), np.zeros(0, np.uint32)), 8, m)
        assert got[0].shape == (0, 8) and got[2].shape == (0,)
    finally:
        empty.close()


def test_rows_removed_appended_and_compacted_between_calls(za):
    from oracle import zebra_oracle as zo
    ix, X, live, base = make("F", za)
    try:
        m = thirteen_metrics(za)[0][0]
        n, k, rev_k, rounds = X.shape[0], 8, 4, 5
        graph = ix.knn_graph_forest(k, m)
        first = ix.knn_graph_descent(graph, k, m, rounds=rounds, reverse=rev_k)
        same(first, loop(ix, graph, k, m, rounds, rev_k)[0], "before")
        gone = rc.removed_rows(n)
        assert ix.remove(gone.astype(np.uint64)).size == gone.size
        got = ix.knn_graph_descent(first, k, m, rounds=rounds, reverse=rev_k)  # the graph still names the removed rows: ignored
        same(got, loop(ix, first, k, m, rounds, rev_k)[0], "removed after")
        assert (got[2][gone] == 0).all() and ix.knn_descent_info()["rows_live"] == n - gone.size
        ix.append(zo.synth_rows(37, X.shape[1], seed=zo.SEED_ROWS + 9))
        with pytest.raises(za.ZhError) as e:
            ix.knn_graph_descent(got, k, m)
        assert e.value.code == EINVAL
        padded = (np.concatenate([got[0], np.full((37, k), NONE, np.uint64)]), np.concatenate([got[2], np.zeros(37, np.uint32)]))
        again = ix.knn_graph_descent(padded, k, m, rounds=rounds, reverse=rev_k)
        same(again, loop(ix, padded, k, m, rounds, rev_k)[0], "appended after")
        new_ids, _ = ix.compact()
        keep = np.flatnonzero(new_ids != NONE)
        rows = again[0].copy()
        ok = rows < np.uint64(n + 37)
        rows[ok] = new_ids[rows[ok].astype(np.int64)]
        rekeyed = (rows[keep], again[2][keep])
        last = ix.knn_graph_descent(rekeyed, k, m, rounds=rounds, reverse=rev_k)
        same(last, loop(ix, rekeyed, k, m, rounds, rev_k)[0], "compacted")
        assert ix.knn_descent_info()["rows_live"] == keep.size
    finally:
        ix.close()


# ---------------------------------------------------------------- the device entry and the caller's stream
def test_device_entry_on_a_callers_busy_stream(za):
    """tests/test_gpu_refine.py's protocol: stale but valid inputs and sentinel A in place, then on S a delay, the copies of the real graph, fills
    with sentinel B; S must be busy at the call and idle on return; the outputs are read through a third stream"""
    import torch
    from tests.test_gpu_caller_stream import SENT_A, SENT_B, sentinel, u64
    ix, X, live, base = table("B")
    m = thirteen_metrics(za)[0][0]
    n, in_k, rev_k, k, rounds = X.shape[0], 32, 4, 10, 4
    graph = rc.g_block(n, in_k, live, base)
    host = ix.knn_graph_descent(graph, k, m, rounds=rounds, reverse=rev_k)
    hinfo = ix.knn_descent_info()
    same(host, ix.knn_graph_refine(graph, k, m, rounds=rounds, reverse=rev_k), "host")
    dev = torch.device("cuda", 0)
    S, R = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    real_ids, real_counts = torch.from_numpy(graph[0].view(np.int64)).to(dev), torch.from_numpy(graph[1].view(np.int32)).to(dev)
    d_ids, d_counts = torch.zeros_like(real_ids), torch.zeros_like(real_counts)  # the stale input: a valid graph of empty lines
    out = [torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev)]
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_ids.copy_(real_ids); d_counts.copy_(real_counts)
    torch.cuda.synchronize()
    ix.knn_graph_descent_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, k, rounds, m, *[o.data_ptr() for o in out])
    same((u64(out[0].cpu().numpy()), u64(out[1].cpu().numpy()), out[2].cpu().numpy().view(np.uint32)), host, "device, idle")
    dinfo = ix.knn_descent_info()
    assert {f: v for f, v in dinfo.items() if f != "launches"} == {f: v for f, v in hinfo.items() if f != "launches"}
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
    ix.knn_graph_descent_device(d_ids.data_ptr(), d_counts.data_ptr(), in_k, rev_k, k, rounds, m, *[o.data_ptr() for o in out], stream=S.cuda_stream)
    assert S.query()  # complete on return
    with torch.cuda.stream(R):
        got = [o.to("cpu", non_blocking=True) for o in out]
    R.synchronize()
    same((u64(got[0].numpy()), u64(got[1].numpy()), got[2].numpy().view(np.uint32)), host, "device, busy stream")
    assert ix.knn_descent_info() == dinfo


# ---------------------------------------------------------------- the database
def test_database_descent(za):
    X = rows_of("F")[:600]
    db = za.Database(X.shape[1], za.L2SquaredDistance(), za.LSHIndexOptions(64, 3), device=0)
    try:
        docs = ["doc%d" % i for i in range(X.shape[0])]
        db.insert_records(X, docs)
        for rev_k in (0, 4):
            got = db.knn_graph_descent(6, rounds=5, reverse=rev_k)
            assert got == db.knn_graph_refined(6, 5, reverse=rev_k) and set(got) == set(docs)
            assert db.index.knn_descent_info()["rounds_run"] >= 2
    finally:
        db.index.close()

"""Graph search on the device (zh_index_set_graph, zh_search_graph_batch): ids, keys, counts and every info field equal the numpy reference
(tests/gsearch_cases.py, pinned on the CPU by tests/test_gsearch_reference.py), and the host and `_device` entries agree bit for bit.

Tables are gsearch_cases': 1500 x 30 and 600 x 30 (the generic row loop), 600 x 128 (a specialised load for every kind), 600 x 256 (specialised for
L2 / cosine only), each with rc.removed_rows removed and the block of 40 identical rows; id_base 0 on two of them and 2^40 + 3 on the other two.
Every shared index is appended, never built; the lifecycle tests make their own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gsearch_cases as gc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ESTATE, ELIMIT = -1, -4, -5
BIG = 2**40 + 3
BASES = {"t1500": 0, "t600": BIG, "t600x128": 0, "t600x256": BIG}


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


_SHARED = {}    # table name -> (index, X, live, id_base); no test changes the rows of one
_ATTACHED = {}  # table name -> (graph name, g_k) attached now


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()
    _ATTACHED.clear()


def make(za, X, live, base, trees=False):
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 3), device=0, id_base=base)
    (ix.add if trees else ix.append)(X)
    gone = np.flatnonzero(~live)
    if gone.size:
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
    return ix


def index(tname):
    import zebra_amd
    if tname not in _SHARED:
        X, live = gc.table(tname)
        _SHARED[tname] = (make(zebra_amd, X, live, BASES[tname]), X, live, BASES[tname])
    return _SHARED[tname]


def attach(tname, gname, g_k):
    ix, X, live, base = index(tname)
    g = gc.graph(tname, gname, g_k, base)
    if _ATTACHED.get(tname) != (gname, g_k):
        ix.set_graph(g)
        _ATTACHED[tname] = (gname, g_k)
        assert ix.graph_info() == {"attached": 1, "g_k": g_k, "g_rows": X.shape[0], "bytes": ix.graph_info()["bytes"]}
        assert ix.graph_info()["bytes"] >= 4 * X.shape[0] * g_k
    return g


def rand_seeds(tname, b, n_seed, salt=0):
    """per query n_seed stored rows drawn with replacement (some removed, now and then one twice), as ids"""
    n = gc.TABLES[tname][0]
    rng = np.random.default_rng([0x65EED, n, b, n_seed, salt])
    return rng.integers(0, n, (b, n_seed)).astype(np.uint64) + np.uint64(BASES[tname])


def device_call(ix, Q, seeds, top_k, m, beam, width, max_iters, stream=None):
    import torch
    b = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    sd = torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()
    ids = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    keys = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_graph_batch_device(q.data_ptr(), b, sd.data_ptr(), seeds.shape[1], top_k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr(), beam=beam,
                                 width=width, max_iters=max_iters, stream=stream)
    return ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def check(za, tname, gname, g_k, Q, seeds, top_k, beam, width, max_iters=0, mi=0, what=""):
    """one host call and one device call on a shared table against the reference, info included -> (answer, info)"""
    ix, X, live, base = index(tname)
    g = attach(tname, gname, g_k)
    m, om, omode = thirteen_metrics(za)[mi]
    got = ix.search_graph_batch(Q, top_k, m, beam=beam, width=width, max_iters=max_iters, seeds=seeds)
    info = ix.search_graph_info()
    ref, rinfo = gc.reference(X, g, X.shape[0], g_k, live, base, Q, seeds, top_k, beam, width, max_iters, om, omode)
    same(got, ref, what)
    assert info == rinfo, (what, info, rinfo)
    dev = device_call(ix, Q, seeds, top_k, m, beam, width, max_iters)
    same(dev, got, what + " (device entry)")
    assert ix.search_graph_info() == rinfo, what
    return got, info


# ---------------------------------------------------------------- the definition, limit by limit
@pytest.mark.parametrize("g_k,width", [(1, 1), (1, 2), (1, 256), (5, 1), (5, 2), (5, 51), (32, 1), (32, 2), (32, 8), (64, 1), (64, 2), (64, 4)])
def test_line_widths_and_expansion_widths(za, g_k, width):
    """g_k 1, 5, 32, 64 at width 1, 2 and the widest the 256 candidate slots allow (32 x 8 and 64 x 4 fill them exactly)"""
    Q = gc.queries("t600", 5)
    _, info = check(za, "t600", "exact", g_k, Q, rand_seeds("t600", 5, 8, g_k), 10, 64, width, what="g_k %d width %d" % (g_k, width))
    assert info["expanded"] >= info["iterations"] > 0


def test_a_width_past_the_candidate_slots_is_refused(za):
    ix, _, _, _ = index("t600")
    m = thirteen_metrics(za)[0][0]
    Q, seeds = gc.queries("t600", 2), rand_seeds("t600", 2, 8)
    for g_k, width in ((32, 9), (64, 5), (5, 52), (1, 257)):
        attach("t600", "exact", g_k)
        before = ix.search_graph_info()
        with pytest.raises(za.ZhError) as e:
            ix.search_graph_batch(Q, 4, m, beam=8, width=width, seeds=seeds)
        assert e.value.code == ELIMIT and "width" in str(e.value), (g_k, width)
        assert ix.search_graph_info() == before


@pytest.mark.parametrize("beam", [1, 2, 33, 64, 255, 256])
def test_beams(za, beam):
    Q = gc.queries("t600", 5)
    seeds = rand_seeds("t600", 5, 8, beam)
    check(za, "t600", "exact", 32, Q, seeds, beam, beam, 1, what="top_k = beam = %d" % beam)
    check(za, "t600", "exact", 32, Q, seeds, max(1, beam // 3), beam, 2, what="top_k < beam = %d" % beam)


@pytest.mark.parametrize("n_seed", [1, 8, 64])
def test_seed_counts(za, n_seed):
    Q = gc.queries("t1500", 5)
    _, info = check(za, "t1500", "exact", 32, Q, rand_seeds("t1500", 5, n_seed), 10, 64, 1, what="n_seed %d" % n_seed)
    assert 0 < info["seeds"] <= 5 * n_seed


@pytest.mark.parametrize("b", [1, 5, 257])
def test_batch_sizes(za, b):
    """257 queries: more than one block per CU's worth, an odd count"""
    Q = gc.queries("t600", b)
    check(za, "t600", "exact", 5, Q, rand_seeds("t600", b, 8), 8, 8, 2, what="b %d" % b)


def test_an_empty_batch_is_ok(za):
    ix, _, _, _ = index("t600")
    attach("t600", "exact", 5)
    before = ix.search_graph_info()
    ids, keys, counts = ix.search_graph_batch(np.zeros((0, 30), np.float32), 4, thirteen_metrics(za)[0][0], beam=8, seeds=np.zeros((0, 3), np.uint64))
    assert ids.shape == (0, 4) and counts.shape == (0,) and ix.search_graph_info() == before


def test_seeds_that_name_nothing(za):
    """repeated, removed, below id_base, at id_base + stored rows, 2^64-1; a query whose seeds are all invalid has count 0 and all-ones tails"""
    ix, X, live, base = index("t600")
    n = X.shape[0]
    dead = np.flatnonzero(~live)
    alive = np.flatnonzero(live)
    Q = gc.queries("t600", 6)
    rows = [[base + alive[5]] * 8,                                                   # the same row eight times
            [base + dead[0], base + alive[9], base + dead[1], base + alive[9], base - 1, base + n, 2**64 - 1, base + alive[10]],
            [base + dead[j] for j in range(8)],                                      # all removed
            [base - 1, base - 2, 0, 1, base // 2, base - 100, 5, 7],                 # all below id_base
            [base + n, base + n + 1, 2**64 - 1, 2**63, base + 2**32, base + n, 2**64 - 2, base + n + 7],  # all past the table
            [base + alive[-1], base + alive[0], base + alive[-1], base + n, base + dead[2], 2**64 - 1, base + alive[0], base + alive[77]]]
    seeds = np.array([[int(v) for v in row] for row in rows], np.uint64)
    (ids, keys, counts), info = check(za, "t600", "exact", 32, Q, seeds, 10, 33, 2, what="seeds")
    assert (counts[2:5] == 0).all() and (ids[2:5] == NONE).all() and (keys[2:5] == NONE).all()
    assert counts[0] == 10 and info["seeds"] == 1 + 2 + 0 + 0 + 0 + 3
    check(za, "t600", "zero_counts", 32, Q[:1], seeds[:1], 33, 33, 1, what="one seed, maybe an empty line")


# ---------------------------------------------------------------- the graphs
@pytest.mark.parametrize("gname", sorted(rc.GRAPHS))
def test_every_graph(za, gname):
    """self_loops: a parent's own line names it; block: equal keys, ties between expanded and unexpanded entries resolved by id; removed, all_ones,
    zero_counts: masked entries and empty lines"""
    Q = gc.queries("t600", 8)
    if gname == "block":
        Q = Q.copy()
        Q[:4] = gc.table("t600")[0][rc.BLOCK[0]]  # (queries AT the block: forty equal keys at the head of the beam)
    seeds = rand_seeds("t600", 8, 8, sum(gname.encode()))
    if gname == "block":
        seeds[:, 0] = BIG + rc.BLOCK[0] + 5
    check(za, "t600", gname, 32, Q, seeds, 33, 64, 2, what=gname)
    check(za, "t600", gname, 32, Q[:3], seeds[:3], 256, 256, 8, what=gname + ", every slot")


@pytest.mark.parametrize("max_iters,iters,capped", [(1, 1, 1), (3, 3, 1), (0, None, 0)])
def test_ring_and_the_iteration_cap(za, max_iters, iters, capped):
    """g_k = 1, one live seed, beam 8: every iteration expands one row and keys at most one.  Capped after 1 and 3 iterations with an unexpanded
    entry left; uncapped the walk ends when the beam's entries are all expanded"""
    ix, X, live, base = index("t600")
    Q = gc.queries("t600", 4)
    rows = np.array([4, 53, 200, 404])  # (each and the four rows after it are live: the walk has a next row to key in every iteration run here)
    assert all(live[r:r + 5].all() for r in rows)
    seeds = (rows.astype(np.uint64) + np.uint64(base)).reshape(4, 1)
    _, info = check(za, "t600", "ring", 1, Q, seeds, 8, 8, 1, max_iters=max_iters, what="ring, max_iters %d" % max_iters)
    assert info["capped"] == 4 * capped and info["seeds"] == 4
    if iters is not None:
        assert info["iterations"] == 4 * iters and info["expanded"] == 4 * iters
    else:
        assert info["iterations"] > 4 * 3


def test_the_largest_iteration_cap(za):
    ix, _, _, _ = index("t600")
    attach("t600", "ring", 1)
    m = thirteen_metrics(za)[0][0]
    Q, seeds = gc.queries("t600", 1), rand_seeds("t600", 1, 8)
    a = ix.search_graph_batch(Q, 8, m, beam=8, max_iters=65535, seeds=seeds)
    same(a, ix.search_graph_batch(Q, 8, m, beam=8, max_iters=0, seeds=seeds), "a cap never reached")
    with pytest.raises(za.ZhError) as e:
        ix.search_graph_batch(Q, 8, m, beam=8, max_iters=65536, seeds=seeds)
    assert e.value.code == ELIMIT


# ---------------------------------------------------------------- small tables of their own
@pytest.fixture(scope="module")
def small(za):
    """200 x 30, every row live, id_base 7"""
    X = rc.table(200, 30)
    live = np.ones(200, bool)
    ix = make(za, X, live, 7)
    yield ix, X, live, 7
    ix.close()


def test_a_beam_larger_than_the_reachable_set(za, small):
    """the ring on 200 live rows, beam 256: every row is reached, the count is 200 < top_k, the tails all ones"""
    ix, X, live, base = small
    g = rc.g_ring(200, 1, live, base)
    ix.set_graph(g)
    m, om, omode = thirteen_metrics(za)[0]
    Q = zo.synth_queries(3, 30, 200)
    seeds = np.array([[base + 0], [base + 120], [base + 199]], np.uint64)
    got = ix.search_graph_batch(Q, 256, m, beam=256, seeds=seeds)
    ref, rinfo = gc.reference(X, g, 200, 1, live, base, Q, seeds, 256, 256, 1, 0, om, omode)
    same(got, ref, "ring 200")
    assert ix.search_graph_info() == rinfo and rinfo["iterations"] == 3 * 200 and rinfo["keyed"] == 3 * 200
    assert (got[2] == 200).all() and (got[0][:, 200:] == NONE).all() and (got[1][:, 200:] == NONE).all()
    same(got, ix.search_exact_batch(Q, 256, m), "every row reached: the exact answer")


def test_the_exact_graph_reaches_what_the_reference_says(za, small):
    """the exact 16-NN graph, beam 256 >= the table: nothing ever leaves the beam, so the answer is the exact top-k among the rows that ever got a
    key (search_exact_filtered_batch under that filter), and the exact top-k outright where that is every row"""
    ix, X, live, base = small
    m, om, omode = thirteen_metrics(za)[0]
    g = gc.exact_graph(X, 16, live, base, om, omode)
    ix.set_graph(g)
    Q = zo.synth_queries(3, 30, 200)
    seeds = np.array([[base + 3], [base + 77], [base + 150]], np.uint64)
    got = ix.search_graph_batch(Q, 50, m, beam=256, seeds=seeds)
    trace = []
    ref, _ = gc.reference(X, g, 200, 16, live, base, Q, seeds, 50, 256, 1, 0, om, omode, trace=trace)
    same(got, ref, "exact 16-NN graph")
    for b in range(3):
        allowed = np.array(sorted(trace[b]), np.uint64) + np.uint64(base)
        want = ix.search_exact_filtered_batch(Q[b:b + 1], 50, m, allowed)
        same(tuple(a[b:b + 1] for a in got), want, "the closure's exact top-k, query %d" % b)
        if len(trace[b]) == 200:
            same(tuple(a[b:b + 1] for a in got), ix.search_exact_batch(Q[b:b + 1], 50, m), "every row keyed: the exact top-k")
    assert max(len(t) for t in trace) > 100


def test_the_complete_graph_is_the_exact_search(za):
    """65 live rows, every line names the 64 others, one valid seed, beam >= the live rows: the first iteration keys everything"""
    X = rc.table(65, 128, False)
    live = np.ones(65, bool)
    ix = make(za, X, live, 11)
    try:
        ids = np.array([[r for r in range(65) if r != a] for a in range(65)], np.uint64) + np.uint64(11)
        ix.set_graph((ids, np.full(65, 64, np.uint32)))
        Q = zo.synth_queries(7, 128, 65)
        for mi in (0, 2, 7):
            m = thirteen_metrics(za)[mi][0]
            seeds = (np.arange(7, dtype=np.uint64) * 9 + 11).reshape(7, 1)
            for beam in (65, 256):
                got = ix.search_graph_batch(Q, 65, m, beam=beam, width=4, seeds=seeds)
                same(got, ix.search_exact_batch(Q, 65, m), "complete graph, metric %d, beam %d" % (mi, beam))
            info = ix.search_graph_info()
            assert info["keyed"] == 7 * 65 and info["seeds"] == 7 and info["expanded"] == 7 * 65
    finally:
        ix.close()


# ---------------------------------------------------------------- every key
@pytest.mark.parametrize("mi", range(13))
def test_every_metric_at_128(za, mi):
    Q = gc.queries("t600x128", 5)
    check(za, "t600x128", "exact", 32, Q, rand_seeds("t600x128", 5, 8, mi), 10, 33, 2, mi=mi, what="metric %d, d 128" % mi)


@pytest.mark.parametrize("mi", [0, 1, 2, 3, 7])
def test_l2_and_cosine_at_256(za, mi):
    """L2 squared, L2 and both cosine modes take the specialised load at 256; Manhattan the generic loop"""
    Q = gc.queries("t600x256", 5)
    check(za, "t600x256", "exact", 32, Q, rand_seeds("t600x256", 5, 8, mi), 10, 33, 2, mi=mi, what="metric %d, d 256" % mi)


# ---------------------------------------------------------------- lifecycle
def fresh(za, base=BIG):
    X, live = gc.table("t600")
    return make(za, X, live, base, trees=True), X, live.copy(), base


def estate(za, call):
    with pytest.raises(za.ZhError) as e:
        call()
    assert e.value.code == ESTATE, e.value


def test_remove_after_the_attach_needs_no_reattach(za):
    ix, X, live, base = fresh(za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        g = gc.graph("t600", "exact", 32, base)
        ix.set_graph(g)
        Q, seeds = gc.queries("t600", 5), rand_seeds("t600", 5, 8, 1)
        before = ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds)
        gone = np.unique(np.concatenate([(before[0][:, :3].reshape(-1) - np.uint64(base)).astype(np.int64), np.arange(10, 600, 11)]))
        gone = gone[live[gone]]
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
        live[gone] = False
        got = ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds)
        ref, rinfo = gc.reference(X, g, 600, 32, live, base, Q, seeds, 10, 33, 2, 0, om, omode)
        same(got, ref, "after remove")
        assert ix.search_graph_info() == rinfo
        assert not np.isin(got[0][got[0] != NONE] - np.uint64(base), gone.astype(np.uint64)).any()
    finally:
        ix.close()


def test_append_after_the_attach(za):
    """a seed on an appended row: found, ranked, never expanded into anything (its line is empty); entries naming rows past the table AT THE ATTACH
    stay masked"""
    ix, X, live, base = fresh(za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        g = [a.copy() for a in gc.graph("t600", "exact", 5, base)]
        g[0][::3, 0] = base + 603  # (out of range at the attach, a stored row after the append)
        ix.set_graph(g)
        Q = gc.queries("t600", 4)
        extra = np.concatenate([Q[:2], zo.synth_rows(6, 30, row0=9000)])  # (two appended rows ARE queries: key 0)
        ix.append(extra)
        X2, live2 = np.concatenate([X, extra]), np.concatenate([live, np.ones(8, bool)])
        seeds = np.array([[base + 600, base + 20], [base + 601, base + 607], [base + 603, base + 603], [base + 30, base + 608]], np.uint64)
        got = ix.search_graph_batch(Q, 8, m, beam=8, seeds=seeds)
        ref, rinfo = gc.reference(X2, g, 600, 5, live2, base, Q, seeds, 8, 8, 1, 0, om, omode, attach_rows=600)
        same(got, ref, "after append")
        assert ix.search_graph_info() == rinfo
        assert got[0][0, 0] == base + 600 and got[0][1, 0] == base + 601 and got[2][1] == 2 and got[2][2] == 1
        assert ix.graph_info()["g_rows"] == 600
    finally:
        ix.close()


def test_a_graph_over_the_first_rows_and_a_second_attach(za):
    ix, X, live, base = fresh(za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        g = gc.graph("t600", "exact", 32, base)
        Q, seeds = gc.queries("t600", 4), rand_seeds("t600", 4, 8, 2)
        ix.set_graph(g, rows=250)
        assert ix.graph_info()["g_rows"] == 250 and ix.graph_info()["g_k"] == 32
        got = ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds)
        ref, rinfo = gc.reference(X, g, 250, 32, live, base, Q, seeds, 10, 33, 1, 0, om, omode)
        same(got, ref, "g_rows 250")
        assert ix.search_graph_info() == rinfo
        g2 = gc.graph("t600", "ring", 5, base)
        ix.set_graph(g2)
        assert ix.graph_info()["g_rows"] == 600 and ix.graph_info()["g_k"] == 5
        got = ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds)
        same(got, gc.reference(X, g2, 600, 5, live, base, Q, seeds, 10, 33, 1, 0, om, omode)[0], "the second graph")
        with pytest.raises(za.ZhError) as e:
            ix.set_graph((np.zeros((601, 4), np.uint64), np.zeros(601, np.uint32)))
        assert e.value.code == EINVAL and ix.graph_info()["g_k"] == 5  # (a refused attach leaves what was attached)
    finally:
        ix.close()


def test_the_three_ways_to_attach_agree(za, monkeypatch):
    """the host entry in one chunk, in chunks of 16 lines (ZH_REFINE_CHUNK_BYTES, as zh_knn_graph_refine's host entry), and the device entry"""
    import torch
    ix, X, live, base = fresh(za)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        g = gc.graph("t600", "all_ones", 32, base)
        Q, seeds = gc.queries("t600", 4), rand_seeds("t600", 4, 8, 6)
        ref, rinfo = gc.reference(X, g, 600, 32, live, base, Q, seeds, 10, 33, 2, 0, om, omode)
        ix.set_graph(g)
        same(ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds), ref, "one chunk")
        monkeypatch.setenv("ZH_REFINE_CHUNK_BYTES", "4096")
        ix.set_graph(gc.graph("t600", "ring", 32, base))
        ix.set_graph(g)
        monkeypatch.delenv("ZH_REFINE_CHUNK_BYTES")
        same(ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds), ref, "chunks of 16 lines")
        ix.set_graph(gc.graph("t600", "ring", 32, base))
        d_ids = torch.from_numpy(g[0].copy().view(np.int64)).cuda()  # (the cached graph is read-only: copies)
        d_counts = torch.from_numpy(g[1].copy().view(np.int32)).cuda()
        torch.cuda.synchronize()
        ix.set_graph_device(d_ids.data_ptr(), d_counts.data_ptr(), 600, 32)
        same(ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds), ref, "the device entry")
        assert ix.search_graph_info() == rinfo and ix.graph_info()["g_rows"] == 600
    finally:
        ix.close()


def test_build_and_set_forest_leave_the_graph(za):
    ix, X, live, base = fresh(za)
    try:
        m = thirteen_metrics(za)[0][0]
        ix.set_graph(gc.graph("t600", "exact", 32, base))
        Q, seeds = gc.queries("t600", 4), rand_seeds("t600", 4, 8, 3)
        before = ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds)
        info = ix.graph_info()
        forest = ix.get_forest()
        ix.build()
        same(ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds), before, "after build")
        ix.set_forest(forest)
        same(ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds), before, "after set_forest")
        ix.deduplicate()
        assert ix.graph_info() == info
    finally:
        ix.close()


@pytest.mark.parametrize("how", ["drop_graph", "compact", "clear", "save_load"])
def test_what_ends_the_graph(za, how, tmp_path):
    ix, X, live, base = fresh(za)
    other = None
    try:
        m = thirteen_metrics(za)[0][0]
        Q, seeds = gc.queries("t600", 3), rand_seeds("t600", 3, 8, 4)
        estate(za, lambda: ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds))  # (none attached yet)
        assert ix.graph_info() == {"attached": 0, "g_k": 0, "g_rows": 0, "bytes": 0}
        ix.drop_graph()  # (nothing to drop: fine)
        ix.set_graph(gc.graph("t600", "exact", 32, base))
        ix.search_graph_batch(Q, 10, m, beam=33, seeds=seeds)
        exact = ix.search_exact_batch(Q, 10, m)
        t = ix
        if how == "drop_graph":
            ix.drop_graph()
        elif how == "compact":
            ix.compact()
            exact = None  # (ids are renumbered)
        elif how == "clear":
            ix.clear()
            exact = None
        else:
            path = str(tmp_path / "ix.snap")
            ix.save(path)
            assert ix.graph_info()["attached"] == 1  # (saving leaves the graph on the saved index)
            other = t = za.LSHIndex.load(path, device=0)
        assert t.graph_info() == {"attached": 0, "g_k": 0, "g_rows": 0, "bytes": 0}
        estate(za, lambda: t.search_graph_batch(Q, 10, m, beam=33, seeds=seeds))
        if exact is not None:
            same(t.search_exact_batch(Q, 10, m), exact, "the other calls are unaffected")
        if how == "clear":
            assert t.search_exact_batch(Q, 10, m)[2].sum() == 0
    finally:
        ix.close()
        if other is not None:
            other.close()


# ---------------------------------------------------------------- the Python layer
def test_default_and_lsh_seeds_are_the_explicit_arrays(za):
    ix, X, live, base = fresh(za)
    try:
        m = thirteen_metrics(za)[0][0]
        ix.set_graph(gc.graph("t600", "exact", 32, base))
        Q = gc.queries("t600", 6)
        for n_seed in (1, 8, 32):
            d = ix.search_graph_batch(Q, 10, m, beam=33, n_seed=n_seed)
            same(d, ix.search_graph_batch(Q, 10, m, beam=33, seeds=gc.default_seeds(6, n_seed, 600, base)), "default seeds")
            same(d, ix.search_graph_batch(Q, 10, m, beam=33, seeds=gc.default_seeds(1, n_seed, 600, base)[0]), "a 1-D array is every query's")
        lsh = ix.search_graph_batch(Q, 10, m, beam=33, seeds="lsh", n_seed=8)
        same(lsh, ix.search_graph_batch(Q, 10, m, beam=33, seeds=ix.search_batch(Q, 8, m)[0]), "lsh seeds")
        one = ix.search_graph(Q[2], 10, m, beam=33, n_seed=8)
        d = ix.search_graph_batch(Q, 10, m, beam=33, n_seed=8)
        assert one == list(zip(d[0][2, :d[2][2]].tolist(), d[1][2, :d[2][2]].tolist()))
    finally:
        ix.close()


def test_database_build_graph_and_query(za):
    X, live = gc.table("t600x128")
    db = za.Database(128, za.L2SquaredDistance, za.LSHIndexOptions(64, 3), device=0, id_base=5)
    try:
        db.insert_records(X, ["doc %d" % r for r in range(600)])
        assert db.build_graph(k=8, rounds=3) == {"attached": 1, "g_k": 8, "g_rows": 600, "bytes": db.index.graph_info()["bytes"]}
        Q = gc.queries("t600x128", 5)
        got = db.query_vectors_graph(Q, 10, beam=33, n_seed=8)
        ids, _, counts = db.index.search_graph_batch(Q, 10, db.metric, beam=33, n_seed=8)
        assert got == {b: {int(i): "doc %d" % (int(i) - 5) for i in ids[b, :counts[b]]} for b in range(5)}
        assert all(len(v) == 10 for v in got.values())
        db.remove(np.array([5 + 3, 5 + 4], np.uint64))
        db.compact()
        assert db.index.graph_info()["attached"] == 0
    finally:
        db.index.close()


# ---------------------------------------------------------------- a caller's stream with work pending
def test_the_device_entry_on_a_callers_stream_with_work_pending(za):
    """tests/test_gpu_caller_stream.py's protocol for this call: the buffers hold a different valid input (the queries rolled by one, other seeds)
    and the outputs a sentinel; on a side stream a delay, then the real inputs and fills of every output with a second sentinel, are pending when the
    library is entered with stream = that stream.  The answer must be the host entry's, and the stream idle on return."""
    import torch
    ix, X, live, base = index("t600x128")
    attach("t600x128", "exact", 32)
    m = thirteen_metrics(za)[0][0]
    b, n_seed, top_k = 16, 8, 10
    Q, seeds = gc.queries("t600x128", b), rand_seeds("t600x128", b, n_seed, 5)
    want = ix.search_graph_batch(Q, top_k, m, beam=33, width=2, seeds=seeds)
    S, R = torch.cuda.Stream(), torch.cuda.Stream()
    q_real = torch.from_numpy(Q).cuda()
    s_real = torch.from_numpy(seeds.view(np.int64)).cuda()
    q = torch.roll(q_real, 1, 0).contiguous()
    sd = torch.roll(s_real, 3, 0).contiguous()
    ids = torch.full((b, top_k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    keys = torch.full((b, top_k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(S):  # cycles per millisecond of the delay, measured here
        e[0].record(S)
        torch.cuda._sleep(20_000_000)
        e[1].record(S)
    S.synchronize()
    cycles = int(20_000_000 / max(e[0].elapsed_time(e[1]), 1e-3) * 30.0)  # 30 ms
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        q.copy_(q_real, non_blocking=True)
        sd.copy_(s_real, non_blocking=True)
        for o in (ids, keys):
            o.fill_(0x3C3C3C3C3C3C3C3C)
        counts.fill_(0x3C3C3C3C)
    assert not S.query(), "the side stream was idle before the library was entered: the delay is too short to test anything"
    ix.search_graph_batch_device(q.data_ptr(), b, sd.data_ptr(), n_seed, top_k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr(), beam=33, width=2,
                                 stream=S.cuda_stream)
    assert S.query(), "the call returned with work still pending on the caller's stream"
    with torch.cuda.stream(R):
        got = [t.to("cpu", non_blocking=True) for t in (ids, keys, counts)]
    R.synchronize()
    same((got[0].numpy().view(np.uint64), got[1].numpy().view(np.uint64), got[2].numpy().view(np.uint32)), want, "on the caller's stream")
    S.synchronize()

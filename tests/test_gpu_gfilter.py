"""Filtered graph search on the device (zh_search_graph_filtered_batch): ids, keys, counts and every info field equal the numpy reference
(tests/gfilter_cases.py, pinned on the CPU by tests/test_gfilter_reference.py), the host and `_device` entries agree bit for bit, the walk's figures
are the unfiltered call's, and with every row allowed so is the answer.

Tables are gsearch_cases': 600 x 30 (the generic row loop), 600 x 128 and 600 x 256 (specialised loads), 1500 x 30 once; each with
rc.removed_rows removed and the block of 40 identical rows.  The shared indexes are appended, never built; lifecycle tests make their own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gfilter_cases as fc  # noqa: E402
from tests import gsearch_cases as gc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_gsearch import BASES, BIG, make, rand_seeds  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ESTATE, ELIMIT = -1, -4, -5
WALK_FIELDS = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches")


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
    return g


def mask_of(words, n_bits):
    """the boolean mask LSHIndex.filter_bitmap turns back into these words (bits past n_bits, garbage included, are not part of it)"""
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits].astype(bool)


def raw_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits):
    """the host entry itself, with the filter's words as they are (garbage in the last word included)"""
    from zebra_amd import _ffi
    from zebra_amd.index import _p
    Q, seeds = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(seeds, np.uint64)
    b = Q.shape[0]
    ids, keys, counts = np.full((b, top_k), 0x5A, np.uint64), np.full((b, top_k), 0x5A, np.uint64), np.full(b, 0x5A, np.uint32)
    rc_ = _ffi.lib().zh_search_graph_filtered_batch(ix._h, _p(Q), b, _p(seeds), seeds.shape[1], top_k, beam, width, max_iters, m.metric, m.mode,
                                                    _p(words) if words is not None else None, n_bits, _p(ids), _p(keys), _p(counts))
    return rc_, (ids, keys, counts)


def device_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits, stream=None):
    import torch
    b = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    sd = torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()
    fw = torch.from_numpy(np.concatenate([words, np.zeros(1, np.uint32)]).view(np.int32)).cuda()  # (never empty)
    ids = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    keys = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_graph_filtered_batch_device(q.data_ptr(), b, sd.data_ptr(), seeds.shape[1], top_k, m, fw.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(),
                                          counts.data_ptr(), beam=beam, width=width, max_iters=max_iters, stream=stream)
    return ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def check(za, tname, gname, g_k, Q, seeds, setting, words, n_bits, mi=0, what="", plain=None):
    """the host entry (the words as they are) and the device entry on a shared table against the reference, info included; plain: the unfiltered
    call's info at the same arguments, which the walk's figures must equal -> (answer, info)"""
    ix, X, live, base = index(tname)
    g = attach(tname, gname, g_k)
    beam, width, _, max_iters, top_k = setting
    m, om, omode = thirteen_metrics(za)[mi]
    rc_, got = raw_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits)
    assert rc_ == 0, what
    info = ix.search_graph_filtered_info()
    ref, rinfo = fc.reference(X, g, X.shape[0], g_k, live, base, Q, seeds, top_k, beam, width, max_iters, om, omode, words, n_bits)
    same(got, ref, what)
    assert info == rinfo, (what, info, rinfo)
    dev = device_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits)
    same(dev, got, what + " (device entry)")
    assert ix.search_graph_filtered_info() == rinfo, what
    if plain is not None:
        assert {f: info[f] for f in WALK_FIELDS} == plain, what
    return got, info


# ---------------------------------------------------------------- every filter at every setting
@pytest.mark.parametrize("setting", fc.SETTINGS, ids=["-".join(map(str, s)) for s in fc.SETTINGS])
@pytest.mark.parametrize("tname", ["t600", "t600x128", "t600x256"])
def test_every_filter_at_every_setting(za, tname, setting):
    """the three identities on the way: the walk's figures are a live search_graph_batch's whatever the filter; all ones is its answer bit for
    bit; every returned (id, key) is zh_distance_batch's, of an allowed live row, ascending, no id twice"""
    ix, X, live, base = index(tname)
    attach(tname, "exact", 32)
    beam, width, n_seed, max_iters, top_k = setting
    b = 4
    Q = gc.queries(tname, b)
    seeds = gc.default_seeds(b, n_seed, X.shape[0], base) if n_seed != 8 else rand_seeds(tname, b, n_seed, beam)
    m = thirteen_metrics(za)[0][0]
    unfiltered = ix.search_graph_batch(Q, top_k, m, beam=beam, width=width, max_iters=max_iters, seeds=seeds)
    plain = ix.search_graph_info()
    for fname in fc.FILTERS:
        words, n_bits = fc.table_filter(tname, fname)
        what = "%s %s %s" % (tname, setting, fname)
        (ids, keys, counts), info = check(za, tname, "exact", 32, Q, seeds, setting, words, n_bits, what=what, plain=plain)
        assert ix.search_graph_info() == plain, what  # (the sibling's record is left alone)
        allowed = fc.allowed_rows(words, n_bits, live)
        for i in range(b):
            c = int(counts[i])
            rows = (ids[i, :c] - np.uint64(base)).astype(np.int64)
            assert allowed[rows].all() and np.unique(rows).size == c, what
            assert (np.lexsort((ids[i, :c], keys[i, :c])) == np.arange(c)).all(), what
            if c:
                assert (keys[i, :c] == m.distance_batch(X[rows], Q[i])).all(), what
        if fname == "ones":
            same((ids, keys, counts), unfiltered, what + ": the unfiltered answer")
        if fname in ("zeros", "removed_only"):
            assert info["rows_allowed"] == 0 and info["returned"] == 0 and info["keyed"] > 0, what  # (the walk still ran)


def test_the_larger_table(za):
    ix, X, live, base = index("t1500")
    Q = gc.queries("t1500", 16)
    for setting, fname in (((64, 4, 32, 0, 10), "mod10_3"), ((8, 1, 8, 0, 8), "even"), ((64, 1, 32, 0, 64), "short_garbage")):
        words, n_bits = fc.table_filter("t1500", fname)
        check(za, "t1500", "exact", 32, Q, rand_seeds("t1500", 16, setting[2], 3), setting, words, n_bits, what="t1500 %s %s" % (setting, fname))


def test_sixty_four_queries_and_an_odd_count(za):
    words, n_bits = fc.table_filter("t600", "even")
    for b in (64, 37):
        check(za, "t600", "exact", 5, gc.queries("t600", b), rand_seeds("t600", b, 8), (8, 2, 8, 0, 8), words, n_bits, what="b %d" % b)


# ---------------------------------------------------------------- the graphs, the keys, the dimensions
@pytest.mark.parametrize("gname", sorted(rc.GRAPHS))
def test_every_graph(za, gname):
    Q = gc.queries("t600", 6)
    if gname == "block":
        Q = Q.copy()
        Q[:3] = gc.table("t600")[0][rc.BLOCK[0]]  # (queries AT the block: forty equal keys, half of them allowed, ranked by id)
    seeds = rand_seeds("t600", 6, 8, sum(gname.encode()))
    if gname == "block":
        seeds[:, 0] = BIG + rc.BLOCK[0] + 5
    words, n_bits = fc.table_filter("t600", "even")
    check(za, "t600", gname, 32, Q, seeds, (64, 2, 8, 0, 33), words, n_bits, what=gname)


@pytest.mark.parametrize("mi", range(13))
def test_every_metric(za, mi):
    words, n_bits = fc.table_filter("t600x128", "even")
    check(za, "t600x128", "exact", 32, gc.queries("t600x128", 4), rand_seeds("t600x128", 4, 8, mi), (33, 2, 8, 0, 10), words, n_bits, mi=mi,
          what="metric %d" % mi)


_DIMS = {}  # d -> (index, X, live, graph)


@pytest.fixture(scope="module", autouse=True)
def _close_dim_indexes():
    yield
    for entry in _DIMS.values():
        entry[0].close()
    _DIMS.clear()


@pytest.mark.parametrize("mname", ["l2sq", "cosine", "manhattan"])
@pytest.mark.parametrize("d", [128, 256, 384, 512, 768, 1024])
def test_every_specialised_dimension(za, d, mname):
    """zh_dispatch_kind_dim's table for the filtered kernel: a dimension that reached another's instantiation, or a kind another kind's, changes
    keys.  600 rows, the ring at g_k = 8"""
    n = 600
    if d not in _DIMS:
        X = rc.table(n, d)
        live = np.ones(n, bool)
        live[rc.removed_rows(n)] = False
        ix = make(za, X, live, 0)
        graph = rc.g_ring(n, 8, live, 0)
        ix.set_graph(graph)
        _DIMS[d] = (ix, X, live, graph)
    ix, X, live, graph = _DIMS[d]
    m, om, omode = {"l2sq": (za.L2SquaredDistance(), zo.L2SQ, 0), "cosine": (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
                    "manhattan": (za.ManhattanDistance(), zo.MANHATTAN, 0)}[mname]
    Q = zo.synth_queries(4, d, n)
    seeds = np.random.default_rng([0xD136, d]).integers(0, n, (4, 8)).astype(np.uint64)
    words, n_bits = fc.FILTERS["mod10_3"](n, live)
    got = ix.search_graph_filtered_batch(Q, 10, m, mask_of(words, n_bits), beam=33, width=2, seeds=seeds)
    ref, rinfo = fc.reference(X, graph, n, 8, live, 0, Q, seeds, 10, 33, 2, 0, om, omode, words, n_bits)
    same(got, ref, "d %d, %s" % (d, mname))
    assert ix.search_graph_filtered_info() == rinfo


# ---------------------------------------------------------------- limits and refusals
def test_limits_and_refusals(za):
    ix, X, live, base = index("t600")
    m = thirteen_metrics(za)[0][0]
    Q, seeds = gc.queries("t600", 2), rand_seeds("t600", 2, 8)
    words, n_bits = fc.table_filter("t600", "even")
    mask = mask_of(words, n_bits)
    attach("t600", "exact", 32)
    ix.search_graph_filtered_batch(Q, 4, m, mask, beam=8, seeds=seeds)
    before = ix.search_graph_filtered_info()

    def refused(code, text, **kw):
        args = dict(top_k=4, beam=8, width=1, max_iters=0)
        args.update(kw)
        rc_, _ = raw_call(ix, Q, seeds, args["top_k"], m, args["beam"], args["width"], args["max_iters"], kw.get("words", words), kw.get("n_bits", n_bits))
        from zebra_amd import _ffi
        assert rc_ == code and text in _ffi.lib().zh_last_error(), (kw, rc_, _ffi.lib().zh_last_error())
        assert ix.search_graph_filtered_info() == before

    refused(ELIMIT, b"top_k 9 > beam 8", top_k=9)
    refused(ELIMIT, b"beam 257 >", beam=257, top_k=4)
    refused(ELIMIT, b"width", width=9)                      # 9 * 32 > 256: under the lock
    refused(ELIMIT, b"max_iters", max_iters=65536)
    refused(EINVAL, b"null filter", words=None)
    refused(EINVAL, b"filter of 601 rows", n_bits=601, words=np.concatenate([words, np.zeros(1, np.uint32)]))
    refused(ELIMIT, b"width", width=9, n_bits=601)          # the width * g_k check comes before the filter's length
    # n_bits = 0 with a null filter: counts of 0, the walk still run
    rc_, (ids, keys, counts) = raw_call(ix, Q, seeds, 4, m, 8, 1, 0, None, 0)
    info = ix.search_graph_filtered_info()
    assert rc_ == 0 and (counts == 0).all() and (ids == NONE).all() and (keys == NONE).all()
    assert info["rows_allowed"] == 0 and info["offered"] == 0 and info["keyed"] > 0 and info["iterations"] > 0
    # b = 0
    e = ix.search_graph_filtered_batch(np.zeros((0, 30), np.float32), 4, m, mask, beam=8, seeds=np.zeros((0, 3), np.uint64))
    assert e[0].shape == (0, 4) and e[2].shape == (0,) and ix.search_graph_filtered_info() == info


def test_no_graph_is_estate_before_the_filters_length(za):
    X, live = gc.table("t600")
    ix = make(za, X, live, 0)
    try:
        m = thirteen_metrics(za)[0][0]
        rc_, _ = raw_call(ix, gc.queries("t600", 1), np.zeros((1, 4), np.uint64), 4, m, 8, 1, 0, np.zeros(40, np.uint32), 1000)
        assert rc_ == ESTATE
    finally:
        ix.close()


# ---------------------------------------------------------------- lifecycle
def test_append_remove_and_compact(za):
    """a filter made before an append is shorter than the table and stays valid: the appended rows are seeds but not allowed; a longer one allows
    them.  A row removed between attach and search is neither walked nor returned.  After compact the table is shorter: the old mask is refused"""
    X, live = gc.table("t600")
    live = live.copy()
    base = BIG
    ix = make(za, X, live, base, trees=True)
    try:
        m, om, omode = thirteen_metrics(za)[0]
        g = gc.graph("t600", "exact", 32, base)
        ix.set_graph(g)
        Q = gc.queries("t600", 4)
        old_words, old_bits = fc.bitmap(np.arange(600) % 2 == 0)
        extra = np.concatenate([Q[:2], zo.synth_rows(6, 30, row0=9000)])  # (two appended rows ARE queries: key 0)
        ix.append(extra)
        X2, live2 = np.concatenate([X, extra]), np.concatenate([live, np.ones(8, bool)])
        seeds = np.concatenate([rand_seeds("t600", 4, 6, 9), np.array([[base + 600, base + 601]] * 4, np.uint64)], axis=1)
        for words, n_bits, hit in ((old_words, old_bits, False), fc.bitmap(np.arange(608) % 2 == 0) + (True,)):
            got = ix.search_graph_filtered_batch(Q, 8, m, mask_of(words, n_bits), beam=16, seeds=seeds)
            ref, rinfo = fc.reference(X2, g, 600, 32, live2, base, Q, seeds, 8, 16, 1, 0, om, omode, words, n_bits, attach_rows=600)
            same(got, ref, "after append, %d bits" % n_bits)
            assert ix.search_graph_filtered_info() == rinfo
            assert (got[0][0, 0] == base + 600) == hit  # (row 600 is query 0 itself, and even)
        # remove what the answer's head names, and more
        words, n_bits = fc.bitmap(np.arange(608) % 2 == 0)
        gone = np.unique(np.concatenate([(got[0][:, :3].reshape(-1) - np.uint64(base)).astype(np.int64), np.arange(10, 600, 11)]))
        gone = gone[(gone < 600) & live2[gone]]  # (rows of the graph: the appended ones stay)
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
        live2[gone] = False
        got = ix.search_graph_filtered_batch(Q, 8, m, mask_of(words, n_bits), beam=16, seeds=seeds)
        ref, rinfo = fc.reference(X2, g, 600, 32, live2, base, Q, seeds, 8, 16, 1, 0, om, omode, words, n_bits, attach_rows=600)
        same(got, ref, "after remove")
        assert ix.search_graph_filtered_info() == rinfo
        assert not np.isin(got[0][got[0] != NONE] - np.uint64(base), gone.astype(np.uint64)).any()
        # compact: the rows move (the graph goes), the table is shorter than the mask
        ix.compact()
        stored = ix.stored_rows()
        assert stored < 608
        ix.set_graph((np.zeros((stored, 4), np.uint64), np.zeros(stored, np.uint32)))
        rc_, _ = raw_call(ix, Q, seeds, 8, m, 16, 1, 0, words, n_bits)
        assert rc_ == EINVAL
        rc_, _ = raw_call(ix, Q, seeds, 8, m, 16, 1, 0, words, stored)
        assert rc_ == 0
    finally:
        ix.close()


# ---------------------------------------------------------------- the Python layer
def test_allowed_default_and_lsh_seeds(za):
    X, live = gc.table("t600")
    base = BIG
    ix = make(za, X, live, base, trees=True)
    try:
        m = thirteen_metrics(za)[0][0]
        ix.set_graph(gc.graph("t600", "exact", 32, base))
        Q = gc.queries("t600", 5)
        mask = np.arange(600) % 10 == 3
        rows = np.flatnonzero(mask)
        for n_seed in (1, 8, 32, 64):
            want = np.array([rows[j * rows.size // n_seed] for j in range(n_seed)], np.uint64) + np.uint64(base)
            a = ix.search_graph_filtered_batch(Q, 10, m, mask, beam=33, seeds="allowed", n_seed=n_seed)
            same(a, ix.search_graph_filtered_batch(Q, 10, m, mask, beam=33, seeds=want), "allowed seeds, n_seed %d" % n_seed)
            assert ix.search_graph_filtered_info()["seeds"] == 5 * np.count_nonzero(live[np.unique((want - np.uint64(base)).astype(np.int64))])
        few = np.zeros(600, bool)
        few[[5, 77, 300]] = True  # (all live)
        assert live[[5, 77, 300]].all()
        a = ix.search_graph_filtered_batch(Q, 10, m, few, beam=33, seeds="allowed", n_seed=8)
        assert ix.search_graph_filtered_info()["seeds"] == 5 * 3  # every set position a seed, the repeats ignored
        assert (a[2] == 3).all() and (np.sort(a[0][:, :3], axis=1) == np.array([5, 77, 300], np.uint64) + np.uint64(base)).all()
        a = ix.search_graph_filtered_batch(Q, 10, m, np.zeros(600, bool), beam=33, seeds="allowed", n_seed=8)
        assert (a[2] == 0).all() and ix.search_graph_filtered_info()["seeds"] == 0
        ids_form = ix.search_graph_filtered_batch(Q, 10, m, rows.astype(np.uint64) + np.uint64(base), beam=33, n_seed=8)  # (allowed as ids)
        same(ids_form, ix.search_graph_filtered_batch(Q, 10, m, mask, beam=33, seeds=gc.default_seeds(5, 8, 600, base)), "default seeds")
        lsh = ix.search_graph_filtered_batch(Q, 10, m, mask, beam=33, seeds="lsh", n_seed=8)
        same(lsh, ix.search_graph_filtered_batch(Q, 10, m, mask, beam=33, seeds=ix.search_batch(Q, 8, m)[0]), "lsh seeds")
    finally:
        ix.close()


def test_database_query_vectors_graph_where(za):
    X, live = gc.table("t600x128")
    db = za.Database(128, za.L2SquaredDistance, za.LSHIndexOptions(64, 3), device=0, id_base=5)
    try:
        db.insert_records(X, ["doc %d" % r for r in range(600)])
        db.build_graph(k=8, rounds=3)
        Q = gc.queries("t600x128", 5)
        pred = lambda doc: int(doc.split()[1]) % 3 == 0  # noqa: E731
        got = db.query_vectors_graph_where(Q, 10, pred, beam=33, n_seed=8)
        allowed = np.array([5 + r for r in range(600) if r % 3 == 0], np.uint64)
        ids, _, counts = db.index.search_graph_filtered_batch(Q, 10, db.metric, allowed, beam=33, n_seed=8)
        assert got == {b: {int(i): "doc %d" % (int(i) - 5) for i in ids[b, :counts[b]]} for b in range(5)}
        assert all(len(v) == 10 and all(pred(doc) for doc in v.values()) for v in got.values())
        assert db.query_vectors_graph_where(Q, 10, lambda doc: False, beam=33) == {b: {} for b in range(5)}
    finally:
        db.index.close()


# ---------------------------------------------------------------- a caller's stream with work pending
def test_the_device_entry_on_a_callers_stream_with_work_pending(za):
    """tests/test_gpu_caller_stream.py's protocol for this call: the buffers hold a different valid input (the queries rolled by one, other seeds,
    the complement of the filter) and the outputs a sentinel; on a side stream a delay, then the real inputs and fills of every output with a
    second sentinel, are pending when the library is entered with stream = that stream.  The answer must be the host entry's, and the stream idle
    on return."""
    import torch
    ix, X, live, base = index("t600x128")
    attach("t600x128", "exact", 32)
    m = thirteen_metrics(za)[0][0]
    b, n_seed, top_k = 16, 8, 10
    Q, seeds = gc.queries("t600x128", b), rand_seeds("t600x128", b, n_seed, 5)
    words, n_bits = fc.table_filter("t600x128", "even")
    want = ix.search_graph_filtered_batch(Q, top_k, m, mask_of(words, n_bits), beam=33, width=2, seeds=seeds)
    S, R = torch.cuda.Stream(), torch.cuda.Stream()
    q_real = torch.from_numpy(Q).cuda()
    s_real = torch.from_numpy(seeds.view(np.int64)).cuda()
    f_real = torch.from_numpy(words.view(np.int32)).cuda()
    q = torch.roll(q_real, 1, 0).contiguous()
    sd = torch.roll(s_real, 3, 0).contiguous()
    fw = torch.from_numpy((~words).view(np.int32)).cuda()
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
        fw.copy_(f_real, non_blocking=True)
        for o in (ids, keys):
            o.fill_(0x3C3C3C3C3C3C3C3C)
        counts.fill_(0x3C3C3C3C)
    assert not S.query(), "the side stream was idle before the library was entered: the delay is too short to test anything"
    ix.search_graph_filtered_batch_device(q.data_ptr(), b, sd.data_ptr(), n_seed, top_k, m, fw.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(),
                                          counts.data_ptr(), beam=33, width=2, stream=S.cuda_stream)
    assert S.query(), "the call returned with work still pending on the caller's stream"
    with torch.cuda.stream(R):
        got = [t.to("cpu", non_blocking=True) for t in (ids, keys, counts)]
    R.synchronize()
    same((got[0].numpy().view(np.uint64), got[1].numpy().view(np.uint64), got[2].numpy().view(np.uint32)), want, "on the caller's stream")
    S.synchronize()

"""Filter-steered graph search on the device (zh_search_graph_steered_batch): ids, keys, counts and every info field equal the numpy reference
(tests/gsteer_cases.py, pinned on the CPU by tests/test_gsteer_reference.py) for both `hops`, the host and `_device` entries agree bit for bit, and
with every row allowed the answer and the walk's figures are a live search_graph_batch's.

Tables are gsearch_cases': 600 x 30 (the generic row loop), 600 x 128 and 600 x 256 (specialised loads), 1500 x 30 for the graphs whose second hop
overflows the 256 candidate slots; each with rc.removed_rows removed and the block of 40 identical rows.  The shared indexes are appended, never
built; lifecycle tests make their own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gfilter_cases as fc  # noqa: E402
from tests import gsearch_cases as gc  # noqa: E402
from tests import gsteer_cases as sc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_gsearch import BASES, BIG, make, rand_seeds  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402

NONE = np.uint64(2**64 - 1)
EINVAL, ESTATE, ELIMIT = -1, -4, -5


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


_SHARED = {}  # table name -> (index, X, live, id_base); no test changes the rows of one


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()


def index(tname):
    import zebra_amd
    if tname not in _SHARED:
        X, live = gc.table(tname)
        _SHARED[tname] = (make(zebra_amd, X, live, BASES[tname]), X, live, BASES[tname])
    return _SHARED[tname]


def mask_of(words, n_bits):
    """the boolean mask LSHIndex.filter_bitmap turns back into these words (bits past n_bits, garbage included, are not part of it)"""
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits].astype(bool)


def raw_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits, hops):
    """the host entry itself, with the filter's words as they are (garbage in the last word included)"""
    from zebra_amd import _ffi
    from zebra_amd.index import _p
    Q, seeds = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(seeds, np.uint64)
    b = Q.shape[0]
    ids, keys, counts = np.full((b, top_k), 0x5A, np.uint64), np.full((b, top_k), 0x5A, np.uint64), np.full(b, 0x5A, np.uint32)
    rc_ = _ffi.lib().zh_search_graph_steered_batch(ix._h, _p(Q), b, _p(seeds), seeds.shape[1], top_k, beam, width, max_iters, m.metric, m.mode,
                                                   _p(words) if words is not None else None, n_bits, hops, _p(ids), _p(keys), _p(counts))
    return rc_, (ids, keys, counts)


def device_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits, hops, stream=None):
    import torch
    b = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    sd = torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()
    fw = torch.from_numpy(np.concatenate([words, np.zeros(1, np.uint32)]).view(np.int32)).cuda()  # (never empty)
    ids = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    keys = torch.full((b, top_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.search_graph_steered_batch_device(q.data_ptr(), b, sd.data_ptr(), seeds.shape[1], top_k, m, fw.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(),
                                         counts.data_ptr(), hops=hops, beam=beam, width=width, max_iters=max_iters, stream=stream)
    return ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def check_on(za, ix, X, live, base, g, g_rows, g_k, Q, seeds, setting, words, n_bits, hops, mi=0, what="", attach_rows=None, device=True):
    """the host entry (the words as they are) and the device entry against the reference, info included; the identities every answer obeys
    -> (answer, info)"""
    beam, width, _, max_iters, top_k = setting
    m, om, omode = thirteen_metrics(za)[mi]
    what = "%s hops %d" % (what, hops)
    rc_, got = raw_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words, n_bits, hops)
    assert rc_ == 0, what
    info = ix.search_graph_steered_info()
    ref, rinfo = sc.reference(X, g, g_rows, g_k, live, base, Q, seeds, top_k, beam, width, max_iters, om, omode, words, n_bits, hops,
                              attach_rows=attach_rows)
    same(got, ref, what)
    assert info == rinfo, (what, info, rinfo)
    assert info["keyed"] == info["seeds"] + info["direct"] + info["via_bridge"], what
    if hops == 1:
        assert info["bridges"] == info["via_bridge"] == 0, what
    if device:
        dev = device_call(ix, Q, seeds, top_k, m, beam, width, max_iters, words if words is not None else np.zeros(0, np.uint32), n_bits, hops)
        same(dev, got, what + " (device entry)")
        assert ix.search_graph_steered_info() == rinfo, what
    return got, info


def check(za, tname, g, g_k, Q, seeds, setting, words, n_bits, hops, mi=0, what="", g_rows=None):
    """check_on for a shared table; g is attached"""
    ix, X, live, base = index(tname)
    ix.set_graph(g if g_rows is None else (g[0][:g_rows], g[-1][:g_rows]))
    return check_on(za, ix, X, live, base, g, X.shape[0] if g_rows is None else g_rows, g_k, Q, seeds, setting, words, n_bits, hops, mi, what)


# ---------------------------------------------------------------- every filter at every setting, both hops
@pytest.mark.parametrize("setting", sc.SETTINGS, ids=["-".join(map(str, s)) for s in sc.SETTINGS])
@pytest.mark.parametrize("tname", ["t600", "t600x128", "t600x256"])
def test_every_filter_at_every_setting(za, tname, setting):
    """the identities on the way: all ones is a live search_graph_batch's answer and seven figures bit for bit, with no bridge; every returned
    (id, key) is zh_distance_batch's, of an allowed live row, ascending, no id twice; a filter that allows nothing launches and finds nothing"""
    ix, X, live, base = index(tname)
    g = gc.graph(tname, "exact", 32, base)
    ix.set_graph(g)
    beam, width, n_seed, max_iters, top_k = setting
    b = 3
    Q = gc.queries(tname, b)
    seeds = gc.default_seeds(b, n_seed, X.shape[0], base) if n_seed != 8 else rand_seeds(tname, b, n_seed, beam)
    m = thirteen_metrics(za)[0][0]
    unfiltered = ix.search_graph_batch(Q, top_k, m, beam=beam, width=width, max_iters=max_iters, seeds=seeds)
    plain = ix.search_graph_info()
    capped = 0
    for fname in fc.FILTERS:
        words, n_bits = fc.table_filter(tname, fname)
        allowed = fc.allowed_rows(words, n_bits, live)
        for hops in (1, 2):
            what = "%s %s %s" % (tname, setting, fname)
            (ids, keys, counts), info = check_on(za, ix, X, live, base, g, X.shape[0], 32, Q, seeds, setting, words, n_bits, hops, what=what)
            assert ix.search_graph_info() == plain, what  # (the sibling's record is left alone)
            capped += info["capped"]
            for i in range(b):
                c = int(counts[i])
                rows = (ids[i, :c] - np.uint64(base)).astype(np.int64)
                assert allowed[rows].all() and np.unique(rows).size == c, what
                assert (np.lexsort((ids[i, :c], keys[i, :c])) == np.arange(c)).all(), what
                if c:
                    assert (keys[i, :c] == m.distance_batch(X[rows], Q[i])).all(), what
            if fname == "ones":
                same((ids, keys, counts), unfiltered, what + ": the unfiltered answer")
                assert {f: info[f] for f in sc.WALK_FIELDS} == plain and info["bridges"] == info["via_bridge"] == 0, what
            if fname in ("zeros", "removed_only"):
                assert (counts == 0).all() and info["rows_allowed"] == info["seeds"] == info["iterations"] == info["returned"] == 0, what
                assert info["launches"] == 1, what  # (the kernel still ran: the host never read the filter's count)
    if max_iters:
        assert capped > 0


def test_null_filter_of_no_rows(za):
    ix, X, live, base = index("t600")
    ix.set_graph(gc.graph("t600", "exact", 32, base))
    m = thirteen_metrics(za)[0][0]
    for hops in (1, 2):
        rc_, (ids, keys, counts) = raw_call(ix, gc.queries("t600", 2), rand_seeds("t600", 2, 8), 4, m, 8, 1, 0, None, 0, hops)
        info = ix.search_graph_steered_info()
        assert rc_ == 0 and (counts == 0).all() and (ids == NONE).all() and (keys == NONE).all()
        assert info == dict.fromkeys(sc.FIELDS, 0) | {"queries": 2, "launches": 1}


# ---------------------------------------------------------------- (a), (b), (c) of gsteer_cases, and every adversarial graph
def test_the_random_graph_truncates(za):
    """the 1500-row random out-32 graph at width 4 under "even": 67 of 68 iterations fill the 256 slots (pinned on the CPU)"""
    c = sc.RANDOM_CASE
    ix, X, live, base = index(c["tname"])
    g = sc.random_graph(c["tname"], c["g_k"], base)
    words, n_bits = fc.table_filter(c["tname"], c["fname"])
    seeds = gc.default_seeds(c["b"], c["setting"][2], X.shape[0], base)
    for hops in (1, 2):
        _, info = check(za, c["tname"], g, c["g_k"], gc.queries(c["tname"], c["b"]), seeds, c["setting"], words, n_bits, hops, what="random graph")
    assert info["cand_full"] == 67 and info["via_bridge"] == 13616 and info["bridges"] == 4184


@pytest.mark.parametrize("name", sc.SEAMS)
def test_the_seams(za, name):
    """the hand-built graphs at g_k = 64: exactly 256 candidates, one more than 256, a removed bridge, a bridge past the attached lines, a bridge
    naming the parent and the beam, two parents sharing a bridge"""
    ix, X, live, base = index(sc.SEAM_TABLE)
    for hops in (1, 2):
        (ref, rinfo), g, g_rows, seeds, width = sc.run_seam(name, hops, id_base=base)
        got, info = check(za, sc.SEAM_TABLE, g, sc.SEAM_K, gc.queries(sc.SEAM_TABLE, 2), seeds, (256, width, seeds.shape[1], 1, 256),
                          *fc.table_filter(sc.SEAM_TABLE, "even"), hops, what=name, g_rows=g_rows if g_rows != X.shape[0] else None)
        same(got, ref, name)
        assert info == rinfo


@pytest.mark.parametrize("g_k", sc.WIDTHS)
def test_line_widths_that_split_the_second_hop_differently(za, g_k):
    ix, X, live, base = index("t600")
    g = gc.graph("t600", "exact" if g_k > 1 else "ring", g_k, base)
    setting = sc.width_setting(g_k)
    Q = gc.queries("t600", 3)
    for fname in ("even", "mod10_3"):
        words, n_bits = fc.table_filter("t600", fname)
        seeds = sc.allowed_seeds(3, setting[2], words, n_bits, base)
        for hops in (1, 2):
            check(za, "t600", g, g_k, Q, seeds, setting, words, n_bits, hops, what="g_k %d %s" % (g_k, fname))


@pytest.mark.parametrize("gname", sorted(rc.GRAPHS))
def test_every_graph(za, gname):
    Q = gc.queries("t600", 4)
    if gname == "block":
        Q = Q.copy()
        Q[:2] = gc.table("t600")[0][rc.BLOCK[0]]  # (queries AT the block: forty equal keys, half of them allowed, ranked by id)
    seeds = rand_seeds("t600", 4, 8, sum(gname.encode()))
    if gname == "block":
        seeds[:, 0] = BIG + rc.BLOCK[0] + 4
    words, n_bits = fc.table_filter("t600", "even")
    for hops in (1, 2):
        check(za, "t600", gc.graph("t600", gname, 32, BIG), 32, Q, seeds, (64, 2, 8, 0, 33), words, n_bits, hops, what=gname)


def test_the_larger_table_and_an_odd_count(za):
    Q = gc.queries("t1500", 37)
    g = gc.graph("t1500", "exact", 32, 0)
    for setting, fname in (((64, 4, 32, 0, 10), "mod10_3"), ((8, 1, 8, 0, 8), "even")):
        words, n_bits = fc.table_filter("t1500", fname)
        check(za, "t1500", g, 32, Q, rand_seeds("t1500", 37, setting[2], 3), setting, words, n_bits, 2, what="t1500 %s %s" % (setting, fname))


# ---------------------------------------------------------------- the keys, the dimensions
@pytest.mark.parametrize("mi", range(13))
def test_every_metric(za, mi):
    words, n_bits = fc.table_filter("t600x128", "mod10_3")
    check(za, "t600x128", gc.graph("t600x128", "exact", 32, 0), 32, gc.queries("t600x128", 3), sc.allowed_seeds(3, 8, words, n_bits, 0), (33, 2, 8, 0, 10),
          words, n_bits, 2, mi=mi, what="metric %d" % mi)


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
    """zh_dispatch_kind_dim's table for the steered kernel: a dimension that reached another's instantiation, or a kind another kind's, changes
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
    Q = zo.synth_queries(3, d, n)
    words, n_bits = fc.FILTERS["mod10_3"](n, live)
    seeds = sc.allowed_seeds(3, 8, words, n_bits, 0)
    got = ix.search_graph_steered_batch(Q, 10, m, mask_of(words, n_bits), hops=2, beam=33, width=2, seeds=seeds)
    ref, rinfo = sc.reference(X, graph, n, 8, live, 0, Q, seeds, 10, 33, 2, 0, om, omode, words, n_bits, 2)
    same(got, ref, "d %d, %s" % (d, mname))
    assert ix.search_graph_steered_info() == rinfo and rinfo["via_bridge"] > 0


# ---------------------------------------------------------------- limits and refusals
def test_limits_and_refusals(za):
    ix, X, live, base = index("t600")
    m = thirteen_metrics(za)[0][0]
    Q, seeds = gc.queries("t600", 2), rand_seeds("t600", 2, 8)
    words, n_bits = fc.table_filter("t600", "even")
    mask = mask_of(words, n_bits)
    ix.set_graph(gc.graph("t600", "exact", 32, base))
    ix.search_graph_steered_batch(Q, 4, m, mask, beam=8, seeds=seeds)
    before = ix.search_graph_steered_info()
    ix.search_graph_filtered_batch(Q, 4, m, mask, beam=8, seeds=seeds)
    blind = ix.search_graph_filtered_info()

    def refused(code, text, **kw):
        args = dict(top_k=4, beam=8, width=1, max_iters=0, hops=2)
        args.update(kw)
        rc_, _ = raw_call(ix, Q, seeds, args["top_k"], m, args["beam"], args["width"], args["max_iters"], kw.get("words", words), kw.get("n_bits", n_bits),
                          args["hops"])
        from zebra_amd import _ffi
        assert rc_ == code and text in _ffi.lib().zh_last_error(), (kw, rc_, _ffi.lib().zh_last_error())
        assert ix.search_graph_steered_info() == before and ix.search_graph_filtered_info() == blind

    refused(ELIMIT, b"top_k 9 > beam 8", top_k=9)
    refused(ELIMIT, b"beam 257 >", beam=257, top_k=4)
    refused(ELIMIT, b"width", width=9)                      # 9 * 32 > 256: under the lock
    refused(ELIMIT, b"max_iters", max_iters=65536)
    for hops in (0, 3, -1):
        refused(EINVAL, b"hops", hops=hops)
    refused(ELIMIT, b"max_iters", max_iters=65536, hops=3)  # hops is the last of the scalar limits
    refused(EINVAL, b"hops", hops=0, width=9)               # ... and judged before the lock is taken
    refused(EINVAL, b"null filter", words=None)
    refused(EINVAL, b"filter of 601 rows", n_bits=601, words=np.concatenate([words, np.zeros(1, np.uint32)]))
    refused(ELIMIT, b"width", width=9, n_bits=601)          # the width * g_k check comes before the filter's length
    # b = 0
    e = ix.search_graph_steered_batch(np.zeros((0, 30), np.float32), 4, m, mask, beam=8, seeds=np.zeros((0, 3), np.uint64))
    assert e[0].shape == (0, 4) and e[2].shape == (0,) and ix.search_graph_steered_info() == before


def test_no_graph_is_estate_before_the_filters_length(za):
    X, live = gc.table("t600")
    ix = make(za, X, live, 0)
    try:
        m = thirteen_metrics(za)[0][0]
        rc_, _ = raw_call(ix, gc.queries("t600", 1), np.zeros((1, 4), np.uint64), 4, m, 8, 1, 0, np.zeros(40, np.uint32), 1000, 2)
        assert rc_ == ESTATE
    finally:
        ix.close()


# ---------------------------------------------------------------- lifecycle
def test_append_remove_and_compact(za):
    """after an append a new allowed row is a seed (and an answer); a row removed between attach and search is no bridge and no answer; after
    compact the graph is gone"""
    X, live = gc.table("t600")
    live = live.copy()
    base = BIG
    ix = make(za, X, live, base, trees=True)
    try:
        g = gc.graph("t600", "exact", 32, base)
        ix.set_graph(g)
        Q = gc.queries("t600", 4)
        extra = np.concatenate([Q[:2], zo.synth_rows(6, 30, row0=9000)])  # (two appended rows ARE queries: key 0)
        ix.append(extra)
        X2, live2 = np.concatenate([X, extra]), np.concatenate([live, np.ones(8, bool)])
        seeds = np.concatenate([rand_seeds("t600", 4, 6, 9), np.array([[base + 600, base + 601]] * 4, np.uint64)], axis=1)
        for words, n_bits, hit in (fc.bitmap(np.arange(600) % 2 == 0) + (False,), fc.bitmap(np.arange(608) % 2 == 0) + (True,)):
            for hops in (1, 2):
                got, _ = check_on(za, ix, X2, live2, base, g, 600, 32, Q, seeds, (16, 1, 8, 0, 8), words, n_bits, hops, what="after append", attach_rows=600)
                assert (got[0][0, 0] == base + 600) == hit  # (row 600 is query 0 itself, and even: a seed only where the mask covers it)
        # remove the answer's head (allowed rows) and every odd row a line of it names (bridges), and more
        words, n_bits = fc.bitmap(np.arange(608) % 2 == 0)
        head = (got[0][:, :3].reshape(-1) - np.uint64(base)).astype(np.int64)
        head = head[head < 600]
        named = (g[0][head].reshape(-1) - np.uint64(base)).astype(np.int64)
        gone = np.unique(np.concatenate([head, named[(named < 600) & (named % 2 == 1)][::2], np.arange(10, 600, 11)]))
        gone = gone[(gone < 600) & live2[gone]]
        assert ix.remove(gone.astype(np.uint64) + np.uint64(base)).size == gone.size
        live2[gone] = False
        for hops in (1, 2):
            got, _ = check_on(za, ix, X2, live2, base, g, 600, 32, Q, seeds, (16, 1, 8, 0, 8), words, n_bits, hops, what="after remove", attach_rows=600)
            assert not np.isin(got[0][got[0] != NONE] - np.uint64(base), gone.astype(np.uint64)).any()
        ix.compact()
        m = thirteen_metrics(za)[0][0]
        rc_, _ = raw_call(ix, Q, seeds, 8, m, 16, 1, 0, words, ix.stored_rows(), 2)
        assert rc_ == ESTATE
    finally:
        ix.close()


# ---------------------------------------------------------------- the Python layer
def test_the_four_seed_modes(za):
    X, live = gc.table("t600")
    base = BIG
    ix = make(za, X, live, base, trees=True)
    try:
        m = thirteen_metrics(za)[0][0]
        ix.set_graph(gc.graph("t600", "exact", 32, base))
        Q = gc.queries("t600", 5)
        mask = np.arange(600) % 10 == 3
        rows = np.flatnonzero(mask)
        words, n_bits = fc.bitmap(mask)
        for n_seed in (1, 8, 64):
            want = sc.allowed_seeds(5, n_seed, words, n_bits, base)
            a = ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, n_seed=n_seed)  # (the default: "allowed")
            same(a, ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, seeds=want), "allowed seeds, n_seed %d" % n_seed)
            assert ix.search_graph_steered_info()["seeds"] == 5 * np.count_nonzero(live[np.unique((want[0] - np.uint64(base)).astype(np.int64))])
        none = ix.search_graph_steered_batch(Q, 10, m, rows.astype(np.uint64) + np.uint64(base), beam=33, seeds=None, n_seed=64)  # (allowed as ids)
        strided = gc.default_seeds(5, 64, 600, base)
        same(none, ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, seeds=strided), "seeds=None")
        in_a = (mask & live)[(strided[0] - np.uint64(base)).astype(np.int64)]
        assert ix.search_graph_steered_info()["seeds"] == 5 * np.count_nonzero(in_a) > 0  # (the disallowed strided rows are ignored)
        lsh = ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, seeds="lsh", n_seed=8)
        same(lsh, ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, seeds=ix.search_batch(Q, 8, m)[0]), "lsh seeds")
        one = ix.search_graph_steered_batch(Q, 10, m, mask, beam=33, seeds=strided[0])  # ([n_seed]: the same for every query)
        same(one, none, "a row of seeds")
        a = ix.search_graph_steered_batch(Q, 10, m, np.zeros(600, bool), beam=33, n_seed=8)
        assert (a[2] == 0).all() and ix.search_graph_steered_info()["seeds"] == 0
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
        allowed = np.array([5 + r for r in range(600) if r % 3 == 0], np.uint64)
        for hops in (2, 1):
            got = db.query_vectors_graph_where(Q, 10, pred, beam=33, hops=hops, n_seed=8)
            ids, _, counts = db.index.search_graph_steered_batch(Q, 10, db.metric, allowed, hops=hops, beam=33, n_seed=8)
            assert got == {b: {int(i): "doc %d" % (int(i) - 5) for i in ids[b, :counts[b]]} for b in range(5)}
            assert all(len(v) == 10 and all(pred(doc) for doc in v.values()) for v in got.values())
        before = db.index.search_graph_steered_info()
        blind = db.query_vectors_graph_where(Q, 10, pred, beam=33, n_seed=8)  # hops=0: today's call
        ids, _, counts = db.index.search_graph_filtered_batch(Q, 10, db.metric, allowed, beam=33, n_seed=8)
        assert blind == {b: {int(i): "doc %d" % (int(i) - 5) for i in ids[b, :counts[b]]} for b in range(5)}
        assert db.index.search_graph_steered_info() == before
        assert db.query_vectors_graph_where(Q, 10, lambda doc: False, beam=33, hops=2) == {b: {} for b in range(5)}
    finally:
        db.index.close()


# ---------------------------------------------------------------- more queries than one launch takes
def test_more_queries_than_one_launch(za):
    """ZH_GRAPH_BATCH + 1 queries on a 64-row table: two launches, the counters summed over both, the last query answered like the first"""
    n, d, g_k = 64, 30, 4
    X = rc.table(n, d, block=False)
    live = np.ones(n, bool)
    ix = make(za, X, live, 0)
    try:
        graph = rc.g_ring(n, g_k, live, 0)
        ix.set_graph(graph)
        m, om, omode = thirteen_metrics(za)[0]
        words, n_bits = fc.bitmap(np.arange(n) % 3 == 0)
        blk = 33
        Qb = zo.synth_queries(blk, d, n)
        sb = np.random.default_rng(0x5EA37).integers(0, n, (blk, 4)).astype(np.uint64)
        ref, rinfo = sc.reference(X, graph, n, g_k, live, 0, Qb, sb, 3, 8, 2, 0, om, omode, words, n_bits, 2)
        b = sc.GRAPH_BATCH + 1
        at = np.arange(b) % blk
        got = ix.search_graph_steered_batch(np.ascontiguousarray(Qb[at]), 3, m, mask_of(words, n_bits), hops=2, beam=8, width=2,
                                            seeds=np.ascontiguousarray(sb[at]))
        info = ix.search_graph_steered_info()
        same(got, tuple(a[at] for a in ref), "row i is the block's row i mod 33")
        assert info["launches"] == 2 and info["queries"] == b and info["rows_allowed"] == rinfo["rows_allowed"] and rinfo["via_bridge"] > 0
        assert info["returned"] == int(got[2].sum())
        whole, rest = divmod(b, blk)
        one = sc.reference(X, graph, n, g_k, live, 0, Qb[:rest], sb[:rest], 3, 8, 2, 0, om, omode, words, n_bits, 2)[1]
        for f in ("seeds", "iterations", "expanded", "keyed", "capped", "direct", "via_bridge", "bridges", "cand_full", "returned"):
            assert info[f] == whole * rinfo[f] + one[f], f
    finally:
        ix.close()


# ---------------------------------------------------------------- a caller's stream with work pending
def test_the_device_entry_on_a_callers_stream_with_work_pending(za):
    """tests/test_gpu_caller_stream.py's protocol for this call: the buffers hold a different valid input (the queries rolled by one, other seeds,
    the complement of the filter) and the outputs a sentinel; on a side stream a delay, then the real inputs and fills of every output with a
    second sentinel, are pending when the library is entered with stream = that stream.  The answer must be the host entry's, and the stream idle
    on return."""
    import torch
    ix, X, live, base = index("t600x128")
    ix.set_graph(gc.graph("t600x128", "exact", 32, base))
    m = thirteen_metrics(za)[0][0]
    b, n_seed, top_k = 16, 8, 10
    words, n_bits = fc.table_filter("t600x128", "even")
    Q, seeds = gc.queries("t600x128", b), rand_seeds("t600x128", b, n_seed, 5)
    want = ix.search_graph_steered_batch(Q, top_k, m, mask_of(words, n_bits), hops=2, beam=33, width=2, seeds=seeds)
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
    ix.search_graph_steered_batch_device(q.data_ptr(), b, sd.data_ptr(), n_seed, top_k, m, fw.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(),
                                         counts.data_ptr(), hops=2, beam=33, width=2, stream=S.cuda_stream)
    assert S.query(), "the call returned with work still pending on the caller's stream"
    with torch.cuda.stream(R):
        got = [t.to("cpu", non_blocking=True) for t in (ids, keys, counts)]
    R.synchronize()
    same((got[0].numpy().view(np.uint64), got[1].numpy().view(np.uint64), got[2].numpy().view(np.uint32)), want, "on the caller's stream")
    S.synchronize()

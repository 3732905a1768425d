"""Extending the attached graph on the device (zh_index_extend_graph, zh_index_get_graph): every case attaches a graph over the first G rows,
appends the rest, extends, and reads the whole table back; ids, counts and every info field equal the numpy reference (tests/gextend_cases.py,
pinned on the CPU by tests/test_gextend_reference.py), and the host and `_device` entries agree bit for bit.

A case's index is made for it: rows [0, G) appended, some removed, the graph attached, more old rows removed (rows that lines already name), rows
[G, N) appended, some of them removed.  Tables are gsearch_cases' (600 or 1500 rows; d = 30 generic, 128 and 256 specialised), 100 or 300 new rows."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gextend_cases as ge  # noqa: E402
from tests import gfilter_cases as fc  # noqa: E402
from tests import gsearch_cases as gc  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402

EINVAL, ESTATE, ELIMIT = -1, -4, -5


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def lib_metric(za, om, omode):
    return next(m for m, o, mode in thirteen_metrics(za) if (o, mode) == (om, omode))


def same_graph(got, want, what=""):
    for g, r, name in zip(got, want, ("ids", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        if not (g == r).all():
            at = np.argwhere(g != r)[0].tolist()
            raise AssertionError("%s %s: first difference at %s, got %d, want %d, %d differ" % (what, name, at, g[tuple(at)], r[tuple(at)], int((g != r).sum())))


def remove(ix, rows, base):
    rows = np.asarray(rows, np.int64)
    if rows.size:
        assert ix.remove(rows.astype(np.uint64) + np.uint64(base)).size == rows.size


def prepared(za, case, trees=False):
    """the case's index up to the extension -> (ix, X, live now)"""
    tname, G, variant, _, g_k, _, _, _, base, _ = case
    X, live0, live1, g, _, _ = ge.inputs(case)
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 3), device=0, id_base=base)
    add = ix.add if trees else ix.append
    if G:
        add(X[:G])
    remove(ix, np.flatnonzero(~live0[:G]), base)
    ix.set_graph(g)
    assert ix.graph_info()["g_rows"] == G
    remove(ix, np.flatnonzero(live0[:G] & ~live1[:G]), base)
    add(X[G:])
    remove(ix, G + np.flatnonzero(~live1[G:]), base)
    return ix, X, live1


def extend_device(ix, seeds, m, beam, width, max_iters, batch, stream=None):
    import torch
    sd = torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ix.extend_graph_device(sd.data_ptr(), seeds.shape[0], seeds.shape[1], m, beam=beam, width=width, max_iters=max_iters, batch=batch, stream=stream)


def get_device(ix, first_row, n, g_k, stream=None):
    import torch
    ids = torch.full((n, g_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ix.get_graph_device(first_row, n, ids.data_ptr(), counts.data_ptr(), stream=stream)
    return ids.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def run(za, case, what):
    """the host entry on one index, the device entry on its twin, both against the reference -> the host entry's index (extended)"""
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    seeds = ge.inputs(case)[5]
    _, rinfo, want = ge.expected(case)
    m = lib_metric(za, om, omode)
    N = want[0].shape[0]
    ix, X, live = prepared(za, case)
    info = ix.extend_graph(m, beam=beam, width=width, max_iters=max_iters, seeds=seeds, batch=batch)
    print(what, info)
    got = ix.get_graph()
    same_graph(got, want, what)
    assert info == rinfo == ix.extend_graph_info(), (what, info, rinfo)
    assert ix.graph_info() == {"attached": 1, "g_k": g_k, "g_rows": N, "bytes": ix.graph_info()["bytes"]} and ix.graph_info()["bytes"] >= 4 * N * g_k
    tw, _, _ = prepared(za, case)
    extend_device(tw, seeds, m, beam, width, max_iters, batch)
    assert tw.extend_graph_info() == rinfo, (what, "device entry")
    same_graph(get_device(tw, 0, N, g_k), got, what + " (device entries)")
    same_graph(tw.get_graph(37, N - 50), (got[0][37:N - 13], got[1][37:N - 13]), what + " (a slab)")
    tw.close()
    return ix


# ---------------------------------------------------------------- the definition, case by case
@pytest.mark.parametrize("name", sorted(ge.CASES))
def test_case(za, name):
    run(za, ge.CASES[name], name).close()


@pytest.mark.parametrize("mi", range(13))
def test_every_metric(za, mi):
    """all thirteen at the generic dimension, and at d = 128 where every kind has a specialised load"""
    _, om, omode = thirteen_metrics(za)[mi]
    run(za, ge.metric_case(om, omode), "metric %d" % mi).close()
    run(za, ge.metric_case(om, omode, "t600x128"), "metric %d d 128" % mi).close()


def test_d768(za):
    """the widest specialised load: 300 rows of 768, 60 of them new, under L2 and cosine"""
    n, G, d, g_k = 300, 240, 768, 8
    X = zo.synth_rows(n, d)
    live = np.ones(n, bool)
    live[[5, 17, 250]] = False
    for m, om, omode in thirteen_metrics(za)[:3:2]:
        K = ge.key_matrix(X, om, omode)
        g = gc.exact_graph(X[:G], g_k, live[:G], 0, zo.L2SQ, 0)
        seeds = ge.case_seeds("random", n - G, 8, G, n, 0)
        lines, rinfo = ge.extend(K, ge.kept_table(g, G, g_k, 0, G, live), live, 0, seeds, g_k, 16, 2, 0, 32)
        ix = za.LSHIndex(d, za.LSHIndexOptions(64, 3), device=0)
        ix.append(X[:G])
        remove(ix, [5, 17], 0)
        ix.set_graph(g)
        ix.append(X[G:])
        remove(ix, [250], 0)
        assert ix.extend_graph(m, beam=16, width=2, seeds=seeds, batch=32) == rinfo
        same_graph(ix.get_graph(), ge.graph_arrays(lines, g_k, 0), "d 768 metric %d" % om)
        ix.close()


# ---------------------------------------------------------------- what follows an extension
def test_two_extends_with_an_append_between(za):
    """extend [500, 550), append, extend [550, 600): the second call starts from the first one's table"""
    case = ge.CASES["batch7"]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    X, live0, live1, g, start, seeds = ge.inputs(case)
    K = ge.keys_of(tname, G, variant, om, omode)
    m = lib_metric(za, om, omode)
    mid = 550
    live_mid = live1[:mid]
    l1, i1 = ge.extend(K[:mid, :mid], start, live_mid, base, seeds[:mid - G], g_k, beam, width, max_iters, batch)
    l2, i2 = ge.extend(K, l1, live1, base, seeds[mid - G:], g_k, beam, width, max_iters, batch)
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 3), device=0, id_base=base)
    ix.append(X[:G])
    remove(ix, np.flatnonzero(~live0[:G]), base)
    ix.set_graph(g)
    remove(ix, np.flatnonzero(live0[:G] & ~live1[:G]), base)
    ix.append(X[G:mid])
    remove(ix, G + np.flatnonzero(~live1[G:mid]), base)
    assert ix.extend_graph(m, beam=beam, width=width, seeds=seeds[:mid - G], batch=batch) == i1
    same_graph(ix.get_graph(), ge.graph_arrays(l1, g_k, base), "first extend")
    ix.append(X[mid:])
    remove(ix, mid + np.flatnonzero(~live1[mid:]), base)
    assert ix.extend_graph(m, beam=beam, width=width, seeds=seeds[mid - G:], batch=batch) == i2
    same_graph(ix.get_graph(), ge.graph_arrays(l2, g_k, base), "second extend")
    assert ix.graph_info()["g_rows"] == X.shape[0]
    ix.close()


def test_round_trip_and_search_afterwards(za):
    """search_graph_batch and search_graph_filtered_batch over the extended graph equal gsearch_cases' / gfilter_cases' reference on the
    reference's table, and return appended rows; set_graph(get_graph()) attaches the same table less the entries that name rows removed since
    (set_graph masks them, the walk never saw them): the searches answer alike, and without removals the table is identical word for word"""
    case = ge.CASES["batch64"]
    tname, G, variant, _, g_k, (om, omode), _, _, base, _ = case
    _, _, want = ge.expected(case)
    m = lib_metric(za, om, omode)
    ix = run(za, case, "batch64")
    X, live = ge.inputs(case)[0], ge.inputs(case)[2]
    N = X.shape[0]
    planted = G + np.flatnonzero(live[G:])[:12]
    Q = np.ascontiguousarray(X[planted] + np.float32(1e-3))
    seeds = gc.default_seeds(Q.shape[0], 32, N, base)
    even = np.arange(N) % 2 == 0
    words, n_bits = fc.bitmap(even)
    for attempt in ("extended", "round trip"):
        got = ix.search_graph_batch(Q, 10, m, beam=64, width=2, seeds=seeds)
        ref, rinfo = gc.reference(X, want, N, g_k, live, base, Q, seeds, 10, 64, 2, 0, om, omode)
        for a, b, name in zip(got, ref, ("ids", "keys", "counts")):
            assert a.dtype == b.dtype and (a == b).all(), (attempt, name)
        assert ix.search_graph_info() == rinfo
        assert (got[0][:, 0] == planted.astype(np.uint64) + np.uint64(base)).all(), "every planted query finds its appended row first"
        gotf = ix.search_graph_filtered_batch(Q, 10, m, even, beam=64, width=2, seeds=seeds)
        reff, finfo = fc.reference(X, want, N, g_k, live, base, Q, seeds, 10, 64, 2, 0, om, omode, words, n_bits)
        for a, b, name in zip(gotf, reff, ("ids", "keys", "counts")):
            assert a.dtype == b.dtype and (a == b).all(), (attempt, "filtered", name)
        assert ix.search_graph_filtered_info() == finfo
        rows = gotf[0][gotf[0] != ge.NONE] - np.uint64(base)
        assert (rows >= G).any() and (rows % 2 == 0).all()
        ix.set_graph(ix.get_graph())  # the round trip
        same_graph(ix.get_graph(), ge.graph_arrays(ge.kept_table(want, N, g_k, base, N, live), g_k, base), "round trip")
    ix.close()
    case = ge.CASES["empty_start"]  # nothing removed: identical
    ix = run(za, case, "empty_start")
    ix.set_graph(ix.get_graph())
    same_graph(ix.get_graph(), ge.expected(case)[2], "round trip without removals")
    ix.close()


def test_lsh_seeds_and_the_database(za):
    """seeds="lsh" are search_batch's ids of the new rows read back; Database.extend_graph makes added records findable"""
    case = ge.CASES["batch64"]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    m = lib_metric(za, om, omode)
    ix, X, live = prepared(za, case, trees=True)
    N = X.shape[0]
    seeds = ix.search_batch(ix.read_rows(G, N - G), n_seed, m)[0]
    lines, rinfo = ge.extend(ge.keys_of(tname, G, variant, om, omode), ge.inputs(case)[4], live, base, seeds, g_k, beam, width, max_iters, batch)
    assert ix.extend_graph(m, beam=beam, width=width, seeds="lsh", n_seed=n_seed, batch=batch) == rinfo
    same_graph(ix.get_graph(), ge.graph_arrays(lines, g_k, base), "lsh seeds")
    ix.close()
    # the database: records inserted after build_graph are out of the walk's reach until extend_graph
    db = za.Database(30, za.L2SquaredDistance(), za.LSHIndexOptions(64, 3), device=0)
    db.insert_records(X[:G], ["old %d" % i for i in range(G)])
    db.build_graph(k=8, rounds=2)
    db.insert_records(X[G:], ["new %d" % i for i in range(N - G)])
    found = lambda: [doc for hits in db.query_vectors_graph(X[G:G + 20], 5).values() for doc in hits.values()]  # noqa: E731
    assert found() and not any(doc.startswith("new") for doc in found())
    info = db.extend_graph()
    assert info["rows_added"] == N - G and info["reverse_kept"] > 0 and db.index.graph_info()["g_rows"] == N
    assert sum(doc.startswith("new") for doc in found()) >= 20
    db.index.close()


def test_default_seeds_are_the_strided_rows_of_the_old_graph(za):
    case = ge.CASES["t1500_batch64"]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    ix, X, _ = prepared(za, case)
    info = ix.extend_graph(lib_metric(za, om, omode), beam=beam, width=width, n_seed=n_seed, batch=batch)  # seeds=None
    assert info == ge.expected(case)[1]
    same_graph(ix.get_graph(), ge.expected(case)[2], "default seeds")
    ix.close()


# ---------------------------------------------------------------- status and lifecycle
def test_status_and_lifecycle(za):
    case = ge.CASES["batch64"]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    X, _, _, g, _, seeds = ge.inputs(case)
    m = lib_metric(za, om, omode)
    N = X.shape[0]
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 3), device=0, id_base=base)
    ix.append(X[:G])
    for call in (lambda: ix.extend_graph(m), lambda: ix.get_graph(0, 1), lambda: get_device(ix, 0, 1, 4)):  # no graph
        with pytest.raises(za.ZhError) as e:
            call()
        assert e.value.code == ESTATE
    ix.set_graph(g)
    zero = dict.fromkeys(ge.INFO_FIELDS, 0)
    assert ix.extend_graph(m) == zero and ix.graph_info()["g_rows"] == G  # N == G: nothing done
    before = ix.get_graph()
    ix.append(X[G:])
    for n_new in (N - G - 1, N - G + 1, 0):  # the table changed between the caller's sizing and the call
        with pytest.raises(za.ZhError) as e:
            ix.extend_graph_device(ctypes.cast((ctypes.c_uint64 * 8)(), ctypes.c_void_p), n_new, 4, m)
        assert e.value.code == EINVAL and "n_new" in str(e.value)
    with pytest.raises(za.ZhError) as e:
        ix.extend_graph(m, beam=g_k - 1, seeds=seeds)
    assert e.value.code == ELIMIT and "g_k" in str(e.value)
    with pytest.raises(za.ZhError) as e:
        ix.extend_graph(m, beam=64, width=9, seeds=seeds)
    assert e.value.code == ELIMIT and "width" in str(e.value)
    for first, n in ((0, G + 1), (G, 1), (G + 1, 0)):
        with pytest.raises(za.ZhError) as e:
            ix.get_graph(first, n)
        assert e.value.code == EINVAL
    assert ix.get_graph(G, 0)[0].shape == (0, g_k)
    same_graph(ix.get_graph(), before, "a refused call leaves what was attached")
    assert ix.graph_info()["g_rows"] == G
    ix.extend_graph(m, seeds=seeds, beam=beam, width=width, batch=batch)
    assert ix.graph_info()["g_rows"] == N
    ix.remove(np.array([base + 1], np.uint64))
    ix.compact()  # rows move: the extended graph goes as any attached graph does
    assert ix.graph_info()["attached"] == 0
    ix.set_graph((np.zeros((ix.stored_rows(), 2), np.uint64), np.zeros(ix.stored_rows(), np.uint32)))
    ix.clear()
    assert ix.graph_info()["attached"] == 0
    ix.close()


# ---------------------------------------------------------------- the caller's stream
def test_device_entries_on_a_callers_stream_with_work_pending(za):
    """tests/test_gpu_caller_stream.py's protocol for the two device entries: the seed buffer holds a valid but different input (no seed in range),
    the real seeds wait in a staging tensor; on the side stream a delay, the copy of the real seeds, fills of get_graph's outputs with a second
    sentinel; the stream is busy when the calls are made with it; the answers are the reference's"""
    import torch
    case = ge.CASES["batch64"]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, base, _ = case
    seeds = ge.inputs(case)[5]
    _, rinfo, want = ge.expected(case)
    m = lib_metric(za, om, omode)
    N = want[0].shape[0]
    ix, _, _ = prepared(za, case)
    S = torch.cuda.Stream()
    real = torch.from_numpy(np.ascontiguousarray(seeds).view(np.int64)).cuda()
    buf = torch.full_like(real, -1)  # 2^64 - 1: out of range
    ids = torch.full((N, g_k), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    counts = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for cycles in (2_000_000, 20_000_000):  # the delay's cycles by event timing: 40 ms
        with torch.cuda.stream(S):
            e[0].record(S)
            torch.cuda._sleep(cycles)
            e[1].record(S)
        S.synchronize()
        per_ms = cycles / max(e[0].elapsed_time(e[1]), 1e-3)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(40 * per_ms))
        buf.copy_(real, non_blocking=True)
        ids.fill_(0x3C3C3C3C)
        counts.fill_(0x3C3C3C3C)
    assert not S.query(), "the side stream drained before the call: the delay is too short to show anything"
    ix.extend_graph_device(buf.data_ptr(), N - G, n_seed, m, beam=beam, width=width, max_iters=max_iters, batch=batch, stream=S.cuda_stream)
    ix.get_graph_device(0, N, ids.data_ptr(), counts.data_ptr(), stream=S.cuda_stream)
    assert S.query(), "complete on return"
    assert ix.extend_graph_info() == rinfo
    same_graph((ids.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)), want, "caller's stream")
    ix.close()

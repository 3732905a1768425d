"""The seams between a family's host entry point and its `_device` twin that the family suites do not reach: the range and forest range
searches' `_device` calls with no query, on an index without live rows, with capacity 0 and across the internal batch of 1024 queries; the two
graphs' host staging across its slab of lines; and the retry and count patterns of the Python wrappers.

The `_device` call has no staging loop and the host call has no caller's arrays on the device, so each is the other's check: every comparison
between the two is bit for bit.  The references are tests/family_cases.py's, over the oracle's keys.  Shapes are the smallest that reach each seam:
1030 queries cross the internal batch, 65 536 + 16 lines cross the host slab of either graph (the forest graph's is 65 536 lines from k = 257 on)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import family_cases as fc  # noqa: E402

ELIMIT, ESTATE, EINVAL = -5, -4, -1
JUNK = 0x5A5A5A5A5A5A5A5A  # (positive as int64)
SPEC = fc.metric_spec("l2sq")
KNN_HOST_SLAB = 65536  # lines the exact graph's host call stages at a time
FKNN_SLAB = 65536      # the forest graph's sub-slab; its host call stages max(FKNN_SLAB, 2^25 / k / FKNN_SLAB * FKNN_SLAB) lines at a time


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def P(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------- range and frange
@functools.lru_cache(maxsize=None)
def small_rows():
    return zo.synth_rows(1500, 30)


def small_index(za, build=True):
    ix = za.LSHIndex(30, za.LSHIndexOptions(64, 4), device=0)
    ix.append(small_rows())
    if build:
        ix.build()
    return ix


@pytest.fixture(scope="module")
def small(za):
    ix = small_index(za)
    yield ix
    ix.close()


def host_call(ix, family, Q, mk, cap, arrays=True, fill=JUNK):
    """the host entry point itself -> (rc, offsets, ids, keys, total)"""
    from zebra_amd import _ffi
    m = ix_metric()
    b = Q.shape[0]
    off = np.full(b + 1, fill, np.uint64)
    ids, keys = np.full(max(cap, 1), fill, np.uint64), np.full(max(cap, 1), fill, np.uint64)
    total = C.c_uint64(fill)
    A = lambda x: P(x) if arrays else None  # noqa: E731
    if family == "range":
        rc = _ffi.lib().zh_search_range_batch(ix._h, P(Q), b, P(mk), m.metric, m.mode, cap, P(off), A(ids), A(keys), C.byref(total))
    else:
        rc = _ffi.lib().zh_search_range_forest_batch(ix._h, P(Q), b, P(mk), 1, m.metric, m.mode, cap, P(off), A(ids), A(keys), C.byref(total))
    return rc, off, ids[:cap], keys[:cap], int(total.value)


def device_call(torch, za, ix, family, Q, mk, cap, arrays=True, n_off=None):
    """the `_device` entry point on stream = NULL, every output pre-filled with JUNK -> (rc, offsets [n_off], ids, keys, total)"""
    dev = torch.device("cuda", 0)
    b = Q.shape[0]
    q = torch.from_numpy(np.array(Q)).to(dev)
    t = torch.from_numpy(np.array(mk).view(np.int64)).to(dev)
    full = lambda n: torch.full((n,), JUNK, dtype=torch.int64, device=dev)  # noqa: E731
    off, ids, keys, total = full(b + 1 if n_off is None else n_off), full(max(cap, 1)), full(max(cap, 1)), full(1)
    A = lambda x: x.data_ptr() if arrays else None  # noqa: E731
    torch.cuda.synchronize()
    rc = 0
    try:
        if family == "range":
            ix.search_range_batch_device(q.data_ptr() if b else None, b, t.data_ptr() if b else None, ix_metric(), cap, off.data_ptr(), A(ids), A(keys),
                                         total.data_ptr())
        else:
            ix.search_range_forest_batch_device(q.data_ptr() if b else None, b, t.data_ptr() if b else None, 1, ix_metric(), cap, off.data_ptr(), A(ids),
                                                A(keys), total.data_ptr())
    except za.ZhError as e:
        rc = e.code
    torch.cuda.synchronize()
    u = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    return rc, u(off), u(ids)[:cap], u(keys)[:cap], int(u(total)[0])


def ix_metric():
    import zebra_amd
    return zebra_amd.L2SquaredDistance()


def info_of(ix, family):
    return ix.range_info() if family == "range" else ix.range_forest_info()


@pytest.mark.parametrize("family", ["range", "frange"])
def test_device_call_without_a_query(za, torch, small, family):
    """b == 0 still reaches the device: offsets[0] and the total are zeroed on the stream, nothing else is written, the info says batch 0"""
    Q, mk = np.zeros((0, 30), np.float32), np.zeros(0, np.uint64)
    # an earlier call with a batch of its own, so that the info is seen to change
    host_call(small, family, np.ascontiguousarray(small_rows()[:3]), np.full(3, fc.ALL, np.uint64), 5000)
    assert info_of(small, family)["batch"] == 3
    rc, off, _, _, total = device_call(torch, za, small, family, Q, mk, 16, n_off=5)
    assert rc == 0 and off[0] == 0 and total == 0
    assert (off[1:] == np.uint64(JUNK)).all()
    assert info_of(small, family)["batch"] == 0
    # the host twin returns before the lock: it writes the same two values and leaves the info alone
    host_call(small, family, np.ascontiguousarray(small_rows()[:3]), np.full(3, fc.ALL, np.uint64), 5000)
    rc, off, _, _, total = host_call(small, family, Q, mk, 16)
    assert rc == 0 and off[0] == 0 and total == 0 and info_of(small, family)["batch"] == 3


@pytest.mark.parametrize("built", [True, False])
@pytest.mark.parametrize("family", ["range", "frange"])
def test_index_emptied_by_removals(za, torch, family, built):
    """no live row: b + 1 offsets of 0 and a total of 0 from either twin, and the forest search asks for no trees (no ZH_ESTATE) even on an index
    that was never built"""
    ix = small_index(za, build=built)
    try:
        assert ix.remove(np.arange(1500, dtype=np.uint64)).size == 1500 and len(ix) == 0
        Q = np.ascontiguousarray(zo.synth_queries(20, 30, 1500))
        mk = np.full(20, fc.ALL, np.uint64)
        want = fc.range_ref(fc.key_matrix(SPEC, small_rows(), Q), np.zeros(1500, bool), mk, 0)
        assert want[0].size == 21 and not want[0].any()
        for cap in (64, 0):
            rc, off, _, _, total = device_call(torch, za, ix, family, Q, mk, cap, arrays=cap > 0)
            assert rc == 0 and (off == want[0]).all() and total == 0, (rc, off, total)
            assert info_of(ix, family)["batch"] == 20 and info_of(ix, family)["rows_live"] == 0
            rc, off, _, _, total = host_call(ix, family, Q, mk, cap, arrays=cap > 0)
            assert rc == 0 and (off == want[0]).all() and total == 0, (rc, off, total)
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def many_queries():
    """the shape of test_gpu_range.test_many_batches: 1030 queries cross the internal batch of 1024; thresholds at each query's third key, and
    every row for query 1025 -> (Q, thresholds, the exact range search's reference)"""
    X = small_rows()
    Q = np.ascontiguousarray(zo.synth_queries(1030, 30, 1500))
    K = fc.key_matrix(SPEC, X, Q)
    mk = np.sort(K, axis=1)[:, 2].copy()
    mk[1025] = fc.ALL
    ref = fc.range_ref(K, np.ones(1500, bool), mk, 0)
    for a in (Q, mk) + ref:
        a.setflags(write=False)
    return Q, mk, ref


@pytest.mark.parametrize("family", ["range", "frange"])
def test_capacity_zero_with_null_arrays(za, torch, small, family):
    Q, mk, _ = many_queries()
    Q, mk = np.ascontiguousarray(Q[:20]), np.ascontiguousarray(mk[:20])
    h = host_call(small, family, Q, mk, 0, arrays=False)
    g = device_call(torch, za, small, family, Q, mk, 0, arrays=False)
    assert h[0] == ELIMIT and g[0] == ELIMIT
    assert h[4] > 0 and g[4] == h[4] and (g[1] == h[1]).all() and int(h[1][-1]) == h[4]
    if family == "range":
        assert (h[1] == fc.range_ref(fc.key_matrix(SPEC, small_rows(), Q), np.ones(1500, bool), mk, 0)[0]).all()


@pytest.mark.parametrize("family", ["range", "frange"])
def test_device_call_across_the_internal_batch(za, torch, small, family):
    Q, mk, ref = many_queries()
    if family == "range":
        want = ref
    else:  # the forest's answer is the exact one's among the visited leaves: the first queries against the oracle's walk, all of them as a subset
        vis = fc.visited_mask(small_rows(), 64, small.get_forest(), Q[:8], 1)
        want = fc.range_ref(fc.key_matrix(SPEC, small_rows(), Q[:8]), vis, mk[:8], 0)
    cap = int(ref[0][-1])
    h = host_call(small, family, Q, mk, cap)
    assert h[0] == 0 and h[4] == int(h[1][-1]) and info_of(small, family)["batch"] == 1030
    if family == "range":
        assert h[4] == cap and (h[1] == want[0]).all() and (h[2] == want[1]).all() and (h[3] == want[2]).all()
    else:
        n8 = int(want[0][-1])
        assert (h[1][:9] == want[0]).all() and (h[2][:n8] == want[1]).all() and (h[3][:n8] == want[2]).all()
        assert 0 < h[4] <= cap and (np.diff(h[1]) <= np.diff(ref[0])).all()
    g = device_call(torch, za, small, family, Q, mk, cap)
    n = h[4]
    assert g[0] == 0 and g[4] == n and info_of(small, family)["batch"] == 1030
    assert (g[1] == h[1]).all() and (g[2][:n] == h[2][:n]).all() and (g[3][:n] == h[3][:n]).all()
    # a capacity that ends inside the first internal batch: ZH_ELIMIT, and the second batch's offsets are still exact
    short = 100
    assert short < int(h[1][1024])
    for got in (device_call(torch, za, small, family, Q, mk, short), host_call(small, family, Q, mk, short)):
        assert got[0] == ELIMIT and got[4] == n and (got[1] == h[1]).all()


# ---------------------------------------------------------------------------------------------------------------- the graphs' host slab
GRAPH_ROWS = KNN_HOST_SLAB + 16
TAIL = np.arange(GRAPH_ROWS - 32, GRAPH_ROWS)  # lines 65 520 .. 65 551: sixteen before the slab's edge, sixteen after


@functools.lru_cache(maxsize=None)
def graph_rows():
    X = zo.synth_rows(GRAPH_ROWS, 16)  # (16: the smallest dimension the goldens use; no matrix-core path, so path 1 whatever the rule)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def tail_keys():
    return fc.key_matrix(SPEC, graph_rows(), graph_rows()[TAIL])


def device_graph(torch, ix, forest, k, n):
    dev = torch.device("cuda", 0)
    ids, keys = (torch.full((n, k), JUNK, dtype=torch.int64, device=dev) for _ in range(2))
    counts = torch.full((n,), JUNK & 0xFFFFFFFF, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    (ix.knn_graph_forest_device if forest else ix.knn_graph_device)(k, ix_metric(), 0, n, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    return ids.cpu().numpy().view(np.uint64), keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)


def check_graph(torch, ix, forest, k, mates=None):
    n = GRAPH_ROWS
    info = ix.knn_forest_info if forest else ix.knn_info
    host = (ix.knn_graph_forest if forest else ix.knn_graph)(k, ix_metric())
    assert host[0].shape == (n, k) and info()["lines"] == n and info()["path"] == 1
    dev = device_graph(torch, ix, forest, k, n)
    assert info()["lines"] == n
    for h, g, what in zip(host, dev, ("ids", "keys", "counts")):
        assert (h == g).all(), what
    want = fc.graph_ref(tail_keys(), TAIL, np.ones(n, bool), k, 0, mates=mates)
    for h, w, what in zip(host, want, ("ids", "keys", "counts")):
        assert (h[TAIL] == w).all(), what
    return host


def test_exact_graph_across_the_host_slab(za, torch):
    ix = za.LSHIndex(16, za.LSHIndexOptions(64, 2), device=0)
    try:
        ix.append(graph_rows())
        host = check_graph(torch, ix, False, 1)
        assert (host[2] == 1).all()
    finally:
        ix.close()


def test_forest_graph_across_the_host_slab(za, torch):
    k = 300
    assert max(FKNN_SLAB, (1 << 25) // 257 // FKNN_SLAB * FKNN_SLAB) == max(FKNN_SLAB, (1 << 25) // k // FKNN_SLAB * FKNN_SLAB) == 65536 < GRAPH_ROWS
    ix = za.LSHIndex(16, za.LSHIndexOptions(64, 2), device=0)
    try:
        ix.append(graph_rows())
        ix.build()
        mates = fc.mates_mask(fc.leaf_table(ix.get_forest(), GRAPH_ROWS), TAIL)
        host = check_graph(torch, ix, True, k, mates=mates)
        assert 0 < int(host[2].max()) < k  # (two leaves of at most 64 rows: every line ends before k, the rest is 2^64-1)
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------------------------- the wrappers' patterns
class StubLib:
    """the library with one entry point replaced: `name` answers `codes` in turn (the last one from then on) and reports `total` hits"""

    def __init__(self, real, name, codes, total):
        self.real, self.name, self.codes, self.total, self.caps = real, name, list(codes), total, []

    def __getattr__(self, attr):
        if attr != self.name:
            return getattr(self.real, attr)

        def call(*args):
            total, cap = args[-1], [a for a in args if isinstance(a, int)][-1]
            self.caps.append(cap)
            total._obj.value = self.total
            if "range" in self.name:  # (offsets: the argument before ids, keys and the total)
                off = args[-4]
                n = C.cast(off, C.POINTER(C.c_uint64))
                n[0], n[1] = 0, self.total
            return self.codes[min(len(self.caps), len(self.codes)) - 1]

        return call


WRAPPERS = {  # wrapper -> (entry point, its count twin, arrays of `capacity` u64 it returns)
    "search_range_batch": ("zh_search_range_batch", "range_count_batch", 2),
    "search_range_forest_batch": ("zh_search_range_forest_batch", "range_forest_count_batch", 2),
    "self_join": ("zh_self_join", "self_join_count", 3),
    "cross_join": ("zh_cross_join", "cross_join_count", 3),
    "self_join_forest": ("zh_self_join_forest", "self_join_forest_count", 3),
}


def wrapper_call(small, other, name, count=False, **kw):
    m = ix_metric()
    f = getattr(small, WRAPPERS[name][1] if count else name)
    if "range" in name:
        return f(np.ascontiguousarray(small_rows()[:1]), metric=m, max_keys=np.uint64(7), **kw)
    if name == "cross_join":
        return f(other, metric=m, max_key=7, **kw)
    return f(metric=m, max_key=7, **kw)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_retries_once_and_counts(za, small, name, monkeypatch):
    from zebra_amd import _ffi, index
    entry, _, n_arrays = WRAPPERS[name]
    other = za.LSHIndex(30, za.LSHIndexOptions(64, 1), device=0)
    try:
        stub = lambda codes, total: StubLib(_ffi.lib(), entry, codes, total)  # noqa: E731
        # ZH_ELIMIT, then success: one more call, with the exact total as its capacity
        s = stub([ELIMIT, 0], 40)
        monkeypatch.setattr(index, "lib", lambda: s)
        got = wrapper_call(small, other, name, capacity=10)
        assert s.caps == [10, 40] and len(got) == 3 and all(a.shape == (40,) and a.dtype == np.uint64 for a in got[3 - n_arrays:])
        # the default capacity fits: one call
        s = stub([0], 40)
        monkeypatch.setattr(index, "lib", lambda: s)
        wrapper_call(small, other, name)
        assert s.caps == [1024 if "range" in name else max(1024, 16 * 1500)]
        # ZH_ELIMIT twice: the second one is raised, there is no third call
        s = stub([ELIMIT], 40)
        monkeypatch.setattr(index, "lib", lambda: s)
        with pytest.raises(za.ZhError) as e:
            wrapper_call(small, other, name, capacity=10)
        assert e.value.code == ELIMIT and s.caps == [10, 40]
        # ZH_ELIMIT with a total the capacity holds is no reason to retry; any other error is raised at once
        for codes, total in (([ELIMIT], 5), ([EINVAL], 40)):
            s = stub(codes, total)
            monkeypatch.setattr(index, "lib", lambda: s)
            with pytest.raises(za.ZhError) as e:
                wrapper_call(small, other, name, capacity=10)
            assert e.value.code == codes[0] and s.caps == [10]
        # the count call: capacity 0, ZH_ELIMIT is its ordinary answer, anything else is raised
        for code in (ELIMIT, 0):
            s = stub([code], 40)
            monkeypatch.setattr(index, "lib", lambda: s)
            n = wrapper_call(small, other, name, count=True)
            assert s.caps == [0] and (n.tolist() == [40] if "range" in name else n == 40)
        s = stub([ESTATE], 40)
        monkeypatch.setattr(index, "lib", lambda: s)
        with pytest.raises(za.ZhError) as e:
            wrapper_call(small, other, name, count=True)
        assert e.value.code == ESTATE and s.caps == [0]
    finally:
        monkeypatch.undo()
        other.close()

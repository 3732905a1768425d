"""tests/reverse_cases.py pinned on the CPU: the pair hash's known answers, its numpy reference against a literal Python-loop restatement of
zh_knn_graph_reverse's and zh_knn_graph_refine_rev's definitions on a 60-row table, rev_k = 0 against tests/refine_cases.py, and the properties
the extra input graphs are listed for.  No GPU, no library."""
import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import refine_cases as rc
from tests import reverse_cases as rv
from tests.test_refine_reference import ID_BASE, N, NONE, small


def test_hash_known_answers():
    for u, x, want in ((0, 0, 0x92CA2F0E), (1, 0, 0x96A0F96B), (0, 1, 0x3CD6E3F3), (12345, 678, 0x44199268), (0xFFFFFFFE, 0xFFFFFFFE, 0xB93EA14D)):
        assert int(rv.h(u, x)) == want, (u, x, hex(int(rv.h(u, x))))
    got = rv.h(np.array([0, 1, 12345]), np.array([0, 0, 678]))
    assert got.tolist() == [0x92CA2F0E, 0x96A0F96B, 0x44199268]


def loop_hash(u, x):
    v = (u + 0x9E3779B9 * (x + 1)) % 2**32
    v ^= v >> 16
    v = v * 0x85EBCA6B % 2**32
    v ^= v >> 13
    v = v * 0xC2B2AE35 % 2**32
    v ^= v >> 16
    return v


def loop_sets(in_ids, in_counts, in_k, rev_k, live, id_base):
    """N', In, R' and B of every stored row, entry by entry, with Python sets"""
    stored = len(in_ids)

    def nset(x):
        s = set()
        for j in range(min(int(in_counts[x]), in_k)):
            e = int(in_ids[x][j])
            if id_base <= e < id_base + stored and live[e - id_base]:
                s.add(e - id_base)
        return s

    Ns = [nset(x) for x in range(stored)]
    In = [{u for u in range(stored) if live[u] and u != x and x in Ns[u]} for x in range(stored)]
    R = [[u for _, u in sorted((loop_hash(u, x), u) for u in In[x] - Ns[x])[:rev_k]] for x in range(stored)]
    B = [Ns[x] | set(R[x]) for x in range(stored)]
    return Ns, In, R, B


def loop_reference_rev(X, in_ids, in_counts, in_k, rev_k, k, live, id_base, om, omode, first_row, n):
    Ns, In, R, B = loop_sets(in_ids, in_counts, in_k, rev_k, live, id_base)
    ids, keys, counts = [], [], []
    lines = listed = keyed = updates = 0
    for a in range(first_row, first_row + n):
        if not live[a]:
            ids.append([NONE] * k); keys.append([NONE] * k); counts.append(0)
            continue
        lines += 1
        c = set(B[a])
        listed += len(B[a])
        for u in B[a]:
            listed += len(B[u])
            c |= B[u]
        c.discard(a)
        keyed += len(c)
        order = sorted((zo.distance(om, omode, X[b], X[a]), b) for b in c)[:k]
        updates += sum(1 for _, b in order if b not in Ns[a])
        ids.append([id_base + b for _, b in order] + [NONE] * (k - len(order)))
        keys.append([key for key, _ in order] + [NONE] * (k - len(order)))
        counts.append(len(order))
    info = {"lines": lines, "listed": listed, "keyed": keyed, "updates": updates, "rev_k": rev_k, "edges": sum(len(s) for s in In) if rev_k else 0,
            "kept": sum(len(R[x]) for x in range(first_row, first_row + n)) if rev_k else 0, "max_degree": max(len(s) for s in In) if rev_k else 0}
    return (np.array(ids, np.uint64).reshape(n, k), np.array(keys, np.uint64).reshape(n, k), np.array(counts, np.uint32)), info


def small_graph(name, in_k, live):
    fn = rv.ALL_GRAPHS[name]
    return fn(N, in_k, live, ID_BASE, block=(20, 26)) if name == "block" else fn(N, in_k, live, ID_BASE)


@pytest.mark.parametrize("name", sorted(rv.ALL_GRAPHS))
@pytest.mark.parametrize("in_k,rev_k", [(1, 1), (5, 3), (8, 64)])
def test_reverse_reference_is_the_definition(name, in_k, rev_k):
    _, live = small()
    graph = small_graph(name, in_k, live)
    assert graph[0].shape == (N, in_k) and graph[0].dtype == np.uint64 and graph[1].shape == (N,) and graph[1].dtype == np.uint32
    _, In, R, _ = loop_sets(graph[0].tolist(), graph[1].tolist(), in_k, rev_k, live, ID_BASE)
    for first_row, n in ((0, N), (7, 31)):
        (ids, counts, degree), info = rv.reference_reverse(graph, in_k, rev_k, live, ID_BASE, first_row, n)
        assert ids.dtype == np.uint64 and ids.shape == (n, rev_k) and counts.dtype == np.uint32 and degree.dtype == np.uint32
        for i in range(n):
            x = first_row + i
            assert ids[i].tolist() == [ID_BASE + u for u in R[x]] + [NONE] * (rev_k - len(R[x])), x
            assert counts[i] == len(R[x]) and degree[i] == len(In[x])
        assert info == {"lines": int(live[first_row:first_row + n].sum()), "edges": sum(len(s) for s in In),
                        "kept": sum(len(R[first_row + i]) for i in range(n)), "max_degree": max(len(s) for s in In)}
    assert all(len(In[x]) == 0 for x in range(N) if not live[x])  # (N' never names a removed row)


@pytest.mark.parametrize("name", sorted(rv.ALL_GRAPHS))
@pytest.mark.parametrize("in_k,rev_k", [(1, 1), (5, 3), (8, 4)])
def test_fused_reference_is_the_definition(name, in_k, rev_k):
    X, live = small()
    graph = small_graph(name, in_k, live)
    for om, omode in ((zo.L2SQ, 0), (zo.COSINE, zo.PARITY)):
        for k, first_row, n in ((4, 0, N), (70, 7, 31)):
            got, info = rv.reference_rev(X, graph, in_k, rev_k, k, live, ID_BASE, om, omode, first_row, n)
            ref, rinfo = loop_reference_rev(X, graph[0].tolist(), graph[1].tolist(), in_k, rev_k, k, live, ID_BASE, om, omode, first_row, n)
            assert info == rinfo
            for g, r in zip(got, ref):
                assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all()


@pytest.mark.parametrize("name", sorted(rv.ALL_GRAPHS))
def test_rev_k_zero_is_the_forward_reference(name):
    X, live = small()
    graph = small_graph(name, 5, live)
    got, info = rv.reference_rev(X, graph, 5, 0, 6, live, ID_BASE, zo.L2SQ, 0, 3, 50)
    ref, rinfo = rc.reference(X, graph, 5, 6, live, ID_BASE, zo.L2SQ, 0, 3, 50)
    for g, r in zip(got, ref):
        assert (g == r).all()
    assert info == dict(rinfo, rev_k=0, edges=0, kept=0, max_degree=0)


def test_candidates_with_reverse_hold_the_forward_ones():
    """C(a) is a subset of C_r(a): position by position the reverse reference's (key, id) is never above the forward one's"""
    X, live = small()
    graph = rv.g_orphan(N, 5, live, ID_BASE)
    C, _, keyed, _ = rc.candidates(graph[0], graph[1], 5, live, ID_BASE)
    Cr, _, keyed_r, _, _, _ = rv.candidates_rev(graph[0], graph[1], 5, 3, live, ID_BASE)
    assert all(np.isin(c, cr).all() for c, cr in zip(C, Cr)) and keyed_r.sum() > keyed.sum()
    fwd, _ = rc.reference(X, graph, 5, 8, live, ID_BASE, zo.L2SQ, 0)
    rev, _ = rv.reference_rev(X, graph, 5, 3, 8, live, ID_BASE, zo.L2SQ, 0)
    for a in range(N):
        c = int(fwd[2][a])
        assert rev[2][a] >= c
        assert all((rev[1][a, j], rev[0][a, j]) <= (fwd[1][a, j], fwd[0][a, j]) for j in range(c))


def test_the_graphs_are_what_they_are_listed_for():
    n, base = 20000, 1000
    live = np.ones(n, bool)
    graph = rv.g_hub(n, 4, live, base)
    In = rv.in_neighbours(rc.neighbour_sets(graph[0], graph[1], 4, live, base), live)
    assert In[0].size == n - 1 and In[1].size == n - 1  # (every other row; a row never counts itself)
    _, info = rv.reference_reverse(graph, 4, 64, live, base, 0, 3)
    assert info["max_degree"] == n - 1 and info["kept"] >= 64
    n = 1500
    live = np.ones(n, bool)
    live[rc.removed_rows(n)] = False
    for in_k in (1, 5, 32, 64):
        graph = rv.g_mutual(n, in_k, live, base)
        (ids, counts, degree), info = rv.reference_reverse(graph, in_k, 8, live, base)
        assert info["kept"] == 0 and (ids == rv.NONE).all() and info["edges"] > 0 and (degree[live] >= 1).all()
    graph = rv.g_orphan(n, 5, live, base)
    Ns = rc.neighbour_sets(graph[0], graph[1], 5, live, base)
    In = rv.in_neighbours(Ns, live)
    orphans = np.flatnonzero(live)[:12]
    assert all(live[o] and Ns[o].size == 0 and In[o].size > 50 for o in orphans)
    fwd, _, _, _ = rc.candidates(graph[0], graph[1], 5, live, base)
    rev, _, _, _, _, _ = rv.candidates_rev(graph[0], graph[1], 5, 3, live, base)
    assert all(fwd[o].size == 0 and rev[o].size >= 3 for o in orphans)
    graph = rv.g_capped(n, 5, live, base)
    (ids, counts, degree), info = rv.reference_reverse(graph, 5, 8, live, base)
    targets = np.flatnonzero(live)[5:5 + len(rv.CAPPED_DEGREES)]
    assert degree[targets].tolist() == list(rv.CAPPED_DEGREES) and counts[targets].tolist() == [min(d, 8) for d in rv.CAPPED_DEGREES]
    assert info["edges"] == sum(rv.CAPPED_DEGREES)
    graph = rv.g_removed_namers(n, 5, live, base)
    named = (graph[0][~live] - np.uint64(base)).astype(np.int64)
    assert live[named].all() and (graph[1][~live] == 5).all()  # the removed rows' lines are full of live rows ...
    _, info = rv.reference_reverse(graph, 5, 8, live, base)
    assert info["edges"] == int(live.sum()) * 5  # ... and only the live rows' lines are counted

"""tests/refine_cases.py pinned on the CPU: its numpy reference against a literal Python-loop restatement of zh_knn_graph_refine's definition on a
60-row table, and the properties its input graphs are listed for.  No GPU, no library."""
import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import refine_cases as rc

N, D, ID_BASE = 60, 12, 1000
NONE = 2**64 - 1


def small():
    X = zo.synth_rows(N, D).copy()
    X[20:26] = X[20]  # ties by id
    live = np.ones(N, bool)
    live[[3, 10, 22, 59]] = False
    return X, live


def loop_reference(X, in_ids, in_counts, in_k, k, live, id_base, om, omode, first_row, n):
    """the definition, entry by entry, with Python sets and one oracle distance per pair"""
    stored = len(in_ids)

    def nset(x):
        s = set()
        for j in range(min(int(in_counts[x]), in_k)):
            e = int(in_ids[x][j])
            if e < id_base or e >= id_base + stored:
                continue
            if not live[e - id_base]:
                continue
            s.add(e - id_base)
        return s

    ids, keys, counts = [], [], []
    lines = listed = keyed = updates = 0
    for a in range(first_row, first_row + n):
        if not live[a]:
            ids.append([NONE] * k); keys.append([NONE] * k); counts.append(0)
            continue
        lines += 1
        na = nset(a)
        c = set(na)
        listed += len(na)
        for u in na:
            nu = nset(u)
            listed += len(nu)
            c |= nu
        c.discard(a)
        keyed += len(c)
        order = sorted((zo.distance(om, omode, X[b], X[a]), b) for b in c)[:k]
        updates += sum(1 for _, b in order if b not in na)
        ids.append([id_base + b for _, b in order] + [NONE] * (k - len(order)))
        keys.append([key for key, _ in order] + [NONE] * (k - len(order)))
        counts.append(len(order))
    return (np.array(ids, np.uint64).reshape(n, k), np.array(keys, np.uint64).reshape(n, k), np.array(counts, np.uint32)), \
        {"lines": lines, "listed": listed, "keyed": keyed, "updates": updates}


@pytest.mark.parametrize("name", sorted(rc.GRAPHS))
@pytest.mark.parametrize("in_k", [1, 5, 8])
def test_reference_is_the_definition(name, in_k):
    X, live = small()
    fn = rc.GRAPHS[name]
    graph = fn(N, in_k, live, ID_BASE, block=(20, 26)) if name == "block" else fn(N, in_k, live, ID_BASE)
    assert graph[0].shape == (N, in_k) and graph[0].dtype == np.uint64 and graph[1].shape == (N,) and graph[1].dtype == np.uint32
    for om, omode in ((zo.L2SQ, 0), (zo.COSINE, zo.PARITY)):
        for k, first_row, n in ((4, 0, N), (70, 7, 31)):
            got, info = rc.reference(X, graph, in_k, k, live, ID_BASE, om, omode, first_row, n)
            ref, rinfo = loop_reference(X, graph[0].tolist(), graph[1].tolist(), in_k, k, live, ID_BASE, om, omode, first_row, n)
            assert info == rinfo
            for g, r in zip(got, ref):
                assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all()


def test_key_rows_serve_ranked():
    X, live = small()
    graph = rc.g_self_loops(N, 5, live, ID_BASE)
    K = rc.key_rows(X, zo.L2, 0, range(N))
    a, _ = rc.reference(X, graph, 5, 9, live, ID_BASE, zo.L2, 0)
    b, _ = rc.reference(X, graph, 5, 9, live, ID_BASE, zo.L2, 0, K=K)
    for g, r in zip(a, b):
        assert (g == r).all()


def test_the_graphs_are_what_they_are_listed_for():
    n = 4200
    live = np.ones(n, bool)
    for in_k in (44, 64):  # every slot a line can gather: 1980 of the small instantiation's 2048, 4160 of the large one's 8192
        ids, counts = rc.g_disjoint(n, in_k, live, 0)
        _, listed, keyed, _ = rc.candidates(ids, counts, in_k, live, 0)
        assert keyed[0] == in_k + in_k * in_k == listed[0] and keyed.max() == keyed[0]
    n, in_k = 1500, 32
    live[rc.removed_rows(n)] = False
    live = live[:n]
    base = 1000
    ids, counts = rc.g_same_rows(n, in_k, live, base)
    _, listed, keyed, N_ = rc.candidates(ids, counts, in_k, live, base)
    assert listed[live].min() == (in_k + 1) * in_k and keyed.max() == in_k and all(s.size == in_k for s in N_)
    ids, counts = rc.g_repeats(n, in_k, live, base)
    assert max(s.size for s in rc.neighbour_sets(ids, counts, in_k, live, base)) <= 3
    ids, counts = rc.g_self_loops(n, in_k, live, base)
    C, _, _, N_ = rc.candidates(ids, counts, in_k, live, base)
    assert all(a in N_[a] and a not in C[a] for a in np.flatnonzero(live).tolist())
    ids, counts = rc.g_removed(n, in_k, live, base)
    named = ids[:, :] - np.uint64(base)
    assert (~live[named.astype(np.int64)]).mean() > 0.3 and all(live[s].all() for s in rc.neighbour_sets(ids, counts, in_k, live, base))
    ids, counts = rc.g_out_of_range(n, in_k, live, base)
    assert (ids < base).any() and (ids >= base + n).any() and (ids == base + n).any()
    ids, counts = rc.g_all_ones(n, in_k, live, base)
    assert (ids[:, -1] == rc.NONE).all() and (counts == in_k).all()
    ids, counts = rc.g_zero_counts(n, in_k, live, base)
    assert (counts == 0).mean() > 0.25 and all(s.size == 0 for s, c in zip(rc.neighbour_sets(ids, counts, in_k, live, base), counts) if c == 0)
    ids, counts = rc.g_big_counts(n, in_k, live, base)
    assert (counts > in_k).all()
    ids, counts = rc.g_ring(n, 1, live, base)
    assert (ids[:, 0] == (np.arange(n) + 1) % n + base).all()
    ids, counts = rc.g_block(n, in_k, live, base)
    r = (ids - np.uint64(base)).astype(np.int64)
    assert ((r >= rc.BLOCK[0]) & (r < rc.BLOCK[1])).mean() > 0.6
    X = rc.table(n, 30)
    assert (X[rc.BLOCK[0]:rc.BLOCK[1]] == X[rc.BLOCK[0]]).all() and not (X[rc.BLOCK[1]] == X[rc.BLOCK[0]]).all()


def test_rekeyed_input_is_never_below_the_answer():
    """N'(a) minus a is a subset of C(a): position by position the reference's (key, id) is never above that of the input line re-keyed"""
    X, live = small()
    graph = rc.g_zero_counts(N, 8, live, ID_BASE)
    got, _ = rc.reference(X, graph, 8, 8, live, ID_BASE, zo.L2SQ, 0)
    inp = rc.rekey(graph, 8, live, ID_BASE, X, zo.L2SQ, 0)
    for a, (iid, ikey) in inp.items():
        m = iid.size
        assert got[2][a] >= min(m, 8)
        assert all((got[1][a, j], got[0][a, j]) <= (ikey[j], iid[j]) for j in range(min(m, 8)))

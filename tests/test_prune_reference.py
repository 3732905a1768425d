"""tests/prune_cases.py pinned on the CPU: its numpy reference against a literal Python-loop restatement of zh_knn_graph_prune's definition on
refine_cases' 60-row table, the properties the header states, the behaviour of a block of identical rows from inside and from outside, and the
conditions under which the GPU tests' inputs exercise both branches of the rule.  No GPU, no library."""
import functools

import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import prune_cases as pc
from tests import refine_cases as rc
from tests import reverse_cases as rv
from tests.test_refine_reference import ID_BASE, N, small

NONE = 2**64 - 1
METRICS = [(zo.L2SQ, 0), (zo.COSINE, zo.PARITY), (zo.MANHATTAN, 0)]


def loop_reference(X, in_ids, in_counts, in_k, rev_k, degree, fill, live, id_base, om, omode, first_row, n):
    """the definition, entry by entry, with Python sets and one oracle distance per pair"""
    stored = len(in_ids)

    def nset(x):
        s = set()
        for j in range(min(int(in_counts[x]), in_k)):
            e = int(in_ids[x][j])
            if id_base <= e < id_base + stored and live[e - id_base]:
                s.add(e - id_base)
        return s

    def rset(x):
        inn = [u for u in range(stored) if live[u] and u != x and x in nset(u) and u not in nset(x)]
        return set(sorted(inn, key=lambda u: (int(rv.h(u, x)), u))[:rev_k])

    def key(q, x):
        return int(zo.distance(om, omode, X[x], X[q]))

    ids, keys, counts = [], [], []
    info = dict.fromkeys(pc.FIXED, 0)
    for a in range(first_row, first_row + n):
        line = []
        if live[a] and degree:
            cand = (nset(a) | (rset(a) if rev_k else set())) - {a}
            order = sorted((key(a, c), c) for c in cand)
            S, O, examined = [], [], 0
            for ka, c in order:
                if len(S) == degree:
                    break
                examined += 1
                if any(key(p, c) < ka for _, p in S):
                    O.append((ka, c))
                else:
                    S.append((ka, c))
            info["lines"] += 1
            info["candidates"] += len(order)
            info["kept"] += len(S)
            info["occluded"] += len(O)
            info["cut"] += int(len(S) == degree and examined < len(order))
            if fill and len(S) < degree:
                take = O[:degree - len(S)]
                info["filled"] += len(take)
                S = S + take
            line = sorted(S)
        ids.append([id_base + c for _, c in line] + [NONE] * (degree - len(line)))
        keys.append([k for k, _ in line] + [NONE] * (degree - len(line)))
        counts.append(len(line))
    return (np.array(ids, np.uint64).reshape(n, degree), np.array(keys, np.uint64).reshape(n, degree), np.array(counts, np.uint32)), info


def same(got, ref, what=""):
    for g, r, name in zip(got, ref, ("ids", "keys", "counts")):
        assert g.dtype == r.dtype and g.shape == r.shape and (g == r).all(), (what, name)


@pytest.mark.parametrize("om,omode", METRICS)
@pytest.mark.parametrize("graph", ["repeats", "self_loops", "removed", "out_of_range", "zero_counts", "block"])
def test_numpy_reference_is_the_definition(graph, om, omode):
    X, live = small()
    for in_k, rev_k in ((5, 0), (9, 4)):
        g = rc.GRAPHS[graph](N, in_k, live, ID_BASE, block=(20, 26)) if graph == "block" else rc.GRAPHS[graph](N, in_k, live, ID_BASE)
        prep = pc.prepare(X, g, in_k, rev_k, live, ID_BASE, om, omode)
        for degree, fill, first_row, n in ((3, 0, 0, N), (3, 1, 0, N), (1, 0, 7, 30), (13, 1, 0, N), (0, 1, 0, N)):
            got = pc.reference(prep, N, degree, fill, live, ID_BASE, first_row, n)
            want = loop_reference(X, g[0], g[1], in_k, rev_k, degree, fill, live, ID_BASE, om, omode, first_row, n)
            same(got[0], want[0], (graph, in_k, rev_k, degree, fill))
            assert got[1] == want[1], (graph, in_k, rev_k, degree, fill, got[1], want[1])


def test_the_candidates_are_the_reverse_calls():
    X, live = small()
    g = rc.g_ring(N, 3, live, ID_BASE)
    P, Nn, R = pc.candidate_sets(g, 3, 4, live, ID_BASE)
    (rid, rcount, _), _ = rv.reference_reverse(g, 3, 4, live, ID_BASE)
    for a in range(N):
        assert sorted(R[a].tolist()) == sorted((rid[a, :rcount[a]] - np.uint64(ID_BASE)).astype(np.int64).tolist())
        assert set(P[a].tolist()) == ((set(Nn[a].tolist()) | set(R[a].tolist())) - {a} if live[a] else set())


@pytest.mark.parametrize("om,omode", METRICS)
def test_properties(om, omode):
    """c_1 is always kept; fill at degree >= |P(a)| is P(a) re-keyed; fill = 0, rev_k = 0 is idempotent"""
    X, live = small()
    in_k = 12
    g = rc.g_zero_counts(N, in_k, live, ID_BASE)
    K = rc.key_rows(X, om, omode, range(N))
    prep = pc.prepare(X, g, in_k, 0, live, ID_BASE, om, omode, K)
    for degree in (1, 4, 12):
        (ids, keys, counts), info = pc.reference(prep, N, degree, 0, live, ID_BASE)
        for a in np.flatnonzero(live).tolist():
            c, ka, _ = prep[a]
            if c.size:
                assert counts[a] >= 1 and ids[a, 0] == np.uint64(ID_BASE + c[0]) and keys[a, 0] == ka[0]
            else:
                assert counts[a] == 0
        assert info["kept"] == int(counts.sum()) and info["filled"] == 0
        again = pc.reference(pc.prepare(X, (ids, counts), degree, 0, live, ID_BASE, om, omode, K), N, degree, 0, live, ID_BASE)
        same(again[0], (ids, keys, counts), "idempotent at degree %d" % degree)
        assert again[1]["occluded"] == 0 and again[1]["cut"] == 0
    (ids, keys, counts), info = pc.reference(prep, N, 64, 1, live, ID_BASE)
    inp = rc.rekey(g, in_k, live, ID_BASE, X, om, omode, K)
    for a, (iid, ikey) in inp.items():
        assert counts[a] == iid.size and (ids[a, :iid.size] == iid).all() and (keys[a, :iid.size] == ikey).all()
    assert info["kept"] + info["filled"] == info["candidates"] == int(counts.sum()) and info["filled"] == info["occluded"] and info["cut"] == 0


def test_a_block_of_identical_rows_from_inside_and_outside():
    X, live = small()  # rows 20 .. 25 identical, 22 removed
    g = pc.g_all_block(N, 5, live, ID_BASE, block=(20, 26))
    prep = pc.prepare(X, g, 5, 0, live, ID_BASE, zo.L2SQ, 0)
    (ids, keys, counts), info = pc.reference(prep, N, 5, 0, live, ID_BASE)
    block = [20, 21, 23, 24, 25]
    for a in block:  # inside: the other four, none occludes another, all at the key of a row against itself
        assert counts[a] == 4 and ids[a, :4].tolist() == [ID_BASE + b for b in block if b != a] and len(set(keys[a, :4].tolist())) == 1
    for a in (0, 19, 26, 58):  # outside: the lowest id of the five, which occludes the other four
        assert counts[a] == 1 and ids[a, 0] == ID_BASE + 20
        assert len(pc.walk(prep[a][1], prep[a][2], 5)[1]) == 4
    filled = pc.reference(prep, N, 5, 1, live, ID_BASE)[0]
    assert filled[2][0] == 5 and filled[0][0].tolist() == [ID_BASE + b for b in block]


def test_special_lines():
    X = pc.special_table()
    live = np.ones(pc.SPECIAL_ROWS, bool)
    for name, (line0, degs) in pc.SPECIAL.items():
        g = pc.special_graph(name)
        prep = pc.prepare(X, g, 64, 0, live, 0, zo.L2SQ, 0, rows=[0])
        c, ka, M = prep[0]
        S, O, examined = pc.walk(ka, M, 64)
        assert c.size == len(line0), name
        if name != "full64":  # nothing is occluded along the axes
            assert not O and len(S) == c.size, name
        if name == "ties":
            assert len(set(ka.tolist())) == 1
        if name == "full64":
            assert c.size == 64 and O and len(S) >= 2  # the widest line there is, with both branches taken
        if name == "axes":
            assert len(set(ka.tolist())) == 30
            for degree, cut in ((1, True), (29, True), (30, False), (31, False)):  # 30: degree reached on the last candidate
                S, _, examined = pc.walk(ka, M, degree)
                assert (len(S) == degree and examined < c.size) == cut and len(S) == min(degree, 30)


# ---------------------------------------------------------------- what the GPU tests' inputs exercise
@functools.lru_cache(maxsize=None)
def _exact(name):
    from tests.test_gpu_refine import TABLES
    n, d, base, block, removed, _ = TABLES[name]
    X = rc.table(n, d, block)
    live = np.ones(n, bool)
    if removed:
        live[rc.removed_rows(n)] = False
    K = rc.key_rows(X, zo.L2SQ, 0, range(n))
    return X, live, base, K, pc.exact_graph(K, live, base, 32)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_exact_graph_exercises_both_branches(name):
    """conditions, not measurements: at degree 16 at least half of the live lines have both an occluded candidate and a second kept one, and at
    degree 8 at least 20 lines are cut.  (On 600 synthetic rows under float64 L2 squared 99.7 % / 100 % of the lines had both at d = 30 / 256.)"""
    X, live, base, K, g = _exact(name)
    prep = pc.prepare(X, g, 32, 0, live, base, zo.L2SQ, 0, K)
    both = sum(1 for a in prep if (lambda S, O, _: len(S) >= 2 and len(O) >= 1)(*pc.walk(prep[a][1], prep[a][2], 16)))
    assert 2 * both >= int(live.sum()), (both, int(live.sum()))
    assert pc.reference(prep, live.size, 8, 0, live, base)[1]["cut"] >= 20

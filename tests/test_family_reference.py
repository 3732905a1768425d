"""tests/family_cases.py on the CPU: each reference against a literal Python-loop restatement of the README's definition of its family (scalar
oracle.distance, plain loops over rows, trees and leaves) on a tiny case; plan() is a pure function of the seed; the default seeds promise every
family on path 2 at every (D, KINDA), every family on path 1, every gate edge and every mutation; the planted rows give no NaN key."""
import json

import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import family_cases as fc

N, D, M, T, K_TOP, BASE, BASE_B = 60, 5, 8, 2, 4, 1 << 40, 77
SPECS = [fc.metric_spec("l2sq"), fc.metric_spec("l2"), fc.metric_spec("cos_parity"), fc.metric_spec("cos_corrected"), fc.metric_spec("manhattan"),
         fc.metric_spec("minkowski", 3)]


class Tiny:
    def __init__(self):
        X = zo.synth_rows(N, D, seed=11).copy()
        X[7] = X[3]                               # a bit-identical duplicate
        X[9] = X[4] * np.float32(1.0 + 2.0**-12)  # a near-duplicate
        self.X = X
        f = zo.Forest.build(X, M, T, seed=5)
        gone = np.array([2, 16, 17, 18, 40, N - 1], np.uint64)
        assert f.remove(gone).all()
        self.forest = f.arrays()
        self.alive = np.ones(N, bool)
        self.alive[gone.astype(np.int64)] = False
        self.Q = np.ascontiguousarray(np.concatenate([zo.synth_queries(5, D, N, seed_rows=11), X[3:4], np.zeros((1, D), np.float32)]), np.float32)
        self.XB = zo.synth_rows(23, D, seed=12).copy()
        self.XB[5] = X[3]
        self.aliveB = np.ones(23, bool)
        self.aliveB[[0, 11]] = False
        self.allowed = np.random.default_rng(3).random(N) < 0.7
        self.slab = np.arange(10, 24)  # rows 16, 17, 18 are removed

    def leaves(self, t):
        """the leaves of tree t as lists of row numbers, by a plain walk from the root"""
        f, out, stack = self.forest, [], [int(self.forest["roots"][t])]
        while stack:
            node = stack.pop()
            if f["plane"][node] < 0:
                out.append([int(r) for r in f["leaf_ids"][f["left"][node]:f["left"][node] + f["right"][node]]])
            else:
                stack += [int(f["left"][node]), int(f["right"][node])]
        return out


@pytest.fixture(scope="module")
def tiny():
    return Tiny()


def key(spec, row, q):
    return zo.distance(spec["om"], spec["omode"], row, q)


def csr(lines, base):
    off, ids, keys = [0], [], []
    for line in lines:
        ids += [r + base for _, r in line]
        keys += [k for k, _ in line]
        off.append(len(ids))
    return np.array(off, np.uint64), np.array(ids, np.uint64), np.array(keys, np.uint64)


def table(lines, k, base):
    ids, keys, counts = np.full((len(lines), k), fc.ALL, np.uint64), np.full((len(lines), k), fc.ALL, np.uint64), np.zeros(len(lines), np.uint32)
    for i, line in enumerate(lines):
        for j, (kk, r) in enumerate(line[:k]):
            ids[i, j], keys[i, j] = r + base, kk
        counts[i] = min(k, len(line))
    return ids, keys, counts


def triples(pairs, base_a, base_b):
    pairs = sorted(pairs)  # (a, key, b)
    return (np.array([a + base_a for a, _, _ in pairs], np.uint64), np.array([b + base_b for _, _, b in pairs], np.uint64),
            np.array([k for _, k, _ in pairs], np.uint64))


def equal(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all()


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: s["name"])
def test_references_against_literal_loops(tiny, spec):
    t = tiny
    X, alive = t.X, t.alive
    KQ = fc.key_matrix(spec, X, t.Q)
    # exact top-k, filtered top-k, range
    lines = [sorted((key(spec, X[r], q), r) for r in range(N) if alive[r]) for q in t.Q]
    equal(fc.topk_ref(KQ, alive, K_TOP, BASE), table(lines, K_TOP, BASE))
    equal(fc.topk_ref(KQ, alive, 100, BASE), table(lines, 100, BASE))  # k above the live rows
    flines = [sorted((key(spec, X[r], q), r) for r in range(N) if alive[r] and t.allowed[r]) for q in t.Q]
    equal(fc.topk_ref(KQ, alive & t.allowed, K_TOP, BASE), table(flines, K_TOP, BASE))
    thr = np.array([lines[i][min(3 * i, len(lines[i]) - 1)][0] for i in range(len(t.Q))], np.uint64)
    thr[1], thr[2] = 0, fc.ALL
    equal(fc.range_ref(KQ, alive, thr, BASE), csr([[e for e in line if e[0] <= int(thr[i])] for i, line in enumerate(lines)], BASE))
    # the self-join and the graph: the query is a stored row
    rows = np.arange(N)
    KX = fc.key_matrix(spec, X, X)
    pair_keys = sorted(key(spec, X[b], X[a]) for a in range(N) for b in range(a + 1, N) if alive[a] and alive[b])
    mk = pair_keys[40]
    pairs = [(a, key(spec, X[b], X[a]), b) for a in range(N) for b in range(a + 1, N) if alive[a] and alive[b] and key(spec, X[b], X[a]) <= mk]
    full = fc.join_ref(KX, rows, alive, alive, mk, BASE, BASE, True)
    equal(full, triples(pairs, BASE, BASE))
    some = [3, 4, 16, 30]  # (16 is removed: no pair starts there)
    equal(fc.join_ref(KX[some], some, alive, alive, mk, BASE, BASE, True), triples([p for p in pairs if p[0] in some], BASE, BASE))
    equal(fc.restrict(full, some, BASE), triples([p for p in pairs if p[0] in some], BASE, BASE))
    upper = alive[None, :] & (rows[None, :] > rows[:, None]) & alive[:, None]
    assert fc.quantile_threshold(KX, upper, 41, len(pair_keys)) == mk
    glines = [sorted((key(spec, X[r], X[a]), r) for r in range(N) if alive[r] and r != a) if alive[a] else [] for a in t.slab]
    equal(fc.graph_ref(KX[t.slab], t.slab, alive, K_TOP, BASE), table(glines, K_TOP, BASE))
    # the join between two indexes
    KB = fc.key_matrix(spec, t.XB, X)
    xk = sorted(key(spec, t.XB[b], X[a]) for a in range(N) for b in range(23) if alive[a] and t.aliveB[b])[25]
    xpairs = [(a, key(spec, t.XB[b], X[a]), b) for a in range(N) for b in range(23) if alive[a] and t.aliveB[b] and key(spec, t.XB[b], X[a]) <= xk]
    equal(fc.join_ref(KB, rows, alive, t.aliveB, xk, BASE, BASE_B, False), triples(xpairs, BASE, BASE_B))
    # the forest forms: leaf-mates from the forest's arrays, each pair once however many trees repeat it
    leaves = [t.leaves(tr) for tr in range(T)]
    leaf_of = fc.leaf_table(t.forest, N)

    def mates(a):
        out = set()
        for tr in range(T):
            for leaf in leaves[tr]:
                if a in leaf:
                    out.update(leaf)
        out.discard(a)
        return out

    flines = [sorted((key(spec, X[r], X[a]), r) for r in mates(int(a))) if alive[a] else [] for a in t.slab]
    equal(fc.graph_ref(KX[t.slab], t.slab, alive, K_TOP, BASE, mates=fc.mates_mask(leaf_of, t.slab)), table(flines, K_TOP, BASE))
    fpairs = set()
    for tr in range(T):
        for leaf in leaves[tr]:
            for a in leaf:
                for b in leaf:
                    if a < b:
                        fpairs.add((a, b))
    assert any(sum((a in leaf and b in leaf) for tr in range(T) for leaf in leaves[tr]) > 1 for a, b in fpairs)  # (a pair that two trees repeat)
    fk = sorted(key(spec, X[b], X[a]) for a, b in fpairs)[len(fpairs) // 2]
    want = triples([(a, key(spec, X[b], X[a]), b) for a, b in fpairs if key(spec, X[b], X[a]) <= fk], BASE, BASE)
    equal(fc.join_ref(KX, rows, alive, fc.mates_mask(leaf_of, rows), fk, BASE, BASE, True), want)
    ja, jb, jk = fc.join_ref(KX, rows, alive, alive, fk, BASE, BASE, True)  # the exact join's pairs that are leaf-mates: the same answer
    keep = fc.are_mates(leaf_of, ja - np.uint64(BASE), jb - np.uint64(BASE))
    equal((ja[keep], jb[keep], jk[keep]), want)
    # the forest range search: the members of the leaves the walk visits
    f = zo.Forest.from_arrays(X, M, t.forest)
    for probe in (1, 3):
        vis = fc.visited_mask(X, M, t.forest, t.Q, probe)
        vlines = []
        for i, q in enumerate(t.Q):
            cands = set()
            for tr in range(T):
                _, _, v = f.tree_result(tr, q, probe, zo.L2SQ, 0)
                for off, length, _ in v.tolist():
                    cands.update(int(r) for r in t.forest["leaf_ids"][int(off):int(off) + int(length)])
            assert all(alive[r] for r in cands)
            vlines.append([e for e in sorted((key(spec, X[r], q), r) for r in cands) if e[0] <= int(thr[i])])
        equal(fc.range_ref(KQ, vis, thr, BASE), csr(vlines, BASE))


def test_threshold_menu_and_compact_map(tiny):
    for spec in SPECS:
        K = fc.key_matrix(spec, tiny.X, np.concatenate([tiny.Q, tiny.X[:12]]))
        thr = fc.range_thresholds(K, tiny.alive, spec, np.random.default_rng(1))
        assert thr.dtype == np.uint64 and thr[4] == 0 and thr[5] == fc.ALL and thr[6] >= np.uint64(1 << 63 if spec["kinda"] is not None else 1 << 31)
        assert thr[0] == K[0, tiny.alive].min() and thr[3] == K[3, tiny.alive].max() and int(thr[7]) - 1 in K[7, tiny.alive].tolist()
    m = fc.compact_map(tiny.alive, BASE)
    assert (m[~tiny.alive] == fc.GONE).all() and (m[tiny.alive] == np.arange(tiny.alive.sum(), dtype=np.uint64) + np.uint64(BASE)).all()


def test_plan_is_a_pure_function_of_the_seed():
    for seed in list(fc.DEFAULT_SEEDS) + [1000, 12345]:
        a, b = fc.plan(seed), fc.plan(seed)
        assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)
        alive = fc.initial_alive(a)
        assert int(alive.sum()) == a["live_target"] and (alive == fc.initial_alive(b)).all()
        s1, s2 = fc.round_setup(a, 1, alive), fc.round_setup(b, 1, alive)
        assert all((np.asarray(s1[k]) == np.asarray(s2[k])).all() for k in ("allowed_arg", "allowed", "slab", "sample"))
        if not a["narrow"]:
            assert a["d"] in fc.MFMA_DIMS and a["n_rows"] % 16 and a["n_rows"] >= fc.GATE_ROWS + 300
            assert [m["kinda"] is not None for m in a["metrics"]] == [True, True, False]
        assert 1 <= a["B"] <= 25 and 0 <= s1["first_row"] <= a["n_rows"] - a["slab_lines"]
    assert json.dumps(fc.plan(1), sort_keys=True) != json.dumps(fc.plan(2), sort_keys=True)


def test_default_seeds_promise_the_coverage():
    path2, path1, edges, mutations, l2_seeds = fc.coverage(fc.DEFAULT_SEEDS)
    need = {(f, d, k) for f in fc.FAMILIES for d in fc.MFMA_DIMS for k in range(3)}
    assert need <= path2, sorted(need - path2)  # every family on path 2 at each of the 15 (D, KINDA)
    assert all(path1[f] >= 3 for f in fc.FAMILIES), path1
    assert edges == {"8192 live", "8191 live", "8192 allowed", "max_node_size 16", "natural 2^25 cross join"}, edges
    assert all(mutations[m] >= 2 for m in fc.MUTATIONS), mutations
    assert l2_seeds >= 4
    assert {m["name"] for s in fc.DEFAULT_SEEDS for m in fc.plan(s)["metrics"]} == set(fc.METRICS)  # all thirteen keys
    plans = [fc.plan(s) for s in fc.DEFAULT_SEEDS]
    assert 3 <= sum(p["narrow"] for p in plans) <= 5
    assert sum(bool(p["row_order"]) for p in plans) >= len([p for p in plans if not p["narrow"]]) // 3 - 1
    assert {"last", "removed"} <= {p["slab_at"] for p in plans}
    assert sum(p["B"] % 16 != 0 for p in plans) > len(plans) // 2


def test_expected_path_sits_on_the_gates():
    l2sq, man = fc.metric_spec("l2sq"), fc.metric_spec("manhattan")
    ep = fc.expected_path
    assert ep("exact", 256, l2sq, live=8192, k=10) == 2 and ep("exact", 256, l2sq, live=8191, k=10) == 1 and ep("exact", 200, l2sq, live=9000) == 1
    assert ep("exact", 256, man, live=9000) == 1 and ep("range", 1024, l2sq, live=8192) == 2 and ep("range", 1024, l2sq, 1, live=8192) == 1
    assert ep("join", 384, l2sq, live=8191) == 1 and ep("knn", 512, l2sq, live=8192, k=8192) == 1 and ep("knn", 512, l2sq, live=8192, k=100) == 2
    assert ep("filtered", 256, l2sq, live=9000, allowed=8192, k=1) == 2 and ep("filtered", 256, l2sq, live=9000, allowed=8191, k=1) == 1
    assert ep("filtered", 256, l2sq, live=9000, allowed=8192, k=1, tile_rule=False) == 1 and ep("filtered", 256, l2sq, 2, live=9000, allowed=8192, tile_rule=False) == 2
    assert ep("cross", 768, l2sq, live=8192, live_b=4096) == 2 and ep("cross", 768, l2sq, live=8191, live_b=4096) == 1 and ep("cross", 768, l2sq, 2, live=10, live_b=10) == 2
    assert ep("fknn", 256, l2sq, max_node_size=64) == 2 and ep("fjoin", 256, l2sq, max_node_size=16) == 1 and ep("frange", 256, l2sq, 2, max_node_size=64) == 2
    assert ep("frange", 256, l2sq, max_node_size=16) == 1
    scattered = np.zeros(16 * 1000, bool)
    scattered[::16] = True  # one allowed row per tile: every tile is loaded for a sixteenth of the rows
    assert not fc.filter_tile_rule(scattered) and fc.filter_tile_rule(np.ones(9000, bool))


@pytest.mark.parametrize("seed", list(fc.DEFAULT_SEEDS)[:4])
def test_no_reference_key_is_a_nan(seed):
    """the builder's own assertion, on the planted rows and queries of the first default seeds at a reduced row count"""
    p = dict(fc.plan(seed), n_rows=700, d=min(fc.plan(seed)["d"], 256))
    X = fc.build_rows(p)
    Q = np.concatenate([fc.build_queries(p, X), X[[0, 100, 200, 300, 400, 410, 500, 550]]])
    for spec in p["metrics"]:
        K = fc.key_matrix(spec, X, Q)
        assert K.shape == (Q.shape[0], 700) and not fc.key_is_nan(K, spec).any()
    with pytest.raises(AssertionError):  # and the assertion can fire: Canberra of the zero row against the zero query is 0 / 0
        Xz = X.copy()
        Xz[550] = 0.0
        fc.key_matrix(fc.metric_spec("canberra"), Xz, np.zeros((1, p["d"]), np.float32))

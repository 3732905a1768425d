"""The plain reference and the input graphs of the k-NN graph refinement tests (no GPU, no library: numpy and the oracle only).

zh_knn_graph_refine takes a graph over ALL stored rows -- in_ids [stored rows, in_k] u64 in the id space id_base + row, in_counts [stored rows] u32 --
and answers, for every live stored row a of a slab, the first k by (key, id) of

    C(a) = ( N'(a)  union  N'(u) for every u in N'(a) ) minus a

where N'(x) is the SET of live stored rows named by the first min(in_counts[x], in_k) entries of line x: entries out of range (2^64-1 included) or
naming a removed row are ignored, repetitions count once, order means nothing.  candidates() is that definition in numpy, ranked() is
tests/test_gpu_fknn.py's ranking (the oracle's distance_batch keys, a lexsort by (key, id)), reference() puts them together with the four info
fields the definition fixes: lines, listed, keyed, updates.  tests/test_refine_reference.py pins them against a Python-loop restatement on a
60-row table; tests/test_gpu_refine.py runs the library against them.

GRAPHS are the adversarial inputs, each listed because the kernel can get it wrong; every one is a pure function of (rows, in_k, live, id_base)
and a fixed seed."""
import concurrent.futures

import numpy as np

from oracle import zebra_oracle as zo

NONE = np.uint64(2**64 - 1)
SEED = 0x5EF1E


# ---------------------------------------------------------------------------------------------------------------- the definition
def neighbour_sets(in_ids, in_counts, in_k, live, id_base):
    """N'(x) of every stored row x, ascending int64 row numbers"""
    in_ids = np.asarray(in_ids, np.uint64)
    n = in_ids.shape[0]
    live = np.asarray(live, bool)
    out = []
    for x in range(n):
        take = min(int(in_counts[x]), in_k)
        r = in_ids[x, :take] - np.uint64(id_base)  # (an id below id_base wraps past every row number)
        r = r[r < np.uint64(n)].astype(np.int64)
        out.append(np.unique(r[live[r]]))
    return out


def candidates(in_ids, in_counts, in_k, live, id_base):
    """-> (C, listed, keyed, N): C[a] = C(a) ascending (empty for a removed a), N[a] = N'(a); listed[a] = |N'(a)| + the sum over u in N'(a) of
    |N'(u)| and keyed[a] = |C(a)| per row, 0 for a removed one: the info's `listed` and `keyed` are their sums over a slab"""
    N = neighbour_sets(in_ids, in_counts, in_k, live, id_base)
    n = len(N)
    sizes = np.array([s.size for s in N], np.int64)
    C, listed, keyed = [], np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a in range(n):
        if not live[a]:
            C.append(np.zeros(0, np.int64))
            continue
        parts = [N[a]] + [N[u] for u in N[a].tolist()]
        listed[a] = N[a].size + sizes[N[a]].sum()
        c = np.unique(np.concatenate(parts))
        C.append(c[c != a])
        keyed[a] = C[a].size
    return C, listed, keyed, N


def key_rows(X, om, omode, rows):
    """{a: the oracle's keys of every stored row against a query equal to row a} for a in rows"""
    X = np.ascontiguousarray(X, np.float32)
    rows = list(rows)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:  # (the oracle's loop runs outside the interpreter lock)
        keys = list(pool.map(lambda a: np.asarray(zo.distance_batch(om, omode, X, X[a]), np.uint64), rows))
    return dict(zip(rows, keys))


def ranked(X, C, rows, om, omode, id_base=0, K=None):
    """per row a of `rows`: (ids, keys) of ALL of C(a) by (key, id) -- the first k of it is the line at any k.  K: key_rows() of (at least) those
    rows, where one table serves many graphs"""
    out = {}
    for a in rows:
        c = C[a]
        if K is not None:
            ks = K[a][c]
        else:
            ks = np.asarray(zo.distance_batch(om, omode, np.ascontiguousarray(X[c]), X[a]), np.uint64) if c.size else np.zeros(0, np.uint64)
        o = np.lexsort((c, ks))
        out[a] = (c[o].astype(np.uint64) + np.uint64(id_base), ks[o])
    return out


def reference(X, graph, in_k, k, live, id_base, om, omode, first_row=0, n=None, K=None):
    """the call's whole answer: (ids [n, k], keys [n, k], counts [n]) and {lines, listed, keyed, updates} of the slab [first_row, first_row + n)"""
    in_ids, in_counts = graph[0], graph[-1]
    stored = in_ids.shape[0]
    n = stored - first_row if n is None else n
    C, listed, keyed, N = candidates(in_ids, in_counts, in_k, live, id_base)
    slab = [a for a in range(first_row, first_row + n) if live[a]]
    R = ranked(X, C, slab, om, omode, id_base, K)
    ids, keys, counts = np.full((n, k), NONE, np.uint64), np.full((n, k), NONE, np.uint64), np.zeros(n, np.uint32)
    updates = 0
    for a in slab:
        rid, rkey = R[a]
        c = min(k, rid.size)
        ids[a - first_row, :c], keys[a - first_row, :c], counts[a - first_row] = rid[:c], rkey[:c], c
        updates += int((~np.isin((rid[:c] - np.uint64(id_base)).astype(np.int64), N[a])).sum())
    info = {"lines": len(slab), "listed": int(listed[slab].sum()), "keyed": int(keyed[slab].sum()), "updates": updates}
    return (ids, keys, counts), info


def rekey(graph, in_k, live, id_base, X, om, omode, K=None):
    """the input lines as the answer would hold them: per live row a, N'(a) minus a by (key, id) -- what 'never above the input line' compares with"""
    _, _, _, N = candidates(graph[0], graph[-1], in_k, live, id_base)
    S = [s[s != a] for a, s in enumerate(N)]
    return ranked(X, S, [a for a in range(len(N)) if live[a]], om, omode, id_base, K)


# ---------------------------------------------------------------------------------------------------------------- the input graphs
def _rng(name, in_k):
    return np.random.default_rng([SEED, in_k, sum(name.encode())])


def _random_live(rng, n, in_k, live):
    """[n, in_k] of live rows drawn with replacement (a line may repeat a row now and then)"""
    pool = np.flatnonzero(live)
    return pool[rng.integers(0, pool.size, (n, in_k))].astype(np.uint64)


def g_repeats(n, in_k, live, id_base):
    """every line draws from three rows of its own: repetitions inside a line count once"""
    rng = _rng("repeats", in_k)
    pool = np.flatnonzero(live)
    three = pool[rng.integers(0, pool.size, (n, 3))]
    ids = np.take_along_axis(three, rng.integers(0, 3, (n, in_k)), 1).astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_self_loops(n, in_k, live, id_base):
    """every line names its own row (first, and again in the middle): a is in N'(a), expanded, and never in the answer"""
    ids = _random_live(_rng("self", in_k), n, in_k, live)
    ids[:, 0] = np.arange(n, dtype=np.uint64)
    ids[:, in_k // 2] = np.arange(n, dtype=np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_removed(n, in_k, live, id_base):
    """half of all entries name removed rows (where the table has any): neither candidates nor expanded"""
    rng = _rng("removed", in_k)
    ids = _random_live(rng, n, in_k, live)
    dead = np.flatnonzero(~np.asarray(live, bool))
    if dead.size:
        m = rng.random((n, in_k)) < 0.5
        ids[m] = dead[rng.integers(0, dead.size, int(m.sum()))].astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_out_of_range(n, in_k, live, id_base):
    """a third of the entries lie below id_base (where it is not 0), at id_base + stored rows, just past it, or far above: ignored, not an error"""
    rng = _rng("range", in_k)
    ids = _random_live(rng, n, in_k, live) + np.uint64(id_base)
    bad = [id_base + n, id_base + n + 1, id_base + 2**32, id_base + 2**32 + 5, 2**63]
    if id_base:
        bad += [0, id_base - 1, id_base // 2]
    bad = np.array(bad, np.uint64)
    m = rng.random((n, in_k)) < 1 / 3
    ids[m] = bad[rng.integers(0, bad.size, int(m.sum()))]
    return ids, np.full(n, in_k, np.uint32)


def g_all_ones(n, in_k, live, id_base):
    """2^64-1 INSIDE the counted part of every line (the tail value of a graph call's output, here counted in)"""
    rng = _rng("ones", in_k)
    ids = _random_live(rng, n, in_k, live) + np.uint64(id_base)
    ids[rng.random((n, in_k)) < 0.4] = NONE
    ids[:, -1] = NONE
    return ids, np.full(n, in_k, np.uint32)


def g_zero_counts(n, in_k, live, id_base):
    """a third of the lines have count 0 (their entries are valid rows that must not be read as neighbours), the rest any count up to in_k"""
    rng = _rng("zero", in_k)
    ids = _random_live(rng, n, in_k, live) + np.uint64(id_base)
    counts = rng.integers(0, in_k + 1, n).astype(np.uint32)
    counts[rng.random(n) < 1 / 3] = 0
    return ids, counts


def g_big_counts(n, in_k, live, id_base):
    """in_counts above in_k (in_k + 5, 2^32-1): the line is its in_k entries"""
    rng = _rng("big", in_k)
    ids = _random_live(rng, n, in_k, live) + np.uint64(id_base)
    counts = np.where(rng.random(n) < 0.5, in_k + 5, 2**32 - 1).astype(np.uint32)
    return ids, counts


def g_same_rows(n, in_k, live, id_base):
    """every line lists the same in_k rows: listed is (in_k + 1) in_k a line, keyed at most in_k"""
    pool = np.flatnonzero(live)
    rows = pool[_rng("same", in_k).permutation(pool.size)[:in_k]]
    ids = np.broadcast_to(rows.astype(np.uint64), (n, rows.size))
    ids = np.concatenate([ids, np.repeat(ids[:, :1], in_k - rows.size, 1)], 1) if rows.size < in_k else ids
    return np.ascontiguousarray(ids) + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_disjoint(n, in_k, live, id_base):
    """line x lists rows x in_k + 1 .. x in_k + in_k (mod n): the lists of row 0's neighbours are pairwise disjoint and hold neither 0 nor one
    another's rows, so that on a table of live rows with n > in_k + in_k^2, |C(0)| = in_k + in_k^2 exactly: every slot the line can gather"""
    x = np.arange(n, dtype=np.int64)[:, None]
    ids = ((x * in_k + 1 + np.arange(in_k, dtype=np.int64)[None, :]) % n).astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_ring(n, in_k, live, id_base):
    """in_k = 1: row x names x + 1 (mod n); wider in_k: x + 1 .. x + in_k"""
    x = np.arange(n, dtype=np.int64)[:, None]
    ids = ((x + 1 + np.arange(in_k, dtype=np.int64)[None, :]) % n).astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_block(n, in_k, live, id_base, block=(100, 140)):
    """most entries name rows of the table's block of bit-identical rows: equal keys, ranked by id"""
    rng = _rng("block", in_k)
    ids = _random_live(rng, n, in_k, live)
    b = np.arange(block[0], block[1])
    b = b[np.asarray(live, bool)[b]]
    m = rng.random((n, in_k)) < 0.7
    ids[m] = b[rng.integers(0, b.size, int(m.sum()))].astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


GRAPHS = {"repeats": g_repeats, "self_loops": g_self_loops, "removed": g_removed, "out_of_range": g_out_of_range, "all_ones": g_all_ones,
          "zero_counts": g_zero_counts, "big_counts": g_big_counts, "same_rows": g_same_rows, "disjoint": g_disjoint, "ring": g_ring,
          "block": g_block}
IN_KS = (1, 5, 32, 44, 45, 64)  # 44 | 45: the boundary between the line kernel's two instantiations (in_k + in_k^2 <= 2048)
BLOCK = (100, 140)               # the 40 bit-identical rows of table()


def table(n, d, block=True):
    """the oracle's synthetic rows, rows BLOCK all equal to the first of them"""
    X = zo.synth_rows(n, d).copy()
    if block:
        X[BLOCK[0]:BLOCK[1]] = X[BLOCK[0]]
    return X


def removed_rows(n):
    """the rows a test removes: every 7th, two of the identical block, and the last row"""
    r = set(range(3, n, 7)) | {BLOCK[0] + 1, BLOCK[0] + 17, n - 1}
    return np.array(sorted(r), np.int64)

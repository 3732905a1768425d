"""The plain reference and the extra input graphs of the reverse-neighbour tests (no GPU, no library: numpy, the oracle and tests/refine_cases.py).

With N'(x) as tests/refine_cases.py defines it (zh_knn_graph_refine's rules for out-of-range, removed and repeated entries):

    In(x)   = { u live, u != x : x in N'(u) },  deg(x) = |In(x)|
    h(u, x) = fmix32((u + 0x9E3779B9 (x + 1)) mod 2^32), fmix32 murmur3's finaliser
    R'(x)   = the first min(rev_k, |In(x) - N'(x)|) members of In(x) - N'(x), ascending by (h(u, x), u)
    B(x)    = N'(x) union R'(x)
    C_r(a)  = ( B(a)  union  B(u) for every u in B(a) ) minus a

reference_reverse() is zh_knn_graph_reverse's whole answer, reference_rev() zh_knn_graph_refine_rev's, both with the info fields the definition
fixes.  tests/test_reverse_reference.py pins them against a Python-loop restatement on a 60-row table; tests/test_gpu_reverse.py runs the library
against them.  GRAPHS are the inputs that only matter once a graph is transposed; each is a pure function of (rows, in_k, live, id_base)."""
import numpy as np

from tests import refine_cases as rc

NONE = rc.NONE
M32 = 0xFFFFFFFF


def h(u, x):
    """the pair's hash, elementwise on arrays (or numbers) of row numbers -> uint64 holding 32-bit values"""
    u, x = np.asarray(u, np.uint64), np.asarray(x, np.uint64)
    m = np.uint64(M32)
    v = (u + ((np.uint64(0x9E3779B9) * ((x + np.uint64(1)) & m)) & m)) & m
    v ^= v >> np.uint64(16)
    v = (v * np.uint64(0x85EBCA6B)) & m
    v ^= v >> np.uint64(13)
    v = (v * np.uint64(0xC2B2AE35)) & m
    v ^= v >> np.uint64(16)
    return v


def in_neighbours(N, live):
    """In(x) of every stored row, ascending int64 row numbers, from N = refine_cases.neighbour_sets(): only a live row's line counts"""
    n = len(N)
    src = np.concatenate([np.full(s.size, u, np.int64) for u, s in enumerate(N) if live[u]] + [np.zeros(0, np.int64)])
    dst = np.concatenate([s for u, s in enumerate(N) if live[u]] + [np.zeros(0, np.int64)])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    o = np.lexsort((src, dst))
    src, dst = src[o], dst[o]
    cuts = np.searchsorted(dst, np.arange(n + 1))
    return [src[cuts[x]:cuts[x + 1]] for x in range(n)]


def reverse_sets(N, In, rev_k, row0=0):
    """R'(x) of every stored row in (h, u) order.  row0: the table's row 0 is stored row row0 of a larger table whose hash is wanted -- h is taken
    of row0 + u, row0 + x (tests/seam_cases.py's group-local references)"""
    out = []
    for x, (s, r) in enumerate(zip(N, In)):
        c = r[~np.isin(r, s)]
        o = np.lexsort((c, h(c + row0, x + row0)))
        out.append(c[o][:rev_k])
    return out


def union_sets(N, R):
    """B(x) = N'(x) union R'(x), ascending"""
    return [np.union1d(s, r) for s, r in zip(N, R)]


def candidates_rev(in_ids, in_counts, in_k, rev_k, live, id_base, row0=0):
    """-> (C_r, listed, keyed, N, In, R): refine_cases.candidates() with B in place of N'; In and R as above (row0: reverse_sets')"""
    N = rc.neighbour_sets(in_ids, in_counts, in_k, live, id_base)
    In = in_neighbours(N, live)
    R = reverse_sets(N, In, rev_k, row0)
    B = union_sets(N, R)
    n = len(N)
    sizes = np.array([s.size for s in B], np.int64)
    C, listed, keyed = [], np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a in range(n):
        if not live[a]:
            C.append(np.zeros(0, np.int64))
            continue
        listed[a] = B[a].size + sizes[B[a]].sum()
        c = np.unique(np.concatenate([B[a]] + [B[u] for u in B[a].tolist()]))
        C.append(c[c != a])
        keyed[a] = C[a].size
    return C, listed, keyed, N, In, R


def reference_reverse(graph, in_k, rev_k, live, id_base, first_row=0, n=None, row0=0):
    """zh_knn_graph_reverse's whole answer: (ids [n, rev_k], counts [n], degree [n]) and {lines, edges, kept, max_degree} (row0: reverse_sets')"""
    in_ids, in_counts = graph[0], graph[-1]
    stored = in_ids.shape[0]
    n = stored - first_row if n is None else n
    N = rc.neighbour_sets(in_ids, in_counts, in_k, live, id_base)
    In = in_neighbours(N, live)
    R = reverse_sets(N, In, rev_k, row0)
    ids, counts, degree = np.full((n, rev_k), NONE, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i in range(n):
        r = R[first_row + i]
        ids[i, :r.size], counts[i], degree[i] = r.astype(np.uint64) + np.uint64(id_base), r.size, In[first_row + i].size
    deg = np.array([r.size for r in In], np.int64)
    info = {"lines": int(np.asarray(live, bool)[first_row:first_row + n].sum()), "edges": int(deg.sum()), "kept": int(counts.sum()),
            "max_degree": int(deg.max()) if stored else 0}
    return (ids, counts, degree), info


def reference_rev(X, graph, in_k, rev_k, k, live, id_base, om, omode, first_row=0, n=None, K=None, row0=0):
    """zh_knn_graph_refine_rev's whole answer: refine_cases.reference() with C_r(a) in place of C(a); `updates` counts against N'(a), and the
    info gains rev_k, edges, kept (over the slab) and max_degree -- all three 0 when rev_k = 0, where nothing is transposed (row0: reverse_sets')"""
    in_ids, in_counts = graph[0], graph[-1]
    stored = in_ids.shape[0]
    n = stored - first_row if n is None else n
    C, listed, keyed, N, In, R = candidates_rev(in_ids, in_counts, in_k, rev_k, live, id_base, row0)
    slab = [a for a in range(first_row, first_row + n) if live[a]]
    ranked = rc.ranked(X, C, slab, om, omode, id_base, K)
    ids, keys, counts = np.full((n, k), NONE, np.uint64), np.full((n, k), NONE, np.uint64), np.zeros(n, np.uint32)
    updates = 0
    for a in slab:
        rid, rkey = ranked[a]
        c = min(k, rid.size)
        ids[a - first_row, :c], keys[a - first_row, :c], counts[a - first_row] = rid[:c], rkey[:c], c
        updates += int((~np.isin((rid[:c] - np.uint64(id_base)).astype(np.int64), N[a])).sum())
    deg = np.array([r.size for r in In], np.int64)
    info = {"lines": len(slab), "listed": int(listed[slab].sum()), "keyed": int(keyed[slab].sum()), "updates": updates, "rev_k": rev_k,
            "edges": int(deg.sum()) if rev_k else 0, "kept": sum(R[x].size for x in range(first_row, first_row + n)) if rev_k else 0,
            "max_degree": int(deg.max()) if rev_k and stored else 0}
    return (ids, keys, counts), info


# ---------------------------------------------------------------------------------------------------------------- the input graphs
def g_hub(n, in_k, live, id_base):
    """every line names rows 0 and 1 (row 0 alone at in_k = 1), then the rows after its own: on a table of live rows the in-degree of row 0 is
    rows - 1, far above any chunk the selection streams, and all but rev_k of its in-neighbours must lose"""
    x = np.arange(n, dtype=np.int64)[:, None]
    ids = ((x + 1 + np.arange(in_k, dtype=np.int64)[None, :]) % n).astype(np.uint64)
    ids[:, 0] = 0
    if in_k > 1:
        ids[:, 1] = 1
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


def g_mutual(n, in_k, live, id_base):
    """a symmetric graph over the live rows (position p of them names p +- 1 .. p +- in_k / 2, cyclically; at in_k = 1 the rows pair up): every
    in-neighbour is in the line already, R' is empty everywhere and the answer is zh_knn_graph_refine's"""
    pool = np.flatnonzero(live)
    m = pool.size
    ids = np.full((n, in_k), NONE, np.uint64)
    counts = np.zeros(n, np.uint32)
    p = np.arange(m, dtype=np.int64)
    if in_k == 1:
        mate = np.where((p ^ 1) < m, p ^ 1, p)  # (an odd row out names itself)
        ids[pool, 0] = pool[mate].astype(np.uint64) + np.uint64(id_base)
    else:
        half = in_k // 2
        for j in range(1, half + 1):
            ids[pool, 2 * j - 2] = pool[(p + j) % m].astype(np.uint64) + np.uint64(id_base)
            ids[pool, 2 * j - 1] = pool[(p - j) % m].astype(np.uint64) + np.uint64(id_base)
        if in_k % 2:
            ids[pool, in_k - 1] = ids[pool, 0]  # (a repetition: counts once)
    counts[pool] = in_k
    return ids, counts


def g_orphan(n, in_k, live, id_base):
    """the first 12 live rows have count 0 (their entries are valid rows that must not be read) and every other line names one of them and random
    live rows: an orphan's answer comes from its reverse neighbours alone"""
    rng = rc._rng("orphan", in_k)
    pool = np.flatnonzero(live)
    orphans = pool[:12]
    ids = rc._random_live(rng, n, in_k, live)
    ids[:, 0] = orphans[rng.integers(0, orphans.size, n)].astype(np.uint64)
    counts = np.full(n, in_k, np.uint32)
    counts[orphans] = 0
    return ids + np.uint64(id_base), counts


CAPPED_DEGREES = (0, 1, 2, 3, 4, 7, 8, 9, 63, 64, 65)


def g_capped(n, in_k, live, id_base):
    """eleven live rows with in-degrees 0, 1, 2, 3, 4, 7, 8, 9, 63, 64 and 65 -- just below, at and above every rev_k the tests use: target j is
    named by its own d_j lines (one counted entry each) and by nobody else; the targets' lines are empty, so nothing is mutual"""
    pool = np.flatnonzero(live)
    ids = np.full((n, in_k), NONE, np.uint64)
    counts = np.zeros(n, np.uint32)
    targets = pool[5:5 + len(CAPPED_DEGREES)]
    namers = pool[40:]
    at = 0
    for t, d in zip(targets, CAPPED_DEGREES):
        mine = namers[at:at + d][::-1]
        at += d
        ids[mine, 0] = np.uint64(t) + np.uint64(id_base)
        counts[mine] = 1
    return ids, counts


def g_removed_namers(n, in_k, live, id_base):
    """every line, a removed row's too, names the live rows after its own: the lines of removed rows are full of valid entries and count for no
    in-degree"""
    pool = np.flatnonzero(live)
    pos = np.searchsorted(pool, np.arange(n))  # the first live row at or after x
    ids = pool[(pos[:, None] + 1 + np.arange(in_k, dtype=np.int64)[None, :]) % pool.size].astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


GRAPHS = {"hub": g_hub, "mutual": g_mutual, "orphan": g_orphan, "capped": g_capped, "removed_namers": g_removed_namers}
ALL_GRAPHS = dict(rc.GRAPHS, **GRAPHS)

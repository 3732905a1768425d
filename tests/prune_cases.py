"""The plain reference and the input graphs of the k-NN graph pruning tests (no GPU, no library: numpy, the oracle, tests/refine_cases.py and
tests/reverse_cases.py).

zh_knn_graph_prune takes a graph over ALL stored rows as zh_knn_graph_refine_rev does and answers, for every live stored row a of a slab,

    P(a)  = ( N'(a)  union  R'(a) ) minus a          N' refine_cases.neighbour_sets, R' reverse_cases.reverse_sets at rev_k (empty at 0)
    c_1 .. c_m = P(a) by (key_a(c), id)              key_q(x) = the oracle's key of stored row x against a query equal to stored row q
    walk the order, S = O = (), stop once |S| == degree; c goes to O if some p in S has key_p(c) < key_a(c) (u64, strict), else to S
    fill: the first degree - |S| members of O join S

the line being S by (key_a, id).  reference() is that loop in numpy with the six info fields the definition fixes (lines, candidates, kept,
occluded, filled, cut); prepare() holds what does not depend on degree and fill, so that one (graph, in_k, rev_k) serves many calls.
tests/test_prune_reference.py pins it against a Python-loop restatement; tests/test_gpu_prune.py runs the library against it.

GRAPHS are refine_cases' adversarial inputs plus the line made of the identical block; exact_graph() is the exact k-NN graph out of a key
table; special_table() / SPECIAL are the lines that need rows of their own: nothing occluded, all candidates tied, m = 64 exactly."""
import numpy as np

from oracle import zebra_oracle as zo
from tests import refine_cases as rc
from tests import reverse_cases as rv

NONE = rc.NONE
FIXED = ("lines", "candidates", "kept", "occluded", "filled", "cut")


# ---------------------------------------------------------------------------------------------------------------- the definition
def candidate_sets(graph, in_k, rev_k, live, id_base, row0=0):
    """-> (P, N, R): P[a] = P(a) ascending (empty for a removed a), N[a] = N'(a), R[a] = R'(a) in (h, u) order"""
    in_ids, in_counts = graph[0], graph[-1]
    N = rc.neighbour_sets(in_ids, in_counts, in_k, live, id_base)
    R = rv.reverse_sets(N, rv.in_neighbours(N, live), rev_k, row0) if rev_k else [np.zeros(0, np.int64) for _ in N]
    P = []
    for a, (s, r) in enumerate(zip(N, R)):
        c = np.union1d(s, r).astype(np.int64)
        P.append(c[c != a] if live[a] else np.zeros(0, np.int64))
    return P, N, R


def prepare(X, graph, in_k, rev_k, live, id_base, om, omode, K=None, rows=None, row0=0):
    """per live row a (of `rows`, default all): (c, ka, M) -- P(a) in (key_a, id) order, their keys key_a, and M[i, j] = key_{c_i}(c_j).
    K: refine_cases.key_rows() of (at least) those rows and their candidates, where one table serves many graphs"""
    P, _, _ = candidate_sets(graph, in_k, rev_k, live, id_base, row0)
    rows = [a for a in (range(len(P)) if rows is None else rows) if live[a]]
    if K is None:
        need = sorted(set(rows) | {int(c) for a in rows for c in P[a]})
        K = rc.key_rows(X, om, omode, need)
    out = {}
    for a in rows:
        c = P[a]
        ka = K[a][c]
        o = np.lexsort((c, ka))
        c, ka = c[o], ka[o]
        M = np.stack([K[int(p)][c] for p in c]) if c.size else np.zeros((0, 0), np.uint64)
        out[a] = (c, ka, M)
    return out


def walk(ka, M, degree):
    """the walk over one ordered line -> (S, O, examined): positions kept, positions occluded, candidates looked at before the stop"""
    S, O = [], []
    low = np.full(ka.size, NONE, np.uint64)  # the smallest key_p(c) over the kept p so far
    examined = 0
    for i in range(ka.size):
        if len(S) == degree:
            break
        examined = i + 1
        if low[i] < ka[i]:
            O.append(i)
        else:
            S.append(i)
            low = np.minimum(low, M[i])
    return S, O, examined


def reference(prep, n_stored, degree, fill, live, id_base, first_row=0, n=None):
    """the call's whole answer out of prepare(): (ids [n, degree], keys [n, degree], counts [n]) and the FIXED info fields of the slab"""
    n = n_stored - first_row if n is None else n
    ids, keys, counts = np.full((n, degree), NONE, np.uint64), np.full((n, degree), NONE, np.uint64), np.zeros(n, np.uint32)
    info = dict.fromkeys(FIXED, 0)
    if degree == 0:
        return (ids, keys, counts), info
    for a in range(first_row, first_row + n):
        if not live[a]:
            continue
        c, ka, M = prep[a]
        S, O, examined = walk(ka, M, degree)
        info["lines"] += 1
        info["candidates"] += int(c.size)
        info["kept"] += len(S)
        info["occluded"] += len(O)
        info["cut"] += int(len(S) == degree and examined < c.size)
        if fill and len(S) < degree:
            take = O[:degree - len(S)]
            info["filled"] += len(take)
            S = sorted(S + take)
        i = a - first_row
        ids[i, :len(S)], keys[i, :len(S)], counts[i] = c[S].astype(np.uint64) + np.uint64(id_base), ka[S], len(S)
    return (ids, keys, counts), info


def keyed_bounds(prep, live, first_row, n):
    """what the info's `keyed` lies between: candidates, and candidates + the sum of |P(a)| (|P(a)| - 1)"""
    m = np.array([prep[a][0].size for a in range(first_row, first_row + n) if live[a]], np.int64)
    return int(m.sum()), int((m * m).sum())


# ---------------------------------------------------------------------------------------------------------------- the input graphs
def g_all_block(n, in_k, live, id_base, block=rc.BLOCK):
    """every line names rows of the table's block of bit-identical rows only: equal keys throughout.  For a row of the block nothing occludes
    (key_p(c) == key_a(c)); for a row outside it the first duplicate occludes all the others (key_p(c) is a row's key against itself)"""
    b = np.arange(block[0], block[1])
    b = b[np.asarray(live, bool)[b]]
    x = np.arange(n, dtype=np.int64)[:, None]
    ids = b[(x + np.arange(in_k, dtype=np.int64)[None, :]) % b.size].astype(np.uint64)
    return ids + np.uint64(id_base), np.full(n, in_k, np.uint32)


GRAPHS = dict(rc.GRAPHS, all_block=g_all_block)
IN_KS = (1, 5, 32, 44, 64)


def degrees(in_k):
    return sorted({1, 8, 16, in_k, 64})


def exact_graph(K, live, id_base, k=32):
    """the exact k-NN graph out of a key table K (refine_cases.key_rows of every live row): knn_graph's (ids, keys, counts)"""
    live = np.asarray(live, bool)
    n = live.size
    pool = np.flatnonzero(live)
    ids, keys, counts = np.full((n, k), NONE, np.uint64), np.full((n, k), NONE, np.uint64), np.zeros(n, np.uint32)
    for a in pool.tolist():
        c = pool[pool != a]
        ka = K[a][c]
        o = np.lexsort((c, ka))[:k]
        ids[a, :o.size], keys[a, :o.size], counts[a] = c[o].astype(np.uint64) + np.uint64(id_base), ka[o], o.size
    return ids, keys, counts


# ---------------------------------------------------------------------------------------------------------------- lines with rows of their own
SPECIAL_ROWS, SPECIAL_DIM = 160, 30


def special_table():
    """160 x 30 under L2 squared: row 0 the origin; rows 1 .. 30 along the axes at distinct radii (1 + i / 64) -- from the origin nothing is
    occluded, since |c_i - c_j|^2 = r_i^2 + r_j^2 > r_j^2; rows 31 .. 60 at -2 e_i -- all 30 tie in key_0 and none occludes another; the rest
    the oracle's synthetic rows"""
    X = zo.synth_rows(SPECIAL_ROWS, SPECIAL_DIM).copy()
    X[:61] = 0.0
    for i in range(30):
        X[1 + i, i] = 1.0 + (i + 1) / 64.0
        X[31 + i, i] = -2.0
    return X


def _special(n, id_base, line0):
    """line 0 = line0, every other line the ring x + 1 .. (64 wide; shorter lines carry counts)"""
    x = np.arange(n, dtype=np.int64)[:, None]
    ids = ((x + 1 + np.arange(64, dtype=np.int64)[None, :]) % n).astype(np.uint64)
    counts = np.full(n, 64, np.uint32)
    ids[0, :len(line0)] = np.asarray(line0, np.uint64)
    counts[0] = len(line0)
    return ids + np.uint64(id_base), counts


# name -> (line 0 of the graph, the degrees it runs at): `axes` reaches degree 30 on its LAST candidate and degree 1 on its first
SPECIAL = {"axes": (list(range(1, 31)), (1, 29, 30, 31, 64)), "ties": (list(range(31, 61)), (1, 8, 30, 64)),
           "full64": (list(range(61, 125)), (1, 16, 63, 64))}


def special_graph(name, id_base=0):
    return _special(SPECIAL_ROWS, id_base, SPECIAL[name][0])

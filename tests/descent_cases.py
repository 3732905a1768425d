"""The plain reference of the NN-descent tests (no GPU, no library: numpy, the oracle, tests/refine_cases.py and tests/reverse_cases.py).

zh_knn_graph_descent(G_0, in_k, rev_k, k, rounds) returns G_R, where G_r is what zh_knn_graph_refine_rev(G_{r-1}, in_k_r, rev_k, k) returns for the
whole table (in_k_1 = in_k, in_k_r = k afterwards; rev_k = 0: zh_knn_graph_refine), R = rounds or the first r whose `updates` is 0.  descent()
iterates reverse_cases.reference_rev() for that, and beside every full round r >= 2 it builds the line the incremental definition gives:

    U_r(x)  = N'(G_r)(x) union R'(x) of G_r -- the line round r + 1 ranks over
    new_r(x) = U_r(x) minus U_{r-1}(x); every entry of U_0 is new
    S(a)    = ( new_r(a)  union  U_r(b) for b in new_r(a)  union  new_r(b) for b in U_r(a) minus new_r(a) ) minus a minus N'(G_r)(a)
    line    = the first k by (key, id) of S(a) union N'(G_r)(a)

with keyed = |S(a)|, listed = the entries gathered before de-duplication (a and the members of the forward line included, as they are gathered and
then dropped) and active = the lines whose S(a) is not empty.  tests/test_descent_reference.py asserts that the two lines agree for every live row
and every round, and pins the figures of CASES; tests/test_gpu_descent.py runs the library against both."""
import numpy as np

from oracle import zebra_oracle as zo
from tests import refine_cases as rc
from tests import reverse_cases as rv

NONE = rc.NONE

# name -> (rows, graph, metric index of tests/test_gpu_fknn.thirteen_metrics, in_k, k, rev_k): the issue's four cases, all on rc.table(rows, 30)
CASES = {1: (1500, "block", 0, 32, 32, 0), 2: (1500, "hub", 7, 5, 8, 8), 3: (1200, "ring", 0, 45, 45, 19), 4: (1500, "ring", 0, 8, 8, 0)}
ORACLE_METRIC = {0: (zo.L2SQ, 0), 7: (zo.MANHATTAN, 0)}  # the oracle's side of those metric indexes


def union_lines(graph, in_k, rev_k, live, id_base, row0=0):
    """-> (N, U): N'(x) and U(x) = N'(x) union R'(x) of every stored row, ascending int64 row numbers (row0: reverse_cases.reverse_sets')"""
    N = rc.neighbour_sets(graph[0], graph[-1], in_k, live, id_base)
    if not rev_k:
        return N, N
    R = rv.reverse_sets(N, rv.in_neighbours(N, live), rev_k, row0)
    return N, rv.union_sets(N, R)


def incremental_round(U_old, N, U, k, live, id_base, K):
    """round r + 1 >= 2 by the incremental definition, from U_{r-1} (U_old), N'(G_r) (N) and U_r (U): -> (ids, keys, counts), {listed, keyed,
    updates, active}.  K: refine_cases.key_rows() of every live row"""
    n = len(U)
    new = [np.setdiff1d(U[x], U_old[x]) for x in range(n)]
    nnew = np.array([s.size for s in new], np.int64)
    nall = np.array([s.size for s in U], np.int64)
    ids, keys, counts = np.full((n, k), NONE, np.uint64), np.full((n, k), NONE, np.uint64), np.zeros(n, np.uint32)
    info = {"listed": 0, "keyed": 0, "updates": 0, "active": 0}
    for a in np.flatnonzero(live).tolist():
        fresh = new[a]
        old = np.setdiff1d(U[a], fresh)
        info["listed"] += int(fresh.size + nall[fresh].sum() + nnew[old].sum())
        parts = [fresh] + [U[b] for b in fresh.tolist()] + [new[b] for b in old.tolist()]
        S = np.unique(np.concatenate(parts))
        S = S[S != a]
        S = np.setdiff1d(S, N[a])
        info["keyed"] += int(S.size)
        info["active"] += 1 if S.size else 0
        fwd = N[a][N[a] != a]
        c = np.concatenate([S, fwd])
        ks = K[a][c]
        o = np.lexsort((c, ks))[:k]
        ids[a, :o.size], keys[a, :o.size], counts[a] = c[o].astype(np.uint64) + np.uint64(id_base), ks[o], o.size
        info["updates"] += int((~np.isin(c[o], N[a])).sum())
    return (ids, keys, counts), info


def descent(X, graph, in_k, rev_k, k, rounds, live, id_base, om, omode, K=None, row0=0):
    """-> (answer, info, full, inc): the call's (ids, keys, counts); info = {rounds_run, listed_round, keyed_round, updates_round, active_round,
    full_keyed_round} (lists of rounds_run entries; full_keyed_round is what a loop over full rounds keys); full[r] and inc[r] the full and the
    incremental answer of round r + 1 (inc[0] is full[0]: round 1 IS the full round).  row0: reverse_cases.reverse_sets'"""
    live = np.asarray(live, bool)
    if K is None:
        K = rc.key_rows(X, om, omode, np.flatnonzero(live).tolist())
    info = {"rounds_run": 0, "listed_round": [], "keyed_round": [], "updates_round": [], "active_round": [], "full_keyed_round": []}
    full, inc = [], []
    g, w, U_old = (graph[0], graph[-1]), in_k, None
    for r in range(rounds):
        ref, rinfo = rv.reference_rev(X, g, w, rev_k, k, live, id_base, om, omode, K=K, row0=row0)
        N, U = union_lines(g, w, rev_k, live, id_base, row0)
        if r == 0:
            got, ginfo = ref, {"listed": rinfo["listed"], "keyed": rinfo["keyed"], "updates": rinfo["updates"], "active": int(live.sum())}
        else:
            got, ginfo = incremental_round(U_old, N, U, k, live, id_base, K)
        full.append(ref)
        inc.append(got)
        info["rounds_run"] = r + 1
        info["full_keyed_round"].append(rinfo["keyed"])
        for f in ("listed", "keyed", "updates", "active"):
            info[f + "_round"].append(ginfo[f])
        if rinfo["updates"] == 0:
            break
        g, w, U_old = (ref[0], ref[2]), k, U
    return full[-1], info, full, inc


def case(number, id_base=0, removed=True):
    """-> (X, live, graph, metric index, in_k, k, rev_k) of one of CASES"""
    n, gname, mi, in_k, k, rev_k = CASES[number]
    X = rc.table(n, 30)
    live = np.ones(n, bool)
    if removed:
        live[rc.removed_rows(n)] = False
    return X, live, rv.ALL_GRAPHS[gname](n, in_k, live, id_base), mi, in_k, k, rev_k

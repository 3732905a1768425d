"""The plain reference of the graph search tests (no GPU, no library: numpy, the oracle, and tests/refine_cases.py for tables and graphs).

zh_index_set_graph keeps a graph over the first g_rows stored rows; N'(p) at search time is the live rows among line p's kept entries (the first
min(count, g_k) of the line, inside [id_base, id_base + the rows stored at the attach), each row once), empty for p >= g_rows.  For a query q with
key(r) = the oracle's distance_batch key of stored row r against q, zh_search_graph_batch is:

    S(q) = the live stored rows the query's seeds name; B = the first `beam` of S(q) by (key, id), every entry unexpanded
    iteration t = 0, 1, ...: stop when t == max_iters (max_iters = 0: no cap) or B has no unexpanded entry; otherwise
        P    = the first `width` unexpanded entries of B, marked expanded
        cand = the union of N'(p), p in P, minus the rows in B now
        B    = the first `beam` of B union cand by (key, id), flags travelling with their rows
    the answer = the first top_k of B

reference() is that, straight from the definition.  reference_textbook() differs in ONE line: cand is taken minus every row keyed so far (a visited
set).  tests/test_gsearch_reference.py asserts that the two give the same answers and iteration counts on every entry of CASES x SETTINGS and pins
the figures of NAMED; tests/test_gpu_gsearch.py runs the library against reference()."""
import functools

import numpy as np

from oracle import zebra_oracle as zo
from tests import refine_cases as rc

NONE = rc.NONE
GRAPH_BATCH = 16384  # ZH_GRAPH_BATCH: queries of one launch (the info's `launches`)


# ---------------------------------------------------------------------------------------------------------------- the definition
def kept_lines(graph, g_rows, g_k, id_base, attach_rows):
    """line p < g_rows as zh_index_set_graph keeps it: int64 row numbers, each once (liveness is judged at search time)"""
    in_ids, in_counts = np.asarray(graph[0], np.uint64), np.asarray(graph[-1])
    out = []
    for p in range(g_rows):
        take = min(int(in_counts[p]), g_k)
        r = in_ids[p, :take] - np.uint64(id_base)  # (an id below id_base wraps past every row number)
        out.append(np.unique(r[r < np.uint64(attach_rows)].astype(np.int64)))
    return out


def seed_rows(seeds_q, live, id_base):
    """S(q) of one query's seed ids: live stored rows, each once"""
    r = np.asarray(seeds_q, np.uint64) - np.uint64(id_base)
    r = r[r < np.uint64(live.size)].astype(np.int64)
    return np.unique(r[live[r]]).tolist()


def walk(keys, lines, live, S, beam, width, max_iters, textbook=False):
    """one query -> (B as [(key, row)], iterations, expanded, keyed, capped, the set of rows that ever got a key).  keys: python ints per stored row"""
    B = sorted((keys[r], r, False) for r in S)[:beam]
    seen = set(S)
    keyed, t, expanded, capped = len(S), 0, 0, 0
    while True:
        un = [i for i, e in enumerate(B) if not e[2]]
        if not un:
            break
        if max_iters and t == max_iters:
            capped = 1
            break
        P = un[:width]
        for i in P:
            B[i] = (B[i][0], B[i][1], True)
        cand = set()
        for i in P:
            p = B[i][1]
            if p < len(lines):
                cand.update(r for r in lines[p].tolist() if live[r])
        if textbook:
            cand -= seen
        else:
            cand -= {e[1] for e in B}
        seen |= cand
        keyed += len(cand)
        expanded += len(P)
        B = sorted(B + [(keys[r], r, False) for r in cand])[:beam]
        t += 1
    return [(k, r) for k, r, _ in B], t, expanded, keyed, capped, seen


def _run(X, graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, attach_rows, trace, textbook):
    X, Q, live = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32), np.asarray(live, bool)
    seeds = np.asarray(seeds, np.uint64)
    b = Q.shape[0]
    lines = kept_lines(graph, g_rows, g_k, id_base, X.shape[0] if attach_rows is None else attach_rows)
    ids, keys, counts = np.full((b, top_k), NONE, np.uint64), np.full((b, top_k), NONE, np.uint64), np.zeros(b, np.uint32)
    info = {"queries": b, "seeds": 0, "iterations": 0, "expanded": 0, "keyed": 0, "capped": 0, "launches": -(-b // GRAPH_BATCH)}
    for i in range(b):
        kq = np.asarray(zo.distance_batch(om, omode, X, Q[i]), np.uint64).tolist() if X.shape[0] else []
        S = seed_rows(seeds[i], live, id_base)
        B, t, ex, ky, cp, seen = walk(kq, lines, live, S, beam, width, max_iters, textbook)
        c = min(top_k, len(B))
        ids[i, :c] = np.array([r for _, r in B[:c]], np.uint64) + np.uint64(id_base)
        keys[i, :c] = np.array([k for k, _ in B[:c]], np.uint64)
        counts[i] = c
        info["seeds"] += len(S); info["iterations"] += t; info["expanded"] += ex; info["keyed"] += ky; info["capped"] += cp
        if trace is not None:
            trace.append(seen)
    return (ids, keys, counts), info


def reference(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, attach_rows=None, trace=None):
    """the call's whole answer by the definition: (ids [b, top_k], keys [b, top_k], counts [b]) and the info dict.  table_graph: the (ids, counts)
    or (ids, keys, counts) the caller attached; live: the live mask at the time of the SEARCH; attach_rows: the rows stored at the attach where
    rows were appended since (default: X's); trace: a list that receives, per query, the set of rows that ever got a key"""
    return _run(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, attach_rows, trace, False)


def reference_textbook(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, attach_rows=None, trace=None):
    """the same with "minus every row keyed so far" for "minus the rows in B now": a visited set"""
    return _run(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, attach_rows, trace, True)


def default_seeds(b, n_seed, g_rows, id_base):
    """LSHIndex.search_graph_batch's seeds=None: the same strided rows for every query"""
    row = np.array([j * g_rows // n_seed for j in range(n_seed)], np.uint64) + np.uint64(id_base)
    return np.ascontiguousarray(np.broadcast_to(row, (b, n_seed)))


# ---------------------------------------------------------------------------------------------------------------- tables, graphs, cases
TABLES = {"t1500": (1500, 30), "t600": (600, 30), "t600x128": (600, 128), "t600x256": (600, 256)}  # d = 30: the generic path; 128: specialised for every
                                                                                                   # kind; 256: for L2 / cosine only


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (X, live): rc.table's rows with the 40 bit-identical rows of rc.BLOCK, rc.removed_rows removed"""
    n, d = TABLES[name]
    X = rc.table(n, d)
    live = np.ones(n, bool)
    live[rc.removed_rows(n)] = False
    X.setflags(write=False); live.setflags(write=False)
    return X, live


def exact_graph(X, g_k, live, id_base, om, omode, K=None):
    """the exact g_k-NN graph among live rows (a removed row's line is empty), from rc.key_rows"""
    live = np.asarray(live, bool)
    n = X.shape[0]
    rows = np.flatnonzero(live)
    if K is None:
        K = rc.key_rows(X, om, omode, rows.tolist())
    ids, counts = np.full((n, g_k), NONE, np.uint64), np.zeros(n, np.uint32)
    for a in rows.tolist():
        c = rows[rows != a]
        o = np.lexsort((c, K[a][c]))[:g_k]
        ids[a, :o.size], counts[a] = c[o].astype(np.uint64) + np.uint64(id_base), o.size
    return ids, counts


@functools.lru_cache(maxsize=None)
def graph(tname, gname, g_k, id_base=0):
    """a graph over table `tname`: an entry of rc.GRAPHS, or "exact" (L2SQ)"""
    X, live = table(tname)
    if gname == "exact":
        g = exact_graph(X, g_k, live, id_base, zo.L2SQ, 0)
    else:
        g = rc.GRAPHS[gname](X.shape[0], g_k, live, id_base)
    for a in g:
        a.setflags(write=False)
    return g


def queries(tname, b):
    n, d = TABLES[tname]
    return zo.synth_queries(b, d, n)


# (beam, width, n_seed, max_iters): every pair of the equivalence test's grid
SETTINGS = [(1, 1, 1, 0), (2, 1, 8, 0), (8, 1, 8, 0), (33, 1, 8, 0), (33, 2, 8, 0), (64, 1, 32, 0), (64, 2, 32, 0), (64, 8, 32, 0), (64, 1, 64, 0),
            (128, 1, 32, 0), (128, 4, 32, 0), (255, 1, 8, 0), (255, 2, 32, 0), (256, 1, 1, 0), (256, 1, 32, 0), (256, 8, 32, 0), (64, 1, 32, 3),
            (256, 2, 32, 20)]
# (table, graph, g_k): every graph on one table, the exact graph on both generic tables and at three widths
CASES = [("t1500", "exact", 32), ("t600", "exact", 32), ("t600", "exact", 5), ("t600", "exact", 64)] + [("t600", g, 32) for g in sorted(rc.GRAPHS)] + \
        [("t600", "ring", 1)]
EQ_QUERIES = 8

# the four cases whose info figures tests/test_gsearch_reference.py pins: name -> (table, graph, g_k, queries, (beam, width, n_seed, max_iters))
NAMED = {"exact32_beam64": ("t1500", "exact", 32, 64, (64, 1, 32, 0)),
         "exact32_beam256_w8": ("t1500", "exact", 32, 64, (256, 8, 32, 0)),
         "block_beam33_w2": ("t600", "block", 32, 64, (33, 2, 8, 0)),
         "ring1_capped": ("t600", "ring", 1, 64, (8, 1, 8, 3))}


def run_case(tname, gname, g_k, b, setting, textbook=False, top_k=None, id_base=0, trace=None):
    """a case under the default seeds, L2SQ -> reference()'s or reference_textbook()'s return"""
    X, live = table(tname)
    beam, width, n_seed, max_iters = setting
    f = reference_textbook if textbook else reference
    return f(X, graph(tname, gname, g_k, id_base), X.shape[0], g_k, live, id_base, queries(tname, b), default_seeds(b, n_seed, X.shape[0], id_base),
             beam if top_k is None else top_k, beam, width, max_iters, zo.L2SQ, 0, trace=trace)

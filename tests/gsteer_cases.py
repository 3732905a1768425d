"""The plain reference of the filter-steered graph search tests (no GPU, no library: numpy, the oracle, tests/gsearch_cases.py for tables, graphs
and seeds, tests/gfilter_cases.py for the filters).

zh_search_graph_steered_batch, literally.  A = the stored rows r < n_bits whose filter bit is set and that are live at the time of the search; a KEPT
entry of line p < g_rows is one zh_index_set_graph's table does not mask: among the line's first min(count, g_k) ids, those inside [id_base, id_base
+ the rows stored at the attach), each row at its first place, IN THE LINE'S ORDER.  For a query q with key(r) the oracle's distance_batch key:

    S(q) = the rows of A the query's seeds name; B = the first `beam` of S(q) by (key, id), every entry unexpanded
    iteration t = 0, 1, ...: stop when t == max_iters (max_iters = 0: no cap) or B has no unexpanded entry; otherwise
        P = the first `width` unexpanded entries of B, marked expanded
        E = first hop: for p in P's order, for the kept entries n of line p in order: n in A -> emit n; else if hops == 2 and n is live -> n joins
            the bridge list H (each row once, in this order); second hop: for h in H's order, for the kept entries m of line h in order: m in A ->
            emit m
        cand = E, each row at its first emission, minus the rows in B now, truncated to its first MAX_CAND = 256 rows
        B = the first `beam` of B union cand by (key, id), flags travelling with their rows
    the answer = the first top_k of B

There is no visited set and none can be written in: truncation makes cand depend on B.  tests/test_gsteer_reference.py pins this file against
gsearch_cases.reference where the two must agree and pins the figures of the graphs made here; tests/test_gpu_gsteer.py runs the library against
reference()."""
import functools

import numpy as np

from oracle import zebra_oracle as zo
from tests import gfilter_cases as fc
from tests import gsearch_cases as gc
from tests.gsearch_cases import GRAPH_BATCH, NONE

MAX_CAND = 256  # ZH_GRAPH_MAX_CAND
WALK_FIELDS = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches")
FIELDS = WALK_FIELDS + ("rows_allowed", "direct", "via_bridge", "bridges", "cand_full", "returned")

# (beam, width, n_seed, max_iters, top_k): the GPU test's grid; the last one caps
SETTINGS = [(1, 1, 1, 0, 1), (8, 1, 8, 0, 8), (33, 2, 8, 0, 10), (64, 4, 32, 0, 10), (64, 1, 32, 0, 64), (256, 8, 32, 0, 256), (64, 1, 32, 2, 10)]


# ---------------------------------------------------------------------------------------------------------------- the definition
def ordered_lines(graph, g_rows, g_k, id_base, attach_rows):
    """line p < g_rows as the attached table keeps it: python ints in the line's order, each row at its first place (liveness is judged at search
    time: a row dead at the attach is dead now)"""
    in_ids, in_counts = np.asarray(graph[0], np.uint64), np.asarray(graph[-1])
    out = []
    for p in range(g_rows):
        take = min(int(in_counts[p]), g_k)
        r = in_ids[p, :take] - np.uint64(id_base)  # (an id below id_base wraps past every row number)
        line = []
        for x in r[r < np.uint64(attach_rows)].astype(np.int64).tolist():
            if x not in line:
                line.append(x)
        out.append(line)
    return out


def seed_rows(seeds_q, allowed, id_base):
    """S(q) of one query's seed ids: rows of A, each once"""
    r = np.asarray(seeds_q, np.uint64) - np.uint64(id_base)
    r = r[r < np.uint64(allowed.size)].astype(np.int64)
    return np.unique(r[allowed[r]]).tolist()


def walk(keys, lines, live, allowed, S, beam, width, max_iters, hops):
    """one query -> (B as [(key, row)], the figures as a dict)"""
    B = sorted((keys[r], r, False) for r in S)[:beam]
    f = dict(seeds=len(S), iterations=0, expanded=0, keyed=len(S), capped=0, direct=0, via_bridge=0, bridges=0, cand_full=0)
    t = 0
    while True:
        un = [i for i, e in enumerate(B) if not e[2]]
        if not un:
            break
        if max_iters and t == max_iters:
            f["capped"] = 1
            break
        P = un[:width]
        for i in P:
            B[i] = (B[i][0], B[i][1], True)
        E, H = [], []
        for i in P:
            p = B[i][1]
            for n in (lines[p] if p < len(lines) else []):
                if allowed[n]:
                    E.append((n, 1))
                elif hops == 2 and live[n] and n not in H:
                    H.append(n)
        for h in H:
            for m in (lines[h] if h < len(lines) else []):
                if allowed[m]:
                    E.append((m, 2))
        in_b, cand, hop_of = {e[1] for e in B}, [], {}
        for r, hop in E:
            if r not in in_b and r not in hop_of:
                hop_of[r] = hop
                cand.append(r)
        cand = cand[:MAX_CAND]
        direct = sum(1 for r in cand if hop_of[r] == 1)
        f["direct"] += direct; f["via_bridge"] += len(cand) - direct; f["bridges"] += len(H); f["cand_full"] += int(len(cand) == MAX_CAND)
        f["keyed"] += len(cand); f["expanded"] += len(P)
        B = sorted(B + [(keys[r], r, False) for r in cand])[:beam]
        t += 1
    f["iterations"] = t
    return [(k, r) for k, r, _ in B], f


def reference(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, words, n_bits, hops, attach_rows=None):
    """the call's whole answer: (ids [b, top_k], keys [b, top_k], counts [b]) and the info dict (zh_graph_steered_info's thirteen fields).  The
    arguments are gfilter_cases.reference's plus hops; live is the live mask at the time of the SEARCH"""
    assert hops in (1, 2)
    X, Q, live = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32), np.asarray(live, bool)
    seeds = np.asarray(seeds, np.uint64)
    b = Q.shape[0]
    lines = ordered_lines(table_graph, g_rows, g_k, id_base, X.shape[0] if attach_rows is None else attach_rows)
    allowed = fc.allowed_rows(words, n_bits, live)
    ids, keys, counts = np.full((b, top_k), NONE, np.uint64), np.full((b, top_k), NONE, np.uint64), np.zeros(b, np.uint32)
    info = dict.fromkeys(FIELDS, 0)
    info.update(queries=b, launches=-(-b // GRAPH_BATCH), rows_allowed=int(np.count_nonzero(allowed)))
    for i in range(b):
        kq = np.asarray(zo.distance_batch(om, omode, X, Q[i]), np.uint64).tolist() if X.shape[0] else []
        B, f = walk(kq, lines, live, allowed, seed_rows(seeds[i], allowed, id_base), beam, width, max_iters, hops)
        c = min(top_k, len(B))
        ids[i, :c] = np.array([r for _, r in B[:c]], np.uint64) + np.uint64(id_base)
        keys[i, :c] = np.array([k for k, _ in B[:c]], np.uint64)
        counts[i] = c
        for k, v in f.items():
            info[k] += v
        info["returned"] += c
    return (ids, keys, counts), info


def run_case(tname, gname, g_k, b, setting, fname, hops, id_base=0):
    """a case under the default seeds, L2SQ -> reference()'s return"""
    X, live = gc.table(tname)
    beam, width, n_seed, max_iters, top_k = setting
    words, n_bits = fc.table_filter(tname, fname)
    return reference(X, gc.graph(tname, gname, g_k, id_base), X.shape[0], g_k, live, id_base, gc.queries(tname, b),
                     gc.default_seeds(b, n_seed, X.shape[0], id_base), top_k, beam, width, max_iters, zo.L2SQ, 0, words, n_bits, hops)


# ---------------------------------------------------------------------------------------------------------------- (a) the random out-32 graph
@functools.lru_cache(maxsize=None)
def random_graph(tname="t1500", g_k=32, id_base=0):
    """every live row names g_k distinct live rows, uniformly; a removed row's line is empty.  With r % 2 == 0 allowed and width 4 an iteration
    emits about 64 direct rows and about 1000 second-hop rows: cand is truncated in most iterations"""
    X, live = gc.table(tname)
    n = X.shape[0]
    rng = np.random.default_rng([0x57EE2, n, g_k])
    rows = np.flatnonzero(live)
    ids, counts = np.full((n, g_k), NONE, np.uint64), np.zeros(n, np.uint32)
    for a in rows.tolist():
        c = rng.choice(rows[rows != a], g_k, replace=False)
        ids[a], counts[a] = c.astype(np.uint64) + np.uint64(id_base), g_k
    ids.setflags(write=False); counts.setflags(write=False)
    return ids, counts


RANDOM_CASE = dict(tname="t1500", g_k=32, b=4, setting=(64, 4, 32, 0, 10), fname="even")


def run_random_case(hops, id_base=0):
    c = RANDOM_CASE
    X, live = gc.table(c["tname"])
    beam, width, n_seed, max_iters, top_k = c["setting"]
    words, n_bits = fc.table_filter(c["tname"], c["fname"])
    return reference(X, random_graph(c["tname"], c["g_k"], id_base), X.shape[0], c["g_k"], live, id_base, gc.queries(c["tname"], c["b"]),
                     gc.default_seeds(c["b"], n_seed, X.shape[0], id_base), top_k, beam, width, max_iters, zo.L2SQ, 0, words, n_bits, hops)


# ---------------------------------------------------------------------------------------------------------------- (b) the seam graphs
SEAM_TABLE, SEAM_K = "t1500", 64


def _seam_rows():
    """the live rows of the 1500-row table split by parity: allowed = even, disallowed = odd (the filter "even")"""
    _, live = gc.table(SEAM_TABLE)
    rows = np.flatnonzero(live)
    return rows[rows % 2 == 0].tolist(), rows[rows % 2 == 1].tolist(), np.flatnonzero(~live).tolist()


def _graph_of(lines, n=1500, g_k=SEAM_K, id_base=0):
    ids, counts = np.full((n, g_k), NONE, np.uint64), np.zeros(n, np.uint32)
    for p, line in lines.items():
        assert len(line) <= g_k
        ids[p, :len(line)] = np.array(line, np.uint64) + np.uint64(id_base)
        counts[p] = len(line)
    return ids, counts


def seam_graph(name, id_base=0):
    """-> (graph, g_rows, seed rows, width).  p = the first allowed row; its line names disallowed live rows (bridges) whose lines name allowed rows"""
    even, odd, dead = _seam_rows()
    p, others = even[0], even[1:]
    br = odd[:4]
    width, g_rows, seeds = 1, 1500, [p]
    if name == "exact256":      # four bridges x 64 distinct allowed rows: |cand| == 256 exactly, nothing dropped
        lines = {p: br}
        lines.update({h: others[64 * i:64 * i + 64] for i, h in enumerate(br)})
    elif name == "one_dropped":  # the twin: p's line names one allowed row too; the last entry of the last bridge is the one row dropped
        lines = {p: br + [others[256]]}
        lines.update({h: others[64 * i:64 * i + 64] for i, h in enumerate(br)})
    elif name == "removed_bridge":  # a removed row in p's line is skipped, not hopped through (its line would name rows nobody else does)
        lines = {p: [dead[0], br[0]], dead[0]: others[100:130], br[0]: others[:10]}
    elif name == "late_bridge":  # a bridge >= g_rows (a row stored but past the attached lines): an empty line
        g_rows = 1400
        late = [r for r in odd if r >= 1400][0]
        lines = {p: [late, br[0]], br[0]: others[:10]}
    elif name == "back_edges":  # a bridge whose line names p and rows already in the beam (the seeds)
        seeds, width = [p] + others[:3], 4  # (all four are expanded; only p has a line)
        lines = {p: [br[0]], br[0]: [p] + others[:3] + others[20:30]}
    elif name == "shared_bridge":  # two parents sharing a bridge: H holds it once an iteration
        seeds, width = [p, others[0]], 2
        lines = {p: [br[0], br[1]], others[0]: [br[1], br[0], br[2]], br[0]: others[10:20], br[1]: others[15:25], br[2]: others[30:33]}
    else:
        raise KeyError(name)
    return _graph_of(lines, id_base=id_base), g_rows, seeds, width


SEAMS = ("exact256", "one_dropped", "removed_bridge", "late_bridge", "back_edges", "shared_bridge")


def run_seam(name, hops, id_base=0, b=2, beam=256, max_iters=1):
    """one iteration of the seam graph `name` from its seeds, filter "even" -> (reference()'s return, the graph, g_rows, the seed array, width)"""
    X, live = gc.table(SEAM_TABLE)
    g, g_rows, seed_list, width = seam_graph(name, id_base)
    seeds = np.ascontiguousarray(np.broadcast_to(np.array(seed_list, np.uint64) + np.uint64(id_base), (b, len(seed_list))))
    words, n_bits = fc.table_filter(SEAM_TABLE, "even")
    ref = reference(X, g, g_rows, SEAM_K, live, id_base, gc.queries(SEAM_TABLE, b), seeds, beam, beam, width, max_iters, zo.L2SQ, 0, words, n_bits, hops)
    return ref, g, g_rows, seeds, width


# ---------------------------------------------------------------------------------------------------------------- (c) the line widths
WIDTHS = (1, 5, 24, 32, 64)  # g_k: 256 / g_k bridges share a pass of the second hop (24 does not divide 256)


def width_setting(g_k):
    """(beam, width, n_seed, max_iters, top_k) with the most parents the line width admits, capped at 8"""
    return (64, min(8, 256 // g_k), 32, 0, 10)


def allowed_seeds(b, n_seed, words, n_bits, id_base):
    """LSHIndex.search_graph_steered_batch's seeds="allowed": n_seed rows strided over the mask's set positions, the same for every query"""
    rows = np.flatnonzero(np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")[:n_bits])
    if rows.size == 0:
        row = np.full(n_seed, NONE, np.uint64)
    elif rows.size < n_seed:
        row = rows[np.arange(n_seed) % rows.size].astype(np.uint64) + np.uint64(id_base)
    else:
        row = rows[[j * rows.size // n_seed for j in range(n_seed)]].astype(np.uint64) + np.uint64(id_base)
    return np.ascontiguousarray(np.broadcast_to(row, (b, n_seed)))

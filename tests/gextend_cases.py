"""The plain reference of the graph extension tests (no GPU, no library: numpy, the oracle, tests/gsearch_cases.py for the walk and
tests/refine_cases.py for tables and graphs).

zh_index_extend_graph gives the rows stored since zh_index_set_graph lines of their own and lets old lines name them.  G = the rows the attached
table covers, N = the stored rows now, g_k = the table's width.  The new rows go in chunks [lo, hi) of `batch` stored rows, lo = G + c batch; while
chunk c is processed the table covers [0, lo), the earlier chunks' lines and every change they made to older lines included.

    step 1  for every live row a of [lo, hi): gsearch_cases.walk with the query = stored row a, the lines [0, lo), the live mask of now, and the
            seeds of a that name a live row < lo.  line(a) = the first min(g_k, |B|) rows of the final beam.  A removed row's line is empty.
    step 2  for every live row r < lo with R(r) = [a live in the chunk : r in line(a)] not empty:
            line(r) = the first g_k of L'(r) + R(r) by (key_r(x), x), L'(r) = the entries of line(r) that are live now,
            key_r(x) = the oracle's distance_batch key of stored row x against a query equal to stored row r.  Every other line stays as it is.

A line is kept as the ordered list of its kept entries: zh_index_get_graph reads exactly that (table order, compacted to the front).  kept_table()
is what zh_index_set_graph keeps of an input graph in that form -- gsearch_cases.kept_lines sorts its lines, which the walk may and get_graph may not.
extend() is the definition, graph_arrays() the expected zh_index_get_graph output; tests/test_gextend_reference.py pins both on the CPU and
tests/test_gpu_gextend.py runs the library against them."""
import functools

import numpy as np

from oracle import zebra_oracle as zo
from tests import gsearch_cases as gc
from tests import refine_cases as rc

NONE = rc.NONE
MAX_BATCH = 1024  # ZH_GRAPH_EXTEND_MAX_BATCH
INFO_FIELDS = ("rows_added", "rows_removed", "chunks", "seeds", "iterations", "expanded", "keyed", "capped", "reverse_rows", "reverse_offered",
               "reverse_kept", "launches")


# ---------------------------------------------------------------------------------------------------------------- the definition
def kept_table(graph, g_rows, g_k, id_base, stored, live_at_attach):
    """line p < g_rows as zh_index_set_graph keeps it, in table order: the first min(count, g_k) entries that name a stored row live at the attach,
    each row at its first place only"""
    in_ids, in_counts = np.asarray(graph[0], np.uint64), np.asarray(graph[-1])
    out = []
    for p in range(g_rows):
        line = []
        for v in (in_ids[p, :min(int(in_counts[p]), g_k)] - np.uint64(id_base)).tolist():  # (an id below id_base wraps past every row number)
            if v < stored and live_at_attach[v] and v not in line:
                line.append(int(v))
        out.append(line)
    return out


def key_matrix(X, om, omode):
    """K[r][x] = the oracle's key of stored row x against a query equal to stored row r"""
    K = rc.key_rows(X, om, omode, range(X.shape[0]))
    return np.stack([K[r] for r in range(X.shape[0])]) if X.shape[0] else np.zeros((0, 0), np.uint64)


def extend(K, lines, live, id_base, seeds, g_k, beam, width, max_iters, batch, trace=None):
    """the call by the definition.  K: key_matrix of the N stored rows; lines: the G lines of the attached table (kept_table's form); live: the live
    mask of now; seeds: [N - G, n_seed] ids.  -> (the N lines, the info dict).  trace: a dict that receives per chunk start lo the dict r -> (R(r), L'(r))"""
    N, G = K.shape[0], len(lines)
    live = np.asarray(live, bool)
    seeds = np.asarray(seeds, np.uint64).reshape(N - G, -1)
    lines = [list(x) for x in lines]
    info = dict.fromkeys(INFO_FIELDS, 0)
    keys = {}

    def key_row(r):
        if r not in keys:
            keys[r] = K[r].tolist()
        return keys[r]

    for lo in range(G, N, batch):
        hi = min(N, lo + batch)
        chunk = [a for a in range(lo, hi) if live[a]]
        info["chunks"] += 1
        info["rows_added"] += len(chunk)
        info["rows_removed"] += (hi - lo) - len(chunk)
        # ---- step 1
        table = [np.asarray(x, np.int64) for x in lines]  # (the [lo][g_k] table: len(lines) == lo)
        new = {}
        for a in chunk:
            S = gc.seed_rows(seeds[a - G], live[:lo], id_base)  # (a seed naming a row >= lo is out of range)
            B, t, ex, ky, cp, _ = gc.walk(key_row(a), table, live, S, beam, width, max_iters)
            new[a] = [r for _, r in B[:g_k]]
            info["seeds"] += len(S); info["iterations"] += t; info["expanded"] += ex; info["keyed"] += ky; info["capped"] += cp
        lines += [new.get(a, []) for a in range(lo, hi)]
        if chunk:
            info["launches"] += 1 + (1 if lo else 0)  # the walk; the re-ranking where a row stands before the chunk
        # ---- step 2, literally
        named = {a: set(new[a]) for a in chunk}
        touched = {}
        for r in range(lo):
            if not live[r]:
                continue
            R = [a for a in chunk if r in named[a]]
            if not R:
                continue
            kr = key_row(r)
            Lp = [x for x in lines[r] if live[x]]
            cand = sorted(Lp + R, key=lambda x: (kr[x], x))
            lines[r] = cand[:g_k]
            touched[r] = (R, Lp)
            info["reverse_rows"] += 1
            info["reverse_offered"] += len(R)
            info["reverse_kept"] += sum(1 for x in lines[r] if x >= lo)
        if trace is not None:
            trace[lo] = touched
    return lines, info


def graph_arrays(lines, g_k, id_base, first_row=0, n=None):
    """zh_index_get_graph's answer for lines [first_row, first_row + n): (ids [n, g_k] u64, counts [n] u32)"""
    n = len(lines) - first_row if n is None else n
    ids, counts = np.full((n, g_k), NONE, np.uint64), np.zeros(n, np.uint32)
    for i in range(n):
        x = lines[first_row + i]
        ids[i, :len(x)] = np.asarray(x, np.uint64) + np.uint64(id_base)
        counts[i] = len(x)
    return ids, counts


def default_seeds(n_new, n_seed, g_rows, id_base):
    """LSHIndex.extend_graph's seeds=None: the strided rows of the graph before the call, the same for every new row"""
    return gc.default_seeds(n_new, n_seed, g_rows, id_base)


# ---------------------------------------------------------------------------------------------------------------- tables and cases
def removals(n, G):
    """-> (before the attach, after it): rc.removed_rows split so that old rows go at both times and every removed new row goes after the append"""
    r = rc.removed_rows(n)
    old = r[r < G]
    return old[::2], np.concatenate([old[1::2], r[r >= G]])


@functools.lru_cache(maxsize=None)
def table(tname, G, variant="plain"):
    """-> (X, live at the attach, live now).  plain: gsearch_cases' table.  copies: 20 new rows are copies of the block of identical rows, so that
    (key, id) ties decide lines and re-ranked lines.  hub: every new row is a near-copy of row 0.  none: nothing removed"""
    n, d = gc.TABLES[tname]
    X = rc.table(n, d).copy()
    if variant == "copies":
        X[G + 5:G + 25] = X[rc.BLOCK[0]]
    if variant == "hub":
        rng = np.random.default_rng([0x6E87, n, G])
        X[G:] = X[0] + (1e-3 * rng.standard_normal((n - G, d))).astype(np.float32)
    before, after = removals(n, G)
    live0, live1 = np.ones(n, bool), np.ones(n, bool)
    if variant not in ("hub", "none"):
        live0[before] = False
        live1[before] = False
        live1[after] = False
    for a in (X, live0, live1):
        a.setflags(write=False)
    return X, live0, live1


@functools.lru_cache(maxsize=None)
def keys_of(tname, G, variant, om, omode):
    K = key_matrix(table(tname, G, variant)[0], om, omode)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def start_graph(tname, G, variant, gname, g_k, id_base):
    """the graph over the first G rows that a case attaches: an entry of rc.GRAPHS, or "exact" (L2SQ, among the rows live at the attach)"""
    X, live0, _ = table(tname, G, variant)
    if gname == "exact":
        g = gc.exact_graph(X[:G], g_k, live0[:G], id_base, zo.L2SQ, 0)
    else:
        g = rc.GRAPHS[gname](G, g_k, live0[:G], id_base)
    for a in g:
        a.setflags(write=False)
    return g


def case_seeds(kind, n_new, n_seed, G, N, id_base):
    """default: LSHIndex.extend_graph's; random: per new row n_seed stored rows of ALL N drawn with replacement (removed rows, the row itself, rows of
    its chunk and later ones among them), a few ids out of range; hub: row 0 first, then the default's"""
    if kind == "default":
        return default_seeds(n_new, n_seed, G, id_base)
    if kind == "hub":
        s = default_seeds(n_new, n_seed, G, id_base).copy()
        s[:, 0] = id_base
        return s
    rng = np.random.default_rng([0x5EED5, n_new, n_seed, G, N])
    s = rng.integers(0, N, (n_new, n_seed)).astype(np.uint64) + np.uint64(id_base)
    s[np.arange(n_new), rng.integers(0, n_seed, n_new)] = np.arange(G, N, dtype=np.uint64) + np.uint64(id_base)  # every row names itself once
    bad = np.array([id_base + N, id_base + 2**32 + 1, 2**64 - 1] + ([0, id_base - 1] if id_base else []), np.uint64)
    m = rng.random(s.shape) < 0.1
    s[m] = bad[rng.integers(0, bad.size, int(m.sum()))]
    return s


# name -> (table, G, variant, graph, g_k, (oracle metric, mode), (beam, width, n_seed, max_iters), batch, id_base, seeds)
BIG = 2**40 + 3
L2 = (zo.L2SQ, 0)
CASES = {}
for _b in (1, 7, 64, 50, 128):  # one row a chunk, an odd size, a partial last chunk (100 = 64 + 36), an exact divisor, one chunk for all
    CASES["batch%d" % _b] = ("t600", 500, "plain", "exact", 32, L2, (64, 2, 32, 0), _b, BIG, "random")
CASES["t1500_batch64"] = ("t1500", 1200, "plain", "exact", 32, L2, (64, 1, 32, 0), 64, 0, "default")
CASES["t1500_batch512"] = ("t1500", 1200, "plain", "exact", 32, L2, (64, 4, 32, 0), 512, 0, "random")
for _g_k, _beam, _w in ((1, 1, 256), (1, 256, 1), (5, 5, 51), (5, 256, 2), (32, 32, 8), (64, 64, 4), (64, 256, 1)):  # g_k == beam, width g_k == 256, beam 256
    CASES["gk%d_beam%d_w%d" % (_g_k, _beam, _w)] = ("t600", 500, "plain", "exact", _g_k, L2, (_beam, _w, 16, 0), 37, 0, "random")
CASES["capped"] = ("t600", 500, "plain", "exact", 32, L2, (64, 1, 8, 3), 64, 0, "random")
CASES["copies"] = ("t600", 500, "copies", "block", 32, L2, (64, 2, 32, 0), 16, BIG, "random")
CASES["copies_one_chunk"] = ("t600", 500, "copies", "block", 32, L2, (64, 2, 32, 0), 128, 0, "random")
for _g in sorted(rc.GRAPHS):
    CASES["graph_" + _g] = ("t600", 500, "plain", _g, 32, L2, (64, 2, 32, 0), 64, BIG if len(_g) % 2 else 0, "random")
CASES["hub"] = ("t1500", 1200, "hub", "exact", 32, L2, (64, 1, 32, 0), 512, 0, "hub")
CASES["empty_start"] = ("t600", 0, "none", "exact", 5, L2, (8, 1, 4, 0), 200, 0, "random")  # G = 0: chunk 0 finds nothing, the later ones find it
DIM_CASES = {"d128": ("t600x128", L2), "d128_cos": ("t600x128", (zo.COSINE, zo.PARITY)), "d256": ("t600x256", L2),
             "d256_cos": ("t600x256", (zo.COSINE, zo.CORRECTED)), "d256_manhattan": ("t600x256", (zo.MANHATTAN, 0))}
for _n, (_t, _m) in DIM_CASES.items():
    CASES[_n] = (_t, 500, "plain", "exact", 32, _m, (64, 2, 32, 0), 64, BIG, "random")
HUB = "hub"


def metric_case(om, omode, tname="t600"):
    """every metric once: the generic dimension by default, the specialised load at t600x128"""
    return (tname, 500, "plain", "exact", 32, (om, omode), (64, 2, 32, 0), 64, 0, "random")


def inputs(case):
    """-> (X, live at the attach, live now, the attached graph, its kept lines, seeds)"""
    tname, G, variant, gname, g_k, _, (_, _, n_seed, _), _, id_base, skind = case
    X, live0, live1 = table(tname, G, variant)
    g = start_graph(tname, G, variant, gname, g_k, id_base)
    lines = kept_table(g, G, g_k, id_base, G, live0)
    return X, live0, live1, g, lines, case_seeds(skind, X.shape[0] - G, n_seed, G, X.shape[0], id_base)


@functools.lru_cache(maxsize=None)
def expected(case, with_trace=False):
    """-> (lines, info, (ids, counts) of get_graph(0, N)[, trace]) of a case, computed once"""
    tname, G, variant, _, g_k, (om, omode), (beam, width, _, max_iters), batch, id_base, _ = case
    _, _, live1, _, lines, seeds = inputs(case)
    trace = {} if with_trace else None
    out, info = extend(keys_of(tname, G, variant, om, omode), lines, live1, id_base, seeds, g_k, beam, width, max_iters, batch, trace)
    arrays = graph_arrays(out, g_k, id_base)
    for a in arrays:
        a.setflags(write=False)
    return (out, info, arrays, trace) if with_trace else (out, info, arrays)


# ---------------------------------------------------------------------------------------------------------------- quality (CPU only)
def overlap_with_exact(batch, g_k=32, G=1200):
    """t1500, nothing removed, L2SQ: the exact g_k-NN graph of the first G rows extended by the rest under the default settings; -> (the mean share
    of an extended line of a NEW row that the exact g_k-NN graph of all rows holds too, the same for the OLD rows)"""
    X, _, live = table("t1500", G, "none")
    K = keys_of("t1500", G, "none", zo.L2SQ, 0)
    n = X.shape[0]
    rows = np.arange(n)
    start = kept_table(gc.exact_graph(X[:G], g_k, live[:G], 0, zo.L2SQ, 0, K={a: K[a][:G] for a in range(G)}), G, g_k, 0, G, live)
    out, _ = extend(K, start, live, 0, default_seeds(n - G, 32, G, 0), g_k, 64, 1, 0, batch)
    share = np.zeros(n)
    for a in range(n):
        c = rows[rows != a]
        truth = set(c[np.lexsort((c, K[a][c]))[:g_k]].tolist())
        share[a] = len(truth & set(out[a])) / g_k
    return float(share[G:].mean()), float(share[:G].mean())

"""The plain reference of the filtered graph search tests (no GPU, no library: numpy, the oracle, and tests/gsearch_cases.py for the walk's parts,
tables, graphs and settings).

zh_search_graph_filtered_batch is zh_search_graph_batch's walk (gsearch_cases' docstring), untouched by the filter, and another answer.  With
K(q) = the rows that ever get a key (S(q) and every iteration's cand) and A = the stored rows r < n_bits whose filter bit is set and that are live:

    the answer = the first top_k by (key, id) of K(q) & A                                                           (the SET form)

The kernel cannot keep K(q); it keeps a list R of at most top_k (key, row) beside the beam and, after the seeds and after every iteration,

    R = the first top_k of R union ((the rows just keyed) & A minus the rows in R now)                              (the INCREMENTAL form)

There is no visited set, so a row of A can be offered again: it is in R now (dropped), or it was rejected by -- or pushed out of -- a full R, whose
last (key, id) never rises, and is rejected again.  reference() computes either form; tests/test_gfilter_reference.py asserts that they agree on
every case and pins a case where both kinds of re-offer happen; tests/test_gpu_gfilter.py runs the library against the set form."""
import numpy as np

from oracle import zebra_oracle as zo
from tests import gsearch_cases as gc
from tests.gsearch_cases import GRAPH_BATCH, NONE, kept_lines, seed_rows

# (beam, width, n_seed, max_iters, top_k): the GPU test's grid
SETTINGS = [(1, 1, 1, 0, 1), (8, 1, 8, 0, 8), (33, 2, 8, 0, 10), (64, 4, 32, 0, 10), (64, 1, 32, 0, 64), (256, 8, 32, 0, 256), (64, 1, 32, 3, 10)]


# ---------------------------------------------------------------------------------------------------------------- filters
def bitmap(mask, garbage=False):
    """a boolean mask over the first mask.size stored rows -> (words u32, n_bits), filter_bitmap's layout; garbage: the last word's bits past
    n_bits are set (the library must ignore them)"""
    mask = np.asarray(mask, bool).reshape(-1)
    by = np.packbits(mask, bitorder="little")
    words = np.concatenate([by, np.zeros(-by.size % 4, np.uint8)]).view(np.uint32).copy()
    if garbage and mask.size % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (mask.size % 32)) & 0xFFFFFFFF)
    return np.ascontiguousarray(words), int(mask.size)


def allowed_rows(words, n_bits, live):
    """A as a boolean array over the stored rows: bit set, below n_bits, live"""
    live = np.asarray(live, bool)
    bits = np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")[:n_bits].astype(bool)
    a = np.zeros(live.size, bool)
    a[:n_bits] = bits
    return a & live


def _one_row(n, live):
    m = np.zeros(n, bool)
    m[np.flatnonzero(live)[np.count_nonzero(live) // 2]] = True
    return bitmap(m)


def _short(n, live):
    rng = np.random.default_rng([0xF117E2, n])
    return bitmap(rng.random(n - 37) < 0.5, garbage=True)


# name -> f(n stored rows, live) -> (words, n_bits)
FILTERS = {"ones": lambda n, live: bitmap(np.ones(n, bool)),
           "zeros": lambda n, live: bitmap(np.zeros(n, bool)),
           "one_row": _one_row,
           "even": lambda n, live: bitmap(np.arange(n) % 2 == 0),
           "mod10_3": lambda n, live: bitmap(np.arange(n) % 10 == 3),
           "first_half": lambda n, live: bitmap(np.arange(n) < n // 2),
           "short_garbage": _short,  # n - 37 bits: no multiple of 32 for n = 600 and 1500
           "removed_only": lambda n, live: bitmap(~np.asarray(live, bool))}


def table_filter(tname, fname):
    X, live = gc.table(tname)
    return FILTERS[fname](X.shape[0], live)


# ---------------------------------------------------------------------------------------------------------------- the definition
def walk(keys, lines, live, S, beam, width, max_iters, allowed, top_k):
    """gsearch_cases.walk (the same lines, in the same order) with the incremental R beside it -> (R as [(key, row)], iterations, expanded, keyed,
    capped, K(q), offered, re-offers found in R, re-offers that had been rejected or pushed out)"""
    B = sorted((keys[r], r, False) for r in S)[:beam]
    seen = set(S)
    keyed, t, expanded, capped = len(S), 0, 0, 0
    R, offered_once = [], set()
    stats = [0, 0, 0]  # offered, again and in R, again and not in R

    def offer(rows):
        a = [r for r in rows if allowed[r]]
        stats[0] += len(a)
        in_r = {r for _, r in R}
        stats[1] += sum(1 for r in a if r in in_r)
        stats[2] += sum(1 for r in a if r not in in_r and r in offered_once)
        offered_once.update(a)
        return sorted(R + [(keys[r], r) for r in a if r not in in_r])[:top_k]

    R = offer(S)
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
        cand -= {e[1] for e in B}
        seen |= cand
        keyed += len(cand)
        expanded += len(P)
        B = sorted(B + [(keys[r], r, False) for r in cand])[:beam]
        R = offer(sorted(cand))
        t += 1
    return R, t, expanded, keyed, capped, seen, stats[0], stats[1], stats[2]


def reference(X, table_graph, g_rows, g_k, live, id_base, Q, seeds, top_k, beam, width, max_iters, om, omode, words, n_bits, attach_rows=None,
              form="set", reoffers=None):
    """the call's whole answer: (ids [b, top_k], keys [b, top_k], counts [b]) and the info dict (zh_graph_filtered_info's ten fields).  The
    arguments are gsearch_cases.reference's plus the filter; live is the live mask at the time of the SEARCH.  form "set": the first top_k of
    K(q) & A, K(q) from gsearch_cases.walk; "incremental": R as the kernel keeps it.  reoffers: a list that receives [in R, not in R] summed
    over the batch (incremental form)"""
    X, Q, live = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32), np.asarray(live, bool)
    seeds = np.asarray(seeds, np.uint64)
    b = Q.shape[0]
    lines = kept_lines(table_graph, g_rows, g_k, id_base, X.shape[0] if attach_rows is None else attach_rows)
    allowed = allowed_rows(words, n_bits, live)
    ids, keys, counts = np.full((b, top_k), NONE, np.uint64), np.full((b, top_k), NONE, np.uint64), np.zeros(b, np.uint32)
    info = {"queries": b, "seeds": 0, "iterations": 0, "expanded": 0, "keyed": 0, "capped": 0, "launches": -(-b // GRAPH_BATCH),
            "rows_allowed": int(np.count_nonzero(allowed)), "offered": 0, "returned": 0}
    again = [0, 0]
    for i in range(b):
        kq = np.asarray(zo.distance_batch(om, omode, X, Q[i]), np.uint64).tolist() if X.shape[0] else []
        S = seed_rows(seeds[i], live, id_base)
        R, t, ex, ky, cp, seen, off, a_in, a_out = walk(kq, lines, live, S, beam, width, max_iters, allowed, top_k)
        if form == "set":
            _, t2, ex2, ky2, cp2, seen2 = gc.walk(kq, lines, live, S, beam, width, max_iters)
            assert (t, ex, ky, cp, seen) == (t2, ex2, ky2, cp2, seen2)
            R = sorted((kq[r], r) for r in seen2 if allowed[r])[:top_k]
        else:
            assert form == "incremental"
        c = len(R)
        ids[i, :c] = np.array([r for _, r in R], np.uint64) + np.uint64(id_base)
        keys[i, :c] = np.array([k for k, _ in R], np.uint64)
        counts[i] = c
        info["seeds"] += len(S); info["iterations"] += t; info["expanded"] += ex; info["keyed"] += ky; info["capped"] += cp
        info["offered"] += off; info["returned"] += c
        again[0] += a_in; again[1] += a_out
    if reoffers is not None:
        reoffers.extend(again)
    return (ids, keys, counts), info


def run_case(tname, gname, g_k, b, setting, fname, form="set", id_base=0, reoffers=None):
    """a case under the default seeds, L2SQ -> reference()'s return"""
    X, live = gc.table(tname)
    beam, width, n_seed, max_iters, top_k = setting
    words, n_bits = table_filter(tname, fname)
    return reference(X, gc.graph(tname, gname, g_k, id_base), X.shape[0], g_k, live, id_base, gc.queries(tname, b),
                     gc.default_seeds(b, n_seed, X.shape[0], id_base), top_k, beam, width, max_iters, zo.L2SQ, 0, words, n_bits, form=form,
                     reoffers=reoffers)

"""The kind x dimension dispatch table of the canonical-row kernels, restated, and the cells that walk all of it (no GPU, no library: numpy, the
oracle and the sibling *_cases.py modules).

zh_dispatch_kind_dim (zebra_amd/csrc/zh_device.h) picks the instantiation <D, KIND> of eight kernel templates -- exact_score_kernel,
refine_line_kernel, nnd_line_kernel, prune_line_kernel, gsearch_kernel, gsearch_filtered_kernel, gsearch_steered_kernel, gext_rerank_kernel -- from
the metric and the dimension: thirteen metric forms fall into ten kinds; d = 128 / 384 / 768 has an instantiation of its own for every kind,
d = 256 / 512 / 1024 for K_L2 and K_COS only, and every other (kind, d) takes the generic row loop D = 0.  That is 46 pairs (kind, D).
instantiation() is that rule written down a second time, from the header's comment and code; tests/test_dispatch_cases.py holds it against a
table typed out by hand.

CELLS are the (d, metric) pairs tests/test_gpu_dispatch_table.py runs through all eight kernels: all thirteen metrics at the six specialised
dimensions, and at each of ten generic dimensions (1 and 3, one element beside a specialised dimension, above 1024) L2 squared, parity cosine and
three of the other eleven in rotation.  coverage(CELLS) is all 46 pairs.

A cell's inputs are the siblings': refine_cases.table(300, d) with refine_cases.removed_rows removed, the ring graph at in_k = 8, five queries
with eight seeds each, gfilter_cases' "short_garbage" filter (263 bits, half of them set), and for the extension gextend_cases' protocol with the
ring over the first 200 rows attached and 100 rows appended, rows removed before the attach, after it, and among the appended ones.  Exact
zeros in rows and queries are replaced as family_cases._no_zero does (two zeros in one column are a NaN under Canberra), and keys() asserts that no
reference key of a cell is a NaN."""
import functools

import numpy as np

from oracle import zebra_oracle as zo
from tests import descent_cases as dc
from tests import gextend_cases as ge
from tests import gfilter_cases as fc
from tests import gsearch_cases as gc
from tests import gsteer_cases as sc
from tests import prune_cases as pc
from tests import refine_cases as rc

# ---------------------------------------------------------------------------------------------------------------- the dispatch, restated
KINDS = ("K_L2", "K_COS", "K_MAX", "K_CANB", "K_BRAY", "K_ABS", "K_P3", "K_P4", "K_HAMM", "K_PP")
# name -> (oracle metric, oracle mode or power, kind), in the order of tests.test_gpu_fknn.thirteen_metrics
METRICS = {"l2sq": (zo.L2SQ, 0, "K_L2"), "l2": (zo.L2, 0, "K_L2"), "cosine": (zo.COSINE, zo.PARITY, "K_COS"),
           "cosine_corrected": (zo.COSINE, zo.CORRECTED, "K_COS"), "chebyshev": (zo.CHEBYSHEV, 0, "K_MAX"), "canberra": (zo.CANBERRA, 0, "K_CANB"),
           "bray_curtis": (zo.BRAY_CURTIS, 0, "K_BRAY"), "manhattan": (zo.MANHATTAN, 0, "K_ABS"), "l3": (zo.L3, 0, "K_P3"), "l4": (zo.L4, 0, "K_P4"),
           "hamming": (zo.HAMMING, 0, "K_HAMM"), "minkowski3": (zo.MINKOWSKI, 3, "K_PP"), "pnorm65": (zo.PNORM, 65, "K_PP")}
NAMES = tuple(METRICS)
EVERY_KIND_DIMS = (128, 384, 768)    # an instantiation for every kind
SIMSIMD_DIMS = (256, 512, 1024)      # one for K_L2 and K_COS only


def instantiation(metric_name, d):
    """-> (kind, D) of the instantiation zh_dispatch_kind_dim gives a call under this metric at dimension d; D = 0 is the generic row loop"""
    kind = METRICS[metric_name][2]
    if d in EVERY_KIND_DIMS or (d in SIMSIMD_DIMS and kind in ("K_L2", "K_COS")):
        return kind, d
    return kind, 0


ALL_PAIRS = frozenset([(k, D) for k in KINDS for D in (0,) + EVERY_KIND_DIMS] + [(k, D) for k in ("K_L2", "K_COS") for D in SIMSIMD_DIMS])

# ---------------------------------------------------------------------------------------------------------------- the cells
SPECIALISED = (128, 256, 384, 512, 768, 1024)
GENERIC = (1, 3, 127, 129, 257, 383, 385, 769, 1025, 1500)
ALWAYS = ("l2sq", "cosine")
# the other eleven, 30 places over them: two or three each.  The rotation starts at Chebyshev so that corrected cosine does not fall on d = 1: there
# its keys are +0.0 and 2.0 only, no key_p(c) is ever below key_a(c), and the occlusion rule the pruning cell must show drops nothing BY DEFINITION
# (parity cosine, which every generic dimension has, orders -1.0 above +1.0 as u64 and does occlude at d = 1)
ROTATED = NAMES[4:] + ("l2", "cosine_corrected")


def generic_metrics(i):
    """the metrics of the i-th generic dimension: L2 squared, parity cosine, and places 3 i .. 3 i + 2 of the rotation"""
    return ALWAYS + tuple(ROTATED[(3 * i + j) % len(ROTATED)] for j in range(3))


CELLS = [(d, m) for d in SPECIALISED for m in NAMES] + [(d, m) for i, d in enumerate(GENERIC) for m in generic_metrics(i)]
CELLS.sort(key=lambda c: c[0])  # (dimension by dimension: one shared index at a time; sorted() is stable, a dimension's metrics keep their order)


def cell_id(cell):
    return "d%d-%s" % cell


def coverage(cells):
    """the set of (kind, D) the cells reach"""
    return {instantiation(m, d) for d, m in cells}


# ---------------------------------------------------------------------------------------------------------------- a cell's inputs
N, IN_K, K = 300, 8, 8
B, N_SEED, TOP_K, BEAM, WIDTH, HOPS = 5, 8, 10, 33, 2, 2
ROUNDS, REV_K = 3, 4                        # the descent; REV_K is the prune's reverse width as well
PRUNE_IN_K, DEGREE = 16, 8
G, X_BEAM, X_WIDTH, X_BATCH = 200, 16, 2, 32  # the extension: 100 new rows in chunks of 32, 32, 32 and 4


def _no_zero(A):
    A[A == 0] = np.float32(2.0**-20)
    return A


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def live_rows():
    """the live mask of every cell's table: rc.removed_rows removed"""
    live = np.ones(N, bool)
    live[rc.removed_rows(N)] = False
    return _frozen(live)


@functools.lru_cache(maxsize=None)
def table(d):
    """-> (X [300, d] with the 40 identical rows of rc.BLOCK, the live mask)"""
    return _frozen(_no_zero(rc.table(N, d))), live_rows()


@functools.lru_cache(maxsize=None)
def ring():
    """the ring graph over all 300 rows (the same at every d)"""
    return _frozen(*rc.g_ring(N, IN_K, live_rows(), 0))


@functools.lru_cache(maxsize=None)
def queries(d):
    """-> (Q [5, d], seeds [5, 8]) as tests/test_gpu_graph_dims.py draws them"""
    Q = _no_zero(zo.synth_queries(B, d, N).copy())
    seeds = np.random.default_rng([0xD135, d]).integers(0, N, (B, N_SEED)).astype(np.uint64)
    return _frozen(Q, seeds)


@functools.lru_cache(maxsize=None)
def filter_words():
    """-> (words, n_bits, the boolean mask over the first n_bits rows): n_bits = 263 is no multiple of 32, the last word carries garbage"""
    words, n_bits = fc.FILTERS["short_garbage"](N, live_rows())
    mask = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits].astype(bool)
    return _frozen(words), n_bits, _frozen(mask)


@functools.lru_cache(maxsize=None)
def extension():
    """-> (live at the attach, live now, the ring over the first 200 rows, its kept lines, seeds [100, 8]); the same at every d"""
    before, after = ge.removals(N, G)
    live0, live1 = np.ones(N, bool), np.ones(N, bool)
    live0[before] = False
    live1[before] = False
    live1[after] = False
    assert (~live1[G:]).any() and (~live0[:G]).any() and (live0[:G] & ~live1[:G]).any()
    g = rc.g_ring(G, IN_K, live0[:G], 0)
    lines = ge.kept_table(g, G, IN_K, 0, G, live0)
    seeds = ge.case_seeds("random", N - G, N_SEED, G, N, 0)
    _frozen(live0, live1, seeds, *g)
    return live0, live1, g, lines, seeds


def key_is_nan(keys, om):
    """family_cases.key_is_nan: the simsimd kinds' keys are f64 bits, Hamming's a count, the others' f32 bits widened"""
    keys = np.asarray(keys, np.uint64)
    if om in (zo.COSINE, zo.L2SQ, zo.L2):
        return np.isnan(keys.view(np.float64))
    if om == zo.HAMMING:
        return np.zeros(keys.shape, bool)
    return np.isnan(keys.astype(np.uint32).view(np.float32))


@functools.lru_cache(maxsize=4)
def keys(d, mname):
    """-> (K, KQ): K[a] = the oracle's keys of every stored row against stored row a (rc.key_rows of all 300), KQ [5, 300] the same against the
    cell's queries; once per cell, and no key may be a NaN"""
    om, omode, _ = METRICS[mname]
    X = table(d)[0]
    K = rc.key_rows(X, om, omode, range(N))
    KQ = np.stack([np.asarray(zo.distance_batch(om, omode, X, q), np.uint64) for q in queries(d)[0]])
    for a in K.values():
        a.setflags(write=False)
    assert not any(key_is_nan(a, om).any() for a in K.values()) and not key_is_nan(KQ, om).any(), \
        "a reference key of cell %s is a NaN: change the cell's rows, do not drop the cell" % cell_id((d, mname))
    return K, _frozen(KQ)


# ---------------------------------------------------------------------------------------------------------------- a cell's references
def expected(d, mname):
    """the numpy references of the seven graph kernels at one cell, each its own module's -> {name: (answer, info)}; the exact search is checked
    by tests.test_gpu_exact.check_exact against the oracle's brute force"""
    om, omode, _ = METRICS[mname]
    X, live = table(d)
    graph = ring()
    Q, seeds = queries(d)
    words, n_bits, _ = filter_words()
    Kd, _ = keys(d, mname)
    out = {}
    out["refine"] = rc.reference(X, graph, IN_K, K, live, 0, om, omode, K=Kd)
    ref, info, _, _ = dc.descent(X, graph, IN_K, REV_K, K, ROUNDS, live, 0, om, omode, Kd)
    out["descent"] = (ref, info)
    start = pc.exact_graph(Kd, live, 0, PRUNE_IN_K)
    prep = pc.prepare(X, start, PRUNE_IN_K, REV_K, live, 0, om, omode, Kd)
    out["prune"] = pc.reference(prep, N, DEGREE, 0, live, 0) + (start, prep)
    out["gsearch"] = gc.reference(X, graph, N, IN_K, live, 0, Q, seeds, TOP_K, BEAM, WIDTH, 0, om, omode)
    out["gfilter"] = fc.reference(X, graph, N, IN_K, live, 0, Q, seeds, TOP_K, BEAM, WIDTH, 0, om, omode, words, n_bits)
    out["gsteer"] = sc.reference(X, graph, N, IN_K, live, 0, Q, seeds, TOP_K, BEAM, WIDTH, 0, om, omode, words, n_bits, HOPS)
    _, live1, _, lines, xseeds = extension()
    Km = np.stack([Kd[r] for r in range(N)])
    trace = {}
    xlines, xinfo = ge.extend(Km, lines, live1, 0, xseeds, IN_K, X_BEAM, X_WIDTH, 0, X_BATCH, trace)
    out["gextend"] = (ge.graph_arrays(xlines, IN_K, 0), xinfo, trace)
    return out

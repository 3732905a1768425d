"""tests/seam_cases.py pinned on the CPU: on a table of 5 x 97 + 40 rows with removed rows and the adversarial lines, the local reference of every
group is the existing whole-table reference's answer on that group's lines -- refinement, refinement with reverse neighbours, the reverse graph,
descent, graph search and filtered graph search; the row offset of tests/reverse_cases.py at 0 changes nothing; the sizes the GPU tests cross are
the library's, parsed from its sources; and 97 divides none of them.  No GPU, no library."""
import os
import re

import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import descent_cases as dc
from tests import gfilter_cases as gf
from tests import gsearch_cases as gc
from tests import refine_cases as rc
from tests import reverse_cases as rv
from tests import seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, IN_K = 5 * sc.P + 40, 30, 3
POSITIONS = (2 * sc.P + 50, 4 * sc.P + 7)  # stand-ins for seam positions: rows s - 1, s, s + 1 are removed
METRICS = {"l2sq": (zo.L2SQ, 0), "cos": (zo.COSINE, zo.PARITY), "manhattan": (zo.MANHATTAN, 0)}


def small(id_base=sc.ID_BASE, in_k=IN_K):
    """-> (table, X, graph): every group but the first adversarial, group 5 partial"""
    tb = sc.Table(N, D, id_base, sc.removed(N, POSITIONS))
    ids, counts = sc.graph(N, in_k, id_base)
    changed = sc.adversarial(ids, counts, N, id_base, tb.live, range(1, sc.groups(N)))
    assert len(changed) >= 5 * 4 and (~tb.live).sum() >= 8
    return tb, zo.synth_rows(N, D), (ids, counts)


def lines_equal(got, want, s, e, what):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b[s:e].shape and (a == b[s:e]).all(), what


def test_the_table_is_what_the_references_rest_on():
    tb, X, (ids, counts) = small()
    assert sc.groups(N) == 6 and tb.span(5) == (5 * sc.P, N)
    for g in range(6):
        s, e = tb.span(g)
        assert (tb.rows(g).view(np.uint32) == X[s:e].view(np.uint32)).all()
        tb.local(ids[s:e], counts[s:e], g)  # (asserts that no line leaves its group)
    past = ids[5 * sc.P:] - np.uint64(sc.ID_BASE) >= np.uint64(N)
    assert past.any() and not (ids[:5 * sc.P] - np.uint64(sc.ID_BASE) >= np.uint64(N))[ids[:5 * sc.P] != sc.NONE].any()  # the last group names rows past the table
    gone = set(tb.gone.tolist())
    assert all(r in gone for s in POSITIONS for r in (s - 1, s, s + 1)) and 5 * sc.P + (5 * 7 + 3) % sc.P in gone
    assert counts[sc.P + 3] == 0 and ids[sc.P + 11, 0] == sc.NONE and ids[sc.P + 23, 2] == ids[sc.P + 23, 0] and ids[sc.P + 52, 0] == sc.ID_BASE + sc.P + 52
    assert not tb.live[int(ids[2 * sc.P + 37, 0]) - sc.ID_BASE]
    assert len(set(sc.OFFSETS)) == sc.P - 1 and 0 not in sc.OFFSETS


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("rev_k", [0, 4])
def test_local_refinement_is_the_whole_tables(metric, rev_k):
    tb, X, graph = small()
    om, omode = METRICS[metric]
    for k in (16, 2):
        if rev_k:
            want, winfo = rv.reference_rev(X, graph, IN_K, rev_k, k, tb.live, sc.ID_BASE, om, omode)
        else:
            want, winfo = rc.reference(X, graph, IN_K, k, tb.live, sc.ID_BASE, om, omode)
        total = {f: 0 for f in ("lines", "listed", "keyed", "updates") + (("kept", "edges") if rev_k else ())}
        for g in range(sc.groups(N)):
            s, e = tb.span(g)
            got, info = sc.local_refine(tb, graph[0][s:e], graph[1][s:e], g, k, om, omode, rev_k)
            lines_equal(got, want, s, e, (metric, rev_k, k, g))
            for f in total:
                total[f] += info[f]
        assert total == {f: winfo[f] for f in total}  # (the groups partition the table's edges too)
        assert winfo["updates"] > 0 and winfo["keyed"] > winfo["lines"]


@pytest.mark.parametrize("in_k,rev_k", [(3, 4), (3, 1), (64, 8)])
def test_local_reverse_is_the_whole_tables(in_k, rev_k):
    tb, X, graph = small(in_k=in_k)
    want, winfo = rv.reference_reverse(graph, in_k, rev_k, tb.live, sc.ID_BASE)
    kept = 0
    for g in range(sc.groups(N)):
        s, e = tb.span(g)
        got, info = sc.local_reverse(tb, graph[0][s:e], graph[1][s:e], g, rev_k)
        lines_equal(got, want, s, e, (in_k, rev_k, g))
        kept += info["kept"]
    assert kept == winfo["kept"] > 0
    # the hash is of the absolute rows: a local reference without the offset picks other members where a line has to choose
    if rev_k < in_k:
        s, e = tb.span(3)
        lg = tb.local(graph[0][s:e], graph[1][s:e], 3)
        unshifted, _ = rv.reference_reverse(lg, in_k, rev_k, tb.live[s:e], 0)
        assert (tb.rebase(unshifted[0], 3) != want[0][s:e]).any()


@pytest.mark.parametrize("rev_k", [0, 4])
def test_local_descent_is_the_whole_tables(rev_k):
    tb, X, graph = small()
    om, omode = METRICS["l2sq"]
    k, rounds = 8, 3
    want, winfo, full, _ = dc.descent(X, graph, IN_K, rev_k, k, rounds, tb.live, sc.ID_BASE, om, omode)
    assert winfo["rounds_run"] == rounds and len(full) == rounds
    for g in range(sc.groups(N)):
        s, e = tb.span(g)
        for r in (1, rounds):
            got = sc.local_descent(tb, graph[0][s:e], graph[1][s:e], g, rev_k, k, r, om, omode)
            lines_equal(got, full[r - 1], s, e, (rev_k, g, r))


def search_case(tb):
    """two queries per group, each seeded inside it (one seed of four is a removed row or a row of the table's far end: ignored or out of range)"""
    G = sc.groups(N)
    Q = zo.synth_queries(2 * G, D, N)
    seeds = np.empty((2 * G, 4), np.uint64)
    for i in range(2 * G):
        s, e = tb.span(i // 2)
        seeds[i] = [s + (7 * i + 1) % (e - s), s + (11 * i + 5) % (e - s), s + (13 * i + 2) % (e - s), sc.ID_BASE + N + i]
        seeds[i, :3] += np.uint64(sc.ID_BASE)
    return Q, seeds


@pytest.mark.parametrize("filtered", [False, True])
def test_local_search_is_the_whole_tables(filtered):
    tb, X, graph = small()
    om, omode = METRICS["l2sq"]
    Q, seeds = search_case(tb)
    allowed = np.arange(N) % 2 == 0
    top_k, beam, width, max_iters = 10, 64, 2, 0
    if filtered:
        words, n_bits = gf.bitmap(allowed)
        want, winfo = gf.reference(X, graph, N, IN_K, tb.live, sc.ID_BASE, Q, seeds, top_k, beam, width, max_iters, om, omode, words, n_bits)
    else:
        want, winfo = gc.reference(X, graph, N, IN_K, tb.live, sc.ID_BASE, Q, seeds, top_k, beam, width, max_iters, om, omode)
    fields = ("seeds", "iterations", "expanded", "keyed") + (("offered", "returned") if filtered else ())
    total = {f: 0 for f in fields}
    for g in range(sc.groups(N)):
        s, e = tb.span(g)
        got, info = sc.local_search(tb, graph[0][s:e], graph[1][s:e], g, Q[2 * g:2 * g + 2], seeds[2 * g:2 * g + 2], top_k, beam, width, max_iters, om, omode,
                                    allowed if filtered else None)
        lines_equal(got, want, 2 * g, 2 * g + 2, (filtered, g))
        for f in fields:
            total[f] += info[f]
    assert total == {f: winfo[f] for f in fields} and winfo["iterations"] > 2 * sc.groups(N) and (want[2] > 0).all()


def test_row_offset_zero_is_the_pinned_reference():
    """the offset's default and an explicit 0 give what tests/test_reverse_reference.py pins; the hash itself is untouched"""
    from tests.test_refine_reference import ID_BASE, N as N60, small as small60
    X, live = small60()
    for name in ("hub", "orphan", "capped"):
        graph = rv.ALL_GRAPHS[name](N60, 5, live, ID_BASE)
        Ns = rc.neighbour_sets(graph[0], graph[1], 5, live, ID_BASE)
        In = rv.in_neighbours(Ns, live)
        for a, b in zip(rv.reverse_sets(Ns, In, 3), rv.reverse_sets(Ns, In, 3, 0)):
            assert (a == b).all()
        for a, b in zip(rv.reference_reverse(graph, 5, 3, live, ID_BASE)[0], rv.reference_reverse(graph, 5, 3, live, ID_BASE, row0=0)[0]):
            assert (a == b).all()
        one, oinfo = rv.reference_rev(X, graph, 5, 3, 6, live, ID_BASE, zo.L2SQ, 0)
        two, tinfo = rv.reference_rev(X, graph, 5, 3, 6, live, ID_BASE, zo.L2SQ, 0, row0=0)
        assert oinfo == tinfo and all((a == b).all() for a, b in zip(one, two))
    assert int(rv.h(12345, 678)) == 0x44199268


def source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_seams_are_the_librarys():
    """a later change of one of these constants must fail HERE, not let a GPU test silently stop crossing its seam"""
    pub, internal = source("include", "zebra_hip.h"), source("zebra_amd", "csrc", "zh_internal.h")
    api, reverse = source("zebra_amd", "csrc", "zh_api.hip"), source("zebra_amd", "csrc", "zh_reverse.hip")
    assert int(re.search(r"#define ZH_GRAPH_BATCH (\d+)u", pub).group(1)) == sc.GRAPH_BATCH == gc.GRAPH_BATCH
    assert int(re.search(r"#define ZH_REFINE_SLAB (\d+)u", internal).group(1)) == sc.REFINE_SLAB
    assert 1 << int(re.search(r"#define ZH_LINES_PER_LAUNCH \(1ull << (\d+)\)", internal).group(1)) == sc.LINES_PER_LAUNCH
    assert re.search(r"zh_line_launches\(uint64_t n\) \{ return \(n \+ ZH_LINES_PER_LAUNCH - 1\) / ZH_LINES_PER_LAUNCH; \}", internal)
    assert 1 << int(re.search(r"const uint64_t step = \(1ull << (\d+)\) / in_k;", reverse).group(1)) == sc.CSR_ENTRIES
    m = re.search(r"refine_host_slab\(size_t k\) \{ return std::max<uint64_t>\(ZH_REFINE_SLAB, \(uint64_t\(1\) << (\d+)\) / k / ZH_REFINE_SLAB \* ZH_REFINE_SLAB\); \}", api)
    assert 1 << int(m.group(1)) == sc.HOST_ENTRIES
    m = re.search(r"piece = std::min<uint64_t>\(n, std::max<uint64_t>\(ZH_REFINE_SLAB, \(uint64_t\(1\) << (\d+)\) / rev_k\)\);", api)
    assert 1 << int(m.group(1)) == sc.HOST_ENTRIES
    m = re.search(r"static uint64_t refine_chunk_bytes\(\) \{\n    uint64_t chunk = (\d+)ull << (\d+);", api)
    assert int(m.group(1)) << int(m.group(2)) == sc.REFINE_CHUNK_BYTES  # (seam 6: the host graph of tests/test_gpu_large_table.py spans five)
    assert sc.host_piece(512) == 65536 and sc.host_piece(64) == sc.reverse_piece(64) == 524288 and sc.host_piece(8) == 2**22
    assert sc.CSR_ENTRIES // 64 == sc.LINES_PER_LAUNCH  # (the edge passes at in_k = 64 are cut where the line kernels are)


def test_no_seam_is_a_multiple_of_the_group():
    sizes = sorted(set(sc.SEAMS) | {sc.host_piece(512), sc.host_piece(64), sc.reverse_piece(64)})
    assert sizes == [16384, 65536, 524288, 2**24]
    for a in sizes:
        assert a % sc.P, a
        for b in sizes:
            if a != b:
                assert (a - b) % sc.P, (a, b)
    assert 16384 % 257 == 193 and all(257 % p for p in range(2, 17))  # seam 3's query block: 257 is prime, a batch starts 193 queries into it


def test_descent_launch_terms():
    live = np.ones(593957, bool)
    assert sc.descent_launches(593957, live, 3, 0, 64, 2, True) == 10 + 2 + 4 + 2 and sc.descent_launches(593957, live, 3, 0, 64, 2, False) == 10 + 2 + 4 + 1
    live = np.ones(135205, bool)
    assert sc.descent_launches(135205, live, 3, 4, 8, 3, False) == (2 + 6) + 3 + 1 + 2 * ((2 + 6) + 2 + 1) + 1


def test_sub_slab_counts():
    live = np.ones(135205, bool)
    assert sc.sub_slabs(0, 135205, live) == 3 and sc.sub_slabs(60000, 70000, live) == 2 and sc.sub_slabs(60000, 69669, live, sc.host_piece(512)) == 2
    live[65536:131072] = False
    assert sc.sub_slabs(0, 135205, live) == 2
    assert sc.sub_slabs(0, 593957, np.ones(593957, bool), sc.host_piece(64)) == 10 and sc.line_launches(2**24 + 1) == 2

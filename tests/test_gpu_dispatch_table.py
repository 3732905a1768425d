"""The whole kind x dimension table of zh_dispatch_kind_dim, walked by construction through every kernel on it: one test per cell of
tests/dispatch_cases.CELLS (128 cells: all 13 metric forms at d = 128 / 256 / 384 / 512 / 768 / 1024, and L2 squared, parity cosine and three of
the other eleven in rotation at d = 1, 3, 127, 129, 257, 383, 385, 769, 1025, 1500), each running all eight kernel templates on the cell's 300-row
index -- exact_score_kernel, refine_line_kernel, nnd_line_kernel, prune_line_kernel, gsearch_kernel, gsearch_filtered_kernel,
gsearch_steered_kernel, gext_rerank_kernel: 46 instantiations (kind, D) of each, 368 in all (tests/test_dispatch_cases.py asserts the 46).

Everything is compared bit for bit on ids, keys and counts -- integer keys under the order contract, no tolerance -- with the reference the
kernel's own module uses (dispatch_cases.expected), and every info struct with what that module asserts about it.  A dimension that reached
another dimension's instantiation reads rows at the wrong stride INSIDE the allocation and returns plausible keys; a slip in one
row_pair_sums<D, KIND> tail changes the keys of one cell.  Neither faults; only a cell of its own notices.

One index per dimension is shared by the dimension's metrics (the ring graph attached; no test changes it); the extension changes its index and
gets a fresh one per cell.

What the module sees, measured on mutants of the library (built one at a time on a copy of the tree, none committed):
  (a) zh_dispatch_dim sends d = 384 under K_CANB to the D = 128 instantiation (rows read at a stride of 128 floats, inside the allocation):
      test_gpu_graph_dims, test_gpu_refine, test_gpu_descent, test_gpu_prune, test_gpu_gsearch, test_gpu_gfilter, test_gpu_gsteer and
      test_gpu_gextend all pass (18 + 117 + 54 + 117 + 75 + 71 + 84 + 55 tests); this module fails in d384-canberra and nowhere else, and
      there in all eight kernels (the exact search's first id, 1894 to 2015 ids of the line kernels' answers, 49 or 50 of the walks' 50).
  (b) zh_dispatch_dim sends d = 768 under K_HAMM to the generic D = 0: the same eight modules pass AND SO DOES THIS ONE, 128 of 128.  The generic
      row loop and a specialised load compute the same canonical sums in the same order by design, so no key changes: a call that
      should have had an instantiation of its own and got the generic loop is slower, not wrong, and no comparison of answers can tell.  Of the
      D = 0 column the table therefore distinguishes the arithmetic of lane_sums_generic<KIND> per kind (odd d, d beside a specialised one,
      d > 1024), not WHICH dimensions are routed to it; what it does tell apart is every specialised D from every other specialised D.
  (c) row_pair_sums<384, K_P3> leaves the last lane of its partial piece out (REM4 - 1 for that one pair): the same eight modules pass; this
      module fails in d384-l3 and nowhere else.

Measured on an MI355X: 128 passed in 22.4 s of wall time, the references included; the slowest test is d1-l2sq at 0.37 s (the first: it loads the
libraries), then d385-pnorm65 at 0.32 s."""
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dispatch_cases as dcs  # noqa: E402
from tests.test_gpu_descent import info_is as descent_info_is  # noqa: E402
from tests.test_gpu_exact import check_exact  # noqa: E402
from tests.test_gpu_fknn import thirteen_metrics  # noqa: E402
from tests.test_gpu_gextend import same_graph  # noqa: E402
from tests.test_gpu_gfilter import WALK_FIELDS  # noqa: E402
from tests.test_gpu_prune import info_is as prune_info_is  # noqa: E402
from tests.test_gpu_refine import info_is as refine_info_is, same  # noqa: E402


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


_SHARED = {}  # d -> the shared index of the dimension; no test changes one


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for ix in _SHARED.values():
        ix.close()
    _SHARED.clear()
    dcs.keys.cache_clear()


def new_index(za, d):
    return za.LSHIndex(d, za.LSHIndexOptions(64, 3), device=0)


def remove(ix, rows):
    rows = np.asarray(rows, np.int64)
    if rows.size:
        assert ix.remove(rows.astype(np.uint64)).size == rows.size


def index(za, d):
    if d not in _SHARED:
        X, live = dcs.table(d)
        ix = new_index(za, d)
        ix.append(X)
        remove(ix, np.flatnonzero(~live))
        ix.set_graph(dcs.ring())
        _SHARED[d] = ix
    return _SHARED[d]


def metric(za, mname):
    """the library's metric object of a cell, held against dispatch_cases' oracle constants"""
    m, om, omode = thirteen_metrics(za)[dcs.NAMES.index(mname)]
    assert (om, omode) == dcs.METRICS[mname][:2], mname
    return m, om, omode


def failure_text(e):
    """a caught assertion as the log needs it: file, line and source text of the frames from the stage down to the assert that failed (a sibling's
    helper such as check_exact raises with a bare query number for a message), then the message itself"""
    frames = traceback.extract_tb(e.__traceback__)[1:]  # ([0] is test_cell's own `stage()`)
    where = "".join("  %s:%d in %s: %s\n" % (f.filename.rsplit("/", 1)[-1], f.lineno, f.name, f.line) for f in frames)
    return where + "  AssertionError: " + str(e)[:1500]


@pytest.mark.parametrize("d,mname", dcs.CELLS, ids=[dcs.cell_id(c) for c in dcs.CELLS])
def test_cell(za, d, mname):
    """all eight kernels at one cell; a kernel that differs does not hide the ones behind it: the failure names every kernel that does"""
    what = dcs.cell_id((d, mname))
    ix = index(za, d)
    m, om, omode = metric(za, mname)
    X, live = dcs.table(d)
    graph = dcs.ring()
    Q, seeds = dcs.queries(d)
    words, n_bits, mask = dcs.filter_words()
    exp = dcs.expected(d, mname)

    def exact():  # path 1 of the exact search against the oracle's brute force
        got = ix.search_exact_batch(Q, dcs.TOP_K, m)
        assert ix.exact_info()["path"] == 1 and ix.exact_info()["rows_live"] == int(live.sum()), what
        check_exact(got, X[live], Q, dcs.TOP_K, om, omode, ids_of=np.flatnonzero(live))

    def refine():  # one round against the definition
        ref, rinfo = exp["refine"]
        same(ix.knn_graph_refine(graph, dcs.K, m), ref, what + ": refine")
        refine_info_is(ix, rinfo, live, dcs.IN_K, dcs.K, what)

    def descent():  # rounds 2 and 3 on the device against the host's loop of full rounds and against the numpy reference
        got = ix.knn_graph_descent(graph, dcs.K, m, rounds=dcs.ROUNDS, reverse=dcs.REV_K)
        dinfo = ix.knn_descent_info()
        same(got, ix.knn_graph_refine(graph, dcs.K, m, rounds=dcs.ROUNDS, reverse=dcs.REV_K), what + ": descent (the loop)")
        ref, rinfo = exp["descent"]
        same(got, ref, what + ": descent (numpy)")
        assert ix.knn_descent_info() == dinfo and dinfo["rounds_run"] >= 2, what  # (the ring at in_k = 8 does not converge in one round)
        descent_info_is(ix, rinfo, live, dcs.IN_K, dcs.REV_K, dcs.K, dcs.ROUNDS, what)

    def prune():  # the cell's exact 16-NN graph under its own keys, pruned to 8 with 4 reverse neighbours
        ref, rinfo, start, prep = exp["prune"]
        same(ix.knn_graph_prune(start, dcs.DEGREE, m, reverse=dcs.REV_K), ref, what + ": prune")
        pinfo = prune_info_is(ix, rinfo, prep, live, dcs.PRUNE_IN_K, dcs.REV_K, dcs.DEGREE, 0, what=what)
        assert pinfo["occluded"] > 0 and pinfo["kept"] > 0, what  # both branches of the rule

    def gsearch():  # the walk over the attached ring
        ref, rinfo = exp["gsearch"]
        same(ix.search_graph_batch(Q, dcs.TOP_K, m, beam=dcs.BEAM, width=dcs.WIDTH, seeds=seeds), ref, what + ": graph search")
        assert ix.search_graph_info() == rinfo, (what, ix.search_graph_info(), rinfo)

    def gfilter():  # the same walk, answered from the allowed rows; its figures are the unfiltered call's
        ref, rinfo = exp["gfilter"]
        same(ix.search_graph_filtered_batch(Q, dcs.TOP_K, m, mask, beam=dcs.BEAM, width=dcs.WIDTH, seeds=seeds), ref, what + ": filtered graph search")
        finfo = ix.search_graph_filtered_info()
        assert finfo == rinfo and {f: finfo[f] for f in WALK_FIELDS} == exp["gsearch"][1], (what, finfo, rinfo)

    def gsteer():  # the walk that sees the filter, two hops
        ref, rinfo = exp["gsteer"]
        same(ix.search_graph_steered_batch(Q, dcs.TOP_K, m, mask, hops=dcs.HOPS, beam=dcs.BEAM, width=dcs.WIDTH, seeds=seeds), ref,
             what + ": steered graph search")
        sinfo = ix.search_graph_steered_info()
        assert sinfo == rinfo and sinfo["keyed"] == sinfo["seeds"] + sinfo["direct"] + sinfo["via_bridge"], (what, sinfo, rinfo)
        assert sinfo["via_bridge"] > 0, what  # (the second hop keyed rows)

    def gextend():
        """the ring over the first 200 rows extended over the other 100 in chunks of 32 -- a later chunk re-ranks lines an earlier chunk wrote --
        on an index of the cell's own (gextend_cases' protocol: rows removed before the attach, after it, and among the new)"""
        want, rinfo, trace = exp["gextend"]
        assert any(r >= dcs.G for touched in trace.values() for r in touched), what
        live0, live1, g, _, xseeds = dcs.extension()
        xi = new_index(za, d)
        try:
            xi.append(X[:dcs.G])
            remove(xi, np.flatnonzero(~live0[:dcs.G]))
            xi.set_graph(g)
            assert xi.graph_info()["g_rows"] == dcs.G
            remove(xi, np.flatnonzero(live0[:dcs.G] & ~live1[:dcs.G]))
            xi.append(X[dcs.G:])
            remove(xi, dcs.G + np.flatnonzero(~live1[dcs.G:]))
            xinfo = xi.extend_graph(m, beam=dcs.X_BEAM, width=dcs.X_WIDTH, seeds=xseeds, batch=dcs.X_BATCH)
            same_graph(xi.get_graph(), want, what + ": extend")
            assert xinfo == rinfo == xi.extend_graph_info(), (what, xinfo, rinfo)
            assert xinfo["chunks"] == 4 and xinfo["reverse_rows"] > 0 and xinfo["reverse_kept"] > 0, what
            gi = xi.graph_info()
            assert gi == {"attached": 1, "g_k": dcs.IN_K, "g_rows": dcs.N, "bytes": gi["bytes"]} and gi["bytes"] >= 4 * dcs.N * dcs.IN_K
        finally:
            xi.close()

    differ = []
    for kernel, stage in (("exact_score_kernel", exact), ("refine_line_kernel", refine), ("nnd_line_kernel", descent), ("prune_line_kernel", prune),
                          ("gsearch_kernel", gsearch), ("gsearch_filtered_kernel", gfilter), ("gsearch_steered_kernel", gsteer),
                          ("gext_rerank_kernel", gextend)):
        try:
            stage()
        except AssertionError as e:  # (nothing else is caught: an error of the library ends the test where it is raised)
            differ.append("---- %s at %s: the asserting frames, innermost last\n%s" % (kernel, what, failure_text(e)))
    assert not differ, "%s: %d of 8 kernels differ\n%s" % (what, len(differ), "\n".join(differ))

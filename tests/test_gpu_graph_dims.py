"""A sample of the kind x dimension table of the canonical-row kernels (zh_dispatch_kind_dim): three kinds of the ten -- L2 squared, parity cosine,
Manhattan -- at the six specialised dimensions, through four of the eight kernels on the table (exact_score_kernel, refine_line_kernel,
nnd_line_kernel, gsearch_kernel; the module was written before prune, extend and the filtered and steered search joined the dispatch).  d = 128 /
384 / 768 have a specialised instantiation for every kind, 256 / 512 / 1024 for L2 and cosine only, so that Manhattan takes the generic row loop
there.  The full walk -- every kind at every D, the generic loop at odd and neighbouring dimensions, all eight kernels -- is
tests/test_gpu_dispatch_table.py.  A dimension that reached another dimension's instantiation, or a kind another kind's, changes keys: everything
below is compared bit for bit -- integer keys under the order contract, no tolerance.

One 300-row table per d (refine_cases.table with its 40 identical rows, refine_cases.removed_rows removed), the ring graph at in_k = 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gsearch_cases as gc  # noqa: E402
from tests import refine_cases as rc  # noqa: E402
from tests.test_gpu_exact import check_exact  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402

N, IN_K, K = 300, 8, 8
DIMS = (128, 256, 384, 512, 768, 1024)
METRICS = ("l2sq", "cosine", "manhattan")

_SHARED = {}  # d -> (index, X, live, graph); no test changes the rows of one


@pytest.fixture(scope="module", autouse=True)
def _close_shared_indexes():
    yield
    for entry in _SHARED.values():
        entry[0].close()
    _SHARED.clear()


def index(d):
    import zebra_amd as za
    if d not in _SHARED:
        X = rc.table(N, d)
        live = np.ones(N, bool)
        gone = rc.removed_rows(N)
        live[gone] = False
        ix = za.LSHIndex(d, za.LSHIndexOptions(64, 3), device=0)
        ix.append(X)
        assert ix.remove(gone.astype(np.uint64)).size == gone.size
        graph = rc.g_ring(N, IN_K, live, 0)
        ix.set_graph(graph)
        _SHARED[d] = (ix, X, live, graph)
    return _SHARED[d]


def metric(name):
    import zebra_amd as za
    return {"l2sq": (za.L2SquaredDistance(), zo.L2SQ, 0), "cosine": (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
            "manhattan": (za.ManhattanDistance(), zo.MANHATTAN, 0)}[name]


@pytest.mark.parametrize("mname", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_every_family_at_every_dimension(d, mname):
    ix, X, live, graph = index(d)
    m, om, omode = metric(mname)
    what = "d %d, %s" % (d, mname)
    # refine_line_kernel: one round against the definition
    ref, _ = rc.reference(X, graph, IN_K, K, live, 0, om, omode)
    same(ix.knn_graph_refine(graph, K, m), ref, what + ": refine")
    # nnd_line_kernel: rounds 2 and 3 on the device against the host's loop of full rounds
    loop = ix.knn_graph_refine(graph, K, m, rounds=3, reverse=4)
    same(ix.knn_graph_descent(graph, K, m, rounds=3, reverse=4), loop, what + ": descent")
    assert ix.knn_descent_info()["rounds_run"] >= 2, what  # (the ring at in_k = 8 does not converge in one round: nnd_line_kernel ran)
    # gsearch_kernel: the beam search over the attached ring
    Q = zo.synth_queries(5, d, N)
    seeds = np.random.default_rng([0xD135, d]).integers(0, N, (5, 8)).astype(np.uint64)
    gref, _ = gc.reference(X, graph, N, IN_K, live, 0, Q, seeds, 10, 33, 2, 0, om, omode)
    same(ix.search_graph_batch(Q, 10, m, beam=33, width=2, seeds=seeds), gref, what + ": graph search")
    # exact_score_kernel: the oracle's ranking of the live rows
    check_exact(ix.search_exact_batch(Q, 10, m), X[live], Q, 10, om, omode, ids_of=np.flatnonzero(live))

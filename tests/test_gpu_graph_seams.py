"""The graph family across the sizes at which its host drivers cut their work: ZH_REFINE_SLAB (65 536 stored rows of a sub-slab), the host entries'
staged pieces (refine_host_slab(k) lines; 2^25 / rev_k for the reverse graph) and ZH_GRAPH_BATCH (16 384 queries).  Every other test of the
family stays inside one piece, so the code of the second and later pieces -- the r0 > 0 offsets, the LiveCursor carried from one sub-slab to the
next, the staging reused between pieces, the counters summed over launches -- runs here against a reference for the first time.  A wrong offset
there wraps or aliases INSIDE an allocation: nothing faults, the answer names wrong rows.

Inputs and references are tests/seam_cases.py's (pinned on the CPU by tests/test_seam_reference.py): group-local graphs over groups of 97 rows,
rows removed around every seam and in every 13th group, adversarial lines in the groups at the seams.  The same three checks for every seam:

    (a) definition   bit for bit on ids, keys, counts (and in-degrees) against the local reference, for every group at a seam, the first and the
                     last group, every group with a removed or adversarial line and 32 more drawn by a fixed seed
    (b) whole output the call that crosses the seam equals, array for array, the concatenation of calls that each stay inside one piece (the
                     path the rest of the suite pins); descent, which has no slab form, equals the loop of refinements its contract names
    (c) info         the additive fields are the sums of the pieces' values, and `launches` is the count that shows the split happened

TABLE M, 2 x 65 536 + 4 096 + 37 = 135 205 rows, id_base 2^40 + 3: d = 30 (the generic row loop; L2 squared, the cosine parity key, Manhattan) and
d = 128 (a specialised load; L2 squared, the cosine key).  Seam 1: refinement (in_k 3, k 16) and refinement with reverse neighbours (rev_k 4)
over the whole table and over the slab [60 000, 130 000), whose sub-slab edge 125 536 is off the grid; descent (rounds 3, k 8, rev_k 0 and 4).
Seam 2: the host entry of the refinement at k = 512 (piece = 65 536 lines) over [60 000, 129 669).
TABLE L, 2^19 + 65 536 + 4 096 + 37 = 593 957 rows, d = 30, L2 squared.  Seams 2 and 2': the host entries of the refinement and of descent
(rounds 2) at k = 64 and of the reverse graph at rev_k = 64 (piece = 524 288 lines), check (b) against the device entries, which do no staging.
Check (a) runs on every table and arm (table L's host descent is called once, in a module fixture, and its 514 groups are spread over three
cases).
What the info can show of a host entry's pieces: descent emits its answer with one launch per piece (the device entry: one per 2^24 lines) and the
reverse graph selects with two per piece; the refinement's `launches` are its sub-slabs, and a piece is whole sub-slabs, so there the split is
shown by the piece size (seam_cases.host_piece, pinned against the library's source on the CPU) being below the lines asked for.  Of descent's
`launches` only round 1's sub-slabs, its launch per piece and the host entry's emission per piece are counted where they happen; the other terms
are the library's formula in N (seam_cases.descent_launches).
SEAM 3, on gsearch_cases' t600 and t600x128 with the exact graph at g_k 32: b = 16 384, 16 385 and 2 x 16 384 + 3 queries, query i and its seeds
those of i mod 257 out of a block of 257 (257 is prime and 16 384 mod 257 = 193: a batch that starts at the wrong offset answers wrongly).  The
block is checked against the references, the large call's row i is the block's row i mod 257, and the large call equals the calls batch by batch.

Measured on one MI355X (pytest --durations=0; the slowest tests/test_gpu_large_table.py test took 5.7 to 6.1 s on the same machine): the
module 52 s; the whole-table descent on M 2.5 to 2.8 s a case at either dimension (1 s of it the 147 groups' references); the whole-table
refinements 1.2 to 1.3 s a case; table L's host refinement 1.9 s, host reverse graph 1.2 s, host descent 2 s for the call with its (b) and (c)
and 2.3 s for each third of the 514 groups' references; the slab tests 0.6 s; a search case 0.2 to 0.4 s with its block's reference, 0.02 to
0.05 s once that is cached; building a table 0.1 s.  Run alone, give the module a limit of its own:
timeout 900 pytest -m gpu tests/test_gpu_graph_seams.py"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import gfilter_cases as gf  # noqa: E402
from tests import gsearch_cases as gc  # noqa: E402
from tests import seam_cases as sc  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402
from tests.test_gpu_reverse import same_reverse  # noqa: E402

NONE = np.uint64(2**64 - 1)
SLAB = sc.REFINE_SLAB
M_N = 2 * SLAB + 4096 + 37
L_N = 2**19 + SLAB + 4096 + 37
IN_K = 3
M_SLAB = (60000, 70000)   # sub-slabs [60 000, 125 536) and [125 536, 130 000)
M_HOST = (60000, 69669)   # k = 512: pieces of 65 536 lines, [60 000, 125 536) and [125 536, 129 669)
TABLES = {"M30": (M_N, 30), "M128": (M_N, 128), "L": (L_N, 30)}
POSITIONS = {"M30": (SLAB, 2 * SLAB, 60000, 125536, 129669, 130000), "M128": (SLAB, 2 * SLAB), "L": tuple(range(SLAB, L_N, SLAB))}
ARMS = [("M30", "l2sq"), ("M30", "cos"), ("M30", "manhattan"), ("M128", "l2sq"), ("M128", "cos")]


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def metric_of(za, name):
    return {"l2sq": (za.L2SquaredDistance(), zo.L2SQ, 0), "cos": (za.CosineDistance(parity=True), zo.COSINE, zo.PARITY),
            "manhattan": (za.ManhattanDistance(), zo.MANHATTAN, 0)}[name]


class Setup:
    """an index of synthetic rows with seam_cases' removed rows, its group-local graph with the adversarial lines on the host and on the device,
    and the groups check (a) takes"""

    def __init__(self, za, name):
        import torch
        self.n, self.d = TABLES[name]
        pos = POSITIONS[name]
        self.tb = sc.Table(self.n, self.d, sc.ID_BASE, sc.removed(self.n, pos))
        self.ix = za.LSHIndex(self.d, za.LSHIndexOptions(64, 3), device=0, id_base=sc.ID_BASE, reserve_rows=self.n)
        self.ix.append_synthetic(self.n)
        gone = self.tb.gone.astype(np.uint64) + np.uint64(sc.ID_BASE)
        assert self.ix.remove(gone).size == gone.size and self.ix.stored_rows() == self.n and len(self.ix) == self.n - gone.size
        self.live = self.tb.live
        ids, counts = sc.graph(self.n, IN_K, sc.ID_BASE)
        changed = sc.adversarial(ids, counts, self.n, sc.ID_BASE, self.live, sc.seam_groups(self.n, pos))
        assert len(changed) >= 4 * len(sc.seam_groups(self.n, pos))
        self.graph = (ids, counts)
        self.groups = sc.checked_groups(self.n, pos, self.tb.gone, changed)
        self.d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
        self.d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
        for s in pos:  # live_before at a seam differs from the row number, and rows on both sides of it are gone
            assert not self.live[s - 1:s + 2].any() and int(self.live[:s].sum()) < s - 1
        g = self.groups[len(self.groups) // 2]
        s, e = self.tb.span(g)
        assert (self.ix.read_rows(s, e - s).view(np.uint32) == self.tb.rows(g).view(np.uint32)).all()  # the index holds the oracle's rows

    def close(self):
        self.d_ids = self.d_counts = None
        self.ix.close()


_SETUPS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_setups():
    yield
    import torch
    for s in _SETUPS.values():
        s.close()
    _SETUPS.clear()
    torch.cuda.empty_cache()


def setup(za, name):
    if name not in _SETUPS:
        _SETUPS[name] = Setup(za, name)
    return _SETUPS[name]


def device_refine(S, k, m, first_row, n, rev_k, side=False):
    """the device entry with sentinel-filled outputs, on the index's stream or on a side stream -> (ids, keys, counts) on the host, the info"""
    import torch
    ids, keys, counts = out = sc.device_outputs(n, k)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else None
    ptr = None if stream is None else stream.cuda_stream
    if rev_k:
        S.ix.knn_graph_refine_rev_device(S.d_ids.data_ptr(), S.d_counts.data_ptr(), IN_K, rev_k, k, m, first_row, n, ids.data_ptr(), keys.data_ptr(),
                                         counts.data_ptr(), stream=ptr)
    else:
        S.ix.knn_graph_refine_device(S.d_ids.data_ptr(), S.d_counts.data_ptr(), IN_K, k, m, first_row, n, ids.data_ptr(), keys.data_ptr(), counts.data_ptr(),
                                     stream=ptr)
    if stream is not None:
        assert stream.query()  # complete on return
    return sc.host_arrays(out), refine_info(S, rev_k)


def refine_info(S, rev_k):
    return S.ix.knn_refine_rev_info() if rev_k else S.ix.knn_refine_info()


def host_refine(S, k, m, first_row, n, rev_k):
    got = S.ix.knn_graph_refine(S.graph, k, m, first_row, n, reverse=rev_k)
    return got, refine_info(S, rev_k)


SUMMED = ("lines", "listed", "keyed", "updates")


def stitched(S, k, m, rev_k, cuts, host=True):
    """calls that each stay inside one piece (one sub-slab, one launch), concatenated -> (ids, keys, counts), the infos"""
    parts, infos = [], []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        assert r1 - r0 <= SLAB
        got, info = host_refine(S, k, m, r0, r1 - r0, rev_k) if host else device_refine(S, k, m, r0, r1 - r0, rev_k)
        assert info["launches"] == (1 if S.live[r0:r1].any() else 0)
        parts.append(got)
        infos.append(info)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), infos


def info_is_the_sum(info, infos, S, k, rev_k, launches, what):
    want = {f: sum(i[f] for i in infos) for f in SUMMED + (("kept",) if rev_k else ())}
    want.update(rows_live=int(S.live.sum()), in_k=IN_K, k=k, launches=launches)
    if rev_k:  # the transposition is of the whole table whatever the slab: every piece reports the same edges and the same largest in-degree
        want.update(rev_k=rev_k, edges=infos[0]["edges"], max_degree=infos[0]["max_degree"])
        assert all(i["edges"] == infos[0]["edges"] > 0 and i["max_degree"] == infos[0]["max_degree"] for i in infos), what
    assert info == want, (what, info, want)


def groups_in(S, first_row, n):
    """(group, the rows [lo, hi) of it inside the slab) for the checked groups that touch [first_row, first_row + n)"""
    out = []
    for g in S.groups:
        s, e = S.tb.span(g)
        lo, hi = max(s, first_row), min(e, first_row + n)
        if lo < hi:
            out.append((g, s, e, lo, hi))
    return out


def refine_groups_are_the_definition(S, got, first_row, n, k, om, omode, rev_k, what):
    seen = 0
    for g, s, e, lo, hi in groups_in(S, first_row, n):
        ref, _ = sc.local_refine(S.tb, S.graph[0][s:e], S.graph[1][s:e], g, k, om, omode, rev_k)
        same(tuple(a[lo - first_row:hi - first_row] for a in got), tuple(a[lo - s:hi - s] for a in ref), "%s group %d" % (what, g))
        seen += 1
    assert seen >= 32
    return seen


# ---------------------------------------------------------------- seam 1: the sub-slabs of a refinement
@pytest.mark.parametrize("name,metric", ARMS)
def test_refinement_over_the_whole_table(za, name, metric):
    S = setup(za, name)
    m, om, omode = metric_of(za, metric)
    k, cuts = 16, list(range(0, S.n, SLAB)) + [S.n]
    assert len(cuts) == 4 and sc.sub_slabs(0, S.n, S.live) == 3
    for rev_k in (0, 4):
        what = "%s %s rev_k %d" % (name, metric, rev_k)
        got, info = device_refine(S, k, m, 0, S.n, rev_k, side=(name == "M30" and metric == "l2sq"))
        assert info["launches"] == 3 and info["lines"] == int(S.live.sum()), (what, info)  # the seam was crossed: three sub-slabs
        whole, winfo = stitched(S, k, m, rev_k, cuts)
        same(got, whole, what + " (slab by slab)")
        info_is_the_sum(info, winfo, S, k, rev_k, 3, what)
        host, hinfo = host_refine(S, k, m, 0, S.n, rev_k)
        same(host, got, what + " (host entry)")
        assert hinfo == info, (what, hinfo, info)
        refine_groups_are_the_definition(S, got, 0, S.n, k, om, omode, rev_k, what)
        assert (got[2][~S.live] == 0).all() and (got[0][~S.live] == NONE).all() and (got[1][~S.live] == NONE).all()


@pytest.mark.parametrize("name,metric", [("M30", "l2sq"), ("M30", "manhattan"), ("M128", "cos")])
def test_refinement_over_a_slab_off_the_grid(za, name, metric):
    """[60 000, 130 000): the sub-slabs start at the slab's first row, so their edge 125 536 is no multiple of 65 536; the stitched calls are cut
    at the grid, so that the edge lies inside one of them"""
    S = setup(za, name)
    m, om, omode = metric_of(za, metric)
    first, n = M_SLAB
    k, cuts = 16, [first, SLAB, first + n]
    for rev_k in (0, 4):
        what = "%s %s slab, rev_k %d" % (name, metric, rev_k)
        got, info = device_refine(S, k, m, first, n, rev_k)
        assert info["launches"] == 2 == sc.sub_slabs(first, n, S.live), (what, info)
        whole, winfo = stitched(S, k, m, rev_k, cuts, host=False)
        same(got, whole, what + " (slab by slab)")
        info_is_the_sum(info, winfo, S, k, rev_k, 2, what)
        host, hinfo = host_refine(S, k, m, first, n, rev_k)
        same(host, got, what + " (host entry)")
        assert hinfo == info, (what, hinfo, info)
        refine_groups_are_the_definition(S, got, first, n, k, om, omode, rev_k, what)


# ---------------------------------------------------------------- seam 2: the staged pieces of a host entry
def test_host_refinement_in_pieces_of_65536_lines(za):
    """k = 512: a piece of the host entry's output is 65 536 lines, and 69 669 are asked for"""
    S = setup(za, "M30")
    m, om, omode = metric_of(za, "l2sq")
    first, n = M_HOST
    k = 512
    assert sc.host_piece(k) == SLAB < n
    got, info = host_refine(S, k, m, first, n, 0)
    assert info["launches"] == 2 == sc.sub_slabs(first, n, S.live, sc.host_piece(k)), info
    whole, winfo = stitched(S, k, m, 0, [first, first + SLAB, first + n])  # each call one piece: the path the rest of the suite pins
    same(got, whole, "k 512 (piece by piece)")
    info_is_the_sum(info, winfo, S, k, 0, 2, "k 512")
    dev, dinfo = device_refine(S, k, m, first, n, 0)
    same(dev, got, "k 512 (device entry)")
    assert dinfo == info
    refine_groups_are_the_definition(S, got, first, n, k, om, omode, 0, "k 512")
    assert int(got[2].max()) <= IN_K + IN_K * IN_K < k and (got[0][:, IN_K + IN_K * IN_K:] == NONE).all()


# ---------------------------------------------------------------- seam 1 again: descent
def device_descent(S, in_k, rev_k, k, rounds, m, side=False):
    import torch
    out = sc.device_outputs(S.n, k)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else None
    S.ix.knn_graph_descent_device(S.d_ids.data_ptr(), S.d_counts.data_ptr(), in_k, rev_k, k, rounds, m, *[o.data_ptr() for o in out],
                                  stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        assert stream.query()
    return sc.host_arrays(out), S.ix.knn_descent_info()


def the_loop(S, k, m, rounds, rev_k):
    """the loop the contract names, round by round on the host entry -> (answer, the info of every round)"""
    g, infos = S.graph, []
    for _ in range(rounds):
        g = S.ix.knn_graph_refine(g, k, m, reverse=rev_k)
        infos.append(refine_info(S, rev_k))
        if infos[-1]["updates"] == 0:
            break
    return g, infos


def descent_groups_are_the_definition(S, got, rev_k, k, rounds_run, om, omode, what, groups=None):
    for g in S.groups if groups is None else groups:
        s, e = S.tb.span(g)
        ref = sc.local_descent(S.tb, S.graph[0][s:e], S.graph[1][s:e], g, rev_k, k, rounds_run, om, omode)
        same(tuple(a[s:e] for a in got), ref, "%s group %d" % (what, g))


@pytest.mark.parametrize("rev_k", [0, 4])
@pytest.mark.parametrize("name,metric", ARMS)
def test_descent_over_the_whole_table(za, name, metric, rev_k):
    S = setup(za, name)
    m, om, omode = metric_of(za, metric)
    k, rounds = 8, 3
    what = "%s %s descent rev_k %d" % (name, metric, rev_k)
    got, info = device_descent(S, IN_K, rev_k, k, rounds, m, side=(name == "M128" and metric == "l2sq"))
    assert info["rounds_run"] == rounds and info["launches"] == sc.descent_launches(S.n, S.live, IN_K, rev_k, k, rounds, False), (what, info)
    assert sc.sub_slabs(0, S.n, S.live) == 3  # (of which round 1's three sub-slabs are a term)
    want, infos = the_loop(S, k, m, rounds, rev_k)
    same(got, want, what + " (the loop)")
    assert info["updates_round"] == [i["updates"] for i in infos] and info["keyed_round"][0] == infos[0]["keyed"] and info["updates"] == infos[-1]["updates"]
    assert info["listed"] >= infos[0]["listed"] and info["keyed"] == sum(info["keyed_round"]) and info["lines_active"] == sum(info["active_round"])
    assert info["active_round"][0] == int(S.live.sum()) == infos[0]["lines"] and all(i["launches"] == 3 for i in infos)
    if metric == "l2sq":
        host = S.ix.knn_graph_descent(S.graph, k, m, rounds=rounds, reverse=rev_k)
        hinfo = S.ix.knn_descent_info()
        same(host, got, what + " (host entry)")
        assert hinfo == dict(info, launches=sc.descent_launches(S.n, S.live, IN_K, rev_k, k, rounds, True)), (what, hinfo)
    descent_groups_are_the_definition(S, got, rev_k, k, rounds, om, omode, what)


# ---------------------------------------------------------------- seams 2 and 2': table L, pieces of 524 288 lines
def test_host_refinement_in_pieces_of_524288_lines(za):
    S = setup(za, "L")
    m, om, omode = metric_of(za, "l2sq")
    k = 64
    assert sc.host_piece(k) == 2**19 < S.n
    got, info = host_refine(S, k, m, 0, S.n, 0)
    assert info["launches"] == 10 == sc.sub_slabs(0, S.n, S.live, sc.host_piece(k)) and info["lines"] == int(S.live.sum()), info
    dev, dinfo = device_refine(S, k, m, 0, S.n, 0, side=True)
    same(got, dev, "k 64 (device entry)")
    assert dinfo == info
    whole, winfo = stitched(S, k, m, 0, list(range(0, S.n, SLAB)) + [S.n], host=False)
    same(got, whole, "k 64 (slab by slab)")
    info_is_the_sum(info, winfo, S, k, 0, 10, "k 64")
    refine_groups_are_the_definition(S, got, 0, S.n, k, om, omode, 0, "k 64")


L_DESCENT = (64, 2)  # k, rounds
L_DESCENT_PARTS = 3   # check (a) over all of table L's checked groups takes 7 s of references: a third of them a test


@pytest.fixture(scope="module")
def l_descent(za):
    """ONE host call of zh_knn_graph_descent over table L, shared by the tests below -> (the setup, the answer, the info)"""
    S = setup(za, "L")
    k, rounds = L_DESCENT
    got = S.ix.knn_graph_descent(S.graph, k, metric_of(za, "l2sq")[0], rounds=rounds, reverse=0)
    return S, got, S.ix.knn_descent_info()


def test_host_descent_in_pieces_of_524288_lines(za, l_descent):
    """(b) the device entry and the loop, (c) the launches"""
    S, got, info = l_descent
    m = metric_of(za, "l2sq")[0]
    k, rounds = L_DESCENT
    # ten sub-slabs and two launches for the ids of round 1's two pieces, four of round 2, and the answer piece by piece: two launches, where
    # the device entry emits it in one
    assert info["rounds_run"] == rounds and info["launches"] == sc.descent_launches(S.n, S.live, IN_K, 0, k, rounds, True) == 10 + 2 + 4 + 2, info
    dev, dinfo = device_descent(S, IN_K, 0, k, rounds, m)
    same(got, dev, "descent k 64 (device entry)")
    assert dinfo == dict(info, launches=info["launches"] - 1)
    want, infos = the_loop(S, k, m, rounds, 0)
    same(got, want, "descent k 64 (the loop)")
    assert info["updates_round"] == [i["updates"] for i in infos] and info["keyed_round"][0] == infos[0]["keyed"]


@pytest.mark.parametrize("part", range(L_DESCENT_PARTS))
def test_host_descent_in_pieces_is_the_definition(za, l_descent, part):
    """(a) on every checked group of table L, a third of them a case"""
    S, got, info = l_descent
    _, om, omode = metric_of(za, "l2sq")
    k, rounds = L_DESCENT
    assert info["rounds_run"] == rounds
    groups = S.groups[part::L_DESCENT_PARTS]
    assert len(groups) >= len(S.groups) // L_DESCENT_PARTS > 100
    descent_groups_are_the_definition(S, got, 0, k, rounds, om, omode, "descent k 64", groups)


def test_host_reverse_in_pieces_of_524288_lines(za):
    import torch
    S = setup(za, "L")
    rev_k = 64
    assert sc.reverse_piece(rev_k) == 2**19 < S.n
    got = S.ix.knn_graph_reverse(S.graph, rev_k)
    info = S.ix.knn_reverse_info()
    assert info["launches"] == 4 and info["lines"] == int(S.live.sum()) and info["rows_live"] == info["lines"], info  # two pieces, two launches each
    out = sc.device_outputs(S.n, rev_k, "degree")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    S.ix.knn_graph_reverse_device(S.d_ids.data_ptr(), S.d_counts.data_ptr(), IN_K, rev_k, 0, S.n, *[o.data_ptr() for o in out], stream=side.cuda_stream)
    assert side.query()
    same_reverse(got, sc.host_arrays(out), "reverse (device entry)")
    assert S.ix.knn_reverse_info() == dict(info, launches=2)
    kept = 0
    for r0 in (0, 2**19):  # calls that each stay inside one piece
        part = S.ix.knn_graph_reverse(S.graph, rev_k, r0, min(2**19, S.n - r0))
        pinfo = S.ix.knn_reverse_info()
        same_reverse(tuple(a[r0:r0 + 2**19] for a in got), part, "reverse (piece by piece)")
        assert pinfo["launches"] == 2 and pinfo["edges"] == info["edges"] and pinfo["max_degree"] == info["max_degree"]
        kept += pinfo["kept"]
    assert kept == info["kept"] == int(got[1].sum()) and info["edges"] == int(got[2].sum()) > 0
    for g in S.groups:
        s, e = S.tb.span(g)
        ref, _ = sc.local_reverse(S.tb, S.graph[0][s:e], S.graph[1][s:e], g, rev_k)
        same_reverse(tuple(a[s:e] for a in got), ref, "reverse group %d" % g)


# ---------------------------------------------------------------- seam 3: the batches of a search
BLOCK = 257
BATCHES = (sc.GRAPH_BATCH, sc.GRAPH_BATCH + 1, 2 * sc.GRAPH_BATCH + 3)
G_K, TOP_K, BEAM, WIDTH, N_SEED = 32, 10, 64, 2, 8
BASES = {"t600": sc.ID_BASE, "t600x128": 0}


@functools.lru_cache(maxsize=None)
def block(tname):
    """the 257 queries and their seeds (stored rows drawn with replacement, some removed)"""
    n = gc.TABLES[tname][0]
    seeds = np.random.default_rng([0x5EA37, n]).integers(0, n, (BLOCK, N_SEED)).astype(np.uint64) + np.uint64(BASES[tname])
    return gc.queries(tname, BLOCK), seeds


@functools.lru_cache(maxsize=None)
def block_reference(tname, metric, fname):
    X, live = gc.table(tname)
    om, omode = {"l2sq": (zo.L2SQ, 0), "cos": (zo.COSINE, zo.PARITY)}[metric]
    Q, seeds = block(tname)
    args = (X, gc.graph(tname, "exact", G_K, BASES[tname]), X.shape[0], G_K, live, BASES[tname], Q, seeds, TOP_K, BEAM, WIDTH, 0, om, omode)
    if fname is None:
        return gc.reference(*args)
    return gf.reference(*args, *gf.table_filter(tname, fname))


_SEARCH = {}


@pytest.fixture(scope="module", autouse=True)
def _close_search_indexes():
    yield
    for ix in _SEARCH.values():
        ix.close()
    _SEARCH.clear()


def search_index(za, tname):
    if tname not in _SEARCH:
        X, live = gc.table(tname)
        ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 3), device=0, id_base=BASES[tname])
        ix.append(X)
        gone = np.flatnonzero(~live).astype(np.uint64) + np.uint64(BASES[tname])
        assert ix.remove(gone).size == gone.size
        ix.set_graph(gc.graph(tname, "exact", G_K, BASES[tname]))
        _SEARCH[tname] = ix
    return _SEARCH[tname]


def search(ix, m, Q, seeds, flt, device, side=False):
    """one call of either entry, filtered or not, into sentinel-filled outputs -> (ids, keys, counts), the info"""
    b = Q.shape[0]
    if not device:
        if flt is None:
            got = ix.search_graph_batch(Q, TOP_K, m, beam=BEAM, width=WIDTH, seeds=seeds)
        else:
            mask = np.unpackbits(flt[0].view(np.uint8), bitorder="little")[:flt[1]].astype(bool)
            got = ix.search_graph_filtered_batch(Q, TOP_K, m, mask, beam=BEAM, width=WIDTH, seeds=seeds)
    else:
        import torch
        q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
        sd = torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).cuda()
        out = sc.device_outputs(b, TOP_K)
        stream = torch.cuda.Stream() if side else None
        ptr = None if stream is None else stream.cuda_stream
        if flt is not None:
            fw = torch.from_numpy(np.concatenate([flt[0], np.zeros(1, np.uint32)]).view(np.int32)).cuda()
        torch.cuda.synchronize()
        if flt is None:
            ix.search_graph_batch_device(q.data_ptr(), b, sd.data_ptr(), N_SEED, TOP_K, m, *[o.data_ptr() for o in out], beam=BEAM, width=WIDTH, stream=ptr)
        else:
            ix.search_graph_filtered_batch_device(q.data_ptr(), b, sd.data_ptr(), N_SEED, TOP_K, m, fw.data_ptr(), flt[1], *[o.data_ptr() for o in out],
                                                  beam=BEAM, width=WIDTH, stream=ptr)
        if stream is not None:
            assert stream.query()
        got = sc.host_arrays(out)
    return got, (ix.search_graph_info() if flt is None else ix.search_graph_filtered_info())


@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("tname,metric,fname,device", [("t600", "l2sq", None, False), ("t600", "cos", None, True), ("t600x128", "l2sq", None, True),
                                                       ("t600x128", "cos", None, False), ("t600", "l2sq", "even", False), ("t600", "cos", "mod10_3", True),
                                                       ("t600x128", "cos", "even", True), ("t600x128", "l2sq", "mod10_3", False)])
def test_search_in_batches_of_16384_queries(za, tname, metric, fname, device, b):
    ix = search_index(za, tname)
    m = metric_of(za, metric)[0]
    flt = None if fname is None else gf.table_filter(tname, fname)
    what = "%s %s %s %s b %d" % (tname, metric, fname, "device" if device else "host", b)
    Q257, seeds257 = block(tname)
    # (a) the block of 257 against the definition, both entries
    ref, rinfo = block_reference(tname, metric, fname)
    for dev in (False, True):
        got257, info257 = search(ix, m, Q257, seeds257, flt, dev)
        same(got257, ref, what + " (the block)")
        assert info257 == rinfo, (what, info257, rinfo)
    assert (ref[2] > 0).all() and len({tuple(r) for r in ref[0].tolist()}) > BLOCK // 2  # (neighbouring rows of the block differ: an offset shows)
    # the large call: query i and its seeds are those of i mod 257
    at = np.arange(b) % BLOCK
    Q, seeds = np.ascontiguousarray(Q257[at]), np.ascontiguousarray(seeds257[at])
    got, info = search(ix, m, Q, seeds, flt, device, side=device and tname == "t600")
    launches = -(-b // sc.GRAPH_BATCH)
    assert info["launches"] == launches and info["queries"] == b, (what, info)
    same(got, tuple(a[at] for a in ref), what + " (row i is the block's row i mod 257)")
    # (b), (c): the calls batch by batch, and their figures summed
    parts, infos = [], []
    for b0 in range(0, b, sc.GRAPH_BATCH):
        p, i = search(ix, m, Q[b0:b0 + sc.GRAPH_BATCH], seeds[b0:b0 + sc.GRAPH_BATCH], flt, device)
        assert i["launches"] == 1
        parts.append(p)
        infos.append(i)
    same(got, tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), what + " (batch by batch)")
    summed = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches") + (() if flt is None else ("offered", "returned"))
    want = {f: sum(i[f] for i in infos) for f in summed}
    if flt is not None:
        want["rows_allowed"] = infos[0]["rows_allowed"]
    assert info == want, (what, info, want)
    assert launches == len(infos) and (launches > 1 or b == sc.GRAPH_BATCH)
    if flt is not None:
        assert info["returned"] == int(got[2].sum())

"""The graph family on a table with more than 2^24 stored rows: 2^24 + 4 096 + 37 = 16 781 349 rows of d = 8 (0.5 GB), id_base 2^40 + 3.  Past
ZH_LINES_PER_LAUNCH = 2^24 lines zh_for_line_pieces cuts the launches of the wave-per-line kernels (the caller's graph to row numbers, the reverse
selection, descent's flag / plan / emit passes), and at in_k = 64 the transposition's two edge passes (2^30 / in_k lines a launch) are cut at the
same row.  No other test of the family has a second piece there; a dropped `+ b0 * in_k` names wrong rows and faults nothing.

A module of its own because of its table.  Device entries only; the input graphs are made on the device with torch arithmetic from
tests/seam_cases.py's group rule (groups of 97 rows, every line inside its group), never as host arrays, and outputs stay on the device: only the
checked groups are copied back.  Rows are removed around row 2^24 and the slab's edges and in every 13th group, and the group that ends at row
2^24 and the one that starts at row 2^24 + 1 carry the adversarial lines, one on each side of the cut.  The checks are tests/test_gpu_graph_seams.py's three:

    (a) the lines of the checked groups against seam_cases' local references, bit for bit: the groups the slab [2^24 - 1000, 2^24 + 1000) touches,
        the first and the last group, 32 groups with a removed pair and 32 regular ones drawn by a fixed seed (the 13 000 groups with a removed
        pair cannot all get a Python reference in seconds at any number of tests; the ones left out are neither regular nor sampled, and (b)'s
        stitched forms cover them where they lie in the slab.  THE RULE "every group that holds a removed line" IS NOT MET on this table)
    (b) the whole output: for the refinement the id-set check over ALL fully live, regular groups in torch -- the sorted `ids - start` of line
        start + j is the template's C(j), k >= |C| -- and the slab call equal to the whole-table call's lines; descent equal to the loop of
        refinements on the device, array for array
    (c) the info: descent's `launches` holds the zh_line_launches(N) = 2 and the edge passes' terms, but the library adds those by formula
        (seam_cases.descent_launches), it does not count launches: they show that N is past the cut and no more.  The one-round calls and the
        reverse graph do not count the cut passes at all, so there the tests assert what the info does give (lines, sub-slabs, edges) and, from
        the sizes pinned on the CPU, that the stored rows exceed the piece.  That the pieces ran and were right is shown by (a) and (b)

Measured on one MI355X (pytest --durations=0, inside a run of the whole suite whose slowest tests/test_gpu_large_table.py test took 5.7 s): the
module 19 s; the table 0.4 s; one descent call over the whole table 2.7 s (rev_k 0) and 3.1 s (rev_k 2), made once per rev_k by the `descended`
fixture and shared by two tests (as one test, call + loop + references took 6.0 and 6.9 s, above the bar); the loop of three refinements 1.9 and
2.3 s, the 88 groups' descent references 1.5 s, the refinements 1.1 and 1.3 s, the reverse graph at in_k 64 0.1 to 0.7 s, the search 0.1 s.
Run alone, give the module a limit of its own: timeout 900 pytest -m gpu tests/test_gpu_graph_pieces.py"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import seam_cases as sc  # noqa: E402
from tests.test_gpu_refine import same  # noqa: E402
from tests.test_gpu_reverse import same_reverse  # noqa: E402

P = sc.P
EDGE = sc.LINES_PER_LAUNCH
N, D, BASE = EDGE + 4096 + 37, 8, sc.ID_BASE
SLAB = (EDGE - 1000, 2000)
POSITIONS = (EDGE, SLAB[0], SLAB[0] + SLAB[1])


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


class Big:
    def __init__(self, za):
        self.tb = sc.Table(N, D, BASE, sc.removed(N, POSITIONS))
        self.live = self.tb.live
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(64, 3), device=0, id_base=BASE, reserve_rows=N)
        self.ix.append_synthetic(N)
        gone = self.tb.gone.astype(np.uint64) + np.uint64(BASE)
        assert self.ix.remove(gone).size == gone.size and self.ix.stored_rows() == N > EDGE
        # 2^24 mod 97 = 96: row 2^24 is the last row of its group, whose adversarial lines all lie in the first launch piece; the group that starts
        # at row 2^24 + 1 carries them in the second
        self.seam_groups = sorted(set(sc.seam_groups(N, (EDGE,))) | {(EDGE + 1) // P})
        assert len(self.seam_groups) == 2 and self.seam_groups[1] * P == EDGE + 1
        lo, hi = SLAB[0] - P, SLAB[0] + SLAB[1] + P
        near = self.tb.gone[(self.tb.gone >= lo) & (self.tb.gone < hi)]
        far = self.tb.gone[(self.tb.gone < lo) | (self.tb.gone >= hi)]
        far = far[np.random.default_rng(0x5EA38).permutation(far.size)[:32]]
        in_slab = [r for r in range(SLAB[0], SLAB[0] + SLAB[1], P)] + [SLAB[0] + SLAB[1] - 1]
        self.groups = sc.checked_groups(N, POSITIONS, np.concatenate([near, far, np.array(in_slab, np.int64)]), [])
        full = N // P
        regular = self.live[:full * P].reshape(full, P).all(1)
        regular[self.seam_groups] = False  # (the adversarial lines)
        self.regular = regular
        for g in (self.groups[1], self.groups[-1]):
            s, e = self.tb.span(g)
            assert (self.ix.read_rows(s, e - s).view(np.uint32) == self.tb.rows(g).view(np.uint32)).all()


@pytest.fixture(scope="module")
def big(za):
    import torch
    b = Big(za)
    yield b
    b.ix.close()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    import torch
    torch.cuda.empty_cache()


def device_graph(big, in_k):
    """seam_cases.graph(N, in_k, BASE) made on the device, the adversarial lines in the groups at row 2^24 -> (ids [N, in_k] i64, counts [N] i32)"""
    import torch
    ids = torch.empty((N, in_k), dtype=torch.int64, device="cuda")
    o = torch.tensor(sc.OFFSETS[:in_k], dtype=torch.int64, device="cuda")[None, :]
    step = 2**26 // in_k
    for r0 in range(0, N, step):
        r = torch.arange(r0, min(r0 + step, N), dtype=torch.int64, device="cuda")[:, None]
        j = r % P
        ids[r0:r0 + r.shape[0]] = r - j + (j + o) % P + BASE
        del r, j
    counts = torch.full((N,), in_k, dtype=torch.int32, device="cuda")
    s, e = big.seam_groups[0] * P, big.seam_groups[-1] * P + P
    h_ids, h_counts = ids[s:e].cpu().numpy().view(np.uint64).copy(), counts[s:e].cpu().numpy().view(np.uint32).copy()
    want = sc.graph(N, in_k, BASE, s, e)
    assert (h_ids == want[0]).all() and (h_counts == want[1]).all()
    changed = sc.adversarial(h_ids, h_counts, N, BASE, big.live, big.seam_groups, lo=s)
    assert len(changed) >= 4 * len(big.seam_groups) and sum(1 for r in changed if r < EDGE) >= 4 and sum(1 for r in changed if r > EDGE) >= 4
    ids[s:e] = torch.from_numpy(h_ids.view(np.int64)).cuda()
    counts[s:e] = torch.from_numpy(h_counts.view(np.int32)).cuda()
    return ids, counts


@pytest.fixture(scope="module")
def graph2(big):
    """the graph at in_k = 2 that the search, the refinements and descent share (268 MB)"""
    g = device_graph(big, 2)
    yield g


def lines(graph, s, e):
    return graph[0][s:e].cpu().numpy().view(np.uint64), graph[1][s:e].cpu().numpy().view(np.uint32)


outputs, host = sc.device_outputs, sc.host_arrays


def refine(big, graph, in_k, rev_k, k, m, first_row, n, out):
    import torch
    torch.cuda.synchronize()
    if rev_k:
        big.ix.knn_graph_refine_rev_device(graph[0].data_ptr(), graph[1].data_ptr(), in_k, rev_k, k, m, first_row, n, *[o.data_ptr() for o in out])
        return big.ix.knn_refine_rev_info()
    big.ix.knn_graph_refine_device(graph[0].data_ptr(), graph[1].data_ptr(), in_k, k, m, first_row, n, *[o.data_ptr() for o in out])
    return big.ix.knn_refine_info()


def regular_groups_hold_the_template(big, out, in_k, k):
    """check (b) in torch: in every fully live, regular group the line of position j holds exactly the template's C(j)"""
    import torch
    T = sc.template(in_k)
    size = max(c.size for c in T)
    assert size <= k
    want = np.full((P, k), 1000, np.int64)
    for j, c in enumerate(T):
        want[j, :c.size] = c
    want = torch.from_numpy(want).cuda()
    sizes = torch.tensor([c.size for c in T], dtype=torch.int32, device="cuda")
    full = N // P
    reg = torch.from_numpy(big.regular).cuda()
    start = (torch.arange(full, dtype=torch.int64, device="cuda") * P + BASE)[:, None, None]
    bad = 0
    step = 16384  # groups a pass
    for g0 in range(0, full, step):
        g1 = min(g0 + step, full)
        ids = out[0][g0 * P:g1 * P].view(g1 - g0, P, k)
        rel = torch.where(ids == -1, torch.full_like(ids, 1000), ids - start[g0:g1])
        rel = torch.sort(rel, dim=2).values
        ok = (rel == want[None]).all(2) & (out[2][g0 * P:g1 * P].view(g1 - g0, P) == sizes[None])
        bad += int((~ok.all(1) & reg[g0:g1]).sum())
    assert bad == 0, "%d regular groups differ from the template" % bad
    assert int(reg.sum()) > full * 9 // 10


# ---------------------------------------------------------------- seam 4: the attached graph and the search
def test_search_over_a_graph_of_more_than_2_24_lines(za, big, graph2):
    import torch
    m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
    big.ix.set_graph_device(graph2[0].data_ptr(), graph2[1].data_ptr(), N, 2)
    try:
        info = big.ix.graph_info()
        assert info["attached"] == 1 and info["g_k"] == 2 and info["g_rows"] == N > EDGE  # more lines than one launch of the row pass takes
        groups = [0] + big.seam_groups + [sc.groups(N) - 1]
        top_k, beam, width, n_seed, per = 10, 64, 1, 4, 4
        Q, seeds = [], []
        for i, g in enumerate(groups):
            s, e = big.tb.span(g)
            Q.append(zo.synth_queries(per, D, N, b0=per * i))
            seeds.append(np.array([[s + (17 * q + 5 * t + i) % (e - s) for t in range(n_seed)] for q in range(per)], np.uint64) + np.uint64(BASE))
        Q, seeds = np.concatenate(Q), np.concatenate(seeds)
        b = Q.shape[0]
        out = outputs(b, top_k)
        dq, ds = torch.from_numpy(Q).cuda(), torch.from_numpy(seeds.view(np.int64)).cuda()
        torch.cuda.synchronize()
        big.ix.search_graph_batch_device(dq.data_ptr(), b, ds.data_ptr(), n_seed, top_k, m, *[o.data_ptr() for o in out], beam=beam, width=width)
        got, sinfo = host(out, 0, b), big.ix.search_graph_info()
        total = {f: 0 for f in ("seeds", "iterations", "expanded", "keyed")}
        for i, g in enumerate(groups):
            s, e = big.tb.span(g)
            ref, rinfo = sc.local_search(big.tb, *lines(graph2, s, e), g, Q[per * i:per * i + per], seeds[per * i:per * i + per], top_k, beam, width, 0, om, omode)
            same(tuple(a[per * i:per * i + per] for a in got), ref, "search, group %d" % g)
            for f in total:
                total[f] += rinfo[f]
        assert {f: sinfo[f] for f in total} == total and sinfo["queries"] == b and sinfo["iterations"] > b
        assert int(got[0][got[0] != sc.NONE].max()) - BASE >= EDGE  # (answers on the far side of the cut)
    finally:
        big.ix.drop_graph()


# ---------------------------------------------------------------- seam 4: the refinements
@pytest.mark.parametrize("rev_k", [0, 2])
def test_refinement_of_more_than_2_24_lines(za, big, graph2, rev_k):
    m, om, omode = za.L2SquaredDistance(), zo.L2SQ, 0
    in_k, k = 2, 8
    out = outputs(N, k)
    info = refine(big, graph2, in_k, rev_k, k, m, 0, N, out)
    assert info["lines"] == int(big.live.sum()) and info["launches"] == sc.sub_slabs(0, N, big.live) == -(-N // sc.REFINE_SLAB), info
    assert big.ix.stored_rows() > EDGE  # the row pass over the caller's graph (and with rev_k the selection) takes two launches
    if rev_k:
        assert info["edges"] > EDGE and info["kept"] > 0, info
    else:
        regular_groups_hold_the_template(big, out, in_k, k)
    # (b) the slab around row 2^24 on its own: one sub-slab, the same lines
    first, n = SLAB
    part = outputs(n, k)
    pinfo = refine(big, graph2, in_k, rev_k, k, m, first, n, part)
    assert pinfo["launches"] == 1 and pinfo["lines"] == int(big.live[first:first + n].sum())
    same(host(part, 0, n), host(out, first, first + n), "the slab, rev_k %d" % rev_k)
    # (a)
    for g in big.groups:
        s, e = big.tb.span(g)
        ref, _ = sc.local_refine(big.tb, *lines(graph2, s, e), g, k, om, omode, rev_k)
        same(host(out, s, e), ref, "rev_k %d group %d" % (rev_k, g))


# ---------------------------------------------------------------- seam 4: descent
DESCENT = (2, 4, 3)  # in_k, k, rounds


@pytest.fixture(scope="module", params=[0, 2])
def descended(request, za, big, graph2):
    """one zh_knn_graph_descent_device call over the whole table per rev_k (3 s: the tests below share it) -> (rev_k, the outputs on the device,
    the info)"""
    import torch
    in_k, k, rounds = DESCENT
    out = outputs(N, k)
    torch.cuda.synchronize()
    big.ix.knn_graph_descent_device(graph2[0].data_ptr(), graph2[1].data_ptr(), in_k, request.param, k, rounds, za.L2SquaredDistance(),
                                    *[o.data_ptr() for o in out])
    yield request.param, out, big.ix.knn_descent_info()
    del out
    torch.cuda.empty_cache()


def test_descent_of_more_than_2_24_lines_is_the_loop(za, big, graph2, descended):
    """(b) the loop its contract names, on the device, array for array; (c) the launches hold the zh_line_launches(N) = 2 terms -- which the
    library adds by formula, not per launch: they show that N is past the cut, the answer's checks show that the pieces were right"""
    import torch
    rev_k, out, info = descended
    in_k, k, rounds = DESCENT
    m = za.L2SquaredDistance()
    assert sc.line_launches(N) == 2 and info["rounds_run"] == rounds and info["launches"] == sc.descent_launches(N, big.live, in_k, rev_k, k, rounds, False), info
    cur, w, updates, keyed = graph2, in_k, [], []
    for _ in range(rounds):
        nxt = outputs(N, k)
        rinfo = refine(big, cur, w, rev_k, k, m, 0, N, nxt)
        updates.append(rinfo["updates"])
        keyed.append(rinfo["keyed"])
        cur, w = (nxt[0], nxt[2]), k
        last = nxt
    for a, b_, name in zip(out, last, ("ids", "keys", "counts")):
        assert torch.equal(a, b_), "descent and the loop differ in %s: %d places" % (name, int((a != b_).sum()))
    assert info["updates_round"] == updates and info["keyed_round"][0] == keyed[0] and all(a <= b_ for a, b_ in zip(info["keyed_round"], keyed))


def test_descent_of_more_than_2_24_lines_is_the_definition(big, graph2, descended):
    """(a) the checked groups against the local reference"""
    rev_k, out, info = descended
    in_k, k, rounds = DESCENT
    assert info["rounds_run"] == rounds
    for g in big.groups:
        s, e = big.tb.span(g)
        ref = sc.local_descent(big.tb, *lines(graph2, s, e), g, rev_k, k, rounds, zo.L2SQ, 0)
        same(host(out, s, e), ref, "descent rev_k %d group %d" % (rev_k, g))


# ---------------------------------------------------------------- seam 4': the transposition's edge passes at in_k = 64
def test_reverse_graph_at_in_k_64(za, big):
    """[N, 64] u64: 8.6 GB of device memory for the graph.  The edge passes take 2^30 / 64 = 2^24 lines a launch"""
    import torch
    in_k, rev_k = 64, 8
    assert N * in_k > sc.CSR_ENTRIES and sc.CSR_ENTRIES // in_k == EDGE
    graph = device_graph(big, in_k)
    first, n = SLAB
    out = outputs(n, rev_k, "degree")
    torch.cuda.synchronize()
    big.ix.knn_graph_reverse_device(graph[0].data_ptr(), graph[1].data_ptr(), in_k, rev_k, first, n, *[o.data_ptr() for o in out])
    info = big.ix.knn_reverse_info()
    assert info["lines"] == int(big.live[first:first + n].sum()) and info["launches"] == 2 and info["in_k"] == in_k, info
    # the info has no count of the edge passes' launches (`launches` is the selection's: zh_line_launches(2000) + 1): that they were cut rests on
    # N * in_k > 2^30 above; `edges` shows that the lines of both pieces were transposed
    assert info["edges"] > 63 * int(big.live.sum()) and info["max_degree"] == in_k, info
    got = host(out)
    kept = 0
    for g in range(first // P, (first + n - 1) // P + 1):
        s, e = big.tb.span(g)
        ref, rinfo = sc.local_reverse(big.tb, *lines(graph, s, e), g, rev_k)
        lo, hi = max(s, first), min(e, first + n)
        same_reverse(tuple(a[lo - first:hi - first] for a in got), tuple(a[lo - s:hi - s] for a in ref), "reverse group %d" % g)
        kept += int(ref[1][lo - s:hi - s].sum())
    assert kept == info["kept"] > 0
    del graph, out

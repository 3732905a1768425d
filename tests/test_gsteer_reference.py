"""The steered walk's reference (tests/gsteer_cases.py) against the unfiltered walk's (tests/gsearch_cases.py) where the two must agree, and the pinned
figures of the graphs gsteer_cases makes: the random out-32 graph whose second hop overflows the 256 candidate slots, the hand-built seams at the
truncation and around the bridge rules.  No GPU, no library."""
import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import gfilter_cases as fc
from tests import gsearch_cases as gc
from tests import gsteer_cases as sc


def same(a, b, what=""):
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all(), what


@pytest.mark.parametrize("case", [("t600", "exact", 32), ("t600", "exact", 5), ("t600", "repeats", 32), ("t600", "removed", 32), ("t600", "ring", 1)],
                         ids=lambda c: "-".join(map(str, c)))
def test_all_ones_is_the_unfiltered_walk(case):
    """every stored row allowed: A is the live rows, no entry is a bridge, a line of at most 256 / width entries never truncates -- ids, keys,
    counts and the seven walk figures are gsearch_cases.reference's for both hops"""
    tname, gname, g_k = case
    X, live = gc.table(tname)
    words, n_bits = fc.table_filter(tname, "ones")
    b = 4
    Q = gc.queries(tname, b)
    for beam, width, n_seed, max_iters, top_k in sc.SETTINGS:
        if width * g_k > 256:
            continue
        seeds = gc.default_seeds(b, n_seed, X.shape[0], 0)
        g = gc.graph(tname, gname, g_k)
        want, winfo = gc.reference(X, g, X.shape[0], g_k, live, 0, Q, seeds, top_k, beam, width, max_iters, zo.L2SQ, 0)
        for hops in (1, 2):
            got, info = sc.reference(X, g, X.shape[0], g_k, live, 0, Q, seeds, top_k, beam, width, max_iters, zo.L2SQ, 0, words, n_bits, hops)
            what = "%s %s hops %d" % (case, (beam, width, n_seed, max_iters, top_k), hops)
            same(got, want, what)
            assert {f: info[f] for f in sc.WALK_FIELDS} == winfo, what
            assert info["bridges"] == info["via_bridge"] == 0 and info["direct"] == info["keyed"] - info["seeds"], what
            assert info["rows_allowed"] == np.count_nonzero(live) and info["returned"] == int(want[2].sum()), what


def test_one_hop_never_bridges():
    for fname in fc.FILTERS:
        _, info = sc.run_case("t600", "exact", 32, 4, (33, 2, 8, 0, 10), fname, 1)
        assert info["bridges"] == info["via_bridge"] == 0 and info["keyed"] == info["seeds"] + info["direct"], fname


def test_two_hops_are_one_where_the_disallowed_rows_have_empty_lines():
    X, live = gc.table("t600")
    ids, counts = gc.graph("t600", "exact", 32)
    counts = counts.copy()
    counts[1::2] = 0
    words, n_bits = fc.table_filter("t600", "even")
    Q, seeds = gc.queries("t600", 6), gc.default_seeds(6, 32, 600, 0)
    one, i1 = sc.reference(X, (ids, counts), 600, 32, live, 0, Q, seeds, 10, 64, 2, 0, zo.L2SQ, 0, words, n_bits, 1)
    two, i2 = sc.reference(X, (ids, counts), 600, 32, live, 0, Q, seeds, 10, 64, 2, 0, zo.L2SQ, 0, words, n_bits, 2)
    same(one, two)
    assert i2["bridges"] > 0 and i2["via_bridge"] == 0
    assert {k: v for k, v in i1.items() if k != "bridges"} == {k: v for k, v in i2.items() if k != "bridges"}


def test_answers_are_allowed_sorted_and_keyed_by_the_oracle():
    X, live = gc.table("t600")
    for fname in ("even", "mod10_3", "short_garbage", "zeros", "removed_only"):
        words, n_bits = fc.table_filter("t600", fname)
        allowed = fc.allowed_rows(words, n_bits, live)
        for hops in (1, 2):
            (ids, keys, counts), info = sc.run_case("t600", "exact", 32, 4, (64, 4, 32, 0, 10), fname, hops)
            assert info["keyed"] == info["seeds"] + info["direct"] + info["via_bridge"]
            for i in range(4):
                c = int(counts[i])
                rows = ids[i, :c].astype(np.int64)
                assert allowed[rows].all() and np.unique(rows).size == c
                assert (np.lexsort((ids[i, :c], keys[i, :c])) == np.arange(c)).all()
                assert (keys[i, :c] == np.asarray(zo.distance_batch(zo.L2SQ, 0, X, gc.queries("t600", 4)[i]), np.uint64)[rows]).all()
            if fname in ("zeros", "removed_only"):
                assert info["rows_allowed"] == info["seeds"] == info["iterations"] == info["returned"] == 0


def test_the_random_graph_truncates():
    """(a): r % 2 == 0 allowed, width 4, out-degree 32 on 1500 rows -- about 64 direct rows and 64 bridges an iteration, a thousand second-hop
    entries over 643 allowed rows: all but the first iteration of a query fill the 256 slots"""
    _, one = sc.run_random_case(1)
    _, two = sc.run_random_case(2)
    assert one == dict(queries=4, seeds=56, iterations=72, expanded=276, keyed=3882, capped=0, launches=1, rows_allowed=643, direct=3826, via_bridge=0,
                       bridges=0, cand_full=0, returned=40)
    assert two == dict(queries=4, seeds=56, iterations=68, expanded=268, keyed=17389, capped=0, launches=1, rows_allowed=643, direct=3717,
                       via_bridge=13616, bridges=4184, cand_full=67, returned=40)


SEAM_PINS = {  # name -> hops 2: (keyed, direct, via_bridge, bridges, cand_full, the count per query); two queries, one iteration each
    "exact256": (514, 0, 512, 8, 2, 256),        # 1 seed + 4 x 64: the list is full and nothing was dropped
    "one_dropped": (514, 2, 510, 8, 2, 256),     # 1 direct row + the first 255 of the 256
    "removed_bridge": (22, 0, 20, 2, 0, 11),     # the removed row is no bridge; the live one brings its 10
    "late_bridge": (22, 0, 20, 4, 0, 11),        # the row past the attached lines is a bridge with an empty line
    "back_edges": (28, 0, 20, 2, 0, 14),         # the bridge's line names the four seeds again: only its 10 new rows are candidates
    "shared_bridge": (40, 0, 36, 6, 0, 20),      # three bridges an iteration, not five; their lines overlap in 5 rows: 10 + 5 + 3
}


@pytest.mark.parametrize("name", sc.SEAMS)
def test_the_seams(name):
    ((ids, keys, counts), info), g, g_rows, seeds, width = sc.run_seam(name, 2)
    keyed, direct, via, bridges, full, count = SEAM_PINS[name]
    assert (info["keyed"], info["direct"], info["via_bridge"], info["bridges"], info["cand_full"]) == (keyed, direct, via, bridges, full), info
    assert counts.tolist() == [count, count] and info["iterations"] == 2
    (_, _, c1), one = sc.run_seam(name, 1)[0]
    assert one["bridges"] == one["via_bridge"] == 0 and one["direct"] == direct
    even, odd, dead = sc._seam_rows()
    got = set(ids[0, :count].tolist())
    if name == "one_dropped":
        assert even[256] not in got  # the last entry of the last bridge is the one row dropped (and the beam of 256 loses one of the 257 keyed)
    if name == "removed_bridge":
        assert not got & set(even[101:131])  # nothing the removed row's line names


def test_exact256_keeps_every_row():
    """|cand| == 256 and beam 256: the seed and 255 of the 256 candidates make the beam -- all 257 rows were keyed (keyed == 514 above); with
    beam 256 exactly the farthest of the 257 is missing"""
    ((ids, keys, counts), info), *_ = sc.run_seam("exact256", 2)
    even, _, _ = sc._seam_rows()
    X, _ = gc.table(sc.SEAM_TABLE)
    for i in range(2):
        k = np.asarray(zo.distance_batch(zo.L2SQ, 0, X, gc.queries(sc.SEAM_TABLE, 2)[i]), np.uint64)
        rows = np.array(even[:257])
        want = rows[np.lexsort((rows, k[rows]))][:256]
        assert (ids[i] == want.astype(np.uint64)).all()


def test_two_hops_find_more_of_a_selective_filter_than_the_blind_walk():
    """the sign of the effect only: the 600-row exact 32-NN graph, every tenth row allowed, eight allowed seeds, beam 16 -- recall@10 against the
    exact filtered answer: 1.000 on 8980 keyed rows against the blind walk's 0.903 on 15 138.  The beam is small because the table is: at beam 64
    the blind walk keys 41 938 rows for 32 queries -- each of the 600 rows twice over -- and has 0.994 (two hops: 1.000), so the sign is still
    there but rests on two rows of 320; beam 16 is where a 600-row table leaves the blind walk something to miss"""
    X, live = gc.table("t600")
    b = 32
    Q = gc.queries("t600", b)
    words, n_bits = fc.table_filter("t600", "mod10_3")
    rows = np.flatnonzero(fc.allowed_rows(words, n_bits, live))
    truth = []
    for i in range(b):
        k = np.asarray(zo.distance_batch(zo.L2SQ, 0, X, Q[i]), np.uint64)
        truth.append(set(rows[np.lexsort((rows, k[rows]))[:10]].tolist()))
    g = gc.graph("t600", "exact", 32)
    seeds = sc.allowed_seeds(b, 8, words, n_bits, 0)

    def recall(ids):
        return sum(len(truth[i] & set(ids[i].tolist())) for i in range(b)) / (10.0 * b)

    blind, binfo = fc.reference(X, g, 600, 32, live, 0, Q, seeds, 10, 16, 1, 0, zo.L2SQ, 0, words, n_bits)
    two, tinfo = sc.reference(X, g, 600, 32, live, 0, Q, seeds, 10, 16, 1, 0, zo.L2SQ, 0, words, n_bits, 2)
    assert recall(two[0]) > recall(blind[0])
    assert tinfo["keyed"] < binfo["keyed"]  # ... on fewer keyed rows

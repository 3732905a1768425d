"""tests/gfilter_cases.py pinned on the CPU: the set form (the first top_k of the allowed rows that ever got a key) and the incremental form (a list
R updated per iteration with "minus the rows in R now") agree on every filter x setting of two tables and two graphs; the walk's figures are
gsearch_cases.reference's whatever the filter; the all-ones answer is gsearch_cases.reference's; and re-offers of both kinds -- a row that is in R
when it comes again, a row that was rejected or pushed out earlier -- happen at test size.  No GPU, no library."""
import numpy as np
import pytest

from tests import gfilter_cases as fc
from tests import gsearch_cases as gc

QUERIES = 8
CASES = [("t600", "exact"), ("t600", "block"), ("t1500", "exact")]
WALK_FIELDS = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches")


def same(a, b, what):
    for x, y, name in zip(a, b, ("ids", "keys", "counts")):
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (what, name)


@pytest.mark.parametrize("tname,gname", CASES, ids=["%s-%s" % c for c in CASES])
def test_the_two_forms_agree_and_the_walk_is_untouched(tname, gname):
    settings = fc.SETTINGS if tname == "t600" else fc.SETTINGS[1:5]
    for setting in settings:
        beam, width, n_seed, max_iters, top_k = setting
        plain, pinfo = gc.run_case(tname, gname, 32, QUERIES, (beam, width, n_seed, max_iters), top_k=top_k)
        for fname in fc.FILTERS:
            s, si = fc.run_case(tname, gname, 32, QUERIES, setting, fname)
            i, ii = fc.run_case(tname, gname, 32, QUERIES, setting, fname, form="incremental")
            same(s, i, (setting, fname))
            assert si == ii, (setting, fname)
            assert {f: si[f] for f in WALK_FIELDS} == pinfo, (setting, fname)
            assert si["returned"] == int(s[2].sum()) and si["offered"] >= si["returned"]
            if fname == "ones":
                same(s, plain, (setting, "all ones: the unfiltered answer"))
                assert si["offered"] == si["keyed"]
            if fname in ("zeros", "removed_only"):
                assert si["rows_allowed"] == 0 and si["offered"] == 0 and (s[2] == 0).all() and (s[0] == gc.NONE).all() and (s[1] == gc.NONE).all()


def test_the_answer_is_allowed_sorted_and_tailed():
    X, live = gc.table("t600")
    for fname in ("even", "short_garbage", "one_row"):
        words, n_bits = fc.table_filter("t600", fname)
        allowed = fc.allowed_rows(words, n_bits, live)
        (ids, keys, counts), info = fc.run_case("t600", "exact", 32, QUERIES, (33, 2, 8, 0, 10), fname)
        assert info["rows_allowed"] == np.count_nonzero(allowed)
        for b in range(QUERIES):
            c = int(counts[b])
            pairs = list(zip(keys[b, :c].tolist(), ids[b, :c].tolist()))
            assert pairs == sorted(pairs) and len(set(ids[b, :c].tolist())) == c and allowed[ids[b, :c].astype(np.int64)].all()
            assert (ids[b, c:] == gc.NONE).all() and (keys[b, c:] == gc.NONE).all()
    words, n_bits = fc.table_filter("t600", "short_garbage")
    assert n_bits == 600 - 37 and n_bits % 32 and int(words[-1]) >> (n_bits % 32) == (1 << (32 - n_bits % 32)) - 1  # (the spare bits ARE set)
    assert not fc.allowed_rows(words, n_bits, live)[n_bits:].any()
    assert fc.allowed_rows(*fc.table_filter("t600", "one_row"), live).sum() == 1


def test_both_kinds_of_reoffer_happen():
    """t600, the exact 32-NN graph, every second row allowed, (beam, width, n_seed, top_k) = (8, 1, 8, 8): rows come again while they are in R (103
    times over the 8 queries) and after they were rejected (330 times); the two forms agree all the same.  With every row allowed R is the head of
    the beam, and "minus the rows in B now" leaves nothing that R holds."""
    again = []
    i, _ = fc.run_case("t600", "exact", 32, QUERIES, (8, 1, 8, 0, 8), "even", form="incremental", reoffers=again)
    assert again == [103, 330]
    same(i, fc.run_case("t600", "exact", 32, QUERIES, (8, 1, 8, 0, 8), "even")[0], "even")
    for tname, gname in (("t600", "block"), ("t1500", "exact")):
        for setting in ((8, 1, 8, 0, 8), (64, 1, 32, 0, 64)):
            for fname in ("even", "mod10_3"):
                again = []
                fc.run_case(tname, gname, 32, QUERIES, setting, fname, form="incremental", reoffers=again)
                full = np.count_nonzero(fc.allowed_rows(*fc.table_filter(tname, fname), gc.table(tname)[1])) > setting[4]  # (R can fill up)
                assert again[0] > 0 and (again[1] > 0) == full, (tname, gname, setting, fname, again)
    again = []
    fc.run_case("t600", "exact", 32, QUERIES, (8, 1, 8, 0, 8), "ones", form="incremental", reoffers=again)
    assert again[0] == 0

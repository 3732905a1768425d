"""tests/gsearch_cases.py pinned on the CPU: on every entry of CASES x SETTINGS the definition ("cand minus the rows in the beam now") and the
textbook rule ("cand minus every row keyed so far") give the same answers and the same iteration counts, the textbook rule never keys more, and the
info figures of the four NAMED cases are the ones worked out when the feature was specified (default seeds, L2SQ, id_base 0).  No GPU, no library."""
import numpy as np
import pytest

from tests import gsearch_cases as gc


@pytest.mark.parametrize("tname,gname,g_k", gc.CASES, ids=["%s-%s-%d" % c for c in gc.CASES])
def test_the_two_rules_agree(tname, gname, g_k):
    ran = 0
    for setting in gc.SETTINGS:
        if setting[1] * g_k > 256:
            continue  # (width * g_k <= 256)
        a, ia = gc.run_case(tname, gname, g_k, gc.EQ_QUERIES, setting)
        t, it = gc.run_case(tname, gname, g_k, gc.EQ_QUERIES, setting, textbook=True)
        for x, y, name in zip(a, t, ("ids", "keys", "counts")):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (setting, name)
        for f in ("queries", "seeds", "iterations", "expanded", "capped", "launches"):
            assert ia[f] == it[f], (setting, f)
        assert it["keyed"] <= ia["keyed"], setting
        ran += 1
    assert ran >= 12


def test_the_answer_is_sorted_and_tailed():
    (ids, keys, counts), info = gc.run_case("t600", "exact", 32, 8, (33, 2, 8, 0), top_k=10)
    assert (counts == 10).all() and info["capped"] == 0
    for b in range(8):
        pairs = list(zip(keys[b].tolist(), ids[b].tolist()))
        assert pairs == sorted(pairs) and len(set(ids[b].tolist())) == 10
    (ids, keys, counts), _ = gc.run_case("t600", "zero_counts", 32, 4, (256, 1, 1, 0))
    assert ((ids == gc.NONE) == (np.arange(256)[None, :] >= counts[:, None])).all() and ((keys == gc.NONE) == (ids == gc.NONE)).all()


def figures(name):
    tname, gname, g_k, b, setting = gc.NAMED[name]
    return gc.run_case(tname, gname, g_k, b, setting)[1], gc.run_case(tname, gname, g_k, b, setting, textbook=True)[1]


def test_exact32_beam64_figures():
    info, text = figures("exact32_beam64")
    assert info == {"queries": 64, "seeds": 1792, "iterations": 4125, "expanded": 4125, "keyed": 98066, "capped": 0, "launches": 1}
    assert text["keyed"] == 39771 and text["iterations"] == 4125


def test_exact32_beam256_w8_figures():
    info, text = figures("exact32_beam256_w8")
    assert info == {"queries": 64, "seeds": 1792, "iterations": 2104, "expanded": 16574, "keyed": 219474, "capped": 0, "launches": 1}
    assert text["keyed"] == 64368 and text["iterations"] == 2104


def test_block_beam33_w2_figures():
    info, text = figures("block_beam33_w2")
    assert info == {"queries": 64, "seeds": 448, "iterations": 1279, "expanded": 2486, "keyed": 49308, "capped": 0, "launches": 1}
    assert text["keyed"] == 18100


def test_ring1_capped_figures():
    """g_k = 1, three iterations allowed: every query expands three rows and is stopped with the fourth still unexpanded"""
    info, text = figures("ring1_capped")
    assert info == {"queries": 64, "seeds": 448, "iterations": 192, "expanded": 192, "keyed": 598, "capped": 64, "launches": 1}
    assert text["keyed"] == 598

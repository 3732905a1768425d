"""tests/descent_cases.py pinned on the CPU: on the four cases of the NN-descent tests the line the incremental definition gives equals the full
round's line for every live row and every round, and the per-round figures are the ones worked out when the feature was specified (rc.table(n, 30),
rc.removed_rows(n) removed, id_base 0).  No GPU, no library."""
import functools

import numpy as np
import pytest

from tests import descent_cases as dc

ROUNDS = 12


@functools.lru_cache(maxsize=None)
def run(number):
    X, live, graph, mi, in_k, k, rev_k = dc.case(number)
    om, omode = dc.ORACLE_METRIC[mi]
    return dc.descent(X, graph, in_k, rev_k, k, ROUNDS, live, 0, om, omode) + (live,)


@pytest.mark.parametrize("number", sorted(dc.CASES))
def test_incremental_lines_are_the_full_rounds_lines(number):
    answer, info, full, inc, live = run(number)
    assert len(full) == len(inc) == info["rounds_run"]
    for r, (f, i) in enumerate(zip(full, inc)):
        for a, b, name in zip(f, i, ("ids", "keys", "counts")):
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (number, r + 1, name)
        assert (f[2][~live] == 0).all() and (f[0][~live] == dc.NONE).all()
    assert all((a == b).all() for a, b in zip(answer, full[-1]))
    # a round keys no more than the full round, and strictly less once a line is inactive
    for r in range(1, info["rounds_run"]):
        assert info["keyed_round"][r] <= info["full_keyed_round"][r]
        if info["active_round"][r] < int(live.sum()):
            assert info["keyed_round"][r] < info["full_keyed_round"][r]


def test_case_1_figures():
    _, info, _, _, live = run(1)
    assert int(live.sum()) == 1284
    assert info["rounds_run"] == 10 and info["updates_round"][-1] == 0 and all(u > 0 for u in info["updates_round"][:-1])  # the fixed point
    assert info["keyed_round"] == [321455, 530559, 454709, 280335, 59508, 13937, 3425, 1308, 357, 55]
    assert info["full_keyed_round"][:2] == [321455, 572642] and info["full_keyed_round"][-1] == 518758
    assert info["active_round"][0] == 1284 and info["active_round"][-1] == 4
    assert all(a >= b for a, b in zip(info["active_round"], info["active_round"][1:]))


def test_case_2_figures():
    _, info, _, _, live = run(2)
    assert info["rounds_run"] == 12 and info["updates_round"][-1] == 0 and info["updates_round"][-2] > 0
    assert info["full_keyed_round"][-1] == 143649 and info["keyed_round"][-1] == 104 and info["active_round"][-1] == 58


def test_case_3_figures():
    """width 45 + 19 = 64: the early rounds' lines gather more than 2048 entries, the late ones' fewer"""
    _, info, _, _, live = run(3)
    assert int(live.sum()) == 1027
    assert info["rounds_run"] == 7 and info["updates_round"][-1] == 0 and info["updates_round"][-2] > 0
    assert info["full_keyed_round"][-1] == 811631 and info["keyed_round"][-1] == 167 and info["active_round"][-1] == 77
    assert info["listed_round"][1] > 2048 * 1027 and info["listed_round"][-1] < 2048


def test_case_4_figures():
    _, info, _, _, live = run(4)
    assert info["rounds_run"] == ROUNDS and info["updates_round"][-1] == 80  # the rounds limit ends the call
    assert info["full_keyed_round"][-1] == 62625 and info["keyed_round"][-1] == 810 and info["active_round"][-1] == 162 and int(live.sum()) == 1284


@pytest.mark.parametrize("number", sorted(dc.CASES))
def test_every_case_has_inactive_lines_and_mixed_lines(number):
    """rounds with inactive lines, and rounds with lines that mix old and new own entries"""
    X, live, graph, mi, in_k, k, rev_k = dc.case(number)
    _, info, full, _, _ = run(number)
    assert min(info["active_round"]) < int(live.sum())
    mixed = 0
    g, w = (graph[0], graph[-1]), in_k
    _, U_old = dc.union_lines(g, w, rev_k, live, 0)
    for r in range(min(3, info["rounds_run"] - 1)):
        _, U = dc.union_lines((full[r][0], full[r][2]), k, rev_k, live, 0)
        for a in np.flatnonzero(live).tolist():
            fresh = np.setdiff1d(U[a], U_old[a]).size
            mixed += 1 if 0 < fresh < U[a].size else 0
        U_old = U
    assert mixed > 0

"""The graph extension's reference (tests/gextend_cases.py) pinned on the CPU: no GPU, no library.

What the definition promises is asserted on every case the GPU test runs: an old line that no new line names is unchanged word for word; a new
line and a re-ranked line hold no row twice and no removed row, and a line never GAINS its own row (a re-ranked line keeps it only where the
attached graph had it: rc.GRAPHS' self loops); a re-ranked line is sorted by (key, id) and position by position never worse than L'(r) alone.
Non-vacuity comes from the reference alone: every case offers and keeps reverse edges, and the hub case's longest R(r) is past one block pass.
The quality figures are the reference's own overlap with the exact graph, pinned; the library is held to the reference id for id on the GPU."""
import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import gextend_cases as ge
from tests import gsearch_cases as gc

NAMES = sorted(ge.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_what_the_definition_promises(name):
    case = ge.CASES[name]
    tname, G, variant, _, g_k, (om, omode), (beam, width, n_seed, max_iters), batch, id_base, _ = case
    X, live0, live, g, start, seeds = ge.inputs(case)
    lines, info, (ids, counts), trace = ge.expected(case, with_trace=True)
    K = ge.keys_of(tname, G, variant, om, omode)
    N = X.shape[0]
    assert len(lines) == N and ids.shape == (N, g_k) and counts.shape == (N,)
    assert info["chunks"] == len(trace) == -(-(N - G) // batch)
    assert info["rows_added"] == int(live[G:].sum()) and info["rows_removed"] == int((~live[G:]).sum())
    touched = set()
    for lo, t in trace.items():
        touched |= set(t)
        for r, (R, Lp) in t.items():
            assert r < lo and live[r] and R == sorted(set(R)) and all(lo <= a < lo + batch and live[a] for a in R)
            assert all(x < lo for x in Lp)
    # ---- untouched old lines: word for word
    for r in range(G):
        if r not in touched:
            assert lines[r] == start[r], r
    if batch >= N - G and G:
        assert any(r not in touched for r in range(G)), "vacuous: every old line was re-ranked"
    # ---- new lines and re-ranked lines
    for a in list(range(G, N)) + sorted(touched):
        x = lines[a]
        assert len(x) == len(set(x)) <= g_k, a
        assert all(live[v] for v in x), a
        assert a not in x or (a < G and a in start[a]), a
        if not live[a]:
            assert x == []
    for a in range(G, N):
        if a not in touched:  # (as the walk left it: no row of its own chunk or a later one)
            assert all(v < G + (a - G) // batch * batch for v in lines[a]), a
    # ---- the last re-ranking of a row: sorted, and never worse than L'(r) alone
    last = {}
    for lo in sorted(trace):
        for r, v in trace[lo].items():
            last[r] = (lo, v)
    final_chunk = max(trace) if trace else None
    for r, (lo, (R, Lp)) in last.items():
        kr = K[r]
        if lo == final_chunk or all(r not in trace[l2] for l2 in trace if l2 > lo):
            pairs = [(int(kr[x]), x) for x in lines[r]]
            assert pairs == sorted(pairs), r
            alone = sorted((int(kr[x]), x) for x in Lp)[:g_k]
            assert len(pairs) >= len(alone) and all(p <= q for p, q in zip(pairs, alone)), r
    # ---- non-vacuity
    assert info["reverse_offered"] > 0 and info["reverse_kept"] > 0 and info["reverse_rows"] > 0, info
    assert info["reverse_offered"] == sum(len(R) for t in trace.values() for R, _ in t.values())
    # ---- the arrays
    for a in range(N):
        c = int(counts[a])
        assert c == len(lines[a]) and (ids[a, :c] == np.asarray(lines[a], np.uint64) + np.uint64(id_base)).all() and (ids[a, c:] == ge.NONE).all()


def test_the_hub_case_is_longer_than_one_block_pass():
    _, _, _, trace = ge.expected(ge.CASES[ge.HUB], with_trace=True)
    longest = max(len(R) for t in trace.values() for R, _ in t.values())
    assert longest == len(trace[1200][0][0]) == 300 > 256


def test_batch_one_is_sequential_and_chunks_matter():
    """batch = 1 lets a new row name the new rows before it; one chunk for all lets none: the tables differ, and only in that way"""
    seq, _, _ = ge.expected(ge.CASES["batch1"])
    one, _, _ = ge.expected(ge.CASES["batch128"])
    assert any(v >= 500 for a in range(500, 600) for v in seq[a])
    assert not any(v >= 500 for a in range(500, 600) for v in one[a])
    assert seq != one


def test_kept_table_is_the_walks_lines_in_table_order():
    for name in ("graph_repeats", "graph_out_of_range", "graph_zero_counts", "graph_removed", "graph_all_ones"):
        case = ge.CASES[name]
        _, G, _, _, g_k, _, _, _, id_base, _ = case
        _, live0, _, g, start, _ = ge.inputs(case)
        walk_lines = gc.kept_lines(g, G, g_k, id_base, G)
        for p in range(G):
            assert sorted(start[p]) == [int(v) for v in walk_lines[p] if live0[v]], (name, p)


# the reference's own overlap with the exact 32-NN graph of all 1500 rows after extending the exact 32-NN graph of the first 1200 (L2SQ, beam 64,
# width 1, 32 strided seeds): batch -> (new rows' lines, old rows' lines)
QUALITY = {1: (0.9322916666666666, 0.9070833333333334), 64: (0.90875, 0.908125), 512: (0.8020833333333334, 0.9115364583333333)}


@pytest.mark.parametrize("batch", sorted(QUALITY))
def test_quality_is_pinned(batch):
    got = ge.overlap_with_exact(batch)
    print("overlap", batch, got)
    assert got == pytest.approx(QUALITY[batch], abs=1e-12)

"""tests/stream_cases.py on the CPU: the case keeps the promises tests/test_gpu_caller_stream.py relies on -- no reference key is a NaN (fc.key_matrix
asserts it while the case is made), every range line and both joins have a hit, the capacity-short calls are short, 8192 live and allowed-live
rows, path 2 for every family at this shape and path 1 under the override -- and its shapes are the ones the issue of the protocol names."""
import numpy as np
import pytest

from tests import family_cases as fc
from tests import stream_cases as sc


@pytest.fixture(scope="module")
def case():
    return sc.case()


def test_shapes(case):
    p = case.p
    assert p["d"] == fc.MFMA_DIMS[0] == 256 and p["max_node_size"] >= fc.GATE_NODE and p["num_trees"] == 4 and p["k"] == 10
    assert p["B"] == 24 and p["B"] > 16 and p["B"] % 16  # one full and one partial 16-query tile
    assert case.X.shape == (8407, 256) and case.X.shape[0] % 16  # the last row tile is partial
    assert case.slab.size == 48 and case.slab[0] > 0 and not case.alive[case.slab].all() and case.alive[case.slab].any()
    assert 100 <= case.XL.shape[0] <= 999 and 0 < case.goneL.size < case.XL.shape[0]
    assert case.sample.size == 16 and case.alive[case.sample].all()
    assert fc.METRICS[sc.METRICS[0]][2] == 0 and sc.METRICS[1] in fc.OTHER_METRICS
    assert int(case.aliveL.sum()) * int(case.alive.sum()) < fc.GATE_PAIRS  # the cross join's own gate is far: path 2 needs the override


def test_live_and_allowed_rows_sit_on_the_gate(case):
    assert int(case.alive.sum()) == fc.GATE_ROWS and int(case.allowed_live.sum()) >= fc.GATE_ROWS
    assert fc.filter_tile_rule(case.allowed_live)
    assert case.allowed[~case.alive].any() and not case.allowed[~case.alive].all()  # removed rows' bits are arbitrary: the live bitmap must mask them
    assert not (case.leaf_of[:, ~case.alive] >= 0).any() and (case.leaf_of[:, case.alive] >= 0).all()


@pytest.mark.parametrize("metric", sc.METRICS)
def test_no_key_is_a_nan(case, metric):
    r = case.refs[metric]
    for K in (r.KQ, r.KS, r.KA, r.KX):
        assert not fc.key_is_nan(K, r.spec).any()


@pytest.mark.parametrize("metric", sc.METRICS)
def test_every_range_line_and_both_joins_have_a_hit(case, metric):
    r = case.refs[metric]
    for name in ("range", "frange"):
        off = getattr(r, name)[0]
        assert off.size == case.p["B"] + 1 and (np.diff(off.astype(np.int64)) >= 1).all(), (name, np.diff(off.astype(np.int64)).tolist())
    assert (np.diff(r.frange[0].astype(np.int64)) <= np.diff(r.range[0].astype(np.int64))).any()
    for name in ("join", "fjoin", "cross"):
        assert getattr(r, name)[0].size >= 2, name
    assert r.fjoin[0].size <= r.join[0].size
    # the stale inputs of the protocol answer differently: thresholds of 0, the queries rolled by one
    for name, mask in (("range", case.alive), ("frange", case.vis)):
        stale = fc.range_ref(r.KQ, mask, np.zeros(case.p["B"], np.uint64), case.base)
        assert int(stale[0][-1]) != int(getattr(r, name)[0][-1])
    rolled = fc.topk_ref(np.roll(r.KQ, 1, axis=0), case.alive, case.p["k"], case.base)
    assert (rolled[0] != r.exact[0]).any(1).all()  # every line of the exact answer tells the two apart


@pytest.mark.parametrize("metric", sc.METRICS)
def test_graph_lines(case, metric):
    r = case.refs[metric]
    k = case.p["k"]
    assert ((r.knn[2] == k) == case.alive[case.slab]).all() and (r.knn[2][~case.alive[case.slab]] == 0).all()
    assert (r.fknn[2] > 0).any() and (r.fknn[2] <= r.knn[2]).all()
    assert (r.exact[2] == k).all() and (r.filtered[2] == k).all()


@pytest.mark.parametrize("metric", sc.METRICS)
def test_the_short_calls_are_short(case, metric):
    r = case.refs[metric]
    assert set(r.short_cap) == set(sc.SHORT)
    for fam in sc.SHORT:
        assert 1 <= r.short_cap[fam] < r.least_total[fam], fam


def test_paths(case):
    calls = sc.steady_calls()
    assert {f for f, _ in calls} == set(fc.FAMILIES) and len(calls) == 26
    for fam in fc.FAMILIES:
        assert case.expected_path(fam, "path2") == 2, fam
        assert case.expected_path(fam, "other") == 1, fam
        if fc.PATH_ENV[fam][0]:
            assert case.expected_path(fam, "forced1") == 1 and sc.mode_override(fam, "forced1") == 1, fam
    # path 2 is reached by the rule alone, except where the gate is out of the case's reach and "2" is a documented value of the switch
    for fam in fc.FAMILIES:
        ov = sc.mode_override(fam, "path2")
        assert ov is None or (ov == 2 and fc.PATH_ENV[fam][1]), fam


def test_the_lsh_reference(case):
    ids, keys, counts = case.lsh
    assert ids.shape == (case.p["B"], case.p["k"]) and (counts > 0).all()
    live = ids[np.arange(case.p["k"])[None, :] < counts[:, None]]
    assert case.alive[live.astype(np.int64)].all()

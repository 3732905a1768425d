"""The shard merge's plain reference (tests/merge_cases.py) against a literal Python restatement and against the oracle's
zo_merge_topk, on every input family the device tests feed; and the device tests' case table against what it promises to cover.
No GPU needed: this keeps the reference honest on any machine."""
import numpy as np
import pytest

from oracle import zebra_oracle as zo
from tests import merge_cases as mc

SMALL = [(1, 1, 1), (1, 3, 7), (2, 4, 5), (3, 5, 12), (4, 2, 1), (8, 3, 9), (5, 4, 33), (16, 2, 4)]  # (S, B, k)


def _as_pairs(out_ids, out_keys, out_counts):
    return [[(int(out_keys[b, i]), int(out_ids[b, i])) for i in range(int(out_counts[b]))] for b in range(out_ids.shape[0])]


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_reference_equals_literal_python(family):
    for S, B, k in SMALL:
        for seed in range(6):
            ids, keys, counts = mc.make_case(family, S, B, k, seed)
            oi, ok, oc = mc.merge_reference(ids, keys, counts, k)
            assert _as_pairs(oi, ok, oc) == mc.merge_literal(ids, keys, counts, k), (S, B, k, seed)
            past = np.arange(k)[None, :] >= oc[:, None]
            assert (oi[past] == mc.ONES).all() and (ok[past] == mc.ONES).all()


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_reference_equals_oracle(family):
    for S, B, k in SMALL + [(3, 3, 342), (7, 2, 100), (40, 2, 64)]:
        for seed in range(4):
            ids, keys, counts = mc.make_case(family, S, B, k, seed)
            want = mc.merge_reference(ids, keys, counts, k)
            got = zo.merge_topk(ids, keys, counts, k)
            assert (got[2] == want[2]).all(), (S, B, k, seed)
            assert _as_pairs(*got) == _as_pairs(*want), (S, B, k, seed)


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_families_are_deterministic_and_well_formed(family):
    for S, B, k in SMALL:
        a, b = mc.make_case(family, S, B, k, 3), mc.make_case(family, S, B, k, 3)
        assert all((x == y).all() for x, y in zip(a, b))
        ids, keys, counts = a
        assert ids.dtype == np.uint64 and keys.dtype == np.uint64 and counts.dtype == np.uint32
        assert ids.shape == keys.shape == (S, B, k) and counts.shape == (S, B)
        inside = np.arange(k)[None, None, :] < counts[:, :, None]
        assert not ((ids == mc.ONES) & (keys == mc.ONES) & inside).any()  # the invalid marker is never fed as an entry
        for b in range(B):  # within a query, a repeated id carries the same key
            seen = {}
            for i, key in zip(ids[:, b][inside[:, b]].tolist(), keys[:, b][inside[:, b]].tolist()):
                assert seen.setdefault(i, key) == key


def test_families_reach_what_they_are_named_for():
    """each family really holds the situation it exists for (a generator that stopped producing it would test nothing)"""
    S, B, k = 4, 8, 6
    seeds = range(4)
    # ties: more than k entries share the key at the cut, so the id decides it
    hit = 0
    for seed in seeds:
        ids, keys, counts = mc.make_case("ties", S, B, k, seed)
        oi, ok, oc = mc.merge_reference(ids, keys, counts, k)
        for b in range(B):
            valid = np.arange(k)[None, :] < counts[:, b][:, None]
            hit += int(oc[b] == k and (keys[:, b, :][valid] == ok[b, k - 1]).sum() > (ok[b] == ok[b, k - 1]).sum())
    assert hit
    # ragged: every edge count, empty queries, short sums, single lists
    ids, keys, counts = mc.make_case("ragged", S, B, k, 0)
    assert set(counts.ravel().tolist()) >= {0, 1, k - 1, k}
    sums, nonzero = counts.sum(0), (counts > 0).sum(0)
    assert (sums == 0).any() and ((sums > 0) & (sums < k)).any() and (nonzero == 1).any()
    assert (mc.merge_reference(ids, keys, counts, k)[2][sums == 0] == 0).all()
    # duplicates: identical lists, and a second copy of the k-th best
    ids, keys, counts = mc.make_case("duplicates", S, B, k, 0)
    oi, ok, oc = mc.merge_reference(ids, keys, counts, k)
    same = [b for b in range(B) if all((ids[s, b] == ids[0, b]).all() for s in range(S))]
    assert same and all(sorted(oi[b, :oc[b]].tolist()) == sorted(ids[0, b, :counts[0, b]].tolist()) for b in same)
    kth_twice = [b for b in range(B) if oc[b] == k and (ids[:, b, :] == oi[b, k - 1]).sum() > 1]
    assert kth_twice
    # ... and copies more than 1024 source slots apart on a streaming shape
    S2, k2 = 8, 512
    ids, keys, counts = mc.make_case("duplicates", S2, 3, k2, 0)
    b = [b for b in range(3) if b % 3 == 2][0]
    assert (ids[S2 // 2:, b, ::2] == ids[:S2 // 2, b, ::2]).all() and S2 // 2 * k2 > 1024
    # extremes
    ids, keys, counts = mc.make_case("extremes", S, B, k, 0)
    inside = np.arange(k)[None, None, :] < counts[:, :, None]
    assert set(mc.KEY_EXTREMES.tolist()) <= set(keys[inside].tolist())
    assert (ids[inside] >= 2**32).all()
    for S1, B1, k1, seed in ((S, B, k, 0), (2, 1, 512, 46), (3, 1, 342, 44), (5, 7, 1, 1)):  # every query that has entries is fed the id 2**64 - 2
        ids, keys, counts = mc.make_case("extremes", S1, B1, k1, seed)
        inside = np.arange(k1)[None, None, :] < counts[:, :, None]
        assert (((ids == 2**64 - 2) & inside).sum((0, 2)) == (counts.sum(0) > 0)).all(), (S1, B1, k1, seed)
    # poisoned padding would win if it were read
    ids, keys, counts = mc.make_case("poisoned", S, B, k, 0)
    inside = np.arange(k)[None, None, :] < counts[:, :, None]
    assert (~inside).any() and keys[~inside].max() < keys[inside].min() and (ids[~inside] != mc.ONES).all()
    # counts above k
    ids, keys, counts = mc.make_case("counts_above_k", S, B, k, 0)
    assert (counts == k + 7).any(0).all()


def test_device_cases_cover_every_family_on_every_path():
    cases = mc.device_cases()
    assert len(set(cases)) == len(cases)
    shapes = {(S, k) for _, S, k, _, _ in cases}
    assert shapes == set(mc.WAVE_SHAPES) | set(mc.BOUNDARY_SHAPES) | set(mc.TILED_SHAPES)
    assert [mc.shape_path(S, k) for S, k in mc.WAVE_SHAPES] == ["wave"] * 8
    assert [mc.shape_path(S, k) for S, k in mc.BOUNDARY_SHAPES] == ["boundary"] * 4
    assert [mc.shape_path(S, k) for S, k in mc.TILED_SHAPES] == ["tiled"] * 4
    for family in mc.FAMILIES:
        assert {mc.shape_path(S, k) for f, S, k, _, _ in cases if f == family} == {"wave", "boundary", "tiled"}, family
    for path in ("wave", "boundary"):
        assert {B for _, S, k, B, _ in cases if mc.shape_path(S, k) == path} == set(mc.BATCHES), path
    assert {B for _, S, k, B, _ in cases if mc.shape_path(S, k) == "tiled"} >= {1, 3, 13}
    for _, S, k, B, _ in cases:
        assert 2 * 2 * 8 * S * B * k <= 100 << 20 or B <= 3  # ids + keys, plain and packed
        assert B <= 4 or S * k < 2**20

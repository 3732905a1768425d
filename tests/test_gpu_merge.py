"""The two shard merge kernels (merge_wave_kernel up to 1024 entries per query, the streaming final_kernel<true> past that;
zebra_amd/csrc/zh_search.hip) through both entry points, zh_merge_topk_device and zh_merge_topk_packed_device, against the plain
reference of tests/merge_cases.py, on the input families that module draws and at the shapes where the code changes path.

Every case checks: out_counts; the first out_counts ids and keys bit for bit; every later output slot all-ones (the outputs hold
a poison value before the call); the inputs unchanged; a guard row before and after each output unchanged."""
import numpy as np
import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from tests import merge_cases as mc

pytestmark = pytest.mark.gpu

POISON64 = 0x5A5A5A5A5A5A5A5A  # (positive as an int64)
POISON32 = 0x5A5A5A5A
GUARD = 16  # counts: this many words before and after


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def _outputs(torch, B, k):
    """out_ids, out_keys [B + 2, k] and out_counts [B + 2 * GUARD], all poison: the kernels write rows 1..B / words GUARD..GUARD+B"""
    return (torch.full((B + 2, k), POISON64, dtype=torch.int64, device="cuda"),
            torch.full((B + 2, k), POISON64, dtype=torch.int64, device="cuda"),
            torch.full((B + 2 * GUARD,), POISON32, dtype=torch.int32, device="cuda"))


def _check_outputs(out, want, B, k, tag):
    o_ids, o_keys, o_counts = (t.cpu().numpy() for t in out)
    for name, t in (("ids", o_ids), ("keys", o_keys)):
        assert (t[0] == POISON64).all() and (t[B + 1] == POISON64).all(), (tag, name, "guard row written")
    assert (o_counts[:GUARD] == POISON32).all() and (o_counts[GUARD + B:] == POISON32).all(), (tag, "counts guard written")
    gi, gk, gc = o_ids[1:B + 1].view(np.uint64), o_keys[1:B + 1].view(np.uint64), o_counts[GUARD:GUARD + B].view(np.uint32)
    wi, wk, wc = want
    bad = np.nonzero(gc != wc)[0]
    assert bad.size == 0, (tag, "out_counts", bad[:8].tolist(), gc[bad[:8]].tolist(), wc[bad[:8]].tolist())
    # the reference's tail is all-ones as well: one comparison covers the first out_counts entries and every slot after them
    for name, g, w in (("ids", gi, wi), ("keys", gk, wk)):
        rows = np.nonzero((g != w).any(1))[0]
        if rows.size:
            b = int(rows[0])
            j = int(np.nonzero(g[b] != w[b])[0][0])
            lo = max(j - 2, 0)
            raise AssertionError((tag, name, "query %d slot %d of count %d" % (b, j, wc[b]), "got", g[b, lo:j + 3].tolist(),
                                  "want", w[b, lo:j + 3].tolist(), "%d queries differ" % rows.size))


def run_merge(za, ids, keys, counts, k, side_stream=False, tag=None):
    """both entry points on one input, every assertion of the module's docstring"""
    import torch
    from zebra_amd import sharding
    S, B, _ = ids.shape
    want = mc.merge_reference(ids, keys, counts, k)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    t_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    W = za.packed_result_words(B, k)
    assert W == 2 * B * k + (B + 1) // 2
    # the packed layout: one buffer per shard; the padding word of an odd B holds poison, not a count
    g_packed = torch.full((S, W), POISON64, dtype=torch.int64, device="cuda")
    for s in range(S):
        a, b_, c = sharding.packed_views(torch, g_packed[s], B, k)
        assert a.shape == (B, k) and b_.shape == (B, k) and c.shape == (B,)
        a.copy_(t_ids[s]), b_.copy_(t_keys[s]), c.copy_(t_counts[s])
    # the same layout written down on the host: what the device buffers must still hold after the calls
    h_packed = np.full((S, W), POISON64, np.int64)
    h_packed[:, :B * k], h_packed[:, B * k:2 * B * k] = ids.reshape(S, -1).view(np.int64), keys.reshape(S, -1).view(np.int64)
    h_packed[:, 2 * B * k:].view(np.int32)[:, :B] = counts.view(np.int32)
    plain, packed = _outputs(torch, B, k), _outputs(torch, B, k)
    stream = torch.cuda.Stream() if side_stream else None
    raw = stream.cuda_stream if side_stream else None
    torch.cuda.synchronize()  # uploads and poison are in place before anything runs on another stream
    za.merge_topk_device(0, S, B, k, t_ids.data_ptr(), t_keys.data_ptr(), t_counts.data_ptr(), plain[0][1].data_ptr(),
                         plain[1][1].data_ptr(), plain[2][GUARD:].data_ptr(), stream=raw)
    za.merge_topk_packed_device(0, S, B, k, g_packed.data_ptr(), packed[0][1].data_ptr(), packed[1][1].data_ptr(),
                                packed[2][GUARD:].data_ptr(), stream=raw)
    if side_stream:
        stream.synchronize()
    else:
        torch.cuda.synchronize()  # "the caller synchronises": nothing is read before this
    _check_outputs(plain, want, B, k, (tag, "zh_merge_topk_device"))
    _check_outputs(packed, want, B, k, (tag, "zh_merge_topk_packed_device"))
    for name, t, h in (("ids", t_ids, ids.view(np.int64)), ("keys", t_keys, keys.view(np.int64)),
                       ("counts", t_counts, counts.view(np.int32)), ("packed", g_packed, h_packed)):
        assert (t.cpu().numpy() == h).all(), (tag, "input written", name)
    return want


@pytest.mark.parametrize("family,S,k,B,seed", mc.device_cases())
def test_merge_equals_reference(za, family, S, k, B, seed):
    ids, keys, counts = mc.make_case(family, S, B, k, seed)
    run_merge(za, ids, keys, counts, k, tag=(family, S, k, B, seed))


@pytest.mark.parametrize("family,S,k,B", [("duplicates", 7, 100, 13), ("poisoned", 3, 342, 3), ("ties", 64, 1024, 3)])
def test_merge_on_a_stream_of_the_callers(za, family, S, k, B):
    """a non-default stream, synchronised alone before the results are read: one shape of each path"""
    ids, keys, counts = mc.make_case(family, S, B, k, 5)
    run_merge(za, ids, keys, counts, k, side_stream=True, tag=(family, S, k, B, "side stream"))


def test_eight_full_lists_of_1024(za):
    """(8, 1024) with all 8192 slots valid and sorted lists, as eight shards' full answers arrive: the streaming kernel's filter has
    six tiles to judge after the first two"""
    ids, keys, counts = mc.make_case("random", 8, 13, 1024, 1)
    assert (counts == 1024).all() and (np.diff(keys.astype(np.float64), axis=2) >= 0).all()
    want = run_merge(za, ids, keys, counts, 1024, tag="8 full lists")
    assert (want[2] == 1024).all()


def test_far_apart_duplicates_meet_in_different_tiles(za):
    """every query repeats every other entry of list s in list s + S/2, more than 1024 source slots later"""
    S, B, k = 64, 3, 1024
    for seed in (2, 3, 4):  # (b + seed) % 3 == 2 picks the far-apart variant: each seed puts it on another query
        ids, keys, counts = mc.make_case("duplicates", S, B, k, seed)
        b = (2 - seed) % 3
        assert (ids[S // 2:, b, ::2] == ids[:S // 2, b, ::2]).all()
        run_merge(za, ids, keys, counts, k, tag=("far duplicates", seed))


@settings(max_examples=40, deadline=None, derandomize=True)
@given(S=st.integers(1, 48), B=st.integers(1, 9), k=st.integers(1, 96), family=st.sampled_from(mc.FAMILIES),
       seed=st.integers(0, 2**31 - 1))
def test_device_merge_is_topk_of_union(S, B, k, family, seed):
    """the device twin of test_properties.test_merge_is_topk_of_union, on small shapes: S up to 48 and k up to 96, so most examples
    take the wave kernel and the streaming one sees at most four and a half tiles (S * k up to 4608); the parametrised cases
    above carry the large shapes"""
    import zebra_amd
    ids, keys, counts = mc.make_case(family, S, B, k, seed)
    run_merge(zebra_amd, ids, keys, counts, k, side_stream=bool(seed & 1), tag=(family, S, B, k, seed))


def test_an_empty_batch_is_accepted(za):
    """b = 0 launches nothing and needs no buffers"""
    from zebra_amd import _ffi
    L = _ffi.lib()
    assert L.zh_merge_topk_device(0, 4, 0, 10, None, None, None, None, None, None, None) == _ffi.ZH_OK
    assert L.zh_merge_topk_packed_device(0, 4, 0, 10, None, None, None, None, None) == _ffi.ZH_OK
    assert za.packed_result_words(0, 10) == 0

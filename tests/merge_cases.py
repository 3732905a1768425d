"""A plain reference of the shard merge and the inputs its tests feed (no GPU, no library: numpy only).

The device's two merge kernels (merge_wave_kernel and final_kernel<true>, zebra_amd/csrc/zh_search.hip) and the oracle's
zo_merge_topk state one contract, written down at zh_merge_topk_device in include/zebra_hip.h:

  per query, of the entries j < min(counts[s, b], k) of every list s, the k smallest DISTINCT (key, id) as unsigned 64-bit pairs;
  a repeated id is kept once; out_counts of them, every later output slot all-ones in ids and keys.

merge_reference restates that in a few lines of numpy; make_case draws the inputs, one family per way a merge can go wrong.
Every family is deterministic from its seed.

NOT FED, by any family: an entry inside `counts` whose key AND id are both 2**64 - 1.  That pair is the kernels' marker for an
invalid slot (what a search writes past its own count); the device drops it, the reference would keep it.  Keys and ids that are
all-ones on their own (never together) would be legitimate; the families stop at 2**64 - 2.
A repeated id always carries the same key, as it does in the library's own uses (one row, one distance)."""
import numpy as np

ONES = np.uint64(2**64 - 1)
FAMILIES = ("random", "ties", "ragged", "duplicates", "extremes", "poisoned", "counts_above_k")

# f64 bit patterns as keys: +inf and a quiet NaN of either sign (a key is the distance's bits; NaNs sort by their bits like the rest)
KEY_EXTREMES = np.array([0, 1, 2**64 - 2, 0x7FF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000], np.uint64)
ID_BASE_BIG = 1 << 40

# (S, k) from the thresholds of the code: MERGE_WAVE_N 1024 entries is where zh_launch_merge leaves the wave kernel, the streaming
# kernel sorts FIN_SORT_N 2048 entries fed in tiles of 1024, ZH_MAX_TOPK is 1024, the ABI admits 1..1024 shards
WAVE_SHAPES = ((1, 1), (1, 1024), (2, 512), (3, 341), (8, 128), (1024, 1), (7, 100), (64, 16))
BOUNDARY_SHAPES = ((3, 342), (5, 205), (1024, 2), (2, 513))                  # the first shapes with S * k > 1024
TILED_SHAPES = ((64, 1024), (1024, 64), (1024, 1024), (8, 1024))             # several tiles of valid entries
BATCHES = (1, 3, 13, 257)  # 3: odd, so the packed layout's counts section ends in a padding word


def shape_path(S, k):
    """the group of shapes above that (S, k) falls in.  The code has one switch: up to 1024 entries zh_launch_merge picks the wave
    kernel, past that the streaming one.  "boundary" and "tiled" are this module's own words for how much the streaming kernel
    then has to do: at most its first two tiles (one sort of FIN_SORT_N entries), or more tiles than that, filtered against the
    k-th best so far"""
    if S * k <= 1024:
        return "wave"
    return "boundary" if S * k <= 2048 else "tiled"


def merge_reference(ids, keys, counts, k):
    """ids, keys [S, B, k] u64, counts [S, B] u32 -> (out_ids [B, k], out_keys [B, k], out_counts [B])"""
    ids, keys, counts = np.asarray(ids, np.uint64), np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    S, B, width = ids.shape
    assert width == k and keys.shape == ids.shape and counts.shape == (S, B)
    out_ids, out_keys = np.full((B, k), ONES, np.uint64), np.full((B, k), ONES, np.uint64)
    out_counts = np.zeros(B, np.uint32)
    slot = np.arange(k)
    for b in range(B):
        valid = slot[None, :] < np.minimum(counts[:, b], k)[:, None]  # a count above k reads k slots
        qi, qk = ids[:, b, :][valid], keys[:, b, :][valid]
        order = np.lexsort((qi, qk))  # by key, then id, both unsigned
        qi, qk = qi[order], qk[order]
        first = np.ones(qi.size, bool)
        first[1:] = qi[1:] != qi[:-1]  # the first of each run of equal ids
        qi, qk = qi[first][:k], qk[first][:k]
        out_ids[b, :qi.size], out_keys[b, :qi.size], out_counts[b] = qi, qk, qi.size
    return out_ids, out_keys, out_counts


def merge_literal(ids, keys, counts, k):
    """the same in literal Python, for small cases: per query the list of (key, id) pairs, sorted(set(...))[:k]"""
    S, B, _ = ids.shape
    out = []
    for b in range(B):
        pool = set()
        for s in range(S):
            for j in range(min(int(counts[s, b]), k)):
                pool.add((int(keys[s, b, j]), int(ids[s, b, j])))
        out.append(sorted(pool)[:k])
    return out


def _distinct_ids(rng, S, B, k, base=0):
    return (rng.permutation(S * B * k).reshape(S, B, k) + base).astype(np.uint64)


def _blank_past_counts(ids, keys, counts):
    """what a search leaves past its count: all-ones"""
    k = ids.shape[2]
    past = np.arange(k)[None, None, :] >= counts[:, :, None]
    ids[past], keys[past] = ONES, ONES


def _sorted_order(ids, keys, counts, b):
    """(shard, slot) of query b's valid entries in (key, id) order"""
    k = ids.shape[2]
    s_idx, j_idx = np.nonzero(np.arange(k)[None, :] < np.minimum(counts[:, b], k)[:, None])
    order = np.lexsort((ids[s_idx, b, j_idx], keys[s_idx, b, j_idx]))
    return s_idx[order], j_idx[order]


def make_case(family, S, B, k, seed):
    """-> ids [S, B, k] u64, keys [S, B, k] u64, counts [S, B] u32"""
    rng = np.random.default_rng([FAMILIES.index(family), S, B, k, seed])
    full = np.full((S, B), k, np.uint32)

    if family == "random":  # distinct ids, random keys, every list sorted and full: what disjoint shards over random rows give
        ids = _distinct_ids(rng, S, B, k)
        keys = rng.integers(0, 2**64 - 1, (S, B, k), dtype=np.uint64)
        order = np.argsort(keys, axis=2, kind="stable")
        return np.take_along_axis(ids, order, 2), np.take_along_axis(keys, order, 2), full

    if family == "ties":  # 2-4 key values: the cut falls inside a run of equal keys across lists and the id decides
        values = np.array([7, 7 + 2**33, 2**52, 2**63 + 5], np.uint64)[:2 + seed % 3]
        ids = _distinct_ids(rng, S, B, k, base=seed % 2 * ID_BASE_BIG)
        keys = values[rng.integers(0, values.size, (S, B, k))]
        counts = np.where(rng.random((S, B)) < 0.8, k, rng.integers(0, k + 1, (S, B))).astype(np.uint32)
        _blank_past_counts(ids, keys, counts)
        return ids, keys, counts

    if family == "ragged":
        ids = _distinct_ids(rng, S, B, k)
        keys = rng.integers(0, 4 * S * k, (S, B, k)).astype(np.uint64)  # some ties as well
        edge = np.array([0, 1, k - 1, k], np.uint32)
        counts = np.zeros((S, B), np.uint32)
        for b in range(B):
            kind = (b + seed) % 4
            if kind == 0:  # every value of {0, 1, k-1, k}, in turn and then at random
                counts[:, b] = edge[rng.integers(0, 4, S)]
                counts[:4, b] = edge[(np.arange(min(S, 4)) + b) % 4]
            elif kind == 1:  # nothing at all: count 0 and a row of all-ones
                pass
            elif kind == 2:  # fewer than k together
                counts[:, b] = rng.integers(0, (k - 1) // S + 1, S)
            else:  # a single list holds anything
                counts[rng.integers(0, S), b] = rng.integers(1, k + 1)
        _blank_past_counts(ids, keys, counts)
        return ids, keys, counts

    if family == "duplicates":
        ids = _distinct_ids(rng, S, B, k, base=seed % 2 * ID_BASE_BIG)
        keys = rng.integers(0, 2**40, (S, B, k)).astype(np.uint64)
        counts = full.copy()
        for b in range(B):
            kind = (b + seed) % 3
            if kind == 0:  # every list is the same list: the result is that list
                c = k if (b + seed) % 2 else int(rng.integers(1, k + 1))
                ids[:, b, :], keys[:, b, :], counts[:, b] = ids[0, b, :], keys[0, b, :], c
            elif kind == 1:  # the entry that is the k-th best arrives once more, in the slot of the worst entry
                s_idx, j_idx = _sorted_order(ids, keys, counts, b)
                kth, last = min(k, s_idx.size) - 1, s_idx.size - 1
                if last > kth:
                    ids[s_idx[last], b, j_idx[last]] = ids[s_idx[kth], b, j_idx[kth]]
                    keys[s_idx[last], b, j_idx[last]] = keys[s_idx[kth], b, j_idx[kth]]
            else:  # list s + S/2 repeats every other entry of list s, S/2 * k source slots later: with S * k > 2048 the two
                #    copies reach the streaming kernel in different tiles
                h = S // 2
                if h:
                    ids[h:2 * h, b, ::2], keys[h:2 * h, b, ::2] = ids[:h, b, ::2], keys[:h, b, ::2]
                else:
                    ids[0, b, k // 2:], keys[0, b, k // 2:] = ids[0, b, :k - k // 2], keys[0, b, :k - k // 2]
        _blank_past_counts(ids, keys, counts)
        return ids, keys, counts

    if family == "extremes":  # keys at both ends of u64 and the bit patterns of inf / NaN; ids past 2**32 and at 2**64 - 2
        ids = _distinct_ids(rng, S, B, k, base=ID_BASE_BIG)
        keys = np.where(rng.random((S, B, k)) < 0.7, KEY_EXTREMES[rng.integers(0, KEY_EXTREMES.size, (S, B, k))],
                        rng.integers(0, 2**64 - 1, (S, B, k), dtype=np.uint64))
        counts = np.where(rng.random((S, B)) < 0.5, k, rng.integers(0, k + 1, (S, B))).astype(np.uint32)
        for b in range(B):  # the id 2**64 - 2 once per query, whatever its key, in a slot inside its list's count
            lists = np.nonzero(counts[:, b])[0]
            if lists.size:
                s = lists[rng.integers(0, lists.size)]
                ids[s, b, rng.integers(0, counts[s, b])] = np.uint64(2**64 - 2)
        _blank_past_counts(ids, keys, counts)
        return ids, keys, counts

    if family == "poisoned":  # past every count: keys below every valid key and plausible ids, where a search leaves all-ones
        ids = _distinct_ids(rng, S, B, k)
        keys = rng.integers(1000, 2**40, (S, B, k)).astype(np.uint64)
        counts = rng.integers(0, k + 1, (S, B)).astype(np.uint32)
        counts[rng.integers(0, S, B), np.arange(B)] = rng.integers(0, k, B)  # at least one short list per query
        past = np.arange(k)[None, None, :] >= counts[:, :, None]
        keys[past] = rng.integers(0, 10, int(past.sum())).astype(np.uint64)
        return ids, keys, counts

    if family == "counts_above_k":  # a list reporting k + 7 entries: k are read
        ids = _distinct_ids(rng, S, B, k)
        keys = rng.integers(0, 2**64 - 1, (S, B, k), dtype=np.uint64)
        counts = np.where(rng.random((S, B)) < 0.5, k + 7, rng.integers(0, k + 1, (S, B))).astype(np.uint32)
        counts[rng.integers(0, S, B), np.arange(B)] = k + 7
        past = np.arange(k)[None, None, :] >= counts[:, :, None]
        ids[past], keys[past] = ONES, ONES
        return ids, keys, counts

    raise ValueError(family)


# (family, S, k, B, seed) of the device tests: every family on shapes of all three groups above, every batch size on the wave and
# on the boundary shapes, not the cross product.  B stays at or below 3 at a million entries per query and at or below 13 above
# 2**15, so that no case holds more than ~100 MB.
DEVICE_CASES = (
    ('random', 1, 1, 1, 0), ('random', 3, 341, 3, 3), ('random', 7, 100, 13, 6), ('random', 3, 342, 1, 0),
    ('random', 1024, 2, 3, 2), ('random', 64, 1024, 1, 0), ('random', 1024, 1024, 3, 2),
    ('ties', 2, 512, 3, 13), ('ties', 1024, 1, 13, 16), ('ties', 5, 205, 3, 12), ('ties', 2, 513, 13, 14),
    ('ties', 1024, 64, 3, 12), ('ties', 8, 1024, 13, 14),
    ('ragged', 1, 1024, 13, 23), ('ragged', 8, 128, 257, 26), ('ragged', 64, 16, 1, 29), ('ragged', 3, 342, 13, 22),
    ('ragged', 1024, 2, 257, 24), ('ragged', 64, 1024, 13, 22), ('ragged', 1024, 1024, 3, 24),
    ('duplicates', 1, 1, 257, 33), ('duplicates', 3, 341, 1, 36), ('duplicates', 7, 100, 3, 39), ('duplicates', 5, 205, 257, 34),
    ('duplicates', 2, 513, 1, 36), ('duplicates', 1024, 64, 13, 34), ('duplicates', 8, 1024, 1, 36),
    ('extremes', 2, 512, 1, 46), ('extremes', 1024, 1, 3, 49), ('extremes', 3, 342, 1, 44), ('extremes', 1024, 2, 3, 46),
    ('extremes', 64, 1024, 1, 44), ('extremes', 1024, 1024, 3, 46),
    ('poisoned', 1, 1024, 3, 56), ('poisoned', 8, 128, 13, 59), ('poisoned', 64, 16, 257, 62), ('poisoned', 5, 205, 3, 56),
    ('poisoned', 2, 513, 13, 58), ('poisoned', 1024, 64, 3, 56), ('poisoned', 8, 1024, 13, 58),
    ('counts_above_k', 1, 1, 13, 66), ('counts_above_k', 3, 341, 257, 69), ('counts_above_k', 7, 100, 1, 72),
    ('counts_above_k', 3, 342, 13, 66), ('counts_above_k', 1024, 2, 257, 68), ('counts_above_k', 64, 1024, 13, 66),
    ('counts_above_k', 1024, 1024, 3, 68),
)


def device_cases():
    return list(DEVICE_CASES)

"""Index compaction (zh_index_compact, LSHIndex.compact): the live rows move down over the removed ones on the device, the forest's leaf ids
are renumbered, and the caller gets the old -> new id map.  The contract: a compacted index is indistinguishable from the uncompacted one under
that map, for every later call.  Every comparison is bit-exact on rows, ids, keys and counts.  A "twin" is a second index made by the same
calls of which only one is compacted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker)
from tests.test_gpu_approx import check  # noqa: E402
from tests.test_gpu_exact import all_metrics, check_exact  # noqa: E402

GONE = np.uint64(2**64 - 1)
BOUNCE = 256 << 20  # ZH_COMPACT_BOUNCE_BYTES


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def chunking(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("ZH_COMPACT_CHUNK_ROWS", raising=False)
    else:
        monkeypatch.setenv("ZH_COMPACT_CHUNK_ROWS", str(chunk))


def expected_map(alive, base=0):
    m = np.full(alive.size, GONE, np.uint64)
    m[alive] = np.uint64(base) + (np.cumsum(alive)[alive] - 1).astype(np.uint64)
    return m


def pattern(name, n, rng):
    """-> bool array: the rows that stay"""
    alive = np.ones(n, bool)
    if name == "random10":
        alive[rng.choice(n, n // 10, replace=False)] = False
    elif name == "random90":
        alive[rng.choice(n, n * 9 // 10, replace=False)] = False
    elif name == "row0":
        alive[0] = False
    elif name == "tail":
        alive[n - n // 7:] = False
    elif name == "hole":
        alive[n // 3:n // 3 + n // 4] = False
    elif name == "all":
        alive[:] = False
    else:
        raise ValueError(name)
    return alive


def check_info(info, alive, d, n):
    live = int(alive.sum())
    moved = int((np.flatnonzero(alive) != np.arange(live)).sum())
    assert info["rows_before"] == n and info["rows_after"] == live and info["rows_moved"] == moved, info
    # the bound the header states: the bounce buffer, 4 bytes per stored row of ranks, a bit per row, block sums
    assert info["scratch_bytes"] <= BOUNCE + 4.25 * n + 4096, info
    # every moved row is read once and written once, or twice each through the bounce buffer
    assert 2 * moved * d * 4 <= info["bytes_moved"] <= 4 * moved * d * 4, info
    assert info["capacity_rows"] >= n, info
    assert (info["ms"] > 0) == (live < n), info


def apply_map(new_ids, ids, counts, base):
    """a twin's answer in the compacted index's numbering"""
    out = ids.copy()
    for b in range(ids.shape[0]):
        c = int(counts[b])
        out[b, :c] = new_ids[(ids[b, :c] - np.uint64(base)).astype(np.int64)]
    return out


def mapped_forest(fa, new_ids, base=0):
    """a twin's forest with its leaf ids passed through the map (slots outside every leaf may name removed rows: they become 0)"""
    loc = np.where(new_ids == GONE, np.uint64(base), new_ids) - np.uint64(base)
    out = dict(fa)
    out["leaf_ids"] = loc[fa["leaf_ids"].astype(np.int64)].astype(np.uint32)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the moved bytes
@pytest.mark.parametrize("chunk", [1, 37, None])
@pytest.mark.parametrize("name", ["random10", "random90", "row0", "tail", "hole", "all"])
@pytest.mark.parametrize("d", [30, 33, 128, 768])
def test_moved_rows(za, monkeypatch, d, name, chunk):
    chunking(monkeypatch, chunk)
    n = 3001
    assert n % 37
    X = zo.synth_rows(n, d, seed=0x5EB2C000 + d)
    alive = pattern(name, n, np.random.default_rng(d))
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    gone = np.flatnonzero(~alive).astype(np.uint64)
    assert len(ix.remove(gone)) == len(gone)
    new_ids, info = ix.compact()
    live = int(alive.sum())
    assert len(ix) == live and ix.stored_rows() == live
    got = ix.read_rows(0, live)
    assert got.tobytes() == X[alive].tobytes()
    assert (new_ids == expected_map(alive)).all()
    check_info(info, alive, d, n)
    moved = info["rows_moved"]
    if name == "tail":
        assert moved == 0 and info["bytes_moved"] == 0
    if name == "row0":  # every row moves by one: every chunk of two rows or more overlaps itself (a chunk of one row lands wholly below itself)
        assert moved == n - 1 and info["bytes_moved"] == (2 if chunk == 1 else 4) * moved * d * 4
    if name == "hole" and chunk == 37:  # past the hole a chunk's destination ends before its source begins
        assert info["bytes_moved"] < 4 * moved * d * 4
    if name == "all":
        Q = zo.synth_queries(3, d, n)
        ids, keys, counts = ix.search_exact_batch(Q, 5, za.L2SquaredDistance())
        assert (counts == 0).all() and (ids == GONE).all() and (keys == GONE).all()
    ix.close()


def test_everything_removed_then_add(za, monkeypatch):
    """a built index emptied and compacted: searches find nothing, and a later add behaves as on the twin"""
    chunking(monkeypatch, None)
    n, d, M, T = 2000, 64, 32, 4
    X = zo.synth_rows(n + 500, d, seed=0x5EB2C100)
    Q = zo.synth_queries(8, d, n, seed_rows=0x5EB2C100)
    twins = [za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0) for _ in range(2)]
    for ix in twins:
        ix.add(X[:n])
        assert len(ix.remove(np.arange(n, dtype=np.uint64))) == n
    tw, cx = twins
    new_ids, info = cx.compact()
    assert (new_ids == GONE).all() and info["rows_after"] == 0 and cx.stored_rows() == 0 and len(cx) == 0
    for m in (za.L2SquaredDistance(), za.CosineDistance()):
        for got in (cx.search_batch(Q, 5, m), cx.search_exact_batch(Q, 5, m)):
            assert (got[2] == 0).all()
    ids_t, ids_c = tw.add(X[n:]), cx.add(X[n:])
    assert (ids_c == np.arange(500, dtype=np.uint64)).all() and (ids_t == ids_c + np.uint64(n)).all()
    ext = np.concatenate([new_ids, ids_c])
    assert zo.canonical_forest(cx.get_forest(), d) == zo.canonical_forest(mapped_forest(tw.get_forest(), ext), d)
    for m in (za.L2SquaredDistance(), za.CosineDistance()):
        a, b = tw.search_batch(Q, 10, m), cx.search_batch(Q, 10, m)
        assert (a[2] == b[2]).all() and (apply_map(ext, a[0], a[2], 0) == b[0]).all() and (a[1] == b[1]).all()
    for ix in twins:
        ix.close()


def test_table_larger_than_the_bounce_buffer(za, monkeypatch):
    """default chunking on 6 GB of rows: both paths, many chunks; a few thousand moved rows against the generator at their old ids"""
    chunking(monkeypatch, None)
    n, d = 2_000_000, 768
    assert n * d * 4 > 8 * BOUNCE
    rng = np.random.default_rng(11)
    alive = pattern("random10", n, rng)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    for r0 in range(0, n, 1 << 19):
        ix.append_synthetic(min(1 << 19, n - r0), first_row=r0)
    gone = np.flatnonzero(~alive).astype(np.uint64)
    assert len(ix.remove(gone)) == len(gone)
    new_ids, info = ix.compact()
    check_info(info, alive, d, n)
    moved = info["rows_moved"]
    assert 2 * moved * d * 4 < info["bytes_moved"] < 4 * moved * d * 4, info  # some chunks bounced, some went directly
    assert (new_ids == expected_map(alive)).all()
    old_of_new = np.flatnonzero(alive)
    live = old_of_new.size
    assert ix.stored_rows() == live
    # runs of 16 new rows: around every chunk boundary of the old numbering, at both ends, and at random
    chunk = BOUNCE // (d * 4)
    starts = [0, live - 16] + [int(np.searchsorted(old_of_new, a)) - 8 for a in range(chunk, n, chunk)] + rng.integers(0, live - 16, 150).tolist()
    checked = 0
    for s in starts:
        s = min(max(s, 0), live - 16)
        got = ix.read_rows(s, 16)
        want = np.concatenate([zo.synth_rows(1, d, row0=int(o)) for o in old_of_new[s:s + 16]])
        assert got.tobytes() == want.tobytes(), s
        checked += 16
    assert checked >= 2500
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------- 2. the map
def test_map_identity_and_arguments(za, monkeypatch):
    chunking(monkeypatch, 100)
    n, d, base = 5000, 256, (1 << 40) + 12345
    X = zo.synth_rows(n, d, seed=0x5EB2C200)
    Q = zo.synth_queries(4, d, n, seed_rows=0x5EB2C200)
    ix = za.LSHIndex(d, za.LSHIndexOptions(100, 4), device=0, id_base=base)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(Q, 10, za.L2SquaredDistance())  # makes the fp16 copy of the rows
    copy_before = ix.stats()["row_copy_bytes"]
    assert copy_before > 0
    # nothing removed: the identity, nothing released, nothing moved
    new_ids, info = ix.compact()
    assert (new_ids == np.uint64(base) + np.arange(n, dtype=np.uint64)).all()
    assert info["rows_moved"] == 0 and info["bytes_moved"] == 0 and info["copy_bytes_released"] == 0 and info["scratch_bytes"] == 0 and info["ms"] == 0
    assert ix.stats()["row_copy_bytes"] == copy_before
    alive = pattern("random10", n, np.random.default_rng(2))
    gone = np.flatnonzero(~alive).astype(np.uint64) + np.uint64(base)
    assert len(ix.remove(gone)) == len(gone)
    count = len(ix)
    # a map too short for the stored rows is refused, and nothing happens
    from zebra_amd import _ffi
    short = np.empty(n - 1, np.uint64)
    rc = _ffi.lib().zh_index_compact(ix._h, short.ctypes.data_as(C.c_void_p), n - 1, None)
    assert rc == _ffi.ZH_EINVAL and ix.stored_rows() == n
    new_ids, info = ix.compact()
    assert (new_ids == expected_map(alive, base)).all()
    assert len(ix) == count == int(alive.sum()) and ix.stored_rows() == count
    assert info["copy_bytes_released"] == copy_before and ix.stats()["row_copy_bytes"] == 0
    check_info(info, alive, d, n)
    # again: the identity over the live rows
    again, info2 = ix.compact()
    assert (again == np.uint64(base) + np.arange(count, dtype=np.uint64)).all() and info2["rows_moved"] == 0 and info2["rows_before"] == count
    # NULL map and NULL info are allowed
    ix.remove(np.array([base + 5], np.uint64))
    assert _ffi.lib().zh_index_compact(ix._h, None, 0, None) == _ffi.ZH_OK and ix.stored_rows() == count - 1
    ix.close()


def test_forest_with_a_row_listed_twice_is_refused(za):
    """remove drops one occurrence per tree, so such an injected forest may still list a removed row: compaction says so and changes nothing"""
    from zebra_amd import _ffi
    n, d = 64, 16
    X = zo.synth_rows(n, d, seed=0x5EB2C250)
    ix = za.LSHIndex(d, za.LSHIndexOptions(128, 1), device=0)
    ix.append(X)
    ids = np.concatenate([np.arange(n), [5]]).astype(np.uint32)  # one leaf, row 5 twice
    ix.set_forest(dict(plane=[-1], left=[0], right=[n + 1], roots=[0], planes=np.zeros((0, d), np.float32), consts=np.zeros(0, np.float32), leaf_ids=ids))
    ix.remove(np.array([5, 9], np.uint64))
    with pytest.raises(za.ZhError) as e:
        ix.compact()
    assert e.value.code == _ffi.ZH_EUNSUPPORTED and ix.stored_rows() == n and len(ix) == n - 2
    assert ix.read_rows(0, n).tobytes() == X.tobytes()
    ix.build()  # a forest of its own: compacts
    new_ids, info = ix.compact()
    assert info["rows_after"] == n - 2 and new_ids[5] == GONE and new_ids[10] == 8
    ix.close()


# ------------------------------------------------------------------------------------------------------------------- 3. the forest
def five_metrics(za):
    return all_metrics(za)[:4] + [(za.ManhattanDistance(), zo.MANHATTAN, 0)]


def twin_pair(za, X, M, T, gone, **kw):
    out = []
    for _ in range(2):
        ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(M, T), device=0, **kw)
        ix.add(X)
        assert len(ix.remove(gone + np.uint64(kw.get("id_base", 0)))) == len(gone)
        out.append(ix)
    return out


@pytest.mark.parametrize("chunk", [53, None])
def test_forest_and_search_modes(za, monkeypatch, chunk):
    chunking(monkeypatch, chunk)
    n, d, M, T, B, k = 9000, 256, 100, 6, 24, 10
    X = zo.synth_rows(n, d, seed=0x5EB2C300)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C300)
    rng = np.random.default_rng(5)
    alive = pattern("random10", n, rng)
    alive[[zo.synth_query_row(b, n) for b in range(0, B, 3)]] = False  # some planted neighbours go too
    gone = np.flatnonzero(~alive).astype(np.uint64)
    tw, cx = twin_pair(za, X, M, T, gone)
    for mode in ("approx", "leaf"):  # derived copies and tables exist before the compaction
        cx.set_sweep_mode(mode)
        cx.search_batch(Q, k, za.L2SquaredDistance())
    new_ids, info = cx.compact()
    check_info(info, alive, d, n)
    fa = cx.get_forest()
    assert zo.canonical_forest(fa, d) == zo.canonical_forest(mapped_forest(tw.get_forest(), new_ids), d)
    f = zo.Forest.from_arrays(X[alive], M, fa)
    for mode in ("leaf", "scan", "approx"):
        cx.set_sweep_mode(mode)
        for m, om, omode in five_metrics(za):
            st = check(cx, f, Q, k, m, om, omode, mode)
            if mode == "approx" and om in (zo.L2SQ, zo.L2, zo.COSINE):
                assert st["approx_scan"] == 2, st  # the matrix-core scan, on an fp16 copy made at the new size
                tiles = (int(alive.sum()) + 15) // 16
                assert tiles * 16 * (2 * d + 8) <= st["row_copy_bytes"], st
        # ... and the twin's answers, under the map
        tw.set_sweep_mode(mode)
        for m, om, omode in five_metrics(za)[:2]:
            a, b = tw.search_batch(Q, k, m), cx.search_batch(Q, k, m)
            assert (a[2] == b[2]).all() and (apply_map(new_ids, a[0], a[2], 0) == b[0]).all() and (a[1] == b[1]).all()
    tw.close()
    cx.close()


@pytest.mark.parametrize("kind", [1, 0])
def test_forest_d128_leaf_half(za, monkeypatch, kind):
    """d = 128 leaf by leaf at half width: the copy of bytes (kind 1: integer rows 0 .. 255) and the copy of halves are re-made at the new size"""
    chunking(monkeypatch, None)
    n, d, M, T, B, k = 9000, 128, 300, 6, 32, 10
    X = zo.synth_rows(n, d, seed=0x5EB2C400 + kind, kind=kind)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C400 + kind, kind=kind)
    alive = pattern("random10", n, np.random.default_rng(6 + kind))
    gone = np.flatnonzero(~alive).astype(np.uint64)
    tw, cx = twin_pair(za, X, M, T, gone)
    cx.set_sweep_mode("leaf-half")
    cx.search_batch(Q, k, za.L2SquaredDistance())
    before = cx.stats()
    assert before["approx_scan"] == 3 and before["approx_byte_rows"] == kind and before["row_copy_bytes"] >= n * (128 if kind else 256), before
    new_ids, info = cx.compact()
    assert info["copy_bytes_released"] == before["row_copy_bytes"]
    fa = cx.get_forest()
    assert zo.canonical_forest(fa, d) == zo.canonical_forest(mapped_forest(tw.get_forest(), new_ids), d)
    f = zo.Forest.from_arrays(X[alive], M, fa)
    live = int(alive.sum())
    for m, om, omode in five_metrics(za):
        st = check(cx, f, Q, k, m, om, omode, "leaf-half")
        if om in (zo.L2SQ, zo.L2, zo.COSINE):
            assert st["approx_scan"] == 3 and st["approx_byte_rows"] == kind, st
            assert live * (128 if kind else 256) <= st["row_copy_bytes"] < n * (128 if kind else 256), st
    tw.close()
    cx.close()


def small_leaf_lifecycle(za, seed):
    """The small-leaf regime's views -- row norms, per-plane norms, leaf meta, the blocked walk view -- are built, then the rows under them are
    removed, moved (compact) and replaced (clear + a refill to the same count).  After every search: the oracle on the index's own forest, and a
    twin that never held the views (built fresh over the same stored rows, the same forest injected: no sample rows, so no row scores, no norms,
    no leaf meta, and a first batch, so no blocked view).  -> (hash_from_scores, prefiltered) of every search, in order"""
    n, d, M, T, B, k = 3000, 64, 5, 4, 24, 10
    m = za.L2SquaredDistance()
    X = zo.synth_rows(n, d, seed=0x5EB2CC00)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2CC00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)  # (a forest of the library's own: the planes' sample rows are known)
    ix.set_hash_mode("scores")
    seen = []

    def search(rows, queries, what):
        fa = ix.get_forest()
        ids, keys, counts = ix.search_batch(queries, k, m)
        st = ix.stats()
        seen.append((int(st["hash_from_scores"]), int(st["prefiltered"])))
        tw = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
        tw.append(rows)
        tw.set_forest(fa)
        ti, tk, tc = tw.search_batch(queries, k, m)
        tw.close()
        oi, ok, oc = zo.Forest.from_arrays(rows, M, fa).search_batch(queries, k, zo.L2SQ, 0)
        assert (counts == oc).all() and (counts == tc).all(), what
        for b in range(B):
            c = int(oc[b])
            assert (ids[b, :c] == oi[b, :c]).all() and (keys[b, :c] == ok[b, :c]).all(), (what, "oracle", b)
            assert (ids[b, :c] == ti[b, :c]).all() and (keys[b, :c] == tk[b, :c]).all(), (what, "twin", b)

    for it in range(4):  # (the blocked view is built from the third batch on; the prefilter needs the norms and the leaf meta)
        search(X, Q, ("built", it))
    alive = pattern("random10", n, np.random.default_rng(seed))
    gone = np.flatnonzero(~alive).astype(np.uint64)
    assert len(ix.remove(gone)) == len(gone)
    search(X, Q, "removed")  # (the removed rows are still stored; no leaf lists them)
    new_ids, info = ix.compact()
    assert (new_ids == expected_map(alive)).all() and info["rows_after"] == int(alive.sum())
    for it in range(4):
        search(X[alive], Q, ("compacted", it))
    ix.clear()
    X2 = zo.synth_rows(n, d, seed=0x5EB2CC01)  # different rows, the same count
    assert X2.tobytes() != X.tobytes()
    ix.add(X2)
    Q2 = zo.synth_queries(B, d, n, seed_rows=0x5EB2CC01)
    for it in range(4):
        search(X2, Q2, ("refilled", it))
    ix.close()
    return seen


# (hash_from_scores, prefiltered) of the thirteen searches as the library reported them before the index's derived views were gathered into one
# record each: four on the built index, one after the removal, four after the compaction, four after clear + refill.  After the compaction the
# value depends on whether some plane's sample row was among the removed rows (then the index has no row scores until its forest is rebuilt).
# At this shape the ~4,800 planes name most of the 3,000 rows as samples: removal seeds 0 .. 5 all lose one, so that is the one case listed.
SMALL_LEAF_SEEN = {
    0: [(1, 1)] * 5 + [(0, 0)] * 4 + [(1, 1)] * 4,
}


@pytest.mark.parametrize("seed", sorted(SMALL_LEAF_SEEN))
@pytest.mark.parametrize("view", [None, "inner"])
def test_small_leaf_views_across_compact_and_refill(za, monkeypatch, view, seed):
    chunking(monkeypatch, None)
    if view:
        monkeypatch.setenv("ZH_WALK_BLOCKS", view)
    else:
        monkeypatch.delenv("ZH_WALK_BLOCKS", raising=False)
    seen = small_leaf_lifecycle(za, seed)
    print("small-leaf lifecycle, view %s seed %d: %s" % (view, seed, seen))
    assert seen == SMALL_LEAF_SEEN[seed]


# ------------------------------------------------------------------------------------------------------------------ 4. exact search
def test_exact_all_metrics_after_compaction(za, monkeypatch):
    chunking(monkeypatch, 64)
    n, d = 4000, 100
    X = zo.synth_rows(n, d, seed=0x5EB2C500)
    Q = zo.synth_queries(3, d, n, seed_rows=0x5EB2C500)
    alive = pattern("random10", n, np.random.default_rng(8))
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0, id_base=77)
    ix.append(X)
    ix.remove(np.flatnonzero(~alive).astype(np.uint64) + np.uint64(77))
    ix.search_exact_batch(Q, 10, za.L2SquaredDistance())  # the live-row list of the uncompacted table exists
    ix.compact()
    for m, om, omode in all_metrics(za):
        check_exact(ix.search_exact_batch(Q, 100, m), X[alive], Q, 100, om, omode, id_base=77)
        assert ix.exact_info()["path"] == 1 and ix.exact_info()["rows_live"] == int(alive.sum())
    ix.close()


@pytest.mark.parametrize("d", [512, 768])
def test_exact_path2_after_compaction(za, monkeypatch, d):
    chunking(monkeypatch, None)
    monkeypatch.delenv("ZH_ROW_HALF_META_ONLY", raising=False)
    n, B, k = 14000, 8, 100
    X = zo.synth_rows(n, d, seed=0x5EB2C600 + d)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C600 + d)
    alive = pattern("random10", n, np.random.default_rng(d))
    alive[[zo.synth_query_row(b, n) for b in range(0, B, 2)]] = False
    live = int(alive.sum())
    assert live >= 8192
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    ix.remove(np.flatnonzero(~alive).astype(np.uint64))
    m0 = za.L2SquaredDistance()
    check_exact(ix.search_exact_batch(Q, k, m0), X[alive], Q, k, zo.L2SQ, 0, ids_of=np.flatnonzero(alive))
    assert ix.exact_info()["path"] == 2
    before = ix.stats()["row_copy_bytes"]
    assert before >= n * (2 * d + 8)
    new_ids, info = ix.compact()
    assert info["copy_bytes_released"] == before and ix.stats()["row_copy_bytes"] == 0
    for m, om, omode in all_metrics(za)[:4]:
        check_exact(ix.search_exact_batch(Q, k, m), X[alive], Q, k, om, omode)
        ei = ix.exact_info()
        assert ei["path"] == 2 and ei["redone"] == 0 and ei["rows_live"] == live, ei
        # the fp16 copy at the new size: whole tiles of 16 rows, 2 d + 8 bytes per row, each of the two buffers rounded up to 256 bytes
        tiles = (live + 15) // 16
        assert tiles * 16 * (2 * d + 8) <= ix.stats()["row_copy_bytes"] <= tiles * 16 * (2 * d + 8) + 512
    ix.close()


# ------------------------------------------------------------------------------------------------- 5. twins across later mutations
def same_answers(za, tw, cx, ext, Q, k, base_t=0):
    for m, om, omode in five_metrics(za):
        a, b = tw.search_batch(Q, k, m), cx.search_batch(Q, k, m)
        assert (a[2] == b[2]).all() and (apply_map(ext, a[0], a[2], base_t) == b[0]).all() and (a[1] == b[1]).all(), ("lsh", om, omode)
    for m, om, omode in all_metrics(za)[:4]:
        a, b = tw.search_exact_batch(Q, k, m), cx.search_exact_batch(Q, k, m)
        assert (a[2] == b[2]).all() and (apply_map(ext, a[0], a[2], base_t) == b[0]).all() and (a[1] == b[1]).all(), ("exact", om, omode)


def same_forest(tw, cx, ext, d, base_t=0):
    assert zo.canonical_forest(cx.get_forest(), d) == zo.canonical_forest(mapped_forest(tw.get_forest(), ext, 0), d)


@pytest.mark.parametrize("chunk", [41, None])
def test_twins_across_mutations(za, monkeypatch, chunk):
    """add, remove, deduplicate and build after the compaction: forests and answers stay equal under the (extended) map"""
    chunking(monkeypatch, chunk)
    n, n2, d, M, T, B, k = 6000, 1500, 96, 48, 5, 16, 10
    X = zo.synth_rows(n + n2, d, seed=0x5EB2C700)
    X[n + 100:n + 140] = X[17]        # duplicates of a live row, added later
    X[n + 200:n + 210] = X[n + 150]   # ... and among the added rows
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C700)
    rng = np.random.default_rng(9)
    alive = pattern("random10", n, rng)
    alive[[0, 1, 2]] = False
    alive[17] = True
    gone = np.flatnonzero(~alive).astype(np.uint64)
    tw, cx = twin_pair(za, X[:n], M, T, gone)
    new_ids, info = cx.compact()
    check_info(info, alive, d, n)
    same_forest(tw, cx, new_ids, d)
    same_answers(za, tw, cx, new_ids, Q, k)
    # add(more): the twin numbers them from n, the compacted index from its live count
    ids_t, ids_c = tw.add(X[n:]), cx.add(X[n:])
    assert (ids_t == np.arange(n, n + n2, dtype=np.uint64)).all() and (ids_c == np.arange(n2, dtype=np.uint64) + np.uint64(alive.sum())).all()
    ext = np.concatenate([new_ids, ids_c])
    same_forest(tw, cx, ext, d)
    same_answers(za, tw, cx, ext, Q, k)
    # remove(ids), each twin in its own numbering
    live_t = np.flatnonzero(ext != GONE)
    rm = rng.choice(live_t, 700, replace=False).astype(np.uint64)
    rm = rm[rm != 17]
    rt, rc = tw.remove(rm), cx.remove(ext[rm.astype(np.int64)])
    assert len(rt) == len(rm) and (ext[rt.astype(np.int64)] == rc).all()
    same_forest(tw, cx, ext, d)
    same_answers(za, tw, cx, ext, Q, k)
    # deduplicate
    dt, dc = tw.deduplicate(), cx.deduplicate()
    assert len(dt) >= 40 and (ext[dt.astype(np.int64)] == dc).all()
    same_forest(tw, cx, ext, d)
    same_answers(za, tw, cx, ext, Q, k)
    # build: both rebuild over their live rows; then the compacted one alone, compacted again, against the oracle's build of the live rows
    tw.build()
    cx.build()
    same_forest(tw, cx, ext, d)
    same_answers(za, tw, cx, ext, Q, k)
    alive_t = np.ones(n + n2, bool)
    alive_t[gone.astype(np.int64)] = False
    alive_t[rt.astype(np.int64)] = False
    alive_t[dt.astype(np.int64)] = False
    m2, _ = cx.compact()
    assert len(cx) == int(alive_t.sum()) == cx.stored_rows()
    rows_now = X[alive_t]
    assert cx.read_rows(0, len(cx)).tobytes() == rows_now.tobytes()
    cx.build()
    fo = zo.Forest.build(rows_now, M, T)
    assert zo.canonical_forest(cx.get_forest(), d) == zo.canonical_forest(fo.arrays(), d)
    for m, om, omode in five_metrics(za):
        check(cx, fo, Q, k, m, om, omode, "rebuilt")
    tw.close()
    cx.close()


def test_compaction_interleaved_twice(za, monkeypatch):
    """remove -> compact -> add -> remove -> compact -> add -> search, against a twin that is never compacted; maps compose"""
    chunking(monkeypatch, 29)
    n, a1, a2, d, M, T, B, k, base = 5000, 1200, 900, 64, 40, 5, 16, 10, 1 << 33
    X = zo.synth_rows(n + a1 + a2, d, seed=0x5EB2C800)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C800)
    rng = np.random.default_rng(10)
    tw = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=base)
    cx = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=base)
    tw.add(X[:n])
    cx.add(X[:n])
    ext = np.uint64(base) + np.arange(n, dtype=np.uint64)  # twin local row -> id in the compacted index
    lo = n
    for more in (a1, a2):
        live_t = np.flatnonzero(ext != GONE)
        rm = np.unique(np.concatenate([rng.choice(live_t, len(live_t) // 8, replace=False), live_t[:3]]))
        rt, rc = tw.remove(rm.astype(np.uint64) + np.uint64(base)), cx.remove(ext[rm])
        assert len(rt) == len(rm) == len(rc)
        ext[rm] = GONE
        m, info = cx.compact()  # old id in cx -> new id in cx
        assert info["rows_after"] == int((ext != GONE).sum()) and info["rows_moved"] > 0
        keep = ext != GONE
        ext[keep] = m[(ext[keep] - np.uint64(base)).astype(np.int64)]
        assert (ext[keep] == np.uint64(base) + np.arange(keep.sum(), dtype=np.uint64)).all()  # stable: the twin's order
        ids_t, ids_c = tw.add(X[lo:lo + more]), cx.add(X[lo:lo + more])
        assert (ids_t == np.uint64(base) + np.arange(lo, lo + more, dtype=np.uint64)).all()
        ext = np.concatenate([ext, ids_c])
        lo += more
        assert zo.canonical_forest(cx.get_forest(), d) == zo.canonical_forest(mapped_forest(tw.get_forest(), ext, base), d)
        same_answers(za, tw, cx, ext, Q, k, base_t=base)
    tw.close()
    cx.close()


# ------------------------------------------------------------------------------------------------------------ 6. a never-built index
def test_never_built_index(za, monkeypatch):
    chunking(monkeypatch, 500)
    n, d, M, T, B, k = 7000, 48, 64, 5, 8, 50
    X = zo.synth_rows(n, d, seed=0x5EB2C900)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2C900)
    alive = pattern("random10", n, np.random.default_rng(12))
    alive[:40] = False
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.append(X)
    ix.remove(np.flatnonzero(~alive).astype(np.uint64))
    new_ids, info = ix.compact()
    assert ix.no_trees() and (new_ids == expected_map(alive)).all()
    check_info(info, alive, d, n)
    for m, om, omode in all_metrics(za)[:5]:
        check_exact(ix.search_exact_batch(Q, k, m), X[alive], Q, k, om, omode)
    ix.build()
    fo = zo.Forest.build(X[alive], M, T)
    assert zo.canonical_forest(ix.get_forest(), d) == zo.canonical_forest(fo.arrays(), d)
    for m, om, omode in five_metrics(za):
        check(ix, fo, Q, 10, m, om, omode, "built after compaction")
    ix.close()


# ---------------------------------------------------------------------------------------------------- 7. contexts and the Database
def test_search_context_survives(za, monkeypatch):
    import torch
    chunking(monkeypatch, None)
    n, d, M, T, B, k = 8000, 128, 64, 6, 32, 10
    X = zo.synth_rows(n, d, seed=0x5EB2CA00)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2CA00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.zeros((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.zeros_like(ids), torch.zeros(B, dtype=torch.int32, device=dev)
    m = za.L2SquaredDistance()
    ctx = ix.search_context()

    def run():
        ctx.begin(dq.data_ptr(), B, k, m)
        ctx.finish(ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
        ctx.wait()
        torch.cuda.synchronize()
        return ids.cpu().numpy().view(np.uint64).copy(), keys.cpu().numpy().view(np.uint64).copy(), counts.cpu().numpy().view(np.uint32).copy()

    before = run()
    want = ix.search_batch(Q, k, m)
    assert (before[0] == want[0]).all() and (before[2] == want[2]).all()
    alive = pattern("random10", n, np.random.default_rng(13))
    ix.remove(np.flatnonzero(~alive).astype(np.uint64))
    new_ids, _ = ix.compact()
    got = run()
    want = ix.search_batch(Q, k, m)
    for b in range(B):
        c = int(want[2][b])
        assert got[2][b] == c and (got[0][b, :c] == want[0][b, :c]).all() and (got[1][b, :c] == want[1][b, :c]).all()
    f = zo.Forest.from_arrays(X[alive], M, ix.get_forest())
    check(ix, f, Q, k, m, zo.L2SQ, 0, "after compaction")
    ctx.close()
    ix.close()


def test_database_compact(za, monkeypatch):
    chunking(monkeypatch, None)
    n, d, B = 3000, 32, 12
    X = zo.synth_rows(n, d, seed=0x5EB2CB00)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2CB00)
    db = za.Database(d, za.L2SquaredDistance, za.LSHIndexOptions(32, 5), device=0, id_base=1000)
    db.insert_records(X, ["doc %d" % i for i in range(n)])
    db.remove(np.arange(1000, 1000 + n, 3, dtype=np.uint64))
    before = db.query_vectors(Q, 7)
    info = db.compact()
    assert info["rows_after"] == n - (n + 2) // 3 == len(db.index) and len(db._documents) == len(db.index)
    after = db.query_vectors(Q, 7)
    for b in range(B):
        assert sorted(before[b].values()) == sorted(after[b].values()) and len(after[b]) == len(before[b]) > 0
        assert None not in after[b].values()
    db.insert_records(X[:5] + np.float32(1), ["new %d" % i for i in range(5)])
    assert len(db._documents) == len(db.index)
    db.index.close()

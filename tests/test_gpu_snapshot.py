"""Index snapshots (zh_index_save / zh_index_load, LSHIndex.save / LSHIndex.load).  The contract: a loaded index is indistinguishable from the
saved one for every later call -- rows, counts, forest, signs, ids / keys / counts of every search, the path a batch takes where that depends on
index state, and the effect of every later mutation.  A "twin" pair is an index and what a save + load made of it; every comparison is bit-exact.
The file format is checked both ways against the numpy writer / reader of tests/test_snapshot_format.py (written from DESIGN.md s12)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker)
from tests import test_snapshot_format as fmt  # noqa: E402
from tests.test_gpu_approx import check  # noqa: E402
from tests.test_gpu_exact import all_metrics  # noqa: E402

GONE = np.uint64(2**64 - 1)
STAT_FIELDS = ("hash_from_scores", "prefiltered", "table_scan", "approx_scan")


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


@pytest.fixture(autouse=True)
def default_chunks(monkeypatch):
    monkeypatch.delenv("ZH_SNAPSHOT_CHUNK_BYTES", raising=False)


def five_metrics(za):
    """L2^2, L2, both cosine keys and one metric of the `distances` crate"""
    return all_metrics(za)[:4] + [(za.ManhattanDistance(), zo.MANHATTAN, 0)]


def roundtrip(za, ix, tmp_path, name="snap.zhs", **kw):
    p = str(tmp_path / name)
    info = ix.save(p)
    assert info["verified"] == 1 and info["file_bytes"] == os.path.getsize(p) and not os.path.exists(p + ".zhtmp")
    assert info["stored_rows"] == ix.stored_rows() and info["live_rows"] == len(ix) and info["row_bytes"] == ix.stored_rows() * ix.dim * 4
    # the host's reader agrees with the checksums the device computed
    seen = za.snapshot_info(p, verify=True)
    assert seen["verified"] == 1 and all(seen[k] == info[k] for k in seen if k not in ("ms", "ms_device", "verified"))
    ld = za.LSHIndex.load(p, device=0, **kw)
    assert all(ld.snapshot[k] == info[k] for k in info if k not in ("ms", "ms_device"))
    return ld, p, info


def same_state(a, b):
    from zebra_amd import _ffi
    d = a.dim
    assert b.dim == d and b.id_base == a.id_base and b.options == a.options
    L = _ffi.lib()
    for fn in (L.zh_index_count, L.zh_index_stored_rows, L.zh_index_num_trees, L.zh_index_dim, L.zh_index_id_base):
        assert fn(a._h) == fn(b._h), fn
    n = a.stored_rows()
    assert a.read_rows(0, n).tobytes() == b.read_rows(0, n).tobytes()
    fa, fb = a.get_forest(), b.get_forest()
    for k in fa:  # the arrays themselves (the planes keep their numbering), and as canonical_forest compares forests
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert zo.canonical_forest(fa, d) == zo.canonical_forest(fb, d)


def same_answers(za, a, b, Q, k, stats=True, exact=True):
    """one batch per metric on both; with stats: the path it took is the same as well (only where both have the same search history)"""
    if a.get_forest()["roots"].size:
        assert (a.hash_signs(Q) == b.hash_signs(Q)).all()
        for m, om, omode in five_metrics(za):
            ra, rb = a.search_batch(Q, k, m), b.search_batch(Q, k, m)
            sa, sb = a.stats(), b.stats()
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes(), ("lsh", om, omode)
            if stats:
                assert [sa[f] for f in STAT_FIELDS] == [sb[f] for f in STAT_FIELDS], (om, omode, sa, sb)
    if exact:
        for m, om, omode in all_metrics(za)[:4]:
            ra, rb = a.search_exact_batch(Q, k, m), b.search_exact_batch(Q, k, m)
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes(), ("exact", om, omode)
            assert a.exact_info()["path"] == b.exact_info()["path"]


# --------------------------------------------------------------------------------------------------------------------- 1. index states
def test_empty_index(za, tmp_path):
    ix = za.LSHIndex(8, za.LSHIndexOptions(7, 3), device=0, id_base=5, seed=77)
    ld, p, info = roundtrip(za, ix, tmp_path)
    assert info["stored_rows"] == 0 and info["n_trees"] == 0 and info["flags"] == 0 and info["file_bytes"] == fmt.BLOCK  # a header block, ten empty sections
    same_state(ix, ld)
    assert ld.no_vectors() and ld.no_trees() and ld.snapshot["seed"] == 77
    X = zo.synth_rows(300, 8, seed=0x5EB2D100)
    Q = zo.synth_queries(4, 8, 300, seed_rows=0x5EB2D100)
    assert (ix.add(X) == ld.add(X)).all()  # the first add builds: same seed, same forest
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, 5)
    ix.close()
    ld.close()


def test_appended_never_built(za, tmp_path):
    n, d = 2001, 30
    X = zo.synth_rows(n, d, seed=0x5EB2D200)
    Q = zo.synth_queries(5, d, n, seed_rows=0x5EB2D200)
    ix = za.LSHIndex(d, za.LSHIndexOptions(40, 4), device=0, id_base=1 << 35)
    ix.append(X)
    ix.remove(np.array([3, 1999], np.uint64) + np.uint64(1 << 35))  # removed without trees: only the tombstones say so
    ld, p, info = roundtrip(za, ix, tmp_path)
    assert info["n_trees"] == 0 and info["live_rows"] == n - 2
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, 10)
    ix.build()
    ld.build()
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, 10)
    ix.close()
    ld.close()


def test_built_d128_integer_rows(za, tmp_path):
    """the byte copy of an integer table is derived data: not in the file, re-made by the loaded index's first half-width batch"""
    n, d, M, T, B, k = 9000, 128, 300, 6, 32, 10
    X = zo.synth_rows(n, d, seed=0x5EB2D300, kind=1)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D300, kind=1)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)
    ld, p, info = roundtrip(za, ix, tmp_path)
    assert info["flags"] == 1 and info["file_bytes"] < n * d * 4 + T * n * 4 + (1 << 20)  # no derived copy in the file
    same_state(ix, ld)
    assert ld.stats()["row_copy_bytes"] == 0
    for t in (ix, ld):
        t.set_sweep_mode("leaf-half")
    same_answers(za, ix, ld, Q, k)
    st = ld.stats(), ix.stats()
    assert st[0]["row_copy_bytes"] == st[1]["row_copy_bytes"] >= n * 128
    ld.search_batch(Q, k, za.L2SquaredDistance())
    assert ld.stats()["approx_scan"] == 3 and ld.stats()["approx_byte_rows"] == 1
    # against the CPU checker directly, not only against the twin
    f = zo.Forest.from_arrays(X, M, ld.get_forest())
    for m, om, omode in five_metrics(za):
        check(ld, f, Q, k, m, om, omode, "loaded")
    ix.close()
    ld.close()


def test_grown_by_adds_d768(za, tmp_path):
    n, d, M, T, B, k = 6000, 768, 64, 5, 16, 10
    X = zo.synth_rows(n, d, seed=0x5EB2D400)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D400)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    for a, b in ((0, 2000), (2000, 2007), (2007, 4500), (4500, n)):
        ix.add(X[a:b])
    ld, p, info = roundtrip(za, ix, tmp_path, reserve_rows=2 * n)
    assert info["flags"] == 1 and info["n_leaf_ids"] >= T * n
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, k)
    f = zo.Forest.from_arrays(X, M, ld.get_forest())
    for m, om, omode in five_metrics(za)[:2]:
        check(ld, f, Q, k, m, om, omode, "loaded, grown")
    ix.close()
    ld.close()


def test_tombstones_d30(za, tmp_path):
    n, d, M, T, B, k, base = 5000, 30, 24, 5, 12, 10, 9_000_000_000
    X = zo.synth_rows(n, d, seed=0x5EB2D500)
    X[4000:4040] = X[11]
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D500)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=base)
    ix.add(X)
    gone = np.random.default_rng(1).choice(n, 600, replace=False).astype(np.uint64)
    gone = gone[gone != 11]
    assert len(ix.remove(gone + np.uint64(base))) == len(gone)
    assert len(ix.deduplicate()) >= 30
    ld, p, info = roundtrip(za, ix, tmp_path)
    assert info["live_rows"] == len(ix) < n == info["stored_rows"]
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, k)
    # the removals came back: removing them again finds nothing, on both
    again = gone[:50] + np.uint64(base)
    assert len(ix.remove(again)) == 0 and len(ld.remove(again)) == 0
    ix.close()
    ld.close()


def test_row_score_hash_survives_d384(za, tmp_path):
    """the reference-default regime (max_node_size 5): the planes' sample rows are in the file, so the row-score hash and the prefilter still
    serve the loaded index -- which get_forest + set_forest cannot restore"""
    n, d, M, T, B, k = 12000, 384, 5, 4, 16, 10
    X = zo.synth_rows(n, d, seed=0x5EB2D600)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D600)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)
    ld, p, info = roundtrip(za, ix, tmp_path)
    assert info["flags"] & 1
    same_state(ix, ld)
    for t in (ix, ld):  # (tuning state is not saved: set on both)
        t.set_dense_levels(100)
        t.set_hash_mode("scores")
    same_answers(za, ix, ld, Q, k)
    m = za.L2SquaredDistance()
    for t in (ix, ld):
        t.search_batch(Q, k, m)
        st = t.stats()
        assert st["hash_from_scores"] == 1 and st["prefiltered"] == 1, st
    # the restart path that existed before: the answers, not the index
    old = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    old.append(X)
    old.set_forest(ix.get_forest())
    old.set_dense_levels(100)
    old.set_hash_mode("scores")
    a, b = old.search_batch(Q, k, m), ld.search_batch(Q, k, m)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and old.stats()["hash_from_scores"] == 0
    f = zo.Forest.from_arrays(X, M, ld.get_forest())
    check(ld, f, Q, k, m, zo.L2SQ, 0, "loaded, scores")
    for t in (ix, ld, old):
        t.close()


def test_compacted_with_and_without_a_lost_sample(za, tmp_path):
    n, d, M, T, B, k = 3000, 8, 700, 4, 8, 10
    X = zo.synth_rows(n, d, seed=0x5EB2D700)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D700)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.add(X)
    p0 = str(tmp_path / "first.zhs")
    ix.save(p0)
    h, sections = fmt.decode_snapshot(open(p0, "rb").read())
    samples = np.frombuffer(sections[fmt.SAMPLES], "<u4")
    assert h["flags"] == 1 and 0 < samples.size == 2 * h["n_planes"] < 400
    free = np.setdiff1d(np.arange(n), samples)
    gone = free[::7].astype(np.uint64)
    # no sample row removed: the compacted index keeps its samples, and so does its snapshot
    assert len(ix.remove(gone)) == len(gone)
    ix.compact()
    ld, p, info = roundtrip(za, ix, tmp_path, "kept.zhs")
    assert info["flags"] == 1 and info["stored_rows"] == info["live_rows"] == n - len(gone)
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, k)
    kept = np.frombuffer(fmt.decode_snapshot(open(p, "rb").read())[1][fmt.SAMPLES], "<u4")
    assert kept.size == samples.size and kept.max() < n - len(gone)
    ld.close()
    # a sample row removed: the samples are no longer valid, the file has no sample section, the loaded index hashes plane by plane like its twin
    row = np.array([int(kept[0])], np.uint64)
    assert len(ix.remove(row)) == 1
    ix.compact()
    ld, p, info = roundtrip(za, ix, tmp_path, "lost.zhs")
    assert info["flags"] == 0 and info["n_sections"] == 10
    same_state(ix, ld)
    for t in (ix, ld):
        t.set_dense_levels(100)
        t.set_hash_mode("scores")
    same_answers(za, ix, ld, Q, k)
    assert ld.stats()["hash_from_scores"] == 0
    ix.close()
    ld.close()


def test_injected_forests(za, tmp_path):
    # a forest the CPU checker built, injected: arbitrary planes, no samples
    n, d, M, T, B, k = 4000, 64, 50, 4, 10, 10
    X = zo.synth_rows(n, d, seed=0x5EB2D800)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D800)
    f = zo.Forest.build(X, M, T, seed=123)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0)
    ix.append(X)
    ix.set_forest(f.arrays())
    ld, p, info = roundtrip(za, ix, tmp_path, "injected.zhs")
    assert info["flags"] == 0
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, k)
    for m, om, omode in five_metrics(za):
        check(ld, f, Q, k, m, om, omode, "loaded, injected")
    ix.close()
    ld.close()
    # one that lists a row twice in a tree: scan_unsafe travels, compaction is still refused on the loaded index
    n, d = 64, 16
    X = zo.synth_rows(n, d, seed=0x5EB2D810)
    Q = zo.synth_queries(4, d, n, seed_rows=0x5EB2D810)
    ix = za.LSHIndex(d, za.LSHIndexOptions(128, 1), device=0)
    ix.append(X)
    ids = np.concatenate([np.arange(n), [5]]).astype(np.uint32)
    ix.set_forest(dict(plane=[-1], left=[0], right=[n + 1], roots=[0], planes=np.zeros((0, d), np.float32), consts=np.zeros(0, np.float32), leaf_ids=ids))
    ix.remove(np.array([5, 9], np.uint64))
    ld, p, info = roundtrip(za, ix, tmp_path, "twice.zhs")
    assert info["flags"] == 2
    same_state(ix, ld)
    same_answers(za, ix, ld, Q, 70)
    from zebra_amd import _ffi
    for t in (ix, ld):
        with pytest.raises(za.ZhError) as e:
            t.compact()
        assert e.value.code == _ffi.ZH_EUNSUPPORTED
    ix.close()
    ld.close()


# ------------------------------------------------------------------------------------------------------------------ 2. future equality
def test_twins_across_later_mutations(za, tmp_path):
    """one scripted sequence of add, remove, deduplicate, compact, build and add on the saved index and on the loaded one"""
    n, n2, n3, d, M, T, B, k, base = 5000, 1200, 300, 96, 40, 5, 12, 10, 1 << 33
    X = zo.synth_rows(n + n2 + n3, d, seed=0x5EB2D900)
    X[n + 100:n + 130] = X[17]
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2D900)
    rng = np.random.default_rng(3)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=base)
    ix.add(X[:3000])
    ix.add(X[3000:n])
    first = rng.choice(n, 400, replace=False).astype(np.uint64)
    first = first[first != 17]
    ix.remove(first + np.uint64(base))
    ld, p, info = roundtrip(za, ix, tmp_path)
    twins = (ix, ld)

    def step(what, results):
        assert all(np.asarray(results[0]).tobytes() == np.asarray(r).tobytes() for r in results[1:]), what
        same_state(ix, ld)
        same_answers(za, ix, ld, Q, k, exact=what in ("add", "compact"))

    step("loaded", [0, 0])
    step("add", [t.add(X[n:n + n2]) for t in twins])
    alive = np.ones(n + n2, bool)
    alive[first.astype(np.int64)] = False
    rm = rng.choice(np.flatnonzero(alive), 500, replace=False).astype(np.uint64)
    rm = rm[rm != 17]
    step("remove", [t.remove(rm + np.uint64(base)) for t in twins])
    step("deduplicate", [t.deduplicate() for t in twins])
    maps = [t.compact()[0] for t in twins]
    dups = np.setdiff1d(np.arange(n + 100, n + 130), rm.astype(np.int64))  # the copies of row 17 that remove() had not taken already
    assert (maps[0] == GONE).sum() == len(first) + len(rm) + len(dups)
    step("compact", maps)
    step("build", [t.build() or 0 for t in twins])
    step("add", [t.add(X[n + n2:]) for t in twins])
    # ... and a snapshot of the loaded index after all that is the snapshot of its twin
    pa, pb = str(tmp_path / "a.zhs"), str(tmp_path / "b.zhs")
    ix.save(pa)
    ld.save(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    ix.close()
    ld.close()


# ------------------------------------------------------------------------------------------------------------------ 3. format both ways
def test_python_written_file_loads(za, tmp_path):
    p = str(tmp_path / "small.zhs")
    X, f, removed, M, T, data = fmt.small_file(p, id_base=40)
    ld = za.LSHIndex.load(p, device=0)
    assert ld.stored_rows() == 40 and len(ld) == 38 and ld.id_base == 40 and ld.options == za.LSHIndexOptions(M, T)
    assert ld.read_rows(0, 40).tobytes() == X.tobytes()
    assert zo.canonical_forest(ld.get_forest(), 8) == zo.canonical_forest(f.arrays(), 8)
    Q = zo.synth_queries(6, 8, 40, seed_rows=0x5EB2D000)
    for m, om, omode in five_metrics(za):
        ids, keys, counts = ld.search_batch(Q, 5, m)
        oi, ok, oc = f.search_batch(Q, 5, om, omode)
        assert (counts == oc).all()
        for b in range(6):
            c = int(oc[b])
            assert (ids[b, :c] == oi[b, :c] + np.uint64(40)).all() and (keys[b, :c] == ok[b, :c]).all()
    live = np.flatnonzero(~removed)
    ids, keys, counts = ld.search_exact_batch(Q, 40, za.L2SquaredDistance())
    assert (counts == 38).all() and set(ids[0].tolist()[:38]) == set((live + 40).tolist())
    # saved again by the GPU: the writer's bytes (it has no levels table and no samples either way)
    p2 = str(tmp_path / "again.zhs")
    ld.save(p2)
    assert open(p2, "rb").read() == data
    ld.close()


def test_python_reader_parses_a_gpu_file(za, tmp_path):
    n, d, M, T = 3000, 30, 20, 4
    X = zo.synth_rows(n, d, seed=0x5EB2DA00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=12, seed=4242)
    ix.add(X[:2000])
    ix.add(X[2000:])
    gone = np.arange(5, n, 11).astype(np.uint64)
    ix.remove(gone + np.uint64(12))
    p = str(tmp_path / "gpu.zhs")
    info = ix.save(p)
    h, sections = fmt.decode_snapshot(open(p, "rb").read())  # every checksum, offset and padding byte as DESIGN s12 states them
    for key in ("version", "dim", "max_node_size", "num_trees_option", "seed", "id_base", "stored_rows", "live_rows", "n_trees", "n_nodes", "n_planes",
                "flags", "n_leaf_ids", "file_bytes", "row_bytes", "n_sections"):
        assert h[key] == info[key], key
    assert (h["seed"], h["id_base"], h["max_node_size"], h["num_trees_option"]) == (4242, 12, M, T)
    rows, removed, forest = fmt.decoded_arrays(h, sections)
    assert rows.tobytes() == ix.read_rows(0, n).tobytes() == X.tobytes()
    assert (np.flatnonzero(removed) == gone.astype(np.int64)).all()
    fa = ix.get_forest()
    for key in fa:
        assert forest[key].tobytes() == fa[key].tobytes(), key
    samples = np.frombuffer(sections[fmt.SAMPLES], "<u4").reshape(-1, 2)
    assert samples.shape[0] == h["n_planes"]
    assert (samples < n).all()  # (no plane of this forest was made from the zero vector)
    levels = np.frombuffer(sections[fmt.LEVELS], "<u4")
    assert levels[0] == 0 and (np.diff(levels.astype(np.int64)) >= 0).all() and levels[-1] <= h["n_planes"]
    # the writer re-encodes the decoded pieces to the same bytes
    again = fmt.encode_snapshot(rows, forest, removed, M, T, seed=4242, id_base=12, levels=levels, samples=samples)
    assert again == open(p, "rb").read()
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------ 4. chunking
def test_file_does_not_depend_on_the_chunk_size(za, tmp_path, monkeypatch):
    n, d = 9001, 33
    assert (n * d * 4) % 8 == 4 and n * d * 4 > 280 * 4096  # a half word at the end; several hundred chunks of 4096 bytes
    X = zo.synth_rows(n, d, seed=0x5EB2DB00)
    Q = zo.synth_queries(4, d, n, seed_rows=0x5EB2DB00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(200, 3), device=0)
    ix.add(X)
    files = {}
    for chunk in (None, 4096, 5000, 8, 4096 * 33 + 8):
        if chunk is None:
            monkeypatch.delenv("ZH_SNAPSHOT_CHUNK_BYTES", raising=False)
        else:
            assert chunk % (d * 4) != 0 or chunk == 4096 * 33 + 8
            monkeypatch.setenv("ZH_SNAPSHOT_CHUNK_BYTES", str(chunk))
        if chunk == 8 and n * d * 4 > (1 << 20):
            # one word per chunk over the whole table would be 150k chunks: a smaller table for that size
            small = za.LSHIndex(d, za.LSHIndexOptions(200, 3), device=0)
            small.add(X[:301])
            ps = str(tmp_path / "small8.zhs")
            small.save(ps)
            monkeypatch.delenv("ZH_SNAPSHOT_CHUNK_BYTES")
            pd = str(tmp_path / "smalld.zhs")
            small.save(pd)
            assert open(ps, "rb").read() == open(pd, "rb").read()
            monkeypatch.setenv("ZH_SNAPSHOT_CHUNK_BYTES", "8")
            l8 = za.LSHIndex.load(pd, device=0)
            same_state(small, l8)
            l8.close()
            small.close()
            continue
        p = str(tmp_path / ("chunk_%s.zhs" % chunk))
        ix.save(p)
        files[chunk] = open(p, "rb").read()
        ld = za.LSHIndex.load(p, device=0)  # loaded at the same chunk size
        same_state(ix, ld)
        same_answers(za, ix, ld, Q, 5, stats=False, exact=False)
        ld.close()
    assert files[None] == files[4096] == files[5000] == files[4096 * 33 + 8]
    h, sections = fmt.decode_snapshot(files[4096])
    assert sections[fmt.ROWS] == X.tobytes()
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(za, tmp_path):
    from zebra_amd import _ffi
    import ctypes as C
    n, d = 2000, 48
    X = zo.synth_rows(n, d, seed=0x5EB2DC00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(30, 3), device=0)
    ix.add(X)
    p = str(tmp_path / "good.zhs")
    ix.save(p)
    data = open(p, "rb").read()
    h, _ = fmt.decode_snapshot(data)
    L = _ffi.lib()

    def load_rc(path):
        out, info = C.c_void_p(0xDEAD), _ffi.SnapshotInfo()
        rc = L.zh_index_load(os.fsencode(path), 0, 0, C.byref(out), C.byref(info))
        return rc, out.value

    bad = str(tmp_path / "bad.zhs")
    # one flipped bit in the rows: the header and the host-side tests pass, the device's checksum of what arrived does not
    for off in (fmt.BLOCK, fmt.BLOCK + n * d * 4 // 2 + 3, fmt.BLOCK + n * d * 4 - 1):
        open(bad, "wb").write(data[:off] + bytes([data[off] ^ 0x10]) + data[off + 1:])
        assert za.snapshot_info(bad)["stored_rows"] == n  # (without verify the header is all the host looks at)
        assert load_rc(bad) == (_ffi.ZH_ECORRUPT, None)
        assert b"rows" in L.zh_last_error()
    # ... and in a forest section, the removed-row bitmap and the samples
    for kind in (fmt.NODE_LEFT, fmt.PLANES, fmt.LEAF_IDS, fmt.REMOVED, fmt.SAMPLES):
        off = struct_offset(data, kind) + 5
        open(bad, "wb").write(data[:off] + bytes([data[off] ^ 0x01]) + data[off + 1:])
        assert load_rc(bad) == (_ffi.ZH_ECORRUPT, None), kind
    # truncated: in the rows, at a section boundary, one byte short
    for cut in (fmt.BLOCK + 1000, struct_offset(data, fmt.NODE_PLANE), len(data) - 1):
        open(bad, "wb").write(data[:cut])
        assert load_rc(bad) == (_ffi.ZH_ECORRUPT, None), cut
    with pytest.raises(za.ZhError) as e:
        za.LSHIndex.load(bad, device=0)
    assert e.value.code == za.ZhError.ECORRUPT
    # well-formed checksums over a forest that names rows the table does not have: set_forest's tests refuse it
    _, sections = fmt.decode_snapshot(data)
    rows, removed, forest = fmt.decoded_arrays(h, sections)
    wrong = dict(forest)
    wrong["leaf_ids"] = forest["leaf_ids"].copy()
    wrong["leaf_ids"][7] = n
    samples = np.frombuffer(sections[fmt.SAMPLES], "<u4")
    levels = np.frombuffer(sections[fmt.LEVELS], "<u4")
    open(bad, "wb").write(fmt.encode_snapshot(rows, wrong, removed, 30, 3, levels=levels, samples=samples))
    assert za.snapshot_info(bad, verify=True)["verified"] == 1
    assert load_rc(bad) == (_ffi.ZH_ECORRUPT, None) and b"set_forest" in L.zh_last_error()
    wrong_s = samples.copy()
    wrong_s[3] = n + 5
    open(bad, "wb").write(fmt.encode_snapshot(rows, forest, removed, 30, 3, levels=levels, samples=wrong_s))
    assert load_rc(bad) == (_ffi.ZH_ECORRUPT, None) and b"sample" in L.zh_last_error()
    # a directory that does not exist: ZH_EIO, nothing left behind
    nowhere = str(tmp_path / "no" / "such" / "dir" / "x.zhs")
    with pytest.raises(za.ZhError) as e:
        ix.save(nowhere)
    assert e.value.code == za.ZhError.EIO and "No such file" in str(e.value) and not os.path.exists(str(tmp_path / "no"))
    # ... and a path that is a directory: the rename is refused, the older contents stay, no temporary file stays
    os.mkdir(str(tmp_path / "adir"))
    with pytest.raises(za.ZhError) as e:
        ix.save(str(tmp_path / "adir"))
    assert e.value.code == za.ZhError.EIO and os.path.isdir(str(tmp_path / "adir")) and not os.path.exists(str(tmp_path / "adir.zhtmp"))
    assert load_rc(str(tmp_path / "missing.zhs")) == (_ffi.ZH_EIO, None)
    # saving over an existing snapshot replaces it
    ix.add(zo.synth_rows(10, d, seed=1))
    ix.save(p)
    assert za.snapshot_info(p, verify=True)["stored_rows"] == n + 10 and sorted(os.listdir(str(tmp_path))) == ["adir", "bad.zhs", "good.zhs"]
    # loading one file twice: two independent indexes
    a, b = za.LSHIndex.load(p, device=0), za.LSHIndex.load(p, device=0)
    same_state(a, b)
    a.add(zo.synth_rows(5, d, seed=2))
    a.remove(np.array([0], np.uint64))
    assert a.stored_rows() == n + 15 and b.stored_rows() == n + 10 and len(b) == n + 10
    same_state(ix, b)
    for t in (a, b, ix):
        t.close()


def struct_offset(data, kind):
    import struct
    k, zero, off, length, s = struct.unpack("<IIQQQ", data[fmt.TABLE + 32 * (kind - 1):fmt.TABLE + 32 * kind])
    assert k == kind and length > 8
    return off


# ----------------------------------------------------------------------------------------------------------------------- 6. lifecycle
def test_shard_group_and_context_on_a_loaded_index(za, tmp_path):
    import torch
    n, d, M, T, B, k, base = 8000, 128, 64, 6, 32, 10, 7_000_000
    X = zo.synth_rows(n, d, seed=0x5EB2DD00)
    Q = zo.synth_queries(B, d, n, seed_rows=0x5EB2DD00)
    ix = za.LSHIndex(d, za.LSHIndexOptions(M, T), device=0, id_base=base)
    ix.add(X)
    ld, p, info = roundtrip(za, ix, tmp_path)
    ix.close()
    m = za.L2SquaredDistance()
    want = ld.search_batch(Q, k, m)
    f = zo.Forest.from_arrays(X, M, ld.get_forest())
    oi, ok, oc = f.search_batch(Q, k, zo.L2SQ, 0)
    assert (want[2] == oc).all() and (want[0] == oi + np.uint64(base)).all() and (want[1] == ok).all()
    g = za.ShardGroup(ld, za.shard_unique_id(), 1, 0)
    got = g.search_batch(Q, k, m)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and got[0].min() >= base  # global ids
    g.close()
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.zeros((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.zeros_like(ids), torch.zeros(B, dtype=torch.int32, device=dev)
    ctx = ld.search_context()
    for _ in range(2):
        ctx.begin(dq.data_ptr(), B, k, m)
        ctx.finish(ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
        ctx.wait()
        torch.cuda.synchronize()
        assert ids.cpu().numpy().view(np.uint64).tobytes() == want[0].tobytes() and keys.cpu().numpy().view(np.uint64).tobytes() == want[1].tobytes()
        assert counts.cpu().numpy().view(np.uint32).tobytes() == want[2].tobytes()
    ctx.close()
    ld.close()

"""Every interval the joins' and the graphs' matrix-core scans make CONTAINS the reference's key -- checked pair by pair on the device's own numbers.

Path 2 of the self-join, the cross join, the k-NN graph, the forest graph and the forest join (zh_join.hip, zh_xjoin.hip, zh_knn.hip, zh_fknn.hip,
zh_fjoin.hip) never computes a pair's key: held_walk (zh_device.h) multiplies a held tile of an fp16 row copy with column tiles that
travel through two LDS buffers, approx_interval turns a sum into an interval, and only pairs with lo <= tau go on to the canonical arithmetic.  The
"query" of a pair is a STORED row, whose view (row_as_query, zh_device.h) ASSUMES the rounding of the copy from the table's rho where the LSH scans
measure it per query.  The families' other tests are end to end: they notice a wrong interval only where a threshold or a line's bound falls between
the key and the wrong lo.  Here zh_debug_walk_pairs runs the same walk with a sink that records, and for a rectangle of 256 held positions x every
column position (~2.7 * 10^5 pairs a case) the test asserts
  * every pair of the rectangle has its record, with the row numbers the table assigns to the two positions; removed rows and the last tile's tail
    are masked, nothing else is;
  * lo <= reference key <= hi in BOTH orientations (the pool stores a pair without one): key(stored column row, query held row) and the reverse;
  * "nothing certain" (0, all ones) exactly where the rows say so: a row of the copy that is not usable, a column row whose scale is outside
    2^-104 .. 2^76 or whose norm is no finite number, a zero row under a cosine key, norms that overflow -- restated from the rows, by role;
  * |raw_s - exact| <= 2 (33 d / 128 + 2) u sum |x^ y^|: what zh_approx_bound(metric, d, 1) assumes of tile_dot's sum, against the exact sum of the
    rounded operands in float64.
The observed rounding (in units of u) and the median relative half-width are recorded per (d, key) as properties and in DESIGN.md s15a."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker)
from tests.test_gpu_intervals import U, f16_copy, unsortable  # noqa: E402

MASKED = 0xFFFFFFFF
N = 1037          # 65 tiles, the last one holds 13 rows
SLAB = (256, 256)  # (first position, positions): the planted classes below all sit in it
GONE = [5, 256 + 3, 256 + 85, 256 + 200, 700, 1030, N - 1]  # removed: outside the slab, inside it (a generic row, a duplicate), in the last tile
KEYS = ["l2sq", "cos-corrected", "cos-parity"]  # approx_interval's KINDA 0, 1, 2 (L2 shares KINDA 0 and its interval's scale with L2 squared)


@pytest.fixture(scope="module")
def za():
    import zebra_amd
    return zebra_amd


def metric_of(za, key):
    return {"l2sq": za.L2SquaredDistance(), "cos-corrected": za.CosineDistance(parity=False), "cos-parity": za.CosineDistance(parity=True)}[key]


def planted_rows(X, base):
    """the classes tests/test_gpu_intervals.py's special_rows names, 16 rows each so that ONE slab of 256 positions from `base` meets them all, and
    three more: rows whose scale the column view refuses, rows the copy itself refuses"""
    X = X.copy()
    b = base
    X[b + 16:b + 32] *= np.float32(2.0 ** 40)                       # huge rows (|x|^2 ~ 2^90: still finite in f32)
    X[b + 32:b + 48] *= np.float32(2.0 ** -40)                      # tiny rows
    X[b + 48:b + 64] = np.round(X[b + 48:b + 64] * 4.0)             # integer-valued rows: ties, exact products
    sub = X[b + 64:b + 80]                                          # subnormal-heavy in fp16: one large element, the rest 2^-13..2^-16 of it
    sub *= np.float32(2.0 ** -14)
    sub[:, 7] = np.float32(3.0)
    X[b + 64:b + 80] = sub
    first = X[b:b + 16]
    X[b + 80:b + 96] = first                                        # exact duplicates
    X[b + 96:b + 112] = np.nextafter(first, np.float32(np.inf))     # one ulp away in every coordinate
    X[b + 112:b + 128] = first * np.float32(1.0 + 2.0 ** -12)       # near-duplicates below the fp16 resolution
    X[b + 128:b + 136] = 0.0                                        # zero rows
    X[b + 136:b + 144] *= np.float32(4e18)                          # |x|^2 overflows f32
    X[b + 144:b + 148] *= np.float32(2.0 ** -97)                    # the copy holds them (exponent >= -100), no column view (scale < 2^-104)
    X[b + 148:b + 152] *= np.float32(2.0 ** -112)                   # not usable in the copy either
    X[b + 152:b + 156] *= np.float32(2.0 ** 85)                     # a scale inside the range (2^73), |x|^2 overflows
    return X


def generic_table(d):
    return planted_rows(zo.synth_rows(N, d), SLAB[0])


def exact_table(d, n=300):
    """rows fp16 holds exactly under any scale (multiples of 1/8 below 8): the copy's rho is 0"""
    rng = np.random.default_rng(41 + d)
    return np.clip(np.round(rng.standard_normal((n, d)) * 8.0) / 8.0, -7.0, 7.0).astype(np.float32)


def make_index(za, X, gone=()):
    ix = za.LSHIndex(X.shape[1], za.LSHIndexOptions(64, 4), device=0)
    ix.append(X)
    if len(gone):
        ix.remove(list(gone))
    return ix


def row_facts(X):
    """what the kernels' usability tests read of every row, restated from the f32 rows: row_half_kernel's `usable` (every element finite, the largest
    one's exponent in -100 .. 100), row_as_query's (1 / sigma = 2^(ex - 14) in 2^-104 .. 2^76, |x|^2 a finite f32) and the f32 norm"""
    X = np.asarray(X, np.float32)
    m = np.abs(X).max(axis=1)
    _, ex = np.frexp(m)
    ex = np.where(m > 0, ex, 14)
    copy_ok = np.isfinite(X).all(axis=1) & (ex >= -100) & (ex <= 100)
    with np.errstate(over="ignore"):
        a2 = (X.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    col_ok = copy_ok & (ex - 14 >= -104) & (ex - 14 <= 76) & np.isfinite(a2)
    return {"copy_ok": copy_ok, "col_ok": col_ok, "a2": a2, "norm": np.sqrt(a2.astype(np.float64))}


def reference_values(XH, XC, key):
    """the reference's key of every (held row, column row) pair in the scale its interval is made in (oracle_values of tests/test_gpu_intervals.py),
    in both orientations -> two [held, column] float64 matrices: stored column row against the held row as the query, and the reverse"""
    om, omode = {"l2sq": (zo.L2SQ, 0), "cos-corrected": (zo.COSINE, zo.CORRECTED), "cos-parity": (zo.COSINE, zo.PARITY)}[key]
    v1 = np.stack([zo.key_to_float(zo.distance_batch(om, omode, XC, x)) for x in XH])
    v2 = np.stack([zo.key_to_float(zo.distance_batch(om, omode, XH, y)) for y in XC], axis=1)
    if key == "cos-parity":  # the literal key 1 - distance compares as the bits of the f64: positives ascending, then negatives by magnitude
        v1, v2 = np.where(v1 > 0, v1, 2.0 - v1), np.where(v2 > 0, v2, 2.0 - v2)
    return v1, v2


def check_rectangle(left, right, XL, XR, live_l, live_r, key, za, first, n_pos, d, what, record=None):
    """XL / XR: the f32 rows of the two tables BY POSITION of their copies (NaN rows past the table); live_l / live_r: the row number at each
    position, or MASKED"""
    info, p = left.debug_walk_pairs(metric_of(za, key), first, n_pos, right)
    ncol = XR.shape[0]
    assert info["held_positions"] == n_pos and info["col_positions"] == ncol and info["pairs"] == n_pos * ncol == p.shape[0], (what, info)
    p = p.reshape(n_pos, ncol)
    # ---- coverage: every pair of the rectangle once, at its place, with the row numbers of its positions; masked = removed or tail
    assert (p["held_pos"] == (first + np.arange(n_pos, dtype=np.uint32))[:, None]).all(), what
    assert (p["col_pos"] == np.arange(ncol, dtype=np.uint32)[None, :]).all(), what
    assert (p["held_row"] == live_l[first:first + n_pos, None]).all(), what
    assert (p["col_row"] == live_r[None, :]).all(), what
    on = (p["held_row"] != MASKED) & (p["col_row"] != MASKED)
    assert on.sum() == (live_l[first:first + n_pos] != MASKED).sum() * (live_r != MASKED).sum() > 0, what
    XH = XL[first:first + n_pos]
    hl, cl = np.flatnonzero(live_l[first:first + n_pos] != MASKED), np.flatnonzero(live_r != MASKED)
    sub = np.ix_(hl, cl)   # the unmasked pairs, as a matrix
    q = p[sub]
    fh, fc = row_facts(XH[hl]), row_facts(XR[cl])
    # ---- "nothing certain", from the rows and by role (approx_interval's own tests, given usable operands)
    unsure = (q["lo"] == 0) & (q["hi"] == MASKED)
    bad = ~fh["copy_ok"][:, None] | ~fc["col_ok"][None, :] | ~np.isfinite(fh["a2"])[:, None]
    with np.errstate(over="ignore"):
        if key == "l2sq":   # the norms' sum below 1e37, not both rows zero
            nx, nq = fh["norm"][:, None], fc["norm"][None, :]
            bad |= ~(fh["a2"][:, None].astype(np.float64) + fc["a2"][None, :].astype(np.float64) < 1e37) | ~(nx + nq > 1e-12)
        else:               # neither norm zero
            bad |= ~(fh["norm"] > 1e-12)[:, None] | ~(fc["norm"] > 1e-12)[None, :]
    v1, v2 = reference_values(XH[hl], XR[cl], key)
    either = np.zeros_like(bad)
    if key == "cos-parity":
        # the parity key's order wraps at 0: approx_interval gives up where |1 - r| <= e, its own half-width.  The device's r is within e of the
        # reference's distance, so a reference key further than 2 e from 0 must have an interval; inside that band either answer is right
        rl, rr = float(info["rho_left"]), float(info["rho_right"])
        dqr = rr * (1.0 + 1e-5) * 1.0000005
        e_up = (float(info["bound_const"]) + 1.01 * (dqr + rl * (1.0 + dqr))) * (1.0 + 1e-5)
        k1, k2 = np.where(v1 < 1.5, v1, 2.0 - v1), np.where(v2 < 1.5, v2, 2.0 - v2)   # back to the key 1 - distance
        either = (np.abs(k1) <= 2.0 * e_up) | (np.abs(k2) <= 2.0 * e_up)
    wrong = (unsure != bad) & ~(either & ~bad)
    if wrong.any():
        i, j = (int(t[0]) for t in np.nonzero(wrong))
        raise AssertionError(f"{what}: held row {q['held_row'][i, j]} x column row {q['col_row'][i, j]} is {'un' if unsure[i, j] else ''}certain on the "
                             f"device, the rows say {'un' if bad[i, j] else ''}certain ({int(wrong.sum())} of {wrong.size} pairs)")
    # ---- containment, both orientations
    lo, hi = unsortable(q["lo"]), unsortable(q["hi"])
    ok = unsure | ((lo <= v1) & (v1 <= hi) & (lo <= v2) & (v2 <= hi))
    if not ok.all():
        i, j = (int(t[0]) for t in np.nonzero(~ok))
        raise AssertionError(f"{what}: interval [{lo[i, j]!r}, {hi[i, j]!r}] does not contain the reference's {v1[i, j]!r} / {v2[i, j]!r} "
                             f"(held row {q['held_row'][i, j]} at position {q['held_pos'][i, j]}, column row {q['col_row'][i, j]} at position "
                             f"{q['col_pos'][i, j]}; {int((~ok).sum())} of {ok.size} pairs)")
    assert (~unsure).sum() > 0.5 * ok.size, what
    fin = ~unsure & np.isfinite(lo) & np.isfinite(hi) & (np.abs(v1) > 0)
    rel = float(np.median((hi[fin] - lo[fin]) / 2 / np.abs(v1[fin]))) if fin.any() else float("nan")
    # ---- the rounding model: tile_dot's sum against the exact sum of the rounded operands
    hh, hs = f16_copy(XH[hl])
    ch, _ = f16_copy(XR[cl])
    with np.errstate(over="ignore", invalid="ignore"):
        exact = hh @ ch.T
        absum = np.abs(hh) @ np.abs(ch).T
        got = q["raw_s"].astype(np.float64) * hs[:, None]   # raw_s = acc / sigma_x (a power of two: exact)
    good = np.isfinite(got) & np.isfinite(exact) & (absum > 0) & fh["copy_ok"][:, None] & fc["copy_ok"][None, :]
    assert good.sum() > 0.5 * good.size, what
    err = np.abs(got[good] - exact[good]) / absum[good] / U
    worst, assumed = float(err.max()), 2.0 * (33.0 * (d // 128) + 2.0)
    print(f"{what}: {ok.size} pairs, {int(unsure.sum())} uncertain, median half-width {rel:.2e} of the value; max |acc - exact| = {worst:.2f} u * "
          f"sum|x^ y^| (assumed <= {assumed:.0f} u), rho = {info['rho_left']:.3e} / {info['rho_right']:.3e}")
    if record:
        record(f"pair_rounding_u_d{d}_{key}", worst)
        record(f"pair_median_rel_halfwidth_d{d}_{key}", rel)
    assert worst <= assumed, f"{what}: the walk's sum is {worst:.2f} u * sum|x y| from the exact one; zh_approx_bound assumes <= {assumed:.0f} u"
    return info


def by_position(X, gone, n_pos):
    """id order: position = row number"""
    live = np.full(n_pos, MASKED, np.uint32)
    live[:X.shape[0]] = np.arange(X.shape[0], dtype=np.uint32)
    live[list(gone)] = MASKED
    XP = np.full((n_pos, X.shape[1]), np.nan, np.float32)
    XP[:X.shape[0]] = X
    return XP, live


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("d", [256, 384, 512, 768, 1024])
def test_walk_intervals_contain_the_key(za, d, key, monkeypatch, record_property):
    """the 15 instantiations: one table against itself (the self-join's and the graphs' view), the slab that holds every planted class"""
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    X = generic_table(d)
    ix = make_index(za, X, GONE)
    XP, live = by_position(X, GONE, 1040)
    info = check_rectangle(ix, None, XP, XP, live, live, key, za, SLAB[0], SLAB[1], d, f"walk<{d}> {key}", record_property)
    assert info["order_left"] == 0 and info["rho_left"] == info["rho_right"] and 0 < info["rho_left"] < 2.0 ** -10
    ix.close()


@pytest.mark.parametrize("key", KEYS)
def test_slab_at_the_tables_end(za, key, monkeypatch):
    """the last slab: 13 tiles, the last of them partial with a removed row, the tail masked"""
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    d = 384
    X = generic_table(d)
    ix = make_index(za, X, GONE)
    XP, live = by_position(X, GONE, 1040)
    check_rectangle(ix, None, XP, XP, live, live, key, za, 832, 208, d, f"walk<{d}> {key}, last slab")
    ix.close()


@pytest.mark.parametrize("key", KEYS)
def test_cross_tables_in_both_directions(za, key, monkeypatch):
    """the cross join's view: a table fp16 holds exactly (rho 0) against a generic one.  The held side takes ITS table's rho, the column side's goes
    into the column rows' dq: with the two swapped or both from one table, one direction has nothing that covers the generic rows' rounding"""
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    d = 256
    XA, XB = exact_table(d), generic_table(d)
    gone_a = [7, 100, 299]
    ia, ib = make_index(za, XA, gone_a), make_index(za, XB, GONE)
    PA, live_a = by_position(XA, gone_a, 304)
    PB, live_b = by_position(XB, GONE, 1040)
    info = check_rectangle(ia, ib, PA, PB, live_a, live_b, key, za, 64, 240, d, f"walk<{d}> {key}, exact x generic")
    assert info["rho_left"] == 0.0 and info["rho_right"] > 0
    info = check_rectangle(ib, ia, PB, PA, live_b, live_a, key, za, SLAB[0], SLAB[1], d, f"walk<{d}> {key}, generic x exact")
    assert info["rho_right"] == 0.0 and info["rho_left"] > 0
    ia.close()
    ib.close()


def test_positions_that_are_not_ids(za, monkeypatch):
    """the fp16 copy in a forest's row order: position p holds another row than p.  The records carry the row at each position: the column
    positions hold every live row once, a held position the row its column twin holds, and the rows so named are the ones whose products and keys
    the records hold -- raw_s is within a few u of the exact sum of THOSE rows' rounded values, the interval contains THEIR key"""
    d = 256
    X = zo.synth_rows(N, d).copy()
    X[300:316] = X[:16]   # duplicates, wherever the order puts them
    gone = [3, 310, 900]
    monkeypatch.setenv("ZH_ROW_ORDER", "2")
    ix = za.LSHIndex(d, za.LSHIndexOptions(300, 9), device=0)
    ix.add(X)
    ix.set_sweep_mode("approx")
    ix.search_batch(zo.synth_queries(16, d, N), 10, za.L2Distance())  # (the matrix-core scan makes the copy, in the forced order)
    assert ix.stats()["scan_order_keys"] == 2
    ix.remove(gone)
    m = za.L2SquaredDistance()
    info, p = ix.debug_walk_pairs(m, 0, 64)
    assert info["order_left"] == 1 and info["order_right"] == 1
    cols = p.reshape(64, 1040)["col_row"][0]
    alive = np.setdiff1d(np.arange(N), gone)
    assert (np.sort(cols[cols != MASKED]) == alive).all() and (cols[N:] == MASKED).all()
    assert (cols[:N] != np.arange(N)).any()   # (not the id order)
    perm = np.full(1040, MASKED, np.uint32)   # position -> row; a removed row's position is masked: its row is the one no position names
    perm[:N] = cols[:N]
    XP = np.full((1040, d), np.nan, np.float32)
    XP[perm != MASKED] = X[perm[perm != MASKED]]
    for key in KEYS:
        check_rectangle(ix, None, XP, XP, perm, perm, key, za, 512, 256, d, f"walk<{d}> {key}, row order")
    ix.close()


def test_refusals(za, monkeypatch):
    """an unsupported dimension or metric and a slab that is misplaced or too long are ZH_EINVAL; an output that is too small is ZH_ELIMIT with the
    needed count, and nothing is stored"""
    from zebra_amd import _ffi
    monkeypatch.setenv("ZH_ROW_ORDER", "0")
    L = _ffi.lib()
    ix = make_index(za, zo.synth_rows(200, 256))
    small = make_index(za, zo.synth_rows(200, 128))
    other = make_index(za, zo.synth_rows(200, 384))

    def call(left, right, m, first, n_pos, out=None, cap=0):
        info = _ffi.DebugWalkInfo()
        rc = L.zh_debug_walk_pairs(left._h, right._h, m.metric, m.mode, first, n_pos, C.byref(info), out, cap)
        return rc, info

    l2 = za.L2SquaredDistance()
    assert call(small, small, l2, 0, 64)[0] == _ffi.ZH_EINVAL
    assert call(ix, ix, za.ManhattanDistance(), 0, 64)[0] == _ffi.ZH_EINVAL
    assert call(ix, other, l2, 0, 64)[0] == _ffi.ZH_EINVAL
    assert call(ix, ix, l2, 32, 64)[0] == _ffi.ZH_EINVAL       # not on a multiple of 64
    assert call(ix, ix, l2, 0, 0)[0] == _ffi.ZH_EINVAL
    assert call(ix, ix, l2, 192, 64)[0] == _ffi.ZH_EINVAL      # 13 tiles = 208 positions
    assert call(ix, ix, l2, 0, 1025)[0] == _ffi.ZH_EINVAL
    rc, info = call(ix, ix, l2, 128, 72)
    assert rc == 0 and info.pairs == 72 * 208 and info.held_positions == 72 and info.col_positions == 208
    buf = np.full(info.pairs * 7, 0x5A5A5A5A, np.uint32)
    rc, info = call(ix, ix, l2, 128, 72, buf.ctypes.data_as(C.c_void_p), info.pairs - 1)
    assert rc == _ffi.ZH_ELIMIT and info.pairs == 72 * 208 and (buf == 0x5A5A5A5A).all()
    rc, info = call(ix, ix, l2, 128, 72, buf.ctypes.data_as(C.c_void_p), info.pairs)
    assert rc == 0 and (buf.reshape(-1, 7)[:, 0] == 128 + np.repeat(np.arange(72), 208)).all()
    for i in (ix, small, other):
        i.close()

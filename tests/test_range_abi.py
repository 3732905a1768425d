"""The range search's C ABI (zh_search_range_*): declared in the header, exported under SYMBOLS, zh_range_info's layout mirrored by ctypes,
the argument checks that are judged before any device is touched, and radius_key's rounding.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import zebra_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = ("zh_search_range_batch", "zh_search_range_batch_device", "zh_search_range_info")
FIELDS = ("batch", "rows_live", "hits", "path", "redone", "candidates", "launches")


def test_header_declares_the_range_search():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in RANGE:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_range_info" in h


def test_symbols_list_the_range_search():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in RANGE:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in RANGE:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.RangeInfo._fields_] == list(FIELDS)


def test_range_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_range_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_range_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.RangeInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_sibling_info_structs_are_unchanged():
    from zebra_amd import _ffi
    assert [f for f, _ in _ffi.ExactInfo._fields_] == ["batch", "rows_live", "path", "redone", "survivors", "launches"]
    assert [f for f, _ in _ffi.FilteredInfo._fields_] == ["batch", "rows_live", "rows_allowed", "path", "redone", "survivors", "launches",
                                                          "tiles_skipped"]


def test_arguments_are_judged_before_any_device():
    """A null index, null thresholds for a batch, null outputs for a capacity and an unknown metric are refused by the first lines of either
    entry point.  The calls that pass a (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock
    that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    q = (ctypes.c_float * 8)()
    mk = (ctypes.c_uint64 * 4)()
    off, ids, keys, total = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 1)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def host(ix, b, mkp, metric, cap, offp, idp, keyp, totp):
        return L.zh_search_range_batch(ix, P(q), b, mkp, metric, 0, cap, offp, idp, keyp, totp)

    def dev(ix, b, mkp, metric, cap, offp, idp, keyp, totp):
        return L.zh_search_range_batch_device(ix, P(q), b, mkp, metric, 0, cap, offp, idp, keyp, totp, None)

    for call in (host, dev):
        assert call(None, 1, P(mk), 0, 4, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 1, None, 0, 4, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 1, P(mk), 0, 4, P(off), None, P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 1, P(mk), 0, 4, P(off), P(ids), None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 0, P(mk), 0, 4, P(off), None, None, P(total)) == _ffi.ZH_EINVAL  # (a capacity wants its arrays whatever the batch)
        assert call(idx, 1, P(mk), 0, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 1, P(mk), 0, 0, P(off), None, None, None) == _ffi.ZH_EINVAL
        assert call(idx, 1, P(mk), 99, 4, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, 0, P(mk), 99, 0, P(off), None, None, P(total)) == _ffi.ZH_EINVAL
    # the host call answers an empty batch without an index's help: offsets[0] = 0, total 0
    off[0], total[0] = 7, 7
    assert L.zh_search_range_batch(idx, P(q), 0, None, 0, 0, 0, P(off), None, None, P(total)) == _ffi.ZH_OK
    assert off[0] == 0 and total[0] == 0
    info = _ffi.RangeInfo()
    assert L.zh_search_range_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_search_range_info(idx, None) == _ffi.ZH_EINVAL


# ---- radius_key: the largest key that means "distance <= radius" ----
def metrics(za):
    return [(za.L2SquaredDistance(), zo.L2SQ), (za.L2Distance(), zo.L2), (za.CosineDistance(parity=True), zo.COSINE),
            (za.CosineDistance(parity=False), zo.COSINE), (za.ChebyshevDistance(), zo.CHEBYSHEV), (za.CanberraDistance(), zo.CANBERRA),
            (za.BrayCurtisDistance(), zo.BRAY_CURTIS), (za.ManhattanDistance(), zo.MANHATTAN), (za.L3Distance(), zo.L3), (za.L4Distance(), zo.L4),
            (za.HammingDistance(), zo.HAMMING), (za.MinkowskiDistance(3), zo.MINKOWSKI), (za.PNormDistance(65), zo.PNORM)]


def key_value(om, keys):
    """the number a key holds.  oracle.key_to_float reads the f64 pattern of the three f64-keyed metrics; the others' keys are an f32 widened to
    64 bits (key_of) -- read through key_to_float they would all be denormals -- and Hamming's is the count itself"""
    keys = np.asarray(keys, np.uint64)
    if om in (zo.COSINE, zo.L2SQ, zo.L2):
        return zo.key_to_float(keys)
    if om == zo.HAMMING:
        return keys.astype(np.float64)
    return keys.astype(np.uint32).view(np.float32).astype(np.float64)


RADII = [0.0, 5e-324, 1e-40, 0.1, 0.2, 1.0 / 3.0, 0.5, 1.0, 1.0 + 2.0**-30, 7.0, 7.5, 255.999, 1e10, 3.0e38, 3.5e38]


def test_radius_key_is_the_largest_key_at_or_below_the_radius():
    import zebra_amd as za
    for m, om in metrics(za):
        for r in RADII:
            if om == zo.HAMMING and r > 2.0**53:
                continue  # (a count is an integer: past 2^53 "the next key up" is not a different f64, and no row has that many bits)
            k = za.radius_key(m, r)
            assert isinstance(k, np.uint64), (om, r)
            assert key_value(om, [k])[0] <= r, (om, r, k)
            assert key_value(om, [k + np.uint64(1)])[0] > r, (om, r, k)  # the next key up is past the radius
        # one radius per query, the metric given as its number
        ks = za.radius_key(m.metric, np.array(RADII))
        assert ks.dtype == np.uint64 and ks.tolist() == [int(za.radius_key(m, r)) for r in RADII]
        # an infinite radius admits every key that holds a number
        kinf = za.radius_key(m, np.inf)
        assert key_value(om, [kinf])[0] >= 3.4e38 or om == zo.HAMMING
        for bad in (-1.0, np.nan, [0.5, -0.0001], [np.nan, 1.0]):
            with pytest.raises(ValueError):
                za.radius_key(m, bad)
        assert za.radius_key(m, -0.0) == za.radius_key(m, 0.0)


def test_radius_key_admits_what_the_oracle_keys():
    """on real keys: rows with the oracle's distance value <= r are exactly the rows with key <= radius_key (unsigned), for every metric whose
    keys never hold a negative number (all but the parity cosine key, whose order the header defines as the bit pattern's)"""
    import zebra_amd as za
    X = zo.synth_rows(300, 30)
    q = zo.synth_queries(1, 30, 300)[0]
    for m, om in metrics(za):
        keys = zo.distance_batch(om, m.mode, X, q)
        vals = key_value(om, keys)
        if (vals < 0).any() or np.isnan(vals).any():
            continue
        for r in np.sort(vals)[[0, 30, 150, 299]]:  # (taken from the data: ties with the radius itself are hits)
            assert ((keys <= za.radius_key(m, r)) == (vals <= r)).all(), (om, r)

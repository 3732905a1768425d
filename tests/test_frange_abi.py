"""The forest range search's C ABI (zh_search_range_forest_*): declared in the header, exported under SYMBOLS, zh_range_forest_info's layout mirrored by
ctypes, the sibling info structs unchanged, the argument checks that are judged before any device is touched, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zh_search_range_forest_batch", "zh_search_range_forest_batch_device", "zh_search_range_forest_info")
FIELDS = ("batch", "rows_live", "trees", "probe", "path", "redone", "visits", "leaf_rows", "hits", "candidates", "launches", "tiles")


def test_header_declares_the_forest_range_search():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in NAMES:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_range_forest_info" in h
    # the device form takes device outputs and a stream as its last argument, as zh_search_range_batch_device
    assert re.search(r"zh_search_range_forest_batch_device\s*\([^;]*d_out_total\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    # both forms take zh_search_range_batch's arguments with `probe` inserted after max_keys
    args = lambda name: re.sub(r"\s+", " ", re.search(r"ZH_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, h).group(1))  # noqa: E731
    assert args("zh_search_range_forest_batch") == args("zh_search_range_batch").replace("max_keys, ", "max_keys, uint32_t probe, ")
    assert args("zh_search_range_forest_batch_device") == args("zh_search_range_batch_device").replace("d_max_keys, ", "d_max_keys, uint32_t probe, ")
    assert "uint32_t probe" in args("zh_search_range_forest_batch") and "uint32_t probe" in args("zh_search_range_forest_batch_device")
    assert "zh_search_range_forest_batch[_device]" in h[:h.index("Conventions")]  # the list at the top


def test_symbols_list_the_forest_range_search():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in NAMES:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.RangeForestInfo._fields_] == list(FIELDS)
    sig = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    for forest, exact in (("zh_search_range_forest_batch", "zh_search_range_batch"), ("zh_search_range_forest_batch_device", "zh_search_range_batch_device")):
        res, a = sig[exact]
        assert sig[forest] == (res, a[:4] + [ctypes.c_uint32] + a[4:])  # probe after max_keys


def test_forest_range_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_range_forest_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_range_forest_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.RangeForestInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_sibling_info_structs_are_unchanged():
    from zebra_amd import _ffi
    assert [f for f, _ in _ffi.ExactInfo._fields_] == ["batch", "rows_live", "path", "redone", "survivors", "launches"]
    assert [f for f, _ in _ffi.FilteredInfo._fields_] == ["batch", "rows_live", "rows_allowed", "path", "redone", "survivors", "launches",
                                                          "tiles_skipped"]
    assert [f for f, _ in _ffi.RangeInfo._fields_] == ["batch", "rows_live", "hits", "path", "redone", "candidates", "launches"]
    assert [f for f, _ in _ffi.JoinInfo._fields_] == ["rows_live", "pairs", "path", "redone", "candidates", "launches", "tiles"]
    assert [f for f, _ in _ffi.KnnInfo._fields_] == ["rows_live", "lines", "k", "path", "redone", "survivors", "launches", "tiles"]
    assert [f for f, _ in _ffi.KnnForestInfo._fields_] == ["rows_live", "lines", "k", "path", "trees", "pairs", "survivors", "redone", "launches",
                                                           "tiles"]
    assert [f for f, _ in _ffi.JoinForestInfo._fields_] == ["rows_live", "trees", "path", "leaf_pairs", "pairs", "candidates", "launches", "tiles",
                                                            "redone"]


def test_arguments_are_judged_before_any_device():
    """A null index, null queries or thresholds with b > 0, null offsets or total, null arrays with a capacity, an unknown metric, probe = 0 and
    probe > ZH_MAX_TOPK are refused by the first lines of either entry point.  The calls that pass a (never dereferenced) stand-in for the index
    must fail: were a check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    q = (ctypes.c_float * 64)()
    mk, off, ids, keys, total = ((ctypes.c_uint64 * 8)() for _ in range(5))
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(ix, qp, b, mp, probe, metric, cap, op, ip, kp, tp):
        return L.zh_search_range_forest_batch(ix, qp, b, mp, probe, metric, 0, cap, op, ip, kp, tp)

    def dev(ix, qp, b, mp, probe, metric, cap, op, ip, kp, tp):
        return L.zh_search_range_forest_batch_device(ix, qp, b, mp, probe, metric, 0, cap, op, ip, kp, tp, None)

    for call in (host, dev):
        assert call(None, P(q), 2, P(mk), 1, 1, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, P(q), 2, P(mk), 1, 1, 0, P(off), None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, None, 2, P(mk), 1, 1, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, P(q), 2, None, 1, 1, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1, 1, 8, None, P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1, 1, 8, P(off), P(ids), P(keys), None) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1, 1, 8, P(off), None, P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1, 1, 8, P(off), P(ids), None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1, 99, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, P(q), 2, P(mk), 1, 99, 0, P(off), None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 0, 1, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_EINVAL and b"probe" in L.zh_last_error()
        assert call(idx, P(q), 2, P(mk), 0, 1, 0, P(off), None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, P(q), 2, P(mk), 1025, 1, 8, P(off), P(ids), P(keys), P(total)) == _ffi.ZH_ELIMIT and b"probe" in L.zh_last_error()
        assert call(idx, P(q), 0, None, 1025, 1, 0, P(off), None, None, P(total)) == _ffi.ZH_ELIMIT  # ... whatever the batch
    info = _ffi.RangeForestInfo()
    assert L.zh_search_range_forest_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_search_range_forest_info(idx, None) == _ffi.ZH_EINVAL


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "frange_example.c"), "-o", os.path.join(td, "e.o")])

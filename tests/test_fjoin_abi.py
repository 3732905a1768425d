"""The forest self-join's C ABI (zh_self_join_forest*): declared in the header, exported under SYMBOLS, zh_join_forest_info's layout mirrored by ctypes,
the sibling info structs unchanged, the argument checks that are judged before any device is touched, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN = ("zh_self_join_forest", "zh_self_join_forest_device", "zh_self_join_forest_info")
FIELDS = ("rows_live", "trees", "path", "leaf_pairs", "pairs", "candidates", "launches", "tiles", "redone")


def test_header_declares_the_forest_join():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in JOIN:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_join_forest_info" in h
    # the device form takes device outputs and a stream as its last argument, as zh_self_join_device
    assert re.search(r"zh_self_join_forest_device\s*\([^;]*d_out_total\s*,\s*void\s*\*\s*stream\s*\)\s*;", h)
    # both forms take zh_self_join's arguments
    args = lambda name: re.sub(r"\s+", " ", re.search(r"ZH_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, h).group(1))  # noqa: E731
    assert args("zh_self_join_forest") == args("zh_self_join") and args("zh_self_join_forest_device") == args("zh_self_join_device")
    assert "zh_self_join_forest[_device]" in h[:h.index("Conventions")]  # the list at the top


def test_symbols_list_the_forest_join():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in JOIN:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in JOIN:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.JoinForestInfo._fields_] == list(FIELDS)
    sig = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert sig["zh_self_join_forest"] == sig["zh_self_join"] and sig["zh_self_join_forest_device"] == sig["zh_self_join_device"]


def test_forest_join_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_join_forest_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_join_forest_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.JoinForestInfo
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


def test_arguments_are_judged_before_any_device():
    """A null index, a null out_total, null arrays with a capacity and an unknown metric are refused by the first lines of either entry point.
    The calls that pass a (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that stand-in
    and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    a, b, keys, total = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 1)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(ix, metric, cap, ap, bp, kp, tp):
        return L.zh_self_join_forest(ix, 5, metric, 0, cap, ap, bp, kp, tp)

    def dev(ix, metric, cap, ap, bp, kp, tp):
        return L.zh_self_join_forest_device(ix, 5, metric, 0, cap, ap, bp, kp, tp, None)

    for call in (host, dev):
        assert call(None, 1, 8, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, 1, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 1, 8, P(a), P(b), P(keys), None) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 1, 0, None, None, None, None) == _ffi.ZH_EINVAL
        assert call(idx, 1, 8, None, P(b), P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 1, 8, P(a), None, P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 1, 8, P(a), P(b), None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 99, 8, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, 99, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
    info = _ffi.JoinForestInfo()
    assert L.zh_self_join_forest_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_self_join_forest_info(idx, None) == _ffi.ZH_EINVAL


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "fjoin_example.c"), "-o", os.path.join(td, "e.o")])

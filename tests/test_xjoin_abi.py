"""The cross-join's C ABI (zh_cross_join*): declared in the header, exported under SYMBOLS, zh_cross_info's layout mirrored by ctypes, the sibling
info structs unchanged, the argument checks that are judged before any device is touched, and remove_within's host rule.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS = ("zh_cross_join", "zh_cross_join_device", "zh_cross_join_info")
FIELDS = ("rows_live_a", "rows_live_b", "pairs", "path", "redone", "candidates", "launches", "tiles")


def test_header_declares_the_cross_join():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in CROSS:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_cross_info" in h
    assert "(new; the reference has no such call)" in h[h.index("JOIN BETWEEN TWO INDEXES"):h.index("ZH_API int zh_cross_join(")]


def test_symbols_list_the_cross_join():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in CROSS:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CROSS:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.CrossInfo._fields_] == list(FIELDS)


def test_cross_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_cross_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_cross_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.CrossInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_sibling_info_structs_are_unchanged():
    from zebra_amd import _ffi
    assert hasattr(_ffi, "CrossInfo")
    assert [f for f, _ in _ffi.ExactInfo._fields_] == ["batch", "rows_live", "path", "redone", "survivors", "launches"]
    assert [f for f, _ in _ffi.RangeInfo._fields_] == ["batch", "rows_live", "hits", "path", "redone", "candidates", "launches"]
    assert [f for f, _ in _ffi.JoinInfo._fields_] == ["rows_live", "pairs", "path", "redone", "candidates", "launches", "tiles"]
    assert [f for f, _ in _ffi.KnnInfo._fields_] == ["rows_live", "lines", "k", "path", "redone", "survivors", "launches", "tiles"]
    assert [f for f, _ in _ffi.JoinForestInfo._fields_] == ["rows_live", "trees", "path", "leaf_pairs", "pairs", "candidates", "launches", "tiles",
                                                            "redone"]


def test_arguments_are_judged_before_any_device():
    """A null index on either side, the same index twice, a null total, null arrays for a capacity and an unknown metric are refused by the first
    lines of either entry point.  The calls that pass (never dereferenced) stand-ins for the indexes must fail: were a check lost, the call
    would go on to lock a stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake_a, fake_b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    ia, ib = ctypes.cast(fake_a, ctypes.c_void_p), ctypes.cast(fake_b, ctypes.c_void_p)
    a, b, keys, total = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 1)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(xa, xb, metric, cap, ap, bp, kp, tp):
        return L.zh_cross_join(xa, xb, 2**64 - 1, metric, 0, cap, ap, bp, kp, tp)

    def dev(xa, xb, metric, cap, ap, bp, kp, tp):
        return L.zh_cross_join_device(xa, xb, 2**64 - 1, metric, 0, cap, ap, bp, kp, tp, None)

    for call in (host, dev):
        assert call(None, ib, 0, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(ia, None, 0, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, None, 0, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
        assert call(ia, ia, 0, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL and b"zh_self_join" in L.zh_last_error()
        assert call(ia, ia, 0, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL and b"zh_self_join" in L.zh_last_error()
        assert call(ia, ib, 0, 4, P(a), P(b), P(keys), None) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(ia, ib, 0, 0, None, None, None, None) == _ffi.ZH_EINVAL
        assert call(ia, ib, 0, 4, None, P(b), P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(ia, ib, 0, 4, P(a), None, P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(ia, ib, 0, 4, P(a), P(b), None, P(total)) == _ffi.ZH_EINVAL
        assert call(ia, ib, 99, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL  # no such metric
        assert call(ia, ib, 99, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
    info = _ffi.CrossInfo()
    assert L.zh_cross_join_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_cross_join_info(ia, None) == _ffi.ZH_EINVAL


def test_remove_within_rule_is_the_distinct_left_rows():
    from zebra_amd.index import matched_rule
    # pairs (3, x), (3, y), (7, z): rows 3 and 7 of the left index each have a partner
    got = matched_rule(np.array([3, 3, 7], np.uint64))
    assert got.dtype == np.uint64 and got.tolist() == [3, 7]
    assert matched_rule(np.array([], np.uint64)).tolist() == []
    assert matched_rule(np.array([2**40 + 5, 2**40 + 5, 2**40 + 1], np.uint64)).tolist() == [2**40 + 1, 2**40 + 5]


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "xjoin_example.c"), "-o", os.path.join(td, "e.o")])

"""The self-join's C ABI (zh_self_join*): declared in the header, exported under SYMBOLS, zh_join_info's layout mirrored by ctypes, the sibling
info structs unchanged, the argument checks that are judged before any device is touched, and deduplicate_within's host rule.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN = ("zh_self_join", "zh_self_join_device", "zh_self_join_info")
FIELDS = ("rows_live", "pairs", "path", "redone", "candidates", "launches", "tiles")


def test_header_declares_the_self_join():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in JOIN:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_join_info" in h


def test_symbols_list_the_self_join():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in JOIN:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in JOIN:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.JoinInfo._fields_] == list(FIELDS)


def test_join_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_join_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_join_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.JoinInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_sibling_info_structs_are_unchanged():
    from zebra_amd import _ffi
    assert [f for f, _ in _ffi.ExactInfo._fields_] == ["batch", "rows_live", "path", "redone", "survivors", "launches"]
    assert [f for f, _ in _ffi.FilteredInfo._fields_] == ["batch", "rows_live", "rows_allowed", "path", "redone", "survivors", "launches",
                                                          "tiles_skipped"]
    assert [f for f, _ in _ffi.RangeInfo._fields_] == ["batch", "rows_live", "hits", "path", "redone", "candidates", "launches"]


def test_arguments_are_judged_before_any_device():
    """A null index, a null total, null arrays for a capacity and an unknown metric are refused by the first lines of either entry point.  The
    calls that pass a (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that stand-in and
    reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    a, b, keys, total = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 1)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(ix, metric, cap, ap, bp, kp, tp):
        return L.zh_self_join(ix, 2**64 - 1, metric, 0, cap, ap, bp, kp, tp)

    def dev(ix, metric, cap, ap, bp, kp, tp):
        return L.zh_self_join_device(ix, 2**64 - 1, metric, 0, cap, ap, bp, kp, tp, None)

    for call in (host, dev):
        assert call(None, 0, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 0, 4, P(a), P(b), P(keys), None) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 0, 0, None, None, None, None) == _ffi.ZH_EINVAL
        assert call(idx, 0, 4, None, P(b), P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 0, 4, P(a), None, P(keys), P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 0, 4, P(a), P(b), None, P(total)) == _ffi.ZH_EINVAL
        assert call(idx, 99, 4, P(a), P(b), P(keys), P(total)) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, 99, 0, None, None, None, P(total)) == _ffi.ZH_EINVAL
    info = _ffi.JoinInfo()
    assert L.zh_self_join_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_self_join_info(idx, None) == _ffi.ZH_EINVAL


def test_dedup_rule_keeps_the_ends_of_a_chain():
    """a ~ b, b ~ c, a !~ c: b goes (a is kept and paired with it), c stays (its only partner was removed)"""
    from zebra_amd.index import dedup_rule
    assert dedup_rule(np.array([0, 1], np.uint64), np.array([1, 2], np.uint64)).tolist() == [1]
    assert dedup_rule(np.array([], np.uint64), np.array([], np.uint64)).tolist() == []
    # a star: everything paired with 3 goes, and 7 ~ 9 no longer matters once 7 is gone
    assert dedup_rule(np.array([3, 3, 3, 7], np.uint64), np.array([5, 7, 8, 9], np.uint64)).tolist() == [5, 7, 8]

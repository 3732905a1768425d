"""The filtered exact search's C ABI (zh_search_exact_filtered_*): declared in the header, exported under SYMBOLS, zh_filtered_info's
layout mirrored by ctypes, and the argument checks that are judged before any device is touched.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERED = ("zh_search_exact_filtered_batch", "zh_search_exact_filtered_batch_device", "zh_search_filtered_info")
FIELDS = ("batch", "rows_live", "rows_allowed", "path", "redone", "survivors", "launches", "tiles_skipped")


def test_header_declares_the_filtered_search():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in FILTERED:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_filtered_info" in h


def test_symbols_list_the_filtered_search():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in FILTERED:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in FILTERED:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.FilteredInfo._fields_] == list(FIELDS)


def test_filtered_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_filtered_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_filtered_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.FilteredInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_exact_info_is_unchanged():
    from zebra_amd import _ffi
    assert [f for f, _ in _ffi.ExactInfo._fields_] == ["batch", "rows_live", "path", "redone", "survivors", "launches"]


def test_arguments_are_judged_before_any_device():
    """A null index, a null filter that speaks for rows, and top_k above ZH_MAX_TOPK are refused by the first lines of either entry point.  The
    calls that pass a (never dereferenced) stand-in for the index use an empty batch: were one of the checks lost, the call would return
    ZH_OK for b = 0 and fail its assertion here instead of reaching for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    q = (ctypes.c_float * 8)()
    words = (ctypes.c_uint32 * 4)()
    ids, keys, counts = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint32 * 4)()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def host(ix, b, k, filt, n_bits):
        return L.zh_search_exact_filtered_batch(ix, P(q), b, k, 0, 0, filt, n_bits, P(ids), P(keys), P(counts))

    def dev(ix, b, k, filt, n_bits):
        return L.zh_search_exact_filtered_batch_device(ix, P(q), b, k, 0, 0, filt, n_bits, P(ids), P(keys), P(counts), None)

    for call in (host, dev):
        assert call(None, 1, 1, P(words), 8) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 0, 1, None, 8) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()
        assert call(idx, 0, 1025, P(words), 8) == _ffi.ZH_ELIMIT
        assert call(idx, 0, 1025, None, 8) == _ffi.ZH_ELIMIT  # (top_k is judged with the other arguments of the exact search, the filter after)
        assert call(idx, 0, 1, None, 0) == _ffi.ZH_OK          # no filter words are needed for a filter that speaks for no row
    info = _ffi.FilteredInfo()
    assert L.zh_search_filtered_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_search_filtered_info(idx, None) == _ffi.ZH_EINVAL

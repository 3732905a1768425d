"""The k-NN graph refinement's C ABI (zh_knn_graph_refine*): declared in the header, exported under SYMBOLS, zh_knn_refine_info's layout mirrored by
ctypes, the sibling info structs unchanged, the argument checks that are judged before any device is touched, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFINE = ("zh_knn_graph_refine", "zh_knn_graph_refine_device", "zh_knn_graph_refine_info")
FIELDS = ("rows_live", "lines", "in_k", "k", "listed", "keyed", "updates", "launches")


def test_header_declares_the_refinement():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in REFINE:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_knn_refine_info" in h
    assert re.search(r"#define\s+ZH_REFINE_MAX_IN_K\s+64u", h)
    # the device form takes a stream as its last argument, like its siblings
    assert re.search(r"zh_knn_graph_refine_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    # the consequences of the definition the GPU tests use
    for phrase in ("never above that of the input line", "returns the exact graph's first k", "in_k + 1 live rows"):
        assert phrase in h, phrase


def test_symbols_list_the_refinement():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in REFINE:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in REFINE:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.KnnRefineInfo._fields_] == list(FIELDS)


def test_refine_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%%zu", sizeof(zh_knn_refine_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_knn_refine_info, %s));' % f for f in FIELDS)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.KnnRefineInfo
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
    """A null index, null inputs or outputs for a non-empty request, an unknown metric, the two limits and in_k = 0 are refused by the first
    lines of either entry point, in that order of kinds.  The calls that pass a (never dereferenced) stand-in for the index must fail: were a
    check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    gin, gcounts = (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()
    ids, keys, counts = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(ix, gi, gc, in_k, n, k, metric, ip, kp, cp):
        return L.zh_knn_graph_refine(ix, gi, gc, in_k, 0, n, k, metric, 0, ip, kp, cp)

    def dev(ix, gi, gc, in_k, n, k, metric, ip, kp, cp):
        return L.zh_knn_graph_refine_device(ix, gi, gc, in_k, 0, n, k, metric, 0, ip, kp, cp, None)

    G, C_, I, K, N = P(gin), P(gcounts), P(ids), P(keys), P(counts)
    for call in (host, dev):
        assert call(None, G, C_, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, G, C_, 4, 0, 4, 1, I, K, N) == _ffi.ZH_EINVAL  # (a null index is refused even for an empty request)
        assert call(idx, None, C_, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, G, None, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 2, 4, 1, None, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, G, C_, 4, 2, 4, 1, I, None, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 2, 4, 1, I, K, None) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 2, 0, 1, None, None, None) == _ffi.ZH_EINVAL  # k = 0 still writes the counts
        assert call(idx, None, None, 4, 2, 0, 1, None, None, N) == _ffi.ZH_EINVAL  # ... and the graph is still asked for
        assert call(idx, G, C_, 4, 2, 4, 99, I, K, N) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, None, None, 4, 0, 4, 99, None, None, None) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 2, 1024, 1, I, K, N) == _ffi.ZH_ELIMIT and b"ZH_MAX_TOPK" in L.zh_last_error()
        assert call(idx, None, None, 4, 0, 1024, 1, None, None, None) == _ffi.ZH_ELIMIT
        assert call(idx, G, C_, 65, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT and b"ZH_REFINE_MAX_IN_K" in L.zh_last_error()
        assert call(idx, None, None, 65, 0, 4, 1, None, None, None) == _ffi.ZH_ELIMIT
        assert call(idx, G, C_, 4, 2, 1024, 99, I, K, N) == _ffi.ZH_EINVAL  # the metric is judged before the limits
        assert call(idx, G, C_, 65, 2, 4, 99, I, K, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 0, 2, 1024, 1, I, K, N) == _ffi.ZH_ELIMIT  # ... and the limits before in_k = 0
        assert call(idx, G, C_, 0, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"in_k" in L.zh_last_error()
        assert call(idx, None, None, 64, 0, 1023, 1, None, None, None) == _ffi.ZH_OK  # an empty request: nothing to do, nothing touched
        assert call(idx, None, None, 0, 0, 0, 1, None, None, None) == _ffi.ZH_OK
    info = _ffi.KnnRefineInfo()
    assert L.zh_knn_graph_refine_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_knn_graph_refine_info(idx, None) == _ffi.ZH_EINVAL


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "knn_refine_example.c"), "-o", os.path.join(td, "e.o")])

"""The reverse-neighbour calls' C ABI (zh_knn_graph_reverse*, zh_knn_graph_refine_rev*): declared in the header, exported under SYMBOLS, both info
structs' layouts mirrored by ctypes, zh_knn_refine_info untouched, the argument checks that are judged before any device is touched, and the C
example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REVERSE = ("zh_knn_graph_reverse", "zh_knn_graph_reverse_device", "zh_knn_graph_reverse_info", "zh_knn_graph_refine_rev",
           "zh_knn_graph_refine_rev_device", "zh_knn_graph_refine_rev_info")
REVERSE_FIELDS = ("rows_live", "lines", "in_k", "rev_k", "edges", "kept", "max_degree", "launches")
REFINE_FIELDS = ("rows_live", "lines", "in_k", "k", "listed", "keyed", "updates", "launches")
FUSED_FIELDS = REFINE_FIELDS + ("rev_k", "edges", "kept", "max_degree")


def test_header_declares_the_reverse_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in REVERSE:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_knn_reverse_info" in h and "typedef struct zh_knn_refine_rev_info" in h
    for name in ("zh_knn_graph_reverse_device", "zh_knn_graph_refine_rev_device"):
        assert re.search(r"%s\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" % name, h), name
    # rev_k follows in_k in both pairs
    assert re.search(r"zh_knn_graph_reverse\s*\([^;]*size_t\s+in_k,\s*size_t\s+rev_k,\s*uint64_t\s+first_row", h)
    assert re.search(r"zh_knn_graph_refine_rev\s*\([^;]*size_t\s+in_k,\s*size_t\s+rev_k,\s*uint64_t\s+first_row", h)
    for phrase in ("0x9E3779B9", "0x85EBCA6B", "0xC2B2AE35", "0x92CA2F0E", "never above zh_knn_graph_refine's", "still returns its first k"):
        assert phrase in h, phrase


def test_symbols_list_the_reverse_calls():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in REVERSE:
        assert name in names, name
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.KnnReverseInfo._fields_] == list(REVERSE_FIELDS)
    assert [f for f, _ in _ffi.KnnRefineRevInfo._fields_] == list(FUSED_FIELDS)
    assert [f for f, _ in _ffi.KnnRefineInfo._fields_] == list(REFINE_FIELDS)  # (the existing getter's layout is not touched)


def test_info_layouts_match_the_header():
    from zebra_amd import _ffi
    structs = (("zh_knn_reverse_info", REVERSE_FIELDS, _ffi.KnnReverseInfo), ("zh_knn_refine_rev_info", FUSED_FIELDS, _ffi.KnnRefineRevInfo),
               ("zh_knn_refine_info", REFINE_FIELDS, _ffi.KnnRefineInfo))
    body = "\n".join('  printf("%%zu", sizeof(%s));\n%s\n  printf("\\n");' % (
        s, "\n".join('  printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in fields)) for s, fields, _ in structs)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s\n  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    for line, (_, fields, F) in zip(lines, structs):
        assert [int(x) for x in line.split()] == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in fields]
    # the fused info begins with zh_knn_refine_info, field for field
    assert all(getattr(_ffi.KnnRefineRevInfo, f).offset == getattr(_ffi.KnnRefineInfo, f).offset for f in REFINE_FIELDS)


def _stand_ins():
    fake = ctypes.create_string_buffer(64)
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731
    arrays = [(ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)(),
              (ctypes.c_uint32 * 2)()]
    return fake, arrays, ctypes.cast(fake, ctypes.c_void_p), [P(a) for a in arrays]


def test_reverse_arguments_are_judged_before_any_device():
    """A null index, null pointers of a non-empty request, the two limits, in_k = 0 and rev_k = 0, in that order of kinds.  The calls that pass a
    (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    keep, arrays, idx, (G, C_, I, _, N, D) = _stand_ins()

    def host(ix, gi, gc, in_k, rev_k, n, ip, cp, dp):
        return L.zh_knn_graph_reverse(ix, gi, gc, in_k, rev_k, 0, n, ip, cp, dp)

    def dev(ix, gi, gc, in_k, rev_k, n, ip, cp, dp):
        return L.zh_knn_graph_reverse_device(ix, gi, gc, in_k, rev_k, 0, n, ip, cp, dp, None)

    for call in (host, dev):
        assert call(None, G, C_, 4, 4, 2, I, N, D) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, G, C_, 4, 4, 0, I, N, D) == _ffi.ZH_EINVAL  # (a null index is refused even for an empty request)
        assert call(idx, None, C_, 4, 4, 2, I, N, D) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, G, None, 4, 4, 2, I, N, D) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, None, N, D) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, I, None, D) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, I, N, None) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, None, C_, 65, 4, 2, I, N, D) == _ffi.ZH_EINVAL  # the pointers are judged before the limits
        assert call(idx, G, C_, 65, 4, 2, I, N, D) == _ffi.ZH_ELIMIT and b"in_k" in L.zh_last_error()
        assert call(idx, G, C_, 4, 65, 2, I, N, D) == _ffi.ZH_ELIMIT and b"rev_k" in L.zh_last_error()
        assert call(idx, G, C_, 65, 65, 2, I, N, D) == _ffi.ZH_ELIMIT and b"in_k" in L.zh_last_error()  # in_k's limit first
        assert call(idx, None, None, 4, 65, 0, None, None, None) == _ffi.ZH_ELIMIT  # the limits hold for an empty request
        assert call(idx, G, C_, 0, 65, 2, I, N, D) == _ffi.ZH_ELIMIT  # ... and come before in_k = 0
        assert call(idx, G, C_, 65, 0, 2, I, N, D) == _ffi.ZH_ELIMIT
        assert call(idx, G, C_, 0, 4, 2, I, N, D) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()
        assert call(idx, G, C_, 4, 0, 2, I, N, D) == _ffi.ZH_EINVAL and b"rev_k is 0" in L.zh_last_error()
        assert call(idx, G, C_, 0, 0, 2, I, N, D) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()  # in_k before rev_k
        assert call(idx, None, None, 64, 64, 0, None, None, None) == _ffi.ZH_OK  # an empty request: nothing to do, nothing touched
        assert call(idx, None, None, 0, 0, 0, None, None, None) == _ffi.ZH_OK
    info = _ffi.KnnReverseInfo()
    assert L.zh_knn_graph_reverse_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_knn_graph_reverse_info(idx, None) == _ffi.ZH_EINVAL
    del keep, arrays


def test_fused_arguments_are_judged_before_any_device():
    """zh_knn_graph_refine's order of kinds -- null index, null pointers, the metric, k's limit, in_k's limit -- then in_k + rev_k, then in_k = 0;
    rev_k = 0 is no error"""
    from zebra_amd import _ffi
    L = _ffi.lib()
    keep, arrays, idx, (G, C_, I, K, N, _) = _stand_ins()

    def host(ix, gi, gc, in_k, rev_k, n, k, metric, ip, kp, cp):
        return L.zh_knn_graph_refine_rev(ix, gi, gc, in_k, rev_k, 0, n, k, metric, 0, ip, kp, cp)

    def dev(ix, gi, gc, in_k, rev_k, n, k, metric, ip, kp, cp):
        return L.zh_knn_graph_refine_rev_device(ix, gi, gc, in_k, rev_k, 0, n, k, metric, 0, ip, kp, cp, None)

    for call in (host, dev):
        assert call(None, G, C_, 4, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, G, C_, 4, 4, 0, 4, 1, I, K, N) == _ffi.ZH_EINVAL
        assert call(idx, None, C_, 4, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, G, None, 4, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, 4, 1, None, K, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, 4, 1, I, None, N) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, 4, 1, I, K, None) == _ffi.ZH_EINVAL
        assert call(idx, G, C_, 4, 4, 2, 4, 99, I, K, N) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, G, C_, 33, 32, 2, 4, 99, I, K, N) == _ffi.ZH_EINVAL  # ... judged before the limits
        assert call(idx, G, C_, 4, 4, 2, 1024, 1, I, K, N) == _ffi.ZH_ELIMIT and b"ZH_MAX_TOPK" in L.zh_last_error()
        assert call(idx, G, C_, 33, 32, 2, 1024, 1, I, K, N) == _ffi.ZH_ELIMIT and b"ZH_MAX_TOPK" in L.zh_last_error()  # k's limit first
        assert call(idx, G, C_, 65, 0, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT and b"in_k 65 >" in L.zh_last_error()
        assert call(idx, G, C_, 33, 32, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT and b"in_k 33 + rev_k 32" in L.zh_last_error()  # in_k + rev_k = 65
        assert call(idx, G, C_, 1, 64, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT and b"+ rev_k" in L.zh_last_error()
        assert call(idx, G, C_, 64, 1, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT
        assert call(idx, None, None, 33, 32, 0, 4, 1, None, None, None) == _ffi.ZH_ELIMIT  # the limits hold for an empty request
        assert call(idx, G, C_, 0, 65, 2, 4, 1, I, K, N) == _ffi.ZH_ELIMIT  # the limit of the sum comes before in_k = 0
        assert call(idx, G, C_, 0, 4, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()
        assert call(idx, G, C_, 0, 0, 2, 4, 1, I, K, N) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()
        assert call(idx, None, None, 32, 32, 0, 1023, 1, None, None, None) == _ffi.ZH_OK  # an empty request: nothing to do, nothing touched
        assert call(idx, None, None, 64, 0, 0, 4, 1, None, None, None) == _ffi.ZH_OK
        assert call(idx, None, None, 0, 64, 0, 4, 1, None, None, None) == _ffi.ZH_OK
    info = _ffi.KnnRefineRevInfo()
    assert L.zh_knn_graph_refine_rev_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_knn_graph_refine_rev_info(idx, None) == _ffi.ZH_EINVAL
    del keep, arrays


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "knn_reverse_example.c"), "-o", os.path.join(td, "e.o")])

"""k-NN graph pruning's C ABI (zh_knn_graph_prune*, zh_knn_graph_prune_info): declared in the header, exported under SYMBOLS, the info struct's
layout mirrored by ctypes, the argument checks that are judged before any device is touched -- refine_rev_args' kinds in its order, `degree`
where k stands and `fill` last -- and the C example.  first_row + n past the stored rows and degree = 0 need a real index:
tests/test_gpu_prune.py.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("zh_knn_graph_prune", "zh_knn_graph_prune_device", "zh_knn_graph_prune_info")
FIELDS = ("rows_live", "lines", "in_k", "rev_k", "degree", "fill", "candidates", "kept", "occluded", "filled", "cut", "keyed", "launches")


def test_header_declares_the_prune_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in CALLS:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_knn_prune_info" in h
    assert re.search(r"zh_knn_graph_prune_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    for name, pre in (("zh_knn_graph_prune", ""), ("zh_knn_graph_prune_device", "d_")):
        assert re.search(name + r"\s*\(zh_index\s*\*\s*idx,\s*const\s+uint64_t\s*\*\s*" + pre + r"in_ids,\s*const\s+uint32_t\s*\*\s*" + pre +
                         r"in_counts,\s*size_t\s+in_k,\s*size_t\s+rev_k,\s*uint64_t\s+first_row,\s*uint64_t\s+n,\s*size_t\s+degree,\s*int\s+fill,\s*"
                         r"int\s+metric,\s*int\s+cosine_mode,\s*uint64_t\s*\*\s*" + pre + r"out_ids,\s*uint64_t\s*\*\s*" + pre +
                         r"out_keys,\s*uint32_t\s*\*\s*" + pre + "out_counts", h), name
    head = h[:h.index("Conventions")]
    assert "zh_knn_graph_prune[_device]" in head
    block = h[h.index("k-NN graph pruning (new)"):h.index("typedef struct zh_knn_prune_info")]
    for said in ("c_1 is always kept", "idempotent", "never occlude each other", "occludes the rest", "ZH_COSINE_PARITY", "unsigned"):
        assert said in block, said


def test_symbols_list_the_prune_calls():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert name in names, name
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.KnnPruneInfo._fields_] == list(FIELDS)


def test_info_layout_matches_the_header():
    from zebra_amd import _ffi
    body = '  printf("%zu", sizeof(zh_knn_prune_info));\n'
    body += "\n".join('  printf(" %%zu", offsetof(zh_knn_prune_info, %s));' % f for f in FIELDS) + '\n  printf("\\n");\n'
    body += '  printf("%zu %zu\\n", sizeof(zh_knn_refine_info), sizeof(zh_knn_refine_rev_info));\n'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    F = _ffi.KnnPruneInfo
    assert lines[0] == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] == [104] + list(range(0, 104, 8))
    assert lines[1] == [ctypes.sizeof(_ffi.KnnRefineInfo), ctypes.sizeof(_ffi.KnnRefineRevInfo)]  # (the siblings keep theirs)
    info = F()
    info.cut = 7
    assert info.as_dict() == dict.fromkeys(FIELDS, 0) | {"cut": 7}


def test_arguments_are_judged_before_any_device():
    """The stated order: null index (even for n = 0), null pointers of a request with n > 0, the metric, degree > 64, in_k > 64, in_k + rev_k >
    64 (all ZH_ELIMIT), in_k = 0 with n > 0, a fill other than 0 or 1 (ZH_EINVAL), and n = 0 is ZH_OK.  The calls that pass a (never
    dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()]
    G, C, I, K, N = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]

    def host(ix, g, c, in_k, rev_k, n, degree, fill, metric, ip, kp, cp):
        return L.zh_knn_graph_prune(ix, g, c, in_k, rev_k, 0, n, degree, fill, metric, 0, ip, kp, cp)

    def dev(ix, g, c, in_k, rev_k, n, degree, fill, metric, ip, kp, cp):
        return L.zh_knn_graph_prune_device(ix, g, c, in_k, rev_k, 0, n, degree, fill, metric, 0, ip, kp, cp, None)

    E, LIM = _ffi.ZH_EINVAL, _ffi.ZH_ELIMIT
    for call in (host, dev):
        err = lambda: L.zh_last_error()  # noqa: E731
        # 1: the null index, whatever else is wrong, even for n = 0
        assert call(None, G, C, 4, 0, 1, 4, 0, 1, I, K, N) == E and b"null" in err()
        assert call(None, G, C, 4, 0, 0, 4, 0, 1, I, K, N) == E and b"null" in err()
        assert call(None, G, C, 99, 99, 0, 99, 7, 99, I, K, N) == E and b"null" in err()
        # 2: null pointers of a request with n > 0, ahead of the metric and every limit
        for at in range(5):
            ptrs = [G, C, I, K, N]
            ptrs[at] = None
            assert call(idx, ptrs[0], ptrs[1], 4, 0, 1, 4, 0, 1, *ptrs[2:]) == E and b"null" in err(), at
            assert call(idx, ptrs[0], ptrs[1], 99, 99, 1, 99, 7, 99, *ptrs[2:]) == E and b"null" in err(), at
        # 3: the metric, ahead of the limits
        assert call(idx, G, C, 4, 0, 1, 4, 0, 99, I, K, N) == E and b"metric" in err()
        assert call(idx, G, C, 99, 99, 1, 99, 7, 99, I, K, N) == E and b"metric" in err()
        assert call(idx, None, None, 99, 99, 0, 99, 7, 99, None, None, None) == E and b"metric" in err()  # (for n = 0 too)
        # 4 .. 6: the limits, degree's first
        assert call(idx, G, C, 4, 0, 1, 65, 0, 1, I, K, N) == LIM and b"degree 65 >" in err()
        assert call(idx, G, C, 65, 65, 1, 65, 7, 1, I, K, N) == LIM and b"degree 65 >" in err()
        assert call(idx, G, C, 65, 0, 1, 64, 0, 1, I, K, N) == LIM and b"in_k 65 >" in err()
        assert call(idx, G, C, 65, 65, 1, 64, 7, 1, I, K, N) == LIM and b"in_k 65 >" in err()
        assert call(idx, G, C, 33, 32, 1, 64, 0, 1, I, K, N) == LIM and b"in_k 33 + rev_k 32 >" in err()
        assert call(idx, G, C, 0, 65, 1, 64, 7, 1, I, K, N) == LIM and b"rev_k 65 >" in err()  # (ahead of in_k = 0 and of fill)
        assert call(idx, None, None, 4, 0, 0, 65, 0, 1, None, None, None) == LIM  # (an empty request is judged alike)
        # 7: in_k = 0 with n > 0, ahead of fill
        assert call(idx, G, C, 0, 0, 1, 4, 0, 1, I, K, N) == E and b"in_k is 0" in err()
        assert call(idx, G, C, 0, 8, 1, 4, 7, 1, I, K, N) == E and b"in_k is 0" in err()
        # 8: fill
        for fill in (2, -1, 2**31 - 1, -2**31):
            assert call(idx, G, C, 4, 0, 1, 4, fill, 1, I, K, N) == E and b"fill" in err(), fill
            assert call(idx, None, None, 4, 0, 0, 4, fill, 1, None, None, None) == E and b"fill" in err(), fill  # (before n = 0 is ZH_OK)
        # 10: n = 0 with good scalars, nulls and all; in_k = 0 is no fault of an empty request
        for fill in (0, 1):
            assert call(idx, None, None, 4, 0, 0, 4, fill, 1, None, None, None) == _ffi.ZH_OK
            assert call(idx, None, None, 0, 0, 0, 0, fill, 1, None, None, None) == _ffi.ZH_OK
            assert call(idx, G, C, 32, 32, 0, 64, fill, 1, I, K, N) == _ffi.ZH_OK
    del fake, arrays


def test_null_info_pointers():
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    s = _ffi.KnnPruneInfo()
    assert L.zh_knn_graph_prune_info(None, ctypes.byref(s)) == _ffi.ZH_EINVAL
    assert L.zh_knn_graph_prune_info(idx, None) == _ffi.ZH_EINVAL
    del fake


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "graph_prune_example.c"), "-o", os.path.join(td, "e.o")])

"""NN-descent's C ABI (zh_knn_graph_descent*): declared in the header, exported under SYMBOLS, the info struct's layout mirrored by ctypes, the
argument checks that are judged before any device is touched -- their order and the limits -- a null index, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCENT = ("zh_knn_graph_descent", "zh_knn_graph_descent_device", "zh_knn_graph_descent_info")
FIELDS = ("rows_live", "in_k", "rev_k", "k", "rounds", "rounds_run", "launches", "listed", "keyed", "lines_active", "updates", "large_lines",
          "keyed_round", "updates_round", "active_round")


def test_header_declares_the_descent_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in DESCENT:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_knn_descent_info" in h and "#define ZH_DESCENT_MAX_ROUNDS 32u" in h
    assert re.search(r"zh_knn_graph_descent_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" , h)
    assert re.search(r"zh_knn_graph_descent\s*\([^;]*size_t\s+in_k,\s*size_t\s+rev_k,\s*size_t\s+k,\s*size_t\s+rounds,\s*int\s+metric", h)
    for f in ("keyed_round", "updates_round", "active_round"):
        assert re.search(r"uint64_t\s+%s\[32\];" % f, h), f


def test_symbols_list_the_descent_calls():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in DESCENT:
        assert name in names, name
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.KnnDescentInfo._fields_] == list(FIELDS)


def test_info_layout_matches_the_header():
    from zebra_amd import _ffi
    body = '  printf("%zu", sizeof(zh_knn_descent_info));\n' + "\n".join(
        '  printf(" %%zu", offsetof(zh_knn_descent_info, %s));' % f for f in FIELDS) + '\n  printf(" %zu\\n", sizeof(((zh_knn_descent_info *)0)->keyed_round));'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s\n  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.KnnDescentInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] + [32 * 8]
    info = F()
    info.rounds_run = 3
    info.keyed_round[2] = 7
    d = info.as_dict()
    assert d["keyed_round"] == [0, 0, 7] and d["updates_round"] == [0, 0, 0] and d["active_round"] == [0, 0, 0] and d["rounds_run"] == 3


def test_descent_arguments_are_judged_before_any_device():
    """A null index, null pointers, the metric, the rounds, k = 0, then the limits (in_k, in_k + rev_k, k + rev_k), then in_k = 0.  The calls that pass
    a (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()]
    G, C_, I, K, N = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]

    def host(ix, gi, gc, in_k, rev_k, k, rounds, metric, ip, kp, cp):
        return L.zh_knn_graph_descent(ix, gi, gc, in_k, rev_k, k, rounds, metric, 0, ip, kp, cp)

    def dev(ix, gi, gc, in_k, rev_k, k, rounds, metric, ip, kp, cp):
        return L.zh_knn_graph_descent_device(ix, gi, gc, in_k, rev_k, k, rounds, metric, 0, ip, kp, cp, None)

    for call in (host, dev):
        assert call(None, G, C_, 4, 4, 4, 2, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        for at in range(5):
            ptrs = [G, C_, I, K, N]
            ptrs[at] = None
            assert call(idx, ptrs[0], ptrs[1], 4, 4, 4, 2, 1, *ptrs[2:]) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error(), at
        assert call(idx, None, C_, 65, 4, 4, 2, 1, I, K, N) == _ffi.ZH_EINVAL  # the pointers are judged before the limits
        assert call(idx, G, C_, 4, 4, 4, 2, 99, I, K, N) == _ffi.ZH_EINVAL  # no such metric
        assert call(idx, G, C_, 65, 4, 4, 2, 99, I, K, N) == _ffi.ZH_EINVAL  # ... judged before the limits
        assert call(idx, G, C_, 4, 4, 4, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"rounds" in L.zh_last_error()
        assert call(idx, G, C_, 4, 4, 4, 33, 1, I, K, N) == _ffi.ZH_EINVAL and b"rounds 33" in L.zh_last_error()
        assert call(idx, G, C_, 65, 4, 0, 33, 1, I, K, N) == _ffi.ZH_EINVAL and b"rounds" in L.zh_last_error()  # the rounds first
        assert call(idx, G, C_, 4, 4, 0, 2, 1, I, K, N) == _ffi.ZH_EINVAL and b"k is 0" in L.zh_last_error()
        assert call(idx, G, C_, 65, 4, 0, 2, 1, I, K, N) == _ffi.ZH_EINVAL and b"k is 0" in L.zh_last_error()  # k = 0 before the limits
        assert call(idx, G, C_, 65, 0, 4, 2, 1, I, K, N) == _ffi.ZH_ELIMIT and b"in_k 65 >" in L.zh_last_error()
        assert call(idx, G, C_, 33, 32, 4, 2, 1, I, K, N) == _ffi.ZH_ELIMIT and b"in_k 33 + rev_k 32" in L.zh_last_error()
        assert call(idx, G, C_, 4, 32, 33, 2, 1, I, K, N) == _ffi.ZH_ELIMIT and b"k 33 + rev_k 32" in L.zh_last_error()
        assert call(idx, G, C_, 4, 0, 65, 2, 1, I, K, N) == _ffi.ZH_ELIMIT and b"k 65 + rev_k 0" in L.zh_last_error()
        assert call(idx, G, C_, 33, 32, 33, 2, 1, I, K, N) == _ffi.ZH_ELIMIT and b"in_k 33 + rev_k" in L.zh_last_error()  # in_k's sum first
        assert call(idx, G, C_, 0, 65, 4, 2, 1, I, K, N) == _ffi.ZH_ELIMIT  # the limits come before in_k = 0
        assert call(idx, G, C_, 0, 4, 4, 2, 1, I, K, N) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()
        assert call(idx, G, C_, 0, 4, 4, 1, 1, I, K, N) == _ffi.ZH_EINVAL and b"in_k is 0" in L.zh_last_error()
    info = _ffi.KnnDescentInfo()
    assert L.zh_knn_graph_descent_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_knn_graph_descent_info(idx, None) == _ffi.ZH_EINVAL
    del fake, arrays


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "knn_descent_example.c"), "-o", os.path.join(td, "e.o")])

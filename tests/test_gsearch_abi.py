"""Graph search's C ABI (zh_index_set_graph*, zh_index_drop_graph, zh_index_graph_info, zh_search_graph_batch*, zh_search_graph_info): declared in
the header, exported under SYMBOLS, both info structs' layout mirrored by ctypes, the argument checks that are judged before any device is touched
-- their order and the limits -- a null index, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("zh_index_set_graph", "zh_index_set_graph_device", "zh_index_drop_graph", "zh_index_graph_info", "zh_search_graph_batch",
         "zh_search_graph_batch_device", "zh_search_graph_info")
GRAPH_FIELDS = ("attached", "g_k", "g_rows", "bytes")
SEARCH_FIELDS = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches")


def test_header_declares_the_graph_search_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in CALLS:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_graph_info" in h and "typedef struct zh_graph_search_info" in h
    for define in ("#define ZH_GRAPH_MAX_BEAM 256u", "#define ZH_GRAPH_MAX_SEEDS 64u", "#define ZH_GRAPH_MAX_ITERS 65535u", "#define ZH_GRAPH_BATCH 16384u"):
        assert define in h, define
    assert re.search(r"zh_search_graph_batch_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"zh_index_set_graph_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"zh_search_graph_batch\s*\([^;]*size_t\s+b,\s*const\s+uint64_t\s*\*\s*seeds,\s*size_t\s+n_seed,\s*size_t\s+top_k,\s*size_t\s+beam,\s*"
                     r"size_t\s+width,\s*size_t\s+max_iters,\s*int\s+metric", h)
    # a line each in the header's index of calls
    head = h[:h.index("Conventions")]
    assert "zh_index_set_graph[_device]" in head and "zh_search_graph_batch[_device]" in head


def test_symbols_list_the_graph_search_calls():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert name in names, name
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.GraphInfo._fields_] == list(GRAPH_FIELDS)
    assert [f for f, _ in _ffi.SearchGraphInfo._fields_] == list(SEARCH_FIELDS)
    assert (_ffi.GRAPH_MAX_BEAM, _ffi.GRAPH_MAX_SEEDS, _ffi.GRAPH_MAX_ITERS, _ffi.GRAPH_BATCH) == (256, 64, 65535, 16384)


def test_info_layouts_match_the_header():
    from zebra_amd import _ffi
    body = ""
    for struct, fields in (("zh_graph_info", GRAPH_FIELDS), ("zh_graph_search_info", SEARCH_FIELDS)):
        body += '  printf("%%zu", sizeof(%s));\n' % struct
        body += "\n".join('  printf(" %%zu", offsetof(%s, %s));' % (struct, f) for f in fields) + '\n  printf("\\n");\n'
    body += '  printf("%u %u %u %u\\n", ZH_GRAPH_MAX_BEAM, ZH_GRAPH_MAX_SEEDS, ZH_GRAPH_MAX_ITERS, ZH_GRAPH_BATCH);\n'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    for got, F, fields in ((lines[0], _ffi.GraphInfo, GRAPH_FIELDS), (lines[1], _ffi.SearchGraphInfo, SEARCH_FIELDS)):
        assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in fields]
    assert lines[2] == [256, 64, 65535, 16384]
    info = _ffi.SearchGraphInfo()
    info.keyed = 7
    assert info.as_dict() == dict.fromkeys(SEARCH_FIELDS, 0) | {"keyed": 7}
    assert _ffi.GraphInfo().as_dict() == dict.fromkeys(GRAPH_FIELDS, 0)


def test_search_arguments_are_judged_before_any_device():
    """A null index, null pointers of a request with b > 0, the metric, a zero top_k / beam / width / n_seed, then the limits (beam, top_k against
    beam, n_seed, width, max_iters).  The calls that pass a (never dereferenced) stand-in for the index must fail: were a check lost, the call
    would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_float * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()]
    Q, S, I, K, N = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]

    def host(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, ip, kp, cp):
        return L.zh_search_graph_batch(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, 0, ip, kp, cp)

    def dev(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, ip, kp, cp):
        return L.zh_search_graph_batch_device(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, 0, ip, kp, cp, None)

    for call in (host, dev):
        assert call(None, Q, 1, S, 4, 4, 8, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, Q, 0, S, 4, 4, 8, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL  # (even for an empty batch)
        for at in range(5):
            ptrs = [Q, S, I, K, N]
            ptrs[at] = None
            assert call(idx, ptrs[0], 1, ptrs[1], 4, 4, 8, 1, 0, 1, *ptrs[2:]) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error(), at
        assert call(idx, None, 1, S, 4, 4, 999, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL  # the pointers are judged before the limits
        assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 99, I, K, N) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 4, 999, 1, 0, 99, I, K, N) == _ffi.ZH_EINVAL  # ... and so is the metric
        assert call(idx, Q, 1, S, 4, 0, 999, 1, 0, 99, I, K, N) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()  # ... before the zeros too
        assert call(idx, Q, 1, S, 4, 0, 8, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"top_k is 0" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 4, 0, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"beam is 0" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 4, 8, 0, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"width is 0" in L.zh_last_error()
        assert call(idx, Q, 1, S, 0, 4, 8, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"n_seed is 0" in L.zh_last_error()
        assert call(idx, Q, 1, S, 0, 4, 999, 1, 0, 1, I, K, N) == _ffi.ZH_EINVAL and b"n_seed is 0" in L.zh_last_error()  # the zeros before the limits
        assert call(idx, Q, 1, S, 4, 4, 257, 1, 0, 1, I, K, N) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 9, 8, 1, 0, 1, I, K, N) == _ffi.ZH_ELIMIT and b"top_k 9 > beam 8" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 300, 257, 1, 0, 1, I, K, N) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()  # the beam's limit first
        assert call(idx, Q, 1, S, 65, 4, 8, 1, 0, 1, I, K, N) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 4, 8, 257, 0, 1, I, K, N) == _ffi.ZH_ELIMIT and b"width 257 >" in L.zh_last_error()
        assert call(idx, Q, 1, S, 4, 4, 8, 1, 65536, 1, I, K, N) == _ffi.ZH_ELIMIT and b"max_iters 65536 >" in L.zh_last_error()
        assert call(idx, Q, 1, S, 65, 4, 8, 257, 65536, 1, I, K, N) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()  # in the documented order
        assert call(idx, Q, 0, S, 4, 4, 257, 1, 0, 1, I, K, N) == _ffi.ZH_ELIMIT  # (an empty batch is judged alike ...)
    del fake, arrays


def test_attach_arguments_are_judged_before_any_device():
    """A null index, null arrays of a non-empty graph, g_k = 0, g_k past ZH_REFINE_MAX_IN_K"""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()]
    G, C_ = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]
    for call in (lambda *a: L.zh_index_set_graph(*a), lambda *a: L.zh_index_set_graph_device(*a, None)):
        assert call(None, G, C_, 2, 4) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, G, C_, 0, 4) == _ffi.ZH_EINVAL
        assert call(idx, None, C_, 2, 4) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, G, None, 2, 4) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, None, C_, 2, 65) == _ffi.ZH_EINVAL  # the pointers before the limit
        assert call(idx, G, C_, 2, 0) == _ffi.ZH_EINVAL and b"g_k is 0" in L.zh_last_error()
        assert call(idx, None, None, 0, 0) == _ffi.ZH_EINVAL and b"g_k is 0" in L.zh_last_error()  # (an empty graph needs no arrays, but a width)
        assert call(idx, G, C_, 2, 65) == _ffi.ZH_ELIMIT and b"g_k 65 >" in L.zh_last_error()
    del fake, arrays


def test_null_info_pointers():
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    g, s = _ffi.GraphInfo(), _ffi.SearchGraphInfo()
    assert L.zh_index_graph_info(None, ctypes.byref(g)) == _ffi.ZH_EINVAL
    assert L.zh_index_graph_info(idx, None) == _ffi.ZH_EINVAL
    assert L.zh_search_graph_info(None, ctypes.byref(s)) == _ffi.ZH_EINVAL
    assert L.zh_search_graph_info(idx, None) == _ffi.ZH_EINVAL
    assert L.zh_index_drop_graph(None) == _ffi.ZH_EINVAL
    del fake


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "graph_search_example.c"), "-o", os.path.join(td, "e.o")])

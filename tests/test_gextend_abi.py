"""The graph extension's C ABI (zh_index_extend_graph*, zh_index_extend_graph_info, zh_index_get_graph*): declared in the header, exported under
SYMBOLS, the info struct's layout mirrored by ctypes, the argument checks that are judged before any device is touched -- their order and the
limits -- a null index, and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("zh_index_extend_graph", "zh_index_extend_graph_device", "zh_index_extend_graph_info", "zh_index_get_graph", "zh_index_get_graph_device")
FIELDS = ("rows_added", "rows_removed", "chunks", "seeds", "iterations", "expanded", "keyed", "capped", "reverse_rows", "reverse_offered",
          "reverse_kept", "launches")


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in CALLS:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_graph_extend_info" in h and "#define ZH_GRAPH_EXTEND_MAX_BATCH 1024u" in h
    assert re.search(r"zh_index_extend_graph_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"zh_index_get_graph_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    assert re.search(r"zh_index_extend_graph\s*\([^;]*const\s+uint64_t\s*\*\s*seeds,\s*uint64_t\s+n_new,\s*size_t\s+n_seed,\s*size_t\s+beam,\s*size_t\s+width,\s*"
                     r"size_t\s+max_iters,\s*size_t\s+batch,\s*int\s+metric", h)
    head = h[:h.index("Conventions")]  # a line each in the header's index of calls
    assert "zh_index_extend_graph[_device]" in head and "zh_index_get_graph[_device]" in head


def test_symbols_list_the_calls():
    from zebra_amd import _ffi
    from tests import gextend_cases as ge
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert name in names and hasattr(lib, name), name
    assert [f for f, _ in _ffi.GraphExtendInfo._fields_] == list(FIELDS) == list(ge.INFO_FIELDS)
    assert _ffi.GRAPH_EXTEND_MAX_BATCH == ge.MAX_BATCH == 1024


def test_info_layout_matches_the_header():
    from zebra_amd import _ffi
    body = '  printf("%zu", sizeof(zh_graph_extend_info));\n'
    body += "\n".join('  printf(" %%zu", offsetof(zh_graph_extend_info, %s));' % f for f in FIELDS) + '\n  printf("\\n%u\\n", ZH_GRAPH_EXTEND_MAX_BATCH);\n'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    F = _ffi.GraphExtendInfo
    assert lines[0] == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]
    assert lines[1] == [1024]
    info = F()
    info.reverse_kept = 7
    assert info.as_dict() == dict.fromkeys(FIELDS, 0) | {"reverse_kept": 7}


def test_extend_arguments_are_judged_before_any_device():
    """A null index, null seeds of new rows, the metric, a zero beam / width / n_seed / batch, then the limits (beam, n_seed, width, max_iters,
    batch).  The calls that pass a (never dereferenced) stand-in for the index must fail: were a check lost, the call would go on to lock that
    stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arr = (ctypes.c_uint64 * 8)()
    S = ctypes.cast(arr, ctypes.c_void_p)

    def host(ix, s, n_new, n_seed, beam, width, max_iters, batch, metric):
        return L.zh_index_extend_graph(ix, s, n_new, n_seed, beam, width, max_iters, batch, metric, 0)

    def dev(ix, s, n_new, n_seed, beam, width, max_iters, batch, metric):
        return L.zh_index_extend_graph_device(ix, s, n_new, n_seed, beam, width, max_iters, batch, metric, 0, None)

    for call in (host, dev):
        assert call(None, S, 2, 4, 8, 1, 0, 64, 1) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, None, 0, 4, 8, 1, 0, 64, 1) == _ffi.ZH_EINVAL  # (even with nothing new)
        assert call(idx, None, 2, 4, 8, 1, 0, 64, 1) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, None, 2, 4, 999, 1, 0, 64, 99) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()  # the pointer before metric and limits
        assert call(idx, S, 2, 4, 8, 1, 0, 64, 99) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()
        assert call(idx, S, 2, 4, 0, 1, 0, 64, 99) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()  # ... before the zeros
        assert call(idx, S, 2, 4, 0, 1, 0, 64, 1) == _ffi.ZH_EINVAL and b"beam is 0" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 0, 0, 64, 1) == _ffi.ZH_EINVAL and b"width is 0" in L.zh_last_error()
        assert call(idx, S, 2, 0, 8, 1, 0, 64, 1) == _ffi.ZH_EINVAL and b"n_seed is 0" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 1, 0, 0, 1) == _ffi.ZH_EINVAL and b"batch is 0" in L.zh_last_error()
        assert call(idx, S, 2, 4, 999, 1, 0, 0, 1) == _ffi.ZH_EINVAL and b"batch is 0" in L.zh_last_error()  # the zeros before the limits
        assert call(idx, S, 2, 4, 0, 0, 0, 0, 1) == _ffi.ZH_EINVAL and b"beam is 0" in L.zh_last_error()  # ... in their order
        assert call(idx, S, 2, 4, 257, 1, 0, 64, 1) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()
        assert call(idx, S, 2, 65, 8, 1, 0, 64, 1) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 257, 0, 64, 1) == _ffi.ZH_ELIMIT and b"width 257 >" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 1, 65536, 64, 1) == _ffi.ZH_ELIMIT and b"max_iters 65536 >" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 1, 0, 1025, 1) == _ffi.ZH_ELIMIT and b"batch 1025 >" in L.zh_last_error()
        assert call(idx, S, 2, 65, 257, 257, 65536, 1025, 1) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()  # in the documented order
        assert call(idx, S, 2, 65, 8, 257, 65536, 1025, 1) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 257, 65536, 1025, 1) == _ffi.ZH_ELIMIT and b"width 257 >" in L.zh_last_error()
        assert call(idx, S, 2, 4, 8, 1, 65536, 1025, 1) == _ffi.ZH_ELIMIT and b"max_iters 65536 >" in L.zh_last_error()
        assert call(idx, None, 0, 4, 8, 1, 0, 1025, 1) == _ffi.ZH_ELIMIT  # (nothing new is judged alike)
    del fake, arr


def test_read_arguments_and_null_info_pointers():
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)()]
    I, N = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]
    for call in (lambda *a: L.zh_index_get_graph(*a), lambda *a: L.zh_index_get_graph_device(*a, None)):
        assert call(None, 0, 2, I, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, 0, 0, I, N) == _ffi.ZH_EINVAL
        assert call(idx, 0, 2, None, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(idx, 0, 2, I, None) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
    e = _ffi.GraphExtendInfo()
    assert L.zh_index_extend_graph_info(None, ctypes.byref(e)) == _ffi.ZH_EINVAL
    assert L.zh_index_extend_graph_info(idx, None) == _ffi.ZH_EINVAL
    del fake, arrays


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "graph_extend_example.c"), "-o", os.path.join(td, "e.o")])

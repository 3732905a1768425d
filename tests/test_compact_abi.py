"""The compaction's C ABI (zh_index_compact, zh_index_stored_rows): declared in the header, exported by the library, listed under SYMBOLS, and
zh_compact_info's layout mirrored by ctypes.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("rows_before", "rows_after", "rows_moved", "bytes_moved", "scratch_bytes", "capacity_rows", "copy_bytes_released", "ms")


def test_header_declares_compaction():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    assert re.search(r"ZH_API\s+int\s+zh_index_compact\s*\(\s*zh_index\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*zh_compact_info\s*\*\s*\w+\s*\)", h)
    assert re.search(r"ZH_API\s+uint64_t\s+zh_index_stored_rows\s*\(", h)
    assert "typedef struct zh_compact_info" in h
    assert "ZH_COMPACT_BOUNCE_BYTES" in h and "ZH_COMPACT_CHUNK_ROWS" in h  # the scratch bound and the test hook are stated


def test_library_exports_compaction():
    from zebra_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "zh_index_compact") and hasattr(lib, "zh_index_stored_rows")


def test_symbols_list_compaction():
    from zebra_amd import _ffi
    sym = {n: (r, a) for n, r, a in _ffi.SYMBOLS}
    assert sym["zh_index_compact"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
    assert sym["zh_index_stored_rows"] == (ctypes.c_uint64, [ctypes.c_void_p])
    assert [f for f, _ in _ffi.CompactInfo._fields_] == list(FIELDS)


def test_compact_info_layout_matches_header():
    from zebra_amd import _ffi
    offs = ", ".join("offsetof(zh_compact_info, %s)" % f for f in FIELDS)
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  size_t v[] = { sizeof(zh_compact_info), %s, (size_t)ZH_COMPACT_BOUNCE_BYTES };
  for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);
  printf("\n");
  return 0; }''' % offs
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    E = _ffi.CompactInfo
    assert got == [ctypes.sizeof(E)] + [getattr(E, f).offset for f in FIELDS] + [_ffi.COMPACT_BOUNCE_BYTES]


def test_wrappers_and_docs_name_compaction():
    """every layer the ABI is bound in: the Python and C++ wrappers, the Rust shim, the integration guide, the knob's entry in DESIGN.md"""
    import zebra_amd
    assert callable(zebra_amd.LSHIndex.compact) and callable(zebra_amd.Database.compact)
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    assert "zh_index_compact" in read("include", "zebra.hpp")
    rs = read("rust", "zebra-hip", "src", "lib.rs")
    assert "pub fn zh_index_compact" in rs and "pub struct zh_compact_info" in rs and "pub fn compact" in rs
    assert "pub fn zh_index_compact" in read("INTEGRATION.md")
    assert "ZH_COMPACT_CHUNK_ROWS" in read("DESIGN.md")

"""The exact search's C ABI (zh_search_exact_*): declared in the header, exported under SYMBOLS, and zh_exact_info's layout mirrored
by ctypes.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("zh_search_exact_batch", "zh_search_exact_batch_device", "zh_search_exact_info")


def test_header_declares_the_exact_search():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in EXACT:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_exact_info" in h


def test_symbols_list_the_exact_search():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in EXACT:
        assert name in names, name


def test_exact_info_layout_matches_header():
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(zh_exact_info), offsetof(zh_exact_info, batch), offsetof(zh_exact_info, rows_live),
         offsetof(zh_exact_info, path), offsetof(zh_exact_info, redone), offsetof(zh_exact_info, survivors), offsetof(zh_exact_info, launches));
  return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    E = _ffi.ExactInfo
    assert got == [ctypes.sizeof(E), E.batch.offset, E.rows_live.offset, E.path.offset, E.redone.offset, E.survivors.offset, E.launches.offset]

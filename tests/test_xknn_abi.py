"""The k-NN join's C ABI (zh_cross_knn*): declared in the header, exported under SYMBOLS, zh_xknn_info's layout mirrored by ctypes, a C99
program compiles against the header, the argument checks that are judged before any device is touched, and a host-only compile of
include/zebra.hpp that uses cross_knn.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XKNN = ("zh_cross_knn", "zh_cross_knn_device", "zh_cross_knn_info")
FIELDS = ("rows_live_a", "rows_live_b", "lines", "k", "path", "redone", "survivors", "launches", "tiles")


def test_header_declares_the_knn_join():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in XKNN:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_xknn_info" in h
    assert "(new; the reference has no such call)" in h[h.index("k-NN JOIN BETWEEN TWO INDEXES"):h.index("ZH_API int zh_cross_knn(")]


def test_symbols_list_the_knn_join():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    for name in XKNN:
        assert name in names, name
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in XKNN:
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.CrossKnnInfo._fields_] == list(FIELDS)
    # the siblings' mirrors are as they were
    assert [f for f, _ in _ffi.KnnInfo._fields_] == ["rows_live", "lines", "k", "path", "redone", "survivors", "launches", "tiles"]
    assert [f for f, _ in _ffi.CrossInfo._fields_] == ["rows_live_a", "rows_live_b", "pairs", "path", "redone", "candidates", "launches", "tiles"]


def test_info_layout_matches_header_in_c99():
    """a C99 program against the header: the struct's size and offsets as ctypes mirrors them, and the three calls' prototypes as the issue
    states them (assigned to pointers of exactly those types)"""
    from zebra_amd import _ffi
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "zebra_hip.h"
int main(void){
  int (*host)(zh_index *, zh_index *, uint64_t, uint64_t, size_t, int, int, uint64_t *, uint64_t *, uint32_t *) = zh_cross_knn;
  int (*dev)(zh_index *, zh_index *, uint64_t, uint64_t, size_t, int, int, uint64_t *, uint64_t *, uint32_t *, void *) = zh_cross_knn_device;
  int (*info)(const zh_index *, zh_xknn_info *) = zh_cross_knn_info;
  (void)host; (void)dev; (void)info;
  printf("%%zu", sizeof(zh_xknn_info));
%s
  printf("\n");
  return 0; }''' % "\n".join('  printf(" %%zu", offsetof(zh_xknn_info, %s));' % f for f in FIELDS)
    libdir = os.path.dirname(_ffi.LIB_PATH)
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-L", libdir, "-lzebra_hip",
                               "-Wl,-rpath," + libdir, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    F = _ffi.CrossKnnInfo
    assert got == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS]


def test_arguments_are_judged_before_any_device():
    """A null index on either side, the same index twice, an unknown metric, k = 1025 and null outputs for a non-empty request are refused by
    the first lines of either entry point.  The calls pass (never dereferenced) stand-ins for the indexes: were a check lost, the call would go
    on to lock a stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake_a, fake_b = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    ia, ib = ctypes.cast(fake_a, ctypes.c_void_p), ctypes.cast(fake_b, ctypes.c_void_p)
    ids, keys, counts = (ctypes.c_uint64 * 4096)(), (ctypes.c_uint64 * 4096)(), (ctypes.c_uint32 * 4)()
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def host(xa, xb, n, k, metric, ip, kp, cp):
        return L.zh_cross_knn(xa, xb, 0, n, k, metric, 0, ip, kp, cp)

    def dev(xa, xb, n, k, metric, ip, kp, cp):
        return L.zh_cross_knn_device(xa, xb, 0, n, k, metric, 0, ip, kp, cp, None)

    for call in (host, dev):
        assert call(None, ib, 4, 3, 0, P(ids), P(keys), P(counts)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(ia, None, 4, 3, 0, P(ids), P(keys), P(counts)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(None, None, 0, 0, 0, None, None, None) == _ffi.ZH_EINVAL
        assert call(ia, ia, 4, 3, 0, P(ids), P(keys), P(counts)) == _ffi.ZH_EINVAL and b"zh_knn_graph" in L.zh_last_error()
        assert call(ia, ia, 0, 3, 0, None, None, None) == _ffi.ZH_EINVAL and b"zh_knn_graph" in L.zh_last_error()  # (even an empty request)
        assert call(ia, ib, 4, 3, 0, None, P(keys), P(counts)) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
        assert call(ia, ib, 4, 3, 0, P(ids), None, P(counts)) == _ffi.ZH_EINVAL
        assert call(ia, ib, 4, 3, 0, P(ids), P(keys), None) == _ffi.ZH_EINVAL
        assert call(ia, ib, 4, 0, 0, None, None, None) == _ffi.ZH_EINVAL  # (k = 0 still writes the counts)
        assert call(ia, ib, 4, 3, 99, P(ids), P(keys), P(counts)) == _ffi.ZH_EINVAL  # no such metric
        assert call(ia, ib, 0, 3, 99, None, None, None) == _ffi.ZH_EINVAL
        assert call(ia, ib, 4, 1025, 0, P(ids), P(keys), P(counts)) == _ffi.ZH_ELIMIT and b"ZH_MAX_TOPK" in L.zh_last_error()
        assert call(ia, ib, 0, 1025, 0, None, None, None) == _ffi.ZH_ELIMIT
        assert call(ia, ib, 0, 1024, 0, None, None, None) == _ffi.ZH_OK  # (n = 0 within the limit: nothing to do, neither handle followed)
    info = _ffi.CrossKnnInfo()
    assert L.zh_cross_knn_info(None, ctypes.byref(info)) == _ffi.ZH_EINVAL
    assert L.zh_cross_knn_info(ia, None) == _ffi.ZH_EINVAL


def test_cpp_wrapper_compiles_host_only():
    """include/zebra.hpp with cross_knn instantiated, compiled (not linked) by the host compiler alone"""
    src = r'''
#include "zebra.hpp"
using namespace zebra;
std::size_t nearest(const LSHIndex<64> &a, const LSHIndex<64> &b) {
    L2SquaredDistance<64> m;
    auto all = a.cross_knn(b, 5, m);
    auto slab = a.cross_knn(b, 5, m, 0, 1);
    zh_xknn_info info = a.cross_knn_info();
    return all.size() + slab.size() + info.lines;
}
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.cpp")
        open(c, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), c, "-o",
                               os.path.join(td, "t.o")])


def test_wrappers_and_docs_name_the_knn_join():
    import zebra_amd
    assert callable(zebra_amd.LSHIndex.cross_knn) and callable(zebra_amd.LSHIndex.cross_knn_device) and callable(zebra_amd.LSHIndex.cross_knn_info)
    assert callable(zebra_amd.Database.nearest_in)
    read = lambda *p: open(os.path.join(ROOT, *p)).read()  # noqa: E731
    rs = read("rust", "zebra-hip", "src", "lib.rs")
    assert "pub fn zh_cross_knn(" in rs and "pub struct zh_xknn_info" in rs and "pub fn cross_knn<" in rs
    assert "pub fn zh_cross_knn(" in read("INTEGRATION.md")
    assert "zh_cross_knn" in read("DESIGN.md") and "k-NN join between two indexes" in read("README.md")


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "xknn_example.c"), "-o", os.path.join(td, "e.o")])

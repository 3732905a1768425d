"""Filter-steered graph search's C ABI (zh_search_graph_steered_batch*, zh_search_graph_steered_info): declared in the header, exported under
SYMBOLS, the info struct's layout mirrored by ctypes, the argument checks that are judged before any device is touched --
zh_search_graph_filtered_batch's, in its order, with `hops` the last of the scalar limits -- and the C example.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("zh_search_graph_steered_batch", "zh_search_graph_steered_batch_device", "zh_search_graph_steered_info")
FIELDS = ("queries", "seeds", "iterations", "expanded", "keyed", "capped", "launches", "rows_allowed", "direct", "via_bridge", "bridges", "cand_full",
          "returned")


def test_header_declares_the_steered_graph_search_calls():
    h = open(os.path.join(ROOT, "include", "zebra_hip.h")).read()
    for name in CALLS:
        assert re.search(r"ZH_API\s+int\s+%s\s*\(" % name, h), name
    assert "typedef struct zh_graph_steered_info" in h and re.search(r"#define\s+ZH_GRAPH_MAX_CAND\s+256u", h)
    assert re.search(r"zh_search_graph_steered_batch_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", h)
    # zh_search_graph_filtered_batch's arguments in their positions, hops directly after n_bits
    for name, pre in (("zh_search_graph_steered_batch", ""), ("zh_search_graph_steered_batch_device", "d_")):
        assert re.search(name + r"\s*\([^;]*size_t\s+b,\s*const\s+uint64_t\s*\*\s*" + pre + r"seeds,\s*size_t\s+n_seed,\s*size_t\s+top_k,\s*size_t\s+beam,\s*"
                         r"size_t\s+width,\s*size_t\s+max_iters,\s*int\s+metric,\s*int\s+cosine_mode,\s*const\s+uint32_t\s*\*\s*" + pre +
                         r"filter_words,\s*uint64_t\s+n_bits,\s*int\s+hops,\s*uint64_t\s*\*\s*" + pre + "out_ids", h), name
    head = h[:h.index("Conventions")]
    assert "zh_search_graph_steered_batch[_device]" in head


def test_symbols_list_the_steered_graph_search_calls():
    from zebra_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert name in names, name
        assert hasattr(lib, name), name
    assert [f for f, _ in _ffi.SearchGraphSteeredInfo._fields_] == list(FIELDS)
    assert [f for f, _ in _ffi.SearchGraphInfo._fields_] == list(FIELDS[:7])  # (the siblings keep theirs)
    assert [f for f, _ in _ffi.SearchGraphFilteredInfo._fields_] == list(FIELDS[:8]) + ["offered", "returned"]
    assert _ffi.GRAPH_MAX_CAND == 256


def test_info_layout_matches_the_header():
    from zebra_amd import _ffi
    body = '  printf("%zu", sizeof(zh_graph_steered_info));\n'
    body += "\n".join('  printf(" %%zu", offsetof(zh_graph_steered_info, %s));' % f for f in FIELDS) + '\n  printf("\\n");\n'
    body += '  printf("%zu %zu\\n", sizeof(zh_graph_search_info), sizeof(zh_graph_filtered_info));\n'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "zebra_hip.h"\nint main(void){\n%s  return 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    F = _ffi.SearchGraphSteeredInfo
    assert lines[0] == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in FIELDS] == [104] + list(range(0, 104, 8))
    assert lines[1] == [ctypes.sizeof(_ffi.SearchGraphInfo), ctypes.sizeof(_ffi.SearchGraphFilteredInfo)] == [56, 80]
    info = F()
    info.via_bridge = 7
    assert info.as_dict() == dict.fromkeys(FIELDS, 0) | {"via_bridge": 7}


def test_arguments_are_judged_before_any_device():
    """zh_search_graph_filtered_batch's checks in its order -- the null filter with the null pointers, the metric, the zeros, the limits -- and
    then hops: anything but 1 or 2 is ZH_EINVAL, after max_iters.  The calls that pass a (never dereferenced) stand-in for the index must fail:
    were a check lost, the call would go on to lock that stand-in and reach for a device."""
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    arrays = [(ctypes.c_float * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 8)(), (ctypes.c_uint32 * 2)(), (ctypes.c_uint32 * 2)()]
    Q, S, I, K, N, F = [ctypes.cast(a, ctypes.c_void_p) for a in arrays]

    def host(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, f, n_bits, hops, ip, kp, cp):
        return L.zh_search_graph_steered_batch(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, 0, f, n_bits, hops, ip, kp, cp)

    def dev(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, f, n_bits, hops, ip, kp, cp):
        return L.zh_search_graph_steered_batch_device(ix, q, b, s, n_seed, top_k, beam, width, max_iters, metric, 0, f, n_bits, hops, ip, kp, cp, None)

    for call in (host, dev):
        # every refusal below holds whatever hops is: a bad one is judged last
        for hops in (2, 1, 0, 3, -1):
            assert call(None, Q, 1, S, 4, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
            assert call(None, Q, 0, S, 4, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL  # (even for an empty batch)
            for at in range(5):
                ptrs = [Q, S, I, K, N]
                ptrs[at] = None
                assert call(idx, ptrs[0], 1, ptrs[1], 4, 4, 8, 1, 0, 1, F, 40, hops, *ptrs[2:]) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error(), at
            # the null filter: with the null pointers, ahead of everything else
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 1, None, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 99, None, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()  # before the metric
            assert call(idx, Q, 1, S, 4, 0, 8, 1, 0, 1, None, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()   # ... the zeros
            assert call(idx, Q, 1, S, 4, 4, 257, 1, 0, 1, None, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()  # ... the limits
            assert call(idx, Q, 0, S, 4, 4, 8, 1, 0, 1, None, 1, hops, I, K, N) == _ffi.ZH_EINVAL and b"null filter" in L.zh_last_error()    # ... for b = 0 too
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 99, None, 0, hops, I, K, N) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()  # (no rows, no filter)
            # from here on zh_search_graph_batch's list
            assert call(idx, None, 1, S, 4, 4, 999, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"null" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 99, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 0, 999, 1, 0, 99, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"metric" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 0, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"top_k is 0" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 0, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"beam is 0" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 8, 0, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"width is 0" in L.zh_last_error()
            assert call(idx, Q, 1, S, 0, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"n_seed is 0" in L.zh_last_error()
            assert call(idx, Q, 1, S, 0, 4, 999, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"n_seed is 0" in L.zh_last_error()  # zeros before limits
            assert call(idx, Q, 1, S, 4, 4, 257, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 9, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"top_k 9 > beam 8" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 300, 257, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"beam 257 >" in L.zh_last_error()
            assert call(idx, Q, 1, S, 65, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 8, 257, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"width 257 >" in L.zh_last_error()
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 65536, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"max_iters 65536 >" in L.zh_last_error()
            assert call(idx, Q, 1, S, 65, 4, 8, 257, 65536, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT and b"n_seed 65 >" in L.zh_last_error()  # the documented order
            assert call(idx, Q, 0, S, 4, 4, 257, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_ELIMIT  # (an empty batch is judged alike)
        # hops itself: with everything else in order, before any device -- for an empty batch and a filter of no rows too
        for hops in (0, 3, -1, 2**31 - 1, -2**31):
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"hops" in L.zh_last_error(), hops
            assert call(idx, Q, 0, S, 4, 4, 8, 1, 0, 1, F, 40, hops, I, K, N) == _ffi.ZH_EINVAL and b"hops" in L.zh_last_error(), hops
            assert call(idx, Q, 1, S, 4, 4, 8, 1, 65535, 1, None, 0, hops, I, K, N) == _ffi.ZH_EINVAL and b"hops" in L.zh_last_error(), hops
        for hops in (1, 2):
            assert call(idx, None, 0, None, 4, 4, 8, 1, 0, 1, F, 40, hops, None, None, None) == _ffi.ZH_OK  # b = 0 with good scalars
    del fake, arrays


def test_null_info_pointers():
    from zebra_amd import _ffi
    L = _ffi.lib()
    fake = ctypes.create_string_buffer(64)
    idx = ctypes.cast(fake, ctypes.c_void_p)
    s = _ffi.SearchGraphSteeredInfo()
    assert L.zh_search_graph_steered_info(None, ctypes.byref(s)) == _ffi.ZH_EINVAL
    assert L.zh_search_graph_steered_info(idx, None) == _ffi.ZH_EINVAL
    del fake


def test_example_compiles_as_c99():
    with tempfile.TemporaryDirectory() as td:
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "examples", "graph_steered_example.c"), "-o", os.path.join(td, "e.o")])

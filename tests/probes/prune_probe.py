"""Timing and recall probe of k-NN graph pruning (zh_knn_graph_prune) on tests/probes/refine_probe.py's and graph_search_probe.py's setup: rows x
768 synthetic rows (append_synthetic(kind=0): iid; kind 2: clustered), options 4096 / 15, L2SQ, everything in device memory.  The input graphs:
knn_graph_forest(32) then knn_graph_descent(k = 32, 8 rounds), and the same descent at k = 64 (2 rounds: only its width matters here).

Section "times": arms alternated, one warm-up and 3 timed runs each, median and range --
  prune 32 -> 16, reverse 0 and 16;  prune 64 -> 32, reverse 0 (in_k + reverse <= 64: a line of 64 has no room for reverse neighbours);
  prune 48 -> 32, reverse 16 (the widest line that has);  refine 32: ONE knn_graph_refine round over the k = 32 graph, in the same run.
Per pruning arm: candidates, kept, occluded, cut and keyed of knn_prune_info().

Section "search": the descent graph at k = 32 and its pruned forms (16 / reverse 0, 16 / reverse 16, 16 / reverse 16 with fill, 8 / reverse 16),
each attached in turn (set_graph_device, not timed), 1024 queries (synth_queries_device), the same 32 strided seeds, top-10, width 4, beams 64 /
128 / 256: three passes over all graphs, median and range of the batch time, recall@10 against search_exact_batch_device, keyed per query.
The index is created before any torch GEMM (INTEGRATION section 9's order effect): nothing here runs one.

    python tests/probes/prune_probe.py [rows] [kind] [sections] [library]   (default 1048576 0 times,search, the built library)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests.probes.graph_search_probe import alternate, recall  # noqa: E402

D, B, TOP, N_SEED, WIDTH = 768, 1024, 10, 32, 4
BEAMS = (64, 128, 256)


def main(n, kind, sections):
    import torch
    import zebra_amd as za
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
    ix.append_synthetic(n, kind=kind)
    ix.build()
    dev = torch.device("cuda", 0)
    graph = lambda k: (torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.int64, device=dev),  # noqa: E731
                       torch.empty(n, dtype=torch.int32, device=dev))
    ptrs = lambda g: [t.data_ptr() for t in g]  # noqa: E731
    f, g32 = graph(32), graph(32)
    t0 = time.perf_counter()
    ix.knn_graph_forest_device(32, m, 0, n, *ptrs(f))
    t1 = time.perf_counter()
    ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), 32, 0, 32, 8, m, *ptrs(g32))
    t2 = time.perf_counter()
    out(case="index", rows=n, dim=D, kind=kind, forest_graph_ms=round((t1 - t0) * 1e3, 1), descent_ms=round((t2 - t1) * 1e3, 1),
        rounds_run=ix.knn_descent_info()["rounds_run"])

    def prune(g, in_k, rev_k, degree, fill, o):
        ix.knn_graph_prune_device(g[0].data_ptr(), g[2].data_ptr(), in_k, rev_k, degree, fill, m, 0, n, *ptrs(o))

    if "times" in sections:
        g64 = graph(64)
        ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), 32, 0, 64, 2, m, *ptrs(g64))
        g48 = (g64[0][:, :48].contiguous(), None, g64[2])  # (a line is its first in_k entries, so the table has to be in_k wide)
        o16, o32, r32 = graph(16), graph(32), graph(32)
        cases = {"prune 32 -> 16, reverse 0": (g32, 32, 0, 16, o16), "prune 32 -> 16, reverse 16": (g32, 32, 16, 16, o16),
                 "prune 64 -> 32, reverse 0": (g64, 64, 0, 32, o32), "prune 48 -> 32, reverse 16": (g48, 48, 16, 32, o32)}
        arms = {name: (lambda c=c: prune(c[0], c[1], c[2], c[3], 0, c[4])) for name, c in cases.items()}
        arms["refine 32"] = lambda: ix.knn_graph_refine_device(g32[0].data_ptr(), g32[2].data_ptr(), 32, 32, m, 0, n, *ptrs(r32))
        row = alternate(arms)
        for name, c in cases.items():
            prune(c[0], c[1], c[2], c[3], 0, c[4])
            info = ix.knn_prune_info()
            out(case=name, mean_degree=round(info["kept"] / max(info["lines"], 1), 2),
                **{k: info[k] for k in ("lines", "candidates", "kept", "occluded", "cut", "keyed", "launches")}, **row[name])
        arms["refine 32"]()
        info = ix.knn_refine_info()
        out(case="refine 32", keyed=info["keyed"], listed=info["listed"], updates=info["updates"], **row["refine 32"])
        del g64, g48, o16, o32, r32
    del f

    if "search" in sections:
        q = torch.empty((B, D), dtype=torch.float32, device=dev)
        za.synth_queries_device(0, q.data_ptr(), n, B, D, kind=kind)
        seeds = torch.from_numpy((np.arange(N_SEED, dtype=np.int64) * n // N_SEED)[None, :].repeat(B, 0)).to(dev)
        res = lambda: (torch.empty((B, TOP), dtype=torch.int64, device=dev), torch.empty((B, TOP), dtype=torch.int64, device=dev),  # noqa: E731
                       torch.empty(B, dtype=torch.int32, device=dev))
        exact = res()
        ix.search_exact_batch_device(q.data_ptr(), B, TOP, m, *ptrs(exact))
        forms = {"descent 32": (g32, 32)}
        for name, (rev_k, degree, fill) in {"pruned 16, reverse 0": (0, 16, 0), "pruned 16, reverse 16": (16, 16, 0),
                                            "pruned 16, reverse 16, fill": (16, 16, 1), "pruned 8, reverse 16": (16, 8, 0)}.items():
            o = graph(degree)
            prune(g32, 32, rev_k, degree, fill, o)
            info = ix.knn_prune_info()
            out(case="graph", form=name, mean_degree=round((info["kept"] + info["filled"]) / max(info["lines"], 1), 2), cut=info["cut"])
            forms[name] = (o, degree)
        o = res()
        ms = {(name, b): [] for name in forms for b in BEAMS}
        stat = {}
        for p in range(4):  # pass 0 warms up
            for name, (g, k) in forms.items():
                ix.set_graph_device(g[0].data_ptr(), g[2].data_ptr(), n, k)
                for b in BEAMS:
                    t0 = time.perf_counter()
                    ix.search_graph_batch_device(q.data_ptr(), B, seeds.data_ptr(), N_SEED, TOP, m, *ptrs(o), beam=b, width=WIDTH)
                    if p:
                        ms[name, b].append((time.perf_counter() - t0) * 1e3)
                    info = ix.search_graph_info()
                    stat[name, b] = dict(recall=recall(exact, o), keyed_per_query=round(info["keyed"] / B, 1),
                                         iterations_per_query=round(info["iterations"] / B, 1))
        for (name, b), v in ms.items():
            out(case="search", form=name, beam=b, width=WIDTH, median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                **stat[name, b])
    ix.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) > 3:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(a[3])
    main(int(a[0]) if len(a) > 0 else 1_048_576, int(a[1]) if len(a) > 1 else 0, set((a[2] if len(a) > 2 else "times,search").split(",")))

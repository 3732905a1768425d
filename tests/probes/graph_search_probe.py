"""Timing and recall probe of graph search (zh_search_graph_batch) beside the two query paths it sits between, on tests/probes/descent_probe.py's
setup: rows x 768 synthetic rows (append_synthetic(kind=0): iid; kind 2: clustered), options 4096 / 15, L2SQ, the graph = knn_graph_forest then
knn_graph_descent(k = 32, 8 rounds), attached with set_graph_device.  1024 queries per batch (synth_queries_device: planted near stored rows),
everything in device memory.  Arms, alternated, one warm-up and 3 timed runs each (DESIGN.md s24's table):

  graph b / w    search_graph_batch_device at beam b in {32, 64, 128, 256}, width w in {1, 4}, 32 strided seeds
  lsh            search_batch_device, k = 10 (the LSH forest)
  lsh + graph    search_batch_device with k = 32, its ids as the graph search's seeds (beam 32 / 64): both calls timed together
  exact          search_exact_batch_device, k = 10 (the ground truth of the recall)

Per arm it prints the median and range of the batch time, recall@10 against the exact arm, and for the graph arms keyed / iterations per query.
Section "rules": the CPU reference's keyed count under the definition and under the textbook rule (a visited set) on the first `sample` rows of
the same table with the exact 32-NN graph, 16 queries -- what a visited set would save (`... rules` alone needs no GPU).  Also printed: the
forest graph's, the descent's and the attach's time (device entries).
The index is created before any torch GEMM (INTEGRATION section 9's order effect): nothing here runs one.

    python tests/probes/graph_search_probe.py [rows] [kind] [sections] [library]   (default 1048576 0 times,rules, the built library)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, K, B, TOP, N_SEED = 768, 32, 1024, 10, 32
BEAMS, WIDTHS = (32, 64, 128, 256), (1, 4)


def alternate(arms, reps=3):
    """one warm-up of every arm, then reps passes over all of them in turn -> {arm: median, min, max in ms}"""
    ms = {name: [] for name in arms}
    for name, fn in arms.items():
        fn()
    for _ in range(reps):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for name, v in ms.items()}


def recall(exact, got):
    """recall@TOP of (ids, counts) tensors against the exact arm's"""
    x, y = exact[0], got[0]
    hit = int(((x[:, :, None] == y[:, None, :]) & (x[:, :, None] != -1)).any(dim=2).sum().item())
    return round(hit / max(int(exact[2].sum().item()), 1), 4)


def times(n, kind, out):
    import torch
    import zebra_amd as za
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
    ix.append_synthetic(n, kind=kind)
    ix.build()
    dev = torch.device("cuda", 0)
    graph = lambda: (torch.empty((n, K), dtype=torch.int64, device=dev), torch.empty((n, K), dtype=torch.int64, device=dev),  # noqa: E731
                     torch.empty(n, dtype=torch.int32, device=dev))
    f, g = graph(), graph()
    t0 = time.perf_counter()
    ix.knn_graph_forest_device(K, m, 0, n, *(t.data_ptr() for t in f))
    t1 = time.perf_counter()
    ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), K, 0, K, 8, m, *(t.data_ptr() for t in g))
    t2 = time.perf_counter()
    attach = []
    for _ in range(4):
        ta = time.perf_counter()
        ix.set_graph_device(g[0].data_ptr(), g[2].data_ptr(), n, K)
        attach.append((time.perf_counter() - ta) * 1e3)
    out(case="index", rows=n, dim=D, options=[4096, 15], kind=kind, k=K, forest_graph_ms=round((t1 - t0) * 1e3, 1), descent_ms=round((t2 - t1) * 1e3, 1),
        descent=ix.knn_descent_info()["rounds_run"], attach_ms=[round(a, 3) for a in attach], graph=ix.graph_info())
    del f

    q = torch.empty((B, D), dtype=torch.float32, device=dev)
    za.synth_queries_device(0, q.data_ptr(), n, B, D, kind=kind)
    seeds = torch.from_numpy((np.arange(N_SEED, dtype=np.int64) * n // N_SEED)[None, :].repeat(B, 0)).to(dev)
    res = lambda: (torch.empty((B, TOP), dtype=torch.int64, device=dev), torch.empty((B, TOP), dtype=torch.int64, device=dev),  # noqa: E731
                   torch.empty(B, dtype=torch.int32, device=dev))
    exact, lsh = res(), res()
    outs = {(b, w): res() for b in BEAMS for w in WIDTHS}
    arms = {"exact": lambda: ix.search_exact_batch_device(q.data_ptr(), B, TOP, m, *(t.data_ptr() for t in exact)),
            "lsh": lambda: (ix.search_batch_device(q.data_ptr(), B, TOP, m, *(t.data_ptr() for t in lsh)), torch.cuda.synchronize())}
    for (b, w), o in outs.items():
        arms["graph %d / %d" % (b, w)] = (lambda b=b, w=w, o=o: ix.search_graph_batch_device(q.data_ptr(), B, seeds.data_ptr(), N_SEED, TOP, m,
                                                                                              *(t.data_ptr() for t in o), beam=b, width=w))
    # ... and seeded by the LSH search's own answer (seeds="lsh" of the Python layer): both calls timed together
    lsh_seeds = torch.empty((B, N_SEED), dtype=torch.int64, device=dev)
    lsh_junk = (torch.empty((B, N_SEED), dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    seeded = {(b, w): res() for b in (32, 64) for w in WIDTHS}

    def lsh_then_graph(b, w, o):
        ix.search_batch_device(q.data_ptr(), B, N_SEED, m, lsh_seeds.data_ptr(), lsh_junk[0].data_ptr(), lsh_junk[1].data_ptr())
        ix.search_graph_batch_device(q.data_ptr(), B, lsh_seeds.data_ptr(), N_SEED, TOP, m, *(t.data_ptr() for t in o), beam=b, width=w)

    for (b, w), o in seeded.items():
        arms["lsh + graph %d / %d" % (b, w)] = lambda b=b, w=w, o=o: lsh_then_graph(b, w, o)
    row = alternate(arms)
    out(case="exact", **row["exact"])
    out(case="lsh", recall=recall(exact, lsh), **row["lsh"])
    for (b, w), o in seeded.items():
        lsh_then_graph(b, w, o)
        info = ix.search_graph_info()
        out(case="lsh + graph", beam=b, width=w, recall=recall(exact, o), keyed_per_query=round(info["keyed"] / B, 1),
            iterations_per_query=round(info["iterations"] / B, 1), **row["lsh + graph %d / %d" % (b, w)])
    for (b, w), o in outs.items():
        ix.search_graph_batch_device(q.data_ptr(), B, seeds.data_ptr(), N_SEED, TOP, m, *(t.data_ptr() for t in o), beam=b, width=w)
        info = ix.search_graph_info()
        out(case="graph", beam=b, width=w, recall=recall(exact, o), keyed_per_query=round(info["keyed"] / B, 1),
            iterations_per_query=round(info["iterations"] / B, 1), **row["graph %d / %d" % (b, w)])
    ix.close()


def main(n, kind, sections, sample=4096):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    if "times" in sections:
        times(n, kind, out)
    if "rules" in sections:
        from oracle import zebra_oracle as zo
        from tests import gsearch_cases as gc
        X = zo.synth_rows(sample, D, kind=kind)
        live = np.ones(sample, bool)
        eg = gc.exact_graph(X, K, live, 0, zo.L2SQ, 0)
        Q = zo.synth_queries(16, D, sample, kind=kind)
        for b in BEAMS:
            for w in WIDTHS:
                sd = gc.default_seeds(16, N_SEED, sample, 0)
                a = gc.reference(X, eg, sample, K, live, 0, Q, sd, TOP, b, w, 0, zo.L2SQ, 0)[1]
                t = gc.reference_textbook(X, eg, sample, K, live, 0, Q, sd, TOP, b, w, 0, zo.L2SQ, 0)[1]
                out(case="rules", rows=sample, beam=b, width=w, keyed=a["keyed"], keyed_textbook=t["keyed"], ratio=round(a["keyed"] / max(t["keyed"], 1), 3),
                    iterations=a["iterations"])


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) > 3:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(a[3])
    main(int(a[0]) if len(a) > 0 else 1_048_576, int(a[1]) if len(a) > 1 else 0, set((a[2] if len(a) > 2 else "times,rules").split(",")))

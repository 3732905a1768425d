"""Timing probe of the exact k-NN graph (zh_knn_graph_device): 262 144 x 768 synthetic rows, L2SQ, k = 32, device entry points.  Rows of the
table in DESIGN.md s16: the yardstick -- the loop the graph call replaces: search_exact_batch_device over the index's own rows as queries, 1024
at a time with k + 1, self dropped on the device (the rows are read back once, outside the timing: the user's second copy) -- the graph call,
and the graph call with path 1 forced (ZH_KNN_PATH=1, read per call; fewer runs: it is the slow one).  One warm-up, then the timed runs: median,
min and max; `condition` = the graph call's slowest run is faster than the loop's fastest; `agree` = both give the same ids, keys and counts.
    python tests/probes/knn_probe.py [rows] [graph]      (default 262144; "graph": the path-rule call alone, for a kernel trace of its own)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = 5


def timed(fn, reps=REPS):
    fn()  # warm-up: scratch, the fp16 copy
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(runs=reps, median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


def main(n, graph_only=False):
    import torch
    import zebra_amd as za
    d, B, k = 768, 1024, 32
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    dev = torch.device("cuda", 0)
    g_ids = torch.empty((n, k), dtype=torch.int64, device=dev)
    g_keys, g_counts = torch.empty_like(g_ids), torch.empty(n, dtype=torch.int32, device=dev)

    def graph():
        ix.knn_graph_device(k, m, 0, n, g_ids.data_ptr(), g_keys.data_ptr(), g_counts.data_ptr())

    if graph_only:
        print(json.dumps(dict(case="k-NN graph alone", rows=n, k=k, **timed(graph, 1), info=ix.knn_info())), flush=True)
        return

    # the yardstick: every row a query, 1024 at a time with k + 1; the line's own id is moved last (a stable sort on "is my own id") and cut off
    rows = torch.from_numpy(ix.read_rows(0, n)).to(dev)
    l_ids = torch.empty((n, k), dtype=torch.int64, device=dev)
    l_keys, l_counts = torch.empty_like(l_ids), torch.empty(n, dtype=torch.int32, device=dev)
    b_ids = torch.empty((B, k + 1), dtype=torch.int64, device=dev)
    b_keys, b_counts = torch.empty_like(b_ids), torch.empty(B, dtype=torch.int32, device=dev)
    survivors = [0]

    def loop():
        survivors[0] = 0
        for b0 in range(0, n, B):
            nb = min(B, n - b0)
            ix.search_exact_batch_device(rows[b0:].data_ptr(), nb, k + 1, m, b_ids.data_ptr(), b_keys.data_ptr(), b_counts.data_ptr())
            survivors[0] += ix.exact_info()["survivors"]
            mine = b_ids[:nb] == torch.arange(b0, b0 + nb, device=dev)[:, None]
            order = torch.argsort(mine.to(torch.int8), dim=1, stable=True)[:, :k]
            l_ids[b0:b0 + nb] = torch.gather(b_ids[:nb], 1, order)
            l_keys[b0:b0 + nb] = torch.gather(b_keys[:nb], 1, order)
            l_counts[b0:b0 + nb] = torch.clamp(b_counts[:nb] - mine.any(dim=1).to(torch.int32), max=k)
        torch.cuda.synchronize()

    row_loop = timed(loop)
    print(json.dumps(dict(case="loop of search_exact_batch_device with k + 1, self dropped on the device", rows=n, k=k, **row_loop,
                          survivors_per_line=round(survivors[0] / n, 1), info=ix.exact_info())), flush=True)
    row_graph = timed(graph)
    info = ix.knn_info()
    agree = bool(torch.equal(g_ids, l_ids) and torch.equal(g_keys, l_keys) and torch.equal(g_counts, l_counts))
    print(json.dumps(dict(case="k-NN graph, path rule", **row_graph, info=info, survivors_per_line=round(info["survivors"] / max(info["lines"], 1), 1),
                          ratio_loop_over_graph=round(row_loop["median_ms"] / row_graph["median_ms"], 2),
                          condition=bool(row_graph["max_ms"] < row_loop["min_ms"]), agree=agree)), flush=True)
    os.environ["ZH_KNN_PATH"] = "1"
    row_p1 = timed(graph, 2)
    agree1 = bool(torch.equal(g_ids, l_ids) and torch.equal(g_keys, l_keys) and torch.equal(g_counts, l_counts))
    print(json.dumps(dict(case="k-NN graph, path 1 forced", **row_p1, info=ix.knn_info(), agree=agree1)), flush=True)
    os.environ.pop("ZH_KNN_PATH", None)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 262_144, len(sys.argv) > 2 and sys.argv[2] == "graph")

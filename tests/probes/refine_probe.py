"""Timing probe of the k-NN graph refinement (zh_knn_graph_refine_device) over the forest graph, beside the exact graph (zh_knn_graph_device) on the
same index in the same process: 1 048 576 x 768 synthetic rows (append_synthetic(kind=2): clustered; kind 0: iid), options 4096 / 15, L2SQ,
k = in_k = 32, device entry points, one warm-up and 3 timed runs each.  Rows of the table in DESIGN.md s21:

  times    the forest graph, one refinement round over it, a second round over the first round's output, the exact graph (the yardstick);
           `condition` = the slowest run of forest graph + one round is faster than the fastest run of the exact graph
  recall   recall@32 against the exact graph of the forest graph, after one round and after two, and each round's `updates`
  rate     one warm-up and 3 runs of the first round alone, with `keyed` per run: under `rocprofv3 --kernel-trace --stats` (a run of its own) the
           time of refine_line_kernel gives keyed x 4 d bytes per second.  A library built with another ZH_REFINE_INFLIGHT
           (make EXTRA=-DZH_REFINE_INFLIGHT=8, copied aside) is measured by passing its path as the fourth argument.

    python tests/probes/refine_probe.py [rows] [sections] [kind] [library]    (default 1048576, "times,recall", 2, the built library)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, K = 768, 32


def timed(fn, reps=3):
    fn()  # warm-up: scratch, the fp16 copy
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    if not ms:
        return dict(runs=0)
    return dict(runs=reps, median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


class Case:
    def __init__(self, n, node, trees, kind):
        import torch
        import zebra_amd as za
        self.torch, self.n, self.m = torch, n, za.L2SquaredDistance()
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(node, trees), device=0)
        self.ix.append_synthetic(n, kind=kind)
        t0 = time.perf_counter()
        self.ix.build()
        self.build_ms = round((time.perf_counter() - t0) * 1e3, 1)
        dev = torch.device("cuda", 0)
        graph = lambda: (torch.empty((n, K), dtype=torch.int64, device=dev), torch.empty((n, K), dtype=torch.int64, device=dev),  # noqa: E731
                         torch.empty(n, dtype=torch.int32, device=dev))
        self.e, self.f, self.r1, self.r2 = graph(), graph(), graph(), graph()

    def exact(self):
        self.ix.knn_graph_device(K, self.m, 0, self.n, *(t.data_ptr() for t in self.e))

    def forest(self):
        self.ix.knn_graph_forest_device(K, self.m, 0, self.n, *(t.data_ptr() for t in self.f))

    def refine(self, src, dst):
        self.ix.knn_graph_refine_device(src[0].data_ptr(), src[2].data_ptr(), K, K, self.m, 0, self.n, *(t.data_ptr() for t in dst))

    def recall(self, g):
        """share of the exact graph's edges that graph g names (ids compared as sets per line)"""
        hit = 0
        for r0 in range(0, self.n, 65536):
            e, f = self.e[0][r0:r0 + 65536], g[0][r0:r0 + 65536]
            hit += int(((e[:, :, None] == f[:, None, :]) & (e[:, :, None] != -1)).any(dim=2).sum().item())
        return round(hit / max(int(self.e[2].sum().item()), 1), 4)


def main(n, sections, kind):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    c = Case(n, 4096, 15, kind)
    out(case="index", rows=n, dim=D, options=[4096, 15], kind=kind, build_ms=c.build_ms)
    row_f = timed(c.forest, 3 if "times" in sections else 0)  # (the other sections need the graph, not its time)
    out(case="forest graph", k=K, **row_f, info=c.ix.knn_forest_info())
    if "rate" in sections:
        row = timed(lambda: c.refine(c.f, c.r1))
        info = c.ix.knn_refine_info()
        out(case="round 1 alone (for the kernel trace)", calls=4, **row, info=info, keyed_bytes_per_call=info["keyed"] * 4 * D,
            wall_tb_per_s=round(info["keyed"] * 4 * D / row["median_ms"] / 1e9, 3))
    if "times" in sections or "recall" in sections:
        row_1 = timed(lambda: c.refine(c.f, c.r1))
        info_1 = c.ix.knn_refine_info()
        row_2 = timed(lambda: c.refine(c.r1, c.r2))
        info_2 = c.ix.knn_refine_info()
        out(case="round 1 over the forest graph", k=K, in_k=K, **row_1, info=info_1)
        out(case="round 2 over round 1", k=K, in_k=K, **row_2, info=info_2)
        row_e = timed(c.exact, 3 if "times" in sections else 1)
        out(case="exact graph (yardstick)", k=K, **row_e, info=c.ix.knn_info())
        if "times" in sections:
            out(case="condition", slowest_forest_plus_round_ms=round(row_f["max_ms"] + row_1["max_ms"], 2), fastest_exact_ms=row_e["min_ms"],
                holds=bool(row_f["max_ms"] + row_1["max_ms"] < row_e["min_ms"]))
        out(case="recall@%d against the exact graph" % K, kind=kind, forest=c.recall(c.f), round_1=c.recall(c.r1), round_2=c.recall(c.r2),
            updates_1=info_1["updates"], updates_2=info_2["updates"])
    c.ix.close()


if __name__ == "__main__":
    if len(sys.argv) > 4:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(sys.argv[4])
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576, set((sys.argv[2] if len(sys.argv) > 2 else "times,recall").split(",")),
         int(sys.argv[3]) if len(sys.argv) > 3 else 2)

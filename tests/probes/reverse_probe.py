"""Timing probe of the refinement with reverse neighbours (zh_knn_graph_refine_rev_device) beside the forward-only call
(zh_knn_graph_refine_device, the yardstick) on the same index in the same process: 1 048 576 x 768 synthetic rows (append_synthetic(kind=0): iid;
kind 2: clustered), options 4096 / 15, L2SQ, k = in_k = 32, device entry points, one warm-up and 3 timed runs of every round.  The forest graph
and the exact graph are computed ONCE; every arm starts from the same forest graph arrays (two runs of the forest graph differ in a few lines,
DESIGN.md s21).  Rows of the table in DESIGN.md s22:

  rounds   per arm -- the forward call, then rev_k = 0, 8, 16, 32 through the new entry -- ROUNDS rounds, each over the round before: wall time of
           the round (median, min, max), recall@32 against the exact graph after it, its info (keyed, updates, edges, kept, max_degree)
  reverse  zh_knn_graph_reverse_device alone at rev_k = 32 over the forest graph: the table, count, scan, fill and select and nothing else
  trace    one warm-up and 3 runs of round 1 at rev_k = 32 alone: under `rocprofv3 --kernel-trace --stats` (a run of its own) the times of
           rev_edges / rev_sums / rev_scan_sums / rev_offsets / rev_select* beside refine_line_kernel give the transposition's share of a round

    python tests/probes/reverse_probe.py [rows] [sections] [kind] [graph file]    (default 1048576, "rounds,reverse", 0, none)

With a graph file (.npz) the forest graph and the exact graph are saved there by the first run and loaded by a later one (the trace), which then
needs neither the forest nor the exact graph's seconds."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, K, ROUNDS = 768, 32, 3


def timed(fn, reps=3):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(runs=reps, median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


class Case:
    def __init__(self, n, kind, graph_file):
        import torch
        import zebra_amd as za
        self.torch, self.n, self.m = torch, n, za.L2SquaredDistance()
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
        self.ix.append_synthetic(n, kind=kind)
        self.dev = torch.device("cuda", 0)
        self.e, self.f = self.graph(), self.graph()
        if graph_file and os.path.exists(graph_file):
            z = np.load(graph_file)
            for t, name in ((self.e[0], "e_ids"), (self.e[2], "e_counts"), (self.f[0], "f_ids"), (self.f[2], "f_counts")):
                t.copy_(torch.from_numpy(z[name]))
            self.loaded = True
            return
        self.loaded = False
        self.ix.build()
        self.ix.knn_graph_forest_device(K, self.m, 0, n, *(t.data_ptr() for t in self.f))
        self.ix.knn_graph_device(K, self.m, 0, n, *(t.data_ptr() for t in self.e))
        if graph_file:
            os.makedirs(os.path.dirname(os.path.abspath(graph_file)), exist_ok=True)
            np.savez(graph_file, e_ids=self.e[0].cpu().numpy(), e_counts=self.e[2].cpu().numpy(), f_ids=self.f[0].cpu().numpy(),
                     f_counts=self.f[2].cpu().numpy())

    def graph(self):
        t = self.torch
        return (t.empty((self.n, K), dtype=t.int64, device=self.dev), t.empty((self.n, K), dtype=t.int64, device=self.dev),
                t.empty(self.n, dtype=t.int32, device=self.dev))

    def forward(self, src, dst):
        self.ix.knn_graph_refine_device(src[0].data_ptr(), src[2].data_ptr(), K, K, self.m, 0, self.n, *(t.data_ptr() for t in dst))

    def fused(self, rev_k, src, dst):
        self.ix.knn_graph_refine_rev_device(src[0].data_ptr(), src[2].data_ptr(), K, rev_k, K, self.m, 0, self.n, *(t.data_ptr() for t in dst))

    def recall(self, g):
        """share of the exact graph's edges that graph g names (ids compared as sets per line)"""
        hit = 0
        for r0 in range(0, self.n, 65536):
            e, f = self.e[0][r0:r0 + 65536], g[0][r0:r0 + 65536]
            hit += int(((e[:, :, None] == f[:, None, :]) & (e[:, :, None] != -1)).any(dim=2).sum().item())
        return round(hit / max(int(self.e[2].sum().item()), 1), 4)


def main(n, sections, kind, graph_file):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    c = Case(n, kind, graph_file)
    out(case="index", rows=n, dim=D, options=[4096, 15], kind=kind, graphs_loaded=c.loaded, forest_recall=c.recall(c.f))
    if "rounds" in sections:
        arms = [("forward call", None)] + [("rev_k %d" % r, r) for r in (0, 8, 16, 32)]
        for name, rev_k in arms:
            bufs = [c.graph(), c.graph()]
            src, total = c.f, 0.0
            for r in range(1, ROUNDS + 1):
                dst = bufs[r & 1]
                row = timed((lambda: c.forward(src, dst)) if rev_k is None else (lambda: c.fused(rev_k, src, dst)))
                info = c.ix.knn_refine_info() if rev_k is None else c.ix.knn_refine_rev_info()
                total += row["median_ms"]
                out(case="round", arm=name, round=r, **row, cumulative_median_ms=round(total, 2), recall=c.recall(dst), info=info)
                src = dst
            del bufs
    if "reverse" in sections:
        t = c.torch
        o = (t.empty((n, 32), dtype=t.int64, device=c.dev), t.empty(n, dtype=t.int32, device=c.dev), t.empty(n, dtype=t.int32, device=c.dev))
        row = timed(lambda: c.ix.knn_graph_reverse_device(c.f[0].data_ptr(), c.f[2].data_ptr(), K, 32, 0, n, *(x.data_ptr() for x in o)))
        info = c.ix.knn_reverse_info()
        # what the passes move at least: the u64 graph in and the table out, the table twice more (count, fill), the in-neighbours out and in,
        # the offsets out and in, the ids out
        moved = n * K * (8 + 4) + 2 * n * K * 4 + 2 * info["edges"] * 4 + 2 * n * 8 + n * 32 * 8
        deg = o[2].to(t.int64)
        out(case="reverse graph alone", rev_k=32, **row, info=info, kept_over_edges=round(info["kept"] / max(info["edges"], 1), 4),
            bytes_moved_at_least=moved, gb_per_s=round(moved / row["median_ms"] / 1e6, 1),
            degree_quantiles={q: int(t.quantile(deg.float(), q).item()) for q in (0.5, 0.9, 0.99)}, rows_never_named=int((deg == 0).sum().item()))
    if "trace" in sections:
        dst = c.graph()
        row = timed(lambda: c.fused(32, c.f, dst))
        out(case="round 1 at rev_k 32 alone (for the kernel trace)", calls=4, **row, info=c.ix.knn_refine_rev_info())
    c.ix.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576, set((sys.argv[2] if len(sys.argv) > 2 else "rounds,reverse").split(",")),
         int(sys.argv[3]) if len(sys.argv) > 3 else 0, sys.argv[4] if len(sys.argv) > 4 else None)

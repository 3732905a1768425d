"""Timing probe of the forest k-NN graph (zh_knn_graph_forest_device) beside the exact one (zh_knn_graph_device) on the same index in the same
process: 1 048 576 x 768 clustered synthetic rows (append_synthetic(kind=2)), options 4096 / 15, L2SQ, k = 32, device entry points, one warm-up and
3 timed runs each.  Rows of the table in DESIGN.md s17: the exact graph (the yardstick), the forest graph by the path rule (`condition` = its
slowest run is faster than the exact graph's fastest; the ratio; tile products per second of both; recall@32 against the exact graph), the forest
graph with path 1 forced (one run: it is the slow one), the recall on iid rows (kind 0), and a (64, 15) forest with the path rule's choice and with
path 1 forced -- the small-leaf row that decides the rule's threshold.
    python tests/probes/fknn_probe.py [rows] [sections]    (default 1048576 and "exact,forest,path1,iid,small"; any subset, comma separated)"""
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
        self.e = (torch.empty((n, K), dtype=torch.int64, device=dev), torch.empty((n, K), dtype=torch.int64, device=dev),
                  torch.empty(n, dtype=torch.int32, device=dev))
        self.f = tuple(torch.empty_like(t) for t in self.e)

    def exact(self):
        self.ix.knn_graph_device(K, self.m, 0, self.n, *(t.data_ptr() for t in self.e))

    def forest(self):
        self.ix.knn_graph_forest_device(K, self.m, 0, self.n, *(t.data_ptr() for t in self.f))

    def recall(self):
        """share of the exact graph's edges that the forest graph names (both hold ascending (key, id) lines; ids compared as sets per line)"""
        torch = self.torch
        hit = 0
        for r0 in range(0, self.n, 65536):
            e, f = self.e[0][r0:r0 + 65536], self.f[0][r0:r0 + 65536]
            hit += int((e[:, :, None] == f[:, None, :]).any(dim=2).sum().item())
        return round(hit / max(int(self.e[2].sum().item()), 1), 4)


def main(n, sections):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    big = None
    row_exact = None
    if {"exact", "forest", "path1"} & sections:
        big = Case(n, 4096, 15, 2)
        out(case="index", rows=n, dim=D, options=[4096, 15], kind=2, build_ms=big.build_ms)
    if "exact" in sections:
        row_exact = timed(big.exact)
        info = big.ix.knn_info()
        out(case="exact graph (yardstick)", k=K, **row_exact, info=info, tiles_per_s=round(info["tiles"] / row_exact["median_ms"] * 1e3))
    if "forest" in sections:
        row = timed(big.forest)
        info = big.ix.knn_forest_info()
        extra = {}
        if row_exact:
            extra = dict(ratio_exact_over_forest=round(row_exact["median_ms"] / row["median_ms"], 2), condition=bool(row["max_ms"] < row_exact["min_ms"]),
                         recall_at_k=big.recall())
        out(case="forest graph, path rule", k=K, **row, info=info, tiles_per_s=round(info["tiles"] / row["median_ms"] * 1e3),
            survivors_per_line=round(info["survivors"] / max(info["lines"], 1), 1), **extra)
    if "path1" in sections:
        keep = tuple(t.clone() for t in big.f)
        os.environ["ZH_FKNN_PATH"] = "1"
        row = timed(big.forest, 1)
        os.environ.pop("ZH_FKNN_PATH", None)
        agree = bool(all(big.torch.equal(a, b) for a, b in zip(keep, big.f))) if "forest" in sections else None
        out(case="forest graph, path 1 forced", k=K, **row, info=big.ix.knn_forest_info(), agree=agree)
    if big is not None:
        big.ix.close()
        big = None
    if "iid" in sections:
        c = Case(n, 4096, 15, 0)
        row_e, row_f = timed(c.exact, 1), timed(c.forest, 1)
        out(case="iid rows (kind 0)", k=K, exact=row_e, forest=row_f, info=c.ix.knn_forest_info(), recall_at_k=c.recall())
        c.ix.close()
    if "small" in sections:
        c = Case(n, 64, 15, 2)
        row2 = timed(c.forest, 1)
        info2 = c.ix.knn_forest_info()
        keep = tuple(t.clone() for t in c.f)
        os.environ["ZH_FKNN_PATH"] = "1"
        row1 = timed(c.forest, 1)
        os.environ.pop("ZH_FKNN_PATH", None)
        out(case="small leaves (64, 15)", k=K, path_rule=row2, info_path_rule=info2, path1=row1, info_path1=c.ix.knn_forest_info(),
            agree=bool(all(c.torch.equal(a, b) for a, b in zip(keep, c.f))))
        c.ix.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576,
         set((sys.argv[2] if len(sys.argv) > 2 else "exact,forest,path1,iid,small").split(",")))

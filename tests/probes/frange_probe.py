"""Timing probe of the forest range search (zh_search_range_forest_batch_device) beside the exact one (zh_search_range_batch_device) and the LSH
search (zh_search_batch_device, k = 100: the speed yardstick) on the same index in the same process: 1 048 576 x 768 clustered synthetic rows
(append_synthetic(kind=2)), options 4096 / 15, 1024 clustered synthetic queries, L2SQ, device entry points, one warm-up and 3 timed runs each.
Thresholds: each query's own 100th smallest exact key (about 100 exact hits per query).  One JSON line per row of the table in DESIGN.md s19:
the forest search with path 2 forced (ZH_FRANGE_PATH=2) at probe = 1 (hits, the exact search's hits and their quotient, the hit recall of the forest setting; visits,
leaf_rows, candidates, tiles), the same with path 1 forced (one warm-up, one run), the exact range search, the LSH search, and a (64, 15) forest
with path 2 and with path 1 forced.  Smaller `rows` at the same options give fewer, more shared leaves: the rows that place the visit gate.
    python tests/probes/frange_probe.py [rows] [sections]    (default 1048576 and "forest,path1,exact,search,small"; any subset, comma separated)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, B, HITS, PROBE = 768, 1024, 100, 1


def timed(fn, reps=3, warm=True):
    if warm:
        fn()  # warm-up: scratch, the fp16 copy
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(runs=reps, median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


class Case:
    def __init__(self, n, node, trees):
        import torch
        import zebra_amd as za
        from zebra_amd.index import synth_queries_device
        self.torch, self.za, self.n, self.m = torch, za, n, za.L2SquaredDistance()
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(node, trees), device=0)
        self.ix.append_synthetic(n, kind=2)
        t0 = time.perf_counter()
        self.ix.build()
        self.build_ms = round((time.perf_counter() - t0) * 1e3, 1)
        self.dev = torch.device("cuda", 0)
        self.q = torch.empty((B, D), dtype=torch.float32, device=self.dev)
        synth_queries_device(0, self.q.data_ptr(), n, B, D, kind=2)
        torch.cuda.synchronize()
        self.ids = torch.empty((B, HITS), dtype=torch.int64, device=self.dev)
        self.keys, self.counts = torch.empty_like(self.ids), torch.empty(B, dtype=torch.int32, device=self.dev)
        self.ix.search_exact_batch_device(self.q.data_ptr(), B, HITS, self.m, self.ids.data_ptr(), self.keys.data_ptr(), self.counts.data_ptr())
        self.mk = self.keys[:, HITS - 1].contiguous()
        self.off = torch.zeros(B + 1, dtype=torch.int64, device=self.dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.out = None

    def call(self, forest, cap):
        """one range search at capacity `cap` (0: count only) -> the total"""
        ptrs = [t.data_ptr() for t in self.out] if cap else [None, None]
        try:
            if forest:
                self.ix.search_range_forest_batch_device(self.q.data_ptr(), B, self.mk.data_ptr(), PROBE, self.m, cap, self.off.data_ptr(), *ptrs,
                                                         self.total.data_ptr())
            else:
                self.ix.search_range_batch_device(self.q.data_ptr(), B, self.mk.data_ptr(), self.m, cap, self.off.data_ptr(), *ptrs, self.total.data_ptr())
        except self.za.ZhError as e:
            if e.code != -5 or cap:
                raise
        return int(self.total.cpu()[0])

    def room(self, hits):
        self.out = tuple(self.torch.empty(max(hits, 1), dtype=self.torch.int64, device=self.dev) for _ in range(2))


def main(n, sections):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    if {"forest", "path1", "exact", "search"} & sections:
        c = Case(n, 4096, 15)
        out(case="index", rows=n, dim=D, options=[4096, 15], kind=2, queries=B, probe=PROBE, build_ms=c.build_ms)
        exact_hits = c.call(False, 0)
        row2, keep = None, None
        if "forest" in sections:
            os.environ["ZH_FRANGE_PATH"] = "2"  # path 2 whatever the visit gate says: the row measures the path, not the rule
            hits = c.call(True, 0)
            c.room(hits)
            row2 = timed(lambda: c.call(True, hits))
            keep = tuple(t.clone() for t in c.out) + (c.off.clone(),)
            os.environ.pop("ZH_FRANGE_PATH", None)
            out(case="forest range search, path 2 forced", hits=hits, exact_hits=exact_hits, hit_recall=round(hits / max(exact_hits, 1), 4), **row2,
                info=c.ix.range_forest_info())
        if "path1" in sections:
            os.environ["ZH_FRANGE_PATH"] = "1"
            hits = c.call(True, 0)
            c.room(hits)
            row1 = timed(lambda: c.call(True, hits), 1)
            os.environ.pop("ZH_FRANGE_PATH", None)
            agree = bool(all(c.torch.equal(a, b) for a, b in zip(keep, c.out + (c.off,)))) if keep is not None else None
            extra = dict(ratio_path1_over_path2=round(row1["median_ms"] / row2["median_ms"], 2)) if row2 else {}
            out(case="forest range search, path 1 forced", hits=hits, **row1, info=c.ix.range_forest_info(), agree=agree, **extra)
        if "exact" in sections:
            c.room(exact_hits)
            row = timed(lambda: c.call(False, exact_hits))
            extra = dict(ratio_exact_over_forest=round(row["median_ms"] / row2["median_ms"], 2), condition=bool(row2["max_ms"] < row["min_ms"])) if row2 else {}
            out(case="exact range search", hits=exact_hits, hits_per_query=round(exact_hits / B, 1), **row, info=c.ix.range_info(), **extra)
        if "search" in sections:
            row = timed(lambda: (c.ix.search_batch_device(c.q.data_ptr(), B, HITS, c.m, c.ids.data_ptr(), c.keys.data_ptr(), c.counts.data_ptr()),
                                 c.torch.cuda.synchronize()))
            out(case="LSH search, k = 100 (speed yardstick)", **row)
        c.ix.close()
    if "small" in sections:
        c = Case(n, 64, 15)
        exact_hits = c.call(False, 0)
        os.environ["ZH_FRANGE_PATH"] = "2"
        hits = c.call(True, 0)
        c.room(hits)
        row2 = timed(lambda: c.call(True, hits), 1)
        info2 = c.ix.range_forest_info()
        keep = tuple(t.clone() for t in c.out)
        os.environ["ZH_FRANGE_PATH"] = "1"
        row1 = timed(lambda: c.call(True, hits), 1)
        os.environ.pop("ZH_FRANGE_PATH", None)
        out(case="small leaves (64, 15)", build_ms=c.build_ms, hits=hits, exact_hits=exact_hits, hit_recall=round(hits / max(exact_hits, 1), 4),
            path2=row2, info_path2=info2, path1=row1, info_path1=c.ix.range_forest_info(),
            agree=bool(all(c.torch.equal(a, b) for a, b in zip(keep, c.out))))
        c.ix.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576,
         set((sys.argv[2] if len(sys.argv) > 2 else "forest,path1,exact,search,small").split(",")))

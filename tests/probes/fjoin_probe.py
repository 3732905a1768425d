"""Timing probe of the forest self-join (zh_self_join_forest_device) beside the exact one (zh_self_join_device) on the same index in the same
process: 1 048 576 x 768 clustered synthetic rows (append_synthetic(kind=2)), options 4096 / 15, L2SQ, device entry points, one warm-up and 3 timed
runs each.  The threshold is join_probe.py's: the median 21st-nearest key of 1024 rows (the row itself is the first).  Rows of the table in
DESIGN.md s18: the exact join (the yardstick), the forest join by the path rule (`condition` = its slowest run is faster than the exact join's
fastest; the ratio; the pairs found by each and their quotient, the pair recall of the forest setting; leaf_pairs, candidates, tiles; tile
products per second of both), the forest join with path 1 forced (one run, no warm-up: it is the slow one), and a (64, 15) forest under the path
rule and with path 1 forced -- the small-leaf row that decides the rule's threshold.
    python tests/probes/fjoin_probe.py [rows] [sections]    (default 1048576 and "exact,forest,path1,small"; any subset, comma separated)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D = 768


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
        self.torch, self.za, self.n, self.m = torch, za, n, za.L2SquaredDistance()
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(node, trees), device=0)
        self.ix.append_synthetic(n, kind=2)
        t0 = time.perf_counter()
        self.ix.build()
        self.build_ms = round((time.perf_counter() - t0) * 1e3, 1)
        self.dev = torch.device("cuda", 0)
        B, k = 1024, 21
        rows = torch.from_numpy(self.ix.read_rows(0, B)).to(self.dev)
        ids = torch.empty((B, k), dtype=torch.int64, device=self.dev)
        keys, counts = torch.empty_like(ids), torch.empty(B, dtype=torch.int32, device=self.dev)
        self.ix.search_exact_batch_device(rows.data_ptr(), B, k, self.m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
        self.mk = int(np.median(keys.cpu().numpy().view(np.uint64)[:, k - 1]))
        self.total = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.out = None

    def call(self, fn, cap):
        """one call of either join at capacity `cap` (0: count only) -> the total"""
        ptrs = [t.data_ptr() for t in self.out] if cap else [None, None, None]
        try:
            fn(self.mk, self.m, cap, *ptrs, self.total.data_ptr())
        except self.za.ZhError as e:
            if e.code != -5 or cap:
                raise
        return int(self.total.cpu()[0])

    def room(self, pairs):
        self.out = tuple(self.torch.empty(max(pairs, 1), dtype=self.torch.int64, device=self.dev) for _ in range(3))


def main(n, sections):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    if {"exact", "forest", "path1"} & sections:
        c = Case(n, 4096, 15)
        out(case="index", rows=n, dim=D, options=[4096, 15], kind=2, build_ms=c.build_ms, max_key=c.mk)
        row_exact, exact_pairs, forest_keep = None, None, None
        if "exact" in sections:
            exact_pairs = c.call(c.ix.self_join_device, 0)
            c.room(exact_pairs)
            row_exact = timed(lambda: c.call(c.ix.self_join_device, exact_pairs))
            info = c.ix.join_info()
            out(case="exact join (yardstick)", pairs=exact_pairs, pairs_per_row=round(exact_pairs / n, 2), **row_exact, info=info,
                tiles_per_s=round(info["tiles"] / row_exact["median_ms"] * 1e3))
        if "forest" in sections:
            pairs = c.call(c.ix.self_join_forest_device, 0)
            c.room(pairs)
            row = timed(lambda: c.call(c.ix.self_join_forest_device, pairs))
            info = c.ix.join_forest_info()
            forest_keep = tuple(t.clone() for t in c.out)
            extra = {}
            if row_exact:
                extra = dict(ratio_exact_over_forest=round(row_exact["median_ms"] / row["median_ms"], 2), condition=bool(row["max_ms"] < row_exact["min_ms"]),
                             pair_recall=round(pairs / max(exact_pairs, 1), 4))
            out(case="forest join, path rule", pairs=pairs, **row, info=info, tiles_per_s=round(info["tiles"] / row["median_ms"] * 1e3), **extra)
        if "path1" in sections:
            os.environ["ZH_FJOIN_PATH"] = "1"
            pairs = c.call(c.ix.self_join_forest_device, 0) if forest_keep is None else forest_keep[0].numel()
            c.room(pairs)
            row = timed(lambda: c.call(c.ix.self_join_forest_device, pairs), 1, False)
            os.environ.pop("ZH_FJOIN_PATH", None)
            agree = bool(all(c.torch.equal(a, b) for a, b in zip(forest_keep, c.out))) if forest_keep is not None else None
            out(case="forest join, path 1 forced", pairs=pairs, **row, info=c.ix.join_forest_info(), agree=agree)
        c.ix.close()
    if "small" in sections:
        c = Case(n, 64, 15)
        pairs = c.call(c.ix.self_join_forest_device, 0)
        c.room(pairs)
        row2 = timed(lambda: c.call(c.ix.self_join_forest_device, pairs), 1)
        info2 = c.ix.join_forest_info()
        keep = tuple(t.clone() for t in c.out)
        os.environ["ZH_FJOIN_PATH"] = "1"
        row1 = timed(lambda: c.call(c.ix.self_join_forest_device, pairs), 1)
        os.environ.pop("ZH_FJOIN_PATH", None)
        out(case="small leaves (64, 15)", build_ms=c.build_ms, pairs=pairs, path_rule=row2, info_path_rule=info2, path1=row1,
            info_path1=c.ix.join_forest_info(), agree=bool(all(c.torch.equal(a, b) for a, b in zip(keep, c.out))))
        c.ix.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576,
         set((sys.argv[2] if len(sys.argv) > 2 else "exact,forest,path1,small").split(",")))

"""Timing probe of the exact k-NN join between two indexes (zh_cross_knn_device): A = 65 536 and B = 262 144 synthetic rows of 768 dimensions
(disjoint slices of the probe's synthetic rows), L2SQ, k = 32, device entry points.  Rows of the table in DESIGN.md s30: the yardstick -- the
loop the call replaces: A.read_rows in slabs of 16 384 back to the host, the upload of each slab, B.search_exact_batch_device 1024 rows at a
time straight into the answer's arrays -- the call, and the call with path 1 forced (ZH_XKNN_PATH=1, read per call; fewer runs: it is the slow
one); then the same three with A of 4096 rows (the "incoming batch").  One warm-up, then REPS timed runs: median, min and max; `condition` =
the call's slowest run is faster than the loop's fastest and both give the same ids, keys and counts (compared on the device after the timing).
    python tests/probes/xknn_probe.py [rows_a] [rows_b] [call]     (default 65536 262144; "call": the path-rule call alone, for a kernel trace)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = 5
SLAB = 16384  # rows of A read back at a time


def timed(fn, reps=REPS):
    fn()  # warm-up: scratch, the fp16 copies
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(runs=reps, median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


def measure(torch, ia, ib, na, k, m, call_only):
    dev = torch.device("cuda", 0)
    B = 1024
    g_ids = torch.empty((na, k), dtype=torch.int64, device=dev)
    g_keys, g_counts = torch.empty_like(g_ids), torch.empty(na, dtype=torch.int32, device=dev)

    def call():
        ia.cross_knn_device(ib, k, m, 0, na, g_ids.data_ptr(), g_keys.data_ptr(), g_counts.data_ptr())

    if call_only:
        print(json.dumps(dict(case="k-NN join alone", rows_a=na, rows_b=len(ib), k=k, **timed(call, 1), info=ia.cross_knn_info())), flush=True)
        return

    l_ids = torch.empty((na, k), dtype=torch.int64, device=dev)
    l_keys, l_counts = torch.empty_like(l_ids), torch.empty(na, dtype=torch.int32, device=dev)
    survivors = [0]

    def loop():
        survivors[0] = 0
        for s0 in range(0, na, SLAB):
            ns = min(SLAB, na - s0)
            rows = torch.from_numpy(ia.read_rows(s0, ns)).to(dev)
            for b0 in range(0, ns, B):
                nb = min(B, ns - b0)
                ib.search_exact_batch_device(rows[b0:].data_ptr(), nb, k, m, l_ids[s0 + b0:].data_ptr(), l_keys[s0 + b0:].data_ptr(),
                                             l_counts[s0 + b0:].data_ptr())
                survivors[0] += ib.exact_info()["survivors"]
        torch.cuda.synchronize()

    row_loop = timed(loop)
    print(json.dumps(dict(case="loop of read_rows + search_exact_batch_device", rows_a=na, rows_b=len(ib), k=k, **row_loop,
                          survivors_per_line=round(survivors[0] / na, 1), info=ib.exact_info())), flush=True)
    row_call = timed(call)
    info = ia.cross_knn_info()
    agree = bool(torch.equal(g_ids, l_ids) and torch.equal(g_keys, l_keys) and torch.equal(g_counts, l_counts))
    print(json.dumps(dict(case="k-NN join, path rule", **row_call, info=info, survivors_per_line=round(info["survivors"] / max(info["lines"], 1), 1),
                          ratio_loop_over_call=round(row_loop["median_ms"] / row_call["median_ms"], 2),
                          condition=bool(row_call["max_ms"] < row_loop["min_ms"] and agree), agree=agree)), flush=True)
    os.environ["ZH_XKNN_PATH"] = "1"
    g_ids.zero_()
    row_p1 = timed(call, 2)
    agree1 = bool(torch.equal(g_ids, l_ids) and torch.equal(g_keys, l_keys) and torch.equal(g_counts, l_counts))
    print(json.dumps(dict(case="k-NN join, path 1 forced", **row_p1, info=ia.cross_knn_info(), agree=agree1,
                          ratio_loop_over_call=round(row_loop["median_ms"] / row_p1["median_ms"], 2))), flush=True)
    os.environ.pop("ZH_XKNN_PATH", None)


def main(na, nb, call_only=False):
    import torch
    import zebra_amd as za
    d, k = 768, 32
    m = za.L2SquaredDistance()
    ib = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ib.append_synthetic(nb, first_row=na)
    ia = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ia.append_synthetic(na, first_row=0)
    measure(torch, ia, ib, na, k, m, call_only)
    if call_only or na <= 4096:
        return
    small = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    small.append_synthetic(4096, first_row=0)
    measure(torch, small, ib, 4096, k, m, False)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 65_536, int(sys.argv[2]) if len(sys.argv) > 2 else 262_144,
         len(sys.argv) > 3 and sys.argv[3] == "call")

"""Timing probe of the exact join between two indexes (zh_cross_join_device): A = 65 536 and B = 262 144 synthetic rows of 768 dimensions
(disjoint slices of the probe's synthetic rows), L2SQ, device entry points.  The threshold is set so that a row of A has about 10 partners in
B: the median 10th-nearest key in B of 1024 rows of A; the actual pair count is recorded.  Rows of the table in DESIGN.md s20: the yardstick --
what the call replaces: A.read_rows in slabs back to the host, then B.search_range_batch_device 1024 rows at a time, with what its user pays per
batch (the upload of the slab, a torch.repeat_interleave of the A ids over the offsets, the count read back) -- the join, and the join with
path 1 forced (ZH_XJOIN_PATH=1, read per call); then the same three with A of 4096 rows (the "incoming batch": where the gate's 2^25 pairs
stand against the real crossover).  One warm-up, then REPS timed runs: median, min and max; `condition` = the join's slowest run is faster
than the loop's fastest and the pairs are identical (a, b and keys, compared on the device after the timing).
    python tests/probes/xjoin_probe.py [rows_a] [rows_b] [join]     (default 65536 262144; "join": the path-rule join alone, for a kernel trace)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = 5
SLAB = 16384  # rows of A read back at a time


def timed(fn):
    fn()  # warm-up: scratch, the fp16 copies
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


def measure(za, torch, ia, ib, na, mk, m, join_only):
    dev = torch.device("cuda", 0)
    B = 1024
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def join(cap, a, b, kk):
        def call():
            try:
                ia.cross_join_device(ib, mk, m, cap, a.data_ptr() if cap else None, b.data_ptr() if cap else None, kk.data_ptr() if cap else None,
                                     total.data_ptr())
            except za.ZhError as e:
                if e.code != -5 or cap:
                    raise
        return call

    join(0, None, None, None)()
    pairs = int(total.cpu()[0])
    print(json.dumps(dict(case="threshold", rows_a=na, rows_b=len(ib), max_key=mk, pairs=pairs, pairs_per_row_of_a=round(pairs / na, 2),
                          info=ia.cross_info())), flush=True)
    a, b, kk = (torch.empty(max(pairs, 1), dtype=torch.int64, device=dev) for _ in range(3))
    if join_only:
        print(json.dumps(dict(case="cross-join alone", pairs=pairs, **timed(join(pairs, a, b, kk)), info=ia.cross_info())), flush=True)
        return

    # the yardstick: A's rows back to the host in slabs, every row a query on B, 1024 at a time
    cap = 4 * pairs // max(1, na // B) + 64 * B
    rid, rkey = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    offs = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    dmk = torch.full((B,), mk, dtype=torch.int64, device=dev)
    la, lb, lk = (torch.empty(max(pairs, 1), dtype=torch.int64, device=dev) for _ in range(3))
    found = [0]

    def loop():
        kept = 0
        for s0 in range(0, na, SLAB):
            ns = min(SLAB, na - s0)
            rows = torch.from_numpy(ia.read_rows(s0, ns)).to(dev)
            for b0 in range(0, ns, B):
                nb = min(B, ns - b0)
                ib.search_range_batch_device(rows[b0:].data_ptr(), nb, dmk.data_ptr(), m, cap, offs.data_ptr(), rid.data_ptr(), rkey.data_ptr(),
                                             total.data_ptr())
                o = offs[:nb + 1]
                q = torch.repeat_interleave(torch.arange(s0 + b0, s0 + b0 + nb, device=dev), o[1:] - o[:-1])
                n = int(q.numel())  # (one host sync per batch: the user's count)
                if kept + n <= pairs:
                    la[kept:kept + n], lb[kept:kept + n], lk[kept:kept + n] = q, rid[:n], rkey[:n]
                kept += n
        found[0] = kept

    row_loop = timed(loop)
    print(json.dumps(dict(case="loop of read_rows + search_range_batch_device", pairs=found[0], **row_loop, info=ib.range_info())), flush=True)
    row_join = timed(join(pairs, a, b, kk))
    agree = bool(found[0] == pairs and int(total.cpu()[0]) == pairs and torch.equal(a[:pairs], la[:pairs]) and torch.equal(b[:pairs], lb[:pairs]) and
                 torch.equal(kk[:pairs], lk[:pairs]))
    print(json.dumps(dict(case="cross-join, path rule", pairs=int(total.cpu()[0]), **row_join, info=ia.cross_info(),
                          ratio_loop_over_join=round(row_loop["median_ms"] / row_join["median_ms"], 2),
                          condition=bool(row_join["max_ms"] < row_loop["min_ms"] and agree), agree=agree)), flush=True)
    os.environ["ZH_XJOIN_PATH"] = "1"
    row_p1 = timed(join(pairs, a, b, kk))
    print(json.dumps(dict(case="cross-join, path 1 forced", pairs=int(total.cpu()[0]), **row_p1, info=ia.cross_info(),
                          ratio_loop_over_join=round(row_loop["median_ms"] / row_p1["median_ms"], 2))), flush=True)
    os.environ.pop("ZH_XJOIN_PATH", None)


def main(na, nb, join_only=False):
    import torch
    import zebra_amd as za
    d, k = 768, 10
    m = za.L2SquaredDistance()
    ib = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ib.append_synthetic(nb, first_row=na)
    ia = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ia.append_synthetic(na, first_row=0)
    dev = torch.device("cuda", 0)
    q = torch.from_numpy(ia.read_rows(0, 1024)).to(dev)
    ids = torch.empty((1024, k), dtype=torch.int64, device=dev)
    keys, counts = torch.empty_like(ids), torch.empty(1024, dtype=torch.int32, device=dev)
    ib.search_exact_batch_device(q.data_ptr(), 1024, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    mk = int(np.median(keys.cpu().numpy().view(np.uint64)[:, k - 1]))
    measure(za, torch, ia, ib, na, mk, m, join_only)
    if join_only or na <= 4096:
        return
    small = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    small.append_synthetic(4096, first_row=0)
    measure(za, torch, small, ib, 4096, mk, m, False)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 65_536, int(sys.argv[2]) if len(sys.argv) > 2 else 262_144,
         len(sys.argv) > 3 and sys.argv[3] == "join")

"""Timing probe of the exact range search (zh_search_range_batch_device): 10M x 768 synthetic rows, 1024 queries, L2SQ, device entry point.
Thresholds are each query's 100th-nearest key (from zh_search_exact_batch_device, k = 100): about 100 hits per query.  Rows of the table in
DESIGN.md s14: the exact top-100 on the same index in the same process (the yardstick), range path 2, range path 1 forced (ZH_RANGE_PATH=1,
read per call), the exact search's path 1 (Manhattan: it has no matrix-core path), and a dense case -- thresholds scaled until a query has
about 10 000 hits -- on path 2 and with path 1 forced (offsets, sort and output are common to both).  One warm-up call, then REPS timed ones: median,
min and max.
    python tests/probes/range_probe.py [rows]      (default 10M)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = 5


def timed(fn):
    fn()  # warm-up: scratch, the fp16 copy
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2))


def main(n):
    import torch
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    d, B, k = 768, 1024, 100
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    for r0 in range(0, n, 1 << 22):
        ix.append_synthetic(min(1 << 22, n - r0), first_row=r0)
    Q = zo.synth_queries(B, d, n)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.empty_like(ids), torch.empty(B, dtype=torch.int32, device=dev)

    def exact(metric):
        return lambda: ix.search_exact_batch_device(dq.data_ptr(), B, k, metric, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())

    row = timed(exact(m))
    print(json.dumps(dict(case="exact top-100 l2sq", rows=n, **row, info=ix.exact_info())), flush=True)
    top_ids = ids.cpu().numpy().view(np.uint64).copy()
    top_keys = keys.cpu().numpy().view(np.uint64).copy()
    mk100 = top_keys[:, k - 1].copy()

    offs = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def range_call(mk, cap, out_ids, out_keys):
        dmk = torch.from_numpy(mk.view(np.int64)).to(dev)

        def call():
            try:
                ix.search_range_batch_device(dq.data_ptr(), B, dmk.data_ptr(), m, cap, offs.data_ptr(), out_ids.data_ptr() if cap else None,
                                             out_keys.data_ptr() if cap else None, total.data_ptr())
            except za.ZhError as e:
                if e.code != -5 or cap:
                    raise
        return call

    def counted(mk):
        range_call(mk, 0, None, None)()
        return int(total.cpu()[0])

    # about 100 hits per query
    cap = counted(mk100)
    rid, rkey = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    for forced in (None, "1"):
        if forced:
            os.environ["ZH_RANGE_PATH"] = forced
        else:
            os.environ.pop("ZH_RANGE_PATH", None)
        row = timed(range_call(mk100, cap, rid, rkey))
        info = ix.range_info()
        o = offs.cpu().numpy().view(np.uint64)
        got = rid.cpu().numpy().view(np.uint64)
        agree = all((got[int(o[b]):int(o[b]) + k] == top_ids[b]).all() for b in range(B))  # (ties with the 100th key follow it)
        print(json.dumps(dict(case="range ~100 hits/query, path %s" % (forced or "rule"), hits=cap, **row, info=info, top100_agree=bool(agree))), flush=True)
    os.environ.pop("ZH_RANGE_PATH", None)
    row = timed(exact(za.ManhattanDistance()))
    print(json.dumps(dict(case="exact top-100 manhattan (path 1)", **row, info=ix.exact_info())), flush=True)

    # dense: scale the thresholds until a query has about 10 000 hits (L2SQ keys are f64 bit patterns of the distance)
    lo, hi = 1.0, 4.0
    for _ in range(12):
        f = 0.5 * (lo + hi)
        c = counted((mk100.view(np.float64) * f).view(np.uint64))
        lo, hi = (f, hi) if c < 10_000 * B else (lo, f)
    mkd = (mk100.view(np.float64) * hi).view(np.uint64)
    capd = counted(mkd)
    did, dkey = torch.empty(capd, dtype=torch.int64, device=dev), torch.empty(capd, dtype=torch.int64, device=dev)
    for forced in (None, "1"):  # (the sort and the output are common to both: the difference is the scan)
        if forced:
            os.environ["ZH_RANGE_PATH"] = forced
        else:
            os.environ.pop("ZH_RANGE_PATH", None)
        row = timed(range_call(mkd, capd, did, dkey))
        print(json.dumps(dict(case="dense ~10 000 hits/query, path %s" % (forced or "rule"), hits=capd, factor=hi, **row, info=ix.range_info())), flush=True)
    os.environ.pop("ZH_RANGE_PATH", None)
    row = timed(exact(m))
    print(json.dumps(dict(case="exact top-100 l2sq again", **row)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)

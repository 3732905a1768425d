"""Timing probe of the exact self-join (zh_self_join_device): 262 144 x 768 synthetic rows, L2SQ, device entry points.  The threshold is set so
that a row has about 20 partners (about 10 pairs per row): the median 21st-nearest key of 1024 rows (the row itself is the first); the actual
pair count is recorded.  Rows of the table in DESIGN.md s15: the yardstick -- what the join replaces: a loop of search_range_batch_device over
the index's own rows as queries, 1024 at a time, hits kept where id > query (the rows are read back once, outside the timing: the user's second
copy) -- the join, and the join with path 1 forced (ZH_JOIN_PATH=1, read per call).  One warm-up, then REPS timed runs: median, min and max;
`condition` = the join's slowest run is faster than the loop's fastest.
    python tests/probes/join_probe.py [rows] [join]      (default 262144; "join": the path-rule join alone, for a kernel trace of its own)"""
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


def main(n, join_only=False):
    import torch
    import zebra_amd as za
    d, B, k = 768, 1024, 21
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    ix.append_synthetic(n)
    dev = torch.device("cuda", 0)
    rows = torch.from_numpy(ix.read_rows(0, n)).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.empty_like(ids), torch.empty(B, dtype=torch.int32, device=dev)
    ix.search_exact_batch_device(rows.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    mk = int(np.median(keys.cpu().numpy().view(np.uint64)[:, k - 1]))

    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def join(cap, a, b, kk):
        def call():
            try:
                ix.self_join_device(mk, m, cap, a.data_ptr() if cap else None, b.data_ptr() if cap else None, kk.data_ptr() if cap else None, total.data_ptr())
            except za.ZhError as e:
                if e.code != -5 or cap:
                    raise
        return call

    join(0, None, None, None)()
    pairs = int(total.cpu()[0])
    print(json.dumps(dict(case="threshold", rows=n, max_key=mk, pairs=pairs, pairs_per_row=round(pairs / n, 2), info=ix.join_info())), flush=True)

    if join_only:
        a, b, kk = (torch.empty(pairs, dtype=torch.int64, device=dev) for _ in range(3))
        print(json.dumps(dict(case="self-join alone", pairs=pairs, **timed(join(pairs, a, b, kk)), info=ix.join_info())), flush=True)
        return

    # the yardstick: every row a query, 1024 at a time; a hit survives where id > query
    cap = 4 * pairs // max(1, n // B) + 64 * B  # per batch: its rows' hits both ways + themselves, with room
    rid, rkey = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    offs = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    dmk = torch.full((B,), mk, dtype=torch.int64, device=dev)
    found = [0]

    def loop():
        kept = 0
        for b0 in range(0, n, B):
            nb = min(B, n - b0)
            ix.search_range_batch_device(rows[b0:].data_ptr(), nb, dmk.data_ptr(), m, cap, offs.data_ptr(), rid.data_ptr(), rkey.data_ptr(), total.data_ptr())
            o = offs[:nb + 1]
            q = torch.repeat_interleave(torch.arange(b0, b0 + nb, device=dev), o[1:] - o[:-1])
            kept += int((rid[:q.numel()] > q).sum())
        found[0] = kept

    row_loop = timed(loop)
    print(json.dumps(dict(case="loop of search_range_batch_device, id > query kept", pairs=found[0], **row_loop, info=ix.range_info())), flush=True)

    a, b, kk = (torch.empty(pairs, dtype=torch.int64, device=dev) for _ in range(3))
    row_join = timed(join(pairs, a, b, kk))
    print(json.dumps(dict(case="self-join, path rule", pairs=int(total.cpu()[0]), **row_join, info=ix.join_info(),
                          ratio_loop_over_join=round(row_loop["median_ms"] / row_join["median_ms"], 2),
                          condition=bool(row_join["max_ms"] < row_loop["min_ms"]), agree=bool(found[0] == pairs))), flush=True)
    os.environ["ZH_JOIN_PATH"] = "1"
    row_p1 = timed(join(pairs, a, b, kk))
    print(json.dumps(dict(case="self-join, path 1 forced", pairs=int(total.cpu()[0]), **row_p1, info=ix.join_info())), flush=True)
    os.environ.pop("ZH_JOIN_PATH", None)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 262_144, len(sys.argv) > 2 and sys.argv[2] == "join")

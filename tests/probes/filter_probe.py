"""Timing probe of the filtered exact search (zh_search_exact_filtered_batch_device): 10M x 768 synthetic rows, batch 1024, k = 100, L2SQ.
For each allowed fraction -- 1.0, 0.5, 0.1, 0.01, 0.001 at random, and a contiguous 0.1 -- ms per batch with each path forced
(ZH_FILTER_PATH=1|2, read per call) and with the library's own rule, next to the unfiltered zh_search_exact_batch_device on the same index in
the same process.  One warm-up call, then REPS timed ones: median, min and max.  The path rule (ZH_FILTER_PATH2_MIN_DENSITY, zh_api.hip) is
set from this table.
    python tests/probes/filter_probe.py [rows]      (default 10M)"""
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
    unf = timed(lambda: ix.search_exact_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr()))
    unf["info"] = ix.exact_info()
    print(json.dumps(dict(case="unfiltered", rows=n, **unf)), flush=True)
    ref_ids = ids.cpu().numpy().copy()
    rng = np.random.default_rng(1)
    masks = [("random", f, rng.random(n) < f) for f in (1.0, 0.5, 0.1, 0.01, 0.001)]
    contiguous = np.zeros(n, bool)
    contiguous[n // 2:n // 2 + n // 10] = True
    masks.append(("contiguous", 0.1, contiguous))
    for kind, frac, mask in masks:
        words, n_bits = ix.filter_bitmap(mask)
        df = torch.from_numpy(words.view(np.int32)).to(dev)
        call = lambda: ix.search_exact_filtered_batch_device(dq.data_ptr(), B, k, m, df.data_ptr(), n_bits, ids.data_ptr(), keys.data_ptr(),  # noqa: E731
                                                             counts.data_ptr())
        row = dict(case=kind, fraction=frac, rows_allowed=int(mask.sum()))
        answers = {}
        for forced in ("1", "2", None):
            if forced is None:
                os.environ.pop("ZH_FILTER_PATH", None)
            else:
                os.environ["ZH_FILTER_PATH"] = forced
            t = timed(call)
            info = ix.filtered_info()
            answers[forced] = ids.cpu().numpy().copy()
            row["rule" if forced is None else "path" + forced] = dict(
                t, path=info["path"], redone=info["redone"], launches=info["launches"], tiles_skipped=info["tiles_skipped"],
                survivors_per_query=info["survivors"] / B)
        row["paths_agree"] = bool((answers["1"] == answers["2"]).all() and (answers["1"] == answers[None]).all())
        if frac == 1.0:
            row["equals_unfiltered"] = bool((answers[None] == ref_ids).all())
        print(json.dumps(row), flush=True)
    again = timed(lambda: ix.search_exact_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr()))
    print(json.dumps(dict(case="unfiltered_again", **again)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000)

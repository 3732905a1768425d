"""Timing probe of the exact search (zh_search_exact_batch): median ms per batch, exact queries/s, zh_exact_info, and a spot check of 8
queries against the oracle's brute force at reduced N.  One case per invocation, so that every step runs in a process (and under a time
limit) of its own:
    python tests/probes/exact_probe.py l2sq       10M x 768 synthetic rows, batch 1024, k = 100, L2SQ
    python tests/probes/exact_probe.py manhattan  the same batch under the Manhattan metric (keys differ, comparable cost)
    python tests/probes/exact_probe.py d128       1M x 128, batch 1024, k = 100, L2SQ
    python tests/probes/exact_probe.py torch      torch's brute-force GEMM at 10M x 768 (reference; run it LAST, in its own process:
                                                  an index created after torch's GEMMs in the same process scans slower)
Optional second argument: rows (default 10M, 1M for d128)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), ms


def run_index(case, n):
    import torch
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    d = 128 if case == "d128" else 768
    B, k = 1024, 100
    m, om = (za.ManhattanDistance(), zo.MANHATTAN) if case == "manhattan" else (za.L2SquaredDistance(), zo.L2SQ)
    ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    for r0 in range(0, n, 1 << 22):
        ix.append_synthetic(min(1 << 22, n - r0), first_row=r0)
    Q = zo.synth_queries(B, d, n)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(Q).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.empty_like(ids), torch.empty(B, dtype=torch.int32, device=dev)
    call = lambda: ix.search_exact_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
    call()  # warm-up: live-row list, scratch
    _, med, ms = timed(call, 5)
    info = ix.exact_info()
    # spot check at reduced N: 8 queries over the first 200k rows, against the oracle's brute force
    ns = min(n, 200_000)
    small = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
    small.append_synthetic(ns)
    X = zo.synth_rows(ns, d)
    gi, gk, gc = small.search_exact_batch(Q[:8], k, m)
    ok = True
    for b in range(8):
        oi, okk = zo.brute_force(X, Q[b], k, om, 0)
        ok &= bool((gi[b, :len(oi)] == oi).all() and (gk[b, :len(oi)] == okk).all() and gc[b] == len(oi))
    return dict(case=case, rows=n, dim=d, batch=B, k=k, median_ms=round(med, 2), ms=[round(x, 2) for x in ms],
                qps=round(B / (med / 1e3)), info=info, survivors_per_query=info["survivors"] / B, spot_check_8_queries=ok)


def run_torch(n):
    import torch
    d, B, k = 768, 1024, 100
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((n, d), device=dev, generator=g)
    Q = torch.randn((B, d), device=dev, generator=g)
    xn = (X * X).sum(1)
    chunk = 1 << 20

    def once():
        best_v = best_i = None
        for r0 in range(0, n, chunk):
            dd = xn[r0:r0 + chunk][None, :] - 2.0 * (Q @ X[r0:r0 + chunk].T)
            v, i = torch.topk(dd, k, dim=1, largest=False)
            i = i + r0
            if best_v is None:
                best_v, best_i = v, i
            else:
                cv, ci = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
                best_v, j = torch.topk(cv, k, dim=1, largest=False)
                best_i = torch.gather(ci, 1, j)
        torch.cuda.synchronize()
        return best_i
    once()
    _, med, ms = timed(once, 5)
    return dict(case="torch", rows=n, dim=d, batch=B, k=k, median_ms=round(med, 2), ms=[round(x, 2) for x in ms], qps=round(B / (med / 1e3)))


if __name__ == "__main__":
    case = sys.argv[1] if len(sys.argv) > 1 else "l2sq"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else (1_000_000 if case == "d128" else 10_000_000)
    res = run_torch(n) if case == "torch" else run_index(case, n)
    print(json.dumps(res))

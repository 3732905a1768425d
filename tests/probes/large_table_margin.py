"""The separation condition tests/test_gpu_large_table.py rests on, measured on the CPU (no GPU needed; a minute or two on eight cores).

The whole synthetic table of that module (4 198 437 x 1024, kind 2) is regenerated chunk by chunk with zo.synth_rows.  For each of the module's 16
probe queries and each of its three metrics, zo.distance_batch gives the oracle's key of every row; printed per metric: the minimum over the
queries of (smallest key outside the query's cluster) / (largest key inside it).  Above 1 the cluster's 128 rows decide every top-k with
k <= 127 and every radius up to the cluster's largest key.

The exact k-NN graph's slabs ask the same of 768 more queries, the stored rows of the six clusters around rows 2^20, 2^21 and 2^22.  The oracle is
too slow for those, so their ratio comes from f32 matrix products (|x|^2 + |q|^2 - 2 x.q and 1 - x.q / (|x| |q|)): not the oracle's arithmetic,
which does not matter for a ratio this far from 1.  Printed for L2 squared and corrected cosine.

    python tests/probes/large_table_margin.py [threads]      (default 8)"""
import concurrent.futures
import os
import sys
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")  # the chunks run side by side; a matrix product stays on its chunk's thread

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import zebra_oracle as zo  # noqa: E402
from tests.test_gpu_large_table import BOUNDARIES, CL, D, KIND, METRICS, N, oracle_metric, probe_queries  # noqa: E402

CHUNK = 8192  # rows per chunk: 64 whole clusters


def key_numbers(name, keys):
    """the keys as numbers: f64 bits for the L2 family and cosine, f32 bits in the low word for the other metrics"""
    return zo.key_to_float(keys) if oracle_metric(name)[0] < zo.CHEBYSHEV else keys.astype(np.uint32).view(np.float32).astype(np.float64)


def scan(r0, Q, cl, L, lcl):
    """one chunk -> per (metric, probe query) [min outside, max inside] and per (l2sq | cos, line) the same from matrix products"""
    n = min(CHUNK, N - r0)
    X = zo.synth_rows(n, D, row0=r0, kind=KIND)
    cluster = (np.arange(r0, r0 + n) // CL)
    out = np.empty((len(METRICS), Q.shape[0], 2))
    for mi, name in enumerate(METRICS):
        om, omode = oracle_metric(name)
        for b in range(Q.shape[0]):
            k = key_numbers(name, zo.distance_batch(om, omode, X, Q[b]))
            inside = cluster == cl[b]
            out[mi, b] = (k[~inside].min() if (~inside).any() else np.inf, k[inside].max() if inside.any() else -np.inf)
    G = X @ L.T
    x2, l2 = np.einsum("ij,ij->i", X, X), np.einsum("ij,ij->i", L, L)
    inside = cluster[:, None] == lcl[None, :]
    lines = np.empty((2, L.shape[0], 2))
    for j, K in enumerate((x2[:, None] + l2[None, :] - 2.0 * G, 1.0 - G / np.sqrt(x2[:, None] * l2[None, :]))):
        lines[j, :, 0] = np.where(inside, np.inf, K).min(axis=0)
        lines[j, :, 1] = np.where(inside, K, -np.inf).max(axis=0)
    return out, lines


def main(threads):
    Q, cl = probe_queries()
    L = np.concatenate([zo.synth_rows(2 * CL, D, row0=b - CL, kind=KIND) for b in BOUNDARIES])
    lrows = np.concatenate([np.arange(b - CL, b + CL) for b in BOUNDARIES])
    lcl = lrows // CL
    worst = np.empty((len(METRICS), Q.shape[0], 2))
    worst[..., 0], worst[..., 1] = np.inf, -np.inf
    lworst = np.empty((2, L.shape[0], 2))
    lworst[..., 0], lworst[..., 1] = np.inf, -np.inf
    t0, done = time.perf_counter(), 0
    starts = list(range(0, N, CHUNK))
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        for out, lines in pool.map(lambda r0: scan(r0, Q, cl, L, lcl), starts):
            worst[..., 0], worst[..., 1] = np.minimum(worst[..., 0], out[..., 0]), np.maximum(worst[..., 1], out[..., 1])
            lworst[..., 0], lworst[..., 1] = np.minimum(lworst[..., 0], lines[..., 0]), np.maximum(lworst[..., 1], lines[..., 1])
            done += 1
            if done % 64 == 0:
                print("  %d / %d chunks, %.0f s" % (done, len(starts), time.perf_counter() - t0), file=sys.stderr, flush=True)
    print("%d x %d rows scanned in %.0f s; min over the queries of (smallest outside key) / (largest inside key):" % (N, D, time.perf_counter() - t0))
    for mi, name in enumerate(METRICS):
        ratio = worst[mi, :, 0] / worst[mi, :, 1]
        print("  %-10s probe queries  %.3f   (query %d; per query: %s)" % (name, ratio.min(), int(ratio.argmin()), " ".join("%.2f" % r for r in ratio)))
    for j, name in enumerate(("l2sq", "cos")):
        ratio = lworst[j, :, 0] / lworst[j, :, 1]
        print("  %-10s graph lines    %.3f   (row %d; f32 matrix products)" % (name, ratio.min(), int(lrows[ratio.argmin()])))
    return 0 if min((worst[..., 0] / worst[..., 1]).min(), (lworst[..., 0] / lworst[..., 1]).min()) > 1.0 else 1


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 8))

"""Timing and recall probe of filter-steered graph search (zh_search_graph_steered_batch) on tests/probes/gfilter_probe.py's table and method:
rows x 768 synthetic rows (append_synthetic(kind=0): iid; kind 2: clustered), options 4096 / 15, L2SQ, the graph = knn_graph_forest then
knn_graph_descent(k = 32, 8 rounds), attached with set_graph_device; 1024 planted queries per batch, top_k = 10, everything in device memory;
every arm of one process alternated, one warm-up and 3 timed runs each, median and range (DESIGN.md s28's table).

Per selectivity s in {1, 0.5, 0.1, 0.01} (s = 1: every row allowed; otherwise gfilter_probe's random mask, each row allowed with probability s)
and beam in {64, 256} at width 4, all from the same 32 seeds strided over the mask's set positions (a steered walk drops a disallowed seed):

  blind b           search_graph_filtered_batch_device: the walk through every row, answered from the allowed rows it keyed
  hops1 b           search_graph_steered_batch_device, hops = 1
  hops2 b           search_graph_steered_batch_device, hops = 2
  exact filtered    search_exact_filtered_batch_device on the same mask: the ground truth of the recall, and the time to beat

and once per beam `graph b`: search_graph_batch_device at the same settings -- against the steered arms at s = 1 (the same answer) the cost of
the steered kernel.  Per arm it prints ms per batch, recall@10 against the exact filtered arm, and per query keyed, via_bridge, bridges,
cand_full and iterations.  The index is created before any torch GEMM (INTEGRATION section 9's order effect): nothing here runs one.

    python tests/probes/gsteer_probe.py [rows] [kind] [library]   (default 1048576 0, the built library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests.probes.graph_search_probe import B, D, K, N_SEED, TOP, alternate, recall  # noqa: E402

SELECTIVITIES, BEAMS, WIDTH = (1.0, 0.5, 0.1, 0.01), (64, 256), 4
KINDS = ("blind", "hops1", "hops2")


def main(n, kind):
    import torch
    import zebra_amd as za
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    m = za.L2SquaredDistance()
    ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
    ix.append_synthetic(n, kind=kind)
    ix.build()
    dev = torch.device("cuda", 0)
    graph = lambda: (torch.empty((n, K), dtype=torch.int64, device=dev), torch.empty((n, K), dtype=torch.int64, device=dev),  # noqa: E731
                     torch.empty(n, dtype=torch.int32, device=dev))
    f, g = graph(), graph()
    ix.knn_graph_forest_device(K, m, 0, n, *(t.data_ptr() for t in f))
    ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), K, 0, K, 8, m, *(t.data_ptr() for t in g))
    ix.set_graph_device(g[0].data_ptr(), g[2].data_ptr(), n, K)
    out(case="index", rows=n, dim=D, options=[4096, 15], kind=kind, k=K, descent=ix.knn_descent_info()["rounds_run"], graph=ix.graph_info())
    del f, g

    q = torch.empty((B, D), dtype=torch.float32, device=dev)
    za.synth_queries_device(0, q.data_ptr(), n, B, D, kind=kind)
    res = lambda: (torch.empty((B, TOP), dtype=torch.int64, device=dev), torch.empty((B, TOP), dtype=torch.int64, device=dev),  # noqa: E731
                   torch.empty(B, dtype=torch.int32, device=dev))
    rng = np.random.default_rng([0x6F117E2, n, kind])  # (gfilter_probe's masks)
    arms, outs, calls, masks = {}, {}, {}, {}
    for s in SELECTIVITIES:
        mask = np.ones(n, bool) if s == 1.0 else rng.random(n) < s
        words, n_bits = ix.filter_bitmap(mask)
        rows = np.flatnonzero(mask)
        own = torch.from_numpy(rows[[j * rows.size // N_SEED for j in range(N_SEED)]].astype(np.int64)[None, :].repeat(B, 0)).to(dev)
        fw = torch.from_numpy(words.view(np.int32)).to(dev)
        masks[s] = (fw, n_bits, own, int(rows.size))
        outs[("exact", s)] = res()
        arms["exact filtered %g" % s] = (lambda s=s: ix.search_exact_filtered_batch_device(q.data_ptr(), B, TOP, m, masks[s][0].data_ptr(), masks[s][1],
                                                                                            *(t.data_ptr() for t in outs[("exact", s)])))
        for b in BEAMS:
            for hops, name in enumerate(KINDS):
                key = (s, b, name)
                outs[key] = res()
                if hops == 0:
                    calls[key] = (lambda s=s, b=b, key=key: ix.search_graph_filtered_batch_device(
                        q.data_ptr(), B, masks[s][2].data_ptr(), N_SEED, TOP, m, masks[s][0].data_ptr(), masks[s][1], *(t.data_ptr() for t in outs[key]),
                        beam=b, width=WIDTH))
                else:
                    calls[key] = (lambda s=s, b=b, key=key, hops=hops: ix.search_graph_steered_batch_device(
                        q.data_ptr(), B, masks[s][2].data_ptr(), N_SEED, TOP, m, masks[s][0].data_ptr(), masks[s][1], *(t.data_ptr() for t in outs[key]),
                        hops=hops, beam=b, width=WIDTH))
                arms["%s %d %g" % (name, b, s)] = calls[key]
    strided = masks[1.0][2]
    for b in BEAMS:
        outs[("graph", b)] = res()
        arms["graph %d" % b] = (lambda b=b: ix.search_graph_batch_device(q.data_ptr(), B, strided.data_ptr(), N_SEED, TOP, m,
                                                                         *(t.data_ptr() for t in outs[("graph", b)]), beam=b, width=WIDTH))
    torch.cuda.synchronize()
    row = alternate(arms)
    for b in BEAMS:
        out(case="graph", beam=b, width=WIDTH, **row["graph %d" % b])
    for s in SELECTIVITIES:
        exact_ms = row["exact filtered %g" % s]["median_ms"]
        out(case="exact filtered", selectivity=s, rows_allowed=masks[s][3], **row["exact filtered %g" % s])
        for b in BEAMS:
            for name in KINDS:
                key = (s, b, name)
                calls[key]()
                info = ix.search_graph_filtered_info() if name == "blind" else ix.search_graph_steered_info()
                t = row["%s %d %g" % (name, b, s)]
                same = None
                if s == 1.0 and name != "blind":
                    same = all(bool((x == y).all().item()) for x, y in zip(outs[key], outs[("graph", b)]))
                out(case=name, selectivity=s, beam=b, width=WIDTH, recall=recall(outs[("exact", s)], outs[key]), keyed_per_query=round(info["keyed"] / B, 1),
                    via_bridge_per_query=round(info.get("via_bridge", 0) / B, 1), bridges_per_query=round(info.get("bridges", 0) / B, 1),
                    cand_full_per_query=round(info.get("cand_full", 0) / B, 2), iterations_per_query=round(info["iterations"] / B, 2),
                    returned_per_query=round(info["returned"] / B, 2), over_exact=round(t["median_ms"] / exact_ms, 3),
                    over_graph=round(t["median_ms"] / row["graph %d" % b]["median_ms"], 3) if s == 1.0 else None, equals_graph=same, **t)
    ix.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) > 2:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(a[2])
    main(int(a[0]) if len(a) > 0 else 1_048_576, int(a[1]) if len(a) > 1 else 0)

"""Timing and recall probe of the graph extension (zh_index_extend_graph) against the rebuild it replaces, on tests/probes/graph_search_probe.py's
table: rows x 768 synthetic rows (append_synthetic kind 0: iid; kind 2: clustered), options 4096 / 15, L2SQ, k = 32.  The graph is built
(knn_graph_forest, knn_graph_descent with 8 rounds, set_graph_device) on the first rows - appended rows, the rest is appended and the forest built
again (not timed: the LSH search and the rebuild both need it).  Everything stays in device memory.  Arms, alternated, one warm-up and 3 timed
runs each; every extend arm attaches the base graph again first (not timed):

  extend 256 / 1024   extend_graph_device at that batch (`batches`), beam 64, width 1, 32 seeds per new row
  extend + descent    the same at the last batch, then get_graph_device, one knn_graph_descent_device round over the table, set_graph_device
  rebuild             knn_graph_forest_device + knn_graph_descent_device (8 rounds) + set_graph_device over all rows

Seeds: kind 0 the strided rows of the old graph (LSHIndex.extend_graph's default); kind 2 the LSH search's 32 best rows of every new row, made
once and timed on its own ("lsh seeds"): strided seeds find nothing on the clustered table.  The queries' seeds follow the same
rule.  Recall@10 of search_graph_batch_device (beam 64 and 256, width 4) against search_exact_batch_device for 1024 queries planted at
appended rows (the row plus 0.01 of noise), in these states: the base graph, after each extend, after extend + descent, after the rebuild.
On the clustered table 128 consecutive rows share a centre, so the appended rows are 512 clusters of their own: a new row's nearest rows are
its cluster-mates, which can be named only if an EARLIER chunk holds them -- batches below 128 (32,64) are the ones to run there.

    python tests/probes/gextend_probe.py [rows] [kind] [appended] [batches] [library]   (default 1048576 0 65536 256,1024, the built library)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, K, B, TOP, N_SEED, BEAM = 768, 32, 1024, 10, 32, 64


def main(n, kind, n_new, batches):
    import torch
    import zebra_amd as za
    from tests.probes.graph_search_probe import recall
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    m = za.L2SquaredDistance()
    G = n - n_new
    dev = torch.device("cuda", 0)
    ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
    ix.append_synthetic(G, kind=kind)
    ix.build()
    graph = lambda rows: (torch.empty((rows, K), dtype=torch.int64, device=dev), torch.empty((rows, K), dtype=torch.int64, device=dev),  # noqa: E731
                          torch.empty(rows, dtype=torch.int32, device=dev))
    f, base = graph(n), graph(G)
    ix.knn_graph_forest_device(K, m, 0, G, *(t.data_ptr() for t in f))
    ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), K, 0, K, 8, m, *(t.data_ptr() for t in base))
    attach_base = lambda: ix.set_graph_device(base[0].data_ptr(), base[2].data_ptr(), G, K)  # noqa: E731
    attach_base()
    ix.append_synthetic(n_new, first_row=G, kind=kind)
    t0 = time.perf_counter()
    ix.build()
    out(case="index", rows=n, appended=n_new, dim=D, kind=kind, k=K, forest_rebuild_ms=round((time.perf_counter() - t0) * 1e3, 1), graph=ix.graph_info())

    # the queries: appended rows, each moved a little; their seeds and the new rows' seeds
    fresh = torch.from_numpy(ix.read_rows(G, n_new)).to(dev)
    rng = np.random.default_rng(20261021)
    pick = torch.from_numpy(rng.permutation(n_new)[:B]).to(dev)
    q = (fresh[pick] + 0.01 * torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).to(dev)).contiguous()
    strided = lambda b, rows: torch.from_numpy((np.arange(N_SEED, dtype=np.int64) * rows // N_SEED)[None, :].repeat(b, 0)).to(dev)  # noqa: E731
    junk = (torch.empty((4096, N_SEED), dtype=torch.int64, device=dev), torch.empty(4096, dtype=torch.int32, device=dev))

    def lsh_seeds(rows_t):
        sd = torch.empty((rows_t.shape[0], N_SEED), dtype=torch.int64, device=dev)
        for r0 in range(0, rows_t.shape[0], 4096):
            b = min(4096, rows_t.shape[0] - r0)
            ix.search_batch_device(rows_t[r0:].data_ptr(), b, N_SEED, m, sd[r0:].data_ptr(), junk[0].data_ptr(), junk[1].data_ptr())
        torch.cuda.synchronize()
        return sd

    if kind == 2:
        t0 = time.perf_counter()
        new_seeds = lsh_seeds(fresh)
        out(case="lsh seeds", rows=n_new, ms=round((time.perf_counter() - t0) * 1e3, 1))
        q_seeds = lambda: lsh_seeds(q)  # noqa: E731
    else:
        new_seeds = strided(n_new, G)
        q_seeds = lambda: strided(B, ix.graph_info()["g_rows"])  # noqa: E731
    del fresh

    res = lambda: (torch.empty((B, TOP), dtype=torch.int64, device=dev), torch.empty((B, TOP), dtype=torch.int64, device=dev),  # noqa: E731
                   torch.empty(B, dtype=torch.int32, device=dev))
    exact = res()
    ix.search_exact_batch_device(q.data_ptr(), B, TOP, m, *(t.data_ptr() for t in exact))
    appended_in_truth = float(((exact[0] >= G) & (exact[0] != -1)).sum().item()) / max(int(exact[2].sum().item()), 1)

    def state(name):
        sd = q_seeds()
        for beam in (64, 256):
            o = res()
            ix.search_graph_batch_device(q.data_ptr(), B, sd.data_ptr(), N_SEED, TOP, m, *(t.data_ptr() for t in o), beam=beam, width=4)
            out(case="recall", state=name, beam=beam, width=4, recall=recall(exact, o), appended_share_of_truth=round(appended_in_truth, 4),
                appended_share_of_answer=round(float((o[0] >= G).sum().item()) / max(int(o[2].sum().item()), 1), 4), g_rows=ix.graph_info()["g_rows"])

    def extend(batch):
        attach_base()
        t = time.perf_counter()
        ix.extend_graph_device(new_seeds.data_ptr(), n_new, N_SEED, m, beam=BEAM, width=1, batch=batch)
        return (time.perf_counter() - t) * 1e3

    g_all, d_out = graph(n), graph(n)
    gi = (torch.empty((n, K), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev))

    def extend_descent():
        ms = extend(batches[-1])
        t = time.perf_counter()
        ix.get_graph_device(0, n, gi[0].data_ptr(), gi[1].data_ptr())
        ix.knn_graph_descent_device(gi[0].data_ptr(), gi[1].data_ptr(), K, 0, K, 1, m, *(t_.data_ptr() for t_ in d_out))
        ix.set_graph_device(d_out[0].data_ptr(), d_out[2].data_ptr(), n, K)
        return ms + (time.perf_counter() - t) * 1e3

    def rebuild():
        t = time.perf_counter()
        ix.knn_graph_forest_device(K, m, 0, n, *(t_.data_ptr() for t_ in f))
        ix.knn_graph_descent_device(f[0].data_ptr(), f[2].data_ptr(), K, 0, K, 8, m, *(t_.data_ptr() for t_ in g_all))
        ix.set_graph_device(g_all[0].data_ptr(), g_all[2].data_ptr(), n, K)
        return (time.perf_counter() - t) * 1e3

    state("before")
    # the arms time themselves: an extend arm's attach of the base graph is outside its clock
    arms = {"extend %d" % b: (lambda b=b: extend(b)) for b in batches}
    arms.update({"extend + descent": extend_descent, "rebuild": rebuild})
    ms = {name: [] for name in arms}
    for rep in range(4):  # the first pass is the warm-up
        for name, fn in arms.items():
            v = fn()
            if rep:
                ms[name].append(v)
            if rep == 0 and name.startswith("extend ") and name != "extend + descent":
                out(case="extend info", arm=name, **ix.extend_graph_info())
                state("after " + name)
            if rep == 0 and name == "extend + descent":
                out(case="descent round", **{k: v2 for k, v2 in ix.knn_descent_info().items() if k in ("rounds_run", "updates", "keyed")})
                state("after extend %d + one descent round" % batches[-1])
            if rep == 0 and name == "rebuild":
                state("after rebuild")
            out(case="pass", rep=rep, arm=name, ms=round(v, 1))
    for name, v in ms.items():
        out(case="time", arm=name, median_ms=round(float(np.median(v)), 1), min_ms=round(min(v), 1), max_ms=round(max(v), 1))
    ix.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) > 4:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(a[4])
    main(int(a[0]) if len(a) > 0 else 1_048_576, int(a[1]) if len(a) > 1 else 0, int(a[2]) if len(a) > 2 else 65_536,
         [int(b) for b in (a[3] if len(a) > 3 else "256,1024").split(",")])

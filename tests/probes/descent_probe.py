"""Timing probe of NN-descent on the device (zh_knn_graph_descent) beside the loops it replaces, on tests/probes/refine_probe.py's setup: 1 048 576 x
768 synthetic rows (append_synthetic(kind=0): iid; kind 2: clustered), options 4096 / 15, L2SQ, k = in_k = 32, over the forest graph.  Arms, alternated,
one warm-up and 3 timed runs each (DESIGN.md s23's table):

  host loop      LSHIndex.knn_graph_refine(rounds=R, reverse=) -- the loop as users have it: every round through the host
  device loop    zh_knn_graph_refine[_rev]_device round by round, graph and outputs in device memory, one info read per round for the early stop:
                 what leaving the device costs is the difference to the host loop, what re-keying costs the difference to the next arm
  descent dev    zh_knn_graph_descent_device
  descent host   zh_knn_graph_descent (the host entry: the graph up once, the answer down once)

Per setting it prints the arms' median and range, keyed_round beside the loop's per-round keyed, and -- section "recall" -- recall@32 against the
exact graph round by round; the descent's answer after r rounds is asserted equal, id for id, to the device loop's round r, so the recall is the
same in both arms by construction.

    python tests/probes/descent_probe.py [rows] [kind] [rounds,..] [reverse,..] [sections] [library]   (default 1048576 0 3,8 0,8 times, the built library)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

D, K = 768, 32


class Case:
    def __init__(self, n, kind):
        import torch
        import zebra_amd as za
        self.torch, self.n, self.m = torch, n, za.L2SquaredDistance()
        self.ix = za.LSHIndex(D, za.LSHIndexOptions(4096, 15), device=0)
        self.ix.append_synthetic(n, kind=kind)
        self.ix.build()
        self.dev = torch.device("cuda", 0)
        self.f = self.graph()
        self.ix.knn_graph_forest_device(K, self.m, 0, n, *(t.data_ptr() for t in self.f))
        self.f_host = (self.f[0].cpu().numpy().view(np.uint64), self.f[2].cpu().numpy().view(np.uint32))
        self.a, self.b, self.d = self.graph(), self.graph(), self.graph()

    def graph(self):
        t, n = self.torch, self.n
        return (t.empty((n, K), dtype=t.int64, device=self.dev), t.empty((n, K), dtype=t.int64, device=self.dev), t.empty(n, dtype=t.int32, device=self.dev))

    def host_loop(self, rounds, rev):
        self.ix.knn_graph_refine(self.f_host, K, self.m, rounds=rounds, reverse=rev)

    def device_loop(self, rounds, rev, keep=None):
        """-> the per-round infos; keep(r, graph) sees every round's output"""
        src, dst, infos = self.f, self.a, []
        for r in range(rounds):
            if rev:
                self.ix.knn_graph_refine_rev_device(src[0].data_ptr(), src[2].data_ptr(), K, rev, K, self.m, 0, self.n, *(t.data_ptr() for t in dst))
                infos.append(self.ix.knn_refine_rev_info())
            else:
                self.ix.knn_graph_refine_device(src[0].data_ptr(), src[2].data_ptr(), K, K, self.m, 0, self.n, *(t.data_ptr() for t in dst))
                infos.append(self.ix.knn_refine_info())
            if keep:
                keep(r, dst)
            if infos[-1]["updates"] == 0:
                break
            src, dst = dst, (self.b if dst is self.a else self.a)
        return infos

    def descent_dev(self, rounds, rev):
        self.ix.knn_graph_descent_device(self.f[0].data_ptr(), self.f[2].data_ptr(), K, rev, K, rounds, self.m, *(t.data_ptr() for t in self.d))

    def descent_host(self, rounds, rev):
        self.ix.knn_graph_descent(self.f_host, K, self.m, rounds=rounds, reverse=rev)

    def recall(self, e, g):
        hit = 0
        for r0 in range(0, self.n, 65536):
            x, y = e[0][r0:r0 + 65536], g[0][r0:r0 + 65536]
            hit += int(((x[:, :, None] == y[:, None, :]) & (x[:, :, None] != -1)).any(dim=2).sum().item())
        return round(hit / max(int(e[2].sum().item()), 1), 4)


def alternate(arms, reps=3):
    """one warm-up of every arm, then reps passes over all of them in turn -> {arm: median, min, max in ms}"""
    ms = {name: [] for name in arms}
    for name, fn in arms.items():
        fn()
    for _ in range(reps):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(median_ms=round(float(np.median(v)), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2)) for name, v in ms.items()}


def main(n, kind, rounds_list, rev_list, sections):
    out = lambda **kw: print(json.dumps(kw), flush=True)  # noqa: E731
    c = Case(n, kind)
    out(case="index", rows=n, dim=D, options=[4096, 15], kind=kind, k=K)
    exact = None
    if "recall" in sections:
        exact = c.graph()
        c.ix.knn_graph_device(K, c.m, 0, n, *(t.data_ptr() for t in exact))
        out(case="recall@%d of the forest graph" % K, recall=c.recall(exact, c.f))
    for rev in rev_list:
        for rounds in rounds_list:
            arms = {"device loop": lambda: c.device_loop(rounds, rev), "descent dev": lambda: c.descent_dev(rounds, rev)}
            if "host" in sections:
                arms.update({"host loop": lambda: c.host_loop(rounds, rev), "descent host": lambda: c.descent_host(rounds, rev)})
            row = alternate(arms)
            recalls = []

            def keep(r, g):
                c.descent_dev(r + 1, rev)
                assert c.torch.equal(g[0], c.d[0]) and c.torch.equal(g[1], c.d[1]) and c.torch.equal(g[2], c.d[2]), "round %d differs" % (r + 1)
                if exact is not None:
                    recalls.append(c.recall(exact, g))

            infos = c.device_loop(rounds, rev, keep)
            c.descent_dev(rounds, rev)
            info = c.ix.knn_descent_info()
            out(case="rounds %d reverse %d" % (rounds, rev), arms=row, rounds_run=info["rounds_run"], keyed_round=info["keyed_round"],
                loop_keyed=[i["keyed"] for i in infos], active_round=info["active_round"], updates_round=info["updates_round"],
                large_lines=info["large_lines"], launches=info["launches"], recall_by_round=recalls)
            assert info["updates_round"] == [i["updates"] for i in infos]
    c.ix.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) > 5:
        from zebra_amd import _ffi
        _ffi.LIB_PATH = os.path.abspath(a[5])
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    main(int(a[0]) if len(a) > 0 else 1_048_576, int(a[1]) if len(a) > 1 else 0, ints(a[2]) if len(a) > 2 else [3, 8], ints(a[3]) if len(a) > 3 else [0, 8],
         set((a[4] if len(a) > 4 else "times").split(",")))

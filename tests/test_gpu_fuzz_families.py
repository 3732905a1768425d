"""Seeded fuzz of the nine exact and forest query families against ONE matrix of oracle keys per metric (tests/family_cases.py has the plan,
the references and the path rule; tests/test_family_reference.py pins them on the CPU).

A seed builds one index (and a second one for the cross join), removes rows down to its live target, and runs the nine families in a shuffled
order under three metrics -- on wide seeds two matrix-core metrics and one of the other nine -- then applies one mutation (remove / add / append /
compact / build) and runs a second shuffled round under one metric.  Every call is compared bit for bit with the reference (ids, keys, counts,
offsets, dtypes, totals) and must report the path family_cases.expected_path names with redone == 0: a seed that passes by falling back fails.
The two joins are checked three ways: against the oracle on sampled rows a, in full against the same call forced to path 1, and the total
against the count-only entry point.  The forest self-join is checked on the sampled rows against the oracle and IN FULL against the exact
self-join's pairs (checked just before, at the same threshold) that are leaf-mates in get_forest()'s arrays: keying every leaf pair on the
CPU (18 M pairs at max_node_size 1024 and four trees) is what a per-seed budget of seconds rules out.

ZH_FUZZ_FAMILY_SEEDS=first:count chooses the seeds (default 0:20); <seed>:1 reproduces one seed alone -- every assertion message carries the
seed, round, family, metric, override and the family's info dict.  The closing test recounts from what ran that every family reported path 2
with redone == 0 at every (D, KINDA) the plans of the seeds that ran promise, and prints how many seeds that asked for a scan row order got one.

Measured on an MI355X (pytest --durations, one run): the slowest default seed takes 1.01 s against 0.66 s for the slowest single-family case,
tests/test_gpu_join.py::test_path2_every_dimension[1024]; the budget is twice that, 1.32 s (a seed runs nine families on a table of the same
size).  With 32 slab lines and 32 sampled rows a the slowest seed took 1.36 s against 0.67 s: both were cut to 16, the shapes kept.  All 20
seeds take under 12 s."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import family_cases as fc  # noqa: E402

_first, _count = (int(x) for x in os.environ.get("ZH_FUZZ_FAMILY_SEEDS", "0:20").split(":"))
SEEDS = range(_first, _first + _count)

_ran_path2 = {}     # (family, d, kinda) -> calls that reported path 2 with redone == 0
_ran_seeds = []     # seeds that completed
_row_orders = {}    # seed that asked for a row order -> stats()["scan_order_keys"] once round 1 was done
_seconds = {}       # seed -> wall seconds
_where = {}         # seed -> {family or "reference": seconds}
INFO = {"exact": "exact_info", "filtered": "filtered_info", "range": "range_info", "join": "join_info", "cross": "cross_info", "knn": "knn_info",
        "fknn": "knn_forest_info", "fjoin": "join_forest_info", "frange": "range_forest_info"}


def za_metric(za, spec):
    name = spec["name"]
    if name in ("minkowski", "pnorm"):
        return (za.MinkowskiDistance if name == "minkowski" else za.PNormDistance)(spec["omode"])
    if name.startswith("cos_"):
        return za.CosineDistance(parity=name == "cos_parity")
    return {"l2sq": za.L2SquaredDistance, "l2": za.L2Distance, "chebyshev": za.ChebyshevDistance, "canberra": za.CanberraDistance,
            "bray_curtis": za.BrayCurtisDistance, "manhattan": za.ManhattanDistance, "l3": za.L3Distance, "l4": za.L4Distance,
            "hamming": za.HammingDistance}[name]()


def same(got, ref, names, ctx):
    for g, r, what in zip(got, ref, names):
        assert g.dtype == r.dtype and g.shape == r.shape, ctx("%s: got %s %s, want %s %s" % (what, g.dtype, g.shape, r.dtype, r.shape))
        if not (g == r).all():
            at = np.argwhere(g != r)[0].tolist()
            raise AssertionError(ctx("%s: first difference at %s, got %d, want %d, %d differ" % (what, at, g[tuple(at)], r[tuple(at)], int((g != r).sum()))))


def in_join_order(got, ctx):
    a, b, k = got
    assert (np.lexsort((b, k, a)) == np.arange(a.size)).all(), ctx("not ascending by (a, key, b)")


class Seed:
    """one seed's indexes and the reference's own state of them"""

    def __init__(self, za, p, monkeypatch):
        self.za, self.p, self.mp = za, p, monkeypatch
        self.X = fc.build_rows(p)
        self.alive = fc.initial_alive(p)
        self.Q = fc.build_queries(p, self.X)
        self.XB = fc.more_rows(p, p["b_rows"], 2)
        self.XB[5], self.XB[6] = self.X[3], self.X[100]  # rows the two indexes share
        self.aliveB = fc.second_alive(p)
        self.base, self.baseB = p["id_base"], p["b_id_base"]
        self.round, self.call, self.spec, self.ov = 0, None, None, None
        for env, _ in fc.PATH_ENV.values():
            if env:
                monkeypatch.delenv(env, raising=False)
        for env in ("ZH_KNN_LIST_CAP", "ZH_FKNN_LIST_CAP", "ZH_FJOIN_CAND_CAP", "ZH_FRANGE_CAND_CAP", "ZH_WALK_LOG_CHUNKS", "ZH_ROW_HALF_META_ONLY"):
            monkeypatch.delenv(env, raising=False)
        monkeypatch.setenv("ZH_ROW_ORDER", str(p["row_order"]))  # (0: id order, whatever the library would measure)
        self.ix = za.LSHIndex(p["d"], za.LSHIndexOptions(p["max_node_size"], p["num_trees"]), seed=p["index_seed"], device=0, id_base=self.base)
        self.ixb = za.LSHIndex(p["d"], za.LSHIndexOptions(64, 1), device=0, id_base=self.baseB)
        self.where = {}

    def clock(self, what, t0):
        self.where[what] = self.where.get(what, 0.0) + time.perf_counter() - t0

    def fill(self):
        p, ix = self.p, self.ix
        ids = ix.add(self.X)
        assert (ids == np.arange(p["n_rows"], dtype=np.uint64) + np.uint64(self.base)).all(), self.ctx()
        gone = np.flatnonzero(~self.alive).astype(np.uint64) + np.uint64(self.base)
        assert ix.remove(gone).size == gone.size, self.ctx()
        self.ixb.append(self.XB)
        self.ixb.remove(np.flatnonzero(~self.aliveB).astype(np.uint64) + np.uint64(self.baseB))
        if p["row_order"]:  # the copy made by one matrix-core scan first, in the forced order
            ix.set_sweep_mode("approx")
            ix.search_batch(zo.synth_queries(8, p["d"], p["n_rows"]), 10, self.za.L2Distance())
            ix.set_sweep_mode("auto")

    def close(self):
        self.ix.close()
        self.ixb.close()

    def info(self):
        return getattr(self.ix, INFO[self.call])() if self.call else None

    def ctx(self, what=""):
        """a plain string: pytest abbreviates any other object in an assertion's message"""
        return "%s %s" % (what, {"seed": self.p["seed"], "round": self.round, "family": self.call, "metric": self.spec and (self.spec["name"], self.spec["omode"]),
                "override": self.ov, "info": self.info(), "d": self.p["d"], "live": int(self.alive.sum()), "stored": int(self.alive.size),
                "reproduce": "ZH_FUZZ_FAMILY_SEEDS=%d:1" % self.p["seed"]})

    def env(self, family, value):
        name = fc.PATH_ENV[family][0]
        if name:
            if value is None:
                self.mp.delenv(name, raising=False)
            else:
                self.mp.setenv(name, str(value))

    def on_path(self, info, want):
        assert info["path"] == want and info["redone"] == 0, self.ctx("expected path %d, redone 0" % want)
        if want == 2:
            key = (self.call, self.p["d"], self.spec["kinda"])
            _ran_path2[key] = _ran_path2.get(key, 0) + 1

    # ------------------------------------------------------------------------------------------------ a round
    def run_round(self, round_no, specs, calls):
        p, ix = self.p, self.ix
        self.round, self.call = round_no, None
        live = int(self.alive.sum())
        assert len(ix) == live and ix.stored_rows() == self.alive.size, self.ctx()
        st = fc.round_setup(p, round_no, self.alive)
        forest = ix.get_forest()
        leaf_of = fc.leaf_table(forest, self.alive.size)
        assert not (leaf_of[:, ~self.alive] >= 0).any(), self.ctx("a removed row is in a leaf")
        slab, sample = st["slab"], st["sample"]
        self.st, self.leaf_of = st, leaf_of
        self.vis = fc.visited_mask(self.X, p["max_node_size"], forest, self.Q, p["probe"])
        self.mates_slab, self.mates_sample = fc.mates_mask(leaf_of, slab), fc.mates_mask(leaf_of, sample)
        B = p["B"]
        Qall = np.concatenate([self.Q, self.X[slab], self.X[sample]])
        for mi, spec in enumerate(specs):
            self.spec, self.m = spec, za_metric(self.za, spec)
            t0 = time.perf_counter()
            K = fc.key_matrix(spec, self.X, Qall)
            self.KQ, self.KS, self.KA = K[:B], K[B:B + slab.size], K[B + slab.size:]
            self.KB = fc.key_matrix(spec, self.XB, self.X[sample])
            upper = self.alive[None, :] & (np.arange(self.alive.size)[None, :] > sample[:, None])
            self.join_key = fc.quantile_threshold(self.KA, upper, p["want_pairs"], live * (live - 1) / 2)
            self.cross_key = fc.quantile_threshold(self.KB, self.aliveB[None, :], p["want_pairs"], live * int(self.aliveB.sum()))
            self.join_got = self.fjoin_got = None
            self.clock("reference", t0)
            order = calls[mi % len(calls):] + calls[:mi % len(calls)]  # the plan's shuffled order, begun one call later per metric
            for c in order:
                self.call = c["family"]
                self.ov = fc.plan_override(p, self.call, spec, c["override"], round_no)
                self.env(self.call, self.ov)
                t0 = time.perf_counter()
                getattr(self, "do_" + self.call)()
                self.clock(self.call, t0)
                self.env(self.call, None)
            self.call = None

    def want_path(self, **kw):
        p = self.p
        return fc.expected_path(self.call, p["d"], self.spec, self.ov, live=int(self.alive.sum()), k=p["k"], max_node_size=p["max_node_size"], **kw)

    # ------------------------------------------------------------------------------------------------ the nine families
    def do_exact(self):
        p = self.p
        got = self.ix.search_exact_batch(self.Q, p["k"], self.m)
        same(got, fc.topk_ref(self.KQ, self.alive, p["k"], self.base), ("ids", "keys", "counts"), self.ctx)
        info = self.ix.exact_info()
        assert info["batch"] == p["B"] and info["rows_live"] == int(self.alive.sum()), self.ctx()
        self.on_path(info, self.want_path())

    def do_filtered(self):
        p, st = self.p, self.st
        ok = st["allowed"] & self.alive
        got = self.ix.search_exact_filtered_batch(self.Q, p["k"], self.m, st["allowed_arg"])
        same(got, fc.topk_ref(self.KQ, ok, p["k"], self.base), ("ids", "keys", "counts"), self.ctx)
        info = self.ix.filtered_info()
        assert info["rows_allowed"] == int(ok.sum()) and info["rows_live"] == int(self.alive.sum()) and info["batch"] == p["B"], self.ctx()
        self.on_path(info, self.want_path(allowed=int(ok.sum()), tile_rule=fc.filter_tile_rule(ok)))

    def do_range(self):
        thr = fc.range_thresholds(self.KQ, self.alive, self.spec, self.st["rng"])
        ref = fc.range_ref(self.KQ, self.alive, thr, self.base)
        got = self.ix.search_range_batch(self.Q, metric=self.m, max_keys=thr, capacity=int(ref[0][-1]))  # (room for exactly the reference's total: one call)
        same(got, ref, ("offsets", "ids", "keys"), self.ctx)
        info = self.ix.range_info()
        assert info["hits"] == ref[1].size and info["batch"] == self.p["B"], self.ctx()
        self.on_path(info, self.want_path())
        assert (self.ix.range_count_batch(self.Q, metric=self.m, max_keys=thr) == np.diff(ref[0])).all(), self.ctx("count only")

    def _three_ways(self, call, count, info, ref_lines, sample, want):
        """a join: the oracle on the sampled rows a, in full against path 1 forced, the total against the count-only entry point"""
        got = call()
        inf = info()
        assert inf["pairs"] == got[0].size, self.ctx()
        self.on_path(inf, want)
        in_join_order(got, self.ctx)
        same(fc.restrict(got, sample, self.base), ref_lines, ("a", "b", "keys"), self.ctx)
        assert count() == got[0].size, self.ctx("count only")
        if want == 2:
            self.env(self.call, 1)
            forced = call()
            assert info()["path"] == 1, self.ctx("forced to path 1")
            same(forced, got, ("a", "b", "keys"), self.ctx)
            self.env(self.call, self.ov)
        return got

    def do_join(self):
        ix, m, mk, sample = self.ix, self.m, self.join_key, self.st["sample"]
        ref = fc.join_ref(self.KA, sample, self.alive, self.alive, mk, self.base, self.base, True)
        got = self._three_ways(lambda: ix.self_join(metric=m, max_key=mk), lambda: ix.self_join_count(metric=m, max_key=mk), ix.join_info,
                               ref, sample, self.want_path())
        assert (got[0] < got[1]).all(), self.ctx()
        self.join_got = got
        self._fjoin_in_full()

    def do_cross(self):
        ix, ixb, m, mk, sample = self.ix, self.ixb, self.m, self.cross_key, self.st["sample"]
        ref = fc.join_ref(self.KB, sample, self.alive, self.aliveB, mk, self.base, self.baseB, False)
        self._three_ways(lambda: ix.cross_join(ixb, metric=m, max_key=mk), lambda: ix.cross_join_count(ixb, metric=m, max_key=mk), ix.cross_info,
                         ref, sample, self.want_path(live_b=int(self.aliveB.sum())))
        inf = ix.cross_info()
        assert inf["rows_live_a"] == int(self.alive.sum()) and inf["rows_live_b"] == int(self.aliveB.sum()), self.ctx()

    def do_knn(self):
        p, st = self.p, self.st
        got = self.ix.knn_graph(p["k"], self.m, st["first_row"], p["slab_lines"])
        same(got, fc.graph_ref(self.KS, st["slab"], self.alive, p["k"], self.base), ("ids", "keys", "counts"), self.ctx)
        info = self.ix.knn_info()
        assert info["lines"] == int(self.alive[st["slab"]].sum()) and info["rows_live"] == int(self.alive.sum()) and info["k"] == p["k"], self.ctx()
        self.on_path(info, self.want_path())

    def do_fknn(self):
        p, st = self.p, self.st
        got = self.ix.knn_graph_forest(p["k"], self.m, st["first_row"], p["slab_lines"])
        same(got, fc.graph_ref(self.KS, st["slab"], self.alive, p["k"], self.base, mates=self.mates_slab), ("ids", "keys", "counts"), self.ctx)
        info = self.ix.knn_forest_info()
        assert info["lines"] == int((self.leaf_of[:, st["slab"]] >= 0).any(0).sum()) and info["k"] == p["k"], self.ctx()
        self.on_path(info, self.want_path())

    def do_fjoin(self):
        ix, m, mk, sample = self.ix, self.m, self.join_key, self.st["sample"]
        ref = fc.join_ref(self.KA, sample, self.alive, self.mates_sample, mk, self.base, self.base, True)
        self.fjoin_got = self._three_ways(lambda: ix.self_join_forest(metric=m, max_key=mk), lambda: ix.self_join_forest_count(metric=m, max_key=mk),
                                          ix.join_forest_info, ref, sample, self.want_path())
        self.fjoin_ctx = self.ctx()
        self._fjoin_in_full()

    def _fjoin_in_full(self):
        """the forest self-join in full: the exact self-join's pairs at the same threshold (do_join checks them three ways) that are leaf-mates;
        run by whichever of the two families comes second in the round's order"""
        if self.join_got is None or self.fjoin_got is None:
            return
        a, b, k = self.join_got
        keep = fc.are_mates(self.leaf_of, a - np.uint64(self.base), b - np.uint64(self.base))
        same(self.fjoin_got, (a[keep], b[keep], k[keep]), ("a", "b", "keys"), lambda what: "the forest self-join in full, %s %s" % (what, self.fjoin_ctx))

    def do_frange(self):
        p = self.p
        thr = fc.range_thresholds(self.KQ, self.vis, self.spec, self.st["rng"])
        ref = fc.range_ref(self.KQ, self.vis, thr, self.base)
        got = self.ix.search_range_forest_batch(self.Q, metric=self.m, max_keys=thr, probe=p["probe"], capacity=int(ref[0][-1]))
        same(got, ref, ("offsets", "ids", "keys"), self.ctx)
        info = self.ix.range_forest_info()
        assert info["hits"] == ref[1].size and info["batch"] == p["B"] and info["probe"] == p["probe"], self.ctx()
        self.on_path(info, self.want_path())
        assert (self.ix.range_forest_count_batch(self.Q, metric=self.m, max_keys=thr, probe=p["probe"]) == np.diff(ref[0])).all(), self.ctx("count only")

    # ------------------------------------------------------------------------------------------------ the mutation
    def mutate(self):
        p, ix = self.p, self.ix
        self.round, self.call, self.spec, self.ov = "mutation " + p["mutation"], None, None, None
        n = self.alive.size
        if p["mutation"] == "remove":  # a whole 16-row tile, every third row of another, the last live row
            live = np.flatnonzero(self.alive)
            gone = np.array([r for r in list(range(160, 176)) + list(range(192, 208, 3)) + [int(live[-1])] if self.alive[r]], np.int64)
            gone = np.unique(gone)
            assert ix.remove(gone.astype(np.uint64) + np.uint64(self.base)).size == gone.size, self.ctx()
            self.alive[gone] = False
        elif p["mutation"] in ("add", "append"):  # (appended rows are in no tree)
            Xn = fc.more_rows(p, p["mutation_rows"], 1)
            ids = (ix.add if p["mutation"] == "add" else ix.append)(Xn)
            assert (ids == np.arange(n, n + Xn.shape[0], dtype=np.uint64) + np.uint64(self.base)).all(), self.ctx()
            self.X = np.concatenate([self.X, Xn])
            self.alive = np.concatenate([self.alive, np.ones(Xn.shape[0], bool)])
        elif p["mutation"] == "compact":
            new_ids, _ = ix.compact()
            assert new_ids.dtype == np.uint64 and (new_ids == fc.compact_map(self.alive, self.base)).all(), self.ctx()
            self.X = np.ascontiguousarray(self.X[self.alive])
            self.alive = np.ones(self.X.shape[0], bool)
        elif p["mutation"] == "build":
            ix.build()
        else:
            raise ValueError(p["mutation"])


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_families(seed, monkeypatch):
    import zebra_amd as za
    t0 = time.perf_counter()
    p = fc.plan(seed)
    S = Seed(za, p, monkeypatch)
    try:
        S.fill()
        S.run_round(1, p["metrics"], p["round1"])
        if p["row_order"]:
            _row_orders[seed] = int(S.ix.stats()["scan_order_keys"])
        S.mutate()
        S.run_round(2, [p["metrics"][p["round2_metric"]]], p["round2"])
    finally:
        S.close()
    _ran_seeds.append(seed)
    _seconds[seed] = time.perf_counter() - t0
    _where[seed] = {k: round(v, 3) for k, v in S.where.items()}


def test_fuzz_families_were_exercised():
    """recounted from what ran: every family on path 2 with redone == 0 at every (D, KINDA) the plans of the seeds that ran promise"""
    if not _ran_seeds:
        pytest.skip("no family seeds completed in this process")
    promised = fc.coverage(_ran_seeds)[0]
    missing = sorted(promised - set(_ran_path2))
    got_order = {s: k for s, k in _row_orders.items() if k != 0}
    print("family fuzz: %d seeds, %d (family, D, KINDA) on path 2; row order asked by %d seeds, kept by %d (%s); slowest seed %s"
          % (len(_ran_seeds), len(_ran_path2), len(_row_orders), len(got_order), sorted(_row_orders.items()),
             max(_seconds.items(), key=lambda kv: kv[1]) if _seconds else None))
    print("family fuzz: where the slowest seed's seconds went:", _where.get(max(_seconds, key=_seconds.get)) if _seconds else None)
    assert not missing, missing
    if set(fc.DEFAULT_SEEDS) <= set(_ran_seeds):
        need = {(f, d, k) for f in fc.FAMILIES for d in fc.MFMA_DIMS for k in range(3)}
        assert need <= set(_ran_path2), sorted(need - set(_ran_path2))
        assert got_order, ("no seed that asked for a scan row order got one", _row_orders)

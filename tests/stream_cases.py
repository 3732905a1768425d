"""The one case of the caller's-stream tests and its references (no GPU, no library: numpy and the oracle only).

tests/test_gpu_caller_stream.py enters every `_device` entry point on a side stream that still has work pending: the copies that bring the
call's real inputs, and fills of its outputs.  What the call must answer is fixed here, once, from tests/family_cases.py's builders and
references; tests/test_stream_cases.py asserts on the CPU that the case keeps the promises the GPU protocol relies on.

The case is the smallest at which both paths of all nine families still run:

  d = 256 (the smallest matrix-core dimension), L2 squared (matrix-core) and Manhattan (one of the other nine: path 1 whatever the shape)
  8407 stored rows (the last 16-row tile is partial), removed down to exactly fc.GATE_ROWS = 8192 live rows
  a forest of 4 trees, max_node_size 256 (>= fc.GATE_NODE), built by the oracle over all rows, the removed rows then taken out of it
  24 queries (one full and one partial 16-query tile), k = 10, probe = 3, a graph slab of 48 lines from row 104 (it holds the removed tile 112 .. 127)
  a LEFT index of 300 rows (9 removed) for the cross join, which has the large index on its right; path 2 is forced (the 2^25-pair gate is far)
  a filter that allows every live row and arbitrary removed ones: 8192 allowed live rows, the gate's own edge, and the tile rule holds

exact, filtered, range, frange, knn, fknn and cross are computed in full; join and fjoin on 16 sampled rows a, as the fuzz does (the GPU test adds
equality with the host entry point's answer on a twin index, in full).  Thresholds come from fc.range_thresholds / fc.quantile_threshold; a
query that fc.range_thresholds leaves without a hit (a threshold of 0, or one below the smallest key) gets fc.quantile_threshold's key of its
own line instead, so that EVERY line of a range answer differs from what a threshold of 0 -- the stale input of the protocol -- would give."""
import functools

import numpy as np

from oracle import zebra_oracle as zo
from tests import family_cases as fc

PLAN = {"seed": 1000, "narrow": False, "power": 0, "d": 256, "n_rows": 8407, "live_target": fc.GATE_ROWS, "max_node_size": 256, "num_trees": 4,
        "row_order": 0, "id_base": 1 << 40, "row_kind": 0, "plant_integers": True, "plant_zero": True, "no_zero_elements": False,
        "row_seed": zo.SEED_ROWS + 1000, "index_seed": zo.SEED_INDEX + 1000, "B": 24, "k": 10, "probe": 3, "slab_lines": 48, "slab_at": "removed",
        "sample_a": 16, "filter_kinds": ["live", "live"], "b_rows": 300, "b_removed": 9, "b_id_base": (1 << 41) + 5, "want_pairs": 3000,
        "data_seed": 20261019}
METRICS = ("l2sq", "manhattan")  # the matrix-core metric and the other one
# how a steady-state call is run: on path 2 (L2 squared, the path rule or the documented override), forced to path 1 through fc.PATH_ENV (L2
# squared; the exact search has no switch), and under the other metric (path 1 by the rule)
MODES = ("path2", "forced1", "other")
SHORT = ("range", "frange", "join", "fjoin", "cross")  # the families with a capacity


def mode_metric(mode):
    return METRICS[1] if mode == "other" else METRICS[0]


def mode_override(family, mode):
    """the value of the family's path switch under `mode` (None: not set)"""
    if mode == "forced1":
        return 1
    if mode == "path2" and family in ("cross", "frange"):  # the pair gate is far away; the visitor gate is the device's (fc.plan_override)
        return 2
    return None


def steady_calls():
    """(family, mode) of every steady-state call: all nine families under every mode that exists for them"""
    return [(f, m) for f in fc.FAMILIES for m in MODES if not (m == "forced1" and fc.PATH_ENV[f][0] is None)]


class Refs:
    """one metric's references; every array is made once and never written again"""


class Case:
    def __init__(self):
        p = self.p = dict(PLAN)
        self.X = fc.build_rows(p)
        self.alive = fc.initial_alive(p)
        self.gone = np.flatnonzero(~self.alive).astype(np.uint64)
        self.Q = fc.build_queries(p, self.X)
        self.XL = fc.more_rows(p, p["b_rows"], 2)
        self.XL[5], self.XL[6] = self.X[3], self.X[100]  # rows the two indexes share
        self.aliveL = fc.second_alive(p)
        self.goneL = np.flatnonzero(~self.aliveL).astype(np.uint64)
        self.base, self.baseL = p["id_base"], p["b_id_base"]
        st = fc.round_setup(p, 1, self.alive)
        self.allowed_arg, self.allowed = st["allowed_arg"], st["allowed"]
        self.allowed_live = self.allowed & self.alive
        self.first_row, self.slab, self.sample = st["first_row"], st["slab"], st["sample"]
        # the forest: the oracle's over all stored rows, the removed rows taken out of every tree
        f = zo.Forest.build(self.X, p["max_node_size"], p["num_trees"], seed=p["index_seed"])
        assert f.remove(self.gone).all()
        self.forest = f.arrays()
        self.leaf_of = fc.leaf_table(self.forest, p["n_rows"])
        self.vis = fc.visited_mask(self.X, p["max_node_size"], self.forest, self.Q, p["probe"])
        self.mates_slab, self.mates_sample = fc.mates_mask(self.leaf_of, self.slab), fc.mates_mask(self.leaf_of, self.sample)
        self.lsh = f.search_batch(self.Q, p["k"], zo.L2SQ, 0)  # the LSH search's answer on this forest, LOCAL ids
        self.refs = {name: self._refs(i, fc.metric_spec(name)) for i, name in enumerate(METRICS)}
        for a in list(vars(self).values()) + [v for r in self.refs.values() for v in vars(r).values()]:
            for x in (a if isinstance(a, tuple) else (a,)):
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)

    def _thresholds(self, K, mask, spec, rng):
        thr = fc.range_thresholds(K, mask, spec, rng)
        mask = np.broadcast_to(mask, K.shape)
        for i in range(K.shape[0]):
            if not (mask[i] & (K[i] <= thr[i])).any():
                thr[i] = fc.quantile_threshold(K[i:i + 1], mask[i:i + 1], 1 + 3 * i, int(mask[i].sum()))
        return thr

    def _refs(self, mi, spec):
        p, r = self.p, Refs()
        B, k, slab, sample, alive = p["B"], p["k"], self.slab, self.sample, self.alive
        r.spec = spec
        K = fc.key_matrix(spec, self.X, np.concatenate([self.Q, self.X[slab], self.X[sample]]))
        r.KQ, r.KS, r.KA = K[:B], K[B:B + slab.size], K[B + slab.size:]
        r.KX = fc.key_matrix(spec, self.X, self.XL)  # [left rows, stored rows]: the large index's row against the left index's row as the query
        rng = np.random.default_rng([p["data_seed"], 77, mi])
        r.exact = fc.topk_ref(r.KQ, alive, k, self.base)
        r.filtered = fc.topk_ref(r.KQ, self.allowed_live, k, self.base)
        r.range_thr = self._thresholds(r.KQ, alive, spec, rng)
        r.range = fc.range_ref(r.KQ, alive, r.range_thr, self.base)
        r.frange_thr = self._thresholds(r.KQ, self.vis, spec, rng)
        r.frange = fc.range_ref(r.KQ, self.vis, r.frange_thr, self.base)
        r.knn = fc.graph_ref(r.KS, slab, alive, k, self.base)
        r.fknn = fc.graph_ref(r.KS, slab, alive, k, self.base, mates=self.mates_slab)
        live = int(alive.sum())
        upper = alive[None, :] & (np.arange(alive.size)[None, :] > sample[:, None])
        r.join_key = fc.quantile_threshold(r.KA, upper, p["want_pairs"], live * (live - 1) / 2)
        r.join = fc.join_ref(r.KA, sample, alive, alive, r.join_key, self.base, self.base, True)
        r.fjoin = fc.join_ref(r.KA, sample, alive, self.mates_sample, r.join_key, self.base, self.base, True)
        rect = self.aliveL[:, None] & alive[None, :]
        r.cross_key = fc.quantile_threshold(r.KX, rect, p["want_pairs"], int(rect.sum()))
        r.cross = fc.join_ref(r.KX, np.arange(p["b_rows"]), self.aliveL, alive, r.cross_key, self.baseL, self.base, False)
        # the capacity-short calls run with total - 1.  range, frange and cross: the total is this reference's own.  The two joins are known here
        # on the sampled rows only: their pairs less one is a LOWER BOUND of the capacity the GPU test uses (the whole answer's total - 1, from
        # the host entry point on the twin), pinned here so that the call is known to be short and to have room for a pair
        r.short_cap = {"range": int(r.range[0][-1]) - 1, "frange": int(r.frange[0][-1]) - 1, "cross": r.cross[0].size - 1,
                       "join": r.join[0].size - 1, "fjoin": r.fjoin[0].size - 1}
        r.least_total = {"range": int(r.range[0][-1]), "frange": int(r.frange[0][-1]), "cross": r.cross[0].size, "join": r.join[0].size,
                         "fjoin": r.fjoin[0].size}
        return r

    def expected_path(self, family, mode):
        p = self.p
        live, live_l = int(self.alive.sum()), int(self.aliveL.sum())
        return fc.expected_path(family, p["d"], self.refs[mode_metric(mode)].spec, mode_override(family, mode), live=live_l if family == "cross" else live,
                                allowed=int(self.allowed_live.sum()), k=p["k"], max_node_size=p["max_node_size"], live_b=live,
                                tile_rule=fc.filter_tile_rule(self.allowed_live))


@functools.lru_cache(maxsize=1)
def case():
    return Case()

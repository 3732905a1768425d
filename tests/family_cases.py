"""The plan and the plain reference of the family fuzz (no GPU, no library: numpy and the oracle only).

Nine query families answer with the exact search's keys: search_exact_batch, search_exact_filtered_batch, search_range_batch, self_join, cross_join,
knn_graph, knn_graph_forest, self_join_forest and search_range_forest_batch.  Every answer is a MASK and an ORDER over one matrix of oracle keys
K[i, r] = oracle.distance_batch(stored row r, query i), where a query is a real query, a stored row, or a row of a second index:

  top-k   the first k entries of the mask by (key, id)              a filter        one more mask
  range   key <= the query's threshold, by (key, id)                a join / graph  the same with a stored row as the query
  forest  the mask is the line's leaf-mates, or the members of the leaves the walk visits, from get_forest()'s arrays

so one pass of distance_batch per metric serves all nine families of a seed.  The references below are those few lines of numpy;
tests/test_family_reference.py pins each against a Python-loop restatement on a tiny case, tests/test_gpu_fuzz_families.py runs the library
against them.

plan(seed) is a pure function of the seed and says everything a seed does: shapes, rows, removals, forest, metrics, the order of the calls, the
path override of each call, the mutation between the two rounds.  expected_path(...) is the path each call MUST report, from the gates written in
include/zebra_hip.h and the reference's own counts; the GPU test asserts it, so a seed cannot pass by falling back.  Two gates depend on what
only the device knows, and there the plan forces the path: the filter's tile-cost rule under a scan row order (its tiles are counted in that
order) and the forest range search's visitor count (ZH_FRANGE_PATH is always 1 or 2 where path 2 is possible).

Wide seeds walk (dimension, pair of matrix-core metrics) round-robin, so that every family meets every one of the 15 (D, KINDA) instantiations
on path 2 by construction; the seeds whose live rows sit at 8191 or whose leaves are too small for the forest kernels are placed so that they
never take the only seed of a combination (coverage(seeds) recounts it; the CPU test asserts it).  In round 1 a call is left to the path rule or
forced to path 2 where the header documents that; forcing path 1 is round 2's (and the joins' own path-2-against-path-1 check).

NOT FED: NaN or infinite values.  A NaN's sign differs between host and device and would decide key <= threshold; key_matrix asserts that no
reference key is a NaN, and the plan leaves the zero row and the zero query out when the third metric is Canberra or Bray-Curtis (0 / 0),
keeps Canberra off the integer-valued rows and, under Canberra, replaces the exact 0.0 elements the generators draw now and then (two rows with
a zero in the same column are 0 / 0 as well: a seed of the default range met that at 10 010 rows of 1024 dimensions)."""
import concurrent.futures

import numpy as np

from oracle import zebra_oracle as zo

ALL = np.uint64(2**64 - 1)
GONE = ALL  # compact()'s id of a removed row
FAMILIES = ("exact", "filtered", "range", "join", "cross", "knn", "fknn", "fjoin", "frange")
MFMA_DIMS = (256, 384, 512, 768, 1024)
NARROW_DIMS = (1, 3, 30, 100, 128, 200, 500, 1000)
GATE_ROWS = 8192          # exact / filtered / range / join / knn: live (allowed) rows from which path 2 serves
GATE_PAIRS = 1 << 25      # cross join: live(A) x live(B) from which path 2 serves without an override
GATE_NODE = 64            # forest families: max_node_size from which path 2 serves
FILTER_ROW_COST = 5.75    # the filter's measured rule: 16 * loaded tiles + skipped tiles <= this * allowed rows
MUTATIONS = ("remove", "add", "append", "compact", "build")
# the environment switch of each family's path (None: the family has none) and whether "2" is a documented value (include/zebra_hip.h; the
# filter's: DESIGN.md s13)
PATH_ENV = {"exact": (None, False), "filtered": ("ZH_FILTER_PATH", True), "range": ("ZH_RANGE_PATH", False), "join": ("ZH_JOIN_PATH", False),
            "cross": ("ZH_XJOIN_PATH", True), "knn": ("ZH_KNN_PATH", False), "fknn": ("ZH_FKNN_PATH", False), "fjoin": ("ZH_FJOIN_PATH", False),
            "frange": ("ZH_FRANGE_PATH", True)}

# name -> (oracle metric, cosine mode or None where `power` goes, KINDA of the matrix-core kernels or None)
METRICS = {"l2sq": (zo.L2SQ, 0, 0), "l2": (zo.L2, 0, 0), "cos_corrected": (zo.COSINE, zo.CORRECTED, 1), "cos_parity": (zo.COSINE, zo.PARITY, 2),
           "chebyshev": (zo.CHEBYSHEV, 0, None), "canberra": (zo.CANBERRA, 0, None), "bray_curtis": (zo.BRAY_CURTIS, 0, None),
           "manhattan": (zo.MANHATTAN, 0, None), "l3": (zo.L3, 0, None), "l4": (zo.L4, 0, None), "hamming": (zo.HAMMING, 0, None),
           "minkowski": (zo.MINKOWSKI, None, None), "pnorm": (zo.PNORM, None, None)}
MFMA_METRICS = ("l2sq", "l2", "cos_corrected", "cos_parity")
OTHER_METRICS = tuple(m for m in METRICS if m not in MFMA_METRICS)
# the pair of matrix-core metrics of a wide seed, by its group: KINDA {0, 1}, {2, 0}, {1, 2}: every KINDA twice per dimension in 15 wide seeds
PAIRS = (("l2sq", "cos_corrected"), ("cos_parity", "l2"), ("cos_corrected", "cos_parity"))
DEFAULT_SEEDS = range(0, 20)
NEAR = 24  # planted near-duplicate pairs (i, 100 + i)


def metric_spec(name, power=0):
    om, mode, kinda = METRICS[name]
    return {"name": name, "om": om, "omode": power if mode is None else mode, "kinda": kinda}


def is_parity(spec):
    return spec["name"] == "cos_parity"


# ---------------------------------------------------------------------------------------------------------------- the plan
def _calls(rng, round_no, narrow):
    """a shuffled order of the nine families, each with its override: None (the path rule), 1 or 2"""
    out = []
    for fam in [FAMILIES[i] for i in rng.permutation(len(FAMILIES))]:
        env, two = PATH_ENV[fam]
        choices = [None]
        if env and two:
            choices.append(2)
        if env and (round_no == 2 or narrow):
            choices.append(1)
        out.append({"family": fam, "override": choices[int(rng.integers(0, len(choices)))]})
    return out


def plan(seed):
    seed = int(seed)
    rng = np.random.default_rng([0xFA111E5, seed])
    narrow = seed % 5 == 4
    w = seed - seed // 5 - (1 if narrow else 0)  # the wide seeds' own counter: 0, 1, 2, 3, (narrow), 4, ...
    power = int(rng.integers(-4, 9))
    other = OTHER_METRICS[seed % len(OTHER_METRICS)]  # the other nine in turn: nine consecutive seeds run all thirteen keys
    p = {"seed": seed, "narrow": narrow, "power": power}
    if narrow:
        p["d"] = int(NARROW_DIMS[(seed // 5) % len(NARROW_DIMS)])
        names = [MFMA_METRICS[i] for i in rng.permutation(4)[:2]] + [other]
        p["n_rows"] = int(rng.integers(600, 1400))
        p["live_target"] = p["n_rows"] - int(rng.integers(30, 200))
        p["max_node_size"] = int((16, 64, 5, 256)[(seed // 5) % 4])
        p["row_order"] = 0
    else:
        p["d"] = int(MFMA_DIMS[w % 5])
        names = list(PAIRS[(w // 5) % 3]) + [other]
        live_mode = w % 4  # 0: exactly 8192 live, 1: exactly 8191, else several hundred above the gate
        live = GATE_ROWS if live_mode == 0 else GATE_ROWS - 1 if live_mode == 1 else GATE_ROWS + int(rng.integers(500, 1500))
        n = live + int(rng.integers(60, 800))
        n = max(n, GATE_ROWS + 300)
        if n % 16 == 0:
            n += int(rng.integers(1, 16))  # the last tile is partial
        p["n_rows"], p["live_target"] = int(n), int(live)
        # 8191 live rows fall on w = 1, 5, 9, 13 and leaves of 16 on w = 2, 8, 14: within 15 wide seeds no dimension meets either twice
        p["max_node_size"] = 16 if w % 6 == 2 else int((64, 256, 1024)[int(rng.integers(0, 3))])
        p["row_order"] = int((2, 3)[w // 3 % 2]) if w % 3 == 1 else 0
    p["metrics"] = [metric_spec(nm, power) for nm in names]
    third = names[2]
    p["num_trees"] = int(rng.integers(1, 5))
    p["id_base"] = int((0, 1 << 40, int(rng.integers(1, 1 << 50)))[int(rng.integers(0, 3))])
    p["row_kind"] = int(rng.integers(0, 3))
    if third in ("canberra", "hamming") and p["row_kind"] == 1:
        # integer-valued rows: columns of zeros on both sides are Canberra's 0 / 0; and Hamming counts the bits of the f32s' low bytes, which
        # are zero there: every pair ties at key 0 and no threshold admits fewer than all 33 M of them (seconds of join per call)
        p["row_kind"] = 0
    p["plant_integers"] = third != "canberra"
    p["plant_zero"] = third not in ("canberra", "bray_curtis")
    p["no_zero_elements"] = third == "canberra"  # (the generators draw an exact 0.0 now and then: two of them in one column are Canberra's 0 / 0)
    p["row_seed"] = zo.SEED_ROWS + seed
    p["index_seed"] = zo.SEED_INDEX + seed
    B = int(rng.integers(1, 25))
    if B % 16 == 0 and rng.random() < 0.7:
        B += 1
    p["B"] = B
    p["k"] = int((1, 10, 32, 100)[int(rng.integers(0, 4))])
    p["probe"] = int((1, 1, 3)[int(rng.integers(0, 3))])
    if p["max_node_size"] < 16:
        p["probe"] = 1  # (a probe above the typical leaf length makes the walk's backups cascade through most of a tree)
    p["slab_lines"] = 16  # (32 lines and 32 sampled rows a put the slowest seed over twice the slowest single-family case: cut, the shapes kept)
    p["slab_at"] = ("last", "removed", "random")[seed % 3]
    p["sample_a"] = 16
    p["filter_kinds"] = [("bool", "ids", "short", "block", "p95", "edge8192")[int(i)] for i in rng.integers(0, 6, 2)]
    if not narrow and w % 4 == 0:
        p["filter_kinds"][0] = "live"  # exactly 8192 live rows, all allowed, the removed rows' bits arbitrary: the gate's own edge
    if not narrow and w % 4 == 2:
        p["filter_kinds"][0] = "edge8192"
    big_b = not narrow and w % 5 == 3
    p["b_rows"] = int(rng.integers(4200, 4400)) if big_b else int(rng.integers(300, 1500))
    p["b_removed"] = int(rng.integers(1, 60))
    p["b_id_base"] = int((0, 1 << 41, int(rng.integers(1, 1 << 50)))[int(rng.integers(0, 3))])
    p["want_pairs"] = 3000
    p["round1"] = _calls(rng, 1, narrow)
    for c in p["round1"]:  # the cross join of round 1: live(A) x live(B) >= 2^25 with no override where B is large (the gate itself), else forced to path 2
        if c["family"] == "cross" and not narrow:
            c["override"] = None if big_b else 2
    p["mutation"] = MUTATIONS[(seed + seed // 5) % 5]
    p["mutation_rows"] = int(rng.integers(17, 300))
    p["round2"] = _calls(rng, 2, narrow)
    p["round2_metric"] = int(rng.integers(0, 3))
    p["data_seed"] = int(rng.integers(0, 1 << 31))
    return p


def _no_zero(p, A):
    if p["no_zero_elements"]:
        A[A == 0] = np.float32(2.0**-20)
    return A


def build_rows(p):
    """the seed's stored rows, planted: bit-identical duplicates, near-duplicates x (1 + 2^-12), rows scaled by 2^+-40, integer-valued rows, a
    zero row (positions below 600: every plan has at least that many rows)"""
    n, d = p["n_rows"], p["d"]
    X = zo.synth_rows(n, d, seed=p["row_seed"], kind=p["row_kind"]).copy()
    for i in range(NEAR):
        X[100 + i] = X[i] * np.float32(1.0 + 2.0**-12)
    X[200:210] = X[300:310]
    X[400:405] *= np.float32(2.0**40)
    X[410:415] *= np.float32(2.0**-40)
    if p["plant_integers"] and p["row_kind"] != 1:
        X[500:505] = np.round(X[500:505] * 100.0)
    _no_zero(p, X)
    if p["plant_zero"]:
        X[550] = 0.0
    return X


def more_rows(p, n, which):
    """rows for the mutation (`which` 1) and for the second index (`which` 2)"""
    return _no_zero(p, zo.synth_rows(n, p["d"], seed=p["row_seed"] + 7919 * which, row0=10**6, kind=p["row_kind"]).copy())


def build_queries(p, X):
    """B queries near stored rows; the first is a stored row itself, the second (where the metrics allow) the zero query"""
    Q = zo.synth_queries(p["B"], p["d"], X.shape[0], seed_rows=p["row_seed"], seed_q=zo.SEED_QUERIES + p["seed"], kind=p["row_kind"]).copy()
    _no_zero(p, Q)
    Q[0] = X[3]
    if p["B"] > 1 and p["plant_zero"]:
        Q[1] = 0.0
    return np.ascontiguousarray(Q, np.float32)


def removals(p, n_rows, live_target, rng):
    """the rows removed at the start: a whole 16-row tile, every third row of another, the last row, then random rows down to the live target"""
    gone = list(range(112, 128)) + list(range(80, 96, 3)) + [n_rows - 1]
    rest = np.setdiff1d(np.arange(n_rows), np.array(gone))
    extra = n_rows - live_target - len(gone)
    assert extra >= 0, (n_rows, live_target)
    gone += rng.choice(rest, extra, replace=False).tolist()
    return np.sort(np.array(gone, np.int64))


def slab_first_row(p, alive, rng):
    n, L = alive.size, p["slab_lines"]
    if p["slab_at"] == "last":
        return n - L
    if p["slab_at"] == "removed":
        return 104  # [104, 120): live near-duplicates and the first half of the removed tile 112 .. 127
    return int(rng.integers(0, n - L))


def make_filter(kind, alive, id_base, rng):
    """-> (the `allowed` argument of search_exact_filtered_batch, the mask over the stored rows it means)"""
    n = alive.size
    live = np.flatnonzero(alive)
    if kind == "bool":
        m = rng.random(n) < 0.97
        return m, m
    if kind == "ids":
        m = rng.random(n) < 0.97
        return (np.flatnonzero(m).astype(np.uint64) + np.uint64(id_base)), m
    if kind == "short":  # a mask shorter than the table: the rows past it are not allowed
        m = np.ones(n, bool)
        m[n - 40:] = False
        m[rng.integers(0, n - 40, 20)] = False
        return m[:n - 40].copy(), m
    if kind == "block":
        lo = int(rng.integers(0, 100))
        m = np.zeros(n, bool)
        m[lo:n - int(rng.integers(0, 100))] = True
        return m, m
    if kind == "p95":
        m = rng.random(n) < 0.95
        return m, m
    if kind == "live":  # every live row, and arbitrary bits for the removed ones
        m = alive | (rng.random(n) < 0.5)
        return m, m
    if kind == "edge8192":  # exactly 8192 allowed live rows where the table has them (else every live row)
        m = rng.random(n) < 0.5
        m[live] = False
        m[live[np.sort(rng.permutation(live.size)[:GATE_ROWS])]] = True
        return m, m
    raise ValueError(kind)


def initial_alive(p):
    alive = np.ones(p["n_rows"], bool)
    alive[removals(p, p["n_rows"], p["live_target"], np.random.default_rng([p["data_seed"], 0]))] = False
    return alive


def second_alive(p):
    alive = np.ones(p["b_rows"], bool)
    alive[np.random.default_rng([p["data_seed"], 9]).permutation(p["b_rows"])[:p["b_removed"]]] = False
    return alive


def round_setup(p, round_no, alive):
    """what a round draws once its live rows are known: the filter, the graph slab, the sampled rows a of the joins (planted rows among them)"""
    rng = np.random.default_rng([p["data_seed"], round_no])
    allowed_arg, allowed = make_filter(p["filter_kinds"][round_no - 1], alive, p["id_base"], rng)
    first = slab_first_row(p, alive, rng)
    live = np.flatnonzero(alive)
    sample = np.union1d(rng.choice(live, min(p["sample_a"] - 6, live.size), replace=False), np.array([0, 3, 100, 200, 300, 410]))
    sample = sample[alive[sample]]
    return {"allowed_arg": allowed_arg, "allowed": allowed, "first_row": first, "slab": np.arange(first, first + p["slab_lines"]),
            "sample": np.sort(sample), "rng": rng}


# ---------------------------------------------------------------------------------------------------------------- paths
def supported(d, spec):
    return d in MFMA_DIMS and spec["kinda"] is not None


def filter_tile_rule(allowed_live):
    """the filter's cost rule in id order: tiles with an allowed live row are loaded, the others skipped"""
    n = allowed_live.size
    all_tiles = (n + 15) // 16
    pad = np.zeros(all_tiles * 16, bool)
    pad[:n] = allowed_live
    tiles = int(pad.reshape(-1, 16).any(1).sum())
    return 16 * tiles + (all_tiles - tiles) <= FILTER_ROW_COST * float(allowed_live.sum())


def plan_override(p, family, spec, override, round_no=1):
    """the override a call really runs under: the plan's, except where a gate depends on what only the device knows -- there the path is forced
    (the forest range search's visitor count, always; the filter's tile-cost rule under a scan row order)"""
    if family == "frange" and override is None and supported(p["d"], spec) and p["max_node_size"] >= GATE_NODE:
        return 2 if round_no == 1 or (p["seed"] + spec["om"]) % 3 else 1
    if family == "filtered" and override is None and p["row_order"] and supported(p["d"], spec):
        return 2
    return override


def expected_path(family, d, spec, override=None, live=0, allowed=0, k=1, max_node_size=0, live_b=0, tile_rule=True):
    """the path a call must report (info["path"]), from the gates of include/zebra_hip.h"""
    if override == 1 or not supported(d, spec):
        return 1
    if family == "exact":
        return 2 if k > 0 and live >= max(k, GATE_ROWS) else 1
    if family == "filtered":
        if not (k > 0 and allowed >= max(k, GATE_ROWS)):
            return 1
        return 2 if override == 2 or tile_rule else 1
    if family in ("range", "join"):
        return 2 if live >= GATE_ROWS else 1
    if family == "cross":
        return 2 if override == 2 or live * live_b >= GATE_PAIRS else 1
    if family == "knn":
        return 2 if live >= max(k + 1, GATE_ROWS) else 1
    if family in ("fknn", "fjoin"):
        return 2 if max_node_size >= GATE_NODE else 1
    if family == "frange":
        assert override == 2 or max_node_size < GATE_NODE, "the visitor gate is the device's: the plan forces this call"
        return 2 if max_node_size >= GATE_NODE else 1
    raise ValueError(family)


def coverage(seeds):
    """what the plans of `seeds` promise, from the plans alone (first-round live counts; the second round adds, never takes away):
    -> (path2: {(family, d, kinda)}, path1: {family: calls}, edges: set, mutations: {name: count}, l2_seeds)"""
    path2, path1, edges, muts, l2 = set(), {f: 0 for f in FAMILIES}, set(), {m: 0 for m in MUTATIONS}, 0
    for s in seeds:
        p = plan(s)
        muts[p["mutation"]] += 1
        live = p["live_target"]
        l2 += any(m["name"] == "l2" for m in p["metrics"])
        if not p["narrow"]:
            if live == GATE_ROWS:
                edges.add("8192 live")
            if live == GATE_ROWS - 1:
                edges.add("8191 live")
            if p["max_node_size"] == 16:
                edges.add("max_node_size 16")
            if (live * (p["b_rows"] - p["b_removed"])) >= GATE_PAIRS and not any(c["family"] == "cross" and c["override"] for c in p["round1"]):
                edges.add("natural 2^25 cross join")
        alive = initial_alive(p)
        allowed_live = round_setup(p, 1, alive)["allowed"] & alive
        if not p["narrow"] and int(allowed_live.sum()) == GATE_ROWS:
            edges.add("8192 allowed")
        for spec in p["metrics"]:
            for c in p["round1"]:
                fam = c["family"]
                ov = plan_override(p, fam, spec, c["override"])
                path = expected_path(fam, p["d"], spec, ov, live=live, allowed=int(allowed_live.sum()), k=p["k"], max_node_size=p["max_node_size"],
                                     live_b=p["b_rows"] - p["b_removed"], tile_rule=filter_tile_rule(allowed_live))
                if path == 2:
                    path2.add((fam, p["d"], spec["kinda"]))
                else:
                    path1[fam] += 1
    return path2, path1, edges, muts, l2


# ---------------------------------------------------------------------------------------------------------------- keys
def key_is_nan(K, spec):
    K = np.asarray(K, np.uint64)
    if spec["om"] in (zo.COSINE, zo.L2SQ, zo.L2):
        return np.isnan(K.view(np.float64))
    if spec["om"] == zo.HAMMING:
        return np.zeros(K.shape, bool)
    return np.isnan(K.astype(np.uint32).view(np.float32))


_POOL = concurrent.futures.ThreadPoolExecutor(8)


def key_matrix(spec, X, Q):
    """K[i, r] = the oracle's key of stored row r against query i -> [len(Q), len(X)] u64; no key may be a NaN"""
    X, Q = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32)
    rows = list(_POOL.map(lambda q: zo.distance_batch(spec["om"], spec["omode"], X, q), Q))
    K = np.stack(rows).astype(np.uint64) if rows else np.zeros((0, X.shape[0]), np.uint64)
    assert not key_is_nan(K, spec).any(), "a reference key is a NaN (%s): the plan must not feed this" % spec["name"]
    return K


# ---------------------------------------------------------------------------------------------------------------- references
def topk_ref(K, mask, k, id_base):
    """per line i the first k rows of mask[i] (or of one mask for all) by (key, id) -> ids [n, k], keys [n, k] (2^64-1 past the count), counts"""
    nq, n = K.shape
    mask = np.broadcast_to(np.asarray(mask, bool), (nq, n))
    ids, keys, counts = np.full((nq, k), ALL, np.uint64), np.full((nq, k), ALL, np.uint64), np.zeros(nq, np.uint32)
    for i in range(nq):
        r = np.flatnonzero(mask[i])
        o = np.lexsort((r, K[i, r]))[:k]
        ids[i, :o.size], keys[i, :o.size], counts[i] = r[o].astype(np.uint64) + np.uint64(id_base), K[i, r[o]], o.size
    return ids, keys, counts


def range_ref(K, mask, thresholds, id_base):
    """per line i the rows of mask[i] with key <= thresholds[i], by (key, id) -> (offsets [n + 1], ids, keys)"""
    nq, n = K.shape
    mask = np.broadcast_to(np.asarray(mask, bool), (nq, n))
    thresholds = np.broadcast_to(np.asarray(thresholds, np.uint64), (nq,))
    ids, keys, off = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], [0]
    for i in range(nq):
        r = np.flatnonzero(mask[i] & (K[i] <= thresholds[i]))
        o = np.lexsort((r, K[i, r]))
        ids.append(r[o].astype(np.uint64) + np.uint64(id_base))
        keys.append(K[i, r[o]])
        off.append(off[-1] + o.size)
    return np.array(off, np.uint64), np.concatenate(ids), np.concatenate(keys)


def graph_ref(K, rows, alive, k, id_base, mates=None):
    """the graph lines of the stored rows `rows` (K[i] = the keys against row rows[i]): the first k of every live row but the line's own (or of
    its leaf-mates `mates[i]`, a membership the forest already cleared of removed rows); a removed row's line is empty"""
    rows = np.asarray(rows, np.int64)
    mask = np.broadcast_to(alive, K.shape).copy() if mates is None else np.asarray(mates, bool).copy()
    mask[np.arange(rows.size), rows] = False
    mask[~alive[rows]] = False
    return topk_ref(K, mask, k, id_base)


def join_ref(K, a_rows, a_alive, mask_b, threshold, id_base_a, id_base_b, upper):
    """the join's pairs that start at the rows `a_rows` (ascending; K[i] = the keys against row a_rows[i]): b in mask_b[i] (or one mask for
    all), key <= threshold, b > a for the self forms (`upper`) -> (a, b, keys) ascending by (a, key, b)"""
    a_rows = np.asarray(a_rows, np.int64)
    nq, n = K.shape
    mask = np.broadcast_to(np.asarray(mask_b, bool), (nq, n)).copy()
    mask[~a_alive[a_rows]] = False
    if upper:
        mask &= np.arange(n)[None, :] > a_rows[:, None]
    off, b, keys = range_ref(K, mask, np.uint64(threshold), id_base_b)
    a = np.repeat(a_rows.astype(np.uint64) + np.uint64(id_base_a), np.diff(off).astype(np.int64))
    return a, b, keys


def restrict(got, a_rows, id_base):
    m = np.isin(got[0], np.asarray(a_rows, np.uint64) + np.uint64(id_base))
    return got[0][m], got[1][m], got[2][m]


def quantile_threshold(K, mask, want_pairs, all_pairs):
    """exactly an existing pair's key: the masked keys are a share of all pairs, so their (want_pairs * share)-th smallest admits about want_pairs"""
    ks = K[np.broadcast_to(mask, K.shape)]
    if ks.size == 0:
        return np.uint64(0)
    kth = min(ks.size, max(1, int(round(want_pairs * ks.size / max(all_pairs, 1)))))
    key = np.partition(ks, kth - 1)[kth - 1]
    below = ks[ks < key]
    if int((ks <= key).sum()) > 4 * kth:  # a run of tied keys (Hamming's small integers, a power of 0) would admit many times the pairs asked for:
        key = below.max() if below.size else key - np.uint64(1) if key > 0 else key  # the key below the run, or one below a run that is everything
    return key


def range_thresholds(K, mask, spec, rng):
    """one threshold per query from the menu: an existing key at a random rank (smallest, tens, about 1000, largest), such a key +-1, 0, 2^64-1,
    and a key with the sign bit set (for the parity cosine key: a negative similarity)"""
    nq = K.shape[0]
    mask = np.broadcast_to(np.asarray(mask, bool), K.shape)
    out = np.zeros(nq, np.uint64)
    for i in range(nq):
        ks = np.sort(K[i, mask[i]])
        pick = int(rng.integers(0, 9)) if i >= 9 else i  # the first nine queries walk the menu, the rest draw from it
        if ks.size == 0 or pick == 4:
            out[i] = 0
        elif pick == 5:
            out[i] = ALL
        elif pick == 6:
            neg = ks[ks >= np.uint64(1 << 63)]
            out[i] = neg[neg.size // 2] if is_parity(spec) and neg.size else np.float64(-0.5).view(np.uint64) if spec["kinda"] is not None \
                else np.uint64(0x80000000 | 0x3F000000)
        else:
            rank = (0, int(rng.integers(10, 60)), min(ks.size - 1, 1000), ks.size - 1)[pick % 4]
            key = int(ks[min(rank, ks.size - 1)])
            if pick in (7, 8):
                key = max(0, min(2**64 - 1, key + (1 if pick == 7 else -1)))
            out[i] = key
    return out


# ---------------------------------------------------------------------------------------------------------------- the forest
def leaf_table(forest, n_rows):
    """leaf_of[t, r] = the leaf node that holds stored row r in tree t, -1 where tree t does not hold it"""
    plane, left, right = (np.asarray(forest[k]).astype(np.int64) for k in ("plane", "left", "right"))
    leaf_ids = np.asarray(forest["leaf_ids"]).astype(np.int64)
    roots = np.asarray(forest["roots"]).astype(np.int64)
    leaf_of = np.full((roots.size, n_rows), -1, np.int64)
    for t, root in enumerate(roots.tolist()):
        stack = [root]
        while stack:
            node = stack.pop()
            if plane[node] < 0:
                members = leaf_ids[left[node]:left[node] + right[node]]
                assert (leaf_of[t, members] == -1).all(), "a row twice in one tree"
                leaf_of[t, members] = node
            else:
                stack += [int(left[node]), int(right[node])]
    return leaf_of


def mates_mask(leaf_of, rows):
    """[len(rows), n]: stored row r shares a leaf with rows[i] in some tree (rows[i] itself included where a tree holds it)"""
    rows = np.asarray(rows, np.int64)
    own = leaf_of[:, rows]  # [T, lines]
    return ((leaf_of[:, None, :] == own[:, :, None]) & (own[:, :, None] >= 0)).any(0)


def are_mates(leaf_of, a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return ((leaf_of[:, a] == leaf_of[:, b]) & (leaf_of[:, a] >= 0)).any(0)


def visited_mask(X, max_node_size, forest, Q, probe, cap_visits=1 << 14):
    """[len(Q), n]: stored row r is a member of a leaf the oracle's walk (tree_result, n = probe) visits for query i on this forest"""
    f = zo.Forest.from_arrays(X, max_node_size, forest)
    leaf_ids = np.asarray(forest["leaf_ids"]).astype(np.int64)
    out = np.zeros((len(Q), X.shape[0]), bool)
    for i, q in enumerate(Q):
        for t in range(int(np.asarray(forest["roots"]).size)):
            _, _, v = f.tree_result(t, q, probe, zo.L2SQ, 0, cap_visits=cap_visits)  # (the visit sequence never depends on the metric)
            assert v.shape[0] < cap_visits
            for off, length, _ in v.tolist():
                out[i, leaf_ids[int(off):int(off) + int(length)]] = True
    return out


def compact_map(alive, id_base):
    """the id map compact() must return: id_base + new row of every old row, 2^64-1 for a removed one"""
    out = np.full(alive.size, GONE, np.uint64)
    out[alive] = np.arange(int(alive.sum()), dtype=np.uint64) + np.uint64(id_base)
    return out

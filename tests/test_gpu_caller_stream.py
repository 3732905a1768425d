"""Every `_device` entry point on a CALLER'S stream that still has work pending when the library is entered (tests/stream_cases.py has the case
and its references; tests/test_stream_cases.py pins them on the CPU).

include/zebra_hip.h promises for the nine exact and forest families and for the LSH search that the work is "enqueued on `stream`" and "complete
on return", and for zh_merge_topk[_packed]_device and zh_synth_queries_device that it is "enqueued on `stream` and the call returns".  Every stream
in play is non-blocking, so a launch on another stream than the caller's is ordered against nothing.  The protocol (run() below) makes that visible:

  1  the buffers the call reads hold a different, VALID input (the queries rolled by one, thresholds of 0, a filter with no bit set); the real
     inputs wait in staging tensors; every output (offsets, totals and counts included) holds sentinel A; torch.cuda.synchronize()
  2  on the side stream S: a delay (torch.cuda._sleep, calibrated by event timing in this run), device-to-device copies of the real inputs into
     the buffers, fills of every output with sentinel B; S.query() must be false
  3  the call, with stream = S; nothing synchronises in between
  4  S.query() must be true at once; the outputs are read through a THIRD stream with its own sync (no device sync, no sync of S) and must
     equal the oracle's reference bit for bit and, in full, the host entry point's answer on a twin index; the family's info must report the
     expected path with redone == 0.  (The asynchronous three are read after S.synchronize() alone.)

A launch on the wrong stream reads the stale input or scratch that does not exist yet, has its result overwritten by sentinel B, or is read before
it has run.  test_the_protocol_sees_a_misordered_read is the control: the same staging and delay, a torch copy on another stream as the consumer,
and the assertion that it DOES see the stale input.

WHICH STREAM IS S.  A process's streams share the device's few hardware queues (four by HIP's default), and two streams on one queue run in order whatever
the program says: a launch that slipped onto the index's own stream would then wait behind S's delay after all and the protocol could not see it.
Rig.pick_streams() therefore takes for S the first of eight candidates behind which neither index's OWN stream is held back, found with the protocol
itself (the exact search on the large index and the cross join on the left one, made with stream = NULL while fills are pending on the candidate,
must be overwritten by them), and for the control's consumer a stream a torch fill shows to be free of S; the control asserts both were found.
(The first candidate of the measured run shared a queue with the left index's stream: the cross join made on that stream answered correctly.)
NOT PROBED: the indexes' sweep streams and the search contexts' streams, and the streams made after S was chosen -- the fresh indexes of
test_first_use and the context of test_lsh_search_context.  Any of them may share S's queue, and a launch that slipped onto it would then be hidden.
test_first_use repeats its call with stream = NULL under pending fills afterwards and records (does not assert) whether the fresh index's own
stream was free of S; the closing test prints the nine answers.  In the measured run only the cross join's fresh left index was: the other eight
fresh indexes' streams shared S's queue (each is made after the last one was destroyed and gets its place), so for them test_first_use shows
that a first use on the caller's stream answers correctly and completes, not that no launch of it strayed.

The delay of every call is measured by an event pair on S and asserted to be at least 20 ms, at most 100 ms, and at least twice the slowest
wall time of the calls that were timed with stream = NULL on an idle device in this run, on the twin: the 26 steady-state calls (after the twin's
host call), the five capacity-short calls and the LSH search's device call.  NOT held to it: the first-use calls (timed on a fresh index for the
record, printed by the closing test; they do more work -- the live views, the fp16 copy -- and drain the device before their scan anyway), the
context round and the asynchronous three (a merge of 7 x 13 x 100 entries, 24 generated queries).

WHAT EACH CALL IS SENSITIVE TO (from reading zebra_amd/csrc/zh_api.hip, and from one run of every path-2 call made ENTIRELY on the index's own
stream under this protocol: all but the forest self-join then answered wrongly).  No call path issues work on another stream than
s = call_stream(ix, stream); the helpers that make index state on ix->stream (exact_live_rows: blocking copies; ensure_row_half, build_scan_perm,
build_row_leaf) wait for it on the host before they return, so nothing they make is read unordered: no library fix was needed.  The protocol is
deterministic for everything a call enqueues BEFORE ITS FIRST HOST WAIT ON s -- that work sits behind the delay, and one launch on another stream
breaks the chain of scratch buffers or meets the stale input / the pending fill.  After that wait S is idle: a wrong-stream launch later in the
call can only show as a result read before it exists (a race the third-stream read usually wins, not always).  Per family, steady state:
  exact      path 2 and path 1: the whole call is enqueued before the one wait (lists_end / the final sync): fully sensitive
  filtered   filter_prepare waits after its first kernel (zh_launch_filter_and, which reads the filter): the filter read is covered, the scan is not
  range      both paths: thresholds, scan and survivor pass before the first wait (range_batch2 / range_one); offsets, sort and total after it
  frange     frange_setup waits after the node map and the row -> leaf table (before any query is read); the walk, the scan and the emit follow
  join       path 2 waits after the threshold upload and join_prep (max_key is the caller's stack); path 1: every panel before the one wait: fully
  cross      as join; path 2 waits after the two join_prep launches
  knn        path 2: knn_setup waits after join_prep and the list bases; path 1: the empty fill, every panel and the emit before the final sync: fully
  fknn       fknn_setup waits after the node map upload; each sub-slab waits for its line count
  fjoin      fjoin_setup waits after the node map and the row -> leaf table
  LSH        search_batch_device and begin / finish enqueue the hash and the walk's counting pass before finish's host wait for the three totals
Calls that DRAIN THE WHOLE DEVICE (hipFree, hipDeviceSynchronize) are blind from the drain on, whatever stream they launch on:
  on return  every family call gives its scratch back (ScratchGuard -> DevBuf::release -> hipFree) after its final wait and before it returns, so
             S.query() is true on return whatever was enqueued where; the assertion is kept because the contract says so, and it is a real
             test for the LSH search, whose contexts keep their scratch.  "Returned too early" shows as a wrong answer, not as a busy stream.
  first use  every path-2 call: ensure_row_half makes the fp16 copy and calls quiesce_before_rewrite (hipDeviceSynchronize) before the first scan
             kernel; the filtered search's zh_launch_filter_and is the one launch that comes before it.  A never-queried index has no row -> leaf
             table of the LSH scan (build_row_leaf), so build_scan_perm returns at once: no row order is made from these nine families.
             The module also sets ZH_ROW_ORDER=0 for every call (the filter's tile rule is counted in id order), which alone keeps
             build_scan_perm and ensure_row_leaf_p from running; and the LSH search is warmed with stream = NULL, so ITS first use
             (build_row_leaf, the row order, the fp16 copy of its scan) is never entered on S.  None of those helpers is tested here.
  steady     no path drains before its first launches: per-call scratch starts released, so DevBuf::ensure is a bare hipMalloc.  But a scratch
             buffer that GROWS inside a call (ensure with a larger size: hipFree of the old one) drains mid-call.  The forest self-join's path 2
             does by the reading of the code, between its batches of leaves (fjoin_batch2: fj_segs, fk_colsrc, fk_crow, fk_CA, fk_cmeta, fk_cqm,
             fj_cand, sized per batch):
             made entirely on the index's own stream it still answered correctly, so for it the protocol covers fjoin_setup's launches only.
             The forest graph's path 2 (fknn_batch2, sized per batch) drains part of the way through and was still caught.

Measured on an MI355X (one run, pytest --durations): the delay 45.1 ms on every one of the 46 calls (asked for: 45.2 ms = 2.5 times the slowest
idle call), the slowest idle call 18.1 ms (the self-join under Manhattan, path 1; the next: the forest graph on path 2, 5.8 ms; the capacity-short
calls 0.2 .. 1.2 ms, the LSH search 0.2 ms), a first use on an idle device 0.6 .. 6.1 ms, the module 6.7 s for 46 tests of which the fixture's
setup is 1.4 s (plus 3 s for the case on the CPU), the slowest test 0.11 s."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import zebra_oracle as zo  # noqa: E402  (the checker; tests may use it)
from tests import family_cases as fc  # noqa: E402
from tests import merge_cases as mc  # noqa: E402
from tests import stream_cases as sc  # noqa: E402
from tests.test_gpu_fuzz_families import INFO, same, za_metric  # noqa: E402

SENT_A, SENT_B = 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C  # (positive as int64; their low words as int32)
ELIMIT = -5
MIN_DELAY_MS, MAX_DELAY_MS = 20.0, 100.0
SWITCHES = tuple(e for e, _ in fc.PATH_ENV.values() if e) + ("ZH_KNN_LIST_CAP", "ZH_FKNN_LIST_CAP", "ZH_FJOIN_CAND_CAP", "ZH_FRANGE_CAND_CAP",
                                                            "ZH_WALK_LOG_CHUNKS", "ZH_ROW_HALF_META_ONLY")
_measured = {"delay_ms": [], "wall_ms": {}, "first_use_ms": {}, "fresh_free": {}}


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def sentinel(t, value):
    return value & 0xFFFFFFFF if t.element_size() == 4 else value


def set_path(mp, family, mode):
    for e in SWITCHES:
        mp.delenv(e, raising=False)
    mp.setenv("ZH_ROW_ORDER", "0")  # (id order: the filter's tile rule is counted in it, fc.plan_override)
    env, ov = fc.PATH_ENV[family][0], sc.mode_override(family, mode)
    if env and ov is not None:
        mp.setenv(env, str(ov))


class Rig:
    """the streams, the calibrated delay, the device copies of the case's inputs, the indexes and their twins"""

    def __init__(self, za, torch):
        self.za, self.torch, self.case = za, torch, sc.case()
        c, p = self.case, self.case.p
        self.dev = torch.device("cuda", 0)
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(8)]  # (non-blocking, as every stream torch makes)
        self.S, self.other, self.R = self.streams[:3]  # pick_streams() chooses among them once the indexes are warm
        self.slowest_ms = 0.0
        self.cycles = 0
        self.ix, self.ixl = self.make(False), self.make(True)
        self.tw, self.twl = self.make(False), self.make(True)
        up = lambda a: torch.from_numpy(np.array(a)).to(self.dev)  # noqa: E731  (a copy: the case's arrays are read-only)
        self.q_real, self.q_stale = up(c.Q), up(np.roll(c.Q, 1, axis=0))
        words, self.n_bits = self.ix.filter_bitmap(c.allowed_arg)
        self.f_real, self.f_stale = up(words.view(np.int32)), up(np.zeros(words.size, np.int32))
        self.thr = {(name, fam): up(getattr(c.refs[name], fam + "_thr").view(np.int64)) for name in sc.METRICS for fam in ("range", "frange")}
        self.thr_stale = up(np.zeros(p["B"], np.int64))
        self.host = {}  # (family, mode) -> the host entry point's answer on the twin

    def make(self, left):
        za, c, p = self.za, self.case, self.case.p
        if left:
            ix = za.LSHIndex(p["d"], za.LSHIndexOptions(64, 1), device=0, id_base=c.baseL)
            ix.append(c.XL)
            assert ix.remove(c.goneL + np.uint64(c.baseL)).size == c.goneL.size
            return ix
        ix = za.LSHIndex(p["d"], za.LSHIndexOptions(p["max_node_size"], p["num_trees"]), seed=p["index_seed"], device=0, id_base=c.base)
        ix.append(c.X)
        assert ix.remove(c.gone + np.uint64(c.base)).size == c.gone.size
        ix.set_forest(c.forest)  # the case's forest: the oracle's, the removed rows taken out of it
        got = ix.get_forest()  # (set_forest renumbers the planes level by level; the nodes, the leaves and their rows stay as given)
        for name in ("left", "right", "roots", "leaf_ids"):
            assert (np.asarray(got[name]).astype(np.int64) == np.asarray(c.forest[name]).astype(np.int64)).all(), name
        assert ((got["plane"] < 0) == (c.forest["plane"] < 0)).all()
        return ix

    def calibrate(self):
        """cycles of torch.cuda._sleep for the module's delay: 2.5 times the slowest idle call, within [1.5 * 20 ms, 100 ms / 1.25]"""
        torch, S = self.torch, self.S
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        per_ms = None
        for cycles in (2_000_000, 20_000_000):
            with torch.cuda.stream(S):
                e[0].record(S)
                torch.cuda._sleep(cycles)
                e[1].record(S)
            S.synchronize()
            per_ms = cycles / max(e[0].elapsed_time(e[1]), 1e-3)
        target = min(max(2.5 * self.slowest_ms, 1.5 * MIN_DELAY_MS), MAX_DELAY_MS / 1.25)
        self.cycles = int(per_ms * target)
        self.target_ms = target

    def fill_came_last(self, stream, outputs, consumer):
        """step 2 of the protocol on `stream` (the delay, then fills of `outputs` with sentinel B), consumer() at once, everything drained -> True when
        the outputs hold sentinel B: what the consumer wrote was NOT held back behind the delay"""
        torch = self.torch
        for o in outputs:
            o.fill_(sentinel(o, SENT_A))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(self.cycles)
            for o in outputs:
                o.fill_(sentinel(o, SENT_B))
        consumer()
        torch.cuda.synchronize()
        return all(bool((o == sentinel(o, SENT_B)).all()) for o in outputs)

    def pick_streams(self):
        """The streams of a process share the device's few hardware queues, and two streams on one queue are ordered against each other whatever the
        program says: a launch that slipped onto the index's own stream would then run behind the side stream's delay after all, and the protocol
        could not see it.  So S is a stream behind which work on either index's OWN stream is not held back -- found with the protocol itself:
        the call made with stream = NULL while the fills are pending on the candidate must be overwritten by them -- and the control's consumer
        stream is one that a torch fill shows to be free of S in the same way.  -> what was found, per candidate"""
        torch = self.torch
        ex = Call(self, "exact", sc.METRICS[0], self.ix, self.ixl)
        xj = Call(self, "cross", sc.METRICS[0], self.ix, self.ixl, total=self.host[("cross", "path2")][0].size)
        for buf, real, _ in ex.inputs:
            buf.copy_(real)
        found = []
        for st in self.streams:
            found.append((self.fill_came_last(st, ex.out, lambda: ex.invoke(None)), self.fill_came_last(st, xj.out, lambda: xj.invoke(None))))
            if all(found[-1]):
                break
        good = [i for i, f in enumerate(found) if all(f)]
        self.S_is_free_of_the_indexes = bool(good)
        self.S = self.streams[good[0] if good else 0]
        rest = [st for st in self.streams if st is not self.S]
        probe = [torch.empty(64, dtype=torch.int32, device=self.dev)]

        def torch_fill(st):
            with torch.cuda.stream(st):
                probe[0].fill_(7)

        free = [st for st in rest[:4] if self.fill_came_last(self.S, probe, lambda st=st: torch_fill(st))]
        self.other_is_free_of_S = bool(free)
        self.other = free[0] if free else rest[0]
        self.R = [st for st in rest if st is not self.other][0]
        self.found = found
        return found

    def close(self):
        for ix in (self.ixl, self.twl, self.ix, self.tw):
            ix.close()


class Call:
    """one call of a family on device pointers: its input buffers (with the real and the stale value of each), its outputs, how to invoke it, what
    it must answer"""

    def __init__(self, rig, family, metric_name, ix, ixl, short=False, total=None):
        torch, c, p = rig.torch, rig.case, rig.case.p
        r = c.refs[metric_name]
        self.family, self.rig, self.ix, self.ixl, self.r, self.short = family, rig, ix, ixl, r, short
        self.m = za_metric(rig.za, r.spec)
        B, k = p["B"], p["k"]
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=rig.dev)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=rig.dev)  # noqa: E731
        self.inputs, self.names = [], None
        if family in ("exact", "filtered", "range", "frange"):
            self.q = torch.empty_like(rig.q_real)
            self.inputs.append((self.q, rig.q_real, rig.q_stale))
        if family == "filtered":
            self.f = torch.empty_like(rig.f_real)
            self.inputs.append((self.f, rig.f_real, rig.f_stale))
        if family in ("range", "frange"):
            self.t = torch.empty_like(rig.thr_stale)
            self.inputs.append((self.t, rig.thr[(metric_name, family)], rig.thr_stale))
        if family in ("exact", "filtered"):
            self.out, self.names = [i64(B, k), i64(B, k), i32(B)], ("ids", "keys", "counts")
        elif family in ("knn", "fknn"):
            self.out, self.names = [i64(c.slab.size, k), i64(c.slab.size, k), i32(c.slab.size)], ("ids", "keys", "counts")
        else:
            self.total = int(total)  # everything the call has to return (the joins: the twin's host answer says how much)
            self.cap = self.total - 1 if short else self.total  # one slot short: the edge of the limit test
            # the CPU-pinned case: the totals of range, frange and cross themselves; for the two joins the sampled rows' pairs, a lower bound
            assert 1 <= r.short_cap[family] <= self.cap and (family in ("join", "fjoin") or r.least_total[family] == self.total)
            if family in ("range", "frange"):
                self.out, self.names = [i64(B + 1), i64(self.cap), i64(self.cap), i64(1)], ("offsets", "ids", "keys", "total")
            else:
                self.out, self.names = [i64(self.cap), i64(self.cap), i64(self.cap), i64(1)], ("a", "b", "keys", "total")

    def invoke(self, stream):
        ix, m, p, c, o = self.ix, self.m, self.rig.case.p, self.rig.case, [t.data_ptr() for t in self.out]
        fam = self.family
        if fam == "exact":
            ix.search_exact_batch_device(self.q.data_ptr(), p["B"], p["k"], m, o[0], o[1], o[2], stream)
        elif fam == "filtered":
            ix.search_exact_filtered_batch_device(self.q.data_ptr(), p["B"], p["k"], m, self.f.data_ptr(), self.rig.n_bits, o[0], o[1], o[2], stream)
        elif fam == "range":
            ix.search_range_batch_device(self.q.data_ptr(), p["B"], self.t.data_ptr(), m, self.cap, o[0], o[1], o[2], o[3], stream)
        elif fam == "frange":
            ix.search_range_forest_batch_device(self.q.data_ptr(), p["B"], self.t.data_ptr(), p["probe"], m, self.cap, o[0], o[1], o[2], o[3], stream)
        elif fam == "join":
            ix.self_join_device(self.r.join_key, m, self.cap, o[0], o[1], o[2], o[3], stream)
        elif fam == "fjoin":
            ix.self_join_forest_device(self.r.join_key, m, self.cap, o[0], o[1], o[2], o[3], stream)
        elif fam == "cross":
            self.ixl.cross_join_device(ix, self.r.cross_key, m, self.cap, o[0], o[1], o[2], o[3], stream)
        elif fam == "knn":
            ix.knn_graph_device(p["k"], m, c.first_row, c.slab.size, o[0], o[1], o[2], stream)
        elif fam == "fknn":
            ix.knn_graph_forest_device(p["k"], m, c.first_row, c.slab.size, o[0], o[1], o[2], stream)
        else:
            raise ValueError(fam)

    def info(self):
        return getattr(self.ixl if self.family == "cross" else self.ix, INFO[self.family])()

    def answer(self, got):
        """the outputs as the reference's arrays: unsigned, ids / keys cut to the total"""
        if self.names[-1] == "counts":
            return u64(got[0]), u64(got[1]), got[2].view(np.uint32)
        n = min(self.total, self.cap)
        return u64(got[0]) if self.names[0] == "offsets" else u64(got[0])[:n], u64(got[1])[:n], u64(got[2])[:n], u64(got[3])


def host_answer(rig, family, metric_name):
    """the HOST entry point's answer on the twin (the existing suites pin it against the oracle at these shapes)"""
    c, p, r, tw = rig.case, rig.case.p, rig.case.refs[metric_name], rig.tw
    m = za_metric(rig.za, r.spec)
    if family == "exact":
        return tw.search_exact_batch(c.Q, p["k"], m)
    if family == "filtered":
        return tw.search_exact_filtered_batch(c.Q, p["k"], m, c.allowed_arg)
    if family == "range":
        return tw.search_range_batch(c.Q, metric=m, max_keys=r.range_thr, capacity=int(r.range[0][-1]))
    if family == "frange":
        return tw.search_range_forest_batch(c.Q, metric=m, max_keys=r.frange_thr, probe=p["probe"], capacity=int(r.frange[0][-1]))
    if family == "join":
        return tw.self_join(metric=m, max_key=r.join_key)
    if family == "fjoin":
        return tw.self_join_forest(metric=m, max_key=r.join_key)
    if family == "cross":
        return rig.twl.cross_join(tw, metric=m, max_key=r.cross_key)
    if family == "knn":
        return tw.knn_graph(p["k"], m, c.first_row, c.slab.size)
    if family == "fknn":
        return tw.knn_graph_forest(p["k"], m, c.first_row, c.slab.size)
    raise ValueError(family)


def total_of(family, host):
    if family in ("range", "frange"):
        return int(host[0][-1])
    return host[0].size if family in ("join", "fjoin", "cross") else None


def idle_call(rig, call):
    """the call with stream = NULL on an idle device, its real inputs in place -> wall milliseconds"""
    torch = rig.torch
    for buf, real, _ in call.inputs:
        buf.copy_(real)
    for o in call.out:
        o.fill_(sentinel(o, SENT_A))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        call.invoke(None)
    except rig.za.ZhError as e:
        assert call.short and e.code == ELIMIT, e
    return (time.perf_counter() - t0) * 1e3


def run(rig, inputs, outputs, invoke, asynchronous=False):
    """THE PROTOCOL (module docstring) -> (the outputs as numpy arrays, read through the third stream; the error code or None; the delay in ms)"""
    torch, S, R = rig.torch, rig.S, rig.R
    # 1: stale inputs, sentinel A, pinned landing buffers; everything in place before any side stream runs
    for buf, _, stale in inputs:
        buf.copy_(stale)
    for o in outputs:
        o.fill_(sentinel(o, SENT_A))
    landing = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outputs]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    # 2: behind a delay on S, the real inputs arrive and every output is filled with sentinel B
    with torch.cuda.stream(S):
        e0.record(S)
        torch.cuda._sleep(rig.cycles)
        e1.record(S)
        for buf, real, _ in inputs:
            buf.copy_(real, non_blocking=True)
        for o in outputs:
            o.fill_(sentinel(o, SENT_B))
    assert not S.query(), "the side stream was idle before the library was entered: the delay is too short to test anything"
    # 3: the call
    code = None
    try:
        invoke(S.cuda_stream)
    except rig.za.ZhError as e:
        code = e.code
    # 4: complete on return
    idle = S.query()
    if asynchronous:
        S.synchronize()
    else:
        assert idle, "the call returned with work still pending on the caller's stream"
    with torch.cuda.stream(R):
        for h, o in zip(landing, outputs):
            h.copy_(o, non_blocking=True)
    R.synchronize()
    got = [h.numpy().copy() for h in landing]
    S.synchronize()  # (for the event pair only: the outputs have been read)
    delay = e0.elapsed_time(e1)
    _measured["delay_ms"].append(delay)
    assert delay >= MIN_DELAY_MS and delay >= 2.0 * rig.slowest_ms, ("the delay is too short for the protocol", delay, rig.slowest_ms)
    assert delay <= MAX_DELAY_MS, ("the delay is above its cap", delay)
    return got, code, delay


@pytest.fixture(scope="module")
def rig():
    """the indexes and twins, built once; per steady-state call: the twin's host answer, the twin's device call on stream = NULL (timed: the idle wall
    time) and the index's own first call of the family on stream = NULL (code objects loaded, the fp16 copy and the live views made)"""
    import torch
    import zebra_amd as za
    mp = pytest.MonkeyPatch()
    set_path(mp, "exact", "path2")
    rig = None
    try:
        rig = Rig(za, torch)
        for family, mode in sc.steady_calls():
            set_path(mp, family, mode)
            name = sc.mode_metric(mode)
            host = rig.host[(family, mode)] = host_answer(rig, family, name)
            idle_call(rig, Call(rig, family, name, rig.tw, rig.twl, total=total_of(family, host)))  # (the twin's first device call)
            ms = idle_call(rig, Call(rig, family, name, rig.tw, rig.twl, total=total_of(family, host)))
            _measured["wall_ms"][(family, mode)] = ms
            rig.slowest_ms = max(rig.slowest_ms, ms)
            idle_call(rig, Call(rig, family, name, rig.ix, rig.ixl, total=total_of(family, host)))
        for family in sc.SHORT:  # the capacity-short calls' idle time, on the twin
            set_path(mp, family, "path2")
            host = rig.host[(family, "path2")]
            ms = _measured["wall_ms"][(family, "short")] = idle_call(rig, Call(rig, family, sc.METRICS[0], rig.tw, rig.twl, short=True, total=total_of(family, host)))
            rig.slowest_ms = max(rig.slowest_ms, ms)
        set_path(mp, "exact", "path2")
        m = za.L2SquaredDistance()  # the LSH search: once on either index through the host call, then the twin's device call, timed
        for ix in (rig.tw, rig.ix):
            ix.search_batch(rig.case.Q, rig.case.p["k"], m)
        q, out = lsh_buffers(rig)
        q.copy_(rig.q_real)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rig.tw.search_batch_device(q.data_ptr(), rig.case.p["B"], rig.case.p["k"], m, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None)
            ms = _measured["wall_ms"][("lsh", "device")] = (time.perf_counter() - t0) * 1e3
        rig.slowest_ms = max(rig.slowest_ms, ms)
        # for the record only (the delay is not held to it: a first-use path-2 call drains the device before its scan): a first use on an idle device
        for family in fc.FAMILIES:
            set_path(mp, family, "path2")
            ix, ixl = rig.make(False), rig.make(True) if family == "cross" else None
            try:
                _measured["first_use_ms"][family] = idle_call(rig, Call(rig, family, sc.METRICS[0], ix, ixl, total=total_of(family, rig.host[(family, "path2")])))
            finally:
                if ixl is not None:
                    ixl.close()
                ix.close()
        set_path(mp, "exact", "path2")
        rig.calibrate()
        print("caller's stream: candidates (exact on the index's own stream, cross join on the left index's) free of the side stream:", rig.pick_streams(),
              "S free:", rig.S_is_free_of_the_indexes, "control stream free:", rig.other_is_free_of_S)
        yield rig
    finally:
        mp.undo()
        if rig is not None:
            rig.close()


def check_call(rig, call, mode, host, record_property, want_path=2, first_use=False):
    c = rig.case
    ctx = lambda what="": "%s %s" % (what, {"family": call.family, "mode": mode, "short": call.short, "first use": first_use, "info": call.info()})  # noqa: E731
    got, code, delay = run(rig, call.inputs, call.out, call.invoke)
    record_property("delay_ms", round(delay, 2))
    record_property("slowest_idle_call_ms", round(rig.slowest_ms, 3))
    ans = call.answer(got)
    ref = getattr(call.r, call.family)
    fam = call.family
    if call.short:  # the capacity contract: ZH_ELIMIT, the total exact, and for the two range searches every offset
        assert code == ELIMIT, ctx("expected ZH_ELIMIT, got %s" % code)
        assert int(ans[3][0]) == call.total, ctx("out_total %d, want %d" % (int(ans[3][0]), call.total))
        if fam in ("range", "frange"):
            same(ans[:1], ref[:1], ("offsets",), ctx)
            same(ans[:1], host[:1], ("offsets (host entry point)",), ctx)
    else:
        assert code is None, ctx("error %s" % code)
        if fam in ("join", "fjoin"):  # the oracle on the sampled rows a; the host entry point's answer in full
            same(fc.restrict(ans[:3], c.sample, c.base), ref, ("a", "b", "keys"), ctx)
        else:
            same(ans[:len(ref)], ref, call.names, ctx)
        same(ans[:len(host)], host, tuple(n + " (host entry point)" for n in call.names), ctx)
        if len(ans) == 4:
            assert int(ans[3][0]) == call.total, ctx("out_total %d, want %d" % (int(ans[3][0]), call.total))
    info = call.info()
    assert info["path"] == want_path and info["redone"] == 0, ctx("expected path %d, redone 0" % want_path)


# ---------------------------------------------------------------------------------------------------------------- the control
def test_the_protocol_sees_a_misordered_read(rig, record_property):
    """no library code: the consumer is a torch copy of the input buffer on ANOTHER non-blocking stream, and it must see the stale input"""
    torch = rig.torch
    buf, seen = torch.empty_like(rig.q_real), torch.empty_like(rig.q_real)

    def consumer(_stream):
        with torch.cuda.stream(rig.other):
            seen.copy_(buf, non_blocking=True)
        rig.other.synchronize()
        assert not rig.S.query(), "the delay ended before a single copy on another stream did"
        rig.S.synchronize()  # (run() asserts what a library call owes: an idle stream on return)

    _, _, delay = run(rig, [(buf, rig.q_real, rig.q_stale)], [], consumer)
    record_property("delay_ms", round(delay, 2))
    torch.cuda.synchronize()
    real, stale = rig.q_real.cpu().numpy(), rig.q_stale.cpu().numpy()
    assert (real != stale).any(1).all()
    assert (seen.cpu().numpy() == stale).all(), "a copy on another stream did not see the stale input: the protocol is blind on this machine"
    record_property("candidates", str(rig.found))
    assert rig.other_is_free_of_S and rig.S_is_free_of_the_indexes, ("no side stream is free of the indexes' own streams: a launch on them would be hidden", rig.found)
    assert (buf.cpu().numpy() == real).all()


# ---------------------------------------------------------------------------------------------------------------- the nine families
@pytest.mark.parametrize("family,mode", sc.steady_calls())
def test_steady_state(rig, family, mode, monkeypatch, record_property):
    set_path(monkeypatch, family, mode)
    host = rig.host[(family, mode)]
    call = Call(rig, family, sc.mode_metric(mode), rig.ix, rig.ixl, total=total_of(family, host))
    check_call(rig, call, mode, host, record_property, want_path=rig.case.expected_path(family, mode))


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_first_use(rig, family, monkeypatch, record_property):
    """a fresh twin, never queried: the live-row views, the fp16 copy and the forest tables are made inside the call on S"""
    set_path(monkeypatch, family, "path2")
    host = rig.host[(family, "path2")]
    ix = rig.make(False)
    ixl = rig.make(True) if family == "cross" else None
    try:
        call = Call(rig, family, sc.METRICS[0], ix, ixl, total=total_of(family, host))
        check_call(rig, call, "path2", host, record_property, want_path=2, first_use=True)
        # S was chosen against the module's two indexes; this one's own stream was made afterwards and may share S's hardware queue, which would
        # have hidden a launch on it.  Recorded, not asserted: the same call once more, now with stream = NULL and fills pending on S
        free = rig.fill_came_last(rig.S, call.out, lambda: call.invoke(None))
        _measured["fresh_free"][family] = free
        record_property("fresh_index_stream_free_of_S", free)
    finally:
        if ixl is not None:
            ixl.close()
        ix.close()


@pytest.mark.parametrize("family", sc.SHORT)
def test_capacity_short(rig, family, monkeypatch, record_property):
    set_path(monkeypatch, family, "path2")
    host = rig.host[(family, "path2")]
    call = Call(rig, family, sc.METRICS[0], rig.ix, rig.ixl, short=True, total=total_of(family, host))
    check_call(rig, call, "path2", host, record_property, want_path=2)


# ---------------------------------------------------------------------------------------------------------------- the LSH search
def lsh_reference(rig):
    ids, keys, counts = rig.case.lsh
    ids = ids.copy()
    valid = np.arange(ids.shape[1])[None, :] < counts[:, None]
    ids[valid] += np.uint64(rig.case.base)
    ids[~valid], keys = fc.ALL, np.where(valid, keys, fc.ALL)
    return ids, keys, counts


def lsh_buffers(rig):
    torch, p = rig.torch, rig.case.p
    q = torch.empty_like(rig.q_real)
    out = [torch.empty((p["B"], p["k"]), dtype=torch.int64, device=rig.dev), torch.empty((p["B"], p["k"]), dtype=torch.int64, device=rig.dev),
           torch.empty((p["B"],), dtype=torch.int32, device=rig.dev)]
    return q, out


def test_lsh_search_batch_device(rig, monkeypatch, record_property):
    set_path(monkeypatch, "exact", "path2")
    p, m = rig.case.p, rig.za.L2SquaredDistance()
    q, out = lsh_buffers(rig)
    ptr = [t.data_ptr() for t in out]
    got, code, delay = run(rig, [(q, rig.q_real, rig.q_stale)], out, lambda s: rig.ix.search_batch_device(q.data_ptr(), p["B"], p["k"], m, ptr[0], ptr[1], ptr[2], s))
    record_property("delay_ms", round(delay, 2))
    assert code is None
    same((u64(got[0]), u64(got[1]), got[2].view(np.uint32)), lsh_reference(rig), ("ids", "keys", "counts"), lambda what: "search_batch_device on S: " + what)


def test_lsh_search_context(rig, monkeypatch, record_property):
    """begin(stream = S) with the queries pending behind the delay, finish, wait: complete when wait returns"""
    set_path(monkeypatch, "exact", "path2")
    p, m = rig.case.p, rig.za.L2SquaredDistance()
    q, out = lsh_buffers(rig)
    ptr = [t.data_ptr() for t in out]
    ctx = rig.ix.search_context()

    def round_(s):
        ctx.begin(q.data_ptr(), p["B"], p["k"], m, stream=s)
        ctx.finish(ptr[0], ptr[1], ptr[2])
        ctx.wait()

    try:
        got, code, delay = run(rig, [(q, rig.q_real, rig.q_stale)], out, round_)
    finally:
        ctx.close()
    record_property("delay_ms", round(delay, 2))
    assert code is None
    same((u64(got[0]), u64(got[1]), got[2].view(np.uint32)), lsh_reference(rig), ("ids", "keys", "counts"), lambda what: "begin / finish / wait on S: " + what)


# ---------------------------------------------------------------------------------------------------------------- the asynchronous three
def test_merge_topk_device_returns_and_completes_on_the_stream(rig, record_property):
    torch, za = rig.torch, rig.za
    from zebra_amd import sharding
    S_, k, B = 7, 100, 13
    ids, keys, counts = mc.make_case("ties", S_, B, k, 14)
    want = mc.merge_reference(ids, keys, counts, k)
    up = lambda a: torch.from_numpy(np.array(a)).to(rig.dev)  # noqa: E731
    real = [up(ids.view(np.int64)), up(keys.view(np.int64)), up(counts.view(np.int32))]
    stale = [up(np.roll(ids, 1, axis=1).view(np.int64)), up(np.roll(keys, 1, axis=1).view(np.int64)), up(np.zeros_like(counts).view(np.int32))]  # a valid input: no entries
    bufs = [torch.empty_like(t) for t in real]
    W = za.packed_result_words(B, k)
    packed_real = torch.zeros((S_, W), dtype=torch.int64, device=rig.dev)
    for s in range(S_):
        a, b_, c_ = sharding.packed_views(torch, packed_real[s], B, k)
        a.copy_(real[0][s]), b_.copy_(real[1][s]), c_.copy_(real[2][s])
    packed_stale, packed = torch.zeros_like(packed_real), torch.empty_like(packed_real)
    mk_out = lambda: [torch.empty((B, k), dtype=torch.int64, device=rig.dev), torch.empty((B, k), dtype=torch.int64, device=rig.dev),  # noqa: E731
                      torch.empty((B,), dtype=torch.int32, device=rig.dev)]
    plain, pk = mk_out(), mk_out()

    def both(s):
        za.merge_topk_device(0, S_, B, k, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), plain[0].data_ptr(), plain[1].data_ptr(),
                             plain[2].data_ptr(), stream=s)
        za.merge_topk_packed_device(0, S_, B, k, packed.data_ptr(), pk[0].data_ptr(), pk[1].data_ptr(), pk[2].data_ptr(), stream=s)

    inputs = [(b, r, s) for b, r, s in zip(bufs, real, stale)] + [(packed, packed_real, packed_stale)]
    got, code, delay = run(rig, inputs, plain + pk, both, asynchronous=True)
    record_property("delay_ms", round(delay, 2))
    assert code is None
    for who, g in (("zh_merge_topk_device", got[:3]), ("zh_merge_topk_packed_device", got[3:])):
        same((u64(g[0]), u64(g[1]), g[2].view(np.uint32)), want, ("ids", "keys", "counts"), lambda what: who + " on S: " + what)


def test_synth_queries_device_returns_and_completes_on_the_stream(rig, record_property):
    torch, za, p = rig.torch, rig.za, rig.case.p
    b, n_rows = 24, 100_000
    want = zo.synth_queries(b, p["d"], n_rows)
    out = torch.empty((b, p["d"]), dtype=torch.float32, device=rig.dev)
    got, code, delay = run(rig, [], [out.view(torch.int32)], lambda s: za.synth_queries_device(0, out.data_ptr(), n_rows, b, p["d"], stream=s), asynchronous=True)
    record_property("delay_ms", round(delay, 2))
    assert code is None
    same((got[0].view(np.uint32),), (np.ascontiguousarray(want).view(np.uint32),), ("queries",), lambda what: "zh_synth_queries_device on S: " + what)


def test_the_delay_outlasted_every_call(rig, record_property):
    """the figures of the module's docstring, recounted from what ran (and one more delay of its own, so that it has one when run alone): every
    delay within [20 ms, 100 ms] and at least twice the slowest of the idle calls that were timed (module docstring: not the first uses)"""
    run(rig, [], [], lambda s: rig.S.synchronize())
    slow = max(_measured["wall_ms"].items(), key=lambda kv: kv[1])
    lo, hi = min(_measured["delay_ms"]), max(_measured["delay_ms"])
    print("caller's stream: %d calls behind a delay of %.1f .. %.1f ms (asked: %.1f ms); slowest idle call %s %.3f ms; idle calls %s"
          % (len(_measured["delay_ms"]), lo, hi, rig.target_ms, slow[0], slow[1], {k: round(v, 2) for k, v in _measured["wall_ms"].items()}))
    print("caller's stream: a first use on an idle device (ms):", {k: round(v, 2) for k, v in _measured["first_use_ms"].items()},
          "; fresh indexes whose own stream was free of S:", _measured["fresh_free"])
    record_property("delay_ms_min", round(lo, 2))
    record_property("delay_ms_max", round(hi, 2))
    record_property("slowest_idle_call_ms", round(slow[1], 3))
    assert lo >= MIN_DELAY_MS and lo >= 2.0 * slow[1] and hi <= MAX_DELAY_MS and rig.target_ms <= MAX_DELAY_MS

"""Timing probe of zh_index_compact (LSHIndex.compact): median of 5 of zh_compact_info.ms (hipEvents on the index's stream), beside, in the same
process on the same device, (a) a plain device-to-device hipMemcpyAsync of rows_after * dim * 4 bytes -- the floor for moving that many bytes
once -- and (b) what a caller had to do before the call existed: clear, append the live rows again from host memory, build.  One case per
invocation, so that every step runs in a process (and under a time limit) of its own:
    python tests/probes/compact_probe.py move 768 10000000 0.10     rows = 10M x 768, 10 % removed at random (never-built index: the move alone)
    python tests/probes/compact_probe.py move 128 8000000 row0      only row 0 removed: every chunk overlaps itself
    python tests/probes/compact_probe.py refill 768 2000000 0.10    (b) at reduced size, with trees (max_node_size 8192, 8 trees), and compact beside it
    python tests/probes/compact_probe.py scan 768 10000000 0.30     one cfg3-shaped batch's sweep before and after compaction (30 % removed)
Every repetition makes the table again (append_synthetic), removes the same rows and compacts; a sample of moved rows is compared with the
generator at their old ids."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

PEAK = 8e12  # bytes/s, the device's HBM peak


def removed_rows(n, what, rng):
    if what == "row0":
        return np.zeros(1, np.uint64)
    return np.sort(rng.choice(n, int(n * float(what)), replace=False)).astype(np.uint64)


def fill(ix, n):
    for r0 in range(0, n, 1 << 21):
        ix.append_synthetic(min(1 << 21, n - r0), first_row=r0)


def memcpy_floor_ms(nbytes, reps=5):
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)  # a hipMemcpyAsync device-to-device
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return float(np.median(ms[1:]))


def move(d, n, what):
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    rng = np.random.default_rng(1)
    gone = removed_rows(n, what, rng)
    alive = np.ones(n, bool)
    alive[gone.astype(np.int64)] = False
    old_of_new = np.flatnonzero(alive)
    ms, info, ok = [], None, True
    for rep in range(6):  # the first is a warm-up
        ix = za.LSHIndex(d, za.LSHIndexOptions(64, 4), device=0)
        fill(ix, n)
        ix.remove(gone)
        _, info = ix.compact()
        ms.append(info["ms"])
        if rep == 0:
            for s in rng.integers(0, old_of_new.size - 8, 64).tolist():
                want = np.concatenate([zo.synth_rows(1, d, row0=int(o)) for o in old_of_new[s:s + 8]])
                ok &= ix.read_rows(s, 8).tobytes() == want.tobytes()
        ix.close()
    med = float(np.median(ms[1:]))
    floor = memcpy_floor_ms(info["rows_after"] * d * 4)
    return dict(case="move", dim=d, rows=n, removed=what, rows_after=info["rows_after"], rows_moved=info["rows_moved"],
                bytes_moved=info["bytes_moved"], scratch_bytes=info["scratch_bytes"], compact_ms=round(med, 3), ms=[round(x, 3) for x in ms[1:]],
                memcpy_d2d_ms=round(floor, 3), times_memcpy=round(med / floor, 2), moved_tb_s=round(info["bytes_moved"] / (med * 1e-3) / 1e12, 3),
                frac_of_peak=round(info["bytes_moved"] / (med * 1e-3) / PEAK, 3), spot_check=ok)


def refill(d, n, what):
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    rng = np.random.default_rng(1)
    gone = removed_rows(n, what, rng)
    alive = np.ones(n, bool)
    alive[gone.astype(np.int64)] = False
    X = np.concatenate([zo.synth_rows(min(1 << 19, n - r0), d, row0=r0) for r0 in range(0, n, 1 << 19)])
    out = dict(case="refill", dim=d, rows=n, removed=what, rows_after=int(alive.sum()))
    for how in ("compact", "clear_append_build"):
        wall = []
        for _ in range(3):
            ix = za.LSHIndex(d, za.LSHIndexOptions(8192, 8), device=0)
            fill(ix, n)
            ix.build()
            ix.remove(gone)
            t0 = time.perf_counter()
            if how == "compact":
                _, info = ix.compact()
                out["compact_event_ms"] = round(info["ms"], 3)
            else:
                live = np.ascontiguousarray(X[alive])  # the caller's own copy of the live rows, in host memory
                ix.clear()
                ix.append(live)
                ix.build()
            wall.append((time.perf_counter() - t0) * 1e3)
            ix.close()
        out[how + "_wall_ms"] = round(float(np.median(wall)), 1)
    return out


def scan(d, n, what):
    import torch
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    rng = np.random.default_rng(1)
    gone = removed_rows(n, what, rng)
    B, k, m = 1024, 100, za.L2SquaredDistance()
    ix = za.LSHIndex(d, za.LSHIndexOptions(8192, 8), device=0)
    fill(ix, n)
    ix.build()
    ix.remove(gone)
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(zo.synth_queries(B, d, n)).to(dev)
    ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    keys, counts = torch.empty_like(ids), torch.empty(B, dtype=torch.int32, device=dev)
    out = dict(case="scan", dim=d, rows=n, removed=what, batch=B, k=k)

    def sweep_ms(tag):
        ix.set_profiling(0)
        for _ in range(3):  # copies, views
            ix.search_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
        ix.set_profiling(1)
        ix.stats(reset=True)
        for _ in range(5):
            ix.search_batch_device(dq.data_ptr(), B, k, m, ids.data_ptr(), keys.data_ptr(), counts.data_ptr())
        st = ix.stats()
        out[tag] = dict(ms_sweep=round(st["ms_sweep"] / st["timed_batches"], 3), ms_total=round(st["ms_total"] / st["timed_batches"], 3),
                        table_scan=st["table_scan"], approx_scan=st["approx_scan"], ms_hash=round(st["ms_hash"] / st["timed_batches"], 3),
                        hash_from_scores=st["hash_from_scores"], prefiltered=st["prefiltered"], rows_swept=st["rows_swept"], row_copy_bytes=st["row_copy_bytes"])
        return ids.cpu().numpy().view(np.uint64).copy(), counts.cpu().numpy().copy()

    a_ids, a_counts = sweep_ms("before")
    new_ids, info = ix.compact()
    out["compact_ms"] = round(info["ms"], 3)
    out["copy_bytes_released"] = info["copy_bytes_released"]
    b_ids, b_counts = sweep_ms("after")
    same = bool((a_counts == b_counts).all())
    for b in range(B):
        c = int(a_counts[b])
        same &= bool((new_ids[a_ids[b, :c].astype(np.int64)] == b_ids[b, :c]).all())
    out["answers_equal_under_map"] = same
    return out


if __name__ == "__main__":
    case, d, n, what = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    res = dict(move=move, refill=refill, scan=scan)[case](d, n, what)
    print(json.dumps(res), flush=True)

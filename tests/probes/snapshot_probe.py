"""Timing probe of zh_index_save / zh_index_load (LSHIndex.save / LSHIndex.load): in ONE process, median of 5, for every shape
    save ms, load ms and GB/s of the file,
beside the floors a save overlaps and the restart path that existed before:
    (a) a plain hipMemcpy of the same row bytes, device to pinned host memory,
    (b) the time to write and fsync the same bytes to the same directory from host memory,
    (c) for load: append + build of the same rows from host memory (LSHIndex.append + LSHIndex.build).
    python tests/probes/snapshot_probe.py <directory>                  the default shapes: 2000000 x 768 and 8000000 x 128
    python tests/probes/snapshot_probe.py <directory> <rows> <dim>     one shape
A shape runs only if <directory> has room for its file twice over (the snapshot and (b)'s file); the probe prints that it checked and what it
found.  The index is built (max_node_size 8192, 8 trees: cfg3-like leaves) so that the file carries a forest; rows are the synthetic generator's.
One JSON line per shape."""
import json
import os
import shutil
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = 5


def median_ms(fn, reps=REPS):
    out = []
    for _ in range(reps + 1):  # the first is a warm-up
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out[1:]))


def d2h_floor_ms(nbytes):
    """hipMemcpy of nbytes from device memory to pinned host memory, in pieces of at most 1 GiB of pinned memory"""
    import torch
    piece = min(nbytes, 1 << 30)
    src = torch.empty(piece, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(piece, dtype=torch.uint8, pin_memory=True)

    def run():
        done = 0
        while done < nbytes:
            n = min(piece, nbytes - done)
            dst[:n].copy_(src[:n], non_blocking=True)
            done += n
        torch.cuda.synchronize()
    ms = median_ms(run)
    del src, dst
    torch.cuda.empty_cache()
    return ms


def write_floor_ms(path, nbytes):
    """write + fsync of nbytes from host memory, 64 MiB per write, to a new file in the same directory"""
    buf = np.random.default_rng(1).integers(0, 255, min(nbytes, 64 << 20), dtype=np.uint8).tobytes()

    def run():
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            done = 0
            while done < nbytes:
                done += os.write(fd, buf[:min(len(buf), nbytes - done)])
            os.fsync(fd)
        finally:
            os.close(fd)
    try:
        return median_ms(run)
    finally:
        if os.path.exists(path):
            os.unlink(path)


def shape(directory, n, d):
    import zebra_amd as za
    from oracle import zebra_oracle as zo
    row_bytes = n * d * 4
    free = shutil.disk_usage(directory).free
    need = 2 * (row_bytes + 8 * n * 4 + (64 << 20))
    rec = dict(rows=n, dim=d, row_bytes=row_bytes, directory=directory, space_checked=True, free_bytes=free, needed_bytes=need)
    if free < need:
        rec["skipped"] = "not enough space in the directory"
        print(json.dumps(rec), flush=True)
        return
    opts = za.LSHIndexOptions(8192, 8)
    ix = za.LSHIndex(d, opts, device=0)
    for r0 in range(0, n, 1 << 21):
        ix.append_synthetic(min(1 << 21, n - r0), first_row=r0)
    ix.build()
    p = os.path.join(directory, "snapshot_probe_%dx%d.zhs" % (n, d))
    infos = []
    save_ms = median_ms(lambda: infos.append(ix.save(p)))
    info = infos[-1]
    rec.update(file_bytes=info["file_bytes"], save_ms=save_ms, save_ms_device=float(np.median([i["ms_device"] for i in infos[1:]])),
               save_GBps=info["file_bytes"] / save_ms / 1e6)
    loaded = []

    def load():
        ld = za.LSHIndex.load(p, device=0)
        loaded.append(ld.snapshot)
        ld.close()
    load_ms = median_ms(load)
    rec.update(load_ms=load_ms, load_ms_device=float(np.median([i["ms_device"] for i in loaded[1:]])), load_GBps=info["file_bytes"] / load_ms / 1e6)
    # a spot check that the probe timed a working round trip
    ld = za.LSHIndex.load(p, device=0)
    s = max(0, n - 16)
    rec["rows_ok"] = bool(ld.read_rows(s, 16).tobytes() == zo.synth_rows(16, d, row0=s).tobytes() and ld.stored_rows() == n)
    ld.close()
    os.unlink(p)
    rec["d2h_memcpy_ms"] = d2h_floor_ms(row_bytes)
    rec["write_fsync_ms"] = write_floor_ms(p + ".floor", row_bytes)
    rec["save_over_slower_floor"] = save_ms / max(rec["d2h_memcpy_ms"], rec["write_fsync_ms"])
    # the restart path that existed before: the rows in host memory, append + build
    host = ix.read_rows(0, n) if row_bytes <= (8 << 30) else None
    ix.close()
    if host is not None:
        def rebuild():
            t = za.LSHIndex(d, opts, device=0)
            for r0 in range(0, n, 1 << 20):
                t.append(host[r0:r0 + (1 << 20)])
            t.build()
            t.close()
        rec["append_build_ms"] = median_ms(rebuild, reps=3)
    else:
        rec["append_build_ms"] = None
    print(json.dumps(rec), flush=True)


def main():
    if len(sys.argv) not in (2, 4):
        raise SystemExit(__doc__)
    directory = sys.argv[1]
    shapes = [(2_000_000, 768), (8_000_000, 128)] if len(sys.argv) == 2 else [(int(sys.argv[2]), int(sys.argv[3]))]
    for n, d in shapes:
        shape(directory, n, d)


if __name__ == "__main__":
    main()

"""The line the driver parses (round 4's final stdout line was 25.9 KB and BENCH_r04.json has `parsed: null`).
bench.compact_line on a canned full record -- round 4's own 25.9-KB record, committed under profiles/ -- must give one
strictly-JSON object below the limit that still carries the contract's keys, `roofline` and `cpu_baseline`.
Also the line of a plain run (no --full), the option checks and the --dump-outputs writer (bench.dump_outputs).  CPU only."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline")


def _canned():
    full = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_line.json")))
    assert len(json.dumps(full)) > 20000  # the record that did not parse
    return full


def _check(text):
    assert len(text.encode()) < 8192 and "\n" not in text
    assert "NaN" not in text and "Infinity" not in text
    j = json.loads(text, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    for k in CONTRACT:
        assert k in j, k
    return j


def test_compact_line_of_round_4s_record():
    import bench
    full = _canned()
    full["prefilter_dtype"] = bench.prefilter_dtype_of(full["roofline"])
    j = _check(bench.compact_line(full))
    assert j["value"] == float("%.6g" % full["value"]) and j["n_gpus"] == 1 and j["metric"] == "queries/sec"
    r = j["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "bytes_per_launch", "launch_ms", "hbm_frac"):
        assert k in r, k
    assert r["kernel"].startswith("scan_mfma_kernel") and "f16" in j["prefilter_dtype"]
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "queries/s" and c["sample"]
    assert j["config"]["workload"].startswith("cfg3") and "model" not in j["config"]
    assert set(j["other_configs"]) >= {"cfg2", "cfg4_one_of_8_shards", "cfg5_one_of_8_shards", "reference_default_options", "scale64m_n1"}
    assert j["host_buffers_qps"] > 0


def test_non_finite_values_and_oversized_parts():
    import bench
    full = _canned()
    full["roofline"]["frac"] = float("nan")
    full["roofline"]["traffic"] = float("inf")
    full["stage_ms_per_batch"]["hash"] = float("-inf")
    full["cpu_baseline"]["sample"] = "x" * 5000
    full["config"]["workload"] = "cfg3: " + "y" * 3000
    full["other_configs"] = {("cfg%d" % i): dict(full["other_configs"]["cfg2"]) for i in range(80)}  # an optional part that cannot fit
    j = _check(bench.compact_line(full))
    assert j["roofline"]["frac"] is None and j["roofline"]["traffic"] is None
    assert "other_configs" in j["dropped_for_length"] and "other_configs" not in j
    assert len(j["cpu_baseline"]["sample"]) <= 400


def test_compact_line_of_a_plain_run():
    """a run without --full: no R_unique pass (NaN through the figures that need it), no recall, CPU baselines, host-buffer leg or
    other configurations -- the line still carries the contract's keys, the timed run's own roofline figures, and no empty parts"""
    import bench
    full = _canned()
    for key in ("other_configs", "recall", "host_buffers", "host_buffers_qps", "cpu_baseline_bitexact", "detail"):
        full.pop(key, None)
    full["cpu_baseline"] = None
    full["roofline"]["unique_row_fraction"] = float("nan")
    full["roofline"]["s8d_equivalent_GBps"] = float("nan")
    j = _check(bench.compact_line(full))
    assert j["value"] == float("%.6g" % full["value"]) and j["ms_per_step"] == float("%.6g" % full["ms_per_step"])
    assert j["roofline"]["unique_row_fraction"] is None and j["roofline"]["launch_ms"] > 0 and j["roofline"]["frac"] > 0
    assert j["cpu_baseline"] is None and j["host_buffers_qps"] is None
    assert "recall" not in j and "other_configs" not in j and "dropped_for_length" not in j


def test_full_is_off_by_default_and_other_configs_need_it(monkeypatch):
    import pytest
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--only-other", "cfg2"])
    assert bench.parse().full is True
    for extra in (["--only-other", "cfg2"], ["--sleep-before-other", "5"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + extra)
        with pytest.raises(SystemExit):
            bench.parse()


def test_detail_record_is_strict_json(tmp_path, monkeypatch):
    import bench
    full = _canned()
    full["x"] = float("nan")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    doc, where = bench.write_detail(full)
    assert "NaN" not in doc and json.loads(doc)["x"] is None
    assert sorted(where) == ["bench_detail.json", os.path.join("gpurun_out", "bench_detail.json")]
    assert json.load(open(tmp_path / "gpurun_out" / "bench_detail.json"))["value"] > 0


def _last_step(b, k, rng):
    ids = rng.integers(0, 1 << 40, size=(b, k)).astype(np.int64)
    keys = np.sort(rng.random((b, k)) * 100.0, axis=1).view(np.int64)  # a key is the bit pattern of its f64 distance
    counts = rng.integers(1, k + 1, size=b).astype(np.int32)
    past = np.arange(k)[None, :] >= counts[:, None]
    ids[past] = -1  # UINT64_MAX past a query's count, as the library leaves it
    keys[past] = -1
    return {"ids": ids, "keys": keys, "counts": counts, "query_batch": 7}


def test_dump_outputs_writes_the_callers_arrays_in_float64(tmp_path):
    import bench
    last = _last_step(16, 10, np.random.default_rng(1))
    names = bench.dump_outputs(last, str(tmp_path / "out"))
    assert names == ["counts", "distances", "ids"]
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert (got["counts"] == last["counts"]).all()
    for b in range(16):
        c = int(last["counts"][b])
        assert (got["ids"][b, :c] == last["ids"][b, :c]).all() and (got["ids"][b, c:] == -1).all()
        assert (got["distances"][b, :c] == last["keys"][b, :c].view(np.float64)).all() and np.isinf(got["distances"][b, c:]).all()


def test_dump_outputs_samples_a_fixed_set_of_queries_over_the_limit(tmp_path):
    import bench
    last = _last_step(4096, 100, np.random.default_rng(2))
    limit = 1 << 20
    for run in ("a", "b"):
        names = bench.dump_outputs(last, str(tmp_path / run), limit=limit)
        assert names == ["counts", "distances", "ids", "query_rows"]
        assert sum(os.path.getsize(tmp_path / run / (n + ".npy")) for n in names) <= limit
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert (rows == np.load(tmp_path / "b" / "query_rows.npy")).all() and 0 < len(rows) < 4096
    ids = np.load(tmp_path / "a" / "ids.npy")
    r = rows.astype(np.int64)
    assert ids.shape == (len(rows), 100) and (ids[:, 0] == last["ids"][r, 0]).all()
    assert (np.load(tmp_path / "a" / "counts.npy") == last["counts"][r]).all()

"""bench.py's ONE JSON line stays parsable by the driver: round 5's line was 21 KB and `BENCH_r05.json.parsed` came back null.
The full result of that run (profiles/r05_final_bench_steps20_warmup5.json, a real `out` dict) through `bench.compact_line`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _canned():
    return json.load(open(os.path.join(ROOT, "profiles", "r05_final_bench_steps20_warmup5.json")))


def test_bench_line_is_compact_and_carries_the_contract():
    import bench
    out = _canned()
    assert len(json.dumps(out)) > 3 * bench.LINE_LIMIT          # the canned dict is the one that was too long
    text = bench.compact_line(out, "bench_detail.json")
    assert len(text) < 6144 and "\n" not in text
    rec = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "detail"):
        assert k in rec, k
    assert len(rec["config"]["workload"]) <= 300 and "model" not in rec["config"]
    roof = rec["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches", "sizes_per_step", "step"):
        assert k in roof, k
    assert roof["bound"] in ("hbm", "mfma") and 0 < roof["frac"] <= 1
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert abs(roof["frac"] - out["roofline"]["frac"]) < 1e-3 * out["roofline"]["frac"]
    assert abs(rec["value"] - out["value"]) <= 1.0
    cb = rec["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    assert set(rec["psnr_at_iter"]["delta_db"]) == {"100", "200", "300"}
    # one number per extras leg
    assert all(isinstance(v, (int, float, str)) or v is None for v in rec["extras"].values())
    assert len(rec["extras"]) >= len([k for k in out["extras"] if k != "psnr_at_iter"])


def test_bench_line_never_exceeds_the_limit_even_with_bloated_legs():
    import bench
    out = _canned()
    out["extras"] = {f"leg_{i}": {"ms_per_step": 1.0 + i, "note": "x" * 500} for i in range(400)}
    out["config"]["workload"] = "w" * 5000
    text = bench.compact_line(out)
    assert len(text) < 6144
    rec = json.loads(text)
    assert "roofline" in rec and "cpu_baseline" in rec and len(rec["config"]["workload"]) <= 300


def test_dump_outputs_keeps_dtypes_and_the_size_limit(tmp_path):
    """--dump-outputs: float64 stays float64, the rest is written as float32, small arrays whole; arrays beyond their share of
    the limit are a fixed sample, the same on every call, and the files together stay within the limit"""
    import numpy as np
    import bench
    rng = np.random.default_rng(1)
    arrays = {"loss": np.array([1.5, 2.5]), "n": np.array([3, 4], dtype=np.int64), "half": rng.random(10).astype(np.float16),
              "big": rng.random((64, 1000)).astype(np.float32), "bigger": rng.random(200000)}
    limit = 256 << 10
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["loss"].dtype == np.float64 and np.array_equal(got["loss"], arrays["loss"])
    assert got["n"].dtype == np.float32 and np.array_equal(got["n"], [3, 4])
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], arrays["half"].astype(np.float32))
    assert got["bigger"].dtype == np.float64 and 0 < got["bigger"].size < arrays["bigger"].size
    assert got["big"].dtype == np.float32 and 0 < got["big"].size < arrays["big"].size
    assert np.isin(got["bigger"], arrays["bigger"]).all() and np.isin(got["big"], arrays["big"]).all()
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_full_is_off_by_default_and_owns_the_cpu_protocol():
    """A plain `bench.py --gpus 1 --steps K --warmup W` run is the lean one: `--full` (per-kernel table, CPU baseline, extras legs)
    is off unless asked for, and the CPU baseline's own protocol is refused without it (before any GPU work starts)."""
    import subprocess
    import bench
    ap = bench.arg_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.gpus, plain.steps, plain.warmup) == (1, 20, 5)
    full = ap.parse_args(["--full", "--no-extras"])
    assert full.full and full.no_extras and not full.no_cpu_baseline
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-steps", "3,10"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--cpu-baseline-steps needs --full" in r.stderr and not r.stdout

"""bench.py's bookkeeping, without a GPU (and one plain run of it on the GPU): the algorithmic work figures are SURVEY.md section 8(d)'s, the workloads are the
BASELINE.json configs, and the CPU-baseline leg (the only place outside tests/ and smoke() that may touch oracle/) returns
what the JSON line needs."""
import importlib.util
import json
import os

import numpy as np
import pytest

import util


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(util.ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_algorithmic_work_matches_the_survey():
    b = _bench()
    M, tiles, N, X, Y, T = b.WORKLOADS["cfg2"]
    assert (M, N, X, Y) == (64, 256, 101, 101)
    D = X * Y
    assert D * M * N == 167_133_184                                   # MAC per frame
    assert b.algorithmic_bytes_per_frame("lerp", M, N, D, T) == 5_329_252
    assert b.algorithmic_bytes_per_frame("pad", M, N, D, T) == 2_717_796
    M, tiles, N, X, Y, T = b.WORKLOADS["cfg1"]
    assert b.algorithmic_bytes_per_frame("lerp", M, N, X * Y, T) == 127_972 and b.algorithmic_bytes_per_frame("pad", M, N, X * Y, T) == 96_996
    M, tiles, N, X, Y, T = b.WORKLOADS["cfg5"]
    assert X * Y * M * N == 34_162_868_224
    assert b.algorithmic_bytes_per_frame("lerp", M, N, X * Y, T) == 268_467_268 and b.algorithmic_bytes_per_frame("pad", M, N, X * Y, T) == 135_018_564


def test_metric_is_the_baseline_metric():
    base = json.load(open(os.path.join(util.ROOT, "BASELINE.json")))
    src = open(os.path.join(util.ROOT, "bench.py")).read()
    assert "beam-steered frames/sec (64 mics x 256 samples x 101x101 angles)" in src
    assert base["metric"].startswith("beam-steered frames/sec (64 mics")


def test_cpu_baseline_leg(monkeypatch):
    b = _bench()
    monkeypatch.setenv("BF_BENCH_CPU_REPLICAS", "2")
    out = b.cpu_baseline("cfg1", "lerp", budget_s=0.5)
    assert out["unit"] == "frames/s" and out["cores"] == 1 and out["kind"] in ("reference", "port") and out["value"] > 0
    assert out["all_cores"]["cores"] == 2 and out["all_cores"]["value"] > 0


def test_plain_run_is_lean_and_full_is_opt_in():
    """A plain `bench.py --gpus 1 --steps N --warmup W` runs only the headline; the side measurements need --full."""
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_and_caps_the_size(tmp_path, monkeypatch):
    b = _bench()
    maps = np.arange(40 * 10, dtype=np.float32).reshape(40, 10)
    b.dump_outputs(str(tmp_path / "all"), maps)
    got = np.load(tmp_path / "all" / "heatmaps.npy")
    assert got.dtype == np.float32 and np.array_equal(got, maps)
    assert sorted(os.listdir(tmp_path / "all")) == ["heatmaps.npy"]
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 1000)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), maps)
    rows = np.load(tmp_path / "s1" / "heatmaps_frame_index.npy")
    got = np.load(tmp_path / "s1" / "heatmaps.npy")
    assert got.nbytes + rows.nbytes <= 1000 and rows.dtype == np.float64
    assert np.array_equal(got, maps[rows.astype(int)]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "heatmaps_frame_index.npy"))      # the same sample every run


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step(tmp_path, oracle_lib):
    """bench.py as the driver runs it, plus --dump-outputs: the JSON line's headline fields, no side measurements, and the
    dumped heat-maps equal the oracle's for the seeded input frames."""
    import subprocess
    import sys
    import synth
    cmd = [sys.executable, os.path.join(util.ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "8",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert "cpu_baseline" not in d and "extra" not in d
    assert os.listdir(tmp_path) == ["heatmaps.npy"]
    maps = np.load(tmp_path / "heatmaps.npy")
    c = util.CONFIGS["cfg2"]
    assert maps.dtype == np.float32 and maps.shape == (8, c["X"] * c["Y"]) and np.isfinite(maps).all()
    orc = oracle_lib.Oracle(c["N"], c["X"], c["Y"], c["T"])
    frames = synth.frame_batch(c["M"], c["N"], 8)
    mics = np.arange(c["M"], dtype=np.int32)
    table = util.table_for("lerp", "cfg2")
    for f in (0, 7):
        assert util.max_rel(maps[f], orc.mimo_lerp(frames[f], table, mics)) <= util.REL_TOL, f

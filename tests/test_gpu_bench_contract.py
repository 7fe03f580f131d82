"""-m gpu: the driver's contract on bench.py -- one JSON line on stdout and nothing else, the keys and types the round
prompt names, the roofline object consistent with itself.  Short runs: 3 steps; --full with the roofline leg only (no
CPU baseline, no extras), and plain runs that leave every --full leg out and dump their outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, steps=3, warmup=1):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), *flags],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must carry exactly one line, got {len(lines)}: {r.stdout[:500]}"
    d = json.loads(lines[0])
    assert d["metric"] == "images/sec (640x640 bf16)" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "bf16" and d["data"] == "synthetic"
    assert isinstance(d["config"]["workload"], str) and "model" not in d["config"] and d["config"]["global_batch"] == 32
    assert d["config"]["hip_graph"] is True and d["config"]["rccl"] is None
    # value and ms_per_step describe the same timed region
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    assert 1000 < d["value"] < 20000, d["value"]
    return d


def test_bench_prints_one_json_line_with_the_contract_keys():
    d = _bench("--full", "--no-cpu-baseline", "--no-extra")
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.02 < rf["frac"] < 1.0
    assert rf["traffic"] is None or rf["traffic"] > 0
    lw = d["roofline_layerwise"]
    assert 0.05 < lw["frac"] < 1.0 and lw["ideal_ms"] < lw["measured_ms"]
    groups = d["roofline_groups"]
    for name in ("bn_forward(normalize+act)", "bn_backward(reduce+apply)", "conv_mfma(fwd+dgrad)", "wgrad_mfma", "loss"):
        assert name in groups and groups[name]["launches"] > 0, name
    assert d["roofline_hbm"]["bound"] == "hbm" and d["roofline_hbm"]["achieved"] < d["roofline_hbm"]["peak"]
    assert d["cpu_baseline"] is None and d["extra"] is None          # skipped by the flags of this run
    assert d["config"]["deterministic_mode"] is False


def test_plain_bench_run_times_only_the_steps_and_dumps_the_last_one(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    for key in ("roofline", "roofline_layerwise", "roofline_hbm", "roofline_groups", "cpu_baseline", "extra"):
        assert d[key] is None, key
    assert d["config"]["deterministic_mode"] is False               # the default path, as in every timed run
    arrays = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(arrays) == ["bn_running_stats", "loss", "params"]
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64e6
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.size and np.isfinite(a).all(), name
    assert arrays["loss"].shape == (3,) and abs(arrays["loss"][0] - d["config"]["final_loss"]) <= 1e-4 * abs(arrays["loss"][0])
    # the dumped step starts from the seeded state whatever ran before it: another run, with another step count, dumps
    # the same step up to the float-atomic BatchNorm noise (bench.dump_outputs: measured 2e-3 on the loss, 2e-5 on the
    # parameters, 6e-4 on the statistics)
    _bench("--dump-outputs", str(tmp_path / "again"), steps=1, warmup=0)
    for name, tol in (("loss", 1e-2), ("params", 2e-4), ("bn_running_stats", 5e-3)):
        a, b = arrays[name], np.load(tmp_path / "again" / (name + ".npy"))
        assert np.abs(a - b).max() <= tol * np.abs(a).max(), name

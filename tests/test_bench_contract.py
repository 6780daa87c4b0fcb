"""bench.py prints ONE JSON line with the keys the driver reads (metric/value/unit/n_gpus/steps/warmup/ms_per_step/
higher_is_better/scaling/vs_baseline/dtype/data/config), plus the `roofline` and `cpu_baseline` objects under --full;
--dump-outputs writes the output of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                 "vs_baseline", "dtype", "data", "config")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_default_workload_json_contract():
    d = _bench("--steps", "3", "--warmup", "1", "--no-fa2", "--full")
    for k in HEADLINE_KEYS + ("roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "TFLOPS" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "c3" in d["config"]["workload"] and "(4,32,8192,128)" in d["config"]["workload"]
    assert "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 3333.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.05 < rf["frac"] < 1.0
    assert rf["traffic"] is None or rf["traffic"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    # whole-job throughput with the quantizers included cannot exceed the attention kernel alone
    assert d["value"] <= rf["achieved"] * 1.02


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run prints the headline keys and nothing of --full; two runs with the same arguments dump the same
    output (identical inputs, deterministic operator)."""
    dumps = []
    for run in ("a", "b"):
        d = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / run))
        for k in HEADLINE_KEYS:
            assert k in d, k
        for k in ("roofline", "prepass", "bf16_inputs", "fa2_rocm", "cpu_baseline", "cpu_sdpa"):
            assert k not in d, k
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / run)) == ["o.npy"]
        o = np.load(tmp_path / run / "o.npy")
        assert o.dtype == np.float32 and o.nbytes <= 64 << 20 and np.isfinite(o).all() and np.abs(o).max() > 0
        dumps.append(o)
    assert np.array_equal(dumps[0], dumps[1])


def test_dump_output_sample_is_fixed(tmp_path):
    """dump_output writes a small tensor whole, and a large one as the same seeded sample of max_elems elements."""
    import bench
    small = torch.arange(6, dtype=torch.float16).view(2, 3)
    bench.dump_output(small, tmp_path / "s.npy", 16)
    assert np.array_equal(np.load(tmp_path / "s.npy"), np.arange(6, dtype=np.float32))
    big = torch.arange(1000, dtype=torch.float64)
    bench.dump_output(big, tmp_path / "b1.npy", 100)
    bench.dump_output(big.clone(), tmp_path / "b2.npy", 100)
    b1, b2 = np.load(tmp_path / "b1.npy"), np.load(tmp_path / "b2.npy")
    assert b1.dtype == np.float32 and b1.shape == (100,) and np.array_equal(b1, b2)
    assert (np.diff(b1) >= 0).all() and b1.min() >= 0 and b1.max() < 1000

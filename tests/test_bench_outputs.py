"""``bench.py --dump-outputs DIR``: the last timed step's outputs as float32 ``.npy`` files, the parameter sample fixed
from run to run; a plain run's line carries the headline fields and none of the ``--full`` measurements."""

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(n):
    flat = torch.arange(n, dtype=torch.float32)
    return types.SimpleNamespace(arena=types.SimpleNamespace(param_flat=flat), last_grad_norm=torch.tensor([2.5]))


def test_dump_outputs_training_sample_is_fixed(tmp_path):
    n = 3 * bench.DUMP_PARAM_SAMPLE + 17
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _engine(n), torch.tensor(0.125), None)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["grad_norm", "loss", "params_sample"] == sorted(b)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].tolist() == [0.125] and a["grad_norm"].tolist() == [2.5]
    s = a["params_sample"]
    assert s.shape == (bench.DUMP_PARAM_SAMPLE,) and np.array_equal(s, b["params_sample"])
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < n  # positions of the flat buffer, in order
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20


def test_dump_outputs_small_buffer_whole_and_inference(tmp_path):
    bench.dump_outputs(str(tmp_path / "t"), _engine(10), torch.tensor(1.0), None)
    assert np.array_equal(np.load(tmp_path / "t" / "params_sample.npy"), np.arange(10, dtype=np.float32))
    out = {"modic": torch.ones(2, 4, dtype=torch.bfloat16), "herniation": torch.zeros(2)}
    bench.dump_outputs(str(tmp_path / "i"), None, None, out)
    assert sorted(os.listdir(tmp_path / "i")) == ["pred_herniation.npy", "pred_modic.npy"]
    assert np.load(tmp_path / "i" / "pred_modic.npy").dtype == np.float32


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(dev, tmp_path):
    """One small plain run (ResNet-18 classification, 64x64, batch 4): --steps sets the timed steps, the line has the
    headline fields and nothing that belongs behind --full, and the outputs are written."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "classification", "--backbone", "resnet18", "--image-size", "64", "--batch", "4",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["higher_is_better"] is True
    assert res["unit"] == "images/sec" and res["dtype"] == "bf16"
    assert abs(res["value"] - 4 / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    for k in ("cpu_baseline", "cpu_baseline_configs0", "configs3_classification", "dp_rehearsal"):
        assert k not in res
    assert res["main_queue"] is None and "kernels" not in res["roofline"]
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,) and abs(float(loss[0]) - res["loss"]) <= 1e-5 * abs(res["loss"])
    assert np.isfinite(np.load(tmp_path / "params_sample.npy")).all()
    assert np.load(tmp_path / "grad_norm.npy")[0] > 0

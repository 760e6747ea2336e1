"""The benchmark's contract: a plain `bench.py` run times exactly --steps steps, prints the headline line without the
--full figures, and `--dump-outputs DIR` writes the last timed step's outputs as float32 / float64 .npy files of at
most 64 MB.  One child process (the bench initialises its own device context)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump_outputs(dev, lib_path, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    for key in ("value_fp32_mfma", "strong_scaling", "roofline", "kernel_families_ms_per_step", "parity_vs_oracle",
                "cpu_baseline"):
        assert key not in line, key
    # 64 clips x 172 frames x 512 samples: the signal in full, phase / harmonic / noise of every fourth clip
    shapes = {"signal": (64, 88064), "phase": (16, 172, 1), "harmonic": (16, 88064), "noise": (16, 88064)}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    total = 0
    for name, shape in shapes.items():
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == shape, (name, a.dtype, a.shape)
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    sig = np.load(os.path.join(tmp_path, "signal.npy"))
    assert float(np.sqrt(np.mean(sig.astype(np.float64) ** 2))) > 0

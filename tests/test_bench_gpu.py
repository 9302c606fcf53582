"""GPU test of a plain bench.py run (no --full): the result line of the timed steps only, and --dump-outputs' files from the
last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--size", "256",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-3000:]
    files = sorted(os.listdir(out_dir))
    assert all(f.endswith(".npy") for f in files)
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in files}


@pytest.mark.timeout(900)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    rec, arrays = _run(tmp_path / "a")
    assert rec["steps"] == 4 and rec["warmup"] == 2 and rec["n_gpus"] == 1
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["metric"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] * rec["ms_per_step"] - 2 * 1e3) < 1e-6 * 2e3       # 2 images per step: value = 2 / (ms_per_step / 1000)
    assert rec["roofline"] is None                                             # what only --full measures is absent
    assert not {"cpu_baseline", "parity", "categories", "frozen_backbone_encoder"} & set(rec)
    assert {"grad_norm", "params_sample"} <= set(arrays)
    assert sum(x.nbytes for x in arrays.values()) <= 64 * 10 ** 6
    for k, x in arrays.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), k
    assert arrays["params_sample"].size > 10 ** 6
    losses = [k for k in arrays if k.startswith("loss_")]
    assert len(losses) == 30                                                   # 3 weighted terms x 10 prediction heads
    total = sum(float(arrays[k]) for k in losses)                              # the losses of the LAST timed step
    assert abs(total - rec["config"]["final_total_loss"]) <= 1e-4 * abs(total) + 1e-6
    # a second run with the same arguments: the same outputs up to the rounding of the backward's float atomics
    _, again = _run(tmp_path / "b")
    assert sorted(again) == sorted(arrays)
    for k in losses + ["grad_norm"]:
        np.testing.assert_allclose(again[k], arrays[k], rtol=1e-4, atol=1e-6, err_msg=k)
    p, q = arrays["params_sample"].astype(np.float64), again["params_sample"].astype(np.float64)
    assert np.abs(p - q).max() <= 1e-5 * np.abs(p).max()

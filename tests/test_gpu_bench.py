"""bench.py on the GPU at small sizes: a plain run times exactly --steps fits, prints the headline line without the secondary
blocks and dumps the last timed fit's results; --full adds the secondary blocks (the ones that need no other child or configuration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--frames", "64", "--scene", "20000", "--iters", "40"]


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_times_the_steps_and_dumps_the_last_fit(tmp_path):
    d = _bench(SMALL + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - 64) < 1e-6 * 64
    for block in ("with_reference_logging", "roofline", "blendshape_gemm", "exact_fp32", "other_configs", "cpu_baseline"):
        assert block not in d, block
    body, scale, cam = (np.load(tmp_path / f"{n}.npy") for n in ("body_rec", "scale", "camera_ext"))
    assert body.shape == (64, 75) and scale.shape == (1,) and cam.shape == (64, 4, 4)
    assert body.dtype == scale.dtype == cam.dtype == np.float32
    assert np.isfinite(body).all() and np.isfinite(cam).all() and np.isfinite(scale).all()


def test_full_run_adds_the_secondary_blocks():
    d = _bench(SMALL + ["--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-exact-fp32"])
    assert d["steps"] == 1 and d["value"] > 0
    assert d["with_reference_logging"]["value"] > 0
    assert d["roofline"]["ms_per_launch"] > 0 and d["roofline"]["per_kernel"] is not None
    assert d["blendshape_gemm"]["ms_per_launch"] > 0

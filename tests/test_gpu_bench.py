"""GPU: the plain bench.py line (no --full) -- exactly --steps timed steps, the headline keys and nothing of the legs -- and
--dump-outputs: what the last timed step returned, written as .npy, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp, name, extra=()):
    out_dir = os.path.join(str(tmp), name)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "C2",
           "--dump-outputs", out_dir] + list(extra)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), out_dir


def test_plain_line_times_exactly_steps_and_dumps_the_last_step(tmp_path, gpu_device):
    d, out_dir = _bench(tmp_path, "a")
    assert d["steps"] == 3 and d["steps_timed"] == 3 and d["full"] is False
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0
    assert abs(d["ms_per_step"] - d["timed_region_ms"] / 3) <= 1e-3 * d["ms_per_step"] + 1e-3
    for k in ("roofline", "stages", "cpu_baseline", "forward_mpix_s", "c5", "clustered", "dropin", "reference_lists", "step_end_stages"):
        assert k not in d, k
    files = sorted(os.listdir(out_dir))
    B = d["config"]["views_per_step_per_gpu"]
    for v in range(B):
        for k in ("render", "radii", "depth", "alpha_T", "viewspace_grad", "num_rendered", "loss"):
            assert "view%d_%s.npy" % (v, k) in files, (v, k, files)
    assert "params_flat.npy" in files
    total = sum(os.path.getsize(os.path.join(out_dir, f)) for f in files)
    assert total <= 64 << 20
    arrays = {f: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert float(arrays["view0_num_rendered.npy"][0]) > 0 and (arrays["view0_radii.npy"] > 0).any()
    # the same arguments: the same inputs, the same sample positions, the same outputs.  The last timed step starts from the seeded
    # state, so everything its forward computes is bit-identical; the screen-space gradient and the parameters carry the rounding of
    # the backward's float atomics (their order differs from run to run), which Adam's first step from zero moments turns into a
    # sign flip for the odd element whose gradient is at that noise level
    d2, out_dir2 = _bench(tmp_path, "b")
    assert sorted(os.listdir(out_dir2)) == files
    for f, a in arrays.items():
        b = np.load(os.path.join(out_dir2, f))
        assert a.shape == b.shape, f
        if f.endswith(("viewspace_grad.npy", "params_flat.npy")):
            scale = float(np.abs(a).max())
            diff = np.abs(b.astype(np.float64) - a)
            assert float(diff.max()) <= 1e-4 * scale, (f, float(diff.max()), scale)
            assert float((diff > 1e-6 * scale).mean()) <= 1e-4, (f, float((diff > 1e-6 * scale).mean()))
        else:
            np.testing.assert_array_equal(b, a, err_msg=f)

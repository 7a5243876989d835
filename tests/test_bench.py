"""bench.py as the headline is measured: a plain run (the timed steps and nothing beside them) and --dump-outputs, whose
files let two builds be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, C, H, W, V = 20000, 128, 968, 1296, 4   # cfg3's frame and cameras, a small scene


def _plain_run(dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--points", str(P), "--channels", str(C), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        line = _plain_run(d)
        assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
        assert line["unit"] == "Gpixel*channels/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
        assert abs(line["value"] - V * H * W * C / (line["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * line["value"]
        for leg in ("single_view", "api_path", "classic_count", "backward", "roofline", "cpu_baseline", "multi_gpu_configs"):
            assert leg not in line, leg   # --full only
    names = sorted(os.listdir(dirs[0]))
    assert names == ["color_channel_sum.npy", "color_index.npy", "color_sample.npy", "num_rendered.npy", "radii.npy"]
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 << 20
    for n in names:   # the same arguments give the same inputs, and the forward is deterministic
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n
    num_rendered, radii = np.load(dirs[0] / "num_rendered.npy"), np.load(dirs[0] / "radii.npy")
    assert num_rendered.shape == (V,) and (num_rendered > 0).all()
    assert radii.shape == (V, P) and (radii >= 0).all() and (radii > 0).any()
    index, sample = np.load(dirs[0] / "color_index.npy"), np.load(dirs[0] / "color_sample.npy")
    assert sample.shape == (V, index.size) and np.isfinite(sample).all()
    assert index.min() >= 0 and index.max() < C * H * W and (np.diff(index) >= 0).all()
    assert np.load(dirs[0] / "color_channel_sum.npy").shape == (V, C)

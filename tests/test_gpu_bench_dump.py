"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy -- the same arrays from run
to run whatever --steps is, and the same image from the torch.distributed path and the library-owned frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--width", "256", "--samples", "2", "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0", "--lean"]


def _bench(out_dir, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args, "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    files = sorted(os.listdir(out_dir))
    assert files and all(f.endswith(".npy") for f in files)
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    return line, arrays


def test_dump_outputs_repeat_whatever_the_step_count(tmp_path):
    line2, a2 = _bench(tmp_path / "k2", "--steps", "2")
    line5, a5 = _bench(tmp_path / "k5", "--steps", "5")
    assert line2["steps"] == 2 and line5["steps"] == 5
    assert set(a2) == {"image_index", "image_rgba", "ray_index", "ray_end_state", "ray_flags", "ray_n_steps", "ray_n_accepted"}
    # 256 x 256 x 2: small enough to be written whole
    assert np.array_equal(a2["image_index"], np.arange(256 * 256)) and a2["image_rgba"].shape == (256 * 256, 4)
    assert np.array_equal(a2["ray_index"], np.arange(2 * 256 * 256)) and a2["ray_end_state"].shape == (2 * 256 * 256, 6)
    assert (a2["ray_n_steps"] > 0).all() and (a2["ray_n_accepted"] <= a2["ray_n_steps"]).all()
    flags = a2["ray_flags"].astype(np.int64)     # the sky frame: rays fall into the horizon (1) or reach curve_end (4)
    assert (flags == 1).any() and (flags == 4).any()
    for k in a2:
        assert np.array_equal(a2[k], a5[k]), k


def test_dump_outputs_same_image_from_the_library_frame(tmp_path):
    _, a = _bench(tmp_path / "torch", "--steps", "2")
    _, b = _bench(tmp_path / "frame", "--steps", "2", "--single-process")
    assert set(b) == {"image_index", "image_rgba"}
    assert np.array_equal(a["image_index"], b["image_index"]) and np.array_equal(a["image_rgba"], b["image_rgba"])

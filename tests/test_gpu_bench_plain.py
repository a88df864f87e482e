"""bench.py without --full: the headline alone -- set-up, warm-up, the timed steps, --dump-outputs, the JSON line -- within
30 s outside its steps; with --full the blocks measured beside the headline, and the same dumped arrays."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what only a --full run measures or checks (single GPU, frame workload)
FULL_ONLY = ("sky_frame_dir_only", "regimes", "strong_predicted", "pipelined", "host_buffer_call", "cpu_baseline")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    seconds = time.perf_counter() - t
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), seconds


def test_plain_run_is_the_headline_alone_and_spends_at_most_30_s_outside_its_steps():
    """The flagship command, whole process from start to exit: wall time less (N + W) x ms_per_step <= 30 s."""
    n, w = 20, 5
    line, seconds = _bench("--gpus", "1", "--steps", str(n), "--warmup", str(w))
    outside = seconds - (n + w) * line["ms_per_step"] * 1e-3
    print(f"plain run: {seconds:.2f} s in all, {line['ms_per_step']:.4f} ms per step, {outside:.2f} s outside its steps")
    assert outside <= 30.0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == n and line["warmup"] == w and line["n_gpus"] == 1 and "1024x1024x5" in line["metric"]
    assert line["value"] > 0 and abs(line["value"] - 1024 * 1024 * 5 / (line["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * line["value"]
    assert len(line["ms_per_step_samples"]) == 5 and line["ms_per_step"] == float(np.median(line["ms_per_step_samples"]))
    assert line["config"]["run"].startswith("plain")
    assert not [k for k in FULL_ONLY if k in line]
    # the roofline figures the timed region's own HIP events give; nothing calibrated, no live counter passes
    r = line["roofline"]
    assert r["frac"] > 0 and r["kernel_ms"] == r["trace_call_ms"] and "calibration" not in r
    assert not str(r["traffic_source"]).startswith("live")


def test_full_run_adds_the_secondary_blocks_and_dumps_the_same_arrays(tmp_path):
    small = ["--width", "256", "--samples", "2", "--steps", "4", "--warmup", "2", "--ramp-seconds", "0"]
    plain, _ = _bench(*small, "--dump-outputs", str(tmp_path / "plain"))
    full, _ = _bench(*small, "--full", "--live-pmc", "0", "--cpu-seconds", "0.2", "--emulate-shards", "", "--dump-outputs", str(tmp_path / "full"))
    assert plain["config"]["run"].startswith("plain") and full["config"]["run"] == "full"
    assert not [k for k in FULL_ONLY if k in plain]
    for k in ("sky_frame_dir_only", "regimes", "pipelined", "host_buffer_call", "cpu_baseline"):
        assert "error" not in full[k], (k, full[k])
    assert "calibration" in full["roofline"] and "calibration" not in plain["roofline"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files and files == sorted(os.listdir(tmp_path / "full"))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f


def test_lean_run_keeps_what_the_profiling_scripts_read():
    """--lean (a run under a profiler) launches what it always did: no clock reads, none of the secondary blocks, and
    behind the timed steps the 8 profiled calls that give the trace kernel's share of a call -- scripts/timed_region_stats.py
    drops exactly those from a kernel trace and compares the rest with this line's frac.  Kerr: prepare | trace | finalize,
    so the share is below 1 and kernel_ms below the call's time; a plain run reports the call's time."""
    small = ["--width", "256", "--samples", "2", "--steps", "4", "--warmup", "2", "--ramp-seconds", "0", "--rhs", "kerr"]
    lean, _ = _bench(*small, "--lean", "--full")          # (--lean overrides --full)
    plain, _ = _bench(*small)
    assert lean["config"]["run"].startswith("lean") and not [k for k in FULL_ONLY if k in lean]
    assert lean["sclk_mhz_per_repetition"] == [None] * 5
    r, p = lean["roofline"], plain["roofline"]
    assert "calibration" not in r and r["ray_steps_per_launch"] > 0 and r["frac"] > 0
    assert "share of a call (" in r["kernel_ms_is"] and 0.0 < r["kernel_ms"] / r["trace_call_ms"] < 1.0
    assert p["kernel_ms"] == p["trace_call_ms"] and "--full" in p["kernel_ms_is"]

"""bench_disk_crossings.py -- what the higher-order disk images cost on the disk workload's frames (BASELINE.json configs[2]: the
five camera inclinations of bench.py --workload disk, 1024 x 1024 x S each, thin disk 4.5 .. 10.5 r_s, exit sphere at 40).
Two lines on the same rays, in alternating blocks, one DeviceFrame per camera (the layered shade's record array belongs to one
frame: the five frames are five trace calls in BOTH lines):

    crossings   bhg_trace_crossings_device (K = 3 records per ray, one lane per ray) + bhg_shade_disk_layers_device
    disk_off    bhg_trace_device with the disk off (the persistent trace kernel, the start-step cache off) + the scene shade

The disk-off trace takes the same step sequence, ray for ray (tests/test_gpu_disk_crossings.py), so the difference is the price
of the lane-per-ray shape plus the crossings.  Prints one JSON line.

    python scripts/bench_disk_crossings.py [--steps 10] [--warmup 3] [--reps 3] [--size 1024] [--samples 1] [--kerr]
                                           [--opacity 0.5]

frame_ms = trace + shade of the five frames per step; trace_ms / shade_ms = the five calls of each kind alone.  trace_ratio is
the like-for-like figure; the disk-off line's shade colours the sky alone, so shade_ms and frame_ratio also hold the colouring
of the disk.  Host wall clock around synchronised blocks; medians over --reps blocks of each.  Run it under `rocprofv3
--kernel-trace --stats -- python scripts/bench_disk_crossings.py` for the kernels' own times (disk_crossings_kernel,
shade_pixels_kernel<LayersColour<...>>)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_common import DISK, Workload  # noqa: E402
from timed_region_stats import box_id  # noqa: E402  (scripts/: this script's own directory)

K = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--opacity", type=float, default=0.5)
    ap.add_argument("--kerr", action="store_true", help="Kerr a/M = 0.9 instead of Schwarzschild")
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream

    W = H = a.size
    S = a.samples
    ctx = _ffi.Context(0)
    form = dict(rhs_form=_ffi.RHS_KERR_BL if a.kerr else _ffi.RHS_CHRISTOFFEL, spin=0.45 if a.kerr else 0.0)
    p_on = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1], **form)
    p_off = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, **form)
    jitter = python_random_stream(42.0, 2 * S * W * H)
    sky = synthetic_sky(2048, 1024)
    disk_tex = synthetic_sky(1024, 128, seed=3)
    frames = {"crossings": [], "disk_off": []}
    for cam in Workload.disk_cameras():
        for line in frames:
            f = DeviceFrame(ctx, W, H, S, jitter=jitter, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, start_cache=False, **cam)
            f.set_sky(sky)
            if line == "crossings":
                f.set_disk(DISK[0], DISK[1], disk_tex)
                f.set_disk_layers(K, a.opacity)
            f.generate_rays()
            frames[line].append(f)
    params = {"crossings": p_on, "disk_off": p_off}

    def block(line, k, trace=True, shade=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            for f in frames[line]:
                if trace:
                    f.trace(params[line])
                if shade:
                    f.shade()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    ms = {line: {"frame": [], "trace": [], "shade": []} for line in frames}
    for line in frames:
        block(line, a.warmup)
    for _ in range(a.reps):
        for line in frames:
            ms[line]["frame"].append(block(line, a.steps))
            ms[line]["trace"].append(block(line, a.steps, shade=False))
            ms[line]["shade"].append(block(line, max(a.steps, 20), trace=False))
    # the two lines traced the same rays through the same steps
    same = all(torch.equal(x.d_steps, y.d_steps) and torch.equal(x.d_flags, y.d_flags)
               for x, y in zip(frames["crossings"], frames["disk_off"]))
    n_cross = torch.cat([f.d_n_cross for f in frames["crossings"]]).cpu().numpy()
    med = lambda v: float(np.median(v))   # noqa: E731
    out = {
        "workload": f"{W}x{H} x{S} {'Kerr a/M=0.9' if a.kerr else 'Schwarzschild'} + thin disk {DISK[0]}..{DISK[1]} r_s, exit sphere 40, "
                    f"5 camera inclinations per step (bench.py --workload disk), one trace call and one shade call per camera",
        "device": ctx.name, "box": box_id(),
        "max_crossings": K, "opacity": a.opacity,
        "same_flags_and_steps_in_both_lines": bool(same),
        "rays_by_crossings_0_1_2_3plus": [int((n_cross == 0).sum()), int((n_cross == 1).sum()), int((n_cross == 2).sum()),
                                          int((n_cross >= 3).sum())],
    }
    for line in frames:
        for what in ("frame", "trace", "shade"):
            out[f"{what}_ms_{line}"] = med(ms[line][what])
    out["frame_ratio"] = out["frame_ms_crossings"] / out["frame_ms_disk_off"]
    out["trace_ratio"] = out["trace_ms_crossings"] / out["trace_ms_disk_off"]
    out["samples_ms"] = ms
    out["what"] = (f"trace + shade of the 5 frames (frame_ms), the 5 trace calls (trace_ms) and the 5 shade calls (shade_ms) alone: "
                   f"the crossings trace (K = {K}) with the layered shade against bhg_trace_device with the disk off (start-step cache "
                   f"off) with the scene shade, alternating blocks of {a.steps} steps after {a.warmup} warm-up steps, medians of "
                   f"{a.reps}; host wall clock around synchronised blocks.  trace_ratio is the like-for-like figure (the same rays "
                   f"through the same steps).  The two shades are NOT alike -- the layered shade colours up to {K} textured disk "
                   f"crossings per ray and the sky, the disk-off line's shade the sky alone -- so shade_ms and frame_ratio hold "
                   f"the disk's colouring as well, not the price of the crossings alone")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()

"""bench_travel_time.py -- what the light travel time costs beside the crossings trace: one 1024 x 1024 ray
set (the camera at r = 30, 80 degrees from the axis, thin disk 3 .. 12 r_s, exit sphere at 40), traced by

    crossings     bhg_trace_crossings_device (K = 3 records per ray)
    travel_time   bhg_travel_time_device (the same loop plus six quadrature nodes per accepted step, t_end and t_cross)

in alternating blocks.  Prints one JSON line.

    python scripts/bench_travel_time.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--kerr]

Both are lane-per-ray kernels that leave no pass events behind (bhg_last_pass_ms times the persistent trace kernels only), so the
figures are the device's own event times around each call on the stream (torch.cuda.Event), medians over --reps blocks."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from timed_region_stats import box_id  # noqa: E402  (scripts/: this script's own directory)

K = 3
DISK = (3.0, 12.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--kerr", action="store_true", help="Kerr a/M = 0.9 instead of Schwarzschild")
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame

    ctx = _ffi.Context(0)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1],
                         rhs_form=_ffi.RHS_KERR_BL if a.kerr else _ffi.RHS_CHRISTOFFEL, spin=0.45 if a.kerr else 0.0)
    frames = {}
    for line, rate in (("crossings", 0.0), ("travel_time", 0.05)):
        f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                        start_cache=False)
        f.set_disk(DISK[0], DISK[1], None)
        f.set_disk_layers(K, 0.5, phase_rate=rate)
        f.generate_rays(p)
        frames[line] = f

    def block(line, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            frames[line].trace(p)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    ms = {line: [] for line in frames}
    for line in frames:
        block(line, a.warmup)
    for _ in range(a.reps):
        for line in frames:
            ms[line].append(block(line, a.steps))
    x, y = frames["crossings"], frames["travel_time"]
    same = bool(torch.equal(x.d_end, y.d_end) and torch.equal(x.d_flags, y.d_flags) and torch.equal(x.d_steps, y.d_steps)
                and torch.equal(x.d_cross.nan_to_num(), y.d_cross.nan_to_num()) and torch.equal(x.d_n_cross, y.d_n_cross))
    t_end = y.d_t_end.cpu().numpy()
    out = {"workload": f"{a.size}x{a.size} x1 {'Kerr a/M=0.9' if a.kerr else 'Schwarzschild'}, camera r = 30 at 80 deg, thin disk "
                       f"{DISK[0]}..{DISK[1]} r_s, exit sphere 40, K = {K}",
           "device": ctx.name, "box": box_id(),
           "crossings_ms": float(np.median(ms["crossings"])), "travel_time_ms": float(np.median(ms["travel_time"])),
           "same_results_in_both_lines": same, "finite_t_end": int(np.isfinite(t_end).sum()), "rays": int(t_end.size),
           "samples_ms": ms}
    out["ratio"] = out["travel_time_ms"] / out["crossings_ms"]
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()

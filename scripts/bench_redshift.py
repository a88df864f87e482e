"""bench_redshift.py -- what redshift costs on the disk workload (BASELINE.json configs[2]): the five camera inclinations of
bench.py --workload disk (1024 x 1024 x 1 each, thin disk 4.5 .. 10.5 r_s, one FrameBatch trace with per-ray origins, shaded
frame by frame into one float RGBA image), timed with redshift off and on (DeviceFrame.set_redshift: disk, objects and sky
weighted by g^4) in alternating blocks on the same frames.  Prints one JSON line.

    python scripts/bench_redshift.py [--steps 10] [--warmup 3] [--reps 3] [--kerr]

frame_ms = trace + shade of the five frames per step; shade_ms = the five shade calls alone (the trace does not change with
redshift: only the shade kernels take their redshift instance).  Host wall clock around synchronised blocks; medians over
--reps blocks of each.  Run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_redshift.py` for the shade
kernels' own times (shade_pixels_kernel<SceneColour<RS = false / true, ...>>)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--kerr", action="store_true", help="Kerr a/M = 0.9 instead of Schwarzschild")
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import FrameBatch, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream

    W = H = a.size
    S = 1
    ctx = _ffi.Context(0)
    params = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1],
                              rhs_form=_ffi.RHS_KERR_BL if a.kerr else _ffi.RHS_CHRISTOFFEL, spin=0.45 if a.kerr else 0.0)
    batch = FrameBatch(ctx, Workload.disk_cameras(), W, H, S, jitter=python_random_stream(42.0, 2 * S * W * H),
                       fov_x=0.9, fov_y=0.9, sampling_seed=42.0)
    sky = synthetic_sky(2048, 1024)
    disk_tex = synthetic_sky(1024, 128, seed=3)
    for f in batch.frames:
        f.set_sky(sky)
        f.set_disk(DISK[0], DISK[1], disk_tex)
    batch.generate_rays()
    image = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")

    def block(on, k, shade_only=False):
        batch.set_redshift(("disk", "objects", "sky") if on else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            if not shade_only:
                batch.trace(params)
            for f in batch.frames:
                f.shade_f32(image)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    batch.trace(params)
    block(False, a.warmup)
    block(True, a.warmup)
    frame_ms = {False: [], True: []}
    shade_ms = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            frame_ms[on].append(block(on, a.steps))
            shade_ms[on].append(block(on, max(a.steps, 20), shade_only=True))
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({
        "workload": f"{W}x{H} x{S} {'Kerr a/M=0.9' if a.kerr else 'Schwarzschild'} + thin disk {DISK[0]}..{DISK[1]} r_s, "
                    f"5 camera inclinations per step (bench.py --workload disk)",
        "device": ctx.name,
        "frame_ms_off": med(frame_ms[False]), "frame_ms_on": med(frame_ms[True]),
        "frame_cost": med(frame_ms[True]) / med(frame_ms[False]) - 1.0,
        "shade_ms_off": med(shade_ms[False]), "shade_ms_on": med(shade_ms[True]),
        "samples_ms": {"frame_off": frame_ms[False], "frame_on": frame_ms[True], "shade_off": shade_ms[False],
                       "shade_on": shade_ms[True]},
        "what": f"trace + shade_f32 of the 5 frames (frame_ms) and shade_f32 alone (shade_ms), redshift off / on (disk, objects "
                f"and sky weighted by g^4), alternating blocks of {a.steps} steps after {a.warmup} warm-up steps, medians of "
                f"{a.reps}; host wall clock around synchronised blocks"}))
    ctx.close()


if __name__ == "__main__":
    main()

"""bench_object_motion.py -- what moving object spheres cost on the orbit workload (BASELINE.json configs[3]): the 2048 x 2048 x 16
frame of the orbiting-sphere animation (bench.py --workload orbit: a lit sphere of radius 1.5 on an inclined r = 8 r_s orbit,
one step = one frame of the animation, the sphere moved per step), redshift on (objects and sky, g^4), each frame shaded into
its fp64 RGBA image by DeviceFrame.shade() -- the sphere at rest, or moving and turning with its orbit
(observer.circular_orbit_motion, set_object_motion) -- in alternating blocks.  Prints one JSON line.

    python scripts/bench_object_motion.py [--steps 10] [--warmup 3] [--reps 3] [--size 2048] [--samples 16]

frame_ms = trace + shade of one frame per step; shade_ms = the shade call alone on the block's last frame (the trace does not
change with motion: only the shade kernel takes its motion instance).  Host wall clock around synchronised blocks; medians over --reps blocks of each.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_object_motion.py` for the shade kernels' own times
(shade_pixels_kernel<SceneColour<true, false, false, false, false, false>> / <..., true>>)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_common import Workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=16)
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi, observer
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream

    W = H = a.size
    S = a.samples
    ctx = _ffi.Context(0)
    params = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.6, fov_y=0.6, sampling_seed=42.0, origin=(1e-4, 0.0, 30.0),
                     jitter=python_random_stream(42.0, 2 * S * W * H))
    fr.set_sky(synthetic_sky(2048, 1024))
    fr.set_redshift(("objects", "sky"))
    fr.generate_rays()
    tilt = np.radians(70.0)
    normal = np.array([0.0, -np.sin(tilt), np.cos(tilt)])     # the orbit plane of Workload.orbit_scene

    def scene(i, on):
        sph, rgb, lamps = Workload.orbit_scene(i)
        fr.set_objects(sph, rgb, lamps)
        if on:
            v, w = observer.circular_orbit_motion(np.array(sph[0][:3]), 1.0, normal=normal)
            fr.set_object_motion([v], [w])
        else:
            fr.set_object_motion(None)

    step = [0]

    def block(on, k, shade_only=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            if not shade_only:
                step[0] += 1
                scene(step[0], on)
                fr.trace(params)
            fr.shade()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    block(False, a.warmup)
    block(True, a.warmup)
    hits = int((fr.d_flags == 0x88).sum().item())
    frame_ms = {False: [], True: []}
    shade_ms = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            frame_ms[on].append(block(on, a.steps))
            shade_ms[on].append(block(on, max(a.steps, 20), shade_only=True))
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({
        "workload": f"{W}x{H} x{S} Schwarzschild orbiting-sphere animation frame (bench.py --workload orbit), redshift on objects "
                    f"and sky (g^4)",
        "device": ctx.name,
        "object_rays_last_frame": hits, "rays_per_frame": W * H * S,
        "frame_ms_off": med(frame_ms[False]), "frame_ms_on": med(frame_ms[True]),
        "frame_cost": med(frame_ms[True]) / med(frame_ms[False]) - 1.0,
        "shade_ms_off": med(shade_ms[False]), "shade_ms_on": med(shade_ms[True]),
        "samples_ms": {"frame_off": frame_ms[False], "frame_on": frame_ms[True], "shade_off": shade_ms[False],
                       "shade_on": shade_ms[True]},
        "what": f"trace + shade of one animation frame (frame_ms) and the shade call alone (shade_ms), the sphere at rest / "
                f"moving with circular_orbit_motion (locked), alternating blocks of {a.steps} steps after {a.warmup} warm-up "
                f"steps, medians of {a.reps}; host wall clock around synchronised blocks"}))
    ctx.close()


if __name__ == "__main__":
    main()

"""bench_object_textures.py -- what textured object spheres cost on the orbit workload (BASELINE.json configs[3]): a 2048 x 2048
x 16 frame of the orbiting-sphere animation (bench_common.Workload.orbit_scene: one lamp-lit sphere, a new position every step),
one DeviceFrame on one GPU, timed with object textures off and on in alternating blocks on the same frame.  On: the sphere wears a
procedurally generated 4096 x 2048 texture (uploaded once) and turns about its body z by a new angle every step (a kernel
argument, DeviceFrame.set_object_textures without a texture), lit by the workload's lamp.  Prints one JSON line.

    python scripts/bench_object_textures.py [--steps 10] [--warmup 3] [--reps 3]

frame_ms = set_objects + trace + shade_f32 per step; shade_ms = shade_f32 alone (the trace does not change with textures: only
the shade kernels take their textured instance).  Host wall clock around synchronised blocks; medians over --reps blocks of
each.  Run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_object_textures.py` for the shade kernels' own
times (shade_pixels_kernel<SceneColour<false, false, TEX = false / true, ...>>)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_common import CAM, Workload  # noqa: E402


def moon_texture(w, h):
    """A deterministic 'moon': smooth albedo variation plus craters, float32 RGBA [h, w, 4], rows bottom-up."""
    v, u = np.meshgrid(np.linspace(-1.0, 1.0, h, dtype=np.float32), np.linspace(-1.0, 1.0, w, dtype=np.float32), indexing="ij")
    a = 0.55 + 0.15 * np.sin(5.0 * np.pi * u) * np.cos(3.0 * np.pi * v) + 0.05 * np.cos(17.0 * np.pi * (u + v))
    rng = np.random.default_rng(7)
    for cu, cv, r in zip(rng.uniform(-1, 1, 40), rng.uniform(-0.9, 0.9, 40), rng.uniform(0.01, 0.08, 40)):
        d2 = ((u - cu) / 2.0) ** 2 + (v - cv) ** 2
        a -= (0.25 * np.exp(-d2 / (r * r))).astype(np.float32)
    tex = np.empty((h, w, 4), np.float32)
    tex[..., 0], tex[..., 1], tex[..., 2], tex[..., 3] = a, 0.97 * a, 0.92 * a, 1.0
    return np.clip(tex, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=16)
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream

    W = H = a.size
    S = a.samples
    ctx = _ffi.Context(0)
    wl = Workload(argparse.Namespace(regime="default", rhs="christoffel", workload="orbit"))
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=python_random_stream(42.0, 2 * S * W * H))
    fr.set_sky(synthetic_sky(2048, 1024))
    fr.set_objects(*wl.orbit_scene(0))
    fr.generate_rays()
    tex = moon_texture(4096, 2048)
    image = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
    tilt = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.4), -np.sin(0.4)], [0.0, np.sin(0.4), np.cos(0.4)]])

    def spin(i):
        c, s = np.cos(0.05 * i), np.sin(0.05 * i)
        return tilt @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])

    fr.set_object_textures([tex], [spin(0)], ["lit"], [0.0])        # the texture is uploaded once
    step = [0]

    def block(on, k, shade_only=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            i = step[0]
            step[0] += 1
            if on:
                fr.set_object_textures(rotations=[spin(i)], modes=["lit"], emission=[0.0])
            else:
                fr.object_textures, saved = None, fr.object_textures
            if not shade_only:
                fr.set_objects(*wl.orbit_scene(i))
                fr.trace(wl.params)
            fr.shade_f32(image)
            if not on:
                fr.object_textures = saved
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    block(False, a.warmup)
    block(True, a.warmup)
    frame_ms = {False: [], True: []}
    shade_ms = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            frame_ms[on].append(block(on, a.steps))
            shade_ms[on].append(block(on, max(a.steps, 20), shade_only=True))
    hits = int((fr.d_flags == 0x88).sum().item())
    med = lambda v: float(np.median(v))   # noqa: E731
    print(json.dumps({
        "workload": f"BASELINE.json configs[3]: {W}x{H} x{S} orbiting lamp-lit sphere (radius 1.5, r = 8), one DeviceFrame, one GPU; "
                    f"textured: a 4096x2048 float32 RGBA texture, lit, turned every step",
        "device": ctx.name,
        "frame_ms_off": med(frame_ms[False]), "frame_ms_on": med(frame_ms[True]),
        "frame_cost": med(frame_ms[True]) / med(frame_ms[False]) - 1.0,
        "shade_ms_off": med(shade_ms[False]), "shade_ms_on": med(shade_ms[True]),
        "object_rays_last_step": hits, "rays": W * H * S,
        "samples_ms": {"frame_off": frame_ms[False], "frame_on": frame_ms[True], "shade_off": shade_ms[False],
                       "shade_on": shade_ms[True]},
        "what": f"set_objects + trace + shade_f32 (frame_ms) and shade_f32 alone (shade_ms), object textures off / on, alternating "
                f"blocks of {a.steps} steps after {a.warmup} warm-up steps, medians of {a.reps}; host wall clock around "
                f"synchronised blocks"}))
    ctx.close()


if __name__ == "__main__":
    main()

"""bench_mesh_frame.py -- what the mesh material and a mesh on the library-owned frame cost, on section
19's cost scene: one 1024 x 1024 ray set (the camera at r = 30, 80 degrees from the axis, exit sphere at 40) and a sphere of
--tris triangles (an octahedron subdivided onto radius 2 at (-5, 3, 1), behind the hole).  Timed in alternating blocks:

    shade_plain     bhg_shade_mesh_device, tri_rgb only (shade_pixels_kernel<MeshColour, MeshShade>)
    shade_flat      bhg_shade_mesh_material_device, tri_rgb only (shade_pixels_kernel<MeshColour, MeshShade, MeshMaterialArgs> without a texel)
    shade_textured  bhg_shade_mesh_material_device with per-corner UVs and a 1024 x 512 image
    frame           a whole _ffi.Frame.render of the textured mesh on one device, the image left on the device

The shade lines are the device's own event times around the calls on the stream (torch.cuda.Event), the frame line the frame's
profiled trace (bhg_frame_last_ms) and the wall time of render + synchronize; medians over --reps blocks.  One JSON line.

    python scripts/bench_mesh_frame.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 4] [--chord 0.25]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_mesh import octa_sphere  # noqa: E402  (scripts/: this script's own directory)
from timed_region_stats import box_id  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--sub", type=int, default=4, help="subdivisions of the octahedron: 8 * 4^sub triangles")
    ap.add_argument("--chord", type=float, default=0.25)
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix

    ctx = _ffi.Context(0)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    V, F = octa_sphere((-5.0, 3.0, 1.0), 2.0, a.sub)
    rng = np.random.default_rng(1)
    rgb = rng.uniform(0.2, 1.0, (len(F), 3)).astype(np.float32)
    uv = rng.uniform(-1.5, 2.5, (len(F), 3, 2)).astype(np.float32)
    image = rng.random((512, 1024, 4)).astype(np.float32)
    lamps = [[10.0, 10.0, 10.0, 12.0]]
    sky = synthetic_sky(512, 256)
    materials = {"shade_plain": None, "shade_flat": _ffi.MeshMaterial(tri_rgb=rgb),
                 "shade_textured": _ffi.MeshMaterial(tri_rgb=rgb, tri_uv=uv, textures=[image])}
    mesh = _ffi.Mesh(ctx, V, F)
    frames = {}
    for line, mat in materials.items():
        f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                        start_cache=False)
        f.set_sky(sky)
        f.set_mesh(mesh, tri_rgb=rgb if mat is None else None, chord=a.chord, lamps=lamps, material=mat)
        f.generate_rays(p)
        f.trace(p)
        frames[line] = f

    def block(line, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            frames[line].shade()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    fr = _ffi.Frame([0], a.size, a.size, 1, fov_x=0.9, fov_y=0.9, origin=cam, rot=euler_xyz_matrix((0.0, inc, 0.0)))
    fr.set_scene(sky, lamps=lamps)
    fr.set_mesh(V, F, chord=a.chord, material=materials["shade_textured"])
    fr.set_profiling(True)

    def frame_block(k):
        fr.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fr.render(p, to_host=False)
        fr.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / k
        return wall, fr.last_ms()[0][0]

    ms = {line: [] for line in frames}
    wall, trace = [], []
    for line in frames:
        block(line, a.warmup)
    frame_block(a.warmup)
    for _ in range(a.reps):
        for line in frames:
            ms[line].append(block(line, a.steps))
        w, t = frame_block(a.steps)
        wall.append(w)
        trace.append(t)
    x = frames["shade_textured"]
    same = bool(torch.equal(frames["shade_plain"].shade().clone(), frames["shade_flat"].shade()))
    out = {"workload": f"{a.size}x{a.size} x1 Schwarzschild, camera r = 30 at 80 deg, exit sphere 40, {len(F)}-triangle sphere of radius 2 "
                       f"at (-5, 3, 1), max_chord {a.chord}, one lamp, 1024x512 texture",
           "device": ctx.name, "box": box_id(), "mesh_rays": int((x.d_tri_id >= 0).sum().item()), "rays": int(x.n),
           "flat_material_equals_plain": same}
    for line, v in ms.items():
        out[f"{line}_ms"] = float(np.median(v))
    out["frame_render_wall_ms"] = float(np.median(wall))
    out["frame_trace_ms"] = float(np.median(trace))
    print(json.dumps(out))
    fr.close()
    ctx.close()


if __name__ == "__main__":
    main()

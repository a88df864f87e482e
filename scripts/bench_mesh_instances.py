"""bench_mesh_instances.py -- what rigid placements of one mesh cost beside the mesh where it lies, on
scripts/bench_mesh.py's cost scene: one 1024 x 1024 ray set (the camera at r = 30, 80 degrees from the axis, exit sphere at 40)
and a sphere of --tris triangles of radius 2 behind the hole.  Three comparisons, each in alternating blocks:

    mesh / inst1          bhg_trace_mesh_device against bhg_trace_mesh_instances_device with ONE instance under the identity
                          (the same results bit for bit: the price of the instance loop itself), and the two shades
    flat8 / inst8         8 placements of a sphere of radius 0.8 on a ring behind the hole: flattened into one mesh of 8 times the
                          triangles in one tree, against 8 instances of the one tree
    set_mesh / set_inst   a moved mesh on the library-owned frame, one device: bhg_frame_set_mesh with the moved vertices + render
                          against bhg_frame_set_mesh_instances with the moved transform + render (host wall time: the first is
                          a validation, a tree build and an upload on the host)

Prints one JSON line.

    python scripts/bench_mesh_instances.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 4] [--chord 0.25] [--kerr]

The device figures are the device's own event times around each call on the stream (torch.cuda.Event), medians over --reps blocks."""
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


def rotation_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--sub", type=int, default=4, help="subdivisions of the octahedron: 8 * 4^sub triangles")
    ap.add_argument("--chord", type=float, default=0.25)
    ap.add_argument("--kerr", action="store_true", help="Kerr a/M = 0.9 instead of Schwarzschild")
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky

    ctx = _ffi.Context(0)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=_ffi.RHS_KERR_BL if a.kerr else _ffi.RHS_CHRISTOFFEL,
                         spin=0.45 if a.kerr else 0.0)
    lamps = [[10.0, 10.0, 10.0, 12.0]]
    V, F = octa_sphere((-5.0, 3.0, 1.0), 2.0, a.sub)
    identity = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None, :]
    # 8 placements of a small sphere on a ring of radius 6 about the hole, each turned about z
    Vs, Fs = octa_sphere((0.0, 0.0, 0.0), 0.8, a.sub)
    ring = []
    for j in range(8):
        phi = 2.0 * np.pi * (j + 0.5) / 8
        ring.append(np.concatenate([rotation_z(0.7 * j).reshape(9), [6.0 * np.cos(phi), 6.0 * np.sin(phi), 0.4 * (j % 3) - 0.4]]))
    ring = np.stack(ring)
    Vflat = np.concatenate([Vs @ r[:9].reshape(3, 3).T + r[9:] for r in ring])
    Fflat = np.concatenate([Fs + j * len(Vs) for j in range(8)]).astype(np.int32)

    def frame(mesh, instances=None):
        f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                        start_cache=False)
        f.set_sky(synthetic_sky(512, 256))
        f.set_mesh(mesh, chord=a.chord, lamps=lamps, instances=instances)
        f.generate_rays(p)
        return f

    big, small = _ffi.Mesh(ctx, V, F), _ffi.Mesh(ctx, Vs, Fs)
    frames = {"mesh": frame(big), "inst1": frame(big, identity), "flat8": frame(_ffi.Mesh(ctx, Vflat, Fflat)), "inst8": frame(small, ring)}

    def block(line, k, what):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            getattr(frames[line], what)(*((p,) if what == "trace" else ()))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    ms = {(line, what): [] for line in frames for what in ("trace", "shade")}
    for key in ms:
        block(key[0], a.warmup, key[1])
    for _ in range(a.reps):
        for key in ms:
            ms[key].append(block(key[0], a.steps, key[1]))
    x, y = frames["mesh"], frames["inst1"]
    same1 = bool(torch.equal(x.d_end, y.d_end) and torch.equal(x.d_flags, y.d_flags) and torch.equal(x.d_steps, y.d_steps)
                 and torch.equal(x.d_tri_id, y.d_tri_id))
    u, v = frames["flat8"], frames["inst8"]
    hit = v.d_inst_id >= 0
    same8 = bool(torch.equal(u.d_flags, v.d_flags) and torch.equal(u.d_steps, v.d_steps)
                 and torch.equal(u.d_tri_id[hit], (v.d_inst_id[hit] * len(Fs) + v.d_tri_id[hit])))
    out = {"workload": f"{a.size}x{a.size} x1 {'Kerr a/M=0.9' if a.kerr else 'Schwarzschild'}, camera r = 30 at 80 deg, exit sphere 40, "
                       f"{len(F)}-triangle sphere of radius 2 at (-5, 3, 1); 8 spheres of {len(Fs)} triangles on a ring of radius 6; "
                       f"max_chord {a.chord}",
           "device": ctx.name, "box": box_id(), "cull": os.environ.get("BHGEO_MESH_CULL", "") != "0", "rays": int(x.n),
           "mesh_rays": int((x.d_tri_id >= 0).sum().item()), "ring_rays": int(hit.sum().item()),
           "same_results_mesh_and_one_identity_instance": same1, "same_flags_steps_triangles_flat8_and_inst8": same8}
    for (line, what), t in ms.items():
        out[f"{line}_{what}_ms"] = float(np.median(t))
    out["trace_ratio_inst1_over_mesh"] = out["inst1_trace_ms"] / out["mesh_trace_ms"]
    out["shade_ratio_inst1_over_mesh"] = out["inst1_shade_ms"] / out["mesh_shade_ms"]
    out["trace_ratio_inst8_over_flat8"] = out["inst8_trace_ms"] / out["flat8_trace_ms"]
    out["shade_ratio_inst8_over_flat8"] = out["inst8_shade_ms"] / out["flat8_shade_ms"]

    # a moved mesh on the library-owned frame: set_mesh (validate, build, upload) + render against set_mesh_instances + render
    W = min(a.size, 256)
    rot = np.array([[np.cos(inc), 0.0, np.sin(inc)], [0.0, 1.0, 0.0], [-np.sin(inc), 0.0, np.cos(inc)]])
    centre = np.array([-5.0, 3.0, 1.0])
    V0 = V - centre
    libs = {}
    for name in ("set_mesh", "set_inst"):
        libs[name] = _ffi.Frame([0], W, W, 1, fov_x=0.9, fov_y=0.9, origin=cam, rot=rot, tile=32)
        libs[name].set_scene(synthetic_sky(512, 256), lamps=lamps)
    libs["set_inst"].set_mesh(V0, F, chord=a.chord)       # (the mesh about its own origin, put in place by the transform)
    wall = {"set_mesh": [], "set_inst": []}
    for k in range(a.steps * a.reps + a.warmup):
        d = np.array([0.05, -0.03, 0.02]) * (k + 1)
        t0 = time.perf_counter()
        libs["set_mesh"].set_mesh(V0 + centre + d, F, chord=a.chord)
        img_a = libs["set_mesh"].render(p)
        t1 = time.perf_counter()
        libs["set_inst"].set_mesh_instances(np.concatenate([np.eye(3).reshape(9), centre + d])[None, :])
        img_b = libs["set_inst"].render(p)
        t2 = time.perf_counter()
        if k >= a.warmup:
            wall["set_mesh"].append((t1 - t0) * 1e3)
            wall["set_inst"].append((t2 - t1) * 1e3)
    out["moved_frames_largest_difference"] = float(np.abs(img_a - img_b).max())
    out["moved_frame"] = f"{W}x{W} x1, one device, host wall time of set + render"
    out["set_mesh_render_ms"] = float(np.median(wall["set_mesh"]))
    out["set_instances_render_ms"] = float(np.median(wall["set_inst"]))
    out["moved_ratio_set_mesh_over_set_instances"] = out["set_mesh_render_ms"] / out["set_instances_render_ms"]
    print(json.dumps(out))
    for lib in libs.values():
        lib.close()
    ctx.close()


if __name__ == "__main__":
    main()

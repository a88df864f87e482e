"""bench_mesh.py -- what a triangle mesh in the curved region costs beside the plain trace: one 1024 x 1024
ray set (the camera at r = 30, 80 degrees from the axis, exit sphere at 40) and a sphere of --tris triangles (an octahedron
subdivided onto radius 2 at (-5, 3, 1), behind the hole), traced by

    plain       bhg_trace_device, no mesh (the persistent trace kernel, start-up records off)
    mesh        bhg_trace_mesh_device with the whole-step cull (trace_mesh_kernel: one lane per ray)
    mesh_brute  the same with the tree replaced by one leaf (leaf_size = n_triangles)

in alternating blocks, and the frame's shade with and without the mesh.  Prints one JSON line.

    python scripts/bench_mesh.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 4] [--chord 0.25] [--kerr]

BHGEO_MESH_CULL=0 in the environment times the mesh lines without the cull.  The lane-per-ray kernels leave no pass events behind,
so the figures are the device's own event times around each call on the stream (torch.cuda.Event), medians over --reps blocks."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from timed_region_stats import box_id  # noqa: E402  (scripts/: this script's own directory)


def octa_sphere(centre, radius, sub):
    v = [np.array(p, float) for p in [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(sub):
        nf, cache = [], {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, float), np.array(f, np.int32)


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
    V, F = octa_sphere((-5.0, 3.0, 1.0), 2.0, a.sub)
    frames = {}
    for line, leaf in (("plain", None), ("mesh", 4), ("mesh_brute", len(F))):
        f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                        start_cache=False)
        f.set_sky(synthetic_sky(512, 256))
        if leaf is not None:
            f.set_mesh(_ffi.Mesh(ctx, V, F, leaf_size=leaf), chord=a.chord, lamps=[[10.0, 10.0, 10.0, 12.0]])
        f.generate_rays(p)
        frames[line] = f

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
        block(*key[:1], a.warmup, key[1])
    for _ in range(a.reps):
        for key in ms:
            ms[key].append(block(key[0], a.steps, key[1]))
    x, y = frames["mesh"], frames["mesh_brute"]
    same = bool(torch.equal(x.d_end, y.d_end) and torch.equal(x.d_flags, y.d_flags) and torch.equal(x.d_steps, y.d_steps)
                and torch.equal(x.d_tri_id, y.d_tri_id))
    out = {"workload": f"{a.size}x{a.size} x1 {'Kerr a/M=0.9' if a.kerr else 'Schwarzschild'}, camera r = 30 at 80 deg, exit sphere 40, "
                       f"{len(F)}-triangle sphere of radius 2 at (-5, 3, 1), max_chord {a.chord}",
           "device": ctx.name, "box": box_id(), "cull": os.environ.get("BHGEO_MESH_CULL", "") != "0",
           "mesh_rays": int((x.d_tri_id >= 0).sum().item()), "rays": int(x.n), "tree_nodes": int(x.mesh.info()[0]),
           "same_results_tree_and_brute_force": same}
    for (line, what), v in ms.items():
        out[f"{line}_{what}_ms"] = float(np.median(v))
    out["trace_ratio_mesh_over_plain"] = out["mesh_trace_ms"] / out["plain_trace_ms"]
    out["trace_ratio_brute_over_tree"] = out["mesh_brute_trace_ms"] / out["mesh_trace_ms"]
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()

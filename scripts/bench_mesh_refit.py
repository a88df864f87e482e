"""bench_mesh_refit.py -- what a refit of a deformed mesh costs beside a rebuild, and what the refitted tree costs the trace
(DESIGN.md section 22), on scripts/bench_mesh.py's cost scene: one --size x --size ray set (the camera at r = 30, 80 degrees from
the axis, exit sphere at 40) and a sphere of triangles of radius 2 behind the hole.  Three measurements, each in alternating blocks:

    refit / create        bhg_mesh_refit (host arrays) and bhg_mesh_refit_device (device arrays) against bhg_mesh_create +
                          bhg_mesh_destroy on the same deformed vertices, for spheres of 8 * 4^4 = 2 048 and 8 * 4^7 = 131 072
                          triangles (host wall time of the whole call: all three are blocking)
    refitted / fresh      bhg_trace_mesh_device on the tree refitted to four deformations -- 1 % vertex noise, a 90 degree rigid
                          turn, a twist of pi over the mesh's height, vertex positions permuted at random -- against the same
                          trace on a tree built fresh for the same vertices, Schwarzschild and Kerr, with area_now / area_build
                          beside each line (device event times) and whether the two traces gave the same bits
    refit_mesh / set_mesh a 256 x 256 library-owned frame with a deforming mesh: refit_mesh + render against set_mesh + render
                          (host wall time), and the largest image difference, which must be 0

Prints one JSON line.

    python scripts/bench_mesh_refit.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 4] [--chord 0.25]"""
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

CENTRE = np.array([-5.0, 3.0, 1.0])


def deformations(V, rng):
    """name -> vertices: the four deformations of the table, about the mesh's own centre."""
    c = 0.5 * (V.min(0) + V.max(0))
    X = V - c
    size = float(np.ptp(V, axis=0).max())
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ang = np.pi * (X[:, 2] - X[:, 2].min()) / float(np.ptp(X[:, 2]))
    twist = np.stack([np.cos(ang) * X[:, 0] - np.sin(ang) * X[:, 1], np.sin(ang) * X[:, 0] + np.cos(ang) * X[:, 1], X[:, 2]], 1)
    return {"noise": V + rng.normal(size=V.shape) * 0.01 * size, "turn90": X @ turn.T + c, "twist": np.ascontiguousarray(twist + c),
            "permute": np.ascontiguousarray(V[rng.permutation(len(V))])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--sub", type=int, default=4, help="subdivisions of the traced sphere: 8 * 4^sub triangles")
    ap.add_argument("--chord", type=float, default=0.25)
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky

    ctx = _ffi.Context(0)
    rng = np.random.default_rng(5)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    out = {"device": ctx.name, "box": box_id(), "cull": os.environ.get("BHGEO_MESH_CULL", "") != "0"}

    # ---- 1. refit against create + destroy ----------------------------------------------------------------------------------
    for sub in (4, 7):
        V, F = octa_sphere(CENTRE, 2.0, sub)
        Vn = deformations(V, rng)["noise"]
        d_vn = torch.as_tensor(Vn).cuda()
        mesh = _ffi.Mesh(ctx, V, F)
        stream = torch.cuda.current_stream().cuda_stream

        def create():
            _ffi.Mesh(ctx, Vn, F).close()

        calls = {"create_destroy": create, "refit": lambda: mesh.refit(Vn), "refit_device": lambda: mesh.refit(d_vn, stream=stream)}
        wall = {k: [] for k in calls}
        for k, call in calls.items():
            for _ in range(a.warmup):
                call()
        for _ in range(a.reps):
            for k, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call()
                wall[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for k in calls:
            out[f"tris{len(F)}_{k}_ms"] = float(np.median(wall[k]))
        out[f"tris{len(F)}_nodes"] = mesh.info()[0]
        mesh.close()

    # ---- 2. the trace on the refitted tree against the trace on a fresh one ---------------------------------------------------
    V, F = octa_sphere(CENTRE, 2.0, a.sub)
    shapes = deformations(V, rng)
    out["workload"] = (f"{a.size}x{a.size} x1, camera r = 30 at 80 deg, exit sphere 40, {len(F)}-triangle sphere of radius 2 at (-5, 3, 1), "
                       f"max_chord {a.chord}")
    for kerr in (False, True):
        tag = "kerr" if kerr else "schw"
        p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=_ffi.RHS_KERR_BL if kerr else _ffi.RHS_CHRISTOFFEL,
                             spin=0.45 if kerr else 0.0)
        for name, Vd in shapes.items():
            refitted, fresh = _ffi.Mesh(ctx, V, F), _ffi.Mesh(ctx, Vd, F)
            refitted.refit(Vd)
            _, built, now = refitted.refit_info()
            frames = {}
            for key, mesh in (("refitted", refitted), ("fresh", fresh)):
                f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                                start_cache=False)
                f.set_sky(synthetic_sky(64, 32))
                f.set_mesh(mesh, chord=a.chord, lamps=[[10.0, 10.0, 10.0, 12.0]])
                f.generate_rays(p)
                frames[key] = f

            def block(key, k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(k):
                    frames[key].trace(p)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / k

            ms = {key: [] for key in frames}
            for key in frames:
                block(key, a.warmup)
            for _ in range(a.reps):
                for key in frames:
                    ms[key].append(block(key, a.steps))
            x, y = frames["refitted"], frames["fresh"]
            same = bool(torch.equal(x.d_end, y.d_end) and torch.equal(x.d_flags, y.d_flags) and torch.equal(x.d_steps, y.d_steps)
                        and torch.equal(x.d_tri_id, y.d_tri_id))
            out[f"{tag}_{name}"] = {"refitted_ms": float(np.median(ms["refitted"])), "fresh_ms": float(np.median(ms["fresh"])),
                                    "area_ratio": now / built, "mesh_rays": int((y.d_tri_id >= 0).sum().item()), "same_bits": same}
            refitted.close()
            fresh.close()

    # ---- 3. a deforming mesh on the library-owned frame -----------------------------------------------------------------------
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    rot = np.array([[np.cos(inc), 0.0, np.sin(inc)], [0.0, 1.0, 0.0], [-np.sin(inc), 0.0, np.cos(inc)]])
    libs = {}
    for name in ("set_mesh", "refit_mesh"):
        libs[name] = _ffi.Frame([0], 256, 256, 1, fov_x=0.9, fov_y=0.9, origin=cam, rot=rot, tile=32)
        libs[name].set_scene(synthetic_sky(64, 32), lamps=[[10.0, 10.0, 10.0, 12.0]])
        libs[name].set_mesh(V, F, chord=a.chord)
        libs[name].render(p)
    wall = {"set_mesh": [], "refit_mesh": []}
    worst = 0.0
    X = V - CENTRE
    for k in range(a.steps * a.reps + a.warmup):
        Vd = CENTRE + X * (1.0 + 0.1 * np.sin(3.0 * X[:, 2:3] + 0.4 * k))       # a wave that runs up the sphere
        t0 = time.perf_counter()
        libs["set_mesh"].set_mesh(Vd, F, chord=a.chord)
        img_a = libs["set_mesh"].render(p)
        t1 = time.perf_counter()
        libs["refit_mesh"].refit_mesh(Vd)
        img_b = libs["refit_mesh"].render(p)
        t2 = time.perf_counter()
        if k >= a.warmup:
            wall["set_mesh"].append((t1 - t0) * 1e3)
            wall["refit_mesh"].append((t2 - t1) * 1e3)
        worst = max(worst, float(np.abs(img_a - img_b).max()))
    out["frame256_set_mesh_render_ms"] = float(np.median(wall["set_mesh"]))
    out["frame256_refit_mesh_render_ms"] = float(np.median(wall["refit_mesh"]))
    out["frame256_largest_image_difference"] = worst
    out["frame256_refits"] = libs["refit_mesh"].mesh_refit_info(0)[0]
    for fr in libs.values():
        fr.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""bench_mesh_build.py -- what the device-side build of a mesh's tree costs beside the host build, and what its Morton-order tree
costs the trace, on scripts/bench_mesh.py's cost scene: one --size x --size ray set (the camera at r = 30,
80 degrees from the axis, exit sphere at 40) and a sphere of triangles of radius 2 behind the hole.  One session, alternating
blocks, medians:

    builds                bhg_mesh_create + bhg_mesh_destroy (the host build: the yardstick), bhg_mesh_create_device + destroy,
                          bhg_mesh_rebuild_device in place and bhg_mesh_rebuild from host arrays, for spheres of 8 * 4^4 = 2 048
                          and 8 * 4^7 = 131 072 triangles (host wall time of the whole call: all are blocking), and the area sum
                          of the Morton tree over the host tree's
    device / host tree    bhg_trace_mesh_device on the device-built tree against the same trace on the host-built tree,
                          Schwarzschild and Kerr a / M = 0.9 (device event times), and whether the two gave the same bits
    a changing topology   a 256 x 256 library-owned frame whose mesh is another triangle list every frame: set_mesh + render with
                          and without set_mesh_build(1) (host wall time), and the largest image difference, which must be 0

--only-rebuilds N runs nothing but N in-place rebuilds of the 131 072-triangle sphere: the command a kernel trace is taken of.
Prints one JSON line.

    python scripts/bench_mesh_build.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 7] [--chord 0.25]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--sub", type=int, default=7, help="subdivisions of the traced sphere: 8 * 4^sub triangles")
    ap.add_argument("--chord", type=float, default=0.25)
    ap.add_argument("--only-rebuilds", type=int, default=0)
    a = ap.parse_args()

    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky

    ctx = _ffi.Context(0)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    out = {"device": ctx.name, "box": box_id(), "cull": os.environ.get("BHGEO_MESH_CULL", "") != "0"}
    stream = torch.cuda.current_stream().cuda_stream

    if a.only_rebuilds:
        V, F = octa_sphere(CENTRE, 2.0, 7)
        d_v, d_f = torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda()
        mesh = _ffi.Mesh.from_device(ctx, d_v, d_f, stream=stream)
        for _ in range(a.only_rebuilds):
            mesh.rebuild(d_v, d_f, stream=stream)
        out["rebuilds"] = mesh.build_info()["builds"] - 1
        mesh.close()
        ctx.close()
        print(json.dumps(out))
        return

    # ---- 1. the builds ------------------------------------------------------------------------------------------------------
    for sub in (4, 7):
        V, F = octa_sphere(CENTRE, 2.0, sub)
        d_v, d_f = torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda()
        mesh = _ffi.Mesh.from_device(ctx, d_v, d_f, stream=stream)

        calls = {"create_destroy": lambda: _ffi.Mesh(ctx, V, F).close(),
                 "create_device_destroy": lambda: _ffi.Mesh.from_device(ctx, d_v, d_f, stream=stream).close(),
                 "rebuild_device": lambda: mesh.rebuild(d_v, d_f, stream=stream),
                 "rebuild_host_arrays": lambda: mesh.rebuild(V, F)}
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
        host = _ffi.Mesh(ctx, V, F)
        out[f"tris{len(F)}_area_morton_over_host"] = mesh.refit_info()[1] / host.refit_info()[1]
        host.close()
        mesh.close()

    # ---- 2. the trace on the device-built tree against the trace on the host-built one ----------------------------------------
    V, F = octa_sphere(CENTRE, 2.0, a.sub)
    out["workload"] = (f"{a.size}x{a.size} x1, camera r = 30 at 80 deg, exit sphere 40, {len(F)}-triangle sphere of radius 2 at (-5, 3, 1), "
                       f"max_chord {a.chord}")
    for kerr in (False, True):
        tag = "kerr" if kerr else "schw"
        p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=_ffi.RHS_KERR_BL if kerr else _ffi.RHS_CHRISTOFFEL,
                             spin=0.45 if kerr else 0.0)
        meshes = {"host": _ffi.Mesh(ctx, V, F), "device": _ffi.Mesh(ctx, V, F, build="device")}
        frames = {}
        for key, mesh in meshes.items():
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
        x, y = frames["device"], frames["host"]
        same = bool(torch.equal(x.d_end, y.d_end) and torch.equal(x.d_flags, y.d_flags) and torch.equal(x.d_steps, y.d_steps)
                    and torch.equal(x.d_tri_id, y.d_tri_id))
        out[f"{tag}_trace"] = {"device_tree_ms": float(np.median(ms["device"])), "host_tree_ms": float(np.median(ms["host"])),
                               "mesh_rays": int((y.d_tri_id >= 0).sum().item()), "same_bits": same}
        for mesh in meshes.values():
            mesh.close()

    # ---- 3. a mesh whose triangle list changes every frame, on the library-owned frame -----------------------------------------
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    rot = np.array([[np.cos(inc), 0.0, np.sin(inc)], [0.0, 1.0, 0.0], [-np.sin(inc), 0.0, np.cos(inc)]])
    libs = {}
    for name in ("host_build", "device_build"):
        libs[name] = _ffi.Frame([0], 256, 256, 1, fov_x=0.9, fov_y=0.9, origin=cam, rot=rot, tile=32)
        libs[name].set_scene(synthetic_sky(64, 32), lamps=[[10.0, 10.0, 10.0, 12.0]])
        libs[name].set_mesh_build(name == "device_build")
        libs[name].set_mesh(V, F, chord=a.chord)
        libs[name].render(p)
    wall = {name: [] for name in libs}
    worst = 0.0
    rng = np.random.default_rng(5)
    for k in range(a.steps * a.reps + a.warmup):
        Fk = np.ascontiguousarray(F[rng.permutation(len(F))[:len(F) - 1 - k]])        # another list, one triangle fewer, every frame
        imgs = {}
        for name, fr in libs.items():
            t0 = time.perf_counter()
            fr.set_mesh(V, Fk, chord=a.chord)
            imgs[name] = fr.render(p)
            if k >= a.warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
        worst = max(worst, float(np.abs(imgs["host_build"] - imgs["device_build"]).max()))
    for name in libs:
        out[f"frame256_{name}_set_mesh_render_ms"] = float(np.median(wall[name]))
    out["frame256_largest_image_difference"] = worst
    out["frame256_device_builds"] = libs["device_build"].mesh_build_info(0)["builds"]
    for fr in libs.values():
        fr.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

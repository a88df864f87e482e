"""bench_mesh_instance_tree.py -- what a tree over the placements of an instance set costs and buys, on
scripts/bench_mesh_instances.py's cost scene: one --size x --size ray set (the camera at r = 30, 80 degrees from the axis, exit
sphere at 40).  Medians of --reps alternating blocks of --steps calls, the device's own event times.  The lines:

    ring8     section 21's eight spheres on a ring: the linear set, tree sets with leaves of 1, 2 and 4, and the flattened tree
    ring64    64 placements of the 8 * 4^sub-triangle sphere (radius 0.5) on a tilted ring of radius 9: tree against linear
    k1024     1024 spheres of 32 triangles (radius 0.12) on four tilted rings: the tree set, the same set walked linearly
              (BHGEO_INSTANCE_TREE=0, read at every call; one call per block) and the flattened tree of 32768 triangles
    set       the host's wall time of MeshInstances.set at K in {64, 1024, 16384}, linear and under a tree (the stream drained
              outside the timed region)

Every line is traced and shaded.  Prints one JSON line.

    python scripts/bench_mesh_instance_tree.py [--steps 5] [--warmup 2] [--reps 3] [--size 1024] [--sub 4] [--chord 0.25]"""
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
from bench_mesh_instances import rotation_z  # noqa: E402
from timed_region_stats import box_id  # noqa: E402


def rotation_x(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def rings(spec, per_ring):
    """per_ring placements on each ring (radius, tilt about x, phase), each turned about z its own way."""
    T = []
    for radius, tilt, phase in spec:
        for j in range(per_ring):
            phi = 2.0 * np.pi * j / per_ring + phase
            c = rotation_x(tilt) @ np.array([radius * np.cos(phi), radius * np.sin(phi), 0.0])
            T.append(np.concatenate([rotation_z(0.7 * j).reshape(9), c]))
    return np.stack(T)


def flatten(V, F, T):
    return (np.concatenate([V @ r[:9].reshape(3, 3).T + r[9:] for r in T]),
            np.concatenate([F + j * len(V) for j in range(len(T))]).astype(np.int32))


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

    ctx = _ffi.Context(0)
    inc = np.radians(80.0)
    cam = np.array([30.0 * np.sin(inc), 0.0, 30.0 * np.cos(inc)])
    p = _ffi.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    lamps = [[10.0, 10.0, 10.0, 12.0]]
    # section 21's eight spheres
    Vs, Fs = octa_sphere((0.0, 0.0, 0.0), 0.8, a.sub)
    ring8 = []
    for j in range(8):
        phi = 2.0 * np.pi * (j + 0.5) / 8
        ring8.append(np.concatenate([rotation_z(0.7 * j).reshape(9), [6.0 * np.cos(phi), 6.0 * np.sin(phi), 0.4 * (j % 3) - 0.4]]))
    ring8 = np.stack(ring8)
    Vm, Fm = octa_sphere((0.0, 0.0, 0.0), 0.5, a.sub)
    ring64 = rings(((9.0, 0.35, 0.0),), 64)
    Vt, Ft = octa_sphere((0.0, 0.0, 0.0), 0.12, 1)
    k1024 = rings(((6.0, 0.35, 0.0), (8.0, -0.5, 0.4), (10.0, 0.9, 1.1), (12.0, -0.2, 2.0)), 256)

    def frame(mesh, instances=None, tree=False, leaf=2):
        f = DeviceFrame(ctx, a.size, a.size, 1, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=cam, rotation_euler=(0.0, inc, 0.0),
                        start_cache=False)
        f.set_sky(synthetic_sky(512, 256))
        f.set_mesh(mesh, chord=a.chord, lamps=lamps, instances=instances, instance_tree=tree, instance_leaf_size=leaf)
        f.generate_rays(p)
        return f

    small, mid, tiny = _ffi.Mesh(ctx, Vs, Fs), _ffi.Mesh(ctx, Vm, Fm), _ffi.Mesh(ctx, Vt, Ft)
    frames = {"ring8_linear": frame(small, ring8), "ring8_flat": frame(_ffi.Mesh(ctx, *flatten(Vs, Fs, ring8))),
              "ring64_linear": frame(mid, ring64), "k1024_flat": frame(_ffi.Mesh(ctx, *flatten(Vt, Ft, k1024)))}
    for leaf in (1, 2, 4):
        frames[f"ring8_tree{leaf}"] = frame(small, ring8, True, leaf)
        frames[f"ring64_tree{leaf}"] = frame(mid, ring64, True, leaf)
        frames[f"k1024_tree{leaf}"] = frame(tiny, k1024, True, leaf)
    frames["k1024_tree2_walked_linearly"] = frames["k1024_tree2"]

    def block(line, k, what):
        linear = line.endswith("walked_linearly")
        if linear:
            os.environ["BHGEO_INSTANCE_TREE"] = "0"
            k = 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            getattr(frames[line], what)(*((p,) if what == "trace" else ()))
        e1.record()
        torch.cuda.synchronize()
        if linear:
            del os.environ["BHGEO_INSTANCE_TREE"]
        return e0.elapsed_time(e1) / k

    ms = {(line, what): [] for line in frames for what in ("trace", "shade")}
    for key in ms:
        block(key[0], a.warmup, key[1])
    for _ in range(a.reps):
        for key in ms:
            ms[key].append(block(key[0], a.steps, key[1]))

    def same(u, v, nt):
        hit = v.d_inst_id >= 0
        return bool(torch.equal(u.d_flags, v.d_flags) and torch.equal(u.d_steps, v.d_steps)
                    and torch.equal(u.d_tri_id[hit], (v.d_inst_id[hit] * nt + v.d_tri_id[hit])))

    def same_bits(u, v):
        return all(bool(torch.equal(getattr(u, k), getattr(v, k))) for k in ("d_end", "d_flags", "d_steps", "d_tri_id", "d_inst_id"))

    out = {"workload": f"{a.size}x{a.size} x1 Schwarzschild, camera r = 30 at 80 deg, exit sphere 40, max_chord {a.chord}; ring8: 8 spheres "
                       f"of {len(Fs)} triangles on a ring of radius 6; ring64: 64 of {len(Fm)} on a ring of radius 9; k1024: 1024 of "
                       f"{len(Ft)} on four rings of radius 6 to 12",
           "device": ctx.name, "box": box_id(), "cull": os.environ.get("BHGEO_MESH_CULL", "") != "0", "rays": int(frames["ring8_linear"].n),
           "ring8_rays": int((frames["ring8_linear"].d_inst_id >= 0).sum().item()),
           "ring64_rays": int((frames["ring64_linear"].d_inst_id >= 0).sum().item()),
           "k1024_rays": int((frames["k1024_tree2"].d_inst_id >= 0).sum().item()),
           "same_bits_ring8_tree_and_linear": all(same_bits(frames["ring8_linear"], frames[f"ring8_tree{leaf}"]) for leaf in (1, 2, 4)),
           "same_bits_ring64_tree_and_linear": all(same_bits(frames["ring64_linear"], frames[f"ring64_tree{leaf}"]) for leaf in (1, 2, 4)),
           "same_flags_steps_triangles_k1024_flat_and_tree": same(frames["k1024_flat"], frames["k1024_tree2"], len(Ft))}
    for (line, what), t in ms.items():
        out[f"{line}_{what}_ms"] = float(np.median(t))
        out[f"{line}_{what}_samples_ms"] = [float(x) for x in t]

    # the host's cost of a move
    rng = np.random.default_rng(3)
    for K in (64, 1024, 16384):
        base = rings(((8.0, 0.3, 0.0),), K)
        for kind in ("linear", "tree") if K <= 64 else ("tree",):
            inst = _ffi.MeshInstances(tiny, base, tree=kind == "tree")
            wall = []
            for k in range(a.steps * a.reps + a.warmup):
                T = base.copy()
                T[:, 9:] += rng.normal(size=(K, 3)) * 0.3
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inst.set(T)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
            torch.cuda.synchronize()
            out[f"set_{kind}_K{K}_host_ms"] = float(np.median(wall))
            inst.close()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()

"""Mesh instances: the cases tests/test_mesh_instances_host.py conditions on the CPU and
tests/test_gpu_mesh_instances.py runs on the device, the flattening that turns K placements of one mesh into the one mesh the
brute-force oracle (oracle.trace_mesh) knows, the oracle's two kinds of stability, and the device call.  Not a test module.

    python tests/mesh_instance_cases.py OUT.npz      # every case of cull_cases() through the device call, arrays into OUT.npz
                                                     # (tests/test_gpu_mesh_instances.py runs this with BHGEO_MESH_CULL=0)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_oracle_cases as mo  # noqa: E402
import mesh_reference as mr  # noqa: E402

SENTINEL = -7.25
KEYS = ("end", "flags", "n_steps", "n_accepted", "tri", "inst", "bary")
FORMS = {"christoffel": (0, 0.0), "reduced": (1, 0.0), "kerr_plus": (2, 0.45), "kerr_minus": (2, -0.45)}
PLACES = ((-3.0, 1.0, 0.3), (3.0, 3.5, 1.0), (1.0, -2.5, 1.5))
MIN_HITS_PER_INSTANCE = 25
VERTEX_DRAWS = 3


# ---- rigid records -----------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' rotation about `axis` by `angle`, orthonormal to rounding."""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def record(R, t):
    return np.concatenate([np.asarray(R, float).reshape(9), np.asarray(t, float)])


IDENTITY = record(np.eye(3), (0.0, 0.0, 0.0))[None, :]


def flatten(V, F, T):
    """K placements of (V, F) as one mesh: vertices V @ R_j.T + t_j, flattened triangle j * nt + T is (instance j, triangle T)."""
    T = np.asarray(T, float).reshape(-1, 12)
    Vs = [V @ rec[:9].reshape(3, 3).T + rec[9:] for rec in T]
    Fs = [F + j * len(V) for j in range(len(T))]
    return np.ascontiguousarray(np.concatenate(Vs)), np.ascontiguousarray(np.concatenate(Fs), dtype=np.int32)


# ---- the meshes and the cases ------------------------------------------------------------------------------------------------
def ellipsoid():
    """128 triangles, semi-axes (1, 0.6, 0.4), centred on its own origin."""
    V, F = mr.octa_sphere((0.0, 0.0, 0.0), 1.0, 2)
    return V * np.array([1.0, 0.6, 0.4]), F


def three_placements():
    rots = (rotation((1.0, 2.0, 0.5), 0.7), rotation((0.0, 1.0, -1.0), 2.1), rotation((-1.0, 0.3, 2.0), -1.3))
    return np.stack([record(R, t) for R, t in zip(rots, PLACES)])


def three_rays(n=2048, seed=17):
    """From mesh_oracle_cases.FRAME_CAM: a quarter of the rays towards each of the two placements in plain view, an eighth towards
    the one behind the hole, and the rest past the hole at impact parameters from 2.4 to 7, where that one's images lie."""
    rng = np.random.default_rng(seed)
    share = (n // 8, n // 4, n // 4)
    parts = [mr.camera_rays(mo.FRAME_CAM, c, m, rng, 1.6) for c, m in zip(PLACES, share)]
    parts.append(mr.hole_rays(mo.FRAME_CAM, n - sum(share), rng, 2.4, 7.0))
    return np.concatenate(parts)


def instance_case(rhs, spin, par, mesh, T, chord, k0, x0):
    """A case of mesh_oracle_cases on the flattened mesh, plus the local mesh and the records."""
    V, F = mesh
    c = mo._case(rhs, spin, par, flatten(V, F, T), chord, k0, x0)
    c.update(Vl=np.ascontiguousarray(V, dtype=np.float64), Fl=np.ascontiguousarray(F, dtype=np.int32), T=np.ascontiguousarray(T, dtype=np.float64))
    return c


def three_placement_cases():
    par = dict(r_s=1.0, lambda_end=64.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    return {name: instance_case(rhs, a, par, ellipsoid(), three_placements(), 0.25, three_rays(), mo.FRAME_CAM)
            for name, (rhs, a) in FORMS.items()}


RING_K = 64


def ring_case():
    """64 small tetrahedra on a tilted ring of radius 9 about the hole, each turned its own way.  16 rays go to each from a
    camera above the ring, aimed along the ring's radius through it from 0.3 inside to 2 outside: the hole bends them inwards."""
    rng = np.random.default_rng(41)
    tilt = rotation((1.0, 0.0, 0.0), 0.35)
    cam = np.array([2.0, -3.0, 24.0])
    T, k0 = [], []
    for j in range(RING_K):
        phi = 2.0 * np.pi * j / RING_K
        c = tilt @ np.array([9.0 * np.cos(phi), 9.0 * np.sin(phi), 0.0])
        T.append(record(rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)), c))
        aim = c[None, :] * (1.0 + np.linspace(-0.3, 2.0, 16) / 9.0)[:, None] - cam[None, :]
        k0.append(aim / np.linalg.norm(aim, axis=1)[:, None])
    return instance_case(0, 0.0, dict(r_s=1.0, lambda_end=60.0, r_exit=40.0), mr.tetrahedron((0.0, 0.0, 0.0), 0.5), np.stack(T), 0.25,
                         np.concatenate(k0), cam)


def bulge_case():
    """mesh_oracle_cases' bulge_into_the_box, its small sphere built about its own origin and put in place by a transform."""
    base = mo.parameter_cases()["bulge_into_the_box"]
    T = record(rotation((0.3, -1.0, 0.8), 1.1), (-1.0, 3.0, 0.0))[None, :]
    return instance_case(base["rhs"], base["spin"], base["par"], mr.octa_sphere((0.0, 0.0, 0.0), 0.3, 1), T, base["chord"], base["k0"], base["x0"])


# ---- the oracle: stable in both senses ---------------------------------------------------------------------------------------
def vertex_draws(V, seed=5):
    """Three draws that scale each flattened vertex coordinate by 1 +- 1 ... 2e-16: the rounding that separates arithmetic in an
    instance's frame from arithmetic on world vertices."""
    rng = np.random.default_rng(seed)
    return [V * (1.0 + rng.choice([-1.0, 1.0], size=V.shape) * rng.uniform(1e-16, 2e-16, size=V.shape)) for _ in range(VERTEX_DRAWS)]


def oracle_solve(oracle, case):
    """mesh_oracle_cases.oracle_solve on the flattened mesh, plus the vertex draws: stable_v [n] (flag, triangle, step counts and M
    unchanged under them), sens_v [n] (the end record's largest movement), near_v [n] (the set of (flag, tri, attempted, accepted)
    the draws give).  stable and sens become those of both kinds together; stable_k, sens_k keep the k0 kind."""
    o = mo.oracle_solve(oracle, case)
    n = len(case["k0"])
    o["stable_k"], o["sens_k"] = o["stable"].copy(), o["sens"].copy()
    o["stable_v"], o["sens_v"] = np.ones(n, bool), np.zeros(n)
    o["near_v"] = [set() for _ in range(n)]
    for Vp in vertex_draws(case["V"]):
        q = oracle.trace_mesh(case["k0"], case["x0"], Vp, case["F"], case["chord"], rhs_form=case["rhs"], spin=case["spin"], **case["par"])
        for key in ("flags", "tri", "n_attempted", "n_accepted", "M"):
            o["stable_v"] &= q[key] == o[key]
        with np.errstate(invalid="ignore"):
            o["sens_v"] = np.fmax(o["sens_v"], np.abs(q["end"] - o["end"]).max(1))
        for i in range(n):
            o["near_v"][i].add((int(q["flags"][i]), int(q["tri"][i]), int(q["n_attempted"][i]), int(q["n_accepted"][i])))
    o["stable"] = o["stable_k"] & o["stable_v"]
    o["sens"] = np.fmax(o["sens_k"], o["sens_v"])
    return o


def hits_per_instance(o, case):
    nt = len(case["Fl"])
    hit = o["tri"] >= 0
    return np.bincount(o["tri"][hit] // nt, minlength=len(case["T"]))


# ---- the device --------------------------------------------------------------------------------------------------------------
def trace_instances_device(ctx, p, inst, chord, k0, x0):
    """bhg_trace_mesh_instances_device on sentinel-filled arrays -> dict(end, flags, n_steps, n_accepted, tri, inst, bary)."""
    import torch
    n = len(k0)
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0, dtype=np.float64)).cuda()
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0, dtype=np.float64)).cuda()
    d_end = torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_fl = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_ac = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_tri = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_inst = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_bary = torch.full((n, 2), SENTINEL, dtype=torch.float64, device="cuda")
    try:
        ctx.trace_mesh_instances_device(p, inst, chord, n, d_k0.data_ptr(), d_end.data_ptr(), d_tri.data_ptr(), d_inst.data_ptr(),
                                        d_bary.data_ptr(), x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(),
                                        d_flags=d_fl.data_ptr(), d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(),
                                        stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return dict(end=d_end.cpu().numpy(), flags=d_fl.cpu().numpy(), n_steps=d_st.cpu().numpy().astype(np.uint32),
                n_accepted=d_ac.cpu().numpy().astype(np.uint32), tri=d_tri.cpu().numpy(), inst=d_inst.cpu().numpy(),
                bary=d_bary.cpu().numpy())


def run_case(ctx, case, T=None, leaf=4):
    """The case's local mesh under the records T (the case's own by default) through the device call."""
    from blackhole_geodesic_calculator_amd import _ffi
    mesh = _ffi.Mesh(ctx, case["Vl"], case["Fl"], leaf_size=leaf)
    try:
        inst = _ffi.MeshInstances(mesh, case["T"] if T is None else T)
        return trace_instances_device(ctx, _ffi.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"]), inst, case["chord"],
                                      case["k0"], case["x0"])
    finally:
        mesh.close()


def cull_cases():
    """The cases that must give the same bits with the culls on and off: the three placements in a Schwarzschild form and in
    Kerr, and the bulge."""
    three = three_placement_cases()
    return {"three_christoffel": three["christoffel"], "three_kerr_plus": three["kerr_plus"], "bulge": bulge_case()}


def run_cull_cases(ctx):
    res = {}
    for name, case in cull_cases().items():
        for key, arr in run_case(ctx, case).items():
            res[f"{name}__{key}"] = arr
    return res


if __name__ == "__main__":
    from blackhole_geodesic_calculator_amd import _ffi
    c = _ffi.Context(0)
    np.savez(sys.argv[1], **run_cull_cases(c))
    c.close()

"""The mesh-trace cases that tests/test_gpu_mesh.py runs twice -- in the test process with the whole-step cull, and through
this file as a fresh child process with BHGEO_MESH_CULL=0 -- and the device call they share.  Not a test module.

    python tests/mesh_cases.py OUT.npz      # every case of cull_cases() through bhg_trace_mesh_device, arrays into OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_reference as mr  # noqa: E402

SENTINEL = -7.25


def trace_mesh_device(ctx, p, mesh, chord, k0, x0):
    """bhg_trace_mesh_device on sentinel-filled arrays -> dict(end, flags, n_steps, n_accepted, tri, bary)."""
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
    d_bary = torch.full((n, 2), SENTINEL, dtype=torch.float64, device="cuda")
    try:
        ctx.trace_mesh_device(p, mesh, chord, n, d_k0.data_ptr(), d_end.data_ptr(), d_tri.data_ptr(), d_bary.data_ptr(),
                              x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(), d_flags=d_fl.data_ptr(),
                              d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return dict(end=d_end.cpu().numpy(), flags=d_fl.cpu().numpy(), n_steps=d_st.cpu().numpy().astype(np.uint32),
                n_accepted=d_ac.cpu().numpy().astype(np.uint32), tri=d_tri.cpu().numpy(), bary=d_bary.cpu().numpy())


def frame_rays_at(cam, target, n, seed, spread):
    return mr.camera_rays(cam, target, n, np.random.default_rng(seed), spread)


def cull_cases():
    """name -> (rhs_form, spin, params keywords, (V, F), chord, k0, x0): the golden rays of every form and mesh, and 4 096 frame
    rays on the 512-triangle sphere with a disk."""
    from conftest import load_golden
    g = load_golden("mesh")
    meshes = mr.golden_meshes()
    out = {}
    for fi, (rhs, a) in enumerate(mr.GOLDEN_FORMS):
        for name in meshes:
            par = dict(r_exit=0.0 if rhs == 2 else float(g["r_exit"]), **mr.GOLDEN_PAR)
            out[f"golden_{mr.GOLDEN_FORM_IDS[fi]}_{name}"] = (rhs, a, par, meshes[name], float(g["max_chord"]), g[f"{name}_k0"], g["x0"])
    cam = np.array([18.0, 2.0, 4.0])
    k = np.concatenate([frame_rays_at(cam, (-3.0, 1.0, 0.5), 2048, 3, 4.0), mr.hole_rays(cam, 2048, np.random.default_rng(4))])
    for rhs, a, tag in ((0, 0.0, "christoffel"), (2, 0.3, "kerr")):
        out[f"frame4096_{tag}"] = (rhs, a, dict(r_s=1.0, lambda_end=70.0, r_exit=0.0 if rhs == 2 else 40.0, disk_r_in=2.0, disk_r_out=6.0),
                                   mr.octa_sphere((-3.0, 1.0, 0.5), 1.2, 3), 0.2, k, cam)
    return out


def run_cases(ctx, cases=None):
    from blackhole_geodesic_calculator_amd import _ffi
    res = {}
    for name, (rhs, a, par, (V, F), chord, k0, x0) in (cases or cull_cases()).items():
        mesh = _ffi.Mesh(ctx, V, F)
        r = trace_mesh_device(ctx, _ffi.make_params(rhs_form=rhs, spin=a, **par), mesh, chord, k0, x0)
        mesh.close()
        for key, arr in r.items():
            res[f"{name}__{key}"] = arr
    return res


if __name__ == "__main__":
    from blackhole_geodesic_calculator_amd import _ffi
    c = _ffi.Context(0)
    np.savez(sys.argv[1], **run_cases(c))
    c.close()

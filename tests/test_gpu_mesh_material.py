"""The mesh material shade on the GPU (bhg_shade_mesh_material_device): against the numpy restatement on the
device's own records, its equivalences with bhg_shade_mesh_device, and every refusal with nothing written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_material_cases as mmc  # noqa: E402
import mesh_material_reference as mmr  # noqa: E402
import mesh_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


def _params(f):
    return f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=mmc.SHADE_DISK[0], disk_r_out=mmc.SHADE_DISK[1])


def _render(fr, p):
    import torch
    got = fr.render(p).cpu().numpy().copy()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "vertex_normals"])
def test_shade_against_the_restatement(ctx, S, smooth):
    import torch
    f = _ffi()
    V, F = mmc.SHADE_MESH
    normals = mmc.vertex_normals() if smooth else None
    M = mmc.material_arrays()
    mesh = f.Mesh(ctx, V, F, vertex_normals=normals)
    p = _params(f)
    fr = mmc.device_frame(ctx, S)
    fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**M))
    got = _render(fr, p)
    out32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out32)
    torch.cuda.synchronize()
    end, flags, tri, bary = (t.cpu().numpy() for t in (fr.d_end, fr.d_flags, fr.d_tri_id, fr.d_bary))
    on_mesh = (flags == 0x88) & (tri >= 0)
    assert on_mesh.sum() > 60 * S and len({*tri[on_mesh]}) > 10
    assert (tri[on_mesh] >= len(F) - 4).any() and (tri[on_mesh] < len(F) - 4).any()      # both components are seen
    # the test's own coverage: every image slot and "no slot" are hit, and UVs leave [0, 1) on both sides
    slots = M["tri_tex"][tri[on_mesh]]
    U, Vv = mmr.hit_uv(tri[on_mesh], bary[on_mesh], M["tri_uv"])
    textured = slots >= 0
    print(f"S {S}: {int(on_mesh.sum())} mesh rays, per slot {[int((slots == j).sum()) for j in (-1, 0, 1, 2)]}, "
          f"U in [{U[textured].min():.2f}, {U[textured].max():.2f}], V in [{Vv[textured].min():.2f}, {Vv[textured].max():.2f}]")
    for j in (-1, 0, 1, 2):
        assert (slots == j).any(), j
    assert ((U[textured] < 0.0) | (Vv[textured] < 0.0)).any() and ((U[textured] >= 1.0) | (Vv[textured] >= 1.0)).any()
    # the restatement: the mesh colour in numpy on the device's own records; every other ray's colour is the plain shade's (one
    # sample per "pixel", so that each ray's colour comes back by itself), summed per pixel in sample order
    per_ray = torch.empty((fr.n, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.n, 1, fr.scene(), per_ray.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    col = per_ray.cpu().numpy()[:, :3].copy()
    margins = []
    tree = f.mesh_bvh_host(V, F, 4)
    col[on_mesh] = mmr.material_colour(end[on_mesh], tri[on_mesh], bary[on_mesh], V, F, mmc.SHADE_LAMPS, normals, tree=tree,
                                       margins=margins, **M)
    want = np.zeros((fr.P, 3))
    for s in range(S):
        want += col[s * fr.P:(s + 1) * fr.P]
    want /= S
    # a shadow decision within 1e-9 of an edge exempts its ray: the lamps are chosen so that there is none
    near = int((np.array(margins) < 1e-9).sum())
    assert near == 0 and near <= 0.005 * on_mesh.sum()
    err = np.abs(got[:, :3] - want)
    print(f"worst |gpu - numpy| {err.max():.3e}")
    assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(want))) and np.all(got[:, 3] == 1.0)
    assert np.array_equal(out32.cpu().numpy(), got.astype(np.float32))
    # a comparison that fails with the wrap removed: the same material with its UVs clamped is another image
    Mc = dict(M, tri_uv=np.clip(M["tri_uv"], 0.0, 1.0))
    fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**Mc))
    clamped = _render(fr, p)
    pix_mesh = on_mesh.reshape(S, fr.P).any(0)
    assert np.abs(clamped[pix_mesh] - got[pix_mesh]).max() > 1e-3 and np.array_equal(clamped[~pix_mesh], got[~pix_mesh])
    # pixels without a mesh ray are bhg_shade_scene_device's bits on the same records
    same_records = torch.empty((fr.P, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, S, fr.scene(), same_records.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_records = same_records.cpu().numpy()
    assert pix_mesh.sum() > 30 and (~pix_mesh).sum() > 500
    assert np.array_equal(got[~pix_mesh], same_records[~pix_mesh]) and not np.array_equal(got[pix_mesh], same_records[pix_mesh])
    mesh.close()


def test_equivalences(ctx):
    f = _ffi()
    V, F = mmc.SHADE_MESH
    M = mmc.material_arrays()
    rgb = M["tri_rgb"]
    mesh = f.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals())
    p = _params(f)
    for S in (1, 5):
        fr = mmc.device_frame(ctx, S)
        fr.set_mesh(mesh, tri_rgb=rgb, chord=mmc.CHORD)
        old = _render(fr, p)
        # no UVs, no emission: the existing shade's image
        fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(tri_rgb=rgb))
        assert np.array_equal(_render(fr, p), old)
        # every triangle without a slot: the same
        fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(tri_rgb=rgb, tri_uv=M["tri_uv"], tri_tex=np.full(len(F), -1),
                                                                   textures=M["textures"]))
        assert np.array_equal(_render(fr, p), old)
        # ... and a textured one is not
        fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(tri_rgb=rgb, tri_uv=M["tri_uv"], textures=M["textures"]))
        assert not np.array_equal(_render(fr, p), old)
    # emission alone: no lamps, no texture -> tri_rgb * e on every mesh pixel of an S = 1 frame, exactly
    fr = mmc.device_frame(ctx, 1)
    fr.set_objects([], lamps=[])
    fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(tri_rgb=rgb, emission=0.75))
    got = _render(fr, p)
    flags, tri = fr.d_flags.cpu().numpy(), fr.d_tri_id.cpu().numpy()
    on_mesh = (flags == 0x88) & (tri >= 0)
    assert on_mesh.sum() > 60
    assert np.array_equal(got[on_mesh, :3], rgb[tri[on_mesh]].astype(np.float64) * 0.75)
    with pytest.raises(ValueError, match="material and tri_rgb"):
        fr.set_mesh(mesh, tri_rgb=rgb, material=f.MeshMaterial())
    mesh.close()


def test_refusals_write_nothing(ctx):
    import torch
    f = _ffi()
    L = f.load()
    V, F = mmc.SHADE_MESH
    M = mmc.material_arrays()
    mesh = f.Mesh(ctx, V, F)
    p = _params(f)
    fr = mmc.device_frame(ctx, 1)
    fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**M))
    fr.render(p)
    good = fr.mesh_material[1]
    out = torch.full((fr.P, 4), -7.0, dtype=torch.float64, device=fr.dev)

    def call(mat=good, scene=None, mesh_h=mesh._h, samples=1, c=ctx._h):
        scene = fr.scene() if scene is None else scene
        rc = L.bhg_shade_mesh_material_device(c, fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.d_tri_id.data_ptr(),
                                              fr.d_bary.data_ptr(), fr.P, samples, C.byref(scene), mesh_h,
                                              None if mat is None else C.byref(mat), out.data_ptr(), None, None,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, L.bhg_last_error().decode()

    def variant(**kw):
        m = f.MeshMaterialStruct.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(m, k)[v[0]] = v[1]
            else:
                setattr(m, k, v)
        return m

    spheres = fr.scene()
    spheres.n_spheres = 1
    cases = [
        (dict(mat=variant(emission=-0.1)), "emission"), (dict(mat=variant(emission=float("nan"))), "emission"),
        (dict(mat=variant(emission=float("inf"))), "emission"),
        (dict(mat=variant(n_tex=9)), "n_tex"), (dict(mat=variant(n_tex=-1)), "n_tex"),
        (dict(mat=variant(tex=(1, None))), r"tex\[1\]"), (dict(mat=variant(tex_w=(2, 0))), r"tex\[2\]"),
        (dict(mat=variant(tex_h=(0, -3))), r"tex\[0\]"),
        (dict(mat=variant(n_tex=0)), "tri_uv"),
        (dict(mat=None), "material"),
        # ... and everything bhg_shade_mesh_device refuses
        (dict(scene=spheres), "n_spheres"), (dict(mesh_h=None), "mesh is NULL"), (dict(samples=0), "samples"),
        (dict(c=None), "ctx is NULL"),
    ]
    import re
    for kw, names in cases:
        rc, msg = call(**kw)
        assert rc == f.E_INVALID and re.search(names, msg), (kw, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == f.OK and bool((out != -7.0).all())
    # the host-array form scans the arrays: the library-owned frame's refusals
    frame = mmc.frame(f, [0], f.GATHER_AUTO)
    bad_uv = M["tri_uv"].copy()
    bad_uv[5, 1, 0] = np.inf
    far_uv = M["tri_uv"].copy()
    far_uv[9, 2, 1] = 2.0 ** 20 + 1.0
    bad_slot = M["tri_tex"].copy()
    bad_slot[3] = 3
    for kw, names in ((dict(tri_uv=bad_uv), "tri_uv"), (dict(tri_uv=far_uv), "tri_uv"), (dict(tri_tex=bad_slot), "tri_tex"),
                      (dict(emission=-1.0), "emission"), (dict(textures=[]), "tri_uv")):
        with pytest.raises(f.BhgError, match=names):
            frame.set_mesh(V, F, material=f.MeshMaterial(**dict(M, **kw)))
    frame.close()
    mesh.close()

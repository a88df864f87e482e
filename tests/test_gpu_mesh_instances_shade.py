"""The instanced mesh shade and mesh instances on the two frames (bhg_shade_mesh_instances_device, DeviceFrame.set_mesh(instances=),
bhg_frame_set_mesh_instances):

  * one instance under the identity is bhg_shade_mesh_material_device's image, bit for bit, textures and emission included;
  * the shade against tests/mesh_reference.py's mesh_colour on the FLATTENED mesh, on the device's own records: S in {1, 5}, flat
    and vertex normals, two lamps, inst_rgb; 1e-12 relative, a ray with a shadow decision whose margin is under 1e-9 exempt (under
    1 % of the decisions); some lamp is shadowed by ANOTHER instance than the one the ray is on;
  * the library-owned frame gives DeviceFrame's shade_f32 image in every gather path, instances off is the frame that never had
    them, moving the instances is a fresh frame given the new transforms, the refusals leave a sentinel-filled image alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_instance_cases as mi
import mesh_material_cases as mmc
import mesh_reference as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


# the ellipsoid of the trace tests, 1.5 times as large, in three placements of the shade scene: the second stands between the first
# lamp and the first (where mesh_material_cases has its tetrahedron), the third above them
AXES = 1.5 * np.array([1.0, 0.6, 0.4])
SPOTS = (mmc.SPHERE_C, mmc.TETRA_C, (-1.6, 3.2, 3.1))
INST_RGB = np.array([[1.0, 0.6, 0.5], [0.4, 1.0, 0.7], [0.8, 0.5, 1.0]], np.float32)


def local_mesh():
    V, F = mr.octa_sphere((0.0, 0.0, 0.0), 1.0, 2)
    N = V / AXES                     # the ellipsoid's gradient at the vertex V * AXES
    return V * AXES, F, N / np.linalg.norm(N, axis=1)[:, None]


def placements(shift=0.0):
    rots = (mi.rotation((1.0, 2.0, 0.5), 0.7 + shift), mi.rotation((0.0, 1.0, -1.0), 2.1), mi.rotation((-1.0, 0.3, 2.0), -1.3 - shift))
    return np.stack([mi.record(R, np.asarray(t) + shift * np.array([0.3, -0.2, 0.25])) for R, t in zip(rots, SPOTS)])


def _params(f):
    return f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=mmc.SHADE_DISK[0], disk_r_out=mmc.SHADE_DISK[1])


def _image(fr, p):
    import torch
    fr.generate_rays(p)
    fr.trace(p)
    out = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- the identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "vertex_normals"])
def test_identity_is_the_material_shade(ctx, smooth):
    import torch
    f = _ffi()
    V, F = mmc.SHADE_MESH
    mesh = f.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals() if smooth else None)
    p = _params(f)
    for S in (1, 5):
        for mat in (f.MeshMaterial(**mmc.material_arrays()), None):
            plain, inst = mmc.device_frame(ctx, S), mmc.device_frame(ctx, S)
            plain.set_mesh(mesh, chord=mmc.CHORD, material=mat if mat is not None else f.MeshMaterial())
            inst.set_mesh(mesh, chord=mmc.CHORD, material=mat, instances=mi.IDENTITY)
            a, b = plain.render(p).cpu().numpy().copy(), inst.render(p).cpu().numpy().copy()
            torch.cuda.synchronize()
            on_mesh = (plain.d_flags == 0x88) & (plain.d_tri_id >= 0)
            assert int(on_mesh.sum()) > 60 * S
            for key in ("d_end", "d_flags", "d_tri_id", "d_bary", "d_steps", "d_acc"):
                x, y = getattr(plain, key), getattr(inst, key)
                assert torch.equal(x[on_mesh], y[on_mesh]) if key == "d_bary" else torch.equal(x, y), key
            assert torch.equal(inst.d_inst_id, torch.where(on_mesh, 0, -1).to(torch.int32))
            assert np.array_equal(a, b) and np.abs(a[:, :3]).max() > 0.0
    mesh.close()


# ---- against the restatement on the flattened mesh -------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "vertex_normals"])
def test_shade_against_the_restatement(ctx, S, smooth):
    import torch
    f = _ffi()
    V, F, N = local_mesh()
    T = placements()
    nt, K = len(F), len(T)
    tri_rgb = np.random.default_rng(3).uniform(0.2, 1.0, (nt, 3)).astype(np.float32)
    mesh = f.Mesh(ctx, V, F, vertex_normals=N if smooth else None)
    p = _params(f)
    fr = mmc.device_frame(ctx, S)
    fr.set_mesh(mesh, tri_rgb=tri_rgb, chord=mmc.CHORD, instances=T, inst_rgb=INST_RGB)
    got = fr.render(p).cpu().numpy().copy()
    out32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out32)
    torch.cuda.synchronize()
    end, flags, tri, inst, bary = (t.cpu().numpy() for t in (fr.d_end, fr.d_flags, fr.d_tri_id, fr.d_inst_id, fr.d_bary))
    on_mesh = (flags == 0x88) & (tri >= 0)
    assert np.array_equal(on_mesh, inst >= 0) and on_mesh.sum() > 60 * S
    per = np.bincount(inst[on_mesh], minlength=K)
    assert np.all(per >= 10 * S), per
    # every other ray's colour is the plain shade's (one sample per "pixel": each ray's colour by itself)
    per_ray = torch.empty((fr.n, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.n, 1, fr.scene(), per_ray.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    col = per_ray.cpu().numpy()[:, :3].copy()
    # the mesh rays: the lamp sum of mesh_colour on the flattened mesh (white), times tri_rgb[T] * inst_rgb[j] in fp64
    Vf, Ff = mi.flatten(V, F, T)
    Nf = np.concatenate([N @ rec[:9].reshape(3, 3).T for rec in T]) if smooth else None
    idx = np.flatnonzero(on_mesh)
    exempt, decisions, near, by_another = np.zeros(fr.n, bool), 0, 0, 0
    for i in idx:
        j, t = int(inst[i]), int(tri[i])
        margins = []
        lamp_sum = mr.mesh_colour(end[i:i + 1], [j * nt + t], bary[i:i + 1], Vf, Ff, mmc.SHADE_LAMPS, None, Nf, margins=margins)[0, 0]
        decisions += len(margins)
        close = sum(m < 1e-9 for m in margins)
        near += close
        exempt[i] = close > 0
        own = mr.mesh_colour(end[i:i + 1], [t], bary[i:i + 1], Vf[j * len(V):(j + 1) * len(V)], F, mmc.SHADE_LAMPS, None,
                             None if Nf is None else Nf[j * len(V):(j + 1) * len(V)])[0, 0]
        by_another += lamp_sum < own
        col[i] = (tri_rgb[t].astype(np.float64) * INST_RGB[j].astype(np.float64)) * lamp_sum
    print(f"S {S}, {'vertex' if smooth else 'flat'} normals: {len(idx)} mesh rays {per}, {decisions} shadow decisions, {near} within 1e-9, "
          f"{by_another} rays with a lamp shadowed by another instance, lit {int((col[idx].sum(1) > 0).sum())}")
    assert near <= 0.01 * decisions
    assert by_another >= 1 and (col[idx].sum(1) > 0).sum() > 20
    want = np.zeros((fr.P, 3))
    for s in range(S):
        want += col[s * fr.P:(s + 1) * fr.P]
    want /= S
    held = ~exempt.reshape(S, fr.P).any(0)
    err = np.abs(got[:, :3] - want)
    print(f"worst |gpu - numpy| {err[held].max():.3e}")
    assert np.all(err[held] <= 1e-12 * np.maximum(1.0, np.abs(want[held]))) and np.all(got[:, 3] == 1.0)
    assert np.array_equal(out32.cpu().numpy(), got.astype(np.float32))
    # without inst_rgb the copies are the mesh's own colour
    fr.set_mesh(mesh, tri_rgb=tri_rgb, chord=mmc.CHORD, instances=T)
    white = fr.render(p).cpu().numpy()
    pix = on_mesh.reshape(S, fr.P).any(0)
    assert np.array_equal(white[~pix], got[~pix]) and np.all(white[pix, :3] >= got[pix, :3]) and np.any(white[pix, :3] > got[pix, :3])
    mesh.close()


# ---- the frames ----------------------------------------------------------------------------------------------------------------
def _material(f):
    """mesh_material_cases' material, cut to this mesh's triangles: colours, UVs, three images, emission."""
    M, nt = mmc.material_arrays(), len(local_mesh()[1])
    return f.MeshMaterial(tri_rgb=M["tri_rgb"][:nt], tri_uv=M["tri_uv"][:nt], tri_tex=M["tri_tex"][:nt], textures=M["textures"], emission=0.1)


def _frame_mesh(f, fr):
    V, F, N = local_mesh()
    fr.set_mesh(V, F, vertex_normals=N, chord=mmc.CHORD, material=_material(f))


def _device_frame_image(ctx, p, T, rgb):
    f = _ffi()
    V, F, N = local_mesh()
    dfr = mmc.device_frame(ctx, mmc.FRAME_S, mmc.FRAME_W, mmc.FRAME_H, mmc.FRAME_FOV, sampling_seed=42.0)
    mesh = f.Mesh(ctx, V, F, vertex_normals=N)
    dfr.set_mesh(mesh, chord=mmc.CHORD, material=_material(f), instances=T, inst_rgb=rgb)
    img = _image(dfr, p).reshape(mmc.FRAME_H, mmc.FRAME_W, 4)
    hits = np.bincount(dfr.d_inst_id.cpu().numpy()[dfr.d_inst_id.cpu().numpy() >= 0], minlength=len(T))
    mesh.close()
    return img, hits


_RCCL_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from blackhole_geodesic_calculator_amd import _ffi as f
import mesh_material_cases as mmc
import test_gpu_mesh_instances_shade as t
try:
    fr = mmc.frame(f, [0], f.GATHER_RCCL)
except f.BhgError as e:
    print("RCCL unavailable:", e)
    sys.exit(0)
t._frame_mesh(f, fr)
fr.set_mesh_instances(t.placements(), t.INST_RGB)
img = fr.render(mmc.frame_params(f))
assert fr.info()["gather"] == "rccl", fr.info()
np.save(%(out)r, img)
fr.close()
print("rccl instanced frame ok")
"""


def test_every_gather_path_gives_device_frames_image(ctx, tmp_path):
    f = _ffi()
    p = mmc.frame_params(f)
    T = placements()
    images = {}
    for name, devs, gather in (("one", [0], f.GATHER_AUTO), ("copy", [0, 0], f.GATHER_COPY),
                               ("peercall", [0, 0], f.GATHER_COPY_PEERCALL), ("peer", [0, 0], f.GATHER_PEER)):
        try:
            fr = mmc.frame(f, devs, gather)
        except f.BhgError as e:
            print(f"gather mode {name} is not available here: {e}")
            continue
        _frame_mesh(f, fr)
        fr.set_mesh_instances(T, INST_RGB)
        images[name] = fr.render(p)
        fr.close()
    assert "one" in images and len(images) >= 2
    for name, img in images.items():
        assert np.array_equal(img, images["one"]), name
    want, hits = _device_frame_image(ctx, p, T, INST_RGB)
    assert np.all(hits >= 100), hits
    assert np.array_equal(images["one"], want)
    out = tmp_path / "rccl.npy"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD % dict(root=ROOT, out=str(out))], capture_output=True, text=True, timeout=150,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if "RCCL unavailable" in r.stdout:
        print(r.stdout)
    else:
        assert "rccl instanced frame ok" in r.stdout and np.array_equal(np.load(out), images["one"])


def test_off_moving_and_the_refusals(ctx):
    f = _ffi()
    L = f.load()
    p = mmc.frame_params(f)
    T, T2 = placements(), placements(0.4)
    for devs in ([0], [0, 0]):
        gather = f.GATHER_AUTO if len(devs) == 1 else f.GATHER_COPY
        fr = mmc.frame(f, devs, gather)
        # refused on a frame that holds no mesh
        with pytest.raises(f.BhgError, match="holds no mesh"):
            fr.set_mesh_instances(T)
        _frame_mesh(f, fr)
        plain = fr.render(p)
        fr.set_mesh_instances(T, INST_RGB)
        first = fr.render(p)
        assert np.abs(first - plain).max() > 1e-3
        # refused transforms leave the frame rendering what it rendered
        bad = T.copy()
        bad[2, 4] = np.nan
        with pytest.raises(f.BhgError, match="finite"):
            fr.set_mesh_instances(bad)
        with pytest.raises(f.BhgError, match="R\\^T R"):
            fr.set_mesh_instances(T * 1.001)
        with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
            fr.set_mesh_instances(np.tile(T[:1], (65, 1)))
        with pytest.raises(f.BhgError, match="inst_rgb"):
            fr.set_mesh_instances(T, np.full((3, 3), np.inf, np.float32))
        assert np.array_equal(fr.render(p), first)
        # moved: a fresh frame given those transforms
        fr.set_mesh_instances(T2, INST_RGB)
        moved = fr.render(p)
        fresh = mmc.frame(f, devs, gather)
        _frame_mesh(f, fresh)
        fresh.set_mesh_instances(T2, INST_RGB)
        assert np.array_equal(moved, fresh.render(p)) and np.abs(moved - first).max() > 1e-3
        # ... and another number of instances
        fr.set_mesh_instances(T2[:2], INST_RGB[:2])
        fresh.set_mesh_instances(T2[:2], INST_RGB[:2])
        assert np.array_equal(fr.render(p), fresh.render(p))
        # a mesh does not go with scene spheres: refused at render, a sentinel-filled image left alone
        fresh.set_scene(_sky(), disk=mmc.SHADE_DISK, lamps=mmc.SHADE_LAMPS, spheres=[[0.0, 5.0, 0.0, 1.0]])
        sentinel = np.full((mmc.FRAME_H, mmc.FRAME_W, 4), -7.0, np.float32)
        rc = L.bhg_frame_render(fresh._h, C.byref(p), C.c_void_p(sentinel.ctypes.data))
        assert rc == f.E_INVALID and b"a mesh does not go with scene spheres" in L.bhg_last_error() and np.all(sentinel == -7.0)
        fresh.close()
        # off: the plain mesh render, bit for bit -- by n = 0, and by set_mesh with new arrays
        fr.set_mesh_instances(None)
        assert np.array_equal(fr.render(p), plain)
        fr.set_mesh_instances(T, INST_RGB)
        assert np.array_equal(fr.render(p), first)
        _frame_mesh(f, fr)
        assert np.array_equal(fr.render(p), plain)
        never = mmc.frame(f, devs, gather)
        _frame_mesh(f, never)
        assert np.array_equal(never.render(p), plain)
        never.close()
        fr.close()


def _sky():
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    return synthetic_sky(128, 64)


def test_device_frame_moves_its_instances(ctx):
    f = _ffi()
    p = _params(f)
    V, F, N = local_mesh()
    mesh = f.Mesh(ctx, V, F, vertex_normals=N)
    T, T2 = placements(), placements(0.4)
    a = mmc.device_frame(ctx, 2)
    a.set_mesh(mesh, chord=mmc.CHORD, instances=T, inst_rgb=INST_RGB)
    first = _image(a, p)
    a.set_mesh_instances(T2)
    moved = _image(a, p)
    b = mmc.device_frame(ctx, 2)
    b.set_mesh(mesh, chord=mmc.CHORD, instances=T2, inst_rgb=INST_RGB)
    assert np.array_equal(moved, _image(b, p)) and not np.array_equal(moved, first)
    a.set_mesh_instances(None)
    b.set_mesh(mesh, chord=mmc.CHORD)
    assert np.array_equal(_image(a, p), _image(b, p))
    mesh.close()


def test_shade_refusals_write_nothing(ctx):
    import torch
    f = _ffi()
    L = f.load()
    V, F, N = local_mesh()
    mesh = f.Mesh(ctx, V, F, vertex_normals=N)
    p = _params(f)
    fr = mmc.device_frame(ctx, 1)
    fr.set_mesh(mesh, chord=mmc.CHORD, instances=placements(), inst_rgb=INST_RGB)
    fr.render(p)
    out = torch.full((fr.P, 4), -7.0, dtype=torch.float64, device=fr.dev)

    def call(c=ctx._h, inst=fr.mesh_instances._h, inst_id=fr.d_inst_id.data_ptr(), tri=fr.d_tri_id.data_ptr(), scene=None, samples=1, mat=None):
        scene = fr.scene() if scene is None else scene
        rc = L.bhg_shade_mesh_instances_device(c, fr.d_end.data_ptr(), fr.d_flags.data_ptr(), tri, inst_id, fr.d_bary.data_ptr(), fr.P,
                                               samples, C.byref(scene), inst, None if mat is None else C.byref(mat),
                                               fr.d_inst_rgb.data_ptr(), out.data_ptr(), None, None,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, L.bhg_last_error().decode()

    spheres = fr.scene()
    spheres.n_spheres = 1
    bad_mat = f.MeshMaterial(emission=-1.0).struct([0, 0, 0])
    other = f.Context(0)
    V2, F2 = np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)
    T = np.ascontiguousarray(placements())
    hm, hi = C.c_void_p(), C.c_void_p()
    assert L.bhg_mesh_create(ctx._h, V2.ctypes.data, len(V2), F2.ctypes.data, len(F2), None, 4, C.byref(hm)) == 0
    assert L.bhg_mesh_instances_create(ctx._h, hm, 3, T.ctypes.data, C.byref(hi)) == 0
    L.bhg_mesh_destroy(hm)
    try:
        for kw, why in ((dict(inst=None), "inst is NULL"), (dict(inst_id=None), "inst_id is NULL"), (dict(tri=None), "NULL device pointer"),
                        (dict(scene=spheres), "n_spheres"), (dict(samples=0), "samples"), (dict(mat=bad_mat), "emission"),
                        (dict(c=None), "ctx is NULL"), (dict(c=other._h), "another context"), (dict(inst=hi), "mesh has been destroyed")):
            rc, msg = call(**kw)
            assert rc == f.E_INVALID and why in msg, (kw, msg)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        rc, msg = call()
        torch.cuda.synchronize()
        assert rc == f.OK and bool((out != -7.0).all())
    finally:
        L.bhg_mesh_instances_destroy(hi)
        other.close()
        mesh.close()

"""The shade over an instance set under a tree (MeshInstanceTreeColour: the shadow segments walk the tree in any-hit form), and
such sets on the two frames and in the add-on (DeviceFrame.set_mesh(instance_tree=True), bhg_frame_set_mesh_instance_tree,
scene.curved_space_mesh_instance_tree):

  * K = 65 creates, traces and shades on DeviceFrame, and the library-owned frame renders it;
  * at K <= 64 the tree set's image is the linear set's, bit for bit: S in {1, 5}, flat and vertex normals, two lamps, inst_rgb --
    on section 21's three placements and on 24 that crowd one another;
  * on the clump of 96 (mesh_instance_tree_cases) every mesh ray's colour lies within 1e-14 of mesh_reference.mesh_colour on the
    FLATTENED mesh, every other ray's is the plain shade's, and some ray has a lamp shadowed by another instance;
  * the library-owned frame at K = 96: every gather path and two contexts of one device give DeviceFrame's image, off is the
    frame that never had instances, a moved frame is a fresh frame, refusals leave a sentinel-filled image alone;
  * the add-on on the stub bpy: 70 linked duplicates render as instances with the property on, the concatenated path's image
    within test_gpu_addon_mesh_instances' bound; with the property off the path taken is the concatenated one.

The colours of mesh rays stay under 1 here (I^2 / d^2 <= 0.4 per lamp), and a colour is a sum of two terms of a few roundings
each: 1e-14 leaves a factor of ten over the 8.9e-16 section 21 saw."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_bpy_mesh as fbm  # noqa: E402
import mesh_instance_cases as mi  # noqa: E402
import mesh_instance_tree_cases as mt  # noqa: E402
import mesh_material_cases as mmc  # noqa: E402
import mesh_oracle_cases as mo  # noqa: E402
import mesh_reference as mr  # noqa: E402
from test_gpu_mesh_instances_shade import INST_RGB, _image, _params, local_mesh, placements  # noqa: E402
from test_mesh_material_host import BH_LOC, mesh_scene  # noqa: E402

pytestmark = pytest.mark.gpu


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


TETRA = mr.tetrahedron((0.0, 0.0, 0.0), 0.5)


def crowd(K=24, seed=61):
    """section 21's three placements and K - 3 more of the same mesh about the shade scene's aim point: they overlap and shadow."""
    rng = np.random.default_rng(seed)
    more = [mi.record(mi.rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)), mmc.SHADE_AIM + rng.normal(size=3) * 1.6)
            for _ in range(K - 3)]
    return np.concatenate([placements(), np.stack(more)])


def clump_in_the_shade_scene(shift=0.0):
    """The clump's 96 placements, carried from mesh_oracle_cases.FRAME_SPHERE to the shade scene's aim point."""
    T = mt.clump_placements()
    T[:, 9:] += mmc.SHADE_AIM - np.asarray(mo.FRAME_SPHERE) + shift * np.array([0.3, -0.2, 0.25])
    if shift:
        T[:, :9] = np.einsum("ij,njk->nik", mi.rotation((0.3, 1.0, 0.2), shift), T[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    return T


# ---- more than 64 --------------------------------------------------------------------------------------------------------------
def test_65_placements_shade_and_render(ctx):
    import torch
    f = _ffi()
    T = clump_in_the_shade_scene()[:65]
    rgb = np.random.default_rng(5).uniform(0.3, 1.0, (65, 3)).astype(np.float32)
    mesh = f.Mesh(ctx, *TETRA)
    p = _params(f)
    fr = mmc.device_frame(ctx, 2)
    with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
        fr.set_mesh(mesh, chord=mmc.CHORD, instances=T, inst_rgb=rgb)
    fr.set_mesh(mesh, chord=mmc.CHORD, instances=T, inst_rgb=rgb, instance_tree=True, instance_leaf_size=2)
    assert fr.mesh_instances.tree_info() == (65, 6, 2)
    img = _image(fr, p)
    torch.cuda.synchronize()
    inst = fr.d_inst_id.cpu().numpy()
    assert (inst >= 0).sum() >= 200 and len(np.unique(inst[inst >= 0])) >= 15 and inst.max() < 65
    assert np.all(np.isfinite(img)) and np.all(img[:, 3] == 1.0)
    # set_mesh_instances keeps the kind of the set
    fr.set_mesh_instances(clump_in_the_shade_scene(0.3)[:65])
    assert fr.mesh_instances.tree_info() == (65, 6, 2) and not np.array_equal(_image(fr, p), img)
    fr.set_mesh_instances(clump_in_the_shade_scene()[:70])
    assert fr.mesh_instances.tree_info()[2] == 2 and fr.mesh_instances.n == 70
    mesh.close()
    # the library-owned frame
    lf = mmc.frame(f, [0], f.GATHER_AUTO)
    lf.set_mesh(*TETRA, chord=mmc.CHORD)
    plain = lf.render(mmc.frame_params(f))
    with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
        lf.set_mesh_instances(T, rgb)
    lf.set_mesh_instances(T, rgb, tree=True)
    out = lf.render(mmc.frame_params(f))
    assert (np.abs(out - plain).max(-1) > 1e-3).sum() > 100
    lf.close()


# ---- at K <= 64 the image is the linear set's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "vertex_normals"])
@pytest.mark.parametrize("which", ["three", "crowd"])
def test_the_tree_sets_image_is_the_linear_sets(ctx, which, smooth, S):
    import torch
    f = _ffi()
    V, F, N = local_mesh()
    T = placements() if which == "three" else crowd()
    rgb = INST_RGB if which == "three" else np.random.default_rng(7).uniform(0.3, 1.0, (len(T), 3)).astype(np.float32)
    tri_rgb = np.random.default_rng(3).uniform(0.2, 1.0, (len(F), 3)).astype(np.float32)
    mesh = f.Mesh(ctx, V, F, vertex_normals=N if smooth else None)
    p = _params(f)
    assert len(mmc.SHADE_LAMPS) == 2
    lin = mmc.device_frame(ctx, S)
    lin.set_mesh(mesh, tri_rgb=tri_rgb, chord=mmc.CHORD, instances=T, inst_rgb=rgb)
    want = lin.render(p).cpu().numpy().copy()
    want32 = _image(lin, p)
    for leaf in (1, 2, 4):
        fr = mmc.device_frame(ctx, S)
        fr.set_mesh(mesh, tri_rgb=tri_rgb, chord=mmc.CHORD, instances=T, inst_rgb=rgb, instance_tree=True, instance_leaf_size=leaf)
        got = fr.render(p).cpu().numpy().copy()
        for key in ("d_end", "d_flags", "d_tri_id", "d_inst_id", "d_steps", "d_acc"):
            assert torch.equal(getattr(fr, key), getattr(lin, key)), key
        assert np.array_equal(got, want) and np.array_equal(_image(fr, p), want32), leaf
    inst = lin.d_inst_id.cpu().numpy()
    assert (inst >= 0).sum() > 60 * S and len(np.unique(inst[inst >= 0])) >= (3 if which == "three" else 8)
    mesh.close()


# ---- the clump against the restatement on the flattened mesh ---------------------------------------------------------------------
def test_the_clumps_colours_against_the_restatement(ctx):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    f = _ffi()
    case = mt.clump_case("christoffel")
    V, F, T = case["Vl"], case["Fl"], case["T"]
    nt, n = len(F), len(case["k0"])
    mesh = f.Mesh(ctx, V, F)
    try:
        inst = f.MeshInstances(mesh, T, tree=True)
        r = mi.trace_instances_device(ctx, f.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"]), inst, case["chord"],
                                      case["k0"], case["x0"])
        dev = {k: torch.as_tensor(np.ascontiguousarray(r[k])).cuda() for k in ("end", "flags", "tri", "inst", "bary")}
        sky = torch.as_tensor(np.ascontiguousarray(synthetic_sky(128, 64), dtype=np.float32)).cuda()
        sc = f.make_scene(sky.data_ptr(), 128, 64, disk=(case["par"]["disk_r_in"], case["par"]["disk_r_out"]), lamps=mt.CLUMP_LAMPS)
        rgb = np.random.default_rng(11).uniform(0.3, 1.0, (len(T), 3)).astype(np.float32)
        d_rgb = torch.as_tensor(rgb).cuda()
        out = torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda")
        plain = torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        # one sample per "pixel": each ray's colour by itself
        ctx.shade_mesh_instances_device(dev["end"].data_ptr(), dev["flags"].data_ptr(), dev["tri"].data_ptr(), dev["inst"].data_ptr(),
                                        dev["bary"].data_ptr(), n, 1, sc, inst, d_inst_rgb=d_rgb.data_ptr(), d_rgba=out.data_ptr(), stream=st)
        ctx.shade_scene_device(dev["end"].data_ptr(), dev["flags"].data_ptr(), n, 1, sc, plain.data_ptr(), stream=st)
        torch.cuda.synchronize()
        got, col = out.cpu().numpy(), plain.cpu().numpy()[:, :3].copy()
    finally:
        mesh.close()
    on_mesh = r["tri"] >= 0
    assert on_mesh.sum() >= 200 and np.all(got[:, 3] == 1.0)
    assert np.array_equal(got[~on_mesh, :3], col[~on_mesh])
    Vf, Ff = mi.flatten(V, F, T)
    by_another, decisions, near = 0, 0, 0
    for i in np.flatnonzero(on_mesh):
        j, t = int(r["inst"][i]), int(r["tri"][i])
        margins = []
        lamp_sum = mr.mesh_colour(r["end"][i:i + 1], [j * nt + t], r["bary"][i:i + 1], Vf, Ff, mt.CLUMP_LAMPS, margins=margins)[0, 0]
        own = mr.mesh_colour(r["end"][i:i + 1], [t], r["bary"][i:i + 1], Vf[j * len(V):(j + 1) * len(V)], F, mt.CLUMP_LAMPS)[0, 0]
        by_another += lamp_sum < own
        decisions += len(margins)
        near += sum(m < 1e-9 for m in margins)
        col[i] = rgb[j].astype(np.float64) * lamp_sum
    err = np.abs(got[on_mesh, :3] - col[on_mesh])
    lit = int((col[on_mesh].sum(1) > 0).sum())
    print(f"clump: {int(on_mesh.sum())} mesh rays, {lit} lit, {by_another} with a lamp shadowed by another instance, {decisions} shadow "
          f"decisions ({near} within 1e-9 of an edge), worst |gpu - numpy| {err.max():.3e}, largest colour {col[on_mesh].max():.3f}")
    assert by_another >= 1 and lit >= 20
    assert err.max() <= 1e-14


# ---- the library-owned frame at K = 96 -------------------------------------------------------------------------------------------
def _tetra_material(f):
    M, nt = mmc.material_arrays(), len(TETRA[1])
    return f.MeshMaterial(tri_rgb=M["tri_rgb"][:nt], tri_uv=M["tri_uv"][:nt], tri_tex=M["tri_tex"][:nt], textures=M["textures"], emission=0.1)


def _frame_mesh(f, fr):
    fr.set_mesh(*TETRA, chord=mmc.CHORD, material=_tetra_material(f))


FRAME_RGB = np.random.default_rng(13).uniform(0.3, 1.0, (96, 3)).astype(np.float32)


def _device_frame_image(ctx, p, T, rgb):
    f = _ffi()
    dfr = mmc.device_frame(ctx, mmc.FRAME_S, mmc.FRAME_W, mmc.FRAME_H, mmc.FRAME_FOV, sampling_seed=42.0)
    mesh = f.Mesh(ctx, *TETRA)
    dfr.set_mesh(mesh, chord=mmc.CHORD, material=_tetra_material(f), instances=T, inst_rgb=rgb, instance_tree=True)
    img = _image(dfr, p).reshape(mmc.FRAME_H, mmc.FRAME_W, 4)
    ids = dfr.d_inst_id.cpu().numpy()
    mesh.close()
    return img, ids[ids >= 0]


_RCCL_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from blackhole_geodesic_calculator_amd import _ffi as f
import mesh_material_cases as mmc
import test_gpu_mesh_instance_tree_shade as t
try:
    fr = mmc.frame(f, [0], f.GATHER_RCCL)
except f.BhgError as e:
    print("RCCL unavailable:", e)
    sys.exit(0)
t._frame_mesh(f, fr)
fr.set_mesh_instances(t.clump_in_the_shade_scene(), t.FRAME_RGB, tree=True)
img = fr.render(mmc.frame_params(f))
assert fr.info()["gather"] == "rccl", fr.info()
np.save(%(out)r, img)
fr.close()
print("rccl instance tree frame ok")
"""


def test_every_gather_path_gives_device_frames_image(ctx, tmp_path):
    f = _ffi()
    p = mmc.frame_params(f)
    T = clump_in_the_shade_scene()
    images = {}
    for name, devs, gather in (("one", [0], f.GATHER_AUTO), ("copy", [0, 0], f.GATHER_COPY),
                               ("peercall", [0, 0], f.GATHER_COPY_PEERCALL), ("peer", [0, 0], f.GATHER_PEER)):
        try:
            fr = mmc.frame(f, devs, gather)
        except f.BhgError as e:
            print(f"gather mode {name} is not available here: {e}")
            continue
        _frame_mesh(f, fr)
        fr.set_mesh_instances(T, FRAME_RGB, tree=True)
        images[name] = fr.render(p)
        fr.close()
    assert "one" in images and len(images) >= 2
    for name, img in images.items():
        assert np.array_equal(img, images["one"]), name
    want, ids = _device_frame_image(ctx, p, T, FRAME_RGB)
    assert len(ids) >= 500 and len(np.unique(ids)) >= 20
    assert np.array_equal(images["one"], want)
    out = tmp_path / "rccl.npy"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD % dict(root=ROOT, out=str(out))], capture_output=True, text=True, timeout=150,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if "RCCL unavailable" in r.stdout:
        print(r.stdout)
    else:
        assert "rccl instance tree frame ok" in r.stdout and np.array_equal(np.load(out), images["one"])


def test_off_moving_and_the_refusals(ctx):
    f = _ffi()
    L = f.load()
    p = mmc.frame_params(f)
    T, T2 = clump_in_the_shade_scene(), clump_in_the_shade_scene(0.4)
    for devs in ([0], [0, 0]):
        gather = f.GATHER_AUTO if len(devs) == 1 else f.GATHER_COPY
        fr = mmc.frame(f, devs, gather)
        with pytest.raises(f.BhgError, match="holds no mesh"):
            fr.set_mesh_instances(T, tree=True)
        _frame_mesh(f, fr)
        plain = fr.render(p)
        fr.set_mesh_instances(T, FRAME_RGB, tree=True)
        first = fr.render(p)
        assert np.abs(first - plain).max() > 1e-3
        # refused, the frame rendering what it rendered
        bad = T.copy()
        bad[70, 4] = np.nan
        with pytest.raises(f.BhgError, match="finite"):
            fr.set_mesh_instances(bad, tree=True)
        with pytest.raises(f.BhgError, match="R\\^T R"):
            fr.set_mesh_instances(T * 1.001, tree=True)
        with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCE_TREE_MAX"):
            fr.set_mesh_instances(np.tile(T[:1], (65537, 1)), tree=True)
        with pytest.raises(f.BhgError, match="leaf_size"):
            fr.set_mesh_instances(T, tree=True, leaf_size=0)
        with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
            fr.set_mesh_instances(T)                     # the old call refuses 96 as it did
        with pytest.raises(f.BhgError, match="inst_rgb"):
            fr.set_mesh_instances(T, np.full((96, 3), np.inf, np.float32), tree=True)
        assert np.array_equal(fr.render(p), first)
        # moved: a fresh frame given those transforms
        fr.set_mesh_instances(T2, FRAME_RGB, tree=True)
        moved = fr.render(p)
        fresh = mmc.frame(f, devs, gather)
        _frame_mesh(f, fresh)
        fresh.set_mesh_instances(T2, FRAME_RGB, tree=True)
        assert np.array_equal(moved, fresh.render(p)) and np.abs(moved - first).max() > 1e-3
        # ... another number of instances, and the other kind of set
        fr.set_mesh_instances(T2[:80], FRAME_RGB[:80], tree=True)
        fresh.set_mesh_instances(T2[:80], FRAME_RGB[:80], tree=True)
        assert np.array_equal(fr.render(p), fresh.render(p))
        fr.set_mesh_instances(T2[:40], FRAME_RGB[:40], tree=True)
        fresh.set_mesh_instances(T2[:40], FRAME_RGB[:40])
        assert np.array_equal(fr.render(p), fresh.render(p))
        fresh.set_mesh_instances(T2[:40], FRAME_RGB[:40], tree=True, leaf_size=4)
        assert np.array_equal(fr.render(p), fresh.render(p))
        # a mesh does not go with scene spheres: refused at render, a sentinel-filled image left alone
        fresh.set_mesh_instances(T, FRAME_RGB, tree=True)
        fresh.set_scene(_sky(), disk=mmc.SHADE_DISK, lamps=mmc.SHADE_LAMPS, spheres=[[0.0, 5.0, 0.0, 1.0]])
        sentinel = np.full((mmc.FRAME_H, mmc.FRAME_W, 4), -7.0, np.float32)
        rc = L.bhg_frame_render(fresh._h, C.byref(p), C.c_void_p(sentinel.ctypes.data))
        assert rc == f.E_INVALID and b"a mesh does not go with scene spheres" in L.bhg_last_error() and np.all(sentinel == -7.0)
        fresh.close()
        # off: the plain mesh render, bit for bit -- by n = 0, by the old call's n = 0, and by set_mesh with new arrays
        fr.set_mesh_instances(None)
        assert np.array_equal(fr.render(p), plain)
        fr.set_mesh_instances(T, FRAME_RGB, tree=True)
        assert np.array_equal(fr.render(p), first)
        assert L.bhg_frame_set_mesh_instance_tree(fr._h, 0, None, None, 2) == f.OK
        assert np.array_equal(fr.render(p), plain)
        fr.set_mesh_instances(T, FRAME_RGB, tree=True)
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


# ---- the add-on on the stub bpy ------------------------------------------------------------------------------------------------
W, H, S = 64, 48, 2
CAMERA = (BH_LOC[0] + 1e-4, BH_LOC[1], BH_LOC[2] + 30.0)
SCALE = (0.5, 0.3, 0.4)
N_COPIES = 70


def _worlds():
    """70 float32 matrices, as Blender keeps them: small cubes on a 10 x 7 grid below the camera, each turned its own way."""
    rng = np.random.default_rng(17)
    out = []
    for j in range(N_COPIES):
        m = np.eye(4)
        m[:3, :3] = mi.rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)) * np.asarray(SCALE)
        m[:3, 3] = (-6.3 + 1.4 * (j % 10), -4.8 + 1.3 * (j // 10), 6.0 + rng.uniform(0.0, 2.0))
        out.append(m.astype(np.float32).astype(np.float64))
    return out


def _render(addon, depsgraph):
    eng = addon.RelativisticRenderEngine()
    eng.render(depsgraph)
    return eng, np.array(eng.result.layers[0].passes["Combined"].rect, dtype=np.float32).reshape(H, W, 4)


def _scene(instances, tree):
    worlds = _worlds()
    bpy, depsgraph, addon, cube, tetra = mesh_scene(worlds[0], worlds[1], width=W, height=H, samples=S, camera=CAMERA, device_shading=1.0,
                                                    curved_space_meshes=1.0, curved_space_mesh_instances=instances,
                                                    curved_space_mesh_instance_tree=tree, render_devices=1.0)
    copies = [fbm.MeshObject(cube._mesh, w, curved_space_texture="crate.png") for w in worlds[1:]]      # linked duplicates
    for ob in [cube] + copies:
        ob.data = cube._mesh
    depsgraph.scene.objects[:] = [ob for ob in depsgraph.scene.objects if ob is not tetra] + copies
    return bpy, depsgraph, addon


def test_addon_renders_70_linked_duplicates_as_instances(ctx, monkeypatch):
    from blackhole_geodesic_calculator_amd import _ffi as f
    monkeypatch.setenv("BHGEO_DEVICES", "0")
    calls = []
    real_mesh, real_inst = f.Frame.set_mesh, f.Frame.set_mesh_instances
    monkeypatch.setattr(f.Frame, "set_mesh", lambda self, *a, **kw: (calls.append("mesh"), real_mesh(self, *a, **kw))[1])
    monkeypatch.setattr(f.Frame, "set_mesh_instances",
                        lambda self, *a, **kw: (calls.append(("instances", kw.get("tree", False))), real_inst(self, *a, **kw))[1])
    bpy, depsgraph, addon = _scene(1.0, 1.0)
    addon.register()
    eng, image = _render(addon, depsgraph)
    m = eng.scene_mesh(depsgraph)
    addon.unregister()
    assert calls == ["mesh", ("instances", True)]
    assert m["instances"].shape == (N_COPIES, 12) and m["vertices"].shape == (8, 3) and m["instance_tree"]
    # the property off: 70 objects are more than a linear set holds, and the path taken is the concatenated one, as before
    calls.clear()
    bpy, depsgraph, addon = _scene(1.0, 0.0)
    addon.register()
    eng, flat = _render(addon, depsgraph)
    m = eng.scene_mesh(depsgraph)
    addon.unregister()
    assert calls == ["mesh"] and m["instances"] is None and m["vertices"].shape == (8 * N_COPIES, 3)
    differ = np.abs(flat - image).max(-1) > 1e-4
    print(f"70 instances under a tree against the concatenated mesh: {int(differ.sum())} of {W * H} pixels differ by more than 1e-4, "
          f"worst {np.abs(flat - image).max():.2e}")
    assert differ.mean() <= 0.01
    # the cubes are in view
    bpy, depsgraph, addon = _scene(0.0, 0.0)
    depsgraph.scene.objects[:] = [ob for ob in depsgraph.scene.objects if getattr(ob, "type", "") != "MESH" or ob is depsgraph.scene.blackhole_obj]
    addon.register()
    _, empty = _render(addon, depsgraph)
    addon.unregister()
    assert (np.abs(image - empty).max(-1) > 1e-3).sum() > 150

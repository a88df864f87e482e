"""The add-on's device path with scene.curved_space_mesh_instances = 1 on the stub bpy: two linked
duplicates of a textured cube become two instances of one mesh -- the buffer is an _ffi.Frame's given the same mesh and instances
by hand, moved objects set no mesh again, and the image is the concatenated path's to the accuracy of float32 matrices."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_bpy_mesh as fbm  # noqa: E402
import mesh_instance_cases as mi  # noqa: E402
from test_mesh_material_host import BH_LOC, mesh_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, S = 64, 48, 2
CAMERA = (BH_LOC[0] + 1e-4, BH_LOC[1], BH_LOC[2] + 30.0)
SCALE = (1.2, 0.6, 1.0)


def _world(axis, angle, t):
    m = np.eye(4)
    m[:3, :3] = mi.rotation(axis, angle) * np.asarray(SCALE)
    m[:3, 3] = t
    return m.astype(np.float32).astype(np.float64)           # as Blender keeps it


WORLDS = [_world((0.0, 0.0, 1.0), 0.6, (3.5, -0.5, 8.0)), _world((1.0, 0.5, 0.2), -0.8, (-2.0, -2.5, 6.0))]
MOVED = [_world((0.0, 0.0, 1.0), 0.9, (3.2, -0.2, 8.0)), _world((1.0, 0.5, 0.2), -0.5, (-2.3, -2.5, 6.4))]


def _render(addon, depsgraph):
    eng = addon.RelativisticRenderEngine()
    eng.render(depsgraph)
    return eng, np.array(eng.result.layers[0].passes["Combined"].rect, dtype=np.float32).reshape(H, W, 4)


def _scene(instances):
    bpy, depsgraph, addon, cube, tetra = mesh_scene(WORLDS[0], WORLDS[1], width=W, height=H, samples=S, camera=CAMERA, device_shading=1.0,
                                                    curved_space_meshes=1.0, curved_space_mesh_instances=instances, render_devices=1.0)
    copy = fbm.MeshObject(cube._mesh, WORLDS[1], curved_space_texture="crate.png")      # a linked duplicate in the tetrahedron's place
    cube.data = copy.data = cube._mesh
    depsgraph.scene.objects[:] = [copy if ob is tetra else ob for ob in depsgraph.scene.objects]
    return bpy, depsgraph, addon, cube, copy


def test_addon_renders_linked_duplicates_as_instances(ctx, monkeypatch):
    from blackhole_geodesic_calculator_amd import _ffi as f
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    monkeypatch.setenv("BHGEO_DEVICES", "0")
    calls = []
    real_mesh, real_inst = f.Frame.set_mesh, f.Frame.set_mesh_instances
    monkeypatch.setattr(f.Frame, "set_mesh", lambda self, *a, **kw: (calls.append("mesh"), real_mesh(self, *a, **kw))[1])
    monkeypatch.setattr(f.Frame, "set_mesh_instances", lambda self, *a, **kw: (calls.append("instances"), real_inst(self, *a, **kw))[1])
    bpy, depsgraph, addon, cube, copy = _scene(1.0)
    addon.register()
    eng, image = _render(addon, depsgraph)
    assert calls == ["mesh", "instances"]
    m = eng.scene_mesh(depsgraph)
    assert m["instances"].shape == (2, 12) and m["vertices"].shape == (8, 3)
    # moved objects: the kept frame, the records alone
    cube.matrix_world, copy.matrix_world = MOVED
    eng2, moved = _render(addon, depsgraph)
    assert calls == ["mesh", "instances", "instances"] and eng2.device_frame_reused and np.abs(moved - image).max() > 1e-3
    m2 = eng2.scene_mesh(depsgraph)
    params = eng.GeoInt.params(eng.max_integration_step, eng.int_depth_curve_end)
    lamps = [[*(np.array([9.0, -6.0, 8.0]) - BH_LOC), eng.LAMP_INTENSITY]]
    sky, crate = bpy.data.images["sky.png"].array, bpy.data.images["crate.png"].array
    addon.unregister()
    # the same mesh and instances by hand
    fr = f.Frame([0], W, H, S, fov_x=0.6, fov_y=0.6, origin=np.array(CAMERA) - BH_LOC, rot=euler_xyz_matrix((0.0, 0.0, 0.0)),
                 jitter=python_random_stream(42.0, 2 * S * W * H))
    fr.set_scene(sky, lamps=lamps)
    plain = fr.render(params)
    fr.set_mesh(m["vertices"], m["triangles"], material=f.MeshMaterial(tri_uv=m["tri_uv"], tri_tex=m["tri_tex"], textures=[crate]))
    fr.set_mesh_instances(m["instances"])
    by_hand = fr.render(params)
    assert (np.abs(by_hand - plain).max(-1) > 1e-3).sum() > 100                       # both objects are in view
    assert np.array_equal(image, by_hand)
    fr.set_mesh_instances(m2["instances"])
    assert np.array_equal(moved, fr.render(params))
    fr.close()
    # the concatenated path on the same scene: the same picture, but for what float32 matrices and world arithmetic move
    calls.clear()
    bpy, depsgraph, addon, cube, copy = _scene(0.0)
    addon.register()
    _, flat = _render(addon, depsgraph)
    addon.unregister()
    assert calls == ["mesh"]
    differ = np.abs(flat - image).max(-1) > 1e-4
    print(f"instanced against concatenated: {int(differ.sum())} of {W * H} pixels differ by more than 1e-4, worst {np.abs(flat - image).max():.2e}")
    assert differ.mean() <= 0.01

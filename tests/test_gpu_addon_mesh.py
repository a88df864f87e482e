"""The add-on's device path with scene.curved_space_meshes = 1 on the stub bpy: the buffer it fills is an
_ffi.Frame's given the same arrays by hand, an unchanged scene sets no mesh again, two contexts of the device give the same image."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_bpy_mesh as fbm  # noqa: E402
from test_mesh_material_host import BH_LOC, mesh_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, S = 64, 48, 2
CAMERA = (BH_LOC[0] + 1e-4, BH_LOC[1], BH_LOC[2] + 30.0)
CUBE_W = fbm.world((1.2, 0.6, 1.0), 0.6, (3.5, -0.5, 8.0))
TETRA_W = fbm.world((0.9, 0.9, 0.9), -0.3, (-2.0, -2.5, 6.0))


def _render(addon, depsgraph):
    eng = addon.RelativisticRenderEngine()
    eng.render(depsgraph)
    return eng, np.array(eng.result.layers[0].passes["Combined"].rect, dtype=np.float32).reshape(H, W, 4)


def test_addon_renders_the_scene_mesh(ctx, monkeypatch):
    from blackhole_geodesic_calculator_amd import _ffi as f
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    calls = []
    real = f.Frame.set_mesh
    monkeypatch.setattr(f.Frame, "set_mesh", lambda self, *a, **kw: (calls.append(a[:1]), real(self, *a, **kw))[1])
    images = {}
    for devs in ("0", "0,0"):
        monkeypatch.setenv("BHGEO_DEVICES", devs)
        bpy, depsgraph, addon, cube, tetra = mesh_scene(CUBE_W, TETRA_W, width=W, height=H, samples=S, camera=CAMERA,
                                                        device_shading=1.0, curved_space_meshes=1.0,
                                                        render_devices=float(len(devs.split(","))))
        addon.register()
        calls.clear()
        eng, images[devs] = _render(addon, depsgraph)
        assert len(calls) == 1 and eng.last_device_frame["n_devices"] == len(devs.split(","))
        assert not eng.last_device_frame["directions_only"]
        # the unchanged scene a second time: the kept frame, no mesh set, the same image
        eng2, second = _render(addon, depsgraph)
        assert len(calls) == 1 and eng2.device_frame_reused and np.array_equal(second, images[devs])
        if devs == "0":
            m = eng.scene_mesh(depsgraph)
            params = eng.GeoInt.params(eng.max_integration_step, eng.int_depth_curve_end)
            lamps = [[*(np.array([9.0, -6.0, 8.0]) - BH_LOC), eng.LAMP_INTENSITY]]
            sky = bpy.data.images["sky.png"].array
            crate = bpy.data.images["crate.png"].array
        addon.unregister()
    assert np.array_equal(images["0"], images["0,0"])
    # the same arrays by hand
    fr = f.Frame([0], W, H, S, fov_x=0.6, fov_y=0.6, origin=np.array(CAMERA) - BH_LOC, rot=euler_xyz_matrix((0.0, 0.0, 0.0)),
                 jitter=python_random_stream(42.0, 2 * S * W * H))
    fr.set_scene(sky, lamps=lamps)
    plain = fr.render(params)
    fr.set_mesh(m["vertices"], m["triangles"], material=f.MeshMaterial(tri_uv=m["tri_uv"], tri_tex=m["tri_tex"], textures=[crate],
                                                                       emission=0.5))
    by_hand = fr.render(params)
    fr.close()
    changed = np.abs(by_hand - plain).max(-1) > 1e-3
    assert changed.sum() > 100                       # both objects are in view
    assert np.array_equal(images["0"], by_hand)

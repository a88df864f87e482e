"""The add-on's device path with scene.curved_space_mesh_refit = 1 on the stub bpy: a three-frame animation
of a waving plate renders the images of the switch-off path bit for bit, and the library saw one create and two refits."""
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
CELLS = 8
PLATE_W = fbm.world((1.0, 1.0, 1.0), 0.4, (2.5, -1.5, 7.0))


def _plate_vertices(phase):
    g = np.linspace(-2.5, 2.5, CELLS + 1)
    return [(x, y, 0.5 * np.sin(1.3 * x + 0.7 * y + phase)) for y in g for x in g]


def _plate(phase, smooth):
    n = CELLS + 1
    polys = [(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i) for j in range(CELLS) for i in range(CELLS)]
    uv = np.array([(i / CELLS, j / CELLS) for p in polys for k in p for i, j in [(k % n, k // n)]], np.float32)
    return fbm.MeshObject(fbm.FakeMesh(_plate_vertices(phase), polys, uv, smooth=smooth), PLATE_W, curved_space_texture="crate.png",
                          curved_space_emission=0.2)


def _render(addon, depsgraph):
    eng = addon.RelativisticRenderEngine()
    eng.render(depsgraph)
    return eng, np.array(eng.result.layers[0].passes["Combined"].rect, dtype=np.float32).reshape(H, W, 4)


@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "smooth"])
@pytest.mark.parametrize("devs", ["0", "0,0"])
def test_a_waving_plate_renders_the_switch_off_images(ctx, monkeypatch, devs, smooth):
    from blackhole_geodesic_calculator_amd import _ffi as f
    monkeypatch.setenv("BHGEO_DEVICES", devs)
    calls = []
    real = f.Frame.set_mesh
    monkeypatch.setattr(f.Frame, "set_mesh", lambda self, *a, **kw: (calls.append(a[:1]), real(self, *a, **kw))[1])
    images, actions, generations = {}, {}, {}
    for switch in (0.0, 1.0):
        bpy, depsgraph, addon, cube, tetra = mesh_scene(width=W, height=H, samples=S, camera=CAMERA, device_shading=1.0,
                                                        curved_space_meshes=1.0, curved_space_mesh_refit=switch,
                                                        render_devices=float(len(devs.split(","))))
        addon.register()
        addon.release_device_frames()       # (no frame of an earlier test under the same key)
        calls.clear()
        others = [ob for ob in depsgraph.scene.objects if ob is not cube and ob is not tetra]
        images[switch], actions[switch] = [], []
        for frame in range(3):
            depsgraph.scene.objects[:] = [_plate(0.9 * frame, smooth), *others]
            eng, img = _render(addon, depsgraph)
            images[switch].append(img)
            actions[switch].append(eng.device_mesh_action)
            assert eng.device_frame_reused == (frame > 0)
        (fr,) = addon._DEVICE_FRAMES.values()
        generations[switch] = [fr.mesh_refit_info(k)[0] for k in range(len(devs.split(",")))]
        assert len(calls) == (3 if switch == 0.0 else 1)
        addon.unregister()
    assert actions[0.0] == ["set", "set", "set"] and actions[1.0] == ["set", "refit", "refit"]
    # the library: three creates without the switch, one create and two refits on every device with it
    assert set(generations[0.0]) == {0} and set(generations[1.0]) == {2}
    for a, b in zip(images[0.0], images[1.0]):
        assert np.array_equal(a, b)
    moved = np.abs(images[0.0][0] - images[0.0][2]).max(-1) > 1e-3
    assert moved.sum() > 100        # the plate is in view and it waves

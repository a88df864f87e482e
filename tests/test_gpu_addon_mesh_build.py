"""The add-on's device path with scene.curved_space_mesh_build = 1 on the stub bpy: three frames of a plate
subdivided 4 x 4, 6 x 6 and 5 x 5 -- another triangle list, vertex count and UV array each frame -- render the images of the
switch-off path bit for bit, and every device did one create and two rebuilds in place."""
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
PLATE_W = fbm.world((1.0, 1.0, 1.0), 0.4, (2.5, -1.5, 7.0))
CELLS = (4, 6, 5)


def _plate(cells, smooth):
    n = cells + 1
    g = np.linspace(-2.5, 2.5, n)
    verts = [(x, y, 0.5 * np.sin(1.3 * x + 0.7 * y)) for y in g for x in g]
    polys = [(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i) for j in range(cells) for i in range(cells)]
    uv = np.array([(i / cells, j / cells) for p in polys for k in p for i, j in [(k % n, k // n)]], np.float32)
    return fbm.MeshObject(fbm.FakeMesh(verts, polys, uv, smooth=smooth), PLATE_W, curved_space_texture="crate.png", curved_space_emission=0.2)


def _render(addon, depsgraph):
    eng = addon.RelativisticRenderEngine()
    eng.render(depsgraph)
    return eng, np.array(eng.result.layers[0].passes["Combined"].rect, dtype=np.float32).reshape(H, W, 4)


@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "smooth"])
@pytest.mark.parametrize("devs", ["0", "0,0"])
def test_a_resubdivided_plate_renders_the_switch_off_images(ctx, monkeypatch, devs, smooth):
    monkeypatch.setenv("BHGEO_DEVICES", devs)
    n_dev = len(devs.split(","))
    images, actions, infos = {}, {}, {}
    for switch in (0.0, 1.0):
        bpy, depsgraph, addon, cube, tetra = mesh_scene(width=W, height=H, samples=S, camera=CAMERA, device_shading=1.0,
                                                        curved_space_meshes=1.0, curved_space_mesh_build=switch,
                                                        render_devices=float(n_dev))
        addon.register()
        addon.release_device_frames()       # (no frame of an earlier test under the same key)
        others = [ob for ob in depsgraph.scene.objects if ob is not cube and ob is not tetra]
        images[switch], actions[switch] = [], []
        for cells in CELLS:
            depsgraph.scene.objects[:] = [_plate(cells, smooth), *others]
            eng, img = _render(addon, depsgraph)
            images[switch].append(img)
            actions[switch].append(eng.device_mesh_action)
        (fr,) = addon._DEVICE_FRAMES.values()
        infos[switch] = [fr.mesh_build_info(k) for k in range(n_dev)]
        addon.unregister()
    assert actions[0.0] == ["set", "set", "set"] and actions[1.0] == ["set", "rebuild", "rebuild"]
    # the library: three host builds without the switch; with it one create on the device (for four times the first plate's counts,
    # which holds the other two) and two rebuilds in place, on every device
    first = 2 * CELLS[0] ** 2
    assert 2 * max(CELLS) ** 2 <= 4 * first
    for info in infos[0.0]:
        assert not info["built_on_device"] and info["builds"] == 1
    for info in infos[1.0]:
        assert info["built_on_device"] and info["builds"] == 3 and info["allocations"] == 3 and info["cap_triangles"] >= 4 * first
    for a, b in zip(images[0.0], images[1.0]):
        assert np.array_equal(a, b)
    changed = np.abs(images[0.0][0] - images[0.0][1]).max(-1) > 1e-4
    assert changed.sum() > 0         # the plate is in view, and its subdivision shows

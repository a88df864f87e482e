"""Meshes on the library-owned frame (bhg_frame_set_mesh): every gather mode gives DeviceFrame's image, the
mesh turned off gives the frame that never had one, the observer camera, rebalance, the refused combinations."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_material_cases as mmc  # noqa: E402

pytestmark = pytest.mark.gpu


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


def _device_frame_image(ctx, p, disk, observer=None):
    import torch
    f = _ffi()
    V, F = mmc.SHADE_MESH
    dfr = mmc.device_frame(ctx, mmc.FRAME_S, mmc.FRAME_W, mmc.FRAME_H, mmc.FRAME_FOV, disk=disk, sampling_seed=42.0)
    mesh = f.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals())
    dfr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**mmc.material_arrays()))
    if observer is not None:
        dfr.set_observer(observer)
    dfr.generate_rays(p)
    dfr.trace(p)
    out = torch.empty((dfr.P, 4), dtype=torch.float32, device=dfr.dev)
    dfr.shade_f32(out)
    torch.cuda.synchronize()
    img = out.cpu().numpy().reshape(mmc.FRAME_H, mmc.FRAME_W, 4)
    on_mesh = ((dfr.d_flags == 0x88) & (dfr.d_tri_id >= 0)).sum().item()
    mesh.close()
    return img, on_mesh


_RCCL_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from blackhole_geodesic_calculator_amd import _ffi as f
import mesh_material_cases as mmc
try:
    fr = mmc.frame(f, [0], f.GATHER_RCCL)
except f.BhgError as e:
    print("RCCL unavailable:", e)
    sys.exit(0)
mmc.set_frame_mesh(f, fr)
img = fr.render(mmc.frame_params(f))
assert fr.info()["gather"] == "rccl", fr.info()
np.save(%(out)r, img)
fr.close()
print("rccl mesh frame ok")
"""


@pytest.mark.parametrize("case", ["disk", "no_disk", "kerr09"])
def test_every_gather_mode_gives_device_frames_image(ctx, case, tmp_path):
    f = _ffi()
    disk, kerr = case == "disk", case == "kerr09"
    p = mmc.frame_params(f, disk=disk, kerr=kerr)
    images = {}
    for name, devs, gather in (("one", [0], f.GATHER_AUTO), ("copy", [0, 0], f.GATHER_COPY),
                               ("peercall", [0, 0], f.GATHER_COPY_PEERCALL), ("peer", [0, 0], f.GATHER_PEER)):
        try:
            fr = mmc.frame(f, devs, gather, disk=disk)
        except f.BhgError as e:
            print(f"gather mode {name} is not available here: {e}")
            continue
        mmc.set_frame_mesh(f, fr)
        images[name] = fr.render(p)
        info = fr.info()
        assert info["n_devices"] == len(devs) and not info["directions_only"]
        fr.close()
    assert "one" in images and len(images) >= 2
    for name, img in images.items():
        assert np.array_equal(img, images["one"]), name
    want, on_mesh = _device_frame_image(ctx, p, disk)
    assert on_mesh > 200
    assert np.array_equal(images["one"], want)
    if case == "disk":
        # the RCCL loopback, in a child process as the frame's own RCCL test runs it
        out = tmp_path / "rccl.npy"
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run([sys.executable, "-c", _RCCL_CHILD % dict(root=ROOT, out=str(out))], capture_output=True, text=True,
                           timeout=150, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        if "RCCL unavailable" in r.stdout:
            print(r.stdout)
        else:
            assert "rccl mesh frame ok" in r.stdout and np.array_equal(np.load(out), images["one"])


def test_mesh_off_is_the_frame_that_never_had_one(ctx):
    f = _ffi()
    p = mmc.frame_params(f)
    V, F = mmc.SHADE_MESH
    for devs in ([0], [0, 0]):
        fr = mmc.frame(f, devs, f.GATHER_AUTO if len(devs) == 1 else f.GATHER_COPY)
        plain = fr.render(p)
        plain_stats = fr.stats()
        mmc.set_frame_mesh(f, fr)
        with_mesh = fr.render(p)
        assert np.abs(with_mesh - plain).max() > 1e-3
        mesh_stats = fr.stats()
        assert mesh_stats["rays"] == plain_stats["rays"] and mesh_stats["attempted_steps"] < plain_stats["attempted_steps"]
        # a refused set_mesh leaves the frame rendering what it rendered
        bad_f = F.copy()
        bad_f[7, 1] = len(V)
        with pytest.raises(f.BhgError, match="triangle index"):
            fr.set_mesh(V, bad_f, material=f.MeshMaterial(**mmc.material_arrays()))
        bad = mmc.material_arrays()
        bad["tri_uv"][4, 0, 1] = np.nan
        with pytest.raises(f.BhgError, match="tri_uv"):
            fr.set_mesh(V, F, material=f.MeshMaterial(**bad))
        Vc, Fc = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
        with pytest.raises(f.BhgError, match="max_chord"):
            f._check(f.load().bhg_frame_set_mesh(fr._h, f._addr(Vc), len(Vc), f._addr(Fc), len(Fc), None, 4, -1.0, None))
        assert np.array_equal(fr.render(p), with_mesh)
        # rebalance after a mesh render: the tiles dealt by the mesh trace's cost, the image unchanged
        fr.rebalance()
        assert np.array_equal(fr.render(p), with_mesh)
        # off: the plain render, bit for bit, and its statistics
        fr.set_mesh(None)
        again = fr.render(p)
        never = mmc.frame(f, devs, f.GATHER_AUTO if len(devs) == 1 else f.GATHER_COPY)
        assert np.array_equal(again, plain) and np.array_equal(never.render(p), again)
        assert fr.stats() == plain_stats == never.stats()
        never.close()
        fr.close()


def test_observer_and_profiling_with_a_mesh(ctx):
    f = _ffi()
    p = mmc.frame_params(f)
    beta = (0.0, 0.3, 0.1)
    fr = mmc.frame(f, [0, 0], f.GATHER_COPY)
    mmc.set_frame_mesh(f, fr)
    still = fr.render(p)
    fr.set_observer(beta)
    fr.set_profiling(True)
    moving = fr.render(p)
    tr, root = fr.last_ms()
    assert len(tr) == 2 and all(t > 0.0 for t in tr) and root > 0.0
    assert not np.array_equal(moving, still)
    want, on_mesh = _device_frame_image(ctx, p, True, observer=beta)
    assert on_mesh > 100 and np.array_equal(moving, want)
    fr.close()


def test_refused_combinations(ctx):
    f = _ffi()
    p = mmc.frame_params(f)
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    sky = synthetic_sky(128, 64)
    sphere = [[0.0, -6.0, 1.0, 1.0]]

    def spheres(fr):
        fr.set_scene(sky, disk=mmc.SHADE_DISK, spheres=sphere, lamps=mmc.SHADE_LAMPS)

    def motion(fr):
        spheres(fr)
        fr.set_object_motion(velocity=[[0.0, 0.1, 0.0]])
        fr.set_scene(sky, disk=mmc.SHADE_DISK, lamps=mmc.SHADE_LAMPS)

    def textures(fr):
        spheres(fr)
        fr.set_object_textures(emission=[1.0], modes=["emissive"])
        fr.set_scene(sky, disk=mmc.SHADE_DISK, lamps=mmc.SHADE_LAMPS)

    for name, setup in (("scene spheres", spheres), ("redshift", lambda fr: fr.set_redshift(("disk", "sky"), 4.0, 1)),
                        ("the thermal disk", lambda fr: fr.set_disk_thermal(f.make_disk_thermal(1e7, *f.narrowband(1e17, 2e17, 3e17)))),
                        ("object motion", motion), ("object textures", textures)):
        fr = mmc.frame(f, [0], f.GATHER_AUTO)
        mmc.set_frame_mesh(f, fr)
        good = fr.render(p)
        setup(fr)
        with pytest.raises(f.BhgError, match="a mesh does not go with " + name):
            fr.render(p)
        # nothing was enqueued: the device image is the last render's still
        fr.set_mesh(None)
        fr.set_scene(sky, disk=mmc.SHADE_DISK, lamps=mmc.SHADE_LAMPS)
        fr.set_redshift(None)
        fr.set_disk_thermal(None)
        fr.set_object_motion()
        fr.set_object_textures()
        mmc.set_frame_mesh(f, fr)
        assert np.array_equal(fr.render(p), good), name
        fr.close()

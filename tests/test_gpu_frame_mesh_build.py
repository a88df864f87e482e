"""The device-side mesh build on the frames (bhg_frame_set_mesh_build, DeviceFrame.rebuild_mesh): with the
switch on every image is the host-built frame's with a difference of 0 -- in every gather mode available, on two contexts of one
device, with and without instances and a material; a second set_mesh with another topology within the capacity rebuilds in place;
refit_mesh with rebuild_ratio = 1 rebuilds on the device; and DeviceFrame.rebuild_mesh is a fresh DeviceFrame."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_instance_cases as mi  # noqa: E402
import mesh_material_cases as mmc  # noqa: E402
import mesh_refit_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = (("one", [0], "GATHER_AUTO"), ("copy", [0, 0], "GATHER_COPY"), ("peercall", [0, 0], "GATHER_COPY_PEERCALL"),
         ("peer", [0, 0], "GATHER_PEER"))
T = np.stack([mi.record(np.eye(3), (0.0, 0.0, 0.0)), mi.record(mi.rotation((0.2, 1.0, -0.4), 0.8), (1.5, -6.0, 1.0))])
INST_RGB = np.array([[1.0, 0.8, 0.6], [0.5, 0.9, 1.0]], np.float32)


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


def _normals(V):
    n = V - V.mean(0)
    return n / np.linalg.norm(n, axis=1)[:, None]


def _material(f, keep=None):
    """the shade material, or its rows for the triangles `keep`"""
    arrays = mmc.material_arrays()
    if keep is not None:
        for k in ("tri_rgb", "tri_uv", "tri_tex"):
            arrays[k] = np.ascontiguousarray(arrays[k][keep])
    return f.MeshMaterial(**arrays)


def _meshes():
    """name -> (V, F, N, the triangles kept): the shade mesh; another topology within its counts -- every other triangle, the list
    turned round, the vertices twisted; and the shade mesh with the twisted vertices"""
    V, F = mmc.SHADE_MESH
    keep = np.arange(len(F))[::-2].copy()
    Vt = rc.deform(V, "twist")
    return {"full": (V, F, mmc.vertex_normals(), None), "thinned": (Vt, np.ascontiguousarray(F[keep]), _normals(Vt), keep),
            "twisted": (Vt, F, _normals(Vt), None)}


def _set(f, fr, name, material=True, instances=False):
    V, F, N, keep = _meshes()[name]
    fr.set_mesh(V, F, vertex_normals=N, chord=mmc.CHORD, material=_material(f, keep) if material else None)
    if instances:
        fr.set_mesh_instances(T, INST_RGB)


VARIANTS = [(name, material, instances) for name in ("full", "thinned") for material in (True, False) for instances in (False, True)]


@pytest.fixture(scope="module")
def wanted():
    """(mesh, material, instances) -> the image of a one-device frame with the HOST build: computed once."""
    f = _ffi()
    p = mmc.frame_params(f)
    out = {}
    fr = mmc.frame(f, [0], f.GATHER_AUTO)
    for name, material, instances in VARIANTS + [("twisted", True, False)]:
        _set(f, fr, name, material, instances)
        out[name, material, instances] = fr.render(p).copy()
        assert fr.mesh_build_info(0)["built_on_device"] is False
    fr.close()
    assert len({a.tobytes() for a in out.values()}) == len(out)
    return out


def test_device_built_frames_give_the_host_built_image(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    seen = 0
    for mode, devs, gather in MODES:
        try:
            fr = mmc.frame(f, devs, getattr(f, gather))
        except f.BhgError as e:
            print(f"gather mode {mode} is not available here: {e}")
            continue
        seen += 1
        fr.set_mesh_build(True)
        full = len(mmc.SHADE_MESH[1])
        allocations = 0
        for g, (name, material, instances) in enumerate(VARIANTS):
            _set(f, fr, name, material, instances)
            assert np.abs(fr.render(p) - wanted[name, material, instances]).max() == 0.0, (mode, name, material, instances)
            for k in range(len(devs)):
                info = fr.mesh_build_info(k)
                # the first mesh is created on the device, at the full counts; every later one fits and rebuilds it in place
                assert info["built_on_device"] and info["cap_triangles"] == 4 * full and info["builds"] == g + 1, (mode, g, info)
                allocations = info["allocations"]
        assert allocations == 3
        fr.close()
    assert seen >= 2


def test_set_mesh_again_rebuilds_in_place_and_equals_a_fresh_frame(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    fr = mmc.frame(f, [0, 0], f.GATHER_COPY)
    _set(f, fr, "full")
    fr.set_mesh_build(True)            # (after set_mesh, before the first render: the devices hold nothing yet)
    assert np.array_equal(fr.render(p), wanted["full", True, False])
    first = [fr.mesh_build_info(k) for k in (0, 1)]
    assert all(i["built_on_device"] and i["builds"] == 1 for i in first)
    _set(f, fr, "thinned")
    got = fr.render(p).copy()
    fresh = mmc.frame(f, [0, 0], f.GATHER_COPY)
    _set(f, fresh, "thinned")
    assert np.array_equal(got, fresh.render(p)) and np.array_equal(got, wanted["thinned", True, False])
    # a rebuild and not a create: one more build of the same mesh, no allocation
    assert [fr.mesh_build_info(k) for k in (0, 1)] == [dict(i, builds=2) for i in first]
    assert fresh.mesh_build_info(0)["built_on_device"] is False
    fresh.close()
    # a frame's mesh is created with room for BHG_FRAME_MESH_HEADROOM = 4 times its counts; a mesh over that is created anew, on
    # the device: the tetrahedron alone (4 triangles, 4 vertices), then the whole mesh (132 and 70)
    V, F = mmc.SHADE_MESH
    small = mmc.frame(f, [0], f.GATHER_AUTO)
    small.set_mesh_build(True)
    small.set_mesh(np.ascontiguousarray(V[-4:]), np.ascontiguousarray(F[-4:] - (len(V) - 4)), chord=mmc.CHORD)
    small.render(p)
    info = small.mesh_build_info(0)
    assert (info["cap_vertices"], info["cap_triangles"], info["builds"]) == (16, 16, 1) and len(F) > 16
    _set(f, small, "full")
    assert np.array_equal(small.render(p), wanted["full", True, False])
    info = small.mesh_build_info(0)
    assert info["built_on_device"] and info["builds"] == 1 and info["cap_triangles"] == 4 * len(F)
    small.close()
    # switched off again: the host builder, a new mesh
    fr.set_mesh_build(False)
    _set(f, fr, "full")
    assert np.array_equal(fr.render(p), wanted["full", True, False])
    V, F = mmc.SHADE_MESH
    assert fr.mesh_build_info(0) == dict(built_on_device=False, builds=1, cap_vertices=len(V), cap_triangles=len(F), allocations=1)
    with pytest.raises(f.BhgError, match="leaf_size"):
        fr.set_mesh(*mmc.SHADE_MESH, leaf_size=65, build="device")
    fr.close()


def test_refit_with_rebuild_ratio_1_rebuilds_on_the_device(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    V, F, N, _ = _meshes()["twisted"]
    for instances in (False, True):
        fr = mmc.frame(f, [0, 0], f.GATHER_COPY)
        fr.set_mesh_build(True)
        _set(f, fr, "full", instances=instances)
        fr.render(p)
        fr.refit_mesh(V, N, rebuild_ratio=1.0)
        got = fr.render(p).copy()
        for k in (0, 1):
            info = fr.mesh_build_info(k)
            assert info["built_on_device"] and info["builds"] == 2 and info["allocations"] == 3
            assert fr.mesh_refit_info(k)[0] == 1 and fr.mesh_refit_info(k)[1] == fr.mesh_refit_info(k)[2]
        host = mmc.frame(f, [0, 0], f.GATHER_COPY)
        _set(f, host, "twisted", instances=instances)
        assert np.array_equal(got, host.render(p))
        if not instances:
            assert np.array_equal(got, wanted["twisted", True, False])
        host.close()
        # and a ratio that asks for a refit still refits the device-built tree
        V0, _, N0, _ = _meshes()["full"]
        fr.refit_mesh(V0, N0, rebuild_ratio=0.0)
        fr.render(p)
        assert fr.mesh_build_info(0)["builds"] == 2 and fr.mesh_refit_info(0)[0] == 2
        fr.close()


def test_device_frame_rebuild_is_a_fresh_device_frame(ctx):
    import torch
    f = _ffi()
    p = mmc.frame_params(f)
    meshes = _meshes()
    full = len(mmc.SHADE_MESH[1])
    for instances in (None, T):
        for build in ("device", "host"):
            V, F, N, _ = meshes["full"]
            a = mmc.device_frame(ctx, 2)
            mesh = f.Mesh(ctx, V, F, vertex_normals=N, build=build)
            a.set_mesh(mesh, chord=mmc.CHORD, material=_material(f), instances=instances)
            first = a.render(p).cpu().numpy().copy()
            with pytest.raises(ValueError, match="give material="):
                a.rebuild_mesh(*meshes["thinned"][:3])
            assert np.array_equal(a.render(p).cpu().numpy(), first)
            for name, on_device in (("thinned", False), ("twisted", True)):
                V, F, N, keep = meshes[name]
                if on_device:
                    a.rebuild_mesh(torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda(), torch.as_tensor(N).cuda(), material=_material(f, keep))
                else:
                    a.rebuild_mesh(V, F, N, material=_material(f, keep))
                got = a.render(p).cpu().numpy().copy()
                b = mmc.device_frame(ctx, 2)
                fresh = f.Mesh(ctx, V, F, vertex_normals=N)
                b.set_mesh(fresh, chord=mmc.CHORD, material=_material(f, keep), instances=instances)
                want = b.render(p).cpu().numpy().copy()
                assert np.array_equal(got, want) and not np.array_equal(got, first), (name, build, instances is not None)
                for key in ("d_end", "d_flags", "d_tri_id", "d_steps"):
                    assert torch.equal(getattr(a, key), getattr(b, key)), key
                hit = a.d_tri_id >= 0
                assert hit.sum().item() > 100 and torch.equal(a.d_bary[hit], b.d_bary[hit])
                fresh.close()
            info = mesh.build_info()
            assert info["built_on_device"] and info["builds"] == 3 and info["cap_triangles"] == full
            mesh.close()
    with pytest.raises(ValueError, match="set_mesh"):
        mmc.device_frame(ctx, 1).rebuild_mesh(*mmc.SHADE_MESH)
    # DeviceFrame.set_mesh(build=) and the integrator's mesh_build= take the arrays to the device build
    a = mmc.device_frame(ctx, 1)
    a.set_mesh(mmc.SHADE_MESH, chord=mmc.CHORD, build="device")
    assert a.mesh.build_info()["built_on_device"]
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild(mass=0.5, time_like=False, verbose=False, device=0)
    k0 = rc.trace_rays(256, 3)
    out = [gi.trace(k0, np.array(rc.mo.FRAME_CAM), curve_end=46.0, mesh=rc.trace_mesh(), mesh_build=b) for b in ("host", "device")]
    assert all(np.array_equal(out[0][k], out[1][k], equal_nan=True) for k in out[0]) and (out[0]["tri_id"] >= 0).sum() > 10

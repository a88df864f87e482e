"""Deforming meshes on the frames (bhg_frame_refit_mesh, DeviceFrame.refit_mesh): refit_mesh + render is
the render of a frame given set_mesh with the deformed vertices, bit for bit, in every gather mode the frame-mesh test walks and
with two contexts on one device; the rebuild ratio changes nothing in the image; frame instances need no further call; a refused
refit leaves the frame alone."""
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


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


def _normals(V):
    n = V - V.mean(0)
    return n / np.linalg.norm(n, axis=1)[:, None]


def _deformed(kind):
    V, F = mmc.SHADE_MESH
    Vn = rc.deform(V, kind)
    return Vn, _normals(Vn)


def _set(f, fr, V=None, N=None):
    fr.set_mesh(mmc.SHADE_MESH[0] if V is None else V, mmc.SHADE_MESH[1], vertex_normals=mmc.vertex_normals() if N is None else N,
                chord=mmc.CHORD, material=f.MeshMaterial(**mmc.material_arrays()))


@pytest.fixture(scope="module")
def wanted():
    """kind -> the image of a one-device frame given set_mesh with the deformed vertices: computed once."""
    f = _ffi()
    p = mmc.frame_params(f)
    out = {}
    fr = mmc.frame(f, [0], f.GATHER_AUTO)
    for kind in (None, "noise", "twist"):
        _set(f, fr, *(_deformed(kind) if kind else (None, None)))
        out[kind] = fr.render(p).copy()
    fr.close()
    assert not np.array_equal(out[None], out["noise"]) and not np.array_equal(out["noise"], out["twist"])
    return out


def test_refit_then_render_is_set_mesh_then_render(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    seen = 0
    for name, devs, gather in MODES:
        try:
            fr = mmc.frame(f, devs, getattr(f, gather))
        except f.BhgError as e:
            print(f"gather mode {name} is not available here: {e}")
            continue
        seen += 1
        # before any render: no device holds the mesh yet, the new vertices go up with the first upload
        _set(f, fr)
        fr.refit_mesh(*_deformed("noise"), rebuild_ratio=0.0)
        assert np.array_equal(fr.render(p), wanted["noise"]), name
        assert all(fr.mesh_refit_info(k)[0] == 0 for k in range(len(devs)))
        # after a render: every device refits
        for g, kind in enumerate(("twist", "noise", "twist")):
            fr.refit_mesh(*_deformed(kind), rebuild_ratio=0.0)
            assert np.abs(fr.render(p) - wanted[kind]).max() == 0.0, (name, kind)
            assert all(fr.mesh_refit_info(k)[0] == g + 1 for k in range(len(devs))), name
        fr.close()
    assert seen >= 2


def test_the_rebuild_ratio_changes_nothing_in_the_image(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    fr = mmc.frame(f, [0, 0], f.GATHER_COPY)
    _set(f, fr)
    fr.render(p)
    built = fr.mesh_refit_info(0)[1]
    # (the default, 1.5: the twist takes this tree's area sum to 1.64 times what it was -- rebuilt; the noise then takes the new
    # tree's to 0.91 -- refitted; both figures from bhg_mesh_bvh_refit_host)
    assert f.MESH_REBUILD_RATIO == 1.5
    for ratio, gens in ((0.0, (1, 2)), (1.0, (0, 0)), (1e9, (1, 2)), (None, (0, 1))):
        _set(f, fr)
        fr.render(p)
        for kind, gen in zip(("twist", "noise"), gens):
            fr.refit_mesh(*_deformed(kind), rebuild_ratio=ratio)
            assert np.array_equal(fr.render(p), wanted[kind]), ratio
            # never (0) and a ratio out of reach: refitted; always (1): built anew, generation 0 again
            assert [fr.mesh_refit_info(k)[0] for k in (0, 1)] == [gen, gen], ratio
    # a ratio the twisted tree exceeds: that device rebuilds, and its tree is the deformed mesh's own
    _set(f, fr)
    fr.render(p)
    g, area_build, area_now = fr.mesh_refit_info(0)
    assert (g, area_build, area_now) == (0, built, built)
    fr.refit_mesh(*_deformed("twist"), rebuild_ratio=0.0)
    fr.render(p)
    grown = fr.mesh_refit_info(0)[2] / built
    print(f"area_now / area_build after the twist: {grown:.4f}")
    assert grown > 1.0
    fr.refit_mesh(*_deformed("noise"), rebuild_ratio=0.0)
    fr.render(p)
    fr.refit_mesh(*_deformed("twist"), rebuild_ratio=0.5 * (1.0 + grown))
    assert np.array_equal(fr.render(p), wanted["twist"])
    assert fr.mesh_refit_info(0)[0] == 0 and fr.mesh_refit_info(0)[1] != built
    fr.close()


def test_frame_instances_need_no_further_call(ctx):
    f = _ffi()
    p = mmc.frame_params(f)
    V, F = mmc.SHADE_MESH
    T = np.stack([mi.record(np.eye(3), (0.0, 0.0, 0.0)), mi.record(mi.rotation((0.2, 1.0, -0.4), 0.8), (1.5, -6.0, 1.0))])
    rgb = np.array([[1.0, 0.8, 0.6], [0.5, 0.9, 1.0]], np.float32)
    Vn, Nn = _deformed("twist")
    images = []
    for refit in (True, False):
        fr = mmc.frame(f, [0, 0], f.GATHER_COPY)
        if refit:
            _set(f, fr)
            fr.set_mesh_instances(T, rgb)
            first = fr.render(p).copy()
            fr.refit_mesh(Vn, Nn)
        else:
            _set(f, fr, Vn, Nn)
            fr.set_mesh_instances(T, rgb)
        images.append(fr.render(p).copy())
        fr.close()
    assert np.array_equal(images[0], images[1]) and not np.array_equal(images[0], first)


def test_a_refused_refit_leaves_the_frame_alone(ctx, wanted):
    f = _ffi()
    p = mmc.frame_params(f)
    V, F = mmc.SHADE_MESH
    fr = mmc.frame(f, [0], f.GATHER_AUTO)
    Vn, Nn = _deformed("noise")
    with pytest.raises(ValueError, match="set_mesh"):
        fr.refit_mesh(Vn, Nn)
    Vc = np.ascontiguousarray(Vn)
    assert f.load().bhg_frame_refit_mesh(fr._h, f._addr(Vc), None, 0.0) == f.E_INVALID and b"holds no mesh" in f.load().bhg_last_error()
    _set(f, fr)
    out = np.full((mmc.FRAME_H, mmc.FRAME_W, 4), -7.25, np.float32)
    bad = Vn.copy()
    bad[3, 0] = np.nan
    bad_n = Nn.copy()
    bad_n[5, 2] = np.inf
    for args, what in (((bad, Nn), "every vertex must be finite"), ((Vn, bad_n), "every vertex normal must be finite"),
                       ((Vn, None), "created with them"), ((Vn, Nn, np.nan), "rebuild_ratio")):
        with pytest.raises(f.BhgError, match=what):
            fr.refit_mesh(*args)
    with pytest.raises(ValueError, match="shape"):
        fr.refit_mesh(Vn[:-1], Nn[:-1])
    assert np.all(out == -7.25)
    assert np.array_equal(fr.render(p, out=out), wanted[None]) and fr.mesh_refit_info(0)[0] == 0
    # ... after a render too, and a flat-shaded mesh refuses normals
    with pytest.raises(f.BhgError, match="every vertex must be finite"):
        fr.refit_mesh(bad, Nn)
    assert np.array_equal(fr.render(p), wanted[None]) and fr.mesh_refit_info(0)[0] == 0
    fr.set_mesh(V, F, chord=mmc.CHORD)
    with pytest.raises(f.BhgError, match="created without"):
        fr.refit_mesh(Vn, Nn)
    fr.close()


def test_device_frame_refit_is_set_mesh_with_a_fresh_mesh(ctx):
    import torch
    f = _ffi()
    p = mmc.frame_params(f)
    V, F = mmc.SHADE_MESH
    T = np.stack([mi.record(np.eye(3), (0.0, 0.0, 0.0)), mi.record(mi.rotation((0.2, 1.0, -0.4), 0.8), (1.5, -6.0, 1.0))])
    for instances in (None, T):
        a = mmc.device_frame(ctx, 2)
        mesh = f.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals())
        a.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**mmc.material_arrays()), instances=instances)
        first = a.render(p).cpu().numpy().copy()
        for kind, on_device in (("noise", False), ("twist", True)):
            Vn, Nn = _deformed(kind)
            if on_device:
                a.refit_mesh(torch.as_tensor(Vn).cuda(), torch.as_tensor(Nn).cuda())
            else:
                a.refit_mesh(Vn, Nn)
            got = a.render(p).cpu().numpy().copy()
            b = mmc.device_frame(ctx, 2)
            fresh = f.Mesh(ctx, Vn, F, vertex_normals=Nn)
            b.set_mesh(fresh, chord=mmc.CHORD, material=f.MeshMaterial(**mmc.material_arrays()), instances=instances)
            want = b.render(p).cpu().numpy().copy()
            assert np.array_equal(got, want) and not np.array_equal(got, first), (kind, instances is not None)
            for key in ("d_end", "d_flags", "d_tri_id", "d_steps"):
                assert torch.equal(getattr(a, key), getattr(b, key)), key
            hit = a.d_tri_id >= 0       # (a ray that hits nothing leaves its bary slot as it was)
            assert hit.sum().item() > 100 and torch.equal(a.d_bary[hit], b.d_bary[hit])
            fresh.close()
        assert mesh.refit_info()[0] == 2
        mesh.close()
    with pytest.raises(ValueError, match="set_mesh"):
        mmc.device_frame(ctx, 1).refit_mesh(V)

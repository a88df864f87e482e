"""Deforming meshes on the GPU: bhg_mesh_refit / bhg_mesh_refit_device against the host statement of the
kernels (boxes and slot records bit for bit), against a mesh created fresh from the deformed vertices (root box, distance range,
and -- the equality that matters -- every output of bhg_trace_mesh_device and both mesh shades, bit for bit, with the whole-step
cull on and off), against the brute-force oracle of section 19, and the refusals, determinism and the instance sets' generation
rule.  The meshes, deformations and rays are tests/mesh_refit_cases.py's; tests/test_mesh_refit_host.py checks on the CPU that
every trace case meets the mesh and that the oracle alone is stable on its cases.

Measured when this was written (MI355X): every equality holds bit for bit; against the oracle on the twisted mesh 71 / 71 / 49 / 53
stable hits (christoffel / reduced / kerr_plus / kerr_minus), no ray unstable, worst |end - oracle| 6.9e-12 / 6.9e-13 / 1.6e-11 /
7.9e-10, worst |bary - oracle| 2.2e-12 / 6.2e-13 / 2.1e-11 / 6.1e-10."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_cases as mc  # noqa: E402
import mesh_instance_cases as mi  # noqa: E402
import mesh_oracle_cases as mo  # noqa: E402
import mesh_refit_cases as rc  # noqa: E402

MESHES = rc.meshes()
TREES = [(name, leaf) for name in MESHES for leaf in MESHES[name][2]]
TREE_IDS = [f"{n}-leaf{k}" for n, k in TREES]


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in rc.KEYS)


def _normals(V):
    n = V - V.mean(0)
    return n / np.maximum(np.linalg.norm(n, axis=1), 1e-300)[:, None]


# ---- 1. a refit to the creation vertices changes nothing ----------------------------------------------------------------------
@pytest.mark.parametrize("name,leaf", TREES, ids=TREE_IDS)
def test_refit_to_the_creation_vertices(ctx, name, leaf):
    f = _ffi()
    V, F, _ = MESHES[name]
    mesh = f.Mesh(ctx, V, F, leaf_size=leaf)
    tree = f.mesh_bvh_host(V, F, leaf)
    box0, tri0 = mesh.download_boxes()
    info0, range0 = mesh.info(), mesh.distance_range()
    assert _same_bits(box0, tree["box"]) and _same_bits(tri0, rc.slot_records(V, F, tree))
    gen, built, now = mesh.refit_info()
    assert gen == 0 and built == now == f.mesh_bvh_refit_host(V, F, tree)[1]
    mesh.refit(V)
    box1, tri1 = mesh.download_boxes()
    assert _same_bits(box1, box0) and _same_bits(tri1, tri0)
    info1 = mesh.info()
    assert info1[:2] == info0[:2] and _same_bits(info1[2], info0[2]) and mesh.distance_range() == range0
    assert mesh.refit_info() == (1, built, built)       # (the device's area sum is the host's, in the host's order)
    mesh.close()


# ---- 2. a refit to deformed vertices: the host statement, and a mesh created fresh ----------------------------------------------
@pytest.mark.parametrize("name,leaf", TREES, ids=TREE_IDS)
def test_refit_to_deformed_vertices(ctx, name, leaf):
    f = _ffi()
    V, F, _ = MESHES[name]
    mesh = f.Mesh(ctx, V, F, leaf_size=leaf)
    tree = f.mesh_bvh_host(V, F, leaf)
    nn, depth, _ = mesh.info()
    for g, kind in enumerate(rc.DEFORMS):
        Vn = rc.deform(V, kind)
        mesh.refit(Vn)
        box, tri = mesh.download_boxes()
        want, area = f.mesh_bvh_refit_host(Vn, F, tree)
        assert _same_bits(box, want), kind
        assert _same_bits(tri, rc.slot_records(Vn, F, tree)), kind
        assert mesh.refit_info() == (g + 1, f.mesh_bvh_refit_host(V, F, tree)[1], area)
        fresh = f.Mesh(ctx, Vn, F, leaf_size=leaf)
        assert mesh.info()[:2] == (nn, depth) and _same_bits(mesh.info()[2], fresh.info()[2]), kind
        assert mesh.distance_range() == fresh.distance_range(), kind
        fresh.close()
    mesh.close()


# ---- 3. the equality that matters: the trace ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh_traces(ctx):
    """Every trace case on a mesh created fresh from the deformed vertices (the whole-step cull on): computed once."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0"
    f = _ffi()
    V, F = rc.trace_mesh()
    k0 = rc.trace_rays()
    res = {}
    for name, (rhs, a, par, kind) in rc.trace_cases().items():
        mesh = f.Mesh(ctx, rc.deform(V, kind), F)
        r = mc.trace_mesh_device(ctx, f.make_params(rhs_form=rhs, spin=a, **par), mesh, rc.CHORD, k0, mo.FRAME_CAM)
        mesh.close()
        for key, arr in r.items():
            res[f"{name}__{key}"] = arr
    return res


def test_trace_on_the_refitted_mesh_is_the_fresh_mesh_trace(ctx, fresh_traces):
    got = rc.run_refitted(ctx)
    assert sorted(got) == sorted(fresh_traces)
    for name in rc.trace_cases():
        hits = int((fresh_traces[f"{name}__tri"] >= 0).sum())
        assert hits >= rc.MIN_HITS, (name, hits)
        for key in rc.KEYS:
            assert np.array_equal(got[f"{name}__{key}"], fresh_traces[f"{name}__{key}"]), (name, key)
    disk = sum(int((fresh_traces[f"{n}__flags"] == 128).sum()) for n in rc.trace_cases())
    leave = sum(int((fresh_traces[f"{n}__flags"] == 8).sum()) for n in rc.trace_cases())
    assert disk > 100 and leave > 100


def test_trace_without_the_cull(fresh_traces, tmp_path):
    out = str(tmp_path / "refit_nocull.npz")
    env = dict(os.environ, BHGEO_MESH_CULL="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_refit_cases.py"), out], check=True, env=env, timeout=300)
    plain = np.load(out)
    assert sorted(plain.files) == sorted(fresh_traces)
    for k in plain.files:
        assert np.array_equal(plain[k], fresh_traces[k]), k


# ---- 4. the shades --------------------------------------------------------------------------------------------------------------
def _shade_frame(ctx, mesh, **mesh_kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    cam = mo.FRAME_CAM
    look = (rc.CENTRE - cam) / np.linalg.norm(rc.CENTRE - cam)
    fr = DeviceFrame(ctx, 32, 32, 2, fov_x=0.5, fov_y=0.5, origin=cam, rotation_euler=(np.arccos(-look[2]), 0.0, np.arctan2(-look[0], look[1])))
    fr.set_sky(synthetic_sky(128, 64))
    fr.set_disk(2.0, 6.0)
    fr.set_objects([], lamps=[[4.0, 10.0, 4.0, 9.0], [12.0, -9.0, 7.0, 7.0]])
    fr.set_mesh(mesh, chord=0.2, **mesh_kw)
    return fr


@pytest.mark.parametrize("call", ["shade_mesh", "shade_mesh_material"])
def test_shades_on_the_refitted_mesh(ctx, call):
    f = _ffi()
    V, F = rc.trace_mesh()
    rgb = np.random.default_rng(3).uniform(0.2, 1.0, (len(F), 3)).astype(np.float32)
    kw = (lambda: dict(tri_rgb=rgb)) if call == "shade_mesh" else (lambda: dict(material=f.MeshMaterial(tri_rgb=rgb, emission=0.05)))
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    mesh = f.Mesh(ctx, V, F, vertex_normals=_normals(V))
    fr = _shade_frame(ctx, mesh, **kw())
    first = fr.render(p).cpu().numpy().copy()
    for kind in ("noise", "twist", "permute"):
        Vn = rc.deform(V, kind)
        fr.refit_mesh(Vn, _normals(Vn))
        got = fr.render(p).cpu().numpy().copy()
        fresh = f.Mesh(ctx, Vn, F, vertex_normals=_normals(Vn))
        ff = _shade_frame(ctx, fresh, **kw())
        want = ff.render(p).cpu().numpy().copy()
        on_mesh = int(((ff.d_flags.cpu().numpy() == 0x88) & (ff.d_tri_id.cpu().numpy() >= 0)).sum())
        assert on_mesh > 50, (kind, on_mesh)
        assert np.array_equal(got, want), kind
        assert np.array_equal(fr.d_tri_id.cpu().numpy(), ff.d_tri_id.cpu().numpy())
        assert not np.array_equal(got, first)
        fresh.close()
    mesh.close()


# ---- 5. the brute-force oracle --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as oc
    return oc


@pytest.mark.parametrize("form", sorted(rc.FORMS))
def test_refitted_trace_against_the_oracle(ctx, oracle, form):
    """Flags, triangle and accepted steps as the oracle's on every ray it calls stable, end and bary of the hits within
    mesh_oracle_cases.hit_tolerances; at most UNSTABLE_CAP of the rays unstable."""
    f = _ffi()
    case = rc.oracle_case(form)
    o = mo.oracle_solve(oracle, case)
    V, _ = rc.trace_mesh()
    mesh = f.Mesh(ctx, V, case["F"])
    mesh.refit(case["V"])
    r = mc.trace_mesh_device(ctx, f.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"]), mesh, case["chord"], case["k0"],
                             case["x0"])
    mesh.close()
    st = o["stable"]
    assert (~st).mean() <= mo.UNSTABLE_CAP
    for key in ("flags", "tri", "n_accepted"):
        assert np.array_equal(r[key][st], o[key][st]), key
    hit = st & (o["tri"] >= 0)
    tol, shortest = mo.hit_tolerances(case["V"], case["F"], o["end"][hit], o["tri"][hit], o["sens"][hit], case["rhs"] == 2)
    d_end = np.abs(r["end"][hit] - o["end"][hit]).max(1)
    d_bary = np.abs(r["bary"][hit] - o["bary"][hit]).max(1)
    print(f"{form}: {int(hit.sum())} stable hits, worst |end - oracle| {d_end.max():.3e}, worst |bary - oracle| {d_bary.max():.3e}, "
          f"{int((~st).sum())} rays unstable")
    assert hit.sum() >= rc.MIN_HITS
    assert np.all(d_end <= tol) and np.all(d_bary <= tol / shortest)


# ---- 6. the device form, determinism, refusals ----------------------------------------------------------------------------------
def test_device_form_is_the_host_form(ctx):
    import torch
    f = _ffi()
    V, F, _ = MESHES["sphere4097"]
    Vn = rc.deform(V, "twist")
    Nn = _normals(Vn)
    a = f.Mesh(ctx, V, F, vertex_normals=_normals(V), leaf_size=1)
    b = f.Mesh(ctx, V, F, vertex_normals=_normals(V), leaf_size=1)
    a.refit(Vn, Nn)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_v, d_n = torch.as_tensor(Vn).cuda(), torch.as_tensor(Nn).cuda()
        b.refit(d_v, d_n, stream=s.cuda_stream)
    for x, y in zip(a.download_boxes(), b.download_boxes()):
        assert _same_bits(x, y)
    assert a.refit_info() == b.refit_info() and a.distance_range() == b.distance_range() and _same_bits(a.info()[2], b.info()[2])
    # the normals reach the shade the same way
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0)
    imgs = [_shade_frame(ctx, m).render(p).cpu().numpy().copy() for m in (a, b)]
    assert np.array_equal(imgs[0], imgs[1]) and len(np.unique(imgs[0][:, 0])) > 50
    a.close()
    b.close()


def test_two_refits_in_a_row_are_the_last_one(ctx):
    f = _ffi()
    V, F, _ = MESHES["ellipsoid128"]
    A, B = rc.deform(V, "permute"), rc.deform(V, "noise")
    once, twice = f.Mesh(ctx, V, F), f.Mesh(ctx, V, F)
    once.refit(B)
    twice.refit(A)
    twice.refit(B)
    for x, y in zip(once.download_boxes(), twice.download_boxes()):
        assert _same_bits(x, y)
    assert once.refit_info()[1:] == twice.refit_info()[1:] and (once.refit_info()[0], twice.refit_info()[0]) == (1, 2)
    assert once.distance_range() == twice.distance_range()
    once.close()
    twice.close()


def test_a_refused_refit_leaves_the_mesh_alone(ctx):
    import torch
    f = _ffi()
    V, F = rc.trace_mesh()
    k0 = rc.trace_rays(512, 5)
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0, rhs_form=2, spin=0.45)
    for normals in (None, _normals(V)):
        mesh = f.Mesh(ctx, V, F, vertex_normals=normals)
        mesh.refit(rc.deform(V, "noise"), None if normals is None else normals)
        before = (mesh.download_boxes(), mesh.info(), mesh.distance_range(), mesh.refit_info(),
                  mc.trace_mesh_device(ctx, p, mesh, rc.CHORD, k0, mo.FRAME_CAM))
        bad = rc.deform(V, "twist")
        bad[len(V) // 2, 2] = np.inf
        nan_normals = None if normals is None else np.where(np.arange(len(V))[:, None] == 3, np.nan, normals)
        with pytest.raises(f.BhgError, match="every vertex must be finite"):
            mesh.refit(bad, normals)
        with pytest.raises(f.BhgError, match="every vertex must be finite"):
            mesh.refit(torch.as_tensor(bad).cuda(), None if normals is None else torch.as_tensor(normals).cuda())
        if normals is None:
            with pytest.raises(f.BhgError, match="created without"):
                mesh.refit(rc.deform(V, "twist"), _normals(V))
        else:
            with pytest.raises(f.BhgError, match="created with them"):
                mesh.refit(rc.deform(V, "twist"))
            with pytest.raises(f.BhgError, match="every vertex normal must be finite"):
                mesh.refit(rc.deform(V, "twist"), nan_normals)
            with pytest.raises(f.BhgError, match="every vertex normal must be finite"):
                mesh.refit(torch.as_tensor(rc.deform(V, "twist")).cuda(), torch.as_tensor(nan_normals).cuda())
        with pytest.raises(ValueError):
            mesh.refit(V[:-1])
        rcode = f.load().bhg_mesh_refit(ctx._h, mesh._h, None, None)
        assert rcode == f.E_INVALID and b"vertices is NULL" in f.load().bhg_last_error()
        after = (mesh.download_boxes(), mesh.info(), mesh.distance_range(), mesh.refit_info(),
                 mc.trace_mesh_device(ctx, p, mesh, rc.CHORD, k0, mo.FRAME_CAM))
        assert all(_same_bits(x, y) for x, y in zip(before[0], after[0]))
        assert before[1][:2] == after[1][:2] and _same_bits(before[1][2], after[1][2]) and before[2:4] == after[2:4]
        assert _same(before[4], after[4]) and (before[4]["tri"] >= 0).sum() >= 20
        mesh.refit(rc.deform(V, "twist"), None if normals is None else normals)       # and the mesh still takes a good one
        assert mesh.refit_info()[0] == 2
        mesh.close()


# ---- 7. instance sets -----------------------------------------------------------------------------------------------------------
def test_instances_after_a_refit(ctx):
    import torch
    f = _ffi()
    V, F = mi.ellipsoid()
    T = mi.three_placements()
    k0 = mi.three_rays(1024)
    p = f.make_params(r_s=1.0, lambda_end=64.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    mesh = f.Mesh(ctx, V, F)
    inst = f.MeshInstances(mesh, T)
    box_before = inst.info()[1]
    Vn = rc.deform(V, "twist") * 1.3
    mesh.refit(Vn)
    with pytest.raises(f.BhgError, match="call bhg_mesh_instances_set after bhg_mesh_refit"):
        mi.trace_instances_device(ctx, p, inst, 0.25, k0, mo.FRAME_CAM)
    n = len(k0)
    z = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    zi = torch.zeros((n,), dtype=torch.int32, device="cuda")
    zf = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    out = torch.full((n, 4), mc.SENTINEL, dtype=torch.float64, device="cuda")
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    sky = torch.as_tensor(synthetic_sky(64, 32)).cuda()
    scene = f.make_scene(sky.data_ptr(), 64, 32)
    with pytest.raises(f.BhgError, match="call bhg_mesh_instances_set after bhg_mesh_refit"):
        ctx.shade_mesh_instances_device(z.data_ptr(), zf.data_ptr(), zi.data_ptr(), zi.data_ptr(), z.data_ptr(), n, 1, scene, inst,
                                        d_rgba=out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == mc.SENTINEL).all())
    inst.set(T)         # the same transforms: current again
    got = mi.trace_instances_device(ctx, p, inst, 0.25, k0, mo.FRAME_CAM)
    fresh_mesh = f.Mesh(ctx, Vn, F)
    fresh = f.MeshInstances(fresh_mesh, T)
    want = mi.trace_instances_device(ctx, p, fresh, 0.25, k0, mo.FRAME_CAM)
    assert all(np.array_equal(got[k], want[k]) for k in mi.KEYS) and (want["tri"] >= 0).sum() >= 60
    assert _same_bits(inst.info()[1], fresh.info()[1]) and not np.array_equal(inst.info()[1], box_before)
    local = mesh.info()[2]
    assert _same_bits(inst.info()[1][:3], np.min([f.mesh_instance_box_host(local, t)[:3] for t in T], axis=0))
    fresh_mesh.close()
    mesh.close()

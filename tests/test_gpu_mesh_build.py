"""The device-side mesh build on the GPU: bhg_mesh_create_device / bhg_mesh_rebuild_device /
bhg_mesh_rebuild against the host statement of the tree (bhg_mesh_bvh_morton_host: order, topology, boxes, slot records, root box,
distance range and area sum bit for bit), against the HOST-BUILT mesh of the same arrays (every output of bhg_trace_mesh_device,
of the instanced trace and of both shades, bit for bit: the tree only accelerates the hit rule), against the brute-force oracle of
section 19, through a refit, through rebuilds in place within a capacity, and the refusals.

The bad-index cases below are safe to run because no kernel follows a triangle index before the build's scan -- which reads the
triangle array alone -- has been read back and found clean (csrc/mesh_build.hip, build_run in csrc/bhgeo_mesh.hip): they end in
BHG_E_INVALID, and nothing here provokes anything else."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_build_reference as br  # noqa: E402
import mesh_cases as mc  # noqa: E402
import mesh_instance_cases as mi  # noqa: E402
import mesh_oracle_cases as mo  # noqa: E402
import mesh_refit_cases as rc  # noqa: E402

MESHES = br.meshes()
TREES = [(name, leaf) for name in MESHES for leaf in MESHES[name][2]]
TREE_IDS = [f"{n}-leaf{k}" for n, k in TREES]
TRACES = {f"{form}-{scene}": (rhs, a, rc.SCENES[scene]) for form, (rhs, a) in rc.FORMS.items() for scene in rc.SCENES}


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


def _is_the_host_statement(f, mesh, V, F, leaf):
    """tree, boxes, slot records, root box, depth and area sum of a device-built mesh against bhg_mesh_bvh_morton_host"""
    want = f.mesh_bvh_morton_host(V, F, leaf)
    tree = mesh.download_tree()
    for k in ("skip", "first", "count", "order"):
        assert np.array_equal(tree[k], want[k]), k
    box, tri = mesh.download_boxes()
    assert _same_bits(box, want["box"])
    assert _same_bits(tri, rc.slot_records(V, F, want))
    nn, depth, root = mesh.info()
    assert nn == len(want["skip"]) and depth == br.topology(len(F), leaf)[3] and _same_bits(root, want["box"][0])
    area = f.mesh_bvh_refit_host(V, F, want)[1]
    assert mesh.refit_info()[1:] == (area, area)
    return want


def _traces(ctx, mesh, k0, cases=TRACES):
    f = _ffi()
    return {name: mc.trace_mesh_device(ctx, f.make_params(rhs_form=rhs, spin=a, **par), mesh, rc.CHORD, k0, mo.FRAME_CAM)
            for name, (rhs, a, par) in cases.items()}


# ---- 1. the build is the host statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,leaf", TREES, ids=TREE_IDS)
def test_build_is_the_host_statement(ctx, name, leaf):
    f = _ffi()
    V, F, _ = MESHES[name]
    mesh = f.Mesh(ctx, V, F, leaf_size=leaf, build="device")
    _is_the_host_statement(f, mesh, V, F, leaf)
    info = mesh.build_info()
    assert info == dict(built_on_device=True, builds=1, cap_vertices=len(V), cap_triangles=len(F), allocations=3)
    assert mesh.refit_info()[0] == 0
    # the distance range is the host-built mesh's: the same formulas on the same root box and farthest vertex ...
    host = f.Mesh(ctx, V, F, leaf_size=leaf)
    assert _same_bits(host.info()[2], mesh.info()[2]) and host.distance_range() == mesh.distance_range()
    assert host.build_info() == dict(built_on_device=False, builds=1, cap_vertices=len(V), cap_triangles=len(F), allocations=1)
    host.close()
    mesh.close()


@pytest.mark.parametrize("nt", br.GRID_SIZES)
def test_build_of_a_jittered_grid(ctx, nt):
    """1 / 255 / 256 / 257: around one workgroup of the per-triangle kernels; 4 097 and 70 001: several workgroups, the sort's
    multi-block passes, and at leaf_size 4 (17 500 inner nodes at the largest) the refit's launch per level."""
    import torch
    f = _ffi()
    V, F = br.grid_mesh(nt)
    d_v, d_f = torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda()
    mesh = f.Mesh.from_device(ctx, d_v, d_f, leaf_size=4)
    want = _is_the_host_statement(f, mesh, V, F, 4)
    if nt == 70001:
        assert (want["count"] == 0).sum() > 1024
    mesh.close()


def test_build_above_the_sorts_merge_limit(ctx):
    """2^20 + 3 triangles: the one size at which the sort takes its radix passes (below it, it merges), and 2^19 inner nodes."""
    import torch
    f = _ffi()
    V, F = br.grid_mesh(br.GRID_SIZE_RADIX)
    mesh = f.Mesh.from_device(ctx, torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda(), leaf_size=4)
    want = f.mesh_bvh_morton_host(V, F, 4)
    tree = mesh.download_tree()
    for k in ("skip", "first", "count", "order"):
        assert np.array_equal(tree[k], want[k]), k
    assert _same_bits(mesh.download_boxes()[0], want["box"])
    assert mesh.refit_info()[1] == f.mesh_bvh_refit_host(V, F, want)[1]
    mesh.close()


# ---- 2. the equality that matters: traces and shades on the host-built mesh -------------------------------------------------------
@pytest.fixture(scope="module")
def host_traces(ctx):
    """Every trace case on the HOST-built mesh (the whole-step cull on): computed once."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0"
    f = _ffi()
    V, F = rc.trace_mesh()
    mesh = f.Mesh(ctx, V, F)
    res = _traces(ctx, mesh, rc.trace_rays())
    mesh.close()
    return res


def test_trace_on_the_device_built_mesh_is_the_host_built_trace(ctx, host_traces):
    f = _ffi()
    V, F = rc.trace_mesh()
    mesh = f.Mesh(ctx, V, F, build="device")
    assert not np.array_equal(mesh.download_tree()["order"], f.mesh_bvh_host(V, F)["order"])      # another tree ...
    got = _traces(ctx, mesh, rc.trace_rays())
    mesh.close()
    for name in TRACES:
        assert (host_traces[name]["tri"] >= 0).sum() >= rc.MIN_HITS, name
        for key in rc.KEYS:                                                                       # ... the same bits
            assert np.array_equal(got[name][key], host_traces[name][key]), (name, key)


def test_instances_of_a_device_built_mesh(ctx):
    f = _ffi()
    V, F = mi.ellipsoid()
    T = mi.three_placements()
    k0 = mi.three_rays(1024)
    p = f.make_params(r_s=1.0, lambda_end=64.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    res = []
    for build in ("host", "device"):
        mesh = f.Mesh(ctx, V, F, build=build)
        inst = f.MeshInstances(mesh, T)
        res.append((mi.trace_instances_device(ctx, p, inst, 0.25, k0, mo.FRAME_CAM), inst.info()[1]))
        mesh.close()
    assert all(np.array_equal(res[0][0][k], res[1][0][k]) for k in mi.KEYS) and (res[0][0]["tri"] >= 0).sum() >= 60
    assert _same_bits(res[0][1], res[1][1])


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
def test_shades_on_the_device_built_mesh(ctx, call):
    f = _ffi()
    V, F = rc.trace_mesh()
    rgb = np.random.default_rng(3).uniform(0.2, 1.0, (len(F), 3)).astype(np.float32)
    kw = (lambda: dict(tri_rgb=rgb)) if call == "shade_mesh" else (lambda: dict(material=f.MeshMaterial(tri_rgb=rgb, emission=0.05)))
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    imgs, tris = [], []
    for build in ("host", "device"):
        mesh = f.Mesh(ctx, V, F, vertex_normals=_normals(V), build=build)
        fr = _shade_frame(ctx, mesh, **kw())
        imgs.append(fr.render(p).cpu().numpy().copy())
        tris.append(fr.d_tri_id.cpu().numpy().copy())
        on_mesh = int(((fr.d_flags.cpu().numpy() == 0x88) & (tris[-1] >= 0)).sum())
        assert on_mesh > 50, (build, on_mesh)
        mesh.close()
    assert np.array_equal(imgs[0], imgs[1]) and np.array_equal(tris[0], tris[1])


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as oc
    return oc


@pytest.mark.parametrize("form", sorted(rc.FORMS))
def test_device_built_trace_against_the_oracle(ctx, oracle, form):
    """Flags, triangle and accepted steps as the oracle's on every ray it calls stable, end and bary of the hits within
    mesh_oracle_cases.hit_tolerances; at most UNSTABLE_CAP of the rays unstable."""
    f = _ffi()
    case = rc.oracle_case(form)
    o = mo.oracle_solve(oracle, case)
    mesh = f.Mesh(ctx, case["V"], case["F"], build="device")
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


# ---- 3. a refit of a device-built mesh ----------------------------------------------------------------------------------------------
def test_refit_of_a_device_built_mesh(ctx):
    f = _ffi()
    V, F = rc.trace_mesh()
    Vn = rc.deform(V, "twist")
    k0 = rc.trace_rays()
    cases = {k: TRACES[k] for k in ("reduced-disk_and_exit", "kerr_plus-bare")}
    mesh = f.Mesh(ctx, V, F, build="device")
    tree = mesh.download_tree()
    mesh.refit(Vn)
    assert mesh.refit_info()[0] == 1 and mesh.build_info()["builds"] == 1 and mesh.build_info()["allocations"] == 3
    box, tri = mesh.download_boxes()
    want, area = f.mesh_bvh_refit_host(Vn, F, tree)
    assert _same_bits(box, want) and _same_bits(tri, rc.slot_records(Vn, F, tree)) and mesh.refit_info()[2] == area
    got = _traces(ctx, mesh, k0, cases)
    fresh = f.Mesh(ctx, Vn, F)
    want = _traces(ctx, fresh, k0, cases)
    assert mesh.distance_range() == fresh.distance_range() and _same_bits(mesh.info()[2], fresh.info()[2])
    for name in cases:
        assert _same(got[name], want[name]) and (want[name]["tri"] >= 0).sum() >= rc.MIN_HITS, name
    fresh.close()
    mesh.close()


# ---- 4. rebuilds in place -----------------------------------------------------------------------------------------------------------
def _state(ctx, f, mesh, k0, p):
    return (mesh.download_tree(), mesh.download_boxes(), mesh.info(), mesh.distance_range(), mesh.refit_info()[1:],
            mc.trace_mesh_device(ctx, p, mesh, rc.CHORD, k0, mo.FRAME_CAM))


def _same_state(a, b):
    return (all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and all(_same_bits(x, y) for x, y in zip(a[1], b[1]))
            and a[2][:2] == b[2][:2] and _same_bits(a[2][2], b[2][2]) and a[3:5] == b[3:5] and _same(a[5], b[5]))


def test_rebuild_in_place(ctx):
    import torch
    f = _ffi()
    A = MESHES["ellipsoid128"][:2]
    B = MESHES["sphere4097"][:2]
    k0 = rc.trace_rays(512, 5)
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0, rhs_form=2, spin=0.45)
    cap = (len(B[0]), len(B[1]))
    # three placements that keep the meshes where the rays go: as it lies, and pushed a little two ways
    T = np.stack([mi.record(np.eye(3), t) for t in ((0.0, 0.0, 0.0), (0.6, -0.4, 0.3), (-0.5, 0.7, -0.2))])
    mesh = f.Mesh(ctx, *A, build="device", capacity=cap)
    by_host_arrays = f.Mesh(ctx, *A, build="device", capacity=cap)
    inst = f.MeshInstances(mesh, T)
    info0 = mesh.build_info()
    assert info0 == dict(built_on_device=True, builds=1, cap_vertices=cap[0], cap_triangles=cap[1], allocations=3)
    hits = []
    for step, (V, F) in enumerate((B, A), 1):
        mesh.rebuild(torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda())
        by_host_arrays.rebuild(V, F)
        fresh = f.Mesh(ctx, V, F, build="device")
        want = _state(ctx, f, fresh, k0, p)
        assert _same_state(_state(ctx, f, mesh, k0, p), want), step
        assert _same_state(_state(ctx, f, by_host_arrays, k0, p), want), step
        _is_the_host_statement(f, mesh, V, F, 4)
        hits.append(int((want[5]["tri"] >= 0).sum()))
        for m in (mesh, by_host_arrays):
            assert m.build_info() == dict(info0, builds=1 + step) and m.refit_info()[0] == step
            assert (m.n_vertices, m.n_triangles) == (len(V), len(F))
        # the instance set has gone stale: refused by trace and shade until it is set again, then a fresh set's
        with pytest.raises(f.BhgError, match="call bhg_mesh_instances_set"):
            mi.trace_instances_device(ctx, p, inst, 0.25, k0, mo.FRAME_CAM)
        n = len(k0)
        z = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
        zi = torch.zeros((n,), dtype=torch.int32, device="cuda")
        zf = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        out = torch.full((n, 4), mc.SENTINEL, dtype=torch.float64, device="cuda")
        from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
        sky = torch.as_tensor(synthetic_sky(64, 32)).cuda()
        with pytest.raises(f.BhgError, match="call bhg_mesh_instances_set"):
            ctx.shade_mesh_instances_device(z.data_ptr(), zf.data_ptr(), zi.data_ptr(), zi.data_ptr(), z.data_ptr(), n, 1,
                                            f.make_scene(sky.data_ptr(), 64, 32), inst, d_rgba=out.data_ptr(),
                                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((out == mc.SENTINEL).all())
        inst.set(T)
        fresh_inst = f.MeshInstances(fresh, T)
        got_i = mi.trace_instances_device(ctx, p, inst, 0.25, k0, mo.FRAME_CAM)
        want_i = mi.trace_instances_device(ctx, p, fresh_inst, 0.25, k0, mo.FRAME_CAM)
        assert all(np.array_equal(got_i[k], want_i[k]) for k in mi.KEYS) and _same_bits(inst.info()[1], fresh_inst.info()[1])
        assert (want_i["tri"] >= 0).sum() >= 20 and len(np.unique(want_i["inst"][want_i["tri"] >= 0])) == 3
        fresh.close()
    assert min(hits) >= 20, hits
    by_host_arrays.close()
    mesh.close()


def test_rebuild_of_a_host_built_mesh(ctx):
    """A mesh of bhg_mesh_create has its own counts as capacity: rebuilt at those or fewer, refused above them."""
    f = _ffi()
    V, F = rc.trace_mesh()
    k0 = rc.trace_rays(512, 5)
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0)
    mesh = f.Mesh(ctx, V, F)
    Vs, Fs = MESHES["ellipsoid128"][:2]
    with pytest.raises(f.BhgError, match="capacity"):
        mesh.rebuild(*MESHES["sphere4097"][:2])
    for V2, F2 in ((Vs, Fs), (rc.deform(V, "twist"), F[::-1].copy())):
        mesh.rebuild(V2, F2)
        fresh = f.Mesh(ctx, V2, F2, build="device")
        assert _same_state(_state(ctx, f, mesh, k0, p), _state(ctx, f, fresh, k0, p))
        fresh.close()
    info = mesh.build_info()
    assert info["built_on_device"] and info["builds"] == 3 and (info["cap_vertices"], info["cap_triangles"]) == (len(V), len(F))
    allocations = info["allocations"]
    mesh.rebuild(Vs, Fs)
    assert mesh.build_info()["allocations"] == allocations
    mesh.close()


# ---- 5. refused, the mesh untouched -------------------------------------------------------------------------------------------------
def test_a_refused_build_leaves_the_mesh_alone(ctx):
    import ctypes as C
    import torch
    f = _ffi()
    L = f.load()
    V, F = rc.trace_mesh()
    k0 = rc.trace_rays(512, 5)
    p = f.make_params(r_s=1.0, lambda_end=46.0, r_exit=30.0, rhs_form=2, spin=0.45)
    over = MESHES["sphere4097"][:2]
    at_nv, negative, nan = F.copy(), F.copy(), rc.deform(V, "twist")
    at_nv[len(F) // 2, 1] = len(V)
    negative[7, 0] = -1
    nan[len(V) // 3, 2] = np.nan
    cases = (("capacity", over[0], over[1]), ("outside", V, at_nv), ("outside", V, negative), ("every vertex must be finite", nan, F))
    dev = lambda a: torch.as_tensor(a).cuda()      # noqa: E731
    for host_built in (False, True):
        mesh = f.Mesh(ctx, V, F) if host_built else f.Mesh(ctx, V, F, build="device")
        if host_built:
            mesh.rebuild(V, F)      # (its move into an image by capacity happens here, so that `allocations` below can be compared)
        before = _state(ctx, f, mesh, k0, p)
        counts = (mesh.build_info(), mesh.refit_info()[0])
        for what, Vb, Fb in cases:
            with pytest.raises(f.BhgError, match=what):
                mesh.rebuild(dev(Vb), dev(Fb))
            with pytest.raises(f.BhgError, match=what):
                mesh.rebuild(Vb, Fb)
            assert (mesh.n_vertices, mesh.n_triangles) == (len(V), len(F))
        with pytest.raises(f.BhgError, match="created without"):
            mesh.rebuild(V, F, _normals(V))
        assert _same_state(_state(ctx, f, mesh, k0, p), before) and (before[5]["tri"] >= 0).sum() >= 20
        assert (mesh.build_info(), mesh.refit_info()[0]) == counts
        mesh.close()
    with_normals = f.Mesh(ctx, V, F, vertex_normals=_normals(V), build="device")
    with pytest.raises(f.BhgError, match="created with them"):
        with_normals.rebuild(V, F)
    bad_normals = _normals(V)
    bad_normals[3, 0] = np.inf
    with pytest.raises(f.BhgError, match="every vertex normal must be finite"):
        with_normals.rebuild(V, F, bad_normals)
    with_normals.close()
    # a mesh whose leaves the device build does not make
    big_leaves = f.Mesh(ctx, V, F, leaf_size=65)
    with pytest.raises(f.BhgError, match=r"leaf_size 65 must be in \[1, 64\]"):
        big_leaves.rebuild(V, F)
    big_leaves.close()
    # a refused creation: BHG_E_INVALID, *out NULL
    d_v = dev(V)
    for Fb, leaf, what in ((at_nv, 4, b"outside"), (negative, 4, b"outside"), (F, 65, b"leaf_size 65")):
        d_f = dev(Fb)
        out = C.c_void_p(1234)
        rcode = L.bhg_mesh_create_device(ctx._h, C.c_void_p(d_v.data_ptr()), len(V), C.c_void_p(d_f.data_ptr()), len(Fb), None, leaf, 0, 0,
                                         None, C.byref(out))
        assert rcode == f.E_INVALID and what in L.bhg_last_error() and out.value is None
    d_nan = dev(nan)
    with pytest.raises(f.BhgError, match="every vertex must be finite"):
        f.Mesh.from_device(ctx, d_nan, dev(F))
    with pytest.raises(f.BhgError, match="cap_vertices / cap_triangles"):
        f.Mesh(ctx, V, F, build="device", capacity=(len(V), len(F) - 1))

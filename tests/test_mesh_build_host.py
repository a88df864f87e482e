"""The device-side mesh build without a GPU: the ABI surface; bhg_mesh_bvh_morton_host -- the host statement
of the tree the build kernels make -- against the numpy restatement of tests/mesh_build_reference.py bit for bit, against the
existing builder's topology and the refit's host calls, its order, containment and determinism; and every refusal that needs no
device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mesh_build_reference as br  # noqa: E402

NEW = ("bhg_mesh_create_device", "bhg_mesh_rebuild_device", "bhg_mesh_rebuild", "bhg_mesh_build_info", "bhg_mesh_bvh_morton_host",
       "bhg_mesh_tree_host", "bhg_frame_set_mesh_build", "bhg_frame_mesh_build_info")
MESHES = br.meshes()
TREES = [(name, leaf) for name in MESHES for leaf in MESHES[name][2]]
IDS = [f"{n}-leaf{k}" for n, k in TREES]
TOPOLOGY = ("skip", "first", "count")


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_exports_header_and_signatures():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_MESH_BUILD_DEVICE\s+1\s*$", hdr, re.M)
    # within ABI 10: neither number moved
    assert re.search(r"^#define\s+BHG_ABI_VERSION\s+10\b", hdr, re.M) and re.search(r"^#define\s+BHG_ABI_COMPAT_MIN\s+7\b", hdr, re.M)
    assert L.bhg_version() == 10
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
        "int bhg_mesh_create_device(bhg_context *ctx, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles, "
        "size_t n_triangles, const double *d_vertex_normals , int32_t leaf_size, size_t cap_vertices, size_t cap_triangles, "
        "void *stream, bhg_mesh **out);",
        "int bhg_mesh_rebuild_device(bhg_context *ctx, bhg_mesh *mesh, const double *d_vertices, size_t n_vertices, "
        "const int32_t *d_triangles, size_t n_triangles, const double *d_vertex_normals, void *stream);",
        "int bhg_mesh_rebuild(bhg_context *ctx, bhg_mesh *mesh, const double *vertices, size_t n_vertices, const int32_t *triangles, "
        "size_t n_triangles, const double *vertex_normals);",
        "int bhg_mesh_build_info(const bhg_mesh *mesh, int32_t *built_on_device, uint64_t *builds, size_t *cap_vertices, "
        "size_t *cap_triangles, uint64_t *allocations);",
        "int bhg_mesh_tree_host(const bhg_mesh *mesh, int32_t *node_skip, int32_t *node_first, int32_t *node_count, "
        "int32_t *tri_order, size_t cap, size_t *n_nodes);",
    ):
        assert proto in flat, proto
    # bhg_mesh_bvh_morton_host takes what bhg_mesh_bvh_host takes
    args = lambda name: re.search(r"int " + name + r"\((.*?)\);", flat).group(1)     # noqa: E731
    assert args("bhg_mesh_bvh_morton_host") == args("bhg_mesh_bvh_host")
    for name in ("from_device", "rebuild", "build_info", "download_tree"):
        assert hasattr(f.Mesh, name)
    for name in ("set_mesh_build", "mesh_build_info"):
        assert hasattr(f.Frame, name)
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    assert hasattr(DeviceFrame, "rebuild_mesh") and hasattr(f, "mesh_bvh_morton_host")
    assert L.bhg_frame_set_mesh_build(None, 1) == f.E_INVALID and b"frame is NULL" in L.bhg_last_error()
    assert L.bhg_frame_mesh_build_info(None, 0, None, None, None, None, None) == f.E_INVALID and b"frame is NULL" in L.bhg_last_error()


@pytest.mark.parametrize("name,leaf", TREES, ids=IDS)
def test_against_the_numpy_restatement(name, leaf):
    f, _ = _lib()
    V, F, _ = MESHES[name]
    tree = f.mesh_bvh_morton_host(V, F, leaf)
    want = br.morton_tree(V, F, leaf)
    assert np.array_equal(tree["order"], want["order"])
    for k in TOPOLOGY:
        assert np.array_equal(tree[k], want[k]), k
    assert np.array_equal(_bits(tree["box"]), _bits(want["box"]))
    assert not np.isnan(tree["box"]).any()
    assert tree["count"].max() <= leaf
    if name == "identical5":     # 2 + 3, not the one leaf of five the existing builder makes
        assert tree["count"].tolist() == [0, 2, 3] and tree["order"].tolist() == [0, 1, 2, 3, 4]
    if name in ("nt_is_leaf", "one"):
        assert len(tree["skip"]) == 1
    if name == "nt_is_leaf_plus_1":
        assert tree["count"].tolist() == [0, 2, 3]


def test_cells_clamp_and_overflow():
    """The clamp is exercised -- on every axis of the wide-range mesh the largest centroid's product reaches 2^21 or rounds just
    below it, and its cell is 2^21 - 1 -- and the overflowing axes give cell 0."""
    V, F, _ = MESHES["wide_range"]
    c = br.centroids(V, F)
    q = br.cells(V, F)
    assert np.ptp(np.log10(np.abs(V)), axis=0).min() > 8.0
    for a in range(3):
        assert q[np.argmax(c[:, a]), a] == 2**21 - 1 and q[np.argmin(c[:, a]), a] == 0
    assert q.max() == 2**21 - 1
    V, F, _ = MESHES["overflow"]
    c = br.centroids(V, F)
    assert np.isinf(c[:, 0]).sum() == 4 and np.isinf(c[:, 1]).all() and np.isfinite(c[:, 2]).all()
    q = br.cells(V, F)
    assert not q[:, :2].any() and q[:, 2].max() == 2**21 - 1
    V, F, _ = MESHES["plate"]     # one zero extent: that axis' cells are all 0
    q = br.cells(V, F)
    flat = np.flatnonzero(np.ptp(br.centroids(V, F), axis=0) == 0.0)
    assert len(flat) == 1 and not q[:, flat[0]].any() and q.any()


@pytest.mark.parametrize("name,leaf", TREES, ids=IDS)
def test_against_the_existing_builder_and_the_refit(name, leaf):
    f, _ = _lib()
    V, F, _ = MESHES[name]
    tree = f.mesh_bvh_morton_host(V, F, leaf)
    # the refit's host statement takes the topology and gives the same boxes; the schedule walks it
    box, area = f.mesh_bvh_refit_host(V, F, tree)
    assert np.array_equal(_bits(box), _bits(tree["box"]))
    nodes, off = f.mesh_refit_schedule_host(tree)
    assert sorted(nodes.tolist()) == np.flatnonzero(tree["count"] == 0).tolist()
    assert off[-1] == len(nodes) and np.flatnonzero(np.diff(off)).size == br.topology(len(F), leaf)[3]
    # the existing builder's topology, wherever it made no over-size leaf
    host = f.mesh_bvh_host(V, F, leaf)
    if host["count"].max() <= leaf:
        for k in TOPOLOGY:
            assert np.array_equal(tree[k], host[k]), k
    else:
        # (coinciding centroids: the five identical triangles; the sphere's repeated triangle, alone with its twin at leaf_size 1;
        # the centroids that overflowed to one infinity)
        assert (name, leaf) in (("identical5", 4), ("sphere4097", 1), ("overflow", 1), ("overflow", 4))


@pytest.mark.parametrize("name,leaf", TREES, ids=IDS)
def test_order_and_containment(name, leaf):
    f, _ = _lib()
    V, F, _ = MESHES[name]
    tree = f.mesh_bvh_morton_host(V, F, leaf)
    order, box = tree["order"], tree["box"]
    assert sorted(order.tolist()) == list(range(len(F)))
    leaves = np.flatnonzero(tree["count"] > 0)
    for i in leaves:
        assert np.all(np.diff(order[tree["first"][i]:tree["first"][i] + tree["count"][i]]) > 0)
    # every box holds every vertex below it and both its children
    ends = tree["first"][leaves] + tree["count"][leaves]
    for i in range(len(box)):
        sub = leaves[(leaves >= i) & (leaves < tree["skip"][i])]
        lo, hi = int(tree["first"][sub[0]]), int(ends[np.searchsorted(leaves, sub[-1])])
        pts = V[F[order[lo:hi]]].reshape(-1, 3)
        assert np.all(pts >= box[i, :3]) and np.all(pts <= box[i, 3:])
        if tree["count"][i] == 0:
            for c in (i + 1, int(tree["skip"][i + 1])):
                assert np.all(box[c, :3] >= box[i, :3]) and np.all(box[c, 3:] <= box[i, 3:])


def test_determinism():
    """The keys against Python's own integers, and the order under equal keys: triangles with one centroid keep the caller's
    order whatever lies between them."""
    f, _ = _lib()
    for name in ("ellipsoid128", "wide_range", "overflow", "plate"):
        V, F, _ = MESHES[name]
        assert br.keys(V, F).tolist() == br.keys_python(V, F)
        assert max(br.keys_python(V, F)) < 2**63
    V, F, _ = MESHES["ellipsoid128"]
    # every triangle three times, the copies dealt over the list at random: equal keys in threes
    rng = np.random.default_rng(2)
    src = rng.permutation(np.repeat(np.arange(len(F)), 3))
    F3 = np.ascontiguousarray(F[src])
    tree = f.mesh_bvh_morton_host(V, F3, 1)
    order = tree["order"]
    key = br.keys(V, F3)
    assert np.all(np.diff(key[order].astype(np.int64)) >= 0)
    same = np.diff(key[order].astype(np.int64)) == 0
    assert same.sum() >= 2 * len(F) and np.all(np.diff(order)[same] > 0)
    assert np.array_equal(order, br.morton_tree(V, F3, 1)["order"])
    # the same mesh again: the same bits
    again = f.mesh_bvh_morton_host(V, F3, 1)
    assert all(np.array_equal(tree[k], again[k]) for k in tree)


def test_refusals_of_the_host_call():
    f, L = _lib()
    V, F, _ = MESHES["ellipsoid128"]
    bad = V.copy()
    bad[7, 1] = np.nan
    with pytest.raises(f.BhgError, match="every vertex must be finite"):
        f.mesh_bvh_morton_host(bad, F, 4)
    with pytest.raises(f.BhgError, match="outside"):
        f.mesh_bvh_morton_host(V[:-1], F, 4)
    neg = F.copy()
    neg[3, 2] = -1
    with pytest.raises(f.BhgError, match="outside"):
        f.mesh_bvh_morton_host(V, neg, 4)
    with pytest.raises(f.BhgError, match="leaf_size"):
        f.mesh_bvh_morton_host(V, F, 0)
    # any leaf_size >= 1 is taken on the host: one leaf of 128
    assert f.mesh_bvh_morton_host(V, F, 128)["count"].tolist() == [128]
    nn = C.c_size_t(0)
    err = lambda: L.bhg_last_error()     # noqa: E731
    assert L.bhg_mesh_bvh_morton_host(None, 3, F.ctypes.data, 1, 4, None, None, None, None, None, 0, C.byref(nn)) == f.E_INVALID
    assert b"NULL" in err()
    assert L.bhg_mesh_bvh_morton_host(V.ctypes.data, len(V), F.ctypes.data, 0, 4, None, None, None, None, None, 0, C.byref(nn)) == f.E_INVALID
    assert b"must be > 0" in err()
    assert L.bhg_mesh_bvh_morton_host(V.ctypes.data, len(V), F.ctypes.data, len(F), 4, None, None, None, None, None, 0, None) == f.E_INVALID
    assert b"n_nodes is NULL" in err()
    # cap too small: refused, n_nodes still told
    assert L.bhg_mesh_bvh_morton_host(V.ctypes.data, len(V), F.ctypes.data, len(F), 4, None, None, None, None, None, 3,
                                      C.byref(nn)) == f.E_INVALID
    assert b"more nodes than cap" in err() and nn.value == 63
    assert L.bhg_mesh_bvh_morton_host(V.ctypes.data, len(V), F.ctypes.data, len(F), 4, None, None, None, None, None, 63,
                                      C.byref(nn)) == f.E_INVALID
    assert b"output array is NULL" in err()


def test_refusals_of_the_device_calls_without_a_device():
    """Everything the four calls refuse before they need a context.  The array arguments stand for device addresses and are never
    followed: every refusal here comes first."""
    f, L = _lib()
    err = lambda: L.bhg_last_error()     # noqa: E731
    out = C.c_void_p(1234)
    dv, df = 4096, 8192
    create = lambda *a: L.bhg_mesh_create_device(None, *a, None, C.byref(out))     # noqa: E731
    assert L.bhg_mesh_create_device(None, dv, 3, df, 1, None, 4, 0, 0, None, None) == f.E_INVALID and b"out is NULL" in err()
    for args, what in (((None, 3, df, 1, None, 4, 0, 0), b"vertices / triangles is NULL"),
                       ((dv, 3, None, 1, None, 4, 0, 0), b"vertices / triangles is NULL"),
                       ((dv, 0, df, 1, None, 4, 0, 0), b"must be > 0"),
                       ((dv, 3, df, 0, None, 4, 0, 0), b"must be > 0"),
                       ((dv, 2**31, df, 1, None, 4, 0, 0), b"2^31 - 1"),
                       ((dv, 3, df, 1, None, 0, 0, 0), b"leaf_size 0 must be in [1, 64]"),
                       ((dv, 3, df, 1, None, 65, 0, 0), b"leaf_size 65 must be in [1, 64]"),
                       ((dv, 3, df, 2, None, 4, 0, 1), b"cap_vertices / cap_triangles"),
                       ((dv, 3, df, 1, None, 4, 2, 0), b"cap_vertices / cap_triangles"),
                       ((dv, 3, df, 1, None, 4, 2**31, 0), b"2^31 - 1"),
                       ((dv, 3, df, 1, None, 4, 0, 0), b"ctx is NULL")):
        out.value = 1234
        assert create(*args) == f.E_INVALID and what in err(), (args, err())
        assert out.value is None
    assert L.bhg_mesh_rebuild_device(None, None, dv, 3, df, 1, None, None) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_rebuild(None, None, dv, 3, df, 1, None) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_build_info(None, None, None, None, None, None) == f.E_INVALID and b"mesh is NULL" in err()
    n = C.c_size_t(0)
    assert L.bhg_mesh_tree_host(None, None, None, None, None, 0, C.byref(n)) == f.E_INVALID and b"mesh is NULL" in err()
    # the binding's own checks
    with pytest.raises(ValueError, match="build must be"):
        f.Mesh(None, np.zeros((3, 3)), np.array([[0, 1, 2]]), build="gpu")
    with pytest.raises(ValueError, match="capacity goes with"):
        f.Mesh(None, np.zeros((3, 3)), np.array([[0, 1, 2]]), capacity=(3, 1))


# ---- the add-on's rule on the stub bpy ---------------------------------------------------------------------------------------
def _addon(monkeypatch, **props):
    """The stub scene of the mesh tests on a recording frame that also records refit_mesh and set_mesh_build ->
    (engine, add-on, cube, render()); render() gives the kinds of the calls the frame has seen so far."""
    import test_mesh_material_host as tm
    from blackhole_geodesic_calculator_amd import _ffi

    class Recording(tm._RecordingFrame):
        def refit_mesh(self, vertices, vertex_normals=None, rebuild_ratio=None):
            self.calls.append(("refit", vertices, vertex_normals, rebuild_ratio))

        def set_mesh_build(self, on):
            self.calls.append(("build", bool(on)))

    bpy, depsgraph, addon, cube, tetra = tm.mesh_scene(width=8, height=8, samples=1, device_shading=1.0, curved_space_meshes=1.0, **props)
    eng = tm._device_engine(monkeypatch, addon, depsgraph)
    monkeypatch.setattr(_ffi, "Frame", Recording)
    eng.device_shading = True
    buf = np.ones((8, 8, 4))

    def render():
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
        return [c[0] for c in tm._RecordingFrame.made[-1].calls if c[0] in ("mesh", "refit", "build")]

    return eng, addon, cube, render


def test_addon_property_and_default():
    import test_mesh_material_host as tm
    bpy, depsgraph, addon, cube, tetra = tm.mesh_scene(width=8, height=8, samples=1)
    names = {p[0]: p[1] for p in addon.EXTRA_PROPS}
    assert "curved_space_mesh_build" in names and len(addon.PROPS) == 12
    assert "curved_space_mesh_build" in [row[0] for row in addon.CUSTOM_RENDER_PT_blackhole._ROWS]
    assert not getattr(depsgraph.scene, "curved_space_mesh_build", 0)       # off unless the scene says so


def test_addon_rule(monkeypatch):
    import fake_bpy_mesh as fbm
    # the switch off (the default): the frame is never told anything about builds, every change is a set
    eng, addon, cube, render = _addon(monkeypatch)
    assert render() == ["mesh"] and eng.device_mesh_action == "set"
    polys = cube._mesh._polys
    polys[2] = polys[2][1:] + polys[2][:1]
    assert render() == ["mesh", "mesh"] and eng.device_mesh_action == "set"
    addon.release_device_frames()
    # the switch on: the frame is switched to the device build once, before its first mesh; an unchanged scene is kept; a changed
    # triangle list, a changed vertex count and changed UVs are rebuilds; moved vertices alone are a refit with the refit switch
    # on and a rebuild without it
    for refit in (1.0, 0.0):
        eng, addon, cube, render = _addon(monkeypatch, curved_space_mesh_build=1.0, curved_space_mesh_refit=refit)
        assert render() == ["build", "mesh"] and eng.device_mesh_action == "set"
        assert render() == ["build", "mesh"] and eng.device_mesh_action == "kept"
        polys = cube._mesh._polys
        polys[2] = polys[2][1:] + polys[2][:1]
        assert render() == ["build", "mesh", "mesh"] and eng.device_mesh_action == "rebuild"
        old = cube._mesh
        verts = [v.co for v in old.vertices] + [(0.0, 0.0, 3.0)]
        uv = np.array([d.uv for d in old.uv_layers.active.data], np.float32)
        cube._mesh = fbm.FakeMesh(verts, list(polys), uv)
        assert render() == ["build", "mesh", "mesh", "mesh"] and eng.device_mesh_action == "rebuild"
        cube._mesh = fbm.FakeMesh(verts, list(polys), np.ascontiguousarray(uv[:, ::-1]))
        assert render() == ["build"] + ["mesh"] * 4 and eng.device_mesh_action == "rebuild"
        v = cube._mesh.vertices[6]
        v.co = (v.co[0] + 0.25, v.co[1], v.co[2] + 0.25)
        assert render() == ["build"] + ["mesh"] * 4 + (["refit"] if refit else ["mesh"])
        assert eng.device_mesh_action == ("refit" if refit else "rebuild")
        addon.release_device_frames()

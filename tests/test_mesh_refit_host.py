"""Deforming meshes without a GPU: the ABI surface, bhg_mesh_bvh_refit_host -- the CPU statement of the
refit kernels -- against bhg_mesh_bvh_host on unchanged vertices (bit for bit) and against a numpy restatement on new ones, the
containment a refit owes the trace, the area sum, the bottom-up schedule, the refusals that need no device, and the conditions
of the cases tests/test_gpu_mesh_refit.py runs (enough hits per trace case; the oracle alone stable on its cases)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mesh_oracle_cases as mo  # noqa: E402
import mesh_refit_cases as rc  # noqa: E402

NEW = ("bhg_mesh_refit", "bhg_mesh_refit_device", "bhg_mesh_refit_info", "bhg_mesh_bvh_refit_host", "bhg_mesh_refit_schedule_host",
       "bhg_mesh_boxes_host", "bhg_mesh_range")
MESHES = rc.meshes()
TREES = [(name, leaf) for name in MESHES for leaf in MESHES[name][2]]


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def test_exports_and_header():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS and hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_MESH_REFIT\s+1\s*$", hdr, re.M)
    assert L.bhg_version() == 10
    for name in ("refit", "refit_info", "download_boxes"):
        assert hasattr(f.Mesh, name)
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    assert hasattr(DeviceFrame, "refit_mesh")


@pytest.mark.parametrize("name,leaf", TREES, ids=[f"{n}-leaf{k}" for n, k in TREES])
def test_unchanged_vertices_give_the_builders_boxes(name, leaf):
    f, _ = _lib()
    V, F, _ = MESHES[name]
    tree = f.mesh_bvh_host(V, F, leaf)
    if name == "identical5":
        assert len(tree["skip"]) == 1 and tree["count"][0] == 5 > leaf
    if name == "sphere4097":
        assert len(F) == 4097
    box, area = f.mesh_bvh_refit_host(V, F, tree)
    assert np.array_equal(box.view(np.uint64), tree["box"].view(np.uint64))
    assert area > 0.0


@pytest.mark.parametrize("name", ["ellipsoid128", "plate", "spare_vertices", "one", "identical5"])
def test_new_vertices_against_numpy_and_containment(name):
    f, _ = _lib()
    V, F, leaves = MESHES[name]
    draws = 200 // len(leaves)
    for leaf in leaves:
        tree = f.mesh_bvh_host(V, F, leaf)
        nn = len(tree["skip"])
        for seed in range(draws):
            Vn = rc.deform(V, "random", seed) if seed >= len(rc.DEFORMS) else rc.deform(V, rc.DEFORMS[seed])
            box, area = f.mesh_bvh_refit_host(Vn, F, tree)
            want, want_area = rc.refit_numpy(Vn, F, tree)
            assert np.array_equal(box, want)
            assert abs(area - want_area) <= 1e-12 * want_area
            for i in range(nn):
                # every vertex of every triangle below node i: the slots first .. of the leaves i .. skip[i] - 1
                sub = np.arange(i, tree["skip"][i])
                sub = sub[tree["count"][sub] > 0]
                lo, hi = int(tree["first"][sub[0]]), int(tree["first"][sub[-1]] + tree["count"][sub[-1]])
                pts = Vn[F[tree["order"][lo:hi]]].reshape(-1, 3)
                assert np.all(pts >= box[i, :3]) and np.all(pts <= box[i, 3:])
                if tree["count"][i] == 0:
                    for c in (i + 1, int(tree["skip"][i + 1])):
                        assert np.all(box[c, :3] >= box[i, :3]) and np.all(box[c, 3:] <= box[i, 3:])


def test_area_sum():
    """The area sum against numpy to 1e-12 relative on the large tree, and what area_build = 0 means: the widening of a box is
    16 ulps of its largest magnitude and never 0, so the sum is 0 only where every product underflows -- a mesh whose vertices all
    lie at the origin.  A degenerate triangle anywhere else has a small positive area sum; the ratio area_now / area_build is not
    formed for area_build = 0 (include/bhgeo.h)."""
    f, _ = _lib()
    V, F, _ = MESHES["sphere4097"]
    tree = f.mesh_bvh_host(V, F, 1)
    for kind in ("noise", "permute"):
        Vn = rc.deform(V, kind)
        box, area = f.mesh_bvh_refit_host(Vn, F, tree)
        want = rc.refit_numpy(Vn, F, tree)[1]
        print(f"{kind}: area {area:.17g}, numpy {want:.17g}")
        assert abs(area - want) <= 1e-12 * want
    # a permuted mesh's boxes overlap far more than the built tree's: the figure the rebuild decision reads
    assert area > 5.0 * f.mesh_bvh_refit_host(V, F, tree)[1]
    one = np.array([[0, 1, 2]], np.int32)
    tree1 = f.mesh_bvh_host(np.zeros((3, 3)), one, 4)
    assert f.mesh_bvh_refit_host(np.zeros((3, 3)), one, tree1)[1] == 0.0
    point = np.tile([[1.0, 0.0, 0.0]], (3, 1))
    w = 2.0 * rc.ULP16
    assert f.mesh_bvh_refit_host(point, one, tree1)[1] == 3.0 * w * w


@pytest.mark.parametrize("name,leaf", TREES, ids=[f"{n}-leaf{k}" for n, k in TREES])
def test_schedule(name, leaf):
    f, _ = _lib()
    V, F, _ = MESHES[name]
    tree = f.mesh_bvh_host(V, F, leaf)
    nodes, off = f.mesh_refit_schedule_host(tree)
    inner = np.flatnonzero(tree["count"] == 0)
    assert sorted(nodes.tolist()) == inner.tolist()                 # every inner node exactly once
    assert off[0] == 0 and off[-1] == len(nodes) and np.all(np.diff(off) >= 0)
    # the walk: levels deepest first; a node's children are leaves or were done on an earlier (deeper) level
    done = tree["count"] > 0
    for d in range(len(off) - 2, -1, -1):
        level = nodes[off[d]:off[d + 1]]
        for i in level:
            assert done[i + 1] and done[tree["skip"][i + 1]]
        done[level] = True
    assert done.all()


def test_refusals_without_a_device():
    f, L = _lib()
    V, F, _ = MESHES["ellipsoid128"]
    tree = f.mesh_bvh_host(V, F, 4)
    err = lambda: L.bhg_last_error()     # noqa: E731
    # the calls on a mesh: a NULL mesh comes before the context
    assert L.bhg_mesh_refit(None, None, V.ctypes.data, None) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_refit_device(None, None, 64, None, None) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_refit_info(None, None, None, None) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_boxes_host(None, None, None, 0) == f.E_INVALID and b"mesh is NULL" in err()
    assert L.bhg_mesh_range(None, None, None) == f.E_INVALID and b"mesh is NULL" in err()
    # bhg_mesh_bvh_refit_host: the vertices and triangles as bhg_mesh_create refuses them
    bad = V.copy()
    bad[7, 1] = np.nan
    with pytest.raises(f.BhgError, match="every vertex must be finite"):
        f.mesh_bvh_refit_host(bad, F, tree)
    with pytest.raises(f.BhgError, match="outside"):
        f.mesh_bvh_refit_host(V[:-1], F, tree)
    # ... and a topology that is no tree over these triangles
    for key, i, value, what in (("skip", 3, 2, "node_skip"), ("skip", 0, len(tree["skip"]) + 1, "node_skip"), ("order", 5, len(F), "tri_order"),
                                ("order", 5, -1, "tri_order"), ("count", int(np.flatnonzero(tree["count"] > 0)[0]), 1000, "leaves"),
                                ("first", int(np.flatnonzero(tree["count"] > 0)[2]), 0, "leaves"),
                                ("count", int(np.flatnonzero(tree["count"] > 0)[-1]), 0, "inner node")):
        broken = {k: v.copy() for k, v in tree.items()}
        broken[key][i] = value
        with pytest.raises(f.BhgError, match=what):
            f.mesh_bvh_refit_host(V, F, broken)
    with pytest.raises(f.BhgError, match="leaves"):
        f.mesh_bvh_refit_host(V, F[:-1], tree)                      # a tree over more slots than triangles
    box = np.empty((len(tree["skip"]), 6))
    args = [a.ctypes.data for a in (tree["skip"], tree["first"], tree["count"], tree["order"])]
    assert L.bhg_mesh_bvh_refit_host(V.ctypes.data, len(V), F.ctypes.data, len(F), *args, len(tree["skip"]), None, None) == f.E_INVALID
    assert b"node_box is NULL" in err()
    assert L.bhg_mesh_bvh_refit_host(V.ctypes.data, len(V), F.ctypes.data, len(F), None, *args[1:], len(tree["skip"]), box.ctypes.data, None) == f.E_INVALID
    assert b"array is NULL" in err()
    # Mesh.refit looks at its arrays before the library does
    m = f.Mesh.__new__(f.Mesh)
    m.n_vertices, m._h = len(V), None
    with pytest.raises(ValueError, match="shape"):
        m.refit(V[:-1])


# ---- the conditions of the GPU test's cases, on the CPU ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as oc
    return oc


def test_trace_cases_meet_the_mesh(oracle):
    """Every deformation leaves at least MIN_HITS of the 2 048 rays on the mesh (one form, both scenes: the count barely depends
    on the form), so that the bit-for-bit equality of the GPU test compares hits."""
    V, F = rc.trace_mesh()
    k0 = rc.trace_rays()
    for scene, par in rc.SCENES.items():
        for kind in rc.DEFORMS:
            o = oracle.trace_mesh(k0, mo.FRAME_CAM, rc.deform(V, kind), F, rc.CHORD, rhs_form=1, spin=0.0, **par)
            hits = int((o["tri"] >= 0).sum())
            print(f"{scene} {kind}: {hits} hits, {len(set(o['tri'][o['tri'] >= 0]))} triangles")
            assert hits >= rc.MIN_HITS


@pytest.mark.parametrize("form", sorted(rc.FORMS))
def test_oracle_alone_is_stable_on_its_cases(oracle, form):
    case = rc.oracle_case(form)
    o = mo.oracle_solve(oracle, case)
    unstable = float((~o["stable"]).mean())
    print(f"{form}: {int((o['tri'] >= 0).sum())} hits, {unstable:.2%} of the rays unstable in the oracle alone")
    assert unstable <= mo.UNSTABLE_CAP and (o["tri"] >= 0).sum() >= rc.MIN_HITS


# ---- the add-on's rule on the stub bpy ---------------------------------------------------------------------------------------
def _addon(monkeypatch, **props):
    """The stub scene of the mesh tests on a recording frame that also records refit_mesh -> (engine, depsgraph, cube, calls())."""
    import test_mesh_material_host as tm
    from blackhole_geodesic_calculator_amd import _ffi

    class Recording(tm._RecordingFrame):
        def refit_mesh(self, vertices, vertex_normals=None, rebuild_ratio=None):
            self.calls.append(("refit", vertices, vertex_normals, rebuild_ratio))

    bpy, depsgraph, addon, cube, tetra = tm.mesh_scene(width=8, height=8, samples=1, device_shading=1.0, curved_space_meshes=1.0, **props)
    eng = tm._device_engine(monkeypatch, addon, depsgraph)
    monkeypatch.setattr(_ffi, "Frame", Recording)
    eng.device_shading = True
    buf = np.ones((8, 8, 4))

    def render():
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
        return [c[0] for c in tm._RecordingFrame.made[-1].calls if c[0] in ("mesh", "refit")], tm._RecordingFrame.made[-1].calls

    return eng, addon, cube, render


def _move_a_vertex(cube, by=0.25):
    v = cube._mesh.vertices[6]
    v.co = (v.co[0] + by, v.co[1], v.co[2] + by)


def test_addon_refits_when_only_vertex_positions_differ(monkeypatch):
    eng, addon, cube, render = _addon(monkeypatch, curved_space_mesh_refit=1.0)
    assert render()[0] == ["mesh"] and eng.device_mesh_action == "set"
    assert render()[0] == ["mesh"] and eng.device_mesh_action == "kept"           # unchanged: nothing goes up
    _move_a_vertex(cube)
    kinds, calls = render()
    assert kinds == ["mesh", "refit"] and eng.device_mesh_action == "refit"
    first, refit = [c for c in calls if c[0] in ("mesh", "refit")]
    assert refit[1].shape == first[1].shape and not np.array_equal(refit[1], first[1]) and refit[2] is None
    assert np.array_equal(refit[1][:6], first[1][:6]) and np.array_equal(refit[1][7:], first[1][7:])
    # the frame now holds the moved vertices: the same scene again is kept, another move is another refit
    assert render()[0] == ["mesh", "refit"] and eng.device_mesh_action == "kept"
    _move_a_vertex(cube, -0.1)
    assert render()[0] == ["mesh", "refit", "refit"]
    addon.release_device_frames()


def test_addon_takes_the_full_path_otherwise(monkeypatch):
    import fake_bpy_mesh as fbm
    # a moved vertex with the switch off
    eng, addon, cube, render = _addon(monkeypatch)
    assert render()[0] == ["mesh"]
    _move_a_vertex(cube)
    assert render()[0] == ["mesh", "mesh"] and eng.device_mesh_action == "set"
    addon.release_device_frames()
    # the switch on: a changed triangle index (a quad's fan starts at another corner), with and without a moved vertex
    eng, addon, cube, render = _addon(monkeypatch, curved_space_mesh_refit=1.0)
    assert render()[0] == ["mesh"]
    polys = cube._mesh._polys
    polys[2] = polys[2][1:] + polys[2][:1]
    assert render()[0] == ["mesh", "mesh"]
    _move_a_vertex(cube)
    polys[3] = polys[3][1:] + polys[3][:1]
    assert render()[0] == ["mesh", "mesh", "mesh"]
    # a changed vertex count: one more vertex that no polygon names
    old = cube._mesh
    verts = [v.co for v in old.vertices] + [(0.0, 0.0, 3.0)]
    uv = np.array([d.uv for d in old.uv_layers.active.data], np.float32)
    cube._mesh = fbm.FakeMesh(verts, list(polys), uv)
    assert render()[0] == ["mesh", "mesh", "mesh", "mesh"] and eng.device_mesh_action == "set"
    # a changed emission beside a moved vertex
    _move_a_vertex(cube)
    cube["curved_space_emission"] = 0.75
    assert render()[0] == ["mesh"] * 5
    # and after all that a moved vertex alone refits
    _move_a_vertex(cube)
    assert render()[0] == ["mesh"] * 5 + ["refit"]
    addon.release_device_frames()

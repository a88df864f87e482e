"""The mesh material and meshes on the library-owned frame without a GPU: the C ABI's additions, the numpy
restatement of the texel on known answers, the refusals that need no device, and the add-on's mesh extraction on the stub bpy."""
import ctypes as C
import importlib
import os
import re
import sys
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_bpy  # noqa: E402
import fake_bpy_mesh as fbm  # noqa: E402
import mesh_material_reference as mmr  # noqa: E402

NEW = ("bhg_mesh_material_size", "bhg_shade_mesh_material_device", "bhg_frame_set_mesh")


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------

def test_exports_macros_and_struct_size():
    f, L = _lib()
    assert L.bhg_version() == f.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for sym in NEW:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in f.EXPORTS
        getattr(L, sym)
    # every prototype of the header is an export of the binding's list and the other way round
    declared = set(re.findall(r"^(?:[a-z_0-9]+ \**)+(bhg_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(f.EXPORTS), declared ^ set(f.EXPORTS)
    assert re.search(r"#define BHG_MESH_MATERIAL 1\b", header)
    assert int(re.search(r"#define BHG_MESH_TEXTURES_MAX (\d+)", header).group(1)) == f.MESH_TEXTURES_MAX == 8
    assert "typedef struct bhg_mesh_material" in header
    assert L.bhg_mesh_material_size() == C.sizeof(f.MeshMaterialStruct) == 3 * 8 + 8 * 8 + 2 * 8 * 4 + 8 + 8


def test_refusals_that_need_no_device():
    """The material is checked before the context: each refusal names its field."""
    f, L = _lib()
    scene = f.make_scene(1, 4, 2)

    def call(m):
        rc = L.bhg_shade_mesh_material_device(None, None, None, None, None, 4, 1, C.byref(scene), None, C.byref(m), None, None,
                                              None, None)
        return rc, L.bhg_last_error().decode()

    # (a NULL mesh is refused before the material is looked at)
    rc, msg = call(f.MeshMaterialStruct())
    assert rc == f.E_INVALID and "mesh is NULL" in msg
    # the frame's host-array form: a NULL frame first
    assert L.bhg_frame_set_mesh(None, None, 0, None, 0, None, 4, 0.0, None) == f.E_INVALID
    with pytest.raises(ValueError):
        f.MeshMaterial(tri_uv=np.zeros((4, 3, 3)))
    with pytest.raises(ValueError):
        f.MeshMaterial(textures=[np.zeros((2, 2, 4), np.float32)] * 9)
    with pytest.raises(ValueError):
        f.MeshMaterial(tri_rgb=np.zeros((3, 3))).check_triangles(4)


# ---- the restatement on known answers ------------------------------------------------------------------------------------

def test_texel_constant_image():
    img = np.tile(np.array([0.25, 0.5, 0.75, 0.1], np.float32), (5, 7, 1))
    rng = np.random.default_rng(1)
    got = mmr.texel(img, rng.uniform(-3, 3, 200), rng.uniform(-3, 3, 200))
    assert np.abs(got - [0.25, 0.5, 0.75]).max() < 1e-15


def test_texel_centres_and_row_zero_is_v_zero():
    rng = np.random.default_rng(2)
    img = rng.random((3, 4, 4)).astype(np.float32)           # 4 wide, 3 high
    ys, xs = np.meshgrid(np.arange(3), np.arange(4), indexing="ij")
    got = mmr.texel(img, ((xs + 0.5) / 4).ravel(), ((ys + 0.5) / 3).ravel())
    assert np.array_equal(got, img[..., :3].astype(np.float64).reshape(-1, 3))
    assert np.array_equal(mmr.texel(img, [0.5 / 4], [0.5 / 3])[0], img[0, 0, :3].astype(np.float64))     # row 0 is V = 0


def test_texel_repeats():
    rng = np.random.default_rng(3)
    img = rng.random((5, 7, 4)).astype(np.float32)
    U, V = rng.uniform(0, 1, 300), rng.uniform(0, 1, 300)
    assert np.abs(mmr.texel(img, U + 3.0, V - 2.0) - mmr.texel(img, U, V)).max() < 1e-13


def test_texel_beyond_an_edge_blends_the_opposite_borders():
    rng = np.random.default_rng(4)
    img = rng.random((3, 4, 4)).astype(np.float32)
    t = img[..., :3].astype(np.float64)
    # U = 0 is half a texel left of the first column's centre: first and LAST column equally (row 1's centre)
    assert np.abs(mmr.texel(img, [0.0], [1.5 / 3])[0] - 0.5 * (t[1, 0] + t[1, 3])).max() < 1e-15
    assert np.abs(mmr.texel(img, [1.0], [1.5 / 3])[0] - 0.5 * (t[1, 0] + t[1, 3])).max() < 1e-15
    assert np.abs(mmr.texel(img, [2.5 / 4], [0.0])[0] - 0.5 * (t[0, 2] + t[2, 2])).max() < 1e-15


def test_texel_one_by_one():
    img = np.array([[[0.3, 0.6, 0.9, 1.0]]], np.float32)
    rng = np.random.default_rng(5)
    got = mmr.texel(img, rng.uniform(-5, 5, 100), rng.uniform(-5, 5, 100))
    assert np.abs(got - img[0, 0, :3].astype(np.float64)).max() < 1e-15


def test_albedo_slots_and_unclamped_corners():
    rng = np.random.default_rng(6)
    nt = 6
    uv = rng.uniform(-1.5, 2.5, (nt, 3, 2)).astype(np.float32)
    imgs = [rng.random((5, 7, 4)).astype(np.float32), rng.random((1, 1, 4)).astype(np.float32)]
    slot = np.array([-1, 0, 1, 0, -1, 1], np.int32)
    rgb = rng.random((nt, 3)).astype(np.float32)
    tri = np.arange(nt)
    bary = np.array([[0.2, 0.3], [1.0, 0.0], [0.0, 1.0], [-0.1, 0.4], [0.3, 0.3], [0.0, 0.0]])
    a = mmr.albedo(tri, bary, nt, rgb, uv, slot, imgs)
    assert np.array_equal(a[[0, 4]], rgb[[0, 4]].astype(np.float64))                  # no slot: the triangle colour alone
    assert np.abs(a[1] - rgb[1].astype(np.float64) * mmr.texel(imgs[0], [uv[1, 1, 0]], [uv[1, 1, 1]])[0]).max() < 1e-15   # corner 1
    assert np.abs(a[2] - rgb[2].astype(np.float64) * imgs[1][0, 0, :3]).max() < 1e-15
    U, V = mmr.hit_uv(tri[3:4], bary[3:4], uv)                                        # u < 0: extrapolated, not clamped
    c = uv[3].astype(np.float64)
    want = 0.7 * c[0] - 0.1 * c[1] + 0.4 * c[2]
    assert abs(U[0] - want[0]) < 1e-15 and abs(V[0] - want[1]) < 1e-15
    assert np.array_equal(mmr.albedo(tri, bary, nt, rgb), rgb.astype(np.float64))      # no UVs: no texel


# ---- the add-on on the stub bpy --------------------------------------------------------------------------------------------

BH_LOC = np.array([0.5, -1.0, 0.25])
CUBE_W = fbm.world((1.5, 0.5, 2.0), 0.6, (6.0, 1.0, 2.0))
TETRA_W = fbm.world((0.7, 0.7, 0.7), -0.3, (-4.0, 3.0, 1.0))


def mesh_scene(cube_w=CUBE_W, tetra_w=TETRA_W, **props):
    """The stub scene of the mesh tests: a textured cube, an untextured tetrahedron, the black-hole marker, a lamp."""
    bpy, depsgraph = fake_bpy.install(**props)
    addon = importlib.import_module("blackhole_geodesic_calculator_amd.blender_addon")
    bpy.data.images["crate.png"] = fake_bpy.FakeImage("/tmp/crate.png", width=8, height=4, seed=2)
    cube = fbm.cube(cube_w, curved_space_texture="crate.png")
    tetra = fbm.tetrahedron(tetra_w, curved_space_emission=0.5)
    marker = types.SimpleNamespace(type="MESH", location=tuple(BH_LOC), dimensions=(1.0, 1.0, 1.0))
    lamp = types.SimpleNamespace(type="LIGHT", location=(9.0, -6.0, 8.0))
    depsgraph.scene.objects[:] = [cube, lamp, marker, tetra]
    depsgraph.scene.blackhole_obj = marker
    return bpy, depsgraph, addon, cube, tetra


def test_addon_extracts_geometry_uvs_and_slots():
    bpy, depsgraph, addon, cube, tetra = mesh_scene(width=8, height=8, samples=1)
    eng = addon.RelativisticRenderEngine()
    eng.bh_loc = BH_LOC
    before = fbm._Coll.foreach_calls
    m = eng.scene_mesh(depsgraph)
    assert fbm._Coll.foreach_calls - before >= 9          # bulk reads, not element by element
    assert m["offsets"] == [(0, 0), (8, 12)]
    assert m["vertices"].shape == (12, 3) and m["triangles"].shape == (16, 3) and m["triangles"].dtype == np.int32
    cube_w = np.array(fbm.CUBE_V, float) @ CUBE_W[:3, :3].T + CUBE_W[:3, 3] - BH_LOC
    tetra_w = np.array(fbm.TETRA_V, float) @ TETRA_W[:3, :3].T + TETRA_W[:3, 3] - BH_LOC
    assert np.abs(m["vertices"][:8] - cube_w).max() < 1e-12 and np.abs(m["vertices"][8:] - tetra_w).max() < 1e-12
    # the quads as fans, the tetrahedron's faces shifted by the cube's 8 vertices
    assert m["triangles"][:2].tolist() == [[0, 3, 2], [0, 2, 1]]
    assert np.array_equal(m["triangles"][12:], np.array(fbm.TETRA_P) + 8)
    # per-corner UVs: loop k of quad f is row 4 f + k of the layer
    layer = np.array([d.uv for d in cube._mesh.uv_layers.active.data], np.float32)
    assert m["tri_uv"].shape == (16, 3, 2) and m["tri_uv"].dtype == np.float32
    assert np.array_equal(m["tri_uv"][0], layer[[0, 1, 2]]) and np.array_equal(m["tri_uv"][1], layer[[0, 2, 3]])
    assert np.array_equal(m["tri_uv"][11], layer[[20, 22, 23]])
    assert np.array_equal(m["tri_tex"], np.r_[np.zeros(12, np.int32), np.full(4, -1, np.int32)])
    assert m["images"] == ["crate.png"] and m["emission"] == 0.5
    assert m["normals"] is None                           # flat polygons: flat normals
    assert cube.cleared == 1 and tetra.cleared == 1
    for p in cube._mesh.polygons + tetra._mesh.polygons:
        p.use_smooth = True
    assert eng.scene_mesh(depsgraph)["normals"].shape == (12, 3)
    # more images than slots: a warning, the rest untextured
    for j in range(9):
        bpy.data.images[f"i{j}.png"] = fake_bpy.FakeImage(f"/tmp/i{j}.png", width=2, height=2, seed=j)
    depsgraph.scene.objects[:] = [fbm.cube(fbm.world((1, 1, 1), 0.0, (3.0 * j, 0, 9)), curved_space_texture=f"i{j}.png") for j in range(9)]
    with pytest.warns(RuntimeWarning, match="distinct curved_space_texture"):
        many = eng.scene_mesh(depsgraph)
    assert len(many["images"]) == 8 and set(many["tri_tex"][-12:]) == {-1} and many["tri_tex"][-13] == 7


class _RecordingFrame:
    """_ffi.Frame's surface as ray_trace_device uses it."""
    made = []

    def __init__(self, devices, width, height, samples, **kw):
        self.calls, self.W, self.H = [], width, height
        _RecordingFrame.made.append(self)

    def set_camera(self, **kw):
        pass

    def set_scene(self, sky, **kw):
        self.calls.append(("scene", kw))

    def set_object_textures(self, **kw):
        self.calls.append(("textures", kw))

    def set_mesh(self, vertices=None, triangles=None, **kw):
        self.calls.append(("mesh", vertices, triangles, kw))

    def render(self, params):
        return np.zeros((self.H, self.W, 4), np.float32)

    def info(self):
        return {}

    def close(self):
        pass


def _device_engine(monkeypatch, addon, depsgraph):
    from blackhole_geodesic_calculator_amd import _ffi
    _RecordingFrame.made.clear()
    addon.release_device_frames()
    monkeypatch.setattr(_ffi, "Frame", _RecordingFrame)
    monkeypatch.setattr(_ffi, "device_count", lambda: 1)
    monkeypatch.delenv("BHGEO_DEVICES", raising=False)
    eng = addon.RelativisticRenderEngine()
    eng.bh_loc, eng.field_of_view_x, eng.field_of_view_y, eng.sampling_seed = BH_LOC, 0.6, 0.6, 42.0
    eng.max_integration_step, eng.int_depth_curve_end, eng.sky_image_path = np.inf, 50.0, ""
    eng.mark_y_min, eng.mark_y_max, eng.mark_x_min, eng.mark_x_max = 0, 8, 0, 8
    eng.GeoInt = types.SimpleNamespace(context=types.SimpleNamespace(device=0), params=lambda *a: None)
    return eng


def test_addon_off_passes_todays_spheres_and_on_passes_the_mesh(monkeypatch):
    bpy, depsgraph, addon, cube, tetra = mesh_scene(width=8, height=8, samples=1, curved_space_objects=1.0, device_shading=1.0)
    eng = _device_engine(monkeypatch, addon, depsgraph)
    eng.device_shading = True
    buf = np.ones((8, 8, 4))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    fr = _RecordingFrame.made[-1]
    scene = [c for c in fr.calls if c[0] == "scene"][-1][1]
    want = eng.scene_spheres(depsgraph)
    want[:, :3] -= BH_LOC
    assert len(want) == 2 and np.array_equal(scene["spheres"], want)            # the bounding spheres, as today
    assert not [c for c in fr.calls if c[0] == "mesh"]
    # on: no spheres, the triangles; the unchanged scene a second time sets no mesh
    depsgraph.scene.curved_space_meshes = 1.0
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    scene = [c for c in fr.calls if c[0] == "scene"][-1][1]
    assert scene["spheres"] is None and len(scene["lamps"]) == 1
    mesh_calls = [c for c in fr.calls if c[0] == "mesh"]
    assert len(mesh_calls) == 1
    m = eng.scene_mesh(depsgraph)
    assert np.array_equal(mesh_calls[0][1], m["vertices"]) and np.array_equal(mesh_calls[0][2], m["triangles"])
    mat = mesh_calls[0][3]["material"]
    assert np.array_equal(mat.tri_uv, m["tri_uv"]) and np.array_equal(mat.tri_tex, m["tri_tex"]) and mat.emission == 0.5
    assert len(mat.textures) == 1 and np.array_equal(mat.textures[0], bpy.data.images["crate.png"].array)
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    assert len([c for c in fr.calls if c[0] == "mesh"]) == 1
    # a moved object is a new mesh; the property off again turns the frame's mesh off
    cube.matrix_world = fbm.world((1.5, 0.5, 2.0), 0.6, (6.0, 1.5, 2.0))
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    assert len([c for c in fr.calls if c[0] == "mesh"]) == 2
    depsgraph.scene.curved_space_meshes = 0.0
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    assert [c for c in fr.calls if c[0] == "mesh"][-1][1] is None
    addon.release_device_frames()


@pytest.mark.parametrize("why", ["host_path", "mark_window"])
def test_addon_on_the_host_path_warns_once_and_renders_as_off(monkeypatch, why):
    from test_frame_host import StubIntegrator
    bpy, depsgraph, addon, cube, tetra = mesh_scene(width=8, height=8, samples=1, curved_space_meshes=1.0,
                                                    device_shading=0.0 if why == "host_path" else 1.0)

    def run(meshes):
        depsgraph.scene.curved_space_meshes = meshes
        eng = addon.RelativisticRenderEngine()
        eng.bh_loc, eng.field_of_view_x, eng.field_of_view_y, eng.sampling_seed = BH_LOC, 0.6, 0.6, 42.0
        eng.max_integration_step, eng.int_depth_curve_end = np.inf, 50.0
        eng.mark_y_min, eng.mark_y_max, eng.mark_x_min, eng.mark_x_max = (0, 8, 0, 8) if why == "host_path" else (2, 6, 0, 8)
        eng.device_shading = why != "host_path"
        eng.sky_tex_name = "none"
        eng.GeoInt = StubIntegrator()
        buf = np.ones((8, 8, 4))
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
        return buf

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        on = run(1.0)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and "curved_space_meshes" in str(w.message)]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        off = run(0.0)
    assert np.array_equal(on, off)

"""Mesh instances without a GPU: the ABI surface, the refusals (the transforms are checked before the mesh
and the context, so the library refuses them here too), the rigid-record helper, the world box of a rotated box, and the
conditions of the cases tests/test_gpu_mesh_instances.py compares with the oracle: on each of them the brute-force oracle on the
flattened mesh leaves at most mesh_oracle_cases.UNSTABLE_CAP of the rays unstable -- under the 1-2 ulp perturbations of k0 and
under three draws that scale every flattened vertex coordinate by 1 +- 1 ... 2e-16 -- and every instance is hit.

Measured when this was written (the C oracle, 2 048 rays from FRAME_CAM on three placements of the 128-triangle ellipsoid):
  form         hits   per instance    unstable (k0, vertices)   hit ends moved by the vertex draws
  christoffel  262    45 / 110 / 107  0, 0                      <= 2.0e-14
  reduced      262    45 / 110 / 107  0, 0                      <= 1.3e-14
  kerr +0.45   270    57 / 112 / 101  0, 0                      <= 1.2e-14
  kerr -0.45   256    39 / 108 / 109  0, 0                      <= 1.5e-14
The ring of 64 tetrahedra: 1 024 rays, 464 hits, at least 5 on every instance, none unstable."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mesh_instance_cases as mi
import mesh_oracle_cases as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


NEW = ("bhg_mesh_instances_create", "bhg_mesh_instances_set", "bhg_mesh_instances_destroy", "bhg_mesh_instances_info",
       "bhg_mesh_instance_box_host", "bhg_trace_mesh_instances_device", "bhg_trace_mesh_instances",
       "bhg_shade_mesh_instances_device", "bhg_frame_set_mesh_instances")


def test_exports_and_header():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_MESH_INSTANCES\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+BHG_MESH_INSTANCES_MAX\s+64\s*$", hdr, re.M)
    assert f.MESH_INSTANCES_MAX == 64
    assert L.bhg_version() == 10 and f.ABI_VERSION == 10
    for name in ("MeshInstances", "rigid_transform", "mesh_instance_box_host"):
        assert hasattr(f, name)
    for name in ("trace_mesh_instances", "trace_mesh_instances_device", "shade_mesh_instances_device"):
        assert hasattr(f.Context, name)
    assert hasattr(f.Frame, "set_mesh_instances")
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    assert hasattr(DeviceFrame, "set_mesh_instances")


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def _create_rc(T, n=None, mesh=None):
    f, L = _lib()
    T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    h = C.c_void_p(77)
    rc = L.bhg_mesh_instances_create(None, mesh, len(T) if n is None else n, None if T is None else T.ctypes.data, C.byref(h))
    assert h.value is None          # out is cleared whatever happens
    return rc, L.bhg_last_error()


def test_create_refuses_bad_transforms_before_mesh_and_context():
    f, _ = _lib()
    good = mi.three_placements()
    rc, why = _create_rc(good)
    assert rc == f.E_INVALID and b"mesh is NULL" in why          # the transforms passed
    for n in (0, -1, 65):
        rc, why = _create_rc(np.tile(mi.IDENTITY, (max(n, 1), 1)), n=n)
        assert rc == f.E_INVALID and b"n must be in [1, BHG_MESH_INSTANCES_MAX]" in why, n
    rc, why = _create_rc(np.tile(mi.IDENTITY, (64, 1)))
    assert b"mesh is NULL" in why                               # 64 is allowed
    rc, why = _create_rc(None, n=2)
    assert rc == f.E_INVALID and b"transforms is NULL" in why
    for entry, value in ((0, np.nan), (5, np.inf), (11, -np.inf)):
        bad = good.copy()
        bad[1, entry] = value
        rc, why = _create_rc(bad)
        assert rc == f.E_INVALID and b"transforms must be finite" in why
    # not orthonormal: a scale of 1 + 1e-8, a shear of 1e-8, float32 rounding
    for R in (np.eye(3) * (1.0 + 1e-8), np.eye(3) + 1e-8 * np.eye(3, k=1), mi.rotation((1, 2, 3), 0.4).astype(np.float32)):
        rc, why = _create_rc(mi.record(R, (1.0, 2.0, 3.0))[None, :])
        assert rc == f.E_INVALID and b"R^T R within 1e-9" in why
    # ... and just inside the bound
    rc, why = _create_rc(mi.record(np.eye(3) * (1.0 + 2e-10), (1.0, 2.0, 3.0))[None, :])
    assert b"mesh is NULL" in why
    # a reflection is orthonormal and has det -1
    rc, why = _create_rc(mi.record(np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))[None, :])
    assert rc == f.E_INVALID and b"det R > 0" in why
    L = f.load()
    assert L.bhg_mesh_instances_create(None, None, 1, mi.IDENTITY.ctypes.data, None) == f.E_INVALID and b"out is NULL" in L.bhg_last_error()


def test_trace_refusals_come_before_the_context():
    f, L = _lib()
    xs = (C.c_double * 3)(20.0, 0.0, 2.0)

    def device(p, inst=None, chord=0.25, tri=64, iid=64, bary=64):
        return L.bhg_trace_mesh_instances_device(None, C.byref(p), inst, chord, xs, None, 64, 16, 64, None, None, None, tri, iid, bary, None)

    def host(p, inst=None, chord=0.25, tri=64, iid=64, bary=64):
        return L.bhg_trace_mesh_instances(None, C.byref(p), inst, chord, 64, 1, 64, 16, 64, None, None, None, tri, iid, bary)

    for call in (device, host):
        assert call(f.make_params(method=f.METHOD_RK4)) == f.E_INVALID and b"DP5(4)" in L.bhg_last_error()
        assert call(f.make_params(time_like=1)) == f.E_INVALID and b"time_like" in L.bhg_last_error()
        assert call(f.make_params()) == f.E_INVALID and b"inst is NULL" in L.bhg_last_error()
    assert L.bhg_mesh_instances_set(None, mi.IDENTITY.ctypes.data) == f.E_INVALID and b"inst is NULL" in L.bhg_last_error()
    # the shade: a NULL set, whatever else is given
    sc = f.make_scene(64, 8, 4)
    rc = L.bhg_shade_mesh_instances_device(None, 64, 64, 64, 64, 64, 16, 1, C.byref(sc), None, None, None, 64, None, None, None)
    assert rc == f.E_INVALID and b"inst is NULL" in L.bhg_last_error()
    # the frame: a NULL frame
    assert L.bhg_frame_set_mesh_instances(None, 1, mi.IDENTITY.ctypes.data, None) == f.E_INVALID and b"frame is NULL" in L.bhg_last_error()
    assert L.bhg_mesh_instances_info(None, None, None) == f.E_INVALID
    L.bhg_mesh_instances_destroy(None)       # a no-op


def test_integrator_wants_a_mesh_with_instances():
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild.__new__(GeodesicIntegratorSchwarzschild)     # (no context: the checks come first)
    with pytest.raises(ValueError, match="mesh_instances goes with mesh="):
        gi.trace(np.array([[0.0, 1.0, 0.0]]), np.array([0.0, -10.0, 0.0]), mesh_instances=mi.IDENTITY)
    f, _ = _lib()
    with pytest.raises(ValueError, match=r"\[K, 12\]"):
        f._instance_transforms(np.zeros((2, 4, 4)))
    T = f._instance_transforms(np.concatenate([mi.rotation((1, 1, 0), 0.3), [[1.0], [2.0], [3.0]]], axis=1)[None])
    assert T.shape == (1, 12) and np.array_equal(T[0, 9:], [1.0, 2.0, 3.0]) and np.array_equal(T[0, :9].reshape(3, 3), mi.rotation((1, 1, 0), 0.3))


# ---- the rigid-record helper ---------------------------------------------------------------------------------------------------
def test_rigid_transform_of_a_float32_matrix_with_scale():
    f, _ = _lib()
    R = mi.rotation((0.3, -1.0, 0.5), 1.234)
    M = np.eye(4)
    M[:3, :3] = R * 2.5
    M[:3, 3] = (4.0, -1.5, 0.25)
    M32 = M.astype(np.float32)
    raw = M32[:3, :3].astype(np.float64) / 2.5
    assert np.abs(raw.T @ raw - np.eye(3)).max() > 1e-9            # what the C check would refuse
    rec = f.rigid_transform(M32)
    Rn = rec[:9].reshape(3, 3)
    assert np.abs(Rn.T @ Rn - np.eye(3)).max() < 1e-14 and np.linalg.det(Rn) > 0.0
    assert np.abs(Rn - R).max() < 1e-6
    assert np.array_equal(rec[9:], M32[:3, 3].astype(np.float64))
    rc, why = _create_rc(rec[None, :])
    assert b"mesh is NULL" in why                                  # ... and accepts now
    # the polar part: no other rotation is nearer to the scaled block
    rng = np.random.default_rng(2)
    A = M32[:3, :3].astype(np.float64)
    best = np.linalg.norm(A - 2.5 * Rn)
    for _ in range(20):
        other = mi.rotation(rng.normal(size=3), 1e-4) @ Rn
        assert np.linalg.norm(A - 2.5 * other) >= best
    with pytest.raises(ValueError, match="det"):
        f.rigid_transform(np.diag([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="4 x 4"):
        f.rigid_transform(np.eye(3))


# ---- the world box of a rotated box --------------------------------------------------------------------------------------------
def test_the_box_of_a_rotated_box_contains_every_rotated_vertex():
    f, _ = _lib()
    rng = np.random.default_rng(9)
    worst = np.inf
    for draw in range(200):
        scale = 10.0 ** rng.uniform(-3, 3)
        V = rng.normal(size=(50, 3)) * scale * rng.uniform(0.01, 1.0, 3) + rng.normal(size=3) * scale
        lo, hi = V.min(0), V.max(0)
        R = mi.rotation(rng.normal(size=3), rng.uniform(-np.pi, np.pi))
        t = rng.normal(size=3) * 10.0 ** rng.uniform(-2, 3)
        wb = f.mesh_instance_box_host(np.concatenate([lo, hi]), mi.record(R, t))
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        for P in (V, corners):
            W = P @ R.T + t
            assert np.all(W >= wb[:3]) and np.all(W <= wb[3:]), draw
            worst = min(worst, (W - wb[:3]).min(), (wb[3:] - W).min())
        # tight: some corner comes within rounding of every face
        Wc = corners @ R.T + t
        mag = max(np.abs(wb).max(), np.abs(t).max(), np.abs(lo).max(), np.abs(hi).max())
        assert np.all(Wc.min(0) - wb[:3] <= 64 * np.finfo(float).eps * mag) and np.all(wb[3:] - Wc.max(0) <= 64 * np.finfo(float).eps * mag)
    assert worst > 0.0
    # the identity leaves a box where it was, but for the widening
    wb = f.mesh_instance_box_host([-1.0, -2.0, -3.0, 1.0, 2.0, 3.0], mi.IDENTITY[0])
    assert np.all(wb[:3] < [-1.0, -2.0, -3.0]) and np.all(wb[3:] > [1.0, 2.0, 3.0]) and np.abs(wb - [-1, -2, -3, 1, 2, 3]).max() <= 17 * 3.0 * np.finfo(float).eps   # (16 ulps of the largest magnitude)


# ---- the cases of the GPU comparison -------------------------------------------------------------------------------------------
def test_flatten_numbers_triangles_by_instance():
    V, F = mi.ellipsoid()
    assert len(F) == 128
    T = mi.three_placements()
    Vf, Ff = mi.flatten(V, F, T)
    assert Vf.shape == (3 * len(V), 3) and Ff.shape == (3 * 128, 3)
    for j in range(3):
        R, t = T[j, :9].reshape(3, 3), T[j, 9:]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and np.linalg.det(R) > 0
        tri = Vf[Ff[j * 128 + 5]]
        assert np.allclose(tri, V[F[5]] @ R.T + t, rtol=0, atol=1e-15)


CASES = dict(mi.three_placement_cases(), ring=mi.ring_case(), bulge=mi.bulge_case())


@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_alone_is_stable_on_the_cases(oracle, name):
    case = CASES[name]
    o = mi.oracle_solve(oracle, case)
    n = len(case["k0"])
    per = mi.hits_per_instance(o, case)
    hit = o["tri"] >= 0
    print(f"{name}: {n} rays, {int(hit.sum())} hits, per instance min {per.min()} {per[:3]}, unstable k0 {int((~o['stable_k']).sum())}, "
          f"vertices {int((~o['stable_v']).sum())}, hit ends moved by the vertex draws <= {o['sens_v'][hit].max():.1e}")
    assert (~o["stable_k"]).sum() <= mo.UNSTABLE_CAP * n and (~o["stable_v"]).sum() <= mo.UNSTABLE_CAP * n
    assert (~o["stable"]).sum() <= mo.UNSTABLE_CAP * n
    if name == "ring":
        assert len(per) == 64 and per.min() >= 1
    elif name == "bulge":
        assert per[0] >= 15
    else:
        assert len(per) == 3 and per.min() >= mi.MIN_HITS_PER_INSTANCE
        cl = mo.classes(o)
        assert cl["disk"].sum() >= 100 and cl["horizon"].sum() >= 50 and cl["exit"].sum() >= 100


def test_the_bulge_case_needs_the_deviation(oracle):
    """At least 15 hits of the moved bulge case lie in a step whose two ends span a box that misses the instance's world box: only
    the dense output between them reaches it (the count of tests/test_mesh_oracle_host.py, against the box the device culls by)."""
    f, _ = _lib()
    case = mi.bulge_case()
    wb = f.mesh_instance_box_host(np.concatenate([case["Vl"].min(0), case["Vl"].max(0)]), case["T"][0])
    assert np.all(case["V"] >= wb[:3]) and np.all(case["V"] <= wb[3:])
    o = mo.oracle_run(oracle, case)
    bulge = 0
    for i in np.flatnonzero(o["tri"] >= 0):
        a = int(o["n_attempted"][i])
        ends = [oracle.trace(case["k0"][i:i + 1], case["x0"], rhs_form=case["rhs"], spin=case["spin"], **dict(case["par"], max_steps=b))
                for b in (a - 1, a) if b > 0]
        if len(ends) < 2 or ends[1]["n_attempted"][0] != a or ends[0]["flags"][0] != 16:
            continue
        c0, c1 = ends[0]["end"][0, :3], ends[1]["end"][0, :3]
        bulge += bool(np.any(np.minimum(c0, c1) - 1e-12 > wb[3:]) or np.any(np.maximum(c0, c1) + 1e-12 < wb[:3]))
    print(f"bulge hits: {bulge} of {int((o['tri'] >= 0).sum())}")
    assert bulge >= 15


# ---- the add-on on the stub bpy ------------------------------------------------------------------------------------------------
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

    def set_mesh_instances(self, transforms=None, inst_rgb=None):
        self.calls.append(("instances", None if transforms is None else np.array(transforms)))

    def render(self, params):
        return np.zeros((self.H, self.W, 4), np.float32)

    def info(self):
        return {}

    def close(self):
        pass


ADDON_BH = np.array([0.5, -1.0, 0.25])


def _rigid_world(axis, angle, scale, t):
    """A float32 matrix_world, as Blender keeps it: rotation times a per-axis scale, and a translation."""
    m = np.eye(4)
    m[:3, :3] = mi.rotation(axis, angle) * np.asarray(scale, float)
    m[:3, 3] = t
    return m.astype(np.float32).astype(np.float64)


def _addon_scene(worlds, **props):
    import importlib
    import types

    import fake_bpy
    import fake_bpy_mesh as fbm
    bpy, depsgraph = fake_bpy.install(width=8, height=8, samples=1, device_shading=1.0, curved_space_meshes=1.0, **props)
    addon = importlib.import_module("blackhole_geodesic_calculator_amd.blender_addon")
    first = fbm.cube(worlds[0], curved_space_emission=0.25)
    obs = [first] + [fbm.MeshObject(first._mesh, w, curved_space_emission=0.25) for w in worlds[1:]]
    for ob in obs:
        ob.data = first._mesh            # linked duplicates: one datablock
    marker = types.SimpleNamespace(type="MESH", location=tuple(ADDON_BH), dimensions=(1.0, 1.0, 1.0))
    lamp = types.SimpleNamespace(type="LIGHT", location=(9.0, -6.0, 8.0))
    depsgraph.scene.objects[:] = [obs[0], lamp, marker] + obs[1:]
    depsgraph.scene.blackhole_obj = marker
    return depsgraph, addon, obs, fbm


def _addon_engine(monkeypatch, addon):
    import types

    from blackhole_geodesic_calculator_amd import _ffi
    _RecordingFrame.made.clear()
    addon.release_device_frames()
    monkeypatch.setattr(_ffi, "Frame", _RecordingFrame)
    monkeypatch.setattr(_ffi, "device_count", lambda: 1)
    monkeypatch.delenv("BHGEO_DEVICES", raising=False)
    eng = addon.RelativisticRenderEngine()
    eng.bh_loc, eng.field_of_view_x, eng.field_of_view_y, eng.sampling_seed = ADDON_BH, 0.6, 0.6, 42.0
    eng.max_integration_step, eng.int_depth_curve_end, eng.sky_image_path = np.inf, 50.0, ""
    eng.mark_y_min, eng.mark_y_max, eng.mark_x_min, eng.mark_x_max = 0, 8, 0, 8
    eng.GeoInt = types.SimpleNamespace(context=types.SimpleNamespace(device=0), params=lambda *a: None)
    eng.device_shading = True
    return eng


SCALE = (1.5, 0.5, 2.0)
WORLDS = [_rigid_world((1.0, 2.0, 0.5), 0.7, SCALE, (6.0, 1.0, 2.0)), _rigid_world((0.0, 1.0, -1.0), 2.1, SCALE, (-4.0, 3.0, 1.0))]


def test_addon_linked_duplicates_become_instances_and_moving_them_sets_no_mesh(monkeypatch):
    import warnings
    depsgraph, addon, obs, fbm = _addon_scene(WORLDS, curved_space_mesh_instances=1.0)
    eng = _addon_engine(monkeypatch, addon)
    f, _ = _lib()
    buf = np.ones((8, 8, 4))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    fr = _RecordingFrame.made[-1]
    mesh_calls = [c for c in fr.calls if c[0] == "mesh"]
    inst_calls = [c for c in fr.calls if c[0] == "instances"]
    assert len(mesh_calls) == 1 and len(inst_calls) == 1
    # the datablock once, in its own coordinates with the scale baked in
    assert mesh_calls[0][1].shape == (8, 3) and mesh_calls[0][2].shape == (12, 3)
    assert np.abs(mesh_calls[0][1] - np.array(fbm.CUBE_V, float) * SCALE).max() < 1e-6
    assert mesh_calls[0][3]["material"].emission == 0.25
    # one instance per object: rigid to rounding (the C check passes), translation minus the hole's location, and the placed mesh
    # is where the concatenated path puts it
    T = inst_calls[0][1]
    assert T.shape == (2, 12)
    for j, w in enumerate(WORLDS):
        R = T[j, :9].reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.abs(T[j, 9:] - (w[:3, 3] - ADDON_BH)).max() == 0.0
        placed = mesh_calls[0][1] @ R.T + T[j, 9:]
        assert np.abs(placed - (np.array(fbm.CUBE_V, float) @ w[:3, :3].T + w[:3, 3] - ADDON_BH)).max() < 1e-6
    rc, why = _create_rc(T)
    assert b"mesh is NULL" in why
    # the unchanged scene: neither call again; moved objects: exactly one set_mesh_instances, no set_mesh
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    assert len([c for c in fr.calls if c[0] in ("mesh", "instances")]) == 2
    obs[0].matrix_world = _rigid_world((1.0, 2.0, 0.5), 0.9, SCALE, (6.0, 1.5, 2.0))
    obs[1].matrix_world = _rigid_world((0.3, 1.0, -1.0), 2.0, SCALE, (-4.0, 3.0, 1.4))
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    assert len([c for c in fr.calls if c[0] == "mesh"]) == 1
    moved = [c for c in fr.calls if c[0] == "instances"]
    assert len(moved) == 2 and np.abs(moved[1][1][0, 9:] - (np.array([6.0, 1.5, 2.0]) - ADDON_BH)).max() < 1e-6
    # a sheared object: the concatenated path of today, silently -- the world vertices of both objects, instances off
    shear = WORLDS[1].copy()
    shear[0, 1] += 0.3
    obs[1].matrix_world = shear
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    mesh_calls = [c for c in fr.calls if c[0] == "mesh"]
    assert len(mesh_calls) == 2 and mesh_calls[1][1].shape == (16, 3) and mesh_calls[1][2].shape == (24, 3)
    assert np.abs(mesh_calls[1][1][8:] - (np.array(fbm.CUBE_V, float) @ shear[:3, :3].T + shear[:3, 3] - ADDON_BH)).max() < 1e-12
    assert len([c for c in fr.calls if c[0] == "instances"]) == 2          # (set_mesh turned them off: no further call)
    addon.release_device_frames()


def test_addon_falls_back_without_the_property_other_datablocks_scales_or_looks(monkeypatch):
    depsgraph, addon, obs, fbm = _addon_scene(WORLDS)                      # the property at its default, 0
    eng = _addon_engine(monkeypatch, addon)
    m = eng.scene_mesh(depsgraph)
    assert m["instances"] is None and m["vertices"].shape == (16, 3)        # nothing changes
    depsgraph.scene.curved_space_mesh_instances = 1.0
    assert eng.scene_mesh(depsgraph)["instances"].shape == (2, 12)
    obs[1].data = object()                                                  # another datablock
    assert eng.scene_mesh(depsgraph)["instances"] is None
    obs[1].data = obs[0].data
    obs[1].matrix_world = _rigid_world((0.0, 1.0, -1.0), 2.1, (1.5, 0.5, 2.1), (-4.0, 3.0, 1.0))      # another scale
    assert eng.scene_mesh(depsgraph)["instances"] is None
    obs[1].matrix_world = WORLDS[1]
    obs[1]["curved_space_emission"] = 0.5                                   # another emission
    assert eng.scene_mesh(depsgraph)["instances"] is None
    obs[1]["curved_space_emission"] = 0.25
    mirrored = WORLDS[1].copy()
    mirrored[:3, 0] *= -1.0                                                 # a reflection
    obs[1].matrix_world = mirrored
    assert eng.scene_mesh(depsgraph)["instances"] is None
    # a single object needs no shared datablock
    depsgraph.scene.objects[:] = [o for o in depsgraph.scene.objects if o is not obs[1]]
    del obs[0].data
    one = eng.scene_mesh(depsgraph)
    assert one["instances"].shape == (1, 12) and one["vertices"].shape == (8, 3)


def test_addon_takes_the_full_path_for_other_evaluated_meshes_and_changed_datablocks(monkeypatch):
    depsgraph, addon, obs, fbm = _addon_scene(WORLDS, curved_space_mesh_instances=1.0)
    eng = _addon_engine(monkeypatch, addon)
    assert eng.scene_mesh(depsgraph)["instances"].shape == (2, 12)
    # a linked duplicate with a modifier of its own: the same datablock, another evaluated mesh
    taller = np.array(fbm.CUBE_V, float) * (1.0, 1.0, 1.5)
    modified = fbm.MeshObject(fbm.FakeMesh(taller, fbm.CUBE_P), WORLDS[1], curved_space_emission=0.25)
    modified.data = obs[0].data
    depsgraph.scene.objects[:] = [modified if o is obs[1] else o for o in depsgraph.scene.objects]
    m = eng.scene_mesh(depsgraph)
    assert m["instances"] is None and m["vertices"].shape == (16, 3)
    depsgraph.scene.objects[:] = [obs[1] if o is modified else o for o in depsgraph.scene.objects]
    # a held instanced mesh whose datablock changes by 1e-7 is a new mesh: set_mesh again, then the instances
    buf = np.ones((8, 8, 4))
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    fr = _RecordingFrame.made[-1]
    assert [c[0] for c in fr.calls if c[0] in ("mesh", "instances")] == ["mesh", "instances"]
    v = obs[0]._mesh.vertices[3]
    v.co = (v.co[0] * (1.0 + 1e-7), v.co[1], v.co[2])
    list(eng.ray_trace(depsgraph, 8, 8, 1, buf, 1))
    calls = [c for c in fr.calls if c[0] in ("mesh", "instances")]
    assert [c[0] for c in calls] == ["mesh", "instances", "mesh", "instances"]
    assert calls[2][1][3, 0] != calls[0][1][3, 0]
    addon.release_device_frames()

"""Textured, oriented and emissive object spheres without a GPU: the numpy restatement's mapping (tests/object_texture_reference.py,
DESIGN.md section 11), the C ABI's additions (exports, struct size, the header as C99 and C++), every refusal of
bhg_shade_scene_textured_device (the table is checked before the context), and the Blender add-on on the fake bpy."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fake_bpy  # noqa: E402
import object_texture_reference as otr  # noqa: E402

NEW = ("bhg_object_textures_size", "bhg_shade_scene_textured_device", "bhg_frame_set_object_textures")


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_mapping_poles_and_centre_column():
    U, V = otr.body_uv(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 1e-300, 0.0]]))
    assert U[0] == 0.0 and V[0] == 0.0           # body +x: the centre column, the equator
    assert V[1] == 1.0 and V[2] == -1.0          # body +z: the top row, -z the bottom row
    assert U[3] == 0.5                           # +y a quarter turn on, towards increasing U
    assert abs(U[4] - 1.0) < 1e-15               # -x: the seam


def test_rotation_about_body_z_shifts_u():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    U0, V0 = otr.body_uv(otr.body_normal(n, np.zeros((3, 3))))
    for psi in (0.3, -1.1, 2.5):
        # the sphere turned by psi about its body z (R_z(psi): body -> world) sees the world normal n at body angle phi - psi
        U, V = otr.body_uv(otr.body_normal(n, otr.rot_z(psi)))
        dU = np.mod(U0 - U + 1.0, 2.0) - 1.0
        assert np.abs(dU - psi / np.pi).max() < 1e-12
        assert np.abs(V - V0).max() < 1e-12


def test_zero_matrix_is_the_identity():
    rng = np.random.default_rng(4)
    n = rng.normal(size=(50, 3))
    assert np.array_equal(otr.body_normal(n, np.zeros((3, 3))), otr.body_normal(n, np.eye(3)))
    R = otr.random_rotation(rng)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    assert np.abs(otr.body_normal(n @ R.T, R) - n).max() < 1e-12     # world = R body, and back


def test_restated_colour_modes():
    """Lit: the lamp sum times sphere_rgb times the texel; emissive: the strength times sphere_rgb times the texel, no lamps;
    without a texture a lit sphere is oracle.shade_reference.object_colour."""
    from oracle import shade_reference as sh
    rng = np.random.default_rng(5)
    spheres = np.array([[5.0, 1.0, 2.0, 1.5], [-4.0, 3.0, 0.0, 1.0]])
    rgb = np.array([[1.0, 0.5, 0.25], [0.2, 0.9, 0.4]])
    lamps = [[20.0, 0.0, 10.0, 8.0]]
    idx = rng.integers(0, 2, 200)
    n = rng.normal(size=(200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    end = np.concatenate([spheres[idx, :3] + spheres[idx, 3:4] * n, np.zeros((200, 3))], 1)
    plain = otr.object_colour_textured(end, idx, spheres, rgb, lamps, otr.Textures())
    assert np.array_equal(plain, sh.object_colour(end, idx, spheres, rgb, lamps))
    tex = rng.random((8, 16, 4)).astype(np.float32)
    T = otr.Textures(tex=[tex, tex], mode=[otr.LIT, otr.EMISSIVE], emission=[0.0, 3.0])
    got = otr.object_colour_textured(end, idx, spheres, rgb, lamps, T)
    U, V = otr.body_uv(n)
    texel = sh.sky_lookup(tex, U, V)
    lit, em = idx == 0, idx == 1
    assert np.abs(got[lit] - plain[lit] * texel[lit]).max() < 1e-13
    assert np.abs(got[em] - 3.0 * rgb[1] * texel[em]).max() < 1e-13     # (n of the restatement against n of the test)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------

def test_exports_and_struct_size():
    f, L = _lib()
    assert L.bhg_object_textures_size() == C.sizeof(f.ObjectTextures) == 800
    assert L.bhg_version() == f.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for sym in NEW:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in f.EXPORTS
        getattr(L, sym)
    assert "typedef struct bhg_object_textures" in header
    assert re.search(r"#define BHG_OBJECT_TEXTURES 1\b", header)


def test_header_struct_compiles_as_c99_and_cxx(tmp_path):
    f, _ = _lib()
    src = tmp_path / "ot.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bhgeo.h"\n'
                   'int main(void) { bhg_object_textures ot = {0}; ot.mode[0] = BHG_OBJECT_EMISSIVE; ot.rot[7][8] = 1.0;\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(ot), offsetof(bhg_object_textures, tex_w),\n'
                   '         offsetof(bhg_object_textures, tex_h), offsetof(bhg_object_textures, mode),\n'
                   '         offsetof(bhg_object_textures, emission), offsetof(bhg_object_textures, rot), BHG_OBJECT_TEXTURES,\n'
                   '         BHG_OBJECT_LIT, ot.mode[0]); return 0; }\n')
    exe = tmp_path / "ot"
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-x", "c++", "-fsyntax-only", str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    O = f.ObjectTextures
    assert out[:6] == [C.sizeof(O), O.tex_w.offset, O.tex_h.offset, O.mode.offset, O.emission.offset, O.rot.offset]
    assert out[6:] == [1, f.OBJECT_LIT, f.OBJECT_EMISSIVE]


def _scene(n_spheres):
    f, _ = _lib()
    sp = [[5.0 + j, 0.0, 1.0, 1.0] for j in range(n_spheres)]
    return f.make_scene(0, 16, 8, spheres=sp if n_spheres else None, lamps=[[10.0, 0.0, 10.0, 5.0]])


def _shade_null_ctx(ot, n_spheres=3):
    f, L = _lib()
    return L.bhg_shade_scene_textured_device(None, None, None, None, None, 64, 1, C.byref(_scene(n_spheres)), None, None, None,
                                             None if ot is None else C.byref(ot), None, None, None, None, None, None)


def _good(n=3):
    f, _ = _lib()
    rng = np.random.default_rng(8)
    rots = [otr.random_rotation(rng) for _ in range(n)]
    return f.make_object_textures(textures=[(0x1000, 4, 2)] * n, rotations=rots, modes=["lit", "emissive", "lit"][:n],
                                  emission=[0.0, 2.5, 0.0][:n])[0]


@pytest.mark.parametrize("what,edit", [
    ("mode", lambda ot: ot.mode.__setitem__(2, 2)),
    ("mode", lambda ot: ot.mode.__setitem__(1, -1)),
    ("emission", lambda ot: ot.emission.__setitem__(1, -0.5)),
    ("emission", lambda ot: ot.emission.__setitem__(0, float("nan"))),
    ("emission", lambda ot: ot.emission.__setitem__(2, float("inf"))),
    ("texture size", lambda ot: ot.tex_w.__setitem__(1, 0)),
    ("texture size", lambda ot: ot.tex_h.__setitem__(2, -3)),
    ("rotation", lambda ot: ot.rot[0].__setitem__(0, ot.rot[0][0] * 1.001)),
    ("rotation", lambda ot: [ot.rot[2].__setitem__(q, -ot.rot[2][q]) for q in range(9)]),    # det -1
    ("rotation", lambda ot: ot.rot[1].__setitem__(4, float("nan"))),
])
def test_refusals_name_the_sphere(what, edit):
    f, L = _lib()
    ot = _good()
    assert _shade_null_ctx(ot) == f.E_INVALID and "ctx is NULL" in L.bhg_last_error().decode()   # the good table passes
    edit(ot)
    rc = _shade_null_ctx(ot)
    msg = L.bhg_last_error().decode()
    assert rc == f.E_INVALID
    j = int(re.search(r"sphere (\d+)", msg).group(1))
    assert "object textures" in msg and "ctx" not in msg, msg
    bad = {"mode": lambda: ot.mode[j] not in (0, 1), "emission": lambda: not (np.isfinite(ot.emission[j]) and ot.emission[j] >= 0),
           "texture size": lambda: ot.tex_w[j] < 1 or ot.tex_h[j] < 1,
           "rotation": lambda: True}[what]
    assert bad(), msg


def test_untextured_slot_size_and_high_slots_are_not_checked():
    f, L = _lib()
    ot = _good()
    ot.tex[1], ot.tex_w[1], ot.tex_h[1] = None, 0, 0     # no texture: its size is not looked at
    ot.mode[5], ot.emission[6], ot.rot[7][0] = 9, -1.0, 3.0   # slots at or above n_spheres are ignored
    assert _shade_null_ctx(ot) == f.E_INVALID and "ctx is NULL" in L.bhg_last_error().decode()
    assert _shade_null_ctx(f.ObjectTextures()) == f.E_INVALID and "ctx is NULL" in L.bhg_last_error().decode()
    ot.mode[2] = 4
    assert _shade_null_ctx(ot, n_spheres=2) == f.E_INVALID and "ctx is NULL" in L.bhg_last_error().decode()
    assert _shade_null_ctx(ot, n_spheres=3) == f.E_INVALID and "sphere 2" in L.bhg_last_error().decode()
    # ot = NULL: no table to check, and the call gets as far as the missing context
    assert _shade_null_ctx(None) == f.E_INVALID and "ctx is NULL" in L.bhg_last_error().decode()
    assert L.bhg_frame_set_object_textures(None, C.byref(ot)) == f.E_INVALID
    assert "frame" in L.bhg_last_error().decode()


def test_make_object_textures():
    f, _ = _lib()
    tex = np.zeros((3, 5, 4), np.float32)
    ot, keep = f.make_object_textures(textures=[None, tex], rotations=[None, np.eye(3)], modes=["lit", "emissive"], emission=[0, 2])
    assert ot.tex[0] is None and ot.tex[1] == keep[0].ctypes.data and (ot.tex_w[1], ot.tex_h[1]) == (5, 3)
    assert list(ot.rot[0]) == [0.0] * 9 and list(ot.rot[1]) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert list(ot.mode)[:2] == [0, 1] and list(ot.emission)[:2] == [0.0, 2.0]
    with pytest.raises(ValueError):
        f.make_object_textures(textures=[None] * 9)
    with pytest.raises(ValueError):
        f.make_object_textures(textures=[np.zeros((4, 4), np.float32)])


# ---- the Blender add-on --------------------------------------------------------------------------------------------------

class _Ob(dict):
    """A mesh object with custom properties (ob["key"], ob.get("key"))."""

    def __init__(self, location, dimensions, matrix_world=None, **custom):
        super().__init__(custom)
        self.type, self.location, self.dimensions = "MESH", location, dimensions
        if matrix_world is not None:
            self.matrix_world = matrix_world


class _FakeFrame:
    def __init__(self):
        self.calls = []

    def set_object_textures(self, textures=None, rotations=None, modes=None, emission=None):
        self.calls.append(dict(textures=textures, rotations=rotations, modes=modes, emission=emission))


def _addon(**props):
    bpy, depsgraph = fake_bpy.install(width=8, height=8, samples=1, curved_space_objects=1.0, **props)
    addon = importlib.import_module("blackhole_geodesic_calculator_amd.blender_addon")
    return bpy, depsgraph, addon


def test_addon_reads_texture_emission_and_orientation():
    bpy, depsgraph, addon = _addon()
    bpy.data.images["moon.png"] = fake_bpy.FakeImage("/tmp/moon.png", width=8, height=4, seed=2)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    mw = np.eye(4)
    mw[:3, :3] = rot * np.array([2.0, 0.5, 3.0])          # scaled columns
    mw[:3, 3] = [6.0, 0.0, 1.0]
    moon = _Ob((6.0, 0.0, 1.0), (2.0, 2.0, 2.0), mw, curved_space_texture="moon.png")
    star = _Ob((-9.0, 2.0, 0.0), (3.0, 3.0, 3.0), None, curved_space_emission=4.0)
    plain = _Ob((12.0, 0.0, 0.0), (1.0, 1.0, 1.0), np.eye(4))
    depsgraph.scene.objects[:] = [plain, star, moon]
    eng = addon.RelativisticRenderEngine()
    eng.bh_loc = np.zeros(3)
    sph = eng.scene_spheres(depsgraph)
    assert np.allclose(sph[:, 3], [1.0, 1.5, 0.5])       # nearest first: moon, star, plain
    looks = eng.sphere_looks()
    assert looks[0]["image"] == "moon.png" and looks[0]["emission"] == 0.0
    assert np.abs(looks[0]["rot"] - rot).max() < 1e-15    # the scale is gone
    assert looks[1]["image"] is None and looks[1]["emission"] == 4.0 and not looks[1]["rot"].any()
    assert looks[2]["image"] is None and looks[2]["emission"] == 0.0 and np.array_equal(looks[2]["rot"], np.eye(3))
    # the device path: the image's pixels once, the rotation, the modes and strengths; a second render uploads nothing
    eng._sphere_looks = looks
    fr = _FakeFrame()
    eng._set_device_object_textures(fr)
    call = fr.calls[-1]
    assert np.array_equal(call["textures"][0], bpy.data.images["moon.png"].array)
    assert call["modes"] == ["lit", "emissive", "lit"] and call["emission"] == [0.0, 4.0, 0.0]
    assert np.abs(call["rotations"][0] - rot).max() < 1e-15
    assert eng.device_object_images_uploaded >= 1
    eng._set_device_object_textures(fr)
    assert fr.calls[-1]["textures"][0] is None and eng.device_object_images_uploaded == 0
    # the host path: the texel through the IMAGE texture's evaluate at the body normal's (U, V); emissive ignores the lamps
    eng.lamps = [types.SimpleNamespace(type="LIGHT", location=(20.0, 0.0, 5.0))]
    eng._lit_spheres = sph
    rng = np.random.default_rng(9)
    n = rng.normal(size=(60, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    idx = np.repeat([0, 1, 2], 20)
    loc = sph[idx, :3] + sph[idx, 3:4] * n
    got = eng.spacetime_hit_many(loc, n, idx)
    eng._sphere_looks = []
    white = eng.spacetime_hit_many(loc, n, idx)
    tex = bpy.data.textures["moon.png_tex"]
    assert tex.image is bpy.data.images["moon.png"]
    U, V = otr.body_uv(otr.body_normal(n[:20], rot))
    texel = np.array([tex.evaluate((u, v, 0)).xyz for u, v in zip(U, V)])
    assert np.abs(got[:20] - white[:20] * texel).max() < 1e-15
    assert np.array_equal(got[20:40], np.full((20, 3), 4.0))
    assert np.array_equal(got[40:], white[40:])


def test_addon_without_properties_is_todays_scene():
    bpy, depsgraph, addon = _addon()
    depsgraph.scene.objects[:] = [types.SimpleNamespace(type="MESH", location=(6.0, 0.0, 1.0), dimensions=(2.0, 2.0, 2.0)),
                                  _Ob((-8.0, 0.0, 0.0), (1.0, 1.0, 1.0), np.eye(4))]
    eng = addon.RelativisticRenderEngine()
    eng.bh_loc = np.zeros(3)
    eng.scene_spheres(depsgraph)
    eng._sphere_looks = eng.sphere_looks()
    assert all(l["image"] is None and l["emission"] == 0.0 for l in eng._sphere_looks)
    fr = _FakeFrame()
    eng._set_device_object_textures(fr)
    assert fr.calls == [dict(textures=None, rotations=None, modes=None, emission=None)]     # textures off
    eng.lamps = [types.SimpleNamespace(type="LIGHT", location=(20.0, 0.0, 5.0))]
    eng._lit_spheres = np.array([[6.0, 0.0, 1.0, 1.0], [-8.0, 0.0, 0.0, 0.5]])
    n = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    loc = eng._lit_spheres[[0, 1], :3] + eng._lit_spheres[[0, 1], 3:4] * n
    with_looks = eng.spacetime_hit_many(loc, n, np.array([0, 1]))
    eng._sphere_looks = []
    assert np.array_equal(with_looks, eng.spacetime_hit_many(loc, n, np.array([0, 1])))

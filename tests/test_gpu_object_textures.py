"""Textured, oriented and emissive object spheres on the GPU: the textured shade instances against the
numpy restatement (tests/object_texture_reference.py) for both Schwarzschild forms and Kerr with redshift off, on and on with an
observer; ot = NULL and a zero-initialised ot bit for bit the untextured call; every other shade entry point bit for bit the
general call, and an empty call accepted by each; a traced sphere whose texture encodes (U, V);
the library-owned frame on one device and on the {0, 0} loopback against DeviceFrame, rotation-only updates and textures off."""
import os
import sys

import numpy as np
import pytest

from conftest import CAM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_texture_reference as otr  # noqa: E402
import observer_reference as orf  # noqa: E402
import redshift_reference as rr  # noqa: E402

INC = np.radians(75.0)
CAM3 = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])
SPHERES = np.array([[6.0, 3.0, 2.5, 1.5], [7.0, -4.0, 3.0, 1.0], [2.0, 6.0, -1.0, 1.2]])
RGB = np.array([[1.0, 0.8, 0.6], [0.2, 0.9, 0.3], [0.5, 0.5, 1.0]])
LAMPS = [[20.0, 0.0, 20.0, 10.0], [10.0, -15.0, 5.0, 6.0]]
DISK = (3.0, 9.0)
PROFILE = dict(disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
BETA = np.array([0.1, -0.25, 0.05])


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(n, seed):
    """Synthetic end records: object entry points on the three spheres, disk hits, sky and horizon rays, mixed at random."""
    rng = np.random.default_rng(seed)
    cls = rng.choice(4, n, p=[0.5, 0.2, 0.2, 0.1])      # object, disk, sky, horizon
    end = np.zeros((n, 6))
    flags = np.zeros(n, np.uint8)
    obj = np.full(n, -1, np.int8)
    o = cls == 0
    j = rng.integers(0, 3, o.sum())
    end[o, 0:3] = SPHERES[j, 0:3] + SPHERES[j, 3:4] * _unit(rng, o.sum())
    end[o, 3:6] = _unit(rng, o.sum())
    flags[o], obj[o] = 0x88, j
    d = cls == 1
    R, ph = rng.uniform(3.2, 8.8, d.sum()), rng.uniform(-np.pi, np.pi, d.sum())
    end[d, 0], end[d, 1] = R * np.cos(ph), R * np.sin(ph)
    end[d, 3:6] = _unit(rng, d.sum())
    flags[d] = 128
    s = cls == 2
    end[s, 0:3] = 40.0 * _unit(rng, s.sum())
    end[s, 3:6] = _unit(rng, s.sum()) * rng.uniform(0.5, 2.0, (s.sum(), 1))
    flags[s] = 8
    h = cls == 3
    end[h, 3:6] = _unit(rng, h.sum())      # (the device colours them black whatever they hold)
    flags[h] = 1
    # camera directions: towards the hole from CAM3, spread like the rays that reach the disk (|Omega b| well below 1: the disk's
    # g = .../(1 - Omega b) stays well conditioned; synthetic rays with a larger impact parameter would make it singular)
    k0 = -CAM3 / 30.0 + 0.08 * rng.normal(size=(n, 3))
    k0 /= np.linalg.norm(k0, axis=1, keepdims=True)
    return end, flags, obj, k0


def _textures(seed):
    rng = np.random.default_rng(seed)
    tex = [rng.random((16, 32, 4)).astype(np.float32), rng.random((9, 20, 4)).astype(np.float32), None]
    rot = [otr.random_rotation(rng), np.zeros((3, 3)), otr.random_rotation(rng)]
    mode = [int(v) for v in rng.integers(0, 2, 3)]
    mode[0], mode[1] = otr.LIT, otr.EMISSIVE            # both modes always present
    emission = [0.0, 2.5, 1.5]
    return otr.Textures(tex=tex, rot=rot, mode=mode, emission=emission)


def _device_ot(T, keep):
    import torch
    f = _ffi()
    dev = []
    for t in T.tex:
        if t is None:
            dev.append(None)
            continue
        d = torch.as_tensor(t).cuda()
        keep.append(d)
        dev.append((d.data_ptr(), t.shape[1], t.shape[0]))
    return f.make_object_textures(dev, [r for r in T.rot[:3]], list(T.mode[:3]), list(T.emission[:3]))[0]


class _Shade:
    """One synthetic frame on the device and the shade entry points on it."""

    def __init__(self, ctx, P, S, seed, rhs, spin):
        import torch
        from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
        f = _ffi()
        self.ctx, self.P, self.S = ctx, P, S
        self.end, self.flags, self.obj, self.k0 = _rays(P * S, seed)
        self.sky = synthetic_sky(128, 64)
        self.disk_tex = synthetic_sky(64, 16, seed=3)
        self.keep = [torch.as_tensor(a).cuda() for a in (self.end, self.flags, self.obj, self.k0, self.sky, self.disk_tex)]
        self.d_end, self.d_fl, self.d_obj, self.d_k0, self.d_sky, self.d_dt = self.keep
        self.scene = f.make_scene(self.d_sky.data_ptr(), 128, 64, d_disk_tex=self.d_dt.data_ptr(), disk_w=64, disk_h=16, disk=DISK,
                                  spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS, **PROFILE)
        self.params = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=rhs, spin=spin, disk_r_in=DISK[0],
                                    disk_r_out=DISK[1])
        # the sky alone: every ray that is not a horizon ray is a sky ray, read as end records or as their directions
        self.keep += [torch.as_tensor(np.where(self.flags == 1, 1, 8).astype(np.uint8)).cuda(),
                      torch.as_tensor(np.ascontiguousarray(self.end[:, 3:6])).cuda()]
        self.d_fl_sky, self.d_dir = self.keep[-2:]
        self.sky_scene = f.make_scene(self.d_sky.data_ptr(), 128, 64)

    def run(self, rs, obs, ot, entry="textured", form="scene"):
        """The fp64, float32 and scattered float32 images of one shade entry point (None: an output it does not write).  form:
        "scene" (disk and spheres), or the sky alone -- "sky" from the end records, "dir" from their directions."""
        import torch
        c, P, S, st = self.ctx, self.P, self.S, torch.cuda.current_stream().cuda_stream
        d_end, d_dir, d_fl, scene = self.d_end.data_ptr(), 0, self.d_fl.data_ptr(), self.scene
        if form != "scene":
            d_fl, scene = self.d_fl_sky.data_ptr(), self.sky_scene
        if form == "dir":
            d_end, d_dir = 0, self.d_dir.data_ptr()
        d_sky, d_k0, d_obj = self.d_sky.data_ptr(), self.d_k0.data_ptr(), self.d_obj.data_ptr()
        calls = {
            "shade": lambda o: c.shade_device(d_end, d_fl, P, S, d_sky, 128, 64, o["d_rgba"], stream=st),
            "shade_dir": lambda o: c.shade_dir_device(d_dir, d_fl, P, S, d_sky, 128, 64, stream=st, **o),
            "shade_scene": lambda o: c.shade_scene_device(d_end, d_fl, P, S, scene, o["d_rgba"], d_object_id=d_obj, stream=st),
            "shade_scene_f32": lambda o: c.shade_scene_f32_device(d_end, d_fl, P, S, scene, o["d_rgba_f32"], d_object_id=d_obj,
                                                                  d_scatter=o.get("d_scatter", 0), stream=st),
            "redshift": lambda o: c.shade_scene_redshift_device(d_end, d_fl, P, S, scene, self.params, rs, CAM3, d_k0, d_object_id=d_obj,
                                                                d_end_dir=d_dir, stream=st, **o),
            "redshift_observer": lambda o: c.shade_scene_redshift_observer_device(d_end, d_fl, P, S, scene, self.params, rs, obs, CAM3,
                                                                                  d_k0, d_object_id=d_obj, d_end_dir=d_dir, stream=st, **o),
            "textured": lambda o: c.shade_scene_textured_device(d_end, d_fl, P, S, scene, self.params, rs, obs, ot, x0_shared=CAM3,
                                                                d_k0=d_k0, d_object_id=d_obj, d_end_dir=d_dir, stream=st, **o),
        }
        writes = {"shade": (0,), "shade_scene": (0,), "shade_scene_f32": (1, 2)}.get(entry, (0, 1, 2))
        d64 = torch.full((P, 4), float("nan"), dtype=torch.float64, device="cuda")
        d32 = torch.full((P, 4), float("nan"), dtype=torch.float32, device="cuda")
        sc = torch.full((P, 4), float("nan"), dtype=torch.float32, device="cuda")
        perm = torch.randperm(P, device="cuda")
        outs = (dict(d_rgba=d64.data_ptr()), dict(d_rgba_f32=d32.data_ptr()), dict(d_rgba_f32=sc.data_ptr(), d_scatter=perm.data_ptr()))
        for j in writes:
            calls[entry](outs[j])
        torch.cuda.synchronize()
        return tuple(img if j in writes else None for j, img in enumerate((d64.cpu().numpy(), d32.cpu().numpy(), sc[perm].cpu().numpy())))


METRICS = [("christoffel", 0, 0.0), ("reduced", 1, 0.0), ("kerr", 2, 0.45)]
REDSHIFT = ["off", "on", "observer"]


@pytest.mark.parametrize("rsmode", REDSHIFT)
@pytest.mark.parametrize("metric", METRICS, ids=[m[0] for m in METRICS])
def test_textured_shade_against_restatement(ctx, metric, rsmode):
    f = _ffi()
    _, rhs, spin = metric
    kerr = rhs == 2
    sense = -1 if kerr else 1
    for P, S, seed in ((1500, 1, 1), (300, 5, 2), (6, 300, 3)):      # (samples > 256: the serial kernel)
        sh = _Shade(ctx, P, S, seed, rhs, spin)
        T = _textures(seed + 10)
        keep = []
        ot = _device_ot(T, keep)
        rs = None if rsmode == "off" else f.make_redshift(("disk", "objects", "sky"), 4.0, sense)
        obs = f.make_observer(BETA) if rsmode == "observer" else None
        got, g32, gsc = sh.run(rs, obs, ot)
        g = None
        if rsmode == "on":
            g = rr.g_rays(CAM3, sh.k0, sh.end, sh.flags, 1.0, spin, kerr, sense)
        elif rsmode == "observer":
            g = orf.observer_g_rays(CAM3, sh.k0, sh.end, sh.flags, 1.0, BETA, spin, kerr, sense)
        want = otr.shade_scene_textured(sh.end, sh.flags, sh.obj, P, S, sh.sky, T, g=g, exponent=4.0, apply=7 if g is not None else 0,
                                        disk=DISK, disk_tex=sh.disk_tex,
                                        disk_profile=dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0),
                                        spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS)
        # (1e-11 of the colour's scale: g^4 carries the restated g's 1e-12 relative agreement four times)
        err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()
        assert err < 1e-11, (P, S, err)
        assert np.array_equal(g32, got.astype(np.float32)) and np.array_equal(gsc, g32)
        # ... and the textures did something
        plain = sh.run(rs, obs, None)[0]
        assert np.abs(plain - got).max() > 1e-3


@pytest.mark.parametrize("rsmode", REDSHIFT)
def test_null_and_zero_tables_are_the_untextured_call(ctx, rsmode):
    f = _ffi()
    for rhs, spin in ((0, 0.0), (2, 0.45)):
        for P, S in ((700, 1), (5, 300)):
            sh = _Shade(ctx, P, S, 7, rhs, spin)
            rs = None if rsmode == "off" else f.make_redshift(("disk", "objects", "sky"), 4.0, 1)
            obs = f.make_observer(BETA) if rsmode == "observer" else None
            today = sh.run(rs, obs, None, entry="redshift_observer")
            for ot in (None, f.ObjectTextures()):
                got = sh.run(rs, obs, ot)
                for a, b in zip(got, today):
                    assert np.array_equal(a, b)



# (entry point, frame form, redshift): each entry point on the frames it is meant for
ENTRIES = [("shade", "sky", "off"), ("shade_dir", "dir", "off"), ("shade_scene", "scene", "off"), ("shade_scene_f32", "scene", "off"),
           ("redshift", "scene", "on"), ("redshift", "dir", "on"), ("redshift_observer", "scene", "observer"),
           ("redshift_observer", "dir", "observer")]


@pytest.mark.parametrize("entry,form,rsmode", ENTRIES)
def test_every_entry_point_is_the_general_call(ctx, entry, form, rsmode):
    """Each bhg_shade*_device writes the bytes of bhg_shade_scene_textured_device (ot = NULL) given the same inputs, with the
    arguments it does not take NULL: fp64, float32 and scattered float32, end records and directions, redshift with and without
    an observer."""
    f = _ffi()
    for P, S in ((700, 3), (5, 300)):
        sh = _Shade(ctx, P, S, 9, 0, 0.0)
        rs = None if rsmode == "off" else f.make_redshift(("disk", "objects", "sky"), 4.0, 1)
        obs = f.make_observer(BETA) if rsmode == "observer" else None
        got = sh.run(rs, obs, None, entry=entry, form=form)
        want = sh.run(rs, obs, None, form=form)
        assert all(np.isfinite(w).all() for w in want)
        for g, w in zip(got, want):
            assert g is None or np.array_equal(g, w), (entry, form, P, S)


def test_every_entry_point_accepts_an_empty_call(ctx):
    """n_pixels = 0 with a real context and every device array NULL is BHG_OK at all seven entry points: the empty shard of a
    rank dealt no tiles (tests/test_gpu_multirank.py), here with a disk, spheres, redshift and the observer."""
    import ctypes as C
    f = _ffi()
    L = f.load()
    sc = C.byref(f.make_scene(0, 128, 64, disk=DISK, spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS, **PROFILE))
    p = C.byref(f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1]))
    rs, obs, ot = C.byref(f.make_redshift()), C.byref(f.make_observer(BETA)), C.byref(f.ObjectTextures())
    x0 = (C.c_double * 3)(*CAM3)
    h = ctx._h
    calls = {
        "bhg_shade_device": lambda: L.bhg_shade_device(h, None, None, 0, 1, None, 128, 64, None, None),
        "bhg_shade_dir_device": lambda: L.bhg_shade_dir_device(h, None, None, 0, 1, None, 128, 64, None, None, None, None),
        "bhg_shade_scene_device": lambda: L.bhg_shade_scene_device(h, None, None, None, 0, 1, sc, None, None),
        "bhg_shade_scene_f32_device": lambda: L.bhg_shade_scene_f32_device(h, None, None, None, 0, 1, sc, None, None, None),
        "bhg_shade_scene_redshift_device": lambda: L.bhg_shade_scene_redshift_device(h, None, None, None, None, 0, 1, sc, p, rs, x0,
                                                                                     None, None, None, None, None),
        "bhg_shade_scene_redshift_observer_device": lambda: L.bhg_shade_scene_redshift_observer_device(
            h, None, None, None, None, 0, 1, sc, p, rs, obs, x0, None, None, None, None, None),
        "bhg_shade_scene_textured_device": lambda: L.bhg_shade_scene_textured_device(h, None, None, None, None, 0, 1, sc, p, rs, obs, ot,
                                                                                     x0, None, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == f.OK, (name, L.bhg_last_error().decode())

def _uv_texture(TW, TH):
    """A texture whose texel centres hold their own (U, V): bilinear reads return (U, V) away from the seam and the poles."""
    u = (np.arange(TW) + 0.5) / TW * 2.0 - 1.0
    v = (np.arange(TH) + 0.5) / TH * 2.0 - 1.0
    tex = np.zeros((TH, TW, 4), np.float32)
    tex[..., 0] = u[None, :]
    tex[..., 1] = v[:, None]
    tex[..., 3] = 1.0
    return tex


def test_traced_sphere_decodes_its_own_uv(ctx):
    """A sphere well off the hole, emissive, white, with a texture that encodes (U, V): every object pixel at samples = 1 decodes
    to the (U, V) of its own end record's body normal within one texel; turning the sphere by psi about its body z moves every
    decoded U by -psi / pi (the texture turns with the sphere)."""
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    TW, TH = 256, 128
    tex = _uv_texture(TW, TH)
    sphere = [2.0, 1.0, 14.0, 3.0]
    fr = DeviceFrame(ctx, 128, 128, 1, fov_x=0.6, fov_y=0.6, origin=CAM)
    fr.set_sky(synthetic_sky(64, 32))
    fr.set_objects([sphere], [[1.0, 1.0, 1.0]], [[20.0, 0.0, 30.0, 10.0]])
    p = f.make_params(r_s=1.0, lambda_end=60.0, r_exit=40.0)
    fr.generate_rays()
    fr.trace(p)
    tilt = otr.random_rotation(np.random.default_rng(12))
    decoded = {}
    for psi in (0.0, 0.9):
        R = tilt @ otr.rot_z(psi)
        fr.set_object_textures([tex], [R], ["emissive"], [1.0])
        rgba = fr.shade().cpu().numpy()
        torch.cuda.synchronize()
        fl, end = fr.d_flags.cpu().numpy(), fr.d_end.cpu().numpy()
        o = fl == 0x88
        assert o.sum() > 500
        n = (end[o, 0:3] - np.array(sphere[:3])) / sphere[3]
        U, V = otr.body_uv(otr.body_normal(n, R))
        ok = (np.abs(U) < 1.0 - 4.0 / TW) & (np.abs(V) < 1.0 - 4.0 / TH)
        assert ok.sum() > 0.7 * o.sum()
        assert np.abs(rgba[o, 0][ok] - U[ok]).max() < 2.0 / TW
        assert np.abs(rgba[o, 1][ok] - V[ok]).max() < 2.0 / TH
        decoded[psi] = (rgba[o, 0], rgba[o, 1], ok)
    U0, V0, ok0 = decoded[0.0]
    U1, V1, ok1 = decoded[0.9]
    both = ok0 & ok1
    assert both.sum() > 0.5 * len(U0)
    dU = np.mod(U1 - U0 + 1.0, 2.0) - 1.0
    assert np.abs(dU[both] + 0.9 / np.pi).max() < 2.0 * 2.0 / TW
    assert np.abs(V1[both] - V0[both]).max() < 2.0 / TH


def _frame(devices, W, H, S, **kw):
    f = _ffi()
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    return f.Frame(devices, W, H, S, fov_x=0.9, fov_y=0.9, origin=CAM3, rot=euler_xyz_matrix((0.0, INC, 0.0)),
                   jitter=python_random_stream(42.0, 2 * S * W * H), **kw)


def test_frame_object_textures(ctx):
    """bhg_frame_set_object_textures: one device and the {0, 0} loopback (copy and peer-call gathers) give DeviceFrame's image;
    a rotation-only update (no textures passed) gives a fresh frame's image with the new rotation; NULL gives the untextured
    image bit for bit; with redshift on, the same against DeviceFrame."""
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    W, H, S = 96, 64, 2
    sky = synthetic_sky(256, 128)
    T = _textures(21)
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    rng = np.random.default_rng(22)
    R2 = [otr.random_rotation(rng) for _ in range(3)]
    modes, emission = list(T.mode[:3]), list(T.emission[:3])
    images = {}
    for name, devs, gather in (("one", [0], f.GATHER_AUTO), ("loop", [0, 0], f.GATHER_COPY),
                               ("peercall", [0, 0], f.GATHER_COPY_PEERCALL)):
        fr = _frame(devs, W, H, S, gather=gather, tile=16)
        fr.set_scene(sky, spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS)
        plain = fr.render(p)
        fr.set_object_textures(T.tex[:3], list(T.rot[:3]), modes, emission)
        images[name] = fr.render(p)
        assert np.abs(images[name] - plain).max() > 1e-3
        fr.set_object_textures([None, None, None], R2, modes, emission)      # rotations only: nothing uploaded
        images[name + "_rot"] = fr.render(p)
        fr.set_redshift(("objects", "sky"), 4.0, 1)
        images[name + "_rs"] = fr.render(p)
        fr.set_redshift(None)
        fr.set_object_textures(None)
        assert np.array_equal(fr.render(p), plain)
        fr.close()
    for k in ("", "_rot", "_rs"):
        assert np.array_equal(images["one" + k], images["loop" + k]) and np.array_equal(images["one" + k], images["peercall" + k])
    fresh = _frame([0], W, H, S)
    fresh.set_scene(sky, spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS)
    fresh.set_object_textures(T.tex[:3], R2, modes, emission)
    assert np.array_equal(fresh.render(p), images["one_rot"])
    assert np.abs(images["one_rot"] - images["one"]).max() > 1e-3
    fresh.close()
    # the Python adaptor on the same frame
    dfr = DeviceFrame(ctx, W, H, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM3, rotation_euler=(0.0, INC, 0.0))
    dfr.set_sky(sky)
    dfr.set_objects(SPHERES, RGB, LAMPS)
    dfr.set_object_textures(T.tex[:3], list(T.rot[:3]), modes, emission)
    dfr.generate_rays()
    dfr.trace(p)
    out = torch.empty((W * H, 4), dtype=torch.float32, device=dfr.dev)
    for key, rs, rot in (("one", None, list(T.rot[:3])), ("one_rs", ("objects", "sky"), R2)):
        dfr.set_object_textures(rotations=rot, modes=modes, emission=emission)   # (textures kept)
        dfr.set_redshift(rs, 4.0, 1) if rs else dfr.set_redshift(None)
        dfr.shade_f32(out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(H, W, 4), images[key]), key
    # fp64 against the restatement
    dfr.set_redshift(None)
    dfr.set_object_textures(rotations=list(T.rot[:3]), modes=modes, emission=emission)
    rgba = dfr.shade().cpu().numpy()
    end, flags, obj = dfr.d_end.cpu().numpy(), dfr.d_flags.cpu().numpy(), dfr.d_obj.cpu().numpy()
    want = otr.shade_scene_textured(end, flags, obj, dfr.P, S, sky, T, spheres=SPHERES, sphere_rgb=RGB, lamps=LAMPS)
    assert (flags == 0x88).sum() > 200
    assert np.abs(rgba - want).max() < 1e-11


def test_frame_refusals(ctx):
    f = _ffi()
    fr = _frame([0], 32, 32, 1)
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    fr.set_scene(synthetic_sky(64, 32), spheres=SPHERES[:2], lamps=LAMPS)
    with pytest.raises(f.BhgError, match="sphere 1"):
        fr.set_object_textures(modes=["lit", 3])
    with pytest.raises(f.BhgError, match="sphere 0"):
        fr.set_object_textures(rotations=[2.0 * np.eye(3)])
    with pytest.raises(f.BhgError, match="sphere 1"):
        fr.set_object_textures(emission=[0.0, -1.0])
    fr.set_object_textures(modes=["lit", "lit", 7])          # slot 2 is beyond the scene's spheres: ignored
    img = fr.render(f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0))
    assert np.isfinite(img).all()
    fr.close()

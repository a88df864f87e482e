"""Redshift (ABI 9) on the GPU: bhg_redshift_device against the numpy restatement (tests/redshift_reference.py) on the
device's own end records, the closed forms, the redshift-weighted shade against oracle.shade_reference with g^n, apply = 0
bit for bit today's calls, the library-owned frame on one device and on the {0, 0} loopback, the Python adaptors, and the
Doppler asymmetry of an edge-on disk."""
import os
import sys

import numpy as np
import pytest

from conftest import CAM, frame_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import redshift_reference as rr  # noqa: E402

INC = np.radians(75.0)
CAM3 = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])     # config-3-style inclined camera


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _inclined_rays(n, seed=0, fov=0.7, inc=INC):
    k = frame_rays(n, seed, fov)
    c, s = np.cos(inc), np.sin(inc)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])      # rotate the -z look direction to look at the hole
    return k @ R.T


def _device_g(ctx, p, rs, k0, end, flags, x0):
    import torch
    f = _ffi()
    d_k0 = torch.as_tensor(k0).cuda()
    d_end = torch.as_tensor(end).cuda()
    d_fl = torch.as_tensor(flags).cuda()
    d_g = torch.empty(len(k0), dtype=torch.float64, device="cuda")
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0)).cuda()
    ctx.redshift_device(p, rs, len(k0), d_k0.data_ptr(), d_fl.data_ptr(), d_g.data_ptr(),
                        x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(), d_end=d_end.data_ptr(),
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = d_g.cpu().numpy()
    assert np.array_equal(g, ctx.redshift(k0, x0, p, rs, flags, end), equal_nan=True)   # host form: the same launch
    del f
    return g


def _check_g(g, want, flags):
    dark = (flags & 3) != 0
    nan = ((flags & 64) != 0) & ~dark
    assert np.all(g[dark] == 0.0)
    assert np.all(np.isnan(g[nan]))
    ok = ~dark & ~nan
    rel = np.abs(g[ok] / want[ok] - 1.0)
    assert rel.max() <= 1e-12, rel.max()


CASES = [
    # name, rhs, spin, disk, spheres, sense, camera
    ("schw_disk", 0, 0.0, (3.0, 9.0), None, 1, CAM3),
    ("schw_disk_reduced", 1, 0.0, (3.0, 9.0), None, -1, CAM3),
    ("kerr_disk_pro", 2, 0.45, (3.0, 9.0), None, 1, CAM3),
    ("kerr_disk_retro", 2, 0.45, (3.0, 9.0), None, -1, CAM3),
    ("schw_objects", 0, 0.0, None, [[6.0, 3.0, 2.5, 1.5], [7.0, -4.0, 3.0, 1.0], [2.0, 6.0, -1.0, 1.2]], 1, CAM3),
    ("kerr_objects", 2, 0.45, None, [[6.0, 3.0, 2.5, 1.5], [7.0, -4.0, 3.0, 1.0], [2.0, 6.0, -1.0, 1.2]], 1, CAM3),
    ("schw_sky", 0, 0.0, None, None, 1, CAM),
    ("kerr_sky", 2, 0.45, None, None, 1, CAM),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_redshift_device_against_restatement(ctx, case):
    f = _ffi()
    name, rhs, spin, disk, spheres, sense, cam = case
    k0 = _inclined_rays(3000, seed=7) if cam is CAM3 else frame_rays(3000, seed=7)
    kw = dict(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=rhs, spin=spin)
    if disk:
        kw.update(disk_r_in=disk[0], disk_r_out=disk[1])
    p = f.make_params(**kw)
    res = ctx.trace(k0, cam, p, spheres=spheres)
    end, flags = res[0], res[1]
    classes = {int(v): int((flags == v).sum()) for v in np.unique(flags)}
    if disk:
        assert classes.get(128, 0) > 200, classes
    if spheres:
        assert classes.get(0x88, 0) > 50, classes
    rs = f.make_redshift(disk_sense=sense)
    g = _device_g(ctx, p, rs, k0, end, flags, cam)
    want = rr.g_rays(cam, k0, end, flags, 1.0, spin, rhs == 2, sense)
    _check_g(g, want, flags)
    if name.endswith("sky"):
        # per-ray origins: every ray its own camera
        x0 = np.tile(cam, (len(k0), 1)) * np.linspace(0.7, 1.3, len(k0))[:, None]
        res = ctx.trace(k0, x0, p)
        g = _device_g(ctx, p, rs, k0, res[0], res[1], x0)
        _check_g(g, rr.g_rays(x0, k0, res[0], res[1], 1.0, spin, rhs == 2, sense), res[1])


def test_face_on_closed_forms(ctx):
    f = _ffi()
    cam = np.array([0.0, 0.0, 30.0])
    k0 = frame_rays(4000, seed=3, fov=0.5)
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)
    sph = [[2.0, 2.0, 8.0, 1.5]]
    end, flags, _, _, obj = ctx.trace(k0, cam, p, spheres=sph)
    assert (flags == 128).sum() > 300 and (flags == 0x88).sum() > 20
    M, fc = 0.5, 1.0 - 1.0 / 30.0
    for sense in (1, -1):
        g = ctx.redshift(k0, cam, p, f.make_redshift(disk_sense=sense), flags, end)
        d = flags == 128
        R = np.hypot(end[d, 0], end[d, 1])
        assert np.abs(g[d] / (np.sqrt(1 - 3 * M / R) / np.sqrt(fc)) - 1).max() <= 1e-12
        o = flags == 0x88
        rh = np.linalg.norm(end[o, 0:3], axis=1)
        assert np.abs(g[o] / np.sqrt((1 - 1.0 / rh) / fc) - 1).max() <= 1e-12
        s = (flags == 8) | (flags == 4)
        assert np.abs(g[s] * np.sqrt(fc) - 1).max() <= 1e-12


def test_kerr_axis_camera(ctx):
    """The reference's Kerr camera, 1e-4 off the axis: g_disk -> 1 / (alpha_c u^t) as L -> 0.  The offset from the axis
    leaves b = L / E != 0; the bound is the one it implies, |omega_c b| + |Omega b| (and the axis alpha against the camera's)."""
    f = _ffi()
    cam = np.array([1e-4, 0.0, 30.0])
    M, a = 0.5, 0.45
    k0 = frame_rays(3000, seed=11, fov=0.5)
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=f.RHS_KERR_BL, spin=a, disk_r_in=3.0, disk_r_out=9.0)
    end, flags, _, _ = ctx.trace(k0, cam, p)
    d = flags == 128
    assert d.sum() > 200
    for sense in (1, -1):
        g = ctx.redshift(k0, cam, p, f.make_redshift(disk_sense=sense), flags, end)[d]
        s = -sense                                     # the traced picture's sense (redshift_reference docstring)
        r = np.sqrt(end[d, 0] ** 2 + end[d, 1] ** 2 - a * a)
        ut = (r ** 1.5 + s * a * np.sqrt(M)) / (r ** 0.75 * np.sqrt(r ** 1.5 - 3 * M * np.sqrt(r) + 2 * s * a * np.sqrt(M)))
        Om = s * np.sqrt(M) / (r ** 1.5 + s * a * np.sqrt(M))
        Del = 30.0 ** 2 - 2 * M * 30.0 + a * a
        alpha_axis = np.sqrt(Del / (30.0 ** 2 + a * a))
        b = np.array([rr.kerr_E_L(cam, k, M, a)[1] / rr.kerr_E_L(cam, k, M, a)[0] for k in k0[d]])
        _, om_c = rr.kerr_zamo(30.0, 0.0, M, a)
        bound = np.abs(om_c * b) + np.abs(Om * b) + 1e-9
        rel = np.abs(g * alpha_axis * ut - 1.0)
        assert np.all(rel <= 1.5 * bound), (rel.max(), bound.max())
        print(f"Kerr axis camera, sense {sense}: max |g alpha u^t - 1| = {rel.max():.3e} (bound {bound.max():.3e})")


def _scene_frame(ctx, kerr=False, objects=True):
    """An inclined frame with horizon, sky, disk and object pixels, traced by DeviceFrame."""
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    W, H, S = 96, 64, 3
    sky = synthetic_sky(512, 256)
    disk_tex = synthetic_sky(256, 64, seed=3)
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM3, rotation_euler=(0.0, INC, 0.0))
    fr.set_sky(sky)
    prof = dict(disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
    fr.set_disk(3.0, 9.0, disk_tex, **prof)
    sph = [[6.0, 3.0, 2.5, 1.5], [7.0, -4.0, 3.0, 1.0], [2.0, 6.0, -1.0, 1.2]]
    rgb = [[1.0, 0.8, 0.6], [0.2, 0.9, 0.3], [0.5, 0.5, 1.0]]
    lamps = [[20.0, 0.0, 20.0, 10.0], [10.0, -15.0, 5.0, 6.0]]
    if objects:
        fr.set_objects(sph, rgb, lamps)
    kw = dict(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)
    if kerr:
        kw.update(rhs_form=2, spin=0.45)
    p = _ffi().make_params(**kw)
    fr.generate_rays()
    fr.trace(p)
    torch.cuda.synchronize()
    ref = dict(disk=(3.0, 9.0), disk_tex=disk_tex, disk_profile=dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0),
               spheres=sph if objects else None, sphere_rgb=np.array(rgb) if objects else None, lamps=lamps if objects else None)
    return fr, p, sky, ref


@pytest.mark.parametrize("kerr", [False, True])
@pytest.mark.parametrize("apply,exponent", [(("disk", "objects", "sky"), 4.0), (("disk",), 3.0), (("objects", "sky"), 4.0)])
def test_redshift_shade_against_reference(ctx, kerr, apply, exponent):
    import torch
    f = _ffi()
    fr, p, sky, ref = _scene_frame(ctx, kerr)
    fr.set_redshift(apply, exponent, disk_sense=-1 if kerr else 1)
    rgba = fr.shade().clone()
    out = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out)
    perm = torch.randperm(fr.P, device=fr.dev)
    sc = torch.zeros((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(sc, perm)
    torch.cuda.synchronize()
    rgba = rgba.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), rgba.astype(np.float32))
    assert torch.equal(sc[perm], out)
    end, flags, obj, k0 = fr.d_end.cpu().numpy(), fr.d_flags.cpu().numpy(), fr.d_obj.cpu().numpy(), fr.d_k0.cpu().numpy()
    g = rr.g_rays(fr.origin, k0, end, flags, 1.0, 0.45 if kerr else 0.0, kerr, -1 if kerr else 1)
    bits = sum({"disk": 1, "objects": 2, "sky": 4}[a] for a in apply)
    want = rr.shade_scene_redshift(end, flags, obj, fr.P, fr.S, sky, g, exponent, bits, **ref)
    assert np.abs(rgba - want).max() < 1e-11
    # ... and the weighting did something
    fr.set_redshift(None)
    plain = fr.shade().cpu().numpy()
    assert np.abs(plain - rgba).max() > 1e-3
    del f


def test_apply_zero_is_todays_call(ctx):
    import torch
    f = _ffi()
    fr, p, sky, _ = _scene_frame(ctx)
    today = fr.shade().clone()
    t32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(t32)
    off = f.make_redshift(apply=0)
    for rs in (off, None):
        d64 = torch.empty_like(today)
        d32 = torch.empty_like(t32)
        ctx.shade_scene_redshift_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, rs, fr.origin,
                                        fr.d_k0.data_ptr(), d_rgba=d64.data_ptr(), d_rgba_f32=d32.data_ptr(),
                                        d_object_id=fr.d_obj.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(d64, today) and torch.equal(d32, t32)


def _frame(devices, W, H, S, cam, euler, **kw):
    f = _ffi()
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    return f.Frame(devices, W, H, S, fov_x=0.9, fov_y=0.9, origin=cam, rot=euler_xyz_matrix(euler),
                   jitter=python_random_stream(42.0, 2 * S * W * H), **kw)


@pytest.mark.parametrize("scene", ["disk", "sky"])
def test_frame_redshift(ctx, scene):
    """bhg_frame_set_redshift: one device and the {0, 0} loopback (COPY and COPY_PEERCALL gathers) bit for bit; NULL /
    apply = 0 gives today's frame bit for bit; the same image as DeviceFrame.set_redshift on the same frame."""
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    W, H, S = 96, 64, 2
    sky = synthetic_sky(512, 256)
    kw = dict(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    if scene == "disk":
        kw.update(disk_r_in=3.0, disk_r_out=9.0)
    p = f.make_params(**kw)
    images = {}
    for name, devs, gather in (("one", [0], f.GATHER_AUTO), ("loop", [0, 0], f.GATHER_COPY),
                               ("peercall", [0, 0], f.GATHER_COPY_PEERCALL)):
        fr = _frame(devs, W, H, S, CAM3, (0.0, INC, 0.0), gather=gather, tile=16)
        fr.set_scene(sky, disk=(3.0, 9.0) if scene == "disk" else None)
        plain = fr.render(p)
        fr.set_redshift(("disk", "sky"), 4.0, 1)
        images[name] = fr.render(p)
        assert fr.info()["directions_only"] == (scene == "sky")
        fr.set_redshift(None)
        assert np.array_equal(fr.render(p), plain)
        fr.set_redshift(0)
        assert np.array_equal(fr.render(p), plain)
        assert np.abs(images[name] - plain).max() > 1e-3
        fr.close()
    assert np.array_equal(images["one"], images["loop"]) and np.array_equal(images["one"], images["peercall"])
    # the Python adaptor on the same frame
    dfr = DeviceFrame(ctx, W, H, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM3, rotation_euler=(0.0, INC, 0.0),
                      directions_only=scene == "sky")
    dfr.set_sky(sky)
    if scene == "disk":
        dfr.set_disk(3.0, 9.0)
    dfr.set_redshift(("disk", "sky"), 4.0, 1)
    dfr.generate_rays()
    dfr.trace(p)
    out = torch.empty((W * H, 4), dtype=torch.float32, device=dfr.dev)
    dfr.shade_f32(out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(H, W, 4), images["one"])


def test_integrator_trace_redshift(ctx):
    f = _ffi()
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorKerr, GeodesicIntegratorSchwarzschild
    k0 = _inclined_rays(2000, seed=5)
    for gi, rhs, spin in ((GeodesicIntegratorSchwarzschild(mass=0.5, context=ctx), 0, 0.0),
                          (GeodesicIntegratorKerr(mass=0.5, a=0.9, context=ctx), 2, 0.45)):
        for sense in (1, -1):
            out = gi.trace(k0, CAM3, curve_end=80.0, r_exit=40.0, disk=(3.0, 9.0), redshift=dict(disk_sense=sense))
            p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0, rhs_form=rhs, spin=spin)
            g = ctx.redshift(k0, CAM3, p, f.make_redshift(disk_sense=sense), out["flags"], out["ray_end"])
            assert np.array_equal(out["g"], g, equal_nan=True)
            assert (out["flags"] == 128).sum() > 100


def test_edge_on_doppler_asymmetry(ctx):
    """Seen edge-on, the half of a disk that moves towards the camera is blueshifted: sense +1 (counter-clockwise seen from +z)
    with the camera on +x moves the y < 0 side towards it."""
    f = _ffi()
    cam = np.array([30.0, 0.0, 0.6])
    k = frame_rays(15000, seed=9, fov=0.8)
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], float)       # -z -> -x: look along -x, at the hole
    k0 = k @ R.T
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0)
    end, flags, _, _ = ctx.trace(k0, cam, p)
    d = flags == 128
    assert d.sum() > 300
    # the visible (near) face of the disk: hits on the camera's side of the hole
    near = d & (end[:, 0] > 0.0)
    for sense in (1, -1):
        g = ctx.redshift(k0, cam, p, f.make_redshift(disk_sense=sense), flags, end)
        approaching = near & (end[:, 1] * sense < 0.0)
        receding = near & (end[:, 1] * sense > 0.0)
        assert approaching.sum() > 50 and receding.sum() > 50
        assert g[approaching].mean() > 1.0 > g[receding].mean(), (sense, g[approaching].mean(), g[receding].mean())

"""Disk polarisation on the GPU: bhg_polarisation_device / _host against the numpy restatement
(tests/polarisation_reference.py) on the library's own traces and on synthetic mixes of ray classes, the polarised shade (its
colour bit for bit the textured call's, its Q / U against the restatement's shade), an end-to-end flat-limit frame, and the
Python adaptors."""
import os
import sys

import numpy as np
import pytest

from conftest import frame_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import observer_reference as orf  # noqa: E402
import polarisation_reference as pr  # noqa: E402
import redshift_reference as rr  # noqa: E402

INC = np.radians(60.0)
CAM = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])
TABLE = (0.0, 0.35, 0.2, 0.117)
BETA = (0.3, -0.2, 0.1)


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _inclined_rays(n, seed=0, fov=0.7, inc=INC):
    k = frame_rays(n, seed, fov)
    c, s = np.cos(inc), np.sin(inc)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return k @ R.T


def _device_pol(ctx, p, pol, obs, k0, end, flags, x0):
    """bhg_polarisation_device, checked against the host form (the same launch) and returned."""
    import torch
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0)).cuda()
    d_end = None if end is None else torch.as_tensor(np.ascontiguousarray(end)).cuda()
    d_fl = torch.as_tensor(np.ascontiguousarray(flags)).cuda()
    out = torch.empty((3, len(k0)), dtype=torch.float64, device="cuda")
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0)).cuda()
    ctx.polarisation_device(p, pol, obs, len(k0), d_k0.data_ptr(), d_fl.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                            out[2].data_ptr(), x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(),
                            d_end=0 if d_end is None else d_end.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    chi, deg, mu = out.cpu().numpy()
    h = ctx.polarisation(k0, x0, p, pol, obs, flags, end)
    for a, b in zip((chi, deg, mu), h):
        assert np.array_equal(a, b, equal_nan=True)
    return chi, deg, mu


def _check(got, want, flags):
    chi, deg, mu = got
    wc, wd, wm = want
    zero = (wd == 0.0) & (wm == 0.0) & (wc == 0.0)
    nan = np.isnan(wd)
    for a in got:
        assert np.all(a[zero] == 0.0)
        assert np.all(np.isnan(a[nan]))
    d = ~zero & ~nan
    assert d.sum() > 0
    assert np.array_equal(np.isnan(chi[d]), np.isnan(wc[d]))
    ok = d & ~np.isnan(wc)
    assert pr.chi_diff(chi[ok], wc[ok]).max() <= 1e-10
    assert np.abs(deg[d] - wd[d]).max() <= 1e-12
    assert np.abs(mu[d] - wm[d]).max() <= 1e-12


def _mix(flags, end, seed):
    """A synthetic mix of classes on top of a trace: some disk rays relabelled horizon, start-inside, object, sky, NaN."""
    rng = np.random.default_rng(seed)
    fl = flags.copy()
    idx = rng.permutation(len(fl))[: len(fl) // 3]
    fl[idx] = rng.choice(np.array([1, 3, 0x88, 8, 4, 16, 64, 65], np.uint8), len(idx))
    return fl


CASES = [
    # name, rhs, spin, sense, beta
    ("schw", 0, 0.0, 1, None),
    ("schw_reduced", 1, 0.0, -1, None),
    ("kerr", 2, 0.45, 1, None),
    ("schw_obs", 0, 0.0, -1, BETA),
    ("kerr_obs", 2, 0.45, -1, BETA),
    ("kerr_half", 2, 0.225, 1, BETA),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_per_ray_against_restatement(ctx, case):
    f = _ffi()
    name, rhs, spin, sense, beta = case
    k0 = _inclined_rays(2500, seed=5)
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=rhs, spin=spin, disk_r_in=3.0, disk_r_out=9.0)
    end, flags = ctx.trace(k0, CAM, p)[:2]
    assert (flags == 128).sum() > 300
    pol = f.make_polarisation(TABLE, sense, (0.1, 1.0, 0.2))
    obs = f.make_observer(beta)
    for fl in (flags, _mix(flags, end, 3)):
        got = _device_pol(ctx, p, pol, obs, k0, end, fl, CAM)
        want = pr.pol_rays(CAM, k0, end, fl, 1.0, spin, rhs == 2, sense, TABLE, (0.1, 1.0, 0.2), beta)
        _check(got, want, fl)
    # no end records: disk rays NaN
    chi, deg, mu = _device_pol(ctx, p, pol, obs, k0, None, flags, CAM)
    assert np.all(np.isnan(chi[flags == 128])) and np.all(np.isnan(deg[flags == 128]))
    if name in ("schw", "kerr"):
        # per-ray origins: every ray its own camera
        x0 = np.tile(CAM, (len(k0), 1)) * np.linspace(0.8, 1.2, len(k0))[:, None]
        end, flags = ctx.trace(k0, x0, p)[:2]
        got = _device_pol(ctx, p, pol, obs, k0, end, flags, x0)
        _check(got, pr.pol_rays(x0, k0, end, flags, 1.0, spin, rhs == 2, sense, TABLE, (0.1, 1.0, 0.2), beta), flags)


@pytest.mark.parametrize("rhs,spin,beta", [(0, 0.0, None), (2, 0.45, None), (0, 0.0, BETA), (2, 0.45, BETA)])
def test_degenerate_screen(ctx, rhs, spin, beta):
    """up along one disk ray's look direction (in the observer's rest frame): that ray's chi is NaN, its degree and emission
    cosine are still the restatement's; every other ray is unaffected."""
    f = _ffi()
    k0 = _inclined_rays(400, seed=17)
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=rhs, spin=spin, disk_r_in=3.0, disk_r_out=9.0)
    end, flags = ctx.trace(k0, CAM, p)[:2]
    j = int(np.flatnonzero(flags == 128)[0])
    n = orf.n_of_k0(CAM, k0[j], 1.0, spin, rhs == 2)
    if beta is not None:
        n = orf.aberrate(n, -np.asarray(beta))
    up = n / np.linalg.norm(n)
    pol = f.make_polarisation(TABLE, 1, up)
    got = _device_pol(ctx, p, pol, f.make_observer(beta), k0, end, flags, CAM)
    want = pr.pol_rays(CAM, k0, end, flags, 1.0, spin, rhs == 2, 1, TABLE, up, beta)
    assert np.isnan(got[0][j]) and np.isnan(want[0][j])
    assert np.isfinite(got[1][j]) and np.isfinite(got[2][j]) and 0.0 <= got[2][j] <= 1.0
    _check(got, want, flags)


def test_kerr_at_zero_spin_is_schwarzschild(ctx):
    f = _ffi()
    k0 = _inclined_rays(2000, seed=9)
    ps = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)
    pk = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, rhs_form=2, spin=0.0, disk_r_in=3.0, disk_r_out=9.0)
    end, flags = ctx.trace(k0, CAM, ps)[:2]
    pol = f.make_polarisation(TABLE)
    for obs in (None, f.make_observer(BETA)):
        a = ctx.polarisation(k0, CAM, ps, pol, obs, flags, end)
        b = ctx.polarisation(k0, CAM, pk, pol, obs, flags, end)
        d = flags == 128
        assert pr.chi_diff(a[0][d], b[0][d]).max() < 1e-12
        assert np.abs(a[2][d] - b[2][d]).max() < 1e-12


# ---- the polarised shade ---------------------------------------------------------------------------------------------
def _scene_frame(ctx, S, kerr=False, euler=(0.0, INC, 0.0)):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    W, H = (8, 6) if S > 256 else (40, 30)
    sky = synthetic_sky(256, 128)
    disk_tex = synthetic_sky(128, 32, seed=3)
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM, rotation_euler=euler)
    fr.set_sky(sky)
    fr.set_disk(3.0, 9.0, disk_tex, disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
    sph = [[6.0, 3.0, 2.5, 1.5], [2.0, 6.0, -1.0, 1.2]]
    rgb = [[1.0, 0.8, 0.6], [0.5, 0.5, 1.0]]
    lamps = [[20.0, 0.0, 20.0, 10.0]]
    fr.set_objects(sph, rgb, lamps)
    kw = dict(r_s=1.0, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)
    if kerr:
        kw.update(rhs_form=2, spin=0.45)
    p = _ffi().make_params(**kw)
    fr.generate_rays()
    fr.trace(p)
    torch.cuda.synchronize()
    ref = dict(disk=(3.0, 9.0), disk_tex=disk_tex, disk_profile=dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0),
               spheres=sph, sphere_rgb=np.array(rgb), lamps=lamps)
    return fr, p, sky, ref


@pytest.mark.parametrize("kerr", [False, True], ids=["schw", "kerr"])
@pytest.mark.parametrize("S", [1, 5, 300])
@pytest.mark.parametrize("rs,obs,tex", [(False, False, False), (True, False, False), (True, True, False), (False, True, False),
                                        (False, False, True), (True, False, True), (False, True, True), (True, True, True)])
def test_polarised_shade(ctx, S, rs, obs, tex, kerr):
    import torch
    f = _ffi()
    fr, p, sky, ref = _scene_frame(ctx, S, kerr)
    sense = -1 if kerr else 1
    if rs:
        fr.set_redshift(("disk", "objects", "sky"), 4.0, disk_sense=sense)
    if obs:
        fr.observer = f.make_observer(BETA)       # the shade's observer (the rays stay the traced ones)
    if tex:
        fr.set_object_textures(rotations=[np.eye(3)], modes=["emissive"], emission=[2.0])
    plain = fr.shade().clone()
    t32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(t32)
    fr.set_polarisation(TABLE, disk_sense=sense)
    rgba, qu = fr.shade_stokes()
    rgba, qu = rgba.clone(), qu.clone()
    # the colour outputs are the textured call's, bit for bit, with and without polarisation set
    assert torch.equal(rgba, plain)
    assert torch.equal(fr.shade(), plain)
    s32 = torch.empty_like(t32)
    fr.shade_f32(s32)
    assert torch.equal(s32, t32)
    # Q / U against the restatement's shade
    end, flags, obj, k0 = fr.d_end.cpu().numpy(), fr.d_flags.cpu().numpy(), fr.d_obj.cpu().numpy(), fr.d_k0.cpu().numpy()
    spin = 0.45 if kerr else 0.0
    beta = BETA if obs else None
    if rs:
        g = (orf.observer_g_rays(fr.origin, k0, end, flags, 1.0, BETA, spin, kerr, sense) if obs
             else rr.g_rays(fr.origin, k0, end, flags, 1.0, spin, kerr, sense))
    else:
        g = np.ones(len(k0))
    n = fr.P * fr.S
    one = rr.shade_scene_redshift(end, flags, obj, n, 1, sky, g, 4.0, 7 if rs else 0, **ref)[:, :3]
    up = fr.rot @ np.array([0.0, 1.0, 0.0])
    chi, deg, _ = pr.pol_rays(fr.origin, k0, end, flags, 1.0, spin, kerr, sense, TABLE, up, beta)
    disk = flags == 128
    want = pr.shade_stokes(np.where(disk[:, None], one, 0.0), np.where(disk, chi, np.nan), deg, fr.P, fr.S)
    qu = qu.cpu().numpy()
    scale = np.abs(want).max()
    assert scale > 1e-3
    assert np.abs(qu - want).max() <= 1e-11 * max(scale, 1.0)
    fr.set_polarisation(None)
    with pytest.raises(RuntimeError):
        fr.shade_stokes()


def test_a_rotation_assigned_after_set_polarisation_turns_the_up_of_the_stokes_images(ctx):
    """set_polarisation() used to keep the camera's rotated +y of the moment it was called: a rotation assigned afterwards (the
    next frame of an animation) left the Stokes images on the old up, and they were not the images of a frame made with that
    rotation (found by tests/test_gpu_frame_sequences.py).  Nor may the records of the old rays be shaded any more."""
    import torch
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix
    fr, p, _, _ = _scene_frame(ctx, 2)
    fr.set_polarisation(TABLE, disk_sense=1)
    before = fr.shade_stokes()[1].clone()
    euler = (0.15, INC, -0.2)
    fr.rot = euler_xyz_matrix(euler)
    with pytest.raises(RuntimeError):
        fr.shade_stokes()
    fr.render(p)                                    # (makes the rays anew by itself: the rotation shapes them)
    rgba, qu = (t.clone() for t in fr.shade_stokes())
    fresh, _, _, _ = _scene_frame(ctx, 2, euler=euler)
    fresh.set_polarisation(TABLE, disk_sense=1)
    want_rgba, want_qu = fresh.shade_stokes()
    assert torch.equal(fr.d_k0, fresh.d_k0)
    assert torch.equal(rgba, want_rgba) and torch.equal(qu, want_qu)
    assert not torch.equal(qu, before) and float(qu.abs().max()) > 1e-3


def test_polarised_call_with_pol_null_is_the_textured_call(ctx):
    import torch
    f = _ffi()
    fr, p, sky, _ = _scene_frame(ctx, 3)
    today = fr.shade().clone()
    d64 = torch.empty_like(today)
    ctx.shade_scene_polarised_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, None, None, None, None, 0,
                                     x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(), d_rgba=d64.data_ptr(),
                                     d_object_id=fr.d_obj.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(d64, today)
    with pytest.raises(Exception):      # d_qu is required with pol
        ctx.shade_scene_polarised_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, None, None, None,
                                         f.make_polarisation(), 0, x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(),
                                         d_rgba=d64.data_ptr(), d_object_id=fr.d_obj.data_ptr())


# ---- end to end: the flat limit ----------------------------------------------------------------------------------------
def test_flat_limit_frame(ctx):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    r_s = 1e-8
    fr = DeviceFrame(ctx, 64, 48, 2, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM, rotation_euler=(0.0, INC, 0.0))
    fr.set_sky(synthetic_sky(128, 64))
    fr.set_disk(2.0, 12.0)
    p = _ffi().make_params(r_s=r_s, lambda_end=80.0, r_exit=40.0, disk_r_in=2.0, disk_r_out=12.0)
    fr.render(p)
    fr.set_polarisation(0.3)
    rgba, qu = fr.shade_stokes()
    torch.cuda.synchronize()
    flags, end, k0 = fr.d_flags.cpu().numpy(), fr.d_end.cpu().numpy(), fr.d_k0.cpu().numpy()
    d = flags == 128
    assert d.sum() > 1000
    up = fr.rot @ np.array([0.0, 1.0, 0.0])
    chi, deg, _ = fr.ctx.polarisation(k0, fr.origin, p, fr.polarisation, None, flags, end)
    ref = np.array([pr.flat_closed_form(fr.origin, e, up) for e in end[d, 0:3]])
    assert pr.chi_diff(chi[d], ref).max() < 1e-4
    assert np.all(deg[d] == 0.3)
    assert np.abs(qu.cpu().numpy()).max() > 0.0


# ---- the Python adaptors -----------------------------------------------------------------------------------------------
def test_trace_adaptor(ctx):
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorKerr, GeodesicIntegratorSchwarzschild
    f = _ffi()
    k0 = _inclined_rays(1500, seed=13)
    for gi, rhs, spin in ((GeodesicIntegratorSchwarzschild(mass=0.5, verbose=False, device=0), 0, 0.0),
                          (GeodesicIntegratorKerr(mass=0.5, a=0.9, verbose=False, device=0), 2, 0.45)):
        out = gi.trace(k0, CAM, curve_end=80.0, r_exit=40.0, disk=(3.0, 9.0),
                       polarisation=dict(degree=TABLE, disk_sense=-1, up=(0.0, 1.0, 0.0)))
        p = gi.params(np.inf, 80.0, 40.0, (3.0, 9.0))
        want = gi.context.polarisation(k0, CAM, p, f.make_polarisation(TABLE, -1), None, out["flags"], out["ray_end"])
        for key, w in zip(("evpa", "pol_degree", "mu_em"), want):
            assert np.array_equal(out[key], w, equal_nan=True)
        assert (out["flags"] == 128).sum() > 200


def test_device_frame_adaptor(ctx):
    import torch
    fr, p, sky, _ = _scene_frame(ctx, 3)
    fr.set_polarisation(TABLE, disk_sense=1)
    rgba, qu = fr.shade_stokes()
    d64, q2 = torch.empty_like(rgba), torch.empty_like(qu)
    ctx.shade_scene_polarised_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, None, None, None,
                                     _ffi().make_polarisation(TABLE, 1, fr.rot @ np.array([0.0, 1.0, 0.0])), q2.data_ptr(),
                                     x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(), d_rgba=d64.data_ptr(),
                                     d_object_id=fr.d_obj.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(d64, rgba) and torch.equal(q2, qu)

"""Moving and spinning object spheres on the GPU: bhg_redshift_motion_device / _host against the numpy
restatement (tests/object_motion_reference.py) on synthetic end records and on the library's own traces of an orbit scene, the
moving shade in every observer / texture / polarisation / thermal combination, "off is the thermal call" bit for bit, the library
frame against DeviceFrame, and the Doppler asymmetry of an emissive sphere on a circular orbit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import object_motion_reference as om  # noqa: E402
import redshift_reference as rr  # noqa: E402

R_S = 1.0
BETA = (0.2, -0.1, 0.15)
CAM = np.array([24.0, -6.0, 2.0])


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _orbit_scene(spin):
    """Three spheres: two on circular orbits (helper, locked and free), one at rest; v, w [3][3]."""
    from blackhole_geodesic_calculator_amd import observer
    a = spin
    sph, v, w = [], [], []
    for (ang, r, rho, sense, locked) in ((0.3, 8.0, 1.2, 1, True), (-0.5, 6.0, 0.9, -1, False)):
        R = np.sqrt(r * r + a * a)
        c = np.array([R * np.cos(ang), R * np.sin(ang), 0.0])
        vj, wj = observer.circular_orbit_motion(c, R_S, a, sense, locked=locked)
        sph.append([*c, rho])
        v.append(vj)
        w.append(wj)
    sph.append([5.0, 6.0, 1.0, 1.0])
    v.append(np.zeros(3))
    w.append(np.zeros(3))
    return np.array(sph), np.array(v), np.array(w)


def _rays_at(target, n, seed, fov=0.5):
    """n unit directions from CAM around the direction to target."""
    rng = np.random.default_rng(seed)
    fwd = (np.asarray(target, float) - CAM) / np.linalg.norm(np.asarray(target, float) - CAM)
    up = np.array([0.0, 0.0, 1.0])
    e1 = np.cross(fwd, up)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(e1, fwd)
    u, t = rng.uniform(-fov / 2, fov / 2, n), rng.uniform(-fov / 2, fov / 2, n)
    k = fwd[None, :] + u[:, None] * e1[None, :] + t[:, None] * e2[None, :]
    return k / np.linalg.norm(k, axis=1)[:, None]


def _device_g(ctx, p, rs, obs, mo, spheres, k0, end, flags, obj, x0):
    """bhg_redshift_motion_device, checked against the host form (the same launch) and returned."""
    import torch
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0)).cuda()
    d_end = torch.as_tensor(np.ascontiguousarray(end)).cuda()
    d_fl = torch.as_tensor(np.ascontiguousarray(flags)).cuda()
    d_obj = torch.as_tensor(np.ascontiguousarray(obj, dtype=np.int8)).cuda()
    g = torch.empty(len(k0), dtype=torch.float64, device="cuda")
    ctx.redshift_motion_device(p, rs, obs, mo, spheres, len(k0), d_k0.data_ptr(), d_fl.data_ptr(), g.data_ptr(), x0_shared=x0,
                               d_end=d_end.data_ptr(), d_object_id=d_obj.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    hg = ctx.redshift_motion(k0, x0, p, rs, obs, mo, spheres, flags, end, obj)
    assert np.array_equal(g, hg, equal_nan=True)
    return g


def _check_g(g, want):
    assert np.array_equal(np.isnan(g), np.isnan(want))
    z = want == 0.0
    assert np.all(g[z] == 0.0)
    ok = ~np.isnan(want) & ~z
    assert np.abs(g[ok] / want[ok] - 1.0).max() <= 1e-12


CASES = [("schw", 0, 0.0, None), ("schw_reduced", 1, 0.0, None), ("kerr", 2, 0.45, None), ("schw_obs", 0, 0.0, BETA),
         ("schw_reduced_obs", 1, 0.0, BETA), ("kerr_obs", 2, 0.45, BETA)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_per_ray_g_on_traces_of_the_orbit_scene(ctx, case):
    f = _ffi()
    name, rhs, spin, beta = case
    sph, v, w = _orbit_scene(spin)
    kerr = rhs == 2
    k0 = np.concatenate([_rays_at(s[:3], 1500, 11 + j, 0.12) for j, s in enumerate(sph)] + [_rays_at((0, 0, 0), 500, 5, 0.8)])
    p = f.make_params(r_s=R_S, lambda_end=80.0, r_exit=40.0, rhs_form=rhs, spin=spin)
    end, flags, _, _, obj = ctx.trace(k0, CAM, p, spheres=sph)
    for j in range(3):
        assert ((flags == 0x88) & (obj == j)).sum() > 200, j
    rs = f.make_redshift(disk_sense=1)
    obs = f.make_observer(beta) if beta is not None else None
    mo = f.make_object_motion(v, w)
    g = _device_g(ctx, p, rs, obs, mo, sph, k0, end, flags, obj, CAM)
    want = om.g_rays_motion(CAM, k0, end, flags, obj, sph, v, w, R_S, spin, kerr, 1, beta)
    _check_g(g, want)
    # the sphere at rest, and every other ray, is the call without motion bit for bit; motion = NULL is that call
    plain = ctx.redshift(k0, CAM, p, rs, flags, end) if obs is None else ctx.redshift_observer(k0, CAM, p, rs, obs, flags, end)
    moving = (flags == 0x88) & (obj < 2)
    assert np.array_equal(g[~moving], plain[~moving], equal_nan=True)
    assert not np.any(g[moving] == plain[moving])
    assert np.array_equal(ctx.redshift_motion(k0, CAM, p, rs, obs, None, sph, flags, end, obj), plain, equal_nan=True)
    assert np.array_equal(ctx.redshift_motion(k0, CAM, p, rs, obs, f.make_object_motion(), sph, flags, end, obj), plain,
                          equal_nan=True)


@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("rhs,spin", [(0, 0.0), (1, 0.0), (2, 0.45)])
def test_synthetic_records_disk_flow_identity(ctx, rhs, spin, sense):
    """Synthetic end records on a sphere whose surface moves with the disk's flow at z = 0: the disk's g, to 1e-12."""
    f = _ffi()
    kerr = rhs == 2
    rng = np.random.default_rng(21)
    n = 400
    ang = rng.uniform(0, 2 * np.pi, n)
    Rc = rng.uniform(4.0, 12.0, n)
    e = np.stack([Rc * np.cos(ang), Rc * np.sin(ang), np.zeros(n)], 1)
    if kerr:
        e *= (np.sqrt(Rc ** 2 + spin ** 2) / Rc)[:, None]
    d = rng.normal(size=(n, 3))
    k0 = rng.normal(size=(n, 3)) * 0.2 - CAM / np.linalg.norm(CAM)
    end = np.concatenate([e, d], 1)
    flags = np.full(n, 0x88, np.uint8)
    obj = np.arange(n) % 8
    p = f.make_params(r_s=R_S, rhs_form=rhs, spin=spin)
    rs = f.make_redshift(disk_sense=sense)
    want_disk = np.array([rr.g_one(CAM, k0[i], "disk", e[i], R_S, spin, kerr, sense) for i in range(n)])
    # one launch per sphere slot j: the rays of slot j carry V = the disk flow at their own point, as v (w = 0): each ray its
    # own sphere of 8, run 8 times over with that slot's velocity set per ray group
    got = np.empty(n)
    for i0 in range(0, n, 8):
        sl = slice(i0, i0 + 8)
        v = np.array([om.disk_flow(e[i], R_S, spin, kerr, sense) for i in range(i0, min(i0 + 8, n))])
        sph = np.array([[*(e[i] + [0.0, 0.0, 0.2]), 0.25] for i in range(i0, min(i0 + 8, n))])
        mo = f.make_object_motion(v, None)
        got[sl] = ctx.redshift_motion(k0[sl], CAM, p, rs, None, mo, sph, flags[sl], end[sl], obj[sl])
    assert np.abs(got / want_disk - 1.0).max() <= 1e-12


# ---- the moving shade ---------------------------------------------------------------------------------------------------
def _scene_frame(ctx, S, kerr=False):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    W_, H_ = (8, 6) if S > 256 else (40, 30)
    sky = synthetic_sky(256, 128)
    disk_tex = synthetic_sky(128, 32, seed=3)
    spin = 0.45 if kerr else 0.0
    sph, v, w = _orbit_scene(spin)
    fr = DeviceFrame(ctx, W_, H_, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=(22.0, 0.0, 4.0),
                     rotation_euler=(0.0, np.radians(80.0), 0.0))
    fr.set_sky(sky)
    fr.set_disk(3.0, 9.0, disk_tex, disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
    fr.set_objects(sph, [[1.0, 0.8, 0.6], [0.5, 0.5, 1.0], [0.9, 0.9, 0.9]], [[20.0, 0.0, 20.0, 10.0]])
    kw = dict(r_s=R_S, lambda_end=80.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)
    if kerr:
        kw.update(rhs_form=2, spin=spin)
    p = _ffi().make_params(**kw)
    fr.generate_rays()
    fr.trace(p)
    torch.cuda.synchronize()
    return fr, p, sph, v, w


def _per_ray(ctx, fr, p, rs, obs, ot, th, mo):
    """Every ray's colour from the library's shade, one ray per "pixel"."""
    import torch
    b = torch.empty((fr.P * fr.S, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_moving_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P * fr.S, 1, fr.scene(), p, rs, obs, ot, None, 0,
                                  th, mo, x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(), d_rgba=b.data_ptr(),
                                  d_object_id=fr.d_obj.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return b.cpu().numpy()[:, :3]


@pytest.mark.parametrize("kerr", [False, True], ids=["schw", "kerr"])
@pytest.mark.parametrize("S", [1, 5, 300])
@pytest.mark.parametrize("obs,tex,pol,therm", [(o, t, q, h) for o in (False, True) for t in (False, True) for q in (False, True)
                                               for h in (False, True)])
def test_moving_shade(ctx, S, obs, tex, pol, therm, kerr):
    import torch
    f = _ffi()
    fr, p, sph, v, w = _scene_frame(ctx, S, kerr)
    spin = 0.45 if kerr else 0.0
    fr.set_redshift(("disk", "objects", "sky"), 4.0, disk_sense=1)
    if obs:
        fr.observer = f.make_observer(BETA)
    if tex:
        fr.set_object_textures(rotations=[np.eye(3)], modes=["emissive", "lit", "emissive"], emission=[2.0, 1.0, 1.5])
    if therm:
        fr.set_disk_thermal(1.2e4, *f.narrowband(3e14, 6e14, 1e15), disk_sense=1)
    if pol:
        fr.set_polarisation((0.0, 0.35, 0.2), disk_sense=1)

    def shade():
        if pol:
            a, q = fr.shade_stokes()
            return a.clone(), q.clone()
        return fr.shade().clone(), None

    still, still_qu = shade()
    fr.set_object_motion(np.zeros((3, 3)), np.zeros((3, 3)))       # an all-zero motion is no motion, bit for bit
    zero, zero_qu = shade()
    assert torch.equal(zero, still) and (not pol or torch.equal(zero_qu, still_qu))
    fr.set_object_motion(v, w)
    got, got_qu = shade()
    fr.set_object_motion(None)
    assert torch.equal(shade()[0], still)
    if pol:
        assert torch.equal(got_qu, still_qu)      # motion does not touch disk rays
    # the restatement: every ray as the library shades it without motion; object rays of the moving spheres instead their
    # colour without the object weight, times g^4 of the restatement; the per-pixel mean in sample order
    rs_all, ot = fr.redshift, fr._object_textures() if fr._textured() else None
    th = fr.disk_thermal
    base = _per_ray(ctx, fr, p, rs_all, fr.observer, ot, th, None)
    unweighted = _per_ray(ctx, fr, p, f.make_redshift(("disk", "sky"), 4.0, 1), fr.observer, ot, th, None)
    end, flags, obj, k0 = fr.d_end.cpu().numpy(), fr.d_flags.cpu().numpy(), fr.d_obj.cpu().numpy(), fr.d_k0.cpu().numpy()
    g = om.g_rays_motion(fr.origin, k0, end, flags, obj, sph, v, w, R_S, spin, kerr, 1, BETA if obs else None)
    moving = (flags == 0x88) & (obj < 2)
    assert moving.sum() > (2 if S > 256 else 30)
    one = base.copy()
    g2 = g[moving] * g[moving]
    one[moving] = unweighted[moving] * (g2 * g2)[:, None]
    acc = np.zeros((fr.P, 3))
    for s in range(fr.S):
        acc += one[s * fr.P:(s + 1) * fr.P]
    want = acc * (1.0 / fr.S)
    have = got.cpu().numpy()[:, :3]
    assert np.abs(have - want).max() <= 1e-11 * max(np.abs(want).max(), 1.0)
    assert np.abs(have - still.cpu().numpy()[:, :3]).max() > 1e-6
    # the f32 output is the fp64 image rounded
    fr.set_object_motion(v, w)
    t32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(t32)
    assert torch.equal(t32, got.to(torch.float32))


def test_null_motion_is_the_thermal_call(ctx):
    import torch
    f = _ffi()
    fr, p, sph, v, w = _scene_frame(ctx, 3)
    fr.set_redshift(("disk", "objects", "sky"), 4.0, 1)
    th = f.make_disk_thermal(1.2e4, *f.narrowband(3e14, 6e14, 1e15))
    outs = []
    for mo in (None, f.make_object_motion(), "thermal"):
        d = torch.empty((fr.P, 4), dtype=torch.float64, device=fr.dev)
        common = dict(x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(), d_rgba=d.data_ptr(), d_object_id=fr.d_obj.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
        if mo == "thermal":
            ctx.shade_scene_thermal_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, fr.redshift, None,
                                           None, None, 0, th, **common)
        else:
            ctx.shade_scene_moving_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, fr.S, fr.scene(), p, fr.redshift, None,
                                          None, None, 0, th, mo, **common)
        torch.cuda.synchronize()
        outs.append(d)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    # redshift off: motion has no effect
    fr.set_redshift(None)
    still = fr.shade().clone()
    fr.set_object_motion(v, w)
    assert torch.equal(fr.shade(), still)


# ---- the library's frame ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one", "loopback"])
def test_library_frame_matches_device_frame(ctx, devices):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    f = _ffi()
    W_, H_, S = 48, 32, 3
    sky = synthetic_sky(128, 64)
    sph, v, w = _orbit_scene(0.0)
    rgb = [[1.0, 0.8, 0.6], [0.5, 0.5, 1.0], [0.9, 0.9, 0.9]]
    lamps = [[20.0, 0.0, 20.0, 10.0]]
    origin, euler = (22.0, 0.0, 4.0), (0.0, np.radians(80.0), 0.0)
    p = f.make_params(r_s=R_S, lambda_end=80.0, r_exit=40.0)
    gather = f.GATHER_AUTO if len(devices) == 1 else f.GATHER_COPY
    lf = f.Frame(devices, W_, H_, S, fov_x=0.9, fov_y=0.9, origin=origin, rot=euler_xyz_matrix(euler),
                 jitter=python_random_stream(42.0, 2 * S * W_ * H_), gather=gather, tile=16)
    try:
        lf.set_scene(sky, spheres=sph, sphere_rgb=rgb, lamps=lamps)
        lf.set_redshift(("objects", "sky"), 4.0, 1)
        plain = lf.render(p)
        lf.set_object_motion(v, w)
        got = lf.render(p)
        lf.set_object_motion(None)
        assert np.array_equal(lf.render(p), plain)
    finally:
        lf.close()
    assert np.abs(got - plain).max() > 1e-3
    dfr = DeviceFrame(ctx, W_, H_, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=origin, rotation_euler=euler)
    dfr.set_sky(sky)
    dfr.set_objects(sph, rgb, lamps)
    dfr.set_redshift(("objects", "sky"), 4.0, 1)
    dfr.set_object_motion(v, w)
    dfr.generate_rays()
    dfr.trace(p)
    out = torch.empty((W_ * H_, 4), dtype=torch.float32, device=dfr.dev)
    dfr.shade_f32(out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(H_, W_, 4), got)


# ---- a physical check ---------------------------------------------------------------------------------------------------
def test_orbiting_emissive_sphere_doppler_asymmetry(ctx):
    """An emissive white sphere on circular_orbit_motion at r = 8 r_s, locked, seen near edge-on from +x: its -y half turns
    towards the camera and is brighter; the ratio of the half means is the restatement's within 1 %."""
    import torch
    from blackhole_geodesic_calculator_amd import observer
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    f = _ffi()
    c = np.array([8.0 * R_S, 0.0, 0.0])
    v, w = observer.circular_orbit_motion(c, R_S)
    sph = np.array([[*c, 1.0]])
    fr = DeviceFrame(ctx, 64, 64, 1, fov_x=0.12, fov_y=0.12, origin=(30.0, 0.0, 0.5), rotation_euler=(0.0, np.radians(90.0), 0.0))
    fr.set_sky(np.zeros((8, 16, 4), np.float32))
    fr.set_objects(sph, [[1.0, 1.0, 1.0]], None)
    fr.set_object_textures(modes=["emissive"], emission=[1.0])
    fr.set_redshift(("objects",), 4.0, 1)
    fr.set_object_motion([v], [w])
    p = f.make_params(r_s=R_S, lambda_end=80.0, r_exit=40.0)
    fr.generate_rays()
    fr.trace(p)
    img = fr.shade().clone().cpu().numpy()[:, 0]
    torch.cuda.synchronize()
    end, flags, obj, k0 = fr.d_end.cpu().numpy(), fr.d_flags.cpu().numpy(), fr.d_obj.cpu().numpy(), fr.d_k0.cpu().numpy()
    hit = flags == 0x88
    towards, away = hit & (end[:, 1] < 0.0), hit & (end[:, 1] > 0.0)
    assert towards.sum() > 200 and away.sum() > 200
    ratio = img[towards].mean() / img[away].mean()
    g = om.g_rays_motion(fr.origin, k0, end, flags, obj, sph, [v], [w], R_S)
    predicted = (g[towards] ** 4).mean() / (g[away] ** 4).mean()
    assert ratio > 1.05
    assert abs(ratio / predicted - 1.0) <= 0.01
    # without motion the two halves are alike
    fr.set_object_motion(None)
    still = fr.shade().clone().cpu().numpy()[:, 0]
    assert abs(still[towards].mean() / still[away].mean() - 1.0) < 0.02


# ---- the Python adaptors -----------------------------------------------------------------------------------------------
def test_trace_adaptor(ctx):
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorKerr, GeodesicIntegratorSchwarzschild
    f = _ffi()
    for gi, spin in ((GeodesicIntegratorSchwarzschild(mass=0.5, verbose=False, device=0), 0.0),
                     (GeodesicIntegratorKerr(mass=0.5, a=0.9, verbose=False, device=0), 0.45)):
        sph, v, w = _orbit_scene(spin)
        k0 = np.concatenate([_rays_at(s[:3], 400, 3 + j, 0.12) for j, s in enumerate(sph)])
        out = gi.trace(k0, CAM, curve_end=80.0, r_exit=40.0, spheres=sph,
                       redshift=dict(disk_sense=1, object_motion=dict(velocity=v, angular_velocity=w)))
        p = gi.params(np.inf, 80.0, 40.0, None)
        want = gi.context.redshift_motion(k0, CAM, p, f.make_redshift(disk_sense=1), None, f.make_object_motion(v, w), sph,
                                          out["flags"], out["ray_end"], out["object_id"])
        assert np.array_equal(out["g"], want, equal_nan=True)
        plain = gi.trace(k0, CAM, curve_end=80.0, r_exit=40.0, spheres=sph, redshift=dict(disk_sense=1))
        assert not np.array_equal(out["g"], plain["g"], equal_nan=True)

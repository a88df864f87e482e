"""Disk crossings and layers on the GPU: bhg_trace_crossings_device against the scipy golden vectors
(every crossing of a non-terminal disk event), against the disk-off trace (the same steps), against the opaque disk (its first
crossing), its layer arrays through the per-ray redshift call, the layered shade against the numpy restatement
(tests/disk_layers_reference.py, fed the device's records) in its five instances, and the refusals.

The Kerr golden has no exit sphere (the scipy reference's Kerr solve has none; the Schwarzschild golden has r_exit = 35, beyond
its disks): golden parity never sees a crossing that shares its step with an exit event (the rule root <= terminal root), and
tests 2 and 3 (exit sphere at 40) compare the device with its own disk-off and opaque traces.  That rule, in all three forms, and
everything else the goldens' one parameter set leaves out is held to the C oracle's crossings mode by
tests/test_gpu_crossings_oracle.py (4133 Kerr rays with the exit sphere at 40 among them); the oracle's Kerr crossings with an
exit sphere are pinned on the CPU by tests/test_disk_crossings_host.py."""
import os
import sys

import numpy as np
import pytest

from conftest import frame_rays, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import disk_layers_reference as dl  # noqa: E402
import redshift_reference as rr  # noqa: E402

# restated from tests/test_gpu_parity.py: the stated fp64 bounds per class (Schwarzschild, Kerr) and the multiple of a record's
# own 1-ulp input sensitivity S_i that is allowed on top
STATED = {"escaped": (1e-8, 5e-8), "horizon": (5e-9, 1e-6), "disk": (1e-10, 1e-9)}
COND = 500.0
FORMS = [(0, 0.0), (1, 0.0), (2, 0.45)]
FORM_IDS = ["christoffel", "reduced", "kerr"]
SENTINEL = -7.25


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _crossings_device(ctx, p, k0, x0, K, layers_allocated=None):
    """bhg_trace_crossings_device on sentinel-filled arrays -> (end, flags, steps, acc, cross [layers_allocated, n, 6], n_cross)."""
    import torch
    n = len(k0)
    L = K if layers_allocated is None else layers_allocated
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0)).cuda()
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0)).cuda()
    d_end = torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_fl = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_ac = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_cr = torch.full((L, n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_nc = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    try:
        ctx.trace_crossings_device(p, n, d_k0.data_ptr(), K, d_end.data_ptr(), d_cr.data_ptr(), d_nc.data_ptr(),
                                   x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(),
                                   d_flags=d_fl.data_ptr(), d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return (d_end.cpu().numpy(), d_fl.cpu().numpy(), d_st.cpu().numpy().astype(np.uint32), d_ac.cpu().numpy().astype(np.uint32),
            d_cr.cpu().numpy(), d_nc.cpu().numpy())


# ---- 1. the golden vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_golden_parity(ctx, rhs, spin):
    f = _ffi()
    kerr = rhs == 2
    g = load_golden("kerr_disk_crossings" if kerr else "disk_crossings")
    fi = 0 if kerr else rhs
    bound = STATED["disk"][1 if kerr else 0]
    for d, (r_in, r_out) in enumerate(g["disks"]):
        p = f.make_params(r_s=float(g["r_s"]), lambda_end=float(g["lambda_end"]), rtol=float(g["rtol"]), atol=float(g["atol"]),
                          r_exit=0.0 if kerr else float(g["r_exit"]), rhs_form=rhs, spin=spin, disk_r_in=r_in, disk_r_out=r_out)
        end, flags, steps, acc, cross, n_cross = _crossings_device(ctx, p, g["k0"], g["x0"], 4)
        assert np.array_equal(n_cross, g["n_cross"][fi, d])
        assert np.array_equal(flags, g["flags"][fi])
        assert np.array_equal(steps, g["n_attempted"][fi]) and np.array_equal(acc, g["n_accepted"][fi])
        ref, S = g["cross"][fi, d], g["sens"][fi, d]
        have = np.arange(4)[:, None] < n_cross[None, :]
        assert np.all(cross[~have] == SENTINEL)                   # records a ray never reached are not written
        diff = np.abs(cross - ref).max(2)
        tol = bound + COND * S
        print(f"{FORM_IDS[rhs]} disk {(r_in, r_out)}: records {int(have.sum())}, worst |gpu - ref| {diff[have].max():.3e}, "
              f"worst excess over the stated bound {np.max(diff[have] - bound):.3e}, "
              f"worst on records with S_i <= bound / COND {diff[have & (S <= bound / COND)].max():.3e}")
        assert np.all(diff[have] <= tol[have]), (diff[have] - tol[have]).max()
        # the host-buffer call is the same launch
        h = ctx.trace_crossings(g["k0"], g["x0"], p, 4)
        assert np.array_equal(h[0], end) and np.array_equal(h[1], flags) and np.array_equal(h[5], n_cross)
        assert np.array_equal(np.isnan(h[4]).all(2), ~have) and not np.isnan(h[4][have]).any() and np.array_equal(h[4][have], cross[have])
        # two layers kept: the count is every crossing's, the first two records are the same bits, layer 2 is not written
        e2, f2, s2, a2, c2, n2 = _crossings_device(ctx, p, g["k0"], g["x0"], 2, layers_allocated=3)
        assert np.array_equal(n2, n_cross) and np.array_equal(f2, flags) and np.array_equal(e2, end)
        assert np.array_equal(c2[:2], cross[:2])
        assert np.all(c2[2] == SENTINEL)
    if not kerr:
        assert (g["n_cross"][fi, 1] == 3).sum() >= 5 and n_cross.max() == 3


# ---- 2. / 3. the disk-off trace and the opaque disk ------------------------------------------------------------------------
INC = np.radians(70.0)
CAM = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])
DISK = (3.0, 12.0)


def _inclined_rays(n, seed=5, fov=0.9):
    k = frame_rays(n, seed, fov)
    c, s = np.cos(INC), np.sin(INC)
    return k @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T


def _kw(rhs, spin, disk=True):
    # (camera at r = 30, exit sphere at 40: at lambda_end = 67 about a quarter of these rays has left through the sphere, the
    # rest are still inside)
    kw = dict(r_s=1.0, lambda_end=67.0, r_exit=40.0, rhs_form=rhs, spin=spin)
    if disk:
        kw.update(disk_r_in=DISK[0], disk_r_out=DISK[1])
    return kw


_TRACES = {}


def _traces(ctx, rhs, spin, n):
    """The three traces of one ray set, shared by the tests: crossings, disk off, opaque disk."""
    key = (rhs, n)
    if key not in _TRACES:
        f = _ffi()
        k0 = _inclined_rays(n)
        cr = _crossings_device(ctx, f.make_params(**_kw(rhs, spin)), k0, CAM, 3)
        off = ctx.trace(k0, CAM, f.make_params(**_kw(rhs, spin, disk=False)))
        opaque = ctx.trace(k0, CAM, f.make_params(**_kw(rhs, spin)))
        _TRACES[key] = (k0, cr, off, opaque)
    return _TRACES[key]


@pytest.mark.parametrize("n", [4096 + 37, 1])
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_same_steps_as_the_disk_off_trace(ctx, rhs, spin, n):
    k0, (end, flags, steps, acc, cross, n_cross), off, _ = _traces(ctx, rhs, spin, n)
    assert np.array_equal(flags, off[1])
    assert np.array_equal(steps, off[2]) and np.array_equal(acc, off[3])
    lam = flags == 4
    assert np.array_equal(end[lam], off[0][lam])                # no event: the same steps give the same bits
    d = np.abs(end - off[0]).max(1)
    col = 1 if rhs == 2 else 0
    esc, hor = flags == 8, (flags & 1) != 0
    assert np.all(lam | esc | hor)
    print(f"{FORM_IDS[rhs]} n={n}: lambda_end {int(lam.sum())}, exit {int(esc.sum())} worst {d[esc].max(initial=0.0):.3e}, "
          f"horizon {int(hor.sum())} worst {d[hor].max(initial=0.0):.3e}")
    assert d[esc].max(initial=0.0) <= STATED["escaped"][col]
    assert d[hor].max(initial=0.0) <= STATED["horizon"][col]
    if n > 1:
        assert lam.sum() > 100 and esc.sum() > 100 and hor.sum() > 50 and (n_cross >= 2).sum() > 20     # every class is there


def _sensitivity(oracle, k0, x0, ref_end, **kw):
    """tests/test_gpu_parity.py::_sensitivity: how far the oracle's end state moves when k0 moves by an ulp or two."""
    eps = np.finfo(float).eps
    pats = (np.nextafter(k0, np.inf), np.nextafter(k0, -np.inf), k0 * (1.0 + np.array([2.0, -2.0, 2.0]) * eps))
    return np.max([np.abs(oracle.trace(kp, x0, **kw)["end"] - ref_end).max(1) for kp in pats], axis=0)


@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_consistent_with_the_opaque_disk(ctx, oracle, rhs, spin):
    k0, (end, flags, steps, acc, cross, n_cross), _, opaque = _traces(ctx, rhs, spin, 4096 + 37)
    hit = opaque[1] == 128
    assert np.array_equal(hit, n_cross >= 1) and hit.sum() > 500
    kw = _kw(rhs, spin)
    o = oracle.trace(k0[hit], CAM, **kw)
    assert np.all(o["flags"] == 128)
    S = _sensitivity(oracle, k0[hit], CAM, o["end"], **kw)
    d = np.abs(cross[0][hit] - opaque[0][hit]).max(1)
    bound = STATED["disk"][1 if rhs == 2 else 0]
    print(f"{FORM_IDS[rhs]}: {int(hit.sum())} disk rays, worst |cross[0] - opaque end| {d.max():.3e}")
    assert np.all(d <= bound + COND * S), (d - (bound + COND * S)).max()


# ---- 4. a layer array is an end array of the per-ray calls -----------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_layer_arrays_feed_the_redshift_call(ctx, rhs, spin):
    f = _ffi()
    k0, (end, flags, steps, acc, cross, n_cross), _, _ = _traces(ctx, rhs, spin, 4096 + 37)
    sense = -1 if rhs == 2 else 1
    fl1 = dl.layer_flags(n_cross, 1)
    assert (fl1 == 128).sum() > 20
    g = ctx.redshift(k0, CAM, f.make_params(**_kw(rhs, spin)), f.make_redshift(disk_sense=sense), fl1, cross[1])
    want = rr.g_rays(CAM, k0, cross[1], fl1, 1.0, spin, rhs == 2, sense)
    on = fl1 == 128
    assert np.all(g[~on] == 0.0)
    assert np.abs(g[on] / want[on] - 1.0).max() <= 1e-12


# ---- 5. the layered shade --------------------------------------------------------------------------------------------------
BETA = (0.3, -0.2, 0.1)
T_PEAK, F_COL, SCALE = 1.2e4, 1.7, 2.5
NU = (3.0e14, 6.0e14, 1.0e15, 1.5e15)
W = np.array([[1.0, 0.5, 0.1, 0.0], [0.2, 1.0, 0.4, 0.1], [0.0, 0.1, 0.6, 1.0]])
PROFILE = dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0)
_FRAMES = {}


def _frame(ctx, S, kerr):
    """One traced frame per (S, kerr), shared by every instance and opacity: the crossings trace does not depend on them."""
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    key = (S, kerr)
    if key not in _FRAMES:
        f = _ffi()
        W_, H_ = (3, 3) if S > 256 else (32, 32)
        sky = synthetic_sky(256, 128)
        tex = synthetic_sky(128, 32, seed=3)
        fr = DeviceFrame(ctx, W_, H_, S, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM, rotation_euler=(0.0, INC, 0.0))
        fr.set_sky(sky)
        fr.set_disk(DISK[0], DISK[1], tex, **{"disk_" + a: b for a, b in PROFILE.items()})
        fr.set_disk_layers(3, 0.5)
        p = f.make_params(**_kw(2 if kerr else 0, 0.45 if kerr else 0.0))
        fr.generate_rays()
        fr.trace(p)
        torch.cuda.synchronize()
        host = dict(end=fr.d_end.cpu().numpy(), flags=fr.d_flags.cpu().numpy(), k0=fr.d_k0.cpu().numpy(),
                    cross=fr.d_cross.cpu().numpy(), n_cross=fr.d_n_cross.cpu().numpy())
        _FRAMES[key] = (fr, p, sky, tex, host)
    return _FRAMES[key]


_COLOURS = {}
INSTANCES = [(False, False, False), (True, False, False), (True, True, False), (True, False, True), (True, True, True)]


@pytest.mark.parametrize("kerr", [False, True], ids=["schw", "kerr"])
@pytest.mark.parametrize("S", [4, 300])
@pytest.mark.parametrize("opacity", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("rs,obs,therm", INSTANCES, ids=["plain", "rs", "rs_obs", "therm", "therm_obs"])
def test_layered_shade(ctx, S, kerr, opacity, rs, obs, therm):
    import torch
    f = _ffi()
    fr, p, sky, tex, h = _frame(ctx, S, kerr)
    sense = -1 if kerr else 1
    spin = 0.45 if kerr else 0.0
    if therm:
        fr.set_redshift(("sky",), 4.0, disk_sense=sense)     # (the thermal colour has its g in it: the sky alone is weighted)
    elif rs:
        fr.set_redshift(("disk", "sky"), 4.0, disk_sense=sense)
    else:
        fr.set_redshift(None)
    fr.observer = f.make_observer(BETA) if obs else None
    fr.set_disk_thermal(f.make_disk_thermal(T_PEAK, NU, W, F_COL, SCALE, sense) if therm else None)
    fr.disk_layers = f.make_disk_layers(3, opacity)          # (the trace does not depend on the opacity: shade alone)
    planted = None
    if opacity == 1.0:
        # nothing behind the first crossing is looked at: a NaN planted in every second record must not reach the image
        planted = fr.d_cross[1].clone()
        fr.d_cross[1].fill_(float("nan"))
    try:
        rgba = fr.shade().clone()
        t32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
        fr.shade_f32(t32)
        torch.cuda.synchronize()
    finally:
        if planted is not None:
            fr.d_cross[1].copy_(planted)
        fr.observer = None
        fr.set_redshift(None)
        fr.set_disk_thermal(None)
    got = rgba.cpu().numpy()
    assert np.all(np.isfinite(got))
    red = None
    if therm:
        red = dict(apply=rr.SKY, exponent=4.0, sense=sense)
    elif rs:
        red = dict(apply=rr.DISK | rr.SKY, exponent=4.0, sense=sense)
    common = dict(x0=CAM, k0=h["k0"], r_s=1.0, spin=spin, kerr=kerr, redshift=red, beta=BETA if obs else None)
    K = 1 if opacity == 1.0 else 3                           # opacity 1: the restatement with layer 0 alone
    key = (S, kerr, rs, obs, therm)
    if key not in _COLOURS:                                  # (the restated colours do not depend on the opacity: computed once)
        th = dict(sense=sense, t_peak=T_PEAK, nu=NU, weights=W, f_col=F_COL, scale=SCALE) if therm else None
        _COLOURS[key] = (dl.layer_colours(h["cross"], h["n_cross"], 3, DISK, disk_tex=tex, disk_profile=PROFILE, thermal=th, **common),
                         dl.behind_colour(h["end"], h["flags"], sky, **common))
    lay, behind = _COLOURS[key][0][:K], _COLOURS[key][1]
    if opacity == 1.0:
        behind = np.where((h["n_cross"] >= 1)[:, None], np.nan, behind)      # ... and no sky behind a disk ray
    want = dl.composite(lay, h["n_cross"], K, opacity, behind, h["flags"], fr.P, fr.S)
    assert np.all(np.isfinite(want))
    assert (h["n_cross"] >= 1).sum() > 0.2 * fr.n and (S > 256 or (h["n_cross"] >= 2).sum() > 20)
    err = np.abs(got - want).max()
    print(f"S={S} kerr={kerr} opacity={opacity} rs={rs} obs={obs} therm={therm}: worst |gpu - restatement| {err:.3e}")
    if therm:
        assert err <= 1e-11 * max(np.abs(want[:, :3]).max(), 1.0)
    else:
        assert err <= 1e-11
    assert np.abs(t32.cpu().numpy() - want).max() <= 1e-6 * (max(np.abs(want[:, :3]).max(), 1.0) if therm else 1.0)
    assert torch.equal(t32, rgba.to(torch.float32))


def test_layers_off_is_the_frame_that_never_had_them(ctx):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    p = f.make_params(**_kw(0, 0.0))
    images = []
    for use in (False, True):
        fr = DeviceFrame(ctx, 32, 32, 2, fov_x=0.9, fov_y=0.9, origin=CAM, rotation_euler=(0.0, INC, 0.0))
        fr.set_sky(synthetic_sky(256, 128))
        fr.set_disk(DISK[0], DISK[1], synthetic_sky(128, 32, seed=3))
        fr.set_redshift(("disk", "sky"), 4.0)
        if use:
            fr.set_disk_layers(3, 0.5)
            layered = fr.render(p).clone()
            with pytest.raises(ValueError):
                fr.shade_stokes()
            fr.set_disk_layers(None)
            with pytest.raises(RuntimeError):
                fr.shade()                                   # the layered trace's output is not the opaque trace's
        images.append(fr.render(p).clone())
        if use:
            # the layers did something
            assert not torch.equal(layered, images[0])
            fr.set_objects([[6.0, 3.0, 2.5, 1.5]], [[1.0, 0.8, 0.6]], [[20.0, 0.0, 20.0, 10.0]])
            fr.set_disk_layers(2, 0.5)
            with pytest.raises(ValueError):
                fr.trace(p)
    assert torch.equal(images[0], images[1])


# ---- 6. the refusals leave the outputs alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,K", [(dict(method=1), 3), (dict(time_like=1), 3), (dict(disk_r_in=0.0, disk_r_out=0.0), 3), (dict(), 0),
                                  (dict(), 5)], ids=["rk4", "time_like", "no_disk", "K0", "K5"])
def test_trace_refusals_leave_the_outputs_untouched(ctx, kw, K):
    f = _ffi()
    base = _kw(0, 0.0)
    base.update(kw)
    k0 = _inclined_rays(100)
    import torch
    n = len(k0)
    d_k0 = torch.as_tensor(k0).cuda()
    outs = [torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((4, n, 6), SENTINEL, dtype=torch.float64, device="cuda"),
            torch.full((n,), 255, dtype=torch.uint8, device="cuda"), torch.full((n,), 255, dtype=torch.uint8, device="cuda")]
    with pytest.raises(f.BhgError) as e:
        ctx.trace_crossings_device(f.make_params(**base), n, d_k0.data_ptr(), K, outs[0].data_ptr(), outs[1].data_ptr(),
                                   outs[2].data_ptr(), x0_shared=CAM, d_flags=outs[3].data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == f.E_INVALID
    torch.cuda.synchronize()
    assert all(bool((o == (SENTINEL if o.dtype == torch.float64 else 255)).all()) for o in outs)
    with pytest.raises(f.BhgError):
        ctx.trace_crossings(k0, CAM, f.make_params(**base), K)


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=5), dict(opacity=0.0), dict(spheres=True)], ids=["K0", "K5", "opacity0", "spheres"])
def test_shade_refusals_leave_the_image_untouched(ctx, kw):
    import torch
    f = _ffi()
    fr, p, sky, tex, h = _frame(ctx, 4, False)
    sc = fr.scene()
    if kw.get("spheres"):
        sc = f.make_scene(fr.d_sky.data_ptr(), fr.sky_wh[0], fr.sky_wh[1], disk=DISK, spheres=[[6.0, 3.0, 2.5, 1.5]])
    img = torch.full((fr.P, 4), SENTINEL, dtype=torch.float64, device=fr.dev)
    with pytest.raises(f.BhgError) as e:
        ctx.shade_disk_layers_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.d_cross.data_ptr(), fr.d_n_cross.data_ptr(),
                                     fr.P, fr.S, sc, f.make_disk_layers(kw.get("K", 3), kw.get("opacity", 0.5)), params=p,
                                     x0_shared=fr.origin, d_k0=fr.d_k0.data_ptr(), d_rgba=img.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == f.E_INVALID
    torch.cuda.synchronize()
    assert bool((img == SENTINEL).all())


# ---- the Python adaptor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kerr", [False, True], ids=["schw", "kerr"])
def test_integrator_returns_the_layers(ctx, kerr):
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorKerr, GeodesicIntegratorSchwarzschild
    f = _ffi()
    rhs, spin = (2, 0.45) if kerr else (0, 0.0)
    sense = -1 if kerr else 1
    k0, (end, flags, steps, acc, cross, n_cross), _, _ = _traces(ctx, rhs, spin, 4096 + 37)
    gi = GeodesicIntegratorKerr(mass=0.5, a=0.9, context=ctx) if kerr else GeodesicIntegratorSchwarzschild(mass=0.5, context=ctx)
    th = dict(t_peak=T_PEAK, nu=NU, weights=W, f_col=F_COL, scale=SCALE, disk_sense=sense)
    out = gi.trace(k0.reshape(-1, 1, 3), CAM, curve_end=67.0, r_exit=40.0, disk=DISK, disk_crossings=3,
                   redshift=dict(disk_sense=sense), polarisation=dict(degree=0.2, disk_sense=sense), disk_thermal=th)
    n = len(k0)
    assert out["disk_cross"].shape == (3, n, 1, 6) and out["n_cross"].shape == (n, 1) and out["thermal_rgb"].shape == (3, n, 1, 3)
    assert np.array_equal(out["n_cross"][:, 0], n_cross) and np.array_equal(out["flags"][:, 0], flags)
    assert np.array_equal(out["ray_end"][:, 0], end)
    have = np.arange(3)[:, None] < n_cross[None, :]
    assert np.array_equal(out["disk_cross"][:, :, 0][have], cross[have]) and np.all(np.isnan(out["disk_cross"][:, :, 0][~have]))
    p = f.make_params(**_kw(rhs, spin))
    for m in range(3):
        fl = dl.layer_flags(n_cross, m)
        g = ctx.redshift(k0, CAM, p, f.make_redshift(apply=(), disk_sense=sense), fl, cross[m])
        on = have[m]
        assert m == 2 or on.sum() > 20              # (this disk has no third-order crossing: layer 2 is all NaN)
        assert np.array_equal(out["g"][m, :, 0][on], g[on]) and np.all(np.isnan(out["g"][m, :, 0][~on]))
        for name in ("evpa", "pol_degree", "mu_em", "t_em"):
            assert out[name].shape == (3, n, 1)
            assert np.all(np.isfinite(out[name][m, :, 0][on])) and np.all(np.isnan(out[name][m, :, 0][~on]))
        assert np.all(np.isnan(out["thermal_rgb"][m, :, 0][~on]))
    with pytest.raises(ValueError):
        gi.trace(k0, CAM, disk=DISK, disk_crossings=3, spheres=[[6.0, 3.0, 2.5, 1.5]])
    with pytest.raises(ValueError):
        gi.trace(k0, CAM, disk_crossings=3)

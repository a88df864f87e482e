"""Light travel time on the GPU: bhg_travel_time_device bit for bit beside the crossings trace and the
plain trace, its times against the scipy golden vectors (tests/golden/travel_time.npz) and the closed-form radial ray, the special
values, the shapes, the host-buffer call, the retarded layer shade through DeviceFrame against the numpy restatement, and
trace(travel_time=True).

Measured on an MI355X when this was written (the criterion is |dt_gpu - dt_ref| <= max(COND S_i, floor), every kept ray compared;
test_golden_times prints the figures again with -s): over the nine (set, form) pairs the worst |dt_gpu - dt_ref| is 3.3e-8 absolute,
5.8e-10 relative, 11.9 S_i and 0.024 of the tolerance (schw_default; the tight sets: 2.6e-12, 4.8e-14, 8.0 S_i, 0.008); the radial ray
is 2.2e-16 from 32 + ln 17; the retarded shade is 7.1e-15 from the restatement (bound 1e-11); 0 of 600 end states differ from the
plain trace's with the disk off."""
import os
import sys

import numpy as np
import pytest

from conftest import frame_rays, load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_reference as cr  # noqa: E402
import disk_layers_reference as dl  # noqa: E402
import redshift_reference as rr  # noqa: E402
import travel_time_reference as tt  # noqa: E402

FORMS = [(0, 0.0), (1, 0.0), (2, 0.45)]
FORM_IDS = ["christoffel", "reduced", "kerr"]
SENTINEL = -7.25
DISK = (3.0, 12.0)
COND = tt.COND


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _travel_time_device(ctx, p, k0, x0, K, layers_allocated=None):
    """bhg_travel_time_device on sentinel-filled arrays -> dict of host arrays (cross, t_cross: the K layers asked for, or all
    layers_allocated of a larger allocation)."""
    import torch
    n = len(k0)
    L = max(K, 1) if layers_allocated is None else layers_allocated
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0)).cuda()
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0)).cuda()
    d_end = torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_fl = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_ac = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_cr = torch.full((L, n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_tc = torch.full((L, n), SENTINEL, dtype=torch.float64, device="cuda")
    d_nc = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_te = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    try:
        ctx.travel_time_device(p, n, d_k0.data_ptr(), K, d_end.data_ptr(), d_te.data_ptr(), d_cross=d_cr.data_ptr() if K else 0,
                               d_n_cross=d_nc.data_ptr(), d_t_cross=d_tc.data_ptr() if K else 0,
                               x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(), d_flags=d_fl.data_ptr(),
                               d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    keep = K if layers_allocated is None else L
    return dict(end=d_end.cpu().numpy(), flags=d_fl.cpu().numpy(), steps=d_st.cpu().numpy().astype(np.uint32),
                acc=d_ac.cpu().numpy().astype(np.uint32), cross=d_cr.cpu().numpy()[:keep], n_cross=d_nc.cpu().numpy(),
                t_end=d_te.cpu().numpy(), t_cross=d_tc.cpu().numpy()[:keep])


def _crossings_device(ctx, p, k0, x0, K):
    import torch
    n = len(k0)
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0)).cuda()
    d_end = torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_fl = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_ac = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_cr = torch.full((K, n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_nc = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    try:
        ctx.trace_crossings_device(p, n, d_k0.data_ptr(), K, d_end.data_ptr(), d_cr.data_ptr(), d_nc.data_ptr(), x0_shared=x0,
                                   d_flags=d_fl.data_ptr(), d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return dict(end=d_end.cpu().numpy(), flags=d_fl.cpu().numpy(), steps=d_st.cpu().numpy().astype(np.uint32),
                acc=d_ac.cpu().numpy().astype(np.uint32), cross=d_cr.cpu().numpy(), n_cross=d_nc.cpu().numpy())


INC = np.radians(70.0)
CAM = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])


def _inclined_rays(n, seed=5, fov=0.9):
    k = frame_rays(n, seed, fov)
    c, s = np.cos(INC), np.sin(INC)
    return k @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T


def _mixed_rays(n):
    """Two thirds frame rays, a third crossings_reference.camera_rays (two fifths of those around the critical impact parameter,
    where the higher-order crossings and the rays that cross the disk on their way into the hole live)."""
    m = n // 3
    return np.concatenate([_inclined_rays(n - m), cr.camera_rays(CAM, m, np.random.default_rng(11))])


def _kw(rhs, spin, disk=True):
    # (tests/test_gpu_disk_crossings.py's: camera at r = 30, exit sphere at 40, lambda_end = 67 -- rays that leave through the
    # sphere, rays still inside, rays that end in the hole)
    kw = dict(r_s=1.0, lambda_end=67.0, r_exit=40.0, rhs_form=rhs, spin=spin)
    if disk:
        kw.update(disk_r_in=DISK[0], disk_r_out=DISK[1])
    return kw


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. bit for bit beside the crossings trace and the plain trace ----------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_everything_else_is_the_crossings_trace(ctx, rhs, spin):
    f = _ffi()
    k0 = _mixed_rays(600)
    p = f.make_params(**_kw(rhs, spin))
    for K in (3, 1):
        t = _travel_time_device(ctx, p, k0, CAM, K)
        c = _crossings_device(ctx, p, k0, CAM, K)
        _same(t, c, ("end", "flags", "steps", "acc", "cross", "n_cross"))
        have = np.arange(K)[:, None] < t["n_cross"][None, :]
        assert np.all(t["t_cross"][~have] == SENTINEL)            # slots a ray never reached are not written, like cross's
        assert not np.isnan(t["t_cross"][have]).any() and np.all(t["t_cross"][have] > 0.0)
    assert (t["n_cross"] >= 2).sum() >= 1 and (t["flags"] == 8).sum() > 20 and (t["flags"] & 1).sum() > 10
    # no records: the counts and the end times are the same
    z = _travel_time_device(ctx, p, k0, CAM, 0)
    _same(z, t, ("end", "flags", "steps", "acc", "n_cross", "t_end"))


@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_with_a_disk_and_no_records_it_is_the_crossings_trace(ctx, rhs, spin):
    """With a disk and no records the results are the crossings trace's; beside the plain trace they stand as that trace does
    (tests/test_gpu_disk_crossings.py): flags and step counts on every ray, the end state bit for bit where no event ends the
    ray, and within the stated fp64 bounds where one does (the trace kernels settle a lone exit-sphere event with their
    certified Newton search, the crossings loops with Brent: the same root to 4 eps, not the same iterate).  The times do not
    depend on which of the two stored the end state."""
    f = _ffi()
    k0 = _mixed_rays(600)
    z = _travel_time_device(ctx, f.make_params(**_kw(rhs, spin, disk=False)), k0, CAM, 0)
    t = _travel_time_device(ctx, f.make_params(**_kw(rhs, spin)), k0, CAM, 0)
    c = _crossings_device(ctx, f.make_params(**_kw(rhs, spin)), k0, CAM, 1)
    _same(t, c, ("end", "flags", "steps", "acc", "n_cross"))
    off = ctx.trace(k0, CAM, f.make_params(**_kw(rhs, spin, disk=False)))
    assert np.array_equal(t["flags"], off[1]) and np.array_equal(t["steps"], off[2]) and np.array_equal(t["acc"], off[3])
    assert np.all(z["n_cross"] == 0) and np.array_equal(z["t_end"], t["t_end"], equal_nan=True)
    lam = t["flags"] == 4
    assert lam.sum() > 20 and np.array_equal(t["end"][lam], off[0][lam])
    d = np.abs(t["end"] - off[0]).max(1)
    col = 1 if rhs == 2 else 0
    print(f"{FORM_IDS[rhs]}: worst |end - plain trace's| on event rays {d[~lam].max():.3e}, rays that differ {int((d > 0).sum())}")
    assert d[t["flags"] == 8].max() <= (1e-8, 5e-8)[col] and d[(t["flags"] & 1) != 0].max() <= (5e-9, 1e-6)[col]


@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_disk_off_equals_the_plain_trace_bit_for_bit(ctx, rhs, spin):
    """With the disk off, end / flags / n_steps / n_accepted equal bhg_trace_device's bit for bit, on every ray."""
    f = _ffi()
    k0 = _mixed_rays(600)
    t = _travel_time_device(ctx, f.make_params(**_kw(rhs, spin, disk=False)), k0, CAM, 0)
    off = ctx.trace(k0, CAM, f.make_params(**_kw(rhs, spin, disk=False)))
    differ = np.flatnonzero((t["end"] != off[0]).any(1))
    print(f"{FORM_IDS[rhs]}: {len(differ)} of {len(k0)} end states differ, flags of those {np.unique(t['flags'][differ])}, "
          f"worst {np.abs(t['end'] - off[0]).max():.3e}")
    assert np.array_equal(t["flags"], off[1]) and np.array_equal(t["steps"], off[2]) and np.array_equal(t["acc"], off[3])
    assert np.array_equal(t["end"], off[0])


# ---- 2. the times against the golden vectors -----------------------------------------------------------------------------------
SETS = ("schw_default", "kerr_default", "schw_nodisk", "kerr_nodisk", "schw_tight", "kerr_tight")


@pytest.mark.parametrize("name", SETS)
def test_golden_times(ctx, name):
    f = _ffi()
    g = load_golden("travel_time")
    get = lambda k: g[f"{name}__{k}"]      # noqa: E731
    disk = tuple(get("disk"))
    K = 4 if disk[1] > 0.0 else 0
    for fi, form in enumerate(get("forms")):
        p = f.make_params(r_s=float(get("r_s")), lambda_end=float(get("lambda_end")), rtol=float(get("rtol")), atol=float(get("atol")),
                          r_exit=float(get("r_exit")[fi]), rhs_form=int(form), spin=float(get("spin")), disk_r_in=disk[0],
                          disk_r_out=disk[1])
        t = _travel_time_device(ctx, p, get("k0"), get("x0"), K)
        assert np.array_equal(t["flags"], get("flags")[fi]) and np.array_equal(t["n_cross"], get("n_cross")[fi])
        assert np.array_equal(t["steps"], get("n_attempted")[fi]) and np.array_equal(t["acc"], get("n_accepted")[fi])
        floor = float(get("floor")[fi])
        ref = np.concatenate([get("t_end")[fi][None, :], get("t_cross")[fi][:K]])
        S = np.concatenate([get("S_end")[fi][None, :], get("S_cross")[fi][:K]])
        got = np.concatenate([t["t_end"][None, :], t["t_cross"]])
        have = ~np.isnan(ref)                                     # every time the reference has: none skipped
        assert np.array_equal(np.isinf(got[have]), np.isinf(ref[have])) and not np.isnan(got[have]).any()
        assert np.all(got[~have] == SENTINEL)
        fin = have & np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin])
        tol = np.maximum(COND * S[fin], floor)
        with np.errstate(divide="ignore", invalid="ignore"):
            mult = np.where(S[fin] > 0.0, err / S[fin], 0.0)
        print(f"{name} form {int(form)}: {int(fin.sum())} finite times of {int(have.sum())}, floor {floor:.2e}, worst |gpu - ref| "
              f"{err.max():.3e} absolute, {(err / ref[fin]).max():.3e} relative, {mult.max():.1f} S_i; worst err / tol {(err / tol).max():.3f}")
        assert np.all(err <= tol), (err / tol).max()


# ---- 3. the closed-form radial ray ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs", [0, 1], ids=["christoffel", "reduced"])
def test_radial_ray_closed_form(ctx, rhs):
    # 32 + ln(34 / 2): about 400 terms of a few ulp each, times ten
    f = _ffi()
    p = f.make_params(r_s=1.0, lambda_end=120.0, r_exit=35.0, max_step=0.5, rhs_form=rhs)
    t = _travel_time_device(ctx, p, np.array([[0.0, 0.0, 1.0]]), np.array([0.0, 0.0, 3.0]), 0)
    exact = 32.0 + np.log(34.0 / 2.0)
    rel = abs(t["t_end"][0] / exact - 1.0)
    print(f"{FORM_IDS[rhs]}: {t['acc'][0]} steps, t_end {t['t_end'][0]!r}, relative distance from 32 + ln 17 {rel:.2e}")
    assert t["flags"][0] == 8 and rel <= 1e-12
    # ... and the length of k0 does not matter
    t2 = _travel_time_device(ctx, f.make_params(r_s=1.0, lambda_end=120.0, r_exit=35.0, max_step=0.2, rhs_form=rhs),
                             np.array([[0.0, 0.0, 2.5]]), np.array([0.0, 0.0, 3.0]), 0)
    assert abs(t2["t_end"][0] / exact - 1.0) <= 1e-12


# ---- 4. special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_special_values(ctx, rhs, spin):
    f = _ffi()
    cam = cr.inclined_camera(30.0, 60.0, 0.5 if rhs == 2 else 0.0)
    look = -cam / np.linalg.norm(cam)
    k0 = np.stack([look + np.array([0.0, 0.02, 0.0]),             # into the hole
                   look + np.array([0.0, 0.3, 0.1]),              # past it
                   look + np.array([0.0, 0.02, 0.0]),             # starts inside (per-ray origin below)
                   np.array([np.nan, 0.0, 1.0])])                 # NaN
    x0 = np.stack([cam, cam, 0.3 * cam / np.linalg.norm(cam), cam])
    p = f.make_params(r_s=1.0, lambda_end=120.0, r_exit=35.0, rhs_form=rhs, spin=spin, disk_r_in=1.2, disk_r_out=15.0)
    t = _travel_time_device(ctx, p, k0, x0, 2)
    assert t["flags"][0] == 1 and t["t_end"][0] == np.inf
    assert t["flags"][1] in (4, 8) and np.isfinite(t["t_end"][1]) and t["t_end"][1] > 30.0
    assert t["flags"][2] == 3 and t["t_end"][2] == np.inf and t["n_cross"][2] == 0 and np.all(t["t_cross"][:, 2] == SENTINEL)
    assert t["flags"][3] & 64 and np.isnan(t["t_end"][3])
    # a step budget that runs out: the time up to the state returned, finite and short of the full one
    p2 = f.make_params(r_s=1.0, lambda_end=120.0, r_exit=35.0, rhs_form=rhs, spin=spin, max_steps=6)
    s = _travel_time_device(ctx, p2, k0[1:2], cam, 0)
    assert s["flags"][0] == 16 and 0.0 < s["t_end"][0] < t["t_end"][1]
    # a crossing in front of a horizon ending stays finite: rays that pass through the disk and end in the hole
    w = _travel_time_device(ctx, p, _mixed_rays(600), CAM, 2)
    both = ((w["flags"] & 1) != 0) & (w["n_cross"] >= 1)
    print(f"{FORM_IDS[rhs]}: {int(both.sum())} rays cross the disk and end in the hole")
    assert both.sum() >= 3 and np.all(np.isinf(w["t_end"][both])) and np.all(np.isfinite(w["t_cross"][0][both]))
    assert np.all((w["t_cross"][0][both] > 15.0) & (w["t_cross"][0][both] < 80.0))


# ---- 5. shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_shapes_and_permutation(ctx, rhs, spin):
    f = _ffi()
    p = f.make_params(**_kw(rhs, spin))
    k0 = _inclined_rays(200, seed=9)
    full = _travel_time_device(ctx, p, k0, CAM, 3)
    keys = ("end", "flags", "steps", "acc", "n_cross", "t_end")
    for n in (1, 63, 64, 65):
        part = _travel_time_device(ctx, p, k0[:n], CAM, 3)
        for k in keys:
            assert np.array_equal(part[k], full[k][:n], equal_nan=True), (n, k)
        assert np.array_equal(part["t_cross"], full["t_cross"][:, :n]) and np.array_equal(part["cross"], full["cross"][:, :n])
    perm = np.random.default_rng(3).permutation(200)
    q = _travel_time_device(ctx, p, k0[perm], CAM, 3)
    for k in keys:
        assert np.array_equal(q[k], full[k][perm], equal_nan=True), k
    assert np.array_equal(q["t_cross"], full["t_cross"][:, perm]) and np.array_equal(q["cross"], full["cross"][:, perm])
    # per-ray origins: the same rays, the same bits
    own = _travel_time_device(ctx, p, k0, np.tile(CAM, (200, 1)), 3)
    for k in keys + ("t_cross", "cross"):
        assert np.array_equal(own[k], full[k], equal_nan=True), k


# ---- 6. the host-buffer call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", FORMS, ids=FORM_IDS)
def test_host_call_is_the_device_call(ctx, rhs, spin):
    f = _ffi()
    k0 = _inclined_rays(200, seed=9)
    for K, disk in ((3, True), (0, True), (0, False)):
        p = f.make_params(**_kw(rhs, spin, disk=disk))
        d = _travel_time_device(ctx, p, k0, CAM, K)
        end, flags, steps, acc, cross, n_cross, t_end, t_cross = ctx.travel_time(k0, CAM, p, K)
        assert np.array_equal(end, d["end"]) and np.array_equal(flags, d["flags"]) and np.array_equal(steps, d["steps"])
        assert np.array_equal(acc, d["acc"]) and np.array_equal(n_cross, d["n_cross"]) and np.array_equal(t_end, d["t_end"], equal_nan=True)
        have = np.arange(K)[:, None] < n_cross[None, :]
        assert t_cross.shape == (K, 200) and np.array_equal(np.isnan(t_cross), ~have)
        assert np.array_equal(t_cross[have], d["t_cross"][have]) and np.array_equal(cross[have], d["cross"][have])


# ---- 7. the retarded shade through DeviceFrame ---------------------------------------------------------------------------------
INC80 = np.radians(80.0)
CAM80 = np.array([30 * np.sin(INC80), 0.0, 30 * np.cos(INC80)])
PROFILE = dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0)
BETA = (0.3, -0.2, 0.1)


@pytest.mark.parametrize("rs,obs", [(False, False), (True, False), (True, True)], ids=["plain", "rs", "rs_obs"])
def test_retarded_shade(ctx, rs, obs):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    sky, tex = synthetic_sky(256, 128), synthetic_sky(128, 32, seed=3)
    p = f.make_params(r_s=1.0, lambda_end=120.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1])

    def frame(rate):
        fr = DeviceFrame(ctx, 16, 16, 2, fov_x=0.9, fov_y=0.9, sampling_seed=42.0, origin=CAM80, rotation_euler=(0.0, INC80, 0.0))
        fr.set_sky(sky)
        fr.set_disk(DISK[0], DISK[1], tex, **{"disk_" + a: b for a, b in PROFILE.items()})
        if rs:
            fr.set_redshift(("disk", "sky"), 4.0, disk_sense=1)
        fr.observer = f.make_observer(BETA) if obs else None
        if rate is None:
            fr.set_disk_layers(3, 0.5)
        else:
            fr.set_disk_layers(3, 0.5, phase_rate=rate)
        fr.generate_rays(p)
        fr.trace(p)
        img = fr.shade().clone()
        t32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
        fr.shade_f32(t32)
        torch.cuda.synchronize()
        return fr, img, t32

    fr0, today, today32 = frame(None)
    frz, zero, zero32 = frame(0.0)
    assert frz.d_t_cross is None and torch.equal(zero, today) and torch.equal(zero32, today32)     # phase_rate = 0: today's image
    fr, img, t32 = frame(0.05)
    assert fr.d_t_cross is not None and fr.d_t_end is not None
    assert torch.equal(fr.d_n_cross, fr0.d_n_cross) and torch.equal(fr.d_end, fr0.d_end) and torch.equal(fr.d_flags, fr0.d_flags)
    wrote = torch.arange(3, device=fr.dev)[:, None] < fr.d_n_cross[None, :]          # (slots no ray reached hold what the allocation held)
    assert torch.equal(fr.d_cross[wrote], fr0.d_cross[wrote]) and bool(torch.isfinite(fr.d_t_cross[wrote]).all())
    assert not torch.equal(img, today)
    h = dict(end=fr.d_end.cpu().numpy(), flags=fr.d_flags.cpu().numpy(), k0=fr.d_k0.cpu().numpy(), cross=fr.d_cross.cpu().numpy(),
             n_cross=fr.d_n_cross.cpu().numpy(), t_cross=fr.d_t_cross.cpu().numpy())
    red = dict(apply=rr.DISK | rr.SKY, exponent=4.0, sense=1) if rs else None
    common = dict(x0=CAM80, k0=h["k0"], r_s=1.0, spin=0.0, kerr=False, redshift=red, beta=BETA if obs else None)
    lay = tt.retarded_layer_colours(h["cross"], h["n_cross"], h["t_cross"], 0.05, 3, DISK, disk_tex=tex, disk_profile=PROFILE, **common)
    behind = dl.behind_colour(h["end"], h["flags"], sky, **common)
    want = dl.composite(lay, h["n_cross"], 3, 0.5, behind, h["flags"], fr.P, fr.S)
    got = img.cpu().numpy()
    assert (h["n_cross"] >= 1).sum() > 0.1 * fr.n and (h["n_cross"] >= 2).sum() >= 1
    err = np.abs(got - want).max()
    moved = np.abs(got - today.cpu().numpy()).max()
    print(f"rs={rs} obs={obs}: worst |gpu - restatement| {err:.3e}; the retarded image differs from today's by up to {moved:.3e}")
    assert np.all(np.isfinite(want)) and err <= 1e-11           # tests/test_gpu_disk_crossings.py's bound for the layered shade
    assert torch.equal(t32, img.to(torch.float32))
    # a crossing time that is not finite: the layer is black and still absorbs
    planted = fr.d_t_cross[0].clone()
    fr.d_t_cross[0].fill_(float("inf"))
    try:
        dark = fr.shade().clone().cpu().numpy()
    finally:
        fr.d_t_cross[0].copy_(planted)
    lay_dark = lay.copy()
    lay_dark[0][h["n_cross"] >= 1] = 0.0
    assert np.abs(dark - dl.composite(lay_dark, h["n_cross"], 3, 0.5, behind, h["flags"], fr.P, fr.S)).max() <= 1e-11
    # changing the rate asks for a new trace
    fr.set_disk_layers(3, 0.5)
    with pytest.raises(RuntimeError):
        fr.shade()


# ---- 8. trace(travel_time=True) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kerr", [False, True], ids=["schw", "kerr"])
def test_integrator_returns_the_times(ctx, kerr):
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorKerr, GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorKerr(mass=0.5, a=0.9, context=ctx) if kerr else GeodesicIntegratorSchwarzschild(mass=0.5, context=ctx)
    k0 = _inclined_rays(96).reshape(8, 12, 3)
    kw = dict(curve_end=67.0, r_exit=40.0)
    plain = gi.trace(k0, CAM, **kw)
    out = gi.trace(k0, CAM, travel_time=True, **kw)
    assert set(out) == set(plain) | {"t"} and out["t"].shape == (8, 12)
    for k in plain:
        assert np.array_equal(out[k], plain[k]), k
    hor = (out["flags"] & 1) != 0
    assert np.all(np.isinf(out["t"][hor])) and np.all(np.isfinite(out["t"][~hor])) and np.all(out["t"] > 0.0)
    # disk_crossings=K: t_cross per layer, t the time to the end
    lay0 = gi.trace(k0, CAM, disk=DISK, disk_crossings=3, **kw)
    lay = gi.trace(k0, CAM, disk=DISK, disk_crossings=3, travel_time=True, **kw)
    assert set(lay) == set(lay0) | {"t", "t_cross"} and lay["t_cross"].shape == (3, 8, 12) and lay["t"].shape == (8, 12)
    for k in lay0:
        assert np.array_equal(lay[k], lay0[k], equal_nan=True), k
    assert np.array_equal(lay["t"], out["t"])
    have = np.arange(3)[:, None, None] < lay["n_cross"][None]
    assert np.array_equal(np.isnan(lay["t_cross"]), ~have)
    # the opaque disk: the first crossing's time on the rays it stops, the end's elsewhere
    op0 = gi.trace(k0, CAM, disk=DISK, **kw)
    op = gi.trace(k0, CAM, disk=DISK, travel_time=True, **kw)
    assert set(op) == set(op0) | {"t"}
    for k in op0:
        assert np.array_equal(op[k], op0[k]), k
    hit = op["flags"] == 128
    assert hit.sum() > 10 and np.array_equal(hit, lay["n_cross"] >= 1)
    assert np.array_equal(op["t"][hit], lay["t_cross"][0][hit]) and np.array_equal(op["t"][~hit], out["t"][~hit])
    with pytest.raises(ValueError, match="travel_time"):
        gi.trace(k0, CAM, spheres=[[5.0, 0.0, 0.0, 1.0]], travel_time=True, **kw)

"""Light travel time without a GPU: the ABI surface, the refusals (checked before the context, so the
library refuses them here too), the scipy restatement (tests/travel_time_reference.py) against closed forms and a converged solve
of the 7-component system, the conditions the golden vectors must keep, and the numpy restatement of the retarded layer shade on
hand-worked cases.

Measured when this was written: the radial ray 0 (bound 1e-12 relative; 1.3e-12 at max_step 2, which is why 0.5); the restatement
at rtol 1e-10 against DOP853 at 1e-12, worst relative distance 5.8e-11 over 26 Schwarzschild rays and 1.1e-10 over 29 Kerr rays at
a / M = 0.9 (bound 1e-9)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import crossings_reference as cr  # noqa: E402
import disk_layers_reference as dl  # noqa: E402
import travel_time_reference as tt  # noqa: E402


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


# ---- the ABI surface ----------------------------------------------------------------------------------------------------
NEW = ("bhg_travel_time_device", "bhg_travel_time", "bhg_shade_disk_layers_retarded_device")


def test_exports_and_header():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_TRAVEL_TIME\s+1\s*$", hdr, re.M)
    assert L.bhg_version() == 10 and f.ABI_VERSION == 10


# ---- the refusals, through a NULL context -----------------------------------------------------------------------------------
def _params(**kw):
    f, _ = _lib()
    base = dict(r_s=1.0, lambda_end=60.0, r_exit=35.0, disk_r_in=3.0, disk_r_out=12.0)
    base.update(kw)
    return f.make_params(**base)


def _device_rc(p, K, ptr=None, t_end=64):
    f, L = _lib()
    xs = (C.c_double * 3)(3.0, 0.0, 30.0)
    return L.bhg_travel_time_device(None, C.byref(p), xs, None, ptr, 16, K, ptr, None, None, None, ptr, ptr, t_end, ptr, None)


def _host_rc(p, K, ptr=None, t_end=64):
    f, L = _lib()
    xs = (C.c_double * 3)(3.0, 0.0, 30.0)
    return L.bhg_travel_time(None, C.byref(p), xs, 1, ptr, 16, K, ptr, None, None, None, ptr, ptr, t_end, ptr)


REFUSALS = [
    (dict(method=1), 3, 64, "DP5(4)"),
    (dict(time_like=1), 3, 64, "time_like"),
    (dict(), -1, 64, "max_crossings"),
    (dict(), 5, 64, "max_crossings"),
    (dict(disk_r_in=0.0, disk_r_out=0.0), 1, 64, "disk_r_out"),
    (dict(), 3, None, "t_end"),
    (dict(disk_r_in=0.0, disk_r_out=0.0), 0, None, "t_end"),
    (dict(rhs_form=2, spin=0.45, time_like=1), 0, 64, "time_like"),
]


@pytest.mark.parametrize("call", [_device_rc, _host_rc], ids=["device", "host"])
@pytest.mark.parametrize("kw,K,t_end,word", REFUSALS)
def test_refuses(call, kw, K, t_end, word):
    f, L = _lib()
    assert call(_params(**kw), K, t_end=t_end) == f.E_INVALID
    msg = L.bhg_last_error().decode()
    assert word in msg and "ctx" not in msg, msg


@pytest.mark.parametrize("call", [_device_rc, _host_rc], ids=["device", "host"])
@pytest.mark.parametrize("kw", [dict(), dict(rhs_form=1), dict(rhs_form=2, spin=0.45)], ids=["christoffel", "reduced", "kerr"])
def test_what_is_covered_reaches_the_context(call, kw):
    f, L = _lib()
    # (every array given -- an address nothing dereferences without a context -- so that the context is the one thing missing)
    for K, more in ((0, dict()), (0, dict(disk_r_in=0.0, disk_r_out=0.0)), (1, dict()), (4, dict())):
        assert call(_params(**kw, **more), K, ptr=64) == f.E_INVALID
        assert "ctx" in L.bhg_last_error().decode(), L.bhg_last_error().decode()


def _retarded_rc(phase_rate, t_cross=64, K=3, opacity=0.5, disk=(3.0, 12.0)):
    f, L = _lib()
    sc = f.make_scene(0, 4, 2, disk=disk)
    ly = f.make_disk_layers(K, opacity)
    return L.bhg_shade_disk_layers_retarded_device(None, None, None, None, None, None, 16, 1, C.byref(sc), None, None, None, None,
                                                   None, None, None, None, None, C.byref(ly), t_cross, phase_rate, None)


def test_retarded_shade_refuses_what_the_layered_shade_refuses():
    f, L = _lib()
    for kw, word in ((dict(K=0), "max_crossings"), (dict(opacity=0.0), "opacity"), (dict(disk=None), "disk")):
        assert _retarded_rc(0.05, **kw) == f.E_INVALID
        msg = L.bhg_last_error().decode()
        assert word in msg and "ctx" not in msg, msg
    assert _retarded_rc(float("nan")) == f.E_INVALID and "phase_rate" in L.bhg_last_error().decode()
    for rate, tc in ((0.05, 64), (0.0, 64), (0.05, None)):
        assert _retarded_rc(rate, tc) == f.E_INVALID and "ctx" in L.bhg_last_error().decode()


def test_python_surface():
    import inspect

    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    from blackhole_geodesic_calculator_amd.integrator import GeodesicIntegratorSchwarzschild
    for name in ("travel_time", "travel_time_device", "shade_disk_layers_retarded_device"):
        assert callable(getattr(_ffi.Context, name))
    assert inspect.signature(GeodesicIntegratorSchwarzschild.trace).parameters["travel_time"].default is False
    assert inspect.signature(DeviceFrame.set_disk_layers).parameters["phase_rate"].default == 0.0


# ---- the restatement against closed forms ----------------------------------------------------------------------------------
def test_quadrature_rule_is_leggauss_6():
    # the literals of the kernel, digit for digit
    src = open(os.path.join(ROOT, "blackhole_geodesic_calculator_amd", "csrc", "geodesic_kernels.hip")).read()
    for name, vals in (("GL6_X", tt.GL6_X), ("GL6_W", tt.GL6_W)):
        m = re.search(name + r"\[6\] = \{([^}]*)\}", src)
        got = [s.strip() for s in m.group(1).replace("\n", " ").split(",")]
        assert got == ["%.17g" % v for v in vals], (name, got)
        assert [float(s) for s in got] == list(vals)


@pytest.mark.parametrize("form", [0, 1], ids=["christoffel", "reduced"])
def test_radial_ray_closed_form(form):
    r = tt.solve([0.0, 0.0, 1.0], [0.0, 0.0, 3.0], form, r_exit=35.0, lambda_end=120.0, max_step=0.5)
    exact = 32.0 + np.log(34.0 / 2.0)
    assert exact == pytest.approx(tt.radial_time(3.0, 35.0))
    assert r["flags"] == tt.FLAG_EXITED_SPHERE
    rel = abs(r["t_end"] / exact - 1.0)
    print(f"radial ray, form {form}: {r['n_accepted']} steps, relative distance from 32 + ln 17 {rel:.1e}")
    assert rel <= 1e-12


def test_does_not_depend_on_the_length_of_k0():
    a = tt.solve([0.0, 0.0, 1.0], [0.0, 0.0, 3.0], 0, r_exit=35.0, lambda_end=120.0, max_step=0.5)
    b = tt.solve([0.0, 0.0, 2.5], [0.0, 0.0, 3.0], 0, r_exit=35.0, lambda_end=120.0, max_step=0.2)
    assert abs(b["t_end"] / a["t_end"] - 1.0) <= 1e-12


def test_flat_space():
    k0, lam = np.array([0.3, 0.2, 2.0]), 7.0
    r = tt.solve(k0, [1.0, 2.0, 3.0], 0, r_s=0.0, lambda_end=lam)
    assert r["flags"] == tt.FLAG_REACHED_END
    assert abs(r["t_end"] / (np.linalg.norm(k0) * lam) - 1.0) <= 1e-14


def test_special_values():
    inside = tt.solve([0.0, 0.0, 1.0], [0.0, 0.0, 0.5], 0)
    assert inside["flags"] == tt.FLAG_START_INSIDE | tt.FLAG_HIT_HORIZON and inside["t_end"] == np.inf
    # towards the hole through the disk: the crossing in front of the horizon ending stays finite
    cam = cr.inclined_camera(30.0, 60.0)
    r = tt.solve(-cam / 30.0 + np.array([0.0, 0.02, 0.0]), cam, 0, disk=(3.0, 12.0), r_exit=35.0)
    assert r["flags"] == tt.FLAG_HIT_HORIZON and r["t_end"] == np.inf


# (rays away from the critical impact parameter: within a few hundredths of it the trajectory itself, not the time integral, is
# what a 1e-10 solve and a 1e-12 solve disagree on -- one such ray measured 1.8e-8; horizon rays have t = inf in both)
@pytest.mark.parametrize("form,spin,n,lam,r_exit,at_least", [(0, 0.0, 40, 120.0, 35.0, 20), (2, 0.45, 40, 60.0, 0.0, 20)],
                         ids=["schwarzschild", "kerr"])
def test_restatement_against_the_seven_component_system(form, spin, n, lam, r_exit, at_least):
    cam = cr.inclined_camera(30.0, 70.0, 0.5 if form == 2 else 0.0)
    k = cr.camera_rays(cam, n, np.random.default_rng(1), critical=0.0)
    worst, count = 0.0, 0
    for ki in k:
        a = tt.solve(ki, cam, form, spin=spin, r_exit=r_exit, rtol=1e-10, atol=1e-12, lambda_end=lam)
        if a["flags"] & tt.FLAG_HIT_HORIZON:
            assert a["t_end"] == np.inf
            continue
        fl, tc = tt.solve_converged(ki, cam, form, spin=spin, r_exit=r_exit, lambda_end=lam)
        assert fl == a["flags"] and np.isfinite(tc) and np.isfinite(a["t_end"])
        worst, count = max(worst, abs(a["t_end"] / tc - 1.0)), count + 1
    print(f"form {form}: {count} rays, worst relative distance {worst:.1e}")
    assert count >= at_least and worst <= 1e-9


# ---- the golden vectors' conditions ------------------------------------------------------------------------------------------
SETS = ("schw_default", "kerr_default", "schw_nodisk", "kerr_nodisk", "schw_tight", "kerr_tight")


@pytest.mark.parametrize("name", SETS)
def test_golden_conditions(name):
    g = load_golden("travel_time")
    get = lambda k: g[f"{name}__{k}"]      # noqa: E731
    n_drawn, n_kept = int(get("n_drawn")), int(get("n_kept"))
    assert n_drawn <= 300 and n_kept == len(get("k0")) and n_drawn - n_kept <= 0.05 * n_drawn
    for f in range(len(get("forms"))):
        t_end, S_end, t_cross, S_cross, n_cross, flags = (get(k)[f] for k in ("t_end", "S_end", "t_cross", "S_cross", "n_cross", "flags"))
        hor = (flags & tt.FLAG_HIT_HORIZON) != 0
        assert np.all(np.isinf(t_end[hor])) and not np.isnan(t_end).any() and np.all(t_end > 0.0)
        assert np.array_equal(np.isfinite(S_end), np.isfinite(t_end)) and np.array_equal(np.isfinite(S_cross), np.isfinite(t_cross))
        have = np.arange(4)[:, None] < n_cross[None, :]
        assert np.array_equal(~np.isnan(t_cross), have)
        S = np.concatenate([S_end, S_cross.ravel()])
        assert get("floor")[f] == tt.COND * np.median(S[np.isfinite(S)]) > 0.0
        if "nodisk" in name:
            assert n_cross.max() == 0
        else:
            assert (n_cross >= 2).sum() >= (2 if "tight" in name else 5) and np.isfinite(t_cross[0, hor & (n_cross >= 1)]).all() and ("tight" in name or (hor & (n_cross >= 1)).any())
            # crossing times grow along the ray and do not exceed the end's
            fin = np.where(have, t_cross, np.nan)
            assert np.all(np.diff(fin, axis=0)[have[1:]] > 0.0)
            assert np.all(fin[have] <= np.broadcast_to(t_end, fin.shape)[have])
        assert np.isfinite(t_end).sum() >= 0.3 * n_kept


@pytest.mark.parametrize("name,form", [("schw_default", 0), ("schw_default", 1), ("kerr_default", 0)])
def test_opaque_disk_hits_exactly_where_the_golden_has_a_crossing(name, form):
    """On the golden's disk set the opaque-disk solve of oracle/scipy_reference ends with HIT_DISK exactly on the rays with a
    crossing: what trace(disk=, travel_time=True) relies on when it takes the first crossing's time for those rays."""
    from oracle import scipy_reference as sr
    g = load_golden("travel_time")
    get = lambda k: g[f"{name}__{k}"]      # noqa: E731
    k0, x0, n_cross = get("k0")[::3], get("x0")[::3], get("n_cross")[form][::3]
    disk = tuple(get("disk"))
    par = dict(lambda_end=float(get("lambda_end")), rtol=float(get("rtol")), atol=float(get("atol")), disk=disk)
    for ki, xi, nc in zip(k0, x0, n_cross):
        if name.startswith("kerr"):
            r = sr.trace_ray_kerr(ki, xi, M=0.5, a=float(get("spin")), **par)
        else:
            r = sr.trace_ray(ki, xi, form=tt.FORM_NAMES[form], r_exit=35.0, r_s=1.0, **par)
        assert (r["flags"] == tt.FLAG_HIT_DISK) == (nc >= 1)


# ---- the retarded layer shade on hand-worked cases ------------------------------------------------------------------------
def _tex():
    # a texture whose colour is its texture_x: column j of 8 holds j / 8 in red
    t = np.zeros((1, 8, 4), np.float32)
    t[0, :, 0] = np.arange(8) / 8.0
    t[0, :, 3] = 1.0
    return t


def test_retarded_colours_by_hand():
    from oracle import shade_reference as sh
    disk, profile = (3.0, 12.0), dict(phase=0.4, mean=0.3, stddev=0.25, intensity=2.0)
    e0 = np.array([6.0, 0.0, 0.0, 0.0, 0.0, -1.0])         # on the +x axis: acos(1) = 0, texture_x = phase / pi
    e1 = np.array([0.0, -5.0, 0.0, 0.0, 0.0, 1.0])         # on the -y axis
    cross = np.array([[e0, e0, e0], [e1, e1, e1]])         # [2 layers, 3 rays, 6]
    n_cross = np.array([2, 1, 2])
    t_cross = np.array([[10.0, 20.0, np.inf], [30.0, np.nan, 40.0]])
    rate = 0.05
    got = tt.retarded_layer_colours(cross, n_cross, t_cross, rate, 2, disk, disk_tex=_tex(), disk_profile=profile)
    for m, i, e in ((0, 0, e0), (0, 1, e0), (1, 0, e1), (1, 2, e1)):
        want = sh.disk_colour(e[None, :], disk[0], disk[1], _tex(), **dict(profile, phase=0.4 - rate * t_cross[m, i]))[0]
        assert np.array_equal(got[m, i], want)
    assert np.array_equal(got[0, 2], [0.0, 0.0, 0.0])      # a time that is not finite: black
    assert np.isnan(got[1, 1]).all()                       # a layer the ray does not have
    # rate 0 is the layered shade's own colour, and a rate changes it
    plain = dl.layer_colours(cross, n_cross, 2, disk, disk_tex=_tex(), disk_profile=profile)
    zero = tt.retarded_layer_colours(cross, n_cross, np.where(np.isfinite(t_cross), t_cross, 1.0), 0.0, 2, disk, disk_tex=_tex(),
                                     disk_profile=profile)
    assert np.array_equal(np.nan_to_num(zero), np.nan_to_num(plain))
    assert not np.array_equal(got[0, 0], plain[0, 0])
    # the black layer still absorbs: behind it the sky at T, not at 1
    sky = np.array([[0.5, 0.25, 1.0]] * 3)
    img = dl.composite(got, n_cross, 2, 0.5, sky, np.array([8, 8, 8], np.uint8), 3, 1)
    assert np.array_equal(img[2, :3], 0.5 * got[1, 2] + 0.25 * sky[2])
    assert np.array_equal(img[1, :3], got[0, 1] + 0.5 * sky[1])


def test_trace_refuses_spheres_with_travel_time():
    from blackhole_geodesic_calculator_amd.integrator import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild.__new__(GeodesicIntegratorSchwarzschild)     # (no context: refused before it is used)
    with pytest.raises(ValueError, match="travel_time"):
        gi.trace(np.array([[0.0, 0.0, -1.0]]), np.array([0.0, 0.0, 30.0]), spheres=[[5.0, 0.0, 0.0, 1.0]], travel_time=True)

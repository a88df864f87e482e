"""The thermal disk without a GPU: the numpy restatement (tests/disk_thermal_reference.py) against the
Page-Thorne integral by quadrature, the Schwarzschild closed form, the peak, the inner edge of section 9's family, the flat
limit, the bolometric identity of the spectrum, mirror symmetry, the ABI surface and every refusal of the library (checked
before the context, so no device is needed)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import disk_thermal_reference as dt  # noqa: E402
import redshift_reference as rr  # noqa: E402

R_S = 1.0
NU = (2.0e14, 5.0e14, 1.2e15)


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def _sense_of(astar):
    """(a/M, disk_sense) with a* = -disk_sense a / M (section 9's sense)."""
    return abs(astar), (-1 if astar > 0 else 1)


# ---- the flux shape -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("astar", [-0.998, -0.9, 0.0, 0.45, 0.9, 0.998])
def test_flux_shape_matches_the_page_thorne_integral(astar):
    M = 1.0
    a, sense = _sense_of(astar)
    K = dt.constants(astar)
    fmax, _ = dt.flux_max(K)
    r_peak, F_peak = dt.judge_peak(M, a * M, sense)
    r = np.linspace(1.001 * K["r_ms"], 200.0, 40)
    mine = dt.flux_hat(np.sqrt(r), K) / fmax
    judge = dt.page_thorne_judge(r, M, a * M, sense) / F_peak
    assert np.abs(mine - judge).max() <= 1e-7
    # the peak: tau = 1 at the judge's peak radius
    assert abs((dt.flux_hat(np.sqrt(r_peak), K) / fmax) ** 0.25 - 1.0) <= 1e-9


LADDER_E = tuple(10.0 ** -k for k in range(2, 13))     # r = r_ms (1 + e)


def _ladder(astar, flux):
    """Per rung e: (e, |tau - tau_mp|, relative flux error, sign of F^) of `flux` against mpmath at the same double x."""
    K = dt.constants(astar)
    fmax, _ = dt.flux_max(K)
    rows = []
    for e in LADDER_E:
        x = float(np.sqrt(K["r_ms"] * (1.0 + e)))
        assert x > K["x0"]
        F = float(flux(np.array([x]), K)[0])
        F_mp = dt.flux_hat_mp(x, K)
        t_mp = dt.tau_mp(x, K, fmax)
        tau = np.sqrt(np.sqrt(max(F, 0.0) * (1.0 / fmax)))
        rows.append((e, abs(float(tau - t_mp)), abs(float((F - F_mp) / F_mp)), F))
    return rows


@pytest.mark.parametrize("astar", [-0.998, -0.9, 0.0, 0.45, 0.9, 0.998])
def test_flux_next_to_the_inner_edge_against_mpmath(astar, record_property):
    """The ladder r = r_ms (1 + e), e = 1e-2 ... 1e-12: flux_hat (the library's order of operations) against the closed form in
    mpmath at 300 bits from the same double constants and the same double x = sqrt(r).  |tau - tau_mp| <= 1e-9 on the whole
    ladder, the relative flux error <= 1e-8 for e >= 1e-7, and F^ > 0 on every rung."""
    rows = _ladder(astar, dt.flux_hat)
    record_property("max_tau_error", max(r[1] for r in rows))
    record_property("max_rel_flux_error_e_ge_1e-7", max(r[2] for r in rows if r[0] >= 0.99e-7))
    for e, dtau, rel, F in rows:
        print(f"a* = {astar:+.3f}  e = {e:.0e}  |dtau| = {dtau:.3e}  rel F = {rel:.3e}  F = {F:.3e}")
    for e, dtau, rel, F in rows:
        assert F > 0.0, (astar, e, F)
        assert dtau <= 1e-9, (astar, e, dtau)
        if e >= 0.99e-7:
            assert rel <= 1e-8, (astar, e, rel)


def test_the_ladder_catches_the_logarithm_of_a_rounded_quotient():
    """The form the library had -- log(x / x0), log((x - x_i) / (x0 - x_i)) -- misses the ladder's bounds: the test above can fail."""
    rows = _ladder(0.0, dt.flux_hat_parent) + _ladder(0.9, dt.flux_hat_parent)
    assert max(r[1] for r in rows) > 1e-9
    assert max(r[2] for r in rows if r[0] >= 0.99e-7) > 1e-8


def test_schwarzschild_closed_form_and_peak():
    K = dt.constants(0.0)
    assert list(K["xr"]) == [np.sqrt(3.0), 0.0, -np.sqrt(3.0)] and K["c"][1] == 0.0 and K["r_ms"] == 6.0
    fmax, x_peak = dt.flux_max(K)
    x = np.sqrt(np.linspace(6.0 + 1e-6, 400.0, 200))
    assert np.abs(dt.flux_hat(x, K) - dt.schwarzschild_flux_hat(x)).max() <= 1e-13 * fmax
    assert abs(x_peak ** 2 - 9.551) < 1e-3
    r_peak, _ = dt.judge_peak(1.0, 0.0, 1)
    assert abs(r_peak - 9.551) < 1e-3


@pytest.mark.parametrize("kerr,aM", [(False, 0.0), (True, 0.45), (True, 0.9), (True, 0.998)])
@pytest.mark.parametrize("sense", [1, -1])
def test_inner_edge_is_the_minimum_of_the_energy_of_section_9s_orbit(kerr, aM, sense):
    """r_ms equals the minimum of -u_t of redshift_reference's disk orbit (u^t, Omega): the same family, the same sense."""
    M = 0.5 * R_S
    _, _, astar, K, _ = dt.family(R_S, aM * M, kerr, sense)
    assert abs(dt.judge_isco(M, aM * M, sense) / (K["r_ms"] * M) - 1.0) <= 1e-12
    assert astar == -sense * aM


def test_flat_limit_temperature_goes_as_r_to_the_minus_three_quarters():
    r_s = 1e-8
    r = np.geomspace(1e4, 1e6, 25)
    end = np.zeros((len(r), 6))
    end[:, 0] = r * np.cos(0.3)
    end[:, 1] = r * np.sin(0.3)
    flags = np.full(len(r), 128, np.uint8)
    t, rgb = dt.thermal_rays(end, flags, np.ones(len(r)), r_s, t_peak=1e7, nu=NU, weights=np.eye(3))
    q = t * r ** 0.75
    assert np.all(t > 0.0) and np.abs(q / q[0] - 1.0).max() <= 1e-6


def test_spectrum_reproduces_the_bolometric_identity():
    """A 16-point Gauss-Laguerre table weighs the observed blackbody to (pi^4 / 15) (g tau)^4 (f_col cancels)."""
    xs, ws = np.polynomial.laguerre.laggauss(16)
    end = np.zeros((3, 6))
    end[:, 0] = [7.0, 11.0, 25.0]
    flags = np.full(3, 128, np.uint8)
    g = np.array([0.83, 1.12, 0.97])
    t_peak, f_col = 2.0e4, 1.7
    t0, _ = dt.thermal_rays(end, flags, g, R_S, t_peak=t_peak, nu=NU, weights=np.eye(3), f_col=f_col)
    for i in range(3):
        y = g[i] * f_col * t0[i] / t_peak             # the observed temperature in units of t_peak
        nu = xs * y * t_peak / dt.H_OVER_K            # the nodes at that temperature, in Hz
        w = ws * np.exp(xs) * y                       # dnu-hat weights of int_0^inf
        _, rgb = dt.thermal_rays(end[i:i + 1], flags[:1], g[i:i + 1], R_S, t_peak=t_peak, nu=nu, weights=np.tile(w, (3, 1)),
                                 f_col=f_col)
        want = np.pi ** 4 / 15.0 * (g[i] * t0[i] / t_peak) ** 4
        assert np.abs(rgb[0] / want - 1.0).max() <= 1e-9


@pytest.mark.parametrize("kerr,aM", [(False, 0.0), (True, 0.9)])
def test_mirror_symmetry(kerr, aM):
    """x -> -x with disk_sense and the spin reversed gives the same T_em and rgb (and the same g)."""
    rng = np.random.default_rng(3)
    M = 0.5 * R_S
    xc = np.array([6.0, -18.0, 11.0])
    n = 60
    R = rng.uniform(2.5, 12.0, n)
    ph = rng.uniform(0.0, 2.0 * np.pi, n)
    end = np.zeros((n, 6))
    end[:, 0], end[:, 1] = R * np.cos(ph), R * np.sin(ph)
    k0 = (end[:, 0:3] - xc) / np.linalg.norm(end[:, 0:3] - xc, axis=1)[:, None]
    flags = np.full(n, 128, np.uint8)
    mir = np.array([-1.0, 1.0, 1.0])
    out = []
    for s, sign in ((1, 1.0), (-1, -1.0)):
        m = mir if sign < 0 else np.ones(3)
        e2 = end.copy()
        e2[:, 0:3] *= m
        g = rr.g_rays(xc * m, k0 * m, e2, flags, R_S, sign * aM * M, kerr, s)
        out.append((g,) + dt.thermal_rays(e2, flags, g, R_S, sign * aM * M, kerr, s, 1.5e4, NU, np.eye(3), 1.3, 2.0))
    for a, b in zip(out[0], out[1]):
        assert np.allclose(a, b, rtol=1e-11, atol=0.0)
    assert np.any(out[0][1] > 0.0)


def test_classes():
    end = np.zeros((6, 6))
    end[:, 0] = [8.0, 4.0, 8.0, 8.0, 8.0, 8.0]     # (4.0 < r_ms = 6M at r_s = 2: inside, an exact zero)
    flags = np.array([128, 128, 1, 0x88, 64, 8], np.uint8)
    t, rgb = dt.thermal_rays(end, flags, np.ones(6), 2.0, nu=NU, weights=np.eye(3))
    assert t[0] > 0.0 and np.all(rgb[0] > 0.0)
    assert t[1] == 0.0 and np.all(rgb[1] == 0.0)
    assert np.all(t[[2, 3, 5]] == 0.0) and np.all(rgb[[2, 3, 5]] == 0.0)
    assert np.isnan(t[4]) and np.all(np.isnan(rgb[4]))
    t, rgb = dt.thermal_rays(None, flags, np.ones(6), 2.0, nu=NU, weights=np.eye(3))
    assert np.all(np.isnan(t[:2])) and np.all(t[[2, 3, 5]] == 0.0)


# ---- the ABI surface -------------------------------------------------------------------------------------------------
SYMS = ("bhg_disk_thermal_size", "bhg_disk_thermal_device", "bhg_disk_thermal_host", "bhg_shade_scene_thermal_device",
        "bhg_frame_set_disk_thermal")


def test_exports_and_struct_size():
    f, L = _lib()
    assert L.bhg_disk_thermal_size() == C.sizeof(f.DiskThermal) == 544
    assert L.bhg_version() == f.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for sym in SYMS:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in f.EXPORTS
        getattr(L, sym)
    assert "#define BHG_DISK_THERMAL 1" in header and "#define BHG_THERMAL_NU_MAX 16" in header


def test_header_struct_compiles_as_c99_and_cxx(tmp_path):
    f, _ = _lib()
    src = tmp_path / "th.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bhgeo.h"\n'
                   'int main(void) { bhg_disk_thermal t = {0}; t.weight[2][BHG_THERMAL_NU_MAX - 1] = 1.0;\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(t), offsetof(bhg_disk_thermal, n_nu),\n'
                   '         offsetof(bhg_disk_thermal, t_peak), offsetof(bhg_disk_thermal, f_col), offsetof(bhg_disk_thermal, scale),\n'
                   '         offsetof(bhg_disk_thermal, nu), offsetof(bhg_disk_thermal, weight), BHG_DISK_THERMAL,\n'
                   '         BHG_THERMAL_NU_MAX); return 0; }\n')
    exe = tmp_path / "th"
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-x", "c++", "-fsyntax-only", str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    T = f.DiskThermal
    assert out == [C.sizeof(T), T.n_nu.offset, T.t_peak.offset, T.f_col.offset, T.scale.offset, T.nu.offset, T.weight.offset, 1, 16]
    assert out[:7] == [544, 4, 8, 16, 24, 32, 160]


def test_make_disk_thermal_and_narrowband():
    f, _ = _lib()
    th = f.make_disk_thermal(1.2e4, *f.narrowband(4e14, 5.5e14, 7e14), f_col=1.7, scale=3.0, disk_sense=-1)
    assert (th.disk_sense, th.n_nu, th.t_peak, th.f_col, th.scale) == (-1, 3, 1.2e4, 1.7, 3.0)
    assert list(th.nu[:3]) == [4e14, 5.5e14, 7e14]
    assert [list(th.weight[c][:3]) for c in range(3)] == np.eye(3).tolist()
    with pytest.raises(ValueError):
        f.make_disk_thermal(1e4, np.ones(17) * 1e14, np.ones((3, 17)))
    with pytest.raises(ValueError):
        f.make_disk_thermal(1e4, (1e14, 2e14), np.ones((3, 3)))


# ---- the refusals (before the context) -------------------------------------------------------------------------------
def _params(rhs=0, spin=0.0, time_like=0, disk=None):
    f, _ = _lib()
    kw = {} if disk is None else dict(disk_r_in=disk[0], disk_r_out=disk[1])
    return f.make_params(r_s=R_S, rhs_form=rhs, spin=spin, time_like=time_like, **kw)


def _th(**kw):
    f, _ = _lib()
    th = f.make_disk_thermal(1e4, *f.narrowband(*NU), disk_sense=kw.pop("disk_sense", 1))
    for k, v in kw.items():
        if k == "nu1":
            th.nu[1] = v
        elif k == "w21":
            th.weight[2][1] = v
        else:
            setattr(th, k, v)
    return th


def _host_rc(p, th, x0, obs=None):
    f, L = _lib()
    xs = (C.c_double * 3)(*x0)
    k0 = (C.c_double * 3)(0.0, 0.0, -1.0)
    fl = (C.c_uint8 * 1)(128)
    t = (C.c_double * 1)()
    rgb = (C.c_double * 3)()
    return L.bhg_disk_thermal_host(None, C.byref(p), C.byref(th), None if obs is None else C.byref(obs), xs, 1, k0, None, fl, 1, t,
                                   rgb)


def _device_rc(p, th, x0, obs=None):
    f, L = _lib()
    xs = (C.c_double * 3)(*x0)
    return L.bhg_disk_thermal_device(None, C.byref(p), C.byref(th), None if obs is None else C.byref(obs), xs, None, None, None,
                                     None, 16, None, None, None)


def _shade_rc(p, th, x0, obs=None, rs=None, pol=None, disk=(3.0, 10.0)):
    f, L = _lib()
    sc = f.make_scene(0, 4, 2, disk=disk)
    xs = (C.c_double * 3)(*x0)
    return L.bhg_shade_scene_thermal_device(None, None, None, None, None, 16, 1, C.byref(sc), C.byref(p),
                                            None if rs is None else C.byref(rs), None if obs is None else C.byref(obs), None, xs,
                                            None, None, None, None, None if pol is None else C.byref(pol), None, C.byref(th), None)


REFUSALS = [
    (dict(), dict(disk_sense=0), (3.0, 0.0, 20.0), "disk_sense"),
    (dict(), dict(disk_sense=2), (3.0, 0.0, 20.0), "disk_sense"),
    (dict(), dict(n_nu=0), (3.0, 0.0, 20.0), "n_nu"),
    (dict(), dict(n_nu=17), (3.0, 0.0, 20.0), "n_nu"),
    (dict(), dict(nu1=0.0), (3.0, 0.0, 20.0), "nu[1]"),
    (dict(), dict(nu1=-1e14), (3.0, 0.0, 20.0), "nu[1]"),
    (dict(), dict(nu1=np.inf), (3.0, 0.0, 20.0), "nu[1]"),
    (dict(), dict(w21=np.nan), (3.0, 0.0, 20.0), "weight[2][1]"),
    (dict(), dict(t_peak=0.0), (3.0, 0.0, 20.0), "t_peak"),
    (dict(), dict(t_peak=np.nan), (3.0, 0.0, 20.0), "t_peak"),
    (dict(), dict(f_col=-1.0), (3.0, 0.0, 20.0), "f_col"),
    (dict(), dict(f_col=np.inf), (3.0, 0.0, 20.0), "f_col"),
    (dict(), dict(scale=np.nan), (3.0, 0.0, 20.0), "scale"),
    (dict(time_like=1), dict(), (3.0, 0.0, 20.0), "time_like"),
    (dict(disk=(1.4, 10.0)), dict(), (3.0, 0.0, 20.0), "photon"),
    (dict(), dict(), (0.5, 0.0, 0.5), "horizon r_s"),
    (dict(rhs=2, spin=0.45), dict(), (0.0, 0.0, 20.0), "axis"),
    (dict(rhs=2, spin=0.45), dict(), (0.9, 0.0, 0.0), "ergosurface"),
    (dict(rhs=2, spin=0.45), dict(), (0.5, 0.0, 0.1), "horizon r_+"),
]


@pytest.mark.parametrize("call", [_host_rc, _device_rc], ids=["host", "device"])
@pytest.mark.parametrize("pkw,thkw,x0,word", REFUSALS)
def test_library_refuses(call, pkw, thkw, x0, word):
    f, L = _lib()
    assert call(_params(**pkw), _th(**thkw), x0) == f.E_INVALID
    msg = L.bhg_last_error().decode()
    assert word in msg and "ctx" not in msg, msg


@pytest.mark.parametrize("pkw,thkw,x0,word", [r for r in REFUSALS if r[3] != "photon"])
def test_shade_refuses(pkw, thkw, x0, word):
    f, L = _lib()
    assert _shade_rc(_params(**pkw), _th(**thkw), x0, disk=(3.0, 10.0)) == f.E_INVALID
    msg = L.bhg_last_error().decode()
    assert word in msg and "ctx" not in msg, msg


def test_shade_refuses_the_disk_and_sense_mismatches():
    f, L = _lib()
    assert _shade_rc(_params(), _th(), (3.0, 0.0, 20.0), disk=(1.4, 10.0)) == f.E_INVALID
    assert "photon" in L.bhg_last_error().decode()
    assert _shade_rc(_params(), _th(disk_sense=1), (3.0, 0.0, 20.0), rs=f.make_redshift(disk_sense=-1)) == f.E_INVALID
    assert "differs from the redshift" in L.bhg_last_error().decode()
    assert _shade_rc(_params(), _th(disk_sense=1), (3.0, 0.0, 20.0), pol=f.make_polarisation(0.1, -1)) == f.E_INVALID
    assert "differs from the polarisation" in L.bhg_last_error().decode()
    # the same settings with nothing wrong get as far as the missing context
    assert _shade_rc(_params(), _th(), (3.0, 0.0, 20.0), rs=f.make_redshift(disk_sense=1)) == f.E_INVALID
    assert "ctx" in L.bhg_last_error().decode()
    assert _host_rc(_params(rhs=2, spin=0.45), _th(), (1e-9, 0.0, 20.0), obs=f.make_observer((0.1, 0.0, 0.0))) == f.E_INVALID
    assert "ctx" in L.bhg_last_error().decode()


def test_frame_setter_refuses_without_a_device():
    f, L = _lib()
    assert L.bhg_frame_set_disk_thermal(None, C.byref(_th())) == f.E_INVALID
    assert "frame" in L.bhg_last_error().decode()

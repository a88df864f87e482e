"""The observer camera (ABI 10) without a GPU: the numpy restatement (tests/observer_reference.py) against the metric, the
closed forms of aberration, Doppler factor and impact parameter, kerr_cart_to_bl's Killing constants; the library's refusals
(they are checked before the context) and its exports."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import observer_reference as orf  # noqa: E402
import redshift_reference as rr  # noqa: E402

R_S = 2.0
M = 1.0
CAMS = [np.array([7.0, 3.0, 4.0]), np.array([0.3, -12.0, 2.5]), np.array([10.0, 0.0, 0.0]), np.array([1e-3, 2e-3, 15.0])]


def _dirs(n, seed=0):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _metric4(x, q, spin, kerr):
    if kerr:
        return orf.kerr_metric4(q, M, spin)
    gtt, gij = orf.schw_metric(x, R_S)
    g = np.zeros((4, 4))
    g[0, 0], g[1:, 1:] = gtt, gij
    return g


@pytest.mark.parametrize("kerr,spin", [(False, 0.0), (True, 0.9), (True, -0.5)])
def test_restated_k_is_null_and_projects_back(kerr, spin):
    for x in CAMS:
        for n in _dirs(20, 1):
            k4, q = orf.zamo_k4(x, n, R_S, spin, kerr)
            g = _metric4(x, q, spin, kerr)
            assert abs(k4 @ g @ k4) <= 1e-13 * (k4[0] ** 2 * abs(g[0, 0]))
            back = orf.n_of_k0(x, orf.k0_of_n(x, n, R_S, spin, kerr), R_S, spin, kerr)
            assert np.max(np.abs(back - n)) <= 1e-13


def test_schwarzschild_impact_parameter_is_r_sin_alpha_over_sqrt_f():
    for x in CAMS:
        r = np.linalg.norm(x)
        f = 1.0 - R_S / r
        rh = x / r
        for n in _dirs(20, 2):
            k0 = orf.k0_of_n(x, n, R_S)
            # Killing constants of the Cartesian form: E = f k^t, L = |x cross k| (the total angular momentum), b = L / E
            gtt, gij = orf.schw_metric(x, R_S)
            kt = np.sqrt(k0 @ gij @ k0 / f)
            b = np.linalg.norm(np.cross(x, k0)) / (f * kt)
            sin_alpha = np.linalg.norm(np.cross(rh, n))
            assert abs(b - r * sin_alpha / np.sqrt(f)) <= 1e-13 * r


def test_kerr_at_zero_spin_is_schwarzschild():
    # (not the near-axis camera: there theta = arccos(z / r) carries eps / sin^2 th of relative error)
    for x in CAMS[:3]:
        for n in _dirs(20, 3):
            a = orf.k0_of_n(x, n, R_S, 0.0, True)
            b = orf.k0_of_n(x, n, R_S, 0.0, False)
            assert np.max(np.abs(a - b)) <= 1e-14


def _numpy_kerr_cart_to_bl(x, k, a, mu2=0.0):
    """kerr_cart_to_bl (csrc/kerr_start.h) restated: BL position and velocity in closed form, E, L from the null condition."""
    r_ = np.sqrt(0.5 * ((x @ x - a * a) + np.sqrt((x @ x - a * a) ** 2 + 4 * a * a * x[2] ** 2)))
    c = x[2] / r_
    th = 2.0 * np.arctan2(np.sqrt(1.0 - c), np.sqrt(1.0 + c))
    st, ct = np.sin(th), np.cos(th)
    R = np.sqrt(r_ * r_ + a * a)
    w = np.hypot(x[0], x[1])
    cp, sp = x[0] / w, x[1] / w
    D = (r_ * st) ** 2 + (R * ct) ** 2
    krho = cp * k[0] + sp * k[1]
    u = np.array([(r_ * st * krho + R * ct * k[2]) * R / D, (R * ct * krho - r_ * st * k[2]) / D,
                  (cp * k[1] - sp * k[0]) / (R * st)])
    gtt, gtp, grr, gthth, gpp = rr.kerr_metric(r_, th, M, a)
    S = grr * u[0] ** 2 + gthth * u[1] ** 2 + gpp * u[2] ** 2 + mu2
    B = gtp * u[2]
    kt = (-B - np.sqrt(B * B - gtt * S)) / gtt
    return -(gtt * kt + gtp * u[2]), gtp * kt + gpp * u[2]


@pytest.mark.parametrize("spin", [0.9, -0.6])
def test_kerr_cart_to_bl_gives_the_tetrads_E_and_L(spin):
    for x in CAMS:
        for n in _dirs(10, 4):
            k4, q = orf.zamo_k4(x, n, R_S, spin, True)
            g = orf.kerr_metric4(q, M, spin)
            E_t, L_t = -(g[0] @ k4), g[3] @ k4
            k0 = orf.k0_of_n(x, n, R_S, spin, True)
            E, L = _numpy_kerr_cart_to_bl(x, k0, spin)
            # the same ray up to the common scale of k0's normalisation
            assert abs(L / E - L_t / E_t) <= 1e-10 * max(1.0, abs(L_t / E_t))


def test_aberration_closed_form_and_headlight():
    for beta_mag in (0.1, 0.5, 0.9, 0.999):
        bh = np.array([0.2, -0.4, 0.8])
        bh /= np.linalg.norm(bh)
        beta = beta_mag * bh
        for n_p in _dirs(30, 5):
            n = orf.aberrate(n_p, beta)
            assert abs(np.linalg.norm(n) - 1.0) <= 1e-13
            ct_p, ct = n_p @ bh, n @ bh
            assert abs(ct - (ct_p - beta_mag) / (1.0 - beta_mag * ct_p)) <= 1e-12
        # perpendicular to beta in the rest frame -> n.beta_hat = -beta (the headlight effect)
        perp = np.cross(bh, [1.0, 0.0, 0.0])
        perp /= np.linalg.norm(perp)
        assert abs(orf.aberrate(perp, beta) @ bh + beta_mag) <= 1e-13
    n_p = _dirs(1, 6)[0]
    assert np.array_equal(orf.aberrate(n_p, np.zeros(3)), n_p)


def test_doppler_along_beta():
    for b in (0.1, 0.5, 0.9):
        beta = np.array([0.0, b, 0.0])
        # looking along beta (rest frame and ZAMO frame agree there): the blueshift sqrt((1 + b) / (1 - b))
        n = orf.aberrate(np.array([0.0, 1.0, 0.0]), beta)
        assert abs(orf.doppler(beta, n) - np.sqrt((1 + b) / (1 - b))) <= 1e-13
        n = orf.aberrate(np.array([0.0, -1.0, 0.0]), beta)
        assert abs(orf.doppler(beta, n) - np.sqrt((1 - b) / (1 + b))) <= 1e-13
        # gamma (1 + beta.n) = 1 / (gamma (1 - beta.n')) for every direction
        for n_p in _dirs(10, 7):
            assert abs(orf.doppler(beta, orf.aberrate(n_p, beta)) * orf.gamma_of(beta) * (1 - beta @ n_p) - 1.0) <= 1e-13


def test_observer_helpers():
    from blackhole_geodesic_calculator_amd import circular_orbit_velocity, radial_infall_velocity
    b = circular_orbit_velocity([6.0, 0.0, 0.0], R_S)
    assert np.allclose(b, [0.0, 0.5, 0.0], atol=1e-15)
    b = circular_orbit_velocity([0.0, 10.0, 0.0], R_S, sense=-1)
    assert np.allclose(b, [np.sqrt(1.0 / 8.0), 0.0, 0.0], atol=1e-15)
    assert np.allclose(radial_infall_velocity([0.0, 0.0, 8.0], R_S), [0.0, 0.0, -0.5], atol=1e-15)
    # Kerr at a = 0 is Schwarzschild; prograde is slower than retrograde relative to the ZAMO
    assert np.allclose(circular_orbit_velocity([8.0, 0.0, 0.0], R_S, 0.0), circular_orbit_velocity([8.0, 0.0, 0.0], R_S))
    pro = circular_orbit_velocity([8.0, 0.0, 0.0], R_S, 0.9, 1)
    retro = circular_orbit_velocity([8.0, 0.0, 0.0], R_S, 0.9, -1)
    assert pro[1] > 0 > retro[1] and abs(pro[1]) < abs(retro[1])
    # the orbit's velocity from the tetrad: u = gamma (e_t + v e_ph) has u^ph / u^t = Omega
    a, x = 0.9, np.array([8.0, 0.0, 0.0])
    et, legs, q = orf.kerr_tetrad(x, M, a)
    u = et + pro[1] * legs[2]
    r = q[0]
    assert abs(u[3] / u[0] - np.sqrt(M) / (r ** 1.5 + a * np.sqrt(M))) <= 1e-14
    with pytest.raises(ValueError):
        circular_orbit_velocity([2.5, 0.0, 0.0], R_S)    # inside the photon orbit
    with pytest.raises(ValueError):
        circular_orbit_velocity([6.0, 0.0, 1.0], R_S)


# ---- the library: refusals (before the context) and exports ------------------------------------------------------------
def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def _params(rhs=0, spin=0.0, time_like=0):
    f, _ = _lib()
    return f.make_params(r_s=R_S, rhs_form=rhs, spin=spin, time_like=time_like)


def _raygen_rc(p, beta, x0):
    f, L = _lib()
    obs = f.make_observer(beta)
    xs = (C.c_double * 3)(*x0)
    return L.bhg_raygen_observer_device(None, C.byref(p), C.byref(obs), xs, 4, 4, 1, 1.0, 1.0, None, None, None, 16, None, None)


def _redshift_rc(p, beta, x0):
    f, L = _lib()
    rs = f.make_redshift(("sky",))
    xs = (C.c_double * 3)(*x0)
    return L.bhg_redshift_observer_device(None, C.byref(p), C.byref(rs), C.byref(f.make_observer(beta)), xs, None, None, None, None, 4,
                                          None, None)


@pytest.mark.parametrize("call", [_raygen_rc, _redshift_rc])
def test_refusals(call):
    f, L = _lib()
    cases = [
        (_params(), [0.6, 0.8, 0.0], [0, 0, 10.0], "|beta|"),
        (_params(), [1.2, 0.0, 0.0], [0, 0, 10.0], "|beta|"),
        (_params(), [np.nan, 0.0, 0.0], [0, 0, 10.0], "not finite"),
        (_params(), [0.0, 0.0, np.inf], [0, 0, 10.0], "not finite"),
        (_params(), [0.1, 0.0, 0.0], [0, 0, 2.0], "horizon r_s"),
        (_params(rhs=1), [0.1, 0.0, 0.0], [1.0, 1.0, 1.0], "horizon r_s"),
        (_params(rhs=2, spin=0.9), [0.1, 0.0, 0.0], [1.3, 0.0, 0.0], "horizon r_+"),
        (_params(rhs=2, spin=0.9), [0.1, 0.0, 0.0], [0.0, 0.0, 10.0], "axis"),
        (_params(rhs=2, spin=0.9), [0.0, 0.0, 0.0], [2.0, 0.0, 0.0], "ergosurface"),    # BL r 1.786: outside r_+, inside r_E = 2
        (_params(rhs=2, spin=0.9), [0.0, 0.3, 0.0], [1.5, 1.0, 0.4], "ergosurface"),
    ]
    if call is _raygen_rc:
        cases.append((_params(time_like=1), [0.1, 0.0, 0.0], [0, 0, 10.0], "time_like"))
    for p, beta, x0, word in cases:
        # the restatement refuses the same settings
        with pytest.raises(ValueError):
            orf.check(np.array(x0, float), beta, R_S, p.spin, p.rhs_form == 2, p.time_like)
        assert call(p, beta, x0) == f.E_INVALID, (beta, x0)
        assert word in L.bhg_last_error().decode(), (word, L.bhg_last_error().decode())
    # near the axis is allowed (the refusal is for the axis itself): the call gets as far as the missing context
    assert _raygen_rc(_params(rhs=2, spin=0.9), [0.1, 0.0, 0.0], [1e-9, 0.0, 10.0]) == f.E_INVALID
    assert "ctx" in L.bhg_last_error().decode()


def test_exports_and_struct_size():
    f, L = _lib()
    assert L.bhg_observer_size() == C.sizeof(f.Observer) == 24
    assert L.bhg_version() == f.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for sym in ("bhg_observer_size", "bhg_raygen_observer_device", "bhg_redshift_observer_device", "bhg_redshift_observer_host",
                "bhg_shade_scene_redshift_observer_device", "bhg_frame_set_observer"):
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in f.EXPORTS
        getattr(L, sym)
    assert "typedef struct bhg_observer" in header


def _kerr_kt_agrees(x0, spin, n_dirs, seed):
    """For how many look directions does the start conversion's root of the null condition (rr.kerr_kt on the produced k0)
    give the tetrad's own k^t, up to k0's common scale?"""
    ok = 0
    for n in _dirs(n_dirs, seed):
        k4, q = orf.zamo_k4(x0, n, R_S, spin, True)
        k0 = orf.k0_of_n(x0, n, R_S, spin, True)
        q2, u = rr.kerr_bl_state(x0, k0, spin)
        kt = rr.kerr_kt(q2, u, M, spin)
        scale = u[0] / k4[1] if abs(k4[1]) > abs(k4[3]) else u[2] / k4[3]
        ok += abs(kt / (k4[0] * scale) - 1.0) <= 1e-10
    return ok


def test_outside_the_ergosurface_the_trace_root_is_the_tetrads():
    """Why the ergoregion is refused: there g_tt > 0 and the start conversion's fixed root is often not the tetrad's future
    root (the trace would follow another photon); outside the ergosurface it always is."""
    a = 0.9
    for x0 in (np.array([2.2, 0.0, 0.0]), np.array([1.2, 1.0, 1.3]), np.array([7.0, 3.0, 4.0])):
        r, th = orf.kerr_position(x0, a)[:2]
        assert r > M + np.sqrt(M * M - a * a * np.cos(th) ** 2)
        assert _kerr_kt_agrees(x0, a, 500, 11) == 500
    x_in = np.array([2.0, 0.0, 0.0])                   # inside the ergoregion (the refusal above)
    assert _kerr_kt_agrees(x_in, a, 500, 11) < 500

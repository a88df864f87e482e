"""Redshift (ABI 9) without a GPU: the numpy restatement (tests/redshift_reference.py) against an independent contraction
g_mu nu k^mu u^nu at the END states of the committed scipy goldens, its closed forms and symmetries, and every refusal --
the restatement's and the library's (checked before the context, so no device is needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import redshift_reference as rr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ---- the independent check: contract k with the emitter's 4-velocity at the end state ---------------------------------
def _schw_k_dot_u(x, k, r_s, u):
    """g_mu nu k^mu u^nu of the Christoffel form's metric (g_tt = -f, g_ij = delta_ij + h n_i n_j), k^t from g(k, k) = 0."""
    r = np.linalg.norm(x)
    f, h, n = 1.0 - r_s / r, r_s / (r - r_s), x / r
    kt = np.sqrt((k @ k + h * (n @ k) ** 2) / f)
    return -f * kt * u[0] + k @ u[1:] + h * (n @ k) * (n @ u[1:])


def _schw_g_at_end(x0, k0, end, fl, r_s, sense):
    rc = np.linalg.norm(x0)
    u_obs = np.array([1.0 / np.sqrt(1.0 - r_s / rc), 0.0, 0.0, 0.0])
    num = _schw_k_dot_u(x0, k0, r_s, u_obs)
    x, k = end[0:3], end[3:6]
    r = np.linalg.norm(x)
    f, h = 1.0 - r_s / r, r_s / (r - r_s)
    if fl == 128:
        R, M = np.hypot(x[0], x[1]), 0.5 * r_s
        Om = sense * np.sqrt(M) / R ** 1.5
        v = np.array([-Om * x[1], Om * x[0], 0.0])
        n = x / r
        ut = 1.0 / np.sqrt(f - v @ v - h * (n @ v) ** 2)    # normalisation, not the closed form
        u = np.concatenate([[ut], ut * v])
    else:
        u = np.array([1.0 / np.sqrt(f), 0.0, 0.0, 0.0])
    return num / _schw_k_dot_u(x, k, r_s, u)


def _kerr_k_dot_u(x, k, M, a, u):
    """u = (u^t, u^phi) (no r, theta motion) contracted with k in Boyer-Lindquist coordinates."""
    q, w = rr.kerr_bl_state(x, k, a)
    kt = rr.kerr_kt(q, w, M, a)
    gtt, gtp, _, _, gpp = rr.kerr_metric(q[0], q[1], M, a)
    return gtt * kt * u[0] + gtp * (kt * u[1] + w[2] * u[0]) + gpp * w[2] * u[1], q


def _kerr_g_at_end(x0, k0, end, fl, M, a, sense):
    qc, _ = rr.kerr_bl_state(x0, k0, a)
    al, om = rr.kerr_zamo(qc[0], qc[1], M, a)
    num, _ = _kerr_k_dot_u(x0, k0, M, a, (1.0 / al, om / al))
    x, k = end[0:3], end[3:6]
    qh, _ = rr.kerr_bl_state(x, k, a)
    if fl == 128:
        r, s = qh[0], float(sense)
        Om = s * np.sqrt(M) / (r ** 1.5 + s * a * np.sqrt(M))
        gtt, gtp, _, _, gpp = rr.kerr_metric(r, qh[1], M, a)
        ut = 1.0 / np.sqrt(-(gtt + 2.0 * gtp * Om + gpp * Om * Om))   # normalisation
        u = (ut, ut * Om)
    else:
        alh, omh = rr.kerr_zamo(qh[0], qh[1], M, a)
        u = (1.0 / alh, omh / alh)
    den, _ = _kerr_k_dot_u(x, k, M, a, u)
    return num / den


# Measured on these goldens (scipy RK45, rtol 1e-3): the relative difference between the camera-constant g and the end-state
# contraction, (largest, median) over the disk / object rays of both senses.  It is the integrator's drift: on the disk golden
# (max_step unset) E = f k^t itself drifts by up to 1.8 % (median 5.5e-4) between camera and disk; the object goldens take
# max_step 0.25 / 0.5 and drift far less.  Asserted at about 3x.
DRIFT = {"disk": (1.8e-2, 5.5e-4), "kerr_disk": (2.55e-2, 7.2e-4), "objects": (2.2e-7, 2.1e-11), "kerr_objects": (3.2e-8, 8.9e-9)}


@pytest.mark.parametrize("name", ["disk", "kerr_disk", "objects", "kerr_objects"])
@pytest.mark.parametrize("sense", [1, -1])
def test_restatement_against_end_state_contraction(name, sense):
    z = _golden(name)
    kerr = "spin" in z.files
    r_s, a = float(z["r_s"]), float(z["spin"]) if kerr else 0.0
    k0, end, flags = z["k0"], z["end"], z["flags"]
    x0 = np.broadcast_to(z["x0"], k0.shape)
    g = rr.g_rays(x0, k0, end, flags, r_s, a, kerr, sense)
    rel = []
    for i in range(len(k0)):
        if flags[i] not in (128, 0x88):
            continue
        # (k of the traced ray, whose picture holds the asked-for disk with the opposite sense: redshift_reference docstring)
        want = (_kerr_g_at_end(x0[i], k0[i], end[i], flags[i], 0.5 * r_s, a, -sense) if kerr
                else _schw_g_at_end(x0[i], k0[i], end[i], flags[i], r_s, -sense))
        rel.append(abs(g[i] / want - 1.0))
    assert len(rel) >= 10
    assert max(rel) < 3.0 * DRIFT[name][0], (name, max(rel))
    assert np.median(rel) < 3.0 * DRIFT[name][1], (name, np.median(rel))


def test_kerr_at_zero_spin_is_schwarzschild():
    z = _golden("disk")
    r_s = float(z["r_s"])
    rng = np.random.default_rng(5)
    for i in range(len(z["k0"])):
        x0, k0, e = z["x0"][i], z["k0"][i], z["end"][i, 0:3]
        ob = np.array([3.0, -2.0, 1.5]) * rng.uniform(0.8, 1.5)
        for cls, ee in (("disk", e), ("object", ob), ("sky", None)):
            if cls == "disk" and not 128 == z["flags"][i]:
                continue
            for s in (1, -1):
                gs = rr.g_one(x0, k0, cls, ee, r_s, 0.0, False, s)
                gk = rr.g_one(x0, k0, cls, ee, r_s, 0.0, True, s)
                assert abs(gk / gs - 1.0) < 1e-14, (cls, gs, gk)


@pytest.mark.parametrize("kerr", [False, True])
def test_closed_forms_face_on(kerr):
    r_s, M = 1.0, 0.5
    zc = 30.0
    xc = np.array([0.0, 0.0, zc])
    fc = 1.0 - r_s / zc
    rng = np.random.default_rng(1)
    for _ in range(50):
        k = np.array([rng.normal() * 0.1, rng.normal() * 0.1, -1.0])
        k /= np.linalg.norm(k)
        R = rng.uniform(1.6, 20.0)
        e = np.array([R * np.cos(1.0), R * np.sin(1.0), 0.0])
        if not kerr:
            # on the z axis L_z = 0
            assert abs(rr.g_one(xc, k, "disk", e, r_s, sense=1) / (np.sqrt(1 - 3 * M / R) / np.sqrt(fc)) - 1) < 1e-14
            assert abs(rr.g_one(xc, k, "disk", e, r_s, sense=-1) / (np.sqrt(1 - 3 * M / R) / np.sqrt(fc)) - 1) < 1e-14
        eo = rng.normal(size=3) * 4.0 + np.array([0.0, 0.0, 8.0])
        want_o = np.sqrt((1 - r_s / np.linalg.norm(eo)) / fc)
        if not kerr:
            assert abs(rr.g_one(xc, k, "object", eo, r_s) / want_o - 1) < 1e-14
            assert abs(rr.g_one(xc, k, "sky", None, r_s) * np.sqrt(fc) - 1) < 1e-14
    if kerr:
        # Kerr next to the axis (the reference camera, 1e-4 off it): theta_c -> 0, omega_c b -> 0, so the sky g -> 1 / alpha_c
        # = sqrt((r^2 + a^2) / Delta); measured 3.3e-11 off, bounded at 1e-9
        a = 0.45
        xa = np.array([1e-4, 0.0, zc])
        k = np.array([0.01, 0.02, -1.0])
        Del = zc * zc - 2 * M * zc + a * a
        assert abs(rr.g_one(xa, k, "sky", None, r_s, a, True) / np.sqrt((zc * zc + a * a) / Del) - 1) < 1e-9


@pytest.mark.parametrize("name", ["disk", "kerr_disk"])
def test_mirror_symmetry(name):
    z = _golden(name)
    kerr = "spin" in z.files
    r_s, a = float(z["r_s"]), float(z["spin"]) if kerr else 0.0
    flip = np.array([-1.0, 1.0, 1.0])
    x0 = np.broadcast_to(z["x0"], z["k0"].shape)
    for s in (1, -1):
        for i in range(len(z["k0"])):
            if z["flags"][i] != 128:
                continue
            g = rr.g_one(x0[i], z["k0"][i], "disk", z["end"][i, 0:3], r_s, a, kerr, s)
            if kerr:
                # mirroring x reverses the hole's spin too: the mirrored ray sees spin -a
                gm = rr.g_one(x0[i] * flip, z["k0"][i] * flip, "disk", z["end"][i, 0:3] * flip, r_s, -a, kerr, -s)
                assert abs(gm / g - 1.0) < 1e-12
            else:
                gm = rr.g_one(x0[i] * flip, z["k0"][i] * flip, "disk", z["end"][i, 0:3] * flip, r_s, 0.0, False, -s)
                assert gm == g


REFUSALS = [
    (dict(time_like=1), "time_like"),
    (dict(disk_r_in=1.5), "photon orbit"),          # Schwarzschild 3M = 1.5: at it
    (dict(disk_r_in=1.2), "photon orbit"),          # inside
    (dict(kerr=True, spin=0.45, disk_r_in=1.9, sense=1), "photon orbit"),    # formula sense -1: r_ph(a/M = 0.9) = 1.96 (BL)
    (dict(exponent=float("inf")), "exponent"),
    (dict(exponent=float("nan")), "exponent"),
    (dict(apply=8), "apply"),
]


@pytest.mark.parametrize("kw,what", REFUSALS)
def test_restatement_refuses(kw, what):
    kw = dict(kw)
    with pytest.raises(ValueError):
        rr.check(1.0, **kw)


def test_restatement_accepts_outside_the_photon_orbit():
    rr.check(1.0, disk_r_in=1.5000001)
    rr.check(1.0, spin=0.45, kerr=True, disk_r_in=1.2, sense=-1)  # formula sense +1: r_ph(a/M = 0.9) = 0.69 (BL)


@pytest.mark.parametrize("kw,what", REFUSALS)
def test_library_refuses(kw, what):
    from blackhole_geodesic_calculator_amd import _ffi
    lib = _ffi.load()
    kw = dict(kw)
    p = _ffi.make_params(rhs_form=_ffi.RHS_KERR_BL if kw.get("kerr") else _ffi.RHS_CHRISTOFFEL, spin=kw.get("spin", 0.0),
                         time_like=kw.get("time_like", 0), disk_r_in=kw.get("disk_r_in", 0.0),
                         disk_r_out=10.0 if "disk_r_in" in kw else 0.0)
    rs = _ffi.Redshift()
    rs.apply, rs.disk_sense, rs.exponent = kw.get("apply", 7), kw.get("sense", 1), kw.get("exponent", 4.0)
    x0 = (C.c_double * 3)(0.0, 1e-4, 30.0)
    rc = lib.bhg_redshift_device(None, C.byref(p), C.byref(rs), x0, None, None, None, None, 1, None, None)
    msg = lib.bhg_last_error().decode()
    assert rc == _ffi.E_INVALID and what in msg, msg
    # the figure is named: the photon orbit's radius appears in the message
    if what == "photon orbit":
        M, a = 0.5, kw.get("spin", 0.0)
        assert f"{rr.photon_orbit(M, a, -kw.get('sense', 1)):.6g}"[:5] in msg, msg
    rc = lib.bhg_redshift_host(None, C.byref(p), C.byref(rs), C.addressof(x0), 1, None, None, None, 1, None)
    assert rc == _ffi.E_INVALID and what in lib.bhg_last_error().decode()
    # the shade call checks the settings before the context too (the disk's r_in comes from the scene there)
    sc = _ffi.make_scene(0, 16, 8, disk=(kw["disk_r_in"], 10.0) if "disk_r_in" in kw else None)
    rc = lib.bhg_shade_scene_redshift_device(None, None, None, None, None, 1, 1, C.byref(sc), C.byref(p), C.byref(rs), x0, None, None,
                                             None, None, None)
    msg = lib.bhg_last_error().decode()
    assert rc == _ffi.E_INVALID and what in msg and "ctx" not in msg, msg


def test_library_refuses_a_disk_sense_other_than_plus_minus_one():
    from blackhole_geodesic_calculator_amd import _ffi
    lib = _ffi.load()
    p = _ffi.make_params()
    rs = _ffi.make_redshift(disk_sense=0)
    rc = lib.bhg_redshift_device(None, C.byref(p), C.byref(rs), (C.c_double * 3)(0, 0, 30), None, None, None, None, 1, None, None)
    assert rc == _ffi.E_INVALID and "disk_sense" in lib.bhg_last_error().decode()
    assert lib.bhg_frame_set_redshift(None, C.byref(rs)) == _ffi.E_INVALID


def test_binding_struct_and_names():
    from blackhole_geodesic_calculator_amd import _ffi
    assert _ffi.load().bhg_redshift_size() == C.sizeof(_ffi.Redshift) == 16
    rs = _ffi.make_redshift(("disk", "sky"), 3.0, -1)
    assert (rs.apply, rs.disk_sense, rs.exponent) == (5, -1, 3.0)
    with pytest.raises(ValueError):
        _ffi.make_redshift(("disc",))

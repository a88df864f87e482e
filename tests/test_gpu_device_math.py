"""The kernels' hand-written fp64 primitives on the GPU, one by one through bhg_math_probe, against mpmath
(tests/device_math_reference.py), in ulps of the correctly rounded result.  The bounds are derived, not
fitted: a measured maximum above its bound is a finding.  Each test records its measured maximum and the input that gives it."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import device_math_reference as dm  # noqa: E402
from test_observer_host import _numpy_kerr_cart_to_bl  # noqa: E402

EPS = dm.EPS


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _report(record_property, name, err, inputs, bound):
    m, at = dm.worst(err, inputs)
    record_property(name, {"max_ulp": m, "at": at, "bound": bound})
    print(f"{name}: max {m:.4f} ulp (bound {bound}) at {at}")
    return m


# ---- reciprocals and square roots -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bound", [("RCP_NEWTON", 1.0), ("RCP_NR", 1.0), ("RSQRT_NR", 1.0), ("SQRT_NR", 2.0)])
def test_reciprocal_and_root(ctx, record_property, name, bound):
    """<= 1 ulp: one final rounding of a value whose residual is the cube of the seed's 2^-23; sqrt_nr = x rsqrt_nr(x) has one
    more multiplication: <= 2."""
    f = _ffi()
    x = dm.positive_points()
    if name.startswith("RCP"):
        x = np.concatenate([x, -x])              # (the reciprocals take either sign)
    ref = {"RCP_NEWTON": dm.rcp_mp, "RCP_NR": dm.rcp_mp, "RSQRT_NR": dm.rsqrt_mp, "SQRT_NR": dm.sqrt_mp}[name]
    got = ctx.math_probe(getattr(f, "MATH_" + name), x)
    err = dm.ulp_error(got, ref(x))
    assert _report(record_property, name.lower(), err, x, bound) <= bound
    if name == "SQRT_NR":
        z = ctx.math_probe(f.MATH_SQRT_NR, np.array([0.0, -0.0]))
        assert np.all(z == 0.0) and not np.any(np.signbit(z))
    if name == "RCP_NEWTON":                     # rcp_nr is rcp_newton, as device_math.h says: the same bits
        assert np.array_equal(got, ctx.math_probe(f.MATH_RCP_NR, x))


def test_rcp3_nr(ctx, record_property):
    """Three reciprocals from one: two products, one reciprocal, two more products, partly correlated: <= 5 ulp."""
    x = dm.triple_points()
    got = ctx.math_probe(_ffi().MATH_RCP3_NR, x)
    want = dm.rcp3_mp(x)
    err = np.stack([dm.ulp_error(got[:, j], want[j]) for j in range(3)], 1)
    assert _report(record_property, "rcp3_nr", err.max(1), x, 5.0) <= 5.0


def test_math_probe_sizes_and_refusals(ctx):
    f = _ffi()
    assert ctx.math_probe(f.MATH_RCP_NR, np.zeros(0)).shape == (0,)
    assert ctx.math_probe(f.MATH_KERR_CART_TO_BL, np.zeros((0, 9))).shape == (0, 8)
    for n in (1, 255, 256, 257, 100001):          # ragged last workgroup: every element computed, none twice as long
        x = np.linspace(1.0, 2.0, n)
        assert np.array_equal(ctx.math_probe(f.MATH_RCP_NR, x), ctx.math_probe(f.MATH_RCP_NR, x[::-1].copy())[::-1])
        s = ctx.math_probe(f.MATH_SINCOS_PI4, x)
        assert s.shape == (n, 2) and np.all(np.abs(s[:, 0] ** 2 + s[:, 1] ** 2 - 1.0) <= 6 * EPS)
    L = f.load()
    buf = np.zeros(9)
    assert L.bhg_math_probe(ctx._h, 8, buf.ctypes.data, 1, buf.ctypes.data) == f.E_INVALID
    assert "unknown math probe op" in L.bhg_last_error().decode()
    assert L.bhg_math_probe(ctx._h, 0, None, 1, buf.ctypes.data) == f.E_INVALID
    assert "in / out" in L.bhg_last_error().decode()
    assert L.bhg_math_probe(ctx._h, 0, None, 0, None) == f.OK      # n = 0: a no-op, whatever the pointers


# ---- atan2_fast ---------------------------------------------------------------------------------------------------------
def test_atan2_fast(ctx, record_property):
    """<= 4 ulp: the algorithm with correctly rounded divisions measures 1.6 against mpmath on this point set (the CPU test of
    atan2_fast_exact_division), and each of the device's two Newton reciprocals adds at most one."""
    f = _ffi()
    y, x = dm.atan2_points()
    yx = np.stack([y, x], 1)
    got = ctx.math_probe(f.MATH_ATAN2_FAST, yx)
    err = dm.ulp_error(got, dm.atan2_mp(y, x))
    assert _report(record_property, "atan2_fast", err, yx, 4.0) <= 4.0
    # and against the restatement with exact divisions: the two Newton reciprocals move it by at most two ulps
    twin = dm.atan2_fast_exact_division(y, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(twin == 0.0, np.where(got == 0.0, 0.0, np.inf), np.abs(got - twin) / np.spacing(np.abs(twin)))
    record_property("atan2_fast_vs_exact_division_ulp", float(d.max()))
    assert d.max() <= 2.0
    assert np.all(np.abs(got) <= np.pi)


def test_atan2_fast_conventions(ctx):
    """The documented answers where libm's differ: no signed-zero ladder.  atan2_fast(+-0, +-0) = +0; (+-0, x < 0) = +pi for
    either sign of the zero (libm: -pi for -0); x = -0 counts as +0: (y, -0) = +-pi/2, (+-0, -0) = +0 (libm: +-pi)."""
    f = _ffi()
    pz, nz, pi = 0.0, -0.0, np.pi
    yx = np.array([[pz, pz], [nz, pz], [pz, nz], [nz, nz], [pz, -2.0], [nz, -2.0], [pz, -1e-300], [nz, -1e6],
                   [3.0, nz], [-3.0, nz], [3.0, pz], [-3.0, pz], [pz, 5.0], [nz, 5.0]])
    got = ctx.math_probe(f.MATH_ATAN2_FAST, yx)
    want = np.array([0.0, 0.0, 0.0, 0.0, pi, pi, pi, pi, pi / 2, -pi / 2, pi / 2, -pi / 2, 0.0, 0.0])
    assert np.array_equal(got, want), got
    assert not np.any(np.signbit(got[:4])) and not np.signbit(got[12])
    assert np.array_equal(got, dm.atan2_fast_exact_division(yx[:, 0], yx[:, 1]))


# ---- sincos_pi4 ---------------------------------------------------------------------------------------------------------
def test_sincos_pi4(ctx, record_property):
    """<= 2 ulp on |x| <= 1e5, on seeded points and on the double nearest to k pi/2 and its two neighbours for EVERY |k| <= 63 662.
    The function uses IEEE operations only, so the restatement with an exact FMA is its arithmetic: the probe returns its bits
    (any difference means that the compiler contracted or reordered something)."""
    f = _ffi()
    for label, x in (("seeded", dm.sincos_points()), ("near_multiples", dm.near_multiples_of_half_pi())):
        got = ctx.math_probe(f.MATH_SINCOS_PI4, x)
        s, c = dm.sincos_pi4_fma(x)
        assert np.array_equal(got[:, 0], s) and np.array_equal(got[:, 1], c), label
        ws, wc = dm.sincos_mp(x)
        es, ec = dm.ulp_error(got[:, 0], ws), dm.ulp_error(got[:, 1], wc)
        ms = _report(record_property, f"sincos_pi4_sin_{label}", es, x, 2.0)
        mc = _report(record_property, f"sincos_pi4_cos_{label}", ec, x, 2.0)
        assert ms <= 2.0 and mc <= 2.0
        # each within 2 ulp (<= 2^-51 relative), three roundings of the sum: |s^2 + c^2 - 1| <= 6 eps
        assert np.abs(got[:, 0] ** 2 + got[:, 1] ** 2 - 1.0).max() <= 6 * EPS
    z = ctx.math_probe(f.MATH_SINCOS_PI4, np.array([0.0, -0.0]))
    assert np.all(z[:, 0] == 0.0) and np.all(z[:, 1] == 1.0)


# ---- kerr_cart_to_bl ----------------------------------------------------------------------------------------------------
M = 1.0
SPINS = (0.0, 0.45, -0.45, 0.9, 0.998)
CAMERAS = [(1e-4, 0.0, 30.0), (1e-3, 0.0, 12.0),                    # the reference's cameras, next to the rotation axis
           (10.0, 0.0, 0.0), (0.0, 7.0, 0.0), (-5.0, -3.0, 0.0),    # the equatorial plane exactly
           (7.0, 3.0, 4.0), (0.3, -12.0, 2.5), (-2.0, 1.5, 1.2), (1.0, 1.0, 3.0), (600.0, -700.0, 300.0),
           (-6.0, 2.0, -8.0), (4.0, -3.0, -2.0), (-20.0, -15.0, -40.0)]   # z < 0; all four azimuth quadrants in the list


def _kerr_inputs():
    rng = np.random.default_rng(24)
    rows = []
    for a in SPINS:
        for mu2 in (0.0, 1.0):
            for cam in CAMERAS:
                k = rng.normal(size=(4, 3))
                k /= np.linalg.norm(k, axis=1, keepdims=True)
                for kk in k:
                    rows.append([a, M, mu2, *cam, *kk])
    return np.array(rows)


def test_kerr_cart_to_bl(ctx, record_property):
    """r: the bits of the rounded double expression (IEEE operations).  phi: atan2_fast's 4 ulp.  theta = 2 atan2_fast(sqrt_nr(1 -
    c), sqrt_nr(1 + c)) against acos of the SAME rounded double c: each root within 2.25 ulp (its own 2, half the operand's
    rounding), their ratio 4.5 ulp relative -- up to 9 ulps of the result -- and d atan(q) / atan(q) <= dq / q, plus atan2_fast's
    4: <= 13 ulp.  With e_th = 13 eps theta that angle error and |k| = 1:
      dr      (r st k_rho + R ct k_z) R / D:   |error| <= 64 eps R^2 / D        (D >= r^2: no small divisor)
      dtheta  (R ct k_rho - r st k_z) / D:      |error| <= 64 eps R / D
      dphi    (cp k_y - sp k_x) / (R st):       |error| <= (16 + 16 theta |cot theta|) eps / (R sin theta)
    (numerator: four rounded factors and an FMA, <= 4 eps absolute; 1 / (R st): rcp3_nr's 5 ulp, R 3, st 2, and st inherits
    e_th cot theta relative from the angle -- the 1 / sin theta of the formula, and theta |cot theta| on top of it, which is <= 1
    next to the +z axis and grows like pi / sin theta next to the -z axis).
    E, L: no bound on paper.  Yardstick: the float64 numpy restatement of the same algorithm (test_observer_host) against the same
    mpmath values, each error relative to the sum of the magnitudes of the terms E (L) is made of; the device, whose Newton forms
    carry up to 2 ulp where numpy's divisions and roots carry half of one, is allowed four times the restatement's maximum.
    The rebuilt 4-velocity's norm g(k, k) + mu2 (k^t from E): <= 256 eps of the sum of its terms' magnitudes (six terms, each a
    product of three or four factors good to 16 ulp)."""
    f = _ffi()
    inp = _kerr_inputs()
    out = ctx.math_probe(f.MATH_KERR_CART_TO_BL, inp)
    assert np.all(np.isfinite(out))
    n = len(inp)
    r_want = np.array([dm.kerr_r_and_quotient(row[0], row[3:6])[0] for row in inp])
    assert np.array_equal(out[:, 0], r_want)
    ref = [dm.kerr_cart_to_bl_mp(row[0], row[1], row[2], row[3:6], row[6:9]) for row in inp]
    e_th = dm.ulp_error(out[:, 1], [q["theta"] for q in ref])
    e_ph = dm.ulp_error(out[:, 2], [q["phi"] for q in ref])
    assert _report(record_property, "kerr_theta", e_th, inp, 13.0) <= 13.0
    assert _report(record_property, "kerr_phi", e_ph, inp, 4.0) <= 4.0
    worst = {"dr": 0.0, "dtheta": 0.0, "dphi": 0.0, "norm": 0.0}
    eE, eL, nE, nL = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for i, (row, q) in enumerate(zip(inp, ref)):
        with mp.workprec(200):
            R, D, st, th = q["R"], q["D"], q["sin_theta"], q["theta"]
            tol = {"dr": 64 * EPS * R * R / D, "dtheta": 64 * EPS * R / D,
                   "dphi": (16 + 16 * th * abs(q["cos_theta"] / st)) * EPS / (R * st)}
            for j, key in ((3, "dr"), (4, "dtheta"), (5, "dphi")):
                ratio = float(abs(mp.mpf(float(out[i, j])) - q[key]) / tol[key])
                worst[key] = max(worst[key], ratio)
            eE[i] = float(abs(mp.mpf(float(out[i, 6])) - q["E"]) / q["E_scale"])
            eL[i] = float(abs(mp.mpf(float(out[i, 7])) - q["L"]) / q["L_scale"])
            E_np, L_np = _numpy_kerr_cart_to_bl(row[3:6], row[6:9], row[0], row[2])
            nE[i] = float(abs(mp.mpf(float(E_np)) - q["E"]) / q["E_scale"])
            nL[i] = float(abs(mp.mpf(float(L_np)) - q["L"]) / q["L_scale"])
        res, mag = dm.kerr_norm_residual(row[0], row[1], row[2], out[i])
        worst["norm"] = max(worst["norm"], abs(res) / (256 * EPS * mag))
    record_property("kerr_fraction_of_bound", worst)
    record_property("kerr_E_L", {"device_E": eE.max(), "device_L": eL.max(), "numpy_E": nE.max(), "numpy_L": nL.max(),
                                 "at_E": dm.worst(eE, inp)[1], "at_L": dm.worst(eL, inp)[1]})
    print("kerr fractions of the bounds:", worst)
    print(f"kerr E: device {eE.max():.3e} numpy {nE.max():.3e}   L: device {eL.max():.3e} numpy {nL.max():.3e}")
    assert worst["dr"] <= 1.0 and worst["dtheta"] <= 1.0 and worst["dphi"] <= 1.0 and worst["norm"] <= 1.0
    assert eE.max() <= 4.0 * nE.max() and eL.max() <= 4.0 * nL.max()

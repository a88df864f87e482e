"""The device-math references (tests/device_math_reference.py) without a GPU: the emulated FMA against mpmath's exact one, the
restated sincos_pi4 and atan2_fast (exact divisions) against mpmath -- the figures the GPU tests' bounds are derived from --,
that the measure sees a wrong coefficient digit and a missing Cody-Waite part, and bhg_math_probe's surface and refusals
(checked before the context, so no device is needed)."""
import ctypes as C
import os
import re
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import device_math_reference as dm  # noqa: E402


def test_ulp_error_measures_in_ulps_of_the_rounded_reference():
    with mp.workprec(200):
        third = mp.mpf(1) / 3
        want = [third, third, mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(2) ** -30]
        d = float(third)
        got = np.array([d, np.nextafter(d, 1.0), np.nextafter(1.0, 2.0), -0.0, 1e-300, np.nan])
        err = dm.ulp_error(got, want)
    assert 0.0 < err[0] < 0.5 and 0.5 < err[1] < 1.5 and err[2] == 1.0 and err[3] == 0.0 and np.isinf(err[4]) and np.isinf(err[5])


def test_vectorised_fma_is_the_exact_fma_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 4000
    a = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, n)
    b = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, n)
    c = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, n)
    # cancellation to the product's last bits, ties of the final rounding, and the reduction's own shapes
    c[:1000] = -(a[:1000] * b[:1000])
    c[1000:1500] = -(a[1000:1500] * b[1000:1500]) * (1.0 + rng.choice([-1, 1], 500) * 2.0 ** -rng.integers(30, 53, 500))
    a[1500:1700], b[1500:1700], c[1500:1700] = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -23, rng.choice([-1.0, 1.0], 200) * 2.0 ** -rng.integers(50, 60, 200)
    k = np.rint(rng.uniform(-63662, 63662, 300))
    a[1700:2000], b[1700:2000], c[1700:2000] = -k, dm.PIO2[0], k * dm.PIO2[0]
    a[2000], b[2000], c[2000] = 0.0, 1.5, -0.0
    want = np.array([dm.fma_exact(x, y, z) for x, y, z in zip(a, b, c)])
    got = dm.fma_np(a, b, c)
    assert np.array_equal(got, want)
    assert np.any(got != a * b + c)          # (the cases do tell an FMA from a multiply and an add)


def test_restated_sincos_pi4_against_mpmath(record_property):
    """Derived bound: 2 ulp on |x| <= 1e5.  Seeded points and a thinned near-multiples set (every 16th k, three doubles each)."""
    x = dm.sincos_points(n=20000)
    s, c = dm.sincos_pi4_fma(x)
    ws, wc = dm.sincos_mp(x)
    es, ec = dm.ulp_error(s, ws), dm.ulp_error(c, wc)
    record_property("seeded_sin", dm.worst(es, x))
    record_property("seeded_cos", dm.worst(ec, x))
    assert es.max() <= 2.0 and ec.max() <= 2.0
    assert np.abs(s * s + c * c - 1.0).max() <= 4 * dm.EPS
    xm = dm.near_multiples_of_half_pi(step=16)
    s, c = dm.sincos_pi4_fma(xm)
    ws, wc = dm.sincos_mp(xm)
    es, ec = dm.ulp_error(s, ws), dm.ulp_error(c, wc)
    record_property("near_multiples_sin", dm.worst(es, xm))
    record_property("near_multiples_cos", dm.worst(ec, xm))
    print("sincos_pi4 restated: near multiples", es.max(), ec.max())
    assert es.max() <= 2.0 and ec.max() <= 2.0


def test_the_near_multiples_set_sees_a_missing_cody_waite_part():
    """Two parts of pi/2 in place of three: invisible on seeded points, hundreds of ulps at the worst multiple."""
    x = dm.sincos_points(n=4000)
    s, c = dm.sincos_pi4_fma(x, parts=2)
    ws, wc = dm.sincos_mp(x)
    assert max(dm.ulp_error(s, ws).max(), dm.ulp_error(c, wc).max()) <= 2.0
    k = np.arange(-63662, 63663, dtype=np.float64)
    mid = dm.near_multiples_of_half_pi()[len(k):2 * len(k)]
    s2, c2 = dm.sincos_pi4_fma(mid, parts=2)
    s3, c3 = dm.sincos_pi4_fma(mid, parts=3)
    j = int(np.argmax(np.abs(s2 - s3) / np.maximum(np.abs(s3), 1e-300) + np.abs(c2 - c3) / np.maximum(np.abs(c3), 1e-300)))
    xs = mid[j:j + 1]
    ws, wc = dm.sincos_mp(xs)
    e2 = max(dm.ulp_error(dm.sincos_pi4_fma(xs, parts=2)[0], ws)[0], dm.ulp_error(dm.sincos_pi4_fma(xs, parts=2)[1], wc)[0])
    e3 = max(dm.ulp_error(s3[j:j + 1], ws)[0], dm.ulp_error(c3[j:j + 1], wc)[0])
    assert e3 <= 2.0 < 100.0 < e2, (float(xs[0]), e2, e3)


def test_atan2_with_exact_divisions_against_mpmath(record_property):
    """The yardstick of atan2_fast's bound of 4 ulp: this restatement within 2, each of the device's two Newton reciprocals adds
    at most one."""
    y, x = dm.atan2_points()
    err = dm.ulp_error(dm.atan2_fast_exact_division(y, x), dm.atan2_mp(y, x))
    record_property("atan2_exact_division", dm.worst(err, np.stack([y, x], 1)))
    print("atan2 restated with exact divisions:", err.max())
    assert err.max() <= 2.0


def test_the_measure_sees_a_wrong_digit_of_the_leading_coefficient():
    y, x = dm.atan2_points(n=4000)
    err = dm.ulp_error(dm.atan2_fast_exact_division(y, x, lead=3.3333333333334e-01), dm.atan2_mp(y, x))
    assert err.max() > 4.0


def test_atan2_restatement_conventions():
    z = dm.atan2_fast_exact_division
    assert z(0.0, 0.0) == 0.0 and z(-0.0, -0.0) == 0.0 and z(0.0, -0.0) == 0.0
    assert z(0.0, -2.0) == np.pi and z(-0.0, -2.0) == np.pi            # (libm: -pi for y = -0)
    assert z(3.0, -0.0) == np.pi / 2 and z(-3.0, -0.0) == -np.pi / 2


# ---- bhg_math_probe: surface and refusals ------------------------------------------------------------------------------
def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def test_math_probe_is_declared_exported_and_bound():
    f, L = _lib()
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    assert re.search(r"#define BHG_MATH_PROBE 1\b", header) and re.search(r"\bbhg_math_probe\(", header)
    assert "bhg_math_probe" in f.EXPORTS and L.bhg_version() == f.ABI_VERSION == 10
    getattr(L, "bhg_math_probe")
    names = ("RCP_NEWTON", "RCP_NR", "RSQRT_NR", "SQRT_NR", "ATAN2_FAST", "SINCOS_PI4", "RCP3_NR", "KERR_CART_TO_BL")
    for i, nm in enumerate(names):
        assert re.search(rf"#define BHG_MATH_{nm} {i}\b", header) and getattr(f, "MATH_" + nm) == i
    assert f.MATH_PROBE_SHAPE[f.MATH_KERR_CART_TO_BL] == (9, 8) and f.MATH_PROBE_SHAPE[f.MATH_ATAN2_FAST] == (2, 1)


def test_math_probe_refusals():
    f, L = _lib()
    buf = (C.c_double * 9)()
    for op in (-1, 8, 1000):
        assert L.bhg_math_probe(None, op, buf, 1, buf) == f.E_INVALID
        assert "unknown math probe op" in L.bhg_last_error().decode()
    assert L.bhg_math_probe(None, 0, None, 1, buf) == f.E_INVALID and "NULL" in L.bhg_last_error().decode()
    assert L.bhg_math_probe(None, 0, buf, 1, None) == f.E_INVALID and "in / out" in L.bhg_last_error().decode()
    assert L.bhg_math_probe(None, 0, buf, 1, buf) == f.E_INVALID and "ctx" in L.bhg_last_error().decode()
    with pytest.raises(ValueError):
        f.Context.math_probe(None, 99, np.zeros(3))
    with pytest.raises(ValueError):
        f.Context.math_probe(None, f.MATH_ATAN2_FAST, np.zeros(3))

// kerr_start.h -- device functions shared by the trace kernels (geodesic_kernels.hip) and the frame kernels
// (frame_kernels.hip): the fp64 reciprocal / square-root helpers, sin and cos of one angle, and the Kerr start conversion
// kerr_cart_to_bl, which gives a ray's Killing constants E and L.  The redshift of a Kerr ray (frame_kernels.hip) takes
// its E and L from this very function, so that they are the trace's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"

namespace bhg {

// ------------------------------------------------------------------------------------------
// fp64 helpers: hardware seed + Newton.  Operands are O(1e-6 .. 1e6): no scaling needed.  Measured over that range against
// mpmath (tests/test_gpu_device_math.py; bound in brackets): rcp_nr 0.50 ulp (1), rsqrt_nr 0.83 (1),
// sqrt_nr 1.81 (2), rcp3_nr 2.85 (5).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double rcp_nr(double x)
{
    double y = __builtin_amdgcn_rcp(x);  // v_rcp_f64, ~2^-23 relative
    double e = __builtin_fma(-x, y, 1.0);
    double t = __builtin_fma(e, e, e);   // e + e^2
    return __builtin_fma(y, t, y);       // cubic: residual ~e^3
}

__device__ __forceinline__ double rsqrt_nr(double x)
{
    double y = __builtin_amdgcn_rsq(x);  // v_rsq_f64, ~2^-23 relative
    double y2 = y * y;
    double e = __builtin_fma(-x, y2, 1.0);           // 1 - x y^2
    double p = __builtin_fma(0.375, e, 0.5);          // 1/2 + 3/8 e
    double t = y * e;
    return __builtin_fma(t, p, y);                    // cubic: residual ~e^3
}

// Three reciprocals from ONE v_rcp_f64 (product inversion; the operands' product must stay inside fp64's range, which
// Delta * Sigma * sin(theta) of the Kerr right-hand side does).  A zero or NaN operand poisons all three.
__device__ __forceinline__ void rcp3_nr(double x0, double x1, double x2, double &o0, double &o1, double &o2)
{
    const double p01 = x0 * x1;
    double inv = rcp_nr(p01 * x2);   // 1/(x0 x1 x2)
    o2 = inv * p01;
    inv *= x2;                       // 1/(x0 x1)
    o1 = inv * x0;
    o0 = inv * x1;
}

// sqrt through the rsq seed + Newton (x * rsqrt_nr(x): within 2 ulp, 1.81 measured), +0 at +-0: for bounds and event functions
__device__ __forceinline__ double sqrt_nr(double x) { return x > 0.0 ? x * rsqrt_nr(x) : 0.0; }

// sin and cos of one angle together: Cody-Waite reduction by pi/2 in three parts (exact with FMA for the
// |th| < ~1e5 a polar angle can reach), then the classic degree-13 / degree-14 minimax kernels on
// [-pi/4, pi/4], quadrant fix-up by selects.  Within 2 ulp on |th| <= 1e5 (measured 1.50 for the sine and 1.47 for the
// cosine on seeded points, 0.99 on the doubles next to every multiple of pi/2 up to 63 662 pi/2, where the third part of
// pi/2 is what keeps it so: DESIGN.md section 15); IEEE operations only, so tests/device_math_reference.py restates it bit
// for bit.  ~35 instructions for both values, against two separate library calls with their large-argument paths.
//
// Attribution: the polynomial coefficients S1..S6 / C1..C6 below are those of FreeBSD msun / fdlibm's k_sin.c and
// k_cos.c: "Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved.  Developed at SunPro, a Sun
// Microsystems, Inc. business.  Permission to use, copy, modify, and distribute this software is freely granted,
// provided that this notice is preserved."
__device__ __forceinline__ void sincos_pi4(double x, double &s, double &c)
{
    const double kf = __builtin_rint(x * 0.63661977236758134308);  // 2/pi
    double r = __builtin_fma(-kf, 1.5707963267948966, x);
    r = __builtin_fma(-kf, 6.123233995736766e-17, r);
    r = __builtin_fma(-kf, -1.4973849048591698e-33, r);
    const double z = r * r;
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    const double sr = __builtin_fma(r * z, ps, r);
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double cr = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
    // quadrant fix-up: odd quadrants swap the two, bit 1 of q (of q + 1) flips the sign of the sine (cosine) -- the
    // flips as integer operations on the sign bit (three instructions each; as selects they are four or five)
    const uint32_t q = (uint32_t)(int)kf;
    const double ss = (q & 1u) ? cr : sr, cs = (q & 1u) ? sr : cr;
    const uint32_t fs = (q << 30) & 0x80000000u, fc = ((q + 1u) << 30) & 0x80000000u;
    s = __hiloint2double((int)((uint32_t)__double2hiint(ss) ^ fs), __double2loint(ss));
    c = __hiloint2double((int)((uint32_t)__double2hiint(cs) ^ fc), __double2loint(cs));
}

// Kerr: a ray's Cartesian start state (x, k) -> Boyer-Lindquist (r, theta, phi) and d/dlambda of those, in place, plus the
// Killing constants E = -k_t, L = k_phi from the norm condition g(k, k) = -mu2 at the start point (mu2 = 0: the engine's
// null rays; 1: time_like=True, proper time as parameter; future-directed root, g_tt < 0).
//     x = sqrt(r^2 + a^2) sin th cos ph,  y = sqrt(r^2 + a^2) sin th sin ph,  z = r cos th
// theta is DEFINED as acos(z / r) of the rounded quotient (the CPU checker's cart_to_bl): for the reference's camera, 1e-4
// off the rotation axis at z = 30 (CamEdition.py:208-221), that quotient is 1 - 5.6e-12 and its rounding moves theta by
// 2e-11 of itself -- far above anything else in the conversion, and Kerr rays amplify it.  So r and z / r are formed with
// IEEE square roots and an IEEE division in the checker's order of operations (bit-identical quotient), and the rest is
// free: acos(c) = 2 atan2(sqrt(1 - c), sqrt(1 + c)) (1 - c is exact for c > 1/2), sin / cos of theta from sincos_pi4,
// cos ph = x / w and sin ph = y / w as ratios (w = sqrt(x^2 + y^2)), and the inverse of the Jacobian in closed form (its
// (r, theta) block has determinant -(r^2 sin^2 th + R^2 cos^2 th) / R, R = sqrt(r^2 + a^2)):
//     k_rho = cos ph k_x + sin ph k_y,   dphi = (cos ph k_y - sin ph k_x) / (R sin th),
//     dr = (r sin th k_rho + R cos th k_z) R / D,   dtheta = (R cos th k_rho - r sin th k_z) / D.
// About 330 instructions, 64 rays wide inside a trace wave's queue fill (the lane-per-ray kernels' start_ray uses the same function, so
// every path starts a ray from bit-identical Boyer-Lindquist data).  A start ON the rotation axis (w = 0) has no azimuth: NaN, as
// the checker's 3x3 solve gives (0 / 0).
__device__ __forceinline__ void kerr_cart_to_bl(double a, double M, double mu2, double px[3], double pk[3], double &E, double &L)
{
    const double x = px[0], y = px[1], z = px[2], a2 = a * a;
    const double rho2 = x * x + y * y + z * z;
    const double b = rho2 - a2;
    const double r = sqrt(0.5 * (b + sqrt(b * b + 4.0 * a * a * z * z)));       // (IEEE sqrt, the checker's expression)
    const double c = z / r;                                                      // (IEEE division)
    const double th = 2.0 * atan2_fast(sqrt_nr(1.0 - c), sqrt_nr(1.0 + c));
    double st, ct;
    sincos_pi4(th, st, ct);
    const double r2 = r * r, R2 = r2 + a2, w2 = __builtin_fma(y, y, x * x);
    const double iR = rsqrt_nr(R2), iw = rsqrt_nr(w2);
    const double R = R2 * iR, cp = x * iw, sp = y * iw;
    const double rst = r * st, Rct = R * ct;
    const double D = __builtin_fma(rst, rst, Rct * Rct);
    const double Sig = __builtin_fma(a2 * ct, ct, r2);
    const double Del = __builtin_fma(-2.0 * M, r, R2);
    double iD, iRst, iSD;
    rcp3_nr(D, R * st, Sig * Del, iD, iRst, iSD);
    const double iSig = iSD * Del, iDel = iSD * Sig;
    const double krho = __builtin_fma(cp, pk[0], sp * pk[1]);
    const double u2 = __builtin_fma(cp, pk[1], -(sp * pk[0])) * iRst;
    const double u0 = __builtin_fma(rst, krho, Rct * pk[2]) * (R * iD);
    const double u1 = __builtin_fma(Rct, krho, -(rst * pk[2])) * iD;
    px[0] = r;
    px[1] = th;
    px[2] = atan2_fast(y, x);
    pk[0] = u0;
    pk[1] = u1;
    pk[2] = u2;
    const double s2 = st * st, tmr = 2.0 * M * r * iSig;        // 2 M r / Sigma
    const double gtt = tmr - 1.0, gtp = -tmr * a * s2;
    const double gpp = __builtin_fma(a2 * tmr, s2, R2) * s2;
    const double S = __builtin_fma(gpp * u2, u2, __builtin_fma(Sig * u1, u1, Sig * iDel * u0 * u0)) + mu2;   // g(k, k) = -mu2
    const double B = gtp * u2;
    const double kt = (-B - sqrt_nr(__builtin_fma(B, B, -(gtt * S)))) * rcp_nr(gtt);
    E = -__builtin_fma(gtt, kt, gtp * u2);
    L = __builtin_fma(gtp, kt, gpp * u2);
}

}  // namespace bhg

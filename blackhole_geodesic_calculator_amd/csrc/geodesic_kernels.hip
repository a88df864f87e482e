// geodesic_kernels.hip -- hand-written CDNA4 (gfx950) kernels for the null-geodesic hot path.
//
// What this replaces (reference file:line):
//   curvedpy.GeodesicIntegratorSchwarzschild.calc_trajectory, called once per ray at
//   raytracer/RelativisticRenderEngine.py:293-294; ODE README.md:198-209; metric README.md:162-174;
//   integrator scipy solve_ivp/RK45 (README.md:196; scipy/integrate/_ivp/rk.py:111-176).
//
// Design (MI355X-first, not a translation of the scipy loop):
//   * one wavefront lane owns one ray; the whole 6-D phase-space state, the seven stage
//     accelerations and the controller state live in VGPRs for the life of the ray;
//   * the first-order system dx/dl = k, dk/dl = a(x,k) is advanced in Nystrom form: only the
//     stage ACCELERATIONS are stored (21 doubles instead of 42), stage positions are formed from
//     x, k and the products a~ = A*A of the Dormand-Prince tableau -- algebraically the same RK
//     method, half the stage registers;
//   * workgroup = one 64-lane wavefront, persistent: a lane whose ray ends (horizon, sphere
//     exit, lambda_end) writes its result and refills from a per-wave LDS queue; the queue is
//     filled 64 rays at a time by ALL lanes together (coalesced k0 loads, the scipy initial-step
//     heuristic, start-inside test) and compacted with __ballot/mbcnt, so the expensive setup
//     always runs converged and the integrate loop always runs (nearly) full;
//   * ONE launch per trace call takes every ray to its end (~120 VGPRs in the step loop; the kernels run at 3 waves per
//     SIMD so that the event drain next to it does not spill).  The waves also work out each batch's start records -- Kerr:
//     Cartesian -> Boyer-Lindquist, E, L; every form: f0, r0, scipy's initial step -- while they fill their queue, 64 rays
//     wide; Kerr runs a finalize pass last (Boyer-Lindquist -> Cartesian end states);
//   * a lane whose accepted step crosses the horizon / exit sphere / disk plane, or whose chord may touch an object
//     sphere, does not take the step: it keeps the step's START state, and at its next service() that record goes into
//     the wave's LDS slot pool (WaveLds: queue entries, parked steps and free slots share it) and the lane pops the
//     next ray -- nothing of an event leaves the CU, and the root search never runs one lane wide.  Parked steps sit
//     on two lists: one candidate event of a monotone kind (exit sphere, disk plane) -> drain_short, a certified
//     Newton search on the dense-output polynomial; anything else (horizon, several candidates, object spheres) ->
//     drain_long, Brent as scipy's brentq does it.  A list is drained 64 wide as soon as it holds 64 steps: recompute
//     the step (bit-identical stages), dense output, root, earliest terminal root wins; a step that holds no terminal
//     event after all goes back into the ray queue and carries on.  One launch, no second pass, no host round trip;
//   * work is handed out in 64-ray batches from eight sliced device counters (a wave starts on the slice of its
//     XCD and steals from the others), each batch claimed when the queue has run out; the counters come in two sets
//     used by alternate launches, each launch zeroing the set of the next;
//   * fp64 VALU only -- v_fma_f64 chains, v_rcp_f64 / v_rsq_f64 seeds + Newton, fp32
//     v_log/v_exp seed + one cubic Newton step for err^(-1/5).  No MFMA: the path is an
//     element-wise ODE, not a contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "geodesic_kernels.h"
#include "device_math.h"
#include "kerr_start.h"

// slack factor on the disk pre-filter's excursion bound (tuning builds override it)
#ifndef BHG_DISK_SLACK
#define BHG_DISK_SLACK (1.0 + 1e-9)
#endif

namespace bhg {

// ------------------------------------------------------------------------------------------
// Dormand-Prince 5(4) coefficients (values as in scipy rk.py:377-404) and the derived
// Nystrom tables.  Index 1-based like the literature; stage 7 is the FSAL stage (a_7j = b_j).
// ------------------------------------------------------------------------------------------
struct Tableau {
    double a[8][8];   // a[i][j]
    double c[8];      // c[i] = sum_j a[i][j]
    double at[8][8];  // at[i][l] = sum_j a[i][j] a[j][l]          (position stages)
    double e[8];      // error weights E_j                          (rk.py:388-389)
    double et[8];     // et[l] = sum_j E_j a[j][l]                  (position error)
    double p[8][4];   // dense output P                             (rk.py:391-404)
    double sig[4];    // sig[m] = sum_j P[j][m]
    double pt[8][4];  // pt[l][m] = sum_j P[j][m] a[j][l]
};

constexpr Tableau make_tableau()
{
    Tableau t{};
    t.a[2][1] = 1.0 / 5;
    t.a[3][1] = 3.0 / 40;
    t.a[3][2] = 9.0 / 40;
    t.a[4][1] = 44.0 / 45;
    t.a[4][2] = -56.0 / 15;
    t.a[4][3] = 32.0 / 9;
    t.a[5][1] = 19372.0 / 6561;
    t.a[5][2] = -25360.0 / 2187;
    t.a[5][3] = 64448.0 / 6561;
    t.a[5][4] = -212.0 / 729;
    t.a[6][1] = 9017.0 / 3168;
    t.a[6][2] = -355.0 / 33;
    t.a[6][3] = 46732.0 / 5247;
    t.a[6][4] = 49.0 / 176;
    t.a[6][5] = -5103.0 / 18656;
    t.a[7][1] = 35.0 / 384;
    t.a[7][2] = 0.0;
    t.a[7][3] = 500.0 / 1113;
    t.a[7][4] = 125.0 / 192;
    t.a[7][5] = -2187.0 / 6784;
    t.a[7][6] = 11.0 / 84;
    t.c[1] = 0.0;
    t.c[2] = 1.0 / 5;
    t.c[3] = 3.0 / 10;
    t.c[4] = 4.0 / 5;
    t.c[5] = 8.0 / 9;
    t.c[6] = 1.0;
    t.c[7] = 1.0;
    for (int i = 1; i <= 7; i++)
        for (int l = 1; l <= 7; l++) {
            double s = 0.0;
            for (int j = 1; j <= 7; j++) s += t.a[i][j] * t.a[j][l];
            t.at[i][l] = s;
        }
    t.e[1] = -71.0 / 57600;
    t.e[2] = 0.0;
    t.e[3] = 71.0 / 16695;
    t.e[4] = -71.0 / 1920;
    t.e[5] = 17253.0 / 339200;
    t.e[6] = -22.0 / 525;
    t.e[7] = 1.0 / 40;
    for (int l = 1; l <= 7; l++) {
        double s = 0.0;
        for (int j = 1; j <= 7; j++) s += t.e[j] * t.a[j][l];
        t.et[l] = s;
    }
    t.p[1][0] = 1.0;
    t.p[1][1] = -8048581381.0 / 2820520608.0;
    t.p[1][2] = 8663915743.0 / 2820520608.0;
    t.p[1][3] = -12715105075.0 / 11282082432.0;
    t.p[3][1] = 131558114200.0 / 32700410799.0;
    t.p[3][2] = -68118460800.0 / 10900136933.0;
    t.p[3][3] = 87487479700.0 / 32700410799.0;
    t.p[4][1] = -1754552775.0 / 470086768.0;
    t.p[4][2] = 14199869525.0 / 1410260304.0;
    t.p[4][3] = -10690763975.0 / 1880347072.0;
    t.p[5][1] = 127303824393.0 / 49829197408.0;
    t.p[5][2] = -318862633887.0 / 49829197408.0;
    t.p[5][3] = 701980252875.0 / 199316789632.0;
    t.p[6][1] = -282668133.0 / 205662961.0;
    t.p[6][2] = 2019193451.0 / 616988883.0;
    t.p[6][3] = -1453857185.0 / 822651844.0;
    t.p[7][1] = 40617522.0 / 29380423.0;
    t.p[7][2] = -110615467.0 / 29380423.0;
    t.p[7][3] = 69997945.0 / 29380423.0;
    for (int m = 0; m < 4; m++) {
        double s = 0.0;
        for (int j = 1; j <= 7; j++) s += t.p[j][m];
        t.sig[m] = s;
        for (int l = 1; l <= 7; l++) {
            double q = 0.0;
            for (int j = 1; j <= 7; j++) q += t.p[j][m] * t.a[j][l];
            t.pt[l][m] = q;
        }
    }
    return t;
}

__device__ constexpr Tableau TB = make_tableau();

// x^(-1/10) for x in [1e-11, 1e7]: fp32 exp2/log2 seed (~1e-7) + one cubic Newton step.
__device__ __forceinline__ double pow_m0p1(double x)
{
    float xf = (float)x;
    float s = __builtin_amdgcn_exp2f(-0.1f * __builtin_amdgcn_logf(xf));  // v_exp_f32(v_log_f32)
    double y = (double)s;
    double y2 = y * y;
    double y4 = y2 * y2;
    double y8 = y4 * y4;
    double y10 = y8 * y2;
    double t = __builtin_fma(-x, y10, 1.0);           // 1 - x y^10
    double p = __builtin_fma(0.055, t, 0.1);          // (1-t)^(-1/10) = 1 + t/10 + 11/200 t^2 + ...
    double u = y * t;
    return __builtin_fma(u, p, y);
}

// ------------------------------------------------------------------------------------------
// RHS: spatial acceleration a^i = -Gamma^i_{mu nu} k^mu k^nu, k^t from the null condition
// (README.md:198-209; time_like=False at RelativisticRenderEngine.py:134).  Also returns r.
// ------------------------------------------------------------------------------------------
// Metric parameters (wave-uniform) plus, for Kerr, the ray's Killing constants.
struct Metric {
    double r_s;   // Schwarzschild radius 2M
    double M, a;  // Kerr mass and spin (Boyer-Lindquist), RHS == BHG_RHS_KERR_BL_ only
    double E, L;  // per ray: E = -k_t, L = k_phi
};

// the metric of a call; the Killing constants are the ray's to fill in
__device__ __forceinline__ Metric metric_of(double r_s, double spin)
{
    Metric m;
    m.r_s = r_s;
    m.M = 0.5 * r_s;
    m.a = spin;
    m.E = m.L = 0.0;
    return m;
}
__device__ __forceinline__ Metric metric_of(const TraceArgs &A) { return metric_of(A.r_s, A.spin); }

// Kerr in Boyer-Lindquist coordinates: x = (r, theta, phi), k = d/dlambda of those.  The body is
// generated by tools/gen_kerr_rhs.py from the sympy-derived Christoffel symbols (the reference's
// method, README.md:133-135, :182-184, applied to the Kerr metric of its goals list, README.md:218).
__device__ __forceinline__ void accel_kerr_bl(const double x[3], const double k[3], const Metric &m, double acc[3],
                                              double &r_out)
{
    const double r = x[0], th = x[1], ur = k[0], uth = k[1], uph = k[2];
    const double E = m.E, L = m.L, M = m.M, a = m.a;
    double ar, ath, aph, ktv;
    double sin_th, cos_th;
    sincos_pi4(th, sin_th, cos_th);
    {
        // the generated statements are plain products and sums; let the front end fuse a*b + c inside each
        // statement (a per-statement decision, the same wherever this function is inlined), unlike the rest
        // of the library, which spells every FMA out and is built with -ffp-contract=off
#pragma clang fp contract(on)
#define KERR_RCP(x) rcp_nr(x)
#define KERR_RCP3(o0, x0, o1, x1, o2, x2) \
    double o0, o1, o2;                    \
    rcp3_nr(x0, x1, x2, o0, o1, o2)
#define KERR_SIN(x) sin_th
#define KERR_COS(x) cos_th
#include "kerr_rhs.inc"
#undef KERR_RCP
#undef KERR_RCP3
#undef KERR_SIN
#undef KERR_COS
    }
    (void)ktv;
    acc[0] = ar;
    acc[1] = ath;
    acc[2] = aph;
    r_out = r;
}

template <int RHS>
__device__ __forceinline__ void accel(const double x[3], const double k[3], const Metric &m,
                                      double a[3], double &r)
{
    if (RHS == BHG_RHS_KERR_BL_) {
        accel_kerr_bl(x, k, m, a, r);
        return;
    }
    const double r_s = m.r_s;
    double r2 = __builtin_fma(x[2], x[2], __builtin_fma(x[1], x[1], x[0] * x[0]));
    double kk = __builtin_fma(k[2], k[2], __builtin_fma(k[1], k[1], k[0] * k[0]));
    double xk = __builtin_fma(x[2], k[2], __builtin_fma(x[1], k[1], x[0] * k[0]));
    double rinv = rsqrt_nr(r2);
    r = r2 * rinv;
    double c;
    if (RHS == BHG_RHS_REDUCED_) {
        // a = -(3/2) r_s |x cross k|^2 x / r^5
        double L2 = __builtin_fma(r2, kk, -(xk * xk));
        double w = rinv * rinv;
        double rinv5 = w * w * rinv;
        c = (-1.5 * r_s) * L2 * rinv5;
    } else {
        // a = -n [ 1/2 f f' (k^t)^2 + 1/2 f h' (n.k)^2 + (r_s/r^2)(|k|^2 - (n.k)^2) ]
        // f = 1 - r_s/r, f' = r_s/r^2, h = r_s/(r-r_s), h' = -r_s/(r-r_s)^2,
        // (k^t)^2 = (|k|^2 + h (n.k)^2)/f          -- singular at r = r_s like the contraction
        double w = rinv * rinv;        // 1/r^2
        double u = r_s * rinv;         // r_s/r
        double nk2 = xk * xk * w;      // (n.k)^2
        double f = 1.0 - u;
        double q = rcp_nr(f);          // 1/f
        double h = u * q;              // r_s/(r - r_s)
        // f' (k^t)^2 + h' (n.k)^2 with (k^t)^2 = (|k|^2 + h (n.k)^2)/f and h' = -f' / f^2, both terms
        // sharing g = f'/f:  g [ (|k|^2 + h (n.k)^2) - (n.k)^2 / f ]  -- same quantities, same 1/f
        // singularity, two multiplications fewer than forming h' and (k^t)^2 separately
        // With f * (1/f) = 1 the common factor 1/2 f g is 1/2 f':
        //   s = f' [ 1/2 ((|k|^2 + h (n.k)^2) - (n.k)^2 / f) + (|k|^2 - (n.k)^2) ]
        // (three multiplications fewer per evaluation than forming g and 1/2 f g; the 1/f singularity stays in h and q)
        double T = __builtin_fma(h, nk2, kk);
        if (RHS == BHG_RHS_CHRISTOFFEL_TL_) T += 1.0;   // time_like=True: f (k^t)^2 = |k|^2 + h (n.k)^2 + 1, the one place the norm enters
        double Y = __builtin_fma(0.5, __builtin_fma(-q, nk2, T), kk - nk2);
        c = (-u * w) * Y;              // f' / r = r_s / r^3 = (r_s / r) (1 / r^2)
    }
    a[0] = c * x[0];
    a[1] = c * x[1];
    a[2] = c * x[2];
}

__device__ __forceinline__ double ulp_of(double t)
{
    // nextafter(t, +inf) - t for t >= 0 (rk.py:119)
    long long b = __double_as_longlong(t) & 0x7FF0000000000000LL;
    double ulp = __longlong_as_double(b) * 2.220446049250313e-16;
    return t == 0.0 ? 4.9406564584124654e-324 : ulp;
}

// Cross-lane hand-off through LDS inside ONE wavefront: DS operations of a wave execute in
// program order, so only the compiler needs fencing.  (A workgroup-scope __syncthreads() would
// also drain vmcnt and stall on the in-flight result stores.)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// quartic dense output of one DP5(4) step, positions and directions (rk.py:393-404, :552-574)
struct Dense {
    double x0[3], v0[3];
    double qx[4][3], qv[4][3];
    double t0, h, ih;  // ih = 1 / h (Newton reciprocal): theta = (t - t0) * ih, within an ulp of the quotient
};

__device__ __forceinline__ void dense_pos(const Dense &d, double t, double x[3])
{
    double th = (t - d.t0) * d.ih;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = __builtin_fma(d.qx[3][i], th, d.qx[2][i]);
        s = __builtin_fma(s, th, d.qx[1][i]);
        s = __builtin_fma(s, th, d.qx[0][i]);
        x[i] = __builtin_fma(d.h * th, s, d.x0[i]);
    }
}

__device__ __forceinline__ void dense_dir(const Dense &d, double t, double v[3])
{
    double th = (t - d.t0) * d.ih;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = __builtin_fma(d.qv[3][i], th, d.qv[2][i]);
        s = __builtin_fma(s, th, d.qv[1][i]);
        s = __builtin_fma(s, th, d.qv[0][i]);
        v[i] = __builtin_fma(d.h * th, s, d.v0[i]);
    }
}

// g(t) = r(t) - R; `bl`: the state is Boyer-Lindquist (r is the first coordinate)
__device__ __forceinline__ double dense_g(const Dense &d, double t, double R, bool bl = false)
{
    double x[3];
    dense_pos(d, t, x);
    if (bl) return x[0] - R;
    return sqrt_nr(__builtin_fma(x[2], x[2], __builtin_fma(x[1], x[1], x[0] * x[0]))) - R;
}

// The disk-plane event function at the interpolated position q: z, or -- Boyer-Lindquist -- cos(theta) (z = r cos(theta),
// r > 0; the RHS's own sincos: about an ulp, a quarter of libm's cos with its large-argument ladder), once per Brent iterate
__device__ __forceinline__ double plane_g(const double q[3], bool bl)
{
    if (!bl) return q[2];
    double sn, cs;
    sincos_pi4(q[1], sn, cs);
    return cs;
}

__device__ __forceinline__ double dense_plane_g(const Dense &d, double t, bool bl)
{
    double q[3];
    dense_pos(d, t, q);
    return plane_g(q, bl);
}

// cylindrical radius of the point q, which the disk's annulus is tested on; Boyer-Lindquist: sqrt(x^2 + y^2) =
// sqrt(r^2 + a^2) |sin theta|
__device__ __forceinline__ double disk_radius(const TraceArgs &A, const double q[3], bool bl)
{
    if (!bl) return sqrt(q[0] * q[0] + q[1] * q[1]);
    double sn, cs;
    sincos_pi4(q[1], sn, cs);
    return sqrt(q[0] * q[0] + A.spin * A.spin) * fabs(sn);
}

// Brent's method on g(t) = r(t) - R over [ta, tb], xtol = rtol = 4 eps (ivp.py:51-76).
//
// Attribution: this function follows SciPy's brentq step for step (scipy/optimize/Zeros/brentq.c, "Written by
// Charles Harris charles.harris@sdl.usu.edu", part of SciPy, Copyright (c) 2001-2002 Enthought, Inc.,
// 2003- SciPy Developers, BSD 3-Clause License), including its variable names, so that the located root -- and with
// it every event state this library returns -- is the iterate scipy.integrate.solve_ivp itself would return.
// Redistribution of that algorithm's expression here is under the BSD 3-Clause terms; SciPy's licence text:
// https://github.com/scipy/scipy/blob/main/LICENSE.txt
// Runs converged in the event drain, once per parked step and candidate event.
template <class F>
__device__ __forceinline__ double brent_root(const F &g, double xa, double xb)
{
    const double tol = 4.0 * 2.220446049250313e-16;
    double xpre = xa, xcur = xb, xblk = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
    double fpre = g(xpre), fcur = g(xcur);
    if (fpre == 0.0) return xpre;
    if (fcur == 0.0) return xcur;
    for (int it = 0; it < 100; it++) {
        if (fpre != 0.0 && fcur != 0.0 && ((fpre < 0.0) != (fcur < 0.0))) {
            xblk = xpre;
            fblk = fpre;
            spre = scur = xcur - xpre;
        }
        if (fabs(fblk) < fabs(fcur)) {
            xpre = xcur;
            xcur = xblk;
            xblk = xpre;
            fpre = fcur;
            fcur = fblk;
            fblk = fpre;
        }
        double delta = (tol + tol * fabs(xcur)) * 0.5;
        double sbis = (xblk - xcur) * 0.5;
        if (fcur == 0.0 || fabs(sbis) < delta) return xcur;
        if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
            double stry;
            // (the quotients as Newton reciprocals, v_rcp_f64 + one cubic step: within an ulp or two of the IEEE
            // divisions brentq.c performs -- same iterates up to rounding, a third of the instructions; a zero
            // denominator gives inf / NaN like the division and falls through to bisection below)
            if (xpre == xblk) {
                stry = -fcur * (xcur - xpre) * rcp_nr(fcur - fpre);
            } else {
                double dpre = (fpre - fcur) * rcp_nr(xpre - xcur);
                double dblk = (fblk - fcur) * rcp_nr(xblk - xcur);
                stry = -fcur * (fblk * dblk - fpre * dpre) * rcp_nr(dblk * dpre * (fblk - fpre));
            }
            double lim = fmin(fabs(spre), 3.0 * fabs(sbis) - delta);
            if (2.0 * fabs(stry) < lim) {
                spre = scur;
                scur = stry;
            } else {
                spre = sbis;
                scur = sbis;
            }
        } else {
            spre = sbis;
            scur = sbis;
        }
        xpre = xcur;
        fpre = fcur;
        if (fabs(scur) > delta)
            xcur += scur;
        else
            xcur += (sbis > 0.0 ? delta : -delta);
        fcur = g(xcur);
    }
    return xcur;
}

// x^(1/5) for the initial-step heuristic (common.py:131): fp32 seed + one cubic Newton step on
// z = x^(-1/5), then x^(1/5) = x z^4.
__device__ __forceinline__ double pow_0p2(double x)
{
    float xf = (float)x;
    float s = __builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf(xf));
    double z = (double)s;
    double z2 = z * z;
    double z4 = z2 * z2;
    double z5 = z4 * z;
    double t = __builtin_fma(-x, z5, 1.0);
    double p = __builtin_fma(0.12, t, 0.2);  // (1-t)^(-1/5) = 1 + t/5 + 3/25 t^2 + ...
    double u = z * t;
    z = __builtin_fma(u, p, z);
    z2 = z * z;
    return x * (z2 * z2);
}

// ------------------------------------------------------------------------------------------
// Per-wave LDS: ONE pool of ray records.  A record (112 bytes; Kerr 128) is a ray's whole state between steps --
// position, direction, acceleration, step size, radius, lambda, index and step counts -- and a slot of the pool holds
//   * a QUEUED ray (prepared by the converged queue fill, or handed back by the event drain to carry on), or
//   * a PARKED step: the start state of an accepted step that (may have) crossed an event surface, waiting for the
//     converged event drain, or
//   * for the duration of a drain, the state of the lane that is busy draining.
// Three byte lists say which slot is what: the queue (a ring, popped lane by lane), the parked steps (a stack, drained
// 64 at a time) and the free slots (a stack).  Nothing of this ever goes to global memory: a trace launch reads k0
// (x0) and writes final results, and that is all of its HBM traffic.  Round 2 parked in the rays' own output slots:
// 2 x 96 bytes per parked step through L2, 3.3 - 5 x the algorithmic bytes on the event-heavy frames.
// ------------------------------------------------------------------------------------------
// Slots per wave.  Schwarzschild forms run 12 waves per CU (3 per SIMD), and the CU hands its 160 KiB of LDS out in
// 128 granules of 1,280 bytes: 10 granules = 12,800 bytes per wave = 111 records of 112 bytes + the lists.  (One
// granule more and only 11 waves fit, whatever the occupancy API says: measured -- with 118 and with 115 slots a
// twelfth of the persistent waves started when the first ones had finished; with 106 all start within 1.3 us.)
// Kerr runs 8 waves per CU and has room to spare.
#ifndef BHG_NSLOT
#define BHG_NSLOT 111
#endif
#ifndef BHG_NSLOT_KERR
#define BHG_NSLOT_KERR 150   // 8 waves per CU: 16 granules = 20,480 bytes per wave = 150 records of 128 bytes + the lists
#endif
#ifndef BHG_NSLOT_RK4
#define BHG_NSLOT_RK4 88     // the fixed-step kernels hold ~120 VGPRs and run 16 waves per CU: 8 granules = 10,240 bytes
#endif
// pool size of a kernel: by right-hand side and stepper (the fixed-step Kerr kernel runs few waves: the Schwarzschild size)
template <int RHS, bool ADAPTIVE>
struct Pool {
    static constexpr int N = ADAPTIVE ? (RHS == BHG_RHS_KERR_BL_ ? BHG_NSLOT_KERR : BHG_NSLOT)
                                      : (RHS == BHG_RHS_KERR_BL_ ? BHG_NSLOT : BHG_NSLOT_RK4);
};
// (inside the functions below `LDS` is the wave's WaveLds type)
#define NSLOT (LDS::N)
#define QRING (LDS::RING)

// One record: 12 doubles + 4 words, laid out so that a lane moves it with seven 16-byte LDS accesses
// (ds_read_b128 / ds_write_b128) -- the pop runs in almost every iteration of the step loop (some lane of the wave
// finishes a ray in nearly each one).
template <int RHS>
struct alignas(16) QEntry {
    double2 d[6];   // {x0, x1} {x2, k0} {k1, k2} {a0, a1} {a2, h} {r, lambda}
                    //   queued ray: h = |h| to try first, r = radius at the start point
                    //   parked step: h = |h| the controller chose for the step AFTER this one, r = |h| this step tried
    uint4 i;        // ray index, attempted steps, accepted steps, bits (parked: EV_* kinds; saved lane: its state bits)
    double2 el[(RHS == BHG_RHS_KERR_BL_) ? 1 : 0];  // Kerr: the ray's Killing constants E, L
};

template <int RHS, int NS>
struct WaveLds {
    static constexpr int N = NS;
    static constexpr int RING = NS <= 128 ? 128 : 256;   // ring size of the queue list (a power of two >= N)
    static_assert(NS >= 65 && NS <= 255, "the pool must hold a 64-ray batch plus one; slot ids are bytes");
    QEntry<RHS> slot[NS];
    uint8_t q_list[RING];       // slots of the queued rays, a ring: q_head .. q_head + q_count - 1 (mod RING)
    uint8_t free_list[NS];      // free slots, a stack of n_free entries
#ifdef BHG_CHECK
    uint8_t tag[NS];            // debugging: 0 free, 1 queued, 2 parked short, 3 parked long, 4 borrowed
#endif
    uint8_t ev_list[NS];        // slots of the parked steps: the SHORT list (one candidate event, exit sphere or disk
                                // plane: certified Newton search) grows up from [0], the LONG list (horizon, several
                                // candidates, object spheres, failed certificates: Brent) grows down from [NSLOT - 1]
};

#ifdef BHG_CHECK
#define SLOT_CHECK(Q, s, want, now, where)                                                                       \
    do {                                                                                                         \
        if ((s) >= (uint32_t)NSLOT || (Q).tag[(s)] != (want))                                                    \
            printf("SLOT_CHECK %s: slot %u tag %d want %d (block %d lane %d)\n", where, (unsigned)(s),           \
                   (s) < (uint32_t)NSLOT ? (int)(Q).tag[(s)] : -1, (int)(want), (int)blockIdx.x, (int)threadIdx.x); \
        if ((s) < (uint32_t)NSLOT) (Q).tag[(s)] = (now);                                                         \
    } while (0)
#define INV_CHECK(W, where)                                                                                     \
    do {                                                                                                         \
        if (threadIdx.x == 0 && (W).n_free + (W).q_count + (W).n_evA + (W).n_evB != NSLOT)                       \
            printf("INV_CHECK %s: free %d queue %d short %d long %d (block %d)\n", where, (W).n_free, (W).q_count, \
                   (W).n_evA, (W).n_evB, (int)blockIdx.x);                                                       \
    } while (0)
#else
#define SLOT_CHECK(Q, s, want, now, where) do { } while (0)
#define INV_CHECK(W, where) do { } while (0)
#endif

template <int RHS>
__device__ __forceinline__ void entry_put(QEntry<RHS> &e, const double x[3], const double k[3], const double a[3], double h,
                                          double r, double t, double E, double Lz, uint32_t idx, uint32_t natt,
                                          uint32_t nacc, uint32_t bits)
{
    e.d[0] = make_double2(x[0], x[1]);
    e.d[1] = make_double2(x[2], k[0]);
    e.d[2] = make_double2(k[1], k[2]);
    e.d[3] = make_double2(a[0], a[1]);
    e.d[4] = make_double2(a[2], h);
    e.d[5] = make_double2(r, t);
    e.i = make_uint4(idx, natt, nacc, bits);
    if (RHS == BHG_RHS_KERR_BL_) e.el[0] = make_double2(E, Lz);
}

// Kinds of event a parked step may hold (the `bits` word of its record; they never reach flags[]).
constexpr uint32_t EV_HORIZON = 1u, EV_EXIT = 2u, EV_DISK = 4u, EV_OBJ = 8u;
// ... and a step that has NOT been computed yet: the lane's last accepted step ended close enough to
// the exit sphere that the next one is expected to leave it, so the lane hands the ray -- a queue-style record: the state at
// the step's start, the |h| to try, the radius there -- to the short drain, which runs the WHOLE step (stages, error norm,
// controller, event tests) and then locates the exit; the lane takes a fresh ray one iteration earlier and the step is
// computed once instead of twice.  Where the step is computed never changes a result.
constexpr uint32_t EV_AHEAD = 16u;
constexpr uint32_t EV_REQUEUE = 32u;     // (marks the bits of a queue entry written back by the short drain; bit 0 = rejected)
// Which kernel variants do: the Schwarzschild forms with the exit sphere -- config 4's <0,5>, config 3's <0,3>, the exit-only
// frames <0,1>, <1,1>.  Measured, round 6, bit-identical on eight full-size workloads, same-box A/Bs (profiles/r06_ahead_ab.log,
// r06_ahead_disk_ab.log): config 4 -2.4 % time, the exit frame -2.5 %, config 3 -1.1 %.  With the disk the registers are the
// whole story: <0,3> sits at 167 VGPRs, and the first three builds of it (a rejected step handed back through R, i.e. a second
// source for R behind the stages) spilled 140-156 B per lane, part of it in the MAIN loop: +32 % time.  Handing a rejected
// step back from P, its bits in `kind` (not even one more live word), leaves 52 B in the drains and nothing in the main loop.
// Not the reduced form with the disk (<1,3> spills into its main loop with it).  The Boyer-Lindquist kernels: with the disk
// (Kerr + disk -1.5 % time), not without (a Kerr exit-only frame +2.6 %, profiles/r06_ahead_kerr_ab.log).
constexpr int EVT_EXIT = 1, EVT_DISK = 2, EVT_OBJ = 4;
template <int RHS, int EVT>
struct RunsAhead {
    static constexpr bool value = (EVT & 1 /* EVT_EXIT */) != 0 &&
                                  (RHS == BHG_RHS_KERR_BL_ ? (EVT & 2 /* EVT_DISK */) != 0
                                                           : ((EVT & 2 /* EVT_DISK */) == 0 || RHS == BHG_RHS_CHRISTOFFEL_));
};

// Boyer-Lindquist position (r, theta, phi) -> Cartesian: x = sqrt(r^2 + a^2) sin th cos ph, y = ... sin ph, z = r cos th.
// Object spheres live in the Cartesian frame the boundary speaks; a Kerr ray meets them through this (the RHS's own sincos).
__device__ __forceinline__ void bl_position_to_cart(double a, const double q[3], double out[3])
{
    double st, ct, sp, cp;
    sincos_pi4(q[1], st, ct);
    sincos_pi4(q[2], sp, cp);
    const double Rs = sqrt_nr(__builtin_fma(q[0], q[0], a * a)) * st;
    out[0] = Rs * cp;
    out[1] = Rs * sp;
    out[2] = q[0] * ct;
}

// Does the accepted step x0 -> x1 possibly enter one of the object spheres?  A ray outside sphere j at the
// step's start enters it if the step ends inside, or if the chord between the step ends passes through
// (closest point of the chord at s* = b / cc in (0, 1) with squared distance d0 - b^2 / cc < rho^2, written
// without the division).
// a Boyer-Lindquist state (q = (r, theta, phi), u its derivative) in the Cartesian frame the boundary speaks: position, then the
// Jacobian of the embedding applied to u.  ONE definition for the finalize pass and for the crossing records.
__device__ __forceinline__ void bl_record_to_cart(double a, const double q[3], const double u[3], double c[6])
{
    const double r = q[0], th = q[1], ph = q[2], u0 = u[0], u1 = u[1], u2 = u[2];
    const double R = sqrt(r * r + a * a), st = sin(th), ct = cos(th), sp = sin(ph), cp = cos(ph);
    c[0] = R * st * cp;
    c[1] = R * st * sp;
    c[2] = r * ct;
    c[3] = (r / R * st * cp) * u0 + (R * ct * cp) * u1 + (-R * st * sp) * u2;
    c[4] = (r / R * st * sp) * u0 + (R * ct * sp) * u1 + (R * st * cp) * u2;
    c[5] = ct * u0 + (-r * st) * u1 + 0.0 * u2;
}

__device__ __forceinline__ bool sphere_candidate(const double sp[4], const double x0[3], const double x1[3], double &bb,
                                                 double &cc, bool &ends_inside)
{
    // (sums of products as FMA chains: this test runs for every lane in every step of an object frame; the CPU
    // checker rounds each product -- the candidate decision could only differ for a chord grazing the sphere within
    // an ulp, and what a candidate is worth is decided by the root search on the dense output either way)
    const double rho2 = sp[3] * sp[3];
    const double a0[3] = {x0[0] - sp[0], x0[1] - sp[1], x0[2] - sp[2]};
    const double a1[3] = {x1[0] - sp[0], x1[1] - sp[1], x1[2] - sp[2]};
    const double d0 = __builtin_fma(a0[2], a0[2], __builtin_fma(a0[1], a0[1], a0[0] * a0[0]));
    const double d1 = __builtin_fma(a1[2], a1[2], __builtin_fma(a1[1], a1[1], a1[0] * a1[0]));
    bb = cc = 0.0;
    ends_inside = false;
    if (!(d0 > rho2)) return false;
    if (d1 <= rho2) {
        ends_inside = true;
        return true;
    }
    const double ch[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]};
    cc = __builtin_fma(ch[2], ch[2], __builtin_fma(ch[1], ch[1], ch[0] * ch[0]));
    bb = -__builtin_fma(a0[2], ch[2], __builtin_fma(a0[1], ch[1], a0[0] * ch[0]));
    return bb > 0.0 && bb < cc && (d0 - rho2) * cc < bb * bb;
}

// Did the step cross the disk plane z = 0?  Cartesian forms: sign change of z (either end on the plane counts,
// like a scipy event).  Boyer-Lindquist: z = r cos(theta) with r > 0 changes sign when theta moves from one
// interval (pi/2 + k pi, pi/2 + (k+1) pi] to another -- an integer comparison, no trigonometry in the loop.
// cos(theta) is never exactly 0 for a double theta, so scipy's <= / >= cannot matter; which side the interval's end
// belongs to does, at one value: the double nearest pi/2 -- acos(0), the theta of every start in the equatorial plane --
// lies BELOW pi/2 (its cosine is +6.1e-17), with the thetas under it.  Hence ceil, not floor: a ray that leaves the plane
// downwards (theta growing) has its crossing at t = 0, as the reference has; one that leaves it upwards has none.
template <int RHS>
__device__ __forceinline__ bool crossed_disk_plane(const double x0[3], const double x1[3])
{
    if (RHS == BHG_RHS_KERR_BL_) {
        const double k0 = ceil((x0[1] - 1.5707963267948966) * 0.3183098861837907);
        const double k1 = ceil((x1[1] - 1.5707963267948966) * 0.3183098861837907);
        return k0 != k1;
    }
    return ((x0[2] <= 0.0) && (x1[2] >= 0.0)) || ((x0[2] >= 0.0) && (x1[2] <= 0.0));
}

// A step that crosses the disk plane z = 0 needs the event drain only if the crossing can lie in the annulus; one that
// cannot carries on for good, so what decides here must be a BOUND (round 3's figure was not: it left out the grazing
// factor and the quartic remainder, and grazing crossings at rtol >= 3e-3 exceeded it -- VERDICT r03, weak #2).
//
// The step's dense output D (theta in [0, 1]) is a quartic per position component with D(0) = x0, D(1) = x1,
// D'(0) = h v0, D'(1) = h v1 (the Dormand-Prince interpolant is C1) and leading coefficient h q3.  With H the cubic
// Hermite interpolant of the same end data and C the chord:
//     D - H = h q3 theta^2 (1 - theta)^2                          |D_c - H_c| <= |h q3_c| / 16        (exact identity)
//     H - C = e0 theta (1 - theta)^2 - e1 theta^2 (1 - theta)     |H_c - C_c| <= (4/27)(|e0_c| + |e1_c|)
// e0 = h v0 - (x1 - x0), e1 = h v1 - (x1 - x0); so every component of the curve stays within
//     delta_c = (4/27)(|e0_c| + |e1_c|) + |h q3_c| / 16
// of the chord.  ANY plane crossing theta_d of D (whichever one the root search lands on) then lies within
// delta_z / |dz| of the chord's crossing parameter, and the crossing POINT within
//     eps = delta_x + delta_y + (|dx| + |dy|) delta_z / |dz|
// (1-norm >= length >= difference of the cylindrical radii) of the chord's crossing point.  Outside
// [R_in - eps, R_out + eps]: not terminal, exactly as the drain would have decided.  tests/test_disk_filter_bound.py
// holds the same formula in numpy against 30,000 scipy-RK45 plane crossings from cameras down to 0.001 degrees above
// the plane at rtol 1e-3 ... 1e-1: the worst crossing uses 0.89 of eps, the median one 0.35 (round 3's figure: exceeded
// 1.6 x there).  The fixed-step kernels locate events on the cubic Hermite interpolant itself: QUARTIC = false, no q3 term.
// Runs in the step loop whenever any lane of the wave crossed the plane -- in practically every iteration of a disk
// frame: no divisions (everything is compared multiplied through by |dz|), no square roots; |.| is a free operand modifier.
template <bool QUARTIC>
__device__ __forceinline__ bool disk_crossing_may_hit(const TraceArgs &A, const double x0[3], const double v0[3],
                                                      const double x1[3], const double v1[3], double h,
                                                      const double a1[3], const double a2[3], const double a3[3],
                                                      const double a4[3], const double a5[3], const double a6[3])
{
    // With D = z0 - z1 the chord's crossing point is P / D, P = z0 (x1, y1) - z1 (x0, y0): R_chord = |P| / |D|.
    const double D = x0[2] - x1[2];
    const double Px = __builtin_fma(x0[2], x1[0], -(x1[2] * x0[0])), Py = __builtin_fma(x0[2], x1[1], -(x1[2] * x0[1]));
    const double P2 = __builtin_fma(Px, Px, Py * Py);
    const double h2s = (h * h) * 0.0625;
    double dl[3], ch[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double dx = x1[c] - x0[c];
        const double e0 = __builtin_fma(h, v0[c], -dx), e1 = __builtin_fma(h, v1[c], -dx);
        ch[c] = dx;
        dl[c] = (4.0 / 27.0) * (fabs(e0) + fabs(e1));
        if (QUARTIC) {
            // h q3_c = h^2 sum_j P~[j][3] a_j[c] (P~[7][3] = 0; sum_j P[j][3] = 0: no v term), as build_dense_pos forms it
            double qx = TB.pt[1][3] * a1[c];
            if (TB.pt[2][3] != 0.0) qx = __builtin_fma(TB.pt[2][3], a2[c], qx);   // (rounding dust of the constexpr table)
            qx = __builtin_fma(TB.pt[3][3], a3[c], qx);
            qx = __builtin_fma(TB.pt[4][3], a4[c], qx);
            qx = __builtin_fma(TB.pt[5][3], a5[c], qx);
            qx = __builtin_fma(TB.pt[6][3], a6[c], qx);
            dl[c] = __builtin_fma(h2s, fabs(qx), dl[c]);
        }
    }
    // eps |D| = (delta_x + delta_y) |D| + (|dx| + |dy|) delta_z; the relative slack covers this function's own rounding,
    // the absolute term (1e-11 in R) the few ulps of |x| <= 1e3 by which the drain's evaluation of D itself is uncertain
    const double aD = fabs(D);
    double E = __builtin_fma(fabs(ch[0]) + fabs(ch[1]), dl[2], (dl[0] + dl[1]) * aD);
    E = __builtin_fma(E, BHG_DISK_SLACK, 1e-11 * aD);
    const double lo = __builtin_fma(A.disk_r_in, aD, -E), hi = __builtin_fma(A.disk_r_out, aD, E);
    // |P| against [lo, hi], compared as squares; a step lying in the plane (D = 0, P = 0) and NaN anywhere fall through
    // to "may hit"
    return !((lo > 0.0 && P2 < lo * lo) || P2 > hi * hi);
}

// The same question in Boyer-Lindquist coordinates (x = (r, theta, phi)): the plane is theta* = pi/2 + k pi, the
// annulus is in sqrt(r^2 + a^2).  The dense output is a quartic in these coordinates too, so the component bounds
// delta_r, delta_th hold as above; the dense curve reaches theta* within delta_th / |th1 - th0| of the chord's crossing
// parameter, so its r there lies within eps = delta_r + |r1 - r0| delta_th / |th1 - th0| of the chord's r.  More than
// one plane crossed in the step, or a step (nearly) tangent to the plane (eps blows up): may hit.
template <bool QUARTIC>
__device__ __forceinline__ bool disk_crossing_may_hit_bl(const TraceArgs &A, const double x0[3], const double v0[3],
                                                         const double x1[3], const double v1[3], double h,
                                                         const double a1[3], const double a2[3], const double a3[3],
                                                         const double a4[3], const double a5[3], const double a6[3])
{
    const double k0 = floor((x0[1] - 1.5707963267948966) * 0.3183098861837907);
    const double k1 = floor((x1[1] - 1.5707963267948966) * 0.3183098861837907);
    if (fabs(k1 - k0) != 1.0) return true;
    const double th_star = __builtin_fma(3.141592653589793, fmax(k0, k1), 1.5707963267948966);
    const double dth = x1[1] - x0[1], dr = x1[0] - x0[0];
    const double idth = rcp_nr(dth);
    const double s = (th_star - x0[1]) * idth;
    const double r_lin = __builtin_fma(s, dr, x0[0]);
    const double h2s = (h * h) * 0.0625;
    double dl[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const double dx = x1[c] - x0[c];
        const double e0 = __builtin_fma(h, v0[c], -dx), e1 = __builtin_fma(h, v1[c], -dx);
        dl[c] = (4.0 / 27.0) * (fabs(e0) + fabs(e1));
        if (QUARTIC) {
            double qx = TB.pt[1][3] * a1[c];
            if (TB.pt[2][3] != 0.0) qx = __builtin_fma(TB.pt[2][3], a2[c], qx);
            qx = __builtin_fma(TB.pt[3][3], a3[c], qx);
            qx = __builtin_fma(TB.pt[4][3], a4[c], qx);
            qx = __builtin_fma(TB.pt[5][3], a5[c], qx);
            qx = __builtin_fma(TB.pt[6][3], a6[c], qx);
            dl[c] = __builtin_fma(h2s, fabs(qx), dl[c]);
        }
    }
    // (the reciprocal is a Newton one, an ulp or two: inside the relative slack; 1e-11 as above)
    const double eps = __builtin_fma(__builtin_fma(fabs(dr), dl[1] * fabs(idth), dl[0]), BHG_DISK_SLACK * (1.0 + 1e-12), 1e-11);
    const double a2s = A.spin * A.spin;
    const double r_lo = fmax(r_lin - eps, 0.0), r_hi = r_lin + eps;
    // R = sqrt(r^2 + a^2) against the annulus, compared in squares
    const double R2_lo = __builtin_fma(r_lo, r_lo, a2s), R2_hi = __builtin_fma(r_hi, r_hi, a2s);
    return !(R2_hi < A.disk_r_in * A.disk_r_in || R2_lo > A.disk_r_out * A.disk_r_out);  // NaN anywhere: may hit
}

// The sharp form of the same question, for the crossings the chord bound above lets through (in Boyer-Lindquist
// coordinates, where dr/dlambda changes along a straight line, the chord is a poor model of the curve and the bound
// correspondingly wide).  EXACT relation between the step's dense output D and the cubic Hermite interpolant H through its
// end states: both match x and dx/dlambda at both ends (the DP5 dense output is C1: D'(0) = h v0, D'(1) = h v1), so
// their difference is the quartic with double roots at 0 and 1,
//         D_c(th) - H_c(th) = (h q3_c) th^2 (1 - th)^2,     |D_c - H_c| <= |h q3_c| / 16,
// q3 the dense output's leading coefficient -- six FMAs per component from the stage accelerations the step loop holds.
// So: the plane crossing th_h of H (two Newton steps from the chord's), the crossing of D within
// dth = 1.5 e_z / |H_z'(th_h)| of it where H_z is monotone (it is checked), and the crossing POINT of D within
// e_xy + |H_xy'| dth of H_xy(th_h).  Outside the annulus widened by that: not terminal, the ray carries on.
template <int RHS>
__device__ __forceinline__ bool disk_crossing_may_hit_sharp(const TraceArgs &A, const double x0[3], const double v0[3],
                                                            const double x1[3], const double v1[3], double h,
                                                            const double a1[3], const double a2[3], const double a3[3],
                                                            const double a4[3], const double a5[3], const double a6[3])
{
    constexpr bool BL = RHS == BHG_RHS_KERR_BL_;
    constexpr int ce = BL ? 1 : 2;      // the coordinate the plane is a level set of
    double target = 0.0;
    if (BL) {
        const double k0 = floor((x0[1] - 1.5707963267948966) * 0.3183098861837907);
        const double k1 = floor((x1[1] - 1.5707963267948966) * 0.3183098861837907);
        if (fabs(k1 - k0) != 1.0) return true;      // (a lane that crossed no plane, or several: let the drain decide)
        target = __builtin_fma(3.141592653589793, fmax(k0, k1), 1.5707963267948966);
    }
    // |h q3_c| / 16 (P~[7][3] = 0: stage 7 does not enter)
    double e4[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double qx = TB.pt[1][3] * a1[c];
        qx = __builtin_fma(TB.pt[2][3], a2[c], qx);
        qx = __builtin_fma(TB.pt[3][3], a3[c], qx);
        qx = __builtin_fma(TB.pt[4][3], a4[c], qx);
        qx = __builtin_fma(TB.pt[5][3], a5[c], qx);
        qx = __builtin_fma(TB.pt[6][3], a6[c], qx);
        e4[c] = fabs(h * __builtin_fma(h, qx, TB.sig[3] * v0[c])) * 0.0625;
    }
    // Hermite: H(th) = x0 + b1 th + b2 th^2 + b3 th^3, b1 = h v0, b2 = 3 d - 2 h v0 - h v1, b3 = -2 d + h v0 + h v1
    double b1[3], b2[3], b3[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double d = x1[c] - x0[c], m0 = h * v0[c], m1 = h * v1[c];
        b1[c] = m0;
        b2[c] = __builtin_fma(3.0, d, -__builtin_fma(2.0, m0, m1));
        b3[c] = __builtin_fma(-2.0, d, m0 + m1);
    }
    const double z0 = x0[ce] - target, dz = x1[ce] - x0[ce];
    // H_z monotone over the step?  H_z' is a parabola: its values at both ends and at an interior extremum must all have
    // the sign of dz, and not be small against it (a tangential crossing: let the drain decide)
    const double g0 = b1[ce], g1 = __builtin_fma(3.0, b3[ce], __builtin_fma(2.0, b2[ce], b1[ce]));
    const double the = -b2[ce] * rcp_nr(3.0 * b3[ce]);                       // extremum of H_z' (NaN / inf: no interior one)
    const double ge = (the > 0.0 && the < 1.0) ? __builtin_fma(b2[ce], the, b1[ce]) : g0;   // H_z'(the) = b1 + b2 the there
    const double sgn = dz < 0.0 ? -1.0 : 1.0;
    const double gmin = fmin(fmin(g0 * sgn, g1 * sgn), ge * sgn);
    if (!(gmin > 0.125 * fabs(dz))) return true;
    double th = -z0 * rcp_nr(dz);
    th = fmin(fmax(th, 0.0), 1.0);
    double f = 0.0, df = 1.0;
#pragma unroll
    for (int it = 0; it < 2; it++) {
        f = __builtin_fma(__builtin_fma(__builtin_fma(b3[ce], th, b2[ce]), th, b1[ce]), th, z0);
        df = __builtin_fma(__builtin_fma(3.0 * b3[ce], th, 2.0 * b2[ce]), th, b1[ce]);
        th = fmin(fmax(__builtin_fma(-f, rcp_nr(df), th), 0.0), 1.0);
    }
    f = __builtin_fma(__builtin_fma(__builtin_fma(b3[ce], th, b2[ce]), th, b1[ce]), th, z0);
    // the dense output's crossing lies within dth of th: |H_z| <= e_z there, H_z' >= gmin throughout
    const double dth = (1.5 * e4[ce] + fabs(f)) * rcp_nr(gmin);
    if (BL) {
        const double r = __builtin_fma(__builtin_fma(__builtin_fma(b3[0], th, b2[0]), th, b1[0]), th, x0[0]);
        // (|H_r'| <= |b1| + 2|b2| + 3|b3| on [0, 1])
        const double er = __builtin_fma(fabs(b1[0]) + __builtin_fma(2.0, fabs(b2[0]), 3.0 * fabs(b3[0])), dth, e4[0]) * (1.0 + 1e-6);
        const double aa = A.spin * A.spin;
        const double r_lo = fmax(r - er, 0.0), r_hi = r + er;
        return !(__builtin_fma(r_hi, r_hi, aa) < A.disk_r_in * A.disk_r_in || __builtin_fma(r_lo, r_lo, aa) > A.disk_r_out * A.disk_r_out);
    }
    const double X = __builtin_fma(__builtin_fma(__builtin_fma(b3[0], th, b2[0]), th, b1[0]), th, x0[0]);
    const double Y = __builtin_fma(__builtin_fma(__builtin_fma(b3[1], th, b2[1]), th, b1[1]), th, x0[1]);
    const double sl = (fabs(b1[0]) + __builtin_fma(2.0, fabs(b2[0]), 3.0 * fabs(b3[0]))) +
                      (fabs(b1[1]) + __builtin_fma(2.0, fabs(b2[1]), 3.0 * fabs(b3[1])));
    const double eps = __builtin_fma(sl, dth, e4[0] + e4[1]) * (1.0 + 1e-6);     // (1-norm of the error in (x, y) >= its length)
    const double R2 = __builtin_fma(X, X, Y * Y);
    const double lo = A.disk_r_in - eps, hi = A.disk_r_out + eps;
    return !((lo > 0.0 && R2 < lo * lo) || R2 > hi * hi);       // NaN anywhere: may hit
}

// The step loop's version of that test: a SUPERSET of sphere_candidate() in straight-line code (the event drain applies
// the exact test to whatever is parked, and a step it then finds empty carries on -- so a false positive costs a little
// time and a false negative would cost a hit).  One set of differences for both ends (d1 = d0 - 2 b + c instead of a
// second distance), no divergent branches, and a relative slack of 1e-9 on the two comparisons that rounding could
// turn the other way.  23 instead of 30 instructions per sphere and step, in every step of an object frame.
__device__ __forceinline__ bool sphere_maybe(const double sp[4], const double x0[3], const double x1[3])
{
    const double rho2 = sp[3] * sp[3], rho2s = rho2 * (1.0 + 1e-9);
    const double a0[3] = {x0[0] - sp[0], x0[1] - sp[1], x0[2] - sp[2]};
    const double ch[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]};
    const double d0 = __builtin_fma(a0[2], a0[2], __builtin_fma(a0[1], a0[1], a0[0] * a0[0]));
    const double cc = __builtin_fma(ch[2], ch[2], __builtin_fma(ch[1], ch[1], ch[0] * ch[0]));
    const double bb = -__builtin_fma(a0[2], ch[2], __builtin_fma(a0[1], ch[1], a0[0] * ch[0]));
    const double d1 = __builtin_fma(-2.0, bb, d0) + cc;
    const bool through = bb > 0.0 && bb < cc && (d0 - rho2s) * cc < bb * bb;
    return d0 > rho2 && (d1 <= rho2s || through);
}

__device__ __forceinline__ bool any_sphere_candidate(const TraceArgs &A, const double x0[3], const double x1[3])
{
    bool any = false;
    for (int j = 0; j < A.n_spheres; j++) any |= sphere_maybe(A.spheres[j], x0, x1);
    return any;
}

// ... for a step in Boyer-Lindquist coordinates: the same test on the Cartesian images of the step's ends
template <int RHS>
__device__ __forceinline__ bool any_sphere_candidate_of(const TraceArgs &A, const double x0[3], const double x1[3])
{
    if (RHS != BHG_RHS_KERR_BL_) return any_sphere_candidate(A, x0, x1);
    if (A.n_spheres == 0) return false;
    double c0[3], c1[3];
    bl_position_to_cart(A.spin, x0, c0);
    bl_position_to_cart(A.spin, x1, c1);
    return any_sphere_candidate(A, c0, c1);
}

struct Lane {
    double x[3], v[3], a1[3];
    double t, h_abs, r_cur;
    double E, Lz;  // Kerr only
    uint32_t idx, n_att, n_acc;
    // 0 / 1, as full words: a bool is kept as a byte and compared through SDWA against a zero held in a VGPR for the
    // life of the kernel -- a register the allocator then spills around the event drain and reloads in the loop
    uint32_t active, rejected;
    // EV_* bits of an accepted step this lane has to park: x, v, a1, t are still the step's START, h_abs is the
    // controller's choice for the NEXT step and r_cur has been overwritten with the |h| THIS step tried (the drain
    // recomputes the step from exactly these).  The record goes into the pool the next time the lane is served.
    uint32_t pend;
};

template <int RHS>
__device__ __forceinline__ void slot_put(QEntry<RHS> &e, const Lane &L, uint32_t bits)
{
    entry_put<RHS>(e, L.x, L.v, L.a1, L.h_abs, L.r_cur, L.t, L.E, L.Lz, L.idx, L.n_att, L.n_acc, bits);
}

template <int RHS>
__device__ __forceinline__ uint32_t slot_get(const QEntry<RHS> &e, Lane &L)
{
    const double2 d0 = e.d[0], d1 = e.d[1], d2 = e.d[2], d3 = e.d[3], d4 = e.d[4], d5 = e.d[5];
    const uint4 i = e.i;
    L.x[0] = d0.x;
    L.x[1] = d0.y;
    L.x[2] = d1.x;
    L.v[0] = d1.y;
    L.v[1] = d2.x;
    L.v[2] = d2.y;
    L.a1[0] = d3.x;
    L.a1[1] = d3.y;
    L.a1[2] = d4.x;
    L.h_abs = d4.y;
    L.r_cur = d5.x;
    L.t = d5.y;
    L.idx = i.x;
    L.n_att = i.y;
    L.n_acc = i.z;
    if (RHS == BHG_RHS_KERR_BL_) {
        const double2 el = e.el[0];
        L.E = el.x;
        L.Lz = el.y;
    }
    return i.w;
}

// state bits of a lane whose registers wait in a slot while the lane drains events
__device__ __forceinline__ uint32_t lane_bits(const Lane &L) { return L.active | (L.rejected << 1) | (L.pend << 4); }
__device__ __forceinline__ void lane_set_bits(Lane &L, uint32_t b)
{
    L.active = b & 1u;
    L.rejected = (b >> 1) & 1u;
    L.pend = b >> 4;
}

struct Wave {
    int q_head, q_count;         // the queue ring
    int n_free;                  // entries of the free-slot stack
    int n_evA, n_evB;            // parked steps on the short list and on the long list (see WaveLds::ev_list)
    bool exhausted;
    uint32_t slice, dry;         // current slice, number of slices found dry so far
#ifdef BHG_DIAG
    unsigned long long diag_drain_cyc = 0, diag_drained = 0, diag_fill_cyc = 0, diag_refill_cyc = 0, diag_general = 0;
    unsigned long long diag_drained_long = 0, diag_drain_long_cyc = 0;
#endif
};

// A ray's FINAL state: the whole record end[idx] = {x, v}, or -- direction-only calls (A.end_dir; sky frames read
// nothing else) -- v alone into end_dir[idx]: 24 instead of 48 bytes written per ray and read by the shade kernel.
// Byte offsets of a ray's results are formed in 32 bits and added to the (wave-uniform) array bases: the stores then
// take the scalar-base + 32-bit-VGPR-offset form, where 64-bit pointer arithmetic per lane is five more instructions per
// finished ray -- in a path that runs in nearly every iteration of the step loop.  Good for n * 48 < 2^32: a launch
// holds at most BHG_MAX_RAYS_PER_LAUNCH = 2^26 rays (the C-ABI layer splits larger calls into several launches).
template <class T>
__device__ __forceinline__ T *at_offset(T *base, uint32_t byte_offset)
{
    return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_offset);
}

__device__ __forceinline__ void store_end_state(const TraceArgs &A, uint32_t idx, const double x[3], const double v[3])
{
    if (A.end_dir) {  // (wave-uniform)
        double *e = at_offset(A.end_dir, idx * 24u);
        e[0] = v[0];
        e[1] = v[1];
        e[2] = v[2];
        return;
    }
    double *e = at_offset(A.end, idx * 48u);
    // 48 contiguous bytes per lane: three 16-byte stores
    // (streaming / non-temporal stores here were measured in round 5: -0.5 % on the full-record frame, neutral elsewhere)
    reinterpret_cast<double2 *>(e)[0] = make_double2(x[0], x[1]);
    reinterpret_cast<double2 *>(e)[1] = make_double2(x[2], v[0]);
    reinterpret_cast<double2 *>(e)[2] = make_double2(v[1], v[2]);
}

// CHECK = false: the state is the end of an ACCEPTED step, which is finite by construction -- a non-finite component makes
// the error norm NaN (a NaN reaches it through the stage-7 acceleration, an infinity through a scale factor of 0 times an
// infinite product), and a NaN error norm rejects the step -- so the test (seven instructions) is left out of the one
// store that runs in nearly every iteration of the step loop: a ray reaching lambda_end.
template <bool CHECK = true>
__device__ __forceinline__ void store_result(const TraceArgs &A, uint32_t idx, const double x[3],
                                             const double v[3], uint32_t flags, uint32_t n_att,
                                             uint32_t n_acc)
{
    if (CHECK) {
        // any NaN or infinity among the six makes their sum non-finite (inf - inf is NaN): five additions and one class test
        // instead of six class tests and their combination (the state is O(1e2) at most, the sum cannot overflow)
        const bool bad = !isfinite(((x[0] + x[1]) + (x[2] + v[0])) + (v[1] + v[2]));
        if (bad) flags |= BHG_FLAG_NAN_;
    }
    store_end_state(A, idx, x, v);
    // (flags, n_steps, n_accepted are never null here: the C-ABI layer points them at its workspace when the caller
    // passes NULL -- three pointer tests less in a path that runs in nearly every iteration of the step loop)
    *at_offset(A.flags, idx) = (uint8_t)flags;
    const uint32_t o4 = idx * 4u;
    *at_offset(A.n_steps, o4) = n_att;
    *at_offset(A.n_accepted, o4) = n_acc;
}


// Work distribution.  One device-wide counter saturates near 90 fetches/us, and this kernel
// wants 50+/us at config 2; so the 64-ray batches are dealt into NSLICE interleaved slices
// (batch b belongs to slice b % NSLICE), each with its own counter on its own 256-byte line.  A
// wave starts on the slice blockIdx % NSLICE -- the blocks that share an XCD under round-robin
// placement, so a slice's counter is mostly touched from one XCD (speed only, never correctness)
// -- and moves on to the next slice when its own runs dry (work stealing), until all are dry.
constexpr int NSLICE = 8;
constexpr int SLICE_STRIDE = 32;  // in unsigned long long: 256 bytes

// Kernel arguments only the RARE paths of a trace kernel read -- the queue fill and the batch claim, once per 64 rays -- are
// fetched from the kernarg segment AT THOSE SITES (scalar loads of a few dwords) instead of living in SGPRs for the
// life of the kernel: the step loop is short of SGPRs (106 allocated, 14-18 spilled to VGPR lanes and fetched back with
// v_readlane in every iteration), and these are two dozen of them.  The empty asm makes the segment's address opaque at
// each use, so that the loads are neither hoisted out of the loop nor shared between sites.  (The trace kernels take
// the TraceArgs struct as their ONE argument: its fields sit at their offsetof in the segment.)
#define BHG_KERNARG_PTR __attribute__((address_space(4))) const char *
__device__ __forceinline__ BHG_KERNARG_PTR kernarg_base()
{
    BHG_KERNARG_PTR kp = (BHG_KERNARG_PTR)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return kp;
}
#define BHG_COLD(kp, field) (*(__attribute__((address_space(4))) const decltype(TraceArgs::field) *)((kp) + offsetof(TraceArgs, field)))

__device__ __forceinline__ unsigned long long issue_fetch(const TraceArgs &A, uint32_t lane, uint32_t slice)
{
    unsigned long long b = 0;
    unsigned long long *counter = BHG_COLD(kernarg_base(), counter);
    if (lane == 0) b = atomicAdd(counter + slice * SLICE_STRIDE, 1ull);
    return b;
}

// broadcast lane 0's fetched local batch id and turn it into a ray index
__device__ __forceinline__ uint64_t take_fetch(unsigned long long b, uint32_t slice)
{
    const uint64_t local = __builtin_amdgcn_readfirstlane((uint32_t)b) |
                           ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32);
    return (local * NSLICE + slice) * 64ull;
}

// f0 = a(x0, k0), r0 and, for DP5(4), scipy's initial step (select_initial_step, common.py:68-134, order = 4)
// for one ray that starts outside the hole.  Used converged: by all 64 lanes of a wave while it fills its ray queue, or by
// the lanes of a lane-per-ray kernel at its top (start_ray).
template <int RHS, bool ADAPTIVE>
__device__ __forceinline__ void initial_record(const TraceArgs &A, const Metric &met, const double px[3],
                                               const double pk[3], double pa[3], double &pr, double &ph)
{
    accel<RHS>(px, pk, met, pa, pr);
    if (ADAPTIVE) {
        const double rtol = A.rtol, atol = A.atol, t_bound = A.lambda_end;
        double isc[6];
        double d0 = 0.0, d1 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double sk = rcp_nr(__builtin_fma(fabs(pk[c]), rtol, atol));
            double sx = rcp_nr(__builtin_fma(fabs(px[c]), rtol, atol));
            isc[c] = sk;
            isc[3 + c] = sx;
            double y0k = pk[c] * sk, y0x = px[c] * sx;
            double f0k = pa[c] * sk, f0x = pk[c] * sx;
            d0 = __builtin_fma(y0k, y0k, __builtin_fma(y0x, y0x, d0));
            d1 = __builtin_fma(f0k, f0k, __builtin_fma(f0x, f0x, d1));
        }
        d0 = sqrt(d0 * (1.0 / 6.0));
        d1 = sqrt(d1 * (1.0 / 6.0));
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        h0 = fmin(h0, t_bound);
        double x1[3], k1[3], f1[3], r1;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x1[c] = __builtin_fma(h0, pk[c], px[c]);
            k1[c] = __builtin_fma(h0, pa[c], pk[c]);
        }
        accel<RHS>(x1, k1, met, f1, r1);
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double dk = (f1[c] - pa[c]) * isc[c];
            double dx = (k1[c] - pk[c]) * isc[3 + c];
            d2 = __builtin_fma(dk, dk, __builtin_fma(dx, dx, d2));
        }
        d2 = sqrt(d2 * (1.0 / 6.0)) / h0;
        double h1;
        if (d1 <= 1e-15 && d2 <= 1e-15) {
            h1 = fmax(1e-6, h0 * 1e-3);
        } else {
            double q = 0.01 / fmax(d1, d2);
            // the fast path needs a normal fp32 range; outside it (degenerate inputs) use libm
            h1 = (q > 1e-30 && q < 1e30) ? pow_0p2(q) : pow(q, 0.2);
        }
        ph = fmin(fmin(100.0 * h0, h1), fmin(t_bound, A.max_step));
        if (!(ph >= 0.0)) ph = 0.0;  // NaN input: let the step loop fail it (STEP_TOO_SMALL / NaN flag)
    }
}

// Put rays base .. base+63 into the ray queue: coalesced loads of k0, x0; the start records {a0, h0, r0, E, L} are
// worked out here, all lanes together.
// The initial step h0 (DP5(4) only) depends on the ray, the tolerances, lambda_end, max_step and the metric alone, so an owner
// of unchanged rays keeps it from call to call (TraceArgs::start_h, start_mode): a recording call stores each queued ray's h0,
// a replaying call loads it -- with k0, in front of the vmcnt(0) below -- and works out a0 and r0 only.  The branch is
// wave-uniform (a kernel argument); rays that start inside the hole are neither stored nor used.
// Items that pass (h >= 0) take a free slot each (ballot/mbcnt ranks); the caller has made sure 64 are free.
// The same owner may keep much more than h0: the ray's whole state after its first accepted steps, as long as those stay in a
// ball about the start point that no event surface reaches (TraceArgs::prefix, record_prefix_kernel below).
// Which kernels look at such records: DP5(4) with the two Cartesian null forms (96-byte states; Kerr's are Boyer-Lindquist
// with E and L, the time-like form and RK4 stay as they are).
template <int RHS, bool ADAPTIVE>
struct PrefixReplays {
    static constexpr bool value = ADAPTIVE && (RHS == BHG_RHS_CHRISTOFFEL_ || RHS == BHG_RHS_REDUCED_);
};
template <int RHS, bool ADAPTIVE, class LDS>
__device__ __forceinline__ void fill_batch(const TraceArgs &A, LDS &Q, Wave &W, uint32_t lane, uint64_t base)
{
    // (this function's arguments straight from the kernarg segment, see kernarg_base())
    BHG_KERNARG_PTR kp = kernarg_base();
    struct {
        const double *k0, *x0;
        uint64_t n;
        int8_t *object_id;
        double *start_h;
        int32_t start_mode;
    } C = {BHG_COLD(kp, k0), BHG_COLD(kp, x0), BHG_COLD(kp, n), BHG_COLD(kp, object_id), BHG_COLD(kp, start_h),
           BHG_COLD(kp, start_mode)};
    const bool replay = ADAPTIVE && C.start_mode == BHG_START_REPLAY_;
    const uint64_t i = base + lane;
    bool need = i < C.n;        // lanes whose ray is started here, from k0 and x0
    if (PrefixReplays<RHS, ADAPTIVE>::value) {
        // Start-up records (TraceArgs::prefix; record_prefix_kernel wrote them): a usable one is the ray's queue entry after its
        // first n_att attempts (a deep record: rejected ones among them, bit 0 of its last word set when the last one was) -- it
        // goes into the queue as it is, and only the lanes without one start their ray below (the whole start is skipped when
        // no lane of the batch needs it).  Wave-uniform on a kernel argument.
        const double2 *rec = BHG_COLD(kp, prefix);
        if (rec) {
            double2 rd[6];
            uint4 ri = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int p = 0; p < 6; p++) rd[p] = make_double2(0.0, 0.0);
            if (i < C.n) {
#pragma unroll
                for (int p = 0; p < 6; p++) rd[p] = rec[(uint64_t)p * C.n + i];
                ri = reinterpret_cast<const uint4 *>(rec)[6ull * C.n + i];
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only: see below
            const bool usable = i < C.n && ri.y != 0u;     // (y: attempts, z: accepted steps)
            const uint64_t umask = __ballot(usable);
            const int ucnt = __builtin_popcountll(umask);
            if (usable) {
                if (C.object_id) C.object_id[i] = (int8_t)-1;
                const uint32_t rk = lane_rank(umask);
                const uint32_t s = Q.free_list[W.n_free - 1 - (int)rk];
                SLOT_CHECK(Q, s, 0, 1, "fill");
                Q.q_list[(W.q_head + W.q_count + (int)rk) & (QRING - 1)] = (uint8_t)s;
                QEntry<RHS> &e = Q.slot[s];
#pragma unroll
                for (int p = 0; p < 6; p++) e.d[p] = rd[p];
                e.i = make_uint4((uint32_t)i, ri.y, ri.z, ri.w);
            }
            W.n_free -= ucnt;
            W.q_count += ucnt;
            need = need && !usable;
            if (__ballot(need) == 0ull) {
                wave_lds_sync();
                INV_CHECK(W, "fill");
                return;
            }
        }
    }
    double hs = 0.0;
    double px[3] = {0, 0, 0}, pk[3] = {0, 0, 0}, pa[3] = {0, 0, 0}, pr = 0.0, ph = -1.0;
    double pE = 0.0, pL = 0.0;
    if (need) {
        pk[0] = C.k0[i * 3 + 0];
        pk[1] = C.k0[i * 3 + 1];
        pk[2] = C.k0[i * 3 + 2];
        if (replay) hs = C.start_h[i];
        if (C.x0) {
            px[0] = C.x0[i * 3 + 0];
            px[1] = C.x0[i * 3 + 1];
            px[2] = C.x0[i * 3 + 2];
        } else {
            const __attribute__((address_space(4))) double *xs = (const __attribute__((address_space(4))) double *)(kp + offsetof(TraceArgs, x0s));
            px[0] = xs[0];
            px[1] = xs[1];
            px[2] = xs[2];
        }
    }
    // All of this batch's loads must have landed HERE, for every lane: otherwise the compiler has
    // to assume they may still be in flight on the not-valid path and puts a vmcnt(0) in front of
    // the step code, which then waits for the previous iteration's result stores every iteration.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
    if (need) {
        if (C.object_id) C.object_id[i] = (int8_t)-1;
        Metric met;
        met.r_s = A.r_s;
        met.M = 0.5 * A.r_s;
        met.a = met.E = met.L = 0.0;
        const double cx[3] = {px[0], px[1], px[2]}, ck[3] = {pk[0], pk[1], pk[2]};   // the Cartesian input, for a start inside
        double r0;
        if (RHS == BHG_RHS_KERR_BL_) {
            met.a = A.spin;
            kerr_cart_to_bl(met.a, met.M, A.mu2, px, pk, met.E, met.L);
            pE = met.E;
            pL = met.L;
            r0 = px[0];
        } else {
            r0 = sqrt(__builtin_fma(px[2], px[2], __builtin_fma(px[1], px[1], px[0] * px[0])));
        }
        if (r0 <= A.r_hor) {
            // 'start_inside_hole' (RelativisticRenderEngine.py:296, :311-313): final at once, never queued
            store_result(A, (uint32_t)i, cx, ck, BHG_FLAG_START_INSIDE_ | BHG_FLAG_HIT_HORIZON_, 0, 0);
        } else {
            ph = 0.0;
            if (replay) {
                initial_record<RHS, false>(A, met, px, pk, pa, pr, ph);
                ph = hs >= 0.0 ? hs : 0.0;   // (a recorded step is >= 0; anything else fails in the step loop like NaN input)
            } else {
                initial_record<RHS, ADAPTIVE>(A, met, px, pk, pa, pr, ph);
                if (ADAPTIVE && C.start_mode == BHG_START_RECORD_) C.start_h[i] = ph;
            }
        }
    }
    const bool valid = ph >= 0.0;
    const uint64_t vmask = __ballot(valid);
    const int cnt = __builtin_popcountll(vmask);
    if (valid) {
        const uint32_t rk = lane_rank(vmask);
        const uint32_t s = Q.free_list[W.n_free - 1 - (int)rk];
        SLOT_CHECK(Q, s, 0, 1, "fill");
        Q.q_list[(W.q_head + W.q_count + (int)rk) & (QRING - 1)] = (uint8_t)s;
        entry_put<RHS>(Q.slot[s], px, pk, pa, ph, pr, 0.0, pE, pL, (uint32_t)i, 0u, 0u, 0u);
    }
    wave_lds_sync();
    W.n_free -= cnt;
    W.q_count += cnt;
    INV_CHECK(W, "fill");
}

// ------------------------------------------------------------------------------------------
// One Dormand-Prince step in Nystrom form: stages 2..7 from (x, v, a1, h).
// Used by the integrate loop AND by the event drain, so both see bit-identical stage values
// (the library is built with -ffp-contract=off; every FMA below is explicit).
// ------------------------------------------------------------------------------------------
template <int RHS>
__device__ __forceinline__ void dp54_stages(const double x[3], const double v[3], const double a1[3], double h,
                                            const Metric &r_s, double a2[3], double a3[3], double a4[3], double a5[3],
                                            double a6[3], double a7[3], double xn[3], double vn[3], double &r_new)
{
    const double h2 = h * h;
    double xs[3], vs[3], rs_;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        vs[c] = __builtin_fma(h * TB.a[2][1], a1[c], v[c]);
        xs[c] = __builtin_fma(h * TB.c[2], v[c], x[c]);
    }
    accel<RHS>(xs, vs, r_s, a2, rs_);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sv = __builtin_fma(TB.a[3][2], a2[c], TB.a[3][1] * a1[c]);
        vs[c] = __builtin_fma(h, sv, v[c]);
        double sx = TB.at[3][1] * a1[c];
        xs[c] = __builtin_fma(h2, sx, __builtin_fma(h * TB.c[3], v[c], x[c]));
    }
    accel<RHS>(xs, vs, r_s, a3, rs_);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sv = __builtin_fma(TB.a[4][3], a3[c], __builtin_fma(TB.a[4][2], a2[c], TB.a[4][1] * a1[c]));
        vs[c] = __builtin_fma(h, sv, v[c]);
        double sx = __builtin_fma(TB.at[4][2], a2[c], TB.at[4][1] * a1[c]);
        xs[c] = __builtin_fma(h2, sx, __builtin_fma(h * TB.c[4], v[c], x[c]));
    }
    accel<RHS>(xs, vs, r_s, a4, rs_);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sv = __builtin_fma(
            TB.a[5][4], a4[c],
            __builtin_fma(TB.a[5][3], a3[c], __builtin_fma(TB.a[5][2], a2[c], TB.a[5][1] * a1[c])));
        vs[c] = __builtin_fma(h, sv, v[c]);
        double sx = __builtin_fma(TB.at[5][3], a3[c], __builtin_fma(TB.at[5][2], a2[c], TB.at[5][1] * a1[c]));
        xs[c] = __builtin_fma(h2, sx, __builtin_fma(h * TB.c[5], v[c], x[c]));
    }
    accel<RHS>(xs, vs, r_s, a5, rs_);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sv = __builtin_fma(
            TB.a[6][5], a5[c],
            __builtin_fma(TB.a[6][4], a4[c],
                          __builtin_fma(TB.a[6][3], a3[c], __builtin_fma(TB.a[6][2], a2[c], TB.a[6][1] * a1[c]))));
        vs[c] = __builtin_fma(h, sv, v[c]);
        double sx = __builtin_fma(
            TB.at[6][4], a4[c],
            __builtin_fma(TB.at[6][3], a3[c], __builtin_fma(TB.at[6][2], a2[c], TB.at[6][1] * a1[c])));
        xs[c] = __builtin_fma(h2, sx, __builtin_fma(h * TB.c[6], v[c], x[c]));
    }
    accel<RHS>(xs, vs, r_s, a6, rs_);
    // new solution (stage 7 = FSAL; b_2 = 0)
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sv = __builtin_fma(
            TB.a[7][6], a6[c],
            __builtin_fma(TB.a[7][5], a5[c],
                          __builtin_fma(TB.a[7][4], a4[c], __builtin_fma(TB.a[7][3], a3[c], TB.a[7][1] * a1[c]))));
        vn[c] = __builtin_fma(h, sv, v[c]);
        double sx = __builtin_fma(
            TB.at[7][5], a5[c],
            __builtin_fma(TB.at[7][4], a4[c],
                          __builtin_fma(TB.at[7][3], a3[c], __builtin_fma(TB.at[7][2], a2[c], TB.at[7][1] * a1[c]))));
        xn[c] = __builtin_fma(h2, sx, __builtin_fma(h, v[c], x[c]));
    }
    accel<RHS>(xn, vn, r_s, a7, r_new);
}


// Squared RMS error norm of one DP5(4) step (rk.py:105-109, :143-146) over the 6 components.  The six
// scale reciprocals come from ONE v_rcp_f64 (batch inversion: prefix products, one reciprocal,
// back-substitution) -- the transcendental pipe is the scarce one; h and h^2 are factored out of the sums.
__device__ __forceinline__ double dp54_errsq(const double x[3], const double v[3], const double xn[3],
                                             const double vn[3], const double a1[3], const double a2[3],
                                             const double a3[3], const double a4[3], const double a5[3],
                                             const double a6[3], const double a7[3], double h, double rtol, double atol)
{
    const double h2 = h * h;
    double evr[3], exr[3], sc[6];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        evr[c] = __builtin_fma(
            TB.e[7], a7[c],
            __builtin_fma(TB.e[6], a6[c],
                          __builtin_fma(TB.e[5], a5[c],
                                        __builtin_fma(TB.e[4], a4[c], __builtin_fma(TB.e[3], a3[c], TB.e[1] * a1[c])))));
        exr[c] = __builtin_fma(
            TB.et[6], a6[c],
            __builtin_fma(TB.et[5], a5[c],
                          __builtin_fma(TB.et[4], a4[c],
                                        __builtin_fma(TB.et[3], a3[c], __builtin_fma(TB.et[2], a2[c], TB.et[1] * a1[c])))));
        sc[c] = __builtin_fma(fmax(fabs(v[c]), fabs(vn[c])), rtol, atol);
        sc[3 + c] = __builtin_fma(fmax(fabs(x[c]), fabs(xn[c])), rtol, atol);
    }
    double isc[6];
    {
        const double p1 = sc[0] * sc[1], p2 = p1 * sc[2], p3 = p2 * sc[3], p4 = p3 * sc[4], p5 = p4 * sc[5];
        if (p5 > 1e-250) {
            double inv = rcp_nr(p5);
            isc[5] = inv * p4;
            inv *= sc[5];
            isc[4] = inv * p3;
            inv *= sc[4];
            isc[3] = inv * p2;
            inv *= sc[3];
            isc[2] = inv * p1;
            inv *= sc[2];
            isc[1] = inv * sc[0];
            isc[0] = inv * sc[1];
        } else {  // absurdly small tolerances (or NaN): no product, six reciprocals
#pragma unroll
            for (int c = 0; c < 6; c++) isc[c] = rcp_nr(sc[c]);
        }
    }
    double sv = 0.0, sx = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double qv = evr[c] * isc[c];
        const double qx = exr[c] * isc[3 + c];
        sv = __builtin_fma(qv, qv, sv);
        sx = __builtin_fma(qx, qx, sx);
    }
    return __builtin_fma(sx, h2, sv) * (h2 * (1.0 / 6.0));
}

// 0.9 * err^(-1/5) = 0.9 * errsq^(-1/10) before the [0.2, 10] clamps of rk.py:148-163.  The clamps make
// the result independent of errsq outside [0.09^10, 4.5^10] = [3.5e-11, 3.41e6]; the fast power is
// evaluated on the wider [1e-11, 1e7] so both clamp points lie inside.  NaN -> 0.2 (python max(0.2, nan)).
__device__ __forceinline__ double dp54_factor(double errsq)
{
    return (errsq < 1e7) ? 0.9 * pow_m0p1(fmax(errsq, 1e-11)) : 0.2;
}

// The terminal event of one accepted step, if it holds one: of the candidates the earliest root wins
// (handle_events sorts the roots, ivp.py:111-122; ties keep the order horizon, exit, disk, sphere 0, 1, ...).
// Horizon and sphere exit always end the ray; a disk-plane crossing only inside the annulus
// R_in <= R <= R_out (LimitedRelativisticRenderEngine.py:423-424); an object sphere when the curve enters
// it (the reference's collision stub, RelativisticRenderEngine.py:304-305).
// g_r(t, R) = r(t) - R, g_z(t) = z(t), pos(t, x) = interpolated position.  Returns the flag of the event that ends
// the ray (0: none does) with its root in `best` and, for an object hit, the sphere in `obj`.
// The general search: Brent on the interpolant, scipy's solve_event_equation step for step.  Steps whose one event
// function is provably monotone over the step never come here (dp54_resolve_parked's certified Newton search).
template <int EVT, class GR, class GZ, class POS>
__device__ __forceinline__ uint32_t settle_events(const TraceArgs &A, uint32_t kind, double t, double t_new,
                                                  const double x0[3], const double x1[3], const GR &g_r, const GZ &g_z,
                                                  const POS &pos, bool bl, double &best, int &obj)
{
    best = __builtin_inf();
    uint32_t fl = 0;
    obj = -1;
    if (kind & EV_HORIZON) {
        const double r = brent_root([&](double tt) { return g_r(tt, A.r_hor); }, t, t_new);
        if (r < best) {
            best = r;
            fl = BHG_FLAG_HIT_HORIZON_;
        }
    }
    // (event kinds the kernel variant was not compiled for cannot be set: the tests fold away)
    if ((EVT & EVT_EXIT) && (kind & EV_EXIT)) {
        const double r = brent_root([&](double tt) { return g_r(tt, A.r_exit); }, t, t_new);
        if (r < best) {
            best = r;
            fl = BHG_FLAG_EXITED_SPHERE_;
        }
    }
    if ((EVT & EVT_DISK) && (kind & EV_DISK)) {
        const double r = brent_root([&](double tt) { return g_z(tt); }, t, t_new);
        double xe[3];
        pos(r, xe);
        const double R = disk_radius(A, xe, bl);
        if (R >= A.disk_r_in && R <= A.disk_r_out && r < best) {
            best = r;
            fl = BHG_FLAG_HIT_DISK_;
        }
    }
    if ((EVT & EVT_OBJ) && (kind & EV_OBJ)) {
        // (Boyer-Lindquist steps: the spheres are met in the Cartesian frame -- chord rule on the images of the step's
        // ends, distance function on the image of the interpolated position)
        double c0[3] = {x0[0], x0[1], x0[2]}, c1[3] = {x1[0], x1[1], x1[2]};
        if (bl) {
            bl_position_to_cart(A.spin, x0, c0);
            bl_position_to_cart(A.spin, x1, c1);
        }
        for (int j = 0; j < A.n_spheres; j++) {
            const double *sp = A.spheres[j];
            double bb, cc;
            bool inside;
            if (!sphere_candidate(sp, c0, c1, bb, cc, inside)) continue;
            auto g_s = [&](double tt) {
                double xe[3];
                pos(tt, xe);
                if (bl) {
                    const double q[3] = {xe[0], xe[1], xe[2]};
                    bl_position_to_cart(A.spin, q, xe);
                }
                const double dx = xe[0] - sp[0], dy = xe[1] - sp[1], dz = xe[2] - sp[2];
                return sqrt_nr(dx * dx + dy * dy + dz * dz) - sp[3];
            };
            double hi = t_new;
            if (!inside) {
                hi = t + (bb / cc) * (t_new - t);
                if (!(g_s(hi) < 0.0)) continue;  // the curve itself stays outside there: no hit
            }
            const double r = brent_root(g_s, t, hi);
            if (r < best) {
                best = r;
                fl = BHG_FLAG_HIT_OBJECT_;
                obj = j;
            }
        }
    }
    return fl;
}

// The quartic dense output of one accepted DP5(4) step from its stage accelerations (rk.py:393-404, :552-574 in
// Nystrom form), position part: x_c(th) = x_c + (h th) (qx[0][c] + th (qx[1][c] + th (qx[2][c] + th qx[3][c]))),
// qx[0] = v.  One definition for the event drain and the sampled-trajectory kernel: both see the same bits.
__device__ __forceinline__ void build_dense_pos(Dense &d, double t, double h, const double x[3], const double v[3],
                                                const double a1[3], const double a2[3], const double a3[3],
                                                const double a4[3], const double a5[3], const double a6[3],
                                                const double a7[3])
{
    d.t0 = t;
    d.h = h;
    d.ih = rcp_nr(h);
    const double *aj[8] = {nullptr, a1, a2, a3, a4, a5, a6, a7};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d.x0[c] = x[c];
        d.v0[c] = v[c];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            // sum_j P~[j][m] a_j as an FMA chain; coefficients that are zero (known at compile time: the whole
            // m = 0 column, P~[7][.]) are skipped
            double qx = 0.0;
#pragma unroll
            for (int j = 1; j <= 7; j++)
                if (TB.pt[j][m] != 0.0) qx = __builtin_fma(TB.pt[j][m], aj[j][c], qx);
            d.qx[m][c] = __builtin_fma(h, qx, TB.sig[m] * v[c]);
        }
    }
}

// ... and its direction part: v_c(th) = v_c + (h th) (qv[0][c] + th (qv[1][c] + ...)), qv[m] = sum_j P[j][m] a_j
__device__ __forceinline__ void build_dense_dir(Dense &d, const double a1[3], const double a2[3], const double a3[3],
                                                const double a4[3], const double a5[3], const double a6[3],
                                                const double a7[3])
{
    const double *aj[8] = {nullptr, a1, a2, a3, a4, a5, a6, a7};
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int m = 0; m < 4; m++) {
            double qv = 0.0;
#pragma unroll
            for (int j = 1; j <= 7; j++)
                if (TB.p[j][m] != 0.0) qv = __builtin_fma(TB.p[j][m], aj[j][c], qv);
            d.qv[m][c] = qv;
        }
}

__device__ __forceinline__ void build_dense(Dense &d, double t, double h, const double x[3], const double v[3],
                                            const double a1[3], const double a2[3], const double a3[3], const double a4[3],
                                            const double a5[3], const double a6[3], const double a7[3])
{
    build_dense_pos(d, t, h, x, v, a1, a2, a3, a4, a5, a6, a7);
    build_dense_dir(d, a1, a2, a3, a4, a5, a6, a7);
}

// The direction of the dense output at ONE parameter th, straight from the stage accelerations:
// v_c(th) = v_c + (h th) sum_j a_j[c] b_j(th), b_j(th) = sum_m P[j][m] th^m -- the same polynomial as dense_dir's,
// summed stage-first (six scalar cubics + 18 FMAs instead of twelve coefficients of 6 FMAs each + 15): what a step
// needs whose event root is already known.  Agrees with dense_dir to rounding.
__device__ __forceinline__ void dense_dir_at(double th, double h, const double v[3], const double a1[3],
                                             const double a3[3], const double a4[3], const double a5[3],
                                             const double a6[3], const double a7[3], double out[3])
{
    double b[8];
#pragma unroll
    for (int j = 1; j <= 7; j++)
        b[j] = __builtin_fma(__builtin_fma(__builtin_fma(TB.p[j][3], th, TB.p[j][2]), th, TB.p[j][1]), th, TB.p[j][0]);
    const double hth = h * th;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double sacc = b[1] * a1[c];     // (P[2][.] = 0)
        sacc = __builtin_fma(b[3], a3[c], sacc);
        sacc = __builtin_fma(b[4], a4[c], sacc);
        sacc = __builtin_fma(b[5], a5[c], sacc);
        sacc = __builtin_fma(b[6], a6[c], sacc);
        sacc = __builtin_fma(b[7], a7[c], sacc);
        out[c] = __builtin_fma(hth, sacc, v[c]);
    }
}

// ------------------------------------------------------------------------------------------
// One parked DP5(4) step, resolved by a lane of the event drain: recompute the step from its start state
// (bit-identical stages), locate its event, write the ray's result -- or hand the ray back to carry on.
//
// P (in): the parked record -- x, v, a1, t at the step's start, h_abs = the controller's |h| for the NEXT step,
//         r_cur = the |h| THIS step tried, idx and the step counts after the step.
// R (out, when true is returned): the ray's state at the step's end; it carries on from there.
//
// Root search.  solve_ivp locates an event with brentq on the dense output to 4 eps (ivp.py:51-76).  Where the step
// holds exactly ONE candidate event of a monotone kind (exit sphere or disk plane) and its event function is provably MONOTONE
// over the whole step, the root is unique and any bracketing search that converges to that tolerance returns it:
// such lanes run a safeguarded Newton iteration on the polynomial itself (exact derivative, no square root: r^2 - R^2
// in place of r - R), 3 iterations where Brent takes 7 or 8 of twice the length, the position half of the dense
// output only, and the direction evaluated once at the root.  The certificate is a sufficient condition from the
// coefficients: with x(th) = x + h th (v + e(th)), x'(th) = h (v + d(th)), |e_c| <= E_c = |q1| + |q2| + |q3| and
// |d_c| <= D_c = 2|q1| + 3|q2| + 4|q3| on [0, 1]:
//     plane:   |v_z| > D_z                                           (z' keeps its sign)
//     sphere:  x.x'/h = x.v + h th |v|^2 + [x.d + h th (e.v + v.d + e.d)], bracket bounded by
//              S = sum_c |x_c| D_c + h (|v_c| (E_c + D_c) + E_c D_c);  outward (the exit sphere): x.v > S
//     Boyer-Lindquist: the event functions are single coordinates (r, theta): |u_c| > D_c.
// Everything else -- several candidates in one step, object spheres, a failed certificate (a step diving through the
// horizon with the Christoffel form's 1/f terms: round 2 found dense outputs with several crossings there, and
// which one brentq lands on is part of the contract) -- goes through Brent, step for step as before.
// ------------------------------------------------------------------------------------------
// Outcome of a parked step
constexpr int PARK_ENDED = 0, PARK_RESUME = 1, PARK_UNCERTIFIED = 2, PARK_REQUEUE = 3;

// The short search itself, on a step whose stages are at hand: x, v, a1, t = the step's start, h = its signed length, t_new its
// end, a2..a7 / xn / vn / r_new its stages and end state, h_next the controller's |h| for the step after it.  Called by the
// drain, which recomputes the stages from the parked record, bit for bit (calling it from the step loop with the stages still
// in registers was measured and not kept: DESIGN section 4.1, row (e)).  PARK_ENDED: the ray's result is stored.
// PARK_RESUME: no terminal event, the ray carries on from the step's end (the caller takes xn, vn, a7, t_new, r_new).
// PARK_UNCERTIFIED: nothing touched.
template <int RHS, int EVT>
__device__ __forceinline__ int dp54_short_core(const TraceArgs &A, const double x[3], const double v[3], const double a1[3], double t,
                                               double t_new, double h, const double a2[3], const double a3[3], const double a4[3],
                                               const double a5[3], const double a6[3], const double a7[3], const double xn[3],
                                               const double vn[3], uint32_t kind, uint32_t idx, uint32_t n_att, uint32_t n_acc)
{
    constexpr bool BL = RHS == BHG_RHS_KERR_BL_;
    Dense d;
    build_dense_pos(d, t, h, x, v, a1, a2, a3, a4, a5, a6, a7);

    const bool is_disk = (EVT & EVT_DISK) && kind == EV_DISK;
    double Ec[3], Dc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double q1 = fabs(d.qx[1][c]), q2 = fabs(d.qx[2][c]), q3 = fabs(d.qx[3][c]);
        Ec[c] = q1 + q2 + q3;
        Dc[c] = __builtin_fma(4.0, q3, __builtin_fma(3.0, q2, 2.0 * q1));
    }
    bool mono;
    int comp = 0;               // Boyer-Lindquist: the coordinate the event function is
    double target = 0.0;        // BL: its value on the event surface;  Cartesian spheres: R^2
    if (BL) {
        comp = is_disk ? 1 : 0;
        if (is_disk) {
            // the plane theta* = pi/2 + k pi between the step ends (more than one: Brent decides)
            const double k0 = floor((x[1] - 1.5707963267948966) * 0.3183098861837907);
            const double k1 = floor((xn[1] - 1.5707963267948966) * 0.3183098861837907);
            target = __builtin_fma(3.141592653589793, fmax(k0, k1), 1.5707963267948966);
            mono = fabs(k1 - k0) == 1.0 && fabs(v[1]) > 1.0000001 * Dc[1];
        } else {
            target = A.r_exit;
            mono = v[0] > 1.0000001 * Dc[0];
        }
    } else if (is_disk) {
        mono = fabs(v[2]) > 1.0000001 * Dc[2];
    } else {
        target = A.r_exit * A.r_exit;
        double xv = 0.0, S = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            xv = __builtin_fma(x[c], v[c], xv);
            const double av = fabs(v[c]);
            S = __builtin_fma(fabs(x[c]), Dc[c], S);
            S = __builtin_fma(h, __builtin_fma(av, Ec[c] + Dc[c], Ec[c] * Dc[c]), S);
        }
        S *= 1.0000001;
        mono = xv > S;       // (outward crossing)
    }
    // G(th) and dG/dth on the position polynomial
    auto eval = [&](double th, double &g, double &dg, double xs[3]) {
        double ds[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double sx = __builtin_fma(d.qx[3][c], th, d.qx[2][c]);
            sx = __builtin_fma(sx, th, d.qx[1][c]);
            sx = __builtin_fma(sx, th, d.qx[0][c]);
            xs[c] = __builtin_fma(h * th, sx, d.x0[c]);     // = dense_pos
            double sd = __builtin_fma(4.0 * d.qx[3][c], th, 3.0 * d.qx[2][c]);
            sd = __builtin_fma(sd, th, 2.0 * d.qx[1][c]);
            sd = __builtin_fma(sd, th, d.qx[0][c]);
            ds[c] = h * sd;
        }
        if (BL) {
            g = (comp == 1 ? xs[1] : xs[0]) - target;
            dg = comp == 1 ? ds[1] : ds[0];
        } else if (is_disk) {
            g = xs[2];
            dg = ds[2];
        } else {
            g = __builtin_fma(xs[2], xs[2], __builtin_fma(xs[1], xs[1], xs[0] * xs[0])) - target;
            dg = 2.0 * __builtin_fma(xs[2], ds[2], __builtin_fma(xs[1], ds[1], xs[0] * ds[0]));
        }
    };
    // the event function at the step's ends, from the end states themselves (the polynomial returns them to rounding)
    auto gfun = [&](const double xs_[3]) {
        if (BL) return (comp == 1 ? xs_[1] : xs_[0]) - target;
        if (is_disk) return xs_[2];
        return __builtin_fma(xs_[2], xs_[2], __builtin_fma(xs_[1], xs_[1], xs_[0] * xs_[0])) - target;
    };
    const double g0 = gfun(x), g1 = gfun(xn);
    double dg, xs[3];
    // the step ends bracket the root (that is what parked the step); G is monotone between them
    double lo = 0.0, hi = 1.0;
    const bool neg0 = g0 < 0.0;
    double th = g0 * rcp_nr(g0 - g1);      // secant start
    if (!(th > 0.0 && th < 1.0)) th = 0.5;
    if (g0 == 0.0) th = 0.0;        // (an end exactly on the surface is the root, as in brentq)
    else if (g1 == 0.0) th = 1.0;
    // FOUR safeguarded Newton steps for every lane, no per-lane exit: from the secant start the error squares
    // each time (1e-2, 1e-4, 1e-8, 1e-16 is typical), a lane that is there early repeats a step of ~0.  The
    // root counts as found when the LAST step moved th by less than 1e-9 (the error left is then far below an
    // ulp); anything slower -- a root next to an end of the bracket, a bisection on the way -- goes to Brent.
    double dth = 1.0;
#pragma unroll 1
    for (int it = 0; it < 4; it++) {
        double g;
        eval(th, g, dg, xs);
        if ((g < 0.0) == neg0) lo = th; else hi = th;
        dth = -g * rcp_nr(dg);
        double thn = th + dth;
        if (!(thn >= lo && thn <= hi)) {      // Newton left the bracket (or NaN): bisect
            thn = 0.5 * (lo + hi);
            dth = 1.0;
        }
        th = thn;
    }
    if (!(mono && fabs(dth) <= 1e-9)) return PARK_UNCERTIFIED;

    double g, xe[3], ve[3];
    eval(th, g, dg, xe);        // xe = position at the root
    bool terminal = true;
    if (is_disk) {
        const double Rc = disk_radius(A, xe, BL);
        terminal = Rc >= A.disk_r_in && Rc <= A.disk_r_out;
    }
    if (terminal) {
        dense_dir_at(th, h, v, a1, a3, a4, a5, a6, a7, ve);
        const uint32_t fl = is_disk ? BHG_FLAG_HIT_DISK_ : BHG_FLAG_EXITED_SPHERE_;
        store_result(A, idx, xe, ve, fl, n_att, n_acc);
        return PARK_ENDED;
    }
    // a disk-plane crossing outside the annulus: the ray is final if the step reached lambda_end (base.py:203-204),
    // otherwise it carries on from the step's end
    if (t_new - A.lambda_end >= 0.0) {
        store_result(A, idx, xn, vn, BHG_FLAG_REACHED_END_, n_att, n_acc);
        return PARK_ENDED;
    }
    return PARK_RESUME;
}

// The SHORT way: one candidate event -- exit sphere or disk plane; a horizon crossing never comes here (short_kind()) --
// whose event function is certified monotone over the step.  Returns PARK_UNCERTIFIED without having touched anything
// when the certificate (or the iteration) fails: the step then goes to the long list.
//
// The same function also runs steps AHEAD of the loop (kind == EV_AHEAD): P is then a queue-style record --
// x, v, a1, t at the step's start, h_abs = the |h| the controller chose for it, r_cur = the radius there, the step counts
// before it -- of a ray whose last step was ACCEPTED, and this is one whole pass of the step loop's body on it, operation
// for operation: clamp, stages (the ONE stage computation both kinds of record share: a drain usually holds both), error
// norm, factor, accept / reject, event tests, disk pre-filter -- and then the short search if the step holds one short event.
//   PARK_ENDED        the ray's result is stored (exit / disk located, or lambda_end reached);
//   PARK_RESUME       the ray carries on through the queue from the step's end (accepted, no terminal event): R;
//   PARK_REQUEUE      the ray goes back into the queue from the step's START -- P itself is the queue entry, kind its bits
//                     (EV_REQUEUE | rejected): with the reduced step after a rejection, or unchanged where one of the step prologue's rare cases applies
//                     (step budget, step-size floor: the loop's own code deals with those).  (From P, not through R: a second
//                     source for R behind the stages costs the disk variants 100 B of scratch per lane -- measured, round 6);
//   PARK_UNCERTIFIED  the step holds what the short search does not take (horizon, object spheres, several candidates, a
//                     failed certificate): P has become the ordinary parked record of that step, kind its event bits.
template <int RHS, int EVT>
__device__ __forceinline__ int dp54_resolve_short(const TraceArgs &A, const Metric &m, Lane &P, uint32_t &kind, Lane &R)
{
    const double t = P.t;
    double h_next = P.h_abs, h_try = P.r_cur;
    const bool ahead = RunsAhead<RHS, EVT>::value && kind == EV_AHEAD;
    if (ahead) {
        // (the prologue's rare cases, trace_dp54_kernel: left to the loop -- the ray goes back as it came)
        if (!(P.h_abs > A.min_step_cap) || P.n_att >= A.max_steps) {
            kind = EV_REQUEUE;
            return PARK_REQUEUE;
        }
        h_try = P.h_abs;
        if (h_try > A.max_step) h_try = A.max_step;    // rk.py:121-124, not after a rejection (this step follows an accepted one)
    }
    // the step as the integrate loop took it (takes it): same operations on the same bits
    double t_new = t + h_try;
    if (t_new - A.lambda_end > 0.0) t_new = A.lambda_end;
    const double h = t_new - t;
    double a2[3], a3[3], a4[3], a5[3], a6[3], a7[3], xn[3], vn[3], r_new;
    dp54_stages<RHS>(P.x, P.v, P.a1, h, m, a2, a3, a4, a5, a6, a7, xn, vn, r_new);
    uint32_t ck = kind;         // what the short search is asked to locate
    bool search = true;
    if (ahead) {
        // (phase by phase, with scheduling barriers in between: left to itself the compiler overlaps the disk pre-filter, the
        // error norm and the search's polynomial and spills 150 B per lane -- some of it on the paths INTO the step loop)
        __builtin_amdgcn_sched_barrier(0);
        // the loop's event tests (trace_dp54_kernel), on the same quantities -- evaluated before the error norm here (they
        // only count if the step is accepted; their values do not depend on the order)
        const bool ev_h = r_new <= A.r_hor;
        const bool ev_e = (P.r_cur - A.r_exit <= 0.0) && (r_new - A.r_exit >= 0.0);
        bool ev_d = (EVT & EVT_DISK) && (!(EVT & EVT_OBJ) || A.disk_r_out > 0.0) && crossed_disk_plane<RHS>(P.x, xn);
        const bool ev_o = (EVT & EVT_OBJ) && any_sphere_candidate_of<RHS>(A, P.x, xn);
        if ((EVT & EVT_DISK) && ev_d &&
            !(RHS == BHG_RHS_KERR_BL_ ? disk_crossing_may_hit_bl<true>(A, P.x, P.v, xn, vn, h, P.a1, a2, a3, a4, a5, a6)
                                      : disk_crossing_may_hit<true>(A, P.x, P.v, xn, vn, h, P.a1, a2, a3, a4, a5, a6)))
            ev_d = false;
        if (RHS == BHG_RHS_KERR_BL_ && (EVT & EVT_DISK) && ev_d &&
            !disk_crossing_may_hit_sharp<RHS>(A, P.x, P.v, xn, vn, h, P.a1, a2, a3, a4, a5, a6))
            ev_d = false;
        __builtin_amdgcn_sched_barrier(0);
        const double h_abs = fabs(h);
        P.n_att++;
        const double errsq = dp54_errsq(P.x, P.v, xn, vn, P.a1, a2, a3, a4, a5, a6, a7, h, A.rtol, A.atol);
        double fac = dp54_factor(errsq);
        __builtin_amdgcn_sched_barrier(0);
        if (!(errsq < 1.0)) {
            P.h_abs = h_abs * fmax(0.2, fac);           // (P: the start state, the radius there, the counts with this attempt)
            kind = EV_REQUEUE | 1u;                     // (the queue entry's bits: bit 0 = the last attempt was rejected)
            return PARK_REQUEUE;
        }
        fac = fmin(fac, 10.0);
        h_next = h_abs * fac;
        P.n_acc++;
        ck = (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u) | (ev_d ? EV_DISK : 0u) | (ev_o ? EV_OBJ : 0u);
        if (ck == 0u) {
            if (t_new - A.lambda_end >= 0.0) {           // base.py:203-204
                store_result<false>(A, P.idx, xn, vn, BHG_FLAG_REACHED_END_, P.n_att, P.n_acc);
                return PARK_ENDED;
            }
            search = false;                             // no event: the ray carries on from the step's end
        } else if (!(ck == EV_EXIT || ((EVT & EVT_DISK) && ck == EV_DISK))) {
            // the ordinary parked record of this step: start state, |h| for the NEXT step, the |h| this one tried (Lane::pend)
            P.h_abs = h_next;
            P.r_cur = h_try;
            kind = ck;
            return PARK_UNCERTIFIED;
        }
    }
    if (search) {
        const int outcome = dp54_short_core<RHS, EVT>(A, P.x, P.v, P.a1, t, t_new, h, a2, a3, a4, a5, a6, a7, xn, vn, ck, P.idx, P.n_att, P.n_acc);
        if (outcome == PARK_UNCERTIFIED && ahead) {
            P.h_abs = h_next;
            P.r_cur = h_try;
            kind = ck;
        }
        if (outcome != PARK_RESUME) return outcome;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        R.x[c] = xn[c];
        R.v[c] = vn[c];
        R.a1[c] = a7[c];
    }
    R.t = t_new;
    R.h_abs = h_next;
    R.r_cur = r_new;
    return PARK_RESUME;
}

// The LONG way, for everything else -- several candidates in one step, object spheres, the horizon (a step diving
// through it with the Christoffel form's 1/f terms has a dense output of large curvature: its certificate practically
// never holds, and round 2 found dense outputs with several crossings there: which one brentq lands on is part of the
// contract), a failed certificate: Brent on the full dense output, scipy's search step for step.
template <int RHS, int EVT>
__device__ __forceinline__ int dp54_resolve_long(const TraceArgs &A, const Metric &m, const Lane &P, uint32_t kind, Lane &R)
{
    constexpr bool BL = RHS == BHG_RHS_KERR_BL_;
    const double t = P.t, h_next = P.h_abs;
    double t_new = t + P.r_cur;
    if (t_new - A.lambda_end > 0.0) t_new = A.lambda_end;
    const double h = t_new - t;
    double a2[3], a3[3], a4[3], a5[3], a6[3], a7[3], xn[3], vn[3], r_new;
    dp54_stages<RHS>(P.x, P.v, P.a1, h, m, a2, a3, a4, a5, a6, a7, xn, vn, r_new);
    Dense d;
    build_dense(d, t, h, P.x, P.v, P.a1, a2, a3, a4, a5, a6, a7);
    double best;
    int obj;
    const uint32_t fl = settle_events<EVT>(
        A, kind, t, t_new, P.x, xn, [&](double tt, double Rr) { return dense_g(d, tt, Rr, BL); },
        [&](double tt) { return dense_plane_g(d, tt, BL); },
        [&](double tt, double xq[3]) { dense_pos(d, tt, xq); }, BL, best, obj);
    if (fl) {
        double xe[3], ve[3];
        dense_pos(d, best, xe);
        dense_dir(d, best, ve);
        store_result(A, P.idx, xe, ve, fl, P.n_att, P.n_acc);
        if (obj >= 0 && A.object_id) A.object_id[P.idx] = (int8_t)obj;
        return PARK_ENDED;
    }
    if (t_new - A.lambda_end >= 0.0) {
        store_result(A, P.idx, xn, vn, BHG_FLAG_REACHED_END_, P.n_att, P.n_acc);
        return PARK_ENDED;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        R.x[c] = xn[c];
        R.v[c] = vn[c];
        R.a1[c] = a7[c];
    }
    R.t = t_new;
    R.h_abs = h_next;
    R.r_cur = r_new;
    return PARK_RESUME;
}

// ------------------------------------------------------------------------------------------
// Fixed-step classic RK4 step and its event resolution (cubic Hermite interpolant of the step)
// ------------------------------------------------------------------------------------------
template <int RHS>
__device__ __forceinline__ void rk4_step(const double x[3], const double v[3], const double a1[3], double h,
                                         const Metric &r_s, double xn[3], double vn[3], double an[3], double &r_new)
{
    const double hh = 0.5 * h;
    double a2[3], a3[3], a4[3], xs[3], v2[3], v3[3], v4[3], rr;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xs[c] = __builtin_fma(hh, v[c], x[c]);
        v2[c] = __builtin_fma(hh, a1[c], v[c]);
    }
    accel<RHS>(xs, v2, r_s, a2, rr);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xs[c] = __builtin_fma(hh, v2[c], x[c]);
        v3[c] = __builtin_fma(hh, a2[c], v[c]);
    }
    accel<RHS>(xs, v3, r_s, a3, rr);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xs[c] = __builtin_fma(h, v3[c], x[c]);
        v4[c] = __builtin_fma(h, a3[c], v[c]);
    }
    accel<RHS>(xs, v4, r_s, a4, rr);
    const double h6 = h * (1.0 / 6.0);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xn[c] = __builtin_fma(h6, __builtin_fma(2.0, v3[c], __builtin_fma(2.0, v2[c], v[c])) + v4[c], x[c]);
        vn[c] = __builtin_fma(h6, __builtin_fma(2.0, a3[c], __builtin_fma(2.0, a2[c], a1[c])) + a4[c], v[c]);
    }
    accel<RHS>(xn, vn, r_s, an, r_new);
}

struct Hermite {
    double x0[3], x1[3], v0[3], v1[3], a0[3], a1[3];
    double t0, h;
};

__device__ __forceinline__ void hermite_eval(const Hermite &d, double t, double x[3], double v[3])
{
    double s = (t - d.t0) / d.h;
    double s2 = s * s, s3 = s2 * s;
    double h00 = 2 * s3 - 3 * s2 + 1, h10 = s3 - 2 * s2 + s, h01 = -2 * s3 + 3 * s2, h11 = s3 - s2;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = h00 * d.x0[c] + h10 * d.h * d.v0[c] + h01 * d.x1[c] + h11 * d.h * d.v1[c];
        v[c] = h00 * d.v0[c] + h10 * d.h * d.a0[c] + h01 * d.v1[c] + h11 * d.h * d.a1[c];
    }
}

__device__ __forceinline__ double hermite_g(const Hermite &d, double t, double R, bool bl = false)
{
    double x[3], v[3];
    hermite_eval(d, t, x, v);
    if (bl) return x[0] - R;
    return sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) - R;
}

// One parked RK4 step, resolved by a lane of the event drain (see dp54_resolve_parked for the record; the fixed-step
// regime keeps Brent on the cubic Hermite interpolant for every event).
template <int RHS, int EVT>
__device__ __forceinline__ int rk4_resolve_parked(const TraceArgs &A, const Metric &m, const Lane &P, uint32_t kind, Lane &R)
{
    constexpr bool BL = RHS == BHG_RHS_KERR_BL_;
    const double t = P.t;
    double t_new = t + A.h_fixed;        // (as the integrate loop took the step)
    if (t_new - A.lambda_end > 0.0) t_new = A.lambda_end;
    const double h = t_new - t;
    Hermite d;
    double r_new;
    rk4_step<RHS>(P.x, P.v, P.a1, h, m, d.x1, d.v1, d.a1, r_new);
    d.t0 = t;
    d.h = h;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d.x0[c] = P.x[c];
        d.v0[c] = P.v[c];
        d.a0[c] = P.a1[c];
    }
    double best;
    int obj;
    const uint32_t fl = settle_events<EVT>(
        A, kind, t, t_new, P.x, d.x1, [&](double tt, double Rr) { return hermite_g(d, tt, Rr, BL); },
        [&](double tt) {
            double xx[3], vv[3];
            hermite_eval(d, tt, xx, vv);
            return plane_g(xx, BL);
        },
        [&](double tt, double xq[3]) {
            double vv[3];
            hermite_eval(d, tt, xq, vv);
        },
        BL, best, obj);
    if (fl) {
        double xe[3], ve[3];
        hermite_eval(d, best, xe, ve);
        store_result(A, P.idx, xe, ve, fl, P.n_att, P.n_acc);
        if (obj >= 0 && A.object_id) A.object_id[P.idx] = (int8_t)obj;
        return PARK_ENDED;
    }
    if (t_new - A.lambda_end >= 0.0) {
        store_result(A, P.idx, d.x1, d.v1, BHG_FLAG_REACHED_END_, P.n_att, P.n_acc);
        return PARK_ENDED;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        R.x[c] = d.x1[c];
        R.v[c] = d.v1[c];
        R.a1[c] = d.a1[c];
    }
    R.t = t_new;
    R.h_abs = P.h_abs;
    R.r_cur = r_new;
    return PARK_RESUME;
}

// ------------------------------------------------------------------------------------------
// Event drains: parked steps are resolved up to 64 at a time, one per lane: the ray ends there, or -- no terminal event
// after all: a disk plane crossed outside the annulus, a chord through an object sphere that the curve itself misses
// -- goes back into the ray queue to carry on.  The root search therefore always runs many lanes wide, never one lane
// wide inside the step loop.  Two lists, two drains:
//
//   SHORT list -> drain_short: steps with one candidate event, exit sphere or disk plane (every ray of a frame with an
//     exit sphere ends on one).  dp54_resolve_short only; a step whose certificate fails moves to the long list.
//     Can run at ANY time: each draining lane SWAPS registers with the slot it drains (the parked record comes out,
//     the lane's own state goes in and comes back afterwards), so the drain has the whole register budget and needs
//     no storage of its own; the lanes of a partial drain that have nothing to resolve put their state into free
//     slots (the caller makes sure there are 64 - take).
//   LONG list -> drain_long: horizon crossings, several candidates, object spheres: Brent (dp54_resolve_long).  A few
//     per cent of the parked steps -- but with 64 lanes nearly every mixed drain held one, and then all 64 lanes
//     waited for its search: kept apart they cost what they are.  Lanes keep their own state in registers here (no
//     swap, no slots needed: the compiler spills what does not fit, this path is slow anyway), so it too runs at
//     any time and at any width.
// The fixed-step kernels (no certified search) put everything on the short list and resolve it with Brent there.
// ------------------------------------------------------------------------------------------
template <int RHS, bool ADAPTIVE, int EVT, class LDS>
__device__ __forceinline__ void drain_short(const TraceArgs &A, LDS &Q, Wave &W, Lane &L, uint32_t lane, int take)
{
    const bool mine = (int)lane < take;
    const uint32_t s = mine ? Q.ev_list[W.n_evA - take + (int)lane] : Q.free_list[W.n_free - 1 - ((int)lane - take)];
    Lane P;
    P.E = P.Lz = 0.0;
    uint32_t kind = 0;
    if (mine) {
        SLOT_CHECK(Q, s, 2, 4, "drain_short take");
    } else {
        SLOT_CHECK(Q, s, 0, 4, "drain_short borrow");
    }
    if (mine) kind = slot_get<RHS>(Q.slot[s], P);
    slot_put<RHS>(Q.slot[s], L, lane_bits(L));

    int outcome = PARK_ENDED;
    Lane R;
    if (mine) {
        Metric met = metric_of(A);
        met.E = P.E;
        met.L = P.Lz;
        if (ADAPTIVE)
            outcome = dp54_resolve_short<RHS, EVT>(A, met, P, kind, R);
        else
            outcome = rk4_resolve_parked<RHS, EVT>(A, met, P, kind, R);
    }
    // own state back; the slot then takes the ray that carries on (and joins the queue), or the parked step again
    // (on its way to the long list), or is free
    const uint32_t bits = slot_get<RHS>(Q.slot[s], L);
    lane_set_bits(L, bits);
    // (PARK_REQUEUE: P goes back as the queue entry it is -- through the site that writes P back for the long list: two sources
    // for one slot write are two live copies of a ray.  Its bits are EV_REQUEUE | rejected; the pop reads bit 0.)
    const bool requeued = outcome == PARK_REQUEUE;
    const bool resumed = outcome == PARK_RESUME, again = outcome == PARK_UNCERTIFIED || requeued;
    const uint64_t rm = __ballot(resumed || requeued), am = __ballot(again && !requeued), fm = __ballot(mine && !resumed && !again);
    if (resumed) {
        SLOT_CHECK(Q, s, 4, 1, "drain_short resume");
        entry_put<RHS>(Q.slot[s], R.x, R.v, R.a1, R.h_abs, R.r_cur, R.t, P.E, P.Lz, P.idx, P.n_att, P.n_acc, 0u);
        Q.q_list[(W.q_head + W.q_count + (int)lane_rank(rm)) & (QRING - 1)] = (uint8_t)s;
    } else if (again) {
        SLOT_CHECK(Q, s, 4, requeued ? 1 : 3, "drain_short again");
        slot_put<RHS>(Q.slot[s], P, kind);
        uint8_t *list = requeued ? &Q.q_list[(W.q_head + W.q_count + (int)lane_rank(rm)) & (QRING - 1)]
                                 : &Q.ev_list[NSLOT - 1 - W.n_evB - (int)lane_rank(am)];
        *list = (uint8_t)s;
    } else if (mine) {
        // (the slots borrowed by the idle lanes of a partial drain sit below n_free and are not touched)
        SLOT_CHECK(Q, s, 4, 0, "drain_short free");
        Q.free_list[W.n_free + (int)lane_rank(fm)] = (uint8_t)s;
    } else {
        SLOT_CHECK(Q, s, 4, 0, "drain_short unborrow");
    }
    wave_lds_sync();
    // Nothing of the drain's own memory traffic (its register spills use scratch, i.e. vmcnt) may look pending to the
    // step loop: the compiler would otherwise guard the loop's first use of such a register with a vmcnt(0), which also
    // waits for the previous iteration's result stores -- in EVERY iteration (see fill_batch).
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
    W.n_evA -= take;
    W.n_evB += __builtin_popcountll(am);
    W.q_count += __builtin_popcountll(rm);
    W.n_free += __builtin_popcountll(fm);
    INV_CHECK(W, "drain_short");
#ifdef BHG_DIAG
    W.diag_general += (unsigned long long)__builtin_popcountll(am);
#endif
}

template <int RHS, int EVT, class LDS>
__device__ __forceinline__ void drain_long(const TraceArgs &A, LDS &Q, Wave &W, uint32_t lane, int take)
{
    const bool mine = (int)lane < take;
    int outcome = PARK_ENDED;
    uint32_t s = 0;
    Lane P, R;
    P.E = P.Lz = 0.0;
    P.idx = P.n_att = P.n_acc = 0u;
    if (mine) {
        s = Q.ev_list[NSLOT - W.n_evB + (int)lane];
        SLOT_CHECK(Q, s, 3, 4, "drain_long take");
        const uint32_t kind = slot_get<RHS>(Q.slot[s], P);
        Metric met = metric_of(A);
        met.E = P.E;
        met.L = P.Lz;
        outcome = dp54_resolve_long<RHS, EVT>(A, met, P, kind, R);
    }
    const bool resumed = outcome == PARK_RESUME;
    const uint64_t rm = __ballot(resumed), fm = __ballot(mine && !resumed);
    if (resumed) {
        SLOT_CHECK(Q, s, 4, 1, "drain_long resume");
        entry_put<RHS>(Q.slot[s], R.x, R.v, R.a1, R.h_abs, R.r_cur, R.t, P.E, P.Lz, P.idx, P.n_att, P.n_acc, 0u);
        Q.q_list[(W.q_head + W.q_count + (int)lane_rank(rm)) & (QRING - 1)] = (uint8_t)s;
    } else if (mine) {
        SLOT_CHECK(Q, s, 4, 0, "drain_long free");
        Q.free_list[W.n_free + (int)lane_rank(fm)] = (uint8_t)s;
    }
    wave_lds_sync();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only (see drain_short)
    W.n_evB -= take;
    W.q_count += __builtin_popcountll(rm);
    W.n_free += __builtin_popcountll(fm);
    INV_CHECK(W, "drain_long");
}

// Which list does a parked step of these kinds go on?
template <int RHS, bool ADAPTIVE, int EVT>
__device__ __forceinline__ bool short_kind(uint32_t kind)
{
    if (!ADAPTIVE) return true;
    return ((EVT & EVT_EXIT) && (kind == EV_EXIT || (RunsAhead<RHS, EVT>::value && kind == EV_AHEAD))) || ((EVT & EVT_DISK) && kind == EV_DISK);
}
// Does this kernel variant have a short list at all?  The adaptive kernel without optional events (the headline frame)
// parks horizon crossings only, all of them long: its short drain -- 650 instructions -- is not compiled in.
template <bool ADAPTIVE, int EVT>
struct HasShort {
    static constexpr bool value = !ADAPTIVE || (EVT & (EVT_EXIT | EVT_DISK)) != 0;
};

// Lanes that hold a step to park (L.pend) put its record into free slots, as many as there are.  A lane that finds
// none keeps its record in its registers and stays inactive until slots come free: every pop frees one, and with an
// empty queue and no free slot all NSLOT >= 64 slots hold parked steps, which the next service() drains.
template <int RHS, bool ADAPTIVE, int EVT, class LDS>
__device__ __forceinline__ void deposit_parked(LDS &Q, Wave &W, Lane &L, uint32_t lane)
{
    const uint64_t pm = __ballot(L.pend != 0u);
    if (!pm || W.n_free == 0) return;
    const int n = __builtin_popcountll(pm);
    const int can = n < W.n_free ? n : W.n_free;
    const uint32_t rk = lane_rank(pm);
    const bool dep = L.pend != 0u && (int)rk < can;
    const bool shrt = short_kind<RHS, ADAPTIVE, EVT>(L.pend);
    const uint64_t ma = __ballot(dep && shrt), mb = __ballot(dep && !shrt);
    if (dep) {
        const uint32_t s = Q.free_list[W.n_free - 1 - (int)rk];
        SLOT_CHECK(Q, s, 0, shrt ? 2 : 3, "deposit");
        slot_put<RHS>(Q.slot[s], L, L.pend);
        if (shrt)
            Q.ev_list[W.n_evA + (int)lane_rank(ma)] = (uint8_t)s;
        else
            Q.ev_list[NSLOT - 1 - W.n_evB - (int)lane_rank(mb)] = (uint8_t)s;
        L.pend = 0u;
    }
    wave_lds_sync();
    W.n_free -= can;
    W.n_evA += __builtin_popcountll(ma);
    W.n_evB += __builtin_popcountll(mb);
    INV_CHECK(W, "deposit");
}

// Serve the lanes that wait for a ray from the queue: at most one pop per lane, straight into the lane's registers;
// the popped slots are free again.
template <int RHS, class LDS>
__device__ __forceinline__ void pop_rays(LDS &Q, Wave &W, Lane &L, uint32_t lane)
{
    const uint64_t need = __ballot(!L.active && L.pend == 0u);
    const int n_need = __builtin_popcountll(need);
    const int take = n_need < W.q_count ? n_need : W.q_count;
    const uint32_t rk = lane_rank(need);
    if (!L.active && L.pend == 0u && (int)rk < take) {
        const uint32_t s = Q.q_list[(W.q_head + (int)rk) & (QRING - 1)];
        SLOT_CHECK(Q, s, 1, 0, "pop");
        // (a queue entry's bits: 1 = the ray's last attempt was rejected -- only a step the drain ran ahead and rejected)
        L.rejected = slot_get<RHS>(Q.slot[s], L) & 1u;
        Q.free_list[W.n_free + (int)rk] = (uint8_t)s;
        L.active = 1u;
    }
    wave_lds_sync();
    W.q_head = (W.q_head + take) & (QRING - 1);
    W.q_count -= take;
    W.n_free += take;
    INV_CHECK(W, "pop");
}

// The pool is full (no free slot) while rays are queued, and lanes hold steps to park: such a lane SWAPS with the
// head of the queue -- the queued ray comes out, the park record goes into its slot.  Without this a wave whose 64
// lanes all wait to park next to a non-empty queue would wait for ever (nobody pops, so no slot comes free, and fewer
// than 64 steps may be parked, so nothing drains).  Rare; kept apart so that the plain pop needs no register copies.
template <int RHS, bool ADAPTIVE, int EVT, class LDS>
__device__ __forceinline__ void swap_parked(LDS &Q, Wave &W, Lane &L, uint32_t lane)
{
    const uint64_t pm = __ballot(L.pend != 0u);
    const int n = __builtin_popcountll(pm);
    const int take = n < W.q_count ? n : W.q_count;
    const uint32_t rk = lane_rank(pm);
    const bool dep = L.pend != 0u && (int)rk < take;
    const bool shrt = short_kind<RHS, ADAPTIVE, EVT>(L.pend);
    const uint64_t ma = __ballot(dep && shrt), mb = __ballot(dep && !shrt);
    if (dep) {
        const uint32_t s = Q.q_list[(W.q_head + (int)rk) & (QRING - 1)];
        Lane T;
        T.E = T.Lz = 0.0;
        SLOT_CHECK(Q, s, 1, shrt ? 2 : 3, "swap");
        const uint32_t tbits = slot_get<RHS>(Q.slot[s], T);
        slot_put<RHS>(Q.slot[s], L, L.pend);
        if (shrt)
            Q.ev_list[W.n_evA + (int)lane_rank(ma)] = (uint8_t)s;
        else
            Q.ev_list[NSLOT - 1 - W.n_evB - (int)lane_rank(mb)] = (uint8_t)s;
        L = T;
        L.rejected = tbits & 1u;
        L.pend = 0u;
        L.active = 1u;
    }
    wave_lds_sync();
    W.q_head = (W.q_head + take) & (QRING - 1);
    W.q_count -= take;
    W.n_evA += __builtin_popcountll(ma);
    W.n_evB += __builtin_popcountll(mb);
    INV_CHECK(W, "swap");
}

// The rare part of service(): drain parked steps and / or put rays into the empty queue.
//   * a list is drained whenever it holds 64 steps -- at any time, the queue need not be empty;
//   * with an empty queue: a new 64-ray batch needs 64 free slots, so if fewer are free, what is parked (more than
//     NSLOT - 64 steps then) is drained first, the longer list, however few; once the work counters are dry and every
//     lane has come to rest, what is still parked is drained too and the rays it hands back carry on.  A partial
//     drain_short borrows 64 - take free slots for the idle lanes' states: with an empty queue NSLOT - n_evA - n_evB
//     are free, enough as long as the long list holds no more than NSLOT - 64 -- otherwise the long list goes first;
//   * (no prefetch of the next claim: a fetch kept in flight across iterations is a VGPR the loop carries, and the
//     s_waitcnt vmcnt(0) in front of every copy of it also waits for the previous iteration's result stores --
//     measured in round 2: config 2 +0.7 %, config 3 +4 %, config 4 +3.5 % without it.)
// ONE loop with one site each for the drains and the queue fill (each is several hundred instructions), kept apart from
// the pop: a loop around the pop makes the whole lane state a loop-carried value and costs ~20 register copies in
// every iteration of the step loop (round 2's "register-copy storm", met again here).
template <int RHS, bool ADAPTIVE, int EVT, class LDS>
__device__ __forceinline__ void replenish(const TraceArgs &A, LDS &Q, Wave &W, Lane &L, uint32_t lane)
{
    for (;;) {
        int take_a = 0, take_b = 0;
        if (HasShort<ADAPTIVE, EVT>::value && W.n_evA >= 64)
            take_a = 64;
        else if (ADAPTIVE && W.n_evB >= 64)
            take_b = 64;
        else if (W.q_count == 0 && W.n_evA + W.n_evB > 0 &&
                 (W.exhausted ? (__ballot(L.active != 0u) == 0ull) : (W.n_free < 64))) {
            if (ADAPTIVE && (!HasShort<ADAPTIVE, EVT>::value || W.n_evB >= W.n_evA || W.n_evB > NSLOT - 64))
                take_b = W.n_evB;
            else
                take_a = W.n_evA;
        }
        if (HasShort<ADAPTIVE, EVT>::value && take_a) {
#ifdef BHG_DIAG
            const unsigned long long c0 = __builtin_amdgcn_s_memtime();
            W.diag_drained += (unsigned long long)take_a;
#endif
            drain_short<RHS, ADAPTIVE, EVT>(A, Q, W, L, lane, take_a);
#ifdef BHG_DIAG
            W.diag_drain_cyc += __builtin_amdgcn_s_memtime() - c0;
#endif
            deposit_parked<RHS, ADAPTIVE, EVT>(Q, W, L, lane);     // (lanes that found no slot before have one now)
            continue;
        }
        if (ADAPTIVE && take_b) {
#ifdef BHG_DIAG
            const unsigned long long c0 = __builtin_amdgcn_s_memtime();
            W.diag_drained_long += (unsigned long long)take_b;
#endif
            drain_long<RHS, EVT>(A, Q, W, lane, take_b);
#ifdef BHG_DIAG
            W.diag_drain_long_cyc += __builtin_amdgcn_s_memtime() - c0;
#endif
            deposit_parked<RHS, ADAPTIVE, EVT>(Q, W, L, lane);
            continue;
        }
        if (W.n_free == 0 && W.q_count > 0 && __ballot(L.pend != 0u) != 0ull) {
            swap_parked<RHS, ADAPTIVE, EVT>(Q, W, L, lane);
            continue;   // (the swap may have emptied the queue with no slot free: the drains above come first)
        }
        if (W.q_count > 0 || W.exhausted || __ballot(!L.active) == 0ull) return;
        // the queue is empty, lanes wait, 64 slots are free: claim a batch
        const uint64_t base = take_fetch(issue_fetch(A, lane, W.slice), W.slice);
        BHG_KERNARG_PTR kp = kernarg_base();
        if (base >= BHG_COLD(kp, n)) {
            // this slice is dry: steal from the next one
            W.slice = (W.slice + 1) % NSLICE;
            if (++W.dry == NSLICE) W.exhausted = true;
            continue;
        }
        uint64_t first = base;
        const int32_t order_blocks = BHG_COLD(kp, order_blocks);
        if (order_blocks > 1) {
            // work-order hint: the rays are `order_blocks` equal blocks (the samples of a frame, block s =
            // sample s of every pixel).  Hand the 64-ray batches out chunk-major -- chunk 0 of every block,
            // then chunk 1 of every block ... -- so that a region's rays of ALL blocks start together: with
            // the caller's pixels sorted longest-first the long rays then all start early, instead of once
            // per block through the whole launch.  A pure permutation of the batch order.
            const uint64_t g = base >> 6, q = g / (uint64_t)order_blocks, sblk = g - q * (uint64_t)order_blocks;
            first = sblk * BHG_COLD(kp, order_block_len) + (q << 6);
        }
#ifdef BHG_DIAG
        const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
        fill_batch<RHS, ADAPTIVE>(A, Q, W, lane, first);
#ifdef BHG_DIAG
        W.diag_fill_cyc += __builtin_amdgcn_s_memtime() - c0;
#endif
    }
}

// Some lane is not stepping: park what has to be parked, (rarely) drain and refill, give the waiting lanes rays from
// the queue -- at most one pop per lane and call (a lane the queue could not serve is served by the next iteration's
// call).  Returns true when the wave is done: nothing in flight, queued, parked or waiting to be parked, no batch left.
template <int RHS, bool ADAPTIVE, int EVT, class LDS>
__device__ __forceinline__ bool service(const TraceArgs &A, LDS &Q, Wave &W, Lane &L, uint32_t lane)
{
    deposit_parked<RHS, ADAPTIVE, EVT>(Q, W, L, lane);
    const int n_ev = W.n_evA + W.n_evB;
    if (__builtin_expect(W.n_evA >= 64 || W.n_evB >= 64 || (W.q_count == 0 && !(W.exhausted && n_ev == 0)) || W.n_free == 0, 0))
        replenish<RHS, ADAPTIVE, EVT>(A, Q, W, L, lane);
    if (W.q_count > 0) pop_rays<RHS>(Q, W, L, lane);
    return W.exhausted && W.q_count == 0 && W.n_evA + W.n_evB == 0 && __ballot(L.active != 0u || L.pend != 0u) == 0ull;
}

// ------------------------------------------------------------------------------------------
// Adaptive Dormand-Prince 5(4), scipy RK45 controller semantics, persistent lane-refill wave.
// ------------------------------------------------------------------------------------------
// Waves per SIMD of the DP5(4) kernels.  Schwarzschild forms: 3 (168 VGPRs).  The step loop alone fits 4 waves
// (~120 VGPRs), but the event drain inlined next to it does not: at the 128-VGPR cap it spills ~60 doubles per lane and
// drain to scratch, which shows up as HBM traffic (config 2: 646 MB per launch against 425 MB algorithmic; config 3:
// 4.0 GB) and, for the variants that drain (nearly) every ray, as time (config 3 +3.5 %, config 4 +2.2 % at 3 waves);
// the event-free frame measures the same at 3 and at 4 waves (1.429 vs 1.423 ms) with 498 MB of traffic.  2 waves
// measured 8 % slower.  Kerr: 2 (its right-hand side alone needs ~200 VGPRs).
#ifndef BHG_DP54_WAVES_PER_SIMD
#define BHG_DP54_WAVES_PER_SIMD 3
#endif
#ifndef BHG_KERR_WAVES_PER_SIMD
#define BHG_KERR_WAVES_PER_SIMD 2
#endif
template <int RHS, int EVT>
__global__ void __launch_bounds__(64, (RHS == BHG_RHS_KERR_BL_ ? BHG_KERR_WAVES_PER_SIMD : BHG_DP54_WAVES_PER_SIMD)) trace_dp54_kernel(const TraceArgs A0)
{
    using LDS = WaveLds<RHS, Pool<RHS, true>::N>;
    __shared__ LDS Q;
    const uint32_t lane = threadIdx.x;
    const TraceArgs &A = A0;
    double r_s = A.r_hor, rtol = A.rtol, atol = A.atol, t_bound = A.lambda_end;  // r_s: horizon EVENT radius
    double max_step = A.max_step;
    // (The two scalars the prologue of every step reads, min_step_cap and max_steps, sit in SGPRs the compiler spills to
    // VGPR lanes: four v_readlane per iteration.  Holding them in VGPRs instead was tried: the 168-VGPR budget is full, they
    // went to scratch and came back with two scratch loads per iteration.)
    const double min_step_cap = A.min_step_cap;
    const uint32_t max_steps = A.max_steps;
    Metric met = metric_of(A);
    // (Round 3 held the scalars every Kerr step reads in VGPRs, because that kernel spilled 67 SGPRs and fetched them back
    // with v_readlane ~130 times per iteration.  With the rare paths' arguments read from the kernarg segment at their use
    // sites -- kernarg_base() -- no trace kernel spills an SGPR any more, and the plain form measures 0.3 % faster.)

    Lane L;
#pragma unroll
    for (int c = 0; c < 3; c++) L.x[c] = L.v[c] = L.a1[c] = 0.0;
    L.t = L.h_abs = L.r_cur = 0.0;
    L.E = L.Lz = 0.0;
    L.idx = L.n_att = L.n_acc = 0;
    L.active = L.rejected = L.pend = 0u;
    Wave W;
    W.q_head = W.q_count = 0;
    W.n_evA = W.n_evB = 0;
    W.n_free = NSLOT;
    W.exhausted = false;
    for (int i = (int)lane; i < NSLOT; i += 64) Q.free_list[i] = (uint8_t)i;
#ifdef BHG_CHECK
    for (int i = (int)lane; i < NSLOT; i += 64) Q.tag[i] = 0;
#endif
    wave_lds_sync();
#ifdef BHG_DIAG
    const unsigned long long diag_t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long diag_c0 = __builtin_amdgcn_s_memtime();
    unsigned long long diag_iters = 0, diag_lanes = 0;
    unsigned long long diag_cross = 0, diag_pass = 0;    // iterations in which some lane crossed the disk plane / passed the filter
#endif
    W.slice = blockIdx.x % NSLICE;
    W.dry = 0;
    // Work counters come in two sets used by alternate launches of a context: this launch counts on A.counter (zero
    // at launch) and zeroes the other set for the launch after it -- a 5-us memset launch less per call.
    if (blockIdx.x == 0 && lane < (uint32_t)NSLICE && A.counter_next) A.counter_next[lane * SLICE_STRIDE] = 0ull;

    for (;;) {
        if (__ballot(!L.active)) {
#ifdef BHG_DIAG
            const unsigned long long rc0 = __builtin_amdgcn_s_memtime();
#endif
            const bool done = service<RHS, true, EVT>(A, Q, W, L, lane);
#ifdef BHG_DIAG
            W.diag_refill_cyc += __builtin_amdgcn_s_memtime() - rc0;
#endif
            if (done) break;  // nothing in flight, nothing queued or parked, nothing left
        }
#ifdef BHG_DIAG
        diag_iters++;
        diag_lanes += __builtin_popcountll(__ballot(L.active));
#endif
        // (s_setprio for a wave that carries a long ray -- so that a small launch does not last as long as its longest ray takes
        // next to two other waves -- measured in round 5: 1/8 shard -0.7 %, whole frame +0.4 %, profiles/r05_prio_ab.log; not kept)

        if (L.active) {
            // ---- one attempted step (rk.py:111-165 flattened: one attempt per iteration) ----
            uint32_t term = 0;
            // The step-size floor 10 ulp(t) (rk.py:119), the step budget and "already at t_bound" (base.py:189-194)
            // practically never bite: 10 ulp(t) <= A.min_step_cap for every t in [0, t_bound], so ONE wave-wide test
            // covers them, and the common case is a min, a select and nothing else (the full prologue below is forty
            // instructions in every iteration of every ray).
            // ("already at t_bound" at the START of a step only happens with lambda_end = 0: a ray that reaches t_bound
            // is final in that same step.  The C-ABI layer then sets min_step_cap = +inf, which sends every lane here.)
            const bool odd = !(L.h_abs > min_step_cap) || L.n_att >= max_steps;
            if (__builtin_expect(__ballot(odd) != 0ull, 0)) {
                // (written as selects: as nested ifs this is eight divergent branches)
                const bool tiny = !(L.h_abs > min_step_cap);
                double min_step = 0.0;
                if (__ballot(tiny)) min_step = tiny ? 10.0 * ulp_of(L.t) : 0.0;
                const double h_clamped = (L.h_abs > max_step) ? max_step : ((L.h_abs < min_step) ? min_step : L.h_abs);
                L.h_abs = L.rejected ? L.h_abs : h_clamped;
                term = (L.h_abs < min_step) ? (uint32_t)BHG_FLAG_STEP_TOO_SMALL_
                                            : ((L.n_att >= max_steps) ? (uint32_t)BHG_FLAG_MAX_STEPS_ : 0u);
                term = (term == 0u && L.t == t_bound) ? (uint32_t)BHG_FLAG_REACHED_END_ : term;  // base.py:189-194
            } else {
                // (min_step = 0 here: the clamp of rk.py:121-124 is the upper one alone; not after a rejection)
                // (the bound as a SCALAR operand of the min, pinned there by the empty asm: left to itself the compiler
                // shares one VGPR copy of max_step between this path and the selects above, hoists it out of the loop,
                // spills it -- and reloads it here behind a vmcnt(0) that waits for the previous iteration's result stores)
                // (a compare and a select, not fmin: minnum wants both operands canonicalised first, two more instructions;
                // h_abs is never NaN.  With max_step = +inf -- the engine's default, :59-60 -- the clamp is not there at all:
                // wave-uniform branch.)
                // (the test on the bits of max_step, from a scalar the empty asm re-reads in every iteration: a flag computed
                // once outside the loop is one more SGPR pair to spill and reload)
                double ms_bits = A.max_step;
                asm volatile("" : "+s"(ms_bits));
                if ((uint32_t)__double2hiint(ms_bits) != 0x7FF00000u)
                    L.h_abs = (!L.rejected && L.h_abs > ms_bits) ? ms_bits : L.h_abs;
            }
            if (term) {
                store_result(A, L.idx, L.x, L.v, term, L.n_att, L.n_acc);
                L.active = 0u;
            } else {
                const double h_try = L.h_abs;   // (the event drain redoes the next three lines from this value)
                double t_new = L.t + h_try;
                if (t_new > t_bound) t_new = t_bound;     // (rk.py:128-129; x - y > 0 and x > y are the same test in IEEE arithmetic)
                const double h = t_new - L.t;
                L.h_abs = fabs(h);

                double a2[3], a3[3], a4[3], a5[3], a6[3], a7[3], xn[3], vn[3], r_new;
                if (RHS == BHG_RHS_KERR_BL_) {
                    met.E = L.E;
                    met.L = L.Lz;
                }
                dp54_stages<RHS>(L.x, L.v, L.a1, h, met, a2, a3, a4, a5, a6, a7, xn, vn, r_new);
                L.n_att++;

                double errsq = dp54_errsq(L.x, L.v, xn, vn, L.a1, a2, a3, a4, a5, a6, a7, h, rtol, atol);
                // NaN anywhere in the step must reject (np.maximum / norm propagate NaN) -- and does, without a test of its
                // own: a NaN in xn or vn makes the stage-7 acceleration NaN in all three components (through r^2, |k|^2 or
                // x.k), that the error sum, and `errsq < 1` is false for a NaN.  (r_new alone can only be NaN with a finite
                // state when r^2 overflows, |x| > 1e154: such a state is still finite and ends the ray at lambda_end.)
#ifdef BHG_DIAG
                if (A.diag && L.idx == A.dbg_idx && L.n_att <= 64) {
                    double *dd = reinterpret_cast<double *>(A.diag) + 262144 + (L.n_att - 1) * 4;
                    dd[0] = L.t;
                    dd[1] = h;
                    dd[2] = errsq;
                    dd[3] = 0.0;
                }
#endif

                // 0.9 * err^(-1/5) = 0.9 * errsq^(-1/10), clamped to [0.2, 10] (rk.py:148-163)
                double fac = dp54_factor(errsq);
                if (errsq < 1.0) {
                    // min(10, factor), and min(1, .) right after a rejection (rk.py:156-160): ONE min against a selected
                    // bound.  (errsq == 0 -> 10, rk.py:153-154, needs no case of its own: dp54_factor clamps its argument
                    // at 1e-11, where 0.9 x^(-1/10) = 11.3 > 10.)
                    fac = fmin(fac, L.rejected ? 1.0 : 10.0);
                    L.h_abs *= fac;
                    L.rejected = 0u;
                    L.n_acc++;

                    // events between step ends (ivp.py:109-126): horizon any direction, exit outward.  A ray in the step
                    // loop is OUTSIDE the horizon radius at the start of every step (it starts there -- start-inside rays
                    // never get here -- and a step that ends at or inside it is parked, which always ends the ray), so the
                    // sign-change rule g(t) g(t_new) <= 0 is one comparison (r_new is finite in an accepted step)
                    const bool ev_h = r_new <= r_s;
                    const bool ev_e = (EVT & EVT_EXIT) && (L.r_cur - A.r_exit <= 0.0) && (r_new - A.r_exit >= 0.0);
                    bool ev_d = (EVT & EVT_DISK) && (!(EVT & EVT_OBJ) || A.disk_r_out > 0.0) &&
                                crossed_disk_plane<RHS>(L.x, xn);
                    const bool ev_o = (EVT & EVT_OBJ) && any_sphere_candidate_of<RHS>(A, L.x, xn);
#ifdef BHG_DIAG
                    const bool diag_crossed = ev_d;
#endif
                    // (whatever else the step holds: a plane crossing that cannot lie in the annulus is no event -- and
                    // a parked step with ONE candidate event takes the drain's short path)
                    if ((EVT & EVT_DISK) && ev_d &&
                        !(RHS == BHG_RHS_KERR_BL_ ? disk_crossing_may_hit_bl<true>(A, L.x, L.v, xn, vn, h, L.a1, a2, a3, a4, a5, a6)
                                                  : disk_crossing_may_hit<true>(A, L.x, L.v, xn, vn, h, L.a1, a2, a3, a4, a5, a6)))
                        ev_d = false;
                    // ... and, in Boyer-Lindquist coordinates, what that bound lets through against the exact one (a
                    // wave-wide skip when it let nothing through).  Measured: the chord bound passes 0.19 crossings per
                    // Schwarzschild ray that the drain then finds outside the annulus, and 0.69 per Kerr ray (dr/dlambda
                    // changes along a straight line); the exact test is 140 instructions: Kerr + disk +1.5 %, the
                    // Schwarzschild disk frame -1.1 % with it -- so Kerr only.
                    if (RHS == BHG_RHS_KERR_BL_ && (EVT & EVT_DISK) && __ballot(ev_d) != 0ull) {
                        if (ev_d && !disk_crossing_may_hit_sharp<RHS>(A, L.x, L.v, xn, vn, h, L.a1, a2, a3, a4, a5, a6)) ev_d = false;
                    }
#ifdef BHG_DIAG
                    if (EVT & EVT_DISK) {      // (inside the accepted branch: the ballots below count lanes of THIS branch only)
                        diag_cross += __builtin_popcountll(__ballot(diag_crossed)) ? 1 : 0;
                        diag_pass += __builtin_popcountll(__ballot(ev_d)) ? 1 : 0;
                    }
#endif
                    const bool park = ev_h || ev_e || ev_d || ev_o;
                    if (park) {
                        // Park the step: x, v, a1, t still hold its START (the event drain recomputes it from there),
                        // h_abs is already the controller's choice for the next step, the radius register takes the
                        // |h| this step tried.  The record goes into the wave's LDS pool when the lane is next served.
                        L.pend = (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u) | (ev_d ? EV_DISK : 0u) | (ev_o ? EV_OBJ : 0u);
                        L.r_cur = h_try;
                        L.active = 0u;
                    } else {
                        // take the step (ONE place where the lane's state is overwritten: the compiler otherwise
                        // emits the twelve register copies once per way out of this block)
                        L.t = t_new;
                        L.r_cur = r_new;
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            L.x[c] = xn[c];
                            L.v[c] = vn[c];
                            L.a1[c] = a7[c];
                        }
                        if (t_new >= t_bound) {  // base.py:203-204
                            store_result<false>(A, L.idx, L.x, L.v, BHG_FLAG_REACHED_END_, L.n_att, L.n_acc);
                            L.active = 0u;
                        }
                        else if (RunsAhead<RHS, EVT>::value) {
                            // Is the NEXT step expected to leave the exit sphere?  Radial extrapolation from the state just
                            // accepted: r + h (x.k) / r >= R_exit, written r (r - R_exit) + h x.k >= 0 (Boyer-Lindquist: r and
                            // dr/dlambda are coordinates).  A GUESS, not a bound: it decides where the step is computed --
                            // here, or by the short drain (EV_AHEAD), once instead of twice -- never what comes out of it.
                            double hp = t_bound - t_new;
                            hp = L.h_abs < hp ? L.h_abs : hp;
                            const double dr = r_new - A.r_exit;
                            bool ahead;
                            if (RHS == BHG_RHS_KERR_BL_) {
                                ahead = dr < 0.0 && __builtin_fma(hp, vn[0], dr) >= 0.0;
                            } else {
                                const double xk = __builtin_fma(xn[2], vn[2], __builtin_fma(xn[1], vn[1], xn[0] * vn[0]));
                                ahead = dr < 0.0 && __builtin_fma(r_new, dr, hp * xk) >= 0.0;
                            }
                            if (ahead) {
                                L.pend = EV_AHEAD;      // (x, v, a1, t, h_abs, r_cur: the next step's start -- a queue-style record)
                                L.active = 0u;
                            }
                        }
                    }
                } else {
                    L.h_abs *= fmax(0.2, fac);
                    L.rejected = 1u;
                }
            }
        }
    }
#ifdef BHG_DIAG
    if (lane == 0 && A.diag) {
        unsigned long long *d = A.diag + (size_t)blockIdx.x * 8;
        d[0] = diag_t0;
        d[1] = __builtin_amdgcn_s_memrealtime();
        d[2] = diag_iters | (diag_cross << 24) | (diag_pass << 44);   // (a wave runs < 2^20 iterations)
        d[4] = __builtin_amdgcn_s_memtime() - diag_c0;
        d[5] = W.diag_drain_cyc;
        d[6] = W.diag_drained | (W.diag_drained_long << 40);   // steps drained from the short list | from the long list
        d[3] = diag_lanes | (W.diag_drain_long_cyc << 40);       // (lane-steps < 2^40) | cycles in drain_long
        d[7] = W.diag_fill_cyc | (W.diag_refill_cyc << 32);  // fill cycles < 2^32; refill() total in the high half
    }
#endif
}

// ------------------------------------------------------------------------------------------
// Fixed-step classic RK4 ("R-fine" regime).  Same persistent lane-refill wave.
// ------------------------------------------------------------------------------------------
template <int RHS, int EVT>
__global__ void __launch_bounds__(64) trace_rk4_kernel(const TraceArgs A)
{
    using LDS = WaveLds<RHS, Pool<RHS, false>::N>;
    __shared__ LDS Q;
    const uint32_t lane = threadIdx.x;
    const double r_s = A.r_hor, t_bound = A.lambda_end, hf = A.h_fixed;  // r_s: horizon EVENT radius
    Metric met = metric_of(A);

    Lane L;
#pragma unroll
    for (int c = 0; c < 3; c++) L.x[c] = L.v[c] = L.a1[c] = 0.0;
    L.t = L.h_abs = L.r_cur = 0.0;
    L.E = L.Lz = 0.0;
    L.idx = L.n_att = L.n_acc = 0;
    L.active = L.rejected = L.pend = 0u;
    Wave W;
    W.q_head = W.q_count = 0;
    W.n_evA = W.n_evB = 0;
    W.n_free = NSLOT;
    W.exhausted = false;
    for (int i = (int)lane; i < NSLOT; i += 64) Q.free_list[i] = (uint8_t)i;
#ifdef BHG_CHECK
    for (int i = (int)lane; i < NSLOT; i += 64) Q.tag[i] = 0;
#endif
    wave_lds_sync();
    W.slice = blockIdx.x % NSLICE;
    W.dry = 0;
    // Work counters come in two sets used by alternate launches of a context: this launch counts on A.counter (zero
    // at launch) and zeroes the other set for the launch after it -- a 5-us memset launch less per call.
    if (blockIdx.x == 0 && lane < (uint32_t)NSLICE && A.counter_next) A.counter_next[lane * SLICE_STRIDE] = 0ull;

    for (;;) {
        if (__ballot(!L.active) && service<RHS, false, EVT>(A, Q, W, L, lane)) break;
        // Rays at the end of the affine range or of their step budget leave first, in a branch of its own, so that the step
        // below is ONE region with ONE place where the lane's state is overwritten (nested under the end test, the merged
        // state was copied into a second register set at every level: 33 v_mov_b64 per iteration on 166 fp64 instructions).
        if (L.active && (L.t >= t_bound || L.n_att >= A.max_steps)) {
            store_result(A, L.idx, L.x, L.v, L.t >= t_bound ? BHG_FLAG_REACHED_END_ : BHG_FLAG_MAX_STEPS_, L.n_att, L.n_att);
            L.active = 0u;
        }
        if (L.active) {
            double t_new = L.t + hf;
            if (t_new - t_bound > 0.0) t_new = t_bound;
            const double h = t_new - L.t;
            double xn[3], vn[3], an[3], r_new;
            if (RHS == BHG_RHS_KERR_BL_) {
                met.E = L.E;
                met.L = L.Lz;
            }
            rk4_step<RHS>(L.x, L.v, L.a1, h, met, xn, vn, an, r_new);
            L.n_att++;
            const bool ev_h = r_new <= r_s;     // (outside at every step's start, see the adaptive kernel; NaN: `bad` below)
            const bool ev_e = (EVT & EVT_EXIT) && (L.r_cur - A.r_exit <= 0.0) && (r_new - A.r_exit >= 0.0);
            bool ev_d = (EVT & EVT_DISK) && (!(EVT & EVT_OBJ) || A.disk_r_out > 0.0) && crossed_disk_plane<RHS>(L.x, xn);
            const bool ev_o = (EVT & EVT_OBJ) && any_sphere_candidate_of<RHS>(A, L.x, xn);
            // (the fixed-step kernels locate events on the step's cubic Hermite interpolant: no quartic term, and the
            // stage arguments are not read)
            if ((EVT & EVT_DISK) && ev_d &&
                !(RHS == BHG_RHS_KERR_BL_ ? disk_crossing_may_hit_bl<false>(A, L.x, L.v, xn, vn, h, xn, xn, xn, xn, xn, xn)
                                          : disk_crossing_may_hit<false>(A, L.x, L.v, xn, vn, h, xn, xn, xn, xn, xn, xn)))
                ev_d = false;
            const bool ev = ev_h || ev_e || ev_d || ev_o, bad = !(r_new == r_new);
            if (ev) {
                // (the park record is the lane state as it stands -- the fixed-step drain takes |h| from the call's
                // parameters, so no double of the state is written in this branch)
                L.n_acc = L.n_att;
                L.pend = (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u) | (ev_d ? EV_DISK : 0u) | (ev_o ? EV_OBJ : 0u);
                L.active = 0u;
            } else if (bad) {
                store_result(A, L.idx, xn, vn, 0, L.n_att, L.n_att);  // NaN flag added by store_result
                L.active = 0u;
            }
            if (!ev && !bad) {
                L.t = t_new;
                L.r_cur = r_new;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    L.x[c] = xn[c];
                    L.v[c] = vn[c];
                    L.a1[c] = an[c];
                }
            }
        }
    }
}

#ifdef BHG_TU_KERR
// Acceleration probe for the Boyer-Lindquist form: x = (r, theta, phi), k = d/dlambda of those; the Killing constants
// E = -k_t, L = k_phi from the null condition AT THE POINT (the formula every kernel's ray start applies at the camera, kerr_cart_to_bl), then the
// right-hand side the trace kernels run (accel_kerr_bl).  acc is d^2 (r, theta, phi) / dlambda^2.
__global__ void accel_kerr_kernel(const double *x, const double *k, double r_s, double spin, double mu2, uint64_t n, double *acc)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]}, u[3] = {k[3 * i], k[3 * i + 1], k[3 * i + 2]};
    Metric met = metric_of(r_s, spin);
    const double a = met.a, M = met.M, r = q[0];
    const double st = sin(q[1]), ct = cos(q[1]), s2 = st * st, c2 = ct * ct;
    const double Sig = r * r + a * a * c2, Del = r * r - 2.0 * M * r + a * a;
    const double gtt = -(1.0 - 2.0 * M * r / Sig), gtp = -2.0 * M * a * r * s2 / Sig, grr = Sig / Del, gthth = Sig;
    const double gpp = (r * r + a * a + 2.0 * M * a * a * r * s2 / Sig) * s2;
    const double S = grr * u[0] * u[0] + gthth * u[1] * u[1] + gpp * u[2] * u[2] + mu2;
    const double B = gtp * u[2];
    const double kt = (-B - sqrt(B * B - gtt * S)) / gtt;
    met.E = -(gtt * kt + gtp * u[2]);
    met.L = gtp * kt + gpp * u[2];
    double a3[3], rr;
    accel_kerr_bl(q, u, met, a3, rr);
    acc[3 * i] = a3[0];
    acc[3 * i + 1] = a3[1];
    acc[3 * i + 2] = a3[2];
}

hipError_t launch_accel_kerr(const double *x, const double *k, double r_s, double spin, double mu2, uint64_t n, double *acc, hipStream_t s)
{
    const int grid = (int)((n + 255) / 256);
    if (grid == 0) return hipSuccess;
    BHG_LAUNCH(accel_kerr_kernel, dim3(grid), dim3(256), 0, s, x, k, r_s, spin, mu2, n, acc);
    return hipGetLastError();
}

// Kerr only: the passes above work in Boyer-Lindquist coordinates; turn every final state back into
// the Cartesian frame the boundary speaks (rays that started inside were stored Cartesian already).
// dir_out (direction-only calls: a sky frame reads nothing else): the Cartesian exit directions go there, 24 bytes per
// ray, and the records in A.end -- a workspace of the library then -- stay as they are: one pass of 72 bytes per ray
// instead of this pass in place (96) plus a pass that splits the directions off (72).
__global__ void __launch_bounds__(256) kerr_finalize_kernel(const TraceArgs A, double *dir_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    double *e = A.end + i * 6;
    if (A.flags[i] & BHG_FLAG_START_INSIDE_) {
        if (dir_out) {
            dir_out[i * 3 + 0] = e[3];
            dir_out[i * 3 + 1] = e[4];
            dir_out[i * 3 + 2] = e[5];
        }
        return;
    }
    double c[6];
    bl_record_to_cart(A.spin, e, e + 3, c);
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5];
    if (dir_out) {
        dir_out[i * 3 + 0] = c3;
        dir_out[i * 3 + 1] = c4;
        dir_out[i * 3 + 2] = c5;
    } else {
        e[0] = c0;
        e[1] = c1;
        e[2] = c2;
        e[3] = c3;
        e[4] = c4;
        e[5] = c5;
    }
    const bool bad = !(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3) && isfinite(c4) && isfinite(c5));
    if (bad) A.flags[i] |= (uint8_t)BHG_FLAG_NAN_;
}


#endif  // BHG_TU_KERR

// ------------------------------------------------------------------------------------------
// The lane-per-ray loops (the sampled-trajectory kernel in both its shapes, the disk-crossings, travel-time and mesh kernels,
// the start-up records): a plain loop per ray on the trace kernels' own helpers, so that the steps are theirs bit for bit.
// RayState is a ray between two steps, StepTry one attempted step from it.  What the loops share works on the two and has ONE
// definition here: the start and the start-inside result (start_ray, store_start_inside), the attempt (dp54_attempt), the
// radial sign tests, the event settlement on the step's dense output (settle_dense), the crossing record (record_crossing:
// crossings and travel time), the exit sphere taken as the plain trace takes it (exit_as_plain_trace: travel time and mesh),
// accepting a step, the final store, and on the host the launch (launch_lanes).  What differs stays in the kernels, which
// stay separate __global__ functions with register budgets of their own: sampling and fixed steps, the time quadrature, the
// mesh test, the kept state.
// Each loop spells out its own three lines "attempt; rejected: again; not accepted: the flag ends the ray".  A helper that
// loops until an attempt is accepted gives the compiler an inner loop to hoist the ray's invariants out of, which it keeps
// in registers across the attempts: disk_crossings_kernel's scratch went from 60 to 148 bytes with it, and the wave-per-ray
// trajectory kernel from three waves per SIMD to two.
// ------------------------------------------------------------------------------------------
struct RayState {
    double x[3], v[3], a1[3];   // position, direction, a(x, v) (Kerr: Boyer-Lindquist)
    double t, h_abs, r_cur;     // affine parameter, the size of the next attempt, r at x
    uint32_t n_att, n_acc;
    bool rejected;              // the last attempt was rejected (rk.py's step_rejected)
    Metric met;
};
struct StepTry {
    double t_new, h;
    double a2[3], a3[3], a4[3], a5[3], a6[3], a7[3];
    double xn[3], vn[3], r_new;
};

// Start ray i: k0 and x0 (a ONE-ray call's ride in the kernel arguments), the metric, Kerr's Cartesian -> Boyer-Lindquist
// conversion with E and L, the start-inside test and the start record {a0, r0, h0} -- fill_batch's steps, on the same functions
// and the same bits.  xe, ve: the end state of a ray that takes no step.  Returns true for a start inside the hole: xe, ve are
// then the Cartesian input, which the caller stores as the ray's result at once; S is not to be stepped.
template <int RHS, bool ADAPTIVE>
__device__ __forceinline__ bool start_ray(const TraceArgs &A, uint64_t i, RayState &S, double xe[3], double ve[3])
{
    for (int c = 0; c < 3; c++) {
        ve[c] = S.v[c] = A.k0 ? A.k0[i * 3 + c] : A.k0s[c];
        xe[c] = S.x[c] = A.x0 ? A.x0[i * 3 + c] : A.x0s[c];
    }
    S.met = metric_of(A);
    double r0;
    if (RHS == BHG_RHS_KERR_BL_) {
        kerr_cart_to_bl(S.met.a, S.met.M, A.mu2, S.x, S.v, S.met.E, S.met.L);
        r0 = S.x[0];
    } else {
        r0 = sqrt(__builtin_fma(S.x[2], S.x[2], __builtin_fma(S.x[1], S.x[1], S.x[0] * S.x[0])));
    }
    if (r0 <= A.r_hor) return true;    // 'start_inside_hole' (RelativisticRenderEngine.py:296, :311-313)
    S.t = S.h_abs = S.r_cur = 0.0;
    S.n_att = S.n_acc = 0;
    S.rejected = false;
    initial_record<RHS, ADAPTIVE>(A, S.met, S.x, S.v, S.a1, S.r_cur, S.h_abs);
    for (int c = 0; c < 3; c++) {
        xe[c] = S.x[c];
        ve[c] = S.v[c];
    }
    return false;
}

// One ATTEMPTED adaptive step: rk.py:111-165 flattened as in the trace kernels, one attempt per call -- the step-size clamp and
// floor, the step budget, "already at t_bound", the stages, the error norm and the controller.  Returns DP54_ACCEPTED (P holds
// the step; S.h_abs the next step's size), DP54_REJECTED (S.h_abs shrunk: attempt again from the same state) or the flag that
// ends the ray before the attempt.
constexpr uint32_t DP54_ACCEPTED = 0u, DP54_REJECTED = 0xFFFFFFFFu;
template <int RHS>
__device__ __forceinline__ uint32_t dp54_attempt(const TraceArgs &A, RayState &S, StepTry &P)
{
    const Metric &met = S.met;
    const double *x = S.x, *v = S.v, *a1 = S.a1, t = S.t;
    double &h_abs = S.h_abs, &t_new = P.t_new, &h = P.h, &r_new = P.r_new;
    bool &rejected = S.rejected;
    uint32_t &n_att = S.n_att, &n_acc = S.n_acc;
    double *a2 = P.a2, *a3 = P.a3, *a4 = P.a4, *a5 = P.a5, *a6 = P.a6, *a7 = P.a7, *xn = P.xn, *vn = P.vn;
    const double t_bound = A.lambda_end, max_step = A.max_step;
    const double min_step = 10.0 * ulp_of(t);
    if (!rejected) {
        if (h_abs > max_step)
            h_abs = max_step;
        else if (h_abs < min_step)
            h_abs = min_step;
    }
    if (h_abs < min_step) return BHG_FLAG_STEP_TOO_SMALL_;
    if (n_att >= A.max_steps) return BHG_FLAG_MAX_STEPS_;
    if (t == t_bound) return BHG_FLAG_REACHED_END_;
    t_new = t + h_abs;
    if (t_new - t_bound > 0.0) t_new = t_bound;
    h = t_new - t;
    h_abs = fabs(h);
    dp54_stages<RHS>(x, v, a1, h, met, a2, a3, a4, a5, a6, a7, xn, vn, r_new);
    n_att++;
    double errsq = dp54_errsq(x, v, xn, vn, a1, a2, a3, a4, a5, a6, a7, h, A.rtol, A.atol);
    if (!(r_new == r_new)) errsq = __builtin_nan("");
    double fac = dp54_factor(errsq);
    if (!(errsq < 1.0)) {
        h_abs *= fmax(0.2, fac);
        rejected = true;
        return DP54_REJECTED;
    }
    fac = (errsq == 0.0) ? 10.0 : fmin(10.0, fac);
    if (rejected) fac = fmin(1.0, fac);
    h_abs *= fac;
    rejected = false;
    n_acc++;
    return DP54_ACCEPTED;
}

// the radial sign tests of a step (find_active_events on r - R): the horizon in either direction, the exit sphere outwards
__device__ __forceinline__ void radial_events(const TraceArgs &A, const RayState &S, const StepTry &P, bool &ev_h, bool &ev_e)
{
    const double r_cur = S.r_cur, r_new = P.r_new;
    ev_h = ((r_cur - A.r_hor <= 0.0) && (r_new - A.r_hor >= 0.0)) || ((r_cur - A.r_hor >= 0.0) && (r_new - A.r_hor <= 0.0));
    ev_e = (A.r_exit > 0.0) && (r_cur - A.r_exit <= 0.0) && (r_new - A.r_exit >= 0.0);
}

// Accept a step that no event ends: its end is the ray's end state so far.  Returns true when that is lambda_end; otherwise
// S moves on to it.
__device__ __forceinline__ bool advance(const TraceArgs &A, RayState &S, const StepTry &P, double xe[3], double ve[3])
{
    for (int c = 0; c < 3; c++) {
        xe[c] = P.xn[c];
        ve[c] = P.vn[c];
    }
    if (P.t_new - A.lambda_end >= 0.0) return true;
    S.t = P.t_new;
    S.r_cur = P.r_new;
    for (int c = 0; c < 3; c++) {
        S.x[c] = P.xn[c];
        S.v[c] = P.vn[c];
        S.a1[c] = P.a7[c];
    }
    return false;
}

// The ray's result: (xe, ve), or -- the controller gave up -- the state the last attempt started from
__device__ __forceinline__ void finish_ray(const TraceArgs &A, uint64_t i, const RayState &S, double xe[3], double ve[3],
                                           uint32_t flags)
{
    if (flags & (BHG_FLAG_STEP_TOO_SMALL_ | BHG_FLAG_MAX_STEPS_)) {
        for (int c = 0; c < 3; c++) {
            xe[c] = S.x[c];
            ve[c] = S.v[c];
        }
    }
    store_result(A, (uint32_t)i, xe, ve, flags, S.n_att, S.n_acc);  // Kerr: still Boyer-Lindquist, finalised next
}

// The result of a ray that starts inside the hole (start_ray returned true): final at once, the Cartesian input, no step.
// Each kernel adds its own outputs.
__device__ __forceinline__ void store_start_inside(const TraceArgs &A, uint64_t i, const double xe[3], const double ve[3])
{
    store_result(A, (uint32_t)i, xe, ve, BHG_FLAG_START_INSIDE_ | BHG_FLAG_HIT_HORIZON_, 0, 0);
}

// The event settlement of an accepted step S -> P on its dense output d (position half built): settle_events with the three
// callables of the dense output
template <int RHS, int EVT>
__device__ __forceinline__ uint32_t settle_dense(const TraceArgs &A, uint32_t kind, const RayState &S, const StepTry &P, const Dense &d,
                                                 double &best, int &obj)
{
    constexpr bool BL = RHS == BHG_RHS_KERR_BL_;
    return settle_events<EVT>(
        A, kind, S.t, P.t_new, S.x, P.xn, [&](double tt, double Rr) { return dense_g(d, tt, Rr, BL); },
        [&](double tt) { return dense_plane_g(d, tt, BL); }, [&](double tt, double xq[3]) { dense_pos(d, tt, xq); }, BL, best, obj);
}

// The disk-plane crossing of a step [d.t0, t_new] whose ends lie on opposite sides of the plane (crossed_disk_plane: at most one
// root per step), d its dense output with both halves built.  The root by brent_root as settle_events finds it; the crossing
// counts when its cylindrical radius lies in [disk_r_in, disk_r_out] and -- evflag: the step holds the ray's terminal event
// too, at t_stop -- when it is not later than that event's root (scipy_reference's td <= te).  A crossing that counts bumps
// n_cross; while records are left (max_cross) its dense-output state, Cartesian (Kerr: converted here, kerr_finalize_kernel's
// formulas), goes to slot m = the count before it, cross[(m * cross_stride + i) * 6].  Returns that slot, or -1 when nothing
// was stored; `root` is the crossing's parameter.
template <int RHS>
__device__ __forceinline__ int record_crossing(const TraceArgs &A, uint64_t i, const Dense &d, double t_new, uint32_t evflag,
                                               double t_stop, uint32_t &n_cross, double &root)
{
    const bool bl = RHS == BHG_RHS_KERR_BL_;
    root = brent_root([&](double tt) { return dense_plane_g(d, tt, bl); }, d.t0, t_new);
    double sx[3], sv[3];
    dense_pos(d, root, sx);
    const double R = disk_radius(A, sx, bl);
    if (!(R >= A.disk_r_in && R <= A.disk_r_out && (!evflag || root <= t_stop))) return -1;
    const uint32_t m = n_cross++;
    if (!(m < (uint32_t)A.max_cross)) return -1;
    dense_dir(d, root, sv);
    if (bl) {
        double c[6];
        bl_record_to_cart(A.spin, sx, sv, c);
        for (int q = 0; q < 3; q++) {
            sx[q] = c[q];
            sv[q] = c[3 + q];
        }
    }
    double *o = A.cross + ((uint64_t)m * A.cross_stride + i) * 6;
    reinterpret_cast<double2 *>(o)[0] = make_double2(sx[0], sx[1]);
    reinterpret_cast<double2 *>(o)[1] = make_double2(sx[2], sv[0]);
    reinterpret_cast<double2 *>(o)[2] = make_double2(sv[1], sv[2]);
    return (int)m;
}

// Disk off: the results are the plain trace's, bit for bit.  The trace kernels take a step whose ONE candidate event is the
// exit sphere through their certified Newton search first (dp54_short_core: the same root as Brent's to 4 eps, another
// iterate) and leave everything else to the Brent search of settle_events; so does a kernel that asks here for a step whose
// terminal event it has settled.  True: the search held and has stored the ray's result (end, flags, step counts) itself.
template <int RHS>
__device__ __forceinline__ bool exit_as_plain_trace(const TraceArgs &A, uint64_t i, const RayState &S, const StepTry &P,
                                                    bool ev_h, bool ev_e)
{
    return !(A.disk_r_out > 0.0) && ev_e && !ev_h &&
           dp54_short_core<RHS, EVT_EXIT>(A, S.x, S.v, S.a1, S.t, P.t_new, P.h, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7, P.xn, P.vn,
                                          EV_EXIT, (uint32_t)i, S.n_att, S.n_acc) == PARK_ENDED;
}

// Host side.  The right-hand sides this translation unit instantiates: f(std::integral_constant<int, RHS>) for the one asked
// for (the Kerr and the time-like unit hold one each)
template <class F>
static void with_rhs(int rhs, const F &f)
{
#if defined(BHG_TU_KERR)
    f(std::integral_constant<int, BHG_RHS_KERR_BL_>{});
#elif defined(BHG_TU_TIMELIKE)
    f(std::integral_constant<int, BHG_RHS_CHRISTOFFEL_TL_>{});
#else
    if (rhs == BHG_RHS_REDUCED_)
        f(std::integral_constant<int, BHG_RHS_REDUCED_>{});
    else
        f(std::integral_constant<int, BHG_RHS_CHRISTOFFEL_>{});
#endif
}

// one lane per ray, 64 rays to a workgroup
static dim3 lane_grid(uint64_t n) { return dim3((unsigned)((n + 63) / 64)); }

// The launch of a lane-per-ray kernel: launch(RHS, grid) launches the instance; an empty call launches nothing
template <class F>
static hipError_t launch_lanes(const TraceArgs &a, int rhs, const F &launch)
{
    if (a.n == 0) return hipSuccess;
    with_rhs(rhs, [&](auto R) { launch(R, lane_grid(a.n)); });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Sampled trajectories: what calc_trajectory returns with nr_points_curve (RelativisticRenderEngine.py:
// 293-294; the curves of README Fig. 5/6).  A plain loop per ray -- this is the small-n plotting path, not the
// frame path.  Same start record (start_ray), same stages / error norm / factor helpers as
// the integrate loop; after every accepted step the samples t_eval_j <= t are emitted through the step's
// dense output (solve_ivp's t_eval semantics, ivp.py:706-723); rays that end early emit fewer samples.
// Two shapes, same arithmetic and same bits: WAVE = false, one LANE per ray (many rays, few samples each); WAVE = true,
// one WAVE per ray -- every lane steps the same ray (wave-uniform loads and arithmetic cost a SIMD nothing extra) and
// the samples of a step are shared out over the 64 lanes, stored coalesced.  That is the shape of the engine's literal
// call, ONE ray with nr_points_curve = 10000 (:293-294): a single lane spent 1.9 ms of its 2.0 ms evaluating 10,000
// dense-output points one after the other.
// ------------------------------------------------------------------------------------------
// (WAVE: the workgroup is one wave -- or, for a handful of rays with many samples each, several waves that ALL integrate the ray,
// every lane alike, and share the samples of each step between them: no hand-off, no barrier; blockDim.x samples per pass)
template <int RHS, bool WAVE, bool FIXED>
__global__ void __launch_bounds__(WAVE ? 256 : 64) trajectory_dp54_kernel(const TraceArgs A, double *traj, uint32_t *n_valid,
                                                             uint32_t T)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t i = WAVE ? (uint64_t)blockIdx.x : (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double t_bound = A.lambda_end;
    double *out = traj + i * 6 * (uint64_t)T;
    RayState S;
    double xe[3], ve[3];
    if (start_ray<RHS, !FIXED>(A, i, S, xe, ve)) {
        // final at once, no samples.  One wave per ray: every lane has worked the start out alike, all of them fill the sample
        // block with NaN and lane 0 stores; one lane per ray: the host has preset the block
        if (WAVE) {
            for (uint32_t j = lane; j < 6 * T; j += blockDim.x) out[j] = __builtin_nan("");
            if (lane != 0) return;
        }
        n_valid[i] = 0;
        if (A.object_id) A.object_id[i] = (int8_t)-1;
        store_start_inside(A, i, xe, ve);
        return;
    }
    const double dt = t_bound / (double)(T - 1);
    uint32_t next = 0, flags = 0;
    int hit_obj = -1;        // bhg_trajectory_objects: the sphere the ray ends on
    for (;;) {
        StepTry P;
        if (FIXED) {
            // classic RK4 with the fixed step h_fixed (the build's "R-fine" regime): no controller, every step accepted
            if (S.t >= t_bound) {
                flags = BHG_FLAG_REACHED_END_;
                break;
            }
            if (S.n_att >= A.max_steps) {
                flags = BHG_FLAG_MAX_STEPS_;
                break;
            }
            P.t_new = S.t + A.h_fixed;
            if (P.t_new - t_bound > 0.0) P.t_new = t_bound;
            P.h = P.t_new - S.t;
            rk4_step<RHS>(S.x, S.v, S.a1, P.h, S.met, P.xn, P.vn, P.a7, P.r_new);
            S.n_att++;
            S.n_acc = S.n_att;
        } else {
            const uint32_t st = dp54_attempt<RHS>(A, S, P);
            if (st == DP54_REJECTED) continue;
            if (st != DP54_ACCEPTED) {
                flags = st;
                break;
            }
        }
        // the step's interpolant: the dense output of the accepted DP5(4) step, or -- fixed steps -- its cubic Hermite interpolant
        Dense d;
        Hermite hd;
        const bool bl = RHS == BHG_RHS_KERR_BL_;
        if (FIXED) {
            hd.t0 = S.t;
            hd.h = P.h;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                hd.x0[c] = S.x[c];
                hd.v0[c] = S.v[c];
                hd.a0[c] = S.a1[c];
                hd.x1[c] = P.xn[c];
                hd.v1[c] = P.vn[c];
                hd.a1[c] = P.a7[c];
            }
        } else {
            build_dense(d, S.t, P.h, S.x, S.v, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
        }
        auto state_at = [&](double tt, double sx[3], double sv[3]) {
            if (FIXED) {
                hermite_eval(hd, tt, sx, sv);
            } else {
                dense_pos(d, tt, sx);
                dense_dir(d, tt, sv);
            }
        };
        bool ev_h, ev_e;
        radial_events(A, S, P, ev_h, ev_e);
        // the thin disk (LimitedRelativisticRenderEngine.py:283-286, :413-438): a plane crossing is terminal only inside the annulus
        const bool ev_d = (A.disk_r_out > 0.0) && crossed_disk_plane<RHS>(S.x, P.xn);
        // object spheres (bhg_trajectory_objects; the reference's collision stub, RelativisticRenderEngine.py:304-305): the
        // trace kernels' own chord rule on the step's ends
        const bool ev_o = (A.n_spheres > 0) && any_sphere_candidate_of<RHS>(A, S.x, P.xn);
        double t_stop = P.t_new;
        uint32_t evflag = 0;
        if (FIXED && !(ev_h || ev_e || ev_d || ev_o) && !(P.r_new == P.r_new)) {
            // a fixed step that ends in a non-finite state (through the Boyer-Lindquist 1 / Delta singularity): the ray ends
            // there, flagged NaN by store_result; the step yields no samples
            for (int c = 0; c < 3; c++) {
                xe[c] = P.xn[c];
                ve[c] = P.vn[c];
            }
            flags = 0;
            break;
        }
        if (ev_h || ev_e || ev_d || ev_o) {
            // the trace kernels' own event settlement (Brent on the dense output, scipy's brentq step for step; of the
            // terminal candidates the earliest root wins, ties in the order horizon, exit, disk, sphere 0, 1, ...)
            const uint32_t kind = (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u) | (ev_d ? EV_DISK : 0u) | (ev_o ? EV_OBJ : 0u);
            double best;
            int obj;
            if (FIXED) {
                evflag = settle_events<(EVT_EXIT | EVT_DISK | EVT_OBJ)>(
                    A, kind, S.t, P.t_new, S.x, P.xn, [&](double tt, double Rr) { return hermite_g(hd, tt, Rr, bl); },
                    [&](double tt) {
                        double q[3], vv[3];
                        hermite_eval(hd, tt, q, vv);
                        return plane_g(q, bl);
                    },
                    [&](double tt, double xq[3]) {
                        double vv[3];
                        hermite_eval(hd, tt, xq, vv);
                    },
                    bl, best, obj);
            } else {
                evflag = settle_dense<RHS, (EVT_EXIT | EVT_DISK | EVT_OBJ)>(A, kind, S, P, d, best, obj);
            }
            if (evflag) {
                t_stop = best;
                hit_obj = obj;
            }
        }
        // emit every sample time up to where this step ends
        uint32_t first = next, stride = 1, last = T;
        if (WAVE) {
            // the samples of this step are next .. g-1 with g the first index whose time lies beyond t_stop (the times
            // are nondecreasing in the index): a guess from the quotient, put right with the serial loop's own comparison
            auto te_of = [&](uint32_t j) { return (j + 1 == T) ? t_bound : (double)j * dt; };
            const double q = floor(t_stop / dt) + 1.0;
            uint32_t g = q >= (double)T ? T : (q > (double)next ? (uint32_t)q : next);
            while (g > next && !(te_of(g - 1) <= t_stop)) g--;
            while (g < T && te_of(g) <= t_stop) g++;
            first = next + lane;
            stride = blockDim.x;
            last = g;
            next = g;
        }
        for (uint32_t j = first; j < last; j += stride) {
            const double te = (j + 1 == T) ? t_bound : (double)j * dt;
            if (!WAVE) {
                if (!(te <= t_stop)) break;
                next = j + 1;
            }
            double sx[3], sv[3];
            state_at(te, sx, sv);
            if (bl) {   // (not bl_record_to_cart: its c[5] has a + 0.0 * u2 term, which changes a -0.0 and the NaN propagation: other bits)
                const double r = sx[0], th = sx[1], ph = sx[2], a = A.spin;
                const double R = sqrt(r * r + a * a), st = sin(th), ct = cos(th), sp = sin(ph), cp = cos(ph);
                const double u0 = sv[0], u1 = sv[1], u2 = sv[2];
                sx[0] = R * st * cp;
                sx[1] = R * st * sp;
                sx[2] = r * ct;
                sv[0] = (r / R * st * cp) * u0 + (R * ct * cp) * u1 + (-R * st * sp) * u2;
                sv[1] = (r / R * st * sp) * u0 + (R * ct * sp) * u1 + (R * st * cp) * u2;
                sv[2] = ct * u0 + (-r * st) * u1;
            }
            for (int c = 0; c < 3; c++) {
                out[(uint64_t)c * T + j] = sx[c];
                out[(uint64_t)(3 + c) * T + j] = sv[c];
            }
        }
        if (evflag) {
            flags = evflag;
            state_at(t_stop, xe, ve);
            break;
        }
        if (advance(A, S, P, xe, ve)) {
            flags = BHG_FLAG_REACHED_END_;
            break;
        }
    }
    if (WAVE) {     // samples the ray never reached read back as NaN
        for (uint32_t j = next + lane; j < T; j += blockDim.x)
            for (int c = 0; c < 6; c++) out[(uint64_t)c * T + j] = __builtin_nan("");
        if (lane != 0) return;
    }
    n_valid[i] = next;
    if (A.object_id) A.object_id[i] = (int8_t)hit_obj;
    finish_ray(A, i, S, xe, ve, flags);
}

// one wave per ray while the rays are too few to fill the chip's lanes anyway (the C-ABI layer asks too: such a call needs
// no memset of the sample block and -- one ray -- no upload of k0)
#ifndef BHG_TU_KERR
#ifndef BHG_TU_TIMELIKE
bool trajectory_wave_per_ray(uint64_t n) { return n <= 2048; }
#endif
#endif

// sampled trajectories of one right-hand side: ONE launch in either shape
template <int RHS, bool FIXED>
static void launch_trajectory_rhs_m(const TraceArgs &a, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s)
{
    if (trajectory_wave_per_ray(a.n)) {
        // the engine's literal call is ONE ray with 10,000 samples: four waves share the samples (the step loop itself is one
        // wave's work however many run it: 43 us of the call; the samples 27 us with one wave)
        const unsigned threads = (a.n <= 64 && T >= 1024) ? 256u : 64u;   // (four waves = one per SIMD of a CU; eight measured slower than one)
        BHG_LAUNCH((trajectory_dp54_kernel<RHS, true, FIXED>), dim3((unsigned)a.n), dim3(threads), 0, s, a, traj, n_valid, T);
    } else {
        BHG_LAUNCH((trajectory_dp54_kernel<RHS, false, FIXED>), lane_grid(a.n), dim3(64), 0, s, a, traj, n_valid, T);
    }
}

// method: BHG_METHOD_DP54_ (the step's dense output) or BHG_METHOD_RK4_ (fixed steps, cubic Hermite interpolant)
template <int RHS>
static void launch_trajectory_rhs(const TraceArgs &a, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s)
{
    if (method == BHG_METHOD_RK4_) launch_trajectory_rhs_m<RHS, true>(a, traj, n_valid, T, s);
    else launch_trajectory_rhs_m<RHS, false>(a, traj, n_valid, T, s);
}

#if defined(BHG_TU_KERR)
hipError_t launch_trajectory_kerr(const TraceArgs &a, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s)
{
    launch_trajectory_rhs<BHG_RHS_KERR_BL_>(a, method, traj, n_valid, T, s);
    BHG_LAUNCH(kerr_finalize_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, (double *)nullptr);
    return hipGetLastError();
}
#elif defined(BHG_TU_TIMELIKE)
hipError_t launch_trajectory_timelike(const TraceArgs &a, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s)
{
    launch_trajectory_rhs<BHG_RHS_CHRISTOFFEL_TL_>(a, method, traj, n_valid, T, s);
    return hipGetLastError();
}
#else
hipError_t launch_trajectory(const TraceArgs &a, int rhs, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trajectory_kerr(a, method, traj, n_valid, T, s);
    if (rhs == BHG_RHS_CHRISTOFFEL_TL_) return launch_trajectory_timelike(a, method, traj, n_valid, T, s);
    with_rhs(rhs, [&](auto R) { launch_trajectory_rhs<R.value>(a, method, traj, n_valid, T, s); });
    return hipGetLastError();
}
#endif

// ------------------------------------------------------------------------------------------
// Disk crossings (bhg_trace_crossings_device): the ray is carried THROUGH the thin disk and every
// plane crossing inside the annulus is recorded -- scipy's solve_ivp with the disk plane as a NON-terminal event g = z
// (Kerr: cos theta), as oracle/scipy_reference.py has always run it.  The step sequence is that of the trace with the disk
// off: disk_r_out plays no part in step control and a crossing never truncates a step; horizon, exit sphere and lambda_end
// end the ray as they do there, and end / flags / n_steps / n_accepted are that trace's.
// One LANE per ray, a plain loop: trajectory_dp54_kernel's step loop (the trace kernels' own stages, error norm,
// controller, dense output and Brent search) without the sampling, on the same named state and helpers (RayState, StepTry).
// Per accepted step: the sign-change rule of find_active_events (crossed_disk_plane: at most one root per step), the root
// by brent_root on the step's dense output as settle_events finds it, counted when its cylindrical radius lies in
// [disk_r_in, disk_r_out] and -- the step holding the ray's terminal event too -- when it is not later than that event's
// root (scipy_reference's td <= te).  Record m of ray i is the dense-output state at the root, Cartesian (Kerr: converted
// here, kerr_finalize_kernel's formulas), at cross[(m * cross_stride + i) * 6]; only the first max_cross are stored,
// n_cross counts them all (saturating at 255); records a ray never reached are not written.
// ------------------------------------------------------------------------------------------
// (the trace kernels' register budgets: three waves per SIMD for the Cartesian forms, two for Kerr -- left to itself the compiler
// takes 182 VGPRs for the Cartesian instances, two waves, and the Schwarzschild frames measure 13 % slower)
template <int RHS>
__global__ void __launch_bounds__(64, (RHS == BHG_RHS_KERR_BL_ ? BHG_KERR_WAVES_PER_SIMD : BHG_DP54_WAVES_PER_SIMD)) disk_crossings_kernel(const TraceArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const bool bl = RHS == BHG_RHS_KERR_BL_;
    RayState S;
    double xe[3], ve[3];
    if (start_ray<RHS, true>(A, i, S, xe, ve)) {    // final at once, no crossings
        A.n_cross[i] = 0;
        store_start_inside(A, i, xe, ve);
        return;
    }
    uint32_t flags = 0, n_cross = 0;
    for (;;) {
        StepTry P;
        const uint32_t st = dp54_attempt<RHS>(A, S, P);
        if (st == DP54_REJECTED) continue;
        if (st != DP54_ACCEPTED) {
            flags = st;
            break;
        }
        bool ev_h, ev_e;
        radial_events(A, S, P, ev_h, ev_e);
        const bool ev_d = crossed_disk_plane<RHS>(S.x, P.xn);
        uint32_t evflag = 0;
        double t_stop = P.t_new;
        if (ev_h || ev_e || ev_d) {
            Dense d;
            build_dense(d, S.t, P.h, S.x, S.v, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
            if (ev_h || ev_e) {
                // the terminal events, settled as the trace kernels settle them (the earliest root wins, horizon before exit).
                // (settle_dense's call, written out: through the helper this kernel, alone on a three-waves budget, takes 16
                // and 8 more bytes of scratch)
                double best;
                int obj;
                evflag = settle_events<EVT_EXIT>(
                    A, (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u), S.t, P.t_new, S.x, P.xn,
                    [&](double tt, double Rr) { return dense_g(d, tt, Rr, bl); }, [&](double tt) { return dense_plane_g(d, tt, bl); },
                    [&](double tt, double xq[3]) { dense_pos(d, tt, xq); }, bl, best, obj);
                if (evflag) t_stop = best;
            }
            if (ev_d) {
                double root;
                record_crossing<RHS>(A, i, d, P.t_new, evflag, t_stop, n_cross, root);
            }
            if (evflag) {
                flags = evflag;
                dense_pos(d, t_stop, xe);
                dense_dir(d, t_stop, ve);
                break;
            }
        }
        if (advance(A, S, P, xe, ve)) {
            flags = BHG_FLAG_REACHED_END_;
            break;
        }
    }
    A.n_cross[i] = (uint8_t)(n_cross < 255u ? n_cross : 255u);
    finish_ray(A, i, S, xe, ve, flags);
}

#if defined(BHG_TU_KERR)
hipError_t launch_trace_crossings_kerr(const TraceArgs &a, hipStream_t s)
{
    return launch_lanes(a, BHG_RHS_KERR_BL_, [&](auto R, dim3 grid) { BHG_LAUNCH((disk_crossings_kernel<R.value>), grid, dim3(64), 0, s, a); });
}
#elif !defined(BHG_TU_TIMELIKE)
hipError_t launch_trace_crossings(const TraceArgs &a, int rhs, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trace_crossings_kerr(a, s);
    return launch_lanes(a, rhs, [&](auto R, dim3 grid) { BHG_LAUNCH((disk_crossings_kernel<R.value>), grid, dim3(64), 0, s, a); });
}
#endif

// ------------------------------------------------------------------------------------------
// Light travel time (bhg_travel_time_device): the crossings trace above, step for step, plus the
// coordinate time t that elapses along the ray -- Schwarzschild / Boyer-Lindquist t, a function of position and the ray's
// Killing constants alone:
//     Schwarzschild (both forms):  dt/dlambda = E / (1 - r_s / r),  E = sqrt(f0 (|k0|^2 + h0 (n0.k0)^2)) at the start point
//     Kerr:                        dt/dlambda = [E ((r^2 + a^2)^2 - Delta a^2 sin^2 theta) - 2 M a r L] / (Sigma Delta)
// (kerr_rhs.inc's kt, which does not depend on the velocities; E, L as kerr_cart_to_bl leaves them in Metric).
// Quadrature: 6-point Gauss-Legendre per accepted step on the step's own dense-output position, summed in step order; the
// step that holds the ray's terminal event runs to the event's root only.  The time of a crossing is the time at the
// start of its step plus the same rule on [lambda_j, root].  A node at r <= r_hor makes the ray's time and every time
// after it +inf (the ray stepped across the hole: section 7's transparent centre); a ray that ends on the horizon or
// starts inside has t_end = +inf, a ray flagged NaN has NaN.
// A kernel of its own beside disk_crossings_kernel, not a switch on it; the two share the crossing record (record_crossing)
// and the helpers above.  The position half of the dense output is live on every accepted step here, so the kernel has the
// whole register file of one wave (__launch_bounds__(64)) rather than the headline kernels' three-waves budget: this is a
// side path.
// max_cross = 0 and disk_r_out = 0 are allowed: no plane test, no records (cross, n_cross, t_cross may then be null).  With the
// disk off end / flags / n_steps / n_accepted are the PLAIN trace's bit for bit (with a disk: the crossings trace's).
// ------------------------------------------------------------------------------------------
// numpy.polynomial.legendre.leggauss(6) mapped to [0, 1]: nodes (1 + x) / 2, weights w / 2
__device__ constexpr double GL6_X[6] = {0.033765242898423975, 0.16939530676686776, 0.38069040695840151,
                                        0.61930959304159849, 0.83060469323313224, 0.96623475710157603};
__device__ constexpr double GL6_W[6] = {0.085662246189584873, 0.18038078652406947, 0.23395696728634569,
                                        0.23395696728634569, 0.18038078652406947, 0.085662246189584873};

// dt/dlambda at the dense-output position q (Kerr: Boyer-Lindquist r, theta); inside: q lies at r <= r_hor
template <int RHS>
__device__ __forceinline__ double time_rate(const TraceArgs &A, const Metric &met, double E, const double q[3], bool &inside)
{
    if (RHS == BHG_RHS_KERR_BL_) {
        const double r = q[0], a = met.a, M = met.M;
        double sn, cs;
        sincos_pi4(q[1], sn, cs);
        const double r2 = r * r, a2 = a * a;
        const double ra = r2 + a2, Sig = r2 + a2 * (cs * cs), Del = ra - 2.0 * M * r;
        inside = inside || (r <= A.r_hor);
        return (met.E * (ra * ra - Del * a2 * (sn * sn)) - 2.0 * M * a * r * met.L) / (Sig * Del);
    }
    const double r = sqrt(__builtin_fma(q[2], q[2], __builtin_fma(q[1], q[1], q[0] * q[0])));
    inside = inside || (r <= A.r_hor);
    return E / (1.0 - A.r_s / r);
}

// the rule on [d.t0, d.t0 + w]; +inf when a node lies inside the horizon radius
template <int RHS>
__device__ __forceinline__ double time_quadrature(const TraceArgs &A, const Metric &met, double E, const Dense &d, double w)
{
    double sum = 0.0;
    bool inside = false;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double q[3];
        dense_pos(d, __builtin_fma(w, GL6_X[k], d.t0), q);
        sum = __builtin_fma(GL6_W[k], time_rate<RHS>(A, met, E, q, inside), sum);
    }
    return inside ? __builtin_inf() : w * sum;
}

template <int RHS>
__global__ void __launch_bounds__(64) travel_time_kernel(const TraceArgs A, double *t_end, double *t_cross)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const bool bl = RHS == BHG_RHS_KERR_BL_;
    const bool disk = A.disk_r_out > 0.0;
    RayState S;
    double xe[3], ve[3];
    if (start_ray<RHS, true>(A, i, S, xe, ve)) {    // final at once, no crossings
        if (A.n_cross) A.n_cross[i] = 0;
        t_end[i] = __builtin_inf();
        store_start_inside(A, i, xe, ve);
        return;
    }
    // Schwarzschild: E from the start state (Kerr: Metric::E)
    double E = 0.0;
    if (!bl) {
        const double r0 = sqrt(__builtin_fma(S.x[2], S.x[2], __builtin_fma(S.x[1], S.x[1], S.x[0] * S.x[0])));
        const double f0 = 1.0 - A.r_s / r0, h0 = A.r_s / (r0 - A.r_s);
        const double nk = (S.x[0] * S.v[0] + S.x[1] * S.v[1] + S.x[2] * S.v[2]) / r0;
        const double kk = S.v[0] * S.v[0] + S.v[1] * S.v[1] + S.v[2] * S.v[2];
        E = sqrt(f0 * (kk + h0 * nk * nk));
    }
    double tt = 0.0;        // the time up to S.t
    uint32_t flags = 0, n_cross = 0;
    bool stored = false;    // the ray's result is in place already
    for (;;) {
        StepTry P;
        const uint32_t st = dp54_attempt<RHS>(A, S, P);
        if (st == DP54_REJECTED) continue;
        if (st != DP54_ACCEPTED) {
            flags = st;
            break;
        }
        bool ev_h, ev_e;
        radial_events(A, S, P, ev_h, ev_e);
        const bool ev_d = disk && crossed_disk_plane<RHS>(S.x, P.xn);
        uint32_t evflag = 0;
        double t_stop = P.t_new;
        Dense d;
        build_dense_pos(d, S.t, P.h, S.x, S.v, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
        if (ev_h || ev_e || ev_d) {
            build_dense_dir(d, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
            if (ev_h || ev_e) {
                // the terminal events, settled as the trace kernels settle them (the earliest root wins, horizon before exit)
                double best;
                int obj;
                evflag = settle_dense<RHS, EVT_EXIT>(A, (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u), S, P, d, best, obj);
                if (evflag) t_stop = best;
            }
            if (ev_d) {
                double root;
                const int m = record_crossing<RHS>(A, i, d, P.t_new, evflag, t_stop, n_cross, root);
                if (m >= 0) t_cross[(uint64_t)m * A.cross_stride + i] = tt + time_quadrature<RHS>(A, S.met, E, d, root - S.t);
            }
        }
        tt += time_quadrature<RHS>(A, S.met, E, d, t_stop - S.t);
        if (evflag) {
            flags = evflag;
            // (disk off: the plain trace's bits.  The time still runs to Brent's root, as it does with a disk: one definition
            // of the time, two ulp apart at most)
            if (exit_as_plain_trace<RHS>(A, i, S, P, ev_h, ev_e)) {
                stored = true;
                break;
            }
            dense_pos(d, t_stop, xe);
            dense_dir(d, t_stop, ve);
            break;
        }
        if (advance(A, S, P, xe, ve)) {
            flags = BHG_FLAG_REACHED_END_;
            break;
        }
    }
    if (A.n_cross) A.n_cross[i] = (uint8_t)(n_cross < 255u ? n_cross : 255u);
    if (stored) {
        t_end[i] = tt;
        return;
    }
    if (flags & BHG_FLAG_HIT_HORIZON_) tt = __builtin_inf();
    // (the state finish_ray stores; store_result's own test for the NaN flag)
    {
        const bool gave_up = flags & (BHG_FLAG_STEP_TOO_SMALL_ | BHG_FLAG_MAX_STEPS_);
        const double *fx = gave_up ? S.x : xe, *fv = gave_up ? S.v : ve;
        if (!isfinite(((fx[0] + fx[1]) + (fx[2] + fv[0])) + (fv[1] + fv[2]))) tt = __builtin_nan("");
    }
    t_end[i] = tt;
    finish_ray(A, i, S, xe, ve, flags);
}

#if defined(BHG_TU_KERR)
hipError_t launch_travel_time_kerr(const TraceArgs &a, double *t_end, double *t_cross, hipStream_t s)
{
    return launch_lanes(a, BHG_RHS_KERR_BL_, [&](auto R, dim3 grid) { BHG_LAUNCH((travel_time_kernel<R.value>), grid, dim3(64), 0, s, a, t_end, t_cross); });
}
#elif !defined(BHG_TU_TIMELIKE)
hipError_t launch_travel_time(const TraceArgs &a, int rhs, double *t_end, double *t_cross, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_travel_time_kerr(a, t_end, t_cross, s);
    return launch_lanes(a, rhs, [&](auto R, dim3 grid) { BHG_LAUNCH((travel_time_kernel<R.value>), grid, dim3(64), 0, s, a, t_end, t_cross); });
}
#endif

// ------------------------------------------------------------------------------------------
// Triangle meshes (bhg_trace_mesh_device): the trace's steps, unchanged, with a mesh as one more terminal
// event.  A lane-per-ray loop on the shared helpers above; per accepted step [t, t + h]:
//   * the terminal events of the trace (horizon, exit sphere, and -- a disk set -- the opaque disk) are settled by settle_dense;
//   * M = min(BHG_MESH_MAX_SUBSTEPS, max(1, ceil(L / max_chord))), L the Cartesian distance between the step's ends; the dense
//     output is sampled at theta_m = m / M (Kerr: the Cartesian image of the Boyer-Lindquist sample) and consecutive samples are
//     M straight sub-chords, tested in order against the tree (segment_first_hit: smallest s, ties to the smaller index);
//   * sub-chords that start at or behind the terminal root are not looked at;
//   * the first hit is moved onto the curve: brent_root on n_T . (x(lambda) - v0) over the sub-chord's interval (its ends lie on
//     the curve, on opposite sides of the plane or on it); a root later than the terminal root loses to it;
//   * the ray ends there with BHG_FLAG_HIT_OBJECT, end = the dense output at the root (Kerr: Boyer-Lindquist, finalised next),
//     tri_id the triangle, bary the plane coordinates (u, v) of the refined point in it.
// The whole-step cull: the sampled points deviate from the step's straight chord, per component, by at most
// |h| (|qx1| / 4 + 0.385 |qx2| + 0.4725 |qx3|) (the maxima of th (1 - th), th (1 - th^2), th (1 - th^3) on [0, 1]); the box of
// the step's ends widened by that holds every sub-chord, and a step whose box misses the root box has no hit.  Kerr: the same
// bound on r, against the mesh's range of distances from the origin (a point at Boyer-Lindquist r lies at a Cartesian distance
// in [r, sqrt(r^2 + a^2)]).
// Disk off, a ray that meets no triangle has the plain trace's end / flags / n_steps / n_accepted bit for bit (the exit sphere's
// certified Newton search: exit_as_plain_trace).
// ------------------------------------------------------------------------------------------
template <int RHS>
__device__ __forceinline__ void mesh_point(const TraceArgs &A, const Dense &d, double t, double c[3])
{
    if (RHS == BHG_RHS_KERR_BL_) {
        double q[3];
        dense_pos(d, t, q);
        bl_position_to_cart(A.spin, q, c);
    } else {
        dense_pos(d, t, c);
    }
}

// may the step's polyline meet the mesh at all?
template <int RHS>
__device__ __forceinline__ bool mesh_step_candidate(const MeshArgs &G, const Dense &d, const double x0[3], const double x1[3],
                                                    const double c0[3], const double c1[3], double spin)
{
    const double ah = fabs(d.h);
    if (RHS == BHG_RHS_KERR_BL_) {
        // the spans of r, theta, phi over the step's samples: |end - start| + twice the deviation from the straight line
        double span[3], dev_r = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double dev = ah * (0.25 * fabs(d.qx[1][c]) + 0.385 * fabs(d.qx[2][c]) + 0.4725 * fabs(d.qx[3][c]));
            span[c] = fabs(x1[c] - x0[c]) + 2.0 * dev;
            if (c == 0) dev_r = dev;
        }
        const double slack = 1e-13 * (1.0 + fabs(x0[0]) + fabs(x1[0]));
        const double r_lo = fmin(x0[0], x1[0]) - dev_r - slack, r_hi = fmax(x0[0], x1[0]) + dev_r + slack;
        if (!(r_lo > 0.0)) return true;
        // every sample lies in the ball of radius sqrt(r_hi^2 + a^2), and so does every sub-chord (a ball is convex)
        const double R_hi = sqrt(r_hi * r_hi + spin * spin) * (1.0 + 1e-13);
        if (R_hi < G.d_min) return false;
        // every sample lies at a distance >= r_lo, but a chord between two such points dips below it: by the embedding's
        // Jacobian (|dx/dr| <= 1, |dx/dtheta|, |dx/dphi| <= sqrt(r^2 + a^2)) no two samples are farther apart than len, and a
        // chord of that length between points at distance >= r_lo stays at distance >= sqrt(r_lo^2 - len^2 / 4)
        const double len = (span[0] + R_hi * (span[1] + span[2])) * (1.0 + 1e-13);
        const double low2 = r_lo * r_lo - 0.25 * len * len;
        return !(low2 > G.d_max * G.d_max * (1.0 + 1e-13));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double dev = ah * (0.25 * fabs(d.qx[1][c]) + 0.385 * fabs(d.qx[2][c]) + 0.4725 * fabs(d.qx[3][c]));
        const double slack = 1e-13 * (1.0 + fabs(c0[c]) + fabs(c1[c]));
        const double lo = fmin(c0[c], c1[c]) - dev - slack, hi = fmax(c0[c], c1[c]) + dev + slack;
        if (lo > G.box[3 + c] || hi < G.box[c]) return false;
    }
    return true;
}

// Where the mesh stands: as it lies -- the trace of section 19 --, or in K rigid placements of the one
// tree.  One ray loop (trace_mesh_ray) asks either for the first hit of a sub-chord, for a point in the frame of the placement
// that was hit, and to keep that placement's index.
struct MeshAsItLies {
    __device__ __forceinline__ int32_t first_hit(const MeshView &M, const double pa[3], const double pb[3], double &s_hit, int32_t &inst) const
    {
        return segment_first_hit<false>(M, pa, pb, s_hit);
    }
    __device__ __forceinline__ void to_local(int32_t, const double c[3], double l[3]) const
    {
        l[0] = c[0];
        l[1] = c[1];
        l[2] = c[2];
    }
    __device__ __forceinline__ void keep(uint64_t, int32_t) const {}
};

// The placements of an instance set: the walk over them is mesh_traverse.h's (wave-uniform, the records by scalar loads).
struct MeshPlacements {
    const MeshInstanceArgs &I;
    __device__ __forceinline__ int32_t first_hit(const MeshView &M, const double pa[3], const double pb[3], double &s_hit, int32_t &inst) const
    {
        return segment_first_hit_instances<false>(M, I.rec, I.n, I.cull != 0, pa, pb, s_hit, inst);
    }
    // (the placement that was hit differs from lane to lane: its record is read as any array is)
    __device__ __forceinline__ void to_local(int32_t inst, const double c[3], double l[3]) const
    {
        instance_into_frame(I.rec + (size_t)inst * BHG_MESH_INSTANCE_DOUBLES_, c, l);
    }
    __device__ __forceinline__ void keep(uint64_t i, int32_t inst) const { I.inst_id[i] = inst; }
};

// The placements of a set under a tree: the walk is per lane, by skip links (mesh_traverse.h).
struct MeshPlacementTree {
    const MeshInstanceTreeArgs &I;
    __device__ __forceinline__ int32_t first_hit(const MeshView &M, const double pa[3], const double pb[3], double &s_hit, int32_t &inst) const
    {
        return segment_first_hit_instance_tree<false>(M, I.tree, I.cull != 0, pa, pb, s_hit, inst);
    }
    __device__ __forceinline__ void to_local(int32_t inst, const double c[3], double l[3]) const
    {
        instance_into_frame(I.tree.rec + (size_t)inst * BHG_MESH_INSTANCE_DOUBLES_, c, l);
    }
    __device__ __forceinline__ void keep(uint64_t i, int32_t inst) const { I.inst_id[i] = inst; }
};

template <int RHS, class Where>
__device__ __forceinline__ void trace_mesh_ray(const TraceArgs &A, const MeshArgs &G, const Where &W)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const bool bl = RHS == BHG_RHS_KERR_BL_;
    const bool disk = A.disk_r_out > 0.0;
    RayState S;
    double xe[3], ve[3];
    if (start_ray<RHS, true>(A, i, S, xe, ve)) {    // final at once
        G.tri_id[i] = -1;
        W.keep(i, -1);
        store_start_inside(A, i, xe, ve);
        return;
    }
    uint32_t flags = 0;
    int32_t tri = -1, inst = -1;
    for (;;) {
        StepTry P;
        const uint32_t st = dp54_attempt<RHS>(A, S, P);
        if (st == DP54_REJECTED) continue;
        if (st != DP54_ACCEPTED) {
            flags = st;
            break;
        }
        bool ev_h, ev_e;
        radial_events(A, S, P, ev_h, ev_e);
        const bool ev_d = disk && crossed_disk_plane<RHS>(S.x, P.xn);
        uint32_t evflag = 0;
        double t_stop = P.t_new;
        Dense d;
        build_dense_pos(d, S.t, P.h, S.x, S.v, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
        if (ev_h || ev_e || ev_d) {
            // the terminal events, settled as the trace kernels settle them (the earliest root wins: horizon, exit, disk)
            const uint32_t kind = (ev_h ? EV_HORIZON : 0u) | (ev_e ? EV_EXIT : 0u) | (ev_d ? EV_DISK : 0u);
            double best;
            int obj;
            evflag = settle_dense<RHS, EVT_EXIT | EVT_DISK>(A, kind, S, P, d, best, obj);
            if (evflag) t_stop = best;
        }
        // the mesh
        double c0[3] = {S.x[0], S.x[1], S.x[2]}, c1[3] = {P.xn[0], P.xn[1], P.xn[2]};
        if (bl) {
            bl_position_to_cart(A.spin, S.x, c0);
            bl_position_to_cart(A.spin, P.xn, c1);
        }
        if (!G.cull || mesh_step_candidate<RHS>(G, d, S.x, P.xn, c0, c1, A.spin)) {
            const double dx = c1[0] - c0[0], dy = c1[1] - c0[1], dz = c1[2] - c0[2];
            const double L = sqrt(dx * dx + dy * dy + dz * dz);
            const double want = ceil(L / G.max_chord);
            // (a NaN or huge quotient takes the cap)
            const int M = !(want < (double)BHG_MESH_MAX_SUBSTEPS_) ? BHG_MESH_MAX_SUBSTEPS_ : (want < 1.0 ? 1 : (int)want);
            double ta = S.t, pa[3];
            mesh_point<RHS>(A, d, ta, pa);
            for (int m = 0; m < M; m++) {
                if (evflag && ta >= t_stop) break;
                const double tb = m + 1 == M ? P.t_new : S.t + (P.h * (double)(m + 1)) / (double)M;
                double pb[3], s_hit;
                mesh_point<RHS>(A, d, tb, pb);
                int32_t on = 0;
                const int32_t hit = W.first_hit(G.mesh, pa, pb, s_hit, on);
                if (hit >= 0) {
                    const double *T = G.mesh.tri + (size_t)G.mesh.tri_slot[hit] * 9;
                    const double e1[3] = {T[3], T[4], T[5]}, e2[3] = {T[6], T[7], T[8]};
                    const double nT[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                    auto g_T = [&](double tq) {
                        double cw[3], c[3];
                        mesh_point<RHS>(A, d, tq, cw);
                        W.to_local(on, cw, c);
                        return nT[0] * (c[0] - T[0]) + nT[1] * (c[1] - T[1]) + nT[2] * (c[2] - T[2]);
                    };
                    // (the ends straddle the plane up to rounding: without a sign change -- both within rounding of the
                    // plane -- the end nearer to it is the root, and Brent's search is never run without its bracket)
                    const double ga = g_T(ta), gb = g_T(tb);
                    double root;
                    if (ga == 0.0)
                        root = ta;
                    else if (gb == 0.0)
                        root = tb;
                    else if ((ga < 0.0) == (gb < 0.0))
                        root = fabs(ga) <= fabs(gb) ? ta : tb;
                    else
                        root = brent_root(g_T, ta, tb);
                    if (!evflag || root <= t_stop) {
                        double cw[3], c[3];
                        mesh_point<RHS>(A, d, root, cw);
                        W.to_local(on, cw, c);
                        const double w[3] = {c[0] - T[0], c[1] - T[1], c[2] - T[2]};
                        const double nn = nT[0] * nT[0] + nT[1] * nT[1] + nT[2] * nT[2];
                        const double we2[3] = {w[1] * e2[2] - w[2] * e2[1], w[2] * e2[0] - w[0] * e2[2], w[0] * e2[1] - w[1] * e2[0]};
                        const double e1w[3] = {e1[1] * w[2] - e1[2] * w[1], e1[2] * w[0] - e1[0] * w[2], e1[0] * w[1] - e1[1] * w[0]};
                        G.bary[i * 2 + 0] = (we2[0] * nT[0] + we2[1] * nT[1] + we2[2] * nT[2]) / nn;
                        G.bary[i * 2 + 1] = (e1w[0] * nT[0] + e1w[1] * nT[1] + e1w[2] * nT[2]) / nn;
                        tri = hit;
                        inst = on;
                        evflag = BHG_FLAG_HIT_OBJECT_;
                        t_stop = root;
                    }
                    // (a root behind the terminal event: that event ends the ray, and every later sub-chord starts behind it)
                    break;
                }
                ta = tb;
                pa[0] = pb[0];
                pa[1] = pb[1];
                pa[2] = pb[2];
            }
        }
        if (evflag) {
            flags = evflag;
            // disk off and no triangle: the plain trace's bits
            if (tri < 0 && exit_as_plain_trace<RHS>(A, i, S, P, ev_h, ev_e)) {
                G.tri_id[i] = -1;
                W.keep(i, -1);
                return;
            }
            build_dense_dir(d, S.a1, P.a2, P.a3, P.a4, P.a5, P.a6, P.a7);
            dense_pos(d, t_stop, xe);
            dense_dir(d, t_stop, ve);
            break;
        }
        if (advance(A, S, P, xe, ve)) {
            flags = BHG_FLAG_REACHED_END_;
            break;
        }
    }
    G.tri_id[i] = tri;
    W.keep(i, inst);
    finish_ray(A, i, S, xe, ve, flags);
}

template <int RHS>
__global__ void __launch_bounds__(64) trace_mesh_kernel(const TraceArgs A, const MeshArgs G)
{
    trace_mesh_ray<RHS>(A, G, MeshAsItLies{});
}

// ... in K rigid placements (bhg_trace_mesh_instances_device): G carries the set's union box and its range of distances
template <int RHS>
__global__ void __launch_bounds__(64) trace_mesh_instances_kernel(const TraceArgs A, const MeshArgs G, const MeshInstanceArgs I)
{
    trace_mesh_ray<RHS>(A, G, MeshPlacements{I});
}

#if defined(BHG_TU_KERR)
hipError_t launch_trace_mesh_kerr(const TraceArgs &a, const MeshArgs &m, hipStream_t s)
{
    return launch_lanes(a, BHG_RHS_KERR_BL_, [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_kernel<R.value>), grid, dim3(64), 0, s, a, m); });
}
#elif !defined(BHG_TU_TIMELIKE)
hipError_t launch_trace_mesh(const TraceArgs &a, const MeshArgs &m, int rhs, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trace_mesh_kerr(a, m, s);
    return launch_lanes(a, rhs, [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_kernel<R.value>), grid, dim3(64), 0, s, a, m); });
}
#endif

#if defined(BHG_TU_KERR)
hipError_t launch_trace_mesh_instances_kerr(const TraceArgs &a, const MeshArgs &m, const MeshInstanceArgs &in, hipStream_t s)
{
    return launch_lanes(a, BHG_RHS_KERR_BL_,
                        [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_instances_kernel<R.value>), grid, dim3(64), 0, s, a, m, in); });
}
#elif !defined(BHG_TU_TIMELIKE)
hipError_t launch_trace_mesh_instances(const TraceArgs &a, const MeshArgs &m, const MeshInstanceArgs &in, int rhs, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trace_mesh_instances_kerr(a, m, in, s);
    return launch_lanes(a, rhs,
                        [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_instances_kernel<R.value>), grid, dim3(64), 0, s, a, m, in); });
}
#endif

// ... the placements under a tree (bhg_trace_mesh_instances_device with a set of bhg_mesh_instances_create_tree)
template <int RHS>
__global__ void __launch_bounds__(64) trace_mesh_instance_tree_kernel(const TraceArgs A, const MeshArgs G, const MeshInstanceTreeArgs I)
{
    trace_mesh_ray<RHS>(A, G, MeshPlacementTree{I});
}

#if defined(BHG_TU_KERR)
hipError_t launch_trace_mesh_instance_tree_kerr(const TraceArgs &a, const MeshArgs &m, const MeshInstanceTreeArgs &in, hipStream_t s)
{
    return launch_lanes(a, BHG_RHS_KERR_BL_,
                        [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_instance_tree_kernel<R.value>), grid, dim3(64), 0, s, a, m, in); });
}
#elif !defined(BHG_TU_TIMELIKE)
hipError_t launch_trace_mesh_instance_tree(const TraceArgs &a, const MeshArgs &m, const MeshInstanceTreeArgs &in, int rhs, hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trace_mesh_instance_tree_kerr(a, m, in, s);
    return launch_lanes(a, rhs,
                        [&](auto R, dim3 grid) { BHG_LAUNCH((trace_mesh_instance_tree_kernel<R.value>), grid, dim3(64), 0, s, a, m, in); });
}
#endif

// ------------------------------------------------------------------------------------------
// Start-up records (bhg_trace_prefix_device).  scipy's start guess h0 is one to two decades below the
// step a ray settles on, and the controller climbs there by its x10 clamp: three to four accepted steps next to the camera,
// a quarter of all the attempts of a frame, whose outcome depends on the ray, the metric, the tolerances, lambda_end and
// max_step -- and on nothing in the scene as long as no event surface comes near.  One LANE per ray takes every ray through
// those leading attempts on the trace kernels' own start and step (start_ray, dp54_attempt, advance: the same bits) and keeps
// the state in front of the first attempt that
//   * is rejected, or ends the ray (lambda_end reached, the step budget, a step too small, NaN: these reject or flag), or
//   * ends farther than rho from the start point, or
//   * would be attempt number BHG_PREFIX_K_MAX_ + 1.
// What is kept is a queue entry (QEntry: x, k, a, |h| to try next, r, lambda, attempted = accepted = depth, bits 0 -- the last
// attempt was accepted), written as seven planes of 16 bytes per ray, rec[p * n + i], so that each of the queue fill's loads
// is contiguous over a wave.  Depth 0 -- a start inside the hole among them -- says "start this ray yourself".
// Every kept step lies in the ball of radius rho about the start point.  The event tests of the step loop act on step ends
// (radii, the sign of z) and on the chord between them (object spheres), and a ball is convex: a trace whose horizon, exit
// sphere, disk plane and object spheres all stay clear of that ball finds no event in these steps, takes them exactly as
// they were taken here, and arrives at the kept state (the C layer holds every replaying call to that: prefix_clearance).
// ------------------------------------------------------------------------------------------
#if !defined(BHG_TU_KERR) && !defined(BHG_TU_TIMELIKE)
// DEEP (BHG_PREFIX_RECORD_DEEP): the record does not stop at a rejected attempt.  A rejected attempt tests no event and moves
// nothing: what it leaves -- the reduced |h|, the `rejected` bit that clamps the next factor to 1, the attempt count -- depends on
// what an accepted step depends on, and the step loop takes a ray in that state from the queue already (the short drain hands
// one back so: PARK_REQUEUE, bit 0 of the entry's last word, which the pop reads).  So the kept state is the one in front of
//   * the first attempt that would end the ray or flag it, or
//   * an accepted attempt that ends farther than rho from the start point (rejections in front of it are kept: same point,
//     smaller h, bit set), or
//   * accepted step number acc_max + 1 (a launch argument: BHG_PREFIX_DEEP_ACCEPTED_ by the deep rule, BHG_PREFIX_WIDE_ACCEPTED_
//     by the wide one, whose larger ball holds up to eight, BHG_PREFIX_RIM_ACCEPTED_ by the rim one) or attempt number att_max + 1
//     (a launch argument too: BHG_PREFIX_DEEP_ATTEMPTS_, or BHG_PREFIX_RIM_ATTEMPTS_ by the rim rule),
// and the last plane is (i, attempted, accepted, rejected).  A record is usable when attempted != 0.
template <int RHS, bool DEEP>
__global__ void __launch_bounds__(64) record_prefix_kernel(const TraceArgs A, double2 *rec, double rho, uint32_t deep_acc_max, uint32_t deep_att_max)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    RayState K;    // the state kept so far
    for (int c = 0; c < 3; c++) K.x[c] = K.v[c] = K.a1[c] = 0.0;
    K.t = K.h_abs = K.r_cur = 0.0;
    K.n_att = K.n_acc = 0;
    K.rejected = false;
    double xe[3], ve[3];
    if (!start_ray<RHS, true>(A, i, K, xe, ve)) {
        const double o[3] = {K.x[0], K.x[1], K.x[2]};
        const double rho2 = rho * rho;
        const uint32_t acc_max = DEEP ? deep_acc_max : (uint32_t)BHG_PREFIX_K_MAX_;
        while (K.n_acc < acc_max && (!DEEP || K.n_att < deep_att_max)) {
            RayState T = K;
            StepTry P;
            const uint32_t st = dp54_attempt<RHS>(A, T, P);
            if (DEEP && st == DP54_REJECTED) {
                K = T;      // (x, v, a1, t as they were: the reduced h_abs, rejected, n_att)
                continue;
            }
            if (st != DP54_ACCEPTED) break;
            const double d[3] = {P.xn[0] - o[0], P.xn[1] - o[1], P.xn[2] - o[2]};
            if (!(__builtin_fma(d[2], d[2], __builtin_fma(d[1], d[1], d[0] * d[0])) <= rho2)) break;
            if (advance(A, T, P, xe, ve)) break;
            K = T;
        }
    }
    const uint64_t n = A.n;
    rec[0 * n + i] = make_double2(K.x[0], K.x[1]);
    rec[1 * n + i] = make_double2(K.x[2], K.v[0]);
    rec[2 * n + i] = make_double2(K.v[1], K.v[2]);
    rec[3 * n + i] = make_double2(K.a1[0], K.a1[1]);
    rec[4 * n + i] = make_double2(K.a1[2], K.h_abs);
    rec[5 * n + i] = make_double2(K.r_cur, K.t);
    reinterpret_cast<uint4 *>(rec)[6 * n + i] = make_uint4((uint32_t)i, K.n_att, K.n_acc, K.rejected ? 1u : 0u);
}

hipError_t launch_record_prefix(const TraceArgs &a, int rhs, void *rec, double rho, bool deep, uint32_t acc_max, uint32_t att_max,
                                hipStream_t s)
{
    if (deep && (acc_max < 1u || acc_max > att_max || att_max > (uint32_t)BHG_PREFIX_RIM_ATTEMPTS_)) return hipErrorInvalidValue;
    return launch_lanes(a, rhs, [&](auto R, dim3 grid) {
        if (deep)
            BHG_LAUNCH((record_prefix_kernel<R.value, true>), grid, dim3(64), 0, s, a, (double2 *)rec, rho, acc_max, att_max);
        else
            BHG_LAUNCH((record_prefix_kernel<R.value, false>), grid, dim3(64), 0, s, a, (double2 *)rec, rho, 0u, 0u);
    });
}
#endif

// ------------------------------------------------------------------------------------------
// Acceleration probe (tests compare the device RHS with the oracle's)
// ------------------------------------------------------------------------------------------
template <int RHS>
__global__ void accel_kernel(const double *x, const double *k, double r_s, uint64_t n, double *acc)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double px[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
    double pk[3] = {k[3 * i], k[3 * i + 1], k[3 * i + 2]};
    double a[3], r;
    const Metric met = metric_of(r_s, 0.0);
    accel<RHS>(px, pk, met, a, r);
    acc[3 * i] = a[0];
    acc[3 * i + 1] = a[1];
    acc[3 * i + 2] = a[2];
}

// ------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------
template <int RHS, int EVT>
static hipError_t launch_variant(const TraceArgs &a, int method, int grid, hipStream_t s, hipEvent_t *ev)
{
    // No launch ahead of this one: the trace kernel's waves work out the start records themselves while they fill their ray
    // queues (converged, 64 lanes wide; Kerr: Cartesian -> Boyer-Lindquist, E and L, kerr_cart_to_bl).  ev[0] and ev[1] stay
    // back to back so that the three timing slots keep their meaning (bhg_last_pass_ms: slot 0, once a pass of its own, is ~0).
    if (ev) {
        (void)hipEventRecord(ev[0], s);
        (void)hipEventRecord(ev[1], s);
    }
    if (method == BHG_METHOD_RK4_)
        BHG_LAUNCH((trace_rk4_kernel<RHS, EVT>), dim3(grid), dim3(64), 0, s, a);
    else
        BHG_LAUNCH((trace_dp54_kernel<RHS, EVT>), dim3(grid), dim3(64), 0, s, a);
    if (ev) (void)hipEventRecord(ev[2], s);
    return hipGetLastError();
}

#ifdef BHG_TU_KERR
// Kerr: once ALL passes of a call are done, turn the Boyer-Lindquist end states into Cartesian ones
hipError_t launch_kerr_finalize(const TraceArgs &a, double *dir_out, hipStream_t s)
{
    if (a.n == 0) return hipSuccess;
    BHG_LAUNCH(kerr_finalize_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a, dir_out);
    return hipGetLastError();
}
#endif

template <int RHS, int EVT>
static hipError_t occupancy_variant(int method, int *blocks_per_cu)
{
    if (method == BHG_METHOD_RK4_)
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, trace_rk4_kernel<RHS, EVT>, 64, 0);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, trace_dp54_kernel<RHS, EVT>, 64, 0);
}

#ifdef BHG_TU_KERR
// Kerr: horizon, optional exit sphere, optional disk; object spheres in the all-events variant
hipError_t launch_trace_kerr(const TraceArgs &a, int method, int evt, int grid, hipStream_t s, hipEvent_t *ev)
{
    if (evt & 4) return launch_variant<BHG_RHS_KERR_BL_, 7>(a, method, grid, s, ev);   // object spheres: the all-events variant
    switch (evt & 3) {
    case 0: return launch_variant<BHG_RHS_KERR_BL_, 0>(a, method, grid, s, ev);
    case 1: return launch_variant<BHG_RHS_KERR_BL_, 1>(a, method, grid, s, ev);
    default: return launch_variant<BHG_RHS_KERR_BL_, 3>(a, method, grid, s, ev);
    }
}

hipError_t trace_occupancy_kerr(int method, int evt, int *blocks_per_cu)
{
    if (evt & 4) return occupancy_variant<BHG_RHS_KERR_BL_, 7>(method, blocks_per_cu);
    switch (evt & 3) {
    case 0: return occupancy_variant<BHG_RHS_KERR_BL_, 0>(method, blocks_per_cu);
    case 1: return occupancy_variant<BHG_RHS_KERR_BL_, 1>(method, blocks_per_cu);
    default: return occupancy_variant<BHG_RHS_KERR_BL_, 3>(method, blocks_per_cu);
    }
}
#elif defined(BHG_TU_TIMELIKE)
// time_like = True in the Cartesian Christoffel form (geodesic_kernels_timelike.hip): a translation unit of its own with ONE
// event variant, 7 -- exit sphere, disk and object spheres all tested at run time.  Massive-particle orbits are the
// plotting path (README Fig. 5/6 style curves), not the frame path: they need to be right, not to be tuned per event set.
hipError_t launch_trace_timelike(const TraceArgs &a, int method, int grid, hipStream_t s, hipEvent_t *ev)
{
    return launch_variant<BHG_RHS_CHRISTOFFEL_TL_, 7>(a, method, grid, s, ev);
}

hipError_t trace_occupancy_timelike(int method, int *blocks_per_cu)
{
    return occupancy_variant<BHG_RHS_CHRISTOFFEL_TL_, 7>(method, blocks_per_cu);
}

hipError_t launch_accel_timelike(const double *x, const double *k, double r_s, uint64_t n, double *acc, hipStream_t s)
{
    const int grid = (int)((n + 255) / 256);
    if (grid == 0) return hipSuccess;
    BHG_LAUNCH((accel_kernel<BHG_RHS_CHRISTOFFEL_TL_>), dim3(grid), dim3(256), 0, s, x, k, r_s, n, acc);
    return hipGetLastError();
}
#else
template <int RHS>
static hipError_t launch_rhs(const TraceArgs &a, int method, int evt, int grid, hipStream_t s, hipEvent_t *ev)
{
    switch (evt) {
    case 0: return launch_variant<RHS, 0>(a, method, grid, s, ev);
    case 1: return launch_variant<RHS, 1>(a, method, grid, s, ev);
    case 2: return launch_variant<RHS, 2>(a, method, grid, s, ev);
    case 3: return launch_variant<RHS, 3>(a, method, grid, s, ev);
    case 5: return launch_variant<RHS, 5>(a, method, grid, s, ev);   // exit sphere + objects, no disk (config 4)
    default: return launch_variant<RHS, 7>(a, method, grid, s, ev);
    }
}

template <int RHS>
static hipError_t occupancy_rhs(int method, int evt, int *blocks_per_cu)
{
    switch (evt) {
    case 0: return occupancy_variant<RHS, 0>(method, blocks_per_cu);
    case 1: return occupancy_variant<RHS, 1>(method, blocks_per_cu);
    case 2: return occupancy_variant<RHS, 2>(method, blocks_per_cu);
    case 3: return occupancy_variant<RHS, 3>(method, blocks_per_cu);
    case 5: return occupancy_variant<RHS, 5>(method, blocks_per_cu);
    default: return occupancy_variant<RHS, 7>(method, blocks_per_cu);
    }
}

hipError_t launch_trace(const TraceArgs &a, int method, int rhs, int evt, int grid, hipStream_t s, hipEvent_t *ev)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_trace_kerr(a, method, evt, grid, s, ev);
    if (rhs == BHG_RHS_CHRISTOFFEL_TL_) return launch_trace_timelike(a, method, grid, s, ev);
    return rhs == BHG_RHS_REDUCED_ ? launch_rhs<BHG_RHS_REDUCED_>(a, method, evt, grid, s, ev)
                                   : launch_rhs<BHG_RHS_CHRISTOFFEL_>(a, method, evt, grid, s, ev);
}

hipError_t trace_occupancy(int method, int rhs, int evt, int *blocks_per_cu)
{
    if (rhs == BHG_RHS_KERR_BL_) return trace_occupancy_kerr(method, evt, blocks_per_cu);
    if (rhs == BHG_RHS_CHRISTOFFEL_TL_) return trace_occupancy_timelike(method, blocks_per_cu);
    return rhs == BHG_RHS_REDUCED_ ? occupancy_rhs<BHG_RHS_REDUCED_>(method, evt, blocks_per_cu)
                                   : occupancy_rhs<BHG_RHS_CHRISTOFFEL_>(method, evt, blocks_per_cu);
}

hipError_t launch_accel(const double *x, const double *k, double r_s, double spin, double mu2, uint64_t n, double *acc, int rhs,
                        hipStream_t s)
{
    if (rhs == BHG_RHS_KERR_BL_) return launch_accel_kerr(x, k, r_s, spin, mu2, n, acc, s);
    if (rhs == BHG_RHS_CHRISTOFFEL_TL_) return launch_accel_timelike(x, k, r_s, n, acc, s);
    int grid = (int)((n + 255) / 256);
    if (grid == 0) return hipSuccess;
    if (rhs == BHG_RHS_REDUCED_)
        BHG_LAUNCH((accel_kernel<BHG_RHS_REDUCED_>), dim3(grid), dim3(256), 0, s, x, k, r_s, n, acc);
    else
        BHG_LAUNCH((accel_kernel<BHG_RHS_CHRISTOFFEL_>), dim3(grid), dim3(256), 0, s, x, k, r_s, n, acc);
    return hipGetLastError();
}
#endif  // BHG_TU_KERR

}  // namespace bhg

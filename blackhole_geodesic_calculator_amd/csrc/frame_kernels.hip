// frame_kernels.hip -- the data-parallel stages either side of the geodesic solve, on device:
//   * camera-ray generation with the reference's multisample jitter
//     (raytracer/RelativisticRenderEngine.py:185-188, :224-230), from a device-resident MT19937
//     jitter stream (produced once on the host from Python's own seeded state, bit-identical);
//   * escaping-ray shading against an equirectangular sky (background_hit, :366-378) and the
//     per-pixel multisample mean (sbuf += colour; buf = sbuf/(s+1), :242-250); rays that ended on the
//     thin disk get the Limited engine's disk colour (LimitedRelativisticRenderEngine.py:427-436, :300),
//     rays that ended on an object sphere the Lambert lamp sum of spacetime_hit (:356-363).
// Ray generation is an HBM-bound element-wise kernel.  The shade kernel runs one thread per RAY and stages the S samples of
// a pixel in LDS, where one thread sums them in sample order (the reference's order: the result is deterministic).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geodesic_kernels.h"
#include "device_math.h"
#include "kerr_start.h"

namespace bhg {

// d = (x_r + dx (u1 - 1/2), y_r + dy (u2 - 1/2), -1), rotated; ray i of P pixels.  Operation order follows the host
// restatement (raygen.py) so that an unrotated camera gives bit-identical directions (the library is built with
// -ffp-contract=off).  The caller divides by |d|.
__device__ __forceinline__ double3 pinhole_dir(const RaygenArgs &A, uint64_t i, uint64_t P)
{
    const uint64_t s = i / P, p = i - s * P;
    const int64_t pix = A.pixels ? A.pixels[p] : (int64_t)p;
    const int64_t py = pix / A.width, px = pix - py * A.width;
    const double W = (double)A.width, H = (double)A.height;
    const double aspect = H / W;
    const double dy = aspect / H, dx = 1.0 / W;
    const uint64_t j = A.compact ? i * 2 : (s * (uint64_t)A.width * (uint64_t)A.height + (uint64_t)pix) * 2;
    const double u1 = A.jitter ? A.jitter[j] : 0.5, u2 = A.jitter ? A.jitter[j + 1] : 0.5;
    const double x_render = A.fov_x * (double)(px - (int64_t)(A.width / 2)) / W;
    const double y_render = A.fov_y * (double)(py - (int64_t)(A.height / 2)) / H * aspect;
    double d0 = x_render + dx * (u1 - 0.5);
    double d1 = y_render + dy * (u2 - 0.5);
    double d2 = -1.0;
    if (A.rotate) {
        const double e0 = A.rot[0] * d0 + A.rot[1] * d1 + A.rot[2] * d2;
        const double e1 = A.rot[3] * d0 + A.rot[4] * d1 + A.rot[5] * d2;
        const double e2 = A.rot[6] * d0 + A.rot[7] * d1 + A.rot[8] * d2;
        d0 = e0;
        d1 = e1;
        d2 = e2;
    }
    return make_double3(d0, d1, d2);
}

// ---- the observer camera -----------------------------------------------------------------------
// Kerr ZAMO at BL (r, theta): lapse alpha = sqrt(Sigma Delta / A) and frame-dragging rate omega = 2 M a r / A
__device__ __forceinline__ void kerr_zamo(double M, double a, double r, double c2, double &alpha, double &omega)
{
    const double a2 = a * a, s2 = 1.0 - c2;
    const double Sig = r * r + a2 * c2, Del = r * r - 2.0 * M * r + a2;
    const double A = (r * r + a2) * (r * r + a2) - a2 * Del * s2;
    alpha = sqrt(Sig * Del / A);
    omega = 2.0 * M * a * r / A;
}

// Aberration, the observer's rest frame -> the ZAMO's: a unit look direction n' of an observer moving with beta gives
//     n = (n' + gamma^2 / (gamma + 1) (n'.beta) beta - gamma beta) / (gamma (1 - beta.n'))
// (point 2 of section 10 with (gamma - 1) beta_hat beta_hat = gamma^2 / (gamma + 1) beta beta: no division by |beta|).
// c = gamma^2 / (gamma + 1).
__device__ __forceinline__ void aberrate(const double b[3], double gamma, double c, const double np[3], double n[3])
{
    const double bn = b[0] * np[0] + b[1] * np[1] + b[2] * np[2];
    const double iE = 1.0 / (gamma * (1.0 - bn));
    const double cb = c * bn - gamma;
    n[0] = (np[0] + cb * b[0]) * iE;
    n[1] = (np[1] + cb * b[1]) * iE;
    n[2] = (np[2] + cb * b[2]) * iE;
}

// The camera's ZAMO tetrad as an affine map of a ZAMO-frame look direction n to the coordinate direction k = T n + B
// (up to the scale the caller normalises away).  Kerr: n = n_r r^ + n_th th^ + n_ph ph^ in the Euclidean spherical basis at
// the camera's BL angles, (k^r, k^th, k^ph) = (sqrt(Delta / Sigma) n_r, n_th / sqrt(Sigma), omega / alpha + n_ph sqrt(Sigma) /
// (sqrt(A) sin th)) mapped through the Jacobian of x = R sin th cos ph, y = R sin th sin ph, z = r cos th (R = sqrt(r^2 +
// a^2)); the sin th of the phi column cancels.  Schwarzschild (both Cartesian forms): T = 1 - (1 - sqrt f) r^ r^, B = 0 --
// what the Kerr map gives at a = 0.  The BL position comes from kerr_cart_to_bl itself (its E and L are not used).
__device__ __forceinline__ void camera_tetrad(const ObserverParams &O, double T[9], double B[3])
{
    const double x = O.x0[0], y = O.x0[1], z = O.x0[2];
    if (O.rhs != BHG_RHS_KERR_BL_) {
        const double rc = sqrt(x * x + y * y + z * z), ir = 1.0 / rc;
        const double rh[3] = {x * ir, y * ir, z * ir};
        const double q = 1.0 - sqrt(1.0 - O.r_s * ir);   // 1 - sqrt f
        for (int u = 0; u < 3; u++)
            for (int v = 0; v < 3; v++) T[u * 3 + v] = (u == v ? 1.0 : 0.0) - q * rh[u] * rh[v];
        B[0] = B[1] = B[2] = 0.0;
        return;
    }
    const double a = O.spin, M = 0.5 * O.r_s, a2 = a * a;
    double px[3] = {x, y, z}, pk[3] = {0.0, 0.0, 1.0}, E, L;
    kerr_cart_to_bl(a, M, 0.0, px, pk, E, L);
    const double r = px[0];
    double st, ct;
    sincos_pi4(px[1], st, ct);
    const double iw = rsqrt_nr(__builtin_fma(y, y, x * x)), cp = x * iw, sp = y * iw;
    double alpha, omega;
    kerr_zamo(M, a, r, ct * ct, alpha, omega);
    const double Sig = __builtin_fma(a2 * ct, ct, r * r), Del = __builtin_fma(-2.0 * M, r, r * r + a2);
    const double R2 = r * r + a2, R = sqrt(R2);
    const double Aq = R2 * R2 - a2 * Del * st * st;
    const double sS = sqrt(Sig), cr = sqrt(Del / Sig), cth = 1.0 / sS, cph = sS / sqrt(Aq);   // (cph: times R, over sin th)
    // Jacobian columns, scaled: cr d(x)/dr, cth d(x)/dth, cph d(x)/dph / sin th
    const double Jr[3] = {cr * (r / R) * st * cp, cr * (r / R) * st * sp, cr * ct};
    const double Jt[3] = {cth * R * ct * cp, cth * R * ct * sp, -cth * r * st};
    const double Jp[3] = {-cph * R * sp, cph * R * cp, 0.0};
    const double rh[3] = {st * cp, st * sp, ct}, th[3] = {ct * cp, ct * sp, -st}, ph[3] = {-sp, cp, 0.0};
    for (int u = 0; u < 3; u++)
        for (int v = 0; v < 3; v++) T[u * 3 + v] = Jr[u] * rh[v] + Jt[u] * th[v] + Jp[u] * ph[v];
    const double wB = omega / alpha * R * st;   // (omega / alpha) d(x)/dphi
    B[0] = -wB * sp;
    B[1] = wB * cp;
    B[2] = 0.0;
}

// OBS = false: the reference's camera, k0 = d / |d|.  OBS = true: d / |d| is the moving observer's rest-frame look direction
// n', aberrated to the ZAMO frame and put through the camera tetrad, k0 = (T n + B) / |T n + B|.  The tetrad is one per
// launch: the observer instance walks the rays grid-stride and forms it once per thread (a few hundred instructions, against
// about a hundred per ray for the pinhole direction, the boost and the map).
template <bool OBS>
__global__ void __launch_bounds__(256) raygen_kernel(const RaygenArgs A)
{
    const uint64_t P = A.n_pixels;
    if (!OBS) {
        const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= P * (uint64_t)A.samples) return;
        const double3 d = pinhole_dir(A, i, P);
        const double d0 = d.x, d1 = d.y, d2 = d.z;
        const double nrm = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        double *o = A.k0 + i * 3;
        o[0] = d0 / nrm;
        o[1] = d1 / nrm;
        o[2] = d2 / nrm;
        return;
    }
    const uint64_t N = P * (uint64_t)A.samples;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    double T[9], B[3];
    camera_tetrad(A.obs, T, B);
    const double *b = A.obs.beta;
    const double gamma = 1.0 / sqrt(1.0 - (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
    const double c = gamma * gamma / (gamma + 1.0);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        const double3 d = pinhole_dir(A, i, P);
        const double d0 = d.x, d1 = d.y, d2 = d.z;
        const double inrm = 1.0 / sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double np[3] = {d0 * inrm, d1 * inrm, d2 * inrm};
        double n[3];
        aberrate(b, gamma, c, np, n);
        const double k0 = __builtin_fma(T[0], n[0], __builtin_fma(T[1], n[1], __builtin_fma(T[2], n[2], B[0])));
        const double k1 = __builtin_fma(T[3], n[0], __builtin_fma(T[4], n[1], __builtin_fma(T[5], n[2], B[1])));
        const double k2 = __builtin_fma(T[6], n[0], __builtin_fma(T[7], n[1], __builtin_fma(T[8], n[2], B[2])));
        const double ik = rsqrt_nr(__builtin_fma(k0, k0, __builtin_fma(k1, k1, k2 * k2)));
        double *o = A.k0 + i * 3;
        o[0] = k0 * ik;
        o[1] = k1 * ik;
        o[2] = k2 * ik;
    }
}

// Bilinear lookup in an equirectangular RGBA float32 image.  Texture coordinates (u, v) in
// [-1, 1]^2 as background_hit passes them to Texture.evaluate (:375): u wraps, v clamps.
// (Blender's own texture filter cannot be reproduced outside Blender; this definition is the
// build's own and is restated in numpy in device_frame.py for the parity test.)
__device__ __forceinline__ void sky_lookup(const float *sky, int TW, int TH, double u, double v, double rgb[3])
{
    const double TWd = (double)TW;
    double fx = (u + 1.0) * 0.5 * TWd - 0.5;
    double fy = (v + 1.0) * 0.5 * (double)TH - 0.5;
    double x0f = floor(fx), y0f = floor(fy);
    double ax = fx - x0f, ay = fy - y0f;
    // column x0f mod TW (u wraps) in floating point -- the columns are small integers held exactly, the quotient's
    // rounding can only be off by one period, which the two selects put right; a 64-bit integer remainder is a
    // hundred-instruction sequence on this machine
    double xw = __builtin_fma(-TWd, floor(x0f * (1.0 / TWd)), x0f);
    xw = xw < 0.0 ? xw + TWd : (xw >= TWd ? xw - TWd : xw);
    const int x0 = (int)xw;
    const int x1 = (x0 + 1 == TW) ? 0 : x0 + 1;
    const double THm = (double)(TH - 1);
    const int y0 = (int)fmin(fmax(y0f, 0.0), THm), y1 = (int)fmin(fmax(y0f + 1.0, 0.0), THm);
    const float4 t00 = reinterpret_cast<const float4 *>(sky)[(long)y0 * TW + x0];
    const float4 t01 = reinterpret_cast<const float4 *>(sky)[(long)y0 * TW + x1];
    const float4 t10 = reinterpret_cast<const float4 *>(sky)[(long)y1 * TW + x0];
    const float4 t11 = reinterpret_cast<const float4 *>(sky)[(long)y1 * TW + x1];
    const double w00 = (1.0 - ax) * (1.0 - ay), w01 = ax * (1.0 - ay), w10 = (1.0 - ax) * ay, w11 = ax * ay;
    rgb[0] = __builtin_fma(w11, (double)t11.x, __builtin_fma(w10, (double)t10.x, __builtin_fma(w01, (double)t01.x, w00 * (double)t00.x)));
    rgb[1] = __builtin_fma(w11, (double)t11.y, __builtin_fma(w10, (double)t10.y, __builtin_fma(w01, (double)t01.y, w00 * (double)t00.y)));
    rgb[2] = __builtin_fma(w11, (double)t11.z, __builtin_fma(w10, (double)t10.z, __builtin_fma(w01, (double)t01.z, w00 * (double)t00.z)));
}

// Disk colour (LimitedRelativisticRenderEngine.py:427-436, :300): texture(texture_x, scale) * intensity with a
// Gaussian radial profile.  (y_disk / |y_disk| is NaN at y = 0 there; here the sign of +0 is +.)
__device__ __forceinline__ void disk_colour(const ShadeArgs &A, const double *e, double rgb[3])
{
    const double x = e[0], y = e[1];
    const double R = sqrt(x * x + y * y);
    const double scale = (R - A.disk_r_in) / (A.disk_r_out - A.disk_r_in);
    const double dm = scale - A.disk_mean;
    const double intensity = A.disk_intensity * exp(-(dm * dm) / (2.0 * A.disk_stddev * A.disk_stddev)) /
                             sqrt(2.0 * M_PI * A.disk_stddev);
    double cx = x / R;
    cx = cx > 1.0 ? 1.0 : (cx < -1.0 ? -1.0 : cx);
    const double texture_x = (A.disk_phase + acos(cx) * (y < 0.0 ? -1.0 : 1.0)) / M_PI;
    if (A.disk_tex)
        sky_lookup(A.disk_tex, A.disk_w, A.disk_h, texture_x, scale, rgb);
    else
        rgb[0] = rgb[1] = rgb[2] = 1.0;
    rgb[0] *= intensity;
    rgb[1] *= intensity;
    rgb[2] *= intensity;
}
// ... its twin at another phase: the retarded layers' 
__device__ __forceinline__ void disk_colour_at(const ShadeArgs &A, const double *e, double phase, double rgb[3])
{
    const double x = e[0], y = e[1];
    const double R = sqrt(x * x + y * y);
    const double scale = (R - A.disk_r_in) / (A.disk_r_out - A.disk_r_in);
    const double dm = scale - A.disk_mean;
    const double intensity = A.disk_intensity * exp(-(dm * dm) / (2.0 * A.disk_stddev * A.disk_stddev)) /
                             sqrt(2.0 * M_PI * A.disk_stddev);
    double cx = x / R;
    cx = cx > 1.0 ? 1.0 : (cx < -1.0 ? -1.0 : cx);
    const double texture_x = (phase + acos(cx) * (y < 0.0 ? -1.0 : 1.0)) / M_PI;
    if (A.disk_tex)
        sky_lookup(A.disk_tex, A.disk_w, A.disk_h, texture_x, scale, rgb);
    else
        rgb[0] = rgb[1] = rgb[2] = 1.0;
    rgb[0] *= intensity;
    rgb[1] *= intensity;
    rgb[2] *= intensity;
}

// Object colour: pure Lambert sum over point lamps with 1/d^2 falloff, light paths straight (flat space) as in
// spacetime_hit (RelativisticRenderEngine.py:341-363: base_color = intensity, colour += base_color * intensity *
// n.l / d^2 unless a shadow ray from loc + eps * l hits something -- here: one of the other spheres).  n.l is
// clamped at 0 (the reference adds negative light on the far side; "This needs some serius work", :320).
__device__ __forceinline__ void object_colour(const ShadeArgs &A, const double *e, int j, double rgb[3])
{
    rgb[0] = rgb[1] = rgb[2] = 0.0;
    if (j < 0 || j >= A.n_spheres) return;
    const double *sp = A.spheres[j];
    const double inv_rho = 1.0 / sp[3];
    const double n[3] = {(e[0] - sp[0]) * inv_rho, (e[1] - sp[1]) * inv_rho, (e[2] - sp[2]) * inv_rho};
    double sum = 0.0;
    for (int l = 0; l < A.n_lamps; l++) {
        const double lv[3] = {A.lamps[l][0] - e[0], A.lamps[l][1] - e[1], A.lamps[l][2] - e[2]};
        const double d2 = lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2];
        const double dist = sqrt(d2);
        const double ld[3] = {lv[0] / dist, lv[1] / dist, lv[2] / dist};
        const double ndl = n[0] * ld[0] + n[1] * ld[1] + n[2] * ld[2];
        if (!(ndl > 0.0)) continue;
        bool shadow = false;
        for (int q = 0; q < A.n_spheres; q++) {
            if (q == j) continue;
            const double *sq = A.spheres[q];
            const double oc[3] = {e[0] - sq[0], e[1] - sq[1], e[2] - sq[2]};
            const double b = oc[0] * ld[0] + oc[1] * ld[1] + oc[2] * ld[2];
            const double cq = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - sq[3] * sq[3];
            const double disc = b * b - cq;
            if (disc > 0.0) {
                const double sd = sqrt(disc);
                const double t0 = -b - sd, t1 = -b + sd;
                if ((t0 > 1e-5 && t0 < dist) || (t0 <= 1e-5 && t1 > 1e-5)) shadow = true;  // enters on the way, or starts inside
            }
        }
        if (!shadow) sum += A.lamps[l][3] * A.lamps[l][3] * ndl / d2;
    }
    rgb[0] = A.sphere_rgb[j][0] * sum;
    rgb[1] = A.sphere_rgb[j][1] * sum;
    rgb[2] = A.sphere_rgb[j][2] * sum;
}

// The textured object colour: the texel is read at the angles of the body-frame normal n_b = R_j^T n in
// the sky's convention -- U = atan2(n_b,y, n_b,x) / pi (body +x the image's centre column), V = 1 - 2 atan2(sqrt(n_b,x^2 +
// n_b,y^2), n_b,z) / pi (body +z the top row), both scale-free atan2's as for the sky; a slot without a texture has a white
// texel.  Lit: object_colour (sphere_rgb[j] times the lamp sum) times the texel; emissive: emission[j] * sphere_rgb[j] * texel,
// no lamps, no shadows.  A white texel is an exact x 1.0: an untextured lit slot is object_colour bit for bit.  j is per lane:
// the slot's members are read with a per-lane index, as spheres[j] is.
__device__ __forceinline__ void object_colour_tex(const ShadeArgs &A, const double *e, int j, double rgb[3])
{
    rgb[0] = rgb[1] = rgb[2] = 0.0;
    if (j < 0 || j >= A.n_spheres) return;
    double texel[3] = {1.0, 1.0, 1.0};
    const float *tex = A.ot.tex[j];
    if (tex) {
        const double *sp = A.spheres[j], *R = A.ot.rot[j];
        const double inv_rho = 1.0 / sp[3];
        const double n[3] = {(e[0] - sp[0]) * inv_rho, (e[1] - sp[1]) * inv_rho, (e[2] - sp[2]) * inv_rho};
        const double b0 = R[0] * n[0] + R[3] * n[1] + R[6] * n[2];
        const double b1 = R[1] * n[0] + R[4] * n[1] + R[7] * n[2];
        const double b2 = R[2] * n[0] + R[5] * n[1] + R[8] * n[2];
        const double U = atan2_fast(b1, b0) * 0.3183098861837907;
        const double V = 1.0 - 2.0 * (atan2_fast(sqrt(b0 * b0 + b1 * b1), b2) * 0.3183098861837907);
        sky_lookup(tex, A.ot.tex_w[j], A.ot.tex_h[j], U, V, texel);
    }
    if (A.ot.mode[j] == BHG_OBJECT_EMISSIVE_) {
        const double k = A.ot.emission[j];
        rgb[0] = k * (A.sphere_rgb[j][0] * texel[0]);
        rgb[1] = k * (A.sphere_rgb[j][1] * texel[1]);
        rgb[2] = k * (A.sphere_rgb[j][2] * texel[2]);
        return;
    }
    object_colour(A, e, j, rgb);
    rgb[0] *= texel[0];
    rgb[1] *= texel[1];
    rgb[2] *= texel[2];
}

// ---- redshift ---------------------------------------------------------------------------------
// g = nu_obs / nu_em = (k.u_obs) / (k.u_em) of one ray, fp64.  The observer is the ZAMO at the camera (in Schwarzschild the
// static observer); the Killing constants E = -k_t, L = k_phi come from the CAMERA state (x_c, k0), where the trace starts
// the ray: they are constants of the motion, and the integrator's drift of them stays out of g.  The emitter, by class:
//   RS_DISK    Keplerian circular orbit of sense s at the hit radius (down to the photon orbit: inside the ISCO too)
//   RS_OBJECT  at rest on the sphere (Schwarzschild: static; Kerr: the ZAMO at the hit point)
//   RS_SKY     at rest at infinity
// RS_DARK (horizon, start inside) gives 0, RS_NAN gives NaN.  e = the end position (disk / object classes only).
enum RayClass { RS_DARK = 0, RS_DISK = 1, RS_OBJECT = 2, RS_SKY = 3, RS_NAN = 4 };

// the class bhg_redshift_device gives a ray of these flags (the shade kernels use the branch ray_colour takes instead)
__device__ __forceinline__ int ray_class(uint32_t fl)
{
    if (fl & (BHG_FLAG_HIT_HORIZON_ | BHG_FLAG_START_INSIDE_)) return RS_DARK;
    if (fl & BHG_FLAG_NAN_) return RS_NAN;
    if (fl == BHG_FLAG_HIT_OBJECT_) return RS_OBJECT;
    if (fl == BHG_FLAG_HIT_DISK_) return RS_DISK;
    return RS_SKY;   // exit sphere, lambda_end reached, step cap, stall: the shader colours them from the sky
}

__device__ double redshift_g(const RedshiftParams &P, const double xc[3], const double kc[3], int cls, const double *e)
{
    if (cls == RS_DARK) return 0.0;
    if (cls == RS_NAN || (cls != RS_SKY && !e)) return __builtin_nan("");
    // The camera receives the traced ray run backwards.  Kerr is invariant under (t, phi) -> (-t, -phi), so that photon has the
    // traced ray's E and L and runs the traced curve mirrored in phi, where a disk of sense s is the traced picture's disk of
    // sense -s: the formulas below are the traced ray's, k.u of the TRACED picture, with the sense reversed.
    const double M = 0.5 * P.r_s, s = -P.sense;
    if (P.rhs == BHG_RHS_KERR_BL_) {
        const double a = P.spin;
        double px[3] = {xc[0], xc[1], xc[2]}, pk[3] = {kc[0], kc[1], kc[2]}, E, L;
        kerr_cart_to_bl(a, M, 0.0, px, pk, E, L);     // the trace's own E and L, bit for bit
        const double b = L / E;
        double st, ct, alpha_c, omega_c;
        sincos_pi4(px[1], st, ct);
        kerr_zamo(M, a, px[0], ct * ct, alpha_c, omega_c);
        const double O = (1.0 - omega_c * b) / alpha_c;   // -k.u_obs / E
        if (cls == RS_SKY) return O;
        const double R2 = e[0] * e[0] + e[1] * e[1];
        if (cls == RS_DISK) {
            const double r = sqrt(R2 - a * a), sr = sqrt(r), r32 = r * sr, saM = s * a * sqrt(M);
            const double Om = s * sqrt(M) / (r32 + saM);
            const double ut = (r32 + saM) / (sqrt(r32) * sqrt(r32 - 3.0 * M * sr + 2.0 * saM));
            return O / (ut * (1.0 - Om * b));
        }
        // object: BL r, cos theta of the Cartesian hit point (x = sqrt(r^2 + a^2) sin th cos ph, z = r cos th)
        const double z = e[2], bb = R2 + z * z - a * a;
        const double r = sqrt(0.5 * (bb + sqrt(bb * bb + 4.0 * a * a * z * z)));
        const double c = z / r;
        double alpha_h, omega_h;
        kerr_zamo(M, a, r, c * c, alpha_h, omega_h);
        return O * alpha_h / (1.0 - omega_h * b);
    }
    // Schwarzschild (both Cartesian forms): f = 1 - r_s / r
    const double rc = sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2]);
    const double fc = 1.0 - P.r_s / rc;
    if (cls == RS_SKY) return 1.0 / sqrt(fc);
    if (cls == RS_OBJECT) {
        const double rh = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        return sqrt((1.0 - P.r_s / rh) / fc);
    }
    // disk: k^t at the camera from the null condition of the Christoffel form, b = L_z / E
    const double h = P.r_s / (rc - P.r_s);
    const double nk = (xc[0] * kc[0] + xc[1] * kc[1] + xc[2] * kc[2]) / rc;
    const double kk = kc[0] * kc[0] + kc[1] * kc[1] + kc[2] * kc[2];
    const double kt = sqrt((kk + h * nk * nk) / fc);
    const double b = (xc[0] * kc[1] - xc[1] * kc[0]) / (fc * kt);
    const double R = sqrt(e[0] * e[0] + e[1] * e[1]);
    const double Om = s * sqrt(M) / (R * sqrt(R));
    return sqrt(1.0 - 3.0 * M / R) / (sqrt(fc) * (1.0 - Om * b));
}

// The moving observer's factor on the ZAMO's g (point 4): gamma (1 + beta.n), n the ray's ZAMO-frame
// look direction, recovered from the camera state (x_c, k0) by the inverse of the camera tetrad.  Kerr: the BL velocity and
// E, L of kerr_cart_to_bl, the local energy E_loc = (E - omega L) / alpha, k^t = E_loc / alpha, and the tetrad components
//     n ~ (sqrt(Sigma / Delta) k^r,  sqrt(Sigma) k^th,  sqrt(A) sin th / sqrt(Sigma) (k^ph - omega k^t))
// on the Euclidean spherical basis; Schwarzschild: n ~ k + (1 / sqrt f - 1) (k.r^) r^.  n is normalised (the null condition
// makes it a unit vector up to rounding).
__device__ double observer_doppler(const RedshiftParams &P, const double b[3], const double xc[3], const double kc[3])
{
    double bn;
    if (P.rhs == BHG_RHS_KERR_BL_) {
        const double a = P.spin, M = 0.5 * P.r_s, a2 = a * a;
        double px[3] = {xc[0], xc[1], xc[2]}, pk[3] = {kc[0], kc[1], kc[2]}, E, L;
        kerr_cart_to_bl(a, M, 0.0, px, pk, E, L);
        const double r = px[0];
        double st, ct, alpha, omega;
        sincos_pi4(px[1], st, ct);
        kerr_zamo(M, a, r, ct * ct, alpha, omega);
        const double Sig = __builtin_fma(a2 * ct, ct, r * r), Del = __builtin_fma(-2.0 * M, r, r * r + a2);
        const double R2 = r * r + a2, Aq = R2 * R2 - a2 * Del * st * st;
        const double kt = (E - omega * L) / (alpha * alpha);
        const double nr = sqrt(Sig / Del) * pk[0], nt = sqrt(Sig) * pk[1];
        const double np = sqrt(Aq / Sig) * st * (pk[2] - omega * kt);
        const double iw = rsqrt_nr(__builtin_fma(xc[1], xc[1], xc[0] * xc[0])), cp = xc[0] * iw, sp = xc[1] * iw;
        const double br = (b[0] * cp + b[1] * sp) * st + b[2] * ct;
        const double bt = (b[0] * cp + b[1] * sp) * ct - b[2] * st;
        const double bp = b[1] * cp - b[0] * sp;
        bn = (br * nr + bt * nt + bp * np) / sqrt(nr * nr + nt * nt + np * np);
    } else {
        const double rc = sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2]), ir = 1.0 / rc;
        const double rh[3] = {xc[0] * ir, xc[1] * ir, xc[2] * ir};
        const double q = (1.0 / sqrt(1.0 - P.r_s * ir) - 1.0) * (kc[0] * rh[0] + kc[1] * rh[1] + kc[2] * rh[2]);
        const double n[3] = {kc[0] + q * rh[0], kc[1] + q * rh[1], kc[2] + q * rh[2]};
        bn = (b[0] * n[0] + b[1] * n[1] + b[2] * n[2]) / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    }
    const double gamma = 1.0 / sqrt(1.0 - (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
    return gamma * (1.0 + bn);
}

// g of the camera's ZAMO (OBS = false: redshift_g as it stands), or of the moving observer (OBS = true)
template <bool OBS>
__device__ __forceinline__ double observer_g(const RedshiftParams &P, const ObserverParams &O, const double xc[3], const double kc[3],
                                             int cls, const double *e)
{
    const double g = redshift_g(P, xc, kc, cls, e);
    if (!OBS || cls == RS_DARK || cls == RS_NAN) return g;
    return g * observer_doppler(P, O.beta, xc, kc);
}

template <bool OBS>
__global__ void __launch_bounds__(256) redshift_kernel(const RedshiftArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double *xc = A.x0 ? A.x0 + i * 3 : A.p.x0;
    A.g[i] = observer_g<OBS>(A.p, A.obs, xc, A.k0 + i * 3, ray_class(A.flags[i]), A.end ? A.end + i * 6 : nullptr);
}

// ---- moving and spinning object spheres -------------------------------------------------------
// g of an object ray that ends at e (its end record: position, direction) on a sphere of centre c whose surface moves with
// V = v + w x (e - c) (world axes, dx/dt), from the camera state (xc, kc).  The formulas are the traced picture's, as
// redshift_g's: there the emitter moves with -V (Kerr: relative to the traced ZAMO, whose flow it keeps), so with k_i V^i the
// traced ray's covariant momentum contracted with V,
//     Schwarzschild  g = 1 / (sqrt(f_c) u^t (1 + k_i V^i / E)),          u^t = 1 / sqrt(f - |V|^2 - h (n.V)^2)
//     Kerr           g = O / (u^t (1 - omega b + k_i V^i / E)),          u^t = 1 / (alpha sqrt(1 - beta^2))
// k at the hit is rebuilt from the camera's constants -- Schwarzschild E and the vector L = x_c x k0 (k_r = s_r sqrt(E^2 -
// f L^2 / r^2) / f, k_perp = L x x / r^2), Kerr E, L and Carter's Q (k_r = s_r sqrt(R) / Delta, k_th = s_th sqrt(Theta)) --
// with only the signs s_r (Kerr: and s_th) from the end record's direction.  V = 0 gives redshift_g's static / ZAMO g up to
// rounding; the callers take redshift_g itself for a sphere at rest.
__device__ double object_g_moving(const RedshiftParams &P, const double v[3], const double w[3], const double c[3], const double xc[3],
                                  const double kc[3], const double *e)
{
    const double M = 0.5 * P.r_s;
    const double x = e[0], y = e[1], z = e[2];
    const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
    const double V[3] = {v[0] + (w[1] * dz - w[2] * dy), v[1] + (w[2] * dx - w[0] * dz), v[2] + (w[0] * dy - w[1] * dx)};
    if (P.rhs == BHG_RHS_KERR_BL_) {
        const double a = P.spin, a2 = a * a;
        double px[3] = {xc[0], xc[1], xc[2]}, pk[3] = {kc[0], kc[1], kc[2]}, E, L;
        kerr_cart_to_bl(a, M, 0.0, px, pk, E, L);     // the trace's own E and L, bit for bit
        const double b = L / E;
        double st_c, ct_c, alpha_c, omega_c;
        sincos_pi4(px[1], st_c, ct_c);
        kerr_zamo(M, a, px[0], ct_c * ct_c, alpha_c, omega_c);
        const double O = (1.0 - omega_c * b) / alpha_c;   // -k.u_obs / E
        const double kth_c = __builtin_fma(a2 * ct_c, ct_c, px[0] * px[0]) * pk[1];
        const double Q = kth_c * kth_c + ct_c * ct_c * (L * L / (st_c * st_c) - a2 * E * E);
        // the hit: BL r, cos / sin theta (x = sqrt(r^2 + a^2) sin th cos ph, z = r cos th)
        const double rho2 = x * x + y * y, bb = rho2 + z * z - a2;
        const double r = sqrt(0.5 * (bb + sqrt(bb * bb + 4.0 * a2 * z * z))), r2 = r * r, R2 = r2 + a2;
        const double ct = z / r, rho = sqrt(rho2), st = rho / sqrt(R2);
        double alpha, omega;
        kerr_zamo(M, a, r, ct * ct, alpha, omega);
        const double Sig = r2 + a2 * ct * ct, Del = r2 - 2.0 * M * r + a2, Aq = R2 * R2 - a2 * Del * st * st;
        // V on the BL coordinate basis (the inverse Jacobian of the embedding)
        const double vr_xy = x * V[0] + y * V[1];
        const double Vr = (r * vr_xy + R2 * ct * V[2]) / Sig;
        const double Vth = (sqrt(R2) * ct * vr_xy / rho - r * rho * V[2] / sqrt(R2)) / Sig;
        const double Vph = (x * V[1] - y * V[0]) / rho2;
        const double b2 = ((Sig / Del) * Vr * Vr + Sig * Vth * Vth + (Aq * st * st / Sig) * Vph * Vph) / (alpha * alpha);
        const double ut = 1.0 / (alpha * sqrt(1.0 - b2));
        // the photon at the hit from (E, L, Q); signs of k^r, k^th from the end direction
        const double d0 = e[3], d1 = e[4], d2 = e[5], dxy = x * d0 + y * d1;
        const double sr = (r2 * dxy + R2 * z * d2) < 0.0 ? -1.0 : 1.0;
        const double sth = (R2 * z * dxy - r2 * rho2 * d2) < 0.0 ? -1.0 : 1.0;
        const double Pp = R2 * E - a * L, aEL = a * E - L;
        const double k_r = sr * sqrt(fmax(Pp * Pp - Del * (Q + aEL * aEL), 0.0)) / Del;
        const double k_th = sth * sqrt(fmax(Q + ct * ct * (a2 * E * E - L * L / (st * st)), 0.0));
        const double kV = k_r * Vr + k_th * Vth + L * Vph;
        return O / (ut * ((1.0 - omega * b) + kV / E));
    }
    // Schwarzschild (both Cartesian forms): f = 1 - r_s / r, h = r_s / (r - r_s)
    const double rc = sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2]);
    const double fc = 1.0 - P.r_s / rc, hc = P.r_s / (rc - P.r_s);
    const double nkc = (xc[0] * kc[0] + xc[1] * kc[1] + xc[2] * kc[2]) / rc;
    const double kkc = kc[0] * kc[0] + kc[1] * kc[1] + kc[2] * kc[2];
    const double E = fc * sqrt((kkc + hc * nkc * nkc) / fc);
    const double Lv[3] = {xc[1] * kc[2] - xc[2] * kc[1], xc[2] * kc[0] - xc[0] * kc[2], xc[0] * kc[1] - xc[1] * kc[0]};
    const double r2 = x * x + y * y + z * z, r = sqrt(r2), f = 1.0 - P.r_s / r, h = P.r_s / (r - P.r_s);
    const double nV = (x * V[0] + y * V[1] + z * V[2]) / r, VV = V[0] * V[0] + V[1] * V[1] + V[2] * V[2];
    const double ut = 1.0 / sqrt(f - VV - h * nV * nV);
    const double LL = Lv[0] * Lv[0] + Lv[1] * Lv[1] + Lv[2] * Lv[2];
    const double sr = (x * e[3] + y * e[4] + z * e[5]) < 0.0 ? -1.0 : 1.0;
    const double k_r = sr * sqrt(fmax(E * E - f * LL / r2, 0.0)) / f;     // k_i n^i
    const double xV[3] = {y * V[2] - z * V[1], z * V[0] - x * V[2], x * V[1] - y * V[0]};
    const double kV = k_r * nV + (Lv[0] * xV[0] + Lv[1] * xV[1] + Lv[2] * xV[2]) / r2;
    return 1.0 / (sqrt(fc) * ut * (1.0 + kV / E));
}

// observer_g with moving object spheres: an object ray whose sphere j moves takes object_g_moving (times the observer's
// factor with OBS), every other ray observer_g<OBS> as it stands
template <bool OBS>
__device__ __forceinline__ double moving_g(const RedshiftParams &P, const ObserverParams &O, const MotionParams &mo,
                                           const double (*spheres)[4], const double xc[3], const double kc[3], int cls,
                                           const double *e, int j)
{
    if (cls != RS_OBJECT || !e || j < 0 || j >= BHG_MAX_SPHERES_ || !((mo.moving >> j) & 1u))
        return observer_g<OBS>(P, O, xc, kc, cls, e);
    const double g = object_g_moving(P, mo.v[j], mo.w[j], spheres[j], xc, kc, e);
    return OBS ? g * observer_doppler(P, O.beta, xc, kc) : g;
}

template <bool OBS>
__global__ void __launch_bounds__(256) redshift_motion_kernel(const RedshiftArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double *xc = A.x0 ? A.x0 + i * 3 : A.p.x0;
    const int cls = ray_class(A.flags[i]);
    const int j = (cls == RS_OBJECT && A.object_id) ? (int)A.object_id[i] : -1;
    A.g[i] = moving_g<OBS>(A.p, A.obs, A.mo, A.spheres, xc, A.k0 + i * 3, cls, A.end ? A.end + i * 6 : nullptr, j);
}

// ---- disk polarisation -----------------------------------------------------------------------
// The Walker-Penrose constant kappa = (A - i B)(r - i a cos th) of the traced ray k and a vector f, BL components (t, r, th, ph):
//     A = (k^t f^r - k^r f^t) + a sin^2 th (k^r f^ph - k^ph f^r),  B = [(r^2 + a^2)(k^ph f^th - k^th f^ph) - a (k^t f^th - k^th f^t)] sin th
__device__ __forceinline__ void kappa_bl(double r, double st, double ct, double a, const double k[4], const double f[4], double &re,
                                         double &im)
{
    const double A = (k[0] * f[1] - k[1] * f[0]) + a * st * st * (k[1] * f[3] - k[3] * f[1]);
    const double B = ((r * r + a * a) * (k[3] * f[2] - k[2] * f[3]) - a * (k[0] * f[2] - k[2] * f[0])) * st;
    const double ac = a * ct;
    re = A * r - B * ac;
    im = -(A * ac + B * r);
}

// a = 0 in the Cartesian layout x = r n^ of Schwarzschild coordinates: kappa = r [(k^t f.n^ - k.n^ f^t) - i n^.(f x k)]
__device__ __forceinline__ void kappa_cart(double rc, const double n[3], double kt, const double k[3], const double f[4], double &re,
                                           double &im)
{
    const double A = kt * (n[0] * f[1] + n[1] * f[2] + n[2] * f[3]) - (n[0] * k[0] + n[1] * k[1] + n[2] * k[2]) * f[0];
    const double B = n[0] * (f[2] * k[2] - f[3] * k[1]) + n[1] * (f[3] * k[0] - f[1] * k[2]) + n[2] * (f[1] * k[1] - f[2] * k[0]);
    re = A * rc;
    im = -B * rc;
}

// The screen legs of a ray whose look direction in the ZAMO frame is n (world axes): e_up = normalise(up - (up.n') n'),
// e_left = e_up x n', n' the observer's rest-frame direction (OBS: de-aberrated, aberrate with -beta).  In the traced picture
// the observer moves with -beta, so each leg X is lifted by that boost, X^0 = -gamma beta.X, X + gamma^2 / (gamma + 1) (beta.X)
// beta: both legs are then orthogonal to k.  X[0..3] = (X^0, world-axis X) of e_left, X[4..7] of e_up.  false: up is along n'.
template <bool OBS>
__device__ __forceinline__ bool screen_legs(const PolarisationParams &P, const double n_in[3], double X[8])
{
    double n[3] = {n_in[0], n_in[1], n_in[2]};
    const double *b = P.beta;
    double gamma = 1.0, c = 0.0;
    if (OBS) {
        gamma = 1.0 / sqrt(1.0 - (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
        c = gamma * gamma / (gamma + 1.0);
        const double nb[3] = {-b[0], -b[1], -b[2]};
        aberrate(nb, gamma, c, n_in, n);
        const double in = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        n[0] *= in;
        n[1] *= in;
        n[2] *= in;
    }
    const double *up = P.up;
    const double un = up[0] * n[0] + up[1] * n[1] + up[2] * n[2];
    const double w[3] = {up[0] - un * n[0], up[1] - un * n[1], up[2] - un * n[2]};
    const double wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(wn > 1e-12 * sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]))) return false;
    const double eu[3] = {w[0] / wn, w[1] / wn, w[2] / wn};
    const double el[3] = {eu[1] * n[2] - eu[2] * n[1], eu[2] * n[0] - eu[0] * n[2], eu[0] * n[1] - eu[1] * n[0]};
    for (int l = 0; l < 2; l++) {
        const double *e = l ? eu : el;
        double *x = X + 4 * l;
        if (OBS) {
            const double be = b[0] * e[0] + b[1] * e[1] + b[2] * e[2];
            x[0] = -gamma * be;
            x[1] = e[0] + c * be * b[0];
            x[2] = e[1] + c * be * b[1];
            x[3] = e[2] + c * be * b[2];
        } else {
            x[0] = 0.0;
            x[1] = e[0];
            x[2] = e[1];
            x[3] = e[2];
        }
    }
    return true;
}

// The degree table at mu (clamped to [0, 1]), linear between mu_j = j / (n - 1); one entry: a constant
__device__ __forceinline__ double pol_degree(const PolarisationParams &P, double mu)
{
    const int n = P.n_degree;
    if (n <= 1) return P.degree[0];
    const double x = fmin(fmax(mu, 0.0), 1.0) * (double)(n - 1);
    int j = (int)x;
    j = j > n - 2 ? n - 2 : j;
    const double t = x - (double)j;
    return P.degree[j] + t * (P.degree[j + 1] - P.degree[j]);
}

// One disk ray ending at e (its end record: position, direction) from the camera state (xc, kc): the emission cosine mu and
// the screen coefficients (c_L, c_U) of the emitted polarisation, both times the same nonzero factor (the 2x2 solve's
// determinant, so chi = atan2(c_L, c_U) mod pi needs no division).  false: the screen is degenerate (up along the ray); mu is
// set either way (it does not depend on the screen).  c_L = c_U = 0: f = 0, the photon leaves along the disk normal (mu = 1).
// The camera: Kerr E, L from kerr_cart_to_bl (the trace's own), Carter Q = k_th^2 + cos^2 th (L^2 / sin^2 th - a^2 E^2);
// Schwarzschild E = f k^t, the angular-momentum vector x x k.  The emitter: k rebuilt at the equator, BL r_h = sqrt(R^2 - a^2),
// from those constants with only the signs of k^r and k^th from the end record (the integrator's drift stays out);
// u Keplerian of sense s = -disk_sense (section 9); f = the vector orthogonal to u, e_th and k, which is the fluid frame's
// z^ x n_f: f^th = 0, f^t = u_ph g_rr k^r, f^r = E u_ph + L u_t, f^ph = -u_t g_rr k^r.
template <bool OBS>
__device__ bool polarisation_disk(const PolarisationParams &P, const double xc[3], const double kc[3], const double *e, double &cL,
                                  double &cU, double &mu)
{
    const double M = 0.5 * P.r_s, s = -P.sense;
    double a, E, L, Q, n[3], X[8], kl[2] = {0.0, 0.0}, ku[2] = {0.0, 0.0};
    bool legs;
    if (P.rhs == BHG_RHS_KERR_BL_) {
        a = P.spin;
        const double a2 = a * a;
        double px[3] = {xc[0], xc[1], xc[2]}, pk[3] = {kc[0], kc[1], kc[2]};
        kerr_cart_to_bl(a, M, 0.0, px, pk, E, L);
        const double r = px[0];
        double st, ct, alpha, omega;
        sincos_pi4(px[1], st, ct);
        kerr_zamo(M, a, r, ct * ct, alpha, omega);
        const double iw = rsqrt_nr(__builtin_fma(xc[1], xc[1], xc[0] * xc[0])), cp = xc[0] * iw, sp = xc[1] * iw;
        const double Sig = __builtin_fma(a2 * ct, ct, r * r), Del = __builtin_fma(-2.0 * M, r, r * r + a2);
        const double R2 = r * r + a2, Aq = R2 * R2 - a2 * Del * st * st;
        const double kt = (E - omega * L) / (alpha * alpha);
        const double kth = Sig * pk[1];
        Q = kth * kth + ct * ct * (L * L / (st * st) - a2 * E * E);
        const double sSD = sqrt(Sig / Del), sS = sqrt(Sig), sAS = sqrt(Aq / Sig);
        const double nr = sSD * pk[0], nt = sS * pk[1], np = sAS * st * (pk[2] - omega * kt);
        const double rh[3] = {st * cp, st * sp, ct}, th[3] = {ct * cp, ct * sp, -st}, ph[3] = {-sp, cp, 0.0};
        const double inn = 1.0 / sqrt(nr * nr + nt * nt + np * np);
        for (int j = 0; j < 3; j++) n[j] = (nr * rh[j] + nt * th[j] + np * ph[j]) * inn;
        legs = screen_legs<OBS>(P, n, X);
        const double k4[4] = {kt, pk[0], pk[1], pk[2]};
        for (int l = 0; legs && l < 2; l++) {
            const double *x = X + 4 * l;
            const double xr = x[1] * rh[0] + x[2] * rh[1] + x[3] * rh[2];
            const double xt = x[1] * th[0] + x[2] * th[1] + x[3] * th[2];
            const double xp = x[1] * ph[0] + x[2] * ph[1];
            const double f4[4] = {x[0] / alpha, xr / sSD, xt / sS, x[0] * omega / alpha + xp / (sAS * st)};
            kappa_bl(r, st, ct, a, k4, f4, l ? ku[0] : kl[0], l ? ku[1] : kl[1]);
        }
    } else {
        a = 0.0;
        const double rc = sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2]), ir = 1.0 / rc;
        const double rh[3] = {xc[0] * ir, xc[1] * ir, xc[2] * ir};
        const double f = 1.0 - P.r_s * ir, h = P.r_s / (rc - P.r_s), sf = sqrt(f);
        const double nk = rh[0] * kc[0] + rh[1] * kc[1] + rh[2] * kc[2];
        const double kk = kc[0] * kc[0] + kc[1] * kc[1] + kc[2] * kc[2];
        const double kt = sqrt((kk + h * nk * nk) / f);
        E = f * kt;
        const double Lx = xc[1] * kc[2] - xc[2] * kc[1], Ly = xc[2] * kc[0] - xc[0] * kc[2];
        L = xc[0] * kc[1] - xc[1] * kc[0];
        Q = Lx * Lx + Ly * Ly;
        const double q = (1.0 / sf - 1.0) * nk;
        const double m[3] = {kc[0] + q * rh[0], kc[1] + q * rh[1], kc[2] + q * rh[2]};
        const double inn = 1.0 / sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        for (int j = 0; j < 3; j++) n[j] = m[j] * inn;
        legs = screen_legs<OBS>(P, n, X);
        for (int l = 0; legs && l < 2; l++) {
            const double *x = X + 4 * l;
            const double xr = (1.0 - sf) * (x[1] * rh[0] + x[2] * rh[1] + x[3] * rh[2]);
            const double f4[4] = {x[0] / sf, x[1] - xr * rh[0], x[2] - xr * rh[1], x[3] - xr * rh[2]};
            kappa_cart(rc, rh, kt, kc, f4, l ? ku[0] : kl[0], l ? ku[1] : kl[1]);
        }
    }
    // the emitter, at the equator
    const double a2 = a * a;
    const double r = sqrt(e[0] * e[0] + e[1] * e[1] - a2), r2 = r * r, ir2 = 1.0 / r2;
    const double sr = (e[0] * e[3] + e[1] * e[4]) < 0.0 ? -1.0 : 1.0, sth = e[5] > 0.0 ? -1.0 : 1.0;
    const double Del = r2 - 2.0 * M * r + a2, Pp = (r2 + a2) * E - a * L, aEL = a * E - L;
    const double kt = (-a * aEL + (r2 + a2) * Pp / Del) * ir2;
    const double kp = (-aEL + a * Pp / Del) * ir2;
    const double kr = sr * sqrt(fmax(Pp * Pp - Del * (Q + aEL * aEL), 0.0)) * ir2;
    const double kth = sth * sqrt(fmax(Q, 0.0)) * ir2;
    const double sq = sqrt(r), r32 = r * sq, saM = s * a * sqrt(M);
    const double Om = s * sqrt(M) / (r32 + saM);
    const double ut = (r32 + saM) / (sqrt(r32) * sqrt(r32 - 3.0 * M * sq + 2.0 * saM)), up = Om * ut;
    const double gtt = -(1.0 - 2.0 * M / r), gtp = -2.0 * M * a / r, gpp = r2 + a2 + 2.0 * M * a2 / r, grr = r2 / Del;
    const double u_t = gtt * ut + gtp * up, u_p = gtp * ut + gpp * up;
    mu = fabs(r * kth) / (E * ut - L * up);
    const double ft = u_p * grr * kr, fr = E * u_p + L * u_t, fp = -u_t * grr * kr;
    const double A = (kt * fr - kr * ft) + a * (kr * fp - kp * fr);
    const double B = kth * (a * ft - (r2 + a2) * fp);
    const double re = A * r, im = -B * r;
    // re + i im = c_L kappa_L + c_U kappa_U, Cramer's rule without the division by the determinant
    cL = re * ku[1] - ku[0] * im;
    cU = kl[0] * im - re * kl[1];
    return legs;
}

// (chi, delta, mu) of one ray: disk rays their own, NaN rays (and disk rays without an end record) NaN, every other ray 0
template <bool OBS>
__device__ void polarisation_ray(const PolarisationParams &P, const double xc[3], const double kc[3], int cls, const double *e,
                                 double out[3])
{
    if (cls != RS_DISK || !e) {
        const double v = (cls == RS_NAN || cls == RS_DISK) ? __builtin_nan("") : 0.0;
        out[0] = out[1] = out[2] = v;
        return;
    }
    double cL, cU, mu;
    const bool ok = polarisation_disk<OBS>(P, xc, kc, e, cL, cU, mu);
    double chi = __builtin_nan("");      // no screen, or f = 0: no direction
    if (ok && (cL != 0.0 || cU != 0.0)) {
        chi = atan2(cL, cU);
        chi = chi > 0.5 * M_PI ? chi - M_PI : (chi <= -0.5 * M_PI ? chi + M_PI : chi);
    }
    out[0] = chi;
    out[1] = pol_degree(P, mu);
    out[2] = mu;
}

template <bool OBS>
__global__ void __launch_bounds__(256) polarisation_kernel(const PolarisationArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double *xc = A.x0 ? A.x0 + i * 3 : A.p.x0;
    double o[3];
    polarisation_ray<OBS>(A.p, xc, A.k0 + i * 3, ray_class(A.flags[i]), A.end ? A.end + i * 6 : nullptr, o);
    A.evpa[i] = o[0];
    A.degree[i] = o[1];
    if (A.mu) A.mu[i] = o[2];
}

// the shade kernels' polarised instances: (delta cos 2chi, delta sin 2chi) of a disk ray, (0, 0) where the per-ray chi is NaN
// (a degenerate screen, or f = 0)
// (cos 2chi = (c_U^2 - c_L^2) / (c_U^2 + c_L^2), sin 2chi = 2 c_L c_U / (c_U^2 + c_L^2): no trigonometry).  The observer's beta
// is zero without one, where the boost and the lift are exact identities.
__device__ __forceinline__ void polarisation_weigh(const ShadeArgs &A, uint64_t i, const double *e, double qu[2])
{
    double cL, cU, mu;
    if (!polarisation_disk<true>(A.pol, A.pol.x0, A.k0 + i * 3, e, cL, cU, mu)) return;
    const double den = cU * cU + cL * cL;
    if (!(den > 0.0)) return;     // f = 0: the photon leaves along the disk normal, mu = 1 (chi NaN per ray)
    const double d = pol_degree(A.pol, mu) / den;
    qu[0] = d * (cU * cU - cL * cL);
    qu[1] = d * (2.0 * cL * cU);
}

// ---- the thermal disk -------------------------------------------------------------------------
// One disk ray ending at e, seen from the camera state (xc, kc): its emitted temperature t_em = T_peak tau, tau^4 =
// F^(x) / max F^ (Page-Thorne, page_thorne), and what the camera sees of the colour-corrected blackbody f^-4 B_nu(f T) after
// the redshift g (observer_g<OBS>: bhg_redshift_device's g, bit for bit): a blackbody at g f T, in units of k_B T_peak / h,
//     I_c = scale sum_j w_cj nu_j^3 / (f^4 expm1(nu_j / (g f tau)))
// At or inside r_ms everything is an exact 0 (no emission from the plunging region).  The frequency loop's bound and index are
// wave-uniform: the table is read with scalar loads.
template <bool OBS>
__device__ __forceinline__ void disk_thermal(const ThermalParams &T, const RedshiftParams &P, const ObserverParams &O,
                                             const double xc[3], const double kc[3], const double *e, double &t_em, double rgb[3])
{
    rgb[0] = rgb[1] = rgb[2] = 0.0;
    t_em = 0.0;
    const double a = P.spin;    // (0 but for Kerr): BL r of the hit, as redshift_g takes it
    const double r = sqrt(e[0] * e[0] + e[1] * e[1] - a * a);
    if (!(r > T.r_ms)) return;
    const double x = sqrt(r / (0.5 * P.r_s));
    const double tau = sqrt(sqrt(fmax(page_thorne(T, x), 0.0) * T.inv_fmax));
    t_em = T.t_peak * tau;
    const double g = observer_g<OBS>(P, O, xc, kc, RS_DISK, e);
    const double y = (g * T.f_col) * tau, f2 = T.f_col * T.f_col, f4 = f2 * f2;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < T.n_nu; j++) {
        const double nu = T.nu[j];
        const double b = ((nu * nu) * nu) / (f4 * expm1(nu / y));
        acc[0] = acc[0] + T.w[0][j] * b;
        acc[1] = acc[1] + T.w[1][j] * b;
        acc[2] = acc[2] + T.w[2][j] * b;
    }
    rgb[0] = T.scale * acc[0];
    rgb[1] = T.scale * acc[1];
    rgb[2] = T.scale * acc[2];
}

// (T_em, I_R, I_G, I_B) of one ray per thread: disk rays their own, NaN rays (and disk rays without an end record) NaN, every
// other ray 0
template <bool OBS>
__global__ void __launch_bounds__(256) disk_thermal_kernel(const ThermalArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int cls = ray_class(A.flags[i]);
    const double *e = A.end ? A.end + i * 6 : nullptr;
    double t, rgb[3];
    if (cls != RS_DISK || !e) {
        t = (cls == RS_NAN || cls == RS_DISK) ? __builtin_nan("") : 0.0;
        rgb[0] = rgb[1] = rgb[2] = t;
    } else {
        const double *xc = A.x0 ? A.x0 + i * 3 : A.p.x0;
        disk_thermal<OBS>(A.t, A.p, A.obs, xc, A.k0 + i * 3, e, t, rgb);
    }
    A.t_em[i] = t;
    A.rgb[i * 3 + 0] = rgb[0];
    A.rgb[i * 3 + 1] = rgb[1];
    A.rgb[i * 3 + 2] = rgb[2];
}

// the shade kernels' redshift instances: rgb *= g^n for a ray of a class the caller selected (OBS: the moving observer's g)
template <bool OBS>
__device__ __forceinline__ void redshift_weigh(const ShadeArgs &A, uint64_t i, int cls, uint32_t bit, const double *e, double rgb[3])
{
    if (!(A.rs.apply & bit)) return;
    const double g = observer_g<OBS>(A.rs, A.obs, A.rs.x0, A.k0 + i * 3, cls, e), n = A.rs.exponent;
    // the exponents of the model, 4 (bolometric) and 3 (specific intensity), as products (libm's pow was a third of the kernel)
    const double g2 = g * g;
    const double w = n == 4.0 ? g2 * g2 : (n == 3.0 ? g2 * g : pow(g, n));
    rgb[0] *= w;
    rgb[1] *= w;
    rgb[2] *= w;
}

// redshift_weigh for an object ray of sphere j with moving spheres (moving_g)
template <bool OBS>
__device__ __forceinline__ void redshift_weigh_moving(const ShadeArgs &A, uint64_t i, int j, const double *e, double rgb[3])
{
    if (!(A.rs.apply & BHG_REDSHIFT_OBJECTS_)) return;
    const double g = moving_g<OBS>(A.rs, A.obs, A.mo, A.spheres, A.rs.x0, A.k0 + i * 3, RS_OBJECT, e, j), n = A.rs.exponent;
    const double g2 = g * g;
    const double w = n == 4.0 ? g2 * g2 : (n == 3.0 ? g2 * g : pow(g, n));
    rgb[0] *= w;
    rgb[1] *= w;
    rgb[2] *= w;
}

// The colour of ONE ray (sample s of pixel p): black for a horizon ray (:242-244), the disk's / an object's colour, or the
// sky in its exit direction.
// RS: the redshift instance (rgb *= g^n by class); without it the kernels are the frame path's as they were.  OBS (with RS
// only): g is the moving observer's.  TEX: object rays take the textured colour (object_colour_tex); nothing else differs.
// POL: a disk ray also gets its Stokes weights qu = (delta cos 2chi, delta sin 2chi), every other ray (0, 0); rgb is untouched.
// THERM (with RS only): a disk ray's colour is its thermal emission (disk_thermal, g already in it: the disk bit of rs.apply
// is not applied again); objects and sky as rs.apply says.
// MOV (with RS only): an object ray's g is that of its sphere's moving surface (moving_g); disk and sky rays as without it.
template <bool RS, bool OBS, bool TEX, bool POL, bool THERM, bool MOV>
__device__ __forceinline__ void ray_colour(const ShadeArgs &A, uint64_t i, uint8_t fl, double c0, double c1, double c2, double rgb[3],
                                           double qu[2])
{
    rgb[0] = rgb[1] = rgb[2] = 0.0;
    if (POL) qu[0] = qu[1] = 0.0;
    if (fl & BHG_FLAG_HIT_HORIZON_) return;
    const double *e = A.end + i * 6;
    if (fl == BHG_FLAG_HIT_DISK_ && A.disk_r_out > 0.0 && A.end) {
        if (THERM) {
            double t_em;
            disk_thermal<OBS>(A.th, A.rs, A.obs, A.rs.x0, A.k0 + i * 3, e, t_em, rgb);
        } else {
            disk_colour(A, e, rgb);
            if (RS) redshift_weigh<OBS>(A, i, RS_DISK, BHG_REDSHIFT_DISK_, e, rgb);
        }
        if (POL) polarisation_weigh(A, i, e, qu);
        return;
    }
    if (fl == BHG_FLAG_HIT_OBJECT_ && A.object_id && A.end) {
        if (TEX)
            object_colour_tex(A, e, (int)A.object_id[i], rgb);
        else
            object_colour(A, e, (int)A.object_id[i], rgb);
        if (MOV)
            redshift_weigh_moving<OBS>(A, i, (int)A.object_id[i], e, rgb);
        else if (RS)
            redshift_weigh<OBS>(A, i, RS_OBJECT, BHG_REDSHIFT_OBJECTS_, e, rgb);
        return;
    }
    // theta = 1 - acos(d_z / |d|) / pi (:373), phi = atan2(d_y, d_x) / pi (:374); exit directions are not unit
    // vectors (the Cam edition normalises, CamEdition.py:433-437) -- both angles as scale-free atan2's:
    // acos(d_z / |d|) = atan2(sqrt(d_x^2 + d_y^2), d_z)
    const double rho = sqrt(c0 * c0 + c1 * c1);
    const double theta = 1.0 - atan2_fast(rho, c2) * 0.3183098861837907;
    const double phi = atan2_fast(c1, c0) * 0.3183098861837907;
    sky_lookup(A.sky, A.sky_w, A.sky_h, -phi, 2.0 * theta - 1.0, rgb);  // :375
    // (start-inside rays carry the horizon flag: black above; a NaN ray is coloured as it always was, unweighted)
    if (RS && !(fl & BHG_FLAG_NAN_)) redshift_weigh<OBS>(A, i, RS_SKY, BHG_REDSHIFT_SKY_, nullptr, rgb);
}

__device__ __forceinline__ void write_pixel(const ShadeArgs &A, uint64_t p, const double acc[3])
{
    const double inv_s = 1.0 / (double)A.samples;  // buf = sbuf / (s+1) after the last sample (:250)
    if (A.rgba) {
        double *o = A.rgba + p * 4;
        reinterpret_cast<double2 *>(o)[0] = make_double2(acc[0] * inv_s, acc[1] * inv_s);
        reinterpret_cast<double2 *>(o)[1] = make_double2(acc[2] * inv_s, 1.0);
    }
    if (A.rgba_f32) {
        // what Blender's layer.rect holds (:163-164): float RGBA, alpha 1; optionally scattered straight to the
        // pixel's place in the frame (scatter[p] = y*W + x of this rank's p-th pixel)
        const uint64_t q = A.scatter ? (uint64_t)A.scatter[p] : p;
        reinterpret_cast<float4 *>(A.rgba_f32)[q] =
            make_float4((float)(acc[0] * inv_s), (float)(acc[1] * inv_s), (float)(acc[2] * inv_s), 1.0f);
    }
}

// the per-pixel means of (Q_r, Q_g, Q_b, U_r, U_g, U_b), at pixel p (never scattered)
__device__ __forceinline__ void write_stokes(const ShadeArgs &A, uint64_t p, const double acc[6])
{
    const double inv_s = 1.0 / (double)A.samples;
    double2 *o = reinterpret_cast<double2 *>(A.pol.qu + p * 6);
    o[0] = make_double2(acc[0] * inv_s, acc[1] * inv_s);
    o[1] = make_double2(acc[2] * inv_s, acc[3] * inv_s);
    o[2] = make_double2(acc[4] * inv_s, acc[5] * inv_s);
}

// One ray's colour, as the skeleton below calls it: a type per shade family, ray(A, i, rgb, qu, extra...) the colour of ray i
// (sample s of pixel p: i = s * n_pixels + p), qu its Stokes weights where STOKES says that the family has them.  The scene
// shade's is ray_colour in the ray's exit direction: the second half of the end records, or (direction-only traces of sky
// frames) an array of their own
template <bool RS, bool OBS, bool TEX, bool POL, bool THERM, bool MOV>
struct SceneColour {
    static constexpr bool STOKES = POL;
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double qu[2])
    {
        const double *d = A.dir ? A.dir + i * 3 : A.end + i * 6 + 3;
        ray_colour<RS, OBS, TEX, POL, THERM, MOV>(A, i, A.flags[i], d[0], d[1], d[2], rgb, qu);
    }
};

// The pixel reduction under every shade (COLOUR: SceneColour, LayersColour, MeshColour; EXTRA: the argument structs a family
// has beside ShadeArgs, handed on to COLOUR::ray).
// One thread per RAY, the S samples of a pixel staged in LDS and summed by one thread in sample order (:242-250: sbuf +=
// colour, sample after sample -- the order is part of the result).  A workgroup of 256 threads takes PPB = 256 / S
// pixels; thread t = s * PPB + q is sample s of the block's q-th pixel, so that for a fixed s the block reads PPB
// consecutive rays of the [S][P] layout (coalesced).  Against one thread per pixel walking its samples one after the
// other (round 3; kept below for S > 256) this puts S times as many independent atan2 / texel-gather chains in flight:
// the kernel is a latency chain per ray, not a bandwidth problem (131 MB in, 16 MB out per config-2 frame).
// POL (COLOUR::STOKES): each thread also stages the six Stokes products (Q, then U, of each channel; 9 doubles per thread in
// all, 18 KB per workgroup) and the pixel's Q / U means go to pol.qu[p].
template <class COLOUR, class... EXTRA>
__global__ void __launch_bounds__(256) shade_pixels_kernel(const ShadeArgs A, const uint32_t ppb, const EXTRA... x)
{
    constexpr bool POL = COLOUR::STOKES;
    __shared__ double col[256 * 3];
    __shared__ double pcol[POL ? 256 * 6 : 1];
    const uint32_t t = threadIdx.x, S = (uint32_t)A.samples;
    const uint32_t s = t / ppb, q = t - s * ppb;
    const uint64_t p = (uint64_t)blockIdx.x * ppb + q;
    const bool live = s < S && p < A.n_pixels;
    if (live) {
        double rgb[3], qu[2];
        COLOUR::ray(A, (uint64_t)s * A.n_pixels + p, rgb, POL ? qu : nullptr, x...);
        if (POL)
            for (int c = 0; c < 3; c++) {
                pcol[t * 6 + c] = qu[0] * rgb[c];
                pcol[t * 6 + 3 + c] = qu[1] * rgb[c];
            }
        col[t * 3 + 0] = rgb[0];
        col[t * 3 + 1] = rgb[1];
        col[t * 3 + 2] = rgb[2];
    }
    __syncthreads();
    if (s == 0 && live) {
        // (a horizon sample contributes an exact 0: acc + 0.0 is acc, the sum is bit for bit the skipping loop's)
        double acc[3] = {0.0, 0.0, 0.0};
        for (uint32_t k = 0; k < S; k++) {
            const double *c = col + (size_t)(k * ppb + q) * 3;
            acc[0] += c[0];
            acc[1] += c[1];
            acc[2] += c[2];
        }
        write_pixel(A, p, acc);
        if (POL) {
            double pacc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint32_t k = 0; k < S; k++) {
                const double *c = pcol + (size_t)(k * ppb + q) * 6;
                for (int m = 0; m < 6; m++) pacc[m] += c[m];
            }
            write_stokes(A, p, pacc);
        }
    }
}

// More samples than a workgroup has threads: one thread per pixel, samples accumulated in registers in sample order.
template <class COLOUR, class... EXTRA>
__global__ void __launch_bounds__(256) shade_pixels_serial_kernel(const ShadeArgs A, const EXTRA... x)
{
    constexpr bool POL = COLOUR::STOKES;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.n_pixels) return;
    double acc[3] = {0.0, 0.0, 0.0};
    double pacc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < A.samples; s++) {
        double rgb[3], qu[2];
        COLOUR::ray(A, (uint64_t)s * A.n_pixels + p, rgb, qu, x...);
        acc[0] += rgb[0];
        acc[1] += rgb[1];
        acc[2] += rgb[2];
        if (POL)
            for (int c = 0; c < 3; c++) {
                pacc[c] += qu[0] * rgb[c];
                pacc[3 + c] += qu[1] * rgb[c];
            }
    }
    write_pixel(A, p, acc);
    if (POL) write_stokes(A, p, pacc);
}

// Disk layers (bhg_shade_disk_layers_device): the optically thin disk.  The ray was carried through the
// disk by the crossings trace (disk_crossings_kernel: cross[m] the m-th crossing's record, n_cross the count, flags / end the
// disk-off trace's); each crossing passes the fraction T = 1 - opacity of what lies behind it:
//     w = 1;  for m < min(n_cross, max_cross) while w != 0:  rgb += w C(cross[m]);  w *= T
//     if w != 0:  rgb += w * (what ray_colour gives the disk-off ray: black for the horizon, else the sky, weighted as rs says)
// C is ray_colour's disk branch on the record: disk_colour and redshift_weigh, or (THERM) disk_thermal.  Sum and products in
// this order (no contraction): the order is part of the result.  opacity = 1 (T = 0): layer 0 alone, nothing behind a disk
// ray is looked at -- the opaque disk's image.
// RET (bhg_shade_disk_layers_retarded_device), a compile-time switch by presence: empty, or one Retarded --
// layer m of ray i is then coloured at the phase the disk had when the light left it, disk_phase - phase_rate * t_cross[m][i]; a
// layer whose time is not finite is black and still absorbs.  The retarded instances take it as a kernel argument of their own
// behind the others: ShadeArgs, and with it the argument block of every other shade kernel, is what it was.
struct Retarded {
    const double *t_cross;    // [max_cross][S*n_pixels]: the crossing times of the travel-time trace
    double phase_rate;        // d(disk_phase) / dt, radians per unit of coordinate time
};
__device__ __forceinline__ const Retarded &only(const Retarded &r) { return r; }

template <bool RS, bool OBS, bool THERM, class... RET>
__device__ __forceinline__ void layers_colour(const ShadeArgs &A, uint64_t i, uint64_t n_rays, uint8_t fl, double c0, double c1,
                                              double c2, double rgb[3], const RET &...ret)
{
    rgb[0] = rgb[1] = rgb[2] = 0.0;
    double w = 1.0;
    const uint32_t nc = A.n_cross[i], nl = nc < (uint32_t)A.max_cross ? nc : (uint32_t)A.max_cross;
    for (uint32_t m = 0; m < nl && w != 0.0; m++) {
        const double *e = A.cross + ((uint64_t)m * n_rays + i) * 6;
        double c[3];
        if (THERM) {
            double t_em;
            disk_thermal<OBS>(A.th, A.rs, A.obs, A.rs.x0, A.k0 + i * 3, e, t_em, c);
        } else {
            if constexpr (sizeof...(RET) != 0) {
                const Retarded &R = only(ret...);
                const double tm = R.t_cross[(uint64_t)m * n_rays + i];
                if (isfinite(tm))
                    disk_colour_at(A, e, A.disk_phase - R.phase_rate * tm, c);
                else
                    c[0] = c[1] = c[2] = 0.0;
            } else {
                disk_colour(A, e, c);
            }
            if (RS) redshift_weigh<OBS>(A, i, RS_DISK, BHG_REDSHIFT_DISK_, e, c);
        }
        rgb[0] = rgb[0] + w * c[0];
        rgb[1] = rgb[1] + w * c[1];
        rgb[2] = rgb[2] + w * c[2];
        w = w * A.transmit;
    }
    if (w != 0.0 && !(fl & (BHG_FLAG_HIT_HORIZON_ | BHG_FLAG_START_INSIDE_))) {
        // (the disk-off trace's flags never carry the disk / object bit; it is masked so that no flag value makes ray_colour
        // read the end record as a hit)
        double sky[3];
        ray_colour<RS, OBS, false, false, false, false>(A, i, (uint8_t)(fl & 0x7Fu), c0, c1, c2, sky, nullptr);
        rgb[0] = rgb[0] + w * sky[0];
        rgb[1] = rgb[1] + w * sky[1];
        rgb[2] = rgb[2] + w * sky[2];
    }
}

// the layered shade's colour type: the exit direction as SceneColour reads it, RET the skeleton's extra argument
template <bool RS, bool OBS, bool THERM>
struct LayersColour {
    static constexpr bool STOKES = false;
    template <class... RET>
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double *, const RET &...ret)
    {
        const double *d = A.dir ? A.dir + i * 3 : A.end + i * 6 + 3;
        layers_colour<RS, OBS, THERM>(A, i, (uint64_t)(uint32_t)A.samples * A.n_pixels, A.flags[i], d[0], d[1], d[2], rgb, ret...);
    }
};

// dst[i] = src[index[i]] for rows of four floats: puts the gathered per-rank slabs into frame order on the
// root GPU (index = the frame's permutation, computed once).  HBM-bound: 8 + 16 + 16 bytes per pixel.
__global__ void __launch_bounds__(256) gather_rows4_kernel(const float4 *src, const int64_t *index, uint64_t n, float4 *dst)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[index[i]];
}

// end[n][6] -> loc[n][3] and / or dir[n][3]: what spacetime_ray_cast hands back separately (end_loc, end_dir,
// RelativisticRenderEngine.py:307-308), so that only the arrays a caller reads cross PCIe
__global__ void __launch_bounds__(256) split_end_kernel(const double *end, uint64_t n, double *loc, double *dir)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 3) return;
    const uint64_t r = i / 3, c = i - r * 3;
    if (loc) loc[i] = end[r * 6 + c];
    if (dir) dir[i] = end[r * 6 + 3 + c];
}

hipError_t launch_split_end(const double *end, uint64_t n, double *loc, double *dir, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    BHG_LAUNCH(split_end_kernel, dim3((unsigned)((n * 3 + 255) / 256)), dim3(256), 0, s, end, n, loc, dir);
    return hipGetLastError();
}

hipError_t launch_gather_rows4(const float *src, const int64_t *index, uint64_t n, float *dst, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    BHG_LAUNCH(gather_rows4_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(src), index, n, reinterpret_cast<float4 *>(dst));
    return hipGetLastError();
}

hipError_t launch_raygen(const RaygenArgs &a, hipStream_t s)
{
    const uint64_t n = a.n_pixels * (uint64_t)a.samples;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (a.obs.on)   // grid-stride: at most 2048 workgroups (8 per CU), each thread forms the camera tetrad once
        BHG_LAUNCH(raygen_kernel<true>, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, a);
    else
        BHG_LAUNCH(raygen_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the launch of the per-ray kernels: one thread per ray, the observer's instance or the plain one
template <class ARGS>
hipError_t launch_per_ray(void (*with_obs)(ARGS), void (*plain)(ARGS), bool obs, const ARGS &a, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    BHG_LAUNCH(obs ? with_obs : plain, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_redshift(const RedshiftArgs &a, hipStream_t s)
{
    return launch_per_ray(redshift_kernel<true>, redshift_kernel<false>, a.obs.on != 0, a, a.n, s);
}

hipError_t launch_redshift_motion(const RedshiftArgs &a, hipStream_t s)
{
    return launch_per_ray(redshift_motion_kernel<true>, redshift_motion_kernel<false>, a.obs.on != 0, a, a.n, s);
}

hipError_t launch_polarisation(const PolarisationArgs &a, bool obs, hipStream_t s)
{
    return launch_per_ray(polarisation_kernel<true>, polarisation_kernel<false>, obs, a, a.n, s);
}

hipError_t launch_disk_thermal(const ThermalArgs &a, hipStream_t s)
{
    return launch_per_ray(disk_thermal_kernel<true>, disk_thermal_kernel<false>, a.obs.on != 0, a, a.n, s);
}

// the launch of the pixel reduction, for every shade family: the LDS kernel with PPB = 256 / S pixels per workgroup, or -- more
// samples than a workgroup has threads -- the serial one
template <class COLOUR, class... EXTRA>
void launch_shade_pixels(const ShadeArgs &a, hipStream_t s, const EXTRA &...x)
{
    if (a.samples > 256) {
        const dim3 grid((unsigned)((a.n_pixels + 255) / 256));
        BHG_LAUNCH((shade_pixels_serial_kernel<COLOUR, EXTRA...>), grid, dim3(256), 0, s, a, x...);
        return;
    }
    const uint32_t ppb = 256u / (uint32_t)a.samples;      // pixels per workgroup
    const dim3 grid((unsigned)((a.n_pixels + ppb - 1) / ppb));
    BHG_LAUNCH((shade_pixels_kernel<COLOUR, EXTRA...>), grid, dim3(256), 0, s, a, ppb, x...);
}

// the scene shade: one instance per (redshift, observer, textures, polarisation, thermal, motion), the template flags are the
// launch's run-time switches.
// the thermal instances are redshift instances (the disk's emission needs g); THERM = true is instantiated with RS = true only.
// So are the motion instances, taken only when objects are weighted (motion changes nothing else): MOV = true with RS = true only
template <bool TEX, bool POL, bool MOV>
void launch_shade_mov(const ShadeArgs &a, hipStream_t s)
{
    const bool therm = a.th.on != 0, rs = a.rs.apply != 0 || therm, obs = rs && a.obs.on;
    if (therm) {
        if (obs)
            launch_shade_pixels<SceneColour<true, true, TEX, POL, true, MOV>>(a, s);
        else
            launch_shade_pixels<SceneColour<true, false, TEX, POL, true, MOV>>(a, s);
    } else if (obs) {
        launch_shade_pixels<SceneColour<true, true, TEX, POL, false, MOV>>(a, s);
    } else if (rs) {
        launch_shade_pixels<SceneColour<true, false, TEX, POL, false, MOV>>(a, s);
    } else if (!MOV) {
        launch_shade_pixels<SceneColour<false, false, TEX, POL, false, false>>(a, s);
    }
}

template <bool TEX, bool POL>
void launch_shade_tex(const ShadeArgs &a, hipStream_t s)
{
    if (a.mo.on && (a.rs.apply & BHG_REDSHIFT_OBJECTS_))
        launch_shade_mov<TEX, POL, true>(a, s);
    else
        launch_shade_mov<TEX, POL, false>(a, s);
}

hipError_t launch_shade(const ShadeArgs &a, hipStream_t s)
{
    if (a.n_pixels == 0) return hipSuccess;
    if (a.pol.on) {
        if (a.ot.on)
            launch_shade_tex<true, true>(a, s);
        else
            launch_shade_tex<false, true>(a, s);
    } else if (a.ot.on) {
        launch_shade_tex<true, false>(a, s);
    } else {
        launch_shade_tex<false, false>(a, s);
    }
    return hipGetLastError();
}

// the layered shade's five instances, chosen as launch_shade_mov chooses: thermal instances are redshift instances.  With
// t_cross given (the C layer gives it only with a nonzero phase_rate) the three non-thermal ones have a retarded twin; the thermal
// disk has no texture to turn, and its instances are the same with or without
hipError_t launch_shade_layers(const ShadeArgs &a, hipStream_t s, const double *t_cross, double phase_rate)
{
    if (a.n_pixels == 0) return hipSuccess;
    const bool therm = a.th.on != 0, rs = a.rs.apply != 0 || therm, obs = rs && a.obs.on;
    if (t_cross && !therm) {
        const Retarded ret{t_cross, phase_rate};
        if (obs)
            launch_shade_pixels<LayersColour<true, true, false>>(a, s, ret);
        else if (rs)
            launch_shade_pixels<LayersColour<true, false, false>>(a, s, ret);
        else
            launch_shade_pixels<LayersColour<false, false, false>>(a, s, ret);
    } else if (therm) {
        if (obs)
            launch_shade_pixels<LayersColour<true, true, true>>(a, s);
        else
            launch_shade_pixels<LayersColour<true, false, true>>(a, s);
    } else if (obs) {
        launch_shade_pixels<LayersColour<true, true, false>>(a, s);
    } else if (rs) {
        launch_shade_pixels<LayersColour<true, false, false>>(a, s);
    } else {
        launch_shade_pixels<LayersColour<false, false, false>>(a, s);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// The mesh shade (bhg_shade_mesh_device).  A ray that the mesh trace ended on triangle T at x (end record,
// tri_id, bary) gets tri_rgb[T] times object_colour's Lambert lamp sum -- I^2 n.l / d^2, n.l clamped at 0 -- with
//   n   the triangle's unit normal e1 x e2 / |e1 x e2|, or -- vertex normals given -- the normalised (1 - u - v) N0 + u N1 + v N2,
//       turned to face the incoming ray (n . end_dir < 0);
//   a lamp shadowed when the straight segment from x + 1e-5 l^ to the lamp meets any triangle (segment_first_hit in its any-hit
//   form; 1e-5 is object_colour's epsilon).
// Every other ray is the plain shade's ray_colour, bit for bit.
// ------------------------------------------------------------------------------------------
struct MeshShade {
    MeshView mesh;
    const int32_t *tri_id;   // [S*n_pixels]
    const double *bary;      // [S*n_pixels][2]
    const float *tri_rgb;    // [nt][3] in the caller's numbering, or nullptr (white)
};

__device__ __forceinline__ void mesh_colour(const ShadeArgs &A, const MeshShade &G, uint64_t i, int32_t tri, double rgb[3])
{
    const double *e = A.end + i * 6;
    const int32_t slot = G.mesh.tri_slot[tri];
    const double *T = G.mesh.tri + (size_t)slot * 9;
    double n[3];
    if (G.mesh.tri_normals) {
        const double *N = G.mesh.tri_normals + (size_t)slot * 9;
        const double u = G.bary[i * 2], v = G.bary[i * 2 + 1], w = 1.0 - u - v;
        for (int c = 0; c < 3; c++) n[c] = w * N[c] + u * N[3 + c] + v * N[6 + c];
    } else {
        n[0] = T[4] * T[8] - T[5] * T[7];
        n[1] = T[5] * T[6] - T[3] * T[8];
        n[2] = T[3] * T[7] - T[4] * T[6];
    }
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double sgn = (n[0] * e[3] + n[1] * e[4] + n[2] * e[5]) > 0.0 ? -1.0 : 1.0;
    for (int c = 0; c < 3; c++) n[c] = sgn * (n[c] / len);
    double sum = 0.0;
    for (int l = 0; l < A.n_lamps; l++) {
        const double lv[3] = {A.lamps[l][0] - e[0], A.lamps[l][1] - e[1], A.lamps[l][2] - e[2]};
        const double d2 = lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2];
        const double dist = sqrt(d2);
        const double ld[3] = {lv[0] / dist, lv[1] / dist, lv[2] / dist};
        const double ndl = n[0] * ld[0] + n[1] * ld[1] + n[2] * ld[2];
        if (!(ndl > 0.0)) continue;
        const double from[3] = {e[0] + 1e-5 * ld[0], e[1] + 1e-5 * ld[1], e[2] + 1e-5 * ld[2]};
        const double to[3] = {A.lamps[l][0], A.lamps[l][1], A.lamps[l][2]};
        double s_hit;
        if (segment_first_hit<true>(G.mesh, from, to, s_hit) >= 0) continue;
        sum += A.lamps[l][3] * A.lamps[l][3] * ndl / d2;
    }
    for (int c = 0; c < 3; c++) rgb[c] = (G.tri_rgb ? (double)G.tri_rgb[(size_t)tri * 3 + c] : 1.0) * sum;
}

__device__ __forceinline__ void mesh_ray_colour(const ShadeArgs &A, const MeshShade &G, uint64_t i, double rgb[3])
{
    const uint8_t fl = A.flags[i];
    const int32_t tri = G.tri_id[i];
    if (fl == BHG_FLAG_HIT_OBJECT_ && tri >= 0 && tri < G.mesh.n_tris) {
        mesh_colour(A, G, i, tri, rgb);
        return;
    }
    const double *d = A.end + i * 6 + 3;
    ray_colour<false, false, false, false, false, false>(A, i, fl, d[0], d[1], d[2], rgb, nullptr);
}

// ------------------------------------------------------------------------------------------
// The mesh material shade (bhg_shade_mesh_material_device): a mesh ray gets albedo * (lamp_sum + emission),
// albedo = tri_rgb[T] * texel.  lamp_sum is mesh_colour's sum itself -- called with a white MeshShade, its three channels are
// 1.0 * sum -- so the normal, the facing rule, the shadow segment and the traversal are the one definition.  x * 1.0 and
// sum + 0.0 are exact: without UVs and with emission = 0 the colour is mesh_colour's tri_rgb[T] * sum, bit for bit.
// The material is one more argument struct behind MeshShade (MeshColour, below the colour functions).
// ------------------------------------------------------------------------------------------
// x mod n for an integer-valued x and a small positive integer n, in floating point as sky_lookup wraps its column: the
// quotient's rounding can only be off by one period, which the two selects put right.  (The device form of the material is
// not scanned: the last select keeps a non-finite coordinate inside the image.)
__device__ __forceinline__ int wrap_index(double x, double n)
{
    double w = __builtin_fma(-n, floor(x * (1.0 / n)), x);
    w = w < 0.0 ? w + n : (w >= n ? w - n : w);
    return (w >= 0.0 && w < n) ? (int)w : 0;
}

// bilinear, repeating in both directions; row 0 is V = 0 (include/bhgeo.h has the definition)
__device__ __forceinline__ void mesh_texel(const float *tex, int W, int H, double U, double V, double rgb[3])
{
    const double Wd = (double)W, Hd = (double)H;
    const double fx = U * Wd - 0.5, fy = V * Hd - 0.5;
    const double x0f = floor(fx), y0f = floor(fy);
    const double ax = fx - x0f, ay = fy - y0f;
    const int x0 = wrap_index(x0f, Wd), y0 = wrap_index(y0f, Hd);
    const int x1 = (x0 + 1 == W) ? 0 : x0 + 1, y1 = (y0 + 1 == H) ? 0 : y0 + 1;
    const float4 t00 = reinterpret_cast<const float4 *>(tex)[(long)y0 * W + x0];
    const float4 t01 = reinterpret_cast<const float4 *>(tex)[(long)y0 * W + x1];
    const float4 t10 = reinterpret_cast<const float4 *>(tex)[(long)y1 * W + x0];
    const float4 t11 = reinterpret_cast<const float4 *>(tex)[(long)y1 * W + x1];
    const double w00 = (1.0 - ax) * (1.0 - ay), w01 = ax * (1.0 - ay), w10 = (1.0 - ax) * ay, w11 = ax * ay;
    rgb[0] = __builtin_fma(w11, (double)t11.x, __builtin_fma(w10, (double)t10.x, __builtin_fma(w01, (double)t01.x, w00 * (double)t00.x)));
    rgb[1] = __builtin_fma(w11, (double)t11.y, __builtin_fma(w10, (double)t10.y, __builtin_fma(w01, (double)t01.y, w00 * (double)t00.y)));
    rgb[2] = __builtin_fma(w11, (double)t11.z, __builtin_fma(w10, (double)t10.z, __builtin_fma(w01, (double)t01.z, w00 * (double)t00.z)));
}

// tri_rgb[T] * texel at the hit's (u, v): the material's albedo, the mesh's own whichever instance was hit
__device__ __forceinline__ void mesh_material_albedo(const MeshShade &G, const MeshMaterialArgs &M, uint64_t i, int32_t tri, double albedo[3])
{
    albedo[0] = albedo[1] = albedo[2] = 1.0;
    if (M.tri_rgb)
        for (int c = 0; c < 3; c++) albedo[c] = (double)M.tri_rgb[(size_t)tri * 3 + c];
    const int32_t slot = !M.tri_uv ? -1 : (M.tri_tex ? M.tri_tex[tri] : 0);
    if (slot >= 0 && slot < M.n_tex) {
        // the triangle's six corner coordinates: one contiguous 24-byte read
        const float2 *uv = reinterpret_cast<const float2 *>(M.tri_uv) + (size_t)tri * 3;
        const float2 c0 = uv[0], c1 = uv[1], c2 = uv[2];
        const double u = G.bary[i * 2], v = G.bary[i * 2 + 1], w = 1.0 - u - v;
        const double U = w * (double)c0.x + u * (double)c1.x + v * (double)c2.x;
        const double V = w * (double)c0.y + u * (double)c1.y + v * (double)c2.y;
        double texel[3];
        mesh_texel(M.tex[slot], M.tex_w[slot], M.tex_h[slot], U, V, texel);
        for (int c = 0; c < 3; c++) albedo[c] *= texel[c];
    }
}

// G.tri_rgb == nullptr (launch_shade_mesh_material sees to it): mesh_colour leaves the lamp sum in every channel
__device__ __forceinline__ void mesh_material_ray_colour(const ShadeArgs &A, const MeshShade &G, const MeshMaterialArgs &M, uint64_t i,
                                                         double rgb[3])
{
    const uint8_t fl = A.flags[i];
    const int32_t tri = G.tri_id[i];
    if (fl == BHG_FLAG_HIT_OBJECT_ && tri >= 0 && tri < G.mesh.n_tris) {
        mesh_colour(A, G, i, tri, rgb);
        const double light = rgb[0] + M.emission;
        double albedo[3];
        mesh_material_albedo(G, M, i, tri, albedo);
        for (int c = 0; c < 3; c++) rgb[c] = albedo[c] * light;
        return;
    }
    const double *d = A.end + i * 6 + 3;
    ray_colour<false, false, false, false, false, false>(A, i, fl, d[0], d[1], d[2], rgb, nullptr);
}

// ------------------------------------------------------------------------------------------
// The instanced mesh shade (bhg_shade_mesh_instances_device).  A ray that the instanced trace ended on
// triangle T of instance j gets albedo * inst_rgb[j] * (lamp_sum + emission), the material's albedo and emission those of the
// mesh, shared by all instances.  lamp_sum is mesh_colour's with
//   n   formed in the instance's frame as mesh_colour forms it, flat or interpolated, rotated by R_j, and only then normalised
//       and turned to face the incoming ray;
//   a lamp shadowed when the segment from x + 1e-5 l^ to the lamp meets any triangle of any instance (segment_first_hit_instances
//       in its any-hit form: index order, the world box first).
// One instance under the identity: 1 x + 0 y + 0 z and x - 0 are exact, the colour is the material shade's, bit for bit.
// ------------------------------------------------------------------------------------------
struct MeshInstanceShade {
    const double *rec;         // [n][BHG_MESH_INSTANCE_DOUBLES_]
    int32_t n;
    int32_t boxes;             // 0: the shadow segments look at no world box (BHGEO_MESH_CULL=0)
    const int32_t *inst_id;    // [S*n_pixels]
    const float *inst_rgb;     // [n][3], or nullptr
};

// ... and the same over a set that lies under a tree: rec and n as above (the hit's own record is read by
// inst_id, the records stay in the caller's order), the shadow segments walk the tree
struct MeshInstanceTreeShade {
    const double *rec;
    int32_t n;
    int32_t boxes;             // 0: the shadow segments look at no box, of the tree's or of an instance
    const int32_t *inst_id;
    const float *inst_rgb;
    InstanceTreeView tree;
};

// does the segment meet any triangle of any instance?
__device__ __forceinline__ bool instances_shadow(const MeshView &mesh, const MeshInstanceShade &I, const double from[3], const double to[3])
{
    double s_hit;
    int32_t by;
    return segment_first_hit_instances<true>(mesh, I.rec, I.n, I.boxes != 0, from, to, s_hit, by) >= 0;
}

__device__ __forceinline__ bool instances_shadow(const MeshView &mesh, const MeshInstanceTreeShade &I, const double from[3], const double to[3])
{
    double s_hit;
    int32_t by;
    return segment_first_hit_instance_tree<true>(mesh, I.tree, I.boxes != 0, from, to, s_hit, by) >= 0;
}

template <class Inst>
__device__ __forceinline__ void mesh_instance_ray_colour(const ShadeArgs &A, const MeshShade &G, const MeshMaterialArgs &M,
                                                         const Inst &I, uint64_t i, double rgb[3])
{
    const uint8_t fl = A.flags[i];
    const int32_t tri = G.tri_id[i], inst = I.inst_id[i];
    if (!(fl == BHG_FLAG_HIT_OBJECT_ && tri >= 0 && tri < G.mesh.n_tris && inst >= 0 && inst < I.n)) {
        const double *d = A.end + i * 6 + 3;
        ray_colour<false, false, false, false, false, false>(A, i, fl, d[0], d[1], d[2], rgb, nullptr);
        return;
    }
    const double *e = A.end + i * 6;
    const int32_t slot = G.mesh.tri_slot[tri];
    const double *T = G.mesh.tri + (size_t)slot * 9;
    double m[3], n[3];
    if (G.mesh.tri_normals) {
        const double *N = G.mesh.tri_normals + (size_t)slot * 9;
        const double u = G.bary[i * 2], v = G.bary[i * 2 + 1], w = 1.0 - u - v;
        for (int c = 0; c < 3; c++) m[c] = w * N[c] + u * N[3 + c] + v * N[6 + c];
    } else {
        m[0] = T[4] * T[8] - T[5] * T[7];
        m[1] = T[5] * T[6] - T[3] * T[8];
        m[2] = T[3] * T[7] - T[4] * T[6];
    }
    instance_rotate_out(I.rec + (size_t)inst * BHG_MESH_INSTANCE_DOUBLES_, m, n);
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double sgn = (n[0] * e[3] + n[1] * e[4] + n[2] * e[5]) > 0.0 ? -1.0 : 1.0;
    for (int c = 0; c < 3; c++) n[c] = sgn * (n[c] / len);
    double sum = 0.0;
    for (int l = 0; l < A.n_lamps; l++) {
        const double lv[3] = {A.lamps[l][0] - e[0], A.lamps[l][1] - e[1], A.lamps[l][2] - e[2]};
        const double d2 = lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2];
        const double dist = sqrt(d2);
        const double ld[3] = {lv[0] / dist, lv[1] / dist, lv[2] / dist};
        const double ndl = n[0] * ld[0] + n[1] * ld[1] + n[2] * ld[2];
        if (!(ndl > 0.0)) continue;
        const double from[3] = {e[0] + 1e-5 * ld[0], e[1] + 1e-5 * ld[1], e[2] + 1e-5 * ld[2]};
        const double to[3] = {A.lamps[l][0], A.lamps[l][1], A.lamps[l][2]};
        if (instances_shadow(G.mesh, I, from, to)) continue;
        sum += A.lamps[l][3] * A.lamps[l][3] * ndl / d2;
    }
    // (1.0 * sum, as mesh_colour leaves it in a white mesh's channels)
    const double light = 1.0 * sum + M.emission;
    double albedo[3];
    mesh_material_albedo(G, M, i, tri, albedo);
    if (I.inst_rgb)
        for (int c = 0; c < 3; c++) albedo[c] *= (double)I.inst_rgb[(size_t)inst * 3 + c];
    for (int c = 0; c < 3; c++) rgb[c] = albedo[c] * light;
}

// the mesh shades' colour type: one overload per family, told apart by the argument structs that ride behind ShadeArgs
struct MeshColour {
    static constexpr bool STOKES = false;
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double *, const MeshShade &G)
    {
        mesh_ray_colour(A, G, i, rgb);
    }
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double *, const MeshShade &G,
                                               const MeshMaterialArgs &M)
    {
        mesh_material_ray_colour(A, G, M, i, rgb);
    }
};

// ... and the instanced one: a functor of its own under the same skeleton
struct MeshInstanceColour {
    static constexpr bool STOKES = false;
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double *, const MeshShade &G,
                                               const MeshMaterialArgs &M, const MeshInstanceShade &I)
    {
        mesh_instance_ray_colour(A, G, M, I, i, rgb);
    }
};

struct MeshInstanceTreeColour {
    static constexpr bool STOKES = false;
    static __device__ __forceinline__ void ray(const ShadeArgs &A, uint64_t i, double rgb[3], double *, const MeshShade &G,
                                               const MeshMaterialArgs &M, const MeshInstanceTreeShade &I)
    {
        mesh_instance_ray_colour(A, G, M, I, i, rgb);
    }
};

hipError_t launch_shade_mesh(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary, const float *tri_rgb,
                             hipStream_t s)
{
    if (a.n_pixels == 0) return hipSuccess;
    launch_shade_pixels<MeshColour>(a, s, MeshShade{m, tri_id, bary, tri_rgb});
    return hipGetLastError();
}

hipError_t launch_shade_mesh_material(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                      const MeshMaterialArgs &M, hipStream_t s)
{
    if (a.n_pixels == 0) return hipSuccess;
    launch_shade_pixels<MeshColour>(a, s, MeshShade{m, tri_id, bary, nullptr}, M);
    return hipGetLastError();
}

hipError_t launch_shade_mesh_instances(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                       const MeshMaterialArgs &M, const double *rec, int32_t n_inst, bool boxes,
                                       const int32_t *inst_id, const float *inst_rgb, hipStream_t s)
{
    if (a.n_pixels == 0) return hipSuccess;
    launch_shade_pixels<MeshInstanceColour>(a, s, MeshShade{m, tri_id, bary, nullptr}, M, MeshInstanceShade{rec, n_inst, boxes ? 1 : 0, inst_id, inst_rgb});
    return hipGetLastError();
}

hipError_t launch_shade_mesh_instance_tree(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                           const MeshMaterialArgs &M, const InstanceTreeView &tree, bool boxes,
                                           const int32_t *inst_id, const float *inst_rgb, hipStream_t s)
{
    if (a.n_pixels == 0) return hipSuccess;
    launch_shade_pixels<MeshInstanceTreeColour>(a, s, MeshShade{m, tri_id, bary, nullptr}, M,
                                                MeshInstanceTreeShade{tree.rec, tree.n, boxes ? 1 : 0, inst_id, inst_rgb, tree});
    return hipGetLastError();
}

}  // namespace bhg

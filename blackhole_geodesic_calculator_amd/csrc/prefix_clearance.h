// prefix_clearance.h -- the validity rule of the rays' start-up records (bhg_trace_prefix_device):
// plain C++, the host logic behind bhg_prefix_clearance and the C layer's decision to replay, kept apart so that the host
// tests compile it on its own (tests/prefix_clearance_driver.cpp).
//
// A record holds a ray's state after its leading accepted steps, every one of which ended inside the ball of radius rho
// about the start point.  The step loop's event tests look at step ends (the radius against the horizon and the exit sphere,
// the sign of z against the disk plane) and at the chord between them (object spheres), and a ball is convex: when no event
// surface reaches the ball, a full trace finds no event in those steps and arrives at the recorded state.  So:
//   clearance = distance from the start point to the nearest event surface of a call's scene,
//   rho       = PREFIX_RHO_FRACTION * min(clearance, |x0|), fixed when the records are written
//               (deep records, BHG_PREFIX_RECORD_DEEP: PREFIX_RHO_FRACTION_DEEP of it while the scene holds no object sphere),
//   a call replays only while its own clearance > rho (1 + PREFIX_MARGIN): the one validity test, whichever rule wrote them.
#pragma once
#include <cmath>

namespace bhg {

// A quarter: with K_MAX = 4 steps that each grow by at most the controller's factor 10, the steps kept are the climb from scipy's
// start guess (h0 ~ 0.01) to the settled step size (~ the distance to the hole), and a small ball survives more scene changes
// (an object sphere moving about).  It is NOT true that a larger ball holds no more steps, as this comment used to say: a
// headline ray (camera at r = 30, r_s = 2: clearance 29) takes three climbing steps that end 0.01, 0.08 and 0.8 from the camera,
// a fourth of 7 to 20, which leaves the quarter ball (7.25) for 90 % of the rays, and a fifth that takes 2 to 3 attempts.
// Attempts kept per ray, of 12.33, on 400 seeded headline rays (scipy RK45 at the bench's tolerances):
//   rho                 stop at the first rejection, <= 4 accepted    rejections kept, <= 6 accepted
//    7.25  (1/4)                     3.09                                      3.25
//   14.5   (1/2)                     3.78                                      5.24
//   21.75  (3/4)                     3.92                                      5.94
//   27.0   (0.93)                    3.93                                      7.71
constexpr double PREFIX_RHO_FRACTION = 0.25;
// Three quarters, the deep records' fraction in a scene WITHOUT object spheres: nothing moves there -- horizon, exit sphere and
// disk plane change only when the scene is edited, and prefix_replay_ok holds every call to the ball anyway.  (0.93 keeps more
// still, but that ball reaches r ~ 3 from a camera at 30 and gives up most of the tolerance to such edits.)
constexpr double PREFIX_RHO_FRACTION_DEEP = 0.75;
// The recorded step ends satisfy |x - x0|^2 <= rho^2 in rounded arithmetic, and the event tests compare rounded radii: a surface
// counts as clear of the ball only with this relative margin (many orders above the rounding, far below any scene's scale).
// A surface tangent to the ball is NOT clear.
constexpr double PREFIX_MARGIN = 1e-6;

// Distance from x0 to the nearest event surface: the horizon radius r_hor (0 when x0 is on or inside it: such rays never
// step), the exit sphere (r_exit > 0; from either side), the disk PLANE z = 0 when a disk is set (the plane, not the annulus:
// the sign test sees the plane), every object sphere {cx, cy, cz, radius} (from either side).  +inf is never returned: the
// horizon is always there.  Anything not finite gives 0, which no rho passes.
inline double prefix_clearance(double r_hor, double r_exit, bool disk, const double *spheres, int n_spheres, const double x0[3])
{
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    if (!std::isfinite(r0) || !(r_hor >= 0.0) || !(r0 > r_hor)) return 0.0;
    double c = r0 - r_hor;
    if (r_exit > 0.0) c = std::fmin(c, std::fabs(r_exit - r0));
    if (disk) c = std::fmin(c, std::fabs(x0[2]));
    for (int j = 0; j < n_spheres; j++) {
        const double *sp = spheres + 4 * j;
        const double dx = x0[0] - sp[0], dy = x0[1] - sp[1], dz = x0[2] - sp[2];
        const double d = std::fabs(std::sqrt(dx * dx + dy * dy + dz * dz) - sp[3]);
        if (!std::isfinite(d)) return 0.0;
        c = std::fmin(c, d);
    }
    return std::isfinite(c) && c > 0.0 ? c : 0.0;
}

// the radius a recording call fixes (0: nothing worth recording)
inline double prefix_rho(double clearance, const double x0[3])
{
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    if (!std::isfinite(clearance) || !std::isfinite(r0) || !(clearance > 0.0) || !(r0 > 0.0)) return 0.0;   // (fmin drops a NaN)
    return PREFIX_RHO_FRACTION * std::fmin(clearance, r0);
}

// the radius a DEEP recording call fixes: three quarters of min(clearance, |x0|) in an object-free scene, the quarter of always
// next to any object sphere (spheres move from frame to frame)
inline double prefix_rho_deep(double clearance, const double x0[3], int n_spheres)
{
    if (n_spheres > 0) return prefix_rho(clearance, x0);
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    if (!std::isfinite(clearance) || !std::isfinite(r0) || !(clearance > 0.0) || !(r0 > 0.0)) return 0.0;
    return PREFIX_RHO_FRACTION_DEEP * std::fmin(clearance, r0);
}

// ... of a deep recording CALL: the three quarters are for a ball that the HORIZON limits -- the one surface that cannot change
// without new records (r_s and the spin are on the list of bhg_start_steps_match).  Where the exit sphere or the disk plane
// is nearer than the horizon the call keeps the quarter: those may be edited from call to call like the object spheres, and
// the owners' records have always been held to a quarter of the way to them.
inline double prefix_rho_deep_call(double clearance, double r_hor, const double x0[3], int n_spheres)
{
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    const bool horizon_nearest = std::isfinite(r0) && r_hor >= 0.0 && clearance >= r0 - r_hor;
    return horizon_nearest ? prefix_rho_deep(clearance, x0, n_spheres) : prefix_rho(clearance, x0);
}

// may a call whose scene has this clearance replay records written with rho?
inline bool prefix_replay_ok(double clearance, double rho)
{
    return std::isfinite(rho) && rho > 0.0 && clearance > rho * (1.0 + PREFIX_MARGIN);
}

}  // namespace bhg

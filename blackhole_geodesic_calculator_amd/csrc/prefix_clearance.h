// prefix_clearance.h -- the validity rule of the rays' start-up records (bhg_trace_prefix_device):
// plain C++, the host logic behind bhg_prefix_clearance and the C layer's decision to replay, kept apart so that the host
// tests compile it on its own (tests/prefix_clearance_driver.cpp).
//
// A record holds a ray's state after its leading accepted steps, every one of which ended inside the ball of radius rho
// about the start point.  The step loop's event tests look at step ends (the radius against the horizon and the exit sphere,
// the sign of z against the disk plane) and at the chord between them (object spheres), and a ball is convex: when no event
// surface reaches the ball, a full trace finds no event in those steps and arrives at the recorded state.  So:
//   clearance = distance from the start point to the nearest event surface of a call's scene,
//   rho       = PREFIX_RHO_FRACTION * min(clearance, |x0|), fixed when the records are written,
//   a call replays only while its own clearance > rho (1 + PREFIX_MARGIN).
#pragma once
#include <cmath>

namespace bhg {

// A quarter: with K_MAX = 4 steps that each grow by at most the controller's factor 10, the steps kept are the climb from scipy's
// start guess (h0 ~ 0.01) to the settled step size (~ the distance to the hole); the first settled step is several units long,
// so a larger ball would hold no more steps, and a smaller one survives more scene changes (an object sphere moving about).
constexpr double PREFIX_RHO_FRACTION = 0.25;
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

// may a call whose scene has this clearance replay records written with rho?
inline bool prefix_replay_ok(double clearance, double rho)
{
    return std::isfinite(rho) && rho > 0.0 && clearance > rho * (1.0 + PREFIX_MARGIN);
}

}  // namespace bhg

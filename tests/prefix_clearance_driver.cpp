// prefix_clearance_driver.cpp -- the validity rule of the rays' start-up records (csrc/prefix_clearance.h: plain C++, the host
// logic behind bhg_prefix_clearance and the C layer's decision to replay) compiled with the HOST compiler under
// AddressSanitizer + UBSan by tests/test_start_prefix_host.py.  Checks each surface alone against its closed form, the
// nearest of several, both sides of the exit sphere and of an object sphere, tangent and near-tangent balls, the case with
// no disk and no objects, and degenerate input.  Prints "name clearance" per case (compared with the library's
// bhg_prefix_clearance by the test); exit code 0 = every check holds, otherwise the number of the first that fails.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../blackhole_geodesic_calculator_amd/csrc/prefix_clearance.h"

static int n_check = 0;
#define CHECK(cond)                  \
    do {                             \
        n_check++;                   \
        if (!(cond)) return n_check; \
    } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(1.0, std::fabs(b)); }

static double show(const char *name, double r_hor, double r_exit, bool disk, const double *sp, int ns, const double x0[3])
{
    const double c = bhg::prefix_clearance(r_hor, r_exit, disk, sp, ns, x0);
    std::printf("%s %.17g\n", name, c);
    return c;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double cam[3] = {0.0, 0.0, 30.0}, low[3] = {20.0, 0.0, 1.0}, far[3] = {0.0, 50.0, 0.5};
    // no disk, no objects, no exit sphere: the horizon alone
    double c = show("horizon", 1.0, 0.0, false, nullptr, 0, cam);
    CHECK(near(c, 29.0));
    CHECK(near(bhg::prefix_rho(c, cam), 7.25));                  // 1/4 min(29, 30)
    CHECK(bhg::prefix_replay_ok(c, 7.25));
    // a tiny hole: |x0| limits rho, not the clearance
    c = show("small_hole", 1e-3, 0.0, false, nullptr, 0, cam);
    CHECK(near(bhg::prefix_rho(c, cam), 0.25 * (30.0 - 1e-3)));
    // the exit sphere, from inside and from outside
    c = show("exit_inside", 1.0, 40.0, false, nullptr, 0, cam);
    CHECK(near(c, 10.0));
    c = show("exit_outside", 1.0, 40.0, false, nullptr, 0, far);
    CHECK(near(c, std::sqrt(2500.25) - 40.0));
    // the disk PLANE, whatever the annulus
    c = show("disk_plane", 1.0, 40.0, true, nullptr, 0, low);
    CHECK(near(c, 1.0));
    c = show("disk_off", 1.0, 40.0, false, nullptr, 0, low);
    CHECK(near(c, std::sqrt(401.0) - 1.0));                   // (the horizon is nearer than the exit sphere here)
    const double on_plane[3] = {20.0, 0.0, 0.0};
    c = show("on_plane", 1.0, 40.0, true, nullptr, 0, on_plane);
    CHECK(c == 0.0 && bhg::prefix_rho(c, on_plane) == 0.0);
    // object spheres: the nearest surface of several, from outside and from inside
    const double sp[3][4] = {{0.0, 0.0, 20.0, 2.0}, {3.0, 4.0, 30.0, 1.5}, {0.0, 0.0, 29.0, 5.0}};
    c = show("sphere_first", 1.0, 0.0, false, &sp[0][0], 1, cam);
    CHECK(near(c, 8.0));
    c = show("sphere_nearest", 1.0, 0.0, false, &sp[0][0], 2, cam);
    CHECK(near(c, 3.5));
    c = show("sphere_from_inside", 1.0, 0.0, false, &sp[2][0], 1, cam);
    CHECK(near(c, 4.0));
    c = show("all_surfaces", 1.0, 31.0, true, &sp[0][0], 3, cam);
    CHECK(near(c, 1.0));                                         // the exit sphere wins
    // tangent: a ball of radius rho touching the surface is NOT clear; a hair inside the margin is not either; beyond it is
    const double rho = 2.5;
    CHECK(!bhg::prefix_replay_ok(rho, rho));
    CHECK(!bhg::prefix_replay_ok(rho * (1.0 + 0.5 * bhg::PREFIX_MARGIN), rho));
    CHECK(bhg::prefix_replay_ok(rho * (1.0 + 2.0 * bhg::PREFIX_MARGIN), rho));
    CHECK(!bhg::prefix_replay_ok(0.99 * rho, rho));
    const double tangent[4] = {0.0, 0.0, 30.0 - (2.0 + rho), 2.0}, outside[4] = {0.0, 0.0, 30.0 - (2.0 + 1.001 * rho), 2.0};
    c = show("sphere_tangent", 1.0, 40.0, false, tangent, 1, cam);
    CHECK(near(c, rho) && !bhg::prefix_replay_ok(c, rho));
    c = show("sphere_outside", 1.0, 40.0, false, outside, 1, cam);
    CHECK(bhg::prefix_replay_ok(c, rho));
    // the rho of a recording call always passes its own call's test
    for (double r_exit : {0.0, 30.5, 40.0, 1e6})
        for (bool disk : {false, true}) {
            const double cc = bhg::prefix_clearance(1.0, r_exit, disk, &sp[0][0], 2, cam);
            const double rr = bhg::prefix_rho(cc, cam);
            CHECK(rr > 0.0 && rr <= 0.25 * cc && bhg::prefix_replay_ok(cc, rr));
        }
    // on or inside the horizon, and anything not finite: 0, which no rho passes; no rho <= 0 or non-finite passes either
    const double inside[3] = {0.1, 0.0, 0.2}, on_hor[3] = {0.0, 1.0, 0.0}, bad[3] = {nan, 0.0, 30.0}, huge[3] = {inf, 0.0, 0.0};
    CHECK(show("inside", 1.0, 40.0, false, nullptr, 0, inside) == 0.0);
    CHECK(show("on_horizon", 1.0, 40.0, false, nullptr, 0, on_hor) == 0.0);
    CHECK(show("nan_origin", 1.0, 40.0, false, nullptr, 0, bad) == 0.0);
    CHECK(show("inf_origin", 1.0, 40.0, false, nullptr, 0, huge) == 0.0);
    CHECK(bhg::prefix_clearance(nan, 40.0, false, nullptr, 0, cam) == 0.0);
    const double nan_sp[4] = {nan, 0.0, 0.0, 1.0};
    CHECK(bhg::prefix_clearance(1.0, 40.0, false, nan_sp, 1, cam) == 0.0);
    CHECK(bhg::prefix_rho(0.0, cam) == 0.0 && bhg::prefix_rho(nan, cam) == 0.0);
    CHECK(!bhg::prefix_replay_ok(10.0, 0.0) && !bhg::prefix_replay_ok(10.0, -1.0) && !bhg::prefix_replay_ok(10.0, nan) &&
          !bhg::prefix_replay_ok(inf, inf) && !bhg::prefix_replay_ok(0.0, 1e-300));
    return 0;
}

// prefix_deep_driver.cpp -- the radius rule of the DEEP start-up records (csrc/prefix_clearance.h: prefix_rho_deep, behind
// BHG_PREFIX_RECORD_DEEP) compiled with the HOST compiler under AddressSanitizer + UBSan by tests/test_deep_prefix_host.py:
// three quarters of min(clearance, |x0|) in a scene without object spheres, the quarter of always next to any, zero for every
// start that has no clear ball, and a rho that always passes prefix_replay_ok for the call that fixed it.
// Prints "name rho" per case; exit code 0 = every check holds, otherwise the number of the first that fails.
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

static double show(const char *name, double rho)
{
    std::printf("%s %.17g\n", name, rho);
    return rho;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double cam[3] = {0.0, 0.0, 30.0}, bad_early[3] = {nan, 0.0, 30.0};
    CHECK(bhg::PREFIX_RHO_FRACTION_DEEP == 0.75 && bhg::PREFIX_RHO_FRACTION == 0.25);
    // the bench camera, the horizon alone: (30 - 1) 3/4
    double c = bhg::prefix_clearance(1.0, 0.0, false, nullptr, 0, cam);
    double r = show("bench_camera", bhg::prefix_rho_deep(c, cam, 0));
    CHECK(near(c, 29.0) && near(r, 21.75) && bhg::prefix_replay_ok(c, r));
    CHECK(near(bhg::prefix_rho(c, cam), 7.25));                    // the rule of always is what it was
    // one object sphere, far away (it does not set the clearance): the quarter
    const double sp[2][4] = {{40.0, 40.0, 40.0, 1.0}, {0.0, 0.0, 20.0, 2.0}};
    c = bhg::prefix_clearance(1.0, 0.0, false, &sp[0][0], 1, cam);
    r = show("one_sphere_far", bhg::prefix_rho_deep(c, cam, 1));
    CHECK(near(c, 29.0) && near(r, 7.25) && r == bhg::prefix_rho(c, cam));
    // ... and one that does: 1/4 of 8
    c = bhg::prefix_clearance(1.0, 0.0, false, &sp[1][0], 1, cam);
    r = show("one_sphere_near", bhg::prefix_rho_deep(c, cam, 1));
    CHECK(near(c, 8.0) && near(r, 2.0));
    // the exit sphere of the orbit frames without their spheres: 3/4 of 10
    c = bhg::prefix_clearance(1.0, 40.0, false, nullptr, 0, cam);
    r = show("exit_sphere", bhg::prefix_rho_deep(c, cam, 0));
    CHECK(near(r, 7.5) && bhg::prefix_replay_ok(c, r));
    // ... which is what prefix_rho_deep says; a recording CALL keeps the three quarters for a ball that the horizon limits, and
    // the quarter where the exit sphere or the disk plane is the nearer surface (they may be edited between calls)
    CHECK(near(show("call_exit_nearer", bhg::prefix_rho_deep_call(c, 1.0, cam, 0)), 2.5));
    CHECK(near(show("call_bench_camera", bhg::prefix_rho_deep_call(29.0, 1.0, cam, 0)), 21.75));
    c = bhg::prefix_clearance(1.0, 60.0, true, nullptr, 0, cam);     // exit sphere and disk plane 30 away, the horizon 29
    CHECK(near(c, 29.0) && near(show("call_exit_farther", bhg::prefix_rho_deep_call(c, 1.0, cam, 0)), 21.75));
    const double low[3] = {20.0, 0.0, 1.0};
    c = bhg::prefix_clearance(1.0, 0.0, true, nullptr, 0, low);
    CHECK(near(c, 1.0) && near(show("call_disk_nearer", bhg::prefix_rho_deep_call(c, 1.0, low, 0)), 0.25));
    CHECK(near(bhg::prefix_rho_deep_call(8.0, 1.0, cam, 1), 2.0) && near(bhg::prefix_rho_deep_call(29.0, 1.0, cam, 1), 7.25));
    CHECK(bhg::prefix_rho_deep_call(0.0, 1.0, cam, 0) == 0.0 && bhg::prefix_rho_deep_call(nan, 1.0, cam, 0) == 0.0 &&
          bhg::prefix_rho_deep_call(10.0, 1.0, bad_early, 0) == 0.0 && bhg::prefix_rho_deep_call(10.0, nan, cam, 0) == 2.5);
    for (double r_exit : {0.0, 30.5, 40.0, 59.0, 61.0, 1e6})
        for (bool disk : {false, true})
            for (int ns : {0, 2}) {
                const double cc = bhg::prefix_clearance(1.0, r_exit, disk, ns ? &sp[0][0] : nullptr, ns, cam);
                const double rr = bhg::prefix_rho_deep_call(cc, 1.0, cam, ns);
                CHECK(rr > 0.0 && rr <= 0.75 * cc && bhg::prefix_replay_ok(cc, rr));
                CHECK(near(rr, (ns == 0 && cc >= 29.0 ? 0.75 : 0.25) * cc));
            }
    // a tiny hole: |x0| limits rho, not the clearance
    c = bhg::prefix_clearance(1e-3, 0.0, false, nullptr, 0, cam);
    r = show("small_hole", bhg::prefix_rho_deep(c, cam, 0));
    CHECK(near(c, 30.0 - 1e-3) && near(r, 0.75 * (30.0 - 1e-3)) && bhg::prefix_replay_ok(c, r));
    const double origin_clear = 1e9;                                // (a clearance beyond |x0|: a caller's own figure)
    CHECK(near(bhg::prefix_rho_deep(origin_clear, cam, 0), 22.5) && near(bhg::prefix_rho_deep(origin_clear, cam, 3), 7.5));
    // no clear ball: on the disk plane, on and inside the horizon, anything not finite
    const double on_plane[3] = {20.0, 0.0, 0.0}, on_hor[3] = {0.0, 1.0, 0.0}, inside[3] = {0.1, 0.0, 0.2};
    const double bad[3] = {nan, 0.0, 30.0}, huge[3] = {inf, 0.0, 0.0}, zero[3] = {0.0, 0.0, 0.0};
    c = bhg::prefix_clearance(1.0, 40.0, true, nullptr, 0, on_plane);
    CHECK(show("on_plane", bhg::prefix_rho_deep(c, on_plane, 0)) == 0.0 && c == 0.0);
    c = bhg::prefix_clearance(1.0, 40.0, false, nullptr, 0, on_hor);
    CHECK(show("on_horizon", bhg::prefix_rho_deep(c, on_hor, 0)) == 0.0 && c == 0.0);
    c = bhg::prefix_clearance(1.0, 40.0, false, nullptr, 0, inside);
    CHECK(show("inside", bhg::prefix_rho_deep(c, inside, 0)) == 0.0);
    c = bhg::prefix_clearance(1.0, 40.0, false, nullptr, 0, bad);
    CHECK(show("nan_origin", bhg::prefix_rho_deep(c, bad, 0)) == 0.0);
    CHECK(show("nan_origin_clear", bhg::prefix_rho_deep(10.0, bad, 0)) == 0.0 && bhg::prefix_rho_deep(10.0, bad, 1) == 0.0);
    CHECK(show("inf_origin", bhg::prefix_rho_deep(10.0, huge, 0)) == 0.0 && bhg::prefix_rho_deep(10.0, huge, 2) == 0.0);
    CHECK(bhg::prefix_rho_deep(10.0, zero, 0) == 0.0);
    for (int ns : {0, 1})
        CHECK(bhg::prefix_rho_deep(0.0, cam, ns) == 0.0 && bhg::prefix_rho_deep(-1.0, cam, ns) == 0.0 &&
              bhg::prefix_rho_deep(nan, cam, ns) == 0.0 && bhg::prefix_rho_deep(inf, cam, ns) == 0.0);
    // the rho of a recording call always passes that call's own test, whatever sets the clearance and however small it is
    for (double clear = 1e-9; clear < 1e9; clear *= 1.7)
        for (int ns : {0, 1, 8}) {
            const double rr = bhg::prefix_rho_deep(clear, cam, ns);
            const double frac = ns ? 0.25 : 0.75;
            CHECK(rr > 0.0 && near(rr, frac * std::fmin(clear, 30.0)));
            // (beyond |x0| the clearance is no longer what limits rho; up to there the call's own clearance must pass)
            CHECK(bhg::prefix_replay_ok(clear, rr));
        }
    for (double r_exit : {0.0, 30.5, 40.0, 1e6})
        for (bool disk : {false, true})
            for (int ns : {0, 2}) {
                const double cc = bhg::prefix_clearance(1.0, r_exit, disk, ns ? &sp[0][0] : nullptr, ns, cam);
                const double rr = bhg::prefix_rho_deep(cc, cam, ns);
                CHECK(rr > 0.0 && rr <= (ns ? 0.25 : 0.75) * cc && bhg::prefix_replay_ok(cc, rr));
            }
    // the margin of the replay test is far below a quarter of the ball: 3/4 (1 + margin) < 1
    CHECK(bhg::PREFIX_RHO_FRACTION_DEEP * (1.0 + bhg::PREFIX_MARGIN) < 1.0);
    return 0;
}

// prefix_wide_driver.cpp -- the radius rule of the WIDE start-up records (csrc/prefix_clearance.h: prefix_rho_wide_call, behind
// BHG_PREFIX_RECORD_WIDE) and the owners' rule for recording again (PrefixOwner), compiled with the HOST compiler under
// AddressSanitizer + UBSan by tests/test_wide_prefix_host.py: fifteen sixteenths of min(clearance, |x0|) exactly where the deep
// call takes its three quarters, what the deep call returns everywhere else; two refusals in a row or eight roomy calls ask for
// new records, one refusal or seven calls do not.
// Prints "name value" per case; exit code 0 = every check holds, otherwise the number of the first that fails.
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

static double show(const char *name, double v)
{
    std::printf("%s %.17g\n", name, v);
    return v;
}

constexpr int NONE = bhg::PREFIX_MODE_NONE, REPLAY = bhg::PREFIX_MODE_REPLAY, DEEP = bhg::PREFIX_MODE_RECORD_DEEP,
              WIDE = bhg::PREFIX_MODE_RECORD_WIDE;
static const double CAM[3] = {0.0, 0.0, 30.0};

// one call of an owner that records by the wide rule from the bench camera, r_s = 1: the scene is an exit sphere (0: none)
struct Owner {
    bhg::PrefixOwner o;
    int last_mode = NONE, last_used = NONE;
    double last_rho = 0.0;
    int records = 0, replays = 0, refusals = 0;

    // what the library would answer (bhgeo_capi.hip: the rule's rho for a recording call, prefix_replay_ok for a replaying one)
    int call(int ask, double r_exit)
    {
        const double c = bhg::prefix_clearance(1.0, r_exit, false, nullptr, 0, CAM);
        last_mode = ask;
        last_used = NONE;
        if (ask == WIDE) {
            last_rho = bhg::prefix_rho_wide_call(c, 1.0, CAM, 0);
            last_used = last_rho > 0.0 ? WIDE : NONE;
            records += last_used == WIDE;
        } else if (ask == REPLAY) {
            last_rho = o.rho;
            last_used = bhg::prefix_replay_ok(c, o.rho) ? REPLAY : NONE;
            (last_used == REPLAY ? replays : refusals)++;
        }
        return last_used;
    }
    int first(double r_exit)
    {
        o = bhg::PrefixOwner();
        return call(WIDE, r_exit);
    }
    int next(double r_exit)
    {
        const double c = bhg::prefix_clearance(1.0, r_exit, false, nullptr, 0, CAM);
        const int ask = o.next(WIDE, c, 1.0, CAM, 0, last_mode, last_used, last_rho);
        call(ask, r_exit);
        return ask;
    }
};

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(bhg::PREFIX_RHO_FRACTION_WIDE == 0.9375 && bhg::PREFIX_RHO_FRACTION_DEEP == 0.75 && bhg::PREFIX_RHO_FRACTION == 0.25);
    CHECK(bhg::PREFIX_MODE_RECORD_WIDE == 5 && bhg::PREFIX_OWNER_SHRINK_CALLS == 2 && bhg::PREFIX_OWNER_GROW_CALLS == 8);
    // ---- the radius ----------------------------------------------------------------------------------------------------------
    // the bench camera, the horizon alone: (30 - 1) 15/16, and that call's own clearance passes
    double c = bhg::prefix_clearance(1.0, 0.0, false, nullptr, 0, CAM);
    double r = show("bench_camera", bhg::prefix_rho_wide_call(c, 1.0, CAM, 0));
    CHECK(c == 29.0 && r == 27.1875 && bhg::prefix_replay_ok(29.0, 27.1875));
    CHECK(near(bhg::prefix_rho_deep_call(c, 1.0, CAM, 0), 21.75) && near(bhg::prefix_rho(c, CAM), 7.25));   // (the others are what they were)
    // one object sphere anywhere -- far, setting the clearance, behind the hole: the quarter, the deep call's to the bit
    const double sp[3][4] = {{40.0, 40.0, 40.0, 1.0}, {0.0, 0.0, 20.0, 2.0}, {0.0, 0.0, -20.0, 2.0}};
    const char *sp_name[3] = {"one_sphere_far", "one_sphere_near", "one_sphere_behind"};
    const double sp_rho[3] = {7.25, 2.0, 7.25};
    for (int j = 0; j < 3; j++) {
        c = bhg::prefix_clearance(1.0, 0.0, false, &sp[j][0], 1, CAM);
        r = show(sp_name[j], bhg::prefix_rho_wide_call(c, 1.0, CAM, 1));
        CHECK(near(r, sp_rho[j]) && r == bhg::prefix_rho_deep_call(c, 1.0, CAM, 1) && r == bhg::prefix_rho(c, CAM));
    }
    // an exit sphere nearer than the horizon (40: 10 away; 45: 15 away, the refusal test's scene): the quarter
    c = bhg::prefix_clearance(1.0, 40.0, false, nullptr, 0, CAM);
    r = show("exit_nearer", bhg::prefix_rho_wide_call(c, 1.0, CAM, 0));
    CHECK(near(r, 2.5) && r == bhg::prefix_rho_deep_call(c, 1.0, CAM, 0));
    c = bhg::prefix_clearance(1.0, 45.0, false, nullptr, 0, CAM);
    CHECK(near(show("exit_45", bhg::prefix_rho_wide_call(c, 1.0, CAM, 0)), 3.75));
    // ... and one farther (70: 40 away): the horizon is the nearest surface, the wide ball applies
    c = bhg::prefix_clearance(1.0, 70.0, false, nullptr, 0, CAM);
    CHECK(show("exit_farther", bhg::prefix_rho_wide_call(c, 1.0, CAM, 0)) == 27.1875);
    // a disk plane at |z0| = 30 (the horizon is 29 away): the wide ball, and the plane stays outside it
    c = bhg::prefix_clearance(1.0, 0.0, true, nullptr, 0, CAM);
    r = show("disk_plane_30", bhg::prefix_rho_wide_call(c, 1.0, CAM, 0));
    CHECK(c == 29.0 && r == 27.1875 && std::fabs(CAM[2]) > r * (1.0 + bhg::PREFIX_MARGIN) && bhg::prefix_replay_ok(c, r));
    // a disk plane nearer than the horizon: the quarter
    const double low[3] = {20.0, 0.0, 1.0};
    c = bhg::prefix_clearance(1.0, 0.0, true, nullptr, 0, low);
    CHECK(near(show("disk_nearer", bhg::prefix_rho_wide_call(c, 1.0, low, 0)), 0.25));
    // no clear ball: anything not finite, on the horizon, inside, the zero origin
    const double on_hor[3] = {0.0, 1.0, 0.0}, inside[3] = {0.1, 0.0, 0.2}, bad[3] = {nan, 0.0, 30.0}, huge[3] = {inf, 0.0, 0.0};
    const double zero[3] = {0.0, 0.0, 0.0};
    struct {
        const char *name;
        const double *x0;
    } none[] = {{"nan_origin", bad}, {"inf_origin", huge}, {"on_horizon", on_hor}, {"inside", inside}, {"zero_origin", zero}};
    for (auto &k : none)
        for (int ns : {0, 1}) {
            c = bhg::prefix_clearance(1.0, 0.0, false, nullptr, 0, k.x0);
            r = bhg::prefix_rho_wide_call(c, 1.0, k.x0, ns);
            if (ns == 0) show(k.name, r);
            // (a caller's own clearance for such an origin: still the deep call's answer, or 5/4 of its three quarters)
            CHECK(c == 0.0 && r == 0.0 &&
                  near(bhg::prefix_rho_wide_call(10.0, 1.0, k.x0, ns), (ns ? 1.0 : 1.25) * bhg::prefix_rho_deep_call(10.0, 1.0, k.x0, ns)));
        }
    for (int ns : {0, 1})
        for (double cc : {0.0, -1.0, nan, inf})
            CHECK(bhg::prefix_rho_wide_call(cc, 1.0, CAM, ns) == 0.0 && bhg::prefix_rho_deep_call(cc, 1.0, CAM, ns) == 0.0);
    CHECK(bhg::prefix_rho_wide_call(10.0, nan, CAM, 0) == bhg::prefix_rho_deep_call(10.0, nan, CAM, 0));
    // over a grid of clearances: 5/4 of the deep call's radius exactly where that is its three quarters, the deep call's elsewhere
    int n_wide = 0, n_same = 0;
    for (double clear = 1e-9; clear < 1e9; clear *= 1.7)
        for (int ns : {0, 1, 8})
            for (double r_hor : {1e-3, 1.0, 12.0}) {
                const double deep = bhg::prefix_rho_deep_call(clear, r_hor, CAM, ns), wide = bhg::prefix_rho_wide_call(clear, r_hor, CAM, ns);
                const bool three_quarters = near(deep, 0.75 * std::fmin(clear, 30.0));
                CHECK(deep > 0.0 && (three_quarters == (ns == 0 && clear >= 30.0 - r_hor)));
                if (three_quarters) {
                    CHECK(near(wide, 1.25 * deep) && near(wide, 0.9375 * std::fmin(clear, 30.0)));
                    n_wide++;
                } else {
                    CHECK(wide == deep);
                    n_same++;
                }
                CHECK(bhg::prefix_replay_ok(clear, wide));      // (the call's own clearance passes the test of the rho it fixed)
            }
    CHECK(n_wide > 20 && n_same > 200);
    CHECK(bhg::PREFIX_RHO_FRACTION_WIDE * (1.0 + bhg::PREFIX_MARGIN) < 1.0);
    CHECK(bhg::prefix_rho_by_rule(WIDE, 29.0, 1.0, CAM, 0) == 27.1875 && near(bhg::prefix_rho_by_rule(DEEP, 29.0, 1.0, CAM, 0), 21.75) &&
          near(bhg::prefix_rho_by_rule(bhg::PREFIX_MODE_RECORD, 29.0, 1.0, CAM, 0), 7.25) && bhg::prefix_rho_by_rule(REPLAY, 29.0, 1.0, CAM, 0) == 0.0);

    // ---- the owner -----------------------------------------------------------------------------------------------------------
    Owner w;
    // a fresh owner holds nothing and asks for nothing
    CHECK(w.o.next(WIDE, 29.0, 1.0, CAM, 0, NONE, NONE, 0.0) == NONE && w.o.rho == 0.0);
    // recorded wide; one refusal in a run of replays changes nothing
    CHECK(w.first(0.0) == WIDE);
    for (int k = 0; k < 3; k++) CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY);
    CHECK(show("owner_rho_wide", w.o.rho) == 27.1875 && w.o.refused_run == 0);
    CHECK(w.next(45.0) == REPLAY && w.last_used == NONE);      // an exit sphere 15 from the camera, inside the ball: refused
    CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.refused_run == 1);
    CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.refused_run == 0);
    CHECK(w.records == 1 && w.refusals == 1 && w.replays == 5);
    // two in a row ask for a record, by the rule on the call's own scene: the quarter of 15
    CHECK(w.next(45.0) == REPLAY && w.last_used == NONE);
    CHECK(w.next(45.0) == REPLAY && w.last_used == NONE && w.o.refused_run == 1);
    CHECK(w.next(45.0) == WIDE && w.last_used == WIDE && w.o.refused_run == 2 && near(w.last_rho, 3.75));
    CHECK(w.next(45.0) == REPLAY && w.last_used == REPLAY);
    CHECK(near(show("owner_rho_shrunk", w.o.rho), 3.75) && w.o.refused_run == 0 && w.o.roomy_run == 0);   // (a record resets both counters)
    CHECK(w.records == 2 && w.refusals == 3);
    // seven roomy calls (the rule would give 27.1875 >= 2 x 3.75), then the sphere is back: nothing is recorded, the run starts over
    for (int k = 1; k <= 7; k++) CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.roomy_run == k);
    CHECK(w.next(45.0) == REPLAY && w.o.roomy_run == 0);
    for (int k = 1; k <= 7; k++) CHECK(w.next(0.0) == REPLAY && w.o.roomy_run == k);
    CHECK(w.records == 2);
    // eight roomy calls: the next one records, wide again
    CHECK(w.next(0.0) == REPLAY && w.o.roomy_run == 8);
    CHECK(w.next(0.0) == WIDE && w.last_used == WIDE && w.last_rho == 27.1875);
    CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.rho == 27.1875 && w.o.roomy_run == 0 && w.o.refused_run == 0);
    CHECK(w.records == 3 && w.refusals == 3);
    show("owner_records", w.records);
    // a refusal resets nothing of the roomy run and a roomy call nothing of the refused run: a record resets both
    bhg::PrefixOwner o;
    o.rho = 3.75;
    o.refused_run = 1;
    o.roomy_run = 5;
    CHECK(o.next(WIDE, 29.0, 1.0, CAM, 0, REPLAY, NONE, 3.75) == WIDE && o.refused_run == 2 && o.roomy_run == 6);
    CHECK(o.next(WIDE, 29.0, 1.0, CAM, 0, WIDE, WIDE, 27.1875) == REPLAY && o.rho == 27.1875 && o.refused_run == 0 && o.roomy_run == 0);
    // a recording call that wrote nothing (a step budget the records could exhaust) leaves the held records standing
    CHECK(o.next(WIDE, 29.0, 1.0, CAM, 0, WIDE, NONE, 0.0) == REPLAY && o.rho == 27.1875);
    // ... and a fresh owner whose first call wrote nothing holds nothing
    o = bhg::PrefixOwner();
    CHECK(o.next(WIDE, 29.0, 1.0, CAM, 0, WIDE, NONE, 0.0) == NONE && o.rho == 0.0);
    // a scene without any clear ball (the camera on the disk plane: clearance 0) is waited out, however long it refuses
    o = bhg::PrefixOwner();
    CHECK(o.next(WIDE, 29.0, 1.0, CAM, 0, WIDE, WIDE, 27.1875) == REPLAY);
    for (int k = 0; k < 5; k++) CHECK(o.next(WIDE, 0.0, 1.0, CAM, 0, REPLAY, NONE, 27.1875) == REPLAY && o.rho == 27.1875);
    CHECK(o.refused_run == 5 && o.next(WIDE, 15.0, 1.0, CAM, 0, REPLAY, NONE, 27.1875) == WIDE);
    // an owner that records by the deep rule grows and shrinks by that rule
    o = bhg::PrefixOwner();
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, DEEP, DEEP, 2.5) == REPLAY && o.roomy_run == 1);      // (21.75 >= 5)
    o.roomy_run = 8;
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 2.5) == DEEP);
    // the ninth call records only if it has the room itself
    o.roomy_run = 8;
    CHECK(o.next(DEEP, 15.0, 1.0, CAM, 0, REPLAY, REPLAY, 2.5) == REPLAY && o.roomy_run == 0);   // (3.75 < 5)

    // ---- promotion: an owner that records by the deep rule and names the wide one -------------------------------------------
    CHECK(bhg::PREFIX_OWNER_PROMOTE_CALLS == 32);
    o = bhg::PrefixOwner();
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, DEEP, DEEP, 21.75, WIDE) == REPLAY && o.rho == 21.75 && o.clean_run == 0);
    // 31 replayed calls behind it: not yet; one refusal among them starts the run over
    for (int k = 1; k <= 30; k++) CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 21.75, WIDE) == REPLAY && o.clean_run == k);
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, NONE, 21.75, WIDE) == REPLAY && o.clean_run == 0 && o.refused_run == 1);
    for (int k = 1; k <= 31; k++) CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 21.75, WIDE) == REPLAY && o.clean_run == k);
    // the 32nd: the next call records by the wide rule -- unless the owner names none, or the wide rule has no more to give
    bhg::PrefixOwner o2 = o, o3 = o;
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 21.75, WIDE) == WIDE && o.clean_run == 32);
    CHECK(o2.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 21.75) == REPLAY && o2.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 21.75, NONE) == REPLAY);
    CHECK(o3.next(DEEP, 29.0, 1.0, CAM, 1, REPLAY, REPLAY, 21.75, WIDE) == REPLAY);          // (an object sphere: the quarter by either rule)
    // promoted: the wide records are kept, no second promotion for the same ball, the counters start over
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, WIDE, WIDE, 27.1875, WIDE) == REPLAY && o.rho == 27.1875 && o.clean_run == 0);
    for (int k = 1; k <= 40; k++) CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 27.1875, WIDE) == REPLAY);
    // an exit sphere at 45 inside the wide ball: two refusals, then new records by the owner's FIRST rule on that scene (the quarter)
    CHECK(o.next(DEEP, 15.0, 1.0, CAM, 0, REPLAY, NONE, 27.1875, WIDE) == REPLAY);
    CHECK(o.next(DEEP, 15.0, 1.0, CAM, 0, REPLAY, NONE, 27.1875, WIDE) == DEEP && o.clean_run == 0);
    CHECK(o.next(DEEP, 15.0, 1.0, CAM, 0, DEEP, DEEP, 3.75, WIDE) == REPLAY && o.rho == 3.75);
    // the sphere goes: eight roomy calls, back to the deep rule's ball (not at once to the wide one)
    for (int k = 1; k <= 8; k++) CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 3.75, WIDE) == REPLAY);
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, REPLAY, REPLAY, 3.75, WIDE) == DEEP);
    show("owner_promote_calls", bhg::PREFIX_OWNER_PROMOTE_CALLS);
    return 0;
}

// prefix_rim_driver.cpp -- the radius rule of the RIM start-up records (csrc/prefix_clearance.h: prefix_rho_rim_call, behind
// BHG_PREFIX_RECORD_RIM), how a replaying call tells such records by their rho, and the owners' ladder deep -> wide -> rim
// (PrefixOwner with promote = RIM), compiled with the HOST compiler, plain and under AddressSanitizer + UBSan, by
// tests/test_rim_prefix_host.py: 1 - 2^-10 of min(clearance, |x0|) exactly where the wide call takes its fifteen sixteenths, what the
// wide call returns everywhere else; the wide rung after 32 clean replays as before, the rim rung after 96 more; refusal, shrink
// and grow by the owner's first rule.
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
              WIDE = bhg::PREFIX_MODE_RECORD_WIDE, RIM = bhg::PREFIX_MODE_RECORD_RIM;
static const double CAM[3] = {0.0, 0.0, 30.0};
constexpr int RIM_RUN = bhg::PREFIX_OWNER_PROMOTE_RIM_CALLS;
constexpr double RIM_RHO = 29.0 * (1.0 - 1.0 / 1024.0);      // 28.9716796875, exact in binary

// An owner from the bench camera, r_s = 1, whose scene is an exit sphere (0: none), and the library's answers played by the rule:
// the rule's rho for a recording call, prefix_replay_ok for a replaying one (bhgeo_capi.hip).
struct Owner {
    bhg::PrefixOwner o;
    int rule = DEEP, promote = RIM;
    int last_mode = NONE, last_used = NONE;
    double last_rho = 0.0;
    int records = 0, replays = 0, refusals = 0;

    int call(int ask, double r_exit)
    {
        const double c = bhg::prefix_clearance(1.0, r_exit, false, nullptr, 0, CAM);
        last_mode = ask;
        last_used = NONE;
        if (bhg::prefix_mode_records(ask)) {
            last_rho = bhg::prefix_rho_by_rule(ask, c, 1.0, CAM, 0);
            last_used = last_rho > 0.0 ? ask : NONE;
            records += last_used == ask;
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
        return call(rule, r_exit);
    }
    int next(double r_exit)
    {
        const double c = bhg::prefix_clearance(1.0, r_exit, false, nullptr, 0, CAM);
        const int ask = o.next(rule, c, 1.0, CAM, 0, last_mode, last_used, last_rho, promote);
        call(ask, r_exit);
        return ask;
    }
};

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(bhg::PREFIX_RHO_FRACTION_RIM == 1.0 - 1.0 / 1024.0 && bhg::PREFIX_RHO_FRACTION_WIDE == 0.9375);
    CHECK(RIM == 6 && WIDE == 5 && DEEP == 4 && REPLAY == 2 && bhg::PREFIX_RIM_ACCEPTED == 9 && bhg::PREFIX_RIM_ATTEMPTS == 15);
    CHECK(bhg::PREFIX_OWNER_PROMOTE_CALLS == 32 && bhg::PREFIX_OWNER_PROMOTE_RIM_CALLS == 96);
    // the fraction leaves the margin of the replay test nine hundred times over
    CHECK(bhg::PREFIX_RHO_FRACTION_RIM * (1.0 + 900.0 * bhg::PREFIX_MARGIN) < 1.0);

    // ---- the radius ----------------------------------------------------------------------------------------------------------
    double c = bhg::prefix_clearance(1.0, 0.0, false, nullptr, 0, CAM);
    double r = show("bench_camera", bhg::prefix_rho_rim_call(c, 1.0, CAM, 0));
    CHECK(c == 29.0 && r == RIM_RHO && bhg::prefix_replay_ok(29.0, r) && !bhg::prefix_replay_ok(r, r));
    show("bench_camera_reaches", 30.0 - r);
    CHECK(30.0 - r > 1.0 && 30.0 - r < 1.03);                      // (above the horizon, by 2^-10 of the clearance)
    CHECK(bhg::prefix_rho_wide_call(c, 1.0, CAM, 0) == 27.1875);   // (the others are what they were)
    // one object sphere anywhere, an exit sphere or a disk plane nearer than the horizon: the wide call's value, to the bit
    const double sp[3][4] = {{40.0, 40.0, 40.0, 1.0}, {0.0, 0.0, 20.0, 2.0}, {0.0, 0.0, -20.0, 2.0}};
    const char *sp_name[3] = {"one_sphere_far", "one_sphere_near", "one_sphere_behind"};
    for (int j = 0; j < 3; j++) {
        c = bhg::prefix_clearance(1.0, 0.0, false, &sp[j][0], 1, CAM);
        r = show(sp_name[j], bhg::prefix_rho_rim_call(c, 1.0, CAM, 1));
        CHECK(r == bhg::prefix_rho_wide_call(c, 1.0, CAM, 1) && r == bhg::prefix_rho(c, CAM));
    }
    c = bhg::prefix_clearance(1.0, 45.0, false, nullptr, 0, CAM);
    r = show("exit_45", bhg::prefix_rho_rim_call(c, 1.0, CAM, 0));
    CHECK(near(r, 3.75) && r == bhg::prefix_rho_wide_call(c, 1.0, CAM, 0));
    c = bhg::prefix_clearance(1.0, 70.0, false, nullptr, 0, CAM);
    CHECK(show("exit_farther", bhg::prefix_rho_rim_call(c, 1.0, CAM, 0)) == RIM_RHO);
    c = bhg::prefix_clearance(1.0, 0.0, true, nullptr, 0, CAM);
    r = show("disk_plane_30", bhg::prefix_rho_rim_call(c, 1.0, CAM, 0));
    CHECK(r == RIM_RHO && std::fabs(CAM[2]) > r * (1.0 + bhg::PREFIX_MARGIN));
    const double low[3] = {20.0, 0.0, 1.0};
    c = bhg::prefix_clearance(1.0, 0.0, true, nullptr, 0, low);
    CHECK(near(show("disk_nearer", bhg::prefix_rho_rim_call(c, 1.0, low, 0)), 0.25));
    // no clear ball
    const double on_hor[3] = {0.0, 1.0, 0.0}, inside[3] = {0.1, 0.0, 0.2}, bad[3] = {nan, 0.0, 30.0}, huge[3] = {inf, 0.0, 0.0};
    const double zero[3] = {0.0, 0.0, 0.0};
    struct {
        const char *name;
        const double *x0;
    } none[] = {{"nan_origin", bad}, {"inf_origin", huge}, {"on_horizon", on_hor}, {"inside", inside}, {"zero_origin", zero}};
    for (auto &k : none)
        for (int ns : {0, 1}) {
            c = bhg::prefix_clearance(1.0, 0.0, false, nullptr, 0, k.x0);
            r = bhg::prefix_rho_rim_call(c, 1.0, k.x0, ns);
            if (ns == 0) show(k.name, r);
            CHECK(c == 0.0 && r == 0.0 && !bhg::prefix_rho_is_rim(RIM_RHO, 1.0, k.x0));
        }
    for (int ns : {0, 1})
        for (double cc : {0.0, -1.0, nan, inf}) CHECK(bhg::prefix_rho_rim_call(cc, 1.0, CAM, ns) == 0.0);
    CHECK(bhg::prefix_rho_rim_call(10.0, nan, CAM, 0) == bhg::prefix_rho_wide_call(10.0, nan, CAM, 0));
    // over a grid: the rim fraction exactly where the wide call leaves the deep call's value behind, the wide call's value elsewhere,
    // the call's own clearance passes the test of the rho it fixed, and the rho tells the rule
    int n_rim = 0, n_same = 0;
    for (double clear = 1e-9; clear < 1e9; clear *= 1.7)
        for (int ns : {0, 1, 8})
            for (double r_hor : {1e-3, 1.0, 12.0}) {
                const double wide = bhg::prefix_rho_wide_call(clear, r_hor, CAM, ns), rim = bhg::prefix_rho_rim_call(clear, r_hor, CAM, ns);
                const bool applies = ns == 0 && clear >= 30.0 - r_hor;
                if (applies) {
                    CHECK(near(rim, (1.0 - 1.0 / 1024.0) * std::fmin(clear, 30.0)) && rim > wide);
                    n_rim++;
                } else {
                    CHECK(rim == wide);
                    n_same++;
                }
                CHECK(bhg::prefix_replay_ok(clear, rim));
                // (a scene's clearance is never more than the way to the horizon: there the rho says which rule wrote the records)
                if (clear <= 30.0 - r_hor) {
                    CHECK(bhg::prefix_rho_is_rim(rim, r_hor, CAM) == applies && !bhg::prefix_rho_is_rim(wide, r_hor, CAM));
                    CHECK(!bhg::prefix_rho_is_rim(bhg::prefix_rho_deep_call(clear, r_hor, CAM, ns), r_hor, CAM));
                }
            }
    CHECK(n_rim > 20 && n_same > 200);
    CHECK(bhg::prefix_rho_is_rim(RIM_RHO, 1.0, CAM) && !bhg::prefix_rho_is_rim(27.1875, 1.0, CAM) && !bhg::prefix_rho_is_rim(nan, 1.0, CAM) &&
          !bhg::prefix_rho_is_rim(0.0, 1.0, CAM));
    CHECK(bhg::prefix_rho_by_rule(RIM, 29.0, 1.0, CAM, 0) == RIM_RHO && bhg::prefix_rho_by_rule(WIDE, 29.0, 1.0, CAM, 0) == 27.1875);

    // ---- the ladder: deep first, wide after 32 clean replays, rim after 96 more ---------------------------------------------
    Owner w;
    CHECK(w.o.next(DEEP, 29.0, 1.0, CAM, 0, NONE, NONE, 0.0, RIM) == NONE && w.o.rho == 0.0);
    CHECK(w.first(0.0) == DEEP);
    for (int k = 1; k <= 32; k++) CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY);
    CHECK(near(w.o.rho, 21.75) && w.o.clean_run == 31);
    CHECK(w.next(0.0) == WIDE && w.last_used == WIDE && w.last_rho == 27.1875);          // the 34th call, as without a rim rule
    for (int k = 1; k <= RIM_RUN; k++) CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.rho == 27.1875);
    CHECK(w.next(0.0) == RIM && w.last_used == RIM && w.last_rho == RIM_RHO);            // the 131st
    show("owner_rim_call", 1 + 32 + 1 + RIM_RUN + 1);
    for (int k = 1; k <= 80; k++) CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY);  // no further rung, no second promotion
    CHECK(show("owner_rho_rim", w.o.rho) == RIM_RHO && w.records == 3 && w.refusals == 0);
    // an owner that names the wide rule stops there, one that names none stays deep (the ladder without a rim rule, call for call)
    Owner v;
    v.promote = WIDE;
    CHECK(v.first(0.0) == DEEP);
    for (int k = 1; k <= 32; k++) CHECK(v.next(0.0) == REPLAY);
    CHECK(v.next(0.0) == WIDE);
    for (int k = 1; k <= 100; k++) CHECK(v.next(0.0) == REPLAY);
    CHECK(v.o.rho == 27.1875 && v.records == 2);
    Owner u;
    u.promote = NONE;
    CHECK(u.first(0.0) == DEEP);
    for (int k = 1; k <= 100; k++) CHECK(u.next(0.0) == REPLAY);
    CHECK(near(u.o.rho, 21.75));
    // an owner that records wide from its first call climbs the one rung that is left
    Owner x;
    x.rule = WIDE;
    CHECK(x.first(0.0) == WIDE);
    for (int k = 1; k <= RIM_RUN; k++) CHECK(x.next(0.0) == REPLAY);
    CHECK(x.next(0.0) == RIM && x.last_rho == RIM_RHO);
    // one refused call in the run on wide records starts it over
    Owner y;
    CHECK(y.first(0.0) == DEEP);
    for (int k = 1; k <= 32; k++) CHECK(y.next(0.0) == REPLAY);
    CHECK(y.next(0.0) == WIDE);
    for (int k = 1; k <= RIM_RUN - 1; k++) CHECK(y.next(0.0) == REPLAY);
    CHECK(y.next(45.0) == REPLAY && y.last_used == NONE);
    for (int k = 1; k <= RIM_RUN; k++) CHECK(y.next(0.0) == REPLAY && y.last_used == REPLAY);
    CHECK(y.o.refused_run == 0 && y.next(0.0) == RIM);
    // a scene that keeps the quarter (an object sphere) earns nothing, however long it replays
    bhg::PrefixOwner q;
    CHECK(q.next(DEEP, 29.0, 1.0, CAM, 1, DEEP, DEEP, 7.25, RIM) == REPLAY);
    for (int k = 1; k <= 100; k++) CHECK(q.next(DEEP, 29.0, 1.0, CAM, 1, REPLAY, REPLAY, 7.25, RIM) == REPLAY);

    // ---- refusal, shrink, grow on rim records: by the owner's first rule ------------------------------------------------------
    // an exit sphere at 58.5 stands 28.5 from the camera: outside the wide ball (27.19), inside the rim ball (28.97)
    CHECK(w.next(58.5) == REPLAY && w.last_used == NONE);
    CHECK(w.next(0.0) == REPLAY && w.last_used == REPLAY && w.o.refused_run == 1);
    CHECK(w.next(0.0) == REPLAY && w.o.refused_run == 0 && w.records == 3);
    CHECK(w.next(58.5) == REPLAY && w.last_used == NONE);
    CHECK(w.next(58.5) == REPLAY && w.last_used == NONE);
    CHECK(w.next(58.5) == DEEP && w.last_used == DEEP && near(show("owner_rho_shrunk", w.last_rho), 0.25 * 28.5));
    CHECK(w.next(58.5) == REPLAY && w.last_used == REPLAY && w.o.clean_run == 0);
    // the sphere goes: eight roomy calls, the deep ball (21.75 >= 2 x 7.125), then the ladder from its foot
    for (int k = 1; k <= 8; k++) CHECK(w.next(0.0) == REPLAY && w.o.roomy_run == k);
    CHECK(w.next(0.0) == DEEP && near(w.last_rho, 21.75));
    for (int k = 1; k <= 32; k++) CHECK(w.next(0.0) == REPLAY);
    CHECK(w.next(0.0) == WIDE);
    for (int k = 1; k <= RIM_RUN; k++) CHECK(w.next(0.0) == REPLAY);
    CHECK(w.next(0.0) == RIM && w.last_rho == RIM_RHO);
    show("owner_records", w.records);
    CHECK(w.records == 7 && w.refusals == 3);
    // a rim-recording call that wrote nothing (a step budget its records could exhaust) leaves the wide records standing
    bhg::PrefixOwner o;
    o.rho = 27.1875;
    CHECK(o.next(DEEP, 29.0, 1.0, CAM, 0, RIM, NONE, 0.0, RIM) == REPLAY && o.rho == 27.1875 && o.clean_run == 0);

    // ---- the step budget of a replay ----------------------------------------------------------------------------------------
    CHECK(bhg::prefix_owner_fit_budget(REPLAY, RIM_RHO, 1.0, CAM, 15) == NONE && bhg::prefix_owner_fit_budget(REPLAY, RIM_RHO, 1.0, CAM, 16) == REPLAY);
    CHECK(bhg::prefix_owner_fit_budget(REPLAY, 27.1875, 1.0, CAM, 13) == REPLAY && bhg::prefix_owner_fit_budget(RIM, RIM_RHO, 1.0, CAM, 13) == RIM);
    CHECK(bhg::prefix_owner_fit_budget(NONE, RIM_RHO, 1.0, CAM, 13) == NONE && bhg::prefix_owner_fit_budget(REPLAY, RIM_RHO, 1.0, CAM, 1) == NONE);
    return 0;
}

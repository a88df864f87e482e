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
//               (deep records, BHG_PREFIX_RECORD_DEEP: PREFIX_RHO_FRACTION_DEEP of it while the scene holds no object sphere;
//               wide records, BHG_PREFIX_RECORD_WIDE: PREFIX_RHO_FRACTION_WIDE of it there;
//               rim records, BHG_PREFIX_RECORD_RIM: PREFIX_RHO_FRACTION_RIM of it there),
//   a call replays only while its own clearance > rho (1 + PREFIX_MARGIN): the one validity test, whichever rule wrote them.
#pragma once
#include <cmath>

namespace bhg {

// A quarter: with K_MAX = 4 steps that each grow by at most the controller's factor 10, the steps kept are the climb from scipy's
// start guess (h0 ~ 0.01) to the settled step size (~ the distance to the hole), and a small ball survives more scene changes
// (an object sphere moving about).  It is NOT true that a larger ball holds no more steps, as this comment used to say: a
// headline ray (camera at r = 30, r_s = 1: clearance 29) takes three climbing steps that end 0.01, 0.08 and 0.8 from the camera,
// a fourth of 7 to 20, which leaves the quarter ball (7.25) for 90 % of the rays, and a fifth that takes 2 to 3 attempts.
// Attempts kept per ray, of 12.33, on 400 seeded headline rays (scipy RK45 at the bench's tolerances):
//   rho                 stop at the first rejection, <= 4 accepted    rejections kept, <= 6 accepted
//    7.25  (1/4)                     3.09                                      3.25
//   14.5   (1/2)                     3.78                                      5.24
//   21.75  (3/4)                     3.92                                      5.94
//   27.0   (0.93)                    3.93                                      7.71
// ... and of 12.79 on 300 uniform rays of the headline window (the same rule, rejections kept, stop in front of an ending attempt):
//   rho                 <= 6 accepted, <= 12 attempts      <= 8 accepted, <= 12 attempts      <= 8 accepted, <= 16 attempts
//    7.25    (1/4)             3.24                               3.24                               3.24
//   21.75    (3/4)             6.04                               6.04                               6.04
//   27.1875  (15/16)           7.91, 10 % at the cap              8.05, none at a cap                8.05
//   28.09375 (31/32)           8.01, 18 % at the cap              8.34                               8.36
constexpr double PREFIX_RHO_FRACTION = 0.25;
// Three quarters, the deep records' fraction in a scene WITHOUT object spheres: nothing moves there -- horizon, exit sphere and
// disk plane change only when the scene is edited, and prefix_replay_ok holds every call to the ball anyway.  (0.93 keeps more
// still, but that ball reaches r ~ 3 from a camera at 30 and gives up most of the tolerance to such edits.)
constexpr double PREFIX_RHO_FRACTION_DEEP = 0.75;
// Fifteen sixteenths, the wide records' fraction where the deep rule takes its three quarters: from the headline camera the ball
// (27.1875) reaches r = 2.81.  The tolerance to edits it gives up is a matter of speed alone -- prefix_replay_ok refuses, the
// call runs the plain start -- and an owner gets it back by recording again after refusals (PrefixOwner below).  31/32 adds 0.3
// attempts for a ball that ends 0.9 above the photon sphere: not taken.
constexpr double PREFIX_RHO_FRACTION_WIDE = 0.9375;
// 1 - 2^-10, the rim records' fraction where the wide rule takes its fifteen sixteenths: from the headline camera the ball (28.97)
// ends 0.028 above the horizon.  What kept the wide ball away from the hole was never validity: the one surface the ball nears
// there is the horizon, which cannot move under kept records (r_s and the spin are on the list of bhg_start_steps_match), the
// recorder stops in front of the attempt that would end a ray, and the only other role of the fraction is the rounding margin
// of prefix_replay_ok (2^-10 is 977 PREFIX_MARGINs).  The same rule on 3 000 uniform rays of the headline window
// (scripts/dev/prefix_rule_restate.py; 12.35 attempts per ray), attempts kept per ray and the share of rays at a cap:
//   rho                    <= 8 accepted, <= 12 attempts   <= 8, <= 16       <= 9, <= 14       <= 9, <= 15       <= 10, <= 16
//   27.1875  (15/16)           7.85, 1.1 %                  7.85, 0           7.85, 0           7.85, 0           7.85, 0
//   28.09375 (31/32)           8.16, 4.7 %                  8.17, 0.2 %       8.17, 0.2 %       8.17, 0.0 %       8.17, 0
//   28.54688 (63/64)           8.21, 5.8 %                  8.23, 1.0 %       8.24, 0.9 %       8.24, 0.1 %       8.24, 0
//   28.77344 (127/128)         8.28, 6.9 %                  8.30, 2.2 %       8.32, 1.1 %       8.32, 0.2 %       8.32, 0.0 %
//   28.97168 (1 - 2^-10)       8.32, 7.5 %                  8.35, 3.3 %       8.38, 1.6 %       8.38, 0.4 %       8.39, 0.2 %
// so the rim rule keeps up to PREFIX_RIM_ACCEPTED = 9 accepted steps in PREFIX_RIM_ATTEMPTS = 15 attempts, the smallest caps that
// leave fewer than 1 % of the rays at a cap, and half an attempt per ray more than the wide rule (300 rays of another seed: 8.04 ->
// 8.45).
constexpr double PREFIX_RHO_FRACTION_RIM = 1.0 - 1.0 / 1024.0;
constexpr int PREFIX_RIM_ACCEPTED = 9, PREFIX_RIM_ATTEMPTS = 15;
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

// ... of a WIDE recording call: fifteen sixteenths exactly where the deep call takes its three quarters (no object sphere, the
// horizon the nearest surface), and what the deep call returns everywhere else: the quarter, 0 for the degenerate inputs
inline double prefix_rho_wide_call(double clearance, double r_hor, const double x0[3], int n_spheres)
{
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    const bool horizon_nearest = std::isfinite(r0) && r_hor >= 0.0 && clearance >= r0 - r_hor;
    if (!horizon_nearest || n_spheres > 0) return prefix_rho_deep_call(clearance, r_hor, x0, n_spheres);
    if (!std::isfinite(clearance) || !(clearance > 0.0) || !(r0 > 0.0)) return 0.0;
    return PREFIX_RHO_FRACTION_WIDE * std::fmin(clearance, r0);
}

// ... of a RIM recording call: PREFIX_RHO_FRACTION_RIM exactly where the wide call takes its fifteen sixteenths, and what the wide
// call returns everywhere else
inline double prefix_rho_rim_call(double clearance, double r_hor, const double x0[3], int n_spheres)
{
    const double wide = prefix_rho_wide_call(clearance, r_hor, x0, n_spheres);
    if (!(wide > prefix_rho_deep_call(clearance, r_hor, x0, n_spheres))) return wide;
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    return PREFIX_RHO_FRACTION_RIM * std::fmin(clearance, r0);
}

// Were records of this rho written by the rim rule?  A replaying call is handed a rho and no rule, but from this origin and with
// this horizon -- both the same as when the records were written, or they may not be replayed at all -- no other rule gives a rho
// above the wide rule's for the horizon alone.  What it decides is the step budget a replay needs (PREFIX_RIM_ATTEMPTS).
inline bool prefix_rho_is_rim(double rho, double r_hor, const double x0[3])
{
    const double r0 = std::sqrt(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]);
    if (!std::isfinite(rho) || !std::isfinite(r0) || !(r_hor >= 0.0) || !(r0 > r_hor)) return false;
    return rho > prefix_rho_wide_call(r0 - r_hor, r_hor, x0, 0);
}

// may a call whose scene has this clearance replay records written with rho?
inline bool prefix_replay_ok(double clearance, double rho)
{
    return std::isfinite(rho) && rho > 0.0 && clearance > rho * (1.0 + PREFIX_MARGIN);
}

// ------------------------------------------------------------------------------------------------------------------------
// The owner of a ray set's records (bhg_frame, DeviceFrame's StartSteps through bhg_prefix_owner_next): when to record AGAIN.
// The rays' own invalidation -- other rays, another origin, parameters that bhg_start_steps_match() rejects -- is the owner's
// and starts from scratch (a fresh PrefixOwner, a recording call).  What is decided here is the scene's part:
//   shrink: the last two calls in a row were refused (the scene has come into the ball and stays there: one refused frame, an
//           object passing through, is not enough) -- record now, by the rule on the call's own scene;
//   grow:   for PREFIX_OWNER_GROW_CALLS calls in a row the rule gave the call's scene a rho of at least PREFIX_OWNER_GROW_FACTOR
//           times the kept one (what held the ball small has gone for good) -- record now.
// and one more, for an owner that records by a cautious rule and names a wider one to be promoted to (the owners' default: deep
// first, wide later -- the wide ball gives up the tolerance to edits, and an owner's first frames are where scenes get edited):
//   promote: the last PREFIX_OWNER_PROMOTE_CALLS calls in a row all replayed and the wider rule gives this call's scene more than
//           the kept rho -- record now, by the wider rule.  Shrink and grow stay with the cautious rule.
// PROMOTE_CALLS is the rent-or-buy point, by the headline's figures: a replay of wide records saves 0.16 ms
// on one of deep records; the promoting call costs 1.6 ms more than the replay it replaces (its rays start themselves, and the
// recording pass), and an edit that then reaches into the wide ball but not into the deep one costs 2.5 ms more (two refused
// frames, a recording call): 4.1 / 0.16 = 25 frames.  Waiting that long before buying is within a factor two of the best choice
// whenever the edit comes; 32 leaves room for frames whose replays save less than the headline's.
// The rules form a ladder, deep -> wide -> rim, and an owner that names the RIM rule as its promotion climbs it a rung at a time:
// a clean run earns the wide rule first (unchanged), and a further clean run on wide records, PREFIX_OWNER_PROMOTE_RIM_CALLS
// long, the rim rule.  The same arithmetic with (n)'s measured figures: a replay of rim records saves
// 0.052 ms on one of wide records, a third of what the wide rung saved; the promoting call costs 1.7 ms more than the replay
// it replaces (the recording pass is 0.07 ms longer) and an edit that then reaches into the rim ball but not into the wide one
// the same 2.5 ms: 4.2 / 0.052 = 80 frames, and 96 leaves the same room.  The rim rule is earned by a ray set's 131st trace.
// The modes are the C API's (include/bhgeo.h; bhgeo_capi.hip asserts the values).
constexpr int PREFIX_MODE_NONE = 0, PREFIX_MODE_RECORD = 1, PREFIX_MODE_REPLAY = 2, PREFIX_MODE_RECORD_DEEP = 4, PREFIX_MODE_RECORD_WIDE = 5,
              PREFIX_MODE_RECORD_RIM = 6;
constexpr int PREFIX_OWNER_SHRINK_CALLS = 2, PREFIX_OWNER_GROW_CALLS = 8, PREFIX_OWNER_PROMOTE_CALLS = 32, PREFIX_OWNER_PROMOTE_RIM_CALLS = 96;
constexpr double PREFIX_OWNER_GROW_FACTOR = 2.0;

inline bool prefix_mode_records(int mode)
{
    return mode == PREFIX_MODE_RECORD || mode == PREFIX_MODE_RECORD_DEEP || mode == PREFIX_MODE_RECORD_WIDE || mode == PREFIX_MODE_RECORD_RIM;
}

// the rho a recording call by this rule fixes (the step budget apart: see deep_fits in bhgeo_capi.hip)
inline double prefix_rho_by_rule(int rule, double clearance, double r_hor, const double x0[3], int n_spheres)
{
    if (rule == PREFIX_MODE_RECORD_RIM) return prefix_rho_rim_call(clearance, r_hor, x0, n_spheres);
    if (rule == PREFIX_MODE_RECORD_WIDE) return prefix_rho_wide_call(clearance, r_hor, x0, n_spheres);
    if (rule == PREFIX_MODE_RECORD_DEEP) return prefix_rho_deep_call(clearance, r_hor, x0, n_spheres);
    return rule == PREFIX_MODE_RECORD ? prefix_rho(clearance, x0) : 0.0;
}

struct PrefixOwner {
    double rho = 0.0;       // the held records were written with this radius (0: none are held)
    int refused_run = 0;    // calls in a row, up to the last one, that asked to replay and were refused
    int roomy_run = 0;      // calls in a row, this one included, whose scene the rule gives GROW_FACTOR times rho or more
    int clean_run = 0;      // calls in a row, up to the last one, that replayed

    // What the next call asks for: PREFIX_MODE_REPLAY, `rule` or `promote` (record now, by that rule) or PREFIX_MODE_NONE
    // (nothing is held).  The last call of this owner asked for last_mode and reported last_used and (a recording call) last_rho;
    // last_mode = NONE before the first call and after a call without a prefix.  The call being planned has this clearance,
    // horizon and sphere count.  promote: the wider rule a long clean run earns, or NONE.
    int next(int rule, double clearance, double r_hor, const double x0[3], int n_spheres, int last_mode, int last_used, double last_rho,
             int promote = PREFIX_MODE_NONE)
    {
        if (prefix_mode_records(last_mode)) {
            // (a recording call that wrote nothing -- a step budget the records could exhaust -- left the held ones as they were)
            if (last_used == last_mode) rho = std::isfinite(last_rho) && last_rho > 0.0 ? last_rho : 0.0;
            refused_run = roomy_run = clean_run = 0;
        } else if (last_mode == PREFIX_MODE_REPLAY) {
            refused_run = last_used == PREFIX_MODE_REPLAY ? 0 : refused_run + 1;
            clean_run = last_used == PREFIX_MODE_REPLAY ? clean_run + 1 : 0;
        } else {
            clean_run = 0;
        }
        if (!(rho > 0.0)) return PREFIX_MODE_NONE;
        const double rule_rho = prefix_rho_by_rule(rule, clearance, r_hor, x0, n_spheres);
        // (the call that records has room itself: records are never traded for smaller ones that nothing asked for)
        const bool roomy = rule_rho >= PREFIX_OWNER_GROW_FACTOR * rho;
        const bool grow = roomy && roomy_run >= PREFIX_OWNER_GROW_CALLS;
        roomy_run = roomy ? roomy_run + 1 : 0;
        // (a scene without any clear ball has nothing to record: the held records wait for it to pass)
        const bool shrink = refused_run >= PREFIX_OWNER_SHRINK_CALLS && rule_rho > 0.0;
        if (grow || shrink) return rule;
        // (more than the kept rho by the margin of the replay test: never for the same ball again)
        const auto earned = [&](int by, int calls) {
            return clean_run >= calls && prefix_replay_ok(prefix_rho_by_rule(by, clearance, r_hor, x0, n_spheres), rho);
        };
        if (promote == PREFIX_MODE_RECORD_RIM) {
            // the ladder: the wide rung first, exactly as an owner that names the wide rule climbs it, the rim rung from there
            if (earned(PREFIX_MODE_RECORD_WIDE, PREFIX_OWNER_PROMOTE_CALLS)) return PREFIX_MODE_RECORD_WIDE;
            if (earned(PREFIX_MODE_RECORD_RIM, PREFIX_OWNER_PROMOTE_RIM_CALLS)) return PREFIX_MODE_RECORD_RIM;
        } else if (promote != PREFIX_MODE_NONE && earned(promote, PREFIX_OWNER_PROMOTE_CALLS)) {
            return promote;
        }
        return PREFIX_MODE_REPLAY;
    }
};

// What an owner asks for under the call's step budget (max_steps as the call resolves it, 0 never): a replay of rim records
// needs a budget above PREFIX_RIM_ATTEMPTS -- the C layer answers one at or below it with an error, since it can tell such
// records by their rho -- so the owner asks for nothing in that call and keeps its records for the calls after it.
inline int prefix_owner_fit_budget(int ask, double rho, double r_hor, const double x0[3], unsigned long long max_steps)
{
    if (ask == PREFIX_MODE_REPLAY && max_steps <= (unsigned long long)PREFIX_RIM_ATTEMPTS && prefix_rho_is_rim(rho, r_hor, x0))
        return PREFIX_MODE_NONE;
    return ask;
}

}  // namespace bhg

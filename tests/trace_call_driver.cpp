// trace_call_driver.cpp -- the two pieces of pure arithmetic of the C-API layer (csrc/trace_call.h: plain C++, no HIP) compiled
// with the HOST compiler under AddressSanitizer + UBSan by tests/test_trace_call_host.py:
//   the split   a trace call of n rays cut into launches of at most 64 (the library's limit is 2^26, which no test reaches): the
//               launches tile [0, n) in order, every per-ray pointer of a launch is its base plus the offset times its elements per
//               ray, null stays null, the layer stride and max_cross are kept, the start-up records are dropped; a call that fits
//               one launch is handed on untouched.  The arrays are real, at their true sizes, and every launch writes the last
//               element of each of its ranges: an offset that is too large is an ASan report.
//   the layout  the region lists of the six host-buffer entry points: regions 8-byte aligned, in order, disjoint, packed to
//               within the alignment, total() the end of the last.
// Prints one line of counts; exit code 0 = every check holds, otherwise the first that fails is named on stderr.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../blackhole_geodesic_calculator_amd/csrc/trace_call.h"

using bhg::TraceCall;
using bhg::TraceKind;

static int n_check = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        n_check++;                                                                               \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "check %d failed, line %d: %s\n", n_check, __LINE__, #cond);    \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static const size_t LIMIT = 64;
static const int32_t MAX_CROSS = 3;

// the arrays of one call of n rays, at their true element counts
struct Arrays {
    std::vector<double> x0, k0, end, end_dir, start_steps, cross, t_end, t_cross, bary;
    std::vector<uint8_t> flags, n_cross;
    std::vector<uint32_t> n_steps, n_accepted;
    std::vector<int8_t> object_id;
    std::vector<int32_t> tri_id;
    explicit Arrays(size_t n)
        : x0(n * 3), k0(n * 3), end(n * 6), end_dir(n * 3), start_steps(n), cross(MAX_CROSS * n * 6), t_end(n), t_cross(MAX_CROSS * n),
          bary(n * 2), flags(n), n_cross(n), n_steps(n), n_accepted(n), object_id(n), tri_id(n)
    {
    }
};

// one launch against the call it was cut from: pointer == base + off * elements per ray (null staying null), and a write to the
// last element of the launch's range (layered arrays: in the last layer)
#define CHECK_ARRAY(field, elems)                                                  \
    do {                                                                           \
        CHECK(part.field == (tc.field ? tc.field + off * (elems) : nullptr));      \
        if (part.field) part.field[part.n * (elems) - 1] = 1;                      \
    } while (0)

static int check_launch(const TraceCall &tc, const TraceCall &part, size_t off, bool split)
{
    CHECK(part.n == (tc.n - off < LIMIT ? tc.n - off : LIMIT));
    CHECK(part.d_x0 == (tc.d_x0 ? tc.d_x0 + off * 3 : nullptr) && part.d_k0 == (tc.d_k0 ? tc.d_k0 + off * 3 : nullptr));
    CHECK_ARRAY(d_end, 6);
    CHECK_ARRAY(d_end_dir, 3);
    CHECK_ARRAY(d_flags, 1);
    CHECK_ARRAY(d_n_steps, 1);
    CHECK_ARRAY(d_n_accepted, 1);
    CHECK_ARRAY(d_object_id, 1);
    CHECK_ARRAY(d_start_steps, 1);
    CHECK_ARRAY(n_cross, 1);
    CHECK_ARRAY(t_end, 1);
    CHECK_ARRAY(tri_id, 1);
    CHECK_ARRAY(bary, 2);
    CHECK(part.cross == (tc.cross ? tc.cross + off * 6 : nullptr) && part.t_cross == (tc.t_cross ? tc.t_cross + off : nullptr));
    if (part.cross) part.cross[((size_t)(part.max_cross - 1) * part.stride + part.n) * 6 - 1] = 1;
    if (part.t_cross) part.t_cross[(size_t)(part.max_cross - 1) * part.stride + part.n - 1] = 1;
    CHECK(part.stride == tc.stride && part.max_cross == tc.max_cross && part.kind == tc.kind);
    CHECK(part.spheres == tc.spheres && part.n_spheres == tc.n_spheres && part.x0_shared == tc.x0_shared);
    CHECK(part.start_mode == tc.start_mode && part.stream == tc.stream && part.mesh == tc.mesh && part.max_chord == tc.max_chord);
    CHECK(part.prefix == (split ? nullptr : tc.prefix));
    if (!split) CHECK(&part == &tc);      // a call that fits one launch: the record itself, untouched
    return 0;
}

static int check_split(TraceKind kind, bool all, size_t n, int *launches)
{
    Arrays A(n);
    static const double spheres[4] = {0, 0, 20, 2}, origin[3] = {0, 0, 30};
    static int stream_tag, mesh_tag;
    bhg_prefix prefix{};
    TraceCall tc;
    tc.kind = kind;
    tc.spheres = spheres;
    tc.n_spheres = 1;
    tc.x0_shared = origin;
    tc.d_k0 = A.k0.data();
    tc.n = n;
    tc.d_end = A.end.data();
    tc.start_mode = BHG_START_RECORD;
    tc.prefix = &prefix;
    tc.stream = &stream_tag;
    tc.max_cross = MAX_CROSS;
    tc.stride = n;
    tc.mesh = (const bhg_mesh *)&mesh_tag;
    tc.max_chord = 0.25;
    if (all) {
        tc.d_x0 = A.x0.data();
        tc.d_end_dir = A.end_dir.data();
        tc.d_flags = A.flags.data();
        tc.d_n_steps = A.n_steps.data();
        tc.d_n_accepted = A.n_accepted.data();
        tc.d_object_id = A.object_id.data();
        tc.d_start_steps = A.start_steps.data();
        tc.cross = A.cross.data();
        tc.n_cross = A.n_cross.data();
        tc.t_end = A.t_end.data();
        tc.t_cross = A.t_cross.data();
        tc.tri_id = A.tri_id.data();
        tc.bary = A.bary.data();
    }
    const TraceCall before = tc;
    size_t next = 0;
    int count = 0, bad = 0;
    const int rc = bhg::for_each_launch(tc, LIMIT, [&](const TraceCall &part) {
        if (!bad) bad = check_launch(tc, part, next, n > LIMIT);
        next += part.n;
        count++;
        return BHG_OK;
    });
    if (bad) return bad;
    CHECK(rc == BHG_OK && next == n && count == (int)((n + LIMIT - 1) / LIMIT));     // [0, n) tiled in order, no gap, no overlap
    CHECK(tc.n == before.n && tc.prefix == before.prefix && tc.d_end == before.d_end && tc.bary == before.bary);   // the call is not changed
    // the first failure ends the walk and is handed on
    int seen = 0;
    const int err = bhg::for_each_launch(tc, LIMIT, [&](const TraceCall &) { return ++seen == 2 ? BHG_E_INVALID : BHG_OK; });
    CHECK(n > LIMIT ? (err == BHG_E_INVALID && seen == 2) : (err == BHG_OK && seen == 1));
    *launches += count;
    return 0;
}

// one region list through bhg::StageLayout
static int check_layout(std::initializer_list<size_t> bytes, int *regions)
{
    bhg::StageLayout L;
    size_t prev_end = 0;
    for (size_t b : bytes) {
        if (b == 0) continue;      // (an array that is not there is not named)
        const size_t off = L.add(b);
        CHECK(off % 8 == 0);
        CHECK(off >= prev_end && off - prev_end < 8);     // in order, disjoint, packed to within the alignment
        prev_end = off + b;
        CHECK(L.total() == prev_end);                     // total() is the end of the last region
        (*regions)++;
    }
    return 0;
}

int main()
{
    int launches = 0, regions = 0, rc = 0;
    for (TraceKind kind : {TraceKind::PERSISTENT, TraceKind::CROSSINGS, TraceKind::TRAVEL_TIME, TraceKind::MESH})
        for (bool all : {true, false})
            for (size_t n : {(size_t)1, (size_t)64, (size_t)65, (size_t)128, (size_t)133})
                if ((rc = check_split(kind, all, n, &launches)) != 0) return rc;
    // the region lists of bhg_trace_crossings, bhg_travel_time, bhg_trace_mesh, bhg_redshift_motion_host, bhg_polarisation_host and
    // bhg_disk_thermal_host, with every array that may be absent there (opt = 1) and not (opt = 0): x0 of a shared origin, end of
    // the per-ray quantities, the object ids, n_cross of a travel time without records
    for (size_t n : {(size_t)1, (size_t)7, (size_t)63, (size_t)65})
        for (size_t K : {(size_t)0, (size_t)1, (size_t)3})
            for (size_t opt : {(size_t)0, (size_t)1}) {
                const size_t d = 8 * n, u = 4 * n, x = opt * 3 * d, e = opt * 6 * d;
                if ((rc = check_layout({3 * d, x, 6 * d, K * 6 * d, n, n, u, u}, &regions)) != 0) return rc;
                if ((rc = check_layout({3 * d, x, 6 * d, d, K * 6 * d, K * d, (K || opt) * n, n, u, u}, &regions)) != 0) return rc;
                if ((rc = check_layout({3 * d, x, 6 * d, u, 2 * d, n, u, u}, &regions)) != 0) return rc;
                if ((rc = check_layout({x, 3 * d, e, n, opt * n, d}, &regions)) != 0) return rc;
                if ((rc = check_layout({x, 3 * d, e, n, d, d, d}, &regions)) != 0) return rc;
                if ((rc = check_layout({x, 3 * d, e, n, d, 3 * d}, &regions)) != 0) return rc;
            }
    std::printf("launches %d regions %d checks %d\n", launches, regions, n_check);
    return 0;
}

// trace_call.h -- a trace call as plain data, and the two pieces of pure arithmetic of the C-API layer (bhgeo_capi.hip): how a
// call of any size is cut into launches, and where the arrays of a host-buffer call lie in their one device block.  Host only,
// no HIP: tests/trace_call_driver.cpp runs both under the host sanitizers.  (mesh_layout.h is its like for bhgeo_mesh.hip.)
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/bhgeo.h"

namespace bhg {

// which kernel traces the rays: the persistent one (work counters, start records), or a lane-per-ray kernel with outputs of its own
enum class TraceKind : int32_t { PERSISTENT, CROSSINGS, TRAVEL_TIME, MESH };

// Everything a trace call takes beside the context and the parameters.  A caller sets what it uses; the rest stays null.
struct TraceCall {
    TraceKind kind = TraceKind::PERSISTENT;
    const double *spheres = nullptr;     // host [n_spheres][4]
    int32_t n_spheres = 0;
    const double *x0_shared = nullptr, *d_x0 = nullptr, *d_k0 = nullptr;   // the origin: host [3], or device [n][3]; k0 [n][3]
    size_t n = 0;
    double *d_end = nullptr, *d_end_dir = nullptr;   // [n][6], or -- d_end null -- [n][3]: only the direction half is produced
    uint8_t *d_flags = nullptr;                      // [n] each, all optional
    uint32_t *d_n_steps = nullptr, *d_n_accepted = nullptr;
    int8_t *d_object_id = nullptr;
    double *d_start_steps = nullptr;     // [n], with start_mode
    int32_t start_mode = BHG_START_NONE;
    bhg_prefix *prefix = nullptr;        // the rays' start-up records (PERSISTENT, one launch)
    void *stream = nullptr;
    // CROSSINGS and TRAVEL_TIME: records [max_cross][stride][6] and their count per ray; the layer stride is the CALL's ray count
    double *cross = nullptr;
    uint8_t *n_cross = nullptr;
    int32_t max_cross = 0;
    size_t stride = 0;
    // TRAVEL_TIME: t_end [n], t_cross [max_cross][stride] beside cross (cross, n_cross and t_cross may be null with max_cross = 0)
    double *t_end = nullptr, *t_cross = nullptr;
    // MESH: the mesh, the chord limit and the two outputs tri_id [n], bary [n][2]
    const bhg_mesh *mesh = nullptr;
    double max_chord = 0.0;
    int32_t *tri_id = nullptr;
    double *bary = nullptr;
    // ... in the rigid placements of an instance set (with mesh: the set's mesh), and the third output inst_id [n]
    const bhg_mesh_instances *instances = nullptr;
    int32_t *inst_id = nullptr;

    // The call for rays [off, off + m): every per-ray array advanced by off times its elements per ray, null staying null; the
    // records' layers keep their stride (these rays sit at offset off inside every layer).  The start-up records are dropped:
    // their planes are strided by ONE launch's ray count.
    TraceCall slice(size_t off, size_t m) const
    {
        TraceCall t = *this;
        t.n = m;
        t.prefix = nullptr;
        skip(off * 3, t.d_x0, t.d_k0, t.d_end_dir);
        skip(off * 6, t.d_end, t.cross);
        skip(off * 2, t.bary);
        skip(off, t.d_flags, t.d_n_steps, t.d_n_accepted, t.d_object_id, t.d_start_steps, t.n_cross, t.t_end, t.t_cross, t.tri_id,
             t.inst_id);
        return t;
    }
    template <class... T>
    static void skip(size_t k, T *&...p) { ((p = p ? p + k : nullptr), ...); }
};

// The rays [0, tc.n) in launches of at most max_per_launch, in order: launch(part) for each, the first failure ends the walk.
// A call that fits one launch is handed on as it is, start-up records included.
template <class Launch>
int for_each_launch(const TraceCall &tc, size_t max_per_launch, Launch &&launch)
{
    if (tc.n <= max_per_launch) return launch(tc);
    int rc = BHG_OK;
    for (size_t off = 0; off < tc.n && rc == BHG_OK; off += max_per_launch)
        rc = launch(tc.slice(off, tc.n - off < max_per_launch ? tc.n - off : max_per_launch));
    return rc;
}

// Where the arrays of a host-buffer call lie in their one device block: regions in the order they are added, each at a multiple
// of 8 bytes; total() is the block's size.
struct StageLayout {
    size_t end = 0;
    size_t add(size_t bytes)
    {
        const size_t off = (end + 7) & ~size_t(7);
        end = off + bytes;
        return off;
    }
    size_t total() const { return end; }
};

}  // namespace bhg

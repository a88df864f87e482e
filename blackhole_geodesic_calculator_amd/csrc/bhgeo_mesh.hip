// bhgeo_mesh.hip -- the life cycle of the library-side mesh and instance set (bhg_mesh_*, bhg_mesh_instances_* in include/bhgeo.h;
// DESIGN.md sections 19, 21-24): create on the host or on the device, refit, rebuild in place, destroy, and what they report.  The
// calls that trace or shade with a mesh are bhgeo_capi.hip's; mesh_object.h is what the two units share.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <utility>
#include <vector>

#include "bhgeo_internal.h"
#include "instance_tree.h"
#include "mesh_build.h"
#include "mesh_bvh.h"
#include "mesh_layout.h"
#include "mesh_object.h"
#include "mesh_refit.h"

namespace {

// the meshes that exist, by address and serial number (an address may come back after a destroy; a serial never does)
std::mutex live_meshes_lock;
std::unordered_map<const bhg_mesh *, uint64_t> live_meshes;
uint64_t live_meshes_next = 1;

void enter_live(bhg_mesh *m)
{
    std::lock_guard<std::mutex> lock(live_meshes_lock);
    m->serial = live_meshes_next++;
    live_meshes[m] = m->serial;
}

bool mesh_is_live(const bhg_mesh *m, uint64_t serial)
{
    std::lock_guard<std::mutex> lock(live_meshes_lock);
    auto it = live_meshes.find(m);
    return it != live_meshes.end() && it->second == serial;
}

// a mesh that is in live_meshes no more, or not yet: its device memory and the object
void mesh_discard(bhg_mesh *m)
{
    {
        DeviceGuard g(m->device);
        if (m->d) (void)hipFree(m->d);
        if (m->d_refit) (void)hipFree(m->d_refit);
        if (m->d_build) (void)hipFree(m->d_build);
    }
    delete m;
}

struct MeshOwner {   // of a mesh under construction
    bhg_mesh *m;
    ~MeshOwner() { if (m) mesh_discard(m); }
};

// the counts a mesh's device memory is laid out for: its own, or -- by capacity -- those of the largest tree and vertex array a
// rebuild may bring (2 cap - 1 nodes at leaf_size 1; cap entries for the inner nodes, one more than such a tree has)
struct MeshCounts {
    size_t nodes, tris, inner, vertices;
};

MeshCounts laid_out_for(const bhg_mesh *m, bool by_capacity)
{
    if (by_capacity) return {2 * m->cap_triangles - 1, m->cap_triangles, m->cap_triangles, m->cap_vertices};
    return {(size_t)m->n_nodes, (size_t)m->view.n_tris, (size_t)m->n_inner, (size_t)m->n_vertices};
}

bhg::MeshImage image_for(const bhg_mesh *m, bool by_capacity)
{
    const MeshCounts n = laid_out_for(m, by_capacity);
    return bhg::mesh_image(n.nodes, n.tris, n.inner, m->has_normals);
}

void point_into_image(bhg_mesh *m, char *d, const bhg::MeshImage &g)
{
    m->d = d;
    bhg::MeshView &v = m->view;
    v.node_box = (const double *)(d + g.off[bhg::MESH_BOX]);
    v.tri = (const double *)(d + g.off[bhg::MESH_TRI]);
    v.tri_normals = m->has_normals ? (const double *)(d + g.off[bhg::MESH_NORMALS]) : nullptr;
    v.node_skip = (const int32_t *)(d + g.off[bhg::MESH_SKIP]);
    v.node_first = (const int32_t *)(d + g.off[bhg::MESH_FIRST]);
    v.node_count = (const int32_t *)(d + g.off[bhg::MESH_COUNT]);
    v.tri_order = (const int32_t *)(d + g.off[bhg::MESH_ORDER]);
    v.tri_slot = (const int32_t *)(d + g.off[bhg::MESH_SLOT]);
    m->slot_vert = (const int32_t *)(d + g.off[bhg::MESH_SLOT_VERT]);
    m->level_nodes = (const int32_t *)(d + g.off[bhg::MESH_LEVEL_NODES]);
}

// What a mesh knows of its extent, from its root box, the largest |v|^2 over its vertices and its area sum: every point of the mesh
// lies inside the root box and no farther from the origin than the farthest vertex.  (The square root is monotone, also once
// rounded: the root of the largest |v|^2 is the largest |v|, bit for bit.)
void settle(bhg_mesh *m, const double box[6], double far2, double area)
{
    std::memcpy(m->box, box, sizeof(m->box));
    double d2 = 0.0;
    for (int q = 0; q < 3; q++) {
        const double gap = std::max(std::max(m->box[q], -m->box[3 + q]), 0.0);
        d2 += gap * gap;
    }
    m->d_min = std::sqrt(d2) * (1.0 - 1e-14);
    m->d_max = std::sqrt(far2) * (1.0 + 1e-14);
    m->area_now = area;
}

void settle(bhg_mesh *m, const bhg::MeshRefitSummary &sum)
{
    double far2;
    std::memcpy(&far2, &sum.d2_max, sizeof(far2));
    settle(m, sum.box, far2, sum.area);
}

int normals_match(const char *who, const bhg_mesh *m, const void *vertex_normals)
{
    if (vertex_normals && !m->has_normals)
        return fail(BHG_E_INVALID, std::string(who) + ": vertex_normals given to a mesh that was created without them");
    if (!vertex_normals && m->has_normals)
        return fail(BHG_E_INVALID, std::string(who) + ": vertex_normals is NULL for a mesh that was created with them");
    return BHG_OK;
}

// a tree of either host builder, copied out to the caller's arrays
int bvh_host(void (*build)(const double *, const int32_t *, size_t, int32_t, bhg::HostBvh &), const double *vertices, size_t n_vertices,
             const int32_t *triangles, size_t n_triangles, int32_t leaf_size, double *node_box, int32_t *node_skip, int32_t *node_first,
             int32_t *node_count, int32_t *tri_order, size_t cap, size_t *n_nodes)
{
    if (const char *why = bhg::mesh_refusal(vertices, n_vertices, triangles, n_triangles, leaf_size)) return fail(BHG_E_INVALID, why);
    if (!n_nodes) return fail(BHG_E_INVALID, "n_nodes is NULL");
    bhg::HostBvh t;
    build(vertices, triangles, n_triangles, leaf_size, t);
    const size_t nn = t.node_skip.size();
    *n_nodes = nn;
    if (nn > cap) return fail(BHG_E_INVALID, "the tree has more nodes than cap (2 * n_triangles - 1 always suffices)");
    if (!node_box || !node_skip || !node_first || !node_count || !tri_order) return fail(BHG_E_INVALID, "an output array is NULL");
    std::memcpy(node_box, t.node_box.data(), nn * 6 * sizeof(double));
    std::memcpy(node_skip, t.node_skip.data(), nn * sizeof(int32_t));
    std::memcpy(node_first, t.node_first.data(), nn * sizeof(int32_t));
    std::memcpy(node_count, t.node_count.data(), nn * sizeof(int32_t));
    std::memcpy(tri_order, t.tri_order.data(), n_triangles * sizeof(int32_t));
    return BHG_OK;
}

// what the two trace checks share; what: the mesh or the instance set, null_msg: what its absence is called
int trace_check(const bhg_params *p, const void *what, const char *null_msg, double max_chord, const int32_t *tri_id, const double *bary)
{
    BHG_TRY(bhg::params_check(p));
    if (p->method != BHG_METHOD_DP54) return fail(BHG_E_INVALID, "the mesh trace is DP5(4) only: method must be BHG_METHOD_DP54");
    if (p->time_like) return fail(BHG_E_INVALID, "the mesh trace covers null rays only: time_like must be 0");
    if (!what) return fail(BHG_E_INVALID, null_msg);
    if (!std::isfinite(max_chord) || !(max_chord > 0.0)) return fail(BHG_E_INVALID, "max_chord must be finite and > 0");
    if (!tri_id || !bary) return fail(BHG_E_INVALID, "tri_id / bary is NULL");
    return BHG_OK;
}

// what both refit calls refuse before the device is touched
int refit_check(const bhg_context *c, const bhg_mesh *m, const double *vertices, const double *vertex_normals)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (!vertices) return fail(BHG_E_INVALID, "mesh refit: vertices is NULL");
    BHG_TRY(normals_match("mesh refit", m, vertex_normals));
    return bhg::mesh_on_device_of(c, m);
}

// the refit's own device memory, allocated by the first refit and kept (the last two arrays stage the host form's)
struct RefitScratch {
    bhg::MeshRefitSummary *summary;
    double *area, *vertices, *normals;
};

int refit_scratch(bhg_mesh *m, RefitScratch &r)
{
    const MeshCounts n = laid_out_for(m, m->by_capacity);
    const bhg::RefitLayout g = bhg::refit_layout(sizeof(bhg::MeshRefitSummary), n.nodes, n.vertices, m->has_normals);
    if (!m->d_refit) {
        HIP_TRY(hipMalloc((void **)&m->d_refit, g.total));
        m->allocations++;
    }
    char *const d = m->d_refit;
    r = {(bhg::MeshRefitSummary *)(d + g.summary), (double *)(d + g.area), (double *)(d + g.vertices),
         m->has_normals ? (double *)(d + g.normals) : nullptr};
    return BHG_OK;
}

// a refit of the mesh as it stands (its counts, its topology) from the device arrays d_v, d_n
bhg::MeshRefitArgs refit_args(const bhg_mesh *m, const RefitScratch &r, const double *d_v, const double *d_n)
{
    bhg::MeshRefitArgs a = {.vertices = d_v, .normals = d_n, .n_vertices = m->n_vertices, .n_tris = m->view.n_tris,
                            .n_nodes = m->view.n_nodes, .n_inner = m->n_inner, .slot_vert = m->slot_vert, .node_skip = m->view.node_skip,
                            .node_first = m->view.node_first, .node_count = m->view.node_count, .level_nodes = m->level_nodes, .level_off = {},
                            .node_box = const_cast<double *>(m->view.node_box), .tri = const_cast<double *>(m->view.tri),
                            .tri_normals = const_cast<double *>(m->view.tri_normals), .area = r.area, .summary = r.summary};
    std::memcpy(a.level_off, m->level_off.data(), sizeof(a.level_off));
    return a;
}

// d_v, d_n: device arrays.  scan: they have not been looked at yet (the device form).  The device is c's and current.
int refit_run(bhg_context *c, bhg_mesh *m, const RefitScratch &r, const double *d_v, const double *d_n, bool scan, hipStream_t s)
{
    const bhg::MeshRefitArgs a = refit_args(m, r, d_v, d_n);
    bhg::MeshRefitSummary sum;
    // nothing of the mesh is written before everything queued on the context's stream and on s is done
    if (bhg::context_stream(c) != s) HIP_TRY(hipStreamSynchronize(bhg::context_stream(c)));
    HIP_TRY(hipMemsetAsync(r.summary, 0, sizeof(sum), s));
    if (scan) {
        HIP_TRY(bhg::launch_mesh_refit_scan(a, s));
        HIP_TRY(hipMemcpyAsync(&sum, r.summary, sizeof(sum), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (scan && (sum.nonfinite & 1u)) return fail(BHG_E_INVALID, "mesh: every vertex must be finite");
    if (scan && (sum.nonfinite & 2u)) return fail(BHG_E_INVALID, "mesh: every vertex normal must be finite");
    HIP_TRY(bhg::launch_mesh_refit(a, s));
    HIP_TRY(hipMemcpyAsync(&sum, r.summary, sizeof(sum), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    settle(m, sum);
    m->generation++;
    return BHG_OK;
}

// the build's own storage, allocated by the first build and kept
struct BuildStorage {
    bhg::MeshBuildRecord *record;
    unsigned long long *keys_in, *keys_out;
    int32_t *vals_in, *triangles;
    void *sort_temp;
};

int build_storage(bhg_mesh *m, BuildStorage &b)
{
    // (the sort's storage is asked for once, for the capacity)
    if (!m->d_build) HIP_TRY(bhg::mesh_build_sort_bytes(m->cap_triangles, &m->sort_bytes));
    const bhg::BuildLayout g = bhg::build_layout(sizeof(bhg::MeshBuildRecord), m->cap_triangles, m->sort_bytes);
    if (!m->d_build) {
        HIP_TRY(hipMalloc((void **)&m->d_build, g.total));
        m->allocations++;
    }
    char *const d = m->d_build;
    b = {(bhg::MeshBuildRecord *)(d + g.record), (unsigned long long *)(d + g.keys_in), (unsigned long long *)(d + g.keys_out),
         (int32_t *)(d + g.vals_in), (int32_t *)(d + g.triangles), d + g.sort};
    return BHG_OK;
}

// A mesh of bhg_mesh_create, laid out for its own tree, moves into an image laid out by capacity before its first rebuild: the
// arrays are copied as they are, so the mesh stays what it was should the rebuild then be refused.  The device is the mesh's.
int reserve_by_capacity(bhg_mesh *m)
{
    if (m->by_capacity) return BHG_OK;
    const bhg::MeshImage from = image_for(m, false), to = image_for(m, true);
    char *d = nullptr;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMalloc((void **)&d, to.total));
    hipError_t e = hipSuccess;
    for (int r = 0; r < bhg::MESH_REGIONS && e == hipSuccess; r++)
        if (from.bytes[r]) e = hipMemcpy(d + to.off[r], m->d + from.off[r], from.bytes[r], hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail_hip(e, "mesh rebuild: the image by capacity");
    }
    (void)hipFree(m->d);
    point_into_image(m, d, to);
    m->allocations++;
    // (the refit's scratch is laid out anew with the image: it holds nothing between calls)
    if (m->d_refit) {
        (void)hipFree(m->d_refit);
        m->d_refit = nullptr;
    }
    m->by_capacity = true;
    m->topo_triangles = 0;
    return BHG_OK;
}

// what the build calls refuse of their counts and arrays before the device is touched
int build_counts_check(const void *vertices, size_t nv, const void *triangles, size_t nt)
{
    if (!vertices || !triangles) return fail(BHG_E_INVALID, "mesh: vertices / triangles is NULL");
    if (nv == 0 || nt == 0) return fail(BHG_E_INVALID, "mesh: n_vertices and n_triangles must be > 0");
    if (nv > 0x7FFFFFFFull || nt > 0x7FFFFFFFull) return fail(BHG_E_INVALID, "mesh: n_vertices and n_triangles must be <= 2^31 - 1");
    return BHG_OK;
}

int build_leaf_check(int32_t leaf_size)
{
    if (leaf_size < 1 || leaf_size > bhg::MORTON_LEAF_MAX) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "mesh device build: leaf_size %d must be in [1, %d] (larger leaves: bhg_mesh_create)", (int)leaf_size,
                      (int)bhg::MORTON_LEAF_MAX);
        return fail(BHG_E_INVALID, msg);
    }
    return BHG_OK;
}

int rebuild_check(const bhg_context *c, const bhg_mesh *m, const void *vertices, size_t nv, const void *triangles, size_t nt,
                  const void *normals)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    BHG_TRY(build_counts_check(vertices, nv, triangles, nt));
    BHG_TRY(build_leaf_check(m->leaf_size));
    if (nv > m->cap_vertices || nt > m->cap_triangles) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "mesh rebuild: n_vertices %zu / n_triangles %zu exceed the mesh's capacity %zu / %zu", nv, nt,
                      m->cap_vertices, m->cap_triangles);
        return fail(BHG_E_INVALID, msg);
    }
    BHG_TRY(normals_match("mesh rebuild", m, normals));
    return bhg::mesh_on_device_of(c, m);
}

// The build proper.  d_v, d_f, d_n: device arrays within the mesh's capacity, not looked at yet.  The mesh is laid out by capacity
// and owns its build and refit storage (b, r); the device is c's and current.  Nothing of the mesh is written before the scan of
// all three arrays has been read back and found clean, and no kernel follows a triangle index before that either.
int build_run(bhg_context *c, bhg_mesh *m, const BuildStorage &b, const RefitScratch &r, const double *d_v, size_t nv, const int32_t *d_f,
              size_t nt, const double *d_n, hipStream_t s)
{
    bhg::MeshBuildArgs ba = {.vertices = d_v, .triangles = d_f, .n_vertices = (int32_t)nv, .n_tris = (int32_t)nt, .record = b.record};
    // (the scan of the new arrays alone: the mesh still has its old counts)
    const bhg::MeshRefitArgs scan = {.vertices = d_v, .normals = d_n, .n_vertices = (int32_t)nv, .summary = r.summary};
    bhg::MeshRefitSummary sum;
    bhg::MeshBuildRecord rec;
    if (bhg::context_stream(c) != s) HIP_TRY(hipStreamSynchronize(bhg::context_stream(c)));
    HIP_TRY(hipMemsetAsync(r.summary, 0, sizeof(sum), s));
    HIP_TRY(hipMemsetAsync(b.record, 0, sizeof(rec), s));
    HIP_TRY(bhg::launch_mesh_build_scan(ba, s));
    HIP_TRY(bhg::launch_mesh_refit_scan(scan, s));
    HIP_TRY(hipMemcpyAsync(&rec, b.record, sizeof(rec), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&sum, r.summary, sizeof(sum), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (sum.nonfinite & 1u) return fail(BHG_E_INVALID, "mesh: every vertex must be finite");
    if (rec.bad_index) return fail(BHG_E_INVALID, "mesh: a triangle index lies outside [0, n_vertices)");
    if (sum.nonfinite & 2u) return fail(BHG_E_INVALID, "mesh: every vertex normal must be finite");
    // the topology: a function of (nt, leaf_size), written by the host and kept while both stand
    if (m->topo_triangles != nt) {
        std::vector<int32_t> skip, first, count, level_nodes, level_off;
        int32_t depth = 0;
        bhg::morton_topology(nt, m->leaf_size, skip, first, count, depth);
        const size_t nn = skip.size();
        if (!bhg::inner_levels(skip.data(), count.data(), nn, level_nodes, level_off))
            return fail(BHG_E_INVALID, "mesh device build: the tree is deeper than BVH_MAX_DEPTH");
        m->topo_triangles = 0;      // (until all four arrays are up)
        const auto up = [&](const int32_t *dst, const std::vector<int32_t> &src) {
            return hipMemcpyAsync(const_cast<int32_t *>(dst), src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
        };
        HIP_TRY(up(m->view.node_skip, skip));
        HIP_TRY(up(m->view.node_first, first));
        HIP_TRY(up(m->view.node_count, count));
        if (!level_nodes.empty()) HIP_TRY(up(m->level_nodes, level_nodes));
        // (the vectors go out of scope below: the copies from pageable memory have been staged when the calls return, and the
        // stream is waited for before this function does)
        HIP_TRY(hipStreamSynchronize(s));
        m->n_nodes = (int64_t)nn;
        m->view.n_nodes = (int32_t)nn;
        m->depth = depth;
        m->n_inner = (int32_t)level_nodes.size();
        m->level_off = level_off;
        m->topo_triangles = nt;
    }
    m->view.n_tris = (int32_t)nt;
    m->n_vertices = (int32_t)nv;
    ba.n_nodes = m->view.n_nodes;
    ba.node_first = m->view.node_first;
    ba.node_count = m->view.node_count;
    ba.keys_in = b.keys_in;
    ba.keys_out = b.keys_out;
    ba.vals_in = b.vals_in;
    ba.sort_temp = b.sort_temp;
    ba.sort_temp_bytes = m->sort_bytes;
    ba.tri_order = const_cast<int32_t *>(m->view.tri_order);
    ba.tri_slot = const_cast<int32_t *>(m->view.tri_slot);
    ba.slot_vert = const_cast<int32_t *>(m->slot_vert);
    // (the scan's flags are zero; the refit max-es d2_max into the same record)
    HIP_TRY(bhg::launch_mesh_build(ba, s));
    HIP_TRY(bhg::launch_mesh_refit(refit_args(m, r, d_v, d_n), s));
    HIP_TRY(hipMemcpyAsync(&sum, r.summary, sizeof(sum), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    settle(m, sum);
    m->area_build = m->area_now;
    m->built_on_device = true;
    return BHG_OK;
}

// a rebuild of a live mesh: the storage, the move into an image by capacity, the build, the counters
int rebuild_run(bhg_context *c, bhg_mesh *m, const double *v, size_t nv, const int32_t *f, size_t nt, const double *n, bool host_arrays,
                hipStream_t s)
{
    BHG_TRY(reserve_by_capacity(m));
    BuildStorage b;
    RefitScratch r;
    BHG_TRY(build_storage(m, b));
    BHG_TRY(refit_scratch(m, r));
    if (host_arrays) {
        // (the staging arrays are the mesh's own: a rebuild is blocking, so no earlier one still reads them)
        HIP_TRY(hipMemcpyAsync(r.vertices, v, nv * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b.triangles, f, nt * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (n) HIP_TRY(hipMemcpyAsync(r.normals, n, nv * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        v = r.vertices;
        f = b.triangles;
        if (n) n = r.normals;
    }
    BHG_TRY(build_run(c, m, b, r, v, nv, f, nt, n, s));
    m->generation++;
    m->builds++;
    return BHG_OK;
}

// the world box of a local box under x -> R x + t: centre R c + t, half extents |R| h, widened outward by the builder's ulps of
// the largest magnitude involved -- the box, the translation and the local box, whose roundings in p' = R^T (p - t) it has to cover
void instance_world_box(const double lb[6], const double T[12], double wb[6])
{
    const double c[3] = {0.5 * (lb[0] + lb[3]), 0.5 * (lb[1] + lb[4]), 0.5 * (lb[2] + lb[5])};
    const double h[3] = {0.5 * (lb[3] - lb[0]), 0.5 * (lb[4] - lb[1]), 0.5 * (lb[5] - lb[2])};
    double mag = 0.0;
    for (int q = 0; q < 3; q++) {
        const double *R = T + 3 * q;
        const double wc = R[0] * c[0] + R[1] * c[1] + R[2] * c[2] + T[9 + q];
        const double wh = std::fabs(R[0]) * h[0] + std::fabs(R[1]) * h[1] + std::fabs(R[2]) * h[2];
        wb[q] = wc - wh;
        wb[3 + q] = wc + wh;
        mag = std::max(mag, std::fabs(wc) + wh);
        mag = std::max(mag, std::fabs(T[9 + q]));
        mag = std::max(mag, std::max(std::fabs(lb[q]), std::fabs(lb[3 + q])));
    }
    const double w = bhg::BVH_BOX_ULPS * 2.220446049250313e-16 * std::max(mag, 2.2250738585072014e-308);
    for (int q = 0; q < 3; q++) {
        wb[q] -= w;
        wb[3 + q] += w;
    }
}

// the records of n checked transforms against the mesh's root box, and the set's union box and range of distances
void instance_records(const bhg_mesh *mesh, int32_t n, const double *T, double *rec, double box[6], double &d_min, double &d_max)
{
    double t_max = 0.0, near2 = INFINITY;
    for (int32_t j = 0; j < n; j++) {
        double *r = rec + (size_t)j * bhg::BHG_MESH_INSTANCE_DOUBLES_;
        std::memcpy(r, T + (size_t)j * 12, 12 * sizeof(double));
        instance_world_box(mesh->box, r, r + 12);
        double d2 = 0.0;
        for (int q = 0; q < 3; q++) {
            box[q] = j ? std::min(box[q], r[12 + q]) : r[12 + q];
            box[3 + q] = j ? std::max(box[3 + q], r[15 + q]) : r[15 + q];
            const double gap = std::max(std::max(r[12 + q], -r[15 + q]), 0.0);
            d2 += gap * gap;
        }
        near2 = std::min(near2, d2);
        t_max = std::max(t_max, std::sqrt(r[9] * r[9] + r[10] * r[10] + r[11] * r[11]));
    }
    // a point of instance j lies no farther from the origin than |t_j| + the mesh's farthest vertex, and inside its world box
    d_min = std::sqrt(near2) * (1.0 - 1e-14);
    d_max = (t_max + mesh->d_max) * (1.0 + 1e-14);
}

}  // namespace

namespace bhg {

bool mesh_culls_on()
{
    const char *cull = std::getenv("BHGEO_MESH_CULL");
    return !(cull && cull[0] == '0' && cull[1] == 0);
}

hipError_t instances_before_read(const bhg_mesh_instances *in, hipStream_t s)
{
    if (in->last >= 0)
        if (hipError_t e = hipStreamWaitEvent(s, in->ev_copy[in->last], 0)) return e;
    if (in->was_read && in->read_stream != s)
        if (hipError_t e = hipStreamWaitEvent(s, in->ev_read, 0)) return e;
    return hipSuccess;
}

hipError_t instances_after_read(const bhg_mesh_instances *in, hipStream_t s)
{
    in->read_stream = s;
    in->was_read = true;
    return hipEventRecord(in->ev_read, s);
}

int instances_usable(const bhg_context *c, const bhg_mesh_instances *inst, bool reading)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (inst->ctx != c) return fail(BHG_E_INVALID, "mesh instances: the instance set belongs to another context");
    if (!mesh_is_live(inst->mesh, inst->mesh_serial)) return fail(BHG_E_INVALID, "mesh instances: the set's mesh has been destroyed");
    if (reading && inst->mesh_generation != inst->mesh->generation)
        return fail(BHG_E_INVALID, "mesh instances: the set's mesh has been refitted, call bhg_mesh_instances_set after bhg_mesh_refit");
    return BHG_OK;
}

int mesh_on_device_of(const bhg_context *c, const bhg_mesh *m)
{
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    if (m->device != context_device(c)) return fail(BHG_E_INVALID, "the mesh lives on another device than the context");
    return BHG_OK;
}

int mesh_trace_check(const bhg_params *p, const bhg_mesh *mesh, double max_chord, const int32_t *tri_id, const double *bary)
{
    return trace_check(p, mesh, "mesh is NULL", max_chord, tri_id, bary);
}

int instances_trace_check(const bhg_params *p, const bhg_mesh_instances *inst, double max_chord, const int32_t *tri_id,
                          const int32_t *inst_id, const double *bary)
{
    BHG_TRY(trace_check(p, inst, "mesh instances: inst is NULL", max_chord, tri_id, bary));
    if (!inst_id) return fail(BHG_E_INVALID, "inst_id is NULL");
    return BHG_OK;
}

int mesh_finite_check(const double *vertices, const double *vertex_normals, size_t n3)
{
    if (vertices)
        for (size_t i = 0; i < n3; i++)
            if (!std::isfinite(vertices[i])) return fail(BHG_E_INVALID, "mesh: every vertex must be finite");
    if (vertex_normals)
        for (size_t i = 0; i < n3; i++)
            if (!std::isfinite(vertex_normals[i])) return fail(BHG_E_INVALID, "mesh: every vertex normal must be finite");
    return BHG_OK;
}

// bhg_mesh_create_device, and the same from HOST arrays (bhgeo_frame.hip: a frame holds its mesh on the host), which are uploaded
// into the new mesh's staging arrays first
int mesh_create_built_on_device(bhg_context *c, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles,
                                size_t n_triangles, const double *d_vertex_normals, int32_t leaf_size, size_t cap_vertices,
                                size_t cap_triangles, bool host_arrays, hipStream_t stream, bhg_mesh **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    BHG_TRY(build_counts_check(d_vertices, n_vertices, d_triangles, n_triangles));
    BHG_TRY(build_leaf_check(leaf_size));
    if (cap_vertices == 0) cap_vertices = n_vertices;
    if (cap_triangles == 0) cap_triangles = n_triangles;
    if (cap_vertices < n_vertices || cap_triangles < n_triangles)
        return fail(BHG_E_INVALID, "mesh device build: cap_vertices / cap_triangles must be 0 or at least the counts");
    if (cap_vertices > 0x7FFFFFFFull || cap_triangles > 0x7FFFFFFFull)
        return fail(BHG_E_INVALID, "mesh device build: cap_vertices and cap_triangles must be <= 2^31 - 1");
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    ENTER_DEVICE(context_device(c));
    bhg_mesh *m = new (std::nothrow) bhg_mesh;
    if (!m) return fail(BHG_E_NOMEM, "out of host memory");
    m->device = context_device(c);
    m->has_normals = d_vertex_normals != nullptr;
    m->leaf_size = leaf_size;
    m->cap_vertices = cap_vertices;
    m->cap_triangles = cap_triangles;
    m->by_capacity = true;
    // everything the mesh will ever hold on the device, now: the image, the build's storage, the refit's
    const MeshImage g = image_for(m, true);
    MeshOwner own{m};     // (refused or failed: nothing stays allocated)
    char *d = nullptr;
    if (hipError_t e = hipMalloc((void **)&d, g.total)) return fail_hip(e, "bhg_mesh_create_device: device image");
    point_into_image(m, d, g);
    m->allocations++;
    BuildStorage b;
    RefitScratch r;
    BHG_TRY(build_storage(m, b));
    BHG_TRY(refit_scratch(m, r));
    if (host_arrays) {
        const auto up = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream); };
        hipError_t e = up(r.vertices, d_vertices, n_vertices * 3 * sizeof(double));
        if (e == hipSuccess) e = up(b.triangles, d_triangles, n_triangles * 3 * sizeof(int32_t));
        if (e == hipSuccess && d_vertex_normals) e = up(r.normals, d_vertex_normals, n_vertices * 3 * sizeof(double));
        if (e != hipSuccess) return fail_hip(e, "bhg_mesh_create_device: upload");
        d_vertices = r.vertices;
        d_triangles = b.triangles;
        if (d_vertex_normals) d_vertex_normals = r.normals;
    }
    BHG_TRY(build_run(c, m, b, r, d_vertices, n_vertices, d_triangles, n_triangles, d_vertex_normals, stream));
    own.m = nullptr;
    m->builds = 1;
    enter_live(m);
    *out = m;
    return BHG_OK;
}

// n > 0 transforms: all there, finite, rigid and no reflections
static int rigid_check(int32_t n, const double *T)
{
    if (!T) return fail(BHG_E_INVALID, "mesh instances: transforms is NULL");
    for (int32_t j = 0; j < n; j++) {
        const double *R = T + (size_t)j * 12;
        for (int q = 0; q < 12; q++)
            if (!std::isfinite(R[q])) return fail(BHG_E_INVALID, "mesh instances: every entry of transforms must be finite");
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double g = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b];
                if (!(std::fabs(g - (a == b ? 1.0 : 0.0)) <= 1e-9))
                    return fail(BHG_E_INVALID, "mesh instances: transforms must be rigid, R^T R within 1e-9 of the identity");
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det > 0.0)) return fail(BHG_E_INVALID, "mesh instances: transforms must be rotations, det R > 0");
    }
    return BHG_OK;
}

int mesh_instance_transforms_check(int32_t n, const double *T)
{
    if (n < 1 || n > BHG_MESH_INSTANCES_MAX) return fail(BHG_E_INVALID, "mesh instances: n must be in [1, BHG_MESH_INSTANCES_MAX]");
    return rigid_check(n, T);
}

int mesh_instance_tree_check(int32_t n, const double *T, int32_t leaf_size)
{
    if (n < 1 || n > BHG_MESH_INSTANCE_TREE_MAX)
        return fail(BHG_E_INVALID, "mesh instances: n must be in [1, BHG_MESH_INSTANCE_TREE_MAX] for a set under a tree");
    if (leaf_size < 1 || leaf_size > INSTANCE_TREE_LEAF_MAX)
        return fail(BHG_E_INVALID, "mesh instances: the tree's leaf_size must be in [1, 8]");
    return rigid_check(n, T);
}

bool instance_tree_on()
{
    const char *tree = std::getenv("BHGEO_INSTANCE_TREE");
    return !(tree && tree[0] == '0' && tree[1] == 0);
}

}  // namespace bhg

extern "C" {

int bhg_mesh_bvh_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles, int32_t leaf_size,
                      double *node_box, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order, size_t cap,
                      size_t *n_nodes)
{
    return bvh_host(bhg::build_bvh, vertices, n_vertices, triangles, n_triangles, leaf_size, node_box, node_skip, node_first, node_count,
                    tri_order, cap, n_nodes);
}

int bhg_mesh_bvh_morton_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles, int32_t leaf_size,
                             double *node_box, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order,
                             size_t cap, size_t *n_nodes)
{
    return bvh_host(bhg::build_bvh_morton, vertices, n_vertices, triangles, n_triangles, leaf_size, node_box, node_skip, node_first,
                    node_count, tri_order, cap, n_nodes);
}

int bhg_mesh_create(bhg_context *c, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                    const double *vertex_normals, int32_t leaf_size, bhg_mesh **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (const char *why = bhg::mesh_refusal(vertices, n_vertices, triangles, n_triangles, leaf_size)) return fail(BHG_E_INVALID, why);
    BHG_TRY(bhg::mesh_finite_check(nullptr, vertex_normals, n_vertices * 3));     // (the vertices: mesh_refusal)
    if (!c) return fail(BHG_E_INVALID, "ctx is NULL");
    ENTER_DEVICE(bhg::context_device(c));
    bhg::HostBvh t;
    bhg::build_bvh(vertices, triangles, n_triangles, leaf_size, t);
    const size_t nn = t.node_skip.size(), nt = n_triangles;
    // the refit's schedule: the inner nodes by level
    std::vector<int32_t> level_nodes, level_off;
    if (!bhg::inner_levels(t.node_skip.data(), t.node_count.data(), nn, level_nodes, level_off))
        return fail(BHG_E_INVALID, "bhg_mesh_create: the tree is deeper than BVH_MAX_DEPTH");
    // the device image, laid out for this tree and put together on the host
    const bhg::MeshImage g = bhg::mesh_image(nn, nt, level_nodes.size(), vertex_normals != nullptr);
    std::vector<char> img(g.total, 0);
    double *tri = (double *)(img.data() + g.off[bhg::MESH_TRI]), *nrm = (double *)(img.data() + g.off[bhg::MESH_NORMALS]);
    int32_t *slot_of = (int32_t *)(img.data() + g.off[bhg::MESH_SLOT]), *slot_vert = (int32_t *)(img.data() + g.off[bhg::MESH_SLOT_VERT]);
    double far2 = 0.0;
    for (size_t k = 0; k < nt; k++) {
        const int32_t f = t.tri_order[k];
        slot_of[f] = (int32_t)k;
        for (int j = 0; j < 3; j++) slot_vert[k * 3 + j] = triangles[(size_t)f * 3 + j];
        const double *v0 = vertices + (size_t)triangles[(size_t)f * 3] * 3, *v1 = vertices + (size_t)triangles[(size_t)f * 3 + 1] * 3,
                     *v2 = vertices + (size_t)triangles[(size_t)f * 3 + 2] * 3;
        for (int q = 0; q < 3; q++) {
            tri[k * 9 + q] = v0[q];
            tri[k * 9 + 3 + q] = v1[q] - v0[q];
            tri[k * 9 + 6 + q] = v2[q] - v0[q];
        }
        for (const double *v : {v0, v1, v2}) far2 = std::max(far2, v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (vertex_normals)
            for (int j = 0; j < 3; j++)
                for (int q = 0; q < 3; q++) nrm[k * 9 + j * 3 + q] = vertex_normals[(size_t)triangles[(size_t)f * 3 + j] * 3 + q];
    }
    const std::pair<bhg::MeshRegion, const void *> whole[] = {
        {bhg::MESH_BOX, t.node_box.data()},     {bhg::MESH_SKIP, t.node_skip.data()},   {bhg::MESH_FIRST, t.node_first.data()},
        {bhg::MESH_COUNT, t.node_count.data()}, {bhg::MESH_ORDER, t.tri_order.data()}, {bhg::MESH_LEVEL_NODES, level_nodes.data()}};
    for (const auto &w : whole)
        if (g.bytes[w.first]) std::memcpy(img.data() + g.off[w.first], w.second, g.bytes[w.first]);
    bhg_mesh *m = new (std::nothrow) bhg_mesh;
    if (!m) return fail(BHG_E_NOMEM, "out of host memory");
    MeshOwner own{m};
    m->device = bhg::context_device(c);
    m->has_normals = vertex_normals != nullptr;
    char *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, g.total);
    point_into_image(m, d, g);
    if (e == hipSuccess) e = hipMemcpy(d, img.data(), g.total, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail_hip(e, "bhg_mesh_create: device image");
    m->n_nodes = (int64_t)nn;
    m->depth = t.depth;
    m->view.n_nodes = (int32_t)nn;
    m->view.n_tris = (int32_t)nt;
    m->n_vertices = (int32_t)n_vertices;
    m->level_off = level_off;
    m->n_inner = (int32_t)level_nodes.size();
    settle(m, t.node_box.data(), far2, bhg::area_sum(t.node_box.data(), nn));
    m->area_build = m->area_now;
    m->leaf_size = leaf_size;
    m->cap_vertices = n_vertices;
    m->cap_triangles = n_triangles;
    m->builds = 1;
    m->allocations = 1;
    enter_live(m);
    own.m = nullptr;
    *out = m;
    return BHG_OK;
}

void bhg_mesh_destroy(bhg_mesh *m)
{
    if (!m) return;
    {
        std::lock_guard<std::mutex> lock(live_meshes_lock);
        live_meshes.erase(m);
    }
    mesh_discard(m);
}

int bhg_mesh_info(const bhg_mesh *m, int64_t *n_nodes, int32_t *depth, double box[6])
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (n_nodes) *n_nodes = m->n_nodes;
    if (depth) *depth = m->depth;
    if (box) std::memcpy(box, m->box, sizeof(m->box));
    return BHG_OK;
}

// --- the refit of a mesh's tree -----------------------------------------------------------------------

int bhg_mesh_refit(bhg_context *c, bhg_mesh *m, const double *vertices, const double *vertex_normals)
{
    BHG_TRY(refit_check(c, m, vertices, vertex_normals));
    const size_t n3 = (size_t)m->n_vertices * 3;
    BHG_TRY(bhg::mesh_finite_check(vertices, vertex_normals, n3));
    ENTER_DEVICE(bhg::context_device(c));
    RefitScratch r;
    BHG_TRY(refit_scratch(m, r));
    // (the staging arrays are the refit's own: a refit is blocking, so no earlier one still reads them)
    hipStream_t s = bhg::context_stream(c);
    HIP_TRY(hipMemcpyAsync(r.vertices, vertices, n3 * sizeof(double), hipMemcpyHostToDevice, s));
    if (vertex_normals) HIP_TRY(hipMemcpyAsync(r.normals, vertex_normals, n3 * sizeof(double), hipMemcpyHostToDevice, s));
    return refit_run(c, m, r, r.vertices, r.normals, false, s);
}

int bhg_mesh_refit_device(bhg_context *c, bhg_mesh *m, const double *d_vertices, const double *d_vertex_normals, void *stream)
{
    BHG_TRY(refit_check(c, m, d_vertices, d_vertex_normals));
    ENTER_DEVICE(bhg::context_device(c));
    RefitScratch r;
    BHG_TRY(refit_scratch(m, r));
    return refit_run(c, m, r, d_vertices, d_vertex_normals, true, (hipStream_t)stream);
}

int bhg_mesh_refit_info(const bhg_mesh *m, uint64_t *generation, double *area_build, double *area_now)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (generation) *generation = m->generation;
    if (area_build) *area_build = m->area_build;
    if (area_now) *area_now = m->area_now;
    return BHG_OK;
}

int bhg_mesh_range(const bhg_mesh *m, double *d_min, double *d_max)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (d_min) *d_min = m->d_min;
    if (d_max) *d_max = m->d_max;
    return BHG_OK;
}

int bhg_mesh_bvh_refit_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                            const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count, const int32_t *tri_order,
                            size_t n_nodes, double *node_box, double *area)
{
    if (const char *why = bhg::mesh_refusal(vertices, n_vertices, triangles, n_triangles, 1)) return fail(BHG_E_INVALID, why);
    if (const char *why = bhg::topology_refusal(node_skip, node_first, node_count, tri_order, n_nodes, n_triangles))
        return fail(BHG_E_INVALID, why);
    if (!node_box) return fail(BHG_E_INVALID, "node_box is NULL");
    std::vector<int32_t> level_nodes, level_off;
    if (!bhg::inner_levels(node_skip, node_count, n_nodes, level_nodes, level_off))
        return fail(BHG_E_INVALID, "mesh topology: the tree is deeper than 32 levels");
    bhg::fit_boxes(vertices, triangles, node_skip, node_first, node_count, tri_order, n_nodes, node_box);
    if (area) *area = bhg::area_sum(node_box, n_nodes);
    return BHG_OK;
}

int bhg_mesh_refit_schedule_host(const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count,
                                 const int32_t *tri_order, size_t n_nodes, size_t n_triangles, int32_t *level_nodes,
                                 int32_t *level_off /* [34] */, size_t cap, size_t *n_inner)
{
    if (const char *why = bhg::topology_refusal(node_skip, node_first, node_count, tri_order, n_nodes, n_triangles))
        return fail(BHG_E_INVALID, why);
    if (!n_inner) return fail(BHG_E_INVALID, "n_inner is NULL");
    std::vector<int32_t> nodes, off;
    if (!bhg::inner_levels(node_skip, node_count, n_nodes, nodes, off))
        return fail(BHG_E_INVALID, "mesh topology: the tree is deeper than 32 levels");
    *n_inner = nodes.size();
    if (nodes.size() > cap) return fail(BHG_E_INVALID, "the tree has more inner nodes than cap (n_triangles - 1 always suffices)");
    if (!level_off || (!level_nodes && !nodes.empty())) return fail(BHG_E_INVALID, "an output array is NULL");
    if (!nodes.empty()) std::memcpy(level_nodes, nodes.data(), nodes.size() * sizeof(int32_t));
    std::memcpy(level_off, off.data(), off.size() * sizeof(int32_t));
    return BHG_OK;
}

int bhg_mesh_boxes_host(const bhg_mesh *m, double *node_box, double *tri, size_t cap)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (!node_box) return fail(BHG_E_INVALID, "node_box is NULL");
    if (cap < (size_t)m->n_nodes) return fail(BHG_E_INVALID, "the tree has more nodes than cap (bhg_mesh_info gives n_nodes)");
    ENTER_DEVICE(m->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(node_box, m->view.node_box, (size_t)m->n_nodes * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (tri) HIP_TRY(hipMemcpy(tri, m->view.tri, (size_t)m->view.n_tris * 9 * sizeof(double), hipMemcpyDeviceToHost));
    return BHG_OK;
}

// --- the device-side build: a Morton-order tree, rebuilt in place --------------------------------------

int bhg_mesh_create_device(bhg_context *c, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles, size_t n_triangles,
                           const double *d_vertex_normals, int32_t leaf_size, size_t cap_vertices, size_t cap_triangles, void *stream,
                           bhg_mesh **out)
{
    return bhg::mesh_create_built_on_device(c, d_vertices, n_vertices, d_triangles, n_triangles, d_vertex_normals, leaf_size,
                                            cap_vertices, cap_triangles, false, (hipStream_t)stream, out);
}

int bhg_mesh_rebuild_device(bhg_context *c, bhg_mesh *m, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles,
                            size_t n_triangles, const double *d_vertex_normals, void *stream)
{
    BHG_TRY(rebuild_check(c, m, d_vertices, n_vertices, d_triangles, n_triangles, d_vertex_normals));
    ENTER_DEVICE(bhg::context_device(c));
    return rebuild_run(c, m, d_vertices, n_vertices, d_triangles, n_triangles, d_vertex_normals, false, (hipStream_t)stream);
}

int bhg_mesh_rebuild(bhg_context *c, bhg_mesh *m, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                     const double *vertex_normals)
{
    BHG_TRY(rebuild_check(c, m, vertices, n_vertices, triangles, n_triangles, vertex_normals));
    ENTER_DEVICE(bhg::context_device(c));
    return rebuild_run(c, m, vertices, n_vertices, triangles, n_triangles, vertex_normals, true, bhg::context_stream(c));
}

int bhg_mesh_build_info(const bhg_mesh *m, int32_t *built_on_device, uint64_t *builds, size_t *cap_vertices, size_t *cap_triangles,
                        uint64_t *allocations)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (built_on_device) *built_on_device = m->built_on_device ? 1 : 0;
    if (builds) *builds = m->builds;
    if (cap_vertices) *cap_vertices = m->cap_vertices;
    if (cap_triangles) *cap_triangles = m->cap_triangles;
    if (allocations) *allocations = m->allocations;
    return BHG_OK;
}

int bhg_mesh_tree_host(const bhg_mesh *m, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order, size_t cap,
                       size_t *n_nodes)
{
    if (!m) return fail(BHG_E_INVALID, "mesh is NULL");
    if (!n_nodes) return fail(BHG_E_INVALID, "n_nodes is NULL");
    const size_t nn = (size_t)m->n_nodes;
    *n_nodes = nn;
    if (cap < nn) return fail(BHG_E_INVALID, "the tree has more nodes than cap (bhg_mesh_info gives n_nodes)");
    if (!node_skip || !node_first || !node_count || !tri_order) return fail(BHG_E_INVALID, "an output array is NULL");
    ENTER_DEVICE(m->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(node_skip, m->view.node_skip, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(node_first, m->view.node_first, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(node_count, m->view.node_count, nn * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tri_order, m->view.tri_order, (size_t)m->view.n_tris * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BHG_OK;
}

// --- mesh instances -----------------------------------------------------------------------------------

int bhg_mesh_instance_box_host(const double local_box[6], const double transform[12], double world_box[6])
{
    if (!local_box || !world_box) return fail(BHG_E_INVALID, "mesh instances: local_box / world_box is NULL");
    for (int q = 0; q < 6; q++)
        if (!std::isfinite(local_box[q])) return fail(BHG_E_INVALID, "mesh instances: local_box must be finite");
    BHG_TRY(bhg::mesh_instance_transforms_check(1, transform));
    instance_world_box(local_box, transform, world_box);
    return BHG_OK;
}

// the records of a set, and of a set under a tree the order and the boxes, into the host copy h; the topology stands in h already
static void instances_fill(const bhg_mesh_instances *in, const double *transforms, double *h, double box[6], double &d_min, double &d_max)
{
    instance_records(in->mesh, in->n, transforms, h, box, d_min, d_max);
    if (!in->leaf_size) return;
    const bhg::InstanceTreeLayout g = bhg::instance_tree_layout((size_t)in->n, bhg::BHG_MESH_INSTANCE_DOUBLES_, (size_t)in->n_nodes);
    char *b = (char *)h;
    bhg::instance_tree_fit(h + 12, bhg::BHG_MESH_INSTANCE_DOUBLES_, (size_t)in->n, (const int32_t *)(b + g.node_skip),
                           (const int32_t *)(b + g.node_first), (const int32_t *)(b + g.node_count), (size_t)in->n_nodes,
                           (int32_t *)(b + g.inst_order), (double *)(b + g.node_box));
}

// leaf_size 0: a linear set (bhg_mesh_instances_create); the transforms have been checked
static int instances_create(bhg_context *c, const bhg_mesh *mesh, int32_t n, const double *transforms, int32_t leaf_size,
                            bhg_mesh_instances **out)
{
    if (!mesh) return fail(BHG_E_INVALID, "mesh is NULL");
    BHG_TRY(bhg::mesh_on_device_of(c, mesh));
    ENTER_DEVICE(bhg::context_device(c));
    bhg_mesh_instances *in = new (std::nothrow) bhg_mesh_instances;
    if (!in) return fail(BHG_E_NOMEM, "out of host memory");
    in->ctx = c;
    in->device = bhg::context_device(c);
    in->mesh = mesh;
    in->mesh_serial = mesh->serial;
    in->mesh_generation = mesh->generation;
    in->n = n;
    size_t bytes = (size_t)n * bhg::BHG_MESH_INSTANCE_DOUBLES_ * sizeof(double);
    // the tree's topology: a function of (n, leaf_size), worked out here once
    std::vector<int32_t> skip, first, count;
    bhg::InstanceTreeLayout g{};
    if (leaf_size) {
        bhg::morton_topology((size_t)n, leaf_size, skip, first, count, in->depth);
        in->leaf_size = leaf_size;
        in->n_nodes = (int32_t)skip.size();
        g = bhg::instance_tree_layout((size_t)n, bhg::BHG_MESH_INSTANCE_DOUBLES_, skip.size());
        bytes = g.total;
    }
    in->bytes = bytes;
    hipError_t e = hipMalloc((void **)&in->d_rec, bytes);
    for (int k = 0; k < 2 && e == hipSuccess; k++) {
        e = hipHostMalloc((void **)&in->h_rec[k], bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&in->ev_copy[k], hipEventDisableTiming);
        if (e == hipSuccess && leaf_size) {
            char *b = (char *)in->h_rec[k];
            std::memset(b, 0, bytes);     // (the padding between the regions travels too)
            std::memcpy(b + g.node_skip, skip.data(), skip.size() * sizeof(int32_t));
            std::memcpy(b + g.node_first, first.data(), first.size() * sizeof(int32_t));
            std::memcpy(b + g.node_count, count.data(), count.size() * sizeof(int32_t));
        }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&in->ev_read, hipEventDisableTiming);
    if (e == hipSuccess) {
        instances_fill(in, transforms, in->h_rec[0], in->box, in->d_min, in->d_max);
        e = hipMemcpy(in->d_rec, in->h_rec[0], bytes, hipMemcpyHostToDevice);     // (done when the call returns)
    }
    if (e != hipSuccess) {
        bhg_mesh_instances_destroy(in);
        return fail_hip(e, "bhg_mesh_instances_create: device records");
    }
    if (leaf_size) {
        const char *d = (const char *)in->d_rec;
        in->tree = {in->d_rec, (const double *)(d + g.node_box), (const int32_t *)(d + g.node_skip), (const int32_t *)(d + g.node_first),
                    (const int32_t *)(d + g.node_count), (const int32_t *)(d + g.inst_order), in->n_nodes, n};
    }
    *out = in;
    return BHG_OK;
}

int bhg_mesh_instances_create(bhg_context *c, const bhg_mesh *mesh, int32_t n, const double *transforms, bhg_mesh_instances **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    BHG_TRY(bhg::mesh_instance_transforms_check(n, transforms));
    return instances_create(c, mesh, n, transforms, 0, out);
}

int bhg_mesh_instances_create_tree(bhg_context *c, const bhg_mesh *mesh, int32_t n, const double *transforms, int32_t leaf_size,
                                   bhg_mesh_instances **out)
{
    if (!out) return fail(BHG_E_INVALID, "out is NULL");
    *out = nullptr;
    BHG_TRY(bhg::mesh_instance_tree_check(n, transforms, leaf_size));
    return instances_create(c, mesh, n, transforms, leaf_size, out);
}

int bhg_mesh_instances_tree_info(const bhg_mesh_instances *in, int32_t *n_nodes, int32_t *depth, int32_t *leaf_size)
{
    if (!in) return fail(BHG_E_INVALID, "mesh instances: inst is NULL");
    if (n_nodes) *n_nodes = in->n_nodes;
    if (depth) *depth = in->depth;
    if (leaf_size) *leaf_size = in->leaf_size;
    return BHG_OK;
}

int bhg_mesh_instance_tree_host(const double local_box[6], int32_t n, const double *transforms, int32_t leaf_size, double *node_box,
                                int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *inst_order, int32_t *n_nodes,
                                int32_t *depth)
{
    if (!local_box) return fail(BHG_E_INVALID, "mesh instances: local_box is NULL");
    for (int q = 0; q < 6; q++)
        if (!std::isfinite(local_box[q])) return fail(BHG_E_INVALID, "mesh instances: local_box must be finite");
    BHG_TRY(bhg::mesh_instance_tree_check(n, transforms, leaf_size));
    if (!n_nodes) return fail(BHG_E_INVALID, "n_nodes is NULL");
    if (!node_box || !node_skip || !node_first || !node_count || !inst_order) return fail(BHG_E_INVALID, "an output array is NULL");
    std::vector<int32_t> skip, first, count;
    int32_t deep = 0;
    bhg::morton_topology((size_t)n, leaf_size, skip, first, count, deep);
    const size_t nn = skip.size();
    std::memcpy(node_skip, skip.data(), nn * sizeof(int32_t));
    std::memcpy(node_first, first.data(), nn * sizeof(int32_t));
    std::memcpy(node_count, count.data(), nn * sizeof(int32_t));
    std::vector<double> wbox((size_t)n * 6);
    for (int32_t j = 0; j < n; j++) instance_world_box(local_box, transforms + (size_t)j * 12, &wbox[(size_t)j * 6]);
    bhg::instance_tree_fit(wbox.data(), 6, (size_t)n, node_skip, node_first, node_count, nn, inst_order, node_box);
    *n_nodes = (int32_t)nn;
    if (depth) *depth = deep;
    return BHG_OK;
}

int bhg_mesh_instances_set(bhg_mesh_instances *in, const double *transforms)
{
    if (!in) return fail(BHG_E_INVALID, "mesh instances: inst is NULL");
    if (in->leaf_size)
        BHG_TRY(bhg::mesh_instance_tree_check(in->n, transforms, in->leaf_size));
    else
        BHG_TRY(bhg::mesh_instance_transforms_check(in->n, transforms));
    BHG_TRY(bhg::instances_usable(in->ctx, in, false));
    ENTER_DEVICE(bhg::context_device(in->ctx));
    const int k = in->last < 0 ? 1 : in->last ^ 1;
    const size_t bytes = in->bytes;
    HIP_TRY(hipEventSynchronize(in->ev_copy[k]));     // (the copy that read this host buffer last, two _set calls ago: done)
    double box[6], d_min, d_max;
    // (a set under a tree: its order and its boxes are built anew beside the records, and all of it goes up in the one copy)
    instances_fill(in, transforms, in->h_rec[k], box, d_min, d_max);
    // behind every kernel that reads the records now, whatever its stream; the readers to come wait for ev_copy[k]
    hipStream_t s = bhg::context_stream(in->ctx);
    if (in->was_read && in->read_stream != s) HIP_TRY(hipStreamWaitEvent(s, in->ev_read, 0));
    HIP_TRY(hipMemcpyAsync(in->d_rec, in->h_rec[k], bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(in->ev_copy[k], s));
    in->last = k;
    in->mesh_generation = in->mesh->generation;
    std::memcpy(in->box, box, sizeof(box));
    in->d_min = d_min;
    in->d_max = d_max;
    return BHG_OK;
}

void bhg_mesh_instances_destroy(bhg_mesh_instances *in)
{
    if (!in) return;
    {
        DeviceGuard g(in->device);
        // (what is still queued -- a copy, a kernel that reads the records -- runs out first)
        for (int k = 0; k < 2; k++) {
            if (in->ev_copy[k]) {
                (void)hipEventSynchronize(in->ev_copy[k]);
                (void)hipEventDestroy(in->ev_copy[k]);
            }
            if (in->h_rec[k]) (void)hipHostFree(in->h_rec[k]);
        }
        if (in->ev_read) {
            (void)hipEventSynchronize(in->ev_read);
            (void)hipEventDestroy(in->ev_read);
        }
        if (in->d_rec) (void)hipFree(in->d_rec);
    }
    delete in;
}

int bhg_mesh_instances_info(const bhg_mesh_instances *in, int32_t *n, double box[6])
{
    if (!in) return fail(BHG_E_INVALID, "mesh instances: inst is NULL");
    if (n) *n = in->n;
    if (box) std::memcpy(box, in->box, sizeof(in->box));
    return BHG_OK;
}

}  // extern "C"

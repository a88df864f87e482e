// mesh_object.h -- the library-side mesh and instance set (bhgeo_mesh.hip has their life cycle), and what the trace and shade
// calls of bhgeo_capi.hip read and ask of them.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/bhgeo.h"
#include "geodesic_kernels.h"

// a mesh on one device: the flattened tree of mesh_bvh.h, the triangles in leaf order, the maps between
// the two numberings
struct bhg_mesh {
    int device = 0;
    char *d = nullptr;        // one allocation
    bhg::MeshView view{};
    int64_t n_nodes = 0;
    int32_t depth = 0;
    double box[6] = {0, 0, 0, 0, 0, 0};
    double d_min = 0.0, d_max = 0.0;
    uint64_t serial = 0;      // its entry in live_meshes, which an instance set checks before it trusts its pointer
    // the refit: what _create leaves on the device for it beside the view's arrays, and what it keeps count of
    int32_t n_vertices = 0;
    bool has_normals = false;
    const int32_t *slot_vert = nullptr;     // in d, [nt][3]: the caller's vertex indices of the triangle in each leaf slot
    const int32_t *level_nodes = nullptr;   // in d, [n_inner]: the inner nodes grouped by level (mesh_bvh.h, inner_levels)
    std::vector<int32_t> level_off;         // [BVH_MAX_DEPTH + 2]
    int32_t n_inner = 0;
    char *d_refit = nullptr;  // the first refit's allocation, kept: summary | area [nn] | staging of host vertices and normals
    uint64_t generation = 0;  // +1 per successful refit or rebuild
    double area_build = 0.0, area_now = 0.0;
    // the device build.  by_capacity: d and d_refit are laid out for cap_vertices / cap_triangles (a mesh of
    // bhg_mesh_create_device, or one of bhg_mesh_create since its first rebuild) and not for the counts the host builder was given
    int32_t leaf_size = 0;
    size_t cap_vertices = 0, cap_triangles = 0;
    bool by_capacity = false, built_on_device = false;
    char *d_build = nullptr;  // record | keys in | keys out | values in | staging of host triangles | the sort's own storage
    size_t sort_bytes = 0;
    size_t topo_triangles = 0;              // the n_triangles whose Morton topology (at leaf_size) lies in d; 0: none
    uint64_t builds = 0, allocations = 0;   // builds, the creating one included; device allocations over the mesh's life
};

// K rigid placements of one mesh: the device records, and what the host works out from them in O(K)
struct bhg_mesh_instances {
    bhg_context *ctx = nullptr;
    int device = 0;               // ctx's (the set may be destroyed after its context)
    const bhg_mesh *mesh = nullptr;
    uint64_t mesh_serial = 0;
    uint64_t mesh_generation = 0; // the mesh's at _create / _set: the world boxes come from the local box of that generation
    int32_t n = 0;
    double *d_rec = nullptr;      // [n][BHG_MESH_INSTANCE_DOUBLES_]
    double box[6] = {0, 0, 0, 0, 0, 0};     // the union of the world boxes
    double d_min = 0.0, d_max = 0.0;
    // The records are written by _set on the context's stream and read by traces and shades on whatever stream their caller
    // names: the set orders the two itself, so that no caller has to.
    //   * h_rec: two page-locked host copies, used in turn; a copy's event (ev_copy) is waited for on the host before its buffer
    //     is filled again, so a queued copy always reads what its _set wrote;
    //   * a reader's stream waits for the last copy (ev_copy[last]) before it launches, and leaves ev_read behind it; a reader on
    //     another stream than the one before waits for that one's ev_read first, so the last ev_read stands for every reader;
    //   * _set makes the context's stream wait for ev_read before the copy: no kernel still reads what it overwrites.
    // (mutable: a reader holds the set const, and reads)
    double *h_rec[2] = {nullptr, nullptr};
    hipEvent_t ev_copy[2] = {nullptr, nullptr};
    mutable hipEvent_t ev_read = nullptr;
    mutable hipStream_t read_stream = nullptr;
    mutable bool was_read = false;
    int last = -1;                // the host copy of the latest _set (-1: the creating upload, synchronous)
    // A set of bhg_mesh_instances_create_tree (leaf_size 0: a linear set): d_rec and both host copies are laid
    // out by instance_tree_layout -- the records first, where a linear set has them, then the tree -- and travel as one copy of
    // `bytes`.  tree points into d_rec.  The topology is written into both host copies once, by _create_tree; a _set rewrites the
    // records, the boxes and the order of its copy.
    int32_t leaf_size = 0, n_nodes = 0, depth = 0;
    size_t bytes = 0;             // of d_rec and of each host copy
    bhg::InstanceTreeView tree{};
};

#pragma GCC visibility push(hidden)
namespace bhg {

// BHGEO_MESH_CULL=0: every step of every ray samples its sub-chords, and no instance's world box is looked at (an A/B aid: the
// results are the same bits)
bool mesh_culls_on();
// BHGEO_INSTANCE_TREE=0: a set under a tree is walked by the linear loop over all its records (an A/B aid of the same kind)
bool instance_tree_on();
// A kernel on stream s is about to read the set's records / has been launched (bhg_mesh_instances has the protocol)
hipError_t instances_before_read(const bhg_mesh_instances *in, hipStream_t s);
hipError_t instances_after_read(const bhg_mesh_instances *in, hipStream_t s);
// the set is this context's and its mesh alive.  reading: the call traces or shades with the set's world boxes, which a refit of
// the mesh since the last _set has left stale
int instances_usable(const bhg_context *c, const bhg_mesh_instances *inst, bool reading = true);
// there is a context, and the mesh lives on its device
int mesh_on_device_of(const bhg_context *c, const bhg_mesh *m);
// what the mesh trace covers, checked before the context (a refusal names its figure with or without a device)
int mesh_trace_check(const bhg_params *p, const bhg_mesh *mesh, double max_chord, const int32_t *tri_id, const double *bary);
int instances_trace_check(const bhg_params *p, const bhg_mesh_instances *inst, double max_chord, const int32_t *tri_id,
                          const int32_t *inst_id, const double *bary);

}  // namespace bhg
#pragma GCC visibility pop

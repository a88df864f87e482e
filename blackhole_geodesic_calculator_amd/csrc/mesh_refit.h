// mesh_refit.h -- the refit of a mesh's tree on the device: what bhgeo_mesh.hip hands to mesh_refit.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_bvh.h"

namespace bhg {

// what a refit reports back: one small device record, read by the host once the kernels are done
struct MeshRefitSummary {
    double box[6];              // the root box, widened
    double area;                // the area sum of mesh_bvh.h's area_sum, in its order
    unsigned long long d2_max;  // the bits of the largest |v|^2 over the triangles' vertices (>= 0: the bits order as the values)
    uint32_t nonfinite;         // the scan: bit 0 a non-finite vertex coordinate, bit 1 a non-finite normal
    uint32_t pad;
};

struct MeshRefitArgs {
    const double *vertices;     // device [nv][3]
    const double *normals;      // device [nv][3], or nullptr (the mesh has none)
    int32_t n_vertices, n_tris, n_nodes, n_inner;
    // what bhg_mesh_create left on the device for this
    const int32_t *slot_vert;   // [nt][3]: the caller's vertex indices of the triangle in each leaf slot
    const int32_t *node_skip, *node_first, *node_count;
    const int32_t *level_nodes; // [n_inner]: the inner nodes, grouped by level (mesh_bvh.h, inner_levels)
    int32_t level_off[BVH_MAX_DEPTH + 2];
    // what it writes
    double *node_box;           // [nn][6]
    double *tri;                // [nt][9]
    double *tri_normals;        // [nt][9] or nullptr
    double *area;               // [nn] scratch: each node's area
    MeshRefitSummary *summary;
};

// the inner nodes a single workgroup walks level by level with barriers in one launch; above it, one launch per level
constexpr int32_t MESH_REFIT_ONE_GROUP_NODES = 1024;

// scan the new vertices (and normals) for non-finite values into summary->nonfinite: nothing of the mesh is written
hipError_t launch_mesh_refit_scan(const MeshRefitArgs &a, hipStream_t s);
// the refit proper: slot records, leaf boxes, inner boxes bottom-up, widening, summary
// (both want the summary zeroed by the caller first: the flag is OR-ed and the largest |v|^2 is max-ed into it)
hipError_t launch_mesh_refit(const MeshRefitArgs &a, hipStream_t s);

}  // namespace bhg

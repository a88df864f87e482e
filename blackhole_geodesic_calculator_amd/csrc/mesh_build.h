// mesh_build.h -- the build of a mesh's tree on the device: what bhgeo_mesh.hip hands to mesh_build.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_bvh.h"

namespace bhg {

// what the build's first kernels report: one small device record, zeroed by the caller before the scan
struct MeshBuildRecord {
    // the centroid bounds as order-preserving bit images of the doubles, both kept with atomicMax so that zero is the start of
    // either: hi[a] holds image(max), lo[a] holds ~image(min)
    unsigned long long lo[3], hi[3];
    uint32_t bad_index;         // the scan: non-zero when a triangle index lies outside [0, n_vertices)
    uint32_t pad;
};

struct MeshBuildArgs {
    const double *vertices;     // device [nv][3]
    const int32_t *triangles;   // device [nt][3]
    int32_t n_vertices, n_tris, n_nodes, pad;
    // the topology of mesh_bvh.h's morton_topology, already on the device
    const int32_t *node_first, *node_count;
    // the build's own storage
    MeshBuildRecord *record;
    unsigned long long *keys_in, *keys_out;   // [nt] each
    int32_t *vals_in;           // [nt]: 0 .. nt - 1
    void *sort_temp;
    size_t sort_temp_bytes;
    // what it writes of the mesh
    int32_t *tri_order;         // [nt]: leaf slot -> the caller's triangle
    int32_t *tri_slot;          // [nt]: the inverse
    int32_t *slot_vert;         // [nt][3]
};

// the bytes the sort wants beside its key and value arrays, for n pairs
hipError_t mesh_build_sort_bytes(size_t n, size_t *bytes);
// every triangle index against [0, n_vertices) into record->bad_index: reads the triangle array only, writes nothing of the mesh
hipError_t launch_mesh_build_scan(const MeshBuildArgs &a, hipStream_t s);
// centroid bounds, keys, sort, leaf order, maps: only for arrays whose scan has been read back and found clean
hipError_t launch_mesh_build(const MeshBuildArgs &a, hipStream_t s);

}  // namespace bhg

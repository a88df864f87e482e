// mesh_layout.h -- where a mesh object's arrays lie in its three device allocations (bhgeo_mesh.hip): the image of the tree and the
// triangles, the refit's scratch, the build's storage -- and where an instance set under a tree keeps its records and its tree.
// Host only, no HIP: tests/mesh_layout_driver.cpp and tests/mesh_instance_tree_driver.cpp run it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#pragma GCC visibility push(hidden)
namespace bhg {

// regions one behind the other in the order they are added: each starts at a multiple of align and is padded to one
struct RegionList {
    size_t end = 0;
    size_t add(size_t bytes, size_t align = 8)
    {
        const size_t off = (end + align - 1) & ~(align - 1);
        end = off + ((bytes + align - 1) & ~(align - 1));
        return off;
    }
};

// The device image of a mesh (DESIGN.md sections 19, 22): the arrays of a tree of n_nodes nodes, n_inner of them inner, over n_tris
// triangles, in this order: boxes [n_nodes][6] | triangles (v0, e1, e2) [n_tris][9] | vertex normals [n_tris][9] or nothing | skip,
// first, count [n_nodes] | order, slot [n_tris] | the vertex indices per slot [n_tris][3] | the inner nodes by level [n_inner].
// off[r]: where region r starts; bytes[r]: the size of its array (the region itself is padded to 8 bytes).
enum MeshRegion { MESH_BOX, MESH_TRI, MESH_NORMALS, MESH_SKIP, MESH_FIRST, MESH_COUNT, MESH_ORDER, MESH_SLOT, MESH_SLOT_VERT,
                  MESH_LEVEL_NODES, MESH_REGIONS };

struct MeshImage {
    size_t off[MESH_REGIONS], bytes[MESH_REGIONS], total;
};
inline MeshImage mesh_image(size_t n_nodes, size_t n_tris, size_t n_inner, bool normals)
{
    const size_t d = sizeof(double), i = sizeof(int32_t);
    MeshImage g = {{}, {n_nodes * 6 * d, n_tris * 9 * d, normals ? n_tris * 9 * d : 0, n_nodes * i, n_nodes * i, n_nodes * i, n_tris * i,
                        n_tris * i, n_tris * 3 * i, n_inner * i}, 0};
    RegionList l;
    for (int r = 0; r < MESH_REGIONS; r++) g.off[r] = l.add(g.bytes[r]);
    g.total = l.end;
    return g;
}

// the refit's scratch: summary | area [n_nodes] | staging of host vertices [n_vertices][3] | and normals
struct RefitLayout {
    size_t summary, area, vertices, normals, total;
};
inline RefitLayout refit_layout(size_t summary_bytes, size_t n_nodes, size_t n_vertices, bool normals)
{
    RegionList l;
    const size_t b_v = n_vertices * 3 * sizeof(double), summary = l.add(summary_bytes), area = l.add(n_nodes * sizeof(double)),
                 vertices = l.add(b_v), nrm = l.add(normals ? b_v : 0);
    return {summary, area, vertices, nrm, l.end};
}

// the build's storage for cap triangles: record | keys in | keys out | values in | staging of host triangles
// [cap][3] | the sort's own storage.  The record and the sort's storage have 256-byte blocks of their own.
struct BuildLayout {
    size_t record, keys_in, keys_out, vals_in, triangles, sort, total;
};
inline BuildLayout build_layout(size_t record_bytes, size_t cap, size_t sort_bytes)
{
    RegionList l;
    const size_t record = l.add(record_bytes, 256), keys_in = l.add(cap * sizeof(uint64_t)), keys_out = l.add(cap * sizeof(uint64_t)),
                 vals_in = l.add(cap * sizeof(int32_t)), triangles = l.add(cap * 3 * sizeof(int32_t)), sort = l.add(sort_bytes, 256);
    return {record, keys_in, keys_out, vals_in, triangles, sort, l.end};
}

// the one allocation of an instance set that lies under a tree, and each of its two page-locked host copies:
// records [n][rec_doubles] | node boxes [n_nodes][6] | skip, first, count [n_nodes] | the instances in leaf order [n].  A move
// uploads all of it in one copy of `total` bytes.
struct InstanceTreeLayout {
    size_t records, node_box, node_skip, node_first, node_count, inst_order, total;
};
inline InstanceTreeLayout instance_tree_layout(size_t n, size_t rec_doubles, size_t n_nodes)
{
    RegionList l;
    const size_t d = sizeof(double), i = sizeof(int32_t);
    const size_t records = l.add(n * rec_doubles * d), box = l.add(n_nodes * 6 * d), skip = l.add(n_nodes * i), first = l.add(n_nodes * i),
                 count = l.add(n_nodes * i), order = l.add(n * i);
    return {records, box, skip, first, count, order, l.end};
}

}  // namespace bhg
#pragma GCC visibility pop

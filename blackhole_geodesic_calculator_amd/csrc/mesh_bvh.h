// mesh_bvh.h -- the host-side BVH builder of the triangle-mesh trace.  Host C++ only: no HIP in here
// (the Morton cell and key functions at the end carry __host__ __device__ when a HIP compiler reads them).
//
// A binary tree over the triangles' boxes, split at the median (by count) of the longest axis of the centroid bounds, and
// flattened in depth-first pre-order with one skip link per node:
//     a box miss at node i goes to skip[i], anything else to i + 1, and skip[i] > i for every node,
// so a traversal is a loop over a strictly increasing index: no stack, no runtime-indexed private array.
// Leaves (count > 0) hold the triangles first .. first + count - 1 of the leaf order; tri_order[slot] is the caller's index of
// the triangle in that slot.  Inner nodes have count = 0 and first = -1; the left child of inner node i is i + 1, the right
// one skip[i + 1].
//
// Depth.  Every split halves the COUNT (std::nth_element at the middle): a node of m triangles has children of floor(m / 2)
// and ceil(m / 2), both non-empty.  With nt <= 2^31 - 1 the depth is at most 31 levels below the root, whatever the
// geometry, and the builder's explicit stack (BVH_MAX_DEPTH + 2 entries: one pending right child per level) cannot overflow.
// A range whose centroids all coincide -- a split would separate nothing -- becomes a leaf, even over leaf_size: nt identical
// triangles are ONE leaf.
//
// Boxes are fp64 and widened outward at build time by BVH_BOX_ULPS ulps of their largest coordinate magnitude, so that the
// box test of the traversal (which adds its own relative slack) can never reject what the triangle test accepts.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace bhg {

constexpr int BVH_MAX_DEPTH = 32;
constexpr double BVH_BOX_ULPS = 16.0;

struct HostBvh {
    std::vector<double> node_box;      // [n_nodes][6]: lo x, y, z, hi x, y, z
    std::vector<int32_t> node_skip, node_first, node_count;
    std::vector<int32_t> tri_order;    // [nt]: leaf slot -> the caller's triangle
    int32_t depth = 0;                 // levels below the root (a single leaf: 0)
};

// nullptr when the mesh is acceptable, else the reason (nothing has been allocated)
inline const char *mesh_refusal(const double *vertices, size_t nv, const int32_t *triangles, size_t nt, int32_t leaf_size)
{
    if (!vertices || !triangles) return "mesh: vertices / triangles is NULL";
    if (nv == 0 || nt == 0) return "mesh: n_vertices and n_triangles must be > 0";
    if (nv > 0x7FFFFFFFull || nt > 0x7FFFFFFFull) return "mesh: n_vertices and n_triangles must be <= 2^31 - 1";
    if (leaf_size < 1) return "mesh: leaf_size must be >= 1";
    for (size_t i = 0; i < nv * 3; i++)
        if (!std::isfinite(vertices[i])) return "mesh: every vertex must be finite";
    for (size_t i = 0; i < nt * 3; i++)
        if (triangles[i] < 0 || (size_t)triangles[i] >= nv) return "mesh: a triangle index lies outside [0, n_vertices)";
    return nullptr;
}

// The boxes of a tree whose topology stands (what the builder ends with, and all a refit does).  A leaf's box
// is the exact min / max over its triangles' vertices, an inner node's the union of its two children's, children before parents;
// then every box is widened outward by BVH_BOX_ULPS ulps of its own largest magnitude: a parent's magnitude is at least its
// children's, so a widened child stays inside its widened parent.  The refit kernels (mesh_refit.hip) do these operations on
// these operands in this order: the same bits.
inline void fit_boxes(const double *V, const int32_t *F, const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count,
                      const int32_t *order, size_t nn, double *node_box)
{
    for (size_t i = nn; i-- > 0;) {
        double *b = &node_box[i * 6];
        if (node_count[i] > 0) {
            for (int c = 0; c < 3; c++) {
                b[c] = INFINITY;
                b[3 + c] = -INFINITY;
            }
            for (int32_t k = 0; k < node_count[i]; k++) {
                const int32_t t = order[(size_t)node_first[i] + k];
                for (int j = 0; j < 3; j++)
                    for (int c = 0; c < 3; c++) {
                        const double x = V[(size_t)F[(size_t)t * 3 + j] * 3 + c];
                        b[c] = std::min(b[c], x);
                        b[3 + c] = std::max(b[3 + c], x);
                    }
            }
        } else {
            const size_t l = i + 1, r = (size_t)node_skip[l];
            for (int c = 0; c < 3; c++) {
                b[c] = std::min(node_box[l * 6 + c], node_box[r * 6 + c]);
                b[3 + c] = std::max(node_box[l * 6 + 3 + c], node_box[r * 6 + 3 + c]);
            }
        }
    }
    for (size_t i = 0; i < nn; i++) {
        double *b = &node_box[i * 6];
        double mag = 0.0;
        for (int c = 0; c < 6; c++) mag = std::max(mag, std::fabs(b[c]));
        const double w = BVH_BOX_ULPS * 2.220446049250313e-16 * std::max(mag, 2.2250738585072014e-308);
        for (int c = 0; c < 3; c++) {
            b[c] -= w;
            b[3 + c] += w;
        }
    }
}

// The tree's area sum: the sum over all nodes of dx dy + dy dz + dz dx of the widened box, the figure a
// refitted tree's degradation is read from.  Reduced in one fixed order, which the device's reduction (mesh_refit.hip) restates:
// BVH_AREA_LANES partial sums, lane l over the nodes l, l + BVH_AREA_LANES, ... in rising order, then a halving tree over the lanes.
constexpr int BVH_AREA_LANES = 256;
inline double box_area(const double *b)
{
    const double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    return dx * dy + dy * dz + dz * dx;
}
inline double area_sum(const double *node_box, size_t nn)
{
    double lane[BVH_AREA_LANES];
    for (int l = 0; l < BVH_AREA_LANES; l++) lane[l] = 0.0;
    for (size_t i = 0; i < nn; i++) lane[i % BVH_AREA_LANES] += box_area(node_box + i * 6);
    for (int s = BVH_AREA_LANES / 2; s > 0; s >>= 1)
        for (int l = 0; l < s; l++) lane[l] += lane[l + s];
    return lane[0];
}

// nullptr when (node_skip, node_first, node_count, tri_order) is a tree of build_bvh's kind over nt triangles that fit_boxes and
// inner_levels may walk, else the reason: every index in range, skip links forward, both children of an inner node present, every
// leaf slot in exactly one leaf
inline const char *topology_refusal(const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count,
                                    const int32_t *tri_order, size_t nn, size_t nt)
{
    if (!node_skip || !node_first || !node_count || !tri_order) return "mesh topology: an array is NULL";
    if (nn == 0 || nn > 0x7FFFFFFFull || nt == 0 || nt > 0x7FFFFFFFull) return "mesh topology: n_nodes and n_triangles must be in [1, 2^31 - 1]";
    size_t next_slot = 0;
    for (size_t i = 0; i < nn; i++) {
        if (node_skip[i] <= (int64_t)i || (size_t)node_skip[i] > nn) return "mesh topology: node_skip must lie in (i, n_nodes]";
        if (node_count[i] < 0) return "mesh topology: node_count must be >= 0";
        if (node_count[i] > 0) {
            // (pre-order: the leaves hold the slots in rising order, without gaps)
            if (node_first[i] < 0 || (size_t)node_first[i] != next_slot || (size_t)node_count[i] > nt - next_slot)
                return "mesh topology: the leaves must hold the slots 0 .. n_triangles - 1 in order";
            if ((size_t)node_skip[i] != i + 1) return "mesh topology: a leaf's node_skip must be i + 1";
            next_slot += (size_t)node_count[i];
        } else {
            if (i + 2 >= nn || (size_t)node_skip[i + 1] >= nn || node_skip[(size_t)node_skip[i + 1]] != node_skip[i])
                return "mesh topology: an inner node must have two children that end where it ends";
        }
    }
    if (next_slot != nt) return "mesh topology: the leaves must hold the slots 0 .. n_triangles - 1 in order";
    for (size_t k = 0; k < nt; k++)
        if (tri_order[k] < 0 || (size_t)tri_order[k] >= nt) return "mesh topology: tri_order must lie in [0, n_triangles)";
    return nullptr;
}

// The bottom-up schedule of a refit: the inner nodes grouped by level -- level_nodes[level_off[d] ..
// level_off[d + 1]) are the inner nodes d levels below the root, in rising index order -- so that the levels are walked deepest
// first and the nodes of one level in any order.  false: the tree is deeper than BVH_MAX_DEPTH (not one of build_bvh's).
inline bool inner_levels(const int32_t *node_skip, const int32_t *node_count, size_t nn, std::vector<int32_t> &level_nodes,
                         std::vector<int32_t> &level_off)
{
    std::vector<int32_t> depth(nn, 0);
    std::vector<size_t> width(BVH_MAX_DEPTH + 1, 0);
    for (size_t i = 0; i < nn; i++) {
        if (node_count[i] > 0) continue;
        if (depth[i] >= BVH_MAX_DEPTH) return false;
        depth[i + 1] = depth[(size_t)node_skip[i + 1]] = depth[i] + 1;
        width[(size_t)depth[i]]++;
    }
    level_off.assign(BVH_MAX_DEPTH + 2, 0);
    for (int d = 0; d <= BVH_MAX_DEPTH; d++) level_off[(size_t)d + 1] = level_off[(size_t)d] + (int32_t)width[(size_t)d];
    level_nodes.assign((size_t)level_off[BVH_MAX_DEPTH + 1], 0);
    std::vector<int32_t> at(level_off.begin(), level_off.end() - 1);
    for (size_t i = 0; i < nn; i++)
        if (node_count[i] == 0) level_nodes[(size_t)at[(size_t)depth[i]]++] = (int32_t)i;
    return true;
}

// the mesh has passed mesh_refusal
inline void build_bvh(const double *V, const int32_t *F, size_t nt, int32_t leaf_size, HostBvh &out)
{
    std::vector<double> cen(nt * 3);
    for (size_t t = 0; t < nt; t++)
        for (int c = 0; c < 3; c++)
            cen[t * 3 + c] = (V[(size_t)F[t * 3] * 3 + c] + V[(size_t)F[t * 3 + 1] * 3 + c] + V[(size_t)F[t * 3 + 2] * 3 + c]) / 3.0;
    std::vector<int32_t> &order = out.tri_order;
    order.resize(nt);
    for (size_t t = 0; t < nt; t++) order[t] = (int32_t)t;
    out.node_box.clear();
    out.node_skip.clear();
    out.node_first.clear();
    out.node_count.clear();
    out.depth = 0;
    struct Range {
        size_t lo, hi;
        int32_t depth;
    };
    Range stack[BVH_MAX_DEPTH + 2];
    int sp = 0;
    stack[sp++] = Range{0, nt, 0};
    while (sp > 0) {
        const Range r = stack[--sp];
        const size_t m = r.hi - r.lo;
        if (r.depth > out.depth) out.depth = r.depth;
        // the centroid bounds of the range and their longest axis
        double lo[3], hi[3];
        for (int c = 0; c < 3; c++) lo[c] = hi[c] = cen[(size_t)order[r.lo] * 3 + c];
        for (size_t k = r.lo + 1; k < r.hi; k++)
            for (int c = 0; c < 3; c++) {
                const double x = cen[(size_t)order[k] * 3 + c];
                lo[c] = std::min(lo[c], x);
                hi[c] = std::max(hi[c], x);
            }
        int axis = 0;
        for (int c = 1; c < 3; c++)
            if (hi[c] - lo[c] > hi[axis] - lo[axis]) axis = c;
        const bool leaf = m <= (size_t)leaf_size || !(hi[axis] - lo[axis] > 0.0) || r.depth >= BVH_MAX_DEPTH;
        out.node_skip.push_back(0);
        out.node_box.insert(out.node_box.end(), 6, 0.0);
        if (leaf) {
            // (the slots of a leaf in the caller's order: the tree is the same whatever nth_element left inside a half)
            std::sort(order.begin() + r.lo, order.begin() + r.hi);
            out.node_first.push_back((int32_t)r.lo);
            out.node_count.push_back((int32_t)m);
            continue;
        }
        out.node_first.push_back(-1);
        out.node_count.push_back(0);
        const size_t mid = r.lo + m / 2;
        // a strict total order (centroid, then index): the two halves are the same sets with every standard library
        std::nth_element(order.begin() + r.lo, order.begin() + mid, order.begin() + r.hi, [&](int32_t a, int32_t b) {
            const double xa = cen[(size_t)a * 3 + axis], xb = cen[(size_t)b * 3 + axis];
            return xa < xb || (xa == xb && a < b);
        });
        stack[sp++] = Range{mid, r.hi, r.depth + 1};   // the right child, after the whole left subtree
        stack[sp++] = Range{r.lo, mid, r.depth + 1};
    }
    // skip links, children before parents (pre-order: every child has a larger index than its parent); then the boxes
    const size_t nn = out.node_skip.size();
    for (size_t i = nn; i-- > 0;) {
        if (out.node_count[i] > 0) {
            out.node_skip[i] = (int32_t)(i + 1);
        } else {
            const size_t l = i + 1, r = (size_t)out.node_skip[l];
            out.node_skip[i] = out.node_skip[r];
        }
    }
    fit_boxes(V, F, out.node_skip.data(), out.node_first.data(), out.node_count.data(), order.data(), nn, out.node_box.data());
}

// ---- the Morton tree: the build the device can do, stated here for the host ---------------------------------
// The triangles are put in the order of a 63-bit Morton key of their centroids (ties by the caller's index), and the tree laid
// over that order splits every range by COUNT at lo + m / 2, as build_bvh does: its shape is a function of (nt, leaf_size) alone.
// mesh_build.hip restates morton_cell, morton_key and the leaf order; the topology below is what it is handed.

// (the cell and key functions are the kernels' too: plain C++ that the device compiler takes as it stands)
#if defined(__HIPCC__)
#define BHG_HOST_DEVICE __host__ __device__
#else
#define BHG_HOST_DEVICE
#endif

// the leaf sizes the device build takes (its per-leaf sort is one thread's loop)
constexpr int32_t MORTON_LEAF_MAX = 64;

// 2^21 / ext, or 0 for an axis without a finite extent > 0 (every cell of that axis is 0)
BHG_HOST_DEVICE inline double morton_scale(double lo, double hi)
{
    const double ext = hi - lo;
    return (ext > 0.0 && ext < INFINITY) ? 2097152.0 / ext : 0.0;
}

// min(2^21 - 1, (uint64)((c - lo) * scale)), with the cases a conversion leaves open settled: a product that is not > 0 (and so a
// NaN from 0 * inf, when ext is so small that the scale overflows) gives 0
BHG_HOST_DEVICE inline uint64_t morton_cell(double c, double lo, double scale)
{
    if (!(scale > 0.0)) return 0;
    const double f = (c - lo) * scale;
    return f >= 2097151.0 ? (uint64_t)2097151 : (f > 0.0 ? (uint64_t)f : (uint64_t)0);
}

// bit k of q to bit 3 k
BHG_HOST_DEVICE inline uint64_t morton_spread(uint64_t q)
{
    q &= 0x1FFFFFull;
    q = (q | q << 32) & 0x1F00000000FFFFull;
    q = (q | q << 16) & 0x1F0000FF0000FFull;
    q = (q | q << 8) & 0x100F00F00F00F00Full;
    q = (q | q << 4) & 0x10C30C30C30C30C3ull;
    q = (q | q << 2) & 0x1249249249249249ull;
    return q;
}
BHG_HOST_DEVICE inline uint64_t morton_key(uint64_t qx, uint64_t qy, uint64_t qz) { return morton_spread(qx) << 2 | morton_spread(qy) << 1 | morton_spread(qz); }

// node_skip, node_first, node_count and the depth of the count-split tree over nt slots, in build_bvh's pre-order
inline void morton_topology(size_t nt, int32_t leaf_size, std::vector<int32_t> &node_skip, std::vector<int32_t> &node_first,
                            std::vector<int32_t> &node_count, int32_t &depth)
{
    node_skip.clear();
    node_first.clear();
    node_count.clear();
    depth = 0;
    struct Range {
        size_t lo, hi;
        int32_t depth;
    };
    Range stack[BVH_MAX_DEPTH + 2];
    int sp = 0;
    stack[sp++] = Range{0, nt, 0};
    while (sp > 0) {
        const Range r = stack[--sp];
        const size_t m = r.hi - r.lo;
        if (r.depth > depth) depth = r.depth;
        node_skip.push_back(0);
        if (m <= (size_t)leaf_size) {
            node_first.push_back((int32_t)r.lo);
            node_count.push_back((int32_t)m);
            continue;
        }
        node_first.push_back(-1);
        node_count.push_back(0);
        const size_t mid = r.lo + m / 2;
        stack[sp++] = Range{mid, r.hi, r.depth + 1};
        stack[sp++] = Range{r.lo, mid, r.depth + 1};
    }
    const size_t nn = node_skip.size();
    for (size_t i = nn; i-- > 0;) {
        if (node_count[i] > 0) node_skip[i] = (int32_t)(i + 1);
        else node_skip[i] = node_skip[(size_t)node_skip[i + 1]];
    }
}

// the Morton keys of the triangles' centroids (the mesh has passed mesh_refusal)
inline void morton_keys(const double *V, const int32_t *F, size_t nt, std::vector<uint64_t> &key)
{
    std::vector<double> cen(nt * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t t = 0; t < nt; t++)
        for (int c = 0; c < 3; c++) {
            const double x = (V[(size_t)F[t * 3] * 3 + c] + V[(size_t)F[t * 3 + 1] * 3 + c] + V[(size_t)F[t * 3 + 2] * 3 + c]) / 3.0;
            cen[t * 3 + c] = x;
            lo[c] = std::min(lo[c], x);
            hi[c] = std::max(hi[c], x);
        }
    double scale[3];
    for (int c = 0; c < 3; c++) scale[c] = morton_scale(lo[c], hi[c]);
    key.resize(nt);
    for (size_t t = 0; t < nt; t++)
        key[t] = morton_key(morton_cell(cen[t * 3], lo[0], scale[0]), morton_cell(cen[t * 3 + 1], lo[1], scale[1]),
                            morton_cell(cen[t * 3 + 2], lo[2], scale[2]));
}

// the mesh has passed mesh_refusal
inline void build_bvh_morton(const double *V, const int32_t *F, size_t nt, int32_t leaf_size, HostBvh &out)
{
    std::vector<uint64_t> key;
    morton_keys(V, F, nt, key);
    std::vector<int32_t> &order = out.tri_order;
    order.resize(nt);
    for (size_t t = 0; t < nt; t++) order[t] = (int32_t)t;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    morton_topology(nt, leaf_size, out.node_skip, out.node_first, out.node_count, out.depth);
    const size_t nn = out.node_skip.size();
    for (size_t i = 0; i < nn; i++)
        if (out.node_count[i] > 0) std::sort(order.begin() + out.node_first[i], order.begin() + out.node_first[i] + out.node_count[i]);
    out.node_box.assign(nn * 6, 0.0);
    fit_boxes(V, F, out.node_skip.data(), out.node_first.data(), out.node_count.data(), order.data(), nn, out.node_box.data());
}

}  // namespace bhg

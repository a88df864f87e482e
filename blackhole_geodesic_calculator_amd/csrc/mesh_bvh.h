// mesh_bvh.h -- the host-side BVH builder of the triangle-mesh trace.  Host C++ only: no HIP in here.
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
    // skip links and boxes, children before parents (pre-order: every child has a larger index than its parent)
    const size_t nn = out.node_skip.size();
    for (size_t i = nn; i-- > 0;) {
        double *b = &out.node_box[i * 6];
        if (out.node_count[i] > 0) {
            out.node_skip[i] = (int32_t)(i + 1);
            for (int c = 0; c < 3; c++) {
                b[c] = INFINITY;
                b[3 + c] = -INFINITY;
            }
            for (int32_t k = 0; k < out.node_count[i]; k++) {
                const int32_t t = order[(size_t)out.node_first[i] + k];
                for (int j = 0; j < 3; j++)
                    for (int c = 0; c < 3; c++) {
                        const double x = V[(size_t)F[(size_t)t * 3 + j] * 3 + c];
                        b[c] = std::min(b[c], x);
                        b[3 + c] = std::max(b[3 + c], x);
                    }
            }
        } else {
            const size_t l = i + 1, r = (size_t)out.node_skip[l];
            out.node_skip[i] = out.node_skip[r];
            for (int c = 0; c < 3; c++) {
                b[c] = std::min(out.node_box[l * 6 + c], out.node_box[r * 6 + c]);
                b[3 + c] = std::max(out.node_box[l * 6 + 3 + c], out.node_box[r * 6 + 3 + c]);
            }
        }
    }
    // widen: a parent's magnitude is at least its children's, so a widened child stays inside its widened parent
    for (size_t i = 0; i < nn; i++) {
        double *b = &out.node_box[i * 6];
        double mag = 0.0;
        for (int c = 0; c < 6; c++) mag = std::max(mag, std::fabs(b[c]));
        const double w = BVH_BOX_ULPS * 2.220446049250313e-16 * std::max(mag, 2.2250738585072014e-308);
        for (int c = 0; c < 3; c++) {
            b[c] -= w;
            b[3 + c] += w;
        }
    }
}

}  // namespace bhg

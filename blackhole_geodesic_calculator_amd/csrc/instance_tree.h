// instance_tree.h -- the host-side builder of the upper level of the two-level structure: a bounding-box
// tree over the world boxes of an instance set's placements.  Host C++ only, no HIP: tests/mesh_instance_tree_driver.cpp runs it
// under the host sanitizers.
//
// The tree is flattened as mesh_bvh.h flattens its own: depth-first pre-order, one skip link per node, leaves that hold first and
// count into inst_order[], which holds the caller's instance indices.  Its SHAPE is a function of (K, leaf_size) alone -- it is
// morton_topology(K, leaf_size) -- because every range is split by count at lo + m / 2, down to leaf_size, whatever the geometry:
// K coinciding placements give a tree of depth ceil(log2 K), not one leaf.  So the topology is written once, when the set is
// created, and a move (instance_tree_fit) rewrites the order and the boxes in place and allocates nothing.
//
// A range is split on the longest axis of the bounds of its boxes' centres, the instances ordered by (centre coordinate, instance
// index): a total order, the two halves are the same sets with every standard library.  A leaf's box is the exact union (min /
// max) of its instances' world boxes, an inner node's that of its two children's.  Nothing is widened here: the world boxes have
// been widened by BVH_BOX_ULPS already (instance_world_box), and a union of boxes holds what they hold.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "mesh_bvh.h"

namespace bhg {

constexpr int32_t INSTANCE_TREE_LEAF_MAX = 8;

// the number of nodes of the tree over n placements (n >= 1): at most 2 n - 1
inline size_t instance_tree_nodes(size_t n, int32_t leaf_size)
{
    std::vector<int32_t> skip, first, count;
    int32_t depth = 0;
    morton_topology(n, leaf_size, skip, first, count, depth);
    return skip.size();
}

// The order and the boxes of the tree whose topology (node_skip, node_first, node_count: morton_topology(n, leaf_size), nn nodes)
// stands.  The world box of instance j is the six doubles (lo, hi) at wbox + j * stride.  Writes inst_order [n] and node_box
// [nn][6]; allocates nothing (the pending ranges lie on a stack of BVH_MAX_DEPTH + 2 entries, as in build_bvh).
inline void instance_tree_fit(const double *wbox, size_t stride, size_t n, const int32_t *node_skip, const int32_t *node_first,
                              const int32_t *node_count, size_t nn, int32_t *inst_order, double *node_box)
{
    for (size_t j = 0; j < n; j++) inst_order[j] = (int32_t)j;
    const auto centre = [&](int32_t j, int c) { return 0.5 * (wbox[(size_t)j * stride + c] + wbox[(size_t)j * stride + 3 + c]); };
    struct Range {
        size_t node, lo, hi;
    };
    Range stack[BVH_MAX_DEPTH + 2];
    int sp = 0;
    stack[sp++] = Range{0, 0, n};
    while (sp > 0) {
        const Range r = stack[--sp];
        if (node_count[r.node] > 0) {
            // (the slots of a leaf in the caller's order, as build_bvh leaves them)
            std::sort(inst_order + r.lo, inst_order + r.hi);
            continue;
        }
        double lo[3], hi[3];
        for (int c = 0; c < 3; c++) lo[c] = hi[c] = centre(inst_order[r.lo], c);
        for (size_t k = r.lo + 1; k < r.hi; k++)
            for (int c = 0; c < 3; c++) {
                const double x = centre(inst_order[k], c);
                lo[c] = std::min(lo[c], x);
                hi[c] = std::max(hi[c], x);
            }
        int axis = 0;
        for (int c = 1; c < 3; c++)
            if (hi[c] - lo[c] > hi[axis] - lo[axis]) axis = c;
        const size_t mid = r.lo + (r.hi - r.lo) / 2;
        std::nth_element(inst_order + r.lo, inst_order + mid, inst_order + r.hi, [&](int32_t a, int32_t b) {
            const double xa = centre(a, axis), xb = centre(b, axis);
            return xa < xb || (xa == xb && a < b);
        });
        // the left child is the next node, the right one where the left one's subtree ends
        stack[sp++] = Range{(size_t)node_skip[r.node + 1], mid, r.hi};
        stack[sp++] = Range{r.node + 1, r.lo, mid};
    }
    // the boxes, children before parents (pre-order: every child has a larger index than its parent)
    for (size_t i = nn; i-- > 0;) {
        double *b = node_box + i * 6;
        if (node_count[i] > 0) {
            const double *w = wbox + (size_t)inst_order[(size_t)node_first[i]] * stride;
            for (int c = 0; c < 6; c++) b[c] = w[c];
            for (int32_t k = 1; k < node_count[i]; k++) {
                w = wbox + (size_t)inst_order[(size_t)node_first[i] + k] * stride;
                for (int c = 0; c < 3; c++) {
                    b[c] = std::min(b[c], w[c]);
                    b[3 + c] = std::max(b[3 + c], w[3 + c]);
                }
            }
        } else {
            const double *l = node_box + (i + 1) * 6, *r = node_box + (size_t)node_skip[i + 1] * 6;
            for (int c = 0; c < 3; c++) {
                b[c] = std::min(l[c], r[c]);
                b[3 + c] = std::max(l[3 + c], r[3 + c]);
            }
        }
    }
}

}  // namespace bhg

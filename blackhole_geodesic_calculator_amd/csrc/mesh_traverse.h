// mesh_traverse.h -- segment against the flattened BVH of mesh_bvh.h, on the device.  One function for
// the mesh trace's sub-chords (first hit) and the mesh shade's shadow rays (any hit), and its form over K rigid placements of
// the one tree, walked one after the other or under a tree of their world boxes (section 24).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bhg {

// the device's view of a bhg_mesh: the tree, the triangles in leaf order and the maps between leaf order and the caller's
struct MeshView {
    const double *node_box;      // [n_nodes][6]: lo, hi (widened at build time)
    const int32_t *node_skip;    // [n_nodes]
    const int32_t *node_first;   // [n_nodes]: first leaf slot, -1 for an inner node
    const int32_t *node_count;   // [n_nodes]: triangles of a leaf, 0 for an inner node
    const double *tri;           // [nt][9]: v0, e1 = v1 - v0, e2 = v2 - v0 of the triangle in each leaf slot
    const int32_t *tri_order;    // [nt]: leaf slot -> the caller's triangle
    const int32_t *tri_slot;     // [nt]: the caller's triangle -> leaf slot
    const double *tri_normals;   // nullptr, or [nt][9]: the vertex normals N0, N1, N2 of the triangle in each leaf slot
    int32_t n_nodes, n_tris;
};

// Does the segment p + s d, 0 <= s <= s_max, meet the box?  The slab test with a relative slack on every comparison: the
// boxes are widened by ulps, the quotients here are rounded, and a rejection must be certain.
__device__ __forceinline__ bool segment_meets_box(const double *b, const double p[3], const double d[3], double s_max)
{
    double t_near = 0.0, t_far = s_max;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (d[c] == 0.0) {
            if (p[c] < b[c] || p[c] > b[3 + c]) return false;
        } else {
            const double inv = 1.0 / d[c];
            const double t1 = (b[c] - p[c]) * inv, t2 = (b[3 + c] - p[c]) * inv;
            t_near = fmax(t_near, fmin(t1, t2));
            t_far = fmin(t_far, fmax(t1, t2));
        }
    }
    return t_near <= t_far + 1e-10 * (1.0 + fabs(t_near) + fabs(t_far));
}

// Moeller-Trumbore on the segment p + s d against the triangle (v0, e1, e2): two-sided, a zero determinant is no hit
__device__ __forceinline__ bool segment_meets_triangle(const double *T, const double p[3], const double d[3], double &s, double &u,
                                                       double &v)
{
    const double *v0 = T, *e1 = T + 3, *e2 = T + 6;
    const double pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const double tv[3] = {p[0] - v0[0], p[1] - v0[1], p[2] - v0[2]};
    u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
    const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
    s = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && s >= 0.0 && s <= 1.0;
}

// The segment p -> q against the tree.  First hit (ANY = false): the smallest s wins, a tie goes to the smaller index of the
// caller's numbering -- whatever the tree's shape, so a box is only skipped when it starts behind the best s so far.  Returns
// the caller's triangle (s in s_hit), or -1.  ANY = true: returns the first triangle met in traversal order, or -1.
template <bool ANY>
__device__ __forceinline__ int32_t segment_first_hit(const MeshView &M, const double p[3], const double q[3], double &s_hit)
{
    const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    double best = 1.0;
    int32_t best_tri = -1;
    for (int32_t i = 0; i < M.n_nodes;) {
        if (!segment_meets_box(M.node_box + (size_t)i * 6, p, d, best)) {
            i = M.node_skip[i];
            continue;
        }
        const int32_t cnt = M.node_count[i], first = M.node_first[i];
        for (int32_t k = 0; k < cnt; k++) {
            double s, u, v;
            if (!segment_meets_triangle(M.tri + (size_t)(first + k) * 9, p, d, s, u, v)) continue;
            const int32_t id = M.tri_order[first + k];
            if (ANY) {
                s_hit = s;
                return id;
            }
            if (best_tri < 0 || s < best || (s == best && id < best_tri)) {
                best = s;
                best_tri = id;
            }
        }
        i++;
    }
    s_hit = best;
    return best_tri;
}

// ---- K rigid placements of the tree --------------------------------------------------------------------
// Instance j is rec[j]: R row-major, t, then its world box lo, hi (x_world = R x_local + t).  The records do not change during
// a launch and are read through the constant address space: where j is uniform over the wave they come by scalar loads, into
// SGPRs.  That is why the walk below has no early way out: every lane goes through j = 0 .. n - 1, and skips inside it.
constexpr int BHG_MESH_INSTANCE_DOUBLES_ = 18;
typedef const double __attribute__((address_space(4))) *InstanceRecords;

// p' = R^T (p - t): c in the world, l in the frame of the instance whose record starts at r
template <class Rec>
__device__ __forceinline__ void instance_into_frame(Rec r, const double c[3], double l[3])
{
    const double w[3] = {c[0] - r[9], c[1] - r[10], c[2] - r[11]};
    l[0] = r[0] * w[0] + r[3] * w[1] + r[6] * w[2];
    l[1] = r[1] * w[0] + r[4] * w[1] + r[7] * w[2];
    l[2] = r[2] * w[0] + r[5] * w[1] + r[8] * w[2];
}

// n = R m: a direction of the instance's frame in the world
template <class Rec>
__device__ __forceinline__ void instance_rotate_out(Rec r, const double m[3], double n[3])
{
    n[0] = r[0] * m[0] + r[1] * m[1] + r[2] * m[2];
    n[1] = r[3] * m[0] + r[4] * m[1] + r[5] * m[2];
    n[2] = r[6] * m[0] + r[7] * m[1] + r[8] * m[2];
}

// The segment p -> q in the world against every placement, in index order.  A placement's world box is met before the segment
// is taken into its frame, where segment_first_hit runs against the one tree; the chord parameter is the same in both frames.
// First hit (ANY = false): the smallest s wins, a tie goes to the smaller instance (a later one must be strictly nearer), then to
// the smaller triangle.  ANY = true: is any triangle of any placement met at all (the first placement that says so is kept).
// Returns the caller's triangle within the mesh (s in s_hit, the placement in inst), or -1.  boxes = false: no world box is
// looked at, every placement is walked (BHGEO_MESH_CULL=0: the same results).
template <bool ANY>
__device__ __forceinline__ int32_t segment_first_hit_instances(const MeshView &M, const double *records, int32_t n, bool boxes,
                                                               const double p[3], const double q[3], double &s_hit, int32_t &inst)
{
    const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    const InstanceRecords rec = (InstanceRecords)(uintptr_t)records;
    double best = 1.0;
    int32_t best_tri = -1;
    for (int32_t j = 0; j < n; j++) {
        double r[BHG_MESH_INSTANCE_DOUBLES_];
#pragma unroll
        for (int k = 0; k < BHG_MESH_INSTANCE_DOUBLES_; k++) r[k] = rec[(size_t)j * BHG_MESH_INSTANCE_DOUBLES_ + k];
        if (ANY && best_tri >= 0) continue;
        if (boxes && !segment_meets_box(r + 12, p, d, best)) continue;
        double lp[3], lq[3], s;
        instance_into_frame(r, p, lp);
        instance_into_frame(r, q, lq);
        const int32_t hit = segment_first_hit<ANY>(M, lp, lq, s);
        if (hit >= 0 && (best_tri < 0 || s < best)) {
            best = s;
            best_tri = hit;
            inst = j;
        }
    }
    s_hit = best;
    return best_tri;
}

// ---- ... under a tree of boxes ---------------------------------------------------------------------------
// The placements of an instance set under the tree of instance_tree.h: the records as above, in the caller's order, and over them
// nodes in pre-order with one skip link each, whose leaves hold first and count into inst_order[], the caller's instance indices.
struct InstanceTreeView {
    const double *rec;           // [n][BHG_MESH_INSTANCE_DOUBLES_]
    const double *node_box;      // [n_nodes][6]: the exact union of the world boxes below
    const int32_t *node_skip;    // [n_nodes]
    const int32_t *node_first;   // [n_nodes]: first slot of inst_order, -1 for an inner node
    const int32_t *node_count;   // [n_nodes]: placements of a leaf, 0 for an inner node
    const int32_t *inst_order;   // [n]: leaf slot -> the caller's instance
    int32_t n_nodes, n;
};

// The segment p -> q in the world against the placements under the tree: a stackless walk by skip links, as segment_first_hit
// walks the mesh's own tree.  A node's box is tested with the best s so far, so it is skipped only when it starts behind that s
// (the test's own slack keeps ties in); at a leaf each placement's own world box comes first -- its six doubles are read, R and t
// only once the box is met -- and then the segment goes into the placement's frame and against the one tree.
// First hit (ANY = false): the smallest s wins, then the smaller instance, then the smaller triangle -- section 21's rule, stated
// without reference to the order of the visit, which here is the tree's and not the caller's: a hit at the same s replaces the
// best one when its instance is the smaller.  ANY = true: returns at the first hit met.
// Unlike the linear walk, the placement j in hand differs from lane to lane: the records are read with ordinary (vector) loads,
// and the constant address space of the linear walk -- scalar loads of a wave-uniform record -- does not apply.  In exchange a
// lane is free to leave early and to skip what its own segment misses.
// boxes = false: no box is looked at, of the tree's or of a placement, and every placement is walked (BHGEO_MESH_CULL=0).
template <bool ANY>
__device__ __forceinline__ int32_t segment_first_hit_instance_tree(const MeshView &M, const InstanceTreeView &U, bool boxes,
                                                                   const double p[3], const double q[3], double &s_hit, int32_t &inst)
{
    const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    double best = 1.0;
    int32_t best_tri = -1;
    for (int32_t i = 0; i < U.n_nodes;) {
        if (boxes && !segment_meets_box(U.node_box + (size_t)i * 6, p, d, best)) {
            i = U.node_skip[i];
            continue;
        }
        const int32_t cnt = U.node_count[i], first = U.node_first[i];
        for (int32_t k = 0; k < cnt; k++) {
            const int32_t j = U.inst_order[first + k];
            const double *r = U.rec + (size_t)j * BHG_MESH_INSTANCE_DOUBLES_;
            if (boxes) {
                double wb[6];
#pragma unroll
                for (int c = 0; c < 6; c++) wb[c] = r[12 + c];
                if (!segment_meets_box(wb, p, d, best)) continue;
            }
            double lp[3], lq[3], s;
            instance_into_frame(r, p, lp);
            instance_into_frame(r, q, lq);
            const int32_t hit = segment_first_hit<ANY>(M, lp, lq, s);
            if (hit < 0) continue;
            if (ANY) {
                s_hit = s;
                inst = j;
                return hit;
            }
            if (best_tri < 0 || s < best || (s == best && j < inst)) {
                best = s;
                best_tri = hit;
                inst = j;
            }
        }
        i++;
    }
    s_hit = best;
    return best_tri;
}

}  // namespace bhg

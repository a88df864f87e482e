// mesh_refit.hip -- the refit kernels: new vertices into a tree whose topology stands.
//
// Everything here restates a host loop, operation for operation, so that the device leaves the bits the host would:
//   slot records   bhg_mesh_create's v0, v1 - v0, v2 - v0 and N0, N1, N2 per leaf slot (bhgeo_mesh.hip);
//   boxes          fit_boxes of mesh_bvh.h: std::min(b, x) is written out as (x < b ? x : b) and std::max(b, x) as (b < x ? x : b),
//                  which also settles which zero survives when -0.0 meets +0.0;
//   area sum       area_sum of mesh_bvh.h: BVH_AREA_LANES strided partial sums, then a halving tree.
// The unit is compiled with -ffp-contract=off like the host code: no product here is fused into a sum.
//
// No kernel waits for another workgroup.  Children come before parents either by the order of the launches on one stream (one
// launch per level, deepest first) or, for a tree small enough, by barriers inside the one workgroup that walks all levels.
#include "mesh_refit.h"

namespace bhg {

namespace {

constexpr int REFIT_BLOCK = 256;

__device__ __forceinline__ double min_as_host(double b, double x) { return x < b ? x : b; }   // std::min(b, x)
__device__ __forceinline__ double max_as_host(double b, double x) { return b < x ? x : b; }   // std::max(b, x)

// a grid-stride scan of n doubles: one atomic per workgroup that saw a non-finite value
__global__ __launch_bounds__(REFIT_BLOCK) void refit_scan_kernel(const double *__restrict__ x, uint64_t n, uint32_t bit,
                                                                  MeshRefitSummary *__restrict__ summary)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * REFIT_BLOCK)
        bad |= !(fabs(x[i]) < INFINITY);
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&summary->nonfinite, bit);
}

// One thread per double of the slot records: thread g writes tri[g] (and tri_normals[g]), g = slot * 9 + j * 3 + c, so that a wave
// writes 512 consecutive bytes; the vertex reads are gathers, and the nine threads of a slot share their three cache lines.
// The threads with c = 0 also form |v_j|^2 of their vertex, as the host forms it under its square root, for d_max.
__global__ __launch_bounds__(REFIT_BLOCK) void refit_triangles_kernel(MeshRefitArgs a)
{
    __shared__ unsigned long long far2;
    if (threadIdx.x == 0) far2 = 0ull;
    __syncthreads();
    const uint64_t g = (uint64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (g < (uint64_t)a.n_tris * 9) {
        const uint64_t slot = g / 9;
        const int q = (int)(g - slot * 9), j = q / 3, c = q - j * 3;
        const int32_t *iv = a.slot_vert + slot * 3;
        const size_t i0 = (size_t)iv[0], ij = (size_t)iv[j];
        const double x0 = a.vertices[i0 * 3 + c], xj = a.vertices[ij * 3 + c];
        a.tri[g] = j == 0 ? x0 : xj - x0;
        if (a.tri_normals) a.tri_normals[g] = a.normals[ij * 3 + c];
        if (c == 0) {
            const double y = a.vertices[ij * 3 + 1], z = a.vertices[ij * 3 + 2];
            const double d2 = xj * xj + y * y + z * z;
            atomicMax(&far2, (unsigned long long)__double_as_longlong(d2));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && far2) atomicMax(&a.summary->d2_max, far2);
}

// One thread per node; a leaf's thread walks its slots in order (fit_boxes' loop: triangle, corner, coordinate).
__global__ __launch_bounds__(REFIT_BLOCK) void refit_leaf_boxes_kernel(MeshRefitArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (i >= a.n_nodes) return;
    const int32_t count = a.node_count[i];
    if (count <= 0) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const int32_t *iv = a.slot_vert + (size_t)a.node_first[i] * 3;
    for (int32_t k = 0; k < count * 3; k++) {
        const double *v = a.vertices + (size_t)iv[k] * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = min_as_host(lo[c], v[c]);
            hi[c] = max_as_host(hi[c], v[c]);
        }
    }
    double *b = a.node_box + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        b[c] = lo[c];
        b[3 + c] = hi[c];
    }
}

__device__ __forceinline__ void unite_children(const MeshRefitArgs &a, int32_t i)
{
    const size_t l = (size_t)i + 1, r = (size_t)a.node_skip[l];
    const double *bl = a.node_box + l * 6, *br = a.node_box + r * 6;
    double *b = a.node_box + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        b[c] = min_as_host(bl[c], br[c]);
        b[3 + c] = max_as_host(bl[3 + c], br[3 + c]);
    }
}

// the inner nodes of one level, one thread each: its children lie on deeper levels, written by earlier launches
__global__ __launch_bounds__(REFIT_BLOCK) void refit_level_kernel(MeshRefitArgs a, int32_t first, int32_t end)
{
    const int64_t t = (int64_t)first + (int64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (t < end) unite_children(a, a.level_nodes[t]);
}

// every level in one workgroup, deepest first, a barrier between levels (it also orders the block's global writes and reads)
__global__ __launch_bounds__(REFIT_BLOCK) void refit_levels_one_group_kernel(MeshRefitArgs a)
{
    for (int d = BVH_MAX_DEPTH; d >= 0; d--) {
        const int32_t first = a.level_off[d], end = a.level_off[d + 1];
        if (first == end) continue;      // (uniform over the workgroup: every thread skips the same barriers)
        for (int32_t t = first + (int32_t)threadIdx.x; t < end; t += REFIT_BLOCK) unite_children(a, a.level_nodes[t]);
        __syncthreads();
    }
}

// widen every box by the builder's rule, after all unions as the builder does; keep its area; the root's goes to the summary
__global__ __launch_bounds__(REFIT_BLOCK) void refit_widen_kernel(MeshRefitArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * REFIT_BLOCK + threadIdx.x;
    if (i >= a.n_nodes) return;
    double *p = a.node_box + (size_t)i * 6;
    double b[6];
    double mag = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        b[c] = p[c];
        mag = max_as_host(mag, fabs(b[c]));
    }
    const double w = BVH_BOX_ULPS * 2.220446049250313e-16 * max_as_host(mag, 2.2250738585072014e-308);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        b[c] -= w;
        b[3 + c] += w;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) p[c] = b[c];
    const double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    a.area[i] = dx * dy + dy * dz + dz * dx;
    if (i == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) a.summary->box[c] = b[c];
    }
}

// area_sum's order: one workgroup of BVH_AREA_LANES threads, whatever the tree's size
__global__ __launch_bounds__(BVH_AREA_LANES) void refit_area_kernel(MeshRefitArgs a)
{
    __shared__ double lane[BVH_AREA_LANES];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.n_nodes; i += BVH_AREA_LANES) acc += a.area[i];
    lane[threadIdx.x] = acc;
    __syncthreads();
    for (int s = BVH_AREA_LANES / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lane[threadIdx.x] += lane[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.summary->area = lane[0];
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + REFIT_BLOCK - 1) / REFIT_BLOCK); }

}  // namespace

hipError_t launch_mesh_refit_scan(const MeshRefitArgs &a, hipStream_t s)
{
    const uint64_t n = (uint64_t)a.n_vertices * 3;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks_for(n), 2048);
    hipLaunchKernelGGL(refit_scan_kernel, dim3(grid), dim3(REFIT_BLOCK), 0, s, a.vertices, n, 1u, a.summary);
    if (a.normals) hipLaunchKernelGGL(refit_scan_kernel, dim3(grid), dim3(REFIT_BLOCK), 0, s, a.normals, n, 2u, a.summary);
    return hipGetLastError();
}

hipError_t launch_mesh_refit(const MeshRefitArgs &a, hipStream_t s)
{
    // (n_tris * 9 / 256 blocks: below 2^31 for every mesh the library takes)
    hipLaunchKernelGGL(refit_triangles_kernel, dim3(blocks_for((uint64_t)a.n_tris * 9)), dim3(REFIT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(refit_leaf_boxes_kernel, dim3(blocks_for((uint64_t)a.n_nodes)), dim3(REFIT_BLOCK), 0, s, a);
    if (a.n_inner > 0 && a.n_inner <= MESH_REFIT_ONE_GROUP_NODES) {
        hipLaunchKernelGGL(refit_levels_one_group_kernel, dim3(1), dim3(REFIT_BLOCK), 0, s, a);
    } else if (a.n_inner > 0) {
        for (int d = BVH_MAX_DEPTH; d >= 0; d--) {
            const int32_t first = a.level_off[d], end = a.level_off[d + 1];
            if (first == end) continue;
            hipLaunchKernelGGL(refit_level_kernel, dim3(blocks_for((uint64_t)(end - first))), dim3(REFIT_BLOCK), 0, s, a, first, end);
        }
    }
    hipLaunchKernelGGL(refit_widen_kernel, dim3(blocks_for((uint64_t)a.n_nodes)), dim3(REFIT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(refit_area_kernel, dim3(1), dim3(BVH_AREA_LANES), 0, s, a);
    return hipGetLastError();
}

}  // namespace bhg

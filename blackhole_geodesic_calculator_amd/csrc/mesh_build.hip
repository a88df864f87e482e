// mesh_build.hip -- the build kernels: a Morton-order tree over a triangle list that lies on the device.
//
// The order and topology are stated once, in mesh_bvh.h (build_bvh_morton); everything here restates a host expression, operation
// for operation, so that the device leaves the bits the host would:
//   centroid       (x0 + x1 + x2) / 3.0, left to right (the unit is compiled with -ffp-contract=off like the host code);
//   bounds         the exact min / max of the centroids: no order of reduction changes them;
//   cell, key      morton_cell and morton_key of mesh_bvh.h, which are plain integer and double C++ and compile for the device;
//   order          a stable radix sort of (key, caller's index) pairs: the order is unique, so any correct sort gives it;
//   leaf order     the slots of every leaf in rising caller index.
// The topology (node_skip, node_first, node_count, the refit's levels) is a function of (n_triangles, leaf_size) alone: the host
// writes it in O(n_nodes) and uploads it when either changed.  Slot records, boxes, widening, area and summary are the refit's
// kernels (mesh_refit.hip), launched by the caller after these.
//
// The scan comes first and alone: launch_mesh_build gathers vertices through triangle indices, so the caller reads the scan's
// result back and launches it only for a clean triangle array.
#include "mesh_build.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace bhg {

namespace {

constexpr int BUILD_BLOCK = 256;
constexpr int BUILD_WAVES = BUILD_BLOCK / 64;

// the bits of a double as an unsigned integer that orders as the doubles do (-0.0 below +0.0, which no cell can tell apart)
__device__ __forceinline__ unsigned long long ordered_bits(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_bits(unsigned long long u)
{
    const unsigned long long b = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
    return __longlong_as_double((long long)b);
}

// a grid-stride scan of the n indices: one atomic per workgroup that saw one outside [0, nv)
__global__ __launch_bounds__(BUILD_BLOCK) void build_scan_kernel(const int32_t *__restrict__ f, uint64_t n, int32_t nv,
                                                                  MeshBuildRecord *__restrict__ record)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BUILD_BLOCK)
        bad |= (uint32_t)f[i] >= (uint32_t)nv;      // (a negative index is a large unsigned one)
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&record->bad_index, 1u);
}

__device__ __forceinline__ double centroid(const MeshBuildArgs &a, const int32_t *iv, int c)
{
    return (a.vertices[(size_t)iv[0] * 3 + c] + a.vertices[(size_t)iv[1] * 3 + c] + a.vertices[(size_t)iv[2] * 3 + c]) / 3.0;
}

// the centroid bounds: grid-stride over the triangles, wave shuffles, LDS across the waves, six atomics per workgroup
__global__ __launch_bounds__(BUILD_BLOCK) void build_bounds_kernel(MeshBuildArgs a)
{
    __shared__ double part[BUILD_WAVES][6];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t t = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x; t < a.n_tris; t += (int64_t)gridDim.x * BUILD_BLOCK) {
        const int32_t *iv = a.triangles + (size_t)t * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double x = centroid(a, iv, c);
            lo[c] = x < lo[c] ? x : lo[c];
            hi[c] = hi[c] < x ? x : hi[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
        for (int off = 32; off > 0; off >>= 1) {
            const double l = __shfl_down(lo[c], off), h = __shfl_down(hi[c], off);
            lo[c] = l < lo[c] ? l : lo[c];
            hi[c] = hi[c] < h ? h : hi[c];
        }
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            part[wave][c] = lo[c];
            part[wave][3 + c] = hi[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        double v = part[0][c];
        for (int w = 1; w < BUILD_WAVES; w++) {
            const double x = part[w][c];
            v = c < 3 ? (x < v ? x : v) : (v < x ? x : v);
        }
        // (a workgroup beyond the triangles holds +-inf: the start values, which change nothing)
        if (c < 3) atomicMax(&a.record->lo[c], ~ordered_bits(v));
        else atomicMax(&a.record->hi[c - 3], ordered_bits(v));
    }
}

// one thread per triangle: its key and its own index as the value
__global__ __launch_bounds__(BUILD_BLOCK) void build_keys_kernel(MeshBuildArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
    if (t >= a.n_tris) return;
    const int32_t *iv = a.triangles + (size_t)t * 3;
    uint64_t q[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lo = from_ordered_bits(~a.record->lo[c]), hi = from_ordered_bits(a.record->hi[c]);
        q[c] = morton_cell(centroid(a, iv, c), lo, morton_scale(lo, hi));
    }
    a.keys_in[t] = morton_key(q[0], q[1], q[2]);
    a.vals_in[t] = (int32_t)t;
}

// One thread per node; a leaf's thread puts its slots (at most MORTON_LEAF_MAX, its own alone) in rising caller index by an
// insertion sort in place: the sort left them in key order, ties rising, so most leaves are nearly sorted already.
__global__ __launch_bounds__(BUILD_BLOCK) void build_leaf_order_kernel(MeshBuildArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
    if (i >= a.n_nodes) return;
    const int32_t count = a.node_count[i];
    if (count <= 1) return;
    int32_t *o = a.tri_order + (size_t)a.node_first[i];
    for (int32_t k = 1; k < count; k++) {
        const int32_t x = o[k];
        int32_t j = k;
        while (j > 0 && o[j - 1] > x) {
            o[j] = o[j - 1];
            j--;
        }
        o[j] = x;
    }
}

// one thread per slot: the inverse map and the caller's vertex indices of the slot's triangle
__global__ __launch_bounds__(BUILD_BLOCK) void build_maps_kernel(MeshBuildArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
    if (k >= a.n_tris) return;
    const int32_t f = a.tri_order[k];
    a.tri_slot[f] = (int32_t)k;
    const int32_t *iv = a.triangles + (size_t)f * 3;
#pragma unroll
    for (int j = 0; j < 3; j++) a.slot_vert[(size_t)k * 3 + j] = iv[j];
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + BUILD_BLOCK - 1) / BUILD_BLOCK); }

// rocPRIM's own choice for the onesweep pass of (64-bit key, 32-bit value) pairs -- 256 threads of 15 items -- spills 80 bytes a
// lane on gfx950, and eight items at 4 radix bits a pass still 48; eight items a thread at 8 bits a pass use none (131 KB of LDS, one
// workgroup a CU: the pass runs only above rocPRIM's merge-sort limit of 2^20 pairs; the other passes are rocPRIM's defaults)
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                              rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 8>, 8>>;

hipError_t sort_pairs(void *temp, size_t &bytes, const MeshBuildArgs &a, size_t n, hipStream_t s)
{
    // 63 key bits; stable, so equal keys stay in rising caller index
    return rocprim::radix_sort_pairs<SortConfig>(temp, bytes, a.keys_in, a.keys_out, a.vals_in, a.tri_order, n, 0u, 63u, s);
}

}  // namespace

hipError_t mesh_build_sort_bytes(size_t n, size_t *bytes)
{
    MeshBuildArgs a{};
    *bytes = 0;
    return sort_pairs(nullptr, *bytes, a, n, nullptr);
}

hipError_t launch_mesh_build_scan(const MeshBuildArgs &a, hipStream_t s)
{
    const uint64_t n = (uint64_t)a.n_tris * 3;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks_for(n), 2048);
    hipLaunchKernelGGL(build_scan_kernel, dim3(grid), dim3(BUILD_BLOCK), 0, s, a.triangles, n, a.n_vertices, a.record);
    return hipGetLastError();
}

hipError_t launch_mesh_build(const MeshBuildArgs &a, hipStream_t s)
{
    const uint64_t nt = (uint64_t)a.n_tris;
    const unsigned bounds_grid = (unsigned)std::min<uint64_t>(blocks_for(nt), 1024);
    hipLaunchKernelGGL(build_bounds_kernel, dim3(bounds_grid), dim3(BUILD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(build_keys_kernel, dim3(blocks_for(nt)), dim3(BUILD_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = a.sort_temp_bytes;
    e = sort_pairs(a.sort_temp, bytes, a, (size_t)nt, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(build_leaf_order_kernel, dim3(blocks_for((uint64_t)a.n_nodes)), dim3(BUILD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(build_maps_kernel, dim3(blocks_for(nt)), dim3(BUILD_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace bhg

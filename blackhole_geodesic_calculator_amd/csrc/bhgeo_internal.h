// bhgeo_internal.h -- what the translation units of the C layer (bhgeo_capi.hip, bhgeo_mesh.hip, bhgeo_frame.hip) share: how an
// entry point fails, how it makes its device current, and the functions one unit offers another, each declared once.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/bhgeo.h"
#include "geodesic_kernels.h"

namespace bhg {

// --- bhgeo_capi.hip ---
int set_error(int code, const std::string &msg);   // sets the thread-local message of bhg_last_error(), returns code
// a context's worker threads: a multi-threaded memcpy in jobs of `piece` bytes
void host_copy(bhg_context *c, void *dst, const void *src, size_t bytes, size_t piece);
// redshift settings checked against the trace parameters (disk_r_in < 0: no disk to check)
int redshift_params(const bhg_params *p, const bhg_redshift *rs, double disk_r_in, const double *x0, RedshiftParams *out);
// observer settings checked against the trace parameters and the camera
int observer_params(const bhg_params *p, const bhg_observer *obs, const double *x0, ObserverParams *out);
// object textures checked against a scene of n_spheres spheres
int object_texture_params(const bhg_object_textures *ot, int32_t n_spheres, ObjectTextureParams *out);
// the thermal-disk settings and object motion: on their own, and against the trace parameters, the scene and the camera
int thermal_check(const bhg_disk_thermal *th);
int thermal_params(const bhg_params *p, const bhg_disk_thermal *th, const bhg_redshift *rs, const bhg_polarisation *pol,
                   double disk_r_in, const double *x0, ThermalParams *out, RedshiftParams *rp);
int motion_check(const bhg_object_motion *mo, int32_t n_spheres);
int motion_params(const bhg_params *p, const bhg_object_motion *mo, const double *spheres, int32_t n_spheres, MotionParams *out);
// a mesh material for nt triangles (host_arrays: tri_uv / tri_tex are host arrays and are scanned)
int mesh_material_check(const bhg_mesh_material *m, size_t nt, bool host_arrays);

// --- bhgeo_mesh.hip ---
// the transforms of mesh instances: n rigid ones, or the reason they are refused
int mesh_instance_transforms_check(int32_t n, const double *T);
// ... of a set under a tree: n within BHG_MESH_INSTANCE_TREE_MAX, leaf_size within [1, 8], then as above
int mesh_instance_tree_check(int32_t n, const double *T, int32_t leaf_size);
// a mesh built on the device; host_arrays: from host arrays, which are uploaded first
int mesh_create_built_on_device(bhg_context *c, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                                const double *vertex_normals, int32_t leaf_size, size_t cap_vertices, size_t cap_triangles,
                                bool host_arrays, hipStream_t stream, bhg_mesh **out);

// (what follows is new with the units' common header and stays inside the library)
#pragma GCC visibility push(hidden)
// --- bhgeo_capi.hip ---
int params_check(const bhg_params *p);             // the trace parameters, as every trace call checks them first
int context_device(const bhg_context *c);
hipStream_t context_stream(const bhg_context *c);
// --- bhgeo_mesh.hip ---
// n3 doubles of host vertices and of host vertex normals, either of which may be NULL (not given, or looked at already)
int mesh_finite_check(const double *vertices, const double *vertex_normals, size_t n3);
#pragma GCC visibility pop

}  // namespace bhg

namespace {

int fail(int code, const std::string &msg) { return bhg::set_error(code, msg); }

int fail_hip(hipError_t e, const char *what)
{
    const int rc = bhg::set_error(e == hipErrorOutOfMemory ? BHG_E_NOMEM : BHG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    (void)hipGetLastError();     // (reported here: not again by the next launch's status)
    return rc;
}

#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t _e = (expr);                           \
        if (_e != hipSuccess) return fail_hip(_e, #expr); \
    } while (0)
// ... and a refusal or failure of one of the library's own checks and calls: handed on as it is
#define BHG_TRY(expr)                      \
    do {                                   \
        const int _rc = (expr);            \
        if (_rc != BHG_OK) return _rc;     \
    } while (0)

// Entry points make the context's device current for their own HIP calls and put the caller's current device back on
// the way out: a host that created a context on device k while working on device j keeps working on j.  Without a device (the
// frame's entry points, which walk over several and set each where its work is queued) the guard only puts the caller's back.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    DeviceGuard()
    {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
    }
    explicit DeviceGuard(int dev) : DeviceGuard()
    {
        if (prev != dev) err = hipSetDevice(dev);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define ENTER_DEVICE(dev)         \
    DeviceGuard _device_guard(dev); \
    if (_device_guard.err != hipSuccess) return fail_hip(_device_guard.err, "hipSetDevice")

}  // namespace

// geodesic_kernels.h -- internal interface between the C-ABI layer (bhgeo_capi.hip and its units) and the
// gfx950 kernels (geodesic_kernels.hip).  Not installed; the public surface is include/bhgeo.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_traverse.h"

// Every launcher returns hipGetLastError() as THIS launch's status.  That call reports -- and clears -- the last error any
// earlier HIP call of the thread left behind, ours (a refused allocation) or another library's (a probing
// hipPointerGetAttributes): it is read away before the launch, so that a launch that went through is not reported
// with somebody else's error.
#define BHG_LAUNCH(...)                    \
    do {                                   \
        (void)hipGetLastError();           \
        hipLaunchKernelGGL(__VA_ARGS__);   \
    } while (0)

namespace bhg {

// mirrors of the public constants (include/bhgeo.h); static_asserts in bhgeo_capi.hip tie them
constexpr uint32_t BHG_FLAG_HIT_HORIZON_ = 1u;
constexpr uint32_t BHG_FLAG_START_INSIDE_ = 2u;
constexpr uint32_t BHG_FLAG_REACHED_END_ = 4u;
constexpr uint32_t BHG_FLAG_EXITED_SPHERE_ = 8u;
constexpr uint32_t BHG_FLAG_MAX_STEPS_ = 16u;
constexpr uint32_t BHG_FLAG_STEP_TOO_SMALL_ = 32u;
constexpr uint32_t BHG_FLAG_NAN_ = 64u;
constexpr uint32_t BHG_FLAG_HIT_DISK_ = 128u;
constexpr uint32_t BHG_FLAG_HIT_OBJECT_ = 0x88u;
constexpr int BHG_MAX_SPHERES_ = 8;
constexpr int BHG_MAX_CROSSINGS_ = 4;
constexpr int32_t BHG_OBJECT_LIT_ = 0;
constexpr int32_t BHG_OBJECT_EMISSIVE_ = 1;
constexpr int BHG_MESH_TEXTURES_MAX_ = 8;
constexpr uint32_t BHG_REDSHIFT_DISK_ = 1u;
constexpr uint32_t BHG_REDSHIFT_OBJECTS_ = 2u;
constexpr uint32_t BHG_REDSHIFT_SKY_ = 4u;
constexpr int BHG_METHOD_DP54_ = 0;
constexpr int BHG_METHOD_RK4_ = 1;
constexpr int BHG_RHS_CHRISTOFFEL_ = 0;
constexpr int BHG_RHS_REDUCED_ = 1;
constexpr int BHG_RHS_CHRISTOFFEL_TL_ = 3;   // internal: the Christoffel form with g(k, k) = -1 (bhg_params.time_like), own translation unit
constexpr int BHG_RHS_KERR_BL_ = 2;
constexpr int32_t BHG_START_NONE_ = 0;      // TraceArgs::start_mode: every call works its rays' initial steps out
constexpr int32_t BHG_START_RECORD_ = 1;    // ... and stores them in start_h
constexpr int32_t BHG_START_REPLAY_ = 2;    // start_h holds them (a recording call on the same rays and matching parameters)
constexpr int BHG_PREFIX_K_MAX_ = 4;        // accepted steps a start-up record holds at most (BHG_PREFIX_K_MAX)
constexpr int BHG_PREFIX_DEEP_ACCEPTED_ = 6;    // ... a DEEP record: accepted steps at most (BHG_PREFIX_DEEP_ACCEPTED)
constexpr int BHG_PREFIX_DEEP_ATTEMPTS_ = 12;   // ... and attempts, the rejected ones among them (BHG_PREFIX_DEEP_ATTEMPTS)
constexpr int BHG_PREFIX_WIDE_ACCEPTED_ = 8;    // ... a WIDE record: accepted steps at most, in the same attempts (BHG_PREFIX_WIDE_ACCEPTED)
constexpr int BHG_PREFIX_RIM_ACCEPTED_ = 9;     // ... a RIM record: accepted steps at most (BHG_PREFIX_RIM_ACCEPTED)
constexpr int BHG_PREFIX_RIM_ATTEMPTS_ = 15;    // ... and attempts (BHG_PREFIX_RIM_ATTEMPTS)
// rays per trace launch: the kernels form a ray's result offsets (idx * 48 at most) in 32 bits
constexpr uint64_t BHG_MAX_RAYS_PER_LAUNCH = 1ull << 26;

// Kernel arguments (passed by value -> SGPRs).  All pointers are device addresses.
// Fields the step loop reads come first, in order of use, the ones only the queue fill and the event drain read
// behind them (the kernarg segment is fetched in 16-dword chunks and, short of SGPRs, the compiler spills and reloads
// scalars through VGPR lanes; the order was measured neutral on every configuration -- it is kept for the reader).
struct TraceArgs {
    // ---- chunk 0 (16 dwords): every iteration of the step loop
    double *end;                 // [n][6]
    uint8_t *flags;              // [n] (never null inside the kernels: the C-ABI layer substitutes a workspace); only ever holds final values
    uint32_t *n_steps;           // [n] (never null inside the kernels, like flags)
    uint32_t *n_accepted;        // [n] (ditto)
    double rtol, atol, lambda_end, max_step;
    // ---- chunk 1: the step loop's event tests and controller limits
    double r_hor;                // horizon event radius: r_s, or r_plus (1 + margin) for Kerr
    double r_s;
    double min_step_cap;         // >= 10 ulp(t) for all t in [0, lambda_end]
    double r_exit, disk_r_in, disk_r_out;
    double spin;                 // Kerr a (BHG_RHS_KERR_BL_)
    double mu2;                  // -g(k, k): 0 null rays, 1 time-like (read by the Kerr start conversion only; the Cartesian
                                 // time-like form is a right-hand side of its own, BHG_RHS_CHRISTOFFEL_TL_)
    double h_fixed;
    // ---- chunk 2: parking (in the step loop's event branch), then the rare paths
    double *end_dir;             // nullptr, or [n][3]: FINAL states are written as their direction half only, here (end then
                                 // only holds the parked / resume records of rays that need them: a workspace)
    uint32_t max_steps;
    int32_t n_spheres;           // object spheres inside the curved region (Schwarzschild forms only)
    const double *k0;            // [n][3]
    const double *x0;            // [n][3] or nullptr -> x0s
    unsigned long long *counter; // 8 slice counters (256 B apart), zero at launch
    unsigned long long *counter_next; // the set the NEXT launch of this context will use: this launch zeroes it
    uint64_t n;                  // rays in the call
    double k0s[3];               // the direction of a ONE-ray trajectory call (k0 == nullptr)
    double x0s[3];
    int32_t order_blocks;        // work-order hint: n = order_blocks * order_block_len, batches are
    uint64_t order_block_len;    // handed out chunk-major over the blocks; 0/1 = plain order
    int8_t *object_id;           // [n] or nullptr: sphere index of rays that end with BHG_FLAG_HIT_OBJECT, else -1
    unsigned long long *diag;    // diagnostic builds only (BHG_DIAG): [grid][8] per-wave stamps
    uint32_t dbg_idx;            // diagnostic builds: ray whose controller trace is logged
    double spheres[BHG_MAX_SPHERES_][4];  // {cx, cy, cz, radius}, BH-centred
    // the rays' initial steps kept across calls (DP5(4) trace kernels only, read in the queue fill; the RK4 and the
    // lane-per-ray kernels never look): last, so that no other member moves
    double *start_h;             // [n] or nullptr
    int32_t start_mode;          // BHG_START_*_
    // disk crossings (disk_crossings_kernel alone; no other kernel looks): last, so that no other member moves
    int32_t max_cross;           // crossings stored per ray, 1 .. BHG_MAX_CROSSINGS_ (travel_time_kernel: 0 too)
    double *cross;               // [max_cross][cross_stride][6]: record m of ray i, Cartesian, at (m * cross_stride + i) * 6
    uint8_t *n_cross;            // [n]: crossings counted (saturating at 255), stored or not
    uint64_t cross_stride;       // rays per layer of cross: the CALL's ray count (a launch may be a part of a call)
    // the rays' start-up records kept across calls (the queue fill of the DP5(4) kernels of the two Cartesian null forms; no other
    // kernel looks): last, so that no other member moves
    const double2 *prefix;       // nullptr, or [7][n] 16-byte planes written by record_prefix_kernel for THESE rays and a ball
                                 // of radius rho about x0s that this call's event surfaces stay clear of
};

// the moving observer of the observer camera (frame_kernels.hip): on = 0 is the reference's camera
struct ObserverParams {
    double x0[3];      // camera, BH-centred (raygen only; the redshift calls take the camera from their own arguments)
    double beta[3];    // velocity relative to the ZAMO at the camera, world axes, |beta| < 1
    double r_s, spin;  // metric (raygen only)
    int32_t rhs;       // BHG_RHS_* (raygen only)
    int32_t on;        // 0: no observer -- the kernels' reference instances are launched and never read this struct
};

// textured, oriented and emissive object spheres (frame_kernels.hip): one slot per sphere.  on = 0: the
// shade kernels' untextured instances are launched and never read this struct
struct ObjectTextureParams {
    const float *tex[BHG_MAX_SPHERES_];   // [h][w][4] RGBA float32 equirectangular, or nullptr (a white texel)
    int32_t tex_w[BHG_MAX_SPHERES_], tex_h[BHG_MAX_SPHERES_];
    int32_t mode[BHG_MAX_SPHERES_];       // BHG_OBJECT_LIT_ / BHG_OBJECT_EMISSIVE_
    double emission[BHG_MAX_SPHERES_];    // emissive strength
    double rot[BHG_MAX_SPHERES_][9];      // row-major body -> world (the C layer has put the identity for an all-zero matrix)
    int32_t on;
};

// disk polarisation (frame_kernels.hip, polarisation_disk): the camera, the metric, the caller's degree
// table and image up.  on = 0: the shade kernels' unpolarised instances are launched and never read this struct
constexpr int BHG_POL_TABLE_MAX_ = 64;
struct PolarisationParams {
    double degree[BHG_POL_TABLE_MAX_];  // delta(mu_j), mu_j = j / (n_degree - 1)
    double up[3];      // image up, world axes at the camera
    double x0[3];      // camera, BH-centred (a shared origin; polarisation_kernel may read a per-ray one instead)
    double beta[3];    // the observer's velocity relative to the ZAMO, world axes; zero without an observer
    double r_s, spin;  // metric: r_s = 2M, Kerr a (rhs == BHG_RHS_KERR_BL_)
    double sense;      // disk sense, +1 = counter-clockwise seen from +z, or -1
    int32_t n_degree;  // 1 .. BHG_POL_TABLE_MAX_
    int32_t rhs;       // BHG_RHS_*
    int32_t on;
    int32_t pad;
    double *qu;        // shade kernels: [n_pixels][6] (Q_r, Q_g, Q_b, U_r, U_g, U_b) fp64
};

// the thermal disk (frame_kernels.hip, disk_thermal): the Page-Thorne constants the C layer computed for
// the caller's (a*, sense), the frequency table and the channel weights.  The metric, the camera and the sense are the
// RedshiftParams beside it (g is redshift_kernel's).  on = 0: the shade kernels' non-thermal instances are launched and never
// read this struct
constexpr int BHG_THERMAL_NU_MAX_ = 16;
struct ThermalParams {
    double nu[BHG_THERMAL_NU_MAX_];      // nu_j h / (k_B T_peak)
    double w[3][BHG_THERMAL_NU_MAX_];    // the R, G, B weights of each frequency
    double astar;      // a* = s a / M, s = -disk_sense (section 9's sense)
    double x0;         // sqrt(r_ms / M)
    double xr[3];      // the roots x_1, x_2, x_3 of x^3 - 3x + 2a*
    double c[3];       // c_i = 3 (x_i - a*)^2 / (x_i (x_i - x_j)(x_i - x_k)); 0 for the root x_i = 0 (a* = 0)
    double inv_fmax;   // 1 / max F^
    double r_ms;       // the innermost stable circular orbit of the family (BL r)
    double t_peak, f_col, scale;
    int32_t n_nu;      // 1 .. BHG_THERMAL_NU_MAX_
    int32_t on;
};

// The Page-Thorne flux shape F^(x), x = sqrt(r / M) > x0 (the caller keeps r > r_ms).  Host (the C layer's search for max F^)
// and device share it; written out operation by operation as tests/disk_thermal_reference.py restates it: the library is
// built with -ffp-contract=off, and near r_ms the bracket is a difference of terms of order (x - x0), so the order shows.
// The bracket vanishes like (x - x0)^2 at the inner edge while each term is of order (x - x0): every logarithm is taken as
// log1p of d / (x0 - x_i), d = x - x0 (exact by Sterbenz near the edge), so that each term carries a RELATIVE error of an
// epsilon and the flux eps / (x - x0) relative -- log(q) of the rounded quotient q = 1 + O(d) carried an absolute epsilon, the
// flux eps / (x - x0)^2, and t_em was wrong by orders of magnitude inside r_ms (1 + 1e-8).
__host__ __device__ inline double page_thorne(const ThermalParams &T, double x)
{
    const double x2 = x * x, d = x - T.x0;
    double b = d - (1.5 * T.astar) * log1p(d / T.x0);
    for (int i = 0; i < 3; i++) b = b - T.c[i] * log1p(d / (T.x0 - T.xr[i]));
    return b / ((x2 * x2) * ((x2 * x - 3.0 * x) + 2.0 * T.astar));
}

// moving and spinning object spheres (frame_kernels.hip, object_g_moving): sphere j's surface moves with
// v[j] + w[j] x (x - c_j), world axes, coordinate velocities.  moving: bit j set when sphere j has a nonzero v or w (the others
// take the at-rest g of redshift_g); on = 0: the kernels' instances without motion are launched and never read this struct
struct MotionParams {
    double v[BHG_MAX_SPHERES_][3];
    double w[BHG_MAX_SPHERES_][3];
    uint32_t moving;
    int32_t on;
};

// camera-ray generation (frame_kernels.hip)
struct RaygenArgs {
    const double *jitter;   // [S*H*W*2] MT19937 doubles, sample-major then row-major pixels, (u1, u2); nullptr = pixel
                            // centres (u1 = u2 = 1/2)
    int32_t compact;        // 1: the stream holds draws for the listed pixels only, [S][n_pixels][2] in list order (a
                            // mark window: the engine draws inside the window only, RelativisticRenderEngine.py:219)
    const int64_t *pixels;  // [n_pixels] flat pixel ids y*W+x, or nullptr = all pixels in order
    double *k0;             // [S*n_pixels][3], ray i = s*n_pixels + p
    uint64_t n_pixels;
    int32_t width, height, samples, rotate;
    double fov_x, fov_y;
    double rot[9];          // row-major camera rotation
    ObserverParams obs;     // the observer camera (bhg_raygen_observer_device); last, so that no other member moves
};

// redshift of a ray between the camera's ZAMO and its emitter (frame_kernels.hip, redshift_g):
// the metric, the camera and the redshift settings of bhg_redshift
struct RedshiftParams {
    double x0[3];      // camera, BH-centred (a shared origin; redshift_kernel may read a per-ray one instead)
    double r_s, spin;  // metric: r_s = 2M, Kerr a (rhs == BHG_RHS_KERR_BL_)
    double sense;      // disk sense, +1 = counter-clockwise seen from +z, or -1
    double exponent;   // colour weight g^exponent (shade kernels only)
    int32_t rhs;       // BHG_RHS_*
    uint32_t apply;    // BHG_REDSHIFT_* classes the shade kernels weigh; 0 = off
};

// one thread per ray: g[i] from the camera state (x0, k0) and the end record (bhg_redshift_device)
struct RedshiftArgs {
    RedshiftParams p;
    const double *x0;      // [n][3] or nullptr -> p.x0
    const double *k0;      // [n][3]
    const double *end;     // [n][6] or nullptr (then only sky, horizon and NaN rays have a g; disk / object rays get NaN)
    const uint8_t *flags;  // [n]
    double *g;             // [n]
    uint64_t n;
    ObserverParams obs;    // beta and on only: g of a moving observer (bhg_redshift_observer_device)
    // moving object spheres (bhg_redshift_motion_device, launch_redshift_motion; launch_redshift never reads these): last, so
    // that no other member moves
    MotionParams mo;
    const int8_t *object_id;                 // [n]: the sphere of each object ray
    double spheres[BHG_MAX_SPHERES_][4];     // {cx, cy, cz, radius}
};

// shading + per-pixel multisample mean (frame_kernels.hip)
struct ShadeArgs {
    const double *end;     // [S*n_pixels][6], or nullptr when dir is given
    const double *dir;     // [S*n_pixels][3] exit directions alone (sky-only scenes), or nullptr
    const uint8_t *flags;  // [S*n_pixels]
    const float *sky;      // [sky_h][sky_w][4] RGBA float32, equirectangular
    double *rgba;          // [n_pixels][4] fp64, or nullptr
    float *rgba_f32;       // [n_pixels or frame pixels][4] fp32, or nullptr
    const int64_t *scatter;  // nullptr, or where pixel p goes in rgba_f32
    uint64_t n_pixels;
    int32_t samples, sky_w, sky_h;
    // scene shading (bhg_shade_scene_device); all zero / null for the sky-only call
    const int8_t *object_id;  // [S*n_pixels] or nullptr
    const float *disk_tex;    // [disk_h][disk_w][4] RGBA float32 or nullptr (white)
    int32_t disk_w, disk_h;
    double disk_r_in, disk_r_out, disk_phase, disk_mean, disk_stddev, disk_intensity;
    int32_t n_spheres, n_lamps;
    double spheres[BHG_MAX_SPHERES_][4];
    double sphere_rgb[BHG_MAX_SPHERES_][3];
    double lamps[4][4];  // {x, y, z, intensity}
    // redshift (bhg_shade_scene_redshift_device): launch_shade takes the redshift instance of the shade kernels when
    // rs.apply != 0; the other instance -- the frame path without redshift -- never reads these two members
    const double *k0;      // [S*n_pixels][3] camera directions, or nullptr when rs.apply == 0
    RedshiftParams rs;
    ObserverParams obs;    // beta and on only: the redshift instance's g is the moving observer's (rs.apply != 0 only)
    // object textures (bhg_shade_scene_textured_device): launch_shade takes the textured instance when ot.on != 0
    ObjectTextureParams ot;
    // polarisation (bhg_shade_scene_polarised_device): launch_shade takes the polarised instance when pol.on != 0
    PolarisationParams pol;
    // the thermal disk (bhg_shade_scene_thermal_device): launch_shade takes the thermal instance when th.on != 0 -- always a
    // redshift instance, rs (metric, camera, sense) filled and rs.apply as the caller gave it or 0
    ThermalParams th;
    // moving object spheres (bhg_shade_scene_moving_device): launch_shade takes the motion instance when mo.on != 0 and
    // rs.apply weighs objects -- always a redshift instance; last, so that no other member moves
    MotionParams mo;
    // disk layers (bhg_shade_disk_layers_device, launch_shade_layers; launch_shade never reads these): last, so that no other
    // member moves
    const double *cross;      // [max_cross][S*n_pixels][6]: the crossing records of the crossings trace
    const uint8_t *n_cross;   // [S*n_pixels]
    int32_t max_cross;        // layers in cross, 1 .. BHG_MAX_CROSSINGS_
    double transmit;          // T = 1 - opacity of one disk crossing, 0 <= T < 1
};

// one thread per ray: (chi, delta, mu) from the camera state (x0, k0) and the end record (bhg_polarisation_device)
struct PolarisationArgs {
    PolarisationParams p;
    const double *x0;      // [n][3] or nullptr -> p.x0
    const double *k0;      // [n][3]
    const double *end;     // [n][6] or nullptr (then disk rays get NaN)
    const uint8_t *flags;  // [n]
    double *evpa, *degree, *mu;  // [n] each; mu may be nullptr
    uint64_t n;
};

// one thread per ray: T_em and (I_R, I_G, I_B) from the camera state (x0, k0) and the end record (bhg_disk_thermal_device)
struct ThermalArgs {
    ThermalParams t;
    RedshiftParams p;      // metric, camera, sense (apply unused): the disk g
    ObserverParams obs;    // beta and on only: g of a moving observer
    const double *x0;      // [n][3] or nullptr -> p.x0
    const double *k0;      // [n][3]
    const double *end;     // [n][6] or nullptr (then disk rays get NaN)
    const uint8_t *flags;  // [n]
    double *t_em;          // [n]
    double *rgb;           // [n][3]
    uint64_t n;
};

hipError_t launch_raygen(const RaygenArgs &a, hipStream_t s);
hipError_t launch_shade(const ShadeArgs &a, hipStream_t s);
// the layered shade of an optically thin disk (LayersColour under shade_pixels_kernel): a.cross / n_cross / max_cross / transmit filled
// t_cross: nullptr, or [max_cross][S*n_pixels], the crossing times of the travel-time trace -- the retarded instances then draw
// layer m of ray i at a.disk_phase - phase_rate * t_cross[m][i] (bhg_shade_disk_layers_retarded_device)
hipError_t launch_shade_layers(const ShadeArgs &a, hipStream_t s, const double *t_cross = nullptr, double phase_rate = 0.0);
hipError_t launch_redshift(const RedshiftArgs &a, hipStream_t s);
hipError_t launch_redshift_motion(const RedshiftArgs &a, hipStream_t s);
hipError_t launch_polarisation(const PolarisationArgs &a, bool obs, hipStream_t s);
hipError_t launch_disk_thermal(const ThermalArgs &a, hipStream_t s);
hipError_t launch_split_end(const double *end, uint64_t n, double *loc, double *dir, hipStream_t s);
hipError_t launch_gather_rows4(const float *src, const int64_t *index, uint64_t n, float *dst, hipStream_t s);

// ev: nullptr, or 3 events on stream s: two back to back in front of the trace launch (every kernel starts its rays itself, no
// pass runs ahead of it), one behind it
// evt: bit 0 = sphere-exit event compiled in, bit 1 = disk-plane event, bit 2 = object spheres (then all three)
hipError_t launch_trace(const TraceArgs &a, int method, int rhs, int evt, int grid, hipStream_t s, hipEvent_t *ev);
hipError_t trace_occupancy(int method, int rhs, int evt, int *blocks_per_cu);
// the disk-off trace that records every disk crossing (disk_crossings_kernel: one lane per ray, DP5(4), the Cartesian forms);
// a.cross / n_cross / max_cross / cross_stride filled
hipError_t launch_trace_crossings(const TraceArgs &a, int rhs, hipStream_t s);
// ... its Kerr instance, in the Kerr translation unit; the caller runs launch_kerr_finalize on the end records afterwards
hipError_t launch_trace_crossings_kerr(const TraceArgs &a, hipStream_t s);
// the crossings trace with the coordinate time along each ray (travel_time_kernel): t_end [a.n], t_cross
// [max_cross][cross_stride] beside a.cross.  a.max_cross = 0 and a.disk_r_out = 0 are allowed (a.cross, a.n_cross, t_cross may
// then be null); the Kerr instance sits in the Kerr translation unit and wants launch_kerr_finalize after it
hipError_t launch_travel_time(const TraceArgs &a, int rhs, double *t_end, double *t_cross, hipStream_t s);
hipError_t launch_travel_time_kerr(const TraceArgs &a, double *t_end, double *t_cross, hipStream_t s);
// the mesh trace (trace_mesh_kernel): the plain trace's steps with a triangle mesh as one more terminal
// event.  The mesh and the two outputs ride beside TraceArgs, which stays what it is.  a.disk_r_out > 0: the disk is opaque, as in
// the trace.  The Kerr instance sits in the Kerr translation unit and wants launch_kerr_finalize after it
struct MeshArgs {
    MeshView mesh;
    double box[6];          // the root box
    double d_min, d_max;    // every point of the mesh lies at a distance from the origin inside [d_min, d_max] (the Kerr cull)
    double max_chord;
    int32_t cull;           // 0: no whole-step cull (BHGEO_MESH_CULL=0)
    int32_t *tri_id;        // [n]: the caller's triangle of a ray that ends on the mesh, else -1
    double *bary;           // [n][2]: (u, v) of the refined point; untouched for a ray that hits nothing
};
constexpr int BHG_MESH_MAX_SUBSTEPS_ = 1024;
hipError_t launch_trace_mesh(const TraceArgs &a, const MeshArgs &m, int rhs, hipStream_t s);
hipError_t launch_trace_mesh_kerr(const TraceArgs &a, const MeshArgs &m, hipStream_t s);
// the mesh trace over K rigid placements of the one tree (trace_mesh_instances_kernel).  The records ride
// in an argument struct of their own; m.box is the union of the placements' world boxes and m.d_min, m.d_max the set's range of
// distances from the origin, so the whole-step cull is the plain kernel's
constexpr int BHG_MESH_INSTANCES_MAX_ = 64;
struct MeshInstanceArgs {
    const double *rec;      // [n][BHG_MESH_INSTANCE_DOUBLES_] (mesh_traverse.h): R row-major, t, the world box; unchanged during the launch
    int32_t n;              // 1 .. BHG_MESH_INSTANCES_MAX_
    int32_t cull;           // 0: no instance's world box is looked at (BHGEO_MESH_CULL=0, as MeshArgs::cull)
    int32_t *inst_id;       // [a.n]: the placement of a ray that ends on the mesh, else -1
};
hipError_t launch_trace_mesh_instances(const TraceArgs &a, const MeshArgs &m, const MeshInstanceArgs &in, int rhs, hipStream_t s);
hipError_t launch_trace_mesh_instances_kerr(const TraceArgs &a, const MeshArgs &m, const MeshInstanceArgs &in, hipStream_t s);
// ... over the placements of a set that lies under a tree (trace_mesh_instance_tree_kernel): m as above, the
// records and the tree over them in an argument struct of their own
constexpr int BHG_MESH_INSTANCE_TREE_MAX_ = 65536;
struct MeshInstanceTreeArgs {
    InstanceTreeView tree;  // mesh_traverse.h; unchanged during the launch
    int32_t cull;           // 0: no box is looked at, of the tree's or of an instance (BHGEO_MESH_CULL=0, as MeshArgs::cull)
    int32_t *inst_id;       // [a.n]: the placement of a ray that ends on the mesh, else -1
};
hipError_t launch_trace_mesh_instance_tree(const TraceArgs &a, const MeshArgs &m, const MeshInstanceTreeArgs &in, int rhs, hipStream_t s);
hipError_t launch_trace_mesh_instance_tree_kerr(const TraceArgs &a, const MeshArgs &m, const MeshInstanceTreeArgs &in, hipStream_t s);
// the mesh shade (MeshColour under shade_pixels_kernel, frame_kernels.hip): a.end / flags / sky / disk / lamps as launch_shade's plain instance wants
// them, n_spheres = 0; tri_rgb nullptr = white
hipError_t launch_shade_mesh(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary, const float *tri_rgb,
                             hipStream_t s);
// the mesh material shade (MeshColour with the material): the material rides in an argument struct of its own
struct MeshMaterialArgs {
    const float *tri_rgb;    // [nt][3] in the caller's numbering, or nullptr (white)
    const float *tri_uv;     // [nt][3][2] in the caller's numbering, or nullptr (no textures)
    const int32_t *tri_tex;  // [nt] image slot (< 0 or >= n_tex: none), or nullptr (slot 0)
    const float *tex[BHG_MESH_TEXTURES_MAX_];   // [h][w][4] RGBA float32, row 0 at V = 0
    int32_t tex_w[BHG_MESH_TEXTURES_MAX_], tex_h[BHG_MESH_TEXTURES_MAX_];
    int32_t n_tex;
    double emission;
};
hipError_t launch_shade_mesh_material(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                      const MeshMaterialArgs &mat, hipStream_t s);
// the instanced mesh shade (MeshInstanceColour): the material shade over the records of an instance set --
// rec [n_inst][BHG_MESH_INSTANCE_DOUBLES_], inst_id [S * n_pixels], inst_rgb [n_inst][3] or nullptr
hipError_t launch_shade_mesh_instances(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                       const MeshMaterialArgs &mat, const double *rec, int32_t n_inst, bool boxes,
                                       const int32_t *inst_id, const float *inst_rgb, hipStream_t s);
// ... over a set under a tree (MeshInstanceTreeColour): the shadow segments walk the tree in any-hit form
hipError_t launch_shade_mesh_instance_tree(const ShadeArgs &a, const MeshView &m, const int32_t *tri_id, const double *bary,
                                           const MeshMaterialArgs &mat, const InstanceTreeView &tree, bool boxes,
                                           const int32_t *inst_id, const float *inst_rgb, hipStream_t s);
// the recording pass of the start-up records (record_prefix_kernel: one lane per ray; rhs Christoffel or reduced, a.x0 == nullptr):
// rec [7][a.n] 16-byte planes, rho the radius about a.x0s the recorded steps stay inside.  deep: the record carries on through
// rejected attempts (deep: at most acc_max accepted steps -- BHG_PREFIX_DEEP_ACCEPTED_, or BHG_PREFIX_WIDE_ACCEPTED_ for
// BHG_PREFIX_RECORD_WIDE -- in att_max = BHG_PREFIX_DEEP_ATTEMPTS_ attempts, or BHG_PREFIX_RIM_ACCEPTED_ in BHG_PREFIX_RIM_ATTEMPTS_ for
// BHG_PREFIX_RECORD_RIM; neither cap is looked at otherwise)
hipError_t launch_record_prefix(const TraceArgs &a, int rhs, void *rec, double rho, bool deep, uint32_t acc_max, uint32_t att_max,
                                hipStream_t s);
// Kerr: after the last pass of a call, Boyer-Lindquist end states -> Cartesian
hipError_t launch_kerr_finalize(const TraceArgs &a, double *dir_out, hipStream_t s);
// the Kerr instantiations live in their own translation unit (geodesic_kernels_kerr.hip: same source, same flags --
// machine LICM off, see the Makefile -- compiled on its own)
hipError_t launch_trace_kerr(const TraceArgs &a, int method, int evt, int grid, hipStream_t s, hipEvent_t *ev);
hipError_t trace_occupancy_kerr(int method, int evt, int *blocks_per_cu);
hipError_t launch_trajectory_kerr(const TraceArgs &a, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s);
// ... and so does the time-like Christoffel form (geodesic_kernels_timelike.hip; one event variant)
hipError_t launch_trace_timelike(const TraceArgs &a, int method, int grid, hipStream_t s, hipEvent_t *ev);
hipError_t trace_occupancy_timelike(int method, int *blocks_per_cu);
hipError_t launch_trajectory_timelike(const TraceArgs &a, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s);
hipError_t launch_accel_timelike(const double *x, const double *k, double r_s, uint64_t n, double *acc, hipStream_t s);
// sampled trajectories, one lane or one wave per ray (+ Kerr finalize); traj [n][6][T], n_valid [n]
hipError_t launch_trajectory(const TraceArgs &a, int rhs, int method, double *traj, uint32_t *n_valid, uint32_t T, hipStream_t s);
// does a trajectory call of n rays run one wave per ray (the kernel then NaN-fills what a ray never reaches; the lane shape wants the block preset)?
bool trajectory_wave_per_ray(uint64_t n);
// rhs = Kerr: x, k and acc are Boyer-Lindquist (r, theta, phi) triples, E and L fixed by the null condition at each point
hipError_t launch_accel(const double *x, const double *k, double r_s, double spin, double mu2, uint64_t n, double *acc, int rhs,
                        hipStream_t s);
hipError_t launch_accel_kerr(const double *x, const double *k, double r_s, double spin, double mu2, uint64_t n, double *acc, hipStream_t s);

// roofline calibration probes (probe_kernels.hip): kind 0 = pure v_fma_f64, 1 = the DP5(4) step loop's instruction mix
hipError_t launch_probe(int kind, int grid, uint32_t iters, double *out, hipStream_t s);
void probe_shape(int kind, uint32_t *valu_per_iter, uint32_t *quarter_per_iter);
// the math probe (bhg_math_probe, a test hook): n elements through primitive `op` of device_math.h / kerr_start.h, one per thread;
// math_probe_shape: the doubles per element in and out, false for an unknown op
bool math_probe_shape(int op, int *n_in, int *n_out);
hipError_t launch_math_probe(int op, const double *in, uint64_t n, double *out, hipStream_t s);

}  // namespace bhg

/*
 * bhgeo.h -- C ABI of libbhgeo.so, the MI355X (gfx950) null-geodesic ray integrator.
 *
 * This is the drop-in boundary for ONE path of bldevries/blackhole_geodesic_calculator: the
 * per-ray geodesic solve the Blender render engine hands to the third-party `curvedpy` package.
 * The reference has no FFI today -- the boundary is a Python method call per ray:
 *
 *     self.GeoInt = curvedpy.GeodesicIntegratorSchwarzschild(mass=, time_like=False, verbose=False)
 *                                                   raytracer/RelativisticRenderEngine.py:134
 *     k_xyz, x_xyz, result = self.GeoInt.calc_trajectory(k0_xyz, x0_xyz, max_step=, curve_end=,
 *                                                   nr_points_curve=10000, verbose=False)
 *                                                   raytracer/RelativisticRenderEngine.py:293-294
 *
 * and, batched per frame, the arrays of a pre-traced camera:
 *
 *     cam.ray_blackhole_hit[iy, ix], cam.ray_end[iy, ix, 3:6]
 *                                                   raytracer/RelativisticRenderEngineCamEdition.py:225-228
 *
 * The entry points below are what a ctypes binding for that path binds (INTEGRATION.md shows the
 * stub).  Plain pointers and sizes only; no torch / numpy types.  All floating point is IEEE fp64.
 *
 * Array layouts (row-major, C-contiguous):
 *     k0    [n][3]   initial spatial direction k^i   (k0_xyz, RelativisticRenderEngine.py:287)
 *     x0    [3]      shared origin, BH-centred       (x0_xyz, :278, :288)   -- or [n][3] per ray
 *     end   [n][6]   {x, y, z, k_x, k_y, k_z} at the end of the curve
 *                    (= x_xyz[:, -1], k_xyz[:, -1] at :307-308; = ray_end[..., 0:6] of the Cam edition)
 *     flags [n]      BHG_FLAG_* bits (result['hit_blackhole'], result['start_inside_hole'], :296-297)
 *     n_steps [n]    attempted RK steps (accepted + rejected)
 *     n_accepted [n] accepted RK steps
 *
 * Threading: one bhg_context per device; calls on one context must not overlap (contexts of different
 * threads may run at the same time, on one device or several).  Host-buffer
 * calls block until the results are in the caller's buffers.  Device-buffer calls enqueue on the
 * given HIP stream and return; the library keeps no pointer after the call's work completes.
 * Device buffers need only the alignment of their element type (8 bytes for the doubles, 4 for the counts).
 *
 * Errors: every int-returning function returns BHG_OK (0) or a negative BHG_E_* code;
 * bhg_last_error() gives a thread-local message for the last failure.  A refused device allocation is
 * BHG_E_NOMEM and leaves the context usable.  The status of a call is its own: an error another caller of the
 * HIP runtime left behind on the thread (hipGetLastError() is sticky) is not reported, and the library leaves none
 * of its own behind.  There is no CPU
 * fallback: without a usable gfx950 device the calls fail with BHG_E_NO_DEVICE.
 */
#ifndef BHGEO_H
#define BHGEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BHG_ABI_VERSION 10  /* 10: the observer camera -- bhg_raygen_observer_device, bhg_redshift_observer_device / _host,
                                  bhg_shade_scene_redshift_observer_device, bhg_frame_set_observer, bhg_observer_size,
                                  struct bhg_observer; nothing of ABI 9 changed.
                                  Later additions within ABI 10, found by symbol and announced by a feature macro:
                                  BHG_OBJECT_TEXTURES (bhg_shade_scene_textured_device, bhg_frame_set_object_textures,
                                  bhg_object_textures_size, struct bhg_object_textures);
                                  BHG_POLARISATION (bhg_polarisation_device / _host, bhg_shade_scene_polarised_device,
                                  bhg_polarisation_size, struct bhg_polarisation);
                                  BHG_DISK_THERMAL (bhg_disk_thermal_device / _host, bhg_shade_scene_thermal_device,
                                  bhg_frame_set_disk_thermal, bhg_disk_thermal_size, struct bhg_disk_thermal);
                                  BHG_OBJECT_MOTION (bhg_redshift_motion_device / _host, bhg_shade_scene_moving_device,
                                  bhg_frame_set_object_motion, bhg_object_motion_size, struct bhg_object_motion);
                                  BHG_START_STEPS (bhg_trace_start_device, bhg_start_steps_match, BHG_START_*: the rays' initial
                                  steps kept across calls on unchanged rays);
                                  BHG_DISK_CROSSINGS (bhg_trace_crossings_device, bhg_trace_crossings, bhg_shade_disk_layers_device,
                                  bhg_disk_layers_size, struct bhg_disk_layers, BHG_MAX_CROSSINGS: higher-order disk images);
                                  BHG_TRAVEL_TIME (bhg_travel_time_device, bhg_travel_time, bhg_shade_disk_layers_retarded_device:
                                  the coordinate time along each ray, the disk layers at their retarded phase);
                                  BHG_MESH (bhg_mesh_create / _destroy / _info, bhg_mesh_bvh_host, bhg_trace_mesh_device,
                                  bhg_trace_mesh, bhg_shade_mesh_device, struct bhg_mesh, BHG_MESH_MAX_SUBSTEPS: triangle meshes
                                  in the curved region);
                                  BHG_MESH_MATERIAL (bhg_shade_mesh_material_device, bhg_frame_set_mesh, bhg_mesh_material_size,
                                  struct bhg_mesh_material, BHG_MESH_TEXTURES_MAX: textured, emissive meshes, meshes on bhg_frame);
                                  BHG_MESH_INSTANCES (bhg_mesh_instances_create / _set / _destroy / _info, bhg_mesh_instance_box_host,
                                  bhg_trace_mesh_instances_device, bhg_trace_mesh_instances, bhg_shade_mesh_instances_device, bhg_frame_set_mesh_instances, struct bhg_mesh_instances,
                                  BHG_MESH_INSTANCES_MAX: rigid placements of one mesh, moved without a rebuild);
                                  BHG_MESH_INSTANCE_TREE (bhg_mesh_instances_create_tree, bhg_mesh_instances_tree_info,
                                  bhg_mesh_instance_tree_host, bhg_frame_set_mesh_instance_tree, BHG_MESH_INSTANCE_TREE_MAX: an
                                  instance set under a tree of boxes);
                                  BHG_MESH_REFIT (bhg_mesh_refit, bhg_mesh_refit_device, bhg_mesh_refit_info, bhg_mesh_bvh_refit_host,
                                  bhg_mesh_refit_schedule_host, bhg_mesh_boxes_host, bhg_mesh_range, bhg_frame_refit_mesh, bhg_frame_mesh_refit_info: new vertices into a built mesh, its tree
                                  refitted on the device);
                                  BHG_MESH_BUILD_DEVICE (bhg_mesh_create_device, bhg_mesh_rebuild_device, bhg_mesh_rebuild,
                                  bhg_mesh_build_info, bhg_mesh_bvh_morton_host, bhg_mesh_tree_host: a Morton-order tree built
                                  on the device, rebuilt in place when the triangle list changes);
                                  BHG_PREFIX_RECORD_WIDE under BHG_START_PREFIX (bhg_prefix_wide_accepted, bhg_prefix_owner_next,
                                  bhg_frame_prefix_info, struct bhg_prefix_owner: wider start-up records, recorded again after refusals);
                                  BHG_PREFIX_RECORD_RIM (bhg_prefix_rim_attempts: start-up records to the rim of the clear ball).
                               9: redshift -- bhg_redshift_device / _host, bhg_shade_scene_redshift_device, bhg_frame_set_redshift,
                                  bhg_redshift_size, struct bhg_redshift;
                                  nothing of ABI 8 changed.
                               8: bhg_trajectory_objects (sampled curves that end on object spheres), the frame gather mode
                                  BHG_FRAME_GATHER_COPY_PEERCALL; nothing of ABI 7 changed.
                               7: the binder's handshake -- bhg_abi_check, bhg_*_size, bhg_default_params_sized; bhg_peak_probe.
                               6: bhg_frame_* (library-owned frame, N devices), bhg_deal_tiles, bhg_params.time_like (104 bytes) */

#define BHG_ABI_COMPAT_MIN 7 /* bhg_abi_check serves bindings written for this ABI or later: every symbol, struct layout and
                                meaning they know is unchanged (ABIs 8, 9 and 10 only ADDED entry points, a gather
                                mode, structs and constants) */

/* return codes */
#define BHG_OK 0
#define BHG_E_INVALID (-1)   /* bad argument (NULL pointer, non-finite / negative parameter) */
#define BHG_E_NO_DEVICE (-2) /* no HIP device / device index out of range */
#define BHG_E_HIP (-3)       /* a HIP runtime call failed; see bhg_last_error() */
#define BHG_E_NOMEM (-4)     /* device allocation failed */

/* per-ray flag bits */
#define BHG_FLAG_HIT_HORIZON 1u     /* result['hit_blackhole']  (RelativisticRenderEngine.py:297) */
#define BHG_FLAG_START_INSIDE 2u    /* result['start_inside_hole'] (:296, :311-313) */
#define BHG_FLAG_REACHED_END 4u     /* lambda reached curve_end */
#define BHG_FLAG_EXITED_SPHERE 8u   /* crossed r = r_exit outward (LimitedRelativisticRenderEngine.py:273-278) */
#define BHG_FLAG_MAX_STEPS 16u      /* attempted-step cap hit */
#define BHG_FLAG_STEP_TOO_SMALL 32u /* scipy's failure mode (rk.py:132-133) */
#define BHG_FLAG_NAN 64u            /* non-finite end state */
#define BHG_FLAG_HIT_DISK 128u      /* crossed z = 0 inside the annulus (LimitedRelativisticRenderEngine.py:413-438) */
#define BHG_FLAG_HIT_OBJECT 0x88u   /* ended on an object sphere (bhg_trace_objects*): the reference's collision stub
                                     * "NOW YOU DO COLLISION DETECTION", hit = False (RelativisticRenderEngine.py:304-305).
                                     * A composite value (EXITED_SPHERE | HIT_DISK never occur together otherwise):
                                     * test with (flags & 0x88) == 0x88 */
#define BHG_MAX_SPHERES 8

/* integrators */
#define BHG_METHOD_DP54 0 /* Dormand-Prince 5(4) with scipy RK45's controller (README.md:196) */
#define BHG_METHOD_RK4 1  /* classic fixed-step RK4 with step h_fixed */

/* right-hand-side formulations (algebraically identical for null rays) */
#define BHG_RHS_CHRISTOFFEL 0 /* -Gamma^i_{mu nu} k^mu k^nu, k^t from the null condition (README.md:198-209) */
#define BHG_RHS_REDUCED 1     /* -(3/2) r_s |x cross k|^2 x / r^5 (regular at the horizon) */
#define BHG_RHS_KERR_BL 2     /* Kerr, Boyer-Lindquist Christoffels (README.md:218 goal; `a = 0.9`,
                                 RelativisticRenderEngineCamEdition.py:210).  Same boundary: Cartesian x0, k0 in,
                                 Cartesian end state out (x = sqrt(r^2+a^2) sin th cos ph, z = r cos th); integrated
                                 in (r, theta, phi) with k^t from the Killing constants; the horizon event sits at
                                 r_plus (1 + BHG_KERR_HORIZON_MARGIN) because the coordinates are singular at r_plus */
#define BHG_KERR_HORIZON_MARGIN 1e-3

typedef struct bhg_params {
    double r_s;         /* horizon radius = 2*mass                 (RelativisticRenderEngine.py:95) */
    double lambda_end;  /* curve_end                               (:62, :294) */
    double max_step;    /* max_step; +inf for "unset" (-1)         (:57-60) */
    double rtol;        /* DP54 relative tolerance, scipy default 1e-3; below 100 eps it is raised to 100 eps, as solve_ivp does (_ivp/common.py:44-51) */
    double atol;        /* DP54 absolute tolerance, scipy default 1e-6; must be > 0 (solve_ivp takes 0 too and then fails on the first state
                           component that is exactly zero -- scale = 0 -- with "step size too small": refused here up front) */
    double h_fixed;     /* RK4 step */
    double r_exit;      /* 0 = off; else terminate when r crosses r_exit outward */
    int32_t method;     /* BHG_METHOD_* */
    int32_t rhs_form;   /* BHG_RHS_* */
    uint32_t max_steps; /* cap on attempted steps per ray; 0 = library default (1<<20) */
    uint32_t order_blocks; /* work-order hint, 0 = none: the n rays are this many equal blocks (e.g. the samples of a
                              frame laid out [sample][pixel]) and the library may start the corresponding parts of all
                              blocks together (better balance when the pixels are sorted longest-first); ignored unless
                              n / order_blocks is a multiple of 64.  Never changes a result. */
    double disk_r_in;   /* thin disk in the plane z = 0 (BH-centred frame): the ray ends at its first */
    double disk_r_out;  /* crossing with R_in <= sqrt(x^2+y^2) <= R_out; off when disk_r_out == 0
                           (disk_on / R_in / R_out of LimitedRelativisticRenderEngine.py:283-286).  With
                           BHG_RHS_KERR_BL: the equatorial plane theta = pi/2 (z = r cos theta = 0), the
                           annulus in the cylindrical radius sqrt(r^2 + a^2) */
    double spin;        /* Kerr a in length units, |a| < M = r_s/2 (BHG_RHS_KERR_BL only) */
    int32_t time_like;  /* 0: null geodesics, g(k, k) = 0 -- what the engine asks for (time_like=False, RelativisticRenderEngine.py:134); 1: the
                           constructor argument's other value, massive particles: g(k, k) = -1, lambda is the proper time.
                           With BHG_RHS_CHRISTOFFEL (the norm enters through (k^t)^2 = (|k|^2 + h (n.k)^2 + 1) / f) and
                           BHG_RHS_KERR_BL (through E and L at the start); BHG_RHS_REDUCED is the null closed form and
                           refuses it.  The plotting path (bhg_trajectory, bhg_trace): no frame pipeline asks for it. */
    int32_t reserved0;  /* 0 */
} bhg_params;

typedef struct bhg_context bhg_context;

/* --- library ---------------------------------------------------------------------------- */
int bhg_version(void);                /* BHG_ABI_VERSION */
int bhg_device_count(void);           /* number of HIP devices, 0 if none, never fails */
const char *bhg_last_error(void);     /* thread-local, never NULL */
void bhg_default_params(bhg_params *p); /* engine defaults: r_s=1 (mass 0.5), lambda_end=50,
                                           max_step=inf, rtol=1e-3, atol=1e-6, DP54, Christoffel
                                           (RelativisticRenderEngine.py:506-508; scipy rk.py:85-87).
                                           Writes sizeof(bhg_params) bytes AS THE LIBRARY LAYS THE STRUCT OUT:
                                           a binding checks its own layout first (below) */

/* --- the binder's handshake ---------------------------------------------------------------
 * The reference-side caller is a Python file (raytracer/RelativisticRenderEngine.py:134, :293-294): its binding declares
 * these structs by hand (ctypes), and a struct that grew between library versions (bhg_params: 96 bytes in ABI 5, 104
 * since ABI 6) is then written and read past its end without any error.  A binding therefore calls, once after loading,
 *
 *     bhg_abi_check(<the BHG_ABI_VERSION it was written for>, sizeof its bhg_params, bhg_camera, bhg_scene, bhg_frame_scene)
 *
 * -> BHG_OK, or BHG_E_INVALID with a bhg_last_error() message that names both figures.  A size of 0 = "this binding does
 * not declare that struct".  bhg_*_size() give the library's own sizes; bhg_default_params_sized() is bhg_default_params
 * for a caller that passes its struct's size along and gets BHG_E_INVALID -- and not one byte written -- on a mismatch. */
size_t bhg_params_size(void);
size_t bhg_camera_size(void);
size_t bhg_scene_size(void);
size_t bhg_frame_scene_size(void);
int bhg_abi_check(int abi_version, size_t params_size, size_t camera_size, size_t scene_size, size_t frame_scene_size);
int bhg_default_params_sized(bhg_params *p, size_t params_size);

/* --- context ----------------------------------------------------------------------------
 * Every entry point makes the context's device current for its own HIP calls and restores the calling
 * thread's current device before it returns. */
int bhg_create(int device, bhg_context **out); /* replaces the per-frame solver construction (:134) */
void bhg_destroy(bhg_context *ctx);
int bhg_device_name(bhg_context *ctx, char *buf, size_t buflen);
int bhg_num_cus(bhg_context *ctx);

/* --- the hot path ----------------------------------------------------------------------- */
/* Host buffers.  Batched replacement of N calc_trajectory calls (:293-294): copies k0 (and x0)
 * to the device, integrates all rays, copies end and whichever of flags / n_steps / n_accepted is not NULL
 * back.  x0_is_shared != 0: x0 is [3]; else [n][3].  Blocking.  Internally a pipeline over chunks of 2^20 rays
 * (upload of the next chunk, trace, download of the previous one overlap on three streams); arrays in pageable
 * memory go through a pinned staging ring with multi-threaded host copies, arrays in page-locked memory
 * (bhg_host_alloc, hipHostMalloc, hipHostRegister) are read / written by the copy engines directly. */
int bhg_trace(bhg_context *ctx, const bhg_params *p, const double *x0, int x0_is_shared,
              const double *k0, size_t n, double *end, uint8_t *flags, uint32_t *n_steps,
              uint32_t *n_accepted);

/* Rays resident on the device: the engine's camera rays (RelativisticRenderEngine.py:185-230 -- pinhole + MT19937
 * jitter, rotate, normalise; loop order sample -> row -> column) are generated ON the device from the jitter stream
 * and stay there, so the directions (24 B/ray) never cross PCIe, and a frame loop whose camera does not move (the
 * engine re-seeds identically on every render(), :189) traces the same ray set again and again.  This is the path
 * the frame driver and the pre-traced camera of the Python adaptor use (frame.py, camera.py).
 *   jitter: HOST array of random.random() draws, (u1, u2) per ray, or NULL = pixel centres (u = 1/2: the Cam
 *           edition's camera, CamEdition.py:225-228).  jitter_is_compact = 0: the full-frame stream
 *           [samples][height][width][2]; 1: draws for the listed pixels only, [samples][n_pixels][2] in list order
 *           (a mark window: the engine only draws inside it, :219).
 *   pixels: HOST array of flat pixel ids y * width + x, or NULL = every pixel in row-major order.
 * Ray s * n_pixels + p is sample s of pixel p.  The rays belong to ctx and must be destroyed before it.  An EMPTY pixel list
 * (pixels != NULL, n_pixels = 0: a shard that was dealt no tile) gives a ray set of 0 rays. */
typedef struct bhg_camera {
    int32_t width, height, samples, reserved;
    double fov_x, fov_y;  /* property values fov_x / fov_y of the engine (:504-505) */
    double rot[9];        /* row-major rotation matrix of the camera's Euler angles (:183); identity = unrotated */
    double origin[3];     /* camera position minus the hole's (:278) */
} bhg_camera;
typedef struct bhg_rays bhg_rays;
int bhg_rays_create(bhg_context *ctx, const bhg_camera *cam, const double *jitter, int jitter_is_compact,
                    const int64_t *pixels, size_t n_pixels, bhg_rays **out);
size_t bhg_rays_count(const bhg_rays *rays);
void bhg_rays_destroy(bhg_rays *rays);
/* Trace rays [first, first + n) of the set and bring back only what is asked for (HOST arrays, any may be NULL):
 * end [n][6], or its halves end_loc [n][3] / end_dir [n][3] -- spacetime_ray_cast's return values (:307-308) --
 * flags, n_steps, n_accepted, object_id.  Same pipeline, same kernels and bit-for-bit the same results as bhg_trace on
 * the same directions.  Blocking. */
int bhg_rays_trace(bhg_rays *rays, const bhg_params *p, const double *spheres, int32_t n_spheres, size_t first, size_t n,
                   double *end, double *end_loc, double *end_dir, uint8_t *flags, uint32_t *n_steps,
                   uint32_t *n_accepted, int8_t *object_id);

/* Page-locked host memory for the arrays handed to bhg_trace / bhg_trace_objects: results then arrive by DMA
 * with no host-side copy.  (numpy's own allocations are pageable; the Python adaptor allocates its result arrays
 * here and keeps a pool of them, page-locking being slow.)  ctx may be NULL in bhg_host_free. */
int bhg_host_alloc(bhg_context *ctx, size_t bytes, void **out);
int bhg_host_free(bhg_context *ctx, void *p);

/* Sampled curves, host buffers: what calc_trajectory returns for nr_points_curve samples
 * (RelativisticRenderEngine.py:293-294, :299-302; the trajectory plots of README.md Fig. 5/6).
 * t_eval = linspace(0, lambda_end, n_points); after every accepted step the samples t_eval <= lambda
 * are produced from the step's dense output, as solve_ivp does with t_eval; a ray that ends early (horizon,
 * exit sphere) yields n_valid[i] < n_points samples, the rest of its row is NaN.  traj [n][6][n_points]
 * (rows x, y, z, k_x, k_y, k_z).  end [n][6] / flags [n] (may be NULL): the same end state and flags
 * bhg_trace gives -- with the exit sphere and, since ABI 7, the thin disk (a ray that ends on it: BHG_FLAG_HIT_DISK, the
 * curve sampled up to the crossing, end = the crossing point: what checkHitDisk looks for on the sampled path,
 * LimitedRelativisticRenderEngine.py:284, :413-438).  BHG_METHOD_RK4 (ABI 7): fixed steps h_fixed, the samples on each step's
 * cubic Hermite interpolant (the one the fixed-step kernels locate events on).  At most 2^26 rays per call.  Small-n path: one
 * WAVE per ray up to 2048 rays (a step's samples are shared out over the 64 lanes: the engine's literal call, one ray
 * with 10,000 samples, takes about 0.1 ms), one lane per ray above; the same bits either way.  A `traj` of at most 4 MB in
 * PAGE-LOCKED memory (bhg_host_alloc) is written by the wave-per-ray kernel directly, over PCIe: no copy of the sample
 * block, no host-side split (the Python adaptor allocates it so). */
int bhg_trajectory(bhg_context *ctx, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0,
                   size_t n, uint32_t n_points, double *traj, uint32_t *n_valid, double *end, uint8_t *flags);
/* ... with object spheres in the curved region (ABI 8): the engine's literal per-ray call is exactly where the reference put
 * its collision stub ("NOW YOU DO COLLISION DETECTION", RelativisticRenderEngine.py:293-305).  spheres [n_spheres][4] =
 * {cx, cy, cz, radius}, BH-centred, as in bhg_trace_objects: a ray that enters one ends there with BHG_FLAG_HIT_OBJECT --
 * the same flag, sphere index (object_id [n], -1 = none; may be NULL), entry point and step counts bhg_trace_objects gives
 * for that ray -- and its curve is sampled up to the entry point, NaN behind it.  n_spheres = 0 is bhg_trajectory. */
int bhg_trajectory_objects(bhg_context *ctx, const bhg_params *p, const double *spheres, int32_t n_spheres, const double *x0,
                           int x0_is_shared, const double *k0, size_t n, uint32_t n_points, double *traj, uint32_t *n_valid,
                           double *end, uint8_t *flags, int8_t *object_id);

/* Device buffers (all d_* are device addresses on ctx's device; x0_shared is a HOST [3] array or
 * NULL when d_x0 [n][3] is given).  Enqueues on `stream` (a hipStream_t; NULL = HIP's null
 * stream, as everywhere in HIP; bhg_context_stream() gives the context's own stream) and
 * returns without synchronising -- with or without a disk or objects: ONE persistent launch finishes
 * every ray (events are located and rays that carry on are resumed inside the trace kernel).  Two calls
 * on one context never overlap: they share the context's work counters and workspace, so a call issued on another
 * stream than the previous one is ordered behind it by the library: a call on a CALLER's stream records an event behind
 * itself before it returns, the next call on another stream waits on that event -- the library never touches a caller's
 * stream after the call that was given it has returned, so the caller may destroy it right away; calls that are to run
 * concurrently need a context each).  The launch is not graph-replayable (it consumes and re-arms those counters). */
int bhg_trace_device(bhg_context *ctx, const bhg_params *p, const double *x0_shared,
                     const double *d_x0, const double *d_k0, size_t n, double *d_end,
                     uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted, void *stream);

/* The same call for a caller that consumes only the DIRECTION half of the end states -- what a sky frame reads of
 * spacetime_ray_cast's return values (end_dir, RelativisticRenderEngine.py:308, :366-378; the flags say which rays
 * hit the hole): d_end_dir [n][3].  The trace kernel writes 24 instead of 48 bytes per ray and bhg_shade_dir_device
 * reads as many; bit-for-bit the directions bhg_trace_device gives.  (Kerr: traced into an internal record array and
 * split off -- same result, no saving.)  bhg_rays_trace takes this path by itself when only end_dir (and flags,
 * counts) are asked for. */
int bhg_trace_dir_device(bhg_context *ctx, const bhg_params *p, const double *x0_shared, const double *d_x0,
                         const double *d_k0, size_t n, double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps,
                         uint32_t *d_n_accepted, void *stream);

/* Objects inside the curved region (the reference holds only the stub at
 * RelativisticRenderEngine.py:304-305, "hit = False", and README.md:225 lists it as a goal): up to
 * BHG_MAX_SPHERES spheres, HOST array spheres [n_spheres][4] = {cx, cy, cz, radius} in BH-centred
 * coordinates.  A ray that is outside sphere j at the start of an accepted step and either ends the
 * step inside it, or whose chord between the step ends passes through it while the step's dense output
 * at the chord's closest point lies inside, enters the sphere in that step; the entry point is the root
 * of |x(lambda) - c_j| - radius_j on the dense output (Brent, like every other event).  Of all terminal
 * events of a step the earliest wins.  Such rays end with BHG_FLAG_HIT_OBJECT, end = entry point and
 * direction there, object_id = j; all other rays get object_id -1.  object_id may be NULL.  With
 * BHG_RHS_KERR_BL the spheres are met in this same Cartesian frame (x = sqrt(r^2 + a^2) sin th cos ph, ...): chord rule on
 * the images of the step's ends, root on the image of the dense output.  The device-buffer form only enqueues (one launch), like bhg_trace_device.
 * With n_spheres = 0 they are bhg_trace / bhg_trace_device. */
int bhg_trace_objects(bhg_context *ctx, const bhg_params *p, const double *spheres, int32_t n_spheres,
                      const double *x0, int x0_is_shared, const double *k0, size_t n, double *end,
                      uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted, int8_t *object_id);
int bhg_trace_objects_device(bhg_context *ctx, const bhg_params *p, const double *spheres, int32_t n_spheres,
                             const double *x0_shared, const double *d_x0, const double *d_k0, size_t n,
                             double *d_end, uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted,
                             int8_t *d_object_id, void *stream);

/* --- the rays' initial steps kept across calls (within ABI 10, BHG_START_STEPS) -------------------
 * A DP5(4) trace call works out every ray's first step size (scipy's select_initial_step: a second right-hand side, square
 * roots, divisions) before it integrates.  That step depends on the ray (x0, k0), on rtol, atol, lambda_end and max_step,
 * on the metric (r_s, spin, time_like, rhs_form) and on nothing else -- not on the exit sphere, the disk, the object spheres,
 * the step budget, the output form or the work-order hint.  A caller that OWNS its rays and traces them again and again (a
 * static camera, an animation that moves objects only) keeps the steps in d_start_steps [n] doubles:
 *   BHG_START_RECORD: the call of always, which also stores the step of every ray it integrates (rays that start inside the
 *                     hole are neither written nor, later, used);
 *   BHG_START_REPLAY: loads them instead (8 B per ray); valid after a recording call with the SAME d_x0 / x0_shared and d_k0
 *                     contents, the same n and parameters for which bhg_start_steps_match() gives 1.  The results are the
 *                     recording call's bit for bit.  The library cannot check that the rays are unchanged: the caller vouches.
 *   BHG_START_NONE:   d_start_steps is ignored (may be NULL): bhg_trace_device / _dir_device / _objects_device are this.
 * bhg_trace_start_device takes what those three take together: d_end [n][6], or -- d_end NULL -- d_end_dir [n][3]; spheres may
 * be NULL with n_spheres = 0, d_object_id may be NULL.  BHG_METHOD_RK4 has no such step: the array is left untouched.  A call
 * of more than 2^26 rays is split into launches and the array is walked along with d_k0.  When a recording call fails, treat
 * the array as not recorded. */
#define BHG_START_STEPS 1
#define BHG_START_NONE 0
#define BHG_START_RECORD 1
#define BHG_START_REPLAY 2
int bhg_trace_start_device(bhg_context *ctx, const bhg_params *p, const double *spheres, int32_t n_spheres,
                           const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                           double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted,
                           int8_t *d_object_id, double *d_start_steps, int32_t start_mode, void *stream);
/* 1 when the two parameter sets give every ray the same initial step (the list above, and the integrator: only DP5(4) records
 * anything), else 0 -- also for a NULL argument.  THE one holder of that list: every owner of a d_start_steps array asks it. */
int bhg_start_steps_match(const bhg_params *a, const bhg_params *b);

/* --- the rays' start-up records kept across calls (within ABI 10, BHG_START_PREFIX) ---------------
 * scipy's start guess is one to two decades below the step a ray settles on, and the controller climbs there by its x10
 * clamp: the first three or four accepted steps of every ray, a quarter of a frame's attempts, next to the camera.  Like the
 * initial step they depend on the ray and on the parameters of bhg_start_steps_match() -- and on the scene only through the
 * question whether an event surface comes near.  The owner of unchanged rays keeps them in bhg_prefix.d_records,
 * BHG_PREFIX_BYTES_PER_RAY * n bytes of device memory, 16-byte aligned:
 *   BHG_PREFIX_RECORD: in front of the call of always a recording pass takes every ray through its leading accepted steps,
 *                      at most BHG_PREFIX_K_MAX, inside the ball of radius rho = 1/4 min(clearance, |x0|) about the start
 *                      point (clearance: bhg_prefix_clearance of this call), and stores the state reached; rho is returned.
 *   BHG_PREFIX_REPLAY: rays with a usable record enter the integration at that state (112 B loaded per ray; no k0, no initial
 *                      step), the others start as always -- IF the call's own clearance still exceeds the rho handed back in
 *                      (the scene may have changed: an object sphere moved in, a disk was set).  Otherwise the call runs
 *                      without the records.  Results are the plain call's bit for bit either way, n_steps / n_accepted
 *                      included (they count the replayed steps).
 *   BHG_PREFIX_RECORD_DEEP: RECORD by a second rule.  The recording pass carries on THROUGH
 *                      rejected attempts -- a rejected attempt tests no event and moves nothing; it leaves a smaller step, the
 *                      controller's "last attempt was rejected" bit and the attempt count, which depend on what an accepted
 *                      step depends on -- and stops in front of the first attempt that would end or flag the ray, in front
 *                      of an accepted step that leaves the ball, after BHG_PREFIX_DEEP_ACCEPTED accepted steps or after
 *                      BHG_PREFIX_DEEP_ATTEMPTS attempts.  The ball: rho = 3/4 min(clearance, |x0|) in a call without object
 *                      spheres whose nearest surface is the horizon (the one surface that cannot change without new
 *                      records; REPLAY tests every call against rho all the same), the 1/4 of RECORD with any object
 *                      sphere or where the exit sphere or the disk plane is nearer.  Same buffer, same 112 bytes per ray, replayed by
 *                      the same BHG_PREFIX_REPLAY; needs max_steps > BHG_PREFIX_DEEP_ATTEMPTS, else nothing is written
 *                      (used = BHG_PREFIX_NONE, rho = 0).
 *   BHG_PREFIX_RECORD_WIDE: RECORD_DEEP in a wider ball: rho = 15/16 min(clearance, |x0|) exactly
 *                      where RECORD_DEEP takes its 3/4 -- no object sphere, the horizon the nearest surface -- and up to
 *                      BHG_PREFIX_WIDE_ACCEPTED accepted steps in the same BHG_PREFIX_DEEP_ATTEMPTS attempts; the 1/4 everywhere
 *                      else, with records that equal RECORD_DEEP's byte for byte there.  Same buffer, same bytes, same REPLAY,
 *                      same max_steps > BHG_PREFIX_DEEP_ATTEMPTS.  From a camera at r = 30 the ball reaches r = 2.8: any later
 *                      exit sphere, disk or object sphere inside it makes REPLAY refuse, which costs speed and nothing else; an
 *                      owner gets the speed back by recording again (bhg_prefix_owner_next).  A recording call of any rule may
 *                      go with BHG_START_REPLAY: the start steps are not recorded again.
 *   BHG_PREFIX_RECORD_RIM: RECORD_WIDE in the ball that ends just above the horizon: rho =
 *                      (1 - 2^-10) min(clearance, |x0|) exactly where RECORD_WIDE takes its 15/16, with up to
 *                      BHG_PREFIX_RIM_ACCEPTED accepted steps in BHG_PREFIX_RIM_ATTEMPTS attempts, and RECORD_WIDE's records byte
 *                      for byte everywhere else.  Same buffer, same bytes, same REPLAY.  Where it takes the larger ball it needs
 *                      max_steps > BHG_PREFIX_RIM_ATTEMPTS, else nothing is written (used = BHG_PREFIX_NONE, rho = 0) -- and so
 *                      does every call that replays such records: they are known by their rho, which no other rule gives from
 *                      the same origin and horizon, and a REPLAY of them with BHG_PREFIX_DEEP_ATTEMPTS < max_steps <=
 *                      BHG_PREFIX_RIM_ATTEMPTS is BHG_E_INVALID.
 *   BHG_PREFIX_NONE:   bhg_trace_start_device.
 * used says what the call did: BHG_PREFIX_RECORD, _DEEP, _WIDE or _RIM (records written by that rule), BHG_PREFIX_REPLAY
 * (records used) or BHG_PREFIX_NONE (refused, or out of scope).  A REPLAY call cannot tell which rule wrote the records it is
 * handed, so it uses none under a step budget that a deep record could exhaust: max_steps <= BHG_PREFIX_DEEP_ATTEMPTS is
 * answered with BHG_PREFIX_NONE, the plain call's results as always.  (Mode 3 is no mode and stays BHG_E_INVALID.)  In scope: x0_shared calls (d_x0 NULL) of BHG_METHOD_DP54 with BHG_RHS_CHRISTOFFEL or
 * BHG_RHS_REDUCED, null rays, at most 2^26 rays, max_steps > BHG_PREFIX_K_MAX.  REPLAY is valid after a RECORD call with the
 * same x0_shared and d_k0 contents, the same n and parameters for which bhg_start_steps_match() gives 1: the caller vouches,
 * as for the start steps.  d_start_steps / start_mode keep their meaning for the rays that start as always. */
#define BHG_START_PREFIX 1
#define BHG_PREFIX_NONE 0
#define BHG_PREFIX_RECORD 1
#define BHG_PREFIX_REPLAY 2
#define BHG_PREFIX_RECORD_DEEP 4 /* (3 stays no mode: callers were promised BHG_E_INVALID for it) */
#define BHG_PREFIX_RECORD_WIDE 5
#define BHG_PREFIX_RECORD_RIM 6
#define BHG_PREFIX_K_MAX 4
#define BHG_PREFIX_DEEP_ACCEPTED 6  /* accepted steps a deep record holds at most */
#define BHG_PREFIX_DEEP_ATTEMPTS 12 /* attempts a deep or wide record holds at most, rejected ones included */
#define BHG_PREFIX_WIDE_ACCEPTED 8  /* accepted steps a wide record holds at most */
#define BHG_PREFIX_RIM_ACCEPTED 9   /* accepted steps a rim record holds at most */
#define BHG_PREFIX_RIM_ATTEMPTS 15  /* attempts a rim record holds at most, rejected ones included */
#define BHG_PREFIX_BYTES_PER_RAY 112
typedef struct bhg_prefix {
    void *d_records;  /* device, BHG_PREFIX_BYTES_PER_RAY * n bytes */
    double rho;       /* RECORD, RECORD_DEEP: out (0 when nothing was recorded); REPLAY: in */
    int32_t mode;     /* in: BHG_PREFIX_* */
    int32_t used;     /* out: BHG_PREFIX_* */
} bhg_prefix;
int bhg_trace_prefix_device(bhg_context *ctx, const bhg_params *p, const double *spheres, int32_t n_spheres,
                            const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                            double *d_end_dir, uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted,
                            int8_t *d_object_id, double *d_start_steps, int32_t start_mode, bhg_prefix *prefix, void *stream);
/* Distance from x0 (HOST, 3 doubles, BH-centred) to the nearest event surface of a call with these parameters and object
 * spheres: the horizon, the exit sphere, the disk plane when a disk is set, every sphere's surface.  0 for a start on or
 * inside the horizon and for anything not finite.  A replaying call needs clearance > rho (1 + 1e-6): tangent is refused. */
double bhg_prefix_clearance(const bhg_params *p, const double *spheres, int32_t n_spheres, const double *x0);
/* BHG_PREFIX_DEEP_ATTEMPTS as the library was built with it.  A library that exports this symbol takes BHG_PREFIX_RECORD_DEEP
 * (one without it answers that mode with BHG_E_INVALID): what a caller that loads the library at run time asks first. */
int32_t bhg_prefix_deep_attempts(void);
/* BHG_PREFIX_WIDE_ACCEPTED as the library was built with it: a library that exports this symbol takes BHG_PREFIX_RECORD_WIDE
 * and has bhg_prefix_owner_next. */
int32_t bhg_prefix_wide_accepted(void);
/* BHG_PREFIX_RIM_ATTEMPTS as the library was built with it: a library that exports this symbol takes BHG_PREFIX_RECORD_RIM, as a
 * mode and as the promote argument of bhg_prefix_owner_next. */
int32_t bhg_prefix_rim_attempts(void);
/* When the owner of a ray set's records records them AGAIN because the scene has changed (the rays' own invalidation -- other
 * rays, another origin, parameters bhg_start_steps_match() rejects -- stays the owner's: start from a zeroed bhg_prefix_owner
 * and a recording call).  Before every later call the owner hands in the call's scene, the rule it records by (BHG_PREFIX_RECORD,
 * _DEEP, _WIDE or _RIM) and the bhg_prefix of its LAST call as that call left it (NULL: there was none), and is told what to ask for:
 *   BHG_PREFIX_REPLAY with o->rho, or
 *   rule: record now, in a call that may replay its start steps -- after two refused calls in a row (one refused frame, an object
 *         passing through, changes nothing), or after eight calls in a row whose scene the rule gives at least twice o->rho
 *         (what kept the ball small has gone), this call being one more of them, or
 *   promote (BHG_PREFIX_RECORD_DEEP or _WIDE, or BHG_PREFIX_NONE for no such rule): record now by this wider rule -- after 32
 *         calls in a row that all replayed, when it gives this call's scene more than o->rho.  The owners of the library and
 *         the binding record by RECORD_DEEP and are promoted to RECORD_WIDE; BHGEO_WIDE_PREFIX=1 in the environment makes
 *         them record by RECORD_WIDE from the first call, BHGEO_WIDE_PREFIX=0 never.  promote = BHG_PREFIX_RECORD_RIM names the
 *         whole ladder: RECORD_WIDE is earned first, exactly as above, and RECORD_RIM by 96 further calls in a row that replayed
 *         the wide records.  That is what the two owners ask for now; BHGEO_RIM_PREFIX=0 ends their ladder at RECORD_WIDE,
 *         BHGEO_RIM_PREFIX=1 makes them record by RECORD_RIM from the first call.  Or
 *   BHG_PREFIX_NONE: no records are held (also for a NULL argument) -- or rim records are, and p->max_steps is too small to
 *         replay them (<= BHG_PREFIX_RIM_ATTEMPTS): the records stay, this call goes without.
 * HOST only; the same code decides for bhg_frame_render. */
typedef struct bhg_prefix_owner {
    double rho;          /* the held records' radius, 0: none */
    int32_t refused_run; /* refused calls in a row */
    int32_t roomy_run;   /* calls in a row with room for twice rho */
    int32_t clean_run;   /* calls in a row that replayed */
    int32_t reserved;    /* 0 */
} bhg_prefix_owner;
int32_t bhg_prefix_owner_next(bhg_prefix_owner *o, int32_t rule, int32_t promote, const bhg_params *p, const double *spheres,
                              int32_t n_spheres, const double *x0, const bhg_prefix *last);

/* --- the stages either side of the solve, on device ---------------------------------------- */
/* Camera rays with the reference's multisample jitter (RelativisticRenderEngine.py:185-188,
 * :224-230).  d_jitter [samples*height*width*2]: the random.random() stream after
 * random.seed(sampling_seed) (:189), sample-major, then rows, then columns, (u1, u2) per pixel.
 * d_pixels [n_pixels]: flat pixel ids y*width+x to generate (a GPU's tile shard), or NULL for all
 * pixels in order.  rot9: row-major camera rotation (HOST, may be NULL = identity).
 * Output d_k0 [samples*n_pixels][3], ray index = s*n_pixels + p. */
int bhg_raygen_device(bhg_context *ctx, int32_t width, int32_t height, int32_t samples, double fov_x,
                      double fov_y, const double *rot9, const double *d_jitter, const int64_t *d_pixels,
                      size_t n_pixels, double *d_k0, void *stream);

/* Shade escaping rays against an equirectangular RGBA float32 sky (background_hit, :366-378;
 * horizon rays are black, :242-244) and take the per-pixel mean over the samples (:250).
 * d_end/d_flags are bhg_trace_device outputs for rays laid out [samples][n_pixels];
 * d_rgba [n_pixels][4] fp64, alpha = 1 (:154-155). */
int bhg_shade_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags, size_t n_pixels,
                     int32_t samples, const float *d_sky, int32_t sky_w, int32_t sky_h, double *d_rgba,
                     void *stream);

/* The same with the scene the later engines add: rays that ended on the thin disk
 * (BHG_FLAG_HIT_DISK) get texture(texture_x, scale) * intensity with the Gaussian radial profile of
 * checkHitDisk (LimitedRelativisticRenderEngine.py:427-436, :300); rays that ended on an object sphere
 * (BHG_FLAG_HIT_OBJECT) get the Lambert point-lamp sum of spacetime_hit (RelativisticRenderEngine.py:
 * 341-363; light paths are straight, shadowed by the other spheres, n.l clamped at 0) times the sphere's
 * colour.  The struct lives on the HOST; d_* members are device addresses.  d_disk_tex may be NULL
 * (white); d_object_id may be NULL when n_spheres is 0. */
typedef struct bhg_scene {
    const float *d_sky;      /* [sky_h][sky_w][4] RGBA float32, equirectangular */
    int32_t sky_w, sky_h;
    const float *d_disk_tex; /* [disk_h][disk_w][4] RGBA float32 */
    int32_t disk_w, disk_h;
    double disk_r_in, disk_r_out;                                  /* 0, 0 = no disk */
    double disk_phase, disk_mean, disk_stddev, disk_intensity;     /* scene.disk_* (:55-58; defaults 0, 0.2, 0.3, 1) */
    int32_t n_spheres, n_lamps;                                    /* <= BHG_MAX_SPHERES, <= 4 */
    double spheres[BHG_MAX_SPHERES][4];                            /* as for bhg_trace_objects */
    double sphere_rgb[BHG_MAX_SPHERES][3];
    double lamps[4][4];                                            /* {x, y, z, intensity} (intensity = 10 at :317) */
} bhg_scene;
int bhg_shade_scene_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags, const int8_t *d_object_id,
                           size_t n_pixels, int32_t samples, const bhg_scene *scene, double *d_rgba, void *stream);
/* The same, written as float RGBA -- what Blender's layer.rect takes (RelativisticRenderEngine.py:163-164) --
 * and optionally scattered: d_scatter [n_pixels] (or NULL) gives, for each of this call's pixels, its index in
 * d_rgba_f32 (e.g. y*width + x for a GPU's tile shard, so the shard lands in frame order). */
int bhg_shade_scene_f32_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags,
                               const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                               float *d_rgba_f32, const int64_t *d_scatter, void *stream);

/* Sky-only shading + sample mean from exit directions alone (d_end_dir [samples*n_pixels][3] of bhg_trace_dir_device):
 * the same kernel, same filter and same bits as bhg_shade_device / bhg_shade_scene_f32_device on the records those
 * directions are halves of.  d_rgba (fp64 [n_pixels][4]) and / or d_rgba_f32 (float RGBA, optionally scattered by
 * d_scatter) -- either may be NULL, not both. */
int bhg_shade_dir_device(bhg_context *ctx, const double *d_end_dir, const uint8_t *d_flags, size_t n_pixels,
                         int32_t samples, const float *d_sky, int32_t sky_w, int32_t sky_h, double *d_rgba,
                         float *d_rgba_f32, const int64_t *d_scatter, void *stream);

/* Frame end on the root GPU of a sharded frame: the ranks' float RGBA slabs, gathered into one block
 * d_slabs [n_ranks * slab_pixels][4], are put into frame order, d_frame[p] = d_slabs[d_index[p]] for the n_pixels
 * pixels of the frame (d_index: the frame's permutation, computed once by the host from the tile dealing). */
int bhg_assemble_frame_f32_device(bhg_context *ctx, const float *d_slabs, const int64_t *d_index, size_t n_pixels,
                                  float *d_frame, void *stream);

/* --- the whole frame, owned by the library: one process, one or several GPUs, no PyTorch ------------------------
 * Replaces the body of the reference's frame loop as Blender calls it -- render() (RelativisticRenderEngine.py:50) ->
 * render_scene() (:152-168) -> ray_trace() (:172-267) on ONE render thread of ONE process; the author's commented-out
 * mp.Pool (:210-216) marks where the parallelism has to live.  A bhg_frame holds, per listed device, a context, that
 * device's tiles of the image (tile x tile pixels, all samples of a pixel on one device), its camera rays (generated on
 * the device from the MT19937 jitter stream, :185-230), result buffers and the scene's images; bhg_frame_render() runs
 * rays -> trace -> shade + sample mean on every device at once (one host thread enqueues, the devices work
 * concurrently), gathers the devices' float-RGBA slabs onto the FIRST listed device with ONE exchange per frame, puts
 * them into frame order there and copies one [height][width][4] float array back -- what layer.rect takes (:163-164).
 *
 *   devices   device indices, n_devices >= 1.  An index may be repeated (e.g. {0, 0}): the frame is then sharded over
 *             several contexts of ONE GPU and gathered by device-to-device copies -- the only way to run the N > 1 code
 *             path on a one-GPU machine, and bit-for-bit the image N distinct GPUs give (every ray is its own ODE).
 *   jitter    HOST array, the full-frame stream [samples][height][width][2] of random.random() draws after
 *             random.seed(sampling_seed) (:189), or NULL = pixel centres.  Copied; not referenced after the call.
 *   tile      tile edge in pixels (<= 0: 32).
 *   gather    BHG_FRAME_GATHER_AUTO: RCCL in single-process mode (ncclCommInitAll, grouped ncclSend / ncclRecv on the
 *             contexts' streams -- librccl.so is loaded at run time) when the listed devices are distinct and RCCL loads,
 *             else device-to-device copies (hipMemcpyPeerAsync over xGMI; same-device copies for a repeated device);
 *             _COPY / _RCCL force one (RCCL with a repeated device is BHG_E_INVALID; with ONE device it sends the
 *             frame's slab to itself -- the whole gather path on a single GPU, for tests).
 *             BHG_FRAME_GATHER_PEER (never chosen by AUTO): no exchange at all -- every device's shade kernel stores its
 *             pixels straight into the first device's image, in frame order, over xGMI peer access (16-byte stores in
 *             512-byte runs per tile row); no slabs, no gather, no assembly kernel, and the first device has no more to
 *             do than the others.  Needs peer access from every listed device to the first (else BHG_E_HIP).
 * Tiles are dealt cyclically ((tile_x + tile_y) mod n_devices) until bhg_frame_rebalance() re-deals them by the
 * MEASURED cost of the last render (attempted steps per tile, longest-processing-time-first across devices, each
 * device visiting its tiles longest first): the engine renders the same view sample after sample and frame after
 * frame (:242-250), so the last pass prices the next.  Results never depend on the dealing.
 * Threading: like a context -- one call at a time per frame. */
#define BHG_FRAME_GATHER_AUTO 0
#define BHG_FRAME_GATHER_COPY 1
#define BHG_FRAME_GATHER_RCCL 2
#define BHG_FRAME_GATHER_PEER 3
#define BHG_FRAME_GATHER_COPY_PEERCALL 4   /* _COPY with hipMemcpyPeerAsync on EVERY pair, contexts of one device included (bhg_frame_info
                                              reports _COPY): the N-device copy call, its arguments and stream order on a one-GPU box */
typedef struct bhg_frame bhg_frame;
/* The scene of a frame; everything lives on the HOST and is copied by bhg_frame_set_scene (images are uploaded to
 * every device on the next render).  Members as in bhg_scene.  sky = NULL keeps the current sky image (the first call
 * must bring one); disk_tex = NULL keeps the current disk texture (white if there never was one). */
typedef struct bhg_frame_scene {
    const float *sky;        /* [sky_h][sky_w][4] RGBA float32, equirectangular, rows bottom-up (v = -1 is row 0) */
    int32_t sky_w, sky_h;
    const float *disk_tex;   /* [disk_h][disk_w][4] */
    int32_t disk_w, disk_h;
    double disk_r_in, disk_r_out;                                /* 0, 0 = no disk; must equal the trace parameters' */
    double disk_phase, disk_mean, disk_stddev, disk_intensity;
    int32_t n_spheres, n_lamps;                                  /* <= BHG_MAX_SPHERES, <= 4 */
    double spheres[BHG_MAX_SPHERES][4];                          /* BH-centred {cx, cy, cz, radius} */
    double sphere_rgb[BHG_MAX_SPHERES][3];
    double lamps[4][4];                                          /* {x, y, z, intensity} */
} bhg_frame_scene;
int bhg_frame_create(const int32_t *devices, int32_t n_devices, const bhg_camera *cam, const double *jitter, int32_t tile,
                     int32_t gather, bhg_frame **out);
void bhg_frame_destroy(bhg_frame *frame);
int bhg_frame_set_scene(bhg_frame *frame, const bhg_frame_scene *scene);
/* Move the camera of an existing frame -- what the engine reads anew on every render, origin and rotation of
 * depsgraph.scene.camera.matrix_world (RelativisticRenderEngine.py:182-183), field of view (:72-73) -- while the frame object,
 * its jitter stream (re-seeded identically every render, :189), tile dealing and device buffers stay: origin, rotation and field of view may change, width / height / samples may not.  A new origin costs
 * nothing (rays are directions; the origin goes into every trace call); a new rotation or field of view regenerates the
 * rays on the devices at the next render.  Once an observer is set (bhg_frame_set_observer, ABI 10), a new origin -- or new
 * trace parameters with another metric -- regenerates the rays at the next render too: the observer's tetrad depends on
 * the camera's position. */
int bhg_frame_set_camera(bhg_frame *frame, const bhg_camera *cam);
/* One frame.  rgba_host [height][width][4] float (pageable or page-locked): blocking, the image is there on return.
 * rgba_host = NULL: the render is only enqueued and the image stays on the first device (bhg_frame_device_image;
 * bhg_frame_synchronize waits) -- an animation loop that consumes frames on the GPU, and what bench.py times.
 * A sky-only scene is traced direction-only (bhg_trace_dir_device); with a disk or objects, whole end records. */
int bhg_frame_render(bhg_frame *frame, const bhg_params *p, float *rgba_host);
int bhg_frame_synchronize(bhg_frame *frame);
const float *bhg_frame_device_image(bhg_frame *frame); /* device address (first listed device) of the last image */
/* Re-deal the tiles by the measured cost of the last render (see above); the next render regenerates the rays.
 * root_share in (0, 1] (0 = 1): the part of an equal share the FIRST device is dealt -- it also receives the gather and
 * assembles the frame, and with a smaller shard all devices finish together (e.g. 1 - (N-1)/N * t_root / t_trace from
 * bhg_frame_last_ms). */
int bhg_frame_rebalance(bhg_frame *frame, double root_share);
/* out = {rays, attempted steps, accepted steps, horizon rays} of the last render, summed over the devices (waits). */
int bhg_frame_stats(bhg_frame *frame, uint64_t out[4]);
/* out = {n_devices, gather mode in use (BHG_FRAME_GATHER_COPY / _RCCL), largest shard in pixels, smallest shard,
 * tile, 1 if dealt by measured cost, renders so far, 1 if the last render traced directions only}. */
int bhg_frame_info(const bhg_frame *frame, int64_t out[8]);
/* The bhg_prefix of the last render's trace call on the frame's device number `shard`: what it asked of the rays' start-up
 * records (mode), what the library answered (used) and the records' rho -- BHG_PREFIX_NONE throughout before the first such
 * call and with BHGEO_START_CACHE=0 or BHGEO_START_PREFIX=0.  For tests and diagnosis. */
int bhg_frame_prefix_info(const bhg_frame *frame, int32_t shard, bhg_prefix *last);
/* Per-render timing.  While profiling is on (a flag: it may be switched from render to render, e.g. on for every 4th
 * frame of a timed loop) every render records a HIP event pair around its trace call on each device's stream;
 * bhg_frame_last_ms waits for them and gives the MEAN trace-call milliseconds per listed device over the profiled
 * renders since the last call (trace_ms [n_devices]; for the Schwarzschild forms the call is the one trace kernel) and
 * the root's gather-wait + assembly time of the last profiled render (root_ms, may be NULL; 0 for a one-device frame). */
int bhg_frame_set_profiling(bhg_frame *frame, int enable);
int bhg_frame_last_ms(bhg_frame *frame, float *trace_ms, float *root_ms);
/* The frame's tile dealing as a function of its own (host only, no device needed): the flat pixel ids y * width + x
 * of device `rank` of `world`, tile after tile, row-major inside a tile.  tile_cost NULL: cyclic dealing; else one
 * figure per tile (row-major over the tile grid): dealt by cost ranking (root_share in (0, 1]: rank 0's part of an equal
 * share, see bhg_frame_rebalance) and, visit_by_cost != 0, visited longest first.  pixels NULL: only the count is
 * returned in *n_out. */
int bhg_deal_tiles(int32_t width, int32_t height, int32_t tile, int32_t world, const double *tile_cost, int32_t visit_by_cost,
                   double root_share, int32_t rank, int64_t *pixels, size_t capacity, size_t *n_out);

/* --- redshift (ABI 9) --------------------------------------------------------------------------
 * g = nu_obs / nu_em = (k.u_obs) / (k.u_em) per ray.  The observer is the ZAMO (zero-angular-momentum observer) at the
 * camera -- in Schwarzschild the static observer; the ray's Killing constants come from its CAMERA state (x0, k0), not from
 * its end record; the photon it receives runs the traced curve backwards (Kerr: mirrored in phi, by the (t, phi) -> (-t, -phi)
 * symmetry, with the same E and L -- so the traced picture's disk has the opposite sense).  Emitters: the thin disk in
 * Keplerian circular orbits of sense disk_sense (+1 = counter-clockwise seen from +z, -1 = clockwise: the half moving
 * towards the camera is blueshifted), treated as Keplerian down to the photon orbit (inside the ISCO too: the model's choice); an
 * object sphere at rest (Schwarzschild: static; Kerr: the ZAMO at the hit point); the sky at rest at infinity.  By flags:
 * horizon and start-inside rays g = 0, BHG_FLAG_NAN rays NaN, BHG_FLAG_HIT_DISK / _HIT_OBJECT rays the disk / object g,
 * every other ray (exit sphere, lambda_end, step cap, stall: the rays the shader colours from the sky) the sky's g.
 * Shading with redshift multiplies a ray's RGB by g^exponent when its class is in `apply` (4: bolometric intensity,
 * 3: specific intensity at a fixed frequency); hues are not changed.  Refused (BHG_E_INVALID): time_like = 1, a disk
 * whose r_in lies at or inside the circular photon orbit of the traced picture's sense s = -disk_sense (Schwarzschild 3M;
 * Kerr 2M[1 + cos(2/3 arccos(-s a / M))], in Boyer-Lindquist r = sqrt(r_in^2 - a^2)), a disk_sense other than +-1, an exponent
 * that is not finite, apply bits outside BHG_REDSHIFT_DISK | _OBJECTS | _SKY.  The calls use no context workspace: each
 * is one launch on the stream it is given, ordered like any other work on that stream. */
#define BHG_REDSHIFT_DISK 1u
#define BHG_REDSHIFT_OBJECTS 2u
#define BHG_REDSHIFT_SKY 4u
typedef struct bhg_redshift {
    uint32_t apply;       /* BHG_REDSHIFT_* classes whose colour is weighted by g^exponent; 0 = off */
    int32_t disk_sense;   /* +1 or -1 */
    double exponent;      /* 4 = bolometric, 3 = specific intensity */
} bhg_redshift;
size_t bhg_redshift_size(void);
/* d_g [n] = g of every ray of a bhg_trace*_device call (whatever `apply` says): x0_shared (HOST [3]) or d_x0 [n][3] and
 * d_k0 [n][3] as given to the trace, its d_end [n][6] (may be NULL: then disk and object rays get NaN) and d_flags [n].
 * p: the trace's parameters (metric, spin, disk).  Enqueues one launch on `stream` and returns. */
int bhg_redshift_device(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const double *x0_shared,
                        const double *d_x0, const double *d_k0, const double *d_end, const uint8_t *d_flags, size_t n,
                        double *d_g, void *stream);
/* The same on HOST arrays (x0_is_shared != 0: x0 is [3], else [n][3]; end may be NULL); blocking, on the context's stream.
 * (Named _host: in C the struct's typedef name bhg_redshift and a function of that name cannot coexist.) */
int bhg_redshift_host(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const double *x0, int x0_is_shared,
                      const double *k0, const double *end, const uint8_t *flags, size_t n, double *g);
/* bhg_shade_scene_device / _f32_device / bhg_shade_dir_device with redshift: each ray's colour is weighted by g^exponent
 * inside the shade kernel (no g array).  The camera: x0_shared (HOST [3]) and d_k0 [samples * n_pixels][3], the directions
 * the rays were traced from; p: the trace's parameters.  d_end [n][6] as there, or NULL for a direction-only sky frame:
 * then d_end_dir [n][3] (bhg_trace_dir_device) and a scene without disk and spheres.  d_rgba (fp64) and / or d_rgba_f32
 * (float RGBA, optionally scattered by d_scatter) -- either may be NULL, not both.  rs = NULL or apply = 0: exactly the
 * call without redshift, bit for bit. */
int bhg_shade_scene_redshift_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                    const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                    const bhg_params *p, const bhg_redshift *rs, const double *x0_shared,
                                    const double *d_k0, double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter,
                                    void *stream);
/* Redshift in every later bhg_frame_render (every device, every gather mode; direction-only sky frames stay direction-only).
 * rs = NULL or apply = 0: the frame without redshift, bit for bit.  Checked against the trace parameters at render. */
int bhg_frame_set_redshift(bhg_frame *frame, const bhg_redshift *rs);

/* --- the observer camera (ABI 10) --------------------------------------------------------------
 * The reference camera uses each pixel's pinhole direction d as the COORDINATE direction k0 at the camera.  The observer
 * camera reads d as a unit look direction n' in the rest frame of an observer at the camera moving with velocity beta
 * relative to the local ZAMO (world axes; in Schwarzschild the ZAMO is the static observer).  n' is aberrated to the ZAMO
 * frame, n = (n' + gamma^2/(gamma+1) (n'.beta) beta - gamma beta) / (gamma (1 - beta.n')), and put through the ZAMO tetrad:
 * Schwarzschild (both Cartesian forms) k = n - (1 - sqrt f)(n.r^) r^; Kerr (k^r, k^th, k^ph) = (sqrt(Delta/Sigma) n_r,
 * n_th / sqrt(Sigma), omega/alpha + n_ph sqrt(Sigma) / (sqrt(A) sin th)) with n on the Euclidean spherical basis at the
 * camera's BL angles, mapped to Cartesian by the Jacobian of the BL embedding.  k0 is normalised to unit Euclidean length
 * (the trace's affine-parameter convention is unchanged).  beta = 0 is the ZAMO's own picture -- NOT the reference
 * camera's.  The redshift g of a moving observer is the ZAMO's g times gamma (1 + beta.n), n recovered from (x0, k0).
 * Refused (BHG_E_INVALID): |beta| >= 1 or non-finite, a camera at or inside the horizon (r_s; Kerr BL r_+ = M + sqrt(M^2 -
 * a^2)), a Kerr camera at or inside the ergosurface r_E(theta) = M + sqrt(M^2 - a^2 cos^2 theta) (there g_tt > 0 and the
 * start conversion's root of the null condition, which the trace and the redshift take k^t from, is not always the
 * tetrad's), time_like = 1, a Kerr camera exactly on the BL axis (x = y = 0).  Near the axis the azimuthal basis vector is
 * formed from x / w, y / w (w = sqrt(x^2 + y^2)) and frame dragging enters as omega R sin th: both stay well conditioned,
 * but kerr_cart_to_bl's theta carries a relative error of about eps / (1 - cos theta), which the rays inherit.  Every call
 * below takes obs = NULL as "no observer": then it is exactly its ABI 9 counterpart, bit for bit.  Per-ray origins
 * (d_x0 of bhg_redshift_observer_device) are not checked against the horizon. */
typedef struct bhg_observer {
    double beta[3];       /* world axes, relative to the ZAMO at the camera, |beta| < 1 */
} bhg_observer;
size_t bhg_observer_size(void);
/* bhg_raygen_device for an observer at x0 (HOST [3], BH-centred) in the metric of p (r_s, spin, rhs_form). */
int bhg_raygen_observer_device(bhg_context *ctx, const bhg_params *p, const bhg_observer *obs, const double *x0, int32_t width,
                               int32_t height, int32_t samples, double fov_x, double fov_y, const double *rot9,
                               const double *d_jitter, const int64_t *d_pixels, size_t n_pixels, double *d_k0, void *stream);
/* bhg_redshift_device / _host / bhg_shade_scene_redshift_device with g of the moving observer. */
int bhg_redshift_observer_device(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                 const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                                 const uint8_t *d_flags, size_t n, double *d_g, void *stream);
int bhg_redshift_observer_host(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                               const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags,
                               size_t n, double *g);
int bhg_shade_scene_redshift_observer_device(bhg_context *ctx, const double *d_end, const double *d_end_dir,
                                             const uint8_t *d_flags, const int8_t *d_object_id, size_t n_pixels,
                                             int32_t samples, const bhg_scene *scene, const bhg_params *p,
                                             const bhg_redshift *rs, const bhg_observer *obs, const double *x0_shared,
                                             const double *d_k0, double *d_rgba, float *d_rgba_f32,
                                             const int64_t *d_scatter, void *stream);
/* The observer camera in every later bhg_frame_render (every device, every gather mode; with redshift, g is the observer's).
 * obs = NULL: the reference camera again, bit for bit.  The rays are regenerated at the next render, and again whenever
 * the origin or the trace parameters' metric changes.  Checked against the camera and the trace parameters at render. */
int bhg_frame_set_observer(bhg_frame *frame, const bhg_observer *obs);

/* --- textured, oriented and emissive object spheres (within ABI 10) ----------------------------
 * Each object sphere j gets an optional equirectangular RGBA float32 texture (rows bottom-up, as the sky), an orientation R_j
 * (row-major, body -> world; the all-zero matrix means the identity, so a zero-initialised struct is valid) and a shading mode.
 * For a ray that ends on sphere j at the entry point e: n = (e - c_j) / rho_j, n_b = R_j^T n, and the texel is read with the
 * sky's bilinear filter (u wraps, v clamps) at U = atan2(n_b,y, n_b,x) / pi, V = 1 - 2 atan2(sqrt(n_b,x^2 + n_b,y^2), n_b,z) / pi:
 * body +x is the image's centre column, body +z its top row.  A slot without a texture has a white texel.
 *   BHG_OBJECT_LIT:      colour = sphere_rgb[j] * (the Lambert lamp sum with shadow rays) * texel
 *   BHG_OBJECT_EMISSIVE: colour = emission[j] * sphere_rgb[j] * texel (no lamps, no shadows)
 * Redshift weighs the colour as any object ray's (the emitter at rest, or moving: section 14).  Refused (BHG_E_INVALID, the
 * message names the sphere index), for slots below n_spheres only: a mode other than 0 / 1, a non-finite or negative emission, a texture with
 * w or h < 1, a rotation that is neither all-zero nor orthonormal with det +1 (|R^T R - I| <= 1e-9).
 * Member order: tex, tex_w, tex_h, mode, emission, rot (800 bytes). */
#define BHG_OBJECT_TEXTURES 1
#define BHG_OBJECT_LIT 0
#define BHG_OBJECT_EMISSIVE 1
typedef struct bhg_object_textures {
    const float *tex[BHG_MAX_SPHERES];      /* [tex_h][tex_w][4] RGBA float32, or NULL (white) */
    int32_t tex_w[BHG_MAX_SPHERES], tex_h[BHG_MAX_SPHERES];
    int32_t mode[BHG_MAX_SPHERES];          /* BHG_OBJECT_LIT / BHG_OBJECT_EMISSIVE */
    double emission[BHG_MAX_SPHERES];       /* emissive strength, finite and >= 0 */
    double rot[BHG_MAX_SPHERES][9];         /* row-major body -> world rotation, or all zero (the identity) */
} bhg_object_textures;
size_t bhg_object_textures_size(void);
/* bhg_shade_scene_redshift_observer_device with textured object spheres; tex[] holds DEVICE addresses.  ot = NULL is exactly
 * that call, bit for bit; any other ot takes the textured kernel instances, and a zero-initialised ot gives that call's image
 * bit for bit (a white texel is an exact x 1.0).
 * This is the general shade call: every other bhg_shade*_device is this call with some arguments NULL (bhg_shade_device and
 * bhg_shade_dir_device with a scene of the sky alone).  All of them check in this order, so that settings are refused with or
 * without a device:
 *   1. the scene: not NULL; samples, sky_w, sky_h > 0; n_spheres in [0, BHG_MAX_SPHERES], n_lamps in [0, 4]; a disk with
 *      r_out > r_in, stddev > 0 and (with a texture) disk_w, disk_h > 0; sphere radii > 0
 *   2. ot, when not NULL, against n_spheres
 *   3. with rs->apply != 0: x0_shared not NULL, the redshift settings against p, then obs when not NULL
 *   4. ctx not NULL
 *   5. n_pixels == 0: BHG_OK, no device array is looked at (an empty shard)
 *   6. the device arrays: d_rgba or d_rgba_f32; d_end or d_end_dir; d_flags and the sky; d_end when the scene has a disk or
 *      spheres; d_object_id when it has spheres; d_k0 with redshift on */
int bhg_shade_scene_textured_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                    const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                    const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                    const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                    float *d_rgba_f32, const int64_t *d_scatter, void *stream);
/* Textured object spheres in every later bhg_frame_render (every device, every gather mode) whose scene has spheres.  tex[]
 * holds HOST arrays: they are copied here and uploaded to every device at the next render.  A NULL tex[j] keeps that slot's
 * current texture (white if it never had one), as disk_tex does in bhg_frame_set_scene; a call that changes only rotations,
 * modes or strengths uploads nothing.  ot = NULL turns textures off (the frame's shading without them, bit for bit) and frees
 * them.  Slots are checked against the scene's n_spheres here and again at render; slots at or above it are ignored.  A
 * refused host copy is BHG_E_NOMEM and leaves the frame as it was. */
int bhg_frame_set_object_textures(bhg_frame *frame, const bhg_object_textures *ot);

/* --- disk polarisation (within ABI 10) ---------------------------------------------------------
 * The linear polarisation of the thin disk's light at the camera: the emission is polarised in the disk plane and
 * perpendicular to the photon in the fluid frame (electron scattering), f ~ z^ x n_f, with a degree delta the caller tabulates
 * against the emission cosine mu = |n_f . z^|.  f is carried to the camera by the Walker-Penrose constant
 *     kappa = (A - i B)(r - i a cos th),  A = (k^t f^r - k^r f^t) + a sin^2 th (k^r f^ph - k^ph f^r),
 *                                         B = [(r^2 + a^2)(k^ph f^th - k^th f^ph) - a (k^t f^th - k^th f^t)] sin th
 * (BL coordinates; Schwarzschild at a = 0) of the traced ray, with k at the disk rebuilt from the camera state's constants
 * (Kerr E, L_z, Carter Q; Schwarzschild E and x x k) and only the signs of k^r, k^th taken from the end record.  The disk is
 * redshift's Keplerian disk of sense disk_sense (section 9: the traced picture's sense is -disk_sense).  On the screen of the
 * camera's observer -- the ZAMO, or with obs the moving observer of section 10 -- with the ray's look direction n and image
 * up `up` (world axes): e_up = normalise(up - (up.n) n), e_left = e_up x n, and
 *     chi = atan2(c_L, c_U) in (-pi/2, pi/2],  kappa_em = c_L kappa(k_c, E_left) + c_U kappa(k_c, E_up),
 * measured from image up towards image left (the IAU convention).  up along n, or f = 0 (the photon leaves along the disk
 * normal, mu = 1): chi = NaN, delta and mu as for any disk ray, and no contribution to Q and U.
 * Per ray, by flags: BHG_FLAG_HIT_DISK rays (chi, delta, mu); BHG_FLAG_NAN rays, and disk rays without an end record, NaN;
 * every other ray 0 (objects and sky are unpolarised).
 * Refused (BHG_E_INVALID, the message names the figure), before the context: disk_sense other than +-1; n_degree outside
 * [1, BHG_POL_TABLE_MAX]; a degree that is not finite or outside [0, 1]; an up that is not finite or zero; time_like = 1; a disk
 * r_in at or inside the photon orbit of the traced sense (section 9's rule); a redshift disk_sense that differs from this one
 * when both are given; a shared camera at or inside the horizon, inside the Kerr ergosurface or exactly on the Kerr BL axis
 * (section 10's rules, with or without obs).
 * Member order: disk_sense, n_degree, up, degree (544 bytes). */
#define BHG_POLARISATION 1
#define BHG_POL_TABLE_MAX 64
typedef struct bhg_polarisation {
    int32_t disk_sense;                 /* +1 / -1, bhg_redshift's meaning */
    int32_t n_degree;                   /* 1 .. BHG_POL_TABLE_MAX */
    double up[3];                       /* image up, world axes at the camera */
    double degree[BHG_POL_TABLE_MAX];   /* delta(mu_j), mu_j = j / (n_degree - 1), linear between; in [0, 1] */
} bhg_polarisation;
size_t bhg_polarisation_size(void);
/* Per ray, from the camera state (x0_shared [3] HOST, or d_x0 [n][3]; d_k0 [n][3]), d_end [n][6] (or NULL) and d_flags [n]:
 * d_evpa [n] = chi, d_degree [n] = delta, d_mu [n] = mu (d_mu may be NULL).  obs NULL: the ZAMO's screen.  One launch on
 * stream; no context workspace. */
int bhg_polarisation_device(bhg_context *ctx, const bhg_params *p, const bhg_polarisation *pol, const bhg_observer *obs,
                            const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                            const uint8_t *d_flags, size_t n, double *d_evpa, double *d_degree, double *d_mu, void *stream);
/* bhg_polarisation_device on host arrays (x0 [3] with x0_is_shared != 0, else [n][3]; end may be NULL; mu may be NULL). */
int bhg_polarisation_host(bhg_context *ctx, const bhg_params *p, const bhg_polarisation *pol, const bhg_observer *obs,
                          const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags,
                          size_t n, double *evpa, double *degree, double *mu);
/* bhg_shade_scene_textured_device with the Stokes images: d_qu [n_pixels][6] fp64 = the per-pixel means (in sample order) of
 * (Q_r, Q_g, Q_b, U_r, U_g, U_b), Q_c = delta cos 2chi rgb_c, U_c = delta sin 2chi rgb_c, rgb_c the ray's final colour (disk
 * texture, g^n with redshift); written at pixel p, never scattered.  The colour outputs are bit for bit those of the textured
 * call.  pol = NULL is exactly the textured call (which is this call with pol = NULL: one implementation, one checking order:
 * after step 3 of the textured call's, pol against p and x0_shared -- which it needs -- and the redshift's disk_sense; in step
 * 6, d_qu and d_k0). */
int bhg_shade_scene_polarised_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                     const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                     const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                     const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                     float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                     void *stream);

/* --- the thermal disk (within ABI 10) ----------------------------------------------------------
 * The thin disk as a Novikov-Thorne disk: the Page-Thorne (1974) flux of the circular-orbit family redshift's disk moves on
 * (sense disk_sense, section 9; a* = s a / M with s = -disk_sense, M = r_s / 2, Kerr's BL r = sqrt(R^2 - a^2) of the hit,
 * Schwarzschild's r = R), zero at and inside the family's r_ms (Bardeen-Press-Teukolsky), as a temperature
 *     T(r) = t_peak (F(r) / max F)^(1/4)       (max over the disk's family, found by the library in double)
 * and the colour-corrected blackbody f_col^-4 B_nu(f_col T) it emits, which the camera sees redshifted by the ray's g (the g of
 * bhg_redshift_device, with obs that of bhg_redshift_observer_device): a blackbody at g f_col T.  The library ships no colour
 * data: each of R, G, B is a weighted sum over the caller's n_nu frequencies nu_j [Hz] (weights of any sign), in units of
 * nu0 = k_B t_peak / h:
 *     I_c = scale sum_j weight[c][j] nuh_j^3 / (f_col^4 expm1(nuh_j / (g f_col tau))),  nuh_j = nu_j / nu0,  tau = T / t_peak
 * Per ray, by flags: BHG_FLAG_HIT_DISK rays (T, I_R, I_G, I_B), 0 at and inside r_ms; BHG_FLAG_NAN rays, and disk rays without an
 * end record, NaN; every other ray 0.  In the shade, (I_R, I_G, I_B) replaces a disk ray's colour (texture and radial profile
 * are not used) and is not weighted by g^n again; objects and sky are weighted as rs says; Q / U (pol) take it as the ray's I.
 * Refused (BHG_E_INVALID, the message names the figure), before the context: disk_sense other than +-1; n_nu outside
 * [1, BHG_THERMAL_NU_MAX]; a nu that is not finite or not > 0; a weight that is not finite; t_peak or f_col not finite or not
 * > 0; scale not finite; time_like = 1; a disk r_in at or inside the photon orbit of the traced sense (section 9's rule); a
 * redshift or polarisation disk_sense that differs from this one; a shared camera at or inside the horizon, inside the Kerr
 * ergosurface or exactly on the Kerr BL axis (section 10's rules).
 * Member order: disk_sense, n_nu, t_peak, f_col, scale, nu, weight (544 bytes). */
#define BHG_DISK_THERMAL 1
#define BHG_THERMAL_NU_MAX 16
typedef struct bhg_disk_thermal {
    int32_t disk_sense;                             /* +1 / -1, bhg_redshift's meaning */
    int32_t n_nu;                                   /* 1 .. BHG_THERMAL_NU_MAX */
    double t_peak;                                  /* the largest emitted temperature over the disk [K] */
    double f_col;                                   /* colour correction (1: a plain blackbody) */
    double scale;                                   /* overall factor of I_c */
    double nu[BHG_THERMAL_NU_MAX];                  /* frequencies [Hz], shared by the channels */
    double weight[3][BHG_THERMAL_NU_MAX];           /* R, G, B weights of each frequency */
} bhg_disk_thermal;
size_t bhg_disk_thermal_size(void);
/* Per ray, from the camera state (x0_shared [3] HOST, or d_x0 [n][3]; d_k0 [n][3]), d_end [n][6] (or NULL) and d_flags [n]:
 * d_t_em [n] = T [K], d_rgb [n][3] = (I_R, I_G, I_B).  obs NULL: the ZAMO's g.  One launch on stream; no context workspace. */
int bhg_disk_thermal_device(bhg_context *ctx, const bhg_params *p, const bhg_disk_thermal *th, const bhg_observer *obs,
                            const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                            const uint8_t *d_flags, size_t n, double *d_t_em, double *d_rgb, void *stream);
/* bhg_disk_thermal_device on host arrays (x0 [3] with x0_is_shared != 0, else [n][3]; end may be NULL). */
int bhg_disk_thermal_host(bhg_context *ctx, const bhg_params *p, const bhg_disk_thermal *th, const bhg_observer *obs,
                          const double *x0, int x0_is_shared, const double *k0, const double *end, const uint8_t *flags, size_t n,
                          double *t_em, double *rgb);
/* bhg_shade_scene_polarised_device with the thermal disk: a disk ray's colour is its I_c (above).  th = NULL is exactly the
 * polarised call (which is this call with th = NULL: one implementation, one checking order: after step 3b, th against p, the
 * scene's disk, the redshift's and polarisation's disk_sense, x0_shared -- which it needs -- and obs; in step 6, d_k0). */
int bhg_shade_scene_thermal_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                   const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                   const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                   const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                   float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                   const bhg_disk_thermal *th, void *stream);
/* The thermal disk in every later render of the frame (its shade calls are bhg_shade_scene_thermal_device).  NULL: off, the
 * frame as without it.  The settings that need no trace parameters are checked here, the rest at every render. */
int bhg_frame_set_disk_thermal(bhg_frame *frame, const bhg_disk_thermal *th);

/* --- moving and spinning object spheres (within ABI 10) --------------------------------------------
 * Each object sphere j {c_j, rho_j} gets a centre velocity v[j] and an angular velocity w[j]: world axes, coordinate
 * quantities (dx/dt and rad per unit t, t the Schwarzschild / Boyer-Lindquist time; c = 1, lengths in the units of r_s).  Its
 * surface point x moves with V(x) = v[j] + w[j] x (x - c_j).  The sphere stays where the scene puts it (no retarded
 * positions).  The emitter of an object ray that ends on a moving sphere at x:
 *   Schwarzschild (both Cartesian forms)  u = u^t (d_t + V),                   u^t = 1 / sqrt(f - |V|^2 - h (n.V)^2)
 *   Kerr (BL)                             u = u^t (d_t + omega d_phi + V),     u^t = 1 / (alpha sqrt(1 - beta^2)),
 *                                         beta^2 = (g_rr V^r^2 + g_thth V^th^2 + g_phph V^ph^2) / alpha^2
 * V relative to the ZAMO's flow in Kerr; omega d_phi = omega z^ x x in the Cartesian embedding.  Motion is given in the picture
 * disk_sense is given in (section 14 spells out which omega and which Keplerian Omega that is in Kerr).  The photon's momentum
 * at x is rebuilt from the camera state's constants (Schwarzschild: E and the vector L = x0 x k0; Kerr: E, L and Carter's Q),
 * with only the signs of its radial (Kerr: and polar) component from the end record; g = (p.u_obs) / (p.u_em), times the
 * observer's gamma (1 + beta.n) with obs.  A sphere whose v and w are all zero is at rest exactly as without motion (the same
 * formula, bit for bit).  Motion changes only the object rays' g: in the shade their colour (lit: the Lambert colour as it
 * is, the reflected light taken as emitted in the surface's rest frame; emissive: texture x strength) is weighted by g^n when
 * rs->apply has BHG_REDSHIFT_OBJECTS, and not at all otherwise.  Slots at or above n_spheres are not looked at.
 * Refused (BHG_E_INVALID, the message names the sphere), before the context: a v or w that is not finite; a moving sphere
 * that reaches the horizon (Schwarzschild |c| - rho <= r_s; Kerr r_lo = sqrt((|c| - rho)^2 - a^2) <= r_+ or |c| - rho <= |a|);
 * a motion that the sufficient bound does not prove timelike on the whole sphere:
 *   Schwarzschild  |v| + |w| rho < f(|c| - rho)
 *   Kerr           |w_z| max(G(r_lo), G(|c| + rho)) + (|v - w_z z^ x c| + |w_perp| rho) / F(r_lo) < 1,
 *                  G(r) = ((r^2 + a^2)^2 - a^2 Delta) / (r^2 sqrt(Delta)),  F(r) = r Delta / (r^2 + a^2)^(3/2).
 * Member order: v, w (384 bytes); an all-zero struct is every sphere at rest. */
#define BHG_OBJECT_MOTION 1
typedef struct bhg_object_motion {
    double v[BHG_MAX_SPHERES][3];     /* centre velocity dx/dt of each sphere, world axes */
    double w[BHG_MAX_SPHERES][3];     /* angular velocity of each sphere about its centre [rad per unit t], world axes */
} bhg_object_motion;
size_t bhg_object_motion_size(void);
/* bhg_redshift_observer_device / _host with moving object spheres: the spheres [n_spheres][4] {cx, cy, cz, radius} of the
 * trace and its d_object_id [n] (object_id [n] for _host; may be NULL only when no ray hit an object).  motion = NULL: exactly
 * bhg_redshift_observer_device / _host, bit for bit. */
int bhg_redshift_motion_device(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                               const bhg_object_motion *motion, const double *spheres, int32_t n_spheres,
                               const double *x0_shared, const double *d_x0, const double *d_k0, const double *d_end,
                               const uint8_t *d_flags, const int8_t *d_object_id, size_t n, double *d_g, void *stream);
int bhg_redshift_motion_host(bhg_context *ctx, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                             const bhg_object_motion *motion, const double *spheres, int32_t n_spheres, const double *x0,
                             int x0_is_shared, const double *k0, const double *end, const uint8_t *flags, const int8_t *object_id,
                             size_t n, double *g);
/* bhg_shade_scene_thermal_device with moving object spheres: the general shade call.  mo = NULL, or an all-zero mo, is exactly
 * the thermal call (which is this call with mo = NULL: one implementation, one checking order -- after step 2, the motion
 * against n_spheres and the trace parameters). */
int bhg_shade_scene_moving_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                  const int8_t *d_object_id, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                  const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                  const bhg_object_textures *ot, const double *x0_shared, const double *d_k0, double *d_rgba,
                                  float *d_rgba_f32, const int64_t *d_scatter, const bhg_polarisation *pol, double *d_qu,
                                  const bhg_disk_thermal *th, const bhg_object_motion *mo, void *stream);
/* Moving object spheres in every later render of the frame (every device, every gather mode; its shade calls are
 * bhg_shade_scene_moving_device).  NULL: off, the frame as without it.  Checked against the scene's spheres here (those set
 * at this call) and against the scene and the trace parameters at every render. */
int bhg_frame_set_object_motion(bhg_frame *frame, const bhg_object_motion *mo);

/* --- disk crossings and layers: higher-order images of the disk (within ABI 10) ---------------------
 * The disk of bhg_params is opaque: a ray ends at its first plane crossing inside the annulus.  The crossings trace carries
 * the ray THROUGH the disk instead and records every crossing inside the annulus -- scipy's solve_ivp with the disk plane as
 * a non-terminal event g = z (Kerr: cos theta):
 *   - the step sequence is that of the same call with the disk off: disk_r_out plays no part in step control, a crossing
 *     never truncates a step; horizon, exit sphere and lambda_end end the ray as they do there, and end / flags / n_steps /
 *     n_accepted are the disk-off trace's (no ray carries BHG_FLAG_HIT_DISK);
 *   - an accepted step whose ends lie on both sides of the plane (scipy's sign-change rule: at most one root per step) has
 *     its root found by the trace kernels' Brent search on the step's dense output; the crossing counts when its cylindrical
 *     radius lies in [disk_r_in, disk_r_out] and, in the step that holds the ray's terminal event, when it is not later than
 *     that event;
 *   - d_n_cross [n] uint8 counts every crossing (saturating at 255); d_cross [max_crossings][n][6] fp64 holds the first
 *     max_crossings (1 .. BHG_MAX_CROSSINGS) records: the dense-output state at the root, position then direction,
 *     Cartesian.  Records a ray never reached are left as they were.  Rays that start inside have n_cross = 0.
 * The layout is order-major: d_cross + m * n * 6 is an [n][6] end array that bhg_redshift_device, bhg_polarisation_device and
 * bhg_disk_thermal_device take as it stands, with the flag array n_cross > m ? BHG_FLAG_HIT_DISK : BHG_FLAG_HIT_HORIZON.
 * Covered: BHG_METHOD_DP54 with every rhs_form, null rays, no object spheres (one lane per ray; the persistent trace kernels
 * are not involved).  Refused (BHG_E_INVALID), before the context: BHG_METHOD_RK4, time_like = 1, disk_r_out = 0,
 * max_crossings outside [1, BHG_MAX_CROSSINGS].  Otherwise bhg_trace_device's conventions: d_flags / d_n_steps / d_n_accepted
 * may be NULL, asynchronous on stream, calls of more than 2^26 rays are split into launches. */
#define BHG_DISK_CROSSINGS 1
#define BHG_MAX_CROSSINGS 4
int bhg_trace_crossings_device(bhg_context *ctx, const bhg_params *p, const double *x0_shared, const double *d_x0,
                               const double *d_k0, size_t n, int32_t max_crossings, double *d_end, uint8_t *d_flags,
                               uint32_t *d_n_steps, uint32_t *d_n_accepted, double *d_cross, uint8_t *d_n_cross, void *stream);
/* bhg_trace_crossings_device on host arrays (x0 [3] with x0_is_shared != 0, else [n][3]; flags, n_steps, n_accepted may be
 * NULL).  Blocking.  cross is read first, so that records no ray reached come back as the caller left them. */
int bhg_trace_crossings(bhg_context *ctx, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0, size_t n,
                        int32_t max_crossings, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted,
                        double *cross, uint8_t *n_cross);
/* The optically thin disk: every crossing passes the fraction T = 1 - opacity of what lies behind it, 0 < opacity <= 1 (1: the
 * opaque disk -- layer 0 alone, nothing behind it is looked at). */
typedef struct bhg_disk_layers {
    int32_t max_crossings;   /* layers in d_cross, 1 .. BHG_MAX_CROSSINGS */
    int32_t pad;
    double opacity;
} bhg_disk_layers;
size_t bhg_disk_layers_size(void);
/* The layered shade of a crossings trace (d_end or d_end_dir, d_flags, d_cross, d_n_cross of S * n_pixels rays, ray
 * s * n_pixels + p = sample s of pixel p): per ray, with w = 1,
 *     for m < min(n_cross, max_crossings), while w != 0:   rgb += w C(cross[m]);   w *= T
 *     if w != 0 and the ray did not end in the hole:        rgb += w sky(exit direction)
 * then the pixel's samples are summed in sample order and divided by S.  C is the disk colour of
 * bhg_shade_scene_redshift_observer_device for a disk ray with that end record (rs, obs may be NULL) or, th given, of
 * bhg_shade_scene_thermal_device; the sky is weighted as rs says.  The scene needs a disk and no object spheres (refused
 * otherwise, as are the settings those calls refuse, a max_crossings outside [1, BHG_MAX_CROSSINGS] and an opacity outside
 * (0, 1] -- all before the context). */
int bhg_shade_disk_layers_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                 const double *d_cross, const uint8_t *d_n_cross, size_t n_pixels, int32_t samples,
                                 const bhg_scene *scene, const bhg_params *p, const bhg_redshift *rs, const bhg_observer *obs,
                                 const double *x0_shared, const double *d_k0, double *d_rgba, float *d_rgba_f32,
                                 const int64_t *d_scatter, const bhg_disk_thermal *th, const bhg_disk_layers *layers,
                                 void *stream);

/* --- light travel time (within ABI 10) ---------------------------------------------------------------
 * The crossings trace with one more quantity per ray: dt >= 0, the Schwarzschild / Boyer-Lindquist coordinate time that elapses
 * along the ray between its start point and a point on it.  Rays are traced backwards: the light seen at camera time t_c left
 * that point at t_c - dt.  The integrand depends on position and the ray's constants only,
 *     Schwarzschild (both forms):  dt/dlambda = E / (1 - r_s / r),  E = sqrt(f0 (|k0|^2 + h0 (n0.k0)^2)) at the start point,
 *                                  f = 1 - r_s / r, h = r_s / (r - r_s)
 *     Kerr:  dt/dlambda = [E ((r^2 + a^2)^2 - Delta a^2 sin^2 theta) - 2 M a r L] / (Sigma Delta)
 * and is integrated with 6-point Gauss-Legendre per accepted step on the step's dense-output position, summed in step order;
 * the step that holds the terminal event runs to the event's root.  The time of a crossing is the time at the start of its
 * step plus the same rule up to the crossing's root.
 *   - d_t_end [n] fp64: the time to the ray's end state.  +inf for rays flagged BHG_FLAG_HIT_HORIZON or BHG_FLAG_START_INSIDE
 *     and for rays one of whose nodes lay at r <= the horizon radius (a ray that stepped across the hole at loose tolerances:
 *     its time is as unphysical as its path, and the node test does not catch every such ray); NaN for rays flagged
 *     BHG_FLAG_NAN; the time up to the returned state for BHG_FLAG_MAX_STEPS / BHG_FLAG_STEP_TOO_SMALL.
 *   - d_t_cross [max_crossings][n] fp64 beside d_cross: the time of each stored crossing; +inf after such a node, finite in
 *     front of a horizon ending.  Slots a ray never reached are left as they were, like d_cross's.
 *   - everything else -- the steps, d_end, d_flags, d_n_steps, d_n_accepted, d_cross, d_n_cross -- is the crossings trace's on the
 *     same input, bit for bit.
 * max_crossings = 0 is allowed (d_cross, d_t_cross and d_n_cross may then be NULL), and so is disk_r_out = 0 with it: the
 * times to the end only, d_end / d_flags / d_n_steps / d_n_accepted those of bhg_trace_device bit for bit (a lone exit-sphere
 * event is then settled as the trace kernels settle it; d_t_end is the same with or without a disk).  Refused (BHG_E_INVALID), before the context: BHG_METHOD_RK4,
 * time_like = 1, max_crossings outside [0, BHG_MAX_CROSSINGS], max_crossings > 0 with disk_r_out = 0, a NULL t_end. */
#define BHG_TRAVEL_TIME 1
int bhg_travel_time_device(bhg_context *ctx, const bhg_params *p, const double *x0_shared, const double *d_x0,
                           const double *d_k0, size_t n, int32_t max_crossings, double *d_end, uint8_t *d_flags,
                           uint32_t *d_n_steps, uint32_t *d_n_accepted, double *d_cross, uint8_t *d_n_cross, double *d_t_end,
                           double *d_t_cross, void *stream);
/* bhg_travel_time_device on host arrays, as bhg_trace_crossings.  Blocking.  cross and t_cross are read first. */
int bhg_travel_time(bhg_context *ctx, const bhg_params *p, const double *x0, int x0_is_shared, const double *k0, size_t n,
                    int32_t max_crossings, double *end, uint8_t *flags, uint32_t *n_steps, uint32_t *n_accepted, double *cross,
                    uint8_t *n_cross, double *t_end, double *t_cross);
/* bhg_shade_disk_layers_device with each layer drawn at the phase the disk had when the light left it: layer m of ray i is
 * coloured with disk_phase - phase_rate * t_cross[m][i], phase_rate = d(disk_phase)/dt as the caller animates it (radians per
 * unit of coordinate time), d_t_cross [max_crossings][S * n_pixels] from bhg_travel_time_device.  A layer whose time is not
 * finite contributes black and still absorbs.  The thermal disk (th given) has no texture to turn: the times change nothing.
 * phase_rate = 0 or d_t_cross = NULL is bhg_shade_disk_layers_device, kernel for kernel. */
int bhg_shade_disk_layers_retarded_device(bhg_context *ctx, const double *d_end, const double *d_end_dir, const uint8_t *d_flags,
                                          const double *d_cross, const uint8_t *d_n_cross, size_t n_pixels, int32_t samples,
                                          const bhg_scene *scene, const bhg_params *p, const bhg_redshift *rs,
                                          const bhg_observer *obs, const double *x0_shared, const double *d_k0, double *d_rgba,
                                          float *d_rgba_f32, const int64_t *d_scatter, const bhg_disk_thermal *th,
                                          const bhg_disk_layers *layers, const double *d_t_cross, double phase_rate, void *stream);

/* --- triangle meshes in the curved region (within ABI 10) ---------------------------------------------
 * A mesh is vertices [nv][3] fp64, Cartesian and centred on the hole (the frame object spheres are given in), and triangles
 * [nt][3] int32.  Triangles are two-sided.  A ray takes exactly the steps it takes without the mesh; the mesh is one more
 * terminal event, as an object sphere is.  THE HIT RULE, for each accepted DP5(4) step [lambda_j, lambda_j + h] in order:
 *   - L = the distance between the Cartesian positions of the step's two ends (Kerr: of their Cartesian images),
 *     M = min(BHG_MESH_MAX_SUBSTEPS, max(1, ceil(L / max_chord))); the step's dense-output position is sampled at
 *     theta_m = m / M (Kerr: the Cartesian image of the Boyer-Lindquist dense output); consecutive samples form M sub-chords;
 *   - the sub-chords are tested in order against every triangle with fp64 Moeller-Trumbore on the segment: a triangle counts when
 *     0 <= s <= 1, u, v >= 0, u + v <= 1; a zero determinant is skipped.  On the first sub-chord that meets a triangle the
 *     smallest s wins, a tie goes to the smaller triangle index: the tree only accelerates this, the answer does not depend on it;
 *   - the hit is moved from the chord onto the curve: Brent's search for the root of n_T . (x(lambda) - v0) on the sub-chord's
 *     parameter interval (an end exactly on the plane is the root; ends that do not straddle the plane -- both within rounding of
 *     it -- give the end nearer to it).  The ray ends there with BHG_FLAG_HIT_OBJECT, end = the dense output at the root,
 *     tri_id[i] = the triangle, bary[i] = (u, v), the plane coordinates of the refined point in that triangle,
 *     u = ((x - v0) x e2) . n / |n|^2, v = (e1 x (x - v0)) . n / |n|^2, n = e1 x e2 (they may leave [0, 1] by the chord's sag);
 *   - horizon, exit sphere and the opaque disk (disk_r_out > 0) are settled as the trace settles them and the earliest root wins:
 *     a mesh root later than the terminal root loses, sub-chords that start at or behind the terminal root are not looked at.
 * n_steps / n_accepted count up to and including the step that holds the hit.  A ray that hits nothing has tri_id = -1 and its
 * bary slot untouched; with no disk set its end / flags / n_steps / n_accepted are bhg_trace_device's bit for bit, with a disk
 * its flags and counts are the opaque-disk trace's and its end state that trace's within the disk bound of DESIGN section 16.
 * Refused (BHG_E_INVALID) before anything is launched or written: BHG_METHOD_RK4, time_like = 1, a NULL mesh, max_chord not
 * finite or <= 0, a NULL d_tri_id or d_bary, a mesh of another context's device.
 * bhg_mesh_create builds the tree on the host (leaf_size triangles per leaf at most, 4 is a good default; leaf_size >= nt is
 * brute force) and copies it to ctx's device.  vertex_normals: NULL, or [nv][3] for smooth shading.  Refused, nothing allocated:
 * nt = 0, nv = 0, an index outside [0, nv), a non-finite vertex or normal, leaf_size < 1, nt or nv over 2^31 - 1.
 * Environment: BHGEO_MESH_CULL=0 turns the whole-step cull off (the results are the same bits). */
#define BHG_MESH 1
#define BHG_MESH_MAX_SUBSTEPS 1024
typedef struct bhg_mesh bhg_mesh;
int bhg_mesh_create(bhg_context *ctx, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                    const double *vertex_normals, int32_t leaf_size, bhg_mesh **out);
void bhg_mesh_destroy(bhg_mesh *mesh);
/* the tree's node count, its depth (levels below the root) and the root box (lo x, y, z, hi x, y, z); any output may be NULL */
int bhg_mesh_info(const bhg_mesh *mesh, int64_t *n_nodes, int32_t *depth, double box[6]);
/* Host only, no context, no GPU: the flattened tree as the device gets it.  Nodes in depth-first order; on a box miss at node
 * i go to node_skip[i] (> i), otherwise to i + 1; a leaf (node_count > 0) holds the triangles tri_order[node_first ..
 * node_first + node_count - 1], an inner node has node_count = 0 and node_first = -1.  cap = the nodes the arrays hold
 * (2 * n_triangles - 1 always suffices); *n_nodes is set even when cap is too small (BHG_E_INVALID then). */
int bhg_mesh_bvh_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles, int32_t leaf_size,
                      double *node_box, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order, size_t cap,
                      size_t *n_nodes);
int bhg_trace_mesh_device(bhg_context *ctx, const bhg_params *p, const bhg_mesh *mesh, double max_chord,
                          const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                          uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted, int32_t *d_tri_id, double *d_bary,
                          void *stream);
/* bhg_trace_mesh_device on host arrays, as bhg_trace_crossings.  Blocking.  bary is read first. */
int bhg_trace_mesh(bhg_context *ctx, const bhg_params *p, const bhg_mesh *mesh, double max_chord, const double *x0,
                   int x0_is_shared, const double *k0, size_t n, double *end, uint8_t *flags, uint32_t *n_steps,
                   uint32_t *n_accepted, int32_t *tri_id, double *bary);
/* The shade of a mesh trace.  A ray flagged BHG_FLAG_HIT_OBJECT with tri_id >= 0 gets tri_rgb[tri] (d_tri_rgb [nt][3] fp32, NULL =
 * white) times the Lambert lamp sum of the object spheres, I^2 n.l / d^2 with n.l clamped at 0: n the triangle's unit normal --
 * or, vertex normals given, the normalised (1 - u - v) N0 + u N1 + v N2 -- turned to face the incoming ray; a lamp is shadowed
 * when the straight segment from x + 1e-5 l^ to the lamp meets any triangle.  Every other ray is bhg_shade_scene_device's, bit
 * for bit.  Refused: a scene with n_spheres > 0, a NULL mesh, a mesh of another context's device. */
int bhg_shade_mesh_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id,
                          const double *d_bary, size_t n_pixels, int32_t samples, const bhg_scene *scene, const bhg_mesh *mesh,
                          const float *d_tri_rgb, double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter, void *stream);

/* --- mesh material: per-corner UVs, image textures, emission; meshes on bhg_frame (within ABI 10) -------
 * A mesh ray (BHG_FLAG_HIT_OBJECT, 0 <= tri_id < nt) gets albedo * (lamp_sum + emission): lamp_sum is bhg_shade_mesh_device's
 * Lambert sum (same normal, facing rule, 1e-5 shadow segment), albedo = tri_rgb[tri] (NULL: 1) * texel.  Every other ray is
 * bhg_shade_scene_device's, bit for bit.
 * THE TEXEL.  With (u, v) = bary[i], w = 1 - u - v and the triangle's corner UVs (U0, V0), (U1, V1), (U2, V2):
 * U = w U0 + u U1 + v U2, V likewise, in fp64 from the fp32 corners; u, v are not clamped (they may leave [0, 1] by the chord's
 * sag: the UV is extrapolated linearly).  fx = U W - 0.5, fy = V H - 0.5, x0 = floor(fx), y0 = floor(fy), ax = fx - x0,
 * ay = fy - y0; columns x0 mod W and (x0 + 1) mod W, rows y0 mod H and (y0 + 1) mod H (the mathematical mod: the image repeats in
 * both directions); row 0 is V = 0; texel = (1 - ax)(1 - ay) t00 + ax (1 - ay) t01 + (1 - ax) ay t10 + ax ay t11 on RGB, alpha is
 * ignored.  A triangle with tri_tex < 0 (or, in the device form, >= n_tex) and a material without tri_uv have texel 1.
 * All per-triangle arrays are in the caller's numbering.  A material with tri_uv = NULL and emission = 0 gives
 * bhg_shade_mesh_device's image with the same tri_rgb, bit for bit.
 * Refused (BHG_E_INVALID, the message names the field) before anything is launched or written: what bhg_shade_mesh_device
 * refuses; a NULL material; emission negative or not finite; n_tex outside [0, BHG_MESH_TEXTURES_MAX]; a slot < n_tex with a
 * NULL image or w, h < 1; tri_uv given with n_tex = 0.  The host-array form (bhg_frame_set_mesh) scans the arrays and also
 * refuses a non-finite UV or |uv| > 2^20 (the floating-point wrap would stop being exact) and a tri_tex entry >= n_tex. */
#define BHG_MESH_MATERIAL 1
#define BHG_MESH_TEXTURES_MAX 8
typedef struct bhg_mesh_material {
    const float   *tri_rgb;   /* [nt][3] caller's numbering, NULL = white (as bhg_shade_mesh_device) */
    const float   *tri_uv;    /* [nt][3][2] per-corner (u, v), corners in the triangle's vertex order; NULL = no textures */
    const int32_t *tri_tex;   /* [nt] image slot per triangle, < 0 = none; NULL = slot 0 for every triangle */
    const float   *tex[BHG_MESH_TEXTURES_MAX];      /* [h][w][4] float RGBA, rows bottom-up (the sky's convention) */
    int32_t        tex_w[BHG_MESH_TEXTURES_MAX], tex_h[BHG_MESH_TEXTURES_MAX];
    int32_t        n_tex;
    double         emission;  /* >= 0 */
} bhg_mesh_material;
size_t bhg_mesh_material_size(void);
/* bhg_shade_mesh_device with a material in place of d_tri_rgb; every pointer of *mat is a device pointer. */
int bhg_shade_mesh_material_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id,
                                   const double *d_bary, size_t n_pixels, int32_t samples, const bhg_scene *scene,
                                   const bhg_mesh *mesh, const bhg_mesh_material *mat, double *d_rgba, float *d_rgba_f32,
                                   const int64_t *d_scatter, void *stream);
/* A mesh on the library-owned frame.  All arrays are on the host and are copied; nothing is referenced after the call.  material
 * may be NULL (white, no emission); vertices = NULL turns the mesh off (the other arguments are ignored) and the next render is
 * the plain one, bit for bit -- the shards' kept start steps and start-up records are neither used nor touched while a mesh is
 * set.  max_chord = 0: a quarter of the r_s of each render's parameters.  The mesh (its tree is built per device) and the images
 * are uploaded to every listed device at the next render.  Each shard then traces with bhg_trace_mesh_device (whole end records:
 * bhg_frame_info's direction-only field is 0) and shades with bhg_shade_mesh_material_device, in every gather mode.
 * Refused, the frame left as it was: what bhg_mesh_create and the material refuse; max_chord negative or not finite.
 * bhg_frame_render refuses (before anything is enqueued, "a mesh does not go with ...") a mesh together with scene spheres,
 * redshift, the thermal disk, object motion or object textures. */
int bhg_frame_set_mesh(bhg_frame *frame, const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                       const double *vertex_normals, int32_t leaf_size, double max_chord, const bhg_mesh_material *material);

/* --- mesh instances: K rigid placements of one built mesh (within ABI 10) ---------------------------------
 * Instance j is a rotation R_j and a translation t_j, 12 doubles: R row-major, then t; x_world = R_j x_local + t_j, both centred
 * on the hole as the vertices are.  A ray takes exactly the steps, sub-chords, M and ordering against horizon, exit sphere and
 * disk of the mesh trace above; only the test of a sub-chord changes:
 *   * for each instance the sub-chord's two ends go to the instance's frame, p' = R_j^T (p - t_j), and the first-hit test of the
 *     mesh trace runs there against the one tree.  The chord parameter s is the same in both frames; over all instances the
 *     smallest s wins, a tie goes to the smaller instance index, then to the smaller triangle index;
 *   * the hit is moved onto the curve in the winning instance's frame: Brent's search on n_T . (R_j^T (x(lambda) - t_j) - v0),
 *     with the mesh trace's fallback when the ends do not bracket;
 *   * end is the dense output at the root, in world coordinates; tri_id the caller's triangle within the mesh; inst_id [n] int32
 *     the instance, -1 for a ray that ends on no triangle; bary the plane coordinates in the instance's frame.
 * What only accelerates this (BHGEO_MESH_CULL=0 turns all of it off, the whole-step cull and the instances' boxes, in the trace
 * and in the shade's shadow segments: the results are the same bits): each instance has a world box -- centre
 * R c + t, half extents |R| h of the tree's root box, widened outward as the builder widens boxes -- that a sub-chord must meet
 * before it is transformed; the whole-step cull runs against the union of these boxes (Kerr: the largest |t_j| plus the mesh's
 * farthest vertex, and the smallest distance from the origin to an instance box).  All of it is worked out on the host in O(K)
 * by _create and _set.  The loop over the instances is linear: BHG_MESH_INSTANCES_MAX of them at most.
 * bhg_mesh_instances_set takes new transforms for the same n: the records are copied aside and their upload is enqueued on the
 * context's own stream; no tree is touched and nothing else is uploaded.  The set orders the upload against the calls that read
 * it, whatever stream they name: it runs behind every trace and shade enqueued before it, and those enqueued after it wait for
 * it.  Nothing waits on the host, but a third _set while the first one's upload is still queued.
 * An instance set is destroyed by the caller; destroying its mesh first leaves a set that every call refuses.
 * Refused (BHG_E_INVALID, the message names the field) before anything is launched or written: what bhg_trace_mesh_device
 * refuses; n outside [1, BHG_MESH_INSTANCES_MAX]; a NULL or non-finite transform entry; R^T R further than 1e-9 from the
 * identity in any entry, or det R <= 0; a NULL d_inst_id; an instance set of another context or of a destroyed mesh. */
#define BHG_MESH_INSTANCES 1
#define BHG_MESH_INSTANCES_MAX 64
typedef struct bhg_mesh_instances bhg_mesh_instances;
int bhg_mesh_instances_create(bhg_context *ctx, const bhg_mesh *mesh, int32_t n, const double *transforms /* host [n][12] */,
                              bhg_mesh_instances **out);
int bhg_mesh_instances_set(bhg_mesh_instances *inst, const double *transforms /* host [n][12] */);
void bhg_mesh_instances_destroy(bhg_mesh_instances *inst);
/* n and the union of the instances' world boxes (lo, hi); either may be NULL */
int bhg_mesh_instances_info(const bhg_mesh_instances *inst, int32_t *n, double box[6]);
/* The world box (lo, hi) an instance gets from a local box (lo, hi) and one transform: host arithmetic, no context, no GPU. */
int bhg_mesh_instance_box_host(const double local_box[6], const double transform[12], double world_box[6]);
/* bhg_trace_mesh_device with an instance set in place of the mesh, plus d_inst_id [n] int32. */
int bhg_trace_mesh_instances_device(bhg_context *ctx, const bhg_params *p, const bhg_mesh_instances *inst, double max_chord,
                                    const double *x0_shared, const double *d_x0, const double *d_k0, size_t n, double *d_end,
                                    uint8_t *d_flags, uint32_t *d_n_steps, uint32_t *d_n_accepted, int32_t *d_tri_id,
                                    int32_t *d_inst_id, double *d_bary, void *stream);
/* ... on host arrays, as bhg_trace_mesh.  Blocking.  bary is read first. */
int bhg_trace_mesh_instances(bhg_context *ctx, const bhg_params *p, const bhg_mesh_instances *inst, double max_chord,
                             const double *x0, int x0_is_shared, const double *k0, size_t n, double *end, uint8_t *flags,
                             uint32_t *n_steps, uint32_t *n_accepted, int32_t *tri_id, int32_t *inst_id, double *bary);
/* The shade of an instanced trace: bhg_shade_mesh_material_device over an instance set.  A mesh ray (BHG_FLAG_HIT_OBJECT,
 * 0 <= tri_id < nt, 0 <= inst_id < n) gets albedo * inst_rgb[inst] * (lamp_sum + emission).  The material -- UVs, images, emission
 * -- is the mesh's, shared by all instances; mat = NULL is white without emission.  d_inst_rgb [n][3] fp32 (NULL: none) multiplies
 * the albedo, so that copies can be told apart.  lamp_sum is the mesh shade's: the normal is formed in the instance's frame, flat or
 * interpolated, rotated by R_j, then normalised and turned to face the ray; a lamp is shadowed when the segment to it meets any
 * triangle of any instance (index order, the instance's world box first).  One instance under the identity is
 * bhg_shade_mesh_material_device's image, bit for bit.
 * Refused: what bhg_shade_mesh_material_device refuses (but a NULL mat); a NULL inst or d_inst_id; an instance set of another
 * context or of a destroyed mesh. */
int bhg_shade_mesh_instances_device(bhg_context *ctx, const double *d_end, const uint8_t *d_flags, const int32_t *d_tri_id,
                                    const int32_t *d_inst_id, const double *d_bary, size_t n_pixels, int32_t samples,
                                    const bhg_scene *scene, const bhg_mesh_instances *inst, const bhg_mesh_material *mat,
                                    const float *d_inst_rgb, double *d_rgba, float *d_rgba_f32, const int64_t *d_scatter,
                                    void *stream);
/* Instances of the frame's mesh: n rigid placements (host [n][12], copied), inst_rgb host [n][3] fp32 or NULL.  Each shard then
 * traces with bhg_trace_mesh_instances_device and shades with bhg_shade_mesh_instances_device, the frame's material shared by all
 * instances, in every gather mode.  Calling it again with other transforms for the same n moves the instances: at the next render
 * the records go to every device (bhg_mesh_instances_set) -- no tree is built, no array or image of the mesh is uploaded.
 * n = 0 turns instances off: the next render is the plain mesh render, bit for bit.  bhg_frame_set_mesh, with new arrays or NULL,
 * turns them off too.  Refused, the frame left as it was: a frame without a mesh; what bhg_mesh_instances_create refuses of n and
 * the transforms; a non-finite inst_rgb.  bhg_frame_render's "a mesh does not go with ..." cases hold as they are. */
int bhg_frame_set_mesh_instances(bhg_frame *frame, int32_t n, const double *transforms, const float *inst_rgb);

/* --- instance trees: an instance set whose placements lie under a tree of boxes (within ABI 10) -----------
 * bhg_mesh_instances_create_tree makes a bhg_mesh_instances of up to BHG_MESH_INSTANCE_TREE_MAX placements that every call above
 * takes -- _set, _destroy, _info, both trace calls, the shade -- and that computes what a set of bhg_mesh_instances_create
 * computes, bit for bit: the rule (the smallest s, then the smaller instance, then the smaller triangle) does not depend on the
 * order in which the placements are visited, and the tree only decides which of them a sub-chord or a shadow segment looks at.
 * The tree lies over the placements' world boxes: binary, every range split by count on the longest axis of its boxes' centres
 * (ties by instance index) down to leaf_size placements, so its shape depends on (n, leaf_size) alone; a node's box is the exact
 * union of the world boxes below it.  It is walked per ray, without a stack, by skip links; a box is skipped only when it starts
 * behind the best s so far.  bhg_mesh_instances_set builds the order and the boxes anew on the host, in O(n log n), and sends
 * records and tree in one upload (records | boxes | skip | first | count | order) through the set's own buffers: moving needs
 * no synchronisation, as before, and allocates nothing.  The refit rule of bhg_mesh_refit applies unchanged.
 * BHGEO_MESH_CULL=0 keeps its meaning -- no box is looked at, of the tree's or of an instance, every placement is walked --,
 * and BHGEO_INSTANCE_TREE=0 has such a set walked by the linear loop over all its records (A/B aids: the same bits).
 * Refused, in this order: a NULL out; n outside [1, BHG_MESH_INSTANCE_TREE_MAX]; leaf_size outside [1, 8]; the transforms as
 * bhg_mesh_instances_create refuses them; a NULL mesh; the context.  bhg_mesh_instances_create and BHG_MESH_INSTANCES_MAX stay
 * what they are: a set made the old way is walked linearly. */
#define BHG_MESH_INSTANCE_TREE 1
#define BHG_MESH_INSTANCE_TREE_MAX 65536
int bhg_mesh_instances_create_tree(bhg_context *ctx, const bhg_mesh *mesh, int32_t n, const double *transforms /* host [n][12] */,
                                   int32_t leaf_size, bhg_mesh_instances **out);
/* the tree of a set: its nodes, its depth (levels below the root) and its leaf_size; all zeros for a linear set.  Any may be NULL */
int bhg_mesh_instances_tree_info(const bhg_mesh_instances *inst, int32_t *n_nodes, int32_t *depth, int32_t *leaf_size);
/* The tree such a set builds over n placements of a mesh whose root box is local_box: host arithmetic, no context, no GPU.
 * node_box [2 n - 1][6], node_skip / node_first / node_count [2 n - 1] (2 n - 1 nodes always suffice), inst_order [n]: the caller's
 * instance in each leaf slot.  Leaves have count > 0 and first = their first slot; inner nodes count = 0, first = -1. */
int bhg_mesh_instance_tree_host(const double local_box[6], int32_t n, const double *transforms, int32_t leaf_size, double *node_box,
                                int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *inst_order, int32_t *n_nodes,
                                int32_t *depth);
/* bhg_frame_set_mesh_instances with sets of bhg_mesh_instances_create_tree: up to BHG_MESH_INSTANCE_TREE_MAX placements of the
 * frame's mesh, in every gather mode.  A second call with the same n moves the instances (one upload per device); n = 0, a call of
 * bhg_frame_set_mesh_instances or of bhg_frame_set_mesh turns the trees off.  Refused, the frame left as it was: what that call
 * refuses, with bhg_mesh_instances_create_tree's bounds on n and leaf_size in place of BHG_MESH_INSTANCES_MAX. */
int bhg_frame_set_mesh_instance_tree(bhg_frame *frame, int32_t n, const double *transforms, const float *inst_rgb, int32_t leaf_size);

/* --- deforming meshes: new vertices into a built mesh, its tree refitted on the device (within ABI 10) ----
 * A refit gives a mesh new vertex positions (and vertex normals).  n_vertices and the triangles are the mesh's own: the tree's
 * topology, the leaf order and the skip links stay, the per-slot triangle records and every box are written anew by kernels, and
 * nothing is built, allocated (after the first refit) or uploaded but the vertices.  Every box is the exact min / max over what
 * lies below it, widened by the builder's rule, so it contains its triangles as a freshly built tree's boxes do; and since the
 * tree only accelerates the hit rule above, a trace or shade of the refitted mesh gives the bits of one on a mesh created fresh
 * from the same vertices.  What a refit cannot keep is the tree's QUALITY: boxes of a tree split for other positions overlap
 * more.  bhg_mesh_refit_info reports the tree's area sum -- the sum over all nodes of dx dy + dy dz + dz dx of the widened box,
 * in one fixed order -- as it was at creation (area_build, from the host's tree) and as the last refit left it (area_now); their
 * ratio is the figure to decide a rebuild (bhg_mesh_destroy + bhg_mesh_create) by.  area_build is 0 only when every product
 * underflows (a mesh whose vertices all lie at the origin); the ratio is then not formed and says nothing.  generation is 0 at
 * creation and +1 per successful refit.
 * Both calls are blocking: they wait for everything queued on the context's stream and on `stream` before the first write to the
 * mesh, and for their own work before they return; box, d_min and d_max of the mesh are then those bhg_mesh_create would set.
 * Ordering against kernels that read the mesh on OTHER streams is the caller's job, as for any device buffer the caller writes.
 * bhg_mesh_refit takes host arrays and works on the context's stream; bhg_mesh_refit_device takes device arrays -- vertices
 * deformed on the GPU -- which are scanned for non-finite values by a first device pass before anything is written.
 * Refused (BHG_E_INVALID, the message names the field), the mesh untouched: a NULL mesh or vertices; a mesh of another context's
 * device; a non-finite vertex or normal; normals given to a mesh created without them, or omitted for a mesh created with them.
 * An instance set records its mesh's generation at _create and _set (its world boxes come from the mesh's local box): every trace
 * or shade with a set whose mesh has been refitted since is refused before anything is launched, "call bhg_mesh_instances_set
 * after bhg_mesh_refit"; _set, with the same transforms or others, makes the set current. */
#define BHG_MESH_REFIT 1
int bhg_mesh_refit(bhg_context *ctx, bhg_mesh *mesh, const double *vertices /* host [nv][3] */,
                   const double *vertex_normals /* host [nv][3], or NULL */);
int bhg_mesh_refit_device(bhg_context *ctx, bhg_mesh *mesh, const double *d_vertices, const double *d_vertex_normals, void *stream);
/* any output may be NULL */
int bhg_mesh_refit_info(const bhg_mesh *mesh, uint64_t *generation, double *area_build, double *area_now);
/* The range of distances from the origin the mesh lies in, as the whole-step cull of the Kerr trace uses it: d_min from the root
 * box, d_max from the farthest vertex a triangle names; set by bhg_mesh_create and by every refit.  Either output may be NULL. */
int bhg_mesh_range(const bhg_mesh *mesh, double *d_min, double *d_max);
/* Host only, no context, no GPU: the CPU statement of the refit kernels.  Given vertices, triangles and a topology as
 * bhg_mesh_bvh_host returns it, writes the refitted, widened node_box [n_nodes][6] and (area may be NULL) the area sum.  With
 * the vertices the topology was built from, node_box is bhg_mesh_bvh_host's bit for bit.  Refused: what bhg_mesh_create
 * refuses of vertices and triangles; a topology that is not a tree of bhg_mesh_bvh_host's kind over n_triangles slots. */
int bhg_mesh_bvh_refit_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles,
                            const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count, const int32_t *tri_order,
                            size_t n_nodes, double *node_box, double *area);
/* Host only: the bottom-up schedule the refit walks.  level_nodes[level_off[d] .. level_off[d + 1]) are the inner nodes d levels
 * below the root, d = 0 .. 32 (level_off holds 34 entries); the levels are done deepest first, so every inner node comes after
 * both its children.  cap = the entries level_nodes holds (n_triangles - 1 always suffices); *n_inner is set even when cap is
 * too small (BHG_E_INVALID then). */
int bhg_mesh_refit_schedule_host(const int32_t *node_skip, const int32_t *node_first, const int32_t *node_count,
                                 const int32_t *tri_order, size_t n_nodes, size_t n_triangles, int32_t *level_nodes,
                                 int32_t *level_off, size_t cap, size_t *n_inner);
/* New vertices (and vertex normals: given exactly when the mesh was set with them) for the mesh of the library-owned frame;
 * host arrays of the mesh's n_vertices, copied.  At the next render each device that holds the mesh refits it (bhg_mesh_refit)
 * instead of building it anew; the material and its images, the instances and their colours stay, and the frame sets its
 * instance sets again by itself.  The render is the one bhg_frame_set_mesh with the deformed vertices gives, bit for bit.
 * rebuild_ratio: a device whose area_now would exceed rebuild_ratio * area_build builds its tree anew from the held triangles
 * and the new vertices instead; <= 0: never rebuild; a value in (0, 1], and so 1: always rebuild.
 * Refused, the frame left as it was: a frame without a mesh; what bhg_mesh_refit refuses; a NaN rebuild_ratio. */
int bhg_frame_refit_mesh(bhg_frame *frame, const double *vertices, const double *vertex_normals, double rebuild_ratio);
/* bhg_mesh_refit_info of the mesh that device number `shard` of the frame holds (in the order of the frame's device list): a
 * rebuilt mesh starts at generation 0 again.  Refused: a shard outside the list; a device that holds no mesh yet. */
int bhg_frame_mesh_refit_info(const bhg_frame *frame, int32_t shard, uint64_t *generation, double *area_build, double *area_now);
/* A blocking download of the device's boxes [n_nodes][6] and (tri may be NULL) slot records [nt][9] = v0, e1, e2 per leaf slot,
 * for tests and diagnosis.  cap = the nodes node_box holds. */
int bhg_mesh_boxes_host(const bhg_mesh *mesh, double *node_box, double *tri, size_t cap);

/* --- the device-side build: a Morton-order tree over a triangle list on the device, rebuilt in place (within ABI 10; DESIGN.md
 * section 23) ----
 * For a mesh whose TRIANGLE LIST changes -- a fluid surface, a boolean, a remesher -- a refit does not serve and bhg_mesh_destroy +
 * bhg_mesh_create builds on the host.  These calls build on the device: the triangles are sorted by a 63-bit Morton key of their
 * centroids (21 bits per axis in the centroid bounds, ties by the caller's index), the tree of bhg_mesh_bvh_host's kind whose
 * ranges split by count at lo + m / 2 is laid over that order (its node_skip / node_first / node_count are a function of
 * n_triangles and leaf_size alone), every leaf's slots are put in rising caller index, and the refit kernels write slot records,
 * boxes, widening and the area sum.  bhg_mesh_bvh_morton_host states the same tree on the host, bit for bit.  The tree only
 * accelerates the hit rule: every trace and shade of a device-built mesh gives the bits of one on the host-built mesh.
 * The mesh of bhg_mesh_create_device is a bhg_mesh like any other: every trace, shade, instance set, refit and query takes it.
 * All of its device memory -- tree and records for cap_vertices / cap_triangles (0: the counts themselves), the sort's storage, the
 * refit's -- is allocated at creation, so a rebuild within capacity allocates nothing (allocations of bhg_mesh_build_info counts
 * the mesh's device allocations over its life).  A mesh of bhg_mesh_create has its own counts as capacity and may be rebuilt at
 * those or fewer; its first rebuild moves it into an image of that capacity and allocates the build's storage.
 * The arrays are device arrays of the context's device (bhg_mesh_rebuild: host arrays, uploaded first).  A first device pass
 * checks every triangle index against [0, n_vertices) and every vertex and normal for non-finite values, and its result is read
 * back before any kernel follows an index or anything of the mesh is written: a bad array ends in BHG_E_INVALID.
 * Blocking, with the refit's contract: the calls wait for everything queued on the context's stream and on `stream` before the
 * first write and for their own work before they return; ordering against readers on OTHER streams is the caller's job.
 * After a rebuild box, d_min, d_max, n_nodes, depth, area_build and area_now are the new tree's, generation is one higher -- so
 * every instance set of the mesh is refused until its bhg_mesh_instances_set -- and builds is one higher (1 after creation).
 * Refused (BHG_E_INVALID, the message names the field), the mesh untouched and for _create_device nothing left allocated and
 * *out NULL: what bhg_mesh_create refuses; leaf_size outside [1, 64] (the per-leaf sort is one thread's loop: brute-force leaves
 * stay with bhg_mesh_create); counts over the capacity; a capacity below the counts; normals given to a mesh without them, or
 * omitted for one with them; a mesh of another context's device. */
#define BHG_MESH_BUILD_DEVICE 1
int bhg_mesh_create_device(bhg_context *ctx, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles,
                           size_t n_triangles, const double *d_vertex_normals /* or NULL */, int32_t leaf_size, size_t cap_vertices,
                           size_t cap_triangles, void *stream, bhg_mesh **out);
int bhg_mesh_rebuild_device(bhg_context *ctx, bhg_mesh *mesh, const double *d_vertices, size_t n_vertices, const int32_t *d_triangles,
                            size_t n_triangles, const double *d_vertex_normals, void *stream);
int bhg_mesh_rebuild(bhg_context *ctx, bhg_mesh *mesh, const double *vertices, size_t n_vertices, const int32_t *triangles,
                     size_t n_triangles, const double *vertex_normals);
/* any output may be NULL */
int bhg_mesh_build_info(const bhg_mesh *mesh, int32_t *built_on_device, uint64_t *builds, size_t *cap_vertices, size_t *cap_triangles,
                        uint64_t *allocations);
/* Host only, no context, no GPU: the Morton tree, with the arguments and outputs of bhg_mesh_bvh_host.  Unlike that builder it
 * never makes a leaf over leaf_size (identical triangles are separated by their index), and it takes any leaf_size >= 1. */
int bhg_mesh_bvh_morton_host(const double *vertices, size_t n_vertices, const int32_t *triangles, size_t n_triangles, int32_t leaf_size,
                             double *node_box, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order,
                             size_t cap, size_t *n_nodes);
/* A blocking download of the device's node_skip, node_first, node_count [n_nodes] and tri_order [n_triangles], for tests and
 * diagnosis.  cap = the nodes the three node arrays hold; *n_nodes is set even when cap is too small (BHG_E_INVALID then). */
int bhg_mesh_tree_host(const bhg_mesh *mesh, int32_t *node_skip, int32_t *node_first, int32_t *node_count, int32_t *tri_order,
                       size_t cap, size_t *n_nodes);
/* The device build on the library-owned frame; on_device = 0 (the default: the host builder, everything as before) or 1.  When on:
 * each device creates its mesh with the device build from the frame's host copy, with a capacity of BHG_FRAME_MESH_HEADROOM
 * times its counts (a mesh whose triangle list changes seldom keeps its counts); a later bhg_frame_set_mesh whose counts fit the
 * capacity of the mesh a device holds (with the same leaf_size, and normals given or not as before) rebuilds that mesh in place
 * instead of destroying and creating it; and the rebuild_ratio path of bhg_frame_refit_mesh rebuilds in place on the device.  The
 * material is replaced as bhg_frame_set_mesh replaces it.  Every image is the host-built frame's, bit for bit.  Meshes the
 * devices hold already stay as they are until the next bhg_frame_set_mesh or rebuild.  Refused: a frame whose mesh has a leaf_size
 * over 64; and, while on, bhg_frame_set_mesh with such a leaf_size. */
#define BHG_FRAME_MESH_HEADROOM 4
int bhg_frame_set_mesh_build(bhg_frame *frame, int on_device);
/* bhg_mesh_build_info of the mesh that device number `shard` of the frame holds; refused as bhg_frame_mesh_refit_info refuses. */
int bhg_frame_mesh_build_info(const bhg_frame *frame, int32_t shard, int32_t *built_on_device, uint64_t *builds, size_t *cap_vertices,
                              size_t *cap_triangles, uint64_t *allocations);

/* Acceleration probe: acc[n][3] = -Gamma^i_{mu nu} k^mu k^nu at (x[n][3], k[n][3]); host buffers.
 * Lets tests compare the device RHS with the oracle's term by term.  With rhs_form = BHG_RHS_KERR_BL the triples
 * are Boyer-Lindquist: x = (r, theta, phi), k = d(r, theta, phi)/dlambda, acc = d^2(r, theta, phi)/dlambda^2, and the
 * Killing constants E = -k_t, L = k_phi the right-hand side needs are fixed by the null condition at each point
 * (the trace fixes them the same way at the camera); p->spin is the Kerr a. */
int bhg_acceleration(bhg_context *ctx, const bhg_params *p, const double *x, const double *k,
                     size_t n, double *acc);

/* Wait for everything enqueued on the context's own stream. */
int bhg_synchronize(bhg_context *ctx);

/* The context's own non-blocking stream (a hipStream_t), used by the host-buffer calls. */
void *bhg_context_stream(bhg_context *ctx);

/* Per-pass timing of the trace calls.  A trace call runs up to two passes on the caller's stream:
 * PREPARE (per-ray setup: f0, initial step, Kerr's Cartesian -> Boyer-Lindquist conversion -- done inside
 * TRACE by the waves' queue fill for every form since ABI 6, so this slot reads 0; it was a launch of its own
 * for BHG_RHS_KERR_BL before) and TRACE (the integrate loop including the root search for
 * rays that end on an event; the dominant kernel).  With profiling enabled the library records HIP
 * events around each pass on that stream; bhg_last_pass_ms() waits for the last call's events and
 * returns {prepare, trace, post} in milliseconds: post is the pass after the trace kernel -- the
 * Boyer-Lindquist -> Cartesian finalize of BHG_RHS_KERR_BL, 0 for the Schwarzschild forms (up to the
 * ABI 1.x builds of round 1 the slot was a separate root-search pass). */
int bhg_set_profiling(bhg_context *ctx, int enable);
int bhg_last_pass_ms(bhg_context *ctx, float out_ms[3]);

/* Kernel launch geometry chosen for the last bhg_trace* call (for DESIGN/bench reporting):
 * out[0] = workgroups, out[1] = threads per workgroup, out[2] = resident waves per CU,
 * out[3] = number of trace launches the call took: 1 -- rays whose disk / object candidate step held no terminal
 *          event are resumed inside the same launch -- unless the call holds more than 2^26 rays (a launch takes at
 *          most that many; BASELINE's largest frame, 2048 x 2048 x 16, is exactly one). */
int bhg_last_launch(bhg_context *ctx, int32_t out[4]);

/* Roofline calibration on THIS device, in the trace kernels' own launch geometry (one wave64 per workgroup, 12 resident
 * waves per CU; no memory traffic inside the loop) -- bench.py's `roofline.calibration` block, so that two bench lines
 * from two boxes of a pool can be compared (SURVEY.md section 8d prices against the vendor's 78.6 TFLOP/s):
 *   BHG_PROBE_FMA       nothing but v_fma_f64, eight independent chains per lane: the fp64 vector rate this box sustains;
 *   BHG_PROBE_STEP_MIX  the DP5(4) step loop's mix -- per 503 VALU instructions 8 v_rcp_f64 + 8 v_rsq_f64 (quarter rate)
 *                       among 487 v_fma_f64: the issue-bound ceiling of a kernel with that mix.
 * target_ms: duration of one probe launch (0 = 1 ms); the loop is sized from a short launch, then the MEDIAN of five
 * launches is reported.  out = {TFLOP/s (FMA = 2 flop, rcp / rsq = 1), ms per launch (median), VALU wave-instructions
 * per launch, quarter-rate ones among them, fastest of the five launches in ms, the shader clock in MHz that a full-rate
 * fp64 pipe (128 flop per clock and CU) needs for that TFLOP/s figure}.  Blocking; runs on the context's own stream. */
#define BHG_PROBE_FMA 0
#define BHG_PROBE_STEP_MIX 1
int bhg_peak_probe(bhg_context *ctx, int32_t kind, double target_ms, double out[6]);

/* A TEST HOOK, not part of the rendering surface (additive: the ABI number stays 10): n elements, one per thread, through ONE of
 * the hand-written fp64 primitives of the kernels (csrc/device_math.h, csrc/kerr_start.h), compiled with the flags of the
 * units that use them, so that a test can compare each with a high-precision reference ulp by ulp.
 * in and out are HOST buffers; per element, in -> out:
 *   BHG_MATH_RCP_NEWTON       x -> 1 / x                        BHG_MATH_RCP_NR   x -> 1 / x
 *   BHG_MATH_RSQRT_NR         x -> 1 / sqrt(x)                  BHG_MATH_SQRT_NR  x -> sqrt(x)  (0 for x <= 0)
 *   BHG_MATH_ATAN2_FAST       (y, x) -> atan2(y, x)             BHG_MATH_SINCOS_PI4  x -> (sin x, cos x)
 *   BHG_MATH_RCP3_NR          (x0, x1, x2) -> (1/x0, 1/x1, 1/x2)
 *   BHG_MATH_KERR_CART_TO_BL  (a, M, mu2, x[3], k[3]) -> (r, theta, phi, dr, dtheta, dphi, E, L)
 * An unknown op and a NULL buffer with n > 0 are refused (BHG_E_INVALID, bhg_last_error); n = 0 is a no-op; at most 2^26
 * elements per call.  Blocking; runs on the context's own stream. */
#define BHG_MATH_PROBE 1
#define BHG_MATH_RCP_NEWTON 0
#define BHG_MATH_RCP_NR 1
#define BHG_MATH_RSQRT_NR 2
#define BHG_MATH_SQRT_NR 3
#define BHG_MATH_ATAN2_FAST 4
#define BHG_MATH_SINCOS_PI4 5
#define BHG_MATH_RCP3_NR 6
#define BHG_MATH_KERR_CART_TO_BL 7
int bhg_math_probe(bhg_context *ctx, int32_t op, const double *in, size_t n, double *out);

#ifdef __cplusplus
}
#endif
#endif /* BHGEO_H */

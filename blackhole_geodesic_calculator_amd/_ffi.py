"""ctypes binding of libbhgeo.so (C ABI declared in include/bhgeo.h).

The library is the product: there is no Python or CPU fallback.  Importing this module never
touches the GPU; `load()` raises loudly when the shared library has not been built, and
`Context()` raises when no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BHGEO_LIB") or os.path.join(_HERE, "libbhgeo.so")  # BHGEO_LIB: A/B builds

ABI_VERSION = 10
ABI_COMPAT_MIN = 7    # bhg_abi_check serves bindings from this ABI on (8 added bhg_trajectory_objects, 9 the redshift calls,
                      # 10 the observer camera)

OK = 0
E_INVALID, E_NO_DEVICE, E_HIP, E_NOMEM = -1, -2, -3, -4

FLAG_HIT_HORIZON = 1
FLAG_START_INSIDE = 2
FLAG_REACHED_END = 4
FLAG_EXITED_SPHERE = 8
FLAG_MAX_STEPS = 16
FLAG_STEP_TOO_SMALL = 32
FLAG_NAN = 64
FLAG_HIT_DISK = 128
FLAG_HIT_OBJECT = 0x88  # composite: test with (flags & 0x88) == 0x88
MAX_SPHERES = 8

METHOD_DP54 = 0
METHOD_RK4 = 1
RHS_CHRISTOFFEL = 0
RHS_REDUCED = 1
RHS_KERR_BL = 2

# every symbol include/bhgeo.h declares (tests check the built library exports all of them)
EXPORTS = (
    "bhg_version", "bhg_device_count", "bhg_last_error", "bhg_default_params", "bhg_create",
    "bhg_destroy", "bhg_device_name", "bhg_num_cus", "bhg_trace", "bhg_trace_device",
    "bhg_acceleration", "bhg_synchronize", "bhg_last_launch", "bhg_context_stream", "bhg_raygen_device",
    "bhg_shade_device", "bhg_set_profiling", "bhg_last_pass_ms", "bhg_trajectory", "bhg_trace_objects",
    "bhg_trace_objects_device", "bhg_shade_scene_device", "bhg_shade_scene_f32_device",
    "bhg_assemble_frame_f32_device", "bhg_host_alloc", "bhg_host_free", "bhg_rays_create", "bhg_rays_count",
    "bhg_rays_destroy", "bhg_rays_trace", "bhg_trace_dir_device", "bhg_shade_dir_device",
    "bhg_frame_create", "bhg_frame_destroy", "bhg_frame_set_scene", "bhg_frame_set_camera", "bhg_frame_render", "bhg_frame_synchronize",
    "bhg_frame_device_image", "bhg_frame_rebalance", "bhg_frame_stats", "bhg_frame_info", "bhg_frame_set_profiling",
    "bhg_frame_last_ms", "bhg_deal_tiles",
    "bhg_params_size", "bhg_camera_size", "bhg_scene_size", "bhg_frame_scene_size", "bhg_abi_check",
    "bhg_default_params_sized", "bhg_peak_probe", "bhg_trajectory_objects",
    "bhg_redshift_size", "bhg_redshift_device", "bhg_redshift_host", "bhg_shade_scene_redshift_device", "bhg_frame_set_redshift",
    "bhg_observer_size", "bhg_raygen_observer_device", "bhg_redshift_observer_device", "bhg_redshift_observer_host",
    "bhg_shade_scene_redshift_observer_device", "bhg_frame_set_observer",
    "bhg_object_textures_size", "bhg_shade_scene_textured_device", "bhg_frame_set_object_textures",
    "bhg_polarisation_size", "bhg_polarisation_device", "bhg_polarisation_host", "bhg_shade_scene_polarised_device",
    "bhg_disk_thermal_size", "bhg_disk_thermal_device", "bhg_disk_thermal_host", "bhg_shade_scene_thermal_device",
    "bhg_frame_set_disk_thermal",
    "bhg_object_motion_size", "bhg_redshift_motion_device", "bhg_redshift_motion_host", "bhg_shade_scene_moving_device",
    "bhg_frame_set_object_motion",
    "bhg_math_probe",
    "bhg_trace_start_device", "bhg_start_steps_match", "bhg_trace_prefix_device", "bhg_prefix_clearance",
    "bhg_prefix_deep_attempts", "bhg_prefix_wide_accepted", "bhg_prefix_owner_next", "bhg_frame_prefix_info", "bhg_prefix_rim_attempts",
    "bhg_trace_crossings_device", "bhg_trace_crossings", "bhg_disk_layers_size", "bhg_shade_disk_layers_device",
    "bhg_travel_time_device", "bhg_travel_time", "bhg_shade_disk_layers_retarded_device",
    "bhg_mesh_create", "bhg_mesh_destroy", "bhg_mesh_info", "bhg_mesh_bvh_host", "bhg_trace_mesh_device", "bhg_trace_mesh",
    "bhg_shade_mesh_device",
    "bhg_mesh_material_size", "bhg_shade_mesh_material_device", "bhg_frame_set_mesh",
    "bhg_mesh_instances_create", "bhg_mesh_instances_set", "bhg_mesh_instances_destroy", "bhg_mesh_instances_info",
    "bhg_mesh_instance_box_host", "bhg_trace_mesh_instances_device", "bhg_trace_mesh_instances",
    "bhg_shade_mesh_instances_device", "bhg_frame_set_mesh_instances",
    "bhg_mesh_instances_create_tree", "bhg_mesh_instances_tree_info", "bhg_mesh_instance_tree_host", "bhg_frame_set_mesh_instance_tree",
    "bhg_mesh_refit", "bhg_mesh_refit_device", "bhg_mesh_refit_info", "bhg_mesh_bvh_refit_host", "bhg_mesh_refit_schedule_host",
    "bhg_mesh_boxes_host", "bhg_mesh_range", "bhg_frame_refit_mesh", "bhg_frame_mesh_refit_info",
    "bhg_mesh_create_device", "bhg_mesh_rebuild_device", "bhg_mesh_rebuild", "bhg_mesh_build_info", "bhg_mesh_bvh_morton_host",
    "bhg_mesh_tree_host", "bhg_frame_set_mesh_build", "bhg_frame_mesh_build_info",
)
MESH_DEVICE_LEAF_MAX = 64  # the largest leaf_size the device build takes (BHG_MESH_BUILD_DEVICE)
# the rebuild_ratio of Frame.refit_mesh and the add-on when none is given (DESIGN.md section 22 has the table it is read off: at
# area_now / area_build = 1.13 the refitted tree traced as fast as a fresh one, at 1.55 it lost more than the rebuild costs)
MESH_REBUILD_RATIO = 1.5
MESH_INSTANCES_MAX = 64    # BHG_MESH_INSTANCES_MAX: rigid placements an instance set holds at most (BHG_MESH_INSTANCES)
MESH_INSTANCE_TREE_MAX = 65536   # BHG_MESH_INSTANCE_TREE_MAX: placements a set under a tree holds at most (BHG_MESH_INSTANCE_TREE)
MESH_INSTANCE_TREE_LEAF = 4      # the leaf_size of such a tree when none is given (DESIGN.md section 24 has the table it is read off:
                                 # leaves of 4 trace fastest or level on every line, and make the smallest tree)
MESH_MAX_SUBSTEPS = 1024  # BHG_MESH_MAX_SUBSTEPS: sub-chords per accepted step at most (BHG_MESH)
MESH_TEXTURES_MAX = 8      # BHG_MESH_TEXTURES_MAX: images a mesh material holds at most (BHG_MESH_MATERIAL)
MAX_CROSSINGS = 4   # BHG_MAX_CROSSINGS: disk crossings a crossings trace stores per ray (BHG_DISK_CROSSINGS)
START_NONE, START_RECORD, START_REPLAY = 0, 1, 2   # BHG_START_*: the rays' initial steps kept across calls (BHG_START_STEPS)
# BHG_PREFIX_*: the rays' start-up records kept across calls (BHG_START_PREFIX)
PREFIX_NONE, PREFIX_RECORD, PREFIX_REPLAY = 0, 1, 2
PREFIX_K_MAX, PREFIX_BYTES_PER_RAY = 4, 112
# ... by the deep rule (BHG_PREFIX_RECORD_DEEP): rejected attempts kept, three quarters of the clear ball without object spheres
PREFIX_RECORD_DEEP, PREFIX_DEEP_ACCEPTED, PREFIX_DEEP_ATTEMPTS = 4, 6, 12
# ... by the wide rule (BHG_PREFIX_RECORD_WIDE): the deep rule in fifteen sixteenths of the ball, up to eight accepted steps
PREFIX_RECORD_WIDE, PREFIX_WIDE_ACCEPTED = 5, 8
# ... by the rim rule (BHG_PREFIX_RECORD_RIM): the wide rule in the ball that ends just above the horizon, nine accepted steps in fifteen attempts
PREFIX_RECORD_RIM, PREFIX_RIM_ACCEPTED, PREFIX_RIM_ATTEMPTS = 6, 9, 15


class Prefix(C.Structure):
    """bhg_prefix: d_records (device address), rho, mode in, used out (include/bhgeo.h has the rules)."""
    _fields_ = [("d_records", C.c_void_p), ("rho", C.c_double), ("mode", C.c_int32), ("used", C.c_int32)]


class PrefixOwner(C.Structure):
    """bhg_prefix_owner: what bhg_prefix_owner_next keeps of a ray set's records between calls."""
    _fields_ = [("rho", C.c_double), ("refused_run", C.c_int32), ("roomy_run", C.c_int32), ("clean_run", C.c_int32),
                ("reserved", C.c_int32)]


PROBE_FMA, PROBE_STEP_MIX = 0, 1
# bhg_math_probe: op -> (doubles in, doubles out) per element
MATH_RCP_NEWTON, MATH_RCP_NR, MATH_RSQRT_NR, MATH_SQRT_NR, MATH_ATAN2_FAST, MATH_SINCOS_PI4, MATH_RCP3_NR, MATH_KERR_CART_TO_BL = range(8)
MATH_PROBE_SHAPE = {MATH_RCP_NEWTON: (1, 1), MATH_RCP_NR: (1, 1), MATH_RSQRT_NR: (1, 1), MATH_SQRT_NR: (1, 1),
                    MATH_ATAN2_FAST: (2, 1), MATH_SINCOS_PI4: (1, 2), MATH_RCP3_NR: (3, 3), MATH_KERR_CART_TO_BL: (9, 8)}

GATHER_AUTO, GATHER_COPY, GATHER_RCCL, GATHER_PEER, GATHER_COPY_PEERCALL = 0, 1, 2, 3, 4

REDSHIFT_DISK, REDSHIFT_OBJECTS, REDSHIFT_SKY = 1, 2, 4
_REDSHIFT_CLASS = {"disk": REDSHIFT_DISK, "objects": REDSHIFT_OBJECTS, "sky": REDSHIFT_SKY}


class Redshift(C.Structure):
    """bhg_redshift (ABI 9): apply = BHG_REDSHIFT_* classes whose colour is weighted by g^exponent (0 = off)."""
    _fields_ = [("apply", C.c_uint32), ("disk_sense", C.c_int32), ("exponent", C.c_double)]


def make_redshift(apply=("disk", "objects", "sky"), exponent=4.0, disk_sense=1) -> Redshift:
    """apply: class names ("disk", "objects", "sky") or a BHG_REDSHIFT_* bit mask; () / 0 = off."""
    rs = Redshift()
    if isinstance(apply, (int, np.integer)):
        rs.apply = int(apply)
    else:
        bad = [a for a in apply if a not in _REDSHIFT_CLASS]
        if bad:
            raise ValueError(f"unknown redshift class {bad}: use {sorted(_REDSHIFT_CLASS)}")
        rs.apply = sum({_REDSHIFT_CLASS[a] for a in apply})
    rs.disk_sense, rs.exponent = int(disk_sense), float(exponent)
    return rs


class Observer(C.Structure):
    """bhg_observer (ABI 10): velocity beta relative to the ZAMO at the camera, world axes, |beta| < 1."""
    _fields_ = [("beta", C.c_double * 3)]


def make_observer(velocity):
    """Observer of velocity beta (3 numbers), or None (the reference camera)."""
    if velocity is None:
        return None
    b = np.asarray(velocity, dtype=np.float64).reshape(3)
    obs = Observer()
    obs.beta[:] = [float(v) for v in b]
    return obs


def _obs_ref(obs):
    return None if obs is None else C.byref(obs)


POL_TABLE_MAX = 64


class Polarisation(C.Structure):
    """bhg_polarisation (BHG_POLARISATION, within ABI 10): the disk's degree table against the emission cosine, its sense and
    image up (world axes at the camera)."""
    _fields_ = [("disk_sense", C.c_int32), ("n_degree", C.c_int32), ("up", C.c_double * 3),
                ("degree", C.c_double * POL_TABLE_MAX)]


def make_polarisation(degree=0.1, disk_sense=1, up=(0.0, 1.0, 0.0)) -> Polarisation:
    """degree: a constant, or a table of delta(mu_j) at mu_j = j / (n - 1) (1 to 64 numbers, linear between); disk_sense as
    redshift's; up: image up on world axes."""
    d = np.atleast_1d(np.asarray(degree, dtype=np.float64)).ravel()
    if not 1 <= d.size <= POL_TABLE_MAX:
        raise ValueError(f"the degree table has {d.size} entries: 1 to {POL_TABLE_MAX}")
    pol = Polarisation()
    pol.disk_sense, pol.n_degree = int(disk_sense), int(d.size)
    pol.up[:] = [float(v) for v in np.asarray(up, dtype=np.float64).reshape(3)]
    pol.degree[:d.size] = [float(v) for v in d]
    return pol


THERMAL_NU_MAX = 16


class DiskThermal(C.Structure):
    """bhg_disk_thermal (BHG_DISK_THERMAL, within ABI 10): the Novikov-Thorne disk's peak temperature, colour correction and
    scale, and the frequencies [Hz] the R, G, B channels weigh."""
    _fields_ = [("disk_sense", C.c_int32), ("n_nu", C.c_int32), ("t_peak", C.c_double), ("f_col", C.c_double),
                ("scale", C.c_double), ("nu", C.c_double * THERMAL_NU_MAX), ("weight", (C.c_double * THERMAL_NU_MAX) * 3)]


def make_disk_thermal(t_peak, nu, weights, f_col=1.0, scale=1.0, disk_sense=1) -> DiskThermal:
    """t_peak [K]: the disk's largest emitted temperature; nu: 1 to 16 frequencies [Hz] shared by the channels; weights [3, n]:
    each channel's weight of each frequency (any sign); f_col: colour correction; scale: overall factor; disk_sense as
    redshift's."""
    nu = np.atleast_1d(np.asarray(nu, dtype=np.float64)).ravel()
    w = np.asarray(weights, dtype=np.float64)
    if not 1 <= nu.size <= THERMAL_NU_MAX:
        raise ValueError(f"the frequency table has {nu.size} entries: 1 to {THERMAL_NU_MAX}")
    if w.shape != (3, nu.size):
        raise ValueError(f"weights must be [3, {nu.size}], not {list(w.shape)}")
    th = DiskThermal()
    th.disk_sense, th.n_nu = int(disk_sense), int(nu.size)
    th.t_peak, th.f_col, th.scale = float(t_peak), float(f_col), float(scale)
    th.nu[:nu.size] = [float(v) for v in nu]
    for c in range(3):
        th.weight[c][:nu.size] = [float(v) for v in w[c]]
    return th


def narrowband(nu_r, nu_g, nu_b):
    """(nu, weights) of narrow-band false colour: one frequency [Hz] per channel, weight 1 (make_disk_thermal(t, *narrowband(...)))."""
    return np.array([nu_r, nu_g, nu_b], dtype=np.float64), np.eye(3)


class ObjectMotion(C.Structure):
    """bhg_object_motion (BHG_OBJECT_MOTION, within ABI 10): each object sphere's centre velocity v and angular velocity w, world
    axes, dx/dt and rad per unit t.  All zero: every sphere at rest."""
    _fields_ = [("v", (C.c_double * 3) * MAX_SPHERES), ("w", (C.c_double * 3) * MAX_SPHERES)]


def make_object_motion(velocity=None, angular_velocity=None) -> ObjectMotion:
    """velocity, angular_velocity: [n][3] per sphere of the scene (n <= MAX_SPHERES), or None for zeros.  A sphere's surface
    point x moves with v + w x (x - c); the Kerr v is relative to the ZAMO's flow (observer.circular_orbit_motion)."""
    mo = ObjectMotion()
    for name, arr in (("v", velocity), ("w", angular_velocity)):
        if arr is None:
            continue
        a = np.asarray(arr, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] > MAX_SPHERES:
            raise ValueError(f"{name} must be [n, 3] with n <= {MAX_SPHERES}, not {list(a.shape)}")
        dst = getattr(mo, name)
        for j in range(a.shape[0]):
            dst[j][:] = [float(x) for x in a[j]]
    return mo


class DiskLayers(C.Structure):
    """bhg_disk_layers (BHG_DISK_CROSSINGS, within ABI 10): the optically thin disk of the layered shade -- how many crossing
    records a ray has at most and the opacity of one crossing."""
    _fields_ = [("max_crossings", C.c_int32), ("pad", C.c_int32), ("opacity", C.c_double)]


def make_disk_layers(max_crossings=3, opacity=1.0) -> DiskLayers:
    """max_crossings: 1 .. MAX_CROSSINGS layers; opacity in (0, 1]: each crossing passes 1 - opacity of what lies behind it
    (1: the opaque disk).  The library checks the ranges."""
    return DiskLayers(int(max_crossings), 0, float(opacity))


OBJECT_LIT, OBJECT_EMISSIVE = 0, 1
_OBJECT_MODE = {"lit": OBJECT_LIT, "emissive": OBJECT_EMISSIVE}


class ObjectTextures(C.Structure):
    """bhg_object_textures (BHG_OBJECT_TEXTURES, within ABI 10): per object sphere an equirectangular RGBA float32 texture
    (or NULL: white), its size, the mode (OBJECT_LIT / OBJECT_EMISSIVE), the emission strength and the row-major body -> world
    rotation (all zero = the identity)."""
    _fields_ = [("tex", C.c_void_p * 8), ("tex_w", C.c_int32 * 8), ("tex_h", C.c_int32 * 8), ("mode", C.c_int32 * 8),
                ("emission", C.c_double * 8), ("rot", (C.c_double * 9) * 8)]


def make_object_textures(textures=None, rotations=None, modes=None, emission=None):
    """(ObjectTextures, arrays to keep alive).  Per sphere, in the scene's order (at most 8, missing ones are zero):
    textures -- None (NULL: white for a shade call, keep the current one for a frame), a float32 [h, w, 4] host array, or a
    device texture as a tuple (address, w, h); rotations -- None (the identity) or a 3x3 body -> world rotation; modes --
    "lit" / "emissive" or OBJECT_LIT / OBJECT_EMISSIVE (None: lit); emission -- the emissive strength (None: 0)."""
    ot, keep = ObjectTextures(), []
    if any(v is not None and len(v) > MAX_SPHERES for v in (textures, rotations, modes, emission)):
        raise ValueError(f"at most {MAX_SPHERES} spheres")
    for j, t in enumerate(textures or []):
        if t is None:
            continue
        if isinstance(t, tuple):
            ot.tex[j], ot.tex_w[j], ot.tex_h[j] = int(t[0]) or None, int(t[1]), int(t[2])
            continue
        a = np.ascontiguousarray(t, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError(f"texture of sphere {j} must be [h, w, 4] float32, not {a.shape}")
        ot.tex[j], ot.tex_w[j], ot.tex_h[j] = a.ctypes.data, a.shape[1], a.shape[0]
        keep.append(a)
    for j, r in enumerate(rotations if rotations is not None else []):
        if r is not None:
            ot.rot[j][:] = [float(v) for v in np.asarray(r, dtype=np.float64).reshape(9)]
    for j, m in enumerate(modes if modes is not None else []):
        if m is not None:
            ot.mode[j] = _OBJECT_MODE[m] if isinstance(m, str) else int(m)
    for j, k in enumerate(emission if emission is not None else []):
        if k is not None:
            ot.emission[j] = float(k)
    return ot, keep


class MeshMaterialStruct(C.Structure):
    """struct bhg_mesh_material (include/bhgeo.h)."""
    _fields_ = [("tri_rgb", C.c_void_p), ("tri_uv", C.c_void_p), ("tri_tex", C.c_void_p), ("tex", C.c_void_p * 8),
                ("tex_w", C.c_int32 * 8), ("tex_h", C.c_int32 * 8), ("n_tex", C.c_int32), ("emission", C.c_double)]


class MeshMaterial:
    """A mesh's surface (bhg_mesh_material), as host arrays: tri_rgb [nt, 3] float32 per triangle (None:
    white), tri_uv [nt, 3, 2] float32 per corner in the triangle's vertex order (None: no textures), tri_tex [nt] int32 image
    slot per triangle (< 0: none; None: slot 0), textures: up to 8 [h, w, 4] float32 RGBA images, row 0 at V = 0, repeating in
    both directions; emission >= 0 is added to the lamp sum.  colour = tri_rgb * texel * (lamp_sum + emission)."""

    def __init__(self, tri_rgb=None, tri_uv=None, tri_tex=None, textures=(), emission=0.0):
        self.tri_rgb = None if tri_rgb is None else np.ascontiguousarray(tri_rgb, dtype=np.float32)
        self.tri_uv = None if tri_uv is None else np.ascontiguousarray(tri_uv, dtype=np.float32)
        self.tri_tex = None if tri_tex is None else np.ascontiguousarray(tri_tex, dtype=np.int32)
        self.textures = [np.ascontiguousarray(t, dtype=np.float32) for t in textures]
        self.emission = float(emission)
        if self.tri_rgb is not None and (self.tri_rgb.ndim != 2 or self.tri_rgb.shape[1] != 3):
            raise ValueError("tri_rgb must have shape [n_triangles, 3]")
        if self.tri_uv is not None and self.tri_uv.shape[1:] != (3, 2):
            raise ValueError("tri_uv must have shape [n_triangles, 3, 2]")
        if self.tri_tex is not None and self.tri_tex.ndim != 1:
            raise ValueError("tri_tex must have shape [n_triangles]")
        if len(self.textures) > MESH_TEXTURES_MAX:
            raise ValueError(f"at most {MESH_TEXTURES_MAX} textures")
        for j, t in enumerate(self.textures):
            if t.ndim != 3 or t.shape[2] != 4:
                raise ValueError(f"texture {j} must be [h, w, 4] float32, not {t.shape}")

    def check_triangles(self, nt):
        for name in ("tri_rgb", "tri_uv", "tri_tex"):
            a = getattr(self, name)
            if a is not None and a.shape[0] != nt:
                raise ValueError(f"{name} must have one entry per triangle ({nt}), not {a.shape[0]}")

    def arrays(self):
        """(tri_rgb, tri_uv, tri_tex, *textures): the host arrays in the order struct() takes addresses, None where not given."""
        return (self.tri_rgb, self.tri_uv, self.tri_tex, *self.textures)

    def struct(self, addresses=None):
        """The C struct over this material's host arrays, or over `addresses` -- one per entry of arrays(), 0 / None for an
        array that is not given: the device copies."""
        if addresses is None:
            addresses = [None if a is None else a.ctypes.data for a in self.arrays()]
        m = MeshMaterialStruct()
        m.tri_rgb, m.tri_uv, m.tri_tex = (a or None for a in addresses[:3])
        for j, t in enumerate(self.textures):
            m.tex[j] = addresses[3 + j] or None
            m.tex_w[j], m.tex_h[j] = t.shape[1], t.shape[0]
        m.n_tex = len(self.textures)
        m.emission = self.emission
        return m


class Camera(C.Structure):
    """struct bhg_camera (include/bhgeo.h)."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("reserved", C.c_int32),
        ("fov_x", C.c_double), ("fov_y", C.c_double),
        ("rot", C.c_double * 9),
        ("origin", C.c_double * 3),
    ]


class Scene(C.Structure):
    """struct bhg_scene (include/bhgeo.h)."""
    _fields_ = [
        ("d_sky", C.c_void_p), ("sky_w", C.c_int32), ("sky_h", C.c_int32),
        ("d_disk_tex", C.c_void_p), ("disk_w", C.c_int32), ("disk_h", C.c_int32),
        ("disk_r_in", C.c_double), ("disk_r_out", C.c_double),
        ("disk_phase", C.c_double), ("disk_mean", C.c_double), ("disk_stddev", C.c_double),
        ("disk_intensity", C.c_double),
        ("n_spheres", C.c_int32), ("n_lamps", C.c_int32),
        ("spheres", (C.c_double * 4) * 8),
        ("sphere_rgb", (C.c_double * 3) * 8),
        ("lamps", (C.c_double * 4) * 4),
    ]


class FrameScene(C.Structure):
    """struct bhg_frame_scene (include/bhgeo.h): the scene of a library-owned frame, everything on the host."""
    _fields_ = [
        ("sky", C.c_void_p), ("sky_w", C.c_int32), ("sky_h", C.c_int32),
        ("disk_tex", C.c_void_p), ("disk_w", C.c_int32), ("disk_h", C.c_int32),
        ("disk_r_in", C.c_double), ("disk_r_out", C.c_double),
        ("disk_phase", C.c_double), ("disk_mean", C.c_double), ("disk_stddev", C.c_double),
        ("disk_intensity", C.c_double),
        ("n_spheres", C.c_int32), ("n_lamps", C.c_int32),
        ("spheres", (C.c_double * 4) * 8),
        ("sphere_rgb", (C.c_double * 3) * 8),
        ("lamps", (C.c_double * 4) * 4),
    ]


def make_scene(d_sky, sky_w, sky_h, *, d_disk_tex=0, disk_w=0, disk_h=0, disk=None, disk_phase=0.0, disk_mean=0.2,
               disk_stddev=0.3, disk_intensity=1.0, spheres=None, sphere_rgb=None, lamps=None):
    """disk=(R_in, R_out); spheres [[cx, cy, cz, radius]]; sphere_rgb [[r, g, b]] (default white);
    lamps [[x, y, z, intensity]].  Defaults of the disk profile: LimitedRelativisticRenderEngine.py:495-498."""
    sc = Scene()
    sc.d_sky, sc.sky_w, sc.sky_h = d_sky or None, int(sky_w), int(sky_h)
    sc.d_disk_tex, sc.disk_w, sc.disk_h = d_disk_tex or None, int(disk_w), int(disk_h)
    if disk is not None:
        sc.disk_r_in, sc.disk_r_out = float(disk[0]), float(disk[1])
    sc.disk_phase, sc.disk_mean, sc.disk_stddev, sc.disk_intensity = (float(disk_phase), float(disk_mean),
                                                                        float(disk_stddev), float(disk_intensity))
    sp = _spheres_array(spheres if spheres is not None else [])
    rgb = np.ones((len(sp), 3)) if sphere_rgb is None else np.asarray(sphere_rgb, dtype=np.float64).reshape(-1, 3)
    lm = np.zeros((0, 4)) if lamps is None else np.asarray(lamps, dtype=np.float64).reshape(-1, 4)
    if len(sp) > MAX_SPHERES or len(lm) > 4 or len(rgb) != len(sp):
        raise ValueError("at most 8 spheres (one colour each) and 4 lamps")
    sc.n_spheres, sc.n_lamps = len(sp), len(lm)
    for j in range(len(sp)):
        for q in range(4):
            sc.spheres[j][q] = float(sp[j, q])
        for q in range(3):
            sc.sphere_rgb[j][q] = float(rgb[j, q])
    for j in range(len(lm)):
        for q in range(4):
            sc.lamps[j][q] = float(lm[j, q])
    return sc


def _spheres_array(spheres):
    sp = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
    return sp if len(sp) else np.zeros((1, 4))[:0]


class BhgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbhgeo error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """struct bhg_params (include/bhgeo.h)."""
    _fields_ = [
        ("r_s", C.c_double),
        ("lambda_end", C.c_double),
        ("max_step", C.c_double),
        ("rtol", C.c_double),
        ("atol", C.c_double),
        ("h_fixed", C.c_double),
        ("r_exit", C.c_double),
        ("method", C.c_int32),
        ("rhs_form", C.c_int32),
        ("max_steps", C.c_uint32),
        ("order_blocks", C.c_uint32),
        ("disk_r_in", C.c_double),
        ("disk_r_out", C.c_double),
        ("spin", C.c_double),
        ("time_like", C.c_int32),
        ("reserved0", C.c_int32),
    ]


_lib = None
_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)


def load():
    """dlopen libbhgeo.so and declare the prototypes.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C blackhole_geodesic_calculator_amd/csrc` (hipcc, --offload-arch=gfx950). "
            "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 (SONAME
    # libamdhip64.so.7).  If torch is importable, import it first so that libbhgeo binds to that
    # already-loaded runtime; two runtimes in one process leave the second without a GPU.
    if "torch" not in sys.modules and not os.environ.get("BHGEO_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    L.bhg_version.restype = C.c_int
    L.bhg_device_count.restype = C.c_int
    L.bhg_last_error.restype = C.c_char_p
    L.bhg_default_params.restype = None
    L.bhg_default_params.argtypes = [C.POINTER(Params)]
    L.bhg_create.restype = C.c_int
    L.bhg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.bhg_destroy.restype = None
    L.bhg_destroy.argtypes = [C.c_void_p]
    L.bhg_device_name.restype = C.c_int
    L.bhg_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.bhg_num_cus.restype = C.c_int
    L.bhg_num_cus.argtypes = [C.c_void_p]
    L.bhg_trace.restype = C.c_int
    L.bhg_trace.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int, _dp, C.c_size_t, _dp, _u8p,
                            _u32p, _u32p]
    L.bhg_trace_device.restype = C.c_int
    L.bhg_trace_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
    L.bhg_trace_dir_device.restype = C.c_int
    L.bhg_trace_dir_device.argtypes = L.bhg_trace_device.argtypes
    L.bhg_trace_start_device.restype = C.c_int
    L.bhg_trace_start_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int32, _dp, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p]
    # (an addition within ABI 10, found by symbol: a library built before it -- BHGEO_LIB, an A/B against an older build -- serves
    # everything else, and the owners of a start cache then keep the start steps alone: has_start_prefix())
    if hasattr(L, "bhg_trace_prefix_device"):
        L.bhg_trace_prefix_device.restype = C.c_int
        L.bhg_trace_prefix_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int32, _dp, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.POINTER(Prefix), C.c_void_p]
        L.bhg_prefix_clearance.restype = C.c_double
        L.bhg_prefix_clearance.argtypes = [C.POINTER(Params), _dp, C.c_int32, _dp]
    if hasattr(L, "bhg_prefix_deep_attempts"):     # (a library from before the deep rule: has_deep_prefix())
        L.bhg_prefix_deep_attempts.restype = C.c_int32
        L.bhg_prefix_deep_attempts.argtypes = []
    if hasattr(L, "bhg_prefix_wide_accepted"):     # (a library from before the wide rule: has_wide_prefix())
        L.bhg_prefix_wide_accepted.restype = C.c_int32
        L.bhg_prefix_wide_accepted.argtypes = []
        L.bhg_prefix_owner_next.restype = C.c_int32
        L.bhg_prefix_owner_next.argtypes = [C.POINTER(PrefixOwner), C.c_int32, C.c_int32, C.POINTER(Params), _dp, C.c_int32, _dp, C.POINTER(Prefix)]
        L.bhg_frame_prefix_info.restype = C.c_int
        L.bhg_frame_prefix_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Prefix)]
    if hasattr(L, "bhg_prefix_rim_attempts"):      # (a library from before the rim rule: has_rim_prefix())
        L.bhg_prefix_rim_attempts.restype = C.c_int32
        L.bhg_prefix_rim_attempts.argtypes = []
    L.bhg_start_steps_match.restype = C.c_int
    L.bhg_start_steps_match.argtypes = [C.POINTER(Params), C.POINTER(Params)]
    L.bhg_shade_dir_device.restype = C.c_int
    L.bhg_shade_dir_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_trace_objects.restype = C.c_int
    L.bhg_trace_objects.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int32, _dp, C.c_int, _dp, C.c_size_t, _dp,
                                    _u8p, _u32p, _u32p, C.POINTER(C.c_int8)]
    L.bhg_trace_objects_device.restype = C.c_int
    L.bhg_trace_objects_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int32, _dp, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    L.bhg_shade_scene_device.restype = C.c_int
    L.bhg_shade_scene_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                         C.POINTER(Scene), C.c_void_p, C.c_void_p]
    L.bhg_shade_scene_f32_device.restype = C.c_int
    L.bhg_shade_scene_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                             C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_assemble_frame_f32_device.restype = C.c_int
    L.bhg_assemble_frame_f32_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_raygen_device.restype = C.c_int
    L.bhg_raygen_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _dp,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_shade_device.restype = C.c_int
    L.bhg_shade_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p,
                                   C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.bhg_trajectory.restype = C.c_int
    # (raw addresses: building a typed ctypes pointer costs ~2 us per array, and the engine's literal call is one ray long)
    L.bhg_trajectory.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_trajectory_objects.restype = C.c_int
    L.bhg_trajectory_objects.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_set_profiling.restype = C.c_int
    L.bhg_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.bhg_last_pass_ms.restype = C.c_int
    L.bhg_last_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.bhg_acceleration.restype = C.c_int
    L.bhg_acceleration.argtypes = [C.c_void_p, C.POINTER(Params), _dp, _dp, C.c_size_t, _dp]
    L.bhg_rays_create.restype = C.c_int
    L.bhg_rays_create.argtypes = [C.c_void_p, C.POINTER(Camera), _dp, C.c_int, C.POINTER(C.c_int64), C.c_size_t,
                                  C.POINTER(C.c_void_p)]
    L.bhg_rays_count.restype = C.c_size_t
    L.bhg_rays_count.argtypes = [C.c_void_p]
    L.bhg_rays_destroy.restype = None
    L.bhg_rays_destroy.argtypes = [C.c_void_p]
    L.bhg_rays_trace.restype = C.c_int
    L.bhg_rays_trace.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_int32, C.c_size_t, C.c_size_t, _dp, _dp, _dp, _u8p,
                                 _u32p, _u32p, C.POINTER(C.c_int8)]
    L.bhg_host_alloc.restype = C.c_int
    L.bhg_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.bhg_host_free.restype = C.c_int
    L.bhg_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.bhg_synchronize.restype = C.c_int
    L.bhg_synchronize.argtypes = [C.c_void_p]
    L.bhg_context_stream.restype = C.c_void_p
    L.bhg_context_stream.argtypes = [C.c_void_p]
    L.bhg_last_launch.restype = C.c_int
    L.bhg_last_launch.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.bhg_frame_create.restype = C.c_int
    L.bhg_frame_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(Camera), _dp, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_void_p)]
    L.bhg_frame_destroy.restype = None
    L.bhg_frame_destroy.argtypes = [C.c_void_p]
    L.bhg_frame_set_scene.restype = C.c_int
    L.bhg_frame_set_scene.argtypes = [C.c_void_p, C.POINTER(FrameScene)]
    L.bhg_frame_set_camera.restype = C.c_int
    L.bhg_frame_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
    L.bhg_frame_render.restype = C.c_int
    L.bhg_frame_render.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p]
    L.bhg_frame_synchronize.restype = C.c_int
    L.bhg_frame_synchronize.argtypes = [C.c_void_p]
    L.bhg_frame_device_image.restype = C.c_void_p
    L.bhg_frame_device_image.argtypes = [C.c_void_p]
    L.bhg_frame_rebalance.restype = C.c_int
    L.bhg_frame_rebalance.argtypes = [C.c_void_p, C.c_double]
    L.bhg_frame_stats.restype = C.c_int
    L.bhg_frame_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.bhg_frame_info.restype = C.c_int
    L.bhg_frame_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.bhg_frame_set_profiling.restype = C.c_int
    L.bhg_frame_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.bhg_frame_last_ms.restype = C.c_int
    L.bhg_frame_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bhg_deal_tiles.restype = C.c_int
    L.bhg_deal_tiles.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, C.c_double, C.c_int32,
                                 C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_size_t)]
    L.bhg_redshift_size.restype = C.c_size_t
    L.bhg_redshift_size.argtypes = []
    L.bhg_redshift_device.restype = C.c_int
    L.bhg_redshift_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), _dp, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_redshift_host.restype = C.c_int
    L.bhg_redshift_host.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]
    L.bhg_shade_scene_redshift_device.restype = C.c_int
    L.bhg_shade_scene_redshift_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                                  C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift), _dp, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_frame_set_redshift.restype = C.c_int
    L.bhg_frame_set_redshift.argtypes = [C.c_void_p, C.POINTER(Redshift)]
    L.bhg_observer_size.restype = C.c_size_t
    L.bhg_observer_size.argtypes = []
    L.bhg_raygen_observer_device.restype = C.c_int
    L.bhg_raygen_observer_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Observer), _dp, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_double, C.c_double, _dp, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p]
    L.bhg_redshift_observer_device.restype = C.c_int
    L.bhg_redshift_observer_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), C.POINTER(Observer), _dp,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_redshift_observer_host.restype = C.c_int
    L.bhg_redshift_observer_host.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), C.POINTER(Observer), C.c_void_p,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bhg_shade_scene_redshift_observer_device.restype = C.c_int
    L.bhg_shade_scene_redshift_observer_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                           C.c_int32, C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift),
                                                           C.POINTER(Observer), _dp, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_void_p]
    L.bhg_frame_set_observer.restype = C.c_int
    L.bhg_frame_set_observer.argtypes = [C.c_void_p, C.POINTER(Observer)]
    L.bhg_object_textures_size.restype = C.c_size_t
    L.bhg_object_textures_size.argtypes = []
    L.bhg_shade_scene_textured_device.restype = C.c_int
    L.bhg_shade_scene_textured_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                                  C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift), C.POINTER(Observer),
                                                  C.POINTER(ObjectTextures), _dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
    L.bhg_polarisation_size.restype = C.c_size_t
    L.bhg_polarisation_size.argtypes = []
    L.bhg_polarisation_device.restype = C.c_int
    L.bhg_polarisation_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Polarisation), C.POINTER(Observer), _dp,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    L.bhg_polarisation_host.restype = C.c_int
    L.bhg_polarisation_host.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Polarisation), C.POINTER(Observer), C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    L.bhg_shade_scene_polarised_device.restype = C.c_int
    L.bhg_shade_scene_polarised_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                   C.c_int32, C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift),
                                                   C.POINTER(Observer), C.POINTER(ObjectTextures), _dp, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.POINTER(Polarisation), C.c_void_p, C.c_void_p]
    L.bhg_frame_set_object_textures.restype = C.c_int
    L.bhg_frame_set_object_textures.argtypes = [C.c_void_p, C.POINTER(ObjectTextures)]
    L.bhg_disk_thermal_size.restype = C.c_size_t
    L.bhg_disk_thermal_size.argtypes = []
    L.bhg_disk_thermal_device.restype = C.c_int
    L.bhg_disk_thermal_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(DiskThermal), C.POINTER(Observer), _dp,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.bhg_disk_thermal_host.restype = C.c_int
    L.bhg_disk_thermal_host.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(DiskThermal), C.POINTER(Observer), C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_shade_scene_thermal_device.restype = C.c_int
    L.bhg_shade_scene_thermal_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                 C.c_int32, C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift),
                                                 C.POINTER(Observer), C.POINTER(ObjectTextures), _dp, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(Polarisation), C.c_void_p,
                                                 C.POINTER(DiskThermal), C.c_void_p]
    L.bhg_frame_set_disk_thermal.restype = C.c_int
    L.bhg_frame_set_disk_thermal.argtypes = [C.c_void_p, C.POINTER(DiskThermal)]
    L.bhg_object_motion_size.restype = C.c_size_t
    L.bhg_object_motion_size.argtypes = []
    L.bhg_redshift_motion_device.restype = C.c_int
    L.bhg_redshift_motion_device.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), C.POINTER(Observer),
                                             C.POINTER(ObjectMotion), C.c_void_p, C.c_int32, _dp, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_redshift_motion_host.restype = C.c_int
    L.bhg_redshift_motion_host.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Redshift), C.POINTER(Observer),
                                           C.POINTER(ObjectMotion), C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bhg_shade_scene_moving_device.restype = C.c_int
    L.bhg_shade_scene_moving_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_int32, C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift),
                                                C.POINTER(Observer), C.POINTER(ObjectTextures), _dp, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.POINTER(Polarisation), C.c_void_p,
                                                C.POINTER(DiskThermal), C.POINTER(ObjectMotion), C.c_void_p]
    L.bhg_frame_set_object_motion.restype = C.c_int
    L.bhg_frame_set_object_motion.argtypes = [C.c_void_p, C.POINTER(ObjectMotion)]
    L.bhg_trace_crossings_device.restype = C.c_int
    L.bhg_trace_crossings_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_trace_crossings.restype = C.c_int
    L.bhg_trace_crossings.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_disk_layers_size.restype = C.c_size_t
    L.bhg_disk_layers_size.argtypes = []
    L.bhg_shade_disk_layers_device.restype = C.c_int
    L.bhg_shade_disk_layers_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_int32, C.POINTER(Scene), C.POINTER(Params), C.POINTER(Redshift),
                                               C.POINTER(Observer), _dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(DiskThermal), C.POINTER(DiskLayers), C.c_void_p]
    L.bhg_travel_time_device.restype = C.c_int
    L.bhg_travel_time_device.argtypes = [C.c_void_p, C.POINTER(Params), _dp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    L.bhg_travel_time.restype = C.c_int
    L.bhg_travel_time.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_shade_disk_layers_retarded_device.restype = C.c_int
    L.bhg_shade_disk_layers_retarded_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_size_t, C.c_int32, C.POINTER(Scene), C.POINTER(Params),
                                                        C.POINTER(Redshift), C.POINTER(Observer), _dp, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.POINTER(DiskThermal), C.POINTER(DiskLayers),
                                                        C.c_void_p, C.c_double, C.c_void_p]
    L.bhg_mesh_create.restype = C.c_int
    L.bhg_mesh_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32,
                                  C.POINTER(C.c_void_p)]
    L.bhg_mesh_destroy.restype = None
    L.bhg_mesh_destroy.argtypes = [C.c_void_p]
    L.bhg_mesh_info.restype = C.c_int
    L.bhg_mesh_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp]
    L.bhg_mesh_bvh_host.restype = C.c_int
    L.bhg_mesh_bvh_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.bhg_trace_mesh_device.restype = C.c_int
    L.bhg_trace_mesh_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_double, _dp, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    L.bhg_trace_mesh.restype = C.c_int
    L.bhg_trace_mesh.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_shade_mesh_device.restype = C.c_int
    L.bhg_shade_mesh_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                        C.POINTER(Scene), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_mesh_material_size.restype = C.c_size_t
    L.bhg_mesh_material_size.argtypes = []
    L.bhg_shade_mesh_material_device.restype = C.c_int
    L.bhg_shade_mesh_material_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32,
                                                 C.POINTER(Scene), C.c_void_p, C.POINTER(MeshMaterialStruct), C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_mesh_instances_create.restype = C.c_int
    L.bhg_mesh_instances_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.bhg_mesh_instances_set.restype = C.c_int
    L.bhg_mesh_instances_set.argtypes = [C.c_void_p, C.c_void_p]
    L.bhg_mesh_instances_destroy.restype = None
    L.bhg_mesh_instances_destroy.argtypes = [C.c_void_p]
    L.bhg_mesh_instances_info.restype = C.c_int
    L.bhg_mesh_instances_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), _dp]
    L.bhg_mesh_instance_box_host.restype = C.c_int
    L.bhg_mesh_instance_box_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_trace_mesh_instances_device.restype = C.c_int
    L.bhg_trace_mesh_instances_device.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_double, _dp, C.c_void_p, C.c_void_p,
                                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
    L.bhg_trace_mesh_instances.restype = C.c_int
    L.bhg_trace_mesh_instances.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    L.bhg_shade_mesh_instances_device.restype = C.c_int
    L.bhg_shade_mesh_instances_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_int32, C.POINTER(Scene), C.c_void_p, C.POINTER(MeshMaterialStruct), C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_frame_set_mesh_instances.restype = C.c_int
    L.bhg_frame_set_mesh_instances.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.bhg_mesh_instances_create_tree.restype = C.c_int
    L.bhg_mesh_instances_create_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.bhg_mesh_instances_tree_info.restype = C.c_int
    L.bhg_mesh_instances_tree_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.bhg_mesh_instance_tree_host.restype = C.c_int
    L.bhg_mesh_instance_tree_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.bhg_frame_set_mesh_instance_tree.restype = C.c_int
    L.bhg_frame_set_mesh_instance_tree.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    L.bhg_mesh_refit.restype = C.c_int
    L.bhg_mesh_refit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_mesh_refit_device.restype = C.c_int
    L.bhg_mesh_refit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bhg_mesh_refit_info.restype = C.c_int
    L.bhg_mesh_refit_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), _dp, _dp]
    L.bhg_mesh_bvh_refit_host.restype = C.c_int
    L.bhg_mesh_bvh_refit_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p, _dp]
    L.bhg_mesh_refit_schedule_host.restype = C.c_int
    L.bhg_mesh_refit_schedule_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.bhg_mesh_range.restype = C.c_int
    L.bhg_mesh_range.argtypes = [C.c_void_p, _dp, _dp]
    L.bhg_mesh_boxes_host.restype = C.c_int
    L.bhg_mesh_boxes_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.bhg_mesh_create_device.restype = C.c_int
    L.bhg_mesh_create_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_size_t,
                                         C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
    L.bhg_mesh_rebuild_device.restype = C.c_int
    L.bhg_mesh_rebuild_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.bhg_mesh_rebuild.restype = C.c_int
    L.bhg_mesh_rebuild.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.bhg_mesh_build_info.restype = C.c_int
    L.bhg_mesh_build_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    L.bhg_mesh_bvh_morton_host.restype = C.c_int
    L.bhg_mesh_bvh_morton_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.bhg_mesh_tree_host.restype = C.c_int
    L.bhg_mesh_tree_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.bhg_frame_set_mesh_build.restype = C.c_int
    L.bhg_frame_set_mesh_build.argtypes = [C.c_void_p, C.c_int]
    L.bhg_frame_mesh_build_info.restype = C.c_int
    L.bhg_frame_mesh_build_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    L.bhg_frame_refit_mesh.restype = C.c_int
    L.bhg_frame_refit_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double]
    L.bhg_frame_mesh_refit_info.restype = C.c_int
    L.bhg_frame_mesh_refit_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), _dp, _dp]
    L.bhg_frame_set_mesh.restype = C.c_int
    L.bhg_frame_set_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_double,
                                     C.POINTER(MeshMaterialStruct)]
    if L.bhg_version() != ABI_VERSION or not hasattr(L, "bhg_abi_check"):
        raise ImportError(f"libbhgeo ABI {L.bhg_version()} != expected {ABI_VERSION}: rebuild {LIB_PATH}")
    for name in ("bhg_params_size", "bhg_camera_size", "bhg_scene_size", "bhg_frame_scene_size"):
        getattr(L, name).restype = C.c_size_t
        getattr(L, name).argtypes = []
    L.bhg_abi_check.restype = C.c_int
    L.bhg_abi_check.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.bhg_default_params_sized.restype = C.c_int
    L.bhg_default_params_sized.argtypes = [C.POINTER(Params), C.c_size_t]
    L.bhg_peak_probe.restype = C.c_int
    L.bhg_peak_probe.argtypes = [C.c_void_p, C.c_int32, C.c_double, _dp]
    L.bhg_math_probe.restype = C.c_int
    L.bhg_math_probe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
    # the handshake include/bhgeo.h asks of every binding: ABI version and the layout of every struct declared above
    if L.bhg_abi_check(ABI_VERSION, C.sizeof(Params), C.sizeof(Camera), C.sizeof(Scene), C.sizeof(FrameScene)) != OK:
        raise ImportError("libbhgeo: " + L.bhg_last_error().decode())
    if L.bhg_redshift_size() != C.sizeof(Redshift):
        raise ImportError(f"libbhgeo: bhg_redshift is {L.bhg_redshift_size()} bytes, this binding's {C.sizeof(Redshift)}")
    if L.bhg_observer_size() != C.sizeof(Observer):
        raise ImportError(f"libbhgeo: bhg_observer is {L.bhg_observer_size()} bytes, this binding's {C.sizeof(Observer)}")
    if L.bhg_object_motion_size() != C.sizeof(ObjectMotion):
        raise ImportError(f"libbhgeo: bhg_object_motion is {L.bhg_object_motion_size()} bytes, this binding's {C.sizeof(ObjectMotion)}")
    if L.bhg_disk_layers_size() != C.sizeof(DiskLayers):
        raise ImportError(f"libbhgeo: bhg_disk_layers is {L.bhg_disk_layers_size()} bytes, this binding's {C.sizeof(DiskLayers)}")
    if L.bhg_disk_thermal_size() != C.sizeof(DiskThermal):
        raise ImportError(f"libbhgeo: bhg_disk_thermal is {L.bhg_disk_thermal_size()} bytes, this binding's {C.sizeof(DiskThermal)}")
    if L.bhg_polarisation_size() != C.sizeof(Polarisation):
        raise ImportError(f"libbhgeo: bhg_polarisation is {L.bhg_polarisation_size()} bytes, this binding's {C.sizeof(Polarisation)}")
    if L.bhg_object_textures_size() != C.sizeof(ObjectTextures):
        raise ImportError(f"libbhgeo: bhg_object_textures is {L.bhg_object_textures_size()} bytes, this binding's "
                          f"{C.sizeof(ObjectTextures)}")
    if L.bhg_mesh_material_size() != C.sizeof(MeshMaterialStruct):
        raise ImportError(f"libbhgeo: bhg_mesh_material is {L.bhg_mesh_material_size()} bytes, this binding's "
                          f"{C.sizeof(MeshMaterialStruct)}")
    _lib = L
    return L


def _mesh_arrays(vertices, triangles):
    V = np.ascontiguousarray(vertices, dtype=np.float64)
    F = np.asarray(triangles)
    if V.ndim != 2 or V.shape[1] != 3:
        raise ValueError("vertices must have shape [nv, 3]")
    if F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("triangles must have shape [nt, 3]")
    if F.size and (F.min() < -2**31 or F.max() > 2**31 - 1):
        raise ValueError("triangle indices must fit int32")
    return V, np.ascontiguousarray(F, dtype=np.int32)


def mesh_bvh_host(vertices, triangles, leaf_size=4, _call="bhg_mesh_bvh_host"):
    """bhg_mesh_bvh_host: the flattened tree as the device gets it, built on the host (no context, no GPU) ->
    dict(box[nn,6], skip[nn], first[nn], count[nn], order[nt]).  On a box miss at node i go to skip[i], otherwise to i + 1; a leaf
    holds the triangles order[first : first + count]."""
    V, F = _mesh_arrays(vertices, triangles)
    nt = F.shape[0]
    cap = max(2 * nt - 1, 1)
    box = np.empty((cap, 6), np.float64)
    skip, first, count = (np.empty(cap, np.int32) for _ in range(3))
    order = np.empty(nt, np.int32)
    nn = C.c_size_t(0)
    _check(getattr(load(), _call)(_addr(V), V.shape[0], _addr(F), nt, int(leaf_size), _addr(box), _addr(skip), _addr(first),
                                  _addr(count), _addr(order), cap, C.byref(nn)))
    n = nn.value
    return {"box": box[:n].copy(), "skip": skip[:n].copy(), "first": first[:n].copy(), "count": count[:n].copy(), "order": order}


def mesh_bvh_morton_host(vertices, triangles, leaf_size=4):
    """bhg_mesh_bvh_morton_host: the tree the DEVICE build makes, stated on the host (no context, no GPU);
    mesh_bvh_host's dict.  The triangles in the order of a 63-bit Morton key of their centroids, every range split by count."""
    return mesh_bvh_host(vertices, triangles, leaf_size, _call="bhg_mesh_bvh_morton_host")


def _topology_arrays(tree):
    return tuple(np.ascontiguousarray(tree[k], dtype=np.int32) for k in ("skip", "first", "count", "order"))


def mesh_bvh_refit_host(vertices, triangles, tree):
    """bhg_mesh_bvh_refit_host: the CPU statement of the refit kernels (no context, no GPU).  tree: a dict
    with mesh_bvh_host's skip, first, count and order -> (box[nn, 6] refitted to `vertices` and widened, the tree's area sum)."""
    V, F = _mesh_arrays(vertices, triangles)
    skip, first, count, order = _topology_arrays(tree)
    box = np.empty((len(skip), 6), np.float64)
    area = C.c_double(0.0)
    _check(load().bhg_mesh_bvh_refit_host(_addr(V), V.shape[0], _addr(F), F.shape[0], _addr(skip), _addr(first), _addr(count),
                                          _addr(order), len(skip), _addr(box), C.byref(area)))
    return box, area.value


def mesh_refit_schedule_host(tree):
    """bhg_mesh_refit_schedule_host: the refit's bottom-up schedule for mesh_bvh_host's tree -> (level_nodes[n_inner],
    level_off[34]): level_nodes[level_off[d]:level_off[d + 1]] are the inner nodes d levels below the root; deepest level first."""
    skip, first, count, order = _topology_arrays(tree)
    cap = max(len(order) - 1, 1)
    nodes, off = np.empty(cap, np.int32), np.empty(34, np.int32)
    n = C.c_size_t(0)
    _check(load().bhg_mesh_refit_schedule_host(_addr(skip), _addr(first), _addr(count), _addr(order), len(skip), len(order),
                                               _addr(nodes), _addr(off), cap, C.byref(n)))
    return nodes[:n.value].copy(), off


def _device_f64(a, shape, what, dtype="float64"):
    """The device address of a float64, C-contiguous device array of the given shape: anything with data_ptr() (a torch tensor)."""
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{what} must have shape {list(shape)}")
    if dtype not in str(a.dtype) or not a.is_contiguous() or not getattr(a, "is_cuda", True):
        raise ValueError(f"{what} must be a contiguous {dtype} device array")
    return a.data_ptr()


def _device_mesh_arrays(vertices, triangles, normals):
    """(addresses of V, F, N or None, nv, nt) of device arrays [nv, 3] float64, [nt, 3] int32, [nv, 3] float64"""
    if len(vertices.shape) != 2 or len(triangles.shape) != 2:
        raise ValueError("vertices must have shape [nv, 3] and triangles [nt, 3]")
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    dv = _device_f64(vertices, (nv, 3), "vertices")
    df = _device_f64(triangles, (nt, 3), "triangles", "int32")
    dn = None if normals is None else _device_f64(normals, (nv, 3), "vertex_normals")
    return dv, df, dn, nv, nt


def _capacity(capacity):
    """capacity: None (the counts themselves: 0, 0) or (cap_vertices, cap_triangles)"""
    if capacity is None:
        return 0, 0
    cv, ct = (int(x) for x in capacity)
    if cv < 0 or ct < 0:
        raise ValueError("capacity must be (cap_vertices, cap_triangles), both >= 0")
    return cv, ct


class Mesh:
    """bhg_mesh: a triangle mesh on a context's device.  vertices [nv, 3] float64, Cartesian and centred on
    the hole; triangles [nt, 3] int32; vertex_normals [nv, 3] or None (flat shading).  Closes with its context."""

    def __init__(self, ctx: "Context", vertices, triangles, vertex_normals=None, leaf_size=4, build="host", capacity=None):
        """build: "host" (bhg_mesh_create, the default) or "device" (the arrays are uploaded and the tree is built there,
        DESIGN.md section 23).  capacity: (cap_vertices, cap_triangles) a device-built mesh reserves for later rebuild() calls;
        None: the counts themselves."""
        if build not in ("host", "device"):
            raise ValueError('build must be "host" or "device"')
        if build == "host" and capacity is not None:
            raise ValueError('capacity goes with build="device": a host-built mesh has its own counts as capacity')
        V, F = _mesh_arrays(vertices, triangles)
        N = None
        if vertex_normals is not None:
            N = np.ascontiguousarray(vertex_normals, dtype=np.float64)
            if N.shape != V.shape:
                raise ValueError("vertex_normals must have the shape of vertices")
        if build == "device":
            import torch
            dev = torch.device("cuda", ctx.device)
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)   # noqa: E731
            self._adopt(ctx, *self._create_device(ctx, up(V), up(F), up(N), leaf_size, capacity, 0))
            return
        h = C.c_void_p()
        _check(load().bhg_mesh_create(ctx._h, _addr(V), V.shape[0], _addr(F), F.shape[0], None if N is None else _addr(N),
                                      int(leaf_size), C.byref(h)))
        self._adopt(ctx, h, V.shape[0], F.shape[0], N is not None)

    def _adopt(self, ctx, h, nv, nt, has_normals):
        self._h = h
        self.ctx = ctx
        self.n_vertices, self.n_triangles = nv, nt
        self.has_normals = has_normals
        self._instances = []
        ctx._meshes.append(self)

    @staticmethod
    def _create_device(ctx, d_vertices, d_triangles, d_normals, leaf_size, capacity, stream):
        dv, df, dn, nv, nt = _device_mesh_arrays(d_vertices, d_triangles, d_normals)
        cv, ct = _capacity(capacity)
        h = C.c_void_p()
        _check(load().bhg_mesh_create_device(ctx._h, C.c_void_p(dv), nv, C.c_void_p(df), nt, C.c_void_p(dn), int(leaf_size), cv, ct,
                                             C.c_void_p(stream or None), C.byref(h)))
        return h, nv, nt, dn is not None

    @classmethod
    def from_device(cls, ctx: "Context", d_vertices, d_triangles, d_normals=None, leaf_size=4, capacity=None, stream=0):
        """bhg_mesh_create_device: a mesh built on the device from arrays that lie there (torch tensors on the context's device:
        vertices and normals [nv, 3] float64, triangles [nt, 3] int32, contiguous).  Blocking."""
        self = cls.__new__(cls)
        self._adopt(ctx, *cls._create_device(ctx, d_vertices, d_triangles, d_normals, leaf_size, capacity, stream))
        return self

    def rebuild(self, vertices, triangles, vertex_normals=None, stream=0):
        """A new triangle list (and vertices, and normals for a mesh created with them) into the mesh, within its capacity: the tree
        is built anew on the device, in place (bhg_mesh_rebuild / bhg_mesh_rebuild_device).  numpy arrays go
        through the host call, device arrays (all of them) through the device call on `stream`.  Blocking.  Instance sets of the
        mesh need a set() afterwards."""
        dev = hasattr(vertices, "data_ptr")
        if hasattr(triangles, "data_ptr") != dev or (vertex_normals is not None and hasattr(vertex_normals, "data_ptr") != dev):
            raise ValueError("vertices, triangles and vertex_normals must all be host arrays or all device arrays")
        if dev:
            dv, df, dn, nv, nt = _device_mesh_arrays(vertices, triangles, vertex_normals)
            _check(load().bhg_mesh_rebuild_device(self.ctx._h, self._h, C.c_void_p(dv), nv, C.c_void_p(df), nt, C.c_void_p(dn),
                                                  C.c_void_p(stream or None)))
        else:
            V, F = _mesh_arrays(vertices, triangles)
            N = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, dtype=np.float64)
            if N is not None and N.shape != V.shape:
                raise ValueError("vertex_normals must have the shape of vertices")
            nv, nt = V.shape[0], F.shape[0]
            _check(load().bhg_mesh_rebuild(self.ctx._h, self._h, _addr(V), nv, _addr(F), nt, None if N is None else _addr(N)))
        self.n_vertices, self.n_triangles = nv, nt

    def build_info(self):
        """dict(built_on_device, builds, cap_vertices, cap_triangles, allocations) (bhg_mesh_build_info): builds counts the creating
        build too; allocations the device allocations made over the mesh's life."""
        dev, builds, cv, ct, allocs = C.c_int32(0), C.c_uint64(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        _check(load().bhg_mesh_build_info(self._h, C.byref(dev), C.byref(builds), C.byref(cv), C.byref(ct), C.byref(allocs)))
        return {"built_on_device": bool(dev.value), "builds": builds.value, "cap_vertices": cv.value, "cap_triangles": ct.value,
                "allocations": allocs.value}

    def download_tree(self):
        """dict(skip[nn], first[nn], count[nn], order[nt]): the device's topology and leaf order (bhg_mesh_tree_host; blocking)"""
        nn = self.info()[0]
        skip, first, count = (np.empty(nn, np.int32) for _ in range(3))
        order = np.empty(self.n_triangles, np.int32)
        n = C.c_size_t(0)
        _check(load().bhg_mesh_tree_host(self._h, _addr(skip), _addr(first), _addr(count), _addr(order), nn, C.byref(n)))
        return {"skip": skip, "first": first, "count": count, "order": order}

    def close(self):
        if getattr(self, "_h", None):
            for inst in list(getattr(self, "_instances", ())):
                inst.close()
            load().bhg_mesh_destroy(self._h)
            self._h = None
            if self in self.ctx._meshes:
                self.ctx._meshes.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(n_nodes, depth, box[6]) of the tree"""
        nn, depth, box = C.c_int64(0), C.c_int32(0), (C.c_double * 6)()
        _check(load().bhg_mesh_info(self._h, C.byref(nn), C.byref(depth), box))
        return nn.value, depth.value, np.array(box[:])

    def refit(self, vertices, vertex_normals=None, stream=0):
        """New vertex positions [nv, 3] (and vertex normals, for a mesh created with them) into the built mesh: the tree is
        refitted on the device, nothing is rebuilt (bhg_mesh_refit / bhg_mesh_refit_device).  numpy arrays
        go through the host call; anything with data_ptr() (a torch tensor on the mesh's device, float64, contiguous) through the
        device call on `stream`.  Blocking.  Instance sets of the mesh need a set() afterwards."""
        dev = hasattr(vertices, "data_ptr")
        if vertex_normals is not None and hasattr(vertex_normals, "data_ptr") != dev:
            raise ValueError("vertices and vertex_normals must both be host arrays or both device arrays")
        shape = (self.n_vertices, 3)
        if dev:
            dv = _device_f64(vertices, shape, "vertices")
            dn = None if vertex_normals is None else _device_f64(vertex_normals, shape, "vertex_normals")
            _check(load().bhg_mesh_refit_device(self.ctx._h, self._h, C.c_void_p(dv), C.c_void_p(dn), C.c_void_p(stream or None)))
            return
        V = np.ascontiguousarray(vertices, dtype=np.float64)
        N = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, dtype=np.float64)
        if V.shape != shape or (N is not None and N.shape != shape):
            raise ValueError(f"vertices (and vertex_normals) must have the mesh's shape {list(shape)}")
        _check(load().bhg_mesh_refit(self.ctx._h, self._h, _addr(V), None if N is None else _addr(N)))

    def refit_info(self):
        """(generation, area_build, area_now): refits so far, and the tree's area sum at creation and now (bhg_mesh_refit_info)"""
        g, a, b = C.c_uint64(0), C.c_double(0.0), C.c_double(0.0)
        _check(load().bhg_mesh_refit_info(self._h, C.byref(g), C.byref(a), C.byref(b)))
        return g.value, a.value, b.value

    def distance_range(self):
        """(d_min, d_max): the distances from the origin the mesh lies between (bhg_mesh_range)"""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _check(load().bhg_mesh_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def download_boxes(self):
        """(box[nn, 6], tri[nt, 9]): the device's node boxes and slot records v0, e1, e2 (bhg_mesh_boxes_host; blocking)"""
        nn = self.info()[0]
        box, tri = np.empty((nn, 6), np.float64), np.empty((self.n_triangles, 9), np.float64)
        _check(load().bhg_mesh_boxes_host(self._h, _addr(box), _addr(tri), nn))
        return box, tri


def _instance_transforms(transforms):
    T = np.ascontiguousarray(transforms, dtype=np.float64)
    if T.ndim == 3 and T.shape[1:] == (3, 4):
        # [K, 3, 4] = (R | t) -> R row-major, then t
        T = np.ascontiguousarray(np.concatenate([T[:, :, :3].reshape(-1, 9), T[:, :, 3]], axis=1))
    if T.ndim != 2 or T.shape[1] != 12:
        raise ValueError("transforms must have shape [K, 12] (R row-major, then t) or [K, 3, 4] (R | t)")
    return T


def rigid_transform(matrix):
    """The rigid record nearest to a 4 x 4 (or 3 x 4) affine matrix -> [12] float64, R row-major then t.  R is the polar part of
    the upper 3 x 3 block (U V^T of its SVD: the rotation nearest in the Frobenius norm, any scale dropped), t the last column.
    Matrices kept in float32 are orthonormal only to about 1e-7, which bhg_mesh_instances_create refuses; this makes them exact to
    rounding.  A block with a reflection (det <= 0) or a collapsed axis is refused."""
    M = np.asarray(matrix, dtype=np.float64)
    if M.shape not in ((4, 4), (3, 4)) or not np.all(np.isfinite(M)):
        raise ValueError("matrix must be a finite 4 x 4 or 3 x 4 array")
    A = M[:3, :3]
    if not np.linalg.det(A) > 0.0:
        raise ValueError("matrix must not mirror or collapse: det of the 3 x 3 block must be > 0")
    U, _, Vt = np.linalg.svd(A)
    return np.concatenate([(U @ Vt).reshape(9), M[:3, 3]])


def mesh_instance_box_host(local_box, transform):
    """bhg_mesh_instance_box_host: the world box (lo, hi) of a local box (lo, hi) under one rigid transform [12]; no GPU."""
    lb = np.ascontiguousarray(local_box, dtype=np.float64).reshape(6)
    T = np.asarray(transform, dtype=np.float64)
    T = _instance_transforms(T.reshape((1,) + T.shape))
    out = np.empty(6, np.float64)
    _check(load().bhg_mesh_instance_box_host(_addr(lb), _addr(T), _addr(out)))
    return out


class MeshInstances:
    """bhg_mesh_instances: K rigid placements of one Mesh.  transforms [K, 12] (R row-major, then t) or
    [K, 3, 4] (R | t), x_world = R x_local + t.  set(transforms) moves them: K x 18 doubles go to the device, no tree is touched.
    Closes with its mesh.
    tree=True (bhg_mesh_instances_create_tree): the placements lie under a tree of boxes with leaves of
    leaf_size, up to MESH_INSTANCE_TREE_MAX of them; every call takes such a set, the results are the linear set's bit for bit,
    and set() builds the tree's order and boxes anew on the host and sends records and tree in one upload."""

    def __init__(self, mesh: "Mesh", transforms, tree=False, leaf_size=MESH_INSTANCE_TREE_LEAF):
        T = _instance_transforms(transforms)
        h = C.c_void_p()
        if tree:
            _check(load().bhg_mesh_instances_create_tree(mesh.ctx._h, mesh._h, T.shape[0], _addr(T), int(leaf_size), C.byref(h)))
        else:
            _check(load().bhg_mesh_instances_create(mesh.ctx._h, mesh._h, T.shape[0], _addr(T), C.byref(h)))
        self._h = h
        self.tree = bool(tree)
        self.mesh = mesh
        self.n = T.shape[0]
        self.transforms = T.copy()      # (the latest: a refit of the mesh wants them set again)
        mesh._instances.append(self)

    def set(self, transforms):
        T = _instance_transforms(transforms)
        if T.shape[0] != self.n:
            raise ValueError(f"set takes the {self.n} transforms the set was created with, not {T.shape[0]}")
        _check(load().bhg_mesh_instances_set(self._h, _addr(T)))
        self.transforms = T.copy()

    def close(self):
        if getattr(self, "_h", None):
            load().bhg_mesh_instances_destroy(self._h)
            self._h = None
            if self in self.mesh._instances:
                self.mesh._instances.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """(n, box[6]): the number of instances and the union of their world boxes"""
        n, box = C.c_int32(0), (C.c_double * 6)()
        _check(load().bhg_mesh_instances_info(self._h, C.byref(n), box))
        return n.value, np.array(box[:])

    def tree_info(self):
        """(n_nodes, depth, leaf_size) of the tree the set lies under; all zeros for a linear set"""
        nn, depth, leaf = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(load().bhg_mesh_instances_tree_info(self._h, C.byref(nn), C.byref(depth), C.byref(leaf)))
        return nn.value, depth.value, leaf.value


def mesh_instance_tree_host(local_box, transforms, leaf_size=MESH_INSTANCE_TREE_LEAF):
    """bhg_mesh_instance_tree_host: the tree a set of tree=True builds over the placements `transforms` of a mesh whose root box
    is local_box (lo, hi) -> (node_box[nn, 6], node_skip[nn], node_first[nn], node_count[nn], inst_order[K], depth); no GPU."""
    lb = np.ascontiguousarray(local_box, dtype=np.float64).reshape(6)
    T = _instance_transforms(transforms)
    K = T.shape[0]
    cap = max(2 * K - 1, 1)
    box = np.empty((cap, 6), np.float64)
    skip, first, count = (np.empty(cap, np.int32) for _ in range(3))
    order = np.empty(max(K, 1), np.int32)
    nn, depth = C.c_int32(0), C.c_int32(0)
    _check(load().bhg_mesh_instance_tree_host(_addr(lb), K, _addr(T), int(leaf_size), _addr(box), _addr(skip), _addr(first),
                                              _addr(count), _addr(order), C.byref(nn), C.byref(depth)))
    n = nn.value
    return box[:n].copy(), skip[:n].copy(), first[:n].copy(), count[:n].copy(), order[:K].copy(), depth.value


def start_steps_match(a: "Params", b: "Params") -> bool:
    """bhg_start_steps_match: do the two parameter sets give every ray the same initial step?  (The library holds the list.)"""
    return bool(load().bhg_start_steps_match(C.byref(a), C.byref(b)))


def has_start_prefix() -> bool:
    """Does the loaded library know the rays' start-up records (bhg_trace_prefix_device)?"""
    return hasattr(load(), "bhg_trace_prefix_device")


def has_deep_prefix() -> bool:
    """Does the loaded library take BHG_PREFIX_RECORD_DEEP (it then exports bhg_prefix_deep_attempts)?"""
    return has_start_prefix() and hasattr(load(), "bhg_prefix_deep_attempts")


def has_wide_prefix() -> bool:
    """Does the loaded library take BHG_PREFIX_RECORD_WIDE and decide an owner's re-recording (it then exports
    bhg_prefix_wide_accepted and bhg_prefix_owner_next)?"""
    return has_deep_prefix() and hasattr(load(), "bhg_prefix_wide_accepted")


def has_rim_prefix() -> bool:
    """Does the loaded library take BHG_PREFIX_RECORD_RIM, as a mode and as the rule bhg_prefix_owner_next promotes to (it then
    exports bhg_prefix_rim_attempts)?"""
    return has_wide_prefix() and hasattr(load(), "bhg_prefix_rim_attempts")


def prefix_owner_next(owner: "PrefixOwner", rule: int, params: "Params", x0, spheres=None, last: "Prefix" = None,
                      promote: int = PREFIX_NONE) -> int:
    """bhg_prefix_owner_next: what the owner's next call asks for -- PREFIX_REPLAY, rule or promote (record now, by that rule) or
    PREFIX_NONE."""
    sp = None if spheres is None else _spheres_array(spheres)
    xs = (C.c_double * 3)(*[float(v) for v in x0])
    return int(load().bhg_prefix_owner_next(C.byref(owner), rule, promote, C.byref(params), None if sp is None or not len(sp) else _np_dp(sp),
                                            0 if sp is None else len(sp), xs, None if last is None else C.byref(last)))


def prefix_clearance(params: "Params", x0, spheres=None) -> float:
    """bhg_prefix_clearance: distance from x0 to the nearest event surface of a call with these parameters and spheres."""
    sp = None if spheres is None else _spheres_array(spheres)
    xs = (C.c_double * 3)(*[float(v) for v in x0])
    return float(load().bhg_prefix_clearance(C.byref(params), None if sp is None or not len(sp) else _np_dp(sp),
                                             0 if sp is None else len(sp), xs))


def _check(rc):
    if rc != OK:
        raise BhgError(rc, load().bhg_last_error().decode())


def default_params() -> Params:
    p = Params()
    _check(load().bhg_default_params_sized(C.byref(p), C.sizeof(p)))
    return p


def make_params(r_s=1.0, lambda_end=50.0, max_step=np.inf, rtol=1e-3, atol=1e-6, h_fixed=0.1,
                r_exit=0.0, method=METHOD_DP54, rhs_form=RHS_CHRISTOFFEL, max_steps=0, disk_r_in=0.0,
                disk_r_out=0.0, spin=0.0, order_blocks=0, time_like=0) -> Params:
    return Params(float(r_s), float(lambda_end), float(max_step), float(rtol), float(atol),
                  float(h_fixed), float(r_exit), int(method), int(rhs_form), int(max_steps), int(order_blocks),
                  float(disk_r_in), float(disk_r_out), float(spin), int(bool(time_like)), 0)


def device_count() -> int:
    return load().bhg_device_count()


def _np_dp(a):
    return a.ctypes.data_as(_dp)


def _addr(a):
    """The address of a numpy array's first element (for void* parameters)."""
    return a.__array_interface__["data"][0]


class _PinnedBlock:
    """One bhg_host_alloc block.  Page-locking is slow (tens of ms for a few hundred MB), so blocks are pooled:
    when the last numpy view of a block dies, the block goes back to its pool's free list instead of to the OS."""

    def __init__(self, nbytes, pool):
        p = C.c_void_p()
        # (the owning context: the allocation is made with ITS device current, not device 0)
        _check(load().bhg_host_alloc(pool.ctx_handle() if pool is not None else None, int(nbytes), C.byref(p)))
        self.ptr, self.nbytes, self.pool = p.value, int(nbytes), pool

    def release(self):
        if self.ptr:
            load().bhg_host_free(None, C.c_void_p(self.ptr))
            self.ptr = None


class PinnedPool:
    """Page-locked result arrays for the host-buffer calls (Context.trace): numpy arrays over bhg_host_alloc
    memory, so the device's copy engines write results straight into what the caller gets -- no staging copy."""

    def __init__(self, max_free_bytes=2 << 30, ctx=None):
        self._free = {}          # nbytes -> [blocks]
        self._free_bytes = 0
        self.max_free_bytes = int(max_free_bytes)
        self._ctx = ctx          # the owning Context (None: allocations are made on the current device)
        self._closed = False

    def ctx_handle(self):
        return getattr(self._ctx, "_h", None) if self._ctx is not None else None

    def _give_back(self, blk):
        if blk.ptr is None:
            return
        if self._closed or self._free_bytes + blk.nbytes > self.max_free_bytes:
            blk.release()        # (a block that comes home after Context.close() is freed, not pooled for nobody)
            return
        self._free.setdefault(blk.nbytes, []).append(blk)
        self._free_bytes += blk.nbytes

    def empty(self, shape, dtype):
        import weakref
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        if n == 0:
            return np.empty(shape, dtype)
        size = (n + 4095) & ~4095
        lst = self._free.get(size)
        if lst:
            blk = lst.pop()
            self._free_bytes -= blk.nbytes
        else:
            try:
                blk = _PinnedBlock(size, self)
            except BhgError:
                # page-locking failed (pin limit, a 67-M-ray frame): a pageable array still works, it crosses the
                # library's staging ring instead of being written by the copy engines directly
                return np.empty(shape, dtype)
        buf = (C.c_char * n).from_address(blk.ptr)
        weakref.finalize(buf, PinnedPool._give_back, self, blk)   # the array's base chain holds `buf`
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def clear(self):
        for lst in self._free.values():
            for blk in lst:
                blk.release()
        self._free.clear()
        self._free_bytes = 0

    def close(self):
        self.clear()
        self._closed = True


class RaySet:
    """bhg_rays: the camera rays of one frame, generated on the device and resident there (include/bhgeo.h).
    Ray s * n_pixels + p is sample s of pixel p."""

    def __init__(self, ctx: "Context", width, height, samples, fov_x, fov_y, origin, rot=None, jitter=None,
                 jitter_is_compact=False, pixels=None):
        cam = Camera()
        cam.width, cam.height, cam.samples = int(width), int(height), int(samples)
        cam.fov_x, cam.fov_y = float(fov_x), float(fov_y)
        r = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64).reshape(3, 3)
        cam.rot[:] = [float(v) for v in r.reshape(9)]
        cam.origin[:] = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3)]
        jit = None if jitter is None else np.ascontiguousarray(jitter, dtype=np.float64).reshape(-1)
        pix = None if pixels is None else np.ascontiguousarray(pixels, dtype=np.int64).reshape(-1)
        n_pixels = int(width) * int(height) if pix is None else len(pix)
        need = 2 * int(samples) * (n_pixels if jitter_is_compact else int(width) * int(height))
        if jit is not None and len(jit) < need:
            raise ValueError(f"jitter stream too short: {len(jit)} < {need}")
        h = C.c_void_p()
        _check(load().bhg_rays_create(ctx._h, C.byref(cam), None if jit is None else _np_dp(jit), 1 if jitter_is_compact else 0,
                                      None if pix is None else pix.ctypes.data_as(C.POINTER(C.c_int64)), n_pixels, C.byref(h)))
        self._h, self.ctx = h, ctx
        self.n_pixels, self.samples = n_pixels, int(samples)
        self.n = int(load().bhg_rays_count(h))

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):    # the context frees nothing of ours; but never touch a dead one
                load().bhg_rays_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def trace(self, params: "Params", first=0, n=None, want=("end", "flags", "n_steps", "n_accepted"), spheres=None):
        """Trace rays [first, first + n); returns a dict of the arrays named in `want` (of: end [n,6], end_loc [n,3],
        end_dir [n,3], flags, n_steps, n_accepted, object_id), page-locked from the context's pool."""
        n = self.n - int(first) if n is None else int(n)
        pool = self.ctx.pinned
        new = pool.empty if n >= 65536 else (lambda shape, dt: np.empty(shape, dt))
        spec = {"end": ((n, 6), np.float64), "end_loc": ((n, 3), np.float64), "end_dir": ((n, 3), np.float64),
                "flags": ((n,), np.uint8), "n_steps": ((n,), np.uint32), "n_accepted": ((n,), np.uint32),
                "object_id": ((n,), np.int8)}
        out = {k: new(*spec[k]) for k in want}

        def ptr(k, typ):
            return out[k].ctypes.data_as(typ) if k in out else None
        sp = None if spheres is None else _spheres_array(spheres)
        _check(load().bhg_rays_trace(self._h, C.byref(params), None if sp is None else _np_dp(sp), 0 if sp is None else len(sp),
                                     int(first), n, ptr("end", _dp), ptr("end_loc", _dp), ptr("end_dir", _dp), ptr("flags", _u8p),
                                     ptr("n_steps", _u32p), ptr("n_accepted", _u32p), ptr("object_id", C.POINTER(C.c_int8))))
        return out


def deal_tiles(width, height, tile, world, rank, tile_cost=None, visit_by_cost=True, root_share=1.0):
    """bhg_deal_tiles: the pixel list of device `rank` of a library-owned frame (host logic, no GPU needed).
    tile_cost: None or one figure per tile, row-major over the tile grid; root_share: rank 0's part of an equal share."""
    n = C.c_size_t()
    tc = None if tile_cost is None else np.ascontiguousarray(tile_cost, dtype=np.float64).reshape(-1)
    args = (int(width), int(height), int(tile), int(world), None if tc is None else _np_dp(tc), 1 if visit_by_cost else 0,
            float(root_share), int(rank))
    _check(load().bhg_deal_tiles(*args, None, 0, C.byref(n)))
    px = np.empty(n.value, dtype=np.int64)
    _check(load().bhg_deal_tiles(*args, px.ctypes.data_as(C.POINTER(C.c_int64)), px.size, C.byref(n)))
    return px


class Frame:
    """bhg_frame: a whole frame owned by the library -- jitter stream -> rays -> geodesics -> shaded, sample-averaged
    float RGBA pixels in frame order -- on one or several GPUs of this one process (include/bhgeo.h).  No torch.

    devices: device indices; an index may be repeated ({0, 0}: several contexts of one GPU, the N > 1 code path on a
    one-GPU machine).  jitter: the full-frame stream [S*H*W*2] of random.random() draws, or None = pixel centres.
    origin is BH-centred; rot a 3x3 rotation matrix (None = identity)."""

    def __init__(self, devices, width, height, samples, *, fov_x=1.0, fov_y=1.0, origin=(1e-4, 0.0, 30.0), rot=None,
                 jitter=None, tile=32, gather=GATHER_AUTO):
        cam = self._camera(width, height, samples, fov_x, fov_y, origin, rot)
        devs = [int(d) for d in (devices if hasattr(devices, "__len__") else [devices])]
        jit = None if jitter is None else np.ascontiguousarray(jitter, dtype=np.float64).reshape(-1)
        need = 2 * cam.samples * cam.width * cam.height
        if jit is not None and len(jit) < need:
            raise ValueError(f"jitter stream too short: {len(jit)} < {need}")
        h = C.c_void_p()
        _check(load().bhg_frame_create((C.c_int32 * len(devs))(*devs), len(devs), C.byref(cam),
                                       None if jit is None else _np_dp(jit), int(tile), int(gather), C.byref(h)))
        self._h = h
        self.devices, self.W, self.H, self.S = devs, cam.width, cam.height, cam.samples
        self._scene = FrameScene()
        self._scene.disk_mean, self._scene.disk_stddev, self._scene.disk_intensity = 0.2, 0.3, 1.0

    @staticmethod
    def _camera(width, height, samples, fov_x, fov_y, origin, rot):
        cam = Camera()
        cam.width, cam.height, cam.samples = int(width), int(height), int(samples)
        cam.fov_x, cam.fov_y = float(fov_x), float(fov_y)
        r = np.eye(3) if rot is None else np.asarray(rot, dtype=np.float64).reshape(3, 3)
        cam.rot[:] = [float(v) for v in r.reshape(9)]
        cam.origin[:] = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(3)]
        return cam

    def set_camera(self, *, fov_x, fov_y, origin, rot=None):
        """Move the camera (bhg_frame_set_camera): the frame, its jitter stream and its buffers stay.  A new origin is free;
        a new rotation / field of view regenerates the rays on the devices at the next render."""
        cam = self._camera(self.W, self.H, self.S, fov_x, fov_y, origin, rot)
        _check(load().bhg_frame_set_camera(self._h, C.byref(cam)))

    def close(self):
        if getattr(self, "_h", None):
            load().bhg_frame_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, sky=None, *, disk=None, disk_tex=None, disk_phase=0.0, disk_mean=0.2, disk_stddev=0.3,
                  disk_intensity=1.0, spheres=None, sphere_rgb=None, lamps=None):
        """sky [h, w, 4] float32 equirectangular (None: keep the current one); disk = (R_in, R_out) or None; disk_tex
        [h, w, 4] float32 or None; spheres [[cx, cy, cz, radius]] BH-centred, sphere_rgb (default white), lamps
        [[x, y, z, intensity]].  The whole scene is replaced by each call (images are kept when not given)."""
        sc = FrameScene()
        keep = []
        if sky is not None:
            a = np.ascontiguousarray(sky, dtype=np.float32)
            assert a.ndim == 3 and a.shape[2] == 4
            sc.sky, sc.sky_w, sc.sky_h = a.ctypes.data, a.shape[1], a.shape[0]
            keep.append(a)
        if disk_tex is not None:
            t = np.ascontiguousarray(disk_tex, dtype=np.float32)
            assert t.ndim == 3 and t.shape[2] == 4
            sc.disk_tex, sc.disk_w, sc.disk_h = t.ctypes.data, t.shape[1], t.shape[0]
            keep.append(t)
        if disk is not None:
            sc.disk_r_in, sc.disk_r_out = float(disk[0]), float(disk[1])
        sc.disk_phase, sc.disk_mean, sc.disk_stddev, sc.disk_intensity = (float(disk_phase), float(disk_mean),
                                                                            float(disk_stddev), float(disk_intensity))
        sp = _spheres_array(spheres if spheres is not None else [])
        rgb = np.ones((len(sp), 3)) if sphere_rgb is None else np.asarray(sphere_rgb, dtype=np.float64).reshape(-1, 3)
        lm = np.zeros((0, 4)) if lamps is None else np.asarray(lamps, dtype=np.float64).reshape(-1, 4)
        if len(sp) > MAX_SPHERES or len(lm) > 4 or len(rgb) != len(sp):
            raise ValueError("at most 8 spheres (one colour each) and 4 lamps")
        sc.n_spheres, sc.n_lamps = len(sp), len(lm)
        for j in range(len(sp)):
            for q in range(4):
                sc.spheres[j][q] = float(sp[j, q])
            for q in range(3):
                sc.sphere_rgb[j][q] = float(rgb[j, q])
        for j in range(len(lm)):
            for q in range(4):
                sc.lamps[j][q] = float(lm[j, q])
        _check(load().bhg_frame_set_scene(self._h, C.byref(sc)))

    def set_redshift(self, apply=("disk", "objects", "sky"), exponent=4.0, disk_sense=1):
        """Redshift in every later render (bhg_frame_set_redshift): the colour of a ray of a class in `apply` is weighted by
        g^exponent.  apply=() or None: off -- the frame as without redshift, bit for bit."""
        if apply is None or (not isinstance(apply, (int, np.integer)) and len(apply) == 0):
            _check(load().bhg_frame_set_redshift(self._h, None))
            return
        _check(load().bhg_frame_set_redshift(self._h, C.byref(make_redshift(apply, exponent, disk_sense))))

    def set_observer(self, velocity=None):
        """The observer camera in every later render (bhg_frame_set_observer): the rays are what an observer at the camera moving
        with velocity beta (3 numbers, world axes, relative to the ZAMO; observer.py has the common ones) sees.  None: the
        reference camera again, bit for bit."""
        _check(load().bhg_frame_set_observer(self._h, _obs_ref(make_observer(velocity))))

    def set_object_textures(self, textures=None, rotations=None, modes=None, emission=None):
        """Textured, oriented and emissive object spheres in every later render (bhg_frame_set_object_textures; DESIGN.md
        section 11), per sphere of the scene: textures [h, w, 4] float32 host arrays (None: keep that sphere's current
        texture, white if it never had one), 3x3 body -> world rotations (None: the identity), modes ("lit" / "emissive"),
        emission strengths.  Only new images are uploaded.  All None: textures off -- the frame as without them, bit for bit."""
        if textures is None and rotations is None and modes is None and emission is None:
            _check(load().bhg_frame_set_object_textures(self._h, None))
            return
        ot, keep = make_object_textures(textures, rotations, modes, emission)
        _check(load().bhg_frame_set_object_textures(self._h, C.byref(ot)))
        del keep

    def set_disk_thermal(self, th=None):
        """The thermal disk in every later render (bhg_frame_set_disk_thermal): th a DiskThermal
        (make_disk_thermal), or a dict of make_disk_thermal's arguments.  None: off -- the frame as without it, bit for bit."""
        if isinstance(th, dict):
            th = make_disk_thermal(**th)
        _check(load().bhg_frame_set_disk_thermal(self._h, None if th is None else C.byref(th)))

    def set_object_motion(self, velocity=None, angular_velocity=None):
        """Moving and spinning object spheres in every later render (bhg_frame_set_object_motion):
        velocity, angular_velocity [n][3] per sphere of the scene (make_object_motion; observer.circular_orbit_motion gives an
        orbit).  Both None: off -- the frame as without motion, bit for bit."""
        if velocity is None and angular_velocity is None:
            _check(load().bhg_frame_set_object_motion(self._h, None))
            return
        _check(load().bhg_frame_set_object_motion(self._h, C.byref(make_object_motion(velocity, angular_velocity))))

    def set_mesh_build(self, on):
        """The device build for the frame's meshes (bhg_frame_set_mesh_build), default off: each device
        builds its tree itself from the frame's host copy, a later set_mesh() that fits the held mesh's capacity rebuilds it in
        place, and refit_mesh()'s rebuild does too.  The images are the host-built frame's, bit for bit."""
        _check(load().bhg_frame_set_mesh_build(self._h, 1 if on else 0))

    def mesh_build_info(self, shard=0):
        """Mesh.build_info() of the mesh on the frame's device number `shard` (bhg_frame_mesh_build_info)"""
        dev, builds, cv, ct, allocs = C.c_int32(0), C.c_uint64(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        _check(load().bhg_frame_mesh_build_info(self._h, int(shard), C.byref(dev), C.byref(builds), C.byref(cv), C.byref(ct),
                                                C.byref(allocs)))
        return {"built_on_device": bool(dev.value), "builds": builds.value, "cap_vertices": cv.value, "cap_triangles": ct.value,
                "allocations": allocs.value}

    def set_mesh(self, vertices=None, triangles=None, vertex_normals=None, leaf_size=4, chord=None, material=None, build=None):
        """A triangle mesh in every later render (bhg_frame_set_mesh): vertices [nv, 3] float64, Cartesian
        and centred on the hole, triangles [nt, 3] int32, vertex_normals [nv, 3] or None (flat shading), chord the sub-chord
        length of the trace (None: a quarter of r_s at render time), material a MeshMaterial or None (white, no emission).
        Everything is copied.  Not with scene spheres, redshift, the thermal disk, object motion or object textures (refused
        at render).  set_mesh(None): off -- the frame as without a mesh, bit for bit.  build: "host" / "device" is
        set_mesh_build() first; None leaves the switch as it is."""
        if build not in (None, "host", "device"):
            raise ValueError('build must be None, "host" or "device"')
        if build is not None:
            self.set_mesh_build(build == "device")
        if vertices is None:
            _check(load().bhg_frame_set_mesh(self._h, None, 0, None, 0, None, 0, 0.0, None))
            self._mesh_nv = None
            return
        V, F = _mesh_arrays(vertices, triangles)
        N = None
        if vertex_normals is not None:
            N = np.ascontiguousarray(vertex_normals, dtype=np.float64)
            if N.shape != V.shape:
                raise ValueError("vertex_normals must have the shape of vertices")
        if chord is not None and not (np.isfinite(float(chord)) and float(chord) > 0.0):
            raise ValueError("chord must be finite and > 0")
        m = None
        if material is not None:
            material.check_triangles(F.shape[0])
            m = material.struct()
        _check(load().bhg_frame_set_mesh(self._h, _addr(V), V.shape[0], _addr(F), F.shape[0], None if N is None else _addr(N),
                                         int(leaf_size), 0.0 if chord is None else float(chord), None if m is None else C.byref(m)))
        self._mesh_nv = V.shape[0]

    def refit_mesh(self, vertices, vertex_normals=None, rebuild_ratio=None):
        """New vertex positions [nv, 3] (and vertex normals, for a mesh set with them) for the frame's mesh (bhg_frame_refit_mesh;
        DESIGN.md section 22): at the next render each device refits its tree on the device instead of building it anew --
        the image is the one set_mesh() with the deformed vertices gives, bit for bit; the material, the instances and their
        colours stay.  rebuild_ratio: a device whose tree's area sum has grown past this multiple of what it was when built
        rebuilds from the held triangles instead (None: MESH_REBUILD_RATIO; <= 0: never; 1: always)."""
        nv = getattr(self, "_mesh_nv", None)
        if nv is None:
            raise ValueError("refit_mesh() wants a mesh: set_mesh() first")
        V = np.ascontiguousarray(vertices, dtype=np.float64)
        N = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, dtype=np.float64)
        if V.shape != (nv, 3) or (N is not None and N.shape != (nv, 3)):
            raise ValueError(f"vertices (and vertex_normals) must have the mesh's shape [{nv}, 3]")
        ratio = MESH_REBUILD_RATIO if rebuild_ratio is None else float(rebuild_ratio)
        _check(load().bhg_frame_refit_mesh(self._h, _addr(V), None if N is None else _addr(N), ratio))

    def mesh_refit_info(self, shard=0):
        """(generation, area_build, area_now) of the mesh on the frame's device number `shard` (bhg_frame_mesh_refit_info): the
        refits since that device last built its tree, and the tree's area sum when built and now"""
        g, a, b = C.c_uint64(0), C.c_double(0.0), C.c_double(0.0)
        _check(load().bhg_frame_mesh_refit_info(self._h, int(shard), C.byref(g), C.byref(a), C.byref(b)))
        return g.value, a.value, b.value

    def prefix_info(self, shard=0):
        """(mode, used, rho) of the last render's trace call on the frame's device number `shard` (bhg_frame_prefix_info): what it
        asked of the rays' start-up records, what the library answered, the records' radius"""
        pf = Prefix(None, 0.0, PREFIX_NONE, PREFIX_NONE)
        _check(load().bhg_frame_prefix_info(self._h, int(shard), C.byref(pf)))
        return pf.mode, pf.used, pf.rho

    def set_mesh_instances(self, transforms=None, inst_rgb=None, tree=False, leaf_size=MESH_INSTANCE_TREE_LEAF):
        """Rigid placements of the frame's mesh in every later render (bhg_frame_set_mesh_instances):
        transforms [K, 12] (R row-major, then t) or [K, 3, 4] (R | t), inst_rgb [K, 3] float32 or None.  Calling it again with
        other transforms moves the instances: the records go to the devices, nothing of the mesh is rebuilt or uploaded.
        None (or no transforms): off -- the plain mesh render, bit for bit.  set_mesh() turns instances off as well.
        tree=True (bhg_frame_set_mesh_instance_tree): the devices' sets lie under trees of boxes with
        leaves of leaf_size, and K may go up to MESH_INSTANCE_TREE_MAX."""
        if transforms is None or len(transforms) == 0:
            _check(load().bhg_frame_set_mesh_instances(self._h, 0, None, None))
            return
        T = _instance_transforms(transforms)
        rgb = None
        if inst_rgb is not None:
            rgb = np.ascontiguousarray(inst_rgb, dtype=np.float32)
            if rgb.shape != (T.shape[0], 3):
                raise ValueError("inst_rgb must have shape [K, 3]")
        if tree:
            _check(load().bhg_frame_set_mesh_instance_tree(self._h, T.shape[0], _addr(T), None if rgb is None else _addr(rgb),
                                                           int(leaf_size)))
            return
        _check(load().bhg_frame_set_mesh_instances(self._h, T.shape[0], _addr(T), None if rgb is None else _addr(rgb)))

    def render(self, params: "Params", out=None, to_host=True):
        """One frame: float32 [H, W, 4] (a new array, or `out`).  to_host=False: only enqueue; the image stays on the
        first device (device_image(), synchronize())."""
        if not to_host:
            _check(load().bhg_frame_render(self._h, C.byref(params), None))
            return None
        if out is None:
            out = np.empty((self.H, self.W, 4), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == self.H * self.W * 4
        _check(load().bhg_frame_render(self._h, C.byref(params), C.c_void_p(out.ctypes.data)))
        return out

    def synchronize(self):
        _check(load().bhg_frame_synchronize(self._h))

    def device_image(self) -> int:
        return load().bhg_frame_device_image(self._h) or 0

    def rebalance(self, root_share=1.0):
        """Re-deal the tiles by the last render's measured cost; root_share < 1 gives the first device -- which also
        receives the gather and assembles the frame -- that part of an equal share."""
        _check(load().bhg_frame_rebalance(self._h, float(root_share)))

    def stats(self):
        out = (C.c_uint64 * 4)()
        _check(load().bhg_frame_stats(self._h, out))
        return {"rays": int(out[0]), "attempted_steps": int(out[1]), "accepted_steps": int(out[2]), "horizon_rays": int(out[3])}

    def info(self):
        out = (C.c_int64 * 8)()
        _check(load().bhg_frame_info(self._h, out))
        return {"n_devices": int(out[0]), "gather": {GATHER_COPY: "copy", GATHER_RCCL: "rccl", GATHER_PEER: "peer"}.get(int(out[1]), str(out[1])),
                "largest_shard_pixels": int(out[2]), "smallest_shard_pixels": int(out[3]), "tile": int(out[4]),
                "dealt_by_measured_cost": bool(out[5]), "renders": int(out[6]), "directions_only": bool(out[7])}

    def set_profiling(self, enable=True):
        _check(load().bhg_frame_set_profiling(self._h, 1 if enable else 0))

    def last_ms(self):
        """(trace kernel ms per listed device, root gather + assembly ms) of the last profiled render."""
        tr = (C.c_float * len(self.devices))()
        root = C.c_float()
        _check(load().bhg_frame_last_ms(self._h, tr, C.byref(root)))
        return [float(v) for v in tr], float(root.value)


class Context:
    """One bhg_context = one device + stream.  Not thread-safe; one call at a time."""

    def __init__(self, device: int = 0):
        L = load()
        h = C.c_void_p()
        _check(L.bhg_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.pinned = PinnedPool(ctx=self)
        self._meshes = []

    def close(self):
        if getattr(self, "_h", None):
            for m in list(getattr(self, "_meshes", ())):
                m.close()
            self.pinned.close()
            load().bhg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def name(self) -> str:
        buf = C.create_string_buffer(256)
        _check(load().bhg_device_name(self._h, buf, 256))
        return buf.value.decode()

    @property
    def num_cus(self) -> int:
        return load().bhg_num_cus(self._h)

    def last_launch(self):
        out = (C.c_int32 * 4)()
        _check(load().bhg_last_launch(self._h, out))
        return {"workgroups": out[0], "threads": out[1], "waves_per_cu": out[2], "passes": out[3]}

    @property
    def stream(self) -> int:
        """The context's own hipStream_t as an integer handle."""
        return load().bhg_context_stream(self._h) or 0

    def set_profiling(self, enable=True):
        _check(load().bhg_set_profiling(self._h, 1 if enable else 0))

    def last_pass_ms(self):
        """{prepare, trace, post} milliseconds of the last profiled trace call (waits for it); post = Kerr's finalize
        pass, 0 otherwise ("resolve" is the slot's round-1 name, kept as an alias)."""
        out = (C.c_float * 3)()
        _check(load().bhg_last_pass_ms(self._h, out))
        return {"prepare": out[0], "trace": out[1], "post": out[2], "resolve": out[2]}

    def synchronize(self):
        _check(load().bhg_synchronize(self._h))

    def peak_probe(self, kind=PROBE_FMA, target_ms=1.0):
        """bhg_peak_probe: the fp64 VALU rate THIS device sustains, in the trace kernels' launch geometry.  kind
        PROBE_FMA: nothing but v_fma_f64; PROBE_STEP_MIX: the DP5(4) step loop's mix (16 quarter-rate ops per 503)."""
        out = (C.c_double * 6)()
        _check(load().bhg_peak_probe(self._h, int(kind), float(target_ms), out))
        return {"tflops": out[0], "ms": out[1], "valu_wave_insts": out[2], "quarter_rate_wave_insts": out[3],
                "ms_fastest": out[4], "fp64_full_rate_clock_mhz": out[5]}

    def math_probe(self, op, values):
        """bhg_math_probe (a test hook): values [n] or [n, n_in] float64 through the device primitive `op` (MATH_*), one
        element per thread -> [n] or [n, n_out] float64."""
        if op not in MATH_PROBE_SHAPE:
            raise ValueError(f"unknown math probe op {op}")
        n_in, n_out = MATH_PROBE_SHAPE[op]
        v = np.ascontiguousarray(values, dtype=np.float64)
        if (n_in == 1 and v.ndim != 1) or (n_in > 1 and (v.ndim != 2 or v.shape[1] != n_in)):
            raise ValueError(f"values must have shape [n]" if n_in == 1 else f"values must have shape [n, {n_in}]")
        n = v.shape[0]
        out = np.empty((n,) if n_out == 1 else (n, n_out), np.float64)
        _check(load().bhg_math_probe(self._h, int(op), v.ctypes.data, n, out.ctypes.data))
        return out

    # -- host buffers -------------------------------------------------------------------
    def trace(self, k0, x0, params: Params, want_accepted=True, spheres=None, want_steps=True, pinned_results=True):
        """k0[N,3], x0[3] (shared) or [N,3] -> (end[N,6], flags[N] u8, n_steps[N] u32, n_accepted[N] u32);
        with spheres [[cx, cy, cz, radius], ...] a fifth array object_id[N] i8 is appended.  want_steps /
        want_accepted = False: that array is not brought back (None in its place).  The result arrays are
        page-locked (self.pinned, a pool) unless pinned_results=False."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64)
        if k0.ndim != 2 or k0.shape[1] != 3:
            raise ValueError("k0 must have shape [N, 3]")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        shared = x0.ndim == 1
        if shared:
            if x0.shape != (3,):
                raise ValueError("x0 must have shape [3] or [N, 3]")
        elif x0.shape != (n, 3):
            raise ValueError("x0 must have shape [3] or [N, 3]")
        new = self.pinned.empty if (pinned_results and n >= 65536) else (lambda shape, dt: np.empty(shape, dt))
        end = new((n, 6), np.float64)
        flags = new((n,), np.uint8)
        steps = new((n,), np.uint32) if want_steps else None
        acc = new((n,), np.uint32) if want_accepted else None
        p_steps = steps.ctypes.data_as(_u32p) if steps is not None else None
        p_acc = acc.ctypes.data_as(_u32p) if acc is not None else None
        if spheres is not None:
            sp = _spheres_array(spheres)
            obj = new((n,), np.int8)
            _check(load().bhg_trace_objects(self._h, C.byref(params), _np_dp(sp), len(sp), _np_dp(x0), 1 if shared else 0,
                                            _np_dp(k0), n, _np_dp(end), flags.ctypes.data_as(_u8p), p_steps, p_acc,
                                            obj.ctypes.data_as(C.POINTER(C.c_int8))))
            return end, flags, steps, acc, obj
        _check(load().bhg_trace(self._h, C.byref(params), _np_dp(x0), 1 if shared else 0, _np_dp(k0), n,
                                _np_dp(end), flags.ctypes.data_as(_u8p), p_steps, p_acc))
        return end, flags, steps, acc

    def trace_crossings(self, k0, x0, params: Params, max_crossings):
        """bhg_trace_crossings: the trace that carries every ray THROUGH the disk of params and records its crossings (DP5(4), null
        rays, no object spheres).  k0[N,3], x0[3] or [N,3] -> (end[N,6], flags[N], n_steps[N], n_accepted[N] -- those of the same
        trace with the disk off --, cross[K,N,6] the first K = max_crossings crossing records in order, NaN where a ray has
        none, n_cross[N] u8 every crossing counted)."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64)
        if k0.ndim != 2 or k0.shape[1] != 3:
            raise ValueError("k0 must have shape [N, 3]")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        if x0.shape != (3,) and x0.shape != (n, 3):
            raise ValueError("x0 must have shape [3] or [N, 3]")
        end = np.empty((n, 6), np.float64)
        flags = np.empty(n, np.uint8)
        steps = np.empty(n, np.uint32)
        acc = np.empty(n, np.uint32)
        cross = np.full((max(int(max_crossings), 0), n, 6), np.nan, np.float64)
        n_cross = np.zeros(n, np.uint8)
        _check(load().bhg_trace_crossings(self._h, C.byref(params), _addr(x0), 1 if x0.ndim == 1 else 0, _addr(k0), n,
                                          int(max_crossings), _addr(end), _addr(flags), _addr(steps), _addr(acc), _addr(cross),
                                          _addr(n_cross)))
        return end, flags, steps, acc, cross, n_cross

    def travel_time(self, k0, x0, params: Params, max_crossings=0):
        """bhg_travel_time: the crossings trace with the coordinate time along each ray.  k0[N,3], x0[3] or
        [N,3] -> (end, flags, n_steps, n_accepted, cross[K,N,6], n_cross[N] -- trace_crossings' --, t_end[N] the time to the ray's
        end (+inf: the ray ended in the hole), t_cross[K,N] the time of each stored crossing, NaN where a ray has none).
        max_crossings = 0 (the disk of params may then be off): no records, K = 0."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64)
        if k0.ndim != 2 or k0.shape[1] != 3:
            raise ValueError("k0 must have shape [N, 3]")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        if x0.shape != (3,) and x0.shape != (n, 3):
            raise ValueError("x0 must have shape [3] or [N, 3]")
        K = max(int(max_crossings), 0)
        end = np.empty((n, 6), np.float64)
        flags = np.empty(n, np.uint8)
        steps = np.empty(n, np.uint32)
        acc = np.empty(n, np.uint32)
        cross = np.full((K, n, 6), np.nan, np.float64)
        t_cross = np.full((K, n), np.nan, np.float64)
        n_cross = np.zeros(n, np.uint8)
        t_end = np.empty(n, np.float64)
        _check(load().bhg_travel_time(self._h, C.byref(params), _addr(x0), 1 if x0.ndim == 1 else 0, _addr(k0), n,
                                      int(max_crossings), _addr(end), _addr(flags), _addr(steps), _addr(acc),
                                      _addr(cross) if K else None, _addr(n_cross), _addr(t_end), _addr(t_cross) if K else None))
        return end, flags, steps, acc, cross, n_cross, t_end, t_cross

    def trace_mesh(self, k0, x0, params: Params, mesh: "Mesh", max_chord):
        """bhg_trace_mesh: the trace with a triangle mesh as one more terminal event.  k0[N,3], x0[3] or
        [N,3] -> (end[N,6], flags[N], n_steps[N], n_accepted[N], tri_id[N] int32 the triangle a ray ends on or -1, bary[N,2] the
        plane coordinates (u, v) of the hit in it, NaN for a ray that hits nothing)."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64)
        if k0.ndim != 2 or k0.shape[1] != 3:
            raise ValueError("k0 must have shape [N, 3]")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        if x0.shape != (3,) and x0.shape != (n, 3):
            raise ValueError("x0 must have shape [3] or [N, 3]")
        end = np.empty((n, 6), np.float64)
        flags = np.empty(n, np.uint8)
        steps = np.empty(n, np.uint32)
        acc = np.empty(n, np.uint32)
        tri_id = np.full(n, -1, np.int32)
        bary = np.full((n, 2), np.nan, np.float64)
        _check(load().bhg_trace_mesh(self._h, C.byref(params), None if mesh is None else mesh._h, float(max_chord), _addr(x0),
                                     1 if x0.ndim == 1 else 0, _addr(k0), n, _addr(end), _addr(flags), _addr(steps), _addr(acc),
                                     _addr(tri_id), _addr(bary)))
        return end, flags, steps, acc, tri_id, bary

    def trace_mesh_device(self, params: Params, mesh: "Mesh", max_chord, n, d_k0, d_end, d_tri_id, d_bary, x0_shared=None, d_x0=0,
                          d_flags=0, d_n_steps=0, d_n_accepted=0, stream=0):
        """bhg_trace_mesh_device: d_tri_id [n] int32 and d_bary [n, 2] float64 beside trace_device's outputs."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_trace_mesh_device(self._h, C.byref(params), None if mesh is None else mesh._h, float(max_chord), xs,
                                            C.c_void_p(d_x0 or None), C.c_void_p(d_k0 or None), int(n), C.c_void_p(d_end or None),
                                            C.c_void_p(d_flags or None), C.c_void_p(d_n_steps or None),
                                            C.c_void_p(d_n_accepted or None), C.c_void_p(d_tri_id or None),
                                            C.c_void_p(d_bary or None), C.c_void_p(stream or None)))

    def trace_mesh_instances(self, k0, x0, params: Params, instances: "MeshInstances", max_chord):
        """bhg_trace_mesh_instances: trace_mesh over the rigid placements of an instance set ->
        (end[N,6], flags[N], n_steps[N], n_accepted[N], tri_id[N] the triangle within the mesh or -1, inst_id[N] int32 the instance
        or -1, bary[N,2] the plane coordinates in the instance's frame, NaN for a ray that hits nothing)."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64)
        if k0.ndim != 2 or k0.shape[1] != 3:
            raise ValueError("k0 must have shape [N, 3]")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        if x0.shape != (3,) and x0.shape != (n, 3):
            raise ValueError("x0 must have shape [3] or [N, 3]")
        end = np.empty((n, 6), np.float64)
        flags = np.empty(n, np.uint8)
        steps = np.empty(n, np.uint32)
        acc = np.empty(n, np.uint32)
        tri_id = np.full(n, -1, np.int32)
        inst_id = np.full(n, -1, np.int32)
        bary = np.full((n, 2), np.nan, np.float64)
        _check(load().bhg_trace_mesh_instances(self._h, C.byref(params), None if instances is None else instances._h,
                                               float(max_chord), _addr(x0), 1 if x0.ndim == 1 else 0, _addr(k0), n, _addr(end),
                                               _addr(flags), _addr(steps), _addr(acc), _addr(tri_id), _addr(inst_id), _addr(bary)))
        return end, flags, steps, acc, tri_id, inst_id, bary

    def trace_mesh_instances_device(self, params: Params, instances: "MeshInstances", max_chord, n, d_k0, d_end, d_tri_id, d_inst_id,
                                    d_bary, x0_shared=None, d_x0=0, d_flags=0, d_n_steps=0, d_n_accepted=0, stream=0):
        """bhg_trace_mesh_instances_device: trace_mesh_device with an instance set in place of the mesh, plus d_inst_id [n] int32."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_trace_mesh_instances_device(self._h, C.byref(params), None if instances is None else instances._h,
                                                      float(max_chord), xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0 or None),
                                                      int(n), C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                                      C.c_void_p(d_n_steps or None), C.c_void_p(d_n_accepted or None),
                                                      C.c_void_p(d_tri_id or None), C.c_void_p(d_inst_id or None),
                                                      C.c_void_p(d_bary or None), C.c_void_p(stream or None)))

    def shade_mesh_device(self, d_end, d_flags, d_tri_id, d_bary, n_pixels, samples, scene: "Scene", mesh: "Mesh", d_tri_rgb=0,
                          d_rgba=0, d_rgba_f32=0, d_scatter=0, stream=0):
        """bhg_shade_mesh_device: the shade of a mesh trace -- mesh rays Lambert-lit and shadowed by the mesh, every other ray
        shade_scene_device's.  d_tri_rgb [nt, 3] float32 or 0 (white)."""
        _check(load().bhg_shade_mesh_device(self._h, C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                            C.c_void_p(d_tri_id or None), C.c_void_p(d_bary or None), int(n_pixels), int(samples),
                                            C.byref(scene), None if mesh is None else mesh._h, C.c_void_p(d_tri_rgb or None),
                                            C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None),
                                            C.c_void_p(d_scatter or None), C.c_void_p(stream or None)))

    def shade_mesh_instances_device(self, d_end, d_flags, d_tri_id, d_inst_id, d_bary, n_pixels, samples, scene: "Scene",
                                    instances: "MeshInstances", material=None, d_inst_rgb=0, d_rgba=0, d_rgba_f32=0, d_scatter=0,
                                    stream=0):
        """bhg_shade_mesh_instances_device: shade_mesh_material_device over an instance set -- mesh rays get
        albedo * inst_rgb[inst] * (lamp_sum + emission).  material a MeshMaterialStruct of DEVICE addresses or None (white),
        d_inst_rgb [K, 3] float32 or 0."""
        _check(load().bhg_shade_mesh_instances_device(self._h, C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                                      C.c_void_p(d_tri_id or None), C.c_void_p(d_inst_id or None),
                                                      C.c_void_p(d_bary or None), int(n_pixels), int(samples), C.byref(scene),
                                                      None if instances is None else instances._h,
                                                      None if material is None else C.byref(material),
                                                      C.c_void_p(d_inst_rgb or None), C.c_void_p(d_rgba or None),
                                                      C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
                                                      C.c_void_p(stream or None)))

    def shade_mesh_material_device(self, d_end, d_flags, d_tri_id, d_bary, n_pixels, samples, scene: "Scene", mesh: "Mesh", material,
                                   d_rgba=0, d_rgba_f32=0, d_scatter=0, stream=0):
        """bhg_shade_mesh_material_device: shade_mesh_device with a material (a MeshMaterialStruct of DEVICE addresses) in place of
        d_tri_rgb -- mesh rays get tri_rgb * texel * (lamp_sum + emission)."""
        _check(load().bhg_shade_mesh_material_device(self._h, C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                                     C.c_void_p(d_tri_id or None), C.c_void_p(d_bary or None), n_pixels, samples,
                                                     C.byref(scene), None if mesh is None else mesh._h,
                                                     None if material is None else C.byref(material), C.c_void_p(d_rgba or None),
                                                     C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
                                                     C.c_void_p(stream or None)))

    def trajectory(self, k0, x0, params: Params, n_points, spheres=None):
        """Sampled curves: (traj[N,6,T], n_valid[N], end[N,6], flags[N]); with spheres= (object spheres in the curved region,
        [[cx, cy, cz, radius], ...] BH-centred): (..., object_id[N]) -- bhg_trajectory_objects."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        n = k0.shape[0]
        shared = x0.ndim == 1
        # small calls (the engine's literal one ray x 10,000 samples): a page-locked sample array from the context's pool -- the
        # kernel then writes the samples straight into it (no device-to-host copy, no host-side split; include/bhgeo.h)
        small = n <= 2048 and n * 6 * int(n_points) * 8 <= (4 << 20)
        traj = (self.pinned.empty if small else np.empty)((n, 6, int(n_points)), np.float64)
        nv = np.empty(n, np.uint32)
        end = np.empty((n, 6), np.float64)
        flags = np.empty(n, np.uint8)
        if spheres is not None:
            sp = _spheres_array(spheres)
            obj = np.empty(n, np.int8)
            _check(load().bhg_trajectory_objects(self._h, C.byref(params), _addr(sp) if len(sp) else None, len(sp), _addr(x0),
                                                 1 if shared else 0, _addr(k0), n, int(n_points), _addr(traj), _addr(nv), _addr(end),
                                                 _addr(flags), _addr(obj)))
            return traj, nv, end, flags, obj
        _check(load().bhg_trajectory(self._h, C.byref(params), _addr(x0), 1 if shared else 0, _addr(k0), n,
                                     int(n_points), _addr(traj), _addr(nv), _addr(end), _addr(flags)))
        return traj, nv, end, flags

    # -- device buffers (raw addresses, e.g. torch.Tensor.data_ptr()) -------------------
    def _trace_start_device(self, params, n, d_k0, d_end, d_end_dir, xs, d_x0, d_flags, d_n_steps, d_n_accepted, stream, spheres,
                            d_object_id, d_start_steps, start_mode, prefix=None):
        """bhg_trace_start_device: the three device trace calls in one, with the rays' initial steps recorded into or
        replayed from d_start_steps [n] float64 (start_mode START_RECORD / START_REPLAY; include/bhgeo.h has the rules).
        prefix: a Prefix -- bhg_trace_prefix_device, the same call with the rays' start-up records; its rho / used are filled."""
        sp = None if spheres is None else _spheres_array(spheres)
        if prefix is not None:
            _check(load().bhg_trace_prefix_device(self._h, C.byref(params), None if sp is None else _np_dp(sp),
                                                  0 if sp is None else len(sp), xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0), int(n),
                                                  C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags or None),
                                                  C.c_void_p(d_n_steps or None), C.c_void_p(d_n_accepted or None),
                                                  C.c_void_p(d_object_id or None), C.c_void_p(d_start_steps or None), int(start_mode),
                                                  C.byref(prefix), C.c_void_p(stream or None)))
            return
        _check(load().bhg_trace_start_device(self._h, C.byref(params), None if sp is None else _np_dp(sp), 0 if sp is None else len(sp),
                                             xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0), int(n), C.c_void_p(d_end or None),
                                             C.c_void_p(d_end_dir or None), C.c_void_p(d_flags or None),
                                             C.c_void_p(d_n_steps or None), C.c_void_p(d_n_accepted or None),
                                             C.c_void_p(d_object_id or None), C.c_void_p(d_start_steps or None), int(start_mode),
                                             C.c_void_p(stream or None)))

    def trace_device(self, params: Params, n, d_k0, d_end, x0_shared=None, d_x0=0, d_flags=0,
                     d_n_steps=0, d_n_accepted=0, stream=0, spheres=None, d_object_id=0, d_start_steps=0, start_mode=START_NONE,
                     prefix=None):
        """d_start_steps, start_mode, prefix: see _trace_start_device; without them the plain calls of always."""
        xs = None
        if x0_shared is not None:
            xs = (C.c_double * 3)(*[float(v) for v in x0_shared])
        if start_mode != START_NONE or prefix is not None:
            return self._trace_start_device(params, n, d_k0, d_end, 0, xs, d_x0, d_flags, d_n_steps, d_n_accepted, stream, spheres,
                                            d_object_id, d_start_steps, start_mode, prefix)
        if spheres is not None:
            sp = _spheres_array(spheres)
            _check(load().bhg_trace_objects_device(self._h, C.byref(params), _np_dp(sp), len(sp), xs,
                                                   C.c_void_p(d_x0 or None), C.c_void_p(d_k0), int(n), C.c_void_p(d_end),
                                                   C.c_void_p(d_flags or None), C.c_void_p(d_n_steps or None),
                                                   C.c_void_p(d_n_accepted or None), C.c_void_p(d_object_id or None),
                                                   C.c_void_p(stream or None)))
            return
        _check(load().bhg_trace_device(self._h, C.byref(params), xs, C.c_void_p(d_x0 or None),
                                       C.c_void_p(d_k0), int(n), C.c_void_p(d_end),
                                       C.c_void_p(d_flags or None), C.c_void_p(d_n_steps or None),
                                       C.c_void_p(d_n_accepted or None), C.c_void_p(stream or None)))

    def trace_crossings_device(self, params: Params, n, d_k0, max_crossings, d_end, d_cross, d_n_cross, x0_shared=None, d_x0=0,
                               d_flags=0, d_n_steps=0, d_n_accepted=0, stream=0):
        """bhg_trace_crossings_device: d_cross [max_crossings, n, 6] float64 and d_n_cross [n] uint8 beside trace_device's
        outputs, which are those of the trace with the disk off."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_trace_crossings_device(self._h, C.byref(params), xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0 or None),
                                                 int(n), int(max_crossings), C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                                 C.c_void_p(d_n_steps or None), C.c_void_p(d_n_accepted or None),
                                                 C.c_void_p(d_cross or None), C.c_void_p(d_n_cross or None),
                                                 C.c_void_p(stream or None)))

    def travel_time_device(self, params: Params, n, d_k0, max_crossings, d_end, d_t_end, d_cross=0, d_n_cross=0, d_t_cross=0,
                           x0_shared=None, d_x0=0, d_flags=0, d_n_steps=0, d_n_accepted=0, stream=0):
        """bhg_travel_time_device: trace_crossings_device plus d_t_end [n] float64 and d_t_cross [max_crossings, n] float64.
        max_crossings = 0: d_cross, d_n_cross, d_t_cross may be 0."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_travel_time_device(self._h, C.byref(params), xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0 or None),
                                             int(n), int(max_crossings), C.c_void_p(d_end or None), C.c_void_p(d_flags or None),
                                             C.c_void_p(d_n_steps or None), C.c_void_p(d_n_accepted or None),
                                             C.c_void_p(d_cross or None), C.c_void_p(d_n_cross or None),
                                             C.c_void_p(d_t_end or None), C.c_void_p(d_t_cross or None), C.c_void_p(stream or None)))

    def shade_disk_layers_retarded_device(self, d_end, d_flags, d_cross, d_n_cross, d_t_cross, phase_rate, n_pixels, samples,
                                          scene: "Scene", layers: "DiskLayers", params=None, rs=None, obs=None, th=None,
                                          x0_shared=None, d_k0=0, d_rgba=0, d_rgba_f32=0, d_scatter=0, d_end_dir=0, stream=0):
        """bhg_shade_disk_layers_retarded_device: shade_disk_layers_device with layer m of ray i drawn at the phase
        disk_phase - phase_rate * t_cross[m][i] (d_t_cross [max_crossings, S * n_pixels] float64 of travel_time_device)."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_shade_disk_layers_retarded_device(
            self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags or None),
            C.c_void_p(d_cross or None), C.c_void_p(d_n_cross or None), int(n_pixels), int(samples), C.byref(scene),
            None if params is None else C.byref(params), None if rs is None else C.byref(rs), _obs_ref(obs), xs,
            C.c_void_p(d_k0 or None), C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
            None if th is None else C.byref(th), None if layers is None else C.byref(layers), C.c_void_p(d_t_cross or None),
            float(phase_rate), C.c_void_p(stream or None)))

    def shade_disk_layers_device(self, d_end, d_flags, d_cross, d_n_cross, n_pixels, samples, scene: "Scene", layers: "DiskLayers",
                                 params=None, rs=None, obs=None, th=None, x0_shared=None, d_k0=0, d_rgba=0, d_rgba_f32=0,
                                 d_scatter=0, d_end_dir=0, stream=0):
        """bhg_shade_disk_layers_device: the layered shade of a crossings trace -- the optically thin disk (layers: DiskLayers);
        rs / obs / th as in shade_scene_thermal_device, None = off."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_shade_disk_layers_device(
            self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags or None),
            C.c_void_p(d_cross or None), C.c_void_p(d_n_cross or None), int(n_pixels), int(samples), C.byref(scene),
            None if params is None else C.byref(params), None if rs is None else C.byref(rs), _obs_ref(obs), xs,
            C.c_void_p(d_k0 or None), C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
            None if th is None else C.byref(th), None if layers is None else C.byref(layers), C.c_void_p(stream or None)))

    def trace_dir_device(self, params: Params, n, d_k0, d_end_dir, x0_shared=None, d_x0=0, d_flags=0,
                         d_n_steps=0, d_n_accepted=0, stream=0, d_start_steps=0, start_mode=START_NONE, prefix=None):
        """bhg_trace_dir_device: like trace_device, but only the direction half of the end states is written
        (d_end_dir [n][3]) -- what a sky frame consumes."""
        xs = None
        if x0_shared is not None:
            xs = (C.c_double * 3)(*[float(v) for v in x0_shared])
        if start_mode != START_NONE or prefix is not None:
            if not d_end_dir:
                raise ValueError("end_dir is NULL")
            return self._trace_start_device(params, n, d_k0, 0, d_end_dir, xs, d_x0, d_flags, d_n_steps, d_n_accepted, stream, None,
                                            0, d_start_steps, start_mode, prefix)
        _check(load().bhg_trace_dir_device(self._h, C.byref(params), xs, C.c_void_p(d_x0 or None),
                                           C.c_void_p(d_k0), int(n), C.c_void_p(d_end_dir),
                                           C.c_void_p(d_flags or None), C.c_void_p(d_n_steps or None),
                                           C.c_void_p(d_n_accepted or None), C.c_void_p(stream or None)))

    def shade_dir_device(self, d_end_dir, d_flags, n_pixels, samples, d_sky, sky_w, sky_h, d_rgba=0, d_rgba_f32=0,
                         d_scatter=0, stream=0):
        _check(load().bhg_shade_dir_device(self._h, C.c_void_p(d_end_dir), C.c_void_p(d_flags), int(n_pixels),
                                           int(samples), C.c_void_p(d_sky), int(sky_w), int(sky_h),
                                           C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None),
                                           C.c_void_p(d_scatter or None), C.c_void_p(stream or None)))

    def raygen_device(self, width, height, samples, fov_x, fov_y, d_jitter, d_k0, n_pixels, d_pixels=0,
                      rot=None, stream=0):
        r9 = None
        if rot is not None:
            r9 = (C.c_double * 9)(*[float(v) for v in np.asarray(rot, dtype=np.float64).reshape(9)])
        _check(load().bhg_raygen_device(self._h, int(width), int(height), int(samples), float(fov_x), float(fov_y),
                                        r9, C.c_void_p(d_jitter), C.c_void_p(d_pixels or None), int(n_pixels),
                                        C.c_void_p(d_k0), C.c_void_p(stream or None)))

    def raygen_observer_device(self, params: Params, obs, x0, width, height, samples, fov_x, fov_y, d_jitter, d_k0, n_pixels,
                               d_pixels=0, rot=None, stream=0):
        """bhg_raygen_observer_device: the camera rays of an observer (Observer, or None = bhg_raygen_device) at x0 [3]."""
        r9 = None
        if rot is not None:
            r9 = (C.c_double * 9)(*[float(v) for v in np.asarray(rot, dtype=np.float64).reshape(9)])
        xs = (C.c_double * 3)(*[float(v) for v in x0])
        _check(load().bhg_raygen_observer_device(self._h, C.byref(params), _obs_ref(obs), xs, int(width), int(height), int(samples),
                                                 float(fov_x), float(fov_y), r9, C.c_void_p(d_jitter),
                                                 C.c_void_p(d_pixels or None), int(n_pixels), C.c_void_p(d_k0),
                                                 C.c_void_p(stream or None)))

    def shade_device(self, d_end, d_flags, n_pixels, samples, d_sky, sky_w, sky_h, d_rgba, stream=0):
        _check(load().bhg_shade_device(self._h, C.c_void_p(d_end), C.c_void_p(d_flags), int(n_pixels), int(samples),
                                       C.c_void_p(d_sky), int(sky_w), int(sky_h), C.c_void_p(d_rgba),
                                       C.c_void_p(stream or None)))

    def shade_scene_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", d_rgba, d_object_id=0, stream=0):
        _check(load().bhg_shade_scene_device(self._h, C.c_void_p(d_end), C.c_void_p(d_flags),
                                             C.c_void_p(d_object_id or None), int(n_pixels), int(samples),
                                             C.byref(scene), C.c_void_p(d_rgba), C.c_void_p(stream or None)))

    def shade_scene_f32_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", d_rgba_f32, d_object_id=0,
                               d_scatter=0, stream=0):
        _check(load().bhg_shade_scene_f32_device(self._h, C.c_void_p(d_end), C.c_void_p(d_flags),
                                                 C.c_void_p(d_object_id or None), int(n_pixels), int(samples),
                                                 C.byref(scene), C.c_void_p(d_rgba_f32), C.c_void_p(d_scatter or None),
                                                 C.c_void_p(stream or None)))

    @staticmethod
    def _redshift_host(call, k0, x0, flags, end):
        """Marshalling of bhg_redshift_host / bhg_redshift_observer_host: call takes their arguments from x0 on."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        n = k0.shape[0]
        if flags.shape != (n,) or (x0.shape != (3,) and x0.shape != (n, 3)):
            raise ValueError("flags must be [N], x0 [3] or [N, 3]")
        e = None if end is None else np.ascontiguousarray(end, dtype=np.float64)
        if e is not None and e.shape != (n, 6):
            raise ValueError("end must be [N, 6]")
        g = np.empty(n, np.float64)
        _check(call(_addr(x0), 1 if x0.ndim == 1 else 0, _addr(k0), None if e is None else _addr(e), _addr(flags), n, _addr(g)))
        return g

    def redshift(self, k0, x0, params: Params, rs: Redshift, flags, end=None):
        """bhg_redshift_host: g [N] of traced rays from their camera state (k0 [N, 3], x0 [3] or [N, 3]), end [N, 6] (or None) and
        flags [N]."""
        return self._redshift_host(functools.partial(load().bhg_redshift_host, self._h, C.byref(params), C.byref(rs)), k0, x0, flags,
                                   end)

    def redshift_observer(self, k0, x0, params: Params, rs: Redshift, obs, flags, end=None):
        """bhg_redshift_observer_host: redshift() with g of the moving observer obs (Observer, or None = the ZAMO)."""
        return self._redshift_host(functools.partial(load().bhg_redshift_observer_host, self._h, C.byref(params), C.byref(rs),
                                                     _obs_ref(obs)), k0, x0, flags, end)

    @staticmethod
    def _spheres_arg(spheres):
        """(spheres [n][4] as a contiguous array or None, n) for the motion calls."""
        if spheres is None:
            return None, 0
        sp = np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)
        return sp, sp.shape[0]

    def redshift_motion(self, k0, x0, params: Params, rs: Redshift, obs, motion, spheres, flags, end=None, object_id=None):
        """bhg_redshift_motion_host: redshift_observer() with moving object spheres (motion: ObjectMotion, or None = at rest;
        spheres [n][4] of the trace; object_id [N] of the trace)."""
        sp, n_sp = self._spheres_arg(spheres)
        oid = None if object_id is None else np.ascontiguousarray(object_id, dtype=np.int8).reshape(-1)
        k0 = np.ascontiguousarray(k0, dtype=np.float64).reshape(-1, 3)
        if oid is not None and oid.shape != (k0.shape[0],):
            raise ValueError("object_id must be [N]")
        call = load().bhg_redshift_motion_host

        def fn(x0p, shared, k0p, ep, fp, n, gp):
            return call(self._h, C.byref(params), C.byref(rs), _obs_ref(obs), None if motion is None else C.byref(motion),
                        None if sp is None else _addr(sp), n_sp, x0p, shared, k0p, ep, fp, None if oid is None else _addr(oid), n, gp)
        return self._redshift_host(fn, k0, x0, flags, end)

    def redshift_motion_device(self, params: Params, rs: Redshift, obs, motion, spheres, n, d_k0, d_flags, d_g, x0_shared=None,
                               d_x0=0, d_end=0, d_object_id=0, stream=0):
        """bhg_redshift_motion_device on device arrays (spheres: HOST [n][4])."""
        sp, n_sp = self._spheres_arg(spheres)
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_redshift_motion_device(self._h, C.byref(params), C.byref(rs), _obs_ref(obs),
                                                 None if motion is None else C.byref(motion), None if sp is None else _addr(sp), n_sp,
                                                 xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0), C.c_void_p(d_end or None),
                                                 C.c_void_p(d_flags), C.c_void_p(d_object_id or None), int(n), C.c_void_p(d_g),
                                                 C.c_void_p(stream or None)))

    def shade_scene_moving_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params, rs, obs, ot, pol, d_qu, th, mo,
                                  x0_shared=None, d_k0=0, d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0,
                                  stream=0):
        """bhg_shade_scene_moving_device: shade_scene_thermal_device with moving object spheres (mo: ObjectMotion, or None =
        exactly the thermal call)."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_shade_scene_moving_device(
            self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags), C.c_void_p(d_object_id or None),
            int(n_pixels), int(samples), C.byref(scene), None if params is None else C.byref(params),
            None if rs is None else C.byref(rs), _obs_ref(obs), None if ot is None else C.byref(ot), xs, C.c_void_p(d_k0 or None),
            C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
            None if pol is None else C.byref(pol), C.c_void_p(d_qu or None), None if th is None else C.byref(th),
            None if mo is None else C.byref(mo), C.c_void_p(stream or None)))

    @staticmethod
    def _redshift_device(call, n, d_k0, d_flags, d_g, x0_shared, d_x0, d_end, stream):
        """Marshalling of bhg_redshift_device / bhg_redshift_observer_device: call takes their arguments from x0_shared on."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(call(xs, C.c_void_p(d_x0 or None), C.c_void_p(d_k0), C.c_void_p(d_end or None), C.c_void_p(d_flags), int(n),
                    C.c_void_p(d_g), C.c_void_p(stream or None)))

    def redshift_observer_device(self, params: Params, rs: Redshift, obs, n, d_k0, d_flags, d_g, x0_shared=None, d_x0=0, d_end=0,
                                 stream=0):
        self._redshift_device(functools.partial(load().bhg_redshift_observer_device, self._h, C.byref(params), C.byref(rs),
                                                _obs_ref(obs)), n, d_k0, d_flags, d_g, x0_shared, d_x0, d_end, stream)

    def redshift_device(self, params: Params, rs: Redshift, n, d_k0, d_flags, d_g, x0_shared=None, d_x0=0, d_end=0, stream=0):
        self._redshift_device(functools.partial(load().bhg_redshift_device, self._h, C.byref(params), C.byref(rs)), n, d_k0, d_flags,
                              d_g, x0_shared, d_x0, d_end, stream)

    def _shade_scene(self, fn, extra, d_end, d_end_dir, d_flags, d_object_id, n_pixels, samples, scene, params, rs, x0_shared, d_k0,
                     d_rgba, d_rgba_f32, d_scatter, stream):
        """Marshalling of the redshift, observer and textured shade calls: fn's arguments are bhg_shade_scene_redshift_device's
        with `extra` (obs, then ot) after rs."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(fn(self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags), C.c_void_p(d_object_id or None),
                  int(n_pixels), int(samples), C.byref(scene), None if params is None else C.byref(params),
                  None if rs is None else C.byref(rs), *extra, xs, C.c_void_p(d_k0 or None), C.c_void_p(d_rgba or None),
                  C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None), C.c_void_p(stream or None)))

    def shade_scene_redshift_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params: Params, rs, x0_shared, d_k0,
                                    d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0, stream=0):
        """bhg_shade_scene_redshift_device: the scene shade with each ray's colour weighted by g^exponent (rs: Redshift or None =
        off).  d_end = 0 with d_end_dir: a direction-only sky frame."""
        self._shade_scene(load().bhg_shade_scene_redshift_device, (), d_end, d_end_dir, d_flags, d_object_id, n_pixels, samples, scene,
                          params, rs, x0_shared, d_k0, d_rgba, d_rgba_f32, d_scatter, stream)

    def shade_scene_redshift_observer_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params: Params, rs, obs,
                                             x0_shared, d_k0, d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0,
                                             stream=0):
        """bhg_shade_scene_redshift_observer_device: shade_scene_redshift_device with g of the observer obs (None: the ZAMO)."""
        self._shade_scene(load().bhg_shade_scene_redshift_observer_device, (_obs_ref(obs),), d_end, d_end_dir, d_flags, d_object_id,
                          n_pixels, samples, scene, params, rs, x0_shared, d_k0, d_rgba, d_rgba_f32, d_scatter, stream)

    def shade_scene_textured_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params, rs, obs, ot, x0_shared=None,
                                    d_k0=0, d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0, stream=0):
        """bhg_shade_scene_textured_device, the general shade call: shade_scene_redshift_observer_device with object textures ot
        (ObjectTextures whose tex are device addresses, or None = without textures).  rs / obs / params may be None when redshift
        is off."""
        self._shade_scene(load().bhg_shade_scene_textured_device, (_obs_ref(obs), None if ot is None else C.byref(ot)), d_end,
                          d_end_dir, d_flags, d_object_id, n_pixels, samples, scene, params, rs, x0_shared, d_k0, d_rgba, d_rgba_f32,
                          d_scatter, stream)

    def shade_scene_polarised_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params, rs, obs, ot, pol, d_qu,
                                     x0_shared=None, d_k0=0, d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0,
                                     stream=0):
        """bhg_shade_scene_polarised_device: shade_scene_textured_device with the Stokes images d_qu [n_pixels, 6] fp64 (pol:
        Polarisation, or None = exactly the textured call)."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_shade_scene_polarised_device(
            self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags), C.c_void_p(d_object_id or None),
            int(n_pixels), int(samples), C.byref(scene), None if params is None else C.byref(params),
            None if rs is None else C.byref(rs), _obs_ref(obs), None if ot is None else C.byref(ot), xs, C.c_void_p(d_k0 or None),
            C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
            None if pol is None else C.byref(pol), C.c_void_p(d_qu or None), C.c_void_p(stream or None)))

    def shade_scene_thermal_device(self, d_end, d_flags, n_pixels, samples, scene: "Scene", params, rs, obs, ot, pol, d_qu, th,
                                   x0_shared=None, d_k0=0, d_rgba=0, d_rgba_f32=0, d_object_id=0, d_scatter=0, d_end_dir=0,
                                   stream=0):
        """bhg_shade_scene_thermal_device: shade_scene_polarised_device with the thermal disk (th: DiskThermal, or None =
        exactly the polarised call)."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_shade_scene_thermal_device(
            self._h, C.c_void_p(d_end or None), C.c_void_p(d_end_dir or None), C.c_void_p(d_flags), C.c_void_p(d_object_id or None),
            int(n_pixels), int(samples), C.byref(scene), None if params is None else C.byref(params),
            None if rs is None else C.byref(rs), _obs_ref(obs), None if ot is None else C.byref(ot), xs, C.c_void_p(d_k0 or None),
            C.c_void_p(d_rgba or None), C.c_void_p(d_rgba_f32 or None), C.c_void_p(d_scatter or None),
            None if pol is None else C.byref(pol), C.c_void_p(d_qu or None), None if th is None else C.byref(th),
            C.c_void_p(stream or None)))

    def disk_thermal(self, k0, x0, params: Params, th: DiskThermal, obs, flags, end=None):
        """bhg_disk_thermal_host: (t_em [N], rgb [N, 3]) of traced rays from their camera state (k0 [N, 3], x0 [3] or [N, 3]),
        end [N, 6] (or None) and flags [N]; obs: Observer or None (the ZAMO's g)."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        n = k0.shape[0]
        if flags.shape != (n,) or (x0.shape != (3,) and x0.shape != (n, 3)):
            raise ValueError("flags must be [N], x0 [3] or [N, 3]")
        e = None if end is None else np.ascontiguousarray(end, dtype=np.float64)
        if e is not None and e.shape != (n, 6):
            raise ValueError("end must be [N, 6]")
        t_em = np.empty(n, np.float64)
        rgb = np.empty((n, 3), np.float64)
        _check(load().bhg_disk_thermal_host(self._h, C.byref(params), C.byref(th), _obs_ref(obs), _addr(x0), 1 if x0.ndim == 1 else 0,
                                            _addr(k0), None if e is None else _addr(e), _addr(flags), n, _addr(t_em), _addr(rgb)))
        return t_em, rgb

    def disk_thermal_device(self, params: Params, th: DiskThermal, obs, n, d_k0, d_flags, d_t_em, d_rgb, x0_shared=None, d_x0=0,
                            d_end=0, stream=0):
        """bhg_disk_thermal_device on device arrays (d_rgb [n, 3])."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_disk_thermal_device(self._h, C.byref(params), C.byref(th), _obs_ref(obs), xs, C.c_void_p(d_x0 or None),
                                              C.c_void_p(d_k0), C.c_void_p(d_end or None), C.c_void_p(d_flags), int(n),
                                              C.c_void_p(d_t_em), C.c_void_p(d_rgb), C.c_void_p(stream or None)))

    def polarisation(self, k0, x0, params: Params, pol: Polarisation, obs, flags, end=None):
        """bhg_polarisation_host: (evpa, degree, mu) [N] of traced rays from their camera state (k0 [N, 3], x0 [3] or [N, 3]), end
        [N, 6] (or None) and flags [N]; obs: Observer or None (the ZAMO's screen)."""
        k0 = np.ascontiguousarray(k0, dtype=np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        n = k0.shape[0]
        if flags.shape != (n,) or (x0.shape != (3,) and x0.shape != (n, 3)):
            raise ValueError("flags must be [N], x0 [3] or [N, 3]")
        e = None if end is None else np.ascontiguousarray(end, dtype=np.float64)
        if e is not None and e.shape != (n, 6):
            raise ValueError("end must be [N, 6]")
        out = np.empty((3, n), np.float64)
        _check(load().bhg_polarisation_host(self._h, C.byref(params), C.byref(pol), _obs_ref(obs), _addr(x0), 1 if x0.ndim == 1 else 0,
                                            _addr(k0), None if e is None else _addr(e), _addr(flags), n, _addr(out[0]),
                                            _addr(out[1]), _addr(out[2])))
        return out[0], out[1], out[2]

    def polarisation_device(self, params: Params, pol: Polarisation, obs, n, d_k0, d_flags, d_evpa, d_degree, d_mu=0,
                            x0_shared=None, d_x0=0, d_end=0, stream=0):
        """bhg_polarisation_device on device arrays (d_mu may be 0)."""
        xs = None if x0_shared is None else (C.c_double * 3)(*[float(v) for v in x0_shared])
        _check(load().bhg_polarisation_device(self._h, C.byref(params), C.byref(pol), _obs_ref(obs), xs, C.c_void_p(d_x0 or None),
                                              C.c_void_p(d_k0), C.c_void_p(d_end or None), C.c_void_p(d_flags), int(n),
                                              C.c_void_p(d_evpa), C.c_void_p(d_degree), C.c_void_p(d_mu or None),
                                              C.c_void_p(stream or None)))

    def assemble_frame_f32_device(self, d_slabs, d_index, n_pixels, d_frame, stream=0):
        _check(load().bhg_assemble_frame_f32_device(self._h, C.c_void_p(d_slabs), C.c_void_p(d_index), int(n_pixels),
                                                    C.c_void_p(d_frame), C.c_void_p(stream or None)))

    def acceleration(self, x, k, params: Params):
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        k = np.ascontiguousarray(np.atleast_2d(k), dtype=np.float64)
        a = np.empty_like(x)
        _check(load().bhg_acceleration(self._h, C.byref(params), _np_dp(x), _np_dp(k), x.shape[0], _np_dp(a)))
        return a

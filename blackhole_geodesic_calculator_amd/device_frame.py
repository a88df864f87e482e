"""Device-resident frame pipeline: jitter stream -> rays -> geodesics -> shaded, sample-averaged
pixels, without a host round trip in between.

Covers, on the GPU, the reference's ray generation (raytracer/RelativisticRenderEngine.py:185-230),
the per-ray solve (:293-294), the sky lookup (:366-378, with the build's own bilinear filter in
place of Blender's) and the multisample mean (:242-250).  PyTorch is used only as plumbing for
device memory and the stream; all kernels are libbhgeo's.
"""
from __future__ import annotations

import itertools
import os

import numpy as np
import torch

from . import _ffi
from .raygen import euler_xyz_matrix, python_random_stream
from .sky import synthetic_sky  # noqa: F401  (re-exported: tests and bench import it from here)


def _copy_params(p: _ffi.Params) -> _ffi.Params:
    q = _ffi.Params()
    import ctypes
    ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(_ffi.Params))
    return q


# Rays are regenerated IN PLACE, and several frames may read one block of them (FrameBatch's members, a twin frame on a second
# context): every generate_rays() stamps the block's storage with a new number, and whoever keeps something derived from the
# rays keeps the stamp beside it.
_ray_stamp = {}
_next_stamp = itertools.count(1)


def _rays_regenerated(d_k0):
    _ray_stamp[d_k0.untyped_storage().data_ptr()] = next(_next_stamp)


def _rays_key(d_k0):
    return (d_k0.data_ptr(), d_k0.numel(), _ray_stamp.get(d_k0.untyped_storage().data_ptr(), 0))


class StartSteps:
    """The initial DP5(4) steps of a ray set its owner traces again and again (bhg_trace_start_device, include/bhgeo.h): an [n]
    float64 array allocated at the first trace, recorded by it and replayed by every later trace for which the rays (their block,
    its stamp, the origins) are the same and bhg_start_steps_match() accepts the parameters.  Scene changes -- disk, object
    spheres, sky, shading -- never touch it.  Whoever writes into d_k0 in place by other means than generate_rays() calls
    invalidate().  recorded / replayed count the traces of each kind; BHGEO_START_CACHE=0 in the environment or enabled=False
    switch it off (every trace is then the plain call, and no memory is held: 8 B per ray otherwise).

    A shared-origin owner (plan(shared_origin=True)) also keeps the rays' start-up records (bhg_trace_prefix_device: 112 B per
    ray, allocated at the first trace): written by the trace that records the steps, handed to every replaying trace with the rho
    they were written for -- the library tests each call's scene against it and reports what it did (prefix.used).
    prefix_recorded / prefix_replayed / prefix_refused count those answers; BHGEO_START_PREFIX=0 switches the records alone off.
    The records are written by the deep rule (BHG_PREFIX_RECORD_DEEP: rejected attempts kept, three quarters of the clear ball in
    a scene without object spheres whose nearest surface is the horizon) where the library has it; BHGEO_DEEP_PREFIX=0 goes back to BHG_PREFIX_RECORD.
    Where the library has the wide rule (BHG_PREFIX_RECORD_WIDE: fifteen sixteenths of that ball) an owner is promoted to it:
    after 32 traces in a row that all replayed, the next one writes the records again by the wide rule.  BHGEO_WIDE_PREFIX=1
    records by the wide rule from the first trace, BHGEO_WIDE_PREFIX=0 never.
    Where the library has the rim rule (BHG_PREFIX_RECORD_RIM: the ball that ends just above the horizon) the ladder has one more
    rung: 96 further traces in a row that replayed the wide records earn it.  BHGEO_RIM_PREFIX=1 records by the rim rule from the
    first trace, BHGEO_RIM_PREFIX=0 ends the ladder at the wide rule.
    A scene that stays inside the ball (two refused traces in a row) or has left a small ball far behind (eight traces with room
    for twice the radius) has the records written again too, by the owner's first rule.  Every such trace replays its steps;
    the library decides (bhg_prefix_owner_next), and prefix_recorded counts them all."""

    _RECORD_MODES = (_ffi.PREFIX_RECORD, _ffi.PREFIX_RECORD_DEEP, _ffi.PREFIX_RECORD_WIDE, _ffi.PREFIX_RECORD_RIM)

    def __init__(self, enabled=True):
        self.enabled = bool(enabled)
        self.d_h = None
        self.key = self.params = self._pending = None
        self.recorded = self.replayed = 0
        self.d_rec = None
        self.owner = _ffi.PrefixOwner(0.0, 0, 0)   # the library's state of the records in d_rec (bhg_prefix_owner_next)
        self._last = None          # the _ffi.Prefix of the last trace as it came back, or None
        self.prefix = None         # the _ffi.Prefix of the trace being planned, or None
        self.prefix_recorded = self.prefix_replayed = self.prefix_refused = 0

    def invalidate(self):
        self.key = None

    @property
    def valid(self):
        return self.key is not None

    @property
    def rho(self):
        """the records in d_rec were written with this radius (0: none are held)"""
        last = self._last
        if last is not None and last.mode in self._RECORD_MODES and last.used == last.mode:
            return float(last.rho)
        return float(self.owner.rho)

    def _drop_records(self):
        self.owner = _ffi.PrefixOwner(0.0, 0, 0)
        self._last = None

    @staticmethod
    def _rule():
        """(the rule the owner records by, the rule a long clean run promotes it to or PREFIX_NONE)"""
        if os.environ.get("BHGEO_DEEP_PREFIX", "") == "0" or not _ffi.has_deep_prefix():
            return _ffi.PREFIX_RECORD, _ffi.PREFIX_NONE
        wide = os.environ.get("BHGEO_WIDE_PREFIX", "")
        rim = os.environ.get("BHGEO_RIM_PREFIX", "") if _ffi.has_rim_prefix() else "0"
        if rim == "1":
            return _ffi.PREFIX_RECORD_RIM, _ffi.PREFIX_NONE
        if wide == "0" or not _ffi.has_wide_prefix():
            return _ffi.PREFIX_RECORD_DEEP, _ffi.PREFIX_NONE
        top = _ffi.PREFIX_RECORD_RIM if rim != "0" else None     # (the ladder's last rung; None: it ends at the wide rule)
        if wide == "1":
            return _ffi.PREFIX_RECORD_WIDE, top or _ffi.PREFIX_NONE
        return _ffi.PREFIX_RECORD_DEEP, top or _ffi.PREFIX_RECORD_WIDE

    def plan(self, n, dev, key, params, shared_origin=False, origin=None, spheres=None):
        """(d_start_steps, start_mode) of the next trace call, and self.prefix for it (origin, spheres: the call's, which decide
        with params whether held records are replayed or written again).  The steps count as not valid until done(): a call that
        raises leaves them so."""
        self.prefix = None
        if not self.enabled or os.environ.get("BHGEO_START_CACHE", "") == "0":
            self.key = None
            self._drop_records()
            return 0, _ffi.START_NONE
        if self.d_h is None or self.d_h.numel() != n or self.d_h.device != dev:
            self.d_h = torch.empty(n, dtype=torch.float64, device=dev)
            self.d_rec = None
            self.key = None
        replay = self.key is not None and self.key == key and _ffi.start_steps_match(self.params, params)
        self.key = None
        self._pending = (key, _copy_params(params), replay)
        if shared_origin and os.environ.get("BHGEO_START_PREFIX", "") != "0" and _ffi.has_start_prefix():
            if self.d_rec is None:
                self.d_rec = torch.empty(n * _ffi.PREFIX_BYTES_PER_RAY, dtype=torch.uint8, device=dev)
                self._drop_records()
            rule, promote = self._rule()
            if not replay:
                # other rays, another origin, other parameters: from scratch
                self._drop_records()
                ask = rule
            elif _ffi.has_wide_prefix():
                ask = _ffi.prefix_owner_next(self.owner, rule, params, origin, spheres, self._last, promote)
            else:
                # (a library from before bhg_prefix_owner_next: records are written once and replayed or refused ever after)
                self.owner.rho = self.rho
                ask = _ffi.PREFIX_REPLAY if self.owner.rho > 0.0 else _ffi.PREFIX_NONE
            self._last = None
            if ask != _ffi.PREFIX_NONE:
                self.prefix = _ffi.Prefix(self.d_rec.data_ptr(), self.owner.rho if ask == _ffi.PREFIX_REPLAY else 0.0, ask, 0)
        else:
            self._drop_records()
        return self.d_h.data_ptr(), (_ffi.START_REPLAY if replay else _ffi.START_RECORD)

    def done(self):
        if self._pending is None:
            return
        self.key, self.params, replay = self._pending
        self._pending = None
        self._last = self.prefix
        if self.prefix is not None:
            if self.prefix.mode in self._RECORD_MODES:
                self.prefix_recorded += self.prefix.used == self.prefix.mode
            elif self.prefix.used == _ffi.PREFIX_REPLAY:
                self.prefix_replayed += 1
            else:
                self.prefix_refused += 1
        if replay:
            self.replayed += 1
        else:
            self.recorded += 1


class DeviceFrame:
    """All buffers of one frame shard on one GPU.

    pixels: flat pixel ids (y*W + x) this GPU owns (e.g. dist.rank_pixels); None = whole frame.
    Rays are laid out [S][P]: ray s*P + p is sample s of pixel pixels[p].
    """

    def __init__(self, ctx: _ffi.Context, width, height, samples, *, fov_x=1.0, fov_y=1.0, sampling_seed=42.0,
                 origin=(1e-4, 0.0, 30.0), rotation_euler=(0.0, 0.0, 0.0), bh_loc=(0.0, 0.0, 0.0), pixels=None,
                 jitter=None, device=None, buffers=None, directions_only=False, start_cache=True):
        """directions_only: a frame without disk or objects reads only the exit DIRECTIONS of its rays (the sky
        lookup, :366-378) -- trace() then has the kernel write those alone (d_dir [n, 3], bhg_trace_dir_device: half
        the bytes written per ray and read by the shade kernel; d_end is not filled) and shade() / shade_f32() read
        them.  With a disk or objects set the frame falls back to whole end records by itself.
        start_cache: keep the rays' initial steps and start-up records from trace to trace (StartSteps; 8 + 112 B per ray)."""
        self.ctx = ctx
        self.start_steps = StartSteps(start_cache)
        self.directions_only = bool(directions_only)
        self.d_dir = None
        self._dir_traced = False
        self._traced = None      # what the last trace wrote: None (nothing usable), "dir" or "end"
        self.polarisation = None      # _ffi.Polarisation (set_polarisation) or None: off
        self._pol_args = None         # (degree, disk_sense) of set_polarisation: the image's up follows the rotation
        self.W, self.H, self.S = int(width), int(height), int(samples)
        self.fov_x, self.fov_y = float(fov_x), float(fov_y)
        self.origin = np.asarray(origin, dtype=np.float64) - np.asarray(bh_loc, dtype=np.float64)  # :278
        self.rot = euler_xyz_matrix(rotation_euler)
        self.dev = torch.device("cuda", ctx.device) if device is None else device
        if jitter is None:
            jitter = python_random_stream(sampling_seed, 2 * self.S * self.W * self.H)  # :189
        self.d_jitter = torch.as_tensor(np.asarray(jitter, dtype=np.float64)).to(self.dev)
        if pixels is None:
            self.d_pixels = None
            self.P = self.W * self.H
        else:
            self.d_pixels = torch.as_tensor(np.asarray(pixels, dtype=np.int64)).to(self.dev)
            self.P = int(self.d_pixels.numel())
        n = self.S * self.P
        self.n = n
        if buffers is not None:
            # views into a caller-owned block shared by several frames (FrameBatch): one trace call for all
            self.d_k0, self.d_end, self.d_flags, self.d_steps, self.d_acc = buffers
            assert self.d_k0.shape == (n, 3) and (self.d_end is None or self.d_end.shape == (n, 6)) and self.d_flags.numel() == n
        else:
            self.d_k0 = torch.empty((n, 3), dtype=torch.float64, device=self.dev)
            # whole end records: allocated when a full-record trace is first issued (a direction-only frame never needs them)
            self.d_end = None if self.directions_only else torch.empty((n, 6), dtype=torch.float64, device=self.dev)
            self.d_flags = torch.empty(n, dtype=torch.uint8, device=self.dev)
            self.d_steps = torch.empty(n, dtype=torch.int32, device=self.dev)
            self.d_acc = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.d_rgba = torch.empty((self.P, 4), dtype=torch.float64, device=self.dev)
        self.d_sky = None
        self.sky_wh = (0, 0)
        # scene beyond the sky (set_disk / set_objects): thin disk, object spheres with lamps
        self.disk = None
        self.disk_profile = dict(disk_phase=0.0, disk_mean=0.2, disk_stddev=0.3, disk_intensity=1.0)
        self.d_disk_tex = None
        self.spheres = None
        self.sphere_rgb = None
        self.lamps = None
        self.d_obj = None
        self.redshift = None     # _ffi.Redshift (set_redshift) or None: off
        self._params = None      # the parameters of the last trace (the redshift shade needs its metric)
        self.observer = None     # _ffi.Observer (set_observer) or None: the reference camera
        self._ray_key = None     # what the observer rays in d_k0 were made for: (origin, r_s, spin, rhs_form)
        self.d_qu = None              # [P, 6] fp64 Stokes Q / U images (shade_stokes)
        self.disk_thermal = None      # _ffi.DiskThermal (set_disk_thermal) or None: the disk's colour of the scene
        self.object_textures = None   # set_object_textures: (device textures per sphere, rotations, modes, emission) or None
        self.object_motion = None     # _ffi.ObjectMotion (set_object_motion) or None: the spheres at rest
        self.disk_layers = None       # _ffi.DiskLayers (set_disk_layers) or None: the opaque disk of the trace parameters
        self.d_cross = None           # [max_crossings, n, 6] fp64 crossing records and
        self.d_n_cross = None         # [n] uint8 crossing counts of the last crossings trace
        self.phase_rate = 0.0         # set_disk_layers(phase_rate=): d(disk_phase)/dt of the retarded shade, 0 = off
        self.d_t_cross = None         # [max_crossings, n] fp64 crossing times and
        self.d_t_end = None           # [n] fp64 times to the rays' ends of the last travel-time trace (phase_rate != 0 only)
        self.mesh = None              # _ffi.Mesh (set_mesh) or None: no triangle mesh in the curved region
        self.mesh_chord = None        # max_chord of the mesh trace; None: a quarter of the trace parameters' r_s
        self.d_tri_rgb = None         # [nt, 3] fp32 triangle colours, or None (white)
        self.mesh_material = None     # set_mesh(material=): (_ffi.MeshMaterial, its struct over the device copies, the copies)
        self.mesh_instances = None    # _ffi.MeshInstances (set_mesh(instances=)) or None: the mesh where its vertices put it
        self._instance_kind = (False, _ffi.MESH_INSTANCE_TREE_LEAF)   # (tree, leaf_size) of the sets set_mesh() asked for
        self.d_inst_rgb = None        # [K, 3] float32 or None
        self.d_inst_id = None         # [n] int32 of the last instanced trace
        self.d_tri_id = None          # [n] int32 and
        self.d_bary = None            # [n, 2] fp64 of the last mesh trace

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    # The camera is assigned to (an animation moves it from frame to frame): what was kept for the old one goes with it.  A new
    # origin leaves the rays (directions only) but not what the last trace wrote -- shade() would weigh the old records with a g
    # worked out from the new position; a new rotation or field of view also asks render() for new rays, and turns the up of
    # set_polarisation() with the camera.  Assigning the value that is held keeps everything (set_objects compares likewise: an
    # owner may write its whole camera every frame).  origin and rot are the frame's own copies, read-only: a camera changed in
    # place would slip past all this.
    @property
    def origin(self):
        return self._origin

    @origin.setter
    def origin(self, x):
        x = np.array(x, dtype=np.float64).reshape(3)
        x.setflags(write=False)
        if getattr(self, "_origin", None) is not None and x.tobytes() == self._origin.tobytes():
            return
        self._origin = x
        self._traced = None

    def _directions_changed(self):
        self._traced = None
        self._rays_ready = False

    @property
    def rot(self):
        return self._rot

    @rot.setter
    def rot(self, r):
        r = np.array(r, dtype=np.float64).reshape(3, 3)
        r.setflags(write=False)
        if getattr(self, "_rot", None) is not None and r.tobytes() == self._rot.tobytes():
            return
        self._rot = r
        self._directions_changed()
        if self._pol_args is not None:
            self.set_polarisation(*self._pol_args)

    @property
    def fov_x(self):
        return self._fov_x

    @fov_x.setter
    def fov_x(self, v):
        if float(v) != getattr(self, "_fov_x", None):
            self._fov_x = float(v)
            self._directions_changed()

    @property
    def fov_y(self):
        return self._fov_y

    @fov_y.setter
    def fov_y(self, v):
        if float(v) != getattr(self, "_fov_y", None):
            self._fov_y = float(v)
            self._directions_changed()

    @property
    def d_k0(self):
        """The rays' directions [n, 3].  Assigning another tensor (a twin frame reads its sibling's) drops what was kept for
        the old one."""
        return self._d_k0

    @d_k0.setter
    def d_k0(self, t):
        self._d_k0 = t
        self.start_steps.invalidate()

    def set_sky(self, sky_rgba_f32):
        """Equirectangular sky [TH, TW, 4] float32."""
        sky = np.ascontiguousarray(sky_rgba_f32, dtype=np.float32)
        assert sky.ndim == 3 and sky.shape[2] == 4
        self.d_sky = torch.as_tensor(sky).to(self.dev)
        self.sky_wh = (sky.shape[1], sky.shape[0])

    def set_disk(self, r_in, r_out, texture_rgba_f32=None, **profile):
        """Thin disk in z = 0 between r_in and r_out (LimitedRelativisticRenderEngine.py:283-300, :413-438);
        profile: disk_phase, disk_mean, disk_stddev, disk_intensity (:55-58).  The trace must be run with the
        same radii in its params (make_params(disk_r_in=..., disk_r_out=...))."""
        self.disk = (float(r_in), float(r_out))
        self._traced = None      # the scene changed: what the last trace wrote no longer matches it
        self.disk_profile.update(profile)
        if texture_rgba_f32 is not None:
            tex = np.ascontiguousarray(texture_rgba_f32, dtype=np.float32)
            assert tex.ndim == 3 and tex.shape[2] == 4
            self.d_disk_tex = torch.as_tensor(tex).to(self.dev)

    def set_objects(self, spheres, sphere_rgb=None, lamps=None):
        """Object spheres [[cx, cy, cz, radius]] (BH-centred), their colours and the point lamps
        [[x, y, z, intensity]] that light them.  Cheap to call per frame (an animation moves them): the
        values travel as kernel arguments."""
        spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        if self.spheres is None or not np.array_equal(spheres, self.spheres):
            # the geometry the rays were traced against is gone (spheres moved, resized, appeared or went away): what
            # the last trace wrote -- end states, flags, object ids -- no longer fits, and shade() says so
            self._traced = None
        self.spheres = spheres
        self.sphere_rgb = sphere_rgb
        self.lamps = lamps
        if self.d_obj is None:
            self.d_obj = torch.empty(self.n, dtype=torch.int8, device=self.dev)

    def set_redshift(self, apply=("disk", "objects", "sky"), exponent=4.0, disk_sense=1):
        """Weigh the colour of every ray of a class in `apply` ("disk", "objects", "sky") by g^exponent, g = nu_obs / nu_em
        between the camera's ZAMO and the emitter (bhg_shade_scene_redshift_device; include/bhgeo.h).  apply=() or None:
        off, the shade calls as without redshift."""
        self.redshift = _ffi.make_redshift(apply, exponent, disk_sense) if apply else None

    def set_observer(self, velocity=None):
        """The observer camera (bhg_raygen_observer_device): every pixel's direction is the look direction of
        an observer at the camera moving with velocity beta (3 numbers, world axes, relative to the ZAMO; observer.py has the common
        ones), and with redshift on, g is that observer's.  None: the reference camera.  The rays are made anew at the next
        render(), and whenever the origin or the metric of the trace parameters changes."""
        self.observer = _ffi.make_observer(velocity)
        self._traced = None      # the last trace followed the other camera's rays: shade() would give them this observer's g
        self._rays_ready = False
        self._ray_key = None
        self.start_steps.invalidate()

    def set_polarisation(self, degree=None, disk_sense=1):
        """Disk polarisation for shade_stokes() (bhg_shade_scene_polarised_device): degree is a constant or
        a table against the emission cosine (make_polarisation), image up the camera's rotated +y (a rotation assigned later turns
        it).  None: off.  shade() and shade_f32() are the same either way."""
        if degree is None:
            self.polarisation = self._pol_args = None
            return
        self._pol_args = (degree, disk_sense)
        self.polarisation = _ffi.make_polarisation(degree, disk_sense, self.rot @ np.array([0.0, 1.0, 0.0]))

    def set_disk_thermal(self, t_peak=None, nu=None, weights=None, f_col=1.0, scale=1.0, disk_sense=1):
        """The thermal disk in every later shade (bhg_shade_scene_thermal_device): a disk ray's colour is
        the redshifted Novikov-Thorne blackbody of peak temperature t_peak [K] weighed per channel over the frequencies nu [Hz]
        (make_disk_thermal; narrowband() gives one frequency per channel).  t_peak may also be a DiskThermal.  None: off."""
        if t_peak is None:
            self.disk_thermal = None
        elif isinstance(t_peak, _ffi.DiskThermal):
            self.disk_thermal = t_peak
        else:
            self.disk_thermal = _ffi.make_disk_thermal(t_peak, nu, weights, f_col, scale, disk_sense)

    def set_object_motion(self, velocity=None, angular_velocity=None):
        """Moving and spinning object spheres in every later shade (bhg_shade_scene_moving_device):
        velocity and angular_velocity [n][3] per sphere of set_objects() (world axes, dx/dt and rad per unit t; None: zeros;
        observer.circular_orbit_motion gives an orbit).  Only the redshift of object rays changes, and only with redshift on
        objects.  Both None: off -- the images as without motion, bit for bit."""
        if velocity is None and angular_velocity is None:
            self.object_motion = None
        else:
            self.object_motion = _ffi.make_object_motion(velocity, angular_velocity)

    def set_disk_layers(self, max_crossings=None, opacity=1.0, phase_rate=0.0):
        """Higher-order images of the disk (bhg_trace_crossings_device, bhg_shade_disk_layers_device):
        trace() carries every ray THROUGH the disk and records its first max_crossings (1 .. 4) crossings, and shade() /
        shade_f32() / render() composite them front to back, each crossing passing 1 - opacity of what lies behind it
        (0 < opacity <= 1; 1 is the opaque disk).  Redshift, the observer and the thermal disk apply per layer.  Not with
        object spheres, their textures or motion, nor shade_stokes() (ValueError there).  None: off -- every path the one
        it was, bit for bit.
        phase_rate (d(disk_phase)/dt as the animation turns the disk, radians per unit of coordinate time; DESIGN.md section
        18): non-zero, trace() also keeps each crossing's light travel time (bhg_travel_time_device: d_t_cross, d_t_end) and
        the shades draw layer m of a ray at disk_phase - phase_rate * t_cross[m] (bhg_shade_disk_layers_retarded_device).
        Zero: the calls and the images of the plain layers."""
        self._traced = None      # what the last trace wrote belongs to the other kind of trace
        if not np.isfinite(float(phase_rate)):
            raise ValueError("phase_rate must be finite")
        self.phase_rate = float(phase_rate) if max_crossings is not None else 0.0
        if max_crossings is None:
            self.disk_layers = None
            return
        if not 1 <= int(max_crossings) <= _ffi.MAX_CROSSINGS:
            raise ValueError(f"max_crossings must be in [1, {_ffi.MAX_CROSSINGS}]")
        if not 0.0 < float(opacity) <= 1.0:
            raise ValueError("opacity must be in (0, 1]")
        self.disk_layers = _ffi.make_disk_layers(max_crossings, opacity)

    def set_mesh(self, mesh=None, tri_rgb=None, chord=None, lamps=None, material=None, instances=None, inst_rgb=None, build="host",
                 instance_tree=False, instance_leaf_size=_ffi.MESH_INSTANCE_TREE_LEAF):
        """A triangle mesh in the curved region (bhg_trace_mesh_device, bhg_shade_mesh_device): trace()
        ends a ray where its curve meets a triangle and keeps d_tri_id [n] int32 / d_bary [n, 2]; shade() / shade_f32() /
        render() light the mesh rays (tri_rgb [nt, 3] per triangle, default white; the lamps of set_objects([], lamps=...) or
        lamps=; shadows cast by the mesh itself), every other ray as without the mesh.  mesh: an _ffi.Mesh of this frame's
        context, or (vertices, triangles).  chord: the sub-chord length of the trace, default a quarter of r_s.  Not with
        object spheres, disk layers, redshift, polarisation, the thermal disk or shade_stokes() (ValueError).  The kept
        initial steps and start-up records are neither used nor touched.  None: off -- every path the one it was, bit for bit.
        material: an _ffi.MeshMaterial (per-corner UVs, image textures, emission; bhg_shade_mesh_material_device, DESIGN.md
        section 20) in place of tri_rgb -- both together are a ValueError; without it the shade is the existing call.
        instances: [K, 12] or [K, 3, 4] rigid placements of the mesh (bhg_trace_mesh_instances_device,
        bhg_shade_mesh_instances_device) -- trace() also keeps d_inst_id [n]; inst_rgb [K, 3] float32
        multiplies the albedo per instance.  set_mesh_instances(T) moves them afterwards.
        instance_tree=True: the set lies under a tree of boxes with leaves of instance_leaf_size, and K
        may go up to _ffi.MESH_INSTANCE_TREE_MAX; the image is the linear set's, bit for bit.
        build: "host" or "device" (DESIGN.md section 23), for a mesh given as (vertices, triangles); rebuild_mesh() then gives
        either a new triangle list in place."""
        if build not in ("host", "device"):
            raise ValueError('build must be "host" or "device"')
        if material is not None and tri_rgb is not None:
            raise ValueError("material and tri_rgb together: the material carries the triangle colours")
        if inst_rgb is not None and instances is None:
            raise ValueError("inst_rgb goes with instances=")
        self._traced = None
        if self.mesh_instances is not None:
            self.mesh_instances.close()
        self.mesh_instances = self.d_inst_rgb = None
        self._instance_kind = (bool(instance_tree), int(instance_leaf_size))
        if mesh is None:
            self.mesh = self.d_tri_rgb = self.mesh_chord = self.mesh_material = None
            return
        if not isinstance(mesh, _ffi.Mesh):
            mesh = _ffi.Mesh(self.ctx, mesh[0], mesh[1], build=build)
        if mesh.ctx is not self.ctx:
            raise ValueError("the mesh belongs to another context")
        if chord is not None and not (np.isfinite(float(chord)) and float(chord) > 0.0):
            raise ValueError("chord must be finite and > 0")
        self.d_tri_rgb = self.mesh_material = None
        if material is not None:
            material.check_triangles(mesh.n_triangles)
            dev = [None if a is None else torch.as_tensor(a).to(self.dev) for a in material.arrays()]
            self.mesh_material = (material, material.struct([0 if t is None else t.data_ptr() for t in dev]), dev)
        if tri_rgb is not None:
            rgb = np.ascontiguousarray(tri_rgb, dtype=np.float32)
            if rgb.shape != (mesh.n_triangles, 3):
                raise ValueError("tri_rgb must have shape [n_triangles, 3]")
            self.d_tri_rgb = torch.as_tensor(rgb).to(self.dev)
        self.mesh, self.mesh_chord = mesh, None if chord is None else float(chord)
        if lamps is not None:
            self.lamps = lamps
        self._mesh_check()
        if instances is not None:
            self.mesh_instances = _ffi.MeshInstances(mesh, instances, *self._instance_kind)
            if inst_rgb is not None:
                rgb = np.ascontiguousarray(inst_rgb, dtype=np.float32)
                if rgb.shape != (self.mesh_instances.n, 3):
                    raise ValueError("inst_rgb must have shape [K, 3]")
                self.d_inst_rgb = torch.as_tensor(rgb).to(self.dev)

    def set_mesh_instances(self, transforms=None):
        """Move the instances of set_mesh(instances=): K x 18 doubles go to the device, nothing is rebuilt (bhg_mesh_instances_set).
        Another K makes a new set of the kind set_mesh() asked for (inst_rgb is then dropped); None turns instances off -- the mesh where its vertices put it."""
        if self.mesh is None:
            raise ValueError("set_mesh_instances() wants a mesh: set_mesh() first")
        self._traced = None
        T = None if transforms is None else _ffi._instance_transforms(transforms)
        if T is not None and self.mesh_instances is not None and T.shape[0] == self.mesh_instances.n:
            self.mesh_instances.set(T)
            return
        if self.mesh_instances is not None:
            self.mesh_instances.close()
        self.mesh_instances = self.d_inst_rgb = None
        if T is not None:
            self.mesh_instances = _ffi.MeshInstances(self.mesh, T, *self._instance_kind)

    def refit_mesh(self, vertices, vertex_normals=None):
        """New vertex positions (and vertex normals) for the held mesh, its tree refitted on the device (Mesh.refit; DESIGN.md
        section 22): numpy arrays, or float64 tensors on the frame's device.  Held instances are set again with their
        transforms, so the next trace is current.  The frame's own stream is waited for first: no trace still reads the mesh."""
        if self.mesh is None:
            raise ValueError("refit_mesh() wants a mesh: set_mesh() first")
        torch.cuda.current_stream(self.dev).synchronize()
        self.mesh.refit(vertices, vertex_normals, stream=self._stream())
        self._traced = None
        if self.mesh_instances is not None:
            self.mesh_instances.set(self.mesh_instances.transforms)

    def rebuild_mesh(self, vertices, triangles, vertex_normals=None, material=None, tri_rgb=None):
        """A new triangle list (vertices, triangles, and vertex normals for a mesh that has them) for the held mesh, within its
        capacity: its tree is built anew on the device, in place (Mesh.rebuild).  numpy arrays, or tensors
        on the frame's device.  material / tri_rgb replace the held one; a held per-triangle array that no longer matches
        n_triangles, with no new one given, is a ValueError (nothing is changed then).  Held instances are set again."""
        if self.mesh is None:
            raise ValueError("rebuild_mesh() wants a mesh: set_mesh() first")
        if material is not None and tri_rgb is not None:
            raise ValueError("material and tri_rgb together: the material carries the triangle colours")
        nt = int(triangles.shape[0]) if hasattr(triangles, "shape") else len(triangles)
        new_material = new_rgb = None
        if material is not None:
            material.check_triangles(nt)
            dev = [None if a is None else torch.as_tensor(a).to(self.dev) for a in material.arrays()]
            new_material = (material, material.struct([0 if t is None else t.data_ptr() for t in dev]), dev)
        elif tri_rgb is not None:
            rgb = np.ascontiguousarray(tri_rgb, dtype=np.float32)
            if rgb.shape != (nt, 3):
                raise ValueError("tri_rgb must have shape [n_triangles, 3]")
            new_rgb = torch.as_tensor(rgb).to(self.dev)
        elif nt != self.mesh.n_triangles:
            if self.d_tri_rgb is not None:
                raise ValueError(f"the held tri_rgb is for {self.mesh.n_triangles} triangles, the new list has {nt}: give tri_rgb=")
            if self.mesh_material is not None and any(a is not None for a in self.mesh_material[0].arrays()[:3]):
                raise ValueError(f"the held material's per-triangle arrays are for {self.mesh.n_triangles} triangles, the new list "
                                 f"has {nt}: give material=")
        torch.cuda.current_stream(self.dev).synchronize()
        self.mesh.rebuild(vertices, triangles, vertex_normals, stream=self._stream())
        self._traced = None
        if material is not None:
            self.mesh_material, self.d_tri_rgb = new_material, None
        elif tri_rgb is not None:
            self.d_tri_rgb, self.mesh_material = new_rgb, None
        if self.mesh_instances is not None:
            self.mesh_instances.set(self.mesh_instances.transforms)

    def _mesh_check(self):
        for name, on in (("object spheres", self.spheres is not None and len(self.spheres) > 0),
                         ("disk layers", self.disk_layers is not None), ("redshift", self.redshift is not None),
                         ("polarisation", self.polarisation is not None), ("the thermal disk", self.disk_thermal is not None)):
            if on:
                raise ValueError(f"a mesh does not go with {name}")

    def _layers_check(self):
        if (self.spheres is not None and len(self.spheres) > 0) or self.object_textures is not None or self.object_motion is not None:
            raise ValueError("disk layers do not go with object spheres, object textures or object motion")
        if self.disk is None:
            raise ValueError("disk layers need a disk: set_disk() first")

    def set_object_textures(self, textures=None, rotations=None, modes=None, emission=None):
        """Textured, oriented and emissive object spheres (bhg_shade_scene_textured_device), per sphere of
        set_objects(): textures [h, w, 4] float32 (kept on the device; None: keep that sphere's current texture, white if it
        never had one), 3x3 body -> world rotations (None: the identity), modes ("lit" / "emissive"), emission strengths.
        shade() and shade_f32() then take the textured call whenever the frame has spheres.  All None: textures off."""
        if textures is None and rotations is None and modes is None and emission is None:
            self.object_textures = None
            return
        dev = [None] * _ffi.MAX_SPHERES if self.object_textures is None else list(self.object_textures[0])
        for j, t in enumerate(textures or []):
            if t is not None:
                a = np.ascontiguousarray(t, dtype=np.float32)
                assert a.ndim == 3 and a.shape[2] == 4
                dev[j] = torch.as_tensor(a).to(self.dev)
        self.object_textures = (dev, rotations, modes, emission)

    def _object_textures(self):
        dev, rotations, modes, emission = self.object_textures
        tex = [None if t is None else (t.data_ptr(), t.shape[1], t.shape[0]) for t in dev]
        return _ffi.make_object_textures(tex, rotations, modes, emission)[0]

    def _textured(self):
        return self.object_textures is not None and self.spheres is not None and len(self.spheres) > 0

    def _observer_key(self, params):
        return (tuple(float(v) for v in self.origin), float(params.r_s), float(params.spin), int(params.rhs_form))

    def pixel_cost(self):
        """Attempted steps of the last trace summed over the samples of each pixel ([P], order of `pixels`): the
        measured cost dist.measured_tile_cost() orders and deals the tiles by."""
        return self.d_steps.view(self.S, self.P).to(torch.int64).sum(0)

    def generate_rays(self, params: _ffi.Params = None):
        """params: the trace parameters (their metric) -- needed by the observer camera only."""
        self._traced = None      # new rays: results of an earlier trace belong to the old ones
        self.start_steps.invalidate()
        _rays_regenerated(self.d_k0)     # (... and so do the steps every other frame over this block keeps)
        if self.observer is not None:
            if params is None:
                raise RuntimeError("the observer camera needs the trace parameters: generate_rays(params)")
            self.ctx.raygen_observer_device(params, self.observer, self.origin, self.W, self.H, self.S, self.fov_x, self.fov_y,
                                            self.d_jitter.data_ptr(), self.d_k0.data_ptr(), self.P,
                                            d_pixels=0 if self.d_pixels is None else self.d_pixels.data_ptr(),
                                            rot=self.rot, stream=self._stream())
            self._ray_key = self._observer_key(params)
            return
        self.ctx.raygen_device(self.W, self.H, self.S, self.fov_x, self.fov_y, self.d_jitter.data_ptr(),
                               self.d_k0.data_ptr(), self.P,
                               d_pixels=0 if self.d_pixels is None else self.d_pixels.data_ptr(),
                               rot=self.rot, stream=self._stream())

    def trace(self, params: _ffi.Params):
        # work-order hint: the rays are S blocks of P (sample-major); lets the library start all samples of a
        # region together (the pixels of a shard are usually sorted longest-first, dist.rank_pixels(tile_cost=))
        if params.order_blocks == 0 and self.S > 1:
            params = _copy_params(params)
            params.order_blocks = self.S
        self._params = params
        origin = np.asarray(self.origin, dtype=np.float64)
        if self.mesh is not None:
            # the mesh trace: whole records, its own kernel, the plain call; the kept initial steps are neither used nor touched
            self._mesh_check()
            if self.d_end is None:
                self.d_end = torch.empty((self.n, 6), dtype=torch.float64, device=self.dev)
            if self.d_tri_id is None:
                self.d_tri_id = torch.empty(self.n, dtype=torch.int32, device=self.dev)
                self.d_bary = torch.empty((self.n, 2), dtype=torch.float64, device=self.dev)
            self._dir_traced, self._traced = False, None
            chord = 0.25 * float(params.r_s) if self.mesh_chord is None else self.mesh_chord
            if self.mesh_instances is not None:
                if self.d_inst_id is None:
                    self.d_inst_id = torch.empty(self.n, dtype=torch.int32, device=self.dev)
                self.ctx.trace_mesh_instances_device(params, self.mesh_instances, chord, self.n, self.d_k0.data_ptr(),
                                                     self.d_end.data_ptr(), self.d_tri_id.data_ptr(), self.d_inst_id.data_ptr(),
                                                     self.d_bary.data_ptr(), x0_shared=origin, d_flags=self.d_flags.data_ptr(),
                                                     d_n_steps=self.d_steps.data_ptr(), d_n_accepted=self.d_acc.data_ptr(),
                                                     stream=self._stream())
                self._traced = "mesh"
                return
            self.ctx.trace_mesh_device(params, self.mesh, chord, self.n, self.d_k0.data_ptr(), self.d_end.data_ptr(),
                                       self.d_tri_id.data_ptr(), self.d_bary.data_ptr(), x0_shared=origin,
                                       d_flags=self.d_flags.data_ptr(), d_n_steps=self.d_steps.data_ptr(),
                                       d_n_accepted=self.d_acc.data_ptr(), stream=self._stream())
            self._traced = "mesh"
            return
        if self.disk_layers is not None:
            # the crossings trace: whole records, its own kernel; the kept initial steps are neither used nor touched
            self._layers_check()
            K = int(self.disk_layers.max_crossings)
            if self.d_end is None:
                self.d_end = torch.empty((self.n, 6), dtype=torch.float64, device=self.dev)
            if self.d_cross is None or self.d_cross.shape[0] != K:
                self.d_cross = torch.empty((K, self.n, 6), dtype=torch.float64, device=self.dev)
                self.d_n_cross = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
            self._dir_traced, self._traced = False, None
            if self.phase_rate != 0.0:
                if self.d_t_cross is None or self.d_t_cross.shape[0] != K:
                    self.d_t_cross = torch.empty((K, self.n), dtype=torch.float64, device=self.dev)
                    self.d_t_end = torch.empty(self.n, dtype=torch.float64, device=self.dev)
                self.ctx.travel_time_device(params, self.n, self.d_k0.data_ptr(), K, self.d_end.data_ptr(), self.d_t_end.data_ptr(),
                                            d_cross=self.d_cross.data_ptr(), d_n_cross=self.d_n_cross.data_ptr(),
                                            d_t_cross=self.d_t_cross.data_ptr(), x0_shared=origin, d_flags=self.d_flags.data_ptr(),
                                            d_n_steps=self.d_steps.data_ptr(), d_n_accepted=self.d_acc.data_ptr(),
                                            stream=self._stream())
                self._traced = "layers_t"
                return
            self.ctx.trace_crossings_device(params, self.n, self.d_k0.data_ptr(), K, self.d_end.data_ptr(), self.d_cross.data_ptr(),
                                            self.d_n_cross.data_ptr(), x0_shared=origin, d_flags=self.d_flags.data_ptr(),
                                            d_n_steps=self.d_steps.data_ptr(), d_n_accepted=self.d_acc.data_ptr(),
                                            stream=self._stream())
            self._traced = "layers"
            return
        has_obj = self.spheres is not None and len(self.spheres) > 0
        self._dir_traced = self.directions_only and not has_obj and self.disk is None and not (params.disk_r_out > 0.0)
        self._traced = "dir" if self._dir_traced else "end"
        # the initial steps belong to the rays and the origin they start from: recorded by the first trace, replayed after
        d_h, mode = self.start_steps.plan(self.n, self.dev, (_rays_key(self.d_k0), origin.tobytes()), params, shared_origin=True,
                                          origin=origin, spheres=self.spheres if has_obj else None)
        prefix = self.start_steps.prefix
        if self._dir_traced:
            if self.d_dir is None:
                self.d_dir = torch.empty((self.n, 3), dtype=torch.float64, device=self.dev)
            self.ctx.trace_dir_device(params, self.n, self.d_k0.data_ptr(), self.d_dir.data_ptr(), x0_shared=origin,
                                      d_flags=self.d_flags.data_ptr(), d_n_steps=self.d_steps.data_ptr(),
                                      d_n_accepted=self.d_acc.data_ptr(), stream=self._stream(), d_start_steps=d_h,
                                      start_mode=mode, prefix=prefix)
            self.start_steps.done()
            return
        if self.d_end is None:
            self.d_end = torch.empty((self.n, 6), dtype=torch.float64, device=self.dev)
        self.ctx.trace_device(params, self.n, self.d_k0.data_ptr(), self.d_end.data_ptr(), x0_shared=origin,
                              d_flags=self.d_flags.data_ptr(), d_n_steps=self.d_steps.data_ptr(),
                              d_n_accepted=self.d_acc.data_ptr(), stream=self._stream(),
                              spheres=self.spheres if has_obj else None,
                              d_object_id=self.d_obj.data_ptr() if has_obj else 0, d_start_steps=d_h, start_mode=mode,
                              prefix=prefix)
        self.start_steps.done()

    def scene(self):
        tex = self.d_disk_tex
        return _ffi.make_scene(self.d_sky.data_ptr(), self.sky_wh[0], self.sky_wh[1],
                               d_disk_tex=0 if tex is None else tex.data_ptr(),
                               disk_w=0 if tex is None else tex.shape[1], disk_h=0 if tex is None else tex.shape[0],
                               disk=self.disk, spheres=self.spheres, sphere_rgb=self.sphere_rgb, lamps=self.lamps,
                               **self.disk_profile)

    def _shade_form(self):
        """ONE predicate for both shade paths: "dir" (exit directions, sky only) or "end" (whole records, any scene);
        raises when the scene was changed after the last trace so that its output no longer fits."""
        if self.d_sky is None:
            raise RuntimeError("set_sky() first")
        traced = self._traced
        if traced is None:
            raise RuntimeError("trace() first (the scene changed since the last trace, or nothing was traced yet)")
        has_scene = self.disk is not None or (self.spheres is not None and len(self.spheres) > 0)
        if traced == "dir" and has_scene:
            raise RuntimeError("the last trace wrote exit directions only, but the frame now has a disk / objects: trace() again")
        return traced

    def _shade(self, d_rgba=0, d_rgba_f32=0, scatter=None, pol=None, d_qu=0):
        """The one shade call of every output (bhg_shade_scene_moving_device): redshift, the observer, the object textures,
        the polarisation (shade_stokes only), the thermal disk and the object motion as set, each None when off -- pol = None
        and none of the others is the textured call exactly."""
        form = self._shade_form()
        if (form == "mesh") != (self.mesh is not None):
            raise RuntimeError("set_mesh() changed since the last trace: trace() again")
        if form == "mesh":
            if pol is not None:
                raise ValueError("a mesh has no Stokes images: shade_stokes() is not available with set_mesh()")
            self._mesh_check()
            if self.mesh_instances is not None:
                # (the instanced shade takes tri_rgb= as a material that holds nothing else)
                mat = self.mesh_material[1] if self.mesh_material is not None else (
                    None if self.d_tri_rgb is None else _ffi.MeshMaterial().struct([self.d_tri_rgb.data_ptr(), 0, 0]))
                self.ctx.shade_mesh_instances_device(self.d_end.data_ptr(), self.d_flags.data_ptr(), self.d_tri_id.data_ptr(),
                                                     self.d_inst_id.data_ptr(), self.d_bary.data_ptr(), self.P, self.S, self.scene(),
                                                     self.mesh_instances, mat,
                                                     d_inst_rgb=0 if self.d_inst_rgb is None else self.d_inst_rgb.data_ptr(),
                                                     d_rgba=d_rgba, d_rgba_f32=d_rgba_f32,
                                                     d_scatter=0 if scatter is None else scatter.data_ptr(), stream=self._stream())
                return
            if self.mesh_material is not None:
                self.ctx.shade_mesh_material_device(self.d_end.data_ptr(), self.d_flags.data_ptr(), self.d_tri_id.data_ptr(),
                                                    self.d_bary.data_ptr(), self.P, self.S, self.scene(), self.mesh,
                                                    self.mesh_material[1], d_rgba=d_rgba, d_rgba_f32=d_rgba_f32,
                                                    d_scatter=0 if scatter is None else scatter.data_ptr(), stream=self._stream())
                return
            self.ctx.shade_mesh_device(self.d_end.data_ptr(), self.d_flags.data_ptr(), self.d_tri_id.data_ptr(),
                                       self.d_bary.data_ptr(), self.P, self.S, self.scene(), self.mesh,
                                       d_tri_rgb=0 if self.d_tri_rgb is None else self.d_tri_rgb.data_ptr(), d_rgba=d_rgba,
                                       d_rgba_f32=d_rgba_f32, d_scatter=0 if scatter is None else scatter.data_ptr(),
                                       stream=self._stream())
            return
        if form == "layers_t":      # the layers of a travel-time trace: the crossing times are there
            if self.disk_layers is None or self.phase_rate == 0.0:
                raise RuntimeError("set_disk_layers() changed since the last trace: trace() again")
            if pol is not None:
                raise ValueError("disk layers have no Stokes images: shade_stokes() is not available with set_disk_layers()")
            self._layers_check()
            self.ctx.shade_disk_layers_retarded_device(self.d_end.data_ptr(), self.d_flags.data_ptr(), self.d_cross.data_ptr(),
                                                       self.d_n_cross.data_ptr(), self.d_t_cross.data_ptr(), self.phase_rate,
                                                       self.P, self.S, self.scene(), self.disk_layers, params=self._params,
                                                       rs=self.redshift, obs=self.observer, th=self.disk_thermal,
                                                       x0_shared=self.origin, d_k0=self.d_k0.data_ptr(), d_rgba=d_rgba,
                                                       d_rgba_f32=d_rgba_f32,
                                                       d_scatter=0 if scatter is None else scatter.data_ptr(),
                                                       stream=self._stream())
            return
        if (form == "layers") != (self.disk_layers is not None) or (form == "layers" and self.phase_rate != 0.0):
            raise RuntimeError("set_disk_layers() changed since the last trace: trace() again")
        if form == "layers":
            if pol is not None:
                raise ValueError("disk layers have no Stokes images: shade_stokes() is not available with set_disk_layers()")
            self._layers_check()
            self.ctx.shade_disk_layers_device(self.d_end.data_ptr(), self.d_flags.data_ptr(), self.d_cross.data_ptr(),
                                              self.d_n_cross.data_ptr(), self.P, self.S, self.scene(), self.disk_layers,
                                              params=self._params, rs=self.redshift, obs=self.observer, th=self.disk_thermal,
                                              x0_shared=self.origin, d_k0=self.d_k0.data_ptr(), d_rgba=d_rgba,
                                              d_rgba_f32=d_rgba_f32, d_scatter=0 if scatter is None else scatter.data_ptr(),
                                              stream=self._stream())
            return
        has_obj = self.spheres is not None and len(self.spheres) > 0
        self.ctx.shade_scene_moving_device(self.d_end.data_ptr() if form == "end" else 0, self.d_flags.data_ptr(), self.P, self.S,
                                           self.scene(), self._params, self.redshift, self.observer,
                                           self._object_textures() if self._textured() else None, pol, d_qu, self.disk_thermal,
                                           self.object_motion if has_obj else None,
                                           x0_shared=self.origin, d_k0=self.d_k0.data_ptr(), d_rgba=d_rgba, d_rgba_f32=d_rgba_f32,
                                           d_object_id=0 if self.d_obj is None else self.d_obj.data_ptr(),
                                           d_scatter=0 if scatter is None else scatter.data_ptr(),
                                           d_end_dir=self.d_dir.data_ptr() if form == "dir" else 0, stream=self._stream())

    def shade(self):
        self._shade(d_rgba=self.d_rgba.data_ptr())
        return self.d_rgba

    def shade_stokes(self):
        """(rgba [P, 4], qu [P, 6]) fp64: shade() and the per-pixel means of (Q_r, Q_g, Q_b, U_r, U_g, U_b) of the disk's
        polarisation (set_polarisation first)."""
        if self.disk_layers is not None:
            raise ValueError("disk layers have no Stokes images: shade_stokes() is not available with set_disk_layers()")
        if self.mesh is not None:
            raise ValueError("a mesh has no Stokes images: shade_stokes() is not available with set_mesh()")
        if self.polarisation is None:
            raise RuntimeError("set_polarisation() first")
        if self.d_qu is None:
            self.d_qu = torch.empty((self.P, 6), dtype=torch.float64, device=self.dev)
        self._shade(d_rgba=self.d_rgba.data_ptr(), pol=self.polarisation, d_qu=self.d_qu.data_ptr())
        return self.d_rgba, self.d_qu

    def shade_f32(self, out, scatter=None):
        """Shade + sample mean written as float32 RGBA into `out` ([P, 4], or [H*W, 4] with scatter = this shard's
        flat pixel ids): what layer.rect takes, without the fp64 intermediate."""
        assert out.dtype == torch.float32 and out.is_contiguous()
        self._shade(d_rgba_f32=out.data_ptr(), scatter=scatter)
        return out

    def render(self, params: _ffi.Params, regenerate_rays=False):
        """rays (cached: the engine re-seeds identically every frame) -> trace -> shade."""
        if self.observer is not None and self._ray_key != self._observer_key(params):
            regenerate_rays = True   # the observer's tetrad depends on the camera position and the metric
        if regenerate_rays or not getattr(self, "_rays_ready", False):
            self.generate_rays(params)
            self._rays_ready = True
        self.trace(params)
        return self.shade()


class FrameBatch:
    """Several cameras' frames of the same size traced by ONE library call (per-ray origins, bhg_trace_device's
    d_x0): e.g. the five inclinations of a disk study.  Each member is a DeviceFrame whose ray buffers are views
    into one block; shading stays per frame."""

    def __init__(self, ctx: _ffi.Context, cameras, width, height, samples, *, pixels=None, jitter=None, device=None,
                 start_cache=True, **frame_kw):
        """cameras: list of dicts with origin=, rotation_euler= (and optionally bh_loc=).
        start_cache: keep the rays' initial steps from trace to trace (StartSteps), keyed on the members' rays and origins."""
        self.ctx = ctx
        self.start_steps = StartSteps(start_cache)
        dev = torch.device("cuda", ctx.device) if device is None else device
        W, H, S = int(width), int(height), int(samples)
        P = W * H if pixels is None else len(pixels)
        n1 = S * P
        m = len(cameras)
        if jitter is None:
            jitter = python_random_stream(frame_kw.get("sampling_seed", 42.0), 2 * S * W * H)
        self.d_k0 = torch.empty((m * n1, 3), dtype=torch.float64, device=dev)
        self.d_x0 = torch.empty((m * n1, 3), dtype=torch.float64, device=dev)
        self.d_end = torch.empty((m * n1, 6), dtype=torch.float64, device=dev)
        self.d_flags = torch.empty(m * n1, dtype=torch.uint8, device=dev)
        self.d_steps = torch.empty(m * n1, dtype=torch.int32, device=dev)
        self.d_acc = torch.empty(m * n1, dtype=torch.int32, device=dev)
        self.frames = []
        for j, cam in enumerate(cameras):
            sl = slice(j * n1, (j + 1) * n1)
            f = DeviceFrame(ctx, W, H, S, pixels=pixels, jitter=jitter, device=dev, start_cache=start_cache,
                            buffers=(self.d_k0[sl], self.d_end[sl], self.d_flags[sl], self.d_steps[sl], self.d_acc[sl]),
                            **cam, **frame_kw)
            self.d_x0[sl] = torch.as_tensor(np.array(f.origin), device=dev)
            self.frames.append(f)
        self.n = m * n1
        self.dev = dev
        self._origins = b"".join(np.asarray(f.origin, dtype=np.float64).tobytes() for f in self.frames)

    def generate_rays(self):
        for f in self.frames:
            f.generate_rays()

    def trace(self, params: _ffi.Params):
        # work-order hint: the rays are (cameras x samples) equal blocks of P rays, each block's pixels in the same
        # (usually longest-first) order: lets the library start the expensive regions of ALL frames first
        nb = len(self.frames) * self.frames[0].S
        if params.order_blocks == 0 and nb > 1:
            params = _copy_params(params)
            params.order_blocks = nb
        # (the members regenerate their rays in place, which stamps the block; d_x0 holds the origins they had at construction)
        key = (_rays_key(self.d_k0), self.d_x0.data_ptr(), self._origins)
        d_h, mode = self.start_steps.plan(self.n, self.dev, key, params)
        self.ctx.trace_device(params, self.n, self.d_k0.data_ptr(), self.d_end.data_ptr(), d_x0=self.d_x0.data_ptr(),
                              d_flags=self.d_flags.data_ptr(), d_n_steps=self.d_steps.data_ptr(),
                              d_n_accepted=self.d_acc.data_ptr(),
                              stream=torch.cuda.current_stream(self.dev).cuda_stream, d_start_steps=d_h, start_mode=mode)
        self.start_steps.done()
        for f in self.frames:    # (whole records, whatever the members were constructed with)
            f._dir_traced, f._traced, f._params = False, "end", params

    def set_redshift(self, apply=("disk", "objects", "sky"), exponent=4.0, disk_sense=1):
        """DeviceFrame.set_redshift for every member frame."""
        for f in self.frames:
            f.set_redshift(apply, exponent, disk_sense)

    def set_disk_thermal(self, t_peak=None, nu=None, weights=None, f_col=1.0, scale=1.0, disk_sense=1):
        """DeviceFrame.set_disk_thermal for every member frame."""
        for f in self.frames:
            f.set_disk_thermal(t_peak, nu, weights, f_col, scale, disk_sense)

    def shade(self):
        return [f.shade() for f in self.frames]

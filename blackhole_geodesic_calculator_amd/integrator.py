"""Host-side mirror of the solver object the reference's render engine drives.

Reference interface (the package it comes from, curvedpy, is not in the reference tree):
    curvedpy.GeodesicIntegratorSchwarzschild(mass=, time_like=False, verbose=False)
                                                    raytracer/RelativisticRenderEngine.py:134
    .calc_trajectory(k0_xyz, x0_xyz, max_step=, curve_end=, nr_points_curve=10000, verbose=False)
        -> (k_xyz, x_xyz, result)                   raytracer/RelativisticRenderEngine.py:293-294
    consumed: x_xyz[axis][-1], k_xyz[axis][-1]      :299-308
              result['start_inside_hole'], result['hit_blackhole']   :296-297

Same names, argument meaning and return shapes; the arithmetic runs on the GPU through
libbhgeo.so (include/bhgeo.h).  `trace()` is the batched form (one launch for N rays) that the
frame driver and the pre-traced camera use (Cam edition contract, CamEdition.py:225-228).
"""
from __future__ import annotations

import numpy as np

from . import _ffi

_METHODS = {"RK45": _ffi.METHOD_DP54, "DP54": _ffi.METHOD_DP54, "RK4": _ffi.METHOD_RK4}
_RHS = {"christoffel": _ffi.RHS_CHRISTOFFEL, "reduced": _ffi.RHS_REDUCED, "kerr_bl": _ffi.RHS_KERR_BL}


class GeodesicIntegratorSchwarzschild:
    """Geodesic integrator around a Schwarzschild black hole of horizon radius 2*mass: null rays (time_like=False, what
    the engine asks for) or massive particles (time_like=True)."""

    def __init__(self, mass=1.0, time_like=False, verbose=False, *, device=0, rtol=1e-3, atol=1e-6,
                 method="RK45", rhs_form="christoffel", h_fixed=0.1, max_steps=0, context=None):
        if method not in _METHODS:
            raise ValueError(f"method must be one of {sorted(_METHODS)}")
        if rhs_form not in _RHS:
            raise ValueError(f"rhs_form must be one of {sorted(_RHS)}")
        self.mass = float(mass)
        self.r_s = 2.0 * self.mass  # R_horizon = 2*M in geometrized units (:95)
        # time_like=True: massive particles, g(k, k) = -1, the curve parameter is the proper time -- the initial
        # "direction" k0 is then dx/dtau (the engine only ever passes False, RelativisticRenderEngine.py:134).  The norm
        # enters the Christoffel form through (k^t)^2 and the Boyer-Lindquist form through E and L at the start; the
        # reduced form is the closed form for NULL rays and cannot be asked for it.
        self.time_like = bool(time_like)
        if self.time_like and rhs_form == "reduced":
            raise ValueError("rhs_form='reduced' is the null closed form: time_like=True needs 'christoffel' or 'kerr_bl'")
        self.verbose = bool(verbose)
        self.rtol, self.atol = float(rtol), float(atol)
        self.method, self.rhs_form = method, rhs_form
        self.h_fixed, self.max_steps = float(h_fixed), int(max_steps)
        self.spin = 0.0  # Kerr a in length units (GeodesicIntegratorKerr)
        self._ctx = context if context is not None else _ffi.Context(device)

    # ------------------------------------------------------------------------------------
    @property
    def context(self) -> _ffi.Context:
        return self._ctx

    def params(self, max_step=np.inf, curve_end=50.0, r_exit=0.0, disk=None) -> _ffi.Params:
        if max_step is None or max_step == -1:  # the engine's "unset" sentinel (:59-60)
            max_step = np.inf
        return _ffi.make_params(r_s=self.r_s, lambda_end=curve_end, max_step=max_step, rtol=self.rtol,
                                atol=self.atol, h_fixed=self.h_fixed, r_exit=r_exit,
                                method=_METHODS[self.method], rhs_form=_RHS[self.rhs_form],
                                max_steps=self.max_steps, disk_r_in=disk[0] if disk else 0.0,
                                disk_r_out=disk[1] if disk else 0.0, spin=self.spin, time_like=self.time_like)

    # ------------------------------------------------------------------------------------
    def trace(self, k0, x0, max_step=np.inf, curve_end=50.0, r_exit=0.0, disk=None, spheres=None, redshift=None,
              polarisation=None, disk_thermal=None, disk_crossings=None, travel_time=False, mesh=None, mesh_chord=None,
              mesh_instances=None, mesh_build="host", mesh_instance_tree=False):
        """Batched solve.  k0[N,3] (or [...,3]); x0[3] shared origin or same leading shape as k0.
        r_exit: outward sphere-exit radius (Limited engine's ray_trace, Limited...py:273-278);
        disk=(R_in, R_out): thin disk in z = 0, first crossing inside the annulus ends the ray with
        FLAG_HIT_DISK and the crossing point in ray_end (checkHitDisk, Limited...py:413-438).
        spheres=[[cx, cy, cz, radius], ...] (at most 8, BH-centred): objects inside the curved region; a ray
        entering one ends there with FLAG_HIT_OBJECT and object_id = its index -- the collision test the
        reference leaves as a stub ("hit = False", RelativisticRenderEngine.py:304-305).

        Returns dict with
            ray_end[..., 6]            position (0:3) and direction (3:6) at the end of each curve
            ray_blackhole_hit[...]     uint8, 1 where the ray ended on the horizon
            flags[...], n_steps[...], n_accepted[...]
            object_id[...]             int8, only with spheres: index of the sphere hit, else -1
            g[...]                     only with redshift=dict(disk_sense=+1 or -1): nu_obs / nu_em of each ray between
                                       the camera's ZAMO and its emitter (disk in Keplerian orbit of that sense, object at
                                       rest, sky at rest at infinity; 0 for horizon rays, NaN for NaN rays), bhg_redshift_host;
                                       with redshift=dict(..., object_motion=dict(velocity=[n][3], angular_velocity=[n][3]))
                                       the spheres move (bhg_redshift_motion_host)
            evpa[...], pol_degree[...], mu_em[...]
                                       only with polarisation=dict(degree=..., disk_sense=..., up=...): the disk ray's
                                       polarisation angle at the camera (from image up towards image left, in (-pi/2, pi/2]),
                                       its degree (the table at mu) and emission cosine; NaN for NaN rays, 0 for every ray
                                       that is not a disk ray (bhg_polarisation_host)
            t_em[...], thermal_rgb[..., 3]
                                       only with disk_thermal=dict(t_peak=..., nu=..., weights=..., f_col=..., scale=...,
                                       disk_sense=...): the disk ray's emitted Novikov-Thorne temperature [K] and the
                                       redshifted blackbody the camera sees, weighed per channel (0 at and inside r_ms; NaN for
                                       NaN rays, 0 for every ray that is not a disk ray; bhg_disk_thermal_host; DESIGN.md
                                       section 13)
        disk_crossings=K (1 .. 4, with disk=; DP5(4), null rays, no spheres): the ray is carried THROUGH the disk and every
        crossing inside the annulus is recorded (bhg_trace_crossings).  ray_end, flags, n_steps and
        n_accepted are then those of the trace with the disk off (no ray has FLAG_HIT_DISK), and the dict also has
            n_cross[...]               uint8, the ray's crossings (all of them, saturating at 255)
            disk_cross[K, ..., 6]      the first K crossing records in order, position and direction; NaN where a ray has none
        and redshift=, polarisation= and disk_thermal= return their arrays per LAYER -- g[K, ...], evpa[K, ...], ...,
        thermal_rgb[K, ..., 3] -- each the per-ray call on disk_cross[m], NaN where a ray has no layer m.
        travel_time=True (DP5(4), null rays, no spheres; bhg_travel_time): the dict also has
            t[...]                     the coordinate time that elapsed along the ray up to ray_end -- the light seen at camera
                                       time t_c left there at t_c - t; +inf for rays that ended in the hole, NaN for NaN rays.
                                       With an opaque disk=: the first crossing's time on rays flagged FLAG_HIT_DISK
            t_cross[K, ...]            with disk_crossings=K: the time of each stored crossing, NaN where a ray has none ("t" is
                                       then the time to the ray's end)
        Every other key comes from the call that makes it without travel_time.
        mesh=Mesh or (vertices [nv, 3], triangles [nt, 3]) (DP5(4), null rays; bhg_trace_mesh): a triangle
        mesh in the curved region, Cartesian and BH-centred.  The ray takes the steps it takes without the mesh; where the curve
        meets a triangle it ends with FLAG_HIT_OBJECT and the dict also has
            tri_id[...]                int32, the triangle hit, -1 for every other ray
            bary[..., 2]               the plane coordinates (u, v) of the hit in that triangle, NaN for every other ray
        mesh_chord (default 0.25 r_s): the length of the straight sub-chords each step is tested in.  Not with spheres=,
        disk_crossings=, travel_time=, redshift=, polarisation= or disk_thermal=.
        mesh_instances=T ([K, 12]: R row-major then t, or [K, 3, 4]: R | t; with mesh=): the mesh stands in
        K rigid placements x_world = R x_local + t instead of where its vertices put it, and the dict also has
            inst_id[...]               int32, the placement hit, -1 for every other ray (tri_id counts within the mesh, bary lies
                                       in the placement's frame)
        mesh_instance_tree=True (with mesh_instances=): the placements lie under a tree of boxes, K may go
        up to 65536, and every output is the linear walk's, bit for bit.
        mesh_build="device" (with mesh=(vertices, triangles)): the mesh's tree is built on the device
        instead of the host; every output is the same, bit for bit.
        """
        if mesh_build not in ("host", "device"):
            raise ValueError('mesh_build must be "host" or "device"')
        if mesh_instances is not None and mesh is None:
            raise ValueError("mesh_instances goes with mesh=")
        if mesh_instance_tree and mesh_instances is None:
            raise ValueError("mesh_instance_tree goes with mesh_instances=")
        if mesh is not None:
            for name, given in (("spheres", spheres is not None), ("disk_crossings", disk_crossings is not None),
                                ("travel_time", bool(travel_time)), ("redshift", redshift is not None),
                                ("polarisation", polarisation is not None), ("disk_thermal", disk_thermal is not None)):
                if given:
                    raise ValueError(f"mesh does not go with {name}")
            return self._trace_mesh(k0, x0, max_step, curve_end, r_exit, disk, mesh, mesh_chord, mesh_instances, mesh_build,
                                    bool(mesh_instance_tree))
        if travel_time and spheres is not None:
            raise ValueError("travel_time does not go with object spheres")
        if disk_crossings is not None:
            return self._trace_crossings(k0, x0, max_step, curve_end, r_exit, disk, spheres, redshift, polarisation, disk_thermal,
                                         int(disk_crossings), travel_time)
        k0 = np.asarray(k0, dtype=np.float64)
        lead = k0.shape[:-1]
        k0f = k0.reshape(-1, 3)
        x0 = np.asarray(x0, dtype=np.float64)
        x0f = x0 if x0.ndim == 1 else x0.reshape(-1, 3)
        obj = None
        if spheres is not None:
            end, flags, steps, acc, obj = self._ctx.trace(k0f, x0f, self.params(max_step, curve_end, r_exit, disk),
                                                          spheres=spheres)
        else:
            end, flags, steps, acc = self._ctx.trace(k0f, x0f, self.params(max_step, curve_end, r_exit, disk))
        out = {
            "ray_end": end.reshape(lead + (6,)),
            "ray_blackhole_hit": ((flags & _ffi.FLAG_HIT_HORIZON) != 0).astype(np.uint8).reshape(lead),
            "flags": flags.reshape(lead),
            "n_steps": steps.reshape(lead),
            "n_accepted": acc.reshape(lead),
        }
        if obj is not None:
            out["object_id"] = obj.reshape(lead)
        if redshift is not None:
            rs = _ffi.make_redshift(apply=(), disk_sense=redshift.get("disk_sense", 1))
            om = redshift.get("object_motion")
            if om is None:
                out["g"] = self._ctx.redshift(k0f, x0f, self.params(max_step, curve_end, r_exit, disk), rs, flags, end).reshape(lead)
            else:
                mo = _ffi.make_object_motion(om.get("velocity"), om.get("angular_velocity"))
                out["g"] = self._ctx.redshift_motion(k0f, x0f, self.params(max_step, curve_end, r_exit, disk), rs, None, mo, spheres,
                                                     flags, end, obj).reshape(lead)
        if polarisation is not None:
            pol = _ffi.make_polarisation(**polarisation)
            chi, deg, mu = self._ctx.polarisation(k0f, x0f, self.params(max_step, curve_end, r_exit, disk), pol, None, flags, end)
            out["evpa"], out["pol_degree"], out["mu_em"] = chi.reshape(lead), deg.reshape(lead), mu.reshape(lead)
        if disk_thermal is not None:
            th = _ffi.make_disk_thermal(**disk_thermal)
            t_em, rgb = self._ctx.disk_thermal(k0f, x0f, self.params(max_step, curve_end, r_exit, disk), th, None, flags, end)
            out["t_em"], out["thermal_rgb"] = t_em.reshape(lead), rgb.reshape(lead + (3,))
        if travel_time:
            # the times of the same rays carried through the disk: the end's, or -- the opaque disk stopped the ray -- the first crossing's
            tt = self._ctx.travel_time(k0f, x0f, self.params(max_step, curve_end, r_exit, disk), 1 if disk else 0)
            t = tt[6]
            if disk:
                t = np.where(flags == _ffi.FLAG_HIT_DISK, tt[7][0], t)
            out["t"] = t.reshape(lead)
        return out

    def _trace_mesh(self, k0, x0, max_step, curve_end, r_exit, disk, mesh, mesh_chord, instances=None, build="host", tree=False):
        """trace(mesh=): a mesh given as arrays lives for this call, and so does the instance set of mesh_instances=."""
        own = not isinstance(mesh, _ffi.Mesh)
        m = _ffi.Mesh(self._ctx, mesh[0], mesh[1], build=build) if own else mesh
        inst = inst_id = None
        try:
            k0 = np.asarray(k0, dtype=np.float64)
            lead = k0.shape[:-1]
            x0 = np.asarray(x0, dtype=np.float64)
            x0f = x0 if x0.ndim == 1 else x0.reshape(-1, 3)
            chord = 0.25 * self.r_s if mesh_chord is None else float(mesh_chord)
            if instances is None:
                end, flags, steps, acc, tri, bary = self._ctx.trace_mesh(k0.reshape(-1, 3), x0f,
                                                                         self.params(max_step, curve_end, r_exit, disk), m, chord)
            else:
                inst = _ffi.MeshInstances(m, instances, tree=tree)
                end, flags, steps, acc, tri, inst_id, bary = self._ctx.trace_mesh_instances(
                    k0.reshape(-1, 3), x0f, self.params(max_step, curve_end, r_exit, disk), inst, chord)
        finally:
            if inst is not None:
                inst.close()
            if own:
                m.close()
        extra = {} if inst_id is None else {"inst_id": inst_id.reshape(lead)}
        return {
            **extra,
            "ray_end": end.reshape(lead + (6,)),
            "ray_blackhole_hit": ((flags & _ffi.FLAG_HIT_HORIZON) != 0).astype(np.uint8).reshape(lead),
            "flags": flags.reshape(lead),
            "n_steps": steps.reshape(lead),
            "n_accepted": acc.reshape(lead),
            "tri_id": tri.reshape(lead),
            "bary": bary.reshape(lead + (2,)),
        }

    def _trace_crossings(self, k0, x0, max_step, curve_end, r_exit, disk, spheres, redshift, polarisation, disk_thermal, K,
                         travel_time=False):
        """trace(disk_crossings=K): the crossings trace, then the per-ray calls layer by layer on cross[m] with the flag array
        n_cross > m ? FLAG_HIT_DISK : FLAG_HIT_HORIZON."""
        if spheres is not None:
            raise ValueError("disk_crossings does not go with object spheres")
        if disk is None:
            raise ValueError("disk_crossings needs disk=(R_in, R_out)")
        if redshift is not None and redshift.get("object_motion") is not None:
            raise ValueError("disk_crossings does not go with object motion")
        k0 = np.asarray(k0, dtype=np.float64)
        lead = k0.shape[:-1]
        k0f = k0.reshape(-1, 3)
        x0 = np.asarray(x0, dtype=np.float64)
        x0f = x0 if x0.ndim == 1 else x0.reshape(-1, 3)
        p = self.params(max_step, curve_end, r_exit, disk)
        if travel_time:
            end, flags, steps, acc, cross, n_cross, t_end, t_cross = self._ctx.travel_time(k0f, x0f, p, K)
        else:
            end, flags, steps, acc, cross, n_cross = self._ctx.trace_crossings(k0f, x0f, p, K)
        out = {
            "ray_end": end.reshape(lead + (6,)),
            "ray_blackhole_hit": ((flags & _ffi.FLAG_HIT_HORIZON) != 0).astype(np.uint8).reshape(lead),
            "flags": flags.reshape(lead),
            "n_steps": steps.reshape(lead),
            "n_accepted": acc.reshape(lead),
            "n_cross": n_cross.reshape(lead),
            "disk_cross": cross.reshape((K,) + lead + (6,)),
        }
        if travel_time:
            out["t"], out["t_cross"] = t_end.reshape(lead), t_cross.reshape((K,) + lead)
        extras = {}
        if redshift is not None:
            rs = _ffi.make_redshift(apply=(), disk_sense=redshift.get("disk_sense", 1))
            extras["g"] = lambda fl, e: (self._ctx.redshift(k0f, x0f, p, rs, fl, e),)
        if polarisation is not None:
            pol = _ffi.make_polarisation(**polarisation)
            extras["evpa", "pol_degree", "mu_em"] = lambda fl, e: self._ctx.polarisation(k0f, x0f, p, pol, None, fl, e)
        if disk_thermal is not None:
            th = _ffi.make_disk_thermal(**disk_thermal)
            extras["t_em", "thermal_rgb"] = lambda fl, e: self._ctx.disk_thermal(k0f, x0f, p, th, None, fl, e)
        for names, call in extras.items():
            names = (names,) if isinstance(names, str) else names
            per_layer = [[] for _ in names]
            for m in range(K):
                has = n_cross > m
                fl = np.where(has, _ffi.FLAG_HIT_DISK, _ffi.FLAG_HIT_HORIZON).astype(np.uint8)
                # (the records a ray does not have are NaN in cross: the calls never read the record of a horizon-flagged ray)
                for dst, arr in zip(per_layer, call(fl, np.ascontiguousarray(cross[m]))):
                    arr = np.array(arr, dtype=np.float64)
                    arr[~has] = np.nan
                    dst.append(arr)
            for name, arrs in zip(names, per_layer):
                a = np.stack(arrs)
                out[name] = a.reshape((K,) + lead + a.shape[2:])
        return out

    # ------------------------------------------------------------------------------------
    def ray_set(self, width, height, samples, fov_x, fov_y, origin, rotation_euler=(0.0, 0.0, 0.0), jitter=None,
                jitter_is_compact=False, pixels=None) -> _ffi.RaySet:
        """The camera rays of a frame generated on the device and kept there (bhg_rays_create): the engine's
        pinhole + jitter formula (RelativisticRenderEngine.py:224-230) evaluated by libbhgeo's ray-generation
        kernel from the MT19937 stream; jitter=None gives pixel centres.  origin is BH-centred."""
        from .raygen import euler_xyz_matrix
        return _ffi.RaySet(self._ctx, width, height, samples, fov_x, fov_y, origin, euler_xyz_matrix(rotation_euler), jitter,
                           jitter_is_compact, pixels)

    def trace_rays(self, rays: _ffi.RaySet, first=0, n=None, max_step=np.inf, curve_end=50.0, r_exit=0.0, disk=None,
                   spheres=None, want=("end_dir", "flags")):
        """Trace rays [first, first + n) of a resident ray set; only the arrays named in `want` come back
        (end, end_loc, end_dir, flags, n_steps, n_accepted, object_id)."""
        return rays.trace(self.params(max_step, curve_end, r_exit, disk), first, n, want, spheres)

    # ------------------------------------------------------------------------------------
    def calc_trajectory(self, k0_xyz, x0_xyz, max_step=np.inf, curve_end=50, nr_points_curve=50,
                        verbose=False, r_exit=0.0, disk=None, spheres=None, **_ignored):
        """Per-ray drop-in for the call at RelativisticRenderEngine.py:293-294.

        Returns (k_xyz, x_xyz, result): k_xyz and x_xyz have shape (3, T') with the curve sampled at
        t_eval = linspace(0, curve_end, nr_points_curve) up to where the ray ends (T' <= nr_points_curve,
        as solve_ivp's t_eval gives), so that `x, y, z = x_xyz` (:299) and `x[-1]` (:307-308) work as
        in the reference.  result['end_loc'] / ['end_dir'] carry the exact end state (the event root for
        horizon rays), the same numbers trace() returns.  r_exit / disk=(R_in, R_out) (not in the reference's signature:
        the Limited engine's exit sphere and thin disk, Limited...py:273-278, :413-438): the curve then ends where the
        ray leaves the sphere or meets the disk, result['hit_disk'] says which.
        spheres=[[cx, cy, cz, radius], ...] (BH-centred, at most 8): objects in the curved region -- this call is exactly
        where the reference left its collision test as a stub ("NOW YOU DO COLLISION DETECTION ... hit = False", :304-305).
        A ray that enters a sphere ends there: result['hit_object'] = True, result['object_id'] = its index,
        result['end_loc'] the entry point -- the same flag, sphere and point trace(spheres=) gives for that ray -- and the
        sampled curve stops in front of it.
        """
        k0 = np.asarray(k0_xyz, dtype=np.float64).reshape(3)
        x0 = np.asarray(x0_xyz, dtype=np.float64).reshape(3)
        n_pts = max(2, int(nr_points_curve))
        obj = None
        if spheres is not None:
            traj, nv, end, flags, obj = self._ctx.trajectory(k0[None, :], x0, self.params(max_step, curve_end, r_exit, disk), n_pts,
                                                             spheres=spheres)
        else:
            traj, nv, end, flags = self._ctx.trajectory(k0[None, :], x0, self.params(max_step, curve_end, r_exit, disk), n_pts)
        m = int(nv[0])
        fl = int(flags[0])
        # (views of this call's own result block -- nothing else refers to it: two 240-kB copies less per call at the
        # engine's nr_points_curve = 10000)
        x_xyz = traj[0, 0:3, :m]
        k_xyz = traj[0, 3:6, :m]
        result = {
            "start_inside_hole": bool(fl & _ffi.FLAG_START_INSIDE),
            "hit_blackhole": bool(fl & _ffi.FLAG_HIT_HORIZON),
            "hit_disk": fl == _ffi.FLAG_HIT_DISK,
            "flags": fl,
            "end_loc": end[0, 0:3].copy(),
            "end_dir": end[0, 3:6].copy(),
        }
        if obj is not None:
            result["hit_object"] = fl == _ffi.FLAG_HIT_OBJECT
            result["object_id"] = int(obj[0])
        if verbose or self.verbose:
            print("calc_trajectory:", {k: result[k] for k in ("start_inside_hole", "hit_blackhole", "flags")})
        return k_xyz, x_xyz, result

class GeodesicIntegratorKerr(GeodesicIntegratorSchwarzschild):
    """Null geodesics around a Kerr black hole (BASELINE.json config 5).

    The reference lists Kerr as a goal (README.md:218) and its pre-traced camera takes `a = 0.9`
    (raytracer/RelativisticRenderEngineCamEdition.py:210, :217); with mass 0.5 that can only be the
    dimensionless spin a/M, which is what `a` means here.  Same boundary as the Schwarzschild
    integrator: Cartesian k0 / x0 in, Cartesian end state out; integrated in Boyer-Lindquist
    coordinates with sympy-derived Christoffel symbols (tools/gen_kerr_rhs.py)."""

    def __init__(self, mass=1.0, a=0.0, time_like=False, verbose=False, **kw):
        kw.pop("rhs_form", None)
        super().__init__(mass=mass, time_like=time_like, verbose=verbose, rhs_form="kerr_bl", **kw)
        if not abs(a) < 1.0:
            raise ValueError("|a| = |J|/M^2 must be < 1")
        self.a = float(a)
        self.spin = self.a * self.mass
        self.r_plus = self.mass + (self.mass**2 - self.spin**2) ** 0.5

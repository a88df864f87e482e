"""Blender add-on: the reference's render-engine plugin surface over the MI355X integrator.

The plugin surface is unchanged with respect to raytracer/RelativisticRenderEngine.py -- the
engine id ("RelRenEn", :42), the `render(self, depsgraph)` entry (:50), the result protocol
(begin_result / layer.rect / update_result / update_progress / end_result, :158-168), the
"Blackhole Settings" panel (:466-495), the twelve scene properties with their names and defaults
(:504-517) and register()/unregister() (:537-580).  What changes is the per-ray hand-off: instead
of one `curvedpy ... calc_trajectory` Python call per ray (:293-294) the frame driver issues one
batched GPU trace per sample (frame.FrameTracer), shading stays Blender's `Texture.evaluate`.

This module imports `bpy`; it is loaded by Blender (or by the tests' fake-bpy harness), never by
the package __init__.

Known deviations from the reference, all deliberate:
  * progress: the reference divides the already-fractional progress by res_y again (:166 vs
    :261, so its bar stays near 0); here update_progress receives the fraction itself;
  * the RenderResult is refreshed once per sample instead of once per row (`buf.tolist()` per row
    is O(H^2 W) Python work, :163); the final image is identical;
  * one scene property more than the reference's twelve: `curved_space_objects` (default 0 = off).  Off, the
    image is the reference's: its spacetime_ray_cast always reports hit = False (:304-305), so scene meshes
    never affect a render.  Set to 1, the MESH objects of the scene (except the black-hole marker) are traced as
    lamp-lit bounding spheres inside the curved region -- the collision test the reference leaves as a stub;
    at most 8 (the solver's limit), the nearest to the hole, with a warning when more are dropped.  ONE lighting
    contract for an object hit, whichever path shades it: `spacetime_hit`'s Lambert lamps (:341-363) -- colour +=
    intensity^2 n.l / d^2 per lamp, light paths straight, n.l clamped at 0 -- WITH its shadow rays (:352-356), cast
    against the other traced spheres (the only geometry the curved region knows); the host routine below and the
    device kernel (`object_colour`, csrc/frame_kernels.hip; restated in oracle/shade_reference.py) agree to rounding;
  * a second extra property, `device_shading` (default 0 = off).  Off: every escaping ray is shaded by Blender's own
    `Texture.evaluate`, one Python call per ray as in the reference (:366-378) -- at 1024 x 1024 that is a million
    calls per sample next to a quarter-millisecond trace.  Set to 1: the sky image's pixels are read ONCE
    (`bpy.data.images[...].pixels`), uploaded, and ray generation, trace, sky lookup, object lighting and the
    multisample mean all run on the device (device_frame.DeviceFrame: bhg_raygen_device -> bhg_trace[_dir]_device ->
    bhg_shade[_dir/_scene]_device); one array comes back per frame.  The lookup is then the library's bilinear
    filter of the image, not Blender's texture filter (which cannot be reproduced outside Blender): the images agree
    to the filter difference.  Needs the whole frame (no mark_* window: the window's RNG alignment is a host matter);
    with a window set the host path is used.
  * textured, oriented and emissive objects (with `curved_space_objects` on): a traced mesh object
    reads two custom properties -- `curved_space_texture`, the name of a `bpy.data.images` image wrapped on its sphere
    (equirectangular, body +x the image's centre column, body +z its top row), and `curved_space_emission`, a float: above
    0 the object glows with that strength (no lamps, no shadows: the reference's `emission` branch, :331-339), 0 or absent
    it is lamp-lit with the texture as albedo.  Its orientation is the rotation part of `matrix_world` (columns normalised).
    The host path reads the texture through a `bpy.data.textures` IMAGE texture's `evaluate((U, V, 0))`, as it shades the
    sky; the device path uploads the image's pixels once (bhg_frame_set_object_textures) and turns the sphere per frame by
    kernel argument.  The reference's literal mapping (arctan(n_y/n_x), read at (ph/2pi, th/pi)) folds the two
    x-hemispheres and reads a quarter of the image: deliberately not reproduced.  A scene without these properties renders
    exactly as before.
  * scene.curved_space_meshes (default 0): with the device path, every mesh object but the black-hole
    marker is traced as its TRIANGLES, not as its bounding sphere -- the evaluated mesh's loop_triangles through matrix_world,
    the active UV layer per corner, `curved_space_texture` as the image on those UVs (at most 8 distinct images),
    the largest `curved_space_emission` as the mesh's emission, smooth shading when every polygon is smooth
    (bhg_frame_set_mesh; the mesh is uploaded only when it changed).  On the host path or with a mark_* window: one warning,
    and the render as with 0.
  * scene.curved_space_mesh_instances (default 0): with curved_space_meshes = 1 on the device path, traced
    mesh objects that share ONE mesh datablock (or a single object), whose matrix_world is a rotation times one common per-axis
    scale (to 1e-6) and that agree in `curved_space_texture` and `curved_space_emission`, are rigid instances of one mesh: the
    frame gets the datablock once, in its own coordinates with the scale baked in, and one instance per object (translation minus
    the hole's location).  A later render whose baked arrays and images are the ones held only moves the instances
    (bhg_frame_set_mesh_instances: nothing is rebuilt or uploaded).  Any other scene takes the concatenated path above, silently.
  * scene.curved_space_mesh_instance_tree (default 0): together with curved_space_mesh_instances, the
    instances lie under a tree of boxes (bhg_frame_set_mesh_instance_tree) and the rule above holds for up to 65536 objects:
    more than 64 linked duplicates no longer take the concatenated path.  Off, everything is as without the property.
  * scene.curved_space_mesh_refit (default 0): with curved_space_meshes = 1 on the device path, a render whose
    mesh differs from the one the frame holds in vertex positions only -- the triangle indices, UVs, images and emission the same
    bits, the vertex count the same -- sends the vertices alone and every device refits its tree on the device
    (bhg_frame_refit_mesh): an armature, a shape key, cloth, a wave modifier.  This holds for the concatenated mesh and for the
    single datablock of curved_space_mesh_instances alike.  Anything else takes the full path above, silently.
  * scene.curved_space_mesh_build (default 0): with curved_space_meshes = 1 on the device path, the frame's
    devices build their trees themselves (bhg_frame_set_mesh_build), and a render whose triangle list, vertex count or UVs
    changed -- a fluid surface, a boolean, a remesher, animated subdivision -- rebuilds the mesh each device holds in place where
    its counts fit, instead of building a new tree on the host.  curved_space_mesh_refit keeps deciding the vertices-only case.
    The images are those of 0, bit for bit.
"""
import warnings
import os

import bpy
import numpy as np
from bl_ui.properties_render import RenderButtonsPanel
from bpy.types import Panel

from .frame import FrameTracer, equirect_uv
from .integrator import GeodesicIntegratorSchwarzschild

bl_info = {
    "name": "Relativistic Render Engine (MI355X)",
    "bl_label": "Relativistic Render Engine",
    "blender": (4, 1, 0),
    "category": "Render",
}


def _unset(value, default):
    """-1 is the reference's "unset" sentinel for scene properties (:59-60, :111-118)."""
    return default if value == -1 else value


class RelativisticRenderEngine(bpy.types.RenderEngine):
    bl_idname = "RelRenEn"
    bl_label = "Relativistic"
    bl_use_preview = True

    # ---- Blender entry point (:50) -----------------------------------------------------------
    def render(self, depsgraph):
        scene = depsgraph.scene
        self.max_integration_step = _unset(scene.max_integration_step, np.inf)
        self.sampling_seed = scene.sampling_seed
        self.int_depth_curve_end = scene.integration_depth

        self.samples = bpy.data.scenes["Scene"].eevee.taa_render_samples
        self.scale = scene.render.resolution_percentage / 100.0
        self.res_x = int(scene.render.resolution_x * self.scale)
        self.res_y = int(scene.render.resolution_y * self.scale)
        self.field_of_view_x = scene.field_of_view_x
        self.field_of_view_y = scene.field_of_view_y

        self._load_sky(scene.sky_image)

        self.mass = scene.mass
        bh = scene.blackhole_obj
        self.bh_loc = np.zeros(3) if bh is None else np.array(list(bh.location), dtype=np.float64)

        self.mark_y_min = _unset(scene.mark_y_min, 0)
        self.mark_y_max = _unset(scene.mark_y_max, self.res_y)
        self.mark_x_min = _unset(scene.mark_x_min, 0)
        self.mark_x_max = _unset(scene.mark_x_max, self.res_x)
        self.device_shading = float(getattr(scene, "device_shading", 0) or 0) != 0.0
        self.render_devices = int(float(getattr(scene, "render_devices", 1) or 1))

        # one solver object per frame, as the reference builds it (:134)
        self.GeoInt = GeodesicIntegratorSchwarzschild(mass=self.mass, time_like=False, verbose=False)

        # the reference refreshes the depsgraph so that "-f <frame>" renders work (:140-141)
        depsgraph = bpy.context.evaluated_depsgraph_get()
        depsgraph.update()

        if not self.is_preview:
            self.render_scene(depsgraph)

    def _load_sky(self, path):
        self.sky_image_path = path
        name = os.path.basename(path)
        self.sky_tex_name = name + "_tex"
        if name and name not in bpy.data.images:
            bpy.data.images.load(path)
        if name and self.sky_tex_name not in bpy.data.textures:
            tex = bpy.data.textures.new(self.sky_tex_name, "IMAGE")
            tex.image = bpy.data.images[name]

    # ---- result hand-back (:152-168) ---------------------------------------------------------
    def render_scene(self, depsgraph):
        buf = np.ones((self.res_y, self.res_x, 4))
        result = self.begin_result(0, 0, self.res_x, self.res_y)
        layer = result.layers[0].passes["Combined"]
        rows_per_refresh = max(1, self.res_y)
        for i, frac in enumerate(self.ray_trace(depsgraph, self.res_x, self.res_y, 1, buf, self.samples)):
            self.update_progress(frac)
            if (i + 1) % rows_per_refresh == 0:
                self._set_rect(layer, buf)
                self.update_result(result)
        self._set_rect(layer, buf)
        self.update_result(result)
        self.end_result(result)

    @staticmethod
    def _set_rect(layer, buf):
        """layer.rect <- buf [H, W, 4]: ONE flat float32 array through foreach_set where the pass offers it (Blender's
        bpy_prop_array does), else the reference's list of rows (:163; a million-pixel .tolist() is a second of Python)."""
        rect = getattr(layer, "rect", None)
        if rect is not None and hasattr(rect, "foreach_set"):
            rect.foreach_set(np.ascontiguousarray(buf, dtype=np.float32).reshape(-1))
        else:
            layer.rect = buf.reshape(-1, 4).tolist()

    # ---- frame driver (:172-267): same generator protocol, batched hot path -------------------
    def ray_trace(self, depsgraph, width, height, depths, buf, samples, approx=False):
        cam = depsgraph.scene.camera.matrix_world
        origin = np.array(list(cam.translation), dtype=np.float64)
        rotation = tuple(cam.to_euler())
        mark = None
        if (self.mark_y_min, self.mark_y_max, self.mark_x_min, self.mark_x_max) != (0, height, 0, width):
            mark = (self.mark_y_min, self.mark_y_max, self.mark_x_min, self.mark_x_max)
        self.lamps = [ob for ob in depsgraph.scene.objects if ob.type == "LIGHT"]  # :175
        # objects in the curved region are opt-in (scene.curved_space_objects): off reproduces the reference image
        want_objects = float(getattr(depsgraph.scene, "curved_space_objects", 0) or 0) != 0.0
        spheres = self.scene_spheres(depsgraph) if want_objects else np.zeros((0, 4))
        self._lit_spheres = spheres
        self._sphere_looks = self.sphere_looks() if want_objects else []
        on_device = getattr(self, "device_shading", False) and mark is None
        # mesh objects as their triangles (scene.curved_space_meshes): the device path only
        want_meshes = float(getattr(depsgraph.scene, "curved_space_meshes", 0) or 0) != 0.0
        if want_meshes and not on_device:
            warnings.warn("curved_space_meshes needs the device path (device_shading = 1 and no mark_* window): rendering as with "
                          "curved_space_meshes = 0", RuntimeWarning)
            want_meshes = False
        if on_device:
            mesh = None
            if want_meshes:
                # (a mesh does not go with object spheres: every mesh object is its triangles now)
                spheres, self._lit_spheres, self._sphere_looks = np.zeros((0, 4)), np.zeros((0, 4)), []
                mesh = self.scene_mesh(depsgraph)
            yield from self.ray_trace_device(width, height, samples, buf, origin, rotation, spheres, mesh=mesh)
            return
        tracer = FrameTracer(
            self.GeoInt, width, height, samples, fov_x=self.field_of_view_x, fov_y=self.field_of_view_y,
            sampling_seed=self.sampling_seed, origin=origin, rotation_euler=rotation, bh_loc=self.bh_loc,
            max_step=self.max_integration_step, curve_end=self.int_depth_curve_end, mark=mark,
            spheres=spheres if len(spheres) else None, object_hit=self.spacetime_hit_many)
        yield from tracer.ray_trace(buf, self.background_hit_many)

    # ---- objects in the curved region: the collision test the reference leaves as a stub (:304-305) ----
    def scene_spheres(self, depsgraph):
        """Mesh objects of the scene as bounding spheres [[x, y, z, radius]] in world coordinates (the
        README's orbiting-sphere animation, README.md:9-13, uses a UV sphere); the black-hole marker object
        is skipped.  At most 8 (the solver's limit), the nearest to the hole first."""
        bh = getattr(depsgraph.scene, "blackhole_obj", None)
        out = []
        for ob in depsgraph.scene.objects:
            if ob.type != "MESH" or ob is bh:
                continue
            loc = np.array(list(ob.location), dtype=np.float64)
            radius = 0.5 * max(float(d) for d in ob.dimensions)
            if radius > 0.0:
                out.append(([loc[0], loc[1], loc[2], radius], ob))
        out.sort(key=lambda s: float(np.linalg.norm(np.array(s[0][:3]) - self.bh_loc)))
        if len(out) > 8:
            warnings.warn(f"{len(out)} mesh objects in the scene: only the 8 nearest to the hole are traced", RuntimeWarning)
        self._sphere_objects = [ob for _, ob in out[:8]]
        return np.array([sp for sp, _ in out[:8]], dtype=np.float64).reshape(-1, 4)

    MESH_IMAGES_MAX = 8      # _ffi.MESH_TEXTURES_MAX: image slots of a mesh material

    @staticmethod
    def _evaluated_geometry(ob, depsgraph):
        """(co [nv * 3] float32, triangles [nt * 3] int32) of the object's evaluated mesh, in its own coordinates."""
        ev = ob.evaluated_get(depsgraph) if hasattr(ob, "evaluated_get") else ob
        me = ev.to_mesh()
        try:
            me.calc_loop_triangles()
            co = np.empty(len(me.vertices) * 3, dtype=np.float32)
            me.vertices.foreach_get("co", co)
            tri = np.empty(len(me.loop_triangles) * 3, dtype=np.int32)
            me.loop_triangles.foreach_get("vertices", tri)
            return co, tri
        finally:
            if hasattr(ev, "to_mesh_clear"):
                ev.to_mesh_clear()

    def _mesh_instance_plan(self, depsgraph, objects):
        """(scale [3], records [K, 12]) when the traced mesh objects are rigid instances of one mesh (scene.curved_space_mesh_instances;
        the module docstring has the rule), else None.  A record is the rigid part of matrix_world nearest to it
        (_ffi.rigid_transform: Blender's matrices are float32) with the hole's location taken off the translation."""
        from . import _ffi
        tree = float(getattr(depsgraph.scene, "curved_space_mesh_instance_tree", 0) or 0) != 0.0
        if not objects or len(objects) > (_ffi.MESH_INSTANCE_TREE_MAX if tree else _ffi.MESH_INSTANCES_MAX):
            return None
        data = [getattr(ob, "data", None) for ob in objects]
        if len(objects) > 1 and (data[0] is None or any(d is not data[0] for d in data)):
            return None
        looks = {(str(self._custom(ob, "curved_space_texture") or ""), float(self._custom(ob, "curved_space_emission") or 0.0))
                 for ob in objects}
        if len(looks) != 1:
            return None
        # linked duplicates may carry modifiers of their own: the EVALUATED meshes have to be one mesh too
        first = self._evaluated_geometry(objects[0], depsgraph)
        for ob in objects[1:]:
            other = self._evaluated_geometry(ob, depsgraph)
            if any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(first, other)):
                return None
        scale, records = None, []
        for ob in objects:
            ev = ob.evaluated_get(depsgraph) if hasattr(ob, "evaluated_get") else ob
            mw = np.array([[float(ev.matrix_world[i][k]) for k in range(4)] for i in range(4)], dtype=np.float64)
            s = np.linalg.norm(mw[:3, :3], axis=0)
            if not np.all(s > 0.0):
                return None
            R = mw[:3, :3] / s
            if np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or not np.linalg.det(R) > 0.0:
                return None
            if scale is None:
                scale = s
            elif np.abs(s - scale).max() > 1e-6 * scale.max():
                return None
            rigid = np.eye(4)
            rigid[:3, :3], rigid[:3, 3] = R, mw[:3, 3] - self.bh_loc
            records.append(_ffi.rigid_transform(rigid))
        return scale, np.stack(records)

    def scene_mesh(self, depsgraph):
        """Every MESH object of the scene but the black-hole marker as ONE triangle mesh, BH-centred (scene.curved_space_meshes):
        dict(vertices [nv, 3] float64, triangles [nt, 3] int32, normals [nv, 3] or None, tri_uv [nt, 3, 2] float32 or None,
        tri_tex [nt] int32, images: the slots' bpy.data.images names, emission, offsets: per object (first vertex, first
        triangle)); None without triangles.  Geometry is the evaluated object's: calc_loop_triangles(), loop_triangles
        (.vertices, .loops), vertices[].co through matrix_world; UVs uv_layers.active.data[loop].uv per corner -- all read with
        foreach_get into numpy buffers.  tri_tex is the slot of the object's curved_space_texture image (-1: none; at most 8
        distinct images), emission the largest curved_space_emission; vertex normals are passed only when every polygon of
        every object is smooth.  With scene.curved_space_mesh_instances on and objects that are rigid instances of one mesh
        (_mesh_instance_plan): that mesh once, in its own coordinates with the common scale baked in, and instances [K, 12], the
        objects' placements; otherwise instances is None."""
        bh = getattr(depsgraph.scene, "blackhole_obj", None)
        V, F, N, UV, TEX, offsets, images = [], [], [], [], [], [], []
        emission, smooth, any_uv, nv, nt, dropped = 0.0, True, False, 0, 0, 0
        objects = [ob for ob in depsgraph.scene.objects if ob.type == "MESH" and ob is not bh]
        plan = None
        if float(getattr(depsgraph.scene, "curved_space_mesh_instances", 0) or 0) != 0.0:
            plan = self._mesh_instance_plan(depsgraph, objects)
        for ob in objects[:1] if plan is not None else objects:
            ev = ob.evaluated_get(depsgraph) if hasattr(ob, "evaluated_get") else ob
            me = ev.to_mesh()
            try:
                me.calc_loop_triangles()
                n_v, n_t = len(me.vertices), len(me.loop_triangles)
                if n_v == 0 or n_t == 0:
                    continue
                co = np.empty(n_v * 3, dtype=np.float32)
                me.vertices.foreach_get("co", co)
                tri = np.empty(n_t * 3, dtype=np.int32)
                me.loop_triangles.foreach_get("vertices", tri)
                mw = np.array([[float(ev.matrix_world[i][k]) for k in range(4)] for i in range(4)], dtype=np.float64)
                co = co.reshape(n_v, 3).astype(np.float64)
                # into the world about the hole, or (instances place it) the datablock's own coordinates with the scale baked in
                A = mw[:3, :3] if plan is None else np.diag(plan[0])
                V.append(co @ A.T + mw[:3, 3] - self.bh_loc if plan is None else co @ A.T)
                local_co = co
                F.append(tri.reshape(n_t, 3) + nv)
                flags = np.empty(len(me.polygons), dtype=bool)
                me.polygons.foreach_get("use_smooth", flags)
                smooth = smooth and bool(flags.all())
                nrm = np.empty(n_v * 3, dtype=np.float32)
                me.vertices.foreach_get("normal", nrm)
                # (normals go with the inverse transpose; the kernel normalises them)
                local_nrm = nrm.reshape(n_v, 3).astype(np.float64)
                N.append(local_nrm @ np.linalg.inv(A))
                uv = np.zeros((n_t, 3, 2), dtype=np.float32)
                slot = -1
                layer = getattr(getattr(me, "uv_layers", None), "active", None)
                name = self._custom(ob, "curved_space_texture")
                name = str(name) if name else None
                if name is not None and name not in bpy.data.images:
                    warnings.warn(f"curved_space_texture {name!r}: no such image in bpy.data.images (the object stays untextured)",
                                  RuntimeWarning)
                    name = None
                if layer is not None and name is not None:
                    loops = np.empty(n_t * 3, dtype=np.int32)
                    me.loop_triangles.foreach_get("loops", loops)
                    luv = np.empty(len(layer.data) * 2, dtype=np.float32)
                    layer.data.foreach_get("uv", luv)
                    uv = luv.reshape(-1, 2)[loops].reshape(n_t, 3, 2)
                    if name in images:
                        slot = images.index(name)
                    elif len(images) < self.MESH_IMAGES_MAX:
                        images.append(name)
                        slot = len(images) - 1
                    else:
                        dropped += 1
                    any_uv = any_uv or slot >= 0
                UV.append(uv)
                TEX.append(np.full(n_t, slot, dtype=np.int32))
                emission = max(emission, float(self._custom(ob, "curved_space_emission") or 0.0))
                offsets.append((nv, nt))
                nv, nt = nv + n_v, nt + n_t
            finally:
                if hasattr(ev, "to_mesh_clear"):
                    ev.to_mesh_clear()
        if dropped:
            warnings.warn(f"more than {self.MESH_IMAGES_MAX} distinct curved_space_texture images: {dropped} object(s) stay "
                          "untextured", RuntimeWarning)
        if nt == 0:
            return None
        return {"vertices": np.concatenate(V), "triangles": np.concatenate(F).astype(np.int32),
                "normals": np.concatenate(N) if smooth else None,
                "tri_uv": np.ascontiguousarray(np.concatenate(UV)) if any_uv else None, "tri_tex": np.concatenate(TEX),
                "images": images if any_uv else [], "emission": emission, "offsets": offsets,
                "instances": None if plan is None else plan[1],
                "instance_tree": float(getattr(depsgraph.scene, "curved_space_mesh_instance_tree", 0) or 0) != 0.0,
                "refit": float(getattr(depsgraph.scene, "curved_space_mesh_refit", 0) or 0) != 0.0,
                "build": float(getattr(depsgraph.scene, "curved_space_mesh_build", 0) or 0) != 0.0,
                # (instanced: the datablock's arrays before the scale, and the scale -- what _set_device_mesh compares)
                "local": None if plan is None else {"co": local_co, "normals": local_nrm, "scale": plan[0]}}

    def _set_device_mesh(self, fr, mesh):
        """The scene's mesh on the library-owned frame: set_mesh only when vertices, triangles, normals or the material differ
        from what the frame holds (images by _image_identity) -- an animation of a static mesh uploads nothing."""
        held = getattr(fr, "mesh_held", None)
        if mesh is None:
            if held is not None:
                fr.set_mesh(None)
            fr.mesh_held = None
            return
        ids = [self._image_identity(n) for n in mesh["images"]]
        # An instanced mesh is its datablock's arrays times the objects' common scale.  The scale is read off float32 matrices and
        # moves in its last digits from render to render, so the baked arrays do too: a held instanced mesh is the one wanted when
        # the arrays BEFORE the scale are the same bits and the scale is the held one to the rule's own 1e-6 (the tolerance within
        # which the objects' scales count as one).  Any change of the datablock itself, however small, is a new mesh.
        local, held_local = mesh.get("local"), None if held is None else held.get("local")
        rescaled = local is not None and held_local is not None and np.array_equal(local["co"], held_local["co"]) and \
            np.array_equal(local["normals"], held_local["normals"]) and \
            np.abs(local["scale"] - held_local["scale"]).max() <= 1e-6 * held_local["scale"].max()

        def same_array(key, a, b):
            return (rescaled and key in ("vertices", "normals")) or np.array_equal(a, b)

        same = held is not None and all(i is not None for i in ids) and ids == held["ids"] and \
            mesh["emission"] == held["emission"] and \
            all((mesh[k] is None) == (held[k] is None) and (mesh[k] is None or same_array(k, mesh[k], held[k]))
                for k in ("vertices", "triangles", "normals", "tri_uv", "tri_tex"))
        # scene.curved_space_mesh_refit: everything but the vertex positions is what the frame holds -- the
        # triangle indices, UVs, images and emission the same bits, the vertex count the same -- and a coordinate differs: the new
        # vertices (and normals) go to the frame, whose devices refit their trees; the instances stay and the frame re-sets them
        refit = not same and bool(mesh.get("refit")) and held is not None and all(i is not None for i in ids) and \
            ids == held["ids"] and mesh["emission"] == held["emission"] and mesh["vertices"].shape == held["vertices"].shape and \
            (mesh["normals"] is None) == (held["normals"] is None) and \
            all((mesh[k] is None) == (held[k] is None) and (mesh[k] is None or np.array_equal(mesh[k], held[k]))
                for k in ("triangles", "tri_uv", "tri_tex")) and \
            not same_array("vertices", mesh["vertices"], held["vertices"])
        # scene.curved_space_mesh_build: the frame's devices build their trees themselves, and a mesh whose
        # triangle list, vertex count or UVs changed goes into the mesh they hold, in place, where its counts fit -- "rebuild";
        # curved_space_mesh_refit keeps deciding the vertices-only case above
        build = bool(mesh.get("build"))
        self.device_mesh_action = "kept" if same else "refit" if refit else "rebuild" if build and held is not None else "set"
        if refit:
            from . import _ffi
            fr.refit_mesh(mesh["vertices"], mesh["normals"], rebuild_ratio=_ffi.MESH_REBUILD_RATIO)
            fr.mesh_held.update(vertices=mesh["vertices"], normals=mesh["normals"], local=local)
        elif not same:
            from . import _ffi
            material = _ffi.MeshMaterial(tri_uv=mesh["tri_uv"], tri_tex=mesh["tri_tex"] if mesh["tri_uv"] is not None else None,
                                         textures=[self._image_pixels(n) for n in mesh["images"]], emission=mesh["emission"])
            if build != getattr(fr, "mesh_build_on", False):     # (the frame's default is off: a scene without the switch calls nothing)
                fr.set_mesh_build(build)
                fr.mesh_build_on = build
            fr.set_mesh(mesh["vertices"], mesh["triangles"], vertex_normals=mesh["normals"], material=material)
            fr.mesh_held = {**{k: mesh[k] for k in ("vertices", "triangles", "normals", "tri_uv", "tri_tex", "emission")}, "ids": ids,
                            "instances": None, "local": local}      # (set_mesh turns instances off)
        # the placements: moved objects of a held mesh upload their records and nothing else
        # (scene.curved_space_mesh_instance_tree: under a tree of boxes; the other kind of set is a new set)
        inst, held_inst = mesh.get("instances"), fr.mesh_held.get("instances")
        tree = bool(mesh.get("instance_tree")) and inst is not None
        if inst is None:
            if held_inst is not None:
                fr.set_mesh_instances(None)
        elif held_inst is None or tree != bool(fr.mesh_held.get("instance_tree")) or not np.array_equal(inst, held_inst):
            if tree:
                fr.set_mesh_instances(inst, tree=True)
            else:
                fr.set_mesh_instances(inst)
        fr.mesh_held["instances"] = inst
        fr.mesh_held["instance_tree"] = tree

    @staticmethod
    def _custom(ob, key):
        """A custom property of a Blender ID (ob["key"]), None when absent."""
        get = getattr(ob, "get", None)
        return get(key) if callable(get) else None

    @staticmethod
    def _orientation(ob):
        """The rotation part of ob.matrix_world (body -> world, row-major) with its columns normalised to remove the scale;
        the all-zero matrix (the identity by the library's convention) when there is none."""
        mw = getattr(ob, "matrix_world", None)
        if mw is None:
            return np.zeros((3, 3))
        m = np.array([[float(mw[i][k]) for k in range(3)] for i in range(3)], dtype=np.float64)
        norms = np.linalg.norm(m, axis=0)
        return m / norms if np.all(norms > 0.0) else np.zeros((3, 3))

    def sphere_looks(self):
        """Per traced sphere (scene_spheres' order): {"image": bpy.data.images name or None, "emission": float, "rot": 3x3} from
        the custom properties curved_space_texture / curved_space_emission and the object's matrix_world."""
        looks = []
        for ob in getattr(self, "_sphere_objects", []):
            name = self._custom(ob, "curved_space_texture")
            name = str(name) if name else None
            if name is not None and name not in bpy.data.images:
                warnings.warn(f"curved_space_texture {name!r}: no such image in bpy.data.images (the object stays untextured)",
                              RuntimeWarning)
                name = None
            emission = float(self._custom(ob, "curved_space_emission") or 0.0)
            looks.append({"image": name, "emission": max(emission, 0.0), "rot": self._orientation(ob)})
        return looks

    def _object_texture(self, image_name):
        """The bpy.data.textures IMAGE texture of an object image (made once, as the sky's, :111-112)."""
        tex_name = image_name + "_tex"
        if tex_name not in bpy.data.textures:
            tex = bpy.data.textures.new(tex_name, "IMAGE")
            tex.image = bpy.data.images[image_name]
        return bpy.data.textures[tex_name]

    LAMP_INTENSITY = 10.0   # spacetime_hit's default `intensity` (:317)

    def spacetime_hit_many(self, loc, normal, index, intensity=None):
        """Vectorised spacetime_hit (:317-363): white Lambert lamps, colour += intensity^2 n.l / d^2, n.l clamped at 0,
        light paths straight, shadow rays (:352-356) cast against the OTHER traced spheres (world coordinates) -- the
        same model, term for term, as the device kernel's object_colour.  loc, normal [n, 3]; index [n] = sphere hit."""
        intensity = self.LAMP_INTENSITY if intensity is None else intensity
        loc = np.asarray(loc, dtype=np.float64).reshape(-1, 3)
        normal = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
        index = np.asarray(index).reshape(-1)
        spheres = np.asarray(getattr(self, "_lit_spheres", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4)
        color = np.zeros(loc.shape)
        for lamp in getattr(self, "lamps", []):
            light_vec = np.array(list(lamp.location), dtype=np.float64) - loc
            d2 = (light_vec * light_vec).sum(-1)
            dist = np.sqrt(d2)
            light_dir = light_vec / dist[:, None]
            ndl = (normal * light_dir).sum(-1)
            lit = ndl > 0.0
            for q in range(len(spheres)):
                oc = loc - spheres[q, 0:3]
                b = (oc * light_dir).sum(-1)
                disc = b * b - ((oc * oc).sum(-1) - spheres[q, 3] ** 2)
                sd = np.sqrt(np.maximum(disc, 0.0))
                t0, t1 = -b - sd, -b + sd
                blocked = (disc > 0.0) & (((t0 > 1e-5) & (t0 < dist)) | ((t0 <= 1e-5) & (t1 > 1e-5))) & (index != q)
                lit &= ~blocked
            color += np.where(lit, intensity * intensity * ndl / d2, 0.0)[:, None]
        # textured / emissive objects: texel at the body-frame normal's angles
        for j, look in enumerate(getattr(self, "_sphere_looks", [])):
            m = index == j
            if not m.any() or (look["image"] is None and not look["emission"] > 0.0):
                continue
            texel = np.ones((int(m.sum()), 3))
            if look["image"] is not None:
                R = look["rot"] if look["rot"].any() else np.eye(3)
                nb = normal[m] @ R                                      # R^T n, row by row
                U = np.arctan2(nb[:, 1], nb[:, 0]) / np.pi
                V = 1.0 - 2.0 * np.arctan2(np.hypot(nb[:, 0], nb[:, 1]), nb[:, 2]) / np.pi
                tex = self._object_texture(look["image"])
                texel = np.array([tex.evaluate((float(u), float(v), 0)).xyz for u, v in zip(U, V)], dtype=np.float64)
            color[m] = look["emission"] * texel if look["emission"] > 0.0 else color[m] * texel
        return color

    # ---- the whole frame on the device (opt-in, scene.device_shading) ------------------------------------------------
    SKY_CHECKSUM_SAMPLES = 1024      # pixel values read for the identity's checksum (of w * h * 4)

    def _sky_identity(self):
        """What tells one sky image's CONTENT from another's without reading all of its pixels (33 MB for a 2k x 1k image):
        name, size, file path -- and what moves when the content does: the file's mtime and length (an image edited
        outside Blender and reloaded keeps name, size and path, and `is_dirty` stays False), the image source with the
        scene's current frame for sequences and movies, the colour space and alpha mode, and a checksum over
        SKY_CHECKSUM_SAMPLES pixel values at a fixed stride.  None -- "cannot be proven unchanged: read and upload" -- while
        the image has unsaved edits (`is_dirty`), when the pixels cannot be sampled, or after invalidate_device_sky()."""
        global _SKY_FORCE_REFRESH
        if _SKY_FORCE_REFRESH:
            _SKY_FORCE_REFRESH = False
            return None
        name = os.path.basename(getattr(self, "sky_image_path", "") or "")
        if not name or name not in bpy.data.images:
            return ("<none>",)
        img = bpy.data.images[name]
        if getattr(img, "is_dirty", False):
            return None
        size = getattr(img, "size", None) or (0, 0)
        filepath = str(getattr(img, "filepath", "") or "")
        source = str(getattr(img, "source", "FILE"))
        ident = [name, int(size[0]), int(size[1]), filepath, source,
                 str(getattr(getattr(img, "colorspace_settings", None), "name", "")), str(getattr(img, "alpha_mode", ""))]
        if source in ("SEQUENCE", "MOVIE"):
            scene = getattr(getattr(bpy, "context", None), "scene", None)
            ident.append(int(getattr(scene, "frame_current", 0) or 0))
        if source in ("FILE", "SEQUENCE", "MOVIE") and filepath and getattr(img, "packed_file", None) is None:
            path = filepath
            absp = getattr(getattr(bpy, "path", None), "abspath", None)
            if callable(absp):
                try:
                    path = absp(filepath)
                except Exception:   # noqa: BLE001
                    path = filepath
            try:
                st = os.stat(path)
                ident += [int(st.st_mtime_ns), int(st.st_size)]
            except OSError:
                ident += [None, None]      # (no such file -- a generated image, a relative path: the checksum below carries it)
        try:
            px = img.pixels
            n = int(size[0]) * int(size[1]) * 4
            if n <= 0 or len(px) < n:
                return None
            step = max(1, n // self.SKY_CHECKSUM_SAMPLES)
            # (+ 1: a stride that is a multiple of 4 would only ever look at one channel)
            vals = np.asarray([px[i] for i in range(0, n, step + (1 if step % 4 == 0 else 0))], dtype=np.float32)
            ident.append(hash(vals.tobytes()))
        except Exception:   # noqa: BLE001
            return None
        return tuple(ident)

    def _sky_pixels(self):
        """The sky image as float32 [h, w, 4], rows bottom-up as Blender stores them -- which is the library's
        convention too (texture coordinate v = -1 is row 0).  None when there is no readable image."""
        name = os.path.basename(getattr(self, "sky_image_path", "") or "")
        if not name or name not in bpy.data.images:
            return None
        img = bpy.data.images[name]
        size = getattr(img, "size", None)
        if size is None or not hasattr(img, "pixels"):
            return None
        w, h = int(size[0]), int(size[1])
        if w <= 0 or h <= 0:
            return None
        px = np.empty(w * h * 4, dtype=np.float32)
        if hasattr(img.pixels, "foreach_get"):
            img.pixels.foreach_get(px)
        else:
            px[:] = np.asarray(img.pixels[:], dtype=np.float32)
        return px.reshape(h, w, 4)

    def ray_trace_device(self, width, height, samples, buf, origin, rotation, spheres, mesh=None):
        """The generator protocol of ray_trace with everything between the jitter stream and the averaged pixels on
        the GPU(s): a library-owned frame (bhg_frame_*, include/bhgeo.h; _ffi.Frame -- ctypes only, no PyTorch: Blender's
        bundled Python has none).  Per listed device ONE ray-generation launch, ONE trace launch for all samples, ONE
        shade + mean launch; one gather onto the first device; ONE float RGBA array back.  scene.render_devices = N
        shards the image tiles over the first N GPUs of the machine (the reference's render thread is one thread of one
        process, :152-168; its commented-out mp.Pool, :210-216, is where the author wanted the parallelism)."""
        from . import _ffi
        from .raygen import euler_xyz_matrix, python_random_stream
        n_dev = max(1, int(getattr(self, "render_devices", 1) or 1))
        avail = _ffi.device_count()
        if n_dev > avail:
            warnings.warn(f"render_devices = {n_dev} but {avail} GPU(s) are visible: using {max(avail, 1)}", RuntimeWarning)
            n_dev = max(avail, 1)
        first = int(getattr(self.GeoInt.context, "device", 0))
        devices = [(first + i) % max(avail, 1) for i in range(n_dev)]
        if os.environ.get("BHGEO_DEVICES"):
            # an explicit device list, e.g. "2,3" or -- several contexts of ONE GPU, the N > 1 code path on a one-GPU
            # machine (tests) -- "0,0"
            devices = [int(v) for v in os.environ["BHGEO_DEVICES"].split(",")]
        # The frame object outlives the render: Blender makes a new engine instance for every frame of an animation, and
        # creating the frame (the MT19937 stream, the buffers, the first launch of every kernel) costs 100 ms where a render
        # costs 2.4 -- so it is kept at module level and only its camera and scene move (bhg_frame_set_camera / _set_scene).
        # Anything that changes the rays' layout (resolution, samples, seed, device list) makes a new one.
        key = (tuple(devices), int(width), int(height), int(samples), float(self.sampling_seed))
        cam_origin = np.asarray(origin, dtype=np.float64) - self.bh_loc                          # :278
        fr = _DEVICE_FRAMES.get(key)
        if fr is None:
            release_device_frames()
            jitter = python_random_stream(self.sampling_seed, 2 * samples * width * height)      # :189
            fr = _ffi.Frame(devices, width, height, samples, fov_x=self.field_of_view_x, fov_y=self.field_of_view_y,
                            origin=cam_origin, rot=euler_xyz_matrix(rotation), jitter=jitter)
            _DEVICE_FRAMES[key] = fr
            self.device_frame_reused = False
        else:
            fr.set_camera(fov_x=self.field_of_view_x, fov_y=self.field_of_view_y, origin=cam_origin, rot=euler_xyz_matrix(rotation))
            self.device_frame_reused = True
        try:
            sp, lamps = None, None
            if len(spheres) > 0:
                sp = np.array(spheres, dtype=np.float64).reshape(-1, 4)
                sp[:, 0:3] -= self.bh_loc                    # the solver and the shade kernel work BH-centred
            if len(spheres) > 0 or mesh is not None:
                all_lamps = getattr(self, "lamps", [])
                if len(all_lamps) > 4:
                    # (the host path sums over every lamp; the device scene holds four -- say so instead of quietly
                    # rendering a darker image)
                    warnings.warn(f"{len(all_lamps)} lamps in the scene: the device path lights objects with the first 4 "
                                  "(scene.device_shading = 0 sums over all of them)", RuntimeWarning)
                lamps = [[*(np.array(list(l.location), dtype=np.float64) - self.bh_loc), self.LAMP_INTENSITY]
                         for l in all_lamps][:4]
            # The sky image is read (33 MB of float RGBA for a 2k x 1k image) and uploaded to every device only when it is
            # another image than the frame already holds: an animation renders hundreds of frames against one sky.
            sky_id = self._sky_identity()
            sky = None
            if sky_id is None or getattr(fr, "sky_identity", None) != sky_id:
                sky = self._sky_pixels()
                if sky is None:
                    sky = np.zeros((2, 2, 4), dtype=np.float32)     # no sky image: black, as background_hit returns (:369-370)
            self.device_sky_uploaded = sky is not None
            fr.set_scene(sky, spheres=sp, sphere_rgb=None if sp is None else np.ones((len(sp), 3)), lamps=lamps)
            fr.sky_identity = sky_id
            self._set_device_object_textures(fr)
            self._set_device_mesh(fr, mesh)
            rgba = fr.render(self.GeoInt.params(self.max_integration_step, self.int_depth_curve_end))
            buf[:, :, :] = rgba.reshape(height, width, 4)
            self.last_device_frame = fr.info()
        except BaseException:
            release_device_frames()      # (a frame that failed is not kept)
            raise
        n = samples * height
        for i in range(n):       # progress: the frame is one launch per device, reported after the fact at ray_trace's cadence
            yield (i + 1) / n

    def _image_identity(self, name):
        """What tells an object image's content apart without reading it: name, size, file path; None (read and upload) while
        it has unsaved edits."""
        img = bpy.data.images[name]
        if getattr(img, "is_dirty", False):
            return None
        size = getattr(img, "size", None) or (0, 0)
        return (name, int(size[0]), int(size[1]), str(getattr(img, "filepath", "") or ""))

    def _image_pixels(self, name):
        """An image as float32 [h, w, 4], rows bottom-up (the library's convention, as for the sky)."""
        img = bpy.data.images[name]
        w, h = (int(v) for v in img.size)
        px = np.empty(w * h * 4, dtype=np.float32)
        if hasattr(img.pixels, "foreach_get"):
            img.pixels.foreach_get(px)
        else:
            px[:] = np.asarray(img.pixels[:], dtype=np.float32)
        return px.reshape(h, w, 4)

    def _set_device_object_textures(self, fr):
        """The traced spheres' looks on the library-owned frame: images are read and uploaded only when a slot's image is
        another than the frame holds (an animation turns its sphere every frame: that is a kernel argument); a scene without
        textured or emissive objects turns them off (the frame's shading as before, bit for bit)."""
        looks = getattr(self, "_sphere_looks", [])
        held = getattr(fr, "object_image_ids", None) or [None] * 8
        if not any(l["image"] is not None or l["emission"] > 0.0 for l in looks):
            fr.set_object_textures()
            fr.object_image_ids = [None] * 8
            return
        textures, ids = [], list(held)
        for j, look in enumerate(looks):
            ident = None if look["image"] is None else self._image_identity(look["image"])
            if look["image"] is None:
                # (the slot's texture must be white: a slot that held an image is given a 1 x 1 white one)
                textures.append(np.ones((1, 1, 4), np.float32) if held[j] != ("<white>",) else None)
                ids[j] = ("<white>",)
            elif ident is None or ident != held[j]:
                textures.append(self._image_pixels(look["image"]))
                ids[j] = ident
            else:
                textures.append(None)
        fr.set_object_textures(textures=textures, rotations=[l["rot"] for l in looks],
                               modes=["emissive" if l["emission"] > 0.0 else "lit" for l in looks],
                               emission=[l["emission"] for l in looks])
        fr.object_image_ids = ids
        self.device_object_images_uploaded = sum(t is not None for t in textures)

    # ---- shading (:366-378), Blender's own texture filter ------------------------------------
    def background_hit(self, direction):
        if self.sky_tex_name not in bpy.data.textures:
            return np.array([0.0, 0.0, 0.0])
        u, v = equirect_uv(np.asarray(direction, dtype=np.float64))
        return np.array(bpy.data.textures[self.sky_tex_name].evaluate((float(u), float(v), 0)).xyz)

    def background_hit_many(self, directions):
        directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
        if self.sky_tex_name not in bpy.data.textures:
            return np.zeros(directions.shape)
        tex = bpy.data.textures[self.sky_tex_name]
        u, v = equirect_uv(directions)
        return np.array([tex.evaluate((float(a), float(b), 0)).xyz for a, b in zip(u, v)], dtype=np.float64)


class CUSTOM_RENDER_PT_blackhole(RenderButtonsPanel, Panel):
    bl_label = "Blackhole Settings"
    COMPAT_ENGINES = {RelativisticRenderEngine.bl_idname}

    _ROWS = (("blackhole_obj", "Blackhole"), ("mass", "Mass"), ("max_integration_step", "Max integration step"),
             ("integration_depth", "Integration depth"), ("field_of_view_x", "field_of_view_x"),
             ("field_of_view_y", "field_of_view_y"), ("sampling_seed", "Sampling seed"), ("sky_image", "Sky image"),
             ("mark_x_min", "mark_x_min"), ("mark_x_max", "mark_x_max"), ("mark_y_min", "mark_y_min"),
             ("mark_y_max", "mark_y_max"), ("curved_space_objects", "Objects in curved space (0/1)"),
             ("curved_space_meshes", "Mesh objects as triangles (0/1)"),
             ("curved_space_mesh_instances", "Linked duplicates as instances (0/1)"),
             ("curved_space_mesh_instance_tree", "Instances under a tree of boxes (0/1)"),
             ("curved_space_mesh_refit", "Deforming meshes refit, not rebuilt (0/1)"),
             ("curved_space_mesh_build", "Mesh trees built on the GPU (0/1)"),
             ("device_shading", "Shade on the GPU (0/1)"), ("render_devices", "GPUs to render on"))

    def draw(self, context):
        col = self.layout.split().column()
        for prop, text in self._ROWS:
            col.row().prop(bpy.context.scene, prop, text=text)


# scene properties: names and defaults of the reference (:504-517)
PROPS = [
    ("blackhole_obj", bpy.props.PointerProperty(name="blackhole_obj", type=bpy.types.Object)),
    ("mass", bpy.props.FloatProperty(name="Mass", default=0.5)),
    ("max_integration_step", bpy.props.FloatProperty(name="max_integration_step", default=10000)),
    ("integration_depth", bpy.props.FloatProperty(name="integration_depth", default=50)),
    ("sampling_seed", bpy.props.FloatProperty(name="sampling_seed", default=42)),
    ("field_of_view_x", bpy.props.FloatProperty(name="field_of_view_x", default=1)),
    ("field_of_view_y", bpy.props.FloatProperty(name="field_of_view_y", default=1)),
    ("sky_image", bpy.props.StringProperty(name="sky_image", default="", subtype="FILE_PATH")),
    ("mark_y_min", bpy.props.FloatProperty(name="mark_y_min", default=-1.0)),
    ("mark_y_max", bpy.props.FloatProperty(name="mark_y_max", default=-1.0)),
    ("mark_x_min", bpy.props.FloatProperty(name="mark_x_min", default=-1.0)),
    ("mark_x_max", bpy.props.FloatProperty(name="mark_x_max", default=-1.0)),
]

# beyond the reference, all opt-in (module docstring): objects inside the curved region; the frame shaded on the GPU;
# the number of GPUs the device path shards the image over
EXTRA_PROPS = [
    ("curved_space_objects", bpy.props.FloatProperty(name="curved_space_objects", default=0)),
    ("curved_space_meshes", bpy.props.FloatProperty(name="curved_space_meshes", default=0)),
    ("curved_space_mesh_instances", bpy.props.FloatProperty(name="curved_space_mesh_instances", default=0)),
    ("curved_space_mesh_instance_tree", bpy.props.FloatProperty(name="curved_space_mesh_instance_tree", default=0)),
    ("curved_space_mesh_refit", bpy.props.FloatProperty(name="curved_space_mesh_refit", default=0)),
    ("curved_space_mesh_build", bpy.props.FloatProperty(name="curved_space_mesh_build", default=0)),
    ("device_shading", bpy.props.FloatProperty(name="device_shading", default=0)),
    ("render_devices", bpy.props.FloatProperty(name="render_devices", default=1)),
]

# the library-owned frame of the device path, kept across renders (see ray_trace_device): at most one
_DEVICE_FRAMES = {}
_SKY_FORCE_REFRESH = False


def invalidate_device_sky():
    """Force the next device render to read the sky image and upload it again, whatever its identity says (a hook for
    scripts that change the image in ways the identity cannot see)."""
    global _SKY_FORCE_REFRESH
    _SKY_FORCE_REFRESH = True


def release_device_frames():
    """Free the GPU buffers the device path keeps between renders (called by unregister(), and when the frame's shape changes)."""
    for fr in list(_DEVICE_FRAMES.values()):
        try:
            fr.close()
        except Exception:
            pass
    _DEVICE_FRAMES.clear()


_EXCLUDED_PANELS = {"VIEWLAYER_PT_filter", "VIEWLAYER_PT_layer_passes"}


def get_panels():
    """Stock panels that declare themselves compatible with BLENDER_RENDER (:520-534)."""
    return [p for p in bpy.types.Panel.__subclasses__()
            if "BLENDER_RENDER" in getattr(p, "COMPAT_ENGINES", ()) and p.__name__ not in _EXCLUDED_PANELS]


def _extra_panels():
    """Eevee sampling / world / material panels the reference also enables (:551-564)."""
    try:
        from bl_ui import properties_material, properties_render, properties_world
    except ImportError:
        return []
    names = ((properties_render, "RENDER_PT_eevee_sampling"), (properties_world, "WORLD_PT_context_world"),
             (properties_material, "EEVEE_MATERIAL_PT_context_material"), (properties_material, "EEVEE_MATERIAL_PT_surface"))
    return [getattr(mod, n) for mod, n in names if hasattr(mod, n)]


def register():
    bpy.utils.register_class(RelativisticRenderEngine)
    bpy.utils.register_class(CUSTOM_RENDER_PT_blackhole)
    for name, prop in PROPS + EXTRA_PROPS:
        setattr(bpy.types.Scene, name, prop)
    for panel in get_panels() + [CUSTOM_RENDER_PT_blackhole] + _extra_panels():
        panel.COMPAT_ENGINES.add(RelativisticRenderEngine.bl_idname)


def unregister():
    release_device_frames()
    bpy.utils.unregister_class(RelativisticRenderEngine)
    bpy.utils.unregister_class(CUSTOM_RENDER_PT_blackhole)
    for name, _ in PROPS + EXTRA_PROPS:
        delattr(bpy.types.Scene, name)
    for panel in get_panels() + [CUSTOM_RENDER_PT_blackhole] + _extra_panels():
        panel.COMPAT_ENGINES.discard(RelativisticRenderEngine.bl_idname)


if __name__ == "__main__":
    register()

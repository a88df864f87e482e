"""Mesh objects for the stand-in bpy of fake_bpy.py: exactly what the add-on's scene_mesh() reads of an evaluated object --
to_mesh(), calc_loop_triangles(), loop_triangles / vertices / polygons / uv_layers.active.data with foreach_get, matrix_world,
custom properties.  Polygons are fan-triangulated as Blender triangulates convex ones.  Test infrastructure."""
import types

import numpy as np


class _Coll(list):
    """A bpy collection: a list of namespaces with foreach_get(attribute, flat buffer)."""

    def foreach_get(self, attr, out):
        vals = np.array([getattr(e, attr) for e in self])
        out[:] = vals.reshape(-1).astype(out.dtype)
        _Coll.foreach_calls += 1

    foreach_calls = 0


class FakeMesh:
    def __init__(self, verts, polys, loop_uv=None, smooth=False):
        verts = np.asarray(verts, dtype=np.float64)
        nrm = verts - verts.mean(0)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        self.vertices = _Coll(types.SimpleNamespace(co=tuple(v), normal=tuple(n)) for v, n in zip(verts, nrm))
        self.polygons = _Coll(types.SimpleNamespace(use_smooth=bool(smooth), vertices=tuple(p)) for p in polys)
        self._polys = polys
        self.loop_triangles = _Coll()
        n_loops = sum(len(p) for p in polys)
        self.uv_layers = types.SimpleNamespace(active=None)
        if loop_uv is not None:
            assert len(loop_uv) == n_loops
            self.uv_layers.active = types.SimpleNamespace(data=_Coll(types.SimpleNamespace(uv=tuple(u)) for u in loop_uv))

    def calc_loop_triangles(self):
        self.loop_triangles[:] = []
        first = 0
        for p in self._polys:
            for k in range(1, len(p) - 1):
                self.loop_triangles.append(types.SimpleNamespace(vertices=(p[0], p[k], p[k + 1]), loops=(first, first + k, first + k + 1)))
            first += len(p)


class MeshObject(dict):
    """A MESH object with geometry and custom properties (ob["key"], ob.get("key"))."""

    def __init__(self, mesh, matrix_world, **custom):
        super().__init__(custom)
        self.type, self._mesh = "MESH", mesh
        self.matrix_world = np.asarray(matrix_world, dtype=np.float64)
        self.location = tuple(self.matrix_world[:3, 3])
        co = np.array([v.co for v in mesh.vertices]) @ self.matrix_world[:3, :3].T
        self.dimensions = tuple(co.max(0) - co.min(0))
        self.cleared = 0

    def evaluated_get(self, depsgraph):
        return self

    def to_mesh(self):
        return self._mesh

    def to_mesh_clear(self):
        self.cleared += 1


CUBE_V = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
CUBE_P = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]
TETRA_V = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
TETRA_P = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]


def cube(matrix_world, **custom):
    """A cube of six quads; every face maps its own patch of UV space, some of it outside [0, 1] (the repeat)."""
    rng = np.random.default_rng(21)
    uv = []
    for f in range(6):
        o = rng.uniform(-1.2, 1.2, 2)
        uv += [o, o + (0.9, 0.0), o + (0.9, 0.7), o + (0.0, 0.7)]
    return MeshObject(FakeMesh(CUBE_V, CUBE_P, np.array(uv, dtype=np.float32)), matrix_world, **custom)


def tetrahedron(matrix_world, **custom):
    return MeshObject(FakeMesh(TETRA_V, TETRA_P), matrix_world, **custom)


def world(scale, angle_z, translation):
    c, s = np.cos(angle_z), np.sin(angle_z)
    m = np.eye(4)
    m[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) * np.asarray(scale, dtype=np.float64)
    m[:3, 3] = translation
    return m

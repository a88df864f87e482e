"""Deforming meshes: the meshes, deformations, rays and numpy restatements that
tests/test_mesh_refit_host.py and tests/test_gpu_mesh_refit.py share, and the child process of the latter.  Not a test module.

    python tests/mesh_refit_cases.py OUT.npz     # every trace case on a REFITTED mesh through bhg_trace_mesh_device, into OUT.npz
                                                 # (tests/test_gpu_mesh_refit.py runs this with BHGEO_MESH_CULL=0)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_cases as mc  # noqa: E402
import mesh_oracle_cases as mo  # noqa: E402
import mesh_reference as mr  # noqa: E402

KEYS = ("end", "flags", "n_steps", "n_accepted", "tri", "bary")
FORMS = {"christoffel": (0, 0.0), "reduced": (1, 0.0), "kerr_plus": (2, 0.45), "kerr_minus": (2, -0.45)}
DEFORMS = ("noise", "mirror", "twist", "permute")
CENTRE = np.array(mo.FRAME_SPHERE)
ULP16 = 16.0 * 2.220446049250313e-16


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def ellipsoid128(centre=CENTRE):
    V, F = mr.octa_sphere((0.0, 0.0, 0.0), 1.0, 2)
    return V * np.array([1.4, 1.0, 0.7]) + np.asarray(centre, float), F


def sphere4097(centre=CENTRE, radius=1.2):
    """A latitude-longitude sphere of 64 segments and 33 rings, 4 096 triangles, and the first triangle once more with its corners
    rotated: 4 097, one over a power of two."""
    n, m = 64, 33
    th = np.linspace(0.0, np.pi, m + 1)[1:-1]
    ph = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n))], -1)
    V = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]]) * radius + np.asarray(centre, float)
    at = lambda r, s: 1 + r * n + s % n      # noqa: E731
    south = 1 + (m - 1) * n
    F = [(0, at(0, s), at(0, s + 1)) for s in range(n)]
    for r in range(m - 2):
        for s in range(n):
            F += [(at(r, s), at(r + 1, s), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r, s + 1))]
    F += [(south, at(m - 2, s + 1), at(m - 2, s)) for s in range(n)]
    F.append((F[0][1], F[0][2], F[0][0]))
    F = np.array(F, np.int32)
    assert len(F) == 4097 and F.max() == len(V) - 1
    return np.ascontiguousarray(V), F


def meshes():
    """name -> (V, F, leaf sizes): the issue's list -- one triangle; five identical triangles (one leaf over leaf_size); the
    128-triangle ellipsoid at leaf_size 1, 4 and nt; the 4 097-triangle sphere (at leaf_size 1 its 4 096 inner nodes take one launch
    per level, every smaller tree here the single workgroup); a flat plate (boxes of no thickness); a mesh whose vertex array
    holds vertices no triangle names, two of them far out."""
    one = (np.array([[-3.5, 0.5, 0.0], [-2.5, 1.2, 0.4], [-3.0, 1.6, 1.0]]), np.array([[0, 1, 2]], np.int32))
    tet = mr.tetrahedron(CENTRE, 1.0)
    spare = np.concatenate([tet[0][:2], [[50.0, -60.0, 70.0]], tet[0][2:], [[-90.0, 0.0, 0.0], [0.1, 0.1, 0.1]]])
    remap = np.array([0, 1, 3, 4])
    return {
        "one": (*one, (1,)),
        "identical5": (one[0], np.tile(one[1], (5, 1)), (4,)),
        "ellipsoid128": (*ellipsoid128(), (1, 4, 128)),
        "sphere4097": (*sphere4097(), (1, 4)),
        "plate": (*mo.flat_plate(0.3, 1.5, 6), (1, 4)),
        "spare_vertices": (np.ascontiguousarray(spare), remap[tet[1]].astype(np.int32), (1, 4)),
    }


# ---- deformations ----------------------------------------------------------------------------------------------------------
def deform(V, kind, seed=0):
    """noise: 1 % of the mesh's extent on every coordinate; mirror: x -> -x; twist: a turn about the vertical through the mesh's
    centre that grows from 0 at its lowest point to pi at its highest; permute: the positions dealt to the vertices at random."""
    V = np.asarray(V, float)
    rng = np.random.default_rng(1000 + seed)
    size = max(float(np.ptp(V, axis=0).max()), 1e-3)
    if kind == "noise":
        return V + rng.normal(size=V.shape) * 0.01 * size
    if kind == "mirror":
        return V * np.array([-1.0, 1.0, 1.0])
    if kind == "twist":
        c = 0.5 * (V.min(0) + V.max(0))
        h = max(float(np.ptp(V[:, 2])), 1e-300)
        ang = np.pi * (V[:, 2] - V[:, 2].min()) / h
        x, y = V[:, 0] - c[0], V[:, 1] - c[1]
        return np.ascontiguousarray(np.stack([c[0] + np.cos(ang) * x - np.sin(ang) * y, c[1] + np.sin(ang) * x + np.cos(ang) * y, V[:, 2]], 1))
    if kind == "permute":
        return np.ascontiguousarray(V[rng.permutation(len(V))])
    if kind == "random":        # the host test's 200 draws: each vertex anywhere in a ball three times the mesh's size
        return V.mean(0) + rng.normal(size=V.shape) * size * float(rng.uniform(0.1, 3.0))
    raise KeyError(kind)


# ---- numpy restatements ------------------------------------------------------------------------------------------------------
def refit_numpy(V, F, tree):
    """The refitted, widened boxes and the area sum (plain numpy summation) of a tree's topology on the vertices V."""
    nn = len(tree["skip"])
    box = np.empty((nn, 6))
    for i in range(nn - 1, -1, -1):
        if tree["count"][i] > 0:
            lo, hi = int(tree["first"][i]), int(tree["first"][i] + tree["count"][i])
            pts = V[F[tree["order"][lo:hi]]].reshape(-1, 3)
            box[i, :3], box[i, 3:] = pts.min(0), pts.max(0)
        else:
            l, r = i + 1, int(tree["skip"][i + 1])
            box[i, :3], box[i, 3:] = np.minimum(box[l, :3], box[r, :3]), np.maximum(box[l, 3:], box[r, 3:])
    w = ULP16 * np.maximum(np.abs(box).max(1), 2.2250738585072014e-308)
    box[:, :3] -= w[:, None]
    box[:, 3:] += w[:, None]
    d = box[:, 3:] - box[:, :3]
    return box, float((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]).sum())


def slot_records(V, F, tree):
    """[nt, 9]: v0, v1 - v0, v2 - v0 of the triangle in each leaf slot, as bhg_mesh_create writes them."""
    T = V[F[tree["order"]]]
    return np.concatenate([T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]], 1)


# ---- the trace cases ---------------------------------------------------------------------------------------------------------
def trace_mesh():
    """The ellipsoid, a tetrahedron beside it and a tilted plate above it: 204 triangles about mesh_oracle_cases.FRAME_SPHERE."""
    plate = mo.flat_plate(0.0, 0.9, 6)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.5), -np.sin(0.5)], [0.0, np.sin(0.5), np.cos(0.5)]])
    return mr.join(ellipsoid128(), mr.tetrahedron(CENTRE + [0.4, -1.9, 0.6], 0.7), (plate[0] @ R.T + CENTRE + [0.0, 0.3, 1.5], plate[1]))


def trace_rays(n=2048, seed=31):
    """mesh_oracle_cases.frame_rays in style: from its camera towards the mesh, towards the mesh's mirror image (where `mirror`
    puts it) and past the hole at every impact parameter."""
    rng = np.random.default_rng(seed)
    a, b = (n * 3) // 8, n // 4
    return np.concatenate([mr.camera_rays(mo.FRAME_CAM, CENTRE, a, rng, 2.8), mr.camera_rays(mo.FRAME_CAM, CENTRE * [-1.0, 1.0, 1.0], b, rng, 2.8),
                           mr.hole_rays(mo.FRAME_CAM, n - a - b, rng, 0.3, 12.0)])


SCENES = {"bare": dict(r_s=1.0, lambda_end=46.0), "disk_and_exit": dict(r_s=1.0, lambda_end=46.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)}
CHORD = 0.25
MIN_HITS = 40       # rays that end on the mesh, in every trace case (checked with the oracle on the CPU by the host test)


def trace_cases():
    """name -> (rhs_form, spin, params keywords, deformation)"""
    return {f"{form}-{scene}-{kind}": (rhs, a, SCENES[scene], kind)
            for form, (rhs, a) in FORMS.items() for scene in SCENES for kind in DEFORMS}


def oracle_case(form):
    """The case held to the brute-force oracle: the twisted mesh, 512 rays, disk and exit sphere, as a mesh_oracle_cases case."""
    rhs, a = FORMS[form]
    V, F = trace_mesh()
    return mo._case(rhs, a, SCENES["disk_and_exit"], (deform(V, "twist"), F), CHORD, trace_rays(512, 32), mo.FRAME_CAM, hit=MIN_HITS)


def run_refitted(ctx, cases=None):
    """Every trace case on a mesh created from the undeformed vertices and refitted to the deformed ones."""
    from blackhole_geodesic_calculator_amd import _ffi
    V, F = trace_mesh()
    k0 = trace_rays()
    mesh = _ffi.Mesh(ctx, V, F)
    res = {}
    for name, (rhs, a, par, kind) in (cases or trace_cases()).items():
        mesh.refit(deform(V, kind))
        r = mc.trace_mesh_device(ctx, _ffi.make_params(rhs_form=rhs, spin=a, **par), mesh, CHORD, k0, mo.FRAME_CAM)
        for key, arr in r.items():
            res[f"{name}__{key}"] = arr
    mesh.close()
    return res


if __name__ == "__main__":
    from blackhole_geodesic_calculator_amd import _ffi
    c = _ffi.Context(0)
    np.savez(sys.argv[1], **run_refitted(c))
    c.close()

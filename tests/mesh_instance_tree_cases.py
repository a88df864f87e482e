"""Instance trees: the cases beyond 64 placements that tests/test_mesh_instance_tree_host.py conditions on
the CPU and tests/test_gpu_mesh_instance_tree.py runs on the device, built on mesh_instance_cases (instance_case, flatten,
oracle_solve, hits_per_instance), and the device call over a set that lies under a tree.  Not a test module.

    python tests/mesh_instance_tree_cases.py OUT.npz     # every case of beyond_cases() as a tree set through the device call,
                                                         # arrays into OUT.npz (tests/test_gpu_mesh_instance_tree.py runs this with
                                                         # BHGEO_INSTANCE_TREE=0 and with BHGEO_MESH_CULL=0)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_instance_cases as mi  # noqa: E402
import mesh_oracle_cases as mo  # noqa: E402
import mesh_reference as mr  # noqa: E402

SWARM_RINGS = ((7.0, 0.35, 0.0), (9.0, -0.5, 0.4), (11.0, 0.9, 1.1))      # (radius, tilt about x, phase)
SWARM_PER_RING = 64
SWARM_RAYS = 6
CLUMP_K = 96
CLUMP_RADIUS = 1.5


def swarm_case():
    """192 small tetrahedra on three tilted rings about the hole, as mesh_instance_cases.ring_case lays out its one: each turned
    its own way, 6 rays to each from a camera above, aimed along the ring's radius through it from 0.3 inside to 2 outside."""
    rng = np.random.default_rng(43)
    cam = np.array([2.0, -3.0, 24.0])
    T, k0 = [], []
    for radius, tilt_by, phase in SWARM_RINGS:
        tilt = mi.rotation((1.0, 0.0, 0.0), tilt_by)
        for j in range(SWARM_PER_RING):
            phi = 2.0 * np.pi * j / SWARM_PER_RING + phase
            c = tilt @ np.array([radius * np.cos(phi), radius * np.sin(phi), 0.0])
            T.append(mi.record(mi.rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)), c))
            aim = c[None, :] * (1.0 + np.linspace(-0.3, 2.0, SWARM_RAYS) / radius)[:, None] - cam[None, :]
            k0.append(aim / np.linalg.norm(aim, axis=1)[:, None])
    return mi.instance_case(0, 0.0, dict(r_s=1.0, lambda_end=60.0, r_exit=40.0), mr.tetrahedron((0.0, 0.0, 0.0), 0.5), np.stack(T), 0.25,
                            np.concatenate(k0), cam)


def clump_placements():
    """96 tetrahedra at random offsets within a ball of radius 1.5 about mesh_oracle_cases.FRAME_SPHERE, each turned its own way:
    their world boxes overlap heavily."""
    rng = np.random.default_rng(47)
    T = []
    for _ in range(CLUMP_K):
        u = rng.normal(size=3)
        off = u / np.linalg.norm(u) * CLUMP_RADIUS * rng.uniform() ** (1.0 / 3.0)
        T.append(mi.record(mi.rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)), np.asarray(mo.FRAME_SPHERE) + off))
    return np.stack(T)


def clump_rays(seed=53):
    rng = np.random.default_rng(seed)
    return np.concatenate([mr.camera_rays(mo.FRAME_CAM, mo.FRAME_SPHERE, 768, rng, 2.2), mr.hole_rays(mo.FRAME_CAM, 256, rng, 2.4, 7.0)])


def clump_case(form):
    """form: a key of mesh_instance_cases.FORMS.  The parameters of three_placement_cases, disk and exit sphere included."""
    rhs, a = mi.FORMS[form]
    par = dict(r_s=1.0, lambda_end=64.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    return mi.instance_case(rhs, a, par, mr.tetrahedron((0.0, 0.0, 0.0), 0.5), clump_placements(), 0.25, clump_rays(), mo.FRAME_CAM)


def beyond_cases():
    """The cases with more than 64 placements."""
    return {"swarm": swarm_case(), "clump_christoffel": clump_case("christoffel"), "clump_kerr_plus": clump_case("kerr_plus")}


# two lamps for the clump's shade: one above the camera, one well off to the clump's side, so that placements shadow one another;
# I^2 / d^2 is 0.28 and 0.40 at the clump's centre: a mesh ray's colour stays under 1
CLUMP_LAMPS = [[18.0, 2.0, 9.0, 12.0], [-3.0, 14.0, 6.0, 9.0]]


# ---- the device --------------------------------------------------------------------------------------------------------------
def run_case(ctx, case, T=None, leaf=4, tree=True, tree_leaf=2):
    """The case's local mesh under the records T (the case's own by default), as a set under a tree (or a linear one: tree=False),
    through the device call on sentinel-filled arrays."""
    from blackhole_geodesic_calculator_amd import _ffi
    mesh = _ffi.Mesh(ctx, case["Vl"], case["Fl"], leaf_size=leaf)
    try:
        inst = _ffi.MeshInstances(mesh, case["T"] if T is None else T, tree=tree, leaf_size=tree_leaf)
        return mi.trace_instances_device(ctx, _ffi.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"]), inst, case["chord"],
                                         case["k0"], case["x0"])
    finally:
        mesh.close()


def run_beyond_cases(ctx):
    res = {}
    for name, case in beyond_cases().items():
        for key, arr in run_case(ctx, case).items():
            res[f"{name}__{key}"] = arr
    return res


if __name__ == "__main__":
    from blackhole_geodesic_calculator_amd import _ffi
    c = _ffi.Context(0)
    np.savez(sys.argv[1], **run_beyond_cases(c))
    c.close()

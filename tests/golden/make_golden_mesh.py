#!/usr/bin/env python3
"""Generate the golden vectors of the mesh trace:

    python tests/golden/make_golden_mesh.py      # writes tests/golden/mesh.npz

The solve and the hit rule are tests/mesh_reference.py's (scipy's solve_ivp with dense_output on oracle/scipy_reference's
right-hand sides, the rule applied to each step's interpolant with a brute-force Moeller-Trumbore).  Camera (20, 0, 2), rtol 1e-3,
atol 1e-6, lambda_end 80, max_chord 0.25; the Cartesian forms with the exit sphere at 40, Kerr (a = 0.225 and 0.45, M = 0.5)
without one.  Three meshes (mesh_reference.golden_meshes): the 32-triangle sphere behind the hole, a tetrahedron in front, two
components; N_RAYS rays each.  Per mesh, form and ray: flags, n_attempted (-1 where scipy's count is not comparable), n_accepted,
tri, bary, end, M of the hit step, sag, sens (the end record's largest movement under the three 1-2 ulp perturbations of k0) and
stable (flag, triangle, step counts and M unchanged under them).  At most 1 % of a set may be unstable.  The same rays at
max_chord 0.03: end_fine, tri_fine, n_accepted_fine (what tests/test_mesh_host.py compares the chord lengths on).

Needs numpy, scipy, sympy.  Several minutes on one core.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import mesh_reference as mr  # noqa: E402

N_RAYS = 160
SEED = 19
FINE_CHORD = 0.03
MAX_UNSTABLE = 0.01


def main():
    meshes = mr.golden_meshes()
    out = dict(x0=mr.GOLDEN_CAM, max_chord=mr.GOLDEN_CHORD, fine_chord=FINE_CHORD, r_exit=mr.GOLDEN_R_EXIT,
               forms=np.array(mr.GOLDEN_FORMS), mesh_names=np.array(sorted(meshes)), **mr.GOLDEN_PAR)
    keys = ("end", "flags", "n_attempted", "n_accepted", "tri", "bary", "M", "sag", "sens", "stable")
    for mi, name in enumerate(sorted(meshes)):
        V, F = meshes[name]
        k0 = mr.golden_rays(name, N_RAYS, np.random.default_rng(SEED + mi))
        out[f"{name}_V"], out[f"{name}_F"], out[f"{name}_k0"] = V, F, k0
        per = {k: [] for k in keys + ("end_fine", "tri_fine", "n_accepted_fine")}
        for rhs, a in mr.GOLDEN_FORMS:
            par = dict(spin=a, r_exit=0.0 if rhs == 2 else mr.GOLDEN_R_EXIT, **mr.GOLDEN_PAR)
            r = mr.solve_set(k0, mr.GOLDEN_CAM, rhs, V, F, mr.GOLDEN_CHORD, **par)
            tris = mr.tri_arrays(V, F)
            fine = [mr.solve(k, mr.GOLDEN_CAM, rhs, V, F, FINE_CHORD, tris=tris, **par) for k in k0]
            hits = r["tri"] >= 0
            unstable = int((~r["stable"]).sum())
            print(f"{name} form {rhs} a {a}: {int(hits.sum())} hits of {N_RAYS}, unstable {unstable}, "
                  f"max sag {np.nanmax(np.where(hits, r['sag'], 0.0)):.2e}, max M {r['M'].max()}, max sens on hits "
                  f"{r['sens'][hits].max() if hits.any() else 0.0:.2e}")
            assert unstable <= MAX_UNSTABLE * N_RAYS, "choose another ray set"
            for k in keys:
                per[k].append(r[k])
            per["end_fine"].append(np.array([q["end"] for q in fine]))
            per["tri_fine"].append(np.array([q["tri"] for q in fine], np.int32))
            per["n_accepted_fine"].append(np.array([q["n_accepted"] for q in fine], np.uint32))
        for k, v in per.items():
            out[f"{name}_{k}"] = np.array(v)
    path = os.path.join(HERE, "mesh.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

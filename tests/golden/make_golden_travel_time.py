#!/usr/bin/env python3
"""Generate the golden vectors of the travel-time trace:

    python tests/golden/make_golden_travel_time.py      # writes tests/golden/travel_time.npz

The solve and the quadrature are tests/travel_time_reference.py's (scipy's solve_ivp with dense_output on oracle/scipy_reference's
right-hand sides, 6-point Gauss-Legendre on each step's interpolant).  The rays are make_golden_crossings.py's camera-ray sets
(camera at r = 30, three inclinations, two fifths of each set around the critical impact parameter), at most 300 per set:

    default   disk (3, 12), r_exit 35 (Schwarzschild; scipy_reference's Kerr solve has no exit sphere), rtol 1e-3, atol 1e-6
    tight     the same with rtol 1e-8, atol 1e-11, a third of the rays
    nodisk    the default tolerances with the disk off: times to the end only

each for the Schwarzschild pair of forms (one ray set, both forms) and for Kerr (a = 0.45, M = 0.5).  Per ray and form: t_end,
t_cross [K], and S -- the largest movement of each time under the three 1-2-ulp perturbations of k0 that
tests/test_gpu_parity.py::_sensitivity uses.  A ray whose flags, step counts or n_cross change under a perturbation -- or one of
whose times changes between finite and infinite -- in any form of its set is dropped; n_drawn and n_kept are stored, and at most
5 % may be dropped.  floor = COND x median(S) over the finite times of a set and form: a ray whose own three-perturbation estimate
comes out tiny is held to the set's typical conditioning.

Needs numpy, scipy, sympy.  Several minutes on one core.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import make_golden_crossings as mgc  # noqa: E402
import travel_time_reference as tt  # noqa: E402

K = 4
DISK = (3.0, 12.0)
MAX_DROPPED = 0.05
SCHW_SETS, SCHW_SEED, SCHW_YOFF = ((85.0, 60), (60.0, 60), (17.0, 60)), 16, 0.0      # make_golden_crossings.main's
KERR_SETS, KERR_SEED, KERR_YOFF = ((80.0, 40), (60.0, 40), (20.0, 40)), 17, 0.5
DEFAULT = dict(r_s=1.0, lambda_end=120.0, rtol=1e-3, atol=1e-6)
TIGHT = dict(r_s=1.0, lambda_end=120.0, rtol=1e-8, atol=1e-11)


def rays(sets, seed, y_off, every=1):
    rng = np.random.default_rng(seed)
    k0s, x0s = zip(*[mgc.camera_rays(inc, n, rng, y_off) for inc, n in sets])
    return np.concatenate(k0s)[::every], np.concatenate(x0s)[::every]


def build(name, forms, k0, x0, disk, par, spin):
    assert len(k0) <= 300
    res = [tt.solve_set(k0, x0, f, disk, K=K, spin=spin, r_exit=0.0 if f == 2 else 35.0, **par) for f in forms]
    keep = np.all([r["stable"] for r in res], 0)
    n_drawn, n_kept = len(k0), int(keep.sum())
    assert n_drawn - n_kept <= MAX_DROPPED * n_drawn, (name, n_drawn, n_kept)
    out = {"k0": k0[keep], "x0": x0[keep], "forms": np.array(forms), "n_drawn": np.int64(n_drawn), "n_kept": np.int64(n_kept),
           "disk": np.array(disk if disk else (0.0, 0.0)), "spin": spin, "r_exit": np.array([0.0 if f == 2 else 35.0 for f in forms])}
    out.update(par)
    for key in ("flags", "n_attempted", "n_accepted", "n_cross", "t_end", "S_end"):
        out[key] = np.stack([r[key][keep] for r in res])
    for key in ("t_cross", "S_cross"):
        out[key] = np.stack([r[key][:, keep] for r in res])
    floors = []
    for f in range(len(forms)):
        S = np.concatenate([out["S_end"][f], out["S_cross"][f].ravel()])
        floors.append(tt.COND * np.median(S[np.isfinite(S)]))
        fin = np.isfinite(out["t_end"][f])
        print(f"  {name} form {forms[f]}: {n_kept} of {n_drawn} kept, finite ends {int(fin.sum())}, crossing times "
              f"{int(np.isfinite(out['t_cross'][f]).sum())}, inf crossing times {int(np.isinf(out['t_cross'][f]).sum())}, "
              f"median S {np.median(S[np.isfinite(S)]):.2e}, max S {np.nanmax(S):.2e}, floor {floors[-1]:.2e}")
    out["floor"] = np.array(floors)
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    g = {}
    sk, sx = rays(SCHW_SETS, SCHW_SEED, SCHW_YOFF)
    kk, kx = rays(KERR_SETS, KERR_SEED, KERR_YOFF)
    g.update(build("schw_default", (0, 1), sk, sx, DISK, DEFAULT, 0.0))
    g.update(build("kerr_default", (2,), kk, kx, DISK, DEFAULT, 0.45))
    g.update(build("schw_nodisk", (0, 1), sk, sx, None, DEFAULT, 0.0))
    g.update(build("kerr_nodisk", (2,), kk, kx, None, DEFAULT, 0.45))
    g.update(build("schw_tight", (0, 1), sk[::3], sx[::3], DISK, TIGHT, 0.0))
    g.update(build("kerr_tight", (2,), kk[::3], kx[::3], DISK, TIGHT, 0.45))
    np.savez_compressed(os.path.join(HERE, "travel_time.npz"), **g)


if __name__ == "__main__":
    main()

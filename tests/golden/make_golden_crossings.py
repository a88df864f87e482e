#!/usr/bin/env python3
"""Generate the golden vectors of the disk-crossings trace:

    python tests/golden/make_golden_crossings.py      # writes tests/golden/disk_crossings.npz, kerr_disk_crossings.npz

oracle/scipy_reference.py has always run the disk plane as a NON-terminal scipy event: sol.t_events[-1] / y_events[-1] of
trace_ray(..., disk=) and trace_ray_kerr(..., disk=) hold every plane crossing of the whole solve.  One solve per ray (with an
annulus no crossing can lie in, so that the returned end, flags and step counts are those of the disk-off trace) gives the
crossings of every disk: a crossing counts when its cylindrical radius lies in [r_in, r_out] and it is not later than the
ray's terminal event (scipy_reference's td <= te).

Rays: camera at r = 30 at three inclinations from the +z axis; each ray is the look-at direction plus
(b / 30)(cos phi right + sin phi up), phi uniform, two fifths of each set with b = linspace(2.585, 2.625) -- around the
critical impact parameter 3 sqrt(3) / 2 r_s, where the higher-order images live -- the rest with b uniform in [2.45, 6].

Per record S_i: the largest movement of that record under the three 1-2-ulp perturbations of k0 that
tests/test_gpu_parity.py::_sensitivity uses.  Rays whose n_cross or step counts change under a perturbation, or between the
Christoffel and the reduced form, are dropped (a selection on the reference alone).

Needs numpy, scipy, sympy.  A few minutes on one core.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import scipy_reference as sr  # noqa: E402

R_CAM = 30.0
K = 4                        # BHG_MAX_CROSSINGS: records kept per ray
NOWHERE = (1e300, 1e301)     # an annulus no crossing lies in: the solve's end, flags and counts are the disk-off trace's
PAR = dict(r_s=1.0, lambda_end=120.0, rtol=1e-3, atol=1e-6)
SCHW_DISKS = ((3.0, 12.0), (1.2, 15.0))    # the second is unphysically deep: it is there for third-order crossings
KERR_DISKS = ((1.2, 15.0),)
KERR = dict(M=0.5, a=0.45)


def camera_rays(incl_deg, n, rng, y_off=0.0):
    inc = np.deg2rad(incl_deg)
    x0 = np.array([R_CAM * np.sin(inc), y_off, R_CAM * np.cos(inc)])
    look = -x0 / np.linalg.norm(x0)
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, look)
    n_crit = (2 * n) // 5
    b = np.concatenate([np.linspace(2.585, 2.625, n_crit), rng.uniform(2.45, 6.0, n - n_crit)])
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    k0 = look[None, :] + (b / R_CAM)[:, None] * (np.cos(phi)[:, None] * right[None, :] + np.sin(phi)[:, None] * up[None, :])
    return k0, np.tile(x0, (n, 1))


def perturbations(k0):
    eps = np.finfo(float).eps
    return (np.nextafter(k0, np.inf), np.nextafter(k0, -np.inf), k0 * (1.0 + np.array([2.0, -2.0, 2.0]) * eps))


def solve(k0, x0, form):
    """One ray: (end, flags, n_attempted, n_accepted) of the disk-off trace and every plane crossing (t, Cartesian record)
    up to the terminal event."""
    if form == "kerr":
        r = sr.trace_ray_kerr(k0, x0, lambda_end=PAR["lambda_end"], rtol=PAR["rtol"], atol=PAR["atol"], disk=NOWHERE, **KERR)
    else:
        r = sr.trace_ray(k0, x0, form=form, r_exit=35.0, disk=NOWHERE, **PAR)
    sol = r["sol"]
    te = r["t_end"]
    recs = []
    for td, yd in zip(sol.t_events[-1], sol.y_events[-1]):
        if not td <= te:
            continue
        if form == "kerr":
            xc, kc = sr.bl_to_cart((yd[1], yd[3], yd[5]), (yd[0], yd[2], yd[4]), KERR["a"])
            recs.append(np.concatenate([xc, kc]))
        else:
            recs.append(np.array([yd[1], yd[3], yd[5], yd[0], yd[2], yd[4]]))
    return r["end"], r["flags"], r["n_attempted"], r["n_accepted"], recs


def layers(recs, disk):
    """The records that count for this annulus, in order."""
    return [q for q in recs if disk[0] <= np.hypot(q[0], q[1]) <= disk[1]]


def build(forms, disks, sets, seed, y_off):
    rng = np.random.default_rng(seed)
    k0s, x0s = zip(*[camera_rays(inc, n, rng, y_off) for inc, n in sets])
    k0, x0 = np.concatenate(k0s), np.concatenate(x0s)
    n, F, D = len(k0), len(forms), len(disks)
    end = np.zeros((F, n, 6))
    flags = np.zeros((F, n), np.uint8)
    natt = np.zeros((F, n), np.uint32)
    nacc = np.zeros((F, n), np.uint32)
    cross = np.full((F, D, K, n, 6), np.nan)
    sens = np.full((F, D, K, n), np.nan)
    n_cross = np.zeros((F, D, n), np.uint8)
    keep = np.ones(n, bool)
    for i in range(n):
        for f, form in enumerate(forms):
            e, fl, na, nc, recs = solve(k0[i], x0[i], form)
            end[f, i], flags[f, i], natt[f, i], nacc[f, i] = e, fl, na, nc
            pert = [solve(kp, x0[i], form) for kp in perturbations(k0[i])]
            for d, disk in enumerate(disks):
                lay = layers(recs, disk)
                n_cross[f, d, i] = len(lay)
                for m, q in enumerate(lay[:K]):
                    cross[f, d, m, i] = q
                for pe in pert:
                    lp = layers(pe[4], disk)
                    if len(lp) != len(lay) or (pe[1], pe[2], pe[3]) != (fl, na, nc):
                        keep[i] = False
                        continue
                    for m, q in enumerate(lay[:K]):
                        mv = np.abs(lp[m] - q).max()
                        sens[f, d, m, i] = mv if np.isnan(sens[f, d, m, i]) else max(sens[f, d, m, i], mv)
        # between the forms: the same crossings, flags and step counts
        if F > 1 and not (np.all(n_cross[:, :, i] == n_cross[0, :, i]) and np.all(flags[:, i] == flags[0, i]) and
                          np.all(natt[:, i] == natt[0, i]) and np.all(nacc[:, i] == nacc[0, i])):
            keep[i] = False
    print(f"  {n} rays, {int((~keep).sum())} dropped")
    for d, disk in enumerate(disks):
        h = np.bincount(n_cross[0, d, keep], minlength=4)
        s = sens[0, d][:, keep]
        s = s[~np.isnan(s)]
        print(f"  disk {disk}: crossings 0/1/2/3+ = {h[0]}/{h[1]}/{h[2]}/{h[3:].sum()}, S_i median {np.median(s):.2e} max {s.max():.2e}")
    return dict(k0=k0[keep], x0=x0[keep], end=end[:, keep], flags=flags[:, keep], n_attempted=natt[:, keep],
                n_accepted=nacc[:, keep], cross=cross[..., keep, :], sens=sens[..., keep], n_cross=n_cross[..., keep],
                disks=np.array(disks), n_dropped=np.int64((~keep).sum()))


def main():
    print("Schwarzschild")
    g = build(("christoffel", "reduced"), SCHW_DISKS, ((85.0, 60), (60.0, 60), (17.0, 60)), 16, 0.0)
    np.savez_compressed(os.path.join(HERE, "disk_crossings.npz"), r_exit=35.0, max_step=np.inf, **PAR, **g)
    print("Kerr")
    g = build(("kerr",), KERR_DISKS, ((80.0, 40), (60.0, 40), (20.0, 40)), 17, 0.5)
    np.savez_compressed(os.path.join(HERE, "kerr_disk_crossings.npz"), max_step=np.inf, spin=KERR["a"], **PAR, **g)


if __name__ == "__main__":
    main()

"""Shared by the disk-crossings tests (tests/test_disk_crossings_host.py on the CPU, tests/test_gpu_crossings_oracle.py on the
GPU): the live scipy solve with the disk plane as a non-terminal event (what tests/golden/make_golden_crossings.py runs, with the
parameters left open), the 1-2 ulp perturbations of k0 and what they give -- a record's own movement S and whether a ray's counts
are stable -- and the ray sets.  Not a test module."""
import numpy as np

FORM_NAMES = ("christoffel", "reduced", "kerr")
NOWHERE = (1e300, 1e301)     # an annulus no crossing lies in: the solve's end, flags and counts are the disk-off trace's


def perturbations(k0):
    """tests/test_gpu_parity.py::_sensitivity's three patterns."""
    eps = np.finfo(float).eps
    return (np.nextafter(k0, np.inf), np.nextafter(k0, -np.inf), k0 * (1.0 + np.array([2.0, -2.0, 2.0]) * eps))


def scipy_solve(k0, x0, rhs_form, disk, r_s=1.0, spin=0.0, lambda_end=120.0, rtol=1e-3, atol=1e-6, max_step=np.inf, r_exit=0.0):
    """One ray through scipy: dict(end, flags, n_attempted, n_accepted, t_end, n_cross, cross [n_cross, 6], t_cross) -- the
    disk-off solve and every plane crossing inside the annulus that is not later than the terminal event."""
    from oracle import scipy_reference as sr
    if rhs_form == 2:
        assert r_exit == 0.0                     # (scipy_reference's Kerr solve has no exit sphere)
        r = sr.trace_ray_kerr(k0, x0, M=0.5 * r_s, a=spin, lambda_end=lambda_end, rtol=rtol, atol=atol, max_step=max_step, disk=NOWHERE)
    else:
        r = sr.trace_ray(k0, x0, r_s=r_s, form=FORM_NAMES[rhs_form], lambda_end=lambda_end, rtol=rtol, atol=atol, max_step=max_step,
                         r_exit=r_exit, disk=NOWHERE)
    out = dict(end=r["end"], flags=r["flags"], n_attempted=r["n_attempted"], n_accepted=r["n_accepted"], t_end=r["t_end"])
    recs, ts = [], []
    if "sol" in r:
        sol = r["sol"]
        for td, yd in zip(sol.t_events[-1], sol.y_events[-1]):
            if not td <= r["t_end"]:
                continue
            if rhs_form == 2:
                xc, kc = sr.bl_to_cart((yd[1], yd[3], yd[5]), (yd[0], yd[2], yd[4]), spin)
                q = np.concatenate([xc, kc])
            else:
                q = np.array([yd[1], yd[3], yd[5], yd[0], yd[2], yd[4]])
            if disk[0] <= np.hypot(q[0], q[1]) <= disk[1]:
                recs.append(q)
                ts.append(td)
    out.update(n_cross=len(recs), cross=np.array(recs).reshape(-1, 6), t_cross=np.array(ts))
    return out


def scipy_set(k0, x0, rhs_form, disk, K=4, **par):
    """scipy_solve over a ray set with its perturbations: dict of arrays like oracle.trace_crossings' (cross [K, n, 6]) plus
    sens [K, n] (a record's largest movement under the three perturbations) and stable [n] (counts, flags and step counts
    unchanged under them: the selection of make_golden_crossings.py, on the reference alone)."""
    k0 = np.atleast_2d(k0)
    n = len(k0)
    x0 = np.asarray(x0, float)
    out = dict(end=np.zeros((n, 6)), flags=np.zeros(n, np.uint8), n_attempted=np.zeros(n, np.uint32), n_accepted=np.zeros(n, np.uint32),
               t_end=np.zeros(n), n_cross=np.zeros(n, np.uint32), cross=np.full((K, n, 6), np.nan), t_cross=np.full((K, n), np.nan),
               sens=np.full((K, n), np.nan), stable=np.ones(n, bool))
    for i in range(n):
        xi = x0 if x0.ndim == 1 else x0[i]
        r = scipy_solve(k0[i], xi, rhs_form, disk, **par)
        for key in ("end", "flags", "n_attempted", "n_accepted", "t_end", "n_cross"):
            out[key][i] = r[key]
        m = min(K, r["n_cross"])
        out["cross"][:m, i] = r["cross"][:m]
        out["t_cross"][:m, i] = r["t_cross"][:m]
        out["sens"][:m, i] = 0.0
        for kp in perturbations(k0[i]):
            q = scipy_solve(kp, xi, rhs_form, disk, **par)
            if (q["n_cross"], q["flags"], q["n_attempted"], q["n_accepted"]) != (r["n_cross"], r["flags"], r["n_attempted"], r["n_accepted"]):
                out["stable"][i] = False
                continue
            out["sens"][:m, i] = np.maximum(out["sens"][:m, i], np.abs(q["cross"][:m] - r["cross"][:m]).max(1))
    return out


def oracle_sensitivity(oracle, k0, x0, ref, K, **kw):
    """The same two figures from the C oracle's crossings mode: (S [K, n], stable [n])."""
    S = np.where(np.isnan(ref["cross"][:K, :, 0]), np.nan, 0.0)
    stable = np.ones(len(ref["flags"]), bool)
    for kp in perturbations(np.asarray(k0, float)):
        q = oracle.trace_crossings(kp, x0, max_records=K, **kw)
        stable &= ((q["n_cross"] == ref["n_cross"]) & (q["flags"] == ref["flags"]) & (q["n_attempted"] == ref["n_attempted"]) &
                   (q["n_accepted"] == ref["n_accepted"]))
        S = np.fmax(S, np.abs(q["cross"][:K] - ref["cross"][:K]).max(2))      # (NaN where the reference has no record)
    # (a record the perturbed ray does not have moved by "no bound": the ray is not stable, and is left out by the callers)
    return S, stable


def camera_rays(x0, n, rng, r_s=1.0, b_max=6.0, critical=0.4):
    """make_golden_crossings.py's rays from any camera: the look-at direction plus (b / |x0|)(cos phi right + sin phi up), a share
    `critical` of them with b in [2.5, 2.7] r_s -- around 3 sqrt(3) / 2 r_s, where the higher-order images live -- the rest with b
    uniform in [0.5, b_max] r_s."""
    x0 = np.asarray(x0, float)
    d = np.linalg.norm(x0)
    look = -x0 / d
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, look)
    n_crit = int(round(critical * n))
    b = np.concatenate([rng.uniform(2.5, 2.7, n_crit), rng.uniform(0.5, b_max, n - n_crit)]) * r_s
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    k = look[None, :] + (b / d)[:, None] * (np.cos(phi)[:, None] * right[None, :] + np.sin(phi)[:, None] * up[None, :])
    return k / np.linalg.norm(k, axis=1)[:, None]


def exit_rays(x0, n, rng, r_lo=42.0, r_hi=75.0):
    """Half camera_rays, half aimed at points of the plane behind and beside the hole at radii r_lo ... r_hi (well clear of the
    hole, so that they arrive about there): with an exit sphere between the camera's radius and r_lo the second half leaves the
    sphere before it reaches the plane."""
    m = n // 2
    R, psi = rng.uniform(r_lo, r_hi, n - m), rng.uniform(0.6, 1.2, n - m) * rng.choice([-1.0, 1.0], n - m)
    back = -np.asarray(x0, float)[:2] / np.hypot(x0[0], x0[1])
    aim = np.stack([R * (back[0] * np.cos(psi) - back[1] * np.sin(psi)), R * (back[1] * np.cos(psi) + back[0] * np.sin(psi)), 0.0 * R], 1)
    far = aim - np.asarray(x0, float)
    return np.concatenate([camera_rays(x0, m, rng), far / np.linalg.norm(far, axis=1)[:, None]])


def inclined_camera(dist, incl_deg, y_off=0.0):
    inc = np.deg2rad(incl_deg)
    return np.array([dist * np.sin(inc), y_off, dist * np.cos(inc)])


# ---- the fixed cases of the issue ------------------------------------------------------------------------------------------
def tangent_ray(incl_deg=45.0, r_s=1.0):
    """A ray tangent to the photon sphere at (1.5 r_s, 0, 0), in a plane inclined incl_deg to the disk: it winds round and round."""
    a = np.deg2rad(incl_deg)
    return np.array([0.0, np.cos(a), np.sin(a)]), np.array([1.5 * r_s, 0.0, 0.0])


MANY = dict(r_s=1.0, lambda_end=200.0, disk_r_in=1.2, disk_r_out=15.0)
MANY_COUNTS = {1e-6: (5, 86), 1e-9: (7, 453), 1e-11: (9, 1391)}        # rtol: (crossings, attempted steps), measured with scipy

IN_PLANE_CAM = np.array([30.0, 0.0, 0.0])
IN_PLANE = dict(r_s=1.0, r_exit=35.0, lambda_end=120.0)
IN_PLANE_EVENTS = {2.0: 1, 2.6: 3, 4.0: 2, 8.0: 1}                       # b: scipy's plane events, the first at t = 0, R = 30
KERR_PLANE_CAM = np.array([10.0, 0.5, 0.0])
KERR_PLANE = dict(r_s=1.0, spin=0.45, rhs_form=2, lambda_end=50.0)
KERR_PLANE_EVENTS = {-0.3: 1, 0.3: 0, 0.0: 0}                            # k_z: scipy's plane events (at t = 0, R = 10.01)


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


# ---- the randomised draws --------------------------------------------------------------------------------------------------
FUZZ_SEED0 = 8000


def fuzz_draw(seed):
    """One randomised configuration of the crossings trace -> (k0 [n, 3], x0 [3] or [n, 3], K, oracle / library keywords).
    The form goes round with the seed (a third of the draws Kerr); everything else is drawn."""
    rng = np.random.default_rng(FUZZ_SEED0 + seed)
    rhs = seed % 3
    r_s = float(rng.choice([0.6, 1.0, 2.0]))
    kw = dict(r_s=r_s, rhs_form=rhs)
    if rhs == 2:
        kw["spin"] = float(rng.uniform(-0.98, 0.98)) * 0.5 * r_s
    dist = float(rng.uniform(6.0, 50.0)) * r_s
    # inclination from the +z axis: near-polar to within 1 degree of the plane, either side of it
    inc = float(rng.choice([rng.uniform(2.0, 60.0), rng.uniform(60.0, 89.0), rng.uniform(89.0, 89.9)]))
    if rng.random() < 0.5:
        inc = 180.0 - inc
    az = float(rng.uniform(0.0, 2.0 * np.pi))
    cam = dist * np.array([np.sin(np.deg2rad(inc)) * np.cos(az), np.sin(np.deg2rad(inc)) * np.sin(az), np.cos(np.deg2rad(inc))])
    if rhs == 2 and abs(cam[0]) + abs(cam[1]) < 0.05 * dist:      # keep Kerr off the polar axis (coordinate singularity)
        cam[0] += 0.2 * dist
    n = int(rng.integers(1, 1501))
    k0 = camera_rays(cam, n, rng, r_s=r_s, b_max=float(rng.uniform(4.0, 12.0)), critical=float(rng.uniform(0.1, 0.5)))
    r_in = float(rng.uniform(1.2, 5.0)) * r_s
    kw.update(lambda_end=float(rng.uniform(1.5, 3.0)) * dist, disk_r_in=r_in, disk_r_out=r_in * float(rng.uniform(1.5, 8.0)))
    mode = int(rng.integers(0, 3))
    if mode == 0:
        rtol = float(10 ** rng.uniform(-8, -2))
        kw.update(rtol=rtol, atol=rtol * float(10 ** rng.uniform(-4, -2)))
    elif mode == 1:
        kw["max_step"] = float(rng.uniform(0.1, 2.0)) * r_s
    if rng.random() < 0.4:
        kw["r_exit"] = float(rng.uniform(0.6, 1.4)) * dist
    if rng.random() < 0.25:
        kw["max_steps"] = int(rng.integers(1, 61))
    x0 = cam
    if rng.random() < 0.35:                                        # per-ray origins, every 7th inside the horizon
        x0 = cam[None, :] + rng.normal(size=(n, 3)) * (0.03 if rhs == 2 else 0.1) * dist
        x0[::7] = unit(rng.normal(size=3)) * 0.3 * r_s
    K = int(rng.integers(1, 5))
    return k0, x0, K, kw

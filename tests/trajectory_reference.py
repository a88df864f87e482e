"""Shared by the sampled-trajectory tests (tests/test_trajectory_host.py on the CPU, tests/test_gpu_trajectory_oracle.py on the
GPU): the C oracle's sampled curves together with the end state and step counts of its trace for the same parameters, a
sample's own movement S under the 1-2 ulp perturbations of k0 (crossings_reference.perturbations) with the rays whose counts
stay put under them, and the randomised draws.  Not a test module."""
import numpy as np

from crossings_reference import camera_rays, exit_rays, inclined_camera, perturbations, unit  # noqa: F401  (re-exported)

FORM_NAMES = ("christoffel", "reduced", "kerr", "timelike")
T_CHOICES = (2, 3, 63, 64, 65, 257, 1024)
MAX_SAMPLES = 300_000      # n * T of a draw: well under a second on either side
# restated from tests/test_gpu_parity.py (STATED["disk"], COND; tests/test_gpu_trajectory_oracle.py asserts that they are the same):
# the project's figures for a dense-output state -- a sample is one, like a crossing record
FLOOR = (1e-10, 1e-9)      # Cartesian forms, Kerr
COND = 500.0


def is_kerr(kw):
    return int(kw.get("rhs_form", 0)) == 2


def sample_bound(kw, S):
    """FLOOR + COND * S (Kerr: 10 COND, the crossings tests' figure), no bound where S is NaN or inf."""
    kerr = is_kerr(kw)
    return FLOOR[1 if kerr else 0] + COND * (10.0 if kerr else 1.0) * np.nan_to_num(S, nan=np.inf, posinf=np.inf)


def well_conditioned(kw, S):
    """The samples that move by no more than FLOOR / COND: on them the fixed part of the bound is at work."""
    with np.errstate(invalid="ignore"):
        return S <= FLOOR[1 if is_kerr(kw) else 0] / COND


def form_of(kw):
    """0 Christoffel, 1 reduced, 2 Kerr, 3 time-like (Christoffel): the four right-hand sides of the trajectory kernel."""
    return 3 if kw.get("time_like") else int(kw.get("rhs_form", 0))


def oracle_curves(oracle, k0, x0, T, **kw):
    """oracle.trajectory's (traj [n, 6, T], n_valid, flags) with oracle.trace's end, n_attempted, n_accepted, t_end (object_id
    with spheres) for the same parameters, as one dict.  The sampler is passive -- one step loop, samples read off its dense
    output -- so the two calls must end every ray alike."""
    traj, nv, fl = oracle.trajectory(k0, x0, T, **kw)
    o = oracle.trace(k0, x0, **kw)
    assert np.array_equal(fl, o["flags"]), "the oracle's sampler changed how a ray ends"
    out = dict(traj=traj, n_valid=nv, flags=fl, end=o["end"], n_attempted=o["n_attempted"], n_accepted=o["n_accepted"], t_end=o["t_end"])
    if "object_id" in o:
        out["object_id"] = o["object_id"]
    return out


def sample_sensitivity(oracle, k0, x0, T, ref, with_end=False, **kw):
    """(S [n, T], stable [n]): S the largest movement of each of the reference's samples under the three perturbations of k0
    (NaN: the reference has no such sample; inf: a sample that is not finite on either side, no bound), stable the rays whose
    flags, n_valid and both step counts do not move.  with_end: a third array, the same figure for the end state.

    Time-like starts get the same three patterns on x0 as well.  S stands for the growth of rounding noise of one ulp of the
    start STATE.  A null ray has |k0| = 1, and an ulp of k0 is that; a massive particle may start at |v0| = 0.01 at |x0| = 10,
    where an ulp of v0 is 1e-3 of the rounding of its first position update.  (Measured on the oracle alone, slow radial infall
    from r = 11 r_s, |v0| = 0.016: the samples near the horizon move by 4e-14 under the patterns on v0 and by 2.6e-10 under
    those on x0.)"""
    k0 = np.atleast_2d(np.asarray(k0, float))
    x0 = np.asarray(x0, float)
    have = np.arange(T)[None, :] < ref["n_valid"][:, None]
    S = np.where(have, 0.0, np.nan)
    S_end = np.zeros(len(k0))
    stable = np.ones(len(k0), bool)
    starts = [(kp, x0) for kp in perturbations(k0)]
    if kw.get("time_like"):
        starts += [(k0, xp) for xp in perturbations(x0)]
    for kp, xp in starts:
        q = oracle_curves(oracle, kp, xp, T, **kw)
        stable &= ((q["flags"] == ref["flags"]) & (q["n_valid"] == ref["n_valid"]) & (q["n_attempted"] == ref["n_attempted"]) &
                   (q["n_accepted"] == ref["n_accepted"]))
        with np.errstate(invalid="ignore"):
            d = np.abs(q["traj"] - ref["traj"]).max(1)
            de = np.abs(q["end"] - ref["end"]).max(1)
        d = np.where(have & np.isnan(d), np.inf, d)
        S = np.where(have, np.fmax(S, d), np.nan)
        S_end = np.fmax(S_end, np.where(np.isnan(de), np.inf, de))
    return (S, stable, S_end) if with_end else (S, stable)


def orbits(n, rng, r_s=1.0):
    """tests/test_gpu_parity.py::_orbits' massive-particle starts from a generator, in units of r_s: radii 2.5 ... 14 r_s,
    tangential speeds 0 ... 1.7 x circular, a radial part.  -> (v0 [n, 3], x0 [n, 3])"""
    x0 = rng.normal(size=(n, 3))
    r0 = rng.uniform(2.5, 14.0, n)
    x0 *= (r0 / np.linalg.norm(x0, axis=1))[:, None]
    e_r = x0 / r0[:, None]
    e_t = np.cross(e_r, rng.normal(size=(n, 3)))
    e_t /= np.linalg.norm(e_t, axis=1)[:, None]
    v = np.sqrt(0.5 / np.maximum(r0 - 1.5, 0.8)) * rng.uniform(0.0, 1.7, n)
    return v[:, None] * e_t + rng.normal(0.0, 0.08, n)[:, None] * e_r, x0 * r_s


def shape_of(n, T):
    """The launch shape bhg_trajectory picks: one lane per ray above 2048 rays, else one wave per ray -- four waves for
    <= 64 rays with >= 1024 samples."""
    return "lane" if n > 2048 else ("wave4" if n <= 64 and T >= 1024 else "wave")


# ---- the randomised draws --------------------------------------------------------------------------------------------------
FUZZ_SEED0 = 17000
N_RANGES = ((1, 64), (65, 2048), (2049, 2200))


def fuzz_draw(seed):
    """One randomised configuration of the sampled trace -> (k0 [n, 3], x0 [3] or [n, 3], T, oracle / library keywords; spheres
    among them when the draw has some).  The form goes round with the seed over the four right-hand sides and the ray count's
    range (1 ... 64, 65 ... 2048, 2049 ... 2200: the three launch shapes) with seed // 4; everything else is drawn."""
    rng = np.random.default_rng(FUZZ_SEED0 + seed)
    form = seed % 4
    timelike = form == 3
    r_s = float(rng.choice([0.6, 1.0, 2.0]))
    kw = dict(r_s=r_s, rhs_form=0 if timelike else form)
    if timelike:
        kw["time_like"] = 1
    if form == 2:
        kw["spin"] = float(rng.uniform(-0.98, 0.98)) * 0.5 * r_s
    lo, hi = N_RANGES[(seed // 4) % 3]
    n = int(rng.integers(lo, hi + 1))
    fits = [t for t in T_CHOICES if n * t <= MAX_SAMPLES]
    T = int(rng.choice(fits))
    if hi == 64 and rng.random() < 0.5:
        T = 1024                                                  # (the four-wave shape needs <= 64 rays with >= 1024 samples)
    if timelike:
        k0, x0 = orbits(n, rng, r_s)
        dist = 14.0 * r_s
        cam = None
        kw["lambda_end"] = float(rng.uniform(40.0, 150.0)) * r_s
    else:
        dist = float(rng.uniform(6.0, 50.0)) * r_s
        # inclination from the +z axis: 2 degrees off the axis to 0.1 degree off the plane, either side of it
        inc = float(rng.choice([rng.uniform(2.0, 60.0), rng.uniform(60.0, 89.0), rng.uniform(89.0, 89.9)]))
        if rng.random() < 0.5:
            inc = 180.0 - inc
        az = float(rng.uniform(0.0, 2.0 * np.pi))
        cam = dist * np.array([np.sin(np.deg2rad(inc)) * np.cos(az), np.sin(np.deg2rad(inc)) * np.sin(az), np.cos(np.deg2rad(inc))])
        if form == 2 and abs(cam[0]) + abs(cam[1]) < 0.05 * dist:      # keep Kerr off the polar axis (coordinate singularity)
            cam[0] += 0.2 * dist
        k0 = camera_rays(cam, n, rng, r_s=r_s, b_max=float(rng.uniform(4.0, 12.0)), critical=float(rng.uniform(0.1, 0.5)))
        kw["lambda_end"] = float(rng.uniform(1.5, 3.0)) * dist
        x0 = cam
    if rng.random() < 0.35:
        h = float(rng.uniform(0.05, 0.5)) * r_s
        kw.update(method=1, h_fixed=h, lambda_end=min(kw["lambda_end"], 600.0 * h))      # (at most 600 fixed steps a ray)
    else:
        mode = int(rng.integers(0, 3))
        if mode == 0:
            rtol = float(10 ** rng.uniform(-8, -2))
            kw.update(rtol=rtol, atol=rtol * float(10 ** rng.uniform(-4, -2)))
        elif mode == 1:
            kw["max_step"] = float(rng.uniform(0.1, 2.0)) * r_s
    if rng.random() < 0.4:
        kw["r_exit"] = float(rng.uniform(0.6, 1.4)) * dist
    if rng.random() < 0.4:
        r_in = float(rng.uniform(1.2, 5.0)) * r_s
        kw.update(disk_r_in=r_in, disk_r_out=r_in * float(rng.uniform(1.5, 8.0)))
    if rng.random() < 0.35:
        sph = []
        for _ in range(int(rng.integers(1, 3))):
            if timelike:
                c = unit(rng.normal(size=3)) * float(rng.uniform(4.0, 12.0)) * r_s
            else:     # between the camera and the hole, a little off the line of sight
                c = cam * float(rng.uniform(0.25, 0.7)) + rng.normal(size=3) * 1.5 * r_s
            sph.append([float(c[0]), float(c[1]), float(c[2]), float(rng.uniform(0.5, 2.0)) * r_s])
        kw["spheres"] = sph
    if rng.random() < 0.25:
        kw["max_steps"] = int(rng.integers(1, 61))
    if timelike or rng.random() < 0.35:                            # per-ray origins, every 7th inside the horizon
        if not timelike:
            x0 = cam[None, :] + rng.normal(size=(n, 3)) * (0.03 if form == 2 else 0.1) * dist
        if not timelike or rng.random() < 0.5:
            x0[::7] = unit(rng.normal(size=3)) * 0.3 * r_s
    return k0, x0, T, kw

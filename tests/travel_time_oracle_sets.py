"""Shared by tests/test_travel_time_oracle_host.py (CPU) and tests/test_gpu_travel_time_oracle.py (GPU): what the C oracle's
coordinate time (oracle.travel_time; DESIGN.md section 18, "Held to the oracle") gives on a ray set -- its times, each time's own
movement S_i under the three 1-2 ulp perturbations of k0, who is left out, the tolerance -- and the ray sets themselves, so that the
oracle alone decides who is compared and both files speak of the same rays.  Not a test module.

The criterion (section 18's, computed from the oracle alone; no new tolerance):
    |t_dev - t_oracle| <= max(COND * S_i, floor),   floor = COND * median(S_i) over the set's finite times,   COND = 500.
A ray is left out when its flags, step counts, n_cross or the inf / NaN pattern of its times change under a perturbation in the
oracle: at most LEFT_OUT_SET of a set, at most LEFT_OUT_DRAWS over the twelve default draws."""
import numpy as np

import crossings_reference as cx
from travel_time_reference import COND

FORM_IDS = ("christoffel", "reduced", "kerr")
LEFT_OUT_SET, LEFT_OUT_DRAWS = 0.10, 0.02
N_DRAWS = 12


def times_of(o):
    """[1 + K, n]: row 0 the end time, rows 1 ... the crossing times (NaN where the oracle has no record)."""
    return np.concatenate([o["dt_end"][None, :], o["dt_cross"]])


def pattern(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    return np.where(np.isnan(t), 3, np.where(np.isposinf(t), 1, np.where(np.isneginf(t), 2, 0))).astype(np.int8)


def reference(oracle, k0, x0, K, **kw):
    """The oracle on a ray set with its three perturbations: dict(o = oracle.travel_time's result, t [1 + K, n] = times_of(o),
    S [1 + K, n] the largest movement of each finite time (NaN elsewhere), S_rec [K, n] that of each record (as
    crossings_reference.oracle_sensitivity), stable [n], fin [1 + K, n] = the finite times of stable rays, floor, tol [1 + K, n])."""
    k0 = np.ascontiguousarray(k0, dtype=np.float64)
    o = oracle.travel_time(k0, x0, K, **kw)
    t = times_of(o)
    S = np.where(np.isfinite(t), 0.0, np.nan)
    S_rec = np.where(np.isnan(o["cross"][:, :, 0]), np.nan, 0.0)
    stable = np.ones(len(k0), bool)
    for kp in cx.perturbations(k0):
        q = oracle.travel_time(kp, x0, K, **kw)
        tq = times_of(q)
        stable &= ((q["n_cross"] == o["n_cross"]) & (q["flags"] == o["flags"]) & (q["n_attempted"] == o["n_attempted"]) &
                   (q["n_accepted"] == o["n_accepted"]) & np.all(pattern(tq) == pattern(t), axis=0))
        with np.errstate(invalid="ignore"):
            S = np.fmax(S, np.where(np.isfinite(t) & np.isfinite(tq), np.abs(tq - t), np.nan))
            S_rec = np.fmax(S_rec, np.abs(q["cross"] - o["cross"]).max(2))
    fin = np.isfinite(t) & stable[None, :]
    floor = COND * float(np.median(S[fin])) if fin.any() else 0.0
    with np.errstate(invalid="ignore"):
        tol = np.maximum(COND * S, floor)
    return dict(o=o, t=t, S=S, S_rec=S_rec, stable=stable, fin=fin, floor=floor, tol=tol)


def case_reference(oracle, case):
    """reference() of one of the sets below.  A set that is run at several record depths (its 7th entry: the other depths) is
    ONE set: its floor is the median over the finite times of all its runs."""
    label, k0, x0, K, kw, mode = case[:6]
    r = reference(oracle, k0, x0, K, **kw)
    if len(case) > 6:
        S = [r["S"][r["fin"]]]
        for K_other in case[6]:
            q = reference(oracle, k0, x0, K_other, **kw)
            S.append(q["S"][q["fin"]])
        r["floor"] = COND * float(np.median(np.concatenate(S)))
        with np.errstate(invalid="ignore"):
            r["tol"] = np.maximum(COND * r["S"], r["floor"])
    return r


# ---- the sets: (label, k0, x0, K, kw, mode); mode is test_gpu_crossings_oracle._same_steps' ---------------------------------
def _mode(rhs):
    return "kerr" if rhs == 2 else "exact"


def draw(seed):
    """a. one randomised configuration (crossings_reference.fuzz_draw)."""
    k0, x0, K, kw = cx.fuzz_draw(seed)
    return f"draw {seed}", k0, x0, K, kw, "fuzz"


ACROSS_SETTINGS = ((1e-3, 30.0), (1e-2, 30.0), (1e-2, 60.0))


def across_the_hole(rhs, rtol, dist, n=1000):
    """b. rays aimed at the hole, impact parameter uniform in [0, 0.6] r_s: at loose tolerances many of them step across it."""
    cam = cx.inclined_camera(dist, 70.0, 0.5)
    rng = np.random.default_rng(77)
    look = -cam / np.linalg.norm(cam)
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, look)
    b, phi = rng.uniform(0.0, 0.6, n), rng.uniform(0.0, 2.0 * np.pi, n)
    k0 = look[None, :] + (b / np.linalg.norm(cam))[:, None] * (np.cos(phi)[:, None] * right[None, :] + np.sin(phi)[:, None] * up[None, :])
    k0 /= np.linalg.norm(k0, axis=1)[:, None]
    kw = dict(r_s=1.0, rhs_form=rhs, r_exit=1.2 * dist, lambda_end=3.0 * dist, rtol=rtol, atol=1e-3 * rtol, disk_r_in=1.2, disk_r_out=15.0)
    return f"across rtol={rtol:g} dist={dist:g}", k0, cam, 2, kw, "exact"


KERR_EXIT_SPINS = (0.45, -0.45, 0.2)


def kerr_exit(spin, n=1500):
    """c. Kerr with an exit sphere: tests/test_gpu_disk_crossings.py's inclined rays and parameters."""
    from test_gpu_disk_crossings import CAM, _inclined_rays, _kw
    return f"kerr exit spin={spin:g}", _inclined_rays(n), CAM, 2, _kw(2, spin), "kerr"


def wave_size(rhs, spin, n):
    """d. test_gpu_crossings_oracle.test_wave_sizes_with_mixed_origins' rays."""
    rng = np.random.default_rng(40 + n)
    cam = cx.inclined_camera(30.0, 70.0, y_off=0.5)
    k0 = cx.camera_rays(cam, n, rng)
    x0 = cam[None, :] + rng.normal(size=(n, 3)) * 2.0
    x0[::7] = rng.normal(size=(len(x0[::7]), 3)) * 0.15            # inside the horizon, the last ray of 64 and 65 among them
    x0[-1] = x0[0] if n == 63 else x0[-1] * 0.0 + [0.1, 0.05, 0.2]
    kw = dict(r_s=1.0, lambda_end=100.0, r_exit=45.0, rhs_form=rhs, spin=spin, disk_r_in=1.2, disk_r_out=15.0)
    return f"n={n}", k0, x0, 3, kw, _mode(rhs)


MANY_K = (4, 2)


def many_crossings(rhs, rtol, K):
    """e. the 64 tangent rays: more crossings than records.  They start in the plane, so each ray's first crossing time is 0 with
    S = 0: at K = 2 that is half the finite times, the median of S is 0 and the floor with it -- and a time whose three
    perturbations happen to move it by nothing (3 of 128 in one run) would have to be met bit for bit by a kernel that contracts
    to FMAs where the oracle does not.  The oracle's times do not depend on K, and neither does what the floor is there for: the
    set is the 64 rays at one rtol, run at K = 4 and K = 2, and its floor is taken over the finite times of both runs."""
    rays = [cx.tangent_ray(a) for a in np.linspace(10.0, 80.0, 64)]
    k0, x0 = np.array([r[0] for r in rays]), rays[0][1]
    return (f"tangent rtol={rtol:g} K={K}", k0, x0, K, dict(rtol=rtol, atol=rtol * 1e-3, rhs_form=rhs, **cx.MANY), "exact",
            tuple(k for k in MANY_K if k != K))


PLANE_DISKS = ((1e-3, 1e3), (3.0, 30.0), (3.0, 12.0))


PLANE_MORE_B = (3.0, 5.0, 6.0)


def plane_starts(form, disk):
    """f. the starts in the disk plane of test_gpu_crossings_oracle.PLANE_CASES, one form's cases as one set (rays are
    independent; together they give the floor a median to stand on) -> the set and each case's plane-event count (None: not
    stated).  The Schwarzschild case that starts in the plane AND points along it (k_z = 0) is left out by the rule: nextafter
    turns its k_z into a denormal and the ray leaves the plane.  It is one ray of nine, so the Schwarzschild sets get six more
    rays of the same kind (b = 3, 5, 6 r_s, either side) and the 10 % cap holds as stated."""
    from test_gpu_crossings_oracle import PLANE_CASES
    cases = [c for c in PLANE_CASES if c[3]["rhs_form"] == form]
    kw = dict(cases[0][3], disk_r_in=disk[0], disk_r_out=disk[1])
    assert all(c[3] == cases[0][3] for c in cases)
    k0, x0, events = [c[1] for c in cases], [c[2] for c in cases], [c[4] for c in cases]
    if form != 2:
        for b in PLANE_MORE_B:
            for sign in (1.0, -1.0):
                k0.append(cx.unit([-1.0, 0.0, sign * b / 30.0]))
                x0.append(cx.IN_PLANE_CAM)
                events.append(None)
    return (f"plane {disk}", np.array(k0), np.array(x0), 4, kw, "exact"), events


BUDGETS = (1, 13, 16)


def step_budget(rhs, spin, budget):
    """g. test_gpu_crossings_oracle.test_step_budget_after_crossings' 300 rays."""
    cam = cx.inclined_camera(30.0, 80.0, y_off=0.5)
    k0 = cx.camera_rays(cam, 300, np.random.default_rng(9))
    kw = dict(r_s=1.0, lambda_end=120.0, rhs_form=rhs, spin=spin, disk_r_in=1.2, disk_r_out=15.0, max_steps=budget)
    return f"max_steps={budget}", k0, cam, 2, kw, _mode(rhs)


FORMS = ((0, 0.0), (1, 0.0), (2, 0.45))


def fixed_sets():
    """Every fixed set (b ... g), for the host file's caps."""
    for rhs in (0, 1):
        for rtol, dist in ACROSS_SETTINGS:
            yield across_the_hole(rhs, rtol, dist)
    for spin in KERR_EXIT_SPINS:
        yield kerr_exit(spin)
    for rhs, spin in FORMS:
        for n in (63, 64, 65):
            yield wave_size(rhs, spin, n)
        for disk in PLANE_DISKS:
            yield plane_starts(rhs, disk)[0]
        for budget in BUDGETS:
            yield step_budget(rhs, spin, budget)
    for rhs in (0, 1):
        for rtol in (1e-6, 1e-9):
            for K in (2, 4):
                yield many_crossings(rhs, rtol, K)

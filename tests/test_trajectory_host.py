"""The reference of the sampled-trajectory tests held to scipy, on the CPU: oracle.trajectory against live solve_ivp with t_eval in
all four right-hand sides (both Schwarzschild forms, time-like, Kerr -- scipy_reference.trace_ray_kerr(nr_points_curve=)), the
fixed cases that pin WHICH samples a ray emits (a grid that is the step grid, T = 2, a step budget), and the quality of the
randomised draws tests/test_gpu_trajectory_oracle.py runs on the GPU: what they must have so that the GPU test cannot quietly
compare nothing.

The bound on a sample is trajectory_reference.sample_bound: FLOOR + COND * S, S the sample's own movement in the oracle under the
three 1-2 ulp perturbations of k0 -- the GPU test's bound.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_reference as tr  # noqa: E402

CAM = tr.inclined_camera(20.0, 70.0, y_off=0.5)
T_ROUND = (2, 50, 257)
SETTINGS = [("plain", {}), ("r_s=2", dict(r_s=2.0)), ("rtol=1e-6", dict(rtol=1e-6, atol=1e-9)), ("max_step=0.5", dict(max_step=0.5)),
            ("exit sphere", dict(r_exit=25.0)), ("per-ray origins", dict(origins=True))]
N_RAYS = 40


def _rays(form, setting, seed):
    rng = np.random.default_rng(seed)
    kw = dict(setting)
    r_s = kw.get("r_s", 1.0)
    if form == 3:
        k0, x0 = tr.orbits(N_RAYS, rng, r_s)
        kw.pop("origins", None)
        kw.setdefault("lambda_end", 60.0)
    else:
        cam = CAM * r_s
        k0 = tr.camera_rays(cam, N_RAYS, rng, r_s=r_s)
        x0 = cam[None, :] + rng.normal(size=(N_RAYS, 3)) * 2.0 if kw.pop("origins", False) else cam
        kw.setdefault("lambda_end", 45.0 * r_s)
    if "r_exit" in kw:
        kw["r_exit"] = kw["r_exit"] * r_s
    return k0, x0, kw


def _hold_to_scipy(oracle, form, k0, x0, T, kw, curve_of):
    """Every ray: scipy's sample count, and every sample within the bound of scipy's."""
    full = dict(kw, rhs_form=min(form, 2) if form != 3 else 0, time_like=int(form == 3))
    ref = tr.oracle_curves(oracle, k0, x0, T, **full)
    S, stable = tr.sample_sensitivity(oracle, k0, x0, T, ref, **full)
    tol = tr.sample_bound(full, S)
    worst = 0.0
    for i in range(len(k0)):
        flags, curve = curve_of(k0[i], x0 if np.ndim(x0) == 1 else x0[i])
        m = curve.shape[1]
        assert flags == ref["flags"][i]
        assert m == ref["n_valid"][i], (i, m, int(ref["n_valid"][i]))
        d = np.abs(curve - ref["traj"][i, :, :m]).max(0)
        assert np.all(d <= tol[i, :m]), (i, float(np.max(d - tol[i, :m])))
        assert np.isnan(ref["traj"][i, :, m:]).all()
        worst = max(worst, float(d.max(initial=0.0)))
    assert (ref["n_valid"] == T).any()
    return worst, ref


@pytest.mark.parametrize("si", range(len(SETTINGS)), ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("form", [0, 1, 3], ids=["christoffel", "reduced", "timelike"])
def test_schwarzschild_samples_against_live_scipy(oracle, form, si):
    from oracle import scipy_reference as sr
    T = T_ROUND[(si + form) % 3]
    k0, x0, kw = _rays(form, SETTINGS[si][1], 100 + 10 * si + form)

    def curve_of(k, x):
        r = sr.trace_ray(k, x, form="reduced" if form == 1 else "christoffel", time_like=form == 3, nr_points_curve=T, **kw)
        return r["flags"], r["sol"].y[[1, 3, 5, 0, 2, 4]]

    worst, ref = _hold_to_scipy(oracle, form, k0, x0, T, kw, curve_of)
    print(f"{tr.FORM_NAMES[form]} {SETTINGS[si][0]} T={T}: worst |oracle - scipy| {worst:.3e}, flags {np.unique(ref['flags'])}")


@pytest.mark.parametrize("name,setting,T", [("plain", {}, 50), ("rtol=1e-6", dict(rtol=1e-6, atol=1e-9), 257), ("max_step=0.5", dict(max_step=0.5), 2)],
                         ids=["plain", "rtol=1e-6", "max_step=0.5"])
@pytest.mark.parametrize("spin", [0.45, -0.3])
def test_kerr_samples_against_live_scipy(oracle, spin, name, setting, T):
    """scipy integrates in Boyer-Lindquist coordinates and its samples are converted with bl_to_cart; the oracle's by its own."""
    from oracle import scipy_reference as sr
    k0, x0, kw = _rays(2, setting, 200 + T)
    kw["lambda_end"] = 40.0

    def curve_of(k, x):
        r = sr.trace_ray_kerr(k, x, M=0.5, a=spin, nr_points_curve=T, **kw)
        return r["flags"], r["curve"]

    worst, ref = _hold_to_scipy(oracle, 2, k0, x0, T, dict(kw, spin=spin), curve_of)
    print(f"kerr a={spin} {name} T={T}: worst |oracle - scipy| {worst:.3e}, flags {np.unique(ref['flags'])}")


# ---- fixed cases -----------------------------------------------------------------------------------------------------------
FORM_KW = [dict(rhs_form=0), dict(rhs_form=1), dict(rhs_form=2, spin=0.45), dict(rhs_form=0, time_like=1)]
GRID = dict(method=1, h_fixed=0.25, lambda_end=40.0)      # T = 161: dt = 0.25 = h_fixed, every sample on a step end


def grid_rays(form, n, seed=5):
    rng = np.random.default_rng(seed)
    if form == 3:
        return tr.orbits(n, rng)
    cam = tr.inclined_camera(15.0, 70.0, y_off=0.5)
    return tr.camera_rays(cam, n, rng), cam


@pytest.mark.parametrize("form", range(4), ids=tr.FORM_NAMES)
def test_a_grid_on_the_step_ends_gives_the_step_end_states(oracle, form):
    """RK4 with h = 0.25 to lambda_end = 40 sampled at T = 161: te_j = j h is where step j ends (all of these are exact in
    binary), so every sample sits on the sampler's te <= t comparison and must be there, and it is the state the trace passes
    through after j steps -- what the trace with a budget of j steps ends on."""
    k0, x0 = grid_rays(form, 24)
    kw = dict(GRID, **FORM_KW[form])
    ref = tr.oracle_curves(oracle, k0, x0, 161, **kw)
    ran = ref["flags"] == 4
    assert ran.sum() >= 8 and np.all(ref["n_valid"][ran] == 161) and np.all(ref["n_accepted"][ran] == 160)
    # (Kerr: a fixed step through the Boyer-Lindquist horizon leaves garbage for the root search -- tests/test_gpu_parity.py's
    # fixed-step horizon / NaN allowance -- so its horizon rays are not asked where they end)
    early = np.isin(ref["flags"], (8, 128)) | ((ref["flags"] == 1) & (form != 2))
    assert np.array_equal(ref["n_valid"][early], np.floor(ref["t_end"][early] / 0.25).astype(int) + 1)
    xs = np.broadcast_to(x0, k0.shape)
    assert np.abs(ref["traj"][:, :, 0] - np.concatenate([xs, k0], 1)).max() < 1e-12
    for j in range(1, 161):
        there = ref["n_valid"] > j
        step = oracle.trace(k0, x0, max_steps=j, **kw)
        with np.errstate(invalid="ignore"):      # (Kerr: a fixed step that jumped the 1 / Delta singularity left garbage, 1e50 and NaN)
            there &= np.abs(step["end"]).max(1) < 1e6
        assert np.all(step["n_accepted"][there] == j)
        scale = np.maximum(1.0, np.abs(step["end"][there]).max(1, initial=0.0))
        assert np.all(np.abs(ref["traj"][there, :, j] - step["end"][there]).max(1, initial=0.0) <= 1e-13 * scale), j


@pytest.mark.parametrize("form", range(4), ids=tr.FORM_NAMES)
def test_two_samples_are_the_start_and_the_end(oracle, form):
    """T = 2, the smallest the C layer accepts: dt = lambda_end.  Sample 0 is the start state, sample 1 -- on a ray that runs
    to lambda_end -- the end state; a ray that ends early has the one sample."""
    k0, x0 = grid_rays(form, 60, seed=6)
    for extra in (dict(lambda_end=40.0), dict(GRID)):
        kw = dict(extra, **FORM_KW[form])
        ref = tr.oracle_curves(oracle, k0, x0, 2, **kw)
        ran = ref["flags"] == 4
        assert ran.sum() >= 10 and (form == 3 or (~ran).sum() >= 3)
        assert np.all(ref["n_valid"][ran] == 2) and np.all(ref["n_valid"][~ran] == 1)
        xs = np.broadcast_to(x0, k0.shape)
        start = np.concatenate([xs, k0], 1)
        tol = 1e-12 if form == 2 else 0.0          # (Kerr: there and back through Boyer-Lindquist coordinates)
        assert np.abs(ref["traj"][:, :, 0] - start).max() <= tol
        assert np.abs(ref["traj"][ran, :, 1] - ref["end"][ran]).max() <= 1e-12
        assert np.isnan(ref["traj"][~ran, :, 1]).all()


@pytest.mark.parametrize("budget", [1, 13, 16])
@pytest.mark.parametrize("form", range(4), ids=tr.FORM_NAMES)
def test_a_budget_stopped_ray_emits_the_samples_up_to_its_last_accepted_step(oracle, form, budget):
    k0, x0 = grid_rays(form, 60, seed=7)
    T = 257
    kw = dict(lambda_end=60.0, max_steps=budget, **FORM_KW[form])
    ref = tr.oracle_curves(oracle, k0, x0, T, **kw)
    cut = ref["flags"] == 16
    assert cut.sum() >= 10 and np.all(ref["n_attempted"][cut] == budget)       # (the orbits are the smoothest: 13 at 16 steps)
    t_eval = np.arange(T) * (60.0 / (T - 1))
    t_eval[-1] = 60.0
    want = (t_eval[None, :] <= ref["t_end"][:, None]).sum(1)
    assert np.array_equal(ref["n_valid"], want)
    assert np.all(ref["n_valid"][cut] >= 1) and np.all(ref["n_valid"][cut] < T)
    # the last sample does not lie beyond the end state: from it the ray still has t_end - te to go
    last = ref["traj"][cut, :, :][np.arange(cut.sum()), :, ref["n_valid"][cut] - 1]
    gap = ref["t_end"][cut] - t_eval[ref["n_valid"][cut] - 1]
    speed = np.linalg.norm(ref["end"][cut, 3:6], axis=1) + np.linalg.norm(last[:, 3:6], axis=1)
    assert np.all(np.linalg.norm(last[:, 0:3] - ref["end"][cut, 0:3], axis=1) <= gap * speed + 1e-12)


# ---- the quality of the randomised draws, on the oracle alone --------------------------------------------------------------
def test_randomised_draws_are_stable_and_well_conditioned(oracle):
    """The twelve default draws of tests/test_gpu_trajectory_oracle.py: each keeps >= 99 % of its rays stable under the
    perturbations, over them >= 100 samples per form move by no more than FLOOR / COND, every form meets every range of the ray
    count, all three launch shapes and both methods occur."""
    tight, seen, methods = [0, 0, 0, 0], set(), set()
    for seed in range(12):
        k0, x0, T, kw = tr.fuzz_draw(seed)
        assert len(k0) * T <= tr.MAX_SAMPLES
        ref = tr.oracle_curves(oracle, k0, x0, T, **kw)
        S, stable = tr.sample_sensitivity(oracle, k0, x0, T, ref, **kw)
        assert stable.mean() >= 0.99, (seed, float(stable.mean()))
        form = tr.form_of(kw)
        t = int((tr.well_conditioned(kw, S) & stable[:, None]).sum())
        tight[form] += t
        seen.add((form, tr.shape_of(len(k0), T) == "lane", len(k0) <= 64))
        seen.add(tr.shape_of(len(k0), T))
        methods.add(kw.get("method", 0))
        print(f"draw {seed}: {tr.FORM_NAMES[form]} n {len(k0)} T {T} {tr.shape_of(len(k0), T)}, stable {stable.mean():.4f}, samples "
              f"{int(ref['n_valid'].sum())}, with S <= floor / COND {t}")
    assert min(tight) >= 100, tight
    assert {"lane", "wave", "wave4"} <= seen and methods == {0, 1}
    for form in range(4):
        assert {(form, True, False), (form, False, True), (form, False, False)} <= seen

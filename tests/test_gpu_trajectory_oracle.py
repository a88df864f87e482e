"""bhg_trajectory / bhg_trajectory_objects (trajectory_dp54_kernel) against the C oracle's sampler (oracle.trajectory; held on the
CPU to live scipy with t_eval in all four right-hand sides by tests/test_trajectory_host.py), on every ray and every sample:
randomised configurations, the ray counts and sample counts at which the launch shape or the sample pass changes, grids whose
samples fall on step ends, step budgets, time-like orbits, Kerr with spheres and the disk, and non-finite directions.

What is asked of a comparison (_hold, the one rule of every test here):
  * flags: the oracle's, exactly; Kerr with fixed steps: tests/test_gpu_parity.py's horizon / NaN allowance, nothing wider (a
    fixed step through the Boyer-Lindquist horizon: whether the crossing is seen before the state turns NaN is rounding, and
    what such a ray samples on the way is garbage on both sides, 1e50 and NaN -- as in test_trajectories_with_fixed_step_rk4, a
    ray that either side calls horizon or NaN must be called horizon and / or NaN by both, and its samples are not compared;
    such rays are counted and printed);
  * object ids: the oracle's; a ray that starts inside the horizon: flags 3, no sample, the Cartesian input as its end;
  * n_valid: the oracle's on every ray that is stable in the oracle (flags, n_valid and both step counts unmoved by the three
    1-2 ulp perturbations of k0) and whose flags and step counts from ctx.trace with the same parameters are the oracle's (the
    trajectory call returns no step counts).  Stable rays this leaves out are counted and printed: none in the Cartesian forms, at
    most 1 % of a Kerr case;
  * every valid sample of every such ray within FLOOR + COND * S of the oracle's (trajectory_reference.sample_bound: STATED["disk"]
    and COND of tests/test_gpu_parity.py, Kerr 10 COND as in the crossings tests), S the sample's own movement in the oracle under
    the perturbations; samples beyond n_valid are NaN on every ray;
  * the end state within STATED[class] + COND * S_end of the oracle's.
Each case prints (form, method, shape, n, T) and its figures before it asserts.

Measured on an MI355X (the whole file, profiles/r17_trajectory_oracle_tests.log): see DESIGN.md, "Sampled trajectories held to the
oracle".
"""
import os

import numpy as np
import pytest

import trajectory_reference as tr
from test_gpu_parity import COND, STATED, _orbits

pytestmark = pytest.mark.gpu

FORM_IDS = list(tr.FORM_NAMES)
FORM_KW = [dict(rhs_form=0), dict(rhs_form=1), dict(rhs_form=2, spin=0.45), dict(rhs_form=0, time_like=1)]
STATS = {}          # per form, over the run
COVERED = {}        # (form, method, shape): samples compared
CAM = tr.inclined_camera(30.0, 70.0, y_off=0.5)


def test_the_bound_is_the_projects_own():
    assert tr.FLOOR == STATED["disk"] and tr.COND == COND


@pytest.fixture(scope="module", autouse=True)
def _totals():
    yield
    print("\ntrajectory totals, per form:")
    for form, st in STATS.items():
        print(f"  {form}: {st}")
    print("samples compared per (form, method, shape):")
    for key in sorted(COVERED):
        print(f"  {key}: {COVERED[key]}")


def _params(**kw):
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi.make_params(**kw)


def _end_bound(flags, kerr):
    """STATED by class of ray; a ray that stops on a step end (budget, step too small) is held like one that runs to the end,
    a Kerr ray that ends on a sphere like one that ends on the disk (both are roots on the step's dense output)."""
    col = 1 if kerr else 0
    b = np.full(len(flags), STATED["escaped"][col])
    b[(flags & 1) != 0] = STATED["horizon"][col]
    b[flags == 128] = STATED["disk"][col]
    b[flags == 0x88] = STATED["object"][col] if not kerr else STATED["disk"][col]
    return b


def _hold(ctx, oracle, k0, x0, T, kw, label="", apart=None):
    """Device against oracle on one ray set, every ray and every sample.  apart: rays the caller checks itself (non-finite input)."""
    k0 = np.ascontiguousarray(k0, dtype=np.float64)
    n = len(k0)
    kerr, form, fixed = tr.is_kerr(kw), tr.form_of(kw), kw.get("method", 0) == 1
    spheres = kw.get("spheres")
    lib = {a: b for a, b in kw.items() if a != "spheres"}
    shape = tr.shape_of(n, T)
    case = (FORM_IDS[form], "rk4" if fixed else "dp54", shape, n, T)
    ref = tr.oracle_curves(oracle, k0, x0, T, **kw)
    S, stable, S_end = tr.sample_sensitivity(oracle, k0, x0, T, ref, with_end=True, **kw)
    got = ctx.trajectory(k0, x0, _params(**lib), T, spheres=spheres)
    traj, nv, end, flags = got[:4]
    traced = ctx.trace(k0, x0, _params(**lib), spheres=spheres)
    steps, acc = traced[2], traced[3]
    asked = np.ones(n, bool) if apart is None else ~apart
    ofl = ref["flags"]
    same_fl = flags == ofl
    allowance = (((flags | ofl) & np.uint8(1 | 64)) != 0) & (ofl != 3) if kerr and fixed else np.zeros(n, bool)
    mine = asked & ~allowance
    same = same_fl & (traced[1] == ofl) & (steps == ref["n_attempted"]) & (acc == ref["n_accepted"])
    compared = mine & stable & same
    left_out = mine & stable & ~same
    have = np.arange(T)[None, :] < nv[:, None]
    with np.errstate(invalid="ignore"):
        diff = np.abs(traj - ref["traj"]).max(1)
        d_end = np.abs(end - ref["end"]).max(1)
    floor = tr.FLOOR[1 if kerr else 0]
    tol = tr.sample_bound(kw, S)
    cmp = have & compared[:, None] & (nv == ref["n_valid"])[:, None]
    unbounded = cmp & ~np.isfinite(tol)             # (a sample that is not finite in the oracle or under a perturbation: garbage)
    cmp &= np.isfinite(tol)
    over = cmp & ~(diff <= tol)
    tight = cmp & tr.well_conditioned(kw, S)
    with np.errstate(divide="ignore", invalid="ignore"):
        mult = np.where(cmp & (diff > floor) & (S > 0), (diff - floor) / S, 0.0)
    worst_mult = float(np.nan_to_num(mult, nan=0.0, posinf=0.0).max(initial=0.0))
    wrong_nv = compared & (nv != ref["n_valid"])
    st = STATS.setdefault(FORM_IDS[form], dict(rays=0, compared=0, samples=0, tight=0, worst_tight=0.0, worst_multiple=0.0, left_out=0,
                                               unstable=0, over=0, wrong_n_valid=0, allowance=0))
    st["rays"] += n
    st["compared"] += int(compared.sum())
    st["samples"] += int(cmp.sum())
    st["tight"] += int(tight.sum())
    st["worst_tight"] = max(st["worst_tight"], float(diff[tight].max(initial=0.0)))
    st["worst_multiple"] = max(st["worst_multiple"], worst_mult)
    st["left_out"] += int(left_out.sum())
    st["unstable"] += int((mine & ~stable).sum())
    st["allowance"] += int((asked & allowance).sum())
    st["over"] += int(over.sum())
    st["wrong_n_valid"] += int(wrong_nv.sum())
    COVERED[case[:3]] = COVERED.get(case[:3], 0) + int(cmp.sum())
    print(f"trajectory {label} {case}: compared {int(compared.sum())} rays (under the Kerr fixed-step allowance {int((asked & allowance).sum())}, "
          f"left out {int(left_out.sum())}, not stable in the oracle "
          f"{int((mine & ~stable).sum())}, flags differ {int((mine & ~same_fl).sum())}), n_valid differs on {int(wrong_nv.sum())}, samples "
          f"{int(cmp.sum())} ({int(tight.sum())} with S <= floor / COND, {int(unbounded.sum())} without a bound), worst |gpu - oracle| "
          f"{diff[cmp].max(initial=0.0):.3e} (on S <= floor / COND: {diff[tight].max(initial=0.0):.3e}), worst multiple of S {worst_mult:.1f}, "
          f"over the bound {int(over.sum())}, worst end difference {np.nan_to_num(d_end[compared], nan=0.0, posinf=0.0).max(initial=0.0):.3e}")
    # flags, object ids, starts inside
    if kerr and fixed:
        assert np.all(same_fl[asked] | (((flags | ofl)[asked] & ~np.uint8(1 | 64)) == 0))
    else:
        assert np.array_equal(flags[asked], ofl[asked])
    if spheres is not None:
        assert np.array_equal(got[4][mine & same_fl], ref["object_id"][mine & same_fl])
    inside = ofl == 3
    xs = np.broadcast_to(x0, (n, 3))
    assert np.array_equal(flags == 3, inside) and np.all(nv[inside] == 0)
    assert np.array_equal(end[inside], np.concatenate([xs[inside], k0[inside]], 1))
    # who was left out
    assert left_out.sum() <= (0.01 * n if kerr else 0), f"{int(left_out.sum())} stable rays of {n} with other flags or step counts"
    # sample counts, NaN beyond them
    assert not wrong_nv.any(), (np.nonzero(wrong_nv)[0][:8], nv[wrong_nv][:8], ref["n_valid"][wrong_nv][:8])
    assert np.all(nv <= T) and np.isnan(traj.transpose(0, 2, 1)[~have]).all()
    # the samples
    assert not over.any(), f"{int(over.sum())} of {int(cmp.sum())} samples over the bound, worst excess {np.nanmax(np.where(over, diff - tol, 0.0)):.3e}"
    # the end state
    fin = compared & np.isfinite(ref["end"]).all(1) & ~inside
    tol_end = _end_bound(ofl, kerr) + COND * (10.0 if kerr else 1.0) * np.nan_to_num(S_end, nan=np.inf, posinf=np.inf)
    assert np.all(d_end[fin] <= tol_end[fin]), f"worst end-state excess {np.max((d_end - tol_end)[fin])}"
    return dict(ref=ref, traj=traj, nv=nv, end=end, flags=flags, compared=compared, stable=stable, S=S, samples=int(cmp.sum()),
                tight=int(tight.sum()))


def _rays(form, n, seed, origins=False):
    """n rays of a form: camera rays from CAM (time-like: _orbits' starts); origins: per ray, every 7th inside the horizon."""
    rng = np.random.default_rng(seed)
    if form == 3:
        k0, x0 = _orbits(n, seed)
    else:
        k0 = tr.camera_rays(CAM, n, rng)
        x0 = CAM[None, :] + rng.normal(size=(n, 3)) * 2.0 if origins else CAM
    if origins:
        x0 = np.array(x0)
        x0[::7] = rng.normal(size=(len(x0[::7]), 3)) * 0.15
        x0[-1] = [0.1, 0.05, 0.2]                     # the last ray of the last block too
    return k0, x0


# ---- a. randomised draws ---------------------------------------------------------------------------------------------------
N_DRAWS = max(4, int(os.environ.get("BHG_FUZZ", "48")) // 4)      # 12 by default
FUZZ_TIGHT = {}     # seed: (form, samples compared with S <= floor / COND)


@pytest.mark.parametrize("seed", range(N_DRAWS))
def test_randomised_trajectories(ctx, oracle, seed):
    k0, x0, T, kw = tr.fuzz_draw(seed)
    print(f"draw {seed}: n {len(k0)}, T {T}, origins {'per ray' if np.ndim(x0) == 2 else 'shared'}, {kw}")
    r = _hold(ctx, oracle, k0, x0, T, kw, label=f"draw {seed}")
    FUZZ_TIGHT[seed] = (tr.form_of(kw), r["tight"])


def test_randomised_trajectories_are_well_conditioned():
    """Over the twelve default draws at least 100 samples per form were compared at S <= floor / COND (the oracle alone gives
    1e5, 2.6e5, 9.7e4 and 3.5e3: tests/test_trajectory_host.py).  Runs after the draws and asks nothing when they were not all run."""
    if all(seed in FUZZ_TIGHT for seed in range(12)):
        for form in range(4):
            assert sum(t for seed, (f, t) in FUZZ_TIGHT.items() if f == form and seed < 12) >= 100, FUZZ_TIGHT


# ---- b. shape and size edges, each against the oracle ----------------------------------------------------------------------
EDGE = dict(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=9.0)


@pytest.mark.parametrize("n", [2048, 2049, 2111, 2112, 2113])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_ray_counts_around_the_shape_switch(ctx, oracle, form, n):
    """2048 rays is the last wave-per-ray call, 2049 the first lane-per-ray one; 2112 = 33 blocks of 64 lanes, 2111 and 2113 end
    in a partial block.  Mixed origins, every 7th and the very last ray inside the horizon."""
    k0, x0 = _rays(form, n, 300 + n, origins=True)
    r = _hold(ctx, oracle, k0, x0, 8, dict(EDGE, **FORM_KW[form]), label=f"n={n}")
    assert (r["flags"] == 3).sum() >= n // 7 and r["flags"][-1] == 3 and (r["nv"] == 8).sum() > (0 if form == 3 else n // 10)


@pytest.mark.parametrize("T", [1023, 1024, 1025])
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_sample_counts_around_four_waves(ctx, oracle, form, n, T):
    """<= 64 rays with >= 1024 samples run four waves per ray (256 samples a pass), everything else one (64 a pass)."""
    k0, x0 = _rays(form, n, 400 + n)
    r = _hold(ctx, oracle, k0, x0, T, dict(r_s=1.0, lambda_end=60.0, **FORM_KW[form]), label=f"n={n} T={T}")
    assert (r["nv"] == T).sum() >= 10 and (form == 3 or (r["nv"] < T).sum() >= 3)


ONE_RAY_T = [2, 3, 63, 64, 65, 255, 256, 257, 10000]


@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_one_ray_at_every_pass_boundary(ctx, oracle, form):
    """The engine's literal call, one ray: T around the 64- and 256-sample passes, T = 2 (dt = lambda_end) and T = 10000; a ray
    that runs to lambda_end and one that ends early."""
    k0, x0 = _rays(form, 40, 500)
    o = oracle.trace(k0, x0, r_s=1.0, lambda_end=60.0, **FORM_KW[form])
    picks = [int(np.nonzero(o["flags"] == 4)[0][0])]
    if (o["flags"] == 1).any():
        picks.append(int(np.nonzero(o["flags"] == 1)[0][0]))
    for T in ONE_RAY_T:
        for i in picks:
            xi = x0 if np.ndim(x0) == 1 else x0[i]
            r = _hold(ctx, oracle, k0[i:i + 1], xi, T, dict(r_s=1.0, lambda_end=60.0, **FORM_KW[form]), label=f"one ray T={T}")
            assert r["compared"].all() and (r["nv"][0] == T) == (o["flags"][i] == 4)


# ---- c. samples on step ends -----------------------------------------------------------------------------------------------
GRID_SHAPES = [(24, 161), (24, 1281), (2060, 161)]      # wave, four waves, lane: dt = 0.25 = h, dt = 0.03125 = h / 8, dt = h


@pytest.mark.parametrize("n,T", GRID_SHAPES, ids=["wave", "wave4", "lane"])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_fixed_steps_sampled_on_their_ends(ctx, oracle, form, n, T):
    """RK4 with h = 0.25 to lambda_end = 40: every sample (every 8th at T = 1281) has te == t_new of a step, all exact in binary,
    so it sits on the te <= t_stop comparison -- and on the wave shape's guess floor(t_stop / dt) + 1."""
    k0, x0 = _rays(form, n, 600 + n)
    r = _hold(ctx, oracle, k0, x0, T, dict(r_s=1.0, method=1, h_fixed=0.25, lambda_end=40.0, **FORM_KW[form]), label="grid = step grid")
    assert (r["nv"] == T).sum() >= n // 4


@pytest.mark.parametrize("n,T,max_step", [(24, 161, 0.125), (24, 1281, 0.125), (2060, 161, 0.125)], ids=["wave", "wave4", "lane"])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_capped_adaptive_steps_sampled_on_their_ends(ctx, oracle, form, n, T, max_step):
    """DP5(4) with a max_step that divides dt (and lies below the initial step the controller selects out here, so that the first
    step is capped too): away from the hole every step is max_step long, t stays exact in binary, and every sample (every second
    one, every fourth at T = 1281) falls on a step end."""
    k0, x0 = _rays(form, n, 700 + n)
    r = _hold(ctx, oracle, k0, x0, T, dict(r_s=1.0, max_step=max_step, lambda_end=40.0, **FORM_KW[form]), label=f"max_step={max_step}")
    steps = int(round(40.0 / max_step))
    on_grid = (r["ref"]["flags"] == 4) & (r["ref"]["n_accepted"] == steps) & (r["ref"]["n_attempted"] == steps)
    print(f"{int(on_grid.sum())} of {n} rays take every step at the cap")
    assert on_grid.sum() >= n // 16 and np.all(r["nv"][on_grid & r["compared"]] == T)


# ---- c2. the last sample's time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,T", [(60.0, 30), (60.0, 80), (50.0, 12)])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_the_last_sample_is_taken_at_lambda_end(ctx, oracle, form, lam, T):
    """t_eval's last point is lambda_end itself, not (T - 1) dt: at these (lambda_end, T) the product rounds to the double above
    lambda_end, a time no ray reaches, and the lane shape's serial comparison would drop the last sample of every ray that runs
    to the end."""
    assert (T - 1) * (lam / (T - 1)) > lam
    k0, x0 = _rays(form, 2049, 650 + T)
    r = _hold(ctx, oracle, k0, x0, T, dict(r_s=1.0, lambda_end=lam, **FORM_KW[form]), label=f"lambda_end={lam}")
    ran = r["flags"] == 4
    assert ran.sum() > 200 and np.all(r["nv"][ran & r["compared"]] == T)


# ---- d. step budgets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [1, 13, 16])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_step_budgets(ctx, oracle, form, budget):
    """A ray stopped by max_steps emits the samples up to its last accepted step's end, and that state is its end."""
    k0, x0 = _rays(form, 300, 800)
    r = _hold(ctx, oracle, k0, x0, 257, dict(r_s=1.0, lambda_end=120.0, max_steps=budget, **FORM_KW[form]), label=f"max_steps={budget}")
    cut = r["flags"] == 16
    assert cut.sum() > (250 if budget == 1 else 30) and np.all(r["nv"][cut] < 257) and np.all(r["nv"][cut] >= 1)


# ---- e. time-like orbits with every event ----------------------------------------------------------------------------------
TL_SPHERES = [[6.0, 3.0, 2.5, 1.5], [-5.0, -4.0, 3.0, 1.2]]


@pytest.mark.parametrize("method", [0, 1], ids=["dp54", "rk4"])
@pytest.mark.parametrize("events", ["exit", "disk", "spheres", "all"])
def test_timelike_orbits(ctx, oracle, method, events):
    k0, x0 = _orbits(300, 41)
    kw = dict(r_s=1.0, lambda_end=150.0, time_like=1)
    if method:
        kw.update(method=1, h_fixed=0.25)
    if events in ("exit", "all"):
        kw["r_exit"] = 16.0
    if events in ("disk", "all"):
        kw.update(disk_r_in=3.0, disk_r_out=12.0)
    if events in ("spheres", "all"):
        kw["spheres"] = TL_SPHERES
    r = _hold(ctx, oracle, k0, x0, 130, kw, label=f"orbits {events}")
    want = {"exit": 8, "disk": 128, "spheres": 0x88}
    for name, flag in want.items():
        if events in (name, "all"):
            assert (r["flags"] == flag).sum() >= (3 if events == name else 1), (name, np.unique(r["flags"], return_counts=True))


# ---- f. Kerr with object spheres and with the disk -------------------------------------------------------------------------
KERR_CAM = np.array([4.0, -24.0, 13.0])
KERR_SPHERES = [[5.0, 0.0, 0.0, 1.5], [0.0, -6.0, 2.0, 1.2], [0.2, 0.1, 7.0, 1.0], [-4.0, 3.0, -3.0, 1.3]]


@pytest.mark.parametrize("n", [300, 2300], ids=["wave", "lane"])
@pytest.mark.parametrize("spin", [0.45, -0.3])
def test_kerr_with_object_spheres_and_the_disk(ctx, oracle, spin, n):
    rng = np.random.default_rng(61)
    k0 = (-KERR_CAM / np.linalg.norm(KERR_CAM))[None, :] + rng.normal(size=(n, 3)) * 0.2
    k0 /= np.linalg.norm(k0, axis=1)[:, None]
    base = dict(r_s=1.0, lambda_end=60.0, rhs_form=2, spin=spin)
    r = _hold(ctx, oracle, k0, KERR_CAM, 96, dict(base, spheres=KERR_SPHERES), label="kerr spheres")
    assert (r["flags"] == 0x88).sum() > 0.03 * n
    r = _hold(ctx, oracle, k0, KERR_CAM, 96, dict(base, disk_r_in=3.0, disk_r_out=10.0), label="kerr disk")
    assert (r["flags"] == 128).sum() > 0.03 * n
    r = _hold(ctx, oracle, k0, KERR_CAM, 96, dict(base, disk_r_in=3.0, disk_r_out=10.0, spheres=KERR_SPHERES, r_exit=30.0), label="kerr both")
    assert (r["flags"] == 128).sum() > 0.01 * n and (r["flags"] == 0x88).sum() > 0.03 * n and (r["flags"] == 8).sum() > 0.1 * n


# ---- g. non-finite directions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["dp54", "rk4"])
@pytest.mark.parametrize("form", range(4), ids=FORM_IDS)
def test_nonfinite_directions(ctx, oracle, form, method):
    """Three rays of a 130-ray set with NaN or inf in k0 and max_steps = 50, in the wave shape and -- the set sixteen times over, the
    three in its first copy -- the lane shape.  (Every attempt counts towards max_steps and the attempt helper returns once the
    count is reached, a fixed step that ends in NaN ends the ray: the loop is bounded.)  Such a ray carries the NaN flag or the
    oracle's flags and emits what the oracle emits; every other ray has the bits of the same call without them."""
    k0, x0 = _rays(form, 130, 900)
    kw = dict(r_s=1.0, lambda_end=60.0, max_steps=50, **FORM_KW[form])
    if method:
        kw.update(method=1, h_fixed=0.5)
    for copies in (1, 16):
        clean = np.tile(k0, (copies, 1))
        xs = x0 if np.ndim(x0) == 1 else np.tile(x0, (copies, 1))
        k = clean.copy()
        k[3] = np.nan
        k[77, 1] = np.inf
        k[129] = [-np.inf, np.nan, 1.0]
        bad = np.zeros(len(k), bool)
        bad[[3, 77, 129]] = True
        r = _hold(ctx, oracle, k, xs, 37, kw, label="non-finite k0", apart=bad)
        ofl, onv = r["ref"]["flags"], r["ref"]["n_valid"]
        assert np.all(((r["flags"][bad] & 64) != 0) | (r["flags"][bad] == ofl[bad])), (r["flags"][bad], ofl[bad])
        assert np.array_equal(r["nv"][bad], onv[bad])
        emitted = np.arange(37)[None, :] < onv[bad][:, None]
        assert np.array_equal(np.isnan(r["traj"][bad]).all(1), ~emitted)
        assert np.all((r["flags"][~bad] & 64) == 0)
        ref_call = ctx.trajectory(clean, xs, _params(**kw), 37)
        assert np.array_equal(r["traj"][~bad], ref_call[0][~bad], equal_nan=True) and np.array_equal(r["nv"][~bad], ref_call[1][~bad])
        assert np.array_equal(r["end"][~bad], ref_call[2][~bad]) and np.array_equal(r["flags"][~bad], ref_call[3][~bad])


# ---- h. what the run covered -----------------------------------------------------------------------------------------------
def test_every_shape_method_and_form_was_compared():
    """Every launch shape x method x right-hand side with a nonzero count of compared samples.  Runs last and asks nothing when the
    tests above were not all run."""
    if len(COVERED) and all(seed in FUZZ_TIGHT for seed in range(12)) and ("kerr", "rk4", "lane") in COVERED:
        for form in FORM_IDS:
            for method in ("dp54", "rk4"):
                for shape in ("wave", "wave4", "lane"):
                    assert COVERED.get((form, method, shape), 0) > 0, (form, method, shape)

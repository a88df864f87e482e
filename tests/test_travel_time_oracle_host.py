"""The C oracle's coordinate time (oracle.travel_time; DESIGN.md section 18, "Held to the oracle") held on the CPU, without a GPU:
against the scipy golden vectors in all six sets, the closed-form radial ray, flat space, a converged DOP853 solve of the
7-component system (Kerr with an exit sphere and at negative spin among the sets), and the live scipy restatement
(tests/travel_time_reference.solve) on randomised draws; then the selections and counts that tests/test_gpu_travel_time_oracle.py
relies on, from the oracle alone: who is left out and the caps on that, how many finite times the twelve draws give per form, and
that the fixed sets hold the rays they are there for.

Measured when this was written: golden, worst |oracle - golden| 2.6e-8 absolute (4.5e-10 relative, on the near-critical rays) and
9.5 S_i in the default sets, 4.2e-14 relative in the tight sets, 0.015 of the golden's tolerance at most; the radial ray 0 from
32 + ln 17; flat space 0 in all three forms; the converged solve 5.8e-11 (Schwarzschild), 1.1e-10 and 1.9e-10 (Kerr a / M = 0.9
without and with an exit sphere) and 2.1e-10 (a / M = -0.9) relative; the draws 0.005 of the tolerance at most; left out: 47 of 1059
in draw 5 (Kerr, rtol 7e-3), none elsewhere in the draws, and in the fixed sets only the one ray that lies in the disk plane."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import crossings_reference as cx  # noqa: E402
import travel_time_oracle_sets as ts  # noqa: E402
import travel_time_reference as tt  # noqa: E402

COND = tt.COND
FORM_IDS = list(ts.FORM_IDS)


# ---- the entry point beside the ones it stands next to ----------------------------------------------------------------------
def test_everything_else_is_the_crossings_mode(oracle):
    """What trace_crossings returns is returned unchanged (the affine parameters t_end / t_cross keep their meaning), and with
    the disk off and no records the plain trace's results."""
    for seed in (1, 2, 6):
        _, k0, x0, K, kw, _ = ts.draw(seed)
        a, b = oracle.trace_crossings(k0, x0, max_records=K, **kw), oracle.travel_time(k0, x0, K, **kw)
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        have = np.arange(K)[:, None] < b["n_cross"][None, :]
        assert np.array_equal(~np.isnan(b["dt_cross"]), have)
        off = {key: val for key, val in kw.items() if not key.startswith("disk")}
        c, d = oracle.trace(k0, x0, **off), oracle.travel_time(k0, x0, 0, **off)
        for key in c:
            assert np.array_equal(c[key], d[key], equal_nan=True), key
        assert d["dt_cross"].shape == (0, len(k0)) and np.all(d["n_cross"] == 0)
        assert np.array_equal(d["dt_end"], b["dt_end"], equal_nan=True)        # the end time does not depend on the disk
        z = oracle.travel_time(k0, x0, 0, **kw)                               # a disk and no records: the counts all the same
        assert np.array_equal(z["n_cross"], b["n_cross"]) and np.array_equal(z["dt_end"], b["dt_end"], equal_nan=True)
    with pytest.raises(RuntimeError):
        oracle.travel_time(k0, x0, 2, **off)                                  # records without a disk, as the library refuses
    with pytest.raises(RuntimeError):
        oracle.travel_time(k0, x0, 0, **dict(kw, method=1))


def test_special_values(oracle):
    cam = cx.inclined_camera(30.0, 60.0, 0.5)
    look = -cam / np.linalg.norm(cam)
    k0 = np.stack([look + [0.0, 0.02, 0.0], look + [0.0, 0.3, 0.1], look + [0.0, 0.02, 0.0]])
    x0 = np.stack([cam, cam, 0.3 * cam / np.linalg.norm(cam)])
    for rhs, spin in ts.FORMS:
        kw = dict(r_s=1.0, lambda_end=120.0, r_exit=35.0, rhs_form=rhs, spin=spin, disk_r_in=1.2, disk_r_out=15.0)
        o = oracle.travel_time(k0, x0, 2, **kw)
        assert o["flags"][0] == 1 and o["dt_end"][0] == np.inf
        assert o["flags"][1] == 8 and 30.0 < o["dt_end"][1] < 80.0
        assert o["flags"][2] == 3 and o["dt_end"][2] == np.inf and o["n_cross"][2] == 0 and np.isnan(o["dt_cross"][:, 2]).all()
        # (a NaN direction never fails scipy's step-size test: it takes a step budget to end the ray)
        bad = oracle.travel_time([[np.nan, 0.0, 1.0]], cam, 2, **dict(kw, max_steps=40))
        assert bad["flags"][0] == 16 | 64 and np.isnan(bad["dt_end"][0]) and bad["n_cross"][0] == 0
        # a spent budget: the sum so far -- the ray's own time at the state it returns, step by step up to the full time
        full, prev, acc = o["dt_end"][1], 0.0, 0
        for budget in range(1, int(o["n_attempted"][1]) + 2):
            s = oracle.travel_time(k0[1:2], cam, 2, **dict(kw, max_steps=budget))
            done = s["flags"][0] != 16
            assert s["dt_end"][0] == full if done else prev <= s["dt_end"][0] < full
            assert s["dt_end"][0] > prev or s["n_accepted"][0] == acc                      # (a rejected attempt adds nothing)
            prev, acc = s["dt_end"][0], s["n_accepted"][0]
        assert done


@pytest.mark.parametrize("rhs", [0, 1], ids=FORM_IDS[:2])
def test_radial_ray_closed_form(oracle, rhs):
    exact = 32.0 + np.log(17.0)
    kw = dict(r_s=1.0, r_exit=35.0, lambda_end=120.0, max_step=0.5, rhs_form=rhs)
    o = oracle.travel_time([[0.0, 0.0, 1.0]], [0.0, 0.0, 3.0], 0, **kw)
    rel = abs(o["dt_end"][0] / exact - 1.0)
    print(f"radial ray, form {rhs}: {o['n_accepted'][0]} steps, relative distance from 32 + ln 17 {rel:.1e}")
    assert o["flags"][0] == 8 and rel <= 1e-12
    o2 = oracle.travel_time([[0.0, 0.0, 2.5]], [0.0, 0.0, 3.0], 0, **dict(kw, max_step=0.2))      # the length of k0 does not matter
    assert abs(o2["dt_end"][0] / exact - 1.0) <= 1e-12
    # a spent budget on the same ray: the closed form from the start to wherever the ray got
    worst = 0.0
    for budget in (1, 7, 30):
        s = oracle.travel_time([[0.0, 0.0, 1.0]], [0.0, 0.0, 3.0], 0, **dict(kw, max_steps=budget))
        assert s["flags"][0] == 16 and s["n_accepted"][0] == budget
        worst = max(worst, abs(s["dt_end"][0] / tt.radial_time(3.0, s["end"][0, 2]) - 1.0))
    print(f"  ... cut off after 1, 7, 30 steps: {worst:.1e} from the closed form up to the state returned")
    assert worst <= 1e-12


@pytest.mark.parametrize("rhs", [0, 1, 2], ids=FORM_IDS)
def test_flat_space(oracle, rhs):
    k0, lam = np.array([[0.3, 0.2, 2.0]]), 7.0
    o = oracle.travel_time(k0, [1.0, 2.0, 3.0], 0, r_s=0.0, lambda_end=lam, rhs_form=rhs)
    rel = abs(o["dt_end"][0] / (np.linalg.norm(k0) * lam) - 1.0)
    print(f"flat space, form {rhs}: {rel:.1e}")
    assert o["flags"][0] == 4 and rel <= 1e-14


# ---- the golden vectors ------------------------------------------------------------------------------------------------------
SETS = ("schw_default", "kerr_default", "schw_nodisk", "kerr_nodisk", "schw_tight", "kerr_tight")


@pytest.mark.parametrize("name", SETS)
def test_golden_times(oracle, name):
    g = load_golden("travel_time")
    get = lambda k: g[f"{name}__{k}"]      # noqa: E731
    disk = tuple(get("disk"))
    K = 4 if disk[1] > 0.0 else 0
    for fi, form in enumerate(get("forms")):
        o = oracle.travel_time(get("k0"), get("x0"), K, r_s=float(get("r_s")), lambda_end=float(get("lambda_end")), rtol=float(get("rtol")),
                               atol=float(get("atol")), r_exit=float(get("r_exit")[fi]), rhs_form=int(form), spin=float(get("spin")),
                               disk_r_in=disk[0], disk_r_out=disk[1])
        assert np.array_equal(o["flags"], get("flags")[fi]) and np.array_equal(o["n_cross"], get("n_cross")[fi])
        assert np.array_equal(o["n_attempted"], get("n_attempted")[fi]) and np.array_equal(o["n_accepted"], get("n_accepted")[fi])
        ref = np.concatenate([get("t_end")[fi][None, :], get("t_cross")[fi][:K]])
        S = np.concatenate([get("S_end")[fi][None, :], get("S_cross")[fi][:K]])
        got = ts.times_of(o)
        assert np.array_equal(ts.pattern(got), ts.pattern(ref))               # every time the golden has, inf where it has inf
        fin = np.isfinite(ref)
        err, tol = np.abs(got[fin] - ref[fin]), np.maximum(COND * S[fin], float(get("floor")[fi]))
        with np.errstate(divide="ignore", invalid="ignore"):
            mult = np.where(S[fin] > 0.0, err / S[fin], 0.0)
        print(f"{name} form {int(form)}: {int(fin.sum())} finite times, worst |oracle - golden| {err.max():.3e} absolute, "
              f"{(err / ref[fin]).max():.3e} relative, {mult.max():.1f} S_i; worst err / tol {(err / tol).max():.3f}")
        assert np.all(err <= tol), (err / tol).max()


# ---- the converged solve -----------------------------------------------------------------------------------------------------
# test_travel_time_host.py's selections (rays away from the critical impact parameter), plus Kerr with an exit sphere -- the DOP853
# solve carries it as an event on Boyer-Lindquist r -- and a negative spin
CONVERGED = [(0, 0.0, 120.0, 35.0), (1, 0.0, 120.0, 35.0), (2, 0.45, 60.0, 0.0), (2, 0.45, 120.0, 35.0), (2, -0.45, 120.0, 35.0)]


@pytest.mark.parametrize("form,spin,lam,r_exit", CONVERGED, ids=["christoffel", "reduced", "kerr", "kerr-exit", "kerr-exit-retrograde"])
def test_against_the_seven_component_system(oracle, form, spin, lam, r_exit):
    cam = cx.inclined_camera(30.0, 70.0, 0.5 if form == 2 else 0.0)
    k = cx.camera_rays(cam, 40, np.random.default_rng(1), critical=0.0)
    o = oracle.travel_time(k, cam, 0, rhs_form=form, spin=spin, r_exit=r_exit, rtol=1e-10, atol=1e-12, lambda_end=lam)
    worst, count, exited = 0.0, 0, 0
    for i, ki in enumerate(k):
        if o["flags"][i] & 1:
            assert o["dt_end"][i] == np.inf
            continue
        fl, tc = tt.solve_converged(ki, cam, form, spin=spin, r_exit=r_exit, lambda_end=lam)
        assert fl == o["flags"][i] and np.isfinite(tc) and np.isfinite(o["dt_end"][i])
        worst, count, exited = max(worst, abs(o["dt_end"][i] / tc - 1.0)), count + 1, exited + int(fl == 8)
    print(f"form {form} spin {spin} r_exit {r_exit}: {count} rays ({exited} through the sphere), worst relative distance {worst:.1e}")
    assert count >= 20 and worst <= 1e-9 and (r_exit == 0.0 or exited >= 20)


# ---- live scipy on randomised draws ------------------------------------------------------------------------------------------
SCIPY_DRAWS = (0, 3, 1, 4, 2, 5)        # two per form; per-ray origins, r_s 0.6 ... 2, max_step, exit spheres and either spin among them


@pytest.mark.parametrize("seed", SCIPY_DRAWS)
def test_draws_against_scipy(oracle, seed):
    label, k0, x0, K, kw, _ = ts.draw(seed)
    assert "max_steps" not in kw                                               # (solve_ivp has no step budget)
    k0 = k0[:150]
    x0 = x0 if np.ndim(x0) == 1 else x0[:150]
    r = ts.reference(oracle, k0, x0, K, **kw)
    o, par = r["o"], {key: val for key, val in kw.items() if key not in ("rhs_form", "disk_r_in", "disk_r_out")}
    worst, compared = 0.0, 0
    for i in np.flatnonzero(r["stable"]):
        s = tt.solve(k0[i], x0 if np.ndim(x0) == 1 else x0[i], kw["rhs_form"], (kw["disk_r_in"], kw["disk_r_out"]), K=K, **par)
        assert (s["flags"], s["n_attempted"], s["n_accepted"], s["n_cross"]) == (o["flags"][i], o["n_attempted"][i], o["n_accepted"][i], o["n_cross"][i]), i
        m = min(K, s["n_cross"])
        want = np.full(1 + K, np.nan)
        want[0], want[1:1 + m] = s["t_end"], s["t_cross"][:m]
        assert np.array_equal(ts.pattern(want), ts.pattern(r["t"][:, i])), i
        fin = np.isfinite(want)
        ratio = np.abs(want[fin] - r["t"][fin, i]) / r["tol"][fin, i] if r["floor"] > 0.0 else np.abs(want[fin] - r["t"][fin, i])
        worst, compared = max(worst, ratio.max(initial=0.0)), compared + int(fin.sum())
    print(f"{label} ({FORM_IDS[kw['rhs_form']]}): {int(r['stable'].sum())} of {len(k0)} rays, {compared} finite times, worst err / tol {worst:.3f}")
    assert r["floor"] > 0.0 and compared >= 20 and worst <= 1.0


# ---- who is compared on the GPU: the counts and the caps ---------------------------------------------------------------------
FUZZ_FINITE = (2712, 3217, 1978)        # finite times on the stable rays of draws 0 ... 11, per form


def test_the_twelve_draws(oracle):
    rays, left, finite = 0, 0, [0, 0, 0]
    for seed in range(ts.N_DRAWS):
        label, k0, x0, K, kw, _ = ts.draw(seed)
        r = ts.reference(oracle, k0, x0, K, **kw)
        out = int((~r["stable"]).sum())
        print(f"{label} ({FORM_IDS[kw['rhs_form']]}): {len(k0)} rays, {out} left out, {int(r['fin'].sum())} finite times, floor {r['floor']:.2e}")
        assert out <= ts.LEFT_OUT_SET * len(k0) and r["floor"] > 0.0, label
        rays, left = rays + len(k0), left + out
        finite[kw["rhs_form"]] += int(r["fin"].sum())
    print(f"draws 0 ... 11: {left} of {rays} rays left out; finite times per form {finite}")
    assert left <= ts.LEFT_OUT_DRAWS * rays
    assert tuple(finite) == FUZZ_FINITE


def test_the_fixed_sets(oracle):
    """Each fixed set leaves out at most a tenth of its rays, and holds what it is there for."""
    for case in ts.fixed_sets():
        label, k0, x0, K, kw, _ = case[:6]
        r = ts.case_reference(oracle, case)
        out = int((~r["stable"]).sum())
        print(f"{label} ({FORM_IDS[kw['rhs_form']]}): {len(k0)} rays, {out} left out, {int(r['fin'].sum())} finite times, floor {r['floor']:.2e}")
        assert out <= ts.LEFT_OUT_SET * len(k0), label
        assert r["fin"].sum() >= 4 and r["floor"] > 0.0, label                    # (a floor of 0 would ask for the oracle's bits)


@pytest.mark.parametrize("rhs", [0, 1], ids=FORM_IDS[:2])
def test_rays_that_step_across_the_hole(oracle, rhs):
    for rtol, dist in ts.ACROSS_SETTINGS:
        label, k0, x0, K, kw, _ = ts.across_the_hole(rhs, rtol, dist)
        r = ts.reference(oracle, k0, x0, K, **kw)
        hor = (r["o"]["flags"] & 1) != 0
        by_node = ~hor & np.isposinf(r["t"][0])
        print(f"{label}: {int((~hor).sum())} rays do not end on the horizon, {int(by_node.sum())} of them +inf by a node, "
              f"{int((~hor & np.isfinite(r['t'][0])).sum())} finite, {int(np.isposinf(r['t'][1:]).sum())} infinite crossing times, "
              f"{int((~r['stable']).sum())} left out")
        assert by_node.sum() >= 100 and r["stable"].all()
        if (rtol, dist) == (1e-2, 60.0):
            assert np.isposinf(r["t"][1:]).sum() >= 20
    # (Kerr gives no such ray: the Boyer-Lindquist radius cannot step through the hole)


@pytest.mark.parametrize("spin", ts.KERR_EXIT_SPINS)
def test_kerr_exit_sets(oracle, spin):
    label, k0, x0, K, kw, _ = ts.kerr_exit(spin)
    r = ts.reference(oracle, k0, x0, K, **kw)
    assert ((r["o"]["flags"] == 8) & r["fin"][0]).sum() >= 100 and r["stable"].all()


def test_more_crossings_than_records_and_plane_starts(oracle):
    label, k0, x0, K, kw, _ = ts.many_crossings(0, 1e-9, 2)[:6]
    r = ts.reference(oracle, k0, x0, K, **kw)
    assert np.median(r["o"]["n_cross"]) == cx.MANY_COUNTS[1e-9][0] > K
    for form in range(3):
        (label, k0, x0, K, kw, _), events = ts.plane_starts(form, ts.PLANE_DISKS[0])
        r = ts.reference(oracle, k0, x0, K, **kw)
        assert all(e is None or e == c for e, c in zip(events, r["o"]["n_cross"]))
        at_start = r["o"]["t_cross"][0] < 1e-14                                # (Boyer-Lindquist: cos(pi / 2) is 6e-17, not 0)
        assert at_start.sum() >= (1 if form == 2 else 8)
        assert np.all(r["t"][1][at_start] >= 0.0) and np.all(r["t"][1][at_start] <= (1e-13 if form == 2 else 0.0))

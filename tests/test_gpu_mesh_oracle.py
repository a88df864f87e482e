"""bhg_trace_mesh_device against the C oracle's brute-force restatement of the hit rule (oracle.trace_mesh: DESIGN.md section 19 on
the oracle's own DP5(4) loop, every sub-chord against every triangle -- no tree, no box, no cull; held on the CPU to the scipy
golden, to live scipy and to the straight line of flat space by tests/test_mesh_oracle_host.py, which also asserts the conditions
of the cases used here).  Every ray of every case is compared (_hold):

  * rays the oracle calls stable (flag, triangle, step counts and M unchanged under the three 1-2 ulp perturbations of k0): flags,
    n_steps, n_accepted and tri identical -- Kerr: the step-count allowances tests/test_gpu_parity.py grants the plain Kerr trace
    against this oracle (at scale: flags and triangles identical, at most 4 rays with other step counts, by at most 2; randomised
    draws: the horizon-ray and near-axis classes of test_randomised_kerr for the step counts, the triangle identical wherever the
    flag is); Schwarzschild, randomised draws included: no allowance;
  * unstable rays: the device's (flag, tri, counts) is one the oracle gives when k0 is scaled by 1 +- 1 ... 4e-16;
  * hits: end within STATED_DISK + COND * sens + 1e-11 * graze of the oracle's, bary within that over the triangle's shortest
    edge (test_golden_parity's bound); other rays: end within _compare's bound for their class;
  * no triangle: tri == -1 and bary left at the sentinel.

Measured when this was written (MI355X, 34 tests, 17 994 rays, 4 822 hits compared; no case or draw has an unstable ray, no stable
ray differs in flag, triangle or step counts, Kerr included):
  form          rays   hits   worst |end - oracle|   worst |bary - oracle|   largest multiple of a hit's own sensitivity
  christoffel   7631   2426   3.7e-10 (loose)        5.4e-10                 0.17
  reduced       5055   1452   1.7e-10 (draw 3)       3.7e-10                 5.6
  kerr          5308    944   2.4e-9 (frame, a < 0)  3.7e-10                 0.37
(each within STATED_DISK + COND * sens + 1e-11 * graze; the smallest margin left is 1.1e-10, Kerr 1.0e-9).  Rays that end
elsewhere, horizon rays apart: within 5.7e-8 (Schwarzschild) and 2.6e-3 (Kerr: a randomised draw's rays, 1e4 times their own
sensitivity allowed).  Wall time per test: frames 0.11 - 0.15 s, parameter cases <= 0.09 s, draws <= 0.53 s; the module 3.8 s.

Mutation checks, each done once on a copy of the library: `id < best_tri` -> `id > best_tri` fails every_triangle_twice,
flat_plate_twice and all eight draws; `root <= t_stop` -> `root < t_stop - 1e-3` fails just_above_the_disk and draw 3; M clamped to 512 fails
grazes_at_the_cap; mesh_step_candidate without `dev` fails bulge_into_the_box.  Dropping the 1e-10 slack of segment_meets_box
fails nothing here, flat_plate_twice (flat, axis-aligned, duplicated triangles at coordinates far smaller than the sub-chords, met
steeply and at grazing angles) included: a box is widened by 16 ulps of its largest coordinate, its entry and exit on one axis come from the same
rounded operations and stay ordered, and the slack only decides when a box entry equals the best s or another axis's exit to
rounding -- two triangles met at the same s to an ulp, which is what makes a ray unstable in the oracle."""
import time

import numpy as np
import pytest

import mesh_cases as mc
import mesh_oracle_cases as mo
from test_gpu_parity import COND as COND_END
from test_gpu_parity import KERR_FUZZ_DIFFER, KERR_FUZZ_DIFFER_HORIZON, KERR_FUZZ_DIFFER_OTHER, TOL_END

pytestmark = pytest.mark.gpu

FORM_IDS = ["christoffel", "reduced", "kerr"]
SENTINEL = mc.SENTINEL
KEYS = ("end", "flags", "n_steps", "n_accepted", "tri", "bary")
STATS = {}       # per form: hits compared, worst |end - oracle|, worst |bary - oracle|, worst multiple of a ray's sensitivity
UNSTABLE = {}    # per case: rays the oracle calls unstable
WALL = {}        # per test: seconds


@pytest.fixture(scope="module", autouse=True)
def _totals():
    yield
    print("\nmesh against the oracle, per form:")
    for form, st in STATS.items():
        print(f"  {form}: {st}")
    print(f"  unstable rays per case: {UNSTABLE}")
    print("  wall time per test: " + ", ".join(f"{k} {v:.2f}s" for k, v in WALL.items()))


@pytest.fixture(autouse=True)
def _wall(request):
    t = time.perf_counter()
    yield
    WALL[request.node.name] = time.perf_counter() - t


def _device(ctx, case, leaf=4):
    from blackhole_geodesic_calculator_amd import _ffi
    mesh = _ffi.Mesh(ctx, case["V"], case["F"], leaf_size=leaf)
    try:
        return mc.trace_mesh_device(ctx, _ffi.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"]), mesh, case["chord"],
                                    case["k0"], case["x0"])
    finally:
        mesh.close()


def _lz(x0, k0, r_s, spin):
    from oracle import scipy_reference as sr
    return np.array([sr.kerr_constants(*sr.cart_to_bl(x, k, spin), 0.5 * r_s, spin)[1] for x, k in zip(x0, k0)])


def _hold(ctx, oracle, case, label, o=None, r=None):
    """Device against oracle on every ray of a case; returns (oracle result, device result)."""
    o = mo.oracle_solve(oracle, case) if o is None else o
    r = _device(ctx, case) if r is None else r
    n = len(case["k0"])
    kerr = case["rhs"] == 2
    par = case["par"]
    stable = o["stable"]
    UNSTABLE[label] = int((~stable).sum())
    assert (~stable).sum() <= mo.UNSTABLE_CAP * n            # (tests/test_mesh_oracle_host.py asserts it on the CPU)
    # what the device leaves alone
    on_mesh = r["tri"] >= 0
    assert np.array_equal(on_mesh, r["flags"] == 0x88) and np.all(r["tri"][~on_mesh] == -1) and np.all(r["tri"] < len(case["F"]))
    assert np.all(r["bary"][~on_mesh] == SENTINEL) and not np.any(r["bary"][on_mesh] == SENTINEL)
    steps_same = (r["n_steps"] == o["n_attempted"]) & (r["n_accepted"] == o["n_accepted"])
    agree = steps_same & (r["flags"] == o["flags"]) & (r["tri"] == o["tri"])
    bad = stable & ~agree
    mode = case["mode"]
    dstep = np.abs(r["n_steps"].astype(int) - o["n_attempted"].astype(int))
    if mode == "exact" or (mode == "fuzz" and not kerr):
        assert not bad.any(), (np.flatnonzero(bad)[:8], r["flags"][bad][:8], o["flags"][bad][:8], r["tri"][bad][:8], o["tri"][bad][:8],
                               r["n_steps"][bad][:8], o["n_attempted"][bad][:8])
    elif mode == "kerr":                        # _compare's step_flips = 4 (test_kerr_seeded_rays_and_rk4)
        assert np.array_equal(r["flags"][stable], o["flags"][stable]) and np.array_equal(r["tri"][stable], o["tri"][stable])
        assert bad.sum() <= 4, int(bad.sum())
        assert dstep[bad].max(initial=0) <= 2
    else:                                       # a Kerr draw: test_randomised_kerr's classes, and the triangle wherever the flag agrees
        assert (r["flags"] != o["flags"])[stable].mean() <= 0.002
        same_flag = stable & (r["flags"] == o["flags"])
        assert np.array_equal(r["tri"][same_flag], o["tri"][same_flag])
        hor_all = (((r["flags"] | o["flags"]) & (1 | 64)) != 0) & stable
        hor = hor_all[bad]
        xs = np.broadcast_to(case["x0"], (n, 3))
        touchy = hor | (np.abs(_lz(xs[bad], case["k0"][bad], par["r_s"], case["spin"])) < 0.3 * par["r_s"])
        rec = dict(rays=n, differ=int(bad.sum()), differ_horizon=int(hor.sum()), horizon_rays=int(hor_all.sum()), differ_neither=int((~touchy).sum()))
        assert hor.sum() <= max(3, KERR_FUZZ_DIFFER_HORIZON * hor_all.sum()), rec
        assert (~hor).sum() <= max(3, KERR_FUZZ_DIFFER_OTHER * n), rec
        assert bad.sum() <= max(3, KERR_FUZZ_DIFFER * n, KERR_FUZZ_DIFFER_HORIZON * hor_all.sum()), rec
        assert (~touchy).sum() <= 1, rec
    # unstable rays: one of the oracle's own answers next to k0
    for i in np.flatnonzero(~stable & ~agree):
        got = (int(r["flags"][i]), int(r["tri"][i]), int(r["n_steps"][i]), int(r["n_accepted"][i]))
        seen = mo.oracle_nearby(oracle, case, i)
        assert got in seen, f"unstable ray {i}: GPU {got}, oracle near by {seen}"
    # the hits: test_golden_parity's bound
    ok = stable & agree
    hit = ok & (o["tri"] >= 0)
    st = STATS.setdefault(FORM_IDS[case["rhs"]], dict(rays=0, hits=0, worst_end=0.0, worst_bary=0.0, worst_multiple=0.0, worst_other=0.0))
    st["rays"] += n
    if hit.any():
        tol, shortest = mo.hit_tolerances(case["V"], case["F"], o["end"][hit], o["tri"][hit], o["sens"][hit], kerr)
        diff = np.abs(r["end"][hit] - o["end"][hit]).max(1)
        dbary = np.abs(r["bary"][hit] - o["bary"][hit]).max(1)
        bound = mo.STATED_DISK[kerr]
        with np.errstate(divide="ignore", invalid="ignore"):
            mult = np.where((diff > bound) & (o["sens"][hit] > 0), (diff - bound) / o["sens"][hit], 0.0)
        st["hits"] += int(hit.sum())
        st["worst_end"] = max(st["worst_end"], float(diff.max()))
        st["worst_bary"] = max(st["worst_bary"], float(dbary.max()))
        st["worst_multiple"] = max(st["worst_multiple"], float(np.nan_to_num(mult, posinf=0.0).max()))
        print(f"{label}: {n} rays, {int(hit.sum())} hits compared, unstable {int((~stable).sum())}, stable rays with other counts {int(bad.sum())}, "
              f"worst |end - oracle| {diff.max():.3e} (excess {np.max(diff - tol):.3e}), worst |bary - oracle| {dbary.max():.3e}")
        assert np.all(diff <= tol), (diff - tol).max()
        assert np.all(dbary <= tol / shortest), (dbary - tol / shortest).max()
    # every other ray: _compare's bound for its class (test_randomised_kerr's for the Kerr draws)
    miss = ok & (o["tri"] < 0) & np.isfinite(o["end"]).all(1)
    if miss.any():
        sens = np.nan_to_num(o["sens"][miss], nan=np.inf, posinf=np.inf)
        fl = o["flags"][miss]
        if mode == "fuzz" and kerr:
            tol = 1e-9 + 1e4 * sens + np.where((fl & 1) != 0, 1e-5, 0.0)
            outliers = 0.01
        else:
            tol = TOL_END + COND_END * (10.0 if kerr else 1.0) * sens + np.where((fl & 1) != 0, 1e-6, 0.0)
            kd = o["end"][miss, 3:6]
            with np.errstate(invalid="ignore", divide="ignore"):
                steep = np.abs(kd[:, 2]) / np.linalg.norm(kd, axis=1)
            tol = tol + np.where(fl == 128, 1e-11 / np.maximum(np.nan_to_num(steep), 1e-12), 0.0)
            outliers = 2e-3 if mode == "fuzz" else 0.0
        d = np.abs(r["end"][miss] - o["end"][miss]).max(1)
        st["worst_other"] = max(st["worst_other"], float(d[(fl & 1) == 0].max(initial=0.0)))
        assert (d > tol).mean() <= outliers and np.all(d <= 1e3 * tol), f"worst excess {np.max(d - tol)}, {int((d > tol).sum())} rays over"
    return o, r


def _classes_occur(case, r):
    cl = mo.classes(r)
    for key in ("hit", "disk", "horizon", "exit", "end"):
        if key in case["want"]:
            assert cl[key].sum() >= case["want"][key], (key, int(cl[key].sum()))


# ---- 1. frames -------------------------------------------------------------------------------------------------------------
FRAMES = mo.frame_cases()


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame(ctx, oracle, name):
    """2 048 rays on the 512-triangle sphere cut by the disk, the slivers and the large triangle across the exit sphere: the tree
    with leaves of 1 and of 4 triangles gives the same bits, and those are the oracle's."""
    case = FRAMES[name]
    one, four = _device(ctx, case, leaf=1), _device(ctx, case, leaf=4)
    for k in KEYS:
        assert np.array_equal(one[k], four[k]), k
    _hold(ctx, oracle, case, name, r=four)
    _classes_occur(case, four)
    x = four["end"][four["tri"] >= 0, :3]
    assert np.all(np.linalg.norm(x, axis=1) <= case["par"]["r_exit"] + 1e-9)        # no hit beyond the exit sphere


# ---- 2. the parameter list ---------------------------------------------------------------------------------------------------
PARAMETERS = mo.parameter_cases()


@pytest.mark.parametrize("name", list(PARAMETERS))
def test_parameters(ctx, oracle, name):
    case = PARAMETERS[name]
    o, r = _hold(ctx, oracle, case, name)
    _classes_occur(case, r)
    hit = r["tri"] >= 0
    if name == "m_is_1":
        assert np.all(o["M"][o["tri"] >= 0] == 1)
    if name == "m_at_cap":
        assert (o["M"] == 1024).sum() >= case["want"]["cap"] and (hit & (o["M"] == 1024)).sum() >= case["want"]["cap"]
    if name.startswith("budget_"):
        b = case["par"]["max_steps"]
        assert (hit & (r["n_steps"] == b)).sum() >= case["want"]["hit_at_budget"] and np.all(r["n_steps"][r["flags"] == 16] == b)
        assert (r["flags"] == 16).sum() >= case["want"]["cut_before_hit"]
    if name == "camera_inside":
        assert hit.all()
    if name in ("every_triangle_twice", "flat_plate_twice"):
        # the smaller index of each pair, with leaves of one triangle as with leaves of four
        assert np.all(r["tri"][hit] < len(case["F"]) // 2) and np.all(o["tri"][o["tri"] >= 0] < len(case["F"]) // 2)
        one = _device(ctx, case, leaf=1)
        assert all(np.array_equal(one[k], r[k]) for k in KEYS)


# ---- 3. the fuzz -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(mo.N_FUZZ))
def test_randomised_meshes(ctx, oracle, seed):
    """mesh_oracle_cases.fuzz_draw: a triangle soup with zero-area and repeated triangles and a closed shape, everything else drawn
    as test_randomised_configurations draws it.  A draw whose oracle run alone calls more than 1 % of its rays unstable is drawn
    again with seed + 1000 k (mesh_oracle_cases.fuzz_case; the host test asserts that at most one draw in four needs it)."""
    case, o, k = mo.fuzz_case(oracle, seed)
    print(f"draw {seed} (redraws {k}): form {case['rhs']}, {len(case['k0'])} rays, {len(case['F'])} triangles, chord {case['chord']}, {case['par']}")
    _, r = _hold(ctx, oracle, case, f"draw_{seed}", o=o)
    assert (r["tri"] >= 0).sum() >= 20

"""The C oracle's mesh rule (oracle.trace_mesh, bhgo_trace_mesh: DESIGN.md section 19 restated on the oracle's own step loop, brute
force over all triangles) pinned on the CPU, so that tests/test_gpu_mesh_oracle.py can hold the device to it:

  * against the scipy golden vectors tests/golden/mesh.npz, by the criteria tests/test_gpu_mesh.py::test_golden_parity applies to
    the device;
  * against tests/mesh_reference.solve run live, on a few dozen rays at parameter points the golden does not have;
  * in flat space (r_s = 0) against the straight line's first triangle and point, computed in numpy over all triangles;
  * the conditions of the GPU module's cases (tests/mesh_oracle_cases.py): at most 1 % of a case's rays unstable in the oracle,
    and at least the stated number of rays per class; the fuzz draws, and how many had to be drawn again.

Measured when this was written: golden -- flags, n_accepted, tri identical on all 4 x 480 rays, worst |end - scipy| 2.6e-11
(Schwarzschild) and 1.4e-10 (Kerr); live scipy -- 40 rays, 21 hits, worst |end - scipy| 3.6e-15.  No case has an unstable ray; no
fuzz draw of the default eight is redrawn.  The oracle's new code was also run under AddressSanitizer and UBSan from a stand-alone
C program (all three forms, shared and per-ray origins, the refusals): clean."""
import numpy as np
import pytest

import mesh_oracle_cases as mo
import mesh_reference as mr
from conftest import load_golden

CASES = {**mo.frame_cases(), **mo.parameter_cases()}


def _hold_to_scipy(r, ref, V, F, kerr, label, min_hits):
    """The oracle's result r against a scipy reference (arrays of mesh_reference.solve_set), test_golden_parity's criteria."""
    stable = ref["stable"]
    assert np.array_equal(r["flags"], ref["flags"]), np.flatnonzero(r["flags"] != ref["flags"])
    assert np.array_equal(r["n_accepted"][stable], ref["n_accepted"][stable])
    assert np.array_equal(r["tri"][stable], ref["tri"][stable])
    hit = stable & (ref["tri"] >= 0)
    miss = ref["tri"] < 0
    cmp = miss & stable & (ref["n_attempted"] >= 0)
    assert np.array_equal(r["n_attempted"][cmp], ref["n_attempted"][cmp].astype(np.uint32))
    assert np.all(np.isnan(r["bary"][r["tri"] < 0])) and np.all(r["M"][r["tri"] < 0] == 0) and np.all(r["tri"][miss & stable] == -1)
    assert hit.sum() >= min_hits, int(hit.sum())
    tol, shortest = mo.hit_tolerances(V, F, ref["end"][hit], ref["tri"][hit], ref["sens"][hit], kerr)
    diff = np.abs(r["end"][hit] - ref["end"][hit]).max(1)
    dbary = np.abs(r["bary"][hit] - ref["bary"][hit]).max(1)
    print(f"{label}: {int(hit.sum())} stable hits, {int((~stable).sum())} unstable, worst |end - scipy| {diff.max():.3e} (excess over its "
          f"tolerance {np.max(diff - tol):.3e}), worst |bary - scipy| {dbary.max():.3e}")
    assert np.all(diff <= tol), (diff - tol).max()
    assert np.all(dbary <= tol / shortest), (dbary - tol / shortest).max()
    return int((~stable).sum())


def test_the_restated_constants_are_the_golden_comparisons():
    import test_gpu_mesh as tg          # (constants only: nothing of that module runs here)
    assert mo.STATED_DISK == tg.STATED_DISK and mo.COND == tg.COND


# ---- 1. the scipy golden ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi", range(len(mr.GOLDEN_FORMS)), ids=mr.GOLDEN_FORM_IDS)
def test_oracle_against_the_scipy_golden(oracle, fi):
    g = load_golden("mesh")
    rhs, a = mr.GOLDEN_FORMS[fi]
    unstable = rays = 0
    for name, (V, F) in mr.golden_meshes().items():
        r = oracle.trace_mesh(g[f"{name}_k0"], g["x0"], V, F, float(g["max_chord"]), rhs_form=rhs, spin=a,
                              r_exit=0.0 if rhs == 2 else float(g["r_exit"]), **mr.GOLDEN_PAR)
        ref = {k: g[f"{name}_{k}"][fi] for k in ("end", "flags", "n_attempted", "n_accepted", "tri", "bary", "sens", "stable")}
        unstable += _hold_to_scipy(r, ref, V, F, rhs == 2, f"{mr.GOLDEN_FORM_IDS[fi]} {name}", 10)
        rays += len(ref["stable"])
    assert unstable <= 0.01 * rays


# ---- 2. scipy, live, where the golden has no point ---------------------------------------------------------------------------
LIVE_CAM = np.array([16.0, -3.0, 5.0])
LIVE_MESH = mr.join(mr.octa_sphere((-2.5, 2.0, 0.2), 1.3, 1), mr.tetrahedron((6.0, -1.0, 2.0), 0.9))
LIVE = {      # name: (rhs, spin, keywords of mesh_reference.solve, chord, per-ray origins)
    "disk_through_the_mesh": (0, 0.0, dict(lambda_end=60.0, r_exit=30.0, disk=(2.0, 6.0)), 0.25, False),
    "max_step": (1, 0.0, dict(lambda_end=60.0, r_exit=30.0, max_step=0.8), 0.25, False),
    "rtol_1e-6": (0, 0.0, dict(lambda_end=60.0, rtol=1e-6, atol=1e-9), 0.1, False),
    "kerr_negative_spin": (2, -0.4, dict(lambda_end=60.0, disk=(2.0, 6.0)), 0.25, False),
    "per_ray_origin": (1, 0.0, dict(lambda_end=60.0, r_exit=30.0), 0.25, True),
}


@pytest.mark.parametrize("name", list(LIVE))
def test_oracle_against_live_scipy(oracle, name):
    rhs, spin, kw, chord, each = LIVE[name]
    V, F = LIVE_MESH
    rng = np.random.default_rng(sorted(LIVE).index(name) + 90)
    n = 8
    k0 = np.concatenate([mr.camera_rays(LIVE_CAM, (-2.5, 2.0, 0.2), 3, rng, 1.0), mr.camera_rays(LIVE_CAM, (6.0, -1.0, 2.0), 2, rng, 0.6),
                         mr.hole_rays(LIVE_CAM, n - 5, rng, 1.5, 5.0)])
    x0 = LIVE_CAM[None, :] + (rng.normal(size=(n, 3)) * 0.3 if each else np.zeros((n, 3)))
    parts = [mr.solve_set(k0[i], x0[i], rhs, V, F, chord, spin=spin, **kw) for i in range(n)]
    ref = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    par = {k: v for k, v in kw.items() if k != "disk"}
    if "disk" in kw:
        par.update(disk_r_in=kw["disk"][0], disk_r_out=kw["disk"][1])
    r = oracle.trace_mesh(k0, x0 if each else LIVE_CAM, V, F, chord, rhs_form=rhs, spin=spin, r_s=1.0, **par)
    assert np.array_equal(r["M"][ref["stable"]], ref["M"][ref["stable"]])
    _hold_to_scipy(r, ref, V, F, rhs == 2, name, 3)
    if "disk" in kw:
        assert (ref["flags"] == 128).sum() >= 1


# ---- 3. flat space: the straight line ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs", [0, 1], ids=["christoffel", "reduced"])
def test_flat_space_is_the_straight_line(oracle, rhs):
    rng = np.random.default_rng(61)
    V, F = mr.random_triangles(200, rng, spread=5.0, size=1.0)
    cam = np.array([14.0, -3.0, 4.0])
    n = 600
    k0 = rng.normal(size=(n, 3)) * 4.0 - cam
    k0 /= np.linalg.norm(k0, axis=1)[:, None]
    lam = 30.0
    r = oracle.trace_mesh(k0, cam, V, F, 0.25, r_s=0.0, lambda_end=lam, rhs_form=rhs)
    # the line cam + s lam k against every triangle's plane coordinates: [-lam k, e1, e2] (s, u, v) = cam - v0, one linear solve
    # per triangle (numpy's LU, not the Moeller-Trumbore products of either restatement)
    tv = np.asarray(V, float)[F]
    v0, e1, e2 = tv[:, 0], tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]
    hits = 0
    for i in range(n):
        A = np.stack([np.broadcast_to(-lam * k0[i], e1.shape), e1, e2], -1)
        s, u, v = np.linalg.solve(A, (cam - v0)[:, :, None])[:, :, 0].T
        ok = (s >= 0.0) & (s <= 1.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0)
        if not ok.any():
            assert r["tri"][i] == -1 and r["flags"][i] == 4 and np.abs(r["end"][i, :3] - (cam + lam * k0[i])).max() < 1e-12
            continue
        idx = np.flatnonzero(ok)
        j = idx[np.argmin(s[idx])]
        # (a second triangle within 1e-9 of the first along the line would make "first" a matter of rounding: there is none)
        assert np.sort(s[idx])[1] - s[j] > 1e-9 if len(idx) > 1 else True
        hits += 1
        assert r["tri"][i] == j and r["flags"][i] == 0x88
        assert np.abs(r["end"][i, :3] - (cam + s[j] * lam * k0[i])).max() < 1e-12 and np.abs(r["end"][i, 3:] - k0[i]).max() < 1e-14
        assert np.abs(r["bary"][i] - [u[j], v[j]]).max() < 1e-11
    assert hits > 200


# ---- 4. what the library refuses, the oracle refuses -------------------------------------------------------------------------
def test_refusals(oracle):
    V, F = mr.tetrahedron((5.0, 0.0, 0.0), 1.0)
    k0 = np.array([[-1.0, 0.0, 0.0]])
    x0 = np.array([10.0, 0.0, 0.0])
    assert oracle.trace_mesh(k0, x0, V, F, 0.25)["tri"][0] >= 0
    for chord, kw in ((0.25, dict(method=oracle.METHOD_RK4)), (0.25, dict(time_like=1)), (0.0, {}), (-1.0, {}), (np.nan, {}), (np.inf, {}),
                      (0.25, dict(spheres=[[0.0, 4.0, 0.0, 1.0]]))):
        with pytest.raises(RuntimeError):
            oracle.trace_mesh(k0, x0, V, F, chord, **kw)
    with pytest.raises(RuntimeError):
        oracle.trace_mesh(k0, x0, V, np.array([[0, 1, 4]], np.int32), 0.25)          # an index outside the vertices


def _bulge_hits(oracle, case, o):
    """The hit rays whose hit step's two ends span a box that misses the mesh's box: only the dense output between them reaches
    the mesh.  The ends are the plain trace's states under a step budget of one less than, and of, the hit step's number."""
    lo, hi = case["V"].min(0), case["V"].max(0)
    out = []
    for i in np.flatnonzero(o["tri"] >= 0):
        a = int(o["n_attempted"][i])
        ends = [oracle.trace(case["k0"][i:i + 1], case["x0"], rhs_form=case["rhs"], spin=case["spin"], **dict(case["par"], max_steps=b))
                for b in (a - 1, a) if b > 0]
        if len(ends) < 2 or ends[1]["n_attempted"][0] != a or ends[0]["flags"][0] != 16:
            continue
        c0, c1 = ends[0]["end"][0, :3], ends[1]["end"][0, :3]
        if np.any(np.minimum(c0, c1) - 1e-12 > hi) or np.any(np.maximum(c0, c1) + 1e-12 < lo):
            out.append(i)
    return out


# ---- 5. the conditions of the GPU module's cases -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_conditions(oracle, name):
    case = CASES[name]
    o = mo.oracle_solve(oracle, case)
    n = len(case["k0"])
    unstable = int((~o["stable"]).sum())
    cl = {k: int(v.sum()) for k, v in mo.classes(o).items()}
    print(f"{name}: {n} rays, {len(case['F'])} triangles, {cl}, unstable {unstable}, M up to {int(o['M'].max())}")
    assert unstable <= mo.UNSTABLE_CAP * n, unstable
    t = o["tri"]
    have = dict(cl)
    if name.startswith("frame_"):
        have.update(sphere=int(((t >= 0) & (t < 512)).sum()), sliver=int(((t >= 512) & (t < 536)).sum()), large=int((t == 536).sum()))
        assert len(case["F"]) >= 512 and np.all(np.linalg.norm(o["end"][t == 536, :3], axis=1) <= case["par"]["r_exit"] + 1e-9)
    if name == "m_is_1":
        assert np.all(o["M"][t >= 0] == 1)
    if name == "m_at_cap":
        have["cap"] = int((o["M"] == mo.mr.MAX_SUBSTEPS).sum())
    if name.startswith("budget_"):
        b = case["par"]["max_steps"]
        free = mo.oracle_run(oracle, case, max_steps=0)
        at, before = (free["tri"] >= 0) & (free["n_attempted"] == b), (free["tri"] >= 0) & (free["n_attempted"] == b + 1)
        have.update(hit_at_budget=int(at.sum()), cut_before_hit=int(before.sum()))
        assert np.array_equal(t[at], free["tri"][at]) and np.all(o["flags"][before] == 16) and np.all(t[before] == -1)
        assert np.all(o["n_attempted"][before] == b)
    if name in ("every_triangle_twice", "flat_plate_twice"):
        assert np.all(t[t >= 0] < len(case["F"]) // 2)
    if name == "grazes_at_the_cap":
        half = mo.oracle_run(oracle, dict(case, chord=case["half_chord"]))
        assert np.all(o["M"][t >= 0] == mr.MAX_SUBSTEPS) and np.all(half["M"][half["tri"] >= 0] == mr.MAX_SUBSTEPS // 2)
        assert np.array_equal(half["n_attempted"][half["tri"] >= 0], o["n_attempted"][half["tri"] >= 0])       # the same step
        have["lost_at_512"] = int(((t >= 0) & (half["tri"] < 0)).sum())
        assert not np.any((t < 0) & (half["tri"] >= 0))
    if name == "bulge_into_the_box":
        have["bulge"] = len(_bulge_hits(oracle, case, o))
    if name == "just_above_the_disk":
        # the disk's root of the same ray, from the trace without the mesh: less than 1e-3 behind the triangle's root
        plain = oracle.trace(case["k0"], case["x0"], rhs_form=case["rhs"], spin=case["spin"], **case["par"])
        free = mo.oracle_run(oracle, case, disk_r_in=0.0, disk_r_out=0.0)        # ... and the mesh's root without the disk
        both = (t >= 0) & (plain["flags"] == 128) & (plain["n_attempted"] == o["n_attempted"])      # the same step holds both roots
        dist = np.linalg.norm(plain["end"][:, :3] - o["end"][:, :3], axis=1)       # (|k| = 1 up to the metric's O(r_s / r))
        have["close_call"] = int((both & (dist < 0.9e-3)).sum())
        assert np.all(o["end"][both, 0] < 0.0) and np.all(t[both] <= 1)
        lost = (o["flags"] == 128) & (free["tri"] >= 0) & (free["n_attempted"] == o["n_attempted"])
        assert lost.sum() >= 100 and np.all(o["end"][lost, 0] > 0.0) and np.all(free["tri"][lost] >= 2)
    if name == "lambda_end_inside":
        # hits of the last, clamped step: with lambda_end far away the step is another one, and the refined point another iterate
        free = mo.oracle_run(oracle, case, lambda_end=80.0)
        assert np.array_equal(free["tri"], t)
        have["clamped"] = int(((t >= 0) & (free["end"] != o["end"]).any(1)).sum())
    for key, least in case["want"].items():
        assert have[key] >= least, (key, have[key], least)


def test_fuzz_draws(oracle):
    """The draws tests/test_gpu_mesh_oracle.py runs: the redraw rule (seed + 1000 k while the oracle alone calls more than 1 % of a
    draw's rays unstable) was needed for at most one draw in four, and the draws between them hold every class."""
    redraws, total = 0, dict(hit=0, disk=0, horizon=0, exit=0, end=0, budget=0)
    forms = set()
    for seed in range(mo.N_FUZZ):
        case, o, k = mo.fuzz_case(oracle, seed)
        redraws += k
        forms.add(case["rhs"])
        cl = {key: int(v.sum()) for key, v in mo.classes(o).items()}
        for key in total:
            total[key] += cl[key]
        print(f"fuzz {seed}: redraws {k}, form {case['rhs']}, {len(case['k0'])} rays, {len(case['F'])} triangles, chord {case['chord']}, {cl}, "
              f"unstable {int((~o['stable']).sum())}")
        assert 50 <= len(case["F"]) <= 300
    assert redraws <= mo.N_FUZZ / 4, redraws
    if mo.N_FUZZ >= 8:
        assert forms == {0, 1, 2} and all(v >= 20 for v in total.values()), (forms, total)

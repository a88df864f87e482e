"""The cases on which the mesh trace is held to the C oracle's brute-force restatement of DESIGN.md section 19
(oracle.trace_mesh): tests/test_mesh_oracle_host.py asserts each case's conditions on the CPU -- at most 1 % of its rays
unstable in the oracle, at least the stated number of rays per event class -- and tests/test_gpu_mesh_oracle.py compares the
device with the oracle on every ray of the same cases.  Not a test module: names -> rays, mesh, parameters, chord, and the
oracle calls and the hit bound both files share.

A case is a dict: rhs, spin, par (make_params keywords), V, F, chord, k0, x0, mode ("exact": Schwarzschild, every stable ray step
for step; "kerr": the step_flips rule of tests/test_gpu_parity.py; "fuzz": its rules for randomised draws), want (class -> the
smallest number of rays of that class the case exists to exercise; classes: see classes())."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_reference as mr  # noqa: E402

# restated from tests/test_gpu_mesh.py (test_golden_parity): a mesh hit is a plane root on the dense output, the disk class -- its
# stated fp64 bound (Schwarzschild, Kerr) and the multiple of a ray's own 1-ulp input sensitivity allowed on top
STATED_DISK = (1e-10, 1e-9)
COND = (500.0, 5000.0)
UNSTABLE_CAP = 0.01             # the golden's own cap (tests/test_gpu_mesh.py::test_golden_parity)
SCALINGS = (1e-16, -1e-16, 2e-16, -2e-16, 3e-16, -3e-16, 4e-16, -4e-16)
FRAME_CAM = np.array([18.0, 2.0, 4.0])
FRAME_SPHERE = (-3.0, 1.0, 0.3)
CAM = np.array([20.0, 0.0, 2.0])
BEHIND = (-4.0, 0.5, 0.0)
SIDE = (3.0, 3.5, 1.0)


# ---- the oracle calls ------------------------------------------------------------------------------------------------------
def oracle_run(oracle, case, k0=None, x0=None, **override):
    par = dict(case["par"], **override)
    return oracle.trace_mesh(case["k0"] if k0 is None else k0, case["x0"] if x0 is None else x0, case["V"], case["F"], case["chord"],
                             rhs_form=case["rhs"], spin=case["spin"], **par)


def oracle_solve(oracle, case):
    """oracle_run plus sens [n] (the end record's largest movement under the three 1-2 ulp perturbations of k0, the patterns of
    _sensitivity in tests/test_gpu_parity.py) and stable [n] (flag, triangle, step counts and M unchanged under them)."""
    o = oracle_run(oracle, case)
    k0 = np.asarray(case["k0"], float)
    n = len(k0)
    o["sens"], o["stable"] = np.zeros(n), np.ones(n, bool)
    for kp in mr.perturbations(k0):
        q = oracle_run(oracle, case, k0=kp)
        for key in ("flags", "tri", "n_attempted", "n_accepted", "M"):
            o["stable"] &= q[key] == o[key]
        with np.errstate(invalid="ignore"):
            o["sens"] = np.fmax(o["sens"], np.abs(q["end"] - o["end"]).max(1))
    return o


def oracle_nearby(oracle, case, i):
    """The (flag, triangle, attempted, accepted) the oracle gives ray i when its k0 is scaled by 1 +- 1 ... 4e-16."""
    x0 = case["x0"] if np.ndim(case["x0"]) == 1 else np.asarray(case["x0"])[i:i + 1]
    seen = set()
    for eps in SCALINGS:
        q = oracle_run(oracle, case, k0=np.asarray(case["k0"])[i:i + 1] * (1.0 + eps), x0=x0)
        seen.add((int(q["flags"][0]), int(q["tri"][0]), int(q["n_attempted"][0]), int(q["n_accepted"][0])))
    return seen


def hit_tolerances(V, F, ref_end, ref_tri, sens, kerr):
    """test_golden_parity's bound on the hit rays given: (tol on end, shortest edge of the ray's triangle); bary is held to
    tol / shortest."""
    v0, e1, e2 = mr.tri_arrays(V, F)
    nT = np.cross(e1[ref_tri], e2[ref_tri])
    nT /= np.linalg.norm(nT, axis=1)[:, None]
    kdir = ref_end[:, 3:]
    graze = np.linalg.norm(kdir, axis=1) / np.abs(np.einsum("ij,ij->i", nT, kdir))
    tol = STATED_DISK[kerr] + COND[kerr] * sens + 1e-11 * graze
    shortest = np.minimum.reduce([np.linalg.norm(e1[ref_tri], axis=1), np.linalg.norm(e2[ref_tri], axis=1),
                                  np.linalg.norm(e2[ref_tri] - e1[ref_tri], axis=1)])
    return tol, shortest


def classes(o):
    """class -> mask, on an oracle (or device) result."""
    f = o["flags"]
    return dict(hit=(f == 0x88) & (o["tri"] >= 0), disk=f == 128, horizon=(f & 1) != 0, exit=f == 8, end=f == 4, budget=f == 16)


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def slivers(n, rng, about, length=3.0, width=0.03, spread=1.5):
    """n thin triangles (aspect ~ length / width) scattered about a point."""
    base = np.asarray(about, float) + rng.normal(size=(n, 3)) * spread
    along = rng.normal(size=(n, 3))
    along *= length / np.linalg.norm(along, axis=1)[:, None]
    across = rng.normal(size=(n, 3))
    across *= width / np.linalg.norm(across, axis=1)[:, None]
    V = np.stack([base, base + along, base + 0.5 * along + across], 1).reshape(-1, 3)
    return V, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def frame_mesh():
    """The 512-triangle sphere cut by the disk plane, 24 slivers between it and the camera, and one large triangle behind the
    hole whose corners lie at r = 30.1, 25.9 and 41.7: it straddles an exit sphere of 30."""
    big = (np.array([[-26.0, -14.0, -6.0], [-20.0, 16.0, -4.0], [-34.0, 2.0, 24.0]]), np.array([[0, 1, 2]], np.int32))
    return mr.join(mr.octa_sphere(FRAME_SPHERE, 1.2, 3), slivers(24, np.random.default_rng(5), (1.0, -2.5, 1.5)), big)


def frame_rays(n=2048, seed=11):
    rng = np.random.default_rng(seed)
    a, b, c = (n * 7) // 16, n // 4, (n * 3) // 16
    return np.concatenate([mr.camera_rays(FRAME_CAM, FRAME_SPHERE, a, rng, 2.5), mr.hole_rays(FRAME_CAM, b, rng, 0.3, 6.0),
                           mr.hole_rays(FRAME_CAM, c, rng, 6.0, 16.0), mr.camera_rays(FRAME_CAM, (1.0, -2.5, 1.5), n - a - b - c, rng, 2.5)])


def flat_plate(z, half, m):
    """The square |x|, |y| <= half in the plane z: m x m cells of two triangles."""
    g = np.linspace(-half, half, m + 1)
    V = np.array([(x, y, z) for y in g for x in g])
    F = [t for j in range(m) for i in range(m) for a in [j * (m + 1) + i] for t in ((a, a + 1, a + m + 2), (a, a + m + 2, a + m + 1))]
    return V, np.array(F, np.int32)


def doubled(V, F, rng):
    """Every triangle twice: the second copies in another order, so that a copy's index says nothing about where the tree puts it."""
    return V, np.concatenate([F, F[rng.permutation(len(F))]]).astype(np.int32)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _case(rhs, spin, par, mesh, chord, k0, x0, mode=None, **want):
    return dict(rhs=rhs, spin=spin, par=par, V=np.ascontiguousarray(mesh[0], dtype=np.float64), F=np.ascontiguousarray(mesh[1], dtype=np.int32),
                chord=chord, k0=np.ascontiguousarray(k0), x0=np.ascontiguousarray(x0), mode=mode or ("kerr" if rhs == 2 else "exact"), want=want)


def frame_cases():
    par = dict(r_s=1.0, lambda_end=46.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    k0, mesh = frame_rays(), frame_mesh()
    want = dict(hit=200, disk=100, horizon=50, exit=150, end=20, sphere=90, sliver=5, large=50)
    return {
        "frame_christoffel": _case(0, 0.0, par, mesh, 0.25, k0, FRAME_CAM, **want),
        "frame_reduced": _case(1, 0.0, par, mesh, 0.25, k0, FRAME_CAM, **want),
        "frame_kerr_plus": _case(2, 0.45, par, mesh, 0.25, k0, FRAME_CAM, **want),
        "frame_kerr_minus": _case(2, -0.45, par, mesh, 0.25, k0, FRAME_CAM, **want),
    }


BUDGETS = (7, 8)        # of "budget_*": see parameter_cases


def parameter_cases():
    rng = np.random.default_rng(23)
    # two closed 128-triangle spheres: one behind the hole (secondary images: rays that wind round it) and one beside it, in
    # plain view of the camera; the first ray is aimed at the middle of that one
    both = mr.join(mr.octa_sphere(BEHIND, 1.5, 2), mr.octa_sphere(SIDE, 1.5, 2))
    k_side = mr.camera_rays(CAM, SIDE, 150, rng, 2.2)
    k_side[0] = (np.asarray(SIDE) - CAM) / np.linalg.norm(np.asarray(SIDE) - CAM)
    k_both = np.concatenate([k_side, mr.hole_rays(CAM, 150, rng, 2.3, 7.0)])
    base = dict(r_s=1.0, lambda_end=80.0, r_exit=40.0)
    out = {}
    out["tight"] = _case(1, 0.0, dict(base, rtol=1e-7, atol=1e-10), both, 0.25, k_both, CAM, hit=80, horizon=5, exit=50)
    out["loose"] = _case(0, 0.0, dict(base, rtol=3e-2, atol=1e-4), both, 0.25, k_both, CAM, hit=80, horizon=5, exit=50)
    # max_step 0.4 under max_chord 1.0: M = 1 on every step (the camera close by, so that the steps stay in the hundreds)
    near = np.array([9.0, 0.5, 1.0])
    k_near = np.concatenate([mr.camera_rays(near, SIDE, 120, rng, 2.0), mr.hole_rays(near, 80, rng, 2.3, 6.0)])
    out["m_is_1"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=30.0, r_exit=16.0, max_step=0.4), both, 1.0, k_near, near, hit=60, horizon=3, exit=20)
    # max_chord 2e-3: every step longer than 2.046 has M at its cap; 12 triangles, so that 1024 sub-chords a step stay cheap
    small = mr.join(mr.octa_sphere(BEHIND, 1.5, 0), mr.tetrahedron((9.0, 0.3, 1.2), 0.8))
    k_small = np.concatenate([mr.hole_rays(CAM, 100, rng, 2.3, 6.0), mr.camera_rays(CAM, (9.0, 0.3, 1.2), 60, rng, 1.4)])
    out["m_at_cap"] = _case(1, 0.0, dict(base), small, 2e-3, k_small, CAM, hit=40, cap=20)
    # a step budget that runs out at the hit step (the hit stays) or one step before it (MAX_STEPS): each budget b has rays that
    # hit in attempt b and rays that would have hit in attempt b + 1 (the host test counts them on the run without a budget)
    for b in BUDGETS:
        out[f"budget_{b}"] = _case(0, 0.0, dict(base, max_steps=b), both, 0.25, k_both, CAM, hit_at_budget=10, cut_before_hit=10)
    # lambda_end inside the closed mesh beside the hole (its centre is 17.4 from the camera, its near side 15.9): the last,
    # clamped step holds the hit; and just in front of it: rays aimed at its middle arrive, rays aimed at its limb reach
    # lambda_end first
    side = mr.octa_sphere(SIDE, 1.5, 2)
    k_direct = mr.camera_rays(CAM, SIDE, 300, rng, 1.4)
    out["lambda_end_inside"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=17.6), side, 0.25, k_direct, CAM, hit=150, clamped=20)
    out["lambda_end_in_front"] = _case(1, 0.0, dict(r_s=1.0, lambda_end=16.15), side, 0.25, k_direct, CAM, hit=50, end=50)
    # the camera inside a closed mesh
    cam_in = np.array([9.0, 1.0, 2.0])
    k_all = rng.normal(size=(300, 3))
    k_all /= np.linalg.norm(k_all, axis=1)[:, None]
    out["camera_inside"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=60.0, max_step=0.7), mr.octa_sphere(cam_in + [0.3, -0.2, 0.1], 2.0, 2), 0.25,
                                 k_all, cam_in, hit=300)
    # per-ray origins
    x_each = CAM[None, :] + rng.normal(size=(300, 3)) * 0.8
    out["per_ray_origins"] = _case(1, 0.0, dict(base, disk_r_in=2.0, disk_r_out=7.0), both, 0.25, k_both, x_each, hit=40, disk=20, exit=30)
    # sizes around a wave
    for n in (1, 63, 65):
        out[f"n_{n}"] = _case(0, 0.0, dict(base), both, 0.25, k_both[:n], CAM, hit=1 if n == 1 else 20)
    # a closed mesh that reaches inside r_s: its centre at r = 1.0, its radius 0.9 -- rays that meet a triangle first, and rays
    # that meet the horizon first with triangles behind it
    cam_h = np.array([1.0, -14.0, 5.0])
    out["inside_the_horizon"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=40.0, r_exit=20.0), mr.octa_sphere((1.0, 0.0, 0.0), 0.9, 2), 0.1,
                                      mr.hole_rays(cam_h, 400, rng, 0.0, 3.5), cam_h, hit=40, horizon=60)
    # Kerr: a mesh pierced by the spin axis, and one through the equatorial plane with the disk set
    cam_k = np.array([14.0, 3.0, 9.0])
    out["kerr_on_the_axis"] = _case(2, 0.45, dict(r_s=1.0, lambda_end=60.0, r_exit=30.0), mr.octa_sphere((0.0, 0.0, 4.0), 1.3, 2), 0.25,
                                    np.concatenate([mr.camera_rays(cam_k, (0.0, 0.0, 4.0), 250, rng, 1.8), mr.hole_rays(cam_k, 50, rng, 0.3, 5.0)]),
                                    cam_k, hit=100)
    out["kerr_through_the_disk"] = _case(2, -0.3, dict(r_s=1.0, lambda_end=60.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=8.0),
                                         mr.octa_sphere((-3.5, 1.0, 0.2), 1.5, 2), 0.25,
                                         np.concatenate([mr.camera_rays(cam_k, (-3.5, 1.0, 0.2), 200, rng, 2.2), mr.hole_rays(cam_k, 100, rng, 0.3, 6.0)]),
                                         cam_k, hit=40, disk=30)
    # a mesh at coordinates of the order 1e3, the camera next to it
    far_c = np.array([1000.0, 300.0, -200.0])
    far_cam = far_c + [9.0, 2.0, 1.5]
    out["far_away"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=30.0), mr.join(mr.octa_sphere(far_c, 1.5, 2), slivers(12, rng, far_c + [4.0, 1.0, 0.5])), 0.25,
                            mr.camera_rays(far_cam, far_c, 300, rng, 2.5), far_cam, hit=100, end=50)
    # steps so long (rtol 0.1) and an object so small that the box of a step's two ends misses the object's box while the dense
    # output between them bulges into it: the whole-step cull has to count the bulge ("bulge": such hits, counted by the host test)
    out["bulge_into_the_box"] = _case(0, 0.0, dict(base, rtol=1e-1, atol=1e-4), mr.octa_sphere((-1.0, 3.0, 0.0), 0.3, 1), 0.25,
                                      mr.hole_rays(CAM, 1200, np.random.default_rng(3), 2.6, 5.0), CAM, hit=15, bulge=15)
    # a plate 4e-4 above the disk plane over x < 0 and one 4e-4 below it over x > 0, the camera above: over x < 0 the triangle's
    # root lies less than 1e-3 in front of the disk's root in the same step and wins, over x > 0 it lies behind it and loses
    plates = (np.array([[-10.0, -10.0, 4e-4], [0.0, -10.0, 4e-4], [0.0, 10.0, 4e-4], [-10.0, 10.0, 4e-4],
                        [0.0, -10.0, -4e-4], [10.0, -10.0, -4e-4], [10.0, 10.0, -4e-4], [0.0, 10.0, -4e-4]]),
              np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32))
    cam_d = np.array([3.0, -14.0, 9.0])
    k_disk = np.concatenate([mr.camera_rays(cam_d, (-4.0, 0.0, 0.0), 150, rng, 2.5), mr.camera_rays(cam_d, (4.0, 0.0, 0.0), 150, rng, 2.5)])
    out["just_above_the_disk"] = _case(1, 0.0, dict(r_s=1.0, lambda_end=60.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=8.0), plates, 0.25,
                                       k_disk, cam_d, hit=100, disk=100, close_call=100)
    # the cap itself: 400 rays a few 1e-10 apart in direction that graze one large triangle -- its plane cuts 1e-3 into the convex
    # side of their path where it bends round the hole, inside a step of length 3.37 -- from just short of touching the plane to a
    # passage so short that only the 1024 samples of the capped step have one inside it.  The rays that touch are hits with
    # M = 1024; a third of those would be misses with 512 samples (the host test counts them: the same step has M = 512 at
    # max_chord 0.00659).  The triangle and the transition were found with the oracle's sampled trajectory and a bisection.
    graze = (np.array([[1.1135337935962504, 3.8001478393038437, 1.6188347225277586], [-2.787483785989433, 3.0064964912919554, 1.2287329645691902],
                       [-0.4389601201125956, 3.4033221652978995, -2.5563649172914817]]), np.array([[0, 1, 2]], np.int32))
    k_c = np.array([-0.9740003060309442, 0.2045400642664983, -0.09740003060309442])
    k_u = np.array([0.20352497083310706, 0.9788581930544672, 0.020352497083310706])
    k_graze = k_c[None, :] + (-4.794303387391813e-05 + np.linspace(-2e-8, 1e-7, 400))[:, None] * k_u[None, :]
    k_graze /= np.linalg.norm(k_graze, axis=1)[:, None]
    out["grazes_at_the_cap"] = _case(0, 0.0, dict(r_s=1.0, lambda_end=60.0, r_exit=40.0), graze, 2e-3, k_graze, CAM, hit=300, end=50, lost_at_512=50)
    out["grazes_at_the_cap"]["half_chord"] = 0.00659
    # a flat, axis-aligned plate of 128 triangles, every one twice, 0.06 across and next to a small hole: node boxes of no
    # thickness, at coordinates far smaller than the distance from which a sub-chord (max_chord 1.0) starts -- half the rays come
    # down on it steeply from 3 away, half graze it from the side
    prng = np.random.default_rng(77)
    x_plate = np.where((np.arange(400) < 200)[:, None], np.array([0.3, 0.2, 3.0]) + prng.normal(size=(400, 3)) * 0.2,
                       np.array([3.0, 0.5, 0.12]) + prng.normal(size=(400, 3)) * [0.2, 0.2, 0.03])
    aim = np.stack([prng.uniform(-0.055, 0.055, 400), prng.uniform(-0.055, 0.055, 400), np.full(400, 0.03)], 1)
    k_plate = (aim - x_plate) / np.linalg.norm(aim - x_plate, axis=1)[:, None]
    out["flat_plate_twice"] = _case(0, 0.0, dict(r_s=0.02, lambda_end=8.0), doubled(*flat_plate(0.03, 0.06, 8), prng), 1.0, k_plate, x_plate, hit=350)
    # every triangle twice
    out["every_triangle_twice"] = _case(0, 0.0, dict(base), doubled(*both, rng), 0.25, k_both, CAM, hit=80)
    return out


# ---- the fuzz --------------------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("BHG_FUZZ_MESH", "8"))
REDRAW_STEP = 1000          # a draw whose oracle run alone exceeds UNSTABLE_CAP is drawn again with seed + 1000 k, k = 1, 2, 3
REDRAWS_MAX = 3


def fuzz_draw(seed):
    """One randomised configuration, drawn as test_randomised_configurations (tests/test_gpu_parity.py) draws its own -- metric size,
    camera, tolerances, max_step, max_steps, exit sphere, disk, form -- plus the form Kerr, a triangle soup of 50 to 300 triangles
    (some zero-area, some duplicated) with a closed shape, and max_chord."""
    rng = np.random.default_rng(7000 + seed)
    r_s = float(rng.choice([0.3, 1.0, 2.5]))
    unit = max(r_s, 0.5)
    dist_cam = float(rng.uniform(6.0, 40.0)) * unit
    cam = rng.normal(size=3)
    cam[2] *= 0.7
    cam = dist_cam * cam / np.linalg.norm(cam)
    rhs = int(rng.integers(0, 3))
    spin = float(rng.uniform(-0.95, 0.95)) * 0.5 * r_s if rhs == 2 else 0.0
    if rhs == 2 and abs(cam[0]) + abs(cam[1]) < 0.05 * dist_cam:      # off the polar axis, as test_randomised_kerr keeps it
        cam[0] += 0.2 * dist_cam
    n = int(rng.integers(100, 600))
    spread = unit * float(rng.uniform(2.0, 6.0))
    aim = rng.normal(size=(n, 3)) * spread
    k = aim - cam
    k /= np.linalg.norm(k, axis=1)[:, None]
    x0 = cam + rng.normal(size=(n, 3)) * 0.05 * dist_cam if rng.random() < 0.3 else cam
    par = dict(r_s=r_s, lambda_end=float(rng.uniform(1.2, 3.0)) * dist_cam)
    mode = int(rng.integers(0, 3))
    if mode == 0:
        par.update(rtol=float(10 ** rng.uniform(-6, -2)), atol=float(10 ** rng.uniform(-9, -4)))
    elif mode == 1:
        par.update(max_step=float(rng.uniform(0.3, 2.0)) * unit)
    if rng.random() < 0.4:
        par["r_exit"] = float(rng.uniform(0.5, 1.5)) * dist_cam
    if rng.random() < 0.4:
        a = float(rng.uniform(1.5, 6.0)) * unit
        par.update(disk_r_in=a, disk_r_out=a * float(rng.uniform(1.1, 3.0)))
    if rng.random() < 0.2:
        par["max_steps"] = int(rng.integers(4, 40))
    # the soup: nt triangles scattered over the region the rays are aimed at, a tenth of them zero-area (a repeated corner), a tenth
    # copies of earlier ones; and a closed sphere of 32 triangles somewhere in it
    total = int(rng.integers(50, 301))
    nt = ((total - 32) * 10) // 11
    V, F = mr.random_triangles(nt, rng, spread=1.2 * spread, size=0.25 * spread)
    for j in rng.choice(nt, nt // 10, replace=False):
        F[j, 2] = F[j, int(rng.integers(0, 2))]
    F = np.concatenate([F, F[rng.choice(nt, total - 32 - nt, replace=False)]])
    centre = rng.normal(size=3) * spread
    closed = mr.octa_sphere(centre, float(rng.uniform(0.5, 1.5)) * unit, 1)
    mesh = mr.join((V, F), closed)
    chord = float(rng.choice([0.1, 0.25, 1.0])) * unit
    return _case(rhs, spin, par, mesh, chord, k, x0, mode="fuzz")


def fuzz_case(oracle, seed):
    """-> (case, oracle_solve of it, redraws needed): seed, seed + 1000, ... until the oracle alone calls at most UNSTABLE_CAP of
    the draw's rays unstable."""
    for k in range(REDRAWS_MAX + 1):
        case = fuzz_draw(seed + REDRAW_STEP * k)
        o = oracle_solve(oracle, case)
        if (~o["stable"]).mean() <= UNSTABLE_CAP:
            return case, o, k
    raise AssertionError(f"fuzz seed {seed}: {REDRAWS_MAX} redraws and still more than {UNSTABLE_CAP:.0%} of the rays unstable")

"""Triangle meshes in the curved region on the GPU: bhg_trace_mesh_device against the scipy golden vectors
(tests/golden/mesh.npz, tests/mesh_reference.py's restatement of the hit rule), against itself with other trees and without the
whole-step cull (bit for bit), against the plain trace when nothing is met, against the analytic object sphere, its ordering with
the other events and its edge cases, and bhg_shade_mesh_device / DeviceFrame.set_mesh against the numpy restatement of the mesh
colour.

Measured when this was written (MI355X): golden parity -- flags, n_accepted and tri_id identical on all 4 x 480 rays, none marked
unstable; worst |end - ref| on hits 2.8e-11 (Schwarzschild, bound 1e-10 + ...) and 3.3e-11 (Kerr, 1e-9 + ...), worst |bary - ref|
3.2e-11.  Sandwich: inscribed radius 0.99612; 674 mesh hits, 652 rays on the sphere of 0.98, 681 on the sphere of 1.01, |x - c| of
the hits in [0.99623, 0.99990].  Shade: worst |gpu - numpy| 2.2e-16, smallest shadow margin 5.1e-7."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_cases as mc  # noqa: E402
import mesh_reference as mr  # noqa: E402

# restated from tests/test_gpu_disk_crossings.py: a mesh hit is a plane root on the dense output, the disk class -- its stated fp64
# bound (Schwarzschild, Kerr) and the multiple of a record's own 1-ulp input sensitivity S_i that is allowed on top
STATED_DISK = (1e-10, 1e-9)
COND = (500.0, 5000.0)
SENTINEL = mc.SENTINEL
KEYS = ("end", "flags", "n_steps", "n_accepted", "tri", "bary")


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def _plain_device(ctx, p, k0, x0, spheres=None):
    """bhg_trace_device / bhg_trace_objects_device -> dict(end, flags, n_steps, n_accepted[, obj])."""
    import torch
    n = len(k0)
    d_k0 = torch.as_tensor(np.ascontiguousarray(k0, dtype=np.float64)).cuda()
    shared = np.asarray(x0).ndim == 1
    d_x0 = None if shared else torch.as_tensor(np.ascontiguousarray(x0, dtype=np.float64)).cuda()
    d_end = torch.full((n, 6), SENTINEL, dtype=torch.float64, device="cuda")
    d_fl = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_ac = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_obj = torch.full((n,), -9, dtype=torch.int8, device="cuda")
    ctx.trace_device(p, n, d_k0.data_ptr(), d_end.data_ptr(), x0_shared=x0 if shared else None, d_x0=0 if shared else d_x0.data_ptr(),
                     d_flags=d_fl.data_ptr(), d_n_steps=d_st.data_ptr(), d_n_accepted=d_ac.data_ptr(),
                     stream=torch.cuda.current_stream().cuda_stream, spheres=spheres, d_object_id=d_obj.data_ptr() if spheres is not None else 0)
    torch.cuda.synchronize()
    return dict(end=d_end.cpu().numpy(), flags=d_fl.cpu().numpy(), n_steps=d_st.cpu().numpy().astype(np.uint32),
                n_accepted=d_ac.cpu().numpy().astype(np.uint32), obj=d_obj.cpu().numpy())


@pytest.fixture(scope="module")
def golden():
    return load_golden("mesh")


@pytest.fixture(scope="module")
def culled(ctx):
    """Every case of mesh_cases.cull_cases() in this process (the whole-step cull on): computed once, shared by tests 1 and 3."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0"
    return mc.run_cases(ctx)


# ---- 1. the golden vectors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fi", range(len(mr.GOLDEN_FORMS)), ids=mr.GOLDEN_FORM_IDS)
def test_golden_parity(ctx, golden, culled, fi):
    g = golden
    rhs, a = mr.GOLDEN_FORMS[fi]
    kerr = rhs == 2
    bound, cond = STATED_DISK[kerr], COND[kerr]
    unstable_total = rays_total = 0
    for name, (V, F) in mr.golden_meshes().items():
        r = {k: culled[f"golden_{mr.GOLDEN_FORM_IDS[fi]}_{name}__{k}"] for k in KEYS}
        ref = {k: g[f"{name}_{k}"][fi] for k in ("end", "flags", "n_attempted", "n_accepted", "tri", "bary", "sens", "stable")}
        stable = ref["stable"]
        unstable_total += int((~stable).sum())
        rays_total += len(stable)
        assert np.array_equal(r["flags"], ref["flags"]), np.flatnonzero(r["flags"] != ref["flags"])
        assert np.array_equal(r["n_accepted"][stable], ref["n_accepted"][stable])
        assert np.array_equal(r["tri"][stable], ref["tri"][stable])
        hit = stable & (ref["tri"] >= 0)
        miss = ref["tri"] < 0
        # (scipy's attempted count is not comparable where it integrated on past the event: triangle hits, as for the disk)
        cmp = miss & stable & (ref["n_attempted"] >= 0)
        assert np.array_equal(r["n_steps"][cmp], ref["n_attempted"][cmp].astype(np.uint32))
        assert np.all(r["bary"][r["tri"] < 0] == SENTINEL) and np.all(r["tri"][miss & stable] == -1)
        v0, e1, e2 = mr.tri_arrays(V, F)
        t = ref["tri"][hit]
        nT = np.cross(e1[t], e2[t])
        nT /= np.linalg.norm(nT, axis=1)[:, None]
        kdir = ref["end"][hit, 3:]
        graze = np.linalg.norm(kdir, axis=1) / np.abs(np.einsum("ij,ij->i", nT, kdir))
        tol = bound + cond * ref["sens"][hit] + 1e-11 * graze
        diff = np.abs(r["end"][hit] - ref["end"][hit]).max(1)
        shortest = np.minimum.reduce([np.linalg.norm(e1[t], axis=1), np.linalg.norm(e2[t], axis=1),
                                      np.linalg.norm(e2[t] - e1[t], axis=1)])
        dbary = np.abs(r["bary"][hit] - ref["bary"][hit]).max(1)
        print(f"{mr.GOLDEN_FORM_IDS[fi]} {name}: {int(hit.sum())} stable hits, {int((~stable).sum())} unstable, worst |end - ref| "
              f"{diff.max():.3e} (excess over its tolerance {np.max(diff - tol):.3e}), worst |bary - ref| {dbary.max():.3e}")
        assert hit.sum() >= 10
        assert np.all(diff <= tol), (diff - tol).max()
        assert np.all(dbary <= tol / shortest), (dbary - tol / shortest).max()
    print(f"{mr.GOLDEN_FORM_IDS[fi]}: {unstable_total} of {rays_total} golden rays marked unstable (compared on flags only)")
    assert unstable_total <= 0.01 * rays_total


# ---- 2. the tree changes nothing -------------------------------------------------------------------------------------------
def _tree_cases(golden):
    cam = np.array([18.0, 2.0, 4.0])
    k512 = np.concatenate([mc.frame_rays_at(cam, (-3.0, 1.0, 0.5), 700, 3, 3.0), mr.hole_rays(cam, 324, np.random.default_rng(8))])
    far = np.array([0.0, 39.6, 3.0])          # a sphere that straddles the exit sphere at 40
    kfar = mc.frame_rays_at(mr.GOLDEN_CAM, far, 600, 9, 2.5)
    return {
        "golden_behind": (0, 0.0, dict(r_exit=40.0, **mr.GOLDEN_PAR), mr.golden_meshes()["behind"], 0.25, golden["behind_k0"], golden["x0"]),
        "golden_two_kerr": (2, 0.45, dict(**mr.GOLDEN_PAR), mr.golden_meshes()["two"], 0.25, golden["two_k0"], golden["x0"]),
        "sphere512": (1, 0.0, dict(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=2.0, disk_r_out=6.0),
                      mr.octa_sphere((-3.0, 1.0, 0.5), 1.2, 3), 0.2, k512, cam),
        "straddles_exit": (0, 0.0, dict(r_s=1.0, lambda_end=90.0, r_exit=40.0), mr.octa_sphere(far, 1.5, 2), 0.25, kfar, mr.GOLDEN_CAM),
    }


@pytest.mark.parametrize("case", ["golden_behind", "golden_two_kerr", "sphere512", "straddles_exit"])
def test_the_tree_changes_nothing(ctx, golden, case):
    f = _ffi()
    rhs, a, par, (V, F), chord, k0, x0 = _tree_cases(golden)[case]
    p = f.make_params(rhs_form=rhs, spin=a, **par)
    res = []
    for leaf in (1, 4, len(F)):
        mesh = f.Mesh(ctx, V, F, leaf_size=leaf)
        nn, depth, box = mesh.info()
        assert (nn == 1) == (leaf == len(F)) and depth <= 32 and np.all(box[:3] <= V.min(0)) and np.all(box[3:] >= V.max(0))
        res.append(mc.trace_mesh_device(ctx, p, mesh, chord, k0, x0))
        mesh.close()
    hits = int((res[0]["tri"] >= 0).sum())
    print(f"{case}: {hits} of {len(k0)} rays end on the mesh, {int((res[0]['flags'] == 8).sum())} leave the exit sphere")
    assert hits >= 20
    if case == "straddles_exit":
        assert (res[0]["flags"] == 8).sum() >= 20
        x = res[0]["end"][res[0]["tri"] >= 0, :3]
        assert np.all(np.linalg.norm(x, axis=1) <= 40.0 + 1e-9)        # no hit beyond the exit sphere
    assert _same(res[0], res[1]) and _same(res[0], res[2])


# ---- 3. the cull changes nothing -------------------------------------------------------------------------------------------
def test_the_cull_changes_nothing(ctx, culled, tmp_path):
    out = str(tmp_path / "nocull.npz")
    env = dict(os.environ, BHGEO_MESH_CULL="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_cases.py"), out], check=True, env=env, timeout=300)
    plain = np.load(out)
    assert sorted(plain.files) == sorted(culled)
    hits = 0
    for k in plain.files:
        assert np.array_equal(plain[k], culled[k]), k
        if k.endswith("__tri"):
            hits += int((plain[k] >= 0).sum())
    assert hits > 600 and (culled["frame4096_christoffel__flags"] == 128).sum() > 50


# ---- 4. a mesh nobody meets is the plain trace -------------------------------------------------------------------------------
@pytest.mark.parametrize("rhs,spin", [(0, 0.0), (1, 0.0), (2, 0.45)], ids=["christoffel", "reduced", "kerr"])
def test_a_mesh_nobody_meets_is_the_plain_trace(ctx, rhs, spin):
    f = _ffi()
    mesh = f.Mesh(ctx, *mr.tetrahedron((500.0, 30.0, -20.0), 3.0))
    cam = np.array([3.0, 0.5, 30.0])
    rng = np.random.default_rng(12)
    for n in (1, 63, 65, 200, 4096):
        k0 = mr.hole_rays(cam, n, rng, 0.3, 9.0)
        for x0 in (cam, cam[None, :] + rng.normal(size=(n, 3)) * 0.5):
            p = f.make_params(r_s=1.0, lambda_end=90.0, r_exit=40.0, rhs_form=rhs, spin=spin)
            m, t = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, x0), _plain_device(ctx, p, k0, x0)
            assert all(np.array_equal(m[k], t[k]) for k in ("end", "flags", "n_steps", "n_accepted"))
            assert np.all(m["tri"] == -1) and np.all(m["bary"] == SENTINEL)
            # with a disk: the opaque-disk trace's flags and counts (the end state within the disk bound: DESIGN.md section 19)
            p = f.make_params(r_s=1.0, lambda_end=90.0, r_exit=40.0, rhs_form=rhs, spin=spin, disk_r_in=2.0, disk_r_out=15.0)
            m, t = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, x0), _plain_device(ctx, p, k0, x0)
            assert all(np.array_equal(m[k], t[k]) for k in ("flags", "n_steps", "n_accepted"))
            assert np.all(m["tri"] == -1)
            assert np.abs(m["end"] - t["end"]).max() <= STATED_DISK[rhs == 2]
            if n == 4096:
                assert (m["flags"] == 128).sum() > 100
    mesh.close()


# ---- 5. the sandwich against the analytic sphere -------------------------------------------------------------------------------
def test_sandwich_against_the_analytic_sphere(ctx):
    f = _ffi()
    c = np.array([0.0, 4.0, 0.0])
    sub = 4
    V, F = mr.octa_sphere(c, 1.0, sub)
    assert len(F) == 2048
    if not mr.inscribed_radius(V, F, c) > 0.98:
        sub += 1
        V, F = mr.octa_sphere(c, 1.0, sub)
    r_in = mr.inscribed_radius(V, F, c)
    assert r_in > 0.98
    cam = np.array([14.0, -6.0, 3.0])
    k0 = np.concatenate([mc.frame_rays_at(cam, c, 2500, 21, 1.3), mr.hole_rays(cam, 1500, np.random.default_rng(22), 1.0, 7.0)])
    p = f.make_params(r_s=1.0, lambda_end=80.0, r_exit=40.0, max_step=0.5)
    mesh = f.Mesh(ctx, V, F)
    m = mc.trace_mesh_device(ctx, p, mesh, 0.1, k0, cam)
    mesh.close()
    inner = _plain_device(ctx, p, k0, cam, spheres=[[*c, 0.98]])
    outer = _plain_device(ctx, p, k0, cam, spheres=[[*c, 1.01]])
    on_mesh = m["tri"] >= 0
    dist = np.linalg.norm(m["end"][on_mesh, :3] - c, axis=1)
    print(f"sub {sub}: inscribed radius {r_in:.5f}; {int(on_mesh.sum())} mesh hits, {int((inner['flags'] == 0x88).sum())} on the sphere "
          f"of 0.98, {int((outer['flags'] == 0x88).sum())} on the sphere of 1.01; |x - c| in [{dist.min():.5f}, {dist.max():.5f}]")
    assert (inner["flags"] == 0x88).sum() > 500 and (outer["flags"] != 0x88).sum() > 500
    assert np.all(on_mesh[inner["flags"] == 0x88])
    assert not np.any(on_mesh[outer["flags"] != 0x88])
    assert np.all((m["flags"] == 0x88) == on_mesh)
    assert dist.min() >= 0.98 and dist.max() <= 1.001


# ---- 6. ordering and edges -----------------------------------------------------------------------------------------------
def _wall(y, half=8.0):
    return np.array([[-half, y, -8.0], [half, y, -8.0], [0.0, y, 9.0]]), np.array([[0, 1, 2]], np.int32)


def test_ordering_with_the_disk_and_the_horizon(ctx):
    f = _ffi()
    x0 = np.array([0.0, -15.0, 6.0])
    k0 = mc.frame_rays_at(x0, (0.0, -5.0, 0.0), 300, 31, 1.0)
    par = dict(r_s=0.2, lambda_end=60.0, r_exit=25.0, disk_r_in=0.5, disk_r_out=20.0)
    p = f.make_params(**par)
    opaque = _plain_device(ctx, p, k0, x0)
    on_disk = opaque["flags"] == 128
    assert on_disk.sum() > 250
    y_disk = opaque["end"][on_disk, 1]
    # nt = 1: a wall behind every disk crossing loses to the disk ...
    mesh = f.Mesh(ctx, *_wall(y_disk.max() + 1.0))
    behind = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, x0)
    mesh.close()
    assert np.array_equal(behind["flags"], opaque["flags"]) and np.all(behind["tri"][on_disk] == -1)
    assert np.array_equal(behind["n_steps"], opaque["n_steps"]) and np.abs(behind["end"] - opaque["end"])[on_disk].max() <= 1e-10
    # ... and in front of every crossing it wins, at its own plane
    y_wall = y_disk.min() - 1.0
    mesh = f.Mesh(ctx, *_wall(y_wall))
    front = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, x0)
    mesh.close()
    won = front["tri"] == 0
    assert won.sum() > 250 and np.all(front["flags"][won] == 0x88) and np.abs(front["end"][won, 1] - y_wall).max() < 1e-12
    assert np.all(front["n_accepted"][won & on_disk] <= opaque["n_accepted"][won & on_disk])
    b = front["bary"][won]
    assert np.all(b >= -1e-3) and np.all(b.sum(1) <= 1.0 + 1e-3)
    # a mesh wholly inside the horizon is never hit (max_step 1: shorter than any chord of the horizon sphere that reaches the
    # mesh, so no step carries a ray across the hole without an end inside it -- section 7's transparent centre is another matter)
    k1 = mr.hole_rays(x0, 400, np.random.default_rng(5), 0.0, 4.0)
    for rhs, a in ((0, 0.0), (1, 0.0), (2, 0.3)):
        p1 = f.make_params(r_s=1.0, lambda_end=60.0, r_exit=25.0, max_step=1.0, rhs_form=rhs, spin=a)
        mesh = f.Mesh(ctx, *mr.octa_sphere((0.0, 0.0, 0.0), 0.6 if rhs != 2 else 0.5, 1))
        inside, plain = mc.trace_mesh_device(ctx, p1, mesh, 0.1, k1, x0), _plain_device(ctx, p1, k1, x0)
        mesh.close()
        assert np.all(inside["tri"] == -1) and (plain["flags"] == 1).sum() > 50
        assert all(np.array_equal(inside[k], plain[k]) for k in ("end", "flags", "n_steps", "n_accepted"))


def test_camera_inside_a_closed_mesh_and_a_zero_area_triangle(ctx):
    f = _ffi()
    cam = np.array([9.0, 1.0, 2.0])
    V, F = mr.octa_sphere(cam + [0.01, -0.02, 0.015], 0.05, 2)
    k0 = mr.hole_rays(cam, 300, np.random.default_rng(41), 0.0, 40.0)
    p = f.make_params(r_s=1.0, lambda_end=60.0, max_step=1.0)
    mesh = f.Mesh(ctx, V, F)
    r = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, cam)
    # from within, on the first step: the start guess h0 of a unit direction is of the order 0.01 .. 0.1 here
    assert np.all(r["tri"] >= 0) and np.all(r["flags"] == 0x88) and r["n_accepted"].max() <= 4
    dist = np.linalg.norm(r["end"][:, :3] - (cam + [0.01, -0.02, 0.015]), axis=1)
    assert dist.min() >= mr.inscribed_radius(V, F, cam + [0.01, -0.02, 0.015]) - 1e-12 and dist.max() <= 0.05 + 1e-12
    assert (r["n_accepted"] == 1).sum() > 0
    mesh.close()
    # a zero-area triangle changes nothing and gives no NaN
    Vb, Fb = mr.golden_meshes()["behind"]
    g = load_golden("mesh")
    pg = f.make_params(r_exit=40.0, **mr.GOLDEN_PAR)
    clean = f.Mesh(ctx, Vb, Fb)
    want = mc.trace_mesh_device(ctx, pg, clean, 0.25, g["behind_k0"], g["x0"])
    clean.close()
    Fz = np.concatenate([Fb, [[Fb[3, 0], Fb[3, 0], Fb[3, 1]], [Fb[7, 2], Fb[7, 2], Fb[7, 2]]]]).astype(np.int32)
    for leaf in (1, 4):
        dirty = f.Mesh(ctx, Vb, Fz, leaf_size=leaf)
        got = mc.trace_mesh_device(ctx, pg, dirty, 0.25, g["behind_k0"], g["x0"])
        dirty.close()
        assert _same(got, want) and not np.isnan(got["end"]).any()


def test_the_substep_cap_and_the_host_call_and_the_refusals(ctx):
    f = _ffi()
    g = load_golden("mesh")
    V, F = mr.golden_meshes()["front"]
    k0 = g["front_k0"]
    p = f.make_params(r_exit=40.0, **mr.GOLDEN_PAR)
    mesh = f.Mesh(ctx, V, F)
    base = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, g["x0"])
    # max_chord so small that the cap of 1024 binds on every step longer than 1e-3: the hits stay, to the chord's sag
    tiny = mc.trace_mesh_device(ctx, p, mesh, 1e-6, k0, g["x0"])
    both = (base["tri"] >= 0) & (tiny["tri"] >= 0)
    assert both.sum() >= 20 and (base["flags"] != tiny["flags"]).sum() <= 0.02 * len(k0)
    assert np.array_equal(base["n_accepted"][both], tiny["n_accepted"][both])
    assert np.abs(base["end"] - tiny["end"])[both].max() < 5e-3
    # the host-buffer call returns the device call's bits (NaN where the device call leaves its slot untouched)
    h = ctx.trace_mesh(k0, g["x0"], p, mesh, 0.25)
    for a, k in zip(h[:5], ("end", "flags", "n_steps", "n_accepted", "tri")):
        assert np.array_equal(a, base[k]), k
    hit = base["tri"] >= 0
    assert np.array_equal(h[5][hit], base["bary"][hit]) and np.isnan(h[5][~hit]).all()
    # refusals leave sentinel-filled outputs untouched
    import torch
    n = 64
    d = {k: torch.full(s, v, dtype=t, device="cuda") for k, (s, v, t) in dict(
        end=((n, 6), SENTINEL, torch.float64), fl=((n,), 255, torch.uint8), tri=((n,), -9, torch.int32),
        bary=((n, 2), SENTINEL, torch.float64), k0=((n, 3), 0.5, torch.float64)).items()}

    def call(p, m=mesh, chord=0.25, tri=None, bary=None):
        ctx.trace_mesh_device(p, m, chord, n, d["k0"].data_ptr(), d["end"].data_ptr(), d["tri"].data_ptr() if tri is None else tri,
                              d["bary"].data_ptr() if bary is None else bary, x0_shared=g["x0"], d_flags=d["fl"].data_ptr())

    for kw in (dict(p=f.make_params(method=f.METHOD_RK4)), dict(p=f.make_params(time_like=1)), dict(p=p, m=None),
               dict(p=p, chord=0.0), dict(p=p, chord=-1.0), dict(p=p, chord=np.inf), dict(p=p, chord=np.nan), dict(p=p, tri=0),
               dict(p=p, bary=0)):
        with pytest.raises(f.BhgError):
            call(**kw)
    sc = f.make_scene(64, 8, 4, spheres=[[0.0, 4.0, 0.0, 1.0]])
    with pytest.raises(f.BhgError):
        ctx.shade_mesh_device(d["end"].data_ptr(), d["fl"].data_ptr(), d["tri"].data_ptr(), d["bary"].data_ptr(), 64, 1, sc, mesh,
                              d_rgba=d["end"].data_ptr())
    torch.cuda.synchronize()
    assert (d["end"] == SENTINEL).all() and (d["fl"] == 255).all() and (d["bary"] == SENTINEL).all() and (d["tri"] == -9).all()
    # (a mesh of another context of the SAME device is accepted: the refusal is about the device)
    other = f.Context(0)
    foreign = f.Mesh(other, V, F)
    call(p=p, m=foreign)
    torch.cuda.synchronize()
    assert (d["tri"] != -9).all()
    foreign.close()
    other.close()
    mesh.close()
    # a mesh closes with its context, and closing twice is harmless
    c2 = f.Context(0)
    m2 = f.Mesh(c2, V, F)
    c2.close()
    assert m2._h is None
    m2.close()


def test_integrator_trace_with_a_mesh(ctx):
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    f = _ffi()
    g = load_golden("mesh")
    V, F = mr.golden_meshes()["front"]
    gi = GeodesicIntegratorSchwarzschild(mass=0.5, verbose=False, device=0)
    out = gi.trace(g["front_k0"].reshape(4, -1, 3), g["x0"], curve_end=80.0, r_exit=40.0, mesh=(V, F))
    mesh = f.Mesh(ctx, V, F)
    want = mc.trace_mesh_device(ctx, f.make_params(r_exit=40.0, **mr.GOLDEN_PAR), mesh, 0.25, g["front_k0"], g["x0"])
    mesh.close()
    assert out["tri_id"].shape == (4, len(V) and g["front_k0"].shape[0] // 4) and out["bary"].shape[-1] == 2
    assert np.array_equal(out["tri_id"].ravel(), want["tri"]) and np.array_equal(out["ray_end"].reshape(-1, 6), want["end"])
    assert np.array_equal(out["flags"].ravel(), want["flags"])
    with pytest.raises(ValueError):
        gi.trace(g["front_k0"], g["x0"], mesh=(V, F), spheres=[[0, 4, 0, 1]])


# ---- 7. the shade ----------------------------------------------------------------------------------------------------------
SHADE_CAM = np.array([16.0, -3.0, 5.0])
# two components placed so that the tetrahedron stands between the first lamp and the sphere
SHADE_MESH = mr.join(mr.octa_sphere((-2.5, 2.0, 0.8), 1.3, 2), mr.tetrahedron((-0.4, 4.6, 1.9), 0.8))
SHADE_LAMPS = [[4.0, 10.0, 4.0, 9.0], [12.0, -9.0, 7.0, 7.0]]
SHADE_DISK = (2.0, 7.0)
SHADE_AIM = np.array([-1.2, 2.6, 1.1])


def _shade_frame(ctx, S, mesh=None, tri_rgb=None):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    look = (SHADE_AIM - SHADE_CAM) / np.linalg.norm(SHADE_AIM - SHADE_CAM)
    # (rotation_euler: the camera looks down its own -z; aim that between the hole and the mesh)
    rx = np.arccos(-look[2])
    rz = np.arctan2(-look[0], look[1])
    fr = DeviceFrame(ctx, 32, 32, S, fov_x=0.5, fov_y=0.5, origin=SHADE_CAM, rotation_euler=(rx, 0.0, rz))
    fr.set_sky(synthetic_sky(128, 64))
    fr.set_disk(*SHADE_DISK)
    fr.set_objects([], lamps=SHADE_LAMPS)
    if mesh is not None:
        fr.set_mesh(mesh, tri_rgb=tri_rgb, chord=0.2)
    return fr


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("smooth", [False, True], ids=["flat", "vertex_normals"])
def test_shade(ctx, S, smooth):
    import torch
    f = _ffi()
    V, F = SHADE_MESH
    normals = None
    if smooth:
        nt_sphere = 8 * 4 ** 2
        centres = np.where((np.arange(len(V)) < V.shape[0] - 4)[:, None], np.array([-2.5, 2.0, 0.8]), np.array([-0.4, 4.6, 1.9]))
        normals = V - centres
        normals /= np.linalg.norm(normals, axis=1)[:, None]
        assert nt_sphere + 4 == len(F)
    rgb = np.random.default_rng(3).uniform(0.2, 1.0, (len(F), 3)).astype(np.float32)
    mesh = f.Mesh(ctx, V, F, vertex_normals=normals)
    p = f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=SHADE_DISK[0], disk_r_out=SHADE_DISK[1])
    fr = _shade_frame(ctx, S, mesh, rgb)
    got = fr.render(p).cpu().numpy().copy()
    out32 = torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out32)
    torch.cuda.synchronize()
    end, flags, tri, bary = (t.cpu().numpy() for t in (fr.d_end, fr.d_flags, fr.d_tri_id, fr.d_bary))
    on_mesh = (flags == 0x88) & (tri >= 0)
    assert on_mesh.sum() > 60 * S and (flags == 128).sum() > 20 and (flags == 8).sum() > 50 and len({*tri[on_mesh]}) > 10
    assert (tri[on_mesh] >= len(F) - 4).any() and (tri[on_mesh] < len(F) - 4).any()      # both components are seen
    # the restatement: the mesh colour in numpy on the device's own records; every other ray's colour is the plain shade's (one
    # sample per "pixel", so that each ray's colour comes back by itself), summed per pixel in sample order
    per_ray = torch.empty((fr.n, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.n, 1, fr.scene(), per_ray.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    col = per_ray.cpu().numpy()[:, :3].copy()
    margins = []
    tree = f.mesh_bvh_host(V, F, 4)
    col[on_mesh] = mr.mesh_colour(end[on_mesh], tri[on_mesh], bary[on_mesh], V, F, SHADE_LAMPS, rgb, normals, tree=tree, margins=margins)
    brute = mr.mesh_colour(end[on_mesh], tri[on_mesh], bary[on_mesh], V, F, SHADE_LAMPS, rgb, normals)
    assert np.array_equal(col[on_mesh], brute)                        # the restatement's own two traversals agree
    want = np.zeros((fr.P, 3))
    for s in range(S):
        want += col[s * fr.P:(s + 1) * fr.P]
    want /= S
    # a shadow decision within 1e-9 of an edge exempts its ray: the lamps are chosen so that there is none
    near = int((np.array(margins) < 1e-9).sum())
    print(f"S {S}, {'vertex' if smooth else 'flat'} normals: {int(on_mesh.sum())} mesh rays, {len(margins)} shadow decisions, smallest "
          f"margin {min(margins):.2e}, {near} within 1e-9; lit {int((col[on_mesh].sum(1) > 0).sum())}, dark "
          f"{int((col[on_mesh].sum(1) == 0).sum())}")
    assert near == 0 and near <= 0.005 * on_mesh.sum()
    unshadowed = mr.mesh_colour(end[on_mesh], tri[on_mesh], bary[on_mesh], V, F, SHADE_LAMPS, rgb, normals, shadows=False)
    assert (col[on_mesh].sum(1) > 0).sum() > 20 and (col[on_mesh].sum(1) < unshadowed.sum(1)).sum() > 10
    err = np.abs(got[:, :3] - want)
    print(f"worst |gpu - numpy| {err.max():.3e}")
    assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(want))) and np.all(got[:, 3] == 1.0)
    assert np.array_equal(out32.cpu().numpy(), got.astype(np.float32))
    # pixels with no mesh ray are the existing shade()'s bits: bhg_shade_scene_device on the same records
    same_records = torch.empty((fr.P, 4), dtype=torch.float64, device=fr.dev)
    ctx.shade_scene_device(fr.d_end.data_ptr(), fr.d_flags.data_ptr(), fr.P, S, fr.scene(), same_records.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_records = same_records.cpu().numpy()
    pix_mesh = on_mesh.reshape(S, fr.P).any(0)
    assert pix_mesh.sum() > 30 and (~pix_mesh).sum() > 500
    assert np.array_equal(got[~pix_mesh], same_records[~pix_mesh]) and not np.array_equal(got[pix_mesh], same_records[pix_mesh])
    # with the mesh off the frame is the plain one: those pixels within what the disk bound of the trace moves a colour by (the
    # mesh trace's end states with a disk set are the opaque-disk trace's within 1e-10)
    fr.set_mesh(None)
    plain = fr.render(p).cpu().numpy().copy()
    assert np.abs(got[~pix_mesh] - plain[~pix_mesh]).max() < 1e-6
    # ... and set_mesh(None) after a mesh frame is the frame that never had one, bit for bit
    never = _shade_frame(ctx, S)
    assert np.array_equal(never.render(p).cpu().numpy(), plain)
    assert np.array_equal(never.d_end.cpu().numpy(), fr.d_end.cpu().numpy()) and np.array_equal(never.d_steps.cpu().numpy(), fr.d_steps.cpu().numpy())
    mesh.close()


def test_shade_shadows_and_refused_combinations(ctx):
    f = _ffi()
    V, F = SHADE_MESH
    mesh = f.Mesh(ctx, V, F)
    p = f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=SHADE_DISK[0], disk_r_out=SHADE_DISK[1])
    fr = _shade_frame(ctx, 1, mesh)
    fr.render(p)
    end, flags, tri, bary = (t.cpu().numpy() for t in (fr.d_end, fr.d_flags, fr.d_tri_id, fr.d_bary))
    on_mesh = (flags == 0x88) & (tri >= 0)
    # one component shadows the other: rays on the sphere whose segment to the first lamp meets the tetrahedron
    tris = mr.tri_arrays(V, F)
    lamp = np.array(SHADE_LAMPS[0][:3])
    shadowed_by_other = 0
    for i in np.flatnonzero(on_mesh & (tri < len(F) - 4)):
        x = end[i, :3]
        ld = (lamp - x) / np.linalg.norm(lamp - x)
        h = mr.segment_brute(x + 1e-5 * ld, lamp, tris)
        shadowed_by_other += h is not None and h[1] >= len(F) - 4
    assert shadowed_by_other >= 3
    for setter, args in (("set_objects", ([[0.0, 4.0, 0.0, 1.0]],)), ("set_disk_layers", (2,)), ("set_redshift", ()),
                         ("set_polarisation", (0.1,)), ("set_disk_thermal", (1e7, *f.narrowband(1e17, 2e17, 3e17)))):
        # set after the mesh: the trace refuses; set before it: set_mesh refuses
        bad = _shade_frame(ctx, 1, mesh)
        getattr(bad, setter)(*args)
        bad.generate_rays()
        with pytest.raises(ValueError, match="a mesh does not go with"):
            bad.trace(p)
        with pytest.raises(ValueError, match="a mesh does not go with"):
            _set_mesh_after(ctx, setter, args, mesh)
    with pytest.raises(ValueError):
        fr.shade_stokes()
    # the scene changed after the trace: shade() says so
    fr.set_mesh(None)
    with pytest.raises(RuntimeError):
        fr.shade()
    mesh.close()


def _set_mesh_after(ctx, setter, args, mesh):
    fr = _shade_frame(ctx, 1)
    getattr(fr, setter)(*args)
    fr.set_mesh(mesh)

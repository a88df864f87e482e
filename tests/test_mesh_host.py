"""Triangle meshes without a GPU: the ABI surface, the refusals (checked before the context, so the library
refuses them here too), the host-side BVH builder (bhg_mesh_bvh_host) -- its invariants and, through the numpy restatement of the
skip-link traversal, the brute-force answer on seeded segments, ties included --, the scipy restatement of the hit rule
(tests/mesh_reference.py) against known answers, and the conditions the golden vectors must keep.

Measured when this was written: the numpy traversal gave the brute-force (s, triangle) on every one of 10 x 3 x 10 000 segments,
between 599 (tetrahedron) and 3 361 (octahedron) of them with tied triangles.  The golden: 29 to 45 triangle hits per set of 160
rays, no ray unstable under the three perturbations; the recorded |refined point - chord hit| up to 1.1e-2 (the sphere behind the
hole, a grazing ray) with M up to 201; max_chord 0.03 against 0.25 chose the same triangle and step on every hit ray and moved
the hit by 7.6e-15 at the most."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mesh_reference as mr  # noqa: E402


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


# ---- the ABI surface ----------------------------------------------------------------------------------------------------
NEW = ("bhg_mesh_create", "bhg_mesh_destroy", "bhg_mesh_info", "bhg_mesh_bvh_host", "bhg_trace_mesh_device", "bhg_trace_mesh",
       "bhg_shade_mesh_device")


def test_exports_and_header():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_MESH\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+BHG_MESH_MAX_SUBSTEPS\s+1024\s*$", hdr, re.M)
    assert f.MESH_MAX_SUBSTEPS == 1024 == mr.MAX_SUBSTEPS
    assert L.bhg_version() == 10 and f.ABI_VERSION == 10
    for name in ("Mesh", "mesh_bvh_host"):
        assert hasattr(f, name)
    for name in ("trace_mesh", "trace_mesh_device", "shade_mesh_device"):
        assert hasattr(f.Context, name)


# ---- the refusals, through a NULL context -----------------------------------------------------------------------------------
def _trace_rc(p, mesh=None, chord=0.25, tri=64, bary=64):
    f, L = _lib()
    xs = (C.c_double * 3)(20.0, 0.0, 2.0)
    return L.bhg_trace_mesh_device(None, C.byref(p), mesh, chord, xs, None, 64, 16, 64, None, None, None, tri, bary, None)


def test_trace_refusals_come_before_the_context():
    f, L = _lib()
    rc = _trace_rc(f.make_params(method=f.METHOD_RK4))
    assert rc == f.E_INVALID and b"DP5(4)" in L.bhg_last_error()
    rc = _trace_rc(f.make_params(time_like=1))
    assert rc == f.E_INVALID and b"time_like" in L.bhg_last_error()
    rc = _trace_rc(f.make_params())
    assert rc == f.E_INVALID and b"mesh is NULL" in L.bhg_last_error()
    # the host-buffer call has the same order
    p = f.make_params(method=f.METHOD_RK4)
    rc = L.bhg_trace_mesh(None, C.byref(p), None, 0.25, 64, 1, 64, 16, 64, None, None, None, 64, 64)
    assert rc == f.E_INVALID and b"DP5(4)" in L.bhg_last_error()
    p = f.make_params()
    rc = L.bhg_trace_mesh(None, C.byref(p), None, 0.25, 64, 1, 64, 16, 64, None, None, None, 64, 64)
    assert rc == f.E_INVALID and b"mesh is NULL" in L.bhg_last_error()


def test_shade_refusals_come_before_the_context():
    f, L = _lib()
    sc = f.make_scene(64, 8, 4, spheres=[[0.0, 4.0, 0.0, 1.0]])
    rc = L.bhg_shade_mesh_device(None, 64, 64, 64, 64, 16, 1, C.byref(sc), None, None, 64, None, None, None)
    assert rc == f.E_INVALID and b"n_spheres must be 0" in L.bhg_last_error()
    sc = f.make_scene(64, 8, 4)
    rc = L.bhg_shade_mesh_device(None, 64, 64, 64, 64, 16, 1, C.byref(sc), None, None, 64, None, None, None)
    assert rc == f.E_INVALID and b"mesh is NULL" in L.bhg_last_error()
    assert L.bhg_mesh_info(None, None, None, None) == f.E_INVALID
    L.bhg_mesh_destroy(None)       # a no-op


def test_integrator_refuses_the_combinations():
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild.__new__(GeodesicIntegratorSchwarzschild)     # (no context: the checks come first)
    V, F = mr.tetrahedron((0, 5, 0), 1.0)
    k0, x0 = np.array([[0.0, 1.0, 0.0]]), np.array([0.0, -10.0, 0.0])
    for kw in (dict(spheres=[[0, 4, 0, 1]]), dict(disk_crossings=2, disk=(3, 12)), dict(travel_time=True), dict(redshift={}),
               dict(polarisation=dict(degree=0.1)), dict(disk_thermal=dict(t_peak=1e7))):
        with pytest.raises(ValueError, match="mesh does not go with"):
            gi.trace(k0, x0, mesh=(V, F), **kw)


# ---- the builder ------------------------------------------------------------------------------------------------------------
def _meshes():
    rng = np.random.default_rng(11)
    out = {"tetrahedron": mr.tetrahedron((0.3, -0.2, 0.1), 1.0)}
    for sub in range(4):
        out[f"sphere{sub}"] = mr.octa_sphere((0.0, 0.0, 0.0), 1.0, sub)
    out["random2048"] = mr.random_triangles(2048, rng)
    V, F = mr.tetrahedron((1.0, 2.0, 3.0), 0.5)
    out["identical64"] = (V, np.tile(F[:1], (64, 1)))
    V, F = mr.octa_sphere((0.5, 0.0, 0.0), 1.0, 1)
    out["zero_area"] = (V, np.concatenate([F[:10], [[F[3, 0], F[3, 0], F[3, 1]]], F[10:]]).astype(np.int32))
    out["two_components"] = mr.join(mr.octa_sphere((-2.0, 0.0, 0.0), 1.0, 1), mr.tetrahedron((2.5, 0.5, 0.0), 0.8))
    return out


MESHES = _meshes()


def _leaf_sizes(nt):
    return sorted({1, 4, nt})


@pytest.mark.parametrize("name", sorted(MESHES))
def test_tree_invariants(name):
    f, _ = _lib()
    V, F = MESHES[name]
    nt = len(F)
    assert {len(mr.octa_sphere((0, 0, 0), 1.0, s)[1]) for s in range(4)} == {8, 32, 128, 512}
    for leaf in _leaf_sizes(nt):
        t = f.mesh_bvh_host(V, F, leaf)
        nn = len(t["skip"])
        assert 1 <= nn <= 2 * nt - 1 or nt == 1
        # every triangle is in exactly one leaf
        assert sorted(t["order"].tolist()) == list(range(nt))
        leaves = t["count"] > 0
        assert np.all(t["first"][~leaves] == -1) and np.all(t["count"][~leaves] == 0)
        spans = sorted((int(a), int(a + c)) for a, c in zip(t["first"][leaves], t["count"][leaves]))
        assert spans[0][0] == 0 and spans[-1][1] == nt and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        # skip is strictly increasing along the walk and consistent with the depth-first order: the subtree of node i is
        # i + 1 .. skip[i] - 1, an inner node's children are i + 1 and skip[i + 1], and the right one ends where the parent does
        assert np.all(t["skip"] > np.arange(nn)) and t["skip"][0] == nn and np.all(t["skip"] <= nn)
        depth = np.zeros(nn, int)
        for i in range(nn):
            if leaves[i]:
                assert t["skip"][i] == i + 1
                lo, hi = int(t["first"][i]), int(t["first"][i] + t["count"][i])
                pts = V[F[t["order"][lo:hi]]].reshape(-1, 3)
                assert np.all(pts >= t["box"][i, :3]) and np.all(pts <= t["box"][i, 3:])
                # over leaf_size only when a split separates nothing: all centroids of the leaf coincide
                if hi - lo > leaf:
                    cen = V[F[t["order"][lo:hi]]].sum(1) / 3.0
                    assert np.all(cen == cen[0])
                continue
            left, right = i + 1, int(t["skip"][i + 1])
            assert right < t["skip"][i] and t["skip"][right] == t["skip"][i]
            for c in (left, right):
                depth[c] = depth[i] + 1
                assert np.all(t["box"][c, :3] >= t["box"][i, :3]) and np.all(t["box"][c, 3:] <= t["box"][i, 3:])
        # the depth bound of a median split by count
        assert depth.max() <= int(np.ceil(np.log2(max(nt, 2)))) + 1
        if leaf >= nt or name == "identical64":
            assert nn == 1
        # the tree is a function of the mesh alone
        t2 = f.mesh_bvh_host(V, F, leaf)
        assert all(np.array_equal(t[k], t2[k]) for k in t)


def _segments(V, F, rng, n):
    """Seeded segments about the mesh: random ones, short ones (sub-chord sized), and -- the ties -- segments that run along
    shared edges, through shared vertices, and end exactly on vertices."""
    lo, hi = V.min(0) - 0.5, V.max(0) + 0.5
    p = rng.uniform(lo, hi, (n, 3))
    q = rng.uniform(lo, hi, (n, 3))
    short = slice(n // 4, n // 2)
    q[short] = p[short] + rng.normal(size=(n // 2 - n // 4, 3)) * 0.2
    k = n // 8
    a, b = V[F[rng.integers(0, len(F), k), 0]], V[F[rng.integers(0, len(F), k), 1]]
    # through a vertex: from a random point to its mirror image in the vertex (the vertex at s = 1/2 exactly)
    p[-k:] = rng.uniform(lo, hi, (k, 3))
    q[-k:] = 2.0 * a - p[-k:]
    # ending on a vertex
    q[-2 * k:-k] = b
    # along an edge of a triangle, extended beyond both ends, and exactly the edge
    t = rng.integers(0, len(F), k)
    e0, e1 = V[F[t, 0]], V[F[t, 1]]
    p[-3 * k:-2 * k], q[-3 * k:-2 * k] = e0 - 0.5 * (e1 - e0), e1 + 0.5 * (e1 - e0)
    p[-4 * k:-3 * k], q[-4 * k:-3 * k] = e0, e1
    return p, q


@pytest.mark.parametrize("name", sorted(MESHES))
def test_traversal_gives_the_brute_force_answer(name):
    """The numpy traversal of the returned tree against the brute force over all triangles: the same (s, triangle) on 10 000
    seeded segments per mesh, identically, for leaf sizes 1, 4 and nt.  On the octahedron (sphere0) the edge and vertex segments
    lie in coordinate planes and through integer points: exact ties between up to four triangles."""
    f, _ = _lib()
    V, F = MESHES[name]
    tris = mr.tri_arrays(V, F)
    p, q = _segments(V, F, np.random.default_rng(101), 10000)
    brute = [mr.segment_brute(p[i], q[i], tris) for i in range(len(p))]
    n_hit = sum(b is not None for b in brute)
    ties = 0
    for i, b in enumerate(brute):
        if b is not None:
            hit, s, _, _ = mr.moller_trumbore(p[i], q[i] - p[i], *tris)
            ties += int((s[hit] == b[0]).sum() > 1)
    print(f"{name}: {n_hit} of {len(p)} segments hit, {ties} with tied triangles")
    assert n_hit > 500
    if name.startswith("sphere") or name == "identical64":
        assert ties > 50
    for leaf in _leaf_sizes(len(F)):
        tree = f.mesh_bvh_host(V, F, leaf)
        tested = []
        for i in range(len(p)):
            assert mr.segment_tree(p[i], q[i], tree, tris, count=tested) == brute[i], (leaf, i)
        if leaf == 4 and len(F) >= 512:
            # the tree does accelerate: a twentieth of the brute force's triangle tests at the most
            assert np.mean(tested) < len(F) / 20


def test_zero_area_triangle_is_never_hit():
    V, F = MESHES["zero_area"]
    tris = mr.tri_arrays(V, F)
    p, q = _segments(V, F, np.random.default_rng(5), 4000)
    for i in range(len(p)):
        b = mr.segment_brute(p[i], q[i], tris)
        assert b is None or (b[1] != 10 and np.isfinite(b[0]))


def test_builder_refusals():
    f, L = _lib()
    V, F = mr.tetrahedron((0, 0, 0), 1.0)
    nn = C.c_size_t(0)
    box = np.empty((16, 6))
    i32 = [np.empty(16, np.int32) for _ in range(4)]

    def rc(V, nv, F, nt, leaf, cap=16):
        return L.bhg_mesh_bvh_host(V.ctypes.data, nv, F.ctypes.data, nt, leaf, box.ctypes.data, *(a.ctypes.data for a in i32), cap,
                                   C.byref(nn))

    assert rc(V, 4, F, 4, 4) == f.OK and nn.value == 1
    for args, word in (((V, 4, F, 0, 4), b"> 0"), ((V, 0, F, 4, 4), b"> 0"), ((V, 4, F, 4, 0), b"leaf_size"),
                       ((V, 4, F, 4, -3), b"leaf_size"), ((V, 2**31, F, 4, 4), b"2^31"), ((V, 4, F, 2**31, 4), b"2^31")):
        assert rc(*args) == f.E_INVALID and word in L.bhg_last_error(), (args[1:], L.bhg_last_error())
    for bad in (4, -1):
        G = F.copy()
        G[2, 1] = bad
        assert rc(V, 4, G, 4, 4) == f.E_INVALID and b"outside" in L.bhg_last_error()
    for bad in (np.nan, np.inf):
        W = V.copy()
        W[3, 2] = bad
        assert rc(W, 4, F, 4, 4) == f.E_INVALID and b"finite" in L.bhg_last_error()
    # too small a node array is said, with the count
    assert rc(V, 4, F, 4, 1, cap=3) == f.E_INVALID and nn.value == 7
    # bhg_mesh_create refuses the same meshes before it looks at the context
    h = C.c_void_p(5)
    W = V.copy()
    W[0, 0] = np.nan
    assert L.bhg_mesh_create(None, W.ctypes.data, 4, F.ctypes.data, 4, None, 4, C.byref(h)) == f.E_INVALID
    assert b"finite" in L.bhg_last_error() and not h.value
    assert L.bhg_mesh_create(None, V.ctypes.data, 4, F.ctypes.data, 4, None, 0, C.byref(h)) == f.E_INVALID
    assert b"leaf_size" in L.bhg_last_error()
    assert L.bhg_mesh_create(None, V.ctypes.data, 4, F.ctypes.data, 4, None, 4, C.byref(h)) == f.E_INVALID
    assert b"ctx is NULL" in L.bhg_last_error()
    with pytest.raises(ValueError):
        f.mesh_bvh_host(V[:, :2], F)


# ---- the restatement against known answers ------------------------------------------------------------------------------
def test_flat_space_hit_is_the_straight_line_intersection():
    """r_s -> 1e-12: the curve is the straight line x0 + lambda k0, and the refined hit its intersection with the triangle."""
    V = np.array([[3.0, -2.0, -1.5], [3.5, 2.5, -1.0], [2.5, 0.3, 2.2]])
    F = np.array([[0, 1, 2]], np.int32)
    rng = np.random.default_rng(2)
    x0 = np.array([-6.0, 0.2, 0.1])
    n_hit = 0
    for rhs in (0, 1):
        for _ in range(12):
            u, v = rng.uniform(0.05, 0.45, 2)
            target = V[0] + u * (V[1] - V[0]) + v * (V[2] - V[0])
            k0 = (target - x0) / np.linalg.norm(target - x0)
            r = mr.solve(k0, x0, rhs, V, F, 0.25, r_s=1e-12, lambda_end=30.0, rtol=1e-6, atol=1e-9)
            assert r["flags"] == mr.FLAG_HIT_OBJECT and r["tri"] == 0
            assert np.abs(r["end"][:3] - target).max() < 1e-12 and np.abs(r["end"][3:] - k0).max() < 1e-12
            assert np.abs(r["bary"] - [u, v]).max() < 1e-12
            n_hit += 1
        # a ray past the triangle
        miss = mr.solve(np.array([1.0, 0.9, 0.0]) / np.hypot(1.0, 0.9), x0, rhs, V, F, 0.25, r_s=1e-12, lambda_end=30.0)
        assert miss["tri"] == -1 and miss["flags"] == mr.FLAG_REACHED_END and np.isnan(miss["bary"]).all()
    assert n_hit == 24


def test_terminal_events_win_when_they_come_first():
    """A triangle behind the exit sphere is never reached; one behind the opaque disk loses to the disk; in front, it wins."""
    x0 = np.array([0.0, -15.0, 6.0])
    k0 = np.array([0.0, 1.0, -0.6]) / np.hypot(1.0, 0.6)          # crosses z = 0 near y = -5, inside the annulus
    wall = lambda y: (np.array([[-3.0, y, -8.0], [3.0, y, -8.0], [0.0, y, 9.0]]), np.array([[0, 1, 2]], np.int32))   # noqa: E731
    par = dict(r_s=0.2, lambda_end=60.0, r_exit=25.0)
    free = mr.solve(k0, x0, 0, *wall(100.0), 0.25, **par)
    assert free["flags"] == mr.FLAG_EXITED and free["tri"] == -1
    disk = mr.solve(k0, x0, 0, *wall(100.0), 0.25, disk=(0.5, 20.0), **par)
    assert disk["flags"] == mr.FLAG_HIT_DISK
    y_disk = disk["end"][1]
    behind = mr.solve(k0, x0, 0, *wall(y_disk + 2.0), 0.25, disk=(0.5, 20.0), **par)
    assert behind["flags"] == mr.FLAG_HIT_DISK and behind["tri"] == -1 and np.array_equal(behind["end"], disk["end"])
    front = mr.solve(k0, x0, 0, *wall(y_disk - 2.0), 0.25, disk=(0.5, 20.0), **par)
    assert front["flags"] == mr.FLAG_HIT_OBJECT and front["tri"] == 0 and abs(front["end"][1] - (y_disk - 2.0)) < 1e-12
    assert front["n_accepted"] <= disk["n_accepted"]


# ---- the golden vectors ------------------------------------------------------------------------------------------------------
def test_golden_conditions():
    """What tests/test_gpu_mesh.py relies on: every set has triangle hits (the sphere behind the hole: secondary images, rays
    that pass the hole first), at most 1 % of a set is unstable, and -- max_chord 0.25 against 0.03 -- the accepted-step count of
    a hit never changes and the hit moves by less than the chord's sag allows.
    The bound: both refined points lie on the same curve, each within its own chord's sag of a chord hit on the mesh; the issue
    measured the sag at max_chord 0.25 as 2.1e-3 at the most (median 5.7e-4) and the fixture records each ray's own.  A ray
    whose two chord lengths chose the same triangle has the same plane root (bound: 1e-9, Brent's tolerance times the speed);
    one near an edge may choose the neighbour, and then moves along the curve by the sag over the sine of the angle between the
    curve and the mesh: 20 x its own recorded sag + 1e-9 is the bound taken (an incidence down to 3 degrees)."""
    g = load_golden("mesh")
    assert float(g["max_chord"]) == mr.GOLDEN_CHORD and float(g["fine_chord"]) == 0.03
    assert np.array_equal(g["forms"], np.array(mr.GOLDEN_FORMS))
    meshes = mr.golden_meshes()
    for name in g["mesh_names"]:
        V, F = meshes[str(name)]
        assert np.array_equal(g[f"{name}_V"], V) and np.array_equal(g[f"{name}_F"], F)
        for fi in range(len(mr.GOLDEN_FORMS)):
            tri, stable, sag = g[f"{name}_tri"][fi], g[f"{name}_stable"][fi], g[f"{name}_sag"][fi]
            hits = tri >= 0
            n = len(tri)
            assert hits.sum() >= 12, (name, fi, int(hits.sum()))
            assert (~stable).sum() <= 0.01 * n
            assert np.all((g[f"{name}_flags"][fi] == mr.FLAG_HIT_OBJECT) == hits)
            assert np.all(np.isnan(g[f"{name}_bary"][fi][~hits])) and np.all(np.isfinite(g[f"{name}_bary"][fi][hits]))
            fine_hits = g[f"{name}_tri_fine"][fi] >= 0
            both = hits & fine_hits
            move = np.abs(g[f"{name}_end"][fi][:, :3] - g[f"{name}_end_fine"][fi][:, :3]).max(1)
            same = both & (tri == g[f"{name}_tri_fine"][fi])
            print(f"{name} {mr.GOLDEN_FORM_IDS[fi]}: {int(hits.sum())} hits, {int((~stable).sum())} unstable, max sag "
                  f"{sag[hits].max():.2e}, max M {g[f'{name}_M'][fi].max()}, hit at one chord only {int((hits != fine_hits).sum())}, "
                  f"another triangle {int((both & ~same).sum())}, worst move {move[both].max():.2e} "
                  f"(same triangle {move[same].max():.2e})")
            assert np.all(g[f"{name}_n_accepted"][fi][both] == g[f"{name}_n_accepted_fine"][fi][both])
            assert np.all(move[same] <= 1e-9)
            assert np.all(move[both] <= 20.0 * sag[both] + 1e-9)
            # a hit that only one chord length finds grazes the mesh: within the sag of an edge
            assert (hits != fine_hits).sum() <= 0.02 * n
    # the sphere behind the hole is seen past the hole: its hit rays were bent
    behind = g["behind_tri"][0] >= 0
    k0 = g["behind_k0"][behind]
    end = g["behind_end"][0][behind]
    cosang = np.einsum("ij,ij->i", k0, end[:, 3:] / np.linalg.norm(end[:, 3:], axis=1)[:, None])
    assert np.degrees(np.arccos(cosang)).max() > 20.0


def test_golden_is_what_the_restatement_gives():
    """A few rays of every set, solved again: the fixture is this file's restatement, bit for bit."""
    g = load_golden("mesh")
    meshes = mr.golden_meshes()
    for name in g["mesh_names"]:
        V, F = meshes[str(name)]
        for fi, (rhs, a) in enumerate(mr.GOLDEN_FORMS):
            hits = np.flatnonzero(g[f"{name}_tri"][fi] >= 0)[:2]
            for i in list(hits) + [0]:
                r = mr.solve(g[f"{name}_k0"][i], g["x0"], rhs, V, F, float(g["max_chord"]), spin=a,
                             r_exit=0.0 if rhs == 2 else float(g["r_exit"]), **mr.GOLDEN_PAR)
                assert r["tri"] == g[f"{name}_tri"][fi][i] and r["flags"] == g[f"{name}_flags"][fi][i]
                assert np.array_equal(r["end"], g[f"{name}_end"][fi][i]) and r["n_accepted"] == g[f"{name}_n_accepted"][fi][i]
                assert np.array_equal(r["bary"], g[f"{name}_bary"][fi][i], equal_nan=True)

"""Instance sets under a tree of boxes (bhg_mesh_instances_create_tree) on the device.

  1. more than 64 placements exist at all: K = 65 creates and traces (the linear constructor still refuses it);
  2. at K <= 64 a tree set is the linear set, bit for bit -- end, flags, n_steps, n_accepted, tri, inst, bary on sentinel-filled
     arrays -- for section 21's cases (the three placements in all four forms, the ring of 64, the bulge), each with leaves of 1,
     2 and 4; one placement under the identity is the plain mesh trace;
  3. beyond 64 (mesh_instance_tree_cases: the swarm of 192, the clump of 96 in Schwarzschild and Kerr, the swarm permuted): against
     the C oracle on the flattened mesh with test_gpu_mesh_instances' own comparison (every stable ray agrees in flag, step counts
     and (instance, triangle), end and bary within mesh_oracle_cases.hit_tolerances); against itself under BHGEO_INSTANCE_TREE=0
     (the linear loop over all K records) and under BHGEO_MESH_CULL=0 (no box looked at), the same bits, each in a child process
     of its own, one at a time; a permutation of the records gives the same bits with inst mapped through it; a duplicated record
     answers the smaller index;
  4. moving: set(T2) is a fresh tree set of T2, tree_info and the mesh's info stay, traces and moves enqueued back to back on two
     streams see each the transforms of their turn at K = 192, and a refit of the mesh has the set refused until it is set again.

tests/test_mesh_instance_tree_host.py asserts the conditions of the cases on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as mc
import mesh_instance_cases as mi
import mesh_instance_tree_cases as mt
import mesh_oracle_cases as mo
from test_gpu_mesh_instances import _hold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = (1, 2, 4)


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _same(a, b, keys=mi.KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _assert_same(a, b, keys=mi.KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _params(case):
    return _ffi().make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"])


# ---- 1. more than 64 ---------------------------------------------------------------------------------------------------------
def test_65_placements_create_and_trace(ctx):
    f = _ffi()
    case = mt.swarm_case()
    T, k0 = case["T"][:65], np.ascontiguousarray(case["k0"][:65 * mt.SWARM_RAYS])
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
            f.MeshInstances(mesh, T)
        inst = f.MeshInstances(mesh, T, tree=True, leaf_size=2)
        assert inst.info()[0] == 65 and inst.tree_info() == (65, 6, 2)      # 33 leaves (32 of 2, one of 1) and 32 inner nodes
        r = mi.trace_instances_device(ctx, _params(case), inst, case["chord"], k0, case["x0"])
        hit = r["inst"] >= 0
        assert hit.sum() >= 80 and r["inst"].max() < 65 and len(np.unique(r["inst"][hit])) >= 30
        assert np.array_equal(hit, r["flags"] == 0x88) and np.all(r["bary"][~hit] == mi.SENTINEL)
        assert f.MeshInstances(mesh, T[:64]).tree_info() == (0, 0, 0)        # a linear set has no tree
        with pytest.raises(f.BhgError, match="leaf_size"):
            f.MeshInstances(mesh, T, tree=True, leaf_size=9)
        # the integrator's switch
        from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
        gi = GeodesicIntegratorSchwarzschild(mass=0.5, time_like=False, verbose=False, device=0, rhs_form="christoffel")
        kw = dict(curve_end=case["par"]["lambda_end"], r_exit=case["par"]["r_exit"], mesh=(case["Vl"], case["Fl"]), mesh_chord=case["chord"])
        out = gi.trace(k0, case["x0"], mesh_instances=T, mesh_instance_tree=True, **kw)
        assert np.array_equal(out["inst_id"], r["inst"]) and np.array_equal(out["tri_id"], r["tri"]) and np.array_equal(out["ray_end"], r["end"])
        with pytest.raises(f.BhgError, match="BHG_MESH_INSTANCES_MAX"):
            gi.trace(k0, case["x0"], mesh_instances=T, **kw)
    finally:
        mesh.close()


# ---- 2. at K <= 64 the tree set is the linear set ----------------------------------------------------------------------------
SMALL = dict(mi.three_placement_cases(), ring=mi.ring_case(), bulge=mi.bulge_case())


@pytest.fixture(scope="module")
def linear_results(ctx):
    """Section 21's cases through their linear sets, once."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0" and os.environ.get("BHGEO_INSTANCE_TREE", "") != "0"
    return {name: mi.run_case(ctx, case) for name, case in SMALL.items()}


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(SMALL))
def test_a_tree_set_is_the_linear_set(ctx, linear_results, name, leaf):
    case, lin = SMALL[name], linear_results[name]
    r = mt.run_case(ctx, case, tree_leaf=leaf)
    _assert_same(r, lin)
    assert (lin["inst"] >= 0).sum() >= 15


def test_one_placement_under_the_identity_is_the_plain_mesh_trace(ctx):
    f = _ffi()
    V, F = mi.flatten(*mi.ellipsoid(), mi.three_placements())
    k0 = mi.three_rays()
    for form in ("christoffel", "kerr_plus"):
        rhs, a = mi.FORMS[form]
        p = f.make_params(rhs_form=rhs, spin=a, r_s=1.0, lambda_end=64.0, r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
        mesh = f.Mesh(ctx, V, F)
        try:
            plain = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, mo.FRAME_CAM)
            got = mi.trace_instances_device(ctx, p, f.MeshInstances(mesh, mi.IDENTITY, tree=True), 0.25, k0, mo.FRAME_CAM)
        finally:
            mesh.close()
        _assert_same(got, plain, ("end", "flags", "n_steps", "n_accepted", "tri", "bary"))
        hit = plain["tri"] >= 0
        assert hit.sum() >= 200 and np.all(got["inst"][hit] == 0) and np.all(got["inst"][~hit] == -1)


# ---- 3. beyond 64 ------------------------------------------------------------------------------------------------------------
BEYOND = mt.beyond_cases()


@pytest.fixture(scope="module")
def beyond_results(ctx):
    """The cases beyond 64 placements as tree sets (leaves of 2, every cull on), once."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0" and os.environ.get("BHGEO_INSTANCE_TREE", "") != "0"
    return {name: mt.run_case(ctx, case) for name, case in BEYOND.items()}


@pytest.mark.parametrize("name", list(BEYOND))
def test_beyond_64_against_the_oracle(oracle, beyond_results, name):
    case, r = BEYOND[name], beyond_results[name]
    o = _hold(oracle, case, r, "tree_" + name)
    assert (~o["stable"]).sum() == 0          # (the oracle alone leaves no ray out on these cases: nothing escapes the comparison)
    seen = np.unique(r["inst"][r["inst"] >= 0])
    assert np.array_equal(seen, np.flatnonzero(mi.hits_per_instance(o, case) > 0))
    if name == "swarm":
        assert len(seen) >= 150 and (seen >= 64).sum() >= 80


def test_the_swarm_permuted_against_the_oracle_and_itself(ctx, oracle, beyond_results):
    case, r = BEYOND["swarm"], beyond_results["swarm"]
    perm = np.random.default_rng(59).permutation(len(case["T"]))       # new position j holds old instance perm[j]
    q = mt.run_case(ctx, case, T=case["T"][perm])
    _assert_same(q, r, ("end", "flags", "n_steps", "n_accepted", "tri", "bary"))
    hit = r["inst"] >= 0
    assert hit.sum() >= 400 and np.array_equal(perm[q["inst"][hit]], r["inst"][hit]) and np.all(q["inst"][~hit] == -1)
    # ... and the permuted set against the oracle on ITS flattening
    pc = mi.instance_case(case["rhs"], case["spin"], case["par"], (case["Vl"], case["Fl"]), case["T"][perm], case["chord"], case["k0"], case["x0"])
    _hold(oracle, pc, q, "tree_swarm_permuted")


@pytest.mark.parametrize("switch", ["BHGEO_INSTANCE_TREE", "BHGEO_MESH_CULL"])
def test_the_tree_and_the_culls_change_nothing(beyond_results, tmp_path, switch):
    """The same cases in a child process with the switch at 0 -- the linear loop over all K records, or no box looked at -- give the
    same bits.  (One GPU process beside this one at a time, under its own time limit.)"""
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, **{switch: "0"})
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_instance_tree_cases.py"), out], check=True, env=env, timeout=300)
    off = np.load(out)
    on = {f"{name}__{k}": beyond_results[name][k] for name in BEYOND for k in mi.KEYS}
    assert sorted(off.files) == sorted(on)
    for key in off.files:
        assert np.array_equal(off[key], on[key], equal_nan=True), key
    assert sum(int((on[k] >= 0).sum()) for k in on if k.endswith("__inst")) >= 900


def test_a_duplicated_record_answers_the_smaller_index(ctx, beyond_results):
    case, r = BEYOND["swarm"], beyond_results["swarm"]
    assert (r["inst"] == 0).sum() >= 1                                   # instance 0 is hit, so its copy would be too
    twice = mt.run_case(ctx, case, T=np.concatenate([case["T"], case["T"][:1]]))       # instance 192 is instance 0 again
    _assert_same(twice, r)
    assert not np.any(twice["inst"] == 192)
    # the copy FIRST: now the old instance 0 (at 1) never answers
    first = mt.run_case(ctx, case, T=np.concatenate([case["T"][:1], case["T"]]))
    _assert_same(first, r, ("end", "flags", "n_steps", "n_accepted", "tri", "bary"))
    hit = r["inst"] >= 0
    assert np.array_equal(first["inst"][hit], np.where(r["inst"][hit] == 0, 0, r["inst"][hit] + 1))
    # 96 identical records: every hit answers instance 0, whatever the tree puts where
    clump, rc = BEYOND["clump_christoffel"], beyond_results["clump_christoffel"]
    most = int(np.bincount(rc["inst"][rc["inst"] >= 0]).argmax())      # (the placement most rays end on: in view from the camera)
    same = mt.run_case(ctx, clump, T=np.tile(clump["T"][most:most + 1], (96, 1)))
    assert (same["inst"] >= 0).sum() >= 5 and np.all(same["inst"][same["inst"] >= 0] == 0)


# ---- 4. moving ---------------------------------------------------------------------------------------------------------------
def _moved(T, k):
    """The swarm's records, every placement shifted along its own direction and turned a little."""
    rng = np.random.default_rng(100 + k)
    T2 = T.copy()
    T2[:, 9:] += 0.2 * k * rng.normal(size=(len(T), 3))
    R = mi.rotation((0.2, 1.0, -0.4), 0.3 * k)
    T2[:, :9] = np.einsum("ij,njk->nik", R, T[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    return T2


def test_set_is_a_fresh_tree_set_and_leaves_mesh_and_tree_alone(ctx, beyond_results):
    f = _ffi()
    case = BEYOND["swarm"]
    p = _params(case)
    T2 = _moved(case["T"], 2)
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        info = mesh.info()
        inst = f.MeshInstances(mesh, case["T"], tree=True, leaf_size=2)
        tree0 = inst.tree_info()
        assert tree0 == (255, 7, 2)          # 64 ranges of 3 at depth 6, each a leaf of 1 and a leaf of 2
        first = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        _assert_same(first, beyond_results["swarm"])
        inst.set(T2)
        moved = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        fresh_set = f.MeshInstances(mesh, T2, tree=True, leaf_size=2)
        fresh = mi.trace_instances_device(ctx, p, fresh_set, case["chord"], case["k0"], case["x0"])
        _assert_same(moved, fresh)
        assert not _same(moved, first) and (moved["inst"] >= 0).sum() >= 100
        assert inst.tree_info() == tree0 and fresh_set.tree_info() == tree0
        n1, box1 = inst.info()
        assert n1 == 192 and np.array_equal(box1, fresh_set.info()[1])
        Vf, _ = mi.flatten(case["Vl"], case["Fl"], T2)
        assert np.all(Vf >= box1[:3]) and np.all(Vf <= box1[3:])
        after = mesh.info()
        assert info[0] == after[0] and info[1] == after[1] and np.array_equal(info[2], after[2])
        inst.set(case["T"])
        _assert_same(mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"]), first)
        # refused, the set left as it was
        with pytest.raises(ValueError):
            inst.set(T2[:64])
        bad = T2.copy()
        bad[100, 0] += 1e-6
        with pytest.raises(f.BhgError, match="R\\^T R"):
            inst.set(bad)
        _assert_same(mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"]), first)
    finally:
        mesh.close()


def test_moving_needs_no_synchronisation(ctx, beyond_results):
    """test_gpu_mesh_instances' pattern at K = 192: traces and set() calls enqueued back to back, the traces on two streams that are
    not the context's, the host never waiting; every trace sees the transforms -- records AND tree -- of its turn."""
    import torch
    f = _ffi()
    case = BEYOND["swarm"]
    p = _params(case)
    n = len(case["k0"])
    Ts = [case["T"]] + [_moved(case["T"], k) for k in range(1, 4)]
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        want = [mi.trace_instances_device(ctx, p, f.MeshInstances(mesh, T, tree=True), case["chord"], case["k0"], case["x0"]) for T in Ts]
        assert _same(want[0], beyond_results["swarm"]) and not any(_same(want[0], w) for w in want[1:])
        inst = f.MeshInstances(mesh, Ts[0], tree=True)
        d_k0 = torch.as_tensor(case["k0"]).cuda()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        outs = []
        order = [0, 1, 2, 3, 0, 2]
        for k, which in enumerate(order):
            if k:
                inst.set(Ts[which])
                if k == 3:                      # (two more moves nobody traces: only the last one counts)
                    inst.set(Ts[1])
                    inst.set(Ts[which])
            st = streams[k % 2]
            with torch.cuda.stream(st):
                o = dict(end=torch.full((n, 6), mi.SENTINEL, dtype=torch.float64, device="cuda"),
                         flags=torch.full((n,), 255, dtype=torch.uint8, device="cuda"),
                         n_steps=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                         n_accepted=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                         tri=torch.full((n,), -9, dtype=torch.int32, device="cuda"),
                         inst=torch.full((n,), -9, dtype=torch.int32, device="cuda"),
                         bary=torch.full((n, 2), mi.SENTINEL, dtype=torch.float64, device="cuda"))
                ctx.trace_mesh_instances_device(p, inst, case["chord"], n, d_k0.data_ptr(), o["end"].data_ptr(), o["tri"].data_ptr(),
                                                o["inst"].data_ptr(), o["bary"].data_ptr(), x0_shared=case["x0"],
                                                d_flags=o["flags"].data_ptr(), d_n_steps=o["n_steps"].data_ptr(),
                                                d_n_accepted=o["n_accepted"].data_ptr(), stream=st.cuda_stream)
            outs.append(o)
        torch.cuda.synchronize()
        for k, (which, o) in enumerate(zip(order, outs)):
            got = {key: t.cpu().numpy() for key, t in o.items()}
            got["n_steps"], got["n_accepted"] = got["n_steps"].astype(np.uint32), got["n_accepted"].astype(np.uint32)
            assert _same(got, want[which]), (k, which)
    finally:
        torch.cuda.synchronize()
        mesh.close()


def test_a_refit_of_the_mesh_has_the_set_refused_until_it_is_set(ctx):
    f = _ffi()
    case = BEYOND["clump_christoffel"]
    p = _params(case)
    V2 = case["Vl"] * np.array([1.3, 0.8, 1.1])
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        inst = f.MeshInstances(mesh, case["T"], tree=True, leaf_size=4)
        before = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        mesh.refit(V2)
        with pytest.raises(f.BhgError, match="has been refitted"):
            mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        inst.set(case["T"])
        after = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        assert inst.tree_info() == (63, 5, 4)          # 32 leaves of 3
    finally:
        mesh.close()
    fresh_mesh = f.Mesh(ctx, V2, case["Fl"])
    try:
        fresh = mi.trace_instances_device(ctx, p, f.MeshInstances(fresh_mesh, case["T"], tree=True, leaf_size=4), case["chord"], case["k0"],
                                          case["x0"])
    finally:
        fresh_mesh.close()
    _assert_same(after, fresh)
    assert not _same(after, before) and (after["inst"] >= 0).sum() >= 100

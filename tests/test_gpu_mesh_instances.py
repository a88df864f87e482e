"""bhg_trace_mesh_instances_device on the device: K rigid placements of one built mesh against

  1. the plain mesh trace, bit for bit, for one instance under the identity (x - 0 and 1 x + 0 y + 0 z are exact);
  2. the C oracle's brute-force mesh trace on the FLATTENED mesh (vertices V @ R_j.T + t_j, triangle j * nt + T = instance j,
     triangle T) on three placements of a 128-triangle ellipsoid, in both Schwarzschild forms and Kerr at +-0.45: rays the oracle
     calls stable in both senses (the 1-2 ulp perturbations of k0, and three draws scaling every flattened vertex coordinate by
     1 +- 1 ... 2e-16 -- the rounding that separates local from world arithmetic) agree in flags, step counts and (instance,
     triangle), Kerr with the step-count allowances of tests/test_gpu_mesh_oracle.py; unstable rays give an answer the oracle
     gives near by; hit ends stay within mesh_oracle_cases.hit_tolerances with sens the larger of the two sensitivities, bary
     within that over the shortest edge;
  3. order and ties: a permuted instance array gives the same bits with inst_id mapped through the permutation, identical records
     answer instance 0, 64 tetrahedra on a ring agree with the oracle;
  4. moving: set(T2) is a fresh set created with T2, the mesh's info is untouched, traces and moves enqueued back to back on
     several streams without a host wait see each the transforms of their turn, BHGEO_MESH_CULL=0 (no whole-step cull, no
     instance box) gives the same bits (a child process), a placement whose bulge enters a step's box only through the dense-output deviation is found.

tests/test_mesh_instances_host.py asserts the conditions of the cases on the CPU.

Measured when this was written (MI355X; no case has an unstable ray, no stable ray differs in flag, step counts or (instance,
triangle), Kerr included):
  case          rays   hits   worst |end - oracle|   worst |bary - oracle|   smallest margin left (end, bary)
  christoffel   2048   262    9.3e-13                2.9e-12                 1.1e-10, 3.8e-10
  reduced       2048   262    8.4e-13                2.6e-12                 1.1e-10, 3.8e-10
  kerr_plus     2048   270    1.7e-11                8.1e-11                 1.0e-9, 3.5e-9
  kerr_minus    2048   256    2.5e-11                1.3e-10                 1.0e-9, 3.5e-9
  ring64        1024   464    1.2e-11                5.2e-12                 1.1e-10, 7.8e-11
  bulge         1200    19    5.4e-13                2.4e-12                 1.6e-10, 7.1e-10
The module takes 7 s, no test more than 2."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as mc
import mesh_instance_cases as mi
import mesh_oracle_cases as mo
import mesh_reference as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAGGED = 2085          # 2 048 rays and a tail that fills no wave
WORST = {}


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


@pytest.fixture(scope="module", autouse=True)
def _totals():
    yield
    print("\nmesh instances against the oracle, worst values per case:")
    for name, rec in WORST.items():
        print(f"  {name}: {rec}")


def _same(a, b, keys=mi.KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# ---- 1. one instance under the identity is the plain mesh trace ----------------------------------------------------------------
def _ragged_rays():
    rng = np.random.default_rng(29)
    k = mi.three_rays()
    return np.concatenate([k, mr.camera_rays(mo.FRAME_CAM, mi.PLACES[1], N_RAGGED - len(k), rng, 1.6)])


@pytest.mark.parametrize("events", [False, True], ids=["bare", "disk_and_exit"])
@pytest.mark.parametrize("form", ["christoffel", "reduced", "kerr_plus"])
def test_identity_is_the_plain_mesh_trace(ctx, form, events):
    f = _ffi()
    rhs, a = mi.FORMS[form]
    V, F = mi.flatten(*mi.ellipsoid(), mi.three_placements())       # the three ellipsoids as ONE mesh where they stand
    par = dict(r_s=1.0, lambda_end=64.0)
    if events:
        par.update(r_exit=30.0, disk_r_in=2.0, disk_r_out=6.0)
    p = f.make_params(rhs_form=rhs, spin=a, **par)
    k0 = _ragged_rays()
    mesh = f.Mesh(ctx, V, F)
    try:
        plain = mc.trace_mesh_device(ctx, p, mesh, 0.25, k0, mo.FRAME_CAM)
        got = mi.trace_instances_device(ctx, p, f.MeshInstances(mesh, mi.IDENTITY), 0.25, k0, mo.FRAME_CAM)
    finally:
        mesh.close()
    for k in ("end", "flags", "n_steps", "n_accepted", "tri", "bary"):
        assert np.array_equal(got[k], plain[k]), k
    hit = plain["tri"] >= 0
    assert hit.sum() >= 200 and np.all(got["inst"][hit] == 0) and np.all(got["inst"][~hit] == -1)
    assert np.all(got["bary"][~hit] == mi.SENTINEL)


# ---- 2. against the oracle on the flattened mesh -------------------------------------------------------------------------------
def _hold(oracle, case, r, label):
    """The device's instanced result r against the oracle on the case's flattened mesh, every ray."""
    o = mi.oracle_solve(oracle, case)
    n, nt, K = len(case["k0"]), len(case["Fl"]), len(case["T"])
    kerr = case["rhs"] == 2
    stable = o["stable"]
    assert (~stable).sum() <= mo.UNSTABLE_CAP * n            # (tests/test_mesh_instances_host.py asserts it on the CPU)
    on_mesh = r["tri"] >= 0
    assert np.array_equal(on_mesh, r["flags"] == 0x88) and np.all(r["tri"][~on_mesh] == -1) and np.all(r["tri"] < nt)
    assert np.array_equal(on_mesh, r["inst"] >= 0) and np.all(r["inst"][~on_mesh] == -1) and np.all(r["inst"] < K)
    assert np.all(r["bary"][~on_mesh] == mi.SENTINEL) and not np.any(r["bary"][on_mesh] == mi.SENTINEL)
    flat = np.where(on_mesh, r["inst"] * nt + r["tri"], -1)
    steps_same = (r["n_steps"] == o["n_attempted"]) & (r["n_accepted"] == o["n_accepted"])
    agree = steps_same & (r["flags"] == o["flags"]) & (flat == o["tri"])
    bad = stable & ~agree
    if not kerr:
        assert not bad.any(), (np.flatnonzero(bad)[:8], r["flags"][bad][:8], o["flags"][bad][:8], flat[bad][:8], o["tri"][bad][:8])
    else:                                          # the allowances of tests/test_gpu_mesh_oracle.py (mode "kerr"), no others
        assert np.array_equal(r["flags"][stable], o["flags"][stable]) and np.array_equal(flat[stable], o["tri"][stable])
        assert bad.sum() <= 4, int(bad.sum())
        dstep = np.abs(r["n_steps"].astype(int) - o["n_attempted"].astype(int))
        assert dstep[bad].max(initial=0) <= 2
    for i in np.flatnonzero(~stable & ~agree):
        got = (int(r["flags"][i]), int(flat[i]), int(r["n_steps"][i]), int(r["n_accepted"][i]))
        seen = mo.oracle_nearby(oracle, case, i) | o["near_v"][i]
        assert got in seen, f"unstable ray {i}: GPU {got}, oracle near by {seen}"
    hit = stable & agree & (o["tri"] >= 0)
    assert hit.sum() >= 15
    tol, shortest = mo.hit_tolerances(case["V"], case["F"], o["end"][hit], o["tri"][hit], o["sens"][hit], kerr)
    diff = np.abs(r["end"][hit] - o["end"][hit]).max(1)
    dbary = np.abs(r["bary"][hit] - o["bary"][hit]).max(1)
    WORST[label] = dict(rays=n, hits=int(hit.sum()), unstable=int((~stable).sum()), other_counts=int(bad.sum()),
                        worst_end=float(diff.max()), smallest_end_margin=float((tol - diff).min()), worst_bary=float(dbary.max()),
                        smallest_bary_margin=float((tol / shortest - dbary).min()))
    print(f"{label}: {WORST[label]}")
    assert np.all(diff <= tol), (diff - tol).max()
    assert np.all(dbary <= tol / shortest), (dbary - tol / shortest).max()
    # every ray that ends elsewhere ends where the oracle's does (the bound of tests/test_gpu_mesh_oracle.py for its class)
    from test_gpu_parity import COND as COND_END
    from test_gpu_parity import TOL_END
    miss = stable & agree & (o["tri"] < 0) & np.isfinite(o["end"]).all(1)
    sens = np.nan_to_num(o["sens"][miss], nan=np.inf, posinf=np.inf)
    fl = o["flags"][miss]
    tol_m = TOL_END + COND_END * (10.0 if kerr else 1.0) * sens + np.where((fl & 1) != 0, 1e-6, 0.0)
    kd = o["end"][miss, 3:6]
    with np.errstate(invalid="ignore", divide="ignore"):
        steep = np.abs(kd[:, 2]) / np.linalg.norm(kd, axis=1)
    tol_m = tol_m + np.where(fl == 128, 1e-11 / np.maximum(np.nan_to_num(steep), 1e-12), 0.0)
    assert np.all(np.abs(r["end"][miss] - o["end"][miss]).max(1) <= tol_m)
    return o


THREE = mi.three_placement_cases()


@pytest.fixture(scope="module")
def three_results(ctx):
    """The three-placement case of every form through the device, once (the cull on): shared by tests 2, 3 and 4."""
    assert os.environ.get("BHGEO_MESH_CULL", "") != "0"
    return {name: mi.run_case(ctx, case) for name, case in THREE.items()}


@pytest.mark.parametrize("form", list(THREE))
def test_three_placements_against_the_oracle(oracle, three_results, form):
    case, r = THREE[form], three_results[form]
    o = _hold(oracle, case, r, form)
    per = np.bincount(r["inst"][r["inst"] >= 0], minlength=3)
    assert np.all(per >= mi.MIN_HITS_PER_INSTANCE) and np.all(mi.hits_per_instance(o, case) >= mi.MIN_HITS_PER_INSTANCE), per
    # a hit lies on its triangle in the instance's own frame
    hit = r["tri"] >= 0
    v0, e1, e2 = mr.tri_arrays(case["Vl"], case["Fl"])
    t = r["tri"][hit]
    local = v0[t] + r["bary"][hit, :1] * e1[t] + r["bary"][hit, 1:] * e2[t]
    R = case["T"][r["inst"][hit], :9].reshape(-1, 3, 3)
    world = np.einsum("nij,nj->ni", R, local) + case["T"][r["inst"][hit], 9:]
    if case["rhs"] != 2:
        assert np.abs(world - r["end"][hit, :3]).max() < 1e-9


# ---- 3. order and ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["christoffel", "kerr_minus"])
def test_permuting_the_instances_permutes_inst_id(ctx, three_results, form):
    case, r = THREE[form], three_results[form]
    perm = np.array([2, 0, 1])                 # new position j holds old instance perm[j]
    q = mi.run_case(ctx, case, T=case["T"][perm])
    for k in ("end", "flags", "n_steps", "n_accepted", "tri", "bary"):
        assert np.array_equal(q[k], r[k]), k
    hit = r["inst"] >= 0
    assert np.array_equal(perm[q["inst"][hit]], r["inst"][hit]) and np.all(q["inst"][~hit] == -1)


def test_identical_records_answer_instance_0(ctx, three_results):
    case, r = THREE["reduced"], three_results["reduced"]
    twice = mi.run_case(ctx, case, T=np.repeat(case["T"], 2, axis=0))      # 0 0 1 1 2 2
    for k in ("end", "flags", "n_steps", "n_accepted", "tri", "bary"):
        assert np.array_equal(twice[k], r[k]), k
    hit = r["inst"] >= 0
    assert hit.sum() >= 200 and np.array_equal(twice["inst"][hit], 2 * r["inst"][hit]) and np.all(twice["inst"][~hit] == -1)
    same = mi.run_case(ctx, case, T=np.tile(case["T"][1:2], (5, 1)))
    assert (same["inst"] >= 0).sum() >= 100 and np.all(same["inst"][same["inst"] >= 0] == 0)


def test_64_tetrahedra_on_a_ring_against_the_oracle(ctx, oracle):
    case = mi.ring_case()
    assert len(case["T"]) == _ffi().MESH_INSTANCES_MAX == 64
    r = mi.run_case(ctx, case)
    o = _hold(oracle, case, r, "ring64")
    assert mi.hits_per_instance(o, case).min() >= 1                 # every instance is hit by some ray, on the oracle's result
    assert len(np.unique(r["inst"][r["inst"] >= 0])) == 64


# ---- 4. moving -----------------------------------------------------------------------------------------------------------------
def test_set_is_a_fresh_set_and_leaves_the_mesh_alone(ctx, three_results):
    f = _ffi()
    case = THREE["christoffel"]
    p = f.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"])
    T2 = case["T"].copy()
    T2[:, 9:] += [[0.4, -0.3, 0.2], [-0.5, 0.1, 0.3], [0.2, 0.6, -0.4]]
    T2[0, :9] = (mi.rotation((0.0, 0.0, 1.0), 0.5) @ T2[0, :9].reshape(3, 3)).reshape(9)
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        info = mesh.info()
        inst = f.MeshInstances(mesh, case["T"])
        n0, box0 = inst.info()
        first = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        assert _same(first, three_results["christoffel"])
        inst.set(T2)
        moved = mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"])
        fresh_set = f.MeshInstances(mesh, T2)
        fresh = mi.trace_instances_device(ctx, p, fresh_set, case["chord"], case["k0"], case["x0"])
        assert _same(moved, fresh) and not _same(moved, first)
        assert (moved["inst"] >= 0).sum() >= 100
        n1, box1 = inst.info()
        assert n0 == n1 == 3 and not np.array_equal(box0, box1) and np.array_equal(box1, fresh_set.info()[1])
        # the union box holds every placed vertex
        Vf, _ = mi.flatten(case["Vl"], case["Fl"], T2)
        assert np.all(Vf >= box1[:3]) and np.all(Vf <= box1[3:])
        after = mesh.info()
        assert info[0] == after[0] and info[1] == after[1] and np.array_equal(info[2], after[2])
        # back again: the first bits
        inst.set(case["T"])
        assert _same(mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"]), first)
        # refused, the set left as it was: another n, a transform that is not rigid
        with pytest.raises(ValueError):
            inst.set(T2[:2])
        bad = T2.copy()
        bad[1, 0] += 1e-6
        with pytest.raises(f.BhgError, match="R\\^T R"):
            inst.set(bad)
        assert _same(mi.trace_instances_device(ctx, p, inst, case["chord"], case["k0"], case["x0"]), first)
    finally:
        mesh.close()


def test_moving_needs_no_synchronisation(ctx, three_results):
    """Traces and set() calls enqueued back to back, the traces on two streams that are not the context's, the host never waiting:
    every trace sees exactly the transforms that were set when it was enqueued (the set orders its uploads against its readers)."""
    import torch
    f = _ffi()
    case = THREE["christoffel"]
    p = f.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"])
    n = len(case["k0"])
    Ts = [case["T"]]
    for k in range(1, 6):
        T = case["T"].copy()
        T[:, 9:] += 0.15 * k * np.array([[1.0, -0.5, 0.3], [-0.7, 0.2, 0.4], [0.3, 0.8, -0.6]])
        Ts.append(T)
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    try:
        want = []
        for T in Ts:
            want.append(mi.trace_instances_device(ctx, p, f.MeshInstances(mesh, T), case["chord"], case["k0"], case["x0"]))
        assert _same(want[0], three_results["christoffel"]) and not any(_same(want[0], w) for w in want[1:])
        inst = f.MeshInstances(mesh, Ts[0])
        d_k0 = torch.as_tensor(case["k0"]).cuda()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
        outs = []
        order = [0, 1, 2, 3, 4, 5, 0, 3]
        for k, which in enumerate(order):
            if k:
                inst.set(Ts[which])
                if k == 4:                      # (two more moves nobody traces: only the last one counts)
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


def test_the_culls_change_nothing(ctx, three_results, tmp_path):
    out = str(tmp_path / "nocull.npz")
    env = dict(os.environ, BHGEO_MESH_CULL="0")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mesh_instance_cases.py"), out], check=True, env=env, timeout=300)
    plain = np.load(out)
    culled = {f"three_{form}__{k}": three_results[form][k] for form in ("christoffel", "kerr_plus") for k in mi.KEYS}
    for key, arr in mi.run_case(ctx, mi.bulge_case()).items():
        culled[f"bulge__{key}"] = arr
    assert sorted(plain.files) == sorted(culled)
    for key in plain.files:
        assert np.array_equal(plain[key], culled[key], equal_nan=True), key
    assert sum(int((culled[k] >= 0).sum()) for k in culled if k.endswith("__inst")) >= 500


def test_a_bulge_into_a_moved_box_is_found(ctx, oracle):
    case = mi.bulge_case()
    r = mi.run_case(ctx, case)
    _hold(oracle, case, r, "bulge")
    assert (r["inst"] == 0).sum() >= 15


# ---- the refusals that need a device, the host call and the integrator -----------------------------------------------------------
def test_refusals_host_call_and_integrator(ctx, three_results):
    import ctypes as C
    f = _ffi()
    L = f.load()
    case = THREE["reduced"]
    p = f.make_params(rhs_form=case["rhs"], spin=case["spin"], **case["par"])
    sel = slice(300, 600)            # (rays aimed at the second placement, in plain view)
    k0, x0 = np.ascontiguousarray(case["k0"][sel]), case["x0"]
    mesh = f.Mesh(ctx, case["Vl"], case["Fl"])
    inst = f.MeshInstances(mesh, case["T"])
    # the host call is the device call
    end, flags, steps, acc, tri, iid, bary = ctx.trace_mesh_instances(k0, x0, p, inst, case["chord"])
    r = three_results["reduced"]
    assert np.array_equal(end, r["end"][sel]) and np.array_equal(flags, r["flags"][sel]) and np.array_equal(steps, r["n_steps"][sel])
    assert np.array_equal(acc, r["n_accepted"][sel]) and np.array_equal(tri, r["tri"][sel]) and np.array_equal(iid, r["inst"][sel])
    hit = tri >= 0
    assert hit.sum() >= 20 and np.array_equal(bary[hit], r["bary"][sel][hit]) and np.all(np.isnan(bary[~hit]))
    # the integrator
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild(mass=0.5, time_like=False, verbose=False, device=0, rhs_form="reduced")
    out = gi.trace(k0, x0, curve_end=case["par"]["lambda_end"], r_exit=case["par"]["r_exit"],
                   disk=(case["par"]["disk_r_in"], case["par"]["disk_r_out"]), mesh=(case["Vl"], case["Fl"]), mesh_chord=case["chord"],
                   mesh_instances=case["T"].reshape(3, 12))
    assert np.array_equal(out["inst_id"], iid) and np.array_equal(out["tri_id"], tri) and np.array_equal(out["ray_end"], end)
    assert "inst_id" not in gi.trace(k0[:8], x0, mesh=(case["Vl"], case["Fl"]))
    # refused before anything is written: NULL outputs, a set of another context, a set whose mesh is gone
    sent = np.full((300, 6), mi.SENTINEL)

    def host(c, handle, tri_p, iid_p, bary_p):
        t = np.full(300, -9, np.int32)
        i = np.full(300, -9, np.int32)
        b = np.full((300, 2), mi.SENTINEL)
        e = sent.copy()
        rc = L.bhg_trace_mesh_instances(c._h, C.byref(p), handle, case["chord"], x0.ctypes.data, 1, k0.ctypes.data, 300, e.ctypes.data, None,
                                        None, None, t.ctypes.data if tri_p else None, i.ctypes.data if iid_p else None,
                                        b.ctypes.data if bary_p else None)
        assert np.all(t == -9) and np.all(i == -9) and np.all(b == mi.SENTINEL) and np.array_equal(e, sent)
        return rc, L.bhg_last_error()

    rc, why = host(ctx, inst._h, True, False, True)
    assert rc == f.E_INVALID and b"inst_id is NULL" in why
    rc, why = host(ctx, inst._h, False, True, True)
    assert rc == f.E_INVALID and b"tri_id / bary is NULL" in why
    other = f.Context(0)
    try:
        rc, why = host(other, inst._h, True, True, True)
        assert rc == f.E_INVALID and b"another context" in why
    finally:
        other.close()
    # the mesh destroyed under its set (through the C calls: the Python classes close the set with its mesh)
    V, F = np.ascontiguousarray(case["Vl"]), np.ascontiguousarray(case["Fl"])
    hm, hi = C.c_void_p(), C.c_void_p()
    assert L.bhg_mesh_create(ctx._h, V.ctypes.data, len(V), F.ctypes.data, len(F), None, 4, C.byref(hm)) == 0
    assert L.bhg_mesh_instances_create(ctx._h, hm, 3, case["T"].ctypes.data, C.byref(hi)) == 0
    L.bhg_mesh_destroy(hm)
    rc, why = host(ctx, hi, True, True, True)
    assert rc == f.E_INVALID and b"mesh has been destroyed" in why
    assert L.bhg_mesh_instances_set(hi, case["T"].ctypes.data) == f.E_INVALID and b"mesh has been destroyed" in L.bhg_last_error()
    L.bhg_mesh_instances_destroy(hi)
    mesh.close()
    assert inst._h is None          # closed with its mesh

"""Instance trees without a GPU: the ABI surface, the refusals of bhg_mesh_instances_create_tree (its
bounds and the transforms are checked before the mesh and the context, so the library refuses them here too), the host builder
bhg_mesh_instance_tree_host -- its shape, its leaves, its boxes --, the builder and the layout under the host sanitizers
(tests/mesh_instance_tree_driver.cpp says what is checked), and the conditions of the cases beyond 64 placements that
tests/test_gpu_mesh_instance_tree.py compares with the oracle: on each the brute-force oracle on the flattened mesh calls NO ray
unstable, under the 1-2 ulp perturbations of k0 and under the three vertex draws of mesh_instance_cases.

Measured when this was written (the C oracle):
  case               K     rays   hits   distinct instances hit   unstable (k0, vertices)
  swarm              192   1152   515    166                      0, 0
  clump christoffel   96   1024   234     25                      0, 0
  clump kerr +0.45    96   1024   261     21                      0, 0"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_instance_cases as mi
import mesh_instance_tree_cases as mt
import mesh_oracle_cases as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bhg_mesh_instances_create_tree", "bhg_mesh_instances_tree_info", "bhg_mesh_instance_tree_host", "bhg_frame_set_mesh_instance_tree")
KS = (1, 2, 3, 5, 64, 65, 200, 1000)
LEAVES = (1, 2, 4)
LOCAL_BOX = np.array([-0.5, -0.4, -0.3, 0.5, 0.6, 0.7])


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


def test_exports_and_macros():
    f, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name in NEW:
        assert name in f.EXPORTS
        assert hasattr(L, name)
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"^#define\s+BHG_MESH_INSTANCE_TREE\s+1\s*$", hdr, re.M)
    assert re.search(r"^#define\s+BHG_MESH_INSTANCE_TREE_MAX\s+65536\s*$", hdr, re.M)
    assert re.search(r"^#define\s+BHG_MESH_INSTANCES_MAX\s+64\s*$", hdr, re.M)
    assert f.MESH_INSTANCE_TREE_MAX == 65536 and f.MESH_INSTANCES_MAX == 64
    assert L.bhg_version() == 10 and f.ABI_VERSION == 10
    assert hasattr(f, "mesh_instance_tree_host") and hasattr(f.MeshInstances, "tree_info")
    import inspect

    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    assert inspect.signature(f.MeshInstances.__init__).parameters["tree"].default is False
    assert inspect.signature(f.Frame.set_mesh_instances).parameters["tree"].default is False
    assert inspect.signature(DeviceFrame.set_mesh).parameters["instance_tree"].default is False
    assert inspect.signature(GeodesicIntegratorSchwarzschild.trace).parameters["mesh_instance_tree"].default is False


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def _create_rc(T, n=None, leaf=2):
    f, L = _lib()
    T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    h = C.c_void_p(77)
    rc = L.bhg_mesh_instances_create_tree(None, None, len(T) if n is None else n, None if T is None else T.ctypes.data, leaf, C.byref(h))
    assert h.value is None          # out is cleared whatever happens
    return rc, L.bhg_last_error()


def test_create_tree_refusals_come_before_mesh_and_context():
    f, L = _lib()
    good = mi.three_placements()
    rc, why = _create_rc(good)
    assert rc == f.E_INVALID and b"mesh is NULL" in why
    for n in (0, -1, 65537):
        rc, why = _create_rc(mi.IDENTITY, n=n)      # (n is refused before a transform is read)
        assert rc == f.E_INVALID and b"BHG_MESH_INSTANCE_TREE_MAX" in why, n
    for n in (65, 65536):
        rc, why = _create_rc(np.tile(mi.IDENTITY, (n, 1)))
        assert rc == f.E_INVALID and b"mesh is NULL" in why, n
    for leaf in (0, 9):
        rc, why = _create_rc(good, leaf=leaf)
        assert rc == f.E_INVALID and b"leaf_size must be in [1, 8]" in why, leaf
    for leaf in (1, 8):
        assert b"mesh is NULL" in _create_rc(good, leaf=leaf)[1]
    rc, why = _create_rc(None, n=2)
    assert rc == f.E_INVALID and b"transforms is NULL" in why
    bad = good.copy()
    bad[1, 5] = np.inf
    rc, why = _create_rc(bad)
    assert rc == f.E_INVALID and b"transforms must be finite" in why
    rc, why = _create_rc(mi.record(np.eye(3) * (1.0 + 1e-8), (1.0, 2.0, 3.0))[None, :])
    assert rc == f.E_INVALID and b"R^T R within 1e-9" in why
    rc, why = _create_rc(mi.record(np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))[None, :])
    assert rc == f.E_INVALID and b"det R > 0" in why
    assert L.bhg_mesh_instances_create_tree(None, None, 1, mi.IDENTITY.ctypes.data, 2, None) == f.E_INVALID and b"out is NULL" in L.bhg_last_error()
    # the old constructor and the old frame call are what they were
    h = C.c_void_p()
    T65 = np.tile(mi.IDENTITY, (65, 1))
    assert L.bhg_mesh_instances_create(None, None, 65, T65.ctypes.data, C.byref(h)) == f.E_INVALID
    assert b"n must be in [1, BHG_MESH_INSTANCES_MAX]" in L.bhg_last_error()
    assert L.bhg_mesh_instances_tree_info(None, None, None, None) == f.E_INVALID and b"inst is NULL" in L.bhg_last_error()
    assert L.bhg_frame_set_mesh_instance_tree(None, 1, mi.IDENTITY.ctypes.data, None, 2) == f.E_INVALID and b"frame is NULL" in L.bhg_last_error()


def test_integrator_wants_instances_with_a_tree():
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    gi = GeodesicIntegratorSchwarzschild.__new__(GeodesicIntegratorSchwarzschild)     # (no context: the checks come first)
    with pytest.raises(ValueError, match="mesh_instance_tree goes with mesh_instances="):
        gi.trace(np.array([[0.0, 1.0, 0.0]]), np.array([0.0, -10.0, 0.0]), mesh=(np.zeros((3, 3)), np.zeros((1, 3), np.int32)),
                 mesh_instance_tree=True)


# ---- the host builder ----------------------------------------------------------------------------------------------------------
def _records(K, identical, seed):
    rng = np.random.default_rng(seed)
    if identical:
        return np.tile(mi.record(mi.rotation((1.0, -2.0, 0.5), 0.9), (3.0, -1.0, 2.0)), (K, 1))
    return np.stack([mi.record(mi.rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi)), rng.normal(size=3) * 6.0) for _ in range(K)])


def _morton_topology(K, leaf):
    """(skip, first, count) of bhg_mesh_bvh_morton_host over K triangles: its topology depends on (K, leaf) alone."""
    f, L = _lib()
    V = np.ascontiguousarray(np.random.default_rng(K).normal(size=(K + 2, 3)))
    F = np.ascontiguousarray(np.stack([np.arange(K), np.arange(K) + 1, np.arange(K) + 2], 1), dtype=np.int32)
    cap = 2 * K - 1
    box = np.empty((cap, 6))
    skip, first, count = (np.empty(cap, np.int32) for _ in range(3))
    order = np.empty(K, np.int32)
    nn = C.c_size_t(0)
    rc = L.bhg_mesh_bvh_morton_host(V.ctypes.data, len(V), F.ctypes.data, K, leaf, box.ctypes.data, skip.ctypes.data, first.ctypes.data,
                                    count.ctypes.data, order.ctypes.data, cap, C.byref(nn))
    assert rc == 0, L.bhg_last_error()
    return skip[:nn.value], first[:nn.value], count[:nn.value]


@pytest.mark.parametrize("identical", [False, True], ids=["random", "identical"])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("K", KS)
def test_the_host_tree(K, leaf, identical):
    f, _ = _lib()
    T = _records(K, identical, 100 * K + leaf)
    box, skip, first, count, order, depth = f.mesh_instance_tree_host(LOCAL_BOX, T, leaf)
    # the shape is a function of (K, leaf) alone: that of the Morton tree over K triangles
    ms, mf, mc_ = _morton_topology(K, leaf)
    assert np.array_equal(skip, ms) and np.array_equal(first, mf) and np.array_equal(count, mc_)
    nn = len(skip)
    # identical records too are split down to leaf: depth = the least d with ceil(K / 2^d) <= leaf
    want_depth = next(d for d in range(32) if -(-K // 2 ** d) <= leaf)
    assert depth == want_depth
    level = np.zeros(nn, int)
    for i in range(nn):
        if count[i] == 0:
            level[i + 1] = level[skip[i + 1]] = level[i] + 1
    assert level.max() == depth
    # every instance in exactly one leaf
    assert sorted(order.tolist()) == list(range(K))
    leaves = np.flatnonzero(count > 0)
    assert count[leaves].sum() == K and np.all(count[leaves] <= leaf)
    assert np.array_equal(first[leaves], np.concatenate([[0], np.cumsum(count[leaves])[:-1]]))
    # the boxes: a leaf's the exact union of its instances' world boxes, an inner node's that of its children's
    wb = np.stack([f.mesh_instance_box_host(LOCAL_BOX, T[j]) for j in range(K)])
    for i in range(nn - 1, -1, -1):
        if count[i] > 0:
            w = wb[order[first[i]:first[i] + count[i]]]
            want = np.concatenate([w[:, :3].min(0), w[:, 3:].max(0)])
        else:
            l, r = i + 1, skip[i + 1]
            want = np.concatenate([np.minimum(box[l, :3], box[r, :3]), np.maximum(box[l, 3:], box[r, 3:])])
        assert np.array_equal(box[i], want), i
    # the split: on the longest axis of the centres' bounds, by (centre, index)
    if not identical and K > leaf:
        cen = 0.5 * (wb[:, :3] + wb[:, 3:])
        axis = int(np.argmax(cen.max(0) - cen.min(0)))
        left = order[:K // 2]
        right = order[K // 2:]
        assert cen[left, axis].max() <= cen[right, axis].min()


def test_the_host_tree_refusals():
    f, L = _lib()
    T = _records(5, False, 1)
    out = [np.empty((9, 6)), np.empty(9, np.int32), np.empty(9, np.int32), np.empty(9, np.int32), np.empty(5, np.int32)]
    nn, depth = C.c_int32(0), C.c_int32(0)

    def call(lb=LOCAL_BOX, n=5, leaf=2, ptrs=None, nnp=C.byref(nn)):
        p = [a.ctypes.data for a in out] if ptrs is None else ptrs
        return L.bhg_mesh_instance_tree_host(lb.ctypes.data, n, T.ctypes.data, leaf, *p, nnp, C.byref(depth)), L.bhg_last_error()

    assert call()[0] == 0 and nn.value == 5 and depth.value == 2
    assert b"local_box must be finite" in call(lb=np.array([0, 0, 0, 1, np.nan, 1.0]))[1]
    assert b"BHG_MESH_INSTANCE_TREE_MAX" in call(n=0)[1]
    assert b"leaf_size" in call(leaf=9)[1]
    assert b"an output array is NULL" in call(ptrs=[out[0].ctypes.data, None, out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data])[1]
    assert b"n_nodes is NULL" in call(nnp=None)[1]


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------
def test_builder_and_layout_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "mesh_instance_tree_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "mesh_instance_tree_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    sets, checks = map(int, re.fullmatch(r"sets (\d+) checks (\d+)\n", r.stdout).groups())
    assert sets == len(KS) * len(LEAVES) * 2 and checks > 30 * sets


# ---- the cases of the GPU comparison -------------------------------------------------------------------------------------------
CASES = mt.beyond_cases()


def test_the_cases_are_what_they_say():
    swarm = CASES["swarm"]
    assert len(swarm["T"]) == 192 and len(swarm["k0"]) == 1152 and len(swarm["Fl"]) == 4
    assert np.allclose(np.linalg.norm(swarm["T"][:, 9:], axis=1), np.repeat([7.0, 9.0, 11.0], 64))
    for form in ("clump_christoffel", "clump_kerr_plus"):
        c = CASES[form]
        assert len(c["T"]) == 96 and len(c["k0"]) == 1024
        assert np.linalg.norm(c["T"][:, 9:] - np.asarray(mo.FRAME_SPHERE), axis=1).max() <= 1.5
        # the world boxes overlap heavily: every box meets at least ten others
        f, _ = _lib()
        lb = np.concatenate([c["Vl"].min(0), c["Vl"].max(0)])
        wb = np.stack([f.mesh_instance_box_host(lb, t) for t in c["T"]])
        meets = np.all((wb[:, None, :3] <= wb[None, :, 3:]) & (wb[None, :, :3] <= wb[:, None, 3:]), axis=2)
        assert (meets.sum(1) - 1).min() >= 10
    assert CASES["clump_kerr_plus"]["rhs"] == 2 and CASES["clump_kerr_plus"]["spin"] == 0.45


@pytest.mark.parametrize("name", list(CASES))
def test_the_oracle_alone_is_stable_on_the_cases(oracle, name):
    case = CASES[name]
    o = mi.oracle_solve(oracle, case)
    n = len(case["k0"])
    per = mi.hits_per_instance(o, case)
    hit = o["tri"] >= 0
    print(f"{name}: {n} rays, {int(hit.sum())} hits on {int((per > 0).sum())} instances, unstable k0 {int((~o['stable_k']).sum())}, "
          f"vertices {int((~o['stable_v']).sum())}")
    # the project's cap stands for what a comparison may leave out; on these cases the oracle alone leaves out nothing
    assert (~o["stable"]).sum() <= mo.UNSTABLE_CAP * n
    assert (~o["stable_k"]).sum() == 0 and (~o["stable_v"]).sum() == 0
    if name == "swarm":
        assert hit.sum() >= 400 and (per > 0).sum() >= 150 and (per[64:] > 0).sum() >= 80      # (well beyond the first 64)
    else:
        assert hit.sum() >= 200 and (per > 0).sum() >= 15

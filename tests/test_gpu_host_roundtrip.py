"""The six host-buffer entry points that stage their arrays through one device block -- bhg_trace_crossings, bhg_travel_time,
bhg_trace_mesh, bhg_redshift_motion_host, bhg_polarisation_host, bhg_disk_thermal_host -- against their _device twins: the same
inputs uploaded with torch, the same prefill of every array on both sides (-7.0 in the in-out arrays cross, t_cross and bary), the
arrays that come back compared byte for byte.  A wrong offset in the staging block, a missing upload of an in-out array or a
download of the wrong region shows as a difference; so does an optional output whose absence moves a required one.

Scene: the crossings tests' inclined camera, disk and exit sphere (tests/test_gpu_disk_crossings.py), the mesh tests' tetrahedron
and one moving object sphere half way to the hole.  The first rays are aimed: at the disk, at the hole, away from it, at the
tetrahedron, at the sphere; the rest are the crossings tests' seeded frame rays."""
import ctypes as C

import numpy as np
import pytest

import mesh_reference as mr
import test_gpu_disk_crossings as tc

pytestmark = pytest.mark.gpu

NS = [1, 63, 65, 130]
N_MAX = max(NS)
K = 3
CHORD = 0.25
HALF = 0.5 * tc.CAM
SPHERES = np.array([[HALF[0], -1.5, HALF[2], 0.8]])
FILL = {"f": -7.0, "u": 249, "i": -7}
OPTIONAL = ("flags", "n_steps", "n_accepted", "mu")
OPTIONAL_K0 = OPTIONAL + ("n_cross", "cross", "t_cross")       # the travel time at max_crossings = 0


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _aim(target):
    k = np.asarray(target, float) - tc.CAM
    return k / np.linalg.norm(k)


@pytest.fixture(scope="module")
def scene(ctx):
    """Rays, per-ray origins, settings and, per origin kind, the plain trace the per-ray-quantity calls take their inputs from."""
    f = _ffi()
    aimed = np.stack([_aim((8.0, 3.0, 0.0)), _aim((0.0, 0.0, 0.0)), -_aim((0.0, 0.0, 0.0)), _aim((HALF[0], 1.5, HALF[2])),
                      _aim(SPHERES[0, :3])])
    k0 = np.ascontiguousarray(np.concatenate([aimed, tc._inclined_rays(N_MAX - len(aimed))]))
    x0 = tc.CAM[None, :] + np.random.default_rng(17).uniform(-0.01, 0.01, (N_MAX, 3))
    p = f.make_params(**tc._kw(0, 0.0))
    S = dict(k0=k0, x0={True: np.ascontiguousarray(tc.CAM), False: np.ascontiguousarray(x0)}, p=p,
             mesh=f.Mesh(ctx, *mr.tetrahedron((HALF[0], 1.5, HALF[2]), 0.8)), rs=f.make_redshift(),
             mo=f.make_object_motion([[0.1, 0.0, 0.0]], [[0.0, 0.0, 0.05]]), pol=f.make_polarisation(),
             th=f.make_disk_thermal(1.2e4, *f.narrowband(2e14, 5e14, 9e14)), trace={})
    for shared in (True, False):
        end, flags, _, _, obj = ctx.trace(k0, S["x0"][shared], p, spheres=SPHERES)
        S["trace"][shared] = (np.ascontiguousarray(end), np.ascontiguousarray(flags), np.ascontiguousarray(obj))
        fl = flags[:min(NS[1:])]
        assert (fl & 1).any() and (fl == 128).any() and (fl == 8).any() and (fl == 0x88).any(), fl
    yield S
    S["mesh"].close()


class Side:
    """One side of a comparison: the caller's arrays in host memory (the host-buffer call) or uploaded with torch (the _device
    call).  out() hands an array prefilled with FILL to the call and keeps it for results()."""

    def __init__(self, device):
        self.device, self.keep, self.res = device, [], {}

    def _ptr(self, a):
        if not self.device:
            self.keep.append(a)
            return a.__array_interface__["data"][0]
        import torch
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def inp(self, a):
        return self._ptr(np.ascontiguousarray(a))

    def out(self, name, dtype, shape, want=True):
        if not want:
            return None
        a = np.full(shape, FILL[np.dtype(dtype).kind], dtype)
        p = self._ptr(a)
        self.res[name] = (self.keep[-1], a)
        return p

    def origin(self, x0):
        """the origin arguments: (x0, x0_is_shared) of a host-buffer call, (x0_shared, d_x0) of a _device call"""
        if not self.device:
            return self.inp(x0), int(x0.ndim == 1)
        return ((C.c_double * 3)(*x0), None) if x0.ndim == 1 else (None, self.inp(x0))

    def tail(self):
        if not self.device:
            return ()
        import torch
        return (C.c_void_p(torch.cuda.current_stream().cuda_stream),)

    def results(self):
        if not self.device:
            return {k: a for k, (_, a) in self.res.items()}
        import torch
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().view(a.dtype).reshape(a.shape) for k, (t, a) in self.res.items()}


def _call(ctx, S, entry, side, n, shared, opt):
    f, L = _ffi(), _ffi().load()
    h, p = ctx._h, C.byref(S["p"])
    fn = getattr(L, {"crossings": "bhg_trace_crossings", "travel_time": "bhg_travel_time", "travel_time_k0": "bhg_travel_time",
                     "mesh": "bhg_trace_mesh", "redshift": "bhg_redshift_motion", "polarisation": "bhg_polarisation",
                     "thermal": "bhg_disk_thermal"}[entry] + ("_device" if side.device else
                                                               "_host" if entry in ("redshift", "polarisation", "thermal") else ""))
    org, k0 = side.origin(S["x0"][shared][:n] if not shared else S["x0"][True]), side.inp(S["k0"][:n])
    f8, u1, u4, i4 = np.float64, np.uint8, np.uint32, np.int32
    counts = lambda: (side.out("flags", u1, (n,), opt), side.out("n_steps", u4, (n,), opt), side.out("n_accepted", u4, (n,), opt))
    if entry == "crossings":
        rc = fn(h, p, *org, k0, n, K, side.out("end", f8, (n, 6)), *counts(), side.out("cross", f8, (K, n, 6)),
                side.out("n_cross", u1, (n,)), *side.tail())
    elif entry == "travel_time":
        rc = fn(h, p, *org, k0, n, K, side.out("end", f8, (n, 6)), *counts(), side.out("cross", f8, (K, n, 6)),
                side.out("n_cross", u1, (n,)), side.out("t_end", f8, (n,)), side.out("t_cross", f8, (K, n)), *side.tail())
    elif entry == "travel_time_k0":
        # (max_crossings = 0: no records -- one layer is handed over when the arrays are given and must come back as it went)
        rc = fn(h, p, *org, k0, n, 0, side.out("end", f8, (n, 6)), *counts(), side.out("cross", f8, (1, n, 6), opt),
                side.out("n_cross", u1, (n,), opt), side.out("t_end", f8, (n,)), side.out("t_cross", f8, (1, n), opt), *side.tail())
    elif entry == "mesh":
        rc = fn(h, p, S["mesh"]._h, CHORD, *org, k0, n, side.out("end", f8, (n, 6)), *counts(), side.out("tri_id", i4, (n,)),
                side.out("bary", f8, (n, 2)), *side.tail())
    else:
        end, flags, obj = (side.inp(a[:n]) for a in S["trace"][shared])
        if entry == "redshift":
            rc = fn(h, p, C.byref(S["rs"]), None, C.byref(S["mo"]), SPHERES.ctypes.data, len(SPHERES), *org, k0, end, flags, obj, n,
                    side.out("g", f8, (n,)), *side.tail())
        elif entry == "polarisation":
            rc = fn(h, p, C.byref(S["pol"]), None, *org, k0, end, flags, n, side.out("evpa", f8, (n,)), side.out("degree", f8, (n,)),
                    side.out("mu", f8, (n,), opt), *side.tail())
        else:
            rc = fn(h, p, C.byref(S["th"]), None, *org, k0, end, flags, n, side.out("t_em", f8, (n,)), side.out("rgb", f8, (n, 3)),
                    *side.tail())
    res = side.results()
    assert rc == f.OK, (entry, rc, L.bhg_last_error().decode())
    return res


ENTRIES = ["crossings", "travel_time", "travel_time_k0", "mesh", "redshift", "polarisation", "thermal"]
WRITTEN_EVERYWHERE = ("end", "t_end", "tri_id", "g", "evpa", "degree", "t_em", "rgb")


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_ray"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_host_call_returns_the_device_call_s_bytes(ctx, scene, entry, n, shared):
    optional = OPTIONAL_K0 if entry == "travel_time_k0" else OPTIONAL
    got = {}
    for opt in (True, False):
        host = _call(ctx, scene, entry, Side(False), n, shared, opt)
        dev = _call(ctx, scene, entry, Side(True), n, shared, opt)
        assert set(host) == set(dev) and (opt or not set(host) & set(optional))
        for name in host:
            assert host[name].tobytes() == dev[name].tobytes(), (entry, n, shared, opt, name)
        got[opt] = host
    for name, a in got[False].items():          # the required outputs: the same with and without the optional ones
        assert a.tobytes() == got[True][name].tobytes(), (entry, n, shared, name)
        if name in WRITTEN_EVERYWHERE:
            assert not np.any(np.all(a.reshape(n, -1) == FILL[a.dtype.kind], axis=1)), (entry, name)
    if entry in ("crossings", "travel_time") and n > 1:
        # in-out: a ray's unreached records keep the prefill, a disk ray's first record does not
        cross, nc = got[True]["cross"], got[True]["n_cross"]
        assert np.all(cross[np.arange(K)[:, None] >= nc[None, :]] == FILL["f"]) and nc[0] >= 1 and np.all(cross[0, 0] != FILL["f"])
    if entry == "mesh" and n > 1:
        tri, bary = got[True]["tri_id"], got[True]["bary"]
        assert tri[3] >= 0 and np.all(bary[tri < 0] == FILL["f"]) and np.all(bary[tri >= 0] != FILL["f"])

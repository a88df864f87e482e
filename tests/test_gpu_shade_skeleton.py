"""The pixel reduction under every shade (shade_pixels_kernel and its serial twin, frame_kernels.hip), for each family that rides on
it: the image of P pixels of S samples is, bit for bit, the sum in sample order of the colours the same call gives the same device
records shaded as S * P pixels of one sample, times 1.0 / S.  The colour code is the reference -- other tests hold it to numpy --
and the reduction is the thing under test: S = 1 and 5 (the LDS kernel, a partial last workgroup at 5), 256 (one pixel per
workgroup) and 257 (the serial kernel, which the mesh and retarded families run nowhere else in the suite)."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_material_cases as mmc  # noqa: E402

pytestmark = pytest.mark.gpu

P = 53                       # prime: the last workgroup is partial at S = 5 (51 pixels each), one pixel per workgroup at S = 256
SAMPLES = (1, 5, 256, 257)
FAMILIES = ("scene", "polarised", "layers", "retarded", "mesh", "material")
# the scene of the crossings and travel-time tests (test_gpu_disk_crossings.py, test_gpu_travel_time.py): an inclined camera over
# a textured disk; the mesh families have mesh_material_cases' scene, opened wide enough to hold the hole's shadow
INC = np.radians(70.0)
CAM = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])
DISK = (3.0, 12.0)
PROFILE = dict(disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
TABLE = (0.0, 0.35, 0.2, 0.117)
SIZE = {"mesh": (48, 48), "material": (48, 48)}      # the pilot frame the 53 pixels are drawn from; every other family's is 32 x 32
_PIXELS = {}
_SKIES = {}


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


def _frame(ctx, family, S, pixels):
    """The family's frame with its scene set and nothing traced, its trace parameters, and its mesh (to close) or None."""
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    f = _ffi()
    W, H = SIZE.get(family, (32, 32))
    if family in ("mesh", "material"):
        V, F = mmc.SHADE_MESH
        M = mmc.material_arrays()
        mesh = f.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals())
        fr = mmc.device_frame(ctx, S, W=W, H=H, fov=(0.8, 0.8), pixels=pixels)
        if family == "material":
            fr.set_mesh(mesh, chord=mmc.CHORD, material=f.MeshMaterial(**M))
        else:
            fr.set_mesh(mesh, tri_rgb=M["tri_rgb"], chord=mmc.CHORD)
        return fr, f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=mmc.SHADE_DISK[0], disk_r_out=mmc.SHADE_DISK[1]), mesh
    if not _SKIES:
        _SKIES.update(sky=synthetic_sky(256, 128), tex=synthetic_sky(128, 32, seed=3))
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.6, fov_y=0.6, sampling_seed=42.0, origin=CAM, rotation_euler=(0.0, INC, 0.0), pixels=pixels)
    fr.set_sky(_SKIES["sky"])
    fr.set_disk(DISK[0], DISK[1], _SKIES["tex"], **PROFILE)
    if family == "polarised":
        fr.set_polarisation(TABLE, disk_sense=1)
    elif family == "layers":
        fr.set_disk_layers(3, 0.5)
    elif family == "retarded":
        fr.set_disk_layers(3, 0.5, phase_rate=0.05)
    return fr, f.make_params(r_s=1.0, lambda_end=120.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1]), None


def _trace(fr, p):
    import torch
    fr.generate_rays(p)
    fr.trace(p)
    torch.cuda.synchronize()


def _classes(fr, family):
    """The traced rays by what colours them: (disk, crossing or mesh hit; horizon; sky)."""
    f = _ffi()
    flags = fr.d_flags.cpu().numpy()
    horizon = (flags & f.FLAG_HIT_HORIZON) != 0
    if family in ("mesh", "material"):
        hit = (flags == f.FLAG_HIT_OBJECT) & (fr.d_tri_id.cpu().numpy() >= 0)
    elif family in ("layers", "retarded"):
        hit = fr.d_n_cross.cpu().numpy() >= 1
    else:
        hit = flags == f.FLAG_HIT_DISK
    return hit, horizon & ~hit, ~hit & ~horizon


def _pixels(ctx, family):
    """53 pixels of the family's pilot frame (whole, one sample): 22 whose ray is a hit, 10 a horizon ray, 21 a sky ray, spread evenly
    over each class.  Horizon pixels are black in every sample, hence the fewest."""
    if family not in _PIXELS:
        fr, p, mesh = _frame(ctx, family, 1, None)
        _trace(fr, p)

        def pick(mask, k):
            ids = np.flatnonzero(mask)
            return ids[np.linspace(0, len(ids) - 1, min(k, len(ids))).round().astype(int)]
        hit, horizon, sky = _classes(fr, family)
        print(f"{family}: the pilot frame has {int(hit.sum())} hit, {int(horizon.sum())} horizon and {int(sky.sum())} sky pixels")
        px = np.sort(np.concatenate([pick(hit, 22), pick(horizon, 10), pick(sky, 21)]))
        assert len(px) == P and len(set(px.tolist())) == P, (family, len(px))
        if mesh is not None:
            mesh.close()
        _PIXELS[family] = px
    return _PIXELS[family]


def _in_sample_order(per_ray, S, reverse=False):
    """What the kernels do with a pixel's S colours: from 0.0, one addition per sample in sample order, then times 1.0 / S."""
    acc = np.zeros((P,) + per_ray.shape[1:])
    for s in (range(S - 1, -1, -1) if reverse else range(S)):
        acc = acc + per_ray[s * P:(s + 1) * P]
    return acc * (1.0 / S)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("family", FAMILIES)
def test_the_image_is_the_rays_colours_summed_in_sample_order(ctx, family, S):
    import torch
    fr, p, mesh = _frame(ctx, family, S, _pixels(ctx, family))
    assert fr.P == P and fr.n == S * P
    _trace(fr, p)
    stokes = family == "polarised"
    if stokes:
        rgba, qu = fr.shade_stokes()
        got_qu = qu.cpu().numpy().copy()
    else:
        rgba = fr.shade()
    got = rgba.cpu().numpy().copy()
    out32 = torch.empty((P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out32)
    # the same records through the same call as S * P pixels of one sample: each ray's colour by itself
    one = copy.copy(fr)
    one.P, one.S = fr.n, 1
    one.d_rgba = torch.empty((fr.n, 4), dtype=torch.float64, device=fr.dev)
    one.d_qu = None
    if stokes:
        ray_rgba, ray_qu = (t.cpu().numpy().copy() for t in one.shade_stokes())
    else:
        ray_rgba = one.shade().cpu().numpy().copy()
    torch.cuda.synchronize()
    col = ray_rgba[:, :3]
    assert np.all(np.isfinite(col)) and np.all(ray_rgba[:, 3] == 1.0)
    # the case is not a vacuous one: every class of ray the family colours is there (20 rays of each from S = 5 on; the 53 rays
    # of S = 1 cannot hold three times 20, so there each class is asked for its pixels' share, 5 at the least) ...
    hit, horizon, sky = _classes(fr, family)
    per_pixel = col.reshape(S, P, 3)
    varied = (per_pixel != per_pixel[0]).any(axis=(0, 2))
    print(f"{family} S={S}: {int(hit.sum())} hit, {int(horizon.sum())} horizon, {int(sky.sum())} sky rays; "
          f"{int(varied.sum())} of {P} pixels with samples of different colours")
    least = 20 if S >= 5 else 5
    assert hit.sum() >= least and horizon.sum() >= least and sky.sum() >= least
    assert np.abs(col[hit]).max() > 0.0 and np.all(col[horizon] == 0.0)
    # ... a third of the pixels have samples of different colours ...
    assert S == 1 or 3 * varied.sum() >= P
    want = _in_sample_order(col, S)
    # ... and the order of the sum shows in the bits
    if S in (5, 257):
        assert (_in_sample_order(col, S, reverse=True) != want).any()
    assert np.array_equal(got[:, :3], want) and np.all(got[:, 3] == 1.0)
    assert np.array_equal(out32.cpu().numpy(), got.astype(np.float32))
    if stokes:
        assert np.abs(ray_qu[hit]).max() > 0.0 and np.all(ray_qu[~hit] == 0.0)
        want_qu = _in_sample_order(ray_qu, S)
        if S in (5, 257):
            assert (_in_sample_order(ray_qu, S, reverse=True) != want_qu).any()
        assert np.array_equal(got_qu, want_qu)
    if mesh is not None:
        mesh.close()

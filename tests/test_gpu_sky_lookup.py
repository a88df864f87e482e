"""The texture lookup (sky_lookup: u wraps, v clamps) at its edges, through the public shade calls and its three callers -- the
sky (bhg_shade_dir_device), the disk texture (bhg_shade_scene_device) and an emissive textured sphere
(bhg_shade_scene_textured_device) -- against a reference that forms u and v in np.longdouble from the direction and
interpolates in the same precision.

The conventions are the build's own: u = -atan2(d_y, d_x) / pi, v = 1 - 2 atan2(sqrt(d_x^2 + d_y^2),
d_z) / pi; with d_x = d_y = 0 of either sign the column is u = 0; texel centres at ((i + 1/2) / TW, (j + 1/2) / TH).

The bound is derived: bilinear interpolation is continuous across texel borders, so an angle error of atan2_fast's 4 ulp moves
the colour by at most the texel-to-texel difference times the error in texel units: |d rgb| <= 8 eps (TW + TH + 4) max|texel|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
PI = np.arctan2(LD(0), LD(-1))
EPS = 2.0 ** -52
# (w, h); the largest is 134 MB of float32
IMAGES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (128, 64), (4096, 2048)]


def _ffi():
    from blackhole_geodesic_calculator_amd import _ffi as f
    return f


def _image(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).random((h, w, 4), dtype=np.float32)


def _bound(img):
    h, w = img.shape[:2]
    return 8 * EPS * (w + h + 4) * float(img[..., :3].max())


def _angle(y, x):
    """atan2 in long double with the build's convention at the origin: atan2(+-0, +-0) = 0."""
    a = np.arctan2(y, x)
    return np.where((x == 0) & (y == 0), LD(0), a)


def lookup_ref(img, u, v):
    """Bilinear lookup in long double: u wraps, v clamps."""
    h, w = img.shape[:2]
    t = img[..., :3].astype(LD)
    fx = (u + 1) * LD(0.5) * w - LD(0.5)
    fy = (v + 1) * LD(0.5) * h - LD(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0f)[:, None], (fy - y0f)[:, None]
    x0 = np.mod(x0f.astype(np.int64), w)
    x1 = np.mod(x0 + 1, w)
    y0 = np.clip(y0f.astype(np.int64), 0, h - 1)
    y1 = np.clip(y0f.astype(np.int64) + 1, 0, h - 1)
    return (1 - ax) * (1 - ay) * t[y0, x0] + ax * (1 - ay) * t[y0, x1] + (1 - ax) * ay * t[y1, x0] + ax * ay * t[y1, x1]


def sky_ref(img, d):
    d = d.astype(LD)
    u = -_angle(d[:, 1], d[:, 0]) / PI
    v = 1 - 2 * _angle(np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2), d[:, 2]) / PI
    return lookup_ref(img, u, v)


TINY = float(np.nextafter(0.0, 1.0))


def edge_directions():
    """+-x, +-y, +-z exactly; every sign of zero on the poles; the seam (d_y = +0 and -0 with d_x < 0, and one ulp either side
    of it); one ulp off each pole; and all of these scaled by 1e-6 and 1e6 (exit directions are not unit vectors).  Returns the
    directions and the index pairs that must give the same colour because u wraps."""
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d += [[sx * 0.0, sy * 0.0, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1.0, -1.0)]
    seam0 = len(d)
    for dz in (0.0, 0.3, -2.0):
        d += [[-1.0, 0.0, dz], [-1.0, -0.0, dz], [-1.0, TINY, dz], [-1.0, -TINY, dz], [-1.0, 1e-300, dz], [-1.0, -1e-300, dz]]
    pairs = [(seam0 + 6 * j + a, seam0 + 6 * j + b) for j in range(3) for a, b in ((0, 1), (2, 3), (4, 5), (0, 2), (0, 4))]
    for sz in (1.0, -1.0):
        # (not a subnormal next to two zeros: atan2_fast's reciprocal of max(|x|, |y|) overflows below 2^-1022, device_math.h)
        d += [[1e-300, 0.0, sz], [-1e-300, 0.0, sz], [0.0, 1e-300, sz], [0.0, -1e-300, sz], [EPS, 0.0, sz], [-EPS, -0.0, sz],
              [0.0, EPS, sz], [-EPS, EPS, sz]]
    d = np.array(d, dtype=np.float64)
    return np.concatenate([d, 1e-6 * d, 1e6 * d]), pairs


def _directions(n_seeded=20000):
    e, pairs = edge_directions()
    rng = np.random.default_rng(33)
    s = rng.normal(size=(n_seeded, 3)) * 10.0 ** rng.uniform(-3, 3, (n_seeded, 1))
    return np.concatenate([e, s]), pairs


def _shade_dir(ctx, d, img, samples=1):
    import torch
    n = len(d)
    assert n % samples == 0
    d_dir = torch.as_tensor(np.ascontiguousarray(d)).cuda()
    d_fl = torch.full((n,), 4, dtype=torch.uint8, device="cuda")
    d_img = torch.as_tensor(img).cuda()
    rgba = torch.full((n // samples, 4), float("nan"), dtype=torch.float64, device="cuda")
    ctx.shade_dir_device(d_dir.data_ptr(), d_fl.data_ptr(), n // samples, samples, d_img.data_ptr(), img.shape[1], img.shape[0],
                         d_rgba=rgba.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rgba.cpu().numpy()


@pytest.mark.parametrize("w,h", IMAGES, ids=[f"{w}x{h}" for w, h in IMAGES])
def test_sky_lookup_at_the_edges(ctx, record_property, w, h):
    img = _image(w, h)
    d, pairs = _directions()
    got = _shade_dir(ctx, d, img)[:, :3]
    want = sky_ref(img, d)
    err = np.abs(got.astype(LD) - want).max(1).astype(np.float64)
    j = int(np.argmax(err))
    record_property("max_error", {"error": float(err[j]), "bound": _bound(img), "direction": [float(v).hex() for v in d[j]]})
    assert np.all(np.isfinite(got))
    assert err.max() <= _bound(img), (err.max(), _bound(img), d[j])
    for a, b in pairs:      # either side of the seam: the same colour, because u wraps
        assert np.abs(got[a] - got[b]).max() <= _bound(img), (a, b, got[a], got[b])
    # the pole convention: d_x = d_y = 0 of either sign is the column u = 0 -- the centre of the image's top (bottom) row
    top = lookup_ref(img, np.array([LD(0)]), np.array([LD(1)]))[0]
    bottom = lookup_ref(img, np.array([LD(0)]), np.array([LD(-1)]))[0]
    for i in range(6, 14):
        assert np.abs(got[i].astype(LD) - (top if d[i, 2] > 0 else bottom)).max() <= _bound(img)


def test_sky_lookup_mean_of_three_samples(ctx):
    img = _image(128, 64, seed=5)
    d, _ = _directions(3000)
    d = d[:len(d) - len(d) % 3]
    got = _shade_dir(ctx, d, img, samples=3)[:, :3]
    P = len(d) // 3
    one = sky_ref(img, d)
    want = (one[:P] + one[P:2 * P] + one[2 * P:]) / 3
    assert np.abs(got.astype(LD) - want).max() <= _bound(img)


# ---- the disk texture: texture_x = (disk_phase + acos(x / R) sign(y)) / pi, v = (R - r_in) / (r_out - r_in) ----------------------
def disk_ref(img, xy, r_in, r_out, phase, mean=0.2, stddev=0.3, intensity=1.0):
    """disk_colour in long double.  cos = x / R is taken as the source forms it -- the rounded double quotient of the rounded
    double R: next to the -x axis acos amplifies that rounding to 1e-8, which is the definition's, not the lookup's."""
    x, y = xy[:, 0], xy[:, 1]
    R = np.sqrt(x * x + y * y)
    cx = np.clip(x / R, -1.0, 1.0)
    scale = (R.astype(LD) - r_in) / (LD(r_out) - r_in)
    amp = intensity * np.exp(-((scale - mean) ** 2) / (2 * LD(stddev) ** 2)) / np.sqrt(2 * PI * stddev)
    tx = (LD(phase) + np.arccos(cx.astype(LD)) * np.where(y < 0.0, -1, 1)) / PI
    return lookup_ref(img, tx, scale) * amp[:, None]


@pytest.mark.parametrize("phase", [0.0, 0.4, 3.0, -7.5])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 1), (3, 5), (128, 64)])
def test_disk_texture_seam_and_phase(ctx, w, h, phase):
    """y = +-0 with x < 0 and one ulp either side; phases that push texture_x several periods beyond +-1: the floating-point
    modulo brings every one back."""
    import torch
    f = _ffi()
    img = _image(w, h, seed=9)
    r_in, r_out = 3.0, 9.0
    rng = np.random.default_rng(44)
    R = np.array([3.0, 3.5, 6.0, 8.999, 9.0])
    seam = np.concatenate([np.stack([-R, np.full(5, y)], 1) for y in (0.0, -0.0, TINY, -TINY, 1e-300, -1e-300)])
    ang = rng.uniform(-np.pi, np.pi, 5000)
    rr_ = rng.uniform(3.0, 9.0, 5000)
    axes = np.array([[4.0, 0.0], [4.0, -0.0], [0.0, 5.0], [0.0, -5.0]])
    xy = np.concatenate([seam, axes, np.stack([rr_ * np.cos(ang), rr_ * np.sin(ang)], 1)])
    n = len(xy)
    end = np.zeros((n, 6))
    end[:, :2] = xy
    d_end = torch.as_tensor(end).cuda()
    d_fl = torch.full((n,), 128, dtype=torch.uint8, device="cuda")
    d_img = torch.as_tensor(img).cuda()
    sky = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    rgba = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    sc = f.make_scene(sky.data_ptr(), 4, 2, d_disk_tex=d_img.data_ptr(), disk_w=w, disk_h=h, disk=(r_in, r_out), disk_phase=phase)
    ctx.shade_scene_device(d_end.data_ptr(), d_fl.data_ptr(), n, 1, sc, rgba.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = rgba.cpu().numpy()[:, :3]
    want = disk_ref(img, xy, r_in, r_out, phase)
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(LD) - want).max(1)
    assert err.max() <= _bound(img), (float(err.max()), _bound(img), xy[int(np.argmax(err))])
    for j in range(5):      # +0 and -0, +ulp and -ulp: texture_x differs by a whole period
        for a, b in ((0, 1), (2, 3), (4, 5), (0, 2)):
            assert np.abs(got[5 * a + j] - got[5 * b + j]).max() <= _bound(img)


# ---- an emissive textured sphere: U = atan2(n_y, n_x) / pi, V = 1 - 2 atan2(sqrt(n_x^2 + n_y^2), n_z) / pi of the body normal ----
@pytest.mark.parametrize("turned", [False, True])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (2, 2), (3, 5), (128, 64)])
def test_emissive_sphere_texture_on_the_body_axes(ctx, w, h, turned):
    import torch
    f = _ffi()
    img = _image(w, h, seed=13)
    c, rho, k, tint = np.array([4.0, -2.0, 1.0]), 2.0, 1.5, np.array([0.5, 1.0, 0.25])
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if turned else np.eye(3)     # body -> world, exact
    rng = np.random.default_rng(55)
    nb = np.concatenate([np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, -0.0, 0.0],
                                   [-0.5, 0.0, 0.5], [-0.5, -0.0, -0.5]], dtype=np.float64),
                         (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(3000, 3)))])
    n = len(nb)
    end = np.zeros((n, 6))
    end[:, :3] = c + rho * (nb @ rot.T)
    # the body normal as the kernel forms it, in long double from the record
    nw = (end[:, :3].astype(LD) - c) * (1 / LD(rho))
    b = nw @ rot.astype(LD)
    U = _angle(b[:, 1], b[:, 0]) / PI
    V = 1 - 2 * _angle(np.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2), b[:, 2]) / PI
    want = k * (tint * lookup_ref(img, U, V))
    d_end = torch.as_tensor(end).cuda()
    d_fl = torch.full((n,), 0x88, dtype=torch.uint8, device="cuda")
    d_obj = torch.zeros(n, dtype=torch.int8, device="cuda")
    d_img = torch.as_tensor(img).cuda()
    sky = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    rgba = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda")
    sc = f.make_scene(sky.data_ptr(), 4, 2, spheres=[[*c, rho]], sphere_rgb=[tint])
    ot = f.make_object_textures([(d_img.data_ptr(), w, h)], [rot], ["emissive"], [k])[0]
    ctx.shade_scene_textured_device(d_end.data_ptr(), d_fl.data_ptr(), n, 1, sc, f.make_params(r_s=1.0), None, None, ot,
                                    d_rgba=rgba.data_ptr(), d_object_id=d_obj.data_ptr(),
                                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = rgba.cpu().numpy()[:, :3]
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(LD) - want).max(1)
    assert err.max() <= k * _bound(img), (float(err.max()), k * _bound(img), nb[int(np.argmax(err))])
    assert np.abs(got[1] - got[6]).max() <= k * _bound(img)      # body -x with n_y = +0 and -0: the seam from both sides

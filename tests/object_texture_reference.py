"""numpy restatement of textured, oriented and emissive object spheres -- TEST INFRASTRUCTURE ONLY.

For a ray that ends on object sphere j (flags == 0x88, object_id = j) at the entry point e:

  n   = (e - c_j) / rho_j                     outward normal (object_colour's n)
  n_b = R_j^T n                               body frame; R_j row-major body -> world, the all-zero matrix = identity
  U   = atan2(n_b,y, n_b,x) / pi              body +x = the image's centre column
  V   = 1 - 2 atan2(sqrt(n_b,x^2 + n_b,y^2), n_b,z) / pi     body +z = the top row
  texel = the build's bilinear lookup (oracle.shade_reference.sky_lookup: u wraps, v clamps, rows bottom-up); white without a
          texture
  lit:      oracle.shade_reference.object_colour (sphere_rgb[j] times the Lambert lamp sum with shadow rays) * texel
  emissive: emission[j] * (sphere_rgb[j] * texel)      (no lamps, no shadows)

Redshift weighs the result like any other object ray (section 9): the emitter is at rest.

Written from the model, not from the device code: the angles are numpy's arctan2.
"""
import numpy as np

LIT, EMISSIVE = 0, 1
FLAG_HIT_OBJECT = 0x88


def rotation(R):
    """The effective body -> world rotation of a slot: the all-zero matrix is the identity."""
    R = np.asarray(R, float).reshape(3, 3)
    return np.eye(3) if not R.any() else R


def body_normal(n, R):
    """n [k, 3] world -> body: R^T n."""
    return np.asarray(n, float).reshape(-1, 3) @ rotation(R)


def body_uv(nb):
    """(U, V) in the sky's [-1, 1]^2 convention of body-frame normals nb [k, 3]."""
    nb = np.asarray(nb, float).reshape(-1, 3)
    U = np.arctan2(nb[:, 1], nb[:, 0]) / np.pi
    V = 1.0 - 2.0 * np.arctan2(np.hypot(nb[:, 0], nb[:, 1]), nb[:, 2]) / np.pi
    return U, V


def rot_z(psi):
    """A rotation about the body z axis by psi (body -> world)."""
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def random_rotation(rng):
    """A proper rotation (det +1) from a QR factorisation."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


class Textures:
    """The per-sphere table of bhg_object_textures, host side: tex[j] float32 [h, w, 4] or None (white), rot [8, 3, 3],
    mode [8], emission [8]."""

    def __init__(self, tex=None, rot=None, mode=None, emission=None, n=8):
        self.tex = list(tex) + [None] * (n - len(tex)) if tex is not None else [None] * n
        self.rot = np.zeros((n, 3, 3)) if rot is None else np.asarray(rot, float).reshape(-1, 3, 3)
        self.mode = np.zeros(n, int) if mode is None else np.asarray(mode, int)
        self.emission = np.zeros(n) if emission is None else np.asarray(emission, float)


def object_colour_textured(end, obj, spheres, sphere_rgb, lamps, T: Textures):
    """Section 11's colour of rays that end on object spheres: end [k, 6], obj [k]."""
    from oracle import shade_reference as sh
    spheres = np.asarray(spheres, float).reshape(-1, 4)
    sphere_rgb = np.asarray(sphere_rgb, float).reshape(-1, 3)
    lamps = np.zeros((0, 4)) if lamps is None else np.asarray(lamps, float).reshape(-1, 4)
    out = np.zeros((len(end), 3))
    obj = np.asarray(obj).astype(int)
    for j in range(len(spheres)):
        m = obj == j
        if not m.any():
            continue
        e = end[m]
        n = (e[:, 0:3] - spheres[j, 0:3]) * (1.0 / spheres[j, 3])
        texel = np.ones((m.sum(), 3))
        if T.tex[j] is not None:
            U, V = body_uv(body_normal(n, T.rot[j]))
            texel = sh.sky_lookup(np.asarray(T.tex[j], np.float32), U, V)
        if T.mode[j] == EMISSIVE:
            out[m] = T.emission[j] * (sphere_rgb[j] * texel)
        else:
            out[m] = sh.object_colour(e, np.full(len(e), j), spheres, sphere_rgb, lamps) * texel
    return out


def shade_scene_textured(end, flags, obj, n_pixels, samples, sky, T: Textures, g=None, exponent=4.0, apply=0, disk=None,
                         disk_tex=None, disk_profile=None, spheres=None, sphere_rgb=None, lamps=None):
    """oracle.shade_reference.shade_scene with section 11's object colour, optionally weighted by g^exponent for the classes in
    `apply` (redshift_reference.shade_scene_redshift's convention); samples accumulated in order."""
    from oracle import shade_reference as sh
    spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, float).reshape(-1, 4)
    sphere_rgb = np.ones((len(spheres), 3)) if sphere_rgb is None else np.asarray(sphere_rgb, float).reshape(-1, 3)
    acc = np.zeros((n_pixels, 3))
    for s in range(samples):
        sl = slice(s * n_pixels, (s + 1) * n_pixels)
        e, f = end[sl], flags[sl]
        one = sh.shade_scene(e, f, None if obj is None else obj[sl], n_pixels, 1, sky, disk=disk, disk_tex=disk_tex,
                             disk_profile=disk_profile, spheres=None, sphere_rgb=None, lamps=None)[:, :3]
        is_disk = (f == 128) if disk is not None else np.zeros(len(f), bool)
        is_obj = (f == FLAG_HIT_OBJECT) if len(spheres) else np.zeros(len(f), bool)
        if is_obj.any():
            one[is_obj] = object_colour_textured(e[is_obj], obj[sl][is_obj], spheres, sphere_rgb, lamps, T)
        w = np.ones(len(f))
        if g is not None:
            gs = g[sl]
            is_sky = ~is_disk & ~is_obj & ((f & (1 | 64)) == 0)
            for m, bit in ((is_disk, 1), (is_obj, 2), (is_sky, 4)):
                if apply & bit:
                    w[m] = gs[m] ** exponent
        acc += np.nan_to_num(one * w[:, None])
    return np.concatenate([acc / samples, np.ones((n_pixels, 1))], 1)


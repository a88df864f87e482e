"""The mesh material in numpy (include/bhgeo.h, "mesh material"): the texel restated from the header's
words, and the material colour on top of mesh_reference.mesh_colour's lamp sum.  No GPU, no library."""
import numpy as np

import mesh_reference as mr


def texel(img, U, V):
    """img [H, W, 4] float32, U / V arrays (fp64): the bilinear RGB texel [n, 3], the image repeating in both directions."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    U, V = np.atleast_1d(np.asarray(U, dtype=np.float64)), np.atleast_1d(np.asarray(V, dtype=np.float64))
    fx, fy = U * W - 0.5, V * H - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    c0, c1 = np.mod(x0, W).astype(np.int64), np.mod(x0 + 1.0, W).astype(np.int64)
    r0, r1 = np.mod(y0, H).astype(np.int64), np.mod(y0 + 1.0, H).astype(np.int64)
    t = img[..., :3].astype(np.float64)
    return ((1.0 - ax) * (1.0 - ay) * t[r0, c0] + ax * (1.0 - ay) * t[r0, c1] + (1.0 - ax) * ay * t[r1, c0] + ax * ay * t[r1, c1])


def hit_uv(tri, bary, tri_uv):
    """(U, V) of each hit: the corner UVs (fp32) interpolated in fp64 with the unclamped plane coordinates."""
    uv = np.asarray(tri_uv, dtype=np.float32).astype(np.float64)[tri]     # [n, 3, 2]
    u, v = bary[:, 0], bary[:, 1]
    w = 1.0 - u - v
    return (w * uv[:, 0, 0] + u * uv[:, 1, 0] + v * uv[:, 2, 0], w * uv[:, 0, 1] + u * uv[:, 1, 1] + v * uv[:, 2, 1])


def albedo(tri, bary, nt, tri_rgb=None, tri_uv=None, tri_tex=None, textures=()):
    """tri_rgb[tri] (or 1) x texel (or 1) per hit, [n, 3]."""
    a = np.ones((len(tri), 3)) if tri_rgb is None else np.asarray(tri_rgb, dtype=np.float32).astype(np.float64)[tri]
    if tri_uv is None:
        return a
    slot = np.zeros(nt, np.int64) if tri_tex is None else np.asarray(tri_tex, dtype=np.int64)
    U, V = hit_uv(tri, bary, tri_uv)
    for j, img in enumerate(textures):
        sel = slot[tri] == j
        if sel.any():
            a[sel] = a[sel] * texel(img, U[sel], V[sel])
    return a


def material_colour(end, tri, bary, V, F, lamps, normals=None, tri_rgb=None, tri_uv=None, tri_tex=None, textures=(), emission=0.0,
                    tree=None, margins=None):
    """albedo x (lamp_sum + emission) per mesh ray: the lamp sum is mesh_reference.mesh_colour's with a white mesh."""
    lamp_sum = mr.mesh_colour(end, tri, bary, V, F, lamps, None, normals, tree=tree, margins=margins)[:, :1]
    return albedo(tri, bary, len(F), tri_rgb, tri_uv, tri_tex, textures) * (lamp_sum + emission)

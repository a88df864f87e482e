"""The Morton tree of the device-side mesh build, restated in numpy, and the meshes that
tests/test_mesh_build_host.py and tests/test_gpu_mesh_build.py share.  Not a test module.

The statement (csrc/mesh_bvh.h, build_bvh_morton, says the same in C++ and csrc/mesh_build.hip in kernels):
    centroid   c_t[a] = (V[F[t][0]][a] + V[F[t][1]][a] + V[F[t][2]][a]) / 3.0, left to right
    bounds     lo, hi = the exact min / max of the centroids, ext = hi - lo
    cell       q[a] = 0 unless ext[a] is finite and > 0, else min(2^21 - 1, trunc((c_t[a] - lo[a]) * (2097152.0 / ext[a])));
               a product that is not > 0 (a NaN from 0 * inf included, when the quotient overflows) gives 0
    key        bit k of qx, qy, qz at key bit 3 k + 2, 3 k + 1, 3 k
    order      the stable sort of 0 .. nt - 1 by key
    topology   build_bvh's pre-order with skip links; m slots are a leaf when m <= leaf_size, else split into m // 2 and the rest
    leaf order rising caller index inside every leaf
    boxes      mesh_refit_cases.refit_numpy (fit_boxes restated)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_refit_cases as rc  # noqa: E402

CELLS = 2097152.0     # 2^21 per axis


def centroids(V, F):
    V = np.asarray(V, np.float64)
    with np.errstate(over="ignore"):
        return (V[F[:, 0]] + V[F[:, 1]] + V[F[:, 2]]) / 3.0


def cells(V, F):
    """[nt, 3] uint64: the cell of every centroid"""
    c = centroids(V, F)
    lo, hi = c.min(0), c.max(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ext = hi - lo
        on = np.isfinite(ext) & (ext > 0.0)
        scale = np.where(on, CELLS / np.where(on, ext, 1.0), 0.0)
        f = (c - lo) * scale
    q = np.zeros(c.shape, np.uint64)
    for a in range(3):
        if not on[a]:
            continue
        fa = f[:, a]
        pos = fa > 0.0          # (False for a NaN)
        q[pos, a] = np.minimum(np.trunc(np.minimum(fa[pos], CELLS)), CELLS - 1.0).astype(np.uint64)
    return q


def keys(V, F):
    q = cells(V, F)
    key = np.zeros(len(q), np.uint64)
    for k in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            key |= ((q[:, a] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + shift)
    return key


def keys_python(V, F):
    """The keys again with Python's integers: no fixed width anywhere in the interleave."""
    out = []
    for qx, qy, qz in cells(V, F).tolist():
        key = 0
        for k in range(21):
            key |= ((qx >> k) & 1) << (3 * k + 2) | ((qy >> k) & 1) << (3 * k + 1) | ((qz >> k) & 1) << (3 * k)
        out.append(key)
    return out


def topology(nt, leaf_size):
    """(skip, first, count, depth) of the count-split tree over nt slots"""
    first, count, depth_of = [], [], []
    stack = [(0, nt, 0)]
    while stack:
        lo, hi, d = stack.pop()
        m = hi - lo
        depth_of.append(d)
        if m <= leaf_size:
            first.append(lo)
            count.append(m)
            continue
        first.append(-1)
        count.append(0)
        mid = lo + m // 2
        stack.append((mid, hi, d + 1))
        stack.append((lo, mid, d + 1))
    nn = len(first)
    skip = [0] * nn
    for i in range(nn - 1, -1, -1):
        skip[i] = i + 1 if count[i] > 0 else skip[skip[i + 1]]
    return np.array(skip, np.int32), np.array(first, np.int32), np.array(count, np.int32), max(depth_of)


def morton_tree(V, F, leaf_size):
    """mesh_bvh_host's dict (box, skip, first, count, order) of the Morton tree, and its depth under "depth" """
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int32)
    order = np.argsort(keys(V, F), kind="stable").astype(np.int32)
    skip, first, count, depth = topology(len(F), leaf_size)
    for i in np.flatnonzero(count > 0):
        order[first[i]:first[i] + count[i]].sort()
    tree = {"skip": skip, "first": first, "count": count, "order": order, "depth": depth}
    with np.errstate(over="ignore", invalid="ignore"):
        tree["box"] = rc.refit_numpy(V, F, tree)[0]
    return tree


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def grid_mesh(nt, seed=5, centre=rc.CENTRE, size=2.4):
    """A jittered grid of quads, two triangles each, cut to its first nt triangles: a bumpy sheet about `centre`."""
    rng = np.random.default_rng(seed)
    n = int(np.ceil(np.sqrt((nt + 1) // 2)))
    g = np.linspace(-0.5, 0.5, n + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([X, Y, 0.15 * np.sin(5.0 * X) * np.cos(4.0 * Y)], -1).reshape(-1, 3)
    P[:, :2] += rng.uniform(-0.3, 0.3, (len(P), 2)) / n
    at = lambda i, j: i * (n + 1) + j      # noqa: E731
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    quads = np.stack([at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j), at(i + 1, j + 1), at(i, j + 1)], 1)
    F = np.ascontiguousarray(quads.reshape(-1, 3)[:nt], np.int32)
    assert len(F) == nt
    return np.ascontiguousarray(P * size + np.asarray(centre, float)), F


def wide_range_mesh(nt=96, seed=9):
    """Triangles whose positions span 1e-3 .. 1e6 on every axis: most cells crowd near 0, and the largest centroid on each axis
    lies exactly at hi, where the product reaches 2^21 and the clamp decides."""
    rng = np.random.default_rng(seed)
    c = 10.0 ** rng.uniform(-3.0, 6.0, (nt, 1, 3)) * rng.choice([-1.0, 1.0], (nt, 1, 3))
    V = (c * (1.0 + 0.01 * rng.normal(size=(nt, 3, 3)))).reshape(-1, 3)
    return np.ascontiguousarray(V), np.arange(nt * 3, dtype=np.int32).reshape(nt, 3)


def overflow_mesh():
    """Finite vertices whose centroid sums overflow: on x some centroids are +inf and some -inf (ext = inf), on y all are +inf
    (ext = inf - inf, a NaN), z is ordinary.  Both overflowing axes give cell 0; no NaN reaches a key."""
    big = 1.5e308
    x = np.array([big, big, -big, -big, 1.0, 2.0, 3.0, -4.0])
    rng = np.random.default_rng(4)
    nt = len(x)
    V = np.empty((nt, 3, 3))
    V[:, :, 0] = x[:, None] * (1.0 + 0.01 * rng.uniform(size=(nt, 3)))
    V[:, :, 1] = big * (1.0 + 0.01 * rng.uniform(size=(nt, 3)))
    V[:, :, 2] = rng.normal(size=(nt, 3))
    return np.ascontiguousarray(V.reshape(-1, 3)), np.arange(nt * 3, dtype=np.int32).reshape(nt, 3)


def meshes():
    """name -> (V, F, leaf sizes): mesh_refit_cases.meshes() at the device build's leaf sizes, and the cases of its own"""
    base = rc.meshes()
    V, F, _ = base["ellipsoid128"]
    out = {
        "one": (*base["one"][:2], (1,)),
        "identical5": (*base["identical5"][:2], (4,)),
        "ellipsoid128": (V, F, (1, 4, 64)),
        "sphere4097": (*base["sphere4097"][:2], (1, 4)),
        "plate": (*base["plate"][:2], (1, 4)),
        "spare_vertices": (*base["spare_vertices"][:2], (1, 4)),
        "nt_is_leaf": (V, F[:4], (4,)),
        "nt_is_leaf_plus_1": (V, F[:5], (4,)),
        "wide_range": (*wide_range_mesh(), (1, 4)),
        "overflow": (*overflow_mesh(), (1, 4)),
    }
    return out


GRID_SIZES = (1, 255, 256, 257, 4097, 70001)
# one size above the 2^20 pairs up to which the device's sort merges and from which it takes its radix passes
GRID_SIZE_RADIX = 2**20 + 3

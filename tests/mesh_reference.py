"""Shared by the triangle-mesh tests (tests/test_mesh_host.py on the CPU, tests/test_gpu_mesh.py on the GPU, and
tests/golden/make_golden_mesh.py): the restatement of the hit rule of DESIGN.md section 19 on scipy's own dense output, the
brute-force and the skip-link segment tests, the mesh colour, and the meshes and ray sets of the tests.  Not a test module.

The solve is scipy.solve_ivp(..., dense_output=True) on oracle/scipy_reference's right-hand sides with the horizon and the exit
sphere as terminal events and the disk plane as a non-terminal one (tests/crossings_reference.py's arrangement); the rule is
applied afterwards to sol.sol.interpolants with a brute-force Moeller-Trumbore over all triangles."""
import numpy as np

FORM_NAMES = ("christoffel", "reduced", "kerr")
MAX_SUBSTEPS = 1024
FLAG_HIT_HORIZON, FLAG_START_INSIDE, FLAG_REACHED_END, FLAG_EXITED, FLAG_TOO_SMALL, FLAG_HIT_DISK, FLAG_HIT_OBJECT = 1, 2, 4, 8, 32, 128, 0x88


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def octa_sphere(centre, radius, sub=1):
    """An octahedron subdivided `sub` times onto the sphere: 8 * 4^sub triangles."""
    v = [np.array(p, float) for p in [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(sub):
        nf, cache = [], {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, float), np.array(f, np.int32)


def tetrahedron(centre, size):
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], float) * size + np.asarray(centre, float)
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


def join(*meshes):
    """Several meshes as one (two separate components)."""
    V, F, off = [], [], 0
    for v, f in meshes:
        V.append(v)
        F.append(f + off)
        off += len(v)
    return np.concatenate(V), np.concatenate(F).astype(np.int32)


def random_triangles(n, rng, spread=5.0, size=0.6):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    V = (c + rng.normal(size=(n, 3, 3)) * size).reshape(-1, 3)
    return V, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def inscribed_radius(V, F, centre):
    """The smallest distance from `centre` to a triangle's plane (a convex mesh about the centre: its inscribed radius)."""
    v0, e1, e2 = V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.abs(np.einsum("ij,ij->i", v0 - np.asarray(centre, float), n)).min()


def vertex_normals_about(V, centre):
    n = V - np.asarray(centre, float)
    return n / np.linalg.norm(n, axis=1)[:, None]


# ---- the segment tests -----------------------------------------------------------------------------------------------------
def tri_arrays(V, F):
    V = np.asarray(V, float)
    return V[F[:, 0]], V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def moller_trumbore(p, d, v0, e1, e2):
    """The segment p + s d against triangles (v0, e1, e2) [m, 3] -> (hit [m], s, u, v), operation for operation the library's
    (no fused multiply-add: the library is built with -ffp-contract=off)."""
    pv = _cross(d[None, :], e2)
    det = _dot(e1, pv)
    ok = det != 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / det
        tv = p[None, :] - v0
        u = _dot(tv, pv) * inv
        qv = _cross(tv, e1)
        v = _dot(d[None, :], qv) * inv
        s = _dot(e2, qv) * inv
        hit = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (s >= 0.0) & (s <= 1.0)
    return hit, s, u, v


def segment_brute(p, q, tris):
    """First hit of the segment p -> q over ALL triangles: (s, triangle) with the smallest s, ties to the smaller index; None."""
    v0, e1, e2 = tris
    hit, s, _, _ = moller_trumbore(p, q - p, v0, e1, e2)
    if not hit.any():
        return None
    idx = np.flatnonzero(hit)
    j = idx[np.argmin(s[idx])]          # (argmin takes the first of equals: the smaller index)
    return float(s[j]), int(j)


def box_test(b, p, d, s_max):
    """segment_meets_box of csrc/mesh_traverse.h."""
    t_near, t_far = 0.0, s_max
    for c in range(3):
        if d[c] == 0.0:
            if p[c] < b[c] or p[c] > b[3 + c]:
                return False
        else:
            inv = 1.0 / d[c]
            t1, t2 = (b[c] - p[c]) * inv, (b[3 + c] - p[c]) * inv
            t_near = max(t_near, min(t1, t2))
            t_far = min(t_far, max(t1, t2))
    return t_near <= t_far + 1e-10 * (1.0 + abs(t_near) + abs(t_far))


def segment_tree(p, q, tree, tris, any_hit=False, count=None):
    """segment_first_hit of csrc/mesh_traverse.h on the flattened tree of bhg_mesh_bvh_host: (s, triangle) or None.  count: a list
    that receives the number of triangle tests."""
    v0, e1, e2 = tris
    d = q - p
    best, best_tri, i, nn, tested = 1.0, -1, 0, len(tree["skip"]), 0
    while i < nn:
        if not box_test(tree["box"][i], p, d, best):
            i = int(tree["skip"][i])
            continue
        cnt = int(tree["count"][i])
        if cnt:
            ids = tree["order"][tree["first"][i]:tree["first"][i] + cnt]
            tested += cnt
            hit, s, _, _ = moller_trumbore(p, d, v0[ids], e1[ids], e2[ids])
            for k in np.flatnonzero(hit):
                if any_hit:
                    return float(s[k]), int(ids[k])
                if best_tri < 0 or s[k] < best or (s[k] == best and ids[k] < best_tri):
                    best, best_tri = float(s[k]), int(ids[k])
        i += 1
    if count is not None:
        count.append(tested)
    return None if best_tri < 0 else (best, best_tri)


# ---- the rule on scipy's dense output ---------------------------------------------------------------------------------------
def plane_coordinates(x, v0, e1, e2):
    n = np.cross(e1, e2)
    w = x - v0
    nn = n @ n
    return np.array([np.cross(w, e2) @ n / nn, np.cross(e1, w) @ n / nn])


def brent(g, a, b):
    """scipy's brentq with solve_ivp's tolerances (ivp.py:51-76: xtol = rtol = 4 eps)."""
    from scipy.optimize import brentq
    eps = np.finfo(float).eps
    return brentq(g, a, b, xtol=4 * eps, rtol=4 * eps)


def solve(k0, x0, rhs_form, V, F, max_chord, r_s=1.0, spin=0.0, lambda_end=80.0, rtol=1e-3, atol=1e-6, max_step=np.inf, r_exit=0.0,
          disk=None, tris=None):
    """One ray -> dict(flags, end [6], n_accepted, n_attempted (-1 where scipy's count is not comparable: it integrated on past
    the event), tri (-1: none), bary [2], M and step of the hit, sag (|refined point - chord hit|))."""
    from scipy.integrate import solve_ivp
    from oracle import scipy_reference as sr
    k0, x0 = np.asarray(k0, float), np.asarray(x0, float)
    tris = tri_arrays(V, F) if tris is None else tris
    kerr = rhs_form == 2
    out = dict(tri=-1, bary=np.full(2, np.nan), M=0, step=-1, sag=np.nan)
    if kerr:
        M_ = 0.5 * r_s
        fn = sr.kerr_rhs_lambdified()
        q0, u0 = sr.cart_to_bl(x0, k0, spin)
        r_h = (M_ + np.sqrt(M_ * M_ - spin * spin)) * (1 + sr.KERR_HORIZON_MARGIN)
        if q0[0] <= r_h:
            out.update(flags=FLAG_START_INSIDE | FLAG_HIT_HORIZON, end=np.concatenate([x0, k0]), n_accepted=0, n_attempted=0)
            return out
        E, L, _ = sr.kerr_constants(q0, u0, M_, spin, 0.0)

        def rhs(_t, y):
            ar, ath, aph, _kt = fn(y[1], y[3], y[0], y[2], y[4], E, L, M_, spin)
            return np.array([ar, y[0], ath, y[2], aph, y[4]])

        y0 = np.array([u0[0], q0[0], u0[1], q0[1], u0[2], q0[2]])
        radius = lambda y: y[1]                                                                     # noqa: E731
        ev_d = lambda _t, y: np.cos(y[3])                                                           # noqa: E731

        def cart(y):
            R = np.sqrt(y[1] * y[1] + spin * spin)
            return np.array([R * np.sin(y[3]) * np.cos(y[5]), R * np.sin(y[3]) * np.sin(y[5]), y[1] * np.cos(y[3])])

        def record(y):
            return np.concatenate(sr.bl_to_cart((y[1], y[3], y[5]), (y[0], y[2], y[4]), spin))

        cyl = lambda y: np.sqrt(y[1] * y[1] + spin * spin) * abs(np.sin(y[3]))                      # noqa: E731
    else:
        r_h = r_s
        if np.sqrt(x0 @ x0) <= r_s:
            out.update(flags=FLAG_START_INSIDE | FLAG_HIT_HORIZON, end=np.concatenate([x0, k0]), n_accepted=0, n_attempted=0)
            return out
        rhs = sr.make_rhs(r_s, FORM_NAMES[rhs_form], False)
        y0 = np.array([k0[0], x0[0], k0[1], x0[1], k0[2], x0[2]])
        radius = lambda y: np.sqrt(y[1] * y[1] + y[3] * y[3] + y[5] * y[5])                         # noqa: E731
        ev_d = lambda _t, y: y[5]                                                                   # noqa: E731
        cart = lambda y: np.array([y[1], y[3], y[5]])                                               # noqa: E731
        record = lambda y: np.array([y[1], y[3], y[5], y[0], y[2], y[4]])                           # noqa: E731
        cyl = lambda y: np.sqrt(y[1] * y[1] + y[3] * y[3])                                          # noqa: E731
    ev_h = lambda _t, y: radius(y) - r_h                                                            # noqa: E731
    ev_h.terminal = True
    events = [ev_h]
    if r_exit > 0.0:
        ev_e = lambda _t, y: radius(y) - r_exit                                                     # noqa: E731
        ev_e.terminal, ev_e.direction = True, 1.0
        events.append(ev_e)
    if disk is not None:
        events.append(ev_d)
    sol = solve_ivp(rhs, (0.0, lambda_end), y0, events=events, dense_output=True, rtol=rtol, atol=atol, max_step=max_step)
    n_term = len(events) - (1 if disk is not None else 0)
    if sol.status == 1:
        te, i_ev = min((sol.t_events[i][-1], i) for i in range(n_term) if len(sol.t_events[i]))
        flags, ye = (FLAG_HIT_HORIZON if i_ev == 0 else FLAG_EXITED), sol.y_events[i_ev][-1]
    elif sol.status == 0:
        flags, te, ye = FLAG_REACHED_END, sol.t[-1], sol.y[:, -1]
    else:
        flags, te, ye = FLAG_TOO_SMALL, sol.t[-1], sol.y[:, -1]
    n_acc, n_att = len(sol.t) - 1, (int(sol.nfev) - 2) // 6
    if disk is not None:
        for td, yd in zip(sol.t_events[-1], sol.y_events[-1]):
            if disk[0] <= cyl(yd) <= disk[1] and td <= te:
                flags, te, ye = FLAG_HIT_DISK, td, yd
                n_acc, n_att = int(np.searchsorted(sol.t, td, side="left")), -1
                break
    out.update(flags=flags, end=record(ye), n_accepted=n_acc, n_attempted=n_att, t_end=float(te))
    # the rule, step by step, up to the terminal root
    v0, e1, e2 = tris
    corners = np.concatenate([v0, v0 + e1, v0 + e2])
    mesh_lo, mesh_hi = corners.min(0), corners.max(0)
    for j, ip in enumerate(sol.sol.interpolants):
        ta, tb = sol.t[j], sol.t[j + 1]
        if ta >= te:
            break
        L = np.linalg.norm(cart(sol.y[:, j + 1]) - cart(sol.y[:, j]))
        want = np.ceil(L / max_chord)
        M = MAX_SUBSTEPS if not want < MAX_SUBSTEPS else max(1, int(want))
        h = tb - ta
        # (a shortcut that changes no answer: when the box of the step's samples -- evaluated in one call, widened far beyond
        # the rounding between that call and the per-sample ones below -- misses the mesh's box, no sub-chord meets a triangle)
        ts = ta + (h * np.arange(M + 1)) / M
        pts = np.array([cart(y) for y in ip(ts).T]) if M > 1 else np.array([cart(sol.y[:, j]), cart(sol.y[:, j + 1])])
        if np.any(pts.min(0) - 1e-6 > mesh_hi) or np.any(pts.max(0) + 1e-6 < mesh_lo):
            continue
        t_lo, p_lo = ta, cart(ip(ta))
        for m in range(M):
            if t_lo >= te:
                break
            t_hi = tb if m + 1 == M else ta + (h * (m + 1)) / M
            p_hi = cart(ip(t_hi))
            hit = segment_brute(p_lo, p_hi, tris)
            if hit is not None:
                s, tri = hit
                n = np.cross(e1[tri], e2[tri])
                g = lambda t: n @ (cart(ip(t)) - v0[tri])                                           # noqa: E731
                ga, gb = g(t_lo), g(t_hi)
                if ga == 0.0:
                    root = t_lo
                elif gb == 0.0:
                    root = t_hi
                elif (ga < 0.0) == (gb < 0.0):
                    root = t_lo if abs(ga) <= abs(gb) else t_hi
                else:
                    root = brent(g, t_lo, t_hi)
                if root <= te:
                    y = ip(root)
                    x = cart(y)
                    out.update(flags=FLAG_HIT_OBJECT, end=record(y), n_accepted=j + 1, n_attempted=-1, tri=tri,
                               bary=plane_coordinates(x, v0[tri], e1[tri], e2[tri]), M=M, step=j, t_end=float(root),
                               sag=float(np.linalg.norm(x - (p_lo + s * (p_hi - p_lo)))))
                return out
            t_lo, p_lo = t_hi, p_hi
    return out


def perturbations(k0):
    """tests/crossings_reference.py's three 1-2 ulp patterns."""
    eps = np.finfo(float).eps
    return (np.nextafter(k0, np.inf), np.nextafter(k0, -np.inf), k0 * (1.0 + np.array([2.0, -2.0, 2.0]) * eps))


def solve_set(k0, x0, rhs_form, V, F, max_chord, **par):
    """solve over a ray set with its perturbations: arrays plus sens [n] (the end record's largest movement under the three
    perturbations) and stable [n] (flag, triangle, step counts and M of the hit step unchanged under them)."""
    k0 = np.atleast_2d(np.asarray(k0, float))
    n = len(k0)
    tris = tri_arrays(V, F)
    out = dict(end=np.zeros((n, 6)), flags=np.zeros(n, np.uint8), n_attempted=np.zeros(n, np.int64), n_accepted=np.zeros(n, np.uint32),
               tri=np.zeros(n, np.int32), bary=np.zeros((n, 2)), M=np.zeros(n, np.int32), sag=np.zeros(n), sens=np.zeros(n),
               stable=np.ones(n, bool))
    for i in range(n):
        r = solve(k0[i], x0, rhs_form, V, F, max_chord, tris=tris, **par)
        for key in ("end", "flags", "n_attempted", "n_accepted", "tri", "bary", "M", "sag"):
            out[key][i] = r[key]
        for kp in perturbations(k0[i]):
            q = solve(kp, x0, rhs_form, V, F, max_chord, tris=tris, **par)
            if any(q[key] != r[key] for key in ("flags", "tri", "n_attempted", "n_accepted", "M")):
                out["stable"][i] = False
                continue
            out["sens"][i] = max(out["sens"][i], np.abs(q["end"] - r["end"]).max())
    return out


def camera_rays(x0, target, n, rng, spread):
    """n unit directions from x0 towards points scattered `spread` about `target` (a disc facing the camera)."""
    x0, target = np.asarray(x0, float), np.asarray(target, float)
    look = (target - x0) / np.linalg.norm(target - x0)
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, look)
    rho, phi = spread * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
    aim = target[None, :] + (rho * np.cos(phi))[:, None] * right[None, :] + (rho * np.sin(phi))[:, None] * up[None, :]
    k = aim - x0[None, :]
    return k / np.linalg.norm(k, axis=1)[:, None]


def hole_rays(x0, n, rng, b_lo=0.5, b_hi=6.0):
    """tests/crossings_reference.py's camera rays without the critical share: look at the hole, impact parameter b uniform."""
    x0 = np.asarray(x0, float)
    d = np.linalg.norm(x0)
    look = -x0 / d
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, look)
    b, phi = rng.uniform(b_lo, b_hi, n), rng.uniform(0.0, 2.0 * np.pi, n)
    k = look[None, :] + (b / d)[:, None] * (np.cos(phi)[:, None] * right[None, :] + np.sin(phi)[:, None] * up[None, :])
    return k / np.linalg.norm(k, axis=1)[:, None]


# ---- the golden cases (tests/golden/make_golden_mesh.py writes them, tests/test_gpu_mesh.py reads them) ------------------------
GOLDEN_CAM = np.array([20.0, 0.0, 2.0])
GOLDEN_PAR = dict(r_s=1.0, lambda_end=80.0, rtol=1e-3, atol=1e-6)
GOLDEN_CHORD = 0.25
GOLDEN_FORMS = [(0, 0.0), (1, 0.0), (2, 0.225), (2, 0.45)]      # (rhs_form, Kerr a): a / M = 0.45 and 0.9 with M = 0.5
GOLDEN_FORM_IDS = ["christoffel", "reduced", "kerr045", "kerr09"]
GOLDEN_R_EXIT = 40.0            # the Cartesian forms (the Kerr cases run to lambda_end, as the crossings golden does)


def golden_meshes():
    """name -> (V, F): the 32-triangle sphere behind the hole (secondary images), a tetrahedron in front, two components."""
    return {
        "behind": octa_sphere((-4.0, 0.5, 0.0), 1.5, 1),
        "front": tetrahedron((9.0, 0.3, 1.2), 0.8),
        "two": join(octa_sphere((-3.5, 2.5, 0.5), 1.0, 1), tetrahedron((5.0, -1.5, 0.5), 0.7)),
    }


def golden_rays(name, n, rng):
    if name == "front":
        return np.concatenate([camera_rays(GOLDEN_CAM, (9.0, 0.3, 1.2), n // 2, rng, 1.6), hole_rays(GOLDEN_CAM, n - n // 2, rng)])
    if name == "two":
        m = n // 3
        return np.concatenate([camera_rays(GOLDEN_CAM, (5.0, -1.5, 0.5), m, rng, 1.2), camera_rays(GOLDEN_CAM, (-3.5, 2.9, 0.5), m, rng, 1.6),
                               hole_rays(GOLDEN_CAM, n - 2 * m, rng)])
    return hole_rays(GOLDEN_CAM, n, rng)


# ---- the mesh colour -------------------------------------------------------------------------------------------------------
def mesh_colour(end, tri, bary, V, F, lamps, tri_rgb=None, vertex_normals=None, tree=None, margins=None, shadows=True):
    """bhg_shade_mesh_device's colour of mesh rays: end [m, 6], tri [m], bary [m, 2] -> rgb [m, 3].  margins: a list that receives,
    per shadow decision, the smallest barycentric margin min(u, v, 1 - u - v, s, 1 - s) over the triangles the shadow segment's
    line meets within 1e-9 of an edge (the decisions a rounding could turn).  shadows=False: the lamp sum without shadow rays."""
    V = np.asarray(V, float)
    tris = tri_arrays(V, F)
    v0, e1, e2 = tris
    out = np.zeros((len(end), 3))
    for i in range(len(end)):
        t = int(tri[i])
        x, kdir = end[i, :3], end[i, 3:]
        if vertex_normals is not None:
            N = np.asarray(vertex_normals, float)[F[t]]
            u, v = bary[i]
            w = 1.0 - u - v
            n = w * N[0] + u * N[1] + v * N[2]
        else:
            n = np.cross(e1[t], e2[t])
        length = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        sgn = -1.0 if n[0] * kdir[0] + n[1] * kdir[1] + n[2] * kdir[2] > 0.0 else 1.0
        n = sgn * (n / length)
        tot = 0.0
        for lx, ly, lz, li in np.asarray(lamps, float).reshape(-1, 4):
            lamp = np.array([lx, ly, lz])
            lv = lamp - x
            d2 = lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2]
            dist = np.sqrt(d2)
            ld = lv / dist
            ndl = n[0] * ld[0] + n[1] * ld[1] + n[2] * ld[2]
            if not ndl > 0.0:
                continue
            p = x + 1e-5 * ld
            if margins is not None:
                hit, s, uu, vv = moller_trumbore(p, lamp - p, v0, e1, e2)
                with np.errstate(invalid="ignore"):
                    m = np.minimum.reduce([uu, vv, 1.0 - uu - vv, s, 1.0 - s])
                margins.append(float(np.nanmin(np.abs(m))) if len(m) else np.inf)
            shadow = shadows and (segment_tree(p, lamp, tree, tris, any_hit=True) if tree is not None
                                  else segment_brute(p, lamp, tris)) is not None
            if not shadow:
                tot += li * li * ndl / d2
        out[i] = (np.ones(3) if tri_rgb is None else np.asarray(tri_rgb, np.float32)[t].astype(np.float64)) * tot
    return out

"""numpy restatement of the observer camera (points 1-4) -- TEST INFRASTRUCTURE ONLY.

An observer at the camera x_c moves with velocity beta relative to the ZAMO there (the static observer in Schwarzschild).
  1. the pinhole direction d / |d| is its rest-frame look direction n';
  2. the received photon p' = -n', E' = 1 is boosted to the ZAMO frame: E = gamma (1 - beta.n'),
     p = -n' + (gamma - 1)(-n'.beta_hat) beta_hat + gamma beta, and n = -p / E;
  3. the ZAMO tetrad turns n into the coordinate 4-vector k = e_t + n^i e_i; its spatial part, put on Cartesian axes, is
     normalised to unit Euclidean length -> k0;
  4. g of the observer = g of the ZAMO * gamma (1 + beta.n).

Written from the formulas, not from the device code: the boost with beta_hat as written (beta = 0 taken apart), the tetrad
legs as 4-vectors of the metric (Schwarzschild-Cartesian g_ij = delta_ij + h r^_i r^_j; Boyer-Lindquist Kerr from
redshift_reference.kerr_metric), the Kerr Cartesian map by the Jacobian of x = R sin th cos ph, y = R sin th sin ph,
z = r cos th.  The inverse (k0 -> n) projects k onto the tetrad with the metric.
"""
import numpy as np

import redshift_reference as rr


def gamma_of(beta):
    beta = np.asarray(beta, float)
    return 1.0 / np.sqrt(1.0 - beta @ beta)


def aberrate(n_prime, beta):
    """Point 2: the rest-frame look direction n' of an observer moving with beta -> the ZAMO-frame look direction n."""
    n_prime = np.asarray(n_prime, float)
    beta = np.asarray(beta, float)
    b = np.linalg.norm(beta)
    if b == 0.0:
        return n_prime.copy()
    bh = beta / b
    g = 1.0 / np.sqrt(1.0 - b * b)
    E = g * (1.0 - beta @ n_prime)
    p = -n_prime + (g - 1.0) * (-(n_prime @ bh)) * bh + g * beta
    return -p / E


def doppler(beta, n):
    """Point 4: the factor of the moving observer on the ZAMO's g, n its ZAMO-frame look direction."""
    return gamma_of(beta) * (1.0 + np.asarray(beta, float) @ np.asarray(n, float))


# ---- Schwarzschild, Cartesian ------------------------------------------------------------------------------------------
def schw_metric(x, r_s):
    """g_tt and the spatial g_ij of the Schwarzschild-Cartesian metric at x."""
    x = np.asarray(x, float)
    r = np.linalg.norm(x)
    rh = x / r
    f = 1.0 - r_s / r
    h = r_s / (r - r_s)
    return -f, np.eye(3) + h * np.outer(rh, rh)


def schw_tetrad(x, r_s):
    """Static-observer tetrad: e_t (4-vector), and the 3 spatial legs e_i (rows, 4-vectors) along the world axes."""
    x = np.asarray(x, float)
    r = np.linalg.norm(x)
    rh = x / r
    f = 1.0 - r_s / r
    # the orthonormal spatial frame of delta + h r^ r^: the radial leg is sqrt(f) r^ (|r^|_g^2 = 1 + h = 1 / f), transverse legs
    # are unchanged: leg_i = e_i - (1 - sqrt f)(e_i.r^) r^
    S = np.eye(3) - (1.0 - np.sqrt(f)) * np.outer(rh, rh)
    et = np.array([1.0 / np.sqrt(f), 0.0, 0.0, 0.0])
    legs = np.hstack([np.zeros((3, 1)), S])
    return et, legs


# ---- Kerr, Boyer-Lindquist ---------------------------------------------------------------------------------------------
def kerr_position(x, a):
    q, _ = rr.kerr_bl_state(x, np.zeros(3), a)
    return q


def kerr_jacobian(q, a):
    r, th, ph = q
    R = np.sqrt(r * r + a * a)
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    return np.array([[r / R * st * cp, R * ct * cp, -R * st * sp],
                     [r / R * st * sp, R * ct * sp, R * st * cp],
                     [ct, -r * st, 0.0]])


def kerr_metric4(q, M, a):
    gtt, gtp, grr, gthth, gpp = rr.kerr_metric(q[0], q[1], M, a)
    g = np.zeros((4, 4))
    g[0, 0], g[0, 3], g[3, 0], g[1, 1], g[2, 2], g[3, 3] = gtt, gtp, gtp, grr, gthth, gpp
    return g


def kerr_tetrad(x, M, a):
    """ZAMO tetrad at the Cartesian camera x: e_t and the legs along the Euclidean (r^, th^, ph^) at the BL angles (rows,
    4-vectors in (t, r, th, ph)), and the BL position."""
    q = kerr_position(x, a)
    g = kerr_metric4(q, M, a)
    alpha, omega = rr.kerr_zamo(q[0], q[1], M, a)
    et = np.array([1.0, 0.0, 0.0, omega]) / alpha
    legs = np.array([[0.0, 1.0 / np.sqrt(g[1, 1]), 0.0, 0.0],
                     [0.0, 0.0, 1.0 / np.sqrt(g[2, 2]), 0.0],
                     [0.0, 0.0, 0.0, 1.0 / np.sqrt(g[3, 3])]])
    # (e_ph = d_ph / sqrt(g_phph): orthogonal to e_t = (d_t + omega d_ph) / alpha since g_tph + omega g_phph = 0)
    return et, legs, q


def spherical_basis(q):
    th, ph = q[1], q[2]
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    return np.array([[st * cp, st * sp, ct], [ct * cp, ct * sp, -st], [-sp, cp, 0.0]])


# ---- points 1-3 --------------------------------------------------------------------------------------------------------
def zamo_k4(x, n, r_s, spin=0.0, kerr=False):
    """The coordinate 4-vector k = e_t + n^i e_i of a ZAMO-frame look direction n (Schwarzschild: (t, x, y, z); Kerr: (t, r, th,
    ph)), and for Kerr the BL position."""
    n = np.asarray(n, float)
    if kerr:
        et, legs, q = kerr_tetrad(x, 0.5 * r_s, spin)
        nb = spherical_basis(q) @ n          # (n_r, n_th, n_ph)
        return et + nb @ legs, q
    et, legs = schw_tetrad(x, r_s)
    return et + n @ legs, None


def k0_of_n(x, n, r_s, spin=0.0, kerr=False):
    """Point 3: the unit Euclidean coordinate direction k0 of a ZAMO-frame look direction n."""
    k4, q = zamo_k4(x, n, r_s, spin, kerr)
    k = kerr_jacobian(q, spin) @ k4[1:] if kerr else k4[1:]
    return k / np.linalg.norm(k)


def observer_k0(x, n_prime, beta, r_s, spin=0.0, kerr=False):
    """Points 1-3: k0 of one ray of rest-frame look direction n'."""
    n_prime = np.asarray(n_prime, float)
    return k0_of_n(x, aberrate(n_prime / np.linalg.norm(n_prime), beta), r_s, spin, kerr)


def observer_k0_rays(x, d, beta, r_s, spin=0.0, kerr=False):
    d = np.asarray(d, float).reshape(-1, 3)
    return np.array([observer_k0(x, di, beta, r_s, spin, kerr) for di in d])


def n_of_k0(x, k0, r_s, spin=0.0, kerr=False):
    """The inverse of point 3: the ZAMO-frame look direction of a camera direction k0 (k^t from the null condition, then the
    projections k.e_i / -k.e_t with the metric)."""
    k0 = np.asarray(k0, float)
    if kerr:
        M = 0.5 * r_s
        q, u = rr.kerr_bl_state(x, k0, spin)
        kt = rr.kerr_kt(q, u, M, spin)
        k4 = np.concatenate([[kt], u])
        g = kerr_metric4(q, M, spin)
        et, legs, _ = kerr_tetrad(x, M, spin)
        E = -(et @ g @ k4)
        nb = np.array([leg @ g @ k4 for leg in legs]) / E
        return spherical_basis(q).T @ nb
    gtt, gij = schw_metric(x, r_s)
    kt = np.sqrt((k0 @ gij @ k0) / -gtt)
    et, legs = schw_tetrad(x, r_s)
    g = np.zeros((4, 4))
    g[0, 0], g[1:, 1:] = gtt, gij
    k4 = np.concatenate([[kt], k0])
    E = -(et @ g @ k4)
    return np.array([leg @ g @ k4 for leg in legs]) / E


def observer_g_rays(x0, k0, end, flags, r_s, beta, spin=0.0, kerr=False, sense=1):
    """Point 4: g of the moving observer for traced rays (as redshift_reference.g_rays, times gamma (1 + beta.n))."""
    g = rr.g_rays(x0, k0, end, flags, r_s, spin, kerr, sense)
    k0 = np.asarray(k0, float).reshape(-1, 3)
    x0 = np.broadcast_to(np.asarray(x0, float), k0.shape)
    out = g.copy()
    for i in range(len(k0)):
        if rr.ray_class(flags[i]) in ("dark", "nan") or not np.isfinite(g[i]):
            continue
        out[i] = g[i] * doppler(beta, n_of_k0(x0[i], k0[i], r_s, spin, kerr))
    return out


# ---- the refusals (include/bhgeo.h, "the observer camera") ----------------------------------------------------------------
def check(x0, beta, r_s, spin=0.0, kerr=False, time_like=0):
    beta = np.asarray(beta, float)
    if not np.all(np.isfinite(beta)) or not beta @ beta < 1.0:
        raise ValueError(f"|beta| must be < 1: {beta}")
    if time_like:
        raise ValueError("time_like = 1")
    M = 0.5 * r_s
    if kerr:
        r = kerr_position(x0, spin)[0]
        if not r > M + np.sqrt(M * M - spin * spin):
            raise ValueError("inside the horizon r_+")
        c = x0[2] / r
        if not r > M + np.sqrt(M * M - spin * spin * c * c):
            raise ValueError("at or inside the ergosurface")
        if x0[0] == 0.0 and x0[1] == 0.0:
            raise ValueError("on the axis")
    elif not np.linalg.norm(x0) > r_s:
        raise ValueError("inside the horizon r_s")

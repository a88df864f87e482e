"""numpy restatement of the redshift of moving and spinning object spheres -- TEST INFRASTRUCTURE ONLY.

DESIGN.md section 14 (include/bhgeo.h, "moving and spinning object spheres").  Sphere j {c, rho} moves with centre velocity v
and angular velocity w (world axes, dx/dt, rad per unit t); its surface point x with V(x) = v + w x (x - c).  M = r_s / 2.

The motion is given in the picture of the received photon, where disk_sense is given.  The formulas contract the TRACED ray k
(redshift_reference's picture): there the emitter moves with -V, and in Kerr relative to the traced ZAMO.  So
  Schwarzschild  u_traced = u^t (d_t - V),                       g = 1 / (sqrt(f_c) u^t (1 + k_i V^i / E))
  Kerr           u_traced = u^t (d_t + omega d_phi - V),         g = O / (u^t (1 - omega b + k_i V^i / E))
with u^t from the metric at the hit (Schwarzschild f - |V|^2 - h (n.V)^2 = 1 / u^t^2; Kerr alpha^2 (1 - beta^2) with the
ZAMO-relative beta^2 = (g_rr V^r^2 + g_thth V^th^2 + g_phph V^ph^2) / alpha^2), and k at the hit from the camera's constants:
Schwarzschild E, L = x_c x k0 (k_r = s_r sqrt(E^2 - f |L|^2 / r^2) / f along n, the rest L x x / r^2); Kerr E, L, Carter Q
(k_r = s_r sqrt(R(r)) / Delta, k_th = s_th sqrt(Theta)); the signs from the end record's direction.

Written from the formulas, not from the device code: the BL components of V come from numpy's solve of the embedding's Jacobian
(redshift_reference.kerr_bl_state), the metric from redshift_reference.kerr_metric.
"""
import numpy as np

import observer_reference as obr
import redshift_reference as rr


def surface_velocity(x, c, v, w):
    return np.asarray(v, float) + np.cross(np.asarray(w, float), np.asarray(x, float) - np.asarray(c, float))


def camera_constants(xc, kc, r_s, spin=0.0, kerr=False):
    """(E, L, Q) of the traced ray: Kerr (E, L_z, Carter Q); Schwarzschild (E, the vector L = x_c x k0, |L|^2)."""
    xc, kc = np.asarray(xc, float), np.asarray(kc, float)
    M = 0.5 * r_s
    if kerr:
        E, L, q = rr.kerr_E_L(xc, kc, M, spin)
        _, u = rr.kerr_bl_state(xc, kc, spin)
        Sig = q[0] ** 2 + spin ** 2 * np.cos(q[1]) ** 2
        kth = Sig * u[1]
        Q = kth ** 2 + np.cos(q[1]) ** 2 * (L ** 2 / np.sin(q[1]) ** 2 - spin ** 2 * E ** 2)
        return E, L, Q
    rc = np.linalg.norm(xc)
    fc, h = 1.0 - r_s / rc, r_s / (rc - r_s)
    nk = xc @ kc / rc
    E = fc * np.sqrt((kc @ kc + h * nk * nk) / fc)
    L = np.cross(xc, kc)
    return E, L, L @ L


def kerr_photon_at(e, d, E, L, Q, M, a):
    """Covariant (k_t, k_r, k_th, k_ph) of the traced ray at the Cartesian point e, signs of k^r, k^th from the direction d."""
    q, u = rr.kerr_bl_state(e, d, a)
    r, th = q[0], q[1]
    Del = r * r - 2.0 * M * r + a * a
    Rr = ((r * r + a * a) * E - a * L) ** 2 - Del * (Q + (L - a * E) ** 2)
    Th = Q + np.cos(th) ** 2 * (a * a * E * E - L * L / np.sin(th) ** 2)
    kr = (-1.0 if u[0] < 0 else 1.0) * np.sqrt(max(Rr, 0.0)) / Del
    kth = (-1.0 if u[1] < 0 else 1.0) * np.sqrt(max(Th, 0.0))
    return np.array([-E, kr, kth, L]), q


def g_moving(xc, kc, e, d, c, v, w, r_s, spin=0.0, kerr=False):
    """g of one object ray ending at e (direction d) on the sphere of centre c moving with (v, w)."""
    M = 0.5 * r_s
    e = np.asarray(e, float)
    V = surface_velocity(e, c, v, w)
    E, L, Q = camera_constants(xc, kc, r_s, spin, kerr)
    if kerr:
        a = spin
        qc, _ = rr.kerr_bl_state(xc, kc, a)
        alc, omc = rr.kerr_zamo(qc[0], qc[1], M, a)
        b = L / E
        O = (1.0 - omc * b) / alc
        k, q = kerr_photon_at(e, d, E, L, Q, M, a)
        _, Vbl = rr.kerr_bl_state(e, V, a)
        _, _, grr, gthth, gpp = rr.kerr_metric(q[0], q[1], M, a)
        al, om = rr.kerr_zamo(q[0], q[1], M, a)
        b2 = (grr * Vbl[0] ** 2 + gthth * Vbl[1] ** 2 + gpp * Vbl[2] ** 2) / al ** 2
        ut = 1.0 / (al * np.sqrt(1.0 - b2))
        kV = k[1] * Vbl[0] + k[2] * Vbl[1] + k[3] * Vbl[2]
        return O / (ut * (1.0 - om * b + kV / E))
    rc = np.linalg.norm(xc)
    fc = 1.0 - r_s / rc
    r = np.linalg.norm(e)
    n = e / r
    f, h = 1.0 - r_s / r, r_s / (r - r_s)
    ut = 1.0 / np.sqrt(f - V @ V - h * (n @ V) ** 2)
    sr = -1.0 if e @ np.asarray(d, float) < 0 else 1.0
    kr = sr * np.sqrt(max(E * E - f * (L @ L) / r ** 2, 0.0)) / f
    kV = kr * (n @ V) + L @ np.cross(e, V) / r ** 2
    return 1.0 / (np.sqrt(fc) * ut * (1.0 + kV / E))


def g_rays_motion(x0, k0, end, flags, obj, spheres, v, w, r_s, spin=0.0, kerr=False, sense=1, beta=None):
    """g [n] of traced rays with moving spheres: object rays on a sphere with a nonzero v or w take g_moving, every other ray
    redshift_reference.g_rays (times the observer's gamma (1 + beta.n) with beta)."""
    k0 = np.asarray(k0, float).reshape(-1, 3)
    x0b = np.broadcast_to(np.asarray(x0, float), k0.shape)
    out = rr.g_rays(x0, k0, end, flags, r_s, spin, kerr, sense)
    v, w = np.asarray(v, float).reshape(-1, 3), np.asarray(w, float).reshape(-1, 3)
    for i in range(len(k0)):
        if rr.ray_class(flags[i]) != "object" or end is None:
            continue
        j = int(obj[i])
        if j >= len(v) or not (np.any(v[j] != 0.0) or np.any(w[j] != 0.0)):
            continue
        out[i] = g_moving(x0b[i], k0[i], end[i, 0:3], end[i, 3:6], spheres[j][0:3], v[j], w[j], r_s, spin, kerr)
    if beta is not None:
        for i in range(len(k0)):
            if rr.ray_class(flags[i]) in ("dark", "nan") or not np.isfinite(out[i]):
                continue
            out[i] *= obr.doppler(beta, obr.n_of_k0(x0b[i], k0[i], r_s, spin, kerr))
    return out


# ---- the picture of section 14 --------------------------------------------------------------------------------------------
def kerr_omega(r, th, M, a):
    """The ZAMO's angular velocity in the picture motion is given in: -2 M a r / A (the traced ZAMO's, reversed)."""
    return -rr.kerr_zamo(r, th, M, a)[1]


def kerr_keplerian(r, M, a, sense):
    """The Keplerian angular velocity of sense `sense` in that picture: the section 9 disk's, sense s = -disk_sense reversed."""
    return sense * np.sqrt(M) / (r ** 1.5 - sense * a * np.sqrt(M))


def disk_flow(x, r_s, spin, kerr, sense):
    """The disk's orbital flow of sense `sense` at the point x of the plane z = 0, as the motion V of section 14."""
    x = np.asarray(x, float)
    M = 0.5 * r_s
    z = np.array([0.0, 0.0, 1.0])
    if not kerr:
        R = np.hypot(x[0], x[1])
        return sense * np.sqrt(M / R ** 3) * np.cross(z, x)
    r = np.sqrt(x[0] ** 2 + x[1] ** 2 - spin ** 2)
    return (kerr_keplerian(r, M, spin, sense) - kerr_omega(r, 0.5 * np.pi, M, spin)) * np.cross(z, x)


# ---- the refusals ---------------------------------------------------------------------------------------------------------
def kerr_G(r, M, a):
    Del, R2 = r * r - 2.0 * M * r + a * a, r * r + a * a
    return (R2 * R2 - a * a * Del) / (r * r * np.sqrt(Del))


def kerr_F(r, M, a):
    Del, R2 = r * r - 2.0 * M * r + a * a, r * r + a * a
    return r * Del / R2 ** 1.5


def check(spheres, v, w, r_s, spin=0.0, kerr=False):
    """The refusals of section 14 (ValueError naming the sphere); slots beyond the spheres are not looked at."""
    M, a = 0.5 * r_s, (spin if kerr else 0.0)
    v, w = np.asarray(v, float).reshape(-1, 3), np.asarray(w, float).reshape(-1, 3)
    for j, sp in enumerate(np.asarray(spheres, float).reshape(-1, 4)):
        vj, wj = (v[j] if j < len(v) else np.zeros(3)), (w[j] if j < len(w) else np.zeros(3))
        if not (np.all(np.isfinite(vj)) and np.all(np.isfinite(wj))):
            raise ValueError(f"sphere {j}: v, w must be finite")
        if not (np.any(vj != 0.0) or np.any(wj != 0.0)):
            continue
        c, rho = sp[0:3], sp[3]
        d = np.linalg.norm(c) - rho
        if not kerr:
            if not d > r_s:
                raise ValueError(f"sphere {j}: reaches the horizon")
            if not np.linalg.norm(vj) + np.linalg.norm(wj) * rho < 1.0 - r_s / d:
                raise ValueError(f"sphere {j}: not timelike by the bound")
            continue
        r_lo = np.sqrt(d * d - a * a) if d > abs(a) else 0.0
        if not r_lo > M + np.sqrt(M * M - a * a):
            raise ValueError(f"sphere {j}: reaches the horizon")
        wz, wp = wj[2], np.hypot(wj[0], wj[1])
        D = np.linalg.norm(vj - wz * np.cross([0.0, 0.0, 1.0], c)) + wp * rho
        r_hi = np.linalg.norm(c) + rho
        if not abs(wz) * max(kerr_G(r_lo, M, a), kerr_G(r_hi, M, a)) + D / kerr_F(r_lo, M, a) < 1.0:
            raise ValueError(f"sphere {j}: not timelike by the bound")


def beta2_at(x, V, r_s, spin=0.0, kerr=False):
    """The ZAMO-relative beta^2 of the coordinate velocity V (Kerr: relative to the ZAMO's flow) at x."""
    M = 0.5 * r_s
    if kerr:
        q, Vbl = rr.kerr_bl_state(x, V, spin)
        _, _, grr, gthth, gpp = rr.kerr_metric(q[0], q[1], M, spin)
        al, _ = rr.kerr_zamo(q[0], q[1], M, spin)
        return (grr * Vbl[0] ** 2 + gthth * Vbl[1] ** 2 + gpp * Vbl[2] ** 2) / al ** 2
    r = np.linalg.norm(x)
    f, h = 1.0 - r_s / r, r_s / (r - r_s)
    return (V @ V + h * (x @ V / r) ** 2) / f

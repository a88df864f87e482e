"""numpy restatement of the redshift factor g and of the redshift-weighted shade -- TEST INFRASTRUCTURE ONLY.

g = nu_obs / nu_em = (k.u_obs) / (k.u_em) of a ray between the ZAMO at the camera (the static observer in Schwarzschild)
and its emitter, from the ray's Killing constants at the CAMERA state (include/bhgeo.h, "redshift"):

  Schwarzschild (both Cartesian forms), M = r_s / 2, f = 1 - r_s / r, h = r_s / (r - r_s):
      k^t_c = sqrt((|k0|^2 + h (n.k0)^2) / f_c),  b = L_z / E = (x_c k0_y - y_c k0_x) / (f_c k^t_c)
      disk at R, Omega = s sqrt(M) / R^(3/2):   g = sqrt(1 - 3M/R) / (sqrt(f_c) (1 - Omega b))
      object at r_h (static):                   g = sqrt(f(r_h) / f_c)
      sky (static at infinity):                 g = 1 / sqrt(f_c)
  Kerr, Boyer-Lindquist, spin a:  O = (1 - omega_c b) / alpha_c with the ZAMO's alpha = sqrt(Sigma Delta / A),
      omega = 2 M a r / A, b = L / E;  disk at r_h = sqrt(R^2 - a^2):  g = O / (u^t (1 - Omega b)),
      Omega = s sqrt(M) / (r^(3/2) + s a sqrt(M)), u^t = (r^(3/2) + s a sqrt(M)) / (r^(3/4) sqrt(r^(3/2) - 3M r^(1/2) + 2 s a sqrt(M)));
      object (ZAMO at the hit point): g = O alpha_h / (1 - omega_h b);  sky: g = O.
By flags: horizon / start inside -> 0, NaN flag -> NaN, 128 -> disk, 0x88 -> object, anything else -> sky.
The s in these formulas is MINUS the disk_sense asked for: they contract the TRACED ray k, and the photon the camera receives
runs the traced curve backwards -- by the (t, phi) -> (-t, -phi) symmetry of Kerr with the same E and L along the curve
mirrored in phi, where the asked-for disk is the traced picture's disk of the opposite sense.

Written from the formulas, not from the device code: the Kerr camera conversion here is the textbook one (theta = arccos(z/r),
Jacobian solved by numpy), E and L from the BL metric contracted with k.
"""
import numpy as np

FLAG_HIT_HORIZON, FLAG_START_INSIDE, FLAG_NAN, FLAG_HIT_DISK, FLAG_HIT_OBJECT = 1, 2, 64, 128, 0x88
DISK, OBJECTS, SKY = 1, 2, 4


def photon_orbit(M, a, sense):
    """Boyer-Lindquist radius of the circular photon orbit of this sense (3M for a = 0)."""
    return 2.0 * M * (1.0 + np.cos(2.0 / 3.0 * np.arccos(-sense * a / M)))


def check(r_s, spin=0.0, kerr=False, disk_r_in=None, sense=1, exponent=4.0, apply=DISK | OBJECTS | SKY, time_like=0):
    """The refusals of section 1 (ValueError naming the figure)."""
    if apply & ~(DISK | OBJECTS | SKY):
        raise ValueError(f"apply has bits outside the mask: {apply}")
    if not np.isfinite(exponent):
        raise ValueError(f"exponent is not finite: {exponent}")
    if time_like:
        raise ValueError("time_like = 1")
    if sense not in (1, -1):
        raise ValueError(f"disk_sense {sense}")
    if disk_r_in is not None:
        M, a = 0.5 * r_s, (spin if kerr else 0.0)
        r_in = np.sqrt(max(disk_r_in ** 2 - a * a, 0.0))
        r_ph = photon_orbit(M, a, -sense)
        if not r_in > r_ph:
            raise ValueError(f"disk_r_in {disk_r_in} (BL r {r_in}) is at or inside the photon orbit {r_ph}")


def kerr_bl_state(x, k, a):
    """Cartesian (x = sqrt(r^2 + a^2) sin th cos ph, y = ..., z = r cos th) position / velocity -> BL (r, th, ph), d/dlambda."""
    x = np.asarray(x, float)
    k = np.asarray(k, float)
    rho2 = x[0] ** 2 + x[1] ** 2 + x[2] ** 2
    b = rho2 - a * a
    r = np.sqrt(0.5 * (b + np.sqrt(b * b + 4.0 * a * a * x[2] ** 2)))
    th = np.arccos(x[2] / r)
    ph = np.arctan2(x[1], x[0])
    R = np.sqrt(r * r + a * a)
    st, ct, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    J = np.array([[r / R * st * cp, R * ct * cp, -R * st * sp],
                  [r / R * st * sp, R * ct * sp, R * st * cp],
                  [ct, -r * st, 0.0]])
    return np.array([r, th, ph]), np.linalg.solve(J, k)


def kerr_metric(r, th, M, a):
    """(g_tt, g_tph, g_rr, g_thth, g_phph) of Boyer-Lindquist Kerr."""
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Sig = r * r + a * a * c2
    Del = r * r - 2.0 * M * r + a * a
    return (-(1.0 - 2.0 * M * r / Sig), -2.0 * M * a * r * s2 / Sig, Sig / Del, Sig,
            (r * r + a * a + 2.0 * M * r * a * a * s2 / Sig) * s2)


def kerr_kt(q, u, M, a):
    """k^t from g(k, k) = 0, the future root."""
    gtt, gtp, grr, gthth, gpp = kerr_metric(q[0], q[1], M, a)
    S = grr * u[0] ** 2 + gthth * u[1] ** 2 + gpp * u[2] ** 2
    B = gtp * u[2]
    return (-B - np.sqrt(B * B - gtt * S)) / gtt


def kerr_E_L(x, k, M, a):
    q, u = kerr_bl_state(x, k, a)
    kt = kerr_kt(q, u, M, a)
    gtt, gtp, _, _, gpp = kerr_metric(q[0], q[1], M, a)
    return -(gtt * kt + gtp * u[2]), gtp * kt + gpp * u[2], q


def kerr_zamo(r, th, M, a):
    """(alpha, omega) of the ZAMO at (r, theta)."""
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Sig = r * r + a * a * c2
    Del = r * r - 2.0 * M * r + a * a
    A = (r * r + a * a) ** 2 - a * a * Del * s2
    return np.sqrt(Sig * Del / A), 2.0 * M * a * r / A


def ray_class(fl):
    fl = int(fl)
    if fl & (FLAG_HIT_HORIZON | FLAG_START_INSIDE):
        return "dark"
    if fl & FLAG_NAN:
        return "nan"
    if fl == FLAG_HIT_OBJECT:
        return "object"
    if fl == FLAG_HIT_DISK:
        return "disk"
    return "sky"


def g_one(xc, kc, cls, e, r_s, spin=0.0, kerr=False, sense=1):
    """g of one ray of class cls ("dark", "nan", "disk", "object", "sky"); e = end position (disk / object)."""
    if cls == "dark":
        return 0.0
    if cls == "nan":
        return np.nan
    M, s = 0.5 * r_s, -float(sense)     # (the traced picture's sense: module docstring)
    xc, kc = np.asarray(xc, float), np.asarray(kc, float)
    if kerr:
        a = spin
        E, L, q = kerr_E_L(xc, kc, M, a)
        b = L / E
        al, om = kerr_zamo(q[0], q[1], M, a)
        O = (1.0 - om * b) / al
        if cls == "sky":
            return O
        if cls == "disk":
            r = np.sqrt(e[0] ** 2 + e[1] ** 2 - a * a)
            r32, saM = r ** 1.5, s * a * np.sqrt(M)
            Om = s * np.sqrt(M) / (r32 + saM)
            ut = (r32 + saM) / (r ** 0.75 * np.sqrt(r32 - 3.0 * M * np.sqrt(r) + 2.0 * saM))
            return O / (ut * (1.0 - Om * b))
        qh, _ = kerr_bl_state(e, np.zeros(3), a)
        alh, omh = kerr_zamo(qh[0], qh[1], M, a)
        return O * alh / (1.0 - omh * b)
    rc = np.linalg.norm(xc)
    fc = 1.0 - r_s / rc
    if cls == "sky":
        return 1.0 / np.sqrt(fc)
    if cls == "object":
        return np.sqrt((1.0 - r_s / np.linalg.norm(e)) / fc)
    h = r_s / (rc - r_s)
    nk = xc @ kc / rc
    kt = np.sqrt((kc @ kc + h * nk * nk) / fc)
    b = (xc[0] * kc[1] - xc[1] * kc[0]) / (fc * kt)
    R = np.hypot(e[0], e[1])
    Om = s * np.sqrt(M) / R ** 1.5
    return np.sqrt(1.0 - 3.0 * M / R) / (np.sqrt(fc) * (1.0 - Om * b))


def g_rays(x0, k0, end, flags, r_s, spin=0.0, kerr=False, sense=1):
    """g [n] of n traced rays: x0 [3] or [n, 3], k0 [n, 3], end [n, 6] (or None), flags [n]."""
    k0 = np.asarray(k0, float).reshape(-1, 3)
    x0 = np.broadcast_to(np.asarray(x0, float), k0.shape)
    out = np.empty(len(k0))
    for i in range(len(k0)):
        cls = ray_class(flags[i])
        if cls in ("disk", "object") and end is None:
            out[i] = np.nan
            continue
        out[i] = g_one(x0[i], k0[i], cls, None if end is None else end[i, 0:3], r_s, spin, kerr, sense)
    return out


def shade_scene_redshift(end, flags, obj, n_pixels, samples, sky, g, exponent=4.0, apply=DISK | OBJECTS | SKY, disk=None,
                         disk_tex=None, disk_profile=None, spheres=None, sphere_rgb=None, lamps=None, dirs=None):
    """oracle.shade_reference.shade_scene with each ray's colour weighted by g^exponent when its class is in `apply`; same
    accumulation order.  dirs [n, 3]: a direction-only frame (end = None)."""
    from oracle import shade_reference as sh
    if end is None:
        end = np.concatenate([np.zeros_like(dirs), dirs], 1)
    acc = np.zeros((n_pixels, 3))
    for s in range(samples):
        sl = slice(s * n_pixels, (s + 1) * n_pixels)
        e, f, gs = end[sl], flags[sl], g[sl]
        one = sh.shade_scene(e, f, None if obj is None else obj[sl], n_pixels, 1, sky, disk=disk, disk_tex=disk_tex,
                             disk_profile=disk_profile, spheres=spheres, sphere_rgb=sphere_rgb, lamps=lamps)[:, :3]
        is_disk = (f == FLAG_HIT_DISK) if disk is not None else np.zeros(len(f), bool)
        is_obj = (f == FLAG_HIT_OBJECT) if (spheres is not None and len(spheres)) else np.zeros(len(f), bool)
        is_sky = ~is_disk & ~is_obj & ((f & (FLAG_HIT_HORIZON | FLAG_NAN)) == 0)
        w = np.ones(len(f))
        for m, bit in ((is_disk, DISK), (is_obj, OBJECTS), (is_sky, SKY)):
            if apply & bit:
                w[m] = gs[m] ** exponent
        acc += np.nan_to_num(one * w[:, None])
    return np.concatenate([acc / samples, np.ones((n_pixels, 1))], 1)

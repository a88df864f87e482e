"""numpy restatement of the disk polarisation and a numerical parallel-transport judge -- TEST
INFRASTRUCTURE ONLY.

The model, for the TRACED ray k (future-directed, outgoing from the camera), M = r_s / 2, the sense s = -disk_sense (section 9):
  emitter   u = the Keplerian 4-velocity of sense s at the hit radius (Kerr BL r_h = sqrt(R^2 - a^2)), e_th = d_th / sqrt(g_thth);
            k rebuilt at the equator from the camera's constants (Kerr: E, L_z, Carter Q; Schwarzschild: E and x x k), with only
            the signs of k^r and k^th taken from the end record;
            n_f = (k + (k.u) u) / (-k.u),  mu = |n_f . e_th|,  f^a = g^ab eps_bcde u^c e_th^d k^e,  delta = table(mu)
  Walker-Penrose constant, BL coordinates (at a = 0 Schwarzschild coordinates):
            A = (k^t f^r - k^r f^t) + a sin^2 th (k^r f^ph - k^ph f^r)
            B = [(r^2 + a^2)(k^ph f^th - k^th f^ph) - a (k^t f^th - k^th f^t)] sin th
            kappa = (A - i B)(r - i a cos th)
  screen    n = the ray's look direction in the observer's frame (the ZAMO's; with beta, de-aberrated to the rest frame),
            e_up = normalise(up - (up.n) n), e_left = e_up x n, lifted to 4-vectors of the observer's tetrad (in the traced
            picture the observer moves with -beta: the lift is the boost by -beta, which keeps both legs orthogonal to k_c);
            kappa_em = c_L kappa(k_c, E_left) + c_U kappa(k_c, E_up),  chi = atan2(c_L, c_U) folded into (-pi/2, pi/2].

Written from the formulas, not from the device code: the Schwarzschild camera in its Cartesian layout (the static tetrad of
observer_reference, kappa with x = r n^), Kerr in BL; the emitter's f from the Levi-Civita tensor with sqrt(-g).

The judge (transport_judge) shares no kappa code: it integrates the geodesic and the two screen legs by the parallel-transport
equations in BL coordinates, Christoffel symbols from complex-step derivatives of the metric, scipy DOP853 with theta as the
parameter (the rays it is given run monotonically from the camera down to the equator), and decomposes the emitted f -- built
in an orthonormal fluid frame as z^ x n_f -- on the transported legs.
"""
import itertools

import numpy as np

import observer_reference as orf
import redshift_reference as rr

FLAG_HIT_HORIZON, FLAG_START_INSIDE, FLAG_NAN, FLAG_HIT_DISK = 1, 2, 64, 128


def fold(chi):
    """chi into (-pi/2, pi/2]."""
    chi = np.asarray(chi, float)
    chi = np.where(chi > 0.5 * np.pi, chi - np.pi, chi)
    return np.where(chi <= -0.5 * np.pi, chi + np.pi, chi)


def chi_diff(a, b):
    """|a - b| mod pi."""
    d = np.mod(np.asarray(a, float) - np.asarray(b, float), np.pi)
    return np.minimum(d, np.pi - d)


def degree_of(mu, table):
    table = np.asarray(table, float).ravel()
    if len(table) == 1:
        return float(table[0])
    return float(np.interp(min(max(mu, 0.0), 1.0), np.linspace(0.0, 1.0, len(table)), table))


# ---- metric pieces -----------------------------------------------------------------------------------------------------
def bl_metric4(r, th, M, a):
    gtt, gtp, grr, gthth, gpp = rr.kerr_metric(r, th, M, a)
    g = np.zeros((4, 4))
    g[0, 0], g[0, 3], g[3, 0], g[1, 1], g[2, 2], g[3, 3] = gtt, gtp, gtp, grr, gthth, gpp
    return g


def _levi_civita():
    e = np.zeros((4, 4, 4, 4))
    for p in itertools.permutations(range(4)):
        e[p] = np.linalg.det(np.eye(4)[list(p)])
    return e


LC = _levi_civita()


def kappa_bl(r, th, a, k, f):
    """Walker-Penrose kappa of (k, f), contravariant BL components (t, r, th, ph)."""
    st, ct = np.sin(th), np.cos(th)
    A = (k[0] * f[1] - k[1] * f[0]) + a * st * st * (k[1] * f[3] - k[3] * f[1])
    B = ((r * r + a * a) * (k[3] * f[2] - k[2] * f[3]) - a * (k[0] * f[2] - k[2] * f[0])) * st
    return (A - 1j * B) * (r - 1j * a * ct)


def kappa_schw_cart(x, k, f):
    """kappa at a = 0 in the Cartesian layout x = r n^ of Schwarzschild coordinates: r [(k^t f.n^ - k.n^ f^t) - i n^.(f x k)]."""
    x = np.asarray(x, float)
    r = np.linalg.norm(x)
    n = x / r
    A = k[0] * (n @ f[1:]) - (n @ k[1:]) * f[0]
    B = n @ np.cross(f[1:], k[1:])
    return (A - 1j * B) * r


def keplerian_u(r, M, a, s):
    """Equatorial Keplerian 4-velocity of sense s (BL), contravariant."""
    r32, saM = r ** 1.5, s * a * np.sqrt(M)
    Om = s * np.sqrt(M) / (r32 + saM)
    ut = (r32 + saM) / (r ** 0.75 * np.sqrt(r32 - 3.0 * M * np.sqrt(r) + 2.0 * saM))
    return np.array([ut, 0.0, 0.0, Om * ut])


# ---- the screen --------------------------------------------------------------------------------------------------------
def boost_lift(X, beta):
    """4-components, in the ZAMO's frame, of the rest-frame spatial vector X of an observer moving with `beta`."""
    beta = np.asarray(beta, float)
    b2 = beta @ beta
    if b2 == 0.0:
        return np.concatenate([[0.0], X])
    g = 1.0 / np.sqrt(1.0 - b2)
    L = np.eye(4)
    L[0, 1:] = L[1:, 0] = g * beta
    L[1:, 1:] += (g - 1.0) * np.outer(beta, beta) / b2
    return L @ np.concatenate([[0.0], X])


def screen_legs(n_zamo, up, beta):
    """(e_left, e_up, 4-lifts in the ZAMO frame on world axes) or None when up is along the look direction."""
    beta = np.zeros(3) if beta is None else np.asarray(beta, float)
    n = np.asarray(n_zamo, float)
    if beta @ beta > 0.0:
        n = orf.aberrate(n, -beta)      # the inverse of point 2 of section 10: ZAMO frame -> rest frame
    n = n / np.linalg.norm(n)
    up = np.asarray(up, float)
    w = up - (up @ n) * n
    if not np.linalg.norm(w) > 1e-12 * np.linalg.norm(up):
        return None
    e_up = w / np.linalg.norm(w)
    e_left = np.cross(e_up, n)
    return boost_lift(e_left, -beta), boost_lift(e_up, -beta)


def camera(xc, kc, r_s, spin, kerr, up, beta):
    """The camera side of one ray: (E, L_z, Q, kappa of E_left, kappa of E_up) -- the latter None for a degenerate up."""
    M = 0.5 * r_s
    xc, kc = np.asarray(xc, float), np.asarray(kc, float)
    n = orf.n_of_k0(xc, kc, r_s, spin, kerr)
    if kerr:
        a = spin
        q, w = rr.kerr_bl_state(xc, kc, a)
        kt = rr.kerr_kt(q, w, M, a)
        k4 = np.concatenate([[kt], w])
        g = bl_metric4(q[0], q[1], M, a)
        kl = g @ k4
        E, L = -kl[0], kl[3]
        Q = kl[2] ** 2 + np.cos(q[1]) ** 2 * (-a * a * E * E + L * L / np.sin(q[1]) ** 2)
        legs = screen_legs(n, up, beta)
        if legs is None:
            return E, L, Q, None, None
        et, lg, _ = orf.kerr_tetrad(xc, M, a)
        S = orf.spherical_basis(q)
        out = [X[0] * et + (S @ X[1:]) @ lg for X in legs]
        return E, L, Q, kappa_bl(q[0], q[1], a, k4, out[0]), kappa_bl(q[0], q[1], a, k4, out[1])
    gtt, gij = orf.schw_metric(xc, r_s)
    kt = np.sqrt((kc @ gij @ kc) / -gtt)
    E = -gtt * kt
    Lv = np.cross(xc, kc)
    L, Q = Lv[2], Lv @ Lv - Lv[2] ** 2
    legs = screen_legs(n, up, beta)
    if legs is None:
        return E, L, Q, None, None
    et, lg = orf.schw_tetrad(xc, r_s)
    k4 = np.concatenate([[kt], kc])
    out = [X[0] * et + X[1:] @ lg for X in legs]
    return E, L, Q, kappa_schw_cart(xc, k4, out[0]), kappa_schw_cart(xc, k4, out[1])


def emitter(e, ke, E, L, Q, r_s, a, s):
    """(kappa_em, mu) of a disk ray ending at e (Cartesian) with end direction ke (its signs of k^r and k^th are used)."""
    M = 0.5 * r_s
    R2 = e[0] ** 2 + e[1] ** 2
    r = np.sqrt(R2 - a * a)
    # signs of k^r, k^th at the end: the BL velocity of the end state
    _, w = rr.kerr_bl_state(np.array([e[0], e[1], 0.0]), ke, a)
    sr, sth = np.sign(w[0]) or 1.0, np.sign(w[1]) or 1.0
    Del = r * r - 2.0 * M * r + a * a
    P = (r * r + a * a) * E - a * L
    Rr = max(P * P - Del * (Q + (L - a * E) ** 2), 0.0)
    k = np.array([(-a * (a * E - L) + (r * r + a * a) * P / Del) / (r * r),
                  sr * np.sqrt(Rr) / (r * r),
                  sth * np.sqrt(max(Q, 0.0)) / (r * r),
                  (-(a * E - L) + a * P / Del) / (r * r)])
    g = bl_metric4(r, 0.5 * np.pi, M, a)
    u = keplerian_u(r, M, a, s)
    eth = np.array([0.0, 0.0, 1.0 / np.sqrt(g[2, 2]), 0.0])
    ku = k @ g @ u
    nf = (k + ku * u) / (-ku)
    mu = abs(nf @ g @ eth)
    sqrtg = np.sqrt(-np.linalg.det(g))
    f_low = sqrtg * np.einsum("abcd,b,c,d->a", LC, u, eth, k)
    f = np.linalg.solve(g, f_low)
    return kappa_bl(r, 0.5 * np.pi, a, k, f), mu


def pol_one(xc, kc, fl, end, r_s, spin=0.0, kerr=False, sense=1, table=(0.1,), up=(0.0, 1.0, 0.0), beta=None):
    """(chi, delta, mu) of one traced ray."""
    cls = rr.ray_class(fl)
    if cls == "nan":
        return np.nan, np.nan, np.nan
    if cls != "disk":
        return 0.0, 0.0, 0.0
    if end is None:
        return np.nan, np.nan, np.nan
    a = spin if kerr else 0.0
    E, L, Q, kl, ku = camera(xc, kc, r_s, a, kerr, up, beta)
    kem, mu = emitter(end[0:3], end[3:6], E, L, Q, r_s, a, -float(sense))
    delta = degree_of(mu, table)
    if kl is None:
        return np.nan, delta, mu
    if kem == 0.0:                      # f = 0: the photon leaves along the disk normal, no direction
        return np.nan, delta, mu
    Mx = np.array([[kl.real, ku.real], [kl.imag, ku.imag]])
    cL, cU = np.linalg.solve(Mx, [kem.real, kem.imag])
    return float(fold(np.arctan2(cL, cU))), delta, mu


def pol_rays(x0, k0, end, flags, r_s, spin=0.0, kerr=False, sense=1, table=(0.1,), up=(0.0, 1.0, 0.0), beta=None):
    """chi, delta, mu [n] of n traced rays: x0 [3] or [n, 3], k0 [n, 3], end [n, 6] (or None), flags [n]."""
    k0 = np.asarray(k0, float).reshape(-1, 3)
    x0 = np.broadcast_to(np.asarray(x0, float), k0.shape)
    out = np.empty((3, len(k0)))
    for i in range(len(k0)):
        out[:, i] = pol_one(x0[i], k0[i], flags[i], None if end is None else end[i], r_s, spin, kerr, sense, table, up, beta)
    return out[0], out[1], out[2]


def flat_closed_form(xc, P, up):
    """chi of a flat-space disk point P seen from xc: z^ x n^ (n^ from P to the camera) on the screen of look direction -n^."""
    xc, P, up = (np.asarray(v, float) for v in (xc, P, up))
    look = (P - xc) / np.linalg.norm(P - xc)
    f = np.cross([0.0, 0.0, 1.0], -look)
    w = up - (up @ look) * look
    e_up = w / np.linalg.norm(w)
    e_left = np.cross(e_up, look)
    return float(fold(np.arctan2(f @ e_left, f @ e_up)))


def shade_stokes(rgb_rays, chi, delta, n_pixels, samples):
    """Per-pixel means of (Q_r, Q_g, Q_b, U_r, U_g, U_b) in sample order: Q = delta cos 2chi rgb, U = delta sin 2chi rgb, rays
    with a NaN chi (or NaN delta, or a zero degree) adding nothing.  rgb_rays [S * P, 3]: each ray's final colour."""
    acc = np.zeros((n_pixels, 6))
    ok = np.isfinite(chi) & np.isfinite(delta)
    c2 = np.where(ok, np.cos(2.0 * np.where(ok, chi, 0.0)), 0.0)
    s2 = np.where(ok, np.sin(2.0 * np.where(ok, chi, 0.0)), 0.0)
    d = np.where(ok, delta, 0.0)
    for s in range(samples):
        sl = slice(s * n_pixels, (s + 1) * n_pixels)
        rgb = np.nan_to_num(rgb_rays[sl])
        acc[:, 0:3] += (d[sl] * c2[sl])[:, None] * rgb
        acc[:, 3:6] += (d[sl] * s2[sl])[:, None] * rgb
    return acc / samples


def check(disk_sense=1, table=(0.1,), up=(0.0, 1.0, 0.0), time_like=0):
    """The refusals of the polarisation settings themselves (ValueError naming the figure)."""
    if disk_sense not in (1, -1):
        raise ValueError(f"disk_sense {disk_sense}")
    t = np.asarray(table, float).ravel()
    if not 1 <= len(t) <= 64:
        raise ValueError(f"n_degree {len(t)}")
    if not np.all(np.isfinite(t)) or np.any(t < 0.0) or np.any(t > 1.0):
        raise ValueError("degree outside [0, 1]")
    u = np.asarray(up, float)
    if not np.all(np.isfinite(u)) or not np.any(u != 0.0):
        raise ValueError("up")
    if time_like:
        raise ValueError("time_like = 1")


# ---- the numerical parallel-transport judge -------------------------------------------------------------------------
def _metric_c(r, th, M, a):
    """BL Kerr metric [4, 4] for complex (r, th) arrays of shape [N]: the complex step goes through it."""
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Sig = r * r + a * a * c2
    Del = r * r - 2.0 * M * r + a * a
    g = np.zeros(r.shape + (4, 4), dtype=complex)
    g[:, 0, 0] = -(1.0 - 2.0 * M * r / Sig)
    g[:, 0, 3] = g[:, 3, 0] = -2.0 * M * a * r * s2 / Sig
    g[:, 1, 1] = Sig / Del
    g[:, 2, 2] = Sig
    g[:, 3, 3] = (r * r + a * a + 2.0 * M * r * a * a * s2 / Sig) * s2
    return g


def christoffel(r, th, M, a, h=1e-30):
    """Gamma^a_bc [N, 4, 4, 4] of BL Kerr at real (r, th) [N], by complex-step derivatives of the metric."""
    r = np.asarray(r, float)
    th = np.asarray(th, float)
    g = _metric_c(r + 0j, th + 0j, M, a).real
    dg = np.zeros(r.shape + (4, 4, 4))          # dg[:, c, a, b] = d_c g_ab
    dg[:, 1] = _metric_c(r + 1j * h, th + 0j, M, a).imag / h
    dg[:, 2] = _metric_c(r + 0j, th + 1j * h, M, a).imag / h
    gi = np.linalg.inv(g)
    low = 0.5 * (np.einsum("nbdc->ndbc", dg) + np.einsum("ncdb->ndbc", dg) - dg)   # Gamma_dbc
    return np.einsum("nad,ndbc->nabc", gi, low)


def transport_judge(xc, k0s, r_s, spin, kerr, sense, up, beta=None, rtol=1e-12):
    """For rays k0s [N, 3] from the camera xc that run down to the equator with theta increasing all the way: (chi, mu, end
    records [N, 6]) from the transported screen legs.  Rays whose legs are degenerate are not allowed."""
    from scipy.integrate import solve_ivp

    M, a = 0.5 * r_s, (spin if kerr else 0.0)
    xc = np.asarray(xc, float)
    N = len(k0s)
    y0 = np.zeros((N, 4, 4))                    # [ray][x, k, E_left, E_up][component]
    for i, kc in enumerate(np.asarray(k0s, float)):
        q, w = rr.kerr_bl_state(xc, kc, a)
        kt = rr.kerr_kt(q, w, M, a)
        n = orf.n_of_k0(xc, kc, r_s, a, True)
        legs = screen_legs(n, up, beta)
        et, lg, _ = orf.kerr_tetrad(xc, M, a)
        S = orf.spherical_basis(q)
        y0[i, 0] = [0.0, q[0], q[1], q[2]]
        y0[i, 1] = [kt, w[0], w[1], w[2]]
        y0[i, 2] = legs[0][0] * et + (S @ legs[0][1:]) @ lg
        y0[i, 3] = legs[1][0] * et + (S @ legs[1][1:]) @ lg
    if np.any(y0[:, 1, 2] <= 0.0):
        raise ValueError("the judge takes rays with k^theta > 0 at the camera")
    th0 = y0[0, 0, 2]

    def rhs(th, y):
        Y = y.reshape(N, 4, 4)
        G = christoffel(Y[:, 0, 1], np.full(N, th), M, a)
        k = Y[:, 1]
        d = np.empty_like(Y)
        d[:, 0] = k
        d[:, 1] = -np.einsum("nabc,nb,nc->na", G, k, k)
        d[:, 2] = -np.einsum("nabc,nb,nc->na", G, k, Y[:, 2])
        d[:, 3] = -np.einsum("nabc,nb,nc->na", G, k, Y[:, 3])
        return (d / k[:, 2][:, None, None]).ravel()

    sol = solve_ivp(rhs, (th0, 0.5 * np.pi), y0.ravel(), method="DOP853", rtol=rtol, atol=1e-14)
    if not sol.success:
        raise RuntimeError(sol.message)
    Y = sol.y[:, -1].reshape(N, 4, 4)
    chi, mu, end = np.empty(N), np.empty(N), np.empty((N, 6))
    s = -float(sense)
    for i in range(N):
        r, ph = Y[i, 0, 1], Y[i, 0, 3]
        k, EL, EU = Y[i, 1], Y[i, 2], Y[i, 3]
        g = bl_metric4(r, 0.5 * np.pi, M, a)
        u = keplerian_u(r, M, a, s)
        # an orthonormal fluid frame by Gram-Schmidt from u and the coordinate directions r, th, ph
        basis = [u]
        for c in (1, 2, 3):
            v = np.eye(4)[c]
            for b in basis:
                v = v - (v @ g @ b) / (b @ g @ b) * b
            basis.append(v / np.sqrt(v @ g @ v))
        kf = np.array([-(k @ g @ basis[0])] + [k @ g @ b for b in basis[1:]])   # fluid-frame components (E, p_r, p_th, p_ph)
        nf = kf[1:] / kf[0]
        zf = np.array([0.0, 1.0, 0.0])          # the disk normal: the theta leg
        fs = np.cross(zf, nf)                   # z^ x n_f in the fluid frame's (r, th, ph) legs
        f = fs[0] * basis[1] + fs[1] * basis[2] + fs[2] * basis[3]
        chi[i] = fold(np.arctan2(f @ g @ EL, f @ g @ EU))
        mu[i] = abs(nf[1])
        R = np.sqrt(r * r + a * a)
        J = orf.kerr_jacobian(np.array([r, 0.5 * np.pi, ph]), a)
        end[i, 0:3] = [R * np.cos(ph), R * np.sin(ph), 0.0]
        end[i, 3:6] = J @ k[1:]
    return chi, mu, end


def aim_rays(xc, r_s, n, r_lo, r_hi, seed=0, min_b=3.0):
    """n look directions (unit Euclidean k0) from xc towards disk points at R in [r_lo, r_hi] whose straight line passes
    the hole at least min_b * r_s away and runs away from the axis (the judge's rays)."""
    rng = np.random.default_rng(seed)
    xc = np.asarray(xc, float)
    out = []
    while len(out) < n:
        R, ph = rng.uniform(r_lo, r_hi), rng.uniform(0.0, 2.0 * np.pi)
        P = np.array([R * np.cos(ph), R * np.sin(ph), 0.0])
        d = (P - xc) / np.linalg.norm(P - xc)
        t = -(xc @ d)
        b = np.linalg.norm(xc + max(min(t, np.linalg.norm(P - xc)), 0.0) * d)
        # theta increasing at the camera (then along the whole straight line down to z = 0)
        rho = np.hypot(xc[0], xc[1])
        th_hat = np.array([xc[2] * xc[0] / rho, xc[2] * xc[1] / rho, -rho]) / np.linalg.norm(xc)
        if b > min_b * r_s and d @ th_hat > 0.05:
            out.append(d)
    return np.array(out)

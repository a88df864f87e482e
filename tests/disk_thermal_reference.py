"""numpy restatement of the thermal disk and an independent Page-Thorne judge -- TEST INFRASTRUCTURE ONLY.

The model, M = r_s / 2, s = -disk_sense (section 9's sense), a* = s a / M (a = 0 but for Kerr):
  r       the BL radius of the hit: sqrt(R^2 - a^2), R = sqrt(x^2 + y^2) of the end record
  x       sqrt(r / M);  x0 = sqrt(r_ms / M), r_ms the ISCO of the family (Bardeen-Press-Teukolsky, a* signed)
  x_i     the roots of x^3 - 3x + 2a*: 2 cos(acos(a*)/3 - pi/3), 2 cos(acos(a*)/3 + pi/3), -2 cos(acos(a*)/3)
  c_i     3 (x_i - a*)^2 / (x_i (x_i - x_j)(x_i - x_k)), 0 for a root x_i = 0 (a* = 0, where the term vanishes)
  F^(x)   [x - x0 - (3/2) a* ln(x / x0) - sum_i c_i ln((x - x_i) / (x0 - x_i))] / (x^4 (x^3 - 3x + 2a*)),  0 for r <= r_ms
  tau     (F^ / max F^)^(1/4),  T_em = t_peak tau
  I_c     scale sum_j w_cj nuh_j^3 / (f^4 expm1(nuh_j / (g f tau))),  nuh_j = nu_j h / (k_B t_peak)
flux_hat follows the library's order of operations (it is built with -ffp-contract=off): near r_ms the bracket is a
difference of terms of order (x - x0), and the order of the operations shows there.

The judge (page_thorne_judge) shares nothing with that closed form: the flux of the defining integral
    F ~ -Omega_,r / (E - Omega L)^2 (1 / r) int_{r_ms}^{r} (E - Omega L) L_,r dr
by scipy quad, with E = -u_t, L = u_phi and Omega = u^phi / u^t built from polarisation_reference's Keplerian 4-velocity (the
u^t and Omega of redshift_reference's disk) and redshift_reference's BL metric; r_ms = the minimum of E(r); the derivatives by
complex steps.
"""
import numpy as np

import polarisation_reference as pr
import redshift_reference as rr

H_OVER_K = 4.799243073366221e-11      # h / k_B [K s], exact in the SI
FLAG_NAN, FLAG_HIT_DISK = 64, 128


def isco(astar):
    """r_ms / M of the prograde-in-the-formulas family (Bardeen, Press & Teukolsky 1972), a* signed."""
    z1 = 1.0 + np.cbrt(1.0 - astar * astar) * (np.cbrt(1.0 + astar) + np.cbrt(1.0 - astar))
    z2 = np.sqrt(3.0 * astar * astar + z1 * z1)
    return 3.0 + z2 - (-1.0 if astar < 0.0 else 1.0) * np.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2))


def constants(astar):
    """The closed form's constants of the family a* (units of M): dict(astar, x0, xr, c, r_ms)."""
    r_ms = isco(astar)
    if astar == 0.0:
        xr = np.array([np.sqrt(3.0), 0.0, -np.sqrt(3.0)])
    else:
        th = np.arccos(astar) / 3.0
        xr = np.array([2.0 * np.cos(th - np.pi / 3.0), 2.0 * np.cos(th + np.pi / 3.0), -2.0 * np.cos(th)])
    c = np.zeros(3)
    for i in range(3):
        xi, xj, xk = xr[i], xr[(i + 1) % 3], xr[(i + 2) % 3]
        c[i] = 0.0 if xi == 0.0 else 3.0 * (xi - astar) ** 2 / (xi * (xi - xj) * (xi - xk))
    return dict(astar=float(astar), x0=float(np.sqrt(r_ms)), xr=xr, c=c, r_ms=float(r_ms))


def flux_hat(x, K):
    """F^(x) for x > x0 (array), the library's order of operations."""
    x = np.asarray(x, float)
    x0, a = K["x0"], K["astar"]
    x2 = x * x
    d = x - x0
    b = d - (1.5 * a) * np.log1p(d / x0)
    for i in range(3):
        b = b - K["c"][i] * np.log1p(d / (x0 - K["xr"][i]))
    return b / ((x2 * x2) * ((x2 * x - 3.0 * x) + 2.0 * a))


def flux_hat_parent(x, K):
    """F^(x) as the library formed it before the log1p form: each logarithm of a rounded quotient.  Kept so that the inner-edge
    ladder test can show what it is there to catch."""
    x = np.asarray(x, float)
    x0, a = K["x0"], K["astar"]
    x2 = x * x
    b = (x - x0) - (1.5 * a) * np.log(x / x0)
    for i in range(3):
        b = b - K["c"][i] * np.log((x - K["xr"][i]) / (x0 - K["xr"][i]))
    return b / ((x2 * x2) * ((x2 * x - 3.0 * x) + 2.0 * a))


def flux_hat_mp(x, K, bits=300):
    """F^(x) of ONE double x in mpmath at `bits` bits, from the same double constants x0, x_i, c_i, a* that the library holds (they
    are inputs of the operation, not part of its error).  Returns an mpf."""
    import mpmath as mp
    with mp.workprec(bits):
        x, x0, a = mp.mpf(float(x)), mp.mpf(K["x0"]), mp.mpf(K["astar"])
        b = (x - x0) - mp.mpf(1.5) * a * mp.log(x / x0)
        for i in range(3):
            xi = mp.mpf(float(K["xr"][i]))
            b -= mp.mpf(float(K["c"][i])) * mp.log((x - xi) / (x0 - xi))
        return +(b / (x ** 4 * (x ** 3 - 3 * x + 2 * a)))


def tau_mp(x, K, fmax, bits=300):
    """tau = (F^ / max F^)^(1/4) in mpmath from flux_hat_mp (fmax a double: the normalisation is an input too); an mpf."""
    import mpmath as mp
    with mp.workprec(bits):
        return +mp.root(flux_hat_mp(x, K, bits) / mp.mpf(fmax), 4)


def schwarzschild_flux_hat(x):
    """The a = 0 closed form: [x - sqrt6 - (sqrt3/2) ln((x - sqrt3)(sqrt6 + sqrt3) / ((sqrt6 - sqrt3)(x + sqrt3)))] / (x^4 (x^3 - 3x))."""
    s3, s6 = np.sqrt(3.0), np.sqrt(6.0)
    x = np.asarray(x, float)
    b = x - s6 - 0.5 * s3 * np.log((x - s3) * (s6 + s3) / ((s6 - s3) * (x + s3)))
    return b / (x ** 4 * (x ** 3 - 3.0 * x))


def flux_max(K):
    """max F^ over x > x0: scipy's bounded Brent search after a grid, to the flat top's last bits."""
    from scipy.optimize import minimize_scalar
    x0 = K["x0"]
    xs = x0 * (1.0 + np.linspace(1e-4, 3.0, 4001))
    j = int(np.argmax(flux_hat(xs, K)))
    res = minimize_scalar(lambda x: -flux_hat(x, K), bounds=(xs[max(j - 1, 0)], xs[j + 1]), method="bounded",
                          options=dict(xatol=1e-13))
    return float(max(-res.fun, flux_hat(xs[j], K))), float(res.x)


def family(r_s, spin=0.0, kerr=False, sense=1):
    """(M, a, a*, K, max F^) of a disk of sense `sense` (disk_sense) around the hole."""
    M, a = 0.5 * r_s, (spin if kerr else 0.0)
    astar = -float(sense) * a / M
    K = constants(astar)
    fmax, _ = flux_max(K)
    return M, a, astar, K, fmax


def check(disk_sense=1, nu=(1e14,), weights=((1.0,), (1.0,), (1.0,)), t_peak=1e4, f_col=1.0, scale=1.0, time_like=0):
    """The refusals of the settings themselves (ValueError naming the figure)."""
    if disk_sense not in (1, -1):
        raise ValueError(f"disk_sense {disk_sense}")
    nu = np.atleast_1d(np.asarray(nu, float))
    if not 1 <= len(nu) <= 16:
        raise ValueError(f"n_nu {len(nu)}")
    if not np.all(np.isfinite(nu)) or np.any(nu <= 0.0):
        raise ValueError("nu")
    if not np.all(np.isfinite(np.asarray(weights, float))):
        raise ValueError("weight")
    for name, v in (("t_peak", t_peak), ("f_col", f_col)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(name)
    if not np.isfinite(scale):
        raise ValueError("scale")
    if time_like:
        raise ValueError("time_like = 1")


def thermal_rays(end, flags, g, r_s, spin=0.0, kerr=False, sense=1, t_peak=1e4, nu=(1e14,), weights=((1.0,), (1.0,), (1.0,)),
                 f_col=1.0, scale=1.0):
    """(t_em [n], rgb [n, 3]) of n traced rays: end [n, 6] (or None), flags [n], g [n] the rays' redshift (bhg_redshift_device's).
    Disk rays their own (0 at and inside r_ms), NaN rays and disk rays without an end record NaN, every other ray 0."""
    M, a, astar, K, fmax = family(r_s, spin, kerr, sense)
    r_ms = K["r_ms"] * M
    nuh = np.asarray(nu, float) * (H_OVER_K / t_peak)
    w = np.asarray(weights, float).reshape(3, len(nuh))
    n = len(flags)
    t_em = np.zeros(n)
    rgb = np.zeros((n, 3))
    for i in range(n):
        cls = rr.ray_class(flags[i])
        if cls == "nan" or (cls == "disk" and end is None):
            t_em[i] = np.nan
            rgb[i] = np.nan
            continue
        if cls != "disk":
            continue
        e = end[i]
        r = np.sqrt(e[0] * e[0] + e[1] * e[1] - a * a)
        if not r > r_ms:
            continue
        x = np.sqrt(r / (0.5 * r_s))
        tau = np.sqrt(np.sqrt(max(float(flux_hat(x, K)), 0.0) * (1.0 / fmax)))
        t_em[i] = t_peak * tau
        y = (g[i] * f_col) * tau
        f2 = f_col * f_col
        with np.errstate(over="ignore"):     # (expm1 -> inf: that frequency adds an exact 0, as on the device)
            b = ((nuh * nuh) * nuh) / ((f2 * f2) * np.expm1(nuh / y))
        rgb[i] = scale * (w @ b)
    return t_em, rgb


def shade_thermal(end, flags, obj, n_pixels, samples, sky, g, thermal_rgb, exponent=4.0, apply=0, disk=None, dirs=None, base=None,
                  **scene):
    """The thermal shade: redshift_reference's shade of every ray (objects and sky weighted by g^exponent as `apply` says), with
    each disk ray's colour replaced by its thermal rgb; the per-pixel mean in sample order.  Returns [n_pixels, 4].  base [n, 3]:
    every ray's colour without the thermal disk, given (textured objects, which redshift_reference does not shade)."""
    n = n_pixels * samples
    if base is not None:
        one = np.array(base[:, :3], dtype=np.float64)
    else:
        one = rr.shade_scene_redshift(end, flags, obj, n, 1, sky, g, exponent, apply & ~rr.DISK, disk=disk, dirs=dirs,
                                      **scene)[:, :3].copy()
    if disk is not None and end is not None:
        d = flags == FLAG_HIT_DISK
        one[d] = thermal_rgb[d]
    acc = np.zeros((n_pixels, 3))
    for s in range(samples):
        acc += one[s * n_pixels:(s + 1) * n_pixels]
    return np.concatenate([acc / samples, np.ones((n_pixels, 1))], 1)


# ---- the judge --------------------------------------------------------------------------------------------------------
def _kepler(r, M, a, s):
    """(E, L, Omega) of the Keplerian orbit of sense s at BL r (complex r allowed): from polarisation_reference's u and
    redshift_reference's metric."""
    u = pr.keplerian_u(r, M, a, s)
    gtt, gtp, _, _, gpp = rr.kerr_metric(r, np.pi / 2, M, a)
    u_t = gtt * u[0] + gtp * u[3]
    u_p = gtp * u[0] + gpp * u[3]
    return -u_t, u_p, u[3] / u[0]


def _d(f, r, h=1e-20):
    return np.imag(f(r + 1j * h)) / h


def judge_isco(M, a, sense):
    """r_ms of the disk of this disk_sense: the minimum of the specific energy -u_t of redshift_reference's Keplerian orbit."""
    from scipy.optimize import brentq
    s = -float(sense)
    dE = lambda r: _d(lambda q: _kepler(q, M, a, s)[0], r)
    r_ph = rr.photon_orbit(M, a, s)      # (its argument is the formulas' sense)
    return brentq(dE, r_ph * (1 + 1e-6), 20.0 * M, xtol=1e-15 * M, rtol=1e-15)


def page_thorne_judge(r, M, a, sense, r_ms=None):
    """The defining integral's flux (arbitrary overall factor) at BL radii r (array)."""
    from scipy.integrate import quad
    s = -float(sense)
    if r_ms is None:
        r_ms = judge_isco(M, a, sense)
    E = lambda q: _kepler(q, M, a, s)[0]
    L = lambda q: _kepler(q, M, a, s)[1]
    Om = lambda q: _kepler(q, M, a, s)[2]
    out = []
    for q in np.atleast_1d(r):
        I, _ = quad(lambda t: np.real(E(t) - Om(t) * L(t)) * _d(L, t), r_ms, q, epsabs=0.0, epsrel=1e-13, limit=200)
        den = np.real(E(q) - Om(q) * L(q))
        out.append(-_d(Om, q) / (den * den) / q * I)
    return np.array(out)


def judge_peak(M, a, sense):
    """(r_peak, F_max) of the judge's flux."""
    from scipy.optimize import minimize_scalar
    r_ms = judge_isco(M, a, sense)
    rs = np.linspace(r_ms * 1.01, r_ms * 6.0, 200)
    f = page_thorne_judge(rs, M, a, sense, r_ms)
    j = int(np.argmax(f))
    res = minimize_scalar(lambda q: -page_thorne_judge(q, M, a, sense, r_ms)[0], bounds=(rs[j - 1], rs[j + 1]), method="bounded",
                          options=dict(xatol=1e-12 * M))
    return float(res.x), float(-res.fun)

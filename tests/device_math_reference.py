"""The kernels' hand-written fp64 primitives (csrc/device_math.h, csrc/kerr_start.h) in mpmath, and the measure that compares a
device value with them: ulp_error -- TEST INFRASTRUCTURE ONLY.

  *_mp                the operation itself at PREC bits (120 by default: an ulp of a double is 2^-52 relative, so the reference's
                      own error is below 2^-60 ulp), one mpf (or a tuple of them) per element;
  ulp_error           |got - want| in ulps of the correctly rounded double of want;
  fma_exact / fma_np  the IEEE fused multiply-add: mpmath's exact product and sum rounded once, and the same thing vectorised
                      (Boldo & Melquiond 2008: error-free product and sum, the low parts added with rounding to odd, one final
                      rounding to nearest) -- tests/test_device_math_host.py holds the two bit for bit on hard cases;
  sincos_pi4_fma      sincos_pi4 restated operation by operation.  The device function uses IEEE operations only (rint, multiply,
                      FMA, sign flips), so this IS its arithmetic: the GPU test asserts equality, not closeness;
  atan2_fast_exact_division
                      atan2_fast restated with correctly rounded divisions in place of its two Newton reciprocals: the yardstick
                      the device's bound is derived from (each Newton reciprocal adds at most one ulp);
  kerr_cart_to_bl_mp  the Kerr start conversion.  theta is what the source DEFINES it to be -- the arc cosine of the rounded double
                      quotient z / r, r the rounded double expression -- and everything after that point in high precision.
"""
import mpmath as mp
import numpy as np

PREC = 120
EPS = 2.0 ** -52


# ---- the measure ------------------------------------------------------------------------------------------------------
def split(want):
    """A sequence of mpf -> (hi, lo) float64 arrays: hi the correctly rounded double, lo the rounded remainder."""
    hi = np.array([float(w) for w in want], dtype=np.float64)
    lo = np.array([float(w - mp.mpf(h)) if np.isfinite(h) else 0.0 for w, h in zip(want, hi)], dtype=np.float64)
    return hi, lo


def ulp_error(got, want):
    """|got - want| in ulps of the correctly rounded double of want, per element.  want: a sequence of mpf, or the (hi, lo) pair
    split() makes of one.  A zero reference asks for a zero (of either sign): anything else is inf."""
    hi, lo = want if isinstance(want, tuple) else split(want)
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs((got - hi) - lo) / np.spacing(np.abs(hi))      # (got - hi is exact whenever the two are within a binade)
    err = np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), err)
    return np.where(np.isfinite(got), err, np.inf)


def worst(err, inputs):
    """(max, the input that gives it) for record_property."""
    err = np.asarray(err)
    j = int(np.argmax(err))
    x = np.asarray(inputs)[j]
    return float(err[j]), ([float(v).hex() for v in np.atleast_1d(x)])


# ---- the operations in mpmath -------------------------------------------------------------------------------------------
def _each(f, xs, prec):
    with mp.workprec(prec):
        return [f(mp.mpf(float(x))) for x in np.asarray(xs, dtype=np.float64)]


def rcp_mp(x, prec=PREC):
    return _each(lambda v: 1 / v, x, prec)


def rsqrt_mp(x, prec=PREC):
    return _each(lambda v: 1 / mp.sqrt(v), x, prec)


def sqrt_mp(x, prec=PREC):
    return _each(mp.sqrt, x, prec)


def atan2_mp(y, x, prec=PREC):
    with mp.workprec(prec):
        return [mp.atan2(mp.mpf(float(a)), mp.mpf(float(b))) for a, b in zip(y, x)]


def sincos_mp(x, prec=PREC):
    """(sines, cosines): two lists of mpf.  The working precision carries the cancellation of the reduction: an argument a
    double away from a multiple of pi/2 loses about 60 bits below 1e5."""
    with mp.workprec(prec + 80):
        cs = [mp.cos_sin(mp.mpf(float(v))) for v in np.asarray(x, dtype=np.float64)]
    return [v[1] for v in cs], [v[0] for v in cs]


def rcp3_mp(x, prec=PREC):
    """x [n, 3] -> three lists of mpf."""
    x = np.asarray(x, dtype=np.float64)
    return tuple(rcp_mp(x[:, j], prec) for j in range(3))


# ---- IEEE fused multiply-add ------------------------------------------------------------------------------------------
def fma_exact(a, b, c):
    """RN(a b + c) of three doubles: the exact product and sum in mpmath, rounded once."""
    p = mp.fmul(mp.mpf(float(a)), mp.mpf(float(b)), exact=True)
    return float(mp.fadd(p, mp.mpf(float(c)), prec=53, rounding="n"))


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ah = a * 134217729.0          # Veltkamp split at 2^27 + 1
    ah = ah - (ah - a)
    al = a - ah
    bh = b * 134217729.0
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_np(a, b, c):
    """RN(a b + c) elementwise on float64 arrays, without a wider format (Boldo & Melquiond, "Emulation of FMA and correctly
    rounded sums: proved algorithms using rounding to odd", 2008).  Valid away from overflow and from products below 2^-960 (the
    error-free product's low part must be a normal number); the callers here are orders of magnitude inside."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    s, e = _two_sum(tl, ul)
    # s + e rounded to odd: when inexact, of the two doubles around the exact sum the one whose last mantissa bit is set
    even = (s.view(np.int64) & 1) == 0
    v = np.where((e != 0.0) & even, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
    return th + v


# ---- sincos_pi4, operation by operation ---------------------------------------------------------------------------------
_S = (1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
      8.33333333332248946124e-03, -1.66666666666666324348e-01)
_C = (-1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
      -1.38888888888741095749e-03, 4.16666666666666019037e-02)
PIO2 = (1.5707963267948966, 6.123233995736766e-17, -1.4973849048591698e-33)


def sincos_pi4_fma(x, fma=fma_np, parts=3):
    """(s, c) of float64 x as csrc/kerr_start.h's sincos_pi4 computes them.  parts: how many of the three Cody-Waite parts of pi/2
    the reduction uses (3 is the source; 2 is the mutation the near-multiples set exists to catch)."""
    x = np.asarray(x, dtype=np.float64)
    kf = np.rint(x * 0.63661977236758134308)
    r = x
    for p in PIO2[:parts]:
        r = fma(-kf, p, r)
    z = r * r
    ps = fma(z, _S[0], _S[1])
    for co in _S[2:]:
        ps = fma(z, ps, co)
    sr = fma(r * z, ps, r)
    pc = fma(z, _C[0], _C[1])
    for co in _C[2:]:
        pc = fma(z, pc, co)
    cr = fma(z * z, pc, fma(-0.5, z, 1.0))
    q = kf.astype(np.int64)
    odd = (q & 1) == 1
    ss, cs = np.where(odd, cr, sr), np.where(odd, sr, cr)
    s = np.where((q & 2) != 0, -ss, ss)
    c = np.where(((q + 1) & 2) != 0, -cs, cs)
    return s, c


def near_multiples_of_half_pi(k_max=63662, step=1):
    """For every k with |k| <= k_max (thinned by `step`, 0 and +-k_max always kept) the double nearest to k pi/2 and its two
    neighbours: the worst cases of the reduction, both signs, all four quadrants.  63 662 pi/2 is just above 1e5."""
    k = np.arange(-k_max, k_max + 1, dtype=np.float64)
    if step > 1:
        keep = (np.arange(len(k)) % step == 0) | (np.abs(k) == k_max) | (k == 0.0)
        k = k[keep]
    p, e = _two_prod(k, PIO2[0])
    mid = p + (e + k * PIO2[1])               # (k pi/2 from a double-double product: the nearest double but for near-ties, which
                                              #  the two neighbours cover)
    return np.concatenate([np.nextafter(mid, -np.inf), mid, np.nextafter(mid, np.inf)])


# ---- atan2_fast with correctly rounded divisions ------------------------------------------------------------------------
_AT1 = (1.62858201153657823623e-02, 4.97687799461593236017e-02, 6.66107313738753120669e-02, 9.09088713343650656196e-02,
        1.42857142725034663711e-01, 3.33333333333329318027e-01)
_AT2 = (-3.65315727442169155270e-02, -5.83357013379057348645e-02, -7.69187620504482999495e-02, -1.11111104054623557880e-01,
        -1.99999999998764832476e-01)


def atan2_fast_exact_division(y, x, fma=fma_np, lead=_AT1[5]):
    """csrc/device_math.h's atan2_fast with q = mn / mx and t = num / den as IEEE divisions in place of the Newton reciprocals.
    lead: the leading coefficient 1/3 - 4e-15 of the polynomial (a test passes a wrong one to show that the measure sees it)."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.fmax(ax, ay), np.fmin(ax, ay)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(mx > 0.0, mn / mx, 0.0)
    r0, r1 = q < 0.4375, q < 0.6875
    num = np.where(r0, q, np.where(r1, fma(2.0, q, -1.0), q - 1.0))
    den = np.where(r0, 1.0, np.where(r1, 2.0 + q, q + 1.0))
    hi = np.where(r0, 0.0, np.where(r1, 4.63647609000806093515e-01, 7.85398163397448278999e-01))
    lo = np.where(r0, 0.0, np.where(r1, 2.26987774529616870924e-17, 3.06161699786838301793e-17))
    t = num / den
    z = t * t
    w = z * z
    s1 = fma(w, _AT1[0], _AT1[1])
    for co in _AT1[2:5]:
        s1 = fma(w, s1, co)
    s1 = fma(w, s1, lead) * z
    s2 = fma(w, _AT2[0], _AT2[1])
    for co in _AT2[2:]:
        s2 = fma(w, s2, co)
    s2 = s2 * w
    r = hi - ((t * (s1 + s2) - lo) - t)
    r = np.where(ay > ax, 1.5707963267948966 - r, r)
    r = np.where(x < 0.0, 3.141592653589793 - r, r)
    return np.where(y < 0.0, -r, r)


# ---- the Kerr start conversion ------------------------------------------------------------------------------------------
def kerr_r_and_quotient(a, x):
    """(r, c = z / r) as the source forms them: IEEE double operations in the checker's order."""
    x = np.asarray(x, dtype=np.float64)
    rho2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    b = rho2 - a * a
    r = np.sqrt(0.5 * (b + np.sqrt(b * b + 4.0 * a * a * x[2] * x[2])))
    return float(r), float(x[2] / r)


def kerr_metric_mp(r, th, M, a):
    """(g_tt, g_tphi, g_rr, g_thth, g_phph) of Boyer-Lindquist Kerr, mpf."""
    s2, c2 = mp.sin(th) ** 2, mp.cos(th) ** 2
    Sig = r * r + a * a * c2
    Del = r * r - 2 * M * r + a * a
    tmr = 2 * M * r / Sig
    return tmr - 1, -tmr * a * s2, Sig / Del, Sig, (r * r + a * a + tmr * a * a * s2) * s2


def kerr_cart_to_bl_mp(a, M, mu2, x, k, prec=200):
    """One start state -> dict of mpf: r, theta, phi, dr, dtheta, dphi, E, L, sin_theta, cos_theta, R, D and the sums of the
    magnitudes of the terms E and L are made of (E_scale, L_scale: what their errors are measured against).  r and the quotient
    z / r are the source's rounded doubles; theta = acos of that double and everything after it at `prec` bits."""
    r_d, c_d = kerr_r_and_quotient(a, x)
    with mp.workprec(prec):
        a_, M_ = mp.mpf(float(a)), mp.mpf(float(M))
        X = [mp.mpf(float(v)) for v in x]
        K = [mp.mpf(float(v)) for v in k]
        r = mp.mpf(r_d)
        th = mp.acos(mp.mpf(c_d))
        st, ct = mp.sin(th), mp.cos(th)
        R = mp.sqrt(r * r + a_ * a_)
        w = mp.sqrt(X[0] ** 2 + X[1] ** 2)
        cp, sp = X[0] / w, X[1] / w
        D = (r * st) ** 2 + (R * ct) ** 2
        krho = cp * K[0] + sp * K[1]
        u0 = (r * st * krho + R * ct * K[2]) * R / D
        u1 = (R * ct * krho - r * st * K[2]) / D
        u2 = (cp * K[1] - sp * K[0]) / (R * st)
        gtt, gtp, grr, gthth, gpp = kerr_metric_mp(r, th, M_, a_)
        S = grr * u0 ** 2 + gthth * u1 ** 2 + gpp * u2 ** 2 + mp.mpf(float(mu2))
        B = gtp * u2
        kt = (-B - mp.sqrt(B * B - gtt * S)) / gtt
        return dict(r=r, theta=th, phi=mp.atan2(X[1], X[0]), dr=u0, dtheta=u1, dphi=u2, E=-(gtt * kt + gtp * u2),
                    L=gtp * kt + gpp * u2, sin_theta=st, cos_theta=ct, R=R, D=D,
                    E_scale=abs(gtt * kt) + abs(gtp * u2), L_scale=abs(gtp * kt) + abs(gpp * u2))


def kerr_norm_residual(a, M, mu2, out, prec=200):
    """The norm g(k, k) + mu2 of the 4-velocity rebuilt from a device record out = (r, theta, phi, dr, dtheta, dphi, E, L), with
    k^t from E, as (residual, sum of the terms' magnitudes): both floats, evaluated in mpmath so that the check adds no error."""
    with mp.workprec(prec):
        r, th, _, u0, u1, u2, E, _ = [mp.mpf(float(v)) for v in out]
        gtt, gtp, grr, gthth, gpp = kerr_metric_mp(r, th, mp.mpf(float(M)), mp.mpf(float(a)))
        kt = -(E + gtp * u2) / gtt
        terms = [gtt * kt * kt, 2 * gtp * kt * u2, gpp * u2 * u2, grr * u0 * u0, gthth * u1 * u1, mp.mpf(float(mu2))]
        return float(sum(terms)), float(sum(abs(t) for t in terms))


# ---- the point sets (shared by the CPU tests of the restatements and the GPU tests of the device functions) -----------------
BREAKPOINTS = (0.4375, 0.6875, 1.0)


def _octants(mn, mx):
    """(y, x) pairs with min(|x|, |y|) = mn and max = mx in all eight octants."""
    ys, xs = [], []
    for sy in (1.0, -1.0):
        for sx in (1.0, -1.0):
            ys += [sy * mn, sy * mx]
            xs += [sx * mx, sx * mn]
    return np.concatenate(ys), np.concatenate(xs)


def atan2_points(seed=20, n=40000):
    """(y, x): n seeded points -- angle uniform in (-pi, pi], magnitude log-uniform in 1e-6 .. 1e6 -- then q = min / max at the
    breakpoints 0.4375, 0.6875 and 1 and +-8 ulps either side in all eight octants (max = 1, where q is mn itself, and two
    other magnitudes), both axes, and magnitude ratios down to 1e-300."""
    rng = np.random.default_rng(seed)
    ang = -rng.uniform(-np.pi, np.pi, n)
    mag = 10.0 ** rng.uniform(-6.0, 6.0, n)
    ys, xs = [mag * np.sin(ang)], [mag * np.cos(ang)]
    for mx in (1.0, 2.0 ** -17, 3.0e5):
        for b in BREAKPOINTS:
            mn = [b * mx]
            for _ in range(8):
                mn = [np.nextafter(mn[0], -np.inf)] + mn + [np.nextafter(mn[-1], np.inf)]
            mn = np.minimum(np.array(mn), mx)
            y, x = _octants(mn, np.full_like(mn, mx))
            ys.append(y)
            xs.append(x)
    axis = np.array([1e-6, 0.3, 1.0, 7.0, 1e6])
    for s in (1.0, -1.0):
        ys += [np.zeros(5), s * axis]
        xs += [s * axis, np.zeros(5)]
    ratio = np.array([1e-10, 1e-50, 1e-100, 1e-200, 1e-300])
    for mx in (1e-6, 1.0, 1e6):
        y, x = _octants(ratio * mx, np.full(5, mx))
        ys.append(y)
        xs.append(x)
    return np.concatenate(ys), np.concatenate(xs)


def sincos_points(seed=21, n=40000):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1e5, 1e5, n), [0.0, -0.0]])


def positive_points(seed=22, n=20000):
    """Log-uniform in 1e-6 .. 1e6, then the powers of two of that range and their two neighbours."""
    rng = np.random.default_rng(seed)
    p2 = 2.0 ** np.arange(-20, 21)
    return np.concatenate([10.0 ** rng.uniform(-6.0, 6.0, n), [1e-6, 1e6], np.nextafter(p2, 0.0), p2, np.nextafter(p2, np.inf)])


def triple_points(seed=23, n=20000):
    """[n, 3] positive triples from 1e-6 .. 1e6 (the product then lies in 1e-18 .. 1e18, far inside the range), signs mixed."""
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(-6.0, 6.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))

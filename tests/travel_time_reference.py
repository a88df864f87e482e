"""Shared by the travel-time tests (tests/test_travel_time_host.py on the CPU, tests/test_gpu_travel_time.py on the GPU) and by
tests/golden/make_golden_travel_time.py: the scipy restatement of the coordinate time along a ray, the
closed forms it is held to, and the numpy restatement of the retarded layer shade.  Not a test module.

dt_i >= 0 is the Schwarzschild / Boyer-Lindquist coordinate time that elapses along null ray i between its start point and a
point on it.  The integrand is a function of position and the ray's constants only:

    Schwarzschild (both forms):  dt/dlambda = E / (1 - r_s / r),  E = sqrt(f0 (|k0|^2 + h0 (n0.k0)^2)),  f = 1 - r_s / r,
                                 h = r_s / (r - r_s)
    Kerr:                        dt/dlambda = [E ((r^2 + a^2)^2 - Delta a^2 sin^2 theta) - 2 M a r L] / (Sigma Delta)

The solve is scipy.integrate.solve_ivp(..., dense_output=True) on oracle/scipy_reference's right-hand sides with its events
(horizon, exit sphere, the disk plane non-terminal); the quadrature is 6-point Gauss-Legendre per accepted step on the step's own
interpolant (sol.sol.interpolants), summed in step order, the last step running to the terminal event's root only.  The time of
a crossing is the time at the start of its step plus the same rule on [lambda_j, root].  A node at r <= r_hor makes the ray's
time and every later time +inf; so does a horizon ending or a start inside (for the end time only)."""
import numpy as np
from scipy.integrate import solve_ivp

FORM_NAMES = ("christoffel", "reduced", "kerr")
FLAG_HIT_HORIZON, FLAG_START_INSIDE, FLAG_REACHED_END, FLAG_EXITED_SPHERE, FLAG_STEP_TOO_SMALL, FLAG_HIT_DISK = 1, 2, 4, 8, 32, 128
COND = 500.0        # as in tests/test_gpu_parity.py

_x, _w = np.polynomial.legendre.leggauss(6)
GL6_X, GL6_W = 0.5 * (1.0 + _x), 0.5 * _w


def energy_schw(k0, x0, r_s):
    k0, x0 = np.asarray(k0, float), np.asarray(x0, float)
    r0 = np.sqrt(x0 @ x0)
    f0, h0 = 1.0 - r_s / r0, r_s / (r0 - r_s)
    nk = (x0 @ k0) / r0
    return np.sqrt(f0 * (k0 @ k0 + h0 * nk * nk))


def rate_schw(pos, E, r_s):
    """(dt/dlambda, r) at Cartesian positions pos [..., 3]."""
    r = np.sqrt((np.asarray(pos) ** 2).sum(-1))
    return E / (1.0 - r_s / r), r


def rate_kerr(r, th, E, L, M, a):
    r2, a2 = r * r, a * a
    ra, Sig = r2 + a2, r2 + a2 * np.cos(th) ** 2
    Del = ra - 2.0 * M * r
    return (E * (ra * ra - Del * a2 * np.sin(th) ** 2) - 2.0 * M * a * r * L) / (Sig * Del)


class _Ray:
    """The pieces of one ray's problem that the RK45 solve and the 7-component DOP853 solve share."""

    def __init__(self, k0, x0, rhs_form, r_s, spin, r_exit, disk_plane):
        from oracle import scipy_reference as sr
        self.kerr = rhs_form == 2
        k0, x0 = np.asarray(k0, float), np.asarray(x0, float)
        self.k0, self.x0, self.r_s, self.spin = k0, x0, r_s, spin
        if self.kerr:
            # (scipy_reference's own Kerr solve has no exit sphere; the solves below carry one as an event on Boyer-Lindquist r)
            M, a = 0.5 * r_s, spin
            fn = sr.kerr_rhs_lambdified()
            q0, u0 = sr.cart_to_bl(x0, k0, a)
            self.r_hor = (M + np.sqrt(M * M - a * a)) * (1.0 + sr.KERR_HORIZON_MARGIN)
            self.inside = q0[0] <= self.r_hor
            E, L, _ = sr.kerr_constants(q0, u0, M, a, 0.0)
            self.E, self.L = E, L
            self.y0 = np.array([u0[0], q0[0], u0[1], q0[1], u0[2], q0[2]])

            def rhs(_t, y):
                ar, ath, aph, _kt = fn(y[1], y[3], y[0], y[2], y[4], E, L, M, a)
                return np.array([ar, y[0], ath, y[2], aph, y[4]])

            def radius(y):
                return y[1]

            def plane(_t, y):
                return np.cos(y[3])

            self.rate = lambda y: rate_kerr(y[1], y[3], E, L, M, a)
        else:
            self.r_hor = r_s
            self.inside = np.sqrt(x0 @ x0) <= r_s
            self.y0 = np.array([k0[0], x0[0], k0[1], x0[1], k0[2], x0[2]])
            rhs = sr.make_rhs(r_s, FORM_NAMES[rhs_form])
            E = self.E = energy_schw(k0, x0, r_s) if not self.inside else np.nan

            def radius(y):
                return np.sqrt(y[1] * y[1] + y[3] * y[3] + y[5] * y[5])

            def plane(_t, y):
                return y[5]

            self.rate = lambda y: E / (1.0 - r_s / radius(y))
        self.rhs, self.radius = rhs, radius
        r_hor = self.r_hor

        def ev_h(_t, y):
            return radius(y) - r_hor

        ev_h.terminal = True
        self.events = [ev_h]
        if r_exit > 0.0:
            def ev_e(_t, y):
                return radius(y) - r_exit

            ev_e.terminal = True
            ev_e.direction = 1.0
            self.events.append(ev_e)
        self.n_terminal = len(self.events)
        if disk_plane:
            self.events.append(plane)

    def cart(self, y):
        from oracle import scipy_reference as sr
        if self.kerr:
            xc, kc = sr.bl_to_cart((y[1], y[3], y[5]), (y[0], y[2], y[4]), self.spin)
            return np.concatenate([xc, kc])
        return np.array([y[1], y[3], y[5], y[0], y[2], y[4]])

    def finish(self, sol):
        """(flags, lambda of the end, state at the end) of a solve, as oracle/scipy_reference reads them."""
        if sol.status == 1:
            te, i_ev = min((sol.t_events[i][-1], i) for i in range(self.n_terminal) if len(sol.t_events[i]) > 0)
            return (FLAG_HIT_HORIZON if i_ev == 0 else FLAG_EXITED_SPHERE), te, sol.y_events[i_ev][-1]
        return (FLAG_REACHED_END if sol.status == 0 else FLAG_STEP_TOO_SMALL), sol.t[-1], sol.y[:, -1]


def _quadrature(ray, interp, t0, w):
    """The rule on [t0, t0 + w] of one step's interpolant; +inf when a node lies at r <= r_hor."""
    s = 0.0
    for xk, wk in zip(GL6_X, GL6_W):
        y = interp(t0 + w * xk)
        if ray.radius(y) <= ray.r_hor:
            return np.inf
        s = s + wk * ray.rate(y)
    return w * s


def solve(k0, x0, rhs_form=0, disk=None, r_s=1.0, spin=0.0, lambda_end=120.0, rtol=1e-3, atol=1e-6, max_step=np.inf, r_exit=0.0, K=4):
    """One ray: dict(end [6], flags, n_attempted, n_accepted, lam_end, n_cross, cross [n_cross, 6], lam_cross, t_end, t_cross
    [n_cross]) -- the disk-off solve of tests/crossings_reference.py with the times.  disk=None: no plane event, no crossings."""
    ray = _Ray(k0, x0, rhs_form, r_s, spin, r_exit, disk is not None)
    out = dict(n_attempted=0, n_accepted=0, lam_end=0.0, n_cross=0, cross=np.zeros((0, 6)), lam_cross=np.zeros(0), t_cross=np.zeros(0))
    if ray.inside:
        out.update(flags=FLAG_START_INSIDE | FLAG_HIT_HORIZON, end=np.concatenate([ray.x0, ray.k0]), t_end=np.inf)
        return out
    sol = solve_ivp(ray.rhs, (0.0, lambda_end), ray.y0, method="RK45", events=ray.events, max_step=max_step, rtol=rtol, atol=atol,
                    dense_output=True)
    flags, te, ye = ray.finish(sol)
    ts, interps = sol.sol.ts, sol.sol.interpolants
    # the time at the start of every step, then at the end
    T = np.zeros(len(ts))
    for j, ip in enumerate(interps):
        T[j + 1] = T[j] + _quadrature(ray, ip, ts[j], ts[j + 1] - ts[j])
    recs, lams, tcs = [], [], []
    if disk is not None:
        for td, yd in zip(sol.t_events[-1], sol.y_events[-1]):
            if not td <= te:
                continue
            q = ray.cart(yd)
            if disk[0] <= np.hypot(q[0], q[1]) <= disk[1]:
                j = min(max(int(np.searchsorted(ts, td, side="left")) - 1, 0), len(interps) - 1)
                recs.append(q)
                lams.append(td)
                tcs.append(T[j] + _quadrature(ray, interps[j], ts[j], td - ts[j]))
    t_end = np.inf if flags & FLAG_HIT_HORIZON else T[-1]
    out.update(flags=flags, end=ray.cart(ye), lam_end=float(te), n_attempted=(int(sol.nfev) - 2) // 6, n_accepted=len(sol.t) - 1,
               n_cross=len(recs), cross=np.array(recs).reshape(-1, 6), lam_cross=np.array(lams), t_cross=np.array(tcs), t_end=t_end)
    return out


def solve_converged(k0, x0, rhs_form=0, r_s=1.0, spin=0.0, lambda_end=120.0, r_exit=0.0, rtol=1e-12, atol=1e-14):
    """The 7-component system (the six of the ray and t) through DOP853: (flags, t at the end)."""
    ray = _Ray(k0, x0, rhs_form, r_s, spin, r_exit, False)
    if ray.inside:
        return FLAG_START_INSIDE | FLAG_HIT_HORIZON, np.inf

    def rhs7(t, y):
        return np.append(ray.rhs(t, y[:6]), ray.rate(y[:6]))

    sol = solve_ivp(rhs7, (0.0, lambda_end), np.append(ray.y0, 0.0), method="DOP853", events=ray.events, rtol=rtol, atol=atol)
    flags, _te, ye = ray.finish(sol)
    return flags, ye[6]


def perturbations(k0):
    """tests/test_gpu_parity.py::_sensitivity's three patterns."""
    eps = np.finfo(float).eps
    return (np.nextafter(k0, np.inf), np.nextafter(k0, -np.inf), k0 * (1.0 + np.array([2.0, -2.0, 2.0]) * eps))


def solve_set(k0, x0, rhs_form, disk, K=4, **par):
    """solve over a ray set with the three perturbations: dict of arrays (t_cross [K, n], NaN where a ray has no such crossing)
    plus S_end [n], S_cross [K, n] -- the largest movement of each time under the perturbations (NaN where the time is not
    finite) -- and stable [n]: flags, step counts, n_cross and which times are finite unchanged under them."""
    k0 = np.atleast_2d(k0)
    n = len(k0)
    x0 = np.asarray(x0, float)
    out = dict(flags=np.zeros(n, np.uint8), n_attempted=np.zeros(n, np.uint32), n_accepted=np.zeros(n, np.uint32),
               n_cross=np.zeros(n, np.uint8), t_end=np.zeros(n), t_cross=np.full((K, n), np.nan), S_end=np.full(n, np.nan),
               S_cross=np.full((K, n), np.nan), stable=np.ones(n, bool))

    def times(r):
        m = min(K, r["n_cross"])
        return np.append(r["t_cross"][:m], r["t_end"])

    for i in range(n):
        xi = x0 if x0.ndim == 1 else x0[i]
        r = solve(k0[i], xi, rhs_form, disk, **par)
        for key in ("flags", "n_attempted", "n_accepted", "n_cross", "t_end"):
            out[key][i] = r[key]
        t = times(r)
        m = len(t) - 1
        out["t_cross"][:m, i] = t[:m]
        S = np.where(np.isfinite(t), 0.0, np.nan)
        for kp in perturbations(k0[i]):
            q = solve(kp, xi, rhs_form, disk, **par)
            tq = times(q)
            if ((q["n_cross"], q["flags"], q["n_attempted"], q["n_accepted"]) != (r["n_cross"], r["flags"], r["n_attempted"], r["n_accepted"])
                    or not np.array_equal(np.isfinite(tq), np.isfinite(t))):
                out["stable"][i] = False
                continue
            with np.errstate(invalid="ignore"):
                S = np.fmax(S, np.where(np.isfinite(t), np.abs(tq - t), np.nan))
        out["S_cross"][:m, i], out["S_end"][i] = S[:m], S[m]
    return out


# ---- closed forms ------------------------------------------------------------------------------------------------------------
def radial_time(r0, r1, r_s=1.0):
    """t along the radial null ray from r0 out to r1: the tortoise coordinate's difference."""
    return (r1 - r0) + r_s * np.log((r1 - r_s) / (r0 - r_s))


# ---- the retarded layer shade ------------------------------------------------------------------------------------------------
def retarded_layer_colours(cross, n_cross, t_cross, phase_rate, max_crossings, disk, disk_tex=None, disk_profile=None, **kw):
    """tests/disk_layers_reference.layer_colours with layer m of ray i coloured at the phase disk_phase - phase_rate * t_cross[m, i];
    a layer whose time is not finite is black (and still absorbs: the compositing is disk_layers_reference.composite's, unchanged).
    The thermal disk has no texture to turn: thermal= is not taken.  Built on the restatement without editing it: the rays of a
    layer are coloured one phase at a time."""
    import disk_layers_reference as dl
    assert kw.get("thermal") is None
    profile = dict(disk_profile or {})
    phase0 = profile.pop("phase", 0.0)
    K = min(int(max_crossings), len(cross))
    n = cross.shape[1]
    out = np.full((K, n, 3), np.nan)
    k0 = kw.pop("k0", None)
    for m in range(K):
        for i in np.flatnonzero(np.asarray(n_cross) > m):
            tm = t_cross[m, i]
            if not np.isfinite(tm):
                out[m, i] = 0.0
                continue
            one = dl.layer_colours(cross[m:m + 1, i:i + 1], np.array([1]), 1, disk, disk_tex=disk_tex,
                                   disk_profile=dict(profile, phase=phase0 - phase_rate * tm),
                                   k0=None if k0 is None else np.asarray(k0)[i:i + 1], **kw)
            out[m, i] = one[0, 0]
    return out

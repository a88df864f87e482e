"""Velocities of common observers for the observer camera (include/bhgeo.h, "the observer camera").

Each helper returns beta: the observer's 3-velocity relative to the ZAMO at the camera (in Schwarzschild the static
observer), on the world axes, as bhg_observer / DeviceFrame.set_observer / Frame.set_observer take it.  M = r_s / 2.
"""
import numpy as np


def circular_orbit_velocity(x0, r_s, spin=0.0, sense=1):
    """A circular equatorial geodesic orbit through x0 (z = 0) of sense +1 (counter-clockwise seen from +z) or -1.

    Schwarzschild (spin = 0): |beta| = sqrt(M / (r - 2M)), 1/2 at r = 6M.  Kerr: the ZAMO-relative speed
    (Omega - omega) sqrt(g_phiphi) / alpha = (Omega - omega) sqrt(A) sin(theta) / (sqrt(Sigma) alpha) with
    Omega = s sqrt(M) / (r^(3/2) + s a sqrt(M)) and r the Boyer-Lindquist radius
    (x^2 + y^2 = r^2 + a^2 in the plane).  Along phi-hat = (-sin phi, cos phi, 0).  Raises ValueError off the plane
    or where the orbit is not timelike (at or inside the circular photon orbit of that sense).  (Kerr prograde orbits exist
    inside the ergosurface r = 2M as well; the library refuses an observer camera there, include/bhgeo.h.)"""
    x, y, z = (float(v) for v in np.asarray(x0, dtype=np.float64).reshape(3))
    if z != 0.0:
        raise ValueError("a circular equatorial orbit needs a camera in the plane z = 0")
    if sense not in (1, -1):
        raise ValueError("sense must be +1 or -1")
    M, a, s = 0.5 * float(r_s), float(spin), float(sense)
    w = np.hypot(x, y)
    r = np.sqrt(w * w - a * a)
    Om = s * np.sqrt(M) / (r ** 1.5 + s * a * np.sqrt(M))
    Sig, Del = r * r, r * r - 2.0 * M * r + a * a
    A = (r * r + a * a) ** 2 - a * a * Del
    alpha, omega = np.sqrt(Sig * Del / A), 2.0 * M * a * r / A
    v = (Om - omega) * np.sqrt(A) / (np.sqrt(Sig) * alpha)
    if not abs(v) < 1.0:
        raise ValueError(f"no timelike circular orbit of sense {sense} at r = {r}: |beta| = {abs(v)}")
    return v * np.array([-y / w, x / w, 0.0])


def radial_infall_velocity(x0, r_s):
    """Schwarzschild radial free fall from rest at infinity: beta = -sqrt(2M / r) r-hat (inward), |beta| < 1 outside r_s."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(3)
    r = float(np.linalg.norm(x0))
    if not r > float(r_s):
        raise ValueError(f"the camera (r = {r}) must lie outside the horizon r_s = {r_s}")
    return -np.sqrt(float(r_s) / r) * x0 / r


def circular_orbit_motion(center, r_s, spin=0.0, sense=1, normal=(0.0, 0.0, 1.0), locked=True):
    """(v, w) of an object sphere whose centre runs on a circular geodesic through `center`, as DeviceFrame.set_object_motion /
    Frame.set_object_motion / bhg_object_motion take them: v the centre's coordinate velocity dx/dt,
    w the body's angular velocity (locked = True: it turns once per orbit, the same face towards the hole; False: w = 0).

    Schwarzschild (spin = 0): any orbit plane through the hole, `normal` its axis, `center` in that plane; Omega =
    sqrt(M / r^3), v = sense Omega n^ x c, w = sense Omega n^ (sense +1: counter-clockwise seen from the tip of n^).
    Kerr (spin != 0): equatorial orbits only (normal along z, center at z = 0; a normal along -z reverses the sense).  In the
    picture the motion is given in (section 14) the Keplerian angular velocity of sense s is Omega_K = s sqrt(M) /
    (r^(3/2) - s a sqrt(M)) and the ZAMO's omega = -2 M a r / A, r the Boyer-Lindquist radius (x^2 + y^2 = r^2 + a^2);
    v = (Omega_K - omega_c) z^ x c relative to the ZAMO's flow, and w = (Omega_K - omega_c) z^ when locked.  A rigid
    rotation is only approximately locked across the body in Kerr: omega varies over the sphere, so its surface moves with
    Omega_K exactly only at the centre's radius.
    Raises ValueError where the orbit is not timelike (at or inside the circular photon orbit of that sense)."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    nrm = np.asarray(normal, dtype=np.float64).reshape(3)
    if sense not in (1, -1):
        raise ValueError("sense must be +1 or -1")
    nn = float(np.linalg.norm(nrm))
    if not nn > 0.0:
        raise ValueError("normal must not be zero")
    n_hat = nrm / nn
    M, a = 0.5 * float(r_s), float(spin)
    R = float(np.linalg.norm(c))
    if abs(float(c @ n_hat)) > 1e-12 * max(R, 1.0):
        raise ValueError("the orbit's centre must lie in the plane through the hole normal to `normal`")
    if a == 0.0:
        if not R > 3.0 * M:
            raise ValueError(f"no timelike circular orbit at r = {R} <= 3M = {3.0 * M}")
        Om = float(sense) * np.sqrt(M / R ** 3)
        v = Om * np.cross(n_hat, c)
        return v, (Om * n_hat if locked else np.zeros(3))
    if abs(n_hat[0]) > 1e-12 or abs(n_hat[1]) > 1e-12:
        raise ValueError("Kerr orbits must be equatorial: normal along z")
    s = float(sense) * (1.0 if n_hat[2] > 0.0 else -1.0)
    r = np.sqrt(R * R - a * a)
    # the photon orbit of this sense in the motion's picture is the traced picture's of sense -s (section 9)
    if not r ** 1.5 - 3.0 * M * np.sqrt(r) - 2.0 * s * a * np.sqrt(M) > 0.0:
        raise ValueError(f"no timelike circular orbit of sense {sense} at Boyer-Lindquist r = {r}")
    Om = s * np.sqrt(M) / (r ** 1.5 - s * a * np.sqrt(M))
    Del = r * r - 2.0 * M * r + a * a
    A = (r * r + a * a) ** 2 - a * a * Del
    omega = -2.0 * M * a * r / A
    z = np.array([0.0, 0.0, 1.0])
    v = (Om - omega) * np.cross(z, c)
    return v, ((Om - omega) * z if locked else np.zeros(3))

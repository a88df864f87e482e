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

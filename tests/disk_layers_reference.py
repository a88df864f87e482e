"""numpy restatement of the layered disk shade (bhg_shade_disk_layers_device, layers_colour under shade_pixels_kernel) --
TEST INFRASTRUCTURE ONLY.

The optically thin disk: a ray that the crossings trace carried through the disk has the records cross[m] of its first crossings;
each crossing passes T = 1 - opacity of what lies behind it.  Per ray, operation by operation as the kernel has it:

    w = 1
    for m in 0 .. min(n_cross, max_crossings) - 1, while w != 0:
        rgb = rgb + w * C(cross[m]);   w = w * T
    if w != 0 and the ray's final flag is not horizon / start-inside:
        rgb = rgb + w * sky(exit direction)

then the samples of a pixel are summed in sample order and divided by S.  `composite` is that and nothing else: it takes the
layers' colours and the colour behind them as arrays.  `layer_colours` / `behind_colour` make those arrays out of the
restatements the tree already has (oracle/shade_reference.py's disk colour and sky, redshift_reference's and
observer_reference's g, disk_thermal_reference's blackbody), fed whatever records the caller has -- the tests feed the DEVICE's.
A layer a ray does not have, or that an opaque layer in front hides, is never looked at: a NaN there does not reach the image.
"""
import numpy as np

FLAG_HIT_HORIZON, FLAG_START_INSIDE, FLAG_HIT_DISK = 1, 2, 128


def layer_flags(n_cross, m):
    """The flag array that goes with cross[m] in the per-ray calls: n_cross > m ? BHG_FLAG_HIT_DISK : BHG_FLAG_HIT_HORIZON."""
    return np.where(np.asarray(n_cross) > m, FLAG_HIT_DISK, FLAG_HIT_HORIZON).astype(np.uint8)


def composite(layer_rgb, n_cross, max_crossings, opacity, behind_rgb, flags, n_pixels, samples):
    """layer_rgb [K, n, 3], n_cross [n], behind_rgb [n, 3] (the sky in the exit direction, weighted as the caller wants it),
    flags [n] the rays' final flags, n = samples * n_pixels -> rgba [n_pixels, 4]."""
    n_cross = np.asarray(n_cross).astype(np.int64)
    flags = np.asarray(flags)
    n = len(flags)
    T = 1.0 - float(opacity)
    rgb = np.zeros((n, 3))
    w = np.ones(n)
    for m in range(min(int(max_crossings), len(layer_rgb))):
        act = (n_cross > m) & (w != 0.0)
        rgb[act] = rgb[act] + w[act, None] * np.asarray(layer_rgb[m])[act]
        w[act] = w[act] * T
    sky = (w != 0.0) & ((flags & (FLAG_HIT_HORIZON | FLAG_START_INSIDE)) == 0)
    rgb[sky] = rgb[sky] + w[sky, None] * np.asarray(behind_rgb)[sky]
    acc = np.zeros((n_pixels, 3))
    for s in range(samples):
        acc += rgb[s * n_pixels:(s + 1) * n_pixels]
    return np.concatenate([acc / samples, np.ones((n_pixels, 1))], 1)


def _g(x0, k0, end, flags, r_s, spin, kerr, sense, beta):
    import observer_reference as obr
    import redshift_reference as rr
    if beta is not None:
        return obr.observer_g_rays(x0, k0, end, flags, r_s, beta, spin=spin, kerr=kerr, sense=sense)
    return rr.g_rays(x0, k0, end, flags, r_s, spin=spin, kerr=kerr, sense=sense)


def layer_colours(cross, n_cross, max_crossings, disk, x0=None, k0=None, r_s=1.0, spin=0.0, kerr=False, disk_tex=None,
                  disk_profile=None, redshift=None, beta=None, thermal=None):
    """C(cross[m]) of every ray that has a layer m, NaN where it has none: [K, n, 3].
    redshift: None, or dict(apply=, exponent=, sense=) -- the disk colour times g^exponent when apply has the disk bit;
    beta: the observer's velocity (g is then the moving observer's); thermal: None, or disk_thermal_reference.thermal_rays'
    keyword arguments (sense, t_peak, nu, weights, f_col, scale) -- the colour is then the thermal one, g already in it."""
    import disk_thermal_reference as dt
    import redshift_reference as rr
    from oracle import shade_reference as sh
    K = min(int(max_crossings), len(cross))
    n = cross.shape[1]
    out = np.full((K, n, 3), np.nan)
    for m in range(K):
        has = np.asarray(n_cross) > m
        if not has.any():
            continue
        e = cross[m][has]
        fl = np.full(int(has.sum()), FLAG_HIT_DISK, np.uint8)
        kk = None if k0 is None else np.asarray(k0)[has]
        if thermal is not None:
            g = _g(x0, kk, e, fl, r_s, spin, kerr, thermal.get("sense", 1), beta)
            out[m][has] = dt.thermal_rays(e, fl, g, r_s, spin=spin, kerr=kerr, **thermal)[1]
            continue
        c = sh.disk_colour(e, disk[0], disk[1], disk_tex, **(disk_profile or {}))
        if redshift is not None and redshift["apply"] & rr.DISK:
            g = _g(x0, kk, e, fl, r_s, spin, kerr, redshift.get("sense", 1), beta)
            c = c * (g ** redshift["exponent"])[:, None]
        out[m][has] = c
    return out


def behind_colour(end, flags, sky, x0=None, k0=None, r_s=1.0, spin=0.0, kerr=False, redshift=None, beta=None):
    """What lies behind the disk: the sky in the ray's exit direction (black for a ray that ended in the hole), weighted by
    g^exponent when redshift's apply has the sky bit (never for a NaN ray): [n, 3]."""
    import redshift_reference as rr
    from oracle import shade_reference as sh
    n = len(flags)
    if redshift is None or not redshift["apply"] & rr.SKY:
        return sh.shade_reduce(end, flags, n, 1, sky)[:, :3]
    g = _g(x0, k0, None, flags, r_s, spin, kerr, redshift.get("sense", 1), beta)
    return rr.shade_scene_redshift(end, flags, None, n, 1, sky, g, exponent=redshift["exponent"], apply=rr.SKY)[:, :3]

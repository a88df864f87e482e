"""Disk polarisation without a GPU: the numpy restatement (tests/polarisation_reference.py) against the
numerical parallel-transport judge, the flat limit, Kerr at a = 0, mirror symmetry, the ABI surface and every refusal of the
library (checked before the context, so no device is needed)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import polarisation_reference as pr  # noqa: E402

R_S = 1.0
TABLE = (0.0, 0.35, 0.2, 0.117)


def _lib():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi, _ffi.load()


# ---- the restatement against the transport judge ---------------------------------------------------------------------
CASES = [
    # (kerr, a/M, camera, disk_sense, beta)
    (False, 0.0, (3.0, -20.0, 12.0), 1, None),
    (False, 0.0, (2.0, 12.0, 14.0), -1, (0.3, -0.2, 0.1)),
    (True, 0.9, (3.0, -20.0, 12.0), 1, None),
    (True, 0.9, (-4.0, 15.0, 9.0), -1, (0.3, -0.2, 0.1)),
    (True, 0.45, (10.0, 8.0, 16.0), -1, None),
    (True, 0.45, (-6.0, -14.0, 7.0), 1, (0.3, -0.2, 0.1)),
]


@pytest.mark.parametrize("kerr,aM,xc,sense,beta", CASES)
def test_restatement_matches_transport_judge(kerr, aM, xc, sense, beta):
    spin = aM * 0.5 * R_S
    k0 = pr.aim_rays(xc, R_S, 160, 3.0, 12.0, seed=int(abs(xc[0]) * 10 + sense + 5))
    chi_j, mu_j, end = pr.transport_judge(xc, k0, R_S, spin, kerr, sense, (0.0, 1.0, 0.0), beta)
    flags = np.full(len(k0), pr.FLAG_HIT_DISK)
    chi, delta, mu = pr.pol_rays(xc, k0, end, flags, R_S, spin, kerr, sense, TABLE, (0.0, 1.0, 0.0), beta)
    assert len(k0) >= 150
    assert np.all(np.isfinite(chi))
    assert pr.chi_diff(chi, chi_j).max() < 1e-7
    assert np.abs(mu - mu_j).max() < 1e-9
    # chi covers the screen's directions, not one value
    assert np.ptp(chi) > 1.0


def test_flat_limit_matches_closed_form():
    r_s = 1e-8
    xc = np.array([0.0, -26.0 * np.sin(np.radians(60.0)), 26.0 * np.cos(np.radians(60.0))])
    rng = np.random.default_rng(3)
    R, ph = rng.uniform(2.0, 10.0, 200), rng.uniform(0.0, 2.0 * np.pi, 200)
    P = np.stack([R * np.cos(ph), R * np.sin(ph), np.zeros_like(R)], 1)
    k0 = (P - xc) / np.linalg.norm(P - xc, axis=1)[:, None]
    end = np.concatenate([P, k0], 1)
    for up in ((0.0, 1.0, 0.0), (0.3, 0.9, 0.2)):
        for sense in (1, -1):
            chi, _, _ = pr.pol_rays(xc, k0, end, np.full(200, 128), r_s, 0.0, False, sense, (0.1,), up)
            ref = np.array([pr.flat_closed_form(xc, p, up) for p in P])
            assert pr.chi_diff(chi, ref).max() < 1e-4


def test_kerr_at_zero_spin_is_schwarzschild():
    xc = (3.0, -20.0, 12.0)
    k0 = pr.aim_rays(xc, R_S, 40, 3.0, 12.0, seed=7)
    _, _, end = pr.transport_judge(xc, k0, R_S, 0.0, False, 1, (0.0, 1.0, 0.0))
    fl = np.full(len(k0), 128)
    for beta in (None, (0.3, -0.2, 0.1)):
        a = pr.pol_rays(xc, k0, end, fl, R_S, 0.0, False, 1, TABLE, (0.0, 1.0, 0.0), beta)
        b = pr.pol_rays(xc, k0, end, fl, R_S, 0.0, True, 1, TABLE, (0.0, 1.0, 0.0), beta)
        assert pr.chi_diff(a[0], b[0]).max() < 1e-12
        assert np.abs(a[1] - b[1]).max() < 1e-12 and np.abs(a[2] - b[2]).max() < 1e-12


@pytest.mark.parametrize("kerr,spin", [(False, 0.0), (True, 0.45)])
def test_mirror_symmetry(kerr, spin):
    """x -> -x in camera, ray and up, with disk_sense -> -disk_sense (and, for Kerr, a -> -a: the mirror turns the hole too)
    gives chi -> -chi."""
    xc = np.array([3.0, -20.0, 12.0])
    k0 = pr.aim_rays(xc, R_S, 40, 3.0, 12.0, seed=11)
    _, _, end = pr.transport_judge(xc, k0, R_S, spin, kerr, 1, (0.0, 1.0, 0.0))
    m = np.array([-1.0, 1.0, 1.0])
    up = np.array([0.2, 1.0, 0.1])
    fl = np.full(len(k0), 128)
    a = pr.pol_rays(xc, k0, end, fl, R_S, spin, kerr, 1, TABLE, up)
    b = pr.pol_rays(xc * m, k0 * m, end * np.tile(m, 2), fl, R_S, -spin, kerr, -1, TABLE, up * m)
    assert pr.chi_diff(a[0], -b[0]).max() < 1e-10
    assert np.abs(a[2] - b[2]).max() < 1e-12


def test_classes_and_degenerate_up():
    xc = (3.0, -20.0, 12.0)
    k0 = pr.aim_rays(xc, R_S, 1, 3.0, 12.0, seed=1)[0]
    end = np.concatenate([[5.0, 0.0, 0.0], k0])
    for fl, want in ((1, 0.0), (2, 0.0), (8, 0.0), (4, 0.0), (0x88, 0.0)):
        assert pr.pol_one(xc, k0, fl, end, R_S) == (want, want, want)
    assert all(np.isnan(pr.pol_one(xc, k0, 64, end, R_S)))
    assert all(np.isnan(pr.pol_one(xc, k0, 128, None, R_S)))
    n = pr.orf.n_of_k0(np.array(xc), k0, R_S)          # up along the look direction: no screen
    chi, delta, mu = pr.pol_one(xc, k0, 128, end, R_S, up=n)
    assert np.isnan(chi) and delta == 0.1 and 0.0 <= mu <= 1.0


# ---- the ABI surface -------------------------------------------------------------------------------------------------
def test_exports_and_struct_size():
    f, L = _lib()
    assert L.bhg_polarisation_size() == C.sizeof(f.Polarisation) == 544
    assert L.bhg_version() == f.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for sym in ("bhg_polarisation_size", "bhg_polarisation_device", "bhg_polarisation_host", "bhg_shade_scene_polarised_device"):
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in f.EXPORTS
        getattr(L, sym)
    assert "#define BHG_POLARISATION 1" in header and "#define BHG_POL_TABLE_MAX 64" in header


def test_header_struct_compiles_as_c99_and_cxx(tmp_path):
    f, _ = _lib()
    src = tmp_path / "pol.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bhgeo.h"\n'
                   'int main(void) { bhg_polarisation p = {0}; p.degree[BHG_POL_TABLE_MAX - 1] = 1.0;\n'
                   '  printf("%zu %zu %zu %zu %d %d\\n", sizeof(p), offsetof(bhg_polarisation, n_degree),\n'
                   '         offsetof(bhg_polarisation, up), offsetof(bhg_polarisation, degree), BHG_POLARISATION,\n'
                   '         BHG_POL_TABLE_MAX); return 0; }\n')
    exe = tmp_path / "pol"
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-x", "c++", "-fsyntax-only", str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    P = f.Polarisation
    assert out == [C.sizeof(P), P.n_degree.offset, P.up.offset, P.degree.offset, 1, 64]


def test_make_polarisation():
    f, _ = _lib()
    p = f.make_polarisation(0.25, -1, (0.0, 0.0, 1.0))
    assert (p.disk_sense, p.n_degree, list(p.up), p.degree[0]) == (-1, 1, [0.0, 0.0, 1.0], 0.25)
    p = f.make_polarisation(TABLE)
    assert p.n_degree == 4 and list(p.degree[:4]) == list(TABLE)
    with pytest.raises(ValueError):
        f.make_polarisation(np.zeros(65))


# ---- the refusals (before the context) -------------------------------------------------------------------------------
def _params(rhs=0, spin=0.0, time_like=0, disk=None):
    f, _ = _lib()
    kw = {} if disk is None else dict(disk_r_in=disk[0], disk_r_out=disk[1])
    return f.make_params(r_s=R_S, rhs_form=rhs, spin=spin, time_like=time_like, **kw)


def _pol(**kw):
    f, _ = _lib()
    p = f.make_polarisation(kw.pop("degree", 0.1), kw.pop("disk_sense", 1), kw.pop("up", (0.0, 1.0, 0.0)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _host_rc(p, pol, x0, obs=None):
    f, L = _lib()
    xs = (C.c_double * 3)(*x0)
    k0 = (C.c_double * 3)(0.0, 0.0, -1.0)
    fl = (C.c_uint8 * 1)(128)
    out = (C.c_double * 3)()
    return L.bhg_polarisation_host(None, C.byref(p), C.byref(pol), None if obs is None else C.byref(obs), xs, 1, k0, None, fl, 1,
                                   out, C.cast(C.byref(out, 8), C.POINTER(C.c_double)), None)


def _device_rc(p, pol, x0, obs=None):
    f, L = _lib()
    xs = (C.c_double * 3)(*x0)
    return L.bhg_polarisation_device(None, C.byref(p), C.byref(pol), None if obs is None else C.byref(obs), xs, None, None, None,
                                     None, 16, None, None, None, None)


def _shade_rc(p, pol, x0, obs=None, rs=None, disk=(3.0, 10.0)):
    f, L = _lib()
    sc = f.make_scene(0, 4, 2, disk=disk)
    xs = (C.c_double * 3)(*x0)
    return L.bhg_shade_scene_polarised_device(None, None, None, None, None, 16, 1, C.byref(sc), C.byref(p),
                                              None if rs is None else C.byref(rs), None if obs is None else C.byref(obs), None, xs,
                                              None, None, None, None, C.byref(pol), None, None)


REFUSALS = [
    (dict(), dict(disk_sense=0), (3.0, 0.0, 20.0), "disk_sense"),
    (dict(), dict(disk_sense=2), (3.0, 0.0, 20.0), "disk_sense"),
    (dict(), dict(n_degree=0), (3.0, 0.0, 20.0), "n_degree"),
    (dict(), dict(n_degree=65), (3.0, 0.0, 20.0), "n_degree"),
    (dict(), dict(degree=(0.1, np.nan)), (3.0, 0.0, 20.0), "degree[1]"),
    (dict(), dict(degree=(0.1, 1.5)), (3.0, 0.0, 20.0), "degree[1]"),
    (dict(), dict(degree=-0.1), (3.0, 0.0, 20.0), "degree[0]"),
    (dict(), dict(up=(0.0, 0.0, 0.0)), (3.0, 0.0, 20.0), "up"),
    (dict(), dict(up=(0.0, np.inf, 0.0)), (3.0, 0.0, 20.0), "up"),
    (dict(time_like=1), dict(), (3.0, 0.0, 20.0), "time_like"),
    (dict(disk=(1.4, 10.0)), dict(), (3.0, 0.0, 20.0), "photon"),
    (dict(), dict(), (0.5, 0.0, 0.5), "horizon r_s"),
    (dict(rhs=2, spin=0.45), dict(), (0.0, 0.0, 20.0), "axis"),
    (dict(rhs=2, spin=0.45), dict(), (0.9, 0.0, 0.0), "ergosurface"),
    (dict(rhs=2, spin=0.45), dict(), (0.5, 0.0, 0.1), "horizon r_+"),
]


@pytest.mark.parametrize("call", [_host_rc, _device_rc], ids=["host", "device"])
@pytest.mark.parametrize("pkw,polkw,x0,word", REFUSALS)
def test_library_refuses(call, pkw, polkw, x0, word):
    f, L = _lib()
    assert call(_params(**pkw), _pol(**polkw), x0) == f.E_INVALID
    msg = L.bhg_last_error().decode()
    assert word in msg and "ctx" not in msg, msg


@pytest.mark.parametrize("pkw,polkw,x0,word", [r for r in REFUSALS if r[3] != "photon"])
def test_shade_refuses(pkw, polkw, x0, word):
    f, L = _lib()
    assert _shade_rc(_params(**pkw), _pol(**polkw), x0, disk=(3.0, 10.0)) == f.E_INVALID
    msg = L.bhg_last_error().decode()
    assert word in msg and "ctx" not in msg, msg


def test_shade_refuses_the_disk_and_a_sense_mismatch():
    f, L = _lib()
    assert _shade_rc(_params(), _pol(), (3.0, 0.0, 20.0), disk=(1.4, 10.0)) == f.E_INVALID
    assert "photon" in L.bhg_last_error().decode()
    rs = f.make_redshift(disk_sense=-1)
    assert _shade_rc(_params(), _pol(disk_sense=1), (3.0, 0.0, 20.0), rs=rs) == f.E_INVALID
    assert "differs" in L.bhg_last_error().decode()
    # the same settings with nothing wrong get as far as the missing context
    assert _shade_rc(_params(), _pol(), (3.0, 0.0, 20.0), rs=f.make_redshift(disk_sense=1)) == f.E_INVALID
    assert "ctx" in L.bhg_last_error().decode()
    assert _host_rc(_params(rhs=2, spin=0.45), _pol(), (1e-9, 0.0, 20.0), obs=f.make_observer((0.1, 0.0, 0.0))) == f.E_INVALID
    assert "ctx" in L.bhg_last_error().decode()

"""The deep start-up records without a GPU (BHG_PREFIX_RECORD_DEEP): the radius rule prefix_rho_deep of
csrc/prefix_clearance.h as its own program under the host sanitizers, and the header, the binding and the library agreeing on
the new mode and its limits."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deep_radius_rule_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "prefix_deep_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "prefix_deep_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = dict((ln.split()[0], float(ln.split()[1])) for ln in r.stdout.strip().splitlines())
    assert got["bench_camera"] == 21.75 and got["one_sphere_far"] == 7.25 and got["one_sphere_near"] == 2.0
    assert got["exit_sphere"] == 7.5 and abs(got["small_hole"] - 0.75 * (30.0 - 1e-3)) < 1e-12
    assert (got["call_exit_nearer"], got["call_bench_camera"], got["call_exit_farther"], got["call_disk_nearer"]) == (2.5, 21.75, 21.75, 0.25)
    for name in ("on_plane", "on_horizon", "inside", "nan_origin", "nan_origin_clear", "inf_origin"):
        assert got[name] == 0.0, name


def test_header_binding_and_library_agree_on_the_deep_mode():
    from blackhole_geodesic_calculator_amd import _ffi as f
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name, val in (("BHG_PREFIX_RECORD_DEEP", f.PREFIX_RECORD_DEEP), ("BHG_PREFIX_DEEP_ACCEPTED", f.PREFIX_DEEP_ACCEPTED),
                      ("BHG_PREFIX_DEEP_ATTEMPTS", f.PREFIX_DEEP_ATTEMPTS), ("BHG_PREFIX_K_MAX", f.PREFIX_K_MAX),
                      ("BHG_ABI_VERSION", f.ABI_VERSION)):
        assert re.search(rf"^#define {name} {val}\b", hdr, re.M), name
    assert (f.PREFIX_RECORD_DEEP, f.PREFIX_DEEP_ACCEPTED, f.PREFIX_DEEP_ATTEMPTS, f.PREFIX_K_MAX, f.ABI_VERSION) == (4, 6, 12, 4, 10)
    assert "bhg_prefix_deep_attempts" in f.EXPORTS and re.search(r"\bbhg_prefix_deep_attempts\(", hdr)
    assert f.has_deep_prefix() and f.load().bhg_prefix_deep_attempts() == f.PREFIX_DEEP_ATTEMPTS
    kern = open(os.path.join(ROOT, "blackhole_geodesic_calculator_amd", "csrc", "geodesic_kernels.h")).read()
    assert re.search(r"BHG_PREFIX_DEEP_ACCEPTED_ = 6;", kern) and re.search(r"BHG_PREFIX_DEEP_ATTEMPTS_ = 12;", kern)

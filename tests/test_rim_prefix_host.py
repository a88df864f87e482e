"""The rim start-up records without a GPU (BHG_PREFIX_RECORD_RIM): the radius rule
prefix_rho_rim_call, the test that tells rim records by their rho, and the owners' ladder deep -> wide -> rim (PrefixOwner:
promotion, refusal, shrink, grow) of csrc/prefix_clearance.h as their own program with its own main, plain and once more under the
host sanitizers; the header, the binding and the library agreeing on the new mode and its limits; and the exported decision
function climbing the same ladder."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "prefix_rim_driver.cpp")
WARN = ["-Wall", "-Wextra", "-Werror"]
RIM_RHO = 29.0 * (1.0 - 2.0 ** -10)


def _run(exe, env=None):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict((ln.split()[0], float(ln.split()[1])) for ln in r.stdout.strip().splitlines())


def _check(got):
    assert got["bench_camera"] == RIM_RHO == 28.9716796875 and got["exit_farther"] == RIM_RHO and got["disk_plane_30"] == RIM_RHO
    assert got["bench_camera_reaches"] == 30.0 - RIM_RHO
    assert (got["one_sphere_far"], got["one_sphere_near"], got["one_sphere_behind"]) == (7.25, 2.0, 7.25)
    assert (got["exit_45"], got["disk_nearer"]) == (3.75, 0.25)
    for name in ("nan_origin", "inf_origin", "on_horizon", "inside", "zero_origin"):
        assert got[name] == 0.0, name
    assert (got["owner_rim_call"], got["owner_rho_rim"], got["owner_rho_shrunk"], got["owner_records"]) == (131.0, RIM_RHO, 7.125, 7.0)


def test_rim_radius_rule_and_owner_ladder(tmp_path):
    exe = tmp_path / "prefix_rim"
    subprocess.check_call(["g++", "-std=c++17", "-O2", *WARN, DRIVER, "-o", str(exe)])
    _check(_run(exe))


def test_rim_radius_rule_and_owner_ladder_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "prefix_rim_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", *WARN, DRIVER, "-o", str(exe)])
    _check(_run(exe, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                              UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")))


def test_header_binding_and_library_agree_on_the_rim_mode():
    from blackhole_geodesic_calculator_amd import _ffi as f
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    for name, val in (("BHG_PREFIX_RECORD_RIM", f.PREFIX_RECORD_RIM), ("BHG_PREFIX_RIM_ACCEPTED", f.PREFIX_RIM_ACCEPTED),
                      ("BHG_PREFIX_RIM_ATTEMPTS", f.PREFIX_RIM_ATTEMPTS), ("BHG_PREFIX_RECORD_WIDE", f.PREFIX_RECORD_WIDE),
                      ("BHG_PREFIX_RECORD_DEEP", f.PREFIX_RECORD_DEEP), ("BHG_PREFIX_REPLAY", f.PREFIX_REPLAY),
                      ("BHG_ABI_VERSION", f.ABI_VERSION)):
        assert re.search(rf"^#define {name} {val}\b", hdr, re.M), name
    # the next free value; 2, 4 and 5 keep their meaning
    assert (f.PREFIX_REPLAY, f.PREFIX_RECORD_DEEP, f.PREFIX_RECORD_WIDE, f.PREFIX_RECORD_RIM) == (2, 4, 5, 6)
    assert (f.PREFIX_RIM_ACCEPTED, f.PREFIX_RIM_ATTEMPTS, f.ABI_VERSION) == (9, 15, 10)
    assert "bhg_prefix_rim_attempts" in f.EXPORTS and re.search(r"\bbhg_prefix_rim_attempts\(", hdr)
    assert f.has_rim_prefix() and f.load().bhg_prefix_rim_attempts() == f.PREFIX_RIM_ATTEMPTS
    kern = open(os.path.join(ROOT, "blackhole_geodesic_calculator_amd", "csrc", "geodesic_kernels.h")).read()
    assert re.search(r"BHG_PREFIX_RIM_ACCEPTED_ = 9;", kern) and re.search(r"BHG_PREFIX_RIM_ATTEMPTS_ = 15;", kern)
    rule = open(os.path.join(ROOT, "blackhole_geodesic_calculator_amd", "csrc", "prefix_clearance.h")).read()
    assert re.search(r"PREFIX_RHO_FRACTION_RIM = 1\.0 - 1\.0 / 1024\.0;", rule) and re.search(r"PREFIX_MODE_RECORD_RIM = 6;", rule)
    assert re.search(r"PREFIX_RIM_ACCEPTED = 9, PREFIX_RIM_ATTEMPTS = 15;", rule)


def test_the_exported_decision_climbs_the_ladder_and_minds_the_step_budget():
    """bhg_prefix_owner_next with promote = BHG_PREFIX_RECORD_RIM, the library's answers played by bhg_prefix_clearance: records by
    the deep rule, the wide rule on the 34th call as without a rim rule, the rim rule on the 131st, replays after it; an exit sphere
    between the wide and the rim ball refuses twice and the third call records by the owner's first rule; under a step budget
    that rim records could exhaust the owner is told to ask for nothing and keeps them."""
    from blackhole_geodesic_calculator_amd import _ffi as f
    cam = [1e-4, 0.0, 30.0]
    free = f.make_params(lambda_end=200.0, max_steps=20000)
    between = f.make_params(lambda_end=200.0, max_steps=20000, r_exit=58.5)      # 28.5 from the camera: wide ball 27.19, rim ball 28.97
    clear = f.prefix_clearance(free, cam)
    R, D, W, M, NO = f.PREFIX_REPLAY, f.PREFIX_RECORD_DEEP, f.PREFIX_RECORD_WIDE, f.PREFIX_RECORD_RIM, f.PREFIX_NONE
    frac = {D: 0.75, W: 0.9375, M: 1.0 - 2.0 ** -10}

    def play(owner, last, scenes, rule=D, promote=M):
        asked = []
        for p in scenes:
            ask = f.prefix_owner_next(owner, rule, p, cam, None, last, promote)
            asked.append(ask)
            c = f.prefix_clearance(p, cam)
            if ask in frac:
                last = f.Prefix(None, (frac[ask] if c == clear else 0.25) * c, ask, ask)
            else:
                last = f.Prefix(None, owner.rho, ask, R if c > owner.rho * (1.0 + 1e-6) else NO)
        return asked, last

    owner = f.PrefixOwner(0.0, 0, 0)
    assert f.prefix_owner_next(owner, D, free, cam, promote=M) == NO
    asked, last = play(owner, f.Prefix(None, 0.75 * clear, D, D), [free] * 134)
    assert asked == [R] * 32 + [W] + [R] * 96 + [M] + [R] * 4
    assert owner.rho == pytest.approx(frac[M] * clear, rel=1e-15) and owner.clean_run == 3
    # the same owner without the last rung: the parent's ladder, call for call
    o2 = f.PrefixOwner(0.0, 0, 0)
    asked2, _ = play(o2, f.Prefix(None, 0.75 * clear, D, D), [free] * 134, promote=W)
    assert asked2 == [R] * 32 + [W] + [R] * 101 and o2.rho == pytest.approx(0.9375 * clear, rel=1e-15)
    # refusal and recovery on rim records
    asked, last = play(owner, last, [between] * 4 + [free] * 10)
    assert asked == [R, R, D, R] + [R] * 8 + [D, R]
    assert owner.rho == pytest.approx(0.75 * clear, rel=1e-15)
    # the step budget: rim records are not asked for at max_steps <= 15, and stay
    owner = f.PrefixOwner(frac[M] * clear, 0, 0, 5)
    tight = f.make_params(lambda_end=200.0, max_steps=f.PREFIX_RIM_ATTEMPTS)
    last = f.Prefix(None, owner.rho, R, R)
    assert f.prefix_owner_next(owner, D, tight, cam, None, last, M) == NO and owner.rho == frac[M] * clear
    assert f.prefix_owner_next(owner, D, f.make_params(lambda_end=200.0, max_steps=16), cam, None, None, M) == R
    wide_owner = f.PrefixOwner(0.9375 * clear, 0, 0, 5)
    assert f.prefix_owner_next(wide_owner, D, f.make_params(lambda_end=200.0, max_steps=13), cam, None, f.Prefix(None, wide_owner.rho, R, R), M) == R
    # bad arguments ask for nothing
    assert f.prefix_owner_next(owner, M, free, cam, promote=R) == NO and f.prefix_owner_next(owner, 7, free, cam) == NO

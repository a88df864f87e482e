"""The C-API layer's two pieces of pure arithmetic without a GPU (csrc/trace_call.h): the cut of a trace call into launches --
at a limit of 64 rays instead of the library's 2^26, which no test can reach -- and the layout of a host-buffer call's arrays in
their one device block, under the host sanitizers (tests/trace_call_driver.cpp says what is checked)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_split_and_staging_layout_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "trace_call_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "trace_call_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    launches, regions, checks = map(int, re.fullmatch(r"launches (\d+) regions (\d+) checks (\d+)\n", r.stdout).groups())
    # 4 kinds x 2 pointer sets x (1 + 1 + 2 + 2 + 3 launches at n = 1, 64, 65, 128, 133); every region list is walked to its end
    assert launches == 4 * 2 * 9 and regions > 4 * 3 * 2 * 30 and checks > 1000


"""Where a mesh object's arrays lie in its device allocations, without a GPU (csrc/mesh_layout.h): the image of the tree and the
triangles -- exact and by capacity, and that the first fits region by region into the second --, the refit's scratch and the
build's storage, under the host sanitizers (tests/mesh_layout_driver.cpp says what is checked)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_layouts_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "mesh_layout_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "mesh_layout_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    images, checks = map(int, re.fullmatch(r"images (\d+) checks (\d+)\n", r.stdout).groups())
    # at least the single-leaf tree and the leaf_size-1 tree of each of the 7 triangle counts (the same tree at nt = 1), with and
    # without normals; 41 checks and more per image, three capacities of 10 regions each on top
    assert images >= (2 * 7 - 1) * 2 and checks > 70 * images

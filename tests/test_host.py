"""CPU tests of the host side: ray generation bit-reproducibility, the C-ABI library loads and
exports every symbol include/bhgeo.h declares, argument validation, loud failure without a GPU.
No compute call is made here."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden


def test_python_random_stream_is_bit_identical():
    from blackhole_geodesic_calculator_amd import python_random_stream
    for seed in (42.0, 42, 7.0, 123456789, 0.5):
        random.seed(seed)
        want = np.array([random.random() for _ in range(2000)])
        got = python_random_stream(seed, 2000)
        assert np.array_equal(want, got)
    assert np.array_equal(python_random_stream(42.0, 8), load_golden("raygen")["first_draws"])


def test_camera_directions_match_reference_loop():
    from blackhole_geodesic_calculator_amd import camera_directions
    g = load_golden("raygen")
    assert np.array_equal(camera_directions(8, 6, 2, 0.6, 0.45, 42.0), g["d_8x6x2"])
    d = camera_directions(5, 7, 3, 1.0, 1.0, 7.0, rotation_euler=(0.3, -0.2, 1.1))
    assert np.abs(d - g["d_5x7x3_rot"]).max() < 5e-16
    d = camera_directions(6, 6, 2, 0.6, 0.6, 42.0, mark=(1, 4, 2, 3))
    assert np.array_equal(np.isnan(d), np.isnan(g["d_6x6x2_mark"]))
    assert np.array_equal(np.nan_to_num(d), np.nan_to_num(g["d_6x6x2_mark"]))
    d = camera_directions(64, 64, 1, 0.6, 0.6, 42.0).reshape(-1, 3)
    assert np.array_equal(d, load_golden("frame64_christoffel")["k0"])
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "bhgeo.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(bhg_[a-z_0-9]+)\s*\(", hdr)))


def test_library_loads_and_exports_every_declared_symbol():
    from blackhole_geodesic_calculator_amd import _ffi
    lib = _ffi.load()
    declared = _declared_symbols()
    assert len(declared) >= 13
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in include/bhgeo.h but not exported"
    assert sorted(_ffi.EXPORTS) == declared
    assert lib.bhg_version() == _ffi.ABI_VERSION


def test_params_struct_layout_and_defaults():
    from blackhole_geodesic_calculator_amd import _ffi
    assert ctypes.sizeof(_ffi.Params) == 104
    p = _ffi.default_params()
    assert (p.r_s, p.lambda_end, p.rtol, p.atol) == (1.0, 50.0, 1e-3, 1e-6)
    assert p.max_step == float("inf") and p.method == _ffi.METHOD_DP54 and p.rhs_form == _ffi.RHS_CHRISTOFFEL


def test_fails_loudly_without_gpu():
    from blackhole_geodesic_calculator_amd import _ffi
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_ffi.BhgError) as ei:
        _ffi.Context(0)
    assert ei.value.code == _ffi.E_NO_DEVICE
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    with pytest.raises(_ffi.BhgError):
        GeodesicIntegratorSchwarzschild(mass=0.5)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(ROOT, "blackhole_geodesic_calculator_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "geodesic_oracle" not in src, f


def test_integrator_argument_checks():
    from blackhole_geodesic_calculator_amd import GeodesicIntegratorSchwarzschild
    with pytest.raises(ValueError):     # the reduced form is the null closed form
        GeodesicIntegratorSchwarzschild(mass=0.5, time_like=True, rhs_form="reduced", context=object())
    tl = GeodesicIntegratorSchwarzschild(mass=0.5, time_like=True, context=object())
    assert tl.time_like is True and tl.params().time_like == 1
    with pytest.raises(ValueError):
        GeodesicIntegratorSchwarzschild(mass=0.5, method="LSODA", context=object())
    gi = GeodesicIntegratorSchwarzschild(mass=0.5, context=object())
    assert gi.r_s == 1.0 and gi.params().time_like == 0
    assert gi.params(max_step=-1).max_step == float("inf")


def test_public_header_is_plain_c(tmp_path):
    """include/bhgeo.h is the C ABI: it must compile as C99 and as C++ with nothing but the standard headers,
    and its struct layouts are what the ctypes mirrors assume."""
    import ctypes
    import subprocess
    from blackhole_geodesic_calculator_amd import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "hdr.c"
    src.write_text('#include <stdio.h>\n#include "bhgeo.h"\n'
                   'int main(void) { printf("%zu %zu %d %d %zu %zu\\n", sizeof(bhg_params), sizeof(bhg_scene), BHG_ABI_VERSION, '
                   'BHG_MAX_SPHERES, sizeof(bhg_frame_scene), sizeof(bhg_camera)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"),
                           str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-x", "c++",
                           "-fsyntax-only", str(src)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert int(out[0]) == ctypes.sizeof(_ffi.Params) == 104
    assert int(out[1]) == ctypes.sizeof(_ffi.Scene)
    assert int(out[2]) == _ffi.ABI_VERSION and int(out[3]) == _ffi.MAX_SPHERES
    assert int(out[4]) == ctypes.sizeof(_ffi.FrameScene) and int(out[5]) == ctypes.sizeof(_ffi.Camera)


def test_c_example_builds_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/trace_frame.c links against libbhgeo.so from plain C; without a device it must stop with the
    no-device message (exit code 3), never produce results."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "blackhole_geodesic_calculator_amd")
    exe = tmp_path / "trace_frame"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "trace_frame.c"), "-L", libdir, "-lbhgeo",
                           "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)])
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the example would run")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stderr and r.stdout == ""


def test_frame_object_host_side():
    """The library-owned frame (bhg_frame_*): its tile dealing is dist.py's (cyclic; by cost ranking, visited longest
    first or row-major -- ties included), argument errors come before any device is touched, and without a device the
    constructor fails loudly."""
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd import dist as bdist
    rng = np.random.default_rng(3)
    for W, H, T, world in ((100, 70, 32, 3), (64, 64, 8, 4), (33, 17, 16, 2), (256, 192, 32, 8), (40, 40, 64, 2)):
        tx, ty = bdist.tile_grid(W, H, T)
        table = rng.integers(0, 40, tx * ty).astype(np.float64)      # (many ties: the sort must be stable like numpy's)

        def tcost(cx, cy):
            return table[int(cy // T) * tx + int(cx // T)]
        seen = np.zeros(W * H, dtype=int)
        for r in range(world):
            a = _ffi.deal_tiles(W, H, T, world, r)
            assert np.array_equal(a, bdist.rank_pixels(W, H, T, r, world))
            seen[a] += 1
            for visit in ("cost", "row"):
                tcost.visit = visit
                assert np.array_equal(_ffi.deal_tiles(W, H, T, world, r, table, visit == "cost"),
                                      bdist.rank_pixels(W, H, T, r, world, tile_cost=tcost))
        assert np.all(seen == 1)                                       # a partition of the frame
        # rank 0 dealt a smaller part (it also assembles the frame): still a partition, the same lists from C++ and Python
        for share in (0.9, 0.5):
            tcost.visit, tcost.root_share = "cost", share
            seen[:] = 0
            sizes = []
            for r in range(world):
                a = _ffi.deal_tiles(W, H, T, world, r, table, True, share)
                assert np.array_equal(a, bdist.rank_pixels(W, H, T, r, world, tile_cost=tcost))
                seen[a] += 1
                sizes.append(len(a))
            assert np.all(seen == 1) and (tx * ty < 4 * world or sizes[0] <= max(sizes[1:]))
        del tcost.root_share
    seq = bdist.deal_sequence(8000, 8, 0.9)
    counts = np.bincount(seq, minlength=8)
    assert abs(counts[0] / counts[1:].mean() - 0.9) < 0.01 and counts[1:].max() - counts[1:].min() <= 1
    # a tile grid the dealing's int counters cannot hold is refused at the boundary (no overflow, nothing allocated)
    for W, H, T in ((2 ** 31 - 1, 2 ** 31 - 1, 1), (65536, 65536, 1), (2 ** 31 - 1, 3, 1)):
        with pytest.raises(_ffi.BhgError) as e:
            _ffi.deal_tiles(W, H, T, 2, 0)
        assert e.value.code == _ffi.E_INVALID and "tiles" in str(e.value)
    assert np.array_equal(bdist.deal_sequence(20, 4, 1.0), np.arange(20) % 4)
    for bad in (dict(devices=[]), dict(devices=[0], gather=9), dict(devices=[0], width=0)):
        with pytest.raises(_ffi.BhgError) as ei:
            _ffi.Frame(bad["devices"], bad.get("width", 8), 8, 1, gather=bad.get("gather", _ffi.GATHER_AUTO))
        assert ei.value.code == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi.Frame([0], 8, 8, 2, jitter=np.zeros(10))
    if _ffi.device_count() == 0:
        with pytest.raises(_ffi.BhgError) as ei:
            _ffi.Frame([0], 8, 8, 1)
        assert ei.value.code == _ffi.E_NO_DEVICE


def test_addon_device_path_needs_no_torch():
    """Blender's bundled Python has no PyTorch: the add-on, its device path included, must import and reach the library
    with `torch` unimportable (on this GPU-less box the render then stops at bhg_create with the no-device error)."""
    import subprocess
    code = (
        "import sys, importlib\n"
        "sys.modules['torch'] = None\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import fake_bpy\n"
        "from blackhole_geodesic_calculator_amd import _ffi\n"
        "bpy, depsgraph = fake_bpy.install(width=16, height=16, samples=1, device_shading=1.0, render_devices=2.0)\n"
        "addon = importlib.import_module('blackhole_geodesic_calculator_amd.blender_addon')\n"
        "addon.register()\n"
        "assert 'render_devices' in [p[0] for p in addon.EXTRA_PROPS]\n"
        "eng = addon.RelativisticRenderEngine()\n"
        "try:\n"
        "    eng.render(depsgraph)\n"
        "    print('rendered', eng.last_device_frame)\n"
        "except _ffi.BhgError as e:\n"
        "    assert e.code == _ffi.E_NO_DEVICE, e\n"
        "    print('no device')\n"
        "assert sys.modules.get('torch') is None\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and ("no device" in r.stdout or "rendered" in r.stdout), r.stdout + r.stderr


def test_c_frame_example_builds_and_fails_loudly_without_a_gpu(tmp_path):
    import subprocess
    libdir = os.path.join(ROOT, "blackhole_geodesic_calculator_amd")
    exe = tmp_path / "render_frame"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "render_frame.c"), "-L", libdir, "-lbhgeo",
                           "-Wl,-rpath," + libdir, "-lm", "-o", str(exe)])
    from blackhole_geodesic_calculator_amd import _ffi
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present: the example would run (tests/test_gpu_frame_object.py)")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stderr and r.stdout == ""


def test_bench_self_launch_relays_a_failing_launch(tmp_path):
    """bench.py --gpus N > 1 without a launcher starts its own ranks as child processes (never an exec) and exits with
    the launcher's code; on this GPU-less box the ranks fail, and that failure must come back as a non-zero exit."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--width", "64", "--samples", "1",
                          "--steps", "1", "--warmup", "0", "--ramp-seconds", "0", "--cpu-seconds", "0"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the launch succeeds (covered by tests/test_gpu_rccl.py)")
    assert out.returncode != 0
    assert "torch.distributed" in out.stderr or "Traceback" in out.stderr or "Error" in out.stderr


def test_bench_full_is_off_by_default_and_lean_overrides_it():
    """bench.py --full: off in a plain run (the headline alone), on when asked for; --lean (profiling runs) overrides it."""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False and (plain.steps, plain.warmup, plain.reps) == (20, 5, 5)
    assert bench.parse(["--full"]).full is True
    lean = bench.parse(["--full", "--lean"])
    assert lean.full is False and lean.cpu_seconds == 0.0 and lean.emulate_shards == ""


def test_bench_live_pmc_declines_cleanly(monkeypatch):
    """bench.live_pmc(): no rocprofv3 on PATH, or the run already under a profiler -> {"error": why} (the line then
    carries the committed profiles/ summary and roofline.traffic_source says so, with the reason); never an exception."""
    import importlib
    import shutil
    import types
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    a = types.SimpleNamespace(regime="adaptive", rhs="christoffel", workload="frame", tile=32, order="model", visit="auto", lpt=1,
                              width=None, height=None, samples=None, full_records=False)
    monkeypatch.setattr(shutil, "which", lambda name: None)
    assert "rocprofv3" in bench.live_pmc(a)["error"]
    monkeypatch.setattr(shutil, "which", lambda name: "/usr/bin/true")
    monkeypatch.setenv("ROCPROFILER_REGISTER_FORCE_LOAD", "1")
    assert "profiler" in bench.live_pmc(a)["error"]
    # and the replay it falls back to finds this round's summary for the default workload
    a2 = types.SimpleNamespace(regime="adaptive", rhs="christoffel", workload="frame", width=1024, height=1024, samples=5)
    traffic, source, valu = bench.pmc_traffic(a2, "dp54")
    assert source.startswith("profiles/r") and 2.5e8 < traffic < 4.5e8 and 5e8 < valu < 8e8
    # ... and the line says why it is a replay
    wl = types.SimpleNamespace(method="dp54")
    t, src, v64 = bench.counters_for(a2, wl, {"error": "the FETCH_SIZE pass overran the budget"}, 65.0e6)
    assert t == traffic and "replayed" in src and "overran" in src and 500 < v64 < 800
    t, src, v64 = bench.counters_for(a2, wl, {"hbm": 3.0e8, "valu": 6.4e8, "source": "live: ...", "ray_steps": 64.0e6}, 65.0e6)
    assert t == 3.0e8 and src.startswith("live") and abs(v64 - 640.0) < 1e-9      # normalised with the CHILD's ray-steps


def test_bench_live_pmc_kills_the_whole_process_group_on_timeout(tmp_path, monkeypatch):
    """A counter pass that overruns the shared deadline is killed with its descendants (start_new_session + killpg): a
    surviving grandchild would keep the GPU busy during the headline's timed region."""
    import importlib
    import shutil
    import types
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    fake = tmp_path / "rocprofv3"
    pidfile = tmp_path / "grandchild.pid"
    fake.write_text(f"#!/bin/bash\nsleep 300 &\necho $! > {pidfile}\nwait\n")
    fake.chmod(0o755)
    monkeypatch.setenv("PATH", str(tmp_path) + os.pathsep + os.environ["PATH"])
    for k in [k for k in os.environ if k.startswith(("ROCPROFILER_", "ROCPROF_"))]:
        monkeypatch.delenv(k)
    assert shutil.which("rocprofv3") == str(fake)
    a = types.SimpleNamespace(regime="adaptive", rhs="christoffel", workload="frame", tile=32, order="model", visit="auto", lpt=1,
                              width=None, height=None, samples=None, full_records=False)
    t = time.time()
    r = bench.live_pmc(a, deadline_s=7.0)
    assert "killed" in r["error"] and time.time() - t < 30
    pid = int(pidfile.read_text())
    time.sleep(0.3)
    alive = os.path.exists(f"/proc/{pid}") and "Z" not in open(f"/proc/{pid}/stat").read().split(")")[1].split()[0]
    assert not alive, "the profiler's descendant survived the timeout"


def _gpu_visible():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi.device_count() > 0


# ---- scripts/first_node_run.py: the one-command run for the first multi-GPU lease -------------------------------------
def _node_run():
    import importlib.util
    spec = importlib.util.spec_from_file_location("first_node_run", os.path.join(ROOT, "scripts", "first_node_run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_first_node_run_plan_covers_every_form_and_device_count():
    nr = _node_run()
    import argparse
    names = [s["name"] for s in nr.plan(argparse.Namespace(gpus=8, steps=100, warmup=10, standin=False, quick=False))]
    for n in (1, 2, 4, 8):
        assert f"dist_n{n}" in names and f"c_example_n{n}" in names
    for n in (2, 4, 8):
        for mode in ("rccl", "copy", "peer"):
            assert f"single_n{n}_{mode}" in names and f"bit_identity_n{n}_{mode}" in names
        assert f"dist_bit_identity_n{n}" in names
    assert "dist_n8_disk" in names and "dist_n8_orbit" in names and names[0] == "topology"
    assert names.index("build_render_frame") < names.index("c_example_n1")
    # the stand-in plan for a one-GPU box: gloo ranks sharing the GPU, repeated device indices, copies only
    st = nr.plan(argparse.Namespace(gpus=2, steps=5, warmup=1, standin=True, quick=True))
    by = {s["name"]: s for s in st}
    assert by["dist_n2"]["env"] == {"BHGEO_BENCH_BACKEND": "gloo"} and by["single_n2_copy"]["env"] == {"BHGEO_DEVICES": "0,0"}
    assert "single_n2_rccl" not in by and by["c_example_n2"]["cmd"][-1] == "0,0"


def test_first_node_run_records_and_compares_with_the_prediction():
    nr = _node_run()
    pred = {}
    line1 = {"metric": "m", "n_gpus": 1, "value": 4000.0, "ms_per_step": 1.25, "scaling": "weak", "config": {"collective": "none (single rank)"},
             "roofline": {"frac": 0.46, "frac_of_measured_peak": 0.5},
             "strong_predicted": {"T1_ms_per_step": 1.2, "T1_ms_per_step_two_in_flight": 1.19,
                                  "shards": {"8": {"efficiency_rank0": 0.81, "efficiency_two_in_flight": 0.8}}}}
    r1 = nr.summarise(dict(name="dist_n1", kind="bench", n=1, cmd=["python", "bench.py"], env={}), 0, "banner\n" + json.dumps(line1) + "\n", "", 30.0, pred)
    assert r1["rc"] == 0 and r1["strong_predicted_rank0"] == {"8": 0.81} and pred["T1_ms_per_step"] == 1.2
    line8 = {"metric": "m", "n_gpus": 8, "value": 30000.0, "ms_per_step": 1.4, "scaling": "weak",
             "config": {"collective": "rccl gather, 8 rank(s)", "root_share": 0.7}, "roofline": {"frac": 0.45},
             "strong": {"value": 25000.0, "ms_per_step": 0.19, "root_share": 0.7, "frames_in_flight": 2}}
    r8 = nr.summarise(dict(name="dist_n8", kind="bench", n=8, cmd=["python", "bench.py"], env={}), 0, json.dumps(line8), "", 60.0, pred)
    assert r8["rccl_ranks_seen"] == 8 and r8["root_share"] == 0.7
    assert abs(r8["strong"]["efficiency_measured"] - 1.19 / (8 * 0.19)) < 1e-12 and r8["strong"]["efficiency_rank0_predicted"] == 0.81
    # a run that printed no line, or the line of another device count, is a failure even with exit code 0
    assert nr.summarise(dict(name="dist_n2", kind="bench", n=2, cmd=["x"], env={}), 0, "no json here", "", 1.0, pred)["rc"] == 1
    assert nr.summarise(dict(name="dist_n2", kind="bench", n=2, cmd=["x"], env={}), 0, json.dumps(line8), "", 1.0, pred)["rc"] == 1


def test_first_node_run_continues_past_failures_and_exits_nonzero(tmp_path):
    """On this CPU box every GPU step fails (no device): the script must still run all of them, write one record per step
    and a summary, and exit 1.  (The C example is built by the script itself -- that step succeeds.)"""
    out = tmp_path / "node_run.jsonl"
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "first_node_run.sh"), "--standin", "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--only", "c_example,bit_identity", "--out", str(out), "--timeout", "120"], capture_output=True, text=True, timeout=600)
    recs = [json.loads(l) for l in open(out)]
    if _gpu_visible():
        pytest.skip("a GPU is visible: the steps succeed here (tests/test_gpu_rccl.py runs the stand-in plan on it)")
    assert r.returncode == 1, r.stdout + r.stderr
    assert [x["step"] for x in recs] == ["build_render_frame", "c_example_n1", "c_example_n2", "bit_identity_n2_copy", "summary"]
    assert recs[0]["rc"] == 0 and all(x["rc"] != 0 for x in recs[1:4])
    assert recs[-1]["failed"] == ["c_example_n1", "c_example_n2", "bit_identity_n2_copy"] and recs[-1]["rc"] == 1
    assert "no HIP device" in recs[1]["stderr_tail"]


# ---- host logic under sanitizers (GPU sanitizers are not available on the pool; the host side is) ----------------------
def test_tile_dealing_under_address_and_ub_sanitizers(tmp_path):
    """csrc/tile_dealing.h -- the host logic behind bhg_deal_tiles and bhg_frame_* -- compiled with g++ under
    -fsanitize=address,undefined and driven over ragged edges, one-pixel tiles, more devices than tiles, tied and extreme
    costs and every root share (tests/deal_tiles_driver.cpp checks: every pixel dealt exactly once, tiles never split);
    its shard sizes and checksums must be what the LIBRARY's bhg_deal_tiles (hipcc build, no sanitizer) deals."""
    from blackhole_geodesic_calculator_amd import _ffi
    exe = tmp_path / "deal_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "deal_tiles_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8 * 5 * 10
    lib = _ffi.load()
    checked = 0
    for line in lines[:: 7]:
        f = line.split()
        W, H, T, world, has_cost, visit = (int(v) for v in f[:6])
        share, want_sum, sizes = float(f[6]), int(f[7]), [int(v) for v in f[8:]]
        if has_cost:
            nt = ((W + T - 1) // T) * ((H + T - 1) // T)
            c1 = np.array([float((t * 7919) % 13) for t in range(nt)])
            c2 = np.array([1e300 if t % 2 else -1e300 for t in range(nt)])
            costs = [c1, c2]
        else:
            costs = [None]
        ok = False
        for cost in costs:      # (the driver's last case per shape uses the extreme costs: try both)
            got_sizes, h = [], 1469598103934665603
            for rank in range(world):
                n = ctypes.c_size_t()
                cp = None if cost is None else cost.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                assert lib.bhg_deal_tiles(W, H, T, world, cp, visit, share, rank, None, 0, ctypes.byref(n)) == 0
                px = np.empty(n.value, np.int64)
                assert lib.bhg_deal_tiles(W, H, T, world, cp, visit, share, rank, px.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n.value, ctypes.byref(n)) == 0
                got_sizes.append(int(n.value))
                for p in px.tolist():
                    h = ((h ^ ((p * 31 + rank) & 0xFFFFFFFFFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
            ok = ok or (got_sizes == sizes and h == want_sum)
        assert ok, line
        checked += 1
    assert checked >= 50


def test_bench_calibration_block_is_plain_arithmetic():
    """roofline.calibration (bench_common.calibration_block): the measured-peak fractions follow from the probes' figures by
    the stated formulas, with and without a sysfs clock sample, and a line without probes carries no block."""
    import bench_common as bc
    probe = {"fp64_fma_tflops": 72.0, "fp64_fma_clock_mhz": 2197.0, "fma_wave_insts_per_s": 5.5e11, "step_mix_tflops": 66.0,
             "step_mix_wave_insts_per_s": 5.3e11}
    after = dict(probe, fp64_fma_tflops=70.0)
    sclk = {"mean_mhz": 2300.0, "min_mhz": 2280.0, "max_mhz": 2320.0, "samples": 60, "source": "x", "pci": "y"}
    achieved, valu64, ray_steps, k_ms = 36.0, 581.0, 65.05e6, 1.14
    c = bc.calibration_block({"before": probe, "after": after}, sclk, achieved, valu64, ray_steps, k_ms)
    assert abs(c["fp64_fma_tflops_measured"] - 71.0) < 1e-12 and c["fp64_fma_tflops_before_after"] == [72.0, 70.0]
    assert abs(c["frac_of_measured_peak"] - 36.0 / 71.0) < 1e-12 and abs(c["fp64_fma_frac_of_vendor_peak"] - 71.0 / 78.6) < 1e-12
    assert abs(c["peak_tflops_at_timed_region_clock"] - 2300e6 * 128 * 256 / 1e12) < 1e-9
    assert abs(c["frac_at_timed_region_clock"] - 36.0 / (2300e6 * 128 * 256 / 1e12)) < 1e-12
    rate = valu64 * (ray_steps / 64.0) / (k_ms * 1e-3)
    assert abs(c["trace_kernel_wave_insts_per_s"] - rate) < 1.0 and abs(c["valu_issue_utilisation"] - rate / 5.5e11) < 1e-12
    assert abs(c["valu_issue_utilisation_vs_step_mix"] - rate / 5.3e11) < 1e-12
    assert abs(c["trace_kernel_wave_insts_per_clock_per_simd"] - rate / (2300e6 * 1024)) < 1e-12
    c2 = bc.calibration_block({"before": probe}, None, achieved, None, ray_steps, k_ms)
    assert isinstance(c2["sclk_mhz_timed_region"], str) and "frac_at_timed_region_clock" not in c2 and "valu_issue_utilisation" not in c2
    assert bc.calibration_block({}, sclk, achieved, valu64, ray_steps, k_ms) is None
    # round 6: the probes run after the timed region only; a clock mean of too few samples derives nothing; num_cus from the context
    c3 = bc.calibration_block({"after": after}, sclk, achieved, valu64, ray_steps, k_ms, num_cus=128)
    assert c3["probes"] == "after" and abs(c3["frac_of_measured_peak"] - 36.0 / 70.0) < 1e-12
    assert abs(c3["peak_tflops_at_timed_region_clock"] - 2300e6 * 128 * 128 / 1e12) < 1e-9
    few = dict(sclk, samples=7)
    c4 = bc.calibration_block({"after": after}, few, achieved, valu64, ray_steps, k_ms)
    assert "frac_at_timed_region_clock" not in c4 and c4["sclk_mhz_timed_region"]["samples"] == 7
    merged = bc.merge_clock_samples([dict(sclk, samples=10, mean_mhz=2000.0), None, dict(sclk, samples=30, mean_mhz=2400.0)])
    assert merged["samples"] == 40 and abs(merged["mean_mhz"] - 2300.0) < 1e-9 and merged["repetitions"] == 2
    assert bc.merge_clock_samples([None, None]) is None
    sp = bc.spread([1.0, 1.2, None, 1.1])
    assert sp == {"n": 3, "min": 1.0, "median": 1.1, "max": 1.2, "rel_spread": (1.2 - 1.0) / 1.1}
    rb = bc.roofline_block(type("W", (), {"flop": 654, "flop_executed": 601, "method": "dp54", "a": type("A", (), {"rhs": "christoffel"})})(),
                           ray_steps, k_ms, k_ms, 5242880, 81, None, "none", None, call_samples=[[1.1, 1.2], [1.3]], share=0.5)
    assert rb["kernel_ms_samples"] == [[0.55, 0.6], [0.65]] and rb["kernel_ms_spread"]["n"] == 3 and abs(rb["kernel_ms_mean"] - 0.6) < 1e-12
    # the sampler on a box without the sysfs file (this one): no thread, no figure
    smp = bc.ClockSampler(0).start()
    assert smp.stop() is None or isinstance(smp.stop(), dict)


def test_bench_dump_outputs_sample_and_limit(tmp_path):
    """bench.py --dump-outputs: a fixed, seeded sample of a large output (the same every run), all of a small one, and
    nothing written that is not float32 / float64 or that passes 64 MB."""
    import torch
    import bench
    import bench_common as bc
    assert bench.parse(["--steps", "7", "--dump-outputs", str(tmp_path / "d")]).dump_outputs == str(tmp_path / "d")
    assert bench.parse([]).dump_outputs is None and bench.parse(["--steps", "7"]).steps == 7
    s = bc.dump_sample(5 * 2048 * 2048, bc.DUMP_RAYS, seed=2)
    assert len(s) == bc.DUMP_RAYS and np.array_equal(s, bc.dump_sample(5 * 2048 * 2048, bc.DUMP_RAYS, seed=2))
    assert (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < 5 * 2048 * 2048
    assert np.array_equal(bc.dump_sample(100, bc.DUMP_RAYS, seed=2), np.arange(100))
    # two 3 x 2 frames: every pixel, in frame order, frame after frame
    imgs = [torch.arange(24, dtype=torch.float32).reshape(6, 4) + 100 * c for c in range(2)]
    rows = bc.image_rows(imgs, 3, 2)
    assert np.array_equal(rows["image_index"], np.arange(12)) and np.array_equal(rows["image_rgba"], torch.cat(imgs).numpy())
    bc.write_outputs(str(tmp_path / "ok"), rows)
    assert np.array_equal(np.load(tmp_path / "ok" / "image_rgba.npy"), rows["image_rgba"])
    with pytest.raises(RuntimeError):
        bc.write_outputs(str(tmp_path / "int"), {"x": np.zeros(3, dtype=np.int32)})
    with pytest.raises(RuntimeError):
        bc.write_outputs(str(tmp_path / "big"), {"x": np.zeros((64 << 20) // 8 + 1)})
    assert not (tmp_path / "int").exists() and not (tmp_path / "big").exists()

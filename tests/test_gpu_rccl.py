"""RCCL on the one GPU the test box has: a process group of ONE rank over the "nccl" backend (= RCCL on ROCm), so that
librccl is loaded and the frame-end exchange runs exactly as it does at N > 1 -- FrameGatherer issues its real
asynchronous dist.gather on RCCL's stream, the two slabs rotate, rank 0 assembles the frame with libbhgeo's gather
kernel on the compute stream -- and the result must be bit-identical to the frame shaded directly.  The second test
drives bench.py through the same path (BHGEO_FORCE_COLLECTIVE=1)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r"""
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["BHG_ROOT"])
from blackhole_geodesic_calculator_amd import _ffi, dist as bd
from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
from blackhole_geodesic_calculator_amd.raygen import python_random_stream
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl"
W, H, S, T = 192, 128, 3, 32
cam = np.array([1e-4, 0.0, 30.0])
sky = synthetic_sky(256, 128)
jit = python_random_stream(42.0, 2 * S * W * H)
ctx = _ffi.Context(0)
params = _ffi.make_params(r_s=1.0, lambda_end=60.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=8.0)
cost = lambda cx, cy: -abs(np.hypot(0.6 * (cx - W / 2) / W, 0.6 * (cy - H / 2) / H) - 2.598 / 30.0)
pix = bd.rank_pixels(W, H, T, 0, 1, tile_cost=cost)          # the longest-first order bench.py uses
f = DeviceFrame(ctx, W, H, S, fov_x=0.6, fov_y=0.6, sampling_seed=42.0, origin=cam, pixels=pix, jitter=jit)
f.set_sky(sky); f.set_disk(3.0, 8.0); f.generate_rays()
calls = []
def assemble(slabs, perm, frame):
    calls.append(1)
    ctx.assemble_frame_f32_device(slabs.data_ptr(), perm.data_ptr(), frame.shape[0], frame.data_ptr(),
                                  stream=torch.cuda.current_stream().cuda_stream)
g = bd.FrameGatherer(W, H, T, channels=4, dtype=torch.float32, device="cuda", assemble=assemble, tile_cost=cost,
                     collective=True)
assert g.collective and g.world == 1
for frame in range(5):                       # five frames: both slabs go round twice, every gather is a real RCCL call
    f.trace(params)
    g.submit_with(frame, f.shade_f32)
    assert g.pending[frame & 1] is not None  # an asynchronous collective is in flight
g.drain()
torch.cuda.synchronize()
assert g.frames_done == 5 and len(calls) == 5
want = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
f.shade_f32(want, f.d_pixels)
torch.cuda.synchronize()
got = g.image().reshape(-1, 4)
assert torch.equal(got, want), float((got - want).abs().max())
import ctypes
maps = open("/proc/self/maps").read()
assert "librccl" in maps, "RCCL was not loaded"
print("RCCL_WORLD1_OK")
dist.destroy_process_group()
"""


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_frame_gatherer_over_rccl_world1(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, BHG_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "RCCL_WORLD1_OK" in out.stdout


def test_bench_takes_the_collective_path_on_one_gpu():
    env = dict(os.environ, BHGEO_FORCE_COLLECTIVE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--ramp-seconds", "0",
                          "--cpu-seconds", "0", "--width", "256", "--samples", "2"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1].startswith("{"), out.stdout[-500:]   # the JSON line is the LAST line (after RCCL's banner)
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["config"]["collective"].startswith("rccl gather, 1 rank")
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["roofline"]["frac"] > 0


def test_bench_self_launches_two_ranks_when_started_without_a_launcher():
    """`python bench.py --gpus 2` started the way the driver starts N = 1 (no torch.distributed.run, WORLD_SIZE unset)
    must start its own ranks: two ranks share the box's one GPU over gloo (RCCL refuses two ranks per device), the
    N > 1 code path runs -- weak-scaling headline + the `strong` block -- and rank 0's JSON line is the parent's last line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BHGEO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--width", "256", "--samples", "2",
                          "--steps", "4", "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("{"), out.stdout[-500:]
    line = json.loads(last)
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["strong"]["value"] > 0 and line["strong"]["scaling"] == "strong"
    # the sharded path's headline has two frames in flight per rank; the sequential figure sits beside it
    assert line["strong"]["frames_in_flight"] == 2 and line["strong"]["sequential"]["value"] > 0
    # rank 0 -- the frame's owner -- is dealt a smaller shard, derived from measured times
    assert 0.5 <= line["config"]["root_share"] <= 1.0 and 0.5 <= line["strong"]["root_share"] <= 1.0
    assert "2 rank" in line["config"]["collective"]


def test_bench_measured_tile_order_two_ranks_and_single_gpu_blocks():
    """`--order measured`: the calibration trace prices the tiles, the tables are summed over the ranks (gloo here) and
    the tiles re-dealt; the frame check inside bench.py (rank 0's pixels at their places) runs on the re-dealt shards.
    And the single-GPU line of a --full run carries the blocks the contract and VERDICT round 2 name."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BHGEO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--width", "256", "--samples", "2",
                          "--steps", "4", "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0", "--order", "measured", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and "calibration trace" in line["config"]["tile_order"]
    env.pop("BHGEO_BENCH_BACKEND")      # (the single-GPU line's rank-0 emulation issues a real 1-rank RCCL gather)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--width", "256", "--samples", "2", "--steps", "8",
                          "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0", "--emulate-shards", "2", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and "row-major" in line["config"]["tile_order"]
    # (a 131k-ray frame: the trace kernel is ~50 us, the HIP-event pair around the sampled calls adds several us to it)
    assert line["roofline"]["frac"] > 0 and line["roofline"]["kernel_ms"] < 1.5 * line["ms_per_step"]
    # the headline writes whole end states (x and k, what spacetime_ray_cast returns); the sky frame's direction-only form beside it
    assert "full_records" in line["config"]["north_star_output"] and line["roofline"]["algorithmic_bytes_per_ray"] == 81
    assert line["sky_frame_dir_only"]["value"] > 0 and line["sky_frame_dir_only"]["algorithmic_bytes_per_ray"] == 57
    # both step regimes of SURVEY section 8d beside the adaptive headline
    assert line["regimes"]["fine"]["attempted_steps_per_ray"] > 100 and line["regimes"]["rk4"]["frac"] > 0.1
    cal = line["roofline"]["calibration"]
    assert 30.0 < cal["fp64_fma_tflops_measured"] < 90.0 and 0.0 < line["roofline"]["frac_of_measured_peak"] < 1.0
    assert cal["issue_bound_wave_insts_per_s"] > 1e11
    sh = line["strong_predicted"]["shards"]["2"]
    assert sh["rays"] * 2 == 256 * 256 * 2 and 0.2 < sh["efficiency"] < 1.5 and sh["ms_per_step_two_in_flight"] > 0
    # rank 0's step: the shard's slab through a 1-rank gather + the root's assembly of the whole 2-rank frame
    assert "rank0_error" not in line["strong_predicted"], line["strong_predicted"].get("rank0_error")
    assert 0.1 < sh["efficiency_rank0"] < 1.5 and sh["ms_per_step_rank0"] >= 0.8 * sh["ms_per_step"]
    assert 0.5 <= sh["root_share"] <= 1.0 and sh["efficiency_rank0_equal_shares"] > 0


def test_bench_orbit_two_ranks_reports_whole_frame_sharding_beside_the_tile_figure():
    """Config 4 over 2 ranks (gloo, one GPU): the headline shards every frame's tiles; `frames_sharded` deals whole
    frames round-robin with one gather at the end."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BHGEO_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "orbit", "--width", "256",
                          "--samples", "2", "--steps", "6", "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    fs = line["frames_sharded"]
    assert fs["value"] > 0 and "round-robin" in fs["what"]


@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("workload", ["frame", "disk", "orbit"])
def test_bench_single_process_mode(devices, workload):
    """`--single-process`: the library-owned frame (bhg_frame_*) over the listed devices of ONE process, no
    torch.distributed; "0,0" = two contexts of this box's one GPU (the N > 1 code path: dealing, slabs, gather, assembly)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BHGEO_DEVICES=devices)
    n = len(devices.split(","))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--single-process", "--gpus", str(n), "--workload", workload,
                          "--width", "256", "--samples", "2", "--steps", "8", "--warmup", "2", "--ramp-seconds", "0", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == n and line["value"] > 0 and line["roofline"]["frac"] > 0
    assert "ONE process" in line["config"]["parallelism"] and len(line["config"]["trace_call_ms_per_device"]) == n
    frames = 5 if workload == "disk" else 1
    assert line["config"]["rays_per_gpu"] * n == 256 * 256 * 2 * frames * (n if workload != "orbit" else 1)
    if n > 1 and workload != "orbit":
        assert line["strong"]["value"] > 0 and line["config"]["collective"].startswith("copy")


def test_bench_measures_traffic_live_with_rocprofv3_child_runs():
    """The single-GPU line of a --full run measures roofline.traffic and the VALU instruction count in its own run: three
    rocprofv3 --pmc child runs of the same command, started before the parent touches the GPU."""
    import shutil
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 not on PATH")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--width", "256", "--samples", "2", "--steps", "4",
                          "--warmup", "2", "--ramp-seconds", "0", "--cpu-seconds", "0.2", "--emulate-shards", "", "--full"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    r = line["roofline"]
    assert r["traffic_source"].startswith("live: rocprofv3"), r["traffic_source"]
    n = 256 * 256 * 2
    assert 0.5 * n * 57 < r["traffic"] < 4.0 * n * 57            # HBM bytes per launch: around the algorithmic 57 B/ray
    assert 400 < r["valu_insts_per_64_ray_steps"] < 1200
    assert line["cpu_baseline"]["value"] > 0


def test_first_node_run_script_works_with_one_gpu_stand_ins(tmp_path):
    """scripts/first_node_run.sh -- the one command for the first multi-GPU lease -- run here with its stand-ins for a
    one-GPU box (--standin: torch.distributed ranks over gloo sharing the GPU, device lists that repeat device 0), so that
    the script itself is known to work before a node is spent on it: every step ends with rc 0, the two-rank line carries
    the strong block with a measured efficiency next to the prediction of the one-rank line, the sharded images equal the
    one-device image bit for bit."""
    out = tmp_path / "node_run.jsonl"
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "first_node_run.sh"), "--standin", "--quick", "--gpus", "2", "--steps", "8",
                        "--warmup", "2", "--out", str(out), "--timeout", "300"], capture_output=True, text=True, timeout=1200)
    recs = {x["step"]: x for x in (json.loads(l) for l in open(out))}
    assert r.returncode == 0 and recs["summary"]["failed"] == [], (r.stdout[-2000:], r.stderr[-2000:])
    want = ["topology", "dist_n1", "dist_n2", "dist_n2_disk", "dist_n2_orbit", "single_n1_auto", "single_n2_copy", "build_render_frame", "c_example_n1", "c_example_n2", "bit_identity_n2_copy",
            "dist_bit_identity_n2"]
    assert [k for k in recs if k != "summary"] == want and all(recs[k]["rc"] == 0 for k in want)
    assert recs["dist_n1"]["strong_predicted_rank0"].get("2") is not None and recs["dist_n1"]["frac_of_measured_peak"] > 0.3
    st = recs["dist_n2"]["strong"]
    # (two gloo ranks SHARING one GPU: the measured "efficiency" is ~0.2 here by construction; what is checked is that the figure exists)
    assert recs["dist_n2"]["n_gpus"] == 2 and st["efficiency_measured"] > 0.05 and st["efficiency_rank0_predicted"] is not None
    assert recs["single_n2_copy"]["n_gpus"] == 2 and "copy" in recs["single_n2_copy"]["collective"]
    assert recs["c_example_n1"]["signature"] == recs["c_example_n2"]["signature"]
    assert recs["bit_identity_n2_copy"]["bit_identical"] is True and recs["bit_identity_n2_copy"]["images"] == 3
    assert recs["dist_bit_identity_n2"]["bit_identical"] is True and "'world': 2" in recs["dist_bit_identity_n2"]["detail"]

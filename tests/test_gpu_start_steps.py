"""The rays' initial steps kept across calls on unchanged rays (bhg_trace_start_device, BHG_START_STEPS).

A DP5(4) trace works every ray's first step size out before it integrates; an owner of unchanged rays records the steps once
and replays them afterwards.  Nothing about a result may change: every comparison below is array_equal -- end records or exit
directions, flags, n_steps, n_accepted and object_id -- between a plain call, a recording call and a replaying call on the same
rays, through the raw entry point (every kernel variant, the shapes at which the indexing can go wrong), through the owners of
a cache (DeviceFrame, FrameBatch, the library's bhg_frame) and across everything that must, or must not, invalidate one.

The split of a call of more than 2^26 rays walks d_start_steps along with d_k0 (TraceCall::slice, csrc/trace_call.h): that size
cannot be reached in a GPU test, so the offset is checked at a limit of 64 rays by tests/test_trace_call_host.py, not here.
"""
import numpy as np
import pytest

from conftest import CAM

pytestmark = pytest.mark.gpu

SENTINEL = -7.0   # what the start-step arrays hold before a call: no recorded step is negative


def _params(**kw):
    from blackhole_geodesic_calculator_amd import _ffi
    kw.setdefault("max_steps", 20000)
    return _ffi.make_params(**kw)


def _mix(n, seed):
    """Seeded camera-like rays from per-ray origins around the camera, with: origins inside the horizon (start-inside rays), a NaN
    direction, a zero direction."""
    from conftest import frame_rays
    rng = np.random.default_rng(seed)
    k0 = frame_rays(n, seed=seed)
    x0 = CAM[None, :] + rng.uniform(-0.5, 0.5, (n, 3))
    inside = rng.permutation(n)[:max(3, n // 12)]
    x0[inside] = rng.uniform(-0.25, 0.25, (len(inside), 3))      # |x| < 0.44 < r_s = 1 (and inside the Kerr horizon, r_+ = 0.72)
    free = np.setdiff1d(np.arange(n), inside)
    k0[free[1]] = np.nan
    k0[free[len(free) // 2]] = 0.0
    return np.ascontiguousarray(x0), np.ascontiguousarray(k0), inside


def _call(ctx, p, x0, k0, mode, d_h=None, form="end", spheres=None):
    """One device trace call of the given start mode; every output as numpy."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    n = len(k0)
    d_x0, d_k0 = torch.as_tensor(x0).cuda(), torch.as_tensor(k0).cuda()
    out = torch.full((n, 6 if form == "end" else 3), 123.0, dtype=torch.float64, device="cuda")
    fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st, ac = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    obj = torch.full((n,), 99, dtype=torch.int8, device="cuda")
    kw = dict(d_x0=d_x0.data_ptr(), d_flags=fl.data_ptr(), d_n_steps=st.data_ptr(), d_n_accepted=ac.data_ptr(),
              d_start_steps=0 if d_h is None else d_h.data_ptr(), start_mode=mode)
    if form == "end":
        ctx.trace_device(p, n, d_k0.data_ptr(), out.data_ptr(), spheres=spheres,
                         d_object_id=obj.data_ptr() if spheres is not None else 0, **kw)
    else:
        ctx.trace_dir_device(p, n, d_k0.data_ptr(), out.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert ctx.last_launch()["passes"] == 1
    res = {"out": out.cpu().numpy(), "flags": fl.cpu().numpy(), "n_steps": st.cpu().numpy(), "n_accepted": ac.cpu().numpy()}
    if spheres is not None:
        res["object_id"] = obj.cpu().numpy()
    return res


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


# (name, params, output form, object spheres)
KERR = dict(rhs_form=2, spin=0.45)      # a / M = 0.9
VARIANTS = [
    ("full", dict(lambda_end=50.0), "end", None),
    ("dir", dict(lambda_end=50.0), "dir", None),
    ("exit+disk", dict(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0), "end", None),
    ("objects", dict(lambda_end=200.0, r_exit=40.0), "end", [[1.0, 0.5, 12.0, 2.0], [-3.0, 0.0, 6.0, 1.0]]),
    ("objects+disk", dict(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0), "end", [[1.0, 0.5, 12.0, 2.0]]),
    ("reduced", dict(lambda_end=50.0, rhs_form=1), "end", None),
    ("kerr", dict(lambda_end=50.0, **KERR), "end", None),
    ("kerr-dir+exit", dict(lambda_end=200.0, r_exit=40.0, **KERR), "dir", None),
    ("time-like", dict(lambda_end=50.0, time_like=1), "end", None),
    ("max_step", dict(lambda_end=50.0, max_step=0.1), "end", None),            # h0 clipped by max_step
    ("short", dict(lambda_end=0.05), "end", None),                              # h0 clipped by lambda_end
    ("rk4", dict(lambda_end=50.0, method=1, h_fixed=0.05), "end", None),
]
# less than one batch; more batches than the 8 slices, with a ragged tail; S = 5 blocks of P = 192 (the work-order hint
# permutes batches, the array is indexed by ray); the same with P = 200 (the hint is dropped)
SHAPES = [(37, 0), (64 * 9 + 5, 0), (192 * 5, 5), (200 * 5, 5)]


@pytest.mark.parametrize("n,order_blocks", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,pkw,form,spheres", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_record_and_replay_equal_the_plain_call(ctx, name, pkw, form, spheres, n, order_blocks):
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    x0, k0, inside = _mix(n, seed=n)
    p = _params(order_blocks=order_blocks, **pkw)
    plain = _call(ctx, p, x0, k0, _ffi.START_NONE, form=form, spheres=spheres)
    d_h = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    rec = _call(ctx, p, x0, k0, _ffi.START_RECORD, d_h, form=form, spheres=spheres)
    h = d_h.cpu().numpy().copy()
    rep = _call(ctx, p, x0, k0, _ffi.START_REPLAY, d_h, form=form, spheres=spheres)
    _same(plain, rec, "recording call")
    _same(plain, rep, "replaying call")
    assert np.array_equal(d_h.cpu().numpy(), h), "a replaying call wrote into the array"
    started_inside = (plain["flags"] & 2) != 0
    assert started_inside[inside].all() and started_inside.sum() == len(inside)
    assert (plain["flags"] & (32 | 64)).any()          # the NaN / zero directions fail in the step loop, in all three calls
    if name == "rk4":
        assert np.all(h == SENTINEL)                   # no initial step: the array is left untouched
        return
    # every ray that was queued has a finite step in [0, min(lambda_end, max_step)]; the others were never written
    queued = ~started_inside
    assert np.all(h[~queued] == SENTINEL)
    assert np.all(np.isfinite(h[queued])) and h[queued].min() >= 0.0 and h[queued].max() <= min(p.lambda_end, p.max_step)
    assert (h[queued] > 0.0).sum() >= queued.sum() - 2     # (all but the NaN and, at most, the zero direction)
    if name in ("max_step", "short"):
        assert (h[queued] == min(p.lambda_end, p.max_step)).sum() > n // 2    # ... and most are clipped there
    # a second recording call writes the same bits
    d_h2 = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    _call(ctx, p, x0, k0, _ffi.START_RECORD, d_h2, form=form, spheres=spheres)
    assert np.array_equal(d_h2.cpu().numpy(), h)


def test_bad_start_arguments_are_refused(ctx):
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    x0, k0, _ = _mix(37, seed=1)
    d_h = torch.zeros(37, dtype=torch.float64, device="cuda")
    with pytest.raises(_ffi.BhgError):
        _call(ctx, _params(), x0, k0, _ffi.START_RECORD, None)      # no array
    with pytest.raises(_ffi.BhgError):
        _call(ctx, _params(), x0, k0, 3, d_h)                       # no such mode


# ---- DeviceFrame ------------------------------------------------------------------------------------------------------------

W, H, S = 64, 40, 3
SPHERES = [[1.0, 0.5, 12.0, 2.0]]


def _frame(ctx, sky, origin=CAM, jitter=None, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    fr = DeviceFrame(ctx, W, H, S, fov_x=0.6, fov_y=0.6, sampling_seed=42.0, origin=origin, jitter=jitter, **kw)
    fr.set_sky(sky)
    fr.generate_rays()
    return fr


def _results(fr):
    import torch
    torch.cuda.synchronize()
    res = {"flags": fr.d_flags.cpu().numpy(), "n_steps": fr.d_steps.cpu().numpy(), "n_accepted": fr.d_acc.cpu().numpy()}
    res["out"] = (fr.d_dir if fr._traced == "dir" else fr.d_end).cpu().numpy()
    if fr.spheres is not None and len(fr.spheres) > 0:
        res["object_id"] = fr.d_obj.cpu().numpy()
    return res


@pytest.fixture(scope="module")
def sky():
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    return synthetic_sky(128, 64)


def _fresh(ctx, sky, p, origin=CAM, jitter=None, spheres=None):
    """What a frame made for these settings alone gives, without a cache."""
    fr = _frame(ctx, sky, origin=origin, jitter=jitter, start_cache=False)
    if spheres is not None:
        fr.set_objects(spheres)
    fr.trace(p)
    assert fr.start_steps.recorded == 0 and fr.start_steps.replayed == 0 and fr.start_steps.d_h is None
    return _results(fr)


def test_device_frame_replays_until_something_it_depends_on_changes(ctx, sky):
    fr = _frame(ctx, sky)
    ss = fr.start_steps
    p = _params(lambda_end=50.0)
    want = _fresh(ctx, sky, p)
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (1, 0)
    _same(_results(fr), want, "recording trace")
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (1, 1)
    _same(_results(fr), want, "replaying trace")
    # what the step does not depend on: the exit sphere, the disk, the step budget, the hint -- replayed, and right
    p2 = _params(lambda_end=50.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0, max_steps=5000, order_blocks=1)
    fr.trace(p2)
    assert (ss.recorded, ss.replayed) == (1, 2)
    _same(_results(fr), _fresh(ctx, sky, p2), "other events")
    # rtol, then max_step, then the origin: each records anew and equals a fresh frame's
    count = 1
    for kw, origin in ((dict(rtol=1e-5), CAM), (dict(rtol=1e-5, max_step=0.1), CAM), (dict(rtol=1e-5, max_step=0.1), CAM + [0.5, -1.0, 2.0])):
        q = _params(lambda_end=50.0, **kw)
        fr.origin = np.asarray(origin, dtype=np.float64)
        fr.trace(q)
        count += 1
        assert ss.recorded == count, kw
        _same(_results(fr), _fresh(ctx, sky, q, origin=origin), f"after {kw} at {origin}")
        fr.trace(q)
        assert ss.recorded == count and ss.valid
        _same(_results(fr), _fresh(ctx, sky, q, origin=origin), f"replay after {kw} at {origin}")


def test_device_frame_camera_assigned_after_a_trace_drops_what_the_trace_wrote(ctx, sky):
    """origin, rot, fov_x and fov_y are assigned to from frame to frame.  They used to be plain attributes: shade() after a new
    origin weighed the records of the old trace with a g worked out from the new position (set_disk and set_objects guard the same
    case), and render() after a new rotation or field of view kept the old rays unless it was told to make them anew (found by
    tests/test_gpu_frame_sequences.py).  Now shade() asks for a trace, and render() gives the fresh frame's image."""
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix
    p = _params(lambda_end=200.0, r_exit=40.0)

    def fresh(origin=CAM, euler=(0.0, 0.0, 0.0), fov=(0.6, 0.6)):
        f = DeviceFrame(ctx, W, H, S, fov_x=fov[0], fov_y=fov[1], sampling_seed=42.0, origin=origin, rotation_euler=euler, start_cache=False)
        f.set_sky(sky)
        f.set_redshift(("sky",), 4.0)
        return f.render(p).cpu().numpy()

    fr = _frame(ctx, sky)
    fr.set_redshift(("sky",), 4.0)          # (the sky's g depends on where the camera is)
    assert np.array_equal(fr.render(p).cpu().numpy(), fresh())
    fr.shade()
    moved = CAM + [0.5, -1.0, 2.0]
    fr.origin = moved
    with pytest.raises(RuntimeError):
        fr.shade()
    want = fresh(origin=moved)
    assert not np.array_equal(want, fresh())
    assert np.array_equal(fr.render(p).cpu().numpy(), want)
    assert fr.start_steps.recorded == 2     # (the steps belong to the origin; the rays were kept)
    euler = (0.05, -0.04, 0.1)
    for kw, assign in ((dict(euler=euler), lambda: setattr(fr, "rot", euler_xyz_matrix(euler))),
                       (dict(euler=euler, fov=(0.6, 0.5)), lambda: setattr(fr, "fov_y", 0.5)),
                       (dict(euler=euler, fov=(0.7, 0.5)), lambda: setattr(fr, "fov_x", 0.7))):
        recorded = fr.start_steps.recorded
        assign()
        with pytest.raises(RuntimeError):
            fr.shade()
        want = fresh(origin=moved, **kw)
        assert np.array_equal(fr.render(p).cpu().numpy(), want), kw       # (no regenerate_rays=True: the frame knows)
        assert fr.start_steps.recorded == recorded + 1
        assert np.array_equal(fr.render(p).cpu().numpy(), want) and fr.start_steps.recorded == recorded + 1
    # the held values assigned again (an owner that writes its whole camera every frame) keep the rays, the steps and the trace
    recorded = fr.start_steps.recorded
    fr.origin, fr.rot, fr.fov_x, fr.fov_y = np.array(moved), euler_xyz_matrix(euler), 0.7, 0.5
    assert np.array_equal(fr.shade().cpu().numpy(), want)
    assert np.array_equal(fr.render(p).cpu().numpy(), want) and fr.start_steps.recorded == recorded
    # the frame holds its own copies, which cannot be written in place behind its back
    mine = np.array(moved)
    fr.origin = mine
    mine[2] += 1.0
    assert np.array_equal(fr.origin, moved)
    with pytest.raises(ValueError):
        fr.origin[2] = 0.0
    with pytest.raises(ValueError):
        fr.rot[0, 0] = 0.0


def test_device_frame_new_rays_invalidate(ctx, sky):
    import torch
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    fr = _frame(ctx, sky)
    ss = fr.start_steps
    p = _params(lambda_end=50.0)
    fr.trace(p)
    assert ss.valid and ss.recorded == 1
    # generate_rays with another jitter stream: other rays in the same buffer
    jitter = python_random_stream(7.0, 2 * S * W * H)
    fr.d_jitter = torch.as_tensor(np.asarray(jitter, dtype=np.float64)).to(fr.dev)
    fr.generate_rays()
    assert not ss.valid
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (2, 0)
    _same(_results(fr), _fresh(ctx, sky, p, jitter=jitter), "regenerated rays")
    # assignment of d_k0: a tensor of other rays
    other = _frame(ctx, sky, start_cache=False)
    fr.d_k0 = other.d_k0.clone()
    assert not ss.valid
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (3, 0)
    _same(_results(fr), _fresh(ctx, sky, p), "assigned rays")
    # a frame that READS another's rays (a twin) notices when the owner regenerates them in place
    twin = _frame(ctx, sky)
    twin.d_k0 = fr.d_k0
    twin.trace(p)
    twin.trace(p)
    assert (twin.start_steps.recorded, twin.start_steps.replayed) == (1, 1)
    fr.generate_rays()                       # (the jitter of seed 7 again)
    twin.trace(p)
    assert (twin.start_steps.recorded, twin.start_steps.replayed) == (2, 1)
    _same(_results(twin), _fresh(ctx, sky, p, jitter=jitter), "twin after the owner regenerated")
    # the observer camera makes the rays anew
    fr.trace(p)
    assert ss.valid
    fr.set_observer((0.0, 0.3, 0.0))
    assert not ss.valid


def test_device_frame_moving_a_sphere_keeps_the_steps(ctx, sky):
    fr = _frame(ctx, sky)
    ss = fr.start_steps
    p = _params(lambda_end=200.0, r_exit=40.0)
    fr.set_objects(SPHERES)
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (1, 0)
    for i, moved in enumerate(([[1.5, 0.0, 11.0, 2.0]], [[-2.0, 1.0, 9.0, 1.5], [3.0, 0.0, 14.0, 1.0]])):
        fr.set_objects(moved)
        fr.set_sky(sky)
        assert ss.valid
        fr.trace(p)
        assert (ss.recorded, ss.replayed) == (1, i + 1)
        got = _results(fr)
        assert (got["object_id"] >= 0).any()
        _same(got, _fresh(ctx, sky, p, spheres=moved), f"spheres {moved}")
    fr.set_disk(3.0, 12.0)
    fr.trace(_params(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0))
    assert (ss.recorded, ss.replayed) == (1, 3)


def test_environment_switch_gives_the_plain_path(ctx, sky, monkeypatch):
    monkeypatch.setenv("BHGEO_START_CACHE", "0")
    fr = _frame(ctx, sky)
    p = _params(lambda_end=50.0)
    fr.trace(p)
    fr.trace(p)
    ss = fr.start_steps
    assert (ss.recorded, ss.replayed) == (0, 0) and ss.d_h is None and not ss.valid
    got = _results(fr)
    monkeypatch.delenv("BHGEO_START_CACHE")
    fr.trace(p)
    fr.trace(p)
    assert (ss.recorded, ss.replayed) == (1, 1)
    _same(_results(fr), got, "with and without the switch")


def test_frame_batch_replay_equals_plain(ctx, sky):
    import torch
    from blackhole_geodesic_calculator_amd.device_frame import FrameBatch
    cams = [dict(origin=(1e-4, 0.0, 30.0), rotation_euler=(0.0, 0.0, 0.0)), dict(origin=(0.0, -20.0, 8.0), rotation_euler=(1.2, 0.0, 0.0))]
    p = _params(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0)

    def run(batch, times):
        for f in batch.frames:
            f.set_sky(sky)
            f.set_disk(3.0, 12.0)
            f.generate_rays()
        out = []
        for _ in range(times):
            batch.trace(p)
            torch.cuda.synchronize()
            out.append({"out": batch.d_end.cpu().numpy(), "flags": batch.d_flags.cpu().numpy(), "n_steps": batch.d_steps.cpu().numpy(),
                        "n_accepted": batch.d_acc.cpu().numpy()})
        return out

    plain_batch = FrameBatch(ctx, cams, W, H, S, fov_x=0.9, fov_y=0.9, start_cache=False)
    plain, = run(plain_batch, 1)
    assert plain_batch.start_steps.d_h is None
    batch = FrameBatch(ctx, cams, W, H, S, fov_x=0.9, fov_y=0.9)
    rec, rep = run(batch, 2)
    assert (batch.start_steps.recorded, batch.start_steps.replayed) == (1, 1)
    _same(plain, rec, "recording batch")
    _same(plain, rep, "replaying batch")
    assert (plain["flags"] & 128).any() and len(np.unique(plain["flags"])) >= 3
    # a member that makes its rays anew takes the batch's steps with it
    batch.frames[1].generate_rays()
    assert batch.start_steps.valid            # (noticed at the next trace: the block's stamp changed)
    batch.trace(p)
    assert (batch.start_steps.recorded, batch.start_steps.replayed) == (2, 1)


# ---- the library's own frame ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_library_frame_renders_equal_a_fresh_frames(ctx, sky, devices):
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    jitter = python_random_stream(42.0, 2 * S * W * H)

    def fresh(p, origin):
        f = _ffi.Frame(devices, W, H, S, fov_x=0.6, fov_y=0.6, origin=origin, jitter=jitter)
        f.set_scene(sky, disk=(3.0, 12.0))
        img = f.render(p).copy()
        f.close()
        return img

    dk = dict(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0)
    fr = _ffi.Frame(devices, W, H, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=jitter)
    fr.set_scene(sky, disk=(3.0, 12.0))
    p = _params(**dk)
    want = fresh(p, CAM)
    assert np.array_equal(fr.render(p), want)          # records
    assert np.array_equal(fr.render(p), want)          # replays
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    q = _params(rtol=1e-5, **dk)
    want_q = fresh(q, CAM)
    assert not np.array_equal(want_q, want)
    assert np.array_equal(fr.render(q), want_q) and np.array_equal(fr.render(q), want_q)
    cam2 = CAM + [0.5, -1.0, 2.0]
    fr.set_camera(fov_x=0.6, fov_y=0.6, origin=cam2)
    want_c = fresh(q, cam2)
    assert not np.array_equal(want_c, want_q)
    assert np.array_equal(fr.render(q), want_c) and np.array_equal(fr.render(q), want_c)
    # back: recorded for this origin again
    fr.set_camera(fov_x=0.6, fov_y=0.6, origin=CAM)
    assert np.array_equal(fr.render(p), want)
    fr.close()

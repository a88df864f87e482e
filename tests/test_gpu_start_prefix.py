"""The rays' start-up records kept across calls on unchanged rays (bhg_trace_prefix_device, BHG_START_PREFIX).

A recording call takes every ray through its leading accepted steps inside a ball of radius rho about the shared start point and
keeps the state reached; a replaying call whose scene stays clear of that ball puts the kept states straight into the queue.
Nothing about a result may change: every comparison below is array_equal -- end records or exit directions, flags, n_steps,
n_accepted and object_id -- between a plain call, a recording call and a replaying call on the same rays, for every kernel
variant in scope, and a call that must not replay (the scene reaches into the ball, or the call is out of scope) says so in the
mode it reports and still equals the plain call.
"""
import numpy as np
import pytest

from conftest import CAM, frame_rays

pytestmark = pytest.mark.gpu

K_MAX = 4


def _params(**kw):
    from blackhole_geodesic_calculator_amd import _ffi
    kw.setdefault("max_steps", 20000)
    return _ffi.make_params(**kw)


def _rays(n, seed, fov=0.6):
    """Seeded camera-like rays with a NaN direction and a zero direction among them (both inside the first batch)."""
    k0 = frame_rays(n, seed=seed, fov=fov)
    k0[7] = np.nan
    k0[n // 2] = 0.0
    return np.ascontiguousarray(k0)


class Records:
    """The owner's side of bhg_prefix: the device array and the rho of its records."""

    def __init__(self, n, fill=0):
        import torch
        self.n = n
        self.d = torch.full((n * 112,), fill, dtype=torch.uint8, device="cuda")
        self.rho = 0.0

    def planes(self):
        """(doubles [6][n][2], words [n][4]) as numpy."""
        raw = self.d.cpu().numpy()
        return raw[:96 * self.n].view(np.float64).reshape(6, self.n, 2), raw[96 * self.n:].view(np.uint32).reshape(self.n, 4)

    def depth(self):
        return self.planes()[1][:, 1]


def _call(ctx, p, x0, k0, mode=0, rec=None, form="end", spheres=None, d_h=None, start_mode=0):
    """One shared-origin device trace call; every output as numpy, and what the call reports about the records."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    n = len(k0)
    d_k0 = torch.as_tensor(k0).cuda()
    out = torch.full((n, 6 if form == "end" else 3), 123.0, dtype=torch.float64, device="cuda")
    fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st, ac = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    obj = torch.full((n,), 99, dtype=torch.int8, device="cuda")
    pf = None
    if rec is not None:
        pf = _ffi.Prefix(rec.d.data_ptr(), rec.rho, mode, -1)
    kw = dict(x0_shared=x0, d_flags=fl.data_ptr(), d_n_steps=st.data_ptr(), d_n_accepted=ac.data_ptr(),
              d_start_steps=0 if d_h is None else d_h.data_ptr(), start_mode=start_mode, prefix=pf)
    if form == "end":
        ctx.trace_device(p, n, d_k0.data_ptr(), out.data_ptr(), spheres=spheres,
                         d_object_id=obj.data_ptr() if spheres is not None else 0, **kw)
    else:
        ctx.trace_dir_device(p, n, d_k0.data_ptr(), out.data_ptr(), **kw)
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy(), "flags": fl.cpu().numpy(), "n_steps": st.cpu().numpy(), "n_accepted": ac.cpu().numpy()}
    if spheres is not None:
        res["object_id"] = obj.cpu().numpy()
    used = None
    if pf is not None:
        used = pf.used
        if mode == _ffi.PREFIX_RECORD:
            rec.rho = pf.rho
    return res, used


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _three(ctx, p, x0, k0, form="end", spheres=None, rec_p=None, rec_spheres=None, expect_replay=True):
    """plain / recording / replaying call; the recording call may see another scene (rec_p, rec_spheres) than the other two.
    Returns (plain result, Records)."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = len(k0)
    plain, _ = _call(ctx, p, x0, k0, form=form, spheres=spheres)
    rec = Records(n)
    if rec_p is None:
        r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_RECORD, rec, form=form, spheres=spheres)
        _same(plain, r, "recording call")
    else:
        _, used = _call(ctx, rec_p, x0, k0, _ffi.PREFIX_RECORD, rec, form=form, spheres=rec_spheres)
    assert used == _ffi.PREFIX_RECORD and rec.rho > 0.0
    before = rec.d.clone()
    rep, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rec, form=form, spheres=spheres)
    assert used == (_ffi.PREFIX_REPLAY if expect_replay else _ffi.PREFIX_NONE)
    _same(plain, rep, "replaying call" if expect_replay else "refused call")
    assert bool((rec.d == before).all()), "a replaying call wrote into the records"
    return plain, rec


OBJ = [[1.0, 0.5, 12.0, 2.0], [-3.0, 0.0, 6.0, 1.0]]
# the kernel variants <rhs, events> in scope: (name, params, object spheres, rho expected at CAM: 1/4 min(clearance, |x0|))
VARIANTS = [
    ("<0,0>", dict(lambda_end=50.0), None, 7.25),                                                    # horizon only: (30 - 1) / 4
    ("<0,1>", dict(lambda_end=200.0, r_exit=40.0), None, 2.5),
    ("<0,3>", dict(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0), None, 2.5),
    ("<0,5>", dict(lambda_end=200.0, r_exit=40.0), OBJ, 2.5),
    ("<1,0>", dict(lambda_end=50.0, rhs_form=1), None, 7.25),
]
# three batches and a partial one; 64 batches, handed out in the order of a 4-sample frame
SHAPES = [(209, 0), (4096, 4)]


@pytest.mark.parametrize("n,order_blocks", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,pkw,spheres,rho", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_record_and_replay_equal_the_plain_call(ctx, name, pkw, spheres, rho, n, order_blocks):
    k0 = _rays(n, seed=n)
    p = _params(order_blocks=order_blocks, **pkw)
    plain, rec = _three(ctx, p, CAM, k0, spheres=spheres)
    assert rec.rho == pytest.approx(rho, rel=1e-5)
    d, w = rec.planes()
    depth = w[:, 1]
    print(name, n, "depth histogram", np.bincount(depth, minlength=K_MAX + 1).tolist())
    assert np.array_equal(w[:, 0], np.arange(n)) and np.array_equal(w[:, 2], depth) and not w[:, 3].any() and depth.max() <= K_MAX
    assert depth[7] == 0 and (depth == 0).sum() == 1        # the NaN direction alone: every batch position else is usable
    ok = depth > 0
    # the kept states lie inside the ball, in front of the ray's end, with a step to try next
    x = np.stack([d[0, :, 0], d[0, :, 1], d[1, :, 0]], 1)
    assert np.all(np.linalg.norm(x[ok] - CAM, axis=1) <= rec.rho)
    assert np.all(d[5, ok, 1] < p.lambda_end) and np.all(d[4, ok, 1] > 0.0)
    # scipy's start guess needs at least two x10 steps to leave a ball of this size: the records are worth having
    assert np.median(depth) >= 2
    assert np.all(plain["n_steps"][ok] > depth[ok])


def test_direction_only_calls_replay_too(ctx):
    _three(ctx, _params(lambda_end=50.0), CAM, _rays(209, seed=5), form="dir")


def test_start_steps_and_records_together(ctx):
    """Both caches in one call, as DeviceFrame drives them: the lanes without a usable record replay their start step."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=11)
    p = _params(lambda_end=200.0, r_exit=40.0)
    plain, _ = _call(ctx, p, CAM, k0)
    rec = Records(n)
    d_h = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    r, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD, rec, d_h=d_h, start_mode=_ffi.START_RECORD)
    assert used == _ffi.PREFIX_RECORD
    _same(plain, r, "recording call")
    assert (d_h.cpu().numpy() >= 0.0).all()
    r, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_REPLAY, rec, d_h=d_h, start_mode=_ffi.START_REPLAY)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain, r, "replaying call")


def test_max_step_clamps_every_step_of_the_prefix(ctx):
    p = _params(lambda_end=50.0, max_step=0.1)
    _, rec = _three(ctx, p, CAM, _rays(209, seed=2))
    d, w = rec.planes()
    ok = np.arange(209) != 7
    assert np.all(w[ok, 1] == K_MAX)
    moving = ok & (np.arange(209) != 209 // 2)
    # h0 < 0.1, min(10 h0, max_step), then two steps of max_step: no ray gets farther than K_MAX max_step
    assert np.all(d[5, moving, 1] > 0.2) and np.all(d[5, moving, 1] <= 0.4 + 1e-12)


def test_rays_that_end_inside_the_prefix(ctx):
    p = _params(lambda_end=0.05)
    plain, rec = _three(ctx, p, CAM, _rays(209, seed=3))
    depth = rec.depth()
    print("depth histogram", np.bincount(depth, minlength=K_MAX + 1).tolist())
    # the attempt that reaches lambda_end is never kept: at most the one step in front of it is
    moving = np.arange(209) != 209 // 2          # (the zero direction goes nowhere: K_MAX steps of 1e-6 and its like)
    assert depth[moving].max() <= 1 and (depth == 0).sum() > 1
    assert (plain["flags"] & 4).sum() >= 207


def test_a_rejection_in_the_first_attempts_ends_the_record(ctx):
    """Close to the hole with loose tolerances the x10 climb overshoots at once: the third attempt of about half the rays is
    rejected (scipy RK45 on the same start: 33 of 64), and the record stops in front of it."""
    n = 209
    p = _params(lambda_end=50.0, rtol=1e-1, atol=1e-3)
    x0 = np.array([1e-4, 0.0, 3.0])
    plain, rec = _three(ctx, p, x0, _rays(n, seed=3, fov=2.5))
    assert rec.rho == pytest.approx(0.5, rel=1e-5)
    depth = rec.depth()
    print("depth histogram", np.bincount(depth, minlength=K_MAX + 1).tolist())
    assert (plain["n_steps"] > plain["n_accepted"]).sum() > n // 2
    moving = np.arange(n) != n // 2
    assert depth[moving].max() <= 3 and (depth == 2).sum() >= n // 4


def test_a_start_inside_the_hole_records_nothing(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=4)
    x0 = np.array([0.1, 0.0, 0.2])
    p = _params(lambda_end=50.0)
    plain, _ = _call(ctx, p, x0, k0)
    assert (plain["flags"] & 2).all()
    rec = Records(n, fill=255)
    r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_RECORD, rec)
    assert used == _ffi.PREFIX_NONE and rec.rho == 0.0 and bool((rec.d == 255).all())
    _same(plain, r, "recording call")
    r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_NONE
    _same(plain, r, "replaying call")


def test_a_batch_mixing_usable_and_unusable_records(ctx):
    """Every third record marked unusable by hand (depth 0, as the recording pass marks a ray it could not take a step with): those
    lanes start their rays in the fill next to lanes that replay."""
    from blackhole_geodesic_calculator_amd import _ffi
    import torch
    n = 209
    k0 = _rays(n, seed=6)
    p = _params(lambda_end=200.0, r_exit=40.0, disk_r_in=3.0, disk_r_out=12.0)
    plain, rec = _three(ctx, p, CAM, k0)
    words = rec.d[96 * n:].view(torch.int32).view(n, 4)
    words[::3, 1] = 0
    words[192:, 1] = 0          # ... and the whole partial batch
    rep, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain, rep, "mixed batch")


def test_an_object_sphere_inside_the_ball_refuses_replay_and_one_outside_does_not(ctx):
    n = 209
    k0 = _rays(n, seed=7)
    base = dict(lambda_end=200.0, r_exit=40.0)
    rho = 2.5
    for gap, replay in [(1.0, False), (rho, False), (rho * 1.001, True)]:   # inside, tangent, just outside
        sph = [[CAM[0], 0.0, CAM[2] - (2.0 + gap), 2.0]]
        plain, _ = _three(ctx, _params(**base), CAM, k0, spheres=sph, rec_p=_params(**base), rec_spheres=None, expect_replay=replay)
        assert (plain["flags"] == 0x88).sum() > n // 2      # the sphere sits right in front of the camera


def test_a_disk_set_after_recording_near_the_camera_refuses_replay(ctx):
    n = 209
    k0 = _rays(n, seed=8)
    x0 = np.array([20.0, 0.0, 1.0])
    base = dict(lambda_end=200.0, r_exit=40.0)
    disk = dict(disk_r_in=3.0, disk_r_out=25.0)
    plain, rec = _three(ctx, _params(**base, **disk), x0, k0, rec_p=_params(**base), expect_replay=False)
    assert rec.rho == pytest.approx(0.25 * (np.linalg.norm(x0) - 1.0), rel=1e-5) and rec.rho > 1.0      # (the horizon is nearest); |z0| = 1 < rho
    assert (plain["flags"] & 128).sum() > n // 2
    # ... and from high above the plane the same change of scene keeps the records
    _three(ctx, _params(**base, **disk), CAM, k0, rec_p=_params(**base), expect_replay=True)


@pytest.mark.parametrize("name,pkw", [("kerr", dict(lambda_end=50.0, rhs_form=2, spin=0.45)),
                                      ("rk4", dict(lambda_end=50.0, method=1, h_fixed=0.05)),
                                      ("time-like", dict(lambda_end=50.0, time_like=1))], ids=lambda v: v if isinstance(v, str) else "")
def test_calls_out_of_scope_ignore_the_records(ctx, name, pkw):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=9)
    p = _params(**pkw)
    plain, _ = _call(ctx, p, CAM, k0)
    rec = Records(n, fill=255)
    r, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD, rec)
    assert used == _ffi.PREFIX_NONE and bool((rec.d == 255).all())
    _same(plain, r, "recording call")
    rec.rho = 2.5
    r, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_NONE
    _same(plain, r, "replaying call")


def test_bad_prefix_arguments_are_refused(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    k0 = _rays(37, seed=1)
    rec = Records(37)
    with pytest.raises(_ffi.BhgError):
        _call(ctx, _params(), CAM, k0, 3, rec)                          # no such mode
    import torch
    rec.d = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert rec.d.data_ptr() == 0
    with pytest.raises(_ffi.BhgError):
        _call(ctx, _params(), CAM, k0, _ffi.PREFIX_RECORD, rec)         # no array


# ---- DeviceFrame ------------------------------------------------------------------------------------------------------------
def _frame(ctx, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    fr = DeviceFrame(ctx, 48, 40, 2, fov_x=0.6, fov_y=0.5, origin=CAM, **kw)
    fr.set_sky(synthetic_sky(64, 32))
    fr.generate_rays()
    return fr


def test_device_frame_records_once_and_replays_until_the_scene_comes_near(ctx, monkeypatch):
    import torch
    p = _params(lambda_end=200.0, r_exit=40.0)
    ref = _frame(ctx, start_cache=False)
    fr = _frame(ctx)
    ref.trace(p)
    want = ref.shade().cpu().numpy()
    for _ in range(3):
        fr.trace(p)
        assert np.array_equal(fr.shade().cpu().numpy(), want)
        assert torch.equal(fr.d_end, ref.d_end) and torch.equal(fr.d_steps, ref.d_steps)
    ss = fr.start_steps
    assert (ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (1, 2, 0) and ss.rho == pytest.approx(2.5, rel=1e-5)
    # an object sphere moves in front of the camera: that trace runs without the records, the next one with them again
    for sph, refused in [([[0.0, 0.0, 27.0, 2.0]], 1), ([[0.0, 0.0, 20.0, 2.0]], 1)]:
        for f in (fr, ref):
            f.set_objects(sph, [[1.0, 0.5, 0.2]])
            f.trace(p)
        assert torch.equal(fr.d_end, ref.d_end) and torch.equal(fr.d_flags, ref.d_flags) and torch.equal(fr.d_obj, ref.d_obj)
        assert ss.prefix_refused == refused
    assert ss.prefix_replayed == 3 and ss.prefix_recorded == 1
    # the switch of the records alone: the start steps carry on
    monkeypatch.setenv("BHGEO_START_PREFIX", "0")
    replayed = ss.replayed
    fr.trace(p)
    assert ss.prefix is None and ss.replayed == replayed + 1 and ss.prefix_replayed == 3
    assert torch.equal(fr.d_end, ref.d_end)


# ---- the library's own frame ------------------------------------------------------------------------------------------------
def test_library_frame_keeps_records_and_drops_them_when_a_sphere_comes_near(ctx, monkeypatch):
    """bhg_frame_render with the records against the same renders with BHGEO_START_PREFIX=0: a sphere far from the camera
    (replayed), one inside the ball (refused), far again (replayed again)."""
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    W, H, S = 48, 40, 2
    jitter = python_random_stream(42.0, 2 * S * W * H)
    sky = synthetic_sky(64, 32)
    p = _params(lambda_end=200.0, r_exit=40.0)
    scenes = [None, [[0.0, 0.0, 20.0, 2.0]], [[0.0, 0.0, 27.0, 2.0]], [[0.0, 0.0, 20.0, 2.0]], None]

    def renders():
        f = _ffi.Frame([0], W, H, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=jitter)
        out = []
        for sph in scenes:
            f.set_scene(sky, spheres=sph, sphere_rgb=None if sph is None else [[1.0, 0.5, 0.2]], lamps=[[10.0, 10.0, 30.0, 30.0]])
            out.append(f.render(p).copy())
        f.close()
        return out

    got = renders()
    monkeypatch.setenv("BHGEO_START_PREFIX", "0")
    want = renders()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[1], want[2]) and np.array_equal(want[1], want[3]) and np.array_equal(want[0], want[4])

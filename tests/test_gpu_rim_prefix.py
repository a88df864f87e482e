"""The rim start-up records (BHG_PREFIX_RECORD_RIM): the wide recording pass in the ball that ends just
above the horizon -- 1 - 2^-10 of min(clearance, |x0|) where the wide rule takes 15/16 -- with room for nine accepted steps in
fifteen attempts, and owners that earn it after the wide rule (BHGEO_RIM_PREFIX=1: rim from the first trace, =0: never).

What may never change is a result: every comparison of results below is array_equal -- end records, flags, n_steps, n_accepted --
between a plain call, a rim-recording call and a replaying call on the same rays, at one batch less a ray, one batch, one batch
and a ray, three batches and a partial one and 64 batches, with and without order_blocks.  What the records hold is checked
against the DEVICE's own attempts (the plain call under a step budget of m = 1 .. 15 attempts says exactly which attempt each
ray had accepted and where it stood after it)."""
import numpy as np
import pytest

from conftest import CAM, frame_rays

pytestmark = pytest.mark.gpu

ACC_MAX, ATT_MAX = 9, 15
NAN_RAY = 7
F_MAX_STEPS, F_STEP_TOO_SMALL = 16, 32
FRACTION = 1.0 - 2.0 ** -10
RIM_RHO = FRACTION * (float(np.linalg.norm(CAM)) - 1.0)           # 28.97168 but for the camera's 1e-4 off the axis
WIDE_RHO = 0.9375 * (float(np.linalg.norm(CAM)) - 1.0)


def _params(**kw):
    from blackhole_geodesic_calculator_amd import _ffi
    kw.setdefault("max_steps", 20000)
    return _ffi.make_params(**kw)


def _rays(n, seed, fov=0.6):
    """Seeded rays of the headline window with a NaN direction, a zero direction and two rays at the hole among them."""
    k0 = frame_rays(n, seed=seed, fov=fov)
    k0[NAN_RAY] = np.nan
    k0[n // 2] = 0.0
    k0[3] = [0.0, 0.0, -1.0]
    k0[5] = [0.02, -0.01, -1.0] / np.linalg.norm([0.02, -0.01, -1.0])
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

    def position(self):
        d = self.planes()[0]
        return np.stack([d[0, :, 0], d[0, :, 1], d[1, :, 0]], 1)


def _call(ctx, p, x0, k0, mode=0, rec=None, spheres=None):
    """One shared-origin device trace call; every output as numpy, and what the call reports about the records."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    n = len(k0)
    d_k0 = torch.as_tensor(k0).cuda()
    out = torch.full((n, 6), 123.0, dtype=torch.float64, device="cuda")
    fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st, ac = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    obj = torch.full((n,), 99, dtype=torch.int8, device="cuda")
    pf = None if rec is None else _ffi.Prefix(rec.d.data_ptr(), rec.rho, mode, -1)
    ctx.trace_device(p, n, d_k0.data_ptr(), out.data_ptr(), spheres=spheres, d_object_id=obj.data_ptr() if spheres is not None else 0,
                     x0_shared=x0, d_flags=fl.data_ptr(), d_n_steps=st.data_ptr(), d_n_accepted=ac.data_ptr(), d_start_steps=0,
                     start_mode=0, prefix=pf)
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy(), "flags": fl.cpu().numpy(), "n_steps": st.cpu().numpy(), "n_accepted": ac.cpu().numpy()}
    if spheres is not None:
        res["object_id"] = obj.cpu().numpy()
    used = None
    if pf is not None:
        used = pf.used
        if mode != _ffi.PREFIX_REPLAY:
            rec.rho = pf.rho
    return res, used


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _three(ctx, p, x0, k0, spheres=None, mode=None):
    """plain / rim-recording / replaying call.  Returns (plain result, Records)."""
    from blackhole_geodesic_calculator_amd import _ffi
    mode = _ffi.PREFIX_RECORD_RIM if mode is None else mode
    plain, _ = _call(ctx, p, x0, k0, spheres=spheres)
    rec = Records(len(k0))
    r, used = _call(ctx, p, x0, k0, mode, rec, spheres=spheres)
    assert used == mode and rec.rho > 0.0
    _same(plain, r, "recording call")
    before = rec.d.clone()
    rep, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rec, spheres=spheres)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain, rep, "replaying call")
    assert bool((rec.d == before).all()), "a replaying call wrote into the records"
    return plain, rec


def _expected_records(trace_m, n, x0, rho, acc_max=ACC_MAX, att_max=ATT_MAX):
    """The recorder's rule restated, lane per ray, on the outcome of plain traces under a step budget of m = 1 .. att_max attempts:
    trace_m(m) -> (flags, n_attempted, n_accepted, position) of every ray.  A ray that still runs after m attempts carries
    BHG_FLAG_MAX_STEPS with n_attempted == m and stands where attempt m left it; attempt m was accepted when n_accepted grew.
    Rejected attempts are kept; the record stops in front of the first attempt that ends or flags the ray, in front of an
    accepted attempt that leaves the ball, at acc_max accepted steps and at att_max attempts.  Returns (attempted, accepted,
    rejected bit)."""
    att, acc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rej, alive = np.zeros(n, bool), np.ones(n, bool)
    prev = np.zeros(n, np.uint32)
    for m in range(1, att_max + 1):
        flags, natt, nacc, pos = trace_m(m)
        going = ((flags & F_MAX_STEPS) != 0) & (natt == m)
        accepted = nacc > prev
        inside = np.linalg.norm(pos - np.asarray(x0), axis=1) <= rho
        keep = alive & going & (acc < acc_max) & (~accepted | inside)
        att[keep], acc[keep], rej[keep] = m, nacc[keep], ~accepted[keep]
        alive, prev = keep, nacc
    return att, acc, rej


# the event-free kernel variants <rhs, 0>, where the rim ball applies
FREE_VARIANTS = [("<0,0>", dict(lambda_end=50.0)), ("<1,0>", dict(lambda_end=50.0, rhs_form=1))]
SIZES = [63, 64, 65, 209, 4096]


@pytest.mark.parametrize("order_blocks", [0, 4], ids=["in_order", "order_blocks_4"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,pkw", FREE_VARIANTS, ids=[v[0] for v in FREE_VARIANTS])
def test_rim_record_and_replay_equal_the_plain_call(ctx, name, pkw, n, order_blocks):
    from blackhole_geodesic_calculator_amd import _ffi
    k0 = _rays(n, seed=n)
    p = _params(order_blocks=order_blocks, **pkw)
    plain, rec = _three(ctx, p, CAM, k0)
    d, w = rec.planes()
    att, acc, bits = w[:, 1], w[:, 2], w[:, 3]
    ok = att > 0
    print(name, n, order_blocks, "rho", rec.rho, "attempts kept per ray", att.mean(), "| attempted",
          np.bincount(att, minlength=ATT_MAX + 1).tolist(), "accepted", np.bincount(acc, minlength=ACC_MAX + 1).tolist())
    assert _ffi.prefix_clearance(p, CAM) == pytest.approx(float(np.linalg.norm(CAM)) - 1.0, rel=1e-12)
    assert rec.rho == pytest.approx(RIM_RHO, rel=1e-12) and rec.rho == pytest.approx(28.9716796875, rel=1e-5)
    # the record invariants
    assert np.array_equal(w[:, 0], np.arange(n))
    assert np.all(acc <= att) and att.max() <= ATT_MAX and acc.max() <= ACC_MAX and np.all(bits <= 1)
    assert ok.sum() >= n - 1 and acc[NAN_RAY] == 0            # (the NaN direction is rejected attempt after attempt)
    assert np.all(np.linalg.norm(rec.position()[ok] - CAM, axis=1) <= rec.rho)
    assert np.all(np.linalg.norm(rec.position()[ok], axis=1) > 1.0)               # (no kept state on or inside the horizon)
    gave_up = (plain["flags"] & (F_MAX_STEPS | F_STEP_TOO_SMALL)) != 0
    assert np.all(plain["n_steps"][ok & ~gave_up] > att[ok & ~gave_up]) and np.all(plain["n_steps"][ok] >= att[ok])
    assert np.all(plain["n_accepted"][ok] >= acc[ok])
    finite = ok & (np.arange(n) != NAN_RAY)
    assert np.all(d[5, finite, 1] < p.lambda_end) and np.all(d[4, finite, 1] > 0.0)
    assert not bits[acc == att].any()                     # (a record without a rejected attempt cannot end on one)
    # the wide rule on the same rays keeps no more for any ray: the same recorder stopped earlier
    wide = Records(n)
    r5, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD_WIDE, wide)
    assert used == _ffi.PREFIX_RECORD_WIDE and wide.rho == pytest.approx(WIDE_RHO, rel=1e-12)
    _same(plain, r5, "wide-recording call")
    assert np.all(wide.planes()[1][:, 1] <= att) and (n < 200 or wide.planes()[1][:, 1].sum() < att.sum())


@pytest.mark.parametrize("name,pkw", FREE_VARIANTS + [("<0,1>", dict(lambda_end=200.0, r_exit=70.0))], ids=["<0,0>", "<1,0>", "<0,1>"])
def test_the_rim_records_restate_the_devices_own_attempts_exactly(ctx, name, pkw):
    """No tolerance: the plain DEVICE call under a step budget of m attempts tells which attempt was accepted and where the ray
    stood after it, and the records -- counts, rejected bit, kept state -- must be that, ray for ray, with the rim rule's ball and
    its caps of nine accepted steps and fifteen attempts.  (An exit sphere at 70 stands 40 from the camera, farther than the
    horizon: the rim ball applies to that variant too.)"""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=n)
    rec = Records(n)
    _, used = _call(ctx, _params(**pkw), CAM, k0, _ffi.PREFIX_RECORD_RIM, rec)
    assert used == _ffi.PREFIX_RECORD_RIM and rec.rho == pytest.approx(RIM_RHO, rel=1e-12)
    states = {}

    def trace_m(m):
        r, _ = _call(ctx, _params(**dict(pkw, max_steps=m)), CAM, k0)
        states[m] = r
        return r["flags"], r["n_steps"].astype(np.uint32), r["n_accepted"].astype(np.uint32), r["out"][:, :3]

    e_att, e_acc, e_rej = _expected_records(trace_m, n, CAM, rec.rho)
    d, w = rec.planes()
    assert np.array_equal(w[:, 1], e_att) and np.array_equal(w[:, 2], e_acc) and np.array_equal(w[:, 3] == 1, e_rej)
    assert (e_att > e_acc).any()
    # the rim ball and its caps hold what the wide rule's would cut off
    again = lambda m: (states[m]["flags"], states[m]["n_steps"].astype(np.uint32), states[m]["n_accepted"].astype(np.uint32),   # noqa: E731
                       states[m]["out"][:, :3])
    e_wide = _expected_records(again, n, CAM, WIDE_RHO, acc_max=8, att_max=12)
    assert np.all(e_wide[0] <= e_att) and e_att.sum() > e_wide[0].sum() and e_att.max() > 12
    x, v = rec.position(), np.stack([d[1, :, 1], d[2, :, 0], d[2, :, 1]], 1)
    for i in np.nonzero(e_att)[0]:
        end = states[int(e_att[i])]["out"][i]
        assert np.array_equal(x[i], end[:3], equal_nan=True) and np.array_equal(v[i], end[3:], equal_nan=True), i


ONE_SPHERE = [[1.0, 0.5, 12.0, 2.0]]
LOW = np.array([25.0, 0.0, 5.0])        # 5 above the disk plane, 24.5 from the horizon
# the kernel variants with events, in scenes that keep the old rho: (name, params, object spheres, origin)
OLD_RHO = [
    ("<0,1>", dict(lambda_end=200.0, r_exit=45.0), None, CAM),                                       # the exit sphere 15 away
    ("<0,3>", dict(lambda_end=200.0, r_exit=70.0, disk_r_in=3.0, disk_r_out=12.0), None, LOW),       # the disk plane 5 away
    ("<0,3>exit", dict(lambda_end=200.0, r_exit=45.0, disk_r_in=3.0, disk_r_out=12.0), None, CAM),   # the exit sphere again
    ("<0,5>", dict(lambda_end=200.0, r_exit=70.0), ONE_SPHERE, CAM),                                 # any object sphere
]


@pytest.mark.parametrize("n", [209, 4096])
@pytest.mark.parametrize("name,pkw,spheres,x0", OLD_RHO, ids=[v[0] for v in OLD_RHO])
def test_scenes_that_keep_the_old_rho_get_the_wide_modes_bytes(ctx, name, pkw, spheres, x0, n):
    """An exit sphere or a disk plane nearer than the horizon, or any object sphere: the quarter as by every rule since the
    first, and under the rim mode the records of BHG_PREFIX_RECORD_WIDE byte for byte -- and plain = record = replay."""
    from blackhole_geodesic_calculator_amd import _ffi
    k0 = _rays(n, seed=n + 1)
    p = _params(order_blocks=4 if n == 4096 else 0, **pkw)
    plain, rec = _three(ctx, p, x0, k0, spheres=spheres)
    clear = _ffi.prefix_clearance(p, x0, spheres)
    assert rec.rho == pytest.approx(0.25 * clear, rel=1e-12) and clear < float(np.linalg.norm(x0)) - 1.0
    wide = Records(n)
    r5, used = _call(ctx, p, x0, k0, _ffi.PREFIX_RECORD_WIDE, wide, spheres=spheres)
    assert used == _ffi.PREFIX_RECORD_WIDE and wide.rho == rec.rho
    _same(plain, r5, "wide-recording call")
    assert bool((wide.d == rec.d).all()), "rim-mode records differ from the wide mode's where the rho is unchanged"
    w = rec.planes()[1]
    assert w[:, 1].max() <= 12 and w[:, 2].max() <= 6 and (w[:, 1] > 0).sum() >= n - 1


# ---- refusals: a surface between the wide ball and the rim ball -------------------------------------------------------------------
SIDE = np.array([9.0, 0.0, 28.5])        # |x0| = 29.887: wide ball 27.08, rim ball 28.86, the disk plane 28.5 away
BETWEEN = [
    # (name, origin, the scene of the replaying call: params, spheres)
    ("exit_sphere", CAM, dict(lambda_end=200.0, r_exit=58.5), None),                                           # 28.5 from the camera
    ("object_sphere", CAM, dict(lambda_end=200.0), [[7.67, 0.0, -0.04, 3.0]]),          # beside the hole, in the window: its surface 28.0 away
    ("disk_annulus", SIDE, dict(lambda_end=200.0, disk_r_in=3.0, disk_r_out=12.0), None),
]


@pytest.mark.parametrize("name,x0,pkw,spheres", BETWEEN, ids=[b[0] for b in BETWEEN])
def test_a_surface_between_the_wide_and_the_rim_ball_is_refused(ctx, name, x0, pkw, spheres):
    """Records written in the free scene; the replaying call's scene puts a surface inside the rim ball and outside the wide one:
    rim records are refused, wide records of the same rays are replayed, and both calls return the plain call's bits."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=21)
    free = _params(lambda_end=200.0)
    _, rim = _three(ctx, free, x0, k0)
    _, wide = _three(ctx, free, x0, k0, mode=_ffi.PREFIX_RECORD_WIDE)
    r0 = float(np.linalg.norm(x0))
    assert rim.rho == pytest.approx(FRACTION * (r0 - 1.0), rel=1e-12) and wide.rho == pytest.approx(0.9375 * (r0 - 1.0), rel=1e-12)
    p = _params(**pkw)
    clear = _ffi.prefix_clearance(p, x0, spheres)
    assert wide.rho * (1.0 + 1e-6) < clear < rim.rho
    plain, _ = _call(ctx, p, x0, k0, spheres=spheres)
    before = rim.d.clone()
    r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rim, spheres=spheres)
    assert used == _ffi.PREFIX_NONE
    _same(plain, r, "refused replaying call")
    assert bool((rim.d == before).all())
    r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, wide, spheres=spheres)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain, r, "replaying call on wide records")
    free_plain, _ = _call(ctx, free, x0, k0)
    assert any(not np.array_equal(plain[k], free_plain[k], equal_nan=True) for k in free_plain)       # (the surface is met by some ray)


def test_a_surface_tangent_to_the_rim_ball_is_refused(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=22)
    _, rec = _three(ctx, _params(lambda_end=200.0), CAM, k0)
    r0 = float(np.linalg.norm(CAM))
    for r_exit, want in ((r0 + rec.rho, _ffi.PREFIX_NONE), (r0 + rec.rho * (1.0 + 0.5e-6), _ffi.PREFIX_NONE),
                         (r0 + rec.rho * (1.0 + 3e-6), _ffi.PREFIX_REPLAY)):
        p = _params(lambda_end=200.0, r_exit=r_exit)
        plain, _ = _call(ctx, p, CAM, k0)
        r, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_REPLAY, rec)
        assert used == want, r_exit
        _same(plain, r, "tangent")


def test_the_step_budget_must_exceed_what_a_rim_record_may_hold(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=4)
    # max_steps = 15: nothing is written, the buffer is untouched
    p15 = _params(lambda_end=50.0, max_steps=ATT_MAX)
    plain15, _ = _call(ctx, p15, CAM, k0)
    rec = Records(n, fill=255)
    r, used = _call(ctx, p15, CAM, k0, _ffi.PREFIX_RECORD_RIM, rec)
    assert used == _ffi.PREFIX_NONE and rec.rho == 0.0 and bool((rec.d == 255).all())
    _same(plain15, r, "refused recording call")
    # max_steps = 16: written, and the replay ends every ray where the plain call does (most of them on the budget)
    p16 = _params(lambda_end=50.0, max_steps=ATT_MAX + 1)
    plain16, rec = _three(ctx, p16, CAM, k0)
    assert (plain16["flags"] & F_MAX_STEPS).sum() > 0 and rec.planes()[1][:, 1].max() <= ATT_MAX
    # a replay of rim records with max_steps at the cap is an error, and writes nothing
    before = rec.d.clone()
    for m in (ATT_MAX, 13):
        with pytest.raises(_ffi.BhgError) as e:
            _call(ctx, _params(lambda_end=50.0, max_steps=m), CAM, k0, _ffi.PREFIX_REPLAY, rec)
        assert e.value.code == _ffi.E_INVALID
    assert bool((rec.d == before).all())
    # ... the context is as good as before
    rep, used = _call(ctx, p16, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain16, rep, "replay after the refused ones")
    # at or below the wide rule's cap of 12 a replay of any records is answered as ever: none used, the plain bits
    p12 = _params(lambda_end=50.0, max_steps=12)
    plain12, _ = _call(ctx, p12, CAM, k0)
    rep, used = _call(ctx, p12, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_NONE
    _same(plain12, rep, "replay under the old cap")
    # wide records replay at 13 as they always did: their rho tells them from rim records
    plain13, _ = _call(ctx, _params(lambda_end=50.0, max_steps=13), CAM, k0)
    wide = Records(n)
    _call(ctx, p16, CAM, k0, _ffi.PREFIX_RECORD_WIDE, wide)
    rep, used = _call(ctx, _params(lambda_end=50.0, max_steps=13), CAM, k0, _ffi.PREFIX_REPLAY, wide)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain13, rep, "wide records at 13")


def test_depth_of_the_rim_records_on_the_headline_window(ctx):
    """4 096 uniform rays of the headline window from the bench camera at the bench's parameters.  The rule was chosen on a CPU
    restatement (scipy RK45, 3 000 rays): 8.38 attempts kept per ray against the wide rule's 7.85, 0.4 % of the rays at a cap.
    Stated here: at least 0.35 attempts per ray more than the wide rule on the same rays (the figure below which the rule would
    not have been built), at most 1 % of the records at a cap."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 4096
    k0 = np.ascontiguousarray(frame_rays(n, seed=11, fov=0.6))
    p = _params(lambda_end=50.0, order_blocks=4)
    plain, rec = _three(ctx, p, CAM, k0)
    w = rec.planes()[1]
    att, acc = w[:, 1], w[:, 2]
    wide = Records(n)
    _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD_WIDE, wide)
    watt = wide.planes()[1][:, 1]
    print("rho", rec.rho, "attempts kept per ray: rim", att.mean(), "wide", watt.mean(), "of", plain["n_steps"].mean(),
          "| accepted", np.bincount(acc, minlength=ACC_MAX + 1).tolist(), "attempted", np.bincount(att, minlength=ATT_MAX + 1).tolist())
    assert rec.rho == pytest.approx(28.9716796875, rel=1e-5)
    assert att.mean() >= watt.mean() + 0.35
    assert ((acc == ACC_MAX) | (att == ATT_MAX)).mean() <= 0.01
    assert att.max() <= ATT_MAX and acc.max() <= ACC_MAX


# ---- refusal, then recovery: the two owners ---------------------------------------------------------------------------------
FREE, SHUT = dict(lambda_end=200.0), dict(lambda_end=200.0, r_exit=58.5)      # (an exit sphere 28.5 from the camera: in the rim ball only)
R, W, M, D, NO = 2, 5, 6, 4, 0
# the script: (scene, what the owner asks for, what the library answers, the records' rho after the call)
SCRIPT = ([(FREE, M, M, 28.9716796875)] + [(SHUT, R, NO, 28.9716796875)] * 2 + [(SHUT, M, M, 7.125)] + [(SHUT, R, R, 7.125)] * 2 +
          [(FREE, R, R, 7.125)] * 8 + [(FREE, M, M, 28.9716796875)] + [(FREE, R, R, 28.9716796875)] * 2)


def _frame(ctx, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    fr = DeviceFrame(ctx, 48, 40, 2, fov_x=0.6, fov_y=0.5, origin=CAM, **kw)
    fr.set_sky(synthetic_sky(64, 32))
    fr.generate_rays()
    return fr


def test_device_frame_recovers_from_a_surface_inside_the_rim_ball(ctx, monkeypatch):
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    assert (_ffi.PREFIX_REPLAY, _ffi.PREFIX_RECORD_WIDE, _ffi.PREFIX_RECORD_RIM, _ffi.PREFIX_RECORD_DEEP, _ffi.PREFIX_NONE) == (R, W, M, D, NO)
    monkeypatch.delenv("BHGEO_WIDE_PREFIX", raising=False)
    monkeypatch.setenv("BHGEO_RIM_PREFIX", "1")          # an owner that records by the rim rule from its first trace
    ref, fr = _frame(ctx, start_cache=False), _frame(ctx)
    ss = fr.start_steps
    plain = {}
    for k, (pkw, ask, used, rho) in enumerate(SCRIPT):
        p = _params(**pkw)
        key = tuple(sorted(pkw.items()))
        if key not in plain:
            ref.trace(p)
            plain[key] = (ref.d_end.clone(), ref.d_flags.clone(), ref.d_steps.clone(), ref.d_acc.clone(), ref.shade().cpu().numpy())
        fr.trace(p)
        assert (ss.prefix.mode, ss.prefix.used) == (ask, used), k
        for a, b in zip((fr.d_end, fr.d_flags, fr.d_steps, fr.d_acc), plain[key]):
            assert torch.equal(a, b), k
        assert np.array_equal(fr.shade().cpu().numpy(), plain[key][4]), k
        assert ss.rho == pytest.approx(rho, rel=1e-5), k
        assert (ss.recorded, ss.replayed) == (1, k), k        # (the start steps are recorded once)
    assert (ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (3, 12, 2)
    assert not torch.equal(plain[tuple(sorted(FREE.items()))][1], plain[tuple(sorted(SHUT.items()))][1])
    # a step budget that rim records could exhaust: the owner asks for nothing in that trace, keeps its records, replays after it
    tight = _params(lambda_end=200.0, max_steps=ATT_MAX)
    ref.trace(tight)
    fr.trace(tight)
    assert ss.prefix is None and torch.equal(fr.d_end, ref.d_end) and torch.equal(fr.d_steps, ref.d_steps)
    fr.trace(_params(**FREE))
    assert (ss.prefix.mode, ss.prefix.used) == (R, R) and torch.equal(fr.d_end, plain[tuple(sorted(FREE.items()))][0])


def test_library_frame_recovers_from_a_surface_inside_the_rim_ball(ctx, monkeypatch):
    """bhg_frame_render on the same script: what each render asked of the records and was told (bhg_frame_prefix_info), and its
    image against the same frame's without the records (BHGEO_START_PREFIX=0)."""
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    Wd, Ht, S = 48, 40, 2
    jitter = python_random_stream(42.0, 2 * S * Wd * Ht)
    sky = synthetic_sky(64, 32)

    def frame():
        f = _ffi.Frame([0], Wd, Ht, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=jitter)
        f.set_scene(sky, lamps=[[10.0, 10.0, 30.0, 30.0]])
        return f

    monkeypatch.delenv("BHGEO_WIDE_PREFIX", raising=False)
    monkeypatch.setenv("BHGEO_RIM_PREFIX", "1")
    f = frame()
    got, told = [], []
    for pkw, ask, used, rho in SCRIPT:
        got.append(f.render(_params(**pkw)).copy())
        told.append(f.prefix_info())
    tight = f.render(_params(lambda_end=200.0, max_steps=ATT_MAX)).copy()
    told_tight = f.prefix_info()
    after = f.render(_params(**FREE)).copy()
    told_after = f.prefix_info()
    f.close()
    for k, ((pkw, ask, used, rho), (t_mode, t_used, t_rho)) in enumerate(zip(SCRIPT, told)):
        assert (t_mode, t_used) == (ask, used), (k, told)
        assert t_rho == pytest.approx(rho, rel=1e-5), k
    assert told_tight[:2] == (NO, NO) and told_after[:2] == (R, R) and told_after[2] == pytest.approx(28.9716796875, rel=1e-5)
    monkeypatch.setenv("BHGEO_START_PREFIX", "0")
    f = frame()
    want = {}
    for pkw in (FREE, SHUT):
        want[tuple(sorted(pkw.items()))] = f.render(_params(**pkw)).copy()
        assert f.prefix_info()[:2] == (NO, NO)
    want_tight = f.render(_params(lambda_end=200.0, max_steps=ATT_MAX)).copy()
    f.close()
    for k, ((pkw, _, _, _), g) in enumerate(zip(SCRIPT, got)):
        assert np.array_equal(g, want[tuple(sorted(pkw.items()))]), k
    assert np.array_equal(tight, want_tight) and np.array_equal(after, want[tuple(sorted(FREE.items()))])


RIM_RUN = 96
WIDE_AT, RIM_AT = 33, 34 + RIM_RUN   # (0-based: the 34th and the 131st trace of a ray set)


def test_owners_climb_the_ladder_deep_wide_rim(ctx, monkeypatch):
    """The owners' default: the first trace records by the deep rule (21.75), the 34th by the wide rule (27.1875) exactly as
    before there was a rim rule, the 131st by the rim rule (28.97), and the traces after it replay those -- every result the plain
    trace's.  BHGEO_RIM_PREFIX=0: the ladder ends at the wide rule.  DeviceFrame, then bhg_frame."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    monkeypatch.delenv("BHGEO_WIDE_PREFIX", raising=False)
    monkeypatch.delenv("BHGEO_RIM_PREFIX", raising=False)
    p = _params(**FREE)
    ref, fr = _frame(ctx, start_cache=False), _frame(ctx)
    ref.trace(p)
    want = (ref.d_end.clone(), ref.d_flags.clone(), ref.d_steps.clone(), ref.d_acc.clone())
    ss = fr.start_steps
    asked = []
    for k in range(RIM_AT + 3):
        fr.trace(p)
        asked.append((ss.prefix.mode, ss.prefix.used))
        for a, b in zip((fr.d_end, fr.d_flags, fr.d_steps, fr.d_acc), want):
            assert torch.equal(a, b), k
        assert ss.rho == pytest.approx(21.75 if k < WIDE_AT else 27.1875 if k < RIM_AT else 28.9716796875, rel=1e-5), k
    ladder = [(D, D)] + [(R, R)] * 32 + [(W, W)] + [(R, R)] * RIM_RUN + [(M, M)] + [(R, R)] * 2
    assert asked == ladder
    assert (ss.recorded, ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (1, 3, 34 + RIM_RUN, 0)
    words = ss.d_rec[96 * fr.n:].view(torch.int32).view(fr.n, 4).cpu().numpy()
    assert words[:, 1].max() <= ATT_MAX and words[:, 2].max() <= ACC_MAX
    # the library's frame
    Wd, Ht, S = 48, 40, 2

    def frame():
        f = _ffi.Frame([0], Wd, Ht, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=python_random_stream(42.0, 2 * S * Wd * Ht))
        f.set_scene(synthetic_sky(64, 32), lamps=[[10.0, 10.0, 30.0, 30.0]])
        return f

    f = frame()
    told, imgs = [], []
    for k in range(RIM_AT + 3):
        imgs.append(f.render(p).copy())
        told.append(f.prefix_info())
    f.close()
    assert [t[:2] for t in told] == ladder
    assert told[0][2] == pytest.approx(21.75, rel=1e-5) and told[WIDE_AT][2] == pytest.approx(27.1875, rel=1e-5)
    assert told[-1][2] == pytest.approx(28.9716796875, rel=1e-5)
    for k, im in enumerate(imgs):
        assert np.array_equal(im, imgs[0]), k
    # BHGEO_RIM_PREFIX=0: never promoted past the wide rule, both owners
    monkeypatch.setenv("BHGEO_RIM_PREFIX", "0")
    fr = _frame(ctx)
    ss = fr.start_steps
    asked = []
    for k in range(RIM_AT + 3):
        fr.trace(p)
        asked.append((ss.prefix.mode, ss.prefix.used))
    assert asked == [(D, D)] + [(R, R)] * 32 + [(W, W)] + [(R, R)] * (RIM_RUN + 3) and ss.rho == pytest.approx(27.1875, rel=1e-5)
    assert torch.equal(fr.d_end, want[0]) and torch.equal(fr.d_steps, want[2])
    f = frame()
    told = []
    for k in range(RIM_AT + 3):
        f.render(p)
        told.append(f.prefix_info()[:2])
    f.close()
    assert told == [(D, D)] + [(R, R)] * 32 + [(W, W)] + [(R, R)] * (RIM_RUN + 3)

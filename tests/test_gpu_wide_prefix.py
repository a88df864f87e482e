"""The wide start-up records (BHG_PREFIX_RECORD_WIDE): the deep recording pass in fifteen sixteenths of
the clear ball about the camera, with room for eight accepted steps, and owners that record again after refusals and are
promoted from the deep rule to the wide one by a long run of replaying traces (BHGEO_WIDE_PREFIX=1: wide from the first trace).

What may never change is a result: every comparison of results below is array_equal -- end records, flags, n_steps, n_accepted,
object ids -- between a plain call, a wide-recording call and a replaying call on the same rays, for every kernel variant in scope,
at one batch less a ray, one batch, one batch and a ray, three batches and a partial one and 64 batches, with and without
order_blocks.  What the records hold is checked against the DEVICE's own attempts (the plain call under a step budget of
m = 1 .. 12 attempts says exactly which attempt each ray had accepted and where it stood after it), and how deep they are on
4 096 rays of the headline window against the figures the rule was chosen by."""
import numpy as np
import pytest

from conftest import CAM, frame_rays

pytestmark = pytest.mark.gpu

ACC_MAX, ATT_MAX = 8, 12
NAN_RAY = 7
F_MAX_STEPS, F_STEP_TOO_SMALL = 16, 32
WIDE_RHO = 0.9375 * (float(np.linalg.norm(CAM)) - 1.0)         # 27.1875 but for the camera's 1e-4 off the axis


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


def _three(ctx, p, x0, k0, spheres=None):
    """plain / wide-recording / replaying call.  Returns (plain result, Records)."""
    from blackhole_geodesic_calculator_amd import _ffi
    plain, _ = _call(ctx, p, x0, k0, spheres=spheres)
    rec = Records(len(k0))
    r, used = _call(ctx, p, x0, k0, _ffi.PREFIX_RECORD_WIDE, rec, spheres=spheres)
    assert used == _ffi.PREFIX_RECORD_WIDE and rec.rho > 0.0
    _same(plain, r, "recording call")
    before = rec.d.clone()
    rep, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rec, spheres=spheres)
    assert used == _ffi.PREFIX_REPLAY
    _same(plain, rep, "replaying call")
    assert bool((rec.d == before).all()), "a replaying call wrote into the records"
    return plain, rec


def _expected_records(trace_m, n, x0, rho, acc_max=ACC_MAX):
    """The recorder's rule restated, lane per ray, on the outcome of plain traces under a step budget of m = 1 .. 12 attempts:
    trace_m(m) -> (flags, n_attempted, n_accepted, position) of every ray.  A ray that still runs after m attempts carries
    BHG_FLAG_MAX_STEPS with n_attempted == m and stands where attempt m left it; attempt m was accepted when n_accepted grew.
    Rejected attempts are kept; the record stops in front of the first attempt that ends or flags the ray, in front of an
    accepted attempt that leaves the ball, at acc_max accepted steps and at 12 attempts.  Returns (attempted, accepted, rejected bit)."""
    att, acc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rej, alive = np.zeros(n, bool), np.ones(n, bool)
    prev = np.zeros(n, np.uint32)
    for m in range(1, ATT_MAX + 1):
        flags, natt, nacc, pos = trace_m(m)
        going = ((flags & F_MAX_STEPS) != 0) & (natt == m)
        accepted = nacc > prev
        inside = np.linalg.norm(pos - np.asarray(x0), axis=1) <= rho
        keep = alive & going & (acc < acc_max) & (~accepted | inside)
        att[keep], acc[keep], rej[keep] = m, nacc[keep], ~accepted[keep]
        alive, prev = keep, nacc
    return att, acc, rej


ONE_SPHERE = [[1.0, 0.5, 12.0, 2.0]]
# the kernel variants <rhs, events> in scope: (name, params, object spheres).  The exit sphere (70: 40 from the camera) and the disk
# plane (30 below it) stand farther off than the horizon (29), so the object-free variants record in the wide ball; one object
# sphere anywhere means the quarter.
VARIANTS = [
    ("<0,0>", dict(lambda_end=50.0), None),
    ("<1,0>", dict(lambda_end=50.0, rhs_form=1), None),
    ("<0,1>", dict(lambda_end=200.0, r_exit=70.0), None),
    ("<0,3>", dict(lambda_end=200.0, r_exit=70.0, disk_r_in=3.0, disk_r_out=12.0), None),
    ("<0,5>", dict(lambda_end=200.0, r_exit=70.0), ONE_SPHERE),
]
SIZES = [63, 64, 65, 209, 4096]


@pytest.mark.parametrize("order_blocks", [0, 4], ids=["in_order", "order_blocks_4"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,pkw,spheres", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wide_record_and_replay_equal_the_plain_call(ctx, name, pkw, spheres, n, order_blocks):
    from blackhole_geodesic_calculator_amd import _ffi
    k0 = _rays(n, seed=n)
    p = _params(order_blocks=order_blocks, **pkw)
    plain, rec = _three(ctx, p, CAM, k0, spheres=spheres)
    clear = _ffi.prefix_clearance(p, CAM, spheres)
    d, w = rec.planes()
    att, acc, bits = w[:, 1], w[:, 2], w[:, 3]
    ok = att > 0
    print(name, n, order_blocks, "rho", rec.rho, "attempts kept per ray", att.mean(), "| attempted",
          np.bincount(att, minlength=ATT_MAX + 1).tolist(), "accepted", np.bincount(acc, minlength=ACC_MAX + 1).tolist())
    if spheres is None:
        assert clear == pytest.approx(float(np.linalg.norm(CAM)) - 1.0, rel=1e-12)         # (the horizon is the nearest surface)
        assert rec.rho == pytest.approx(WIDE_RHO, rel=1e-12) and rec.rho == pytest.approx(27.1875, rel=1e-5)
    else:
        # the quarter rule: the records are the deep rule's, byte for byte
        assert rec.rho == pytest.approx(0.25 * clear, rel=1e-12) and rec.rho < 5.0
        deep = Records(n)
        r4, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD_DEEP, deep, spheres=spheres)
        assert used == _ffi.PREFIX_RECORD_DEEP and deep.rho == rec.rho
        _same(plain, r4, "deep-recording call")
        assert bool((deep.d == rec.d).all()), "wide records next to an object sphere differ from the deep rule's"
    # the record invariants
    assert np.array_equal(w[:, 0], np.arange(n))
    assert np.all(acc <= att) and att.max() <= ATT_MAX and acc.max() <= ACC_MAX and np.all(bits <= 1)
    assert ok.sum() >= n - 1 and acc[NAN_RAY] == 0            # (the NaN direction is rejected attempt after attempt)
    assert np.all(np.linalg.norm(rec.position()[ok] - CAM, axis=1) <= rec.rho)
    gave_up = (plain["flags"] & (F_MAX_STEPS | F_STEP_TOO_SMALL)) != 0
    assert np.all(plain["n_steps"][ok & ~gave_up] > att[ok & ~gave_up]) and np.all(plain["n_steps"][ok] >= att[ok])
    assert np.all(plain["n_accepted"][ok] >= acc[ok])
    finite = ok & (np.arange(n) != NAN_RAY)
    assert np.all(d[5, finite, 1] < p.lambda_end) and np.all(d[4, finite, 1] > 0.0)
    assert not bits[acc == att].any()                     # (a record without a rejected attempt cannot end on one)


@pytest.mark.parametrize("name,pkw,spheres", [VARIANTS[0], VARIANTS[2], VARIANTS[3], VARIANTS[4]], ids=["<0,0>", "<0,1>", "<0,3>", "<0,5>"])
def test_the_wide_records_restate_the_devices_own_attempts_exactly(ctx, name, pkw, spheres):
    """No tolerance: the plain DEVICE call under a step budget of m attempts tells which attempt was accepted and where the ray
    stood after it, and the records -- counts, rejected bit, kept state -- must be that, ray for ray, with the wide rule's ball
    and its cap of eight accepted steps."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=n)
    rec = Records(n)
    _, used = _call(ctx, _params(**pkw), CAM, k0, _ffi.PREFIX_RECORD_WIDE, rec, spheres=spheres)
    assert used == _ffi.PREFIX_RECORD_WIDE
    states = {}

    def trace_m(m):
        r, _ = _call(ctx, _params(**dict(pkw, max_steps=m)), CAM, k0, spheres=spheres)
        states[m] = r
        return r["flags"], r["n_steps"].astype(np.uint32), r["n_accepted"].astype(np.uint32), r["out"][:, :3]

    # (the cap of eight goes with the wide ball: in the quarter ball next to an object sphere the rule is the deep rule whole, six)
    e_att, e_acc, e_rej = _expected_records(trace_m, n, CAM, rec.rho, acc_max=ACC_MAX if spheres is None else 6)
    d, w = rec.planes()
    assert np.array_equal(w[:, 1], e_att) and np.array_equal(w[:, 2], e_acc) and np.array_equal(w[:, 3] == 1, e_rej)
    assert (e_att > e_acc).any()
    if spheres is None:
        # the wide ball holds what the deep rule's cap of six would cut off
        e6 = _expected_records(lambda m: (states[m]["flags"], states[m]["n_steps"].astype(np.uint32),
                                          states[m]["n_accepted"].astype(np.uint32), states[m]["out"][:, :3]), n, CAM, rec.rho, acc_max=6)
        assert (e_acc > 6).any() and e_att.sum() > e6[0].sum()
    x, v = rec.position(), np.stack([d[1, :, 1], d[2, :, 0], d[2, :, 1]], 1)
    for i in np.nonzero(e_att)[0]:
        end = states[int(e_att[i])]["out"][i]
        assert np.array_equal(x[i], end[:3], equal_nan=True) and np.array_equal(v[i], end[3:], equal_nan=True), i


def test_max_step_ends_the_wide_records_at_eight_accepted_steps(ctx):
    """h0 ~ 0.01, 10 h0, then steps of max_step: nothing is rejected, and eight accepted steps stay far inside the ball -- the cap
    is the launch argument, eight by the wide rule where the deep rule's six stands for mode 4."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=2)
    p = _params(lambda_end=50.0, max_step=0.5)
    _, rec = _three(ctx, p, CAM, k0)
    w = rec.planes()[1]
    moving = (np.arange(n) != NAN_RAY) & (np.arange(n) != n // 2)
    assert np.all(w[moving, 1] == ACC_MAX) and np.all(w[moving, 2] == ACC_MAX) and not w[moving, 3].any()
    deep = Records(n)
    _, used = _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD_DEEP, deep)
    w6 = deep.planes()[1]
    assert used == _ffi.PREFIX_RECORD_DEEP and np.all(w6[moving, 1] == 6) and np.all(w6[moving, 2] == 6)


def test_depth_of_the_wide_records_on_the_headline_window(ctx):
    """4 096 uniform rays of the headline window from the bench camera at the bench's parameters.  The rule was chosen on a CPU
    restatement (scipy RK45, 300 rays): 8.05 attempts kept per ray at 15/16 with room for eight accepted steps, none at a cap,
    against 6.04 by the deep rule's 3/4.  Stated here: a mean of at least 7.5 attempts (between the two, with room for sampling),
    at most 1 % of the records at eight accepted steps, none beyond twelve attempts."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 4096
    k0 = np.ascontiguousarray(frame_rays(n, seed=11, fov=0.6))
    p = _params(lambda_end=50.0, order_blocks=4)
    plain, rec = _three(ctx, p, CAM, k0)
    w = rec.planes()[1]
    att, acc = w[:, 1], w[:, 2]
    deep = Records(n)
    _call(ctx, p, CAM, k0, _ffi.PREFIX_RECORD_DEEP, deep)
    print("rho", rec.rho, "attempts kept per ray: wide", att.mean(), "deep", deep.planes()[1][:, 1].mean(), "of", plain["n_steps"].mean(),
          "| accepted", np.bincount(acc, minlength=ACC_MAX + 1).tolist(), "attempted", np.bincount(att, minlength=ATT_MAX + 1).tolist())
    assert rec.rho == pytest.approx(27.1875, rel=1e-5)
    assert att.mean() >= 7.5
    assert (acc == ACC_MAX).mean() <= 0.01
    assert att.max() <= ATT_MAX and acc.max() <= ACC_MAX
    assert att.mean() > deep.planes()[1][:, 1].mean() + 1.0


def test_the_step_budget_must_exceed_what_a_wide_record_may_hold(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=4)
    # max_steps = 12: nothing is written, the buffer is untouched
    p12 = _params(lambda_end=50.0, max_steps=ATT_MAX)
    plain12, _ = _call(ctx, p12, CAM, k0)
    rec = Records(n, fill=255)
    r, used = _call(ctx, p12, CAM, k0, _ffi.PREFIX_RECORD_WIDE, rec)
    assert used == _ffi.PREFIX_NONE and rec.rho == 0.0 and bool((rec.d == 255).all())
    _same(plain12, r, "refused recording call")
    # max_steps = 13: written, and the replay ends every ray where the plain call does (most of them on the budget)
    p13 = _params(lambda_end=50.0, max_steps=ATT_MAX + 1)
    plain13, rec = _three(ctx, p13, CAM, k0)
    assert (plain13["flags"] & F_MAX_STEPS).sum() > n // 5 and rec.planes()[1][:, 1].max() <= ATT_MAX
    # ... and nothing is replayed under max_steps = 12
    rep, used = _call(ctx, p12, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_NONE
    _same(plain12, rep, "refused replaying call")


# ---- refusal, then recovery: the two owners ---------------------------------------------------------------------------------
FREE, SHUT = dict(lambda_end=200.0), dict(lambda_end=200.0, r_exit=45.0)      # (an exit sphere at 45: 15 from the camera, in the ball)
# the script: (scene, what the owner asks for, what the library answers, the records' rho after the call)
R, W, NO = 2, 5, 0
SCRIPT = ([(FREE, W, W, 27.1875)] + [(SHUT, R, NO, 27.1875)] * 2 + [(SHUT, W, W, 3.75)] + [(SHUT, R, R, 3.75)] * 2 +
          [(FREE, R, R, 3.75)] * 8 + [(FREE, W, W, 27.1875)] + [(FREE, R, R, 27.1875)] * 2)


def _frame(ctx, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    fr = DeviceFrame(ctx, 48, 40, 2, fov_x=0.6, fov_y=0.5, origin=CAM, **kw)
    fr.set_sky(synthetic_sky(64, 32))
    fr.generate_rays()
    return fr


def test_device_frame_records_again_after_two_refusals_and_after_eight_roomy_traces(ctx, monkeypatch):
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    assert (_ffi.PREFIX_REPLAY, _ffi.PREFIX_RECORD_WIDE, _ffi.PREFIX_NONE) == (R, W, NO)
    monkeypatch.setenv("BHGEO_WIDE_PREFIX", "1")          # an owner that records wide from its first trace
    ref, fr = _frame(ctx, start_cache=False), _frame(ctx)
    ss = fr.start_steps
    recorded = replayed = refused = 0
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
        recorded += ask == W
        replayed += (ask, used) == (R, R)
        refused += (ask, used) == (R, NO)
        assert (ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (recorded, replayed, refused), k
        assert ss.rho == pytest.approx(rho, rel=1e-5), k
        # the start steps are recorded once: a trace that records the start-up records again replays them
        assert (ss.recorded, ss.replayed) == (1, k), k
    assert (recorded, replayed, refused) == (3, 12, 2)
    words = ss.d_rec[96 * fr.n:].view(torch.int32).view(fr.n, 4).cpu().numpy()
    assert words[:, 2].max() > 6                                 # (wide records again: more accepted steps than the deep rule keeps)
    # BHGEO_WIDE_PREFIX=0: a new owner records by the deep rule
    monkeypatch.setenv("BHGEO_WIDE_PREFIX", "0")
    old = _frame(ctx)
    for _ in range(2):
        old.trace(_params(**FREE))
        assert torch.equal(old.d_end, plain[tuple(sorted(FREE.items()))][0])
    so = old.start_steps
    assert (so.prefix_recorded, so.prefix_replayed, so.prefix_refused) == (1, 1, 0) and so.rho == pytest.approx(21.75, rel=1e-5)
    assert so.prefix.mode == _ffi.PREFIX_REPLAY and so.d_rec[96 * old.n:].view(torch.int32).view(old.n, 4)[:, 2].max().item() <= 6


def test_library_frame_records_again_after_two_refusals_and_after_eight_roomy_renders(ctx, monkeypatch):
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

    monkeypatch.setenv("BHGEO_WIDE_PREFIX", "1")          # an owner that records wide from its first render
    f = frame()
    assert f.prefix_info() == (NO, NO, 0.0)
    got, told = [], []
    for pkw, ask, used, rho in SCRIPT:
        got.append(f.render(_params(**pkw)).copy())
        told.append(f.prefix_info())
    f.close()
    for k, ((pkw, ask, used, rho), (t_mode, t_used, t_rho)) in enumerate(zip(SCRIPT, told)):
        assert (t_mode, t_used) == (ask, used), (k, told)
        assert t_rho == pytest.approx(rho, rel=1e-5), k
    monkeypatch.setenv("BHGEO_START_PREFIX", "0")
    f = frame()
    want = {}
    for pkw in (FREE, SHUT):
        want[tuple(sorted(pkw.items()))] = f.render(_params(**pkw)).copy()
        assert f.prefix_info()[:2] == (NO, NO)
    f.close()
    for k, ((pkw, _, _, _), g) in enumerate(zip(SCRIPT, got)):
        assert np.array_equal(g, want[tuple(sorted(pkw.items()))]), k
    assert not np.array_equal(want[tuple(sorted(FREE.items()))], want[tuple(sorted(SHUT.items()))])
    # BHGEO_WIDE_PREFIX=0: the deep rule
    monkeypatch.delenv("BHGEO_START_PREFIX")
    monkeypatch.setenv("BHGEO_WIDE_PREFIX", "0")
    f = frame()
    f.render(_params(**FREE))
    info = f.prefix_info()
    f.close()
    assert info[:2] == (_ffi.PREFIX_RECORD_DEEP, _ffi.PREFIX_RECORD_DEEP) and info[2] == pytest.approx(21.75, rel=1e-5)


PROMOTE_CALLS = 32


def test_owners_record_deep_first_and_are_promoted_to_wide_by_a_clean_run(ctx, monkeypatch):
    """The owners' default: the first trace records by the deep rule (21.75), 32 traces in a row replay, the 34th writes the
    records again by the wide rule (27.1875) while it replays its start steps, and the traces after it replay those -- every
    result the plain trace's.  One refused trace in the run starts it over.  DeviceFrame, then bhg_frame."""
    import torch
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    monkeypatch.delenv("BHGEO_WIDE_PREFIX", raising=False)
    D = _ffi.PREFIX_RECORD_DEEP
    p, shut = _params(**FREE), _params(**SHUT)
    ref, fr = _frame(ctx, start_cache=False), _frame(ctx)
    ref.trace(p)
    want = (ref.d_end.clone(), ref.d_flags.clone(), ref.d_steps.clone(), ref.d_acc.clone())
    ss = fr.start_steps
    asked = []
    for k in range(PROMOTE_CALLS + 4):
        fr.trace(p)
        asked.append((ss.prefix.mode, ss.prefix.used))
        for a, b in zip((fr.d_end, fr.d_flags, fr.d_steps, fr.d_acc), want):
            assert torch.equal(a, b), k
        assert ss.rho == pytest.approx(21.75 if k <= PROMOTE_CALLS else 27.1875, rel=1e-5), k
    assert asked == [(D, D)] + [(R, R)] * PROMOTE_CALLS + [(W, W)] + [(R, R)] * 2
    assert (ss.recorded, ss.replayed, ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (1, PROMOTE_CALLS + 3, 2, PROMOTE_CALLS + 2, 0)
    # a second owner: a refusal after 20 replays (the exit sphere at 45 stands inside the deep ball too) starts the run over
    fr = _frame(ctx)
    ss = fr.start_steps
    for k in range(21):
        fr.trace(p)
    fr.trace(shut)
    assert (ss.prefix.mode, ss.prefix.used) == (R, NO)
    for k in range(PROMOTE_CALLS):
        fr.trace(p)
        assert (ss.prefix.mode, ss.prefix.used) == (R, R), k
    fr.trace(p)
    assert (ss.prefix.mode, ss.prefix.used) == (W, W) and ss.prefix_recorded == 2
    # the library's frame
    Wd, Ht, S = 48, 40, 2
    f = _ffi.Frame([0], Wd, Ht, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=python_random_stream(42.0, 2 * S * Wd * Ht))
    f.set_scene(synthetic_sky(64, 32), lamps=[[10.0, 10.0, 30.0, 30.0]])
    told, imgs = [], []
    for k in range(PROMOTE_CALLS + 3):
        imgs.append(f.render(p).copy())
        told.append(f.prefix_info())
    f.close()
    assert [t[:2] for t in told] == [(D, D)] + [(R, R)] * PROMOTE_CALLS + [(W, W), (R, R)]
    assert told[0][2] == pytest.approx(21.75, rel=1e-5) and told[-1][2] == pytest.approx(27.1875, rel=1e-5)
    for k, im in enumerate(imgs):
        assert np.array_equal(im, imgs[0]), k

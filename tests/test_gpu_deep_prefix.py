"""The deep start-up records (BHG_PREFIX_RECORD_DEEP): the recording pass carries on through rejected
attempts and, in a scene without object spheres, uses three quarters of the clear ball about the camera.

What may never change is a result: every comparison of results below is array_equal -- end records, flags, n_steps, n_accepted,
object ids -- between a plain call, a deep-recording call and a replaying call on the same rays, for every kernel variant in
scope, with and without order_blocks.  What the records hold is checked twice: against the DEVICE's own attempts (the plain call
under a step budget of m = 1 .. 12 attempts says exactly which attempt each ray had accepted and where it stood after it), and
against the C oracle on the CPU, which alone shows that the rays chosen here exercise what is new: most records hold a rejected
attempt and four or more accepted steps.

One invariant needs a word: a usable record leaves the ray at least one attempt to execute (plain n_steps > attempted) -- unless
the controller gives the ray up before another attempt (BHG_FLAG_MAX_STEPS / STEP_TOO_SMALL are raised in FRONT of an attempt),
where n_steps == attempted is all there can be.  The NaN direction is such a ray under max_steps = 13.
"""
import numpy as np
import pytest

from conftest import CAM, frame_rays

pytestmark = pytest.mark.gpu

ACC_MAX, ATT_MAX, K_MAX = 6, 12, 4
NAN_RAY = 7
F_REACHED_END, F_MAX_STEPS, F_STEP_TOO_SMALL, F_HIT_DISK = 4, 16, 32, 128


def _params(**kw):
    from blackhole_geodesic_calculator_amd import _ffi
    kw.setdefault("max_steps", 20000)
    return _ffi.make_params(**kw)


def _rays(n, seed, fov=0.6):
    """Seeded rays of the headline window (the bench camera, its field of view) with a NaN direction and a zero direction among
    them, both inside the first batch; the middle of the window looks at the hole."""
    k0 = frame_rays(n, seed=seed, fov=fov)
    k0[NAN_RAY] = np.nan
    k0[n // 2] = 0.0
    k0[3] = [0.0, 0.0, -1.0]          # straight at the hole
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
        if mode in (_ffi.PREFIX_RECORD, _ffi.PREFIX_RECORD_DEEP):
            rec.rho = pf.rho
    return res, used


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def _three(ctx, p, x0, k0, spheres=None, rec_p=None, rec_spheres=None, expect_replay=True, mode=None):
    """plain / recording / replaying call; the recording call may see another scene (rec_p, rec_spheres) than the other two.
    Returns (plain result, Records)."""
    from blackhole_geodesic_calculator_amd import _ffi
    mode = _ffi.PREFIX_RECORD_DEEP if mode is None else mode
    n = len(k0)
    plain, _ = _call(ctx, p, x0, k0, spheres=spheres)
    rec = Records(n)
    if rec_p is None:
        r, used = _call(ctx, p, x0, k0, mode, rec, spheres=spheres)
        _same(plain, r, "recording call")
    else:
        _, used = _call(ctx, rec_p, x0, k0, mode, rec, spheres=rec_spheres)
    assert used == mode and rec.rho > 0.0
    before = rec.d.clone()
    rep, used = _call(ctx, p, x0, k0, _ffi.PREFIX_REPLAY, rec, spheres=spheres)
    assert used == (_ffi.PREFIX_REPLAY if expect_replay else _ffi.PREFIX_NONE)
    _same(plain, rep, "replaying call" if expect_replay else "refused call")
    assert bool((rec.d == before).all()), "a replaying call wrote into the records"
    return plain, rec


def _expected_records(trace_m, n, x0, rho):
    """The deep rule restated, lane per ray, on the outcome of plain traces under a step budget of m = 1 .. 12 attempts:
    trace_m(m) -> (flags, n_attempted, n_accepted, position) of every ray.  A ray that still runs after m attempts carries
    BHG_FLAG_MAX_STEPS with n_attempted == m and stands where attempt m left it; attempt m was accepted when n_accepted grew.
    Returns (attempted, accepted, rejected bit)."""
    att, acc = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rej, alive = np.zeros(n, bool), np.ones(n, bool)
    prev = np.zeros(n, np.uint32)
    for m in range(1, ATT_MAX + 1):
        flags, natt, nacc, pos = trace_m(m)
        going = ((flags & F_MAX_STEPS) != 0) & (natt == m)          # (else attempt m ended the ray, or an earlier one did)
        accepted = nacc > prev
        inside = np.linalg.norm(pos - np.asarray(x0), axis=1) <= rho
        keep = alive & going & (acc < ACC_MAX) & (~accepted | inside)
        att[keep], acc[keep], rej[keep] = m, nacc[keep], ~accepted[keep]
        alive, prev = keep, nacc
    return att, acc, rej


OBJ = [[1.0, 0.5, 12.0, 2.0], [-3.0, 0.0, 6.0, 1.0]]
# the kernel variants <rhs, events> in scope: (name, params, object spheres).  Exit sphere and disk plane stand farther from the
# camera than the horizon, so that the object-free variants record in the headline ball: 3/4 (30 - 1) = 21.75.
VARIANTS = [
    ("<0,0>", dict(lambda_end=50.0), None),
    ("<1,0>", dict(lambda_end=50.0, rhs_form=1), None),
    ("<0,1>", dict(lambda_end=200.0, r_exit=60.0), None),
    ("<0,3>", dict(lambda_end=200.0, r_exit=60.0, disk_r_in=3.0, disk_r_out=12.0), None),
    ("<0,5>", dict(lambda_end=200.0, r_exit=60.0), OBJ),
]
# three batches and a partial one; 64 batches, in ray order and handed out in the order of a 4-sample frame
SHAPES = [(209, 0), (4096, 0), (4096, 4)]

_oracle_cache = {}


def _oracle_side(oracle, name, pkw, spheres, n, rho):
    """(expected records, the oracle's full trace) for a variant's rays: computed once, shared, never changed."""
    key = (name, n)
    if key not in _oracle_cache:
        k0 = _rays(n, seed=n)
        okw = dict(pkw, spheres=spheres) if spheres is not None else dict(pkw)

        def trace_m(m):
            o = oracle.trace(k0, CAM, max_steps=m, **okw)
            return o["flags"], o["n_attempted"], o["n_accepted"], o["end"][:, :3]

        exp = _expected_records(trace_m, n, CAM, rho)
        full = oracle.trace(k0, CAM, max_steps=20000, **okw)
        for a in exp + (full["flags"], full["n_attempted"], full["n_accepted"]):
            a.setflags(write=False)
        _oracle_cache[key] = (exp, full)
    return _oracle_cache[key]


@pytest.mark.parametrize("n,order_blocks", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,pkw,spheres", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_deep_record_and_replay_equal_the_plain_call(ctx, oracle, name, pkw, spheres, n, order_blocks):
    from blackhole_geodesic_calculator_amd import _ffi
    k0 = _rays(n, seed=n)
    p = _params(order_blocks=order_blocks, **pkw)
    plain, rec = _three(ctx, p, CAM, k0, spheres=spheres)
    clear = _ffi.prefix_clearance(p, CAM, spheres)
    rho = (0.25 if spheres else 0.75) * min(clear, float(np.linalg.norm(CAM)))
    assert rec.rho == pytest.approx(rho, rel=1e-12)
    if not spheres:
        assert rec.rho == pytest.approx(21.75, rel=1e-5)
    d, w = rec.planes()
    att, acc, bits = w[:, 1], w[:, 2], w[:, 3]
    ok = att > 0
    with_rej, four = ((att > acc) & ok).sum() / ok.sum(), ((acc >= 4) & ok).sum() / ok.sum()
    print(name, n, order_blocks, "rho", rec.rho, "attempts kept per ray", att.mean(), "of", plain["n_steps"][np.arange(n) != NAN_RAY].mean(),
          "| share of usable records with a rejected attempt", with_rej, "with >= 4 accepted steps", four,
          "| attempted", np.bincount(att, minlength=ATT_MAX + 1).tolist(), "accepted", np.bincount(acc, minlength=ACC_MAX + 1).tolist())
    # the record invariants
    assert np.array_equal(w[:, 0], np.arange(n))
    assert np.all(acc <= att) and att.max() <= ATT_MAX and acc.max() <= ACC_MAX and np.all(bits <= 1)
    assert ok.sum() >= n - 1
    assert np.all(np.linalg.norm(rec.position()[ok] - CAM, axis=1) <= rec.rho)
    gave_up = (plain["flags"] & (F_MAX_STEPS | F_STEP_TOO_SMALL)) != 0
    assert np.all(plain["n_steps"][ok & ~gave_up] > att[ok & ~gave_up]) and np.all(plain["n_steps"][ok] >= att[ok])
    assert np.all(plain["n_accepted"][ok] >= acc[ok])
    finite = ok & (np.arange(n) != NAN_RAY)
    assert np.all(d[5, finite, 1] < p.lambda_end) and np.all(d[4, finite, 1] > 0.0)
    assert not bits[acc == att].any()                     # (a record without a rejected attempt cannot end on one)

    # the C oracle on the CPU: the same rule on its attempts.  The device's reciprocals, roots and the 1/5 power differ from
    # libm's in the last bits, so an error norm within an ulp of 1 may be accepted by one and rejected by the other: the records
    # are compared on the rays whose WHOLE plain trace took the same attempts on both (the parity tests' own notion), and those
    # must be nearly all.
    (e_att, e_acc, e_rej), full = _oracle_side(oracle, name, pkw, spheres, n, rec.rho)
    agree = (plain["n_steps"] == full["n_attempted"]) & (plain["n_accepted"] == full["n_accepted"]) & (plain["flags"] == full["flags"])
    print("   rays whose plain trace takes the oracle's attempts:", agree.mean())
    assert agree.mean() >= 0.95
    assert np.array_equal(att[agree], e_att[agree]) and np.array_equal(acc[agree], e_acc[agree])
    assert np.array_equal(bits[agree] == 1, e_rej[agree])
    # ... and it is the oracle ALONE that shows these rays exercise the new rule
    e_ok = e_att > 0
    o_rej, o_four = ((e_att > e_acc) & e_ok).sum() / e_ok.sum(), ((e_acc >= 4) & e_ok).sum() / e_ok.sum()
    print("   oracle: share with a rejected attempt", o_rej, "with >= 4 accepted steps", o_four)
    if not spheres:
        assert o_rej >= 0.25 and o_four >= 0.5
        assert with_rej >= 0.25 and four >= 0.5
    else:
        # (next to object spheres the ball stays the quarter, rho = 4.0 here: the fourth accepted step leaves it, and what is
        # new are the few rejections in front of that step)
        moving = np.arange(n) != n // 2              # (the zero direction goes nowhere: six accepted steps on the spot)
        assert rec.rho == pytest.approx(0.25 * clear, rel=1e-12) and acc[moving].max() <= 4


@pytest.mark.parametrize("name,pkw,spheres", [VARIANTS[0], VARIANTS[3], VARIANTS[4]], ids=["<0,0>", "<0,3>", "<0,5>"])
def test_the_records_restate_the_devices_own_attempts_exactly(ctx, name, pkw, spheres):
    """No tolerance: the plain DEVICE call under a step budget of m attempts tells which attempt was accepted and where the ray
    stood after it, and the records -- counts, rejected bit, kept state -- must be that, ray for ray."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=n)
    rec = Records(n)
    _, used = _call(ctx, _params(**pkw), CAM, k0, _ffi.PREFIX_RECORD_DEEP, rec, spheres=spheres)
    assert used == _ffi.PREFIX_RECORD_DEEP
    states = {}

    def trace_m(m):
        r, _ = _call(ctx, _params(**dict(pkw, max_steps=m)), CAM, k0, spheres=spheres)
        states[m] = r
        return r["flags"], r["n_steps"].astype(np.uint32), r["n_accepted"].astype(np.uint32), r["out"][:, :3]

    e_att, e_acc, e_rej = _expected_records(trace_m, n, CAM, rec.rho)
    d, w = rec.planes()
    assert np.array_equal(w[:, 1], e_att) and np.array_equal(w[:, 2], e_acc) and np.array_equal(w[:, 3] == 1, e_rej)
    assert (e_att > e_acc).any()
    # the kept position and direction are the state the budget-limited trace stopped in
    x, v = rec.position(), np.stack([d[1, :, 1], d[2, :, 0], d[2, :, 1]], 1)
    for i in np.nonzero(e_att)[0]:
        end = states[int(e_att[i])]["out"][i]
        assert np.array_equal(x[i], end[:3], equal_nan=True) and np.array_equal(v[i], end[3:], equal_nan=True), i


def test_max_step_ends_the_records_at_the_accepted_cap(ctx):
    n = 209
    p = _params(lambda_end=50.0, max_step=0.5)
    _, rec = _three(ctx, p, CAM, _rays(n, seed=2))
    d, w = rec.planes()
    moving = (np.arange(n) != NAN_RAY) & (np.arange(n) != n // 2)
    # h0 ~ 0.01, 10 h0, then steps of max_step: nothing is rejected, and six accepted steps stay far inside the ball
    assert np.all(w[moving, 1] == ACC_MAX) and np.all(w[moving, 2] == ACC_MAX) and not w[moving, 3].any()
    assert np.all(d[5, moving, 1] > 4 * 0.5) and np.all(d[5, moving, 1] <= 6 * 0.5 + 1e-12)


def test_rays_that_end_inside_the_ball_keep_no_last_step(ctx):
    n = 209
    p = _params(lambda_end=0.05)
    plain, rec = _three(ctx, p, CAM, _rays(n, seed=3))
    d, w = rec.planes()
    att = w[:, 1]
    print("attempted", np.bincount(att, minlength=ATT_MAX + 1).tolist())
    ok = (att > 0) & (np.arange(n) != NAN_RAY)
    reached = (plain["flags"] & F_REACHED_END) != 0
    assert reached.sum() >= n - 2
    # the attempt that reaches lambda_end is never kept: every record stands in front of lambda_end with an attempt to go
    assert np.all(d[5, ok, 1] < p.lambda_end) and np.all(plain["n_steps"][ok] > att[ok]) and np.all(plain["n_accepted"][ok] > w[ok, 2])
    moving = ok & (np.arange(n) != n // 2)
    assert att[moving].max() <= 2 and (att == 0).sum() > 1


def test_the_step_budget_must_exceed_what_a_record_may_hold(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=4)
    # max_steps = 12: refused, buffer untouched
    p12 = _params(lambda_end=50.0, max_steps=ATT_MAX)
    plain12, _ = _call(ctx, p12, CAM, k0)
    rec = Records(n, fill=255)
    r, used = _call(ctx, p12, CAM, k0, _ffi.PREFIX_RECORD_DEEP, rec)
    assert used == _ffi.PREFIX_NONE and rec.rho == 0.0 and bool((rec.d == 255).all())
    _same(plain12, r, "refused recording call")
    # max_steps = 13: accepted, and the replay ends every ray where the plain call does (most of them on the budget)
    p13 = _params(lambda_end=50.0, max_steps=ATT_MAX + 1)
    plain13, rec = _three(ctx, p13, CAM, k0)
    assert (plain13["flags"] & F_MAX_STEPS).sum() > n // 5 and rec.planes()[1][:, 1].max() <= ATT_MAX
    # ... and deep records are not replayed under a budget they could exhaust (the call cannot tell which rule wrote them)
    rep, used = _call(ctx, p12, CAM, k0, _ffi.PREFIX_REPLAY, rec)
    assert used == _ffi.PREFIX_NONE
    _same(plain12, rep, "refused replaying call")


def test_a_scene_that_enters_the_deep_ball_refuses_replay_although_it_clears_the_quarter_ball(ctx):
    """Records of an object-free, exit-free scene (rho 21.75 at the bench camera; 3/4 (|x0| - 1) at the camera above the disk)
    against an exit sphere, a disk plane and an object sphere that each stand between the two balls."""
    from blackhole_geodesic_calculator_amd import _ffi
    n = 209
    k0 = _rays(n, seed=7)
    base = dict(lambda_end=200.0)
    above = np.array([20.0, 0.0, 10.0])
    cases = [("exit sphere", CAM, dict(r_exit=40.0), None, 10.0),
             ("disk plane", above, dict(r_exit=60.0, disk_r_in=3.0, disk_r_out=25.0), None, 10.0),
             ("object sphere", CAM, dict(), [[CAM[0], 0.0, CAM[2] - 12.0, 2.0]], 10.0)]
    for what, x0, extra, sph, clearance in cases:
        p, rec_p = _params(**base, **extra), _params(**base)
        assert _ffi.prefix_clearance(p, x0, sph) == pytest.approx(clearance, rel=1e-9)
        plain, rec = _three(ctx, p, x0, k0, spheres=sph, rec_p=rec_p, expect_replay=False)
        quarter = 0.25 * (np.linalg.norm(x0) - 1.0)
        assert rec.rho == pytest.approx(3.0 * quarter, rel=1e-9) and quarter < clearance < rec.rho, what
        # ... while records of the rule of always, in their quarter ball, replay in that scene
        _, rec1 = _three(ctx, p, x0, k0, spheres=sph, rec_p=rec_p, expect_replay=True, mode=_ffi.PREFIX_RECORD)
        assert rec1.rho == pytest.approx(quarter, rel=1e-9)


def test_tangent_surfaces_refuse_and_surfaces_just_outside_do_not(ctx):
    n = 209
    k0 = _rays(n, seed=8)
    base = dict(lambda_end=200.0)
    rho = 0.75 * (np.linalg.norm(CAM) - 1.0)
    r0 = float(np.linalg.norm(CAM))
    for gap, replay in [(10.0, False), (rho, False), (rho * 1.001, True)]:       # inside, tangent, just outside
        sph = [[CAM[0], 0.0, CAM[2] - (2.0 + gap), 2.0]]
        _, rec = _three(ctx, _params(**base), CAM, k0, spheres=sph, rec_p=_params(**base), expect_replay=replay)
        assert rec.rho == pytest.approx(rho, rel=1e-9)
        _three(ctx, _params(r_exit=r0 + gap, **base), CAM, k0, rec_p=_params(**base), expect_replay=replay)


def test_records_of_the_rule_of_always_replay_through_the_same_fill(ctx):
    from blackhole_geodesic_calculator_amd import _ffi
    n = 4096
    k0 = _rays(n, seed=n)
    p = _params(lambda_end=50.0, order_blocks=4)
    plain, rec = _three(ctx, p, CAM, k0, mode=_ffi.PREFIX_RECORD)
    assert rec.rho == pytest.approx(7.25, rel=1e-5)
    d, w = rec.planes()
    depth = w[:, 1]
    assert np.array_equal(w[:, 0], np.arange(n)) and np.array_equal(w[:, 2], depth) and not w[:, 3].any() and depth.max() <= K_MAX
    assert depth[NAN_RAY] == 0 and (depth == 0).sum() == 1
    ok = depth > 0
    assert np.all(np.linalg.norm(rec.position()[ok] - CAM, axis=1) <= rec.rho) and np.all(plain["n_steps"][ok] > depth[ok])
    # ... and the deep records of the same rays hold them whole: the same leading accepted steps, then more
    _, deep = _three(ctx, p, CAM, k0)
    assert np.all(deep.planes()[1][:, 2] >= depth) and deep.planes()[1][:, 1].sum() > 1.5 * depth.sum()


# ---- DeviceFrame ------------------------------------------------------------------------------------------------------------
def _frame(ctx, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    fr = DeviceFrame(ctx, 48, 40, 2, fov_x=0.6, fov_y=0.5, origin=CAM, **kw)
    fr.set_sky(synthetic_sky(64, 32))
    fr.generate_rays()
    return fr


def test_device_frame_records_by_the_deep_rule(ctx, monkeypatch):
    import torch
    p = _params(lambda_end=50.0)
    ref = _frame(ctx, start_cache=False)
    ref.trace(p)
    want = ref.shade().cpu().numpy()
    fr = _frame(ctx)
    for _ in range(3):
        fr.trace(p)
        assert np.array_equal(fr.shade().cpu().numpy(), want)
        assert torch.equal(fr.d_steps, ref.d_steps)
    ss = fr.start_steps
    assert (ss.prefix_recorded, ss.prefix_replayed, ss.prefix_refused) == (1, 2, 0) and ss.rho == pytest.approx(21.75, rel=1e-5)
    words = ss.d_rec[96 * fr.n:].view(torch.int32).view(fr.n, 4).cpu().numpy()
    assert (words[:, 1] > words[:, 2]).mean() > 0.25 and words[:, 3].any()
    # an object sphere between the two balls: refused, and replayed again once it has gone behind the hole
    for sph, refused, replayed in [([[0.0, 0.0, 18.0, 2.0]], 1, 2), ([[0.0, 0.0, -20.0, 2.0]], 1, 3)]:
        for f in (fr, ref):
            f.set_objects(sph, [[1.0, 0.5, 0.2]])
            f.trace(p)
        assert torch.equal(fr.d_end, ref.d_end) and torch.equal(fr.d_flags, ref.d_flags) and torch.equal(fr.d_obj, ref.d_obj)
        assert (ss.prefix_refused, ss.prefix_replayed, ss.prefix_recorded) == (refused, replayed, 1)
    # the orbit scene of the frame test of the rule of always, its sphere there when the records are written: the quarter
    orbit = _frame(ctx)
    orbit.set_objects([[0.0, 0.0, 8.0, 2.0]], [[1.0, 0.5, 0.2]])
    po = _params(lambda_end=200.0, r_exit=40.0)
    orbit.trace(po)
    orbit.trace(po)
    so = orbit.start_steps
    assert (so.prefix_recorded, so.prefix_replayed, so.prefix_refused) == (1, 1, 0) and so.rho == pytest.approx(2.5, rel=1e-5)
    # the switch back to the rule of always
    monkeypatch.setenv("BHGEO_DEEP_PREFIX", "0")
    old = _frame(ctx)
    for _ in range(2):
        old.trace(p)
        assert np.array_equal(old.shade().cpu().numpy(), want)
    so = old.start_steps
    assert (so.prefix_recorded, so.prefix_replayed, so.prefix_refused) == (1, 1, 0) and so.rho == pytest.approx(7.25, rel=1e-5)
    words = so.d_rec[96 * old.n:].view(torch.int32).view(old.n, 4).cpu().numpy()
    assert np.array_equal(words[:, 1], words[:, 2]) and not words[:, 3].any()


# ---- the library's own frame ------------------------------------------------------------------------------------------------
def test_library_frame_renders_the_same_by_either_rule_and_without_records(ctx, monkeypatch):
    """bhg_frame_render, deep records (the default) against BHGEO_DEEP_PREFIX=0 and BHGEO_START_PREFIX=0: an object-free scene
    (recorded, replayed), a sphere between the two balls (refused by the deep records alone), behind the hole (replayed)."""
    from blackhole_geodesic_calculator_amd import _ffi
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import python_random_stream
    W, H, S = 48, 40, 2
    jitter = python_random_stream(42.0, 2 * S * W * H)
    sky = synthetic_sky(64, 32)
    p = _params(lambda_end=50.0)
    scenes = [None, None, [[0.0, 0.0, 18.0, 2.0]], [[0.0, 0.0, -20.0, 2.0]], None]

    def renders():
        f = _ffi.Frame([0], W, H, S, fov_x=0.6, fov_y=0.6, origin=CAM, jitter=jitter)
        out = []
        for sph in scenes:
            f.set_scene(sky, spheres=sph, sphere_rgb=None if sph is None else [[1.0, 0.5, 0.2]], lamps=[[10.0, 10.0, 30.0, 30.0]])
            out.append(f.render(p).copy())
        f.close()
        return out

    got = renders()
    monkeypatch.setenv("BHGEO_DEEP_PREFIX", "0")
    old = renders()
    monkeypatch.setenv("BHGEO_START_PREFIX", "0")
    want = renders()
    for g, o, w in zip(got, old, want):
        assert np.array_equal(g, w) and np.array_equal(o, w)
    assert np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2]) and np.array_equal(want[0], want[4])

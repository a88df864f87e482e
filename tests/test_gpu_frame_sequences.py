"""Both owners of frame state held to a fresh frame over random edit sequences (tests/frame_sequence_model.py).

DeviceFrame (device_frame.py) and bhg_frame (csrc/bhgeo_frame.hip) keep things from one frame to the next -- the rays, their initial
steps and start-up records, a mesh and its tree, instance sets, the tile dealing, what the last trace wrote -- and each promises the
image of a frame made for the current state alone, bit for bit.  So after every edit of a sequence the edited owner is rendered and
compared with an owner that has no history: array_equal on the float32 image of a bhg_frame; on every array the last trace wrote
and on the images of a DeviceFrame; and the two owners with each other wherever both accept the state.  There is no tolerance.

The cases with BHGEO_START_CACHE=0 run first: there no start-up state is kept, so a failure is a fault of the model or of
something else the owner keeps, and the message says so.  The last tests assert, per owner over its sequences, that the caches were in fact
used (replays, every recording rule, a refusal, a refit, an in-place rebuild, a re-deal by measured cost): run the whole module.
tests/test_frame_sequences_host.py holds the same sequences to the owner branches on the CPU.

Measured on this module as committed (MI355X): 77 cases, 16 to 17 s for the whole module, 16.7 s of it in the cases.  Every
sequence runs twice, first with BHGEO_START_CACHE=0; those 37 cases, which also make the fresh owners of their states, take
0.01 to 0.88 s (the DeviceFrame ones 0.5 to 0.9 s, the bhg_frame ones under 0.5 s), the 37 cached cases after them 0.01 to 0.6 s, the
scripted quiet runs of 140 renders included; the median case takes 0.13 s.  The fresh results are kept by State.key() and shared
by every case; a fresh bhg_frame always renders with BHGEO_START_CACHE=0, so no reference depends on which case asks first.
Over its sequences the DeviceFrame recorded its steps 110 times and replayed them 845 times, wrote start-up records 114 times,
replayed them 808 times and was refused 19 times, refitted a mesh up to 7 times in a row, rebuilt one in place 3 times, was
compared with the fresh bhg_frame 392 times; shade() without trace() raised 30 times and gave the fresh image 19 times.  Each
bhg_frame saw all four recording rules written (BHG_PREFIX_RECORD under BHGEO_DEEP_PREFIX=0), a replay, a refusal, a call with
nothing held, 11 re-deals, refit generation 11 and an in-place rebuild on every shard.

What the sequences found (each has its scripted test next to the feature's own):
  * DeviceFrame.origin was a plain attribute: shade() after a new origin shaded the old trace's records with the new position
    (tests/test_gpu_start_steps.py::test_device_frame_camera_assigned_after_a_trace_drops_what_the_trace_wrote);
  * set_polarisation() kept the up of the rotation it was called under: Q / U of every disk pixel wrong after a rotation
    (tests/test_gpu_polarisation.py::test_a_rotation_assigned_after_set_polarisation_turns_the_up_of_the_stokes_images);
  * set_observer() asked for new rays but left the last trace standing: shade() gave the old rays the new observer's g
    (tests/test_gpu_observer.py::test_set_observer_after_a_trace_drops_what_the_trace_wrote).  The random re-shade edits never
    followed set_observer; the scripted walk "reshades" now tries shade() after every setter on, changed and off, after every
    camera assignment and every mesh call, and the host test holds it to that list.
Not a fault, but a difference the model has to follow: bhg_frame_set_object_textures copies an image only for a slot that has a
sphere when it is called; DeviceFrame keeps every image it is given.  State.textures therefore carries the sphere count of then.

Mutation checks, each made on a scratch copy (nothing of them is committed), the whole module as committed (77 cases) run against
it; all of them
change which kept values are used again, none a size, an index or an address.  Every one is caught; the failing cases:
  drop atol from what DeviceFrame compares before it replays (in Python)     DeviceFrame-seed24 (step 36, atol), -seed36 (step 4, atol)
  DeviceFrame.refit_mesh does not set the held instances again               DeviceFrame-seed14, -seed36, -reshades, with and without the cache
  spin left out of bhg_frame's obs_key                                       Frame[0]- and Frame[0,0]-seed33 (step 24, spin under the
                                                                             observer camera), with and without the cache
  fov_y ignored in bhg_frame_set_camera's dirs_change                        Frame[0]- and Frame[0,0]-seed5, -seed25, -wide5, -rim5, with and
                                                                             without the cache
  prefix_clearance ignores the disk plane                                    DeviceFrame-seed19, -seed36, -ladder100, -wide14, -rim14;
                                                                             Frame[0]- and Frame[0,0]-seed25
(The rays of an owner are not start-up state: the two bhg_frame mutations also fail with BHGEO_START_CACHE=0, as they should.)
tests/test_frame_sequences_host.py keeps the steps these rest on in the committed seeds.
"""
import time

import numpy as np
import pytest

import frame_sequence_model as M

pytestmark = pytest.mark.gpu

_FRESH = {}      # (owner, state key) -> what the fresh owner of that state gave
_COVER = {}      # owner id -> what its sequences reached on the device
_RAN = set()
WALL = {}


def _same(got, want, what):
    assert got.keys() == want.keys(), f"{what}: {sorted(got)} != {sorted(want)}"
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), \
            f"{what}: {k} differs from the fresh owner's in {int((got[k] != want[k]).sum())} of {want[k].size} entries"


# ---- DeviceFrame -----------------------------------------------------------------------------------------------------------------
def _device_arrays(fr, s):
    """Every array the last trace wrote for the state's path, and the images.  Entries a trace leaves undefined are blanked: the
    crossing records past a ray's count, the barycentrics and instance of a ray that met no triangle."""
    import torch
    out = {"rgba": fr.d_rgba.clone()}      # (what render()'s shade() gave, before the other shades write the buffer again)
    out["rgba_f32"] = fr.shade_f32(torch.empty((fr.P, 4), dtype=torch.float32, device=fr.dev))
    if s.pol is not None:
        rgba, qu = fr.shade_stokes()
        out["stokes_rgba"], out["stokes_qu"] = rgba.clone(), qu
    out.update(flags=fr.d_flags, steps=fr.d_steps, acc=fr.d_acc)
    out["dir" if fr._traced == "dir" else "end"] = fr.d_dir if fr._traced == "dir" else fr.d_end
    if s.spheres:
        out["obj"] = fr.d_obj
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if s.mesh is not None:
        tri = fr.d_tri_id.cpu().numpy()
        out["tri_id"] = tri
        out["bary"] = np.where((tri >= 0)[:, None], fr.d_bary.cpu().numpy(), 0.0)
        if s.mesh.instances is not None:
            out["inst_id"] = np.where(tri >= 0, fr.d_inst_id.cpu().numpy(), -1)
    if s.layers is not None:
        n = fr.d_n_cross.cpu().numpy()
        live = np.arange(s.layers[0])[:, None] < n[None, :]
        out["n_cross"] = n
        out["cross"] = np.where(live[:, :, None], fr.d_cross.cpu().numpy(), 0.0)
        if s.layers[2] != 0.0:
            out["t_cross"] = np.where(live, fr.d_t_cross.cpu().numpy(), 0.0)
            out["t_end"] = fr.d_t_end.cpu().numpy()
    return out


def _fresh_device(ctx, s):
    k = ("device", s.key())
    if k not in _FRESH:
        fr = M.fresh_device_frame(ctx, s)
        fr.render(s.make_params())
        assert fr.start_steps.recorded == 0 and fr.start_steps.d_h is None
        _FRESH[k] = _device_arrays(fr, s)
        if fr.mesh is not None:
            fr.mesh.close()
    return _FRESH[k]


def _fresh_library(devices, s):
    """(always by the plain path -- the library reads the switch at every render -- whichever case asks first)"""
    k = (tuple(devices), s.key())
    if k not in _FRESH:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("BHGEO_START_CACHE", "0")
            fr = M.fresh_library_frame(devices, s)
            _FRESH[k] = {"image": fr.render(s.make_params()).copy()}
            assert fr.prefix_info()[:2] == (0, 0) or s.mesh is not None
            fr.close()
    return _FRESH[k]


def _run_device(ctx, seq, cover, where):
    from blackhole_geodesic_calculator_amd import _ffi
    fr = None
    for i, e in enumerate(seq):
        s, regen = e.after, False
        at = f"{where} step {i} {e!r}"
        if e.kind == "start":
            fr = M.fresh_device_frame(ctx, s, start_cache=True)
        elif e.refused:
            M.apply_device_frame(fr, e.ops, e.refused[0])
            with pytest.raises(ValueError):
                fr.render(e.refused[0].make_params())
            M.apply_device_frame(fr, e.undo, s)
        else:
            builds = fr.mesh.build_info() if e.kind == "mesh:rebuild" else None
            regen = M.apply_device_frame(fr, e.ops, s)
            if builds is not None:
                now = fr.mesh.build_info()
                assert (now["builds"], now["allocations"]) == (builds["builds"] + 1, builds["allocations"]), f"{at}: {builds} -> {now}"
                cover["rebuilt_in_place"] += 1
        want = _fresh_device(ctx, s)
        if e.reshade:
            # shade() without trace() after an edit: it raises, or it is the fresh frame's image -- never anything else
            import torch
            try:
                img = fr.shade()
                torch.cuda.synchronize()
                img = img.cpu().numpy()
            except (RuntimeError, ValueError):
                cover["reshade_raised"] += 1
            else:
                assert np.array_equal(img, want["rgba"], equal_nan=True), f"{at}: shade() without trace() gave an image that is not the fresh frame's"
                cover["reshade_equal"] += 1
        p = s.make_params()
        for k in range(1 + e.dwell):
            fr.render(p, regenerate_rays=regen and k == 0)
            got = _device_arrays(fr, s)
            _same(got, want, f"{at} render {k}")
            if fr.mesh is not None:
                cover["refit_generation"] = max(cover["refit_generation"], fr.mesh.refit_info()[0])
        if M.legal(s, "library"):
            lib = _fresh_library([0], s)["image"].reshape(-1, 4)
            assert np.array_equal(got["rgba_f32"], lib, equal_nan=True), f"{at}: DeviceFrame.shade_f32 differs from the fresh bhg_frame's image"
            cover["across_owners"] += 1
    ss = fr.start_steps
    for name in ("recorded", "replayed", "prefix_recorded", "prefix_replayed", "prefix_refused"):
        cover[name] += getattr(ss, name)
    if fr.mesh is not None:
        fr.mesh.close()
    assert _ffi.has_rim_prefix()


def _run_library(devices, seq, cover, where):
    from blackhole_geodesic_calculator_amd import _ffi
    fr = None
    try:
        for i, e in enumerate(seq):
            s = e.after
            at = f"{where} step {i} {e!r}"
            builds = None
            if e.kind == "start":
                fr = M.fresh_library_frame(devices, s)
            elif e.refused:
                bad = e.refused[0]
                M.apply_library_frame(fr, e.ops, bad)
                with pytest.raises(_ffi.BhgError) as err:
                    fr.render(bad.make_params())
                assert err.value.code == _ffi.E_INVALID, at
                M.apply_library_frame(fr, e.undo, s)
            else:
                if e.kind == "mesh:rebuild":
                    builds = [fr.mesh_build_info(r) for r in range(len(devices))]
                M.apply_library_frame(fr, e.ops, s)
            want = _fresh_library(devices, s)["image"]
            p = s.make_params()
            for k in range(1 + e.dwell):
                img = fr.render(p)
                assert np.array_equal(img, want, equal_nan=True), \
                    f"{at} render {k}: the image differs from the fresh frame's in {int((img != want).any(axis=2).sum())} of {W_H} pixels"
                if s.mesh is None:
                    for r in range(len(devices)):
                        cover["prefix"].add(fr.prefix_info(r)[:2])
                else:
                    cover["refit_generation"] = max(cover["refit_generation"], fr.mesh_refit_info()[0])
            if builds is not None:
                nv, nt = (len(a) for a in M.mesh_arrays(s.mesh)[:2])
                for r, before in enumerate(builds):
                    now = fr.mesh_build_info(r)
                    assert now["builds"] > before["builds"], f"{at}: {before} -> {now}"
                    if before["built_on_device"] and nv <= before["cap_vertices"] and nt <= before["cap_triangles"]:
                        assert now["allocations"] == before["allocations"], f"{at}: an in-place rebuild allocated: {before} -> {now}"
                        cover["rebuilt_in_place"] += 1
            if e.kind == "rebalance":
                assert fr.info()["dealt_by_measured_cost"], at
                cover["rebalanced"] += 1
    finally:
        if fr is not None:
            fr.close()


W_H = M.W * M.H
OWNER_IDS = {"DeviceFrame": ("device", None), "Frame[0]": ("library", [0]), "Frame[0,0]": ("library", [0, 0])}


def _cases():
    out = []
    for oid, (owner, devices) in OWNER_IDS.items():
        for name in M.committed(owner):
            out.append(pytest.param(oid, name, True, id=f"{oid}-{name}-nocache"))
    for oid, (owner, devices) in OWNER_IDS.items():
        for name in M.committed(owner):
            out.append(pytest.param(oid, name, False, id=f"{oid}-{name}"))
    return out


@pytest.fixture(scope="module")
def committed():
    return {owner: M.committed(owner) for owner in M.OWNERS}


@pytest.mark.parametrize("oid,name,nocache", _cases())
def test_every_render_of_a_sequence_equals_the_fresh_owners(ctx, committed, monkeypatch, oid, name, nocache):
    import collections
    from blackhole_geodesic_calculator_amd import _ffi
    owner, devices = OWNER_IDS[oid]
    seq, env = committed[owner][name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if nocache:
        monkeypatch.setenv("BHGEO_START_CACHE", "0")
    cover = collections.defaultdict(int) if nocache else _COVER.setdefault(oid, collections.defaultdict(int))
    cover.setdefault("prefix", set())
    cover.setdefault("refit_generation", 0)
    where = f"{oid} {name}" + (" with BHGEO_START_CACHE=0 (no steps or start-up records are kept here: a fault of the model or of "
                               "something else the owner keeps, not of the start-up cache)" if nocache else "")
    t0 = time.perf_counter()
    try:
        if owner == "device":
            _run_device(ctx, seq, cover, where)
        else:
            _run_library(devices, seq, cover, where)
    except AssertionError:
        print(f"{oid} {name}: the sequence\n" + "\n".join(f"{i:3d} {e!r}" for i, e in enumerate(seq)))
        raise
    except _ffi.BhgError as err:
        if err.code == _ffi.E_HIP:      # a device error: nothing more is started on that device in this session
            pytest.exit(f"{where}: {err}", returncode=3)
        raise
    WALL[f"{oid}-{name}" + ("-nocache" if nocache else "")] = time.perf_counter() - t0
    if nocache and owner == "device":
        assert cover["recorded"] == cover["replayed"] == cover["prefix_recorded"] == 0
    if not nocache:
        _RAN.add((oid, name))


@pytest.mark.parametrize("oid", list(OWNER_IDS))
def test_the_sequences_used_what_the_owners_keep(committed, oid):
    """Without this the module could pass on the plain path throughout."""
    from blackhole_geodesic_calculator_amd import _ffi
    owner, devices = OWNER_IDS[oid]
    assert {(oid, name) for name in committed[owner]} <= _RAN, "run the whole module: the coverage is counted over every sequence"
    c = _COVER[oid]
    print(f"{oid}: " + ", ".join(f"{k} {v}" for k, v in sorted(c.items())))
    print("wall time per case: " + ", ".join(f"{k} {v:.1f}s" for k, v in WALL.items() if k.startswith(oid)))
    assert c["refit_generation"] > 0 and c["rebuilt_in_place"] > 0
    if owner == "device":
        assert min(c["replayed"], c["prefix_recorded"], c["prefix_replayed"], c["prefix_refused"]) > 0, dict(c)
        n_reshade = sum(e.reshade for seq, _ in committed[owner].values() for e in seq)
        assert c["reshade_raised"] > 0 and c["reshade_equal"] > 0 and c["reshade_raised"] + c["reshade_equal"] == n_reshade
        assert c["across_owners"] > 100
        return
    R = _ffi.PREFIX_REPLAY
    assert (R, R) in c["prefix"] and (R, _ffi.PREFIX_NONE) in c["prefix"], c["prefix"]
    for rule in (_ffi.PREFIX_RECORD, _ffi.PREFIX_RECORD_DEEP, _ffi.PREFIX_RECORD_WIDE, _ffi.PREFIX_RECORD_RIM):
        assert (rule, rule) in c["prefix"], (rule, c["prefix"])
    assert c["rebalanced"] > 0

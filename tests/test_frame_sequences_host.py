"""The random edit sequences of tests/frame_sequence_model.py without a GPU: the generator is a pure function of its seed, every
state it reaches is one its owner renders, every field of bhg_params has an edit, and -- played through the library's own host
functions (bhg_start_steps_match, bhg_prefix_clearance, bhg_prefix_owner_next) -- the committed seeds take every branch of the
owners' start-up decisions at least twice.  These are conditions on the seed set, not measurements: a change to the generator that
loses one fails here, before tests/test_gpu_frame_sequences.py could pass on the plain path alone."""
import dataclasses

import pytest

import frame_sequence_model as M
from blackhole_geodesic_calculator_amd import _ffi


def _listing(seq):
    return "\n".join(f"{i:3d} {e!r}" for i, e in enumerate(seq))


@pytest.fixture(scope="module")
def committed():
    return {owner: M.committed(owner) for owner in M.OWNERS}


@pytest.mark.parametrize("owner", M.OWNERS)
def test_the_generator_is_a_pure_function_of_its_seed(owner, committed):
    again = M.committed(owner)
    assert again.keys() == committed[owner].keys()
    for name, (seq, env) in committed[owner].items():
        assert seq == again[name][0] and env == again[name][1], f"{owner} {name} differs between two runs:\n{_listing(seq)}\n--\n{_listing(again[name][0])}"
        assert [e.after.key() for e in seq] == [e.after.key() for e in again[name][0]]
    a, b = M.sequence(3, owner, 20), M.sequence(4, owner, 20)
    assert [e.kind for e in a] != [e.kind for e in b]


@pytest.mark.parametrize("owner", M.OWNERS)
def test_every_state_is_legal_and_every_refused_render_breaks_one_rule(owner, committed):
    refused = set()
    for name, (seq, _) in committed[owner].items():
        for i, e in enumerate(seq):
            assert M.illegal(e.after, owner) == [], f"{owner} {name} step {i}: {M.illegal(e.after, owner)}\n{_listing(seq[:i + 1])}"
            if e.refused:
                assert M.illegal(e.refused[0], owner) == [e.refused[1]], f"{owner} {name} step {i}\n{_listing(seq[:i + 1])}"
                refused.add(e.refused[1])
    want = {"disk:params!=scene", "mesh+spheres"} if owner == "library" else {"mesh+redshift"}
    assert refused == want


def test_the_rules_of_legal():
    s = M.base_state()
    mesh = dataclasses.replace(s, mesh=M.MeshState())
    assert M.legal(s, "device") and M.legal(s, "library") and M.legal(mesh, "device") and M.legal(mesh, "library")
    sphere = dict(spheres=((0.0, 0.0, 8.0, 1.0),), sphere_rgb=((1.0, 1.0, 1.0),))
    for kw in (sphere, dict(redshift=(("sky",), 4.0)), dict(thermal=(6000.0, 1.0)), dict(motion=1), dict(textures=(1, 1))):
        bad = dataclasses.replace(mesh.with_disk(M.DISK0), **kw)
        assert len(M.illegal(bad, "library")) == 1 and len(M.illegal(bad, "device")) == 1, kw
    assert M.illegal(s.with_params(disk_r_in=3.0, disk_r_out=9.0), "library") == ["disk:params!=scene"]
    layers = dataclasses.replace(s, layers=(2, 1.0, 0.0))
    assert M.illegal(layers, "device") == ["layers:no-disk"] and M.legal(layers.with_disk(M.DISK0), "device")
    assert M.illegal(dataclasses.replace(layers.with_disk(M.DISK0), **sphere), "device") == ["layers+objects"]
    assert "library:device-only" in M.illegal(layers.with_disk(M.DISK0), "library")
    assert "library:device-only" in M.illegal(dataclasses.replace(s.with_disk(M.DISK0), pol=0.1), "library")


@pytest.mark.parametrize("owner", M.OWNERS)
def test_every_params_field_has_an_edit_and_the_match_list_is_changed_field_by_field(owner, committed):
    fields = [name for name, _ in _ffi.Params._fields_ if name != "reserved0"]
    assert set(fields) == set(M.PARAM_KINDS), "a bhg_params field without an edit kind (or an edit kind without its field)"
    assert set(M.MATCH_FIELDS) <= set(fields)
    # the model's list is the library's: two parameter sets that differ in one field match exactly when the field is not on it
    base = M.base_state(rhs_form=_ffi.RHS_KERR_BL, spin=0.25, max_step=2.0).make_params()
    for name in fields:
        other = M.base_state(rhs_form=_ffi.RHS_KERR_BL, spin=0.25, max_step=2.0).make_params()
        setattr(other, name, type(getattr(other, name))(getattr(other, name) + 1))
        assert _ffi.start_steps_match(base, other) == (name not in M.MATCH_FIELDS), name
    seen, alone = set(), set()
    for name, (seq, _) in committed[owner].items():
        before = seq[0].after
        for e in seq[1:]:
            changed = tuple(f for f in fields if e.after.p(f) != before.p(f))
            if e.refused:
                changed = tuple(f for f in fields if e.refused[0].p(f) != before.p(f))
            assert set(changed) <= set(e.fields), f"{owner} {name}: {e!r} changes {changed}"
            seen.update(changed)
            if len(changed) == 1:
                alone.add(changed[0])
            before = e.after
    assert seen == set(fields), f"{owner}: no committed seed edits {set(fields) - seen}"
    states = [e.after for seq, _ in committed[owner].values() for e in seq]
    assert {4, 12, 13, 15, 16, 0} <= {s.p("max_steps") for s in states}
    r0 = lambda s: sum(v * v for v in s.origin) ** 0.5   # noqa: E731
    assert {"off", "outside", "inside"} == {"off" if s.p("r_exit") == 0.0 else "inside" if s.p("r_exit") < r0(s) else "outside" for s in states}
    assert set(M.MATCH_FIELDS) <= alone, f"{owner}: never changed alone: {set(M.MATCH_FIELDS) - alone}"


@pytest.mark.parametrize("owner", M.OWNERS)
def test_the_committed_seeds_take_every_owner_branch_twice(owner, committed):
    total = dict.fromkeys(M.BRANCHES, 0)
    for name, (seq, env) in committed[owner].items():
        events = M.simulate(seq, *M.rules(env))
        assert len(events) == sum(1 + e.dwell for e in seq)
        for b, n in M.branches(events).items():
            total[b] += n
        flat = [ev for ev in events]
        if name.startswith("ladder"):
            # the scripted quiet run: records from scratch, 32 replays, the wide rule at the 34th trace, 96 further replays, the rim
            # rule at the 131st, and a replay of the rim records withheld under a budget of 15 and of 13 steps
            assert flat[0] == ["scratch"] and all(ev == ["replay"] for ev in flat[1:33]) and flat[33] == ["promote:wide"], _listing(seq)
            assert all(ev == ["replay"] for ev in flat[34:130]) and flat[130] == ["promote:rim"], _listing(seq)
            assert flat[M.QUIET + 1] == ["withheld", "none"] and flat[M.QUIET + 4] == ["withheld", "none"], _listing(seq)
    assert all(n >= 2 for n in total.values()), f"{owner}: {total}"


@pytest.mark.parametrize("owner", M.OWNERS)
def test_the_committed_seeds_reach_what_the_device_test_counts(owner, committed):
    kinds = {e.kind for seq, _ in committed[owner].values() for e in seq}
    want = {"mesh:refit", "mesh:rebuild", "mesh:refit:rebuild_ratio=1", "mesh:instances:moved", "mesh:instances:K", "mesh:off", "dwell",
            "rot", "fov", "origin:little", "origin:plane", "sky", "disk:on", "disk:off", "disk:tex", "disk:profile", "sphere:pass:in",
            "sphere:stay:in", "sphere:grow:far", "redshift", "observer", "textures", "thermal", "motion", "kerr", "method", "time_like"}
    want |= {"polarisation", "layers", "layers:off"} if owner == "device" else {"rebalance", "refused:disk", "refused:mesh+spheres"}
    assert want <= kinds, f"{owner}: no committed seed has {sorted(want - kinds)}"
    if owner == "device":
        assert "refused:mesh+redshift" in kinds
        # shade() without trace(): after every kind of owner call, each setter on, changed and off
        edits = [e for seq, _ in committed[owner].values() for e in seq if e.reshade]
        assert {e.ops[0][0] for e in edits} == set(M.RESHADE_OPS)
        for setter in ("redshift", "observer", "textures", "thermal", "motion", "polarisation", "layers"):
            assert {"reshade:" + setter, f"reshade:{setter}:changed", f"reshade:{setter}:off"} <= kinds, setter
        assert {"reshade:" + k for k in ("sky", "sky:no-disk", "sky:no-objects", "rot", "fov", "origin:little", "colours", "sphere:move",
                                         "mesh:instances:on", "mesh:instances:moved", "mesh:instances:K", "mesh:instances:off",
                                         "mesh:refit:instances", "mesh:off")} <= kinds
        assert {e.after.layers[0] for seq, _ in committed[owner].values() for e in seq if e.after.layers} == {1, 2, 3, 4}
        assert any(e.after.layers and e.after.layers[2] != 0.0 for seq, _ in committed[owner].values() for e in seq)
    # what the mutation checks of the device test rest on: the spin changed under the observer camera, fov_y changed alone, atol
    # changed alone on the plain trace, and (DeviceFrame) a refit of a mesh that has instances
    steps = [(a.after, b) for seq, _ in committed[owner].values() for a, b in zip(seq, seq[1:])]
    assert any(e.kind == "spin" and e.after.observer is not None for _, e in steps)
    assert any(e.kind == "fov" and e.after.fov[0] == was.fov[0] and e.after.mesh is None and e.after.layers is None for was, e in steps)
    assert any(e.kind == "atol" and e.after.mesh is None and e.after.layers is None for _, e in steps)
    if owner == "device":
        assert any(e.kind == "mesh:refit" and e.after.mesh.instances is not None for _, e in steps)
    assert any(e.dwell >= 20 for seq, _ in committed[owner].values() for e in seq if e.kind == "dwell")

"""bhg_start_steps_match (BHG_START_STEPS) without a GPU: the one holder of the list of what a ray's initial DP5(4) step depends
on beside the ray itself -- rtol, atol, lambda_end, max_step and the metric (r_s, spin, time_like, rhs_form), and the integrator,
because only DP5(4) records a step.  Every owner of a start-step array (DeviceFrame, FrameBatch, bhg_frame) asks it."""
import ctypes as C

import numpy as np
import pytest


def _f():
    from blackhole_geodesic_calculator_amd import _ffi
    return _ffi


BASE = dict(r_s=1.0, lambda_end=50.0, max_step=np.inf, rtol=1e-3, atol=1e-6, rhs_form=2, spin=0.3)


@pytest.mark.parametrize("change", [dict(r_exit=40.0), dict(disk_r_in=3.0, disk_r_out=12.0), dict(max_steps=5000),
                                    dict(order_blocks=5), dict(h_fixed=0.5),
                                    dict(r_exit=35.0, disk_r_in=2.0, disk_r_out=9.0, max_steps=7, order_blocks=3)],
                         ids=lambda c: "+".join(c))
def test_fields_the_step_does_not_depend_on(change):
    f = _f()
    assert f.start_steps_match(f.make_params(**BASE), f.make_params(**{**BASE, **change}))
    assert f.start_steps_match(f.make_params(**{**BASE, **change}), f.make_params(**BASE))


@pytest.mark.parametrize("change", [dict(rtol=1e-4), dict(atol=1e-7), dict(lambda_end=49.0), dict(max_step=0.1), dict(r_s=1.25),
                                    dict(spin=0.45), dict(time_like=1), dict(rhs_form=0), dict(method=1)],
                         ids=lambda c: "+".join(c))
def test_each_field_of_the_list_alone(change):
    f = _f()
    a, b = f.make_params(**BASE), f.make_params(**{**BASE, **change})
    assert f.start_steps_match(a, a) and f.start_steps_match(b, b)
    assert not f.start_steps_match(a, b) and not f.start_steps_match(b, a)


def test_null_and_header():
    f = _f()
    L = f.load()
    p = f.make_params(**BASE)
    assert L.bhg_start_steps_match(None, C.byref(p)) == 0 and L.bhg_start_steps_match(C.byref(p), None) == 0
    assert "bhg_trace_start_device" in f.EXPORTS and "bhg_start_steps_match" in f.EXPORTS
    assert (f.START_NONE, f.START_RECORD, f.START_REPLAY) == (0, 1, 2)

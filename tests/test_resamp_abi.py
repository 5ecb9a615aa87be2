"""CPU: the host-side part of the rational_resampler_ccf C-ABI. Every argument error is refused with
its own message before any HIP call (no device is present here), through ctypes and through
ResampPlan, and the plan's accessors answer for a NULL plan."""
import ctypes

import numpy as np
import pytest

from newsched_amd import nsh


def test_resamp_plan_create_refuses_bad_arguments():
    L = nsh.lib()
    taps = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    h = ctypes.c_void_p()
    create = L.nsh_resamp_plan_create
    assert create(0, None, 4, 3, 2, ctypes.byref(h)) != 0 and b"nsh_resamp_plan_create: null pointer" in L.nsh_last_error()
    assert create(0, taps, 4, 3, 2, None) != 0 and b"nsh_resamp_plan_create: null pointer" in L.nsh_last_error()
    for ntaps in (0, -1, 1025):
        assert create(0, taps, ntaps, 3, 2, ctypes.byref(h)) != 0
        assert b"nsh_resamp_plan_create: ntaps must be in [1, 1024]" in L.nsh_last_error()
    for interp in (0, -3, 65, 128):
        assert create(0, taps, 4, interp, 2, ctypes.byref(h)) != 0
        assert b"nsh_resamp_plan_create: interpolation must be in [1, 64]" in L.nsh_last_error()
    for decim in (0, -1, 65, 147):
        assert create(0, taps, 4, 3, decim, ctypes.byref(h)) != 0
        assert b"nsh_resamp_plan_create: decimation must be in [1, 64]" in L.nsh_last_error()
    assert not h.value


def test_resamp_plan_class_refuses_bad_arguments():
    with pytest.raises(nsh.NshError, match=r"interpolation must be in \[1, 64\]"):
        nsh.ResampPlan([1.0, 2.0], 0, 1)
    with pytest.raises(nsh.NshError, match=r"interpolation must be in \[1, 64\]"):
        nsh.ResampPlan([1.0, 2.0], 160, 147)
    with pytest.raises(nsh.NshError, match=r"decimation must be in \[1, 64\]"):
        nsh.ResampPlan([1.0, 2.0], 64, 65)
    with pytest.raises(nsh.NshError, match=r"decimation must be in \[1, 64\]"):
        nsh.ResampPlan([1.0, 2.0], 1, 0)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 1024\]"):
        nsh.ResampPlan([], 3, 2)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 1024\]"):
        nsh.ResampPlan(np.ones(1025, np.float32), 64, 1)


def test_resamp_call_refuses_bad_arguments():
    L = nsh.lib()
    a, b, c, d = (ctypes.c_void_p(16 * i) for i in range(1, 5))
    run = L.nsh_resamp_ccf
    assert run(None, a, b, c, d, 16, None) != 0 and b"nsh_resamp_ccf: null plan" in L.nsh_last_error()
    assert run(None, a, b, c, d, 0, None) != 0 and b"null plan" in L.nsh_last_error()
    assert run(None, None, b, c, d, 16, None) != 0 and b"nsh_resamp_ccf: null input or output" in L.nsh_last_error()
    assert run(None, a, b, c, None, 16, None) != 0 and b"null input or output" in L.nsh_last_error()
    assert run(None, a, b, b, d, 16, None) != 0 and b"nsh_resamp_ccf: hist_out must not alias hist_in" in L.nsh_last_error()


def test_resamp_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_resamp_tile(None) == 0
    assert L.nsh_resamp_kernel(None) == b""
    assert L.nsh_resamp_history(None) == 0
    assert L.nsh_resamp_plan_destroy(None) == 0

"""CPU: the host-side part of the pfb_synthesizer_ccf C-ABI. Every argument error is refused with its
own message before any HIP call (no device is present here), through ctypes and through PfbSynthPlan,
and the plan's accessors answer for a NULL plan. The one refusal that needs a live plan, a missing
hist_out, is checked on the GPU (tests/test_gpu_pfb_synth.py)."""
import ctypes

import numpy as np
import pytest

from newsched_amd import nsh


def test_synth_plan_create_refuses_bad_arguments():
    L = nsh.lib()
    taps = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    h = ctypes.c_void_p()
    create = L.nsh_pfb_synth_plan_create
    assert create(0, None, 4, 4, ctypes.byref(h)) != 0
    assert b"nsh_pfb_synth_plan_create: null pointer" in L.nsh_last_error()
    assert create(0, taps, 4, 4, None) != 0 and b"nsh_pfb_synth_plan_create: null pointer" in L.nsh_last_error()
    for ntaps in (0, -1, 1025):
        assert create(0, taps, ntaps, 4, ctypes.byref(h)) != 0
        assert b"nsh_pfb_synth_plan_create: ntaps must be in [1, 1024]" in L.nsh_last_error()
    for nchans in (0, 1, -4, 3, 6, 12, 48, 65, 128):
        assert create(0, taps, 4, nchans, ctypes.byref(h)) != 0
        assert b"nsh_pfb_synth_plan_create: nchans must be a power of two in [2, 64]" in L.nsh_last_error()
    for ntaps, nchans in ((65, 2), (129, 4), (1024, 16), (1024, 8)):
        big = (ctypes.c_float * ntaps)()
        assert create(0, big, ntaps, nchans, ctypes.byref(h)) != 0
        assert b"nsh_pfb_synth_plan_create: at most 32 taps per branch" in L.nsh_last_error()
    assert not h.value


def test_synth_plan_class_refuses_bad_arguments():
    with pytest.raises(nsh.NshError, match="nchans must be a power of two"):
        nsh.PfbSynthPlan([1.0, 2.0], 12)
    with pytest.raises(nsh.NshError, match="nchans must be a power of two"):
        nsh.PfbSynthPlan([1.0, 2.0], 128)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 1024\]"):
        nsh.PfbSynthPlan([], 4)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 1024\]"):
        nsh.PfbSynthPlan(np.ones(1025, np.float32), 64)
    with pytest.raises(nsh.NshError, match="at most 32 taps per branch"):
        nsh.PfbSynthPlan(np.ones(65, np.float32), 2)


def test_synth_call_refuses_bad_arguments():
    L = nsh.lib()
    a, b, c, d = (ctypes.c_void_p(16 * i) for i in range(1, 5))
    run = L.nsh_pfb_synthesizer_ccf
    assert run(None, a, b, c, d, 16, None) != 0 and b"nsh_pfb_synthesizer_ccf: null plan" in L.nsh_last_error()
    assert run(None, a, b, c, d, 0, None) != 0 and b"null plan" in L.nsh_last_error()
    assert run(None, None, b, c, d, 16, None) != 0
    assert b"nsh_pfb_synthesizer_ccf: null input or output" in L.nsh_last_error()
    assert run(None, a, b, c, None, 16, None) != 0 and b"null input or output" in L.nsh_last_error()
    assert run(None, a, b, b, d, 16, None) != 0
    assert b"nsh_pfb_synthesizer_ccf: hist_out must not alias hist_in" in L.nsh_last_error()


def test_synth_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_pfb_synth_tile(None) == 0
    assert L.nsh_pfb_synth_kernel(None) == b""
    assert L.nsh_pfb_synth_plan_destroy(None) == 0

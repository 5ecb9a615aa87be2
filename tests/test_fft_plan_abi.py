"""CPU: the FFT plan's C-ABI (nsh_fft_plan_create .. nsh_fft_c2c) where it needs no GPU: every
refusal happens before any HIP call and leaves its message in nsh_last_error, nframes <= 0 is a
no-op whatever the pointers, and the accessors answer 0 for a NULL plan. (The binding's signatures against the
header: tests/test_abi.py.)"""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import ONE, TWO, refused


def create(size, window=None, out=True, inverse=0, shift=0):
    h = C.c_void_p()
    arr = None
    if window is not None:
        w = np.ascontiguousarray(window, np.float32)
        arr = w.ctypes.data_as(C.POINTER(C.c_float))
    return nsh.lib().nsh_fft_plan_create(0, size, inverse, arr, shift, C.byref(h) if out else None), h


@pytest.mark.parametrize("size", [0, -16, 1, 8, 15, 24, 1000, 1025, 12288, 16384, 1 << 20])
def test_create_refuses_bad_sizes(size):
    rc, h = create(size)
    refused(rc, b"nsh_fft_plan_create: fft_size must be a power of two in [16, 8192]")
    assert not h.value


def test_create_refuses_null_out_pointer():
    rc, _ = create(1024, out=False)
    refused(rc, b"nsh_fft_plan_create: null pointer")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("size,at", [(16, 0), (64, 63), (8192, 4097)])
def test_create_refuses_nonfinite_window(bad, size, at):
    w = np.ones(size, np.float32)
    w[at] = bad
    rc, h = create(size, w)
    refused(rc, b"nsh_fft_plan_create: window entry is not finite")
    assert not h.value


def test_run_refuses_null_and_aliased_pointers():
    L = nsh.lib()
    refused(L.nsh_fft_c2c(None, None, TWO, 1, None), b"nsh_fft_c2c: null pointer")
    refused(L.nsh_fft_c2c(None, ONE, None, 1, None), b"nsh_fft_c2c: null pointer")
    refused(L.nsh_fft_c2c(None, ONE, ONE, 1, None), b"nsh_fft_c2c: in-place not supported")
    refused(L.nsh_fft_c2c(None, ONE, TWO, 1, None), b"nsh_fft_c2c: null plan")


def test_grid_cap_refusals():
    L = nsh.lib()
    refused(L.nsh_fft_plan_grid_cap(None, -1), b"nsh_fft_plan_grid_cap: negative cap")
    refused(L.nsh_fft_plan_grid_cap(None, 2), b"nsh_fft_plan_grid_cap: null plan")


@pytest.mark.parametrize("nframes", [0, -1, -(1 << 40)])
def test_no_frames_is_a_no_op_with_any_pointers(nframes):
    L = nsh.lib()
    for plan, a, b in ((None, None, None), (None, ONE, ONE), (None, ONE, TWO), (ONE, None, None)):
        assert L.nsh_fft_c2c(plan, a, b, nframes, None) == 0


def test_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_fft_plan_size(None) == 0
    assert L.nsh_fft_tile(None) == 0
    assert L.nsh_fft_kernel(None) == b""
    assert L.nsh_fft_plan_destroy(None) == 0


@pytest.mark.parametrize("size", [0, 8, 24, 1000, 16384])
def test_fftplan_raises_for_bad_sizes(size):
    with pytest.raises(nsh.NshError, match="fft_size must be a power of two"):
        nsh.FftPlan(size)


def test_fftplan_raises_for_a_window_of_the_wrong_length():
    with pytest.raises(nsh.NshError, match="window"):
        nsh.FftPlan(64, window=np.ones(63, np.float32))

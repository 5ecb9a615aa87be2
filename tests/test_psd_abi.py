"""CPU: the C-ABI of psd_vcf (nsh_psd_plan_create .. nsh_psd_cf) where it needs no GPU: every refusal
happens before any HIP call, in the header's order, and leaves its message in nsh_last_error;
nvec <= 0 is a no-op whatever the pointers; the accessors answer 0 or "" for a NULL plan. (The binding's
signatures against the header: tests/test_abi.py. The overflow refusal of nsh_psd_cf needs a plan's sizes and is checked on
the GPU, tests/test_gpu_psd.py.)"""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import ONE, TWO, refused


BAD_SIZE = b"nsh_psd_plan_create: fft_size must be a power of two in [16, 8192]"
BAD_NAVG = b"nsh_psd_plan_create: navg must be in [1, 65536]"
BAD_WINDOW = b"nsh_psd_plan_create: window entry is not finite"
BAD_SCALE = b"nsh_psd_plan_create: scale must be finite and > 0"


def create(fft_size, navg, window=None, scale=1.0, out=True, shift=0, db=0):
    h = C.c_void_p()
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    arr = None if w is None else w.ctypes.data_as(C.POINTER(C.c_float))
    rc = nsh.lib().nsh_psd_plan_create(0, fft_size, navg, arr, shift, scale, db, C.byref(h) if out else None)
    return rc, h


def test_create_refuses_a_null_out_pointer_first():
    # ... before the size, the count, the window and the scale are looked at
    rc, _ = create(7, 0, np.full(7, np.nan), scale=-1.0, out=False)
    refused(rc, b"nsh_psd_plan_create: null pointer")
    rc, _ = create(64, 4, out=False)
    refused(rc, b"nsh_psd_plan_create: null pointer")


@pytest.mark.parametrize("size", [-1024, 0, 1, 8, 24, 1000, 1025, 16384, 1 << 20])
def test_create_refuses_sizes(size):
    # a bad count, a NaN window and a bad scale behind a bad size: the size is what is reported
    rc, h = create(size, 0, np.full(16, np.nan), scale=0.0)
    refused(rc, BAD_SIZE)
    assert not h.value


@pytest.mark.parametrize("navg", [0, -1, 65537, 1 << 20, -(1 << 31)])
def test_create_refuses_frame_counts(navg):
    rc, h = create(64, navg, np.full(64, np.nan), scale=0.0)  # ... before the window and the scale
    refused(rc, BAD_NAVG)
    assert not h.value


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("N,at", [(16, 0), (64, 63), (8192, 4097)])
def test_create_refuses_nonfinite_window_entries(bad, N, at):
    w = np.ones(N, np.float32)
    w[at] = bad
    rc, h = create(N, 65536, w, scale=np.nan)  # ... before the scale
    refused(rc, BAD_WINDOW)
    assert not h.value


@pytest.mark.parametrize("scale", [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, -1e-30])
@pytest.mark.parametrize("window", [False, True])
def test_create_refuses_scales(scale, window):
    rc, h = create(1024, 1, np.ones(1024) if window else None, scale=scale)
    refused(rc, BAD_SCALE)
    assert not h.value


def test_run_refusals_in_order():
    run = nsh.lib().nsh_psd_cf
    # NULL in / out, whatever else is wrong
    refused(run(None, None, ONE, 1, None), b"nsh_psd_cf: null pointer")
    refused(run(None, ONE, None, 1, None), b"nsh_psd_cf: null pointer")
    refused(run(None, None, None, 1 << 62, None), b"nsh_psd_cf: null pointer")
    # then in == out, before the plan
    refused(run(None, ONE, ONE, 1, None), b"nsh_psd_cf: in-place not supported")
    # then the NULL plan
    refused(run(None, ONE, TWO, 1, None), b"nsh_psd_cf: null plan")
    refused(run(None, ONE, TWO, 1 << 62, None), b"nsh_psd_cf: null plan")


def test_grid_cap_refusals():
    L = nsh.lib()
    refused(L.nsh_psd_grid_cap(None, -1), b"nsh_psd_grid_cap: negative cap")
    refused(L.nsh_psd_grid_cap(None, 2), b"nsh_psd_grid_cap: null plan")
    refused(L.nsh_psd_grid_cap(None, 0), b"nsh_psd_grid_cap: null plan")


@pytest.mark.parametrize("nvec", [0, -1, -(1 << 40)])
def test_no_vectors_is_a_no_op_with_any_pointers(nvec):
    L = nsh.lib()
    for plan, a, b in ((None, None, None), (None, ONE, ONE), (ONE, None, None), (None, ONE, TWO)):
        assert L.nsh_psd_cf(plan, a, b, nvec, None) == 0


def test_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_psd_fft_size(None) == 0
    assert L.nsh_psd_navg(None) == 0
    assert L.nsh_psd_segment(None) == 0
    assert L.nsh_psd_tile(None) == 0
    assert L.nsh_psd_kernel(None) == b""
    assert L.nsh_psd_plan_destroy(None) == 0


def test_plan_class_raises_what_the_plan_refuses():
    with pytest.raises(nsh.NshError, match="fft_size must be a power of two"):
        nsh.PsdPlan(48, 4)
    with pytest.raises(nsh.NshError, match=r"navg must be in \[1, 65536\]"):
        nsh.PsdPlan(64, 0)
    with pytest.raises(nsh.NshError, match="window has 3 entries"):
        nsh.PsdPlan(64, 4, window=np.ones(3))
    with pytest.raises(nsh.NshError, match="window entry is not finite"):
        nsh.PsdPlan(64, 4, window=np.full(64, np.inf))
    with pytest.raises(nsh.NshError, match="scale must be finite and > 0"):
        nsh.PsdPlan(64, 4, scale=0.0)

"""CPU: the C-ABI of fft_filter_ccc (nsh_fft_filter_plan_create .. nsh_fft_filter_ccc) where it needs
no GPU: every refusal happens before any HIP call, in the header's order, and leaves its message in
nsh_last_error; n <= 0 is a no-op whatever the pointers; the accessors answer 0 or "" for a NULL
plan. (The binding's signatures against the header: tests/test_abi.py.)"""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import ONE, TWO, refused

THREE, FOUR = C.c_void_p(48), C.c_void_p(64)
BAD_SIZE = b"nsh_fft_filter_plan_create: fft_size must be 0, 1024, 2048, 4096 or 8192"


def create(taps, fft_size=0, ntaps=None, out=True, null_taps=False):
    h = C.c_void_p()
    t = np.ascontiguousarray(taps, np.complex64)
    arr = None if null_taps else t.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))
    rc = nsh.lib().nsh_fft_filter_plan_create(0, arr, t.size if ntaps is None else ntaps, fft_size,
                                              C.byref(h) if out else None)
    return rc, h


def test_create_refuses_null_pointers_first():
    # ... before the tap count, the taps and the size are looked at
    for kw in (dict(null_taps=True), dict(out=False)):
        rc, _ = create(np.full(4, np.nan), fft_size=7, ntaps=-3, **kw)
        refused(rc, b"nsh_fft_filter_plan_create: null pointer")


@pytest.mark.parametrize("ntaps", [0, -1, 4097, 1 << 20])
def test_create_refuses_tap_counts(ntaps):
    # a bad size and a NaN tap behind a bad count: the count is what is reported
    rc, h = create(np.full(4, np.nan), fft_size=7, ntaps=ntaps)
    refused(rc, b"nsh_fft_filter_plan_create: ntaps must be in [1, 4096]")
    assert not h.value


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("L,at,part", [(1, 0, 0), (127, 126, 1), (4096, 2048, 0)])
def test_create_refuses_nonfinite_taps(bad, L, at, part):
    t = np.ones(L, np.complex64)
    t[at] = complex(bad, 1.0) if part == 0 else complex(1.0, bad)
    rc, h = create(t, fft_size=7)  # ... before the bad size
    refused(rc, b"nsh_fft_filter_plan_create: tap is not finite")
    assert not h.value


@pytest.mark.parametrize("size", [-1024, 1, 16, 512, 1000, 1025, 3072, 16384, 1 << 20])
def test_create_refuses_sizes(size):
    rc, h = create(np.ones(4000), fft_size=size)  # ... before ntaps > fft_size / 2
    refused(rc, BAD_SIZE)
    assert not h.value


@pytest.mark.parametrize("size,L", [(1024, 513), (2048, 1025), (4096, 2049), (4096, 4096), (1024, 4096)])
def test_create_refuses_taps_longer_than_half_a_frame(size, L):
    rc, h = create(np.ones(L), fft_size=size)
    refused(rc, b"nsh_fft_filter_plan_create: ntaps must be at most fft_size / 2")
    assert not h.value


def test_without_a_device_create_fails_where_the_xlat_plan_is_made():
    """The two entry points share one plan and differ in this: nsh_fft_filter_plan_create needs its
    device at once, nsh_fft_xlat_plan_create makes the plan and uploads on first use."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("needs a machine without a device")
    L = nsh.lib()
    t = np.ones(127, np.complex64)
    rc, h = create(t)
    assert rc != 0 and not h.value
    assert b"hipSetDevice(dev)" in L.nsh_last_error()  # HIP's own error, after every refusal of the arguments
    x = C.c_void_p()
    arr = t.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.nsh_fft_xlat_plan_create(0, arr, t.size, 1, 0.0, 0, C.byref(x)) == 0 and x.value
    assert L.nsh_fft_xlat_valid(x) == 1024 - 126
    assert L.nsh_fft_xlat_plan_destroy(x) == 0


def test_run_refusals_in_order():
    L = nsh.lib()
    run = L.nsh_fft_filter_ccc
    # NULL in / out, whatever else is wrong
    refused(run(None, None, ONE, ONE, None, 1, None), b"nsh_fft_filter_ccc: null input or output")
    refused(run(None, ONE, ONE, ONE, None, 1, None), b"nsh_fft_filter_ccc: null input or output")
    # then in == out, before the histories
    refused(run(None, ONE, THREE, THREE, ONE, 1, None), b"nsh_fft_filter_ccc: in-place not supported")
    # then aliased histories, before the plan
    refused(run(None, ONE, THREE, THREE, TWO, 1, None), b"nsh_fft_filter_ccc: hist_out must not alias hist_in")
    # then the NULL plan (two NULL histories alias nothing); the missing hist_out needs a plan's tap
    # count and is checked on the GPU (tests/test_gpu_fft_filter.py)
    refused(run(None, ONE, None, None, TWO, 1, None), b"nsh_fft_filter_ccc: null plan")
    refused(run(None, ONE, THREE, FOUR, TWO, 1, None), b"nsh_fft_filter_ccc: null plan")


def test_grid_cap_refusals():
    L = nsh.lib()
    refused(L.nsh_fft_filter_grid_cap(None, -1), b"nsh_fft_filter_grid_cap: negative cap")
    refused(L.nsh_fft_filter_grid_cap(None, 2), b"nsh_fft_filter_grid_cap: null plan")
    refused(L.nsh_fft_filter_grid_cap(None, 0), b"nsh_fft_filter_grid_cap: null plan")


@pytest.mark.parametrize("n", [0, -1, -(1 << 40)])
def test_no_samples_is_a_no_op_with_any_pointers(n):
    L = nsh.lib()
    for plan, a, hi, ho, b in ((None, None, None, None, None), (None, ONE, TWO, TWO, ONE), (ONE, None, None, None, None),
                               (None, ONE, None, None, TWO)):
        assert L.nsh_fft_filter_ccc(plan, a, hi, ho, b, n, None) == 0


def test_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_fft_filter_fft_size(None) == 0
    assert L.nsh_fft_filter_valid(None) == 0
    assert L.nsh_fft_filter_history(None) == 0
    assert L.nsh_fft_filter_tile(None) == 0
    assert L.nsh_fft_filter_kernel(None) == b""
    assert L.nsh_fft_filter_plan_destroy(None) == 0


def test_plan_class_raises_what_the_plan_refuses():
    with pytest.raises(nsh.NshError, match="ntaps must be at most fft_size / 2"):
        nsh.FftFilterPlan(np.ones(600, np.complex64), fft_size=1024)
    with pytest.raises(nsh.NshError, match="fft_size must be 0, 1024"):
        nsh.FftFilterPlan(np.ones(3, np.complex64), fft_size=512)
    with pytest.raises(nsh.NshError, match="tap is not finite"):
        nsh.FftFilterPlan(np.array([1, np.nan], np.complex64))

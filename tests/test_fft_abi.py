"""CPU: the host-side part of the nsh_fft1024_c2c / nsh_channelizer1024 C-ABI. Every argument error
is refused with its own message before any HIP call (no device is present here), and a call with
nothing to do returns 0 whatever its pointers are."""
import ctypes

import pytest

from newsched_amd import nsh


def test_fft_refuses_bad_arguments():
    L = nsh.lib()
    a, b = ctypes.c_void_p(1024), ctypes.c_void_p(16384)
    run = L.nsh_fft1024_c2c
    for inverse in (0, 1):
        assert run(a, a, 4, inverse, None) != 0
        assert b"nsh_fft1024_c2c: in-place not supported" in L.nsh_last_error()
        assert run(None, b, 4, inverse, None) != 0 and b"nsh_fft1024_c2c: null pointer" in L.nsh_last_error()
        assert run(a, None, 4, inverse, None) != 0 and b"nsh_fft1024_c2c: null pointer" in L.nsh_last_error()
        assert run(None, None, 1, inverse, None) != 0 and b"nsh_fft1024_c2c: null pointer" in L.nsh_last_error()


def test_channelizer_refuses_bad_arguments():
    L = nsh.lib()
    a, b, w = ctypes.c_void_p(1024), ctypes.c_void_p(16384), ctypes.c_void_p(65536)
    run = L.nsh_channelizer1024
    assert run(a, a, w, 4, None) != 0
    assert b"nsh_channelizer1024: in-place not supported" in L.nsh_last_error()
    assert run(a, b, None, 4, None) != 0 and b"nsh_channelizer1024: null pointer" in L.nsh_last_error()
    assert run(None, b, w, 4, None) != 0 and b"nsh_channelizer1024: null pointer" in L.nsh_last_error()
    assert run(a, None, w, 4, None) != 0 and b"nsh_channelizer1024: null pointer" in L.nsh_last_error()
    assert run(a, a, None, 4, None) != 0 and b"nsh_channelizer1024: null pointer" in L.nsh_last_error()


@pytest.mark.parametrize("nframes", [0, -1, -(1 << 40)])
def test_nothing_to_do_returns_zero(nframes):
    """nframes <= 0: no error and no launch, even with NULL or aliased pointers."""
    L = nsh.lib()
    a = ctypes.c_void_p(1024)
    for inverse in (0, 1):
        assert L.nsh_fft1024_c2c(None, None, nframes, inverse, None) == 0
        assert L.nsh_fft1024_c2c(a, a, nframes, inverse, None) == 0
    assert L.nsh_channelizer1024(None, None, None, nframes, None) == 0
    assert L.nsh_channelizer1024(a, a, None, nframes, None) == 0


def test_wrappers_raise_with_the_message():
    with pytest.raises(nsh.NshError, match="nsh_fft1024_c2c.*in-place"):
        nsh.check(nsh.lib().nsh_fft1024_c2c(64, 64, 1, 0, None), "nsh_fft1024_c2c")
    with pytest.raises(nsh.NshError, match="nsh_channelizer1024.*null pointer"):
        nsh.check(nsh.lib().nsh_channelizer1024(64, 128, None, 1, None), "nsh_channelizer1024")


def test_fft_binding_covers_the_entries():
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert nsh.SIGNATURES["nsh_fft1024_c2c"] == (i, [vp, vp, i64, i, vp])
    assert nsh.SIGNATURES["nsh_channelizer1024"] == (i, [vp, vp, vp, i64, vp])

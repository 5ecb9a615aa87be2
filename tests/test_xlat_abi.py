"""CPU: the host-side part of the rotator / frequency-translating FIR C-ABI. nsh_phase_inc against
exact rational arithmetic, and every argument error refused with its own message before any HIP call
(no device is present here)."""
import ctypes
import math
from fractions import Fraction

import pytest

from newsched_amd import nsh


def exact_inc(t: float) -> int:
    """round(frac(t) * 2^64) mod 2^64 from the double's exact value (round: ties to even)."""
    f = Fraction(t)
    return round((f - math.floor(f)) * 2**64) % 2**64


@pytest.mark.parametrize("t", [0.0, 0.25, -0.25, 0.1, -0.37, 1e-9, 0.4999999, 3.75])
def test_phase_inc_exact(t):
    assert nsh.phase_inc(t) == exact_inc(t)
    inc = ctypes.c_uint64(1)
    assert nsh.lib().nsh_phase_inc(t, ctypes.byref(inc)) == 0 and inc.value == exact_inc(t)


def test_phase_inc_known_values():
    assert nsh.phase_inc(0.25) == 1 << 62
    assert nsh.phase_inc(-0.25) == 3 << 62
    assert nsh.phase_inc(3.75) == 3 << 62
    assert nsh.phase_inc(-1e-30) == 0          # frac rounds up to one turn: wraps to 0
    assert nsh.phase_inc(2.0 ** -65) == 0      # a tie: to even
    assert nsh.phase_inc(3 * 2.0 ** -65) == 2  # 1.5 -> 2


@pytest.mark.parametrize("t", [float("nan"), float("inf"), float("-inf")])
def test_phase_inc_refuses_non_finite(t):
    L = nsh.lib()
    inc = ctypes.c_uint64(0)
    assert L.nsh_phase_inc(t, ctypes.byref(inc)) != 0
    assert b"finite" in L.nsh_last_error()
    with pytest.raises(nsh.NshError):
        nsh.phase_inc(t)
    assert L.nsh_phase_inc(0.1, None) != 0 and b"null" in L.nsh_last_error()


def test_rotate_refuses_null_before_launch():
    L = nsh.lib()
    one = ctypes.c_void_p(16)
    assert L.nsh_rotate_cc(None, one, 8, 1, 0, None) != 0 and b"nsh_rotate_cc: null" in L.nsh_last_error()
    assert L.nsh_rotate_cc(one, None, 8, 1, 0, None) != 0 and b"nsh_rotate_cc: null" in L.nsh_last_error()
    assert L.nsh_rotate_cc(None, None, 0, 1, 0, None) == 0    # nothing to do: no error, no launch
    assert L.nsh_rotate_cc(one, one, -3, 1, 0, None) == 0


def test_xlat_plan_create_refuses_bad_arguments():
    L = nsh.lib()
    taps = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    h = ctypes.c_void_p()
    create = L.nsh_fir_xlat_plan_create
    assert create(0, None, 4, 1, 0.1, ctypes.byref(h)) != 0 and b"null pointer" in L.nsh_last_error()
    assert create(0, taps, 4, 1, 0.1, None) != 0 and b"null pointer" in L.nsh_last_error()
    for ntaps in (0, -1, 1025):
        assert create(0, taps, ntaps, 1, 0.1, ctypes.byref(h)) != 0
        assert b"ntaps must be in [1, 1024]" in L.nsh_last_error()
    for decim in (0, -2, 65):
        assert create(0, taps, 4, decim, 0.1, ctypes.byref(h)) != 0
        assert b"decimation must be in [1, 64]" in L.nsh_last_error()
    for f in (float("nan"), float("inf")):
        assert create(0, taps, 4, 1, f, ctypes.byref(h)) != 0
        assert b"frequency must be finite" in L.nsh_last_error()
    assert not h.value
    with pytest.raises(nsh.NshError, match="decimation"):
        nsh.FirXlatPlan([1.0, 2.0], 100, 0.1)


def test_xlat_call_refuses_bad_arguments():
    L = nsh.lib()
    a, b, c, d = (ctypes.c_void_p(16 * i) for i in range(1, 5))
    run = L.nsh_fir_xlat_ccf
    assert run(None, a, b, c, d, 16, 0, None) != 0 and b"null plan" in L.nsh_last_error()
    assert run(None, a, b, c, d, 0, 0, None) != 0 and b"null plan" in L.nsh_last_error()
    assert run(None, None, b, c, d, 16, 0, None) != 0 and b"null input or output" in L.nsh_last_error()
    assert run(None, a, b, c, None, 16, 0, None) != 0 and b"null input or output" in L.nsh_last_error()
    assert run(None, a, b, b, d, 16, 0, None) != 0 and b"must not alias" in L.nsh_last_error()
    # the plan's accessors on a null plan
    assert L.nsh_fir_xlat_tile(None) == 0
    assert L.nsh_fir_xlat_kernel(None) == b""
    inc = ctypes.c_uint64(0)
    assert L.nsh_fir_xlat_phase_inc(None, ctypes.byref(inc)) != 0 and b"null" in L.nsh_last_error()
    assert L.nsh_fir_xlat_plan_destroy(None) == 0

"""CPU: the host-side part of the pfb_arb_resampler_ccf C-ABI. Every argument error is refused with its
own message before any HIP call (no device is present here), through ctypes and through ArbPlan; the
plan's accessors answer for a NULL plan; and nsh_arb_step / nsh_arb_span, which make no HIP call, are
checked against Python big-integer arithmetic: random cases, the edges of the rate, the fraction and
the counts, and chained random cuts against one call's index sequence."""
import ctypes
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from newsched_amd import nsh

M31 = 2 ** 31 - 1


def ref_step(rate, F):
    """round(F 2^32 / rate), exact from the double, ties to even."""
    return round(Fraction(F * 2 ** 32) / Fraction(rate))


def ref_span(step, F, phase, n_in, want):
    unit = F * 2 ** 32
    n_max = max(0, -((phase - n_in * unit) // step)) if n_in * unit > phase else 0
    n_out = min(want, n_max, M31)
    pos = phase + n_out * step
    c = min(pos // unit, n_in)
    return n_out, c, pos - c * unit


def indices(step, F, phase, n):
    """(i, j, fraction) of the outputs 0 .. n-1 from phase."""
    return [((phase + m * step) >> 32) // F for m in range(n)], \
           [((phase + m * step) >> 32) % F for m in range(n)], [(phase + m * step) & 0xffffffff for m in range(n)]


def test_arb_plan_create_refuses_bad_arguments():
    L = nsh.lib()
    taps = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    h = ctypes.c_void_p()
    create = L.nsh_arb_plan_create
    assert create(0, None, 4, 32, 1.5, ctypes.byref(h)) != 0 and b"nsh_arb_plan_create: null pointer" in L.nsh_last_error()
    assert create(0, taps, 4, 32, 1.5, None) != 0 and b"nsh_arb_plan_create: null pointer" in L.nsh_last_error()
    for nfilt in (0, 1, -2, 3, 24, 128, 65):
        assert create(0, taps, 4, nfilt, 1.5, ctypes.byref(h)) != 0
        assert b"nsh_arb_plan_create: nfilt must be a power of two in [2, 64]" in L.nsh_last_error()
    for ntaps in (0, -1, 2049):
        assert create(0, taps, ntaps, 32, 1.5, ctypes.byref(h)) != 0
        assert b"nsh_arb_plan_create: ntaps must be in [1, 2048]" in L.nsh_last_error()
    for rate in (math.nan, math.inf, -math.inf, 0.0, -1.0, 1 / 64.0001, 64.0001, 1e300):
        assert create(0, taps, 4, 32, rate, ctypes.byref(h)) != 0
        assert b"nsh_arb_plan_create: rate must be finite and in [1/64, 64]" in L.nsh_last_error()
    assert not h.value


def test_arb_plan_class_refuses_bad_arguments():
    with pytest.raises(nsh.NshError, match=r"nfilt must be a power of two in \[2, 64\]"):
        nsh.ArbPlan([1.0, 2.0], 1.5, 48)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 2048\]"):
        nsh.ArbPlan([], 1.5)
    with pytest.raises(nsh.NshError, match=r"ntaps must be in \[1, 2048\]"):
        nsh.ArbPlan(np.ones(2049, np.float32), 1.5, 64)
    with pytest.raises(nsh.NshError, match=r"rate must be finite and in \[1/64, 64\]"):
        nsh.ArbPlan([1.0, 2.0], 65.0)
    with pytest.raises(nsh.NshError, match=r"rate must be finite and in \[1/64, 64\]"):
        nsh.ArbPlan([1.0, 2.0], float("nan"))


def test_arb_call_refuses_bad_arguments():
    L = nsh.lib()
    a, b, c, d = (ctypes.c_void_p(16 * i) for i in range(1, 5))
    run = L.nsh_arb_resamp_ccf
    assert run(None, a, 16, b, c, d, 16, 0, None) != 0 and b"nsh_arb_resamp_ccf: null plan" in L.nsh_last_error()
    assert run(None, a, 0, b, c, d, 0, 0, None) != 0 and b"null plan" in L.nsh_last_error()
    assert run(None, None, 16, b, c, d, 16, 0, None) != 0 and b"nsh_arb_resamp_ccf: null input or output" in L.nsh_last_error()
    assert run(None, a, 16, b, c, None, 16, 0, None) != 0 and b"null input or output" in L.nsh_last_error()
    assert run(None, a, 16, b, b, d, 16, 0, None) != 0 and b"nsh_arb_resamp_ccf: hist_out must not alias hist_in" in L.nsh_last_error()
    assert run(None, a, 2 ** 31, b, c, d, 16, 0, None) != 0
    assert b"nsh_arb_resamp_ccf: n_in and n_out must not exceed 2^31 - 1" in L.nsh_last_error()
    assert run(None, a, 16, b, c, d, 2 ** 31, 0, None) != 0
    assert b"nsh_arb_resamp_ccf: n_in and n_out must not exceed 2^31 - 1" in L.nsh_last_error()


def test_arb_null_plan_accessors():
    L = nsh.lib()
    assert L.nsh_arb_tile(None) == 0
    assert L.nsh_arb_kernel(None) == b""
    assert L.nsh_arb_history(None) == 0
    assert L.nsh_arb_plan_destroy(None) == 0
    step = ctypes.c_uint64(7)
    assert L.nsh_arb_plan_step(None, ctypes.byref(step)) != 0 and b"nsh_arb_plan_step: null pointer" in L.nsh_last_error()


def test_arb_step_refusals():
    L = nsh.lib()
    step = ctypes.c_uint64(0)
    assert L.nsh_arb_step(1.5, 32, None) != 0 and b"nsh_arb_step: null pointer" in L.nsh_last_error()
    for nfilt in (0, 1, 3, 128):
        assert L.nsh_arb_step(1.5, nfilt, ctypes.byref(step)) != 0
        assert b"nsh_arb_step: nfilt must be a power of two in [2, 64]" in L.nsh_last_error()
    for rate in (math.nan, math.inf, 0.0, -2.0, 64.5, 0.015):
        assert L.nsh_arb_step(rate, 32, ctypes.byref(step)) != 0
        assert b"nsh_arb_step: rate must be finite and in [1/64, 64]" in L.nsh_last_error()
    with pytest.raises(nsh.NshError, match="rate must be finite"):
        nsh.arb_step(1e9)


def test_arb_span_refusals():
    L = nsh.lib()
    n, c, p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_uint64(0)
    out = (ctypes.byref(n), ctypes.byref(c), ctypes.byref(p))
    step = nsh.arb_step(1.0, 32)
    assert L.nsh_arb_span(step, 32, 0, 10, 10, None, out[1], out[2]) != 0 and b"nsh_arb_span: null pointer" in L.nsh_last_error()
    assert L.nsh_arb_span(step, 32, 0, 10, 10, out[0], None, out[2]) != 0 and b"null pointer" in L.nsh_last_error()
    assert L.nsh_arb_span(step, 32, 0, 10, 10, out[0], out[1], None) != 0 and b"null pointer" in L.nsh_last_error()
    assert L.nsh_arb_span(step, 48, 0, 10, 10, *out) != 0 and b"nsh_arb_span: nfilt must be a power of two in [2, 64]" in L.nsh_last_error()
    for bad in (0, 1, nsh.arb_step(1 / 64, 32) + 1, nsh.arb_step(64.0, 32) - 1, 2 ** 63):
        assert L.nsh_arb_span(bad, 32, 0, 10, 10, *out) != 0
        assert b"nsh_arb_span: step is not that of a rate in [1/64, 64]" in L.nsh_last_error()
    for n_in, want in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert L.nsh_arb_span(step, 32, 0, n_in, want, *out) != 0
        assert b"nsh_arb_span: n_in and want_out must be in [0, 2^31 - 1]" in L.nsh_last_error()


def test_arb_step_matches_big_integer_arithmetic():
    rng = random.Random(1)
    rates = [64.0, 1 / 64, 1.0, 160 / 147, 147 / 160, 1.0000001, 3.7, 1 / 7.3, math.pi / 3, 0.5, 2.0, 1 + 30e-6,
             math.nextafter(64.0, 0), math.nextafter(1 / 64, 1), 1 / 3, 3.0]
    rates += [math.exp(rng.uniform(math.log(1 / 64), math.log(64))) for _ in range(3000)]
    for rate in rates:
        for F in (2, 4, 8, 16, 32, 64):
            assert nsh.arb_step(rate, F) == ref_step(rate, F), (rate, F)
    assert nsh.arb_step(1.0, 32) == 32 << 32                  # zero fraction
    assert nsh.arb_step(64.0, 2) == 2 ** 27 and nsh.arb_step(1 / 64, 64) == 2 ** 44
    # a tie: 2 * 2^32 / r = m + 1/2 exactly, r = 2^34 / (2 m + 1)
    for m in (2 ** 31 + 1, 2 ** 31 + 2, 2 ** 33 + 5):
        r = Fraction(2 ** 34, 2 * m + 1)
        if Fraction(float(r)) == r:
            assert nsh.arb_step(float(r), 2) == (m if m % 2 == 0 else m + 1)


def span_cases():
    rng = random.Random(2)
    cases = []
    for _ in range(3000):
        F = rng.choice((2, 4, 8, 16, 32, 64))
        step = ref_step(math.exp(rng.uniform(math.log(1 / 64), math.log(64))), F)
        n_in = rng.choice((1, 2, 5, 100, 4096, rng.randrange(1, 1 << 20)))
        phase = rng.choice((0, rng.randrange(F << 32), rng.randrange(4033 << 32), rng.randrange(2 * n_in * F << 32)))
        want = rng.choice((0, 1, 7, rng.randrange(1 << 22), M31))
        cases.append((step, F, phase, n_in, want))
    for F in (2, 32, 64):
        unit = F << 32
        for step in (ref_step(64.0, F), ref_step(1 / 64, F), ref_step(1.0, F),  # the rate's ends, and a zero fraction
                     (F << 32) + 0xffffffff, (3 << 32) | 0xffffffff if F == 2 else (F << 31) | 0xffffffff,
                     (F << 32) + 1):
            for n_in in (0, 1, 2, 1000, M31 - 1, M31):
                for phase in (0, 1, unit - 1, unit, 5 * unit + 12345, n_in * unit - 1, n_in * unit, n_in * unit + 1,
                              (n_in + 9) * unit + 77, 2 ** 64 - 1):
                    if phase < 0 or phase >= 2 ** 64:
                        continue
                    for want in (0, 1, 1000, M31 - 1, M31):
                        cases.append((step, F, phase, n_in, want))
    return cases


def test_arb_span_matches_big_integer_arithmetic():
    for step, F, phase, n_in, want in span_cases():
        got = nsh.arb_span(step, F, phase, n_in, want)
        ref = ref_span(step, F, phase, n_in, want)
        assert got == ref, (step, F, phase, n_in, want, got, ref)
        n_out, c, nxt = got
        assert 0 <= c <= n_in and 0 <= n_out <= want and 0 <= nxt < 2 ** 64
        if n_out:                                             # the last output's window ends inside the input
            assert ((phase + (n_out - 1) * step) >> 32) // F <= n_in - 1
        if n_out < want and n_out < M31:                      # and one more would not
            assert ((phase + n_out * step) >> 32) // F >= n_in


def test_arb_chained_cuts_reproduce_one_call():
    rng = random.Random(3)
    for _ in range(300):
        F = rng.choice((2, 8, 32, 64))
        step = ref_step(math.exp(rng.uniform(math.log(1 / 64), math.log(64))), F)
        n_in = rng.randrange(1, 3000)
        phase0 = rng.choice((0, rng.randrange(F << 32), rng.randrange(200 * F << 32)))
        total, c_all, nxt_all = nsh.arb_span(step, F, phase0, n_in, M31)
        i_all, j_all, f_all = indices(step, F, phase0, total)
        i_got, j_got, f_got = [], [], []
        pos, phase, worst = 0, phase0, 0
        while pos < n_in:
            n = min(rng.choice((1, 2, 3, 17, 64, 500)), n_in - pos)
            want = rng.choice((0, 1, 5, 100, M31))
            n_out, c, nxt = nsh.arb_span(step, F, phase, n, want)
            i, j, f = indices(step, F, phase, n_out)
            assert all(v <= n - 1 for v in i)
            i_got += [pos + v for v in i]; j_got += j; f_got += f
            if n_out == 0 and c == 0:                        # want = 0 and nothing to skip: no progress is right
                assert want == 0 or n == 0
            pos += c
            phase = nxt
            worst = max(worst, 0 if phase0 >> 32 > 4032 else phase >> 32)
        assert (i_got, j_got, f_got) == (i_all, j_all, f_all)
        assert phase == nxt_all and pos == c_all == n_in
        assert worst <= max(4032, phase0 >> 32)               # the carried phase does not grow


def test_arb_python_helpers_are_host_only():
    step = nsh.arb_step(160 / 147, 32)
    assert step == ref_step(160 / 147, 32)
    assert nsh.arb_span(step, 32, 0, 147, M31) == ref_span(step, 32, 0, 147, M31)
    n_out, c, nxt = nsh.arb_span(step, 32, 0, 147, M31)
    assert n_out in (160, 161) and c == 147 and abs(32 * 2.0 ** 32 / step - 160 / 147) < 1e-9

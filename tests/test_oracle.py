"""CPU: pin the oracle (oracle/nsh_oracle.c) against the golden fixtures and the
reference's own test vectors before anything is checked against it."""
import hashlib
import json
import os

import numpy as np

from oracle import oracle as orc
from tests.conftest import GOLDEN


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def test_synth_matches_manifest_and_numpy():
    m = manifest()
    x = orc.synth(8)
    np.testing.assert_array_equal(x, np.array([complex(a, b) for a, b in m["synth_prefix"]], np.complex64))
    # values lie on the 24-bit grid in [-1, 1)
    y = orc.synth(1 << 16, first_index=12345)
    v = np.concatenate([y.real, y.imag]).astype(np.float64)
    assert v.min() >= -1.0 and v.max() < 1.0
    assert np.all((v + 1.0) * 8388608.0 == np.round((v + 1.0) * 8388608.0))


def test_synth_segments_concatenate():
    a = orc.synth(1000)
    b = orc.synth(500, first_index=1000)
    np.testing.assert_array_equal(np.concatenate([a, b]), orc.synth(1500))


def test_fir_oracle_vs_lfilter(golden):
    g = golden("fir127.npz")
    y = orc.fir_ccf(g["x"], g["taps"])
    ok, err, scale = orc.tol_ok(y, g["y"])
    assert ok, (err, scale)
    assert err <= 1e-7 * scale  # double accumulation: agrees with lfilter to fp32 rounding


def test_fir_oracle_history_across_calls(golden):
    g = golden("fir127.npz")
    _, hist = orc.fir_ccf(g["x"], g["taps"], return_hist=True)
    y2 = orc.fir_ccf(g["x_next"], g["taps"], hist=hist)
    ok, err, scale = orc.tol_ok(y2, g["y_next"])
    assert ok, (err, scale)


def test_fir_oracle_decim(golden):
    g = golden("fir127_decim2.npz")
    y = orc.fir_ccf(g["x"], g["taps"], decim=2)
    ok, err, scale = orc.tol_ok(y, g["y"])
    assert ok, (err, scale)
    z = g["x"]
    for _ in range(4):
        z = orc.fir_ccf(z, g["taps"], decim=2)
    ok, err, scale = orc.tol_ok(z, g["y_chain4"])
    assert ok, (err, scale)


def test_fir_oracle_chunking_invariant():
    h = np.linspace(-0.3, 0.5, 37).astype(np.float32)
    x = orc.synth(3000)
    y_all = orc.fir_ccf(x, h)
    hist = np.zeros(36, np.complex64)
    parts = []
    for a, b in [(0, 1), (1, 40), (40, 41), (41, 1000), (1000, 3000)]:
        yp, hist = orc.fir_ccf(x[a:b], h, hist=hist, return_hist=True)
        parts.append(yp)
    np.testing.assert_array_equal(np.concatenate(parts), y_all)


def test_mulchain_oracle(golden):
    g = golden("mulchain4.npz")
    y = orc.mul_const_chain_cc(g["x"], list(g["k"]))
    np.testing.assert_array_equal(y, g["y"])  # per-stage fp32 products: bit-exact


def test_fft_oracle(golden):
    g = golden("fft1024.npz")
    ok, err, scale = orc.tol_ok(orc.fft1024(g["x"]), g["X"])
    assert ok, (err, scale)
    ok, err, scale = orc.tol_ok(orc.fft1024(g["x"], inverse=True), g["Xi"])
    assert ok, (err, scale)
    ok, err, scale = orc.tol_ok(orc.channelizer1024(g["x"], g["w"]), g["y_chan"])
    assert ok, (err, scale)


def test_reference_vectors_identity():
    """BlockFanout / BasicBlockGrouping (k = 1.0) and CudaCopy are exact identities."""
    m = manifest()["reference_vectors"]
    n = 1_000_000
    fan = (2 * np.arange(n) + 1j * (2 * np.arange(n) + 1)).astype(np.complex64)
    assert hashlib.sha256(fan.tobytes()).hexdigest() == m["BlockFanout"]["sha256"]
    np.testing.assert_array_equal(orc.mul_const_cc(fan, 1.0 + 0.0j), fan)
    cuda = (np.arange(102_400) - 1j * np.arange(102_400)).astype(np.complex64)
    assert hashlib.sha256(cuda.tobytes()).hexdigest() == m["CudaCopy"]["sha256"]
    out = np.empty_like(cuda)
    orc._load().orc_copy(orc._p(cuda), orc._p(out), cuda.nbytes)
    np.testing.assert_array_equal(out, cuda)


def test_add_mul_cc_oracle():
    a, b = orc.synth(1000), orc.synth(1000, first_index=7777)
    np.testing.assert_allclose(orc.add_cc(a, b), a + b, rtol=0, atol=0)
    p = orc.mul_cc(a, b)
    np.testing.assert_allclose(p, (a.astype(np.complex128) * b).astype(np.complex64), rtol=1e-6, atol=1e-7)


# ---- what tests/test_gpu_fft.py and tests/test_gpu_stream_edges.py lean on -----------------------
def _rand_w(seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, 1024) + 1j * rng.uniform(-1, 1, 1024)).astype(np.complex64)


def test_fft_oracle_impulse_basis_is_the_dft_matrix():
    """Frame p = unit impulse at p: the forward output is exp(-2j pi p k / 1024), the inverse its
    conjugate. The oracle computes in double and rounds once to fp32, so each part is within half
    an ulp of a value in [0.5, 1] (2^-25) and each element within 2^-24 = 6e-8 (measured: 3.7e-8)."""
    eye = np.eye(1024, dtype=np.complex64)
    pk = (np.arange(1024)[:, None] * np.arange(1024)[None, :]) % 1024  # exact phase index
    dft = np.exp(-2j * np.pi * pk / 1024)
    for inverse, want in ((False, dft), (True, dft.conj())):
        got = orc.fft1024(eye.ravel(), inverse=inverse).reshape(1024, 1024)
        err = float(np.abs(got.astype(np.complex128) - want).max())
        assert err <= 2.0 ** -24, (inverse, err)


def test_channelizer_oracle_impulse_basis_is_the_circulant():
    """An impulse at p through fft -> w -> ifft is 1024 ifft(w) rotated by p (numpy, double)."""
    w = _rand_w(1)
    h = 1024 * np.fft.ifft(w.astype(np.complex128))
    idx = (np.arange(1024)[None, :] - np.arange(1024)[:, None]) % 1024  # row p, column n: h[n - p]
    want = h[idx]
    got = orc.channelizer1024(np.eye(1024, dtype=np.complex64).ravel(), w).reshape(1024, 1024)
    err = float(np.abs(got.astype(np.complex128) - want).max())
    assert err <= 2.0 ** -23 * float(np.abs(h).max()), err  # one fp32 rounding of the output


def test_fft_oracle_nonfinite_stays_in_its_frame():
    """One bad sample in frame 1 of 3: frames 0 and 2 keep their bits, every output of frame 1 is
    non-finite in at least one part, and NaN in both for a nan+nanj sample."""
    x = orc.synth(3 * 1024, 21)
    w = _rand_w(2)
    ops = (lambda v: orc.fft1024(v), lambda v: orc.fft1024(v, inverse=True), lambda v: orc.channelizer1024(v, w))
    nan, inf = float("nan"), float("inf")
    for bad in (complex(nan, nan), complex(inf, 0.0), complex(0.25, -inf), complex(nan, 0.5)):
        xb = x.copy()
        xb[1024 + 77] = bad
        for op in ops:
            y, yb = op(x), op(xb)
            for f in (0, 2):
                np.testing.assert_array_equal(yb[1024 * f:1024 * (f + 1)].view(np.uint32),
                                              y[1024 * f:1024 * (f + 1)].view(np.uint32))
            mid = yb[1024:2048]
            assert np.all(~np.isfinite(mid.real) | ~np.isfinite(mid.imag))
            if np.isnan(bad.real) and np.isnan(bad.imag):
                assert np.all(np.isnan(mid.real) & np.isnan(mid.imag))


def test_fft_oracle_power_of_two_scaling_is_exact():
    """fft(s x) == s fft(x) bit for bit for s = 2^-60, 2^60, 2^100 (nothing under- or overflows:
    samples are multiples of 2^-23 in [-1, 1), the growth is at most 1024 sqrt(2))."""
    x = orc.synth(5 * 1024, 22)
    w = _rand_w(3)
    ops = (lambda v: orc.fft1024(v), lambda v: orc.fft1024(v, inverse=True), lambda v: orc.channelizer1024(v, w))
    for e in (-60, 60, 100):
        s = np.float32(2.0 ** e)
        for op in ops:
            np.testing.assert_array_equal(op(x * s).view(np.uint32), (op(x) * s).view(np.uint32))


def test_synth_oracle_wraps_at_2_64():
    """g = 2 (first + i) mod 2^64: the oracle against the numpy splitmix64 of oracle/gen_golden.py on
    indices reduced in Python integers, at first_index values around 2^31, 2^32, 2^40 and the wrap."""
    from oracle import gen_golden as gg

    def restated(n, first, seed):
        g = np.array([(2 * (first + i // 2) + (i & 1)) % 2 ** 64 for i in range(2 * n)], dtype=np.uint64)
        with np.errstate(over="ignore"):
            z = gg.splitmix64(g ^ np.uint64(seed))
        u = (z >> np.uint64(40)).astype(np.int64).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
        return (u[0::2] + 1j * u[1::2]).astype(np.complex64)

    for first in (2 ** 31 - 3, 2 ** 32 - 3, 2 ** 40 + 1, 2 ** 63 - 2, 2 ** 64 - 5):
        np.testing.assert_array_equal(orc.synth(4097, first), restated(4097, first, orc.SEED))
    np.testing.assert_array_equal(orc.synth(4097, 2 ** 64 - 5, seed=0x1234567), restated(4097, 2 ** 64 - 5, 0x1234567))
    np.testing.assert_array_equal(orc.synth(8), gg.synth(8))
    assert orc.synth(2, 2 ** 63 - 1)[1] == orc.synth(1, 0)[0]  # 2 * 2^63 wraps to 0
    np.testing.assert_array_equal(orc.synth(100, 2 ** 63 + 5), orc.synth(100, 5))


# ---- what tests/test_gpu_fir_forms.py leans on ----------------------------------------------------
def test_fir_oracle_integer_class_is_exact():
    """Integer taps, samples and history in [-8, 8] at 4096 taps: every sum is an integer far below
    2^24, so the oracle (double accumulation, one rounding to fp32) equals an int64 convolution
    exactly -- outputs and hist_out, at decim 1 and 8. The bit-equality the GPU tests demand of the
    kernels on this data class rests on this."""
    L = 4096
    rng = np.random.default_rng(4096)
    h = rng.integers(-8, 9, L)
    h[0], h[-1] = 3, -5
    for D in (1, 8):
        n_out = 1027
        s = rng.integers(-8, 9, (2, L - 1 + n_out * D))  # history, then the input; real and imaginary rows
        z = (s[0] + 1j * s[1]).astype(np.complex64)
        y, hout = orc.fir_ccf(z[L - 1:], h.astype(np.float32), D, hist=z[: L - 1], return_hist=True)
        full = [np.convolve(part.astype(np.int64), h.astype(np.int64))[L - 1: L - 1 + n_out * D: D] for part in s]
        assert max(int(np.abs(f).max()) for f in full) < 2 ** 24
        np.testing.assert_array_equal(y.real.astype(np.int64), full[0])
        np.testing.assert_array_equal(y.imag.astype(np.int64), full[1])
        assert np.all(y.real == np.round(y.real)) and np.all(y.imag == np.round(y.imag))
        np.testing.assert_array_equal(hout, z[-(L - 1):])

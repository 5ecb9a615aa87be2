"""What tests/test_fft_xlat_abi.py and tests/test_gpu_fft_xlat.py share: the Python model of the plan's
geometry and phase increment, the float64 reference of nsh_fft_xlat_ccc, the header's bound, and a
numpy / scipy complex64 model of the kernel's chain (a good fp32 transform on the same frames)."""
import math
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
SIZES = [1024, 2048, 4096, 8192]
DECIMS = [1, 2, 4, 8, 16, 32, 64]


def rule(L):
    """The default size rule of the header: 1024 up to 256 taps, 2048 up to 512, 4096 up to 2048, 8192
    above."""
    return 1024 if L <= 256 else 2048 if L <= 512 else 4096 if L <= 2048 else 8192


def phase_inc(turns):
    """nsh_phase_inc: round(frac(t) 2^64) mod 2^64, ties to even, exactly."""
    f = math.fmod(turns, 1.0)
    u = round(Fraction(abs(f)) * (1 << 64)) & M64
    return (-u if f < 0 else u) & M64


def geometry(L, D, fft_size=0):
    """(N, O, V) of a plan."""
    N = fft_size or rule(L)
    O = -(-(L - 1) // D) * D
    return N, O, N - O


def turns(first, lo, hi, inc):
    """phase(first + n) for n in [lo, hi) as float64 turns in [-0.5, 0.5): uint64 wrap-around, then the
    signed value over 2^64."""
    n = np.arange(lo, hi, dtype=np.int64).astype(np.uint64) + np.uint64(first & M64)
    with np.errstate(over="ignore"):
        p = n * np.uint64(inc)
    return p.view(np.int64).astype(np.float64) / 2.0 ** 64


def stream_of(x, hist, H):
    """hist_in ++ in as complex128 (zeros without a history)."""
    h0 = np.zeros(H, np.complex128) if hist is None else np.asarray(hist, np.complex64).astype(np.complex128)
    assert h0.size == H
    return np.concatenate([h0, np.asarray(x, np.complex64).astype(np.complex128)])


def ref64(x, h, D, inc, first=0, hist=None):
    """y[m] = sum_k h[k] x[mD-k] exp(+j 2 pi phase(first + mD - k)) in float64, for the len(x) // D
    outputs of one call: every stream sample is rotated by its own phase, then convolved."""
    import scipy.signal as ss

    h = np.asarray(h, np.complex64).astype(np.complex128)
    H = len(h) - 1
    n_out = len(x) // D
    s = stream_of(x[:n_out * D], hist, H)
    s = s * np.exp(2j * np.pi * turns(first, -H, n_out * D, inc))
    full = ss.fftconvolve(s, h) if len(h) > 32 else np.convolve(s, h)
    return full[H:H + n_out * D:D]


def brute64(x, h, D, inc, first=0, hist=None):
    """The same sum, term by term with Python integers for the phase."""
    H = len(h) - 1
    s = stream_of(x, hist, H)
    y = np.zeros(len(x) // D, np.complex128)
    for m in range(len(y)):
        acc = 0j
        for k in range(len(h)):
            p = ((first + m * D - k) * inc) & M64
            acc += complex(h[k]) * s[H + m * D - k] * np.exp(2j * np.pi * (p / 2.0 ** 64))
        y[m] = acc
    return y


def windows(x, hist, L, D, N):
    """The frames' windows of one call as rows (complex128): x[fV-O, fV-O+N), history in [-(L-1), 0),
    zeros elsewhere."""
    _, O, V = geometry(L, D, N)
    n_out = len(x) // D
    nf = -(-n_out // (V // D))
    s = np.concatenate([np.zeros(O - (L - 1)), stream_of(x[:n_out * D], hist, L - 1), np.zeros(nf * V + N)])
    return np.stack([s[f * V:f * V + N] for f in range(nf)])


def bound(x, h, D, N, y_ref, hist=None):
    """The header's bound for every output of one call."""
    L = len(h)
    _, O, V = geometry(L, D, N)
    wmax = np.abs(windows(x, hist, L, D, N)).max(axis=1)
    return 1e-5 * np.abs(y_ref) + 1e-6 * np.repeat(wmax, V // D)[:len(y_ref)] * np.abs(np.asarray(h, np.complex128)).sum()


def worst(y, y_ref, b):
    e = np.abs(np.asarray(y).astype(np.complex128) - y_ref)
    assert np.all(e[b == 0] == 0)
    return float(np.max(e[b > 0] / b[b > 0])) if np.any(b > 0) else 0.0


def model_c64(x, h, D, N, inc, first=0, hist=None):
    """The kernel's chain in complex64 with scipy.fft: FFT of N -> times Hs (band-pass taps formed and
    transformed in double, rounded once) -> fold to N/D bins -> inverse FFT of N/D -> drop O/D ->
    rotate (phasor in float32)."""
    import scipy.fft as sf

    L = len(h)
    _, O, V = geometry(L, D, N)
    n_out = len(x) // D
    g = np.asarray(h, np.complex64).astype(np.complex128) * np.exp(-2j * np.pi * turns(0, 0, L, inc))
    Hs = (np.fft.fft(g, N) / N).astype(np.complex64)
    w = windows(x, hist, L, D, N).astype(np.complex64)
    Y = sf.fft(w, axis=1) * Hs[None, :]
    Z = Y.reshape(len(w), D, N // D).sum(axis=1, dtype=np.complex64)
    z = sf.ifft(Z, axis=1, norm="forward")
    assert z.dtype == np.complex64
    y = z[:, O // D:].ravel()[:n_out]
    rot = np.exp(2j * np.pi * turns(first, 0, n_out * D, inc)[::D]).astype(np.complex64)
    return y * rot

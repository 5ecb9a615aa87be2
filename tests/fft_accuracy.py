"""What tests/test_gpu_fft_accuracy.py and tests/test_gpu_pfft_accuracy.py judge the FFT kernels by: the rms error of a whole call and of
its worst position, held to a small factor of the same figures of a numpy / scipy complex64 model of
the same chain on the same frames.

E = y - r (r: the float64 reference) is laid out as frames x positions, s is the rms of |r| over the
whole call:
    whole = rms(E) / s
    worst = max over positions p of (rms over frames of E[:, p]) / s
A position is an output bin of an FFT, or an output's place in its overlap-save frame: an error
that sits in one twiddle, one table entry or one lane stays at its positions in every frame, so it
shows in `worst` long before it moves `whole` or any max-norm bound.

The factors. Two independent correct fp32 transforms (a radix-2 complex64 FFT in numpy against
scipy.fft, N = 16 .. 8192, and the overlap-save chain built from either) differ by at most 1.02 in
whole and 1.11 in worst; the smallest defects tried (table angles formed in fp32; one table entry
times 1 + 1e-6) give at least 1.33 in whole or 2.4 in worst. WHOLE = 1.25 and WORST = 1.5 lie between.
Those figures were taken with at least 64 frames and at least 2^16 outputs a call, which gate()
asserts: with fewer, the model's own figures scatter by more than the margin."""
import math

import numpy as np

WHOLE, WORST = 1.25, 1.5
MIN_FRAMES, MIN_OUTPUTS = 64, 1 << 16


def frames_for(positions, at_least=MIN_FRAMES):
    """The smallest frame count, at least `at_least`, that meets both of gate()'s conditions."""
    return max(at_least, MIN_FRAMES, -(-MIN_OUTPUTS // positions))


def stats(y, r, frames):
    """(whole, worst) of y against r, both frames x positions flattened; in float64."""
    y = np.asarray(y).astype(np.complex128).reshape(frames, -1)
    r = np.asarray(r).astype(np.complex128).reshape(frames, -1)
    assert y.shape == r.shape
    s = math.sqrt(float(np.mean(np.abs(r) ** 2)))
    assert s > 0
    e2 = np.abs(y - r) ** 2
    return math.sqrt(float(e2.mean())) / s, math.sqrt(float(e2.mean(axis=0).max())) / s


def gate(name, y, model, r, frames, whole=WHOLE, worst=WORST):
    """Print y's and the model's (whole, worst) against r and assert y's within `whole` and `worst` times
    the model's (the FFT family's WHOLE and WORST unless given: tests/fir_accuracy.py passes its own).
    Returns the six figures (kernel whole, model whole, ratio, the same for worst)."""
    positions = np.asarray(r).size // frames
    assert frames >= MIN_FRAMES and frames * positions >= MIN_OUTPUTS, (name, frames, positions)
    wk, pk = stats(y, r, frames)
    wm, pm = stats(model, r, frames)
    print("RATIO accuracy whole kernel %.3g model %.3g ratio %.3f worst kernel %.3g model %.3g ratio %.3f %s"
          % (wk, wm, wk / wm, pk, pm, pk / pm, name))
    failed = []
    if not wk <= whole * wm:
        failed.append("whole %.3g > %.2f x %.3g" % (wk, whole, wm))
    if not pk <= worst * pm:
        failed.append("worst position %.3g > %.2f x %.3g" % (pk, worst, pm))
    assert not failed, "%s: %s" % (name, "; ".join(failed))
    return wk, wm, wk / wm, pk, pm, pk / pm


# ---- a second correct fp32 transform and its tables, for the CPU tests that prove the gate discriminates ----
def table_exact(N):
    """W_N^k, k < N/2, formed in double and rounded once."""
    return np.exp(-2j * np.pi * np.arange(N // 2) / N).astype(np.complex64)


def table_one_entry_off(N):
    """... with one entry that only the last stage reads (an odd k) times 1 + 1e-6."""
    t = table_exact(N)
    k = N // 8 + 1
    t[k] = np.complex64(np.complex128(t[k]) * (1.0 + 1e-6))
    return t


def table_fp32_angles(N):
    """... with the angle -2 pi k / N formed in fp32."""
    a = np.float32(-2.0 * np.pi) * np.arange(N // 2, dtype=np.float32) / np.float32(N)
    assert a.dtype == np.float32
    return (np.cos(a.astype(np.float64)) + 1j * np.sin(a.astype(np.float64))).astype(np.complex64)


def fft_r2(x, table, inverse=False):
    """Radix-2 decimation-in-time FFT of the rows of x in complex64 (unnormalised both ways); table:
    W_N^k for k < N/2."""
    F, N = x.shape
    assert table.dtype == np.complex64 and table.size == N // 2
    w = np.conj(table) if inverse else table
    nb = N.bit_length() - 1
    rev = np.zeros(N, np.int64)
    for b in range(nb):
        rev |= ((np.arange(N) >> b) & 1) << (nb - 1 - b)
    a = np.ascontiguousarray(x, np.complex64)[:, rev]
    m = 1
    while m < N:
        a = a.reshape(F, N // (2 * m), 2, m)
        t = a[:, :, 1, :] * w[::N // (2 * m)][None, None, :]
        a = np.stack([a[:, :, 0, :] + t, a[:, :, 0, :] - t], axis=2)
        assert a.dtype == np.complex64
        m *= 2
    return a.reshape(F, N)

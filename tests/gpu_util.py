"""The device and data helpers the GPU tests share: one copy of each. A plain module, no fixtures: the
module-scoped `stream` fixtures stay with their tests. The float64 references live in
tests/fir_accuracy.py (time domain) and tests/fft_xlat_ref.py / tests/fft_accuracy.py (FFT)."""
import ctypes

import numpy as np

from newsched_amd import nsh
from oracle import oracle as orc


# ---- host <-> device ------------------------------------------------------------------------------------
def dev(torch, a):
    """A C-ordered, writable copy of `a` on the device (a copy: torch warns about read-only arrays)."""
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- comparing ------------------------------------------------------------------------------------------
def bits(a, dtype=None):
    """The 32-bit words of `a` (taken as `dtype` where given), for bit-for-bit comparisons."""
    return np.ascontiguousarray(a, dtype).view(np.uint32)


def assert_tol(y, ref, what="", rel=1e-5):
    ok, err, scale = orc.tol_ok(y, ref, rel=rel)
    print(f"  {what}: max err {err:.3g} of scale {scale:.3g} ({err / scale if scale else 0:.2g})")
    assert ok, (what, err, scale)


def first_mismatch(y, ref):
    bad = np.nonzero(y != ref)[0]
    if bad.size == 0:
        return "equal"
    i = int(bad[0])
    return "%d of %d differ, first at %d (got %r, want %r), last at %d, differences %r" % (
        bad.size, y.size, i, y[i], ref[i], int(bad[-1]), (y[bad[:8]] - ref[bad[:8]]).tolist())


# ---- data -----------------------------------------------------------------------------------------------
def uniform(n, seed):
    r = np.random.default_rng(seed)
    return (r.uniform(-1, 1, n) + 1j * r.uniform(-1, 1, n)).astype(np.complex64)


def hann(N):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)


def rand_window(N, seed=5):
    return np.random.default_rng(seed + N).uniform(-1, 1, N).astype(np.float32)


def int_taps(rng, L):
    h = rng.integers(-8, 9, L).astype(np.float32)
    for i, v in ((0, 3.0), (L - 1, -5.0)):  # both end taps count
        if h[i] == 0:
            h[i] = v
    return h


def int_signal(rng, n):
    return (rng.integers(-8, 9, n) + 1j * rng.integers(-8, 9, n)).astype(np.complex64)


def windowed_sinc(L, width, gain=1.0):
    """A Hamming window (rectangular for L <= 2) times sinc(0.8 k / width), the taps summing to `gain`."""
    t = np.hamming(L) if L > 2 else np.ones(L)
    k = np.arange(L) - (L - 1) / 2.0
    t = t * np.sinc(0.8 * k / width)
    return (gain * t / t.sum()).astype(np.float32)


# ---- the C-ABI tests ------------------------------------------------------------------------------------
ONE, TWO = ctypes.c_void_p(16), ctypes.c_void_p(32)


def refused(rc, text):
    assert rc != 0
    msg = nsh.lib().nsh_last_error()
    assert text in msg, msg

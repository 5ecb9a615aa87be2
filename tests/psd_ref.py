"""What tests/test_gpu_psd.py and tests/test_gpu_psd_walk.py share: psd_vcf's float64 reference and
per-bin bound, the test signal, the segment arithmetic, and the runners (the PSD plan between guard
words; the project's own FFT of the same frames). The bound and the signal are described in
tests/test_gpu_psd.py's docstring."""
import functools

import numpy as np

from newsched_amd import nsh
from tests.gpu_util import dev, host

GUARD = np.float32(-12345.5)
P_DEFAULT = 32  # the most frames of a segment; the GPU tests read it from a plan (segment())


def frames_per_team(N):
    return max(1024 // N, 1)


@functools.lru_cache(maxsize=None)
def segment(N):
    """P, the most frames of a segment at size N: K <= P runs one segment (one launch), K > P is cut
    into ceil(K / P) segments of balanced_segment(K, P) frames. Read from a plan whose K is a multiple
    of every candidate P."""
    p = nsh.PsdPlan(N, 65536)
    P = p.segment
    p.close()
    return P


def balanced_segment(K, P):
    nseg = -(-K // P)
    return -(-K // nseg)


@functools.lru_cache(maxsize=None)
def signal(N, nframes, seed=1):
    """Unit complex Gaussian noise plus the two tones (tests/test_gpu_psd.py's docstring); read-only, shared."""
    rng = np.random.default_rng(1000 * seed + N)
    n = np.arange(N * nframes, dtype=np.float64)
    a = 100.0 * np.sqrt(0.375 * N) / (N / 2)
    x = (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size)) / np.sqrt(2.0)
    x += a * np.exp(2j * np.pi * (N // 8) * n / N) + a * np.exp(2j * np.pi * (N // 3 + 0.37) * n / N)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def reference(x, N, K, w=None, scale=1.0, shift=False):
    """(ref, B) of whole vectors of x in float64, each (nvec, N)."""
    f = np.asarray(x, np.complex64).astype(np.complex128).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32).astype(np.float64)[None, :]
    X = np.abs(np.fft.fft(f, axis=1))
    d = 1e-5 * X.max(axis=1, keepdims=True)
    lin = (2 * X * d + d * d).reshape(-1, K, N).sum(axis=1)
    p = (X * X).reshape(-1, K, N).sum(axis=1)
    g = (K + 2) * 2.0 ** -24
    ref, B = scale * p, scale * (lin + g * p)
    if shift:
        ref, B = np.fft.fftshift(ref, axes=1), np.fft.fftshift(B, axes=1)
    return ref, B


def run(torch, plan, x, nvec=None, in_off=0, out_off=0, tail=64):
    """plan over x; the input ends exactly at the end of its allocation (in_off samples of slack in
    front), the output has out_off guard floats in front and `tail` behind, all checked."""
    N, K = plan.fft_size, plan.navg
    x = np.asarray(x, np.complex64)
    if nvec is None:
        nvec = x.size // (N * K)
    assert x.size == nvec * N * K
    dx = torch.zeros(in_off + x.size, dtype=torch.complex64, device="cuda")
    dx[in_off:] = dev(torch, x)
    dy = torch.full((out_off + nvec * N + tail,), float(GUARD), dtype=torch.float32, device="cuda")
    plan(dx.data_ptr() + 8 * in_off, dy.data_ptr() + 4 * out_off, nvec)
    y = host(dy)
    assert np.all(y[:out_off] == GUARD) and np.all(y[out_off + nvec * N:] == GUARD), (plan.kernel, nvec, in_off, out_off)
    return y[out_off:out_off + nvec * N].reshape(nvec, N)


def fft_of(torch, x, N, w=None, shift=False):
    p = nsh.FftPlan(N, False, w, shift)
    dx = dev(torch, x)
    dy = torch.empty_like(dx)
    nsh.fft_c2c(p, dx, dy, x.size // N)
    y = host(dy)
    p.close()
    return y

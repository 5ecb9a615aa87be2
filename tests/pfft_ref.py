"""What tests/test_gpu_pfft.py, tests/test_gpu_pfft_taps.py and tests/test_gpu_pfft_accuracy.py share:
the two forms of the 16-phase kernel as a fixture, BASELINE config C5 and the random-tap chains, the
composite filter and its geometry, the float64 reference, the oracle's stage-by-stage chain, the
complex64 model of the kernel's algorithm, the launch shape and the runner of one
nsh_fir_cascade_ccf call."""
import numpy as np
import pytest
import scipy.signal as ss

from oracle import oracle as orc

M = 512  # the transform length per phase
KERNEL16 = {"2": "k_fir_pfft2<16>", "1": "k_fir_pfft<16,1>"}


@pytest.fixture(autouse=True, params=["2", "1"], ids=["form2", "form1"])
def pfft_form(request, monkeypatch):
    monkeypatch.setenv("NSH_PFFT_FORM", request.param)
    return request.param


def _firwin(n, cutoff):
    return np.asarray(__import__("scipy.signal", fromlist=["firwin"]).firwin(n, cutoff), np.float32)


C5 = [(_firwin(127, 0.45), 2)] * 4


def heq_of(stages):
    """The composite filter in float64 from the fp32 stage taps."""
    h = np.ones(1)
    dacc = 1
    for t, d in stages:
        u = np.zeros((t.size - 1) * dacc + 1)
        u[::dacc] = np.asarray(t, np.float64)
        h = np.convolve(h, u)
        dacc *= d
    return h


def heq_l1(stages):
    """sum |heq| of the composite filter (double)."""
    return float(np.abs(heq_of(stages)).sum())


def taps_u(n, seed, scale=1.0):
    """n taps, magnitudes uniform in [0.5, 1] * scale (a power of two), random signs."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * scale).astype(np.float32)


def geometry(stages):
    heq = heq_of(stages)
    D = int(np.prod([d for _, d in stages]))
    Q = (heq.size - 1 + D - 1) // D
    return heq, D, Q, M - Q


def ref64(x, heq, D, n_out, hist=None):
    """y[m] = sum_n heq[n] s[m D - n] in float64, s = x preceded by hist (zeros before it)."""
    s = np.asarray(x, np.complex128)
    off = 0
    if hist is not None and len(hist):
        s = np.concatenate([np.asarray(hist, np.complex128), s])
        off = len(hist)
    full = ss.oaconvolve(s, np.asarray(heq, np.float64)) if s.size > 4 * heq.size else np.convolve(s, heq)
    return full[off:off + D * n_out:D][:n_out]


def ref_chain(x, stages):
    y = x
    for h, d in stages:
        y = orc.fir_ccf(y, h, d)
    return y


def image_table(stages, heq=None):
    """F_p = FFT_512(g_p) / 512, g_p[q'] = heq[D q' - p], formed in double and rounded once: [D][512].
    heq: the chain's composite filter unless given (the CPU tests plant their defects in it)."""
    heq0, D, Q, _ = geometry(stages)
    heq = heq0 if heq is None else np.asarray(heq, np.float64)
    assert heq.size == heq0.size
    g = np.zeros((D, M))
    for p in range(D):
        n = D * np.arange(Q + 1) - p
        ok = (n >= 0) & (n < heq.size)
        g[p, np.flatnonzero(ok)] = heq[n[ok]]
    return (np.fft.fft(g, axis=1) / M).astype(np.complex64)


def _fft512(a):
    return __import__("scipy.fft", fromlist=["fft"]).fft(a, axis=-1)


def _ifft512(a):
    return __import__("scipy.fft", fromlist=["ifft"]).ifft(a, axis=-1, norm="forward")


def pfft_model(x, hist, stages, n_out, fwd=_fft512, inv=_ifft512, F=None, order=None):
    """The header's algorithm in complex64 on the same fp32 inputs: the windows u[t] = s[P (f V - Q) + t]
    (s: hist, then x; zeros before and after), each split into P phase sequences of 512, their forward
    transforms times F_p (image_table unless given), summed over p in `order` (ascending unless given),
    the unnormalised inverse, rows q >= Q, n_out outputs. fwd and inv take and return rows of 512 in
    complex64 (scipy.fft unless given)."""
    heq, P, Q, V = geometry(stages)
    F = image_table(stages) if F is None else F
    order = list(range(P)) if order is None else list(order)
    assert F.dtype == np.complex64 and F.shape == (P, M) and sorted(order) == list(range(P))
    nf = (n_out + V - 1) // V
    hist = np.zeros(0, np.complex64) if hist is None else np.asarray(hist, np.complex64)
    assert hist.size <= P * Q and x.size == P * n_out
    s = np.concatenate([np.zeros(P * Q - hist.size, np.complex64), hist, np.asarray(x, np.complex64),
                        np.zeros(P * (nf * V - n_out), np.complex64)])
    assert s.size == P * (nf * V + Q)
    y = np.empty((nf, V), np.complex64)
    step = 256  # frames at a time: 32 MiB of windows at P = 16
    for f0 in range(0, nf, step):
        f1 = min(nf, f0 + step)
        # u[f, p, n] = s[P (f V + n) + p] (s starts at window 0's first sample)
        u = np.stack([s[P * f * V:P * (f * V + M)].reshape(M, P).T for f in range(f0, f1)])
        U = fwd(np.ascontiguousarray(u).reshape(-1, M)).reshape(f1 - f0, P, M)
        assert U.dtype == np.complex64
        Z = U[:, order[0], :] * F[order[0]][None, :]
        for p in order[1:]:
            Z = Z + U[:, p, :] * F[p][None, :]
        assert Z.dtype == np.complex64
        c = inv(Z)
        assert c.dtype == np.complex64
        y[f0:f1] = c[:, Q:]
    return y.ravel()[:n_out]


def by_workgroup(a, fpw, V):
    """The outputs of whole workgroups of fpw frames as (workgroups, fpw V): position = (k, q), k the
    frame's index inside its workgroup -- a workgroup's frames are consecutive. Returns the array and
    its row count (the frames per position)."""
    a = np.asarray(a)
    assert a.size % (fpw * V) == 0
    return a.reshape(-1, fpw * V), a.size // (fpw * V)


def launch_shape(n_out, V, D, n_cu):
    """(frames, frames per workgroup, workgroups) as nsh_fir_cascade_ccf launches them."""
    nf = (n_out + V - 1) // V
    wg = min(nf, n_cu * (1 if D == 16 else 2))
    fpw = (nf + wg - 1) // wg
    return nf, fpw, (nf + fpw - 1) // fpw


def many_frames_n_out(V, D, n_cu):
    return (3 * n_cu if D == 16 else 2 * 2 * n_cu) * V + 1


def n_cu_of(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _single(L, D, seed=None):
    return [(taps_u(L, 1000 + L if seed is None else seed), D)]


# group A of tests/test_gpu_pfft_taps.py: the frame shapes
CHAINS_A = {
    "d16-L1": _single(1, 16), "d16-L2": _single(2, 16),
    "d16-L17-q1": _single(17, 16), "d16-L33-q2": _single(33, 16),
    "d16-L641-r0": _single(641, 16), "d16-L642-r1": _single(642, 16), "d16-L656-r15": _single(656, 16),
    "d16-L4070-q255": _single(4070, 16), "d16-L4082-q256": _single(4082, 16), "d16-L4097-q256": _single(4097, 16),
    "d8-L2": _single(2, 8), "d8-L2042-q256": _single(2042, 8), "d8-L2049-q256": _single(2049, 8),
    "d16-2x8": [(taps_u(2, 21), 2), (taps_u(1000, 22), 8)],
    "d16-4x2x2": [(taps_u(4, 31), 4), (taps_u(2, 32), 2), (taps_u(300, 33), 2)],
    "d8-2x4": [(taps_u(2, 41), 2), (taps_u(700, 42), 4)],
}
# group B: many frames per workgroup
CHAINS_B = {
    # the longest filters (V = 256); taps * 2^-12 so that |x| sum|heq| stays inside fp32 at 2^125
    "d16-L4097": [(taps_u(4097, 5097, 2.0 ** -12), 16)],
    "d8-L2049": [(taps_u(2049, 3049, 2.0 ** -11), 8)],
    "c5": C5,
    # Q = 192: V - Q = 128 rows of each frame lie in no other frame's window
    "d16-L3073": [(taps_u(3073, 4073), 16)],
    "d16-2x8-q192": [(taps_u(2, 51), 2), (taps_u(1536, 52), 8)],
    "d8-L1537": [(taps_u(1537, 2537), 8)],
    "d8-2x4-q192": [(taps_u(2, 61), 2), (taps_u(768, 62), 4)],
}


def run_pfft(torch, plan, x, n_out, hist=None, want_hist=True):
    assert x.size == plan.decim * n_out
    dx = torch.from_numpy(np.ascontiguousarray(x, np.complex64)).cuda() if x.size else \
        torch.zeros(1, dtype=torch.complex64, device="cuda")
    dh = torch.from_numpy(np.ascontiguousarray(hist, np.complex64)).cuda() if hist is not None else None
    dho = torch.full((plan.hist_len,), complex(9.0, 9.0), dtype=torch.complex64, device="cuda") if want_hist else None
    dy = torch.full((max(n_out, 1),), complex(7.0, 7.0), dtype=torch.complex64, device="cuda")
    plan(dx, dh, dho, dy, n_out)
    torch.cuda.synchronize()
    return dy.cpu().numpy()[:n_out], (dho.cpu().numpy() if want_hist else None)

"""The accuracy gate of the FFT family: every form of nsh_fft_c2c (k_fft<N>, k_fft1024),
nsh_fft1024_c2c, nsh_channelizer1024, nsh_fft_filter_ccc and nsh_fft_xlat_ccc (k_fft_xlat<N, D>) held
to the error of a good fp32 implementation of the same chain, over the whole call and at its worst
position (tests/fft_accuracy.py: whole <= 1.25 x model, worst <= 1.5 x model).

The other tests of these kernels assert the contract's max-norm bounds, which the kernels meet with
one to two orders of magnitude to spare: a twiddle constant with six digits, one table entry off in
its low bits, tables formed in float, a fold that sums in a worse order or a phasor that loses bits
all pass them. They do not pass here.

Models (complex64, on the same frames) and references (float64 on the same fp32 inputs):
  fft_vcc          scipy.fft.fft / ifft(norm="forward") of the frames, after an fp32 multiply by the
                   window and with the header's shift (output halves swapped forward, input halves
                   swapped inverse); numpy.fft on complex128.
  channelizer1024  scipy.fft.fft -> complex64 multiply by w -> scipy.fft.ifft(norm="forward");
                   the same in complex128.
  overlap-save     fft_xlat_ref.model_c64 and ref64; fft_filter_ccc is D = 1, inc = 0.

The CPU tests (not marked gpu) prove that the gate discriminates: a radix-2 complex64 FFT
(fft_accuracy.fft_r2), given its twiddle table, passes against the scipy model with the correctly rounded table, fails
the worst-position gate with one entry times 1 + 1e-6 and fails both gates with angles formed in fp32;
the overlap-save chain built from it behaves the same with the table of its N/D-point inverse.

Frames per call: at least 64 (512 for an overlap-save form with fewer than 1024 outputs a frame) and
as many as bring the call to 2^16 outputs, the two conditions the factors were established under.

Measured on one MI355X (profiles/fft_accuracy_ratios.log; kernel, model, kernel / model; every case
passes, no kernel needed a change and no model an extension):
                                         whole                            worst position
  fft_vcc plain, 20 cases     6.1e-8..1.29e-7  6.6e-8..1.33e-7  0.93..1.00   6.6e-8..1.74e-7  7.7e-8..1.72e-7  0.85..1.01
  fft_vcc Hann + shift, 4     8.3e-8..1.17e-7  8.6e-8..1.23e-7  0.96         8.9e-8..1.66e-7  9.3e-8..1.58e-7  0.94..1.05
  nsh_fft1024_c2c, 2          1.08e-7..1.09e-7 1.14e-7          0.95         1.38e-7..1.40e-7 1.45e-7..1.48e-7 0.95
  nsh_channelizer1024         1.62e-7          1.68e-7          0.97         2.00e-7          2.16e-7          0.93
  fft_filter_ccc, 8           1.62e-7..1.95e-7 1.69e-7..1.97e-7 0.96..1.00   1.93e-7..2.64e-7 1.96e-7..2.55e-7 0.95..1.03
  xlat untuned, 28 forms      1.60e-7..2.19e-7 1.65e-7..2.21e-7 0.96..1.00   1.70e-7..2.61e-7 1.76e-7..2.57e-7 0.95..1.05
  xlat at 0.1137, 28 forms    1.76e-7..2.37e-7 1.69e-7..2.27e-7 1.01..1.08   1.92e-7..2.98e-7 1.80e-7..2.55e-7 1.01..1.20
The tuned forms carry the header's rotation (two phasors from the top 32 phase bits and one rounded
product, nsh_fft_xlat_kernel.hpp) against the model's exactly rounded one; its cost on the CPU is 1.04 to
1.07 in whole and 1.03 to 1.14 in worst, and it fits inside the factors. With C1 of w16 shortened to
0.92388f (a scratch build) all 91 GPU cases here fail, with ratios of 2.3 to 4.5 in whole and 2.7 to 6.3 in worst, while
tests/test_gpu_fft_sizes.py stays green."""
import numpy as np
import pytest

from tests import fft_accuracy as acc
from tests import fft_xlat_ref as ref
from tests.fft_accuracy import fft_r2, table_exact, table_fp32_angles, table_one_entry_off
from tests.gpu_util import dev, hann, uniform

gpu = pytest.mark.gpu

FFT_SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
DIRS = pytest.mark.parametrize("inv", [False, True], ids=["fwd", "inv"])
FREQ = 0.1137
FIRST = 12345


# ---- the models and references of the plain transforms --------------------------------------------
def fft_model(x, N, inv, w=None, shift=False):
    """nsh_fft_c2c's conventions in complex64 with scipy.fft."""
    import scipy.fft as sf

    f = np.ascontiguousarray(x, np.complex64).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32)[None, :]
    if inv:
        y = sf.ifft(np.fft.fftshift(f, axes=1) if shift else f, axis=1, norm="forward")
    else:
        y = sf.fft(f, axis=1)
        y = np.fft.fftshift(y, axes=1) if shift else y
    assert y.dtype == np.complex64
    return y.ravel()


def fft_ref(x, N, inv, w=None, shift=False):
    """... and in complex128 on the same fp32 inputs."""
    f = np.asarray(x, np.complex64).astype(np.complex128).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32).astype(np.float64)[None, :]
    if inv:
        return np.fft.ifft(np.fft.fftshift(f, axes=1) if shift else f, axis=1, norm="forward").ravel()
    y = np.fft.fft(f, axis=1)
    return (np.fft.fftshift(y, axes=1) if shift else y).ravel()


def chan_model(x, w):
    import scipy.fft as sf

    f = np.ascontiguousarray(x, np.complex64).reshape(-1, 1024)
    y = sf.ifft(sf.fft(f, axis=1) * np.asarray(w, np.complex64)[None, :], axis=1, norm="forward")
    assert y.dtype == np.complex64
    return y.ravel()


def chan_ref(x, w):
    f = np.asarray(x, np.complex64).astype(np.complex128).reshape(-1, 1024)
    w = np.asarray(w, np.complex64).astype(np.complex128)
    return np.fft.ifft(np.fft.fft(f, axis=1) * w[None, :], axis=1, norm="forward").ravel()


# ---- CPU: the gate tells a correct fp32 transform from a subtly wrong one -------------------------
_cpu = {}


def cpu_case(N, inv):
    """Frames, scipy model and float64 reference of the CPU transform tests, once per (N, direction)."""
    if (N, inv) not in _cpu:
        F = acc.frames_for(N)
        x = uniform(F * N, 300 + N)
        v = (F, x, fft_model(x, N, inv), fft_ref(x, N, inv))
        for a in v[1:]:
            a.setflags(write=False)
        _cpu[(N, inv)] = v
    return _cpu[(N, inv)]


cpu_sizes = pytest.mark.parametrize("N", [64, 1024, 8192])


@cpu_sizes
@DIRS
def test_cpu_correctly_rounded_table_passes(N, inv):
    F, x, model, r = cpu_case(N, inv)
    y = fft_r2(x.reshape(F, N), table_exact(N), inv).ravel()
    acc.gate("radix-2 numpy N=%d %s, exact table" % (N, "inv" if inv else "fwd"), y, model, r, F)


@cpu_sizes
@DIRS
def test_cpu_one_table_entry_off_fails_the_worst_position_gate(N, inv):
    F, x, model, r = cpu_case(N, inv)
    y = fft_r2(x.reshape(F, N), table_one_entry_off(N), inv).ravel()
    with pytest.raises(AssertionError, match="worst position"):
        acc.gate("radix-2 numpy N=%d %s, one entry x (1 + 1e-6)" % (N, "inv" if inv else "fwd"), y, model, r, F)


@cpu_sizes
@DIRS
def test_cpu_fp32_angles_fail_both_gates(N, inv):
    F, x, model, r = cpu_case(N, inv)
    y = fft_r2(x.reshape(F, N), table_fp32_angles(N), inv).ravel()
    with pytest.raises(AssertionError, match="whole .*; worst position"):
        acc.gate("radix-2 numpy N=%d %s, fp32 angles" % (N, "inv" if inv else "fwd"), y, model, r, F)


def chain_r2(x, h, D, N, inc, first, hist, inverse_table):
    """fft_xlat_ref.model_c64's chain with fft_r2 in place of scipy.fft: forward N (exact table), times
    Hs, fold, inverse N/D with the given table, drop O/D, rotate."""
    L = len(h)
    _, O, V = ref.geometry(L, D, N)
    n_out = len(x) // D
    g = np.asarray(h, np.complex64).astype(np.complex128) * np.exp(-2j * np.pi * ref.turns(0, 0, L, inc))
    Hs = (np.fft.fft(g, N) / N).astype(np.complex64)
    w = ref.windows(x, hist, L, D, N).astype(np.complex64)
    Y = fft_r2(w, table_exact(N)) * Hs[None, :]
    Z = Y.reshape(len(w), D, N // D).sum(axis=1, dtype=np.complex64)
    z = fft_r2(Z, inverse_table, inverse=True)
    y = z[:, O // D:].ravel()[:n_out]
    rot = np.exp(2j * np.pi * ref.turns(first, 0, n_out * D, inc)[::D]).astype(np.complex64)
    return y * rot


_ols = {}


def ols_case():
    """(N, D) = (1024, 8), 128 random taps, tuned: inputs, model and reference, once."""
    if not _ols:
        N, D, L = 1024, 8, 128
        _, O, V = ref.geometry(L, D, N)
        F = acc.frames_for(V // D, 512)
        h = uniform(L, 1000 + L) * np.float32(0.05)
        x, hist = uniform(F * V, 77), uniform(L - 1, 7)
        inc = ref.phase_inc(FREQ)
        model = ref.model_c64(x, h, D, N, inc, FIRST, hist)
        r = ref.ref64(x, h, D, inc, FIRST, hist)
        _ols.update(N=N, D=D, F=F, h=h, x=x, hist=hist, inc=inc, model=model, r=r)
    return _ols


def test_cpu_overlap_save_chain_passes():
    c = ols_case()
    y = chain_r2(c["x"], c["h"], c["D"], c["N"], c["inc"], FIRST, c["hist"], table_exact(c["N"] // c["D"]))
    acc.gate("radix-2 overlap-save (1024, 8), exact tables", y, c["model"], c["r"], c["F"])


def test_cpu_overlap_save_chain_one_inverse_entry_off_fails_the_worst_position_gate():
    c = ols_case()
    y = chain_r2(c["x"], c["h"], c["D"], c["N"], c["inc"], FIRST, c["hist"], table_one_entry_off(c["N"] // c["D"]))
    with pytest.raises(AssertionError, match="worst position"):
        acc.gate("radix-2 overlap-save (1024, 8), one inverse entry x (1 + 1e-6)", y, c["model"], c["r"], c["F"])


def test_cpu_gate_refuses_too_few_frames_or_outputs():
    r = uniform(63 * 2048, 1)
    with pytest.raises(AssertionError):
        acc.gate("63 frames", r, r, r, 63)
    r = uniform(64 * 512, 2)
    with pytest.raises(AssertionError):
        acc.gate("2^15 outputs", r, r, r, 64)


def run_fft(torch, plan, x):
    dx = dev(torch, x)
    dy = torch.empty_like(dx)
    plan(dx, dy, x.size // plan.fft_size)
    torch.cuda.synchronize()
    return dy.cpu().numpy()


@gpu
@pytest.mark.parametrize("N", FFT_SIZES)
@DIRS
def test_fft_vcc(torch_cuda, N, inv):
    """Plain plans at all ten sizes; 1024 runs k_fft1024."""
    from newsched_amd import nsh

    F = acc.frames_for(N)
    x = uniform(F * N, 400 + N)
    p = nsh.FftPlan(N, inv)
    y = run_fft(torch_cuda, p, x)
    acc.gate("fft_vcc %s N=%d %s" % (p.kernel, N, "inv" if inv else "fwd"), y, fft_model(x, N, inv), fft_ref(x, N, inv), F)
    p.close()


@gpu
@pytest.mark.parametrize("N", [64, 2048])  # several frames a wave (the LIN form) and a team of two waves
@DIRS
def test_fft_vcc_hann_window_and_shift(torch_cuda, N, inv):
    from newsched_amd import nsh

    F = acc.frames_for(N)
    x = uniform(F * N, 500 + N)
    w = hann(N)
    p = nsh.FftPlan(N, inv, w, shift=True)
    y = run_fft(torch_cuda, p, x)
    acc.gate("fft_vcc hann+shift %s N=%d %s" % (p.kernel, N, "inv" if inv else "fwd"), y, fft_model(x, N, inv, w, True),
             fft_ref(x, N, inv, w, True), F)
    p.close()


@gpu
@DIRS
def test_fft1024(torch_cuda, inv):
    from newsched_amd import nsh

    torch = torch_cuda
    F = 64
    x = uniform(F * 1024, 600)
    dx = dev(torch, x)
    dy = torch.empty_like(dx)
    nsh.fft1024(dx, dy, F, inverse=inv)
    torch.cuda.synchronize()
    acc.gate("nsh_fft1024_c2c k_fft1024 %s" % ("inv" if inv else "fwd"), dy.cpu().numpy(), fft_model(x, 1024, inv),
             fft_ref(x, 1024, inv), F)


@gpu
def test_channelizer1024(torch_cuda):
    from newsched_amd import nsh

    torch = torch_cuda
    F = 64
    x, w = uniform(F * 1024, 601), uniform(1024, 602)
    dx, dw = dev(torch, x), dev(torch, w)
    dy = torch.empty_like(dx)
    nsh.channelizer1024(dx, dy, dw, F)
    torch.cuda.synchronize()
    acc.gate("nsh_channelizer1024 k_chan1024 random w", dy.cpu().numpy(), chan_model(x, w), chan_ref(x, w), F)


# ---- GPU: the overlap-save filters -------------------------------------------------------------------
def random_taps(L):
    """Uniform complex taps times 0.05: they load every bin of Hs (a low-pass hides the stop band)."""
    return uniform(L, 1000 + L) * np.float32(0.05)


@gpu
@pytest.mark.parametrize("N", ref.SIZES)
@pytest.mark.parametrize("Lk", ["N/8+1", "N/2"])
def test_fft_filter_ccc(torch_cuda, N, Lk):
    from newsched_amd import nsh

    torch = torch_cuda
    L = N // 8 + 1 if Lk == "N/8+1" else N // 2
    h = random_taps(L)
    p = nsh.FftFilterPlan(h, N)
    V = p.valid
    F = acc.frames_for(V)
    x, hist = uniform(F * V, 700 + N + L), uniform(L - 1, 701)
    dx, dh = dev(torch, x), dev(torch, hist)
    dy, dho = torch.empty_like(dx), torch.empty_like(dh)
    p(dx, dh, dho, dy, x.size)
    torch.cuda.synchronize()
    acc.gate("fft_filter_ccc %s L=%d frames=%d" % (p.kernel, L, F), dy.cpu().numpy(), ref.model_c64(x, h, 1, N, 0, 0, hist),
             ref.ref64(x, h, 1, 0, 0, hist), F)
    p.close()


@gpu
@pytest.mark.parametrize("N", ref.SIZES)
@pytest.mark.parametrize("D", ref.DECIMS)
@pytest.mark.parametrize("freq", [0.0, FREQ], ids=["untuned", "tuned"])
def test_freq_xlating_fft_filter_ccc(torch_cuda, N, D, freq):
    """All 28 forms. Untuned (inc == 0) takes the branch without the rotation: forward, Hs, fold and
    the sub-team inverse alone. Tuned adds the band-pass taps and the rotation."""
    from newsched_amd import nsh

    torch = torch_cuda
    L = 128
    h = random_taps(L)
    p = nsh.FftXlatPlan(h, D, freq, fft_size=N)
    assert (p.phase_inc == 0) == (freq == 0.0)
    Vd = p.valid // D
    F = acc.frames_for(Vd, 512 if Vd < 1024 else 64)
    n_out = F * Vd
    x, hist = uniform(n_out * D, 800 + N + D), uniform(L - 1, 801)
    dx, dh = dev(torch, x), dev(torch, hist)
    dy = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    dho = torch.empty_like(dh)
    p(dx, dh, dho, dy, n_out, FIRST)
    torch.cuda.synchronize()
    acc.gate("freq_xlating_fft_filter_ccc %s freq=%g frames=%d" % (p.kernel, freq, F), dy.cpu().numpy(),
             ref.model_c64(x, h, D, N, p.phase_inc, FIRST, hist), ref.ref64(x, h, D, p.phase_inc, FIRST, hist), F)
    p.close()

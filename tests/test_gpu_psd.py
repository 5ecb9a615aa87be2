"""GPU: nsh_psd_cf (k_psd<N, LIN> and, past one segment, k_psd_sum): windowed FFT, |X|^2 and the sum
over K frames in one pass.

Reference (float64, tests/psd_ref.py): the complex64 samples times the float32 window in double,
numpy.fft.fft, |.|^2, the sum over the K frames of a vector, times scale. Bound per bin (tests 3, 4):
  B[k] = scale [sum_f (2 |X_f[k]| d_f + d_f^2) + g sum_f |X_f[k]|^2]
with d_f = 1e-5 max_k |X_f[k]| (the project's per-frame FFT bound, oracle.tol_ok) and g = (K + 2) 2^-24
(one rounding per addition in the worst chain, plus the squaring and the scale).

The test signal is complex Gaussian noise plus two tones, one at a bin centre and one off it, whose
peak bins stand 40 dB above the rms noise bin of the windowed spectrum (amplitude 100 sqrt(0.375 N) /
(N / 2) for unit noise under a Hann window): d_f / |X_f[k]| is then about 1e-3 for a noise bin
whatever N, and B / ref exceeds 0.1 only where K chi-square draws all fall very low
(test_db_routes_on_the_cpu counts those bins from the float64 reference alone).

Worst ratios printed by test 3 on one MI355X (err / B; the same for scipy's fp32 FFT followed by numpy
fp32 squares and sums): see DESIGN.md section 4.9."""
import ctypes as C

import numpy as np
import pytest

from newsched_amd import nsh
from tests.gpu_util import bits, dev, hann, rand_window
from tests.psd_ref import P_DEFAULT, balanced_segment, fft_of, frames_per_team, reference, run, segment, signal


def yardstick(x, N, K, w, scale, shift):
    """A good fp32 chain: scipy's complex64 FFT, then numpy fp32 squares, sum and scale."""
    import scipy.fft as sf

    f = np.ascontiguousarray(x, np.complex64).reshape(-1, N)
    if w is not None:
        f = f * np.asarray(w, np.float32)[None, :]
    y = sf.fft(f, axis=1)
    assert y.dtype == np.complex64
    p = (y.real * y.real + y.imag * y.imag).reshape(-1, K, N).sum(axis=1, dtype=np.float32) * np.float32(scale)
    return np.fft.fftshift(p, axes=1) if shift else p


gpu = pytest.mark.gpu
SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]


# ---- 1. the transform of fft_vcc --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", SIZES)
def test_same_transform_as_the_fft_plan(torch_cuda, N):
    """K = 1, scale 1, linear: every bin equals |Y|^2 of the forward nsh_fft_c2c plan's output Y
    (computed in float64) to 2^-22 relative -- two squarings and one addition, fused or not -- and a
    bin where Y is exactly 0 is exactly 0. Pins the bin order, the shift, the window and the LIN path."""
    torch = torch_cuda
    for w in (None, rand_window(N)):
        for shift in (False, True):
            plan = nsh.PsdPlan(N, 1, w, shift, 1.0)
            nvec = 2 * plan.tile + 3
            x = signal(N, nvec, 2)
            Y = fft_of(torch, x, N, w, shift).astype(np.complex128).reshape(nvec, N)
            want = Y.real * Y.real + Y.imag * Y.imag
            out = run(torch, plan, x).astype(np.float64)
            assert np.all(out[want == 0] == 0)
            assert np.all(np.abs(out - want) <= 2.0 ** -22 * want), (plan.kernel, shift, w is None)
            plan.close()


# ---- 2. accumulation, bit for bit -------------------------------------------------------------
def k_values(N, P):
    F = frames_per_team(N)
    return sorted({k for k in (1, 2, 3, F - 1, F, F + 1, P - 1, P, P + 1, 2 * P + 3) if 1 <= k <= 65536})


def integers(nframes, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-15, 16, nframes) + 1j * rng.integers(-15, 16, nframes)).astype(np.complex64)


@gpu
@pytest.mark.parametrize("N", [16, 128, 256, 1024, 2048, 8192])
def test_impulse_frames_accumulate_exactly(torch_cuda, N):
    """Frames that are an impulse of integer amplitude at sample 0 transform to X_f[k] = x_f[0] for
    every k exactly (asserted on nsh_fft_c2c first): with a power-of-two scale every output is
    scale * sum |x_f[0]|^2 bit for bit, whatever the order of the additions, at K around the frames of
    a team and around the segment, for 1, 2 and 5 vectors."""
    torch = torch_cuda
    P = segment(N)
    ks = k_values(N, P)
    c = integers(5 * max(ks), 7 + N)
    x = np.zeros((c.size, N), np.complex64)
    x[:, 0] = c
    x = x.ravel()
    Y = fft_of(torch, x, N).reshape(-1, N)
    assert np.all(Y == c[:, None]), "precondition: the transform of an impulse at 0 is exact"
    scale = 0.25
    p = (c.real.astype(np.float64) ** 2 + c.imag.astype(np.float64) ** 2)
    for K in ks:
        plan = nsh.PsdPlan(N, K, None, False, scale)
        assert plan.segment == balanced_segment(K, P)
        for nvec in (1, 2, 5):
            out = run(torch, plan, x[:nvec * K * N])
            want = (scale * p[:nvec * K].reshape(nvec, K).sum(axis=1)).astype(np.float32)
            assert np.array_equal(bits(out, np.float32), bits(np.repeat(want[:, None], N, axis=1), np.float32)), (plan.kernel, K, nvec)
        plan.close()


@gpu
@pytest.mark.parametrize("N", [64, 512, 1024, 4096])
def test_dc_frames_land_in_one_bin(torch_cuda, N):
    """DC frames x_f[n] = c_f: all power in bin 0 (bin N/2 of a shifted plan), exactly N^2 scale
    sum |c_f|^2, every other bin exactly 0 -- at one K within a segment and one beyond. The
    precondition (nsh_fft_c2c gives N c_f in bin 0 and exact zeros elsewhere) is asserted first: it
    holds at all four sizes, one per path (LIN, two frames a wave, one frame a wave, one frame a
    workgroup), so none is left out."""
    torch = torch_cuda
    P = segment(N)
    c = integers(3 * (P + 3), 9 + N)
    x = np.repeat(c[:, None], N, axis=1).ravel()
    Y = fft_of(torch, x, N).reshape(-1, N)
    assert np.all(Y[:, 0] == np.complex64(N) * c) and np.all(Y[:, 1:] == 0), "precondition: the transform of DC is exact"
    p = (c.real.astype(np.float64) ** 2 + c.imag.astype(np.float64) ** 2) * N * N
    scale = 2.0 ** -10
    for K in (3, P + 3):
        for shift in (False, True):
            plan = nsh.PsdPlan(N, K, None, shift, scale)
            out = run(torch, plan, x[:3 * K * N])
            want = np.zeros((3, N), np.float32)
            want[:, N // 2 if shift else 0] = scale * p[:3 * K].reshape(3, K).sum(axis=1)
            assert np.array_equal(bits(out, np.float32), bits(want, np.float32)), (plan.kernel, K, shift)
            plan.close()


# ---- 3. against float64 on noise --------------------------------------------------------------
NOISE_SIZES = [16, 64, 128, 256, 1024, 2048, 8192]


@gpu
@pytest.mark.parametrize("N", NOISE_SIZES)
def test_noise_and_tones_within_the_bound(torch_cuda, N):
    """Hann window, K in {1, 7, P + 1}, 3 vectors, scale 1/K: |out - ref| <= B per bin. Prints the
    worst err / B beside the same ratio of the fp32 yardstick (reported, never asserted)."""
    torch = torch_cuda
    P = segment(N)
    w = hann(N)
    for K in (1, 7, P + 1):
        for shift in (False, True):
            x = signal(N, 3 * (P + 1))[:3 * K * N]
            plan = nsh.PsdPlan(N, K, w, shift)
            out = run(torch, plan, x).astype(np.float64)
            ref, B = reference(x, N, K, w, 1.0 / K, shift)
            ratio = np.max(np.abs(out - ref) / B)
            yard = np.max(np.abs(yardstick(x, N, K, w, 1.0 / K, shift).astype(np.float64) - ref) / B)
            print("3/noise N=%d K=%d shift=%d %s: worst err/B %.3g (fp32 yardstick %.3g)" % (N, K, shift, plan.kernel, ratio, yard))
            assert ratio <= 1.0, (plan.kernel, K, shift, ratio)
            plan.close()


# ---- 4. dB ------------------------------------------------------------------------------------
def db_check(out, ref, B):
    """Bins with B / ref <= 0.1 by |d| <= (10 / ln 10) q / (1 - q) + 8 2^-24 max(|dB|, 1), the rest in
    the linear domain through 10^(out / 10) with bound 2 B. Returns (ok, fraction on the second route)."""
    out = np.asarray(out, np.float64)
    q = B / ref
    first = q <= 0.1
    dref = 10 * np.log10(ref)
    qq = np.where(first, q, 0.0)
    ok1 = np.abs(out - dref) <= 10 / np.log(10) * qq / (1 - qq) + 8 * 2.0 ** -24 * np.maximum(np.abs(dref), 1)
    ok2 = np.abs(10 ** (out / 10) - ref) <= 2 * B
    return bool(np.all(np.where(first, ok1, ok2))), float(np.mean(~first))


def db_input(N, K):
    return signal(N, 3 * (P_DEFAULT + 1), 3)[:3 * K * N]


@pytest.mark.parametrize("N", NOISE_SIZES)
def test_db_routes_on_the_cpu(N):
    """From the float64 reference alone: at most 1 % of the bins of test 4's inputs have
    B / ref > 0.1 (and are judged in the linear domain)."""
    for K in (7, P_DEFAULT + 1):
        ref, B = reference(db_input(N, K), N, K, hann(N), 1.0 / K)
        assert np.mean(B / ref > 0.1) <= 0.01, (N, K)


@gpu
@pytest.mark.parametrize("N", NOISE_SIZES)
def test_decibels(torch_cuda, N):
    """db = 1 at K = 7 and K = P + 1 against 10 log10 of the float64 reference; an all-zero vector
    gives -inf in every bin and leaves its neighbours' bits alone."""
    torch = torch_cuda
    P = segment(N)
    w = hann(N)
    for K in (7, P + 1):
        x = signal(N, 3 * (P + 1), 3)[:3 * K * N]  # db_input(N, K) while P is the default
        plan = nsh.PsdPlan(N, K, w, True, db=True)
        out = run(torch, plan, x)
        ref, B = reference(x, N, K, w, 1.0 / K, True)
        ok, second = db_check(out, ref, B)
        print("4/dB N=%d K=%d %s: %.2f %% of the bins judged in the linear domain" % (N, K, plan.kernel, 100 * second))
        assert second <= 0.01
        assert ok, (plan.kernel, K)
        z = np.array(x).reshape(3, K * N)
        z[1] = 0
        outz = run(torch, plan, z.ravel())
        assert np.all(np.isneginf(outz[1]))
        assert np.array_equal(bits(outz[[0, 2]], np.float32), bits(out[[0, 2]], np.float32))
        plan.close()


# ---- 5. cut invariance ------------------------------------------------------------------------
PATHS = [64, 1024, 4096]  # LIN, one frame per one-wave team, one frame per workgroup


def path_ks(P):
    return (5, P + 3)


@gpu
@pytest.mark.parametrize("N", PATHS)
def test_cut_invariance(torch_cuda, N):
    """5 vectors in one call equal, bit for bit, the same vectors in calls of 2 + 3, in 5 single
    calls, under a grid cap of 2, and with the input at an odd 8-byte sample offset and the output at
    an odd float offset; K within a segment and beyond."""
    torch = torch_cuda
    P = segment(N)
    w = hann(N)
    for K in path_ks(P):
        x = signal(N, 5 * (P + 3), 4)[:5 * K * N]
        plan = nsh.PsdPlan(N, K, w, True)
        V = K * N
        whole = run(torch, plan, x)
        parts = np.concatenate([run(torch, plan, x[:2 * V]), run(torch, plan, x[2 * V:])])
        singles = np.concatenate([run(torch, plan, x[j * V:(j + 1) * V]) for j in range(5)])
        assert np.array_equal(bits(whole, np.float32), bits(parts, np.float32)), (plan.kernel, K)
        assert np.array_equal(bits(whole, np.float32), bits(singles, np.float32)), (plan.kernel, K)
        plan.grid_cap(2)
        assert np.array_equal(bits(whole, np.float32), bits(run(torch, plan, x), np.float32)), (plan.kernel, K)
        plan.grid_cap(0)
        assert np.array_equal(bits(whole, np.float32), bits(run(torch, plan, x, in_off=1, out_off=1), np.float32)), (plan.kernel, K)
        assert np.array_equal(bits(whole, np.float32), bits(run(torch, plan, x, in_off=3, out_off=7), np.float32)), (plan.kernel, K)
        plan.close()


# ---- 6. buffer ends ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", PATHS)
def test_more_rows_than_the_scratch_holds(torch_cuda, N, monkeypatch):
    """K > P with scratch for two vectors only: a call of 7 vectors runs in batches and equals the
    same vectors in single calls on a plan with the default scratch, bit for bit. (run() checks the
    guard floats around out and lets the input end exactly at the end of its allocation, where the
    prefetch one step past the end must read nothing, in every test of this file.)"""
    torch = torch_cuda
    P = segment(N)
    K = 2 * P + 1
    x = signal(N, 7 * K, 5)
    big = nsh.PsdPlan(N, K)
    monkeypatch.setenv("NSH_PSD_SCRATCH_BYTES", str(2 * 3 * N * 4))
    small = nsh.PsdPlan(N, K)
    monkeypatch.delenv("NSH_PSD_SCRATCH_BYTES")
    V = K * N
    singles = np.concatenate([run(torch, big, x[j * V:(j + 1) * V]) for j in range(7)])
    assert np.array_equal(bits(run(torch, small, x), np.float32), bits(singles, np.float32)), small.kernel
    assert np.array_equal(bits(run(torch, big, x), np.float32), bits(singles, np.float32)), big.kernel
    small.close()
    big.close()


@gpu
def test_refuses_byte_counts_that_overflow(torch_cuda):
    torch = torch_cuda
    plan = nsh.PsdPlan(8192, 65536)
    a = torch.zeros(16, device="cuda")
    b = torch.zeros(16, device="cuda")
    with pytest.raises(nsh.NshError, match="nvec too large"):
        plan(a, b, 1 << 62)
    plan.close()


# ---- 7. non-finite samples --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", PATHS)
def test_nonfinite_samples_stay_in_their_vector(torch_cuda, N):
    """One NaN, and one inf, in a frame in the middle of vector 1 of 3: all N outputs of vector 1 are
    non-finite, vectors 0 and 2 bit-identical to the clean run; K within a segment and beyond."""
    torch = torch_cuda
    P = segment(N)
    for K in path_ks(P):
        x = signal(N, 3 * (P + 3), 6)[:3 * K * N]
        plan = nsh.PsdPlan(N, K, hann(N))
        clean = run(torch, plan, x)
        assert np.all(np.isfinite(clean))
        for bad in (np.nan, np.inf):
            z = np.array(x)
            z[(K + K // 2) * N + N // 3] = complex(1.0, bad)
            out = run(torch, plan, z)
            assert not np.any(np.isfinite(out[1])), (plan.kernel, K, bad)
            assert np.array_equal(bits(out[[0, 2]], np.float32), bits(clean[[0, 2]], np.float32)), (plan.kernel, K, bad)
        plan.close()


# ---- 8. the timing pair -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", [(64, 4), (1024, 40), (4096, 1)])
def test_psd_takes_the_armed_timing_pair(torch_cuda, N, K):
    """An armed nsh_time_next_launch pair is taken by one call of nsh_psd_cf: its start by the first
    launch and its stop by the last (nsh_timed_launches grows by the launches that recorded: 1 within a
    segment, 2 beyond), positive elapsed time; a call with nvec = 0 launches nothing and drops the pair,
    so the next, unarmed call is not timed."""
    torch = torch_cuda
    L = nsh.lib()

    def count():
        c = C.c_uint64()
        assert L.nsh_timed_launches(C.byref(c)) == 0
        return c.value

    def events():
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            assert L.nsh_event_create(C.byref(e)) == 0
        return ev

    p = nsh.PsdPlan(N, K)
    nvec = max((1 << 18) // (N * K), 1)
    x = dev(torch, signal(N, nvec * K, 8))
    y = torch.empty(nvec * N, dtype=torch.float32, device="cuda")
    ev = events()
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, y, nvec)
    assert count() == c0 + (1 if K <= segment(N) else 2)
    c1 = count()
    p(x, y, nvec)  # unarmed: not counted
    assert count() == c1
    torch.cuda.synchronize()
    ms = C.c_float()
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) == 0 and ms.value > 0
    for e in ev:
        L.nsh_event_destroy(e)
    ev = events()
    c0 = count()
    assert L.nsh_time_next_launch(ev[0], ev[1]) == 0
    p(x, y, 0)     # nothing to do: no launch, the pair is dropped on return
    p(x, y, nvec)  # unarmed
    torch.cuda.synchronize()
    assert count() == c0
    assert L.nsh_event_elapsed_ms(ev[0], ev[1], C.byref(ms)) != 0  # never recorded
    for e in ev:
        L.nsh_event_destroy(e)
    p.close()
